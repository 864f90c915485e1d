"""LAS ingest without laspy: disk -> HBM, SURVEY §8f row f4.

`read_las(path, device)` mirrors baseline/datasets/laserlane_proposals.py:618-636 (`[N,4]` = x, y, z, intensity clipped to
[800, 33000] and normalised (i - 800) / 33000); `read_las_raw` keeps the raw intensity, which is what the rasteriser
(`ops.bev_raster_batch`) takes.  The public header block is parsed on the host (`lm_las_parse_header`); the point records
go to the GPU as raw bytes and are decoded there (`lm_las_decode_points`), straight into the `[N,4]` float32 layout of the
hot path.  Differences from the reference, both deliberate: float32 instead of float64 (the hot path is fp32; pass
`shift=las_read_offset` of the tile's parameter file so that metre-scale coordinates keep millimetre precision), and no
`exit()` on clouds with fewer than 5 points (a ValueError instead).

`select=PointFilter(...)` on any reader keeps only the records that pass a predicate on their classification, flag bits, return numbers
and decoded height (`lm_las_decode_select`: decode, select and stable compaction on the GPU, file order kept), e.g. to keep noise,
withheld points and gantry signs out of the rasteriser, which takes the brightest return of a pixel.

`GroundFilter` / `ground_datum` describe how the map routes follow the terrain: a per-tile elevation datum and a height-above-ground
selection, both from the ground model the GPU computes out of the binned points (`ops.tile_ground`, `ops.ground_select`).

`IntensityStretch` / `intensity_window` describe how the map routes fit the rasteriser's intensity window to the data: two percentiles of
the intensities a tile, or the whole strip, keeps (`ops.tile_intensity_window`), stretched over the intensity channel.

`GapFill` / `gap_radius` describe how the map routes close the holes between the returns of a sparse scanner in the rasterised tiles
(`ops.tile_gap_hist`, `ops.tile_gap_fill`).

`MarkingLabels` / `line_segments` / `label_las` are the way back: the returns of a file labelled by the lane lines found in it
(`ops.line_index`, `ops.label_points`, `lm_las_label_records`), and the file written again with the markings classified.

`MarkingSurvey` / `line_stations` / `survey_las` / `marking_summary` profile the lines from the same returns: per station bin along every
line the count, intensity and lateral spread of its returns (`ops.line_profile`, `lm_las_line_profile_records`), and on the host the paint
runs, dash pattern, width and brightness read off the bins.

`MarkingColour` / `rgb_offset` / `survey_colour_las` / `marking_colours` add the colour of a marking, white or yellow, from the R, G, B
triple that point formats 2, 3, 5, 7, 8 and 10 carry per return: the same pass over the records fills a second table per station bin
(`lm_las_line_colour_records`), and the host reads a colour per line and per paint run off it.

`CrossSection` / `cross_files` / `cross_summary` / `snap_lines` take cross-sections along the lines: per station bin a row of lateral cells
holding the count, the paint count, the summed intensity and the summed height of every return of the band (`ops.line_cross`,
`lm_las_line_cross_records`), and on the host the stripes of every station - single or double line, a width and a paint centre read off
the distribution, the road's cross-fall - and the lines moved onto their paint.

`PaintResidue` / `residue_files` / `residue_summary` inventory the paint that no line explains - stop bars, crossing bars, arrows,
hatching, a line the network missed: the bright road-level returns away from every line, gridded, labelled into connected blobs and
described on the GPU (`ops.paint_residue`), and on the host the centre, size, fill and heading of every blob against its nearest line.

`PaintThreshold` / `hist_files` / `paint_threshold` (lanemapping_amd/threshold.py, reached from here by name) find the intensity
threshold between asphalt and paint that the four stages above need, from the returns on the lines against the returns beside them;
min_intensity='auto' / paint_intensity='auto' ask the map routes for it.

`StripStream` / `LasChunks` / `tile_groups` (lanemapping_amd/las_stream.py, reached from here by name) map a strip that does not fit in
memory: the files read in chunks of records, counted and then scattered into groups of tiles (`ops.StripBinner`), and the record passes
above fed chunk by chunk (`chunk_records=`).
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from ._lib import lib, check, LmLasHeader, LmLasSelect, LanemapHipError

INTEN_MIN, INTEN_MAX = 800.0, 33000.0
DROP_SYNTHETIC, DROP_KEYPOINT, DROP_WITHHELD, DROP_OVERLAP = 1, 2, 4, 8          # LM_LAS_DROP_* (include/lanemap_hip.h)
RETURNS = {'all': 0, 'first': 1, 'last': 2, 'single': 3}                         # LM_LAS_RETURNS_*


def _number(v):
    """A Python or numpy number, no bool: what an option that is a length, a ratio or an intensity takes."""
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def _whole(v):
    """A Python or numpy integer, no bool: what an option that is a count takes."""
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


_THRESHOLD = ('PaintThreshold', 'hist_records', 'hist_files', 'paint_threshold', 'KS_COEFF', 'HIST_BIN')
_STREAM = ('StripStream', 'LasChunks', 'tile_groups')


def __getattr__(name):
    """las_io.PaintThreshold, .hist_records, .hist_files, .paint_threshold, .KS_COEFF, .HIST_BIN: the names of
    lanemapping_amd/threshold.py, which is built on this module and so cannot be imported at its top."""
    if name in _THRESHOLD:
        from . import threshold
        return getattr(threshold, name)
    if name in _STREAM:                     # lanemapping_amd/las_stream.py, built on this module in the same way
        from . import las_stream
        return getattr(las_stream, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')


AUTO = 'auto'                       # min_intensity / paint_intensity: "the strip's own threshold" (PaintThreshold, paint_threshold)


def _is_auto(v):
    return isinstance(v, str) and v == AUTO


def _resolved(who, options, name):
    """-> options.<name>, refused where it still is 'auto': only the map routes, which run the threshold pass, resolve it."""
    v = getattr(options, name)
    if _is_auto(v):
        raise ValueError(f"{who}: {type(options).__name__}.{name}='auto' is not resolved; the map routes (infer_las_*_to_map) replace it by "
                         f"the threshold of las_io.paint_threshold, here pass that number")
    return v


class _Options:
    """What the option classes of this module share: a value that cannot be changed, compared, hashed and printed by the __slots__ of its
    class, in their order.  A class validates its arguments in __init__ and stores them with _set."""
    __slots__ = ()

    def _set(self, **values):
        for k, v in values.items():
            object.__setattr__(self, k, v)

    def _replace(self, **changes):
        """A copy with some arguments changed, validated again (for the classes whose __slots__ are their constructor's arguments)."""
        return type(self)(**{**{k: getattr(self, k) for k in self.__slots__}, **changes})

    def __setattr__(self, name, value):
        raise AttributeError(f'{type(self).__name__} is immutable')

    def __delattr__(self, name):
        raise AttributeError(f'{type(self).__name__} is immutable')

    def __repr__(self):
        return type(self).__name__ + '(' + ', '.join(f'{k}={getattr(self, k)!r}' for k in self.__slots__) + ')'

    def __eq__(self, other):
        return type(other) is type(self) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, k) for k in self.__slots__))


class PointFilter(_Options):
    """Which point records a reader keeps (immutable).  A record is kept when all of these hold:

      classes        its classification is one of `classes` (values 0..255; None: every class)
      drop_withheld, drop_synthetic, drop_keypoint, drop_overlap
                     it carries none of the flags asked to be dropped.  Point formats 0-5 have no overlap bit (overlap is class 12
                     there): drop_overlap drops nothing in such a file
      returns        'all'; 'first': return number == 1; 'last': return number == number of returns; 'single': number of returns == 1
      z_range        (lo, hi): lo <= z <= hi on the float32 z the reader returns, i.e. AFTER `shift`; None or infinite bounds: no limit
    """
    __slots__ = ('classes', 'drop_withheld', 'drop_synthetic', 'drop_keypoint', 'drop_overlap', 'returns', 'z_range')

    def __init__(self, classes=None, drop_withheld=True, drop_synthetic=False, drop_keypoint=False, drop_overlap=False, returns='all',
                 z_range=None):
        if classes is not None:
            classes = tuple(sorted({int(c) for c in classes}))
            bad = [c for c in classes if not 0 <= c <= 255]
            if bad:
                raise ValueError(f'PointFilter: classes must lie in 0..255, got {bad}')
        if returns not in RETURNS:
            raise ValueError(f'PointFilter: returns={returns!r} is none of {sorted(RETURNS)}')
        if z_range is not None:
            lo, hi = (float(v) for v in z_range)
            if math.isnan(lo) or math.isnan(hi):
                raise ValueError(f'PointFilter: z_range={z_range!r} has a NaN bound')
            if lo > hi:
                raise ValueError(f'PointFilter: z_range={z_range!r} is empty (lo > hi)')
            z_range = (lo, hi)
        self._set(classes=classes, drop_withheld=bool(drop_withheld), drop_synthetic=bool(drop_synthetic), drop_keypoint=bool(drop_keypoint),
                  drop_overlap=bool(drop_overlap), returns=returns, z_range=z_range)

    def for_format(self, point_format):
        """-> self, after checking the filter against a file's point data record format: formats 0-5 store the classification in five
        bits, so a class above 31 cannot occur there and asking for one is refused."""
        if not 0 <= int(point_format) <= 10:
            raise ValueError(f'PointFilter: unknown point data record format {point_format}')
        if self.classes is not None and int(point_format) <= 5:
            bad = [c for c in self.classes if c > 31]
            if bad:
                raise ValueError(f'PointFilter: classes {bad} do not exist in point format {point_format} (formats 0-5 hold 0..31)')
        return self

    def as_struct(self):
        """-> the LmLasSelect of include/lanemap_hip.h."""
        s = LmLasSelect()
        for w in range(8):
            s.class_mask[w] = 0xFFFFFFFF if self.classes is None else sum(1 << (c & 31) for c in self.classes if c >> 5 == w)
        s.drop_flags = (DROP_SYNTHETIC * self.drop_synthetic | DROP_KEYPOINT * self.drop_keypoint | DROP_WITHHELD * self.drop_withheld |
                        DROP_OVERLAP * self.drop_overlap)
        s.returns = RETURNS[self.returns]
        s.z_lo, s.z_hi = (-math.inf, math.inf) if self.z_range is None else self.z_range
        return s


class GroundFilter(_Options):
    """How the LAS -> map routes follow the terrain (immutable; Runner.infer_las_strip_to_map / infer_las_to_map, `ground=`).  Both parts
    rest on the per-tile ground model of ops.tile_ground: cells of cell_px x cell_px pixels, each the lower median over its 3 x 3
    neighbourhood of the cells' smallest tile-frame heights.

      height_range   (lo, hi): only points with lo <= height above the ground of their cell <= hi reach the rasteriser
                     (ops.ground_select); None or infinite bounds: no limit.  The ground of a cell is a MINIMUM over the cell: on a slope
                     it lies below the surface by up to cell size x (|dz/dx| + |dz/dy|), 0.16 m for 1.6 m cells on 5 % + 5 %; `lo` must
                     allow for it (and for the noise of the lowest return), e.g. (-0.5, 1.0) for road paint
      cell_px        8 .. 128 pixels per cell (default 32: 1.6 m at 0.05 m per pixel)
      datum          True: every tile's local_min_ele becomes ground_datum(its ground_min, ele_reso, datum_margin), so that the elevation
                     channel G = round((z - local_min_ele) / ele_reso) starts datum_margin below the tile's own ground instead of at one
                     value per strip; a tile without points keeps the local_min_ele it came with
      datum_margin   metres (>= 0) between the datum and the tile's lowest ground cell
    """
    __slots__ = ('height_range', 'cell_px', 'datum', 'datum_margin')

    def __init__(self, height_range=None, cell_px=32, datum=True, datum_margin=1.0):
        if height_range is not None:
            lo, hi = (float(v) for v in height_range)
            if math.isnan(lo) or math.isnan(hi):
                raise ValueError(f'GroundFilter: height_range={height_range!r} has a NaN bound')
            if lo > hi:
                raise ValueError(f'GroundFilter: height_range={height_range!r} is empty (lo > hi)')
            height_range = (lo, hi)
        if isinstance(cell_px, bool) or int(cell_px) != cell_px or not 8 <= int(cell_px) <= 128:
            raise ValueError(f'GroundFilter: cell_px={cell_px!r} must be a whole number of pixels in 8..128')
        margin = float(datum_margin)
        if not (margin >= 0.0 and math.isfinite(margin)):
            raise ValueError(f'GroundFilter: datum_margin={datum_margin!r} must be a finite number >= 0')
        self._set(height_range=height_range, cell_px=int(cell_px), datum=bool(datum), datum_margin=margin)


def ground_datum(ground_min, ele_reso, margin, fallback):
    """The elevation datum of a tile from its lowest ground cell: floor((ground_min - margin) / ele_reso) * ele_reso in float64, a whole
    number of elevation steps so that G of a point at the datum is exactly 0; `fallback` for ground_min = +inf (a tile without points)."""
    g = float(ground_min)
    if math.isnan(g) or g == -math.inf:
        raise ValueError(f'ground_datum: ground_min={ground_min!r} is neither finite nor +inf')
    if g == math.inf:
        return float(fallback)
    return math.floor((g - float(margin)) / float(ele_reso)) * float(ele_reso)


class IntensityStretch(_Options):
    """How the LAS -> map routes choose the rasteriser's intensity window (immutable; Runner.infer_las_strip_to_map / infer_las_to_map,
    `intensity=`).  The window is read off the data: two percentiles of the intensities of the points a tile keeps
    (ops.tile_intensity_window), stretched so that the upper one lands on `white` (intensity_window below).

      percentiles   (lo, hi) in percent, 0 <= lo <= hi <= 100, resolved to parts per million
      scope         'tile': every tile its own window, from the point ranges the rasteriser will see; 'strip': one window for all tiles of
                    the call, from all binned ranges before the batch loop (infer_las_strip_to_map only)
      white         the level (0 < white <= 255) the upper percentile maps to; the reference's own window puts 33000 at
                    255 * 32200 / 33000 = 248.8
      min_span      the window is at least this many intensity steps wide (> 0): a featureless tile is not amplified into noise
      min_points    a tile or strip with fewer counted points keeps the `fallback` window and the reference's rule
      fallback      (inten_lo, inten_hi) of that case: the constants of the reference's read_las
    min_span and min_points are plain defaults, not tuned values."""
    __slots__ = ('percentiles', 'scope', 'white', 'min_span', 'min_points', 'fallback')

    def __init__(self, percentiles=(1.0, 99.9), scope='tile', white=249, min_span=16, min_points=1024, fallback=(800.0, 33000.0)):
        try:
            lo, hi = (float(v) for v in percentiles)
        except (TypeError, ValueError):
            raise ValueError(f'IntensityStretch: percentiles={percentiles!r} must be a pair of numbers') from None
        if not (0.0 <= lo <= hi <= 100.0):
            raise ValueError(f'IntensityStretch: percentiles={percentiles!r} must satisfy 0 <= lo <= hi <= 100')
        if scope not in ('tile', 'strip'):
            raise ValueError(f"IntensityStretch: scope={scope!r} must be 'tile' or 'strip'")
        if isinstance(white, bool) or not (0.0 < float(white) <= 255.0):
            raise ValueError(f'IntensityStretch: white={white!r} must be a level in (0, 255]')
        if isinstance(min_span, bool) or not (0.0 < float(min_span) < math.inf):
            raise ValueError(f'IntensityStretch: min_span={min_span!r} must be a finite number > 0')
        if isinstance(min_points, bool) or int(min_points) != min_points or int(min_points) < 0:
            raise ValueError(f'IntensityStretch: min_points={min_points!r} must be a whole number >= 0')
        try:
            f_lo, f_hi = (float(v) for v in fallback)
        except (TypeError, ValueError):
            raise ValueError(f'IntensityStretch: fallback={fallback!r} must be a pair of numbers') from None
        if not (f_lo < f_hi < math.inf and f_hi > 0.0 and f_lo > -math.inf):
            raise ValueError(f'IntensityStretch: fallback={fallback!r} must be a finite window lo < hi with hi > 0')
        self._set(percentiles=(lo, hi), scope=scope, white=float(white), min_span=float(min_span), min_points=int(min_points),
                  fallback=(f_lo, f_hi))


def intensity_window(lo_key, hi_key, count, stretch):
    """The rasteriser's intensity window from the two percentile keys and the count of ops.tile_intensity_window: -> (inten_lo, inten_hi,
    scale).  count < stretch.min_points (or no point at all): the fallback window with scale None, i.e. the reference's rule
    I = round(255 (clip(i) - lo) / hi).  Otherwise lo = lo_key, hi = max(hi_key, lo + min_span), scale = white / (hi - lo):
    I = clamp(floor((clip(i, lo, hi) - lo) * scale + .5), 1, 255) puts the upper percentile at `white`."""
    if not isinstance(stretch, IntensityStretch):
        raise TypeError(f'intensity_window: stretch must be a las_io.IntensityStretch, not {type(stretch).__name__}')
    lo_key, hi_key, count = int(lo_key), int(hi_key), int(count)
    if count < stretch.min_points or count <= 0:
        return stretch.fallback[0], stretch.fallback[1], None
    if not 0 <= lo_key <= hi_key <= 65535:
        raise ValueError(f'intensity_window: keys ({lo_key}, {hi_key}) of {count} points are not 0 <= lo <= hi <= 65535')
    lo = float(lo_key)
    hi = max(float(hi_key), lo + stretch.min_span)
    return lo, hi, stretch.white / (hi - lo)


class ElevationDrape(_Options):
    """How the LAS -> map routes give their 3-D lane vertices a height (immutable; Runner.infer_las_strip_to_map / infer_las_to_map,
    `elevation=`).  The height of a vertex is read off the points the rasteriser saw (ops.drape_vertices): the lower median, over the
    (2 radius_px + 1)^2 pixels around the vertex pixel, of each pixel's smallest tile-frame height - instead of the 8-bit elevation of the
    brightest return in the vertex pixel.

      radius_px    0 .. 8: half the window side in pixels (default 4: 0.45 m x 0.45 m at 0.05 m per pixel)
      min_pixels   a vertex with fewer non-empty window pixels (>= 1) falls back to the elevation channel of the tile, as without the
                   argument
      fit          'line': every line's heights are replaced by their least-squares line over the vertex index, as the reference does;
                   'none': the heights stay as read, so a crest, dip or ramp inside a tile keeps its shape
    min_pixels is a plain default, not a tuned value."""
    __slots__ = ('radius_px', 'min_pixels', 'fit')

    def __init__(self, radius_px=4, min_pixels=5, fit='line'):
        if isinstance(radius_px, bool) or int(radius_px) != radius_px or not 0 <= int(radius_px) <= 8:
            raise ValueError(f'ElevationDrape: radius_px={radius_px!r} must be a whole number of pixels in 0..8')
        if isinstance(min_pixels, bool) or int(min_pixels) != min_pixels or int(min_pixels) < 1:
            raise ValueError(f'ElevationDrape: min_pixels={min_pixels!r} must be a whole number >= 1')
        if fit not in ('line', 'none'):
            raise ValueError(f"ElevationDrape: fit={fit!r} must be 'line' or 'none'")
        self._set(radius_px=int(radius_px), min_pixels=int(min_pixels), fit=fit)


class GapFill(_Options):
    """How the LAS -> map routes close the holes between the returns of a scanner that delivers fewer returns than pixels (immutable;
    Runner.infer_las_strip_to_map / infer_las_to_map, `density=`).  Between the rasteriser and the network every empty pixel of a tile
    takes the three bytes of the nearest non-empty pixel of the same tile within a disc of `radius` pixels, ties in distance going to the
    brightest, then highest (ops.tile_gap_fill); pixels further away stay empty.

      radius_px      'auto': per tile, the smallest radius that makes `coverage` of the tile's near pixels non-empty (gap_radius, from
                     ops.tile_gap_hist); or a whole number in 0..max_radius_px used for every tile (0: the tile is not changed)
      max_radius_px  1 .. 8: the largest radius 'auto' may choose; pixels further than this from every return are the black area beside
                     the swath and do not count
      coverage       0 < coverage <= 1: the share of the near pixels (non-empty, or within max_radius_px of a return) to be non-empty
    coverage = 0.9 and max_radius_px = 4 are plain defaults, not tuned values."""
    __slots__ = ('radius_px', 'max_radius_px', 'coverage')

    def __init__(self, radius_px='auto', max_radius_px=4, coverage=0.9):
        if not _whole(max_radius_px) or not 1 <= int(max_radius_px) <= 8:
            raise ValueError(f'GapFill: max_radius_px={max_radius_px!r} must be a whole number of pixels in 1..8')
        if not (isinstance(radius_px, str) and radius_px == 'auto'):
            if not _whole(radius_px) or not 0 <= int(radius_px) <= int(max_radius_px):
                raise ValueError(f"GapFill: radius_px={radius_px!r} must be 'auto' or a whole number of pixels in 0..max_radius_px="
                                 f'{int(max_radius_px)}')
            radius_px = int(radius_px)
        if not _number(coverage) or not 0 < float(coverage) <= 1:
            raise ValueError(f'GapFill: coverage={coverage!r} must be a number with 0 < coverage <= 1')
        self._set(radius_px=radius_px, max_radius_px=int(max_radius_px), coverage=float(coverage))


def gap_radius(hist_row, fill):
    """The fill radius of one tile from its row of ops.tile_gap_hist (Rmax + 2 counters for Rmax = fill.max_radius_px): a fixed
    fill.radius_px as it is; 'auto': with near = sum(hist_row[0 : Rmax + 1]) - the far pixels, the black area beside the swath, left out -
    the smallest r in 0..Rmax with sum(hist_row[0 : r + 1]) * 10**6 >= round(coverage * 10**6) * near, in integers; 0 for near == 0."""
    if not isinstance(fill, GapFill):
        raise TypeError(f'gap_radius: fill must be a las_io.GapFill, not {type(fill).__name__}')
    if fill.radius_px != 'auto':
        return fill.radius_px
    row = [int(v) for v in hist_row]
    R = fill.max_radius_px
    if len(row) != R + 2 or any(v < 0 for v in row):
        raise ValueError(f'gap_radius: hist_row must hold max_radius_px + 2 = {R + 2} counters >= 0, not {row}')
    near = sum(row[0:R + 1])
    if near == 0:
        return 0
    want = int(round(fill.coverage * 10 ** 6)) * near
    for r in range(R + 1):
        if sum(row[0:r + 1]) * 10 ** 6 >= want:
            return r
    return R


class MarkingLabels(_Options):
    """How the LAS -> map routes label the returns of their input by the lines they found (immutable; Runner.infer_las_strip_to_map /
    infer_las_to_map, `label=`; label_las).  A return is labelled with line k (counted from 1 in the order of the lines) when it lies within
    half_width of the line in the plane and within z_tol of it in height, the nearest line winning (the rule: include/lanemap_hip.h).

      half_width      metres (finite, >= 0): half the width of the band around a line in which a return counts as its paint
      z_tol           metres (>= 0, may be infinite): the height band; it only keeps a carriageway from labelling the one under or over it
      min_intensity   None, the smallest raw intensity a labelled return has (paint is bright), or 'auto': the threshold the map routes
                      find in the strip's own returns (PaintThreshold)
      marking_class   the classification a labelled record gets, 0..255; None: 64 on point formats 6-10 (the first user-definable class of
                      LAS 1.4), 31 on formats 0-5 (the largest class their five bits hold)
      line_ids        True: the point source ID of a labelled record becomes its line number (at most 65535 lines)
    half_width = 0.15 and z_tol = 0.5 are plain defaults, not tuned values."""
    __slots__ = ('half_width', 'z_tol', 'min_intensity', 'marking_class', 'line_ids')

    def __init__(self, half_width=0.15, z_tol=0.5, min_intensity=None, marking_class=None, line_ids=True):
        if not _number(half_width) or not (0.0 <= float(half_width) < math.inf):
            raise ValueError(f'MarkingLabels: half_width={half_width!r} must be a finite number >= 0')
        if not _number(z_tol) or not float(z_tol) >= 0.0:
            raise ValueError(f'MarkingLabels: z_tol={z_tol!r} must be a number >= 0')
        if min_intensity is not None and not _is_auto(min_intensity):
            if not _number(min_intensity) or math.isnan(float(min_intensity)):
                raise ValueError(f"MarkingLabels: min_intensity={min_intensity!r} must be None, a number or 'auto'")
            min_intensity = float(min_intensity)
        if marking_class is not None:
            if not _whole(marking_class) or not 0 <= int(marking_class) <= 255:
                raise ValueError(f'MarkingLabels: marking_class={marking_class!r} must be None or a class in 0..255')
            marking_class = int(marking_class)
        self._set(half_width=float(half_width), z_tol=float(z_tol), min_intensity=min_intensity, marking_class=marking_class,
                  line_ids=bool(line_ids))

    def for_format(self, point_format):
        """-> the classification labelled records of a file of this point data record format get: marking_class, or its default for the
        format.  Formats 0-5 store the classification in five bits: a class above 31 asked of such a file is refused."""
        if not 0 <= int(point_format) <= 10:
            raise ValueError(f'MarkingLabels: unknown point data record format {point_format}')
        if self.marking_class is None:
            return 64 if int(point_format) >= 6 else 31
        if int(point_format) <= 5 and self.marking_class > 31:
            raise ValueError(f'MarkingLabels: marking_class={self.marking_class} does not exist in point format {point_format} '
                             '(formats 0-5 hold 0..31)')
        return self.marking_class


def line_segments(lines, shift=None):
    """Lines (a list of [n_i,3] float64 arrays in the LAS frame: what infer_las_*_to_map returns) -> the [S,8] float32 segment table of
    the labelling: per consecutive vertex pair ax, ay, az, dx, dy, dz, inv, line.  Every vertex minus `shift` in float64, rounded to
    float32; d = the float32 difference of the rounded endpoints; inv = 1 / (dx*dx + dy*dy) in float32, 0 where that is 0; line = the
    int32 bit pattern of (line index + 1).  Line order, then vertex order; a line with fewer than two vertices gives no segment."""
    sh = np.zeros(3) if shift is None else np.asarray(shift, dtype=np.float64).reshape(3)
    rows = []
    for k, line in enumerate(lines):
        v = np.asarray(line, dtype=np.float64)
        if v.size == 0:
            continue
        if v.ndim != 2 or v.shape[1] != 3:
            raise ValueError(f'line_segments: line {k} has shape {v.shape}, not [n,3]')
        if v.shape[0] < 2:
            continue
        v = (v - sh).astype(np.float32)
        a, d = v[:-1], v[1:] - v[:-1]
        len2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        inv = np.zeros_like(len2)
        np.divide(np.float32(1.0), len2, out=inv, where=len2 != 0)
        seg = np.empty((len(a), 8), dtype=np.float32)
        seg[:, 0:3], seg[:, 3:6], seg[:, 6] = a, d, inv
        seg[:, 7] = np.full(len(a), k + 1, dtype=np.int32).view(np.float32)
        rows.append(seg)
    return np.concatenate(rows) if rows else np.zeros((0, 8), dtype=np.float32)


def _d3(v):
    """Three numbers -> the double[3] the C entries take."""
    return (C.c_double * 3)(*[float(x) for x in v])


def _upload_records(data, header, device):
    """The point records of a parsed file (data: its bytes as a uint8 array, header: parse_header's dict) -> a uint8 tensor on `device`,
    zero-padded to a multiple of four bytes as the record entries take them.  The copy is asynchronous."""
    off, nbytes = header['offset_to_points'], header['n_points'] * header['record_len']
    padded = np.zeros(((nbytes + 3) // 4 * 4,), dtype=np.uint8)
    padded[:nbytes] = data[off:off + nbytes]
    return torch.from_numpy(padded).to(device, non_blocking=True)


def _records_args(who, records_u8, header, shift, select, index, stations, asker, half_width, bin=None):
    """What the record entries (label_records, profile_records, profile_colour_records, cross_records) share: the checks of select, of
    the records' device and of the tables against what the caller's options ask (`asker`: the words of the message, 'the survey asks';
    bin None: the entry takes no stations), and -> (the leading arguments of the C entry, the records' device).  The arguments: the
    current stream of the RECORDS' device, the records, record_len, point_format, n, scale, offset, shift or None, the select or None,
    index.args() and, with stations, stations.args()."""
    from . import ops
    if select is not None and not isinstance(select, PointFilter):
        raise TypeError(f'{who}: select must be a PointFilter, not {type(select).__name__}')
    if not records_u8.is_cuda:
        raise LanemapHipError(f'{who} needs the records on an MI355X (HIP) device; no CPU fallback exists')
    if bin is not None and (not isinstance(index, ops.LineIndex) or not isinstance(stations, ops.LineStations)):
        raise TypeError(f'{who}: index must be an ops.LineIndex and stations an ops.LineStations')
    fmt, rl, n = header['point_format'], header['record_len'], header['n_points']
    sel = select.for_format(fmt).as_struct() if select is not None else None
    if index.half_width != np.float32(half_width):
        raise ValueError(f'{who}: the index was built for half_width={index.half_width}, {asker} {half_width}')
    if bin is not None and (stations.bin != bin or stations.n_segments != index.n_segments):
        raise ValueError(f'{who}: the stations were cut for bin={stations.bin} and {stations.n_segments} segments, {asker} bin={bin}, '
                         f'the index holds {index.n_segments}')
    dev = records_u8.device
    return (C.c_void_p(torch._C._cuda_getCurrentRawStream(dev.index)), C.c_void_p(records_u8.data_ptr()), int(rl), int(fmt), int(n),
            _d3(header['scale']), _d3(header['offset']), _d3(shift) if shift is not None else None,
            C.byref(sel) if sel is not None else None, *index.args(), *(stations.args() if bin is not None else ())), dev


def label_records(records_u8, header, index, labels, shift=None, select=None, n_lines=None, want_line=False):
    """One lm_las_label_records call on the DEVICE records of a file (padded to a multiple of 4 bytes; `header`: parse_header's dict)
    against an ops.line_index: -> (patched records, counts [n_lines + 1] int64 device tensor[, line [n] int32]).  Asynchronous."""
    if not isinstance(labels, MarkingLabels):
        raise TypeError(f'las_io.label_records: labels must be a MarkingLabels, not {type(labels).__name__}')
    args, dev = _records_args('las_io.label_records', records_u8, header, shift, select, index, None, 'labels ask', labels.half_width)
    cls = labels.for_format(header['point_format'])
    L = index.n_lines if n_lines is None else int(n_lines)
    out = torch.empty_like(records_u8)
    counts = torch.empty((L + 1,), device=dev, dtype=torch.int64)
    line = torch.empty((header['n_points'],), device=dev, dtype=torch.int32) if want_line else None
    mi = _resolved('las_io.label_records', labels, 'min_intensity')
    mi = math.nan if mi is None else mi
    check(lib().lm_las_label_records(*args, labels.z_tol, mi, cls, int(labels.line_ids), C.c_void_p(out.data_ptr()),
                                     C.c_void_p(line.data_ptr()) if want_line else None, C.c_void_p(counts.data_ptr()), L))
    return (out, counts, line) if want_line else (out, counts)


def _label_las_chunked(path, out_path, lines, labels, shift, select, device, chunk_records):
    """label_las for a file that is never held whole: the bytes before the records, then every chunk of records relabelled (one
    lm_las_label_records call and one read-back per chunk, written as it comes back), then the bytes after them; the counts add up.  A
    label depends on its record alone, so the file is byte for byte the one the whole-file pass writes."""
    from . import ops, las_stream
    chunks = las_stream.LasChunks(path, chunk_records, device)
    h = chunks.header
    rl = h['record_len']
    labels.for_format(h['point_format'])                                  # refused before anything is uploaded
    if select is not None:
        if not isinstance(select, PointFilter):
            raise TypeError(f'las_io.label_las: select must be a PointFilter, not {type(select).__name__}')
        select.for_format(h['point_format'])
    index = ops.line_index(line_segments(lines, shift), labels.half_width, device=device)
    total = np.zeros(len(lines) + 1, dtype=np.int64)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'wb') as f:
        f.write(chunks.head_bytes)
        for rec, m, _ in chunks:
            out, counts = label_records(rec, {**h, 'n_points': m}, index, labels, shift, select, n_lines=len(lines))
            both = torch.cat([out, counts.view(torch.uint8)]).cpu().numpy()    # the chunk's one read-back
            f.write(both[:m * rl].tobytes())
            total += both[len(rec):].view(np.int64)
        f.write(chunks.tail_bytes)
    per_line = [int(c) for c in total[1:]]
    return {'records': int(h['n_points']), 'labelled': int(sum(per_line)), 'per_line': per_line}


def label_las(path, out_path, lines, labels, shift, select=None, device='cuda:0', chunk_records=None):
    """The LAS file `path` written again as `out_path` with the returns of the `lines` (list of [n,3] float64, LAS frame) classified:
    the records are uploaded, labelled in one lm_las_label_records call (the rule and what is patched: include/lanemap_hip.h) and read back
    once, together with the counts.  out_path = the input's bytes up to offset_to_points (header and VLRs), the patched records, whatever
    followed them (EVLRs).  shift: the read offset of the frame the float32 arithmetic runs in (the las_read_offset the lines were found
    with); select: the PointFilter the file was read with - a record that fails it is never relabelled.  chunk_records: None, or the
    records read, labelled and written at a time (LasChunks): the same file, never held whole.
    -> {'records': n, 'labelled': records with a label, 'per_line': [count of line 1, ...]}."""
    from . import ops
    if not isinstance(labels, MarkingLabels):
        raise TypeError(f'las_io.label_las: labels must be a MarkingLabels, not {type(labels).__name__}')
    _resolved('las_io.label_las', labels, 'min_intensity')
    device = torch.device(device)
    if chunk_records is not None:
        return _label_las_chunked(path, out_path, list(lines), labels, shift, select, device, chunk_records)
    data = np.fromfile(path, dtype=np.uint8)
    h = parse_header(data)
    n, rl, off = h['n_points'], h['record_len'], h['offset_to_points']
    labels.for_format(h['point_format'])                                  # refused before anything is uploaded
    if select is not None:
        if not isinstance(select, PointFilter):
            raise TypeError(f'las_io.label_las: select must be a PointFilter, not {type(select).__name__}')
        select.for_format(h['point_format'])
    lines = list(lines)
    index = ops.line_index(line_segments(lines, shift), labels.half_width, device=device)
    nbytes = n * rl
    rec = _upload_records(data, h, device)
    out, counts = label_records(rec, h, index, labels, shift, select, n_lines=len(lines))
    both = torch.cat([out, counts.view(torch.uint8)]).cpu().numpy()        # the one read-back
    counts = both[len(rec):].view(np.int64)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'wb') as f:
        f.write(data[:off].tobytes())
        f.write(both[:nbytes].tobytes())
        f.write(data[off + nbytes:].tobytes())
    per_line = [int(c) for c in counts[1:]]
    return {'records': int(n), 'labelled': int(sum(per_line)), 'per_line': per_line}


class MarkingSurvey(_Options):
    """How the LAS -> map routes profile the lane lines they found from the returns of their input (immutable;
    Runner.infer_las_strip_to_map / infer_las_to_map, `survey=`; survey_las, marking_summary).  The returns the labelling rule gives a line
    (within half_width in the plane and z_tol in height, the nearest line winning) are accumulated per station bin along the line (the
    rule: include/lanemap_hip.h); marking_summary then reads paint runs, width and intensity off the bins.

      bin             metres (finite, > 0): the length of a station bin along a line
      half_width      metres (finite, 0 .. 16): half the width of the band around a line whose returns are profiled
      z_tol           metres (>= 0, may be infinite): the height band
      min_intensity   None, or the smallest raw intensity a profiled return has.  WITHOUT it a bin counts returns, not paint: every bin of
                      a line over asphalt is 'painted', the width is the width of the band and the dash pattern that of the point density.
                      A threshold between asphalt and paint is needed for width, runs and type to mean anything; 'auto': the one the
                      map routes find in the strip's own returns (PaintThreshold)
      min_points      a bin counts as painted when it holds at least this many returns (whole number >= 1)
      max_gap         metres (finite, >= 0): runs of painted bins separated by at most this length of unpainted bins are joined
      solid_cover     0 < solid_cover <= 1: a line whose painted share reaches it is 'solid'
    All defaults are plain defaults, not tuned values."""
    __slots__ = ('bin', 'half_width', 'z_tol', 'min_intensity', 'min_points', 'max_gap', 'solid_cover')

    def __init__(self, bin=0.25, half_width=0.3, z_tol=0.5, min_intensity=None, min_points=3, max_gap=0.5, solid_cover=0.8):
        if not _number(bin) or not (0.0 < float(bin) < math.inf):
            raise ValueError(f'MarkingSurvey: bin={bin!r} must be a finite length > 0')
        if not _number(half_width) or not (0.0 <= float(half_width) <= 16.0):
            raise ValueError(f'MarkingSurvey: half_width={half_width!r} must be a number in 0 .. 16 (metres)')
        if not _number(z_tol) or not float(z_tol) >= 0.0:
            raise ValueError(f'MarkingSurvey: z_tol={z_tol!r} must be a number >= 0')
        if min_intensity is not None and not _is_auto(min_intensity):
            if not _number(min_intensity) or math.isnan(float(min_intensity)):
                raise ValueError(f"MarkingSurvey: min_intensity={min_intensity!r} must be None, a number or 'auto'")
            min_intensity = float(min_intensity)
        if not _whole(min_points) or int(min_points) < 1:
            raise ValueError(f'MarkingSurvey: min_points={min_points!r} must be a whole number >= 1')
        if not _number(max_gap) or not (0.0 <= float(max_gap) < math.inf):
            raise ValueError(f'MarkingSurvey: max_gap={max_gap!r} must be a finite length >= 0')
        if not _number(solid_cover) or not (0.0 < float(solid_cover) <= 1.0):
            raise ValueError(f'MarkingSurvey: solid_cover={solid_cover!r} must be a number with 0 < solid_cover <= 1')
        self._set(bin=float(bin), half_width=float(half_width), z_tol=float(z_tol), min_intensity=min_intensity, min_points=int(min_points),
                  max_gap=float(max_gap), solid_cover=float(solid_cover))


def line_stations(lines, shift=None, bin=0.25):
    """Lines (as line_segments takes them) -> (stations [S,4] float32, bin_start [L + 1] int32): the station table of the marking profile,
    its rows in exactly the order of line_segments(lines, shift), and the CSR table of the bins each of the L = len(lines) lines owns.
    Row s0, len, rlen, 0: len64 = sqrt(dx^2 + dy^2) in float64 from the float32 dx, dy of the segment row; s0 = the float64 running sum
    of the len64 of the earlier segments of the same line, rounded to float32; len = float32(len64); rlen = float32(1 / len64), 0 where
    len64 == 0.  Line k (from 1) owns the bins bin_start[k-1] .. bin_start[k] - 1: max(1, ceil(total len64 / bin)) of them for a line with
    segments, none for a line with fewer than two vertices."""
    if not _number(bin) or not (0.0 < float(bin) < math.inf):
        raise ValueError(f'line_stations: bin={bin!r} must be a finite length > 0')
    bin = float(bin)
    lines = list(lines)
    seg = line_segments(lines, shift)
    of_line = np.ascontiguousarray(seg[:, 7]).view(np.int32)
    stations = np.zeros((len(seg), 4), dtype=np.float32)
    bin_start = np.zeros(len(lines) + 1, dtype=np.int64)
    for k in range(len(lines)):
        rows = np.nonzero(of_line == k + 1)[0]                              # (consecutive, in vertex order)
        nb = 0
        if len(rows):
            d = seg[rows, 3:5].astype(np.float64)
            len64 = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
            run = np.concatenate([[0.0], np.add.accumulate(len64)])         # sequential float64 sums
            stations[rows, 0] = run[:-1].astype(np.float32)
            stations[rows, 1] = len64.astype(np.float32)
            rlen = np.zeros_like(len64)
            np.divide(1.0, len64, out=rlen, where=len64 != 0)
            stations[rows, 2] = rlen.astype(np.float32)
            nb = max(1, int(math.ceil(run[-1] / bin)))
        bin_start[k + 1] = bin_start[k] + nb
    if bin_start[-1] > 2147483647:
        raise ValueError(f'line_stations: {int(bin_start[-1])} bins of {bin} m, at most 2^31 - 1 are supported (choose a larger bin)')
    return stations, bin_start.astype(np.int32)


def profile_records(records_u8, header, index, stations, survey, shift=None, select=None, out=None):
    """One lm_las_line_profile_records call on the DEVICE records of a file (padded to a multiple of 4 bytes; `header`: parse_header's
    dict) against an ops.LineIndex and the ops.LineStations of the same segments: -> bins [n_bins, 6] int64 device tensor (see
    ops.line_profile).  The records are only read; a record `select` drops contributes nothing.  out: the bins of an earlier call to add to
    - the files of a strip go into one profile this way.  Asynchronous."""
    from . import ops
    who = 'las_io.profile_records'
    if not isinstance(survey, MarkingSurvey):
        raise TypeError(f'{who}: survey must be a MarkingSurvey, not {type(survey).__name__}')
    args, dev = _records_args(who, records_u8, header, shift, select, index, stations, 'the survey asks', survey.half_width, survey.bin)
    nb = stations.n_bins
    bins = ops._table_out(who, (nb, 6), out, dev)
    mi = _resolved(who, survey, 'min_intensity')
    mi = math.nan if mi is None else mi
    check(lib().lm_las_line_profile_records(*args, survey.z_tol, mi, int(out is not None), C.c_void_p(bins.data_ptr()) if nb else None, nb))
    return bins


def _file_chunks(path, chunk_records, device):
    """One file as the record passes take it: -> (header, an iterable of (records on the device, header of those records)).
    chunk_records None: the file is read whole and uploaded once (_upload_records); else it goes through a LasChunks of that many records,
    every chunk under the file's header with n_points = the chunk's records.  A file without records is one empty run either way."""
    if chunk_records is None:
        data = np.fromfile(path, dtype=np.uint8)
        h = parse_header(data)
        return h, ((_upload_records(data, h, device), h) for _ in range(1))
    from . import las_stream
    chunks = las_stream.LasChunks(path, chunk_records, device)
    h = chunks.header
    if h['n_points'] == 0:
        return h, ((las_stream.empty_records(device), h) for _ in range(1))
    return h, ((rec, {**h, 'n_points': m}) for rec, m, _ in chunks)


def _each_file(who, files, lines, bin, half_width, device, per_file, require=None, chunk_records=None):
    """The loop of survey_files, survey_colour_files and cross_files over `files`, a list of (path, shift, select).  Every select is
    checked and `require`, if given, is called with every path before a file is read.  Then every file is read once and uploaded once
    (_upload_records) and goes through one call per_file(records, header, tables, shift, select, out) with tables = the ops.LineIndex
    (of `half_width`) and the ops.LineStations (of `bin`) of the lines in the frame of its own shift - built once per distinct shift -
    and the result of the call before it as `out`.  The bins each line owns, bin_start, are those of the FIRST file's frame, in every table.
    -> (what the last call returned, bin_start); without a file (None, the bin_start of the unshifted lines).  Nothing is read back.
    chunk_records: None, or the records of a file read, uploaded and passed to per_file at a time (LasChunks): one call per chunk into
    the same `out` - the tables are integer sums, which do not depend on the partition."""
    from . import ops
    device = torch.device(device)
    lines, files = list(lines), list(files)
    for _, _, select in files:
        if select is not None and not isinstance(select, PointFilter):
            raise TypeError(f'{who}: select must be a PointFilter, not {type(select).__name__}')
    for path, _, _ in files if require is not None else ():
        require(path)
    tables, bin_start, out = {}, None, None
    for path, shift, select in files:
        h, runs = _file_chunks(path, chunk_records, device)
        if select is not None:
            select.for_format(h['point_format'])
        key = None if shift is None else tuple(float(v) for v in shift)
        if key not in tables:
            st, bs = line_stations(lines, shift, bin)
            bin_start = bs if bin_start is None else bin_start
            tables[key] = (ops.line_index(line_segments(lines, shift), half_width, device=device),
                           ops.line_stations(st, bin_start, bin, device=device))
        for rec, hc in runs:
            out = per_file(rec, hc, tables[key], shift, select, out)
    if out is None:
        bin_start = line_stations(lines, None, bin)[1]
    return out, bin_start


def _empty_bins(bin_start):
    """-> the [n_bins, 6] int64 numpy profile no return went into: four zeros, then the empty minimum and maximum of q."""
    host = np.zeros((int(bin_start[-1]), 6), dtype=np.int64)
    host[:, 4], host[:, 5] = 2 ** 31 - 1, -2 ** 31
    return host


def survey_files(files, lines, survey, device='cuda:0', chunk_records=None):
    """The marking profile of `lines` (list of [n,3] float64, LAS frame) from the LAS files `files`, a list of (path, shift, select): every
    file is uploaded and profiled in one lm_las_line_profile_records call with its own read offset and PointFilter, all into one bins
    tensor, which is read back once.  The bins each line owns (bin_start) are those of the first file's frame; where another file's shift
    rounds a line's length into one bin more, the rule's clamp to the line's last bin holds.  chunk_records: as for _each_file.
    -> (bins [n_bins, 6] int64 numpy, bin_start [L + 1] int32 numpy)."""
    if not isinstance(survey, MarkingSurvey):
        raise TypeError(f'las_io.survey_files: survey must be a MarkingSurvey, not {type(survey).__name__}')
    _resolved('las_io.survey_files', survey, 'min_intensity')
    bins, bin_start = _each_file('las_io.survey_files', files, lines, survey.bin, survey.half_width, device,
                                 lambda rec, h, tables, shift, select, out: profile_records(rec, h, *tables, survey, shift, select, out=out),
                                 chunk_records=chunk_records)
    if bins is None:                                                        # no file: the empty profile of the lines
        return _empty_bins(bin_start), bin_start
    return bins.cpu().numpy(), bin_start                                    # the one read-back


def survey_las(paths, lines, survey, shift, select=None, device='cuda:0'):
    """survey_files for files that share one read offset `shift` (the las_read_offset the lines were found with) and one PointFilter:
    one call per file into one bins tensor, then one read-back.  -> (bins [n_bins, 6] int64 numpy, bin_start [L + 1] int32 numpy);
    marking_summary(bins, bin_start, survey) reads the markings off them."""
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    return survey_files([(p, shift, select) for p in paths], lines, survey, device)


def marking_summary(bins, bin_start, survey):
    """The markings read off a profile (host, integers and float64): bins [n_bins, 6] int64 (n, sum iq, sum q, sum q^2, min q, max q) and
    bin_start [L + 1] -> one dict per line:

      length      metres: the line's bins times survey.bin (the last bin may reach past the line's end)
      painted     the number of painted bins; a bin counts as painted when n >= survey.min_points
      runs        [[start_m, end_m], ...]: the maximal runs of painted bins, after runs separated by at most survey.max_gap metres of
                  unpainted bins are joined
      cover       painted bins over bins (painted length over length; 0.0 for a line without bins)
      type        'solid' when cover >= survey.solid_cover; else 'dashed' with at least two runs; 'none' without a run; else 'partial'
      dash, gap   the median run length and the median length between consecutive runs, metres (None without a run / below two runs)
      width       metres: the median over the painted bins of (max q - min q) / 1024 (None without a painted bin)
      intensity   sum iq / n over the painted bins (None without a painted bin)
    Without survey.min_intensity a bin counts returns, not paint (see MarkingSurvey)."""
    if not isinstance(survey, MarkingSurvey):
        raise TypeError(f'marking_summary: survey must be a las_io.MarkingSurvey, not {type(survey).__name__}')
    bins = np.asarray(bins)
    bs = np.asarray(bin_start, dtype=np.int64)
    if bins.ndim != 2 or bins.shape[1] != 6 or bins.dtype != np.int64 or bs.ndim != 1 or len(bs) < 1 or bs[0] != 0 or (np.diff(bs) < 0).any() \
            or bs[-1] != len(bins):
        raise ValueError(f'marking_summary: bins must be [bin_start[L], 6] int64 and bin_start a CSR table from 0, not {bins.shape} '
                         f'{bins.dtype} and {bs.tolist() if len(bs) < 8 else bs.shape}')
    w = survey.bin
    gap_bins = int(math.floor(survey.max_gap / w + 1e-9))                   # the longest hole, in bins, that is joined
    out = []
    for k in range(len(bs) - 1):
        b = bins[bs[k]:bs[k + 1]]
        nb = len(b)
        on = b[:, 0] >= survey.min_points
        idx = np.nonzero(on)[0]
        runs = []
        for i in idx:
            i = int(i)
            if runs and i - runs[-1][1] - 1 <= gap_bins:
                runs[-1][1] = i
            else:
                runs.append([i, i])
        painted = int(on.sum())
        cover = painted / nb if nb else 0.0
        runs_m = [[i0 * w, (i1 + 1) * w] for i0, i1 in runs]
        gaps_m = [(runs[j + 1][0] - runs[j][1] - 1) * w for j in range(len(runs) - 1)]
        kind = 'solid' if (nb and cover >= survey.solid_cover) else 'dashed' if len(runs) >= 2 else 'none' if not runs else 'partial'
        n_sum = int(b[on, 0].sum())
        out.append({'length': nb * w, 'painted': painted, 'runs': runs_m, 'cover': cover, 'type': kind,
                    'dash': float(np.median([(i1 - i0 + 1) * w for i0, i1 in runs])) if runs else None,
                    'gap': float(np.median(gaps_m)) if gaps_m else None,
                    'width': float(np.median((b[on, 5] - b[on, 4]).astype(np.float64) / 1024.0)) if painted else None,
                    'intensity': int(b[on, 1].sum()) / n_sum if painted else None})
    return out


RGB_OFFSET = {2: 20, 3: 28, 5: 28, 7: 30, 8: 30, 10: 30}      # byte offset of the u16 LE R, G, B triple (LAS 1.4 R15, tables 10 .. 18)


def rgb_offset(point_format):
    """-> the byte offset of the 16-bit R, G, B triple in a record of this point data record format (2: 20; 3, 5: 28; 7, 8, 10: 30), or
    None for a format without colour (0, 1, 4, 6, 9)."""
    if not _whole(point_format) or not 0 <= int(point_format) <= 10:
        raise ValueError(f'rgb_offset: unknown point data record format {point_format!r}')
    return RGB_OFFSET.get(int(point_format))


class MarkingColour(_Options):
    """How the LAS -> map routes tell white markings from yellow ones (immutable; Runner.infer_las_strip_to_map / infer_las_to_map,
    `colour=` beside `survey=`; survey_colour_las, marking_colours).  The returns of a line's station bins (MarkingSurvey's rule) that
    carry a colour - any R, G, B triple but three zeros, which colourisation leaves where no camera saw the point - are counted and
    summed per bin, and each votes yellow when its blue lies below yellow_ratio of the mean of its red and green (the rule:
    include/lanemap_hip.h).

      yellow_ratio    0 < yellow_ratio <= 1: a coloured return votes yellow when B < yellow_ratio (R + G) / 2, evaluated in integers as
                      2048 B < blue_q (R + G) with blue_q = round(1024 yellow_ratio), at least 1
      yellow_share    0 < yellow_share <= 1: a line, or a paint run, is 'yellow' when at least this share of its coloured returns votes
                      yellow, else 'white'
      min_coloured    a line or run with fewer coloured returns than this is 'unknown' (whole number >= 1)
    The three defaults are plain defaults, not tuned values."""
    __slots__ = ('yellow_ratio', 'yellow_share', 'min_coloured')

    def __init__(self, yellow_ratio=0.75, yellow_share=0.5, min_coloured=10):
        if not _number(yellow_ratio) or not (0.0 < float(yellow_ratio) <= 1.0):
            raise ValueError(f'MarkingColour: yellow_ratio={yellow_ratio!r} must be a number with 0 < yellow_ratio <= 1')
        if not _number(yellow_share) or not (0.0 < float(yellow_share) <= 1.0):
            raise ValueError(f'MarkingColour: yellow_share={yellow_share!r} must be a number with 0 < yellow_share <= 1')
        if not _whole(min_coloured) or int(min_coloured) < 1:
            raise ValueError(f'MarkingColour: min_coloured={min_coloured!r} must be a whole number >= 1')
        self._set(yellow_ratio=float(yellow_ratio), yellow_share=float(yellow_share), min_coloured=int(min_coloured))

    @property
    def blue_q(self):
        """The integer lm_las_line_colour_records takes: round(1024 yellow_ratio), halves up, in 1 .. 1024."""
        return min(1024, max(1, int(math.floor(1024.0 * self.yellow_ratio + 0.5))))


def profile_colour_records(records_u8, header, index, stations, survey, colour, shift=None, select=None, out=None):
    """One lm_las_line_colour_records call on the DEVICE records of a file, as profile_records: -> (bins, colours), two [n_bins, 6] int64
    device tensors filled in one pass over the records - bins bit for bit profile_records', colours = n_c, sum R, sum G, sum B, n_yellow,
    n_black per station bin (the rule: include/lanemap_hip.h).  out: the (bins, colours) pair of an earlier call to add to.  A header
    whose point format has no colour is refused with a ValueError.  Asynchronous."""
    from . import ops
    who = 'las_io.profile_colour_records'
    if not isinstance(survey, MarkingSurvey):
        raise TypeError(f'{who}: survey must be a MarkingSurvey, not {type(survey).__name__}')
    if not isinstance(colour, MarkingColour):
        raise TypeError(f'{who}: colour must be a MarkingColour, not {type(colour).__name__}')
    args, dev = _records_args(who, records_u8, header, shift, select, index, stations, 'the survey asks', survey.half_width, survey.bin)
    fmt = header['point_format']
    if rgb_offset(fmt) is None:
        raise ValueError(f'{who}: point format {fmt} carries no RGB (formats {sorted(RGB_OFFSET)} do)')
    if out is not None and not (isinstance(out, (tuple, list)) and len(out) == 2):
        raise ValueError(f'{who}: out must be the (bins, colours) pair of an earlier call')
    nb = stations.n_bins
    bins = ops._table_out(who, (nb, 6), None if out is None else out[0], dev)
    colours = ops._table_out(who, (nb, 6), None if out is None else out[1], dev)
    mi = _resolved(who, survey, 'min_intensity')
    mi = math.nan if mi is None else mi
    check(lib().lm_las_line_colour_records(*args, survey.z_tol, mi, colour.blue_q, int(out is not None),
                                           C.c_void_p(bins.data_ptr()) if nb else None, C.c_void_p(colours.data_ptr()) if nb else None, nb))
    return bins, colours


def survey_colour_files(files, lines, survey, colour, device='cuda:0', chunk_records=None):
    """survey_files with the colour table: every file of `files`, a list of (path, shift, select), is uploaded and goes through one
    lm_las_line_colour_records call into one (bins, colours) pair, which is read back once.  All headers are read before anything is
    uploaded: a file whose point format has no colour is refused with a ValueError that names the file and its format.
    -> (bins [n_bins, 6] int64 numpy, colours [n_bins, 6] int64 numpy, bin_start [L + 1] int32 numpy)."""
    if not isinstance(survey, MarkingSurvey):
        raise TypeError(f'las_io.survey_colour_files: survey must be a MarkingSurvey, not {type(survey).__name__}')
    if not isinstance(colour, MarkingColour):
        raise TypeError(f'las_io.survey_colour_files: colour must be a MarkingColour, not {type(colour).__name__}')
    _resolved('las_io.survey_colour_files', survey, 'min_intensity')
    pair, bin_start = _each_file('las_io.survey_colour_files', files, lines, survey.bin, survey.half_width, device,
                                 lambda rec, h, tables, shift, select, out:
                                 profile_colour_records(rec, h, *tables, survey, colour, shift, select, out=out), require=require_colour,
                                 chunk_records=chunk_records)
    if pair is None:                                                        # no file: the empty tables of the lines
        host = _empty_bins(bin_start)
        return host, np.zeros_like(host), bin_start
    both = torch.stack(pair).cpu().numpy()                                  # the one read-back
    return both[0], both[1], bin_start


def require_colour(path):
    """-> the point data record format of the LAS file `path`, read off the public header block alone (byte 104, the low six bits, as
    lm_las_parse_header reads it); a format without R, G, B is refused with a ValueError that names the file and the format.  What is
    no LAS file at all is left to parse_header, which refuses it when the file is read."""
    with open(path, 'rb') as f:
        head = f.read(105)
    fmt = head[104] & 0x3F if len(head) == 105 and head[:4] == b'LASF' else None
    if fmt is not None and fmt <= 10 and rgb_offset(fmt) is None:
        raise ValueError(f'colour: {path} is of point format {fmt}, which carries no RGB (formats {sorted(RGB_OFFSET)} do)')
    return fmt


def survey_colour_las(paths, lines, survey, colour, shift, select=None, device='cuda:0'):
    """survey_colour_files for files that share one read offset `shift` and one PointFilter, as survey_las: -> (bins, colours, bin_start);
    marking_summary(bins, bin_start, survey) and marking_colours(bins, colours, bin_start, survey, colour) read the markings off them."""
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    return survey_colour_files([(p, shift, select) for p in paths], lines, survey, colour, device)


def marking_colours(bins, colours, bin_start, survey, colour):
    """The colour of the markings read off the two tables of survey_colour_las (host, integers and float64): bins [n_bins, 6] int64, colours
    [n_bins, 6] int64 (n_c, sum R, sum G, sum B, n_yellow, n_black) and bin_start [L + 1] -> one dict per line:

      coloured, yellow, black   the sums of n_c, n_yellow, n_black over the line's painted bins (painted as in marking_summary: n >=
                                survey.min_points)
      rgb          [sum R / n_c, sum G / n_c, sum B / n_c] over the painted bins, the raw values, not rescaled; None when nothing is coloured
      colour       'unknown' when coloured < colour.min_coloured; 'yellow' when yellow >= colour.yellow_share * coloured (compared exactly,
                   as integers times the share's own rational value); else 'white'
      run_colours  the same three-way answer per paint run, in the order of marking_summary's `runs` (the same joining over
                   survey.max_gap), each from the painted bins of its run: a line that turns from white to yellow says so."""
    from fractions import Fraction
    if not isinstance(survey, MarkingSurvey):
        raise TypeError(f'marking_colours: survey must be a las_io.MarkingSurvey, not {type(survey).__name__}')
    if not isinstance(colour, MarkingColour):
        raise TypeError(f'marking_colours: colour must be a las_io.MarkingColour, not {type(colour).__name__}')
    bins, colours = np.asarray(bins), np.asarray(colours)
    bs = np.asarray(bin_start, dtype=np.int64)
    if bins.ndim != 2 or bins.shape[1] != 6 or bins.dtype != np.int64 or bs.ndim != 1 or len(bs) < 1 or bs[0] != 0 or (np.diff(bs) < 0).any() \
            or bs[-1] != len(bins):
        raise ValueError(f'marking_colours: bins must be [bin_start[L], 6] int64 and bin_start a CSR table from 0, not {bins.shape} '
                         f'{bins.dtype} and {bs.tolist() if len(bs) < 8 else bs.shape}')
    if colours.shape != bins.shape or colours.dtype != np.int64:
        raise ValueError(f'marking_colours: colours must be {list(bins.shape)} int64 like bins, not {list(colours.shape)} {colours.dtype}')
    share = Fraction(colour.yellow_share)                                   # the float's exact value
    gap_bins = int(math.floor(survey.max_gap / survey.bin + 1e-9))

    def decide(n_c, n_y):
        return 'unknown' if n_c < colour.min_coloured else 'yellow' if n_y >= share * n_c else 'white'

    out = []
    for k in range(len(bs) - 1):
        b, c = bins[bs[k]:bs[k + 1]], colours[bs[k]:bs[k + 1]]
        on = b[:, 0] >= survey.min_points
        runs = []
        for i in np.nonzero(on)[0]:
            i = int(i)
            if runs and i - runs[-1][1] - 1 <= gap_bins:
                runs[-1][1] = i
            else:
                runs.append([i, i])
        n_c, n_y, n_k = (int(c[on, j].sum()) for j in (0, 4, 5))
        sums = [int(c[on, j].sum()) for j in (1, 2, 3)]
        run_colours = []
        for i0, i1 in runs:
            sel = on[i0:i1 + 1]
            run_colours.append(decide(int(c[i0:i1 + 1][sel, 0].sum()), int(c[i0:i1 + 1][sel, 4].sum())))
        out.append({'coloured': n_c, 'yellow': n_y, 'black': n_k, 'rgb': [s / n_c for s in sums] if n_c else None,
                    'colour': decide(n_c, n_y), 'run_colours': run_colours})
    return out


class CrossSection(_Options):
    """How the LAS -> map routes take cross-sections along the lane lines they found (immutable; Runner.infer_las_strip_to_map /
    infer_las_to_map, `cross=`; cross_files, cross_summary, snap_lines).  EVERY finite return the labelling rule gives a line (within
    half_width in the plane and z_tol in height, the nearest line winning, no intensity threshold) goes into a table: per station bin
    along the line a row of lateral cells, each holding the count, the paint count, the summed intensity and the summed height above the
    line (the rule: include/lanemap_hip.h).  cross_summary reads stripes, double lines, width, the paint's centre and the cross-fall off
    the table; snap_lines moves the lines onto the paint.

      paint_intensity raw intensity (a number, not NaN; required): a return is paint when its intensity, rounded to a whole number and
                      clamped into 0 .. 65535, is at least ceil(paint_intensity) - `paint_iq`, clamped into 0 .. 65536 (65536: nothing is);
                      or 'auto': the threshold the map routes find in the strip's own returns (PaintThreshold)
      bin             metres (finite, > 0): the length of a station bin along a line
      half_width      metres (finite, 0 .. 16): half the width of the band around a line
      lateral         metres (finite, > 0): the width of a lateral cell; the rule takes lateral_q = max(1, round(1024 lateral)) / 1024 m
      z_tol           metres (0 .. 16): the height band
      min_points      a cell is KNOWN when it holds at least this many returns (whole number >= 1)
      paint_share     0 < paint_share <= 1: a known cell is PAINTED when at least this share of its returns is paint (compared exactly)
      max_hole        up to this many consecutive unknown cells between two painted cells count as painted (whole number >= 0)
      min_stripe      metres (finite, >= 0): a stripe is a maximal painted run at least this wide
      smooth          metres (finite, >= 0): snap_lines moves a vertex by the median centre of the stations whose bin midpoint lies within
                      smooth / 2 of it
      min_stations    with fewer such stations the vertex stays (whole number >= 1)
      max_shift       metres (finite, >= 0): a vertex that would move farther stays - an outlier, not a clamp
    Apart from paint_intensity, which only the data can give ('auto' asks them), the values are plain defaults, not tuned values."""
    __slots__ = ('paint_intensity', 'bin', 'half_width', 'lateral', 'z_tol', 'min_points', 'paint_share', 'max_hole', 'min_stripe', 'smooth',
                 'min_stations', 'max_shift')

    def __init__(self, paint_intensity, bin=0.5, half_width=0.625, lateral=0.03125, z_tol=0.5, min_points=3, paint_share=0.5, max_hole=1,
                 min_stripe=0.05, smooth=2.0, min_stations=2, max_shift=0.3):
        if not _is_auto(paint_intensity) and (not _number(paint_intensity) or math.isnan(float(paint_intensity))):
            raise ValueError(f"CrossSection: paint_intensity={paint_intensity!r} must be a number or 'auto'")
        if not _number(bin) or not (0.0 < float(bin) < math.inf):
            raise ValueError(f'CrossSection: bin={bin!r} must be a finite length > 0')
        if not _number(half_width) or not (0.0 <= float(half_width) <= 16.0):
            raise ValueError(f'CrossSection: half_width={half_width!r} must be a number in 0 .. 16 (metres)')
        if not _number(lateral) or not (0.0 < float(lateral) < math.inf):
            raise ValueError(f'CrossSection: lateral={lateral!r} must be a finite width > 0')
        if not _number(z_tol) or not (0.0 <= float(z_tol) <= 16.0):
            raise ValueError(f'CrossSection: z_tol={z_tol!r} must be a number in 0 .. 16 (metres)')
        if not _whole(min_points) or int(min_points) < 1:
            raise ValueError(f'CrossSection: min_points={min_points!r} must be a whole number >= 1')
        if not _number(paint_share) or not (0.0 < float(paint_share) <= 1.0):
            raise ValueError(f'CrossSection: paint_share={paint_share!r} must be a number with 0 < paint_share <= 1')
        if not _whole(max_hole) or int(max_hole) < 0:
            raise ValueError(f'CrossSection: max_hole={max_hole!r} must be a whole number >= 0')
        if not _number(min_stripe) or not (0.0 <= float(min_stripe) < math.inf):
            raise ValueError(f'CrossSection: min_stripe={min_stripe!r} must be a finite width >= 0')
        if not _number(smooth) or not (0.0 <= float(smooth) < math.inf):
            raise ValueError(f'CrossSection: smooth={smooth!r} must be a finite length >= 0')
        if not _whole(min_stations) or int(min_stations) < 1:
            raise ValueError(f'CrossSection: min_stations={min_stations!r} must be a whole number >= 1')
        if not _number(max_shift) or not (0.0 <= float(max_shift) < math.inf):
            raise ValueError(f'CrossSection: max_shift={max_shift!r} must be a finite length >= 0')
        self._set(paint_intensity=AUTO if _is_auto(paint_intensity) else float(paint_intensity), bin=float(bin), half_width=float(half_width),
                  lateral=float(lateral),
                  z_tol=float(z_tol), min_points=int(min_points), paint_share=float(paint_share), max_hole=int(max_hole),
                  min_stripe=float(min_stripe), smooth=float(smooth), min_stations=int(min_stations), max_shift=float(max_shift))

    @property
    def lateral_q(self):
        """The cell width the device entries take, in 1/1024 m: max(1, round(1024 lateral)), halves up."""
        return max(1, int(math.floor(1024.0 * self.lateral + 0.5)))

    @property
    def paint_iq(self):
        """The integer the device entries take: ceil(paint_intensity), clamped into 0 .. 65536."""
        p = _resolved('CrossSection.paint_iq', self, 'paint_intensity')
        return 65536 if p > 65535.0 else 0 if p <= 0.0 else int(math.ceil(p))

    @property
    def hq(self):
        """ceil(float32(half_width) 1024): the rule's half width in 1/1024 m."""
        return int(math.ceil(float(np.float32(self.half_width)) * 1024.0))

    @property
    def nl(self):
        """The lateral cells of a station bin: 2 hq // lateral_q + 1."""
        return 2 * self.hq // self.lateral_q + 1


def cross_records(records_u8, header, index, stations, cross, shift=None, select=None, out=None):
    """One lm_las_line_cross_records call on the DEVICE records of a file (as profile_records takes them) against an ops.LineIndex and the
    ops.LineStations of the same segments: -> cells [n_bins, nl, 4] int64 device tensor (see ops.line_cross).  The records are only read; a
    record `select` drops contributes nothing.  out: the cells of an earlier call to add to.  Asynchronous."""
    from . import ops
    who = 'las_io.cross_records'
    if not isinstance(cross, CrossSection):
        raise TypeError(f'{who}: cross must be a CrossSection, not {type(cross).__name__}')
    args, dev = _records_args(who, records_u8, header, shift, select, index, stations, 'the cross-section asks', cross.half_width, cross.bin)
    nl = cross.nl
    cells = ops._table_out(who, (stations.n_bins, nl, 4), out, dev)
    n_cells = stations.n_bins * nl
    check(lib().lm_las_line_cross_records(*args, cross.z_tol, cross.lateral_q, cross.paint_iq, int(out is not None),
                                          C.c_void_p(cells.data_ptr()) if n_cells else None, n_cells))
    return cells


def cross_files(files, lines, cross, device='cuda:0', chunk_records=None):
    """The cross-section table of `lines` (list of [n,3] float64, LAS frame) from the LAS files `files`, a list of (path, shift, select):
    every file is read once, uploaded and goes through one lm_las_line_cross_records call with its own read offset and PointFilter, all
    into one table, which is read back once.  The bins each line owns are those of the first file's frame, as in survey_files.
    -> (cells [n_bins, nl, 4] int64 numpy, bin_start [L + 1] int32 numpy)."""
    if not isinstance(cross, CrossSection):
        raise TypeError(f'las_io.cross_files: cross must be a CrossSection, not {type(cross).__name__}')
    _resolved('las_io.cross_files', cross, 'paint_intensity')
    cells, bin_start = _each_file('las_io.cross_files', files, lines, cross.bin, cross.half_width, device,
                                  lambda rec, h, tables, shift, select, out: cross_records(rec, h, *tables, cross, shift, select, out=out),
                                  chunk_records=chunk_records)
    if cells is None:                                                       # no file: the empty table of the lines
        return np.zeros((int(bin_start[-1]), cross.nl, 4), dtype=np.int64), bin_start
    return cells.cpu().numpy(), bin_start                                   # the one read-back


def _median(values):
    v = sorted(values)
    return None if not v else float(v[len(v) // 2]) if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def cross_summary(cells, bin_start, cross):
    """What the cross-section table says about every line (host, integers and float64): cells [n_bins, nl, 4] int64 (n, n_paint, sum iq,
    sum zq) and bin_start [L + 1] -> one dict per line.  Cell c of a station covers the offsets [(c lateral_q - hq) / 1024,
    ((c + 1) lateral_q - hq) / 1024) m, left of the line positive.  A cell is KNOWN with n >= min_points, PAINTED when known and n_paint >=
    paint_share n (exactly: the share's own rational value); up to max_hole consecutive unknown cells between two painted cells count as
    painted; the STRIPES of a station are its maximal painted runs at least min_stripe wide; a station with a stripe is painted and its
    centre is the midpoint of its outermost stripe edges.

      stations    the number of painted stations
      stripes     the most frequent stripe count over the painted stations, ties to the smaller (None without a painted station)
      double      stripes == 2
      width       metres: the median stripe width over the stations with that count
      separation  metres: the median gap between the two stripes of those stations; None unless double
      extent      metres: the median distance between the outermost stripe edges of those stations
      offset      metres: the median centre of those stations - where the paint is, left of the given line positive
      crossfall   m/m, positive rising to the left: the median, over the stations with at least 3 known cells, of the n-weighted least-squares
                  slope of the cells' mean height (sum zq / n / 1024) against the offset of the cell centres; None without such a station
      centres     per station the centre, None where the station is not painted
      counts      per station the number of stripes
    The first five medians are taken over the stations whose stripe count is the line's, so that a stretch where one stripe of a double
    line is worn does not pull them."""
    from fractions import Fraction
    if not isinstance(cross, CrossSection):
        raise TypeError(f'cross_summary: cross must be a las_io.CrossSection, not {type(cross).__name__}')
    cells = np.asarray(cells)
    bs = np.asarray(bin_start, dtype=np.int64)
    hq, lq, nl = cross.hq, cross.lateral_q, cross.nl
    if cells.ndim != 3 or cells.shape[1:] != (nl, 4) or cells.dtype != np.int64 or bs.ndim != 1 or len(bs) < 1 or bs[0] != 0 \
            or (np.diff(bs) < 0).any() or bs[-1] != len(cells):
        raise ValueError(f'cross_summary: cells must be [bin_start[L], {nl}, 4] int64 and bin_start a CSR table from 0, not {cells.shape} '
                         f'{cells.dtype} and {bs.tolist() if len(bs) < 8 else bs.shape}')
    share = Fraction(cross.paint_share)                                     # the float's exact value
    out = []
    for k in range(len(bs) - 1):
        per_station, falls = [], []
        for row in cells[bs[k]:bs[k + 1]]:
            n, npaint, szq = row[:, 0], row[:, 1], row[:, 3]
            known = n >= cross.min_points
            state = [0] * nl                                                # 0 unknown, 1 known and not painted, 2 painted
            for c in np.nonzero(known)[0]:
                state[c] = 2 if int(npaint[c]) >= share * int(n[c]) else 1
            last = None                                                     # the holes
            for c in range(nl):
                if state[c] == 2:
                    if last is not None and 0 < c - last - 1 <= cross.max_hole and all(state[j] == 0 for j in range(last + 1, c)):
                        for j in range(last + 1, c):
                            state[j] = 2
                    last = c
            stripes, c = [], 0
            while c < nl:
                if state[c] == 2:
                    e = c
                    while e + 1 < nl and state[e + 1] == 2:
                        e += 1
                    if (e - c + 1) * lq / 1024.0 >= cross.min_stripe:
                        stripes.append(((c * lq - hq) / 1024.0, ((e + 1) * lq - hq) / 1024.0))
                    c = e + 1
                else:
                    c += 1
            per_station.append(stripes)
            idx = np.nonzero(known)[0]
            if len(idx) >= 3:                                               # X = 2048 x, the cell centre: exact integers up to one division
                X = [(2 * int(c) + 1) * lq - 2 * hq for c in idx]
                w, z = [int(n[c]) for c in idx], [int(szq[c]) for c in idx]
                N, sx, sz = sum(w), sum(a * b for a, b in zip(w, X)), sum(z)
                num = N * sum(a * b for a, b in zip(X, z)) - sx * sz
                den = N * sum(a * b * b for a, b in zip(w, X)) - sx * sx
                falls.append(2.0 * num / den)
        counts = [len(s) for s in per_station]
        painted = [i for i, cnt in enumerate(counts) if cnt]
        stripes = None
        if painted:
            freq = {}
            for i in painted:
                freq[counts[i]] = freq.get(counts[i], 0) + 1
            stripes = min(freq, key=lambda cnt: (-freq[cnt], cnt))
        typical = [per_station[i] for i in painted if counts[i] == stripes]
        centre = lambda s: 0.5 * (s[0][0] + s[-1][1])
        out.append({'stations': len(painted), 'stripes': stripes, 'double': stripes == 2,
                    'width': _median([b - a for s in typical for a, b in s]),
                    'separation': _median([s[1][0] - s[0][1] for s in typical]) if stripes == 2 else None,
                    'extent': _median([s[-1][1] - s[0][0] for s in typical]),
                    'offset': _median([centre(s) for s in typical]),
                    'crossfall': _median(falls),
                    'centres': [centre(s) if s else None for s in per_station],
                    'counts': counts})
    return out


def snap_lines(lines, summary, bin_start, cross):
    """Lines (list of [n, >= 2] float64 arrays, as cross_files took them) moved onto their paint: -> a list of arrays of the same shapes.
    A vertex at station s_v (the arc length in the plane up to it, float64) moves along its left normal by the median centre
    (cross_summary's `centres`) of the stations that qualify: painted, with the line's stripe count, their bin midpoint (i + 1/2) bin within
    smooth / 2 of s_v.  The normal is the normalised sum of the unit left normals (-dy, dx) / len of the nearest segment of non-zero
    length on either side of the vertex.  With fewer than min_stations such stations, a shift beyond max_shift (an outlier, not a clamp)
    or no normal the vertex stays.  Only x and y change."""
    if not isinstance(cross, CrossSection):
        raise TypeError(f'snap_lines: cross must be a las_io.CrossSection, not {type(cross).__name__}')
    lines, bs = list(lines), np.asarray(bin_start, dtype=np.int64)
    if len(summary) != len(lines) or len(bs) != len(lines) + 1:
        raise ValueError(f'snap_lines: {len(lines)} lines, {len(summary)} summaries and a bin_start of {len(bs)} entries do not belong together')
    out = []
    for line, m, nb in zip(lines, summary, np.diff(bs)):
        new = np.array(line, dtype=np.float64, copy=True)
        if len(m['centres']) != nb:
            raise ValueError(f"snap_lines: a line of {int(nb)} bins with {len(m['centres'])} centres")
        if len(new) >= 2 and m['stripes'] is not None:
            d = np.diff(new[:, :2], axis=0)
            seg_len = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
            s_v = np.concatenate([[0.0], np.add.accumulate(seg_len)])
            good = [((i + 0.5) * cross.bin, c) for i, (c, cnt) in enumerate(zip(m['centres'], m['counts'])) if c is not None and cnt == m['stripes']]
            for v in range(len(new)):
                near = [c for mid, c in good if abs(mid - s_v[v]) <= 0.5 * cross.smooth]
                if len(near) < cross.min_stations:
                    continue
                shift = _median(near)
                if abs(shift) > cross.max_shift:
                    continue
                nx = ny = 0.0
                before = [j for j in range(v - 1, -1, -1) if seg_len[j] > 0][:1]
                after = [j for j in range(v, len(seg_len)) if seg_len[j] > 0][:1]
                for j in before + after:
                    nx, ny = nx - d[j, 1] / seg_len[j], ny + d[j, 0] / seg_len[j]
                norm = math.sqrt(nx * nx + ny * ny)
                if norm > 0.0:
                    new[v, 0], new[v, 1] = line[v][0] + shift * nx / norm, line[v][1] + shift * ny / norm
        out.append(new)
    return out


class PaintResidue(_Options):
    """How the LAS -> map routes inventory the paint that no lane line explains (immutable; Runner.infer_las_strip_to_map /
    infer_las_to_map, `residue=`; residue_files, residue_summary).  A return is RESIDUE when it is bright, lies within `reach` in the plane
    and z_tol in height of some line the call found - so signs, vehicles and bridges stay out - and farther than `clear` from the nearest
    such line (the rule: include/lanemap_hip.h).  The residue is put on a grid of `cell` metres, the connected blobs of the grid are
    found and described on the GPU, and residue_summary reads centre, size and heading off every blob large enough.

      min_intensity   REQUIRED, finite: the smallest raw intensity of a paint return.  Without a threshold between asphalt and paint the
                      whole road is one blob, so there is no default; 'auto': the one the map routes find in the strip's own returns
                      (PaintThreshold)
      clear           metres, 0 <= clear < reach: returns within it of their nearest line are that line's paint, not residue
      reach           metres, clear < reach <= 16: how far from a line paint is looked for
      z_tol           metres (>= 0, may be infinite): the height band around the line
      cell            metres (finite, > 0): the size of a grid cell
      connectivity    8 or 4: which cells count as neighbours
      min_cells       a blob is reported when it covers at least this many cells ... (whole number >= 1)
      min_points      ... and holds at least this many returns (whole number >= 1)
      elongated       a blob whose length / width reaches it has a direction; below it the blob is 'compact' (finite, >= 1)
      angle_tol_deg   degrees in 0 .. 45: an elongated blob within it of the nearest segment's direction is 'along', within it of the
                      normal 'across', else 'oblique'
    All defaults are plain defaults, not tuned values."""
    __slots__ = ('min_intensity', 'clear', 'reach', 'z_tol', 'cell', 'connectivity', 'min_cells', 'min_points', 'elongated', 'angle_tol_deg')

    def __init__(self, min_intensity, clear=0.3, reach=6.0, z_tol=0.5, cell=0.1, connectivity=8, min_cells=20, min_points=20, elongated=2.0,
                 angle_tol_deg=30.0):
        if not _is_auto(min_intensity) and (not _number(min_intensity) or not math.isfinite(float(min_intensity))):
            raise ValueError(f"PaintResidue: min_intensity={min_intensity!r} must be a finite number or 'auto' (without one the whole road is "
                             f"one blob)")
        if not _number(reach) or not (0.0 < float(reach) <= 16.0):
            raise ValueError(f'PaintResidue: reach={reach!r} must be a number with 0 < reach <= 16 (metres)')
        if not _number(clear) or not (0.0 <= float(clear) < float(reach)):
            raise ValueError(f'PaintResidue: clear={clear!r} must be a number with 0 <= clear < reach={reach!r}')
        if not _number(z_tol) or not float(z_tol) >= 0.0:
            raise ValueError(f'PaintResidue: z_tol={z_tol!r} must be a number >= 0')
        if not _number(cell) or not (0.0 < float(cell) < math.inf):
            raise ValueError(f'PaintResidue: cell={cell!r} must be a finite size > 0')
        if isinstance(connectivity, bool) or connectivity not in (4, 8):
            raise ValueError(f'PaintResidue: connectivity={connectivity!r} is neither 4 nor 8')
        for name, v in (('min_cells', min_cells), ('min_points', min_points)):
            if not _whole(v) or int(v) < 1:
                raise ValueError(f'PaintResidue: {name}={v!r} must be a whole number >= 1')
        if not _number(elongated) or not (1.0 <= float(elongated) < math.inf):
            raise ValueError(f'PaintResidue: elongated={elongated!r} must be a finite ratio >= 1')
        if not _number(angle_tol_deg) or not (0.0 <= float(angle_tol_deg) <= 45.0):
            raise ValueError(f'PaintResidue: angle_tol_deg={angle_tol_deg!r} must be a number in 0 .. 45 (degrees)')
        self._set(min_intensity=AUTO if _is_auto(min_intensity) else float(min_intensity), clear=float(clear), reach=float(reach), z_tol=float(z_tol), cell=float(cell),
                  connectivity=int(connectivity), min_cells=int(min_cells), min_points=int(min_points), elongated=float(elongated),
                  angle_tol_deg=float(angle_tol_deg))


def residue_index_cell(residue):
    """The cell of the line index residue_files builds, metres.  The index' default, max(1 m, 2 half_width), is sized for the narrow band
    of the labelling; with half_width = reach it lists every segment within reach + a cell's diagonal of the cell, so a large cell
    makes every bright point test several times the segments that can hit it.  The cell decides the cost, never the result."""
    return max(1.0, residue.reach / 4.0)


def decode_chunks(chunks, shift=None, select=None, scratch=None):
    """The clouds of a LasChunks on a device, chunk by chunk: yields [kept,4] float32 tensors (x, y, z, RAW intensity: read_las_raw's
    bits for those records).  select: a PointFilter, applied per chunk (one read of `kept` per chunk, as decode_points).  scratch: a
    [chunk_records,4] float32 tensor every chunk is decoded into - the cloud a step yields is then valid until the next step."""
    h = chunks.header
    if select is not None:
        select.for_format(h['point_format'])
    for rec, m, _ in chunks:
        out = None if scratch is None else scratch[:m]
        if select is None:
            yield decode_points(rec, h['record_len'], m, h['scale'], h['offset'], shift, False, out=out)
        else:
            yield decode_points(rec, h['record_len'], m, h['scale'], h['offset'], shift, False, out=out, point_format=h['point_format'],
                                select=select)


def residue_files(files, lines, residue, device='cuda:0', chunk_records=None):
    """The paint residue of `lines` (list of [n,3] float64, LAS frame) in the LAS files `files`, a list of (path, shift, select) like
    survey_files takes: every file is read once with its own PointFilter (read_las_raw), all clouds go through one ops.paint_residue
    call, and the result is read back once.  The grid lives in ONE frame, that of the first file's read offset: a file listed with
    another offset is decoded against the first one (the decode subtracts the offset in float64, so nothing is lost as long as the
    files lie within float32 reach of it).  chunk_records: None, or the records of a file read and decoded at a time (LasChunks): the
    clouds then reach ops.paint_residue chunk by chunk, and the result is the same.  -> an ops.ResidueBlobs of numpy arrays (cells [M,2] int32, comp [M] int32, stats [K,12]
    int64, grid); grid['shift'] is the frame, what residue_summary needs."""
    from . import ops
    if not isinstance(residue, PaintResidue):
        raise TypeError(f'las_io.residue_files: residue must be a PaintResidue, not {type(residue).__name__}')
    _resolved('las_io.residue_files', residue, 'min_intensity')
    device = torch.device(device)
    lines, files = list(lines), list(files)
    for _, _, select in files:
        if select is not None and not isinstance(select, PointFilter):
            raise TypeError(f'las_io.residue_files: select must be a PointFilter, not {type(select).__name__}')
    frame = None if not files or files[0][1] is None else [float(v) for v in files[0][1]]
    index = ops.line_index(line_segments(lines, frame), residue.reach, cell=residue_index_cell(residue), device=device)
    if chunk_records is None:
        clouds = [read_las_raw(path, device, frame, select)[0] for path, _, select in files]
    else:                                   # ops.paint_residue takes its clouds one at a time and keeps the residue keys only
        from . import las_stream
        clouds = (pts for path, _, select in files for pts in decode_chunks(las_stream.LasChunks(path, chunk_records, device), frame, select))
    out = ops.paint_residue(clouds, index, residue.z_tol, residue.min_intensity, residue.clear, residue.cell, residue.connectivity).numpy()
    out.grid['shift'] = [0.0, 0.0, 0.0] if frame is None else frame
    return out


def _nearest_segment(c, seg):
    """The segment of seg [S,4] float64 (ax, ay, dx, dy) nearest to the point c in the plane: -> (index, signed lateral offset of c, left
    positive, direction of the segment in degrees), by brute force."""
    px, py = c[0] - seg[:, 0], c[1] - seg[:, 1]
    l2 = seg[:, 2] ** 2 + seg[:, 3] ** 2
    t = np.clip(np.divide(px * seg[:, 2] + py * seg[:, 3], l2, out=np.zeros_like(l2), where=l2 > 0), 0.0, 1.0)
    d = np.hypot(px - t * seg[:, 2], py - t * seg[:, 3])
    d = np.where(l2 > 0, d, np.inf) if (l2 > 0).any() else d               # a doubled vertex has no direction: another segment if there is one
    s = int(np.argmin(d))
    ln = math.sqrt(l2[s])
    off = (seg[s, 2] * py[s] - seg[s, 3] * px[s]) / ln if ln > 0 else float(d[s])
    return s, float(off), math.degrees(math.atan2(seg[s, 3], seg[s, 2]))


def residue_summary(result, lines, residue, shift=None):
    """The blobs read off a paint residue (host, Python integers and float64): result an ops.ResidueBlobs of numpy arrays (residue_files),
    lines the lines it was computed against (LAS frame), shift the frame of its grid (default: result.grid['shift'], else none) -> one
    dict per component with n_cells >= residue.min_cells and n_points >= residue.min_points, in component order:

      blob        the component's number, from 1 (its row of stats, its value + 1 in comp)
      centre      [x, y] in the LAS frame: the mean of the cell centres
      cells, points, area (cells cell^2, m^2), intensity (sum iq / points)
      length, width   metres: sqrt(12 l + 1) cell for the larger and the smaller eigenvalue l of the covariance of the cell indices -
                  exact for a filled axis-parallel rectangle of whole cells
      fill        area / (length width): 1 for a filled rectangle, lower for an outline, an arrow, a diagonal
      heading     degrees in [0, 180): the principal axis, counter-clockwise from +x
      bbox        [x_min, y_min, x_max, y_max] of the cells in the LAS frame
      line        the number (from 1) of the line nearest to the centre in the plane, None without a line
      offset      metres: the signed lateral offset of the centre from that line's nearest segment, left positive
      shape       'compact' when length / width < residue.elongated; else 'along' / 'across' when the axis lies within
                  residue.angle_tol_deg of the nearest segment's direction / of its normal; else 'oblique'"""
    if not isinstance(residue, PaintResidue):
        raise TypeError(f'residue_summary: residue must be a las_io.PaintResidue, not {type(residue).__name__}')
    stats, grid = np.asarray(result.stats), result.grid
    if stats.ndim != 2 or stats.shape[1] != 12 or stats.dtype != np.int64:
        raise ValueError(f'residue_summary: stats must be [K,12] int64, not {stats.shape} {stats.dtype}')
    if shift is None:
        shift = grid.get('shift')
    sh = np.zeros(3) if shift is None else np.asarray(shift, dtype=np.float64).reshape(3)
    cell, x0, y0 = float(grid['cell']), float(grid['x0']) + sh[0], float(grid['y0']) + sh[1]
    rows, of_line = [], []
    for k, line in enumerate(lines):
        v = np.asarray(line, dtype=np.float64)
        if v.ndim == 2 and v.shape[0] >= 2:
            rows.append(np.concatenate([v[:-1, :2], v[1:, :2] - v[:-1, :2]], axis=1))
            of_line += [k + 1] * (v.shape[0] - 1)
    seg = np.concatenate(rows) if rows else np.zeros((0, 4))
    out = []
    for k in range(len(stats)):
        n, npts, siq, sx, sy, sxx, sxy, syy, x_lo, x_hi, y_lo, y_hi = (int(v) for v in stats[k])
        if n < residue.min_cells or npts < residue.min_points:
            continue
        # the covariance of the cell indices from exact integers: (n sum x^2 - (sum x)^2) / n^2
        vxx, vxy, vyy = (n * sxx - sx * sx) / (n * n), (n * sxy - sx * sy) / (n * n), (n * syy - sy * sy) / (n * n)
        mid, rad = 0.5 * (vxx + vyy), math.hypot(0.5 * (vxx - vyy), vxy)
        length, width = math.sqrt(12.0 * (mid + rad) + 1.0) * cell, math.sqrt(max(12.0 * (mid - rad), 0.0) + 1.0) * cell
        heading = math.degrees(0.5 * math.atan2(2.0 * vxy, vxx - vyy)) % 180.0
        centre = [x0 + (sx / n + 0.5) * cell, y0 + (sy / n + 0.5) * cell]
        area = n * cell * cell
        line, offset, shape = None, None, 'compact' if length / width < residue.elongated else 'oblique'
        if len(seg):
            s, offset, along = _nearest_segment(centre, seg)
            line = of_line[s]
            if shape != 'compact':
                turn = abs((heading - along + 90.0) % 180.0 - 90.0)         # the angle between two undirected axes, 0 .. 90
                shape = 'along' if turn <= residue.angle_tol_deg else 'across' if turn >= 90.0 - residue.angle_tol_deg else 'oblique'
        out.append({'blob': k + 1, 'centre': centre, 'cells': n, 'points': npts, 'area': area, 'intensity': siq / npts, 'length': length,
                    'width': width, 'fill': area / (length * width), 'heading': heading,
                    'bbox': [x0 + x_lo * cell, y0 + y_lo * cell, x0 + (x_hi + 1) * cell, y0 + (y_hi + 1) * cell], 'line': line,
                    'offset': offset, 'shape': shape})
    return out


def parse_header(data):
    """bytes -> dict of the header fields (raises LanemapHipError on non-LAS / LAZ / truncated files)."""
    h = LmLasHeader()
    data = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data)
    check(lib().lm_las_parse_header(C.c_void_p(data.ctypes.data), int(data.shape[0]), C.byref(h)))
    return {'version': (h.version_major, h.version_minor), 'point_format': h.point_format, 'record_len': h.record_len,
            'n_points': h.n_points, 'offset_to_points': h.offset_to_points, 'scale': list(h.scale), 'offset': list(h.offset),
            'min': list(h.min_xyz), 'max': list(h.max_xyz)}


def decode_points(records_u8, record_len, n, scale, offset, shift=None, normalise=True, out=None, point_format=None, select=None,
                  return_hist=False):
    """records_u8: DEVICE uint8 tensor holding n records (padded to a multiple of 4 bytes) -> [n,4] float32 on that device
    (`out`: a contiguous [n,4] float32 tensor to decode into, e.g. a slice of a batch's point buffer).

    select: a PointFilter (needs `point_format`, the file's point data record format) -> the [kept,4] rows of the records that pass it,
    in file order, the same bits the plain decode gives them: the contiguous view out[:kept] (rows from `kept` on are not written).
    UNLIKE the plain decode this synchronises once, as ops.strip_bin_points does: `kept` is read back to size the view.  z_range is
    compared with the z that is returned, i.e. after `shift`.  return_hist=True: -> (points, hist), hist = int64 numpy [256], the
    classification counts of ALL n records (it travels in the same read-back)."""
    if not records_u8.is_cuda:
        raise LanemapHipError('las_io.decode_points needs the records on an MI355X (HIP) device; no CPU fallback exists')
    if select is not None:
        return _decode_select(records_u8, record_len, n, scale, offset, shift, normalise, out, point_format, select, return_hist)
    if return_hist:
        raise ValueError('las_io.decode_points: return_hist needs select= (PointFilter(drop_withheld=False) keeps every record)')
    out = _decode_out(out, n, records_u8.device)
    check(lib().lm_las_decode_points(C.c_void_p(torch._C._cuda_getCurrentRawStream(records_u8.device.index)), C.c_void_p(records_u8.data_ptr()),
                                     int(record_len), int(n), _d3(scale), _d3(offset), _d3(shift) if shift is not None else None,
                                     INTEN_MIN, INTEN_MAX, int(normalise), C.c_void_p(out.data_ptr())))
    return out


def _decode_out(out, n, device):
    """-> `out` after its check, or a new [n,4] float32 tensor on `device`: where decode_points writes its rows."""
    if out is None:
        return torch.empty((n, 4), device=device, dtype=torch.float32)
    if tuple(out.shape) != (n, 4) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != device:
        raise ValueError(f'las_io.decode_points: out must be a contiguous [{n},4] float32 tensor on {device}')
    return out


def _decode_select(records_u8, record_len, n, scale, offset, shift, normalise, out, point_format, select, return_hist):
    if not isinstance(select, PointFilter):
        raise TypeError(f'las_io.decode_points: select must be a PointFilter, not {type(select).__name__}')
    if point_format is None:
        raise ValueError('las_io.decode_points: select= needs point_format (classification and flags sit in other bits from format 6 on)')
    sel = select.for_format(point_format).as_struct()
    dev = records_u8.device
    out = _decode_out(out, n, dev)
    L = lib()
    need = int(L.lm_las_select_workspace_bytes(int(n)))
    ws = torch.empty((max(need, 4),), device=dev, dtype=torch.uint8)
    meta = torch.empty((257,), device=dev, dtype=torch.int64)          # kept, then the class histogram
    check(L.lm_las_decode_select(C.c_void_p(torch._C._cuda_getCurrentRawStream(dev.index)), C.c_void_p(records_u8.data_ptr()),
                                 int(record_len), int(point_format), int(n), _d3(scale), _d3(offset), _d3(shift) if shift is not None else None,
                                 INTEN_MIN, INTEN_MAX, int(normalise), C.byref(sel), C.c_void_p(ws.data_ptr()), need,
                                 C.c_void_p(out.data_ptr()), C.c_void_p(meta.data_ptr()),
                                 C.c_void_p(meta.data_ptr() + 8) if return_hist else None))
    host = (meta if return_hist else meta[:1]).cpu().numpy()          # the one synchronisation
    kept = int(host[0])
    pts = out[:kept]
    return (pts, host[1:].copy()) if return_hist else pts


def _read(path, device, shift, normalise, select=None, class_hist=False):
    data = np.fromfile(path, dtype=np.uint8)
    h = parse_header(data)
    n, rl = h['n_points'], h['record_len']
    if select is not None:
        select.for_format(h['point_format'])                          # refused before anything is uploaded
    elif class_hist:
        raise ValueError('las_io: class_hist needs select= (PointFilter(drop_withheld=False) keeps every record)')
    rec = _upload_records(data, h, device)
    if select is None:
        return decode_points(rec, rl, n, h['scale'], h['offset'], shift, normalise), h
    res = decode_points(rec, rl, n, h['scale'], h['offset'], shift, normalise, point_format=h['point_format'], select=select,
                        return_hist=class_hist)
    pts = res[0] if class_hist else res
    h['n_kept'] = int(pts.shape[0])
    if class_hist:
        h['class_hist'] = res[1]
    return pts, h


def read_las(filepath, device='cuda:0', shift=None, select=None):
    """-> [N,4] float32 (x, y, z, normalised intensity) on `device`, like the reference's read_las.  select: a PointFilter, see
    decode_points (one synchronisation; the "fewer than 5 points" refusal then counts the kept points)."""
    pts, _ = _read(filepath, torch.device(device), shift, True, select)
    if pts.shape[0] < 5:
        raise ValueError(f'{filepath}: only {pts.shape[0]} lidar points' + (' pass the filter' if select is not None else ''))
    return pts


def read_las_raw(filepath, device='cuda:0', shift=None, select=None, class_hist=False):
    """-> ([N,4] float32 with RAW intensity, header dict): the record layout lm_bev_raster_batch consumes.  select: a PointFilter, see
    decode_points: the kept points only, header['n_kept'] their number (header['n_points'] stays the file's); class_hist=True adds
    header['class_hist'], int64 [256], the classification counts of all records of the file."""
    return _read(filepath, torch.device(device), shift, False, select, class_hist)


def grid_layout(header, img_reso=(0.05, 0.05), overlap_px=128, H=1152, W=1152, ele_reso=0.05, las_read_offset=None):
    """A tile layout for a strip that comes without one: axis-aligned H x W windows (identity quaternion) over the bounding box of the
    LAS header, neighbours sharing `overlap_px` pixels, rows along x and columns along y like the rasteriser.  -> list of parameter
    dicts (the keys of io_utils.load_pc_2_img_transform_paras), x-major.  las_read_offset defaults to the header's minimum corner,
    floored to whole metres; local_min_ele is the header's z minimum in that frame: ONE datum for the whole strip, which is only a
    fallback - the elevation channel spans 255 steps of ele_reso above it (12.75 m at 0.05), so relief along the strip or one low noise
    return saturates it.  Pass `ground=GroundFilter()` to Runner.infer_las_strip_to_map to give every tile a datum under its own
    ground."""
    lo, hi = header['min'], header['max']
    off = [float(np.floor(v)) for v in lo] if las_read_offset is None else [float(v) for v in las_read_offset]
    assert 0 <= overlap_px < min(H, W)
    span = [(H - overlap_px) * float(img_reso[0]), (W - overlap_px) * float(img_reso[1])]
    size = [H * float(img_reso[0]), W * float(img_reso[1])]
    n = [max(1, int(np.ceil(((hi[a] - lo[a]) - size[a]) / span[a] - 1e-9)) + 1) for a in range(2)]
    out = []
    for i in range(n[0]):
        for j in range(n[1]):
            out.append({'coor_las_path': '', 'las_read_offset': list(off),
                        'las_rotation_trans_quan': [lo[0] - off[0] + i * span[0], lo[1] - off[1] + j * span[1], 0.0, 1.0, 0.0, 0.0, 0.0],
                        'bev_img_offset': [0.0, 0.0], 'img_reso': [float(img_reso[0]), float(img_reso[1])],
                        'local_min_ele': float(lo[2] - off[2]), 'ele_reso': float(ele_reso)})
    return out
