"""The option classes of the LAS routes, and nothing else: one immutable value per stage argument of Runner.infer_las_to_map /
infer_las_strip_to_map (select, ground, intensity, elevation, density, label, survey, colour, cross, residue, threshold, stream), each
validating its arguments in __init__; `_Options` is what they share.  las_io imports every name here at its top: `las_io.<name>` is the
same object.  The passes over the records and the policy functions that take an options object (ground_datum, intensity_window,
gap_radius, marking_summary, paint_threshold, tile_groups, ...) are in las_io.py.  This module imports math, numpy and the ctypes structs
of _lib (PointFilter.as_struct; that does not load the library) - nothing else of the package, no torch, no library call.

A new stage: its options class goes here and into OPTION_CASES of tests/test_las_select_cpu.py, its passes go into las_io.py."""
import math

import numpy as np

from ._lib import LmLasSelect

DROP_SYNTHETIC, DROP_KEYPOINT, DROP_WITHHELD, DROP_OVERLAP = 1, 2, 4, 8          # LM_LAS_DROP_* (include/lanemap_hip.h)
RETURNS = {'all': 0, 'first': 1, 'last': 2, 'single': 3}                         # LM_LAS_RETURNS_*
CHUNK_MULTIPLE = 256                # records per workgroup of the record kernels: every chunk but the last is whole workgroups


def _number(v):
    """A Python or numpy number, no bool: what an option that is a length, a ratio or an intensity takes."""
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def _whole(v):
    """A Python or numpy integer, no bool: what an option that is a count takes."""
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


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


def _is_table(v):
    """A las_io.PaintTable: a threshold per line or station window, which min_intensity / paint_intensity take wherever they take 'auto'."""
    return isinstance(v, _Table)


def paint_iq_of(p):
    """The integer the cross-section entries compare iq with: ceil(p), clamped into 0 .. 65536 (65536: nothing is paint)."""
    return 65536 if p > 65535.0 else 0 if p <= 0.0 else int(math.ceil(p))


def _check_chunk_records(who, chunk_records):
    if not _whole(chunk_records) or int(chunk_records) <= 0 or int(chunk_records) % CHUNK_MULTIPLE:
        raise ValueError(f'{who}: chunk_records={chunk_records!r} must be a positive multiple of {CHUNK_MULTIPLE}')
    return int(chunk_records)


class _Options:
    """What the option classes of this module share: a value that cannot be changed, compared, hashed and printed by the __slots__ of its
    class, in their order.  A class validates its arguments in __init__ and stores them with _set."""
    __slots__ = ()
    _later = {}                         # arguments a class took on after its __slots__ were what callers compare with: {name: default};
    #                                     they are kept in the slots of a base class, compared and hashed like the others, and printed
    #                                     where they differ from the default - so a value without them prints as it always did

    def _set(self, **values):
        for k, v in values.items():
            object.__setattr__(self, k, v)

    def _fields(self):
        return tuple(self.__slots__) + tuple(self._later)

    def _replace(self, **changes):
        """A copy with some arguments changed, validated again (for the classes whose __slots__ are their constructor's arguments)."""
        return type(self)(**{**{k: getattr(self, k) for k in self._fields()}, **changes})

    def __setattr__(self, name, value):
        raise AttributeError(f'{type(self).__name__} is immutable')

    def __delattr__(self, name):
        raise AttributeError(f'{type(self).__name__} is immutable')

    def __repr__(self):
        shown = tuple(self.__slots__) + tuple(k for k, d in self._later.items() if getattr(self, k) != d)
        return type(self).__name__ + '(' + ', '.join(f'{k}={getattr(self, k)!r}' for k in shown) + ')'

    def __eq__(self, other):
        return type(other) is type(self) and all(getattr(self, k) == getattr(other, k) for k in self._fields())

    def __hash__(self):
        return hash(tuple(getattr(self, k) for k in self._fields()))


def _later_slots(*names):
    """-> a base class that holds the `_later` arguments of an options class in slots of its own, so that the class keeps its __slots__."""
    return type('_LaterSlots', (_Options,), {'__slots__': names})


class _Table(_Options):
    """The base of las_io.PaintTable, here so that the stage options can tell one without importing las_io."""
    __slots__ = ()


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


class IntensityStretch(_later_slots('balance', 'cell_px', 'cell_min_points', 'max_gain')):
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
      balance       True: before the window is fitted, the binned points are balanced in place (ops.tile_intensity_cells,
                    balance_gains, ops.tile_intensity_apply; the rule: include/lanemap_hip.h).  A scanner's intensity falls with range, so
                    under any single window the outer lanes rasterise as dark paint on black and the near lane as asphalt brighter than
                    that paint.  Per cell of cell_px x cell_px pixels the median intensity is the local asphalt level (paint is the
                    minority of a road cell); the lower median of that over the 3 x 3 known cells keeps a cell that is mostly paint from
                    dimming itself; every point is multiplied by the gain that takes its place's level to one reference level - the
                    median of the tile ('tile') or of the call ('strip') - interpolated between the cell centres.  False (the default):
                    nothing changes, bit for bit and call for call
      cell_px       16 .. 128 pixels per cell (default 32: 1.6 m at 0.05 m per pixel)
      cell_min_points  a cell is known with at least this many counted points (whole number >= 1); unknown cells keep gain 1
      max_gain      finite, >= 1: gains are clipped into [1 / max_gain, max_gain]
    min_span, min_points, cell_px, cell_min_points and max_gain are plain defaults, not tuned values."""
    __slots__ = ('percentiles', 'scope', 'white', 'min_span', 'min_points', 'fallback')
    _later = {'balance': False, 'cell_px': 32, 'cell_min_points': 64, 'max_gain': 4.0}

    def __init__(self, percentiles=(1.0, 99.9), scope='tile', white=249, min_span=16, min_points=1024, fallback=(800.0, 33000.0),
                 balance=False, cell_px=32, cell_min_points=64, max_gain=4.0):
        if not isinstance(balance, (bool, np.bool_)):
            raise ValueError(f'IntensityStretch: balance={balance!r} must be True or False')
        if not _whole(cell_px) or not 16 <= int(cell_px) <= 128:
            raise ValueError(f'IntensityStretch: cell_px={cell_px!r} must be a whole number of pixels in 16..128')
        if not _whole(cell_min_points) or int(cell_min_points) < 1:
            raise ValueError(f'IntensityStretch: cell_min_points={cell_min_points!r} must be a whole number >= 1')
        if not _number(max_gain) or not (1.0 <= float(max_gain) < math.inf):
            raise ValueError(f'IntensityStretch: max_gain={max_gain!r} must be a finite number >= 1')
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
                  fallback=(f_lo, f_hi), balance=bool(balance), cell_px=int(cell_px), cell_min_points=int(cell_min_points),
                  max_gain=float(max_gain))


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


class MarkingLabels(_Options):
    """How the LAS -> map routes label the returns of their input by the lines they found (immutable; Runner.infer_las_strip_to_map /
    infer_las_to_map, `label=`; label_las).  A return is labelled with line k (counted from 1 in the order of the lines) when it lies within
    half_width of the line in the plane and within z_tol of it in height, the nearest line winning (the rule: include/lanemap_hip.h).

      half_width      metres (finite, >= 0): half the width of the band around a line in which a return counts as its paint
      z_tol           metres (>= 0, may be infinite): the height band; it only keeps a carriageway from labelling the one under or over it
      min_intensity   None, the smallest raw intensity a labelled return has (paint is bright), 'auto': the threshold the map routes
                      find in the strip's own returns (PaintThreshold), or a las_io.PaintTable: a threshold per line or station window
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
        if min_intensity is not None and not _is_auto(min_intensity) and not _is_table(min_intensity):
            if not _number(min_intensity) or math.isnan(float(min_intensity)):
                raise ValueError(f"MarkingLabels: min_intensity={min_intensity!r} must be None, a number, 'auto' or a PaintTable")
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
        if min_intensity is not None and not _is_auto(min_intensity) and not _is_table(min_intensity):
            if not _number(min_intensity) or math.isnan(float(min_intensity)):
                raise ValueError(f"MarkingSurvey: min_intensity={min_intensity!r} must be None, a number, 'auto' or a PaintTable")
            min_intensity = float(min_intensity)
        if not _whole(min_points) or int(min_points) < 1:
            raise ValueError(f'MarkingSurvey: min_points={min_points!r} must be a whole number >= 1')
        if not _number(max_gap) or not (0.0 <= float(max_gap) < math.inf):
            raise ValueError(f'MarkingSurvey: max_gap={max_gap!r} must be a finite length >= 0')
        if not _number(solid_cover) or not (0.0 < float(solid_cover) <= 1.0):
            raise ValueError(f'MarkingSurvey: solid_cover={solid_cover!r} must be a number with 0 < solid_cover <= 1')
        self._set(bin=float(bin), half_width=float(half_width), z_tol=float(z_tol), min_intensity=min_intensity, min_points=int(min_points),
                  max_gap=float(max_gap), solid_cover=float(solid_cover))


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
        given = _is_auto(paint_intensity) or _is_table(paint_intensity)
        if not given and (not _number(paint_intensity) or math.isnan(float(paint_intensity))):
            raise ValueError(f"CrossSection: paint_intensity={paint_intensity!r} must be a number, 'auto' or a PaintTable")
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
        self._set(paint_intensity=paint_intensity if given else float(paint_intensity), bin=float(bin), half_width=float(half_width),
                  lateral=float(lateral),
                  z_tol=float(z_tol), min_points=int(min_points), paint_share=float(paint_share), max_hole=int(max_hole),
                  min_stripe=float(min_stripe), smooth=float(smooth), min_stations=int(min_stations), max_shift=float(max_shift))

    @property
    def lateral_q(self):
        """The cell width the device entries take, in 1/1024 m: max(1, round(1024 lateral)), halves up."""
        return max(1, int(math.floor(1024.0 * self.lateral + 0.5)))

    @property
    def paint_iq(self):
        """The integer the device entries take: ceil(paint_intensity), clamped into 0 .. 65536; of a PaintTable, that of every row."""
        p = _resolved('CrossSection.paint_iq', self, 'paint_intensity')
        return np.array([paint_iq_of(float(v)) for v in p.thr], dtype=np.int32) if _is_table(p) else paint_iq_of(p)

    @property
    def hq(self):
        """ceil(float32(half_width) 1024): the rule's half width in 1/1024 m."""
        return int(math.ceil(float(np.float32(self.half_width)) * 1024.0))

    @property
    def nl(self):
        """The lateral cells of a station bin: 2 hq // lateral_q + 1."""
        return 2 * self.hq // self.lateral_q + 1


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
        given = _is_auto(min_intensity) or _is_table(min_intensity)
        if not given and (not _number(min_intensity) or not math.isfinite(float(min_intensity))):
            raise ValueError(f"PaintResidue: min_intensity={min_intensity!r} must be a finite number, 'auto' or a PaintTable (without one the "
                             f"whole road is one blob)")
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
        self._set(min_intensity=min_intensity if given else float(min_intensity), clear=float(clear), reach=float(reach), z_tol=float(z_tol), cell=float(cell),
                  connectivity=int(connectivity), min_cells=int(min_cells), min_points=int(min_points), elongated=float(elongated),
                  angle_tol_deg=float(angle_tol_deg))


THRESHOLD_SCOPES = ('strip', 'line', 'window')


class PaintThreshold(_later_slots('scope', 'window')):
    """How the LAS -> map routes find the intensity threshold between asphalt and paint in the strip's own returns (immutable;
    Runner.infer_las_strip_to_map / infer_las_to_map, `threshold=`; hist_files, paint_threshold) - the number MarkingLabels, MarkingSurvey
    and PaintResidue take as min_intensity and CrossSection as paint_intensity, which they ask for with 'auto'.  Every finite return the
    labelling rule gives a line (within half_width in the plane and z_tol in height, no intensity threshold) is counted per line and per
    lateral ring r = min(|q|, hq) // ring_q in a histogram of its intensity >> bin_shift (the rule: include/lanemap_hip.h).  The INNER
    rings, on the line, hold paint plus some asphalt; the OUTER rings, beside it, asphalt; paint_threshold takes the threshold that
    separates the two populations best, for the strip and for every line.

      half_width      metres (finite, 0 .. 16): half the width of the band around a line
      ring            metres (finite, > 0): the width of a ring; ring_q = round(1024 ring) / 1024 m, at least 1/1024
      inner           metres: ring r is an inner ring when (r + 1) ring_q <= inner_q = round(1024 inner)
      outer           metres: ring r is an outer ring when r ring_q >= outer_q = round(1024 outer); inner <= outer <= half_width, and
                      neither set may be empty
      z_tol           metres (0 .. 16): the height band
      bin_shift       whole number 0 .. 8: a histogram has 65536 >> bin_shift counts, the threshold is a multiple of 1 << bin_shift
      min_returns     a group (the strip, a line) is supported only with at least this many inner and this many outer returns
      min_separation  ... and a separation D (paint_threshold) of at least this, 0 .. 1
      tolerance_shift whole number 1 .. 30: the threshold is the middle of the plateau on which J stays within M >> tolerance_shift of its
                      maximum M
      scope           'strip': one threshold for the strip, which replaces every 'auto' (the default, and all there was before `scope`);
                      'line': one per line; 'window': one per station window of `window` metres along every line.  With 'line' and 'window'
                      the histograms are taken per window (hist_window_files), paint_table reads a las_io.PaintTable off them - a window
                      without support takes its line's threshold, a line without support the strip's - and every 'auto' becomes that table,
                      looked up for each return on the GPU.  A scanner's intensity falls with range, so the paint of an outer lane is
                      routinely darker than the asphalt under the scanner: no single number serves such a strip
      window          metres (finite, > 0): the length of a station window; only read with scope='window'
    Apart from the derived KS_COEFF = 1.95 of the support test, the defaults - scope and window = 50 m among them - are plain defaults, not
    tuned values."""
    __slots__ = ('half_width', 'ring', 'inner', 'outer', 'z_tol', 'bin_shift', 'min_returns', 'min_separation', 'tolerance_shift')
    _later = {'scope': 'strip', 'window': 50.0}

    def __init__(self, half_width=0.625, ring=0.0625, inner=0.125, outer=0.375, z_tol=0.5, bin_shift=6, min_returns=1000,
                 min_separation=0.05, tolerance_shift=5, scope='strip', window=50.0):
        if not (isinstance(scope, str) and scope in THRESHOLD_SCOPES):
            raise ValueError(f"PaintThreshold: scope={scope!r} must be 'strip', 'line' or 'window'")
        if not _number(window) or not (0.0 < float(window) < math.inf):
            raise ValueError(f'PaintThreshold: window={window!r} must be a finite length > 0')
        if not _number(half_width) or not (0.0 <= float(half_width) <= 16.0):
            raise ValueError(f'PaintThreshold: half_width={half_width!r} must be a number in 0 .. 16 (metres)')
        if not _number(ring) or not (0.0 < float(ring) < math.inf):
            raise ValueError(f'PaintThreshold: ring={ring!r} must be a finite width > 0')
        for name, v in (('inner', inner), ('outer', outer)):
            if not _number(v) or not (0.0 <= float(v) < math.inf):
                raise ValueError(f'PaintThreshold: {name}={v!r} must be a finite width >= 0')
        if float(inner) > float(outer):
            raise ValueError(f'PaintThreshold: inner={inner!r} lies beyond outer={outer!r}')
        if float(outer) > float(half_width):
            raise ValueError(f'PaintThreshold: outer={outer!r} lies beyond half_width={half_width!r}')
        if not _number(z_tol) or not (0.0 <= float(z_tol) <= 16.0):
            raise ValueError(f'PaintThreshold: z_tol={z_tol!r} must be a number in 0 .. 16 (metres)')
        if not _whole(bin_shift) or not 0 <= int(bin_shift) <= 8:
            raise ValueError(f'PaintThreshold: bin_shift={bin_shift!r} must be a whole number in 0 .. 8')
        if not _whole(min_returns) or int(min_returns) < 1:
            raise ValueError(f'PaintThreshold: min_returns={min_returns!r} must be a whole number >= 1')
        if not _number(min_separation) or not (0.0 <= float(min_separation) <= 1.0):
            raise ValueError(f'PaintThreshold: min_separation={min_separation!r} must be a number in 0 .. 1')
        if not _whole(tolerance_shift) or not 1 <= int(tolerance_shift) <= 30:
            raise ValueError(f'PaintThreshold: tolerance_shift={tolerance_shift!r} must be a whole number in 1 .. 30')
        self._set(half_width=float(half_width), ring=float(ring), inner=float(inner), outer=float(outer), z_tol=float(z_tol),
                  bin_shift=int(bin_shift), min_returns=int(min_returns), min_separation=float(min_separation),
                  tolerance_shift=int(tolerance_shift), scope=scope, window=float(window))
        if not self.inner_rings:
            raise ValueError(f'PaintThreshold: no ring of {self.ring_q}/1024 m lies within inner={inner!r}: the inner set is empty')
        if not self.outer_rings:
            raise ValueError(f'PaintThreshold: no ring of {self.ring_q}/1024 m starts at or beyond outer={outer!r} inside half_width='
                             f'{half_width!r}: the outer set is empty')

    @property
    def ring_q(self):
        """The ring width the device entries take, in 1/1024 m: max(1, round(1024 ring)), halves up."""
        return max(1, int(math.floor(1024.0 * self.ring + 0.5)))

    @property
    def inner_q(self):
        return int(math.floor(1024.0 * self.inner + 0.5))

    @property
    def outer_q(self):
        return int(math.floor(1024.0 * self.outer + 0.5))

    @property
    def hq(self):
        """ceil(float32(half_width) 1024): the rule's half width in 1/1024 m."""
        return int(math.ceil(float(np.float32(self.half_width)) * 1024.0))

    @property
    def rings(self):
        """Z, the rings of a line: hq // ring_q + 1."""
        return self.hq // self.ring_q + 1

    @property
    def n_counts(self):
        """NB, the counts of a histogram: 65536 >> bin_shift."""
        return 65536 >> self.bin_shift

    @property
    def inner_rings(self):
        return [r for r in range(self.rings) if (r + 1) * self.ring_q <= self.inner_q]

    @property
    def outer_rings(self):
        return [r for r in range(self.rings) if r * self.ring_q >= self.outer_q]


class StripStream(_Options):
    """How Runner.infer_las_strip_to_map maps a strip that does not fit in memory (immutable; `stream=`).

      chunk_records   the records read, uploaded, decoded and binned at a time: a positive multiple of 256.  Device memory per chunk is
                      its records, a scratch cloud of 16 bytes per record and the binning's table
      binned_budget   None, or the bytes (whole number > 0) the binned points of one group of tiles may take: the tiles are cut, in layout
                      order and at multiples of the batch size, into groups with 16 * sum(counts) <= binned_budget, and the files are
                      read once more per group.  A batch that alone exceeds the budget is a group of its own.  None: one group
    Both defaults are plain defaults, not tuned values."""
    __slots__ = ('chunk_records', 'binned_budget')

    def __init__(self, chunk_records=1 << 24, binned_budget=None):
        chunk_records = _check_chunk_records('StripStream', chunk_records)
        if binned_budget is not None:
            if not _whole(binned_budget) or int(binned_budget) <= 0:
                raise ValueError(f'StripStream: binned_budget={binned_budget!r} must be None or a whole number of bytes > 0')
            binned_budget = int(binned_budget)
        self._set(chunk_records=chunk_records, binned_budget=binned_budget)
