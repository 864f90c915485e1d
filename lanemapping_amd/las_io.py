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

`PaintThreshold` / `hist_files` / `paint_threshold` find the intensity threshold between asphalt and paint that the four stages above
need: a histogram of the intensities per line and lateral ring (`ops.line_hist`, `lm_las_line_hist_records`), off which the host reads
the threshold that best separates the returns ON the lines from those BESIDE them; 'auto' in the four classes asks the map routes for it.

`StripStream` / `LasChunks` / `tile_groups` map a strip that does not fit in memory: the files read in chunks of records, counted and
then scattered into groups of tiles (`ops.StripBinner`), and the record passes above fed chunk by chunk (`chunk_records=`).

`PaintThreshold(scope='line' | 'window')` / `hist_window_files` / `paint_table` / `PaintTable` make the threshold a table, one value per
line or per station window along every line, for strips whose intensity falls with range: the histograms are taken per window
(`lm_las_line_hist_window_records`), a window without support takes its line's threshold and a line without support the strip's, and the
four stages look the value up for every return on the GPU (the `_local` entries) where their option holds the table.

The option classes are defined in las_options.py and imported here (`las_io.<name>` is the same object); the readers, the passes over
the records and the policy functions that take an options object are here.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from ._lib import lib, check, LmLasHeader, LanemapHipError
from .las_options import (AUTO, CHUNK_MULTIPLE, DROP_KEYPOINT, DROP_OVERLAP, DROP_SYNTHETIC, DROP_WITHHELD, RETURNS, CrossSection,
                          ElevationDrape, GapFill, GroundFilter, IntensityStretch, MarkingColour, MarkingLabels, MarkingSurvey, PaintResidue,
                          PaintThreshold, PointFilter, StripStream, THRESHOLD_SCOPES, _Options, _Table, _check_chunk_records, _is_auto, _is_table,
                          _number, _resolved, _whole, paint_iq_of)

INTEN_MIN, INTEN_MAX = 800.0, 33000.0


def ground_datum(ground_min, ele_reso, margin, fallback):
    """The elevation datum of a tile from its lowest ground cell: floor((ground_min - margin) / ele_reso) * ele_reso in float64, a whole
    number of elevation steps so that G of a point at the datum is exactly 0; `fallback` for ground_min = +inf (a tile without points)."""
    g = float(ground_min)
    if math.isnan(g) or g == -math.inf:
        raise ValueError(f'ground_datum: ground_min={ground_min!r} is neither finite nor +inf')
    if g == math.inf:
        return float(fallback)
    return math.floor((g - float(margin)) / float(ele_reso)) * float(ele_reso)


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


def balance_gains(model, reference, stretch, count=None):
    """The gain field of the intensity balance (the rule: include/lanemap_hip.h) from ops.tile_intensity_cells' model [B, Gy, Gx] (-1: no
    known cell near) and a reference level per tile, reference [B] - the lower median key of the tile ('tile') or of the call ('strip'),
    ops.tile_intensity_window(percentiles=(50, 50)).  -> float32 [B, Gy, Gx]: for a known model and reference[b] > 0
    clip(float32(reference[b]) / float32(max(model, 1)), 1 / max_gain, max_gain) in float32 operations, else 1.  count [B], when given,
    holds the counted points behind every reference: a tile whose count is below stretch.min_points keeps gain 1 everywhere, as its window
    keeps the fallback."""
    if not isinstance(stretch, IntensityStretch):
        raise TypeError(f'balance_gains: stretch must be a las_io.IntensityStretch, not {type(stretch).__name__}')
    model = np.asarray(model)
    if model.ndim != 3 or model.dtype.kind not in 'iu':
        raise ValueError(f'balance_gains: model must be a [B, Gy, Gx] integer array, not {model.dtype} {list(model.shape)}')
    ref = np.asarray(reference, dtype=np.int64).reshape(-1)
    if len(ref) != model.shape[0]:
        raise ValueError(f'balance_gains: {len(ref)} reference levels for {model.shape[0]} tiles')
    if count is not None:
        cnt = np.asarray(count, dtype=np.int64).reshape(-1)
        if len(cnt) != len(ref):
            raise ValueError(f'balance_gains: {len(cnt)} counts for {len(ref)} tiles')
        ref = np.where(cnt < stretch.min_points, 0, ref)
    top = np.float32(stretch.max_gain)
    ratio = ref.astype(np.float32)[:, None, None] / np.maximum(model, 1).astype(np.float32)
    gains = np.clip(ratio, np.float32(1.0) / top, top).astype(np.float32)
    return np.where((model >= 0) & (ref[:, None, None] > 0), gains, np.float32(1.0)).astype(np.float32)


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


def _paint_rows(who, table, stations, n_lines, cross=False):
    """The PaintTable of a stage option on the device of `stations` (the [S,4] f32 tensor of the segments' ops.LineStations), checked
    against the lines: -> an ops.PaintRows.  cross: with the cross-sections' integer of every row."""
    from . import ops
    if len(table.win_start) != n_lines + 1:
        raise ValueError(f'{who}: the paint table was cut for {len(table.win_start) - 1} lines, the call has {n_lines}')
    key = (table, stations.data_ptr(), str(stations.device), bool(cross))
    if _ROWS[:1] != [key]:                  # the chunks of a file, and the files of a frame, come with the same tables: uploaded once
        _ROWS[:] = [key, ops.paint_rows(table.thr, table.win_start, table.window, stations,
                                        paint_iq=np.array([paint_iq_of(float(v)) for v in table.thr], dtype=np.int32) if cross else None)]
    return _ROWS[1]


_ROWS = []                          # the last (key, ops.PaintRows) of _paint_rows


def label_records(records_u8, header, index, labels, shift=None, select=None, n_lines=None, want_line=False, stations=None):
    """One lm_las_label_records call on the DEVICE records of a file (padded to a multiple of 4 bytes; `header`: parse_header's dict)
    against an ops.line_index: -> (patched records, counts [n_lines + 1] int64 device tensor[, line [n] int32]).  Asynchronous.
    Where labels.min_intensity is a PaintTable the call is lm_las_label_records_local, and `stations` - the ops.LineStations of the same
    segments, any bin - is required: the table's rows are looked up with it."""
    if not isinstance(labels, MarkingLabels):
        raise TypeError(f'las_io.label_records: labels must be a MarkingLabels, not {type(labels).__name__}')
    args, dev = _records_args('las_io.label_records', records_u8, header, shift, select, index, None, 'labels ask', labels.half_width)
    cls = labels.for_format(header['point_format'])
    L = index.n_lines if n_lines is None else int(n_lines)
    out = torch.empty_like(records_u8)
    counts = torch.empty((L + 1,), device=dev, dtype=torch.int64)
    line = torch.empty((header['n_points'],), device=dev, dtype=torch.int32) if want_line else None
    mi = _resolved('las_io.label_records', labels, 'min_intensity')
    tail = (cls, int(labels.line_ids), C.c_void_p(out.data_ptr()), C.c_void_p(line.data_ptr()) if want_line else None,
            C.c_void_p(counts.data_ptr()), L)
    if _is_table(mi):
        if stations is None or stations.n_segments != index.n_segments:
            raise ValueError('las_io.label_records: a PaintTable needs stations=, the ops.LineStations of the index\' segments')
        table = _paint_rows('las_io.label_records', mi, stations.stations, L).struct()
        check(lib().lm_las_label_records_local(*args[1:], labels.z_tol, C.byref(table), *tail, args[0]))
    else:
        check(lib().lm_las_label_records(*args, labels.z_tol, math.nan if mi is None else mi, *tail))
    return (out, counts, line) if want_line else (out, counts)


def _label_stations(lines, labels, shift, device):
    """The station table label_las needs beside its index when labels.min_intensity is a PaintTable (else None)."""
    from . import ops
    if not _is_table(labels.min_intensity):
        return None
    return ops.line_stations(*line_stations(lines, shift, labels.min_intensity.window), labels.min_intensity.window, device=device)


def _label_las_chunked(path, out_path, lines, labels, shift, select, device, chunk_records):
    """label_las for a file that is never held whole: the bytes before the records, then every chunk of records relabelled (one
    lm_las_label_records call and one read-back per chunk, written as it comes back), then the bytes after them; the counts add up.  A
    label depends on its record alone, so the file is byte for byte the one the whole-file pass writes."""
    from . import ops
    chunks = LasChunks(path, chunk_records, device)
    h = chunks.header
    rl = h['record_len']
    labels.for_format(h['point_format'])                                  # refused before anything is uploaded
    if select is not None:
        if not isinstance(select, PointFilter):
            raise TypeError(f'las_io.label_las: select must be a PointFilter, not {type(select).__name__}')
        select.for_format(h['point_format'])
    index = ops.line_index(line_segments(lines, shift), labels.half_width, device=device)
    stations = _label_stations(lines, labels, shift, device)
    total = np.zeros(len(lines) + 1, dtype=np.int64)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'wb') as f:
        f.write(chunks.head_bytes)
        for rec, m, _ in chunks:
            out, counts = label_records(rec, {**h, 'n_points': m}, index, labels, shift, select, n_lines=len(lines), stations=stations)
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
    out, counts = label_records(rec, h, index, labels, shift, select, n_lines=len(lines), stations=_label_stations(lines, labels, shift, device))
    both = torch.cat([out, counts.view(torch.uint8)]).cpu().numpy()        # the one read-back
    counts = both[len(rec):].view(np.int64)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'wb') as f:
        f.write(data[:off].tobytes())
        f.write(both[:nbytes].tobytes())
        f.write(data[off + nbytes:].tobytes())
    per_line = [int(c) for c in counts[1:]]
    return {'records': int(n), 'labelled': int(sum(per_line)), 'per_line': per_line}


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
    tail = (int(out is not None), C.c_void_p(bins.data_ptr()) if nb else None, nb)
    if _is_table(mi):
        table = _paint_rows(who, mi, stations.stations, stations.n_lines).struct()
        check(lib().lm_las_line_profile_records_local(*args[1:], survey.z_tol, C.byref(table), *tail, args[0]))
    else:
        check(lib().lm_las_line_profile_records(*args, survey.z_tol, math.nan if mi is None else mi, *tail))
    return bins


HEADER_BYTES = 375                  # the public header block of LAS 1.4, the longest there is


def tile_groups(counts, batch, binned_budget):
    """The tiles of a layout cut into groups for pass B: counts, the points of every tile (pass A); batch, the batch size; -> a list of
    (t0, t1), consecutive runs that cover 0 .. len(counts), every cut at a multiple of `batch`.  A group takes whole batches as long as
    16 * sum(counts) of its tiles stays within binned_budget (reaching it exactly is within); a batch that alone exceeds the budget is a
    group of its own.  binned_budget None: one group.  No tiles: no group."""
    counts = [int(c) for c in counts]
    T, batch = len(counts), int(batch)
    if batch < 1 or any(c < 0 for c in counts):
        raise ValueError(f'tile_groups: batch={batch} must be >= 1 and no count negative')
    if T == 0:
        return []
    if binned_budget is None:
        return [(0, T)]
    groups, t0, size = [], 0, 0
    for b0 in range(0, T, batch):
        need = 16 * sum(counts[b0:b0 + batch])
        if b0 > t0 and size + need > binned_budget:
            groups.append((t0, b0))
            t0, size = b0, 0
        size += need
    groups.append((t0, T))
    return groups


class LasChunks:
    """The point records of the LAS file `path`, `chunk_records` at a time (a positive multiple of 256).

    header          las_io.parse_header's dict, read off the first bytes of the file
    iteration       yields (records, n, first) for consecutive runs of chunk_records records, the last one shorter: records = the n
                    records from number `first` on as uint8, zero-padded to a multiple of four bytes - a tensor on `device` (uploaded
                    asynchronously from a pinned buffer), or with device=None a numpy view of the read buffer, valid until the next chunk
                    is asked for.  A file without records yields nothing.  The object may be iterated again: the file is read again
    head_bytes      the bytes before the records (header, VLRs); tail_bytes: the bytes after them (EVLRs)
    A file shorter than its header says is refused with both byte counts; more than 2^31 - 1 records are accepted."""

    def __init__(self, path, chunk_records, device=None):
        self.chunk_records = _check_chunk_records('LasChunks', chunk_records)
        self.path = os.fspath(path)
        self.device = None if device is None else torch.device(device)
        self.size = os.path.getsize(self.path)
        with open(self.path, 'rb') as f:
            head = f.read(HEADER_BYTES)
        if len(head) < 227 or head[:4] != b'LASF':
            raise LanemapHipError(f'{self.path}: not a LAS file')
        block = np.zeros(HEADER_BYTES, dtype=np.uint8)                          # a shorter header (LAS 1.0 - 1.3: 227 / 235 bytes) is padded
        block[:len(head)] = np.frombuffer(head, dtype=np.uint8)
        h = LmLasHeader()
        # (the length lm_las_parse_header checks the point data against is the file's, checked below with both numbers in the message)
        check(lib().lm_las_parse_header(C.c_void_p(block.ctypes.data), 1 << 62, C.byref(h)))
        self.header = {'version': (h.version_major, h.version_minor), 'point_format': h.point_format, 'record_len': h.record_len,
                       'n_points': h.n_points, 'offset_to_points': h.offset_to_points, 'scale': list(h.scale), 'offset': list(h.offset),
                       'min': list(h.min_xyz), 'max': list(h.max_xyz)}
        self.record_bytes = int(h.n_points) * int(h.record_len)
        expected = int(h.offset_to_points) + self.record_bytes
        if self.size < expected:
            raise LanemapHipError(f'{self.path}: truncated LAS file: {h.n_points} records of {h.record_len} B from byte {h.offset_to_points} '
                                  f'need {expected} bytes, the file has {self.size}')
        self._bufs = None

    def __len__(self):
        """The number of chunks."""
        return -(-int(self.header['n_points']) // self.chunk_records)

    @property
    def head_bytes(self):
        with open(self.path, 'rb') as f:
            return f.read(self.header['offset_to_points'])

    @property
    def tail_bytes(self):
        with open(self.path, 'rb') as f:
            f.seek(self.header['offset_to_points'] + self.record_bytes)
            return f.read()

    def _buffers(self):
        if self._bufs is None:
            cap = (min(self.chunk_records, max(int(self.header['n_points']), 1)) * self.header['record_len'] + 3) // 4 * 4
            pin = self.device is not None and self.device.type == 'cuda'
            self._bufs = [torch.empty(cap, dtype=torch.uint8, pin_memory=pin) for _ in range(2)]
        return self._bufs

    def __iter__(self):
        from concurrent.futures import ThreadPoolExecutor
        n, rl, c = int(self.header['n_points']), int(self.header['record_len']), self.chunk_records
        if n == 0:
            return
        bufs, events = self._buffers(), [None, None]

        def read(f, k):
            """Chunk k into buffer k & 1, once the last upload out of that buffer has finished."""
            slot, m = k & 1, min(c, n - k * c)
            if events[slot] is not None:
                events[slot].synchronize()
            view, nb, at = bufs[slot].numpy(), m * rl, 0
            while at < nb:
                got = f.readinto(memoryview(view)[at:nb])
                if not got:
                    raise LanemapHipError(f'{self.path}: the file ended {nb - at} bytes into chunk {k}')
                at += got
            padded = (nb + 3) // 4 * 4
            view[nb:padded] = 0
            return slot, m, padded

        with open(self.path, 'rb') as f, ThreadPoolExecutor(max_workers=1) as pool:
            f.seek(self.header['offset_to_points'])
            fut = pool.submit(read, f, 0)
            for k in range(len(self)):
                slot, m, padded = fut.result()
                if k + 1 < len(self):
                    fut = pool.submit(read, f, k + 1)
                if self.device is None:
                    yield bufs[slot].numpy()[:padded], m, k * c
                    continue
                rec = bufs[slot][:padded].to(self.device, non_blocking=True)
                if self.device.type == 'cuda':
                    events[slot] = torch.cuda.Event()
                    events[slot].record(torch.cuda.current_stream(self.device))
                yield rec, m, k * c


def empty_records(device):
    """What a file without records hands a record pass: no bytes, on the device."""
    return torch.zeros((0,), dtype=torch.uint8, device=device)


def _file_chunks(path, chunk_records, device):
    """One file as the record passes take it: -> (header, an iterable of (records on the device, header of those records)).
    chunk_records None: the file is read whole and uploaded once (_upload_records); else it goes through a LasChunks of that many records,
    every chunk under the file's header with n_points = the chunk's records.  A file without records is one empty run either way."""
    if chunk_records is None:
        data = np.fromfile(path, dtype=np.uint8)
        h = parse_header(data)
        return h, ((_upload_records(data, h, device), h) for _ in range(1))
    chunks = LasChunks(path, chunk_records, device)
    h = chunks.header
    if h['n_points'] == 0:
        return h, ((empty_records(device), h) for _ in range(1))
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
    tail = (colour.blue_q, int(out is not None), C.c_void_p(bins.data_ptr()) if nb else None, C.c_void_p(colours.data_ptr()) if nb else None, nb)
    if _is_table(mi):
        table = _paint_rows(who, mi, stations.stations, stations.n_lines).struct()
        check(lib().lm_las_line_colour_records_local(*args[1:], survey.z_tol, C.byref(table), *tail, args[0]))
    else:
        check(lib().lm_las_line_colour_records(*args, survey.z_tol, math.nan if mi is None else mi, *tail))
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
    tail = (int(out is not None), C.c_void_p(cells.data_ptr()) if n_cells else None, n_cells)
    if _is_table(_resolved(who, cross, 'paint_intensity')):
        table = _paint_rows(who, cross.paint_intensity, stations.stations, stations.n_lines, cross=True).struct(cross=True)
        check(lib().lm_las_line_cross_records_local(*args[1:], cross.z_tol, cross.lateral_q, C.byref(table), *tail, args[0]))
    else:
        check(lib().lm_las_line_cross_records(*args, cross.z_tol, cross.lateral_q, cross.paint_iq, *tail))
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


KS_COEFF = 1.95                     # sqrt(-ln(0.0005) / 2) = 1.9495: the two-sample Kolmogorov-Smirnov coefficient at alpha = 0.001
HIST_BIN = 1.0                      # the station bin hist_files cuts its tables with: the histogram rule reads rlen alone, any bin serves


def hist_records(records_u8, header, index, stations, threshold, shift=None, select=None, out=None):
    """One lm_las_line_hist_records call on the DEVICE records of a file (as profile_records takes them) against an ops.LineIndex and the
    ops.LineStations of the same segments (only their rlen column is read; L = stations.n_lines): -> hist [L, Z, NB] int64 device tensor
    (see ops.line_hist).  The records are only read; a record `select` drops contributes nothing.  out: the table of an earlier call to
    add to.  Asynchronous."""
    from . import ops
    who = 'las_io.hist_records'
    if not isinstance(threshold, PaintThreshold):
        raise TypeError(f'{who}: threshold must be a PaintThreshold, not {type(threshold).__name__}')
    if not isinstance(index, ops.LineIndex) or not isinstance(stations, ops.LineStations):
        raise TypeError(f'{who}: index must be an ops.LineIndex and stations an ops.LineStations')
    if stations.n_segments != index.n_segments:
        raise ValueError(f'{who}: stations hold {stations.n_segments} rows, the index {index.n_segments} segments')
    args, dev = _records_args(who, records_u8, header, shift, select, index, None, 'the threshold asks', threshold.half_width)
    L, Z, NB = stations.n_lines, threshold.rings, threshold.n_counts
    hist = ops._table_out(who, (L, Z, NB), out, dev)
    n_hist = L * Z * NB
    check(lib().lm_las_line_hist_records(*args[1:], stations.args()[0], L, threshold.z_tol, threshold.ring_q, threshold.bin_shift,
                                         int(out is not None), C.c_void_p(hist.data_ptr()) if n_hist else None, n_hist, args[0]))
    return hist


def hist_files(files, lines, threshold, device='cuda:0', chunk_records=None):
    """The paint / asphalt histograms of `lines` (list of [n,3] float64, LAS frame) from the LAS files `files`, a list of (path, shift,
    select): every file is read once, uploaded and goes through one lm_las_line_hist_records call with its own read offset and
    PointFilter, all into one table, which is read back once.  -> hist [L, Z, NB] int64 numpy, L = len(lines); paint_threshold(hist,
    threshold) reads the thresholds off it.  chunk_records: None, or the records of a file read and counted at a time (LasChunks)."""
    if not isinstance(threshold, PaintThreshold):
        raise TypeError(f'las_io.hist_files: threshold must be a PaintThreshold, not {type(threshold).__name__}')
    lines = list(lines)
    hist, _ = _each_file('las_io.hist_files', files, lines, HIST_BIN, threshold.half_width, device,
                         lambda rec, h, tables, shift, select, out: hist_records(rec, h, *tables, threshold, shift, select, out=out),
                         chunk_records=chunk_records)
    if hist is None:                                                        # no file: the empty table of the lines
        return np.zeros((len(lines), threshold.rings, threshold.n_counts), dtype=np.int64)
    return hist.cpu().numpy()                                               # the one read-back


def _threshold_group(A, O, threshold):
    """paint_threshold for one group: A, O the inner and outer histograms as lists of Python integers."""
    NB, sh = len(A), threshold.bin_shift
    NA, NO = sum(A), sum(O)
    a, o = [0] * (NB + 1), [0] * (NB + 1)                                   # a[T] = the inner returns of the bins >= T
    for b in range(NB - 1, -1, -1):
        a[b], o[b] = a[b + 1] + A[b], o[b + 1] + O[b]
    J = [a[T] * NO - o[T] * NA for T in range(NB)]                          # (J[0] = 0 is not a candidate)
    M = max(J[1:])
    t0 = J.index(M, 1)
    floor = M - (M >> threshold.tolerance_shift)
    lo = hi = t0
    while lo > 1 and J[lo - 1] >= floor:
        lo -= 1
    while hi < NB - 1 and J[hi + 1] >= floor:
        hi += 1
    T = (lo + hi) // 2
    D = M / (NA * NO) if NA and NO else 0.0
    supported = bool(NA >= threshold.min_returns and NO >= threshold.min_returns and M > 0
                     and D >= max(threshold.min_separation, KS_COEFF * math.sqrt((NA + NO) / (NA * NO))))
    w = 1 << sh                                                             # (one division of integers: correctly rounded)
    centre = lambda H, n: (2 * w * sum(b * c for b, c in enumerate(H)) + (w - 1) * n) / (2 * n) if n else None
    return {'threshold': float(T << sh) if supported else None, 'supported': supported, 'separation': D, 'inner_returns': NA,
            'outer_returns': NO, 'paint_share': a[T] / NA if NA else None, 'false_share': o[T] / NO if NO else None,
            'inner_mean': centre(A, NA), 'outer_mean': centre(O, NO), 'plateau': [lo << sh, hi << sh]}


def paint_threshold(hist, threshold):
    """The thresholds read off the histograms (host, Python integers and float64): hist [L, Z, NB] int64 (hist_files, ops.line_hist) ->
    {'strip': group, 'lines': {k: group}}, k = 1 .. L; the strip's group sums all lines.  For a group, with A[b] and O[b] the sums of its
    inner and outer rings (PaintThreshold) and NA, NO their totals:

      a(T), o(T)      the inner and the outer returns of the bins b >= T
      J(T)            a(T) NO - o(T) NA for T = 1 .. NB - 1: NA NO times the gap between the two populations' shares above T
      M, t0           the maximum of J and the smallest T that reaches it
      plateau         [lo << bin_shift, hi << bin_shift] of the largest contiguous run [lo, hi] around t0 with J >= M - (M >> tolerance_shift)
      T*              (lo + hi) // 2; threshold = float(T* << bin_shift) - None unless the group is supported
      separation      D = M / (NA NO), in 0 .. 1 (0.0 without inner or outer returns)
      supported       NA >= min_returns, NO >= min_returns, M > 0 and D >= max(min_separation, KS_COEFF sqrt((NA + NO) / (NA NO))): the
                      inner returns ARE brighter than the outer ones.  An unsupported line has no paint under it that the data shows
      inner_returns, outer_returns   NA, NO
      paint_share, false_share       a(T*) / NA, o(T*) / NO: the inner returns that are paint, the outer ones that pass for it (None
                                     where the count is 0)
      inner_mean, outer_mean         the mean intensities, taken at the bin centres (b << bin_shift) + ((1 << bin_shift) - 1) / 2 (None
                                     where the count is 0)"""
    if not isinstance(threshold, PaintThreshold):
        raise TypeError(f'paint_threshold: threshold must be a las_io.PaintThreshold, not {type(threshold).__name__}')
    hist = np.asarray(hist)
    Z, NB = threshold.rings, threshold.n_counts
    if hist.ndim != 3 or hist.dtype != np.int64 or hist.shape[1:] != (Z, NB) or (hist < 0).any():
        raise ValueError(f'paint_threshold: hist must be an [L, {Z}, {NB}] int64 table of counts, not {hist.dtype} {hist.shape}')
    inner = hist[:, threshold.inner_rings, :].sum(axis=1)                   # [L, NB]; 2^31 returns per file stay far inside 64 bits
    outer = hist[:, threshold.outer_rings, :].sum(axis=1)
    group = lambda A, O: _threshold_group([int(v) for v in A], [int(v) for v in O], threshold)
    return {'strip': group(inner.sum(axis=0), outer.sum(axis=0)), 'lines': {k + 1: group(inner[k], outer[k]) for k in range(len(hist))}}


SOURCES = ('window', 'line', 'strip')            # PaintTable.source: whose group a row's threshold was read off


class PaintTable(_Table):
    """A paint threshold per line or per station window along every line (immutable): what paint_table reads off the windowed
    histograms, and what MarkingLabels.min_intensity, MarkingSurvey.min_intensity, CrossSection.paint_intensity and
    PaintResidue.min_intensity take wherever they take a number or 'auto'.  The stages then look the value up for every return on the GPU
    (the rule: include/lanemap_hip.h).

      thr         float32 [R], every value finite: the threshold of every row
      win_start   int32 [L + 1], a CSR table from 0, not descending, ending in R: line k (from 1) owns the rows win_start[k-1] ..
                  win_start[k] - 1, its station windows in order - line_stations(lines, shift, bin=window)'s bin_start
      window      metres (finite, > 0): the length of a window.  One row per line with a window longer than every line is
                  PaintThreshold's scope='line': the same table, not a second code path
      source      uint8 [R]: 0 the window's own group gave the threshold, 1 the line's, 2 the strip's (SOURCES)
    The arrays are copied and read-only; two tables are equal when all four hold the same values."""
    __slots__ = ('thr', 'win_start', 'window', 'source')

    def __init__(self, thr, win_start, window, source=None):
        thr = np.array(thr, dtype=np.float32, order='C', copy=True)
        ws = np.array(win_start, order='C', copy=True)
        if thr.ndim != 1 or not np.isfinite(thr).all():
            raise ValueError(f'PaintTable: thr must be a [R] array of finite numbers, not {thr.shape}' + ('' if thr.ndim != 1 else ' with a '
                             'value that is not finite'))
        if ws.ndim != 1 or len(ws) < 1 or ws.dtype.kind not in 'iu' or ws[0] != 0 or (np.diff(ws.astype(np.int64)) < 0).any() \
                or int(ws[-1]) != len(thr):
            raise ValueError(f'PaintTable: win_start must be a [L + 1] table of whole numbers from 0, not descending, ending in R={len(thr)}, '
                             f'not {ws.tolist() if ws.ndim == 1 and len(ws) < 8 else ws.shape}')
        if not _number(window) or not (0.0 < float(window) < math.inf):
            raise ValueError(f'PaintTable: window={window!r} must be a finite length > 0')
        src = np.zeros(len(thr), np.uint8) if source is None else np.array(source, order='C', copy=True)
        if src.shape != thr.shape or src.dtype.kind not in 'iu' or (src.astype(np.int64) > 2).any() or (src.astype(np.int64) < 0).any():
            raise ValueError(f'PaintTable: source must be a [R={len(thr)}] array of 0 (window), 1 (line), 2 (strip), not {src.shape} {src.dtype}')
        ws, src = ws.astype(np.int32), src.astype(np.uint8)
        for a in (thr, ws, src):
            a.setflags(write=False)
        self._set(thr=thr, win_start=ws, window=float(window), source=src)

    def _key(self):
        return (self.thr.tobytes(), self.win_start.tobytes(), self.window, self.source.tobytes())

    def __eq__(self, other):
        return type(other) is type(self) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f'PaintTable(thr={self.thr.tolist()!r}, win_start={self.win_start.tolist()!r}, window={self.window!r}, source={self.source.tolist()!r})'


def save_paint_table(path, table):
    """A PaintTable as one float64 array [4, max(R, L + 1)] in a .npy file: row 0 thr, row 1 source, row 2 win_start, row 3 the window
    length, each padded with NaN (float64 holds every value exactly)."""
    R, n = len(table.thr), len(table.win_start)
    a = np.full((4, max(R, n)), np.nan)
    a[0, :R], a[1, :R], a[2, :n], a[3, 0] = table.thr, table.source, table.win_start, table.window
    np.save(path, a)


def load_paint_table(path):
    """-> the PaintTable save_paint_table wrote."""
    a = np.load(path)
    n = int(np.isfinite(a[2]).sum())
    R = int(a[2, n - 1])
    return PaintTable(a[0, :R].astype(np.float32), a[2, :n].astype(np.int32), float(a[3, 0]), a[1, :R].astype(np.uint8))


def threshold_window(lines, shift, threshold):
    """The window length a PaintThreshold's scope cuts the lines with, metres: threshold.window for 'window'; for 'line' (and 'strip') a
    length beyond every line in the frame of `shift` - twice the longest, at least 1 m - so that every line owns one row."""
    if threshold.scope == 'window':
        return threshold.window
    seg = line_segments(lines, shift)
    if not len(seg):
        return 1.0
    of_line = np.ascontiguousarray(seg[:, 7]).view(np.int32)
    d = seg[:, 3:5].astype(np.float64)
    total = np.bincount(of_line, weights=np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]))
    return max(1.0, 2.0 * float(total.max()))


def hist_window_records(records_u8, header, index, stations, threshold, shift=None, select=None, out=None):
    """One lm_las_line_hist_window_records call on the DEVICE records of a file, as hist_records: -> hist [R, Z, NB] int64 device tensor,
    a histogram per station window of every line and lateral ring (the rule: include/lanemap_hip.h).  stations: the ops.LineStations cut
    with bin = the window length - its bin_start is the table of the windows, R = stations.n_bins.  out: the table of an earlier call to
    add to.  Asynchronous."""
    from . import ops
    who = 'las_io.hist_window_records'
    if not isinstance(threshold, PaintThreshold):
        raise TypeError(f'{who}: threshold must be a PaintThreshold, not {type(threshold).__name__}')
    if not isinstance(index, ops.LineIndex) or not isinstance(stations, ops.LineStations):
        raise TypeError(f'{who}: index must be an ops.LineIndex and stations an ops.LineStations')
    if stations.n_segments != index.n_segments:
        raise ValueError(f'{who}: stations hold {stations.n_segments} rows, the index {index.n_segments} segments')
    args, dev = _records_args(who, records_u8, header, shift, select, index, None, 'the threshold asks', threshold.half_width)
    st, ws, ws_host, L, window = stations.args()
    R, Z, NB = stations.n_bins, threshold.rings, threshold.n_counts
    hist = ops._table_out(who, (R, Z, NB), out, dev)
    n_hist = R * Z * NB
    check(lib().lm_las_line_hist_window_records(*args[1:], st, L, threshold.z_tol, threshold.ring_q, threshold.bin_shift, int(out is not None),
                                                C.c_void_p(hist.data_ptr()) if n_hist else None, n_hist, ws, ws_host, window, args[0]))
    return hist


def hist_window_files(files, lines, threshold, window=None, device='cuda:0', chunk_records=None):
    """hist_files with a histogram per station window: every file of `files`, a list of (path, shift, select), is read once and goes through
    one lm_las_line_hist_window_records call per file (or chunk, chunk_records as for hist_files) into one table, which is read back once.
    window: the window length in metres; None: threshold_window(lines, the first file's shift, threshold) - threshold.window for
    scope='window', one window per line otherwise.  The windows each line owns are those of the first file's frame, as the bins of
    survey_files.  -> (hist [R, Z, NB] int64 numpy, win_start [L + 1] int32 numpy, window); summed over the windows of a line it is
    hist_files' table."""
    if not isinstance(threshold, PaintThreshold):
        raise TypeError(f'las_io.hist_window_files: threshold must be a PaintThreshold, not {type(threshold).__name__}')
    lines, files = list(lines), list(files)
    if window is None:
        window = threshold_window(lines, files[0][1] if files else None, threshold)
    hist, win_start = _each_file('las_io.hist_window_files', files, lines, window, threshold.half_width, device,
                                 lambda rec, h, tables, shift, select, out: hist_window_records(rec, h, *tables, threshold, shift, select, out=out),
                                 chunk_records=chunk_records)
    if hist is None:                                                        # no file: the empty table of the lines
        return np.zeros((int(win_start[-1]), threshold.rings, threshold.n_counts), dtype=np.int64), win_start, float(window)
    return hist.cpu().numpy(), win_start, float(window)                      # the one read-back


def line_hist_of_windows(hist_w, win_start):
    """The per-line table [L, Z, NB] of a windowed one [R, Z, NB]: the sum of every line's windows - hist_files' table."""
    hist_w, ws = np.asarray(hist_w), np.asarray(win_start, dtype=np.int64)
    out = np.zeros((len(ws) - 1,) + hist_w.shape[1:], dtype=np.int64)
    for k in range(len(ws) - 1):
        out[k] = hist_w[ws[k]:ws[k + 1]].sum(axis=0)
    return out


def paint_table(hist_w, win_start, threshold, window=None):
    """The paint table read off the windowed histograms (host, Python integers and float64): hist_w [R, Z, NB] int64 and win_start [L + 1]
    (hist_window_files) -> (PaintTable, {'strip': group, 'lines': {k: group}, 'windows': {k: [group, ...]}}).  _threshold_group, unchanged,
    on three kinds of group: every window; every line, the sum of its windows; the strip, the sum of all.  thr[row] is the window's
    threshold where its group is supported, else its line's where that is supported, else the strip's - PaintTable.source says which (0,
    1, 2).  A strip that is not supported is a ValueError, as it is where 'auto' asks for the strip's one number.  No smoothing between
    neighbouring windows.  window: the window length the table was cut with; None: threshold.window."""
    if not isinstance(threshold, PaintThreshold):
        raise TypeError(f'paint_table: threshold must be a las_io.PaintThreshold, not {type(threshold).__name__}')
    hist_w, ws = np.asarray(hist_w), np.asarray(win_start)
    Z, NB = threshold.rings, threshold.n_counts
    if hist_w.ndim != 3 or hist_w.dtype != np.int64 or hist_w.shape[1:] != (Z, NB) or (hist_w < 0).any():
        raise ValueError(f'paint_table: hist_w must be an [R, {Z}, {NB}] int64 table of counts, not {hist_w.dtype} {hist_w.shape}')
    if ws.ndim != 1 or len(ws) < 1 or ws[0] != 0 or (np.diff(ws.astype(np.int64)) < 0).any() or int(ws[-1]) != len(hist_w):
        raise ValueError(f'paint_table: win_start must be a CSR table from 0 ending in R={len(hist_w)}, not {ws.tolist() if len(ws) < 8 else ws.shape}')
    inner = hist_w[:, threshold.inner_rings, :].sum(axis=1)                 # [R, NB]
    outer = hist_w[:, threshold.outer_rings, :].sum(axis=1)
    group = lambda A, O: _threshold_group([int(v) for v in A], [int(v) for v in O], threshold)
    strip = group(inner.sum(axis=0), outer.sum(axis=0))
    lines, windows = {}, {}
    for k in range(len(ws) - 1):
        a, b = int(ws[k]), int(ws[k + 1])
        lines[k + 1] = group(inner[a:b].sum(axis=0), outer[a:b].sum(axis=0))
        windows[k + 1] = [group(inner[r], outer[r]) for r in range(a, b)]
    found = {'strip': strip, 'lines': lines, 'windows': windows}
    if not strip['supported'] and len(hist_w):
        raise ValueError(f"paint_table: the strip's returns support no threshold between asphalt and paint: separation "
                         f"{strip['separation']:.4f} with {strip['inner_returns']} returns on the lines and {strip['outer_returns']} beside them")
    thr, source = np.zeros(len(hist_w), np.float32), np.zeros(len(hist_w), np.uint8)
    for k in range(len(ws) - 1):
        for j, g in enumerate(windows[k + 1]):
            src = 0 if g['supported'] else 1 if lines[k + 1]['supported'] else 2
            thr[int(ws[k]) + j] = (g, lines[k + 1], strip)[src]['threshold']
            source[int(ws[k]) + j] = src
    return PaintTable(thr, ws, threshold.window if window is None else window, source), found


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
        clouds = (pts for path, _, select in files for pts in decode_chunks(LasChunks(path, chunk_records, device), frame, select))
    mi = residue.min_intensity
    if _is_table(mi):                       # the rows are looked up with the station table of the index' own segments, in its frame
        st = ops.line_stations(*line_stations(lines, frame, mi.window), mi.window, device=device)
        mi = _paint_rows('las_io.residue_files', mi, st.stations, len(lines))
    out = ops.paint_residue(clouds, index, residue.z_tol, mi, residue.clear, residue.cell, residue.connectivity).numpy()
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
