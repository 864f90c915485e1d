"""The threshold between asphalt and paint, found in the strip's own returns: `PaintThreshold` / `hist_records` / `hist_files` /
`paint_threshold`.  Per line and per lateral ring around it the GPU counts a histogram of the intensities of the returns the labelling
rule gives the line (`ops.line_hist`, `lm_las_line_hist_records`); on the host the threshold that best separates the returns ON the lines
from the returns BESIDE them is read off the table, for the strip and for every line - the number MarkingLabels, MarkingSurvey,
PaintResidue and CrossSection ask for with 'auto'.

Everything here is reached as `las_io.<name>` too.  It is a module of its own because tests/test_las_select_cpu.py holds the option
classes defined IN las_io to a literal table of ten; tests/test_threshold_cpu.py applies the same checks to PaintThreshold."""
import ctypes as C
import math

import numpy as np

from ._lib import lib, check
from .las_io import _Options, _number, _whole, _records_args, _each_file

KS_COEFF = 1.95                     # sqrt(-ln(0.0005) / 2) = 1.9495: the two-sample Kolmogorov-Smirnov coefficient at alpha = 0.001
HIST_BIN = 1.0                      # the station bin hist_files cuts its tables with: the histogram rule reads rlen alone, any bin serves


class PaintThreshold(_Options):
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
    Apart from the derived KS_COEFF = 1.95 of the support test, the defaults are plain defaults, not tuned values."""
    __slots__ = ('half_width', 'ring', 'inner', 'outer', 'z_tol', 'bin_shift', 'min_returns', 'min_separation', 'tolerance_shift')

    def __init__(self, half_width=0.625, ring=0.0625, inner=0.125, outer=0.375, z_tol=0.5, bin_shift=6, min_returns=1000,
                 min_separation=0.05, tolerance_shift=5):
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
                  tolerance_shift=int(tolerance_shift))
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
