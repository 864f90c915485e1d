"""Numpy restatement of the marking profile rule (include/lanemap_hip.h, csrc/profile.hip) for the tests: the host tables with plain
loops, the per-point terms in float32 on top of label_ref.label_f32's winner - brute force over all segments, no grid -, the integer
accumulation, a pruned form for clouds of millions of points, and a float64 checker of las_io.marking_summary.

The float32 expressions round after every operation like the kernels built without contraction."""
import math

import numpy as np

import label_ref as lr

f32 = np.float32
Q_EMPTY_MIN, Q_EMPTY_MAX = 2 ** 31 - 1, -2 ** 31


def stations_ref(seg, n_lines, bin):
    """The rule's host tables from the [S,8] segment table: -> (stations [S,4] float32, bin_start [n_lines + 1] int32)."""
    lines = lr.seg_lines(seg)
    st = np.zeros((len(seg), 4), f32)
    total = [0.0] * (n_lines + 1)
    has = [False] * (n_lines + 1)
    for s in range(len(seg)):
        k = int(lines[s])
        dx, dy = float(seg[s, 3]), float(seg[s, 4])
        len64 = math.sqrt(dx * dx + dy * dy)
        st[s, 0], st[s, 1], st[s, 2] = f32(total[k]), f32(len64), f32(1.0 / len64) if len64 != 0 else f32(0)
        total[k] += len64
        has[k] = True
    bin_start = [0]
    for k in range(1, n_lines + 1):
        bin_start.append(bin_start[-1] + (max(1, int(math.ceil(total[k] / float(bin)))) if has[k] else 0))
    return st, np.asarray(bin_start, np.int32)


def point_terms(pts, seg, stations, bin_start, bin, line, win):
    """The rule's terms of every point from its label and winning segment: -> dict of t, st (float32), b (the bin inside the line), B (the
    absolute bin, -1 without a label), q, iq (int64)."""
    pts, seg, stations = np.asarray(pts, f32), np.asarray(seg, f32), np.asarray(stations, f32)
    N = len(pts)
    on = np.asarray(line) > 0
    s = np.where(on, win, 0)
    if len(seg) == 0:
        z = np.zeros(N, np.int64)
        return {'t': np.zeros(N, f32), 'st': np.zeros(N, f32), 'b': z, 'B': z - 1, 'q': z, 'iq': z}
    ax, ay, dx, dy, inv = (seg[s, k] for k in (0, 1, 3, 4, 6))
    s0, ln, rlen = (stations[s, k] for k in range(3))
    inv_bin = f32(1.0 / float(bin))
    bs = np.asarray(bin_start, np.int64)
    k = np.where(on, line, 1).astype(np.int64)
    base, nb = bs[k - 1], bs[k] - bs[k - 1]
    with np.errstate(all='ignore'):
        px, py = pts[:, 0] - ax, pts[:, 1] - ay
        t = np.fmin(np.fmax((px * dx + py * dy) * inv, f32(0)), f32(1))
        st = s0 + t * ln
        b = np.minimum(np.trunc(st * inv_bin).astype(np.int64), nb - 1)
        o = (dx * py - dy * px) * rlen
        q = np.rint(o * f32(1024)).astype(np.int64)
        iq = np.fmin(np.fmax(np.rint(pts[:, 3]), f32(0)), f32(65535)).astype(np.int64)
    assert st.dtype == f32 and o.dtype == f32
    B = np.where(on, base + b, -1)
    return {'t': np.where(on, t, f32(0)), 'st': np.where(on, st, f32(0)), 'b': np.where(on, b, 0), 'B': B, 'q': np.where(on, q, 0),
            'iq': np.where(on, iq, 0)}


def accumulate(terms, n_bins, bins=None):
    """The integer accumulation: -> bins [n_bins, 6] int64 (n, sum iq, sum q, sum q^2, min q, max q); bins: what to add to."""
    if bins is None:
        bins = np.zeros((n_bins, 6), np.int64)
        bins[:, 4], bins[:, 5] = Q_EMPTY_MIN, Q_EMPTY_MAX
    else:
        bins = np.array(bins, np.int64, copy=True)
    on = terms['B'] >= 0
    B, q, iq = terms['B'][on], terms['q'][on], terms['iq'][on]
    np.add.at(bins[:, 0], B, 1)
    np.add.at(bins[:, 1], B, iq)
    np.add.at(bins[:, 2], B, q)
    np.add.at(bins[:, 3], B, q * q)
    np.minimum.at(bins[:, 4], B, q)
    np.maximum.at(bins[:, 5], B, q)
    return bins


def profile_f32(pts, seg, stations, bin_start, bin, half_width, z_tol, min_intensity=None, mask=None, line_tie=True, bins=None):
    """The whole rule by brute force: -> (bins, terms, line, win)."""
    line, _, win = lr.label_f32(pts, seg, half_width, z_tol, min_intensity, mask=mask, line_tie=line_tie)
    terms = point_terms(pts, seg, stations, bin_start, bin, line, win)
    return accumulate(terms, int(bin_start[-1]), bins), terms, line, win


def winner_f32_pruned(pts, seg, half_width, z_tol, min_intensity=None, mask=None):
    """label_ref.label_f32_pruned that also keeps the winning segment: the same float32 expression per (point, segment) pair, evaluated
    only for the points in the segment's bounding box widened by 2 half_width + 1 mm.  -> (line, win)."""
    pts, seg = np.asarray(pts, f32), np.asarray(seg, f32)
    N = len(pts)
    line, best, win = np.zeros(N, np.int32), np.full(N, lr.INF32), np.full(N, -1, np.int64)
    ok = lr.eligible(pts, min_intensity)
    if mask is not None:
        ok &= mask
    order = np.argsort(pts[:, 0], kind='stable')
    xs = pts[order, 0].astype(np.float64)
    xs = np.where(np.isnan(xs), np.inf, xs)
    hw2, zt, lines = f32(half_width) * f32(half_width), f32(z_tol), lr.seg_lines(seg)
    r = 2.0 * float(half_width) + 1e-3
    with np.errstate(all='ignore'):
        for s in range(len(seg)):
            ax, ay, az, dx, dy, dz, inv = (seg[s, k] for k in range(7))
            x0, x1 = min(float(ax), float(ax) + float(dx)) - r, max(float(ax), float(ax) + float(dx)) + r
            y0, y1 = min(float(ay), float(ay) + float(dy)) - r, max(float(ay), float(ay) + float(dy)) + r
            idx = order[np.searchsorted(xs, x0, 'left'):np.searchsorted(xs, x1, 'right')]
            idx = idx[(pts[idx, 1] >= y0) & (pts[idx, 1] <= y1) & ok[idx]]
            if not len(idx):
                continue
            px, py = pts[idx, 0] - ax, pts[idx, 1] - ay
            t = np.fmin(np.fmax((px * dx + py * dy) * inv, f32(0)), f32(1))
            ex, ey = px - t * dx, py - t * dy
            d2 = ex * ex + ey * ey
            hit = (d2 <= hw2) & (np.abs(pts[idx, 2] - (az + t * dz)) <= zt)
            take = hit & ((d2 < best[idx]) | ((d2 == best[idx]) & (lines[s] < line[idx])))
            best[idx[take]], line[idx[take]], win[idx[take]] = d2[take], lines[s], s
    return line, win


def profile_f32_pruned(pts, seg, stations, bin_start, bin, half_width, z_tol, min_intensity=None, mask=None):
    line, win = winner_f32_pruned(pts, seg, half_width, z_tol, min_intensity, mask)
    terms = point_terms(pts, seg, stations, bin_start, bin, line, win)
    return accumulate(terms, int(bin_start[-1])), terms, line, win


# ---------------------------------------------------------------------------------------------------------------- the summary
def summary(bins, bin_start, bin, min_points, max_gap, solid_cover):
    """What las_io.marking_summary must return, with plain loops in float64: one dict per line."""
    out = []
    for k in range(len(bin_start) - 1):
        rows = [tuple(int(v) for v in r) for r in np.asarray(bins)[int(bin_start[k]):int(bin_start[k + 1])]]
        nb = len(rows)
        on = [r[0] >= min_points for r in rows]
        runs, i = [], 0
        while i < nb:                                        # maximal runs of painted bins
            if on[i]:
                j = i
                while j + 1 < nb and on[j + 1]:
                    j += 1
                runs.append([i, j])
                i = j + 1
            else:
                i += 1
        joined = []
        for a, b in runs:                                    # holes of at most max_gap metres are closed
            if joined and (a - joined[-1][1] - 1) * bin <= max_gap + 1e-9 * bin:
                joined[-1][1] = b
            else:
                joined.append([a, b])
        painted = sum(on)
        cover = painted / nb if nb else 0.0
        lens = sorted((b - a + 1) * bin for a, b in joined)
        gaps = sorted((joined[j + 1][0] - joined[j][1] - 1) * bin for j in range(len(joined) - 1))
        med = lambda v: None if not v else (v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]))
        widths = sorted((r[5] - r[4]) / 1024.0 for r, o in zip(rows, on) if o)
        n_sum, i_sum = sum(r[0] for r, o in zip(rows, on) if o), sum(r[1] for r, o in zip(rows, on) if o)
        kind = 'solid' if nb and cover >= solid_cover else 'dashed' if len(joined) >= 2 else 'none' if not joined else 'partial'
        out.append({'length': nb * bin, 'painted': painted, 'runs': [[a * bin, (b + 1) * bin] for a, b in joined], 'cover': cover,
                    'type': kind, 'dash': med(lens), 'gap': med(gaps), 'width': med(widths), 'intensity': i_sum / n_sum if painted else None})
    return out


def summary_of(bins, bin_start, survey):
    return summary(bins, bin_start, survey.bin, survey.min_points, survey.max_gap, survey.solid_cover)


# ---------------------------------------------------------------------------------------------------------------- the scene
BIN_EXACT, BIN_INEXACT = 0.125, 0.1          # 0.125 is a float32 and every border k * 0.125 is one; 0.1 is not
ENDS = (25, 26, 27, 28)                      # label_ref.scene_points: (-0.1, 2), (40.1, 2), (0, 2), (40, 2) around the ends of line 1
BORDER, LEFT, RIGHT = 0, 1, 2                # the points added here, counted from the end of label_ref's scene


def scene_points(seg, grid=None):
    """label_ref.scene_points followed by three points of this rule's own: one with st exactly on a bin border of line 1 (x = 1: t = 0.5
    on the first segment, st = 1.0 = 8 bins of 0.125), one 0.1 m left and one 0.1 m right of line 1 in a bin of their own part of the
    line.  -> ([N,4] float32, index of the first added point)."""
    base = lr.scene_points(seg, grid)
    extra = np.asarray([(1.0, 2.0, 0.01, 1000.0), (5.0, 2.1, 0.05, 1200.0), (5.0, 1.9, 0.05, 800.0)], f32)
    return np.concatenate([base, extra]), len(base)


def check_scene(terms, line, win, first, bin_start, bin):
    """The reference puts the special points where the rule says (bin = BIN_EXACT)."""
    assert bin == BIN_EXACT
    nb1 = int(bin_start[1] - bin_start[0])
    assert nb1 == 320 and int(bin_start[0]) == 0                                          # line 1: 40 m
    i = first + BORDER
    assert line[i] == 1 and win[i] == 0 and terms['t'][i] == f32(0.5) and terms['st'][i] == f32(1.0) and terms['b'][i] == 8, 'upper bin'
    before, at_start, at_end = ENDS[0], ENDS[2], ENDS[3]
    past = ENDS[1]
    assert line[before] == 1 and terms['t'][before] == 0 and terms['b'][before] == 0, 'before the start: t clamps to 0'
    assert line[at_start] == 1 and terms['b'][at_start] == 0
    assert line[past] == 1 and terms['t'][past] == 1 and terms['st'][past] == f32(40.0) and terms['b'][past] == nb1 - 1, 'past the end'
    assert line[at_end] == 1 and terms['t'][at_end] == 1 and terms['b'][at_end] == nb1 - 1, 'st / bin = 320 is clamped to the last bin'
    assert line[first + LEFT] == 1 and terms['q'][first + LEFT] == 102 and line[first + RIGHT] == 1 and terms['q'][first + RIGHT] == -102
    assert terms['B'][first + LEFT] == terms['B'][first + RIGHT] == 40
    sv = lr.SHARED_VERTEX
    assert line[sv] == 1 and win[sv] == 2 and terms['t'][sv] == 1 and terms['st'][sv] == f32(6.0) and terms['b'][sv] == 48 and terms['q'][sv] == 0
    tr = lr.TRIPLE
    assert line[tr] == 5 and terms['q'][tr] == 0 and terms['t'][tr] == 0 and terms['B'][tr] == int(bin_start[4]), 'the doubled vertex'
