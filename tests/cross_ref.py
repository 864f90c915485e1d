"""Numpy restatement of the cross-section rule (include/lanemap_hip.h, csrc/profile.hip) for the tests: the table by brute force on top of
label_ref.label_f32's winner and profile_ref.point_terms, accumulated with np.add.at into int64, and las_io.cross_summary /
las_io.snap_lines restated independently with plain loops and exact fractions.

The float32 expressions round after every operation like the kernels built without contraction."""
import math
from fractions import Fraction

import numpy as np

import label_ref as lr
import profile_ref as pr

f32 = np.float32


def hq_nl(half_width, lateral_q):
    hq = int(math.ceil(float(f32(half_width)) * 1024.0))
    return hq, 2 * hq // int(lateral_q) + 1


def cross_terms(pts, seg, stations, bin_start, bin, half_width, lateral_q, line, win):
    """The rule's terms of every point from its label and winning segment: profile_ref.point_terms plus c, zq (int64) and row (the
    absolute row of the table, -1 without a label)."""
    pts, seg = np.asarray(pts, f32), np.asarray(seg, f32)
    terms = pr.point_terms(pts, seg, stations, bin_start, bin, line, win)
    hq, nl = hq_nl(half_width, lateral_q)
    on = terms['B'] >= 0
    N = len(pts)
    if len(seg) == 0:
        z = np.zeros(N, np.int64)
        return {**terms, 'c': z, 'zq': z, 'row': z - 1}
    s = np.where(on, win, 0)
    az, dz = seg[s, 2], seg[s, 5]
    with np.errstate(all='ignore'):
        zl = az + terms['t'] * dz
        d = (pts[:, 2] - zl) * f32(1024)
        assert d.dtype == f32
        zq = np.rint(np.where(on, d, f32(0))).astype(np.int64)
    u = np.clip(terms['q'] + hq, 0, 2 * hq)
    c = u // int(lateral_q)
    return {**terms, 'c': np.where(on, c, 0), 'zq': np.where(on, zq, 0), 'row': np.where(on, terms['B'] * nl + c, -1)}


def accumulate(terms, n_bins, nl, paint_iq, cells=None):
    """The integer accumulation: -> cells [n_bins, nl, 4] int64 (n, n_paint, sum iq, sum zq); cells: what to add to."""
    flat = np.zeros((n_bins * nl, 4), np.int64) if cells is None else np.array(cells, np.int64, copy=True).reshape(n_bins * nl, 4)
    on = terms['row'] >= 0
    row, iq, zq = terms['row'][on], terms['iq'][on], terms['zq'][on]
    np.add.at(flat[:, 0], row, 1)
    np.add.at(flat[:, 1], row, (iq >= paint_iq).astype(np.int64))
    np.add.at(flat[:, 2], row, iq)
    np.add.at(flat[:, 3], row, zq)
    return flat.reshape(n_bins, nl, 4)


def cross_f32(pts, seg, stations, bin_start, bin, half_width, z_tol, lateral_q, paint_iq, mask=None, cells=None, pruned=False):
    """The whole rule by brute force (no min_intensity: every finite return counts): -> (cells, terms, line, win).  pruned: the winner
    from profile_ref.winner_f32_pruned, for clouds of millions of points."""
    if pruned:
        line, win = pr.winner_f32_pruned(pts, seg, half_width, z_tol, None, mask)
    else:
        line, _, win = lr.label_f32(pts, seg, half_width, z_tol, None, mask=mask)
    terms = cross_terms(pts, seg, stations, bin_start, bin, half_width, lateral_q, line, win)
    return accumulate(terms, int(bin_start[-1]), hq_nl(half_width, lateral_q)[1], paint_iq, cells), terms, line, win


# ---------------------------------------------------------------------------------------------------------------- the host policy
def _med(v):
    v = sorted(v)
    if not v:
        return None
    h = len(v) // 2
    return float(v[h]) if len(v) % 2 else 0.5 * (v[h - 1] + v[h])


def station_stripes(row, hq, lq, min_points, paint_share, max_hole, min_stripe):
    """One station's cells [nl, 4] -> (stripes as (left edge, right edge) in metres, indices of the known cells)."""
    nl = len(row)
    share = Fraction(paint_share)
    known = [int(row[c][0]) >= min_points for c in range(nl)]
    painted = [known[c] and Fraction(int(row[c][1])) >= share * int(row[c][0]) for c in range(nl)]
    filled = list(painted)
    c = 0
    while c < nl:                                            # runs of unknown cells between two painted ones
        if not known[c]:
            e = c
            while e + 1 < nl and not known[e + 1]:
                e += 1
            if c > 0 and e + 1 < nl and painted[c - 1] and painted[e + 1] and e - c + 1 <= max_hole:
                for j in range(c, e + 1):
                    filled[j] = True
            c = e + 1
        else:
            c += 1
    stripes, c = [], 0
    while c < nl:
        if filled[c]:
            e = c
            while e + 1 < nl and filled[e + 1]:
                e += 1
            if Fraction((e - c + 1) * lq, 1024) >= Fraction(min_stripe):
                stripes.append(((c * lq - hq) / 1024.0, ((e + 1) * lq - hq) / 1024.0))
            c = e + 1
        else:
            c += 1
    return stripes, [c for c in range(nl) if known[c]]


def crossfall_of(row, idx, hq, lq):
    """The n-weighted least-squares slope of sum zq / n / 1024 against the cell-centre offset, as one exact fraction rounded once."""
    x = [Fraction((2 * c + 1) * lq - 2 * hq, 2048) for c in idx]
    w = [int(row[c][0]) for c in idx]
    y = [Fraction(int(row[c][3]), 1024 * int(row[c][0])) for c in idx]
    W = sum(w)
    xm, ym = sum(a * b for a, b in zip(w, x)) / W, sum(a * b for a, b in zip(w, y)) / W
    return float(sum(a * (b - xm) * (c - ym) for a, b, c in zip(w, x, y)) / sum(a * (b - xm) ** 2 for a, b in zip(w, x)))


def summary(cells, bin_start, half_width, lateral_q, min_points, paint_share, max_hole, min_stripe):
    hq, nl = hq_nl(half_width, lateral_q)
    cells = np.asarray(cells)
    out = []
    for k in range(len(bin_start) - 1):
        st, falls = [], []
        for i in range(int(bin_start[k]), int(bin_start[k + 1])):
            stripes, idx = station_stripes(cells[i], hq, lateral_q, min_points, paint_share, max_hole, min_stripe)
            st.append(stripes)
            if len(idx) >= 3:
                falls.append(crossfall_of(cells[i], idx, hq, lateral_q))
        counts = [len(s) for s in st]
        best = None
        for cnt in sorted(set(c for c in counts if c)):      # ascending: a tie stays with the smaller
            if best is None or counts.count(cnt) > counts.count(best):
                best = cnt
        typ = [s for s in st if s and len(s) == best]
        out.append({'stations': sum(1 for c in counts if c), 'stripes': best, 'double': best == 2,
                    'width': _med([b - a for s in typ for a, b in s]),
                    'separation': _med([s[1][0] - s[0][1] for s in typ]) if best == 2 else None,
                    'extent': _med([s[-1][1] - s[0][0] for s in typ]),
                    'offset': _med([0.5 * (s[0][0] + s[-1][1]) for s in typ]),
                    'crossfall': _med(falls),
                    'centres': [0.5 * (s[0][0] + s[-1][1]) if s else None for s in st],
                    'counts': counts})
    return out


def summary_of(cells, bin_start, cross):
    return summary(cells, bin_start, cross.half_width, cross.lateral_q, cross.min_points, cross.paint_share, cross.max_hole, cross.min_stripe)


def snap(lines, summ, bin_start, bin, smooth, min_stations, max_shift):
    """las_io.snap_lines with plain loops."""
    out = []
    for k, line in enumerate(lines):
        line = np.asarray(line, np.float64)
        new = line.copy()
        m = summ[k]
        s = [0.0]
        for v in range(1, len(line)):
            s.append(s[-1] + math.sqrt((line[v, 0] - line[v - 1, 0]) ** 2 + (line[v, 1] - line[v - 1, 1]) ** 2))
        for v in range(len(line)):
            if len(line) < 2 or m['stripes'] is None:
                break
            near = [m['centres'][i] for i in range(len(m['centres']))
                    if m['centres'][i] is not None and m['counts'][i] == m['stripes'] and abs((i + 0.5) * bin - s[v]) <= smooth / 2]
            if len(near) < min_stations:
                continue
            shift = _med(near)
            if abs(shift) > max_shift:
                continue
            normal = np.zeros(2)
            for step, stop in ((-1, -1), (1, len(line) - 1)):            # the nearest segment of non-zero length on either side
                j = v - 1 if step < 0 else v
                while j != stop:
                    dx, dy = line[j + 1, 0] - line[j, 0], line[j + 1, 1] - line[j, 1]
                    ln = math.sqrt(dx * dx + dy * dy)
                    if ln > 0:
                        normal += np.array([-dy / ln, dx / ln])
                        break
                    j += step
            norm = math.sqrt(normal[0] ** 2 + normal[1] ** 2)
            if norm > 0:
                new[v, :2] = line[v, :2] + shift * normal / norm
        out.append(new)
    return out


def snap_of(lines, summ, bin_start, cross):
    return snap(lines, summ, bin_start, cross.bin, cross.smooth, cross.min_stations, cross.max_shift)
