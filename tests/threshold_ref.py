"""Restatement of the paint / asphalt histogram rule (include/lanemap_hip.h, csrc/profile.hip: hist_cell) and of the threshold policy
(las_io.paint_threshold) for the tests: the table by brute force on top of label_ref.label_f32's winner and profile_ref.point_terms'
q and iq, accumulated with np.add.at into int64, and the policy with plain loops over Python integers - a(T) and o(T) as the total minus the
returns counted upwards from bin 0, the other way round than las_io sums them.

The float32 expressions round after every operation like the kernels built without contraction."""
import math
from fractions import Fraction

import numpy as np

import label_ref as lr
import profile_ref as pr

f32 = np.float32
KS = math.sqrt(-math.log(0.0005) / 2.0)          # 1.9495...: the issue's 1.95 is this, rounded up to three digits


def shape(half_width, ring_q, bin_shift):
    """-> (hq, Z, NB)."""
    hq = int(math.ceil(float(f32(half_width)) * 1024.0))
    return hq, hq // int(ring_q) + 1, 65536 >> int(bin_shift)


def hist_terms(pts, seg, stations, half_width, ring_q, bin_shift, line, win):
    """The rule's terms of every point from its label and winning segment: profile_ref.point_terms' q and iq (any bin: neither depends on
    it), then r, ib (int64) and cell (the flat index into the table, -1 without a label)."""
    pts, seg = np.asarray(pts, f32), np.asarray(seg, f32)
    n_lines = int(np.max(line)) if len(line) else 0
    terms = pr.point_terms(pts, seg, stations, np.zeros(n_lines + 2, np.int64), 1.0, line, win)
    hq, Z, NB = shape(half_width, ring_q, bin_shift)
    on = np.asarray(line) > 0
    r = np.minimum(np.abs(terms['q']), hq) // int(ring_q)
    ib = terms['iq'] >> int(bin_shift)
    k = np.asarray(line, np.int64)
    return {'q': terms['q'], 'iq': terms['iq'], 'r': np.where(on, r, 0), 'ib': np.where(on, ib, 0),
            'cell': np.where(on, ((k - 1) * Z + r) * NB + ib, -1)}


def accumulate(terms, L, Z, NB, hist=None):
    flat = np.zeros(L * Z * NB, np.int64) if hist is None else np.array(hist, np.int64, copy=True).reshape(-1)
    np.add.at(flat, terms['cell'][terms['cell'] >= 0], 1)
    return flat.reshape(L, Z, NB)


def hist_f32(pts, seg, stations, L, half_width, z_tol, ring_q, bin_shift, mask=None, hist=None, pruned=False):
    """The whole rule by brute force (no min_intensity: every finite return counts): -> (hist [L, Z, NB], terms, line, win).  pruned: the
    winner from profile_ref.winner_f32_pruned, for clouds of millions of points."""
    if pruned:
        line, win = pr.winner_f32_pruned(pts, seg, half_width, z_tol, None, mask)
    else:
        line, _, win = lr.label_f32(pts, seg, half_width, z_tol, None, mask=mask)
    terms = hist_terms(pts, seg, stations, half_width, ring_q, bin_shift, line, win)
    _, Z, NB = shape(half_width, ring_q, bin_shift)
    return accumulate(terms, L, Z, NB, hist), terms, line, win


# ---------------------------------------------------------------------------------------------------------------- the policy
def rings(half_width, ring, inner, outer):
    """-> (ring_q, Z, inner rings, outer rings) of PaintThreshold's arguments."""
    rq = lambda v: int(math.floor(1024.0 * v + 0.5))
    ring_q, inner_q, outer_q = max(1, rq(ring)), rq(inner), rq(outer)
    Z = shape(half_width, ring_q, 0)[1]
    return ring_q, Z, [r for r in range(Z) if (r + 1) * ring_q <= inner_q], [r for r in range(Z) if r * ring_q >= outer_q]


def group(A, O, bin_shift, min_returns, min_separation, tolerance_shift, coeff=1.95):
    """One group, A and O lists of Python integers."""
    NB = len(A)
    NA, NO = sum(A), sum(O)
    below_a, below_o, run_a, run_o = [], [], 0, 0                 # the returns of the bins b < T, counted upwards
    for b in range(NB):
        below_a.append(run_a), below_o.append(run_o)
        run_a, run_o = run_a + A[b], run_o + O[b]
    a = lambda T: NA - below_a[T]
    o = lambda T: NO - below_o[T]
    J = {T: a(T) * NO - o(T) * NA for T in range(1, NB)}
    M = max(J.values())
    t0 = min(T for T in J if J[T] == M)
    floor = M - (M >> tolerance_shift)
    lo = t0
    while lo - 1 >= 1 and J[lo - 1] >= floor:
        lo -= 1
    hi = t0
    while hi + 1 <= NB - 1 and J[hi + 1] >= floor:
        hi += 1
    T = (lo + hi) // 2
    D = M / (NA * NO) if NA * NO else 0.0
    ok = NA >= min_returns and NO >= min_returns and M > 0 and D >= max(min_separation, coeff * math.sqrt((NA + NO) / (NA * NO)))
    w = 1 << bin_shift
    mean = lambda H, n: float(sum(c * Fraction(2 * b * w + w - 1, 2) for b, c in enumerate(H)) / n) if n else None
    return {'threshold': float(T * w) if ok else None, 'supported': bool(ok), 'separation': D, 'inner_returns': NA, 'outer_returns': NO,
            'paint_share': a(T) / NA if NA else None, 'false_share': o(T) / NO if NO else None, 'inner_mean': mean(A, NA),
            'outer_mean': mean(O, NO), 'plateau': [lo * w, hi * w]}


def policy(hist, half_width=0.625, ring=0.0625, inner=0.125, outer=0.375, bin_shift=6, min_returns=1000, min_separation=0.05,
           tolerance_shift=5):
    """las_io.paint_threshold on PaintThreshold's arguments, restated."""
    hist = np.asarray(hist)
    _, Z, inn, out = rings(half_width, ring, inner, outer)
    assert hist.shape[1:] == (Z, 65536 >> bin_shift)
    L, NB = hist.shape[0], hist.shape[2]

    def of(ks):
        A = [sum(int(hist[k, r, b]) for k in ks for r in inn) for b in range(NB)]
        O = [sum(int(hist[k, r, b]) for k in ks for r in out) for b in range(NB)]
        return group(A, O, bin_shift, min_returns, min_separation, tolerance_shift)

    return {'strip': of(range(L)), 'lines': {k + 1: of([k]) for k in range(L)}}


def same_group(got, want, tag=''):
    """Every field equal, the floats to the last bit: each is one correctly rounded quotient of integers on both sides."""
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for key in want:
        assert got[key] == want[key] and type(got[key]) is type(want[key]), (tag, key, got[key], want[key])


def same_policy(got, want, tag=''):
    assert set(got) == {'strip', 'lines'} and set(got['lines']) == set(want['lines']), tag
    same_group(got['strip'], want['strip'], f'{tag} strip')
    for k in want['lines']:
        same_group(got['lines'][k], want['lines'][k], f'{tag} line {k}')
