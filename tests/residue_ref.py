"""Numpy / scipy / plain Python restatement of the paint residue (include/lanemap_hip.h, csrc/residue.hip) for the tests: the per-point
rule on top of label_ref.label_f32 (brute force over all segments, no grid), the connected components two ways that must agree -
scipy.ndimage.label on the dense grid and a plain Python union-find -, the statistics in Python integers, and the cell scenes the GPU
tests share."""
import numpy as np
from scipy import ndimage

import label_ref as lr

f32 = np.float32
I31 = 2 ** 31


def keys_f32(pts, seg, reach, z_tol, min_intensity, clear, grid, pruned=False):
    """pts [N,4] float32, seg [S,8] float32 (cut for any half width: the brute force needs no grid), grid: the dict of ops.residue_grid
    -> (key [N] int64, iq [N] int32).  pruned: label_ref.label_f32_pruned instead of label_f32, for clouds of millions of points."""
    pts = np.asarray(pts, f32)
    line, d2 = (lr.label_f32_pruned if pruned else lr.label_f32)(pts, seg, reach, z_tol, min_intensity)[:2]
    clear2 = f32(clear) * f32(clear)
    res = (line > 0) & (d2 > clear2)
    x0, y0, inv = f32(grid['x0']), f32(grid['y0']), f32(1.0 / grid['cell'])
    nx, ny = int(grid['nx']), int(grid['ny'])
    key = np.full(len(pts), -1, np.int64)
    iq = np.zeros(len(pts), np.int32)
    i = np.nonzero(res)[0]                                    # (a residue point is eligible: finite coordinates, a number for intensity)
    fx, fy = (pts[i, 0] - x0) * inv, (pts[i, 1] - y0) * inv
    assert fx.dtype == f32
    cx, cy = fx.astype(np.int64), fy.astype(np.int64)         # truncation towards zero, like (int)
    ok = (cx >= 0) & (cx < nx) & (cy >= 0) & (cy < ny)
    key[i[ok]] = cy[ok] * nx + cx[ok]
    q = np.fmin(np.fmax(np.rint(pts[i[ok], 3]), f32(0)), f32(65535))
    iq[i[ok]] = q.astype(np.int32)
    return key, iq


def roots_union_find(cells, nx, connectivity):
    """cells: ascending distinct keys -> root [M]: the smallest cell index of every cell's component, by a plain Python union-find over all
    neighbour pairs (neighbourhood on (cx, cy))."""
    cells = [int(k) for k in cells]
    at = {k: m for m, k in enumerate(cells)}
    parent = list(range(len(cells)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    steps = [(-1, 0), (0, -1)] + ([(-1, -1), (1, -1)] if connectivity == 8 else [])
    for m, k in enumerate(cells):
        cx, cy = k % nx, k // nx
        for dx, dy in steps:
            x, y = cx + dx, cy + dy
            if 0 <= x < nx and y >= 0 and (y * nx + x) in at:
                a, b = find(m), find(at[y * nx + x])
                if a != b:
                    parent[max(a, b)] = min(a, b)
    return np.array([find(m) for m in range(len(cells))], dtype=np.int32).reshape(len(cells))


def roots_scipy(cells, nx, connectivity):
    """The same roots from scipy.ndimage.label on the dense grid of the cells' bounding box."""
    cells = np.asarray(cells, np.int64)
    if not len(cells):
        return np.zeros(0, np.int32)
    cx, cy = cells % nx, cells // nx
    x0, y0 = cx.min(), cy.min()
    dense = np.zeros((cy.max() - y0 + 1, cx.max() - x0 + 1), bool)
    dense[cy - y0, cx - x0] = True
    lab, n = ndimage.label(dense, structure=np.ones((3, 3)) if connectivity == 8 else None)
    of = lab[cy - y0, cx - x0]
    first = np.full(n + 1, len(cells), np.int64)
    np.minimum.at(first, of, np.arange(len(cells)))
    return first[of].astype(np.int32)


def roots(cells, nx, connectivity):
    a, b = roots_union_find(cells, nx, connectivity), roots_scipy(cells, nx, connectivity)
    assert np.array_equal(a, b), 'the two references disagree'
    return a


def dense_ids(root):
    """root [M] -> (comp [M] int32, K): components numbered 0 .. K-1 in ascending root."""
    u, comp = np.unique(np.asarray(root), return_inverse=True)
    return comp.astype(np.int32).reshape(len(root)), len(u)


def stats(cells, nx, comp, K, cell_points, cell_iq):
    """-> [K,12] int64 from Python integers (each checked to fit)."""
    rows = [[0, 0, 0, 0, 0, 0, 0, 0, I31 - 1, -I31, I31 - 1, -I31] for _ in range(K)]
    for m, k in enumerate(cells):
        k = int(k)
        cx, cy, r = k % nx, k // nx, rows[int(comp[m])]
        for c, v in enumerate((1, int(cell_points[m]), int(cell_iq[m]), cx, cy, cx * cx, cx * cy, cy * cy)):
            r[c] += v
        r[8], r[9], r[10], r[11] = min(r[8], cx), max(r[9], cx), min(r[10], cy), max(r[11], cy)
    assert all(-2 ** 63 <= v < 2 ** 63 for r in rows for v in r)
    return np.array(rows, dtype=np.int64).reshape(K, 12)


def blobs(keys_list, iq_list, nx, connectivity):
    """The whole pipeline after the keys: per-cloud key / iq arrays -> (cells [M], comp [M], stats [K,12])."""
    key = np.concatenate([np.asarray(k, np.int64) for k in keys_list]) if keys_list else np.zeros(0, np.int64)
    iq = np.concatenate([np.asarray(q, np.int64) for q in iq_list]) if iq_list else np.zeros(0, np.int64)
    on = key >= 0
    cells, inverse, counts = np.unique(key[on], return_inverse=True, return_counts=True)
    cell_iq = np.zeros(len(cells), np.int64)
    np.add.at(cell_iq, inverse.reshape(-1), iq[on])
    comp, K = dense_ids(roots(cells, nx, connectivity))
    return cells, comp, stats(cells, nx, comp, K, counts, cell_iq)


# ---------------------------------------------------------------------------------------------------------------- cell scenes
def _keys(xy, nx):
    xy = np.asarray(sorted(set((int(x), int(y)) for x, y in xy)), np.int64).reshape(-1, 2)
    return np.sort(xy[:, 1] * nx + xy[:, 0])


def serpentine(n=64):
    """A one-cell-wide path over an n x n grid: the even rows full, joined at alternating ends - one chain of n*n/2 + n/2 - 1 cells."""
    xy = [(x, y) for y in range(0, n, 2) for x in range(n)]
    xy += [((n - 1) if (y // 2) % 2 == 0 else 0, y) for y in range(1, n - 1, 2)]
    return _keys(xy, n), n, n


def u_shape(h=40, gap=5):
    """Two arms that meet only in the last row - at the largest keys: the arms have grown into two trees by then, roots must be hooked."""
    nx = gap + 2
    xy = [(0, y) for y in range(h)] + [(gap + 1, y) for y in range(h)] + [(x, h) for x in range(gap + 2)]
    return _keys(xy, nx), nx, h + 1


def diagonal_blobs():
    """Two 3 x 3 blocks that touch at one corner only: one component at 8, two at 4."""
    xy = [(x, y) for x in range(3) for y in range(3)] + [(x, y) for x in range(3, 6) for y in range(3, 6)]
    return _keys(xy, 9), 9, 7


def checkerboard(n=16):
    return _keys([(x, y) for x in range(n) for y in range(n) if (x + y) % 2 == 0], n), n, n


def row_wrap():
    """(nx - 1, 0) and (0, 1) are consecutive keys and no neighbours; likewise (nx - 1, 2) and (0, 3) with (nx - 2, 2) beside."""
    nx = 8
    return _keys([(7, 0), (0, 1), (7, 2), (6, 2), (0, 3), (1, 4)], nx), nx, 5


def random_grid(n=96, occupancy=0.4, seed=96):
    on = np.random.RandomState(seed).rand(n, n) < occupancy
    ys, xs = np.nonzero(on)
    return _keys(zip(xs, ys), n), n, n


def cell_scenes():
    """{name: (keys, nx, ny)}: the scenes above and prefixes of the random grid with M = 0, 1, 63, 64, 65, 257 cells."""
    out = {'serpentine': serpentine(), 'u': u_shape(), 'diagonal': diagonal_blobs(), 'checkerboard': checkerboard(), 'row_wrap': row_wrap(),
           'random': random_grid()}
    k, nx, ny = out['random']
    for M in (0, 1, 63, 64, 65, 257):
        out[f'random[:{M}]'] = (k[:M].copy(), nx, ny)
    return out


def point_counts(keys, seed=1):
    """Point counts and intensity sums to attach to a cell set: (cell_points [M], cell_iq [M]) int64."""
    rng = np.random.RandomState(seed + len(keys))
    n = rng.randint(1, 40, len(keys)).astype(np.int64)
    return n, (n * rng.randint(0, 65536, len(keys))).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- the point scene
REACH, CLEAR, ZTOL, MIN_I, CELL = 1.5, lr.HW, lr.ZTOL, 500.0, 0.125      # all exact in float32: 'exactly clear away' exists
AT_CLEAR, AT_REACH, PAST_REACH, AT_ZTOL, PAST_ZTOL, AT_MIN_I, BELOW_MIN_I, NAN_I = (3, 4), 0, 1, 2, 3, 4, 5, 6   # AT_CLEAR: label_ref's EXACT_HW


def scene_points(seg, index_grid=None, seed=11):
    """-> (pts [N,4] float32, first): label_ref.scene_points (its special points first - those exactly half_width = CLEAR beside line 1
    among them -, NaN / Inf coordinates, random points around the lines with intensities 0 .. 1999), then from index `first` the special
    points of the residue rule (the indices above are relative to it), then two painted bars across lines 1 and 2 and a stripe beside
    line 2."""
    base = lr.scene_points(seg, index_grid)
    rng = np.random.RandomState(seed)
    P = []
    add = lambda x, y, z, i=1000.0: P.append((x, y, z, i))
    add(4.0, 2.0 - REACH, 0.04)                          # exactly REACH beside line 1: d2 = reach^2, a hit, and residue
    add(4.0, 2.0 - REACH - 2.0 ** -12, 0.04)             # just past it: no line within reach
    add(0.0, 3.0, ZTOL)                                  # 1 m beside the first vertex of line 1 (height 0), exactly z_tol above: residue
    add(0.0, 3.0, float(np.nextafter(f32(ZTOL), f32(1))))
    add(8.0, 3.0, 0.08, MIN_I)                           # the threshold met exactly
    add(8.0, 3.0, 0.08, float(np.nextafter(f32(MIN_I), f32(0))))
    add(8.0, 3.0, 0.08, np.nan)
    add(8.0, 3.0, 0.08, 1000.5), add(8.0, 3.0, 0.08, 1001.5), add(8.0, 3.0, 0.08, 70000.0)     # rintf to even; the clamp at 65535
    n = 1500
    for x0 in (20.0, 26.0):                              # two bars of 0.3 m across lines 1 and 2
        for x, y in zip(rng.uniform(x0, x0 + 0.3, n), rng.uniform(1.0, 6.5, n)):
            add(x, y, 0.01 * x, float(rng.randint(600, 3000)))
    for x, y in zip(rng.uniform(30.0, 36.0, n), rng.uniform(6.4, 6.6, n)):                      # a stripe 1 m beside line 2
        add(x, y, 0.01 * x, float(rng.randint(600, 3000)))
    return np.concatenate([base, np.asarray(P, np.float64).astype(f32)]), len(base)
