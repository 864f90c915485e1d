"""Numpy restatement of the labelling rule (include/lanemap_hip.h, csrc/label.hip) for the tests: the float32 rule by brute force over all
segments - no grid -, the same rule in float64, a record patcher for point formats 0-10, and the scene the GPU tests share.

The float32 functions round after every operation like the kernel built without contraction; np.fmax / np.fmin drop a NaN like fmaxf /
fminf do."""
import numpy as np

f32 = np.float32
INF32 = f32(np.inf)


def seg_lines(seg):
    return np.ascontiguousarray(seg[:, 7]).view(np.int32)


def eligible(pts, min_intensity=None):
    ok = np.isfinite(pts[:, 0]) & np.isfinite(pts[:, 1]) & np.isfinite(pts[:, 2])
    if min_intensity is not None:
        with np.errstate(invalid='ignore'):
            ok &= pts[:, 3] >= f32(min_intensity)
    return ok


def label_f32(pts, seg, half_width, z_tol, min_intensity=None, mask=None, line_tie=True):
    """pts [N,4] float32, seg [S,8] float32 -> (line [N] int32, dist2 [N] float32, winner [N] segment index or -1).  mask: points that
    may be labelled at all (the records that pass a select).  line_tie=False: a WRONG rule, ties in d2 to the smaller segment index
    alone, for the tests that show that a case tells the two rules apart."""
    pts, seg = np.asarray(pts, f32), np.asarray(seg, f32)
    N = len(pts)
    line, best, win = np.zeros(N, np.int32), np.full(N, INF32), np.full(N, -1, np.int64)
    ok = eligible(pts, min_intensity)
    if mask is not None:
        ok &= mask
    hw2, zt = f32(half_width) * f32(half_width), f32(z_tol)
    lines = seg_lines(seg)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all='ignore'):
        for s in range(len(seg)):                                          # ascending: a tie in d2 and line stays with the smaller index
            ax, ay, az, dx, dy, dz, inv = (seg[s, k] for k in range(7))
            px, py = x - ax, y - ay
            t = np.fmin(np.fmax((px * dx + py * dy) * inv, f32(0)), f32(1))
            ex, ey = px - t * dx, py - t * dy
            d2 = ex * ex + ey * ey
            zl = az + t * dz
            hit = ok & (d2 <= hw2) & (np.abs(z - zl) <= zt)
            take = hit & ((d2 < best) | ((d2 == best) & (lines[s] < line) & line_tie))
            best[take], line[take], win[take] = d2[take], lines[s], s
    assert best.dtype == f32
    return line, best, win


def permuted_table(seg):
    """The segment table with the rows of line 3 moved in front of all others: a table no longer sorted by line, which a caller may pass."""
    three = seg_lines(seg) == 3
    return np.concatenate([seg[three], seg[~three]])


def label_f32_pruned(pts, seg, half_width, z_tol, min_intensity=None, mask=None):
    """label_f32 for clouds of millions of points: the same float32 expression per (point, segment) pair, evaluated only for the points in
    the segment's bounding box widened by 2 half_width + 1 mm - a point outside it is further than half_width from the segment by far more
    than float32 rounding, so it is no hit and leaving the pair out changes nothing.  -> (line, dist2)."""
    pts, seg = np.asarray(pts, f32), np.asarray(seg, f32)
    N = len(pts)
    line, best = np.zeros(N, np.int32), np.full(N, INF32)
    ok = eligible(pts, min_intensity)
    if mask is not None:
        ok &= mask
    order = np.argsort(pts[:, 0], kind='stable')
    xs = pts[order, 0].astype(np.float64)
    xs = np.where(np.isnan(xs), np.inf, xs)                                # NaNs sort last: keep the array ascending
    hw2, zt, lines = f32(half_width) * f32(half_width), f32(z_tol), seg_lines(seg)
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
            best[idx[take]], line[idx[take]] = d2[take], lines[s]
    return line, best


def label_f64(pts, seg, half_width, z_tol, min_intensity=None):
    """The rule in float64 on the same float32 inputs: -> (line [N], d [N, n_lines] the distance to every line where the height band
    holds (inf elsewhere), dz [N, n_lines] the smallest | |z - zl| - z_tol | over the line's segments within 2 half_width)."""
    p, g = np.asarray(pts, np.float64), np.asarray(seg, np.float64)
    lines = seg_lines(np.asarray(seg, f32))
    L = int(lines.max()) if len(lines) else 0
    N = len(p)
    d = np.full((N, L), np.inf)
    zgap = np.full((N, L), np.inf)
    ok = eligible(np.asarray(pts, f32), min_intensity)
    with np.errstate(all='ignore'):
        for s in range(len(g)):
            ax, ay, az, dx, dy, dz = g[s, :6]
            l2 = dx * dx + dy * dy
            px, py = p[:, 0] - ax, p[:, 1] - ay
            t = np.clip((px * dx + py * dy) / l2, 0.0, 1.0) if l2 > 0 else np.zeros(N)
            dist = np.hypot(px - t * dx, py - t * dy)
            off = np.abs(p[:, 2] - (az + t * dz))
            k = lines[s] - 1
            inband = ok & (off <= z_tol)
            d[:, k] = np.where(inband & (dist < d[:, k]), dist, d[:, k])
            near = ok & (dist <= 2 * half_width)
            zgap[:, k] = np.where(near, np.minimum(zgap[:, k], np.abs(off - z_tol)), zgap[:, k])
    line = np.zeros(N, np.int32)
    if L:
        k = np.argmin(d, axis=1)
        dm = d[np.arange(N), k]
        line = np.where(dm <= half_width, k + 1, 0).astype(np.int32)
    return line, d, zgap


# ---------------------------------------------------------------------------------------------------------------- records
CLASS_BYTE = {True: 16, False: 15}          # keyed by (format >= 6)
SOURCE_ID = {True: 20, False: 18}


def patch_records(rec, fmt, line, marking_class, write_line_id):
    """rec [n, record_len] uint8 -> a patched copy: in a record with line > 0 the classification becomes marking_class (formats 0-5: the
    low five bits of byte 15; 6-10: byte 16) and, with write_line_id, the point source ID (u16 LE) becomes the line."""
    out = np.array(rec, dtype=np.uint8, copy=True)
    six = fmt >= 6
    on = np.asarray(line) > 0
    if six:
        out[on, 16] = marking_class
    else:
        assert 0 <= marking_class <= 31
        out[on, 15] = (out[on, 15] & 0xE0) | marking_class
    if write_line_id:
        o = SOURCE_ID[six]
        out[on, o] = np.asarray(line)[on] & 255
        out[on, o + 1] = np.asarray(line)[on] >> 8
    return out


def decode_f32(rec, scale, offset, shift):
    """The decode's rows for [n, record_len] uint8 records: X * scale + (offset - shift) in float64, rounded to float32; raw intensity."""
    rec = np.ascontiguousarray(rec)
    xyz = np.stack([np.ascontiguousarray(rec[:, 4 * a:4 * a + 4]).view('<i4')[:, 0] for a in range(3)], axis=1).astype(np.float64)
    o = np.asarray(offset, np.float64) - np.asarray(shift, np.float64)
    out = np.empty((len(rec), 4), f32)
    out[:, :3] = (xyz * np.asarray(scale, np.float64) + o).astype(f32)
    out[:, 3] = np.ascontiguousarray(rec[:, 12:14]).view('<u2')[:, 0].astype(f32)
    return out


# ---------------------------------------------------------------------------------------------------------------- the scene
SHARED_VERTEX, TRIPLE, CROSSING, EXACT_HW, EXACT_ZTOL, BETWEEN, ON_LINE_4, INTENSITY = 0, 1, 2, (3, 4), (6, 7), 8, 9, (10, 11, 12)
HW, ZTOL = 0.15625, 0.5              # both exact in float32, so that 'exactly half_width away' and 'exactly z_tol off' exist


def scene_lines():
    """Line 1 and 2: parallel, 3.5 m apart, vertices every 2 m over 40 m, climbing 1 %.  Line 3 crosses both.  Line 4 runs 6 m above line
    1.  Line 5 holds a zero-length segment (a doubled vertex).  Line 6 has one vertex and gives no segment.  All values are exact in
    float32 after the shift."""
    xs = np.arange(0.0, 42.0, 2.0)
    l1 = np.stack([xs, np.full_like(xs, 2.0), 0.01 * xs], axis=1)
    l2 = l1 + np.array([0.0, 3.5, 0.0])
    l3 = np.array([[10.0, -1.0, 0.1], [14.0, 2.0, 0.14], [20.0, 8.0, 0.2]])
    l4 = l1 + np.array([0.0, 0.0, 6.0])
    l5 = np.array([[30.0, 9.0, 0.3], [30.0, 9.0, 0.3], [32.0, 9.0, 0.32], [32.0, 11.0, 0.32]])
    l6 = np.array([[5.0, 5.0, 0.0]])
    return [l1, l2, l3, l4, l5, l6]


SHIFT = np.array([351200.0, 3433000.0, 12.0])


def scene_points(seg, grid=None, seed=5, n_random=3000):
    """The special points of the exactness test followed by random points around the lines: [N,4] float32 (intensity 1000 unless said)."""
    rng = np.random.RandomState(seed)
    hw = f32(HW)
    P = []
    add = lambda x, y, z, i=1000.0: P.append((x, y, z, i))
    add(6.0, 2.0, 0.06)                        # on a shared vertex of line 1: two segments at d2 = 0, the lower index wins
    add(30.0, 9.0, 0.3)                        # on the doubled vertex of line 5: three segments at d2 = 0
    add(14.0, 2.0, 0.14)                       # the crossing of line 3 with line 1, a vertex of both: tie in d2, smaller line wins
    add(8.0, 2.0 + float(hw), 0.08)            # exactly half_width beside line 1: py = hw, d2 = hw * hw = hw2 (points 3, 4: EXACT_HW)
    add(8.0, 2.0 - float(hw), 0.08)
    add(9.0, 2.0, 0.09 + 0.5)                  # about z_tol above line 1
    add(0.0, 2.0, ZTOL)                        # exactly z_tol above the first vertex of line 1, whose height is 0 (points 6, 7: EXACT_ZTOL)
    add(0.0, 2.0, -ZTOL)
    add(8.0, 2.0, 3.0)                         # between the carriageways: no label
    add(8.0, 2.0, 6.08)                        # on line 4
    add(8.0, 2.05, 0.08, 500.0)                # intensity met exactly by min_intensity = 500
    add(8.0, 2.05, 0.08, 499.0)
    add(8.0, 2.05, 0.08, np.nan)
    add(np.nan, 2.0, 0.0), add(8.0, np.nan, 0.0), add(8.0, 2.0, np.nan)
    add(np.inf, 2.0, 0.0), add(8.0, -np.inf, 0.0), add(8.0, 2.0, np.inf)
    add(1e30, 2.0, 0.0), add(-1e30, -1e30, 0.0), add(3e38, 3e38, 0.0)
    add(-50.0, 2.0, 0.0), add(100.0, 2.0, 0.4), add(8.0, 500.0, 0.0)          # outside the grid
    add(-0.1, 2.0, 0.0), add(40.1, 2.0, 0.4), add(0.0, 2.0, 0.0), add(40.0, 2.0, 0.4)   # the ends of line 1
    if grid is not None:                       # cell borders and the edges of the inflated box
        x0, y0, c, nx, ny = grid
        for i in range(0, nx + 1, max(1, nx // 12)):
            for y in (2.0, 2.1, 5.5):
                add(float(f32(x0 + i * c)), y, 0.01 * (x0 + i * c))
        for j in range(0, ny + 1, max(1, ny // 6)):
            for x in (8.0, 13.0, 31.0):
                add(x, float(f32(y0 + j * c)), 0.01 * x)
        add(x0, y0, 0.0), add(float(f32(x0 + nx * c)), float(f32(y0 + ny * c)), 0.0)
    pts = np.asarray(P, dtype=np.float64)
    # random points within +-1 m of random places on the segments, a third of them snapped onto the 1/64 m lattice (ties, exact values)
    s = rng.randint(0, len(seg), n_random)
    t = rng.uniform(0, 1, n_random)
    base = seg[s, 0:3].astype(np.float64) + t[:, None] * seg[s, 3:6].astype(np.float64)
    rnd = base + np.stack([rng.uniform(-1, 1, n_random), rng.uniform(-1, 1, n_random), rng.uniform(-0.8, 0.8, n_random)], axis=1)
    snap = rng.rand(n_random) < 0.33
    rnd[snap, :2] = np.round(rnd[snap, :2] * 64) / 64
    inten = rng.randint(0, 2000, n_random).astype(np.float64)
    return np.concatenate([pts, np.concatenate([rnd, inten[:, None]], axis=1)]).astype(f32)
