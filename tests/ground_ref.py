"""The per-tile ground model (csrc/ground.hip) restated in float32 numpy, for tests/test_ground_cpu.py and tests/test_gpu_ground.py.

Every float operation is rounded on its own in the order of the kernels (csrc/raster_xf.h is compiled without fused multiply-add), and
minima and medians are taken on the kernels' order-preserving u32 keys, so the GPU results can be compared bit for bit.
  (a) cell_keys     per tile the smallest key of vz over the points of each cell, EMPTY = 0xFFFFFFFF
  (b) smooth        lower median of the non-empty keys of the 3 x 3 neighbourhood; tile minimum
  (c) select        stable per-tile selection by height above the ground
"""
import math

import numpy as np

f32 = np.float32
EMPTY = np.uint32(0xFFFFFFFF)


def xf(p):
    """lm_raster_derive restated: double, then rounded to float (the operation order of csrc/raster_xf.h)."""
    q = [float(v) for v in p.quat]
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    w, x, y, z = q[0] / n, q[1] / n, q[2] / n, q[3] / n
    R = [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
         2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]
    m = [f32(R[j * 3 + i] / n) for i in range(3) for j in range(3)]
    return {'m': m, 't': [f32(v) for v in p.trans], 'off': [f32(v) for v in p.bev_img_offset],
            'irow': f32(1.0) / f32(p.img_reso[0]), 'icol': f32(1.0) / f32(p.img_reso[1])}


def window(pts, p, H, W):
    """lm_point_window + the finite-height rule: -> (counts [n] bool, row [n] int, col [n] int, vz [n] f32); row / col are only
    meaningful where `counts` holds."""
    X = xf(p)
    m, t = X['m'], X['t']
    pts = np.asarray(pts, dtype=f32).reshape(-1, 4)
    with np.errstate(invalid='ignore', over='ignore'):
        dx, dy, dz = pts[:, 0] - t[0], pts[:, 1] - t[1], pts[:, 2] - t[2]
        vx = (m[0] * dx + m[1] * dy) + m[2] * dz
        vy = (m[3] * dx + m[4] * dy) + m[5] * dz
        vz = (m[6] * dx + m[7] * dy) + m[8] * dz
        assert vx.dtype == np.float32 and vz.dtype == np.float32
        row = np.floor((vx - X['off'][0]) * X['irow'] + f32(0.5))
        col = np.floor((vy - X['off'][1]) * X['icol'] + f32(0.5))
        on = (row >= 0) & (row < H) & (col >= 0) & (col < W) & np.isfinite(vz)
    ri, ci = np.zeros(len(pts), np.int64), np.zeros(len(pts), np.int64)
    ri[on], ci[on] = row[on].astype(np.int64), col[on].astype(np.int64)
    return on, ri, ci, vz


def key_of(v):
    """float32 -> u32, ascending with the value: sign bit flipped for v >= +0, all bits flipped below (-0.0 < +0.0)."""
    b = np.asarray(v, dtype=f32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def value_of(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(f32)


def grid_shape(H, W, cell_px):
    return -(-H // cell_px), -(-W // cell_px)


def cell_keys(pts, offs, params, H, W, cell_px):
    """(a) -> keys [B, Gy, Gx] u32."""
    Gy, Gx = grid_shape(H, W, cell_px)
    keys = np.full((len(params), Gy * Gx), EMPTY, dtype=np.uint32)
    for b, p in enumerate(params):
        on, row, col, vz = window(pts[offs[b]:offs[b + 1]], p, H, W)
        cell = (row[on] // cell_px) * Gx + col[on] // cell_px
        np.minimum.at(keys[b], cell, key_of(vz[on]))
    return keys.reshape(len(params), Gy, Gx)


def keys_to_values(keys):
    """u32 keys -> f32 values, NaN where EMPTY (the cell_min output)."""
    keys = np.asarray(keys, dtype=np.uint32)
    out = value_of(np.where(keys == EMPTY, np.uint32(0), keys)).copy()
    out[keys == EMPTY] = np.nan
    return out


def values_to_keys(values):
    """f32 grid with NaN = empty -> u32 keys (for hand-built grids)."""
    values = np.asarray(values, dtype=f32)
    k = key_of(np.where(np.isnan(values), f32(0), values))
    k[np.isnan(values)] = EMPTY
    return k


def smooth(keys):
    """(b) keys [B, Gy, Gx] -> (ground [B, Gy, Gx] f32 with NaN = no filled neighbour, ground_min [B] f32 with +inf = none)."""
    keys = np.asarray(keys, dtype=np.uint32)
    B, Gy, Gx = keys.shape
    med = np.full((B, Gy, Gx), EMPTY, dtype=np.uint32)
    for b in range(B):
        for cy in range(Gy):
            for cx in range(Gx):
                nb = keys[b, max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2].reshape(-1)
                nb = np.sort(nb[nb != EMPTY])
                if len(nb):
                    med[b, cy, cx] = nb[(len(nb) - 1) // 2]
    ground = keys_to_values(med)
    gmin = np.full(B, np.inf, dtype=f32)
    for b in range(B):
        if (med[b] != EMPTY).any():
            gmin[b] = value_of(med[b].min())
    return ground, gmin


def tile_ground(pts, offs, params, H, W, cell_px):
    """-> (ground, ground_min, cell_min) as ops.tile_ground(want_cell_min=True) returns them."""
    keys = cell_keys(pts, offs, params, H, W, cell_px)
    ground, gmin = smooth(keys)
    return ground, gmin, keys_to_values(keys)


def select(pts, offs, params, ground, H, W, cell_px, h_range):
    """(c) -> (kept rows [sum kept, 4] f32, offsets [B+1] int64)."""
    lo, hi = f32(h_range[0]), f32(h_range[1])
    Gy, Gx = grid_shape(H, W, cell_px)
    rows, out_offs = [], [0]
    for b, p in enumerate(params):
        tile = np.asarray(pts[offs[b]:offs[b + 1]], dtype=f32).reshape(-1, 4)
        on, row, col, vz = window(tile, p, H, W)
        g = np.asarray(ground[b], dtype=f32).reshape(-1)[(row // cell_px) * Gx + col // cell_px]
        with np.errstate(invalid='ignore'):
            h = vz - g
            assert h.dtype == np.float32
            keep = on & (h >= lo) & (h <= hi)
        rows.append(tile[keep])
        out_offs.append(out_offs[-1] + int(keep.sum()))
    return (np.concatenate(rows) if rows else np.zeros((0, 4), f32)), np.asarray(out_offs, dtype=np.int64)
