"""The intensity balance (csrc/intensity.hip: lm_tile_intensity_cells, lm_tile_intensity_apply; the rule: include/lanemap_hip.h) restated
in numpy, for tests/test_balance_cpu.py and tests/test_gpu_balance.py.  Everything here is integers or float32 operations rounded one by
one in the order of the kernels, so the GPU results are compared for equality.

  counted       which points of a tile count (window test of tests/ground_ref.py && intensity not NaN), their pixel and key
  cells         level, count and model per cell
  gains         the host policy, restated apart from las_io.balance_gains
  apply         the balanced points
  falloff_tile  the scenario of the issue: a tile whose intensity falls to a quarter across its columns
"""
import numpy as np

import ground_ref as gr

f32 = np.float32


def counted(pts, p, H, W):
    """-> (on [n] bool, row [n], col [n], key [n] int64) of the points of one tile; row, col and key mean something where `on` holds."""
    pts = np.asarray(pts, dtype=f32).reshape(-1, 4)
    assert np.isfinite(pts[:, :3]).all(), 'the reference window test needs finite coordinates'
    on, row, col, _ = gr.window(pts, p, H, W)
    i = pts[:, 3]
    on = on & ~np.isnan(i)
    with np.errstate(invalid='ignore'):
        k = np.floor(np.minimum(np.maximum(np.where(np.isnan(i), f32(0), i), f32(0)), f32(65535)))
    assert k.dtype == np.float32
    return on, row, col, k.astype(np.int64)


def lower_median(values):
    s = np.sort(np.asarray(values, dtype=np.int64))
    return int(s[(len(s) - 1) // 2])


def cells(pts, offs, params, H, W, cell_px=32, q_ppm=500000, min_points=64):
    """-> (level, count, model), each [B, Gy, Gx] int32, as ops.tile_intensity_cells returns them."""
    Gy, Gx = gr.grid_shape(H, W, cell_px)
    B = len(params)
    level = np.full((B, Gy, Gx), -1, np.int32)
    count = np.zeros((B, Gy, Gx), np.int32)
    model = np.full((B, Gy, Gx), -1, np.int32)
    for b, p in enumerate(params):
        on, row, col, key = counted(pts[offs[b]:offs[b + 1]], p, H, W)
        cell = (row[on] // cell_px) * Gx + col[on] // cell_px
        k = key[on]
        order = np.lexsort((k, cell))
        cell, k = cell[order], k[order]
        starts = np.searchsorted(cell, np.arange(Gy * Gx + 1))
        for c in range(Gy * Gx):
            n = int(starts[c + 1] - starts[c])
            count[b, c // Gx, c % Gx] = n
            if n:
                level[b, c // Gx, c % Gx] = k[starts[c] + (n - 1) * int(q_ppm) // 10 ** 6]
        known = count[b] >= min_points
        for cy in range(Gy):
            for cx in range(Gx):
                sl = (slice(max(cy - 1, 0), cy + 2), slice(max(cx - 1, 0), cx + 2))
                near = level[b][sl][known[sl]]
                if len(near):
                    model[b, cy, cx] = lower_median(near)
    return level, count, model


def gains(model, reference, max_gain=4.0):
    """-> float32 [B, Gy, Gx]: clip(f32(reference[b]) / f32(max(model, 1)), 1 / max_gain, max_gain) for a known model (>= 0) and
    reference[b] > 0, else 1; every operation in float32."""
    model = np.asarray(model)
    out = np.ones(model.shape, f32)
    top = f32(max_gain)
    low = f32(1.0) / top
    for b in range(model.shape[0]):
        if int(reference[b]) <= 0:
            continue
        for idx in np.ndindex(model.shape[1:]):
            m = int(model[b][idx])
            if m >= 0:
                g = f32(int(reference[b])) / f32(max(m, 1))
                out[b][idx] = min(max(g, low), top)
    return out


def _axis(px, cell_px, G):
    u = (2 * px + 1 - cell_px).astype(f32) / f32(2 * cell_px)
    u = np.minimum(np.maximum(u, f32(0)), f32(G - 1))
    fl = np.floor(u)
    i0 = fl.astype(np.int64)
    return i0, np.minimum(i0 + 1, G - 1), u - fl


def gain_at(g, row, col, cell_px):
    """The gain of pixels (row, col) of one tile from its gains g [Gy, Gx]: bilinear between the cell centres, each operation rounded."""
    g = np.asarray(g, dtype=f32)
    Gy, Gx = g.shape
    x0, x1, fx = _axis(np.asarray(col, np.int64), cell_px, Gx)
    y0, y1, fy = _axis(np.asarray(row, np.int64), cell_px, Gy)
    ux, uy = f32(1) - fx, f32(1) - fy
    top = g[y0, x0] * ux + g[y0, x1] * fx
    bot = g[y1, x0] * ux + g[y1, x1] * fx
    out = top * uy + bot * fy
    assert out.dtype == np.float32 and fx.dtype == np.float32
    return out


def apply(pts, offs, params, gain, H, W, cell_px=32):
    """-> a copy of pts [N, 4] f32 with the intensities of the rows offs[0] .. offs[B] balanced, as ops.tile_intensity_apply leaves them."""
    out = np.array(pts, dtype=f32, copy=True).reshape(-1, 4)
    for b, p in enumerate(params):
        tile = out[offs[b]:offs[b + 1]]
        on, row, col, _ = counted(tile, p, H, W)
        with np.errstate(invalid='ignore', over='ignore'):
            v = tile[on, 3] * gain_at(gain[b], row[on], col[on], cell_px)
            assert v.dtype == np.float32
            tile[on, 3] = np.fmin(v, f32(65535))
    return out


def falloff_tile(p, T=96, per_pixel=4, seed=3):
    """The scenario: `per_pixel` returns at every pixel centre of the T x T window of the axis-aligned tile p.  Asphalt falls as
    8000 * 0.25 ** (col / (T - 1)), paint is 2.5 x the local asphalt on the columns with col % 32 in 14..16, multiplicative noise of
    +-5 %.  -> (pts [T T per_pixel, 4] f32, paint [n] bool, col [n])."""
    rng = np.random.RandomState(seed)
    r, c = np.meshgrid(np.arange(T), np.arange(T), indexing='ij')
    r, c = np.repeat(r.ravel(), per_pixel), np.repeat(c.ravel(), per_pixel)
    asphalt = 8000.0 * 0.25 ** (c / (T - 1.0))
    paint = (c % 32 >= 14) & (c % 32 <= 16)
    inten = np.floor(np.where(paint, 2.5, 1.0) * asphalt * rng.uniform(0.95, 1.05, len(c)))
    x = r * float(p.img_reso[0]) + float(p.bev_img_offset[0]) + float(p.trans[0])
    y = c * float(p.img_reso[1]) + float(p.bev_img_offset[1]) + float(p.trans[1])
    pts = np.stack([x, y, np.full(len(c), 0.5 + float(p.trans[2])), inten], axis=1).astype(f32)
    order = rng.permutation(len(pts))
    return pts[order], paint[order], c[order]
