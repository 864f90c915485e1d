"""The intensity window (csrc/intensity.hip) and the scaled pixel rule of the rasteriser (lm_bev_raster_batch_scaled) restated in float32
numpy, for tests/test_intensity_cpu.py and tests/test_gpu_intensity.py.  Everything here is integers or float32 operations rounded one by
one in the order of the kernels, so the GPU results can be compared for equality.

  keys          the key of every counted point of one tile: window test (tests/ground_ref.py) && intensity not NaN
  window        the two order statistics, the count and the coarse histogram per group
  raster        the rasteriser's pixel rule with a per-tile intensity scale: scatter-max of I << 8 | G

The window test is ground_ref.window, which also asks for a finite tile-frame height: the clouds of these tests have finite coordinates
(asserted), for which it is exactly lm_point_window.
"""
import numpy as np

import ground_ref as gr

f32 = np.float32
NBIN = 4096


def keys(pts, p, H, W):
    """-> int64 keys of the points of `pts` that count for tile p: k = floor(min(max(i, 0), 65535)), NaN intensities do not count."""
    pts = np.asarray(pts, dtype=f32).reshape(-1, 4)
    assert np.isfinite(pts[:, :3]).all(), 'the reference window test needs finite coordinates'
    on = gr.window(pts, p, H, W)[0]
    i = pts[:, 3]
    on = on & ~np.isnan(i)
    k = np.floor(np.minimum(np.maximum(i[on], f32(0)), f32(65535)))
    assert k.dtype == np.float32
    return k.astype(np.int64)


def ppm(percent):
    return int(round(float(percent) * 1e4))


def order_stats(k, q_lo_ppm, q_hi_ppm):
    """sorted keys' elements of 0-based ranks (n - 1) q // 10**6; (-1, -1) for n = 0."""
    n = len(k)
    if n == 0:
        return -1, -1
    s = np.sort(np.asarray(k, dtype=np.int64))
    return int(s[(n - 1) * int(q_lo_ppm) // 10 ** 6]), int(s[(n - 1) * int(q_hi_ppm) // 10 ** 6])


def window(pts, offs, params, H, W, percentiles=(1.0, 99.9), group=None):
    """-> (window [G, 2] int32, count [G] int64, coarse_hist [G, 4096] int32) as ops.tile_intensity_window(want_hist=True) returns them."""
    B = len(params)
    group = list(range(B)) if group is None else [int(g) for g in group]
    G = max(group + [0]) + 1
    per = [[] for _ in range(G)]
    for b, p in enumerate(params):
        per[group[b]].append(keys(pts[offs[b]:offs[b + 1]], p, H, W))
    win = np.zeros((G, 2), np.int32)
    cnt = np.zeros((G,), np.int64)
    hist = np.zeros((G, NBIN), np.int64)
    for g in range(G):
        k = np.concatenate(per[g]) if per[g] else np.zeros((0,), np.int64)
        win[g] = order_stats(k, ppm(percentiles[0]), ppm(percentiles[1]))
        cnt[g] = len(k)
        hist[g] = np.bincount(k >> 4, minlength=NBIN)
    return win, cnt, hist.astype(np.int32)


def raster(pts, offs, params, H, W, scales=None):
    """-> u8 [B, H, W, 3] tiles: I = clamp(floor((clip(i, lo, hi) - lo) * scale + .5), 1, 255) with scale = the tile's entry of `scales`
    where that is given and positive, else float32(255) / float32(inten_hi); G = clamp(floor((vz - min_ele) / ele_reso + .5), 0, 255); a
    pixel keeps the maximum of I << 8 | G over its points; R = B = I."""
    B = len(params)
    out = np.zeros((B, H, W, 3), np.uint8)
    for b, p in enumerate(params):
        tile = np.asarray(pts[offs[b]:offs[b + 1]], dtype=f32).reshape(-1, 4)
        assert np.isfinite(tile[:, :3]).all()
        on, row, col, vz = gr.window(tile, p, H, W)
        lo, hi = f32(p.inten_lo), f32(p.inten_hi)
        scale = f32(255.0) / hi
        if scales is not None and scales[b] is not None and f32(scales[b]) > 0:
            scale = f32(scales[b])
        it = np.fmin(np.fmax(tile[on, 3], lo), hi) - lo            # fmaxf / fminf: a NaN intensity becomes lo
        I = np.clip(np.floor(it * scale + f32(0.5)), 1, 255)
        Gc = np.clip(np.floor((vz[on] - f32(p.local_min_ele)) * (f32(1.0) / f32(p.ele_reso)) + f32(0.5)), 0, 255)
        assert it.dtype == np.float32 and I.dtype == np.float32 and Gc.dtype == np.float32
        key = np.zeros(H * W, np.int64)
        np.maximum.at(key, row[on] * W + col[on], (I.astype(np.int64) << 8) | Gc.astype(np.int64))
        key = key.reshape(H, W)
        out[b, ..., 0] = key >> 8
        out[b, ..., 1] = key & 255
        out[b, ..., 2] = key >> 8
    return out
