#!/usr/bin/env python3
"""Micro-bench of the vertex drape (csrc/drape.hip) on the bench's synthetic clouds: T tiles of N points each.

  raster     ops.bev_raster_batch on the batch, the yardstick of the ratios
  drape_8    ops.drape_vertices for 8 lanes x 144 vertices per tile (a vertex every 8 rows, the head's row pitch), radius_px R
  drape_72   the same for 72 lanes x 144 vertices per tile, the most the head can emit
Each drape call includes its host part (the band sort of the vertices and the upload of the index).  Times are HIP events around each
call, median of `--reps` (default 20) after 3 warm-up calls.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lanemapping_amd import ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=int, default=4194304, help='points per tile')
ap.add_argument('--tiles', type=int, default=16)
ap.add_argument('--radius-px', type=int, default=4)
ap.add_argument('--reps', type=int, default=20)
a = ap.parse_args()
N, T, H, W, R = a.points, a.tiles, 1152, 1152, a.radius_px
dev = torch.device('cuda:0')
base = [torch.from_numpy(synth.las_points(2021 + i, N)).to(dev) for i in range(4)]
cloud = torch.cat([base[i % 4] for i in range(T)])
del base
offs = [N * i for i in range(T + 1)]
par = [ops.make_raster_params(local_min_ele=-0.5, ele_reso=0.02) for _ in range(T)]


def lanes(n_lanes):
    """n_lanes slightly slanted lanes of 144 vertices on every tile: -> (vertices [T * n_lanes * 144, 2] int32, vertex_offsets)."""
    rows = np.arange(3, H, 8)
    one = np.concatenate([np.stack([rows, np.clip((l + 0.5) * W / n_lanes + 0.02 * (rows - H / 2), 0, W - 1).astype(np.int64)], axis=1)
                          for l in range(n_lanes)])
    return np.ascontiguousarray(np.tile(one, (T, 1)), dtype=np.int32), [len(one) * i for i in range(T + 1)]


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in ev)
    return {'median_ms': ms[len(ms) // 2], 'min_ms': ms[0], 'max_ms': ms[-1], 'reps': reps}


out = torch.empty((T, H, W, 3), device=dev, dtype=torch.uint8)
res = {'tiles': T, 'points': int(cloud.shape[0]), 'radius_px': R}
res['raster'] = timed(lambda: ops.bev_raster_batch(cloud, offs, par, H, W, out_u8=out, u8_only=True), a.reps)
for n_lanes in (8, 72):
    vert, voffs = lanes(n_lanes)
    z, npix = ops.drape_vertices(cloud, offs, par, vert, voffs, H, W, radius_px=R)
    res[f'drape_{n_lanes}'] = timed(lambda: ops.drape_vertices(cloud, offs, par, vert, voffs, H, W, radius_px=R), a.reps)
    res[f'drape_{n_lanes}']['vertices'] = len(vert)
    res[f'drape_{n_lanes}']['mean_npix'] = float(npix.float().mean())
    res[f'drape_{n_lanes}_over_raster'] = res[f'drape_{n_lanes}']['median_ms'] / res['raster']['median_ms']
    res[f'drape_{n_lanes}_frac_of_8TBps'] = 16 * int(cloud.shape[0]) / (res[f'drape_{n_lanes}']['median_ms'] * 1e-3) / 8e12
print(json.dumps(res))
