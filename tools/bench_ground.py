#!/usr/bin/env python3
"""Micro-bench of the per-tile ground model (csrc/ground.hip) on the bench's synthetic clouds: T tiles of N points each.

  raster     ops.bev_raster_batch on the batch (the stage the ground model sits in front of), the yardstick of the ratios
  ground     ops.tile_ground: cell minima (16 N read), smoothing and tile minimum
  select     ops.ground_select with h_range = (-0.5, 1.0): count and emit (32 N read, 16 kept written); its one read-back of the
             offsets is inside
  chain      ground + select + raster of the selected points, what Runner does per batch with ground=GroundFilter(height_range=...)
Times are HIP events around each call, median of `--reps` (default 20) after 3 warm-up calls.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lanemapping_amd import ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=int, default=4194304, help='points per tile')
ap.add_argument('--tiles', type=int, default=16)
ap.add_argument('--cell-px', type=int, default=32)
ap.add_argument('--reps', type=int, default=20)
a = ap.parse_args()
N, T, H, W = a.points, a.tiles, 1152, 1152
dev = torch.device('cuda:0')
base = [torch.from_numpy(synth.las_points(2021 + i, N)).to(dev) for i in range(4)]
cloud = torch.cat([base[i % 4] for i in range(T)])
del base
offs = [N * i for i in range(T + 1)]
par = [ops.make_raster_params(local_min_ele=-0.5, ele_reso=0.02) for _ in range(T)]
H_RANGE = (-0.5, 1.0)


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
ground, gmin = ops.tile_ground(cloud, offs, par, H, W, cell_px=a.cell_px)
sel, soffs = ops.ground_select(cloud, offs, par, ground, H, W, a.cell_px, H_RANGE)
res = {'tiles': T, 'points': int(cloud.shape[0]), 'cell_px': a.cell_px, 'kept_points': soffs[-1], 'ground_min_tile0': float(gmin[0])}
res['raster'] = timed(lambda: ops.bev_raster_batch(cloud, offs, par, H, W, out_u8=out, u8_only=True), a.reps)
res['ground'] = timed(lambda: ops.tile_ground(cloud, offs, par, H, W, cell_px=a.cell_px), a.reps)
res['select'] = timed(lambda: ops.ground_select(cloud, offs, par, ground, H, W, a.cell_px, H_RANGE), a.reps)


def chain():
    g, _ = ops.tile_ground(cloud, offs, par, H, W, cell_px=a.cell_px)
    p, o = ops.ground_select(cloud, offs, par, g, H, W, a.cell_px, H_RANGE)
    ops.bev_raster_batch(p, o, par, H, W, out_u8=out, u8_only=True)


res['chain'] = timed(chain, a.reps)
r = res['raster']['median_ms']
res['ground_over_raster'] = res['ground']['median_ms'] / r
res['select_over_raster'] = res['select']['median_ms'] / r
res['ground_plus_select_over_raster'] = (res['ground']['median_ms'] + res['select']['median_ms']) / r
res['chain_over_raster'] = res['chain']['median_ms'] / r
npts = int(cloud.shape[0])
res['ground_frac_of_8TBps'] = 16 * npts / (res['ground']['median_ms'] * 1e-3) / 8e12
res['select_frac_of_8TBps'] = (32 * npts + 16 * soffs[-1]) / (res['select']['median_ms'] * 1e-3) / 8e12
print(json.dumps(res))
