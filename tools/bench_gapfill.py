#!/usr/bin/env python3
"""Micro-bench of the gap fill (csrc/gapfill.hip) on T tiles of 1152 x 1152 pixels, at max_radius_px 4 and 8, on three inputs:

  dense    the bench's synthetic clouds, N points per tile, rasterised (about three returns per pixel: almost nothing to fill)
  sparse   the same clouds thinned to one point in sixteen
  empty    tiles without a return: no block finds a source in its staged area, so every block skips the walk
and, per input and radius:
  hist     ops.tile_gap_hist(tiles, R)
  fill     ops.tile_gap_fill(tiles, R) (every tile at the full radius: the most the fill can cost)
  both     the two one after the other, as Runner's density= issues them (without its read-back of the histograms)
against raster = ops.bev_raster_batch(u8_only=True) of the dense clouds in the same process, the yardstick of the ratios.  Times are HIP
events around each call, median of `--reps` (default 20) after 3 warm-up calls.  Prints one JSON line."""
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
ap.add_argument('--reps', type=int, default=20)
a = ap.parse_args()
N, T, H, W = a.points, a.tiles, 1152, 1152
dev = torch.device('cuda:0')
base = [torch.from_numpy(synth.las_points(2021 + i, N)).to(dev) for i in range(4)]
par = [ops.make_raster_params(local_min_ele=-0.5, ele_reso=0.02) for _ in range(T)]


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


def rasterised(step):
    clouds = [b[::step].contiguous() for b in base]
    n = clouds[0].shape[0]
    cloud = torch.cat([clouds[i % 4] for i in range(T)])
    return cloud, [n * i for i in range(T + 1)]


cloud, offs = rasterised(1)
out = torch.empty((T, H, W, 3), device=dev, dtype=torch.uint8)
res = {'tiles': T, 'points_per_tile': N}
res['raster'] = timed(lambda: ops.bev_raster_batch(cloud, offs, par, H, W, out_u8=out, u8_only=True), a.reps)
inputs = {'dense': ops.bev_raster_batch(cloud, offs, par, H, W, u8_only=True)}
del cloud
thin, thin_offs = rasterised(16)
inputs['sparse'] = ops.bev_raster_batch(thin, thin_offs, par, H, W, u8_only=True)
inputs['empty'] = torch.zeros((T, H, W, 3), device=dev, dtype=torch.uint8)
del thin, base
for name, tiles in inputs.items():
    res[name] = {'non_empty': float((tiles.view(-1, 3).max(dim=1).values > 0).float().mean())}
    for R in (4, 8):
        r = res[name][f'R{R}'] = {'hist_row0': ops.tile_gap_hist(tiles, R)[0].tolist()}
        r['hist'] = timed(lambda: ops.tile_gap_hist(tiles, R), a.reps)
        r['fill'] = timed(lambda: ops.tile_gap_fill(tiles, R), a.reps)
        r['both'] = timed(lambda: (ops.tile_gap_hist(tiles, R), ops.tile_gap_fill(tiles, R)), a.reps)
        for k in ('hist', 'fill', 'both'):
            r[f'{k}_over_raster'] = r[k]['median_ms'] / res['raster']['median_ms']
        # bytes the algorithm needs: the tiles read once per entry, written once by the fill
        r['both_frac_of_8TBps'] = 3 * 3 * T * H * W / (r['both']['median_ms'] * 1e-3) / 8e12
print(json.dumps(res))
