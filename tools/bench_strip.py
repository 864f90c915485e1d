#!/usr/bin/env python3
"""Micro-bench of the strip binning (csrc/strip.hip): one cloud of T x N points over a strip of T overlapping tiles.

  bin        ops.strip_bin_points: HIP events around the whole call (count, scan, offsets read-back, scatter; the host-side grid build
             and the one synchronisation are inside), against the compulsory bytes 16 Ntot + 16 Ntot + 16 sum(counts) at 8 TB/s
  raster     ops.bev_raster_batch on the binned ranges (the stage the binning feeds), same process
  strip      bin + raster
  whole      the route without the binning: every tile rasterised from the whole cloud (T launches over Ntot points each)
Prints one JSON line.  `--reps R` (default 20), `--no-whole` skips the last route (for a profiler run of the binning kernels)."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lanemapping_amd import ops, synth  # noqa: E402
from lanemapping_amd._lib import LmRasterParams, LmStripGrid, check, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=int, default=4194304, help='points per tile-sized piece of the strip')
ap.add_argument('--tiles', type=int, default=16)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--no-whole', action='store_true')
a = ap.parse_args()
N, T, H, W = a.points, a.tiles, 1152, 1152
dev = torch.device('cuda:0')
STEP = 50.0                                                        # 57.6 m windows every 50 m
base = [torch.from_numpy(synth.las_points(2021 + i, N)).to(dev) for i in range(4)]
cloud = torch.cat([base[i % 4] + torch.tensor([STEP * i, 0.0, 0.0, 0.0], device=dev) for i in range(T)])
del base
par = [ops.make_raster_params(trans=(STEP * i, 0.0, 0.0), local_min_ele=-0.5, ele_reso=0.02) for i in range(T)]
Ntot = cloud.shape[0]


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


binned, offs = ops.strip_bin_points(cloud, par, H, W)
total = offs[-1]
out = torch.empty((T, H, W, 3), device=dev, dtype=torch.uint8)
res = {'tiles': T, 'points': Ntot, 'binned_points': total, 'capacity_first_guess': Ntot + Ntot // 4}
res['bin'] = timed(lambda: ops.strip_bin_points(cloud, par, H, W, capacity=total), a.reps)
g, par_c = LmStripGrid(), (LmRasterParams * T)(*par)
t0 = time.perf_counter()
for _ in range(10):                                                # the host part of a call: one build of the lookup grid
    check(lib().lm_strip_build_grid(par_c, T, H, W, -math.inf, math.inf, C.byref(g), None, 0))
res['grid_build_host_ms'] = (time.perf_counter() - t0) / 10 * 1e3
res['raster'] = timed(lambda: ops.bev_raster_batch(binned, offs, par, H, W, out_u8=out, u8_only=True), a.reps)


def strip():
    b, o = ops.strip_bin_points(cloud, par, H, W, capacity=total)
    ops.bev_raster_batch(b, o, par, H, W, out_u8=out, u8_only=True)


res['strip'] = timed(strip, a.reps)
nbytes = 16 * Ntot + 16 * Ntot + 16 * total
res['bin_compulsory_bytes'] = nbytes
res['bin_frac_of_8TBps'] = nbytes / (res['bin']['median_ms'] * 1e-3) / 8e12
res['bin_over_raster'] = res['bin']['median_ms'] / res['raster']['median_ms']
if not a.no_whole:
    ref = out.clone()
    one = torch.empty((1, H, W, 3), device=dev, dtype=torch.uint8)

    def whole():
        for t in range(T):
            ops.bev_raster_batch(cloud, [0, Ntot], [par[t]], H, W, out_u8=one, u8_only=True)

    res['whole'] = timed(whole, a.reps)
    res['whole_over_strip'] = res['whole']['median_ms'] / res['strip']['median_ms']
    res['last_tile_equal'] = bool(torch.equal(one[0], ref[T - 1]))
print(json.dumps(res))
