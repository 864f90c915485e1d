#!/usr/bin/env python3
"""Micro-bench of the intensity window (csrc/intensity.hip) on the bench's synthetic clouds: T tiles of N points each.

  raster     ops.bev_raster_batch on the batch (the stage the window sits in front of), the yardstick of the ratios
  window     ops.tile_intensity_window, the whole call (memsets, coarse pass, locate, fine pass, resolve), with G = T (every tile its own
             window) and G = 1 (one window for the strip)
  equal      the same call on a cloud whose intensities are all equal: every point of a wave on one LDS counter, the worst case for
             same-address collisions
  passes     device times of the four kernels of one call each, coarse = inten_count_kernel<false>, fine = inten_count_kernel<true>.
             The C entry launches its kernels back to back and takes no event arguments, so HIP events from outside can only bracket
             the whole call; the per-kernel times therefore come from torch.profiler's device activity records (the same device
             timestamps a kernel trace reports) of one profiled call after the timed runs.  This step runs LAST and fails loudly - a
             traceback and a non-zero exit - when the profiler yields no record for the coarse or the fine pass; the line with the
             event times is printed before it.
Whole-call times are HIP events around each call, median of `--reps` (default 20) after 3 warm-up calls.  Prints two JSON lines: the
event times and ratios, then the per-kernel times."""
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
cloud = torch.cat([base[i % 4] for i in range(T)])
del base
offs = [N * i for i in range(T + 1)]
par = [ops.make_raster_params(local_min_ele=-0.5, ele_reso=0.02) for _ in range(T)]
PCT = (1.0, 99.9)


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


def passes(fn):
    """{pass: device microseconds} of one profiled call; the kernels are told apart by their template argument in the (mangled or
    demangled) kernel name.  Raises when the coarse or the fine pass is not among the profiler's device records."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    found = {}
    for e in prof.events():
        if 'inten_' not in e.name:
            continue
        us = float(getattr(e, 'device_time', 0.0) or getattr(e, 'cuda_time', 0.0))
        if 'inten_count_kernel' in e.name:
            fine = 'ILb1' in e.name or '<true>' in e.name
            assert fine or 'ILb0' in e.name or '<false>' in e.name, f'cannot tell the pass of kernel {e.name!r}'
            name = 'fine' if fine else 'coarse'
        else:
            name = 'locate' if 'locate' in e.name else 'resolve' if 'resolve' in e.name else e.name
        found[name + '_us'] = found.get(name + '_us', 0.0) + us
    if not (found.get('coarse_us', 0.0) > 0.0 and found.get('fine_us', 0.0) > 0.0):
        raise RuntimeError(f'torch.profiler gave no device time for the coarse / fine pass: {found}')
    return found


out = torch.empty((T, H, W, 3), device=dev, dtype=torch.uint8)
one = [0] * T
win, cnt = ops.tile_intensity_window(cloud, offs, par, H, W, PCT)
res = {'tiles': T, 'points': int(cloud.shape[0]), 'percentiles': PCT, 'window_tile0': win[0].tolist(), 'count_tile0': int(cnt[0])}
res['raster'] = timed(lambda: ops.bev_raster_batch(cloud, offs, par, H, W, out_u8=out, u8_only=True), a.reps)
res['window_G_tiles'] = timed(lambda: ops.tile_intensity_window(cloud, offs, par, H, W, PCT), a.reps)
res['window_G_1'] = timed(lambda: ops.tile_intensity_window(cloud, offs, par, H, W, PCT, group=one), a.reps)
cloud[:, 3] = 33000.0
res['equal_G_tiles'] = timed(lambda: ops.tile_intensity_window(cloud, offs, par, H, W, PCT), a.reps)
res['equal_G_1'] = timed(lambda: ops.tile_intensity_window(cloud, offs, par, H, W, PCT, group=one), a.reps)
r = res['raster']['median_ms']
for k in ('window_G_tiles', 'window_G_1', 'equal_G_tiles', 'equal_G_1'):
    res[k + '_over_raster'] = res[k]['median_ms'] / r
res['equal_over_synthetic_G_tiles'] = res['equal_G_tiles']['median_ms'] / res['window_G_tiles']['median_ms']
res['equal_over_synthetic_G_1'] = res['equal_G_1']['median_ms'] / res['window_G_1']['median_ms']
npts = int(cloud.shape[0])
res['window_frac_of_8TBps'] = 32 * npts / (res['window_G_tiles']['median_ms'] * 1e-3) / 8e12
print(json.dumps(res), flush=True)
per = {'passes_equal_G_tiles': passes(lambda: ops.tile_intensity_window(cloud, offs, par, H, W, PCT))}
del cloud
base = [torch.from_numpy(synth.las_points(2021 + i, N)).to(dev) for i in range(4)]
cloud = torch.cat([base[i % 4] for i in range(T)])
del base
per['passes_G_tiles'] = passes(lambda: ops.tile_intensity_window(cloud, offs, par, H, W, PCT))
per['passes_G_1'] = passes(lambda: ops.tile_intensity_window(cloud, offs, par, H, W, PCT, group=one))
print(json.dumps(per))
