#!/usr/bin/env python3
"""Micro-bench of the chunked strip binning (ops.StripBinner: lm_strip_bin_count / lm_strip_bin_scatter) against the whole-cloud call
(ops.strip_bin_points), on tools/bench_strip.py's strip: T x N points under T overlapping tiles.

  whole      ops.strip_bin_points on the whole cloud with the capacity known: HIP events around the call
  chunks     for chunk sizes 2^24, 2^22 and 2^20 points: pass A (count every chunk, read the counts) + pass B (begin, scatter every chunk,
             finish) on slices of the same cloud, HIP events around both; `ratio` = over the whole-cloud call
  memory     torch.cuda.max_memory_allocated of one call of each, and the same above what is allocated before the call (the bench holds
             the cloud itself in both cases: a streaming caller of the chunked form holds one chunk)
  grid       the host cost of the lookup grid: per call before (one lm_strip_build_grid per whole-cloud call, and per chunk if the
             chunk entries rebuilt it), and with the plan: one lm_strip_plan_create per layout, then the host time of one
             lm_strip_bin_count enqueue per chunk
Traffic model: pass A reads 16 N, pass B reads 32 N and writes 16 sum(counts), against 32 N + 16 sum(counts) of the whole-cloud call.
Prints one JSON line.  `--reps R` (default 10)."""
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
ap.add_argument('--reps', type=int, default=10)
a = ap.parse_args()
N, T, H, W = a.points, a.tiles, 1152, 1152
dev = torch.device('cuda:0')
STEP = 50.0                                                        # 57.6 m windows every 50 m
base = [torch.from_numpy(synth.las_points(2021 + i, N)).to(dev) for i in range(4)]
cloud = torch.cat([base[i % 4] + torch.tensor([STEP * i, 0.0, 0.0, 0.0], device=dev) for i in range(T)])
del base
par = [ops.make_raster_params(trans=(STEP * i, 0.0, 0.0), local_min_ele=-0.5, ele_reso=0.02) for i in range(T)]
Ntot = cloud.shape[0]


def timed(fn, reps, warm=2):
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


def peak(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize()
    top = torch.cuda.max_memory_allocated(dev)
    del out
    return {'max_memory_allocated': top, 'above_start': top - before}


want, woffs = ops.strip_bin_points(cloud, par, H, W)
total = woffs[-1]
res = {'tiles': T, 'points': Ntot, 'binned_points': total, 'cloud_bytes': 16 * Ntot}
res['whole'] = timed(lambda: ops.strip_bin_points(cloud, par, H, W, capacity=total), a.reps)
res['whole'].update(peak(lambda: ops.strip_bin_points(cloud, par, H, W, capacity=total)))
res['whole']['model_bytes'] = 32 * Ntot + 16 * total
res['model_ratio'] = (48 * Ntot + 16 * total) / (32 * Ntot + 16 * total)


def chunked(size, binner=None):
    b = binner or ops.StripBinner(par, H, W, None, dev)
    for i in range(0, Ntot, size):
        b.count(cloud[i:i + size])
    b.counts()
    b.begin()
    for i in range(0, Ntot, size):
        b.scatter(cloud[i:i + size])
    return b.finish()


res['chunks'] = {}
for shift in (24, 22, 20):
    size = 1 << shift
    binned, offs = chunked(size)
    same = offs == woffs and bool(torch.equal(binned.view(torch.int32), want.view(torch.int32)))
    del binned
    r = timed(lambda: chunked(size), a.reps)
    r.update(peak(lambda: chunked(size)))
    r.update(chunks=-(-Ntot // size), equal_to_whole=same, ratio=r['median_ms'] / res['whole']['median_ms'])
    # the host side of one chunk with the plan in place: the enqueue of one count call (no synchronisation inside)
    b = ops.StripBinner(par, H, W, None, dev)
    b.count(cloud[:size])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        b.count(cloud[:size])
    r['count_call_host_ms'] = (time.perf_counter() - t0) / 20 * 1e3
    torch.cuda.synchronize()
    res['chunks'][f'2^{shift}'] = r
g, par_c = LmStripGrid(), (LmRasterParams * T)(*par)
t0 = time.perf_counter()
for _ in range(10):                                                # before: every call builds the grid on the host
    check(lib().lm_strip_build_grid(par_c, T, H, W, -math.inf, math.inf, C.byref(g), None, 0))
res['grid_build_host_ms_per_call_before'] = (time.perf_counter() - t0) / 10 * 1e3
t0 = time.perf_counter()
for _ in range(10):                                                # after: once per layout (grid, tile constants, upload, synchronise)
    plan = ops._StripPlan(par, H, W, -math.inf, math.inf, dev)
    del plan
res['plan_create_host_ms_once'] = (time.perf_counter() - t0) / 10 * 1e3
print(json.dumps(res))
