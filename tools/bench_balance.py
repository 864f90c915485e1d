#!/usr/bin/env python3
"""Micro-bench of the intensity balance (csrc/intensity.hip) on the bench's synthetic clouds: T tiles of N points each.

  raster     ops.bev_raster_batch on the batch (the stage the balance sits in front of), the yardstick of the ratios
  window     ops.tile_intensity_window with every tile its own window, the neighbouring stage of the same two-pass shape
  cells      ops.tile_intensity_cells, the whole call: memset of the counters, coarse pass, locate, fine pass, level, model
  apply      ops.tile_intensity_apply into a second buffer (the same kernel as in place; the input keeps its values over the repetitions)
  both       cells, the model read back, las_io.balance_gains on the host, the gains uploaded, apply: what the runner adds per batch
Each on the cloud AS DRAWN (acquisition order: the 64 points of a wave fall into 64 cells) and IN CELL ORDER (every tile's points sorted
by their cell, as a scanner delivers consecutive returns: the lanes of a wave share a cell and, among asphalt, often a counter).
Whole-call times are HIP events around each call, median of `--reps` (default 20) after 3 warm-up calls; `passes` are the device times
of the kernels of one profiled cells call (torch.profiler's device records).  Prints JSON lines."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lanemapping_amd import las_io, ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=int, default=4194304, help='points per tile')
ap.add_argument('--tiles', type=int, default=16)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--cell-px', type=int, default=32)
a = ap.parse_args()
N, T, H, W, CELL = a.points, a.tiles, 1152, 1152, a.cell_px
dev = torch.device('cuda:0')
offs = [N * i for i in range(T + 1)]
par = [ops.make_raster_params(local_min_ele=-0.5, ele_reso=0.02) for _ in range(T)]
st = las_io.IntensityStretch(balance=True, cell_px=CELL)


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
    """{kernel: device microseconds} of one profiled call."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    found = {}
    for e in prof.events():
        if 'cells_' not in e.name and 'balance_apply' not in e.name:
            continue
        us = float(getattr(e, 'device_time', 0.0) or getattr(e, 'cuda_time', 0.0))
        if 'cells_count_kernel' in e.name:
            name = 'fine' if ('ILb1' in e.name or '<true>' in e.name) else 'coarse'
        else:
            name = next((k for k in ('locate', 'level', 'model', 'apply') if k in e.name), e.name)
        found[name + '_us'] = found.get(name + '_us', 0.0) + us
    return found


def in_cell_order(tile):
    """The points of one tile (identity frame, 0.05 m pixels) sorted by their cell; points outside the window last."""
    row, col = torch.floor(tile[:, 0] / 0.05 + 0.5), torch.floor(tile[:, 1] / 0.05 + 0.5)
    inside = (row >= 0) & (row < H) & (col >= 0) & (col < W)
    gx = -(-W // CELL)
    cell = torch.where(inside, torch.div(row, CELL, rounding_mode='floor') * gx + torch.div(col, CELL, rounding_mode='floor'),
                       torch.full_like(row, float(gx * gx)))
    return tile[torch.argsort(cell, stable=True)]


def both(cloud):
    _, count, model = ops.tile_intensity_cells(cloud, offs, par, H, W, cell_px=CELL, min_points=st.cell_min_points)
    gains = las_io.balance_gains(model.cpu().numpy(), [4000] * T, st)
    return ops.tile_intensity_apply(cloud, offs, par, torch.from_numpy(gains).to(dev), H, W, cell_px=CELL, out=scratch)


base = [torch.from_numpy(synth.las_points(2021 + i, N)).to(dev) for i in range(4)]
scratch = torch.empty((N * T, 4), device=dev, dtype=torch.float32)
out = torch.empty((T, H, W, 3), device=dev, dtype=torch.uint8)
npts = N * T
for order in ('as_drawn', 'cell_order'):
    tiles = base if order == 'as_drawn' else [in_cell_order(b) for b in base]
    cloud = torch.cat([tiles[i % 4] for i in range(T)])
    del tiles
    _, count, model = ops.tile_intensity_cells(cloud, offs, par, H, W, cell_px=CELL, min_points=st.cell_min_points)
    gains = torch.from_numpy(las_io.balance_gains(model.cpu().numpy(), [4000] * T, st)).to(dev)
    res = {'order': order, 'tiles': T, 'points': npts, 'cell_px': CELL, 'known_cells_tile0': int((count[0] >= st.cell_min_points).sum()),
           'model_tile0_range': [int(model[0].min()), int(model[0].max())]}
    res['raster'] = timed(lambda: ops.bev_raster_batch(cloud, offs, par, H, W, out_u8=out, u8_only=True), a.reps)
    res['window'] = timed(lambda: ops.tile_intensity_window(cloud, offs, par, H, W, (1.0, 99.9)), a.reps)
    res['cells'] = timed(lambda: ops.tile_intensity_cells(cloud, offs, par, H, W, cell_px=CELL, min_points=st.cell_min_points), a.reps)
    res['apply'] = timed(lambda: ops.tile_intensity_apply(cloud, offs, par, gains, H, W, cell_px=CELL, out=scratch), a.reps)
    res['both'] = timed(lambda: both(cloud), a.reps)
    for k in ('cells', 'apply', 'both'):
        res[k + '_over_raster'] = res[k]['median_ms'] / res['raster']['median_ms']
        res[k + '_over_window'] = res[k]['median_ms'] / res['window']['median_ms']
    res['cells_frac_of_8TBps'] = 32 * npts / (res['cells']['median_ms'] * 1e-3) / 8e12
    res['apply_frac_of_8TBps'] = 32 * npts / (res['apply']['median_ms'] * 1e-3) / 8e12
    print(json.dumps(res), flush=True)
    print(json.dumps({'order': order, 'passes': passes(lambda: both(cloud))}), flush=True)
    del cloud
