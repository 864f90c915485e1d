#!/usr/bin/env python3
"""Config 2 with column_att off and on (ColumnProposal2's proposal-attention branch) in ONE process: pre-rasterised uint8 1152^2 tiles
at batch 8 and 16 through TilePipeline (device network + decode + host polyline assembly, HIP graphs unless --no-graphs), timed with
HIP events after a warm-up, steady state.  The two settings run on the same net (cfg.column_att toggled, one pipeline each) and are
alternated `--rounds` times, so a drift of the machine shows as a spread instead of a bias.  Prints one JSON line per (setting, batch,
round) and a summary line with the best tiles/s of each setting and the time the branch adds per batch.
Weights: synth.fill_module_ seed 2021 (the speed does not depend on them).

usage: bench_colatt.py [--steps K] [--warmup W] [--batches 8 16] [--rounds R] [--no-graphs]
Per-kernel times of the branch: run this under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lanemapping_amd import synth  # noqa: E402
from lanemapping_amd.boundary import build_net_from_config  # noqa: E402
from lanemapping_amd.pipeline import TilePipeline  # noqa: E402

CONFIG = 'Proj_polyline_fpn_vit_vertex_2'


def time_batch(net, pipe, att, tiles, steps, warmup):
    net.heads.cfg.column_att = att
    with torch.no_grad():
        for _ in range(warmup):
            pipe.run_batch(tiles)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            pipe.run_batch(tiles)
        t1.record()
        t1.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batches', type=int, nargs='+', default=[8, 16])
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--no-graphs', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    net = build_net_from_config(CONFIG, device='cpu')
    synth.fill_module_(net, 2021)
    net = net.to(dev)
    # one pipeline per setting: a captured graph bakes the branch in, and the graph key does not see cfg.column_att
    pipes = {att: TilePipeline(net, use_graph=not a.no_graphs) for att in (False, True)}
    best = {}
    try:
        for B in a.batches:
            tiles = torch.from_numpy(np.stack([synth.bev_tile_u8(3000 + i, 1152) for i in range(B)])).to(dev)
            for r in range(a.rounds):
                for att in (False, True):
                    ms = time_batch(net, pipes[att], att, tiles, a.steps, a.warmup)
                    rec = {'config': CONFIG, 'column_att': att, 'batch': B, 'round': r, 'steps': a.steps, 'warmup': a.warmup,
                           'graphs': not a.no_graphs, 'ms_per_batch': round(ms, 3), 'tiles_per_s': round(1000.0 * B / ms, 1)}
                    print(json.dumps(rec), flush=True)
                    k = (att, B)
                    best[k] = min(best.get(k, ms), ms)
    finally:
        net.heads.cfg.column_att = False
        for p in pipes.values():
            p.clear_graphs()
    summary = {'metric': 'tiles/s, config 2 with column_att off / on, same process, best of rounds',
               'tiles_per_s': {f'column_att={att}@B{B}': round(1000.0 * B / ms, 1) for (att, B), ms in best.items()},
               'ms_added_per_batch': {str(B): round(best[(True, B)] - best[(False, B)], 3) for B in a.batches},
               'device': torch.cuda.get_device_name(dev)}
    print(json.dumps(summary), flush=True)


if __name__ == '__main__':
    main()
