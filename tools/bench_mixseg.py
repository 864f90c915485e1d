#!/usr/bin/env python3
"""Config 2 (ViT backbone) vs the MLP-Mixer config (MixSegNet backbone, spatial_att=False head) in ONE process: pre-rasterised
uint8 1152^2 tiles at batch 8 and 16 through TilePipeline (device network + decode + host polyline assembly), timed with HIP events
after a warm-up, steady state.  Prints one JSON line per (config, batch) and a summary line with the MixSeg / config-2 tiles/s ratio.
Weights: synth.fill_module_ seed 2021 (the speed does not depend on them).

usage: bench_mixseg.py [--steps K] [--warmup W] [--batches 8 16] [--no-graphs]
Per-kernel times of the token-mixing kernel: run this under `rocprofv3 --kernel-trace --stats`."""
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

CONFIGS = ('Proj_polyline_fpn_vit_vertex_2', 'Proj_polyline_fpn_mixseg_vertex')


def time_config(name, batches, steps, warmup, use_graph, dev):
    net = build_net_from_config(name, device='cpu')
    synth.fill_module_(net, 2021)
    net = net.to(dev)
    pipe = TilePipeline(net, use_graph=use_graph)
    out = []
    for B in batches:
        tiles = torch.from_numpy(np.stack([synth.bev_tile_u8(3000 + i, 1152) for i in range(B)])).to(dev)
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
        ms = t0.elapsed_time(t1) / steps
        out.append({'config': name, 'batch': B, 'steps': steps, 'warmup': warmup, 'graphs': use_graph,
                    'ms_per_batch': round(ms, 3), 'tiles_per_s': round(1000.0 * B / ms, 1)})
        print(json.dumps(out[-1]), flush=True)
    pipe.clear_graphs()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batches', type=int, nargs='+', default=[8, 16])
    ap.add_argument('--no-graphs', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    res = {}
    for name in CONFIGS:
        for r in time_config(name, a.batches, a.steps, a.warmup, not a.no_graphs, dev):
            res[(name, r['batch'])] = r['tiles_per_s']
    summary = {'metric': 'tiles/s, MixSeg config vs config 2, same process',
               'ratio_mixseg_over_config2': {str(B): round(res[(CONFIGS[1], B)] / res[(CONFIGS[0], B)], 3) for B in a.batches},
               'tiles_per_s': {f'{n}@B{B}': v for (n, B), v in res.items()}, 'device': torch.cuda.get_device_name(dev)}
    print(json.dumps(summary), flush=True)


if __name__ == '__main__':
    main()
