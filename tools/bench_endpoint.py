#!/usr/bin/env python3
"""Config 2 with heads.endp_mode = 'endp_est' (off) and 'endpoint' (on: the head's own endpoint map, lm_head_endpoint) in ONE process:
pre-rasterised uint8 1152^2 tiles at batch 16 through TilePipeline (device network + decode + host polyline assembly, HIP graphs
unless --no-graphs), timed with HIP events after a warm-up, steady state.  The two settings run on the same net (cfg.heads.endp_mode
toggled, one pipeline each) and are alternated `--rounds` times, so a drift of the machine shows as a spread instead of a bias.  Then
the kernel alone, from HIP events around `--steps` back-to-back launches on the head's real operand shapes, with the fraction of the
fp32 vector peak it reaches (13.8 GMAC per batch-16 launch: 17 x 9 x 4 + 4 x 9 MACs per output pixel; peak = CUs x 128 FMA lanes
(packed fp32) x clock).  Prints one JSON line per measurement and a summary line; --out writes them to a file as well
(profiles/endpoint_mode_b16.txt).
Weights: synth.fill_module_ seed 2021 (the speed does not depend on them).

usage: bench_endpoint.py [--steps K] [--warmup W] [--batch 16] [--rounds R] [--no-graphs] [--clock-mhz F] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lanemapping_amd import ops, synth  # noqa: E402
from lanemapping_amd.boundary import build_net_from_config  # noqa: E402
from lanemapping_amd.pipeline import TilePipeline  # noqa: E402

CONFIG = 'Proj_polyline_fpn_vit_vertex_2'
MACS_PER_PIXEL = 17 * 9 * 4 + 4 * 9


def time_batch(net, pipe, mode, tiles, steps, warmup):
    net.heads.cfg.heads['endp_mode'] = mode
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


def time_kernel(net, B, dev, steps, warmup):
    h = net.heads
    col = ops.new_act(B, 16, 288, 288, dev).normal_()
    x_endp = torch.randn(B, 1, 1152, 1152, device=dev)
    out = torch.empty_like(x_endp)
    with torch.no_grad():
        packed = h._pack_endpoint()['ep']
        for _ in range(warmup):
            ops.head_endpoint(col, x_endp, packed, out=out)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            ops.head_endpoint(col, x_endp, packed, out=out)
        t1.record()
        t1.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--no-graphs', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--clock-mhz', type=float, default=2400.0, help='engine clock the vector peak is computed for (MI355X: 2400)')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    net = build_net_from_config(CONFIG, device='cpu')
    synth.fill_module_(net, 2021)
    net = net.to(dev)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    # one pipeline per setting: a captured graph bakes the mode in, and the graph key does not see cfg.heads.endp_mode
    pipes = {m: TilePipeline(net, use_graph=not a.no_graphs) for m in ('endp_est', 'endpoint')}
    best = {}
    B = a.batch
    try:
        tiles = torch.from_numpy(np.stack([synth.bev_tile_u8(3000 + i, 1152) for i in range(B)])).to(dev)
        for r in range(a.rounds):
            for m in ('endp_est', 'endpoint'):
                ms = time_batch(net, pipes[m], m, tiles, a.steps, a.warmup)
                emit({'config': CONFIG, 'endp_mode': m, 'batch': B, 'round': r, 'steps': a.steps, 'warmup': a.warmup,
                      'graphs': not a.no_graphs, 'ms_per_batch': round(ms, 3), 'tiles_per_s': round(1000.0 * B / ms, 1)})
                best[m] = min(best.get(m, ms), ms)
    finally:
        net.heads.cfg.heads['endp_mode'] = 'endp_est'
        for p in pipes.values():
            p.clear_graphs()
    kms = time_kernel(net, B, dev, a.steps, a.warmup)
    props = torch.cuda.get_device_properties(dev)
    peak = props.multi_processor_count * 128 * a.clock_mhz * 1e6          # MAC/s: 4 SIMDs x 16 lanes x 2 (packed fp32) per CU and clock
    gmac = B * 1152 * 1152 * MACS_PER_PIXEL / 1e9
    emit({'kernel': 'lm_head_endpoint', 'batch': B, 'ms': round(kms, 4), 'gmac': round(gmac, 2),
          'fraction_of_fp32_vector_peak': round(gmac * 1e9 / (kms * 1e-3) / peak, 3), 'peak_tmac_per_s': round(peak / 1e12, 1)})
    emit({'metric': 'tiles/s, config 2 with endp_mode endp_est / endpoint, same process, best of rounds',
          'tiles_per_s': {m: round(1000.0 * B / ms, 1) for m, ms in best.items()},
          'ms_added_per_batch': round(best['endpoint'] - best['endp_est'], 3),
          'fraction_of_step_added': round(best['endpoint'] / best['endp_est'] - 1.0, 4), 'kernel_ms': round(kms, 4),
          'device': torch.cuda.get_device_name(dev)})
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
