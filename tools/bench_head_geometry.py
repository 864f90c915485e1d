#!/usr/bin/env python3
"""ColumnProposal2 head + proposal decode per batch at each supported proposal geometry (config 2 with cfg.heads overridden):
(num_prop, prop_width, dim_shared) = (72, 2, 100) [the shipped one], (36, 4, 100), (18, 8, 100), (72, 2, 512).  The head runs on
seeded [B,8,144,144] / [B,8,288,288] inputs, then lm_decode_proposals; timed with HIP events after a warm-up, eager launches.
Prints one JSON line per geometry.  Weights: synth.fill_module_ seed 2021 (the speed does not depend on them).

usage: bench_head_geometry.py [--batch 16] [--steps K] [--warmup W]
Per-kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_head_geometry.py`."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

import cases  # noqa: E402
from lanemapping_amd import ops, synth  # noqa: E402
from lanemapping_amd.boundary import build_net_from_config, load_config  # noqa: E402

CONFIG = 'Proj_polyline_fpn_vit_vertex_2'
GEOMETRIES = ((72, 2, 100), (36, 4, 100), (18, 8, 100), (72, 2, 512))


def time_geometry(P, pw, D, B, steps, warmup, dev):
    h = dict(load_config(CONFIG).heads)
    h.update(num_prop=P, prop_width=pw, dim_shared=D)
    net = build_net_from_config(CONFIG, device='cpu', heads=h)
    synth.fill_module_(net, 2021)
    head = net.heads.to(dev)
    x, x_up = cases.head_inputs(41, batch=B)
    x = torch.from_numpy(x).to(dev).contiguous(memory_format=torch.channels_last)
    x_up = torch.from_numpy(x_up).to(dev)
    thre = float(head.cfg.exist_thre)

    def step():
        o = head._forward_impl(x, x_up)
        return ops.decode_proposals(o['proposal_conf'], o['ext2'], o['cls2'], o['offset2'], thre, pw, head.prop_half_buff)
    with torch.no_grad():
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            step()
        t1.record()
        t1.synchronize()
    ms = t0.elapsed_time(t1) / steps
    return {'num_prop': P, 'prop_width': pw, 'prop_fea_width': pw + 8, 'dim_shared': D, 'batch': B, 'steps': steps, 'warmup': warmup,
            'ms_head_plus_decode_per_batch': round(ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    for P, pw, D in GEOMETRIES:
        print(json.dumps(time_geometry(P, pw, D, a.batch, a.steps, a.warmup, dev)), flush=True)


if __name__ == '__main__':
    main()
