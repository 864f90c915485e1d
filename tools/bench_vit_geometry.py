#!/usr/bin/env python3
"""VitSegNet (GFC-T) at each supported patch size, on one MI355X: writes profiles/vit_geometry_b16.txt (and prints it).

  * lm_attention_f32 per launch at N = 324 (patch 8, attention_mfma_kernel) and N = 576 / 1296 (patches 6 / 4) and 2304
    (attention_flash_kernel), B = 16, 16 heads, and its share of the fp32 MFMA peak (157.3 TF/s) in 4 B heads N^2 64 FLOP;
  * lm_layernorm_rows per launch at the widths of patches 8 / 4 / 6 / 12 / 16 (B x tokens rows);
  * the backbone (config 2 with cfg.backbone overridden, dim = 8 p^2) per batch of 16;
  * TilePipeline tiles/s on config 2 at patches 8 / 6 / 4, batch 16, graph replay as the headline bench uses it.
Times: HIP events around `steps` back-to-back launches after `warmup` (eager launches).  Weights: synth.fill_module_ seed 2021.

usage: bench_vit_geometry.py [--steps K] [--warmup W] [--out profiles/vit_geometry_b16.txt]"""
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
FP32_MFMA_PEAK = 157.3e12
PATCH_DIM = {8: 512, 4: 128, 6: 288, 12: 1152, 16: 2048}


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / steps


def _net(p, dev):
    b = dict(load_config(CONFIG).backbone)
    b.update(patch_h_size=p, patch_w_size=p, dim=PATCH_DIM[p])
    net = build_net_from_config(CONFIG, device='cpu', backbone=b)
    synth.fill_module_(net, 2021)
    return net.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vit_geometry_b16.txt'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    g = torch.Generator().manual_seed(7)
    lines = [f'# VitSegNet geometries on one MI355X (tools/bench_vit_geometry.py, HIP events, {a.steps} steps after {a.warmup} warm-up)']
    B, heads = 16, 16
    with torch.no_grad():
        for N in (324, 576, 1296, 2304):
            qkv = (torch.randn((B * N, 3 * heads * 64), generator=g) * 3).to(dev)
            ms = _time(lambda: ops.attention(qkv, B, N, heads, 64, 0.125), a.steps, a.warmup)
            flop = 4.0 * B * heads * N * N * 64
            lines.append(json.dumps({'op': 'attention', 'kernel': 'attention_mfma_kernel' if N == 324 else 'attention_flash_kernel',
                                     'N': N, 'B': B, 'heads': heads, 'us_per_launch': round(ms * 1e3, 1),
                                     'tflops': round(flop / ms / 1e9, 2), 'frac_fp32_mfma_peak': round(flop / ms / 1e-3 / FP32_MFMA_PEAK, 3)}))
        for p, D in PATCH_DIM.items():
            rows = B * (144 // p) ** 2
            x = torch.randn((rows, D), generator=g).to(dev)
            gm, bt = torch.randn(D, generator=g).to(dev), torch.randn(D, generator=g).to(dev)
            ms = _time(lambda: ops.layernorm(x, gm, bt, 1e-5), a.steps, a.warmup)
            lines.append(json.dumps({'op': 'layernorm', 'D': D, 'rows': rows, 'us_per_launch': round(ms * 1e3, 1),
                                     'GB_per_s': round(2 * 4 * rows * D / ms / 1e6, 1)}))
        fea = torch.from_numpy(cases.vit_input(31)).repeat(B, 1, 1, 1).to(dev)
        for p in PATCH_DIM:
            bb = _net(p, dev).backbone
            ms = _time(lambda: bb(fea), a.steps, a.warmup)
            lines.append(json.dumps({'op': 'backbone', 'patch': p, 'dim': PATCH_DIM[p], 'tokens': (144 // p) ** 2, 'batch': B,
                                     'ms_per_batch': round(ms, 3)}))
    from lanemapping_amd.pipeline import TilePipeline
    x = torch.from_numpy(synth.bev_batch(list(range(2021, 2021 + B)), 1152)).to(dev)
    for p in (8, 6, 4):
        pipe = TilePipeline(_net(p, dev), use_graph=True)
        ms = _time(lambda: pipe.run_batch(x), max(5, a.steps // 3), 2)
        pipe.clear_graphs()
        lines.append(json.dumps({'op': 'TilePipeline', 'patch': p, 'dim': PATCH_DIM[p], 'batch': B, 'graphs': True,
                                 'tiles_per_s': round(B / ms * 1e3, 1)}))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
