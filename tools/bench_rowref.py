#!/usr/bin/env python3
"""Micro-bench of the config-4 path (Proj28_GFC-T3_RowRef): B pre-rasterised tiles -> FPN -> ViT -> RowSharNotReducRef ->
decode -> per-lane line tracing.  Prints stage times and tiles/s as one JSON line for config 4's own head (off_grid = 2, separate
second-stage networks) and, with --off-grid / --reuse, a second line for the chosen head geometry and a summary line with both rates
side by side (same process, same tiles, the chosen setting after config 4's own).  --out writes the lines to a file as well
(profiles/rowref_geometry.txt).
Weights: synth.fill_module_ seed 2021 (the speed does not depend on them, except through the number of lanes the head selects).

usage: bench_rowref.py [B] [--off-grid 1..4] [--reuse] [--rep N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lanemapping_amd import synth  # noqa: E402
from lanemapping_amd.boundary import build_net_from_config, load_config  # noqa: E402

CONFIG = 'Proj28_GFC-T3_RowRef_82_73_laser'


def timed(fn, rep=3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(rep):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / rep * 1e3, out


def measure(x, dev, rep, off_grid=None, reuse=None):
    heads = dict(load_config(CONFIG).heads)
    if off_grid is not None:
        heads['off_grid'] = off_grid
    if reuse is not None:
        heads['is_reuse_same_network'] = reuse
    net = build_net_from_config(CONFIG, device='cpu', heads=heads)
    synth.fill_module_(net, 2021)
    net = net.to(dev)
    B = x.shape[0]
    with torch.no_grad():
        t_enc, enc = timed(lambda: net.pcencoder({'proj': x}), rep)
        t_vit, fea = timed(lambda: net.backbone(enc[0]), rep)
        t_head, _ = timed(lambda: net.heads(fea), rep)
        t_raw, _ = timed(lambda: net.forward_raw({'proj': x}), rep)
        t_full, _ = timed(lambda: net({'proj': x}), rep=max(rep - 1, 1))
    return {'off_grid': net.heads.off_grid, 'is_reuse_same_network': net.heads.is_reuse_same_network, 'tiles': B, 'ms_fpn': t_enc,
            'ms_vit': t_vit, 'ms_rowref_head': t_head, 'ms_forward_raw': t_raw, 'ms_full_forward': t_full,
            'tiles_per_s_raw': B / t_raw * 1e3, 'tiles_per_s_full': B / t_full * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('tiles', nargs='?', type=int, default=8)
    ap.add_argument('--off-grid', type=int, default=None, help='heads.off_grid of the second measurement (1..4)')
    ap.add_argument('--reuse', action='store_true', help='heads.is_reuse_same_network = True in the second measurement')
    ap.add_argument('--rep', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    x = torch.from_numpy(synth.bev_batch([2021 + i for i in range(a.tiles)], 1152)).to(dev)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    own = measure(x, dev, a.rep)
    emit(own)
    if a.off_grid is not None or a.reuse:
        chosen = measure(x, dev, a.rep, off_grid=a.off_grid, reuse=a.reuse)
        emit(chosen)
        emit({'metric': 'tiles/s, config 4 with its own head / the chosen head geometry, same process',
              'config4': {'off_grid': own['off_grid'], 'is_reuse_same_network': own['is_reuse_same_network'],
                          'tiles_per_s_raw': round(own['tiles_per_s_raw'], 1), 'tiles_per_s_full': round(own['tiles_per_s_full'], 1)},
              'chosen': {'off_grid': chosen['off_grid'], 'is_reuse_same_network': chosen['is_reuse_same_network'],
                         'tiles_per_s_raw': round(chosen['tiles_per_s_raw'], 1), 'tiles_per_s_full': round(chosen['tiles_per_s_full'], 1)},
              'ms_rowref_head': {'config4': round(own['ms_rowref_head'], 3), 'chosen': round(chosen['ms_rowref_head'], 3)},
              'tiles': a.tiles, 'device': torch.cuda.get_device_name(dev)})
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
