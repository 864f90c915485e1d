#!/usr/bin/env python3
"""State-dict layouts of the reference's RowSharNotReducRef head (config 4) at every `off_grid` in 1..4 and both
`is_reuse_same_network` settings, produced by building the upstream reference's module on CPU through the same loader as make_golden.py.

    python tests/golden/make_golden_rowref_geometry.py

Writes rowref_geometry_keys.json: {"og<off_grid>_reuse<0|1>": {"off_grid", "is_reuse_same_network", "state_dict": [[name, shape], ...]}}.
Names and shapes only, no values.  The `emb_<c>` entries are left out: the reference makes them with `nn.Parameter(...).cuda()` (:140),
plain tensors on a real GPU that never reach a checkpoint; only the loader's CPU stub of `.cuda()` keeps them Parameters.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402
import make_golden  # noqa: E402  (puts the repo root on sys.path)

CONFIG = 'configs/Proj28_GFC-T3_RowRef_82_73_laser.py'
OFF_GRIDS = (1, 2, 3, 4)


def layout(off_grid, reuse):
    cfg = make_golden._refload.load_cfg(CONFIG, vit_seg=True, is_gt_avai=False)
    heads = dict(cfg.heads)
    heads['off_grid'] = off_grid
    heads['is_reuse_same_network'] = reuse
    cfg.heads = heads
    from baseline.models.registry import build_heads
    torch.manual_seed(2021)
    head = build_heads(cfg)
    assert head.off_grid == off_grid and hasattr(head, 'ext2_0') != reuse
    return [[k, list(v.shape)] for k, v in head.state_dict().items() if not re.fullmatch(r'emb_\d+', k)]


def main():
    out = {}
    for og in OFF_GRIDS:
        for reuse in (False, True):
            tag = f'og{og}_reuse{int(reuse)}'
            out[tag] = {'off_grid': og, 'is_reuse_same_network': reuse, 'state_dict': layout(og, reuse)}
            print(f'  {tag}: {len(out[tag]["state_dict"])} state-dict entries')
    path = os.path.join(HERE, 'rowref_geometry_keys.json')
    with open(path, 'w') as f:
        json.dump(out, f)
        f.write('\n')
    print('wrote rowref_geometry_keys.json', os.path.getsize(path))


if __name__ == '__main__':
    main()
