#!/usr/bin/env python3
"""Golden vectors of the GFC-T backbone (VitSegNet) at the other patch sizes the reference's config schema offers
(`patch_h_size = patch_w_size = 4, 6, 12, 16`, dim = 8 p^2 so that the backbone still hands the head 8 channels), produced by the
upstream reference on CPU through the same harness as make_golden.py / make_golden_propgeom.py.

    python tests/golden/make_golden_vitgeom.py [p4 p6 p12 p16 p4_mlp]

Geometries (GEOMETRIES): config 2 with cfg.backbone overridden.  Per geometry one g26_vitgeom_<tag>.npz holding
  bb_*    the backbone on cases.vit_input(31) and on the batch of two (32, 33), floats sampled (the G21 pattern);
  e2e_*   for p4 and p6, one 1152^2 tile through the whole reference net, decisions whole with their margin lists (the G10 / G23 /
          G25 pattern, make_golden_propgeom.e2e).
g26_vitgeom_layout.json holds each geometry's state-dict layout as the reference net builds it (the G20 / G24 / G25 pattern).
Weights: synth.fill_module_ with seed 2021; inputs from the seeded generators, so the fixtures hold seeds and expected outputs only.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402
import make_golden  # noqa: E402  (puts the repo root on sys.path)
from make_golden import ref_net, save, cases  # noqa: E402
from make_golden_mixseg import sampled, BATCH2_SEEDS  # noqa: E402
from make_golden_propgeom import e2e  # noqa: E402

CONFIG2 = 'Proj_polyline_fpn_vit_vertex_2'
# tag -> backbone overrides
GEOMETRIES = {
    'p4': dict(patch_h_size=4, patch_w_size=4, dim=128),
    'p6': dict(patch_h_size=6, patch_w_size=6, dim=288),
    'p12': dict(patch_h_size=12, patch_w_size=12, dim=1152),
    'p16': dict(patch_h_size=16, patch_w_size=16, dim=2048),
    'p4_mlp': dict(patch_h_size=4, patch_w_size=4, dim=512, is_with_shared_mlp=True, output_channels=8),
}
E2E = ('p4', 'p6')
BB = dict(n_samples=4096, n_chunks=512)


def backbone(net):
    x = torch.from_numpy(cases.vit_input(31))
    x2 = torch.from_numpy(np.concatenate([cases.vit_input(s) for s in BATCH2_SEEDS]))
    with torch.no_grad():
        y, y2 = net.backbone(x), net.backbone(x2)
    assert y.shape[1] == 8 and y.shape[2:] == (144, 144), y.shape
    return {**sampled('bb_out', y, **BB), **sampled('bb_out_batch2', y2, **BB)}


def main():
    which = sys.argv[1:] or list(GEOMETRIES)
    make_golden._stable_sorts(True)
    path = os.path.join(HERE, 'g26_vitgeom_layout.json')
    layouts = json.load(open(path)) if os.path.exists(path) else {}
    for tag in which:
        over = GEOMETRIES[tag]
        print('==', tag, over)
        cfg0 = make_golden._refload.load_cfg(f'configs/{CONFIG2}.py')
        bb = dict(cfg0.backbone)
        bb.update(over)
        cfg, net = ref_net(f'configs/{CONFIG2}.py', backbone=bb)
        b = net.backbone
        assert b.to_patch_embedding[1].in_features == 64 * over['patch_h_size'] ** 2 and b.pos_embedding.shape[-1] == over['dim']
        keep = backbone(net)
        if tag in E2E:
            keep.update(e2e(cfg, net, tag))
        save(f'g26_vitgeom_{tag}.npz', config=CONFIG2, backbone=json.dumps(over), input_seed=31, batch2_seeds=np.array(BATCH2_SEEDS),
             weight_seed=2021, **keep)
        layouts[tag] = {'config': CONFIG2, 'backbone': over, 'state_dict': [[k, list(v.shape)] for k, v in net.state_dict().items()]}
    with open(path, 'w') as f:
        json.dump(layouts, f)
        f.write('\n')
    print('wrote g26_vitgeom_layout.json', os.path.getsize(path))


if __name__ == '__main__':
    main()
