#!/usr/bin/env python3
"""Golden vectors of ColumnProposal2's proposal-attention branch (`column_att = True`), produced by the upstream reference on CPU
through the same harness as make_golden_propgeom.py.

    python tests/golden/make_golden_colatt.py [att_p72 att_p36 att_p18 att_t2]

Tags (TAGS): config 2 with `column_att = True` at the proposal geometries (72, 2), (36, 4), (18, 8), and at (72, 2) with a deeper,
narrower lane transformer (tr_depth 2, dim_token 512, 8 heads, mlp 1024).  Per tag one g27_colatt_<tag>.npz holding
  stage_*  the branch's intermediate values on cases.head_inputs(41, batch=2), taken with hooks on the reference's own submodules:
           feat_down [B,Cd,P,P] (generate_line_proposal), tok [B,P,dim_token] (tr_lane_correlator) and colfeat [B,8,144,P]
           (line_expand, permuted as the reference's forward does), all sampled;
  head_*   the head outputs of that run, floats sampled, cls2 / orient argmax with low-margin indices (the G25 pattern);
  e2e_*    one 1152^2 tile through the whole reference net, decisions whole with their margin lists and the assembled polylines.
g27_colatt_layout.json holds each tag's state-dict layout as the reference net builds it (the G25 pattern).
Weights: synth.fill_module_ with seed 2021 (non-zero BatchNorm shifts, so a BN folded into the zero-padded stride-2 convolutions
would show); inputs from the seeded generators, so the fixtures hold seeds and expected outputs only.
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
from make_golden_mixseg import sampled, _top2_margin, _low  # noqa: E402
from make_golden_propgeom import e2e  # noqa: E402

CONFIG2 = 'Proj_polyline_fpn_vit_vertex_2'
TAGS = {
    'att_p72': dict(),
    'att_p36': dict(num_prop=36, prop_width=4),
    'att_p18': dict(num_prop=18, prop_width=8),
    'att_t2': dict(tr_depth=2, dim_token=512, tr_heads=8, tr_mlp_dim=1024),
}
S = dict(n_samples=2048, n_chunks=512)
BATCH = 2


def stages_and_head(net):
    h = net.heads
    x, x_up = cases.head_inputs(41, batch=BATCH)
    cap = {'expand': []}
    hooks = [h.generate_line_proposal.register_forward_hook(lambda m, a, o: cap.__setitem__('feat_down', o.detach().clone())),
             h.tr_lane_correlator.register_forward_hook(lambda m, a, o: cap.setdefault('tok', []).append(o.detach().clone())),
             h.line_expand.register_forward_hook(lambda m, a, o: cap['expand'].append(o.detach().clone()))]
    try:
        with torch.no_grad():
            out = h(torch.from_numpy(x), torch.from_numpy(x_up), torch.zeros(BATCH, 1, 1152, 1152))
    finally:
        for k in hooks:
            k.remove()
    tok = torch.cat(cap['tok'], dim=0)                                          # per image [1, P, dim_token]
    colfeat = torch.cat([e[0, :, :, :, 0].permute(1, 2, 0)[None] for e in cap['expand']], dim=0)     # [B, 8, 144, P]
    keep = {}
    keep.update(sampled('stage_feat_down', cap['feat_down'], **S))
    keep.update(sampled('stage_tok', tok, **S))
    keep.update(sampled('stage_colfeat', colfeat, **S))
    keep['head_proposal_conf'] = out['proposal_conf'].numpy()
    for k in ('ext2', 'cls2', 'offset2', 'orient'):
        keep.update(sampled(f'head_{k}', out[k], **S))
    keep['head_cls2_argmax'] = out['cls2'].argmax(-1).numpy().astype(np.uint8)
    keep['head_cls2_lowmargin'] = _low(_top2_margin(out['cls2'], -1))
    keep['head_orient_argmax'] = out['orient'].argmax(1).numpy().astype(np.uint8)
    keep['head_orient_lowmargin'] = _low(_top2_margin(out['orient'], 1))
    return keep


def main():
    which = sys.argv[1:] or list(TAGS)
    make_golden._stable_sorts(True)
    path = os.path.join(HERE, 'g27_colatt_layout.json')
    layouts = json.load(open(path)) if os.path.exists(path) else {}
    for tag in which:
        over = TAGS[tag]
        print('==', tag, over)
        cfg0 = make_golden._refload.load_cfg(f'configs/{CONFIG2}.py')
        heads = dict(cfg0.heads)
        heads.update(over)
        cfg, net = ref_net(f'configs/{CONFIG2}.py', heads=heads, column_att=True)
        assert cfg.column_att and cfg.spatial_att and not cfg.column_transformer_decoder
        keep = {**stages_and_head(net), **e2e(cfg, net, tag)}
        save(f'g27_colatt_{tag}.npz', config=CONFIG2, heads=json.dumps(over), input_seed=41, batch=BATCH, weight_seed=2021, **keep)
        layouts[tag] = {'config': CONFIG2, 'heads': over, 'column_att': True,
                        'state_dict': [[k, list(v.shape)] for k, v in net.state_dict().items()]}
    with open(path, 'w') as f:
        json.dump(layouts, f)
        f.write('\n')
    print('wrote g27_colatt_layout.json', os.path.getsize(path))


if __name__ == '__main__':
    main()
