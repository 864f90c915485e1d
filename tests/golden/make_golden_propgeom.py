#!/usr/bin/env python3
"""Golden vectors of ColumnProposal2 at the other proposal geometries the reference's config schema offers
(`num_prop = 72, 36, 18` / `prop_width = 2, 4, 8` / `dim_shared = 100, used to be 512`), produced by the upstream reference on CPU
through the same harness as make_golden.py / make_golden_mixseg.py.

    python tests/golden/make_golden_propgeom.py [c2_p36 c2_p18 c2_d512 mixseg_p36]

Geometries (GEOMETRIES): config 2 with cfg.heads overridden to (36, 4), (18, 8) and (72, 2, dim_shared=512), and the MixSeg config at
(36, 4); prop_half_buff stays 4.  Per geometry one g25_propgeom_<tag>.npz holding
  head_*  the head on cases.head_inputs(41) (the G4 / G22 pattern), floats sampled, cls2 / orient argmax with low-margin indices;
  dec_*   the decode dict of get_exist_coor_endp_dict on decode_inputs(51, batch=2) cut to the geometry (the G5 pattern);
  e2e_*   one 1152^2 tile through the whole reference net, decisions whole with their margin lists (the G10 / G23 pattern).
g25_propgeom_layout.json holds each geometry's state-dict layout as the reference net builds it (the G20 / G24 pattern).
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
from make_golden import ref_net, save, _decode_ref, cases, synth  # noqa: E402
from make_golden_mixseg import sampled, _top2_margin, _low  # noqa: E402

CONFIG2 = 'Proj_polyline_fpn_vit_vertex_2'
MIXSEG = 'Proj_polyline_fpn_mixseg_vertex'
# tag -> (config, heads overrides)
GEOMETRIES = {
    'c2_p36': (CONFIG2, dict(num_prop=36, prop_width=4)),
    'c2_p18': (CONFIG2, dict(num_prop=18, prop_width=8)),
    'c2_d512': (CONFIG2, dict(dim_shared=512)),
    'mixseg_p36': (MIXSEG, dict(num_prop=36, prop_width=4)),
}
S = dict(n_samples=2048, n_chunks=512)


def decode_inputs(P, FW, seed=51, batch=2):
    """cases.decode_inputs cut to P proposals of width FW: the leading elements of its i.i.d. flat tensors, reshaped (the GPU test
    derives the same arrays the same way)."""
    raw = cases.decode_inputs(seed, batch=batch)
    R = raw['ext2'].shape[2]
    raw['proposal_conf'] = np.ascontiguousarray(raw['proposal_conf'][:, :P])
    raw['ext2'] = np.ascontiguousarray(raw['ext2'][:, :P])
    for k in ('cls2', 'offset2'):
        raw[k] = raw[k].reshape(-1)[:batch * P * R * FW].reshape(batch, P, R, FW).copy()
    return raw


def head(net, tag):
    x, x_up = cases.head_inputs(41)
    with torch.no_grad():
        out = net.heads(torch.from_numpy(x), torch.from_numpy(x_up), torch.zeros(1, 1, 1152, 1152))
    keep = {'head_proposal_conf': out['proposal_conf'].numpy()}
    for k in ('ext2', 'cls2', 'offset2', 'orient'):
        keep.update(sampled(f'head_{k}', out[k], **S))
    keep['head_cls2_argmax'] = out['cls2'].argmax(-1).numpy().astype(np.uint8)
    keep['head_cls2_lowmargin'] = _low(_top2_margin(out['cls2'], -1))
    keep['head_orient_argmax'] = out['orient'].argmax(1).numpy().astype(np.uint8)
    keep['head_orient_lowmargin'] = _low(_top2_margin(out['orient'], 1))
    return keep


def dec(cfg, net, tag):
    h = net.heads
    raw = decode_inputs(h.num_prop, h.prop_fea_width)
    d = _decode_ref(cfg, net, raw)
    assert d['prop_cls_conf'].shape[-1] == h.prop_fea_width
    c = raw['cls2']
    top2 = np.sort(c, axis=-1)[..., -2:]
    return {'dec_prop_conf': d['prop_conf'].numpy(), 'dec_prop_v_ext': d['prop_v_ext'].numpy().astype(np.uint8),
            'dec_cls_offset': d['cls_offset'].numpy(), 'dec_cls_argmax': c.argmax(-1).astype(np.uint8),
            'dec_cls_lowmargin': _low(top2[..., 1] - top2[..., 0]),
            **sampled('dec_prop_cls_conf', d['prop_cls_conf'], **S)}


def e2e(cfg, net, tag):
    """As make_golden_mixseg.g23, for this geometry."""
    x = torch.from_numpy(synth.bev_batch([2021], 1152))
    cap = {}

    def hook(mod, args, out):
        cap['raw'] = {k: v.detach().clone() for k, v in out.items() if k not in ('prop_bi_seg', 'endpoint')}
    hd = net.heads.register_forward_hook(hook)
    orig = net.heads.get_exist_coor_endp_dict

    def spy(out):
        cap['sem_logits'] = out['semantic_seg'].detach().clone()
        d = orig(out)
        cap['dec'] = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in d.items()}
        return d
    net.heads.get_exist_coor_endp_dict = spy
    try:
        with torch.no_grad():
            o = net({'proj': x})
    finally:
        hd.remove()
        net.heads.get_exist_coor_endp_dict = orig
    raw, d = cap['raw'], cap['dec']
    sm = cap['sem_logits'].softmax(1)[0]
    s1, s2 = sm[1], sm[2]
    sem_margin = torch.minimum((s1 - s2).abs(), (torch.maximum(s1, s2) - cfg.coor_thre).abs())
    e = raw['ext2'].softmax(3)[0]
    ext_margin = torch.minimum((e[..., 1] - e[..., 2]).abs(), (torch.maximum(e[..., 1], e[..., 2]) - cfg.exist_thre).abs())
    keep = {'e2e_proposal_conf': raw['proposal_conf'].numpy()}
    for k, name in (('ext2', 'ext2'), ('cls2', 'cls2'), ('offset2', 'offset2'), ('orient', 'orient_logits')):
        keep.update(sampled(f'e2e_{name}', raw[k], **S))
    V = o['lane_maps']['cls_offset_smooth'][0]
    print(f'  {tag}: {int((np.count_nonzero(V[:, :, 0] > 0, axis=1) >= 2).sum())} polylines')
    keep.update(
        e2e_tile_seed=2021, e2e_cls2_argmax=raw['cls2'].argmax(-1).numpy().astype(np.uint8),
        e2e_cls2_lowmargin=_low(_top2_margin(raw['cls2'], -1)), e2e_sem_lowmargin=_low(sem_margin), e2e_ext_lowmargin=_low(ext_margin),
        e2e_orient_lowmargin=_low(_top2_margin(raw['orient'], 1)[0]),
        e2e_prop_conf=d['prop_conf'].numpy(), e2e_prop_v_ext=d['prop_v_ext'].numpy().astype(np.uint8),
        e2e_cls_offset=d['cls_offset'].numpy(), e2e_orient=d['orient'].numpy().astype(np.uint8),
        e2e_semantic_seg=d['semantic_seg'].numpy().astype(np.uint8),
        e2e_endp=np.stack(np.nonzero(d['endp'][0].numpy()), axis=1),
        e2e_endp_final=np.stack(np.nonzero(o['lane_maps']['endp_by_cls'][0]), axis=1), e2e_cls_offset_smooth=V)
    return keep


def main():
    which = sys.argv[1:] or list(GEOMETRIES)
    make_golden._stable_sorts(True)
    path = os.path.join(HERE, 'g25_propgeom_layout.json')
    layouts = json.load(open(path)) if os.path.exists(path) else {}
    for tag in which:
        config, over = GEOMETRIES[tag]
        print('==', tag, config, over)
        cfg0 = make_golden._refload.load_cfg(f'configs/{config}.py')
        heads = dict(cfg0.heads)
        heads.update(over)
        cfg, net = ref_net(f'configs/{config}.py', heads=heads)
        h = net.heads
        assert (h.num_prop, h.prop_width, h.prop_half_buff, h.cls2[0].out_channels) == (
            heads['num_prop'], heads['prop_width'], heads['prop_half_buff'], heads['dim_shared'])
        keep = {**head(net, tag), **dec(cfg, net, tag), **e2e(cfg, net, tag)}
        save(f'g25_propgeom_{tag}.npz', config=config, heads=json.dumps(over), input_seed=41, decode_seed=51, weight_seed=2021, **keep)
        layouts[tag] = {'config': config, 'heads': over, 'state_dict': [[k, list(v.shape)] for k, v in net.state_dict().items()]}
    with open(path, 'w') as f:
        json.dump(layouts, f)
        f.write('\n')
    print('wrote g25_propgeom_layout.json', os.path.getsize(path))


if __name__ == '__main__':
    main()
