#!/usr/bin/env python3
"""Golden vectors of the MLP-Mixer lane config (configs/Proj_polyline_fpn_mixseg_vertex.py: MixSegNet backbone, ColumnProposal2
with spatial_att=False), produced by the upstream reference on CPU through the same harness as make_golden.py.

    python tests/golden/make_golden_mixseg.py [g21 g22 g23 g24]

Weights: synth.fill_module_ with seed 2021 (pretrained=False); inputs from the seeded generators of cases.py / synth.py, so the
fixtures hold seeds and expected outputs only.  Large float outputs are kept as samples plus chunk means (`sampled`), decisions
(argmax, thresholds, endpoints, polylines) whole with the flat indices of their low-margin entries.  Committed outputs: g21_mixseg_backbone.npz, g22_mixseg_head.npz, g23_mixseg_e2e.npz,
g24_mixseg_layout.json.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402
import make_golden  # noqa: E402  (puts the repo root on sys.path)
from make_golden import ref_net, save, _refload, cases, synth  # noqa: E402

CONFIG = 'Proj_polyline_fpn_mixseg_vertex'
BATCH2_SEEDS = (32, 33)
SAMPLES, CHUNKS = 4096, 1024      # per sampled float tensor: ~16 KB of samples + 8 KB of chunk means


def _top2_margin(t, dim):
    top2 = torch.topk(t, 2, dim=dim).values
    return (top2.select(dim, 0) - top2.select(dim, 1)).numpy()


def _low(margin):
    """flat indices of the decisions whose reference margin is inside fp32 noise (< 1e-4)"""
    return np.flatnonzero(np.asarray(margin).reshape(-1) < 1e-4).astype(np.int64)


def _is_prime(n):
    return n > 1 and all(n % d for d in range(2, int(n ** 0.5) + 1))


def sampled(name, t, n_samples=SAMPLES, n_chunks=CHUNKS):
    """A float tensor in a few tens of KB instead of whole: its shape and largest magnitude, every `stride`-th element of the flat
    tensor (stride a prime near size / n_samples, so the samples walk across every axis) and the fp64 means of n_chunks contiguous
    chunks of the flat tensor (np.array_split), which cover every element.  tests/test_gpu_mixseg.py::_close_sampled reads them."""
    a = t.detach().numpy() if torch.is_tensor(t) else np.asarray(t)
    stride = max(2, a.size // n_samples)
    while not _is_prime(stride):
        stride += 1
    flat = a.reshape(-1)
    return {f'{name}_shape': np.array(a.shape, dtype=np.int64), f'{name}_absmax': np.float64(np.abs(flat).max()),
            f'{name}_stride': np.int64(stride), f'{name}_samples': flat[::stride].astype(np.float32),
            f'{name}_chunk_mean': np.array([c.astype(np.float64).mean() for c in np.array_split(flat, n_chunks)])}


def g21(cfg, net):
    x = torch.from_numpy(cases.vit_input(31))
    x2 = torch.from_numpy(np.concatenate([cases.vit_input(s) for s in BATCH2_SEEDS]))
    with torch.no_grad():
        y, y2 = net.backbone(x), net.backbone(x2)
    save('g21_mixseg_backbone.npz', input_seed=31, batch2_seeds=np.array(BATCH2_SEEDS), weight_seed=2021,
         **sampled('out', y), **sampled('out_batch2', y2))


def g22(cfg, net):
    x, x_up = cases.head_inputs(41)
    with torch.no_grad():
        out = net.heads(torch.from_numpy(x), torch.from_numpy(x_up), torch.zeros(1, 1, 1152, 1152))
    assert not out['prop_bi_seg'].any(), 'spatial_att=False: prop_bi_seg is zeros'
    keep = {'proposal_conf': out['proposal_conf'].numpy()}
    for k in ('ext2', 'cls2', 'offset2', 'orient'):
        keep.update(sampled(k, out[k]))
    keep['cls2_argmax'] = out['cls2'].argmax(-1).numpy().astype(np.uint8)
    keep['cls2_lowmargin'] = _low(_top2_margin(out['cls2'], -1))
    keep['orient_argmax'] = out['orient'].argmax(1).numpy().astype(np.uint8)
    keep['orient_lowmargin'] = _low(_top2_margin(out['orient'], 1))
    save('g22_mixseg_head.npz', input_seed=41, weight_seed=2021, **keep)


def g23(cfg, net):
    """One 1152² synthetic tile through the whole reference net: the decisions of g10 (make_golden.py) whole, with their margin lists,
    the raw float outputs sampled."""
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
    raw, dec = cap['raw'], cap['dec']
    sm = cap['sem_logits'].softmax(1)[0]
    s1, s2 = sm[1], sm[2]
    sem_margin = torch.minimum((s1 - s2).abs(), (torch.maximum(s1, s2) - cfg.coor_thre).abs())
    e = raw['ext2'].softmax(3)[0]
    ext_margin = torch.minimum((e[..., 1] - e[..., 2]).abs(), (torch.maximum(e[..., 1], e[..., 2]) - cfg.exist_thre).abs())
    keep = {'proposal_conf': raw['proposal_conf'].numpy()}
    for k, name in (('ext2', 'ext2'), ('cls2', 'cls2'), ('offset2', 'offset2'), ('orient', 'orient_logits')):
        keep.update(sampled(name, raw[k]))
    save('g23_mixseg_e2e.npz', tile_seed=2021, weight_seed=2021, **keep,
         cls2_argmax=raw['cls2'].argmax(-1).numpy().astype(np.uint8), cls2_lowmargin=_low(_top2_margin(raw['cls2'], -1)),
         sem_lowmargin=_low(sem_margin), ext_lowmargin=_low(ext_margin), orient_lowmargin=_low(_top2_margin(raw['orient'], 1)[0]),
         prop_conf=dec['prop_conf'].numpy(), prop_v_ext=dec['prop_v_ext'].numpy().astype(np.uint8),
         cls_offset=dec['cls_offset'].numpy(), orient=dec['orient'].numpy().astype(np.uint8),
         semantic_seg=dec['semantic_seg'].numpy().astype(np.uint8),
         endp=np.stack(np.nonzero(dec['endp'][0].numpy()), axis=1),
         endp_final=np.stack(np.nonzero(o['lane_maps']['endp_by_cls'][0]), axis=1),
         cls_offset_smooth=o['lane_maps']['cls_offset_smooth'][0])


def g24(cfg, net):
    """State-dict layout (keys in order, shapes) and entry keys of the reference's UNMODIFIED config built through the product's
    boundary (keys in the product's order), checked here against the state dict of the reference net itself: the same keys and
    shapes, the backbone's keys in the same order."""
    from lanemapping_amd.boundary import load_config, build_net_from_config
    path = os.path.join(_refload.REF_ROOT, 'configs', CONFIG + '.py')
    sd = build_net_from_config(path, device='cpu').state_dict()
    layout = [[k, list(v.shape)] for k, v in sd.items()]
    ref_layout = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert sorted(layout) == sorted(ref_layout), 'product and reference state-dict layouts differ'
    bb = [e for e in layout if e[0].startswith('backbone.')]
    assert bb == [e for e in ref_layout if e[0].startswith('backbone.')], 'backbone state-dict order differs'
    rc = load_config(path)
    out = {CONFIG: {'state_dict': layout, 'dataset_test': dict(rc.dataset.test), 'train_type': rc.dataset.train.type,
                    'entry': {'log_dir': rc.log_dir, 'batch_size': rc.batch_size, 'seed': rc.seed, 'validate_buffer': rc.validate_buffer}}}
    path = os.path.join(HERE, 'g24_mixseg_layout.json')
    with open(path, 'w') as f:
        json.dump(out, f)
        f.write('\n')
    print(f'wrote g24_mixseg_layout.json ({len(sd)} state-dict entries)', os.path.getsize(path))


def main():
    which = sys.argv[1:] or ['g21', 'g22', 'g23', 'g24']
    make_golden._stable_sorts(True)
    cfg, net = ref_net(f'configs/{CONFIG}.py')
    assert cfg.spatial_att is False and cfg.backbone.type == 'MixSegNet'
    for w in which:
        print('==', w)
        globals()[w](cfg, net)


if __name__ == '__main__':
    main()
