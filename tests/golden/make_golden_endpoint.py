#!/usr/bin/env python3
"""Golden vectors of ColumnProposal2 with `heads.endp_mode = 'endpoint'` (the head's own endpoint map, decoded instead of the FPN's
`endp_est`), produced by the upstream reference on CPU through the same harness as make_golden_colatt.py.

    python tests/golden/make_golden_endpoint.py [ep_c2 ep_att ep_mixseg]

Tags (TAGS): config 2, config 2 with `column_att = True`, and the MixSeg config (spatial_att=False), each with
cfg.heads.endp_mode = 'endpoint'.  Per tag one g28_endpoint_<tag>.npz holding
  head_*   the reference head on cases.head_inputs(41, batch=2) and x_endp = synth.endp_logits(43, 2): the `endpoint` map sampled and
           its 2-pixel frame whole (rows and columns 0, 1, 1150, 1151: where the zero paddings of both convolutions act), the other
           head outputs as in G27;
  e2e_*    one 1152^2 tile through the whole reference net (make_golden_propgeom.e2e), plus the `endpoint` map sampled and the firm /
           any endpoint sets of G15: the reference's decode alone is re-run on the endpoint map perturbed by +-1e-4 in four noise
           patterns; `endp_firm` = the endpoints present in all nine runs, `endp_any` = the union.
The generator asserts that the decode gives at least MIN_ENDP endpoints and that at least half of them are firm, and that tied
logits among the top 520 cropped scores all sit on the map's one plateau (see e2e_endpoint; their count is stored).
g28_endpoint_layout.json holds each tag's state-dict layout as the reference net builds it.
Weights: synth.fill_module_ with seed 2021 (non-zero BatchNorm shifts, so a BN folded into the zero-padded second convolution would
show in the frame).  The .npz members carry a fixed timestamp, so the fixtures regenerate byte for byte.
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402
import make_golden  # noqa: E402  (puts the repo root on sys.path)
import make_golden_propgeom  # noqa: E402
from make_golden import ref_net, cases, synth  # noqa: E402
from make_golden_mixseg import sampled, _top2_margin, _low  # noqa: E402

CONFIG2 = 'Proj_polyline_fpn_vit_vertex_2'
MIXSEG = 'Proj_polyline_fpn_mixseg_vertex'
# tag -> (config, top-level config overrides)
TAGS = {
    'ep_c2': (CONFIG2, dict()),
    'ep_att': (CONFIG2, dict(column_att=True)),
    'ep_mixseg': (MIXSEG, dict()),
}
S = dict(n_samples=2048, n_chunks=512)
BATCH = 2
ENDP_SEED = 43
TILE_SEEDS = tuple(range(2021, 2031))      # the first seed at which every tag meets the generator's conditions is used for all tags
MIN_ENDP = 3
FRAME = (0, 1, 1150, 1151)


def save(name, **arrs):
    """np.savez_compressed with a fixed member timestamp (numpy stamps the members with the wall clock)."""
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrs.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print(f'wrote {name}: {os.path.getsize(path) / 1e6:.2f} MB')


def head(net):
    h = net.heads
    x, x_up = cases.head_inputs(41, batch=BATCH)
    x_endp = synth.endp_logits(ENDP_SEED, BATCH)
    with torch.no_grad():
        out = h(torch.from_numpy(x), torch.from_numpy(x_up), torch.from_numpy(x_endp))
    ep = out['endpoint']
    assert tuple(ep.shape) == (BATCH, 1, 1152, 1152)
    keep = dict(sampled('head_endpoint', ep, **S))
    keep['head_endpoint_frame_rows'] = ep[:, 0, list(FRAME), :].numpy()             # [B, 4, 1152]
    keep['head_endpoint_frame_cols'] = ep[:, 0, :, list(FRAME)].numpy()             # [B, 1152, 4]
    keep['head_proposal_conf'] = out['proposal_conf'].numpy()
    for k in ('ext2', 'cls2', 'offset2', 'orient'):
        keep.update(sampled(f'head_{k}', out[k], **S))
    keep['head_cls2_argmax'] = out['cls2'].argmax(-1).numpy().astype(np.uint8)
    keep['head_cls2_lowmargin'] = _low(_top2_margin(out['cls2'], -1))
    keep['head_orient_argmax'] = out['orient'].argmax(1).numpy().astype(np.uint8)
    keep['head_orient_lowmargin'] = _low(_top2_margin(out['orient'], 1))
    return keep


def _endp_set(d):
    return {tuple(int(v) for v in r) for r in np.stack(np.nonzero(d['endp'][0].numpy()), axis=1)}


def e2e_endpoint(cfg, net, tag, tile_seed):
    """make_golden_propgeom.e2e on tile `tile_seed` + the endpoint map and its firm / any endpoint sets; None if the tile does not meet
    the conditions."""
    h = net.heads
    true_decode = h.get_exist_coor_endp_dict
    cap = {}

    def keep_inputs(out):           # e2e's own capture drops 'endpoint': keep what the decode is handed, before it edits it in place
        cap['out'] = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in out.items()}
        return true_decode(out)
    h.get_exist_coor_endp_dict = keep_inputs
    bev_batch = synth.bev_batch
    make_golden_propgeom.synth.bev_batch = lambda seeds, size=1152: bev_batch([tile_seed], size)
    try:
        keep = make_golden_propgeom.e2e(cfg, net, tag)
    finally:
        make_golden_propgeom.synth.bev_batch = bev_batch
        h.get_exist_coor_endp_dict = true_decode
    keep['e2e_tile_seed'] = tile_seed
    full = cap['out']
    ep = full['endpoint']
    assert tuple(ep.shape) == (1, 1, 1152, 1152)
    # make_golden.py g5 asserts that the top-520 cropped scores are distinct.  This map cannot promise that: wherever every ReLU'd input
    # of a 5 x 5 neighbourhood is zero it holds ONE value (conv 2 of the constant bn(relu(b1)), plus b2), and with the seeded weights that
    # plateau reaches the top 520 on every tile seed for at least one tag.  Asserted instead: the tied logits among the top 520 all
    # hold that one value.  The ties resolve to the lower index here (stable sorts) and in lm_endp_topk; the count is stored, and the
    # firm / any sets below bound what a 1e-4 error may do to them.
    logits = torch.sort(ep[0, 0, 20:-20, 20:-20].reshape(-1), descending=True).values[:520]
    tied = logits[1:][logits[1:] == logits[:-1]]
    assert tied.numel() == 0 or bool((tied == tied[0]).all()), 'top-520 endpoint logits tie at more than one value'
    keep['e2e_endp_top520_tied'] = np.int64(tied.numel())
    keep['e2e_endp_plateau'] = np.float32(tied[0]) if tied.numel() else np.float32('nan')

    def decode(endpoint):
        out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in full.items()}
        out['endpoint'] = endpoint
        h.b_size = 1
        with torch.no_grad():
            return _endp_set(true_decode(out))
    base = decode(ep.clone())
    assert base == {tuple(int(v) for v in r) for r in keep['e2e_endp']}, 'the decode re-run differs from the end-to-end run'
    firm, anyset = set(base), set(base)
    for key in (1, 2, 3, 4):
        n = synth.uniform(synth.fnv1a64('g28margin%d' % key) ^ tile_seed, ep.numel())
        n4 = torch.from_numpy(((n > 0.5).astype(np.float32) * 2 - 1).reshape(tuple(ep.shape)))
        for sgn in (1.0, -1.0):
            d4 = decode(ep + sgn * 1e-4 * n4)
            firm &= d4
            anyset |= d4
    print(f'  {tag} tile {tile_seed}: {len(base)} endpoints, {len(firm)} firm, {len(anyset)} in any run')
    if len(base) < MIN_ENDP or 2 * len(firm) < len(base):
        return None
    as_arr = lambda st: np.array(sorted(st), dtype=np.int32).reshape(-1, 2)      # noqa: E731
    keep.update(sampled('e2e_endpoint', ep, **S))
    keep['e2e_endp_firm'] = as_arr(firm)
    keep['e2e_endp_any'] = as_arr(anyset)
    return keep


def build(tag):
    config, over = TAGS[tag]
    cfg0 = make_golden._refload.load_cfg(f'configs/{config}.py')
    heads = dict(cfg0.heads)
    heads['endp_mode'] = 'endpoint'
    cfg, net = ref_net(f'configs/{config}.py', heads=heads, **over)
    assert cfg.heads.endp_mode == 'endpoint' and net.heads.endp_mode == 'endpoint'
    return cfg, net


def main():
    which = sys.argv[1:] or list(TAGS)
    make_golden._stable_sorts(True)
    nets = {tag: build(tag) for tag in TAGS}          # the tile seed is chosen over ALL tags, whichever are written
    e2e = None
    for seed in TILE_SEEDS:
        e2e = {}
        for tag, (cfg, net) in nets.items():
            e2e[tag] = e2e_endpoint(cfg, net, tag, seed)
            if e2e[tag] is None:
                break
        if all(e2e.get(tag) is not None for tag in TAGS):
            break
        e2e = None
    assert e2e is not None, f'no tile seed of {TILE_SEEDS} meets the conditions for every tag'
    path = os.path.join(HERE, 'g28_endpoint_layout.json')
    layouts = json.load(open(path)) if os.path.exists(path) else {}
    for tag in which:
        config, over = TAGS[tag]
        print('==', tag, config, over)
        cfg, net = nets[tag]
        keep = {**head(net), **e2e[tag]}
        save(f'g28_endpoint_{tag}.npz', config=config, overrides=json.dumps(over), endp_mode='endpoint', input_seed=41,
             endp_seed=ENDP_SEED, batch=BATCH, weight_seed=2021, **keep)
        layouts[tag] = {'config': config, 'overrides': over, 'endp_mode': 'endpoint',
                        'state_dict': [[k, list(v.shape)] for k, v in net.state_dict().items()]}
    with open(path, 'w') as f:
        json.dump({k: layouts[k] for k in sorted(layouts)}, f)
        f.write('\n')
    print('wrote g28_endpoint_layout.json', os.path.getsize(path))


if __name__ == '__main__':
    main()
