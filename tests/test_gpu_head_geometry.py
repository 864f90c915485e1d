"""GPU tests (-m gpu) of ColumnProposal2 at the proposal geometries (num_prop, prop_width) = (36, 4) / (18, 8), i.e. window width
FW = prop_width + 2 * prop_half_buff = 12 / 16, and dim_shared 512: the widened device entries (lm_head_tokens / _window, lm_decode_proposals,
the stage-2 small-conv route) against fp64 and under guarded buffers, then the head, the decode and the whole net against the reference's
goldens G25 (tests/golden/make_golden_propgeom.py), batch invariance, graph replay and the Runner entry."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from gpu_common import (_ab_npz, _cached_net, _chk, _close, _close_sampled, _flips_inside_noise, _g, _lib, _nhwc_dev, _nhwc_rows,
                        _quarter_grid, _same_polylines)
from guards import NAN, Slab, batched, guarded_runs
from lanemapping_amd import ops, synth
from test_head_geometry_cpu import build_geometry

pytestmark = pytest.mark.gpu

TAGS = ('c2_p36', 'c2_p18', 'c2_d512', 'mixseg_p36')
GEOM = {12: (36, 4), 16: (18, 8)}        # FW -> (num_prop, prop_width); prop_half_buff = 4


# ----------------------------------------------------------------------------------------------- fp64 restatements
def _tokens_ref(row, seg, P, pw, hb, seg_bias):
    """:382-405 in fp64 for one image: row [16,Hr,Wr], seg [Hs,Ws] (bi_seg_proposal of relu(col_fea_up); the zero-padded columns of
    col_fea_up evaluate to the conv bias) or None (spatial_att=False) -> tok [P*Hr, 16*FW], tok[(p,h), c*FW+w]."""
    Cc, Hr, Wr = row.shape
    fw = pw + 2 * hb
    # right padding wide enough for every window (P * pw may exceed Wr in the small cases: those columns are zeros / the bias too)
    rowp = F.pad(row.double(), (hb, hb + pw * P, 0, 0))
    segp = None if seg is None else F.pad(seg.double(), (2 * hb, 2 * hb + 2 * pw * P, 0, 0), value=seg_bias)
    toks = []
    for p in range(P):
        win = rowp[:, :, pw * p: pw * p + fw]                                           # [16, Hr, FW]
        if segp is not None:
            sw = segp[None, None, :, 2 * pw * p: 2 * pw * p + 2 * fw]
            up = F.interpolate(sw, size=(8 * Hr, 8 * fw), mode='bilinear', align_corners=True)
            win = win * F.avg_pool2d(up, 8)[0]
        toks.append(win.permute(1, 0, 2).reshape(Hr, Cc * fw))
    return torch.cat(toks)


def _decode_ref(pconf, ext2, cls2, off2, thre, pw, hb):
    """:610, :694-702, :726-738 in fp64 (decisions on the logits: softmax is monotone, the inputs keep clear of fp32 ties)."""
    B, P, R, fw = cls2.shape
    e = ext2.double().softmax(3)
    v = torch.zeros(B, P, R)
    v[(e[..., 1] > e[..., 2]) & (e[..., 1] > thre)] = 1
    v[(e[..., 2] > e[..., 1]) & (e[..., 2] > thre)] = 2
    idx = torch.from_numpy(cls2.numpy().argmax(-1))                                      # first maximum: lowest index wins
    off = torch.gather(off2, 3, idx.unsqueeze(-1)).squeeze(-1)
    co = (idx.to(torch.float32) + off).to(torch.float64)
    co = torch.where(co > fw, torch.full_like(co, float(fw)), co)
    co = co + (pw * torch.arange(P, dtype=torch.float64) - hb).view(1, P, 1)
    return {'prop_conf': pconf.double().softmax(2), 'v_ext': v, 'cls_conf': cls2.double().softmax(3), 'cls_idx': idx.to(torch.int32),
            'cls_offset': co}


# ----------------------------------------------------------------------------------------------- head tokens
@pytest.mark.parametrize('spatial', [True, False])
@pytest.mark.parametrize('fw', [12, 16])
def test_head_tokens_vs_fp64(dev, fw, spatial):
    """lm_head_tokens / lm_head_tokens_window at FW 12 and 16 on the real map size (Hr = Wr = 144, every proposal, the first and last
    windows leaving the map), batch 2, against fp64."""
    P, pw = GEOM[fw]
    g = _g(fw * 2 + spatial)
    B, Hr = 2, 144
    row = torch.randn(B, 16, Hr, Hr, generator=g)
    seg = torch.randn(B, 1, 2 * Hr, 2 * Hr, generator=g)
    tok = ops.head_tokens(seg.to(dev) if spatial else None, _nhwc_dev(row, dev), P, pw, 4, -0.37)
    assert tuple(tok.shape) == (B * P * Hr, 16 * fw)
    for b in range(B):
        ref = _tokens_ref(row[b], seg[b, 0] if spatial else None, P, pw, 4, -0.37)
        _close(tok[b * P * Hr:(b + 1) * P * Hr], ref, 1e-5, f'tokens FW={fw} b={b}')


_TOKENS_AB = r"""
import sys, numpy as np, torch
from lanemapping_amd import ops
dev = torch.device('cuda:0')
g = torch.Generator().manual_seed(83)
out = {}
for fw, pw in ((12, 4), (16, 8)):
    for k, (B, Hr, P) in enumerate([(2, 144, 144 // pw), (1, 40, 10), (3, 25, 6)]):   # (Hr = 25: a ragged last block of token rows)
        seg = torch.randn(B, 1, 2 * Hr, 2 * Hr, generator=g).to(dev)
        row = torch.randn(B, Hr, Hr, 16, generator=g).to(dev).permute(0, 3, 1, 2)
        out[f'tok{fw}_{k}'] = ops.head_tokens(seg, row, P, pw, 4, -0.37).cpu().numpy()
np.savez(sys.argv[1], **out)
"""


def test_head_tokens_lds_bit_identical_to_gather_fw12_fw16(dev, tmp_path):
    """head_tokens_lds_kernel<12 / 16> (its own tiling: 21 / 16 token rows per workgroup) against the one-thread-per-token gather kernel
    (LM_HEAD_TOKENS_GATHER=1, read once per process, so each runs in a fresh child process): bit for bit."""
    res = _ab_npz(_TOKENS_AB, (('lds', {}), ('gather', {'LM_HEAD_TOKENS_GATHER': '1'})), tmp_path, timeout=600)
    assert len(res['lds'].files) == 6
    for k in res['lds'].files:
        a, b = res['lds'][k], res['gather'][k]
        assert np.isfinite(a).all() and a.shape == b.shape
        assert np.array_equal(a, b), (k, float(np.abs(a - b).max()))


def test_head_tokens_refuses_other_widths(dev):
    row = torch.zeros(1, 16, 8, 8, device=dev)
    with pytest.raises(RuntimeError, match='10, 12 or 16'):
        ops.head_tokens(None, row, 4, 2, 2, 0.)
    with pytest.raises(RuntimeError, match='10, 12 or 16'):
        ops.head_tokens(torch.zeros(1, 1, 16, 16, device=dev), row, 4, 4, 5, 0.)


# ----------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize('fw', [12, 16])
def test_decode_proposals_ties_saturation_clamp(dev, fw):
    """lm_decode_proposals at FW 12 / 16 against fp64: cls_idx, v_ext and cls_offset bit-exact for every proposal index, probabilities at
    1e-6.  FW-way and 2-way ties of the column bin (lowest index wins), saturated logits (+-100: every other probability underflows),
    3-way existence ties, and idx + off exactly on (FW), above (FW + 0.5 -> FW) and below (FW - 0.25) the clamp."""
    P, pw = GEOM[fw]
    g = _g(700 + fw)
    B, R = 2, 8
    pconf = _quarter_grid(torch.randn(B, P, 2, generator=g) * 2)
    pconf[0, :4] = 0.75
    pconf[1, :3, 0], pconf[1, :3, 1] = 100.0, -100.0                     # saturated
    ext2 = _quarter_grid(torch.randn(B, P, R, 3, generator=g) * 2)
    ext2[:, :, 0] = 1.25                                                 # 3-way tie: v = 0
    ext2[1, :, 1, 1:] = 2.0                                              # e1 == e2 > e0: v = 0
    cls2 = _quarter_grid(torch.randn(B, P, R, fw, generator=g) * 2).clamp(-8, 8)
    cls2[:, :, 1] = -0.5                                                 # FW-way tie -> 0
    cls2[:, 0::2, 2, 4] = 9.0
    cls2[:, 0::2, 2, fw - 3] = 9.0                                       # 2-way tie -> 4
    cls2[:, :, 3:6, fw - 1] = 20.0                                       # the last bin wins: idx + off around the clamp
    cls2[:, :, 6] = -100.0
    cls2[:, :, 6, fw - 2] = 100.0                                        # saturated: one probability 1, the others 0
    cls2[:, 1::2, 7, fw - 1] = 100.0
    cls2[:, 1::2, 7, fw - 2] = 100.0                                     # saturated tie -> fw - 2
    off2 = _quarter_grid(torch.rand(B, P, R, fw, generator=g) * 3 - 1)
    off2[:, :, 3, fw - 1] = 1.0                                          # (FW - 1) + 1 = FW exactly: kept
    off2[:, :, 4, fw - 1] = 1.5                                          # FW + 0.5 -> FW
    off2[:, :, 5, fw - 1] = 0.75                                         # FW - 0.25
    off2[:, :, 6, fw - 2] = 3.0                                          # (FW - 2) + 3 -> FW
    ref = _decode_ref(pconf, ext2, cls2, off2, 0.2, pw, 4)
    dd = [t.to(dev) for t in (pconf, ext2, cls2, off2)]
    prop_conf, v_ext, cls_conf, cls_idx, cls_offset = ops.decode_proposals(*dd, 0.2, pw, 4)
    assert tuple(cls_conf.shape) == (B, P, R, fw)
    assert torch.equal(cls_idx.cpu(), ref['cls_idx'])
    assert bool((cls_idx[:, :, 1] == 0).all()) and bool((cls_idx[:, 0::2, 2] == 4).all())
    assert bool((cls_idx[:, 1::2, 7] == fw - 2).all())
    assert torch.equal(cls_offset.cpu(), ref['cls_offset'])
    co = cls_offset.cpu() - (pw * torch.arange(P, dtype=torch.float64) - 4).view(1, P, 1)
    assert bool((co[:, :, 3] == fw).all()) and bool((co[:, :, 4] == fw).all()) and bool((co[:, :, 5] == fw - 0.25).all())
    assert bool((co[:, :, 6] == fw).all())
    assert torch.equal(v_ext.cpu(), ref['v_ext'])
    assert bool((v_ext[:, :, 0] == 0).all()) and bool((v_ext[1, :, 1] == 0).all())
    _close(prop_conf, ref['prop_conf'], 1e-6, 'prop_conf')
    _close(cls_conf, ref['cls_conf'], 1e-6, 'cls_conf')
    again = ops.decode_proposals(*dd, 0.2, pw, 4)
    for a, b in zip((prop_conf, v_ext, cls_conf, cls_idx, cls_offset), again):
        assert torch.equal(a, b)


def test_decode_proposals_refuses_other_widths(dev):
    z = [torch.zeros(s, device=dev) for s in ((1, 4, 2), (1, 4, 3, 3), (1, 4, 3, 8), (1, 4, 3, 8))]
    with pytest.raises(RuntimeError, match='10, 12 or 16'):
        _chk(_lib().lm_decode_proposals(ops._stream(), *[ops._ptr(t) for t in z], ops._ptr(torch.zeros(1, 4, 2, device=dev)),
                                        ops._ptr(torch.zeros(1, 4, 3, device=dev)), ops._ptr(torch.zeros(1, 4, 3, 8, device=dev)),
                                        ops._ptr(torch.zeros(1, 4, 3, device=dev, dtype=torch.int32)),
                                        ops._ptr(torch.zeros(1, 4, 3, device=dev, dtype=torch.float64)), 1, 4, 3, C.c_float(0.2), 2, 3))


# ----------------------------------------------------------------------------------------------- stage 2
def _stage2_case(D, fw, M, ldh, seed):
    g = _g(seed)
    hid = torch.randn(M, ldh, generator=g)
    w2 = torch.randn(3 + 2 * fw, D, generator=g) / D ** 0.5
    b2 = torch.randn(3 + 2 * fw, generator=g)
    h, w, b = hid.double(), w2.double(), b2.double()
    refs = [h[:, 0:D] @ w[0:3].t() + b[0:3], h[:, D:2 * D] @ w[3:3 + fw].t() + b[3:3 + fw],
            h[:, 2 * D:3 * D] @ w[3 + fw:].t() + b[3 + fw:]]
    return hid, w2, b2, refs


def _w_small(w2, fw, dev):
    D = w2.shape[1]
    return [ops.pack_small(w2[a:b].reshape(b - a, D, 1, 1).to(dev)) for a, b in ((0, 3), (3, 3 + fw), (3 + fw, 3 + 2 * fw))]


@pytest.mark.parametrize('D', [100, 512])
@pytest.mark.parametrize('fw', [10, 12, 16])
def test_head_stage2_route_vs_fp64(dev, fw, D):
    """The stage-2 route the head takes: FW = 10 through lm_head_stage2 (D = 512 is past its LDS kernel's limit: the direct kernel),
    FW = 12 / 16 through three 1x1 lm_conv2d_nhwc_small over the branch slices of the hidden rows (row pitch = the head's, 3 D rounded
    up to 64).  M = 2 * P * 144 rows, against fp64."""
    P = {10: 72, 12: 36, 16: 18}[fw]
    M, ldh = 2 * P * 144, -(-3 * D // 64) * 64
    hid, w2, b2, refs = _stage2_case(D, fw, M, ldh, seed=fw * 1000 + D)
    ws = None if fw == 10 else _w_small(w2, fw, dev)
    outs = ops.head_stage2(hid.to(dev), D, w2.to(dev), b2.to(dev), 2, P, 144, w_small=ws)
    for name, o, r, n in zip(('ext2', 'cls2', 'off2'), outs, refs, (3, fw, fw)):
        assert tuple(o.shape) == (2, P, 144, n)
        _close(o.reshape(M, n), r, 1e-5, f'{name} FW={fw} D={D}')


# ----------------------------------------------------------------------------------------------- guarded buffers
@pytest.mark.parametrize('spatial', [False, True])
@pytest.mark.parametrize('fw', [12, 16])
def test_head_tokens_bounds_fw(dev, fw, spatial):
    """As test_gpu_1_bounds.test_head_tokens_bounds, at FW 12 / 16: Hr = Wr = 25 (a ragged block of token rows), P = 6, windows that
    leave the map on both sides.  Window tokens against fp64, seg-weighted ones bit-exact to the unguarded call (pinned to fp64 by
    test_head_tokens_vs_fp64).  Guards: 2 image rows + 256 pixels on row / seg, 64 token rows on tok."""
    P, pw = 6, GEOM[fw][1]
    Hr = Wr = 25
    g = _g(250 + fw + spatial)
    row = torch.randn(1, 16, Hr, Wr, generator=g)
    seg = torch.randn(1, 2 * Hr, 2 * Wr, generator=g)
    if spatial:
        ref = ops.head_tokens(seg.view(1, 1, 2 * Hr, 2 * Wr).to(dev), _nhwc_dev(row, dev), P, pw, 4, -0.37).cpu()
    else:
        ref = _tokens_ref(row[0], None, P, pw, 4, 0.)
    rows_el = P * Hr

    def run(B, poisoned):
        pad = NAN if poisoned else 0.0
        rs = Slab(dev, B * Hr * Wr, 16, None, 0, 2 * Wr + 256, 2 * Wr + 256).fill_input(batched(_nhwc_rows(row[:1]), B, NAN), pad)
        ts = Slab(dev, B * rows_el, 16 * fw, None, 0, 64, 64).fill_canary()
        if spatial:
            ss = Slab(dev, B * 2 * Hr, 2 * Wr, None, 0, 8, 8).fill_input(batched(seg[0], B, NAN), pad)
            _chk(_lib().lm_head_tokens(ops._stream(), ss.ptr(), rs.ptr(), ts.ptr(), C.c_float(-0.37), B, P, Hr, Wr, pw, 4))
        else:
            _chk(_lib().lm_head_tokens_window(ops._stream(), rs.ptr(), ts.ptr(), B, P, Hr, Wr, pw, 4))
        return {'tok': (ts, rows_el)}
    tok = guarded_runs(run, f'head_tokens FW={fw} spatial={spatial}')['tok']
    if spatial:
        assert torch.equal(tok, ref)
    else:
        _close(tok, ref, 1e-5, 'head_tokens_window')


@pytest.mark.parametrize('D', [100, 512])
@pytest.mark.parametrize('fw', [12, 16])
def test_head_stage2_small_conv_bounds(dev, fw, D):
    """The FW = 12 / 16 stage-2 route under guards: each branch reads its D-column slice of hidden rows with pitch ldh = 3 D + 8 (so the
    columns beside every slice are poison) and writes [M][Cout].  M = 185 rows per element (not a multiple of the 256-row block).
    Guards: 256 rows on hid and on the outputs."""
    M, ldh = 185, 3 * D + 8
    hid, w2, b2, refs = _stage2_case(D, fw, M, 3 * D, seed=31 * fw + D)
    ws, bd = _w_small(w2, fw, dev), b2.to(dev)
    bounds = (0, 3, 3 + fw, 3 + 2 * fw)

    def run(B, poisoned):
        hs = Slab(dev, B * M, 3 * D, ldh, 4, 256, 256).fill_input(batched(hid, B, NAN), NAN if poisoned else 0.0)
        outs = [Slab(dev, B * M, n, None, 0, 256, 256).fill_canary() for n in (3, fw, fw)]
        for br, (o, w16) in enumerate(zip(outs, ws)):
            n = bounds[br + 1] - bounds[br]
            _chk(_lib().lm_conv2d_nhwc_small(ops._stream(), C.c_void_p(hs.ptr() + 4 * br * D), ldh, w16.data_ptr(), None,
                                             C.c_void_p(bd[bounds[br]:].data_ptr()), o.ptr(), n, 1, 1, B * M, D, n, 1, 1, 1, 0, 0, 0, 0))
        return {k: (o, M) for k, o in zip(('ext2', 'cls2', 'off2'), outs)}
    out = guarded_runs(run, f'head_stage2 small FW={fw} D={D}')
    for k, r in zip(('ext2', 'cls2', 'off2'), refs):
        _close(out[k], r, 1e-5, k)


@pytest.mark.parametrize('fw', [12, 16])
def test_head_proposal_conf_bounds_fw(dev, fw):
    """lm_head_proposal_conf with L = 16 * FW * Hr (Hr = 25), P = 6.  Guards: 2 token rows of L on tok, 2 rows on conf."""
    P, L = 6, 16 * fw * 25
    g = _g(90 + fw)
    tok = torch.randn(P, L, generator=g)
    wt = torch.randn(2, L, generator=g) / 50
    bias = torch.randn(2, generator=g)
    ref = tok.double() @ wt.double().t() + bias.double()
    wd, bd = wt.to(dev), bias.to(dev)

    def run(B, poisoned):
        ts = Slab(dev, B * P, L, None, 0, 2, 2).fill_input(batched(tok, B, NAN), NAN if poisoned else 0.0)
        cs = Slab(dev, B * P, 2, None, 0, 2, 2).fill_canary()
        _chk(_lib().lm_head_proposal_conf(ops._stream(), ts.ptr(), wd.data_ptr(), bd.data_ptr(), cs.ptr(), B * P, L))
        return {'conf': (cs, P)}
    _close(guarded_runs(run, f'proposal_conf FW={fw}')['conf'], ref, 1e-5, 'proposal_conf')


# ----------------------------------------------------------------------------------------------- goldens
def _net(dev, tag):
    """The geometry's net with the synthetic weights of seed 2021 on the GPU (tests do not mutate it)."""
    def build():
        from test_head_geometry_cpu import _layouts
        ref = _layouts()[tag]
        return build_geometry(ref['config'], ref['heads'])
    return _cached_net(dev, (__name__, tag), build)


@pytest.mark.parametrize('tag', TAGS)
def test_head_golden(dev, golden, tag):
    g = golden(f'g25_propgeom_{tag}.npz')
    net = _net(dev, tag)
    x, x_up = cases.head_inputs(int(g['input_seed']))
    with torch.no_grad():
        out = net.heads(torch.from_numpy(x).to(dev), torch.from_numpy(x_up).to(dev), None)
    _close(out['proposal_conf'], g['head_proposal_conf'], 1e-4, 'proposal_conf')
    for k in ('ext2', 'cls2', 'offset2', 'orient'):
        _close_sampled(out[k], g, f'head_{k}')
    for k, dim in (('cls2', -1), ('orient', 1)):
        _flips_inside_noise(out[k].argmax(dim).cpu().numpy(), g[f'head_{k}_argmax'], g[f'head_{k}_lowmargin'], k, 10 ** 9)


def _decode_inputs(P, FW, seed, batch=2):
    """make_golden_propgeom.decode_inputs: cases.decode_inputs cut to P proposals of width FW."""
    raw = cases.decode_inputs(seed, batch=batch)
    R = raw['ext2'].shape[2]
    raw['proposal_conf'] = np.ascontiguousarray(raw['proposal_conf'][:, :P])
    raw['ext2'] = np.ascontiguousarray(raw['ext2'][:, :P])
    for k in ('cls2', 'offset2'):
        raw[k] = raw[k].reshape(-1)[:batch * P * R * FW].reshape(batch, P, R, FW).copy()
    return raw


@pytest.mark.parametrize('tag', TAGS)
def test_decode_golden(dev, golden, tag):
    """get_exist_coor_endp_dict's proposal half (device decode) vs the reference's on the G5-pattern inputs of this geometry."""
    g = golden(f'g25_propgeom_{tag}.npz')
    h = _net(dev, tag).heads
    raw = _decode_inputs(h.num_prop, h.prop_fea_width, int(g['decode_seed']))
    d = {k: torch.from_numpy(raw[k]).to(dev) for k in ('proposal_conf', 'ext2', 'cls2', 'offset2')}
    prop_conf, v_ext, cls_conf, cls_idx, cls_offset = ops.decode_proposals(d['proposal_conf'], d['ext2'], d['cls2'], d['offset2'],
                                                                           h.cfg.exist_thre, h.prop_width, h.prop_half_buff)
    _close(prop_conf, g['dec_prop_conf'], 1e-6, 'prop_conf')
    _close_sampled(cls_conf, g, 'dec_prop_cls_conf', tol=1e-6)
    assert np.array_equal(v_ext.cpu().numpy().astype(np.uint8), g['dec_prop_v_ext'])
    _flips_inside_noise(cls_idx.cpu().numpy(), g['dec_cls_argmax'], g['dec_cls_lowmargin'], 'cls_idx', 0)
    np.testing.assert_array_equal(cls_offset.cpu().numpy(), g['dec_cls_offset'])


@pytest.mark.parametrize('tag', TAGS)
def test_end_to_end_golden(dev, golden, tag):
    """One full 1152^2 tile through Detector1stage at this geometry vs the reference's own end-to-end run (G10 / G23 tolerances)."""
    g = golden(f'g25_propgeom_{tag}.npz')
    net = _net(dev, tag)
    x = torch.from_numpy(synth.bev_batch([int(g['e2e_tile_seed'])], 1152)).to(dev)
    with torch.no_grad():
        raw = net.forward_raw({'proj': x})
        _close(raw['proposal_conf'], g['e2e_proposal_conf'], 1e-4, 'proposal_conf')
        for k, gk in (('ext2', 'ext2'), ('cls2', 'cls2'), ('offset2', 'offset2'), ('orient', 'orient_logits')):
            _close_sampled(raw[k], g, f'e2e_{gk}')
        o = net({'proj': x})
    _flips_inside_noise(o['prop_v_ext'].numpy().astype(np.uint8)[0], g['e2e_prop_v_ext'][0], g['e2e_ext_lowmargin'], 'prop_v_ext', 0)
    _flips_inside_noise(o['orient'].numpy().astype(np.uint8)[0], g['e2e_orient'][0], g['e2e_orient_lowmargin'], 'orient', 1)
    _flips_inside_noise(o['semantic_seg'].numpy().astype(np.uint8)[0], g['e2e_semantic_seg'][0], g['e2e_sem_lowmargin'], 'semantic_seg', 32)
    cls_idx = net.heads._compact['cls_idx'].cpu().numpy()[0]
    _flips_inside_noise(cls_idx, g['e2e_cls2_argmax'][0], g['e2e_cls2_lowmargin'], 'cls_idx', 4)
    off_scale = max(1.0, float(g['e2e_offset2_absmax']))
    np.testing.assert_allclose(o['cls_offset'].numpy(), g['e2e_cls_offset'], rtol=0, atol=1e-4 * off_scale)
    _close(o['prop_conf'], g['e2e_prop_conf'], 1e-4, 'prop_conf')
    assert np.array_equal(np.stack(np.nonzero(o['endp'][0].numpy()), axis=1), g['e2e_endp'])
    assert np.array_equal(np.stack(np.nonzero(o['lane_maps']['endp_by_cls'][0]), axis=1), g['e2e_endp_final'])
    _same_polylines(o['lane_maps']['cls_offset_smooth'][0], g, 'polylines')
    assert int((np.count_nonzero(g['e2e_cls_offset_smooth'][:, :, 0] > 0, axis=1) >= 2).sum()) > 0


# ----------------------------------------------------------------------------------------------- invariance, graphs, Runner
@pytest.mark.parametrize('tag', TAGS)
def test_tile_inside_batch8_bit_identical(dev, tag):
    net = _net(dev, tag)
    x = torch.from_numpy(synth.bev_batch([7200 + i for i in range(8)], 1152)).to(dev)
    with torch.no_grad():
        raw = {k: v.clone() for k, v in net.forward_raw({'proj': x}).items()}
        for t in (2, 7):
            one = net.forward_raw({'proj': x[t:t + 1].contiguous()})
            for k in ('proposal_conf', 'ext2', 'cls2', 'offset2', 'orient'):
                assert torch.equal(raw[k][t:t + 1], one[k]), f'{tag} tile {t} {k}: batch-8 result != single-tile result'


@pytest.mark.parametrize('tag', TAGS)
def test_pipeline_graph_replay_bit_identical(dev, tag):
    """TilePipeline eager vs captured-graph replay (what LANEMAP_GRAPHS=1 selects): the same lanes and endpoints; fewer than 72
    proposals come padded into the [72,144,2] block (col -1, label 0)."""
    from lanemapping_amd.pipeline import TilePipeline
    net = _net(dev, tag)
    P = net.heads.num_prop
    eager, graph = TilePipeline(net, use_graph=False), TilePipeline(net, use_graph=True)
    for seeds in ([2021, 2022], [2030, 2031]):
        x = torch.from_numpy(synth.bev_batch(seeds, 1152)).to(dev)
        want, got = eager.run_batch(x), graph.run_batch(x)
        assert len(want) == len(got) == len(seeds)
        for (la, ea), (lb, eb) in zip(want, got):
            la = np.asarray(la)
            assert la.shape == (72, 144, 2)
            assert bool((la[P:, :, 0] == -1).all()) and bool((la[P:, :, 1] == 0).all())
            assert np.array_equal(la, np.asarray(lb)) and np.array_equal(np.asarray(ea), np.asarray(eb))
    graph.clear_graphs()


def test_runner_tiles_to_json_p36(dev, golden, tmp_path, monkeypatch):
    """load_config_and_runner on config 2 with heads (36, 4), a strict reference checkpoint, a PNG tile -> per-tile JSON of the
    reference's polylines (G25 c2_p36), the 36 lanes padded into the 72-lane block."""
    from PIL import Image
    from lanemapping_amd import io_utils
    from lanemapping_amd.boundary import REPO_ROOT
    from lanemapping_amd.runner import load_config_and_runner
    g = golden('g25_propgeom_c2_p36.npz')
    net = _net(dev, 'c2_p36')
    monkeypatch.chdir(tmp_path)
    cfg_path = tmp_path / 'Proj_polyline_fpn_vit_vertex_2_p36.py'
    base = open(os.path.join(REPO_ROOT, 'configs', 'Proj_polyline_fpn_vit_vertex_2.py')).read()
    cfg_path.write_text(base + '\n' + 'heads.update(num_prop=36, prop_width=4)\n')
    ckpt = tmp_path / 'best.pth'
    torch.save({'net': {'module.' + k: v.cpu() for k, v in net.state_dict().items()}}, ckpt)
    tiles = tmp_path / 'tiles'
    tiles.mkdir()
    Image.fromarray(synth.bev_tile_u8(int(g['e2e_tile_seed']), 1152)).save(tiles / '19012021_0001_extra.png')
    cfg, runner = load_config_and_runner(str(cfg_path), '0')
    assert runner.net.heads.num_prop == 36
    runner.load_ckpt(str(ckpt))
    out = tmp_path / 'out'
    res = runner.infer_lane_coordinate_endpoint_semantics(tiles=str(tiles), batch_size=1, work_dirs=str(out), write_lane_vertex=True)
    assert list(res) == ['19012021_00']
    lanes = res['19012021_00'][0]
    assert lanes.shape == (72, 144, 2) and bool((lanes[36:, :, 0] == -1).all())
    _same_polylines(lanes[:36], g, 'runner polylines')
    recs = json.load(open(out / '19012021_00.json'))
    want = io_utils.lane_records(io_utils.pack_lane_vertices(g['e2e_cls_offset_smooth']))
    assert len(recs) == len(want) > 0 and [r['seq_len'] for r in recs] == [r['seq_len'] for r in want]
    for r, w in zip(recs, want):
        assert [v[2] for v in r['seq']] == [v[2] for v in w['seq']]
        np.testing.assert_allclose(np.array(r['seq'])[:, :2], np.array(w['seq'])[:, :2], rtol=0, atol=1e-3)


def test_colprop_head_opcheck_p18(dev):
    """The stage op's fake kernel gives the true FW-wide shapes (torch.export / opcheck see them)."""
    from lanemapping_amd import torch_ops
    h = _net(dev, 'c2_p18').heads
    x, x_up = cases.head_inputs(41)
    x = _nhwc_dev(torch.from_numpy(x), dev)
    col = ops.new_act(1, 16, 288, 288, dev)
    col[:, 8:16].copy_(torch.from_numpy(x_up).to(dev))
    w, n = torch_ops.stage_weights(h), torch_ops.stage_name(h)
    with torch.no_grad():
        torch.library.opcheck(torch.ops.lanemap_hip.colprop_head.default, (x, col, w, n), test_utils=('test_schema', 'test_faketensor'))
        conf, ext2, cls2, off2, orient = torch.ops.lanemap_hip.colprop_head(x, col, w, n)
    assert tuple(cls2.shape) == tuple(off2.shape) == (1, 18, 144, 16) and tuple(conf.shape) == (1, 18, 2)
