"""GPU tests (-m gpu) of ColumnProposal2 with column_att=True (the proposal-attention branch, heads/polyline_fpn_vit_vertex_2.py:317-345):
lm_conv2d_nhwc_small widened to Cout 32 / 48 / 64 against fp64 and under guarded buffers, then the branch's stages, the head and the
whole net against the reference's goldens G27 (tests/golden/make_golden_colatt.py), batch invariance, graph replay, the Runner entry,
opcheck of the stage op, and the column_att=False outputs of the same weights unchanged (G25)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from gpu_common import (_cached_net, _chk, _close, _close_sampled, _flips_inside_noise, _g, _lib, _nhwc_dev, _nhwc_rows, _rows_nchw,
                        _same_polylines)
from guards import INF, NAN, Slab, batched, guarded_runs
from lanemapping_amd import ops, synth
from test_column_att_cpu import _layouts, build_colatt

pytestmark = pytest.mark.gpu

TAGS = ('att_p72', 'att_p36', 'att_p18', 'att_t2')


# ----------------------------------------------------------------------------------------------- widened small conv
@pytest.mark.parametrize('name,H,W,cin,cout,k,stride,pre_relu', [
    ('mfma_c8_o32_s2', 37, 29, 8, 32, 3, 2, False),     # generate_line_proposal at num_prop 72 (16 real + 16 zero outputs)
    ('mfma_c16_o32_s2', 37, 29, 16, 32, 3, 2, True),    # (36, 4) / (18, 8) second stage
    ('mfma_c32_o64_s2', 37, 29, 32, 64, 3, 2, False),   # (18, 8) third stage
    ('mfma_c8_o48_s1', 19, 35, 8, 48, 3, 1, True),
    ('mfma_c16_o64_s1', 19, 35, 16, 64, 3, 1, False),
    ('mfma_c32_o48_s2', 40, 33, 32, 48, 3, 2, True),
    ('mfma_c32_o32_s1', 17, 17, 32, 32, 3, 1, False),
    ('valu_c32_o32_1x1', 19, 23, 32, 32, 1, 1, False),  # the diagonal BatchNorm of a 32-channel stage: one VALU launch per 16 outputs
    ('valu_c8_o48_5x3', 19, 23, 8, 48, (5, 3), 1, True),
    ('valu_c12_o64_s2', 19, 23, 12, 64, 3, 2, False),   # Cin outside {8, 16, 32}: VALU
])
def test_small_conv_wide_bounds(dev, name, H, W, cin, cout, k, stride, pre_relu):
    """lm_conv2d_nhwc_small with Cout > 16 vs fp64 F.conv2d: x a slice (ldx = Cin + 4 at column 4), y a slice (ldy = Cout + 8 at column
    4), scale and shift, ragged H / W; poisoned guards, canaries and batch independence (tests/guards.py)."""
    kh, kw = (k, k) if isinstance(k, int) else k
    g = _g(H * cin + cout + stride)
    x = torch.randn(1, cin, H, W, generator=g)
    w = torch.randn(cout, cin, kh, kw, generator=g) / (cin * kh * kw) ** 0.5
    if pre_relu:
        w = w.abs()
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    xin = F.relu(x.double()) if pre_relu else x.double()
    ref = F.conv2d(xin, w.double(), None, stride, (kh // 2, kw // 2)) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    Ho, Wo = ref.shape[2:]
    w16, scd, shd = ops.pack_small(w.to(dev)), sc.to(dev), sh.to(dev)
    assert tuple(w16.shape) == (cout // 16, kh * kw, cin, 16)
    poison = INF if pre_relu else NAN
    ldx, ldy, P, Po = cin + 4, cout + 8, H * W, Ho * Wo

    def run(B, poisoned):
        pad = poison if poisoned else 0.0
        xs = Slab(dev, B * P, cin, ldx, 4, 256 + 2 * W, 256 + 2 * W).fill_input(batched(_nhwc_rows(x[:1]), B, poison), pad)
        ys = Slab(dev, B * Po, cout, ldy, 4, 256, 256).fill_canary()
        _chk(_lib().lm_conv2d_nhwc_small(ops._stream(), xs.ptr(), ldx, w16.data_ptr(), scd.data_ptr(), shd.data_ptr(), ys.ptr(), ldy, B,
                                         H, W, cin, cout, kh, kw, stride, kh // 2, kw // 2, int(pre_relu), ops.ACT_NONE))
        return {'y': (ys, Po)}
    y = guarded_runs(run, f'conv_small {name}')['y']
    _close(_rows_nchw(y, 1, Ho, Wo), ref, 1e-5, name)


@pytest.mark.parametrize('cout', [32, 64])
def test_small_conv_wide_relu_no_scale(dev, cout):
    """act = RELU without a scale (the stride-2 stages of generate_line_proposal): through ops.conv_small on an NHWC tensor."""
    g = _g(300 + cout)
    x = torch.randn(2, 16, 30, 26, generator=g)
    w = torch.randn(cout, 16, 3, 3, generator=g) / 12
    b = torch.randn(cout, generator=g)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), 2, 1))
    with torch.no_grad():
        y = ops.conv_small(_nhwc_dev(x, dev), ops.pack_small(w.to(dev)), cout, 3, 3, 2, 1, shift=b.to(dev), act=ops.ACT_RELU)
    assert y.stride(1) == 1
    _close(y, ref, 1e-5, f'relu cout {cout}')


@pytest.mark.parametrize('cout', [65, 40, 17, 80])
def test_small_conv_wide_refusals(dev, cout):
    x = torch.zeros(1, 4, 4, 16, device=dev)
    w = torch.zeros(max(cout, 16) * 9 * 16, device=dev)
    y = torch.zeros(1, 4, 4, cout, device=dev)
    with pytest.raises(RuntimeError, match='Cout'):
        _chk(_lib().lm_conv2d_nhwc_small(ops._stream(), x.data_ptr(), 16, w.data_ptr(), None, None, y.data_ptr(), cout, 1, 4, 4, 16, cout,
                                         3, 3, 1, 1, 1, 0, ops.ACT_NONE))


# ----------------------------------------------------------------------------------------------- goldens
def _net(dev, tag):
    """The tag's column_att net with the synthetic weights of seed 2021 on the GPU (tests restore whatever they change)."""
    return _cached_net(dev, (__name__, tag), lambda: build_colatt(_layouts()[tag]['heads']))


@pytest.mark.parametrize('tag', TAGS)
def test_stages_golden(dev, golden, tag):
    """feat_down, the tokens after tr_lane_correlator and colfeat [B,8,144,P] within 1e-4 of the reference's scale, at batch 2."""
    g = golden(f'g27_colatt_{tag}.npz')
    h = _net(dev, tag).heads
    x, _ = cases.head_inputs(int(g['input_seed']), batch=int(g['batch']))
    with torch.no_grad():
        P = h.packed()
        if 'ca.tok.w' not in P:
            P.update(h._pack_column_att())
        colfeat, feat_down, tok = h._column_att_features(_nhwc_dev(torch.from_numpy(x), dev), P)
    cd = int(g['stage_feat_down_shape'][1])
    assert feat_down.shape[1] == max(cd, 32)
    assert bool((feat_down[:, cd:] == 0).all()), 'padded feat_down channels must be exact zeros'
    _close_sampled(feat_down[:, :cd], g, 'stage_feat_down')
    _close_sampled(tok.reshape(x.shape[0], h.num_prop, -1), g, 'stage_tok')
    _close_sampled(colfeat, g, 'stage_colfeat')


@pytest.mark.parametrize('tag', TAGS)
def test_head_golden(dev, golden, tag):
    g = golden(f'g27_colatt_{tag}.npz')
    net = _net(dev, tag)
    x, x_up = cases.head_inputs(int(g['input_seed']), batch=int(g['batch']))
    with torch.no_grad():
        out = net.heads(torch.from_numpy(x).to(dev), torch.from_numpy(x_up).to(dev), None)
    _close(out['proposal_conf'], g['head_proposal_conf'], 1e-4, 'proposal_conf')
    for k in ('ext2', 'cls2', 'offset2', 'orient'):
        _close_sampled(out[k], g, f'head_{k}')
    for k, dim in (('cls2', -1), ('orient', 1)):
        _flips_inside_noise(out[k].argmax(dim).cpu().numpy(), g[f'head_{k}_argmax'], g[f'head_{k}_lowmargin'], k, 10 ** 9)


@pytest.mark.parametrize('tag', TAGS)
def test_end_to_end_golden(dev, golden, tag):
    """One full 1152^2 tile through Detector1stage with column_att vs the reference's own end-to-end run (G25 tolerances)."""
    g = golden(f'g27_colatt_{tag}.npz')
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


def test_column_att_changes_the_outputs(dev, golden):
    """The branch is live: with column_att=False the same weights give ext2 far from G27's (the goldens pin the branch)."""
    g = golden('g27_colatt_att_p72.npz')
    h = _net(dev, 'att_p72').heads
    x, x_up = cases.head_inputs(int(g['input_seed']), batch=int(g['batch']))
    h.cfg.column_att = False
    try:
        with torch.no_grad():
            out = h(torch.from_numpy(x).to(dev), torch.from_numpy(x_up).to(dev), None)
    finally:
        h.cfg.column_att = True
    with pytest.raises(AssertionError):
        _close_sampled(out['ext2'], g, 'head_ext2')


@pytest.mark.parametrize('tag,g25', [('att_p36', 'c2_p36'), ('att_p18', 'c2_p18')])
def test_column_att_false_unchanged(dev, golden, tag, g25):
    """column_att=False on the same weights (the layouts are the same, so is fill_module_) keeps today's outputs: G25's head golden, and
    bit-identical outputs before and after a column_att run in the same process."""
    g = golden(f'g25_propgeom_{g25}.npz')
    net = _net(dev, tag)
    h = net.heads
    x, x_up = cases.head_inputs(int(g['input_seed']))
    xd, xud = torch.from_numpy(x).to(dev), torch.from_numpy(x_up).to(dev)
    h.cfg.column_att = False
    try:
        with torch.no_grad():
            before = {k: v.clone() for k, v in h(xd, xud, None).items()}
            h.cfg.column_att = True
            h(xd, xud, None)
            h.cfg.column_att = False
            after = h(xd, xud, None)
    finally:
        h.cfg.column_att = True
    _close(before['proposal_conf'], g['head_proposal_conf'], 1e-4, 'proposal_conf')
    for k in ('ext2', 'cls2', 'offset2', 'orient'):
        _close_sampled(before[k], g, f'head_{k}')
        assert torch.equal(before[k], after[k]), k


# ----------------------------------------------------------------------------------------------- invariance, graphs, Runner, opcheck
@pytest.mark.parametrize('tag', ['att_p72', 'att_p18', 'att_t2'])
def test_tile_inside_batch3_bit_identical(dev, tag):
    net = _net(dev, tag)
    x = torch.from_numpy(synth.bev_batch([7300 + i for i in range(3)], 1152)).to(dev)
    with torch.no_grad():
        raw = {k: v.clone() for k, v in net.forward_raw({'proj': x}).items()}
        one = net.forward_raw({'proj': x[1:2].contiguous()})
    for k in ('proposal_conf', 'ext2', 'cls2', 'offset2', 'orient'):
        assert torch.equal(raw[k][1:2], one[k]), f'{tag} tile 1 {k}: batch-3 result != single-tile result'


@pytest.mark.parametrize('tag', ['att_p72', 'att_p36'])
def test_pipeline_graph_replay_bit_identical(dev, tag):
    """TilePipeline eager vs captured-graph replay with column_att: the same lanes and endpoints."""
    from lanemapping_amd.pipeline import TilePipeline
    net = _net(dev, tag)
    eager, graph = TilePipeline(net, use_graph=False), TilePipeline(net, use_graph=True)
    for seeds in ([2021, 2022], [2030, 2031]):
        x = torch.from_numpy(synth.bev_batch(seeds, 1152)).to(dev)
        want, got = eager.run_batch(x), graph.run_batch(x)
        assert len(want) == len(got) == len(seeds)
        for (la, ea), (lb, eb) in zip(want, got):
            assert np.array_equal(np.asarray(la), np.asarray(lb)) and np.array_equal(np.asarray(ea), np.asarray(eb))
    graph.clear_graphs()


def test_runner_tiles_to_json(dev, golden, tmp_path, monkeypatch):
    """load_config_and_runner on config 2 with column_att = True, a strict reference checkpoint, a PNG tile -> per-tile JSON of the
    reference's polylines (G27 att_p72)."""
    from PIL import Image
    from lanemapping_amd import io_utils
    from lanemapping_amd.boundary import REPO_ROOT
    from lanemapping_amd.runner import load_config_and_runner
    g = golden('g27_colatt_att_p72.npz')
    net = _net(dev, 'att_p72')
    monkeypatch.chdir(tmp_path)
    cfg_path = tmp_path / 'Proj_polyline_fpn_vit_vertex_2_colatt.py'
    base = open(os.path.join(REPO_ROOT, 'configs', 'Proj_polyline_fpn_vit_vertex_2.py')).read()
    cfg_path.write_text(base + '\ncolumn_att = True\n')
    ckpt = tmp_path / 'best.pth'
    torch.save({'net': {'module.' + k: v.cpu() for k, v in net.state_dict().items()}}, ckpt)
    tiles = tmp_path / 'tiles'
    tiles.mkdir()
    Image.fromarray(synth.bev_tile_u8(int(g['e2e_tile_seed']), 1152)).save(tiles / '19012021_0001_extra.png')
    cfg, runner = load_config_and_runner(str(cfg_path), '0')
    assert runner.net.heads.cfg.column_att is True
    runner.load_ckpt(str(ckpt))
    out = tmp_path / 'out'
    res = runner.infer_lane_coordinate_endpoint_semantics(tiles=str(tiles), batch_size=1, work_dirs=str(out), write_lane_vertex=True)
    assert list(res) == ['19012021_00']
    _same_polylines(res['19012021_00'][0], g, 'runner polylines')
    recs = json.load(open(out / '19012021_00.json'))
    want = io_utils.lane_records(io_utils.pack_lane_vertices(g['e2e_cls_offset_smooth']))
    assert len(recs) == len(want) > 0 and [r['seq_len'] for r in recs] == [r['seq_len'] for r in want]
    for r, w in zip(recs, want):
        assert [v[2] for v in r['seq']] == [v[2] for v in w['seq']]
        np.testing.assert_allclose(np.array(r['seq'])[:, :2], np.array(w['seq'])[:, :2], rtol=0, atol=1e-3)


def test_colprop_head_opcheck(dev):
    from lanemapping_amd import torch_ops
    h = _net(dev, 'att_p36').heads
    x, x_up = cases.head_inputs(41)
    x = _nhwc_dev(torch.from_numpy(x), dev)
    col = ops.new_act(1, 16, 288, 288, dev)
    col[:, 8:16].copy_(torch.from_numpy(x_up).to(dev))
    w, n = torch_ops.stage_weights(h), torch_ops.stage_name(h)
    with torch.no_grad():
        torch.library.opcheck(torch.ops.lanemap_hip.colprop_head.default, (x, col, w, n), test_utils=('test_schema', 'test_faketensor'))
        conf, ext2, cls2, off2, orient = torch.ops.lanemap_hip.colprop_head(x, col, w, n)
    assert tuple(cls2.shape) == tuple(off2.shape) == (1, 36, 144, 12) and tuple(conf.shape) == (1, 36, 2)
