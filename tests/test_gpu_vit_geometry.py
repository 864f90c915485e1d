"""GPU tests (-m gpu) of VitSegNet (GFC-T) at patch sizes 4 / 6 / 12 / 16: the long-sequence attention path of lm_attention_f32
(attention_flash_kernel, N >= 382 tokens) and the other LayerNorm widths of lm_layernorm_rows against fp64 and under guarded buffers,
then the backbone and the whole net against the reference's goldens G26 (tests/golden/make_golden_vitgeom.py), batch invariance, graph
replay, the stage op's fake kernel and the Runner entry."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from gpu_common import _cached_net, _chk, _close, _close_sampled, _flips_inside_noise, _g, _lib, _same_polylines
from guards import NAN, Slab, batched, guarded_runs
from lanemapping_amd import ops, synth
from test_vit_geometry_cpu import _layouts, build_geometry

pytestmark = pytest.mark.gpu

TAGS = ('p4', 'p6', 'p12', 'p16', 'p4_mlp')
E2E_TAGS = ('p4', 'p6')


def _net(dev, tag):
    """The geometry's net with the synthetic weights of seed 2021 on the GPU (tests do not mutate it)."""
    def build():
        ref = _layouts()[tag]
        return build_geometry(ref['backbone'], ref['config'])
    return _cached_net(dev, (__name__, tag), build)


# ----------------------------------------------------------------------------------------------- attention, N >= 382
def _qkv(B, N, heads, seed, amp=3.0):
    """Activations of scale 3: scores q.k / 8 spread over tens of units, so a later key block's max exceeds the running max in most rows
    and the online rescale exp(m_old - m_new) fires; a ramp on the keys makes the last (ragged) block hold many row maxima."""
    g = _g(seed)
    qkv = torch.randn((B * N, 3 * heads * 64), generator=g) * amp
    ramp = torch.linspace(0.5, 1.5, N).repeat(B)[:, None]
    qkv[:, heads * 64:2 * heads * 64] *= ramp
    return qkv


def _attn64(qkv, B, N, heads, dev):
    """fp64 softmax(q k^T / 8) v on the device, one batch element at a time."""
    outs = []
    for b in range(B):
        q, k, v = [z.reshape(N, heads, 64).transpose(0, 1).to(dev, torch.float64) for z in qkv[b * N:(b + 1) * N].chunk(3, dim=-1)]
        o = torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v
        outs.append(o.transpose(0, 1).reshape(N, heads * 64).cpu())
    return torch.cat(outs)


def _rescale_fires(qkv, N, heads):
    """Fraction of (query, head) rows of batch element 0 whose running max over 32-key blocks rises after the first block."""
    q, k = [z.reshape(N, heads, 64).transpose(0, 1).double() for z in qkv[:N].chunk(3, dim=-1)[:2]]
    s = q[:, :256] @ k.transpose(-1, -2) * 0.125
    nb = (N + 31) // 32
    bm = torch.stack([s[..., 32 * i:min(N, 32 * i + 32)].amax(-1) for i in range(nb)], -1)
    return float((bm[..., 1:].amax(-1) > bm[..., 0]).double().mean())


@pytest.mark.parametrize('N', [382, 576, 1000, 1296, 2304, 5184])
@pytest.mark.parametrize('B,heads', [(1, 1), (1, 16), (2, 16), (16, 1)])
def test_flash_attention_vs_fp64(dev, N, B, heads):
    qkv = _qkv(B, N, heads, N + 7 * B + heads)
    assert _rescale_fires(qkv, N, heads) > 0.5
    got = ops.attention(qkv.to(dev).contiguous(), B, N, heads, 64, 0.125)
    _close(got, _attn64(qkv, B, N, heads, dev), 1e-5, f'attention N={N} B={B} heads={heads}')


def test_flash_attention_b16_h16_vs_fp64_repeat_and_batch_invariant(dev):
    """N = 1296 (patch 4), B = 16, 16 heads: fp64; a second run bit-identical; every batch element bit-identical to a B = 1 call on
    its rows."""
    B, N, heads = 16, 1296, 16
    qkv = _qkv(B, N, heads, 4242).to(dev).contiguous()
    got = ops.attention(qkv, B, N, heads, 64, 0.125)
    _close(got, _attn64(qkv.cpu(), B, N, heads, dev), 1e-5, 'attention N=1296 B=16')
    assert torch.equal(got, ops.attention(qkv, B, N, heads, 64, 0.125)), 'repeat run differs'
    for k in range(B):
        one = ops.attention(qkv[k * N:(k + 1) * N].contiguous(), 1, N, heads, 64, 0.125)
        assert torch.equal(one, got[k * N:(k + 1) * N]), f'batch element {k} of 16 != the B = 1 call'


@pytest.mark.parametrize('N', [382, 1000, 1296])
def test_flash_attention_bounds(dev, N):
    """lm_attention_f32 on the long-sequence path, two heads.  Guards: 64 token rows on qkv and out (one LDS stage of keys)."""
    heads = 2
    qkv = _qkv(1, N, heads, 900 + N)
    ref = _attn64(qkv, 1, N, heads, dev)

    def run(B, poisoned):
        qs = Slab(dev, B * N, 3 * heads * 64, None, 0, 64, 64).fill_input(batched(qkv, B, NAN), NAN if poisoned else 0.0)
        ys = Slab(dev, B * N, heads * 64, None, 0, 64, 64).fill_canary()
        _chk(_lib().lm_attention_f32(ops._stream(), qs.ptr(), ys.ptr(), B, N, heads, 64, C.c_float(0.125)))
        return {'out': (ys, N)}
    y = guarded_runs(run, f'attention N={N}')['out']
    _close(y, ref, 1e-5, f'attention N={N}')


# ----------------------------------------------------------------------------------------------- LayerNorm, other widths
@pytest.mark.parametrize('D', [32, 96, 128, 288, 1152, 2048, 4096])
def test_layernorm_widths_vs_fp64(dev, D):
    g = _g(D)
    x = torch.randn(333, D, generator=g) * 3 + 1
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    y = ops.layernorm(x.to(dev), gamma.to(dev), beta.to(dev), 1e-5)
    _close(y, F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5), 1e-5, f'layernorm {D}')


@pytest.mark.parametrize('D', [128, 288, 2048])
def test_layernorm_widths_bounds(dev, D):
    """lm_layernorm_rows at the patch-4 / 6 / 16 widths: 37 rows per batch element.  Guards: 64 rows."""
    rows = 37
    g = _g(D + 1)
    x = torch.randn(rows, D, generator=g) * 3 + 1
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    ref = F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5)
    gd, bd = gamma.to(dev), beta.to(dev)

    def run(B, poisoned):
        xs = Slab(dev, B * rows, D, None, 0, 64, 64).fill_input(batched(x, B, NAN), NAN if poisoned else 0.0)
        ys = Slab(dev, B * rows, D, None, 0, 64, 64).fill_canary()
        _chk(_lib().lm_layernorm_rows(ops._stream(), xs.ptr(), gd.data_ptr(), bd.data_ptr(), ys.ptr(), B * rows, D, C.c_float(1e-5)))
        return {'y': (ys, rows)}
    y = guarded_runs(run, f'layernorm {D}')['y']
    _close(y, ref, 1e-5, 'layernorm')


# ----------------------------------------------------------------------------------------------- goldens G26
@pytest.mark.parametrize('tag', TAGS)
def test_backbone_golden(dev, golden, tag):
    g = golden(f'g26_vitgeom_{tag}.npz')
    bb = _net(dev, tag).backbone
    with torch.no_grad():
        y = bb(torch.from_numpy(cases.vit_input(int(g['input_seed']))).to(dev))
        y2 = bb(torch.from_numpy(np.concatenate([cases.vit_input(int(s)) for s in g['batch2_seeds']])).to(dev))
    assert y.stride(1) == 1, 'NHWC-stored like every activation'
    _close_sampled(y, g, 'bb_out')
    _close_sampled(y2, g, 'bb_out_batch2')


@pytest.mark.parametrize('tag', E2E_TAGS)
def test_end_to_end_golden(dev, golden, tag):
    """One full 1152^2 tile through Detector1stage at this backbone geometry vs the reference's own run (G25 tolerances)."""
    g = golden(f'g26_vitgeom_{tag}.npz')
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


# ----------------------------------------------------------------------------------------------- invariance, graphs, op, Runner
@pytest.mark.parametrize('tag', E2E_TAGS)
def test_tile_inside_batch8_bit_identical(dev, tag):
    net = _net(dev, tag)
    x = torch.from_numpy(synth.bev_batch([7300 + i for i in range(8)], 1152)).to(dev)
    with torch.no_grad():
        raw = {k: v.clone() for k, v in net.forward_raw({'proj': x}).items()}
        for t in (2, 7):
            one = net.forward_raw({'proj': x[t:t + 1].contiguous()})
            for k in ('proposal_conf', 'ext2', 'cls2', 'offset2', 'orient'):
                assert torch.equal(raw[k][t:t + 1], one[k]), f'{tag} tile {t} {k}: batch-8 result != single-tile result'


@pytest.mark.parametrize('tag', E2E_TAGS)
def test_pipeline_graph_replay_bit_identical(dev, tag):
    """TilePipeline eager vs captured-graph replay (what LANEMAP_GRAPHS=1 selects): the same lanes and endpoints."""
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


def test_vit_backbone_opcheck_p4(dev):
    """The stage op's fake kernel gives the true shape at patch 4 (torch.export / opcheck see it)."""
    from lanemapping_amd import torch_ops
    bb = _net(dev, 'p4').backbone
    w, n = torch_ops.stage_weights(bb), torch_ops.stage_name(bb)
    fea = ops.new_act(2, 64, 144, 144, dev)
    fea.copy_(torch.from_numpy(np.concatenate([cases.vit_input(32), cases.vit_input(33)])).to(dev))
    with torch.no_grad():
        torch.library.opcheck(torch.ops.lanemap_hip.vit_backbone.default, (fea, w, n), test_utils=('test_schema', 'test_faketensor'))
        y = torch.ops.lanemap_hip.vit_backbone(fea, w, n)
    assert tuple(y.shape) == (2, 8, 144, 144) and y.stride(1) == 1


def test_runner_tiles_to_json_p4(dev, tmp_path, monkeypatch):
    """load_config_and_runner on a copy of config 2 with a patch-4 backbone and a strict checkpoint: per-tile JSON of exactly the lanes
    TilePipeline computes for the same net and tile."""
    from PIL import Image
    from lanemapping_amd import io_utils
    from lanemapping_amd.boundary import REPO_ROOT
    from lanemapping_amd.pipeline import TilePipeline
    from lanemapping_amd.runner import load_config_and_runner
    net = _net(dev, 'p4')
    monkeypatch.chdir(tmp_path)
    cfg_path = tmp_path / 'Proj_polyline_fpn_vit_vertex_2_p4.py'
    base = open(os.path.join(REPO_ROOT, 'configs', 'Proj_polyline_fpn_vit_vertex_2.py')).read()
    cfg_path.write_text(base + '\n' + 'backbone.update(patch_h_size=4, patch_w_size=4, dim=128)\n')
    ckpt = tmp_path / 'best.pth'
    torch.save({'net': {'module.' + k: v.cpu() for k, v in net.state_dict().items()}}, ckpt)
    tiles = tmp_path / 'tiles'
    tiles.mkdir()
    tile = synth.bev_tile_u8(2021, 1152)
    Image.fromarray(tile).save(tiles / '19012021_0001_extra.png')
    cfg, runner = load_config_and_runner(str(cfg_path), '0')
    assert runner.net.backbone.patch == 4 and runner.net.backbone.dim == 128
    runner.load_ckpt(str(ckpt))
    out = tmp_path / 'out'
    res = runner.infer_lane_coordinate_endpoint_semantics(tiles=str(tiles), batch_size=1, work_dirs=str(out), write_lane_vertex=True)
    assert list(res) == ['19012021_00']
    lanes = np.asarray(res['19012021_00'][0])
    x = torch.from_numpy(synth.bev_batch([2021], 1152)).to(dev)
    want, _ = TilePipeline(net, use_graph=False).run_batch(x)[0]
    assert np.array_equal(lanes, np.asarray(want))
    recs = json.load(open(out / '19012021_00.json'))
    expect = io_utils.lane_records(io_utils.pack_lane_vertices(np.asarray(want)))
    assert len(recs) == len(expect) > 0 and [r['seq_len'] for r in recs] == [r['seq_len'] for r in expect]
    for r, w in zip(recs, expect):
        assert [v[2] for v in r['seq']] == [v[2] for v in w['seq']]
        np.testing.assert_allclose(np.array(r['seq'])[:, :2], np.array(w['seq'])[:, :2], rtol=0, atol=1e-3)
