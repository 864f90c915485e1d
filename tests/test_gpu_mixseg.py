"""GPU tests (-m gpu) of the MLP-Mixer lane config (configs/Proj_polyline_fpn_mixseg_vertex.py): the token-mixing kernel
(lm_token_mix_mfma_f32) against fp64 torch, MixSegNet / the spatial_att=False head / the whole net against the reference's goldens
G21-G23 (tests/golden/make_golden_mixseg.py), batch invariance, graph replay, the Runner entry and the stage op's registration."""
import json
import os

import numpy as np
import pytest
import torch

import cases
from gpu_common import _close, _close_sampled, _same_polylines
from lanemapping_amd import ops, synth

pytestmark = pytest.mark.gpu

NAME = 'Proj_polyline_fpn_mixseg_vertex'


@pytest.fixture(scope='module')
def mnet(dev):
    """MixSeg detector with the synthetic weights of seed 2021 on the GPU (tests do not mutate it)."""
    from lanemapping_amd.boundary import build_net_from_config
    n = build_net_from_config(NAME, device='cpu')
    synth.fill_module_(n, 2021)
    return n.to(dev)


# ----------------------------------------------------------------------------------------------- token-mixing kernel
def _token_mix_case(dev, B, K, M, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * K, N, generator=g, dtype=torch.float64)
    w = torch.randn(M, K, generator=g, dtype=torch.float64) / K ** 0.5
    bias = torch.randn(M, generator=g, dtype=torch.float64) * 0.1
    res = torch.randn(B * M, N, generator=g, dtype=torch.float64)
    return x, w, bias, res


def _token_mix_ref(x, w, bias, B, res=None, gelu=False):
    K, N = x.shape[0] // B, x.shape[1]
    y = torch.einsum('mk,bkn->bmn', w, x.reshape(B, K, N)) + bias[None, :, None]
    if gelu:
        y = 0.5 * y * (1.0 + torch.erf(y / 2 ** 0.5))
    y = y.reshape(-1, N)
    return y + res if res is not None else y


@pytest.mark.parametrize('B,K,M,N,act,with_res', [
    (16, 324, 1296, 512, 'gelu', False),     # the Mixer's first token-mixing layer at batch 16
    (16, 1296, 324, 512, 'none', True),      # the second one, residual added
    (1, 324, 1296, 512, 'gelu', True),       # batch 1 (the small-tile route)
    (1, 1296, 324, 512, 'none', False),
    (3, 37, 70, 96, 'gelu', True),           # K not a multiple of 8, M not a multiple of any tile, N not a multiple of 64
    (2, 5, 129, 12, 'none', True),           # K below one slab, M one past a 128 tile
])
def test_token_mix_vs_fp64(dev, B, K, M, N, act, with_res):
    x, w, bias, res = _token_mix_case(dev, B, K, M, N, seed=K * 7 + M)
    gelu = act == 'gelu'
    want = _token_mix_ref(x, w, bias, B, res if with_res else None, gelu)
    y = ops.token_mix(x.float().to(dev), ops.pack_token_mix(w.float().to(dev)), M, bias.float().to(dev), B,
                      res=res.float().to(dev) if with_res else None, act=ops.ACT_GELU if gelu else ops.ACT_NONE)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (B * M, N)
    _close(y, want, 1e-5, f'token_mix B{B} K{K} M{M} N{N} {act} res={with_res}')


@pytest.mark.parametrize('K,M', [(324, 1296), (1296, 324), (37, 70)])
def test_token_mix_batch_isolation(dev, K, M):
    """A batch element computed alone equals the same element inside a batch of 16, bit for bit - with NaN in every other element,
    so a K-tail load that crossed into the next batch element would show."""
    B, N, pick = 16, 512, 5
    x, w, bias, res = _token_mix_case(dev, B, K, M, N, seed=11)
    x = x.float().to(dev)
    res = res.float().to(dev)
    wt, b = ops.pack_token_mix(w.float().to(dev)), bias.float().to(dev)
    one = ops.token_mix(x[pick * K:(pick + 1) * K].contiguous(), wt, M, b, 1, res=res[pick * M:(pick + 1) * M].contiguous(),
                        act=ops.ACT_GELU)
    full = ops.token_mix(x, wt, M, b, B, res=res, act=ops.ACT_GELU)
    assert torch.equal(full[pick * M:(pick + 1) * M], one)
    xn = torch.full_like(x, float('nan'))
    xn[pick * K:(pick + 1) * K] = x[pick * K:(pick + 1) * K]
    poisoned = ops.token_mix(xn, wt, M, b, B, res=res, act=ops.ACT_GELU)
    assert torch.equal(poisoned[pick * M:(pick + 1) * M], one)
    assert torch.isnan(poisoned[(pick + 1) * M:]).all()


# ----------------------------------------------------------------------------------------------- goldens
def test_mixseg_backbone_golden_g21(dev, mnet, golden):
    g = golden('g21_mixseg_backbone.npz')
    with torch.no_grad():
        y = mnet.backbone(torch.from_numpy(cases.vit_input(int(g['input_seed']))).to(dev))
        x2 = np.concatenate([cases.vit_input(int(s)) for s in g['batch2_seeds']])
        y2 = mnet.backbone(torch.from_numpy(x2).to(dev))
    assert y.stride(1) == 1, 'NHWC-stored like every activation'
    _close_sampled(y, g, 'out')
    _close_sampled(y2, g, 'out_batch2')


def test_mixseg_head_golden_g22(dev, mnet, golden):
    """ColumnProposal2 with spatial_att=False (raw row windows as tokens) vs the reference."""
    g = golden('g22_mixseg_head.npz')
    x, x_up = cases.head_inputs(int(g['input_seed']))
    with torch.no_grad():
        out = mnet.heads(torch.from_numpy(x).to(dev), torch.from_numpy(x_up).to(dev), None)
    _close(out['proposal_conf'], g['proposal_conf'], 1e-4, 'proposal_conf')
    for k in ('ext2', 'cls2', 'offset2', 'orient'):
        _close_sampled(out[k], g, k)
    for k, dim in (('cls2', -1), ('orient', 1)):
        bad = np.flatnonzero(out[k].argmax(dim).cpu().numpy().reshape(-1) != g[f'{k}_argmax'].reshape(-1))
        outside = np.setdiff1d(bad, g[f'{k}_lowmargin'])
        assert outside.size == 0, f'{k}: {outside.size} argmax flips where the reference margin is >= 1e-4'


def test_mixseg_end_to_end_golden_g23(dev, mnet, golden):
    """One full 1152^2 tile through Detector1stage (MixSeg config) vs the reference's own end-to-end run."""
    g = golden('g23_mixseg_e2e.npz')
    x = torch.from_numpy(synth.bev_batch([int(g['tile_seed'])], 1152)).to(dev)
    with torch.no_grad():
        raw = mnet.forward_raw({'proj': x})
        _close(raw['proposal_conf'], g['proposal_conf'], 1e-4, 'proposal_conf')
        for k, gk in (('ext2', 'ext2'), ('cls2', 'cls2'), ('offset2', 'offset2'), ('orient', 'orient_logits')):
            _close_sampled(raw[k], g, gk)
        o = mnet({'proj': x})

    def flips_inside_noise(mine, ref, low_idx, name, budget):
        bad = np.flatnonzero(mine.reshape(-1) != ref.reshape(-1))
        outside = np.setdiff1d(bad, low_idx)
        assert outside.size == 0, f'{name}: {outside.size} mismatches where the reference margin is >= 1e-4'
        assert bad.size <= budget, f'{name}: {bad.size} noise-margin flips (budget {budget})'
    flips_inside_noise(o['prop_v_ext'].numpy().astype(np.uint8)[0], g['prop_v_ext'][0], g['ext_lowmargin'], 'prop_v_ext', 0)
    flips_inside_noise(o['orient'].numpy().astype(np.uint8)[0], g['orient'][0], g['orient_lowmargin'], 'orient', 1)
    flips_inside_noise(o['semantic_seg'].numpy().astype(np.uint8)[0], g['semantic_seg'][0], g['sem_lowmargin'], 'semantic_seg', 32)
    cls_idx = mnet.heads._compact['cls_idx'].cpu().numpy()[0]
    flips_inside_noise(cls_idx, g['cls2_argmax'][0], g['cls2_lowmargin'], 'cls_idx', 4)
    off_scale = max(1.0, float(g['offset2_absmax']))
    np.testing.assert_allclose(o['cls_offset'].numpy(), g['cls_offset'], rtol=0, atol=1e-4 * off_scale)
    _close(o['prop_conf'], g['prop_conf'], 1e-4, 'prop_conf')
    assert np.array_equal(np.stack(np.nonzero(o['endp'][0].numpy()), axis=1), g['endp'])
    assert np.array_equal(np.stack(np.nonzero(o['lane_maps']['endp_by_cls'][0]), axis=1), g['endp_final'])
    _same_polylines(o['lane_maps']['cls_offset_smooth'][0], g, 'polylines', prefix='')


def test_mixseg_tile_inside_batch8_bit_identical(dev, mnet):
    seeds = [7100 + i for i in range(8)]
    x = torch.from_numpy(synth.bev_batch(seeds, 1152)).to(dev)
    with torch.no_grad():
        raw = {k: v.clone() for k, v in mnet.forward_raw({'proj': x}).items()}
        for t in (3, 6):
            one = mnet.forward_raw({'proj': x[t:t + 1].contiguous()})
            for k in ('proposal_conf', 'ext2', 'cls2', 'offset2', 'orient', 'semantic_seg', 'endp_est'):
                assert torch.equal(raw[k][t:t + 1], one[k]), f'tile {t} {k}: batch-8 result != single-tile result'


def test_mixseg_pipeline_graph_replay_bit_identical(dev, mnet):
    from lanemapping_amd.pipeline import TilePipeline
    eager, graph = TilePipeline(mnet, use_graph=False), TilePipeline(mnet, use_graph=True)
    for seeds in ([2021, 2022], [2030, 2031]):
        x = torch.from_numpy(synth.bev_batch(seeds, 1152)).to(dev)
        want, got = eager.run_batch(x), graph.run_batch(x)
        assert len(want) == len(got) == len(seeds)
        for (la, ea), (lb, eb) in zip(want, got):
            assert np.array_equal(np.asarray(la), np.asarray(lb)) and np.array_equal(np.asarray(ea), np.asarray(eb))
    graph.clear_graphs()


def test_mixseg_runner_tiles_to_json(dev, mnet, golden, tmp_path, monkeypatch):
    """The reference's call: load_config_and_runner(config, '0'), a strict reference checkpoint, PNG tiles -> per-tile JSON of the
    polylines the entry returns, which are G23's."""
    from PIL import Image
    from lanemapping_amd import io_utils
    from lanemapping_amd.boundary import REPO_ROOT
    from lanemapping_amd.runner import load_config_and_runner
    g = golden('g23_mixseg_e2e.npz')
    monkeypatch.chdir(tmp_path)
    ckpt = tmp_path / 'best.pth'
    torch.save({'net': {'module.' + k: v.cpu() for k, v in mnet.state_dict().items()}}, ckpt)
    tiles = tmp_path / 'tiles'
    tiles.mkdir()
    Image.fromarray(synth.bev_tile_u8(int(g['tile_seed']), 1152)).save(tiles / '19012021_0001_extra.png')
    cfg, runner = load_config_and_runner(os.path.join(REPO_ROOT, 'configs', NAME + '.py'), '0')
    runner.load_ckpt(str(ckpt))
    out = tmp_path / 'out'
    res = runner.infer_lane_coordinate_endpoint_semantics(tiles=str(tiles), batch_size=1, work_dirs=str(out), write_lane_vertex=True)
    assert list(res) == ['19012021_00']
    lanes = res['19012021_00'][0]
    _same_polylines(lanes, g, 'runner polylines', prefix='')
    recs = json.load(open(out / '19012021_00.json'))
    assert recs == io_utils.lane_records(io_utils.pack_lane_vertices(lanes))
    want = io_utils.lane_records(io_utils.pack_lane_vertices(g['cls_offset_smooth']))
    assert len(recs) == len(want) > 0 and [r['seq_len'] for r in recs] == [r['seq_len'] for r in want]


def test_mixer_backbone_opcheck(dev, mnet):
    from lanemapping_amd import torch_ops
    bb = mnet.backbone
    w, n = torch_ops.stage_weights(bb), torch_ops.stage_name(bb)
    fea = ops.new_act(2, 64, 144, 144, dev)
    fea.copy_(torch.from_numpy(np.concatenate([cases.vit_input(32), cases.vit_input(33)])).to(dev))
    with torch.no_grad():
        torch.library.opcheck(torch.ops.lanemap_hip.mixer_backbone.default, (fea, w, n), test_utils=('test_schema', 'test_faketensor'))
        y = torch.ops.lanemap_hip.mixer_backbone(fea, w, n)
    assert tuple(y.shape) == (2, 8, 144, 144) and y.stride(1) == 1
