"""GPU tests (-m gpu) of ColumnProposal2 with heads.endp_mode = 'endpoint' (the head's own endpoint map, heads/polyline_fpn_vit_vertex_2.py
:254-260, :371-373, :650-653): lm_head_endpoint against fp64 under guarded buffers, then the head and the whole net against the
reference's goldens G28 (tests/golden/make_golden_endpoint.py), batch invariance, graph replay, the fusion as a memory bound, the Runner
entry, opcheck of the stage op, and the endp_est outputs of the same code unchanged (G25)."""
import json
import os

import numpy as np
import pytest
import torch

import cases
from gpu_common import _cached_net, _chk, _close, _close_sampled, _flips_inside_noise, _g, _lib, _nhwc_dev, _same_polylines
from guards import INF, Slab, batched, guarded_runs
from lanemapping_amd import ops, synth
from test_endpoint_mode_cpu import _layouts, build_endpoint, build_tag, endpoint_ref64

pytestmark = pytest.mark.gpu

TAGS = ('ep_c2', 'ep_att', 'ep_mixseg')
FRAME = (0, 1, 1150, 1151)


# ----------------------------------------------------------------------------------------------- the kernel
def _tile():
    return ops.head_endpoint_tile()


def _kernel_shapes():
    """(h, w, H, W): smaller than one tile, a non-integer ratio, a single row, H or W at T - 1, T, T + 1 and 2 T + 3 (T = the kernel's
    output tile edge, 32: read from the library when the test runs), and a down-sampling call (the low-resolution patch of a tile then
    does not fit the kernel's LDS patch and is read from global memory: the other path of the kernel)."""
    T = 32
    return [(3, 5, 12, 20), (7, 6, 25, 23), (1, 4, 1, 16),
            (9, 5, T - 1, T + 1), (5, 9, T, T - 1), (8, 8, T + 1, T), (11, 7, 2 * T + 3, T - 1), (6, 13, T, 2 * T + 3),
            (40, 37, 9, 11)]


def _endpoint_module(seed):
    """Conv2d(17, 4, 3) - ReLU - BatchNorm2d(4) - Conv2d(4, 1, 3) with weights of both signs and BatchNorm shifts of +-0.5 .. 1."""
    import torch.nn as nn
    g = _g(seed)
    ep = nn.Sequential(nn.Conv2d(17, 4, 3, 1, 1), nn.ReLU(), nn.BatchNorm2d(4), nn.Conv2d(4, 1, 3, 1, 1)).eval()
    with torch.no_grad():
        ep[0].weight.copy_(torch.randn(4, 17, 3, 3, generator=g) / 153 ** 0.5)
        ep[0].bias.copy_(torch.randn(4, generator=g) * 0.3)
        ep[2].weight.copy_((torch.rand(4, generator=g) + 0.5) * torch.tensor([1., -1., 1., -1.]))
        ep[2].bias.copy_((torch.rand(4, generator=g) * 0.5 + 0.5) * torch.tensor([-1., 1., 1., -1.]))
        ep[2].running_mean.copy_(torch.randn(4, generator=g) * 0.2)
        ep[2].running_var.copy_(torch.rand(4, generator=g) + 0.5)
        ep[3].weight.copy_(torch.randn(1, 4, 3, 3, generator=g) / 6)
        ep[3].bias.copy_(torch.randn(1, generator=g))
    return ep


@pytest.mark.parametrize('h,w,H,W', _kernel_shapes())
def test_head_endpoint_kernel_bounds(dev, h, w, H, W):
    """lm_head_endpoint vs fp64 F.interpolate + F.relu + F.conv2d on the CPU: col a slice (ldc = 20 at column 4), +Inf poison (the
    inputs go through a ReLU, which swallows NaN) in the guards, the ld padding and the neighbouring batch elements; canaries around the
    output; element 1 of a poisoned batch of 3 bit-identical to the batch-1 call.  Guards: 2 low-resolution rows + 256 pixels on col,
    2 rows + 256 floats on x_endp and the output.  Tolerance: the kernel-level 1e-5 of scale of lm_conv2d_nhwc_small (K = 288; here
    K = 153, then 36), on the 2-pixel frame (both zero paddings) and the interior separately."""
    assert _tile() == 32, 'the shapes of this test straddle a tile edge of 32'
    g = _g(1000 * h + 10 * w + H + W)
    col = torch.randn(1, 16, h, w, generator=g)
    x_endp = torch.randn(1, 1, H, W, generator=g) * 2
    ep = _endpoint_module(h + W)
    ref = endpoint_ref64(col, x_endp, ep)
    with torch.no_grad():
        packed = [t.to(dev) for t in ops.pack_head_endpoint(ep[0], ep[2], ep[3])]
    ldc, P = 20, h * w
    col_rows = col.permute(0, 2, 3, 1).reshape(-1, 16)

    def run(B, poisoned):
        pad = INF if poisoned else 0.0
        cs = Slab(dev, B * P, 16, ldc, 4, 256 + 2 * w, 256 + 2 * w).fill_input(batched(col_rows, B, INF), pad)
        xs = Slab(dev, B * H, W, None, 0, 2 + -(-256 // W), 2 + -(-256 // W)).fill_input(batched(x_endp.reshape(H, W), B, INF), pad)
        ys = Slab(dev, B * H, W, None, 0, 2 + -(-256 // W), 2 + -(-256 // W)).fill_canary()
        _chk(_lib().lm_head_endpoint(ops._stream(), cs.ptr(), ldc, xs.ptr(), *[t.data_ptr() for t in packed], ys.ptr(), B, h, w, H, W))
        return {'y': (ys, H)}
    y = guarded_runs(run, f'head_endpoint {h}x{w}->{H}x{W}')['y'].reshape(1, 1, H, W)
    scale = max(1.0, float(ref.abs().max()))
    err = (y.double() - ref).abs()[0, 0]
    frame = torch.zeros(H, W, dtype=torch.bool)
    frame[:2], frame[-2:], frame[:, :2], frame[:, -2:] = True, True, True, True
    print(f'head_endpoint {h}x{w}->{H}x{W}: max err frame {float(err[frame].max()):.3e}, '
          f'interior {float(err[~frame].max()) if bool((~frame).any()) else 0.0:.3e}, scale {scale:.3f}')
    for name, rows in (('top rows', err[:2]), ('bottom rows', err[-2:]), ('left columns', err[:, :2]), ('right columns', err[:, -2:])):
        assert float(rows.max()) <= 1e-5 * scale, f'{name}: max err {float(rows.max()):.3e} > 1e-5 * scale {scale:.3f}'
    _close(y, ref, 1e-5, 'endpoint')


def test_head_endpoint_matches_upsample_then_convs(dev):
    """The fused kernel against the unfused device route (ops.upsample_nhwc, then the same convolutions in fp64 on the CPU from the
    device's own up-sampled values): the interpolation inside the kernel is the bits of lm_upsample_bilinear_nhwc."""
    import torch.nn.functional as F
    g = _g(77)
    col = torch.randn(2, 16, 9, 11, generator=g)
    x_endp = torch.randn(2, 1, 35, 41, generator=g)
    ep = _endpoint_module(5)
    with torch.no_grad():
        packed = [t.to(dev) for t in ops.pack_head_endpoint(ep[0], ep[2], ep[3])]
        cd = _nhwc_dev(col, dev)
        y = ops.head_endpoint(cd, x_endp.to(dev), packed)
        u = torch.cat([ops.upsample_nhwc(cd, (35, 41)).cpu(), x_endp], dim=1).double()
        r = F.relu(F.conv2d(F.relu(u), ep[0].weight.double(), ep[0].bias.double(), padding=1))
        t = packed[2].cpu().double().view(1, 4, 1, 1) * r + packed[3].cpu().double().view(1, 4, 1, 1)
        ref = F.conv2d(t, ep[3].weight.double(), ep[3].bias.double(), padding=1)
    _close(y, ref, 1e-5, 'endpoint vs device up-sampling')


def test_head_endpoint_refusals(dev):
    z, y = torch.zeros(1024, device=dev), torch.zeros(64, device=dev)         # (the packed conv-1 weights are 612 floats)
    p = [z.data_ptr()] * 6
    args = lambda **k: (ops._stream(), k.get('col', z.data_ptr()), k.get('ldc', 16), z.data_ptr(), *p, k.get('out', y.data_ptr()),   # noqa: E731
                        1, 2, 2, k.get('H', 4), 4)
    _chk(_lib().lm_head_endpoint(*args()))
    with pytest.raises(RuntimeError, match='null pointer'):
        _chk(_lib().lm_head_endpoint(*args(col=None)))
    with pytest.raises(RuntimeError, match='null pointer'):
        _chk(_lib().lm_head_endpoint(*args(out=None)))
    with pytest.raises(RuntimeError, match='ldc=15'):
        _chk(_lib().lm_head_endpoint(*args(ldc=15)))
    with pytest.raises(RuntimeError, match='bad sizes'):
        _chk(_lib().lm_head_endpoint(*args(H=0)))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- goldens
def _net(dev, tag):
    """The tag's endpoint-mode net with the synthetic weights of seed 2021 on the GPU (tests restore whatever they change)."""
    return _cached_net(dev, (__name__, tag), lambda: build_tag(tag))


class _endp_est_mode:
    """The net's heads with cfg.heads.endp_mode = 'endp_est' for the duration of the block."""

    def __init__(self, net):
        self.h = net.heads

    def __enter__(self):
        self.h.cfg.heads['endp_mode'] = 'endp_est'
        assert not self.h.endpoint_mode()

    def __exit__(self, *exc):
        self.h.cfg.heads['endp_mode'] = 'endpoint'
        return False


@pytest.mark.parametrize('tag', TAGS)
def test_head_golden(dev, golden, tag):
    g = golden(f'g28_endpoint_{tag}.npz')
    net = _net(dev, tag)
    x, x_up = cases.head_inputs(int(g['input_seed']), batch=int(g['batch']))
    x_endp = synth.endp_logits(int(g['endp_seed']), int(g['batch']))
    with torch.no_grad():
        out = net.heads(torch.from_numpy(x).to(dev), torch.from_numpy(x_up).to(dev), torch.from_numpy(x_endp).to(dev))
    ep = out['endpoint']
    _close_sampled(ep, g, 'head_endpoint')
    scale = max(1.0, float(g['head_endpoint_absmax']))
    for name, mine, ref in (('frame rows', ep[:, 0, list(FRAME), :], g['head_endpoint_frame_rows']),
                            ('frame columns', ep[:, 0, :, list(FRAME)], g['head_endpoint_frame_cols'])):
        err = float(np.abs(mine.cpu().numpy() - ref).max())
        assert err <= 1e-4 * scale, f'{name}: max err {err:.3e} > 1e-4 * scale {scale:.3f}'
    _close(out['proposal_conf'], g['head_proposal_conf'], 1e-4, 'proposal_conf')
    for k in ('ext2', 'cls2', 'offset2', 'orient'):
        _close_sampled(out[k], g, f'head_{k}')
    for k, dim in (('cls2', -1), ('orient', 1)):
        _flips_inside_noise(out[k].argmax(dim).cpu().numpy(), g[f'head_{k}_argmax'], g[f'head_{k}_lowmargin'], k, 10 ** 9)


def _endp_sets(g):
    return {tuple(r) for r in g['e2e_endp_firm'].tolist()}, {tuple(r) for r in g['e2e_endp_any'].tolist()}


@pytest.mark.parametrize('tag', TAGS)
def test_end_to_end_golden(dev, golden, tag):
    """One full 1152^2 tile through Detector1stage in endpoint mode vs the reference's own end-to-end run: the endpoint map within 1e-4
    of scale, every endpoint the reference keeps under a 1e-4 perturbation of that map found and none outside what any such run
    gives; the rest by the G27 rules."""
    g = golden(f'g28_endpoint_{tag}.npz')
    net = _net(dev, tag)
    x = torch.from_numpy(synth.bev_batch([int(g['e2e_tile_seed'])], 1152)).to(dev)
    with torch.no_grad():
        raw = net.forward_raw({'proj': x})
        assert 'endpoint' in raw and tuple(raw['endpoint'].shape) == (1, 1, 1152, 1152)
        _close_sampled(raw['endpoint'], g, 'e2e_endpoint')
        _close(raw['proposal_conf'], g['e2e_proposal_conf'], 1e-4, 'proposal_conf')
        for k, gk in (('ext2', 'ext2'), ('cls2', 'cls2'), ('offset2', 'offset2'), ('orient', 'orient_logits')):
            _close_sampled(raw[k], g, f'e2e_{gk}')
        o = net({'proj': x})
    mine = {tuple(r) for r in np.stack(np.nonzero(o['endp'][0].numpy()), axis=1).tolist()}
    firm, anyset = _endp_sets(g)
    assert len(firm) >= 2 and firm <= mine, f'firm endpoints missing: {sorted(firm - mine)}'
    assert mine <= anyset, f'endpoints the reference never gives: {sorted(mine - anyset)}'
    _flips_inside_noise(o['prop_v_ext'].numpy().astype(np.uint8)[0], g['e2e_prop_v_ext'][0], g['e2e_ext_lowmargin'], 'prop_v_ext', 0)
    _flips_inside_noise(o['orient'].numpy().astype(np.uint8)[0], g['e2e_orient'][0], g['e2e_orient_lowmargin'], 'orient', 1)
    _flips_inside_noise(o['semantic_seg'].numpy().astype(np.uint8)[0], g['e2e_semantic_seg'][0], g['e2e_sem_lowmargin'], 'semantic_seg', 32)
    cls_idx = net.heads._compact['cls_idx'].cpu().numpy()[0]
    _flips_inside_noise(cls_idx, g['e2e_cls2_argmax'][0], g['e2e_cls2_lowmargin'], 'cls_idx', 4)
    _same_polylines(o['lane_maps']['cls_offset_smooth'][0], g, 'polylines')


def test_mode_is_live(dev, golden):
    """With endp_mode = 'endp_est' on the same weights nothing of the branch runs: no 'endpoint' key, and the decoded endpoints are the
    FPN's, not G28's."""
    g = golden('g28_endpoint_ep_c2.npz')
    net = _net(dev, 'ep_c2')
    x = torch.from_numpy(synth.bev_batch([int(g['e2e_tile_seed'])], 1152)).to(dev)
    with _endp_est_mode(net), torch.no_grad():
        raw = net.forward_raw({'proj': x})
        assert 'endpoint' not in raw
        o = net({'proj': x})
    mine = {tuple(r) for r in np.stack(np.nonzero(o['endp'][0].numpy()), axis=1).tolist()}
    firm, anyset = _endp_sets(g)
    assert not (firm <= mine) and not (mine <= anyset)


def test_default_mode_unchanged(dev, golden):
    """Config 2 at (36, 4) with endp_mode = 'endp_est' still reproduces G25's end-to-end entries, as test_gpu_head_geometry asserts
    them - in a process that has run the endpoint mode on the same net before."""
    g = golden('g25_propgeom_c2_p36.npz')
    net = build_endpoint('Proj_polyline_fpn_vit_vertex_2', dict(), endp_mode='endpoint')
    h = dict(net.cfg.heads)
    h.update(num_prop=36, prop_width=4)
    from lanemapping_amd.boundary import build_net_from_config
    net = build_net_from_config('Proj_polyline_fpn_vit_vertex_2', device='cpu', heads=h)
    synth.fill_module_(net, 2021)
    net = net.to(dev)
    x = torch.from_numpy(synth.bev_batch([int(g['e2e_tile_seed'])], 1152)).to(dev)
    with torch.no_grad():
        assert 'endpoint' in net.forward_raw({'proj': x})
    with _endp_est_mode(net), torch.no_grad():
        raw = net.forward_raw({'proj': x})
        assert 'endpoint' not in raw
        _close(raw['proposal_conf'], g['e2e_proposal_conf'], 1e-4, 'proposal_conf')
        for k, gk in (('ext2', 'ext2'), ('cls2', 'cls2'), ('offset2', 'offset2'), ('orient', 'orient_logits')):
            _close_sampled(raw[k], g, f'e2e_{gk}')
        o = net({'proj': x})
    _flips_inside_noise(o['prop_v_ext'].numpy().astype(np.uint8)[0], g['e2e_prop_v_ext'][0], g['e2e_ext_lowmargin'], 'prop_v_ext', 0)
    _flips_inside_noise(o['orient'].numpy().astype(np.uint8)[0], g['e2e_orient'][0], g['e2e_orient_lowmargin'], 'orient', 1)
    _flips_inside_noise(o['semantic_seg'].numpy().astype(np.uint8)[0], g['e2e_semantic_seg'][0], g['e2e_sem_lowmargin'], 'semantic_seg', 32)
    _flips_inside_noise(net.heads._compact['cls_idx'].cpu().numpy()[0], g['e2e_cls2_argmax'][0], g['e2e_cls2_lowmargin'], 'cls_idx', 4)
    off_scale = max(1.0, float(g['e2e_offset2_absmax']))
    np.testing.assert_allclose(o['cls_offset'].numpy(), g['e2e_cls_offset'], rtol=0, atol=1e-4 * off_scale)
    _close(o['prop_conf'], g['e2e_prop_conf'], 1e-4, 'prop_conf')
    assert np.array_equal(np.stack(np.nonzero(o['endp'][0].numpy()), axis=1), g['e2e_endp'])
    assert np.array_equal(np.stack(np.nonzero(o['lane_maps']['endp_by_cls'][0]), axis=1), g['e2e_endp_final'])
    _same_polylines(o['lane_maps']['cls_offset_smooth'][0], g, 'polylines')


# ----------------------------------------------------------------------------------------------- invariance, graphs, memory, Runner, opcheck
@pytest.mark.parametrize('tag', ['ep_c2', 'ep_mixseg'])
def test_tile_inside_batch3_bit_identical(dev, tag):
    net = _net(dev, tag)
    x = torch.from_numpy(synth.bev_batch([7400 + i for i in range(3)], 1152)).to(dev)
    with torch.no_grad():
        raw = {k: v.clone() for k, v in net.forward_raw({'proj': x}).items()}
        one = net.forward_raw({'proj': x[1:2].contiguous()})
    for k in ('endpoint', 'proposal_conf', 'ext2', 'cls2', 'offset2', 'orient'):
        assert torch.equal(raw[k][1:2], one[k]), f'{tag} tile 1 {k}: batch-3 result != single-tile result'


def test_pipeline_graph_replay_bit_identical(dev):
    """TilePipeline eager vs captured-graph replay in endpoint mode: the same lanes and endpoints (the decode reads the head's map)."""
    from lanemapping_amd.pipeline import TilePipeline
    net = _net(dev, 'ep_c2')
    eager, graph = TilePipeline(net, use_graph=False, with_decode_endp=True), TilePipeline(net, use_graph=True, with_decode_endp=True)
    for seeds in ([2021, 2022], [2030, 2031]):
        x = torch.from_numpy(synth.bev_batch(seeds, 1152)).to(dev)
        want, got = eager.run_batch(x), graph.run_batch(x)
        assert len(want) == len(got) == len(seeds)
        for a, b in zip(want, got):
            assert all(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(a, b))
    graph.clear_graphs()


def test_pipeline_decodes_the_heads_map(dev, golden):
    g = golden('g28_endpoint_ep_c2.npz')
    from lanemapping_amd.pipeline import TilePipeline
    net = _net(dev, 'ep_c2')
    x = torch.from_numpy(synth.bev_batch([int(g['e2e_tile_seed'])], 1152)).to(dev)
    lanes, kept, pts = TilePipeline(net, use_graph=False, with_decode_endp=True).run_batch(x)[0]
    mine = {tuple(r) for r in np.asarray(pts).tolist()}
    firm, anyset = _endp_sets(g)
    assert firm <= mine <= anyset


def test_fusion_peak_memory(dev):
    """The [B,17,H,W] concatenation is never built: over the head stage at B = 2 the endpoint mode's peak allocation exceeds the
    default mode's by at most the output map (B * H * W * 4 bytes) plus 1 MiB."""
    net = _net(dev, 'ep_c2')
    B = 2
    x, x_up = cases.head_inputs(41, batch=B)
    xd, xud = torch.from_numpy(x).to(dev), torch.from_numpy(x_up).to(dev)
    x_endp = torch.from_numpy(synth.endp_logits(43, B)).to(dev)

    def peak():
        with torch.no_grad():
            net.heads(xd, xud, x_endp)          # warm: packed weights, workspaces
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = net.heads(xd, xud, x_endp)
            torch.cuda.synchronize()
            p = torch.cuda.max_memory_allocated() - base
        del out
        return p
    on = peak()
    with _endp_est_mode(net):
        off = peak()
    print(f'head stage peak at B = {B}: endpoint mode {on / 2 ** 20:.1f} MiB, default {off / 2 ** 20:.1f} MiB')
    assert on - off <= B * 1152 * 1152 * 4 + 2 ** 20, f'endpoint mode adds {(on - off) / 2 ** 20:.1f} MiB to the head stage'


def test_runner_tiles_to_json(dev, golden, tmp_path, monkeypatch):
    """load_config_and_runner on config 2 with heads.endp_mode = 'endpoint', a strict reference checkpoint, a PNG tile -> per-tile JSON
    of the reference's polylines (G28 ep_c2)."""
    from PIL import Image
    from lanemapping_amd import io_utils
    from lanemapping_amd.boundary import REPO_ROOT
    from lanemapping_amd.runner import load_config_and_runner
    g = golden('g28_endpoint_ep_c2.npz')
    net = _net(dev, 'ep_c2')
    monkeypatch.chdir(tmp_path)
    cfg_path = tmp_path / 'Proj_polyline_fpn_vit_vertex_2_endpoint.py'
    base = open(os.path.join(REPO_ROOT, 'configs', 'Proj_polyline_fpn_vit_vertex_2.py')).read()
    cfg_path.write_text(base + "\nheads.update(endp_mode='endpoint')\n")
    ckpt = tmp_path / 'best.pth'
    torch.save({'net': {'module.' + k: v.cpu() for k, v in net.state_dict().items()}}, ckpt)
    tiles = tmp_path / 'tiles'
    tiles.mkdir()
    Image.fromarray(synth.bev_tile_u8(int(g['e2e_tile_seed']), 1152)).save(tiles / '19012021_0001_extra.png')
    cfg, runner = load_config_and_runner(str(cfg_path), '0')
    assert runner.net.heads.endpoint_mode()
    runner.load_ckpt(str(ckpt))
    out = tmp_path / 'out'
    res = runner.infer_lane_coordinate_endpoint_semantics(tiles=str(tiles), batch_size=1, work_dirs=str(out), write_lane_vertex=True)
    assert list(res) == ['19012021_00']
    _same_polylines(res['19012021_00'][0], g, 'runner polylines')
    recs = json.load(open(out / '19012021_00.json'))
    want = io_utils.lane_records(io_utils.pack_lane_vertices(g['e2e_cls_offset_smooth']))
    assert len(recs) == len(want) > 0 and [r['seq_len'] for r in recs] == [r['seq_len'] for r in want]


def test_colprop_endpoint_opcheck(dev):
    from lanemapping_amd import torch_ops
    h = _net(dev, 'ep_c2').heads
    g = _g(9)
    col = _nhwc_dev(torch.randn(1, 16, 288, 288, generator=g), dev)
    x_endp = torch.from_numpy(synth.endp_logits(43, 1)).to(dev)
    w, n = torch_ops.stage_weights(h), torch_ops.stage_name(h)
    with torch.no_grad():
        torch.library.opcheck(torch.ops.lanemap_hip.colprop_endpoint.default, (col, x_endp, w, n), test_utils=('test_schema', 'test_faketensor'))
        y = torch.ops.lanemap_hip.colprop_endpoint(col, x_endp, w, n)
    assert tuple(y.shape) == (1, 1, 1152, 1152)
