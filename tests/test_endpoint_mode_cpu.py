"""ColumnProposal2 with heads.endp_mode = 'endpoint' (the head's own endpoint map, lm_head_endpoint), without a GPU: the packed operands
of the kernel reproduce the definition in fp64, the net builds the reference's state-dict layout for every tag of golden G28
(tests/golden/g28_endpoint_layout.json, make_golden_endpoint.py) and reference checkpoints load strictly, the stage op
torch.ops.lanemap_hip.colprop_endpoint is registered with a schema and a fake kernel, the mode switch picks the map the decode reads,
column_att with spatial_att=False is still refused, and the C entry is declared in the header."""
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

from lanemapping_amd import ops, synth
from lanemapping_amd.boundary import build_net_from_config, load_config, load_reference_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
TAGS = ('ep_c2', 'ep_att', 'ep_mixseg')


def _layouts():
    with open(os.path.join(GOLDEN, 'g28_endpoint_layout.json')) as f:
        return json.load(f)


def build_endpoint(config, over=None, device='cpu', endp_mode='endpoint'):
    """The config with cfg.heads.endp_mode overridden (and the top-level overrides `over`), as make_golden_endpoint.py builds the
    reference net."""
    h = dict(load_config(config).heads)
    h['endp_mode'] = endp_mode
    return build_net_from_config(config, device=device, heads=h, **(over or {}))


def build_tag(tag, device='cpu', endp_mode='endpoint'):
    ref = _layouts()[tag]
    return build_endpoint(ref['config'], ref['overrides'], device, endp_mode)


def endpoint_ref64(col, x_endp, ep, size=None):
    """The definition in fp64: conv2(bn(relu(conv1(relu(cat(up(col), x_endp)))))) with the module's own parameters (eval BatchNorm)."""
    H, W = x_endp.shape[2:]
    with torch.no_grad():
        return _endpoint_ref64(col, x_endp, ep, H, W)


def _endpoint_ref64(col, x_endp, ep, H, W):
    u = torch.cat([F.interpolate(col.double(), size=(H, W), mode='bilinear', align_corners=True), x_endp.double()], dim=1)
    conv1, bn, conv2 = ep[0], ep[2], ep[3]
    r = F.relu(F.conv2d(F.relu(u), conv1.weight.double(), conv1.bias.double(), padding=1))
    t = F.batch_norm(r, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(), False, 0.0, bn.eps)
    return F.conv2d(t, conv2.weight.double(), conv2.bias.double(), padding=1)


def test_golden_covers_every_tag():
    assert sorted(_layouts()) == sorted(TAGS)


def test_packing_matches_definition_fp64():
    """pack_head_endpoint's operands, applied as lm_head_endpoint documents them (w1p [17][3][3][4]; t = s * relu(.) + beta, ZERO
    outside the image; w2 [4][3][3]), against the module in fp64 - on the 1-pixel frame too, where a folded BatchNorm would differ."""
    net = build_endpoint('Proj_polyline_fpn_vit_vertex_2')
    synth.fill_module_(net, 2021)
    ep = net.heads.endpoint
    with torch.no_grad():
        w1p, b1, s, beta, w2, b2 = ops.pack_head_endpoint(ep[0], ep[2], ep[3])
        assert tuple(w1p.shape) == (17, 3, 3, 4) and tuple(w2.shape) == (4, 3, 3) and b2.numel() == 1
        assert all(t.is_contiguous() and t.dtype == torch.float32 for t in (w1p, b1, s, beta, w2, b2))
        assert float(beta.abs().min()) > 0, 'the seeded BatchNorm shift must be non-zero for this test to see a folded BN'
        g = torch.Generator().manual_seed(3)
        col = torch.randn(2, 16, 5, 6, generator=g)
        x_endp = torch.randn(2, 1, 17, 21, generator=g)
        want = endpoint_ref64(col, x_endp, ep)
        a = F.relu(torch.cat([F.interpolate(col.double(), size=(17, 21), mode='bilinear', align_corners=True), x_endp.double()], dim=1))
        r = F.relu(F.conv2d(a, w1p.permute(3, 0, 1, 2).double(), b1.double(), padding=1))
        t = s.double().view(1, 4, 1, 1) * r + beta.double().view(1, 4, 1, 1)
        got = F.conv2d(t, w2.double()[None], b2.double(), padding=1)
    # (s and beta are fp32 roundings of the module's fp64 values)
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6 * max(1.0, float(want.abs().max())))
    # folding beta into conv 2's bias is wrong exactly on the frame
    folded = F.conv2d(s.double().view(1, 4, 1, 1) * r, w2.double()[None], b2.double() + (w2.double().sum((1, 2)) * beta.double()).sum(),
                      padding=1)
    assert float((folded - want)[:, :, 1:-1, 1:-1].abs().max()) < 1e-6 and float((folded - want)[:, :, 0].abs().max()) > 1e-4


@pytest.mark.parametrize('tag', TAGS)
def test_state_dict_layout_matches_reference(tag):
    ref = _layouts()[tag]
    assert ref['endp_mode'] == 'endpoint'
    net = build_tag(tag)
    assert net.heads.endp_mode == 'endpoint' and net.heads.endpoint_mode()
    want = [(k, tuple(s)) for k, s in ref['state_dict']]
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert len(got) == len(want) and dict(got) == dict(want)
    sd = net.state_dict()
    assert tuple(sd['heads.endpoint.0.weight'].shape) == (4, 17, 3, 3) and tuple(sd['heads.endpoint.3.weight'].shape) == (1, 4, 3, 3)
    assert tuple(sd['heads.endpoint.2.running_var'].shape) == (4,)


@pytest.mark.parametrize('tag', TAGS)
def test_reference_checkpoint_loads_strictly(tag, tmp_path):
    src = build_tag(tag)
    synth.fill_module_(src, 2021)
    path = tmp_path / 'best.pth'
    torch.save({'net': {'module.' + k: v for k, v in src.state_dict().items()}, 'epoch': 1}, path)
    dst = build_tag(tag)
    res = load_reference_checkpoint(dst, str(path), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k in ('heads.endpoint.0.weight', 'heads.endpoint.2.bias', 'heads.endpoint.3.bias'):
        assert torch.equal(dst.state_dict()[k], src.state_dict()[k]), k


def test_colprop_endpoint_registered_with_schema_and_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from lanemapping_amd import torch_ops
    assert 'colprop_endpoint' in torch_ops.OP_NAMES
    sch = str(torch.ops.lanemap_hip.colprop_endpoint.default._schema)
    assert 'Tensor col' in sch and 'Tensor x_endp' in sch and 'Tensor[] weights' in sch and 'str stage' in sch and sch.endswith('-> Tensor'), sch
    # colprop_head keeps its schema: five outputs, col mutated
    head = str(torch.ops.lanemap_hip.colprop_head.default._schema)
    assert 'Tensor(a1!) col' in head and head.endswith('-> (Tensor, Tensor, Tensor, Tensor, Tensor)'), head
    h = build_endpoint('Proj_polyline_fpn_vit_vertex_2').heads
    w, n = torch_ops.stage_weights(h), torch_ops.stage_name(h)
    with FakeTensorMode(allow_non_fake_inputs=True):
        col = torch.empty((3, 288, 288, 16), device='cuda').permute(0, 3, 1, 2)
        x_endp = torch.empty((3, 1, 1152, 1152), device='cuda')
        y = torch.ops.lanemap_hip.colprop_endpoint(col, x_endp, w, n)
        assert tuple(y.shape) == (3, 1, 1152, 1152) and y.dtype == torch.float32 and y.is_contiguous()
    with pytest.raises((NotImplementedError, RuntimeError)):          # no CPU kernel: the dispatcher refuses
        torch.ops.lanemap_hip.colprop_endpoint(torch.zeros(1, 16, 2, 2), torch.zeros(1, 1, 4, 4), w, n)


def test_mode_switch_picks_the_decoded_map():
    on = build_endpoint('Proj_polyline_fpn_vit_vertex_2').heads
    off = build_endpoint('Proj_polyline_fpn_vit_vertex_2', endp_mode='endp_est').heads
    out = {'endpoint': torch.zeros(1), 'endp_est': torch.ones(1)}
    assert on.endpoint_mode() and on.endp_logits(out) is out['endpoint']
    assert not off.endpoint_mode() and off.endp_logits(out) is out['endp_est']
    assert not build_net_from_config('Proj_polyline_fpn_vit_vertex_2', device='cpu').heads.endpoint_mode()    # the shipped configs


def test_endpoint_mode_needs_x_endp_and_no_longer_refuses():
    """The mode is accepted: decode_compact no longer raises NotImplementedError("endp_mode='endpoint' ..."), and a forward without the
    FPN's endpoint logits is a ValueError naming x_endp - checked before any device work is attempted with it."""
    import inspect
    from lanemapping_amd import heads as heads_mod
    assert 'dead branch' not in inspect.getsource(heads_mod)
    h = build_endpoint('Proj_polyline_fpn_vit_vertex_2').heads
    h_forward = heads_mod.ColumnProposal2.forward
    from lanemapping_amd import torch_ops
    real = torch_ops.colprop_head
    torch_ops.colprop_head = lambda x, col, w, n: tuple(torch.zeros(1) for _ in range(5))      # (no device here)
    try:
        with pytest.raises(ValueError, match='x_endp'):
            h_forward(h, torch.zeros(1, 8, 144, 144), torch.zeros(1, 8, 288, 288), None, col=torch.zeros(1, 16, 288, 288))
    finally:
        torch_ops.colprop_head = real


def test_column_att_with_spatial_att_false_still_refused():
    h = build_endpoint('Proj_polyline_fpn_vit_vertex_2', dict(column_att=True, spatial_att=False)).heads
    with pytest.raises(NotImplementedError, match='spatial_att=False'):
        h._forward_impl(torch.zeros(1, 8, 144, 144), torch.zeros(1, 8, 288, 288))


def test_entry_declared_in_header_and_bound():
    from lanemapping_amd._lib import SIGNATURES
    text = open(os.path.join(ROOT, 'include', 'lanemap_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    m = re.search(r'\bint\s+lm_head_endpoint\s*\(([^)]*)\)', code)
    assert m, 'lm_head_endpoint is not declared in include/lanemap_hip.h'
    params = [p.strip() for p in m.group(1).split(',')]
    assert params[0] == 'void* hip_stream' and 'int ldc' in params and len(params) == len(SIGNATURES['lm_head_endpoint'][1]) == 16
    assert 'test_gpu_endpoint_mode.py::test_head_endpoint_kernel_bounds' in text        # where its guarded-buffer case lives
    assert re.search(r'\bint\s+lm_head_endpoint_tile\s*\(\s*void\s*\)', code) and 'lm_head_endpoint_tile' in SIGNATURES
