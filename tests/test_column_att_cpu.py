"""ColumnProposal2 with column_att=True (the proposal-attention branch), without a GPU: the net builds the reference's state-dict layout
for every tag of golden G27 (tests/golden/g27_colatt_layout.json, make_golden_colatt.py), reference checkpoints load strictly,
check_column_att accepts the supported matrix and refuses the rest with NotImplementedError naming the parameter, before any device
work, and the pack-time layouts (to_token as a (P x 1) convolution with zero-padded channels, line_expand rows in (h c) order, the
diagonal BatchNorm, the 16-wide blocks of pack_small for Cout > 16) reproduce the reference's arithmetic in fp64."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from lanemapping_amd import heads as heads_mod, ops, synth
from lanemapping_amd.boundary import build_net_from_config, load_config, load_reference_checkpoint

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CONFIG2 = 'Proj_polyline_fpn_vit_vertex_2'
TAGS = ('att_p72', 'att_p36', 'att_p18', 'att_t2')


def _layouts():
    with open(os.path.join(GOLDEN, 'g27_colatt_layout.json')) as f:
        return json.load(f)


def build_colatt(over, device='cpu', config=CONFIG2):
    """Config 2 with cfg.heads overridden and column_att = True, as make_golden_colatt.py builds the reference net."""
    h = dict(load_config(config).heads)
    h.update(over)
    return build_net_from_config(config, device=device, heads=h, column_att=True)


def test_golden_covers_every_tag():
    assert sorted(_layouts()) == sorted(TAGS)


@pytest.mark.parametrize('tag', TAGS)
def test_state_dict_layout_matches_reference(tag):
    ref = _layouts()[tag]
    assert ref['column_att'] is True
    net = build_colatt(ref['heads'])
    assert net.heads.cfg.column_att is True
    want = [(k, tuple(s)) for k, s in ref['state_dict']]
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert len(got) == len(want) and dict(got) == dict(want)
    h = net.heads
    sd = net.state_dict()
    assert tuple(sd['heads.to_token.1.weight'].shape) == (h.dim_token, 1152)
    assert tuple(sd['heads.line_expand.0.weight'].shape) == (1152, h.dim_token)


@pytest.mark.parametrize('tag', TAGS)
def test_reference_checkpoint_loads_strictly(tag, tmp_path):
    ref = _layouts()[tag]
    src = build_colatt(ref['heads'])
    synth.fill_module_(src, 2021)
    path = tmp_path / 'best.pth'
    torch.save({'net': {'module.' + k: v for k, v in src.state_dict().items()}, 'epoch': 1}, path)
    dst = build_colatt(ref['heads'])
    res = load_reference_checkpoint(dst, str(path), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v), k


@pytest.mark.parametrize('dim_token,heads,dim_head,mlp,depth', [
    (1024, 16, 64, 2048, 1), (512, 8, 64, 1024, 2), (32, 1, 64, 32, 1), (64, 2, 64, 64, 3), (4096, 4, 64, 4096, 1), (992, 3, 64, 96, 0),
])
def test_check_column_att_accepts(dim_token, heads, dim_head, mlp, depth):
    heads_mod.check_column_att(True, dim_token, heads, dim_head, mlp, depth)


@pytest.mark.parametrize('args,name', [
    ((True, 768, 16, 64, 2048, 1), 'dim_token=768'),
    ((True, 4128, 16, 64, 2048, 1), 'dim_token=4128'),
    ((True, 1000, 16, 64, 2048, 1), 'dim_token=1000'),
    ((True, 1024, 16, 32, 2048, 1), 'tr_dim_head=32'),
    ((True, 1024, 16, 64, 1000, 1), 'tr_mlp_dim=1000'),
    ((True, 64, 1, 64, 128, 1), 'tr_heads=1'),
    ((False, 1024, 16, 64, 2048, 1), 'spatial_att=False'),
])
def test_check_column_att_refuses_naming_the_parameter(args, name):
    with pytest.raises(NotImplementedError, match='column_att') as e:
        heads_mod.check_column_att(*args)
    assert name in str(e.value)


@pytest.mark.parametrize('over,name', [
    (dict(dim_token=768), 'dim_token=768'),
    (dict(dim_token=4128), 'dim_token=4128'),
    (dict(tr_dim_head=32), 'tr_dim_head=32'),
    (dict(tr_mlp_dim=1000), 'tr_mlp_dim=1000'),
])
def test_head_refuses_before_the_device(over, name):
    """The refusal comes from the head's own checks: nothing is packed or launched first (CPU tensors would be refused by the library
    with another exception)."""
    h = build_colatt(over).heads
    x, x_up = torch.zeros(1, 8, 144, 144), torch.zeros(1, 8, 288, 288)
    with pytest.raises(NotImplementedError, match=name):
        h._forward_impl(x, x_up)
    assert '_packed_cache' not in h.__dict__


def test_spatial_att_false_refused_before_the_device():
    h = build_net_from_config(CONFIG2, device='cpu', column_att=True, spatial_att=False).heads
    with pytest.raises(NotImplementedError, match='spatial_att=False'):
        h._forward_impl(torch.zeros(1, 8, 144, 144), torch.zeros(1, 8, 288, 288))


def test_column_transformer_decoder_still_refused():
    h = build_net_from_config(CONFIG2, device='cpu', column_transformer_decoder=True).heads
    with pytest.raises(NotImplementedError, match='column_transformer_decoder'):
        h._forward_impl(torch.zeros(1, 8, 144, 144), torch.zeros(1, 8, 288, 288))


@pytest.mark.parametrize('over', [dict(), dict(num_prop=36, prop_width=4), dict(num_prop=18, prop_width=8)])
def test_column_att_gets_past_the_head_checks(over):
    """column_att=True is accepted by the head: with CPU tensors the call then fails in the library (no device, or CPU tensors refused:
    never a fallback), not with NotImplementedError."""
    h = build_colatt(over).heads
    x, x_up = torch.zeros(1, 8, 144, 144), torch.zeros(1, 8, 288, 288)
    with pytest.raises(Exception) as e:
        h._forward_impl(x, x_up)
    assert not isinstance(e.value, NotImplementedError), e.value


def _packed(over, seed=2021):
    net = build_colatt(over)
    synth.fill_module_(net, seed)
    h = net.heads
    with torch.no_grad():
        return h, h._pack_column_att()


@pytest.mark.parametrize('over', [dict(), dict(num_prop=36, prop_width=4), dict(num_prop=18, prop_width=8), dict(dim_token=512)])
def test_to_token_as_convolution_matches_linear_fp64(over):
    """to_token + emb (:322-324) per (b, w) on feat_down[b, :, :, w] flattened (c h) == the (P x 1) convolution over feat_down with the
    packed weight (channels zero padded to >= 32; the padded input channels hold zeros, as the last stage's padded outputs do)."""
    h, P = _packed(over)
    Np, D = h.num_prop, h.dim_token
    lin = h.to_token[1]
    cd = lin.in_features // Np
    cdp = max(cd, 32)
    fd = torch.randn(2, cd, Np, Np, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    emb = torch.stack([getattr(h, f'emb_{i}') for i in range(Np)]).double()
    want = torch.stack([torch.stack([F.linear(fd[b, :, :, w].reshape(-1), lin.weight.double(), lin.bias.double()) + emb[w]
                                     for w in range(Np)]) for b in range(2)])               # [B, P, D]
    wp = P['ca.tok.w']
    assert tuple(wp.shape) == (Np, (D + 127) // 128 * 128, cdp)
    wconv = wp[:, :D, :].permute(1, 2, 0)[:, :, :, None].double()                           # [D, cdp, P(h), 1]
    fdp = torch.cat([fd, torch.zeros(2, cdp - cd, Np, Np, dtype=torch.float64)], dim=1)
    got = F.conv2d(fdp, wconv)[:, :, 0, :].permute(0, 2, 1) + P['ca.tok.b'].double() + P['ca.emb'].double()
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-10)


@pytest.mark.parametrize('over', [dict(), dict(dim_token=512)])
def test_line_expand_rows_in_hc_order_match_linear_fp64(over):
    """line_expand (:330-333, `b n (c h w) -> b n c h w`, c = 8, h = 144) with rows permuted to (h c): output column 8 h + c of the GEMM
    is the reference's element (c, h)."""
    h, P = _packed(over)
    D = h.dim_token
    ex = h.line_expand[0]
    t = torch.randn(5, D, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    want = F.linear(t, ex.weight.double(), ex.bias.double()).reshape(5, 8, 144)
    wp = P['ca.exp.w']
    assert tuple(wp.shape) == (1, 1152 + (-1152) % 128, D)
    got = (t @ wp[0, :1152].double().t() + P['ca.exp.b'].double()).reshape(5, 144, 8).permute(0, 2, 1)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-10)


@pytest.mark.parametrize('over', [dict(), dict(num_prop=36, prop_width=4), dict(num_prop=18, prop_width=8)])
def test_generate_line_proposal_packing_matches_module_fp64(over):
    """The packed stage weights (5x3 conv, diagonal BatchNorm 1x1, stride-2 convs with the last one zero padded to >= 32 outputs) run
    through fp64 F.conv2d reproduce generate_line_proposal (eval BatchNorm), the padded outputs being exact zeros."""
    h, P = _packed(over)
    layers = h.generate_line_proposal[0].layers
    x = torch.randn(1, 8, 144, 144, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    with torch.no_grad():
        want = x.clone()
        for layer in layers.double():                                                        # Conv_Pool_2d.forward (:62-65)
            want = layer(want)
    h.float()

    def unpack(wp, cout, cin, kh, kw):
        blocks = wp.reshape(-1, kh * kw, cin, 16)                                             # [Cout/16 or 1, taps, cin, 16]
        w = blocks.permute(0, 3, 2, 1).reshape(-1, cin, kh, kw)                                # [16 nb + j, cin, kh, kw]
        return w[:cout].double()

    f = F.relu(F.conv2d(x, unpack(P['ca.f0.w'], 8, 8, 5, 3), P['ca.f0.b'].double(), padding=(2, 1)))
    S = len(layers) - 1
    for i in range(S):
        c = f.shape[1]
        f = F.conv2d(f, unpack(P[f'ca.bn{i}.w'], c, c, 1, 1), P[f'ca.bn{i}.b'].double())
        cout = P[f'ca.s{i}.b'].numel()
        f = F.conv2d(f, unpack(P[f'ca.s{i}.w'], cout, c, 3, 3), P[f'ca.s{i}.b'].double(), stride=2, padding=1)
        if i < S - 1:
            f = F.relu(f)
    cd = want.shape[1]
    assert f.shape[1] == max(cd, 32) and f.shape[2:] == want.shape[2:] == (h.num_prop, h.num_prop)
    # (the packed BatchNorm scale / shift are fp32 roundings of the module's fp64 values)
    torch.testing.assert_close(f[:, :cd], want, rtol=1e-6, atol=1e-6 * max(1.0, float(want.abs().max())))
    assert bool((f[:, cd:] == 0).all())


@pytest.mark.parametrize('cout', [32, 48, 64])
def test_pack_small_wide_blocks(cout):
    w = torch.randn(cout, 12, 3, 3, generator=torch.Generator().manual_seed(cout))
    p = ops.pack_small(w)
    assert tuple(p.shape) == (cout // 16, 9, 12, 16) and p.is_contiguous()
    for nb in range(cout // 16):
        assert torch.equal(p[nb], ops.pack_small(w[16 * nb:16 * nb + 16]))
    with pytest.raises(AssertionError):
        ops.pack_small(torch.zeros(40, 4, 1, 1))
