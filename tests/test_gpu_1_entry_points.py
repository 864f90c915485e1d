"""GPU tests (-m gpu) of the C-ABI entry points that the end-to-end goldens used to be the only check of, each against a plain fp64
restatement of the same operation (torch double on the CPU / numpy) and, for integer decisions, against the oracle functions pinned to
the reference goldens (oracle/decode_ref.py, oracle/rowref_ref.py).

Rules: floats within 1e-5 of the tensor scale (1e-4 only for the Winograd F(4x4) outputs, the tolerance of its existing tests: transform
constants up to 8); every integer / index / permutation output bit-exact; every kernel runs twice and must give identical bits.  Decision
inputs are built on a coarse value grid (multiples of 1/4) so that each decision is either an EXACT tie - where the documented rule
(strict comparisons, lowest index on ties) is asserted - or has a clear margin.  Argument refusals are host-side
LM_REQUIRE checks (RuntimeError before any launch); no case passes an index or size that a check lets through out of range."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import _close, _gn_ref, _lib, _quarter_grid

pytestmark = pytest.mark.gpu


def _rel_close(a, ref, tol, name, floor=1e-30):
    """Element-wise relative check |a - ref| <= tol * max(|ref|, floor) (rstd: one constant channel would otherwise set the scale of
    every other channel)."""
    a = a.detach().double().cpu() if torch.is_tensor(a) else torch.as_tensor(a, dtype=torch.float64)
    ref = ref.detach().double().cpu() if torch.is_tensor(ref) else torch.as_tensor(ref, dtype=torch.float64)
    assert a.shape == ref.shape, (name, a.shape, ref.shape)
    err = float(((a - ref).abs() / ref.abs().clamp_min(floor)).max())
    assert err <= tol, f'{name}: max relative err {err:.3e} > {tol:.0e}'


def _nhwc(t, dev):
    """Logical [B,C,H,W] tensor stored channels-last on the device."""
    return t.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _act64(y, act):
    from lanemapping_amd import ops
    if act == ops.ACT_RELU:
        return F.relu(y)
    if act == ops.ACT_GELU:
        return F.gelu(y)           # erf form, like the kernel's gelu_erf
    return y


# ================================================================================ 1. conv_mfma dispatch branches (csrc/conv_mfma.hip conv_dispatch)
@pytest.mark.parametrize('name,B,cin,cout,k,stride,hw,bn,res,act', [
    # 3x3 / stride 2, 128 -> 256 @290x286, B = 3: Ho x Wo = 145 x 143, M = 62 205 = 485 * 128 + 125 (ragged M tail);
    # K = 9 * 128 = 1152 > 256 (not tiny-K); big_blocks = ceil(M/128) * ceil(256/128) = 486 * 2 = 972 >= 700 -> launch<128,128,64,64>
    ('big_tile_stride2_m_tail', 3, 128, 256, 3, 2, (290, 286), True, True, 'relu'),
    # 3x3 / stride 1, 256 -> 200 @150x300, B = 1: M = 45 000, big_blocks = 352 * 2 = 704 >= 700 -> launch<128,128,64,64>; the second
    # 128-wide N tile holds 72 real channels (its upper wave column 192..255 is mostly beyond Cout: channel tail)
    ('big_tile_cout_tail', 1, 256, 200, 3, 1, (150, 300), False, True, 'none'),
    # 1x1 / stride 2 downsample, Cin = 320: K = 320 > 256 (not the tiny-K tile), M = 2 * 150 * 150 = 45 000, big_blocks = 352 * 2 = 704
    # -> launch<128,128,64,64>; BN scale and shift
    ('1x1_stride2_k320', 2, 320, 256, 1, 2, (300, 300), True, False, 'relu'),
])
def test_conv_mfma_big_tile_vs_fp64(dev, name, B, cin, cout, k, stride, hw, bn, res, act):
    """lm_conv2d_nhwc_mfma_f32 on the 128x128 tile (four 64x64 wave tiles) that most non-Winograd layers run on, against an fp64
    convolution with the same scale / shift / residual / activation: stride-2 tap addressing, a ragged M tail, a ragged Cout, and the
    non-tiny-K 1x1 path.  The parameter comments give the instantiation each case reaches."""
    from lanemapping_amd import ops
    g = torch.Generator().manual_seed(cin * 13 + cout + k * 7 + stride)
    x = torch.randn(B, cin, *hw, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    pad = k // 2
    ref = F.conv2d(x.double(), w.double(), None, stride, pad)
    scale = (torch.rand(cout, generator=g) + 0.5) if bn else None
    shift = torch.randn(cout, generator=g)
    if scale is not None:
        ref = ref * scale.double().view(1, -1, 1, 1)
    ref = ref + shift.double().view(1, -1, 1, 1)
    r = torch.randn(ref.shape, generator=g) if res else None
    if r is not None:
        ref = ref + r.double()
    a = {'none': ops.ACT_NONE, 'relu': ops.ACT_RELU}[act]
    ref = _act64(ref, a)
    xd, wp = _nhwc(x, dev), ops.pack_mfma(w.to(dev))
    sd = None if scale is None else scale.to(dev)
    rd = None if r is None else _nhwc(r, dev)
    run = lambda: ops.conv_mfma(xd, wp, cout, k, k, stride, pad, 1, scale=sd, shift=shift.to(dev), res=rd, act=a)
    y = run()
    _close(y, ref, 1e-5, name)
    assert torch.equal(y, run()), f'{name}: not deterministic'


def _gemm_ref(x, w, scale, shift, res, res_rows, act):
    y = x.double() @ w.double().t()
    if scale is not None:
        y = y * scale.double()
    if shift is not None:
        y = y + shift.double()
    if res is not None:
        M = y.shape[0]
        idx = torch.arange(M) % res_rows if res_rows else torch.arange(M)
        y = y + res.double()[idx]
    return _act64(y, act)


def test_linear_mfma_vit_fc1_gelu_big_tile(dev):
    """The ViT fc1 GEMM (M = 5184 tokens of 16 tiles, K = 1024, N = 3072) with bias + GELU(erf): big_blocks = ceil(5184/128) *
    ceil(3072/128) = 41 * 24 = 984 >= 700 -> launch<128,128,64,64> and its GELU epilogue (vector path), against fp64."""
    from lanemapping_amd import ops
    g = torch.Generator().manual_seed(3072)
    M, K, N = 5184, 1024, 3072
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    ref = _gemm_ref(x, w, None, b, None, 0, ops.ACT_GELU)
    xd, wp, bd = x.to(dev), ops.pack_mfma(w.to(dev)), b.to(dev)
    y = ops.linear_mfma(xd, wp, N, shift=bd, act=ops.ACT_GELU)
    _close(y, ref, 1e-5, 'fc1 + gelu')
    assert torch.equal(y, ops.linear_mfma(xd, wp, N, shift=bd, act=ops.ACT_GELU))


@pytest.mark.parametrize('M,K,N,res_rows', [
    (650, 512, 300, 26),      # big_blocks = 6 * 3 = 18 < 700 -> launch<64,64,32,32> (small-M tile); 650 = 25 * 26 rows
    (9000, 320, 1280, 324),   # big_blocks = 71 * 10 = 710 >= 700 -> launch<128,128,64,64>; 9000 = 27 * 324 + 252: the wrap ends mid-table
])
def test_linear_mfma_res_rows_broadcast(dev, M, K, N, res_rows):
    """`res_rows` > 0: output row m adds residual row m % res_rows (positional / lane embeddings: vitsegnet's pos_embedding, RowRef's
    emb_c), the div_rr fast-division path, on the small-M tile and on the big tile; with scale, shift and ReLU."""
    from lanemapping_amd import ops
    g = torch.Generator().manual_seed(M + res_rows)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    sc, sh = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    emb = torch.randn(res_rows, N, generator=g) * 2
    ref = _gemm_ref(x, w, sc, sh, emb, res_rows, ops.ACT_RELU)
    xd, wp = x.to(dev), ops.pack_mfma(w.to(dev))
    run = lambda: ops.linear_mfma(xd, wp, N, scale=sc.to(dev), shift=sh.to(dev), res=emb.to(dev), res_rows=res_rows, act=ops.ACT_RELU)
    y = run()
    _close(y, ref, 1e-5, f'res_rows={res_rows}')
    assert torch.equal(y, run())


@pytest.mark.parametrize('M,K,N,ldx,x_off,ldy,y_off', [
    (650, 512, 300, 800, 96, 700, 40),       # big_blocks = 6 * 3 = 18 -> launch<64,64,32,32>; ldx, ldy multiples of 4: vector epilogue
    (9000, 320, 1280, 416, 64, 1352, 36),    # big_blocks = 71 * 10 = 710 -> launch<128,128,64,64>
])
def test_linear_mfma_leading_dims(dev, M, K, N, ldx, x_off, ldy, y_off):
    """Input = a column slice of a wider row-major matrix (ldx > K: rowref.py feeds `hid[:, c*D:(c+1)*D]`) and output = a column
    slice of a wider matrix (`out=`, ldy > n_out): values against fp64, and every column outside the output slice keeps its bits."""
    from lanemapping_amd import ops
    g = torch.Generator().manual_seed(ldx + ldy)
    wide = torch.randn(M, ldx, generator=g)
    x = wide[:, x_off:x_off + K]
    w = torch.randn(N, K, generator=g) / K ** 0.5
    sh = torch.randn(N, generator=g)
    ref = _gemm_ref(x, w, None, sh, None, 0, ops.ACT_NONE)
    wd, wp, shd = wide.to(dev), ops.pack_mfma(w.to(dev)), sh.to(dev)
    outs = []
    for _ in range(2):
        out_wide = torch.full((M, ldy), 3.25, device=dev)
        ops.linear_mfma(wd[:, x_off:x_off + K], wp, N, shift=shd, out=out_wide[:, y_off:y_off + N])
        outs.append(out_wide)
    _close(outs[0][:, y_off:y_off + N], ref, 1e-5, 'leading dims')
    assert bool((outs[0][:, :y_off] == 3.25).all()) and bool((outs[0][:, y_off + N:] == 3.25).all()), 'columns outside the slice changed'
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('M,K,N,ldy,y_off,res,act', [
    (650, 512, 2, 2, 0, False, 'none'),        # ext head (n_out = 2): Cout <= 64 -> launch<128,64,32,64>; n + 3 >= Cout: scalar epilogue
    (650, 512, 37, 37, 0, True, 'relu'),       # Cout <= 64 tile; channel quads 0..32 vector, 36 scalar (Cout % 4 = 1)
    (650, 512, 37, 41, 3, True, 'none'),       # odd ldy = 41 (output slice at column 3 of a 41-wide matrix): every quad scalar
    (9000, 320, 1283, 1283, 0, True, 'gelu'),  # big_blocks = 71 * 11 = 781 -> launch<128,128,64,64>, odd ldy: scalar epilogue on the big tile
])
def test_linear_mfma_scalar_epilogue(dev, M, K, N, ldy, y_off, res, act):
    """The scalar (non-vector) epilogue of conv_mfma_kernel, taken when Cout % 4 != 0 or ldy % 4 != 0 (or ldr % 4 != 0): scale,
    shift, an odd-stride residual and the activation per element, against fp64; columns outside the output slice untouched."""
    from lanemapping_amd import ops
    a = {'none': ops.ACT_NONE, 'relu': ops.ACT_RELU, 'gelu': ops.ACT_GELU}[act]
    g = torch.Generator().manual_seed(N * 3 + ldy)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    sc, sh = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 2
    r = torch.randn(M, N, generator=g) if res else None      # ldr = N: odd for 37 and 1283
    ref = _gemm_ref(x, w, sc, sh, r, 0, a)
    xd, wp = x.to(dev), ops.pack_mfma(w.to(dev))
    outs = []
    for _ in range(2):
        out_wide = torch.full((M, ldy), -7.5, device=dev)
        ops.linear_mfma(xd, wp, N, scale=sc.to(dev), shift=sh.to(dev), res=None if r is None else r.to(dev), act=a,
                        out=out_wide[:, y_off:y_off + N])
        outs.append(out_wide)
    _close(outs[0][:, y_off:y_off + N], ref, 1e-5, f'scalar epilogue N={N} ldy={ldy}')
    if ldy > N:
        assert bool((outs[0][:, :y_off] == -7.5).all()) and bool((outs[0][:, y_off + N:] == -7.5).all())
    assert torch.equal(outs[0], outs[1])


def test_conv_mfma_refusals(dev):
    """conv_dispatch's host checks raise a clean RuntimeError (lm_last_error text) before any launch."""
    from lanemapping_amd import ops
    x = torch.zeros(1, 48, 8, 8, device=dev)
    with pytest.raises(RuntimeError, match='Cin=48 must be a multiple of 32'):
        ops.conv_mfma(x, ops.pack_mfma(torch.zeros(64, 48, 3, 3, device=dev)), 64, 3, 3, 1, 1)
    x = torch.zeros(1, 64, 8, 8, device=dev)
    with pytest.raises(RuntimeError, match='CoutP=64 must be Cout=64 rounded up to 128'):
        ops.conv_mfma(x, torch.zeros(9, 64, 64, device=dev), 64, 3, 3, 1, 1)
    from lanemapping_amd._lib import check
    a, wp, y = torch.zeros(64, 64, device=dev), torch.zeros(1, 128, 64, device=dev), torch.zeros(64, 40, device=dev)
    with pytest.raises(RuntimeError, match='bad leading dims'):     # ldy = 32 < Cout = 40
        check(_lib().lm_conv2d_nhwc_mfma_f32(ops._stream(), ops._ptr(a), 64, ops._ptr(wp), 128, None, None, None, 0, 0, ops._ptr(y), 32,
                                             1, 1, 64, 64, 40, 1, 1, 1, 0, 0, 1, ops.ACT_NONE))


# ================================================================================ 2. GroupNorm statistics
def _check_stats(st, y_ref, name):
    mean, rstd = _gn_ref(y_ref)
    _rel_close(st[..., 0], mean, 1e-5, name + ' mean', floor=1.0)
    _rel_close(st[..., 1], rstd, 1e-5, name + ' rstd')


@pytest.mark.parametrize('B,C,H,W', [(1, 32, 15, 20), (3, 64, 16, 32), (1, 128, 41, 25), (3, 256, 13, 21),
                                     (1, 256, 16, 32), (3, 32, 41, 25), (1, 64, 3, 1), (2, 128, 32, 48)])
def test_gn_stats_vs_fp64(dev, B, C, H, W):
    """ops.gn_stats (two-kernel reduction over 512-pixel chunks) against fp64: HW < 512 (300, 3), = 512, 512 k + 1 (1025) and
    a multiple (1536); C = 32 / 64 / 128 / 256 (8 / 4 / 2 / 1 pixel lanes per channel); B = 1 and 3.  Channel means of +-1e3 times
    the channel's standard deviation (where E[x^2] - mean^2 cancels in fp32) and one constant channel (var = 0 -> rstd =
    1/sqrt(eps)); rstd is held to 1e-5 RELATIVE per channel."""
    from lanemapping_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + C + H * W)
    std = torch.rand(B, C, 1, 1, generator=g) * 1.5 + 0.5
    sign = torch.where(torch.rand(B, C, 1, 1, generator=g) < 0.5, -1.0, 1.0)
    big = torch.rand(B, C, 1, 1, generator=g) < 0.5
    mean = torch.where(big, 1e3 * std * sign, torch.randn(B, C, 1, 1, generator=g))
    x = mean + std * torch.randn(B, C, H, W, generator=g)
    x[:, C // 2] = 0.3                                   # constant channel
    xd = _nhwc(x, dev)
    st = ops.gn_stats(xd, 1e-5)
    _check_stats(st, x, f'gn_stats B{B} C{C} HW{H * W}')
    assert torch.equal(st, ops.gn_stats(xd, 1e-5))
    assert float(st[0, C // 2, 1]) == pytest.approx(1 / math.sqrt(1e-5), rel=1e-6)


def test_gn_stats_refusal(dev):
    from lanemapping_amd import ops
    with pytest.raises(RuntimeError, match='must divide 256'):
        ops.gn_stats(_nhwc(torch.zeros(1, 96, 4, 4), dev))


@pytest.mark.parametrize('B,cin,cout,k,stride,hw', [
    (2, 64, 128, 3, 1, (24, 32)),    # Ho*Wo = 768 = 6 * 128; one 128-wide N tile
    (1, 128, 256, 3, 2, (64, 64)),   # stride 2: Ho*Wo = 1024; two N tiles
    (3, 96, 192, 1, 1, (16, 40)),    # 1x1, Ho*Wo = 640; Cout = 192: the second N tile is half empty
])
def test_conv_mfma_gnstats_vs_fp64(dev, B, cin, cout, k, stride, hw):
    """lm_conv2d_nhwc_mfma_f32_gnstats (the LANEMAP_WINO_F44=0 route of the FPN's GroupNorm'd convolutions): statistics mode always
    runs launch<128,128,64,64>, 64-row wave tiles -> per (image, 64-row chunk, channel) sum / sum of squares, then lm_gn_finalize.
    Output vs an fp64 convolution + shift, statistics vs fp64 statistics of that convolution."""
    from lanemapping_amd import ops
    g = torch.Generator().manual_seed(cin + cout + k)
    x = torch.randn(B, cin, *hw, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    sh = torch.randn(cout, generator=g)
    pad = k // 2
    ref = F.conv2d(x.double(), w.double(), None, stride, pad) + sh.double().view(1, -1, 1, 1)
    xd, wp, shd = _nhwc(x, dev), ops.pack_mfma(w.to(dev)), sh.to(dev)
    y, st = ops.conv_mfma_gnstats(xd, wp, cout, k, k, stride, pad, 1, shd)
    _close(y, ref, 1e-5, 'gnstats conv')
    _check_stats(st, ref, 'gnstats')
    y2, st2 = ops.conv_mfma_gnstats(xd, wp, cout, k, k, stride, pad, 1, shd)
    assert torch.equal(y, y2) and torch.equal(st, st2)


def test_conv_mfma_gnstats_refusals(dev):
    from lanemapping_amd import ops
    g = torch.Generator().manual_seed(1)
    x = _nhwc(torch.randn(1, 64, 16, 16, generator=g), dev)
    with pytest.raises(RuntimeError, match='needs Cout > 64'):      # Cout = 64
        ops.conv_mfma_gnstats(x, ops.pack_mfma(torch.zeros(64, 64, 3, 3, device=dev)), 64, 3, 3, 1, 1, 1, torch.zeros(64, device=dev))
    x = _nhwc(torch.randn(1, 64, 20, 20, generator=g), dev)           # Ho*Wo = 400: not whole 128-row tiles
    with pytest.raises(RuntimeError, match='needs Cout > 64'):
        ops.conv_mfma_gnstats(x, ops.pack_mfma(torch.zeros(128, 64, 3, 3, device=dev)), 128, 3, 3, 1, 1, 1, torch.zeros(128, device=dev))


@pytest.mark.parametrize('B,cin,cout,H,W,split', [(2, 128, 128, 60, 64, 1), (1, 64, 256, 72, 80, 2), (2, 32, 128, 37, 45, 2)])
def test_winograd44_gn_stats_vs_fp64(dev, B, cin, cout, H, W, split):
    """GroupNorm statistics from the Winograd F(4x4) epilogue (conv_wino44(gn_eps=)) against fp64 statistics of the convolution's own
    output (1e-5; the output itself vs an fp64 convolution at the F(4x4) tolerance 1e-4).  split = 2: lm_gn_finalize_split's
    [split][B][C/split][2] layout (the two semantic branches of one merged convolution): group s holds channels s*C/2 .. (s+1)*C/2-1."""
    from lanemapping_amd import ops
    assert ops.wino44_supported(H, W, cin, 1)
    g = torch.Generator().manual_seed(cin * cout + H + split)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sh = torch.randn(cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1) + sh.double().view(1, -1, 1, 1)
    xd, shd = _nhwc(x, dev), sh.to(dev)
    wf = ops.pack_wino44_fragments(ops.pack_wino44(w.to(dev)))
    y, st = ops.conv_wino44(xd, wf, cout, 1, shift=shd, gn_eps=1e-5, gn_split=split)
    _close(y, ref, 1e-4, 'winograd output')
    mean, rstd = _gn_ref(y)
    if split > 1:
        cg = cout // split
        assert st.shape == (split, B, cg, 2)
        mean = mean.view(B, split, cg).permute(1, 0, 2)
        rstd = rstd.view(B, split, cg).permute(1, 0, 2)
    _rel_close(st[..., 0], mean, 1e-5, 'winograd gn mean', floor=1.0)
    _rel_close(st[..., 1], rstd, 1e-5, 'winograd gn rstd')
    y2, st2 = ops.conv_wino44(xd, wf, cout, 1, shift=shd, gn_eps=1e-5, gn_split=split)
    assert torch.equal(y, y2) and torch.equal(st, st2)


# ================================================================================ 3. ViT / MixSeg / head glue
@pytest.mark.parametrize('D,rows', [(512, 1023), (1024, 258)])
def test_layernorm_vs_fp64(dev, D, rows):
    """lm_layernorm_rows (one wave per row; layernorm_kernel<8> for D = 512, <16> for D = 1024) against fp64: a row count that is not a
    multiple of the 4 rows of a workgroup, rows offset by +-100 times their standard deviation (a one-pass E[x^2] - mean^2 in fp32 would
    lose ~3 digits there), and rows holding one dyadic constant, whose output must be beta exactly (x - mean = 0)."""
    from lanemapping_amd import ops
    g = torch.Generator().manual_seed(D + rows)
    std = torch.rand(rows, 1, generator=g) * 1.5 + 0.5
    off = torch.randn(rows, 1, generator=g)
    far = torch.arange(rows).view(-1, 1) % 3 == 1
    off = torch.where(far, 100 * std * torch.sign(off), off)
    x = off + std * torch.randn(rows, D, generator=g)
    x[5] = 0.375
    x[rows - 1] = -12.5
    gamma, beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    ref = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(1, keepdim=True) + 1e-5) * gamma.double() + beta.double()
    xg, gg, bg = x.to(dev), gamma.to(dev), beta.to(dev)
    y = ops.layernorm(xg, gg, bg, 1e-5)
    _close(y, ref, 1e-5, f'layernorm D={D}')
    assert torch.equal(y[5].cpu(), beta) and torch.equal(y[rows - 1].cpu(), beta), 'a constant row must give beta exactly'
    assert torch.equal(y, ops.layernorm(xg, gg, bg, 1e-5))


def test_layernorm_refusal(dev):
    from lanemapping_amd import ops
    z = torch.zeros(4, 768, device=dev)
    with pytest.raises(RuntimeError, match='D=768 must be 512 or 1024'):
        ops.layernorm(z, torch.ones(768, device=dev), torch.zeros(768, device=dev))


@pytest.mark.parametrize('B,G,P,C', [(2, 18, 8, 8), (1, 18, 8, 16), (3, 5, 3, 7)])
def test_unpatchify_vs_permute(dev, B, G, P, C):
    """lm_unpatchify ('b (h w) (p1 p2 c) -> b c (h p1) (w p2)', vitsegnet.py:180) against reshape / permute, bit-exact: the config-2 /
    MixSeg grid (18 x 18 patches of 8 x 8, 8 channels), 16 channels, and an odd size (5 x 5 patches of 3 x 3, 7 channels)."""
    from lanemapping_amd import ops
    g = torch.Generator().manual_seed(G * P * C)
    tok = torch.randn(B, G * G, P * P * C, generator=g)
    ref = tok.view(B, G, G, P, P, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, G * P, G * P)
    td = tok.to(dev)
    y = ops.unpatchify(td, B, G, P, C)
    assert torch.equal(y.cpu(), ref)
    assert torch.equal(y, ops.unpatchify(td, B, G, P, C))


@pytest.mark.parametrize('B,P,L', [(2, 72, 23040), (3, 5, 1000)])
def test_head_proposal_conf_vs_fp64(dev, B, P, L):
    """lm_head_proposal_conf (Linear(L -> 2) per proposal, one workgroup per (b, p), 256-lane strided dot products + tree) against fp64:
    the config-2 size (P = 72 proposals of 144 x 160 = 23 040 features) and L = 1000 (not a multiple of 256)."""
    from lanemapping_amd import ops
    g = torch.Generator().manual_seed(L + P)
    tok = torch.randn(B * P, L, generator=g)
    wt = torch.randn(2, L, generator=g) / L ** 0.5
    bias = torch.randn(2, generator=g)
    ref = (tok.double() @ wt.double().t() + bias.double()).view(B, P, 2)
    td, wd, bd = tok.to(dev), wt.to(dev), bias.to(dev)
    conf = ops.head_proposal_conf(td, wd, bd, B, P)
    _close(conf, ref, 1e-5, 'proposal_conf')
    assert torch.equal(conf, ops.head_proposal_conf(td, wd, bd, B, P))


# ================================================================================ 4. decode (csrc/decode.hip)
def test_decode_orient_ties_inf_and_slices(dev):
    """lm_decode_orient = argmax over the orientation channels (:615) with ties to the LOWEST index: 11 channels on a
    quarter grid of few values (many exact ties), -inf entries and all--inf pixels (-> 0); once as a whole NHWC tensor, once as an
    11-channel slice of a 16-channel tensor (ldx = 16 > C).  Bit-exact against numpy's first-maximum argmax."""
    from lanemapping_amd import ops
    g = torch.Generator().manual_seed(11)
    B, C, H, W = 2, 11, 37, 45
    x = _quarter_grid(torch.randint(0, 3, (B, C, H, W), generator=g).float() * 0.5)
    x[torch.rand(B, C, H, W, generator=g) < 0.1] = float('-inf')
    x[0, :, 0, :5] = float('-inf')                        # every channel -inf
    x[1, :, 2, 3] = 1.0                                   # 11-way tie
    want = torch.from_numpy(np.argmax(x.numpy(), axis=1).astype(np.uint8))
    xd = _nhwc(x, dev)
    y = ops.decode_orient(xd)
    assert torch.equal(y.cpu(), want)
    assert torch.equal(y, ops.decode_orient(xd))
    assert int(y[0, 0, 0]) == 0 and int(y[1, 2, 3]) == 0
    wide = ops.new_act(B, 16, H, W, dev).fill_(5.0)       # the other channels of the wide tensor would win every argmax
    wide[:, 3:3 + C].copy_(xd)
    y2 = ops.decode_orient(wide[:, 3:3 + C])
    assert torch.equal(y2.cpu(), want)


def test_decode_orient_refusal(dev):
    z = torch.zeros(16, device=dev)
    from lanemapping_amd._lib import check
    from lanemapping_amd import ops
    with pytest.raises(RuntimeError, match='decode_orient: bad args'):
        check(_lib().lm_decode_orient(ops._stream(), ops._ptr(z), 4, 0, ops._ptr(torch.zeros(4, device=dev, dtype=torch.uint8)), 4))


def _oracle_column_decode(pconf, ext2, cls2, off2, sem_logits):
    """decode_ref.decode_column_proposals on the given tensors (orient / endpoint inputs: small dummies, their outputs unused; R = 6
    keeps the dummy endpoint map at 48 x 48, an 8 x 8 crop for the oracle's clustering loop)."""
    from oracle import decode_ref
    B, P, R, _ = cls2.shape
    return decode_ref.decode_column_proposals({'proposal_conf': pconf, 'ext2': ext2, 'cls2': cls2, 'offset2': off2,
                                               'orient': torch.zeros(B, 11, 8, 8), 'semantic_seg': sem_logits,
                                               'endp_est': torch.zeros(B, 1, 8 * R, 8 * R)})


def _semantic_logits(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = _quarter_grid(torch.randn(B, 3, H, W, generator=g) * 3)
    x[:, 2, 0::7] = x[:, 1, 0::7]                                        # exact ties l1 == l2 on every 7th row
    x[0, :, 1, 0:3] = torch.tensor([[-80., 80., -80.], [80., -80., 80.], [-80., 80., 80.]])   # saturated: classes 1, 2, tie
    x[0, :, 1, 3:6] = torch.tensor([[80., 80., -80.], [-80., 80., -80.], [-80., -80., 80.]])  # saturated: 0, 1 (l0 = l1: 0.5 each), 2
    x[1, :, 2, 0:4] = torch.tensor([[5., 5., 5., 0.], [5., 5., 5., 0.], [5., 5., 5., 0.]])    # 3-way ties: 1/3 each
    return x


def test_decode_semantic_softmax_ties_saturation(dev):
    """lm_decode_semantic, softmax mode (:627-632): sem = 1 iff s1 > s2 and s1 > thre, 2 iff s2 > s1 and s2 > thre (strict: a tie
    s1 == s2 gives 0); biseg = s1 + s2 against an fp64 softmax (1e-5); rows (the H/8 row gather) == biseg[:, 3::8] bit for bit.  Exact
    ties, 3-way ties and saturated +-80 logits (expf underflows to 0).  Classes equal the oracle's (decode_ref) on every pixel: the
    quarter grid leaves no near-tie, and the pixels the fp64 softmax calls exact ties are asserted to be 0."""
    from lanemapping_amd import ops
    B, H, W = 2, 48, 40
    x = _semantic_logits(B, H, W, 627)
    s = x.double().softmax(1)
    s1, s2 = s[:, 1], s[:, 2]
    tie = s1 == s2
    assert int(tie.sum()) > 50
    margin = torch.minimum((s1 - s2).abs(), torch.minimum((s1 - 0.2).abs(), (s2 - 0.2).abs()))
    clear = tie | (margin > 1e-6)
    assert int((~clear).sum()) <= 4, 'the quarter grid should leave (almost) no near-tie'
    want64 = torch.zeros(B, H, W, dtype=torch.uint8)
    want64[(s1 > s2) & (s1 > 0.2)] = 1
    want64[(s2 > s1) & (s2 > 0.2)] = 2
    oracle = _oracle_column_decode(torch.zeros(B, 1, 2), torch.zeros(B, 1, 6, 3), torch.zeros(B, 1, 6, 10), torch.zeros(B, 1, 6, 10), x)
    xd = x.to(dev)
    sem, biseg, rows = ops.decode_semantic(xd, 0.2)
    sem_c = sem.cpu()
    assert torch.equal(sem_c[clear], oracle['semantic_seg'].to(torch.uint8)[clear])
    assert torch.equal(sem_c[clear], want64[clear])
    assert bool((sem_c[tie] == 0).all()), 'a tie s1 == s2 must give class 0 (strict comparisons)'
    assert sem_c[0, 1, :6].tolist() == [1, 2, 0, 0, 1, 2]
    _close(biseg, s1 + s2, 1e-5, 'biseg')
    assert torch.equal(rows, biseg[:, 3::8])
    sem2, biseg2, rows2 = ops.decode_semantic(xd, 0.2)
    assert torch.equal(sem, sem2) and torch.equal(biseg, biseg2) and torch.equal(rows, rows2)


def test_decode_semantic_raw_mode_threshold(dev):
    """Raw mode (the segmentor, postprojector.py:122-127, quirk C11: thresholds on raw logits): a logit EQUAL to the threshold is not
    above it (class 0), ties l1 == l2 give 0; against decode_ref.segmentor_decode bit for bit; without the biseg / rows outputs."""
    from lanemapping_amd import ops
    from oracle import decode_ref
    B, H, W = 2, 48, 48
    x = _semantic_logits(B, H, W, 122) / 8
    thre = np.float32(0.1)
    x[:, 1, 5, :] = float(thre)                          # l1 == thre ...
    x[:, 2, 5, :] = -1.0                                 # ... above l2: still class 0
    x[:, 2, 6, :] = float(thre)
    x[:, 1, 6, :] = -1.0
    x[:, 1, 9, :] = float(thre) + 0.25
    x[:, 2, 9, :] = float(thre) + 0.25                   # tie above the threshold
    want = decode_ref.segmentor_decode(x, torch.zeros(B, 1, H, W))['seg'].to(torch.uint8)
    xd = x.to(dev)
    sem, biseg, rows = ops.decode_semantic(xd, float(thre), raw_mode=True, want_biseg=False)
    assert biseg is None and rows is None
    assert torch.equal(sem.cpu(), want)
    assert bool((sem[:, 5:7] == 0).all()) and bool((sem[:, 9] == 0).all())
    assert torch.equal(sem, ops.decode_semantic(xd, float(thre), raw_mode=True, want_biseg=False)[0])


def test_decode_semantic_refusal(dev):
    from lanemapping_amd import ops
    with pytest.raises(RuntimeError, match='H must be a multiple of 8'):
        ops.decode_semantic(torch.zeros(1, 3, 20, 16, device=dev), 0.2)


def test_decode_proposals_ties_clamp_every_proposal(dev):
    """lm_decode_proposals (:610, :694-702, :726-738) against decode_ref.decode_column_proposals: cls_idx and v_ext bit-exact,
    cls_offset (fp32 idx + offset kept in f64, clamped at 10, + prop_width * p - half_buff) bit-exact for every proposal p of
    config 2 (P = 72, prop_width 2, half_buff 4), probabilities against fp64 at 1e-6.  10-way and 2-way ties of the column bin (lowest
    index wins), 3-way existence ties (v = 0), and idx + off exactly on (10), above (10.5 -> 10) and below (9.75) the clamp."""
    from lanemapping_amd import ops
    g = torch.Generator().manual_seed(702)
    B, P, R = 2, 72, 6
    pconf = _quarter_grid(torch.randn(B, P, 2, generator=g) * 2)
    pconf[0, :4] = 0.75                                        # 2-way tie -> 0.5 / 0.5
    ext2 = _quarter_grid(torch.randn(B, P, R, 3, generator=g) * 2)
    ext2[:, :, 0] = 1.25                                       # 3-way ties: 1/3 each, e1 == e2 -> v = 0
    ext2[1, :, 1, 1:] = 2.0                                    # e1 == e2 > e0
    cls2 = _quarter_grid(torch.randn(B, P, R, 10, generator=g) * 2).clamp(-8, 8)
    cls2[:, :, 1] = -0.5                                       # 10-way tie -> idx 0
    cls2[:, 0::2, 2, 4] = 9.0
    cls2[:, 0::2, 2, 7] = 9.0                                  # 2-way tie between bins 4 and 7 -> 4
    cls2[:, :, 3:6, 9] = 20.0                                  # bin 9 wins: idx + off around the clamp
    off2 = _quarter_grid(torch.rand(B, P, R, 10, generator=g) * 3 - 1)
    off2[:, :, 3, 9] = 1.0                                     # 9 + 1.0 = 10 exactly (not above: kept)
    off2[:, :, 4, 9] = 1.5                                     # 10.5 -> 10
    off2[:, :, 5, 9] = 0.75                                    # 9.75
    ref = _oracle_column_decode(pconf, ext2, cls2, off2, torch.zeros(B, 3, 8, 8))
    dd = [t.to(dev) for t in (pconf, ext2, cls2, off2)]
    prop_conf, v_ext, cls_conf, cls_idx, cls_offset = ops.decode_proposals(*dd, 0.2, 2, 4)
    assert torch.equal(cls_idx.cpu(), ref['cls_idx'].to(torch.int32))
    assert bool((cls_idx[:, :, 1] == 0).all()) and bool((cls_idx[:, 0::2, 2] == 4).all())
    assert torch.equal(cls_offset.cpu(), ref['cls_offset'])
    co = cls_offset.cpu() - (2 * torch.arange(P, dtype=torch.float64) - 4).view(1, P, 1)
    assert bool((co[:, :, 3] == 10).all()) and bool((co[:, :, 4] == 10).all()) and bool((co[:, :, 5] == 9.75).all())
    e = ext2.double().softmax(3)
    d12 = e[..., 1] - e[..., 2]
    near = ((d12.abs() < 1e-6) & (d12 != 0)) | ((e[..., 1:] - 0.2).abs() < 1e-6).any(-1)
    assert int(near.sum()) == 0, 'the quarter grid should leave no near-tie of the existence decision'
    assert torch.equal(v_ext.cpu(), ref['prop_v_ext'].float())
    assert bool((v_ext[:, :, 0] == 0).all()) and bool((v_ext[1, :, 1] == 0).all())
    _close(prop_conf, pconf.double().softmax(2), 1e-6, 'prop_conf')
    _close(cls_conf, cls2.double().softmax(3), 1e-6, 'cls_conf')
    again = ops.decode_proposals(*dd, 0.2, 2, 4)
    for a, b in zip((prop_conf, v_ext, cls_conf, cls_idx, cls_offset), again):
        assert torch.equal(a, b)


# ================================================================================ 5. RowRef kernels (config 4, csrc/rowref.hip)
def _softmax_rows(x, rows, cols):
    from lanemapping_amd import ops
    from lanemapping_amd._lib import check
    check(_lib().lm_softmax_rows(ops._stream(), ops._ptr(x), rows, cols))


@pytest.mark.parametrize('cols', [1, 2, 63, 64, 65, 144])
def test_softmax_rows_vs_fp64(dev, cols):
    """lm_softmax_rows (in place, one wave per row, 64-lane strided columns): cols below, at and above one wave's width, the ext (2) and
    cls (144) rows of config 4; 1027 rows (not a multiple of the 4 rows of a workgroup); against fp64."""
    g = torch.Generator().manual_seed(cols)
    rows = 1027
    x = torch.randn(rows, cols, generator=g) * 4
    ref = x.double().softmax(1)
    a, b = x.to(dev), x.to(dev)
    _softmax_rows(a, rows, cols)
    _softmax_rows(b, rows, cols)
    _close(a, ref, 1e-5, f'softmax cols={cols}')
    assert torch.equal(a, b)


def test_softmax_rows_refusal(dev):
    with pytest.raises(RuntimeError, match='softmax_rows: bad args'):
        _softmax_rows(torch.zeros(4, device=dev), 4, 0)


def _select(ext, cls, thr, dev):
    from lanemapping_amd import ops
    from lanemapping_amd._lib import check
    B, H, L, W = cls.shape
    mean = torch.empty((B, L), device=dev)
    valid = torch.empty((B, L), device=dev, dtype=torch.int32)
    corr = torch.empty((B, L, H), device=dev, dtype=torch.int32)
    check(_lib().lm_rowref_select(ops._stream(), ops._ptr(ext), ops._ptr(cls), ops._ptr(mean), ops._ptr(valid), float(thr), ops._ptr(corr),
                                  B, H, W, L))
    return mean, valid, corr


@pytest.mark.parametrize('B,H,W,L', [(2, 144, 144, 12), (1, 300, 37, 3)])
def test_rowref_select_vs_fp64(dev, B, H, W, L):
    """lm_rowref_select (:199-204): the mean existence of each lane against fp64, the selection flag with lane means placed clearly
    above / below thr_ext = 0.3, and the per-row column argmax with ties to the lowest index (quarter-grid probabilities); H = 300 runs
    the 256-thread row loop twice."""
    g = torch.Generator().manual_seed(H + W)
    ext = torch.rand(B, H, L, 2, generator=g) * 0.2
    hi = torch.rand(B, 1, L, generator=g) < 0.5
    hi[..., 0], hi[..., 1] = True, False
    ext[..., 0] += torch.where(hi, 0.35, 0.05)                # lane means ~0.45 or ~0.15
    cls = _quarter_grid(torch.rand(B, H, L, W, generator=g) * 2)
    cls[:, 0] = 0.5                                           # a whole row tied -> column 0
    ed, cd = ext.to(dev), cls.to(dev)
    mean, valid, corr = _select(ed, cd, 0.3, dev)
    mref = ext[..., 0].double().mean(1)
    _close(mean, mref, 1e-5, 'lane mean')
    assert torch.equal(valid.cpu(), (mref > 0.3).int()) and int(valid.sum()) not in (0, B * L)
    want = torch.from_numpy(np.argmax(cls.numpy(), axis=3).astype(np.int32)).permute(0, 2, 1)
    assert torch.equal(corr.cpu(), want)
    m2, v2, c2 = _select(ed, cd, 0.3, dev)
    assert torch.equal(mean, m2) and torch.equal(valid, v2) and torch.equal(corr, c2)


def _gather(x, corr, B, H, W, L, dev):
    from lanemapping_amd import ops
    from lanemapping_amd._lib import check
    tok = torch.full((B * L, 8 * H * 5), 9.0, device=dev)
    check(_lib().lm_rowref_gather(ops._stream(), ops._ptr(x), ops._ptr(corr), ops._ptr(tok), B, H, W, L))
    return tok


def _corr_with_borders(B, L, H, W, g):
    corr = torch.randint(0, W, (B, L, H), generator=g, dtype=torch.int32)
    corr[:, 0, :] = torch.tensor([0, 1, W - 2, W - 1], dtype=torch.int32).repeat(H // 4 + 1)[:H]
    return corr


def test_rowref_gather_borders(dev):
    """lm_rowref_gather (:207-211): the 5-column window around each row's arg-max column, tokens in (c h w) order; windows that run off
    either border of the row (column 0, 1, W-2, W-1) are zero-filled.  Bit-exact against an fp64 zero-padded slice."""
    B, H, W, L = 2, 144, 144, 12
    g = torch.Generator().manual_seed(207)
    x = torch.randn(B, H, W, 8, generator=g)
    corr = _corr_with_borders(B, L, H, W, g)
    pad = F.pad(x.double(), (0, 0, 2, 2))                    # [B,H,W+4,8]
    idx = (corr.long().unsqueeze(-1) + torch.arange(5)).view(B, L, H, 5)                  # padded column of window entry j
    bb = torch.arange(B).view(B, 1, 1, 1)
    hh = torch.arange(H).view(1, 1, H, 1)
    win = pad[bb, hh, idx]                                    # [B,L,H,5,8]
    want = win.permute(0, 1, 4, 2, 3).reshape(B * L, 8 * H * 5).float()
    xd, cd = x.to(dev), corr.to(dev)
    tok = _gather(xd, cd, B, H, W, L, dev)
    assert torch.equal(tok.cpu(), want)
    assert torch.equal(tok, _gather(xd, cd, B, H, W, L, dev))
    assert float(tok.view(B * L, 8, H, 5)[0, :, 0, :2].abs().max()) == 0.0      # row 0 of lane 0: corr = 0, two columns off the left


def _scatter_ref(x, tok, corr, valid):
    """The reference's write-back loop (row_shared_not_reduc_ref.py:227-230, quirk C8): selected lanes in order, each on rows
    range(idx_h) where idx_h starts at H - 1 and becomes the last row written - the range shrinks by one per lane; later lanes win."""
    B, H, W, C = x.shape
    L = valid.shape[1]
    pad = np.pad(x.numpy(), ((0, 0), (0, 0), (2, 2), (0, 0)))
    t = tok.numpy().reshape(B * L, C, H, 5)
    for b in range(B):
        idx_h = H - 1
        for c in range(L):
            if not valid[b, c]:
                continue
            ci = corr[b, c].numpy()
            for h in range(idx_h):
                pad[b, h, ci[h]:ci[h] + 5, :] = t[b * L + c, :, h, :].T
                idx_h = h
    return torch.from_numpy(pad[:, :, 2:W + 2])


def _scatter(x, tok, corr, valid, dev):
    from lanemapping_amd import ops
    from lanemapping_amd._lib import check
    B, H, W, _ = x.shape
    L = valid.shape[1]
    y = torch.full_like(x, 9.0)
    check(_lib().lm_rowref_scatter(ops._stream(), ops._ptr(x), ops._ptr(tok), ops._ptr(corr), ops._ptr(valid), ops._ptr(y), B, H, W, L))
    return y


def test_rowref_scatter_shrinking_range(dev):
    """lm_rowref_scatter against a plain loop restating the reference's shrinking write-back range, bit-exact: tile 0 with
    every lane selected (lane n writes rows < H-1-n), tile 1 with none (y == x), tile 2 with a random subset; lanes with overlapping
    windows (the later lane wins) and windows over the borders."""
    B, H, W, L = 3, 144, 40, 12
    g = torch.Generator().manual_seed(227)
    x = torch.randn(B, H, W, 8, generator=g)
    tok = torch.randn(B * L, 8 * H * 5, generator=g)
    corr = torch.randint(10, 16, (B, L, H), generator=g, dtype=torch.int32)       # narrow band: windows overlap everywhere
    corr[:, 1] = _corr_with_borders(B, 1, H, W, g)[:, 0]
    valid = torch.zeros(B, L, dtype=torch.int32)
    valid[0] = 1
    valid[2] = (torch.rand(L, generator=g) < 0.5).int()
    valid[2, 3] = valid[2, 4] = 1
    want = _scatter_ref(x, tok, corr, valid)
    xd, td, cd, vd = x.to(dev), tok.to(dev), corr.to(dev), valid.to(dev)
    y = _scatter(xd, td, cd, vd, dev)
    assert torch.equal(y.cpu(), want)
    assert torch.equal(y[1].cpu(), x[1]), 'no lane selected: y must equal x'
    assert torch.equal(y, _scatter(xd, td, cd, vd, dev))


def _rowref_decode(ext2, cls2, dev, dense):
    from lanemapping_amd import ops
    from lanemapping_amd._lib import check
    B, H, L, W = cls2.shape
    conf = torch.full((B, H, W), 7, device=dev, dtype=torch.uint8) if dense else None
    cmap = torch.full((B, L + 1, H, W), 7, device=dev, dtype=torch.uint8) if dense else None
    col = torch.empty((B, L, H), device=dev, dtype=torch.int32)
    check(_lib().lm_rowref_decode(ops._stream(), ops._ptr(ext2), ops._ptr(cls2), ops._ptr(conf), ops._ptr(cmap), ops._ptr(col), B, H, W, L))
    return conf, cmap, col


def test_rowref_decode_ties_and_null_maps(dev):
    """lm_rowref_decode (:334-363): a row exists iff argmax(ext2) == 0 - an exact tie ext2[0] == ext2[1] counts as 0 (first maximum) -
    and its column is argmax(cls2) with ties to the lowest index.  conf / cls_map against rowref_ref.rowref_decode, col_idx
    against a numpy restatement (-1 = row absent), with the dense maps requested and passed as NULL (same col_idx)."""
    from oracle import rowref_ref
    B, H, W, L = 2, 144, 144, 12
    g = torch.Generator().manual_seed(334)
    ext2 = _quarter_grid(torch.rand(B, H, L, 2, generator=g))
    ext2[:, 0::5, :, 1] = ext2[:, 0::5, :, 0]                  # exact ties: the row exists
    cls2 = _quarter_grid(torch.rand(B, H, L, W, generator=g))  # ~9 distinct values over 144 columns: the maximum is nearly always tied
    out = {}
    for c in range(L):
        out[f'ext2_{c}'] = ext2[:, :, c, :]
        out[f'cls2_{c}'] = cls2[:, :, c, :]
    conf_ref, cls_ref = rowref_ref.rowref_decode(out, num_cls=L)
    en, cn = ext2.numpy(), cls2.numpy()
    col_ref = np.where(np.argmax(en, axis=3) == 0, np.argmax(cn, axis=3), -1).transpose(0, 2, 1).astype(np.int32)
    ed, cd = ext2.to(dev), cls2.to(dev)
    conf, cmap, col = _rowref_decode(ed, cd, dev, True)
    assert torch.equal(col.cpu(), torch.from_numpy(col_ref))
    assert torch.equal(conf.cpu(), torch.from_numpy(conf_ref).to(torch.uint8))
    assert torch.equal(cmap.cpu(), torch.from_numpy(cls_ref).to(torch.uint8))
    _, _, col2 = _rowref_decode(ed, cd, dev, False)
    assert torch.equal(col, col2)
    conf3, cmap3, _ = _rowref_decode(ed, cd, dev, True)
    assert torch.equal(conf, conf3) and torch.equal(cmap, cmap3)


# ================================================================================ 6. LiDAR tail (config 5)
@pytest.mark.parametrize('B,C,H,W,Ho,Wo', [(2, 64, 75, 75, 288, 288), (1, 8, 37, 50, 100, 61), (1, 4, 2, 3, 9, 7), (1, 4, 1, 1, 4, 5),
                                           (2, 12, 20, 21, 7, 9)])
def test_upsample_bicubic_vs_fp64(dev, B, C, H, W, Ho, Wo):
    """lm_upsample_bicubic_nhwc against F.interpolate(mode='bicubic', align_corners=False) in fp64: the config-5 75 -> 288, a non-square
    size, 2x3 -> 9x7 and 1x1 -> 4x5 (the source coordinate lies before the first pixel: border clamping two taps deep on both sides),
    and a down-sampling."""
    from lanemapping_amd import ops
    g = torch.Generator().manual_seed(H * W + Ho)
    x = torch.randn(B, C, H, W, generator=g)
    ref = F.interpolate(x.double(), size=(Ho, Wo), mode='bicubic', align_corners=False)
    xd = _nhwc(x, dev)
    y = ops.upsample_bicubic(xd, (Ho, Wo))
    _close(y, ref, 1e-5, f'bicubic {H}x{W}->{Ho}x{Wo}')
    assert torch.equal(y, ops.upsample_bicubic(xd, (Ho, Wo)))


def test_upsample_bicubic_refusal(dev):
    from lanemapping_amd import ops
    with pytest.raises(RuntimeError, match='upsample_bicubic: bad args'):
        ops.upsample_bicubic(_nhwc(torch.zeros(1, 6, 4, 4), dev), (8, 8))


@pytest.mark.parametrize('cin,cout,taps,M,res', [
    (16, 16, 27, 1037, False),    # Cin = 16: tap pairs, 27 taps -> 14 slabs, the last pair half empty; Cout <= 32 -> launch<128,32,32,32,true,2>
    (16, 64, 27, 2000, True),     # tap pairs, Cout <= 64 (every Cout > 32) -> launch<128,64,32,64,true,2>
    (16, 96, 9, 700, False),      # tap pairs with Cout > 64: two 64-wide N tiles of launch<128,64,32,64,true,2>
    (32, 32, 27, 1500, True),     # Cin % 32 == 0, Cout <= 32 -> launch<128,32,32,32,true>
    (64, 64, 27, 1299, False),    # Cout <= 64 -> launch<128,64,32,64,true>
    (64, 128, 27, 2053, True),    # Cout > 64 -> launch<128,128,64,64,true>
    (32, 200, 9, 900, True),      # Cout > 64, ragged: launch<128,128,64,64,true>, 200 of 256 columns
    (128, 128, 3, 900, True),     # conv_out of the network: the 3 taps of a (3,1,1) kernel, Cin = Cout = 128
])
def test_conv_gather_vs_fp64(dev, cin, cout, taps, M, res):
    """lm_conv_gather_mfma_f32 (the sparse convolutions of config 5) against the fp64 sum over taps of W[t]^T x[nbr[m][t]] with -1
    rulebook entries skipped, BatchNorm scale / shift, optional residual rows, ReLU; M ragged (not a multiple of 128 rows)."""
    from lanemapping_amd import ops
    g = torch.Generator().manual_seed(cin * 7 + cout + taps + M)
    V = 1200
    ldx = ops.sparse_ld(cin)
    x = torch.zeros(V, ldx)
    x[:, :cin] = torch.randn(V, cin, generator=g)
    nbr = torch.randint(0, V, (M, taps), generator=g, dtype=torch.int32)
    nbr[torch.rand(M, taps, generator=g) < 0.35] = -1
    nbr[:5] = -1                                                   # rows with no active input at all
    kdims = {27: (3, 3, 3), 9: (1, 3, 3), 3: (3, 1, 1)}[taps]
    w = torch.randn(*kdims, cin, cout, generator=g) / (taps * cin) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    ldy = ops.sparse_ld(cout)
    r = None
    xe = torch.cat([x[:, :cin].double(), torch.zeros(1, cin, dtype=torch.float64)])
    gath = xe[torch.where(nbr < 0, V, nbr).long()]                  # [M, taps, cin]
    ref = torch.einsum('mtc,tco->mo', gath, w.double().reshape(taps, cin, cout)) * sc.double() + sh.double()
    if res:
        r = torch.zeros(M, ldy)
        r[:, :cout] = torch.randn(M, cout, generator=g)
        ref = ref + r[:, :cout].double()
    ref = F.relu(ref)
    xd, nd, wp = x.to(dev), nbr.to(dev), ops.pack_sparse(w.to(dev))
    rd = None if r is None else r.to(dev)
    run = lambda: ops.conv_gather(xd, nd, wp, cin, cout, scale=sc.to(dev), shift=sh.to(dev), res=rd, act=ops.ACT_RELU)
    y = run()
    assert y.shape == (M, ldy)
    _close(y[:, :cout], ref, 1e-5, f'conv_gather {cin}->{cout} taps {taps}')
    if ldy > cout:
        assert float(y[:, cout:].abs().max()) == 0.0
    assert torch.equal(y, run())


def test_conv_gather_refusal(dev):
    from lanemapping_amd import ops
    from lanemapping_amd._lib import check
    x = torch.zeros(8, 48, device=dev)
    nbr = torch.zeros(4, 3, device=dev, dtype=torch.int32)
    wp = torch.zeros(3, 128, 48, device=dev)
    y = torch.zeros(4, 64, device=dev)
    with pytest.raises(RuntimeError, match='Cin=48 must be 16 or a multiple of 32'):
        check(_lib().lm_conv_gather_mfma_f32(ops._stream(), ops._ptr(x), 48, ops._ptr(nbr), 3, ops._ptr(wp), 128, None, None, None, 0,
                                             ops._ptr(y), 64, 4, 48, 64, ops.ACT_NONE))


@pytest.mark.parametrize('flip_h', [False, True])
def test_sparse_to_dense_vs_indexing(dev, flip_h):
    """lm_sparse_to_dense_nhwc = SparseConvTensor.dense().view(N, C*D, H, W) (+ torch.flip(dims=[2]), lidarencoder.py:70) against torch
    indexing, bit-exact: channel c of depth d lands in channel c*D + d; feature rows wider than C (ldf = 32 > C = 20); unset cells 0."""
    from lanemapping_amd import ops
    B, D, H, W, C = 2, 3, 75, 61, 20
    g = torch.Generator().manual_seed(70 + flip_h)
    cells = torch.randperm(B * D * H * W, generator=g)[:4000]
    b, r = cells // (D * H * W), cells % (D * H * W)
    z, r = r // (H * W), r % (H * W)
    yy, xx = r // W, r % W
    coords = torch.stack([b, z, yy, xx], 1).int()
    feats = torch.randn(4000, 32, generator=g)
    dense = torch.zeros(B, C, D, H, W)
    dense[b, :, z, yy, xx] = feats[:, :C]
    want = dense.view(B, C * D, H, W)
    if flip_h:
        want = torch.flip(want, dims=[2])
    fd, cd = feats.to(dev), coords.to(dev)
    y = ops.sparse_to_dense(fd, cd, B, (D, H, W), C, flip_h)
    assert torch.equal(y.cpu(), want)
    assert torch.equal(y, ops.sparse_to_dense(fd, cd, B, (D, H, W), C, flip_h))


def test_sparse_to_dense_refusal(dev):
    from lanemapping_amd import ops
    with pytest.raises(RuntimeError, match='sparse_to_dense: bad args'):
        ops.sparse_to_dense(torch.zeros(4, 16, device=dev), torch.zeros(4, 4, device=dev, dtype=torch.int32), 1, (1, 2, 2), 20, False)
