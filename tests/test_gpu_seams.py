"""GPU tests (-m gpu) of the seams between kernels: every place where a host-side `if` picks a kernel, and every launch whose dynamic
LDS is sized by a caller's argument, at the sizes on both sides of the seam.

A workgroup on gfx950 can be granted 163840 B (160 KB) of LDS, static and dynamic together.  The sites that size dynamic LDS
(every lm_ensure_dynamic_lds call), the argument that sizes it, the kernel's static bytes (.group_segment_fixed_size of the gfx950 code
object), the largest dynamic size the host admits, and the case that reaches it:

  site (csrc/)                            sized by                        static   largest dynamic   reached by
  conv_direct small_conv3x3_mfma<S>       stride (fixed: 33^2 x 16 x 4)        0     69696           test_small_conv_mfma_bit_identical_to_valu
  conv_direct small_conv3x3_mfma_wide     Cin <= 32, Cout <= 64, stride        0    143424           test_gpu_1_entry_points (stride 2, 32 -> 64)
  conv_mfma   conv_mfma_kernel<...>       tile shape (fixed)                   0     69632           every convolution test
  conv_mfma   lateral_mfma_kernel         Cin in {64, 128}                     0     69632           test_conv1x1_lateral_residuals
  conv_wino44 wino44_kernel               fixed                                0    155136           every Winograd test
  head        head_stage2_lds_kernel      D: 128 (D + 1) 4 <= 65536            0     64000 (D 124)   config 2 runs D = 64 (33280); wider D: VALU kernel
  norm_resize gn_relu_up_lds_kernel       source block x C <= 73728          384     73728           test_gn_relu_upsample_one_term_lds_block
  norm_resize gn_sum3_lds_kernel          source block x C <= 65536          384     65536           test_gn_sum_three_terms_lds_bit_identical
  vit         attention_mfma_kernel       fixed (352 keys x 68)                0     95744           N = 321 .. 352
  vit         attention_flash_kernel      fixed (64 keys x 140)                0     35840           N >= 381: test_attention_routes[381], [382]
  vit         attention_kernel            N: 404 N + 9792                    272    163312 (N 380)   test_attention_routes[380]
  raster      raster_partition_kernel     fixed                             3472     70864           every raster test
  raster      raster_band_kernel          rows x W x 4, rows in {16, 12}       0    163840           test_raster_width_seam[32-2560-16] (12 rows: 163824)
  ground      ground_min_kernel           cells x 4, cells <= 32768            0    131072           test_ground_cell_cap_reached (32761 cells: 131044)
  drape       drape_min_kernel            band starts x 4 + vertices x 8       0    147464           test_drape_vertex_and_height_caps_reached
  strip       strip_pass_kernel<*>        4 waves x T x 4, T <= 4096           0     65536           test_strip_tile_cap_reached

Two of these did not hold before this file: attention_kernel was routed by its dynamic bytes alone (N = 381: 163716 + 272 > 163840) and
the raster admitted bands of up to 65536 pixels (256 KB).  Both are now decided on the host from the totals above; no other site admits
more than 163840 B.

Floats are held to 1e-5 of the tensor scale against fp64 on the same fp32 inputs (_close); integer and byte outputs are bit-exact; every
call runs twice and must give the same bits."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import drape_ref as dr
import ground_ref as gr
from gpu_common import _chk, _close, _g, _lib, _quarter_grid, _s
from lanemapping_amd import ops
from lanemapping_amd._lib import LanemapHipError
from test_gpu_strip import _member
from test_gpu_vit_geometry import _attn64, _qkv

pytestmark = pytest.mark.gpu

f32 = np.float32
LDS_PER_WG = 160 * 1024


def _bits_equal(a, b, name):
    a, b = [t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (a, b)]
    a, b = np.ascontiguousarray(a, dtype=f32).view(np.uint32), np.ascontiguousarray(b, dtype=f32).view(np.uint32)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.array_equal(a, b), f'{name}: {int((a != b).sum())} of {a.size} words differ (first at {np.argwhere(a != b)[0].tolist()})'


# ================================================================================ 1. attention routes
def test_valu_attention_lds_arithmetic():
    """The numbers the routing rests on: the VALU kernel's LDS for N keys is 404 N + 9792 dynamic + 272 static bytes."""
    lds = lambda N: 4 * (65 * N + 36 * (N + 4) + 36 * 64) + 272
    assert lds(380) == 163584 <= LDS_PER_WG < lds(381) == 163988
    assert lds(64) == 35920


@pytest.mark.parametrize('N', [1, 2, 35, 36, 37, 72, 73, 353, 380, 381, 382])
@pytest.mark.parametrize('B,heads', [(1, 1), (2, 2)])
def test_attention_routes(dev, N, B, heads):
    """lm_attention_f32 on both sides of every seam of its dispatch: one key; one query chunk of the VALU kernel (36 rows) full, one row
    short and one row over, two chunks and one over; the first length past the MFMA kernel's 321 .. 352; 380, the last the VALU kernel's
    LDS holds (163312 + 272 B); 381, which passed the old host test and could not be launched, and 382: both on the flash kernel."""
    qkv = _qkv(B, N, heads, 31 * N + 7 * B + heads).to(dev).contiguous()
    got = ops.attention(qkv, B, N, heads, 64, 0.125)
    _close(got, _attn64(qkv.cpu(), B, N, heads, dev), 1e-5, f'attention N={N} B={B} heads={heads}')
    assert torch.equal(got, ops.attention(qkv, B, N, heads, 64, 0.125)), 'repeat run differs'
    for b in range(B if B > 1 else 0):
        one = ops.attention(qkv[b * N:(b + 1) * N].contiguous(), 1, N, heads, 64, 0.125)
        assert torch.equal(one, got[b * N:(b + 1) * N]), f'batch element {b} of {B} != the B = 1 call'


# ================================================================================ 2. masked attention at its cap
@pytest.mark.parametrize('N', [63, 64])
def test_attention_masked_at_the_token_cap(dev, N):
    """lm_attention_masked_f32 at N = 63 and 64 (the ballot compaction's last lane): all tokens, only the last, only the first, every
    other one.  Bitwise the plain call on the gathered rows, as test_attention_masked_vs_plain_on_compacted_tokens checks at N = 12, 7."""
    B, heads = 2, 2
    qkv = torch.randn((B * N, 3 * heads * 64), generator=_g(640 + N)).to(dev)
    masks = {'all': torch.ones(N), 'last': F.one_hot(torch.tensor(N - 1), N), 'first': F.one_hot(torch.tensor(0), N),
             'alternating': torch.arange(N) % 2}
    for name, m in masks.items():
        valid = torch.stack([m, m.flip(0) if name == 'alternating' else m]).to(torch.int32)
        vd = valid.to(dev).contiguous()
        out = ops.attention(qkv, B, N, heads, 64, 0.125, valid=vd)
        assert torch.equal(out, ops.attention(qkv, B, N, heads, 64, 0.125, valid=vd)), f'{name}: repeat run differs'
        for b in range(B):
            idx = torch.nonzero(valid[b]).flatten().to(dev)
            rows = qkv[b * N:(b + 1) * N][idx].contiguous()
            want = ops.attention(rows, 1, int(idx.numel()), heads, 64, 0.125)
            assert torch.equal(out[b * N:(b + 1) * N][idx], want), (name, b)
            if idx.numel() == 1:                                    # one key: every query row is that key's value row
                v = qkv[b * N + int(idx[0]), 2 * heads * 64:]
                assert torch.equal(out[b * N:(b + 1) * N], v.expand(N, -1)), (name, b)
        if name == 'all':
            assert torch.equal(out, ops.attention(qkv, B, N, heads, 64, 0.125))


def test_attention_masked_refuses_65_tokens(dev):
    qkv = torch.zeros((65, 3 * 64), device=dev)
    with pytest.raises(RuntimeError, match='N=65 at most 64'):
        ops.attention(qkv, 1, 65, 1, 64, 0.125, valid=torch.ones((1, 65), dtype=torch.int32, device=dev))


# ================================================================================ 3. the max-subtraction of every softmax
def _grid_qkv(B, N, heads, seed):
    """q and k on the half-integer grid in [-6, 6] (every product a multiple of 1/4 below 36, every 64-term dot product below 2304: exact
    in fp32 in any summation order, and so is the scale 1/8); the keys 0, N // 2 and N - 1 of every batch element are copies of the
    queries N - 1, 0 and N // 2, so q.k / 8 = |q|^2 / 8 is about 64 * 13 / 8 = 104 there.  v is random."""
    g = _g(seed)
    inner = heads * 64
    qkv = torch.randn((B * N, 3 * inner), generator=g)
    qkv[:, :2 * inner] = torch.randint(-12, 13, (B * N, 2 * inner), generator=g).float() * 0.5
    for b in range(B):
        for key, query in ((0, N - 1), (N // 2, 0), (N - 1, N // 2)):
            qkv[b * N + key, inner:2 * inner] = qkv[b * N + query, :inner]
    return qkv


@pytest.mark.parametrize('N', [37, 324, 382])
def test_attention_needs_its_max_subtraction(dev, N):
    """One N per kernel (VALU 37, MFMA 324, flash 382) with scores above 89: expf of a raw score is +inf in fp32, so a softmax that lost its
    `- m` (in the flash kernel: in the probabilities or in the rescale exp(m_old - m_new)) gives inf / inf = NaN.  The inputs lie on a grid
    on which the scores are exact in fp32, so the ordinary 1e-5 holds; both preconditions are asserted here on the CPU."""
    B, heads = 2, 2
    qkv = _grid_qkv(B, N, heads, 89 + N)
    q, k = [z.reshape(B, N, heads, 64).transpose(1, 2) for z in qkv.chunk(3, dim=-1)[:2]]
    s64 = q.double() @ k.double().transpose(-1, -2) * 0.125
    s32 = (q @ k.transpose(-1, -2)) * np.float32(0.125)
    assert float(s64.max()) > 89 and bool(torch.isinf(torch.exp(s64.max().float()))), 'some raw score overflows expf'
    assert torch.equal(s64, s64.float().double()) and torch.equal(s32.double(), s64), 'the scores are exact in fp32'
    if N == 382:                                                    # the running max rises after the first 32-key block in most rows
        assert float((s64[..., 32:].amax(-1) > s64[..., :32].amax(-1)).double().mean()) > 0.5
    qd = qkv.to(dev).contiguous()
    got = ops.attention(qd, B, N, heads, 64, 0.125)
    assert bool(torch.isfinite(got).all())
    _close(got, _attn64(qkv, B, N, heads, dev), 1e-5, f'attention N={N}, scores up to {float(s64.max()):.1f}')
    assert torch.equal(got, ops.attention(qd, B, N, heads, 64, 0.125))


def _softmax_rows(x):
    _chk(_lib().lm_softmax_rows(_s(), ops._ptr(x), x.shape[0], x.shape[1]))


@pytest.mark.parametrize('cols', [2, 65, 144])
def test_softmax_rows_needs_its_max_subtraction(dev, cols):
    """lm_softmax_rows on rows shifted by +1e4 and -1e4 (quarter grid: exact in fp32 at that magnitude) and on rows that span 200
    (-100 .. 100): without `- m` the first and third kind overflow expf, the second underflows every term to 0."""
    rows = 130
    g = _g(cols)
    x = _quarter_grid(torch.randn(rows, cols, generator=g) * 2)
    kind = torch.arange(rows) % 3
    x[kind == 0] += 1e4
    x[kind == 1] -= 1e4
    x[kind == 2] = _quarter_grid(torch.rand(int((kind == 2).sum()), cols, generator=g) * 200 - 100)
    x[kind == 2, 0], x[kind == 2, cols - 1] = -100.0, 100.0       # every such row spans exactly 200
    assert torch.equal(x.double(), _quarter_grid(x.double())), 'the shifted rows are still on the quarter grid'
    raw = torch.exp(x)
    assert bool(torch.isinf(raw[kind == 0]).all()) and float(raw[kind == 1].sum()) == 0.0 and bool(torch.isinf(raw[kind == 2].amax(1)).all())
    ref = x.double().softmax(1)
    a, b = x.to(dev), x.to(dev)
    _softmax_rows(a)
    _softmax_rows(b)
    assert bool(torch.isfinite(a).all())
    _close(a, ref, 1e-5, f'softmax cols={cols}')
    assert torch.equal(a, b)


def _saturated(shape, seed):
    """Quarter-grid logits around +100, around -100 and around 0 in equal parts along the first axis: expf of the first kind is +inf in
    fp32, of the second a denormal of a few bits (or 0)."""
    g = _g(seed)
    x = _quarter_grid(torch.randn(shape, generator=g) * 1.5)
    n = shape[0]
    shift = torch.tensor([100.0, -100.0, 0.0])[torch.arange(n) % 3].view(n, *([1] * (len(shape) - 1)))
    x = x + shift
    raw = torch.exp(x)
    assert bool(torch.isinf(raw[0::3]).all()) and float(raw[1::3].max()) < 2.0 ** -126
    return x


def test_decode_proposals_needs_its_max_subtraction(dev):
    """The 2-, 3- and FW-way softmaxes of lm_decode_proposals on logits around +-100: classes and bins equal the oracle's wherever the
    fp64 softmax leaves a margin (the quarter grid leaves nothing closer), probabilities against fp64."""
    from test_gpu_1_entry_points import _oracle_column_decode
    P, B, R = 6, 3, 6                                               # the saturation kind runs along the first axis: P
    pconf = _saturated((P, B, 2), 1).transpose(0, 1).contiguous()
    ext2 = _saturated((P, B, R, 3), 2).transpose(0, 1).contiguous()
    cls2 = _saturated((P, B, R, 10), 3).transpose(0, 1).contiguous()
    ext2[:, :, 0, 1:] = ext2[:, :, 0, :1]                           # 3-way ties at +100, -100 and 0: v = 0
    off2 = _quarter_grid(torch.rand(B, P, R, 10, generator=_g(4)) - 0.5)
    ref = _oracle_column_decode(pconf, ext2, cls2, off2, torch.zeros(B, 3, 8, 8))
    e = ext2.double().softmax(3)
    d12 = e[..., 1] - e[..., 2]
    near = ((d12.abs() < 1e-6) & (d12 != 0)) | ((e[..., 1:] - 0.2).abs() < 1e-6).any(-1)
    assert int(near.sum()) == 0, 'the quarter grid leaves no near-tie of the existence decision'
    c = cls2.double().softmax(3).sort(3).values
    assert float((c[..., -1] - c[..., -2]).abs()[c[..., -1] != c[..., -2]].min()) > 1e-6
    dd = [t.to(dev) for t in (pconf, ext2, cls2, off2)]
    prop_conf, v_ext, cls_conf, cls_idx, cls_offset = ops.decode_proposals(*dd, 0.2, 2, 4)
    assert torch.equal(cls_idx.cpu(), ref['cls_idx'].to(torch.int32))
    assert torch.equal(v_ext.cpu(), ref['prop_v_ext'].float()) and bool((v_ext[:, :, 0] == 0).all())
    assert len(torch.unique(v_ext)) == 3
    assert torch.equal(cls_offset.cpu(), ref['cls_offset'])
    _close(prop_conf, pconf.double().softmax(2), 1e-5, 'prop_conf')
    _close(cls_conf, cls2.double().softmax(3), 1e-5, 'cls_conf')
    for a, b in zip((prop_conf, v_ext, cls_conf, cls_idx, cls_offset), ops.decode_proposals(*dd, 0.2, 2, 4)):
        assert torch.equal(a, b)


def test_decode_semantic_needs_its_max_subtraction(dev):
    """The 3-way softmax of lm_decode_semantic on logits around +-100 (the existing tie test saturates single pixels at +-80, where
    expf(80) is still finite)."""
    from test_gpu_1_entry_points import _oracle_column_decode
    B, H, W = 2, 48, 40
    x = _saturated((H, B, 3, W), 5).permute(1, 2, 0, 3).contiguous()          # the kind runs along the image rows
    x[:, 2, :, 0::5] = x[:, 1, :, 0::5]                                        # exact ties l1 == l2 at every magnitude
    s = x.double().softmax(1)
    s1, s2 = s[:, 1], s[:, 2]
    tie = s1 == s2
    margin = torch.minimum((s1 - s2).abs(), torch.minimum((s1 - 0.2).abs(), (s2 - 0.2).abs()))
    clear = tie | (margin > 1e-6)
    assert int(tie.sum()) >= B * H * W // 5 and int((~clear).sum()) <= 4
    oracle = _oracle_column_decode(torch.zeros(B, 1, 2), torch.zeros(B, 1, 6, 3), torch.zeros(B, 1, 6, 10), torch.zeros(B, 1, 6, 10), x)
    xd = x.to(dev)
    sem, biseg, rows = ops.decode_semantic(xd, 0.2)
    sem_c = sem.cpu()
    assert torch.equal(sem_c[clear], oracle['semantic_seg'].to(torch.uint8)[clear])
    assert bool((sem_c[tie] == 0).all()) and len(torch.unique(sem_c)) == 3
    assert bool(torch.isfinite(biseg).all())
    _close(biseg, s1 + s2, 1e-5, 'biseg')
    assert torch.equal(rows, biseg[:, 3::8])
    sem2, biseg2, rows2 = ops.decode_semantic(xd, 0.2)
    assert torch.equal(sem, sem2) and torch.equal(biseg, biseg2) and torch.equal(rows, rows2)


# ================================================================================ 4. LayerNorm widths
@pytest.mark.parametrize('D', [64, 160, 192, 256, 544, 736, 800, 992, 1056, 2080, 4064])
def test_layernorm_every_instantiation_vs_fp64(dev, D):
    """lm_layernorm_rows at a width inside every instantiation of layernorm_masked_kernel<PER> (columns per lane: 1 at D = 64; 4 at 160,
    192, 256 and 16 at 544 .. 992, which no other test runs; 32 at 1056, 2080; 64 at 4064), at its upper edge (64, 256) and with a partly
    masked last lane slot (every D that is no multiple of 64).  The input recipe of test_layernorm_vs_fp64; the output buffer starts as NaN,
    so a dispatcher that picked a narrower instantiation leaves columns unwritten and fails.

    A constant row gives beta exactly at EVERY width of this list: the row's constant c is dyadic (0.375, -12.5), so each lane's sum of
    up to 64 copies (masked columns add 0), the butterfly over the lanes and the total D c are exact in fp32; mean = fl(D c / D) = c,
    x - mean = 0, and 0 * rstd * gamma + beta = beta with or without a fused multiply-add."""
    rows = 333
    g = _g(D + rows)
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
    y = torch.full((rows, D), float('nan'), device=dev)
    _chk(_lib().lm_layernorm_rows(_s(), ops._ptr(xg), ops._ptr(gg), ops._ptr(bg), ops._ptr(y), rows, D, 1e-5))
    assert bool(torch.isfinite(y).all()), 'every column of every row is written'
    _close(y, ref, 1e-5, f'layernorm D={D}')
    assert torch.equal(y[5].cpu(), beta) and torch.equal(y[rows - 1].cpu(), beta), 'a constant row must give beta exactly'
    assert torch.equal(y, ops.layernorm(xg, gg, bg, 1e-5))


def test_layernorm_768_stays_refused(dev):
    with pytest.raises(RuntimeError, match='D=768 must be 512 or 1024'):
        ops.layernorm(torch.zeros(4, 768, device=dev), torch.ones(768, device=dev), torch.zeros(768, device=dev))


# ================================================================================ 5. raster width seam
RESO = 0.0625                                                       # 1/16 m: every pixel border is exact in float32
CHUNK = 16384                                                       # points per pass-1 workgroup (csrc/raster.hip)


def _raster_ws_bytes(B, n, nbands):
    """lm_bev_raster_workspace_bytes restated for a known number of bands."""
    nblk = max(1, -(-n // CHUNK))
    return (B * nbands * nblk * 4 + 255) // 256 * 256 + B * nbands * nblk * CHUNK * 4


def _edge_cloud(seed, n, kw, H, W):
    """n points over 1.1 x the tile (a tenth outside), then points exactly on the last row and the last column, on the row and the column
    just outside, and half a pixel beyond the last ones (floor(.. + .5) puts those outside as well)."""
    rng = np.random.RandomState(seed)
    uv = rng.uniform(-0.05, 1.05, (n, 2)) * [H * RESO, W * RESO]
    edge = [((H - 1) * RESO, c * RESO) for c in (0.0, 1.0, W // 2, W - 2.0, W - 1.0, W, W - 0.5)]
    edge += [(r * RESO, (W - 1) * RESO) for r in (0.0, 1.0, H // 2, H - 2.0, H - 1.0, H, H - 0.5)]
    edge += [(H * RESO, (W - 1) * RESO), ((H - 1) * RESO, W * RESO), (0.0, W * RESO), (H * RESO, 0.0)]
    uv = np.concatenate([uv, np.asarray(edge)])
    xyz = np.concatenate([uv + kw['bev_img_offset'] + kw['trans'][:2], rng.uniform(-0.5, 2.0, (len(uv), 1)) + kw['trans'][2]], axis=1)
    return np.concatenate([xyz, np.floor(rng.uniform(0, 65535, (len(uv), 1)))], axis=1).astype(f32)


@pytest.mark.parametrize('H,W,rows', [(32, 2560, 16), (48, 3413, 12), (48, 2561, 12)])
def test_raster_width_seam(dev, H, W, rows):
    """lm_bev_raster_batch at the widest tiles a band of 16 rows (W = 2560: 163840 B of LDS, all there is) and of 12 rows (W = 3413:
    163824 B) can hold, and one pixel past the 16-row limit on a height that has 12-row bands: u8 and f32 bit-exact against the C
    oracle; the workspace size tells which band height was picked."""
    from oracle import raster_ref
    assert rows * W * 4 <= LDS_PER_WG < (rows + 4) * W * 4
    kws = [dict(trans=(8.0, 16.0, 0.5), bev_img_offset=(-1.0, 0.5), img_reso=(RESO, RESO), local_min_ele=-1.0, ele_reso=0.02),
           dict(trans=(-32.0, 4.0, 0.0), bev_img_offset=(0.25, -2.0), img_reso=(RESO, RESO), local_min_ele=-0.5, ele_reso=0.01)]
    clouds = [_edge_cloud(10 * H + b, n, kw, H, W) for b, (n, kw) in enumerate(zip((5000, 3001), kws))]
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).tolist()
    pars = [ops.make_raster_params(**kw) for kw in kws]
    assert _lib().lm_bev_raster_workspace_bytes(2, len(clouds[0]), H, W) == _raster_ws_bytes(2, len(clouds[0]), H // rows), \
        f'{rows}-row bands are expected for H={H} W={W}'
    allp = torch.from_numpy(np.concatenate(clouds)).to(dev)
    out, u8 = ops.bev_raster_batch(allp, offs, pars, H, W, want_u8=True)
    out2, u82 = ops.bev_raster_batch(allp, offs, pars, H, W, want_u8=True)
    assert torch.equal(out, out2) and torch.equal(u8, u82)
    for b in range(2):
        want = raster_ref.raster(clouds[b], raster_ref.params(**kws[b]), H, W)
        assert want[H - 1].any() and want[:, W - 1].any(), 'the oracle has points in the last row and the last column'
        assert np.array_equal(u8[b].cpu().numpy(), want), f'tile {b}'
        assert np.array_equal(out[b].cpu().numpy(), (want.astype(f32) / f32(255.0)).transpose(2, 0, 1)), f'tile {b} (f32)'


def test_raster_widest_band_where_the_cost_model_prefers_16_rows(dev):
    """B = 16 tiles of H = 240, W = 3413: 16-row bands would take one round of workgroups (240 on 256 CUs) against two of 12-row bands
    (320), so a band choice by cost alone takes 16 rows, 218432 B that no CU has.  The 12-row bands must be picked; u8 bit-exact."""
    from oracle import raster_ref
    B, H, W = 16, 240, 3413
    kw = dict(trans=(8.0, 16.0, 0.5), bev_img_offset=(-1.0, 0.5), img_reso=(RESO, RESO), local_min_ele=-1.0, ele_reso=0.02)
    clouds = [_edge_cloud(240 + b, 700 + 13 * b, kw, H, W) for b in range(B)]
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).tolist()
    assert _lib().lm_bev_raster_workspace_bytes(B, max(len(c) for c in clouds), H, W) == _raster_ws_bytes(B, max(len(c) for c in clouds), H // 12)
    allp = torch.from_numpy(np.concatenate(clouds)).to(dev)
    u8 = ops.bev_raster_batch(allp, offs, [ops.make_raster_params(**kw)] * B, H, W, u8_only=True)
    assert torch.equal(u8, ops.bev_raster_batch(allp, offs, [ops.make_raster_params(**kw)] * B, H, W, u8_only=True))
    got = u8.cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], raster_ref.raster(clouds[b], raster_ref.params(**kw), H, W)), f'tile {b}'


@pytest.mark.parametrize('H,W', [(32, 2561), (48, 3414)])
def test_raster_refuses_a_band_beyond_the_lds(dev, H, W):
    """One pixel wider than a band of the tile's height can be: LM_ERR_ARG that names the bound, the outputs untouched (the refusal
    precedes every launch), and the workspace query returns 0."""
    assert _lib().lm_bev_raster_workspace_bytes(2, 1000, H, W) == 0
    pts = torch.zeros((2000, 4), device=dev)
    pars = [ops.make_raster_params(img_reso=(RESO, RESO))] * 2
    out = torch.full((2, 3, H, W), 7.0, device=dev)
    u8 = torch.full((2, H, W, 3), 7, device=dev, dtype=torch.uint8)
    with pytest.raises(LanemapHipError, match=rf'error 1: bev_raster: H={H} W={W}: .*rows\*W <= 40960'):
        ops.bev_raster_batch(pts, [0, 1000, 2000], pars, H, W, out=out, out_u8=u8)
    ws = torch.empty(1 << 20, device=dev, dtype=torch.uint8)        # a caller that brings a workspace of its own is refused the same way
    import ctypes as C
    offs, par = (C.c_long * 3)(0, 1000, 2000), (type(pars[0]) * 2)(*pars)
    rc = _lib().lm_bev_raster_batch_scaled(_s(), ops._ptr(pts), offs, par, 2, ops._ptr(ws), ws.numel(), ops._ptr(out), ops._ptr(u8), H, W, None)
    assert rc == 1 and b'rows*W <= 40960' in _lib().lm_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((u8 == 7).all())


# ================================================================================ 6. the caps that size LDS, reached
def _rot(q):
    q = np.asarray(q, dtype=np.float64)
    n = np.linalg.norm(q)
    w, x, y, z = q / n
    return n * np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _tile_cloud(seed, n, p, H, W):
    """n points over 1.1 x the window of tile p (a tenth outside), heights on a slope with noise, in the LAS frame of the tile."""
    rng = np.random.RandomState(seed)
    v = rng.uniform(-0.05, 1.05, (n, 2)) * [H * float(p.img_reso[0]), W * float(p.img_reso[1])]
    vz = 0.5 + 0.01 * v[:, 0] + 0.02 * v[:, 1] + rng.normal(0, 0.05, n)
    local = np.stack([v[:, 0] + p.bev_img_offset[0], v[:, 1] + p.bev_img_offset[1], vz], axis=1)
    world = (_rot([float(c) for c in p.quat]) @ local.T).T + np.array([float(c) for c in p.trans])
    return np.ascontiguousarray(np.concatenate([world, np.floor(rng.uniform(500, 40000, (n, 1)))], axis=1), dtype=f32)


def test_ground_cell_cap_reached(dev):
    """ops.tile_ground with 181 x 181 = 32761 cells per tile (H = W = 1448, cell_px = 8; the cap is 32768 cells, 128 KB of LDS keys; the
    existing tests reach 36 x 36 and the refusal at 32769+): an axis-aligned and a rotated, tilted tile of about 20,000 points, two
    workgroups each.  cell_min, ground, ground_min and the selection on that ground against tests/ground_ref.py, bit for bit."""
    H = W = 1448
    cell_px = 8
    assert gr.grid_shape(H, W, cell_px) == (181, 181) and 181 * 181 * 4 == 131044
    yaw = 0.4
    tiles = [ops.make_raster_params(trans=(8.0, 16.0, 0.5), bev_img_offset=(-1.0, 0.5), img_reso=(RESO, RESO), local_min_ele=-1.0, ele_reso=0.02),
             ops.make_raster_params(quat=np.array([math.cos(yaw / 2), 0.013, -0.017, math.sin(yaw / 2)]) * 1.03, trans=(40.0, 3.0, -0.25),
                                    bev_img_offset=(0.3, -0.6), img_reso=(0.05, 0.05), local_min_ele=-1.0, ele_reso=0.02)]
    clouds = [_tile_cloud(181, 20011, tiles[0], H, W), _tile_cloud(182, 19937, tiles[1], H, W)]
    pts = np.concatenate(clouds)
    offs = [0, len(clouds[0]), len(pts)]
    cloud = torch.from_numpy(pts).to(dev)
    ground, gmin, cmin = ops.tile_ground(cloud, offs, tiles, H, W, cell_px=cell_px, want_cell_min=True)
    rg, rmin, rc = gr.tile_ground(pts, offs, tiles, H, W, cell_px)
    assert np.isfinite(rc[:, 180, :]).any() and np.isfinite(rc[:, :, 180]).any() and np.isnan(rc).any(), 'the last cells are used, some are empty'
    _bits_equal(cmin, rc, 'cell_min')
    _bits_equal(ground, rg, 'ground')
    _bits_equal(gmin, rmin, 'ground_min')
    g2, m2 = ops.tile_ground(cloud, offs, tiles, H, W, cell_px=cell_px)
    assert torch.equal(g2.view(torch.int32), ground.view(torch.int32)) and torch.equal(m2.view(torch.int32), gmin.view(torch.int32))
    out, o = ops.ground_select(cloud, offs, tiles, ground, H, W, cell_px, (-0.05, 0.2))
    want, woffs = gr.select(pts, offs, tiles, ground.cpu().numpy(), H, W, cell_px, (-0.05, 0.2))
    assert o == woffs.tolist() and 0 < woffs[1] < woffs[2] < len(pts)
    _bits_equal(out, want, 'kept rows')
    out2, o2 = ops.ground_select(cloud, offs, tiles, ground, H, W, cell_px, (-0.05, 0.2))
    assert o2 == o and torch.equal(out2.view(torch.int32), out.view(torch.int32))


def test_drape_vertex_and_height_caps_reached(dev):
    """ops.drape_vertices with both per-tile caps at once: 16384 vertices (128 KB of LDS entries) on one tile of H = 32768 rows (4097 band
    starts, 16 KB; rows and columns are packed into 16 bits each), W = 8, R = 0: 147464 B of dynamic LDS.  Three quarters of the vertices
    sit on pixels that hold a point, rows 0 and H - 1 among them; z, npix and pixel_min against tests/drape_ref.py, bit for bit."""
    H, W, R, V = 32768, 8, 0, 16384
    assert ((H // 8 + 2) // 2 * 2) * 4 + V * 8 == 147464
    p = ops.make_raster_params(trans=(8.0, 16.0, 0.5), bev_img_offset=(-1.0, 0.5), img_reso=(RESO, RESO), local_min_ele=-1.0, ele_reso=0.02)
    pts = _tile_cloud(32768, 40000, p, H, W)
    on, row, col, _ = gr.window(pts, p, H, W)
    assert 30000 < int(on.sum()) < len(pts)
    hit = np.stack([row[on], col[on]], axis=1)[:3 * V // 4 - 2]
    rng = np.random.RandomState(3)
    rest = np.stack([rng.randint(0, H, V - len(hit) - 2), rng.randint(0, W, V - len(hit) - 2)], axis=1)
    pts[-2:, :2] = [[p.bev_img_offset[0] + p.trans[0], 3 * RESO + p.bev_img_offset[1] + p.trans[1]],
                    [(H - 1) * RESO + p.bev_img_offset[0] + p.trans[0], 4 * RESO + p.bev_img_offset[1] + p.trans[1]]]
    verts = np.concatenate([hit, rest, [[0, 3], [H - 1, 4]]]).astype(np.int32)
    verts = verts[rng.permutation(V)]
    assert verts.shape == (V, 2)
    offs, voffs = [0, len(pts)], [0, V]
    cloud = torch.from_numpy(pts).to(dev)
    z, npix, pmin = ops.drape_vertices(cloud, offs, [p], verts, voffs, H, W, radius_px=R, want_pixel_min=True)
    rz, rn, rp = dr.drape_vertices(pts, offs, [p], verts, voffs, H, W, R)
    first, last = [int(np.flatnonzero((verts == v).all(1))[0]) for v in ([0, 3], [H - 1, 4])]
    assert rn[first] == 1 and rn[last] == 1 and 3 * V // 4 - 2 <= int(rn.sum()) < V
    _bits_equal(pmin, rp, 'pixel_min')
    assert np.array_equal(npix.cpu().numpy(), rn), 'npix'
    _bits_equal(z, rz, 'z')
    z2, n2 = ops.drape_vertices(cloud, offs, [p], verts, voffs, H, W, radius_px=R)
    assert torch.equal(z2.view(torch.int32), z.view(torch.int32)) and torch.equal(n2, npix)


def test_strip_tile_cap_reached(dev):
    """ops.strip_bin_points with T = 4096 tiles (the cap: 4 waves x 4096 counters = 64 KB of LDS; the existing tests reach 12 tiles and
    the refusal at 4097): 64 x 64 axis-aligned tiles of 16 x 16 pixels (1 m) every 1.5 m, 300,000 points over the whole layout and a
    little beyond.  Offsets and binned points against the host cut of tests/test_gpu_strip.py (its float32 window test, applied per tile
    to the points of a float64 box one pixel larger than the tile), bit for bit."""
    G, S, step, T = 64, 16, 1.5, 4096
    off = (-0.25, 0.5)
    params = [ops.make_raster_params(trans=(step * (t // G), step * (t % G), 0.25), bev_img_offset=off, img_reso=(RESO, RESO),
                                     local_min_ele=-0.5, ele_reso=0.02) for t in range(T)]
    rng = np.random.RandomState(4096)
    n = 300_000
    xy = rng.uniform(-1.0, step * G + 1.0, (n, 2))
    pts = np.concatenate([xy, rng.normal(0, 0.05, (n, 1)), np.floor(rng.uniform(500, 40000, (n, 1)))], axis=1).astype(f32)
    # the host cut: the candidates of a tile are the points of its box grown by one pixel (float64), the float32 window test decides
    idx = []
    x64, y64 = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    for i in range(G):
        x0 = step * i + off[0] - 1.5 * RESO
        col_i = np.flatnonzero((x64 >= x0) & (x64 <= x0 + (S + 2) * RESO))
        for j in range(G):
            y0 = step * j + off[1] - 1.5 * RESO
            cand = col_i[(y64[col_i] >= y0) & (y64[col_i] <= y0 + (S + 2) * RESO)]
            _, row, col = _member(pts[cand], params[i * G + j])
            idx.append(cand[(row >= 0) & (row < S) & (col >= 0) & (col < S)])
    woffs = np.concatenate([[0], np.cumsum([len(i) for i in idx])]).astype(np.int64)
    want = pts[np.concatenate(idx)]
    counts = np.diff(woffs)
    assert counts.min() >= 1 and 0.3 * n < woffs[-1] < 0.6 * n, 'every tile holds points, about 4 in 9 of the cloud are binned'
    cloud = torch.from_numpy(pts).to(dev)
    binned, offs = ops.strip_bin_points(cloud, params, S, S)
    assert offs == woffs.tolist(), 'offsets differ from the host cut'
    assert np.array_equal(binned.cpu().numpy().view(np.uint32), want.view(np.uint32)), 'binned is not bit-identical to the host cut'
    binned2, offs2 = ops.strip_bin_points(cloud, params, S, S)
    assert offs2 == offs and torch.equal(binned2.view(torch.int32), binned.view(torch.int32))
