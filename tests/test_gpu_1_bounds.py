"""GPU bounds tests (-m gpu): every device kernel reads only its operands and writes only its outputs.

Each operand lives in a guarded slab (tests/guards.py): front guard | rows of `ld` elements | back guard, the operand being a view with the
strides the kernel is given (a channel slice of a wider NHWC tensor, rows with ld > width).  Inputs carry POISON outside the operand (NaN
where nothing stands between a load and a multiply or add; +Inf where the kernel's own max / ReLU would swallow a NaN - those cases use
positive weights and GroupNorm gains so that a stray +Inf survives to the output; 255 for u8; the documented inactive value for integer
operands, never an out-of-range index).  Outputs are pre-filled with a canary bit pattern: afterwards every guard / padding word still
holds it and no logical element does.  Every case runs with benign (zero) guards, with poisoned guards (logical outputs bit-identical) and,
where the entry has a batch dimension, at B = 3 with elements 0 and 2 poisoned (element 1 bit-identical to the B = 1 call).  The benign
outputs are held to an fp64 restatement at the tolerances of the existing tests (1e-5 of the tensor scale, 1e-4 for Winograd F(4x4)).

Guard sizes are given per case: at least one workgroup tile of the kernel that reads or writes the slab.  Shapes are chosen so that a
workgroup tile straddles a batch boundary (H*W not a multiple of the tile, ragged Winograd blocks, 324 / 330 attention tokens)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import ROOT, _chk, _close, _g, _gn_ref, _lib, _nhwc_dev, _nhwc_rows, _rows_nchw, _run_child, _s
from guards import INF, NAN, Slab, batched, guarded_runs

pytestmark = pytest.mark.gpu

# Entries taking a stream that this file does not run through guarded slabs, each with the reason.
BOUNDS_EXEMPT = {
    'lm_wino44_split_fragments': 'elementwise over whole 16-byte quads of a packed weight tensor; run here by ops.pack_wino44_fragments_split',
    'lm_decode_proposals': 'decision kernel on dense head outputs with no ld or slice operand; ties / saturation covered by test_gpu_1_entry_points',
    'lm_decode_orient': 'decision kernel; its ld slice operand is covered by test_decode_orient_ties_inf_and_slices',
    'lm_decode_semantic': 'decision kernel on a dense CHW map with no ld or slice operand; covered against the oracle in test_gpu_1_entry_points',
    'lm_endp_topk': 'decision kernel; saturated / tied inputs covered by test_endp_topk_tied_scores',
    'lm_pack_segments': 'byte copy of host-described segments; destination checked whole by test_pack_segments_vs_torch',
    'lm_softmax_rows': 'in-place rows without ld; covered against fp64 by test_softmax_rows_vs_fp64',
    'lm_rowref_select': 'RowRef decision kernel on dense tensors; covered against the oracle by test_rowref_select_vs_fp64',
    'lm_rowref_gather': 'index kernel whose indices it derives itself; borders covered by test_rowref_gather_borders',
    'lm_rowref_scatter': 'index kernel; shrinking write-back range covered by test_rowref_scatter_shrinking_range',
    'lm_rowref_decode': 'RowRef decision kernel; covered by test_rowref_decode_ties_and_null_maps',
    'lm_exclusive_scan_u32': 'device-wide primitive on a dense vector; sizes up to 2^25 + 1 covered by test_exclusive_scan_u32',
    'lm_sort_pairs_u32': 'device-wide primitive on dense vectors; covered by test_sort_pairs_u32_stable',
    'lm_voxelize_hard': 'variable-length output (row_end on the device); canary slabs under cap_rows, ldf and chaining in test_gpu_sparse_index.py::test_voxelize_raw_*',
    'lm_sparse_grid_build': 'hash-grid build whose output extent depends on the coordinates; guarded slab in test_gpu_sparse_index.py::test_sparse_grid_build',
    'lm_sparse_conv_outputs': 'variable-length output site list; canary slabs under cap_rows in test_gpu_sparse_index.py::test_conv_outputs_raw_cap_rows',
    'lm_sparse_rulebook': 'writes the rulebook conv_gather reads; every word in a canary slab in test_gpu_sparse_index.py::test_conv_outputs_and_rulebook',
    'lm_las_decode_points': 'byte-record parser; every point format covered against the oracle by test_las_read_vs_oracle',
}


def _up(x, Ho, Wo):
    return F.interpolate(x, size=(Ho, Wo), mode='bilinear', align_corners=True)


# ==================================================================================================== conv_mfma
# (name, B-element geometry H x W, Cin, Cout, k, ldx, xlo, ldy, ylo, ldr, rlo).  ACT_NONE throughout: a ReLU epilogue would hide NaN.
@pytest.mark.parametrize('name,H,W,cin,cout,k,ldx,xlo,ldy,ylo,ldr,rlo', [
    # 3x3, K = 288 > 256, M = 143 per element (128-row tiles straddle elements), big_blocks tiny -> launch<64,64,32,32>; ldy vector path
    ('tile64', 13, 11, 32, 96, 3, 40, 4, 104, 4, 100, 0),
    # the same tile with an odd ldy: scalar epilogue, every store of a pixel next to its padding
    ('tile64_scalar', 13, 11, 32, 96, 3, 40, 4, 97, 1, 100, 0),
    # Cout <= 64 -> launch<128,64,32,64>, Cout % 4 != 0: the last channel quad scalar
    ('tile128x64', 9, 23, 64, 37, 3, 72, 8, 44, 4, 41, 2),
    # 1x1 with K = 320 (not tiny-K), 212 x 212 = 44 944 pixels = 351 * 128 + 16: big_blocks = 352 * 2 = 704 >= 700 -> launch<128,128,64,64>
    ('tile128', 212, 212, 320, 256, 1, 328, 4, 264, 4, 260, 4),
])
def test_conv_mfma_bounds(dev, name, H, W, cin, cout, k, ldx, xlo, ldy, ylo, ldr, rlo):
    """lm_conv2d_nhwc_mfma_f32 with x, res and y all column slices of wider NHWC tensors.  Guards: 128 pixel rows + 2 image rows on the
    input (one M tile plus the 3x3 halo), 128 pixel rows on the residual and the output."""
    from lanemapping_amd import ops
    g = _g(H * W + cout)
    x = torch.randn(1, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    r = torch.randn(1, cout, H, W, generator=g)
    ref = F.conv2d(x.double(), w.double(), None, 1, k // 2) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1) + r.double()
    wp, scd, shd = ops.pack_mfma(w.to(dev)), sc.to(dev), sh.to(dev)
    P = H * W
    gi, go = 128 + 2 * W, 128

    def run(B, poisoned):
        pad = NAN if poisoned else 0.0
        xs = Slab(dev, B * P, cin, ldx, xlo, gi, gi).fill_input(batched(_nhwc_rows(x), B, NAN), pad)
        rs = Slab(dev, B * P, cout, ldr, rlo, go, go).fill_input(batched(_nhwc_rows(r), B, NAN), pad)
        ys = Slab(dev, B * P, cout, ldy, ylo, go, go).fill_canary()
        _chk(_lib().lm_conv2d_nhwc_mfma_f32(_s(), xs.ptr(), ldx, wp.data_ptr(), wp.shape[1], scd.data_ptr(), shd.data_ptr(), rs.ptr(), ldr,
                                            0, ys.ptr(), ldy, B, H, W, cin, cout, k, k, 1, k // 2, k // 2, 1, ops.ACT_NONE))
        return {'y': (ys, P)}
    y = guarded_runs(run, f'conv_mfma {name}')['y']
    _close(_rows_nchw(y, 1, H, W), ref, 1e-5, name)


@pytest.mark.parametrize('W,K,N,res_rows', [(130, 512, 300, 26), (650, 320, 1280, 325)])
def test_conv_mfma_res_rows_bounds(dev, W, K, N, res_rows):
    """res_rows broadcast (positional embedding): one-image-row GEMM of W tokens per batch element (W a multiple of res_rows, so
    element 1 of 3 wraps the table like a batch-1 call; W not a multiple of 128: tiles straddle elements).  (130, 300): big_blocks 2 * 3
    -> launch<64,64,32,32>; (650, 1280) at B = 1: 6 * 10 -> 64-wide tiles, at B = 3: 16 * 10 -> same.  x a slice (ldx = K + 8), the
    embedding table rows ld = N + 4 with one table of guard rows (128) on both sides, output guards 128 rows."""
    from lanemapping_amd import ops
    g = _g(W + N)
    x = torch.randn(W, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    sh = torch.randn(N, generator=g)
    emb = torch.randn(res_rows, N, generator=g)
    ref = x.double() @ w.double().t() + sh.double() + emb.double().repeat(W // res_rows, 1)
    wp, shd = ops.pack_mfma(w.to(dev)), sh.to(dev)

    def run(B, poisoned):
        pad = NAN if poisoned else 0.0
        xs = Slab(dev, B * W, K, K + 8, 4, 128, 128).fill_input(batched(x, B, NAN), pad)
        es = Slab(dev, res_rows, N, N + 4, 0, 128, 128).fill_input(emb, pad)
        ys = Slab(dev, B * W, N, N + 4, 4, 128, 128).fill_canary()
        _chk(_lib().lm_conv2d_nhwc_mfma_f32(_s(), xs.ptr(), K + 8, wp.data_ptr(), wp.shape[1], None, shd.data_ptr(), es.ptr(), N + 4,
                                            res_rows, ys.ptr(), N + 4, B, 1, W, K, N, 1, 1, 1, 0, 0, 1, ops.ACT_NONE))
        return {'y': (ys, W)}
    y = guarded_runs(run, f'res_rows {res_rows}')['y']
    _close(y, ref, 1e-5, 'res_rows')


@pytest.mark.parametrize('name,H,W,cin,k,cout,Hr,Wr', [
    ('lateral_up', 20, 24, 64, 1, 256, 10, 12),       # lateral_mfma_kernel<8, true, false>: 1x1 64 -> 256, 480 px = 15 * 32, Wo % 32 != 0
    ('lateral_up_rows', 8, 64, 64, 1, 256, 4, 32),    # lateral_mfma_kernel<8, true, true>: Wo % 32 == 0
    ('tiled', 13, 11, 32, 3, 96, 5, 6),               # not a lateral (3x3, scale): conv_mfma_kernel's resup epilogue, launch<64,64,32,32>
])
def test_conv_mfma_resup_bounds(dev, name, H, W, cin, k, cout, Hr, Wr):
    """lm_conv2d_nhwc_mfma_resup_f32: conv + bilinear(align_corners) upsampled COARSE residual, the coarse residual a column slice
    (ldr = Cout + 8, at column 4).  Guards: 128 pixel rows + 2 image rows on x, one whole coarse image on the residual, 128 on y."""
    from lanemapping_amd import ops
    g = _g(H * W + Hr)
    x = torch.randn(1, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    sc = None if name.startswith('lateral') else torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g)
    rc = torch.randn(1, cout, Hr, Wr, generator=g)
    ref = F.conv2d(x.double(), w.double(), None, 1, k // 2)
    if sc is not None:
        ref = ref * sc.double().view(1, -1, 1, 1)
    ref = ref + sh.double().view(1, -1, 1, 1) + _up(rc.double(), H, W)
    wp, shd = ops.pack_mfma(w.to(dev)), sh.to(dev)
    scd = None if sc is None else sc.to(dev)
    scp = None if scd is None else scd.data_ptr()
    P, ldx, ldr, ldy = H * W, cin + 8, cout + 8, cout + 4

    def run(B, poisoned):
        pad = NAN if poisoned else 0.0
        xs = Slab(dev, B * P, cin, ldx, 4, 128 + 2 * W, 128 + 2 * W).fill_input(batched(_nhwc_rows(x), B, NAN), pad)
        rs = Slab(dev, B * Hr * Wr, cout, ldr, 4, Hr * Wr, Hr * Wr).fill_input(batched(_nhwc_rows(rc), B, NAN), pad)
        ys = Slab(dev, B * P, cout, ldy, 0, 128, 128).fill_canary()
        _chk(_lib().lm_conv2d_nhwc_mfma_resup_f32(_s(), xs.ptr(), ldx, wp.data_ptr(), wp.shape[1], scp, shd.data_ptr(), rs.ptr(), ldr, Hr,
                                                  Wr, ys.ptr(), ldy, B, H, W, cin, cout, k, k, 1, k // 2, k // 2, 1, ops.ACT_NONE))
        return {'y': (ys, P)}
    y = guarded_runs(run, f'resup {name}')['y']
    _close(_rows_nchw(y, 1, H, W), ref, 1e-5, name)


def test_conv_mfma_lateral_plain_residual_bounds(dev):
    """The FPN lateral with a plain residual (lateral_mfma_kernel<16, false, false>: 1x1 128 -> 256, no scale): x, res, y all slices.
    288 px per element = 9 tiles of 32.  Guards: 128 pixel rows everywhere (four of the kernel's 32-pixel tiles)."""
    from lanemapping_amd import ops
    H, W, cin, cout = 12, 24, 128, 256
    g = _g(7)
    x = torch.randn(1, cin, H, W, generator=g)
    w = torch.randn(cout, cin, generator=g) / cin ** 0.5
    sh = torch.randn(cout, generator=g)
    r = torch.randn(1, cout, H, W, generator=g)
    ref = torch.einsum('oc,bchw->bohw', w.double(), x.double()) + sh.double().view(1, -1, 1, 1) + r.double()
    wp, shd, P = ops.pack_mfma(w.to(dev)), sh.to(dev), H * W

    def run(B, poisoned):
        pad = NAN if poisoned else 0.0
        xs = Slab(dev, B * P, cin, 136, 4, 128, 128).fill_input(batched(_nhwc_rows(x), B, NAN), pad)
        rs = Slab(dev, B * P, cout, 264, 8, 128, 128).fill_input(batched(_nhwc_rows(r), B, NAN), pad)
        ys = Slab(dev, B * P, cout, 260, 4, 128, 128).fill_canary()
        _chk(_lib().lm_conv2d_nhwc_mfma_f32(_s(), xs.ptr(), 136, wp.data_ptr(), wp.shape[1], None, shd.data_ptr(), rs.ptr(), 264, 0,
                                            ys.ptr(), 260, B, H, W, cin, cout, 1, 1, 1, 0, 0, 1, ops.ACT_NONE))
        return {'y': (ys, P)}
    y = guarded_runs(run, 'lateral plain')['y']
    _close(_rows_nchw(y, 1, H, W), ref, 1e-5, 'lateral plain residual')


def _stats_close(st, y_ref, name):
    """st [C, 2] (mean, rstd) of one image against fp64: mean within 1e-5 of max(1, |mean|), rstd within 1e-5 relative."""
    mean, rstd = _gn_ref(y_ref)
    mean, rstd = mean[0], rstd[0]
    st = st.double()
    assert float(((st[:, 0] - mean).abs() / mean.abs().clamp_min(1.0)).max()) <= 1e-5, name + ' mean'
    assert float(((st[:, 1] - rstd).abs() / rstd).max()) <= 1e-5, name + ' rstd'


def test_conv_mfma_gnstats_bounds(dev):
    """lm_conv2d_nhwc_mfma_f32_gnstats + lm_gn_finalize: x a slice, y a slice, the fp64 partial buffer and the stats guarded (one
    image's worth of partial rows / 2 stats rows of guard).  Ho * Wo = 384 = 3 tiles of 128; stats of element 1 of 3 equal batch 1."""
    from lanemapping_amd import ops
    H, W, cin, cout = 16, 24, 32, 96
    g = _g(96)
    x = torch.randn(1, cin, H, W, generator=g) + 3.0
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sh = torch.randn(cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), sh.double(), 1, 1)
    wp, shd, P, nch = ops.pack_mfma(w.to(dev)), sh.to(dev), H * W, H * W // 64

    def run(B, poisoned):
        pad = NAN if poisoned else 0.0
        xs = Slab(dev, B * P, cin, 40, 4, 128 + 2 * W, 128 + 2 * W).fill_input(batched(_nhwc_rows(x), B, NAN), pad)
        ys = Slab(dev, B * P, cout, 100, 4, 128, 128).fill_canary()
        ps = Slab(dev, B * nch * cout, 2, 2, 0, nch * cout, nch * cout, torch.float64).fill_canary()
        st = Slab(dev, B * cout, 2, 2, 0, cout, cout).fill_canary()
        _chk(_lib().lm_conv2d_nhwc_mfma_f32_gnstats(_s(), xs.ptr(), 40, wp.data_ptr(), wp.shape[1], shd.data_ptr(), ys.ptr(), 100,
                                                    ps.ptr(), B, H, W, cin, cout, 3, 3, 1, 1, 1, 1))
        _chk(_lib().lm_gn_finalize(_s(), ps.ptr(), st.ptr(), B, P, cout, nch, C.c_float(1e-5)))
        return {'y': (ys, P), 'partial': (ps, nch * cout), 'stats': (st, cout)}
    out = guarded_runs(run, 'gnstats conv')
    _close(_rows_nchw(out['y'], 1, H, W), ref, 1e-5, 'gnstats y')
    _stats_close(out['stats'], ref, 'gnstats')


# ==================================================================================================== Winograd F(4x4, 3x3)
# ragged H and W (W not a multiple of 4 * dil; the fused kernel needs W >= ~41 dil), dilation 1..3, ldy % 4 != 0 (scalar store) and ldy % 4 == 0 (vector store)
_W44 = [(13, 45, 1, 43), (22, 86, 2, 48), (17, 125, 3, 41), (13, 45, 1, 44)]


def _w44_case(seed, H, W, cin, cout, dil):
    g = _g(seed)
    x = torch.randn(1, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    r = torch.randn(1, cout, H, W, generator=g)
    return x, w, sc, sh, r


@pytest.mark.parametrize('split', [False, True])
@pytest.mark.parametrize('H,W,dil,ldy', _W44)
def test_winograd44_and_twin_bounds(dev, H, W, dil, ldy, split):
    """lm_conv3x3_winograd44_f32 and lm_conv3x3_winograd44_twin_f32 (split: the fp16-split second line and its twin; |x| < 4 << 650)
    with x, res, y as slices: both against fp64 at 1e-4 and bit-identical to each other.  Guards: 4 * dil + 2 image rows + 64 pixels
    (one ragged 4x4 block row with its halo) on x, res and y."""
    from lanemapping_amd import ops
    cin, cout = 32, 40
    x, w, sc, sh, r = _w44_case(H * W + dil, H, W, cin, cout, dil)
    assert ops.wino44_supported(H, W, cin, dil)
    ref = (F.conv2d(x.double(), w.double(), None, 1, dil, dil) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
           + r.double())
    wu = ops.pack_wino44(w.to(dev))
    if split:
        wf = ops.pack_wino44_fragments_split(wu)
        words, post = wf.words, wf.post
        wu_t = (wu * ops.split_scale(wu)).contiguous()
    else:
        words, post, wu_t = ops.pack_wino44_fragments(wu), None, wu
    scd, shd, P, gd = sc.to(dev), sh.to(dev), H * W, (4 * dil + 2) * W + 64
    ldx, ldr = 40, 44

    def run(B, poisoned, twin):
        pad = NAN if poisoned else 0.0
        xs = Slab(dev, B * P, cin, ldx, 8, gd, gd).fill_input(batched(_nhwc_rows(x), B, NAN), pad)
        rs = Slab(dev, B * P, cout, ldr, 4, gd, gd).fill_input(batched(_nhwc_rows(r), B, NAN), pad)
        ys = Slab(dev, B * P, cout, ldy, 1 if ldy % 4 else 4, gd, gd).fill_canary()      # (16-byte aligned on the vector path)
        a = (_s(), xs.ptr(), ldx)
        b = (scd.data_ptr(), shd.data_ptr(), rs.ptr(), ldr, ys.ptr(), ldy, B, H, W, cin, cout, dil, ops.ACT_NONE)
        L = _lib()
        if twin:
            need = L.lm_winograd44_twin_workspace_bytes(B, H, W, cin, wu.shape[1], dil)
            ws = torch.empty(need, device=dev, dtype=torch.uint8)
            if split:
                _chk(L.lm_conv3x3_winograd44_split_twin_f32(*a, wu_t.data_ptr(), wu.shape[1], *b, ws.data_ptr(), need, C.c_float(post)))
            else:
                _chk(L.lm_conv3x3_winograd44_twin_f32(*a, wu_t.data_ptr(), wu.shape[1], *b, ws.data_ptr(), need))
        elif split:
            _chk(L.lm_conv3x3_winograd44_split_f32(*a, words.data_ptr(), words.shape[2] * 32, *b, None, C.c_float(post)))
        else:
            _chk(L.lm_conv3x3_winograd44_f32(*a, words.data_ptr(), words.shape[2] * 32, *b, None))
        return {'y': (ys, P)}
    tag = 'split ' if split else ''
    y = guarded_runs(lambda B, p: run(B, p, False), f'{tag}wino44 H{H} W{W} d{dil} ldy{ldy}')['y']
    yt = guarded_runs(lambda B, p: run(B, p, True), f'{tag}wino44 twin H{H} W{W} d{dil} ldy{ldy}')['y']
    _close(_rows_nchw(y, 1, H, W), ref, 1e-4, f'{tag}wino44')
    assert torch.equal(y, yt), 'fused and twin Winograd differ'


@pytest.mark.parametrize('split', [1, 2])
def test_winograd44_gn_partial_bounds(dev, split):
    """The Winograd gn_partial epilogue (+ lm_gn_finalize / lm_gn_finalize_split): x a slice, y a slice (ldy = 132), the partial buffer
    and the stats guarded by one image's worth of rows; H = 21, W = 46 (ragged 4x4 blocks, 966 pixels).  Element 1's stats of a
    poisoned batch of 3 are finite and equal to batch 1 ([split][B][C/split][2]: picked per half)."""
    from lanemapping_amd import ops
    H, W, cin, cout = 21, 46, 32, 128
    g = _g(split)
    x = torch.randn(1, cin, H, W, generator=g) + 1.0
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sh = torch.randn(cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), sh.double(), 1, 1)
    wf = ops.pack_wino44_fragments(ops.pack_wino44(w.to(dev)))
    shd, P, nch, gd = sh.to(dev), H * W, _lib().lm_winograd44_gn_chunks(H, W, 1), 6 * W + 64
    cs = cout // split

    def run(B, poisoned):
        pad = NAN if poisoned else 0.0
        xs = Slab(dev, B * P, cin, 36, 4, gd, gd).fill_input(batched(_nhwc_rows(x), B, NAN), pad)
        ys = Slab(dev, B * P, cout, 132, 4, gd, gd).fill_canary()
        ps = Slab(dev, B * nch * cout, 2, 2, 0, nch * cout, nch * cout, torch.float64).fill_canary()
        st = Slab(dev, B * cout, 2, 2, 0, cout, cout).fill_canary()
        L = _lib()
        _chk(L.lm_conv3x3_winograd44_f32(_s(), xs.ptr(), 36, wf.data_ptr(), wf.shape[2] * 32, None, shd.data_ptr(), None, 0, ys.ptr(), 132,
                                         B, H, W, cin, cout, 1, ops.ACT_NONE, ps.ptr()))
        if split == 1:
            _chk(L.lm_gn_finalize(_s(), ps.ptr(), st.ptr(), B, P, cout, nch, C.c_float(1e-5)))
        else:
            _chk(L.lm_gn_finalize_split(_s(), ps.ptr(), st.ptr(), B, P, cout, nch, C.c_float(1e-5), split))
        return {'y': (ys, P), 'partial': (ps, nch * cout), 'stats': (st, cout)}
    if split == 1:
        out = guarded_runs(run, 'wino44 gn_partial')
        st = out['stats']
    else:   # [split][B][C/split][2]: element rows are not contiguous; check the batch-3 element by hand
        out = guarded_runs(run, 'wino44 gn_partial split', batch=False)
        st = out['stats']
        three = run(3, True)
        torch.cuda.synchronize()
        three['stats'][0].check_canary('wino44 gn split stats B=3')
        s3 = three['stats'][0].view.cpu().view(split, 3, cs, 2)[:, 1].reshape(cout, 2)
        assert torch.isfinite(s3).all() and torch.equal(s3, st), 'gn_split = 2: element 1 of 3 differs from batch 1'
        st = st.view(split, cs, 2).reshape(cout, 2)
    _close(_rows_nchw(out['y'], 1, H, W), ref, 1e-4, 'wino44 gn y')
    assert torch.isfinite(st).all()
    _stats_close(st, ref, f'wino44 gn split {split}')


# ==================================================================================================== thin layers
@pytest.mark.parametrize('name,H,W,cin,cout,k,stride,pre_relu', [
    ('mfma_s1', 19, 23, 16, 5, 3, 1, False),      # small_conv3x3_mfma_kernel<1>
    ('mfma_s2', 19, 23, 16, 5, 3, 2, False),      # small_conv3x3_mfma_kernel<2>
    ('valu_3x3', 19, 23, 8, 5, 3, 1, False),      # Cin != 16: small_conv_kernel (VALU)
    ('valu_1x1', 19, 23, 32, 3, 1, 1, False),
    ('valu_pre_relu', 19, 23, 8, 5, 3, 1, True),  # relu(x) inside: +Inf poison, positive weights
])
def test_conv_small_bounds(dev, name, H, W, cin, cout, k, stride, pre_relu):
    """lm_conv2d_nhwc_small, x a slice (ldx = Cin + 4 at column 4), y a slice (ldy = 12 for Cout <= 5: seven padding channels per pixel).
    Guards: 256 pixel rows + 2 image rows (one 256-pixel VALU workgroup and the halo) on x, 256 pixel rows on y."""
    _small_conv_case(dev, name, H, W, cin, cout, k, stride, pre_relu)


def _small_conv_case(dev, name, H, W, cin, cout, k, stride, pre_relu):
    from lanemapping_amd import ops
    g = _g(H * cin + cout + stride)
    x = torch.randn(1, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    if pre_relu:
        w = w.abs()
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    xin = F.relu(x.double()) if pre_relu else x.double()
    ref = F.conv2d(xin, w.double(), None, stride, k // 2) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    Ho, Wo = ref.shape[2:]
    w16, scd, shd = ops.pack_small(w.to(dev)), sc.to(dev), sh.to(dev)
    poison = INF if pre_relu else NAN
    ldx, ldy, P, Po = cin + 4, 12, H * W, Ho * Wo

    def run(B, poisoned):
        pad = poison if poisoned else 0.0
        xs = Slab(dev, B * P, cin, ldx, 4, 256 + 2 * W, 256 + 2 * W).fill_input(batched(_nhwc_rows(x), B, poison), pad)
        ys = Slab(dev, B * Po, cout, ldy, 0, 256, 256).fill_canary()
        _chk(_lib().lm_conv2d_nhwc_small(_s(), xs.ptr(), ldx, w16.data_ptr(), scd.data_ptr(), shd.data_ptr(), ys.ptr(), ldy, B, H, W, cin,
                                         cout, k, k, stride, k // 2, k // 2, int(pre_relu), ops.ACT_NONE))
        return {'y': (ys, Po)}
    y = guarded_runs(run, f'conv_small {name}')['y']
    _close(_rows_nchw(y, 1, Ho, Wo), ref, 1e-5, name)


_SMALL_VALU_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']
import torch
import test_gpu_1_bounds as t
dev = torch.device('cuda:0')
for s in (1, 2):
    t._small_conv_case(dev, f'valu_forced_s{s}', 19, 23, 16, 5, 3, s, False)
print('ok')
"""


def test_conv_small_forced_valu_bounds(dev):
    """The Cin = 16 3x3 shapes on the VALU kernel (LM_SMALL_CONV_VALU=1, read once per process: a child process)."""
    p = _run_child(_SMALL_VALU_CHILD, ROOT, env={'LM_SMALL_CONV_VALU': '1'}, timeout=600)
    assert p.stdout.strip().endswith('ok'), p.stdout[-2000:] + p.stderr[-4000:]


@pytest.mark.parametrize('u8', [False, True])
def test_stem_bounds(dev, u8):
    """lm_stem_conv7x7_bn_relu (planar f32) and its u8 HWC form: relu(bn(conv7x7 s2)) with positive weights and scales, so that a stray
    +Inf (f32 poison) / 255 (u8 poison) read shows through the ReLU.  H = 37, W = 43 (ragged 16 x 16 output tiles).  Guards: 48 input
    rows (16 output rows' worth of all three planes), 256 output pixel rows (one 16 x 16 tile)."""
    from lanemapping_amd import ops
    H, W = 37, 43
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = _g(37 + u8)
    if u8:
        xu = torch.randint(0, 200, (1, H, W, 3), generator=g, dtype=torch.uint8)
        x64 = xu.permute(0, 3, 1, 2).double() / 255.0
    else:
        x = torch.rand(1, 3, H, W, generator=g)
        x64 = x.double()
    w = torch.rand(64, 3, 7, 7, generator=g) / 20
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    ref = F.relu(F.conv2d(x64, w.double(), None, 2, 3) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
    wk, scd, shd = w.permute(2, 3, 1, 0).contiguous().to(dev), sc.to(dev), sh.to(dev)

    def run(B, poisoned):
        if u8:
            xs = Slab(dev, B * H, W * 3, None, 0, 48, 48, torch.uint8).fill_input(batched(xu.reshape(H, W * 3), B, 255), 255 if poisoned else 0)
        else:
            xs = Slab(dev, B * 3 * H, W, None, 0, 48, 48).fill_input(batched(x.reshape(3 * H, W), B, INF), INF if poisoned else 0.0)
        ys = Slab(dev, B * Ho * Wo, 64, None, 0, 256, 256).fill_canary()
        fn = _lib().lm_stem_conv7x7_bn_relu_u8 if u8 else _lib().lm_stem_conv7x7_bn_relu
        _chk(fn(_s(), xs.ptr(), wk.data_ptr(), scd.data_ptr(), shd.data_ptr(), ys.ptr(), B, H, W))
        return {'y': (ys, Ho * Wo)}
    y = guarded_runs(run, f'stem u8={u8}')['y']
    _close(_rows_nchw(y, 1, Ho, Wo), ref, 1e-5, 'stem')


def test_maxpool_bounds(dev):
    """lm_maxpool3x3s2_nhwc with +Inf poison (a max swallows NaN): H = 19, W = 25, C = 12.  Guards: 2 image rows + 256 pixels on x,
    256 pixel rows on y (one 256-thread workgroup of channel quads)."""
    H, W, Cc = 19, 25, 12
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = torch.randn(1, Cc, H, W, generator=_g(19))
    ref = F.max_pool2d(x.double(), 3, 2, 1)

    def run(B, poisoned):
        xs = Slab(dev, B * H * W, Cc, None, 0, 2 * W + 256, 2 * W + 256).fill_input(batched(_nhwc_rows(x), B, INF), INF if poisoned else 0.0)
        ys = Slab(dev, B * Ho * Wo, Cc, None, 0, 256, 256).fill_canary()
        _chk(_lib().lm_maxpool3x3s2_nhwc(_s(), xs.ptr(), ys.ptr(), B, H, W, Cc))
        return {'y': (ys, Ho * Wo)}
    y = guarded_runs(run, 'maxpool')['y']
    _close(_rows_nchw(y, 1, Ho, Wo), ref, 1e-5, 'maxpool')


# ==================================================================================================== normalisation / resampling
def test_gn_stats_bounds(dev):
    """lm_gn_stats: H * W = 15 * 13 = 195 (not a multiple of the 64-pixel chunks: a chunk straddles elements).  Guards: 256 pixel rows on
    x, one element's stats on the output."""
    H, W, Cc = 15, 13, 64
    x = torch.randn(1, Cc, H, W, generator=_g(64)) * 2 + 5

    def run(B, poisoned):
        xs = Slab(dev, B * H * W, Cc, None, 0, 256, 256).fill_input(batched(_nhwc_rows(x), B, NAN), NAN if poisoned else 0.0)
        ws = torch.empty(_lib().lm_gn_stats_workspace_bytes(B, H * W, Cc) // 8, device=dev, dtype=torch.float64)
        st = Slab(dev, B * Cc, 2, None, 0, Cc, Cc).fill_canary()
        _chk(_lib().lm_gn_stats(_s(), xs.ptr(), ws.data_ptr(), st.ptr(), B, H * W, Cc, C.c_float(1e-5)))
        return {'stats': (st, Cc)}
    st = guarded_runs(run, 'gn_stats')['stats']
    assert torch.isfinite(st).all()
    _stats_close(st, x, 'gn_stats')


def _gn_relu64(x, st, gamma, beta):
    m, r = st[:, 0].double().view(1, -1, 1, 1), st[:, 1].double().view(1, -1, 1, 1)
    return F.relu((x.double() - m) * r * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1))


def _gn_input(seed, Cc, H, W):
    g = _g(seed)
    x = torch.randn(1, Cc, H, W, generator=g) * 2 + 1
    m, r = _gn_ref(x)
    st = torch.stack([m[0], r[0]], 1).float()
    return x, st


def test_gn_relu_upsample_bounds(dev):
    """lm_gn_relu_upsample: 7 x 9 -> 15 x 18, C = 32, gamma > 0 so that +Inf poison survives the ReLU.  Guards: 2 input image rows +
    256 pixels, 256 output pixel rows."""
    Hi, Wi, Ho, Wo, Cc = 7, 9, 15, 18, 32
    x, st = _gn_input(5, Cc, Hi, Wi)
    g = _g(6)
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1
    ref = _up(_gn_relu64(x, st, gamma, beta), Ho, Wo)
    gd, bd = gamma.to(dev), beta.to(dev)

    def run(B, poisoned):
        pad = INF if poisoned else 0.0
        xs = Slab(dev, B * Hi * Wi, Cc, None, 0, 2 * Wi + 256, 2 * Wi + 256).fill_input(batched(_nhwc_rows(x), B, INF), pad)
        ss = Slab(dev, B * Cc, 2, None, 0, Cc, Cc).fill_input(batched(st, B, NAN), pad)
        ys = Slab(dev, B * Ho * Wo, Cc, None, 0, 256, 256).fill_canary()
        _chk(_lib().lm_gn_relu_upsample(_s(), xs.ptr(), ss.ptr(), gd.data_ptr(), bd.data_ptr(), ys.ptr(), B, Hi, Wi, Ho, Wo, Cc, 0))
        return {'y': (ys, Ho * Wo)}
    y = guarded_runs(run, 'gn_relu_upsample')['y']
    _close(_rows_nchw(y, 1, Ho, Wo), ref, 1e-5, 'gn_relu_upsample')


@pytest.mark.parametrize('proj', [False, True])
def test_gn_relu_upsample_sum_bounds(dev, proj):
    """lm_gn_relu_upsample_sum (and _conv1x1 with y = NULL): three terms, each a channel slice of a merged two-branch tensor (ldx = 2C,
    terms at column 0, C, 0 as the FPN's merged Winograd outputs), gamma > 0 and +Inf poison.  37 x 45 output: 9 x 11, 19 x 23 and
    37 x 45 inputs.  The projection: cout = 5 into ldy1 = 8.  Guards: 2 image rows + 256 pixels per term, 256 output pixel rows."""
    Cc, Ho, Wo = 32, 37, 45
    sizes = [(9, 11), (19, 23), (37, 45)]
    los = [0, Cc, 0]
    terms = [_gn_input(10 + k, Cc, h, w) for k, (h, w) in enumerate(sizes)]
    g = _g(11)
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1
    ref = None
    for (x, st) in terms:
        t = _up(_gn_relu64(x, st, gamma, beta), Ho, Wo)
        ref = t if ref is None else ref + t
    gd, bd = gamma.to(dev), beta.to(dev)
    cout = 5
    w1 = torch.randn(cout, Cc, 1, 1, generator=g) / Cc ** 0.5
    b1 = torch.randn(cout, generator=g)
    ref1 = torch.einsum('oc,bchw->bohw', w1[:, :, 0, 0].double(), ref) + b1.double().view(1, -1, 1, 1)
    from lanemapping_amd import ops
    w16, b1d = ops.pack_small(w1.to(dev)), b1.to(dev)

    def run(B, poisoned):
        pad = INF if poisoned else 0.0
        xs, ss = [], []
        for k, ((x, st), (h, w)) in enumerate(zip(terms, sizes)):
            xs.append(Slab(dev, B * h * w, Cc, 2 * Cc, los[k], 2 * w + 256, 2 * w + 256).fill_input(batched(_nhwc_rows(x), B, INF), pad))
            ss.append(Slab(dev, B * Cc, 2, None, 0, Cc, Cc).fill_input(batched(st, B, NAN), pad))
        vp3, i3 = C.c_void_p * 3, C.c_int * 3
        head = (_s(), 3, vp3(*[s.ptr() for s in xs]), vp3(*[s.ptr() for s in ss]), i3(*[h for h, _ in sizes]), i3(*[w for _, w in sizes]),
                i3(2 * Cc, 2 * Cc, 2 * Cc), gd.data_ptr(), bd.data_ptr())
        if not proj:
            ys = Slab(dev, B * Ho * Wo, Cc, None, 0, 256, 256).fill_canary()
            _chk(_lib().lm_gn_relu_upsample_sum(*head, ys.ptr(), B, Ho, Wo, Cc))
            return {'y': (ys, Ho * Wo)}
        y1 = Slab(dev, B * Ho * Wo, cout, 8, 0, 256, 256).fill_canary()
        _chk(_lib().lm_gn_relu_upsample_sum_conv1x1(*head, None, B, Ho, Wo, Cc, w16.data_ptr(), b1d.data_ptr(), cout, y1.ptr(), 8))
        return {'y1': (y1, Ho * Wo)}
    out = guarded_runs(run, f'gn_relu_upsample_sum proj={proj}')
    if proj:
        _close(_rows_nchw(out['y1'], 1, Ho, Wo), ref1, 1e-5, 'gn sum conv1x1')
    else:
        _close(_rows_nchw(out['y'], 1, Ho, Wo), ref, 1e-5, 'gn sum')


@pytest.mark.parametrize('Hi,Wi,Ho,Wo', [(5, 7, 11, 16), (6, 5, 13, 13)])     # Wo % 4 == 0 (quad path) and Wo = 13 (scalar path)
def test_upsample_bilinear_bounds(dev, Hi, Wi, Ho, Wo):
    """lm_upsample_bilinear_nhwc with x, add and y as slices (ldx = C + 8 at column 4, lda = C + 4, ldy = C + 4 at column 4), and
    lm_upsample_bilinear_to_chw from the same slice into planar rows.  Guards: 2 image rows + 256 pixels on x / add / y; 4 planar rows
    on the CHW output."""
    Cc = 12
    g = _g(Ho * Wo)
    x = torch.randn(1, Cc, Hi, Wi, generator=g)
    add = torch.randn(1, Cc, Ho, Wo, generator=g)
    ref = _up(x.double(), Ho, Wo)
    gi, go = 2 * Wi + 256, 2 * Wo + 256

    def run(B, poisoned):
        pad = NAN if poisoned else 0.0
        xs = Slab(dev, B * Hi * Wi, Cc, Cc + 8, 4, gi, gi).fill_input(batched(_nhwc_rows(x), B, NAN), pad)
        ad = Slab(dev, B * Ho * Wo, Cc, Cc + 4, 0, go, go).fill_input(batched(_nhwc_rows(add), B, NAN), pad)
        ys = Slab(dev, B * Ho * Wo, Cc, Cc + 4, 4, go, go).fill_canary()
        yc = Slab(dev, B * Cc * Ho, Wo, None, 0, 4, 4).fill_canary()
        L = _lib()
        _chk(L.lm_upsample_bilinear_nhwc(_s(), xs.ptr(), Cc + 8, ad.ptr(), Cc + 4, ys.ptr(), Cc + 4, B, Hi, Wi, Ho, Wo, Cc))
        _chk(L.lm_upsample_bilinear_to_chw(_s(), xs.ptr(), Cc + 8, yc.ptr(), B, Hi, Wi, Ho, Wo, Cc))
        return {'y': (ys, Ho * Wo), 'chw': (yc, Cc * Ho)}
    out = guarded_runs(run, f'upsample {Hi}x{Wi}->{Ho}x{Wo}')
    _close(_rows_nchw(out['y'], 1, Ho, Wo), ref + add.double(), 1e-5, 'upsample + add')
    _close(out['chw'].view(1, Cc, Ho, Wo), ref, 1e-5, 'upsample to chw')


def test_upsample_bicubic_bounds(dev):
    """lm_upsample_bicubic_nhwc: 9 x 11 -> 20 x 23, C = 8.  Guards: 4 image rows + 256 pixels on x (two-tap-deep borders), 256 output
    pixel rows."""
    H, W, Ho, Wo, Cc = 9, 11, 20, 23, 8
    x = torch.randn(1, Cc, H, W, generator=_g(23))
    ref = F.interpolate(x.double(), size=(Ho, Wo), mode='bicubic', align_corners=False)

    def run(B, poisoned):
        xs = Slab(dev, B * H * W, Cc, None, 0, 4 * W + 256, 4 * W + 256).fill_input(batched(_nhwc_rows(x), B, NAN), NAN if poisoned else 0.0)
        ys = Slab(dev, B * Ho * Wo, Cc, None, 0, 256, 256).fill_canary()
        _chk(_lib().lm_upsample_bicubic_nhwc(_s(), xs.ptr(), ys.ptr(), B, H, W, Cc, Ho, Wo))
        return {'y': (ys, Ho * Wo)}
    y = guarded_runs(run, 'bicubic')['y']
    _close(_rows_nchw(y, 1, Ho, Wo), ref, 1e-5, 'bicubic')


@pytest.mark.parametrize('D', [512, 1024])
def test_layernorm_bounds(dev, D):
    """lm_layernorm_rows: 37 rows per batch element.  Guards: 64 rows."""
    rows = 37
    g = _g(D)
    x = torch.randn(rows, D, generator=g) * 3 + 1
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    ref = F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5)
    gd, bd = gamma.to(dev), beta.to(dev)

    def run(B, poisoned):
        xs = Slab(dev, B * rows, D, None, 0, 64, 64).fill_input(batched(x, B, NAN), NAN if poisoned else 0.0)
        ys = Slab(dev, B * rows, D, None, 0, 64, 64).fill_canary()
        _chk(_lib().lm_layernorm_rows(_s(), xs.ptr(), gd.data_ptr(), bd.data_ptr(), ys.ptr(), B * rows, D, C.c_float(1e-5)))
        return {'y': (ys, rows)}
    y = guarded_runs(run, f'layernorm {D}')['y']
    _close(y, ref, 1e-5, 'layernorm')


def test_unpatchify_bounds(dev):
    """lm_unpatchify: 5 x 5 patches of 3 x 3, 7 channels, bit-exact.  Guards: one image of tokens / of output pixels."""
    G, P, Cc = 5, 3, 7
    tok = torch.randn(G * G, P * P * Cc, generator=_g(357))
    ref = tok.view(1, G, G, P, P, Cc).permute(0, 5, 1, 3, 2, 4).reshape(1, Cc, G * P, G * P)
    npx = G * P * G * P

    def run(B, poisoned):
        ts = Slab(dev, B * G * G, P * P * Cc, None, 0, G * G, G * G).fill_input(batched(tok, B, NAN), NAN if poisoned else 0.0)
        ys = Slab(dev, B * npx, Cc, None, 0, npx, npx).fill_canary()
        _chk(_lib().lm_unpatchify(_s(), ts.ptr(), ys.ptr(), B, G, P, Cc))
        return {'y': (ys, npx)}
    y = guarded_runs(run, 'unpatchify')['y']
    assert torch.equal(_rows_nchw(y, 1, G * P, G * P), ref)


def test_token_mix_bounds(dev):
    """lm_token_mix_mfma_f32: K = 37, M = 70, N = 96 (no tile multiple), residual.  Guards: 128 rows of N on x, res and y."""
    from lanemapping_amd import ops
    K, M, N = 37, 70, 96
    g = _g(3770)
    x = torch.randn(K, N, generator=g)
    w = torch.randn(M, K, generator=g) / K ** 0.5
    bias = torch.randn(M, generator=g)
    res = torch.randn(M, N, generator=g)
    ref = w.double() @ x.double() + bias.double()[:, None] + res.double()
    wt, bd = ops.pack_token_mix(w.to(dev)), bias.to(dev)

    def run(B, poisoned):
        pad = NAN if poisoned else 0.0
        xs = Slab(dev, B * K, N, None, 0, 128, 128).fill_input(batched(x, B, NAN), pad)
        rs = Slab(dev, B * M, N, None, 0, 128, 128).fill_input(batched(res, B, NAN), pad)
        ys = Slab(dev, B * M, N, None, 0, 128, 128).fill_canary()
        _chk(_lib().lm_token_mix_mfma_f32(_s(), xs.ptr(), wt.data_ptr(), wt.shape[1], bd.data_ptr(), rs.ptr(), ys.ptr(), B, M, K, N,
                                          ops.ACT_NONE))
        return {'y': (ys, M)}
    y = guarded_runs(run, 'token_mix')['y']
    _close(y, ref, 1e-5, 'token_mix')


# ==================================================================================================== attention
def _attn_ref(qkv, N, heads, valid=None):
    q, k, v = [z.reshape(1, N, heads, 64).transpose(1, 2).double() for z in qkv.chunk(3, dim=-1)]
    s = q @ k.transpose(-1, -2) * 0.125
    if valid is not None:
        s = s.masked_fill(~valid.bool().view(1, 1, 1, N), float('-inf'))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(N, heads * 64)


@pytest.mark.parametrize('N', [50, 324, 330])     # 50: attention_kernel (VALU); 324 / 330: attention_mfma_kernel, 32-key blocks past N
def test_attention_bounds(dev, N):
    """lm_attention_f32, two heads.  Guards: 64 token rows on qkv and out (two 32-key blocks)."""
    heads = 2
    qkv = torch.randn(N, 3 * heads * 64, generator=_g(N)) * 1.5
    ref = _attn_ref(qkv, N, heads)

    def run(B, poisoned):
        qs = Slab(dev, B * N, 3 * heads * 64, None, 0, 64, 64).fill_input(batched(qkv, B, NAN), NAN if poisoned else 0.0)
        ys = Slab(dev, B * N, heads * 64, None, 0, 64, 64).fill_canary()
        _chk(_lib().lm_attention_f32(_s(), qs.ptr(), ys.ptr(), B, N, heads, 64, C.c_float(0.125)))
        return {'out': (ys, N)}
    y = guarded_runs(run, f'attention N={N}')['out']
    _close(y, ref, 1e-5, f'attention N={N}')


def test_attention_masked_bounds(dev):
    """lm_attention_masked_f32, N = 45, about half the tokens keys.  The valid slab's guards hold 0 (inactive); the poisoned batch
    elements flag every token (in range, pointing at NaN rows).  Guards: 64 token rows on qkv / out, one element's flags on valid."""
    N, heads = 45, 2
    g = _g(45)
    qkv = torch.randn(N, 3 * heads * 64, generator=g)
    valid = (torch.rand(N, generator=g) < 0.5).int()
    valid[3] = 1
    ref = _attn_ref(qkv, N, heads, valid)

    def run(B, poisoned):
        qs = Slab(dev, B * N, 3 * heads * 64, None, 0, 64, 64).fill_input(batched(qkv, B, NAN), NAN if poisoned else 0.0)
        vs = Slab(dev, B, N, None, 0, 1, 1, torch.int32).fill_input(batched(valid.view(1, N), B, 1), 0)
        ys = Slab(dev, B * N, heads * 64, None, 0, 64, 64).fill_canary()
        _chk(_lib().lm_attention_masked_f32(_s(), qs.ptr(), ys.ptr(), vs.ptr(), B, N, heads, 64, C.c_float(0.125)))
        return {'out': (ys, N)}
    y = guarded_runs(run, 'attention masked')['out']
    _close(y, ref, 1e-5, 'attention masked')


# ==================================================================================================== column-proposal head
def test_head_proposal_conf_bounds(dev):
    """lm_head_proposal_conf: 5 proposals per element, L = 1000.  Guards: 2 rows of L on tok (one workgroup each), 2 rows on conf."""
    P, L = 5, 1000
    g = _g(1000)
    tok = torch.randn(P, L, generator=g)
    wt = torch.randn(2, L, generator=g) / L ** 0.5
    bias = torch.randn(2, generator=g)
    ref = tok.double() @ wt.double().t() + bias.double()
    wd, bd = wt.to(dev), bias.to(dev)

    def run(B, poisoned):
        ts = Slab(dev, B * P, L, None, 0, 2, 2).fill_input(batched(tok, B, NAN), NAN if poisoned else 0.0)
        cs = Slab(dev, B * P, 2, None, 0, 2, 2).fill_canary()
        _chk(_lib().lm_head_proposal_conf(_s(), ts.ptr(), wd.data_ptr(), bd.data_ptr(), cs.ptr(), B * P, L))
        return {'conf': (cs, P)}
    y = guarded_runs(run, 'proposal_conf')['conf']
    _close(y, ref, 1e-5, 'proposal_conf')


@pytest.mark.parametrize('D', [100, 132])     # 100: head_stage2_lds_kernel (128 * 101 * 4 B <= 64 KB); 132: head_stage2_kernel (LDS too small)
def test_head_stage2_bounds(dev, D):
    """lm_head_stage2 with ldh = 3 D + 8 (> 3 D: the hidden rows are slices of a wider matrix), M = 185 rows per element (a ragged
    128-row block).  Guards: 128 rows on hid and on the three outputs."""
    M, ldh = 185, 3 * D + 8
    g = _g(D)
    hid = torch.randn(M, 3 * D, generator=g)
    w2 = torch.randn(23, D, generator=g) / 10
    b2 = torch.randn(23, generator=g)
    h64, w64, b64 = hid.double(), w2.double(), b2.double()
    refs = [h64[:, 0:D] @ w64[0:3].t() + b64[0:3], h64[:, D:2 * D] @ w64[3:13].t() + b64[3:13],
            h64[:, 2 * D:3 * D] @ w64[13:23].t() + b64[13:23]]
    wd, bd = w2.to(dev), b2.to(dev)

    def run(B, poisoned):
        hs = Slab(dev, B * M, 3 * D, ldh, 4, 128, 128).fill_input(batched(hid, B, NAN), NAN if poisoned else 0.0)
        outs = [Slab(dev, B * M, n, None, 0, 128, 128).fill_canary() for n in (3, 10, 10)]
        _chk(_lib().lm_head_stage2(_s(), hs.ptr(), ldh, D, wd.data_ptr(), bd.data_ptr(), *[o.ptr() for o in outs], B * M))
        return {k: (o, M) for k, o in zip(('ext2', 'cls2', 'off2'), outs)}
    out = guarded_runs(run, f'head_stage2 D={D}')
    for k, r in zip(('ext2', 'cls2', 'off2'), refs):
        _close(out[k], r, 1e-5, k)


def _window_tokens_ref(row, P, prop_width=2, half_buff=4):
    """tok[(p, h), c * 10 + w] = zero-padded row[c, h, prop_width p + w - half_buff] (polyline_fpn_vit_vertex_2.py:382,392-395)."""
    Cc, Hr, Wr = row.shape[1:]
    rowp = F.pad(row.double(), (half_buff, half_buff, 0, 0))
    fw = prop_width + 2 * half_buff
    toks = [rowp[0, :, :, prop_width * p: prop_width * p + fw].permute(1, 0, 2).reshape(Hr, Cc * fw) for p in range(P)]
    return torch.cat(toks)


@pytest.mark.parametrize('spatial', [False, True])
def test_head_tokens_bounds(dev, spatial):
    """lm_head_tokens_window (fp64 restatement of the zero-padded row windows) and lm_head_tokens (seg-weighted: its values are held
    bit-exact to the unguarded ops.head_tokens call, which the G3 / G22 goldens pin).  Hr = Wr = 25 (a ragged block of token rows),
    P = 12.  Guards: 2 image rows + 256 pixels on row / seg, 64 token rows on tok."""
    from lanemapping_amd import ops
    Hr, Wr, P = 25, 25, 12
    g = _g(25 + spatial)
    row = torch.randn(1, 16, Hr, Wr, generator=g)
    seg = torch.randn(1, 2 * Hr, 2 * Wr, generator=g)
    if spatial:
        ref = ops.head_tokens(seg.view(1, 1, 2 * Hr, 2 * Wr).to(dev), _nhwc_dev(row, dev), P, 2, 4, -0.37).cpu()
    else:
        ref = _window_tokens_ref(row, P)
    rows_el = P * Hr

    def run(B, poisoned):
        pad = NAN if poisoned else 0.0
        rs = Slab(dev, B * Hr * Wr, 16, None, 0, 2 * Wr + 256, 2 * Wr + 256).fill_input(batched(_nhwc_rows(row), B, NAN), pad)
        ts = Slab(dev, B * rows_el, 160, None, 0, 64, 64).fill_canary()
        if spatial:
            ss = Slab(dev, B * 2 * Hr, 2 * Wr, None, 0, 8, 8).fill_input(batched(seg[0], B, NAN), pad)
            _chk(_lib().lm_head_tokens(_s(), ss.ptr(), rs.ptr(), ts.ptr(), C.c_float(-0.37), B, P, Hr, Wr, 2, 4))
        else:
            _chk(_lib().lm_head_tokens_window(_s(), rs.ptr(), ts.ptr(), B, P, Hr, Wr, 2, 4))
        return {'tok': (ts, rows_el)}
    tok = guarded_runs(run, f'head_tokens spatial={spatial}')['tok']
    if spatial:
        assert torch.equal(tok, ref)
    else:
        _close(tok, ref, 1e-5, 'head_tokens_window')


# ==================================================================================================== sparse (config 5)
@pytest.mark.parametrize('cin,cout,taps,M', [(16, 16, 27, 1037), (32, 200, 9, 900)])
def test_conv_gather_bounds(dev, cin, cout, taps, M):
    """lm_conv_gather_mfma_f32: x rows a slice (ldx = Cin + 16, at column 0, padding channels poisoned), y a slice (ldy = Cout + 4), the
    rulebook's guard entries -1 (inactive).  No batch dimension.  Guards: 128 rows on x, nbr and y (one M tile)."""
    from lanemapping_amd import ops
    V = 500
    g = _g(cin + cout + taps)
    x = torch.randn(V, cin, generator=g)
    nbr = torch.randint(0, V, (M, taps), generator=g, dtype=torch.int32)
    nbr[torch.rand(M, taps, generator=g) < 0.35] = -1
    kd = (3, 3, 3) if taps == 27 else (1, 3, 3)
    w = torch.randn(*kd, cin, cout, generator=g) / (taps * cin) ** 0.5
    sh = torch.randn(cout, generator=g)
    xe = torch.cat([x.double(), torch.zeros(1, cin, dtype=torch.float64)])
    ref = torch.einsum('mtc,tco->mo', xe[torch.where(nbr < 0, V, nbr).long()], w.double().reshape(taps, cin, cout)) + sh.double()
    wp, shd = ops.pack_sparse(w.to(dev)), sh.to(dev)
    ldx, ldy = cin + 16, cout + 4

    def run(B, poisoned):
        xs = Slab(dev, V, cin, ldx, 0, 128, 128).fill_input(x, NAN if poisoned else 0.0)
        ns = Slab(dev, M, taps, None, 0, 128, 128, torch.int32).fill_input(nbr, -1)
        ys = Slab(dev, M, cout, ldy, 0, 128, 128).fill_canary()
        _chk(_lib().lm_conv_gather_mfma_f32(_s(), xs.ptr(), ldx, ns.ptr(), taps, wp.data_ptr(), wp.shape[1], None, shd.data_ptr(), None, 0,
                                            ys.ptr(), ldy, M, cin, cout, ops.ACT_NONE))
        return {'y': (ys, M)}
    y = guarded_runs(run, f'conv_gather {cin}->{cout}', batch=False)['y']
    _close(y, ref, 1e-5, 'conv_gather')


@pytest.mark.parametrize('flip_h', [False, True])
def test_sparse_to_dense_bounds(dev, flip_h):
    """lm_sparse_to_dense_nhwc: feature rows a slice (ldf = 32 > C = 20, padding poisoned), every output cell written (0 where no
    site); the batch index lives in the coordinates, so batch isolation is element 1 of 3 with sites in elements 0 and 2 carrying NaN.
    Guards: 64 feature / coordinate rows (coordinates: copies of a real site of the same element - in range), 256 output pixel rows."""
    D, H, W, Cc, n = 3, 19, 23, 20, 300
    g = _g(70 + flip_h)
    cells = torch.randperm(D * H * W, generator=g)[:n]
    z, r = cells // (H * W), cells % (H * W)
    coords1 = torch.stack([torch.zeros_like(z), z, r // W, r % W], 1).int()
    feats = torch.randn(n, Cc, generator=g)
    dense = torch.zeros(1, Cc, D, H, W)
    dense[0, :, z, r // W, r % W] = feats.t()
    want = dense.view(1, Cc * D, H, W)
    if flip_h:
        want = torch.flip(want, dims=[2])

    def run(B, poisoned):
        pad = NAN if poisoned else 0.0
        if B == 1:
            co, fe = coords1, feats
        else:
            co = torch.cat([coords1 + torch.tensor([b, 0, 0, 0], dtype=torch.int32) for b in range(3)])
            fe = torch.cat([torch.full_like(feats, NAN), feats, torch.full_like(feats, NAN)])
        fs = Slab(dev, co.shape[0], Cc, 32, 0, 64, 64).fill_input(fe, pad)
        cs = Slab(dev, co.shape[0], 4, None, 0, 64, 64, torch.int32).fill_input(co, 0)
        cs.flat.view(-1, 4)[:64] = co[0]
        cs.flat.view(-1, 4)[-64:] = co[0]
        ys = Slab(dev, B * H * W, Cc * D, None, 0, 256, 256).fill_canary()
        _chk(_lib().lm_sparse_to_dense_nhwc(_s(), fs.ptr(), 32, cs.ptr(), co.shape[0], ys.ptr(), B, D, H, W, Cc, int(flip_h)))
        return {'y': (ys, H * W)}
    y = guarded_runs(run, f'sparse_to_dense flip={flip_h}')['y']
    assert torch.equal(_rows_nchw(y, 1, H, W), want)


# ==================================================================================================== rasteriser / ingest
def test_tile_ingest_bounds(dev):
    """lm_tile_ingest_u8: [B][H][W][4] u8 -> planar f32 (u8 / 255, first three channels), 255 poison, H = 17, W = 29.  Guards: 4 image
    rows on the source, 4 planar rows on the output."""
    H, W, Cc = 17, 29, 4
    u = torch.randint(0, 255, (H, W * Cc), generator=_g(17), dtype=torch.uint8)
    ref = u.view(1, H, W, Cc)[..., :3].permute(0, 3, 1, 2).double() / 255.0

    def run(B, poisoned):
        xs = Slab(dev, B * H, W * Cc, None, 0, 4, 4, torch.uint8).fill_input(batched(u, B, 255), 255 if poisoned else 0)
        ys = Slab(dev, B * 3 * H, W, None, 0, 4, 4).fill_canary()
        _chk(_lib().lm_tile_ingest_u8(_s(), xs.ptr(), ys.ptr(), B, H, W, Cc))
        return {'y': (ys, 3 * H)}
    y = guarded_runs(run, 'tile_ingest')['y']
    _close(y.view(1, 3, H, W), ref, 1e-7, 'tile_ingest')


def test_bev_raster_decoys(dev):
    """lm_bev_raster_batch with decoy points - inside the tile, intensity and elevation at their maxima - placed before tile_offsets[0]
    and after tile_offsets[B] (64 records each), and elements 0 and 2 of a batch of 3 made of decoys only: element 1 (and the batch-1
    call) bit-identical to the call on the real points alone, which test_gpu_1_kernels holds to the C oracle.  Outputs guarded by 4
    planar rows (f32) and 4 image rows (u8)."""
    from lanemapping_amd import ops
    from lanemapping_amd import synth
    Hh = Ww = 1152
    pts = torch.from_numpy(synth.las_points(96, 20000))
    prm = ops.make_raster_params()
    decoy = pts[:64].clone()
    decoy[:, 2] = 1e4
    decoy[:, 3] = 1e9
    plain, plain_u8 = ops.bev_raster_batch(pts.to(dev), [0, pts.shape[0]], [prm], Hh, Ww, want_u8=True)
    assert int((plain_u8 != 0).sum()) > 1000, 'the real points must land inside the tile'

    def run(B, poisoned):
        lead = decoy if poisoned else torch.zeros(0, 4)
        parts = [lead] + ([decoy, pts, decoy] if B == 3 else [pts]) + [decoy if poisoned else torch.zeros(0, 4)]
        offs = [lead.shape[0]]
        for p in parts[1:-1]:
            offs.append(offs[-1] + p.shape[0])
        allp = torch.cat(parts).contiguous().to(dev)
        cap = max(offs[i + 1] - offs[i] for i in range(B))
        need = _lib().lm_bev_raster_workspace_bytes(B, cap, Hh, Ww)
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
        ys = Slab(dev, B * 3 * Hh, Ww, None, 0, 4, 4).fill_canary()
        us = Slab(dev, B * Hh, Ww * 3, None, 0, 4, 4, torch.uint8).fill_canary()
        from lanemapping_amd._lib import LmRasterParams
        _chk(_lib().lm_bev_raster_batch(_s(), allp.data_ptr(), (C.c_long * (B + 1))(*offs), (LmRasterParams * B)(*([prm] * B)), B,
                                        ws.data_ptr(), need, ys.ptr(), us.ptr(), Hh, Ww))
        torch.cuda.synchronize()
        return {'chw': (ys, 3 * Hh), 'u8': (us, Hh)}
    out = guarded_runs(run, 'bev_raster')
    assert torch.equal(out['chw'].view(1, 3, Hh, Ww), plain.cpu())
    assert torch.equal(out['u8'].view(1, Hh, Ww, 3), plain_u8.cpu())
