"""Thin torch-tensor front end of the C-ABI (plumbing only: pointers, shapes, the current HIP stream).

Activation convention: tensors are *logically* NCHW (same shapes as the reference) but stored
channels-last (NHWC) — ``x.stride(1) == 1`` — so every kernel sees pixel-major rows with the channel
vector contiguous.  A channel slice of a wider NHWC buffer is a legal operand (its pixel stride ``ld``
is read from ``x.stride(3)``).  Every function raises if a tensor is not on a HIP device: there is no
CPU fallback.
"""
import ctypes as C
import math

import torch

from ._lib import lib, check, LmRasterParams, LmStripGrid, LmLineGrid, LmPaintTable, LanemapHipError

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2


def _stream():
    # raw current-stream handle straight from the C bindings: torch.cuda.current_stream() spends ~8 us per call in Python
    # device-index plumbing, and every launch asks for it
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise LanemapHipError('lanemapping_amd ops need tensors on an MI355X (HIP) device; no CPU fallback exists')
    if t.device.index != torch._C._cuda_getDevice():
        # the library launches on the current HIP device and _stream() is that device's current stream
        raise LanemapHipError(f'tensor on cuda:{t.device.index} but the current device is cuda:{torch._C._cuda_getDevice()}: '
                              'call torch.cuda.set_device() (one process drives one GPU)')
    return C.c_void_p(t.data_ptr())


def new_act(B, C_, H, W, device, dtype=torch.float32):
    """Fresh NHWC-stored activation, returned as a logical [B,C,H,W] view."""
    return torch.empty((B, H, W, C_), device=device, dtype=dtype).permute(0, 3, 1, 2)


def nhwc_ld(x):
    """Pixel stride of x [B,C,H,W] if it is NHWC-stored (channel stride 1, pixel-major rows, pixel stride >= C), else None."""
    B, C_, H, W = x.shape
    sb, sc, sh, sw = x.stride()
    ok = (sc == 1 or C_ == 1) and sw >= C_ and (sh == W * sw or H == 1) and (sb == H * W * sw or B == 1)
    return sw if ok else None


def as_nhwc(x):
    """Return (tensor, ld): x itself if it is NHWC-stored (channel stride 1, pixel-major rows, pixel
    stride ld >= C), else an NHWC copy."""
    ld = nhwc_ld(x)
    if ld is None:
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        ld = x.shape[1]
    return x, ld


# ------------------------------------------------------------------------------- weight packing
def fold_bn(bn, conv_bias=None, eps=1e-5):
    """Eval-mode BatchNorm as a per-channel (scale, shift) applied to the raw conv accumulator."""
    scale = bn.weight / torch.sqrt(bn.running_var + eps)
    shift = bn.bias - bn.running_mean * scale
    if conv_bias is not None:
        shift = shift + conv_bias * scale
    return scale.float().contiguous(), shift.float().contiguous()


def pack_mfma(w):
    """[Cout,Cin,KH,KW] (or [N,K] linear) -> [KH*KW, CoutP, Cin] with CoutP = Cout rounded up to 128."""
    if w.dim() == 2:
        w = w[:, :, None, None]
    if w.dim() == 3:
        w = w[:, :, :, None]
    co, ci, kh, kw = w.shape
    cop = (co + 127) // 128 * 128
    p = torch.zeros((kh * kw, cop, ci), device=w.device, dtype=torch.float32)
    p[:, :co, :] = w.permute(2, 3, 0, 1).reshape(kh * kw, co, ci)
    return p.contiguous()


_W44_G = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]


def pack_wino44(w):
    """[Cout,Cin,3,3] -> Winograd F(4x4,3x3) weights U = G g G^T as [36, CoutP, Cin] (xi = 6 i + j), CoutP = Cout rounded up to 64.
    The product is formed in fp64 and rounded to fp32 once (G carries 1/6, 1/12, 1/24: csrc/conv_wino44.hip)."""
    co, ci, kh, kw = w.shape
    assert kh == 3 and kw == 3
    G = torch.tensor(_W44_G, device=w.device, dtype=torch.float64)
    U = torch.einsum('ij,ocjk,lk->iloc', G, w.double(), G).reshape(36, co, ci).float()
    cop = (co + 63) // 64 * 64
    p = torch.zeros((36, cop, ci), device=w.device, dtype=torch.float32)
    p[:, :co, :] = U
    return p.contiguous()


def pack_wino44_fragments(wu):
    """pack_wino44 output U [36, CoutP, Cin] -> the per-wave-fragment order of lm_conv3x3_winograd44_f32:
    [36][Cin/8][CoutP/32][lane 64][4] with lane = khalf * 32 + row, channel = u*8 + khalf*4 + e."""
    xi, cop, ci = wu.shape
    assert xi == 36 and cop % 64 == 0 and ci % 16 == 0
    t = wu.reshape(36, cop // 32, 32, ci // 8, 2, 4)                       # xi, nt, row, u, khalf, e
    return t.permute(0, 3, 1, 4, 2, 5).contiguous().reshape(36, ci // 8, cop // 32, 64, 4)


class SplitFragments:
    """U fragments of the split-precision second line (lm_conv3x3_winograd44_split_f32): `words` = the fp16 term words in fragment order
    (a float32 tensor holding bits, the shape pack_wino44_fragments gives), `post` = 1 / the power of two U was scaled by."""
    __slots__ = ('words', 'post')

    def __init__(self, words, post):
        self.words, self.post = words, float(post)

    @property
    def shape(self):
        return self.words.shape


def split_scale(wu):
    """The power of two that brings max |U| to [2^12, 2^13): the fp16 low terms of U then stay normal numbers."""
    m = float(wu.abs().max())
    return 1.0 if m == 0.0 else 2.0 ** (12 - math.floor(math.log2(m)))


def pack_wino44_fragments_split(wu):
    """pack_wino44 output U [36, CoutP, Cin] (on the GPU) -> SplitFragments: U * 2^k in fragment order, split into fp16 term words on the
    device by the helper the kernels use (lm_wino44_split_fragments)."""
    assert wu.is_cuda, 'the fragments are split on the device (no CPU path)'
    sc = split_scale(wu)
    frag = pack_wino44_fragments(wu * sc)
    out = torch.empty_like(frag)
    check(lib().lm_wino44_split_fragments(_stream(), _ptr(frag), _ptr(out), frag.numel() // 4))
    return SplitFragments(out, 1.0 / sc)


def pack_small(w):
    """[Cout<=16,Cin,KH,KW] -> [KH*KW, Cin, 16].  Cout = 32, 48 or 64 -> [Cout/16, KH*KW, Cin, 16]: one 16-wide block per 16 outputs
    (lm_conv2d_nhwc_small)."""
    co, ci, kh, kw = w.shape
    if co > 16:
        assert co % 16 == 0 and co <= 64, f'pack_small: Cout={co} must be <= 16 or 32 / 48 / 64'
        return torch.stack([pack_small(w[16 * i:16 * (i + 1)]) for i in range(co // 16)]).contiguous()
    p = torch.zeros((kh * kw, ci, 16), device=w.device, dtype=torch.float32)
    p[:, :, :co] = w.permute(2, 3, 1, 0).reshape(kh * kw, ci, co)
    return p.contiguous()


def pack_token_mix(w):
    """Token-mixing weight [M,K] (or Conv1d [M,K,1]) -> W^T zero padded to [ceil(K/16)*16, ceil(M/128)*128] (lm_token_mix_mfma_f32)."""
    if w.dim() == 3:
        w = w[:, :, 0]
    m, k = w.shape
    p = torch.zeros(((k + 15) // 16 * 16, (m + 127) // 128 * 128), device=w.device, dtype=torch.float32)
    p[:k, :m] = w.t()
    return p.contiguous()


# ------------------------------------------------------------------------------- convolutions / GEMM
_conv_hook = None   # optional profiler hook: called as hook(kind, algorithmic_flops, launch_fn[, executed_flops])


def set_conv_hook(fn):
    global _conv_hook
    _conv_hook = fn


def conv_mfma(x, wp, cout, kh=1, kw=1, stride=1, pad=0, dil=1, scale=None, shift=None, res=None, act=ACT_NONE,
              out=None, res_rows=0, res_up=None):
    """res_up: a COARSE [B,cout,Hr,Wr] map that is added through bilinear (align_corners) interpolation to the output size inside the
    epilogue (`_upsample_add` of the FPN) - the upsampled map is never written."""
    x, ldx = as_nhwc(x)
    B, cin, H, W = x.shape
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    Ho = (H + 2 * ph - dil * (kh - 1) - 1) // stride + 1
    Wo = (W + 2 * pw - dil * (kw - 1) - 1) // stride + 1
    if out is None:
        out = new_act(B, cout, Ho, Wo, x.device)
    out_, ldy = as_nhwc(out)
    assert out_.data_ptr() == out.data_ptr(), 'conv_mfma: `out` must already be NHWC-stored'
    ldr = 0
    if res is not None:
        if res.dim() == 4:
            res, ldr = as_nhwc(res)
        else:
            ldr = res.stride(0)
    if res_up is not None:
        assert res is None and res_rows == 0
        ru, ldu = as_nhwc(res_up)
        assert ru.shape[0] == B and ru.shape[1] == cout

    def launch():
        if res_up is not None:
            check(lib().lm_conv2d_nhwc_mfma_resup_f32(_stream(), _ptr(x), ldx, _ptr(wp), wp.shape[1], _ptr(scale), _ptr(shift),
                                                      _ptr(ru), ldu, ru.shape[2], ru.shape[3], _ptr(out), ldy, B, H, W, cin, cout,
                                                      kh, kw, stride, ph, pw, dil, act))
            return
        check(lib().lm_conv2d_nhwc_mfma_f32(_stream(), _ptr(x), ldx, _ptr(wp), wp.shape[1], _ptr(scale), _ptr(shift),
                                            _ptr(res), ldr, res_rows, _ptr(out), ldy, B, H, W, cin, cout, kh, kw,
                                            stride, ph, pw, dil, act))
    if _conv_hook is not None:
        _conv_hook(f'conv {cin}->{cout} k{kh}x{kw} s{stride} d{dil} @{H}x{W} B{B}', 2.0 * B * Ho * Wo * cout * cin * kh * kw, launch)
    else:
        launch()
    return out


def _hooked(kind, flops, launch, executed=None):
    if _conv_hook is not None:
        _conv_hook(kind, flops, launch, executed)
    else:
        launch()


def wino44_supported(H, W, cin, dil=1, ldx=None):
    """ldx: pixel stride of the input in floats (default: dense, cin).  The Winograd kernel addresses an image through 32-bit byte
    offsets: an image that spans 2^31 bytes or more (a narrow channel slice of a very wide tensor) is not covered."""
    return bool(lib().lm_winograd44_supported_ld(int(H), int(W), int(cin), int(dil), int(cin if ldx is None else ldx)))


def wino44_covers(x, dil=1):
    """wino44_supported for the tensor x [B,C,H,W] as conv_wino44 would see it (as_nhwc: its own pixel stride when it is NHWC-stored,
    a dense copy otherwise) - what the callers that fall back to the direct kernel ask."""
    return wino44_supported(x.shape[2], x.shape[3], x.shape[1], dil, nhwc_ld(x))


def conv_wino44(x, wf, cout, dil=1, scale=None, shift=None, res=None, act=ACT_NONE, out=None, gn_eps=None, gn_split=1):
    """3x3 / stride 1 / pad = dil convolution via Winograd F(4x4,3x3), exact fp32 MFMA, no transformed tensors in HBM
    (csrc/conv_wino44.hip wino44_kernel: 0.5625x the matrix work of the F(2x2) kernels).  wf = pack_wino44_fragments(pack_wino44(w)).
    Bit-identical to conv_wino44_twin.  With gn_eps returns (y, stats)."""
    x, ldx = as_nhwc(x)
    B, cin, H, W = x.shape
    cop = wf.shape[2] * 32
    y = out if out is not None else new_act(B, cout, H, W, x.device)
    y_, ldy = as_nhwc(y)
    assert y_.data_ptr() == y.data_ptr(), 'conv_wino44: `out` must already be NHWC-stored'
    r, ldr = (None, 0) if res is None else as_nhwc(res)
    part = None
    if gn_eps is not None:
        part = torch.empty((B, lib().lm_winograd44_gn_chunks(H, W, dil), cout, 2), device=x.device, dtype=torch.float64)
    tiles = lib().lm_winograd44_tiles(B, H, W, dil)
    if isinstance(wf, SplitFragments):          # second line: fp16 x 2 split products (three MFMA terms per product: 3 x the algorithmic count executed)
        _hooked(f'wino44split {cin}->{cout} k3x3 d{dil} @{H}x{W} B{B}', 2.0 * B * H * W * cout * cin * 9,
                lambda: check(lib().lm_conv3x3_winograd44_split_f32(_stream(), _ptr(x), ldx, _ptr(wf.words), cop, _ptr(scale), _ptr(shift), _ptr(r),
                                                                    ldr, _ptr(y), ldy, B, H, W, cin, cout, dil, act, _ptr(part), wf.post)),
                3 * 2.0 * 36 * tiles * cin * cout)
    else:
        _hooked(f'wino44 {cin}->{cout} k3x3 d{dil} @{H}x{W} B{B}', 2.0 * B * H * W * cout * cin * 9,
                lambda: check(lib().lm_conv3x3_winograd44_f32(_stream(), _ptr(x), ldx, _ptr(wf), cop, _ptr(scale), _ptr(shift), _ptr(r), ldr,
                                                              _ptr(y), ldy, B, H, W, cin, cout, dil, act, _ptr(part))),
                2.0 * 36 * tiles * cin * cout)
    if gn_eps is None:
        return y
    if gn_split > 1:
        stats = torch.empty((gn_split, B, cout // gn_split, 2), device=x.device, dtype=torch.float32)
        check(lib().lm_gn_finalize_split(_stream(), _ptr(part), _ptr(stats), B, H * W, cout, part.shape[1], gn_eps, gn_split))
        return y, stats
    stats = torch.empty((B, cout, 2), device=x.device, dtype=torch.float32)
    check(lib().lm_gn_finalize(_stream(), _ptr(part), _ptr(stats), B, H * W, cout, part.shape[1], gn_eps))
    return y, stats


def conv_wino44_twin(x, wu, cout, dil=1, scale=None, shift=None, res=None, act=ACT_NONE, out=None, split=False):
    """The same convolution through the materialising twin (V and M tensors in HBM, three plain kernels): test infrastructure,
    bit-identical to conv_wino44.  wu = pack_wino44(w).  split: the twin of the split-precision second line (same scale rule as
    pack_wino44_fragments_split)."""
    x, ldx = as_nhwc(x)
    B, cin, H, W = x.shape
    cop = wu.shape[1]
    y = out if out is not None else new_act(B, cout, H, W, x.device)
    y_, ldy = as_nhwc(y)
    assert y_.data_ptr() == y.data_ptr(), 'conv_wino44_twin: `out` must already be NHWC-stored'
    r, ldr = (None, 0) if res is None else as_nhwc(res)
    need = lib().lm_winograd44_twin_workspace_bytes(B, H, W, cin, cop, dil)
    ws = torch.empty(need, device=x.device, dtype=torch.uint8)
    if split:
        sc = split_scale(wu)
        wus = (wu * sc).contiguous()
        check(lib().lm_conv3x3_winograd44_split_twin_f32(_stream(), _ptr(x), ldx, _ptr(wus), cop, _ptr(scale), _ptr(shift), _ptr(r), ldr,
                                                         _ptr(y), ldy, B, H, W, cin, cout, dil, act, _ptr(ws), need, 1.0 / sc))
        return y
    check(lib().lm_conv3x3_winograd44_twin_f32(_stream(), _ptr(x), ldx, _ptr(wu), cop, _ptr(scale), _ptr(shift), _ptr(r), ldr,
                                               _ptr(y), ldy, B, H, W, cin, cout, dil, act, _ptr(ws), need))
    return y


def conv_mfma_gnstats(x, wp, cout, kh, kw, stride, pad, dil, shift, eps=1e-5):
    """conv (+bias) and, from the same kernel, the GroupNorm(C,C) statistics of its output -> (y, stats [B,C,2])."""
    x, ldx = as_nhwc(x)
    B, cin, H, W = x.shape
    Ho = (H + 2 * pad - dil * (kh - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    out = new_act(B, cout, Ho, Wo, x.device)
    nchunk = Ho * Wo // 64
    part = torch.empty((B, nchunk, cout, 2), device=x.device, dtype=torch.float64)
    stats = torch.empty((B, cout, 2), device=x.device, dtype=torch.float32)
    def launch():
        check(lib().lm_conv2d_nhwc_mfma_f32_gnstats(_stream(), _ptr(x), ldx, _ptr(wp), wp.shape[1], _ptr(shift), _ptr(out), cout,
                                                    _ptr(part), B, H, W, cin, cout, kh, kw, stride, pad, pad, dil))
    if _conv_hook is not None:
        _conv_hook(f'conv+gn {cin}->{cout} k{kh}x{kw} s{stride} d{dil} @{H}x{W} B{B}', 2.0 * B * Ho * Wo * cout * cin * kh * kw, launch)
    else:
        launch()
    check(lib().lm_gn_finalize(_stream(), _ptr(part), _ptr(stats), B, Ho * Wo, cout, nchunk, eps))
    return out, stats


def linear_mfma(x2d, wp, n_out, scale=None, shift=None, res=None, res_rows=0, act=ACT_NONE, out=None):
    """y[M,n_out] = act((x2d @ W^T) * scale + shift + res).  x2d [M,K] row-major (K % 32 == 0)."""
    assert x2d.dim() == 2 and x2d.stride(1) == 1
    M, K = x2d.shape
    if out is None:
        out = torch.empty((M, n_out), device=x2d.device, dtype=torch.float32)
    ldr = res.stride(0) if res is not None else 0
    def launch():
        check(lib().lm_conv2d_nhwc_mfma_f32(_stream(), _ptr(x2d), x2d.stride(0), _ptr(wp), wp.shape[1], _ptr(scale),
                                            _ptr(shift), _ptr(res), ldr, res_rows, _ptr(out), out.stride(0),
                                            1, 1, M, K, n_out, 1, 1, 1, 0, 0, 1, act))
    if _conv_hook is not None:
        _conv_hook(f'gemm M{M} K{K} N{n_out}', 2.0 * M * n_out * K, launch)
    else:
        launch()
    return out


def token_mix(x2d, wt, M, bias, B, res=None, act=ACT_NONE, out=None):
    """MLP-Mixer token mixing: y[b] = act(W @ x[b] + bias[:, None]) (+ res[b]) for each of the B batch elements.
    x2d [B*K, N] row-major (token rows, channels contiguous), wt = pack_token_mix(W) of W [M, K], bias [M] -> [B*M, N]."""
    assert x2d.dim() == 2 and x2d.is_contiguous() and x2d.shape[0] % B == 0
    K, N = x2d.shape[0] // B, x2d.shape[1]
    assert wt.shape[0] >= K and wt.shape[1] >= M and bias.numel() == M
    if out is None:
        out = torch.empty((B * M, N), device=x2d.device, dtype=torch.float32)
    assert out.is_contiguous() and tuple(out.shape) == (B * M, N)
    if res is not None:
        assert res.is_contiguous() and tuple(res.shape) == (B * M, N)
    def launch():
        check(lib().lm_token_mix_mfma_f32(_stream(), _ptr(x2d), _ptr(wt), wt.shape[1], _ptr(bias), _ptr(res), _ptr(out),
                                          B, M, K, N, act))
    if _conv_hook is not None:
        _conv_hook(f'token_mix M{M} K{K} N{N} B{B}', 2.0 * B * M * K * N, launch)
    else:
        launch()
    return out


def conv_small(x, w16, cout, kh=1, kw=1, stride=1, pad=0, scale=None, shift=None, pre_relu=False, act=ACT_NONE, out=None):
    x, ldx = as_nhwc(x)
    B, cin, H, W = x.shape
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    Ho = (H + 2 * ph - kh) // stride + 1
    Wo = (W + 2 * pw - kw) // stride + 1
    if out is None:
        out = new_act(B, cout, Ho, Wo, x.device)
    out_, ldy = as_nhwc(out)
    assert out_.data_ptr() == out.data_ptr()
    check(lib().lm_conv2d_nhwc_small(_stream(), _ptr(x), ldx, _ptr(w16), _ptr(scale), _ptr(shift), _ptr(out), ldy,
                                     B, H, W, cin, cout, kh, kw, stride, ph, pw, int(pre_relu), act))
    return out


def stem(x, w_k64, scale, shift):
    """proj -> relu(bn(conv7x7 s2)) [B,64,H/2,W/2] NHWC-stored.  proj: [B,3,H,W] f32 planar (the reference's tensor) or
    [B,H,W,3] uint8 (rasteriser / PNG reader output; u8 / 255 is applied inside the kernel: same bits)."""
    x = x.contiguous()
    if x.dtype == torch.uint8:
        B, H, W, C_ = x.shape
        assert C_ == 3, 'u8 tiles are [B,H,W,3]'
    else:
        B, _, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = new_act(B, 64, Ho, Wo, x.device)
    fn = lib().lm_stem_conv7x7_bn_relu_u8 if x.dtype == torch.uint8 else lib().lm_stem_conv7x7_bn_relu
    check(fn(_stream(), _ptr(x), _ptr(w_k64), _ptr(scale), _ptr(shift), _ptr(out), B, H, W))
    return out


def maxpool3x3s2(x):
    x, ld = as_nhwc(x)
    B, C_, H, W = x.shape
    assert ld == C_
    out = new_act(B, C_, (H - 1) // 2 + 1, (W - 1) // 2 + 1, x.device)
    check(lib().lm_maxpool3x3s2_nhwc(_stream(), _ptr(x), _ptr(out), B, H, W, C_))
    return out


# ------------------------------------------------------------------------------- norm / resize
def gn_stats(x, eps=1e-5):
    x, ld = as_nhwc(x)
    B, C_, H, W = x.shape
    assert ld == C_
    ws = torch.empty(lib().lm_gn_stats_workspace_bytes(B, H * W, C_) // 8, device=x.device, dtype=torch.float64)
    stats = torch.empty((B, C_, 2), device=x.device, dtype=torch.float32)
    check(lib().lm_gn_stats(_stream(), _ptr(x), _ptr(ws), _ptr(stats), B, H * W, C_, eps))
    return stats


def gn_relu_upsample(x, stats, gamma, beta, size, out=None, accumulate=False):
    x, ld = as_nhwc(x)
    B, C_, H, W = x.shape
    assert ld == C_
    Ho, Wo = size
    if out is None:
        assert not accumulate
        out = new_act(B, C_, Ho, Wo, x.device)
    check(lib().lm_gn_relu_upsample(_stream(), _ptr(x), _ptr(stats), _ptr(gamma), _ptr(beta), _ptr(out),
                                    B, H, W, Ho, Wo, C_, int(accumulate)))
    return out


def gn_relu_upsample_sum(terms, gamma, beta, size, out=None, proj=None, keep_sum=True):
    """((t0 + t1) + t2) with t_k = bilinear(relu(gn(x_k))) for terms = [(x_k, stats_k), ...] (at most 3) in one pass.
    proj = (w16, bias, cout[, out1]): also returns the 1x1 convolution of the sum (cout <= 8, weights packed by pack_small), computed
    from registers; with keep_sum=False the sum itself is never written and only the projection is returned."""
    n = len(terms)
    xs = [as_nhwc(x) for x, _ in terms]             # a term may be a channel slice of a wider NHWC tensor (ld > C)
    B, C_ = xs[0][0].shape[:2]
    for (x, ld) in xs:
        assert ld >= C_ and ld % 4 == 0 and x.shape[0] == B and x.shape[1] == C_
    Ho, Wo = size
    dev = xs[0][0].device
    if out is None and (keep_sum or proj is None):
        out = new_act(B, C_, Ho, Wo, dev)
    vp_arr, i_arr = C.c_void_p * n, C.c_int * n
    head = (_stream(), n, vp_arr(*[_ptr(x) for x, _ in xs]), vp_arr(*[_ptr(st) for _, st in terms]),
            i_arr(*[x.shape[2] for x, _ in xs]), i_arr(*[x.shape[3] for x, _ in xs]), i_arr(*[ld for _, ld in xs]),
            _ptr(gamma), _ptr(beta))
    if proj is None:
        check(lib().lm_gn_relu_upsample_sum(*head, _ptr(out), B, Ho, Wo, C_))
        return out
    w16, bias, cout = proj[:3]
    out1 = proj[3] if len(proj) > 3 and proj[3] is not None else new_act(B, cout, Ho, Wo, dev)
    o1, ldy1 = as_nhwc(out1)
    assert o1.data_ptr() == out1.data_ptr()
    check(lib().lm_gn_relu_upsample_sum_conv1x1(*head, _ptr(out) if keep_sum else None, B, Ho, Wo, C_, _ptr(w16), _ptr(bias), cout,
                                                _ptr(out1), ldy1))
    return (out, out1) if keep_sum else out1


def upsample_nhwc(x, size, add=None, out=None):
    x, ldx = as_nhwc(x)
    B, C_, H, W = x.shape
    Ho, Wo = size
    if out is None and add is None and (Ho, Wo) == (H, W):
        return x      # align_corners=True bilinear to the same size is the identity (source coordinate == destination, weight 1)
    if out is None:
        out = new_act(B, C_, Ho, Wo, x.device)
    out_, ldy = as_nhwc(out)
    assert out_.data_ptr() == out.data_ptr()
    lda = 0
    if add is not None:
        add, lda = as_nhwc(add)
    check(lib().lm_upsample_bilinear_nhwc(_stream(), _ptr(x), ldx, _ptr(add), lda, _ptr(out), ldy, B, H, W, Ho, Wo, C_))
    return out


def pack_head_endpoint(conv1, bn, conv2):
    """The `endpoint` stack of ColumnProposal2 (Conv2d(17, 4, 3) - ReLU - BatchNorm2d(4) - Conv2d(4, 1, 3)) -> the operands of
    lm_head_endpoint: (w1p [17][3][3][4], b1 [4], bn scale [4], bn shift [4], w2 [4][3][3], b2 [1]).  The BatchNorm stays a scale and a
    shift of its own: it sits between a ReLU and a zero-padded convolution, so its shift must not reach the padding."""
    s, beta = fold_bn(bn)
    return (conv1.weight.permute(1, 2, 3, 0).float().contiguous(), conv1.bias.float().contiguous(), s, beta,
            conv2.weight[0].float().contiguous(), conv2.bias.float().contiguous())


def head_endpoint_tile():
    return int(lib().lm_head_endpoint_tile())


def head_endpoint(col, x_endp, packed, out=None):
    """col [B,16,h,w] NHWC-stored (a channel slice of a wider buffer is fine), x_endp [B,1,H,W], packed = pack_head_endpoint(...)
    -> the endpoint logits [B,1,H,W] of heads.endp_mode = 'endpoint', one fused kernel (csrc/head_endpoint.hip)."""
    col_, ldc = as_nhwc(col)
    B, C_, h, w = col_.shape
    assert C_ == 16, 'head_endpoint: col has 16 channels'
    x_endp = x_endp.contiguous()
    assert x_endp.dim() == 4 and x_endp.shape[0] == B and x_endp.shape[1] == 1 and x_endp.dtype == torch.float32
    H, W = x_endp.shape[2:]
    if out is None:
        out = torch.empty((B, 1, H, W), device=col.device, dtype=torch.float32)
    w1p, b1, s, beta, w2, b2 = packed
    assert w1p.numel() == 17 * 36 and w2.numel() == 36
    check(lib().lm_head_endpoint(_stream(), _ptr(col_), ldc, _ptr(x_endp), _ptr(w1p), _ptr(b1), _ptr(s), _ptr(beta), _ptr(w2), _ptr(b2),
                                 _ptr(out), B, h, w, H, W))
    return out


def upsample_to_chw(x, size):
    x, ldx = as_nhwc(x)
    B, C_, H, W = x.shape
    Ho, Wo = size
    out = torch.empty((B, C_, Ho, Wo), device=x.device, dtype=torch.float32)
    check(lib().lm_upsample_bilinear_to_chw(_stream(), _ptr(x), ldx, _ptr(out), B, H, W, Ho, Wo, C_))
    return out


def layernorm(x2d, gamma, beta, eps=1e-5):
    assert x2d.is_contiguous()
    out = torch.empty_like(x2d)
    check(lib().lm_layernorm_rows(_stream(), _ptr(x2d), _ptr(gamma), _ptr(beta), _ptr(out), x2d.shape[0], x2d.shape[1], eps))
    return out


def unpatchify(tokens, B, G, P, C_):
    out = new_act(B, C_, G * P, G * P, tokens.device)
    check(lib().lm_unpatchify(_stream(), _ptr(tokens.contiguous()), _ptr(out), B, G, P, C_))
    return out


def attention(qkv, B, N, heads, dim_head, scale, valid=None):
    """valid (optional, [B, N] int32 on the device, N <= 64): per batch element only the flagged tokens are keys (compacted in token
    order: the arithmetic of a call on those tokens alone); every token still gets an output row."""
    assert qkv.is_contiguous()
    out = torch.empty((B * N, heads * dim_head), device=qkv.device, dtype=torch.float32)
    if valid is None:
        check(lib().lm_attention_f32(_stream(), _ptr(qkv), _ptr(out), B, N, heads, dim_head, float(scale)))
    else:
        assert valid.dtype == torch.int32 and valid.is_contiguous() and tuple(valid.shape) == (B, N)
        check(lib().lm_attention_masked_f32(_stream(), _ptr(qkv), _ptr(out), _ptr(valid), B, N, heads, dim_head, float(scale)))
    return out


# ------------------------------------------------------------------------------- head
def head_tokens(seg, row, P, prop_width, half_buff, seg_bias):
    """seg [B,1,288,288], row [B,16,144,144] (NHWC-stored) -> tok [B*P*144, 16*FW], FW = prop_width + 2*half_buff (10, 12 or 16).
    seg None: spatial_att=False, the tokens are the raw row windows."""
    row, ld = as_nhwc(row)
    B, C_, Hr, Wr = row.shape
    assert C_ == 16 and ld == 16
    tok = torch.empty((B * P * Hr, 16 * (prop_width + 2 * half_buff)), device=row.device, dtype=torch.float32)
    if seg is None:
        check(lib().lm_head_tokens_window(_stream(), _ptr(row), _ptr(tok), B, P, Hr, Wr, prop_width, half_buff))
        return tok
    seg = seg.reshape(B, 2 * Hr, 2 * Wr).contiguous()
    check(lib().lm_head_tokens(_stream(), _ptr(seg), _ptr(row), _ptr(tok), float(seg_bias), B, P, Hr, Wr, prop_width, half_buff))
    return tok


def head_stage2(hid, D, w2, b2, B, P, R, w_small=None):
    """Second Conv1d of ext2 / cls2 / offset2 on the hidden rows hid [M, >= 3D] (ext | cls | off, D each): w2 [3 + 2 FW, D], b2 [3 + 2 FW]
    -> ext2 [B,P,R,3], cls2 / off2 [B,P,R,FW].  FW = 10: lm_head_stage2.  Other widths: w_small = the three branches' weights packed by
    pack_small, each branch one 1x1 lm_conv2d_nhwc_small over its slice of the hidden rows (row pitch hid.stride(0), bias as shift)."""
    M = hid.shape[0]
    FW = (w2.shape[0] - 3) // 2
    assert w2.shape == (3 + 2 * FW, D) and b2.numel() == 3 + 2 * FW and hid.shape[1] >= 3 * D and hid.stride(1) == 1
    ext2 = torch.empty((B, P, R, 3), device=hid.device, dtype=torch.float32)
    cls2 = torch.empty((B, P, R, FW), device=hid.device, dtype=torch.float32)
    off2 = torch.empty((B, P, R, FW), device=hid.device, dtype=torch.float32)
    if FW == 10:
        check(lib().lm_head_stage2(_stream(), _ptr(hid), hid.stride(0), D, _ptr(w2), _ptr(b2), _ptr(ext2), _ptr(cls2), _ptr(off2), M))
        return ext2, cls2, off2
    if w_small is None:
        raise ValueError(f'head_stage2: prop_fea_width {FW} runs through lm_conv2d_nhwc_small and needs the pack_small weights')
    bounds = (0, 3, 3 + FW, 3 + 2 * FW)
    for br, (y, w16) in enumerate(zip((ext2, cls2, off2), w_small)):
        n = bounds[br + 1] - bounds[br]
        assert tuple(w16.shape) == (1, D, 16)
        x = hid[:, br * D:(br + 1) * D]
        shift = b2[bounds[br]:bounds[br + 1]]
        check(lib().lm_conv2d_nhwc_small(_stream(), _ptr(x), hid.stride(0), _ptr(w16), None, _ptr(shift), _ptr(y), n,
                                         1, 1, M, D, n, 1, 1, 1, 0, 0, 0, ACT_NONE))
    return ext2, cls2, off2


def head_proposal_conf(tok, wt, bias, B, P):
    L = tok.numel() // (B * P)
    conf = torch.empty((B, P, 2), device=tok.device, dtype=torch.float32)
    check(lib().lm_head_proposal_conf(_stream(), _ptr(tok), _ptr(wt), _ptr(bias), _ptr(conf), B * P, L))
    return conf


# ------------------------------------------------------------------------------- decode
def pack_readback(tensors, block=None):
    """Gather device tensors (contiguous, byte sizes multiples of 4) into ONE uint8 device block at 256-byte aligned offsets
    (lm_pack_segments); returns (block, [(offset, nbytes)]).  The pipeline then moves a batch's decode outputs to the host with one copy."""
    offs, sizes, off = [], [], 0
    for t in tensors:
        assert t.is_contiguous()
        nb = t.numel() * t.element_size()
        assert nb % 4 == 0, 'lm_pack_segments copies 4-byte words'
        off = (off + 255) // 256 * 256
        offs.append(off); sizes.append(nb)
        off += nb
    if block is None or block.numel() < off or block.device != tensors[0].device:
        block = torch.empty(max(off, 1), device=tensors[0].device, dtype=torch.uint8)
    n = len(tensors)
    src = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    nby = (C.c_long * n)(*sizes)
    dof = (C.c_long * n)(*offs)
    check(lib().lm_pack_segments(_stream(), n, src, nby, dof, _ptr(block)))
    return block, list(zip(offs, sizes))


def decode_proposals(pconf, ext2, cls2, off2, exist_thre, prop_width, half_buff):
    B, P, R, FW = cls2.shape
    assert FW == prop_width + 2 * half_buff and off2.shape[-1] == FW, 'cls2 / offset2 are prop_fea_width wide'
    dev = cls2.device
    prop_conf = torch.empty((B, P, 2), device=dev, dtype=torch.float32)
    v_ext = torch.empty((B, P, R), device=dev, dtype=torch.float32)
    cls_conf = torch.empty((B, P, R, FW), device=dev, dtype=torch.float32)
    cls_idx = torch.empty((B, P, R), device=dev, dtype=torch.int32)
    cls_offset = torch.empty((B, P, R), device=dev, dtype=torch.float64)
    check(lib().lm_decode_proposals(_stream(), _ptr(pconf.contiguous()), _ptr(ext2.contiguous()), _ptr(cls2.contiguous()),
                                    _ptr(off2.contiguous()), _ptr(prop_conf), _ptr(v_ext), _ptr(cls_conf), _ptr(cls_idx),
                                    _ptr(cls_offset), B, P, R, float(exist_thre), prop_width, half_buff))
    return prop_conf, v_ext, cls_conf, cls_idx, cls_offset


def decode_orient(orient_logits):
    x, ld = as_nhwc(orient_logits)
    B, C_, H, W = x.shape
    out = torch.empty((B, H, W), device=x.device, dtype=torch.uint8)
    check(lib().lm_decode_orient(_stream(), _ptr(x), ld, C_, _ptr(out), B * H * W))
    return out


def decode_semantic(logits_chw, thre, raw_mode=False, want_biseg=True):
    x = logits_chw.contiguous()
    B, C_, H, W = x.shape
    assert C_ == 3
    sem = torch.empty((B, H, W), device=x.device, dtype=torch.uint8)
    biseg = rows = None
    if want_biseg:
        biseg = torch.empty((B, H, W), device=x.device, dtype=torch.float32)
        rows = torch.empty((B, H // 8, W), device=x.device, dtype=torch.float32)
    check(lib().lm_decode_semantic(_stream(), _ptr(x), _ptr(sem), _ptr(biseg), _ptr(rows), B, H, W, float(thre), int(raw_mode)))
    return sem, biseg, rows


def endp_topk(endp_logits, K=512, clip=20):
    x = endp_logits.contiguous()
    B, C_, H, W = x.shape
    assert C_ == 1
    ws = torch.empty(lib().lm_endp_topk_workspace_bytes(B), device=x.device, dtype=torch.uint8)
    idx = torch.empty((B, K), device=x.device, dtype=torch.int32)
    score = torch.empty((B, K), device=x.device, dtype=torch.float32)
    status = torch.empty((B,), device=x.device, dtype=torch.int32)
    check(lib().lm_endp_topk(_stream(), _ptr(x), _ptr(ws), _ptr(idx), _ptr(score), _ptr(status), B, H, W, clip, K))
    return idx, score, status


# ------------------------------------------------------------------------------- raster / ingest
def make_raster_params(quat=(1, 0, 0, 0), trans=(0, 0, 0), bev_img_offset=(0, 0), img_reso=(0.05, 0.05),
                       local_min_ele=0.0, ele_reso=0.05, inten_lo=800.0, inten_hi=33000.0):
    p = LmRasterParams()
    p.quat[:] = [float(v) for v in quat]
    p.trans[:] = [float(v) for v in trans]
    p.bev_img_offset[:] = [float(v) for v in bev_img_offset]
    p.img_reso[:] = [float(v) for v in img_reso]
    p.local_min_ele, p.ele_reso, p.inten_lo, p.inten_hi = float(local_min_ele), float(ele_reso), float(inten_lo), float(inten_hi)
    return p


_raster_ws = {}


def _workspace(points, need):
    """The scratch buffer of the raster section: one per (device, stream), grown and never shrunk."""
    key = (points.device, _stream().value)
    ws = _raster_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _raster_ws[key] = torch.empty(need, device=points.device, dtype=torch.uint8)
    return ws


def _tile_range_args(who, points, tile_offsets, params):
    """The (points, tile_offsets, params) triple of bev_raster_batch, checked -> (B, offsets as C longs, params as a C array)."""
    if not points.is_cuda:
        _ptr(points)
    assert points.dim() == 2 and points.shape[1] == 4 and points.is_contiguous() and points.dtype == torch.float32
    B = len(params)
    if len(tile_offsets) != B + 1:
        raise ValueError(f'{who}: {len(tile_offsets)} tile_offsets for {B} tiles (B + 1 are needed)')
    offs = (C.c_long * (B + 1))(*[int(o) for o in tile_offsets])
    if B and offs[B] > points.shape[0]:
        raise ValueError(f'{who}: tile_offsets end at {offs[B]}, points has {points.shape[0]} rows')
    return B, offs, (LmRasterParams * B)(*params)


def bev_raster_batch(points, tile_offsets, params, H=1152, W=1152, out=None, want_u8=False, u8_only=False, out_u8=None, inten_scale=None):
    """points [sum N,4] f32 (x,y,z,raw intensity) on device, tile_offsets: B+1 ints, params: list of LmRasterParams
    -> proj [B,3,H,W] f32 (= u8/255), optional u8 [B,H,W,3].  u8_only: only the u8 HWC tile is written (the stem takes it
    directly, ops.stem) - a quarter of the output bytes.
    inten_scale: a sequence of B floats (None or an entry <= 0: the derived 255 / inten_hi): the tile's intensity channel becomes
    I = clamp(floor((clip(i, inten_lo, inten_hi) - inten_lo) * scale + .5), 1, 255) (lm_bev_raster_batch_scaled)."""
    assert points.dim() == 2 and points.shape[1] == 4 and points.is_contiguous() and points.dtype == torch.float32
    B = len(params)
    assert len(tile_offsets) == B + 1
    offs = (C.c_long * (B + 1))(*[int(o) for o in tile_offsets])
    par = (LmRasterParams * B)(*params)
    cap = max([offs[b + 1] - offs[b] for b in range(B)] + [0])
    ws = _workspace(points, lib().lm_bev_raster_workspace_bytes(B, cap, H, W))
    want_u8 = want_u8 or u8_only or out_u8 is not None
    if out is None and not u8_only:
        out = torch.empty((B, 3, H, W), device=points.device, dtype=torch.float32)
    u8 = None
    if want_u8:
        u8 = out_u8 if out_u8 is not None else torch.empty((B, H, W, 3), device=points.device, dtype=torch.uint8)
        assert u8.dtype == torch.uint8 and u8.is_contiguous() and tuple(u8.shape) == (B, H, W, 3)
    if inten_scale is None:
        check(lib().lm_bev_raster_batch(_stream(), _ptr(points) if points.numel() else None, offs, par, B, _ptr(ws), ws.numel(),
                                        None if u8_only else _ptr(out), _ptr(u8), H, W))
    else:
        if len(inten_scale) != B:
            raise ValueError(f'bev_raster_batch: {len(inten_scale)} inten_scale entries for {B} tiles')
        scale = (C.c_float * B)(*[0.0 if v is None else float(v) for v in inten_scale])
        check(lib().lm_bev_raster_batch_scaled(_stream(), _ptr(points) if points.numel() else None, offs, par, B, _ptr(ws), ws.numel(),
                                               None if u8_only else _ptr(out), _ptr(u8), H, W, scale))
    if u8_only:
        return u8
    return (out, u8) if want_u8 else out


def bev_raster(points, params, H=1152, W=1152, want_u8=False):
    """Single tile convenience wrapper: points [N,4] -> proj [3,H,W] (and u8 [H,W,3])."""
    r = bev_raster_batch(points, [0, points.shape[0]], [params], H, W, want_u8=want_u8)
    return (r[0][0], r[1][0]) if want_u8 else r[0]


def strip_grid(params, H=1152, W=1152, z_range=None):
    """The host-built point-to-tile grid behind strip_bin_points (no GPU): -> (dict x0, y0, cell, nx, ny; cells [ny, nx, 8] uint16
    numpy array of tile indices, 0xFFFF = none).  Raises LanemapHipError when more than 8 tiles touch one cell: the limit counts the tiles
    whose window reaches into a cell (cells are halved up to three times first), not the tiles a single point can lie in."""
    import numpy as np
    T = len(params)
    par = (LmRasterParams * T)(*params)
    z_lo, z_hi = (float(z_range[0]), float(z_range[1])) if z_range is not None else (-math.inf, math.inf)
    g = LmStripGrid()
    check(lib().lm_strip_build_grid(par, T, H, W, z_lo, z_hi, C.byref(g), None, 0))
    cells = np.empty((g.ny, g.nx, 8), dtype=np.uint16)
    check(lib().lm_strip_build_grid(par, T, H, W, z_lo, z_hi, C.byref(g), C.c_void_p(cells.ctypes.data), g.nx * g.ny))
    return {'x0': g.x0, 'y0': g.y0, 'cell': g.cell, 'nx': g.nx, 'ny': g.ny}, cells


class LineIndex:
    """The segment table of las_io.line_segments with its lookup grid (lm_line_index_build), on the device: what label_points and
    las_io.label_records take.  segments [S,8] f32, cell_start [nx ny + 1] and cell_segs [n_entries] int32 are device tensors; grid is
    the host LmLineGrid; half_width the float32 half width the lists were built for; n_lines the largest line a segment carries."""

    def __init__(self, segments, cell_start, cell_segs, grid, half_width):
        self.segments, self.cell_start, self.cell_segs, self.grid, self.half_width = segments, cell_start, cell_segs, grid, half_width
        self.n_segments, self.n_lines = int(segments.shape[0]), int(grid.max_line)

    def args(self):
        """-> the (segments, S, grid, cell_start, cell_segs, half_width) run of arguments of the two device entries."""
        S = self.n_segments
        return (_ptr(self.segments) if S else None, S, C.byref(self.grid), _ptr(self.cell_start) if S else None,
                _ptr(self.cell_segs) if S else None, float(self.half_width))


def line_index_host(segments, half_width, cell=None):
    """lm_line_index_build on the host (no GPU): segments [S,8] float32 numpy (las_io.line_segments) -> (LmLineGrid, cell_start
    [nx ny + 1] int32, cell_segs [n_entries] int32).  cell: the cell size in metres; None: max(1 m, 2 half_width).  The two-call protocol:
    the first call sizes the lists, the second fills them."""
    import numpy as np
    seg = np.ascontiguousarray(segments, dtype=np.float32)
    if seg.ndim != 2 or seg.shape[1] != 8:
        raise ValueError(f'line_index: segments must be [S,8] float32 (las_io.line_segments), not {seg.shape}')
    S, g = int(seg.shape[0]), LmLineGrid()
    if cell is not None and not float(cell) > 0.0:
        raise ValueError(f'line_index: cell={cell!r} must be a size > 0 (None: the default)')
    cell = 0.0 if cell is None else float(cell)                              # (0: the entry's default)
    sp = C.c_void_p(seg.ctypes.data) if S else None
    check(lib().lm_line_index_build(sp, S, float(half_width), cell, C.byref(g), None, 0, None, 0))
    cell_start = np.zeros(g.nx * g.ny + 1, dtype=np.int32)
    cell_segs = np.zeros(max(int(g.n_entries), 1), dtype=np.int32)
    check(lib().lm_line_index_build(sp, S, float(half_width), cell, C.byref(g), C.c_void_p(cell_start.ctypes.data), cell_start.size,
                                    C.c_void_p(cell_segs.ctypes.data), cell_segs.size))
    return g, cell_start, cell_segs[:int(g.n_entries)]


def line_index(segments, half_width, cell=None, device='cuda:0'):
    """segments [S,8] float32 numpy (las_io.line_segments) -> a LineIndex on `device`: the table and the grid's lists uploaded once, to
    label any number of clouds with.  cell: see line_index_host; it changes the cost of a lookup, never a label."""
    import numpy as np
    seg = np.ascontiguousarray(segments, dtype=np.float32)
    g, cell_start, cell_segs = line_index_host(seg, half_width, cell)
    device = torch.device(device)
    if device.type != 'cuda':
        raise LanemapHipError('lanemapping_amd ops need tensors on an MI355X (HIP) device; no CPU fallback exists')
    up = lambda a: torch.from_numpy(np.array(a, order='C', copy=True)).to(device)      # (a copy: the caller's array may be read-only)
    return LineIndex(up(seg), up(cell_start), up(cell_segs), g, np.float32(half_width))


def _line_args(who, points, index, *stations):
    """The argument checks of label_points, line_profile, line_cross and line_hist: points [N,4] float32, contiguous, on the device; index an
    ops.LineIndex; stations (passed where the entry takes them) the ops.LineStations of the same segments."""
    if not points.is_cuda:
        raise LanemapHipError('lanemapping_amd ops need tensors on an MI355X (HIP) device; no CPU fallback exists')
    assert points.dim() == 2 and points.shape[1] == 4 and points.is_contiguous() and points.dtype == torch.float32
    if not isinstance(index, LineIndex):
        raise TypeError(f'{who}: index must be an ops.LineIndex (ops.line_index), not {type(index).__name__}')
    for st in stations:
        if not isinstance(st, LineStations):
            raise TypeError(f'{who}: stations must be an ops.LineStations (ops.line_stations), not {type(st).__name__}')
        if st.n_segments != index.n_segments:
            raise ValueError(f'{who}: stations hold {st.n_segments} rows, the index {index.n_segments} segments')


def _table_out(who, shape, out, device):
    """-> `out` after its check, or a new int64 tensor of `shape` on `device`: the table an accumulating entry writes."""
    if out is None:
        return torch.empty(shape, device=device, dtype=torch.int64)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.int64 or not out.is_contiguous() or out.device != device:
        raise ValueError(f'{who}: out must be a contiguous [{",".join(str(v) for v in shape)}] int64 tensor on {device}')
    return out


def label_points(points, index, z_tol, min_intensity=None, want_dist2=False):
    """points [N,4] f32 on device (x, y, z, intensity in the frame of the index' segments) -> line [N] int32: 0, or the number (from 1) of
    the line whose band the point lies in, the nearest winning (the rule: include/lanemap_hip.h).  want_dist2: -> (line, dist2 [N] f32),
    the squared horizontal distance to the winner, +inf without one.  No synchronisation."""
    _line_args('label_points', points, index)
    N = int(points.shape[0])
    line = torch.empty((N,), device=points.device, dtype=torch.int32)
    dist2 = torch.empty((N,), device=points.device, dtype=torch.float32) if want_dist2 else None
    mi = math.nan if min_intensity is None else float(min_intensity)
    check(lib().lm_label_points(_stream(), _ptr(points) if N else None, N, *index.args(), float(z_tol), mi, _ptr(line) if N else None,
                                _ptr(dist2) if (want_dist2 and N) else None))
    return (line, dist2) if want_dist2 else line


class LineStations:
    """The station table of las_io.line_stations on the device, beside the LineIndex of the same segments: what line_profile and
    las_io.profile_records take.  stations [S,4] f32 and bin_start [L + 1] int32 are device tensors; bin_start_host the same table as a
    numpy array (the entries check it on the host); bin the bin length in metres; n_lines = L, n_bins = bin_start[L]."""

    def __init__(self, stations, bin_start, bin_start_host, bin):
        self.stations, self.bin_start, self.bin_start_host, self.bin = stations, bin_start, bin_start_host, float(bin)
        self.n_segments, self.n_lines, self.n_bins = int(stations.shape[0]), int(bin_start_host.shape[0]) - 1, int(bin_start_host[-1])

    def args(self):
        """-> the (stations, bin_start, bin_start_host, L, bin) run of arguments of the two device entries."""
        return (_ptr(self.stations) if self.n_segments else None, _ptr(self.bin_start), C.c_void_p(self.bin_start_host.ctypes.data),
                self.n_lines, self.bin)

    def new_bins(self):
        """-> an uninitialised [n_bins, 6] int64 tensor on the tables' device."""
        return torch.empty((self.n_bins, 6), device=self.bin_start.device, dtype=torch.int64)


def line_stations(stations, bin_start, bin, device='cuda:0'):
    """(stations [S,4] float32, bin_start [L + 1] int32) numpy, as las_io.line_stations(lines, shift, bin) returns them -> a LineStations
    on `device`, uploaded once to profile any number of clouds with."""
    import numpy as np
    st = np.ascontiguousarray(stations, dtype=np.float32)
    bs = np.array(bin_start, dtype=np.int32, order='C', copy=True)
    if st.ndim != 2 or st.shape[1] != 4 or bs.ndim != 1 or bs.shape[0] < 1:
        raise ValueError(f'line_stations: stations must be [S,4] float32 and bin_start [L + 1] int32, not {st.shape} and {bs.shape}')
    if not (math.isfinite(float(bin)) and float(bin) > 0.0):
        raise ValueError(f'line_stations: bin={bin!r} must be a finite length > 0')
    device = torch.device(device)
    if device.type != 'cuda':
        raise LanemapHipError('lanemapping_amd ops need tensors on an MI355X (HIP) device; no CPU fallback exists')
    return LineStations(torch.from_numpy(st.copy()).to(device), torch.from_numpy(bs).to(device), bs, bin)


class PaintRows:
    """A paint table (las_io.PaintTable: a threshold per station window of every line) on the device, beside the station table of the
    segments it is looked up with: what the _local entries take in place of a min_intensity (the rule: include/lanemap_hip.h).  thr [R]
    f32, paint_iq [R] int32 (the cross-sections' integer of every row) and win_start [L + 1] int32 are device tensors, win_start_host
    the same table as a numpy array, stations the [S,4] f32 device tensor of an ops.LineStations of the same segments, window the window
    length in metres; thr_min = min(thr), the pre-filter that lets a wave of asphalt leave before the search (0 without rows)."""

    def __init__(self, thr, paint_iq, win_start, win_start_host, stations, window, thr_min):
        self.thr, self.paint_iq, self.win_start, self.win_start_host, self.stations = thr, paint_iq, win_start, win_start_host, stations
        self.window, self.thr_min = float(window), float(thr_min)
        self.n_lines, self.n_rows, self.n_segments = int(win_start_host.shape[0]) - 1, int(win_start_host[-1]), int(stations.shape[0])

    def struct(self, cross=False):
        """-> the LmPaintTable of one call: the cross-section entry reads paint_iq and no thr, the others thr and no paint_iq."""
        t = LmPaintTable()
        p = lambda x, on: x.data_ptr() if on and x.numel() else None
        t.thr, t.paint_iq = p(self.thr, not cross), p(self.paint_iq, cross)
        t.win_start, t.win_start_host = self.win_start.data_ptr(), self.win_start_host.ctypes.data
        t.stations, t.window, t.thr_min, t.n_rows = p(self.stations, True), self.window, self.thr_min, self.n_rows
        t.rows = self                                                       # (the struct holds addresses: the tensors live as long as it)
        return t


def paint_rows(thr, win_start, window, stations, paint_iq=None):
    """(thr [R] float32, win_start [L + 1] int32) numpy, as a las_io.PaintTable holds them, the window length and the [S,4] f32 device
    tensor of the station table (ops.LineStations.stations) -> a PaintRows on that tensor's device.  paint_iq: [R] int32 numpy, the
    cross-sections' integer per row; None: not uploaded (zeros)."""
    import numpy as np
    thr = np.ascontiguousarray(thr, dtype=np.float32)
    ws = np.array(win_start, dtype=np.int32, order='C', copy=True)
    if thr.ndim != 1 or ws.ndim != 1 or ws.shape[0] < 1 or int(ws[-1]) != thr.shape[0] or not np.isfinite(thr).all():
        raise ValueError(f'paint_rows: thr must be [R] finite float32 and win_start [L + 1] int32 ending in R, not {thr.shape} and {ws.shape}')
    if not (math.isfinite(float(window)) and float(window) > 0.0):
        raise ValueError(f'paint_rows: window={window!r} must be a finite length > 0')
    if not stations.is_cuda:
        raise LanemapHipError('lanemapping_amd ops need tensors on an MI355X (HIP) device; no CPU fallback exists')
    assert stations.dim() == 2 and stations.shape[1] == 4 and stations.is_contiguous() and stations.dtype == torch.float32
    dev = stations.device
    iq = np.zeros(thr.shape, np.int32) if paint_iq is None else np.ascontiguousarray(paint_iq, dtype=np.int32)
    if iq.shape != thr.shape or (iq < 0).any() or (iq > 65536).any():
        raise ValueError(f'paint_rows: paint_iq must be [R] int32 in 0 .. 65536, not {iq.shape}')
    return PaintRows(torch.from_numpy(thr.copy()).to(dev), torch.from_numpy(iq.copy()).to(dev), torch.from_numpy(ws).to(dev), ws, stations,
                     window, float(thr.min()) if thr.size else 0.0)


def line_profile(points, index, stations, z_tol, min_intensity=None, out=None):
    """points [N,4] f32 on device -> bins [n_bins, 6] int64 on device: per station bin of every line the columns n, sum iq, sum q,
    sum q^2, min q, max q over the points the labelling rule gives that line (the rule: include/lanemap_hip.h; q the lateral offset in
    1/1024 m, left positive; iq the intensity rounded into 0..65535); an empty bin reads 0, 0, 0, 0, 2^31 - 1, -2^31.  index: the
    ops.LineIndex, stations: the ops.LineStations of the same segments.  out: a bins tensor of an earlier call to add to.  Integer sums,
    minima and maxima only: the same bits whatever the order of the points.  No synchronisation."""
    _line_args('line_profile', points, index, stations)
    bins = _table_out('line_profile', (stations.n_bins, 6), out, points.device)
    N = int(points.shape[0])
    mi = math.nan if min_intensity is None else float(min_intensity)
    check(lib().lm_line_profile_points(_stream(), _ptr(points) if N else None, N, *index.args(), *stations.args(), float(z_tol), mi,
                                       int(out is not None), _ptr(bins) if stations.n_bins else None, stations.n_bins))
    return bins


def cross_cells(half_width, lateral_q):
    """-> (hq, nl) of the cross-section rule (include/lanemap_hip.h): hq = ceil(float32(half_width) * 1024) and the nl = 2 hq // lateral_q
    + 1 lateral cells of a station bin."""
    import numpy as np
    if isinstance(lateral_q, bool) or not isinstance(lateral_q, (int, np.integer)) or int(lateral_q) < 1:
        raise ValueError(f'cross_cells: lateral_q={lateral_q!r} must be a whole number >= 1 (the cell width in 1/1024 m)')
    hq = int(math.ceil(float(np.float32(half_width)) * 1024.0))
    return hq, 2 * hq // int(lateral_q) + 1


def line_cross(points, index, stations, z_tol, lateral_q, paint_iq, out=None):
    """points [N,4] f32 on device -> cells [n_bins, nl, 4] int64 on device: per station bin of every line a row of nl lateral cells, each
    n, n_paint, sum iq, sum zq over the returns the labelling rule gives that line without a min_intensity (the rule:
    include/lanemap_hip.h; cell c covers the offsets [(c lateral_q - hq) / 1024, ((c + 1) lateral_q - hq) / 1024) m, left positive; a
    return is paint when its intensity, rounded into 0..65535, is at least paint_iq; zq its height above the line in 1/1024 m); an empty
    cell reads four zeros.  index: the ops.LineIndex, stations: the ops.LineStations of the same segments.  out: the cells of an earlier
    call to add to.  Integer sums only: the same bits whatever the order of the points.  No synchronisation."""
    _line_args('line_cross', points, index, stations)
    hq, nl = cross_cells(index.half_width, lateral_q)
    cells = _table_out('line_cross', (stations.n_bins, nl, 4), out, points.device)
    N, n_cells = int(points.shape[0]), stations.n_bins * nl
    check(lib().lm_line_cross_points(_stream(), _ptr(points) if N else None, N, *index.args(), *stations.args(), float(z_tol), int(lateral_q),
                                     int(paint_iq), int(out is not None), _ptr(cells) if n_cells else None, n_cells))
    return cells


def hist_shape(half_width, ring_q, bin_shift):
    """-> (hq, Z, NB) of the histogram rule (include/lanemap_hip.h): hq = ceil(float32(half_width) * 1024), the Z = hq // ring_q + 1 lateral
    rings of a line and the NB = 65536 >> bin_shift counts of a histogram."""
    import numpy as np
    whole = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer))
    if not whole(ring_q) or int(ring_q) < 1:
        raise ValueError(f'hist_shape: ring_q={ring_q!r} must be a whole number >= 1 (the ring width in 1/1024 m)')
    if not whole(bin_shift) or not 0 <= int(bin_shift) <= 8:
        raise ValueError(f'hist_shape: bin_shift={bin_shift!r} must be a whole number in 0 .. 8')
    hq = int(math.ceil(float(np.float32(half_width)) * 1024.0))
    return hq, hq // int(ring_q) + 1, 65536 >> int(bin_shift)


def line_hist(points, index, stations, z_tol, ring_q, bin_shift, out=None):
    """points [N,4] f32 on device -> hist [L, Z, NB] int64 on device: per line and per lateral ring r = min(|q|, hq) // ring_q a histogram
    of iq >> bin_shift over the returns the labelling rule gives that line without a min_intensity (the rule: include/lanemap_hip.h; q the
    lateral offset in 1/1024 m, iq the intensity rounded into 0..65535).  index: the ops.LineIndex, stations: the ops.LineStations of the
    same segments (only their rlen column is read; L = stations.n_lines).  out: the table of an earlier call to add to.  Integer adds
    only: the same bits whatever the order of the points.  No synchronisation."""
    _line_args('line_hist', points, index, stations)
    hq, Z, NB = hist_shape(index.half_width, ring_q, bin_shift)
    L = stations.n_lines
    hist = _table_out('line_hist', (L, Z, NB), out, points.device)
    N, n_hist = int(points.shape[0]), L * Z * NB
    check(lib().lm_line_hist_points(_ptr(points) if N else None, N, *index.args(), stations.args()[0], L, float(z_tol), int(ring_q),
                                    int(bin_shift), int(out is not None), _ptr(hist) if n_hist else None, n_hist, _stream()))
    return hist


RESIDUE_MAX_SIDE, RESIDUE_MAX_CELLS = 1 << 20, 1 << 22
STATS_COLUMNS = ('n_cells', 'n_points', 'sum_iq', 'sum_cx', 'sum_cy', 'sum_cx2', 'sum_cxcy', 'sum_cy2', 'min_cx', 'max_cx', 'min_cy', 'max_cy')


def residue_grid(index, cell=0.1):
    """The host grid of the paint residue over the box of an ops.LineIndex (no GPU): -> dict x0, y0 (the index grid's float32 origin),
    cell (metres), nx, ny - enough cells to cover the index grid's box, so that every point the labelling rule can hit has a cell.  Refused:
    a cell that is no finite size > 0; nx or ny above 2^20 (a cell index must stay exact in float32)."""
    import numpy as np
    if not isinstance(index, LineIndex):
        raise TypeError(f'residue_grid: index must be an ops.LineIndex (ops.line_index), not {type(index).__name__}')
    if isinstance(cell, bool) or not isinstance(cell, (int, float, np.integer, np.floating)) or not (0.0 < float(cell) < math.inf):
        raise ValueError(f'residue_grid: cell={cell!r} must be a finite size > 0')
    cell, g = float(cell), index.grid
    inv = float(np.float32(1.0 / cell))
    # a point the index accepts has (x - x0) < nx_index * cell_index up to a few float32 roundings: 1e-6 relative and two cells cover them
    side = lambda n: int(math.floor(n * g.cell * inv * (1.0 + 1e-6))) + 2 if index.n_segments else 0
    nx, ny = side(g.nx), side(g.ny)
    if nx > RESIDUE_MAX_SIDE or ny > RESIDUE_MAX_SIDE:
        raise ValueError(f'residue_grid: nx={nx}, ny={ny} cells of {cell} m, at most 2^20 a side are supported (choose a larger cell)')
    return {'x0': float(np.float32(g.x0)), 'y0': float(np.float32(g.y0)), 'cell': cell, 'nx': nx, 'ny': ny}


def residue_keys(points, index, z_tol, min_intensity, clear, grid, want_iq=True):
    """points [N,4] f32 on device -> (key [N] int64, iq [N] int32 or None): the residue cell of every point on `grid` (residue_grid), -1
    where the point is no residue - not within the index' half_width (the reach) and z_tol of a line, below min_intensity, or within
    `clear` of its nearest line (the rule: include/lanemap_hip.h).  min_intensity: a number, or a PaintRows (paint_rows) of the same
    segments: the threshold of the return's own line and station window (lm_residue_keys_local).  No synchronisation."""
    if not points.is_cuda:
        raise LanemapHipError('lanemapping_amd ops need tensors on an MI355X (HIP) device; no CPU fallback exists')
    assert points.dim() == 2 and points.shape[1] == 4 and points.is_contiguous() and points.dtype == torch.float32
    if not isinstance(index, LineIndex):
        raise TypeError(f'residue_keys: index must be an ops.LineIndex (ops.line_index), not {type(index).__name__}')
    N = int(points.shape[0])
    key = torch.empty((N,), device=points.device, dtype=torch.int64)
    iq = torch.empty((N,), device=points.device, dtype=torch.int32) if want_iq else None
    tail = (float(clear), float(grid['cell']), int(grid['nx']), int(grid['ny']), _ptr(key) if N else None, _ptr(iq) if (want_iq and N) else None)
    if isinstance(min_intensity, PaintRows):
        if min_intensity.n_segments != index.n_segments:
            raise ValueError(f'residue_keys: the paint table looks rows up in {min_intensity.n_segments} station rows, the index holds '
                             f'{index.n_segments} segments')
        table = min_intensity.struct()
        check(lib().lm_residue_keys_local(_ptr(points) if N else None, N, *index.args(), float(z_tol), C.byref(table), min_intensity.n_lines,
                                          *tail, _stream()))
    else:
        check(lib().lm_residue_keys(_stream(), _ptr(points) if N else None, N, *index.args(), float(z_tol), float(min_intensity), *tail))
    return key, iq


def cell_components(keys, nx, ny, connectivity=8):
    """keys [M] int64 on device, ascending and distinct cells cy * nx + cx of an nx x ny grid -> (root [M] int32, err [1] int32):
    root[m] the smallest index of the cells connected with cell m under 4- or 8-connectivity on (cx, cy); err non-zero when a loop of
    the union-find ran into its cap (a bug, never a hang).  No synchronisation."""
    if not keys.is_cuda:
        raise LanemapHipError('lanemapping_amd ops need tensors on an MI355X (HIP) device; no CPU fallback exists')
    assert keys.dim() == 1 and keys.is_contiguous() and keys.dtype == torch.int64
    M = int(keys.shape[0])
    root = torch.empty((M,), device=keys.device, dtype=torch.int32)
    err = torch.empty((1,), device=keys.device, dtype=torch.int32)
    check(lib().lm_cell_components(_stream(), _ptr(keys) if M else None, M, int(nx), int(ny), int(connectivity), _ptr(root) if M else None,
                                   _ptr(err)))
    return root, err


def residue_stats(comp, keys, nx, ny, cell_points, cell_iq, K):
    """comp [M] int32 (dense component ids 0 .. K-1), keys [M] int64, cell_points and cell_iq [M] int64 on device -> stats [K,12] int64,
    the columns STATS_COLUMNS: cells, points and summed iq of every component, the first and second moments and the extents of its
    cells (each cell once).  Integer sums, minima and maxima only.  No synchronisation."""
    if not keys.is_cuda:
        raise LanemapHipError('lanemapping_amd ops need tensors on an MI355X (HIP) device; no CPU fallback exists')
    M = int(keys.shape[0])
    for t, dt in ((comp, torch.int32), (keys, torch.int64), (cell_points, torch.int64), (cell_iq, torch.int64)):
        assert t.dim() == 1 and t.shape[0] == M and t.is_contiguous() and t.dtype == dt and t.device == keys.device
    stats = torch.empty((int(K), 12), device=keys.device, dtype=torch.int64)
    p = lambda t: _ptr(t) if M else None
    check(lib().lm_residue_stats(_stream(), p(comp), p(keys), int(nx), int(ny), p(cell_points), p(cell_iq), M, int(K),
                                 _ptr(stats) if K else None))
    return stats


class ResidueBlobs:
    """What paint_residue returns: cells [M,2] int32 (cx, cy of the occupied cells, ascending in cy * nx + cx), comp [M] int32 (the blob
    of every cell, blobs numbered from 0 in the order of their first cell), stats [K,12] int64 (STATS_COLUMNS) and grid, the host dict of
    residue_grid.  numpy(): the same with numpy arrays (the one read-back of the results)."""

    def __init__(self, cells, comp, stats, grid):
        self.cells, self.comp, self.stats, self.grid = cells, comp, stats, grid

    def numpy(self):
        if not isinstance(self.cells, torch.Tensor):
            return self
        M = int(self.cells.shape[0])
        flat = torch.cat([self.cells.reshape(-1).to(torch.int64), self.comp.to(torch.int64), self.stats.reshape(-1)]).cpu().numpy()
        return ResidueBlobs(flat[:2 * M].reshape(M, 2).astype('int32'), flat[2 * M:3 * M].astype('int32'),
                            flat[3 * M:].reshape(-1, 12).copy(), dict(self.grid))


def paint_residue(clouds, index, z_tol, min_intensity, clear, cell=0.1, connectivity=8):
    """The paint no line explains.  clouds: a list of [N,4] f32 device tensors (x, y, z, raw intensity) in the frame of `index`, an
    ops.LineIndex built with half_width = the reach.  The residue points of all clouds (residue_keys) are put on one grid, the occupied
    cells are labelled into connected blobs (cell_components) and every blob gets its footprint statistics (residue_stats): -> a
    ResidueBlobs of device tensors.  The result does not depend on the order of the clouds or of their points.  The keys are compacted,
    made unique and counted with torch (an integer index_add_ sums iq per cell); the call itself reads one word back (the error word of
    the union-find, with M and K known from the shapes).  Refused: more than 2^22 occupied cells.  The per-point pass is bound by the
    candidate search: build the index with a cell well below 2 reach (las_io.residue_index_cell), the default cell of line_index is
    sized for the narrow band of the labelling."""
    if not isinstance(index, LineIndex):
        raise TypeError(f'paint_residue: index must be an ops.LineIndex (ops.line_index), not {type(index).__name__}')
    if connectivity not in (4, 8):
        raise ValueError(f'paint_residue: connectivity={connectivity!r} is neither 4 nor 8')
    grid = residue_grid(index, cell)
    dev = index.segments.device
    ks, qs = [torch.empty((0,), device=dev, dtype=torch.int64)], [torch.empty((0,), device=dev, dtype=torch.int64)]
    for pts in clouds:
        key, iq = residue_keys(pts, index, z_tol, min_intensity, clear, grid)
        on = key >= 0
        ks.append(key[on])
        qs.append(iq[on].to(torch.int64))
    keys, iqs = torch.cat(ks), torch.cat(qs)
    cells, inverse, counts = torch.unique(keys, sorted=True, return_inverse=True, return_counts=True)
    M = int(cells.shape[0])
    if M > RESIDUE_MAX_CELLS:
        raise LanemapHipError(f'paint_residue: {M} occupied cells of {grid["cell"]} m, at most 2^22 are supported: refusing to proceed '
                              '(raise min_intensity or choose a larger cell)')
    cell_iq = torch.zeros((M,), device=dev, dtype=torch.int64).index_add_(0, inverse, iqs)      # integer adds: the same bits every run
    nx, ny = grid['nx'], grid['ny']
    root, err = cell_components(cells, nx, ny, connectivity)
    roots, comp = torch.unique(root, sorted=True, return_inverse=True)                           # numbered in ascending root
    comp, K = comp.to(torch.int32), int(roots.shape[0])
    stats = residue_stats(comp, cells, nx, ny, counts, cell_iq, K)
    if int(err):
        raise LanemapHipError('paint_residue: the union-find of lm_cell_components ran into a loop cap (a bug: please report the input)')
    cxy = torch.stack([cells % max(nx, 1), cells // max(nx, 1)], dim=1).to(torch.int32)
    return ResidueBlobs(cxy, comp, stats, grid)


def _tilted(p):
    return p.quat[1] != 0.0 or p.quat[2] != 0.0


def _strip_cloud(points):
    """Both forms of the strip binning: a host tensor is refused (_ptr's message); -> whether it is a contiguous [N,4] float32 tensor."""
    if not points.is_cuda:
        _ptr(points)
    return points.dim() == 2 and points.shape[1] == 4 and points.is_contiguous() and points.dtype == torch.float32


def _strip_z(z_range, params):
    """Both forms of the strip binning: -> (z_lo, z_hi, ok); None is the whole axis; ok: the range is finite, or no tile is tilted."""
    z_lo, z_hi = (float(z_range[0]), float(z_range[1])) if z_range is not None else (-math.inf, math.inf)
    return z_lo, z_hi, (math.isfinite(z_lo) and math.isfinite(z_hi)) or not any(_tilted(p) for p in params)


def strip_bin_points(points, params, H=1152, W=1152, z_range=None, capacity=None):
    """points [N,4] f32 on device (one whole strip), params: list of T LmRasterParams -> (binned [sum counts, 4], offsets: T+1 host
    ints): the points of tile 0, then tile 1, ... in cloud order, exactly those the rasteriser keeps for each tile - the
    (points, tile_offsets) pair bev_raster_batch takes.  z_range = (lo, hi) of the cloud (the LAS header's) bounds the lookup grid of
    tilted tiles; None: taken from the points when a tile is tilted (one more pass and sync).  One device-to-host read of the offsets;
    if the first guess of the output size was short, one second call.  Not inside a graph capture (the entry refuses a capturing
    stream by name)."""
    ok = _strip_cloud(points)
    assert ok
    T, N = len(params), points.shape[0]
    par = (LmRasterParams * T)(*params)
    if z_range is None and N and any(_tilted(p) for p in params):
        z = points[:, 2]
        z = z[torch.isfinite(z)]
        z_range = (float(z.min()), float(z.max())) if z.numel() else (0.0, 0.0)
    z_lo, z_hi, ok = _strip_z(z_range, params)
    if not ok:
        if N:
            raise ValueError('strip_bin_points: tilted tiles need a finite z_range (or None: it is then taken from the points)')
        z_lo, z_hi = 0.0, 0.0                                                   # no points: any range will do
    need = lib().lm_strip_bin_workspace_bytes(N, T)
    if need <= 0:
        raise LanemapHipError(f'strip_bin_points: {T} tiles / {N} points are not supported (1 to 4096 tiles)')
    ws = _workspace(points, need)
    meta = torch.empty(2 * T + 1, device=points.device, dtype=torch.int64)        # counts [T] | offsets [T+1]
    offs = (C.c_long * (T + 1))()
    cap = int(capacity) if capacity is not None else N + N // 4
    binned = None
    for attempt in range(2):
        del binned                                                              # a retry must not hold both buffers
        binned = torch.empty((cap, 4), device=points.device, dtype=torch.float32)
        rc = lib().lm_strip_bin_points(_stream(), _ptr(points) if N else None, N, par, T, H, W, z_lo, z_hi, _ptr(ws), ws.numel(),
                                       C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 8 * T), offs, _ptr(binned) if cap else None, cap)
        if rc == 4 and attempt == 0 and capacity is None:                       # LM_ERR_CAPACITY: offs[T] is the size needed
            cap = int(offs[T])
            continue
        check(rc)
        break
    return binned[:offs[T]], [int(o) for o in offs]


class _StripPlan:
    """The layout constants of a run of tiles on the device (lm_strip_plan_create): the handle and the tensor it points into."""

    def __init__(self, params, H, W, z_lo, z_hi, device):
        T = len(params)
        par = (LmRasterParams * T)(*params)
        g = LmStripGrid()
        check(lib().lm_strip_build_grid(par, T, H, W, z_lo, z_hi, C.byref(g), None, 0))        # the geometry: how many cells
        need = int(lib().lm_strip_plan_consts_bytes(T, g.nx * g.ny))
        self.consts = torch.empty(need, device=device, dtype=torch.uint8)
        self.handle = C.c_void_p()
        self._destroy = lib().lm_strip_plan_destroy                                          # (bound now: __del__ may run at interpreter exit)
        check(lib().lm_strip_plan_create(par, T, H, W, z_lo, z_hi, _ptr(self.consts), need, C.byref(self.handle), _stream()))

    def __del__(self):
        if getattr(self, 'handle', None):
            self._destroy(self.handle)
            self.handle = None


class StripBinner:
    """strip_bin_points for a strip that arrives in chunks and is never held as one cloud (lm_strip_bin_count / lm_strip_bin_scatter).

        b = StripBinner(params, H, W, z_range, device)
        for every chunk:  b.count(points)                  pass A: the per-tile counts add up on the device
        counts = b.counts()                                the one read-back of pass A: int64 numpy [T]
        b.begin()  or  b.begin((t0, t1), capacity)         binned for all tiles, or for the consecutive tiles t0 .. t1 - 1 only
        for every chunk, in the same order:  b.scatter(points)
        binned, offsets = b.finish()                       the pair bev_raster_batch takes, for the tiles of begin()

    With the chunks of pass B those of pass A, (binned, offsets) are bit for bit what strip_bin_points returns for the chunks
    concatenated - for a run of tiles, what it returns for that sub-list of `params`.  begin() may be called again for another run.
    The lookup grid and the tile constants go to the device once per run of tiles (a plan), not once per chunk.  z_range as for
    strip_bin_points, but never taken from the points: tilted tiles need a finite one.  capacity: rows of binned (default: the run's
    total); a chunk that overruns it writes nothing outside binned, and finish() raises."""

    def __init__(self, params, H=1152, W=1152, z_range=None, device='cuda:0'):
        self.params, self.H, self.W, self.device = list(params), int(H), int(W), torch.device(device)
        if self.device.type != 'cuda':
            raise LanemapHipError('StripBinner needs an MI355X (HIP) device; no CPU fallback exists')
        z_lo, z_hi, ok = _strip_z(z_range, self.params)
        if not ok:
            raise ValueError('StripBinner: tilted tiles need a finite z_range')
        self.z = (z_lo, z_hi)
        T = len(self.params)
        self._plans = {}
        self._plan((0, T))                                                          # (a layout the grid refuses is refused here)
        self._counts = torch.zeros(T, device=self.device, dtype=torch.int64)
        self._host_counts = None
        self._ws = None
        self._run = None

    def _plan(self, tiles):
        if tiles not in self._plans:
            self._plans[tiles] = _StripPlan(self.params[tiles[0]:tiles[1]], self.H, self.W, *self.z, self.device)
        return self._plans[tiles]

    def _chunk(self, who, points, T):
        if not _strip_cloud(points) or points.device != self.device:
            raise ValueError(f'StripBinner.{who}: points must be a contiguous [N,4] float32 tensor on {self.device}')
        N = points.shape[0]
        need = int(lib().lm_strip_chunk_workspace_bytes(N, T))
        if need <= 0:
            raise LanemapHipError(f'StripBinner.{who}: a chunk of {N} points is not supported (at most 2^31 - 1)')
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, device=self.device, dtype=torch.uint8)
        return N

    def count(self, points):
        """Pass A, one chunk: asynchronous."""
        if self._host_counts is not None:
            raise ValueError('StripBinner.count: the counts were read already (counts()); pass A is over')
        N = self._chunk('count', points, len(self.params))
        check(lib().lm_strip_bin_count(self._plan((0, len(self.params))).handle, _ptr(points) if N else None, N, _ptr(self._ws), self._ws.numel(),
                                       _ptr(self._counts), _stream()))

    def counts(self):
        """-> int64 numpy [T]: the points of every tile over all chunks counted.  The one read-back of pass A."""
        if self._host_counts is None:
            self._host_counts = self._counts.cpu().numpy()
        return self._host_counts

    def begin(self, tiles=None, capacity=None):
        """Pass B for the tiles (t0, t1) (None: all): allocates binned and sets the cursors to the exclusive prefix of their counts."""
        T = len(self.params)
        t0, t1 = (0, T) if tiles is None else (int(tiles[0]), int(tiles[1]))
        if not 0 <= t0 < t1 <= T:
            raise ValueError(f'StripBinner.begin: tiles={tiles!r} is no run t0 < t1 of the {T} tiles')
        c = [int(v) for v in self.counts()[t0:t1]]
        offs = [0]
        for v in c:
            offs.append(offs[-1] + v)
        cap = offs[-1] if capacity is None else int(capacity)
        if cap < 0:
            raise ValueError(f'StripBinner.begin: capacity={capacity!r} is negative')
        import numpy as np
        meta = torch.from_numpy(np.asarray(offs[:-1] + [0], dtype=np.int64)).to(self.device)          # cursors [t1 - t0] | err
        self._run = {'plan': self._plan((t0, t1)), 'T': t1 - t0, 'offs': offs, 'cap': cap, 'meta': meta,
                     'binned': torch.empty((cap, 4), device=self.device, dtype=torch.float32)}

    def scatter(self, points):
        """Pass B, one chunk: asynchronous."""
        r = self._run
        if r is None:
            raise ValueError('StripBinner.scatter: call begin() first')
        N = self._chunk('scatter', points, r['T'])
        m = r['meta']
        check(lib().lm_strip_bin_scatter(r['plan'].handle, _ptr(points) if N else None, N, _ptr(self._ws), self._ws.numel(), _ptr(m),
                                         _ptr(r['binned']) if r['cap'] else None, r['cap'], C.c_void_p(m.data_ptr() + 8 * r['T']), _stream()))

    def finish(self):
        """-> (binned [sum counts, 4], offsets: t1 - t0 + 1 host ints) of the run begin() opened.  Reads the error word and the
        cursors back (one read) and raises LanemapHipError when a chunk overran binned or the chunks of pass B were not those of pass A."""
        r, self._run = self._run, None
        if r is None:
            raise ValueError('StripBinner.finish: call begin() first')
        host = r['meta'].cpu().numpy()
        if host[-1] != 0:
            raise LanemapHipError(f"StripBinner.finish: a chunk overran binned ({r['cap']} rows): the points of pass B are not those that "
                                  'were counted, or capacity is short; nothing was written outside binned')
        if [int(v) for v in host[:-1]] != r['offs'][1:]:
            raise LanemapHipError('StripBinner.finish: the chunks scattered are not the chunks counted (the cursors do not end at the offsets)')
        return r['binned'][:r['offs'][-1]], r['offs']


def tile_ground(points, tile_offsets, params, H=1152, W=1152, cell_px=32, want_cell_min=False):
    """The coarse ground model under every tile (csrc/ground.hip), from the (points, tile_offsets, params) triple bev_raster_batch takes:
    -> (ground [B,Gy,Gx] f32, ground_min [B] f32) on the device, Gy = ceil(H / cell_px), Gx = ceil(W / cell_px).  A cell's raw value is
    the smallest tile-frame height vz of the points the rasteriser keeps for the tile in that cell; ground is the lower median of the
    non-empty cells of its 3 x 3 neighbourhood (NaN where all nine are empty), ground_min the tile's smallest finite ground (+inf: none).
    want_cell_min: -> (ground, ground_min, cell_min [B,Gy,Gx]), the raw minima, NaN = empty.  No synchronisation, but the tile table is
    copied from host memory of the call: not inside a graph capture (the entry refuses a capturing stream by name)."""
    B, offs, par = _tile_range_args('tile_ground', points, tile_offsets, params)
    H, W, cell_px = int(H), int(W), int(cell_px)
    need = lib().lm_tile_ground_workspace_bytes(B, H, W, cell_px)
    Gy, Gx = (-(-H // cell_px), -(-W // cell_px)) if cell_px > 0 else (0, 0)
    ws = _workspace(points, max(need, 16))
    ground = torch.empty((B, Gy, Gx), device=points.device, dtype=torch.float32)
    gmin = torch.empty((B,), device=points.device, dtype=torch.float32)
    cmin = torch.empty_like(ground) if want_cell_min else None
    # (need == 0: unsupported arguments; the call below refuses them with the argument's name)
    check(lib().lm_tile_ground(_stream(), _ptr(points) if points.numel() else None, offs, par, B, H, W, cell_px, _ptr(ws), ws.numel() if need else 0,
                               _ptr(ground), _ptr(gmin), _ptr(cmin)))
    return (ground, gmin, cmin) if want_cell_min else (ground, gmin)


def ground_select(points, tile_offsets, params, ground, H=1152, W=1152, cell_px=32, h_range=(-math.inf, math.inf)):
    """The points of every tile whose height above the tile's ground model lies in h_range = (lo, hi): kept <=> the rasteriser keeps the
    point for the tile, vz is finite and lo <= vz - ground[b, cell] <= hi (infinite bounds switch a side off).  -> (points_out
    [sum kept, 4], offsets: B+1 host ints) as strip_bin_points returns them: each tile's kept points in their input order, the pair
    bev_raster_batch takes.  `ground` is tile_ground's for the same tiles, H, W and cell_px.  One device-to-host read of the offsets: not
    inside a graph capture (the entry refuses a capturing stream by name)."""
    B, offs, par = _tile_range_args('ground_select', points, tile_offsets, params)
    H, W, cell_px = int(H), int(W), int(cell_px)
    Gy, Gx = (-(-H // cell_px), -(-W // cell_px)) if cell_px > 0 else (0, 0)
    if tuple(ground.shape) != (B, Gy, Gx) or ground.dtype != torch.float32 or not ground.is_contiguous() or ground.device != points.device:
        raise ValueError(f'ground_select: ground must be a contiguous [{B},{Gy},{Gx}] float32 tensor on {points.device} (tile_ground\'s output)')
    N = int(offs[B] - offs[0]) if B else 0
    need = lib().lm_ground_select_workspace_bytes(max(N, 0), B)
    ws = _workspace(points, max(need, 16))
    out = torch.empty((max(N, 0), 4), device=points.device, dtype=torch.float32)
    doffs = torch.empty((B + 1,), device=points.device, dtype=torch.int64)
    hoffs = (C.c_long * (B + 1))()
    check(lib().lm_ground_select(_stream(), _ptr(points) if points.numel() else None, offs, par, B, H, W, cell_px, _ptr(ground),
                                 float(h_range[0]), float(h_range[1]), _ptr(ws), ws.numel() if need else 0, _ptr(out) if N > 0 else None,
                                 C.c_void_p(doffs.data_ptr()), hoffs))
    return out[:hoffs[B]], [int(o) for o in hoffs]


def tile_intensity_window(points, tile_offsets, params, H=1152, W=1152, percentiles=(1.0, 99.9), group=None, want_hist=False):
    """Two percentiles of the intensities of the points every tile (or group of tiles) keeps (csrc/intensity.hip), from the (points,
    tile_offsets, params) triple bev_raster_batch takes: -> (window [G,2] int32, count [G] int64) on the device, with want_hist also
    hist [G,4096] int32 (the counted points per coarse bin key >> 4).  A point counts for a tile when the rasteriser keeps it for the
    tile and its intensity is not NaN; its key is floor(clamp(intensity, 0, 65535)).  With n counted points in a group, window[g] holds the
    keys of 0-based ranks (n - 1) * ppm // 10**6 in ascending order for ppm = round(p * 10**4) of the two percentiles; n = 0: (-1, -1).
    group: B ints in 0..G-1 with G = max + 1 (None: every tile its own group).  Exact and reproducible.  No synchronisation, but the
    tile table is copied from host memory of the call: not inside a graph capture (the entry refuses a capturing stream by name)."""
    B, offs, par = _tile_range_args('tile_intensity_window', points, tile_offsets, params)
    H, W = int(H), int(W)
    if group is None:
        G, grp = B, None
    else:
        if len(group) != B:
            raise ValueError(f'tile_intensity_window: {len(group)} group entries for {B} tiles')
        ids = [int(g) for g in group]
        if any(not 0 <= g < B for g in ids):                    # before anything is sized by G (the library names G <= B the same way)
            bad = next(b for b, g in enumerate(ids) if not 0 <= g < B)
            raise ValueError(f'tile_intensity_window: group[{bad}]={ids[bad]} is outside 0..B-1={B - 1} (G = max(group) + 1 <= B)')
        grp = (C.c_int * B)(*ids)
        G = max(ids + [0]) + 1
    q_lo, q_hi = (int(round(float(p) * 1e4)) for p in percentiles)
    need = lib().lm_tile_intensity_workspace_bytes(B, G)
    ws = _workspace(points, max(need, 16))
    window = torch.empty((max(G, 0), 2), device=points.device, dtype=torch.int32)
    count = torch.empty((max(G, 0),), device=points.device, dtype=torch.int64)
    hist = torch.empty((max(G, 0), 4096), device=points.device, dtype=torch.int32) if want_hist else None
    # (need == 0: unsupported arguments; the call below refuses them with the argument's name)
    check(lib().lm_tile_intensity_window(_stream(), _ptr(points) if points.numel() else None, offs, par, B, H, W, grp, G, q_lo, q_hi,
                                         _ptr(ws), ws.numel() if need else 0, _ptr(window), _ptr(count), _ptr(hist)))
    return (window, count, hist) if want_hist else (window, count)


CELLS_WORKSPACE_CAP = 256 << 20     # bytes: tile_intensity_cells takes its tiles in groups whose counters (1 KiB per cell) stay below it


def _cell_grid(H, W, cell_px):
    return (-(-H // cell_px), -(-W // cell_px)) if cell_px > 0 else (0, 0)


def tile_intensity_cells(points, tile_offsets, params, H=1152, W=1152, cell_px=32, q_ppm=500000, min_points=64):
    """The local intensity level under every tile (csrc/intensity.hip), from the (points, tile_offsets, params) triple bev_raster_batch
    takes: -> (level, count, model), each [B,Gy,Gx] int32 on the device, Gy = ceil(H / cell_px), Gx = ceil(W / cell_px).  A point counts
    for a tile when the rasteriser keeps it for the tile and its intensity is not NaN; its key is floor(clamp(intensity, 0, 65535)), its
    cell (row // cell_px, col // cell_px).  count = the counted points n of the cell; level = the key of 0-based rank
    (n - 1) * q_ppm // 10**6 among them (500000: the lower median; -1 for n = 0); model = the lower median of the levels of the KNOWN cells
    (n >= min_points) of the 3 x 3 neighbourhood, -1 where none is known.  Exact and reproducible.  The counters take 1 KiB per cell:
    the tiles are processed in groups whose workspace stays below CELLS_WORKSPACE_CAP (a group is at least one tile).  No
    synchronisation, but the tile table is copied from host memory of the call: not inside a graph capture (the entry refuses a capturing
    stream by name)."""
    B, offs, par = _tile_range_args('tile_intensity_cells', points, tile_offsets, params)
    H, W, cell_px = int(H), int(W), int(cell_px)
    Gy, Gx = _cell_grid(H, W, cell_px)
    level, count, model = (torch.empty((B, Gy, Gx), device=points.device, dtype=torch.int32) for _ in range(3))
    one = lib().lm_tile_intensity_cells_workspace_bytes(1, H, W, cell_px)
    step = max(1, min(B, CELLS_WORKSPACE_CAP // one)) if one else max(B, 1)
    for b0 in range(0, B, step):
        n = min(step, B - b0)
        need = lib().lm_tile_intensity_cells_workspace_bytes(n, H, W, cell_px)
        ws = _workspace(points, max(need, 16))
        sub = (C.c_long * (n + 1)).from_buffer(offs, 8 * b0)
        # (need == 0: unsupported arguments; the call below refuses them with the argument's name)
        check(lib().lm_tile_intensity_cells(_ptr(points) if points.numel() else None, sub, (LmRasterParams * n).from_buffer(par, b0 * C.sizeof(LmRasterParams)),
                                            n, H, W, cell_px, int(q_ppm), int(min_points), _ptr(ws), ws.numel() if need else 0,
                                            _ptr(level[b0:b0 + n]), _ptr(count[b0:b0 + n]), _ptr(model[b0:b0 + n]), _stream()))
    return level, count, model


def tile_intensity_apply(points, tile_offsets, params, gains, H=1152, W=1152, cell_px=32, out=None):
    """Every counted point's intensity times the gain of its place (csrc/intensity.hip): gains [B,Gy,Gx] f32 on the device, one per cell
    of tile_intensity_cells' grid, interpolated bilinearly between the cell centres (clamped at the tile's edge) with every float32
    operation rounded on its own; i' = min(i * g, 65535).  x, y, z and the points that do not count keep every bit.  out: None - IN PLACE,
    -> points; or a [N,4] f32 tensor of points' shape, which gets the rows tile_offsets[0] .. tile_offsets[B] and is returned.  One
    streaming pass.  Not inside a graph capture (the entry refuses a capturing stream by name)."""
    B, offs, par = _tile_range_args('tile_intensity_apply', points, tile_offsets, params)
    H, W, cell_px = int(H), int(W), int(cell_px)
    Gy, Gx = _cell_grid(H, W, cell_px)
    if not torch.is_tensor(gains) or tuple(gains.shape) != (B, Gy, Gx) or gains.dtype != torch.float32 or not gains.is_contiguous() or \
            gains.device != points.device:
        raise ValueError(f'tile_intensity_apply: gains must be a contiguous [{B},{Gy},{Gx}] float32 tensor on {points.device}')
    out = points if out is None else out
    if out.shape != points.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != points.device:
        raise ValueError(f'tile_intensity_apply: out must be a contiguous {list(points.shape)} float32 tensor on {points.device}')
    need = lib().lm_tile_intensity_apply_workspace_bytes(B)
    ws = _workspace(points, max(need, 16))
    check(lib().lm_tile_intensity_apply(_ptr(points) if points.numel() else None, offs, par, B, H, W, cell_px, _ptr(gains), _ptr(ws),
                                        ws.numel() if need else 0, _ptr(out) if out.numel() else None, _stream()))
    return out


def drape_vertices(points, tile_offsets, params, vertices, vertex_offsets, H=1152, W=1152, radius_px=4, want_pixel_min=False):
    """Heights of polyline vertices read off the points (csrc/drape.hip), from the (points, tile_offsets, params) triple bev_raster_batch
    takes: vertices [V,2] int32 host array of (row, col) pixels, tile 0's first; vertex_offsets: B+1 ints, vertex_offsets[0] = 0.
    -> (z [V] f32, npix [V] int32) on the device, with want_pixel_min also pixel_min [V, 2R+1, 2R+1] f32 (NaN = empty).  pixel_min[v, i, j]
    is the smallest tile-frame height vz of the points the rasteriser keeps for the vertex's tile in pixel (row + i - R, col + j - R), z[v]
    the lower median of the npix[v] non-empty ones (NaN for none).  Exact and reproducible.  No synchronisation, but the tile and vertex
    tables are copied from host memory of the call: not inside a graph capture (the entry refuses a capturing stream by name)."""
    import numpy as np
    B, offs, par = _tile_range_args('drape_vertices', points, tile_offsets, params)
    H, W, R = int(H), int(W), int(radius_px)
    vert = np.ascontiguousarray(np.asarray(vertices, dtype=np.int32).reshape(-1, 2))
    if len(vertex_offsets) != B + 1:
        raise ValueError(f'drape_vertices: {len(vertex_offsets)} vertex_offsets for {B} tiles (B + 1 are needed)')
    voffs = (C.c_long * (B + 1))(*[int(o) for o in vertex_offsets])
    if voffs[B] != vert.shape[0]:
        raise ValueError(f'drape_vertices: vertex_offsets end at {voffs[B]}, vertices has {vert.shape[0]} rows')
    V, D = vert.shape[0], 2 * max(R, 0) + 1
    need = lib().lm_drape_workspace_bytes(V, B, R)
    ws = _workspace(points, max(need, 16))
    z = torch.empty((V,), device=points.device, dtype=torch.float32)
    npix = torch.empty((V,), device=points.device, dtype=torch.int32)
    pmin = torch.empty((V, D, D), device=points.device, dtype=torch.float32) if want_pixel_min else None
    # (need == 0: unsupported arguments; the call below refuses them with the argument's name)
    check(lib().lm_drape_vertices(_stream(), _ptr(points) if points.numel() else None, offs, par, B, H, W, C.c_void_p(vert.ctypes.data), voffs, R,
                                  _ptr(ws), ws.numel() if need else 0, _ptr(z), _ptr(npix), _ptr(pmin)))
    return (z, npix, pmin) if want_pixel_min else (z, npix)


def _gap_args(who, u8):
    if not u8.is_cuda:
        _ptr(u8)
    if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3 or not u8.is_contiguous():
        raise ValueError(f'{who}: tiles must be a contiguous uint8 tensor [B,H,W,3], not {u8.dtype} {tuple(u8.shape)}'
                         + ('' if u8.is_contiguous() else ' (not contiguous)'))
    return int(u8.shape[0]), int(u8.shape[1]), int(u8.shape[2])


def tile_gap_hist(u8, max_radius_px=4):
    """How far the empty pixels of every u8 HWC tile [B,H,W,3] lie from a return (csrc/gapfill.hip): -> hist [B, Rmax + 2] int32 on the
    device, Rmax = max_radius_px in 1..8.  hist[b, 0] = the non-empty pixels (a pixel is empty when its three bytes are 0), hist[b, k],
    k = 1..Rmax, = the empty pixels whose nearest non-empty pixel of the same tile, d2 = dr^2 + dc^2 <= Rmax^2 away, has
    (k - 1)^2 < d2 <= k^2, hist[b, Rmax + 1] = the empty pixels without one.  Every row sums to H W.  Exact and reproducible.  No
    synchronisation."""
    B, H, W = _gap_args('tile_gap_hist', u8)
    R = int(max_radius_px)
    hist = torch.empty((B, max(R, 0) + 2), device=u8.device, dtype=torch.int32)
    check(lib().lm_tile_gap_hist(_stream(), _ptr(u8), B, H, W, R, _ptr(hist)))
    return hist


def tile_gap_fill(u8, radius_px):
    """The u8 HWC tiles [B,H,W,3] with their gaps filled (csrc/gapfill.hip): -> a new u8 [B,H,W,3].  radius_px: an int or B ints in 0..8,
    per tile.  A non-empty pixel keeps its bytes; an empty pixel takes the three bytes of the nearest non-empty pixel of the same INPUT
    tile within the disc of that radius (ties in distance: the largest R << 16 | G << 8 | B, i.e. brightest, then highest); every other
    pixel stays empty.  Radius 0 is a copy.  Exact and reproducible.  No synchronisation."""
    B, H, W = _gap_args('tile_gap_fill', u8)
    radii = [int(r) for r in radius_px] if hasattr(radius_px, '__len__') else [int(radius_px)] * B
    if len(radii) != B:
        raise ValueError(f'tile_gap_fill: {len(radii)} radius_px entries for {B} tiles')
    out = torch.empty_like(u8)
    check(lib().lm_tile_gap_fill(_stream(), _ptr(u8), B, H, W, (C.c_int * B)(*radii), _ptr(out)))
    return out


def tile_ingest(u8_hwc):
    """[B,H,W,C>=3] uint8 (decoded PNG) -> [B,3,H,W] f32 = u8/255 (reference load_img contract)."""
    x = u8_hwc.contiguous()
    B, H, W, C_ = x.shape
    out = torch.empty((B, 3, H, W), device=x.device, dtype=torch.float32)
    check(lib().lm_tile_ingest_u8(_stream(), _ptr(x), _ptr(out), B, H, W, C_))
    return out


# ------------------------------------------------------------------------------- sparse-voxel LiDAR encoder (config 5)
_vox_ws = {}


def exclusive_scan_u32(x, out=None):
    """out[i] = x[0] + .. + x[i-1] over a device int32/uint32 vector (u32 arithmetic; csrc/prim.hip)."""
    x = x.contiguous()
    assert x.dim() == 1 and x.dtype in (torch.int32, torch.uint32)
    out = torch.empty_like(x) if out is None else out
    n = x.numel()
    ws = torch.empty((lib().lm_scan_workspace_bytes(n),), device=x.device, dtype=torch.uint8)
    check(lib().lm_exclusive_scan_u32(_stream(), _ptr(x), _ptr(out), n, _ptr(ws), ws.numel()))
    return out


def sort_pairs_u32_(keys, vals, end_bit=32):
    """Stable in-place sort of (keys, vals) (device int32 vectors read as u32) by the low end_bit bits of the keys (csrc/prim.hip)."""
    assert keys.dim() == 1 and keys.shape == vals.shape and keys.is_contiguous() and vals.is_contiguous()
    assert keys.dtype in (torch.int32, torch.uint32) and vals.dtype in (torch.int32, torch.uint32)
    n = keys.numel()
    ws = torch.empty((lib().lm_sort_pairs_workspace_bytes(n),), device=keys.device, dtype=torch.uint8)
    check(lib().lm_sort_pairs_u32(_stream(), _ptr(keys), _ptr(vals), n, int(end_bit), _ptr(ws), ws.numel()))
    return keys, vals


def voxelize_batch(points, range_lo, voxel_size, grid_xyz, max_points, max_voxels, ldf=16, raster_order=False):
    """Hard-voxelise a list of [N_i,4] device tensors -> (feats [V,ldf] (mean x,y,z,i; rest 0), coords [V,4] i32 (b,z,y,x),
    row_ends list).  One host sync at the end (the row count sizes every later launch).  Rows of a sample come in the
    reference's order (voxels numbered by first point) or, with raster_order, sorted by (z, y, x) - same voxel set."""
    dev = points[0].device
    B = len(points)
    cells = int(grid_xyz[0]) * int(grid_xyz[1]) * int(grid_xyz[2])
    caps = [min(int(p.shape[0]), int(max_voxels), cells) for p in points]
    cap = max(1, sum(caps))
    feats = torch.empty((cap, ldf), device=dev, dtype=torch.float32)
    coords = torch.empty((cap, 4), device=dev, dtype=torch.int32)
    ends = torch.zeros((B,), device=dev, dtype=torch.int32)
    nmax = max(int(p.shape[0]) for p in points)
    need = lib().lm_voxelize_workspace_bytes(nmax)
    key = (dev.index, _stream().value)
    ws = _vox_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty((need,), device=dev, dtype=torch.uint8)
        _vox_ws[key] = ws
    lo = (C.c_float * 3)(*[float(v) for v in range_lo])
    vs = (C.c_float * 3)(*[float(v) for v in voxel_size])
    g = (C.c_int * 3)(*[int(v) for v in grid_xyz])
    for b, p in enumerate(points):
        if not p.is_cuda:
            raise LanemapHipError('voxelize_batch needs device tensors; no CPU fallback exists')
        p = p.contiguous().float()
        assert p.dim() == 2 and p.shape[1] == 4
        base = C.c_void_p(ends[b - 1:b].data_ptr()) if b > 0 else None
        check(lib().lm_voxelize_hard(_stream(), _ptr(p) if p.shape[0] else None, p.shape[0], lo, vs, g, int(max_points),
                                     int(max_voxels), b, base, cap, _ptr(feats), ldf, _ptr(coords),
                                     C.c_void_p(ends[b:b + 1].data_ptr()), int(raster_order), _ptr(ws), ws.numel()))
    row_ends = [int(v) for v in ends.cpu()]
    V = row_ends[-1]
    return feats[:V], coords[:V], row_ends


def _ksp(kernel, stride, padding):
    return (C.c_int * 9)(*[int(v) for v in (*kernel, *stride, *padding)])


def sparse_grid(coords, B, shape):
    D, H, W = shape
    grid = torch.empty((B, D, H, W), device=coords.device, dtype=torch.int32)
    check(lib().lm_sparse_grid_build(_stream(), _ptr(coords), coords.shape[0], _ptr(grid), B, D, H, W))
    return grid


def sparse_conv_outputs(in_coords, B, in_shape, kernel, stride, padding):
    """Active output sites of a SparseConv3d -> (out_grid [B,Do,Ho,Wo] i32, out_coords [Vo,4] i32, out_shape).  Host sync."""
    out_shape = tuple((in_shape[a] + 2 * padding[a] - kernel[a]) // stride[a] + 1 for a in range(3))
    Do, Ho, Wo = out_shape
    dev = in_coords.device
    cells = B * Do * Ho * Wo
    n_in = in_coords.shape[0]
    taps_per_axis = [(kernel[a] + stride[a] - 1) // stride[a] for a in range(3)]
    cap = max(1, min(cells, n_in * taps_per_axis[0] * taps_per_axis[1] * taps_per_axis[2]))
    grid = torch.empty((B, Do, Ho, Wo), device=dev, dtype=torch.int32)
    coords = torch.empty((cap, 4), device=dev, dtype=torch.int32)
    count = torch.zeros((1,), device=dev, dtype=torch.int32)
    need = lib().lm_sparse_conv_outputs_workspace_bytes(cells)
    ws = torch.empty((need,), device=dev, dtype=torch.uint8)
    check(lib().lm_sparse_conv_outputs(_stream(), _ptr(in_coords), n_in, B, _ksp(kernel, stride, padding), Do, Ho, Wo,
                                       _ptr(grid), _ptr(coords), cap, _ptr(count), _ptr(ws), need))
    n = int(count.item())
    if n > cap:
        raise LanemapHipError(f'sparse_conv_outputs: {n} active sites exceed the bound {cap}')
    return grid, coords[:n], out_shape


def sparse_rulebook(out_coords, in_grid, kernel, stride, padding):
    B, D, H, W = in_grid.shape
    taps = kernel[0] * kernel[1] * kernel[2]
    nbr = torch.empty((out_coords.shape[0], taps), device=out_coords.device, dtype=torch.int32)
    check(lib().lm_sparse_rulebook(_stream(), _ptr(out_coords), out_coords.shape[0], _ptr(in_grid), B, D, H, W,
                                   _ksp(kernel, stride, padding), _ptr(nbr)))
    return nbr


def pack_sparse(w):
    """spconv weight [kD,kH,kW,Cin,Cout] -> kernel layout of lm_conv_gather_mfma_f32: Cin > 16: [taps, CoutP, CinP]
    (CinP = Cin up to 32s); Cin <= 16: tap pairs [ceil(taps/2), CoutP, 32] with k = (tap & 1) * 16 + c.  Zero filled."""
    kd, kh, kw, ci, co = w.shape
    taps = kd * kh * kw
    cop = (co + 127) // 128 * 128
    wt = w.reshape(taps, ci, co).permute(0, 2, 1).float()          # [taps, co, ci]
    if ci <= 16:
        p = torch.zeros(((taps + 1) // 2 * 2, cop, 16), device=w.device, dtype=torch.float32)
        p[:taps, :co, :ci] = wt
        return p.reshape(-1, 2, cop, 16).permute(0, 2, 1, 3).reshape(-1, cop, 32).contiguous()
    cip = (ci + 31) // 32 * 32
    p = torch.zeros((taps, cop, cip), device=w.device, dtype=torch.float32)
    p[:, :co, :ci] = wt
    return p.contiguous()


def sparse_ld(c):
    """Row stride of a c-channel sparse feature matrix: 16 for <= 16 channels (tap-pair kernel), else c up to 32s."""
    return 16 if c <= 16 else (c + 31) // 32 * 32


def conv_gather(x, nbr, wp, cin, cout, scale=None, shift=None, res=None, act=ACT_NONE):
    """Rulebook convolution: y[m, :cout] = act(bn(sum_t W[t] x[nbr[m, t]]) + res[m]).  x [V, sparse_ld(cin)] with zero padding
    channels; returns y [M, sparse_ld(cout)] padded the same way."""
    M, taps = nbr.shape
    cin_k = sparse_ld(cin)
    assert x.stride(1) == 1 and x.stride(0) >= cin_k
    ldy = sparse_ld(cout)
    y = torch.zeros((M, ldy), device=x.device, dtype=torch.float32) if ldy != cout else \
        torch.empty((M, ldy), device=x.device, dtype=torch.float32)
    def launch():
        check(lib().lm_conv_gather_mfma_f32(_stream(), _ptr(x), x.stride(0), _ptr(nbr), taps, _ptr(wp), wp.shape[1], _ptr(scale),
                                            _ptr(shift), _ptr(res), res.stride(0) if res is not None else 0, _ptr(y), ldy,
                                            M, cin_k, cout, act))
    if _conv_hook is not None:
        _conv_hook(f'spconv M{M} taps{taps} {cin}->{cout}', 2.0 * M * taps * cin * cout, launch)
    else:
        launch()
    return y


def sparse_to_dense(feats, coords, B, shape, C_, flip_h):
    """-> logical [B, C*D, H, W] tensor stored NHWC."""
    D, H, W = shape
    out = new_act(B, C_ * D, H, W, feats.device)
    check(lib().lm_sparse_to_dense_nhwc(_stream(), _ptr(feats), feats.stride(0), _ptr(coords), feats.shape[0], _ptr(out),
                                        B, D, H, W, C_, int(flip_h)))
    return out


def upsample_bicubic(x, size):
    x, ld = as_nhwc(x)
    B, C_, H, W = x.shape
    assert ld == C_
    out = new_act(B, C_, size[0], size[1], x.device)
    check(lib().lm_upsample_bicubic_nhwc(_stream(), _ptr(x), _ptr(out), B, H, W, C_, size[0], size[1]))
    return out
