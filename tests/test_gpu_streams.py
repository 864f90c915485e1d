"""GPU stream tests (-m gpu): every `lm_*` entry that takes a stream uses that stream and nothing else - on a side stream beside a busy
default stream, and (class 'async') in three replays of a captured graph over altered inputs and poisoned outputs (tests/stream_state.py).

One case per entry, or per ops function that chains several; CASE_ENTRIES names what each case is expected to reach, and the last test
holds the union of what the interposer SAW on the side stream to lds_state.stream_entries() minus STREAM_EXEMPT.  Every case also holds
its side-stream outputs to the reference the entry has elsewhere in the suite (an fp64 torch expression, numpy, or the tests/*_ref.py
twin), so a case cannot pass by being wrong three times.  Shapes are the smallest that reach every enqueue of the entry: tiles of at
most 64 x 64 pixels, a few thousand points.  The 'host' entries get a fourth test each: inside a capture they refuse by name."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stream_state
from gpu_common import _chk, _close, _g, _gn_ref, _lib, _nhwc_dev, _quarter_grid, _s
from lanemapping_amd import ops
from lanemapping_amd._lib import LanemapHipError
from stream_state import Case, stream_runs

pytestmark = pytest.mark.gpu

# (a literal: tests/test_stream_inventory_cpu.py reads it without importing this file)
CASE_ENTRIES = {
    'conv_mfma_lateral': ['lm_conv2d_nhwc_mfma_f32'],
    'conv_mfma_tiny_k': ['lm_conv2d_nhwc_mfma_f32'],
    'conv_mfma_small_m': ['lm_conv2d_nhwc_mfma_f32'],
    'conv_mfma_big_tile': ['lm_conv2d_nhwc_mfma_f32'],
    'conv_mfma_resup': ['lm_conv2d_nhwc_mfma_resup_f32'],
    'conv_mfma_gnstats': ['lm_conv2d_nhwc_mfma_f32_gnstats', 'lm_gn_finalize'],
    'wino44_gn_partial': ['lm_conv3x3_winograd44_f32', 'lm_gn_finalize'],
    'wino44_gn_split': ['lm_conv3x3_winograd44_f32', 'lm_gn_finalize_split'],
    'wino44_twin': ['lm_conv3x3_winograd44_twin_f32'],
    'wino44_split': ['lm_wino44_split_fragments', 'lm_conv3x3_winograd44_split_f32', 'lm_conv3x3_winograd44_split_twin_f32'],
    'stem_f32': ['lm_stem_conv7x7_bn_relu'],
    'stem_u8': ['lm_stem_conv7x7_bn_relu_u8'],
    'maxpool': ['lm_maxpool3x3s2_nhwc'],
    'conv_small': ['lm_conv2d_nhwc_small'],
    'gn_stats': ['lm_gn_stats'],
    'gn_relu_upsample': ['lm_gn_relu_upsample'],
    'gn_relu_upsample_sum': ['lm_gn_relu_upsample_sum'],
    'gn_relu_upsample_sum_conv1x1': ['lm_gn_relu_upsample_sum_conv1x1'],
    'upsample_bilinear': ['lm_upsample_bilinear_nhwc', 'lm_upsample_bilinear_to_chw'],
    'upsample_bicubic': ['lm_upsample_bicubic_nhwc'],
    'layernorm': ['lm_layernorm_rows'],
    'unpatchify': ['lm_unpatchify'],
    'token_mix': ['lm_token_mix_mfma_f32'],
    'attention': ['lm_attention_f32'],
    'attention_masked': ['lm_attention_masked_f32'],
    'head_tokens': ['lm_head_tokens', 'lm_head_tokens_window'],
    'head_stage2': ['lm_head_stage2'],
    'head_proposal_conf': ['lm_head_proposal_conf'],
    'head_endpoint': ['lm_head_endpoint'],
    'decode_proposals': ['lm_decode_proposals'],
    'decode_orient': ['lm_decode_orient'],
    'decode_semantic': ['lm_decode_semantic'],
    'endp_topk': ['lm_endp_topk'],
    'pack_segments': ['lm_pack_segments'],
    'softmax_rows': ['lm_softmax_rows'],
    'rowref_select': ['lm_rowref_select'],
    'rowref_gather_scatter': ['lm_rowref_gather', 'lm_rowref_scatter', 'lm_rowref_gather_win', 'lm_rowref_scatter_win'],
    'rowref_decode': ['lm_rowref_decode'],
    'exclusive_scan': ['lm_exclusive_scan_u32'],
    'sort_pairs': ['lm_sort_pairs_u32'],
    'bev_raster': ['lm_bev_raster_batch', 'lm_bev_raster_batch_scaled'],
    'tile_ingest': ['lm_tile_ingest_u8'],
    'tile_gap': ['lm_tile_gap_hist', 'lm_tile_gap_fill'],
    'strip_bin': ['lm_strip_bin_points'],
    'tile_ground': ['lm_tile_ground', 'lm_ground_select'],
    'tile_intensity_window': ['lm_tile_intensity_window'],
    'drape_vertices': ['lm_drape_vertices'],
    'voxelize': ['lm_voxelize_hard'],
    'sparse_index': ['lm_sparse_grid_build', 'lm_sparse_conv_outputs', 'lm_sparse_rulebook'],
    'conv_gather': ['lm_conv_gather_mfma_f32'],
    'sparse_to_dense': ['lm_sparse_to_dense_nhwc'],
    'las_decode': ['lm_las_decode_points', 'lm_las_decode_select'],
    'label': ['lm_label_points', 'lm_las_label_records'],
    'line_profile': ['lm_line_profile_points', 'lm_las_line_profile_records', 'lm_las_line_colour_records'],
    'line_cross': ['lm_line_cross_points', 'lm_las_line_cross_records'],
    'residue': ['lm_residue_keys', 'lm_cell_components', 'lm_residue_stats'],
}


# ==================================================================================================== the cases' scaffold
class _Built:
    """One case as its builder returns it: make(k) -> {input name: CPU tensor} of data set k (0: the original; the reference is computed
    from make(0)); up: {input name: uploader(t, dev)} where a plain .to(dev) is not the layout the call takes; call(ins, dev) -> outs;
    check(outs, make(0)) holds the side-stream outputs to the reference; work(dev) -> {name: workspace tensor} of a raw-entry case,
    allocated once in setup, handed to call(ins, dev, work) and filled with 0xFF by the harness before every replay."""

    def __init__(self, make, call, check, up=None, work=None):
        self.make, self.call, self.check, self.up, self.work = make, call, check, up or {}, work


BUILDERS = {}
_DONE = {}


def case(name):
    def reg(fn):
        assert name in CASE_ENTRIES and name not in BUILDERS, name
        BUILDERS[name] = fn
        return fn
    return reg


def _as_case(name, b):
    def put(t, n, dev):
        return b.up[n](t, dev) if n in b.up else t.to(dev)

    def setup(dev):
        sets = [{n: put(t, n, dev) for n, t in b.make(k).items()} for k in range(3)]
        state = {'ins': {n: put(t, n, dev) for n, t in b.make(0).items()}, 'sets': sets, 'dev': dev}
        if b.work is not None:
            state['work_named'] = b.work(dev)
            state['work'] = list(state['work_named'].values())
        return state

    def run(state):
        return b.call(state['ins'], state['dev'], state['work_named']) if b.work is not None else b.call(state['ins'], state['dev'])

    def alter(state, k):
        for n, t in state['ins'].items():
            t.copy_(state['sets'][k][n])
    return Case(name, CASE_ENTRIES[name], setup, run, alter)


def _result(name, dev):
    """The case run through the harness once per session, checked against its reference, and what it reached."""
    if name not in _DONE:
        b = BUILDERS[name]()
        out = stream_runs(_as_case(name, b), dev)
        reached = {e for e, names in stream_state.SEEN.items() if name in names}
        missing = set(CASE_ENTRIES[name]) - reached
        assert not missing, f'{name}: declared but not reached on the side stream: {sorted(missing)}'
        b.check(out, b.make(0))
        _DONE[name] = reached
    return _DONE[name]


def _act(t, dev, ld=None):
    """logical [B,C,H,W] CPU tensor -> NHWC-stored device tensor, optionally a channel slice (column 0) of rows ld wide."""
    if ld is None:
        return _nhwc_dev(t, dev)
    B, Cc, H, W = t.shape
    buf = torch.zeros(B, H, W, ld, device=dev)
    buf[..., :Cc] = t.to(dev).permute(0, 2, 3, 1)
    return buf[..., :Cc].permute(0, 3, 1, 2)


def _affine(y, sc, sh):
    if sc is not None:
        y = y * sc.double().view(1, -1, 1, 1)
    return y + sh.double().view(1, -1, 1, 1)


def _stats_close(st, y_ref, name):
    mean, rstd = _gn_ref(y_ref)
    st = st.double().cpu()
    assert float(((st[..., 0] - mean).abs() / mean.abs().clamp_min(1.0)).max()) <= 1e-5, name + ' mean'
    assert float(((st[..., 1] - rstd).abs() / rstd).max()) <= 1e-5, name + ' rstd'


def _up(x, Ho, Wo):
    return F.interpolate(x, size=(Ho, Wo), mode='bilinear', align_corners=True)


def _randn_sets(shapes, seed, scale=1.0, shift=0.0):
    """make(k) for float inputs: {name: randn(shape) * scale + shift} from seed + 1000 k."""
    def make(k):
        g = _g(seed + 1000 * k)
        return {n: torch.randn(*s, generator=g) * scale + shift for n, s in shapes.items()}
    return make


# ==================================================================================================== convolutions
def _conv_case(B, H, W, cin, cout, k, seed, res_ld=None, res_up=None):
    """ops.conv_mfma, stride 1, pad k // 2, shift and (where res_ld) a full-size residual or (res_up) a coarse bilinear one."""
    g = _g(seed)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    sh = torch.randn(cout, generator=g)
    shapes = {'x': (B, cin, H, W)}
    if res_ld:
        shapes['res'] = (B, cout, H, W)
    if res_up:
        shapes['rc'] = (B, cout) + res_up
    const = {}

    def call(ins, dev):
        if not const:
            const.update(wp=ops.pack_mfma(w.to(dev)), sh=sh.to(dev))
        kw = {'res': ins['res']} if res_ld else {'res_up': ins['rc']} if res_up else {}
        return ops.conv_mfma(ins['x'], const['wp'], cout, k, k, 1, k // 2, 1, None, const['sh'], **kw)

    def check(out, d):
        ref = F.conv2d(d['x'].double(), w.double(), sh.double(), 1, k // 2)
        if res_ld:
            ref = ref + d['res'].double()
        if res_up:
            ref = ref + _up(d['rc'].double(), H, W)
        _close(out, ref, 1e-5, 'conv_mfma')
    up = {'x': _act, 'res': lambda t, dev: _act(t, dev, res_ld), 'rc': _act}
    return _Built(_randn_sets(shapes, seed), call, check, up)


@case('conv_mfma_lateral')
def _():            # lateral_mfma_kernel<16, false, false>: 128 -> 256 1x1 with a plain residual, M = 2 * 12 * 16 = 384 (a multiple of 32)
    return _conv_case(2, 12, 16, 128, 256, 1, 11, res_ld=256)


@case('conv_mfma_tiny_k')
def _():            # K = 64 <= 256, Cout = 136 > 64: launch<128,128,32,64>; 9 x 7: ragged tiles
    return _conv_case(2, 9, 7, 64, 136, 1, 12, res_ld=140)


@case('conv_mfma_small_m')
def _():            # K = 864, 3 x 2 big tiles < 700: launch<64,64,32,32>
    return _conv_case(2, 13, 11, 96, 200, 3, 13)


@case('conv_mfma_big_tile')
def _():            # K = 288 > 256, M = 8192: 64 x 11 = 704 big tiles >= 700: launch<128,128,64,64>
    return _conv_case(2, 64, 64, 288, 1408, 1, 14)


@case('conv_mfma_resup')
def _():            # the coarse-residual epilogue of the tiled kernel (Cout = 96: not a lateral)
    return _conv_case(2, 13, 11, 32, 96, 3, 15, res_up=(5, 6))


@case('conv_mfma_gnstats')
def _():            # 64 -> 128 3x3 on 16 x 16 (Ho Wo = 256 = 2 x 128), statistics epilogue + lm_gn_finalize
    B, H, W, cin, cout = 2, 16, 16, 64, 128
    g = _g(21)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sh = torch.randn(cout, generator=g)
    const = {}

    def call(ins, dev):
        if not const:
            const.update(wp=ops.pack_mfma(w.to(dev)), sh=sh.to(dev))
        return dict(zip(('y', 'stats'), ops.conv_mfma_gnstats(ins['x'], const['wp'], cout, 3, 3, 1, 1, 1, const['sh'])))

    def check(out, d):
        ref = F.conv2d(d['x'].double(), w.double(), sh.double(), 1, 1)
        _close(out['y'], ref, 1e-5, 'gnstats y')
        _stats_close(out['stats'], ref, 'gnstats')
    return _Built(_randn_sets({'x': (B, cin, H, W)}, 21, shift=3.0), call, check, {'x': _act})


def _wino_case(seed, gn_split):
    """Cin 16 -> Cout 64 on 13 x 45, B = 2: the gn_partial epilogue of lm_conv3x3_winograd44_f32 and lm_gn_finalize / _split."""
    B, H, W, cin, cout = 2, 13, 45, 16, 64
    g = _g(seed)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sh = torch.randn(cout, generator=g)
    const = {}

    def call(ins, dev):
        if not const:
            const.update(wf=ops.pack_wino44_fragments(ops.pack_wino44(w.to(dev))), sh=sh.to(dev))
        return dict(zip(('y', 'stats'), ops.conv_wino44(ins['x'], const['wf'], cout, 1, None, const['sh'], gn_eps=1e-5, gn_split=gn_split)))

    def check(out, d):
        ref = F.conv2d(d['x'].double(), w.double(), sh.double(), 1, 1)
        _close(out['y'], ref, 1e-4, 'wino44 y')
        st = out['stats']
        if gn_split > 1:                                     # [split, B, C / split, 2] -> [B, C, 2]
            st = st.permute(1, 0, 2, 3).reshape(B, cout, 2)
        _stats_close(st, ref, 'wino44 gn')
    return _Built(_randn_sets({'x': (B, cin, H, W)}, seed, shift=1.0), call, check, {'x': _act})


@case('wino44_gn_partial')
def _():
    return _wino_case(31, 1)


@case('wino44_gn_split')
def _():
    return _wino_case(32, 2)


@case('wino44_twin')
def _():            # the materialising twin (three kernels over a workspace of its own), scale + residual + ReLU, dilation 2
    B, H, W, cin, cout, dil = 2, 13, 22, 16, 40, 2
    g = _g(33)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    const = {}

    def call(ins, dev):
        if not const:
            const.update(wu=ops.pack_wino44(w.to(dev)), sc=sc.to(dev), sh=sh.to(dev))
        return ops.conv_wino44_twin(ins['x'], const['wu'], cout, dil, const['sc'], const['sh'], ins['res'], ops.ACT_RELU)

    def check(out, d):
        ref = F.relu(_affine(F.conv2d(d['x'].double(), w.double(), None, 1, dil, dil), sc, sh) + d['res'].double())
        _close(out, ref, 1e-4, 'wino44 twin')
    return _Built(_randn_sets({'x': (B, cin, H, W), 'res': (B, cout, H, W)}, 33), call, check, {'x': _act, 'res': _act})


@case('wino44_split')
def _():
    """The split-precision second line: lm_wino44_split_fragments on the (fixed) weights, then the fused kernel and its twin on them.
    The raw entries: the ops wrappers read the weights' magnitude back on every call."""
    B, H, W, cin, cout = 2, 13, 45, 16, 64
    g = _g(34)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sh = torch.randn(cout, generator=g)
    const = {}

    def work(dev):
        return {'ws': torch.empty(_lib().lm_winograd44_twin_workspace_bytes(B, H, W, cin, 64, 1), device=dev, dtype=torch.uint8)}

    def call(ins, dev, wk):
        L = _lib()
        if not const:
            wu = ops.pack_wino44(w.to(dev))
            s = ops.split_scale(wu)
            assert wu.shape[1] == 64
            const.update(wu=wu, s=s, wus=(wu * s).contiguous(), frag=ops.pack_wino44_fragments(wu * s), sh=sh.to(dev), need=wk['ws'].numel())
        x, c = ins['x'], const
        words = torch.empty_like(c['frag'])
        _chk(L.lm_wino44_split_fragments(_s(), c['frag'].data_ptr(), words.data_ptr(), c['frag'].numel() // 4))
        y, yt = ops.new_act(B, cout, H, W, dev), ops.new_act(B, cout, H, W, dev)
        ws = wk['ws']
        cop = c['wu'].shape[1]
        _chk(L.lm_conv3x3_winograd44_split_f32(_s(), x.data_ptr(), cin, words.data_ptr(), cop, None, c['sh'].data_ptr(), None, 0, y.data_ptr(),
                                               cout, B, H, W, cin, cout, 1, ops.ACT_NONE, None, C.c_float(1.0 / c['s'])))
        _chk(L.lm_conv3x3_winograd44_split_twin_f32(_s(), x.data_ptr(), cin, c['wus'].data_ptr(), cop, None, c['sh'].data_ptr(), None, 0,
                                                    yt.data_ptr(), cout, B, H, W, cin, cout, 1, ops.ACT_NONE, ws.data_ptr(), c['need'],
                                                    C.c_float(1.0 / c['s'])))
        return {'words': words, 'y': y, 'twin': yt}

    def check(out, d):
        ref = F.conv2d(d['x'].double(), w.double(), sh.double(), 1, 1)
        _close(out['y'], ref, 1e-4, 'wino44 split')
        assert torch.equal(out['y'], out['twin']), 'split line and its twin differ'
    return _Built(_randn_sets({'x': (B, cin, H, W)}, 34), call, check, {'x': _act}, work)


def _stem_case(u8):
    B, H, W = 2, 37, 43
    g = _g(3743 + u8)
    w = torch.randn(64, 3, 7, 7, generator=g) / 12
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    const = {}

    def make(k):
        gk = _g(50 + u8 + 1000 * k)
        return {'x': torch.randint(0, 256, (B, H, W, 3), generator=gk, dtype=torch.uint8) if u8 else torch.rand(B, 3, H, W, generator=gk)}

    def call(ins, dev):
        if not const:
            const.update(wk=w.permute(2, 3, 1, 0).contiguous().to(dev), sc=sc.to(dev), sh=sh.to(dev))
        return ops.stem(ins['x'], const['wk'], const['sc'], const['sh'])

    def check(out, d):
        x64 = d['x'].permute(0, 3, 1, 2).double() / 255.0 if u8 else d['x'].double()
        _close(out, F.relu(_affine(F.conv2d(x64, w.double(), None, 2, 3), sc, sh)), 1e-5, 'stem')
    return _Built(make, call, check)


@case('stem_f32')
def _():
    return _stem_case(False)


@case('stem_u8')
def _():
    return _stem_case(True)


@case('maxpool')
def _():
    def check(out, d):
        _close(out, F.max_pool2d(d['x'].double(), 3, 2, 1), 1e-5, 'maxpool')
    return _Built(_randn_sets({'x': (2, 12, 19, 25)}, 61), lambda ins, dev: ops.maxpool3x3s2(ins['x']), check, {'x': _act})


@case('conv_small')
def _():            # the wide kernel (32 -> 48, stride 2) with pre-ReLU, 19 x 23: ragged tiles
    B, H, W, cin, cout = 2, 19, 23, 32, 48
    g = _g(62)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    const = {}

    def call(ins, dev):
        if not const:
            const.update(w16=ops.pack_small(w.to(dev)), sc=sc.to(dev), sh=sh.to(dev))
        return ops.conv_small(ins['x'], const['w16'], cout, 3, 3, 2, 1, const['sc'], const['sh'], True)

    def check(out, d):
        _close(out, _affine(F.conv2d(F.relu(d['x'].double()), w.double(), None, 2, 1), sc, sh), 1e-5, 'conv_small')
    return _Built(_randn_sets({'x': (B, cin, H, W)}, 62), call, check, {'x': lambda t, dev: _act(t, dev, cin + 4)})


# ==================================================================================================== normalisation / resampling
@case('gn_stats')
def _():            # HW = 25 * 41 = 1025: the two-kernel reduction with a last chunk of one pixel
    def check(out, d):
        _stats_close(out, d['x'], 'gn_stats')
    return _Built(_randn_sets({'x': (2, 32, 25, 41)}, 71, 2.0, 5.0), lambda ins, dev: ops.gn_stats(ins['x']), check, {'x': _act})


def _gn_relu64(x, gamma, beta):
    m, r = _gn_ref(x)
    st = torch.stack([m, r], 2).float()
    y = F.relu((x.double() - st[..., 0].double()[:, :, None, None]) * st[..., 1].double()[:, :, None, None] * gamma.double().view(1, -1, 1, 1)
               + beta.double().view(1, -1, 1, 1))
    return y, st


def _gn_terms_case(seed, Cc, sizes, Ho, Wo, proj):
    """ops.gn_relu_upsample (one term, lm_gn_relu_upsample) or gn_relu_upsample_sum of len(sizes) terms, with the 1x1 projection."""
    B = 2
    g = _g(seed)
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1
    w1, b1 = torch.randn(5, Cc, 1, 1, generator=g) / Cc ** 0.5, torch.randn(5, generator=g)
    const = {}

    def make(k):
        gk = _g(seed + 1000 * k)
        d = {}
        for i, (h, w) in enumerate(sizes):
            x = torch.randn(B, Cc, h, w, generator=gk) * 2 + 1
            d[f'x{i}'], d[f'st{i}'] = x, _gn_relu64(x, gamma, beta)[1]
        return d

    def call(ins, dev):
        if not const:
            const.update(g=gamma.to(dev), b=beta.to(dev), w16=ops.pack_small(w1.to(dev)), b1=b1.to(dev))
        terms = [(ins[f'x{i}'], ins[f'st{i}']) for i in range(len(sizes))]
        if proj is None:
            return ops.gn_relu_upsample(*terms[0], const['g'], const['b'], (Ho, Wo))
        if not proj:
            return ops.gn_relu_upsample_sum(terms, const['g'], const['b'], (Ho, Wo))
        return dict(zip(('sum', 'proj'), ops.gn_relu_upsample_sum(terms, const['g'], const['b'], (Ho, Wo), proj=(const['w16'], const['b1'], 5))))

    def check(out, d):
        ref = sum(_up(_gn_relu64(d[f'x{i}'], gamma, beta)[0], Ho, Wo) for i in range(len(sizes)))
        if not proj:
            return _close(out, ref, 1e-5, 'gn_relu_upsample(_sum)')
        _close(out['sum'], ref, 1e-5, 'gn sum')
        _close(out['proj'], torch.einsum('oc,bchw->bohw', w1[:, :, 0, 0].double(), ref) + b1.double().view(1, -1, 1, 1), 1e-5, 'gn sum conv1x1')
    return _Built(make, call, check, {f'x{i}': _act for i in range(len(sizes))})


@case('gn_relu_upsample')
def _():
    return _gn_terms_case(72, 32, [(7, 9)], 15, 18, None)


@case('gn_relu_upsample_sum')
def _():            # two terms: the generic kernel
    return _gn_terms_case(73, 32, [(9, 11), (19, 23)], 37, 45, False)


@case('gn_relu_upsample_sum_conv1x1')
def _():            # s2 + up(s3) + s4 with the projection: gn_sum3_lds_kernel
    return _gn_terms_case(74, 32, [(37, 45), (19, 23), (37, 45)], 37, 45, True)


@case('upsample_bilinear')
def _():
    Hi, Wi, Ho, Wo, Cc = 6, 5, 13, 13, 12

    def call(ins, dev):
        return {'y': ops.upsample_nhwc(ins['x'], (Ho, Wo), add=ins['add']), 'chw': ops.upsample_to_chw(ins['x'], (Ho, Wo))}

    def check(out, d):
        ref = _up(d['x'].double(), Ho, Wo)
        _close(out['y'], ref + d['add'].double(), 1e-5, 'upsample + add')
        _close(out['chw'], ref, 1e-5, 'upsample to chw')
    return _Built(_randn_sets({'x': (2, Cc, Hi, Wi), 'add': (2, Cc, Ho, Wo)}, 75), call, check,
                  {'x': lambda t, dev: _act(t, dev, Cc + 8), 'add': _act})


@case('upsample_bicubic')
def _():
    def check(out, d):
        _close(out, F.interpolate(d['x'].double(), size=(20, 23), mode='bicubic', align_corners=False), 1e-5, 'bicubic')
    return _Built(_randn_sets({'x': (2, 8, 9, 11)}, 76), lambda ins, dev: ops.upsample_bicubic(ins['x'], (20, 23)), check, {'x': _act})


@case('layernorm')
def _():
    D = 512
    g = _g(77)
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    const = {}

    def call(ins, dev):
        if not const:
            const.update(g=gamma.to(dev), b=beta.to(dev))
        return ops.layernorm(ins['x'], const['g'], const['b'])

    def check(out, d):
        _close(out, F.layer_norm(d['x'].double(), (D,), gamma.double(), beta.double(), 1e-5), 1e-5, 'layernorm')
    return _Built(_randn_sets({'x': (37, D)}, 77, 3.0, 1.0), call, check)


@case('unpatchify')
def _():
    B, G, P, Cc = 2, 5, 3, 7

    def check(out, d):
        assert torch.equal(out, d['tok'].view(B, G, G, P, P, Cc).permute(0, 5, 1, 3, 2, 4).reshape(B, Cc, G * P, G * P))
    return _Built(_randn_sets({'tok': (B, G * G, P * P * Cc)}, 78), lambda ins, dev: ops.unpatchify(ins['tok'], B, G, P, Cc), check)


@case('token_mix')
def _():
    B, K, M, N = 2, 37, 70, 96
    g = _g(79)
    w = torch.randn(M, K, generator=g) / K ** 0.5
    bias = torch.randn(M, generator=g)
    const = {}

    def call(ins, dev):
        if not const:
            const.update(wt=ops.pack_token_mix(w.to(dev)), b=bias.to(dev))
        return ops.token_mix(ins['x'], const['wt'], M, const['b'], B, res=ins['res'])

    def check(out, d):
        ref = torch.einsum('mk,bkn->bmn', w.double(), d['x'].double().view(B, K, N)) + bias.double()[None, :, None] + d['res'].double().view(B, M, N)
        _close(out, ref.reshape(B * M, N), 1e-5, 'token_mix')
    return _Built(_randn_sets({'x': (B * K, N), 'res': (B * M, N)}, 79), call, check)


def _attn_ref(qkv, B, N, heads, valid=None):
    q, k, v = [z.reshape(B, N, heads, 64).transpose(1, 2).double() for z in qkv.chunk(3, dim=-1)]
    s = q @ k.transpose(-1, -2) * 0.125
    if valid is not None:
        s = s.masked_fill(~valid.bool().view(B, 1, 1, N), float('-inf'))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * N, heads * 64)


@case('attention')
def _():            # N = 37: attention_kernel
    B, N, heads = 2, 37, 2

    def check(out, d):
        _close(out, _attn_ref(d['qkv'], B, N, heads), 1e-5, 'attention')
    return _Built(_randn_sets({'qkv': (B * N, 3 * heads * 64)}, 81, 1.5), lambda ins, dev: ops.attention(ins['qkv'], B, N, heads, 64, 0.125), check)


@case('attention_masked')
def _():
    B, N, heads = 2, 7, 2
    valid = torch.tensor([[1, 0, 1, 0, 1, 0, 1], [0, 1, 0, 1, 0, 1, 0]], dtype=torch.int32)
    const = {}

    def call(ins, dev):
        if not const:
            const.update(v=valid.to(dev))
        return ops.attention(ins['qkv'], B, N, heads, 64, 0.125, const['v'])

    def check(out, d):
        _close(out, _attn_ref(d['qkv'], B, N, heads, valid), 1e-5, 'attention masked')
    return _Built(_randn_sets({'qkv': (B * N, 3 * heads * 64)}, 82), call, check)


# ==================================================================================================== column-proposal head
def _tokens_ref(row, seg, P, pw, hb, seg_bias):
    """The seg-weighted proposal tokens of one image in fp64, as tests/test_gpu_head_geometry.py restates them (seg None: raw windows)."""
    Cc, Hr, Wr = row.shape
    fw = pw + 2 * hb
    rowp = F.pad(row.double(), (hb, hb + pw * P, 0, 0))
    toks = []
    for p in range(P):
        win = rowp[:, :, pw * p: pw * p + fw]
        if seg is not None:
            segp = F.pad(seg.double(), (2 * hb, 2 * hb + 2 * pw * P, 0, 0), value=seg_bias)
            up = F.interpolate(segp[None, None, :, 2 * pw * p: 2 * pw * p + 2 * fw], size=(8 * Hr, 8 * fw), mode='bilinear', align_corners=True)
            win = win * F.avg_pool2d(up, 8)[0]
        toks.append(win.permute(1, 0, 2).reshape(Hr, Cc * fw))
    return torch.cat(toks)


@case('head_tokens')
def _():
    B, Hr, P, pw, hb = 2, 25, 12, 2, 4

    def call(ins, dev):
        return {'seg': ops.head_tokens(ins['seg'], ins['row'], P, pw, hb, -0.37), 'window': ops.head_tokens(None, ins['row'], P, pw, hb, 0.0)}

    def check(out, d):
        for b in range(B):
            sl = slice(b * P * Hr, (b + 1) * P * Hr)
            _close(out['seg'][sl], _tokens_ref(d['row'][b], d['seg'][b, 0], P, pw, hb, -0.37), 1e-5, f'tokens b={b}')
            _close(out['window'][sl], _tokens_ref(d['row'][b], None, P, pw, hb, 0.0), 1e-5, f'window tokens b={b}')
    return _Built(_randn_sets({'row': (B, 16, Hr, Hr), 'seg': (B, 1, 2 * Hr, 2 * Hr)}, 83), call, check, {'row': _act})


@case('head_stage2')
def _():
    B, P, R, D = 1, 5, 37, 100
    M = B * P * R
    g = _g(84)
    w2, b2 = torch.randn(23, D, generator=g) / 10, torch.randn(23, generator=g)
    const = {}

    def call(ins, dev):
        if not const:
            const.update(w=w2.to(dev), b=b2.to(dev))
        return dict(zip(('ext2', 'cls2', 'off2'), ops.head_stage2(ins['hid'], D, const['w'], const['b'], B, P, R)))

    def check(out, d):
        h, w, b = d['hid'].double(), w2.double(), b2.double()
        for k, (lo, hi, c) in {'ext2': (0, 3, 0), 'cls2': (3, 13, 1), 'off2': (13, 23, 2)}.items():
            _close(out[k].reshape(M, hi - lo), h[:, c * D:(c + 1) * D] @ w[lo:hi].t() + b[lo:hi], 1e-5, k)
    return _Built(_randn_sets({'hid': (M, 3 * D)}, 84), call, check)


@case('head_proposal_conf')
def _():
    B, P, L = 2, 5, 1000
    g = _g(85)
    wt, bias = torch.randn(2, L, generator=g) / L ** 0.5, torch.randn(2, generator=g)
    const = {}

    def call(ins, dev):
        if not const:
            const.update(w=wt.to(dev), b=bias.to(dev))
        return ops.head_proposal_conf(ins['tok'], const['w'], const['b'], B, P)

    def check(out, d):
        _close(out, (d['tok'].double() @ wt.double().t() + bias.double()).view(B, P, 2), 1e-5, 'proposal_conf')
    return _Built(_randn_sets({'tok': (B * P, L)}, 85), call, check)


@case('head_endpoint')
def _():
    from test_endpoint_mode_cpu import endpoint_ref64
    from test_gpu_endpoint_mode import _endpoint_module
    ep = _endpoint_module(5)
    const = {}

    def call(ins, dev):
        if not const:
            with torch.no_grad():
                const.update(p=[t.to(dev) for t in ops.pack_head_endpoint(ep[0], ep[2], ep[3])])
        return ops.head_endpoint(ins['col'], ins['x'], const['p'])

    def check(out, d):
        _close(out, endpoint_ref64(d['col'], d['x'], ep), 1e-5, 'head_endpoint')
    return _Built(_randn_sets({'col': (2, 16, 9, 11), 'x': (2, 1, 35, 41)}, 86), call, check, {'col': lambda t, dev: _act(t, dev, 20)})


# ==================================================================================================== decode
@case('decode_proposals')
def _():
    from test_gpu_1_entry_points import _oracle_column_decode
    B, P, R = 2, 72, 6

    def make(k):
        g = _g(702 + 1000 * k)
        return {'pconf': _quarter_grid(torch.randn(B, P, 2, generator=g) * 2), 'ext2': _quarter_grid(torch.randn(B, P, R, 3, generator=g) * 2),
                'cls2': _quarter_grid(torch.randn(B, P, R, 10, generator=g) * 2).clamp(-8, 8),
                'off2': _quarter_grid(torch.rand(B, P, R, 10, generator=g) * 3 - 1)}

    def call(ins, dev):
        return dict(zip(('prop_conf', 'v_ext', 'cls_conf', 'cls_idx', 'cls_offset'),
                        ops.decode_proposals(ins['pconf'], ins['ext2'], ins['cls2'], ins['off2'], 0.2, 2, 4)))

    def check(out, d):
        ref = _oracle_column_decode(d['pconf'], d['ext2'], d['cls2'], d['off2'], torch.zeros(B, 3, 8, 8))
        e = d['ext2'].double().softmax(3)
        d12 = e[..., 1] - e[..., 2]
        near = ((d12.abs() < 1e-6) & (d12 != 0)) | ((e[..., 1:] - 0.2).abs() < 1e-6).any(-1)
        assert int(near.sum()) == 0, 'the quarter grid should leave no near-tie of the existence decision'
        assert torch.equal(out['cls_idx'], ref['cls_idx'].to(torch.int32)) and torch.equal(out['cls_offset'], ref['cls_offset'])
        assert torch.equal(out['v_ext'], ref['prop_v_ext'].float())
        _close(out['prop_conf'], d['pconf'].double().softmax(2), 1e-6, 'prop_conf')
        _close(out['cls_conf'], d['cls2'].double().softmax(3), 1e-6, 'cls_conf')
    return _Built(make, call, check)


@case('decode_orient')
def _():
    B, Cc, H, W = 2, 11, 37, 45

    def make(k):
        g = _g(11 + 1000 * k)
        x = torch.randint(0, 3, (B, Cc, H, W), generator=g).float() * 0.5
        x[torch.rand(B, Cc, H, W, generator=g) < 0.1] = float('-inf')
        return {'x': x}

    def check(out, d):
        assert torch.equal(out, torch.from_numpy(np.argmax(d['x'].numpy(), axis=1).astype(np.uint8)))
    return _Built(make, lambda ins, dev: ops.decode_orient(ins['x']), check, {'x': lambda t, dev: _act(t, dev, 16)})


@case('decode_semantic')
def _():
    from test_gpu_1_entry_points import _semantic_logits
    B, H, W = 2, 48, 40

    def call(ins, dev):
        return dict(zip(('sem', 'biseg', 'rows'), ops.decode_semantic(ins['x'], 0.2)))

    def check(out, d):
        s = d['x'].double().softmax(1)
        s1, s2 = s[:, 1], s[:, 2]
        tie = s1 == s2
        clear = tie | (torch.minimum((s1 - s2).abs(), torch.minimum((s1 - 0.2).abs(), (s2 - 0.2).abs())) > 1e-6)
        want = torch.zeros(B, H, W, dtype=torch.uint8)
        want[(s1 > s2) & (s1 > 0.2)] = 1
        want[(s2 > s1) & (s2 > 0.2)] = 2
        assert int((~clear).sum()) <= 4 and torch.equal(out['sem'][clear], want[clear])
        _close(out['biseg'], s1 + s2, 1e-5, 'biseg')
        assert torch.equal(out['rows'], out['biseg'][:, 3::8])
    return _Built(lambda k: {'x': _semantic_logits(B, H, W, 627 + k)}, call, check)


@case('endp_topk')
def _():            # 64 x 64, crop 4: a plateau of 600 pixels on one score above everything else, K = 64 of them: the ties kernel
    B, H, W, clip, K = 2, 64, 64, 4, 64

    def make(k):
        x = torch.randn((B, 1, H, W), generator=_g(5 + 1000 * k)) - 4.0
        x[:, 0, 10 + k:30 + k, 20:50] = 2.5
        return {'x': x}

    def call(ins, dev):
        return dict(zip(('idx', 'score', 'status'), ops.endp_topk(ins['x'], K=K, clip=clip)))

    def check(out, d):
        assert int(out['status'].max()) == 0
        for b in range(B):
            s = torch.sigmoid(d['x'][b, 0, clip:H - clip, clip:W - clip]).numpy().reshape(-1)
            want = np.lexsort((np.arange(s.size), -s.astype(np.float64)))[:K]
            assert np.array_equal(out['idx'][b].numpy(), want), f'tile {b}'
            assert float(np.abs(out['score'][b].numpy() - s[want]).max()) <= 1e-6
    return _Built(make, call, check)


@case('pack_segments')
def _():
    def make(k):
        g = _g(60 + k)
        return {'a': torch.randn(17, generator=g), 'b': torch.randint(-2 ** 31, 2 ** 31 - 1, (144,), generator=g, dtype=torch.int32),
                'c': torch.randn(5, generator=g, dtype=torch.float64)}

    def call(ins, dev):
        block = torch.zeros(1280, device=dev, dtype=torch.uint8)                 # (the gaps between the segments are nobody's to write)
        got, segs = ops.pack_readback([ins['a'], ins['b'], ins['c']], block=block)
        assert got.data_ptr() == block.data_ptr() and segs == [(0, 68), (256, 576), (1024, 40)]
        return block

    def check(out, d):
        hb, covered = out.numpy(), np.zeros(1280, bool)
        for t, (o, nb) in zip((d['a'], d['b'], d['c']), [(0, 68), (256, 576), (1024, 40)]):
            assert np.array_equal(hb[o:o + nb], t.view(torch.uint8).numpy())
            covered[o:o + nb] = True
        assert not hb[~covered].any()
    return _Built(make, call, check)


# ==================================================================================================== RowRef
@case('softmax_rows')
def _():
    rows, cols = 1027, 65

    def call(ins, dev):
        x = ins['x'].clone()                                                     # (the entry works in place)
        _chk(_lib().lm_softmax_rows(_s(), x.data_ptr(), rows, cols))
        return x

    def check(out, d):
        _close(out, d['x'].double().softmax(1), 1e-5, 'softmax_rows')
    return _Built(_randn_sets({'x': (rows, cols)}, 87, 4.0), call, check)


@case('rowref_select')
def _():
    B, H, W, L = 1, 300, 37, 3

    def make(k):
        g = _g(H + W + 1000 * k)
        ext = torch.rand(B, H, L, 2, generator=g) * 0.2
        ext[..., 0] += torch.tensor([0.35, 0.05, 0.35]).view(1, 1, L)
        return {'ext': ext, 'cls': _quarter_grid(torch.rand(B, H, L, W, generator=g) * 2)}

    def call(ins, dev):
        mean = torch.empty((B, L), device=dev)
        valid = torch.empty((B, L), device=dev, dtype=torch.int32)
        corr = torch.empty((B, L, H), device=dev, dtype=torch.int32)
        _chk(_lib().lm_rowref_select(_s(), ins['ext'].data_ptr(), ins['cls'].data_ptr(), mean.data_ptr(), valid.data_ptr(), C.c_float(0.3),
                                     corr.data_ptr(), B, H, W, L))
        return {'mean': mean, 'valid': valid, 'corr': corr}

    def check(out, d):
        mref = d['ext'][..., 0].double().mean(1)
        _close(out['mean'], mref, 1e-5, 'lane mean')
        assert torch.equal(out['valid'], (mref > 0.3).int())
        assert torch.equal(out['corr'], torch.from_numpy(np.argmax(d['cls'].numpy(), axis=3).astype(np.int32)).permute(0, 2, 1))
    return _Built(make, call, check)


@case('rowref_gather_scatter')
def _():
    """The four window entries on one small map: the fixed-width pair (off_grid 2) and the _win pair at off_grid 3; windows over both
    borders, overlapping lanes, tile 1 with no lane selected."""
    from test_gpu_rowref_geometry import _corr, _gather_ref, _scatter_ref
    B, H, W, L = 2, 6, 9, 3

    def make(k):
        g = _g(207 + 1000 * k)
        valid = torch.zeros(B, L, dtype=torch.int32)
        valid[0] = 1
        return {'x': torch.randn(B, H, W, 8, generator=g), 'corr': _corr(B, L, H, W, g), 'valid': valid,
                'tok2': torch.randn(B * L, 8 * H * 5, generator=g), 'tok3': torch.randn(B * L, 8 * H * 7, generator=g)}

    def call(ins, dev):
        Lb, p = _lib(), lambda t: t.data_ptr()
        g2, g3 = torch.empty((B * L, 8 * H * 5), device=dev), torch.empty((B * L, 8 * H * 7), device=dev)
        y2, y3 = torch.empty((B, H, W, 8), device=dev), torch.empty((B, H, W, 8), device=dev)
        _chk(Lb.lm_rowref_gather(_s(), p(ins['x']), p(ins['corr']), p(g2), B, H, W, L))
        _chk(Lb.lm_rowref_gather_win(_s(), p(ins['x']), p(ins['corr']), p(g3), B, H, W, L, 3))
        _chk(Lb.lm_rowref_scatter(_s(), p(ins['x']), p(ins['tok2']), p(ins['corr']), p(ins['valid']), p(y2), B, H, W, L))
        _chk(Lb.lm_rowref_scatter_win(_s(), p(ins['x']), p(ins['tok3']), p(ins['corr']), p(ins['valid']), p(y3), B, H, W, L, 3))
        return {'g2': g2, 'g3': g3, 'y2': y2, 'y3': y3}

    def check(out, d):
        n = {k: v.numpy() for k, v in d.items()}
        bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)
        for og, gk, yk, tk in ((2, 'g2', 'y2', 'tok2'), (3, 'g3', 'y3', 'tok3')):
            assert np.array_equal(bits(out[gk].numpy()), bits(_gather_ref(n['x'], n['corr'], L, og))), f'gather off_grid={og}'
            assert np.array_equal(bits(out[yk].numpy()), bits(_scatter_ref(n['x'], n[tk], n['corr'], n['valid'], og))), f'scatter off_grid={og}'
    return _Built(make, call, check)


@case('rowref_decode')
def _():            # conf and cls_map non-NULL: the two maps the entry zeroes before its kernel
    from oracle import rowref_ref
    B, H, W, L = 2, 16, 24, 3

    def make(k):
        g = _g(334 + 1000 * k)
        ext2 = _quarter_grid(torch.rand(B, H, L, 2, generator=g))
        ext2[:, 0::5, :, 1] = ext2[:, 0::5, :, 0]
        return {'ext2': ext2, 'cls2': _quarter_grid(torch.rand(B, H, L, W, generator=g))}

    def call(ins, dev):
        conf = torch.empty((B, H, W), device=dev, dtype=torch.uint8)
        cmap = torch.empty((B, L + 1, H, W), device=dev, dtype=torch.uint8)
        col = torch.empty((B, L, H), device=dev, dtype=torch.int32)
        _chk(_lib().lm_rowref_decode(_s(), ins['ext2'].data_ptr(), ins['cls2'].data_ptr(), conf.data_ptr(), cmap.data_ptr(), col.data_ptr(),
                                     B, H, W, L))
        return {'conf': conf, 'cls_map': cmap, 'col': col}

    def check(out, d):
        o = {}
        for c in range(L):
            o[f'ext2_{c}'], o[f'cls2_{c}'] = d['ext2'][:, :, c, :], d['cls2'][:, :, c, :]
        conf_ref, cls_ref = rowref_ref.rowref_decode(o, num_cls=L)
        en, cn = d['ext2'].numpy(), d['cls2'].numpy()
        col_ref = np.where(np.argmax(en, axis=3) == 0, np.argmax(cn, axis=3), -1).transpose(0, 2, 1).astype(np.int32)
        assert np.array_equal(out['col'].numpy(), col_ref)
        assert torch.equal(out['conf'], torch.from_numpy(conf_ref).to(torch.uint8))
        assert torch.equal(out['cls_map'], torch.from_numpy(cls_ref).to(torch.uint8))
    return _Built(make, call, check)


# ==================================================================================================== primitives
def _u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32))


@case('exclusive_scan')
def _():            # n = 4097: three kernels over two levels
    n = 4097

    def make(k):
        return {'x': _u32(np.random.default_rng(n + k).integers(0, 2 ** 31, size=n, dtype=np.int64).astype(np.uint32))}

    def check(out, d):
        x = d['x'].numpy().view(np.uint32)
        want = np.zeros(n, dtype=np.uint32)
        want[1:] = np.cumsum(x[:-1].astype(np.uint64)).astype(np.uint32)
        np.testing.assert_array_equal(out.numpy().view(np.uint32), want)
    return _Built(make, lambda ins, dev: ops.exclusive_scan_u32(ins['x']), check)


@case('sort_pairs')
def _():            # end_bit 24: three passes, the result ends in the workspace and is copied back; 32: four passes, none
    n = 4097

    def make(k):
        key = np.random.default_rng(7 + k).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        key[::5] = key[0]
        return {'k': _u32(key), 'v': _u32(np.arange(n, dtype=np.uint32))}

    def call(ins, dev):
        out = {}
        for eb in (24, 32):
            out[f'k{eb}'], out[f'v{eb}'] = ops.sort_pairs_u32_(ins['k'].clone(), ins['v'].clone(), eb)
        return out

    def check(out, d):
        key, v = d['k'].numpy().view(np.uint32), d['v'].numpy().view(np.uint32)
        for eb in (24, 32):
            order = np.argsort(key & np.uint32((1 << eb) - 1 if eb < 32 else 0xFFFFFFFF), kind='stable')
            np.testing.assert_array_equal(out[f'v{eb}'].numpy().view(np.uint32), v[order])
            np.testing.assert_array_equal(out[f'k{eb}'].numpy().view(np.uint32), key[order])
    return _Built(make, call, check)


# ==================================================================================================== tiles of points
T = 64                                                             # H = W of every tile below


def _tiles3():
    from test_gpu_intensity import FAR, _axis_tile, _rot_tile
    return [_axis_tile(), FAR, _rot_tile()]                        # the middle tile holds no point


def _clouds(seed, counts, tiles, k):
    from test_gpu_intensity import KINDS, _cloud
    parts = [_cloud(seed + 10 * t + 1000 * k, n, tiles[t], KINDS['uniform_u16'], T=T) for t, n in enumerate(counts)]
    return np.concatenate(parts), [0] + np.cumsum(counts).tolist()


@case('bev_raster')
def _():
    import intensity_ref as ir
    tiles, counts = _tiles3(), (3000, 0, 2000)
    offs = _clouds(1, counts, tiles, 0)[1]
    scales = [249.0 / 10000.0, None, 0.0]

    def call(ins, dev):
        chw, u8 = ops.bev_raster_batch(ins['pts'], offs, tiles, T, T, want_u8=True)
        return {'chw': chw, 'u8': u8, 'scaled': ops.bev_raster_batch(ins['pts'], offs, tiles, T, T, u8_only=True, inten_scale=scales)}

    def check(out, d):
        want = ir.raster(d['pts'].numpy(), offs, tiles, T, T)
        assert int((want.sum(3) > 0).sum()) > 1000 and not want[1].any()
        assert np.array_equal(out['u8'].numpy(), want)
        assert np.array_equal(out['chw'].numpy(), want.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))
        assert np.array_equal(out['scaled'].numpy(), ir.raster(d['pts'].numpy(), offs, tiles, T, T, scales))
    return _Built(lambda k: {'pts': torch.from_numpy(_clouds(1, counts, tiles, k)[0])}, call, check)


@case('tile_ingest')
def _():
    B, H, W = 2, 17, 29

    def check(out, d):
        _close(out, d['u'][..., :3].permute(0, 3, 1, 2).double() / 255.0, 1e-7, 'tile_ingest')
    return _Built(lambda k: {'u': torch.randint(0, 256, (B, H, W, 4), generator=_g(17 + k), dtype=torch.uint8)},
                  lambda ins, dev: ops.tile_ingest(ins['u']), check)


@case('tile_gap')
def _():
    import gapfill_ref as gf
    B, H, W = 2, 40, 48

    def make(k):
        g = _g(90 + k)
        u = torch.randint(1, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
        u[torch.rand(B, H, W, generator=g) > 0.08] = 0
        return {'u': u}

    def call(ins, dev):
        return {'hist': ops.tile_gap_hist(ins['u'], 4), 'fill': ops.tile_gap_fill(ins['u'], [3, 0])}

    def check(out, d):
        assert np.array_equal(out['hist'].numpy(), gf.hist(d['u'].numpy(), 4).astype(np.int32))
        assert np.array_equal(out['fill'].numpy(), gf.fill(d['u'].numpy(), [3, 0]))
    return _Built(make, call, check)


@case('strip_bin')
def _():
    import ground_ref as gr
    tiles, counts = _tiles3(), (3000, 0, 2000)

    def make(k):
        pts = _clouds(2, counts, tiles, k)[0]
        return {'pts': torch.from_numpy(pts[np.random.RandomState(k).permutation(len(pts))])}      # one cloud, the tiles find their points

    def call(ins, dev):
        binned, offs = ops.strip_bin_points(ins['pts'], tiles, T, T, z_range=(-10.0, 10.0))
        return {'binned': binned, 'offsets': torch.tensor(offs, dtype=torch.int64)}

    def check(out, d):
        pts = d['pts'].numpy()
        idx = [np.flatnonzero(gr.window(pts, p, T, T)[0]) for p in tiles]
        assert out['offsets'].tolist() == [0] + np.cumsum([len(i) for i in idx]).tolist() and len(idx[0]) > 500 and len(idx[1]) == 0
        assert np.array_equal(out['binned'].numpy().view(np.uint32), pts[np.concatenate(idx)].view(np.uint32))
    return _Built(make, call, check)


@case('tile_ground')
def _():            # B = 3 with an empty tile; ground_select with the host copy of its offsets (ops always asks for it)
    import ground_ref as gr
    tiles, counts = _tiles3(), (3000, 0, 2000)
    offs = _clouds(3, counts, tiles, 0)[1]

    def call(ins, dev):
        ground, gmin, cmin = ops.tile_ground(ins['pts'], offs, tiles, T, T, cell_px=16, want_cell_min=True)
        kept, koffs = ops.ground_select(ins['pts'], offs, tiles, ground, T, T, 16, (-0.05, 0.3))
        return {'ground': ground, 'ground_min': gmin, 'cell_min': cmin, 'kept': kept, 'kept_offsets': torch.tensor(koffs, dtype=torch.int64)}

    def check(out, d):
        pts = d['pts'].numpy()
        bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
        rg, rmin, rc = gr.tile_ground(pts, offs, tiles, T, T, 16)
        for k, r in (('cell_min', rc), ('ground', rg), ('ground_min', rmin)):
            assert np.array_equal(bits(out[k].numpy()), bits(r)), k
        want, woffs = gr.select(pts, offs, tiles, out['ground'].numpy(), T, T, 16, (-0.05, 0.3))
        assert out['kept_offsets'].tolist() == woffs.tolist() and 0 < woffs[-1] < len(pts) and woffs[1] == woffs[2]
        assert np.array_equal(bits(out['kept'].numpy()), bits(want))
    return _Built(lambda k: {'pts': torch.from_numpy(_clouds(3, counts, tiles, k)[0])}, call, check)


@case('tile_intensity_window')
def _():            # points in two of three tiles: both count passes run, around the locate and resolve kernels
    import intensity_ref as ir
    tiles, counts = _tiles3(), (3000, 0, 2000)
    offs = _clouds(4, counts, tiles, 0)[1]

    def call(ins, dev):
        return dict(zip(('window', 'count', 'hist'), ops.tile_intensity_window(ins['pts'], offs, tiles, T, T, (1.0, 99.9), want_hist=True)))

    def check(out, d):
        rw, rc, rh = ir.window(d['pts'].numpy(), offs, tiles, T, T, (1.0, 99.9))
        assert rc[0] > 500 and rc[1] == 0 and rw[1].tolist() == [-1, -1]
        for k, r in (('window', rw), ('count', rc), ('hist', rh)):
            assert np.array_equal(out[k].numpy(), r), k
    return _Built(lambda k: {'pts': torch.from_numpy(_clouds(4, counts, tiles, k)[0])}, call, check)


@case('drape_vertices')
def _():
    """Two tiles over the same window: every vertex lies in both; within a tile two identical vertices and one whose window overlaps
    theirs."""
    import drape_ref as dr
    from test_gpu_intensity import _axis_tile
    tiles, counts = [_axis_tile(), _axis_tile()], (3000, 2500)
    offs = _clouds(5, counts, tiles, 0)[1]
    verts = np.asarray([(0, 0), (T - 1, T - 1), (40, 40), (40, 40), (40, 43), (7, 20), (8, 22)] * 2, np.int32)
    voffs = [0, 7, 14]

    def call(ins, dev):
        return dict(zip(('z', 'npix', 'pixel_min'), ops.drape_vertices(ins['pts'], offs, tiles, verts, voffs, T, T, radius_px=4, want_pixel_min=True)))

    def check(out, d):
        rz, rn, rp = dr.drape_vertices(d['pts'].numpy(), offs, tiles, verts, voffs, T, T, 4)
        bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
        assert np.array_equal(out['npix'].numpy(), rn) and (rn[2:5] > 0).all()
        assert np.array_equal(bits(out['z'].numpy()), bits(rz)) and np.array_equal(bits(out['pixel_min'].numpy()), bits(rp))
    return _Built(lambda k: {'pts': torch.from_numpy(_clouds(5, counts, tiles, k)[0])}, call, check)


# ==================================================================================================== sparse voxels
@case('voxelize')
def _():
    """Three calls, chained through device row counters: a sample with points (row_base NULL), a sample without (its row_end is a
    device-to-device copy of row_base), and a sample without points and without a base (its row_end is a memset)."""
    from oracle import lidar_ref
    lo, vs, grid, n, cap = [-3.0, -2.0, -1.0], [0.5, 0.25, 0.5], [12, 10, 4], 2000, 480

    def make(k):
        rng = np.random.RandomState(31 + k)
        return {'p': torch.from_numpy((rng.uniform(-0.1, 1.1, (n, 4)) * [6.0, 2.5, 2.0, 1.0] + [-3.0, -2.0, -1.0, 0.0]).astype(np.float32))}

    def work(dev):
        return {'ws': torch.empty(_lib().lm_voxelize_workspace_bytes(n), device=dev, dtype=torch.uint8)}

    def call(ins, dev, wk):
        L, p, ws = _lib(), ins['p'], wk['ws']
        need = ws.numel()
        feats, coords = torch.zeros((cap, 16), device=dev), torch.zeros((cap, 4), device=dev, dtype=torch.int32)
        ends = torch.empty((3,), device=dev, dtype=torch.int32)
        geo = ((C.c_float * 3)(*lo), (C.c_float * 3)(*vs), (C.c_int * 3)(*grid))
        tail = (cap, feats.data_ptr(), 16, coords.data_ptr())
        _chk(L.lm_voxelize_hard(_s(), p.data_ptr(), n, *geo, 3, 1000, 0, None, *tail, ends[0:1].data_ptr(), 0, ws.data_ptr(), need))
        _chk(L.lm_voxelize_hard(_s(), None, 0, *geo, 3, 1000, 1, ends[0:1].data_ptr(), *tail, ends[1:2].data_ptr(), 0, ws.data_ptr(), need))
        _chk(L.lm_voxelize_hard(_s(), None, 0, *geo, 3, 1000, 2, None, *tail, ends[2:3].data_ptr(), 0, ws.data_ptr(), need))
        return {'feats': feats, 'coords': coords, 'ends': ends}

    def check(out, d):
        f_ref, c_ref = lidar_ref.voxelize_ref([d['p'].numpy()], lo, vs, grid, 3, 1000)
        V = len(c_ref)
        assert 100 < V <= cap and out['ends'].tolist() == [V, V, 0]
        assert np.array_equal(out['coords'].numpy()[:V], c_ref) and not out['coords'].numpy()[V:].any()
        f = out['feats'].numpy()
        assert np.array_equal(f[:V, :4].view(np.int32), np.ascontiguousarray(f_ref, np.float32).view(np.int32)) and not f[:, 4:].any()
    return _Built(make, call, check, work=work)


@case('sparse_index')
def _():
    """lm_sparse_grid_build, the raw lm_sparse_conv_outputs (the ops wrapper reads the count back) and lm_sparse_rulebook of the
    submanifold geometry on the same n active sites."""
    import sparse_ref as R
    B, shape, n = 2, (4, 9, 8), 150
    D, H, W = shape
    geom = ((3, 3, 3), (2, 2, 2), (1, 1, 1))
    oshape = R.out_shape_of(shape, *geom)
    cells = B * oshape[0] * oshape[1] * oshape[2]

    def make(k):
        g = _g(17 + k)
        c = torch.randperm(B * D * H * W, generator=g)[:n]
        return {'coords': torch.stack([c // (D * H * W), c // (H * W) % D, c // W % H, c % W], 1).int()}

    def work(dev):
        return {'ws': torch.empty(_lib().lm_sparse_conv_outputs_workspace_bytes(cells), device=dev, dtype=torch.uint8)}

    def call(ins, dev, wk):
        L, co, ws = _lib(), ins['coords'], wk['ws']
        grid = ops.sparse_grid(co, B, shape)
        need = ws.numel()
        og = torch.empty((B,) + tuple(oshape), device=dev, dtype=torch.int32)
        oc, cnt = torch.zeros((cells, 4), device=dev, dtype=torch.int32), torch.zeros((1,), device=dev, dtype=torch.int32)
        _chk(L.lm_sparse_conv_outputs(_s(), co.data_ptr(), n, B, ops._ksp(*geom), *oshape, og.data_ptr(), oc.data_ptr(), cells, cnt.data_ptr(),
                                      ws.data_ptr(), need))
        return {'grid': grid, 'out_grid': og, 'out_coords': oc, 'count': cnt, 'nbr': ops.sparse_rulebook(co, grid, *R.SUBM)}

    def check(out, d):
        inc = d['coords'].numpy()
        assert np.array_equal(out['grid'].numpy(), R.grid_ref(inc, B, shape))
        _, oc, og = R.conv_outputs_ref(inc, B, shape, *geom)
        assert int(out['count']) == len(oc) > 10 and np.array_equal(out['out_coords'].numpy()[:len(oc)], oc)
        assert np.array_equal(out['out_grid'].numpy(), og) and not out['out_coords'].numpy()[len(oc):].any()
        assert np.array_equal(out['nbr'].numpy(), R.rulebook_ref(inc, inc, shape, *R.SUBM))
    return _Built(make, call, check, work=work)


@case('conv_gather')
def _():
    V, M, cin, cout, taps = 200, 333, 16, 16, 27
    g = _g(cin + cout + taps)
    w = torch.randn(3, 3, 3, cin, cout, generator=g) / (taps * cin) ** 0.5
    sh = torch.randn(cout, generator=g)
    const = {}

    def make(k):
        gk = _g(59 + 1000 * k)
        nbr = torch.randint(0, V, (M, taps), generator=gk, dtype=torch.int32)
        nbr[torch.rand(M, taps, generator=gk) < 0.35] = -1
        return {'x': torch.randn(V, cin, generator=gk), 'nbr': nbr}

    def call(ins, dev):
        if not const:
            const.update(wp=ops.pack_sparse(w.to(dev)), sh=sh.to(dev))
        return ops.conv_gather(ins['x'], ins['nbr'], const['wp'], cin, cout, shift=const['sh'])

    def check(out, d):
        xe = torch.cat([d['x'].double(), torch.zeros(1, cin, dtype=torch.float64)])
        ref = torch.einsum('mtc,tco->mo', xe[torch.where(d['nbr'] < 0, V, d['nbr']).long()], w.double().reshape(taps, cin, cout)) + sh.double()
        _close(out[:, :cout], ref, 1e-5, 'conv_gather')
    return _Built(make, call, check)


@case('sparse_to_dense')
def _():
    B, D, H, W, Cc, n = 2, 3, 19, 23, 20, 300

    def make(k):
        g = _g(70 + k)
        c = torch.randperm(B * D * H * W, generator=g)[:n]
        return {'coords': torch.stack([c // (D * H * W), c // (H * W) % D, c // W % H, c % W], 1).int(), 'feats': torch.randn(n, Cc, generator=g)}

    def check(out, d):
        co = d['coords'].long()
        dense = torch.zeros(B, Cc, D, H, W)
        dense[co[:, 0], :, co[:, 1], co[:, 2], co[:, 3]] = d['feats']
        assert torch.equal(out, torch.flip(dense.view(B, Cc * D, H, W), dims=[2]))
    return _Built(make, lambda ins, dev: ops.sparse_to_dense(ins['feats'], ins['coords'], B, (D, H, W), Cc, True), check)


# ==================================================================================================== LAS records and line tables
def _rec_sets(n, seed):
    """make(k) -> {'rec': the padded flat bytes of n format-7 records of 37 bytes around label_ref's lines}, and the [n, 37] records of
    set k (tests/test_gpu_colour.py builds them: positions on the 1/1024 m lattice, RGB, class 2 / 7)."""
    from test_gpu_colour import _flat, _random
    recs = [_random(7, 1, n, seed + k) for k in range(3)]
    return (lambda k: {'rec': torch.from_numpy(_flat(recs[k]))}), recs


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


@case('las_decode')
def _():
    """lm_las_decode_points through las_io.decode_points, and the raw lm_las_decode_select with class_hist (the package wrapper reads
    `kept` back on every call): on the n records, and once with n = 0, where the entry only zeroes `kept` and `class_hist`."""
    import label_ref as lr
    from lanemapping_amd import las_io
    from test_gpu_colour import OFFSET, SCALE, _passes
    n, rl = 1001, 37
    make, recs = _rec_sets(n, 300)
    select = las_io.PointFilter(classes=[2], drop_withheld=False)
    sel = select.for_format(7).as_struct()

    def work(dev):
        return {'ws': torch.empty(int(_lib().lm_las_select_workspace_bytes(n)), device=dev, dtype=torch.uint8)}

    def call(ins, dev, wk):
        L, rec, ws = _lib(), ins['rec'], wk['ws']
        plain = las_io.decode_points(rec, rl, n, SCALE, OFFSET, lr.SHIFT, normalise=False)
        need = ws.numel()
        assert 0 < int(L.lm_las_select_workspace_bytes(0)) <= need
        out, meta = torch.zeros((n, 4), device=dev), torch.empty((257,), device=dev, dtype=torch.int64)
        meta0 = torch.empty((257,), device=dev, dtype=torch.int64)
        head = (_d3(SCALE), _d3(OFFSET), _d3(lr.SHIFT), las_io.INTEN_MIN, las_io.INTEN_MAX, 0, C.byref(sel), ws.data_ptr(), need)
        _chk(L.lm_las_decode_select(_s(), rec.data_ptr(), rl, 7, n, *head, out.data_ptr(), meta.data_ptr(), meta.data_ptr() + 8))
        _chk(L.lm_las_decode_select(_s(), None, rl, 7, 0, *head, None, meta0.data_ptr(), meta0.data_ptr() + 8))
        return {'plain': plain, 'kept': out, 'meta': meta, 'meta_of_no_records': meta0}

    def check(out, d):
        dec, ok = lr.decode_f32(recs[0], SCALE, OFFSET, lr.SHIFT), _passes(recs[0], 7, select)
        assert np.array_equal(out['plain'].numpy().view(np.int32), dec.view(np.int32))
        kept = int(out['meta'][0])
        assert kept == int(ok.sum()) and 0 < kept < n
        assert np.array_equal(out['kept'].numpy()[:kept].view(np.int32), dec[ok].view(np.int32)) and not out['kept'].numpy()[kept:].any()
        assert np.array_equal(out['meta'].numpy()[1:], np.bincount(recs[0][:, 16], minlength=256))
        assert not out['meta_of_no_records'].numpy().any()
    return _Built(make, call, check, work=work)


@case('label')
def _():
    """lm_label_points on 3000 points around label_ref's lines; lm_las_label_records with line and counts (counts non-NULL: the
    histogram the entry zeroes first)."""
    import label_ref as lr
    from lanemapping_amd import las_io
    from test_gpu_colour import OFFSET, SCALE, _header, _scene
    seg = _scene()[0]
    n = 513
    make_rec, recs = _rec_sets(n, 400)
    pts = [lr.scene_points(seg, seed=50 + k) for k in range(3)]
    m = min(len(p) for p in pts)
    labels = las_io.MarkingLabels(lr.HW, lr.ZTOL)
    const = {}

    def call(ins, dev):
        if not const:
            const.update(index=ops.line_index(seg, lr.HW, device=dev))
        line, d2 = ops.label_points(ins['pts'], const['index'], lr.ZTOL, want_dist2=True)
        out, counts, rline = las_io.label_records(ins['rec'], _header(7, recs[0]), const['index'], labels, lr.SHIFT, None, want_line=True)
        return {'line': line, 'dist2': d2, 'records': out, 'counts': counts, 'rec_line': rline}

    def check(out, d):
        wl, wd, _ = lr.label_f32(d['pts'].numpy(), seg, lr.HW, lr.ZTOL)
        assert np.array_equal(out['line'].numpy(), wl) and np.array_equal(out['dist2'].numpy().view(np.int32), wd.view(np.int32))
        assert set(np.unique(wl)) >= {0, 1, 2}
        rl_ = lr.label_f32(lr.decode_f32(recs[0], SCALE, OFFSET, lr.SHIFT), seg, lr.HW, lr.ZTOL)[0]
        assert (rl_ > 0).sum() > n // 20 and np.array_equal(out['rec_line'].numpy(), rl_)
        want = lr.patch_records(recs[0], 7, rl_, labels.for_format(7), labels.line_ids)
        assert np.array_equal(out['records'].numpy()[:want.size].reshape(want.shape), want)
        assert np.array_equal(out['counts'].numpy(), np.bincount(rl_, minlength=len(out['counts'])))
    return _Built(lambda k: {'pts': torch.from_numpy(pts[k][:m].copy()), **make_rec(k)}, call, check)


@case('line_profile')
def _():
    """The profile of points, of records, and of records with their colours: each once fresh (accumulate = 0 over an uninitialised
    table) and once more into a copy of that table (accumulate = 1)."""
    import label_ref as lr
    import profile_ref as pr
    from lanemapping_amd import las_io
    from test_gpu_colour import BIN, _device_tables, _header, _scene, _want
    seg, st, bs = _scene()
    n = 513
    make_rec, recs = _rec_sets(n, 500)
    pts = [lr.scene_points(seg, seed=60 + k) for k in range(3)]
    m = min(len(p) for p in pts)
    survey, colour = las_io.MarkingSurvey(BIN, lr.HW, lr.ZTOL), las_io.MarkingColour()
    const = {}

    def call(ins, dev):
        if not const:
            const.update(t=_device_tables(dev))
        index, stations = const['t']
        h = _header(7, recs[0])
        p0 = ops.line_profile(ins['pts'], index, stations, lr.ZTOL)
        p1 = ops.line_profile(ins['pts'], index, stations, lr.ZTOL, out=p0.clone())
        r0 = las_io.profile_records(ins['rec'], h, index, stations, survey, lr.SHIFT)
        r1 = las_io.profile_records(ins['rec'], h, index, stations, survey, lr.SHIFT, out=r0.clone())
        b0, c0 = las_io.profile_colour_records(ins['rec'], h, index, stations, survey, colour, lr.SHIFT)
        b1, c1 = las_io.profile_colour_records(ins['rec'], h, index, stations, survey, colour, lr.SHIFT, out=(b0.clone(), c0.clone()))
        return {'p0': p0, 'p1': p1, 'r0': r0, 'r1': r1, 'b0': b0, 'c0': c0, 'b1': b1, 'c1': c1}

    def check(out, d):
        w0 = pr.profile_f32(d['pts'].numpy(), seg, st, bs, BIN, lr.HW, lr.ZTOL)[0]
        w1 = pr.profile_f32(d['pts'].numpy(), seg, st, bs, BIN, lr.HW, lr.ZTOL, bins=w0.copy())[0]
        assert w0[:, 0].sum() > 100 and np.array_equal(out['p0'].numpy(), w0) and np.array_equal(out['p1'].numpy(), w1)
        wb, wc = _want(recs[0], 7, colour.blue_q)[:2]
        wb2, wc2 = _want(recs[0], 7, colour.blue_q, bins=wb.copy(), colours=wc.copy())[:2]
        assert wb[:, 0].sum() > 20 and wc[:, 0].sum() > 10
        for k, w in (('r0', wb), ('r1', wb2), ('b0', wb), ('b1', wb2), ('c0', wc), ('c1', wc2)):
            assert np.array_equal(out[k].numpy(), w), k
    return _Built(lambda k: {'pts': torch.from_numpy(pts[k][:m].copy()), **make_rec(k)}, call, check)


@case('line_cross')
def _():
    """The cross-sections of points and of records (tests/test_gpu_cross.py's lines and records), each fresh and accumulated."""
    import cross_ref as cr
    import label_ref as lr
    import profile_ref as pr
    import test_gpu_cross as X
    from lanemapping_amd import las_io
    bin, n, npts = pr.BIN_INEXACT, 257, 3000
    seg, scene = X._scene()[1], X._scene()[2]
    st, bs = X._tables(bin)
    cross = las_io.CrossSection(X.PAINT, bin=bin, half_width=X.HW, lateral=X.LQ / 1024, z_tol=X.ZTOL)
    recs = [X._records(None, 7, 1, n, seed=700 + k) for k in range(3)]
    const = {}

    def make(k):
        return {'pts': torch.from_numpy(scene[np.random.RandomState(k).permutation(len(scene))[:npts]].copy()), 'rec': torch.from_numpy(recs[k][1])}

    def call(ins, dev):
        if not const:
            const.update(t=X._device_tables(dev, bin))
        index, stations = const['t']
        h = X._header(7, 37, n)
        p0 = ops.line_cross(ins['pts'], index, stations, X.ZTOL, X.LQ, X.PAINT)
        p1 = ops.line_cross(ins['pts'], index, stations, X.ZTOL, X.LQ, X.PAINT, out=p0.clone())
        r0 = las_io.cross_records(ins['rec'], h, index, stations, cross, None)
        r1 = las_io.cross_records(ins['rec'], h, index, stations, cross, None, out=r0.clone())
        return {'p0': p0, 'p1': p1, 'r0': r0, 'r1': r1}

    def check(out, d):
        args = (seg, st, bs, bin, X.HW, X.ZTOL, X.LQ, X.PAINT)
        w0 = cr.cross_f32(d['pts'].numpy(), *args)[0]
        w1 = cr.cross_f32(d['pts'].numpy(), *args, cells=w0.copy())[0]
        dec = lr.decode_f32(recs[0][0], X.SCALE, X.OFFSET, X.ZERO)
        v0 = cr.cross_f32(dec, *args)[0]
        v1 = cr.cross_f32(dec, *args, cells=v0.copy())[0]
        assert w0[..., 0].sum() > 100 and v0[..., 0].sum() > 20
        for k, w in (('p0', w0), ('p1', w1), ('r0', v0), ('r1', v1)):
            assert np.array_equal(out[k].numpy(), w), k
    return _Built(make, call, check)


@case('residue')
def _():
    """lm_residue_keys on 3000 points of residue_ref's scene; lm_cell_components on a random 32 x 32 grid of cells; lm_residue_stats of
    one fixed labelling with the per-cell counts as the data that changes."""
    import residue_ref as rr
    import test_gpu_residue as X
    seg, scene, _, _, grid, _, _ = X._scene()
    npts, nx = 3000, 32
    cells = [rr.random_grid(n=nx, occupancy=0.4, seed=96 + k)[0] for k in range(3)]
    M = min(len(c) for c in cells)
    comp, K = rr.dense_ids(rr.roots(cells[0][:M], nx, 8))
    const = {}

    def make(k):
        rng = np.random.RandomState(11 + k)
        n = rng.randint(1, 40, M).astype(np.int64)
        return {'pts': torch.from_numpy(scene[rng.permutation(len(scene))[:npts]].copy()), 'cells': torch.from_numpy(cells[k][:M].copy()),
                'n': torch.from_numpy(n), 'iq': torch.from_numpy(n * rng.randint(0, 65536, M))}

    def call(ins, dev):
        if not const:
            const.update(index=ops.line_index(seg, rr.REACH, device=dev), comp=torch.from_numpy(comp).to(dev),
                         keys0=torch.from_numpy(cells[0][:M].copy()).to(dev))
        key, iq = ops.residue_keys(ins['pts'], const['index'], rr.ZTOL, rr.MIN_I, rr.CLEAR, grid)
        root, err = ops.cell_components(ins['cells'], nx, nx, 8)
        return {'key': key, 'iq': iq, 'root': root, 'err': err,
                'stats': ops.residue_stats(const['comp'], const['keys0'], nx, nx, ins['n'], ins['iq'], K)}

    def check(out, d):
        wk, wq = rr.keys_f32(d['pts'].numpy(), seg, rr.REACH, rr.ZTOL, rr.MIN_I, rr.CLEAR, grid)
        assert (wk >= 0).sum() > 100 and (wk < 0).sum() > 100
        assert np.array_equal(out['key'].numpy(), wk) and np.array_equal(out['iq'].numpy(), wq)
        assert int(out['err']) == 0 and np.array_equal(out['root'].numpy(), rr.roots(cells[0][:M], nx, 8))
        assert np.array_equal(out['stats'].numpy(), rr.stats(cells[0][:M], nx, comp, K, d['n'].numpy(), d['iq'].numpy()))
    return _Built(make, call, check)


# ==================================================================================================== the tests
@pytest.mark.parametrize('name', list(CASE_ENTRIES))
def test_stream_case(dev, name):
    assert set(BUILDERS) == set(CASE_ENTRIES), sorted(set(CASE_ENTRIES) ^ set(BUILDERS))
    _result(name, dev)


def test_every_stream_entry_was_seen_on_the_side_stream(dev):
    """The union of what the interposer saw in the side-stream runs (of every case: one that has not run yet in this session runs now)
    is every stream entry of the header but the exempted ones."""
    import lds_state
    seen = set()
    for name in CASE_ENTRIES:
        seen |= _result(name, dev)
    want = lds_state.stream_entries() - set(stream_state.STREAM_EXEMPT)
    assert seen == want, f'never seen on a side stream: {sorted(want - seen)}; seen but exempted or unknown: {sorted(seen - want)}'


# ---------------------------------------------------------------------------------------------------- the harness catches what it is for
def _fake(name, run, alter=None):
    def setup(dev):
        return {'x': torch.randn(4096, generator=_g(3)).to(dev), 'value': 1.0, 'dev': dev}
    return Case(name, (), setup, run, alter or (lambda state, k: None), klass='async')


def test_work_on_the_default_stream_is_caught(dev):
    """A pure-torch stand-in of an entry that zeroes its output on the DEFAULT stream and runs its "kernel" on the current one: right
    while the current stream is the default stream, and on a side stream the zeroing lands behind the blocker, after the kernel."""
    def run(state):
        stream_state.fake_entry('fake_zero_on_default')
        out = torch.empty_like(state['x'])
        with torch.cuda.stream(torch.cuda.default_stream(state['dev'])):
            out.zero_()
        out.add_(state['x'])
        return out
    with pytest.raises(AssertionError, match=r'on a side stream beside a busy default stream \[out\]: \d+ of 4096 output words differ'):
        stream_runs(_fake('fake_zero_on_default', run), dev)


def test_a_device_wide_wait_is_caught(dev):
    def run(state):
        stream_state.fake_entry('fake_device_sync')
        out = state['x'] * 2
        torch.cuda.synchronize(state['dev'])
        return out
    with pytest.raises(AssertionError, match='waited for the default stream or for the whole device'):
        stream_runs(_fake('fake_device_sync', run), dev)


def test_a_value_baked_in_from_the_host_is_caught(dev):
    """The stand-in fills its output with a Python number it reads from the state when it is CALLED: a replay keeps the number of the
    capture, the eager run on data set k has another."""
    def run(state):
        stream_state.fake_entry('fake_host_value')
        return torch.empty_like(state['x']).fill_(state['value'])

    def alter(state, k):
        state['value'] = 1.0 + k
    with pytest.raises(AssertionError, match=r'graph replay on data set 1 over outputs pre-filled with 0xFF \[out\]: 4096 of 4096'):
        stream_runs(_fake('fake_host_value', run, alter), dev)


def test_a_call_that_reaches_no_entry_is_refused(dev):
    with pytest.raises(AssertionError, match='called no stream-taking lm_'):
        stream_runs(_fake('fake_nothing', lambda state: state['x'] + 1), dev)


# ---------------------------------------------------------------------------------------------------- the 'host' entries refuse a capture
def _host_calls(dev):
    """{entry: (call, the reason its message gives)} on the small clouds of the cases above; nothing here is reached while capturing:
    the guard is each entry's first statement."""
    tiles, counts = _tiles3(), (300, 0, 200)
    pts, offs = _clouds(9, counts, tiles, 0)
    cloud = torch.from_numpy(pts).to(dev)
    ground = ops.tile_ground(cloud, offs, tiles, T, T, cell_px=16)[0]
    verts = np.asarray([(3, 3), (40, 40), (5, 9)], np.int32)
    torch.cuda.synchronize(dev)
    copy, sync = 'it copies call-local host memory to the device', 'it copies call-local host memory to the device and synchronises the stream'
    return {
        'lm_strip_bin_points': (lambda: ops.strip_bin_points(cloud, tiles, T, T, z_range=(-10.0, 10.0)), 'strip_bin', sync),
        'lm_tile_ground': (lambda: ops.tile_ground(cloud, offs, tiles, T, T, cell_px=16), 'tile_ground', copy),
        'lm_ground_select': (lambda: ops.ground_select(cloud, offs, tiles, ground, T, T, 16, (-0.05, 0.3)), 'ground_select', sync),
        'lm_tile_intensity_window': (lambda: ops.tile_intensity_window(cloud, offs, tiles, T, T), 'tile_intensity_window', copy),
        'lm_drape_vertices': (lambda: ops.drape_vertices(cloud, offs, tiles, verts, [0, 1, 2, 3], T, T, radius_px=2), 'drape_vertices', copy),
    }


@pytest.mark.parametrize('entry', ['lm_strip_bin_points', 'lm_tile_ground', 'lm_ground_select', 'lm_tile_intensity_window', 'lm_drape_vertices'])
def test_host_entry_refuses_a_capturing_stream(dev, entry):
    """Inside a capture that also records one torch op the call raises with the entry's name and the reason; the capture ends cleanly
    and the graph replays.  The same call outside the capture, before and after, is served."""
    assert stream_state.STREAM_CLASS[entry] == 'host'
    call, who, why = _host_calls(dev)[entry]
    call()                                                           # served, and the warm-up of everything the call allocates or loads
    torch.cuda.synchronize(dev)
    x = torch.arange(8, device=dev, dtype=torch.float32)
    y = torch.zeros_like(x)
    graph, cap = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    with torch.cuda.graph(graph, stream=cap):
        y.copy_(x * 2)
        with pytest.raises(LanemapHipError, match=f'{who}: must not be called on a stream that is being captured into a graph: {why}'):
            call()
    y.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert y.tolist() == [0.0, 2.0, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0], 'the capture did not survive the refused call'
    call()
    torch.cuda.synchronize(dev)
