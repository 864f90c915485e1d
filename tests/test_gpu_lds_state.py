"""GPU LDS-state tests (-m gpu): no kernel's result depends on what LDS held before its launch (tests/lds_state.py).

Two layers.  (a) guards.guarded_runs repeats every bounds / guard case after LDS pre-filled with 0xFFFFFFFF and with +Inf, so every
device entry is covered at the ragged shapes chosen there.  (b) This file names every kernel that has LDS: LDS_KERNELS maps it to the
case(s) that run it after poisoned LDS as the first kernel of an entry - a guarded case of another file where that already reaches the
kernel with padding cells, else a case below at the smallest shape that has them (B <= 2) - and LDS_EXEMPT gives the reason where no case
can.  tests/test_lds_inventory_cpu.py keeps the two tables complete.  Every case below runs under each word of lds_state.WORDS,
bit-identical to the run after zeros, and holds the run after 0xFFFFFFFF to the fp64 / exact reference and tolerance of the kernel's
present test, so three runs that agree on the same wrong answer do not pass.  Caller-supplied scratch of the older entries gets the same
treatment at the end: pre-filled with 0x00 and with 0xFF bytes, same output bits."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lds_state
from gpu_common import _chk, _close, _g, _gn_ref, _lib, _nhwc_dev, _quarter_grid, _s
from lds_state import WORDS, lds_state_runs

# (both tables are literals: tests/test_lds_inventory_cpu.py reads them without importing this file)
LDS_KERNELS = {
    'conv_mfma_kernel': ['test_gpu_lds_state.py::test_conv_mfma_instantiations', 'test_gpu_lds_state.py::test_conv_mfma_gnstats', 'test_gpu_lds_state.py::test_conv_gather_variants',
                         'test_gpu_1_bounds.py::test_conv_mfma_bounds', 'test_gpu_1_bounds.py::test_conv_mfma_res_rows_bounds', 'test_gpu_1_bounds.py::test_conv_mfma_resup_bounds',      # (its 'tiled' case)
                         'test_gpu_1_bounds.py::test_conv_gather_bounds'],
    # (the 'lateral_up' and 'lateral_up_rows' cases, and the plain residual: its three instantiations)
    'lateral_mfma_kernel': ['test_gpu_1_bounds.py::test_conv_mfma_resup_bounds',
                            'test_gpu_1_bounds.py::test_conv_mfma_lateral_plain_residual_bounds'],
    'wino44_kernel': ['test_gpu_lds_state.py::test_wino44', 'test_gpu_lds_state.py::test_wino44_gn_partial_and_split', 'test_gpu_1_bounds.py::test_winograd44_and_twin_bounds',
                      'test_gpu_1_bounds.py::test_winograd44_gn_partial_bounds'],
    'stem_mfma_kernel': ['test_gpu_lds_state.py::test_stem', 'test_gpu_1_bounds.py::test_stem_bounds'],
    'small_conv3x3_mfma_kernel': ['test_gpu_lds_state.py::test_small_conv', 'test_gpu_1_bounds.py::test_conv_small_bounds'],
    'small_conv3x3_mfma_wide_kernel': 'test_gpu_lds_state.py::test_small_conv',
    'gn_partial_kernel': ['test_gpu_lds_state.py::test_gn_stats', 'test_gpu_1_bounds.py::test_gn_stats_bounds'],
    'gn_final_kernel': ['test_gpu_lds_state.py::test_conv_mfma_gnstats', 'test_gpu_lds_state.py::test_wino44_gn_partial_and_split', 'test_gpu_1_bounds.py::test_conv_mfma_gnstats_bounds'],
    'gn_relu_up_lds_kernel': 'test_gpu_lds_state.py::test_gn_relu_up_lds',
    'gn_sum3_lds_kernel': 'test_gpu_lds_state.py::test_gn_sum3_lds',
    'gn_relu_upsample_sum_kernel': 'test_gpu_1_bounds.py::test_gn_relu_upsample_sum_bounds',
    'attention_kernel': ['test_gpu_lds_state.py::test_attention', 'test_gpu_lds_state.py::test_attention_masked', 'test_gpu_1_bounds.py::test_attention_bounds', 'test_gpu_1_bounds.py::test_attention_masked_bounds'],
    'attention_mfma_kernel': ['test_gpu_lds_state.py::test_attention', 'test_gpu_1_bounds.py::test_attention_bounds'],
    'attention_flash_kernel': 'test_gpu_lds_state.py::test_attention',
    'token_mix_kernel': 'test_gpu_1_bounds.py::test_token_mix_bounds',
    'head_tokens_lds_kernel': ['test_gpu_lds_state.py::test_head_tokens', 'test_gpu_1_bounds.py::test_head_tokens_bounds'],
    'head_stage2_lds_kernel': 'test_gpu_1_bounds.py::test_head_stage2_bounds',           # (D = 100)
    'head_conf_kernel': 'test_gpu_1_bounds.py::test_head_proposal_conf_bounds',
    'head_endpoint_kernel': 'test_gpu_endpoint_mode.py::test_head_endpoint_kernel_bounds',
    'rowref_select_kernel': 'test_gpu_lds_state.py::test_rowref_select',
    # lm_endp_topk zeroes its counters with a kernel that has no LDS first: the first pass still meets the poison
    'topk_pass_kernel': 'test_gpu_lds_state.py::test_endp_topk_plateau',
    'scan_tile_kernel': 'test_gpu_lds_state.py::test_scan_and_sort',               # n = 63: the one-tile route, where it is the only kernel
    'scan_tile_sums_kernel': 'test_gpu_lds_state.py::test_scan_and_sort',          # n = 4097: first of three
    'sort_hist_kernel': 'test_gpu_lds_state.py::test_scan_and_sort',
    'raster_partition_kernel': ['test_gpu_1_bounds.py::test_bev_raster_decoys', 'test_gpu_intensity.py::test_scaled_raster_guards'],
    'gap_kernel': ['test_gpu_gapfill.py::test_tile_gap_hist_guards', 'test_gpu_gapfill.py::test_tile_gap_fill_guards'],
    'ground_min_kernel': 'test_gpu_ground.py::test_tile_ground_guards',
    'ground_select_kernel': 'test_gpu_ground.py::test_ground_select_guards',
    'inten_count_kernel': 'test_gpu_intensity.py::test_tile_intensity_window_guards',
    'drape_min_kernel': 'test_gpu_drape.py::test_drape_vertices_guards',
    'strip_pass_kernel': 'test_gpu_strip.py::test_strip_bin_guards',
    'las_label_kernel': 'test_gpu_label.py::test_label_records_guards',
    # lm_las_line_profile_records initialises the bins with a kernel that has no LDS first: this one still meets the poison
    'las_profile_kernel': 'test_gpu_profile.py::test_profile_records_guards',
    'las_decode_kernel': 'test_gpu_lds_state.py::test_las_decode',
    'las_select_count_kernel': 'test_gpu_las_select.py::test_select_guards',
}
LDS_EXEMPT = {
    'stem_kernel': 'alternative kernel behind a test-only environment switch, compared bit for bit with the default one',
    'topk_ties_kernel': 'reached only as the second kernel of entry lm_endp_topk',
    'topk_sort_kernel': 'reached only as the second kernel of entry lm_endp_topk',
    'sort_scatter_kernel': 'reached only as the second kernel of entry lm_sort_pairs_u32',
    'ground_smooth_kernel': 'reached only as the second kernel of entry lm_tile_ground',
    'inten_locate_kernel': 'reached only as the second kernel of entry lm_tile_intensity_window',
    'strip_offsets_kernel': 'reached only as the second kernel of entry lm_strip_bin_points',
    'drape_median_kernel': 'reached only as the second kernel of entry lm_drape_vertices',
    'raster_band_kernel': 'reached only as the second kernel of entry lm_bev_raster_batch',
    'las_select_emit_kernel': 'reached only as the second kernel of entry lm_las_decode_select',
}


# ==================================================================================================== the harness itself
class _FakeLib:
    """Records the calls made on it; any attribute is an entry."""

    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        def entry(*args):
            self._log.append((name, args[0] if args else None))
            return 0
        return entry


@pytest.fixture(scope='module')
def lds_outlives_dispatch(dev):
    """The precondition of every other test here: what fill() stores is what the next dispatch finds.  Where it does not hold, the tests
    that depend on it are errors, not vacuous passes."""
    n, wg = {}, lds_state.workgroups()
    for word in WORDS:
        lds_state.fill(word)
        other = WORDS[(WORDS.index(word) + 1) % len(WORDS)]
        n[word] = (lds_state.probe(word), lds_state.probe(other))
    print(f'LDS probe, {wg} workgroups x {lds_state.LDS_WORDS} words: ' +
          ', '.join(f'0x{w:08X}: {a} mismatches, {b} against another word' for w, (a, b) in n.items()))
    bad = {f'0x{w:08X}': v for w, v in n.items() if v != (0, wg * lds_state.LDS_WORDS)}
    assert not bad, (f'LDS contents do not outlive a dispatch on this device, or the fill does not reach every CU: (mismatches with the '
                     f'filled word, with another word) = {bad}, expected (0, {wg * lds_state.LDS_WORDS}); the LDS-state tests of this file '
                     f'and of guards.guarded_runs prove nothing here')
    return n


def test_lds_contents_outlive_a_dispatch(lds_outlives_dispatch):
    assert set(lds_outlives_dispatch) == set(WORDS)


def test_the_planted_leak_is_caught(dev, lds_outlives_dispatch):
    """lmd_lds_leaky adds 0 * (an LDS cell it never wrote): exact after zeros, and lds_state_runs must say so after NaN and after +Inf."""
    x = torch.randn(1000, generator=_g(1)).to(dev)
    with lds_state.poisoned(WORDS[0]):
        assert torch.equal(lds_state.leaky(x), x)
    for word in WORDS[1:]:
        with lds_state.poisoned(word):
            y = lds_state.leaky(x)
        assert bool(torch.isnan(y).all()), f'the planted leak is finite after LDS = 0x{word:08X}'

    with pytest.raises(AssertionError) as e:
        lds_state_runs(lambda: lds_state.leaky(x), 'planted leak')
    for word in WORDS[1:]:
        assert f'planted leak after LDS = 0x{word:08X} [out]: 1000 of 1000 output words differ' in str(e.value), str(e.value)


def test_poisoned_wraps_every_stream_entry(monkeypatch):
    """With a fake library and a fake fill (no GPU needed): inside poisoned() a call of any stream-taking entry - through
    gpu_common._lib(), lanemapping_amd._lib.lib() (which ops and torch_ops call) or a handle taken BEFORE the context - is preceded by
    exactly one fill on the same stream and counted; entries without a stream get none; a context that enqueued no fill fails; the
    library object is restored on exit."""
    from lanemapping_amd import _lib as L
    from test_bounds_inventory_cpu import _stream_entries
    log = []
    fake = _FakeLib(log)

    class Diag:
        @staticmethod
        def lmd_lds_fill(stream, word, workgroups):
            log.append(('fill', stream, word))
            return 0
    monkeypatch.setattr(L, '_lib', fake)
    monkeypatch.setattr(lds_state, '_DIAG', Diag)
    names = _stream_entries()
    assert set(names) <= lds_state.stream_entries() and 'lm_head_endpoint' in lds_state.stream_entries()
    early = L.lib()                                    # as `L = lib()` at the top of a test
    bound = early.lm_gn_stats                          # an entry bound outside: the one thing that escapes
    with lds_state.poisoned(0x7F800000) as p:
        for k, name in enumerate(names):
            del log[:]
            getattr((_lib(), L.lib(), early)[k % 3], name)(1000 + k, 1, 2)
            assert log == [('fill', 1000 + k, 0x7F800000), (name, 1000 + k)], (name, log)
        assert p.fills == len(names)
        for name in ('lm_winograd44_supported', 'lm_endp_cluster', 'lm_last_error', 'lm_gn_stats_workspace_bytes'):
            del log[:]
            getattr(_lib(), name)(7)
            assert log == [(name, 7)], (name, log)
        with lds_state.poisoned(0xFFFFFFFF) as q:     # nested: one fill, the inner word
            del log[:]
            early.lm_gn_stats(5)
            assert log == [('fill', 5, 0xFFFFFFFF), ('lm_gn_stats', 5)] and q.fills == 1
        assert p.fills == len(names) + 1
    assert L._lib is fake and not [k for k in vars(fake) if k.startswith('lm_')]
    del log[:]
    _lib().lm_gn_stats(5)
    assert log == [('lm_gn_stats', 5)]
    with pytest.raises(AssertionError, match='no stream-taking lm_'):
        with lds_state.poisoned(0xFFFFFFFF):
            bound(5)                                   # goes round the context: not a poisoned run, and said so
    with pytest.raises(AssertionError, match='no stream-taking lm_'):
        with lds_state.poisoned(0xFFFFFFFF):
            _lib().lm_gn_stats_workspace_bytes(1, 2, 3)
    assert lds_state._ACTIVE is None and not [k for k in vars(fake) if k.startswith('lm_')]


def test_poisoned_fills_before_each_entry_on_the_device(dev, lds_outlives_dispatch):
    """The same on the device: after an ops call under poisoned(word) made of kernels without LDS, every CU's LDS holds the word."""
    from lanemapping_amd import ops
    x = _nhwc_dev(torch.randn(1, 8, 5, 7, generator=_g(2)), dev)
    lds_state.fill(WORDS[0])
    with lds_state.poisoned(WORDS[1]):
        ops.upsample_nhwc(x, (9, 13))
    assert lds_state.probe(WORDS[1]) == 0


# ==================================================================================================== helpers
def _act(t, dev, ld=None):
    """logical [B,C,H,W] CPU tensor -> NHWC-stored device tensor, optionally a channel slice (column 0) of rows ld wide."""
    B, Cc, H, W = t.shape
    if ld is None:
        return _nhwc_dev(t, dev)
    buf = torch.zeros(B, H, W, ld, device=dev)
    buf[..., :Cc] = t.to(dev).permute(0, 2, 3, 1)
    return buf[..., :Cc].permute(0, 3, 1, 2)


def _out(B, Cc, H, W, dev, ld):
    return torch.zeros(B, H, W, ld, device=dev)[..., :Cc].permute(0, 3, 1, 2)


def _affine(y, sc, sh):
    if sc is not None:
        y = y * sc.double().view(1, -1, 1, 1)
    return y + sh.double().view(1, -1, 1, 1)


def _stats_close(st, y_ref, name):
    """st [B, C, 2] (mean, rstd) against fp64, as the bounds tests hold them: mean within 1e-5 of max(1, |mean|), rstd 1e-5 relative."""
    mean, rstd = _gn_ref(y_ref)
    st = st.double().cpu()
    assert float(((st[..., 0] - mean).abs() / mean.abs().clamp_min(1.0)).max()) <= 1e-5, name + ' mean'
    assert float(((st[..., 1] - rstd).abs() / rstd).max()) <= 1e-5, name + ' rstd'


# ==================================================================================================== conv_mfma
@pytest.mark.parametrize('name,H,W,cin,cout,k,stride,extra', [
    ('t128x64', 13, 11, 32, 40, 3, 1, 'res'),              # Cout <= 64: launch<128,64,32,64>
    ('t128x128_smallk', 9, 7, 64, 136, 1, 1, 'res'),       # K = 64 <= 256: launch<128,128,32,64>
    ('t64', 17, 19, 96, 200, 3, 2, 'res'),                 # K = 864, few blocks: launch<64,64,32,32>
    ('t64_odd_ldy', 13, 11, 32, 96, 3, 1, 'odd_ldy'),      # ldy = 97: the scalar epilogue
    ('resup', 13, 11, 32, 96, 3, 1, 'res_up'),             # the coarse-residual epilogue
    ('res_rows', 1, 130, 64, 72, 1, 1, 'res_rows'),        # positional-embedding residual, 26 table rows
])
def test_conv_mfma_instantiations(dev, lds_outlives_dispatch, name, H, W, cin, cout, k, stride, extra):
    from lanemapping_amd import ops
    B = 2
    g = _g(H * W + cout)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    ref = _affine(F.conv2d(x.double(), w.double(), None, stride, k // 2), sc, sh)
    Ho, Wo = ref.shape[2:]
    kw = {}
    if extra == 'res_up':
        rc = torch.randn(B, cout, 5, 6, generator=g)
        ref = ref + F.interpolate(rc.double(), size=(Ho, Wo), mode='bilinear', align_corners=True)
        kw['res_up'] = _act(rc, dev, cout + 8)
    elif extra == 'res_rows':
        emb = torch.randn(26, cout, generator=g)
        ref = ref + emb.double().t().repeat(1, W // 26).view(1, cout, 1, W)
        kw.update(res=emb.to(dev), res_rows=26)
    else:
        r = torch.randn(B, cout, Ho, Wo, generator=g)
        ref = ref + r.double()
        kw['res'] = _act(r, dev, cout + 4)
    xd, wp, scd, shd = _act(x, dev, cin + 8), ops.pack_mfma(w.to(dev)), sc.to(dev), sh.to(dev)
    ldy = cout + 1 if extra == 'odd_ldy' else cout + 4

    def run():
        return ops.conv_mfma(xd, wp, cout, k, k, stride, k // 2, 1, scd, shd, out=_out(B, cout, Ho, Wo, dev, ldy), **kw)
    y = lds_state_runs(run, f'conv_mfma {name}')
    _close(y, ref, 1e-5, name)


def test_conv_mfma_gnstats(dev, lds_outlives_dispatch):
    """lm_conv2d_nhwc_mfma_f32_gnstats, 64 -> 128 3x3 on 24 x 32 (launch<128,128,64,64> with the statistics epilogue), and lm_gn_finalize
    (gn_final_kernel as the only kernel of its entry)."""
    from lanemapping_amd import ops
    B, H, W, cin, cout = 2, 24, 32, 64, 128
    g = _g(2432)
    x = torch.randn(B, cin, H, W, generator=g) + 3.0
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sh = torch.randn(cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), sh.double(), 1, 1)
    xd, wp, shd = _act(x, dev), ops.pack_mfma(w.to(dev)), sh.to(dev)
    y, st = lds_state_runs(lambda: ops.conv_mfma_gnstats(xd, wp, cout, 3, 3, 1, 1, 1, shd), 'conv_mfma gnstats').values()
    _close(y, ref, 1e-5, 'gnstats y')
    _stats_close(st, ref, 'gnstats')


@pytest.mark.parametrize('cin,cout,taps', [(16, 16, 27), (32, 32, 9), (32, 64, 9), (32, 72, 9)])
def test_conv_gather_variants(dev, lds_outlives_dispatch, cin, cout, taps):
    """lm_conv_gather_mfma_f32: Cin 16 with 27 taps (the last tap pair has an odd half that only zero weights meet), Cin 32 with
    Cout <= 32, <= 64 and > 64 (its three tile widths).  M = 333: a ragged M tile; a third of the rulebook inactive."""
    from lanemapping_amd import ops
    V, M = 200, 333
    g = _g(cin + cout + taps)
    x = torch.randn(V, cin, generator=g)
    nbr = torch.randint(0, V, (M, taps), generator=g, dtype=torch.int32)
    nbr[torch.rand(M, taps, generator=g) < 0.35] = -1
    kd = (3, 3, 3) if taps == 27 else (1, 3, 3)
    w = torch.randn(*kd, cin, cout, generator=g) / (taps * cin) ** 0.5
    sh = torch.randn(cout, generator=g)
    xe = torch.cat([x.double(), torch.zeros(1, cin, dtype=torch.float64)])
    ref = torch.einsum('mtc,tco->mo', xe[torch.where(nbr < 0, V, nbr).long()], w.double().reshape(taps, cin, cout)) + sh.double()
    xd, nd, wp, shd = x.to(dev), nbr.to(dev), ops.pack_sparse(w.to(dev)), sh.to(dev)
    y = lds_state_runs(lambda: ops.conv_gather(xd, nd, wp, cin, cout, shift=shd), f'conv_gather {cin}->{cout}')
    _close(y[:, :cout], ref, 1e-5, 'conv_gather')


# ==================================================================================================== Winograd F(4x4, 3x3)
@pytest.mark.parametrize('H,W,cin,cout,dil', [(5, 41, 16, 70, 1),       # the narrowest tile row; Cin 16: the K tail only; ragged N tile
                                              (5, 41, 48, 70, 1),       # Cin 48: one channel pair and the tail
                                              (13, 86, 48, 70, 2)])
def test_wino44(dev, lds_outlives_dispatch, H, W, cin, cout, dil):
    """lm_conv3x3_winograd44_f32 with scale, residual and ReLU, against fp64 at the Winograd tolerance (1e-4) and bit-identical to the
    materialising twin under every word (the twin's own kernels are poisoned too)."""
    from lanemapping_amd import ops
    B = 2
    assert ops.wino44_supported(H, W, cin, dil)
    g = _g(H * W + cin + dil)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    r = torch.randn(B, cout, H, W, generator=g)
    ref = F.relu(_affine(F.conv2d(x.double(), w.double(), None, 1, dil, dil), sc, sh) + r.double())
    wu = ops.pack_wino44(w.to(dev))
    wf = ops.pack_wino44_fragments(wu)
    xd, rd, scd, shd = _act(x, dev, cin + 8), _act(r, dev), sc.to(dev), sh.to(dev)

    def run():
        return {'y': ops.conv_wino44(xd, wf, cout, dil, scd, shd, rd, ops.ACT_RELU),
                'twin': ops.conv_wino44_twin(xd, wu, cout, dil, scd, shd, rd, ops.ACT_RELU)}
    out = lds_state_runs(run, f'wino44 {H}x{W} {cin}->{cout} d{dil}')
    _close(out['y'], ref, 1e-4, 'wino44')
    assert torch.equal(out['y'], out['twin']), 'fused and twin Winograd differ after LDS = 0xFFFFFFFF'


def test_wino44_gn_partial_and_split(dev, lds_outlives_dispatch):
    """Cin 16 -> Cout 64 on 13 x 45: the gn_partial epilogue (+ lm_gn_finalize) of the fp32 line, and the split-precision second line
    with its twin."""
    from lanemapping_amd import ops
    B, H, W, cin, cout = 2, 13, 45, 16, 64
    g = _g(1345)
    x = torch.randn(B, cin, H, W, generator=g) + 1.0
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sh = torch.randn(cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), sh.double(), 1, 1)
    wu = ops.pack_wino44(w.to(dev))
    wf, ws = ops.pack_wino44_fragments(wu), ops.pack_wino44_fragments_split(wu)
    xd, shd = _act(x, dev), sh.to(dev)

    def run():
        y, st = ops.conv_wino44(xd, wf, cout, 1, None, shd, gn_eps=1e-5)
        return {'y': y, 'stats': st, 'split': ops.conv_wino44(xd, ws, cout, 1, None, shd),
                'split_twin': ops.conv_wino44_twin(xd, wu, cout, 1, None, shd, split=True)}
    out = lds_state_runs(run, 'wino44 gn_partial / split')
    _close(out['y'], ref, 1e-4, 'wino44 gn y')
    _stats_close(out['stats'], ref, 'wino44 gn')
    _close(out['split'], ref, 1e-4, 'wino44 split')
    assert torch.equal(out['split'], out['split_twin']), 'split line and its twin differ after LDS = 0xFFFFFFFF'


# ==================================================================================================== stem, thin layers
@pytest.mark.parametrize('u8', [False, True])
def test_stem(dev, lds_outlives_dispatch, u8):
    """stem_mfma_kernel<f32> / <u8> on 37 x 43, B = 2: ragged 16 x 16 output tiles, and the k = 21 pad of each 7-tap row group that only
    a zero weight meets."""
    from lanemapping_amd import ops
    B, H, W = 2, 37, 43
    g = _g(3743 + u8)
    if u8:
        xin = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
        x64 = xin.permute(0, 3, 1, 2).double() / 255.0
    else:
        xin = torch.rand(B, 3, H, W, generator=g)
        x64 = xin.double()
    w = torch.randn(64, 3, 7, 7, generator=g) / 12
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    ref = F.relu(_affine(F.conv2d(x64, w.double(), None, 2, 3), sc, sh))
    xd, wk, scd, shd = xin.to(dev), w.permute(2, 3, 1, 0).contiguous().to(dev), sc.to(dev), sh.to(dev)
    y = lds_state_runs(lambda: ops.stem(xd, wk, scd, shd), f'stem u8={u8}')
    _close(y, ref, 1e-5, 'stem')


@pytest.mark.parametrize('cin,cout,stride,pre_relu', [(16, 5, 1, False), (16, 16, 2, True),      # small_conv3x3_mfma_kernel<1> / <2>
                                                      (32, 48, 1, True), (32, 48, 2, False)])   # small_conv3x3_mfma_wide_kernel
def test_small_conv(dev, lds_outlives_dispatch, cin, cout, stride, pre_relu):
    """lm_conv2d_nhwc_small on 19 x 23 (ragged tiles, patch border cells), B = 2."""
    from lanemapping_amd import ops
    B, H, W = 2, 19, 23
    g = _g(cin + cout + stride)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    xin = F.relu(x.double()) if pre_relu else x.double()
    ref = _affine(F.conv2d(xin, w.double(), None, stride, 1), sc, sh)
    xd, w16, scd, shd = _act(x, dev, cin + 4), ops.pack_small(w.to(dev)), sc.to(dev), sh.to(dev)
    y = lds_state_runs(lambda: ops.conv_small(xd, w16, cout, 3, 3, stride, 1, scd, shd, pre_relu), f'conv_small {cin}->{cout} s{stride}')
    _close(y, ref, 1e-5, 'conv_small')


# ==================================================================================================== GroupNorm
@pytest.mark.parametrize('Cc', [32, 256])
@pytest.mark.parametrize('H,W', [(1, 3), (19, 27)])        # HW = 3: less than one chunk; 513 = 8 chunks of 64 and one pixel
def test_gn_stats(dev, lds_outlives_dispatch, H, W, Cc):
    from lanemapping_amd import ops
    x = torch.randn(2, Cc, H, W, generator=_g(H * W + Cc)) * 2 + 5
    xd = _act(x, dev)
    st = lds_state_runs(lambda: ops.gn_stats(xd), f'gn_stats HW={H * W} C={Cc}')
    _stats_close(st, x, 'gn_stats')


def _gn_relu64(x, gamma, beta):
    m, r = _gn_ref(x)
    st = torch.stack([m, r], 2).float()
    y = F.relu((x.double() - st[..., 0].double()[:, :, None, None]) * st[..., 1].double()[:, :, None, None] * gamma.double().view(1, -1, 1, 1)
               + beta.double().view(1, -1, 1, 1))
    return y, st


def _up(x, Ho, Wo):
    return F.interpolate(x, size=(Ho, Wo), mode='bilinear', align_corners=True)


def test_gn_relu_up_lds(dev, lds_outlives_dispatch):
    """gn_relu_up_lds_kernel: one term, 128 channels, 37 x 21 -> 75 x 50 (ragged output tiles, source blocks clipped at the border)."""
    from lanemapping_amd import ops
    B, Cc, Hi, Wi, Ho, Wo = 2, 128, 37, 21, 75, 50
    g = _g(3721)
    x = torch.randn(B, Cc, Hi, Wi, generator=g) * 2 + 1
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1
    t, st = _gn_relu64(x, gamma, beta)
    xd, sd, gd, bd = _act(x, dev), st.to(dev), gamma.to(dev), beta.to(dev)
    y = lds_state_runs(lambda: ops.gn_relu_upsample_sum([(xd, sd)], gd, bd, (Ho, Wo)), 'gn_relu_up_lds')
    _close(y, _up(t, Ho, Wo), 1e-5, 'gn_relu_up_lds')


def test_gn_sum3_lds(dev, lds_outlives_dispatch):
    """gn_sum3_lds_kernel: s2 + up(s3) + s4 at C = 32 with the 1x1 projection (5 outputs), 37 x 45 output, the middle term 19 x 23."""
    from lanemapping_amd import ops
    B, Cc, Ho, Wo, cout = 2, 32, 37, 45, 5
    g = _g(3745)
    xs = [torch.randn(B, Cc, h, w, generator=g) * 2 + 1 for h, w in ((Ho, Wo), (19, 23), (Ho, Wo))]
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1
    w1, b1 = torch.randn(cout, Cc, 1, 1, generator=g) / Cc ** 0.5, torch.randn(cout, generator=g)
    ref, terms = None, []
    for x in xs:
        t, st = _gn_relu64(x, gamma, beta)
        t = _up(t, Ho, Wo)
        ref = t if ref is None else ref + t
        terms.append((_act(x, dev, 2 * Cc), st.to(dev)))
    ref1 = torch.einsum('oc,bchw->bohw', w1[:, :, 0, 0].double(), ref) + b1.double().view(1, -1, 1, 1)
    gd, bd, w16, b1d = gamma.to(dev), beta.to(dev), ops.pack_small(w1.to(dev)), b1.to(dev)
    out = lds_state_runs(lambda: ops.gn_relu_upsample_sum(terms, gd, bd, (Ho, Wo), proj=(w16, b1d, cout)), 'gn_sum3_lds')
    _close(out['out0'], ref, 1e-5, 'gn sum3')
    _close(out['out1'], ref1, 1e-5, 'gn sum3 conv1x1')


# ==================================================================================================== attention
def _attn_ref(qkv, B, N, heads, valid=None):
    q, k, v = [z.reshape(B, N, heads, 64).transpose(1, 2).double() for z in qkv.chunk(3, dim=-1)]
    s = q @ k.transpose(-1, -2) * 0.125
    if valid is not None:
        s = s.masked_fill(~valid.bool().view(B, 1, 1, N), float('-inf'))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * N, heads * 64)


@pytest.mark.parametrize('N', [37, 321, 382])      # attention_kernel; attention_mfma_kernel with 31 padded keys; attention_flash_kernel
def test_attention(dev, lds_outlives_dispatch, N):
    from lanemapping_amd import ops
    B, heads = 2, 2
    qkv = torch.randn(B * N, 3 * heads * 64, generator=_g(N)) * 1.5
    qd = qkv.to(dev)
    y = lds_state_runs(lambda: ops.attention(qd, B, N, heads, 64, 0.125), f'attention N={N}')
    _close(y, _attn_ref(qkv, B, N, heads), 1e-5, f'attention N={N}')


def test_attention_masked(dev, lds_outlives_dispatch):
    """attention_kernel with a key mask: N = 7, alternating flags (the compacted keys leave LDS rows behind them unwritten)."""
    from lanemapping_amd import ops
    B, N, heads = 2, 7, 2
    qkv = torch.randn(B * N, 3 * heads * 64, generator=_g(7))
    valid = torch.tensor([[1, 0, 1, 0, 1, 0, 1], [0, 1, 0, 1, 0, 1, 0]], dtype=torch.int32)
    qd, vd = qkv.to(dev), valid.to(dev)
    y = lds_state_runs(lambda: ops.attention(qd, B, N, heads, 64, 0.125, vd), 'attention masked')
    _close(y, _attn_ref(qkv, B, N, heads, valid), 1e-5, 'attention masked')


# ==================================================================================================== heads
def _tokens_ref(row, seg, P, pw, hb, seg_bias):
    """The seg-weighted proposal tokens of one image in fp64, as tests/test_gpu_head_geometry.py restates them."""
    Cc, Hr, Wr = row.shape
    fw = pw + 2 * hb
    rowp = F.pad(row.double(), (hb, hb + pw * P, 0, 0))
    segp = F.pad(seg.double(), (2 * hb, 2 * hb + 2 * pw * P, 0, 0), value=seg_bias)
    toks = []
    for p in range(P):
        win = rowp[:, :, pw * p: pw * p + fw]
        up = F.interpolate(segp[None, None, :, 2 * pw * p: 2 * pw * p + 2 * fw], size=(8 * Hr, 8 * fw), mode='bilinear', align_corners=True)
        toks.append((win * F.avg_pool2d(up, 8)[0]).permute(1, 0, 2).reshape(Hr, Cc * fw))
    return torch.cat(toks)


@pytest.mark.parametrize('fw,pw,P', [(10, 2, 12), (12, 4, 6), (16, 8, 3)])
def test_head_tokens(dev, lds_outlives_dispatch, fw, pw, P):
    """head_tokens_lds_kernel<10 / 12 / 16> at Hr = Wr = 25: a ragged last block of token rows, windows that leave the map."""
    from lanemapping_amd import ops
    B, Hr = 2, 25
    g = _g(fw)
    row = torch.randn(B, 16, Hr, Hr, generator=g)
    seg = torch.randn(B, 1, 2 * Hr, 2 * Hr, generator=g)
    rd, sd = _nhwc_dev(row, dev), seg.to(dev)
    tok = lds_state_runs(lambda: ops.head_tokens(sd, rd, P, pw, 4, -0.37), f'head_tokens FW={fw}')
    for b in range(B):
        _close(tok[b * P * Hr:(b + 1) * P * Hr], _tokens_ref(row[b], seg[b, 0], P, pw, 4, -0.37), 1e-5, f'tokens FW={fw} b={b}')


def test_rowref_select(dev, lds_outlives_dispatch):
    """rowref_select_kernel: H = 300 (the 256-thread row loop runs twice, ragged), W = 37, L = 3; means against fp64, flags and arg-max
    columns exact."""
    from lanemapping_amd import ops
    B, H, W, L = 1, 300, 37, 3
    g = _g(H + W)
    ext = torch.rand(B, H, L, 2, generator=g) * 0.2
    ext[..., 0] += torch.tensor([0.35, 0.05, 0.35]).view(1, 1, L)
    cls = _quarter_grid(torch.rand(B, H, L, W, generator=g) * 2)
    cls[:, 0] = 0.5
    ed, cd = ext.to(dev), cls.to(dev)

    def run():
        mean = torch.empty((B, L), device=dev)
        valid = torch.empty((B, L), device=dev, dtype=torch.int32)
        corr = torch.empty((B, L, H), device=dev, dtype=torch.int32)
        _chk(_lib().lm_rowref_select(_s(), ed.data_ptr(), cd.data_ptr(), mean.data_ptr(), valid.data_ptr(), C.c_float(0.3), corr.data_ptr(),
                                     B, H, W, L))
        return {'mean': mean, 'valid': valid, 'corr': corr}
    out = lds_state_runs(run, 'rowref_select')
    mref = ext[..., 0].double().mean(1)
    _close(out['mean'], mref, 1e-5, 'lane mean')
    assert torch.equal(out['valid'], (mref > 0.3).int())
    assert torch.equal(out['corr'], torch.from_numpy(np.argmax(cls.numpy(), axis=3).astype(np.int32)).permute(0, 2, 1))


# ==================================================================================================== decision and index kernels
def test_endp_topk_plateau(dev, lds_outlives_dispatch):
    """lm_endp_topk on the tied-score plateau of test_endp_topk_tied_scores (17,000 pixels on one score above everything else): exactly
    the K best under (score descending, index ascending)."""
    from lanemapping_amd import ops
    H = W = 256
    clip, K = 20, 512
    x = torch.randn((2, 1, H, W), generator=_g(5)) - 4.0
    x[:, 0, 50:150, 30:200] = 2.5
    xd = x.to(dev)
    out = lds_state_runs(lambda: dict(zip(('idx', 'score', 'status'), ops.endp_topk(xd, K=K, clip=clip))), 'endp_topk plateau')
    assert int(out['status'].max()) == 0
    for b in range(2):
        s = torch.sigmoid(xd[b, 0, clip:H - clip, clip:W - clip]).cpu().numpy().reshape(-1)
        want = np.lexsort((np.arange(s.size), -s.astype(np.float64)))[:K]
        assert np.array_equal(out['idx'][b].numpy(), want), f'tile {b}'


def test_scan_and_sort(dev, lds_outlives_dispatch):
    """lm_exclusive_scan_u32 at n = 63 (one tile) and 4097 (a second tile of one element), lm_sort_pairs_u32 at n = 4097: against numpy's
    cumsum and stable argsort."""
    from lanemapping_amd import ops
    for n in (63, 4097):
        x = np.random.default_rng(n).integers(0, 2 ** 31, size=n, dtype=np.int64).astype(np.uint32)
        want = np.zeros(n, dtype=np.uint32)
        want[1:] = np.cumsum(x[:-1].astype(np.uint64)).astype(np.uint32)
        xd = torch.from_numpy(x.view(np.int32)).to(dev)
        got = lds_state_runs(lambda: ops.exclusive_scan_u32(xd), f'exclusive_scan n={n}')
        np.testing.assert_array_equal(got.numpy().view(np.uint32), want)
    n = 4097
    k = np.random.default_rng(7).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    k[::5] = k[0]                                                    # duplicates: stability shows
    v = np.arange(n, dtype=np.uint32)
    order = np.argsort(k, kind='stable')
    kd, vd = torch.from_numpy(k.view(np.int32)).to(dev), torch.from_numpy(v.view(np.int32)).to(dev)
    out = lds_state_runs(lambda: dict(zip(('keys', 'vals'), ops.sort_pairs_u32_(kd.clone(), vd.clone()))), 'sort_pairs n=4097')
    np.testing.assert_array_equal(out['vals'].numpy().view(np.uint32), v[order])
    np.testing.assert_array_equal(out['keys'].numpy().view(np.uint32), k[order])


@pytest.mark.parametrize('fmt', [1, 6])
def test_las_decode(dev, lds_outlives_dispatch, tmp_path, fmt):
    """las_decode_kernel (lm_las_decode_points) on 1001 records with extra bytes (record lengths 29 / 31: records straddle the staged
    words): bit-exact against the numpy reader."""
    from lanemapping_amd import las_io
    from oracle import las_ref
    n = 1001
    rng = np.random.RandomState(fmt)
    xyz = rng.rand(n, 3) * [57.6, 57.6, 3] + [351200.0, 3433000.0, 10.0]
    path = str(tmp_path / 't.las')
    las_ref.write_las(path, xyz, rng.randint(0, 65535, n), point_format=fmt, version=(1, 4) if fmt >= 6 else (1, 2),
                      offset=(351000.0, 3433000.0, 0.0), extra_bytes=1)
    shift = [351200.0, 3433000.0, 10.0]
    got = lds_state_runs(lambda: las_io.read_las(path, dev, shift=shift), f'las_decode fmt {fmt}')
    assert np.array_equal(got.numpy(), las_ref.read_las_ref(path, shift=shift).astype(np.float32))


# ==================================================================================================== caller-supplied scratch
def _scratch_runs(run, name):
    """run(byte) -> outputs of one call whose caller-supplied workspace is pre-filled with `byte`: 0x00 and 0xFF give the same bits."""
    a = run(0x00)
    torch.cuda.synchronize()
    a = {k: v.clone() for k, v in lds_state._named(a).items()}
    b = run(0xFF)
    torch.cuda.synchronize()
    try:
        lds_state.assert_same_bits(b, a, name)
    except AssertionError as e:
        raise AssertionError(str(e).replace('the run after zeroed LDS', 'the run on a zeroed workspace')
                             .replace('an LDS cell this launch never wrote', 'a workspace word this call never wrote')) from None
    return a


def _ws(nbytes, byte, dev):
    return torch.full((max(int(nbytes), 8),), byte, dtype=torch.uint8, device=dev)


def test_scratch_scan_sort_topk(dev):
    L = _lib()
    n = 4097
    x = torch.from_numpy(np.random.default_rng(1).integers(0, 2 ** 31, size=n, dtype=np.int64).astype(np.uint32).view(np.int32)).to(dev)

    def scan(byte):
        ws, out = _ws(L.lm_scan_workspace_bytes(n), byte, dev), torch.empty_like(x)
        _chk(L.lm_exclusive_scan_u32(_s(), x.data_ptr(), out.data_ptr(), n, ws.data_ptr(), ws.numel()))
        return out
    _scratch_runs(scan, 'exclusive_scan workspace')

    def sort(byte):
        ws, k, v = _ws(L.lm_sort_pairs_workspace_bytes(n), byte, dev), x.clone(), torch.arange(n, dtype=torch.int32, device=dev)
        _chk(L.lm_sort_pairs_u32(_s(), k.data_ptr(), v.data_ptr(), n, 32, ws.data_ptr(), ws.numel()))
        return {'keys': k, 'vals': v}
    _scratch_runs(sort, 'sort_pairs workspace')
    e = torch.randn((2, 1, 256, 256), generator=_g(5)) - 4.0
    e[:, 0, 50:150, 30:200] = 2.5
    ed = e.to(dev)

    def topk(byte):
        ws = _ws(L.lm_endp_topk_workspace_bytes(2), byte, dev)
        idx, score = torch.empty((2, 512), device=dev, dtype=torch.int32), torch.empty((2, 512), device=dev)
        status = torch.empty((2,), device=dev, dtype=torch.int32)
        _chk(L.lm_endp_topk(_s(), ed.data_ptr(), ws.data_ptr(), idx.data_ptr(), score.data_ptr(), status.data_ptr(), 2, 256, 256, 20, 512))
        return {'idx': idx, 'score': score, 'status': status}
    _scratch_runs(topk, 'endp_topk workspace')


def test_scratch_gn_stats_and_partials(dev):
    from lanemapping_amd import ops
    L = _lib()
    B, Cc, H, W = 2, 64, 15, 13
    x = _act(torch.randn(B, Cc, H, W, generator=_g(64)) * 2 + 5, dev)

    def gn(byte):
        ws, st = _ws(L.lm_gn_stats_workspace_bytes(B, H * W, Cc), byte, dev), torch.empty((B, Cc, 2), device=dev)
        _chk(L.lm_gn_stats(_s(), x.data_ptr(), ws.data_ptr(), st.data_ptr(), B, H * W, Cc, C.c_float(1e-5)))
        return st
    _scratch_runs(gn, 'gn_stats workspace')
    # the gn_partial buffers of the two convolutions: every word the finalize reads is written by the convolution
    cin, cout, H, W = 32, 96, 16, 24                            # (the statistics epilogue needs Cout > 64 and Ho * Wo % 128 == 0)
    g = _g(9)
    xc = _act(torch.randn(B, cin, H, W, generator=g), dev)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    wp, wf, sh = ops.pack_mfma(w.to(dev)), ops.pack_wino44_fragments(ops.pack_wino44(w.to(dev))), torch.randn(cout, generator=g).to(dev)

    def mfma(byte):
        nch = H * W // 64
        y, part, st = ops.new_act(B, cout, H, W, dev), _ws(B * nch * cout * 16, byte, dev), torch.empty((B, cout, 2), device=dev)
        _chk(L.lm_conv2d_nhwc_mfma_f32_gnstats(_s(), xc.data_ptr(), cin, wp.data_ptr(), wp.shape[1], sh.data_ptr(), y.data_ptr(), cout,
                                               part.data_ptr(), B, H, W, cin, cout, 3, 3, 1, 1, 1, 1))
        _chk(L.lm_gn_finalize(_s(), part.data_ptr(), st.data_ptr(), B, H * W, cout, nch, C.c_float(1e-5)))
        return {'y': y, 'stats': st}
    _scratch_runs(mfma, 'conv_mfma gn_partial buffer')
    H, W = 13, 45

    xw = _act(torch.randn(B, cin, H, W, generator=g), dev)

    def wino(byte):
        nch = L.lm_winograd44_gn_chunks(H, W, 1)
        y, part, st = ops.new_act(B, cout, H, W, dev), _ws(B * nch * cout * 16, byte, dev), torch.empty((B, cout, 2), device=dev)
        _chk(L.lm_conv3x3_winograd44_f32(_s(), xw.data_ptr(), cin, wf.data_ptr(), wf.shape[2] * 32, None, sh.data_ptr(), None, 0, y.data_ptr(),
                                         cout, B, H, W, cin, cout, 1, ops.ACT_NONE, part.data_ptr()))
        _chk(L.lm_gn_finalize(_s(), part.data_ptr(), st.data_ptr(), B, H * W, cout, nch, C.c_float(1e-5)))
        return {'y': y, 'stats': st}
    _scratch_runs(wino, 'wino44 gn_partial buffer')


@pytest.mark.parametrize('split', [False, True])
def test_scratch_wino44_twin(dev, split):
    from lanemapping_amd import ops
    L = _lib()
    B, H, W, cin, cout = 2, 13, 45, 32, 40
    g = _g(45 + split)
    x = _act(torch.randn(B, cin, H, W, generator=g), dev)
    wu = ops.pack_wino44((torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).to(dev))
    sc = ops.split_scale(wu)
    wt = (wu * sc).contiguous() if split else wu
    need = L.lm_winograd44_twin_workspace_bytes(B, H, W, cin, wu.shape[1], 1)

    def run(byte):
        ws, y = _ws(need, byte, dev), ops.new_act(B, cout, H, W, dev)
        a = (_s(), x.data_ptr(), cin, wt.data_ptr(), wu.shape[1], None, None, None, 0, y.data_ptr(), cout, B, H, W, cin, cout, 1, ops.ACT_NONE,
             ws.data_ptr(), need)
        _chk(L.lm_conv3x3_winograd44_split_twin_f32(*a, C.c_float(1.0 / sc)) if split else L.lm_conv3x3_winograd44_twin_f32(*a))
        return y
    _scratch_runs(run, f'wino44 twin workspace split={split}')


def test_scratch_raster(dev):
    """lm_bev_raster_batch with a workspace of its own: the tiles, not the workspace, are compared."""
    from lanemapping_amd import ops, synth
    L = _lib()
    B, H, W, n = 2, 96, 128, 5000
    pts = torch.from_numpy(np.concatenate([synth.las_points(70 + b, n) for b in range(B)])).to(dev)
    pts[:, :2] *= 0.1                                              # a few points per pixel of the small tile
    offs = (C.c_long * (B + 1))(*[b * n for b in range(B + 1)])
    par = (type(ops.make_raster_params()) * B)(*[ops.make_raster_params(local_min_ele=-0.5, ele_reso=0.02) for _ in range(B)])
    need = L.lm_bev_raster_workspace_bytes(B, n, H, W)

    def run(byte):
        ws = _ws(need, byte, dev)
        f32 = torch.empty((B, 3, H, W), device=dev)
        u8 = torch.empty((B, H, W, 3), device=dev, dtype=torch.uint8)
        _chk(L.lm_bev_raster_batch(_s(), pts.data_ptr(), offs, par, B, ws.data_ptr(), ws.numel(), f32.data_ptr(), u8.data_ptr(), H, W))
        return {'f32': f32, 'u8': u8}
    out = _scratch_runs(run, 'bev_raster workspace')
    assert int(out['u8'].count_nonzero()) > 0


def test_scratch_voxelize_conv_outputs_las_select(dev, tmp_path):
    from lanemapping_amd import las_io, ops, synth
    from oracle import las_ref
    L = _lib()
    p = torch.from_numpy(synth.lidar_points(31, 20000)).to(dev)
    lo, vs, grid = (C.c_float * 3)(-15., -25., -2.), (C.c_float * 3)(0.3125, 0.5208334, 0.4), (C.c_int * 3)(96, 96, 10)
    need, cap = L.lm_voxelize_workspace_bytes(p.shape[0]), 700

    def vox(byte):
        ws = _ws(need, byte, dev)
        feats, coords = torch.zeros((cap, 16), device=dev), torch.zeros((cap, 4), device=dev, dtype=torch.int32)
        end = torch.zeros((1,), device=dev, dtype=torch.int32)
        _chk(L.lm_voxelize_hard(_s(), p.data_ptr(), p.shape[0], lo, vs, grid, 3, cap, 0, None, cap, feats.data_ptr(), 16, coords.data_ptr(),
                                end.data_ptr(), 0, ws.data_ptr(), ws.numel()))
        return {'feats': feats, 'coords': coords, 'end': end}
    v = _scratch_runs(vox, 'voxelize workspace')
    assert int(v['end']) == cap
    coords = v['coords'].contiguous()
    Do, Ho, Wo = 5, 48, 48
    cells = Do * Ho * Wo
    need2 = L.lm_sparse_conv_outputs_workspace_bytes(cells)

    def conv_out(byte):
        ws = _ws(need2, byte, dev)
        g_, oc = torch.zeros((1, Do, Ho, Wo), device=dev, dtype=torch.int32), torch.zeros((cells, 4), device=dev, dtype=torch.int32)
        cnt = torch.zeros((1,), device=dev, dtype=torch.int32)
        _chk(L.lm_sparse_conv_outputs(_s(), coords.data_ptr(), cap, 1, ops._ksp((3, 3, 3), (2, 2, 2), (1, 1, 1)), Do, Ho, Wo, g_.data_ptr(),
                                      oc.data_ptr(), cells, cnt.data_ptr(), ws.data_ptr(), need2))
        return {'grid': g_, 'coords': oc, 'count': cnt}
    assert int(_scratch_runs(conv_out, 'sparse_conv_outputs workspace')['count']) > 0
    n = 5000
    rng = np.random.RandomState(3)
    xyz = rng.rand(n, 3) * [57.6, 57.6, 3] + [351200.0, 3433000.0, 10.0]
    path = str(tmp_path / 's.las')
    las_ref.write_las(path, xyz, rng.randint(0, 65535, n), point_format=1, offset=(351000.0, 3433000.0, 0.0))
    data = np.fromfile(path, dtype=np.uint8)
    h = las_io.parse_header(data)
    rl, off = h['record_len'], h['offset_to_points']
    rec = torch.from_numpy(np.concatenate([data[off:off + n * rl], np.zeros(3, np.uint8)])[:(n * rl + 3) // 4 * 4].copy()).to(dev)
    sel = las_io.PointFilter(z_range=(10.5, 12.0)).for_format(1).as_struct()
    need3 = int(L.lm_las_select_workspace_bytes(n))
    d3 = lambda v: (C.c_double * 3)(*[float(t) for t in v])

    def select(byte):
        ws, out, meta = _ws(need3, byte, dev), torch.zeros((n, 4), device=dev), torch.zeros((257,), device=dev, dtype=torch.int64)
        _chk(L.lm_las_decode_select(_s(), rec.data_ptr(), rl, 1, n, d3(h['scale']), d3(h['offset']), None, las_io.INTEN_MIN, las_io.INTEN_MAX, 1,
                                    C.byref(sel), ws.data_ptr(), need3, out.data_ptr(), meta.data_ptr(), meta.data_ptr() + 8))
        return {'points': out, 'meta': meta}
    kept = int(_scratch_runs(select, 'las_decode_select workspace')['meta'][0])
    assert 0 < kept < n


# every test of this file needs the GPU, except the one that drives poisoned() with a fake library
for _name, _fn in list(globals().items()):
    if _name.startswith('test_') and _name != 'test_poisoned_wraps_every_stream_entry':
        pytest.mark.gpu(_fn)
