"""GPU: the colour of the markings (csrc/profile.hip: lm_las_line_colour_records, the <true> instantiation of las_profile_kernel;
las_io.profile_colour_records / survey_colour_las / marking_colours, Runner `colour=`).

The reference is tests/colour_ref.py on top of tests/profile_ref.py: which bin a return lands in is the profile's brute force, what it
adds to the colour row is plain integer numpy.  Both tables are compared in every int64, and bins also with what
lm_las_line_profile_records writes for the same arguments."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import colour_ref as cr
import label_ref as lr
import lds_state
import profile_ref as pr
from guards import Slab, guarded_runs
from lanemapping_amd import io_utils, las_io, ops
from lanemapping_amd._lib import lib
from lanemapping_amd.las_io import MarkingColour, MarkingSurvey, PointFilter
from oracle import las_ref

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float('nan')
POISON = -7
BIN = pr.BIN_EXACT                                                # 0.125 m: every border is a float32
SCALE, OFFSET = (2.0 ** -10,) * 3, tuple(lr.SHIFT)                # the decode gives X / 1024 exactly: a record's place is what the test says
YELLOW, WHITE, GREY = (60000, 50000, 10000), (60000, 60000, 58000), (20000, 21000, 22000)


@functools.lru_cache(maxsize=None)
def _scene():
    """-> (segments, stations, bin_start) of label_ref's lines: computed once, never changed."""
    lines = [l + lr.SHIFT for l in lr.scene_lines()]
    seg = las_io.line_segments(lines, lr.SHIFT)
    st, bs = las_io.line_stations(lines, lr.SHIFT, BIN)
    for a in (seg, st, bs):
        a.setflags(write=False)
    return seg, st, bs


def _device_tables(dev):
    seg, st, bs = _scene()
    return ops.line_index(seg, lr.HW, device=dev), ops.line_stations(st, bs, BIN, device=dev)


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _make(fmt, extra, local, inten, rgb, seed=0):
    """[n, record_len] records of format `fmt` at the places `local` ([n, 3], metres in the shifted frame, quantised to 1/1024 m), junk in
    every other field, classification 2 for four records of five and 7 for the fifth, then the triples."""
    local = np.asarray(local, np.float64)
    n, rl = len(local), cr.MIN_LEN[fmt] + extra
    rec = np.zeros((n, rl), np.uint8)
    rec[:, 0:12] = np.round(local * 1024.0).astype('<i4').view(np.uint8).reshape(n, 12)
    rec[:, 12:14] = np.asarray(inten).astype('<u2').reshape(n, 1).view(np.uint8)
    rec[:, 14:] = ((np.arange(n)[:, None] + seed) * 7 + np.arange(rl - 14)[None, :]) % 251
    cls = np.where(np.arange(n) % 5 == 4, 7, 2)
    if fmt >= 6:
        rec[:, 16] = cls
    else:
        rec[:, 15] = (rec[:, 15] & 0xE0) | cls
    return cr.put_rgb(rec, fmt, rgb)


def _random(fmt, extra, n, seed):
    """n records around the scene's lines: intensities 0..1999; one triple in eight black, the others spread on both sides of the vote."""
    seg = _scene()[0]
    rng = np.random.RandomState(seed)
    s = rng.randint(0, len(seg), n)
    base = seg[s, 0:3].astype(np.float64) + rng.uniform(0, 1, n)[:, None] * seg[s, 3:6].astype(np.float64)
    off = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), rng.uniform(-0.7, 0.7, n)], axis=1)
    rgb = rng.randint(0, 65536, (n, 3))
    rgb[rng.randint(0, 8, n) == 0] = 0
    small = rng.randint(0, 4, n) == 1                              # 8-bit values in the 16-bit fields
    rgb[small] = rgb[small] >> 8
    return _make(fmt, extra, base + off, rng.randint(0, 2000, n), rgb, seed)


def _flat(rec):
    flat = np.zeros((rec.size + 3) // 4 * 4, np.uint8)
    flat[:rec.size] = rec.reshape(-1)
    return flat


def _header(fmt, rec):
    return {'point_format': fmt, 'record_len': rec.shape[1], 'n_points': len(rec), 'scale': SCALE, 'offset': OFFSET}


def _passes(rec, fmt, select):
    if select is None:
        return None
    cls = rec[:, 16] if fmt >= 6 else rec[:, 15] & 31
    withheld = (rec[:, 15] & 4) != 0 if fmt >= 6 else (rec[:, 15] & 128) != 0
    keep = np.isin(cls, np.asarray(select.classes)) if select.classes is not None else np.ones(len(rec), bool)
    assert select.returns == 'all' and select.z_range is None and not (select.drop_synthetic or select.drop_keypoint or select.drop_overlap)
    return keep & ~(withheld & select.drop_withheld)


def _want(rec, fmt, blue_q, min_intensity=None, select=None, bins=None, colours=None):
    """The brute force on the records: -> (bins, colours, terms, line)."""
    seg, st, bs = _scene()
    return cr.colour_f32(lr.decode_f32(rec, SCALE, OFFSET, lr.SHIFT), cr.get_rgb(rec, fmt), seg, st, bs, BIN, lr.HW, lr.ZTOL, blue_q, min_intensity,
                         _passes(rec, fmt, select), bins, colours)


def _got(dev, tables, rec, fmt, colour=MarkingColour(), min_intensity=None, select=None, out=None):
    survey = MarkingSurvey(BIN, lr.HW, lr.ZTOL, min_intensity=min_intensity)
    d_rec = torch.from_numpy(_flat(rec)).to(dev)
    before = d_rec.clone()
    pair = las_io.profile_colour_records(d_rec, _header(fmt, rec), *tables, survey, colour, lr.SHIFT, select, out=out)
    assert torch.equal(d_rec, before), 'the records were written'
    return pair


def _same(tag, got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.int64 and got.shape == want.shape, f'{tag}: {got.dtype} {got.shape}'
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), f'{tag}: {len(bad)} rows differ from the brute force; first row {bad[0]}: {got[bad[0]].tolist()} != {want[bad[0]].tolist()}'


# ------------------------------------------------------------------------------------------------ 1. bit equality
@pytest.mark.parametrize('fmt', cr.COLOUR_FORMATS)
def test_both_tables_equal_the_brute_force(dev, fmt):
    """Every colour format at its minimum record length and with 1 and 3 bytes of padding (records and colour words then straddle the
    dwords of the stage), at 1, 255, 256, 257 and 513 records: the block seam of 256 and a tail block.  The first n records of one
    drawing of 513, so one brute force serves all five."""
    seg, st, bs = _scene()
    tables = _device_tables(dev)
    survey = MarkingSurvey(BIN, lr.HW, lr.ZTOL)
    n_bins = int(bs[-1])
    for extra in (0, 1, 3):
        rec = _random(fmt, extra, 513, seed=10 * fmt + extra)
        rl = rec.shape[1]
        assert rl == cr.MIN_LEN[fmt] + extra
        rgb = cr.get_rgb(rec, fmt)
        for min_intensity in (None, 700.0):
            _, _, terms, line = _want(rec, fmt, 768, min_intensity)
            assert (line > 0).sum() > 50 and (line == 0).sum() > 50
            for n in (1, 255, 256, 257, 513):
                tag = f'format {fmt}, {rl} B, n={n}, min_intensity={min_intensity}'
                want_b = pr.accumulate({k: v[:n] for k, v in terms.items()}, n_bins)
                want_c = cr.accumulate(terms['B'][:n], rgb[:n], 768, n_bins)
                bins, colours = _got(dev, tables, rec[:n], fmt, min_intensity=min_intensity)
                _same(tag + ': bins', bins, want_b)
                _same(tag + ': colours', colours, want_c)
                plain = las_io.profile_records(torch.from_numpy(_flat(rec[:n])).to(dev), _header(fmt, rec[:n]), *tables,
                                               MarkingSurvey(BIN, lr.HW, lr.ZTOL, min_intensity=min_intensity), lr.SHIFT)
                assert torch.equal(bins, plain), f'{tag}: bins differ from lm_las_line_profile_records'
            assert want_c[:, 0].sum() > 20 and want_c[:, 4].sum() > 5 and want_c[:, 5].sum() > 2 and want_c[:, 0].sum() > want_c[:, 4].sum(), \
                'the drawing holds coloured, yellow and black returns on the lines'
            assert (want_c[:, 0] + want_c[:, 5] == want_b[:, 0]).all(), 'every profiled return is coloured or black'


# ------------------------------------------------------------------------------------------------ 2. the wave merge
def _on_line_1(bins_of_lane):
    """Places on line 1 (y = 2, climbing 1 %), in the middle of bin k of 0.125 m for every lane; k < 0: far beside every line."""
    k = np.asarray(bins_of_lane, np.float64)
    x = 0.0625 + 0.125 * np.maximum(k, 0)
    return np.stack([x, np.where(k >= 0, 2.0, 300.0), np.round(0.01 * x * 1024) / 1024], axis=1)


def test_wave_merge_paths(dev):
    tables = _device_tables(dev)
    fmt = 7
    ones = np.ones(64, np.int64)
    # all 64 lanes of a wave in one bin, R = G = B = 65535: the 32-bit partial sums at their maximum
    rec = _make(fmt, 0, _on_line_1(0 * ones), 1000 * ones, np.full((64, 3), 65535))
    want_b, want_c, _, line = _want(rec, fmt, 768)
    assert (line == 1).all() and want_c[0].tolist() == [64, 64 * 65535, 64 * 65535, 64 * 65535, 0, 0] and want_c[1:].sum() == 0
    bins, colours = _got(dev, tables, rec, fmt)
    _same('64 x white at the maximum: bins', bins, want_b), _same('64 x white at the maximum: colours', colours, want_c)
    # ... and voting yellow at the maximum of R and G
    rec = _make(fmt, 0, _on_line_1(0 * ones), 1000 * ones, np.tile([65535, 65535, 0], (64, 1)))
    want_c = _want(rec, fmt, 768)[1]
    assert want_c[0].tolist() == [64, 64 * 65535, 64 * 65535, 0, 64, 0]
    _same('64 x yellow', _got(dev, tables, rec, fmt)[1], want_c)
    # the same wave with every return black
    rec = _make(fmt, 0, _on_line_1(0 * ones), 1000 * ones, np.zeros((64, 3), np.int64))
    want_b, want_c, _, _ = _want(rec, fmt, 768)
    assert want_c[0].tolist() == [0, 0, 0, 0, 0, 64] and want_b[0, 0] == 64
    bins, colours = _got(dev, tables, rec, fmt)
    _same('64 x black: bins', bins, want_b), _same('64 x black: colours', colours, want_c)
    # a wave with exactly one hitting lane: the shortcut - coloured, then black
    for rgb, row in ((YELLOW, [1, *YELLOW, 1, 0]), ((0, 0, 0), [0, 0, 0, 0, 0, 1])):
        k = -ones
        k[17] = 5
        rec = _make(fmt, 0, _on_line_1(k), 1000 * ones, np.tile(rgb, (64, 1)))
        want_c, line = _want(rec, fmt, 768)[1::2]
        assert (line > 0).sum() == 1 and line[17] == 1 and want_c[5].tolist() == row and want_c.sum() == sum(row)
        _same(f'one lane alone, {rgb}', _got(dev, tables, rec, fmt)[1], want_c)
    # a wave whose lanes fall into three bins with different colours (and, lane by lane, different triples), over three waves
    j = np.arange(192)
    rgb = np.stack([40000 + 101 * j, 30000 + 97 * (j % 50), 5000 * (j % 3) * (j % 7)], axis=1)
    rgb[j % 3 == 1] = np.asarray(WHITE) - (j[j % 3 == 1] % 9)[:, None]
    rgb[(j % 3 == 2) & (j % 4 == 0)] = 0
    rec = _make(fmt, 3, _on_line_1(j % 3), 1000 + j, rgb)
    want_b, want_c, terms, _ = _want(rec, fmt, 768)
    assert np.array_equal(terms['B'], j % 3) and (want_b[:3, 0] == 64).all()
    assert want_c[0, 4] == 64 and want_c[1, 4] == 0 and want_c[1, 0] == 64 and want_c[2, 5] == 16 and 0 < want_c[2, 4] < want_c[2, 0] == 48
    bins, colours = _got(dev, tables, rec, fmt)
    _same('three bins: bins', bins, want_b), _same('three bins: colours', colours, want_c)
    # two lanes of a wave alone in their bins beside 62 lanes in one
    k = 0 * ones
    k[5], k[40] = 72, 88
    rec = _make(fmt, 1, _on_line_1(k), 1000 * ones, rgb[:64])
    want_c = _want(rec, fmt, 768)[1]
    assert want_c[0, 0] + want_c[0, 5] == 62 and want_c[72].tolist()[0] + want_c[72, 5] == 1 and want_c[88, 0] + want_c[88, 5] == 1
    _same('62 + 1 + 1', _got(dev, tables, rec, fmt)[1], want_c)
    # yellow votes on both sides of equality: 2048 B == blue_q (R + G) is not yellow, one unit less of B is
    for blue_q, ratio, at in ((768, 0.75, (40000, 40000, 30000)), (1024, 1.0, (300, 100, 200)), (1, 1 / 1024, (65535, 1, 32)),
                              (512, 0.5, (255, 1, 64))):
        assert MarkingColour(yellow_ratio=ratio).blue_q == blue_q and 2048 * at[2] == blue_q * (at[0] + at[1])
        below = (at[0], at[1], at[2] - 1)
        rec = _make(fmt, 0, _on_line_1(j[:128] % 2), 1000 * np.ones(128), np.where((j[:128] % 2 == 0)[:, None], at, below))
        want_c = _want(rec, fmt, blue_q)[1]
        assert want_c[0].tolist() == [64, 64 * at[0], 64 * at[1], 64 * at[2], 0, 0] and want_c[1, 4] == 64 == want_c[1, 0]
        _same(f'equality at blue_q={blue_q}', _got(dev, tables, rec, fmt, MarkingColour(yellow_ratio=ratio))[1], want_c)
    # blue_q at its two ends on a drawing
    rec = _random(3, 1, 513, seed=77)
    counts = []
    for ratio, blue_q in ((1 / 1024, 1), (1.0, 1024)):
        want_b, want_c, _, _ = _want(rec, 3, blue_q)
        bins, colours = _got(dev, tables, rec, 3, MarkingColour(yellow_ratio=ratio))
        _same(f'blue_q={blue_q}: bins', bins, want_b), _same(f'blue_q={blue_q}: colours', colours, want_c)
        counts.append(int(want_c[:, 4].sum()))
    assert counts[0] < counts[1] and counts[1] > 10


# ------------------------------------------------------------------------------------------------ 3. order and accumulation
def test_order_changes_no_bit_and_files_accumulate(dev):
    tables = _device_tables(dev)
    fmt = 5
    rec = _random(fmt, 1, 1500, seed=3)
    want_b, want_c, _, line = _want(rec, fmt, 768, 500.0)
    assert (line > 0).sum() > 100
    for seed in (1, 2):
        perm = rec[np.random.RandomState(seed).permutation(len(rec))]
        for attempt in range(2):
            bins, colours = _got(dev, tables, perm, fmt, min_intensity=500.0)
            _same(f'permutation {seed}, run {attempt}: bins', bins, want_b), _same(f'permutation {seed}, run {attempt}: colours', colours, want_c)
    # two files, of two formats, into one pair of tables: the brute force over their union
    other = _random(8, 3, 700, seed=4)
    first = _got(dev, tables, rec, fmt, min_intensity=500.0)
    both = _got(dev, tables, other, 8, min_intensity=500.0, out=first)
    assert both[0].data_ptr() == first[0].data_ptr() and both[1].data_ptr() == first[1].data_ptr()
    union_b, union_c, _, _ = _want(other, 8, 768, 500.0, bins=want_b, colours=want_c)
    assert union_c[:, 0].sum() > want_c[:, 0].sum()
    _same('two files: bins', both[0], union_b), _same('two files: colours', both[1], union_c)
    # a fresh call initialises both tables, whatever they held
    index, stations = tables
    n_bins = stations.n_bins
    bins = torch.full((n_bins, 6), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    colours = torch.full((n_bins, 6), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    d_rec = torch.from_numpy(_flat(rec)).to(dev)
    d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])
    rc = lib().lm_las_line_colour_records(_stream(dev), C.c_void_p(d_rec.data_ptr()), rec.shape[1], fmt, len(rec), d3(SCALE), d3(OFFSET),
                                          d3(lr.SHIFT), None, *index.args(), *stations.args(), lr.ZTOL, 500.0, 768, 0,
                                          C.c_void_p(bins.data_ptr()), C.c_void_p(colours.data_ptr()), n_bins)
    assert rc == 0, lib().lm_last_error()
    _same('accumulate=0 on poison: bins', bins, want_b), _same('accumulate=0 on poison: colours', colours, want_c)
    # no record, and no bins: LM_OK after the initialisation
    empty = _got(dev, tables, rec[:0], fmt)
    _same('n=0: bins', empty[0], pr.accumulate({'B': np.zeros(0, np.int64), 'q': np.zeros(0, np.int64), 'iq': np.zeros(0, np.int64)}, n_bins))
    assert not bool(empty[1].any()) and tuple(empty[1].shape) == (n_bins, 6)
    with pytest.raises(ValueError, match='out must be'):
        _got(dev, tables, rec, fmt, out=(first[0], first[1][:-1]))
    with pytest.raises(ValueError, match='pair'):
        _got(dev, tables, rec, fmt, out=first[0])


# ------------------------------------------------------------------------------------------------ 4. select
@pytest.mark.parametrize('fmt, extra', [(3, 0), (8, 1)])
def test_dropped_records_reach_neither_table(dev, fmt, extra):
    tables = _device_tables(dev)
    rec = _random(fmt, extra, 1200, seed=fmt)
    every_b, every_c, _, _ = _want(rec, fmt, 768)
    for name, select in (('class 2 only', PointFilter(classes=[2], drop_withheld=False)), ('no withheld', PointFilter())):
        ok = _passes(rec, fmt, select)
        assert 100 < ok.sum() < len(rec) - 100, name
        want_b, want_c, _, _ = _want(rec, fmt, 768, select=select)
        assert want_b[:, 0].sum() < every_b[:, 0].sum() and want_c[:, 0].sum() < every_c[:, 0].sum(), f'{name}: a dropped record lies on a line'
        bins, colours = _got(dev, tables, rec, fmt, select=select)
        _same(f'format {fmt}, {name}: bins', bins, want_b), _same(f'format {fmt}, {name}: colours', colours, want_c)


# ------------------------------------------------------------------------------------------------ 5. guards and LDS
def _bins_of(slab_view):
    return np.ascontiguousarray(slab_view.numpy()).view(np.int64)


def test_colour_records_guards(dev):
    """lm_las_line_colour_records with the records, the tables, bins and colours each between guard slabs: 257 records of 37 bytes (the
    last dword of the records is padding, the last block holds one record), with a select; then the same call on plain tensors after
    every word of lds_state.WORDS in LDS."""
    seg, st, bs = _scene()
    fmt, n = 7, 257
    rec = _random(fmt, 1, n, seed=7)
    rl, flat = rec.shape[1], _flat(rec)
    assert rl == 37 and len(flat) == n * rl + 3
    g, start, segs = ops.line_index_host(seg, lr.HW)
    n_bins, host = int(bs[-1]), np.array(bs, np.int32)
    sel = PointFilter(classes=[2], drop_withheld=False)
    want_b, want_c, _, _ = _want(rec, fmt, 768, select=sel)
    assert want_c[:, 0].sum() > 10 and want_c[:, 4].sum() > 0 and want_c[:, 5].sum() > 0
    d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])
    sst = sel.as_struct()
    t = lambda a: torch.from_numpy(np.array(a, copy=True))

    def run(B, poisoned):
        s_rec = Slab(dev, 1, len(flat), front=1, back=1, dtype=torch.uint8).fill_input(torch.from_numpy(flat), 0xFF if poisoned else 0)
        s_seg = Slab(dev, len(seg), 8, front=4, back=4).fill_input(t(seg), NAN if poisoned else 0.0)
        s_start = Slab(dev, 1, len(start), front=1, back=1, dtype=torch.int32).fill_input(torch.from_numpy(start), 0x7FFFFFF0 if poisoned else 0)
        s_segs = Slab(dev, 1, len(segs), front=1, back=1, dtype=torch.int32).fill_input(torch.from_numpy(segs), 0x7FFFFFF0 if poisoned else 0)
        s_st = Slab(dev, len(st), 4, front=8, back=8).fill_input(t(st), NAN if poisoned else 0.0)
        s_bs = Slab(dev, 1, len(bs), front=1, back=1, dtype=torch.int32).fill_input(t(bs), 0x7FFFFFF0 if poisoned else 0)
        s_bins = Slab(dev, n_bins, 12, front=8, back=8, dtype=torch.int32).fill_canary()
        s_col = Slab(dev, n_bins, 12, front=8, back=8, dtype=torch.int32).fill_canary()
        ins = (s_rec, s_seg, s_start, s_segs, s_st, s_bs)
        before = [s.bits().clone() for s in ins]
        rc = lib().lm_las_line_colour_records(_stream(dev), C.c_void_p(s_rec.ptr()), rl, fmt, n, d3(SCALE), d3(OFFSET), d3(lr.SHIFT),
                                              C.byref(sst), C.c_void_p(s_seg.ptr()), len(seg), C.byref(g), C.c_void_p(s_start.ptr()),
                                              C.c_void_p(s_segs.ptr()), lr.HW, C.c_void_p(s_st.ptr()), C.c_void_p(s_bs.ptr()),
                                              C.c_void_p(host.ctypes.data), len(bs) - 1, BIN, lr.ZTOL, NAN, 768, 0, C.c_void_p(s_bins.ptr()),
                                              C.c_void_p(s_col.ptr()), n_bins)
        assert rc == 0, lib().lm_last_error()
        torch.cuda.synchronize()
        for s, b in zip(ins, before):
            assert torch.equal(s.bits(), b), 'an input was written'
        return {'bins': (s_bins, n_bins), 'colours': (s_col, n_bins)}

    for attempt in range(2):                                             # the second round: the same bits again
        got = guarded_runs(run, 'las_line_colour_records', batch=False)
        _same('guarded: bins', _bins_of(got['bins']), want_b), _same('guarded: colours', _bins_of(got['colours']), want_c)
    # the colour instantiation after poisoned LDS: it reads only what las_stage_block staged for the current block
    tables = _device_tables(dev)
    d_rec = torch.from_numpy(flat).to(dev)
    survey = MarkingSurvey(BIN, lr.HW, lr.ZTOL)

    def plain():
        bins, colours = las_io.profile_colour_records(d_rec, _header(fmt, rec), *tables, survey, MarkingColour(), lr.SHIFT, sel)
        return {'bins': bins, 'colours': colours}

    got = lds_state.lds_state_runs(plain, 'las_line_colour_records')
    _same('after poisoned LDS: bins', got['bins'], want_b), _same('after poisoned LDS: colours', got['colours'], want_c)
    for word in lds_state.WORDS:
        with lds_state.poisoned(word) as state:
            out = plain()
            torch.cuda.synchronize()
        assert state.fills == 1
        _same(f'LDS = 0x{word:08X}: bins', out['bins'], want_b), _same(f'LDS = 0x{word:08X}: colours', out['colours'], want_c)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_the_argument_and_write_nothing(dev):
    index, stations = _device_tables(dev)
    n_bins, n, fmt = stations.n_bins, 300, 3
    rec = _random(fmt, 0, n, seed=1)
    d_rec = torch.from_numpy(_flat(rec)).to(dev)
    both = torch.full((2 * n_bins + 1, 6), POISON, dtype=torch.int64, device=dev)
    bins, colours = both[:n_bins], both[n_bins:2 * n_bins]
    L = lib()
    d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])
    # positions: records 1, record_len 2, point_format 3, n 4, scale 5, select 8, segments 9, grid 11, half_width 14, stations 15, bin 19,
    # z_tol 20, min_intensity 21, blue_q 22, accumulate 23, bins 24, colours 25, n_bins 26
    base = [_stream(dev), C.c_void_p(d_rec.data_ptr()), rec.shape[1], fmt, n, d3(SCALE), d3(OFFSET), d3(lr.SHIFT), None, *index.args(),
            *stations.args(), lr.ZTOL, NAN, 768, 0, C.c_void_p(bins.data_ptr()), C.c_void_p(colours.data_ptr()), n_bins]
    assert len(base) == 27
    assert L.lm_las_line_colour_records(*base) == 0, L.lm_last_error()
    torch.cuda.synchronize()
    assert bool((bins[:, 0] >= 0).all()) and bool((colours >= 0).all()) and int(colours[:, 0].sum()) > 0
    both.fill_(POISON)

    def refused(what, **change):
        a = list(base)
        for pos, v in change.items():
            a[int(pos[1:])] = v
        rc = L.lm_las_line_colour_records(*a)
        torch.cuda.synchronize()
        msg = L.lm_last_error().decode()
        assert rc == 1 and msg.startswith('las_line_colour_records:') and what in msg, f'{what}: rc={rc}, message {msg!r}'
        assert bool((both == POISON).all()), f'{what}: bins or colours was written'

    # what this entry adds: a format without colour (with a record length that format allows), blue_q, colours
    for f in (0, 1, 4, 6, 9):
        refused(f'point_format={f} carries no RGB', p3=f, p2=max(cr.MIN_LEN[f], rec.shape[1]))
    for q in (0, 1025, -1):
        refused(f'blue_q={q}', p22=q)
    refused('colours is not 8-byte aligned', p25=C.c_void_p(colours.data_ptr() + 4))
    refused('null pointer (colours)', p25=None)
    refused('colours overlaps bins', p25=C.c_void_p(bins.data_ptr()))
    refused('colours overlaps bins', p25=C.c_void_p(bins.data_ptr() + 48 * (n_bins - 1)))
    refused('colours overlaps bins', p24=C.c_void_p(colours.data_ptr() + 48), p25=C.c_void_p(colours.data_ptr()))
    # what lm_las_line_profile_records refuses, through this entry
    refused('bins is not', p24=C.c_void_p(bins.data_ptr() + 4))
    refused('bins', p24=None)
    refused('records is not', p1=C.c_void_p(d_rec.data_ptr() + 1))
    refused('record_len', p2=33)
    refused('point_format', p3=11)
    refused('n=', p4=-1)
    refused('scale', p5=None)
    refused('n_bins', p26=n_bins + 1)
    refused('accumulate', p23=2)
    refused('bin=', p19=0.0)
    refused('z_tol', p20=NAN)
    refused('half_width', p14=-1.0)
    refused('stations', p15=None)
    refused('segments', p9=None)
    # the package entries
    header = _header(fmt, rec)
    survey = MarkingSurvey(BIN, lr.HW, lr.ZTOL)
    with pytest.raises(ValueError, match='point format 1 carries no RGB'):
        las_io.profile_colour_records(d_rec, dict(header, point_format=1), index, stations, survey, MarkingColour(), lr.SHIFT)
    with pytest.raises(TypeError, match='MarkingColour'):
        las_io.profile_colour_records(d_rec, header, index, stations, survey, survey, lr.SHIFT)
    with pytest.raises(TypeError, match='MarkingSurvey'):
        las_io.profile_colour_records(d_rec, header, index, stations, MarkingColour(), MarkingColour(), lr.SHIFT)
    with pytest.raises(ValueError, match='bin='):
        las_io.profile_colour_records(d_rec, header, index, stations, MarkingSurvey(0.5, lr.HW, lr.ZTOL), MarkingColour(), lr.SHIFT)
    torch.cuda.synchronize()
    assert bool((both == POISON).all())


# ------------------------------------------------------------------------------------------------ 7. painted patches
def test_survey_colour_las_tells_yellow_from_white(dev, tmp_path, monkeypatch):
    """Four lines from x = 0 to 24 at y = 2, 6, 10, 14 over returns at x = 0.025 + 0.05 i, y = 0.025 + 0.05 j (24 m x 16 m), painted
    (intensity 24000, else 3000) in the two rows beside each line where floor(x / 3) is even, as in the profile's patch test.  Line 1 is
    painted yellow, line 2 white, line 3 white up to x = 12 and yellow beyond, the paint of line 4 was seen by no camera (black).  The
    asphalt is grey.  The cloud is split over a format-3 and a format-7 file."""
    i, j = np.meshgrid(np.arange(480), np.arange(320), indexing='ij')
    i, j = i.ravel(), j.ravel()
    x, y = (2 * i + 1) * 0.025, (2 * j + 1) * 0.025
    lane = (j // 80)
    paint = ((i // 60) % 2 == 0) & (np.abs(2 * (j % 80) + 1 - 80) < 3)
    assert paint.sum() == 4 * 4 * 60 * 2
    inten = np.where(paint, 24000, 3000)
    rgb = np.tile(GREY, (len(x), 1))
    rgb[paint & (lane == 0)] = YELLOW
    rgb[paint & (lane == 1)] = WHITE
    rgb[paint & (lane == 2)] = WHITE
    rgb[paint & (lane == 2) & (x > 12)] = (255, 210, 40)                 # 8-bit values in the 16-bit fields: the vote does not care
    rgb[paint & (lane == 3)] = 0
    world = np.stack([x, y, np.zeros_like(x)], axis=1) + lr.SHIFT
    order = np.random.RandomState(11).permutation(len(world))
    half = len(order) // 2
    paths, recs = [], []
    for k, part in enumerate((order[:half], order[half:])):
        paths.append(str(tmp_path / f'patch{k}.las'))
        recs.append(cr.write_colour_las(paths[k], world[part], inten[part], rgb[part], (3, 7)[k], offset=tuple(lr.SHIFT), extra_bytes=k))
    xs = np.arange(0.0, 26.0, 2.0)
    lines = [np.stack([xs, np.full_like(xs, 2.0 + 4.0 * l), np.zeros_like(xs)], axis=1) + lr.SHIFT for l in range(4)]
    survey, colour = MarkingSurvey(bin=0.25, min_intensity=10000), MarkingColour()
    # the reference's own numbers first
    seg = las_io.line_segments(lines, lr.SHIFT)
    st, bs = las_io.line_stations(lines, lr.SHIFT, survey.bin)
    assert bs.tolist() == [0, 96, 192, 288, 384]
    dec = np.concatenate([(world - lr.SHIFT), inten[:, None]], axis=1).astype(f32)
    want_b, want_c, _, lab = cr.colour_f32(dec, rgb, seg, st, bs, survey.bin, survey.half_width, survey.z_tol, colour.blue_q,
                                           survey.min_intensity, pruned=True)
    assert (lab > 0).sum() == paint.sum()
    on = np.tile((np.arange(96) // 12) % 2 == 0, 4)
    assert (want_b[on, 0] == 10).all() and (want_b[~on, 0] == 0).all()
    assert (want_c[:96][on[:96]] == [10, 600000, 500000, 100000, 10, 0]).all() and (want_c[288:][on[288:]] == [0, 0, 0, 0, 0, 10]).all()
    # one read-back: count what leaves the device
    copies = []
    real_cpu, real_item, real_tolist, real_to = torch.Tensor.cpu, torch.Tensor.item, torch.Tensor.tolist, torch.Tensor.to
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (copies.append('cpu') if self.is_cuda else None, real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, 'item', lambda self: (copies.append('item') if self.is_cuda else None, real_item(self))[1])
    monkeypatch.setattr(torch.Tensor, 'tolist', lambda self: (copies.append('tolist') if self.is_cuda else None, real_tolist(self))[1])

    def to(self, *a, **k):
        res = real_to(self, *a, **k)
        if self.is_cuda and not res.is_cuda:
            copies.append('to')
        return res

    monkeypatch.setattr(torch.Tensor, 'to', to)
    bins, colours, bin_start = las_io.survey_colour_las(paths, lines, survey, colour, lr.SHIFT, device=dev)
    monkeypatch.undo()
    assert copies == ['cpu'], f'device-to-host copies: {copies}'
    assert bin_start.tolist() == bs.tolist()
    _same('survey_colour_las: bins', bins, want_b), _same('survey_colour_las: colours', colours, want_c)
    plain, _ = las_io.survey_las(paths, lines, survey, lr.SHIFT, device=dev)
    assert np.array_equal(plain, bins), 'bins differ from survey_las'
    got = las_io.marking_colours(bins, colours, bin_start, survey, colour)
    assert got == cr.colours_of(want_b, want_c, bs, survey.bin, survey.min_points, survey.max_gap, colour.yellow_share, colour.min_coloured)
    summary = las_io.marking_summary(bins, bin_start, survey)
    assert all(m['runs'] == [[0.0, 3.0], [6.0, 9.0], [12.0, 15.0], [18.0, 21.0]] for m in summary)
    assert got[0] == {'coloured': 480, 'yellow': 480, 'black': 0, 'rgb': [60000.0, 50000.0, 10000.0], 'colour': 'yellow', 'run_colours': ['yellow'] * 4}
    assert got[1] == {'coloured': 480, 'yellow': 0, 'black': 0, 'rgb': [60000.0, 60000.0, 58000.0], 'colour': 'white', 'run_colours': ['white'] * 4}
    assert got[2]['run_colours'] == ['white', 'white', 'yellow', 'yellow'] and (got[2]['coloured'], got[2]['yellow']) == (480, 240)
    assert got[2]['colour'] == 'yellow', 'half of the votes reach yellow_share = 0.5'
    assert got[3] == {'coloured': 0, 'yellow': 0, 'black': 480, 'rgb': None, 'colour': 'unknown', 'run_colours': ['unknown'] * 4}
    # a file without colour among them is refused by name and format before anything is uploaded
    grey = str(tmp_path / 'grey.las')
    las_ref.write_las(grey, world[:10], inten[:10], point_format=1, offset=tuple(lr.SHIFT))
    with pytest.raises(ValueError, match='grey.las is of point format 1'):
        las_io.survey_colour_las([paths[0], grey], lines, survey, colour, lr.SHIFT, device=dev)
    # no file: the empty tables
    b0, c0, s0 = las_io.survey_colour_las([], lines, survey, colour, lr.SHIFT, device=dev)
    assert s0.tolist() == bs.tolist() and not c0.any() and c0.shape == b0.shape == (384, 6) and (b0[:, 4] == 2 ** 31 - 1).all()


# ------------------------------------------------------------------------------------------------ 8. Runner
def _strip(tmp_path):
    """The strip of tests/test_gpu_profile.py's Runner test (a copy of its generator) in point format 3: three overlapping 1152 x 1152
    tiles over a climbing plane, one point at every pixel centre, six painted stripes - the first two yellow, the others white, the
    asphalt grey, every 11th return black.  -> (las path, parameter file paths, read offset, records)."""
    H = W = 1152
    reso, ele, A, Bs = 0.05, 0.05, 0.075, 0.02
    off = np.array([351200.0, 3433000.0, 12.0])
    step = 1024
    rows = 2 * step + H
    r, c = np.meshgrid(np.arange(rows), np.arange(W), indexing='ij')
    x, y = (r * reso).ravel(), (c * reso).ravel()
    lane_y = [(0.12 + 0.152 * l) * 57.6 + 0.01 * (l - 2.5) * x for l in range(6)]
    paint = np.zeros(len(x), bool)
    rgb = np.tile(GREY, (len(x), 1))
    for l, ly in enumerate(lane_y):
        stripe = np.abs(y - ly) < 0.075
        paint |= stripe
        rgb[stripe] = YELLOW if l < 2 else WHITE
    rgb[np.arange(len(x)) % 11 == 0] = 0
    inten = np.where(paint, 24000.0, 3000.0 + 40.0 * ((r + 3 * c) % 97).ravel())
    world = np.stack([x, y, A * x + Bs * y], axis=1)
    order = np.random.RandomState(3).permutation(len(world))
    las = str(tmp_path / 'strip.las')
    rec = cr.write_colour_las(las, world[order] + off, inten[order], rgb[order], 3, offset=tuple(off))
    prm_paths = []
    for t in range(3):
        p = {'coor_las_path': '', 'las_read_offset': list(off), 'las_rotation_trans_quan': [t * step * reso, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0],
             'bev_img_offset': [0.0, 0.0], 'img_reso': [reso, reso], 'local_min_ele': -0.5, 'ele_reso': ele}
        prm_paths.append(str(tmp_path / f'18102{t}_0209.txt'))
        io_utils.save_pc_2_img_transform_paras(prm_paths[t], p)
    return las, prm_paths, off, rec


def test_runner_strip_surveys_the_colours_of_its_lines(dev, net, tmp_path):
    """Runner.infer_las_strip_to_map with survey= and colour= on a colourised strip: params/marking_colours.npy equals the brute force
    against the lines the call returned, params/markings.json carries the keys of marking_summary and of marking_colours,
    params/markings.npy holds the bytes of a run with survey= alone, which writes no marking_colours.npy; the return values agree.
    colour= without survey=, and an input file without colour, are refused before any output file exists."""
    from lanemapping_amd.runner import Runner
    las, prm_paths, off, rec = _strip(tmp_path)
    rn = Runner.__new__(Runner)
    rn.cfg, rn.device, rn.net = net.cfg, dev, net
    assert rn.cfg.get('las_colour') is None
    out = {k: str(tmp_path / k) for k in ('survey', 'colour', 'alone', 'grey')}
    survey, colour = MarkingSurvey(min_intensity=10000.0), MarkingColour()
    with pytest.raises(ValueError, match='pass survey='):
        rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['alone'], batch_size=2, colour=colour)
    grey = str(tmp_path / 'grey.las')
    las_ref.write_las(grey, np.zeros((8, 3)) + off, np.zeros(8), point_format=1, offset=tuple(off))
    with pytest.raises(ValueError, match='grey.las is of point format 1'):
        rn.infer_las_strip_to_map([las, grey], prm_paths, work_dirs=out['grey'], batch_size=2, survey=survey, colour=colour)
    with pytest.raises(ValueError, match='grey.las is of point format 1'):
        rn.infer_las_to_map([(grey, prm_paths[0])], work_dirs=out['grey'], survey=survey, colour=colour)
    assert not os.path.exists(out['alone']) and not os.path.exists(out['grey'])
    plain = rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['survey'], batch_size=2, survey=survey)
    lines3d, merged = rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['colour'], batch_size=2, survey=survey, colour=colour)
    assert sorted(plain[0]) == sorted(lines3d) and len(plain[1]) == len(merged) and all(np.array_equal(a, b) for a, b in zip(plain[1], merged))
    par = {k: os.path.join(out[k], 'params') for k in ('survey', 'colour')}
    assert not os.path.exists(os.path.join(par['survey'], 'marking_colours.npy')) and os.path.exists(os.path.join(par['colour'], 'marking_colours.npy'))
    assert open(os.path.join(par['survey'], 'markings.npy'), 'rb').read() == open(os.path.join(par['colour'], 'markings.npy'), 'rb').read()
    lines = list(merged) if len(merged) else [l for name in sorted(lines3d) for l in lines3d[name]]
    assert lines, 'the strip yielded no lines'
    h = las_io.parse_header(np.fromfile(las, np.uint8))
    seg = las_io.line_segments(lines, off)
    st, bs = las_io.line_stations(lines, off, survey.bin)
    want_b, want_c, _, line = cr.colour_f32(lr.decode_f32(rec, h['scale'], h['offset'], off), cr.get_rgb(rec, 3), seg, st, bs, survey.bin,
                                            survey.half_width, survey.z_tol, colour.blue_q, survey.min_intensity, pruned=True)
    _same('markings.npy', np.load(os.path.join(par['colour'], 'markings.npy')), want_b)
    _same('marking_colours.npy', np.load(os.path.join(par['colour'], 'marking_colours.npy')), want_c)
    used = json.load(open(os.path.join(par['colour'], 'markings.json')))
    shapes = las_io.marking_summary(want_b, bs, survey)
    tints = las_io.marking_colours(want_b, want_c, bs, survey, colour)
    assert tints == cr.colours_of(want_b, want_c, bs, survey.bin, survey.min_points, survey.max_gap, colour.yellow_share, colour.min_coloured)
    assert used == json.loads(json.dumps({str(k + 1): {**m, **c} for k, (m, c) in enumerate(zip(shapes, tints))})) and len(used) == len(lines)
    assert set(used['1']) == set(shapes[0]) | {'coloured', 'yellow', 'black', 'rgb', 'colour', 'run_colours'}
    alone = json.load(open(os.path.join(par['survey'], 'markings.json')))
    assert alone == json.loads(json.dumps({str(k + 1): m for k, m in enumerate(shapes)})), 'survey= alone writes what it wrote'
    print(f'{len(lines)} lines, {int(bs[-1])} bins, {int((line > 0).sum())} of {len(rec)} records profiled; coloured {int(want_c[:, 0].sum())}, '
          f'yellow {int(want_c[:, 4].sum())}, black {int(want_c[:, 5].sum())}; colours {[c["colour"] for c in tints]}')
    assert want_c[:, 0].sum() > 0 and want_c[:, 5].sum() > 0, 'no coloured or no black return on a line: the test shows nothing'
