"""GPU: the marking profile (csrc/profile.hip: lm_line_profile_points, lm_las_line_profile_records; ops.line_stations / line_profile,
las_io.profile_records / survey_las / marking_summary, Runner `survey=`).

The reference is tests/profile_ref.py: the float32 rule by brute force over all segments on top of label_ref's winner, and an integer
accumulation.  The bins are compared in every int64."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import label_ref as lr
import profile_ref as pr
from guards import Slab, guarded_runs
from lanemapping_amd import io_utils, las_io, ops
from lanemapping_amd._lib import lib
from lanemapping_amd.las_io import MarkingSurvey, PointFilter
from oracle import las_ref

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float('nan')
CHUNK = 1024                                   # points per workgroup of profile_points_kernel (csrc/profile.hip: CHUNK = 256 * PER)
POISON = -7


@functools.lru_cache(maxsize=None)
def _scene():
    """-> (lines, segments, points, index of the first point added by profile_ref): computed once, never changed."""
    lines = [l + lr.SHIFT for l in lr.scene_lines()]
    seg = las_io.line_segments(lines, lr.SHIFT)
    g, _, _ = ops.line_index_host(seg, lr.HW)
    pts, first = pr.scene_points(seg, (g.x0, g.y0, g.cell, g.nx, g.ny))
    seg.setflags(write=False), pts.setflags(write=False)
    return lines, seg, pts, first


@functools.lru_cache(maxsize=None)
def _tables(bin):
    lines = _scene()[0]
    st, bs = las_io.line_stations(lines, lr.SHIFT, bin)
    st.setflags(write=False), bs.setflags(write=False)
    return st, bs


@functools.lru_cache(maxsize=None)
def _ref(bin, min_intensity=None):
    """The brute force on the whole scene: (bins, terms, line, win)."""
    _, seg, pts, _ = _scene()
    st, bs = _tables(bin)
    return pr.profile_f32(pts, seg, st, bs, bin, lr.HW, lr.ZTOL, min_intensity)


def _ref_first(bin, min_intensity, N):
    """The reference bins of the first N points of the scene, from the per-point terms of the one brute-force run."""
    terms = _ref(bin, min_intensity)[1]
    return pr.accumulate({k: v[:N] for k, v in terms.items()}, int(_tables(bin)[1][-1]))


def _t(a):
    return torch.from_numpy(np.array(a, copy=True))              # (the shared scene arrays are read-only)


def _device_tables(dev, bin, seg=None, st=None):
    seg = _scene()[1] if seg is None else seg
    st0, bs = _tables(bin)
    return ops.line_index(seg, lr.HW, device=dev), ops.line_stations(st0 if st is None else st, bs, bin, device=dev)


def _same(tag, got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.int64 and got.shape == want.shape, f'{tag}: {got.dtype} {got.shape}'
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), f'{tag}: {len(bad)} bins differ from the brute force; first bin {bad[0]}: {got[bad[0]].tolist()} != {want[bad[0]].tolist()}'


# ------------------------------------------------------------------------------------------------ 1. exactness
@pytest.mark.parametrize('bin', [pr.BIN_EXACT, pr.BIN_INEXACT])
def test_bins_equal_the_float32_brute_force(dev, bin):
    lines, seg, pts, first = _scene()
    st, bs = _tables(bin)
    bins, terms, line, win = _ref(bin)
    if bin == pr.BIN_EXACT:                                     # the scene holds what it is meant to hold
        pr.check_scene(terms, line, win, first, bs, bin)
    else:
        assert float(f32(bin)) != bin and float(f32(pr.BIN_EXACT)) == pr.BIN_EXACT
    assert set(np.unique(line)) == {0, 1, 2, 3, 4, 5} and (bins[:, 0] > 1).sum() > 50 and (bins[:, 0] == 0).sum() > 50
    bright = _ref(bin, 500.0)
    assert 0 < bright[0][:, 0].sum() < bins[:, 0].sum()
    index, stations = _device_tables(dev, bin)
    assert stations.n_bins == bs[-1] == len(bins) and stations.n_lines == 6 and index.n_lines == 5
    d_pts = _t(pts).to(dev)
    full = len(pts)
    assert full > 2 * CHUNK
    for N in (1, 63, 64, 65, 255, 256, 257, CHUNK + 1, full):
        _same(f'bin={bin}, N={N}', ops.line_profile(d_pts[:N], index, stations, lr.ZTOL), _ref_first(bin, None, N))
        _same(f'bin={bin}, N={N}, min_intensity', ops.line_profile(d_pts[:N], index, stations, lr.ZTOL, min_intensity=500.0),
              _ref_first(bin, 500.0, N))
    _same('full', ops.line_profile(d_pts, index, stations, lr.ZTOL), bins)
    # no points: the empty profile; no segments: no bins
    _same('N=0', ops.line_profile(d_pts[:0], index, stations, lr.ZTOL), pr.accumulate({k: v[:0] for k, v in terms.items()}, len(bins)))
    none_st, none_bs = las_io.line_stations([lr.scene_lines()[5]], None, bin)
    assert none_bs.tolist() == [0, 0] and none_st.shape == (0, 4)
    empty = ops.line_profile(d_pts, ops.line_index(np.zeros((0, 8), f32), lr.HW, device=dev), ops.line_stations(none_st, none_bs, bin, device=dev),
                             lr.ZTOL)
    assert empty.shape == (0, 6) and empty.dtype == torch.int64


def test_tie_goes_to_the_smaller_line_whatever_the_table_order(dev):
    """The point on the vertex that line 1 and line 3 share: with line 3's rows in front of the table only the rule 'ties go to the smaller
    line' puts it into line 1's bin; the wrong rule (ties to the smaller segment index alone) puts it into line 3's."""
    _, seg, pts, _ = _scene()
    st, bs = _tables(pr.BIN_EXACT)
    three = lr.seg_lines(seg) == 3
    perm, perm_st = lr.permuted_table(seg), np.concatenate([st[three], st[~three]])
    want, terms, line, _ = pr.profile_f32(pts, perm, perm_st, bs, pr.BIN_EXACT, lr.HW, lr.ZTOL)
    wrong, wterms, wline, _ = pr.profile_f32(pts, perm, perm_st, bs, pr.BIN_EXACT, lr.HW, lr.ZTOL, line_tie=False)
    c = lr.CROSSING
    assert line[c] == 1 and wline[c] == 3 and terms['B'][c] == 14 * 8 and wterms['B'][c] >= bs[2] and (want != wrong).any()
    assert np.array_equal(want, _ref(pr.BIN_EXACT)[0]), 'the table order changes nothing'
    index = ops.line_index(perm, lr.HW, device=dev)
    stations = ops.line_stations(perm_st, bs, pr.BIN_EXACT, device=dev)
    _same('permuted table', ops.line_profile(_t(pts).to(dev), index, stations, lr.ZTOL), want)


# ------------------------------------------------------------------------------------------------ 2. contention and order
def test_many_lanes_into_few_bins(dev):
    _, seg, pts, _ = _scene()
    st, bs = _tables(pr.BIN_EXACT)
    index, stations = _device_tables(dev, pr.BIN_EXACT)
    # the shared-vertex point 4,096 times: one bin, n = 4096
    many = np.repeat(pts[lr.SHARED_VERTEX:lr.SHARED_VERTEX + 1], 4096, axis=0)
    want = pr.profile_f32(many, seg, st, bs, pr.BIN_EXACT, lr.HW, lr.ZTOL)[0]
    assert want[48].tolist() == [4096, 4096 * 1000, 0, 0, 0, 0] and want[:, 0].sum() == 4096
    _same('4096 x one point', ops.line_profile(_t(many).to(dev), index, stations, lr.ZTOL), want)
    # 64 k points cycling lane by lane over m distinct bins of line 1, with offsets and intensities that differ from lane to lane
    for m, k in ((2, 5), (3, 5), (64, 3)):
        j = np.arange(64 * k)
        x = 0.0625 + 0.125 * (j % m)
        cyc = np.stack([x, 2.0 + ((j * 7) % 19 - 9) / 64.0, 0.01 * x, 100.0 + 37.0 * (j % 11)], axis=1).astype(f32)
        want, terms, line, _ = pr.profile_f32(cyc, seg, st, bs, pr.BIN_EXACT, lr.HW, lr.ZTOL)
        assert (line == 1).all() and np.array_equal(terms['B'], j % m) and len(np.unique(terms['q'])) > 10
        assert (want[:m, 0] == 64 * k // m + (np.arange(m) < 64 * k % m)).all() and want[:, 0].sum() == 64 * k
        _same(f'{64 * k} points over {m} bins', ops.line_profile(_t(cyc).to(dev), index, stations, lr.ZTOL), want)
    # two lanes of a wave alone in their bins beside 62 lanes in one
    mix = cyc[:64].copy()
    mix[:, 0] = 0.0625
    mix[5, 0], mix[40, 0] = 9.0625, 11.0625
    mix[:, 2] = 0.01 * mix[:, 0]
    want = pr.profile_f32(mix, seg, st, bs, pr.BIN_EXACT, lr.HW, lr.ZTOL)[0]
    assert want[0, 0] == 62 and want[72, 0] == 1 and want[88, 0] == 1
    _same('62 + 1 + 1', ops.line_profile(_t(mix).to(dev), index, stations, lr.ZTOL), want)


def test_the_order_of_the_points_changes_no_bit(dev):
    _, seg, pts, _ = _scene()
    want = _ref(pr.BIN_INEXACT, 500.0)[0]
    index, stations = _device_tables(dev, pr.BIN_INEXACT)
    for seed in (1, 2, 3):
        d = _t(pts[np.random.RandomState(seed).permutation(len(pts))]).to(dev)
        for attempt in range(2):
            _same(f'permutation {seed}, run {attempt}', ops.line_profile(d, index, stations, lr.ZTOL, min_intensity=500.0), want)


# ------------------------------------------------------------------------------------------------ 3. accumulate
def test_accumulate_adds_and_a_fresh_call_initialises(dev):
    _, seg, pts, _ = _scene()
    want = _ref(pr.BIN_EXACT)[0]
    index, stations = _device_tables(dev, pr.BIN_EXACT)
    d_pts = _t(pts).to(dev)
    h = len(pts) // 2 + 7
    part = ops.line_profile(d_pts[:h], index, stations, lr.ZTOL)
    _same('first part', part, _ref_first(pr.BIN_EXACT, None, h))
    both = ops.line_profile(d_pts[h:], index, stations, lr.ZTOL, out=part)
    assert both.data_ptr() == part.data_ptr()
    _same('two parts', both, want)
    # accumulate = 0 on a poisoned buffer: as a fresh run
    bins = torch.full((stations.n_bins, 6), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    rc = lib().lm_line_profile_points(_stream(dev), C.c_void_p(d_pts.data_ptr()), len(pts), *index.args(), *stations.args(), lr.ZTOL, NAN, 0,
                                      C.c_void_p(bins.data_ptr()), stations.n_bins)
    assert rc == 0, lib().lm_last_error()
    _same('accumulate=0 on poison', bins, want)
    with pytest.raises(ValueError, match='out must be'):
        ops.line_profile(d_pts, index, stations, lr.ZTOL, out=bins[:-1])
    with pytest.raises(TypeError, match='LineStations'):
        ops.line_profile(d_pts, index, _tables(pr.BIN_EXACT)[0], lr.ZTOL)


# ------------------------------------------------------------------------------------------------ 4. records
SCALE, OFFSET = (0.001, 0.001, 0.001), tuple(lr.SHIFT + [3.0, -2.0, 0.5])
RECORD_LEN = {0: 20, 1: 28, 3: 34, 6: 30, 7: 36}


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _world(n, seed):
    """n points around the scene's lines in the LAS frame, intensities 0..1999."""
    seg = _scene()[1]
    rng = np.random.RandomState(seed)
    s = rng.randint(0, len(seg), n)
    base = seg[s, 0:3].astype(np.float64) + rng.uniform(0, 1, n)[:, None] * seg[s, 3:6].astype(np.float64)
    off = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), rng.uniform(-0.7, 0.7, n)], axis=1)
    return base + off + lr.SHIFT, rng.randint(0, 2000, n)


def _records(tmp_path, fmt, extra, n, seed):
    """-> ([n, rl] records, padded flat copy for the device): written by oracle/las_ref.write_las where it knows the format, by the same
    layout here for format 7.  Classification 2 for four records of five and 7 for the fifth; flag bits from the junk bytes."""
    world, inten = _world(n, seed)
    rl = RECORD_LEN[fmt] + extra
    if fmt in las_ref.RECORD_LEN:
        path = str(tmp_path / f'f{fmt}_{n}.las')
        las_ref.write_las(path, world, inten, point_format=fmt, version=(1, 4) if fmt >= 6 else (1, 2), scale=SCALE, offset=OFFSET,
                          extra_bytes=extra)
        data = np.fromfile(path, np.uint8)
        h = las_io.parse_header(data)
        assert (h['point_format'], h['record_len'], h['n_points']) == (fmt, rl, n)
        rec = data[h['offset_to_points']:h['offset_to_points'] + n * rl].reshape(n, rl).copy()
    else:
        q = np.round((world - np.asarray(OFFSET)) / np.asarray(SCALE)).astype('<i4')
        rec = np.zeros((n, rl), np.uint8)
        rec[:, 0:12] = q.view(np.uint8).reshape(n, 12)
        rec[:, 12:14] = inten.astype('<u2').reshape(n, 1).view(np.uint8)
        rec[:, 14:] = (np.arange(n)[:, None] * 7 + np.arange(rl - 14)[None, :]) % 251
    cls = np.where(np.arange(n) % 5 == 4, 7, 2)
    if fmt >= 6:
        rec[:, 16] = cls
    else:
        rec[:, 15] = (rec[:, 15] & 0xE0) | cls
    flat = np.zeros((n * rl + 3) // 4 * 4, np.uint8)
    flat[:n * rl] = rec.reshape(-1)
    return rec, flat


def _passes(rec, fmt, select):
    if select is None:
        return np.ones(len(rec), bool)
    cls = rec[:, 16] if fmt >= 6 else rec[:, 15] & 31
    withheld = (rec[:, 15] & 4) != 0 if fmt >= 6 else (rec[:, 15] & 128) != 0
    keep = np.isin(cls, np.asarray(select.classes)) if select.classes is not None else np.ones(len(rec), bool)
    assert select.returns == 'all' and select.z_range is None and not (select.drop_synthetic or select.drop_keypoint or select.drop_overlap)
    return keep & ~(withheld & select.drop_withheld)


def _header(fmt, rl, n):
    return {'point_format': fmt, 'record_len': rl, 'n_points': n, 'scale': SCALE, 'offset': OFFSET}


@pytest.mark.parametrize('fmt, extra', [(1, 3), (3, 0), (6, 0), (7, 1)])
def test_records_equal_the_points_entry(dev, tmp_path, fmt, extra):
    _, seg, _, _ = _scene()
    bin = pr.BIN_INEXACT
    st, bs = _tables(bin)
    index, stations = _device_tables(dev, bin)
    rl = RECORD_LEN[fmt] + extra
    assert rl in (31, 34, 30, 37)
    parts = []
    for n in (255, 256, 257):
        rec, flat = _records(tmp_path, fmt, extra, n, seed=100 * fmt + n)
        dec = lr.decode_f32(rec, SCALE, OFFSET, lr.SHIFT)
        d_rec = torch.from_numpy(flat).to(dev)
        parts.append((rec, d_rec, dec, n))
        for name, survey, select in (('plain', MarkingSurvey(bin, lr.HW, lr.ZTOL), None),
                                     ('class 2 only', MarkingSurvey(bin, lr.HW, lr.ZTOL), PointFilter(classes=[2], drop_withheld=False)),
                                     ('no withheld, bright', MarkingSurvey(bin, lr.HW, lr.ZTOL, min_intensity=700), PointFilter())):
            tag = f'format {fmt}, {rl} B, n={n}, {name}'
            ok = _passes(rec, fmt, select)
            want, _, line, _ = pr.profile_f32(dec, seg, st, bs, bin, lr.HW, lr.ZTOL, survey.min_intensity, mask=ok)
            assert (line > 0).sum() > n // 20 and (line == 0).sum() > n // 20, tag
            before = d_rec.clone()
            got = las_io.profile_records(d_rec, _header(fmt, rl, n), index, stations, survey, lr.SHIFT, select)
            _same(tag, got, want)
            assert torch.equal(d_rec, before), f'{tag}: the records were written'
            if select is None:                                  # the points entry on the decode's rows
                d_dec = las_io.decode_points(d_rec, rl, n, SCALE, OFFSET, lr.SHIFT, normalise=False)
                assert np.array_equal(d_dec.cpu().numpy().view(np.int32), dec.view(np.int32))
                assert torch.equal(got, ops.line_profile(d_dec, index, stations, lr.ZTOL)), f'{tag}: the two entries differ'
            else:                                               # a dropped record on a line is not counted
                unfiltered = pr.profile_f32(dec, seg, st, bs, bin, lr.HW, lr.ZTOL, survey.min_intensity)[0]
                assert unfiltered[:, 0].sum() > want[:, 0].sum(), tag
    # the three files into one profile
    survey = MarkingSurvey(bin, lr.HW, lr.ZTOL)
    bins, want = None, None
    for rec, d_rec, dec, n in parts:
        bins = las_io.profile_records(d_rec, _header(fmt, rl, n), index, stations, survey, lr.SHIFT, out=bins)
        want = pr.profile_f32(dec, seg, st, bs, bin, lr.HW, lr.ZTOL, bins=want)[0]
    _same(f'format {fmt}: three files into one profile', bins, want)
    assert want[:, 0].sum() > 100


# ------------------------------------------------------------------------------------------------ 5. guarded buffers
def _table_slabs(dev, seg, start, segs, st, bs, poisoned):
    s_seg = Slab(dev, len(seg), 8, front=4, back=4).fill_input(_t(seg), NAN if poisoned else 0.0)
    s_start = Slab(dev, 1, len(start), front=1, back=1, dtype=torch.int32).fill_input(torch.from_numpy(start), 0x7FFFFFF0 if poisoned else 0)
    s_segs = Slab(dev, 1, len(segs), front=1, back=1, dtype=torch.int32).fill_input(torch.from_numpy(segs), 0x7FFFFFF0 if poisoned else 0)
    s_st = Slab(dev, len(st), 4, front=8, back=8).fill_input(_t(st), NAN if poisoned else 0.0)
    s_bs = Slab(dev, 1, len(bs), front=1, back=1, dtype=torch.int32).fill_input(_t(bs), 0x7FFFFFF0 if poisoned else 0)
    return s_seg, s_start, s_segs, s_st, s_bs


def _bins_of(slab_view):
    return np.ascontiguousarray(slab_view.numpy()).view(np.int64)


def test_profile_points_guards(dev):
    """lm_line_profile_points with the points, the segment table, the two lists, the stations, bin_start and bins each between guard slabs,
    N one past a workgroup's share: bins is written only inside [0, n_bins), poisoned guards change no output bit, no input is written."""
    _, seg, pts, _ = _scene()
    bin = pr.BIN_EXACT
    st, bs = _tables(bin)
    N, n_bins = CHUNK + 1, int(bs[-1])
    g, start, segs = ops.line_index_host(seg, lr.HW)
    host = np.array(bs, np.int32)

    def run(B, poisoned):
        s_pts = Slab(dev, N, 4, front=8, back=8).fill_input(_t(pts[:N]), NAN if poisoned else 0.0)
        s_seg, s_start, s_segs, s_st, s_bs = _table_slabs(dev, seg, start, segs, st, bs, poisoned)
        s_bins = Slab(dev, n_bins, 12, front=8, back=8, dtype=torch.int32).fill_canary()
        ins = (s_pts, s_seg, s_start, s_segs, s_st, s_bs)
        before = [s.bits().clone() for s in ins]
        rc = lib().lm_line_profile_points(_stream(dev), C.c_void_p(s_pts.ptr()), N, C.c_void_p(s_seg.ptr()), len(seg), C.byref(g),
                                          C.c_void_p(s_start.ptr()), C.c_void_p(s_segs.ptr()), lr.HW, C.c_void_p(s_st.ptr()),
                                          C.c_void_p(s_bs.ptr()), C.c_void_p(host.ctypes.data), len(bs) - 1, bin, lr.ZTOL, NAN, 0,
                                          C.c_void_p(s_bins.ptr()), n_bins)
        assert rc == 0, lib().lm_last_error()
        torch.cuda.synchronize()
        for s, b in zip(ins, before):
            assert torch.equal(s.bits(), b), 'an input was written'
        return {'bins': (s_bins, n_bins)}

    got = guarded_runs(run, 'line_profile_points', batch=False)
    _same('guarded', _bins_of(got['bins']), _ref_first(bin, None, N))


def test_profile_records_guards(dev, tmp_path):
    """lm_las_line_profile_records with the records, the tables and bins between guard slabs: 257 records of 37 bytes (the last dword of
    the records is padding, the last block holds one record), with a select."""
    _, seg, _, _ = _scene()
    bin = pr.BIN_EXACT
    st, bs = _tables(bin)
    fmt, extra, n = 7, 1, 257
    rl = RECORD_LEN[fmt] + extra
    rec, flat = _records(tmp_path, fmt, extra, n, seed=7)
    g, start, segs = ops.line_index_host(seg, lr.HW)
    n_bins, host = int(bs[-1]), np.array(bs, np.int32)
    sel = PointFilter(classes=[2], drop_withheld=False)
    want = pr.profile_f32(lr.decode_f32(rec, SCALE, OFFSET, lr.SHIFT), seg, st, bs, bin, lr.HW, lr.ZTOL, mask=_passes(rec, fmt, sel))[0]
    assert want[:, 0].sum() > 10
    d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])
    sst = sel.as_struct()

    def run(B, poisoned):
        s_rec = Slab(dev, 1, len(flat), front=1, back=1, dtype=torch.uint8).fill_input(torch.from_numpy(flat), 0xFF if poisoned else 0)
        s_seg, s_start, s_segs, s_st, s_bs = _table_slabs(dev, seg, start, segs, st, bs, poisoned)
        s_bins = Slab(dev, n_bins, 12, front=8, back=8, dtype=torch.int32).fill_canary()
        ins = (s_rec, s_seg, s_start, s_segs, s_st, s_bs)
        before = [s.bits().clone() for s in ins]
        rc = lib().lm_las_line_profile_records(_stream(dev), C.c_void_p(s_rec.ptr()), rl, fmt, n, d3(SCALE), d3(OFFSET), d3(lr.SHIFT),
                                               C.byref(sst), C.c_void_p(s_seg.ptr()), len(seg), C.byref(g), C.c_void_p(s_start.ptr()),
                                               C.c_void_p(s_segs.ptr()), lr.HW, C.c_void_p(s_st.ptr()), C.c_void_p(s_bs.ptr()),
                                               C.c_void_p(host.ctypes.data), len(bs) - 1, bin, lr.ZTOL, NAN, 0, C.c_void_p(s_bins.ptr()), n_bins)
        assert rc == 0, lib().lm_last_error()
        torch.cuda.synchronize()
        for s, b in zip(ins, before):
            assert torch.equal(s.bits(), b), 'an input was written'
        return {'bins': (s_bins, n_bins)}

    for attempt in range(2):                                             # the second round: the same bits again
        got = guarded_runs(run, 'las_line_profile_records', batch=False)
        _same('guarded', _bins_of(got['bins']), want)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_the_argument_and_write_nothing(dev, tmp_path):
    _, seg, pts, _ = _scene()
    bin = pr.BIN_EXACT
    st, bs = _tables(bin)
    index, stations = _device_tables(dev, bin)
    n_bins, n = stations.n_bins, 300
    rec, flat = _records(tmp_path, 1, 0, n, seed=1)
    d_rec = torch.from_numpy(flat).to(dev)
    d_pts = _t(pts[:n + 1]).to(dev)
    bins = torch.full((n_bins + 1, 6), POISON, dtype=torch.int64, device=dev)
    L = lib()
    d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])
    # positions: points 1, N 2, segments 3, grid 5, cell_start 6, cell_segs 7, half_width 8, stations 9, bin_start 10, bin_start_host 11,
    # L 12, bin 13, z_tol 14, accumulate 16, bins 17, n_bins 18; the record entry: the same from segments on, six further back
    p_base = [_stream(dev), C.c_void_p(d_pts.data_ptr()), n, *index.args(), *stations.args(), lr.ZTOL, NAN, 0, C.c_void_p(bins.data_ptr()), n_bins]
    r_base = [_stream(dev), C.c_void_p(d_rec.data_ptr()), 28, 1, n, d3(SCALE), d3(OFFSET), d3(lr.SHIFT), None, *index.args(), *stations.args(),
              lr.ZTOL, NAN, 0, C.c_void_p(bins.data_ptr()), n_bins]
    assert len(p_base) == 19 and len(r_base) == 25
    assert L.lm_line_profile_points(*p_base) == 0 and L.lm_las_line_profile_records(*r_base) == 0, L.lm_last_error()
    torch.cuda.synchronize()
    bins.fill_(POISON)

    def refused(what, **change):
        """`change`: position in the points entry -> new value; applied to both entries (the record entry: position + 6 from 3 on)."""
        for name, fn, base, shift in (('line_profile_points', L.lm_line_profile_points, p_base, 0),
                                      ('las_line_profile_records', L.lm_las_line_profile_records, r_base, 6)):
            a = list(base)
            for pos, v in change.items():
                a[int(pos[1:]) + shift] = v
            rc = fn(*a)
            torch.cuda.synchronize()
            msg = L.lm_last_error().decode()
            assert rc == 1 and msg.startswith(name + ':') and what in msg, f'{name}, {what}: rc={rc}, message {msg!r}'
            assert bool((bins == POISON).all()), f'{name}, {what}: bins was written'

    off = lambda pos, by: {f'p{pos}': C.c_void_p(p_base[pos].value + by)}
    # misaligned buffers, each named alone
    for pos, what, by in ((3, 'segments', 8), (6, 'cell_start', 1), (7, 'cell_segs', 2), (9, 'stations', 4), (10, 'bin_start', 2), (17, 'bins', 4)):
        refused(f'{what} is not', **off(pos, by))
    # null pointers
    refused('stations', p9=None)
    refused('bin_start', p10=None)
    refused('bin_start_host', p11=None)
    refused('bins', p17=None)
    refused('segments', p3=None)
    # n_bins != bin_start[L]
    refused('n_bins', p18=n_bins + 1)
    refused('n_bins', p18=n_bins - 1)
    # lines outside 1 .. L: the segments carry line 5
    short = np.array(bs[:5], np.int32)
    refused('segments carry lines', p11=C.c_void_p(short.ctypes.data), p12=4, p18=int(short[-1]))
    # a bin_start that descends or does not start at 0
    down = np.array(bs, np.int32)
    down[2] = down[1] - 1
    refused('bin_start[2]', p11=C.c_void_p(down.ctypes.data))
    late = np.array(bs, np.int32)
    late[0] = 1
    refused('bin_start[0]', p11=C.c_void_p(late.ctypes.data))
    # a grid built for another half_width or table; half_width above 16 m; bin <= 0; accumulate; NaN z_tol
    wide = ops.line_index(seg, 0.25, device=dev)
    refused('half_width', p5=C.byref(wide.grid))
    other = ops.line_index(seg[:-1], lr.HW, device=dev)
    refused('grid', p5=C.byref(other.grid))
    huge = ops.line_index(seg, 16.5, device=dev)
    ha = huge.args()
    refused('half_width=16.5', p3=ha[0], p5=ha[2], p6=ha[3], p7=ha[4], p8=16.5)
    for bad in (0.0, -0.125, NAN, float('inf')):
        refused('bin=', p13=bad)
    refused('accumulate', p16=2)
    refused('z_tol', p14=NAN)
    refused('half_width', p8=-1.0)
    # what only one entry takes
    for pos, v, what in ((1, C.c_void_p(d_pts.data_ptr() + 4), 'points_xyzi is not'), (1, None, 'points_xyzi'), (2, -1, 'N=')):
        a = list(p_base)
        a[pos] = v
        assert L.lm_line_profile_points(*a) == 1 and what in L.lm_last_error().decode(), (what, L.lm_last_error())
    for pos, v, what in ((1, C.c_void_p(d_rec.data_ptr() + 1), 'records is not'), (1, None, 'records'), (2, 27, 'record_len'), (3, 11, 'point_format'),
                         (4, -1, 'n='), (5, None, 'scale')):
        a = list(r_base)
        a[pos] = v
        assert L.lm_las_line_profile_records(*a) == 1 and what in L.lm_last_error().decode(), (what, L.lm_last_error())
    torch.cuda.synchronize()
    assert bool((bins == POISON).all())
    # the package entries
    with pytest.raises(ValueError, match='half_width'):
        las_io.profile_records(d_rec, _header(1, 28, n), wide, stations, MarkingSurvey(bin, lr.HW, lr.ZTOL), lr.SHIFT)
    with pytest.raises(ValueError, match='bin='):
        las_io.profile_records(d_rec, _header(1, 28, n), index, stations, MarkingSurvey(0.5, lr.HW, lr.ZTOL), lr.SHIFT)
    with pytest.raises(TypeError, match='MarkingSurvey'):
        las_io.profile_records(d_rec, _header(1, 28, n), index, stations, las_io.MarkingLabels(), lr.SHIFT)


# ------------------------------------------------------------------------------------------------ 7. a painted patch
def test_survey_las_reads_the_dash_pattern_off_a_painted_patch(dev, tmp_path):
    """A line from (0, 2, 0) to (24, 2, 0) with a vertex every 2 m over returns at x = 0.025 + 0.05 i, y = 0.025 + 0.05 j (24 m x 4 m),
    painted (intensity 24000, else 3000) where floor(x / 3) is even and |y - 2| < 0.075: the two rows y = 1.975 and 2.025, told by their
    whole index (|2 j + 1 - 80| < 3) so that no rounding of 0.05 j decides.  No return lies within 0.02 m of a bin border of 0.25 m, so
    float32 changes no bin and the summary is exact.  The cloud is split over two files."""
    i, j = np.meshgrid(np.arange(480), np.arange(80), indexing='ij')
    i, j = i.ravel(), j.ravel()
    x, y = (2 * i + 1) * 0.025, (2 * j + 1) * 0.025
    paint = ((i // 60) % 2 == 0) & (np.abs(2 * j + 1 - 80) < 3)
    assert paint.sum() == 4 * 60 * 2
    inten = np.where(paint, 24000, 3000)
    world = np.stack([x, y, np.zeros_like(x)], axis=1) + lr.SHIFT
    order = np.random.RandomState(11).permutation(len(world))
    half = len(order) // 2
    paths = []
    for k, part in enumerate((order[:half], order[half:])):
        paths.append(str(tmp_path / f'patch{k}.las'))
        las_ref.write_las(paths[k], world[part], inten[part], point_format=(1, 6)[k], version=((1, 2), (1, 4))[k], offset=tuple(lr.SHIFT))
    xs = np.arange(0.0, 26.0, 2.0)
    line = np.stack([xs, np.full_like(xs, 2.0), np.zeros_like(xs)], axis=1) + lr.SHIFT
    survey = MarkingSurvey(bin=0.25, min_intensity=10000)
    # the reference's own numbers first
    seg = las_io.line_segments([line], lr.SHIFT)
    st, bs = las_io.line_stations([line], lr.SHIFT, survey.bin)
    assert bs.tolist() == [0, 96]
    dec = np.concatenate([(world - lr.SHIFT), inten[:, None]], axis=1).astype(f32)
    want, terms, lab, _ = pr.profile_f32_pruned(dec, seg, st, bs, survey.bin, survey.half_width, survey.z_tol, survey.min_intensity)
    frac = (x / 0.25) % 1.0
    assert (np.minimum(frac, 1 - frac) * 0.25 > 0.02).all() and (lab > 0).sum() == paint.sum()
    on = (np.arange(96) // 12) % 2 == 0
    assert (want[on, 0] == 10).all() and (want[~on, 0] == 0).all() and (want[on, 4] == -26).all() and (want[on, 5] == 26).all()
    assert (want[on, 1] == 240000).all() and (want[on, 2] == 0).all() and (want[on, 3] == 10 * 26 * 26).all()
    bins, bin_start = las_io.survey_las(paths, [line], survey, lr.SHIFT, device=dev)
    assert bin_start.tolist() == [0, 96]
    _same('survey_las', bins, want)
    got = las_io.marking_summary(bins, bin_start, survey)
    assert got == pr.summary_of(want, bs, survey) and len(got) == 1
    m = got[0]
    assert m['runs'] == [[0.0, 3.0], [6.0, 9.0], [12.0, 15.0], [18.0, 21.0]] and m['type'] == 'dashed' and m['width'] == 52 / 1024
    assert m['dash'] == 3.0 and m['gap'] == 3.0 and m['cover'] == 0.5 and m['intensity'] == 24000.0 and m['length'] == 24.0 and m['painted'] == 48
    # without the threshold a bin counts returns, not paint: every bin is 'painted', the width is the band's
    loose = MarkingSurvey(bin=0.25)
    b2, _ = las_io.survey_las(paths, [line], loose, lr.SHIFT, device=dev)
    m2 = las_io.marking_summary(b2, bin_start, loose)[0]
    assert m2['type'] == 'solid' and m2['runs'] == [[0.0, 24.0]] and m2['width'] > 0.5
    _same('no threshold', b2, pr.profile_f32_pruned(dec, seg, st, bs, 0.25, loose.half_width, loose.z_tol)[0])
    # with a select (the junk bytes of the writer give every record a class): only the records that pass are counted
    sel = PointFilter(classes=[3, 5, 7], drop_withheld=False)
    b3, _ = las_io.survey_las(paths, [line], survey, lr.SHIFT, select=sel, device=dev)
    want3 = None
    for path in paths:
        data = np.fromfile(path, np.uint8)
        h = las_io.parse_header(data)
        o, rl, n = h['offset_to_points'], h['record_len'], h['n_points']
        rec = data[o:o + n * rl].reshape(n, rl)
        terms3 = pr.profile_f32_pruned(lr.decode_f32(rec, h['scale'], h['offset'], lr.SHIFT), seg, st, bs, survey.bin, survey.half_width,
                                       survey.z_tol, survey.min_intensity, mask=_passes(rec, h['point_format'], sel))[1]
        want3 = pr.accumulate(terms3, 96, bins=want3)
    assert 0 < want3[:, 0].sum() < want[:, 0].sum()
    _same('with a select', b3, want3)


# ------------------------------------------------------------------------------------------------ 8. Runner
def _strip(tmp_path):
    """The strip of tests/test_gpu_label.py's Runner test (a copy of its generator): three overlapping 1152 x 1152 tiles over a climbing
    plane, one point at every pixel centre, six painted stripes.  -> (las path, parameter file paths, read offset)."""
    H = W = 1152
    reso, ele, A, Bs = 0.05, 0.05, 0.075, 0.02
    off = np.array([351200.0, 3433000.0, 12.0])
    step = 1024
    rows = 2 * step + H
    r, c = np.meshgrid(np.arange(rows), np.arange(W), indexing='ij')
    x, y = (r * reso).ravel(), (c * reso).ravel()
    lane_y = [(0.12 + 0.152 * l) * 57.6 + 0.01 * (l - 2.5) * x for l in range(6)]
    paint = np.zeros(len(x), bool)
    for ly in lane_y:
        paint |= np.abs(y - ly) < 0.075
    inten = np.where(paint, 24000.0, 3000.0 + 40.0 * ((r + 3 * c) % 97).ravel())
    world = np.stack([x, y, A * x + Bs * y], axis=1)
    order = np.random.RandomState(3).permutation(len(world))
    las = str(tmp_path / 'strip.las')
    las_ref.write_las(las, world[order] + off, inten[order], point_format=1, offset=tuple(off))
    prm_paths = []
    for t in range(3):
        p = {'coor_las_path': '', 'las_read_offset': list(off), 'las_rotation_trans_quan': [t * step * reso, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0],
             'bev_img_offset': [0.0, 0.0], 'img_reso': [reso, reso], 'local_min_ele': -0.5, 'ele_reso': ele}
        prm_paths.append(str(tmp_path / f'18102{t}_0209.txt'))
        io_utils.save_pc_2_img_transform_paras(prm_paths[t], p)
    return las, prm_paths, off


def test_runner_strip_surveys_its_lines(dev, net, tmp_path):
    """Runner.infer_las_strip_to_map with survey=MarkingSurvey(min_intensity=10000): params/markings.npy equals the brute force against
    the lines the call returned, params/markings.json is marking_summary of it; the return value and merged.txt equal the plain call's,
    which writes neither file."""
    from lanemapping_amd.runner import Runner
    las, prm_paths, off = _strip(tmp_path)
    rn = Runner.__new__(Runner)
    rn.cfg, rn.device, rn.net = net.cfg, dev, net
    assert rn.cfg.get('las_survey') is None
    out = {k: str(tmp_path / k) for k in ('plain', 'survey')}
    plain = rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['plain'], batch_size=2)
    survey = MarkingSurvey(min_intensity=10000.0)
    lines3d, merged = rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['survey'], batch_size=2, survey=survey)
    assert sorted(plain[0]) == sorted(lines3d) and len(plain[1]) == len(merged) and all(np.array_equal(a, b) for a, b in zip(plain[1], merged))
    for name in ('markings.json', 'markings.npy'):
        assert not os.path.exists(os.path.join(out['plain'], 'params', name)) and os.path.exists(os.path.join(out['survey'], 'params', name))
    pc = os.path.join('out_pc_seq_json_dir', 'merged.txt')
    assert open(os.path.join(out['plain'], pc), 'rb').read() == open(os.path.join(out['survey'], pc), 'rb').read()
    lines = list(merged) if len(merged) else [l for name in sorted(lines3d) for l in lines3d[name]]
    assert lines, 'the strip yielded no lines'
    data = np.fromfile(las, np.uint8)
    h = las_io.parse_header(data)
    o, rl, n = h['offset_to_points'], h['record_len'], h['n_points']
    rec = data[o:o + n * rl].reshape(n, rl)
    seg = las_io.line_segments(lines, off)
    st, bs = las_io.line_stations(lines, off, survey.bin)
    want, _, line, _ = pr.profile_f32_pruned(lr.decode_f32(rec, h['scale'], h['offset'], off), seg, st, bs, survey.bin, survey.half_width,
                                             survey.z_tol, survey.min_intensity)
    got = np.load(os.path.join(out['survey'], 'params', 'markings.npy'))
    _same('markings.npy', got, want)
    used = json.load(open(os.path.join(out['survey'], 'params', 'markings.json')))
    summary = las_io.marking_summary(want, bs, survey)
    assert used == json.loads(json.dumps({str(k + 1): m for k, m in enumerate(summary)})) and len(used) == len(lines)
    assert summary == pr.summary_of(want, bs, survey)
    painted = sum(m['painted'] for m in summary)
    print(f'{len(lines)} lines, {len(seg)} segments, {int(bs[-1])} bins, {painted} painted, {int((line > 0).sum())} of {n} records profiled; '
          f'types {[m["type"] for m in summary]}')
    assert painted > 0, 'no bin is painted: the test shows nothing'
