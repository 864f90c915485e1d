"""GPU: the paint / asphalt histograms (csrc/profile.hip: lm_line_hist_points, lm_las_line_hist_records; ops.line_hist,
las_io.hist_records / hist_files / paint_threshold, Runner `threshold=` and 'auto').

The reference is tests/threshold_ref.py: the float32 rule by brute force over all segments on top of label_ref's winner and profile_ref's
q and iq, an integer accumulation, and the policy in Python integers.  The table is compared in every int64.

The two entries take their stream LAST (include/lanemap_hip.h says why), so the harnesses that find entries by their first parameter -
lds_state.poisoned, stream_state.stream_runs - do not see them.  Their cases are here: guarded buffers (4), poisoned LDS before the
record kernel (6), a side stream and graph replay (7)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import label_ref as lr
import lds_state
import test_gpu_cross as tc
import threshold_ref as tr
from guards import Slab, guarded_runs
from lanemapping_amd import las_io, ops
from lanemapping_amd._lib import lib
from lanemapping_amd.las_io import CrossSection, MarkingSurvey, PaintResidue, PaintThreshold, PointFilter

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float('nan')
CHUNK = 1024                                   # points per workgroup of hist_points_kernel (csrc/profile.hip: CHUNK = 256 * PER)
POISON = -7
HW, ZTOL, RQ, SH = tc.HW, tc.ZTOL, 32, 6       # half_width 0.3125: hq = 320; rings of 32/1024 m: Z = 11; bins of 64: NB = 1024
L = 3                                          # the scene's lines; line 3 has one vertex and no segment
EXTRA = {'ring_edge': 0, 'ring_below': 1, 'ring_right': 2, 'bin_edge': 3, 'bin_below': 4, 'brightest': 5, 'beyond': 6}
PARAMS = [(32, 6), (1, 8), (1000, 0)]


@functools.lru_cache(maxsize=None)
def _scene():
    """test_gpu_cross's scene (20 010 points, 7 segments, 3 lines; its special points hold |q| = hq, a NaN intensity, NaN x, y, z) with
    the histogram's own special points in front, all beside the first segment of line 1 (y = 2, along +x): -> (lines, segments, points,
    stations)."""
    lines, seg, pts = tc._scene()
    z = 0.015625
    X = [(1.5, 2.0 + 32.0 / 1024, z, 1000.0),            # |q| = 32 = ring_q: the first return of ring 1
         (1.5, 2.0 + 31.0 / 1024, z, 1000.0),            # |q| = 31: the last of ring 0
         (1.5, 2.0 - 64.0 / 1024, z, 1000.0),            # q = -64: ring 2 from the right
         (1.5, 2.01, z, 6400.0), (1.5, 2.01, z, 6399.0),  # iq on a bin edge of 64 and of 256, and one below it
         (1.5, 2.01, z, 65535.0), (1.5, 2.01, z, 70000.0)]   # iq = 65535, and an intensity clamped to it
    pts = np.concatenate([np.asarray(X, f32), pts])
    st, _ = las_io.line_stations(lines, None, las_io.HIST_BIN)
    pts.setflags(write=False), st.setflags(write=False)
    return lines, seg, pts, st


@functools.lru_cache(maxsize=None)
def _winner(half_width):
    _, seg, pts, _ = _scene()
    line, _, win = lr.label_f32(pts, seg, half_width, ZTOL)
    return line, win


@functools.lru_cache(maxsize=None)
def _ref(half_width=HW, ring_q=RQ, bin_shift=SH, N=None):
    """The brute force on the first N points of the scene: -> (hist [L, Z, NB], terms).  Computed once per parameter set, never changed."""
    _, seg, pts, st = _scene()
    line, win = _winner(half_width)
    N = len(pts) if N is None else N
    terms = tr.hist_terms(pts[:N], seg, st, half_width, ring_q, bin_shift, line[:N], win[:N])
    _, Z, NB = tr.shape(half_width, ring_q, bin_shift)
    hist = tr.accumulate(terms, L, Z, NB)
    hist.setflags(write=False)
    return hist, terms


def _t(a):
    return torch.from_numpy(np.array(a, copy=True))              # (the shared scene arrays are read-only)


def _device_tables(dev, half_width=HW):
    lines, seg, _, st = _scene()
    bs = las_io.line_stations(lines, None, las_io.HIST_BIN)[1]
    return ops.line_index(seg, half_width, device=dev), ops.line_stations(st, bs, las_io.HIST_BIN, device=dev)


def _same(tag, got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.int64 and got.shape == want.shape, f'{tag}: {got.dtype} {got.shape}, expected {want.shape}'
    bad = np.argwhere(got != want)
    assert not len(bad), (f'{tag}: {len(bad)} counts differ from the brute force; first [line, ring, bin] = {bad[0].tolist()}: '
                          f'{int(got[tuple(bad[0])])} != {int(want[tuple(bad[0])])}')


def _handle(stream):
    return C.c_void_p(stream.cuda_stream)


def _points_call(d_pts, N, index, stations, ring_q, bin_shift, accumulate, hist, stream, z_tol=ZTOL):
    """lm_line_hist_points through the library object, the stream handle given explicitly."""
    n_hist = hist.numel()
    rc = lib().lm_line_hist_points(C.c_void_p(d_pts.data_ptr()) if N else None, N, *index.args(), stations.args()[0], stations.n_lines, z_tol,
                                   ring_q, bin_shift, accumulate, C.c_void_p(hist.data_ptr()) if n_hist else None, n_hist, _handle(stream))
    assert rc == 0, lib().lm_last_error()


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def _records_call(d_rec, rl, fmt, n, sel, index, stations, ring_q, bin_shift, accumulate, hist, stream):
    n_hist = hist.numel()
    rc = lib().lm_las_line_hist_records(C.c_void_p(d_rec.data_ptr()), rl, fmt, n, _d3(tc.SCALE), _d3(tc.OFFSET), None,
                                        C.byref(sel) if sel is not None else None, *index.args(), stations.args()[0], stations.n_lines, ZTOL,
                                        ring_q, bin_shift, accumulate, C.c_void_p(hist.data_ptr()) if n_hist else None, n_hist, _handle(stream))
    assert rc == 0, lib().lm_last_error()


def _fill_if_poisoned():
    """Inside lds_state.poisoned() (guarded_runs opens it): the fill its wrapper enqueues before an entry it finds, counted like one - for
    the two entries it cannot find.  The last thing on the stream before the entry."""
    state = lds_state._ACTIVE
    if state is not None:
        lds_state.fill(state.word)
        state.fills += 1


# ------------------------------------------------------------------------------------------------ 1. exactness
def test_the_scene_holds_what_it_is_meant_to_hold():
    """No GPU work: the reference puts the special points where the rule says, so the comparisons below mean what they claim."""
    _, seg, pts, st = _scene()
    hist, terms = _ref()
    line, win = _winner(HW)
    hq, Z, NB = tr.shape(HW, RQ, SH)
    assert (hq, Z, NB) == (320, 11, 1024) and hist.shape == (3, 11, 1024) and len(seg) == 7 and len(pts) == 20017
    E, n = EXTRA, len(EXTRA)
    assert all(line[i] == 1 for i in range(n))
    assert (terms['q'][E['ring_edge']], terms['r'][E['ring_edge']]) == (32, 1) and (terms['q'][E['ring_below']], terms['r'][E['ring_below']]) == (31, 0)
    assert (terms['q'][E['ring_right']], terms['r'][E['ring_right']]) == (-64, 2)
    assert (terms['iq'][E['bin_edge']], terms['ib'][E['bin_edge']]) == (6400, 100) and (terms['iq'][E['bin_below']], terms['ib'][E['bin_below']]) == (6399, 99)
    assert terms['iq'][E['brightest']] == terms['iq'][E['beyond']] == 65535 and terms['ib'][E['beyond']] == NB - 1
    S = tc.SPECIAL
    assert line[n + S['left_edge']] == 1 and terms['q'][n + S['left_edge']] == hq and terms['r'][n + S['left_edge']] == Z - 1, '|q| = hq: the last ring'
    assert line[n + S['right_edge']] == 1 and terms['q'][n + S['right_edge']] == -hq and terms['r'][n + S['right_edge']] == Z - 1
    assert line[n + S['nan_i']] == 1 and terms['iq'][n + S['nan_i']] == 0 and all(line[n + S[k]] == 0 for k in ('nan_x', 'nan_y', 'nan_z'))
    assert line[n + S['tie']] == 1, 'an exact tie between lines 1 and 2 goes to line 1'
    assert set(np.unique(line)) == {0, 1, 2} and (line == 0).sum() > 2000 and (line > 0).sum() > 6000
    assert hist.sum() == (line > 0).sum() and not hist[2].any() and (hist > 1).sum() > 300
    per_ring = hist.sum(axis=2)                                            # every ring of both lines is used; the last holds |q| = hq alone
    assert (per_ring[:2, :Z - 1] > 100).all() and per_ring[0, Z - 1] >= 2
    # 6400 = 25 x 256 is an edge of the bins of 256 as well, and with bin_shift 0 a bin is one intensity
    wide, fine = _ref(HW, 1, 8)[1]['ib'], _ref(HW, 1000, 0)[1]['ib']
    assert (wide[E['bin_below']], wide[E['bin_edge']]) == (24, 25) and (fine[E['bin_below']], fine[E['bin_edge']]) == (6399, 6400)
    assert _ref(HW, 1000, 0)[0].shape == (3, 1, 65536)
    assert _ref(HW, 1, 8)[0].shape == (3, 321, 256) and _ref(0.03, 1, 8)[0].shape == (3, 32, 256) and _ref(0.03, 1, 8)[0].sum() > 300


@pytest.mark.parametrize('half_width', [HW, 0.03])
@pytest.mark.parametrize('ring_q, bin_shift', PARAMS)
def test_table_equals_the_float32_brute_force(dev, half_width, ring_q, bin_shift):
    _, seg, pts, st = _scene()
    index, stations = _device_tables(dev, half_width)
    d_pts = _t(pts).to(dev)
    want = _ref(half_width, ring_q, bin_shift)[0]
    assert len(pts) > 2 * CHUNK and ops.hist_shape(half_width, ring_q, bin_shift) == tr.shape(half_width, ring_q, bin_shift)
    got = ops.line_hist(d_pts, index, stations, ZTOL, ring_q, bin_shift)
    assert tuple(got.shape) == want.shape and got.dtype == torch.int64
    _same(f'half_width={half_width}, ring_q={ring_q}, bin_shift={bin_shift}', got, want)
    if ring_q == 1000:
        assert want.shape[1] == 1, 'ring_q > hq: one ring'


@pytest.mark.parametrize('N', [0, 1, 63, 64, 65, 1024, 1025])
def test_sizes(dev, N):
    _, seg, pts, st = _scene()
    index, stations = _device_tables(dev)
    want = _ref(N=N)[0]
    _same(f'N={N}', ops.line_hist(_t(pts[:N]).to(dev), index, stations, ZTOL, RQ, SH), want)
    assert want.sum() == (_winner(HW)[0][:N] > 0).sum() and (N < 2 or want.sum() > 0)


def test_no_segments(dev):
    """S = 0: a line with one vertex alone - L = 1, an all-zero table after the initialisation."""
    _, _, pts, _ = _scene()
    none_st, none_bs = las_io.line_stations([tc._lines()[2]], None, las_io.HIST_BIN)
    index = ops.line_index(np.zeros((0, 8), f32), HW, device=dev)
    stations = ops.line_stations(none_st, none_bs, las_io.HIST_BIN, device=dev)
    hist = torch.full((1, 11, 1024), POISON, dtype=torch.int64, device=dev)
    _points_call(_t(pts).to(dev), len(pts), index, stations, RQ, SH, 0, hist, torch.cuda.current_stream(dev))
    assert not bool(hist.any())
    assert tuple(ops.line_hist(_t(pts).to(dev), index, stations, ZTOL, RQ, SH).shape) == (1, 11, 1024)


# ------------------------------------------------------------------------------------------------ 2. accumulation and order
def test_accumulate_and_order(dev):
    _, seg, pts, st = _scene()
    want = _ref()[0]
    index, stations = _device_tables(dev)
    d_pts = _t(pts).to(dev)
    cur = torch.cuda.current_stream(dev)
    hist = torch.full(want.shape, 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    _points_call(d_pts, len(pts), index, stations, RQ, SH, 0, hist, cur)
    _same('accumulate=0 on poison', hist, want)
    _points_call(d_pts, len(pts), index, stations, RQ, SH, 1, hist, cur)
    _same('accumulate=1 adds', hist, 2 * want)
    h = len(pts) // 2 + 7
    part = ops.line_hist(d_pts[:h], index, stations, ZTOL, RQ, SH)
    _same('first part', part, _ref(N=h)[0])
    both = ops.line_hist(d_pts[h:], index, stations, ZTOL, RQ, SH, out=part)
    assert both.data_ptr() == part.data_ptr()
    _same('two halves', both, want)
    for seed in (1, 2):                                                    # a permutation of the points changes no bit
        d = _t(pts[np.random.RandomState(seed).permutation(len(pts))]).to(dev)
        for attempt in range(2):
            _same(f'permutation {seed}, run {attempt}', ops.line_hist(d, index, stations, ZTOL, RQ, SH), want)
    with pytest.raises(ValueError, match='out must be'):
        ops.line_hist(d_pts, index, stations, ZTOL, RQ, SH, out=hist[:-1])
    with pytest.raises(TypeError, match='LineStations'):
        ops.line_hist(d_pts, index, st, ZTOL, RQ, SH)
    with pytest.raises(ValueError, match='ring_q'):
        ops.line_hist(d_pts, index, stations, ZTOL, 0, SH)
    with pytest.raises(ValueError, match='bin_shift'):
        ops.line_hist(d_pts, index, stations, ZTOL, RQ, 9)


def test_accumulation_corners(dev):
    """The corners of the accumulation, whichever form it takes: every lane of every wave in one cell (4096 adds to one count); no two
    lanes of a wave in one cell; the lanes of a wave split between two cells.  Along the last segment of line 1, from (10, 5) to
    (14, 5), far from line 2."""
    _, seg, _, st = _scene()
    index, stations = _device_tables(dev)

    def run(tag, p):
        want, terms, line, _ = tr.hist_f32(p, seg, st, L, HW, ZTOL, 4, 0)
        assert (line == 1).all()
        _same(tag, ops.line_hist(_t(p).to(dev), index, stations, ZTOL, 4, 0), want)
        return want, terms

    one = np.repeat(np.asarray([[12.0, 5.0 + 20.0 / 1024, 0.125, 30000.0]], f32), 4096, axis=0)
    want, _ = run('4096 points in one cell', one)
    assert want.max() == 4096 and (want > 0).sum() == 1
    k = np.arange(4096)
    spread = np.stack([np.full(4096, 12.0), 5.0 + (4 * (k % 64) + 2) / 1024.0, np.full(4096, 0.125), 100.0 + k // 64], axis=1).astype(f32)
    want, terms = run('4096 points in 4096 cells', spread)
    assert len(np.unique(terms['cell'])) == 4096 and want.max() == 1
    two = spread[:64].copy()
    two[:, 3] = np.where(np.arange(64) % 2 == 0, 500.0, 501.0).astype(f32)
    two[:, 1] = f32(5.0 + 2.0 / 1024)
    want, _ = run('64 points in two cells', two)
    assert sorted(want[want > 0].tolist()) == [32, 32]


# ------------------------------------------------------------------------------------------------ 3. records
@pytest.mark.parametrize('fmt, extra', [(0, 0), (1, 3), (3, 0), (6, 0), (7, 1)])
def test_records_equal_the_brute_force_and_the_points_entry(dev, tmp_path, fmt, extra):
    _, seg, _, st = _scene()
    index, stations = _device_tables(dev)
    thr = PaintThreshold(half_width=HW, ring=RQ / 1024, inner=RQ / 1024, outer=0.25, z_tol=ZTOL, bin_shift=SH)
    assert (thr.ring_q, thr.rings, thr.n_counts, thr.hq) == (RQ, 11, 1024, 320)
    rl = tc.RECORD_LEN[fmt] + extra
    assert rl in (20, 31, 34, 30, 37)
    parts = []
    for n in (255, 256, 257):
        rec, flat = tc._records(tmp_path, fmt, extra, n, seed=100 * fmt + n)
        dec = lr.decode_f32(rec, tc.SCALE, tc.OFFSET, tc.ZERO)
        d_rec = torch.from_numpy(flat).to(dev)
        parts.append((d_rec, dec, n))
        for name, select in (('plain', None), ('class 2 only', PointFilter(classes=[2], drop_withheld=False))):
            tag = f'format {fmt}, {rl} B, n={n}, {name}'
            want, _, line, _ = tr.hist_f32(dec, seg, st, L, HW, ZTOL, RQ, SH, mask=tc._passes(rec, fmt, select))
            assert (line > 0).sum() > n // 20 and (line == 0).sum() > n // 20, tag
            before = d_rec.clone()
            got = las_io.hist_records(d_rec, tc._header(fmt, rl, n), index, stations, thr, None, select)
            _same(tag, got, want)
            assert torch.equal(d_rec, before), f'{tag}: the records were written'
            if select is None:                                  # the points entry on the decode's rows
                d_dec = las_io.decode_points(d_rec, rl, n, tc.SCALE, tc.OFFSET, None, normalise=False)
                assert np.array_equal(d_dec.cpu().numpy().view(np.int32), dec.view(np.int32))
                assert torch.equal(got, ops.line_hist(d_dec, index, stations, ZTOL, RQ, SH)), f'{tag}: the two entries differ'
            else:                                               # a dropped record on a line is not counted
                assert tr.hist_f32(dec, seg, st, L, HW, ZTOL, RQ, SH)[0].sum() > want.sum(), tag
    hist, want = None, None                                     # the three files into one table
    for d_rec, dec, n in parts:
        hist = las_io.hist_records(d_rec, tc._header(fmt, rl, n), index, stations, thr, None, out=hist)
        want = tr.hist_f32(dec, seg, st, L, HW, ZTOL, RQ, SH, hist=want)[0]
    _same(f'format {fmt}: three files into one table', hist, want)
    assert want.sum() > 150


# ------------------------------------------------------------------------------------------------ 4. guarded buffers
def _table_slabs(dev, seg, start, segs, st, poisoned):
    s_seg = Slab(dev, len(seg), 8, front=4, back=4).fill_input(_t(seg), NAN if poisoned else 0.0)
    s_start = Slab(dev, 1, len(start), front=1, back=1, dtype=torch.int32).fill_input(torch.from_numpy(start), 0x7FFFFFF0 if poisoned else 0)
    s_segs = Slab(dev, 1, len(segs), front=1, back=1, dtype=torch.int32).fill_input(torch.from_numpy(segs), 0x7FFFFFF0 if poisoned else 0)
    s_st = Slab(dev, len(st), 4, front=8, back=8).fill_input(_t(st), NAN if poisoned else 0.0)
    return s_seg, s_start, s_segs, s_st


def _hist_of(slab_view, shape):
    return np.ascontiguousarray(slab_view.numpy()).view(np.int64).reshape(shape)


def test_hist_points_guards(dev):
    """lm_line_hist_points with the points, the segment table, the two lists, the stations and hist each between guard slabs, N one past
    a workgroup's share: hist is written only inside [0, n_hist), poisoned guards change no output bit, no input is written."""
    _, seg, pts, st = _scene()
    N = CHUNK + 1
    want = _ref(N=N)[0]
    n_hist = want.size
    g, start, segs = ops.line_index_host(seg, HW)
    cur = _handle(torch.cuda.current_stream(dev))

    def run(B, poisoned):
        s_pts = Slab(dev, N, 4, front=8, back=8).fill_input(_t(pts[:N]), NAN if poisoned else 0.0)
        s_seg, s_start, s_segs, s_st = _table_slabs(dev, seg, start, segs, st, poisoned)
        s_hist = Slab(dev, n_hist, 2, front=64, back=64, dtype=torch.int32).fill_canary()
        ins = (s_pts, s_seg, s_start, s_segs, s_st)
        before = [s.bits().clone() for s in ins]
        _fill_if_poisoned()
        rc = lib().lm_line_hist_points(C.c_void_p(s_pts.ptr()), N, C.c_void_p(s_seg.ptr()), len(seg), C.byref(g), C.c_void_p(s_start.ptr()),
                                       C.c_void_p(s_segs.ptr()), HW, C.c_void_p(s_st.ptr()), L, ZTOL, RQ, SH, 0, C.c_void_p(s_hist.ptr()),
                                       n_hist, cur)
        assert rc == 0, lib().lm_last_error()
        torch.cuda.synchronize()
        for s, b in zip(ins, before):
            assert torch.equal(s.bits(), b), 'an input was written'
        return {'hist': (s_hist, n_hist)}

    got = guarded_runs(run, 'line_hist_points', batch=False)
    _same('guarded', _hist_of(got['hist'], want.shape), want)


def test_hist_records_guards(dev, tmp_path):
    """lm_las_line_hist_records with the records, the tables and hist between guard slabs: 257 records of 37 bytes (the last dword of the
    records is padding, the last block holds one record), with a select; las_profile_kernel<false, false, true> after poisoned LDS."""
    _, seg, _, st = _scene()
    fmt, extra, n = 7, 1, 257
    rl = tc.RECORD_LEN[fmt] + extra
    rec, flat = tc._records(tmp_path, fmt, extra, n, seed=7)
    g, start, segs = ops.line_index_host(seg, HW)
    sel = PointFilter(classes=[2], drop_withheld=False)
    want = tr.hist_f32(lr.decode_f32(rec, tc.SCALE, tc.OFFSET, tc.ZERO), seg, st, L, HW, ZTOL, RQ, SH, mask=tc._passes(rec, fmt, sel))[0]
    n_hist = want.size
    assert want.sum() > 10
    sst = sel.as_struct()
    cur = _handle(torch.cuda.current_stream(dev))

    def run(B, poisoned):
        s_rec = Slab(dev, 1, len(flat), front=1, back=1, dtype=torch.uint8).fill_input(torch.from_numpy(flat), 0xFF if poisoned else 0)
        s_seg, s_start, s_segs, s_st = _table_slabs(dev, seg, start, segs, st, poisoned)
        s_hist = Slab(dev, n_hist, 2, front=64, back=64, dtype=torch.int32).fill_canary()
        ins = (s_rec, s_seg, s_start, s_segs, s_st)
        before = [s.bits().clone() for s in ins]
        _fill_if_poisoned()
        rc = lib().lm_las_line_hist_records(C.c_void_p(s_rec.ptr()), rl, fmt, n, _d3(tc.SCALE), _d3(tc.OFFSET), None, C.byref(sst),
                                            C.c_void_p(s_seg.ptr()), len(seg), C.byref(g), C.c_void_p(s_start.ptr()), C.c_void_p(s_segs.ptr()),
                                            HW, C.c_void_p(s_st.ptr()), L, ZTOL, RQ, SH, 0, C.c_void_p(s_hist.ptr()), n_hist, cur)
        assert rc == 0, lib().lm_last_error()
        torch.cuda.synchronize()
        for s, b in zip(ins, before):
            assert torch.equal(s.bits(), b), 'an input was written'
        return {'hist': (s_hist, n_hist)}

    for attempt in range(2):                                             # the second round: the same bits again
        got = guarded_runs(run, 'las_line_hist_records', batch=False)
        _same('guarded', _hist_of(got['hist'], want.shape), want)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_name_the_argument_and_write_nothing(dev, tmp_path):
    _, seg, pts, st = _scene()
    index, stations = _device_tables(dev)
    Z, NB = 11, 1024
    n_hist, n = L * Z * NB, 300
    rec, flat = tc._records(tmp_path, 1, 0, n, seed=1)
    d_rec = torch.from_numpy(flat).to(dev)
    d_pts = _t(pts[:n + 1]).to(dev)
    hist = torch.full((n_hist + NB,), POISON, dtype=torch.int64, device=dev)
    Lb = lib()
    cur = _handle(torch.cuda.current_stream(dev))
    # positions: points 0, N 1, segments 2, S 3, grid 4, cell_start 5, cell_segs 6, half_width 7, stations 8, L 9, z_tol 10, ring_q 11,
    # bin_shift 12, accumulate 13, hist 14, n_hist 15, stream 16; the record entry: the same from segments on, six further back
    p_base = [C.c_void_p(d_pts.data_ptr()), n, *index.args(), stations.args()[0], L, ZTOL, RQ, SH, 0, C.c_void_p(hist.data_ptr()), n_hist, cur]
    r_base = [C.c_void_p(d_rec.data_ptr()), 28, 1, n, _d3(tc.SCALE), _d3(tc.OFFSET), None, None, *index.args(), stations.args()[0], L, ZTOL, RQ, SH,
              0, C.c_void_p(hist.data_ptr()), n_hist, cur]
    assert len(p_base) == 17 and len(r_base) == 23
    assert Lb.lm_line_hist_points(*p_base) == 0 and Lb.lm_las_line_hist_records(*r_base) == 0, Lb.lm_last_error()
    torch.cuda.synchronize()
    assert bool((hist[n_hist:] == POISON).all()) and int(hist[:n_hist].sum()) > 0
    hist.fill_(POISON)

    def refused(what, **change):
        """`change`: position in the points entry -> new value; applied to both entries (the record entry: position + 6 from 2 on)."""
        for name, fn, base, shift in (('line_hist_points', Lb.lm_line_hist_points, p_base, 0),
                                      ('las_line_hist_records', Lb.lm_las_line_hist_records, r_base, 6)):
            a = list(base)
            for pos, v in change.items():
                a[int(pos[1:]) + shift] = v
            rc = fn(*a)
            torch.cuda.synchronize()
            msg = Lb.lm_last_error().decode()
            assert rc == 1 and msg.startswith(name + ':') and what in msg, f'{name}, {what}: rc={rc}, message {msg!r}'
            assert bool((hist == POISON).all()), f'{name}, {what}: hist was written'

    off = lambda pos, by: {f'p{pos}': C.c_void_p(p_base[pos].value + by)}
    for pos, what, by in ((2, 'segments', 8), (5, 'cell_start', 1), (6, 'cell_segs', 2), (8, 'stations', 4), (14, 'hist', 4)):
        refused(f'{what} is not', **off(pos, by))
    refused('hist is not 8-byte aligned', **off(14, 4))
    refused('null pointer (stations)', p8=None)
    refused('null pointer (hist)', p14=None)
    refused('segments', p2=None)
    # what the histogram adds
    refused('ring_q=0', p11=0)
    refused('ring_q=-3', p11=-3)
    refused('bin_shift=-1', p12=-1)
    refused('bin_shift=9', p12=9)
    refused('n_hist', p15=n_hist + 1)
    refused('n_hist', p15=n_hist - NB)
    refused('n_hist', p11=RQ // 2)                                        # another ring_q: another Z for the same n_hist
    refused('n_hist', p12=SH + 1)                                         # another bin_shift: another NB
    refused('accumulate=2', p13=2)
    refused('accumulate=-1', p13=-1)
    # the 2^27 cap: 7 lines of 321 rings of 65536 counts are 1.09 x 2^27 (6 lines would be inside it).  n_hist stays the size of the
    # buffer there is: whatever the cap check does, no call here may be told of more counts than `hist` holds
    assert 7 * 321 * 65536 > 1 << 27 > 6 * 321 * 65536
    refused('at most 2^27', p9=7, p11=1, p12=0)
    # what the cross entries refuse of the shared arguments
    refused('z_tol=16.5', p10=16.5)
    refused('z_tol', p10=float('inf'))
    refused('z_tol', p10=NAN)
    refused('segments carry lines', p9=1, p15=Z * NB)
    refused('L=-1', p9=-1)
    wide = ops.line_index(seg, 0.25, device=dev)
    refused('half_width', p4=C.byref(wide.grid))
    other = ops.line_index(seg[:-1], HW, device=dev)
    refused('grid', p4=C.byref(other.grid))
    huge = ops.line_index(seg, 16.5, device=dev)
    ha = huge.args()
    refused('half_width=16.5', p2=ha[0], p4=ha[2], p5=ha[3], p6=ha[4], p7=16.5)
    refused('half_width', p7=-1.0)
    # what only one entry takes
    for pos, v, what in ((0, C.c_void_p(d_pts.data_ptr() + 4), 'points_xyzi is not'), (0, None, 'points_xyzi'), (1, -1, 'N=')):
        a = list(p_base)
        a[pos] = v
        assert Lb.lm_line_hist_points(*a) == 1 and what in Lb.lm_last_error().decode(), (what, Lb.lm_last_error())
    for pos, v, what in ((0, C.c_void_p(d_rec.data_ptr() + 1), 'records is not'), (0, None, 'records'), (1, 27, 'record_len'), (2, 11, 'point_format'),
                         (3, -1, 'n='), (4, None, 'scale')):
        a = list(r_base)
        a[pos] = v
        assert Lb.lm_las_line_hist_records(*a) == 1 and what in Lb.lm_last_error().decode(), (what, Lb.lm_last_error())
    torch.cuda.synchronize()
    assert bool((hist == POISON).all())
    # the package entries
    thr = PaintThreshold(half_width=HW, ring=RQ / 1024, inner=RQ / 1024, outer=0.25, z_tol=ZTOL)
    with pytest.raises(ValueError, match='half_width'):
        las_io.hist_records(d_rec, tc._header(1, 28, n), wide, stations, thr)
    with pytest.raises(TypeError, match='PaintThreshold'):
        las_io.hist_records(d_rec, tc._header(1, 28, n), index, stations, MarkingSurvey())
    with pytest.raises(TypeError, match='LineStations'):
        las_io.hist_records(d_rec, tc._header(1, 28, n), index, st, thr)


# ------------------------------------------------------------------------------------------------ 6. LDS state
def test_records_entry_does_not_depend_on_what_lds_held(dev, tmp_path):
    """The record entry's own LDS-state case (lds_state.poisoned finds entries by a leading stream and cannot wrap this one): for each
    word of lds_state.WORDS all of every CU's LDS is filled with it on the current stream, as the last thing before the entry; the
    table must not change by a bit.  Two files: 37-byte records with a last block of one, and 28-byte records."""
    _, seg, _, st = _scene()
    index, stations = _device_tables(dev)
    cur = torch.cuda.current_stream(dev)
    for fmt, extra, n in ((7, 1, 257), (1, 0, 700)):
        rl = tc.RECORD_LEN[fmt] + extra
        rec, flat = tc._records(tmp_path, fmt, extra, n, seed=31 + fmt)
        d_rec = torch.from_numpy(flat).to(dev)
        want = tr.hist_f32(lr.decode_f32(rec, tc.SCALE, tc.OFFSET, tc.ZERO), seg, st, L, HW, ZTOL, RQ, SH)[0]
        outs = {}
        for word in lds_state.WORDS:
            hist = torch.full(want.shape, POISON, dtype=torch.int64, device=dev)
            lds_state.fill(word)
            _records_call(d_rec, rl, fmt, n, None, index, stations, RQ, SH, 0, hist, cur)
            torch.cuda.synchronize()
            outs[word] = hist.cpu()
        for word in lds_state.WORDS[1:]:
            lds_state.assert_same_bits(outs[word], outs[lds_state.WORDS[0]], f'las_line_hist_records, format {fmt}, after LDS = 0x{word:08X}')
        _same(f'format {fmt} after poisoned LDS', outs[0xFFFFFFFF], want)


# ------------------------------------------------------------------------------------------------ 7. streams
def _stream_case(dev, name, make_inputs, call, want_of):
    """The two entries' own stream case.  make_inputs(k) -> the host arrays of data set k (same sizes); call(device inputs, hist, stream)
    enqueues the entry on `stream`; want_of(k) -> the brute force.  (a) on a side stream, given that stream's handle: the bits of the
    default-stream run.  (b) captured on one stream into a graph, then per data set: the inputs altered in place, hist pre-filled with
    0xFF, one replay - bit-identical to an eager run on the same data."""
    default = torch.cuda.current_stream(dev)
    ins = [torch.from_numpy(np.array(a, copy=True)).to(dev) for a in make_inputs(0)]
    shape = want_of(0).shape
    base = torch.full(shape, POISON, dtype=torch.int64, device=dev)
    call(ins, base, default)
    torch.cuda.synchronize(dev)
    _same(f'{name}, default stream', base, want_of(0))
    side = torch.cuda.Stream(dev)
    assert side.cuda_stream != default.cuda_stream
    on_side = torch.full(shape, POISON, dtype=torch.int64, device=dev)
    side.wait_stream(default)
    with torch.cuda.stream(side):
        call(ins, on_side, side)
    side.synchronize()
    lds_state.assert_same_bits(on_side, base, f'{name} on a side stream')
    cap = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    out = torch.empty(shape, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.graph(graph, stream=cap):
        call(ins, out, torch.cuda.current_stream(dev))
    for k in (1, 2, 0):
        for t, a in zip(ins, make_inputs(k)):
            t.copy_(torch.from_numpy(np.array(a, copy=True)))
        out.view(torch.uint8).fill_(0xFF)
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        replayed = out.cpu().clone()
        eager = torch.full(shape, POISON, dtype=torch.int64, device=dev)
        call(ins, eager, torch.cuda.current_stream(dev))
        torch.cuda.synchronize(dev)
        lds_state.assert_same_bits(replayed, eager, f'{name}, graph replay on data set {k} over a table pre-filled with 0xFF')
        _same(f'{name}, data set {k}', eager, want_of(k))
    del graph


def test_points_entry_on_a_side_stream_and_in_graph_replay(dev):
    _, seg, pts, st = _scene()
    index, stations = _device_tables(dev)
    N = 3 * CHUNK + 5
    sets = {k: pts[np.random.RandomState(40 + k).permutation(len(pts))[:N]] if k else pts[:N] for k in range(3)}

    @functools.lru_cache(maxsize=None)
    def want_of(k):
        return tr.hist_f32(sets[k], seg, st, L, HW, ZTOL, RQ, SH)[0]

    assert not np.array_equal(want_of(1), want_of(2)) and not np.array_equal(want_of(0), want_of(1))
    _stream_case(dev, 'line_hist_points', lambda k: [sets[k]],
                 lambda ins, hist, s: _points_call(ins[0], N, index, stations, RQ, SH, 0, hist, s), want_of)


def test_records_entry_on_a_side_stream_and_in_graph_replay(dev, tmp_path):
    _, seg, _, st = _scene()
    index, stations = _device_tables(dev)
    fmt, extra, n = 3, 0, 777
    rl = tc.RECORD_LEN[fmt] + extra
    files = {k: tc._records(tmp_path, fmt, extra, n, seed=60 + k) for k in range(3)}

    @functools.lru_cache(maxsize=None)
    def want_of(k):
        return tr.hist_f32(lr.decode_f32(files[k][0], tc.SCALE, tc.OFFSET, tc.ZERO), seg, st, L, HW, ZTOL, RQ, SH)[0]

    assert not np.array_equal(want_of(1), want_of(2)) and not np.array_equal(want_of(0), want_of(1))
    _stream_case(dev, 'las_line_hist_records', lambda k: [files[k][1]],
                 lambda ins, hist, s: _records_call(ins[0], rl, fmt, n, None, index, stations, RQ, SH, 0, hist, s), want_of)


# ------------------------------------------------------------------------------------------------ 8. files
def test_hist_files_finds_the_threshold_of_a_painted_scene(dev, tmp_path):
    """Two lines along +x, 12 m long, A at y = 2 and B at y = 5, under the defaults (half_width 0.625 m, rings of 1/16 m, bins of 64).
    Returns on a lattice, x = 0.025 + 0.05 i, lateral offsets (2 j + 1) / 128 m, j = -48 .. 47 (q = 8 (2 j + 1): 8 or 24 past a multiple
    of 16, float32 decides nothing).  A is painted (24000) where -6 <= j <= 5, |o| < 0.09 m; B is not.  Asphalt 3000 + 40 (i mod 97).
    Two files of two point formats, each return in one of them.  The strip and line 1 have a threshold between asphalt and paint, line
    2 has none."""
    thr = PaintThreshold()
    i, j = np.meshgrid(np.arange(240), np.arange(-48, 48), indexing='ij')
    i, j = i.ravel(), j.ravel()
    world, inten = [], []
    for y0, painted in ((2.0, True), (5.0, False)):
        world.append(np.stack([0.025 + 0.05 * i, y0 + (2 * j + 1) / 128.0, np.zeros(len(i))], axis=1))
        inten.append(np.where(painted & (j >= -6) & (j <= 5), 24000, 3000 + 40 * (i % 97)))
    world, inten = np.concatenate(world) + lr.SHIFT, np.concatenate(inten)
    order = np.random.RandomState(11).permutation(len(world))
    half = len(order) // 2
    paths = []
    for k, part in enumerate((order[:half], order[half:])):
        paths.append(str(tmp_path / f'scene{k}.las'))
        tc.las_ref.write_las(paths[k], world[part], inten[part], point_format=(1, 6)[k], version=((1, 2), (1, 4))[k], offset=tuple(lr.SHIFT),
                             scale=(1 / 1024, 1 / 1024, 1 / 1024))
    xs = np.arange(0.0, 14.0, 2.0)
    lines = [np.stack([xs, np.full_like(xs, y0), np.zeros_like(xs)], axis=1) + lr.SHIFT for y0 in (2.0, 5.0)]
    seg = las_io.line_segments(lines, lr.SHIFT)
    st, _ = las_io.line_stations(lines, lr.SHIFT, las_io.HIST_BIN)
    dec = []
    for path in paths:
        data = np.fromfile(path, np.uint8)
        h = las_io.parse_header(data)
        o, rl, n = h['offset_to_points'], h['record_len'], h['n_points']
        dec.append(lr.decode_f32(data[o:o + n * rl].reshape(n, rl), h['scale'], h['offset'], lr.SHIFT))
    want, terms, lab, _ = tr.hist_f32(np.concatenate(dec), seg, st, 2, thr.half_width, thr.z_tol, thr.ring_q, thr.bin_shift)
    assert (lab > 0).sum() == 2 * 240 * 80 and set(np.unique(terms['q'][lab > 0] % 16)) == {8}
    got = las_io.hist_files([(p, lr.SHIFT, None) for p in paths], lines, thr, device=dev)
    _same('hist_files', got, want)
    found = las_io.paint_threshold(got, thr)
    tr.same_policy(found, tr.policy(want))
    g = found['strip']
    print(f'strip {g}\nline 1 {found["lines"][1]}\nline 2 {found["lines"][2]}')
    assert g['supported'] and 6880 < g['threshold'] <= 24000 and found['lines'][1]['supported'] and found['lines'][1]['paint_share'] == 0.75
    assert not found['lines'][2]['supported'] and found['lines'][2]['threshold'] is None and found['lines'][2]['inner_returns'] == 240 * 16
    none = las_io.hist_files([], lines, thr, device=dev)
    assert none.shape == (2, 11, 1024) and none.dtype == np.int64 and not none.any()


# ------------------------------------------------------------------------------------------------ 9. Runner
def _dir_files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


ASPHALT, PAINT, CLIP = 34000, 60000, 33000.0


def _tile_strip(tmp_path):
    """A strip of one tile, modelled on test_gpu_cross's: a 1152 x 1152 window over a climbing plane, one return at every pixel centre,
    ASPHALT + 40 ((r + 3 c) mod 97) bright - every return at or above the rasteriser's CLIP, so the tile the network sees is the same
    whatever is painted above it.  -> (world [n, 3], intensity [n], the file order, the parameter file, the read offset)."""
    H = W = 1152
    reso, A, Bs = 0.05, 0.075, 0.02
    off = np.array([351200.0, 3433000.0, 12.0])
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    x, y = (r * reso).ravel(), (c * reso).ravel()
    inten = ASPHALT + 40 * ((r + 3 * c) % 97).ravel()
    world = np.stack([x, y, A * x + Bs * y], axis=1)
    order = np.random.RandomState(3).permutation(len(world))
    p = {'coor_las_path': '', 'las_read_offset': list(off), 'las_rotation_trans_quan': [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0],
         'bev_img_offset': [0.0, 0.0], 'img_reso': [reso, reso], 'local_min_ele': -0.5, 'ele_reso': 0.05}
    prm = str(tmp_path / '181020_0209.txt')
    tc.io_utils.save_pc_2_img_transform_paras(prm, p)
    assert inten.min() == ASPHALT > CLIP == las_io.INTEN_MAX and inten.max() == ASPHALT + 3840 < PAINT
    return world[order] + off, inten[order], prm, off


def _result_lines(result):
    lines3d, merged = result
    return list(merged) if len(merged) else [l for name in sorted(lines3d) for l in lines3d[name]]


def test_runner_strip_finds_its_threshold_and_hands_it_to_the_auto_stages(dev, net, tmp_path):
    """Runner.infer_las_strip_to_map with survey, cross and residue all asking for 'auto'.  The network of the tests carries synthetic
    weights: the lines it returns follow no paint.  So the paint is planted where the lines are: every return of the strip lies at or
    above the rasteriser's intensity clip, which makes the tile, and with it the lines, the same for every such file (asserted); the
    BARE file holds asphalt alone, the PAINTED one PAINT on the returns within 0.075 m of a line the bare run returned.
    On the painted file: params/paint_hist.npy equals the brute force against the returned lines, paint_threshold.json is
    threshold_ref's policy of it, the threshold lies between the brightest asphalt and the paint, and markings.npy,
    cross_sections.npy and residue.npy hold the bytes of a second run that is handed the found number.  A run with neither
    `threshold=` nor 'auto' writes neither file; the bare strip is refused."""
    from lanemapping_amd.runner import Runner
    world, inten, prm, off = _tile_strip(tmp_path)
    rn = Runner.__new__(Runner)
    rn.cfg, rn.device, rn.net = net.cfg, dev, net
    assert rn.cfg.get('las_threshold') is None
    out = {k: str(tmp_path / k) for k in ('plain', 'auto', 'given', 'asphalt')}
    bare = str(tmp_path / 'bare' / 'strip.las')
    os.makedirs(os.path.dirname(bare))
    tc.las_ref.write_las(bare, world, inten, point_format=1, offset=tuple(off))
    plain = rn.infer_las_strip_to_map(bare, [prm], work_dirs=out['plain'], batch_size=2)
    lines = _result_lines(plain)
    assert lines, 'the strip yielded no lines'
    # the paint: the returns within 0.075 m of a returned line, found with the labelling entry (tests/test_gpu_label.py holds it to its
    # own brute force; here it only builds the scene)
    cloud = las_io.read_las_raw(bare, dev, shift=off)[0]
    near = ops.label_points(cloud, ops.line_index(las_io.line_segments(lines, off), 0.075, device=dev), 0.5).cpu().numpy() > 0
    assert len(near) == len(inten) and 0.02 < near.mean() < 0.5
    painted = str(tmp_path / 'painted' / 'strip.las')
    os.makedirs(os.path.dirname(painted))
    tc.las_ref.write_las(painted, world, np.where(near, PAINT, inten), point_format=1, offset=tuple(off))
    auto = rn.infer_las_strip_to_map(painted, [prm], work_dirs=out['auto'], batch_size=2, survey=MarkingSurvey(min_intensity='auto'),
                                     cross=CrossSection('auto'), residue=PaintResidue('auto'))
    again = _result_lines(auto)
    assert len(again) == len(lines) and all(np.array_equal(a, b) for a, b in zip(again, lines)), 'paint above the clip moved the lines'
    thr = PaintThreshold()
    data = np.fromfile(painted, np.uint8)
    h = las_io.parse_header(data)
    o, rl, n = h['offset_to_points'], h['record_len'], h['n_points']
    dec = lr.decode_f32(data[o:o + n * rl].reshape(n, rl), h['scale'], h['offset'], off)
    seg = las_io.line_segments(lines, off)
    st, _ = las_io.line_stations(lines, off, las_io.HIST_BIN)
    want, _, line, _ = tr.hist_f32(dec, seg, st, len(lines), thr.half_width, thr.z_tol, thr.ring_q, thr.bin_shift, pruned=True)
    _same('paint_hist.npy', np.load(os.path.join(out['auto'], 'params', 'paint_hist.npy')), want)
    policy = tr.policy(want)
    used = json.load(open(os.path.join(out['auto'], 'params', 'paint_threshold.json')))
    assert used == json.loads(json.dumps({'strip': policy['strip'], 'lines': {str(k): g for k, g in policy['lines'].items()}}))
    g = policy['strip']
    print(f'{len(lines)} lines, {len(seg)} segments, {int((line > 0).sum())} of {n} records in the table, {int(near.sum())} painted; strip {g}; '
          f'{sum(v["supported"] for v in policy["lines"].values())} lines supported')
    assert g['supported'] and ASPHALT + 3840 < g['threshold'] <= PAINT
    # the same stages, handed the number
    T = g['threshold']
    rn.infer_las_strip_to_map(painted, [prm], work_dirs=out['given'], batch_size=2, survey=MarkingSurvey(min_intensity=T),
                              cross=CrossSection(T), residue=PaintResidue(T))
    for name in ('markings.npy', 'cross_sections.npy', 'residue.npy', 'markings.json', 'cross_sections.json', 'residue.json'):
        a, b = (open(os.path.join(out[k], 'params', name), 'rb').read() for k in ('auto', 'given'))
        assert a == b and len(a) > 0, name
    assert int(np.load(os.path.join(out['auto'], 'params', 'markings.npy'))[:, 0].sum()) > 0, 'the survey counted no paint'
    new = [os.path.join('params', 'paint_hist.npy'), os.path.join('params', 'paint_threshold.json')]
    assert sorted(set(_dir_files(out['auto'])) - set(_dir_files(out['given']))) == sorted(new)
    assert not set(_dir_files(out['plain'])) & set(new) and set(_dir_files(out['plain'])) <= set(_dir_files(out['given']))
    # asphalt alone
    with pytest.raises(ValueError, match=r"'auto' needs a threshold.*separation 0\.\d+ with \d+ returns on the lines and \d+ beside them") as e:
        rn.infer_las_strip_to_map(bare, [prm], work_dirs=out['asphalt'], batch_size=2, survey=MarkingSurvey(min_intensity='auto'))
    print(e.value)
    refused = json.load(open(os.path.join(out['asphalt'], 'params', 'paint_threshold.json')))
    assert refused['strip']['supported'] is False and refused['strip']['threshold'] is None and refused['strip']['inner_returns'] > 1000
    assert not os.path.exists(os.path.join(out['asphalt'], 'params', 'markings.npy')), 'no stage ran'
