"""GPU: the cross-sections along every line (csrc/profile.hip: lm_line_cross_points, lm_las_line_cross_records; ops.line_cross,
las_io.cross_records / cross_files / cross_summary / snap_lines, Runner `cross=`).

The reference is tests/cross_ref.py: the float32 rule by brute force over all segments on top of label_ref's winner and profile_ref's
per-point terms, and an integer accumulation.  The table is compared in every int64."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import cross_ref as cr
import label_ref as lr
import profile_ref as pr
from guards import Slab, guarded_runs
from lanemapping_amd import io_utils, las_io, ops
from lanemapping_amd._lib import lib
from lanemapping_amd.las_io import CrossSection, PointFilter
from oracle import las_ref

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float('nan')
CHUNK = 1024                                   # points per workgroup of cross_points_kernel (csrc/profile.hip: CHUNK = 256 * PER)
POISON = -7
HW, ZTOL, LQ, PAINT = 0.3125, 0.5, 32, 24000   # half_width exact in float32: hq = 320, nl = 21
SPECIAL = {'tie': 0, 'left_edge': 1, 'right_edge': 2, 'before': 3, 'past': 4, 'doubled': 5, 'nan_i': 6, 'nan_x': 7, 'nan_y': 8, 'nan_z': 9}


def _lines():
    """Line 1: a polyline with a bend and a zero-length segment (a doubled vertex).  Line 2 crosses it in a vertex of both.  Line 3 has
    one vertex: no segment, no bins.  All values are exact in float32."""
    l1 = np.array([[0.0, 2.0, 0.0], [3.0, 2.0, 0.03125], [6.0, 2.0, 0.0625], [6.0, 2.0, 0.0625], [10.0, 5.0, 0.125], [14.0, 5.0, 0.125]])
    l2 = np.array([[3.0, -1.0, 0.0], [3.0, 2.0, 0.03125], [3.0, 5.0, 0.0625]])
    l3 = np.array([[8.0, 0.0, 0.0]])
    return [l1, l2, l3]


@functools.lru_cache(maxsize=None)
def _scene(n_random=20000, seed=9):
    """-> (lines, segments, points): the special points (SPECIAL) followed by random points around the segments, a third of them on the
    1/64 m lattice (exact ties), intensities 0 .. 39999 and a few NaN.  Computed once, never changed."""
    lines = _lines()
    seg = las_io.line_segments(lines, None)
    rng = np.random.RandomState(seed)
    P = [(3.0, 2.0, 0.03125, 30000.0),                   # the vertex both lines share: d2 = 0 to both, the smaller line wins
         (1.5, 2.0 + HW, 0.015625, 30000.0),             # exactly half_width left of line 1: q = hq, the last cell
         (1.5, 2.0 - HW, 0.015625, 1000.0),              # exactly half_width right: cell 0
         (-0.2, 2.0, 0.0, 30000.0), (14.2, 5.0, 0.125, 1000.0),     # before the start and past the end of line 1: t is clamped
         (6.0, 2.0, 0.0625, 24000.0),                    # on the doubled vertex, intensity exactly paint_iq
         (2.0, 2.1, 0.02, NAN),                          # a NaN intensity: counted, iq = 0
         (NAN, 2.0, 0.0, 1000.0), (2.0, NAN, 0.0, 1000.0), (2.0, 2.0, NAN, 1000.0)]
    s = rng.randint(0, len(seg), n_random)
    t = rng.uniform(-0.05, 1.05, n_random)
    base = seg[s, 0:3].astype(np.float64) + t[:, None] * seg[s, 3:6].astype(np.float64)
    rnd = base + np.stack([rng.uniform(-0.5, 0.5, n_random), rng.uniform(-0.5, 0.5, n_random), rng.uniform(-0.7, 0.7, n_random)], axis=1)
    snap = rng.rand(n_random) < 0.33
    rnd[snap, :2] = np.round(rnd[snap, :2] * 64) / 64
    inten = rng.randint(0, 40000, n_random).astype(np.float64)
    inten[rng.rand(n_random) < 0.01] = NAN
    pts = np.concatenate([np.asarray(P, np.float64), np.concatenate([rnd, inten[:, None]], axis=1)]).astype(f32)
    seg.setflags(write=False), pts.setflags(write=False)
    return lines, seg, pts


@functools.lru_cache(maxsize=None)
def _tables(bin):
    st, bs = las_io.line_stations(_scene()[0], None, bin)
    st.setflags(write=False), bs.setflags(write=False)
    return st, bs


@functools.lru_cache(maxsize=None)
def _winner(half_width):
    _, seg, pts = _scene()
    line, best, win = lr.label_f32(pts, seg, half_width, ZTOL)
    return line, best, win


def _ref(bin, half_width=HW, lateral_q=LQ, paint_iq=PAINT, N=None):
    """The brute force on the first N points of the scene: -> (cells, terms)."""
    _, seg, pts = _scene()
    st, bs = _tables(bin)
    line, _, win = _winner(half_width)
    N = len(pts) if N is None else N
    terms = cr.cross_terms(pts[:N], seg, st, bs, bin, half_width, lateral_q, line[:N], win[:N])
    return cr.accumulate(terms, int(bs[-1]), cr.hq_nl(half_width, lateral_q)[1], paint_iq), terms


def _t(a):
    return torch.from_numpy(np.array(a, copy=True))              # (the shared scene arrays are read-only)


def _device_tables(dev, bin, half_width=HW):
    st, bs = _tables(bin)
    return ops.line_index(_scene()[1], half_width, device=dev), ops.line_stations(st, bs, bin, device=dev)


def _same(tag, got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.int64 and got.shape == want.shape, f'{tag}: {got.dtype} {got.shape}, expected {want.shape}'
    g, w = got.reshape(-1, 4), want.reshape(-1, 4)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert not len(bad), f'{tag}: {len(bad)} cells differ from the brute force; first row {bad[0]}: {g[bad[0]].tolist()} != {w[bad[0]].tolist()}'


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ------------------------------------------------------------------------------------------------ 1. exactness
def test_the_scene_holds_what_it_is_meant_to_hold():
    """No GPU work: the reference puts the special points where the rule says, so the comparisons below mean what they claim."""
    _, seg, pts = _scene()
    bin = pr.BIN_EXACT
    st, bs = _tables(bin)
    cells, terms = _ref(bin)
    line, best, win = _winner(HW)
    hq, nl = cr.hq_nl(HW, LQ)
    assert (hq, nl) == (320, 21) and bs.tolist()[-2:] == [int(bs[2]), int(bs[2])] and bs[1] == 120 and bs[2] == 168 and len(seg) == 7
    S = SPECIAL
    two = lr.label_f32(pts[:1], seg[lr.seg_lines(seg) == 2], HW, ZTOL)
    assert line[S['tie']] == 1 and best[S['tie']] == 0 and two[0][0] == 2 and two[1][0] == 0, 'an exact tie between lines 1 and 2'
    assert line[S['left_edge']] == 1 and terms['q'][S['left_edge']] == hq and terms['c'][S['left_edge']] == nl - 1
    assert line[S['right_edge']] == 1 and terms['q'][S['right_edge']] == -hq and terms['c'][S['right_edge']] == 0
    assert line[S['before']] == 1 and terms['t'][S['before']] == 0 and terms['b'][S['before']] == 0
    assert line[S['past']] == 1 and terms['t'][S['past']] == 1 and terms['b'][S['past']] == 119
    assert line[S['doubled']] == 1 and terms['q'][S['doubled']] == 0 and terms['iq'][S['doubled']] == PAINT
    assert line[S['nan_i']] == 1 and terms['iq'][S['nan_i']] == 0 and all(line[S[k]] == 0 for k in ('nan_x', 'nan_y', 'nan_z'))
    assert set(np.unique(line)) == {0, 1, 2} and (line == 0).sum() > 2000 and (line > 0).sum() > 6000
    assert (terms['zq'] != 0).sum() > 5000 and terms['zq'].min() < -400 and terms['zq'].max() > 400
    n = cells[..., 0]
    assert (n > 1).sum() > 500 and (n == 0).sum() > 100 and 0 < cells[..., 1].sum() < n.sum() and n.sum() == (line > 0).sum()
    d2 = best[line > 0]
    assert len(d2) - len(np.unique(d2)) > 100, 'lattice points at equal distances'


@pytest.mark.parametrize('bin', [pr.BIN_EXACT, pr.BIN_INEXACT])
def test_table_equals_the_float32_brute_force(dev, bin):
    _, seg, pts = _scene()
    st, bs = _tables(bin)
    assert (float(f32(bin)) == bin) == (bin == pr.BIN_EXACT)
    index, stations = _device_tables(dev, bin)
    d_pts = _t(pts).to(dev)
    nl = cr.hq_nl(HW, LQ)[1]
    assert len(pts) > 2 * CHUNK
    for paint_iq in (0, PAINT, 65536):
        want = _ref(bin, paint_iq=paint_iq)[0]
        got = ops.line_cross(d_pts, index, stations, ZTOL, LQ, paint_iq)
        assert tuple(got.shape) == (int(bs[-1]), nl, 4) and got.dtype == torch.int64
        _same(f'bin={bin}, paint_iq={paint_iq}', got, want)
        if paint_iq == 0:
            assert np.array_equal(want[..., 0], want[..., 1])
        if paint_iq == 65536:
            assert not want[..., 1].any()
    for N in (0, 1, 255, 1025):
        _same(f'bin={bin}, N={N}', ops.line_cross(d_pts[:N], index, stations, ZTOL, LQ, PAINT), _ref(bin, N=N)[0])
    assert _ref(bin, N=0)[0].sum() == 0 and _ref(bin, N=1)[0][..., 0].sum() == 1


def test_no_segments_one_cell_rows_and_the_finest_cells(dev):
    _, seg, pts = _scene()
    bin = pr.BIN_EXACT
    d_pts = _t(pts).to(dev)
    # S = 0: a line with one vertex alone - no bins, an empty table
    none_st, none_bs = las_io.line_stations([_lines()[2]], None, bin)
    assert none_bs.tolist() == [0, 0] and none_st.shape == (0, 4)
    empty = ops.line_cross(d_pts, ops.line_index(np.zeros((0, 8), f32), HW, device=dev), ops.line_stations(none_st, none_bs, bin, device=dev),
                           ZTOL, LQ, PAINT)
    assert tuple(empty.shape) == (0, 21, 4) and empty.dtype == torch.int64
    # lateral_q > 2 hq: one cell per station bin
    index, stations = _device_tables(dev, bin)
    wide = 2 * 320 + 1
    assert cr.hq_nl(HW, wide) == (320, 1) == ops.cross_cells(HW, wide)
    want = _ref(bin, lateral_q=wide)[0]
    _same('nl = 1', ops.line_cross(d_pts, index, stations, ZTOL, wide, PAINT), want)
    assert np.array_equal(want[:, 0], _ref(bin)[0].sum(axis=1))
    # lateral_q = 1 with half_width = 0.03: hq = ceil(30.72) = 31, 63 cells of 1/1024 m
    assert cr.hq_nl(0.03, 1) == (31, 63) == ops.cross_cells(0.03, 1)
    fine_index, _ = _device_tables(dev, bin, 0.03)
    want, terms = _ref(bin, half_width=0.03, lateral_q=1)
    assert want[..., 0].sum() > 300 and len(np.unique(terms['c'][terms['row'] >= 0])) > 40
    _same('lateral_q = 1', ops.line_cross(d_pts, fine_index, stations, ZTOL, 1, PAINT), want)


# ------------------------------------------------------------------------------------------------ 2. the corners of the accumulation
def test_merge_corners(dev):
    """What a merged accumulation can get wrong: every lane of every wave in one cell; no two lanes of any wave in one cell; the lanes of
    a wave split between two cells of one station bin.  Along the last segment of line 1, from (10, 5) to (14, 5), far from line 2."""
    _, seg, pts = _scene()
    bin, lq = 0.0625, 4
    st, bs = _tables(bin)
    index, stations = _device_tables(dev, bin)
    nl = cr.hq_nl(HW, lq)[1]
    assert nl == 161

    def run(tag, p):
        want, terms, line, _ = cr.cross_f32(p, seg, st, bs, bin, HW, ZTOL, lq, PAINT)
        assert (line == 1).all()
        _same(tag, ops.line_cross(_t(p).to(dev), index, stations, ZTOL, lq, PAINT), want)
        return want, terms

    one = np.repeat(np.asarray([[12.03125, 5.0 + 20.0 / 1024, 0.125 + 0.25, 30000.0]], f32), 4096, axis=0)
    want, terms = run('4096 points in one cell', one)
    assert want.max(axis=(0, 1)).tolist() == [4096, 4096, 4096 * 30000, 4096 * 256] and (want[..., 0] > 0).sum() == 1
    k = np.arange(4096)
    i, j = k // 128, k % 128                                               # 32 station bins x 128 lateral cells, 1 m and more from the bend
    spread = np.stack([11.03125 + 0.0625 * i, 5.0 + (4 * j + 2 - 256) / 1024.0, 0.125 + ((k * 7) % 41 - 20) / 256.0, 1000.0 * (k % 37)], axis=1).astype(f32)
    want, terms = run('4096 points in 4096 cells', spread)
    assert len(np.unique(terms['row'])) == 4096 and want[..., 0].max() == 1 and len(np.unique(terms['zq'])) == 41
    two = spread[:64].copy()
    two[:, 0] = 12.03125
    two[:, 1] = np.where(np.arange(64) % 2 == 0, 5.0 + 4.0 / 1024, 5.0 + 12.0 / 1024).astype(f32)
    want, terms = run('64 points in two cells of one row', two)
    assert len(np.unique(terms['B'])) == 1 and sorted(want[..., 0][want[..., 0] > 0].tolist()) == [32, 32]


def test_order_and_accumulation(dev):
    _, seg, pts = _scene()
    bin = pr.BIN_INEXACT
    want = _ref(bin)[0]
    index, stations = _device_tables(dev, bin)
    nl = cr.hq_nl(HW, LQ)[1]
    for seed in (1, 2):                                                    # a permutation of the points changes no bit
        d = _t(pts[np.random.RandomState(seed).permutation(len(pts))]).to(dev)
        for attempt in range(2):
            _same(f'permutation {seed}, run {attempt}', ops.line_cross(d, index, stations, ZTOL, LQ, PAINT), want)
    d_pts = _t(pts).to(dev)
    h = len(pts) // 2 + 7
    part = ops.line_cross(d_pts[:h], index, stations, ZTOL, LQ, PAINT)
    _same('first part', part, _ref(bin, N=h)[0])
    both = ops.line_cross(d_pts[h:], index, stations, ZTOL, LQ, PAINT, out=part)
    assert both.data_ptr() == part.data_ptr()
    _same('two accumulating calls', both, want)
    # accumulate = 0 on a poisoned buffer: as a fresh run
    cells = torch.full((stations.n_bins, nl, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    rc = lib().lm_line_cross_points(_stream(dev), C.c_void_p(d_pts.data_ptr()), len(pts), *index.args(), *stations.args(), ZTOL, LQ, PAINT, 0,
                                    C.c_void_p(cells.data_ptr()), stations.n_bins * nl)
    assert rc == 0, lib().lm_last_error()
    _same('accumulate=0 on poison', cells, want)
    with pytest.raises(ValueError, match='out must be'):
        ops.line_cross(d_pts, index, stations, ZTOL, LQ, PAINT, out=cells[:-1])
    with pytest.raises(TypeError, match='LineStations'):
        ops.line_cross(d_pts, index, _tables(bin)[0], ZTOL, LQ, PAINT)


# ------------------------------------------------------------------------------------------------ 3. records
SCALE, OFFSET = (0.001, 0.001, 0.001), (3.0, -2.0, 0.5)
ZERO = np.zeros(3)
RECORD_LEN = {0: 20, 1: 28, 3: 34, 6: 30, 7: 36}


def _world(n, seed):
    """n points around the scene's lines, intensities 0..39999."""
    seg = _scene()[1]
    rng = np.random.RandomState(seed)
    s = rng.randint(0, len(seg), n)
    base = seg[s, 0:3].astype(np.float64) + rng.uniform(0, 1, n)[:, None] * seg[s, 3:6].astype(np.float64)
    off = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.7, 0.7, n)], axis=1)
    return base + off, rng.randint(0, 40000, n)


def _records(tmp_path, fmt, extra, n, seed):
    """-> ([n, rl] records, padded flat copy for the device), as tests/test_gpu_profile.py builds them: written by oracle/las_ref.write_las
    where it knows the format, by the same layout here for format 7.  Classification 2 for four records of five and 7 for the fifth."""
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
    _, seg, _ = _scene()
    bin = pr.BIN_INEXACT
    st, bs = _tables(bin)
    index, stations = _device_tables(dev, bin)
    cross = CrossSection(PAINT, bin=bin, half_width=HW, lateral=LQ / 1024, z_tol=ZTOL)
    assert (cross.lateral_q, cross.paint_iq, cross.nl) == (LQ, PAINT, 21)
    rl = RECORD_LEN[fmt] + extra
    parts = []
    for n in (255, 257):
        rec, flat = _records(tmp_path, fmt, extra, n, seed=100 * fmt + n)
        dec = lr.decode_f32(rec, SCALE, OFFSET, ZERO)
        d_rec = torch.from_numpy(flat).to(dev)
        parts.append((d_rec, dec, n))
        for name, select in (('plain', None), ('class 2 only', PointFilter(classes=[2], drop_withheld=False))):
            tag = f'format {fmt}, {rl} B, n={n}, {name}'
            want, _, line, _ = cr.cross_f32(dec, seg, st, bs, bin, HW, ZTOL, LQ, PAINT, mask=_passes(rec, fmt, select))
            assert (line > 0).sum() > n // 20 and (line == 0).sum() > n // 20, tag
            before = d_rec.clone()
            got = las_io.cross_records(d_rec, _header(fmt, rl, n), index, stations, cross, None, select)
            _same(tag, got, want)
            assert torch.equal(d_rec, before), f'{tag}: the records were written'
            if select is None:                                  # the points entry on the decode's rows
                d_dec = las_io.decode_points(d_rec, rl, n, SCALE, OFFSET, None, normalise=False)
                assert np.array_equal(d_dec.cpu().numpy().view(np.int32), dec.view(np.int32))
                assert torch.equal(got, ops.line_cross(d_dec, index, stations, ZTOL, LQ, PAINT)), f'{tag}: the two entries differ'
            else:                                               # a dropped record on a line is not counted
                assert cr.cross_f32(dec, seg, st, bs, bin, HW, ZTOL, LQ, PAINT)[0][..., 0].sum() > want[..., 0].sum(), tag
    cells, want = None, None                                    # the two files into one table
    for d_rec, dec, n in parts:
        cells = las_io.cross_records(d_rec, _header(fmt, rl, n), index, stations, cross, None, out=cells)
        want = cr.cross_f32(dec, seg, st, bs, bin, HW, ZTOL, LQ, PAINT, cells=want)[0]
    _same(f'format {fmt}: two files into one table', cells, want)
    assert want[..., 0].sum() > 100


# ------------------------------------------------------------------------------------------------ 4. guarded buffers
def _table_slabs(dev, seg, start, segs, st, bs, poisoned):
    s_seg = Slab(dev, len(seg), 8, front=4, back=4).fill_input(_t(seg), NAN if poisoned else 0.0)
    s_start = Slab(dev, 1, len(start), front=1, back=1, dtype=torch.int32).fill_input(torch.from_numpy(start), 0x7FFFFFF0 if poisoned else 0)
    s_segs = Slab(dev, 1, len(segs), front=1, back=1, dtype=torch.int32).fill_input(torch.from_numpy(segs), 0x7FFFFFF0 if poisoned else 0)
    s_st = Slab(dev, len(st), 4, front=8, back=8).fill_input(_t(st), NAN if poisoned else 0.0)
    s_bs = Slab(dev, 1, len(bs), front=1, back=1, dtype=torch.int32).fill_input(_t(bs), 0x7FFFFFF0 if poisoned else 0)
    return s_seg, s_start, s_segs, s_st, s_bs


def _cells_of(slab_view, nl):
    return np.ascontiguousarray(slab_view.numpy()).view(np.int64).reshape(-1, nl, 4)


def test_cross_points_guards(dev):
    """lm_line_cross_points with the points, the segment table, the two lists, the stations, bin_start and cells each between guard slabs,
    N one past a workgroup's share: cells is written only inside [0, n_cells), poisoned guards change no output bit, no input is written."""
    _, seg, pts = _scene()
    bin = pr.BIN_EXACT
    st, bs = _tables(bin)
    nl = cr.hq_nl(HW, LQ)[1]
    N, n_cells = CHUNK + 1, int(bs[-1]) * nl
    g, start, segs = ops.line_index_host(seg, HW)
    host = np.array(bs, np.int32)

    def run(B, poisoned):
        s_pts = Slab(dev, N, 4, front=8, back=8).fill_input(_t(pts[:N]), NAN if poisoned else 0.0)
        s_seg, s_start, s_segs, s_st, s_bs = _table_slabs(dev, seg, start, segs, st, bs, poisoned)
        s_cells = Slab(dev, n_cells, 8, front=8, back=8, dtype=torch.int32).fill_canary()
        ins = (s_pts, s_seg, s_start, s_segs, s_st, s_bs)
        before = [s.bits().clone() for s in ins]
        rc = lib().lm_line_cross_points(_stream(dev), C.c_void_p(s_pts.ptr()), N, C.c_void_p(s_seg.ptr()), len(seg), C.byref(g),
                                        C.c_void_p(s_start.ptr()), C.c_void_p(s_segs.ptr()), HW, C.c_void_p(s_st.ptr()),
                                        C.c_void_p(s_bs.ptr()), C.c_void_p(host.ctypes.data), len(bs) - 1, bin, ZTOL, LQ, PAINT, 0,
                                        C.c_void_p(s_cells.ptr()), n_cells)
        assert rc == 0, lib().lm_last_error()
        torch.cuda.synchronize()
        for s, b in zip(ins, before):
            assert torch.equal(s.bits(), b), 'an input was written'
        return {'cells': (s_cells, n_cells)}

    got = guarded_runs(run, 'line_cross_points', batch=False)
    _same('guarded', _cells_of(got['cells'], nl), _ref(bin, N=N)[0])


def test_cross_records_guards(dev, tmp_path):
    """lm_las_line_cross_records with the records, the tables and cells between guard slabs: 257 records of 37 bytes (the last dword of
    the records is padding, the last block holds one record), with a select; las_profile_kernel<false, true> after poisoned LDS."""
    _, seg, _ = _scene()
    bin = pr.BIN_EXACT
    st, bs = _tables(bin)
    nl = cr.hq_nl(HW, LQ)[1]
    fmt, extra, n = 7, 1, 257
    rl = RECORD_LEN[fmt] + extra
    rec, flat = _records(tmp_path, fmt, extra, n, seed=7)
    g, start, segs = ops.line_index_host(seg, HW)
    n_cells, host = int(bs[-1]) * nl, np.array(bs, np.int32)
    sel = PointFilter(classes=[2], drop_withheld=False)
    want = cr.cross_f32(lr.decode_f32(rec, SCALE, OFFSET, ZERO), seg, st, bs, bin, HW, ZTOL, LQ, PAINT, mask=_passes(rec, fmt, sel))[0]
    assert want[..., 0].sum() > 10
    d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])
    sst = sel.as_struct()

    def run(B, poisoned):
        s_rec = Slab(dev, 1, len(flat), front=1, back=1, dtype=torch.uint8).fill_input(torch.from_numpy(flat), 0xFF if poisoned else 0)
        s_seg, s_start, s_segs, s_st, s_bs = _table_slabs(dev, seg, start, segs, st, bs, poisoned)
        s_cells = Slab(dev, n_cells, 8, front=8, back=8, dtype=torch.int32).fill_canary()
        ins = (s_rec, s_seg, s_start, s_segs, s_st, s_bs)
        before = [s.bits().clone() for s in ins]
        rc = lib().lm_las_line_cross_records(_stream(dev), C.c_void_p(s_rec.ptr()), rl, fmt, n, d3(SCALE), d3(OFFSET), None,
                                             C.byref(sst), C.c_void_p(s_seg.ptr()), len(seg), C.byref(g), C.c_void_p(s_start.ptr()),
                                             C.c_void_p(s_segs.ptr()), HW, C.c_void_p(s_st.ptr()), C.c_void_p(s_bs.ptr()),
                                             C.c_void_p(host.ctypes.data), len(bs) - 1, bin, ZTOL, LQ, PAINT, 0, C.c_void_p(s_cells.ptr()), n_cells)
        assert rc == 0, lib().lm_last_error()
        torch.cuda.synchronize()
        for s, b in zip(ins, before):
            assert torch.equal(s.bits(), b), 'an input was written'
        return {'cells': (s_cells, n_cells)}

    for attempt in range(2):                                             # the second round: the same bits again
        got = guarded_runs(run, 'las_line_cross_records', batch=False)
        _same('guarded', _cells_of(got['cells'], nl), want)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_name_the_argument_and_write_nothing(dev, tmp_path):
    _, seg, pts = _scene()
    bin = pr.BIN_EXACT
    st, bs = _tables(bin)
    index, stations = _device_tables(dev, bin)
    nl = cr.hq_nl(HW, LQ)[1]
    n_cells, n = stations.n_bins * nl, 300
    rec, flat = _records(tmp_path, 1, 0, n, seed=1)
    d_rec = torch.from_numpy(flat).to(dev)
    d_pts = _t(pts[:n + 1]).to(dev)
    cells = torch.full((n_cells + nl, 4), POISON, dtype=torch.int64, device=dev)
    L = lib()
    d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])
    # positions: points 1, N 2, segments 3, grid 5, cell_start 6, cell_segs 7, half_width 8, stations 9, bin_start 10, bin_start_host 11,
    # L 12, bin 13, z_tol 14, lateral_q 15, paint_iq 16, accumulate 17, cells 18, n_cells 19; the record entry: the same from segments
    # on, six further back
    p_base = [_stream(dev), C.c_void_p(d_pts.data_ptr()), n, *index.args(), *stations.args(), ZTOL, LQ, PAINT, 0, C.c_void_p(cells.data_ptr()), n_cells]
    r_base = [_stream(dev), C.c_void_p(d_rec.data_ptr()), 28, 1, n, d3(SCALE), d3(OFFSET), None, None, *index.args(), *stations.args(),
              ZTOL, LQ, PAINT, 0, C.c_void_p(cells.data_ptr()), n_cells]
    assert len(p_base) == 20 and len(r_base) == 26
    assert L.lm_line_cross_points(*p_base) == 0 and L.lm_las_line_cross_records(*r_base) == 0, L.lm_last_error()
    torch.cuda.synchronize()
    assert bool((cells[n_cells:] == POISON).all()) and int(cells[:n_cells, 0].sum()) > 0
    cells.fill_(POISON)

    def refused(what, **change):
        """`change`: position in the points entry -> new value; applied to both entries (the record entry: position + 6 from 3 on)."""
        for name, fn, base, shift in (('line_cross_points', L.lm_line_cross_points, p_base, 0),
                                      ('las_line_cross_records', L.lm_las_line_cross_records, r_base, 6)):
            a = list(base)
            for pos, v in change.items():
                a[int(pos[1:]) + shift] = v
            rc = fn(*a)
            torch.cuda.synchronize()
            msg = L.lm_last_error().decode()
            assert rc == 1 and msg.startswith(name + ':') and what in msg, f'{name}, {what}: rc={rc}, message {msg!r}'
            assert bool((cells == POISON).all()), f'{name}, {what}: cells was written'

    off = lambda pos, by: {f'p{pos}': C.c_void_p(p_base[pos].value + by)}
    for pos, what, by in ((3, 'segments', 8), (6, 'cell_start', 1), (7, 'cell_segs', 2), (9, 'stations', 4), (10, 'bin_start', 2), (18, 'cells', 4)):
        refused(f'{what} is not', **off(pos, by))
    refused('cells is not 8-byte aligned', **off(18, 4))
    refused('stations', p9=None)
    refused('bin_start', p10=None)
    refused('bin_start_host', p11=None)
    refused('cells', p18=None)
    refused('segments', p3=None)
    # what the cross-section adds
    refused('lateral_q=0', p15=0)
    refused('lateral_q=-3', p15=-3)
    refused('paint_iq=-1', p16=-1)
    refused('paint_iq=65537', p16=65537)
    refused('n_cells', p19=n_cells + 1)
    refused('n_cells', p19=n_cells - nl)
    refused('n_cells', p15=LQ // 2)                                       # another lateral_q: another nl for the same n_cells
    refused('z_tol=16.5', p14=16.5)
    refused('z_tol', p14=float('inf'))
    refused('z_tol', p14=NAN)
    # the 2^27 cap: 2^20 bins of 1281 cells
    big = np.array([0, 1 << 20, 1 << 20, 1 << 20], np.int32)
    refused('at most 2^27', p11=C.c_void_p(big.ctypes.data), p15=1, p8=HW, p19=(1 << 20) * 641)
    # what the profile entries refuse
    short = np.array(bs[:2], np.int32)
    refused('segments carry lines', p11=C.c_void_p(short.ctypes.data), p12=1, p19=int(short[-1]) * nl)
    down = np.array(bs, np.int32)
    down[2] = down[1] - 1
    refused('bin_start[2]', p11=C.c_void_p(down.ctypes.data))
    late = np.array(bs, np.int32)
    late[0] = 1
    refused('bin_start[0]', p11=C.c_void_p(late.ctypes.data))
    wide = ops.line_index(seg, 0.25, device=dev)
    refused('half_width', p5=C.byref(wide.grid))
    other = ops.line_index(seg[:-1], HW, device=dev)
    refused('grid', p5=C.byref(other.grid))
    huge = ops.line_index(seg, 16.5, device=dev)
    ha = huge.args()
    refused('half_width=16.5', p3=ha[0], p5=ha[2], p6=ha[3], p7=ha[4], p8=16.5)
    for bad in (0.0, -0.125, NAN, float('inf')):
        refused('bin=', p13=bad)
    refused('accumulate', p17=2)
    refused('half_width', p8=-1.0)
    # what only one entry takes
    for pos, v, what in ((1, C.c_void_p(d_pts.data_ptr() + 4), 'points_xyzi is not'), (1, None, 'points_xyzi'), (2, -1, 'N=')):
        a = list(p_base)
        a[pos] = v
        assert L.lm_line_cross_points(*a) == 1 and what in L.lm_last_error().decode(), (what, L.lm_last_error())
    for pos, v, what in ((1, C.c_void_p(d_rec.data_ptr() + 1), 'records is not'), (1, None, 'records'), (2, 27, 'record_len'), (3, 11, 'point_format'),
                         (4, -1, 'n='), (5, None, 'scale')):
        a = list(r_base)
        a[pos] = v
        assert L.lm_las_line_cross_records(*a) == 1 and what in L.lm_last_error().decode(), (what, L.lm_last_error())
    torch.cuda.synchronize()
    assert bool((cells == POISON).all())
    # the package entries
    cross = CrossSection(PAINT, bin=bin, half_width=HW, z_tol=ZTOL)
    with pytest.raises(ValueError, match='half_width'):
        las_io.cross_records(d_rec, _header(1, 28, n), wide, stations, cross)
    with pytest.raises(ValueError, match='bin='):
        las_io.cross_records(d_rec, _header(1, 28, n), index, stations, CrossSection(PAINT, bin=0.5, half_width=HW))
    with pytest.raises(TypeError, match='CrossSection'):
        las_io.cross_records(d_rec, _header(1, 28, n), index, stations, las_io.MarkingSurvey())
    with pytest.raises(ValueError, match='lateral_q'):
        ops.line_cross(d_pts, index, stations, ZTOL, 0, PAINT)


# ------------------------------------------------------------------------------------------------ 6. a painted scene
def test_cross_files_reads_stripes_offset_and_crossfall_off_a_painted_scene(dev, tmp_path):
    """Two lines along +x, 12 m long with a vertex every 2 m, A at y = 2 and B at y = 5, z = 0, under the defaults (half_width 0.625 m,
    lateral_q 32: 41 cells of 1/32 m, bin 0.5 m).  Around each, returns on a lattice: x = 0.025 + 0.05 i (stored on the file's 1/1024 m
    grid: at least 0.02 m from every station border), lateral offsets o = (2 j + 1) / 128 m, j = -48 .. 47, so q = 8 (2 j + 1) is 8 or 24
    past a cell border (a multiple of 32) and float32 decides nothing; |o| <= 79/128 is inside the band, 81/128 is outside, neither near
    it.  Every cell 0 .. 39 of every station holds 2 x 10 returns, cell 40 none.  Paint (24000, else 3000) by the whole number j: A where
    0 <= j <= 9 - cells 20 .. 24, one stripe from 0 to 0.15625 m, centre 0.078125 m left; B where 6 <= j <= 15 or 26 <= j <= 35 - cells
    23 .. 27 and 33 .. 37, two stripes 5 cells apart, centre 0.328125 m: beyond max_shift = 0.3, so snap_lines leaves B where it is (the
    outlier rule) and moves A by exactly 10/128 m along +y.

    The surface is z = 0.025 o = (2 j + 1) / 5120 m, stored exactly on a z grid of 1/5120 m.  THE CROSS-FALL MARGIN.  Per station the
    table's fit is the n-weighted least-squares line through (x_c, m_c): x_c the centre of cell c, m_c = sum zq / n / 1024.  A return's
    zq / 1024 differs from its z - zl by at most d = (1/2) / 1024 m (rintf) plus the float32 rounding of z and of (z - zl) 1024, below
    2^-22 |z| < 4e-9 m here; so every m_c lies within d + 4e-9 of the cell's true mean height.  The slope is linear in the m_c:
    sum w_c (x_c - xbar) m_c / sum w_c (x_c - xbar)^2, so it moves by at most (d + 4e-9) sum w_c |x_c - xbar| / sum w_c (x_c - xbar)^2.
    The two returns of a cell lie symmetric about its centre (1/128 and 3/128 m into it) and the surface is linear, so with the true
    means the fit through the cell centres IS the float64 least-squares slope over the returns themselves - the cells add no error of
    their own.  With 40 cells of equal weight at x_c = (2 c - 39) / 64: sum |x_c| = 800 / 64 = 12.5, sum x_c^2 = 2 x 10660 / 4096 =
    5.2051, margin = 12.5 / 5.2051 / 2048 = 0.0011726 (+ 1e-8 for the 4e-9).  The median over stations of values within the margin lies
    within it."""
    cross = CrossSection(paint_intensity=10000)
    assert (cross.half_width, cross.lateral_q, cross.bin, cross.hq, cross.nl, cross.max_shift) == (0.625, 32, 0.5, 640, 41, 0.3)
    i, j = np.meshgrid(np.arange(240), np.arange(-48, 48), indexing='ij')
    i, j = i.ravel(), j.ravel()
    world, inten, paint_j = [], [], ((range(0, 10),), (range(6, 16), range(26, 36)))
    for y0, stripes in zip((2.0, 5.0), paint_j):
        world.append(np.stack([0.025 + 0.05 * i, y0 + (2 * j + 1) / 128.0, (2 * j + 1) / 5120.0], axis=1))
        inten.append(np.where(np.isin(j, np.concatenate([np.asarray(r) for r in stripes])), 24000, 3000))
    world, inten = np.concatenate(world) + lr.SHIFT, np.concatenate(inten)
    order = np.random.RandomState(11).permutation(len(world))
    half = len(order) // 2
    paths = []
    for k, part in enumerate((order[:half], order[half:])):
        paths.append(str(tmp_path / f'scene{k}.las'))
        las_ref.write_las(paths[k], world[part], inten[part], point_format=(1, 6)[k], version=((1, 2), (1, 4))[k], offset=tuple(lr.SHIFT),
                          scale=(1 / 1024, 1 / 1024, 1 / 5120))
    xs = np.arange(0.0, 14.0, 2.0)
    lines = [np.stack([xs, np.full_like(xs, y0), np.zeros_like(xs)], axis=1) + lr.SHIFT for y0 in (2.0, 5.0)]
    # the reference's own numbers first, on what the files hold
    seg = las_io.line_segments(lines, lr.SHIFT)
    st, bs = las_io.line_stations(lines, lr.SHIFT, cross.bin)
    assert bs.tolist() == [0, 24, 48]
    dec = []
    for path in paths:
        data = np.fromfile(path, np.uint8)
        h = las_io.parse_header(data)
        o, rl, n = h['offset_to_points'], h['record_len'], h['n_points']
        dec.append(lr.decode_f32(data[o:o + n * rl].reshape(n, rl), h['scale'], h['offset'], lr.SHIFT))
    dec = np.concatenate(dec)
    want, terms, lab, _ = cr.cross_f32(dec, seg, st, bs, cross.bin, cross.half_width, cross.z_tol, cross.lateral_q, cross.paint_iq)
    on = lab > 0
    assert on.sum() == 2 * 240 * 80 and (want[:, :40, 0] == 20).all() and (want[:, 40] == 0).all()
    assert set(np.unique(terms['q'][on] % 32)) == {8, 24}
    frac = (dec[:, 0].astype(np.float64) / 0.5) % 1.0
    assert (np.minimum(frac, 1 - frac) * 0.5 > 0.02).all()
    assert (want[:24, 20:25, 1] == 20).all() and want[:24, :, 1].sum() == 24 * 5 * 20 and want[24:, :, 1].sum() == 24 * 10 * 20
    # the table and the summary
    cells, bin_start = las_io.cross_files([(p, lr.SHIFT, None) for p in paths], lines, cross, device=dev)
    assert bin_start.tolist() == [0, 24, 48]
    _same('cross_files', cells, want)
    got = las_io.cross_summary(cells, bin_start, cross)
    assert got == cr.summary_of(want, bs, cross) and len(got) == 2
    a, b = got
    assert a['stations'] == 24 and a['stripes'] == 1 and a['double'] is False and a['width'] == 0.15625 and a['offset'] == 0.078125
    assert a['separation'] is None and a['extent'] == 0.15625 and a['centres'] == [0.078125] * 24
    assert b['stations'] == 24 and b['stripes'] == 2 and b['double'] is True and b['separation'] == 0.15625 and b['width'] == 0.15625
    assert b['offset'] == 0.328125 and b['extent'] == 0.46875
    # the cross-fall against the float64 least squares over the returns themselves
    xc = (2 * np.arange(40) - 39) / 64.0
    margin = (0.5 / 1024 + 4e-9) * np.abs(xc).sum() / (xc * xc).sum()
    assert abs(margin - 0.0011726) < 1e-6
    for k, m in enumerate(got):
        sel = lab == k + 1
        o = dec[sel, 1].astype(np.float64) - (2.0, 5.0)[k]
        z = dec[sel, 2].astype(np.float64)
        direct = ((o - o.mean()) * (z - z.mean())).sum() / ((o - o.mean()) ** 2).sum()
        print(f'line {k + 1}: crossfall {m["crossfall"]!r}, float64 least squares over the returns {direct!r}, margin {margin!r}')
        assert abs(direct - 0.025) < 1e-8 and abs(m['crossfall'] - direct) <= margin
    # the snapped lines
    snapped = las_io.snap_lines(lines, got, bin_start, cross)
    assert all(np.array_equal(x, y) for x, y in zip(snapped, cr.snap_of(lines, got, bin_start, cross)))
    assert np.array_equal(snapped[0], lines[0] + np.array([0.0, 0.078125, 0.0])) and np.array_equal(snapped[1], lines[1])
    # no file: the empty table of the lines
    none, bs0 = las_io.cross_files([], lines, cross, device=dev)
    assert none.shape == (48, 41, 4) and not none.any() and bs0.tolist() == [0, 24, 48]


# ------------------------------------------------------------------------------------------------ 7. Runner
def _strip(tmp_path):
    """The strip of tests/test_gpu_profile.py's Runner test (a copy of its generator): three overlapping 1152 x 1152 tiles over a climbing
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


def test_runner_strip_takes_cross_sections_of_its_lines(dev, net, tmp_path):
    """Runner.infer_las_strip_to_map with cross=CrossSection(10000): params/cross_sections.npy equals the brute force against the lines
    the call returned, cross_sections.json is cross_summary of it, merged_snapped.txt is save_seqs_list of snap_lines; the return value
    and merged.txt equal the plain call's, which writes none of the four files."""
    from lanemapping_amd.runner import Runner
    las, prm_paths, off = _strip(tmp_path)
    rn = Runner.__new__(Runner)
    rn.cfg, rn.device, rn.net = net.cfg, dev, net
    assert rn.cfg.get('las_cross') is None
    out = {k: str(tmp_path / k) for k in ('plain', 'cross')}
    plain = rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['plain'], batch_size=2)
    cross = CrossSection(paint_intensity=10000.0)
    lines3d, merged = rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['cross'], batch_size=2, cross=cross)
    assert sorted(plain[0]) == sorted(lines3d) and len(plain[1]) == len(merged) and all(np.array_equal(a, b) for a, b in zip(plain[1], merged))
    assert all(len(plain[0][k]) == len(lines3d[k]) and all(np.array_equal(a, b) for a, b in zip(plain[0][k], lines3d[k])) for k in lines3d)
    new = [os.path.join('params', 'cross_sections.npy'), os.path.join('params', 'cross_sections.json'),
           os.path.join('out_pc_seq_json_dir', 'merged_snapped.txt'), os.path.join('out_pc_seq_json_dir', 'merged_snapped_downsample.txt')]
    for name in new:
        assert not os.path.exists(os.path.join(out['plain'], name)) and os.path.exists(os.path.join(out['cross'], name)), name
    pc = os.path.join('out_pc_seq_json_dir', 'merged.txt')
    assert open(os.path.join(out['plain'], pc), 'rb').read() == open(os.path.join(out['cross'], pc), 'rb').read()
    lines = list(merged) if len(merged) else [l for name in sorted(lines3d) for l in lines3d[name]]
    assert lines, 'the strip yielded no lines'
    data = np.fromfile(las, np.uint8)
    h = las_io.parse_header(data)
    o, rl, n = h['offset_to_points'], h['record_len'], h['n_points']
    rec = data[o:o + n * rl].reshape(n, rl)
    seg = las_io.line_segments(lines, off)
    st, bs = las_io.line_stations(lines, off, cross.bin)
    want, _, line, _ = cr.cross_f32(lr.decode_f32(rec, h['scale'], h['offset'], off), seg, st, bs, cross.bin, cross.half_width, cross.z_tol,
                                    cross.lateral_q, cross.paint_iq, pruned=True)
    got = np.load(os.path.join(out['cross'], new[0]))
    _same('cross_sections.npy', got, want)
    used = json.load(open(os.path.join(out['cross'], new[1])))
    summary = las_io.cross_summary(want, bs, cross)
    assert used == json.loads(json.dumps({str(k + 1): m for k, m in enumerate(summary)})) and len(used) == len(lines)
    assert summary == cr.summary_of(want, bs, cross)
    snapped = las_io.snap_lines(lines, summary, bs, cross)
    io_utils.save_seqs_list(snapped, str(tmp_path / 'expect.txt'))
    assert open(str(tmp_path / 'expect.txt'), 'rb').read() == open(os.path.join(out['cross'], new[2]), 'rb').read()
    painted = sum(m['stations'] for m in summary)
    moved = sum(int((a[:, :2] != b[:, :2]).any(axis=1).sum()) for a, b in zip(snapped, lines))
    print(f'{len(lines)} lines, {len(seg)} segments, {int(bs[-1])} station bins x {cross.nl} cells, {painted} painted stations, '
          f'{int((line > 0).sum())} of {n} records in the table, {moved} vertices moved; stripes {[m["stripes"] for m in summary]}, '
          f'offsets {[m["offset"] for m in summary]}, crossfall {[m["crossfall"] for m in summary]}')
    assert painted > 0, 'no station is painted: the test shows nothing'
    assert all(np.array_equal(a[:, 2], b[:, 2]) for a, b in zip(snapped, lines))
