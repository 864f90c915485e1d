"""GPU: the paint no lane line explains (csrc/residue.hip: lm_residue_keys, lm_cell_components, lm_residue_stats; ops.paint_residue /
cell_components, las_io.residue_files / residue_summary, Runner `residue=`).

The reference is tests/residue_ref.py: the float32 rule by brute force over all segments, the components by scipy.ndimage.label and by a
plain Python union-find (which must agree), the statistics in Python integers.  Keys, roots and statistics are compared in every
integer."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import label_ref as lr
import residue_ref as rr
from guards import Slab, guarded_runs
from lanemapping_amd import las_io, ops
from lanemapping_amd._lib import LanemapHipError, lib
from lanemapping_amd.las_io import PaintResidue
from oracle import las_ref

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float('nan')
CHUNK = 1024                                   # points per workgroup of residue_keys_kernel (csrc/residue.hip: CHUNK = 256 * PER)
BIG = 0x7FFFFFF0


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def _scene():
    """-> (segments, points, first, host grid of the index, residue grid, reference keys, reference iq): computed once, never changed."""
    seg = las_io.line_segments([l + lr.SHIFT for l in lr.scene_lines()], lr.SHIFT)
    g, start, segs = ops.line_index_host(seg, rr.REACH)
    host = ops.LineIndex(torch.from_numpy(np.array(seg)), torch.from_numpy(start), torch.from_numpy(segs), g, f32(rr.REACH))
    grid = ops.residue_grid(host, rr.CELL)
    pts, first = rr.scene_points(seg, (g.x0, g.y0, g.cell, g.nx, g.ny))
    key, iq = rr.keys_f32(pts, seg, rr.REACH, rr.ZTOL, rr.MIN_I, rr.CLEAR, grid)
    for a in (seg, pts, key, iq, start, segs):
        a.setflags(write=False)
    return seg, pts, first, (g, start, segs), grid, key, iq


@functools.lru_cache(maxsize=None)
def _cell_scenes():
    """{name: (keys, nx, ny, {connectivity: reference roots})}: computed once."""
    out = {}
    for name, (keys, nx, ny) in rr.cell_scenes().items():
        keys.setflags(write=False)
        out[name] = (keys, nx, ny, {c: rr.roots(keys, nx, c) for c in (4, 8)})
    return out


def _t(a):
    return torch.from_numpy(np.array(a, copy=True))


def _keys_call(dev, pts, index, grid, N):
    key, iq = ops.residue_keys(pts[:N], index, rr.ZTOL, rr.MIN_I, rr.CLEAR, grid)
    return key.cpu().numpy(), iq.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. keys
def test_keys_equal_the_float32_brute_force(dev):
    seg, pts, first, _, grid, key, iq = _scene()
    assert (key >= 0).sum() > 2000 and (key < 0).sum() > 500 and len(pts) > 2 * CHUNK
    assert key[first + rr.AT_REACH] >= 0 and key[first + rr.PAST_REACH] < 0 and key[first + rr.AT_ZTOL] >= 0 and key[first + rr.PAST_ZTOL] < 0
    assert all(key[i] < 0 for i in rr.AT_CLEAR) and key[first + rr.AT_MIN_I] >= 0 and key[first + rr.BELOW_MIN_I] < 0 and key[first + rr.NAN_I] < 0
    index = ops.line_index(seg, rr.REACH, device=dev)
    assert ops.residue_grid(index, rr.CELL) == grid
    d_pts = _t(pts).to(dev)
    for N in (1, 63, 64, 65, 255, 256, 257, CHUNK + 1, len(pts)):
        k, q = _keys_call(dev, d_pts, index, grid, N)
        assert np.array_equal(k, key[:N]), f'N={N}: {int((k != key[:N]).sum())} keys differ from the float32 brute force'
        assert np.array_equal(q, iq[:N]), f'N={N}: {int((q != iq[:N]).sum())} iq differ'
    # the special points and the bars alone (another alignment of the same points), and the same bits on a second run
    k, q = _keys_call(dev, d_pts[first:].contiguous(), index, grid, len(pts) - first)
    assert np.array_equal(k, key[first:]) and np.array_equal(q, iq[first:])
    k, q = _keys_call(dev, d_pts, index, grid, len(pts))
    assert np.array_equal(k, key) and np.array_equal(q, iq)
    # iq = NULL
    k = ops.residue_keys(d_pts, index, rr.ZTOL, rr.MIN_I, rr.CLEAR, grid, want_iq=False)
    assert k[1] is None and np.array_equal(k[0].cpu().numpy(), key)
    # no segments (S = 0): every key -1; no points
    empty = ops.line_index(np.zeros((0, 8), f32), rr.REACH, device=dev)
    k0, q0 = ops.residue_keys(d_pts, empty, rr.ZTOL, rr.MIN_I, rr.CLEAR, ops.residue_grid(empty, rr.CELL))
    assert bool((k0 == -1).all()) and not bool(q0.any())
    k0, q0 = ops.residue_keys(d_pts[:0], index, rr.ZTOL, rr.MIN_I, rr.CLEAR, grid)
    assert k0.shape == (0,) and q0.shape == (0,)


# ------------------------------------------------------------------------------------------------ 2. components
@pytest.mark.parametrize('connectivity', [8, 4])
def test_roots_equal_the_reference(dev, connectivity):
    scenes = _cell_scenes()
    assert sorted(len(v[0]) for k, v in scenes.items() if k.startswith('random[')) == [0, 1, 63, 64, 65, 257]
    assert len(scenes['serpentine'][0]) > 2000 and len(scenes['random'][0]) > 3000
    for name, (keys, nx, ny, want) in scenes.items():
        d_keys = _t(keys).to(dev)
        root, err = ops.cell_components(d_keys, nx, ny, connectivity)
        got = root.cpu().numpy()
        assert int(err) == 0, f'{name}: a loop cap ran out'
        assert got.dtype == np.int32 and np.array_equal(got, want[connectivity]), \
            f'{name}, {connectivity}-connectivity: {int((got != want[connectivity]).sum())} of {len(keys)} roots differ from the reference'
        again, err = ops.cell_components(d_keys, nx, ny, connectivity)
        assert int(err) == 0 and torch.equal(again, root), f'{name}: a second run gives other bits'
    want = scenes['diagonal'][3]
    assert len(np.unique(want[8])) == 1 and len(np.unique(want[4])) == 2
    keys, nx, _, want = scenes['row_wrap']
    assert keys[1] == keys[0] + 1 and want[8][1] == 1 and want[4][1] == 1


# ------------------------------------------------------------------------------------------------ 3. statistics
@pytest.mark.parametrize('connectivity', [8, 4])
def test_stats_equal_the_python_integers(dev, connectivity):
    for name, (keys, nx, ny, roots) in _cell_scenes().items():
        n, s = rr.point_counts(keys)
        comp, K = rr.dense_ids(roots[connectivity])
        want = rr.stats(keys, nx, comp, K, n, s)
        got = ops.residue_stats(_t(comp).to(dev), _t(keys).to(dev), nx, ny, _t(n).to(dev), _t(s).to(dev), K).cpu().numpy()
        assert got.shape == (K, 12) and np.array_equal(got, want), f'{name}, {connectivity}: {int((got != want).sum())} statistics differ'


def test_paint_residue_does_not_depend_on_the_order_or_the_split_of_the_clouds(dev):
    seg, pts, first, _, grid, key, iq = _scene()
    cells, comp, st = rr.blobs([key], [iq], grid['nx'], 8)
    assert len(st) >= 3 and (st[:, 0] >= 20).sum() >= 3
    index = ops.line_index(seg, rr.REACH, device=dev)
    d_pts = _t(pts).to(dev)
    perm = torch.from_numpy(np.random.RandomState(7).permutation(len(pts))).to(dev)
    third = len(pts) // 3
    for tag, clouds in (('one cloud', [d_pts]), ('permuted', [d_pts[perm].contiguous()]),
                        ('three clouds', [d_pts[2 * third:].contiguous(), d_pts[:third].contiguous(), d_pts[third:2 * third].contiguous()]),
                        ('with an empty cloud', [d_pts[:0], d_pts])):
        got = ops.paint_residue(clouds, index, rr.ZTOL, rr.MIN_I, rr.CLEAR, rr.CELL).numpy()
        assert got.grid == grid
        assert np.array_equal(got.cells[:, 1].astype(np.int64) * grid['nx'] + got.cells[:, 0], cells), f'{tag}: the cells differ'
        assert np.array_equal(got.comp, comp) and got.comp.dtype == np.int32, f'{tag}: the components differ'
        assert np.array_equal(got.stats, st), f'{tag}: {int((got.stats != st).sum())} statistics differ from the Python integers'
    four = ops.paint_residue([d_pts], index, rr.ZTOL, rr.MIN_I, rr.CLEAR, rr.CELL, connectivity=4).numpy()
    assert np.array_equal(four.stats, rr.blobs([key], [iq], grid['nx'], 4)[2]) and len(four.stats) >= len(st)
    none = ops.paint_residue([], index, rr.ZTOL, rr.MIN_I, rr.CLEAR, rr.CELL).numpy()
    assert none.cells.shape == (0, 2) and none.comp.shape == (0,) and none.stats.shape == (0, 12)
    with pytest.raises(ValueError, match='connectivity'):
        ops.paint_residue([d_pts], index, rr.ZTOL, rr.MIN_I, rr.CLEAR, rr.CELL, connectivity=3)
    with pytest.raises(TypeError, match='LineIndex'):
        ops.paint_residue([d_pts], seg, rr.ZTOL, rr.MIN_I, rr.CLEAR)


# ------------------------------------------------------------------------------------------------ 4. guarded buffers
def _i64_slab(dev, data, pad):
    """An int64 operand between guards, as a Slab of int32 pairs."""
    data = np.ascontiguousarray(data, np.int64)
    return Slab(dev, len(data), 2, front=4, back=4, dtype=torch.int32).fill_input(_t(data.view(np.int32).reshape(len(data), 2)), pad)


def _i64(t):
    return np.ascontiguousarray(t.numpy()).view(np.int64).reshape(t.shape[0], -1)


@pytest.mark.parametrize('N', [65, 257, CHUNK + 1])
def test_residue_keys_guards(dev, N):
    """lm_residue_keys with the points, the segment table, the two lists, key and iq each between guard slabs: N one past a wave, one
    past a workgroup's threads and one past a workgroup's share."""
    seg, pts, first, (g, start, segs), grid, key, iq = _scene()
    sl = slice(first, first + N)
    assert (key[sl] >= 0).sum() > N // 4 and (key[sl] < 0).sum() >= 5

    def run(B, poisoned):
        s_pts = Slab(dev, N, 4, front=8, back=8).fill_input(_t(pts[sl]), NAN if poisoned else 0.0)
        s_seg = Slab(dev, len(seg), 8, front=4, back=4).fill_input(_t(seg), NAN if poisoned else 0.0)
        s_start = Slab(dev, 1, len(start), front=1, back=1, dtype=torch.int32).fill_input(_t(start), BIG if poisoned else 0)
        s_segs = Slab(dev, 1, len(segs), front=1, back=1, dtype=torch.int32).fill_input(_t(segs), BIG if poisoned else 0)
        s_key = Slab(dev, N, 2, front=4, back=4, dtype=torch.int32).fill_canary()
        s_iq = Slab(dev, 1, N, front=1, back=1, dtype=torch.int32).fill_canary()
        ins = (s_pts, s_seg, s_start, s_segs)
        before = [s.bits().clone() for s in ins]
        rc = lib().lm_residue_keys(_stream(dev), C.c_void_p(s_pts.ptr()), N, C.c_void_p(s_seg.ptr()), len(seg), C.byref(g),
                                   C.c_void_p(s_start.ptr()), C.c_void_p(s_segs.ptr()), rr.REACH, rr.ZTOL, rr.MIN_I, rr.CLEAR, grid['cell'],
                                   grid['nx'], grid['ny'], C.c_void_p(s_key.ptr()), C.c_void_p(s_iq.ptr()))
        assert rc == 0, lib().lm_last_error()
        torch.cuda.synchronize()
        for s, b in zip(ins, before):
            assert torch.equal(s.bits(), b), 'an input was written'
        return {'key': (s_key, N), 'iq': (s_iq, 1)}

    got = guarded_runs(run, 'residue_keys', batch=False)
    assert np.array_equal(_i64(got['key'])[:, 0], key[sl]) and np.array_equal(got['iq'].numpy()[0], iq[sl])


@pytest.mark.parametrize('M', [65, 257])
def test_cell_components_guards(dev, M):
    """lm_cell_components with keys, root and err between guard slabs: M one past a wave and one past a workgroup."""
    keys, nx, ny, _ = _cell_scenes()['random']
    keys = keys[:M]
    want = rr.roots(keys, nx, 8)
    assert len(np.unique(want)) < M

    def run(B, poisoned):
        s_keys = _i64_slab(dev, keys, BIG if poisoned else 0)
        s_root = Slab(dev, 1, M, front=1, back=1, dtype=torch.int32).fill_canary()
        s_err = Slab(dev, 1, 1, front=8, back=8, dtype=torch.int32).fill_canary()
        before = s_keys.bits().clone()
        rc = lib().lm_cell_components(_stream(dev), C.c_void_p(s_keys.ptr()), M, nx, ny, 8, C.c_void_p(s_root.ptr()), C.c_void_p(s_err.ptr()))
        assert rc == 0, lib().lm_last_error()
        torch.cuda.synchronize()
        assert torch.equal(s_keys.bits(), before), 'keys was written'
        return {'root': (s_root, 1), 'err': (s_err, 1)}

    got = guarded_runs(run, 'cell_components', batch=False)
    assert np.array_equal(got['root'].numpy()[0], want) and int(got['err'][0, 0]) == 0


@pytest.mark.parametrize('M', [65, 257])
def test_residue_stats_guards(dev, M):
    """lm_residue_stats with comp, keys, cell_points, cell_iq and stats between guard slabs: M one past a wave and one past a workgroup."""
    keys, nx, ny, _ = _cell_scenes()['random']
    keys = keys[:M]
    comp, K = rr.dense_ids(rr.roots(keys, nx, 8))
    n, s = rr.point_counts(keys)
    want = rr.stats(keys, nx, comp, K, n, s)

    def run(B, poisoned):
        pad = BIG if poisoned else 0
        s_comp = Slab(dev, 1, M, front=1, back=1, dtype=torch.int32).fill_input(_t(comp), pad)
        s_keys, s_n, s_s = _i64_slab(dev, keys, pad), _i64_slab(dev, n, pad), _i64_slab(dev, s, pad)
        s_stats = Slab(dev, K, 24, front=2, back=2, dtype=torch.int32).fill_canary()
        ins = (s_comp, s_keys, s_n, s_s)
        before = [x.bits().clone() for x in ins]
        rc = lib().lm_residue_stats(_stream(dev), C.c_void_p(s_comp.ptr()), C.c_void_p(s_keys.ptr()), nx, ny, C.c_void_p(s_n.ptr()),
                                    C.c_void_p(s_s.ptr()), M, K, C.c_void_p(s_stats.ptr()))
        assert rc == 0, lib().lm_last_error()
        torch.cuda.synchronize()
        for x, b in zip(ins, before):
            assert torch.equal(x.bits(), b), 'an input was written'
        return {'stats': (s_stats, K)}

    got = guarded_runs(run, 'residue_stats', batch=False)
    assert np.array_equal(_i64(got['stats']), want)


def test_device_tables_the_host_cannot_check_stay_in_bounds(dev):
    """Unsorted and duplicate keys, keys outside the grid and component ids outside [0, K): garbage in root and stats, nothing outside
    them, and the calls end."""
    M, nx, ny, K = 257, 96, 96, 5
    rng = np.random.RandomState(3)
    keys = rng.randint(-50, nx * ny + 50, M).astype(np.int64)
    keys[10:20] = keys[30]
    comp = rng.randint(-3, K + 3, M).astype(np.int32)
    s_keys = _i64_slab(dev, keys, BIG)
    s_comp = Slab(dev, 1, M, front=1, back=1, dtype=torch.int32).fill_input(_t(comp), BIG)
    s_n = _i64_slab(dev, np.ones(M, np.int64), BIG)
    s_root = Slab(dev, 1, M, front=1, back=1, dtype=torch.int32).fill_canary()
    s_err = Slab(dev, 1, 1, front=8, back=8, dtype=torch.int32).fill_canary()
    s_stats = Slab(dev, K, 24, front=2, back=2, dtype=torch.int32).fill_canary()
    L = lib()
    assert L.lm_cell_components(_stream(dev), C.c_void_p(s_keys.ptr()), M, nx, ny, 8, C.c_void_p(s_root.ptr()), C.c_void_p(s_err.ptr())) == 0
    assert L.lm_residue_stats(_stream(dev), C.c_void_p(s_comp.ptr()), C.c_void_p(s_keys.ptr()), nx, ny, C.c_void_p(s_n.ptr()),
                              C.c_void_p(s_n.ptr()), M, K, C.c_void_p(s_stats.ptr())) == 0
    torch.cuda.synchronize()
    for name, s in (('root', s_root), ('err', s_err), ('stats', s_stats)):
        s.check_canary(name)
    root = s_root.view.cpu().numpy()[0]
    assert (root >= 0).all() and (root <= np.arange(M)).all() and int(s_err.view[0, 0]) == 0
    st = _i64(s_stats.view.cpu())
    ok = (comp >= 0) & (comp < K) & (keys >= 0) & (keys < nx * ny)
    assert st[:, 0].tolist() == np.bincount(comp[ok], minlength=K).tolist()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_name_the_argument_and_write_nothing(dev):
    seg, pts, first, _, grid, _, _ = _scene()
    index = ops.line_index(seg, rr.REACH, device=dev)
    L = lib()
    n = 300
    d_pts = _t(pts[:n + 1]).to(dev)
    key = torch.full((n + 1,), -77, dtype=torch.int64, device=dev)
    iq = torch.full((n + 1,), 0x7EADBEEF, dtype=torch.int32, device=dev)

    def refused(what, rc, outs):
        torch.cuda.synchronize()
        msg = L.lm_last_error().decode()
        assert rc == 1 and what in msg, f'{what}: rc={rc}, message {msg!r}'
        for t, v in outs:
            assert bool((t == v).all()), f'{what}: an output was written'

    kbase = [_stream(dev), _p(d_pts), n, *index.args(), rr.ZTOL, rr.MIN_I, rr.CLEAR, grid['cell'], grid['nx'], grid['ny'], _p(key), _p(iq)]
    kouts = ((key, -77), (iq, 0x7EADBEEF))
    #           0       1     2  3    4  5     6           7          8      9      10     11     12    13  14  15   16
    for pos, value, what in ((10, NAN, 'min_intensity'), (10, float('inf'), 'min_intensity'), (11, rr.REACH, 'clear'), (11, 2.0, 'clear'),
                             (11, -0.5, 'clear'), (11, NAN, 'clear'), (13, (1 << 20) + 1, 'nx'), (14, (1 << 20) + 1, 'ny'), (13, -1, 'nx'),
                             (12, 0.0, 'cell'), (12, NAN, 'cell'), (9, NAN, 'z_tol'), (2, -1, 'N=')):
        a = list(kbase)
        a[pos] = value
        refused(f'residue_keys: {what}', L.lm_residue_keys(*a), kouts)
    a = list(kbase)
    a[13] = 1 << 20                                                             # (2^20 itself is fine)
    assert L.lm_residue_keys(*a) == 0, L.lm_last_error()
    key.fill_(-77), iq.fill_(0x7EADBEEF)
    # a grid built for another half_width (reach), a reach above 16
    for hw, what in ((2.0, 'half_width'), (17.0, 'half_width')):
        other = ops.line_index(seg, hw, device=dev)
        a = list(kbase)
        a[3:9] = other.args()
        a[8] = rr.REACH if hw == 2.0 else hw
        refused(f'residue_keys: {what}' if hw == 17.0 else what, L.lm_residue_keys(*a), kouts)
    # misaligned buffers, each named alone; null buffers
    for pos, what, by in ((1, 'points_xyzi', 4), (15, 'key', 4), (16, 'iq', 2), (3, 'segments', 8), (6, 'cell_start', 1), (7, 'cell_segs', 2)):
        a = list(kbase)
        a[pos] = C.c_void_p(a[pos].value + by)
        refused(f'residue_keys: {what} is not', L.lm_residue_keys(*a), kouts)
    for pos in (1, 15):
        a = list(kbase)
        a[pos] = None
        refused('residue_keys: null pointer', L.lm_residue_keys(*a), kouts)

    keys, nx, ny, _ = _cell_scenes()['random']
    M = 300
    d_keys = _t(keys[:M + 1]).to(dev)
    root = torch.full((M + 1,), 0x7EADBEEF, dtype=torch.int32, device=dev)
    err = torch.full((2,), 0x7EADBEEF, dtype=torch.int32, device=dev)
    cbase = [_stream(dev), _p(d_keys), M, nx, ny, 8, _p(root), _p(err)]
    couts = ((root, 0x7EADBEEF), (err, 0x7EADBEEF))
    for pos, value, what in ((5, 3, 'connectivity=3'), (5, 0, 'connectivity'), (3, (1 << 20) + 1, 'nx'), (4, (1 << 20) + 1, 'ny'), (2, -1, 'M='),
                             (1, None, 'null pointer'), (6, None, 'null pointer'), (7, None, 'null pointer')):
        a = list(cbase)
        a[pos] = value
        refused(f'cell_components: {what}', L.lm_cell_components(*a), couts)
    for pos, what, by in ((1, 'keys', 4), (6, 'root', 2), (7, 'err', 2)):
        a = list(cbase)
        a[pos] = C.c_void_p(a[pos].value + by)
        refused(f'cell_components: {what} is not', L.lm_cell_components(*a), couts)
    with pytest.raises(LanemapHipError, match='connectivity=3'):
        ops.cell_components(d_keys, nx, ny, 3)

    comp = torch.zeros((M + 1,), dtype=torch.int32, device=dev)
    cnt = torch.ones((M + 1,), dtype=torch.int64, device=dev)
    stats = torch.full((4 * 12 + 1,), -77, dtype=torch.int64, device=dev)
    sbase = [_stream(dev), _p(comp), _p(d_keys), nx, ny, _p(cnt), _p(cnt), M, 4, _p(stats)]
    souts = ((stats, -77),)
    for pos, value, what in ((3, (1 << 20) + 1, 'nx'), (4, (1 << 20) + 1, 'ny'), (7, (1 << 22) + 1, 'M='), (7, -1, 'M='), (8, M + 1, 'K='),
                             (8, -1, 'K='), (1, None, 'null pointer'), (2, None, 'null pointer'), (5, None, 'null pointer'),
                             (6, None, 'null pointer'), (9, None, 'null pointer')):
        a = list(sbase)
        a[pos] = value
        refused(f'residue_stats: {what}', L.lm_residue_stats(*a), souts)
    for pos, what, by in ((1, 'comp', 2), (2, 'keys', 4), (5, 'cell_points', 4), (6, 'cell_iq', 4), (9, 'stats', 4)):
        a = list(sbase)
        a[pos] = C.c_void_p(a[pos].value + by)
        refused(f'residue_stats: {what} is not', L.lm_residue_stats(*a), souts)


# ------------------------------------------------------------------------------------------------ 6. end to end
SCALE, OFFSET = (0.001, 0.001, 0.001), tuple(lr.SHIFT + [3.0, -2.0, 0.5])
BAR, STRIPE = (10.0, 10.4, 0.4, 2.8), (20.0, 26.0, 4.45, 4.6)             # x0, x1, y0, y1 (shifted frame)


def _road(tmp_path):
    """Two lines along x, 3.5 m apart, with their paint; asphalt below the threshold; a bar of 0.4 m x 2.4 m between the lines, across them
    and nearer to line 1; a stripe of 6 m x 0.15 m along line 2, its centre 1.025 m to the left; a bright sign 3 m above the road.  Two
    files, the points dealt at random.  -> (paths, lines in the LAS frame)."""
    rng = np.random.RandomState(40)
    xs = np.arange(0.0, 42.0, 2.0)
    lines = [np.stack([xs, np.full_like(xs, y), np.zeros_like(xs)], axis=1) + lr.SHIFT for y in (0.0, 3.5)]
    lattice = lambda x0, x1, y0, y1, h=0.02: np.stack(np.meshgrid(np.arange(x0 + h / 2, x1, h), np.arange(y0 + h / 2, y1, h)), axis=-1).reshape(-1, 2)
    parts = [(np.stack([rng.uniform(0, 40, 6000), rng.uniform(-3, 7, 6000)], axis=1), 0.0, (300, 2000))]
    parts += [(lattice(0.0, 40.0, y - 0.075, y + 0.075, 0.05), 0.0, (20000, 26000)) for y in (0.0, 3.5)]
    parts += [(lattice(*BAR), 0.0, (20000, 26000)), (lattice(*STRIPE), 0.0, (20000, 26000)), (lattice(30.0, 30.5, 1.0, 2.0), 3.0, (30000, 31000))]
    xyz = np.concatenate([np.concatenate([xy, np.full((len(xy), 1), z)], axis=1) for xy, z, _ in parts])
    inten = np.concatenate([rng.randint(lo, hi, len(xy)) for xy, _, (lo, hi) in parts])
    deal = rng.rand(len(xyz)) < 0.5
    paths = []
    for k, on in enumerate((deal, ~deal)):
        paths.append(str(tmp_path / f'road{k}.las'))
        las_ref.write_las(paths[k], xyz[on] + lr.SHIFT, inten[on], point_format=1, scale=SCALE, offset=OFFSET)
    return paths, lines


def _decoded(path, shift):
    data = np.fromfile(path, np.uint8)
    h = las_io.parse_header(data)
    o, rl, n = h['offset_to_points'], h['record_len'], h['n_points']
    return lr.decode_f32(data[o:o + n * rl].reshape(n, rl), h['scale'], h['offset'], shift)


def test_residue_files_find_the_bar_and_the_stripe(dev, tmp_path):
    paths, lines = _road(tmp_path)
    res = PaintResidue(min_intensity=10000.0)
    blobs = las_io.residue_files([(p, lr.SHIFT, None) for p in paths], lines, res, device=dev)
    out = las_io.residue_summary(blobs, lines, res)
    # every integer against the reference on the decoded records
    seg = las_io.line_segments(lines, lr.SHIFT)
    ref = [rr.keys_f32(_decoded(p, lr.SHIFT), seg, res.reach, res.z_tol, res.min_intensity, res.clear, blobs.grid) for p in paths]
    cells, comp, st = rr.blobs([k for k, _ in ref], [q for _, q in ref], blobs.grid['nx'], 8)
    assert np.array_equal(blobs.cells[:, 1].astype(np.int64) * blobs.grid['nx'] + blobs.cells[:, 0], cells)
    assert np.array_equal(blobs.comp, comp) and np.array_equal(blobs.stats, st)
    # the bar and the stripe, nothing else: no sign, no paint of the lines themselves
    assert len(out) == 2 and len(st) == 2, [(b['centre'], b['cells']) for b in out]
    bar, stripe = sorted(out, key=lambda b: b['centre'][0])
    cell = res.cell
    c = np.array(bar['centre']) - lr.SHIFT[:2]
    assert abs(c[0] - 10.2) <= cell and abs(c[1] - 1.6) <= cell
    assert bar['shape'] == 'across' and abs(bar['length'] - 2.4) <= cell + 1e-9 and abs(bar['width'] - 0.4) <= cell + 1e-9 and bar['line'] == 1
    assert abs(bar['offset'] - 1.6) <= cell and bar['fill'] > 0.9 and 20000 <= bar['intensity'] < 26000
    c = np.array(stripe['centre']) - lr.SHIFT[:2]
    assert abs(c[0] - 23.0) <= cell and abs(c[1] - 4.525) <= cell
    assert stripe['shape'] == 'along' and abs(stripe['length'] - 6.0) <= cell + 1e-9 and stripe['line'] == 2 and abs(stripe['offset'] - 1.025) <= cell
    assert stripe['width'] <= 0.15 + 2 * cell
    # the files in the other order: the same bits; one file alone: fewer points in the same blobs
    again = las_io.residue_files([(p, lr.SHIFT, None) for p in paths[::-1]], lines, res, device=dev)
    assert np.array_equal(again.stats, blobs.stats) and np.array_equal(again.cells, blobs.cells) and np.array_equal(again.comp, blobs.comp)
    # no lines: nothing
    none = las_io.residue_files([(p, lr.SHIFT, None) for p in paths], [], res, device=dev)
    assert none.stats.shape == (0, 12) and none.cells.shape == (0, 2) and las_io.residue_summary(none, [], res) == []


def test_runner_strip_writes_the_residue(dev, net, tmp_path):
    """The strip of tests/test_gpu_profile.py's Runner test through Runner.infer_las_strip_to_map with residue=PaintResidue(...):
    params/residue.npy, residue_cells.npy and residue.json hold the reference's integers against the lines the call returned and
    residue_summary of them; the same call without residue= writes none of the three and returns the same lines, bit for bit."""
    from lanemapping_amd.runner import Runner
    from test_gpu_profile import _strip
    las, prm_paths, off = _strip(tmp_path)
    rn = Runner.__new__(Runner)
    rn.cfg, rn.device, rn.net = net.cfg, dev, net
    assert rn.cfg.get('las_residue') is None
    out = {k: str(tmp_path / k) for k in ('plain', 'residue')}
    plain = rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['plain'], batch_size=2)
    res = PaintResidue(min_intensity=10000.0, reach=1.0, clear=0.25)
    lines3d, merged = rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['residue'], batch_size=2, residue=res)
    assert sorted(plain[0]) == sorted(lines3d) and all(len(plain[0][k]) == len(lines3d[k]) and
                                                       all(np.array_equal(a, b) for a, b in zip(plain[0][k], lines3d[k])) for k in lines3d)
    assert len(plain[1]) == len(merged) and all(np.array_equal(a, b) for a, b in zip(plain[1], merged))
    names = ('residue.json', 'residue.npy', 'residue_cells.npy')
    for name in names:
        assert not os.path.exists(os.path.join(out['plain'], 'params', name)) and os.path.exists(os.path.join(out['residue'], 'params', name))
    pc = os.path.join('out_pc_seq_json_dir', 'merged.txt')
    assert open(os.path.join(out['plain'], pc), 'rb').read() == open(os.path.join(out['residue'], pc), 'rb').read()
    lines = list(merged) if len(merged) else [l for name in sorted(lines3d) for l in lines3d[name]]
    assert lines, 'the strip yielded no lines'
    seg = las_io.line_segments(lines, off)
    index = ops.line_index(seg, res.reach, cell=las_io.residue_index_cell(res), device=dev)     # (the residue grid covers the index grid's box)
    grid = ops.residue_grid(index, res.cell)
    key, iq = rr.keys_f32(_decoded(las, off), seg, res.reach, res.z_tol, res.min_intensity, res.clear, grid, pruned=True)
    cells, comp, st = rr.blobs([key], [iq], grid['nx'], 8)
    got_st = np.load(os.path.join(out['residue'], 'params', 'residue.npy'))
    got_cells = np.load(os.path.join(out['residue'], 'params', 'residue_cells.npy'))
    assert got_st.dtype == np.int64 and got_cells.dtype == np.int32 and got_cells.shape == (len(cells), 3)
    assert np.array_equal(got_cells[:, 1].astype(np.int64) * grid['nx'] + got_cells[:, 0], cells) and np.array_equal(got_cells[:, 2], comp)
    assert np.array_equal(got_st, st), f'{int((got_st != st).sum())} statistics differ from the reference'
    used = json.load(open(os.path.join(out['residue'], 'params', 'residue.json')))
    grid['shift'] = [float(v) for v in off]
    summary = las_io.residue_summary(ops.ResidueBlobs(got_cells[:, :2], got_cells[:, 2], got_st, grid), lines, res)
    assert used == json.loads(json.dumps({str(b['blob']): b for b in summary}))
    print(f'{len(lines)} lines, {len(seg)} segments, {int((key >= 0).sum())} residue points, {len(cells)} cells, {len(st)} blobs, {len(summary)} reported')
    assert len(cells) > 0, 'no residue: the test shows nothing'
