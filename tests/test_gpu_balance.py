"""GPU: the intensity balance (csrc/intensity.hip) - ops.tile_intensity_cells and ops.tile_intensity_apply against the numpy restatement
of tests/balance_ref.py, compared for equality in every int32 and every float32 bit; the cases the stream, bounds and LDS inventories
cannot hold for entries that take the stream last (guarded buffers around every operand and the workspace, a side stream beside a busy
default stream, the refusal on a capturing stream); refusals by name; Runner.infer_las_strip_to_map with IntensityStretch(balance=True)
in both scopes.

Shapes: H = W = 72 with cells of 16 px is a 5 x 5 grid whose last row and column of cells are 8 px wide; a workgroup streams a span of
65,536 points of one tile, a wave is 64 points, a cell's counters are two levels of 256 keys."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import balance_ref as br
import ground_ref as gr
import intensity_ref as ir
import lds_state
import stream_state
import test_gpu_intensity as ti
from guards import NAN, Slab, guarded_runs
from lanemapping_amd import io_utils, ops
from lanemapping_amd._lib import LanemapHipError, LmRasterParams, lib
from lanemapping_amd.las_io import IntensityStretch, balance_gains, intensity_window

pytestmark = pytest.mark.gpu

f32 = np.float32
T = 72                                                             # H = W
CELL = 16
G = 5                                                              # ceil(72 / 16)
MINP = 8
ISPAN = 65536
RESO = ti.RESO


def _pixel_points(p, rows, cols, inten):
    """One return at the centre of every pixel (rows[i], cols[i]) of the axis-aligned tile p; pixels outside 0 .. T - 1 lie outside."""
    x = np.asarray(rows, np.float64) * RESO + p.bev_img_offset[0] + p.trans[0]
    y = np.asarray(cols, np.float64) * RESO + p.bev_img_offset[1] + p.trans[1]
    return np.stack([x, y, np.full(len(x), 0.5 + p.trans[2]), np.asarray(inten, np.float64)], axis=1).astype(f32)


def _crafted(p):
    """The cells the rule can go wrong at, on the axis-aligned tile p (cells of 16 px, MINP = 8)."""
    rows, cols, inten = [], [], []

    def add(r, c, v):
        rows.append(r), cols.append(c), inten.append(v)

    for j in range(130):                                           # cell (0, 0): every return on one key - every lane of a wave on one counter
        add(j % 16, (j // 16) % 16, 1234.0)
    for j in range(MINP - 1):                                      # cell (0, 1): one short of known
        add(j, 16 + j, 100.0 + j)
    for j in range(MINP):                                          # cell (0, 2): just known, even n: the lower median is the 4th of 8
        add(j, 32 + j, 200.0 + 10 * j)
    for j in range(5):                                             # cell (1, 0): the median on the seam of two coarse bins
        add(16 + j, j, 255.0)
        add(16 + j, 8 + j, 256.0)
    for j, v in enumerate([np.nan, -7.0, 0.0, 65535.0, 70000.0, np.inf, 12.75, -np.inf, 65534.5]):   # cell (1, 1): what clamps, what does not count
        add(16 + j, 16 + j, v)
    for j in range(20):                                            # cell (4, 4): the partial last cell, 8 x 8 px
        add(64 + j % 8, 64 + (j * 3) % 8, 3000.0 + 17 * j)
    for j, (r, c) in enumerate([(-2, 5), (72, 5), (80, 80), (5, -1), (5, 72), (-1, -1)]):             # outside the window
        add(r, c, [0.0, 65535.0, 1e9, -1e9][j % 4])
    pts = _pixel_points(p, rows, cols, inten)
    return pts[np.random.RandomState(8).permutation(len(pts))]


def _scenes():
    """name -> (pts, offs, tiles): B = 3 each."""
    A, R = ti._axis_tile(), ti._rot_tile()
    one = _pixel_points(A, [70], [3], [500.0])
    crafted = _crafted(A)
    rot = ti._cloud(5, 6000, R, ti.KINDS['nan_and_inf'], T=T)
    junk = ti._cloud(6, 700, ti.FAR, ti.KINDS['uniform_u16'], T=T)
    big = ti._cloud(7, ISPAN + 1, A, ti.KINDS['non_integers'], T=T)
    dense = ti._cloud(9, 9000, R, ti.KINDS['two_values'], T=T)
    return {
        'crafted, rotated, empty': (np.concatenate([crafted, rot]), [0, len(crafted), len(crafted) + len(rot), len(crafted) + len(rot)], [A, R, A]),
        'one point, a span and one, rotated; rows before the first offset': (
            np.concatenate([junk, one, big, dense]), [700, 701, 701 + len(big), 701 + len(big) + len(dense)], [A, A, R]),
    }


def _eq(got, want, name):
    ti._eq(got, want, name)


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. cells
def test_the_crafted_cells_hold_what_they_are_meant_to_hold():
    """No GPU work: the reference puts the special cells where the rule says."""
    pts, offs, tiles = _scenes()['crafted, rotated, empty']
    level, count, model = br.cells(pts, offs, tiles, T, T, CELL, 500000, MINP)
    assert level.shape == (3, G, G) and (count[2] == 0).all() and (level[2] == -1).all() and (model[2] == -1).all()
    assert (count[0, 0, 0], level[0, 0, 0]) == (130, 1234) and (count[0, 0, 1], count[0, 0, 2]) == (MINP - 1, MINP) and level[0, 0, 2] == 230
    assert (count[0, 1, 0], level[0, 1, 0]) == (10, 255) and br.cells(pts, offs, tiles, T, T, CELL, 555556, MINP)[0][0, 1, 0] == 256
    assert count[0, 1, 1] == 8 and level[0, 1, 1] == 12, 'NaN does not count; -7, -inf and 0 are key 0; 12.75 is key 12'
    assert br.cells(pts, offs, tiles, T, T, CELL, 1000000, MINP)[0][0, 1, 1] == 65535 and count[0, 4, 4] == 20 and count[0].sum() == 183
    # (0, 1) is not known: the model of (0, 0) is the lower median of the levels of (0, 0), (1, 0), (1, 1)
    assert model[0, 0, 0] == 255 and model[0, 4, 4] == level[0, 4, 4] and model[0, 2, 4] == -1
    assert (count[1] > 0).all() and 0.3 * 6000 < count[1].sum() < 6000 and (count[1] >= MINP).any() and (model[1] >= 0).all()
    pts, offs, tiles = _scenes()['one point, a span and one, rotated; rows before the first offset']
    count = br.cells(pts, offs, tiles, T, T, CELL, 500000, MINP)[1]
    assert count[0].sum() == 1 and count[0, 4, 0] == 1 and offs[2] - offs[1] == ISPAN + 1 and count[1].sum() > 30000


@pytest.mark.parametrize('q_ppm', [0, 500000, 1000000])
@pytest.mark.parametrize('scene', sorted(_scenes()))
def test_cells_equal_the_reference_in_every_int32(dev, scene, q_ppm):
    pts, offs, tiles = _scenes()[scene]
    cloud = torch.from_numpy(pts).to(dev)
    before = cloud.clone()
    want = br.cells(pts, offs, tiles, T, T, CELL, q_ppm, MINP)
    got = ops.tile_intensity_cells(cloud, offs, tiles, T, T, cell_px=CELL, q_ppm=q_ppm, min_points=MINP)
    for g, w, name in zip(got, want, ('level', 'count', 'model')):
        _eq(g, w, f'{scene}, q_ppm={q_ppm}: {name}')
    again = ops.tile_intensity_cells(cloud, offs, tiles, T, T, cell_px=CELL, q_ppm=q_ppm, min_points=MINP)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), 'two runs differ'
    assert torch.equal(cloud.view(torch.int32), before.view(torch.int32)), 'the points were written'
    # another order of the points of every tile: the same bits
    perm = np.concatenate([np.arange(offs[0])] + [offs[b] + np.random.RandomState(b).permutation(offs[b + 1] - offs[b]) for b in range(3)]
                          + [np.arange(offs[3], len(pts))])
    shuffled = ops.tile_intensity_cells(torch.from_numpy(pts[perm]).to(dev), offs, tiles, T, T, cell_px=CELL, q_ppm=q_ppm, min_points=MINP)
    assert all(torch.equal(a, b) for a, b in zip(got, shuffled)), 'the order of the points shows'


def test_cells_other_grids_and_tile_groups(dev, monkeypatch):
    """cell_px 32 (a 3 x 3 grid with a cell of 8 px) and 128 (one cell), min_points 0 and a large one; then the same call with the
    workspace cap so low that every tile is a group of its own."""
    pts, offs, tiles = _scenes()['crafted, rotated, empty']
    cloud = torch.from_numpy(pts).to(dev)
    for cell_px, minp in ((32, 1), (128, 0), (16, 0), (16, 10 ** 6)):
        want = br.cells(pts, offs, tiles, T, T, cell_px, 500000, minp)
        got = ops.tile_intensity_cells(cloud, offs, tiles, T, T, cell_px=cell_px, q_ppm=500000, min_points=minp)
        for g, w, name in zip(got, want, ('level', 'count', 'model')):
            _eq(g, w, f'cell_px={cell_px}, min_points={minp}: {name}')
    whole = ops.tile_intensity_cells(cloud, offs, tiles, T, T, cell_px=CELL, min_points=MINP)
    monkeypatch.setattr(ops, 'CELLS_WORKSPACE_CAP', 1)
    calls = []
    real = lib().lm_tile_intensity_cells
    monkeypatch.setattr(lib(), 'lm_tile_intensity_cells', lambda *a: calls.append(a[3]) or real(*a), raising=False)
    split = ops.tile_intensity_cells(cloud, offs, tiles, T, T, cell_px=CELL, min_points=MINP)
    assert calls == [1, 1, 1] and all(torch.equal(a, b) for a, b in zip(whole, split))


# ------------------------------------------------------------------------------------------------ 2. apply
def _gains(seed, B=3):
    g = np.random.RandomState(seed).uniform(0.25, 4.0, (B, G, G)).astype(f32)
    g[0, 1, 1] = 4.0                                               # the cell of 65535, 70000 and inf
    return g


@pytest.mark.parametrize('scene', sorted(_scenes()))
def test_apply_equals_the_reference_in_every_bit(dev, scene):
    pts, offs, tiles = _scenes()[scene]
    gains = _gains(11)
    want = br.apply(pts, offs, tiles, gains, T, T, CELL)
    cloud = torch.from_numpy(pts).to(dev)
    d_gains = torch.from_numpy(gains).to(dev)
    out = torch.full_like(cloud, -77.0)
    got = ops.tile_intensity_apply(cloud, offs, tiles, d_gains, T, T, cell_px=CELL, out=out)
    assert got is out and torch.equal(cloud.view(torch.int32).cpu(), torch.from_numpy(pts).view(torch.int32)), 'out of place: the points stay'
    lo, hi = offs[0], offs[-1]
    assert bool((out[:lo] == -77.0).all()) and bool((out[hi:] == -77.0).all()), 'rows outside the tiles were written'
    assert np.array_equal(_bits(out)[lo:hi], _bits(want)[lo:hi]), f'{int((_bits(out)[lo:hi] != _bits(want)[lo:hi]).sum())} words differ from the reference'
    # in place equals out of place
    same = ops.tile_intensity_apply(cloud, offs, tiles, d_gains, T, T, cell_px=CELL)
    assert same is cloud and np.array_equal(_bits(cloud)[lo:hi], _bits(out)[lo:hi]) and np.array_equal(_bits(cloud)[:lo], _bits(pts)[:lo])
    # x, y, z keep their bits everywhere; the points that do not count keep all four words
    assert np.array_equal(_bits(cloud)[:, :3], _bits(pts)[:, :3])
    counts = np.zeros(len(pts), bool)
    for b, p in enumerate(tiles):
        counts[offs[b]:offs[b + 1]] = br.counted(pts[offs[b]:offs[b + 1]], p, T, T)[0]
    assert 0 < (~counts[lo:hi]).sum() and np.array_equal(_bits(cloud)[~counts], _bits(pts)[~counts]), 'a point that does not count changed'
    changed = (_bits(cloud)[:, 3] != _bits(pts)[:, 3])
    assert changed[counts].mean() > 0.5
    # gains of all 1: the buffer keeps every bit
    again = torch.from_numpy(pts).to(dev)
    ops.tile_intensity_apply(again, offs, tiles, torch.ones_like(d_gains), T, T, cell_px=CELL)
    with np.errstate(invalid='ignore'):
        over = counts & (pts[:, 3] > 65535)                       # the rule's own clamp: i' = fminf(i * 1, 65535)
    assert np.array_equal(_bits(again)[~over], _bits(pts)[~over]), 'gains of 1 changed the buffer'
    assert bool((again.cpu().numpy()[over, 3] == 65535.0).all()) and (over.any() == (scene == 'crafted, rotated, empty'))


def test_apply_clamps_at_65535(dev):
    pts, offs, tiles = _scenes()['crafted, rotated, empty']
    cloud = torch.from_numpy(pts).to(dev)
    ops.tile_intensity_apply(cloud, offs, tiles, torch.full((3, G, G), 4.0, device=dev), T, T, cell_px=CELL)
    got = cloud.cpu().numpy()
    first = got[:offs[1]]
    on = br.counted(pts[:offs[1]], tiles[0], T, T)[0]
    src = pts[:offs[1], 3]
    assert (first[on & (src >= 16384), 3] == 65535.0).sum() >= 3, '65535, 70000 and inf times 4 clamp'
    assert first[on, 3].max() == 65535.0 and np.array_equal(first[on & (src < 16000), 3], src[on & (src < 16000)] * f32(4))
    assert (first[on & (src < 0), 3] < 0).any(), 'a negative intensity stays negative: the key clamps, the value does not'


# ------------------------------------------------------------------------------------------------ 3. the scenario on the GPU chain
def _chain(cloud, offs, tiles, st, H, W):
    """tile_intensity_window -> tile_intensity_cells -> balance_gains -> tile_intensity_apply, in place: what the runner does per batch."""
    window, count = ops.tile_intensity_window(cloud, offs, tiles, H, W, percentiles=(50.0, 50.0))
    both = torch.cat([window[:, :1].to(torch.int64), count[:, None]], dim=1).cpu().numpy()
    level, cnt, model = ops.tile_intensity_cells(cloud, offs, tiles, H, W, cell_px=st.cell_px, min_points=st.cell_min_points)
    gains = balance_gains(model.cpu().numpy(), both[:, 0], st, count=both[:, 1])
    ops.tile_intensity_apply(cloud, offs, tiles, torch.from_numpy(gains).to(cloud.device), H, W, cell_px=st.cell_px)
    return {'points': cloud, 'level': level, 'count': cnt, 'model': model, 'gains': torch.from_numpy(gains)}


def _chain_ref(pts, offs, tiles, st, H, W):
    level, cnt, model = br.cells(pts, offs, tiles, H, W, st.cell_px, 500000, st.cell_min_points)
    keys = [br.counted(pts[offs[b]:offs[b + 1]], p, H, W) for b, p in enumerate(tiles)]
    ref = [br.lower_median(k[3][k[0]]) if k[0].any() else -1 for k in keys]
    ref = [r if k[0].sum() >= st.min_points else 0 for r, k in zip(ref, keys)]
    gains = br.gains(model, ref, st.max_gain)
    return {'points': br.apply(pts, offs, tiles, gains, H, W, st.cell_px), 'level': level, 'count': cnt, 'model': model, 'gains': gains}


def test_the_falloff_scenario_on_the_gpu_chain(dev):
    """A 96 x 96 tile whose intensity falls to a quarter across its columns (tests/test_balance_cpu.py): the GPU chain gives the
    reference's bits, and after it one threshold separates paint from asphalt."""
    p = ti._axis_tile()
    pts, paint, col = br.falloff_tile(p)
    offs = [0, len(pts)]
    st = IntensityStretch(balance=True, cell_px=16)
    assert pts[~paint, 3].max() > pts[paint, 3].min()
    want = _chain_ref(pts, offs, [p], st, 96, 96)
    got = _chain(torch.from_numpy(pts).to(dev), offs, [p], st, 96, 96)
    for k in ('level', 'count', 'model'):
        _eq(got[k], want[k], f'scenario: {k}')
    assert np.array_equal(_bits(got['gains']), _bits(want['gains'])) and np.array_equal(_bits(got['points']), _bits(want['points']))
    out = got['points'].cpu().numpy()
    assert out[~paint, 3].max() < out[paint, 3].min(), 'after the balance one threshold separates paint from asphalt'


# ------------------------------------------------------------------------------------------------ 4. guards, streams, capture
def _fill_if_poisoned():
    """Inside lds_state.poisoned() (guarded_runs opens it): the fill its wrapper enqueues before an entry it finds, counted like one - for
    the entries it cannot find, which take the stream last.  The last thing on the stream before the entry."""
    state = lds_state._ACTIVE
    if state is not None:
        lds_state.fill(state.word)
        state.fills += 1


def _guard_case():
    pts, offs, tiles = _scenes()['one point, a span and one, rotated; rows before the first offset']
    pts, offs = pts[offs[0]:], [o - offs[0] for o in offs]
    return pts, offs, tiles


def test_tile_intensity_cells_guards(dev):
    """lm_tile_intensity_cells with the points, every output and the workspace between guard slabs; the points are not changed."""
    L = lib()
    pts, offs, tiles = _guard_case()
    B = len(tiles)
    need = L.lm_tile_intensity_cells_workspace_bytes(B, T, T, CELL)
    assert need > 0 and need % 256 == 0 and need >= B * G * G * 1024
    for bad in ((0, T, T, CELL), (4097, T, T, CELL), (B, 0, T, CELL), (B, T, T, 15), (B, T, T, 129), (B, 32768, 32768, 16)):
        assert L.lm_tile_intensity_cells_workspace_bytes(*bad) == 0, bad
    par, coffs = (LmRasterParams * B)(*tiles), (C.c_long * (B + 1))(*offs)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(_, poisoned):
        s_pts = Slab(dev, len(pts), 4, front=64, back=64).fill_input(torch.from_numpy(pts), NAN if poisoned else 0.0)
        before = s_pts.bits().clone()
        s_l, s_c, s_m = (Slab(dev, B, G * G, front=2, back=2, dtype=torch.int32).fill_canary() for _ in range(3))
        s_ws = Slab(dev, 1, need, front=1, back=1, dtype=torch.uint8).fill_canary()
        _fill_if_poisoned()
        rc = L.lm_tile_intensity_cells(C.c_void_p(s_pts.ptr()), coffs, par, B, T, T, CELL, 500000, MINP, C.c_void_p(s_ws.ptr()), need,
                                       C.c_void_p(s_l.ptr()), C.c_void_p(s_c.ptr()), C.c_void_p(s_m.ptr()), stream)
        assert rc == 0, L.lm_last_error()
        torch.cuda.synchronize()
        assert torch.equal(s_pts.bits(), before), 'the points buffer was written'
        return {'level': (s_l, B), 'count': (s_c, B), 'model': (s_m, B), 'workspace': (s_ws, 1)}

    got = guarded_runs(run, 'tile_intensity_cells', batch=False)
    want = br.cells(pts, offs, tiles, T, T, CELL, 500000, MINP)
    for k, w in zip(('level', 'count', 'model'), want):
        _eq(got[k].numpy().reshape(B, G, G), w, f'guards: {k}')


@pytest.mark.parametrize('in_place', [False, True])
def test_tile_intensity_apply_guards(dev, in_place):
    """lm_tile_intensity_apply with the points, the gains, the output and the workspace between guard slabs."""
    L = lib()
    pts, offs, tiles = _guard_case()
    B = len(tiles)
    gains = _gains(12)
    need = L.lm_tile_intensity_apply_workspace_bytes(B)
    assert need > 0 and need % 256 == 0 and L.lm_tile_intensity_apply_workspace_bytes(0) == 0 and L.lm_tile_intensity_apply_workspace_bytes(4097) == 0
    par, coffs = (LmRasterParams * B)(*tiles), (C.c_long * (B + 1))(*offs)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(_, poisoned):
        s_g = Slab(dev, B, G * G, front=2, back=2).fill_input(torch.from_numpy(gains), NAN if poisoned else 0.0)
        s_ws = Slab(dev, 1, need, front=1, back=1, dtype=torch.uint8).fill_canary()
        if in_place:                                               # the guards of an in-out buffer are canaries: a stray write shows
            s_out = Slab(dev, len(pts), 4, front=64, back=64).fill_canary()
            s_out.view.copy_(torch.from_numpy(pts))
            s_pts = s_out
        else:
            s_pts = Slab(dev, len(pts), 4, front=64, back=64).fill_input(torch.from_numpy(pts), NAN if poisoned else 0.0)
            s_out = Slab(dev, len(pts), 4, front=64, back=64).fill_canary()
        before = s_pts.bits().clone()
        _fill_if_poisoned()
        rc = L.lm_tile_intensity_apply(C.c_void_p(s_pts.ptr()), coffs, par, B, T, T, CELL, C.c_void_p(s_g.ptr()), C.c_void_p(s_ws.ptr()), need,
                                       C.c_void_p(s_out.ptr()), stream)
        assert rc == 0, L.lm_last_error()
        torch.cuda.synchronize()
        assert in_place or torch.equal(s_pts.bits(), before), 'the points buffer was written'
        return {'out': (s_out, len(pts)), 'workspace': (s_ws, 1)}

    got = guarded_runs(run, 'tile_intensity_apply', batch=False)
    assert np.array_equal(_bits(got['out']), _bits(br.apply(pts, offs, tiles, gains, T, T, CELL)))


def test_both_entries_on_a_side_stream_beside_a_busy_default_stream(dev):
    """The chain of a batch (window, cells, gains, apply) through tests/stream_state.py: on a side stream while a blocker keeps the default
    stream busy, the bits of the run on the default stream, without waiting for that stream.  The harness watches the entries that take
    the stream first (lm_tile_intensity_window here); the two new entries take it last and are watched here: each was given exactly the
    stream that was current."""
    pts, offs, tiles = _guard_case()
    st = IntensityStretch(balance=True, cell_px=CELL, cell_min_points=MINP, min_points=1)
    real = lib()
    seen = []
    saved = {name: getattr(real, name) for name in ('lm_tile_intensity_cells', 'lm_tile_intensity_apply')}

    def watch(name, fn):
        def entry(*args):
            seen.append((name, getattr(args[-1], 'value', args[-1]) or 0, ops._stream().value or 0))
            return fn(*args)
        return entry

    def run(state):
        return _chain(state['pts'].clone(), offs, tiles, st, T, T)

    try:
        for name, fn in saved.items():
            setattr(real, name, watch(name, fn))
        got = stream_state.stream_runs(stream_state.Case('intensity balance chain', ['lm_tile_intensity_window'],
                                                         lambda d: {'pts': torch.from_numpy(pts).to(d)}, run, lambda state, k: None), dev)
    finally:
        for name, fn in saved.items():
            setattr(real, name, fn)
    assert {n for n, _, _ in seen} == set(saved) and all(given == current for _, given, current in seen), seen
    assert len({given for _, given, _ in seen}) == 2, 'one run on the default stream, one on the side stream'
    want = _chain_ref(pts, offs, tiles, st, T, T)
    for k in ('level', 'count', 'model'):
        _eq(got[k], want[k], f'side stream: {k}')
    assert np.array_equal(_bits(got['points']), _bits(want['points'])) and np.array_equal(_bits(got['gains']), _bits(want['gains']))


@pytest.mark.parametrize('entry', ['tile_intensity_cells', 'tile_intensity_apply'])
def test_entry_refuses_a_capturing_stream(dev, entry):
    """tests/test_gpu_streams.py's case for the entries that copy host memory: inside a capture the call raises with the entry's name and
    the reason and writes nothing; the capture ends cleanly and the graph replays; outside the capture the call is served."""
    pts, offs, tiles = _guard_case()
    cloud = torch.from_numpy(pts).to(dev)
    gains = torch.from_numpy(_gains(13)).to(dev)
    out = torch.full_like(cloud, -77.0)
    if entry == 'tile_intensity_cells':
        call = lambda: ops.tile_intensity_cells(cloud, offs, tiles, T, T, cell_px=CELL, min_points=MINP)
    else:
        call = lambda: ops.tile_intensity_apply(cloud, offs, tiles, gains, T, T, cell_px=CELL, out=out)
    call()                                                           # served, and the warm-up of everything the call allocates
    torch.cuda.synchronize(dev)
    out.fill_(-77.0)
    x = torch.arange(8, device=dev, dtype=torch.float32)
    y = torch.zeros_like(x)
    graph, cap = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    with torch.cuda.graph(graph, stream=cap):
        y.copy_(x * 2)
        with pytest.raises(LanemapHipError, match=f'{entry}: must not be called on a stream that is being captured into a graph: '
                                                  'it copies call-local host memory to the device'):
            call()
    y.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert y.tolist() == [0.0, 2.0, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0], 'the capture did not survive the refused call'
    assert bool((out == -77.0).all()), 'the refused call wrote'
    call()
    torch.cuda.synchronize(dev)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_bad_arguments_are_refused_by_name_and_nothing_is_written(dev):
    L = lib()
    pts, offs, tiles = _guard_case()
    B = len(tiles)
    cloud = torch.from_numpy(pts).to(dev)
    par, coffs = (LmRasterParams * B)(*tiles), (C.c_long * (B + 1))(*offs)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    need = L.lm_tile_intensity_cells_workspace_bytes(B, T, T, CELL)
    need_a = L.lm_tile_intensity_apply_workspace_bytes(B)
    ws = torch.empty(need + 16, device=dev, dtype=torch.uint8)
    lvl, cnt, mdl = (torch.full((B, G, G), 77, device=dev, dtype=torch.int32) for _ in range(3))
    gains = torch.from_numpy(_gains(14)).to(dev)
    out = torch.full((len(pts) + 1, 4), -77.0, device=dev)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def cells(points=vp(cloud), offsets=coffs, params=par, B_=B, cell_px=CELL, q_ppm=500000, min_points=MINP, wsp=vp(ws), ws_bytes=need,
              level=vp(lvl), count=vp(cnt), model=vp(mdl)):
        rc = L.lm_tile_intensity_cells(points, offsets, params, B_, T, T, cell_px, q_ppm, min_points, wsp, ws_bytes, level, count, model, stream)
        return rc, L.lm_last_error().decode()

    def apply(points=vp(cloud), offsets=coffs, params=par, B_=B, cell_px=CELL, g=vp(gains), wsp=vp(ws), ws_bytes=need_a, o=vp(out)):
        rc = L.lm_tile_intensity_apply(points, offsets, params, B_, T, T, cell_px, g, wsp, ws_bytes, o, stream)
        return rc, L.lm_last_error().decode()

    down = (C.c_long * (B + 1))(0, 500, 400, 600)
    for kw, msg in (({'B_': -1}, 'B=-1 tiles'), ({'B_': 4097}, 'B=4097 tiles'), ({'cell_px': 15}, 'cell_px=15'), ({'cell_px': 129}, 'cell_px=129'),
                    ({'q_ppm': -1}, 'q_ppm=-1 is outside'), ({'q_ppm': 1000001}, 'q_ppm=1000001 is outside'), ({'min_points': -1}, 'min_points=-1'),
                    ({'points': None}, 'null points'), ({'points': vp(cloud, 4)}, 'points and workspace must be 16-byte aligned'),
                    ({'offsets': None}, 'null pointer (tile_offsets / params)'), ({'params': None}, 'null pointer (tile_offsets / params)'),
                    ({'offsets': down}, 'tile_offsets must be non-decreasing'),
                    ({'wsp': None}, 'null pointer (workspace / level / count / model)'), ({'wsp': vp(ws, 8)}, 'points and workspace must be 16-byte aligned'),
                    ({'ws_bytes': need - 1}, 'workspace too small'), ({'level': None}, 'null pointer (workspace / level / count / model)'),
                    ({'count': None}, 'null pointer (workspace / level / count / model)'), ({'model': None}, 'null pointer (workspace / level / count / model)'),
                    ({'level': vp(lvl, 2)}, 'level, count and model must be 4-byte aligned'), ({'model': vp(mdl, 1)}, 'level, count and model must be 4-byte aligned')):
        rc, err = cells(**kw)
        assert rc == 1 and 'tile_intensity_cells' in err and msg in err, (kw, rc, err)
    for kw, msg in (({'B_': -1}, 'B=-1 tiles'), ({'B_': 4097}, 'B=4097 tiles'), ({'cell_px': 15}, 'cell_px=15'), ({'cell_px': 129}, 'cell_px=129'),
                    ({'points': None}, 'null points'), ({'points': vp(cloud, 4)}, 'points and workspace must be 16-byte aligned'),
                    ({'offsets': None}, 'null pointer (tile_offsets / params)'), ({'offsets': down}, 'tile_offsets must be non-decreasing'),
                    ({'g': None}, 'null pointer (workspace / gains)'), ({'g': vp(gains, 2)}, 'out must be 16-byte aligned, gains 4-byte'),
                    ({'wsp': None}, 'null pointer (workspace / gains)'), ({'ws_bytes': need_a - 1}, 'workspace too small'),
                    ({'o': None}, 'null out'), ({'o': vp(out, 4)}, 'out must be 16-byte aligned, gains 4-byte')):
        rc, err = apply(**kw)
        assert rc == 1 and 'tile_intensity_apply' in err and msg in err, (kw, rc, err)
    # B = 0 is served and touches nothing, whatever the pointers
    assert cells(B_=0, points=None, offsets=None, params=None, wsp=None, ws_bytes=0, level=None, count=None, model=None)[0] == 0
    assert apply(B_=0, points=None, offsets=None, params=None, g=None, wsp=None, ws_bytes=0, o=None)[0] == 0
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in (lvl, cnt, mdl)) and bool((out == -77.0).all()), 'a refused call writes nothing'
    assert torch.equal(cloud.cpu(), torch.from_numpy(pts))
    # the wrappers: what they refuse themselves, and what they pass on
    with pytest.raises(LanemapHipError, match='cell_px=8'):
        ops.tile_intensity_cells(cloud, offs, tiles, T, T, cell_px=8)
    with pytest.raises(LanemapHipError, match='q_ppm=2000000'):
        ops.tile_intensity_cells(cloud, offs, tiles, T, T, cell_px=CELL, q_ppm=2000000)
    with pytest.raises(ValueError, match=r'gains must be a contiguous \[3,5,5\] float32'):
        ops.tile_intensity_apply(cloud, offs, tiles, gains[:, :4], T, T, cell_px=CELL)
    with pytest.raises(ValueError, match='out must be a contiguous'):
        ops.tile_intensity_apply(cloud, offs, tiles, gains, T, T, cell_px=CELL, out=out)
    with pytest.raises(ValueError, match='tile_offsets for 3 tiles'):
        ops.tile_intensity_cells(cloud, offs[:-1], tiles, T, T, cell_px=CELL)


# ------------------------------------------------------------------------------------------------ 6. Runner
def test_runner_strip_balances_before_the_window(dev, net, tmp_path, monkeypatch):
    """tests/test_gpu_intensity.py's strip - two overlapping axis-aligned 1152 x 1152 tiles, one point per 2 x 2 pixels - with a scanner
    whose intensity falls to a quarter across the strip.  IntensityStretch(balance=False) equals IntensityStretch(), file by file and
    tile by tile, and neither it nor a call without `intensity=` reaches the new ops; balance=True in both scopes writes the reference
    chain's gains to params/balance_gains.npy and balance.json and rasterises the reference chain's tiles."""
    from lanemapping_amd.runner import Runner
    from oracle import las_ref
    H = W = 1152
    reso, ele = 0.05, 0.05
    off = np.array([351200.0, 3433000.0, 12.0])
    step = 1024
    rows = step + H
    r, c = np.meshgrid(np.arange(0, rows, 2), np.arange(0, W, 2), indexing='ij')
    x, y = (r * reso).ravel(), (c * reso).ravel()
    rng = np.random.RandomState(4)
    lane_y = [(0.12 + 0.152 * l) * 57.6 + 0.01 * (l - 2.5) * x for l in range(6)]
    paint = np.zeros(len(x), bool)
    for ly in lane_y:
        paint |= np.abs(y - ly) < 0.1
    asphalt = 8000.0 * 0.25 ** (y / y.max()) * (1.0 + 0.2 * x / x.max())     # falls across the strip, rises a little along it
    inten = np.floor(np.where(paint, 2.5, 1.0) * asphalt * rng.uniform(0.95, 1.05, len(x)))
    assert inten[~paint].max() > inten[paint].min(), 'before: no threshold separates paint from asphalt'
    world = np.stack([x, y, 0.02 * x + 0.01 * y], axis=1)
    order = rng.permutation(len(world))
    las = str(tmp_path / 'strip.las')
    las_ref.write_las(las, world[order] + off, inten[order], point_format=1, offset=tuple(off))
    plist, prm_paths, names = [], [], []
    for t in range(2):
        plist.append({'coor_las_path': '', 'las_read_offset': list(off), 'las_rotation_trans_quan': [t * step * reso, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0],
                      'bev_img_offset': [0.0, 0.0], 'img_reso': [reso, reso], 'local_min_ele': -0.5, 'ele_reso': ele})
        names.append(f'18102{t}_0209')
        prm_paths.append(str(tmp_path / (names[t] + '.txt')))
        io_utils.save_pc_2_img_transform_paras(prm_paths[t], plist[t])
    rn = Runner.__new__(Runner)
    rn.cfg, rn.device, rn.net = net.cfg, dev, net
    assert rn.cfg.get('las_intensity') is None
    seen, new_calls = [], []
    real = ops.bev_raster_batch
    real_cells, real_apply = ops.tile_intensity_cells, ops.tile_intensity_apply

    def recording(points, offs, rpar, H_, W_, **kw):
        out = real(points, offs, rpar, H_, W_, **kw)
        seen.append((out[1].cpu().numpy(), kw.get('inten_scale')))
        return out

    monkeypatch.setattr(ops, 'bev_raster_batch', recording)
    monkeypatch.setattr(ops, 'tile_intensity_cells', lambda *a, **k: new_calls.append('cells') or real_cells(*a, **k))
    monkeypatch.setattr(ops, 'tile_intensity_apply', lambda *a, **k: new_calls.append('apply') or real_apply(*a, **k))
    out = {k: str(tmp_path / k) for k in ('omitted', 'plain', 'off', 'tile', 'strip')}
    tree = lambda root: sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)
    rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['omitted'], batch_size=2)
    rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['plain'], batch_size=2, intensity=IntensityStretch())
    rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['off'], batch_size=2, intensity=IntensityStretch(balance=False, cell_px=16))
    assert not new_calls and len(seen) == 3 and seen[0][1] is None, 'without balance=True no new code runs'
    assert np.array_equal(seen[1][0], seen[2][0]) and list(seen[1][1]) == list(seen[2][1]), 'balance=False changed a tile'
    files = tree(out['plain'])
    assert files == tree(out['off']) and sorted(f for f in files if f.startswith('params')) == ['params/intensity.json']
    assert not any(f.startswith('params') for f in tree(out['omitted']))
    for f in files:
        assert open(os.path.join(out['plain'], f), 'rb').read() == open(os.path.join(out['off'], f), 'rb').read(), f

    # the reference chain: the points each tile holds, from the file as the reference reader decodes it
    host = las_ref.read_las_ref(las, shift=off, normalise=False).astype(f32)
    rps = [io_utils.raster_params_from_dict(p) for p in plist]
    held = [host[gr.window(host, rp, H, W)[0]] for rp in rps]
    assert all(len(h) == (H // 2) * (W // 2) for h in held)
    keys = [ir.keys(h, rp, H, W) for h, rp in zip(held, rps)]
    for scope in ('tile', 'strip'):
        seen.clear(), new_calls.clear()
        st = IntensityStretch(scope=scope, balance=True)
        rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out[scope], batch_size=2, intensity=st)
        assert new_calls == ['cells', 'apply'] and len(seen) == 1
        ref = [br.lower_median(k) for k in keys] if scope == 'tile' else [br.lower_median(np.concatenate(keys))] * 2
        models = [br.cells(held[t], [0, len(held[t])], [rps[t]], H, W, st.cell_px, 500000, st.cell_min_points) for t in range(2)]
        gains = np.concatenate([br.gains(models[t][2], [ref[t]], st.max_gain) for t in range(2)])
        assert gains.shape == (2, 36, 36) and gains.min() < 0.8 and gains.max() > 1.5
        got_gains = np.load(os.path.join(out[scope], 'params', 'balance_gains.npy'))
        assert got_gains.dtype == np.float32 and np.array_equal(_bits(got_gains), _bits(gains)), f'scope={scope}: balance_gains.npy'
        rows = json.load(open(os.path.join(out[scope], 'params', 'balance.json')))
        assert rows == {names[t]: [ref[t], int((models[t][1] >= st.cell_min_points).sum()), 36 * 36, float(gains[t].min()), float(gains[t].max())]
                        for t in range(2)}, rows
        bal = [br.apply(held[t], [0, len(held[t])], [rps[t]], gains[t:t + 1], H, W, st.cell_px) for t in range(2)]
        bkeys = [ir.keys(b, rp, H, W) for b, rp in zip(bal, rps)]
        q = [ir.ppm(v) for v in st.percentiles]
        if scope == 'tile':
            want = {names[t]: [*intensity_window(*ir.order_stats(bkeys[t], *q), len(bkeys[t]), st), len(bkeys[t])] for t in range(2)}
        else:
            both = np.concatenate(bkeys)
            want = {names[t]: [*intensity_window(*ir.order_stats(both, *q), len(both), st), len(both)] for t in range(2)}
        used = json.load(open(os.path.join(out[scope], 'params', 'intensity.json')))
        assert used == want, (scope, used, want)
        for t in range(2):
            rp = LmRasterParams.from_buffer_copy(rps[t])
            rp.inten_lo, rp.inten_hi = want[names[t]][0], want[names[t]][1]
            ref_tile = ir.raster(bal[t], [0, len(bal[t])], [rp], H, W, [want[names[t]][2]])
            _eq(seen[0][0][t], ref_tile[0], f'scope={scope}: tile {t}')
        assert sorted(f for f in tree(out[scope]) if f.startswith('params')) == ['params/balance.json', 'params/balance_gains.npy',
                                                                                 'params/intensity.json']
        # what the balance is for: in the balanced points of a tile one threshold separates the paint from the asphalt
        pmask = np.zeros(len(bal[0]), bool)
        for l in range(6):
            pmask |= np.abs(bal[0][:, 1] - ((0.12 + 0.152 * l) * 57.6 + 0.01 * (l - 2.5) * bal[0][:, 0])) < 0.1 - 1e-3
        amask = np.ones(len(bal[0]), bool)
        for l in range(6):
            amask &= np.abs(bal[0][:, 1] - ((0.12 + 0.152 * l) * 57.6 + 0.01 * (l - 2.5) * bal[0][:, 0])) > 0.1 + 1e-3
        assert pmask.sum() > 1000 and bal[0][amask, 3].max() < bal[0][pmask, 3].min(), 'after the balance the paint is brighter than the asphalt'
