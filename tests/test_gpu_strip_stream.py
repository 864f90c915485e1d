"""GPU: the chunked strip route.  ops.StripBinner (lm_strip_bin_count / lm_strip_bin_scatter, csrc/strip.hip) against
ops.strip_bin_points on the whole cloud, bit for bit, at chunk seams around the 2048-point wave seam and for groups of tiles; the
capacity check and both entries between guards, after poisoned LDS and on a side stream; the record passes chunk by chunk against the
whole-file passes; Runner.infer_las_strip_to_map(stream=) against the same call without it, every file byte for byte, and its peak
device memory."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import lds_state
from guards import CANARY, Slab, _signed
from lanemapping_amd import io_utils, las_io, ops
from lanemapping_amd._lib import LanemapHipError, LmRasterParams, LmStripGrid, lib
from lanemapping_amd.las_io import (CrossSection, GroundFilter, IntensityStretch, MarkingColour, MarkingLabels, MarkingSurvey, PaintResidue,
                                    PaintThreshold, StripStream)
from oracle import las_ref

pytestmark = pytest.mark.gpu

H = W = 1152                                                       # the tile size of tests/test_gpu_strip.py
f32 = np.float32
Z_RANGE = (-2.0, 3.0)


# ------------------------------------------------------------------------------------------------ the cloud and the layout
def _layout():
    """Six tiles: two that overlap, one rotated, one tilted, one no finite point reaches, one that holds every finite point of the box."""
    yaw = 0.4
    tilt = np.array([math.cos(0.1), 0.012, -0.017, math.sin(0.1)])
    return [ops.make_raster_params(trans=(2.0, 1.0, 0.0), bev_img_offset=(-1.0, 0.5), local_min_ele=-0.5, ele_reso=0.02),
            ops.make_raster_params(trans=(30.0, 4.0, 0.25), local_min_ele=-0.5, ele_reso=0.02),
            ops.make_raster_params(quat=(math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)), trans=(20.0, -10.0, 0.0)),
            ops.make_raster_params(quat=tilt / np.linalg.norm(tilt) * 1.02, trans=(8.0, 6.0, -0.2), bev_img_offset=(0.5, -0.5)),
            ops.make_raster_params(trans=(4000.0, 4000.0, 0.0)),
            ops.make_raster_params(trans=(-12.0, -12.0, 0.0), img_reso=(0.1, 0.1))]


_CLOUD = {}


def _cloud(dev):
    """10,007 points in acquisition-like order over a box of 90 m x 70 m, with NaN, +-inf and points outside Z_RANGE spread over it
    (their waves test every tile), and the whole-cloud result every test compares against: computed once, never changed."""
    if not _CLOUD:
        rng = np.random.RandomState(5)
        n = 10007
        s = np.sort(rng.uniform(0, 1, n))
        pts = np.stack([90.0 * s + rng.normal(0, 0.5, n), rng.uniform(-5, 65, n), rng.normal(0.3, 0.2, n), np.floor(rng.uniform(500, 40000, n))],
                       axis=1).astype(f32)
        pts[rng.choice(n, 40, replace=False), rng.randint(0, 3, 40)] = np.nan
        pts[rng.choice(n, 20, replace=False), rng.randint(0, 3, 20)] = np.inf
        pts[rng.choice(n, 20, replace=False), rng.randint(0, 3, 20)] = -np.inf
        pts[rng.choice(n, 300, replace=False), 2] = rng.choice([-7.5, 9.0], 300).astype(f32)           # outside Z_RANGE, inside the windows
        pts[2047:2050, 2] = 11.0                                                                        # and on the wave seam
        cloud = torch.from_numpy(pts).to(dev)
        params = _layout()
        binned, offs = ops.strip_bin_points(cloud, params, H, W, z_range=Z_RANGE)
        counts = np.diff(offs)
        # (where a point with a non-finite coordinate lands is the rasteriser's window test's business: some land in every tile)
        finite = np.isfinite(binned.cpu().numpy()[:, :3]).all(axis=1)
        assert not finite[offs[4]:offs[5]].any() and finite[offs[5]:].sum() == np.isfinite(pts[:, :3]).all(axis=1).sum(), counts
        assert min(counts[0:4]) > 500, counts
        assert offs[-1] > 2 * n, 'overlap: most points are in several tiles'
        _CLOUD.update(pts=pts, cloud=cloud, params=params, binned=binned.view(torch.int32).cpu(), offs=offs)
    return _CLOUD


def _chunks(cloud, size):
    return [cloud[i:i + size] for i in range(0, cloud.shape[0], size)]


def _binned_by_chunks(dev, size, tiles=None, budget_groups=None):
    K = _cloud(dev)
    b = ops.StripBinner(K['params'], H, W, Z_RANGE, dev)
    for c in _chunks(K['cloud'], size):
        b.count(c)
    counts = b.counts()
    out = []
    for run in (budget_groups(counts) if budget_groups else [tiles]):
        b.begin(run)
        for c in _chunks(K['cloud'], size):
            b.scatter(c)
        out.append((run, *b.finish()))
    return counts, out


# ------------------------------------------------------------------------------------------------ 1. chunked = whole
@pytest.mark.parametrize('size', [256, 2047, 2048, 2304, 10240])
def test_chunked_binning_equals_whole_binning(dev, size):
    """Chunk seams before, on and after the wave seam at 2048 points, and one chunk that holds the whole cloud."""
    K = _cloud(dev)
    counts, [(_, binned, offs)] = _binned_by_chunks(dev, size)
    assert counts.dtype == np.int64 and counts.tolist() == np.diff(K['offs']).tolist(), 'the accumulated counts are the whole-cloud counts'
    assert offs == K['offs']
    assert tuple(binned.shape) == (K['offs'][-1], 4) and torch.equal(binned.view(torch.int32).cpu(), K['binned']), \
        f'binned from chunks of {size} points is not bit-identical to the whole-cloud call'


def test_uneven_and_empty_chunks(dev):
    """Chunks of every size in turn, an empty one among them: pass B only has to repeat pass A's points, not a chunk size."""
    K = _cloud(dev)
    cuts = [0, 1, 1, 64, 700, 2048, 2049, 6000, 6000, 10007]
    b = ops.StripBinner(K['params'], H, W, Z_RANGE, dev)
    for a, z in zip(cuts, cuts[1:]):
        b.count(K['cloud'][a:z])
    b.begin()
    for c in _chunks(K['cloud'], 3000):                            # other seams in pass B: the same points in the same order
        b.scatter(c)
    binned, offs = b.finish()
    assert offs == K['offs'] and torch.equal(binned.view(torch.int32).cpu(), K['binned'])
    with pytest.raises(ValueError, match='pass A is over'):
        b.count(K['cloud'][:10])


def test_an_empty_tile_and_an_empty_cloud(dev):
    """The finite points alone: the far tile counts nothing and owns an empty range; no points at all: offsets of zeros."""
    K = _cloud(dev)
    cloud = K['cloud'][torch.isfinite(K['cloud']).all(dim=1)].contiguous()
    want, woffs = ops.strip_bin_points(cloud, K['params'], H, W, z_range=Z_RANGE)
    b = ops.StripBinner(K['params'], H, W, Z_RANGE, dev)
    for c in _chunks(cloud, 2047):
        b.count(c)
    assert b.counts().tolist() == np.diff(woffs).tolist() and b.counts()[4] == 0
    b.begin()
    for c in _chunks(cloud, 2047):
        b.scatter(c)
    binned, offs = b.finish()
    assert offs == woffs and offs[4] == offs[5] and torch.equal(binned.view(torch.int32), want.view(torch.int32))
    b.begin((4, 5))                                                # the empty tile alone: nothing to allocate, nothing written
    for c in _chunks(cloud, 2047):
        b.scatter(c)
    binned, offs = b.finish()
    assert offs == [0, 0] and tuple(binned.shape) == (0, 4)
    e = ops.StripBinner(K['params'], H, W, Z_RANGE, dev)
    e.count(cloud[:0])
    e.begin()
    e.scatter(cloud[:0])
    binned, offs = e.finish()
    assert offs == [0] * 7 and tuple(binned.shape) == (0, 4)


# ------------------------------------------------------------------------------------------------ 2. groups of tiles
@pytest.mark.parametrize('n_groups', [3, 2])
def test_tile_groups_concatenate_to_the_whole(dev, n_groups):
    """Batches of two tiles; a budget below any batch gives one batch per group, one that holds four of the six tiles gives two groups."""
    K = _cloud(dev)
    whole = np.diff(K['offs'])
    budget = 1 if n_groups == 3 else 16 * int(whole[0:4].sum())
    counts, runs = _binned_by_chunks(dev, 2304, budget_groups=lambda c: las_io.tile_groups(c, 2, budget))
    assert [r for r, _, _ in runs] == ([(0, 2), (2, 4), (4, 6)] if n_groups == 3 else [(0, 4), (4, 6)])
    for (t0, t1), binned, offs in runs:
        assert offs == [o - K['offs'][t0] for o in K['offs'][t0:t1 + 1]]
        assert torch.equal(binned.view(torch.int32).cpu(), K['binned'][K['offs'][t0]:K['offs'][t1]]), f'tiles {t0} .. {t1 - 1}'
    assert torch.equal(torch.cat([b for _, b, _ in runs]).view(torch.int32).cpu(), K['binned'])


# ------------------------------------------------------------------------------------------------ raw entries between guards
def _s(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _fill_if_poisoned():
    """Inside lds_state.poisoned(): the fill its wrapper enqueues before an entry it finds (it finds entries by the stream in first
    place), counted like one - the last thing on the stream before the entry."""
    state = lds_state._ACTIVE
    if state is not None:
        lds_state.fill(state.word)
        state.fills += 1


class _Raw:
    """The chunk entries called directly, every operand a guards.Slab: points (input: pad around it), consts, workspace, counts,
    cursors, err and binned (outputs: canaries around them)."""

    def __init__(self, dev, params, pts, capacity, pad=0.0, chunk=2304):
        L = lib()
        self.dev, self.L, self.T, self.chunk, self.cap, self.n = dev, L, len(params), chunk, capacity, len(pts)
        T = self.T
        par = (LmRasterParams * T)(*params)
        g = LmStripGrid()
        assert L.lm_strip_build_grid(par, T, H, W, *Z_RANGE, C.byref(g), None, 0) == 0, L.lm_last_error()
        self.pts = Slab(dev, len(pts), 4, front=512, back=512).fill_input(torch.from_numpy(pts), pad)
        self.consts = Slab(dev, 1, int(L.lm_strip_plan_consts_bytes(T, g.nx * g.ny)), front=1, back=1, dtype=torch.uint8).fill_canary()
        self.ws = Slab(dev, 1, int(L.lm_strip_chunk_workspace_bytes(chunk, T)), front=1, back=1, dtype=torch.uint8).fill_canary()
        self.counts = Slab(dev, 1, 2 * T, front=4, back=4, dtype=torch.int32).fill_canary()            # int64 [T] as int32 pairs
        self.cursors = Slab(dev, 1, 2 * T, front=4, back=4, dtype=torch.int32).fill_canary()
        self.err = Slab(dev, 1, 1, front=64, back=64, dtype=torch.int32).fill_canary()
        self.binned = Slab(dev, capacity, 4, front=512, back=512).fill_canary()
        self.counts.view.zero_()
        self.err.view.zero_()
        self.plan = C.c_void_p()
        rc = L.lm_strip_plan_create(par, T, H, W, *Z_RANGE, C.c_void_p(self.consts.ptr()), self.consts.width, C.byref(self.plan), _s(dev))
        assert rc == 0, L.lm_last_error()

    def _each(self):
        for first in range(0, self.n, self.chunk):
            yield C.c_void_p(self.pts.ptr() + 16 * first), min(self.chunk, self.n - first)

    def count(self):
        for p, n in self._each():
            _fill_if_poisoned()
            rc = self.L.lm_strip_bin_count(self.plan, p, n, C.c_void_p(self.ws.ptr()), self.ws.width, C.c_void_p(self.counts.ptr()), _s(self.dev))
            assert rc == 0, self.L.lm_last_error()
        return self.counts.view.cpu().numpy().view(np.int64).reshape(-1)

    def scatter(self, cursors):
        self.cursors.view.copy_(torch.from_numpy(np.asarray(cursors, dtype=np.int64).view(np.int32)).reshape(1, -1))
        for p, n in self._each():
            _fill_if_poisoned()
            rc = self.L.lm_strip_bin_scatter(self.plan, p, n, C.c_void_p(self.ws.ptr()), self.ws.width, C.c_void_p(self.cursors.ptr()),
                                             C.c_void_p(self.binned.ptr()) if self.cap else None, self.cap, C.c_void_p(self.err.ptr()), _s(self.dev))
            assert rc == 0, self.L.lm_last_error()
        torch.cuda.synchronize(self.dev)
        return self.cursors.view.cpu().numpy().view(np.int64).reshape(-1), int(self.err.view.cpu()[0, 0])

    def check_guards(self, name):
        torch.cuda.synchronize(self.dev)
        for what in ('consts', 'ws', 'counts', 'cursors', 'err', 'binned'):
            s = getattr(self, what)
            c = _signed(CANARY[s.dtype], s.dtype)
            bad = (~s.inside) & (s.bits() != c)
            assert not bool(bad.any()), f'{name}: {int(bad.sum())} words of the guards around {what} changed'

    def close(self):
        assert self.L.lm_strip_plan_destroy(self.plan) == 0
        self.plan = None


# ------------------------------------------------------------------------------------------------ 3. capacity
def test_a_chunk_that_overruns_capacity_writes_nothing_outside_binned(dev):
    K = _cloud(dev)
    total, offs = K['offs'][-1], K['offs']
    want = K['binned']
    short = 37
    r = _Raw(dev, K['params'], K['pts'], total - short)
    assert r.count().tolist() == np.diff(offs).tolist()
    cursors, err = r.scatter(offs[:-1])
    r.check_guards('capacity 37 rows short')
    assert err != 0, 'the last chunk overran binned and err was not set'
    assert cursors.tolist() == offs[1:], 'the cursors advance all the same'
    assert torch.equal(r.binned.logical_bits(), want[:total - short]), 'what fits is what the whole-cloud call writes there'
    r.close()
    # cursors that start before binned: the first five slots of tile 0 lie at negative rows
    r = _Raw(dev, K['params'], K['pts'], total)
    r.count()
    cursors, err = r.scatter([o - 5 for o in offs[:-1]])
    r.check_guards('cursors 5 rows early')
    assert err != 0
    got = r.binned.logical_bits()
    assert torch.equal(got[:total - 5], want[5:]) and bool((got[total - 5:] == r.binned.bits()[0]).all()), 'rows no slot reached keep the canary'
    r.close()
    # capacity 0 and no binned at all
    r = _Raw(dev, K['params'], K['pts'], 0)
    r.count()
    cursors, err = r.scatter(offs[:-1])
    r.check_guards('capacity 0')
    assert err != 0 and cursors.tolist() == offs[1:]
    r.close()
    # the wrapper: finish() reads err back and raises
    b = ops.StripBinner(K['params'], H, W, Z_RANGE, dev)
    b.count(K['cloud'])
    b.begin(capacity=total - 1)
    b.scatter(K['cloud'])
    with pytest.raises(LanemapHipError, match=f'overran binned.*{total - 1} rows'):
        b.finish()
    b.begin()                                                      # pass B of other points than pass A counted: caught by the cursors
    b.scatter(K['cloud'][:5000])
    with pytest.raises(LanemapHipError, match='not the chunks counted'):
        b.finish()


# ------------------------------------------------------------------------------------------------ 4. guards, LDS, side stream
def test_both_entries_between_guards_and_after_poisoned_lds(dev):
    """Every operand between guards: benign and poisoned (NaN) input guards, then after LDS pre-filled with each word of
    lds_state.WORDS (the tile rows with their UNSET sentinel are the launch's own).  Counts, cursors and binned keep their bits."""
    K = _cloud(dev)
    total, offs = K['offs'][-1], K['offs']

    def run(name, pad):
        r = _Raw(dev, K['params'], K['pts'], total, pad=pad)
        counts = r.count()
        cursors, err = r.scatter(offs[:-1])
        r.check_guards(name)
        assert counts.tolist() == np.diff(offs).tolist() and cursors.tolist() == offs[1:] and err == 0, name
        assert torch.equal(r.binned.logical_bits(), K['binned']), f'{name}: binned differs from the whole-cloud call'
        r.close()

    run('benign guards', 0.0)
    run('poisoned guards', float('nan'))
    for word in lds_state.WORDS:
        with lds_state.poisoned(word) as lds:
            run(f'LDS = 0x{word:08X}', 0.0)
        assert lds.fills == 2 * -(-len(K['pts']) // 2304)


def test_refusals_name_the_argument(dev):
    K = _cloud(dev)
    L = lib()
    r = _Raw(dev, K['params'], K['pts'], 16)
    ws, cur, cnt = C.c_void_p(r.ws.ptr()), C.c_void_p(r.cursors.ptr()), C.c_void_p(r.counts.ptr())
    p, b, e = C.c_void_p(r.pts.ptr()), C.c_void_p(r.binned.ptr()), C.c_void_p(r.err.ptr())

    def refused(rc, what):
        assert rc == 1 and what.encode() in L.lm_last_error(), (rc, L.lm_last_error())

    fake = (C.c_char * 64)()
    refused(L.lm_strip_bin_count(None, p, 10, ws, r.ws.width, cnt, _s(dev)), 'plan is no handle')
    refused(L.lm_strip_bin_count(C.cast(fake, C.c_void_p), p, 10, ws, r.ws.width, cnt, _s(dev)), 'plan is no handle')
    refused(L.lm_strip_bin_count(r.plan, p, -1, ws, r.ws.width, cnt, _s(dev)), 'N=-1')
    refused(L.lm_strip_bin_count(r.plan, p, 1 << 31, ws, r.ws.width, cnt, _s(dev)), 'at most 2^31 - 1')
    refused(L.lm_strip_bin_count(r.plan, None, 10, ws, r.ws.width, cnt, _s(dev)), 'null points')
    refused(L.lm_strip_bin_count(r.plan, C.c_void_p(r.pts.ptr() + 4), 10, ws, r.ws.width, cnt, _s(dev)), 'points is not 16-byte aligned')
    refused(L.lm_strip_bin_count(r.plan, p, 10, ws, 16, cnt, _s(dev)), 'workspace too small')
    refused(L.lm_strip_bin_count(r.plan, p, 10, ws, r.ws.width, None, _s(dev)), 'counts_accum')
    refused(L.lm_strip_bin_scatter(r.plan, p, 10, ws, r.ws.width, None, b, 16, e, _s(dev)), 'cursors')
    refused(L.lm_strip_bin_scatter(r.plan, p, 10, ws, r.ws.width, cur, b, -1, e, _s(dev)), 'capacity=-1')
    refused(L.lm_strip_bin_scatter(r.plan, p, 10, ws, r.ws.width, cur, None, 16, e, _s(dev)), 'binned')
    refused(L.lm_strip_bin_scatter(r.plan, p, 10, ws, r.ws.width, cur, b, 16, None, _s(dev)), 'err')
    r.check_guards('refused calls')
    assert bool((r.binned.logical_bits() == r.binned.bits()[0]).all()), 'a refused call wrote to binned'
    r.close()
    # the plan: what lm_strip_bin_points refuses of a layout, and a consts buffer that is too small
    T = 9
    nine = [ops.make_raster_params(trans=(0.5 * i, 0.25 * i, 0), local_min_ele=-0.5) for i in range(T)]
    consts = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    plan = C.c_void_p()
    refused(L.lm_strip_plan_create((LmRasterParams * T)(*nine), T, H, W, -1.0, 1.0, C.c_void_p(consts.data_ptr()), consts.numel(), C.byref(plan),
                                   _s(dev)), 'more than 8 of the 9 tiles')
    assert not plan.value
    refused(L.lm_strip_plan_create((LmRasterParams * 8)(*nine[:8]), 8, H, W, -1.0, 1.0, C.c_void_p(consts.data_ptr()), 256, C.byref(plan), _s(dev)),
            'consts too small')
    refused(L.lm_strip_plan_create((LmRasterParams * 8)(*nine[:8]), 0, H, W, -1.0, 1.0, C.c_void_p(consts.data_ptr()), consts.numel(), C.byref(plan),
                                   _s(dev)), 'T=0')
    assert L.lm_strip_plan_destroy(None) == 0
    with pytest.raises(ValueError, match='finite z_range'):
        ops.StripBinner(K['params'], H, W, None, dev)
    with pytest.raises(LanemapHipError, match='more than 8 of the 9 tiles'):
        ops.StripBinner(nine, H, W, (-1.0, 1.0), dev)


def test_both_entries_on_a_side_stream(dev):
    """Off the default stream: every chunk entry is given exactly the side stream's handle, and the result has the bits of the run on the
    default stream."""
    K = _cloud(dev)
    real = lib()
    seen = []
    saved = {name: getattr(real, name) for name in ('lm_strip_plan_create', 'lm_strip_bin_count', 'lm_strip_bin_scatter')}

    def watch(name, fn):
        def entry(*args):
            seen.append((name, getattr(args[-1], 'value', args[-1]) or 0))
            return fn(*args)
        return entry

    side = torch.cuda.Stream(dev)
    default = torch.cuda.current_stream(dev)
    assert side.cuda_stream != default.cuda_stream
    side.wait_stream(default)
    try:
        for name, fn in saved.items():
            setattr(real, name, watch(name, fn))
        with torch.cuda.stream(side):
            b = ops.StripBinner(K['params'], H, W, Z_RANGE, dev)
            for c in _chunks(K['cloud'], 2304):
                b.count(c)
            counts = b.counts()
            b.begin()
            for c in _chunks(K['cloud'], 2304):
                b.scatter(c)
            binned, offs = b.finish()
            side.synchronize()
    finally:
        for name, fn in saved.items():
            setattr(real, name, fn)
    assert {n for n, _ in seen} == set(saved) and all(s == side.cuda_stream for _, s in seen), seen
    assert counts.tolist() == np.diff(K['offs']).tolist() and offs == K['offs']
    assert torch.equal(binned.view(torch.int32).cpu(), K['binned'])


# ------------------------------------------------------------------------------------------------ 5. the record passes
SHIFT = np.array([351200.0, 3433000.0, 12.0])


def _road(tmp_path):
    """Two lines along x, 3.5 m apart, with their paint, asphalt around them, a bright bar between them: about 2,000 records in each of
    two files of point format 3 (RGB), the points dealt at random, VLR bytes in front and bytes behind the records.
    -> (paths, lines in the LAS frame)."""
    rng = np.random.RandomState(41)
    xs = np.arange(0.0, 42.0, 2.0)
    lines = [np.stack([xs, np.full_like(xs, y), 0.01 * xs], axis=1) + SHIFT for y in (0.0, 3.5)]
    lattice = lambda x0, x1, y0, y1, h: np.stack(np.meshgrid(np.arange(x0 + h / 2, x1, h), np.arange(y0 + h / 2, y1, h)), axis=-1).reshape(-1, 2)
    parts = [(np.stack([rng.uniform(0, 40, 1500), rng.uniform(-3, 7, 1500)], axis=1), (300, 2000))]
    parts += [(lattice(0.0, 40.0, y - 0.075, y + 0.075, 0.075), (20000, 26000)) for y in (0.0, 3.5)]
    parts += [(lattice(10.0, 10.4, 0.4, 2.8, 0.05), (20000, 26000))]
    xy = np.concatenate([p for p, _ in parts])
    xyz = np.concatenate([xy, 0.01 * xy[:, :1] + rng.normal(0, 0.01, (len(xy), 1))], axis=1)
    inten = np.concatenate([rng.randint(lo, hi, len(p)) for p, (lo, hi) in parts])
    deal = rng.rand(len(xyz)) < 0.5
    paths = []
    for k, on in enumerate((deal, ~deal)):
        paths.append(str(tmp_path / f'road{k}.las'))
        las_ref.write_las(paths[k], xyz[on] + SHIFT, inten[on], point_format=3, offset=tuple(SHIFT + [3.0, -2.0, 0.5]), extra_bytes=1, vlr_bytes=54)
        with open(paths[k], 'ab') as f:
            f.write(b'bytes-behind-the-records')
        assert 1500 < int(on.sum()) < 2500
    return paths, lines


def test_record_passes_chunk_by_chunk_equal_the_whole_file_passes(dev, tmp_path):
    """chunk_records = 256 (seven to nine chunks per file, records of 35 bytes: most chunks are padded): the profile, colour, cross and
    histogram tables, the residue and the labelled files equal what the whole-file passes give, in every integer and byte."""
    paths, lines = _road(tmp_path)
    files = [(p, SHIFT, None) for p in paths]
    survey, colour = MarkingSurvey(min_intensity=10000.0), MarkingColour()
    cross, thr = CrossSection(paint_intensity=10000.0), PaintThreshold()
    res = PaintResidue(min_intensity=10000.0, reach=3.0, clear=0.25, min_cells=4, min_points=4)
    labels = MarkingLabels(min_intensity=10000.0)
    for name, call in (('survey', lambda **kw: las_io.survey_files(files, lines, survey, device=dev, **kw)),
                       ('colour', lambda **kw: las_io.survey_colour_files(files, lines, survey, colour, device=dev, **kw)),
                       ('cross', lambda **kw: las_io.cross_files(files, lines, cross, device=dev, **kw)),
                       ('hist', lambda **kw: (las_io.hist_files(files, lines, thr, device=dev, **kw),))):
        whole, chunked = call(), call(chunk_records=256)
        assert len(whole) == len(chunked)
        for a, b in zip(whole, chunked):
            assert a.dtype == b.dtype and np.array_equal(a, b), f'{name}: the chunked table differs from the whole-file table'
        assert int(np.asarray(whole[0] != 0).sum()) > 50, f'{name}: an empty table shows nothing'
    a, b = las_io.residue_files(files, lines, res, device=dev), las_io.residue_files(files, lines, res, device=dev, chunk_records=256)
    assert np.array_equal(a.cells, b.cells) and np.array_equal(a.comp, b.comp) and np.array_equal(a.stats, b.stats) and a.grid == b.grid
    assert len(a.stats) >= 1 and las_io.residue_summary(a, lines, res) == las_io.residue_summary(b, lines, res)
    assert len(las_io.residue_summary(a, lines, res)) >= 1, 'the bar is a blob'
    for k, p in enumerate(paths):
        out_a, out_b = str(tmp_path / 'whole' / f'road{k}.las'), str(tmp_path / 'chunked' / f'road{k}.las')
        ra = las_io.label_las(p, out_a, lines, labels, SHIFT, device=dev)
        rb = las_io.label_las(p, out_b, lines, labels, SHIFT, device=dev, chunk_records=256)
        assert ra == rb and ra['labelled'] > 300 and min(ra['per_line']) > 100
        data = open(out_a, 'rb').read()
        assert data == open(out_b, 'rb').read(), 'the labelled file written chunk by chunk differs'
        assert data != open(p, 'rb').read() and len(data) == os.path.getsize(p) and data.endswith(b'bytes-behind-the-records')


# ------------------------------------------------------------------------------------------------ 6. the Runner
STEP, STRIDE = 1024, 3


def _wide_strip(tmp_path):
    """Four overlapping 1152 x 1152 tiles along x over a climbing plane with six painted stripes, a return at every third pixel centre
    (540,672 returns) - and a swath much wider than the layout: 2.5 M returns beside the tiles, as a scanner that sees 100 m to the side
    of a carriageway delivers them.  Dealt at random into two files.  -> (las paths, parameter file paths, N)."""
    reso, ele, A, Bs = 0.05, 0.05, 0.075, 0.02
    rows = 3 * STEP + H
    r, c = np.meshgrid(np.arange(0, rows, STRIDE), np.arange(0, W, STRIDE), indexing='ij')
    x, y = (r * reso).ravel(), (c * reso).ravel()
    lane_y = [(0.12 + 0.152 * l) * 57.6 + 0.01 * (l - 2.5) * x for l in range(6)]
    paint = np.zeros(len(x), bool)
    for ly in lane_y:
        paint |= np.abs(y - ly) < 0.1
    inten = np.where(paint, 24000.0, 3000.0 + 40.0 * ((r + 3 * c) % 97).ravel())
    rng = np.random.RandomState(7)
    n_side = 2_500_000
    sx, sy = rng.uniform(-20.0, rows * reso + 20.0, n_side), rng.uniform(W * reso + 5.0, W * reso + 150.0, n_side)
    x, y, inten = np.concatenate([x, sx]), np.concatenate([y, sy]), np.concatenate([inten, rng.uniform(1000.0, 6000.0, n_side).round()])
    world = np.stack([x, y, A * x + Bs * y], axis=1)
    order = rng.permutation(len(world))
    deal = rng.rand(len(world)) < 0.5
    las = []
    for k, on in enumerate((deal, ~deal)):
        las.append(str(tmp_path / f'swath{k}.las'))
        keep = order[on[order]]
        las_ref.write_las(las[k], world[keep] + SHIFT, inten[keep], point_format=1, offset=tuple(SHIFT))
    prm_paths = []
    for t in range(4):
        p = {'coor_las_path': '', 'las_read_offset': list(SHIFT), 'las_rotation_trans_quan': [t * STEP * reso, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0],
             'bev_img_offset': [0.0, 0.0], 'img_reso': [reso, reso], 'local_min_ele': -0.5, 'ele_reso': ele}
        prm_paths.append(str(tmp_path / f'18104{t}_0209.txt'))
        io_utils.save_pc_2_img_transform_paras(prm_paths[t], p)
    return las, prm_paths, len(world)


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_runner_stream_route_writes_the_same_files_in_less_memory(dev, net, tmp_path):
    """Two LAS files, four tiles, batches of two; chunks of 2^19 records (three per file) and a budget that holds two of the four tiles
    (two groups), with ground, tile-scope intensity, label, survey, cross, residue and threshold switched on.  Every file under work_dirs
    is byte for byte the file of the same call without stream=, which adds params/stream.json alone.
    Memory, from torch.cuda.max_memory_allocated reset before each call (the network is built): the stream= call stays below the plain
    call by at least 16 N bytes, the whole decoded cloud.  Why it can: both calls peak in the batch loop, on the same network; the plain
    call holds its binned buffer there (N + N / 4 rows of 16 bytes), the stream= call the binned points of one group (here a tenth of N
    rows) - the layout covers a sixth of the swath, so that 20 N - 16 sum(counts of a group) exceeds 16 N.  Measured on an MI355X: plain 1,791,841,280 B, stream= 1,710,586,880 B,
    16 N = 48,650,752 B."""
    from lanemapping_amd.runner import Runner
    las, prm_paths, N = _wide_strip(tmp_path)
    rn = Runner.__new__(Runner)
    rn.cfg, rn.device, rn.net = net.cfg, dev, net
    assert rn.cfg.get('las_stream') is None
    stages = dict(ground=GroundFilter(height_range=(-0.5, 1.0)), intensity=IntensityStretch(), label=MarkingLabels(min_intensity=10000.0),
                  survey=MarkingSurvey(min_intensity=10000.0), cross=CrossSection(paint_intensity=10000.0),
                  residue=PaintResidue(min_intensity=10000.0, reach=1.0, clear=0.25), threshold=PaintThreshold())
    per_tile = (H // STRIDE) * (W // STRIDE)
    stream = StripStream(chunk_records=1 << 19, binned_budget=16 * (2 * per_tile + 1000))
    out = {k: str(tmp_path / k) for k in ('plain', 'stream')}
    peak = {}
    for key, extra in (('plain', {}), ('stream', {'stream': stream})):
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        lines3d, merged = rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out[key], batch_size=2, **stages, **extra)
        torch.cuda.synchronize(dev)
        peak[key] = torch.cuda.max_memory_allocated(dev)
    assert len(lines3d) >= 2 and (len(merged) or lines3d), 'the strip yielded no lines: the stages after the merge show nothing'
    done = json.load(open(os.path.join(out['stream'], 'params', 'stream.json')))
    assert [f['chunks'] for f in done['files']] == [3, 3] and sum(f['records'] for f in done['files']) == N == sum(f['kept'] for f in done['files'])
    assert [g['tiles'] for g in done['groups']] == [[0, 2], [2, 4]] and done['tile_counts'] == [per_tile] * 4
    assert [g['binned_bytes'] for g in done['groups']] == [32 * per_tile] * 2
    files = _tree(out['plain'])
    assert _tree(out['stream']) == sorted(files + [os.path.join('params', 'stream.json')])
    for f in ('181040_0209.json', os.path.join('out_pc_seq_json_dir', 'merged.txt'), os.path.join('labelled', 'swath0.las'),
              os.path.join('labelled', 'swath1.las'), *(os.path.join('params', n) for n in (
                  'intensity.json', 'labels.json', 'markings.npy', 'markings.json', 'cross_sections.npy', 'residue.npy', 'residue_cells.npy',
                  'paint_hist.npy', 'paint_threshold.json', '181040_0209.txt'))):
        assert f in files, f
    for f in files:
        a, b = open(os.path.join(out['plain'], f), 'rb').read(), open(os.path.join(out['stream'], f), 'rb').read()
        assert a == b, f'{f} differs between the plain call and the stream= call'
    print(f"peak device memory: plain {peak['plain']} B, stream= {peak['stream']} B, difference {peak['plain'] - peak['stream']} B, "
          f'16 N = {16 * N} B (N = {N})')
    assert peak['plain'] - peak['stream'] >= 16 * N, (peak, 16 * N)
    # scope='strip' and a budget with more tiles than a batch: refused before any file is opened
    with pytest.raises(ValueError, match='binned_budget'):
        rn.infer_las_strip_to_map([str(tmp_path / 'missing.las')], prm_paths, work_dirs=str(tmp_path / 'refused'), batch_size=2,
                                  intensity=IntensityStretch(scope='strip'), stream=stream)
    # without a budget the strip window is the whole-cloud window: one group
    a = rn.infer_las_strip_to_map(las[:1], prm_paths[:1], work_dirs=str(tmp_path / 'strip_a'), batch_size=2, intensity=IntensityStretch(scope='strip'))
    b = rn.infer_las_strip_to_map(las[:1], prm_paths[:1], work_dirs=str(tmp_path / 'strip_b'), batch_size=2, intensity=IntensityStretch(scope='strip'),
                                  stream=StripStream(chunk_records=1 << 19))
    ia, ib = (open(os.path.join(str(tmp_path / d), 'params', 'intensity.json'), 'rb').read() for d in ('strip_a', 'strip_b'))
    assert ia == ib and sorted(a[0]) == sorted(b[0]) and all(np.array_equal(x, y) for k in a[0] for x, y in zip(a[0][k], b[0][k]))
