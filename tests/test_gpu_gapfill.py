"""GPU: the gap fill of sparse tiles (csrc/gapfill.hip) - ops.tile_gap_hist and ops.tile_gap_fill against the numpy restatement of
tests/gapfill_ref.py, compared as integers; constructed cases; the seams between workgroups; the shipped shape; guarded buffers;
refusals; what it is for; Runner.infer_las_strip_to_map with `density=`.

Sizes the kernel switches at (csrc/gapfill.hip): a workgroup owns a block of GW x GH = 64 x 32 pixels (columns x rows) and stages it with
a halo of R pixels on every side, R = max_radius_px for the histogram and the tile's own radius for the fill; rows travel as aligned dwords
with up to 3 head and 3 tail bytes each (3 W and 3 H W are no multiples of 4 for odd sizes); a launch takes 256 tiles."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import gapfill_ref as gf
import ground_ref as gr
import intensity_ref as ir
from guards import Slab, batched, guarded_runs
from lanemapping_amd import coor_img2pc, io_utils, ops, synth
from lanemapping_amd._lib import LanemapHipError, check, lib
from lanemapping_amd.las_io import GapFill, gap_radius

pytestmark = pytest.mark.gpu

u8 = np.uint8
f32 = np.float32
GW, GH = 64, 32
S = 96
RESO = 0.0625                                                      # 1/16 m: every pixel border is exact in float32


def _random_tiles(seed, B, H, W, occupancy):
    """B tiles with about `occupancy` of their pixels non-empty: R and G random, B = R except in a fifth of the pixels."""
    rng = np.random.RandomState(seed)
    t = rng.randint(0, 256, (B, H, W, 3)).astype(u8)
    same = rng.uniform(size=(B, H, W)) >= 0.2
    t[..., 2][same] = t[..., 0][same]
    t[rng.uniform(size=(B, H, W)) >= occupancy] = 0
    return t


def _eq(got, want, name):
    g = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    w = np.asarray(want)
    assert g.shape == w.shape, (name, g.shape, w.shape)
    bad = g.astype(np.int64) != w.astype(np.int64)
    assert not bad.any(), f'{name}: {int(bad.sum())} of {g.size} elements differ from the reference (first at {np.argwhere(bad)[0].tolist()})'


def _check(dev, tiles, Rmax, radii, name):
    """hist and fill equal the reference; a second call gives the same bytes.  -> (hist, filled) of the reference."""
    t = torch.from_numpy(tiles).to(dev)
    hist, out = ops.tile_gap_hist(t, Rmax), ops.tile_gap_fill(t, radii)
    rh, ro = gf.hist(tiles, Rmax), gf.fill(tiles, radii)
    assert hist.dtype == torch.int32 and out.dtype == torch.uint8 and out.data_ptr() != t.data_ptr()
    _eq(hist, rh, f'{name}: hist')
    _eq(out, ro, f'{name}: fill')
    assert torch.equal(ops.tile_gap_hist(t, Rmax), hist) and torch.equal(ops.tile_gap_fill(t, radii), out), f'{name}: two runs differ'
    assert torch.equal(t.cpu(), torch.from_numpy(tiles)), f'{name}: the input was changed'
    return rh, ro


# ------------------------------------------------------------------------------------------------ 1. equality with the reference
@pytest.mark.parametrize('Rmax', [1, 4, 8])
@pytest.mark.parametrize('H,W', [(96, 96), (67, 131), (5, 300), (1, 1), (GH + 1, GW + 1)])
def test_hist_and_fill_equal_the_reference(dev, H, W, Rmax):
    """Three tiles with the radii (0, Rmax, Rmax // 2) at three occupancies.  67 and 131 are odd: 3 W and 3 H W are no multiples of 4, so
    rows and the tiles with b > 0 start unaligned."""
    for k, occ in enumerate((0.02, 0.3, 0.9)):
        tiles = _random_tiles(1000 * Rmax + 10 * H + k, 3, H, W, occ)
        if H * W > 1:
            assert (tiles[..., 0] != tiles[..., 2]).any() or occ < 0.1
        rh, ro = _check(dev, tiles, Rmax, (0, Rmax, Rmax // 2), f'{H}x{W} Rmax={Rmax} occ={occ}')
        assert np.array_equal(ro[0], tiles[0]), 'radius 0 is a copy'
        assert (rh.sum(axis=1) == H * W).all()
    one = _random_tiles(7, 3, H, W, 0.3)
    _eq(ops.tile_gap_fill(torch.from_numpy(one).to(dev), Rmax), gf.fill(one, Rmax), 'one radius for every tile')


def test_many_tiles_cross_the_launch_chunks(dev):
    """515 tiles of 4 x 6 pixels with the radii b % 9 (a launch takes 256 tiles and carries their radii); 4096 tiles through the histogram."""
    tiles = _random_tiles(3, 515, 4, 6, 0.15)
    radii = [b % 9 for b in range(515)]
    _eq(ops.tile_gap_fill(torch.from_numpy(tiles).to(dev), radii), gf.fill(tiles, radii), '515 tiles')
    many = _random_tiles(4, 4096, 2, 3, 0.3)
    _eq(ops.tile_gap_hist(torch.from_numpy(many).to(dev), 1), gf.hist(many, 1), '4096 tiles')


# ------------------------------------------------------------------------------------------------ 2. constructed cases on 96 x 96
def _empty(B=1):
    return np.zeros((B, S, S, 3), u8)


@pytest.mark.parametrize('Rmax', [1, 4, 8])
def test_constructed_cases(dev, Rmax):
    R = Rmax
    # (a) equidistant sources with different I, and with equal I and different G
    t = _empty(2)
    t[0, 40, 40 - R], t[0, 40, 40 + R] = (90, 200, 90), (91, 3, 91)
    t[1, 40 - R, 40], t[1, 40 + R, 40] = (90, 4, 90), (90, 5, 90)
    _, ro = _check(dev, t, Rmax, R, 'ties')
    assert ro[0, 40, 40].tolist() == [91, 3, 91] and ro[1, 40, 40].tolist() == [90, 5, 90]
    # (b) a source exactly Rmax away along a row fills; one at (Rmax, 1) does not
    t = _empty(2)
    t[0, 50, 50 + R] = (7, 7, 7)
    t[1, 50 + R, 51] = (7, 7, 7)
    rh, ro = _check(dev, t, Rmax, R, 'rim')
    assert ro[0, 50, 50].tolist() == [7, 7, 7] and ro[1, 50, 50].tolist() == [0, 0, 0] and ro[1, 50, 51].tolist() == [7, 7, 7]
    # (c) holes in all four corners and along every border of a full tile; sources in the corners and on the borders of an empty one
    t = np.full((2, S, S, 3), 200, u8)
    t[..., 1] = (np.arange(S)[:, None] + np.arange(S)[None, :]) % 251 + 1
    t[0, :3, :3] = t[0, :3, -3:] = t[0, -3:, :3] = t[0, -3:, -3:] = 0
    t[0, 0, 20:30] = t[0, -1, 50:70] = t[0, 30:40, 0] = t[0, 60:66, -1] = 0
    t[1] = 0
    t[1, 0, 0], t[1, 0, S - 1], t[1, S - 1, 0], t[1, S - 1, S - 1] = (1, 0, 0), (0, 1, 0), (0, 0, 1), (255, 255, 255)
    t[1, 0, 48], t[1, S - 1, 31], t[1, 33, 0], t[1, 64, S - 1] = (9, 9, 9), (8, 8, 8), (7, 7, 7), (6, 6, 6)
    rh, ro = _check(dev, t, Rmax, R, 'corners and borders')
    assert rh[1, 0] == 8 and ro[1, 0, S - 1 - R].tolist() == [0, 1, 0] and ro[1, S - 1, R].tolist() == [0, 0, 1]
    # (d) the middle tile of a batch between two all-255 tiles, with holes: nothing leaks across tiles or across the row end
    t = np.full((3, S, S, 3), 255, u8)
    t[1] = 0
    t[1, 48, 48] = (5, 6, 7)
    rh, ro = _check(dev, t, Rmax, R, 'neighbours all 255')
    assert rh[1].tolist() == gf.hist(t[1:2], Rmax)[0].tolist() and rh[1, 0] == 1 and rh[1, Rmax + 1] == S * S - len(gf.disc(Rmax)) - 1
    assert ro[1, 0].sum() == 0 and ro[1, -1].sum() == 0 and ro[1, :, 0].sum() == 0 and ro[1, :, -1].sum() == 0
    # a source in the last column does not reach the first columns of the next row
    t = _empty()
    t[0, 10, S - 1] = (3, 3, 3)
    _, ro = _check(dev, t, Rmax, R, 'row end')
    assert ro[0, 11, :S - 1 - R].sum() == 0 and ro[0, 10, :S - 1 - R].sum() == 0
    # (e) an all-empty and an all-full tile
    t = _empty(2)
    t[1] = 17
    rh, ro = _check(dev, t, Rmax, R, 'empty and full')
    assert rh[0].tolist() == [0] * (Rmax + 1) + [S * S] and rh[1].tolist() == [S * S] + [0] * (Rmax + 1)


# ------------------------------------------------------------------------------------------------ 3. seams
@pytest.mark.parametrize('Rmax', [1, 4, 8])
def test_seams_between_workgroups(dev, Rmax):
    """A 96 x 96 tile has 2 x 3 blocks of 64 x 32 pixels.  For every pair of adjacent blocks a lone source in the last pixel of one block,
    next to the other (and the reverse): the holes up to Rmax into the other block are filled through the halo."""
    spots = []
    for br in range(3):                                             # horizontal neighbours: the border between columns 63 | 64
        spots += [(GH * br + 13, GW - 1), (GH * br + 13, GW)]
    for br in range(2):                                             # vertical neighbours: rows 31 | 32 and 63 | 64, next to the diagonal block too
        for col in (GW - 1, GW):
            spots += [(GH * (br + 1) - 1, col), (GH * (br + 1), col)]
    t = _empty(len(spots))
    for b, (r, c) in enumerate(spots):
        t[b, r, c] = (100 + b, 50, 100 + b)
    rh, ro = _check(dev, t, Rmax, Rmax, 'seams')
    n = len(gf.disc(Rmax))
    for b, (r, c) in enumerate(spots):
        assert rh[b].tolist()[0] == 1 and rh[b].sum() - rh[b, Rmax + 1] == n + 1
        for dr, dc in ((0, Rmax), (0, -Rmax), (Rmax, 0), (-Rmax, 0)):
            assert ro[b, r + dr, c + dc].tolist() == [100 + b, 50, 100 + b], (b, dr, dc)
        assert ro[b, r, c + Rmax + 1].sum() == 0 and ro[b, r + Rmax + 1, c].sum() == 0


# ------------------------------------------------------------------------------------------------ 4. the shipped shape, once
def test_shipped_shape(dev):
    """Two 1152 x 1152 tiles rasterised from synthetic clouds thinned to one point in eight, Rmax = 4."""
    pts = [synth.las_points(91 + i)[::8] for i in range(2)]
    cloud = torch.from_numpy(np.ascontiguousarray(np.concatenate(pts))).to(dev)
    par = [ops.make_raster_params(local_min_ele=-0.5, ele_reso=0.02)] * 2
    tiles = ops.bev_raster_batch(cloud, [0, len(pts[0]), len(pts[0]) + len(pts[1])], par, u8_only=True)
    host = tiles.cpu().numpy()
    filled = (host.sum(axis=3) > 0).mean()
    assert 0.2 < filled < 0.5, filled
    hist, rh = ops.tile_gap_hist(tiles, 4), gf.hist(host, 4)
    _eq(hist, rh, 'shipped: hist')
    radii = [gap_radius(row, GapFill()) for row in rh]
    assert radii == [2, 2], (radii, rh.tolist())
    out = ops.tile_gap_fill(tiles, radii)
    _eq(out, gf.fill(host, radii), 'shipped: fill')
    assert torch.equal(ops.tile_gap_hist(tiles, 4), hist) and torch.equal(ops.tile_gap_fill(tiles, radii), out), 'two runs differ'


# ------------------------------------------------------------------------------------------------ 5. guarded buffers
GH_, GW_ = 67, 131                                                  # the guarded tile: odd, more than one block each way


def _guard_tile():
    return _random_tiles(21, 1, GH_, GW_, 0.3)[0]


def test_tile_gap_hist_guards(dev):
    """lm_tile_gap_hist with the tiles between slabs of 0xFF (a stray read of a guard byte would be a return next to a hole) and hist on
    canaries; batch element 1 between two all-255 tiles equals the batch-1 call."""
    L = lib()
    tile, Rmax = _guard_tile(), 8
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(B, poisoned):
        data = batched(torch.from_numpy(tile.reshape(GH_, 3 * GW_)), B, 0xFF)
        s_in = Slab(dev, B * GH_, 3 * GW_, front=3, back=3, dtype=torch.uint8).fill_input(data, 0xFF if poisoned else 0)
        s_h = Slab(dev, B, Rmax + 2, front=2, back=2, dtype=torch.int32).fill_canary()
        assert s_in.ptr() % 4 != 0, 'the guarded tile starts unaligned'
        rc = L.lm_tile_gap_hist(stream, C.c_void_p(s_in.ptr()), B, GH_, GW_, Rmax, C.c_void_p(s_h.ptr()))
        assert rc == 0, L.lm_last_error()
        return {'hist': (s_h, 1)}

    got = guarded_runs(run, 'tile_gap_hist')
    _eq(got['hist'], gf.hist(tile[None], Rmax), 'guards: hist')


def test_tile_gap_fill_guards(dev):
    """lm_tile_gap_fill with the tiles between slabs of 0xFF and the output on canaries; batch element 1 (radius 4) between two all-255
    tiles (radius 8) equals the batch-1 call."""
    L = lib()
    tile = _guard_tile()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(B, poisoned):
        data = batched(torch.from_numpy(tile.reshape(GH_, 3 * GW_)), B, 0xFF)
        s_in = Slab(dev, B * GH_, 3 * GW_, front=3, back=3, dtype=torch.uint8).fill_input(data, 0xFF if poisoned else 0)
        s_out = Slab(dev, B * GH_, 3 * GW_, front=5, back=5, dtype=torch.uint8).fill_canary()
        radii = (C.c_int * B)(*([4] if B == 1 else [8, 4, 8]))
        rc = L.lm_tile_gap_fill(stream, C.c_void_p(s_in.ptr()), B, GH_, GW_, radii, C.c_void_p(s_out.ptr()))
        assert rc == 0, L.lm_last_error()
        return {'out': (s_out, GH_)}

    got = guarded_runs(run, 'tile_gap_fill')
    _eq(got['out'].reshape(1, GH_, GW_, 3), gf.fill(tile[None], 4), 'guards: fill')


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_bad_arguments_are_refused_by_name_and_nothing_is_launched(dev):
    L = lib()
    B, H, W = 2, 9, 11
    tiles = torch.from_numpy(_random_tiles(2, B, H, W, 0.3)).to(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    canary = 0x5A

    def call_hist(B_=B, H_=H, W_=W, R_=4, tiles_=tiles.data_ptr(), null_hist=False):
        hist = torch.full((B * 10,), canary, device=dev, dtype=torch.int32)
        rc = L.lm_tile_gap_hist(stream, C.c_void_p(tiles_), B_, H_, W_, R_, None if null_hist else C.c_void_p(hist.data_ptr()))
        torch.cuda.synchronize()
        return rc, hist.cpu().numpy()

    def call_fill(B_=B, H_=H, W_=W, radii=(1, 2), tiles_=tiles.data_ptr(), out_=None, null=None):
        out = torch.full((B * H * W * 3 + 64,), canary, device=dev, dtype=torch.uint8)
        optr = out.data_ptr() if out_ is None else out_
        rc = L.lm_tile_gap_fill(stream, C.c_void_p(tiles_), B_, H_, W_, None if null == 'radius_px' else (C.c_int * len(radii))(*radii),
                                None if null == 'out' else C.c_void_p(optr))
        torch.cuda.synchronize()
        return rc, out.cpu().numpy()

    rc, h = call_hist()
    assert rc == 0 and (h[:B * 6] != canary).all() and (h[B * 6:] == canary).all()
    rc, o = call_fill()
    assert rc == 0 and np.array_equal(o[:B * H * W * 3].reshape(B, H, W, 3), gf.fill(tiles.cpu().numpy(), (1, 2))) and (o[B * H * W * 3:] == canary).all()
    before = tiles.cpu().numpy().copy()
    shape = [(dict(B_=0), 'B=0'), (dict(B_=4097), 'B=4097'), (dict(H_=0), 'H=0'), (dict(H_=32769), 'H=32769'), (dict(W_=0), 'W=0'),
             (dict(W_=32769), 'W=32769'), (dict(B_=-1), 'B=-1'), (dict(tiles_=0), 'null pointer')]
    for kw, word in shape + [(dict(R_=0), 'max_radius_px=0'), (dict(R_=9), 'max_radius_px=9'), (dict(null_hist=True), 'null pointer')]:
        rc, h = call_hist(**kw)
        with pytest.raises(LanemapHipError, match=word):
            check(rc)
        assert (h == canary).all(), f'{word}: refused, yet something was written'
    for kw, word in shape + [(dict(radii=(1, -1)), r'radius_px\[1\]=-1'), (dict(radii=(9, 0)), r'radius_px\[0\]=9'),
                             (dict(null='radius_px'), 'null pointer'), (dict(null='out'), 'null pointer'),
                             (dict(out_=tiles.data_ptr()), 'overlaps'), (dict(out_=tiles.data_ptr() + 3 * W), 'overlaps')]:
        rc, o = call_fill(**kw)
        with pytest.raises(LanemapHipError, match=word):
            check(rc)
        assert (o == canary).all(), f'{word}: refused, yet something was written'
    assert np.array_equal(tiles.cpu().numpy(), before), 'a refused call wrote into its input'
    # the Python layer
    with pytest.raises(LanemapHipError, match='max_radius_px'):
        ops.tile_gap_hist(tiles, 9)
    with pytest.raises(LanemapHipError, match=r'radius_px\[1\]'):
        ops.tile_gap_fill(tiles, [0, 9])
    with pytest.raises(ValueError, match='radius_px entries'):
        ops.tile_gap_fill(tiles, [1])
    for bad in (tiles.to(torch.int32), tiles[:, :, :, :2], tiles[:, ::2], tiles[0], tiles.permute(0, 2, 1, 3)):
        with pytest.raises(ValueError, match=r'\[B,H,W,3\]'):
            ops.tile_gap_hist(bad)
        with pytest.raises(ValueError, match=r'\[B,H,W,3\]'):
            ops.tile_gap_fill(bad, 1)
    with pytest.raises(LanemapHipError, match='HIP'):
        ops.tile_gap_hist(tiles.cpu())
    with pytest.raises(LanemapHipError, match='HIP'):
        ops.tile_gap_fill(tiles.cpu(), 1)


# ------------------------------------------------------------------------------------------------ 7. what it is for
def _axis_tile():
    return ops.make_raster_params(trans=(8.0, 16.0, 0.5), bev_img_offset=(-1.0, 0.5), img_reso=(RESO, RESO), local_min_ele=-1.0, ele_reso=0.02)


def test_a_thinned_tile_becomes_solid_again(dev):
    """One point per pixel of a 96 x 96 tile, asphalt 5000..9000 with paint 30000..33000 on columns 40..43, thinned to the points of even
    row and even column: three pixels in four are empty.  The histogram is exactly [S^2/4, S^2/2, S^2/4, 0, 0, 0], the rule picks radius 2,
    the filled tile has no empty pixel and its paint covers columns 40..43 and stays inside 39..44."""
    p = _axis_tile()
    r, c = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    rng = np.random.RandomState(11)
    inten = np.where((c >= 40) & (c < 44), np.floor(rng.uniform(30000, 33001, (S, S))), np.floor(rng.uniform(5000, 9001, (S, S))))
    x = r * RESO + p.bev_img_offset[0] + p.trans[0]
    y = c * RESO + p.bev_img_offset[1] + p.trans[1]
    pts = np.stack([x.ravel(), y.ravel(), np.full(S * S, 0.5 + p.trans[2]), inten.ravel()], axis=1).astype(f32)
    on, row, col, _ = gr.window(pts, p, S, S)
    assert on.all() and np.array_equal(row, r.ravel()) and np.array_equal(col, c.ravel())
    thin = np.ascontiguousarray(pts[((r % 2 == 0) & (c % 2 == 0)).ravel()])
    offs = [0, len(thin)]
    tile = ops.bev_raster_batch(torch.from_numpy(thin).to(dev), offs, [p], S, S, u8_only=True)
    ref_tile = ir.raster(thin, offs, [p], S, S)
    _eq(tile, ref_tile, 'the thinned tile')
    assert (ref_tile.sum(axis=3) == 0).mean() == 0.75
    hist = ops.tile_gap_hist(tile, 4).cpu().numpy()
    assert hist.tolist() == [[S * S // 4, S * S // 2, S * S // 4, 0, 0, 0]] and gf.hist(ref_tile, 4).tolist() == hist.tolist()
    radius = gap_radius(hist[0], GapFill())
    assert radius == 2
    for out in (ops.tile_gap_fill(tile, radius).cpu().numpy()[0], gf.fill(ref_tile, radius)[0]):
        assert (out.sum(axis=2) > 0).all(), 'no empty pixel is left'
        paint = out[..., 0] > 128
        assert paint[:, 40:44].all(), 'the paint covers its four columns'
        assert not paint[:, :39].any() and not paint[:, 45:].any(), 'the tie rule gives the brighter neighbour one pixel, no more'
    _eq(ops.tile_gap_fill(tile, radius), gf.fill(ref_tile, radius), 'the filled tile')


# ------------------------------------------------------------------------------------------------ 8. Runner
def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_runner_strip_fills_the_gaps(dev, net, tmp_path, monkeypatch):
    """Two overlapping axis-aligned 1152 x 1152 tiles over a strip with one point per 2 x 2 pixels.  density=None equals a call without
    the argument, file by file and call by call; density=GapFill() writes the reference's radii and histograms to params/density.json,
    submits the reference's filled tile and back-projects on it; GapFill(radius_px=0) submits the unfilled tile's bytes."""
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
    inten = np.floor(np.where(paint, rng.uniform(24000, 30000, len(x)), rng.uniform(3000, 7000, len(x))))
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
    assert rn.cfg.get('las_density') is None
    rastered, filled = [], []
    real_raster, real_fill = ops.bev_raster_batch, ops.tile_gap_fill

    def recording_raster(points, offs, rpar, H_, W_, **kw):
        out = real_raster(points, offs, rpar, H_, W_, **kw)
        rastered.append((kw, (out if kw.get('u8_only') else out[1]).cpu().numpy()))
        return out

    def recording_fill(tiles, radii):
        out = real_fill(tiles, radii)
        filled.append((list(radii), out, out.cpu().numpy()))
        return out

    monkeypatch.setattr(ops, 'bev_raster_batch', recording_raster)
    monkeypatch.setattr(ops, 'tile_gap_fill', recording_fill)
    submitted = []
    from lanemapping_amd import pipeline
    real_submit = pipeline.TilePipeline.submit
    monkeypatch.setattr(pipeline.TilePipeline, 'submit', lambda self, proj: (submitted.append(proj), real_submit(self, proj))[1])
    out = {k: str(tmp_path / k) for k in ('omitted', 'none', 'auto', 'zero')}
    rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['omitted'], batch_size=2)
    rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['none'], batch_size=2, density=None)
    assert len(rastered) == 2 and rastered[0][0] == {'want_u8': True} == rastered[1][0] and np.array_equal(rastered[0][1], rastered[1][1])
    assert not filled and all(s.dtype == torch.float32 for s in submitted), "without density= today's calls are made"
    files = _tree(out['omitted'])
    assert files == _tree(out['none']) and not any(f.startswith('params') for f in files)
    for f in files:
        assert open(os.path.join(out['omitted'], f), 'rb').read() == open(os.path.join(out['none'], f), 'rb').read(), f

    # the reference: the tile the numpy rasteriser makes of the points each tile holds, from the file as the reference reader decodes it
    host = las_ref.read_las_ref(las, shift=off, normalise=False).astype(f32)
    rps = [io_utils.raster_params_from_dict(p) for p in plist]
    held = [host[gr.window(host, rp, H, W)[0]] for rp in rps]
    ref_tiles = np.concatenate([ir.raster(h, [0, len(h)], [rp], H, W) for h, rp in zip(held, rps)])
    assert np.array_equal(rastered[0][1], ref_tiles) and (ref_tiles.sum(axis=3) == 0).mean() == 0.75
    fill = GapFill()
    ref_hist = gf.hist(ref_tiles, fill.max_radius_px)
    assert ref_hist.tolist() == [[H * W // 4, H * W // 2, H * W // 4, 0, 0, 0]] * 2

    for key, fill, want_r in (('auto', GapFill(), 2), ('zero', GapFill(radius_px=0), 0)):
        rastered.clear(), filled.clear(), submitted.clear()
        lines, _ = rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out[key], batch_size=2, density=fill)
        used = json.load(open(os.path.join(out[key], 'params', 'density.json')))
        assert used == {names[t]: [want_r] + ref_hist[t].tolist() for t in range(2)}, (key, used)
        assert len(rastered) == 1 and rastered[0][0] == {'u8_only': True} and np.array_equal(rastered[0][1], ref_tiles)
        assert len(filled) == 1 and filled[0][0] == [want_r, want_r] and len(submitted) == 1 and submitted[0] is filled[0][1], \
            'the filled u8 tile is what the pipeline gets'
        ref_filled = gf.fill(ref_tiles, want_r)
        assert np.array_equal(filled[0][2], ref_filled), f'{key}: the submitted tile is not the reference\'s'
        if want_r == 0:
            assert np.array_equal(filled[0][2], ref_tiles), 'radius 0 submits the unfilled tile'
        else:
            assert (ref_filled.sum(axis=3) > 0).all()
        assert [f for f in _tree(out[key]) if f.startswith('params')] == [os.path.join('params', 'density.json')]
        # every 3-D file is the back-projection of the written 2-D lines on the filled tile
        for t, name in enumerate(names):
            pc = os.path.join(out[key], 'out_pc_seq_json_dir', name + '.json')
            recs2d = io_utils.load_lane_seq(os.path.join(out[key], name + '.json'))
            lens = [int(n) for n in recs2d[1]]
            if len(lens) < 2:
                assert name not in lines and not os.path.exists(pc)
                continue
            seq2d = np.asarray(recs2d[0], dtype=np.float64)[:, :, :2]
            want = coor_img2pc.transform_coordinate_from_img_2_pc(plist[t], seq2d, lens, ref_filled[t])
            recs = [{'seq': want[i, :lens[i], :], 'seq_len': lens[i], 'init_vertex': want[i, 0, :], 'end_vertex': want[i, lens[i] - 1, :]}
                    for i in range(len(lens))]
            io_utils.save_seqs_json(recs, str(tmp_path / 'want.json'))
            assert open(tmp_path / 'want.json', 'rb').read() == open(pc, 'rb').read(), f'{key}: {name} is not back-projected on the filled tile'
            assert name in lines and len(lines[name]) == len(lens)
        assert len(lines) == 2, 'both tiles yield lanes: the back-projection above was compared'
        print(f'{key}: radius {want_r}, lines per tile {[len(lines.get(n, [])) for n in names]}')
