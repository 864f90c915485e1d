"""GPU: vertex heights from the points (csrc/drape.hip) - ops.drape_vertices against the numpy restatement of tests/drape_ref.py, compared
on bit patterns; guarded buffers; refusals; the accuracy on a crest; Runner.infer_las_strip_to_map with `elevation=`.

Sizes the kernels switch at (csrc/drape.hip): the window-minimum pass takes DCHUNK = 16,384 points per workgroup, the vertex index has
bands of 8 rows, the median pass takes one wave per vertex, four per workgroup."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import drape_ref as dr
import ground_ref as gr
from guards import NAN, Slab, guarded_runs
from lanemapping_amd import coor_img2pc, io_utils, ops
from lanemapping_amd._lib import LanemapHipError, LmRasterParams, check, lib
from lanemapping_amd.las_io import ElevationDrape

pytestmark = pytest.mark.gpu

f32 = np.float32
DCHUNK = 16384
S = 96                                                             # H = W of the small tiles
RESO = 0.0625                                                      # 1/16 m: every pixel border is exact in float32


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _same(got, want, name):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (name, g.shape, w.shape)
    assert np.array_equal(g, w), f'{name}: {int((g != w).sum())} of {g.size} words differ from the reference (first at {np.argwhere(g != w)[0].tolist()})'


def _check(dev, pts, offs, params, verts, voffs, R, name):
    """ops.drape_vertices == drape_ref in every bit of z, npix and pixel_min; a second call without pixel_min gives the same z and npix."""
    cloud = torch.from_numpy(pts).to(dev)
    z, npix, pmin = ops.drape_vertices(cloud, offs, params, verts, voffs, S, S, radius_px=R, want_pixel_min=True)
    rz, rn, rp = dr.drape_vertices(pts, offs, params, verts, voffs, S, S, R)
    _same(pmin, rp, f'{name}: pixel_min')
    assert np.array_equal(npix.cpu().numpy(), rn), f'{name}: npix'
    _same(z, rz, f'{name}: z')
    z2, n2 = ops.drape_vertices(cloud, offs, params, verts, voffs, S, S, radius_px=R)
    assert torch.equal(z2.view(torch.int32), z.view(torch.int32)) and torch.equal(n2, npix), f'{name}: two runs differ'
    return rz, rn, rp


def _axis_tile():
    return ops.make_raster_params(trans=(8.0, 16.0, 0.5), bev_img_offset=(-1.0, 0.5), img_reso=(RESO, RESO), local_min_ele=-1.0, ele_reso=0.02)


def _rot_tile(seed=7):
    rng = np.random.RandomState(seed)
    yaw = 0.4
    q = np.array([math.cos(yaw / 2), 0.013, -0.017, math.sin(yaw / 2)]) * 1.03
    return ops.make_raster_params(quat=q, trans=(40.0, 3.0, -0.25), bev_img_offset=rng.uniform(-1, 1, 2), img_reso=(0.05, 0.05),
                                  local_min_ele=-1.0, ele_reso=0.02)


def _far_tile():
    return ops.make_raster_params(trans=(4000.0, 4000.0, 0.0), img_reso=(RESO, RESO))


def _small_cloud(seed, n, p, spread=1.3):
    """n points around the window of tile p (a fifth outside it), heights 0.5 + a slope + noise, in the LAS frame of the tile."""
    rng = np.random.RandomState(seed)
    reso = float(p.img_reso[0])
    v = rng.uniform(-0.15 * S * reso, (spread - 0.15) * S * reso, (n, 2))
    vz = 0.5 + 0.05 * v[:, 0] + 0.03 * v[:, 1] + rng.normal(0, 0.05, n)
    q = np.array([float(c) for c in p.quat])
    nq = np.linalg.norm(q)
    w, x, y, z = q / nq
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    local = np.stack([v[:, 0] + p.bev_img_offset[0], v[:, 1] + p.bev_img_offset[1], vz], axis=1)
    world = (nq * Rm @ local.T).T + np.array([float(c) for c in p.trans])
    return np.ascontiguousarray(np.concatenate([world, np.floor(rng.uniform(500, 40000, (n, 1)))], axis=1), dtype=f32)


HOLE = (70, 20)                                                    # the vertex whose window holds no counted point
# corners; two identical vertices and one whose window overlaps theirs; four in one band of 8 rows; pairs in adjacent bands within R of
# the band border (rows 7 | 8 and 31 | 32); the hole; one more in the last band
VERTS = [(0, 0), (S - 1, S - 1), (40, 40), (40, 40), (40, 43), (16, 10), (17, 30), (18, 50), (23, 70), (7, 20), (8, 22), (31, 60), (32, 61),
         HOLE, (S - 1, 3)]


def _dig_hole(pts, p):
    """Every point within 10 pixels of HOLE loses its place: its z becomes NaN, +inf or -inf, or its x NaN, in turn."""
    on, row, col, _ = gr.window(pts, p, S, S)
    near = np.flatnonzero(on & (np.abs(row - HOLE[0]) <= 10) & (np.abs(col - HOLE[1]) <= 10))
    for k, i in enumerate(near):
        if k % 4 == 3:
            pts[i, 0] = np.nan
        else:
            pts[i, 2] = (np.nan, np.inf, -np.inf)[k % 4]
    return len(near)


# ------------------------------------------------------------------------------------------------ 1. counts, radii, placements
@pytest.mark.parametrize('R', [0, 4, 8])
def test_point_counts_radii_and_vertex_placements(dev, R):
    """Tile 0 axis-aligned with n points around the chunk size, tile 1 rotated and tilted, tile 2 without points (its vertices get NaN),
    tile 3 with points and without vertices."""
    axis, rot, far = _axis_tile(), _rot_tile(), _far_tile()
    rot_pts = _small_cloud(5, 3001, rot)
    rot_verts = [(0, 0), (50, 50), (51, 50), (S - 1, S - 1), (12, 80)]
    far_verts = [(3, 3), (90, 2)]
    verts = np.asarray(VERTS + rot_verts + far_verts, dtype=np.int32)
    voffs = [0, len(VERTS), len(VERTS) + len(rot_verts), len(verts), len(verts)]
    tail = _small_cloud(6, 700, axis)
    for n in (1, DCHUNK - 1, DCHUNK, DCHUNK + 1, 2 * DCHUNK + 300):
        a = _small_cloud(100 + n, n, axis)
        dug = _dig_hole(a, axis)
        pts = np.concatenate([a, rot_pts, tail])
        offs = [0, n, n + len(rot_pts), n + len(rot_pts), len(pts)]
        rz, rn, rp = _check(dev, pts, offs, [axis, rot, far, axis], verts, voffs, R, f'R={R} n={n}')
        assert rn[-2:].tolist() == [0, 0] and np.isnan(rz[-2:]).all(), 'the tile without points'
        if n >= DCHUNK - 1:
            hole = VERTS.index(HOLE)
            assert dug > 20 and rn[hole] == 0 and np.isnan(rz[hole]), 'the hole is empty'
            assert np.isnan(rp[0][:R]).all() and np.isnan(rp[0][:, :R]).all() and np.isnan(rp[1][R + 1:]).all(), 'corner windows are clipped'
            assert rz[2].view(np.uint32) == rz[3].view(np.uint32) and np.array_equal(rp[2].view(np.uint32), rp[3].view(np.uint32))
            if R:
                assert (rn[:hole] > 0).all() and np.isfinite(rz[len(VERTS):len(VERTS) + len(rot_verts)]).all()
                assert np.array_equal(rp[2][:, 3:].view(np.uint32), rp[4][:, :-3].view(np.uint32)), 'overlapping windows share their pixels'
    # one vertex in all, a point range that does not start at row 0, the tiles without work first
    pts = np.concatenate([_small_cloud(1, 700, far), rot_pts])
    _check(dev, pts, [700, 700, 700, 700 + len(rot_pts)], [far, axis, rot], np.asarray([(50, 50)], np.int32), [0, 0, 0, 1], R, f'R={R} one vertex')


def test_negative_zero_is_below_positive_zero(dev):
    """One pixel with the heights +0.0 and -0.0: the minimum is -0.0.  |q| = 2 halves every coordinate, so dz = -2^-149 becomes
    vz = -0.0 (round to even), and with dx, dy < 0 the two zero products in front of it are -0.0 as well."""
    p = ops.make_raster_params(quat=(2, 0, 0, 0), bev_img_offset=(-10.0, -10.0), img_reso=(RESO, RESO))
    tiny = np.array([1], np.uint32).view(f32)[0]
    pts = np.array([[-16.0, -16.0, 0.0, 900.0], [-16.0, -16.0, -tiny, 900.0], [-16.0, -16.0, 0.0, 900.0], [-15.9, -16.0, 0.25, 900.0]], dtype=f32)
    on, row, col, vz = gr.window(pts, p, S, S)
    assert on.all() and (row[:3] == 32).all() and (col[:3] == 32).all() and (row[3], col[3]) == (33, 32)
    assert vz[1] == 0 and np.signbit(vz[1]) and vz[0] == 0 and not np.signbit(vz[0]), 'the case holds both zeros'
    verts = np.asarray([(32, 32), (31, 31), (33, 32)], np.int32)
    for R in (0, 1):
        rz, rn, rp = _check(dev, pts, [0, 4], [p], verts, [0, 3], R, f'zeros R={R}')
        assert rp[0, R, R].view(np.uint32) == 0x80000000
    assert rn.tolist() == [2, 1, 2] and rz[0].view(np.uint32) == 0x80000000 and rz[1].view(np.uint32) == 0x80000000 and rz[2].view(np.uint32) == 0x80000000
    assert rp[2, 1, 1] == 0.125 and rp[2, 0, 1].view(np.uint32) == 0x80000000


def test_vertex_cap_on_one_tile(dev):
    """72 x 144 = 10,368 vertices on one tile (more than it has pixels: many are identical), one vertex on the next."""
    axis, rot = _axis_tile(), _rot_tile()
    a, b = _small_cloud(11, 5000, axis), _small_cloud(12, 900, rot)
    rng = np.random.RandomState(4)
    verts = np.concatenate([rng.randint(0, S, (72 * 144, 2)), [[47, 48]]]).astype(np.int32)
    rz, rn, _ = _check(dev, np.concatenate([a, b]), [0, len(a), len(a) + len(b)], [axis, rot], verts, [0, 72 * 144, 72 * 144 + 1], 4, 'cap')
    assert (rn > 0).all() and len(np.unique(rz.view(np.uint32))) > 1000


def test_empty_tile_between_two_tiles_across_the_chunk_seam(dev):
    """Three 64 x 64 tiles of 16,385 / 0 / 255 points - two workgroups, none, one - with vertices in the first and the last.  The last
    point of either range is the lowest of its pixel and a vertex sits on that pixel: the first tile's point 16,384 is alone in its
    tile's second chunk, and the third tile's workgroup follows the first tile's two, not the empty tile's none."""
    T, R = 64, 2
    tiles = [_axis_tile(), _far_tile(), _rot_tile()]
    clouds, verts, voffs = [], [], [0]
    for seed, n, p in ((51, DCHUNK + 1, tiles[0]), (0, 0, tiles[1]), (52, 255, tiles[2])):
        c = _small_cloud(seed, n, p, spread=0.85) if n else np.zeros((0, 4), f32)
        if n:
            c[-1] = c[np.flatnonzero(gr.window(c, p, T, T)[0])[0]]      # a place inside the window ...
            c[-1, 2] -= 1.0                                             # ... and a metre under everything else
            on, row, col, vz = gr.window(c, p, T, T)
            assert on[-1] and vz[-1] < vz[:-1][on[:-1]].min()
            verts += [(int(row[-1]), int(col[-1])), (0, 0), (T - 1, T - 1), (30, 33)]
        clouds.append(c)
        voffs.append(len(verts))
    pts = np.concatenate(clouds)
    offs = [0, DCHUNK + 1, DCHUNK + 1, DCHUNK + 1 + 255]
    verts = np.asarray(verts, np.int32)
    z, npix, pmin = ops.drape_vertices(torch.from_numpy(pts).to(dev), offs, tiles, verts, voffs, T, T, radius_px=R, want_pixel_min=True)
    rz, rn, rp = dr.drape_vertices(pts, offs, tiles, verts, voffs, T, T, R)
    _same(pmin, rp, 'seam: pixel_min')
    assert np.array_equal(npix.cpu().numpy(), rn), 'seam: npix'
    _same(z, rz, 'seam: z')
    for v, c, p in ((0, clouds[0], tiles[0]), (4, clouds[2], tiles[2])):
        assert rp[v, R, R].view(np.uint32) == gr.window(c[-1:], p, T, T)[3].view(np.uint32)[0], 'the last point of the range is its pixel\'s minimum'
        assert rn[v] > 1


# ------------------------------------------------------------------------------------------------ 2. guards and refusals
def _guard_case():
    axis, rot = _axis_tile(), _rot_tile()
    a, b = _small_cloud(41, DCHUNK + 257, axis), _small_cloud(42, 1500, rot)
    _dig_hole(a, axis)
    pts = np.concatenate([a, b])
    verts = np.asarray(VERTS + [(0, S - 1), (60, 60)], dtype=np.int32)
    return pts, [0, len(a), len(pts)], [axis, rot], verts, [0, len(VERTS), len(verts)]


def test_drape_vertices_guards(dev):
    """lm_drape_vertices with the points, every output and the workspace between guard slabs; the rows past V belong to the back guard."""
    L = lib()
    pts, offs, params, verts, voffs = _guard_case()
    B, V, R = len(params), len(verts), 4
    D = 2 * R + 1
    need = L.lm_drape_workspace_bytes(V, B, R)
    assert need > 0 and L.lm_drape_workspace_bytes(V, B, 9) == 0 and L.lm_drape_workspace_bytes(V, 4097, R) == 0 \
        and L.lm_drape_workspace_bytes(-1, B, R) == 0
    par, coffs, cvoffs = (LmRasterParams * B)(*params), (C.c_long * (B + 1))(*offs), (C.c_long * (B + 1))(*voffs)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(_, poisoned):
        s_pts = Slab(dev, len(pts), 4, front=64, back=64).fill_input(torch.from_numpy(pts), NAN if poisoned else 0.0)
        s_z = Slab(dev, V, 1, front=8, back=8).fill_canary()
        s_n = Slab(dev, V, 1, front=8, back=8, dtype=torch.int32).fill_canary()
        s_p = Slab(dev, V, D * D, front=2, back=2).fill_canary()
        s_ws = Slab(dev, 1, need, front=1, back=1, dtype=torch.uint8).fill_canary()
        rc = L.lm_drape_vertices(stream, C.c_void_p(s_pts.ptr()), coffs, par, B, S, S, C.c_void_p(verts.ctypes.data), cvoffs, R,
                                 C.c_void_p(s_ws.ptr()), need, C.c_void_p(s_z.ptr()), C.c_void_p(s_n.ptr()), C.c_void_p(s_p.ptr()))
        assert rc == 0, L.lm_last_error()
        return {'z': (s_z, V), 'npix': (s_n, V), 'pixel_min': (s_p, V), 'workspace': (s_ws, 1)}

    got = guarded_runs(run, 'drape_vertices', batch=False)
    rz, rn, rp = dr.drape_vertices(pts, offs, params, verts, voffs, S, S, R)
    _same(got['z'].reshape(V), rz, 'guards: z')
    assert np.array_equal(got['npix'].numpy().reshape(V), rn)
    _same(got['pixel_min'].reshape(V, D, D), rp, 'guards: pixel_min')


def test_bad_arguments_are_refused_and_nothing_is_launched(dev):
    L = lib()
    pts, offs, params, verts, voffs = _guard_case()
    B, V, R = len(params), len(verts), 4
    cloud = torch.from_numpy(pts).to(dev)
    need = L.lm_drape_workspace_bytes(V, B, R)
    ws = torch.empty(need, device=dev, dtype=torch.uint8)
    par = (LmRasterParams * B)(*params)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    canary = 0x7EADBEEF

    def call(offs_=offs, verts_=verts, voffs_=voffs, R_=R, ws_bytes=need):
        """The C entry with canaries in z and npix: -> (return code, the two outputs afterwards)."""
        v = np.ascontiguousarray(verts_, dtype=np.int32)
        z = torch.full((V,), canary, device=dev, dtype=torch.int32)
        n = torch.full((V,), canary, device=dev, dtype=torch.int32)
        rc = L.lm_drape_vertices(stream, C.c_void_p(cloud.data_ptr()), (C.c_long * (B + 1))(*offs_), par, B, S, S, C.c_void_p(v.ctypes.data),
                                 (C.c_long * (B + 1))(*voffs_), R_, C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(z.data_ptr()),
                                 C.c_void_p(n.data_ptr()), None)
        torch.cuda.synchronize()
        return rc, z.cpu().numpy(), n.cpu().numpy()

    rc, z, n = call()
    assert rc == 0 and (z != canary).all() and (n != canary).all(), 'the good call writes every row'
    outside = [verts.copy() for _ in range(4)]
    outside[0][3] = (S, 5)
    outside[1][3] = (5, S)
    outside[2][3] = (-1, 5)
    outside[3][V - 1] = (5, -1)
    cases = [(dict(verts_=v), 'outside') for v in outside] + [
        (dict(R_=-1), 'radius_px'), (dict(R_=9), 'radius_px'),
        (dict(offs_=[0, offs[1], offs[1] - 1]), 'tile_offsets'), (dict(voffs_=[0, V, V - 1]), 'vertex_offsets'),
        (dict(voffs_=[1, voffs[1], V]), 'vertex_offsets'), (dict(ws_bytes=need - 1), 'workspace too small')]
    for kw, word in cases:
        rc, z, n = call(**kw)
        with pytest.raises(LanemapHipError, match=word):
            check(rc)
        assert (z == canary).all() and (n == canary).all(), f'{word}: refused, yet something was written'
    # the Python layer raises the same errors
    with pytest.raises(LanemapHipError, match='outside'):
        ops.drape_vertices(cloud, offs, params, outside[0], voffs, S, S)
    with pytest.raises(LanemapHipError, match='radius_px'):
        ops.drape_vertices(cloud, offs, params, verts, voffs, S, S, radius_px=9)
    with pytest.raises(LanemapHipError, match='tile_offsets'):
        ops.drape_vertices(cloud, [0, 500, 400], params, verts, voffs, S, S)
    with pytest.raises(ValueError, match='vertex_offsets'):
        ops.drape_vertices(cloud, offs, params, verts, voffs[:-1], S, S)
    # nothing to do is not an error and launches nothing
    z, n = ops.drape_vertices(cloud, offs, params, np.zeros((0, 2), np.int32), [0, 0, 0], S, S)
    assert z.shape == (0,) and n.shape == (0,)
    z, n = ops.drape_vertices(cloud, [0], [], np.zeros((0, 2), np.int32), [0], S, S)
    assert z.shape == (0,)
    # B = 4096 is served: every tile but the last two without points and vertices
    many = [params[0]] * 4094 + params
    z, n = ops.drape_vertices(cloud, [0] * 4095 + offs[1:], many, verts, [0] * 4095 + voffs[1:], S, S, radius_px=R)
    rz, rn, _ = dr.drape_vertices(pts, offs, params, verts, voffs, S, S, R)
    _same(z, rz, 'B = 4096')
    assert np.array_equal(n.cpu().numpy(), rn)


# ------------------------------------------------------------------------------------------------ 3. accuracy on a crest
def test_crest_accuracy(dev):
    """The draped heights, back-projected without the line fit, lie within g (R + 1) reso sqrt 2 + one float32 ulp of the surface at every
    vertex (tests/drape_ref.py crest_bound).  tests/test_drape_cpu.py shows that the plain call on the same inputs breaks that bound."""
    params, kw, pts, seqs, lens, g = dr.crest_case()
    T, R = dr.CREST_S, dr.CREST_R
    rp = ops.make_raster_params(**kw)
    cloud = torch.from_numpy(pts).to(dev)
    _, u8 = ops.bev_raster_batch(cloud, [0, len(pts)], [rp], T, T, want_u8=True)
    tile = u8[0].cpu().numpy()
    assert (tile.sum(axis=2) > 0).all()
    verts = np.asarray([(int(seqs[l, v, 0]), int(seqs[l, v, 1])) for l in range(3) for v in range(lens[l])], np.int32)
    z, npix = ops.drape_vertices(cloud, [0, len(pts)], [rp], verts, [0, len(verts)], T, T, radius_px=R)
    rz, rn, _ = dr.drape_vertices(pts, [0, len(pts)], [rp], verts, [0, len(verts)], T, T, R)
    _same(z, rz, 'crest: z')
    assert np.array_equal(npix.cpu().numpy(), rn) and rn.min() >= (R + 1) * (2 * R + 1)
    vz = np.full(seqs.shape[:2], np.nan, f32)
    at = 0
    for l, n in enumerate(lens):
        vz[l, :n] = z.cpu().numpy()[at:at + n]
        at += n
    out = coor_img2pc.transform_coordinate_from_img_2_pc(params, seqs, lens, tile, vertex_z=vz, fit='none')
    err, bound = dr.crest_error(params, out, lens), dr.crest_bound(g)
    print(f'crest: worst |z - f| = {err.max():.4f} m, bound {bound:.4f} m')
    assert (err <= bound).all(), f'{int((err > bound).sum())} vertices off the crest by more than {bound:.4f} m (worst {err.max():.4f} m)'
    plain = dr.crest_error(params, coor_img2pc.transform_coordinate_from_img_2_pc(params, seqs, lens, tile), lens)
    assert (plain > bound).any(), 'the plain call breaks the bound on this crest'


# ------------------------------------------------------------------------------------------------ 4. Runner
def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_runner_strip_drapes_its_lanes(dev, net, tmp_path):
    """The strip of tests/test_gpu_ground.py's Runner test: three overlapping 1152 x 1152 tiles over a plane that climbs 12 m, one point at
    every pixel centre, six painted stripes.  elevation=None equals a call without the argument file by file, and those 3-D files are what
    the plain back-projection makes of the written 2-D files; with elevation=ElevationDrape() the 2-D files stay, params/elevation.json
    counts the vertices, and every 3-D line is drape_ref + the restated back-projection of the written 2-D line."""
    from lanemapping_amd.runner import Runner
    from oracle import las_ref
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
    plist, prm_paths, names = [], [], []
    for t in range(3):
        plist.append({'coor_las_path': '', 'las_read_offset': list(off), 'las_rotation_trans_quan': [t * step * reso, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0],
                      'bev_img_offset': [0.0, 0.0], 'img_reso': [reso, reso], 'local_min_ele': -0.5, 'ele_reso': ele})
        names.append(f'18102{t}_0209')
        prm_paths.append(str(tmp_path / (names[t] + '.txt')))
        io_utils.save_pc_2_img_transform_paras(prm_paths[t], plist[t])
    rn = Runner.__new__(Runner)
    rn.cfg, rn.device, rn.net = net.cfg, dev, net
    assert rn.cfg.get('las_elevation') is None
    out = {k: str(tmp_path / k) for k in ('omitted', 'none', 'drape')}
    rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['omitted'], batch_size=2)
    rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['none'], batch_size=2, elevation=None)
    drape = ElevationDrape()
    lines, merged = rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['drape'], batch_size=2, elevation=drape)
    files = _tree(out['omitted'])
    assert files == _tree(out['none']) and not any(f.startswith('params') for f in files)
    for f in files:
        assert open(os.path.join(out['omitted'], f), 'rb').read() == open(os.path.join(out['none'], f), 'rb').read(), f
    assert sorted(set(_tree(out['drape'])) - set(files)) == [os.path.join('params', 'elevation.json')]
    for name in names:
        f = name + '.json'
        assert open(os.path.join(out['omitted'], f), 'rb').read() == open(os.path.join(out['drape'], f), 'rb').read(), f'2-D file {f} changed'
    used = json.load(open(os.path.join(out['drape'], 'params', 'elevation.json')))
    assert sorted(used) == names and all(v[0] == v[1] + v[2] and min(v) >= 0 for v in used.values())
    assert lines and sorted(lines) == sorted(n for n in names if used[n][0] > 0), 'no tile yielded lines'

    host = las_ref.read_las_ref(las, shift=off, normalise=False).astype(f32)
    checked = 0
    for name, seqs3d in lines.items():
        t = names.index(name)
        rp = io_utils.raster_params_from_dict(plist[t])
        mine = host[gr.window(host, rp, H, W)[0]]
        seq2d, lens, _, _ = io_utils.load_lane_seq(os.path.join(out['drape'], name + '.json'))
        lens = [int(n) for n in lens]
        seq2d = np.asarray(seq2d, dtype=np.float64)[:, :, :2]
        verts = np.asarray([(int(seq2d[l, v, 0]), int(seq2d[l, v, 1])) for l in range(len(lens)) for v in range(lens[l])], np.int32)
        z, npix, _ = dr.drape_vertices(mine, [0, len(mine)], [rp], verts, [0, len(verts)], H, W, drape.radius_px)
        assert used[name] == [len(verts), len(verts), 0] and (npix >= drape.min_pixels).all(), 'one point per pixel: every vertex is draped'
        assert len(seqs3d) == len(lens)
        at = 0
        for l, n in enumerate(lens):
            want = dr.backproject_z(plist[t], seq2d[l, :n], dr.fit_line(z[at:at + n]))
            at += n
            assert np.array_equal(seqs3d[l].view(np.uint64), want.view(np.uint64)), f'{name} line {l}: not drape_ref + the back-projection'
            # on the plane: a draped height is the height of a pixel centre within R pixels of the vertex pixel, and the vertex lies less
            # than a pixel from that centre: E = (|A| + |B|) (R + 1) reso, + the LAS file's 1 mm grid (0.5 mm) + float32 z (2^-18 m at
            # 12 m).  The line fit z' = P z (P the projector onto span{1, i}) then leaves |z' - plane| <= max-row-sum(|P|) E + |(P - I) plane|
            truth = A * (seq2d[l, :n, 0] * reso + t * step * reso) + Bs * seq2d[l, :n, 1] * reso
            E = (abs(A) + abs(Bs)) * (drape.radius_px + 1) * reso + 0.0005 + 2.0 ** -18
            X = np.stack([np.ones(n), np.arange(n, dtype=np.float64)], axis=1)
            P = X @ np.linalg.inv(X.T @ X) @ X.T
            err = np.abs(seqs3d[l][:, 2] - off[2] - truth)
            assert (err <= np.abs(P).sum(axis=1).max() * E + np.abs(P @ truth - truth)).all(), f'{name} line {l}: off the plane by {err.max():.4f} m'
            checked += n
        # the run without elevation=: the plain back-projection of the same 2-D lines on the tile the rasteriser made
        _, u8 = ops.bev_raster_batch(torch.from_numpy(mine).to(dev), [0, len(mine)], [rp], H, W, want_u8=True)
        plain = coor_img2pc.transform_coordinate_from_img_2_pc(plist[t], seq2d, lens, u8[0].cpu().numpy())
        recs = [{'seq': plain[i, :lens[i], :], 'seq_len': lens[i], 'init_vertex': plain[i, 0, :], 'end_vertex': plain[i, lens[i] - 1, :]}
                for i in range(len(lens))]
        io_utils.save_seqs_json(recs, str(tmp_path / 'plain.json'))
        assert open(tmp_path / 'plain.json', 'rb').read() == open(os.path.join(out['omitted'], 'out_pc_seq_json_dir', name + '.json'), 'rb').read()
    assert checked > 0
