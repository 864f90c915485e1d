"""GPU: the per-tile ground model (csrc/ground.hip) - ops.tile_ground and ops.ground_select against the float32 numpy restatement of
tests/ground_ref.py, compared on bit patterns; guarded buffers; the effect on the rasterised tiles; Runner.infer_las_strip_to_map with
`ground=`.

Sizes the kernels switch at (csrc/ground.hip): the cell-minimum pass takes GCHUNK = 16,384 points per workgroup; the selection counts
blocks of SEL_BLOCK = 256 points, SEL_CHUNK = 2,048 points (8 blocks) per workgroup."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import ground_ref as gr
from guards import NAN, Slab, guarded_runs
from lanemapping_amd import io_utils, ops
from lanemapping_amd._lib import LanemapHipError, LmRasterParams, lib
from lanemapping_amd.las_io import GroundFilter, ground_datum

pytestmark = pytest.mark.gpu

f32 = np.float32
GCHUNK, SEL_BLOCK, SEL_CHUNK = 16384, 256, 2048


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _same(got, want, name):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (name, g.shape, w.shape)
    assert np.array_equal(g, w), f'{name}: {int((g != w).sum())} of {g.size} words differ from the reference (first at {np.argwhere(g != w)[0].tolist()})'


def _check_ground(dev, pts, offs, params, H, W, cell_px, name):
    ground, gmin, cmin = ops.tile_ground(torch.from_numpy(pts).to(dev), offs, params, H, W, cell_px=cell_px, want_cell_min=True)
    rg, rmin, rc = gr.tile_ground(pts, offs, params, H, W, cell_px)
    _same(cmin, rc, f'{name}: cell_min')
    _same(ground, rg, f'{name}: ground')
    _same(gmin, rmin, f'{name}: ground_min')
    g2, m2 = ops.tile_ground(torch.from_numpy(pts).to(dev), offs, params, H, W, cell_px=cell_px)
    assert torch.equal(g2.view(torch.int32), ground.view(torch.int32)) and torch.equal(m2.view(torch.int32), gmin.view(torch.int32))
    return ground, rg, rmin, rc


def _check_select(dev, pts, offs, params, ground, H, W, cell_px, h_range, name):
    out, o = ops.ground_select(torch.from_numpy(pts).to(dev), offs, params, ground, H, W, cell_px, h_range)
    want, woffs = gr.select(pts, offs, params, ground.cpu().numpy(), H, W, cell_px, h_range)
    assert o == woffs.tolist(), f'{name}: offsets {o} differ from the reference {woffs.tolist()}'
    assert tuple(out.shape) == want.shape
    _same(out, want, f'{name}: kept rows')
    return out, o


# ------------------------------------------------------------------------------------------------ clouds for the small grid
S = 96                                                             # H = W of the small grid
RESO = 0.0625                                                      # 1/16 m: every pixel and cell border is exact in float32


def _axis_tile():
    return ops.make_raster_params(trans=(8.0, 16.0, 0.5), bev_img_offset=(-1.0, 0.5), img_reso=(RESO, RESO), local_min_ele=-1.0, ele_reso=0.02)


def _rot_tile(seed=7):
    rng = np.random.RandomState(seed)
    yaw = 0.4
    q = np.array([math.cos(yaw / 2), 0.013, -0.017, math.sin(yaw / 2)]) * 1.03
    return ops.make_raster_params(quat=q, trans=(40.0, 3.0, -0.25), bev_img_offset=rng.uniform(-1, 1, 2), img_reso=(0.05, 0.05),
                                  local_min_ele=-1.0, ele_reso=0.02)


def _border_points(p, cell_px):
    """Axis-aligned tile: points exactly on, one ulp below and one ulp above every cell border and both window edges, along both axes, and
    points with NaN / +-Inf z in the middle of a cell."""
    out = []
    edges = [-0.5, S - 0.5] + [k * cell_px - 0.5 for k in range(1, -(-S // cell_px))]
    for e in edges:
        for axis in (0, 1):
            v = f32(e * RESO + p.bev_img_offset[axis] + p.trans[axis])
            for d in (np.nextafter(v, f32(-1e9)), v, np.nextafter(v, f32(1e9))):
                for k, other in enumerate((3.3, 47.2, 90.9)):
                    w = f32(other * RESO + p.bev_img_offset[1 - axis] + p.trans[1 - axis])
                    xy = (d, w) if axis == 0 else (w, d)
                    out.append([xy[0], xy[1], -3.0 - 0.01 * len(out), 1000.0])   # lower than any cloud point: each decides its cell
    mid = [f32(50.3 * RESO + p.bev_img_offset[a] + p.trans[a]) for a in (0, 1)]
    for z in (np.nan, np.inf, -np.inf):
        out.append([mid[0], mid[1], z, 1000.0])
    return np.asarray(out, dtype=f32)


def _small_cloud(seed, n, p, spread=1.3):
    """n points around the window of tile p (a fifth outside it), heights 0.5 + a slope + noise, in the LAS frame of the tile."""
    rng = np.random.RandomState(seed)
    reso = float(p.img_reso[0])
    v = rng.uniform(-0.15 * S * reso, (spread - 0.15) * S * reso, (n, 2))      # tile-frame x, y before the image offset
    vz = 0.5 + 0.05 * v[:, 0] + 0.03 * v[:, 1] + rng.normal(0, 0.05, n)
    q = np.array([float(c) for c in p.quat])
    nq = np.linalg.norm(q)
    w, x, y, z = q / nq
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    local = np.stack([v[:, 0] + p.bev_img_offset[0], v[:, 1] + p.bev_img_offset[1], vz], axis=1)
    world = (nq * R @ local.T).T + np.array([float(c) for c in p.trans])
    return np.ascontiguousarray(np.concatenate([world, np.floor(rng.uniform(500, 40000, (n, 1)))], axis=1), dtype=f32)   # row-major


# ------------------------------------------------------------------------------------------------ 1. small grid
@pytest.mark.parametrize('cell_px', [32, 40])
def test_small_grid_borders_nonfinite_and_chunk_sizes(dev, cell_px):
    """3 x 3 cells (cell_px 32) and a ragged last cell (cell_px 40: 40 + 40 + 16 pixels); tile 0 axis-aligned, tile 1 rotated and tilted,
    tile 2 empty; N of tile 0 around the block and chunk sizes of both kernels."""
    axis, rot = _axis_tile(), _rot_tile()
    far = ops.make_raster_params(trans=(4000.0, 4000.0, 0.0), img_reso=(RESO, RESO))
    rot_pts = _small_cloud(5, 3001, rot)
    border = _border_points(axis, cell_px)
    on, row, col, _ = gr.window(border, axis, S, S)
    assert on.any() and (~on[:-3]).any() and (row[on] == 0).any() and (row[on] == S - 1).any() and (col[on] == cell_px).any() \
        and (col[on] == cell_px - 1).any() and not on[-3:].any(), 'the border points straddle window edges and cell borders'
    for n in (0, 1, 255, 256, 257, SEL_CHUNK - 1, SEL_CHUNK, SEL_CHUNK + 1, GCHUNK - 1, GCHUNK, GCHUNK + 1, 2 * GCHUNK + 300):
        a = _small_cloud(100 + n, n, axis)
        if n >= len(border) + 300:
            a[200:200 + len(border)] = border                      # across a block border of the selection, order kept
        pts = np.concatenate([a, rot_pts])
        params, offs = [axis, rot, far], [0, n, n + len(rot_pts), n + len(rot_pts)]
        ground, rg, rmin, rc = _check_ground(dev, pts, offs, params, S, S, cell_px, f'cell_px={cell_px} n={n}')
        assert np.isnan(rg[2]).all() and rmin[2] == np.inf and np.isfinite(rg[1]).all(), 'the empty tile has no ground, the rotated one is full'
        if n >= len(border) + 300:
            assert np.isfinite(rc[0]).all() and (rc[0] < -2.9).sum() >= 4, 'border points decide their cells'
        if n == 0:
            assert np.isnan(rg[0]).all() and rmin[0] == np.inf
        _check_select(dev, pts, offs, params, ground, S, S, cell_px, (-0.05, 0.2), f'cell_px={cell_px} n={n} select')
    # the two empty tiles first and a point range that does not start at row 0
    pts = np.concatenate([_small_cloud(1, 700, far), rot_pts])
    ground, *_ = _check_ground(dev, pts, [700, 700, 700, 700 + len(rot_pts)], [far, axis, rot], S, S, cell_px, 'leading empty tiles')
    _check_select(dev, pts, [700, 700, 700, 700 + len(rot_pts)], [far, axis, rot], ground, S, S, cell_px, (-math.inf, 0.15), 'leading empty tiles')


# ------------------------------------------------------------------------------------------------ 2. shipped grid
def test_shipped_grid_outliers_vanish_and_holes_fill(dev):
    """1152 x 1152, 36 x 36 cells: 200 k points on a plane of 5 % + 3 % slope; isolated outlier cells (below: one noise return; above:
    every point of the cell raised, a lorry roof) at least 3 cells apart, and a hole of 2 x 2 cells without points."""
    H = W = 1152
    p = ops.make_raster_params(trans=(100.0, -20.0, 1.0), bev_img_offset=(0.5, -0.25), local_min_ele=-1.0, ele_reso=0.02)
    rng = np.random.RandomState(2)
    n = 200_000
    v = rng.uniform(0.0, 57.6, (n, 2))
    z = 2.0 + 0.05 * v[:, 0] + 0.03 * v[:, 1] + rng.normal(0, 0.02, n)
    pts = np.stack([v[:, 0] + 100.5, v[:, 1] - 20.25, z + 1.0, np.floor(rng.uniform(800, 9000, n))], axis=1).astype(f32)
    on, row, col, _ = gr.window(pts, p, H, W)
    cy, cx = row // 32, col // 32
    below, above, hole = [(3, 4), (10, 30), (20, 7), (35, 35)], [(6, 12), (15, 15), (28, 28), (0, 20)], (24, 18)
    for c in below:
        i = np.flatnonzero(on & (cy == c[0]) & (cx == c[1]))[0]
        pts[i, 2] -= 20.0
    for c in above:
        pts[on & (cy == c[0]) & (cx == c[1]), 2] += 3.0
    pts = pts[~(on & (cy >= hole[0]) & (cy < hole[0] + 2) & (cx >= hole[1]) & (cx < hole[1] + 2))]
    ground, rg, rmin, rc = _check_ground(dev, pts, [0, len(pts)], [p], H, W, 32, 'shipped')
    g = ground.cpu().numpy()[0]
    surface = 2.0 + 0.05 * (np.arange(36)[:, None] * 1.6) + 0.03 * (np.arange(36)[None, :] * 1.6)   # the plane at each cell's low corner
    assert np.isnan(rc[0, hole[0]:hole[0] + 2, hole[1]:hole[1] + 2]).all() and np.isfinite(g).all(), 'the hole has no minimum but a ground'
    for c in below:
        assert rc[0][c] < surface[c] - 15 and abs(g[c] - surface[c]) < 0.3, f'outlier below ground in cell {c} shows in ground'
    for c in above:
        assert rc[0][c] > surface[c] + 2.5 and abs(g[c] - surface[c]) < 0.3, f'outlier above ground in cell {c} shows in ground'
    assert np.abs(g - surface).max() < 0.3, 'ground follows the plane (cell minimum: below the surface by at most one cell of slope + noise)'
    assert float(rmin[0]) == float(np.nanmin(rg)) and abs(float(rmin[0]) - 2.0) < 0.3


# ------------------------------------------------------------------------------------------------ 3. selection
def test_select_variants_order_and_determinism(dev):
    """Two tiles adjacent in the buffer (5,000 and 2,049 + 777 points: several 256-blocks each, the second tile's range starting inside what
    would be the first tile's last block), an empty tile between them; both sides, one side infinite, nothing kept; the same bytes twice."""
    axis, rot = _axis_tile(), _rot_tile()
    far = ops.make_raster_params(trans=(4000.0, 4000.0, 0.0), img_reso=(RESO, RESO))
    a, b = _small_cloud(31, 5000, axis), _small_cloud(32, SEL_CHUNK + 1 + 777, rot)
    a[1000:1010, 2] += 2.0                                         # a sign above the road, marked by its intensity
    a[1000:1010, 3] = 111.0
    a[2000, 2] -= 2.0                                              # one noise return below: its cell's minimum, the median hides it
    a[2000, 3] = 222.0
    pts = np.concatenate([a, b])
    offs, params = [0, len(a), len(a), len(pts)], [axis, far, rot]
    ground, *_ = _check_ground(dev, pts, offs, params, S, S, 32, 'select input')
    cloud = torch.from_numpy(pts).to(dev)
    for h_range, some in (((-0.1, 0.25), True), ((0.05, math.inf), True), ((-math.inf, 0.1), True), ((50.0, 60.0), False)):
        out, o = _check_select(dev, pts, offs, params, ground, S, S, 32, h_range, f'h_range={h_range}')
        out2, o2 = ops.ground_select(cloud, offs, params, ground, S, S, 32, h_range)
        assert o == o2 and torch.equal(out.view(torch.int32), out2.view(torch.int32)), 'two runs differ'
        kept = np.diff(o)
        assert kept[1] == 0 and ((kept[0] > 100 and kept[2] > 100 and o[-1] < len(pts)) if some else o[-1] == 0), (h_range, o)
    both = ops.ground_select(cloud, offs, params, ground, S, S, 32, (-0.1, 0.25))[0].cpu().numpy()
    on = gr.window(a, axis, S, S)[0]
    assert on[1000:1010].sum() >= 3 and on[2000], 'the sign and the noise return lie inside the window'
    assert not np.isin(both[:, 3], (111.0, 222.0)).any(), 'the sign and the noise are gone'
    # the torch.ops entries give the same tensors
    from lanemapping_amd import torch_ops
    par = torch_ops.raster_params_tensor(params)
    g2, m2 = torch.ops.lanemap_hip.tile_ground(cloud, offs, par, S, S, 32)
    o3, f3 = torch.ops.lanemap_hip.ground_select(cloud, offs, par, g2, S, S, 32, -0.1, 0.25)
    assert torch.equal(g2.view(torch.int32), ground.view(torch.int32)) and np.array_equal(_bits(o3), _bits(both)) and f3.tolist()[-1] == len(both)


# ------------------------------------------------------------------------------------------------ 4. guards and refusals
def _guard_case():
    axis, rot = _axis_tile(), _rot_tile()
    a, b = _small_cloud(41, 2 * SEL_CHUNK + 257, axis), _small_cloud(42, 1500, rot)
    pts = np.concatenate([a, b])
    return pts, [0, len(a), len(pts)], [axis, rot]


def test_tile_ground_guards(dev):
    """lm_tile_ground with the points, every output and the workspace between guard slabs (cell_px 40: a ragged grid)."""
    L = lib()
    pts, offs, params = _guard_case()
    B, cell_px = len(params), 40
    Gy, Gx = gr.grid_shape(S, S, cell_px)
    need = L.lm_tile_ground_workspace_bytes(B, S, S, cell_px)
    assert need > 0 and L.lm_tile_ground_workspace_bytes(B, S, S, 7) == 0 and L.lm_tile_ground_workspace_bytes(4097, S, S, 32) == 0
    par, coffs = (LmRasterParams * B)(*params), (C.c_long * (B + 1))(*offs)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(_, poisoned):
        s_pts = Slab(dev, len(pts), 4, front=64, back=64).fill_input(torch.from_numpy(pts), NAN if poisoned else 0.0)
        s_g = Slab(dev, B * Gy, Gx, front=8, back=8).fill_canary()
        s_c = Slab(dev, B * Gy, Gx, front=8, back=8).fill_canary()
        s_m = Slab(dev, 1, B, front=8, back=8).fill_canary()
        s_ws = Slab(dev, 1, need, front=1, back=1, dtype=torch.uint8).fill_canary()
        rc = L.lm_tile_ground(stream, C.c_void_p(s_pts.ptr()), coffs, par, B, S, S, cell_px, C.c_void_p(s_ws.ptr()), need,
                              C.c_void_p(s_g.ptr()), C.c_void_p(s_m.ptr()), C.c_void_p(s_c.ptr()))
        assert rc == 0, L.lm_last_error()
        return {'ground': (s_g, B * Gy), 'cell_min': (s_c, B * Gy), 'ground_min': (s_m, 1), 'workspace': (s_ws, 1)}

    got = guarded_runs(run, 'tile_ground', batch=False)
    rg, rmin, rc_ = gr.tile_ground(pts, offs, params, S, S, cell_px)
    _same(got['ground'].reshape(B, Gy, Gx), rg, 'guards: ground')
    _same(got['cell_min'].reshape(B, Gy, Gx), rc_, 'guards: cell_min')
    _same(got['ground_min'].reshape(B), rmin, 'guards: ground_min')


def test_ground_select_guards(dev):
    """lm_ground_select likewise: rows of points_out from `kept` on stay untouched, the offsets sit between canaries."""
    L = lib()
    pts, offs, params = _guard_case()
    B, cell_px, h = len(params), 32, (-0.05, 0.2)
    rg, _, _ = gr.tile_ground(pts, offs, params, S, S, cell_px)
    want, woffs = gr.select(pts, offs, params, rg, S, S, cell_px, h)
    kept, N = int(woffs[-1]), len(pts)
    assert N // 4 < kept < N
    need = L.lm_ground_select_workspace_bytes(N, B)
    assert need > 0 and L.lm_ground_select_workspace_bytes(-1, B) == 0 and L.lm_ground_select_workspace_bytes(N, 0) == 0
    par, coffs = (LmRasterParams * B)(*params), (C.c_long * (B + 1))(*offs)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    host = (C.c_long * (B + 1))()

    def run(_, poisoned):
        s_pts = Slab(dev, N, 4, front=64, back=64).fill_input(torch.from_numpy(pts), NAN if poisoned else 0.0)
        s_g = Slab(dev, B * rg.shape[1], rg.shape[2], front=8, back=8).fill_input(torch.from_numpy(rg), NAN if poisoned else 0.0)
        s_out = Slab(dev, kept, 4, front=64, back=N - kept + 64).fill_canary()     # rows kept .. N-1 are part of the back guard
        s_off = Slab(dev, 1, 2 * (B + 1), front=8, back=8, dtype=torch.int32).fill_canary()
        s_ws = Slab(dev, 1, need, front=1, back=1, dtype=torch.uint8).fill_canary()
        rc = L.lm_ground_select(stream, C.c_void_p(s_pts.ptr()), coffs, par, B, S, S, cell_px, C.c_void_p(s_g.ptr()), h[0], h[1],
                                C.c_void_p(s_ws.ptr()), need, C.c_void_p(s_out.ptr()), C.c_void_p(s_off.ptr()), host)
        assert rc == 0, L.lm_last_error()
        assert list(host) == woffs.tolist()
        return {'out': (s_out, kept), 'offsets': (s_off, 1), 'workspace': (s_ws, 1)}

    for attempt in range(2):                                       # the second round: the same bits again
        got = guarded_runs(run, 'ground_select', batch=False)
        _same(got['out'], want, 'guards: kept rows')
        assert got['offsets'].numpy().view(np.int64).reshape(-1).tolist() == woffs.tolist()


def test_bad_arguments_are_refused_by_name(dev):
    pts, offs, params = _guard_case()
    cloud = torch.from_numpy(pts).to(dev)
    ground, _ = ops.tile_ground(cloud, offs, params, S, S, 32)
    for cell_px in (7, 129, 0):
        with pytest.raises(LanemapHipError, match='cell_px'):
            ops.tile_ground(cloud, offs, params, S, S, cell_px=cell_px)
    with pytest.raises(LanemapHipError, match='tile_offsets'):
        ops.tile_ground(cloud, [0, 500, 400], params, S, S)
    with pytest.raises(LanemapHipError, match='tile_offsets'):
        ops.ground_select(cloud, [0, 500, 400], params, ground, S, S, 32, (0.0, 1.0))
    with pytest.raises(LanemapHipError, match='h_lo'):
        ops.ground_select(cloud, offs, params, ground, S, S, 32, (float('nan'), 1.0))
    with pytest.raises(LanemapHipError, match='h_hi'):
        ops.ground_select(cloud, offs, params, ground, S, S, 32, (0.0, float('nan')))
    with pytest.raises(LanemapHipError, match='h_lo=1 > h_hi=0'):
        ops.ground_select(cloud, offs, params, ground, S, S, 32, (1.0, 0.0))
    with pytest.raises(LanemapHipError, match='cell_px'):
        ops.ground_select(cloud, offs, params, torch.zeros((2, 14, 14), device=dev), S, S, 7, (0.0, 1.0))
    with pytest.raises(LanemapHipError, match='B=4097'):
        ops.tile_ground(cloud, [0] * 4098, [params[0]] * 4097, S, S)
    with pytest.raises(ValueError, match='ground must be'):
        ops.ground_select(cloud, offs, params, ground[:, :2], S, S, 32, (0.0, 1.0))
    # B = 4096 is served: every tile but the last two empty
    many = [params[0]] * 4094 + params
    g, m = ops.tile_ground(cloud, [0] * 4095 + offs[1:], many, S, S)
    assert torch.equal(g[-2:].view(torch.int32), ground.view(torch.int32)) and bool(torch.isinf(m[:-2]).all()) and bool(torch.isnan(g[:-2]).all())
    out, o = ops.ground_select(cloud, [0] * 4095 + offs[1:], many, g, S, S, 32, (-0.05, 0.2))
    want, woffs = gr.select(pts, offs, params, ground.cpu().numpy(), S, S, 32, (-0.05, 0.2))
    assert o[-3:] == woffs.tolist() and o[:-3] == [0] * 4094
    _same(out, want, 'B = 4096')


# ------------------------------------------------------------------------------------------------ 5. the effect on the tiles
def _pixel_grid(T, p, z_of, inten_of):
    """One point at every pixel centre of the T x T tile p (axis-aligned): -> [T*T, 4] float32."""
    r, c = np.meshgrid(np.arange(T), np.arange(T), indexing='ij')
    x = r * float(p.img_reso[0]) + float(p.bev_img_offset[0]) + float(p.trans[0])
    y = c * float(p.img_reso[1]) + float(p.bev_img_offset[1]) + float(p.trans[1])
    return np.stack([x.ravel(), y.ravel(), z_of(r, c).ravel() + float(p.trans[2]), inten_of(r, c).ravel()], axis=1).astype(f32)


def test_datum_and_height_range_change_the_tiles_as_promised(dev):
    """Two 192 x 192 tiles 6 m apart in height at ele_reso 0.02 (G spans 5.1 m), a bright sheet 5 m above one painted lane of each."""
    T, ele = 192, 0.02
    road = lambda r, c: 0.01 * r * 0.05 + 0.02 * c * 0.05          # 1 % + 2 %
    inten = lambda r, c: np.where((c >= 90) & (c < 94), 24000.0, 3000.0 + 10.0 * ((r + c) % 50))
    tiles = [ops.make_raster_params(trans=(10.0 * t, 0.0, 0.0), local_min_ele=-0.5, ele_reso=ele) for t in range(2)]
    clouds, sheets = [], (slice(40, 120), slice(80, 104))
    for t, p in enumerate(tiles):
        g = _pixel_grid(T, p, lambda r, c: road(r, c) + 6.0 * t, inten)
        r, c = np.meshgrid(np.arange(T)[sheets[0]], np.arange(T)[sheets[1]], indexing='ij')
        sheet = g.reshape(T, T, 4)[r, c].reshape(-1, 4).copy()
        sheet[:, 2] += 5.0
        sheet[:, 3] = 32000.0
        clouds.append(np.concatenate([g, sheet]))
    pts = np.concatenate(clouds)
    offs = [0, len(clouds[0]), len(pts)]
    cloud = torch.from_numpy(pts).to(dev)
    under = np.zeros((T, T), bool)
    under[sheets] = True

    # the defect: one datum for both tiles pins G of the upper one
    _, u8 = ops.bev_raster_batch(cloud, offs, tiles, T, T, want_u8=True)
    u8 = u8.cpu().numpy()
    filled = u8.sum(axis=3) > 0
    assert filled.all() and (u8[1][..., 1] == 255).sum() > filled[1].sum() // 2, 'strip-wide datum: G of the upper tile is saturated'
    assert (u8[0][..., 1][~under] < 255).all()

    # a datum under every tile's own ground
    ground, gmin = ops.tile_ground(cloud, offs, tiles, T, T, cell_px=32)
    rg, rmin, _ = gr.tile_ground(pts, offs, tiles, T, T, 32)
    _same(ground, rg, 'effect: ground')
    _same(gmin, rmin, 'effect: ground_min')
    datum = [ground_datum(m, ele, 1.0, -0.5) for m in gmin.cpu().numpy()]
    assert abs(datum[1] - datum[0] - 6.0) < 2 * ele and datum[0] <= -1.0
    mine = [LmRasterParams.from_buffer_copy(p) for p in tiles]
    for p, d in zip(mine, datum):
        p.local_min_ele = d
    _, u8 = ops.bev_raster_batch(cloud, offs, mine, T, T, want_u8=True)
    u8 = u8.cpu().numpy()
    for t in range(2):
        _, row, col, vz = gr.window(clouds[t][:T * T], mine[t], T, T)
        want = np.floor((vz - f32(mine[t].local_min_ele)) * (f32(1.0) / f32(ele)) + f32(0.5)).reshape(T, T)
        G = u8[t][..., 1]
        assert np.array_equal(G[~under], want[~under].astype(np.uint8)), f'tile {t}: G is not round((z - datum) / ele_reso)'
        assert G[~under].min() >= 1 and G[~under].max() <= 254 and want[~under].min() >= 50 - 1, (G.min(), G.max())
        assert (u8[t][..., 0][under] == round((32000.0 - 800.0) * 255.0 / 33000.0)).all(), 'without a height range the sheet wins its pixels'

    # only what lies within -0.5 .. 1.0 m of the ground is rasterised: the paint under the sheet shows
    sel, soffs = ops.ground_select(cloud, offs, mine, ground, T, T, 32, (-0.5, 1.0))
    assert soffs == [0, T * T, 2 * T * T], 'exactly the sheets are gone'
    _, u8s = ops.bev_raster_batch(sel, soffs, mine, T, T, want_u8=True)
    u8s = u8s.cpu().numpy()
    r, c = np.meshgrid(np.arange(T), np.arange(T), indexing='ij')
    want_I = np.clip(np.floor((np.clip(inten(r, c), 800.0, 33000.0).astype(f32) - f32(800.0)) * (f32(255.0) / f32(33000.0)) + f32(0.5)), 1, 255)
    for t in range(2):
        assert np.array_equal(u8s[t][..., 0], want_I.astype(np.uint8)), f'tile {t}: the pixels under the sheet do not carry the road intensity'
        assert np.array_equal(u8s[t][..., 1][~under], u8[t][..., 1][~under]) and (u8s[t][..., 1][under] < 120).all()


# ------------------------------------------------------------------------------------------------ 6. Runner
def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_runner_strip_follows_the_terrain(dev, net, tmp_path):
    """Three overlapping axis-aligned 1152 x 1152 tiles over a strip that climbs 12 m (7.5 % along the strip, 2 % across), one point at
    every pixel centre, six painted stripes.  ground=None equals a call without the argument, file by file; ground=GroundFilter() writes
    per-tile datums = ground_datum(reference ground_min) and every back-projected vertex lies on the plane."""
    from lanemapping_amd.runner import Runner
    from oracle import las_ref
    H = W = 1152
    reso, ele, A, Bs = 0.05, 0.05, 0.075, 0.02
    off = np.array([351200.0, 3433000.0, 12.0])
    step = 1024                                                    # pixels between tile origins: 128 shared
    rows = 2 * step + H
    r, c = np.meshgrid(np.arange(rows), np.arange(W), indexing='ij')
    x, y = (r * reso).ravel(), (c * reso).ravel()
    plane = lambda x_, y_: A * x_ + Bs * y_
    lane_y = [(0.12 + 0.152 * l) * 57.6 + 0.01 * (l - 2.5) * x for l in range(6)]
    paint = np.zeros(len(x), bool)
    for ly in lane_y:
        paint |= np.abs(y - ly) < 0.075
    inten = np.where(paint, 24000.0, 3000.0 + 40.0 * ((r + 3 * c) % 97).ravel())
    world = np.stack([x, y, plane(x, y)], axis=1)
    order = np.random.RandomState(3).permutation(len(world))      # not tile by tile, not row by row
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
    assert rn.cfg.get('las_ground') is None
    out = {k: str(tmp_path / k) for k in ('omitted', 'none', 'ground')}
    rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['omitted'], batch_size=2)
    rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['none'], batch_size=2, ground=None)
    lines, merged = rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['ground'], batch_size=2, ground=GroundFilter())
    files = _tree(out['omitted'])
    assert files == _tree(out['none']) and not any(f.startswith('params') for f in files)
    for f in files:
        assert open(os.path.join(out['omitted'], f), 'rb').read() == open(os.path.join(out['none'], f), 'rb').read(), f

    # the datums: from the reference's ground model of the points each tile holds
    host = las_ref.read_las_ref(las, shift=off, normalise=False).astype(f32)
    datums = []
    for t in range(3):
        rp = io_utils.raster_params_from_dict(plist[t])
        keep = gr.window(host, rp, H, W)[0]
        assert keep.sum() == H * W
        _, rmin, _ = gr.tile_ground(host[keep], [0, int(keep.sum())], [rp], H, W, 32)
        used = io_utils.load_pc_2_img_transform_paras(os.path.join(out['ground'], 'params', names[t] + '.txt'))
        assert used['local_min_ele'] == ground_datum(rmin[0], ele, 1.0, -0.5), f'tile {t}: datum'
        assert {k: v for k, v in used.items() if k != 'local_min_ele'} == {k: v for k, v in plist[t].items() if k != 'local_min_ele'}
        datums.append(used['local_min_ele'])
    assert datums[0] < datums[1] < datums[2] and abs(datums[2] - datums[0] - 2 * step * reso * A) < 2 * ele

    # every vertex on the plane.  A vertex (row, col) reads G of pixel (int row, int col), whose one point sits at that pixel's centre:
    #   quantisation     G = round((z - datum) / ele_reso): ele_reso / 2, + the LAS file's 1 mm grid (0.5 mm) + float32 z (2^-18 m at 12 m)
    #   pixel footprint  nothing here (the point is at the centre); in general half a pixel along each axis
    #   truncation       int() moves the look-up by less than one pixel along each axis: reso * (|A| + |B|)
    # so each looked-up z is within E of the plane at the vertex.  The back-projection then replaces the z of a line by their
    # least-squares line over the vertex INDEX, z' = P z with P the projector onto span{1, i}: z' - plane = P e + (P - I) plane, at most
    # max-row-sum(|P|) * E + |(P - I) plane|, the second term being how far the plane along this polyline is from linear in the index.
    E = ele / 2 + 0.0005 + 2.0 ** -18 + reso * (abs(A) + abs(Bs))
    assert lines, 'no tile yielded lines'
    checked = 0
    for name, seqs3d in lines.items():
        seq2d, lens, _, _ = io_utils.load_lane_seq(os.path.join(out['ground'], name + '.json'))
        t = names.index(name)
        assert len(seqs3d) == len(lens)
        for l, z3 in enumerate(seqs3d):
            n = lens[l]
            vx = seq2d[l, :n, 0] * reso + t * step * reso
            vy = seq2d[l, :n, 1] * reso
            truth = plane(vx, vy)
            X = np.stack([np.ones(n), np.arange(n, dtype=np.float64)], axis=1)
            P = X @ np.linalg.inv(X.T @ X) @ X.T
            bound = np.abs(P).sum(axis=1).max() * E + np.abs(P @ truth - truth)
            err = np.abs((z3[:n, 2] - off[2]) - truth)
            assert (err <= bound).all(), f'{name} line {l}: vertex z off the plane by {err.max():.4f} m (bound {bound.max():.4f})'
            assert np.allclose(z3[:n, 0] - off[0], vx, atol=1e-6) and np.allclose(z3[:n, 1] - off[1], vy, atol=1e-6)
            checked += n
    assert checked > 0
