"""GPU tests (-m gpu) of the four index kernels under the sparse-voxel LiDAR encoder (csrc/lidar.hip): lm_voxelize_hard,
lm_sparse_grid_build, lm_sparse_conv_outputs, lm_sparse_rulebook.

They produce integers (and fp32 means summed in a fixed order), so everything here is held to EQUALITY: coordinates, row order, grids,
counts and every rulebook word against the brute-force references of tests/sparse_ref.py (checked on the CPU against the dense conv3d
formulation by tests/test_sparse_index_ref_cpu.py), the voxeliser against oracle/lidar_ref.py::voxelize_ref with bit-equal means (both
sum in fp32 in point-index order and divide once; lidar.hip is built without fp contraction, and bit-equality held on the MI355X in every
case of this file the first time it ran).  Every case runs twice and must repeat bit for bit; raw calls write into canary slabs (tests/guards.py).  The only tolerance is the 1e-5 of
test_conv_gather_vs_fp64, where the device rulebook is tied to a float64 conv3d through lm_conv_gather_mfma_f32."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lds_state
import sparse_ref as R
from gpu_common import _chk, _close, _lib, _s
from guards import CANARY, Slab, _signed

pytestmark = pytest.mark.gpu

I32_CANARY = _signed(CANARY[torch.int32], torch.int32)
F32_CANARY = _signed(CANARY[torch.float32], torch.float32)          # the fp32 canary read as int32 bits


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same_f32(got, ref, name):
    """Bit-equal fp32 arrays; a NaN matches a NaN (sign and payload of a NaN are not defined by the arithmetic)."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bad = (_bits(got) != _bits(ref)) & ~(np.isnan(got) & np.isnan(ref))
    if bad.any():
        with np.errstate(invalid='ignore'):
            err = float(np.nanmax(np.abs(got.astype(np.float64) - ref.astype(np.float64))[bad]))
        r = int(np.argwhere(bad)[0][0])
        raise AssertionError(f'{name}: {int(bad.sum())} of {bad.size} fp32 words differ in their bits (max abs diff {err:.3e}); first in row '
                             f'{r}: got {got[r].tolist()}, want {ref[r].tolist()}')


def _key(c, grid_xyz):
    c = np.asarray(c, np.int64)
    return ((c[:, 0] * grid_xyz[2] + c[:, 1]) * grid_xyz[1] + c[:, 2]) * grid_xyz[0] + c[:, 3]


def _dev_pts(pts, dev):
    return [torch.from_numpy(np.ascontiguousarray(p, np.float32).reshape(-1, 4)).to(dev) for p in pts]


def _vox_case(dev, pts, lo, vs, grid, max_points, max_voxels, name, ref_pts=None):
    """ops.voxelize_batch in both row orders, twice each, against voxelize_ref of `ref_pts` (default: the same points)."""
    from lanemapping_amd import ops
    from oracle import lidar_ref
    with np.errstate(invalid='ignore'):                                   # the oracle casts NaN / huge cells to int64 on its way to dropping them
        f_ref, c_ref = lidar_ref.voxelize_ref(pts if ref_pts is None else ref_pts, lo, vs, grid, max_points, max_voxels)
    ends_ref = np.cumsum([int((c_ref[:, 0] == b).sum()) for b in range(len(pts))]).tolist()
    order = np.argsort(_key(c_ref, grid), kind='stable')
    d = _dev_pts(pts, dev)
    for raster in (False, True):
        tag = f'{name} [{"raster" if raster else "first-appearance"} order]'
        f, c, ends = ops.voxelize_batch(d, lo, vs, grid, max_points, max_voxels, raster_order=raster)
        f2, c2, ends2 = ops.voxelize_batch(d, lo, vs, grid, max_points, max_voxels, raster_order=raster)
        fn, cn = f.cpu().numpy(), c.cpu().numpy()
        assert ends == ends2 and np.array_equal(cn, c2.cpu().numpy()) and np.array_equal(_bits(fn), _bits(f2.cpu().numpy())), \
            f'{tag}: the second run differs from the first'
        want_c, want_f = (c_ref[order], f_ref[order]) if raster else (c_ref, f_ref)
        assert ends == ends_ref, f'{tag}: row_end chain {ends}, want {ends_ref}'
        assert cn.shape == want_c.shape and cn.dtype == np.int32 and np.array_equal(cn, want_c), f'{tag}: coords differ from the oracle'
        if raster:
            assert np.all(np.diff(_key(cn, grid)) > 0), f'{tag}: rows not strictly ascending in (b, z, y, x)'
        _same_f32(fn[:, :4], want_f, tag + ' means')
        assert not _bits(fn[:, 4:]).any(), f'{tag}: channels 4.. are not zero'
    return f_ref, c_ref


def _mid(lo, vs, cell):
    """Centre of cell index `cell` along one axis, float64."""
    return np.float64(lo) + (np.float64(cell) + 0.5) * np.float64(vs)


# ================================================================================================ lm_voxelize_hard
def test_voxelize_cell_edges_real_geometry(dev):
    """The network's own geometry (575 x 575 x 9 cells of 30/575 x 50/575 x 4/9): for every axis and every k in 0..grid the fp32 value
    lo + k * vs and its two fp32 neighbours, the other two coordinates mid-cell; 3486 points, shuffled.  Holds the lower edge (kept), the
    upper edge (dropped) and one ulp either side of both, and fails if floor((p - lo) / vs) is computed any other way than with the
    correctly rounded fp32 subtract and divide (a multiply by 1 / vs moves 512 of the 1728 x-edge points into the neighbouring cell)."""
    from oracle import lidar_ref
    lo, vs, grid = lidar_ref.voxel_geometry([-15., -25., -2., 15., 25., 2.], grid_shape=[576, 576, 10])
    assert grid == [575, 575, 9]
    pts = []
    for a in range(3):
        for k in range(grid[a] + 1):
            e = np.float32(np.float64(lo[a]) + k * np.float64(vs[a]))
            for v in (np.nextafter(e, np.float32(-np.inf)), e, np.nextafter(e, np.float32(np.inf))):
                p = [_mid(lo[b], vs[b], (k * 7 + 3 + b) % grid[b]) for b in range(3)]
                p[a] = v
                pts.append(p + [k % 11 / 10.0])
    pts = np.asarray(pts, np.float32)
    assert len(pts) == 3 * (576 + 576 + 10)
    pts = pts[np.random.RandomState(5).permutation(len(pts))]
    _, c_ref = _vox_case(dev, [pts], lo, vs, grid, 10, 100000, 'cell edges')
    assert c_ref[:, 3].min() == 0 and c_ref[:, 3].max() == 574 and c_ref[:, 1].min() == 0 and c_ref[:, 1].max() == 8


def _small_geom():
    return [-3.0, -2.0, -1.0], [0.5, 0.25, 0.5], [12, 10, 4]            # lo, voxel size, grid (x, y, z)


def test_voxelize_nonfinite_coordinates_are_dropped(dev):
    """NaN, +Inf, -Inf and +-1e30 in each of x, y, z, the other two coordinates inside cell 0 of their axes, mixed among ordinary points
    of which many lie in cell 0 of an axis and some in cell (0, 0, 0).  The device result must equal the oracle on ALL points and the
    oracle on the ordinary points alone: the bad points produce no voxel and change no voxel's mean or number.  A second sample holds
    bad points only and contributes no row.  A NaN intensity on finite coordinates stays in the mean of its own voxel.

    Measured on the MI355X before the range test moved onto the float in vox_keys_kernel: (int)floorf(NaN) == 0, so a point with a NaN
    x, y or z landed in cell 0 of that axis - a lone such point produced the voxel (0, 0, 0) with a NaN mean, one among ordinary points
    of that cell turned their mean into NaN, and the sample of bad points alone here produced one row (row_end chain [267, 268, 315]
    for [267, 267, 314]).  +-Inf and +-1e30 were already dropped: the conversion saturates them out of range."""
    lo, vs, grid = _small_geom()
    rng = np.random.RandomState(11)
    n = 400
    good = np.empty((n, 4), np.float32)
    for a in range(3):
        good[:, a] = lo[a] + rng.rand(n) * grid[a] * vs[a] * 0.998 + 0.001 * vs[a]
    good[:, 3] = rng.rand(n)
    for a in range(3):                                                    # 40 points in cell 0 of each axis ...
        good[40 * a:40 * a + 40, a] = lo[a] + (0.1 + 0.8 * rng.rand(40)) * vs[a]
    for a in range(3):                                                    # ... and 12 in cell (0, 0, 0)
        good[120:132, a] = lo[a] + (0.1 + 0.8 * rng.rand(12)) * vs[a]
    good = good[rng.permutation(n)]
    bad = []
    for a in range(3):
        for v in (np.nan, np.inf, -np.inf, 1e30, -1e30):
            p = [lo[b] + 0.5 * vs[b] for b in range(3)] + [0.5]
            p[a] = v
            bad.append(p)
    bad.append([np.nan, np.nan, np.nan, 0.5])
    bad = np.asarray(bad, np.float32)
    is_bad = np.zeros(n + len(bad), bool)
    is_bad[np.r_[0, n + len(bad) - 1, rng.choice(np.arange(1, n + len(bad) - 1), len(bad) - 2, replace=False)]] = True
    mixed = np.empty((n + len(bad), 4), np.float32)
    mixed[is_bad], mixed[~is_bad] = bad, good
    ordinary = mixed[~is_bad]
    third = good[:50].copy()
    pts = [mixed, bad, third]
    f_all, c_all = _vox_case(dev, pts, lo, vs, grid, 10, 100000, 'non-finite vs oracle(all points)')
    f_ord, c_ord = _vox_case(dev, pts, lo, vs, grid, 10, 100000, 'non-finite vs oracle(ordinary points)',
                             ref_pts=[ordinary, np.zeros((0, 4), np.float32), third])
    assert np.array_equal(c_all, c_ord) and np.array_equal(_bits(f_all), _bits(f_ord))
    assert not np.isnan(f_all).any() and (c_all[:, 0] != 1).all() and (c_all[:, 1:] == 0).all(axis=1).any()
    # NaN intensity: two such points in cell (x 5, y 5, z 2), which holds a point of finite intensity too
    tgt = [_mid(lo[0], vs[0], 5), _mid(lo[1], vs[1], 5), _mid(lo[2], vs[2], 2)]
    inten = np.insert(mixed, [50, 100, 300], np.asarray([tgt + [0.25], tgt + [np.nan], tgt + [np.nan]], np.float32), axis=0)
    f_i, c_i = _vox_case(dev, [inten, bad], lo, vs, grid, 10, 100000, 'NaN intensity')
    nan_rows = np.isnan(f_i).any(axis=1)
    assert nan_rows.sum() == 1 and c_i[nan_rows][0].tolist() == [0, 2, 5, 5]
    assert np.isnan(f_i[nan_rows][0, 3]) and not np.isnan(f_i[nan_rows][0, :3]).any()


def _capped_cloud():
    """Voxels holding 1, 3, 4 and 50 points plus ten more holding 2 each, interleaved in index order (seeded shuffle)."""
    lo, vs, grid = _small_geom()
    rng = np.random.RandomState(23)
    cells = [((1, 1, 1), 1), ((11, 9, 3), 3), ((0, 0, 0), 4), ((6, 4, 2), 50)] + [((2 + i, i, i % 4), 2) for i in range(10)]
    pts = []
    for (cx, cy, cz), cnt in cells:
        for _ in range(cnt):
            pts.append([lo[0] + (cx + 0.05 + 0.9 * rng.rand()) * vs[0], lo[1] + (cy + 0.05 + 0.9 * rng.rand()) * vs[1],
                        lo[2] + (cz + 0.05 + 0.9 * rng.rand()) * vs[2], rng.rand()])
    pts = np.asarray(pts, np.float32)
    return lo, vs, grid, pts[rng.permutation(len(pts))], len(cells)


@pytest.mark.parametrize('max_points', [1, 3])
@pytest.mark.parametrize('max_voxels', [1, 7, 1000])
def test_voxelize_caps(dev, max_points, max_voxels):
    """max_points below / at / above the occupancy of voxels with 1, 3, 4 and 50 points: the mean is of the first max_points by index.
    max_voxels below the 14 voxels: the kept set is the first-appearance one in both row orders and row_end equals the cap."""
    lo, vs, grid, pts, n_vox = _capped_cloud()
    _, c_ref = _vox_case(dev, [pts], lo, vs, grid, max_points, max_voxels, f'caps {max_points}/{max_voxels}')
    assert len(c_ref) == min(max_voxels, n_vox)                           # _vox_case holds row_end to this count in both row orders


@pytest.mark.parametrize('max_points', [1, 3, 10000])
def test_voxelize_all_points_in_one_voxel(dev, max_points):
    lo, vs, grid = _small_geom()
    rng = np.random.RandomState(3)
    pts = np.stack([lo[0] + (7 + rng.rand(5000)) * vs[0], lo[1] + (3 + rng.rand(5000)) * vs[1], lo[2] + (1 + rng.rand(5000)) * vs[2],
                    rng.rand(5000)], axis=1).astype(np.float32)
    pts[:, :3] = np.clip(pts[:, :3], np.float32([lo[0] + 7.001 * vs[0], lo[1] + 3.001 * vs[1], lo[2] + 1.001 * vs[2]]),
                         np.float32([lo[0] + 7.999 * vs[0], lo[1] + 3.999 * vs[1], lo[2] + 1.999 * vs[2]]))
    _, c_ref = _vox_case(dev, [pts], lo, vs, grid, max_points, 100, f'one voxel, max_points {max_points}')
    assert c_ref.tolist() == [[0, 1, 3, 7]]


# cells = 255, 256 (8-bit keys full / one over), 65535, 65536, 2^24 - 1, 2^24, and 65536 x 65535 x 1 whose largest key 0xFFFEFFFF lies
# just under the all-ones invalid key.  The voxeliser allocates nothing of grid size.
KEY_GRIDS = [(15, 17, 1), (16, 4, 4), (255, 257, 1), (256, 16, 16), (4095, 4097, 1), (256, 256, 256), (65536, 65535, 1)]


@pytest.mark.parametrize('grid', KEY_GRIDS, ids=lambda g: 'x'.join(str(v) for v in g))
def test_voxelize_sort_key_width(dev, grid):
    """Unit voxels from the origin, so a point (cx + u, cy + v, cz + w) lies in cell (cx, cy, cz) exactly.  n in {1, 255, 256, 257, 1000}
    points cycling through: outside, cell 0, the last cell, a middle cell, outside again; the first and the last point are outside.  The
    radix sort takes only the bits a cell index can have: the invalid key must still sort last and never merge with the last cell."""
    gx, gy, gz = grid
    cells = gx * gy * gz
    lo, vs = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    mid = cells // 2
    targets = {1: (0, 0, 0), 2: (gx - 1, gy - 1, gz - 1), 3: (mid % gx, mid // gx % gy, mid // (gx * gy))}
    outside = [(gx + 0.5, 0.5, 0.5), (-0.5, gy - 0.5, gz - 0.5), (gx - 0.5, gy + 0.5, gz - 0.5), (gx - 0.5, gy - 0.5, gz + 0.5),
               (0.5, 0.5, -0.5), (0.5, -1e-6, 0.5)]
    rng = np.random.RandomState(cells % 9973)
    for n in (1, 255, 256, 257, 1000):
        kind = np.arange(n) % 5                                          # 0 and 4: outside
        kind[0], kind[-1] = (0, 0) if n > 1 else (2, 2)                  # a single point: the last cell
        pts = np.empty((n, 4), np.float32)
        for i in range(n):
            if kind[i] in targets:
                pts[i, :3] = np.asarray(targets[kind[i]], np.float64) + 0.25 + 0.5 * rng.rand(3)
            else:
                pts[i, :3] = outside[i % len(outside)]
            pts[i, 3] = rng.rand()
        _, c_ref = _vox_case(dev, [pts], lo, vs, grid, 1000, 100000, f'grid {grid} n {n}')
        want = sorted({tuple(reversed(targets[k])) for k in set(kind.tolist()) if k in targets})
        assert sorted(tuple(r[1:]) for r in c_ref.tolist()) == want


def _vox_raw(dev, pts, lo, vs, grid, max_points, max_voxels, batch_idx, row_base, cap_rows, feats, ldf, coords, row_end, raster):
    """One raw lm_voxelize_hard call.  pts: device [n,4] or None; feats / coords: Slabs; row_base / row_end: one-element device views."""
    n = 0 if pts is None else pts.shape[0]
    need = _lib().lm_voxelize_workspace_bytes(n)
    ws = torch.empty((need,), device=dev, dtype=torch.uint8)
    _chk(_lib().lm_voxelize_hard(_s(), pts.data_ptr() if n else None, n, (C.c_float * 3)(*lo), (C.c_float * 3)(*vs), (C.c_int * 3)(*grid),
                                 max_points, max_voxels, batch_idx, None if row_base is None else row_base.data_ptr(), cap_rows,
                                 feats.ptr(), ldf, coords.ptr(), row_end.data_ptr(), int(raster), ws.data_ptr(), need))
    torch.cuda.synchronize()


@pytest.mark.parametrize('raster', [False, True])
def test_voxelize_raw_cap_rows(dev, raster):
    """cap_rows (6) below the voxel count (14): row_end == cap_rows, rows 0..5 are the first six of the row order asked for, and the
    rows from cap_rows on (the back guard of both slabs) keep the canary."""
    from oracle import lidar_ref
    lo, vs, grid, pts, n_vox = _capped_cloud()
    f_ref, c_ref = lidar_ref.voxelize_ref([pts], lo, vs, grid, 3, 1000)
    if raster:
        order = np.argsort(_key(c_ref, grid), kind='stable')
        f_ref, c_ref = f_ref[order], c_ref[order]
    cap, ldf = 6, 16
    d = _dev_pts([pts], dev)[0]
    got = []
    for word in lds_state.WORDS:                       # three runs, each after another content of LDS (tests/lds_state.py)
        fs = Slab(dev, cap, ldf, back=n_vox).fill_canary()
        cs = Slab(dev, cap, 4, back=n_vox, dtype=torch.int32).fill_canary()
        end = torch.full((3,), I32_CANARY, device=dev, dtype=torch.int32)
        with lds_state.poisoned(word):
            _vox_raw(dev, d, lo, vs, grid, 3, 1000, 0, None, cap, fs, ldf, cs, end[1:2], raster)
        fs.check_canary('voxelize cap_rows feats')
        cs.check_canary('voxelize cap_rows coords')
        assert end.tolist() == [I32_CANARY, cap, I32_CANARY]
        got.append((fs.view.cpu().numpy(), cs.view.cpu().numpy()))
    for other in got[1:]:
        assert np.array_equal(_bits(got[0][0]), _bits(other[0])) and np.array_equal(got[0][1], other[1])
    assert np.array_equal(got[0][1], c_ref[:cap])
    _same_f32(got[0][0][:, :4], f_ref[:cap], 'voxelize cap_rows means')
    assert not _bits(got[0][0][:, 4:]).any()


@pytest.mark.parametrize('ldf', [4, 5, 16])
@pytest.mark.parametrize('raster', [False, True])
def test_voxelize_raw_ldf(dev, ldf, raster):
    """Row stride 4 (nothing but the means), 5 and 16: columns 4.. are zero and nothing is written behind the last row."""
    from oracle import lidar_ref
    lo, vs, grid, pts, n_vox = _capped_cloud()
    f_ref, c_ref = lidar_ref.voxelize_ref([pts], lo, vs, grid, 10, 1000)
    if raster:
        order = np.argsort(_key(c_ref, grid), kind='stable')
        f_ref, c_ref = f_ref[order], c_ref[order]
    d = _dev_pts([pts], dev)[0]
    fs = Slab(dev, n_vox, ldf, front=2, back=4).fill_canary()
    cs = Slab(dev, n_vox, 4, front=2, back=4, dtype=torch.int32).fill_canary()
    end = torch.full((1,), I32_CANARY, device=dev, dtype=torch.int32)
    _vox_raw(dev, d, lo, vs, grid, 10, 1000, 0, None, n_vox, fs, ldf, cs, end, raster)
    fs.check_canary(f'voxelize ldf {ldf} feats')
    cs.check_canary(f'voxelize ldf {ldf} coords')
    assert end.tolist() == [n_vox]
    f = fs.view.cpu().numpy()
    assert np.array_equal(cs.view.cpu().numpy(), c_ref)
    _same_f32(f[:, :4], f_ref, f'voxelize ldf {ldf} means')
    assert not _bits(f[:, 4:]).any()


@pytest.mark.parametrize('raster', [False, True])
def test_voxelize_raw_chain(dev, raster):
    """Four samples chained through device row counters: row_base = NULL for the first, a sample with n = 0 and points = NULL, a sample
    entirely outside, a last sample.  The row_end chain and the batch_idx column are exact; rows beyond the last keep the canary."""
    from oracle import lidar_ref
    lo, vs, grid, pts, n_vox = _capped_cloud()
    rng = np.random.RandomState(8)
    last = pts[rng.permutation(len(pts))[:40]]
    out = np.array([[100., 0., 0., 1.], [0., -50., 0., 1.], [0., 0., 9., 1.]], np.float32)
    samples = [pts, None, out, last]
    f_ref, c_ref = lidar_ref.voxelize_ref([pts, np.zeros((0, 4), np.float32), out, last], lo, vs, grid, 4, 9)
    n0, n3 = int((c_ref[:, 0] == 0).sum()), int((c_ref[:, 0] == 3).sum())
    assert n0 == 9 and 0 < n3 <= 9 and set(c_ref[:, 0].tolist()) == {0, 3}
    if raster:
        order = np.lexsort((c_ref[:, 3], c_ref[:, 2], c_ref[:, 1], c_ref[:, 0]))
        f_ref, c_ref = f_ref[order], c_ref[order]
    V = n0 + n3
    fs = Slab(dev, V, 4, ld=5, back=3).fill_canary()
    cs = Slab(dev, V, 4, back=3, dtype=torch.int32).fill_canary()
    ends = torch.full((6,), I32_CANARY, device=dev, dtype=torch.int32)
    for b, p in enumerate(samples):
        d = None if p is None else _dev_pts([p], dev)[0]
        _vox_raw(dev, d, lo, vs, grid, 4, 9, b, None if b == 0 else ends[b:b + 1], V + 3, fs, 5, cs, ends[b + 1:b + 2], raster)
    assert ends.tolist() == [I32_CANARY, n0, n0, n0, V, I32_CANARY]
    cs.check_canary('voxelize chain coords')
    c = cs.view.cpu().numpy()
    assert np.array_equal(c, c_ref) and c[:n0, 0].tolist() == [0] * n0 and c[n0:, 0].tolist() == [3] * n3
    fb = fs.bits().reshape(-1, 5).numpy()
    assert (fb[V:] == F32_CANARY).all(), 'feats rows behind the last sample were written'
    _same_f32(fs.flat.cpu().numpy().reshape(-1, 5)[:V, :4], f_ref, 'voxelize chain means')
    assert not fb[:V, 4].any()                                            # ldf = 5: column 4 is the kernel's to zero


# ================================================================================================ lm_sparse_grid_build
def test_sparse_grid_build(dev):
    from lanemapping_amd import ops
    B, shape = 3, (3, 7, 5)
    D, H, W = shape
    rng = np.random.RandomState(17)
    mask = rng.rand(B, D, H, W) < 0.2
    mask[0, 0, 0, 0] = mask[B - 1, D - 1, H - 1, W - 1] = True
    coords = np.argwhere(mask).astype(np.int32)
    coords = coords[rng.permutation(len(coords))]
    cd = torch.from_numpy(coords).to(dev)
    want = R.grid_ref(coords, B, shape)
    for n in (len(coords), len(coords), 0):
        gs = Slab(dev, B * D * H, W, front=3, back=3, dtype=torch.int32).fill_canary()
        _chk(_lib().lm_sparse_grid_build(_s(), cd.data_ptr() if n else None, n, gs.ptr(), B, D, H, W))
        torch.cuda.synchronize()
        gs.check_canary(f'sparse_grid_build n {n}')
        got = gs.view.cpu().numpy().reshape(B, D, H, W)
        assert np.array_equal(got, want if n else np.full_like(want, -1))
    assert np.array_equal(ops.sparse_grid(cd, B, shape).cpu().numpy(), want)


# ================================================================================================ lm_sparse_conv_outputs / lm_sparse_rulebook
@functools.lru_cache(maxsize=None)
def _case(gi, vi, aset):
    """(B, in_coords, out_shape, out_coords, out_grid, rulebook) of one geometry x volume x active set, computed once."""
    kernel, stride, padding = (R.GEOMETRIES + [R.SUBM])[gi]
    shape = R.VOLUMES[vi]
    B, inc = R.active_sets(shape)[aset]
    out_shape, oc, og = R.conv_outputs_ref(inc, B, shape, kernel, stride, padding)
    nbr = R.rulebook_ref(oc, inc, shape, kernel, stride, padding)
    return B, inc, out_shape, oc, og, nbr


def _rulebook_raw(dev, out_coords_d, in_grid_d, geom, name):
    """lm_sparse_rulebook into a canary slab, once after each LDS word -> [n_out, taps] int32 on the device."""
    kernel, stride, padding = geom
    from lanemapping_amd import ops
    B, D, H, W = in_grid_d.shape
    taps = kernel[0] * kernel[1] * kernel[2]
    n_out = out_coords_d.shape[0]
    got = []
    for word in lds_state.WORDS:                       # three runs, each after another content of LDS (tests/lds_state.py)
        ns = Slab(dev, n_out, taps, front=2, back=2, dtype=torch.int32).fill_canary()
        with lds_state.poisoned(word):
            _chk(_lib().lm_sparse_rulebook(_s(), out_coords_d.data_ptr(), n_out, in_grid_d.data_ptr(), B, D, H, W,
                                           ops._ksp(kernel, stride, padding), ns.ptr()))
        torch.cuda.synchronize()
        ns.check_canary(name)
        got.append(ns.view.clone())                                       # its own allocation: conv_gather reads it
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2]), f'{name}: a later run differs from the first'
    return got[0]


def _chain(dev, geom, B, shape, inc, in_d, oc, nbr_d, cin, cout, name):
    """Random features on the active rows -> ops.conv_gather over the DEVICE rulebook vs float64 conv3d of the zero-filled volume read
    at the device's output sites, at the 1e-5 of test_conv_gather_vs_fp64."""
    from lanemapping_amd import ops
    kernel, stride, padding = geom
    g = torch.Generator().manual_seed(cin * 31 + cout + len(inc))
    taps = kernel[0] * kernel[1] * kernel[2]
    x = torch.zeros(len(inc), ops.sparse_ld(cin))
    x[:, :cin] = torch.randn(len(inc), cin, generator=g)
    w = torch.randn(*kernel, cin, cout, generator=g) / (taps * cin) ** 0.5
    ref = R.conv3d_rows_ref(x[:, :cin], inc, B, shape, w, kernel, stride, padding, oc)
    xd, wp = x.to(dev), ops.pack_sparse(w.to(dev))
    y = ops.conv_gather(xd, nbr_d, wp, cin, cout)
    assert y.shape == (len(oc), ops.sparse_ld(cout))
    _close(y[:, :cout], ref, 1e-5, f'{name} chain {cin}->{cout}')
    assert torch.equal(y, ops.conv_gather(xd, nbr_d, wp, cin, cout))


def _channel_pairs(geom):
    return [(16, 16), (32, 64)] + ([(128, 128)] if geom[0] == (3, 1, 1) else [])       # 128 -> 128 over 3 taps: conv_out of the network


GEOM_IDS = [R.geom_id(g) for g in R.GEOMETRIES]


@pytest.mark.parametrize('aset', R.SETS)
@pytest.mark.parametrize('vi', range(len(R.VOLUMES)), ids=['5x6x7', '4x9x8'])
@pytest.mark.parametrize('gi', range(len(R.GEOMETRIES)), ids=GEOM_IDS)
def test_conv_outputs_and_rulebook(dev, gi, vi, aset):
    """ops.sparse_conv_outputs + raw lm_sparse_rulebook against the brute-force references: output shape, site list and its order, row
    grid, count, every rulebook word; then the chain check through conv_gather.  On the hand-placed set (corners, row / plane / sample
    seams, an empty sample) the defining property is also stated directly on the device rulebook."""
    from lanemapping_amd import ops
    geom = R.GEOMETRIES[gi]
    kernel, stride, padding = geom
    shape = R.VOLUMES[vi]
    B, inc, out_shape, oc_ref, og_ref, nbr_ref = _case(gi, vi, aset)
    name = f'{R.geom_id(geom)} {shape} {aset}'
    in_d = torch.from_numpy(inc).to(dev)
    in_grid = ops.sparse_grid(in_d, B, shape)
    assert np.array_equal(in_grid.cpu().numpy(), R.grid_ref(inc, B, shape))
    og, oc, oshape = ops.sparse_conv_outputs(in_d, B, shape, kernel, stride, padding)        # 'full': also the wrapper's row bound
    og2, oc2, _ = ops.sparse_conv_outputs(in_d, B, shape, kernel, stride, padding)
    assert torch.equal(og, og2) and torch.equal(oc, oc2), f'{name}: the second run differs from the first'
    assert tuple(oshape) == out_shape and tuple(og.shape) == (B,) + out_shape
    ocn = oc.cpu().numpy()
    assert ocn.shape == oc_ref.shape, f'{name}: {ocn.shape[0]} output sites, want {oc_ref.shape[0]}'
    assert np.array_equal(ocn, oc_ref), f'{name}: output sites or their order differ'
    assert np.array_equal(og.cpu().numpy(), og_ref), f'{name}: output row grid differs'
    if len(oc_ref) == 0:
        return                                                            # the asymmetric geometry reaches no cell of the placed set in (5, 6, 7)
    nbr = _rulebook_raw(dev, oc, in_grid, geom, name + ' rulebook')
    nn = nbr.cpu().numpy()
    bad = nn != nbr_ref
    assert not bad.any(), f'{name}: {int(bad.sum())} of {bad.size} rulebook words differ; first at (row, tap) {np.argwhere(bad)[0].tolist()}'
    if aset == 'placed':
        taps = [(kz, ky, kx) for kz in range(kernel[0]) for ky in range(kernel[1]) for kx in range(kernel[2])]
        assert not (ocn[:, 0] == 1).any()                                 # the empty sample has no output
        for m, t in np.argwhere(nn >= 0):
            src, o = inc[nn[m, t]], ocn[m]
            assert src[0] == o[0], f'{name}: output row {m} of sample {o[0]} reads input row {nn[m, t]} of sample {src[0]}'
            want = [o[1 + a] * stride[a] - padding[a] + taps[t][a] for a in range(3)]
            assert src[1:].tolist() == want, f'{name}: output {o.tolist()} tap {taps[t]} reads {src.tolist()}, not {want}'
    for cin, cout in _channel_pairs(geom):
        _chain(dev, geom, B, shape, inc, in_d, ocn, nbr, cin, cout, name)


@pytest.mark.parametrize('aset', R.SETS)
@pytest.mark.parametrize('vi', range(len(R.VOLUMES)), ids=['5x6x7', '4x9x8'])
def test_submanifold_rulebook(dev, vi, aset):
    """SubMConv3d: out == in (the input's own, shuffled, row order), (3,3,3) / 1 / 1."""
    from lanemapping_amd import ops
    shape = R.VOLUMES[vi]
    B, inc = R.active_sets(shape)[aset]
    kernel, stride, padding = R.SUBM
    name = f'subm {shape} {aset}'
    in_d = torch.from_numpy(inc).to(dev)
    in_grid = ops.sparse_grid(in_d, B, shape)
    nbr = _rulebook_raw(dev, in_d, in_grid, R.SUBM, name)
    want = R.rulebook_ref(inc, inc, shape, kernel, stride, padding)
    assert np.array_equal(nbr.cpu().numpy(), want), f'{name}: rulebook differs'
    assert np.array_equal(nbr.cpu().numpy()[:, 13], np.arange(len(inc)))  # the centre tap is the row itself
    assert torch.equal(ops.sparse_rulebook(in_d, in_grid, kernel, stride, padding), nbr)
    for cin, cout in [(16, 16), (32, 64)]:
        _chain(dev, R.SUBM, B, shape, inc, in_d, inc, nbr, cin, cout, name)


@pytest.mark.parametrize('gi,aset', [(0, 'random'), (5, 'full'), (9, 'random')])
def test_conv_outputs_raw_cap_rows(dev, gi, aset):
    """Raw lm_sparse_conv_outputs with cap_rows below the number of active sites: *out_count is still the full count, the coordinate
    rows from cap_rows on keep the canary, the grid cells of the dropped sites are -1, the back guards are intact."""
    from lanemapping_amd import ops
    geom = R.GEOMETRIES[gi]
    shape = R.VOLUMES[1]
    B, inc, out_shape, oc_ref, og_ref, _ = _case(gi, 1, aset)
    Do, Ho, Wo = out_shape
    cells = B * Do * Ho * Wo
    cap = len(oc_ref) // 2
    assert cap >= 3
    in_d = torch.from_numpy(inc).to(dev)
    need = _lib().lm_sparse_conv_outputs_workspace_bytes(cells)
    got = []
    for word in lds_state.WORDS:                       # three runs, each after another content of LDS (tests/lds_state.py)
        ws = torch.empty((need,), device=dev, dtype=torch.uint8)
        gs = Slab(dev, B * Do * Ho, Wo, front=2, back=2, dtype=torch.int32).fill_canary()
        cs = Slab(dev, cap, 4, front=2, back=len(oc_ref) - cap + 2, dtype=torch.int32).fill_canary()
        cnt = torch.full((3,), I32_CANARY, device=dev, dtype=torch.int32)
        with lds_state.poisoned(word):
            _chk(_lib().lm_sparse_conv_outputs(_s(), in_d.data_ptr(), len(inc), B, ops._ksp(*geom), Do, Ho, Wo, gs.ptr(), cs.ptr(), cap,
                                               cnt[1:2].data_ptr(), ws.data_ptr(), need))
        torch.cuda.synchronize()
        gs.check_canary('conv_outputs cap_rows grid')
        cs.check_canary('conv_outputs cap_rows coords')
        assert cnt.tolist() == [I32_CANARY, len(oc_ref), I32_CANARY]
        got.append((gs.view.cpu().numpy().reshape(B, Do, Ho, Wo), cs.view.cpu().numpy()))
    for other in got[1:]:
        assert np.array_equal(got[0][0], other[0]) and np.array_equal(got[0][1], other[1])
    assert np.array_equal(got[0][1], oc_ref[:cap])
    assert np.array_equal(got[0][0], np.where(og_ref < cap, og_ref, -1))
