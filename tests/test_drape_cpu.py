"""CPU: las_io.ElevationDrape, the cfg['las_elevation'] / elevation= plumbing of the Runner, the back-projection with vertex heights
(lm_polyline_backproject_z through coor_img2pc and directly) on the inputs of golden g12, and the numpy restatement of the drape
(tests/drape_ref.py) on hand-made cases whose answers are written out."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import cases
import drape_ref as dr
import ground_ref as gr
from lanemapping_amd import coor_img2pc, ops
from lanemapping_amd._lib import lib
from lanemapping_amd.las_io import ElevationDrape
from lanemapping_amd.runner import Runner

f32 = np.float32
NaN = float('nan')


# ------------------------------------------------------------------------------------------------ ElevationDrape
def test_elevation_drape_validation():
    e = ElevationDrape()
    assert (e.radius_px, e.min_pixels, e.fit) == (4, 5, 'line')
    assert ElevationDrape(0, 1, 'none') == ElevationDrape(radius_px=0, min_pixels=1, fit='none') and ElevationDrape(8).radius_px == 8
    for bad in (-1, 9, 2.5, True, 'four'):
        with pytest.raises((ValueError, TypeError), match='radius_px|invalid literal'):
            ElevationDrape(radius_px=bad)
    for bad in (0, -3, 1.5, False):
        with pytest.raises(ValueError, match='min_pixels'):
            ElevationDrape(min_pixels=bad)
    for bad in ('cubic', None, 1, 'LINE'):
        with pytest.raises(ValueError, match='fit'):
            ElevationDrape(fit=bad)
    with pytest.raises(AttributeError):
        e.fit = 'none'
    assert 'not a tuned value' in ElevationDrape.__doc__


class _Cfg(dict):
    list_img_size_xy = [1152, 1152]


def _runner(**cfg):
    r = Runner.__new__(Runner)
    r.cfg, r.device, r.net = _Cfg(cfg), torch.device('cpu'), None
    return r


def test_las_elevation_argument_and_cfg_default():
    assert _runner()._las_elevation(None) is None, "absent: today's behaviour"
    assert _runner(las_elevation={'radius_px': 2, 'fit': 'none'})._las_elevation(None) == ElevationDrape(2, 5, 'none')
    mine = ElevationDrape(min_pixels=9)
    assert _runner(las_elevation={'radius_px': 2})._las_elevation(mine) is mine, 'the argument wins over the config'
    with pytest.raises(TypeError, match='ElevationDrape'):
        _runner()._las_elevation({'radius_px': 2})
    with pytest.raises(ValueError, match='radius_px'):
        _runner(las_elevation={'radius_px': 9})._las_elevation(None)
    for fn in (Runner.infer_las_strip_to_map, Runner.infer_las_to_map):
        assert inspect.signature(fn).parameters['elevation'].default is None
    assert inspect.signature(Runner._las_chain).parameters['elevation'].default is None


# ------------------------------------------------------------------------------------------------ back-projection with vertex heights
def _backproject(entry, params, seqs, lens, tile, *more):
    """The C entry itself on the caller's tile (coor_img2pc works on a copy): -> out [L, V, 3]; `tile` is mutated in place."""
    seqs = np.ascontiguousarray(seqs, dtype=np.float64)
    L, V, _ = seqs.shape
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    p13 = np.array(list(params['img_reso'][:2]) + list(params['bev_img_offset'][:2]) + [params['ele_reso'], params['local_min_ele']] +
                   list(params['las_rotation_trans_quan'][:7]), dtype=np.float64)
    off = np.array(params['las_read_offset'][:3], dtype=np.float64)
    out = np.zeros((L, V, 3))
    vp = C.c_void_p
    assert tile.flags.c_contiguous and tile.dtype == np.uint8
    rc = getattr(lib(), entry)(vp(tile.ctypes.data), tile.shape[0], tile.shape[1], tile.shape[2], vp(seqs.ctypes.data), vp(lens.ctypes.data),
                               L, V, vp(p13.ctypes.data), vp(off.ctypes.data), vp(out.ctypes.data), *more)
    assert rc == 0, lib().lm_last_error()
    return out


def _backproject_z(params, seqs, lens, tile, vz, fit):
    vz = np.ascontiguousarray(vz, dtype=f32)
    return _backproject('lm_polyline_backproject_z', params, seqs, lens, tile, C.c_void_p(vz.ctypes.data), fit)


def _fill_ref(tile, ph, pw):
    """Step 1 for one vertex pixel, restated: the mean G of the smallest non-empty half-open window [p - step, p + step)."""
    H, W, _ = tile.shape
    if (ph == 0 and pw == 0) or int(tile[ph, pw].astype(np.int64).sum()) > 1:
        return
    for step in range(1, H + W):
        win = tile[max(ph - step, 0):min(ph + step, H), max(pw - step, 0):min(pw + step, W)].astype(np.int64)
        if win.sum() > 0:
            tile[ph, pw, 1] = int(float(win[..., 1].sum()) / float((win.sum(axis=2) > 0).sum()))
            return


def _g_rule(params, tile, seqs):
    r, c = seqs[..., 0].astype(np.int64), seqs[..., 1].astype(np.int64)
    return tile[r, c, 1].astype(np.float64) * float(params['ele_reso']) + float(params['local_min_ele'])


def _real(seqs, lens):
    m = np.zeros(seqs.shape[:2], bool)
    for l, n in enumerate(lens):
        m[l, :n] = True
    return m


def test_all_nan_heights_with_line_fit_are_the_plain_call(golden):
    g = golden('g12_img2pc.npz')
    for i, seed in enumerate(g['seeds']):
        params, seqs, lens, tile = cases.img2pc_case(int(seed))
        nan = np.full(seqs.shape[:2], np.nan, dtype=f32)
        out = coor_img2pc.transform_coordinate_from_img_2_pc(params, seqs.copy(), lens, tile, vertex_z=nan, fit='line')
        assert np.array_equal(out.view(np.uint64), g[f'out_{i}'].view(np.uint64)), 'vertex_z all NaN, fit=line: the golden output in every bit'
        t_old, t_new = tile.copy(), tile.copy()
        o_old = _backproject('lm_polyline_backproject', params, seqs, lens, t_old)
        o_new = _backproject_z(params, seqs, lens, t_new, nan, 1)
        assert np.array_equal(o_old.view(np.uint64), o_new.view(np.uint64)) and np.array_equal(t_old, t_new) and not np.array_equal(t_old, tile)


def test_defaults_take_the_old_entry(golden, monkeypatch):
    g = golden('g12_img2pc.npz')
    params, seqs, lens, tile = cases.img2pc_case(int(g['seeds'][0]))
    calls = []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(lib(), name)

    monkeypatch.setattr(coor_img2pc, 'lib', lambda: Spy())
    out = coor_img2pc.transform_coordinate_from_img_2_pc(params, seqs.copy(), lens, tile)
    assert calls == ['lm_polyline_backproject'] and np.array_equal(out, g['out_0'])
    out = coor_img2pc.transform_coordinate_from_img_2_pc(params, seqs.copy(), lens, tile, vertex_z=None, fit='line')
    assert calls == ['lm_polyline_backproject'] * 2 and np.array_equal(out, g['out_0'])
    coor_img2pc.transform_coordinate_from_img_2_pc(params, seqs.copy(), lens, tile, fit='none')
    assert calls[2:] == ['lm_polyline_backproject_z']
    with pytest.raises(ValueError, match='fit'):
        coor_img2pc.transform_coordinate_from_img_2_pc(params, seqs, lens, tile, fit='spline')
    with pytest.raises(ValueError, match='vertex_z'):
        coor_img2pc.transform_coordinate_from_img_2_pc(params, seqs, lens, tile, vertex_z=np.zeros((2, 2), f32))
    with pytest.raises(AssertionError, match='fit=2'):             # the entry refuses a fit that is neither 0 nor 1
        _backproject_z(params, seqs, lens, tile.copy(), np.zeros(seqs.shape[:2], f32), 2)


def test_finite_heights_without_fit_equal_the_float64_restatement(golden):
    g = golden('g12_img2pc.npz')
    for i, seed in enumerate(g['seeds']):
        params, seqs, lens, tile = cases.img2pc_case(int(seed))
        rng = np.random.RandomState(int(seed))
        vz = rng.uniform(-3.0, 4.0, seqs.shape[:2]).astype(f32)
        real = _real(seqs, lens)
        mine = tile.copy()
        out = _backproject_z(params, seqs, lens, mine, vz, 0)
        assert np.array_equal(mine, tile), 'every vertex has a height: the tile is not touched'
        want = dr.backproject_z(params, seqs, np.where(real, vz.astype(np.float64), _g_rule(params, tile, seqs)))
        assert np.array_equal(out.view(np.uint64), want.view(np.uint64)), 'steps 2 and 4 in float64, bit for bit (padding: the G rule)'
        via = coor_img2pc.transform_coordinate_from_img_2_pc(params, seqs.copy(), lens, tile, vertex_z=vz, fit='none')
        assert np.array_equal(via.view(np.uint64), out.view(np.uint64))
        # the heights are really used, and the line fit is really off: z is not linear in the vertex index
        l = int(np.argmax(lens))
        assert np.abs(np.diff(out[l, :lens[l], 2], 2)).max() > 0.1
        fitted = _backproject_z(params, seqs, lens, tile.copy(), vz, 1)
        assert not np.array_equal(fitted, out) and np.array_equal(fitted[..., :1].shape, out[..., :1].shape)


def test_mixed_heights_fill_only_the_vertices_without_one(golden):
    g = golden('g12_img2pc.npz')
    filled_some = False
    for i, seed in enumerate(g['seeds']):
        params, seqs, lens, tile = cases.img2pc_case(int(seed))
        real = _real(seqs, lens)
        r, c = seqs[..., 0].astype(np.int64), seqs[..., 1].astype(np.int64)
        empty = real & (tile[r, c].astype(np.int64).sum(axis=2) <= 1) & ~((r == 0) & (c == 0))
        assert empty.sum() >= 4, 'the case has vertices on empty pixels'
        vz = np.full(seqs.shape[:2], np.nan, dtype=f32)
        order = np.argwhere(empty)
        given = order[::2]                                          # every other empty vertex gets a height, and every third other one
        vz[given[:, 0], given[:, 1]] = 1.25
        vz[:, ::3] = np.where(np.isnan(vz[:, ::3]), f32(-0.5), vz[:, ::3])
        vz[0, 1] = np.inf                                           # not finite: no height either
        want_tile = tile.copy()
        for l in range(len(lens)):
            for v in range(lens[l]):
                if not np.isfinite(vz[l, v]):
                    _fill_ref(want_tile, int(seqs[l, v, 0]), int(seqs[l, v, 1]))
        mine = tile.copy()
        out = _backproject_z(params, seqs, lens, mine, vz, 0)
        assert np.array_equal(mine, want_tile), 'the fill ran for exactly the vertices without a height, in order'
        has = real & np.isfinite(vz)
        assert np.array_equal(mine[r[has & empty], c[has & empty]], tile[r[has & empty], c[has & empty]])
        filled_some |= bool((mine != tile).any())
        want = dr.backproject_z(params, seqs, np.where(has, vz.astype(np.float64), _g_rule(params, want_tile, seqs)))
        assert np.array_equal(out.view(np.uint64), want.view(np.uint64))
    assert filled_some


# ------------------------------------------------------------------------------------------------ drape_ref by inspection
def test_median_takes_the_lower_element_and_nan_for_none():
    slots = gr.values_to_keys(np.array([[3.0, NaN, 1.0, 2.0, NaN, 4.0, NaN, NaN, NaN],      # k = 4: 1 2 3 4 -> element 1 = 2
                                        [NaN] * 9,                                          # k = 0
                                        [5.0] + [NaN] * 8,                                  # k = 1
                                        [0.0, -0.0, NaN, NaN, NaN, NaN, NaN, NaN, NaN],     # k = 2: -0.0 < +0.0 -> -0.0
                                        [9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0],      # k = 9: element 4 = 5
                                        [-1.0, -2.0, 7.0, 7.0, -2.0, NaN, NaN, NaN, NaN]],  # k = 5: -2 -2 -1 7 7 -> element 2 = -1
                                       dtype=f32))
    z, npix = dr.median(slots.reshape(6, 3, 3))
    assert npix.tolist() == [4, 0, 1, 2, 9, 5]
    assert z.dtype == np.float32 and np.isnan(z[1])
    assert [float(v) for v in z[[0, 2, 4, 5]]] == [2.0, 5.0, 5.0, -1.0]
    assert z[3] == 0.0 and np.signbit(z[3])


def test_window_is_clipped_at_the_tile_corner():
    H, W, R = 6, 5, 1
    pix = gr.values_to_keys(np.arange(H * W, dtype=f32).reshape(H, W))
    win = gr.keys_to_values(dr.window_keys(pix, [(0, 0), (H - 1, W - 1), (2, 2)], R))
    assert np.array_equal(np.isnan(win[0]), [[True, True, True], [True, False, False], [True, False, False]])
    assert win[0][1:, 1:].tolist() == [[0.0, 1.0], [5.0, 6.0]]
    assert win[1][:2, :2].tolist() == [[23.0, 24.0], [28.0, 29.0]] and np.isnan(win[1][2]).all() and np.isnan(win[1][:, 2]).all()
    assert win[2].tolist() == [[6.0, 7.0, 8.0], [11.0, 12.0, 13.0], [16.0, 17.0, 18.0]]
    z, npix = dr.median(dr.window_keys(pix, [(0, 0), (H - 1, W - 1), (2, 2)], R))
    assert npix.tolist() == [4, 4, 9] and z.tolist() == [1.0, 24.0, 12.0]        # 0 1 5 6 -> 1;  23 24 28 29 -> 24


def test_drape_ref_from_points():
    """An identity tile of 8 x 8 pixels of 1 m: a point (x, y, z) lands in pixel (round x, round y) with vz = z."""
    p = ops.make_raster_params(img_reso=(1.0, 1.0))
    pts = np.array([[2.0, 3.0, 5.0, 1.0], [2.2, 2.9, 4.0, 1.0],      # pixel (2, 3): min 4
                    [3.0, 3.0, 1.0, 1.0],                             # pixel (3, 3)
                    [1.0, 2.0, NaN, 1.0], [1.0, 2.0, np.inf, 1.0],    # not finite: nowhere
                    [NaN, 2.0, 0.0, 1.0],
                    [9.0, 3.0, -7.0, 1.0],                            # outside the window
                    [7.0, 7.0, 2.0, 1.0]], dtype=f32)
    verts = [(2, 3), (2, 3), (0, 0), (7, 7), (3, 4)]
    z, npix, pmin = dr.drape_vertices(pts, [0, len(pts)], [p], verts, [0, len(verts)], 8, 8, 1)
    assert npix.tolist() == [2, 2, 0, 1, 2]
    assert z[[0, 1, 3, 4]].tolist() == [1.0, 1.0, 2.0, 1.0] and np.isnan(z[2])
    assert pmin.shape == (5, 3, 3) and pmin[0, 1, 1] == 4.0 and pmin[0, 2, 1] == 1.0 and np.isnan(pmin[0]).sum() == 7
    assert pmin[4, 0, 0] == 4.0 and pmin[4, 1, 0] == 1.0 and pmin[3, 1, 1] == 2.0
    z0, n0, _ = dr.drape_vertices(pts, [0, len(pts)], [p], verts, [0, len(verts)], 8, 8, 0)
    assert n0.tolist() == [1, 1, 0, 1, 0] and z0[[0, 1, 3]].tolist() == [4.0, 4.0, 2.0]
    # two tiles, the second without vertices, the first without points
    z2, n2, _ = dr.drape_vertices(pts, [0, 0, len(pts)], [p, p], verts, [0, len(verts), len(verts)], 8, 8, 1)
    assert n2.tolist() == [0] * 5 and np.isnan(z2).all()


# ------------------------------------------------------------------------------------------------ the crest of the GPU accuracy test
def test_plain_backprojection_breaks_the_drape_bound_on_the_crest():
    """The scene of tests/test_gpu_drape.py::test_crest_accuracy is sized so that today's heights (8-bit elevation of the vertex pixel,
    then a least-squares line over the vertex index) miss the bound the draped heights have to keep; the restated drape keeps it."""
    from oracle import raster_ref
    params, kw, pts, seqs, lens, g = dr.crest_case()
    S = dr.CREST_S
    tile = raster_ref.raster(pts, raster_ref.params(quat=(1, 0, 0, 0), **kw), S, S)
    assert (tile.sum(axis=2) > 0).all(), 'one point in every pixel'
    bound = dr.crest_bound(g)
    plain = coor_img2pc.transform_coordinate_from_img_2_pc(params, seqs, lens, tile)
    err = dr.crest_error(params, plain, lens)
    assert (err > bound).any(), f'the plain call keeps the bound {bound:.3f} m everywhere (worst {err.max():.3f} m): the crest is too flat'
    verts = [(int(seqs[l, v, 0]), int(seqs[l, v, 1])) for l in range(3) for v in range(lens[l])]
    z, npix, _ = dr.drape_vertices(pts, [0, len(pts)], [ops.make_raster_params(**kw)], verts, [0, len(verts)], S, S, dr.CREST_R)
    vz = np.full(seqs.shape[:2], np.nan, f32)
    vz[_real(seqs, lens)] = z
    draped = coor_img2pc.transform_coordinate_from_img_2_pc(params, seqs, lens, tile, vertex_z=vz, fit='none')
    assert (dr.crest_error(params, draped, lens) <= bound).all() and npix.min() >= 25
