"""CPU: the numpy restatement of the ground model (tests/ground_ref.py) against hand-built grids, las_io.GroundFilter / ground_datum, and
the cfg['las_ground'] / ground= plumbing of the Runner with the device calls stubbed."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

import ground_ref as gr
from lanemapping_amd import io_utils, las_io, ops
from lanemapping_amd.las_io import GroundFilter, ground_datum
from lanemapping_amd.runner import Runner

f32 = np.float32
NaN = float('nan')


def _ground(values):
    g, gmin = gr.smooth(gr.values_to_keys(np.asarray(values, dtype=f32))[None])
    return g[0], gmin[0]


# ------------------------------------------------------------------------------------------------ the reference on hand-built grids
def test_keys_are_ordered_like_the_values_and_round_trip():
    v = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.25, np.inf], dtype=f32)
    k = gr.key_of(v)
    assert (np.diff(k.astype(np.int64)) > 0).all(), 'ascending values give strictly ascending keys, -0.0 below +0.0'
    assert np.array_equal(gr.value_of(k).view(np.uint32), v.view(np.uint32))
    finite = np.array([np.finfo(f32).max, -np.finfo(f32).max], dtype=f32)
    assert (gr.key_of(finite) != gr.EMPTY).all(), 'no finite value collides with EMPTY'


def test_full_3x3_corner_edge_interior_ranks():
    g, gmin = _ground([[5, 1, 7],
                       [3, 9, 2],
                       [8, 4, 6]])
    assert g[0, 0] == 3      # corner: {1, 3, 5, 9} -> rank 1
    assert g[0, 2] == 2      # corner: {1, 2, 7, 9} -> rank 1
    assert g[2, 0] == 4      # corner: {3, 4, 8, 9}
    assert g[2, 2] == 4      # corner: {2, 4, 6, 9}
    assert g[0, 1] == 3      # edge: {1, 2, 3, 5, 7, 9} -> rank 2
    assert g[1, 0] == 4      # edge: {1, 3, 4, 5, 8, 9}
    assert g[1, 2] == 4      # edge: {1, 2, 4, 6, 7, 9}
    assert g[2, 1] == 4      # edge: {2, 3, 4, 6, 8, 9}
    assert g[1, 1] == 5      # interior: 1..9 -> rank 4
    assert gmin == 2


def test_interior_with_1_2_8_9_filled_neighbours():
    v = np.full((4, 4), NaN, dtype=f32)
    v[3, 3] = 7.0                                                  # k = 1 for the interior cell (2, 2)
    g, gmin = _ground(v)
    assert g[2, 2] == 7 and g[3, 3] == 7 and g[2, 3] == 7 and g[3, 2] == 7
    assert np.isnan(g[0:2, :]).all() and np.isnan(g[:, 0:2]).all(), 'a neighbourhood of empty cells gives NaN'
    assert gmin == 7
    v[1, 1] = -2.0                                                 # k = 2 for (2, 2): {-2, 7} -> rank 0, the lower one
    g, gmin = _ground(v)
    assert g[2, 2] == -2 and g[3, 3] == 7 and g[1, 1] == -2 and gmin == -2
    full = np.arange(16, dtype=f32).reshape(4, 4)
    g9, _ = _ground(full)
    assert g9[1, 1] == 5 and g9[2, 2] == 10 and g9[1, 2] == 6     # k = 9: the centre of 0,1,2,4,5,6,8,9,10 etc.
    full8 = full.copy()
    full8[0, 0] = NaN                                              # k = 8 for (1, 1): {1,2,4,5,6,8,9,10} -> rank 3 = 5
    g8, _ = _ground(full8)
    assert g8[1, 1] == 5
    full8[0, 0], full8[2, 2] = 0.0, NaN                            # k = 8: {0,1,2,4,5,6,8,9} -> rank 3 = 4: one below the k = 9 answer
    g8, _ = _ground(full8)
    assert g8[1, 1] == 4


def test_outlier_cell_vanishes_and_a_filled_cell_is_finite():
    v = np.full((4, 4), 1.0, dtype=f32)
    v[1, 2] = -50.0                                                # a noise return below ground
    g, gmin = _ground(v)
    assert (g == 1.0).all() and gmin == 1.0
    v[1, 2] = 4.0                                                  # a lorry roof
    g, _ = _ground(v)
    assert (g == 1.0).all()
    lone = np.full((3, 3), NaN, dtype=f32)
    lone[0, 0] = 3.0
    g, _ = _ground(lone)
    assert g[0, 0] == 3.0 and np.isfinite(g[0:2, 0:2]).all() and np.isnan(g[2, :]).all()


def test_all_empty_grid_and_signed_zero():
    g, gmin = _ground(np.full((3, 3), NaN, dtype=f32))
    assert np.isnan(g).all() and gmin == np.inf
    z = np.full((3, 3), NaN, dtype=f32)
    z[0, 0], z[0, 1] = 0.0, -0.0
    g, gmin = _ground(z)
    assert np.signbit(g[0, 0]) and np.signbit(gmin), 'the minimum is taken on the key: -0.0 < +0.0'
    # vz = (m6 dx + m7 dy) + m8 dz keeps a -0.0 only when every term is one: dx, dy < 0 under m6 = m7 = 0
    pts = np.array([[-0.5, -0.5, 0.0, 900], [-0.45, -0.5, -0.0, 900], [-0.5, -0.45, 0.0, 900]], dtype=f32)
    p = ops.make_raster_params(bev_img_offset=(-1.0, -1.0))
    _, _, cmin = gr.tile_ground(pts, [0, 3], [p], 96, 96, 32)
    assert cmin[0, 0, 0] == 0 and np.signbit(cmin[0, 0, 0]) and np.isnan(cmin[0, 1, 1])


def test_reference_cells_select_and_non_finite_points():
    p = ops.make_raster_params(img_reso=(0.0625, 0.0625))         # 96 x 96 pixels of 1/16 m: cells of 2 m at cell_px 32
    pts = np.array([[0.5, 0.5, 1.0, 900], [0.6, 0.5, 0.25, 900], [2.5, 0.5, 3.0, 900], [0.5, 4.5, NaN, 900], [0.5, 4.5, np.inf, 900],
                    [0.7, 0.7, 2.0, 900], [99.0, 0.5, -9.0, 900]], dtype=f32)
    ground, gmin, cmin = gr.tile_ground(pts, [0, len(pts)], [p], 96, 96, 32)
    assert cmin[0, 0, 0] == 0.25 and cmin[0, 1, 0] == 3.0 and np.isnan(cmin[0, 0, 2]), 'NaN / inf heights and foreign points count nowhere'
    assert ground[0, 0, 0] == 0.25 and gmin[0] == 0.25            # {0.25, 3.0} -> the lower one
    out, offs = gr.select(pts, [0, len(pts)], [p], ground, 96, 96, 32, (0.0, 1.0))
    assert offs.tolist() == [0, 2] and np.array_equal(out, pts[[0, 1]]), 'input order; 2.75 and 1.75 above ground are out'
    out, offs = gr.select(pts, [0, len(pts)], [p], ground, 96, 96, 32, (-np.inf, np.inf))
    assert offs.tolist() == [0, 4] and np.array_equal(out, pts[[0, 1, 2, 5]])


# ------------------------------------------------------------------------------------------------ GroundFilter, ground_datum
def test_ground_filter_validation_and_immutability():
    f = GroundFilter()
    assert (f.height_range, f.cell_px, f.datum, f.datum_margin) == (None, 32, True, 1.0)
    g = GroundFilter(height_range=(-0.5, 1), cell_px=64, datum=False, datum_margin=0)
    assert g.height_range == (-0.5, 1.0) and g == GroundFilter((-0.5, 1.0), 64, False, 0.0) and hash(g) == hash(GroundFilter((-0.5, 1.0), 64, False, 0.0))
    assert g != f and 'cell_px=64' in repr(g)
    assert GroundFilter(height_range=(-math.inf, 2.0)).height_range == (-math.inf, 2.0)
    for kw, word in (({'height_range': (NaN, 1.0)}, 'NaN'), ({'height_range': (0.0, NaN)}, 'NaN'), ({'height_range': (2.0, 1.0)}, 'lo > hi'),
                     ({'cell_px': 7}, 'cell_px'), ({'cell_px': 129}, 'cell_px'), ({'cell_px': 32.5}, 'cell_px'), ({'cell_px': True}, 'cell_px'),
                     ({'datum_margin': -0.1}, 'datum_margin'), ({'datum_margin': NaN}, 'datum_margin'), ({'datum_margin': math.inf}, 'datum_margin')):
        with pytest.raises(ValueError, match=word):
            GroundFilter(**kw)
    with pytest.raises(AttributeError, match='immutable'):
        f.cell_px = 16
    with pytest.raises(AttributeError, match='immutable'):
        del f.datum
    with pytest.raises(AttributeError):
        f.other = 1


def test_ground_datum():
    assert ground_datum(2.0, 0.25, 1.0, -7.0) == 1.0               # an exact multiple stays where it is
    assert ground_datum(f32(3.5), 0.5, 0.0, -7.0) == 3.5
    d = ground_datum(-0.31, 0.05, 1.0, -7.0)                       # -1.31 / 0.05 = -26.2 -> -27 steps
    assert d == -27 * 0.05 and d <= -1.31 < d + 0.05
    d = ground_datum(12.34, 0.05, 1.0, 0.0)
    assert d == math.floor(11.34 / 0.05) * 0.05 and isinstance(d, float) and d <= 11.34 < d + 0.05
    assert ground_datum(math.inf, 0.05, 1.0, -7.0) == -7.0 and ground_datum(f32(np.inf), 0.05, 1.0, 3) == 3.0
    for bad in (NaN, -math.inf):
        with pytest.raises(ValueError):
            ground_datum(bad, 0.05, 1.0, 0.0)


# ------------------------------------------------------------------------------------------------ Runner plumbing, device calls stubbed
class _Cfg(dict):
    list_img_size_xy = [1152, 1152]


def _runner(**cfg):
    r = Runner.__new__(Runner)
    r.cfg, r.device, r.net = _Cfg(cfg), torch.device('cpu'), None
    return r


def test_las_ground_argument_and_cfg_default():
    assert _runner()._las_ground(None) is None, "absent: today's behaviour"
    assert _runner(las_ground={'height_range': (-0.5, 1.0), 'cell_px': 16})._las_ground(None) == GroundFilter((-0.5, 1.0), 16)
    mine = GroundFilter(datum=False)
    assert _runner(las_ground={'cell_px': 16})._las_ground(mine) is mine, 'the argument wins over the config'
    with pytest.raises(TypeError, match='GroundFilter'):
        _runner()._las_ground({'cell_px': 16})
    with pytest.raises(ValueError, match='cell_px'):
        _runner(las_ground={'cell_px': 4})._las_ground(None)
    for fn in (Runner.infer_las_strip_to_map, Runner.infer_las_to_map):
        assert inspect.signature(fn).parameters['ground'].default is None
    from lanemapping_amd.runner_ranks import MultiGpuRunner
    with pytest.raises(NotImplementedError, match='single-GPU'):
        MultiGpuRunner.infer_las_strip_to_map(None, 'a.las', [], ground=GroundFilter())


def _batch():
    plist = [{'coor_las_path': '', 'las_read_offset': [1.0, 2.0, 3.0], 'las_rotation_trans_quan': [40.0 * t, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0],
              'bev_img_offset': [0.0, 0.0], 'img_reso': [0.05, 0.05], 'local_min_ele': -4.0, 'ele_reso': 0.05} for t in range(3)]
    return plist, [io_utils.raster_params_from_dict(p) for p in plist]


def test_follow_ground_sets_the_datum_in_both_places_and_selects(monkeypatch, tmp_path):
    calls = []
    points = torch.zeros((10, 4))
    gmin = torch.tensor([2.0, math.inf, 8.03], dtype=torch.float32)

    def tile_ground(pts, offs, rpar, H, W, cell_px=32, want_cell_min=False):
        calls.append(('ground', list(offs), [r.local_min_ele for r in rpar], H, W, cell_px))
        return torch.zeros((3, 36, 36)), gmin

    def ground_select(pts, offs, rpar, ground, H, W, cell_px, h_range):
        calls.append(('select', list(offs), [r.local_min_ele for r in rpar], tuple(ground.shape), cell_px, h_range))
        return pts[:6], [0, 1, 1, 6]

    monkeypatch.setattr(ops, 'tile_ground', tile_ground)
    monkeypatch.setattr(ops, 'ground_select', ground_select)
    plist, rpar = _batch()
    names = ['t0', 't1', 't2']
    r = _runner()
    gf = GroundFilter(height_range=(-0.5, 1.0))
    pl2, pts2, offs2, rp2 = r._follow_ground(gf, names, plist, points, [2, 4, 4, 10], rpar, 1152, 1152, str(tmp_path))
    want = [ground_datum(2.0, 0.05, 1.0, -4.0), -4.0, ground_datum(float(f32(8.03)), 0.05, 1.0, -4.0)]
    assert want[0] == 1.0 and want[1] == -4.0 and 6.95 <= want[2] <= 7.03
    assert [p['local_min_ele'] for p in pl2] == want, 'the dict the back-projection reads'
    assert [r_.local_min_ele for r_ in rp2] == [float(f32(w)) for w in want], 'the struct the rasteriser reads: the same datum in float32'
    assert all(p['local_min_ele'] == -4.0 for p in plist) and all(r_.local_min_ele == -4.0 for r_ in rpar), "the caller's parameters are not edited"
    assert calls[0] == ('ground', [2, 4, 4, 10], [-4.0] * 3, 1152, 1152, 32)
    assert calls[1] == ('select', [2, 4, 4, 10], [float(f32(w)) for w in want], (3, 36, 36), 32, (-0.5, 1.0)) and len(calls) == 2
    assert offs2 == [0, 1, 1, 6] and pts2.shape[0] == 6, 'the tiles are rasterised from the selected ranges'
    for name, p in zip(names, pl2):
        back = io_utils.load_pc_2_img_transform_paras(os.path.join(str(tmp_path), 'params', name + '.txt'))
        assert back == p, 'the parameters actually used are written'

    # datum only: no selection, the points pass through; selection only: the parameters stay, but are still written
    calls.clear()
    pl3, pts3, offs3, _ = r._follow_ground(GroundFilter(cell_px=64), names, plist, points, [2, 4, 4, 10], rpar, 1152, 1152, str(tmp_path / 'b'))
    assert [c[0] for c in calls] == ['ground'] and calls[0][5] == 64 and pts3 is points and offs3 == [2, 4, 4, 10]
    assert [p['local_min_ele'] for p in pl3] == want
    calls.clear()
    pl4, _, offs4, rp4 = r._follow_ground(GroundFilter(height_range=(0.0, 2.0), datum=False), names, plist, points, [2, 4, 4, 10], rpar, 1152, 1152,
                                          str(tmp_path / 'c'))
    assert [c[0] for c in calls] == ['ground', 'select'] and offs4 == [0, 1, 1, 6]
    assert [p['local_min_ele'] for p in pl4] == [-4.0] * 3 and [r_.local_min_ele for r_ in rp4] == [-4.0] * 3
    assert sorted(os.listdir(str(tmp_path / 'c' / 'params'))) == ['t0.txt', 't1.txt', 't2.txt']
