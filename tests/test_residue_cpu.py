"""CPU: the paint residue's host side - the numpy / scipy / Python reference itself (tests/residue_ref.py), las_io.PaintResidue,
las_io.residue_summary on hand-made statistics, the residue grid, and the argument checks of the Runner entries that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import label_ref as lr
import residue_ref as rr
from lanemapping_amd import las_io, ops
from lanemapping_amd.las_io import PaintResidue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _host_index(seg, reach):
    g, start, segs = ops.line_index_host(seg, reach)
    return ops.LineIndex(torch.from_numpy(np.array(seg)), torch.from_numpy(start), torch.from_numpy(segs), g, f32(reach))


# ------------------------------------------------------------------------------------------------ the reference
def test_the_two_component_references_agree_and_the_scenes_hold_what_they_are_meant_to():
    want = {'serpentine': (1, 1), 'u': (1, 1), 'diagonal': (1, 2), 'row_wrap': (4, 5)}
    for name, (keys, nx, ny) in rr.cell_scenes().items():
        assert np.array_equal(keys, np.unique(keys)) and (len(keys) == 0 or (keys.min() >= 0 and keys.max() < nx * ny)), name
        for conn in (8, 4):
            root = rr.roots(keys, nx, conn)                                    # (asserts that scipy and the union-find agree)
            assert np.array_equal(root[root], root) and (root <= np.arange(len(keys))).all(), name
            if name in want:
                assert len(np.unique(root)) == want[name][conn == 4], (name, conn)
    keys, nx, _ = rr.checkerboard()
    assert len(np.unique(rr.roots(keys, nx, 8))) == 1 and len(np.unique(rr.roots(keys, nx, 4))) == len(keys)
    keys, nx, _ = rr.serpentine()
    assert len(keys) == 32 * 64 + 31
    keys, nx, _ = rr.row_wrap()
    assert keys[1] == keys[0] + 1 and rr.roots(keys, nx, 8)[1] == 1            # consecutive keys across the row end: not joined
    keys, nx, _ = rr.random_grid()
    assert 3000 < len(keys) < 4500 and len(np.unique(rr.roots(keys, nx, 4))) > len(np.unique(rr.roots(keys, nx, 8))) > 1


def test_reference_statistics_are_python_integers_of_the_cells():
    keys, nx, _ = rr.diagonal_blobs()
    n, s = rr.point_counts(keys)
    comp, K = rr.dense_ids(rr.roots(keys, nx, 4))
    st = rr.stats(keys, nx, comp, K, n, s)
    assert st.shape == (2, 12) and st.dtype == np.int64
    assert st[0, [0, 3, 4, 5, 6, 7]].tolist() == [9, 9, 9, 15, 9, 15] and st[0, 8:].tolist() == [0, 2, 0, 2]
    assert st[1, [0, 3, 4]].tolist() == [9, 36, 36] and st[1, 8:].tolist() == [3, 5, 3, 5]
    assert st[:, 1].sum() == n.sum() and st[:, 2].sum() == s.sum()
    empty = rr.stats(keys[:0], nx, comp[:0], 0, n[:0], s[:0])
    assert empty.shape == (0, 12)


def test_reference_keys_put_the_special_points_where_the_rule_says():
    seg = las_io.line_segments([l + lr.SHIFT for l in lr.scene_lines()], lr.SHIFT)
    index = _host_index(seg, rr.REACH)
    grid = ops.residue_grid(index, rr.CELL)
    g = index.grid
    assert grid['x0'] == float(f32(g.x0)) and grid['nx'] * grid['cell'] >= g.nx * g.cell and grid['ny'] * grid['cell'] >= g.ny * g.cell
    pts, first = rr.scene_points(seg, (g.x0, g.y0, g.cell, g.nx, g.ny))
    key, iq = rr.keys_f32(pts, seg, rr.REACH, rr.ZTOL, rr.MIN_I, rr.CLEAR, grid)
    line, d2, _ = lr.label_f32(pts, seg, rr.REACH, rr.ZTOL, rr.MIN_I)
    clear2 = f32(rr.CLEAR) * f32(rr.CLEAR)
    for i in rr.AT_CLEAR:
        assert d2[i] == clear2 and line[i] == 1 and key[i] == -1, 'exactly clear away: no residue'
    assert d2[first + rr.AT_REACH] == f32(rr.REACH) * f32(rr.REACH) and key[first + rr.AT_REACH] >= 0
    assert key[first + rr.PAST_REACH] == -1 and key[first + rr.AT_ZTOL] >= 0 and key[first + rr.PAST_ZTOL] == -1
    assert key[first + rr.AT_MIN_I] >= 0 and key[first + rr.BELOW_MIN_I] == -1 and key[first + rr.NAN_I] == -1
    assert iq[first + rr.AT_MIN_I] == 500 and iq[first + 7:first + 10].tolist() == [1000, 1002, 65535]
    assert (iq[key < 0] == 0).all() and (key >= 0).sum() > 2000 and (key < 0).sum() > 500
    bad = ~np.isfinite(pts[:, :3]).all(axis=1)
    assert bad.sum() >= 6 and (key[bad] == -1).all()
    # the pipeline on it: the two bars and the stripe are blobs of their own
    cells, comp, st = rr.blobs([key], [iq], grid['nx'], 8)
    assert len(cells) == st[:, 0].sum() and st[:, 1].sum() == (key >= 0).sum() and st[:, 2].sum() == iq.sum()
    assert (st[:, 0] >= 20).sum() >= 3


# ------------------------------------------------------------------------------------------------ the host policy
GRID = {'x0': -7.0, 'y0': -7.0, 'cell': 0.1, 'nx': 400, 'ny': 200}
LINE = [np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [20.0, 0.0, 0.0]])]


def _blobs(cell_sets):
    keys, comp = [], []
    for k, xy in enumerate(cell_sets):
        keys += [y * GRID['nx'] + x for x, y in xy]
        comp += [k] * len(xy)
    order = np.argsort(keys)
    keys, comp = np.asarray(keys, np.int64)[order], np.asarray(comp, np.int32)[order]
    st = rr.stats(keys, GRID['nx'], comp, len(cell_sets), np.full(len(keys), 3, np.int64), np.full(len(keys), 3000, np.int64))
    return ops.ResidueBlobs(np.stack([keys % GRID['nx'], keys // GRID['nx']], axis=1).astype(np.int32), comp, st, dict(GRID))


def test_residue_summary_on_hand_made_statistics():
    across = [(x, y) for x in range(100, 104) for y in range(50, 90)]                       # 4 x 40 cells, centred on the line y = 0
    along = [(x, y) for x in range(150, 190) for y in range(78, 82)]                         # 40 x 4 cells, 1 m left of the line
    s2 = np.sqrt(0.5)
    tilted = [(x, y) for x in range(200, 260) for y in range(40, 100)
              if abs(((x - 230) + (y - 70)) * s2) <= 20 and abs(((y - 70) - (x - 230)) * s2) <= 2]
    square = [(x, y) for x in range(300, 306) for y in range(60, 66)]
    small = [(x, y) for x in range(350, 353) for y in range(60, 63)]
    res = PaintResidue(min_intensity=500.0)
    out = las_io.residue_summary(_blobs([across, along, tilted, square, small]), LINE, res)
    assert [b['blob'] for b in out] == [1, 2, 3, 4], 'the blob below min_cells is dropped'
    a, b, c, d = out
    assert a['shape'] == 'across' and abs(a['length'] - 4.0) < 1e-9 and abs(a['width'] - 0.4) < 1e-9 and abs(a['fill'] - 1.0) < 1e-9
    assert abs(a['heading'] - 90.0) < 1e-9 and a['line'] == 1 and abs(a['offset']) < 1e-9 and a['cells'] == 160 and a['points'] == 480
    assert np.allclose(a['centre'], [3.2, 0.0]) and abs(a['area'] - 1.6) < 1e-9 and a['intensity'] == 1000.0
    assert np.allclose(a['bbox'], [3.0, -2.0, 3.4, 2.0])
    assert b['shape'] == 'along' and abs(b['length'] - 4.0) < 1e-9 and abs(b['width'] - 0.4) < 1e-9 and abs(b['heading']) < 1e-9
    assert abs(b['offset'] - 1.0) < 1e-9 and b['line'] == 1
    assert c['shape'] == 'oblique' and abs(c['heading'] - 45.0) < 1.0 and c['length'] / c['width'] > 5 and 0.8 < c['fill'] < 1.1
    assert d['shape'] == 'compact' and abs(d['length'] - 0.6) < 1e-9 and abs(d['width'] - 0.6) < 1e-9
    # a shift moves the frame, a line on the right of the blob flips the offset's sign, no line: no `line`
    moved = las_io.residue_summary(_blobs([along]), [LINE[0] + [100.0, 50.0, 0.0]], res, shift=[100.0, 50.0, 0.0])[0]
    assert np.allclose(moved['centre'], [110.0, 51.0]) and abs(moved['offset'] - 1.0) < 1e-9
    back = las_io.residue_summary(_blobs([along]), [LINE[0][::-1]], res)[0]
    assert abs(back['offset'] + 1.0) < 1e-9 and back['shape'] == 'along'
    alone = las_io.residue_summary(_blobs([along, square]), [], res)
    assert [(v['line'], v['offset'], v['shape']) for v in alone] == [(None, None, 'oblique'), (None, None, 'compact')]
    assert las_io.residue_summary(_blobs([]), LINE, res) == []
    # min_points, elongated and angle_tol_deg are the policy's
    assert las_io.residue_summary(_blobs([across]), LINE, PaintResidue(500.0, min_points=481)) == []
    assert las_io.residue_summary(_blobs([across]), LINE, PaintResidue(500.0, elongated=11.0))[0]['shape'] == 'compact'
    assert las_io.residue_summary(_blobs([tilted]), LINE, PaintResidue(500.0, angle_tol_deg=45.0))[0]['shape'] in ('along', 'across')
    with pytest.raises(TypeError, match='PaintResidue'):
        las_io.residue_summary(_blobs([across]), LINE, {'min_intensity': 500.0})


# ------------------------------------------------------------------------------------------------ validation
def test_paint_residue_is_validated_and_immutable():
    r = PaintResidue(500)
    assert (r.min_intensity, r.clear, r.reach, r.z_tol, r.cell, r.connectivity, r.min_cells, r.min_points, r.elongated, r.angle_tol_deg) == \
        (500.0, 0.3, 6.0, 0.5, 0.1, 8, 20, 20, 2.0, 30.0)
    assert 'plain defaults, not tuned' in PaintResidue.__doc__
    with pytest.raises(TypeError):
        PaintResidue()                                                         # min_intensity is required
    for kw, what in (({'min_intensity': float('nan')}, 'min_intensity'), ({'min_intensity': float('inf')}, 'min_intensity'),
                     ({'min_intensity': None}, 'min_intensity'), ({'min_intensity': True}, 'min_intensity'),
                     ({'clear': -0.1}, 'clear'), ({'clear': 6.0}, 'clear'), ({'clear': 7.0}, 'clear'), ({'reach': 16.5}, 'reach'),
                     ({'reach': 0.0}, 'reach'), ({'reach': float('nan')}, 'reach'), ({'z_tol': -1.0}, 'z_tol'), ({'z_tol': float('nan')}, 'z_tol'),
                     ({'cell': 0.0}, 'cell'), ({'cell': float('inf')}, 'cell'), ({'connectivity': 3}, 'connectivity'),
                     ({'connectivity': 6}, 'connectivity'), ({'min_cells': 0}, 'min_cells'), ({'min_points': 1.5}, 'min_points'),
                     ({'elongated': 0.5}, 'elongated'), ({'angle_tol_deg': 50.0}, 'angle_tol_deg')):
        with pytest.raises(ValueError, match=what):
            PaintResidue(**{'min_intensity': 500.0, **kw})
    assert PaintResidue(500.0, reach=16.0, clear=0.0, z_tol=float('inf'), connectivity=4).connectivity == 4
    with pytest.raises(AttributeError):
        r.clear = 1.0
    assert r == PaintResidue(500.0) and hash(r) == hash(PaintResidue(500.0)) and r != PaintResidue(501.0) and 'clear=0.3' in repr(r)


def test_residue_grid_covers_the_index_and_refuses_a_side_above_2_to_20():
    seg = las_io.line_segments([np.array([[0.0, 0.0, 0.0], [1000.0, 0.0, 0.0]])])
    index = _host_index(seg, 6.0)
    g = ops.residue_grid(index, 0.1)
    assert g['nx'] >= 10120 and g['ny'] >= 120 and g['nx'] < 10300
    with pytest.raises(ValueError, match='nx='):
        ops.residue_grid(index, 0.0005)
    for bad in (0.0, -1.0, float('nan'), float('inf'), True):
        with pytest.raises(ValueError, match='cell='):
            ops.residue_grid(index, bad)
    with pytest.raises(TypeError, match='LineIndex'):
        ops.residue_grid(seg, 0.1)
    empty = ops.residue_grid(_host_index(np.zeros((0, 8), f32), 6.0), 0.1)
    assert (empty['nx'], empty['ny']) == (0, 0)


def test_runner_entries_take_the_cfg_key_and_refuse_a_wrong_residue_without_a_device():
    from lanemapping_amd.config import Config
    from lanemapping_amd.runner import Runner
    r = Runner.__new__(Runner)
    r.cfg = Config({'list_img_size_xy': [1152, 1152]})
    assert r._las_residue(None) is None
    with pytest.raises(TypeError, match='residue must be a las_io.PaintResidue'):
        r.infer_las_strip_to_map('none.las', [], residue={'min_intensity': 500.0})
    with pytest.raises(TypeError, match='residue must be a las_io.PaintResidue'):
        r.infer_las_to_map([], residue=500.0)
    with pytest.raises(TypeError, match='residue must be a las_io.PaintResidue'):
        r.infer_las_to_map([], residue=las_io.MarkingSurvey())
    r.cfg = Config({'list_img_size_xy': [1152, 1152], 'las_residue': {'min_intensity': 500.0, 'clear': 0.4}})
    assert r._las_residue(None) == PaintResidue(500.0, clear=0.4) and r._las_residue(PaintResidue(7.0)) == PaintResidue(7.0)
    r.cfg = Config({'list_img_size_xy': [1152, 1152], 'las_residue': {'min_intensity': 500.0, 'clear': 9.0}})
    with pytest.raises(ValueError, match='clear'):
        r.infer_las_to_map([])
    with pytest.raises(ValueError, match='clear'):
        r.infer_las_strip_to_map('none.las', [])
    with pytest.raises(TypeError, match='PaintResidue'):
        las_io.residue_files([('none.las', None, None)], [], {'min_intensity': 500.0})


# ------------------------------------------------------------------------------------------------ header, build, binding
def test_the_entries_are_declared_bound_and_built_exact():
    from lanemapping_amd import build
    from lanemapping_amd._lib import SIGNATURES
    header = open(os.path.join(ROOT, 'include', 'lanemap_hip.h')).read()
    for name, last in (('lm_residue_keys', ['long* key', 'int* iq']), ('lm_cell_components', ['int* root', 'int* err']),
                       ('lm_residue_stats', ['long K', 'long* stats'])):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
        assert params[0] == 'void* hip_stream' and len(params) == len(SIGNATURES[name][1]) and params[-2:] == last, name
    assert 'residue.hip' in build.SOURCES and 'residue.hip' in build.EXACT_FP
    src = open(os.path.join(ROOT, 'lanemapping_amd', 'csrc', 'residue.hip')).read()
    assert '#include "label_rule.h"' in src and '__shared__' not in src
    assert 'constexpr int PER = 4;' in src and 'constexpr int CHUNK = 256 * PER;' in src
    assert 'NOT HERE: a raw-records entry' in header
