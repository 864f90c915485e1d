"""CPU: the host side of the marking profile (las_io.line_stations, las_io.MarkingSurvey, las_io.marking_summary, the brute force of
tests/profile_ref.py) and the argument checks of the Runner entries that need no device."""
import os
import re

import numpy as np
import pytest

import label_ref as lr
import profile_ref as pr
from lanemapping_amd import las_io, ops
from lanemapping_amd.las_io import MarkingSurvey

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lines():
    return [l + lr.SHIFT for l in lr.scene_lines()]


# ------------------------------------------------------------------------------------------------ line_stations
def test_line_stations_rows_follow_line_segments():
    lines = _lines()
    seg = las_io.line_segments(lines, lr.SHIFT)
    st, bs = las_io.line_stations(lines, lr.SHIFT, 0.25)
    assert st.shape == (len(seg), 4) and st.dtype == f32 and bs.shape == (len(lines) + 1,) and bs.dtype == np.int32
    want_st, want_bs = pr.stations_ref(seg, len(lines), 0.25)
    assert np.array_equal(st.view(np.int32), want_st.view(np.int32)) and np.array_equal(bs, want_bs)
    of_line = lr.seg_lines(seg)
    # row order: s0 starts at 0 with every line and grows by the row's own length inside it; the lengths are those of the segment rows
    for k in range(1, 6):
        rows = np.nonzero(of_line == k)[0]
        assert st[rows[0], 0] == 0 and np.array_equal(rows, np.arange(rows[0], rows[-1] + 1))
        assert np.allclose(np.diff(st[rows, 0]), st[rows[:-1], 1], rtol=1e-6, atol=0)
    assert np.allclose(st[:, 1], np.hypot(seg[:, 3], seg[:, 4]), rtol=1e-6) and not st[:, 3].any()
    # lines 1, 2, 4: 20 segments of exactly 2 m
    one = np.nonzero(of_line == 1)[0]
    assert np.array_equal(st[one, 0], np.arange(0, 40, 2, dtype=f32)) and (st[one, 1] == 2).all() and (st[one, 2] == 0.5).all()
    # the doubled vertex of line 5: len = rlen = 0, and s0 does not move over it
    five = np.nonzero(of_line == 5)[0]
    assert len(five) == 3 and st[five[0], 1] == 0 and st[five[0], 2] == 0 and st[five[1], 0] == 0 and st[five[2], 0] == 2
    # a one-vertex line owns no bins; a line of length exactly k bin owns k
    assert bs[6] == bs[5] and bs[-1] == bs[5]
    assert bs[1] - bs[0] == 160 and bs[5] - bs[4] == 16                      # 40 m and 0 + 2 + 2 m at 0.25
    for b, k in ((0.125, 320), (0.5, 80), (40.0, 1), (80.0, 1), (39.0, 2), (3.0, 14)):
        assert las_io.line_stations(lines[:1], lr.SHIFT, b)[1].tolist() == [0, k], b
    # only a doubled vertex: segments of length 0 still own one bin
    dot = [np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0]])]
    assert las_io.line_stations(dot, None, 0.25)[1].tolist() == [0, 1]
    assert las_io.line_stations([], None, 0.25)[1].tolist() == [0] and las_io.line_stations([], None, 0.25)[0].shape == (0, 4)
    for bad in (0, 0.0, -0.25, float('nan'), float('inf'), True, '0.25', None):
        with pytest.raises(ValueError, match='bin'):
            las_io.line_stations(lines, lr.SHIFT, bad)


# ------------------------------------------------------------------------------------------------ MarkingSurvey
def test_marking_survey_is_validated_and_immutable():
    s = MarkingSurvey()
    assert (s.bin, s.half_width, s.z_tol, s.min_intensity, s.min_points, s.max_gap, s.solid_cover) == (0.25, 0.3, 0.5, None, 3, 0.5, 0.8)
    assert 'plain defaults, not tuned' in MarkingSurvey.__doc__ and 'counts returns, not paint' in MarkingSurvey.__doc__
    assert s == MarkingSurvey() and hash(s) == hash(MarkingSurvey()) and s != MarkingSurvey(bin=0.5) and 'bin=0.25' in repr(s)
    assert MarkingSurvey(min_intensity=10000).min_intensity == 10000.0 and MarkingSurvey(half_width=16).half_width == 16.0
    assert MarkingSurvey(z_tol=float('inf')).z_tol == float('inf') and MarkingSurvey(max_gap=0).max_gap == 0.0
    with pytest.raises(AttributeError, match='immutable'):
        s.bin = 1.0
    with pytest.raises(AttributeError, match='immutable'):
        del s.bin
    nan, inf = float('nan'), float('inf')
    for key, values in (('bin', (0, -1.0, nan, inf, True, '1')), ('half_width', (-0.1, 16.5, nan, inf, True)), ('z_tol', (-1.0, nan, None)),
                        ('min_intensity', (nan, True, '5')), ('min_points', (0, -1, 2.5, True)), ('max_gap', (-0.1, nan, inf)),
                        ('solid_cover', (0, 1.5, nan, True))):
        for v in values:
            with pytest.raises(ValueError, match=key):
                MarkingSurvey(**{key: v})


# ------------------------------------------------------------------------------------------------ marking_summary
def _bins(n):
    b = np.zeros((n, 6), np.int64)
    b[:, 4], b[:, 5] = pr.Q_EMPTY_MIN, pr.Q_EMPTY_MAX
    return b


def _paint(b, rows, n=10, iq=24000, qmin=-26, qmax=26):
    b[rows, 0], b[rows, 1], b[rows, 2], b[rows, 3], b[rows, 4], b[rows, 5] = n, n * iq, 0, n * 26 * 26, qmin, qmax


def test_marking_summary_on_hand_made_bins():
    sv = MarkingSurvey(min_intensity=10000.0)
    # line 1: 3 m on / 3 m off over 24 m; line 2: solid but for a one-bin hole; line 3: empty; line 4: no bins; line 5: one short run
    bs = np.array([0, 96, 136, 156, 156, 196], np.int32)
    b = _bins(196)
    on = (np.arange(96) // 12) % 2 == 0
    _paint(b, np.nonzero(on)[0])
    _paint(b, 96 + np.arange(40), n=5, iq=20000, qmin=-50, qmax=52)
    b[96 + 17] = _bins(1)[0]
    _paint(b, 156 + np.arange(4, 10), n=3, iq=1000, qmin=10, qmax=30)
    b[156 + 20, 0] = 2                                                      # below min_points: not painted
    got = las_io.marking_summary(b, bs, sv)
    assert len(got) == 5
    one, two, three, four, five = got
    assert one['runs'] == [[0.0, 3.0], [6.0, 9.0], [12.0, 15.0], [18.0, 21.0]] and one['type'] == 'dashed' and one['cover'] == 0.5
    assert one['dash'] == 3.0 and one['gap'] == 3.0 and one['length'] == 24.0 and one['painted'] == 48
    assert one['width'] == 52 / 1024 and one['intensity'] == 24000.0
    assert two['type'] == 'solid' and two['runs'] == [[0.0, 10.0]] and two['painted'] == 39 and two['cover'] == 39 / 40
    assert two['width'] == 102 / 1024 and two['intensity'] == 20000.0 and two['gap'] is None and two['dash'] == 10.0
    assert three == {'length': 5.0, 'painted': 0, 'runs': [], 'cover': 0.0, 'type': 'none', 'dash': None, 'gap': None, 'width': None,
                     'intensity': None}
    assert four['type'] == 'none' and four['length'] == 0.0 and four['runs'] == []
    assert five['type'] == 'partial' and five['runs'] == [[1.0, 2.5]] and five['painted'] == 6 and five['width'] == 20 / 1024
    assert five['intensity'] == 1000.0 and five['cover'] == 6 / 40
    assert got == pr.summary_of(b, bs, sv)
    # the hole stays open without max_gap: two runs, still 'solid' by cover; with a lower cover demanded 'dashed' shows
    open_ = las_io.marking_summary(b, bs, MarkingSurvey(max_gap=0.0))[1]
    assert open_['runs'] == [[0.0, 4.25], [4.5, 10.0]] and open_['type'] == 'solid' and open_['gap'] == 0.25
    assert las_io.marking_summary(b, bs, MarkingSurvey(max_gap=0.0, solid_cover=1.0))[1]['type'] == 'dashed'
    # max_gap joins the 3 m gaps of line 1 when it reaches them: one run, yet cover stays the painted share
    far = las_io.marking_summary(b, bs, MarkingSurvey(max_gap=3.0))[0]
    assert far['runs'] == [[0.0, 21.0]] and far['cover'] == 0.5 and far['type'] == 'partial'
    # min_points
    assert las_io.marking_summary(b, bs, MarkingSurvey(min_points=4))[4]['type'] == 'none'
    assert las_io.marking_summary(b, bs, MarkingSurvey(min_points=2))[4]['painted'] == 7
    for s2 in (MarkingSurvey(max_gap=0.0), MarkingSurvey(max_gap=3.0), MarkingSurvey(min_points=2), MarkingSurvey(bin=0.1, max_gap=0.3)):
        assert las_io.marking_summary(b, bs, s2) == pr.summary_of(b, bs, s2), s2
    with pytest.raises(TypeError, match='MarkingSurvey'):
        las_io.marking_summary(b, bs, {'bin': 0.25})
    with pytest.raises(ValueError, match='bins'):
        las_io.marking_summary(b[:-1], bs, sv)
    with pytest.raises(ValueError, match='bins'):
        las_io.marking_summary(b.astype(np.int32), bs, sv)


# ------------------------------------------------------------------------------------------------ the brute force itself
def test_reference_puts_the_special_points_where_the_rule_says():
    lines = _lines()
    seg = las_io.line_segments(lines, lr.SHIFT)
    g, _, _ = ops.line_index_host(seg, lr.HW)
    pts, first = pr.scene_points(seg, (g.x0, g.y0, g.cell, g.nx, g.ny))
    st, bs = las_io.line_stations(lines, lr.SHIFT, pr.BIN_EXACT)
    bins, terms, line, win = pr.profile_f32(pts, seg, st, bs, pr.BIN_EXACT, lr.HW, lr.ZTOL)
    pr.check_scene(terms, line, win, first, bs, pr.BIN_EXACT)
    assert bins.shape == (int(bs[-1]), 6) and bins[:, 0].sum() == (line > 0).sum() > 300
    empty = bins[:, 0] == 0
    assert empty.any() and (bins[empty] == [0, 0, 0, 0, pr.Q_EMPTY_MIN, pr.Q_EMPTY_MAX]).all()
    assert (bins[~empty, 4] <= bins[~empty, 5]).all() and bins[40, 4] <= -102 and bins[40, 5] >= 102
    # a NaN intensity counts with iq = 0 when no min_intensity is asked; the pruned form agrees with the brute force
    nan_i = lr.INTENSITY[2]
    assert line[nan_i] == 1 and terms['iq'][nan_i] == 0 and terms['iq'][lr.INTENSITY[0]] == 500
    pruned = pr.profile_f32_pruned(pts, seg, st, bs, pr.BIN_EXACT, lr.HW, lr.ZTOL)
    assert np.array_equal(pruned[0], bins) and np.array_equal(pruned[3], win)
    # two halves accumulate to the whole
    h = len(pts) // 2
    first_half = pr.profile_f32(pts[:h], seg, st, bs, pr.BIN_EXACT, lr.HW, lr.ZTOL)[0]
    assert np.array_equal(pr.profile_f32(pts[h:], seg, st, bs, pr.BIN_EXACT, lr.HW, lr.ZTOL, bins=first_half)[0], bins)


# ------------------------------------------------------------------------------------------------ the Runner entries
def test_runner_entries_refuse_a_wrong_survey_without_a_device():
    from lanemapping_amd.config import Config
    from lanemapping_amd.runner import Runner
    r = Runner.__new__(Runner)
    r.cfg = Config({'list_img_size_xy': [1152, 1152]})
    with pytest.raises(TypeError, match='survey must be a las_io.MarkingSurvey'):
        r.infer_las_strip_to_map('none.las', [], survey={'bin': 0.25})
    with pytest.raises(TypeError, match='survey must be a las_io.MarkingSurvey'):
        r.infer_las_to_map([], survey=0.25)
    with pytest.raises(TypeError, match='survey must be a las_io.MarkingSurvey'):
        r.infer_las_to_map([], survey=las_io.MarkingLabels())
    r.cfg = Config({'list_img_size_xy': [1152, 1152], 'las_survey': {'bin': -1.0}})
    with pytest.raises(ValueError, match='bin'):
        r.infer_las_to_map([])
    with pytest.raises(ValueError, match='bin'):
        r.infer_las_strip_to_map('none.las', [])
    with pytest.raises(TypeError, match='MarkingSurvey'):
        las_io.survey_las(['none.las'], [], {'bin': 0.25}, None)


# ------------------------------------------------------------------------------------------------ header, build, binding
def test_the_entries_are_declared_bound_and_built_exact():
    from lanemapping_amd import build
    from lanemapping_amd._lib import SIGNATURES
    header = open(os.path.join(ROOT, 'include', 'lanemap_hip.h')).read()
    for name in ('lm_line_profile_points', 'lm_las_line_profile_records'):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
        assert params[0] == 'void* hip_stream' and len(params) == len(SIGNATURES[name][1]), name
        assert params[-2:] == ['long* bins', 'long n_bins'] and 'int accumulate' in params
    assert 'profile.hip' in build.SOURCES and 'profile.hip' in build.EXACT_FP
    csrc = os.path.join(ROOT, 'lanemapping_amd', 'csrc')
    for f in ('label.hip', 'profile.hip'):
        assert '#include "label_rule.h"' in open(os.path.join(csrc, f)).read()
    label = open(os.path.join(csrc, 'label.hip')).read()
    assert 'constexpr int PER = 4;' in label and 'constexpr int CHUNK = 256 * PER;' in label
