"""CPU: paint thresholds per line and station window, the host side - PaintThreshold's scope and window, las_io.PaintTable and the stage
options that take one, las_io.paint_table against the plain-loop restatement (tests/local_ref.py), the fallback chain window -> line ->
strip, and the planted two-line strip on which one number for the strip loses the dim line."""
import re

import numpy as np
import pytest

import local_ref as lo
import threshold_ref as tr
from lanemapping_amd import las_io
from lanemapping_amd.las_io import CrossSection, MarkingLabels, MarkingSurvey, PaintResidue, PaintTable, PaintThreshold


# ------------------------------------------------------------------------------------------------ the options
def test_scope_and_window_are_arguments_of_the_threshold():
    t = PaintThreshold()
    assert (t.scope, t.window) == ('strip', 50.0) and repr(t) == repr(PaintThreshold(scope='strip', window=50)), 'the default prints as before'
    w = PaintThreshold(scope='window', window=20)
    assert (w.scope, w.window) == ('window', 20.0) and isinstance(w.window, float) and w != t and hash(w) != hash(t)
    assert eval(repr(w), {'PaintThreshold': PaintThreshold}) == w and "scope='window', window=20.0" in repr(w)
    assert w._replace(bin_shift=4).scope == 'window' and w._replace(scope='line') == PaintThreshold(scope='line', window=20)
    assert PaintThreshold(scope='line') != t and not hasattr(w, '__dict__')
    for name in ('scope', 'window'):
        with pytest.raises(AttributeError, match='immutable'):
            setattr(w, name, 1)
    assert las_io.THRESHOLD_SCOPES == ('strip', 'line', 'window')


@pytest.mark.parametrize('kwargs, what', [
    (dict(scope='tile'), 'scope='), (dict(scope=None), 'scope='), (dict(scope=1), 'scope='),
    (dict(window=0), 'window='), (dict(window=-5.0), 'window='), (dict(window=float('inf')), 'window='), (dict(window=float('nan')), 'window='),
    (dict(window='x'), 'window='), (dict(window=True), 'window='),
])
def test_the_threshold_refuses_a_bad_scope_or_window(kwargs, what):
    with pytest.raises(ValueError, match=re.escape(what)):
        PaintThreshold(**kwargs)


def test_paint_table_is_a_value_and_validates():
    t = PaintTable([100, 200.5, 300], [0, 1, 1, 3], 50, [0, 1, 2])
    assert issubclass(PaintTable, las_io._Options) and not hasattr(t, '__dict__')
    assert t.thr.dtype == np.float32 and t.win_start.dtype == np.int32 and t.source.dtype == np.uint8 and t.window == 50.0
    assert t.thr.tolist() == [100.0, 200.5, 300.0] and t.win_start.tolist() == [0, 1, 1, 3] and t.source.tolist() == [0, 1, 2]
    assert t == PaintTable(np.float32([100, 200.5, 300]), np.int64([0, 1, 1, 3]), 50.0, [0, 1, 2]) and hash(t) == hash(eval(repr(t), {'PaintTable': PaintTable}))
    assert t != PaintTable([100, 200.5, 301], [0, 1, 1, 3], 50, [0, 1, 2]) and t != PaintTable([100, 200.5, 300], [0, 1, 1, 3], 51, [0, 1, 2])
    assert PaintTable([1.0], [0, 1], 5).source.tolist() == [0] and len(PaintTable([], [0], 5).thr) == 0
    with pytest.raises(AttributeError, match='immutable'):
        t.window = 1.0
    with pytest.raises(ValueError):
        t.thr[0] = 1.0                                                     # the arrays are read-only
    for args, what in ((([1.0, float('nan')], [0, 2], 5), 'thr'), (([1.0, float('inf')], [0, 2], 5), 'thr'), (([[1.0]], [0, 1], 5), 'thr'),
                       (([1.0, 2.0], [0, 2, 1], 5), 'win_start'), (([1.0, 2.0], [1, 2], 5), 'win_start'), (([1.0, 2.0], [0, 1], 5), 'win_start'),
                       (([1.0, 2.0], [0.0, 2.0], 5), 'win_start'), (([1.0], [0, 1], 0), 'window='), (([1.0], [0, 1], float('inf')), 'window='),
                       (([1.0], [0, 1], 5, [3]), 'source'), (([1.0], [0, 1], 5, [0, 0]), 'source')):
        with pytest.raises(ValueError, match=re.escape(what)):
            PaintTable(*args)


def test_the_stage_options_take_a_table_wherever_they_take_auto():
    t = PaintTable([100.2, 70000, -3], [0, 2, 3], 50)
    assert MarkingLabels(min_intensity=t).min_intensity is t and MarkingSurvey(min_intensity=t).min_intensity is t
    assert PaintResidue(t).min_intensity is t and CrossSection(t).paint_intensity is t
    assert CrossSection(t).paint_iq.tolist() == [101, 65536, 0] and CrossSection(t).paint_iq.dtype == np.int32
    assert CrossSection(100.2).paint_iq == 101 and CrossSection(70000).paint_iq == 65536 and CrossSection(-3).paint_iq == 0
    assert MarkingSurvey(min_intensity='auto')._replace(min_intensity=t) == MarkingSurvey(min_intensity=t)
    for bad in ('table', [1.0], object()):
        with pytest.raises(ValueError, match='PaintTable'):
            MarkingLabels(min_intensity=bad)
        with pytest.raises(ValueError, match='PaintTable'):
            CrossSection(bad)
    # an unresolved 'auto' is still refused by the low-level functions
    for call, opt in ((las_io.survey_files, MarkingSurvey(min_intensity='auto')), (las_io.cross_files, CrossSection('auto')),
                      (las_io.residue_files, PaintResidue('auto'))):
        with pytest.raises(ValueError, match="'auto' is not resolved"):
            call([], [], opt)
    with pytest.raises(ValueError, match="'auto' is not resolved"):
        CrossSection('auto').paint_iq


# ------------------------------------------------------------------------------------------------ the policy
def _window_hist(rng, R, Z, NB, kind):
    if kind == 'sparse':
        h = rng.randint(0, 3, (R, Z, NB)) * (rng.rand(R, Z, NB) < 0.05)
    else:                                                            # bright inner rings over a dark road; window 1 has no paint
        b = np.arange(NB)
        h = np.zeros((R, Z, NB))
        for r in range(R):
            road = np.exp(-0.5 * ((b - (0.08 + 0.01 * r) * NB) / (0.03 * NB)) ** 2)
            paint = np.exp(-0.5 * ((b - (0.3 + 0.05 * r) * NB) / (0.05 * NB)) ** 2)
            for z in range(Z):
                h[r, z] = (3e4 if r != 2 else 3) * road + ((2e4 if r != 2 else 2) * paint if z < 2 and r != 1 else 0)
        h = rng.poisson(h)
    return h.astype(np.int64)


@pytest.mark.parametrize('bin_shift', [8, 6])
def test_the_table_policy_equals_the_plain_loop_restatement(bin_shift):
    rng = np.random.RandomState(5 + bin_shift)
    win_start = np.array([0, 3, 3, 4, 6], np.int32)                       # four lines: 3 windows, none, 1, 2
    for kind in ('paint', 'sparse'):
        for kw in (dict(), dict(min_returns=1, min_separation=0.0, tolerance_shift=1)):
            t = PaintThreshold(bin_shift=bin_shift, scope='window', window=25.0, **kw)
            hist_w = _window_hist(rng, 6, t.rings, t.n_counts, kind)
            thr, source, want = lo.table_policy(hist_w, win_start, bin_shift=bin_shift, **kw)
            if not want['strip']['supported']:
                with pytest.raises(ValueError, match='support no threshold'):
                    las_io.paint_table(hist_w, win_start, t)
                continue
            table, got = las_io.paint_table(hist_w, win_start, t)
            assert table.thr.tolist() == [float(np.float32(v)) for v in thr] and table.source.tolist() == source, (kind, kw)
            assert table.win_start.tolist() == win_start.tolist() and table.window == 25.0
            tr.same_group(got['strip'], want['strip'], 'strip')
            assert set(got['lines']) == {1, 2, 3, 4} and set(got['windows']) == {1, 2, 3, 4} and got['windows'][2] == []
            for k in want['lines']:
                tr.same_group(got['lines'][k], want['lines'][k], f'line {k}')
                assert len(got['windows'][k]) == len(want['windows'][k])
                for a, b in zip(got['windows'][k], want['windows'][k]):
                    tr.same_group(a, b, f'line {k} window')
            if kind == 'paint' and not kw:
                assert source[:3] == [0, 1, 1], 'window 1 has no paint and window 2 too few returns: both take the line\'s threshold'
                assert 0 in source[3:]
            # the per-line table is the sum of the windows, and the per-line policy of that sum is paint_threshold's
            per_line = las_io.line_hist_of_windows(hist_w, win_start)
            assert per_line.shape == (4,) + hist_w.shape[1:] and per_line.sum() == hist_w.sum() and not per_line[1].any()
            assert np.array_equal(per_line[0], hist_w[0] + hist_w[1] + hist_w[2]) and np.array_equal(per_line[3], hist_w[4] + hist_w[5])
            flat = las_io.paint_threshold(per_line, t)
            tr.same_group(flat['strip'], got['strip'], 'the strip of the summed table')
            for k in flat['lines']:
                tr.same_group(flat['lines'][k], got['lines'][k], f'line {k} of the summed table')
    t = PaintThreshold(bin_shift=bin_shift, scope='window', window=25.0)
    hist_w = _window_hist(rng, 6, t.rings, t.n_counts, 'paint')
    assert las_io.paint_table(hist_w, win_start, t, window=7.5)[0].window == 7.5
    with pytest.raises(ValueError, match='hist_w'):
        las_io.paint_table(hist_w[:, :-1], win_start, t)
    with pytest.raises(ValueError, match='win_start'):
        las_io.paint_table(hist_w, win_start[:-1], t)
    with pytest.raises(TypeError, match='PaintThreshold'):
        las_io.paint_table(hist_w, win_start, MarkingSurvey())


def _normal(rng, mean, sd, n, NB, shift):
    return np.bincount(np.clip(np.rint(rng.normal(mean, sd, n)), 0, 65535).astype(np.int64) >> shift, minlength=NB)


def _planted(rng, t, lines):
    """lines: per line a list of windows (paint mean, paint sd, asphalt mean, asphalt sd, inner paint, inner asphalt, outer asphalt) ->
    (hist_w, win_start).  The inner returns go to ring 0, the outer ones to the first outer ring."""
    rows, win_start = [], [0]
    for windows in lines:
        for pm, ps, am, asd, n_paint, n_in, n_out in windows:
            h = np.zeros((t.rings, t.n_counts), np.int64)
            h[t.inner_rings[0]] = _normal(rng, pm, ps, n_paint, t.n_counts, t.bin_shift) + _normal(rng, am, asd, n_in, t.n_counts, t.bin_shift)
            h[t.outer_rings[0]] = _normal(rng, am, asd, n_out, t.n_counts, t.bin_shift)
            rows.append(h)
        win_start.append(len(rows))
    return np.stack(rows), np.array(win_start, np.int32)


def test_the_fallback_chain_window_line_strip():
    """A hand-made table.  Line 1: a supported window, then one with too few returns -> the line's threshold.  Line 2: asphalt alone, no
    support in its window nor as a line -> the strip's.  A strip of asphalt alone raises."""
    t = PaintThreshold(scope='window', window=10.0)
    rng = np.random.RandomState(3)
    good = (20000, 1500, 4000, 400, 6000, 4000, 10000)
    few = (20000, 1500, 4000, 400, 60, 40, 100)                            # below min_returns = 1000
    bare = (4000, 400, 4000, 400, 0, 10000, 10000)
    hist_w, ws = _planted(rng, t, [[good, few], [bare]])
    table, found = las_io.paint_table(hist_w, ws, t, window=10.0)
    w = found['windows']
    assert w[1][0]['supported'] and not w[1][1]['supported'] and found['lines'][1]['supported']
    assert not w[2][0]['supported'] and not found['lines'][2]['supported'] and found['strip']['supported']
    assert table.source.tolist() == [0, 1, 2]
    assert table.thr.tolist() == [w[1][0]['threshold'], found['lines'][1]['threshold'], found['strip']['threshold']]
    assert all(4000 + 3 * 400 < v < 20000 - 3 * 1500 for v in table.thr.tolist())
    thr, source, _ = lo.table_policy(hist_w, ws)
    assert table.thr.tolist() == thr and table.source.tolist() == source
    with pytest.raises(ValueError, match=r'support no threshold.*separation 0\.\d+ with \d+ returns on the lines and \d+ beside them'):
        las_io.paint_table(*_planted(rng, t, [[bare], [bare]]), t)


def test_one_number_for_the_strip_loses_the_dim_line_and_a_table_does_not():
    """The planted strip of two lines: line 1 paint N(20000, 1500) on asphalt N(4000, 400), line 2 - an outer lane - paint N(3000, 250)
    on asphalt N(1000, 150); per line 10000 returns in the inner rings, paint six of ten, and 10000 asphalt returns in the outer ones.
    The strip's threshold lies above all of line 2's paint; each line's own lies between its asphalt and its paint.  The conditions are on
    the planted means and deviations (three deviations clear of either population), and the reference policy alone satisfies them.
    THE DRAW.  With exactly 6000 paint returns on both lines the strip's J has two maxima of exactly the same height, 6000 NO - one
    between line 2's asphalt and its paint, one between line 1's - and the policy takes the lower; either way one line is lost.  A scanner
    delivers no such tie: whether an inner return is paint is drawn, with probability 0.6, and the seed is one whose draw gives line 1
    the larger share (asserted), so that the strip's maximum is line 1's."""
    t = PaintThreshold(scope='line')
    rng = np.random.RandomState(12)
    p1, p2 = (int(rng.binomial(10000, 0.6)) for _ in range(2))
    assert p1 > p2 and abs(p1 - 6000) < 200 and abs(p2 - 6000) < 200, (p1, p2)
    l1, l2 = (20000, 1500, 4000, 400, p1, 10000 - p1, 10000), (3000, 250, 1000, 150, p2, 10000 - p2, 10000)
    hist_w, ws = _planted(rng, t, [[l1], [l2]])
    for policy in ('reference', 'package'):
        if policy == 'reference':
            thr, source, found = lo.table_policy(hist_w, ws)
        else:
            table, found = las_io.paint_table(hist_w, ws, t, window=1000.0)
            thr, source = table.thr.tolist(), table.source.tolist()
        strip = found['strip']['threshold']
        assert found['strip']['supported'] and strip > 3000 + 3 * 250, f'{policy}: the strip\'s number leaves line 2 without paint'
        assert 4000 + 3 * 400 < thr[0] < 20000 - 3 * 1500, policy
        assert 1000 + 3 * 150 < thr[1] < 3000 - 3 * 250, policy
        assert source == [0, 0] and thr[1] < 4000 - 3 * 400 < strip, f'{policy}: line 2\'s paint is darker than line 1\'s asphalt'
    flat = las_io.paint_threshold(las_io.line_hist_of_windows(hist_w, ws), t)
    assert flat['strip']['threshold'] == strip and flat['lines'][2]['threshold'] == thr[1] and flat['lines'][1]['threshold'] == thr[0]


def test_threshold_window_and_the_table_file(tmp_path):
    lines = [np.array([[0.0, 0.0, 0.0], [30.0, 40.0, 1.0]]), np.array([[0.0, 5.0, 0.0], [10.0, 5.0, 0.0], [10.0, 25.0, 0.0]]), np.zeros((1, 3))]
    assert las_io.threshold_window(lines, None, PaintThreshold(scope='window', window=12.5)) == 12.5
    w = las_io.threshold_window(lines, None, PaintThreshold(scope='line'))
    assert w == 100.0 and las_io.line_stations(lines, None, w)[1].tolist() == [0, 1, 2, 2], 'one window per line with segments'
    assert las_io.threshold_window([], None, PaintThreshold(scope='line')) == 1.0
    assert las_io.line_stations(lines, None, 12.5)[1].tolist() == [0, 4, 7, 7]
    t = PaintTable([1.5, 2.0, 70000.0], [0, 2, 2, 3], 12.5, [0, 2, 1])
    las_io.save_paint_table(str(tmp_path / 't.npy'), t)
    assert las_io.load_paint_table(str(tmp_path / 't.npy')) == t
    assert np.load(str(tmp_path / 't.npy')).shape == (4, 4)
