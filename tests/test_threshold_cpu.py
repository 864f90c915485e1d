"""CPU: the paint threshold's host side - las_io.PaintThreshold, las_io.paint_threshold against the Python-integer restatement
(tests/threshold_ref.py) on random and on planted histograms, 'auto' in the four option classes and its refusal where nothing resolves
it, the Runner's `threshold=` argument, and the header block of the two entries."""
import os
import re

import numpy as np
import pytest

import threshold_ref as tr
from lanemapping_amd import las_io, ops
from lanemapping_amd.las_io import CrossSection, MarkingLabels, MarkingSurvey, PaintResidue, PaintThreshold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the options
def test_defaults_and_derived_integers():
    t = PaintThreshold()
    assert (t.half_width, t.ring, t.inner, t.outer, t.z_tol, t.bin_shift, t.min_returns, t.min_separation, t.tolerance_shift) == \
        (0.625, 0.0625, 0.125, 0.375, 0.5, 6, 1000, 0.05, 5)
    assert (t.ring_q, t.inner_q, t.outer_q, t.hq, t.rings, t.n_counts) == (64, 128, 384, 640, 11, 1024)
    assert t.inner_rings == [0, 1] and t.outer_rings == [6, 7, 8, 9, 10]
    assert tr.rings(0.625, 0.0625, 0.125, 0.375) == (64, 11, [0, 1], [6, 7, 8, 9, 10])
    assert (t.hq, t.rings, t.n_counts) == tr.shape(0.625, 64, 6) == ops.hist_shape(0.625, 64, 6)
    assert ops.hist_shape(0.3125, 1000, 0) == (320, 1, 65536) and ops.hist_shape(0.03, 1, 8) == (31, 32, 256)
    assert 1.949 < tr.KS < las_io.KS_COEFF == 1.95, 'the coefficient is sqrt(-ln(0.0005) / 2), rounded up'
    assert t == PaintThreshold(**{k: getattr(t, k) for k in t.__slots__}) and t != PaintThreshold(bin_shift=5)
    assert PaintThreshold(ring=0.0001).ring_q == 1
    with pytest.raises(AttributeError):
        t.ring = 1.0


def test_paint_threshold_is_a_value_like_the_other_option_classes():
    """What tests/test_las_select_cpu.py checks of every option class, and what it does not: the types of the stored values."""
    assert las_io.PaintThreshold is PaintThreshold and issubclass(PaintThreshold, las_io._Options)
    with pytest.raises(AttributeError):
        las_io.no_such_name
    kwargs = dict(half_width=0.5, ring=0.03125, inner=0.0625, outer=0.25, z_tol=1, bin_shift=4, min_returns=10, min_separation=0.1,
                  tolerance_shift=3)
    x = PaintThreshold(**kwargs)
    assert tuple(kwargs) == PaintThreshold.__slots__ and all(getattr(x, k) == v for k, v in kwargs.items())
    assert eval(repr(x), {'PaintThreshold': PaintThreshold}) == x and hash(x) == hash(PaintThreshold(**kwargs)) and x != PaintThreshold()
    assert x != tuple(kwargs.values()) and not hasattr(x, '__dict__') and isinstance(x.z_tol, float) and isinstance(x.bin_shift, int)
    for k in PaintThreshold.__slots__:
        with pytest.raises(AttributeError, match='immutable'):
            setattr(x, k, 1)
        with pytest.raises(AttributeError, match='immutable'):
            delattr(x, k)


@pytest.mark.parametrize('kwargs, what', [
    (dict(inner=0.01), 'inner set is empty'),                         # no ring of 64/1024 m ends within 10/1024 m
    (dict(ring=0.1, outer=0.62), 'outer set is empty'),                # rings start at 0, 102, ..., 612 < 635
    (dict(inner=0.4, outer=0.375), 'inner='),                          # inner > outer
    (dict(outer=0.7), 'outer='),                                       # outer > half_width
    (dict(half_width=16.5, outer=1.0), 'half_width='),
    (dict(half_width=-1.0), 'half_width='), (dict(half_width=True), 'half_width='),
    (dict(ring=0.0), 'ring='), (dict(ring=float('inf')), 'ring='), (dict(ring='x'), 'ring='),
    (dict(inner=-0.1), 'inner='), (dict(outer=float('nan')), 'outer='),
    (dict(z_tol=16.5), 'z_tol='), (dict(z_tol=-1.0), 'z_tol='),
    (dict(bin_shift=9), 'bin_shift='), (dict(bin_shift=-1), 'bin_shift='), (dict(bin_shift=2.0), 'bin_shift='),
    (dict(min_returns=0), 'min_returns='), (dict(min_separation=1.5), 'min_separation='), (dict(min_separation=-0.1), 'min_separation='),
    (dict(tolerance_shift=0), 'tolerance_shift='), (dict(tolerance_shift=31), 'tolerance_shift='),
])
def test_the_constructor_refuses(kwargs, what):
    with pytest.raises(ValueError, match=re.escape(what)):
        PaintThreshold(**kwargs)


# ------------------------------------------------------------------------------------------------ the policy
def _random_hist(rng, L, Z, NB, kind):
    if kind == 'sparse':                                             # mostly empty: ties, empty lines, J = 0 everywhere for some
        h = rng.randint(0, 3, (L, Z, NB)) * (rng.rand(L, Z, NB) < 0.02)
        h[0] = 0
    elif kind == 'flat':
        h = rng.randint(0, 50, (L, Z, NB))
    else:                                                            # bright inner rings over a dark road, large counts
        b = np.arange(NB)
        road = np.exp(-0.5 * ((b - 0.1 * NB) / (0.03 * NB)) ** 2)
        paint = np.exp(-0.5 * ((b - 0.4 * NB) / (0.05 * NB)) ** 2)
        h = np.zeros((L, Z, NB))
        for k in range(L):
            for r in range(Z):
                h[k, r] = 3e6 * road + (2e6 * paint if r < 2 and k != 1 else 0)
        h = rng.poisson(h)
    return h.astype(np.int64)


@pytest.mark.parametrize('bin_shift, kinds', [(8, ('sparse', 'flat', 'paint')), (6, ('sparse', 'flat', 'paint')), (0, ('paint',))])
def test_the_policy_equals_the_python_integer_restatement(bin_shift, kinds):
    rng = np.random.RandomState(17 + bin_shift)
    for kind in kinds:
        variants = (dict(), dict(min_returns=1, min_separation=0.0, tolerance_shift=1), dict(ring=0.03125, inner=0.0625, outer=0.5))
        for kw in variants[:1 if bin_shift == 0 else 3]:                  # (NB = 65536: 3 groups of 65536 Python integers are enough)
            t = PaintThreshold(bin_shift=bin_shift, **kw)
            L = 2 if bin_shift == 0 else 3
            hist = _random_hist(rng, L, t.rings, t.n_counts, kind)
            got = las_io.paint_threshold(hist, t)
            want = tr.policy(hist, bin_shift=bin_shift, **kw)
            tr.same_policy(got, want, f'NB={t.n_counts}, {kind}, {kw}')
            assert list(got['lines']) == list(range(1, L + 1)) and t.n_counts in (256, 1024, 65536)
            if kind == 'paint' and not kw:
                assert got['strip']['supported'] and got['lines'][1]['supported'] and not got['lines'][2]['supported']
                lo, hi = got['strip']['plateau']
                assert lo <= got['strip']['threshold'] <= hi and 0.1 * 65536 < got['strip']['threshold'] < 0.4 * 65536
                assert got['lines'][2]['threshold'] is None and got['lines'][2]['separation'] < 0.01
            if kind == 'sparse':
                g = got['lines'][1]                                       # an empty line: nothing divides by zero
                assert (g['inner_returns'], g['outer_returns'], g['separation'], g['supported'], g['threshold']) == (0, 0, 0.0, False, None)
                assert g['paint_share'] is None and g['inner_mean'] is None and g['plateau'] == [1 << bin_shift, (t.n_counts - 1) << bin_shift]


def test_hand_made_group():
    """Two counts by hand, bin_shift 8 (NB = 256): 1000 inner returns in bin 100 and 1000 in bin 20, 2000 outer returns in bin 20.
    a(T) = 2000, 1000, 0 and o(T) = 2000, 0, 0 for T <= 20, 21 .. 100, > 100: J = 0, 2 000 000, 0.  M = 2e6 on 21 .. 100, the floor M - M/32
    keeps exactly that run, T* = 60, threshold 60 x 256 = 15360, D = 0.5, paint share 0.5, false share 0."""
    t = PaintThreshold(bin_shift=8)
    hist = np.zeros((1, t.rings, 256), np.int64)
    hist[0, 0, 100], hist[0, 1, 20], hist[0, 7, 20] = 1000, 1000, 2000
    hist[0, 3, 200] = 5000                                              # a ring that is neither inner nor outer: ignored
    g = las_io.paint_threshold(hist, t)['strip']
    assert g == {'threshold': 15360.0, 'supported': True, 'separation': 0.5, 'inner_returns': 2000, 'outer_returns': 2000, 'paint_share': 0.5,
                 'false_share': 0.0, 'inner_mean': 60 * 256 + 127.5, 'outer_mean': 20 * 256 + 127.5, 'plateau': [21 * 256, 100 * 256]}
    tr.same_group(g, tr.policy(hist, bin_shift=8)['strip'])
    few = las_io.paint_threshold(hist, PaintThreshold(bin_shift=8, min_returns=2001))['strip']
    assert few['threshold'] is None and not few['supported'] and few['separation'] == 0.5
    with pytest.raises(ValueError, match='hist must be'):
        las_io.paint_threshold(hist[:, :-1], t)
    with pytest.raises(ValueError, match='hist must be'):
        las_io.paint_threshold(hist.astype(np.int32), t)
    with pytest.raises(TypeError, match='PaintThreshold'):
        las_io.paint_threshold(hist, MarkingSurvey())


def _planted(paint, noise, seed, n=120000, off=0.0):
    """The planted scene: n returns uniform over the band of one line (|o| <= 0.625 m) and over 30 m of station; asphalt U(800, 9000)
    everywhere, paint U(15000, 33000) within 0.075 m of a stripe `off` beside the line - 'solid': all along, 'dashed': on one metre of
    three, None: nowhere - and a share `noise` of the returns U(0, 65535) instead.  -> hist [1, 11, 1024] under the defaults."""
    rng = np.random.RandomState(seed)
    o, st = rng.uniform(-0.625, 0.625, n), rng.uniform(0.0, 30.0, n)
    inten = rng.uniform(800.0, 9000.0, n)
    on = np.abs(o - off) < 0.075
    if paint == 'dashed':
        on &= (st % 3.0) < 1.0
    if paint is None:
        on[:] = False
    inten[on] = rng.uniform(15000.0, 33000.0, int(on.sum()))
    stray = rng.rand(n) < noise
    inten[stray] = rng.uniform(0.0, 65535.0, int(stray.sum()))
    q = np.rint(o.astype(np.float32) * np.float32(1024)).astype(np.int64)
    iq = np.clip(np.rint(inten.astype(np.float32)), 0, 65535).astype(np.int64)
    hist = np.zeros((1, 11, 1024), np.int64)
    np.add.at(hist[0], (np.minimum(np.abs(q), 640) // 64, iq >> 6), 1)
    return hist


@pytest.mark.parametrize('noise', [0.0, 0.02, 0.05])
@pytest.mark.parametrize('paint, off, d_min', [('solid', 0.0, 0.5), ('dashed', 0.0, 0.15), ('solid', 0.08, 0.35)])
def test_planted_paint_is_found_by_the_reference_alone(paint, off, d_min, noise):
    hist = _planted(paint, noise, seed=int(1000 * noise) + len(paint), off=off)
    want = tr.policy(hist)
    g = want['strip']
    print(f'{paint}, off {off}, noise {noise}: threshold {g["threshold"]}, D {g["separation"]:.4f}, plateau {g["plateau"]}, '
          f'NA {g["inner_returns"]}, NO {g["outer_returns"]}')
    assert g['supported'] and 9000 < g['threshold'] <= 15000 and g['separation'] > d_min
    tr.same_policy(las_io.paint_threshold(hist, PaintThreshold()), want)


@pytest.mark.parametrize('noise', [0.0, 0.02])
def test_a_planted_road_without_paint_has_no_threshold(noise):
    hist = _planted(None, noise, seed=5 + int(100 * noise))
    want = tr.policy(hist)
    g = want['strip']
    print(f'no paint, noise {noise}: D {g["separation"]:.5f}, NA {g["inner_returns"]}, NO {g["outer_returns"]}')
    assert g['threshold'] is None and not g['supported'] and g['inner_returns'] > 10000 and g['outer_returns'] > 10000
    tr.same_policy(las_io.paint_threshold(hist, PaintThreshold()), want)


# ------------------------------------------------------------------------------------------------ 'auto'
def test_auto_is_accepted_by_the_four_classes_and_nothing_else_is():
    assert MarkingLabels(min_intensity='auto').min_intensity == 'auto' == las_io.AUTO
    assert MarkingSurvey(min_intensity='auto').min_intensity == 'auto'
    assert PaintResidue('auto').min_intensity == 'auto' and PaintResidue(min_intensity='auto', clear=0.4).clear == 0.4
    assert CrossSection('auto').paint_intensity == 'auto' and CrossSection(paint_intensity='auto').lateral_q == 32
    for make in (lambda v: MarkingLabels(min_intensity=v), lambda v: MarkingSurvey(min_intensity=v), PaintResidue, CrossSection):
        for bad in ('x', 'Auto', '', 'auto ', b'auto'):
            with pytest.raises(ValueError, match='intensity'):
                make(bad)
    assert MarkingSurvey(min_intensity='auto')._replace(min_intensity=12096.0) == MarkingSurvey(min_intensity=12096.0)
    assert CrossSection('auto', bin=0.25)._replace(paint_intensity=12096.0) == CrossSection(12096.0, bin=0.25)
    assert PaintResidue('auto', reach=5.0)._replace(min_intensity=1.0) == PaintResidue(1.0, reach=5.0)
    assert MarkingLabels(min_intensity='auto', line_ids=False)._replace(min_intensity=2.0) == MarkingLabels(min_intensity=2.0, line_ids=False)
    with pytest.raises(ValueError, match='paint_threshold'):
        CrossSection('auto').paint_iq


def test_an_unresolved_auto_is_refused_by_the_low_level_functions():
    files = [('none.las', None, None)]
    with pytest.raises(ValueError, match='paint_threshold'):
        las_io.survey_files(files, [], MarkingSurvey(min_intensity='auto'))
    with pytest.raises(ValueError, match='paint_threshold'):
        las_io.survey_colour_files(files, [], MarkingSurvey(min_intensity='auto'), las_io.MarkingColour())
    with pytest.raises(ValueError, match='paint_threshold'):
        las_io.cross_files(files, [], CrossSection('auto'))
    with pytest.raises(ValueError, match='paint_threshold'):
        las_io.residue_files(files, [], PaintResidue('auto'))
    with pytest.raises(ValueError, match='paint_threshold'):
        las_io.label_las('none.las', 'out.las', [], MarkingLabels(min_intensity='auto'), None)
    with pytest.raises(TypeError, match='PaintThreshold'):
        las_io.hist_files(files, [], MarkingSurvey())


def test_runner_takes_threshold_from_the_argument_the_cfg_or_an_auto_stage():
    from lanemapping_amd.config import Config
    from lanemapping_amd.runner import Runner
    r = Runner.__new__(Runner)
    r.cfg = Config({'list_img_size_xy': [1152, 1152]})
    none = {'label': None, 'survey': None, 'cross': None, 'residue': None}
    assert r._las_threshold(None, none) is None
    assert r._las_threshold(None, {**none, 'survey': MarkingSurvey(min_intensity=5.0), 'cross': CrossSection(5.0)}) is None
    for key, stage in (('label', MarkingLabels(min_intensity='auto')), ('survey', MarkingSurvey(min_intensity='auto')),
                       ('cross', CrossSection('auto')), ('residue', PaintResidue('auto'))):
        assert r._las_threshold(None, {**none, key: stage}) == PaintThreshold()
        assert r._las_threshold(PaintThreshold(bin_shift=4), {**none, key: stage}) == PaintThreshold(bin_shift=4)
    assert r._las_threshold(PaintThreshold(ring=0.125), none) == PaintThreshold(ring=0.125)
    with pytest.raises(TypeError, match='threshold must be a las_io.PaintThreshold'):
        r.infer_las_strip_to_map('none.las', [], threshold={'bin_shift': 4})
    with pytest.raises(TypeError, match='threshold must be a las_io.PaintThreshold'):
        r.infer_las_to_map([], threshold=12000.0)
    r.cfg = Config({'list_img_size_xy': [1152, 1152], 'las_threshold': {'bin_shift': 4, 'min_returns': 10}})
    assert r._las_threshold(None, none) == PaintThreshold(bin_shift=4, min_returns=10)
    r.cfg = Config({'list_img_size_xy': [1152, 1152], 'las_threshold': {'bin_shift': 9}})
    with pytest.raises(ValueError, match='bin_shift'):
        r.infer_las_to_map([])


# ------------------------------------------------------------------------------------------------ header, build, binding
def test_the_entries_are_declared_bound_and_described():
    from lanemapping_amd._lib import SIGNATURES
    from lds_state import stream_entries
    from test_lds_inventory_cpu import lds_kernels
    header = open(os.path.join(ROOT, 'include', 'lanemap_hip.h')).read()
    for name, n in (('lm_line_hist_points', 17), ('lm_las_line_hist_records', 23)):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
        assert m, name
        params = [re.sub(r'\s+', ' ', p.strip()) for p in m.group(1).split(',')]
        assert params[-1] == 'void* hip_stream' and params[-3:-1] == ['long* hist', 'long n_hist'] and len(params) == len(SIGNATURES[name][1]) == n
        assert name not in stream_entries(), 'the stream comes last: the inventories of the older entries do not list these two'
    block = header[header.index('/* ---- the paint / asphalt histograms'):header.index('int lm_line_hist_points(')]
    for words in ('hist_cell', 'tests/threshold_ref.py', 'WITHOUT a min_intensity', 'only rlen is read', 'hq / ring_q + 1', 'min(|q|, hq) / ring_q',
                  '65536 >> bin_shift', 'iq >> bin_shift', 'hist[((k-1) Z + r) NB + ib] += 1', 'line_hist_points', 'las_line_hist_records',
                  'half_width > 16', 'z_tol > 16', 'ring_q < 1', 'bin_shift outside 0 .. 8', 'L Z NB > 2^27', 'n_hist != L Z NB',
                  'accumulate outside 0, 1', 'a null hist', 'hist is not 8-byte aligned', 'LAST parameter', 'no __shared__', 'las_profile_kernel'):
        assert words in re.sub(r'\s*\n \*\s*', ' ', block), words
    src = open(os.path.join(ROOT, 'lanemapping_amd', 'csrc', 'profile.hip')).read()
    assert 'hist_points_kernel' not in lds_kernels(src) and 'las_profile_kernel' in lds_kernels(src)
    assert 'las_profile_records<false, false, true>' in src and 'hipMemsetAsync' not in src and not re.search(r'^\s*#\s*if', src, re.M)
    entry = src[src.index('LM_API int lm_line_hist_points('):]
    assert 'lm_zero_async(' in entry and not re.search(r'hip(Stream|Device)Synchronize|hipMemcpy', entry)
