"""CPU: the host side of the marking colours (las_io.rgb_offset, las_io.MarkingColour, las_io.marking_colours, the brute force of
tests/colour_ref.py) and the argument checks of the Runner entries that need no device."""
import numpy as np
import pytest

import colour_ref as cr
import profile_ref as pr
from lanemapping_amd import las_io
from lanemapping_amd.las_io import MarkingColour, MarkingSurvey


# ------------------------------------------------------------------------------------------------ rgb_offset
def test_rgb_offset_of_every_format():
    assert [las_io.rgb_offset(f) for f in range(11)] == [None, None, 20, 28, None, 28, None, 30, 30, None, 30]
    assert {f: las_io.rgb_offset(f) for f in cr.COLOUR_FORMATS} == cr.RGB_OFFSET
    for f, o in cr.RGB_OFFSET.items():
        assert o + 6 <= cr.MIN_LEN[f], 'the triple lies inside the shortest record of its format'
    assert las_io.rgb_offset(np.int64(7)) == 30
    for bad in (-1, 11, 2.0, '2', None, True):
        with pytest.raises(ValueError, match='point data record format'):
            las_io.rgb_offset(bad)


# ------------------------------------------------------------------------------------------------ MarkingColour
def test_marking_colour_is_validated_and_immutable():
    c = MarkingColour()
    assert (c.yellow_ratio, c.yellow_share, c.min_coloured) == (0.75, 0.5, 10) and c.blue_q == 768
    assert repr(c) == 'MarkingColour(yellow_ratio=0.75, yellow_share=0.5, min_coloured=10)'
    assert c == MarkingColour(0.75, 0.5, 10) and hash(c) == hash(MarkingColour()) and c != MarkingColour(min_coloured=11)
    assert 'plain defaults, not tuned values' in MarkingColour.__doc__
    with pytest.raises(AttributeError, match='immutable'):
        c.yellow_ratio = 0.5
    with pytest.raises(AttributeError, match='immutable'):
        del c.min_coloured
    with pytest.raises(AttributeError):
        c.other = 1
    for ratio, q in ((1.0, 1024), (1, 1024), (0.5, 512), (1 / 1024, 1), (1e-9, 1), (1.5 / 1024, 2), (1.4999 / 1024, 1), (0.9999, 1024),
                     (np.float32(0.25), 256)):
        assert MarkingColour(yellow_ratio=ratio).blue_q == q == cr.blue_q_of(float(ratio)), ratio
    for bad in (0, 0.0, -0.5, 1.0001, float('nan'), float('inf'), True, '0.75', None):
        with pytest.raises(ValueError, match='yellow_ratio'):
            MarkingColour(yellow_ratio=bad)
        with pytest.raises(ValueError, match='yellow_share'):
            MarkingColour(yellow_share=bad)
    for bad in (0, -1, 1.0, 2.5, True, '3', None):
        with pytest.raises(ValueError, match='min_coloured'):
            MarkingColour(min_coloured=bad)
    assert MarkingColour(yellow_share=1, min_coloured=np.int32(1)).min_coloured == 1
    # a new class: the survey keeps its slots and its repr
    assert MarkingSurvey.__slots__ == ('bin', 'half_width', 'z_tol', 'min_intensity', 'min_points', 'max_gap', 'solid_cover')
    assert repr(MarkingSurvey()) == ('MarkingSurvey(bin=0.25, half_width=0.3, z_tol=0.5, min_intensity=None, min_points=3, max_gap=0.5, '
                                     'solid_cover=0.8)')


# ------------------------------------------------------------------------------------------------ the brute force
def test_brute_force_on_the_worked_example():
    """The four returns of colour_ref's docstring, worked by hand there."""
    B, rgb, blue_q, n_bins, want = cr.worked_example()
    black, col, yellow = cr.votes(rgb, blue_q)
    assert black.tolist() == [False, False, True, False] and col.tolist() == [True, True, False, True]
    assert yellow.tolist() == [True, False, False, True]
    assert 2048 * 30000 == 768 * 80000, 'return b sits exactly on the border'
    got = cr.accumulate(B, rgb, blue_q, n_bins)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    # a return without a bin adds nothing; adding to a table adds; the order changes nothing
    assert np.array_equal(cr.accumulate(np.array([-1, 0, -1, 2]), rgb, blue_q, n_bins)[:, 0], [1, 0, 1])
    assert np.array_equal(cr.accumulate(B[2:], rgb[2:], blue_q, n_bins, colours=cr.accumulate(B[:2], rgb[:2], blue_q, n_bins)), want)
    assert np.array_equal(cr.accumulate(B[::-1], rgb[::-1], blue_q, n_bins), want)
    # blue_q at its ends: 1 makes almost nothing yellow, 1024 everything whose blue is below the mean of red and green
    assert cr.votes(rgb, 1)[2].tolist() == [False] * 4 and cr.votes(rgb, 1024)[2].tolist() == [True, True, False, True]
    assert cr.votes([[65535, 65535, 63], [65535, 65535, 64]], 1)[2].tolist() == [True, False]        # 2048 * 64 > 131070 > 2048 * 63
    assert cr.votes([[100, 100, 99], [100, 100, 100]], 1024)[2].tolist() == [True, False]
    # the helper that writes the triples: every colour format at its minimum length and padded, byte by byte
    for fmt in cr.COLOUR_FORMATS:
        for extra in (0, 3):
            rec = np.full((4, cr.MIN_LEN[fmt] + extra), 0xEE, np.uint8)
            cr.put_rgb(rec, fmt, rgb)
            o = cr.RGB_OFFSET[fmt]
            assert rec[0, o:o + 6].tolist() == [0x60, 0xEA, 0x50, 0xC3, 0x10, 0x27]                  # 60000, 50000, 10000 little-endian
            assert (rec[:, :o] == 0xEE).all() and (rec[:, o + 6:] == 0xEE).all() and np.array_equal(cr.get_rgb(rec, fmt), rgb)


# ------------------------------------------------------------------------------------------------ marking_colours
def _tables(n_per_bin, rows):
    """bins and colours of one line: bin i holds n_per_bin[i] returns; rows[i] = (n_c, n_yellow, n_black) with R = G = 200, B = 100."""
    bins = np.zeros((len(n_per_bin), 6), np.int64)
    bins[:, 0], bins[:, 4], bins[:, 5] = n_per_bin, pr.Q_EMPTY_MIN, pr.Q_EMPTY_MAX
    col = np.array([[c, 200 * c, 200 * c, 100 * c, y, k] for c, y, k in rows], np.int64).reshape(len(rows), 6)
    return bins, col


def _check(bins, col, bs, survey, colour):
    got = las_io.marking_colours(bins, col, bs, survey, colour)
    assert got == cr.colours_of(bins, col, bs, survey.bin, survey.min_points, survey.max_gap, colour.yellow_share, colour.min_coloured)
    return got


def test_marking_colours_decides_exactly_at_the_share():
    survey = MarkingSurvey(min_points=3)
    # shares that are binary fractions: yellow == share * coloured exactly is yellow, one vote less is white
    for share, n_c, n_y in ((0.5, 10, 5), (1.0, 10, 10), (0.125, 4096, 512)):
        colour = MarkingColour(yellow_share=share, min_coloured=10)
        for y, want in ((n_y, 'yellow'), (n_y - 1, 'white')):
            bins, col = _tables([n_c], [(n_c, y, 0)])
            got = _check(bins, col, [0, 1], survey, colour)[0]
            assert got['colour'] == want and got['run_colours'] == [want], (share, y)
    # a share that is none: the float's own value decides, as a rational, never a rounded product.  The double 0.3 lies below 3 / 10, so
    # 3 of 10 is yellow; the double 0.7 lies below 7 / 10 too; the double 0.1 lies above 1 / 10, so 100 of 1000 is white and 101 yellow
    from fractions import Fraction
    assert Fraction(0.3) < Fraction(3, 10) and Fraction(0.7) < Fraction(7, 10) and Fraction(0.1) > Fraction(1, 10)
    for share, n_c, y, want in ((0.3, 10, 3, 'yellow'), (0.3, 10, 2, 'white'), (0.7, 10, 7, 'yellow'), (0.7, 10, 6, 'white'),
                                (0.1, 1000, 100, 'white'), (0.1, 1000, 101, 'yellow')):
        bins, col = _tables([n_c], [(n_c, y, 0)])
        assert _check(bins, col, [0, 1], survey, MarkingColour(yellow_share=share))[0]['colour'] == want, (share, y)
    # yellow == share * coloured exactly, and one below, with a share that is a binary fraction
    colour = MarkingColour(yellow_share=0.25, min_coloured=1)
    bins, col = _tables([8, 8], [(4, 1, 4), (4, 1, 4)])
    got = _check(bins, col, [0, 2], survey, colour)[0]
    assert got == {'coloured': 8, 'yellow': 2, 'black': 8, 'rgb': [200.0, 200.0, 100.0], 'colour': 'yellow', 'run_colours': ['yellow']}
    bins, col = _tables([8, 8], [(4, 1, 4), (4, 0, 4)])
    assert _check(bins, col, [0, 2], survey, colour)[0]['colour'] == 'white'


def test_marking_colours_min_coloured_painted_bins_and_empty_lines():
    survey = MarkingSurvey(min_points=3)
    # min_coloured at its edge: 10 coloured returns decide, 9 do not - however many are black
    for n_c, want in ((10, 'yellow'), (9, 'unknown')):
        bins, col = _tables([40], [(n_c, n_c, 40 - n_c)])
        got = _check(bins, col, [0, 1], survey, MarkingColour())[0]
        assert got['colour'] == want and got['black'] == 40 - n_c and got['run_colours'] == [want]
    # only painted bins count: the second bin holds 2 returns < min_points and its yellow votes are not read
    bins, col = _tables([12, 2], [(12, 0, 0), (2, 2, 0)])
    got = _check(bins, col, [0, 2], survey, MarkingColour(min_coloured=1))[0]
    assert (got['coloured'], got['yellow'], got['colour']) == (12, 0, 'white')
    # nothing coloured: rgb None, unknown; a line without bins; a line with bins and no paint
    bins, col = _tables([5, 0], [(0, 0, 5), (0, 0, 0)])
    got = _check(bins, col, [0, 0, 1, 2], survey, MarkingColour())
    assert got[0] == {'coloured': 0, 'yellow': 0, 'black': 0, 'rgb': None, 'colour': 'unknown', 'run_colours': []}
    assert got[1] == {'coloured': 0, 'yellow': 0, 'black': 5, 'rgb': None, 'colour': 'unknown', 'run_colours': ['unknown']}
    assert got[2] == got[0]
    assert las_io.marking_colours(np.zeros((0, 6), np.int64), np.zeros((0, 6), np.int64), [0], survey, MarkingColour()) == []
    # rgb is the raw mean, not rescaled
    bins, col = _tables([4], [(3, 0, 1)])
    col[0, 1:4] = [3 * 255, 3 * 254, 100]
    assert _check(bins, col, [0, 1], survey, MarkingColour(min_coloured=1))[0]['rgb'] == [255.0, 254.0, 100 / 3]


def test_run_colours_follow_the_runs_of_marking_summary():
    """Twelve bins of 0.25 m: paint in 0-1, 3-4 (a hole of one bin: joined at max_gap 0.5), 8-9 and 11 (a hole of one bin again); white
    first, yellow after the long gap.  A hole of three bins (5-7) is not joined."""
    survey = MarkingSurvey(bin=0.25, min_points=3, max_gap=0.5)
    colour = MarkingColour(min_coloured=5)
    n = [6, 6, 0, 6, 6, 0, 1, 0, 6, 6, 2, 6]
    rows = [(6, 0, 0), (6, 1, 0), (0, 0, 0), (6, 0, 0), (6, 0, 0), (0, 0, 0), (1, 1, 0), (0, 0, 0), (6, 6, 0), (6, 5, 0), (2, 0, 0), (6, 6, 0)]
    bins, col = _tables(n, rows)
    got = _check(bins, col, [0, 12], survey, colour)[0]
    summary = las_io.marking_summary(bins, [0, 12], survey)[0]
    assert summary['runs'] == [[0.0, 1.25], [2.0, 3.0]] and len(got['run_colours']) == len(summary['runs'])
    assert got['run_colours'] == ['white', 'yellow'] and (got['coloured'], got['yellow']) == (42, 18) and got['colour'] == 'white'
    # without joining: four runs, the last of one bin with 6 coloured returns
    tight = MarkingSurvey(bin=0.25, min_points=3, max_gap=0.0)
    got = _check(bins, col, [0, 12], tight, colour)[0]
    assert len(las_io.marking_summary(bins, [0, 12], tight)[0]['runs']) == 4 and got['run_colours'] == ['white', 'white', 'yellow', 'yellow']
    # a run below min_coloured is unknown while its line is decided
    got = _check(bins, col, [0, 12], tight, MarkingColour(min_coloured=7))[0]
    assert got['run_colours'] == ['white', 'white', 'yellow', 'unknown'] and got['colour'] == 'white'


def test_marking_colours_refuses_wrong_shapes_and_types():
    survey, colour = MarkingSurvey(), MarkingColour()
    bins, col = _tables([4, 4], [(4, 0, 0), (4, 0, 0)])
    for b, c, bs, what in ((bins[:, :5], col, [0, 2], 'bins must be'), (bins.astype(np.int32), col, [0, 2], 'bins must be'),
                           (bins, col, [0, 3], 'bins must be'), (bins, col, [1, 2], 'bins must be'), (bins, col, [0, 2, 1], 'bins must be'),
                           (bins, col[:1], [0, 2], 'colours must be'), (bins, col.astype(np.float64), [0, 2], 'colours must be'),
                           (bins, col[:, :5], [0, 2], 'colours must be')):
        with pytest.raises(ValueError, match=what):
            las_io.marking_colours(b, c, bs, survey, colour)
    with pytest.raises(TypeError, match='MarkingSurvey'):
        las_io.marking_colours(bins, col, [0, 2], colour, colour)
    with pytest.raises(TypeError, match='MarkingColour'):
        las_io.marking_colours(bins, col, [0, 2], survey, {'yellow_ratio': 0.75})
    with pytest.raises(TypeError, match='MarkingColour'):
        las_io.survey_colour_las(['none.las'], [], survey, survey, None)
    with pytest.raises(TypeError, match='MarkingSurvey'):
        las_io.survey_colour_las(['none.las'], [], None, colour, None)


# ------------------------------------------------------------------------------------------------ the Runner entries
def test_runner_entries_refuse_colour_without_survey_without_a_device(tmp_path):
    from lanemapping_amd.config import Config
    from lanemapping_amd.runner import Runner
    r = Runner.__new__(Runner)
    r.cfg = Config({'list_img_size_xy': [1152, 1152]})
    with pytest.raises(ValueError, match='colour: .* pass survey='):
        r.infer_las_to_map([], colour=MarkingColour(), work_dirs=str(tmp_path / 'a'))
    with pytest.raises(ValueError, match='colour: .* pass survey='):
        r.infer_las_strip_to_map('none.las', [], colour=MarkingColour(), work_dirs=str(tmp_path / 'b'))
    with pytest.raises(TypeError, match='colour must be a las_io.MarkingColour'):
        r.infer_las_to_map([], survey=MarkingSurvey(), colour={'yellow_ratio': 0.5})
    r.cfg = Config({'list_img_size_xy': [1152, 1152], 'las_colour': {'yellow_share': 2.0}})
    with pytest.raises(ValueError, match='yellow_share'):
        r.infer_las_to_map([])
    r.cfg = Config({'list_img_size_xy': [1152, 1152], 'las_colour': {'yellow_ratio': 0.5}})
    with pytest.raises(ValueError, match='pass survey='):
        r.infer_las_strip_to_map('none.las', [])
    assert not (tmp_path / 'a').exists() and not (tmp_path / 'b').exists()
    # a header of a format without colour is refused by name, a coloured one passes, what is no LAS file is left to the reader
    for fmt, ok in ((1, False), (6, False), (2, True), (7, True)):
        path = tmp_path / f'f{fmt}.las'
        head = bytearray(375)
        head[:4], head[104] = b'LASF', fmt
        path.write_bytes(bytes(head))
        if ok:
            assert las_io.require_colour(str(path)) == fmt
        else:
            with pytest.raises(ValueError, match=f'f{fmt}.las is of point format {fmt}, which carries no RGB'):
                las_io.require_colour(str(path))
    (tmp_path / 'junk.las').write_bytes(b'no las')
    assert las_io.require_colour(str(tmp_path / 'junk.las')) is None
