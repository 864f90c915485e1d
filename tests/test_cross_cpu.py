"""CPU: the host policy of the cross-sections (las_io.CrossSection, cross_summary, snap_lines) on handmade tables, each case against exact
expected values and against the independent restatement in tests/cross_ref.py.  No GPU.

The tables use the defaults: half_width 0.625 m -> hq = 640, lateral 0.03125 m -> lateral_q = 32, nl = 41 cells; cell c covers
[(32 c - 640) / 1024, (32 c - 608) / 1024) m, so cell 20 starts on the line and every edge is a multiple of 1/32 m, exact in float64."""
import numpy as np
import pytest

import cross_ref as cr
from lanemapping_amd import las_io
from lanemapping_amd.las_io import CrossSection

CROSS = CrossSection(paint_intensity=10000)
NL = 41
ASPHALT, PAINT, UNKNOWN = (5, 0, 5 * 3000, 0), (5, 5, 5 * 24000, 0), (1, 1, 24000, 0)


def _station(painted=(), unknown=(), other=None):
    row = np.array([ASPHALT] * NL, np.int64)
    for c in painted:
        row[c] = PAINT
    for c in unknown:
        row[c] = UNKNOWN
    for c, v in (other or {}).items():
        row[c] = v
    return row


def _summary(stations, bin_start=None, cross=CROSS):
    cells = np.stack(stations)
    bs = np.array([0, len(cells)] if bin_start is None else bin_start, np.int32)
    got = las_io.cross_summary(cells, bs, cross)
    assert got == cr.summary_of(cells, bs, cross)
    return got


def test_the_geometry_of_the_defaults():
    assert (CROSS.hq, CROSS.lateral_q, CROSS.nl, CROSS.paint_iq) == (640, 32, NL, 10000) == (*cr.hq_nl(0.625, 32)[:1], 32, cr.hq_nl(0.625, 32)[1], 10000)
    assert CrossSection(10000, half_width=0.03, lateral=1 / 1024).nl == 63 and CrossSection(10000, half_width=0.03, lateral=1 / 1024).hq == 31
    assert CrossSection(10000, lateral=2.0).nl == 1 and CrossSection(10000, lateral=1e-9).lateral_q == 1
    assert CrossSection(0.5).paint_iq == 1 and CrossSection(-3).paint_iq == 0 and CrossSection(65535).paint_iq == 65535
    assert CrossSection(65535.5).paint_iq == 65536 and CrossSection(float('inf')).paint_iq == 65536 and CrossSection(9999.2).paint_iq == 10000


def test_a_single_stripe():
    m, = _summary([_station(range(18, 23))] * 4)
    assert m['stations'] == 4 and m['stripes'] == 1 and m['double'] is False and m['separation'] is None
    assert m['width'] == 0.15625 == m['extent'] and m['offset'] == 0.015625 and m['centres'] == [0.015625] * 4 and m['counts'] == [1] * 4
    assert m['crossfall'] == 0.0


def test_a_double_line_with_a_one_cell_hole():
    m, = _summary([_station([10, 11, 13, 14] + list(range(20, 25)), unknown=[12])] * 3)
    assert m['stripes'] == 2 and m['double'] is True and m['stations'] == 3
    assert m['width'] == 0.15625 and m['separation'] == 0.15625 and m['extent'] == 15 * 32 / 1024
    assert m['offset'] == 0.5 * ((10 * 32 - 640) + (25 * 32 - 640)) / 1024 == -0.078125
    # the same hole with max_hole = 0: three stripes, two of them 0.0625 wide
    m0, = _summary([_station([10, 11, 13, 14] + list(range(20, 25)), unknown=[12])] * 3, cross=CrossSection(10000, max_hole=0))
    assert m0['stripes'] == 3 and m0['double'] is False and m0['separation'] is None and m0['width'] == 0.0625


def test_a_stripe_narrower_than_min_stripe_is_none():
    m, = _summary([_station([20]), _station([20]), _station([19, 20])])
    assert 0.03125 < CROSS.min_stripe <= 0.0625
    assert m['stations'] == 1 and m['counts'] == [0, 0, 1] and m['centres'] == [None, None, 0.0] and m['width'] == 0.0625 and m['stripes'] == 1
    none, = _summary([_station([20])] * 2)
    assert none == {'stations': 0, 'stripes': None, 'double': False, 'width': None, 'separation': None, 'extent': None, 'offset': None,
                    'crossfall': 0.0, 'centres': [None, None], 'counts': [0, 0]}


def test_unknown_cells():
    # a hole of two unknown cells is not closed by max_hole = 1; a KNOWN cell that is not painted is never closed; an unknown cell at
    # the edge of a stripe does not widen it; a cell below paint_share is asphalt, one exactly on it is paint
    two, = _summary([_station([10, 11, 14, 15], unknown=[12, 13])])
    assert two['counts'] == [2] and two['width'] == 0.0625 and two['separation'] == 0.0625
    known, = _summary([_station([10, 11, 13, 14])])
    assert known['counts'] == [2] and known['separation'] == 0.03125
    edge, = _summary([_station([10, 11], unknown=[9, 12])])
    assert edge['counts'] == [1] and edge['width'] == 0.0625
    share, = _summary([_station([10, 11], other={12: (4, 2, 0, 0), 13: (5, 2, 0, 0)})])
    assert share['counts'] == [1] and share['width'] == 3 * 32 / 1024
    # below min_points everywhere: nothing is known, no stripe and no cross-fall
    dark, = _summary([np.array([UNKNOWN] * NL, np.int64)])
    assert dark['stations'] == 0 and dark['crossfall'] is None and dark['stripes'] is None
    # an empty line and a line without bins
    empty = _summary([_station([20, 21])], bin_start=[0, 0, 1, 1])
    assert [m['stations'] for m in empty] == [0, 1, 0] and empty[0]['centres'] == [] and empty[2]['stripes'] is None


def test_ties_in_the_stripe_count_go_to_the_smaller():
    one, two = _station(range(18, 23)), _station(list(range(10, 15)) + list(range(20, 25)))
    m, = _summary([two, one, two, one])
    assert m['stripes'] == 1 and m['double'] is False and m['stations'] == 4 and m['counts'] == [2, 1, 2, 1]
    assert m['width'] == 0.15625 and m['offset'] == 0.015625 and m['separation'] is None     # read off the single-stripe stations alone
    m, = _summary([two, one, two, one, two])
    assert m['stripes'] == 2 and m['double'] is True and m['offset'] == -0.078125 and m['separation'] == 0.15625


def test_an_exact_crossfall():
    """The cell centres lie at (2 c - 39) / 64 m; with n = 5 and sum zq = 2 (2 c - 39) the mean height is 0.4 (2 c - 39) / 1024 m =
    0.025 x exactly, so the least-squares slope is the fraction 1/40 whatever the weights."""
    row = np.array([(5, 0, 0, 2 * (2 * c - 39)) for c in range(NL)], np.int64)
    m, = _summary([row])
    assert m['crossfall'] == 0.025 and m['stations'] == 0
    uneven = row.copy()
    uneven[:, 0] *= np.arange(1, NL + 1)
    uneven[:, 3] *= np.arange(1, NL + 1)
    uneven[3] = (2, 0, 0, 999)                                # unknown: left out
    m, = _summary([uneven, row, -row * np.array([-1, 1, 1, 1])])
    assert m['crossfall'] == 0.025                            # the median of 0.025, 0.025, -0.025
    # two known cells are no fit; three are
    few = np.zeros((NL, 4), np.int64)
    few[[5, 30]] = [(5, 0, 0, 0), (5, 0, 0, 512)]
    assert _summary([few])[0]['crossfall'] is None
    few[35] = (5, 0, 0, 0)
    assert _summary([few])[0]['crossfall'] is not None


def test_snap_lines_on_a_bent_polyline():
    """A line east for 4 m, a doubled vertex, then north for 4 m: 16 bins of 0.5 m.  The paint is 0.0625 m left of it everywhere, except
    one station that says 0.25 (an outlier the median ignores) and the last two, which say 0.5 (beyond max_shift: the vertex stays)."""
    line = np.array([[100.0, 200.0, 5.0], [102.0, 200.0, 5.5], [104.0, 200.0, 6.0], [104.0, 200.0, 6.0], [104.0, 202.0, 6.5], [104.0, 204.0, 7.0]])
    bs = np.array([0, 16, 16], np.int32)
    centres = [0.0625] * 16
    centres[4] = 0.25
    centres[14] = centres[15] = 0.5
    summ = [{'stripes': 1, 'centres': centres, 'counts': [1] * 16}, {'stripes': None, 'centres': [], 'counts': []}]
    lone = np.array([[1.0, 2.0, 3.0]])
    got = las_io.snap_lines([line, lone], summ, bs, CROSS)
    want = cr.snap_of([line, lone], summ, bs, CROSS)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and got[0].shape == line.shape and np.array_equal(got[1], lone)
    r = 0.0625 * np.sqrt(0.5)
    expect = line.copy()
    expect[0, 1] += 0.0625                                    # one segment: its own normal, north
    expect[1, 1] += 0.0625                                    # (the outlier at station 2.25 m is within 1 m: the median of four)
    expect[2, :2] += [-r, r]                                  # the corner, both of them: the mean of north and west, past the doubled vertex
    expect[3, :2] += [-r, r]
    expect[4, 0] -= 0.0625
    assert np.array_equal(got[0][:, 2], line[:, 2])
    assert np.allclose(got[0][:5], expect[:5], rtol=0, atol=1e-15) and np.array_equal(got[0][[0, 1, 4]], expect[[0, 1, 4]])
    assert np.array_equal(got[0][5], line[5])                 # stations 7.25 and 7.75 say 0.5: beyond max_shift, the vertex stays
    # too few stations: nothing moves; a stripe count that is not the line's does not qualify
    alone = las_io.snap_lines([line, lone], summ, bs, CrossSection(10000, min_stations=5))
    assert np.array_equal(alone[0], line)
    summ[0]['counts'] = [2] * 16
    assert np.array_equal(las_io.snap_lines([line, lone], summ, bs, CROSS)[0], line)
    with pytest.raises(ValueError, match='do not belong together'):
        las_io.snap_lines([line], summ, bs, CROSS)


def test_cross_section_refuses_bad_arguments():
    with pytest.raises(TypeError):
        CrossSection()
    for kw, bad in (('paint_intensity', [None, 'x', float('nan'), True]), ('bin', [0, -1.0, float('inf'), None]),
                    ('half_width', [-0.1, 16.5, float('nan')]), ('lateral', [0, -1, float('inf')]), ('z_tol', [-1, 17, float('inf'), float('nan')]),
                    ('min_points', [0, 2.5, True]), ('paint_share', [0, 1.5, -0.1]), ('max_hole', [-1, 0.5]), ('min_stripe', [-0.1, float('inf')]),
                    ('smooth', [-1, float('nan')]), ('min_stations', [0, 1.5]), ('max_shift', [-0.1, float('inf')])):
        for v in bad:
            args = {'paint_intensity': 10000, kw: v}
            with pytest.raises(ValueError, match=f'CrossSection: {kw}='):
                CrossSection(**args)
    c = CrossSection(10000, bin=0.25)
    assert c == CrossSection(10000.0, bin=0.25) and hash(c) == hash(CrossSection(10000, bin=0.25)) and c != CROSS and 'bin=0.25' in repr(c)
    with pytest.raises(AttributeError):
        c.bin = 1.0
    with pytest.raises(TypeError, match='CrossSection'):
        las_io.cross_summary(np.zeros((0, NL, 4), np.int64), [0], las_io.MarkingSurvey())
    with pytest.raises(ValueError, match='cells must be'):
        las_io.cross_summary(np.zeros((1, NL + 1, 4), np.int64), [0, 1], CROSS)
