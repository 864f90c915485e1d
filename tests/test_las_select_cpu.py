"""CPU: the point filter of the LAS readers (las_io.PointFilter -> LmLasSelect -> lm_las_decode_select).  What needs no GPU: the
validation, the packing of the class set and flag mask, the refusals that come before the device, the promise that select=None makes
the call it made before the filter existed, and the header spelling the bounds inventory depends on."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import test_bounds_inventory_cpu as bounds_inventory
import test_entry_inventory_cpu as entry_inventory
from lanemapping_amd import las_io
from lanemapping_amd._lib import SIGNATURES, LanemapHipError, LmLasSelect, lib
from lanemapping_amd.las_io import PointFilter
from oracle import las_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ validation
@pytest.mark.parametrize('kwargs, field', [
    (dict(classes=[2, 256]), 'classes'),
    (dict(classes=[-1]), 'classes'),
    (dict(returns='second'), 'returns'),
    (dict(z_range=(1.0, 0.5)), 'z_range'),
    (dict(z_range=(math.nan, 1.0)), 'z_range'),
    (dict(z_range=(0.0, math.nan)), 'z_range'),
])
def test_point_filter_refusals_name_the_field(kwargs, field):
    with pytest.raises(ValueError, match=field):
        PointFilter(**kwargs)


def test_point_filter_defaults_and_immutability():
    f = PointFilter()
    assert (f.classes, f.drop_withheld, f.drop_synthetic, f.drop_keypoint, f.drop_overlap, f.returns, f.z_range) == \
        (None, True, False, False, False, 'all', None)
    with pytest.raises(AttributeError):
        f.returns = 'first'
    with pytest.raises(AttributeError):
        del f.classes
    with pytest.raises(AttributeError):
        f.extra = 1
    g = PointFilter(classes=[11, 2, 2], z_range=[-1, 2])
    assert g.classes == (2, 11) and g.z_range == (-1.0, 2.0)
    assert g == PointFilter(classes=(2, 11), z_range=(-1.0, 2.0)) and hash(g) == hash(PointFilter(classes=(2, 11), z_range=(-1.0, 2.0)))
    assert g != f and 'classes=(2, 11)' in repr(g)
    assert PointFilter(z_range=(0.25, 0.25)).z_range == (0.25, 0.25)       # one height is a window, not an empty one


# ------------------------------------------------------------------------------------------------ packing
def _bits(s):
    return {32 * w + b for w in range(8) for b in range(32) if s.class_mask[w] >> b & 1}


def test_struct_layout_is_the_header_s():
    text = open(os.path.join(ROOT, 'include', 'lanemap_hip.h')).read()
    assert 'typedef struct { unsigned class_mask[8]; unsigned drop_flags; int returns; float z_lo, z_hi; } LmLasSelect;' in text
    assert C.sizeof(LmLasSelect) == 48
    assert [(n, LmLasSelect.__dict__[n].offset) for n, _ in LmLasSelect._fields_] == \
        [('class_mask', 0), ('drop_flags', 32), ('returns', 36), ('z_lo', 40), ('z_hi', 44)]
    for name, value in (('LM_LAS_DROP_SYNTHETIC', las_io.DROP_SYNTHETIC), ('LM_LAS_DROP_KEYPOINT', las_io.DROP_KEYPOINT),
                        ('LM_LAS_DROP_WITHHELD', las_io.DROP_WITHHELD), ('LM_LAS_DROP_OVERLAP', las_io.DROP_OVERLAP),
                        ('LM_LAS_RETURNS_ALL', las_io.RETURNS['all']), ('LM_LAS_RETURNS_FIRST', las_io.RETURNS['first']),
                        ('LM_LAS_RETURNS_LAST', las_io.RETURNS['last']), ('LM_LAS_RETURNS_SINGLE', las_io.RETURNS['single'])):
        assert re.search(r'\b%s = %d\b' % (name, value), text), name


@pytest.mark.parametrize('classes', [[], [0], [2, 11], [31, 32], [7, 18, 64, 255], list(range(256))])
def test_class_mask_packing(classes):
    s = PointFilter(classes=classes).as_struct()
    assert isinstance(s, LmLasSelect) and _bits(s) == set(classes)


def test_struct_packing_of_flags_returns_and_window():
    s = PointFilter().as_struct()
    assert _bits(s) == set(range(256)) and s.drop_flags == 4 and s.returns == 0 and s.z_lo == -math.inf and s.z_hi == math.inf
    s = PointFilter(drop_withheld=False).as_struct()
    assert s.drop_flags == 0
    s = PointFilter(drop_withheld=False, drop_synthetic=True).as_struct()
    assert s.drop_flags == 1
    s = PointFilter(drop_withheld=False, drop_keypoint=True).as_struct()
    assert s.drop_flags == 2
    s = PointFilter(drop_withheld=False, drop_overlap=True).as_struct()
    assert s.drop_flags == 8
    s = PointFilter(drop_synthetic=True, drop_keypoint=True, drop_overlap=True, returns='last', z_range=(-0.5, 2.25)).as_struct()
    assert s.drop_flags == 15 and s.returns == 2 and (s.z_lo, s.z_hi) == (-0.5, 2.25)
    assert [PointFilter(returns=r).as_struct().returns for r in ('all', 'first', 'last', 'single')] == [0, 1, 2, 3]
    s = PointFilter(z_range=(-math.inf, 3.0)).as_struct()
    assert s.z_lo == -math.inf and s.z_hi == 3.0


def test_for_format_refuses_a_class_the_format_cannot_hold():
    f = PointFilter(classes=[2, 40])
    with pytest.raises(ValueError, match=r'classes \[40\].*point format 1'):
        f.for_format(1)
    assert f.for_format(6) is f and f.for_format(10) is f
    assert PointFilter(classes=[2, 31]).for_format(0).classes == (2, 31)
    assert PointFilter().for_format(3).classes is None
    with pytest.raises(ValueError, match='format 11'):
        f.for_format(11)


# ------------------------------------------------------------------------------------------------ refusals before the device
def _las_file(tmp_path, point_format=1, n=16):
    rng = np.random.RandomState(3)
    path = str(tmp_path / f'f{point_format}.las')
    las_ref.write_las(path, rng.uniform(0, 50, (n, 3)), rng.randint(0, 40000, n), point_format=point_format,
                      version=(1, 4) if point_format >= 6 else (1, 2))
    return path


def test_readers_with_a_filter_refuse_a_cpu_device(tmp_path):
    path = _las_file(tmp_path)
    for call in (lambda: las_io.read_las_raw(path, 'cpu', select=PointFilter(classes=[2])),
                 lambda: las_io.read_las(path, 'cpu', select=PointFilter()),
                 lambda: las_io.decode_points(torch.zeros(80, dtype=torch.uint8), 20, 4, [1e-3] * 3, [0.0] * 3, point_format=0,
                                              select=PointFilter())):
        with pytest.raises(LanemapHipError, match='no CPU fallback'):
            call()


def test_reader_refuses_a_class_above_31_for_a_legacy_file_before_the_upload(tmp_path):
    with pytest.raises(ValueError, match='point format 1'):
        las_io.read_las_raw(_las_file(tmp_path), 'cpu', select=PointFilter(classes=[40]))     # (a CPU device would be refused next)


class _FakeDevice:
    index = 0

    def __eq__(self, other):
        return other is self


class _FakeTensor:
    """Stands in for a device tensor where only the call that is made matters."""
    is_cuda = True
    dtype = torch.float32

    def __init__(self, shape, device):
        self.shape, self.device = shape, device

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return 4096


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('lm_'):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_without_a_filter_the_plain_decode_is_called_and_nothing_else(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(las_io, 'lib', lambda: rec)
    monkeypatch.setattr(torch._C, '_cuda_getCurrentRawStream', lambda index: 0, raising=False)
    d = _FakeDevice()
    records, out = _FakeTensor((80,), d), _FakeTensor((4, 4), d)
    got = las_io.decode_points(records, 20, 4, [1e-3] * 3, [0.0] * 3, [1.0, 2.0, 3.0], False, out=out)
    assert got is out
    assert [name for name, _ in rec.calls] == ['lm_las_decode_points']
    args = rec.calls[0][1]
    assert len(args) == len(SIGNATURES['lm_las_decode_points'][1]) == 11
    assert (args[2], args[3], args[7], args[8], args[9]) == (20, 4, las_io.INTEN_MIN, las_io.INTEN_MAX, 0)
    assert list(args[6]) == [1.0, 2.0, 3.0]
    rec.calls.clear()
    las_io.decode_points(records, 20, 4, [1e-3] * 3, [0.0] * 3, out=out, point_format=6, select=None)
    assert [name for name, _ in rec.calls] == ['lm_las_decode_points']
    with pytest.raises(ValueError, match='return_hist'):
        las_io.decode_points(records, 20, 4, [1e-3] * 3, [0.0] * 3, out=out, return_hist=True)
    with pytest.raises(ValueError, match='point_format'):
        las_io.decode_points(records, 20, 4, [1e-3] * 3, [0.0] * 3, out=out, select=PointFilter())
    with pytest.raises(TypeError, match='PointFilter'):
        las_io.decode_points(records, 20, 4, [1e-3] * 3, [0.0] * 3, out=out, point_format=0, select={'classes': [2]})
    assert [name for name, _ in rec.calls] == ['lm_las_decode_points']


def test_runner_takes_its_default_filter_from_the_config():
    from lanemapping_amd.config import Config
    from lanemapping_amd.runner import Runner
    r = Runner.__new__(Runner)
    r.cfg = Config({'batch_size': 2})
    assert r._las_select(None) is None
    f = PointFilter(classes=[2])
    assert r._las_select(f) is f
    r.cfg = Config({'las_select': {'classes': [2, 11], 'z_range': (-1.0, 4.0)}})
    assert r._las_select(None) == PointFilter(classes=[2, 11], z_range=(-1.0, 4.0)) and r._las_select(f) is f
    with pytest.raises(TypeError, match='PointFilter'):
        r._las_select({'classes': [2]})
    r.cfg = Config({'las_select': {'returns': 'second'}})
    with pytest.raises(ValueError, match='returns'):
        r._las_select(None)


# ------------------------------------------------------------------------------------------------ the C entry without a GPU
def test_entry_refuses_bad_arguments_without_a_gpu():
    L = lib()
    d3 = (C.c_double * 3)(1e-3, 1e-3, 1e-3)
    kept = C.c_long(-1)

    def call(record_len=20, fmt=0, n=0, sel=None):
        s = sel if sel is not None else PointFilter().as_struct()
        return L.lm_las_decode_select(None, None, record_len, fmt, n, d3, d3, None, 800.0, 33000.0, 0, C.byref(s), None, 0, None,
                                      C.byref(kept), None)

    assert call(record_len=19) == 1 and b'record length 19' in L.lm_last_error()
    assert call(record_len=161) == 1 and b'record length 161' in L.lm_last_error()
    assert call(fmt=11) == 1 and b'format 11' in L.lm_last_error()
    assert call(n=-1) == 1 and call(n=1 << 31) == 1 and b'2^31 - 1' in L.lm_last_error()
    assert call(n=5) == 1 and b'null pointer' in L.lm_last_error()
    s = PointFilter().as_struct()
    s.z_lo = math.nan
    assert call(sel=s) == 1 and b'NaN' in L.lm_last_error()
    s = PointFilter().as_struct()
    s.returns = 4
    assert call(sel=s) == 1 and b'returns=4' in L.lm_last_error()
    s = PointFilter().as_struct()
    s.drop_flags = 16
    assert call(sel=s) == 1 and b'drop_flags=16' in L.lm_last_error()
    assert L.lm_las_select_workspace_bytes(-1) == 0 and L.lm_las_select_workspace_bytes(1 << 31) == 0
    sizes = [L.lm_las_select_workspace_bytes(n) for n in (0, 1, 256, 257, 1 << 20, (1 << 31) - 1)]
    assert all(v > 0 for v in sizes) and sizes == sorted(sizes)


# ------------------------------------------------------------------------------------------------ the header and the inventories
def test_header_declares_the_entry_with_hip_stream_and_the_inventories_hold():
    text = open(os.path.join(ROOT, 'include', 'lanemap_hip.h')).read()
    assert re.search(r'\blm_las_decode_select\(void\* hip_stream\b', text)
    assert 'lm_las_decode_select' not in bounds_inventory._stream_entries()
    assert 'lm_las_decode_points' in bounds_inventory._stream_entries()
    assert {'lm_las_decode_select', 'lm_las_select_workspace_bytes'} <= set(entry_inventory._declared())
    bounds_inventory.test_header_stream_entries_parse()
    bounds_inventory.test_every_stream_entry_has_a_bounds_case_or_reason()
    entry_inventory.test_header_parses_into_entries()
    entry_inventory.test_every_entry_point_is_tested_or_listed()
    # the guarded-buffer case the header's NOTE points to exists
    gpu = open(os.path.join(ROOT, 'tests', 'test_gpu_las_select.py')).read()
    assert re.search(r'^def test_select_guards\(', gpu, flags=re.M) and 'lm_las_decode_select(' in gpu


# ------------------------------------------------------------------------------------------------ the twelve option classes
OPTION_CASES = [
    (las_io.PointFilter, dict(classes=[11, 2], drop_keypoint=True, returns='last', z_range=(-1, 2.5))),
    (las_io.GroundFilter, dict(height_range=(-0.5, 1), cell_px=16, datum=False, datum_margin=0.5)),
    (las_io.IntensityStretch, dict(percentiles=(2, 99), scope='strip', white=240, min_span=8, min_points=10, fallback=(100, 2000))),
    (las_io.ElevationDrape, dict(radius_px=2, min_pixels=3, fit='none')),
    (las_io.GapFill, dict(radius_px=2, max_radius_px=3, coverage=0.5)),
    (las_io.MarkingLabels, dict(half_width=0.25, z_tol=1, min_intensity=700, marking_class=70, line_ids=False)),
    (las_io.MarkingSurvey, dict(bin=0.5, half_width=0.25, z_tol=1, min_intensity=900, min_points=2, max_gap=1, solid_cover=0.75)),
    (las_io.MarkingColour, dict(yellow_ratio=0.5, yellow_share=0.25, min_coloured=3)),
    (las_io.CrossSection, dict(paint_intensity=9000)),
    (las_io.PaintResidue, dict(min_intensity=9000)),
    (las_io.PaintThreshold, dict(half_width=0.5, ring=0.03125, inner=0.0625, outer=0.25, z_tol=1, bin_shift=4, min_returns=10,
                                 min_separation=0.1, tolerance_shift=3)),
    (las_io.StripStream, dict(chunk_records=512, binned_budget=1 << 20)),
]


def test_the_option_case_list_names_every_option_class():
    """Every class of las_options that declares __slots__ of its own is in OPTION_CASES: a new stage's options get the same checks.
    las_io hands each of them on under its name."""
    from lanemapping_amd import las_options
    slotted = {c for c in vars(las_options).values()
               if isinstance(c, type) and c.__module__ == las_options.__name__ and c.__dict__.get('__slots__')}
    assert slotted == {c for c, _ in OPTION_CASES} and len(OPTION_CASES) == 12
    for c in slotted:
        assert getattr(las_io, c.__name__) is c, c.__name__


def test_las_io_hands_on_every_name_it_once_fetched_on_demand():
    """The names las_io used to fetch from two other modules on first use are plain attributes of it, and the options module stands on
    its own: importing it in a fresh interpreter loads neither torch nor las_io."""
    import subprocess
    import sys
    for name in ('PaintThreshold', 'hist_records', 'hist_files', 'paint_threshold', 'KS_COEFF', 'HIST_BIN', 'StripStream', 'LasChunks',
                 'tile_groups'):
        assert name in vars(las_io), name
    code = ("import sys, lanemapping_amd.las_options\n"
            "print(int('torch' in sys.modules), int('lanemapping_amd.las_io' in sys.modules))")
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.split() == ['0', '0'], out


@pytest.mark.parametrize('cls, kwargs', OPTION_CASES, ids=[c.__name__ for c, _ in OPTION_CASES])
def test_option_classes_are_values(cls, kwargs):
    """What the twelve option classes share: repr round-trips, equality and hash by value within the class only, no assignment, no deletion,
    no instance dictionary, the arguments in __slots__ order."""
    name = cls.__name__
    x = cls(**kwargs)
    values = tuple(getattr(x, k) for k in cls.__slots__)
    y = eval(repr(x), {name: cls})
    assert y == x and y is not x and hash(y) == hash(x) and not (y != x)
    assert cls(**kwargs) == x and hash(cls(**kwargs)) == hash(x)
    other = next(c(**kw) for c, kw in OPTION_CASES if c is not cls)
    assert x != other and not (x == other) and x != values and not (x == values) and x != None    # noqa: E711
    for k in cls.__slots__:
        with pytest.raises(AttributeError, match=f'{name} is immutable'):
            setattr(x, k, getattr(x, k))
        with pytest.raises(AttributeError, match=f'{name} is immutable'):
            delattr(x, k)
    with pytest.raises(AttributeError):
        x.no_such_option = 1
    assert not hasattr(x, '__dict__')
    assert repr(x) == name + '(' + ', '.join(f'{k}={v!r}' for k, v in zip(cls.__slots__, values)) + ')'
    assert tuple(getattr(x, k) for k in cls.__slots__) == values, 'a refused assignment changed nothing'


# ------------------------------------------------------------------------------------------------ the Runner's stages after the map
def _stage_runner():
    from lanemapping_amd.runner import Runner
    rn = Runner.__new__(Runner)
    rn.device = 'cuda:0'
    return rn


def test_runner_stages_take_each_real_file_once_and_the_lines_the_call_returns(tmp_path, monkeypatch):
    """The four stages after the map (label, survey with and without colour, cross, residue) hand las_io each real file once, in input
    order, with the (path, shift, select) of its first listing - a symbolic link to a listed file is that file -, and the lines the call
    returns: `merged` when there are any, else the tiles' 3-D lines in the order of the sorted tile names.  las_io's file functions are
    replaced by recorders, so nothing here needs a GPU."""
    from lanemapping_amd import ops
    a, b, link = str(tmp_path / 'a.las'), str(tmp_path / 'b.las'), str(tmp_path / 'again.las')
    for p in (a, b):
        open(p, 'wb').close()
    os.symlink(a, link)
    sel = PointFilter(classes=[2])
    files = [(b, [5.0, 0.0, 0.0], None), (a, [1.0, 2.0, 3.0], sel), (b, [6.0, 0.0, 0.0], sel), (link, [7.0, 0.0, 0.0], None), (a, [8.0, 0.0, 0.0], None)]
    once = [(b, [5.0, 0.0, 0.0], None), (a, [1.0, 2.0, 3.0], sel)]
    line = lambda x: np.array([[x, 0.0, 0.0], [x, 4.0, 0.0]])
    lines3d = {'t2': [line(3.0)], 't10': [line(1.0), line(2.0)]}                  # 't10' sorts before 't2'
    merged = [line(9.0), line(8.0)]
    got = {}
    real = {k: getattr(las_io, k) for k in ('survey_files', 'survey_colour_files', 'cross_files')}

    def label_las(path, out_path, lines, labels, shift, select=None, device='cuda:0'):
        got.setdefault('label', []).append(((path, shift, select), lines, out_path))
        return {'records': 0, 'labelled': 0, 'per_line': [0] * len(lines)}

    def table(kind):
        def fake(files_, lines, *options, device='cuda:0'):
            got[kind] = (list(files_), lines)
            return real[kind]([], lines, *options, device=device)              # the tables of no file: host only
        return fake

    def residue_files(files_, lines, residue, device='cuda:0'):
        got['residue'] = (list(files_), lines)
        return ops.ResidueBlobs(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), np.zeros((0, 12), np.int64),
                                {'x0': 0.0, 'y0': 0.0, 'cell': residue.cell, 'nx': 1, 'ny': 1, 'shift': [0.0, 0.0, 0.0]})

    monkeypatch.setattr(las_io, 'label_las', label_las)
    monkeypatch.setattr(las_io, 'residue_files', residue_files)
    for kind in real:
        monkeypatch.setattr(las_io, kind, table(kind))
    rn = _stage_runner()
    survey, colour = las_io.MarkingSurvey(), las_io.MarkingColour()
    for tag, result, want in (('merged', (lines3d, merged), merged), ('tiles', (lines3d, []), [line(1.0), line(2.0), line(3.0)])):
        got.clear()
        out = str(tmp_path / tag)
        rn._label_inputs(las_io.MarkingLabels(), files, result, out)
        rn._survey_inputs(survey, files, result, out)
        rn._survey_inputs(survey, files, result, out, colour)
        rn._cross_inputs(las_io.CrossSection(9000.0), files, result, out)
        rn._residue_inputs(las_io.PaintResidue(9000.0), files, result, out)
        assert [g[0] for g in got['label']] == once, tag
        assert [g[2] for g in got['label']] == [os.path.join(out, 'labelled', 'b.las'), os.path.join(out, 'labelled', 'a.las')]
        for kind in ('survey_files', 'survey_colour_files', 'cross_files', 'residue'):
            assert got[kind][0] == once, (tag, kind)
        for lines in [g[1] for g in got['label']] + [got[k][1] for k in ('survey_files', 'survey_colour_files', 'cross_files', 'residue')]:
            assert len(lines) == len(want) and all(np.array_equal(l, w) for l, w in zip(lines, want)), tag
        assert sorted(os.listdir(os.path.join(out, 'params'))) == ['cross_sections.json', 'cross_sections.npy', 'labels.json', 'marking_colours.npy',
                                                                   'markings.json', 'markings.npy', 'residue.json', 'residue.npy', 'residue_cells.npy']
    # two different files under one basename: refused by the label stage before anything is labelled
    os.makedirs(str(tmp_path / 'd'))
    twin = str(tmp_path / 'd' / 'a.las')
    open(twin, 'wb').close()
    got.clear()
    with pytest.raises(ValueError, match="share the basename 'a.las'"):
        rn._label_inputs(las_io.MarkingLabels(), [(a, None, None), (twin, None, None)], (lines3d, merged), str(tmp_path / 'twin'))
    assert 'label' not in got and not os.path.exists(str(tmp_path / 'twin'))
