"""GPU: labelling the returns by the lane lines (csrc/label.hip: lm_label_points, lm_las_label_records; ops.line_index / label_points,
las_io.label_las, Runner `label=`).

The reference is tests/label_ref.py: the float32 rule by brute force over all segments, without a grid.  Labels, distances, patched records
and counts are compared for equal bits."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import label_ref as lr
import lds_state
from guards import Slab, guarded_runs
from lanemapping_amd import io_utils, las_io, ops
from lanemapping_amd._lib import lib
from lanemapping_amd.las_io import MarkingLabels, PointFilter
from oracle import las_ref

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float('nan')
CHUNK = 1024                                   # points per workgroup of label_points_kernel (csrc/label.hip: CHUNK = 256 * PER)


def _chunk():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lanemapping_amd', 'csrc', 'label.hip')).read()
    assert 'constexpr int PER = 4;' in text and 'constexpr int CHUNK = 256 * PER;' in text
    return CHUNK


@functools.lru_cache(maxsize=None)
def _scene():
    """-> (segments, points, float32 brute-force reference without and with min_intensity = 500): computed once, never changed."""
    seg = las_io.line_segments([l + lr.SHIFT for l in lr.scene_lines()], lr.SHIFT)
    g, _, _ = ops.line_index_host(seg, lr.HW)
    pts = lr.scene_points(seg, (g.x0, g.y0, g.cell, g.nx, g.ny))
    plain = lr.label_f32(pts, seg, lr.HW, lr.ZTOL)
    bright = lr.label_f32(pts, seg, lr.HW, lr.ZTOL, min_intensity=500.0)
    for a in (seg, pts, *plain, *bright):
        a.setflags(write=False)
    return seg, pts, plain, bright


def _t(a):
    return torch.from_numpy(np.array(a, copy=True))              # (the shared scene arrays are read-only)


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.int32) if a.dtype == f32 else a


def _check(tag, got, want):
    line, d2 = got
    assert np.array_equal(_bits(line), want[0]), f'{tag}: {int((_bits(line) != want[0]).sum())} labels differ from the float32 brute force'
    assert np.array_equal(_bits(d2), want[1].view(np.int32)), f'{tag}: dist2 differs from the float32 brute force in its bits'


# ------------------------------------------------------------------------------------------------ 1. exactness
def test_labels_equal_the_float32_brute_force(dev):
    seg, pts, plain, bright = _scene()
    line, d2, win = plain
    # the scene holds what it is meant to hold
    assert line[lr.SHARED_VERTEX] == 1 and win[lr.SHARED_VERTEX] == 2 and line[lr.TRIPLE] == 5 and line[lr.CROSSING] == 1
    hw2 = f32(lr.HW) * f32(lr.HW)
    assert all(line[i] == 1 and d2[i] == hw2 for i in lr.EXACT_HW) and all(line[i] == 1 for i in lr.EXACT_ZTOL)
    assert line[lr.BETWEEN] == 0 and line[lr.ON_LINE_4] == 4 and [bright[0][i] for i in lr.INTENSITY] == [1, 0, 0]
    assert set(np.unique(line)) == {0, 1, 2, 3, 4, 5} and not np.isfinite(pts[:, :3]).all() and np.isnan(pts[:, 3]).any()
    index = ops.line_index(seg, lr.HW, device=dev)
    d_pts = _t(pts).to(dev)
    full = len(pts)
    assert full > 2 * _chunk()
    for N in (1, 63, 64, 65, 255, 256, 257, _chunk() + 1, full):
        _check(f'N={N}', ops.label_points(d_pts[:N], index, lr.ZTOL, want_dist2=True), (line[:N], d2[:N]))
        _check(f'N={N}, min_intensity', ops.label_points(d_pts[:N], index, lr.ZTOL, min_intensity=500.0, want_dist2=True),
               (bright[0][:N], bright[1][:N]))
    # the labels alone (dist2 = NULL), and the same bits on a second run
    assert np.array_equal(_bits(ops.label_points(d_pts, index, lr.ZTOL)), line)
    _check('second run', ops.label_points(d_pts, index, lr.ZTOL, want_dist2=True), (line, d2))
    # no segments (S = 0), no lines (L = 0), no points
    for empty in (ops.line_index(np.zeros((0, 8), f32), lr.HW, device=dev), ops.line_index(las_io.line_segments([]), lr.HW, device=dev),
                  ops.line_index(las_io.line_segments([lr.scene_lines()[5]]), lr.HW, device=dev)):
        l0, d0 = ops.label_points(d_pts, empty, lr.ZTOL, want_dist2=True)
        assert not bool(l0.any()) and bool(torch.isinf(d0).all()) and bool((d0 > 0).all())
    l0, d0 = ops.label_points(d_pts[:0], index, lr.ZTOL, want_dist2=True)
    assert l0.shape == (0,) and d0.shape == (0,)


def test_tie_goes_to_the_smaller_line_whatever_the_table_order(dev):
    """line_segments lists line 1 before line 3, so at their shared vertex list order alone already picks line 1.  With line 3's rows
    moved to the front of the table, line 3 is met first at d2 = 0 and only the rule 'ties go to the smaller line' picks line 1."""
    seg, pts, plain, _ = _scene()
    perm = lr.permuted_table(seg)
    assert lr.seg_lines(perm)[0] == 3 and sorted(lr.seg_lines(perm)) == sorted(lr.seg_lines(seg))
    want = lr.label_f32(pts, perm, lr.HW, lr.ZTOL)
    assert want[0][lr.CROSSING] == 1 and np.array_equal(want[0], plain[0]) and np.array_equal(want[1].view(np.int32), plain[1].view(np.int32))
    first = lr.label_f32(pts, perm, lr.HW, lr.ZTOL, line_tie=False)[0]
    assert first[lr.CROSSING] == 3 and (first != want[0]).sum() >= 1, 'without the line rule the permuted table gives another label'
    index = ops.line_index(perm, lr.HW, device=dev)
    _check('permuted table', ops.label_points(_t(pts).to(dev), index, lr.ZTOL, want_dist2=True), want[:2])


# ------------------------------------------------------------------------------------------------ 2. the grid decides the cost only
def test_labels_do_not_depend_on_the_grid(dev):
    seg, pts, plain, _ = _scene()
    d_pts = _t(pts).to(dev)
    shapes = []
    for cell in (None, 0.5, 4.0, 1e6):
        index = ops.line_index(seg, lr.HW, cell=cell, device=dev)
        shapes.append((index.grid.nx, index.grid.ny))
        _check(f'cell={cell}', ops.label_points(d_pts, index, lr.ZTOL, want_dist2=True), plain[:2])
    assert shapes[3] == (1, 1) and shapes[1][0] > shapes[0][0] > shapes[2][0] > 1


# ------------------------------------------------------------------------------------------------ 3. against float64
def test_labels_against_float64(dev):
    """20,000 points drawn uniformly within +-1 m of the scene's lines.  A label may differ from the float64 brute force only where the
    float64 distance lies within 1e-4 m of half_width, the height difference within 1e-4 m of z_tol, or two lines' distances within
    1e-4 m of each other; such points are at most 1 % of the cloud (by area the band is about 2e-4 of the corridor)."""
    seg = _scene()[0]
    rng = np.random.RandomState(64)
    n, eps = 20000, 1e-4
    length = np.hypot(seg[:, 3], seg[:, 4]).astype(np.float64) + 0.05            # (the zero-length segment gets its share too)
    s = rng.choice(len(seg), n, p=length / length.sum())
    base = seg[s, 0:3].astype(np.float64) + rng.uniform(0, 1, n)[:, None] * seg[s, 3:6].astype(np.float64)
    pts = np.concatenate([base + rng.uniform(-1, 1, (n, 3)), np.full((n, 1), 1000.0)], axis=1).astype(f32)
    l64, d, zgap = lr.label_f64(pts, seg, lr.HW, lr.ZTOL)
    ds = np.sort(d, axis=1)
    with np.errstate(invalid='ignore'):                          # (inf - inf where no line is in reach: NaN, which compares false)
        close = (ds[:, 1] - ds[:, 0] <= eps) & (ds[:, 0] <= lr.HW + eps)
    unsure = (np.abs(d - lr.HW) <= eps).any(axis=1) | (zgap <= eps).any(axis=1) | close
    print(f'float64 reference: {int(unsure.sum())} of {n} points lie in a band of {eps} m around a decision; {int((l64 > 0).sum())} labelled')
    assert unsure.sum() <= 0.01 * n, 'the bands hold more than 1 % of the cloud'
    assert (l64 > 0).sum() > 0.03 * n and (l64 == 0).sum() > 0.3 * n
    index = ops.line_index(seg, lr.HW, device=dev)
    got = ops.label_points(_t(pts).to(dev), index, lr.ZTOL).cpu().numpy()
    differ = got != l64
    print(f'labels differing from float64: {int(differ.sum())}, all in a band: {bool(unsure[differ].all())}')
    assert unsure[differ].all(), f'{int((differ & ~unsure).sum())} labels differ from the float64 brute force away from every decision'
    assert np.array_equal(got, lr.label_f32(pts, seg, lr.HW, lr.ZTOL)[0])


# ------------------------------------------------------------------------------------------------ 4. records
SCALE, OFFSET = (0.001, 0.001, 0.001), tuple(lr.SHIFT + [3.0, -2.0, 0.5])
RECORD_LEN = {0: 20, 1: 28, 3: 34, 6: 30, 7: 36}


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _world(n, seed):
    """n points around the scene's lines in the LAS frame, intensities 0..1999."""
    seg = _scene()[0]
    rng = np.random.RandomState(seed)
    s = rng.randint(0, len(seg), n)
    base = seg[s, 0:3].astype(np.float64) + rng.uniform(0, 1, n)[:, None] * seg[s, 3:6].astype(np.float64)
    off = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), rng.uniform(-0.7, 0.7, n)], axis=1)
    return base + off + lr.SHIFT, rng.randint(0, 2000, n)


def _records(tmp_path, fmt, extra, n, seed):
    """-> ([n, rl] records, padded flat copy for the device): written by oracle/las_ref.write_las where it knows the format, by the same
    layout here for format 7.  Classification 2 for four records of five and 7 for the fifth; flag bits from the junk bytes."""
    world, inten = _world(n, seed)
    rl = RECORD_LEN[fmt] + extra
    if fmt in las_ref.RECORD_LEN:
        path = str(tmp_path / f'f{fmt}_{n}.las')
        las_ref.write_las(path, world, inten, point_format=fmt, version=(1, 4) if fmt >= 6 else (1, 2), scale=SCALE, offset=OFFSET,
                          extra_bytes=extra)
        data = np.fromfile(path, np.uint8)
        h = las_io.parse_header(data)
        assert (h['point_format'], h['record_len'], h['n_points']) == (fmt, rl, n)
        rec = data[h['offset_to_points']:h['offset_to_points'] + n * rl].reshape(n, rl).copy()
    else:
        q = np.round((world - np.asarray(OFFSET)) / np.asarray(SCALE)).astype('<i4')
        rec = np.zeros((n, rl), np.uint8)
        rec[:, 0:12] = q.view(np.uint8).reshape(n, 12)
        rec[:, 12:14] = inten.astype('<u2').reshape(n, 1).view(np.uint8)
        rec[:, 14:] = (np.arange(n)[:, None] * 7 + np.arange(rl - 14)[None, :]) % 251
    cls = np.where(np.arange(n) % 5 == 4, 7, 2)
    if fmt >= 6:
        rec[:, 16] = cls
    else:
        rec[:, 15] = (rec[:, 15] & 0xE0) | cls
    flat = np.zeros((n * rl + 3) // 4 * 4, np.uint8)
    flat[:n * rl] = rec.reshape(-1)
    return rec, flat


def _passes(rec, fmt, select):
    if select is None:
        return np.ones(len(rec), bool)
    cls = rec[:, 16] if fmt >= 6 else rec[:, 15] & 31
    withheld = (rec[:, 15] & 4) != 0 if fmt >= 6 else (rec[:, 15] & 128) != 0
    keep = np.isin(cls, np.asarray(select.classes)) if select.classes is not None else np.ones(len(rec), bool)
    assert select.returns == 'all' and select.z_range is None and not (select.drop_synthetic or select.drop_keypoint or select.drop_overlap)
    return keep & ~(withheld & select.drop_withheld)


def _label_call(dev, d_rec, rl, fmt, n, index, L, labels, select=None, d_out=None, want_line=True, want_counts=True, cls=None):
    """One lm_las_label_records call through ctypes: -> (rc, records_out, line, counts) as device tensors (None where not asked)."""
    d_out = torch.full_like(d_rec, 0xA5) if d_out is None else d_out
    line = torch.full((n,), 0x7EADBEEF, dtype=torch.int32, device=dev) if want_line else None
    counts = torch.full((L + 1,), -1, dtype=torch.int64, device=dev) if want_counts else None
    d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])
    sel = select.as_struct() if select is not None else None
    mi = NAN if labels.min_intensity is None else labels.min_intensity
    rc = lib().lm_las_label_records(_stream(dev), C.c_void_p(d_rec.data_ptr()), rl, fmt, n, d3(SCALE), d3(OFFSET), d3(lr.SHIFT),
                                    C.byref(sel) if sel is not None else None, *index.args(), labels.z_tol, mi,
                                    labels.for_format(fmt) if cls is None else cls, int(labels.line_ids), C.c_void_p(d_out.data_ptr()),
                                    C.c_void_p(line.data_ptr()) if want_line else None,
                                    C.c_void_p(counts.data_ptr()) if want_counts else None, L)
    return rc, d_out, line, counts


@pytest.mark.parametrize('fmt, extra', [(0, 0), (1, 3), (3, 0), (6, 0), (7, 1)])
def test_records_equal_the_patcher(dev, tmp_path, fmt, extra):
    seg = _scene()[0]
    index = ops.line_index(seg, lr.HW, device=dev)
    L = index.n_lines
    assert L == 5
    rl = RECORD_LEN[fmt] + extra
    assert (extra == 0) or rl % 2 == 1
    for n in (255, 256, 257, 513):
        rec, flat = _records(tmp_path, fmt, extra, n, seed=100 * fmt + n)
        dec = lr.decode_f32(rec, SCALE, OFFSET, lr.SHIFT)
        d_rec = torch.from_numpy(flat).to(dev)
        # the decode's own rows: what the labelling sees
        assert np.array_equal(_bits(las_io.decode_points(d_rec, rl, n, SCALE, OFFSET, lr.SHIFT, normalise=False)), dec.view(np.int32))
        for name, labels, select in (('plain', MarkingLabels(lr.HW, lr.ZTOL), None),
                                     ('class 2 only', MarkingLabels(lr.HW, lr.ZTOL), PointFilter(classes=[2], drop_withheld=False)),
                                     ('no withheld, bright', MarkingLabels(lr.HW, lr.ZTOL, min_intensity=700), PointFilter()),
                                     ('no line ids', MarkingLabels(lr.HW, lr.ZTOL, line_ids=False, marking_class=9), None)):
            tag = f'format {fmt}, {rl} B, n={n}, {name}'
            ok = _passes(rec, fmt, select)
            want_line = lr.label_f32(dec, seg, lr.HW, lr.ZTOL, labels.min_intensity, mask=ok)[0]
            assert (want_line > 0).sum() > n // 20 and (want_line == 0).sum() > n // 20, tag
            want = lr.patch_records(rec, fmt, want_line, labels.for_format(fmt), labels.line_ids)
            want_counts = np.bincount(want_line, minlength=L + 1)
            want_counts[0] = int((ok & (want_line == 0)).sum())
            rc, d_out, line, counts = _label_call(dev, d_rec, rl, fmt, n, index, L, labels, select)
            assert rc == 0, lib().lm_last_error()
            out = d_out.cpu().numpy()
            assert np.array_equal(out[:n * rl].reshape(n, rl), want), f'{tag}: records_out differs from the patcher'
            assert np.array_equal(out[n * rl:], flat[n * rl:]), f'{tag}: the padding bytes changed'
            assert np.array_equal(line.cpu().numpy(), want_line), f'{tag}: line differs'
            assert np.array_equal(counts.cpu().numpy(), want_counts), f'{tag}: counts {counts.cpu().numpy()} != {want_counts}'
            cb, so = (16, 20) if fmt >= 6 else (15, 18)
            if fmt < 6:
                assert np.array_equal(out[:n * rl].reshape(n, rl)[:, 15] >> 5, rec[:, 15] >> 5), f'{tag}: flag bits of byte 15 changed'
            if not labels.line_ids:
                assert np.array_equal(out[:n * rl].reshape(n, rl)[:, so:so + 2], rec[:, so:so + 2]), f'{tag}: the source ID changed'
            if name == 'class 2 only':
                seven = (rec[:, cb] & (255 if fmt >= 6 else 31)) == 7
                on_line = lr.label_f32(dec, seg, lr.HW, lr.ZTOL)[0] > 0
                assert (seven & on_line).sum() > 0 and np.array_equal(out[:n * rl].reshape(n, rl)[seven], rec[seven]), \
                    f'{tag}: a class-7 record on a line was relabelled under classes=[2]'
            # in place, and without line / counts: the same bytes
            d_same = d_rec.clone()
            rc, d_got, _, _ = _label_call(dev, d_same, rl, fmt, n, index, L, labels, select, d_out=d_same, want_line=False, want_counts=False)
            assert rc == 0 and d_got.data_ptr() == d_same.data_ptr() and np.array_equal(d_same.cpu().numpy(), out), f'{tag}: in place'
    # the package entry on the last case gives the same as the direct call
    out2, counts2, line2 = las_io.label_records(d_rec, {'point_format': fmt, 'record_len': rl, 'n_points': n, 'scale': SCALE, 'offset': OFFSET},
                                                index, labels, lr.SHIFT, select, want_line=True)
    assert np.array_equal(out2.cpu().numpy(), out) and np.array_equal(counts2.cpu().numpy(), want_counts)
    assert np.array_equal(line2.cpu().numpy(), want_line)
    # no segments: a copy, every record that passes counted under 0
    empty = ops.line_index(np.zeros((0, 8), f32), lr.HW, device=dev)
    rc, d_out, line, counts = _label_call(dev, d_rec, rl, fmt, n, empty, 0, MarkingLabels(lr.HW, lr.ZTOL), PointFilter(classes=[2], drop_withheld=False))
    assert rc == 0 and np.array_equal(d_out.cpu().numpy(), flat) and not bool(line.any())
    assert counts.cpu().numpy().tolist() == [int(_passes(rec, fmt, PointFilter(classes=[2], drop_withheld=False)).sum())]


def test_counts_of_more_lines_than_the_lds_histogram_holds(dev, tmp_path):
    """1,100 one-segment lines: labels from 1,024 on are counted by adds to device memory, the others in the workgroup's LDS histogram.
    counts, line, the point source IDs (two bytes are needed) and the records equal the reference."""
    L, n = 1100, 3000
    x0 = 0.5 * np.arange(L)
    lines = [np.array([[x, 1.0, 0.0], [x + 0.375, 1.0, 0.0]]) + lr.SHIFT for x in x0]
    seg = las_io.line_segments(lines, lr.SHIFT)
    rng = np.random.RandomState(1024)
    k = np.concatenate([rng.randint(0, L, n - 400), rng.randint(1023, L, 400)])          # every part of the range is met
    world = np.stack([x0[k] + rng.uniform(-0.05, 0.425, n), 1.0 + rng.uniform(-0.25, 0.25, n), rng.uniform(-0.6, 0.6, n)], axis=1) + lr.SHIFT
    for i, kk in enumerate((1022, 1022, 1023, 1023)):                                    # on lines 1,023 and 1,024: both sides of the seam
        world[i] = np.array([x0[kk] + 0.125 * (1 + i % 2), 1.0, 0.0]) + lr.SHIFT
    path = str(tmp_path / 'many.las')
    las_ref.write_las(path, world, rng.randint(0, 2000, n), point_format=1, scale=SCALE, offset=OFFSET)
    data = np.fromfile(path, np.uint8)
    h = las_io.parse_header(data)
    rec = data[h['offset_to_points']:h['offset_to_points'] + n * 28].reshape(n, 28)
    flat = np.ascontiguousarray(rec).reshape(-1).copy()
    assert len(flat) % 4 == 0
    want_line = lr.label_f32(lr.decode_f32(rec, SCALE, OFFSET, lr.SHIFT), seg, lr.HW, lr.ZTOL)[0]
    assert (want_line >= 1024).sum() > 100 and ((want_line > 0) & (want_line < 1024)).sum() > 100 and (want_line == 0).sum() > 100
    assert (want_line == 1024).sum() >= 2 and (want_line == 1023).sum() >= 2 and want_line.max() > 1050
    index = ops.line_index(seg, lr.HW, device=dev)
    assert index.n_lines == L
    labels = MarkingLabels(lr.HW, lr.ZTOL)
    for word in lds_state.WORDS:                                         # integer adds: the same counts every run, whatever LDS held before
        with lds_state.poisoned(word):                                   # (0xFFFFFFFF / +Inf in the LDS histogram the kernel must clear itself)
            rc, d_out, line, counts = _label_call(dev, torch.from_numpy(flat).to(dev), 28, 1, n, index, L, labels)
        assert rc == 0, lib().lm_last_error()
        assert np.array_equal(line.cpu().numpy(), want_line)
        assert np.array_equal(counts.cpu().numpy(), np.bincount(want_line, minlength=L + 1))
        assert np.array_equal(d_out.cpu().numpy().reshape(n, 28), lr.patch_records(rec, 1, want_line, 31, True))


def test_label_las_keeps_header_vlrs_and_evlrs(dev, tmp_path):
    """las_io.label_las on a format-3 file with VLR bytes in front of the records and EVLR bytes behind them: both survive, the records
    equal the patcher, the counts are the reference's."""
    lines = [l + lr.SHIFT for l in lr.scene_lines()]
    seg = las_io.line_segments(lines, lr.SHIFT)
    n = 1500
    world, inten = _world(n, 9)
    src, dst = str(tmp_path / 'in.las'), str(tmp_path / 'sub' / 'out.las')
    las_ref.write_las(src, world, inten, point_format=3, scale=SCALE, offset=OFFSET, extra_bytes=1, vlr_bytes=54)
    tail = (np.arange(77) * 3 % 256).astype(np.uint8)
    with open(src, 'ab') as f:
        f.write(tail.tobytes())
    data = np.fromfile(src, np.uint8)
    h = las_io.parse_header(data)
    off, rl = h['offset_to_points'], h['record_len']
    rec = data[off:off + n * rl].reshape(n, rl)
    labels = MarkingLabels(lr.HW, lr.ZTOL)
    got = las_io.label_las(src, dst, lines, labels, lr.SHIFT, device=dev)
    want_line = lr.label_f32(lr.decode_f32(rec, SCALE, OFFSET, lr.SHIFT), seg, lr.HW, lr.ZTOL)[0]
    assert got == {'records': n, 'labelled': int((want_line > 0).sum()), 'per_line': np.bincount(want_line, minlength=7)[1:].tolist()}
    assert len(got['per_line']) == 6 and got['per_line'][5] == 0 and got['labelled'] > 100
    out = np.fromfile(dst, np.uint8)
    assert len(out) == len(data) and np.array_equal(out[:off], data[:off]) and np.array_equal(out[off + n * rl:], tail)
    assert np.array_equal(out[off:off + n * rl].reshape(n, rl), lr.patch_records(rec, 3, want_line, 31, True))
    with pytest.raises(ValueError, match='marking_class=40'):
        las_io.label_las(src, dst, lines, MarkingLabels(marking_class=40), lr.SHIFT, device=dev)


# ------------------------------------------------------------------------------------------------ 5. guarded buffers
def _index_slabs(dev, seg, start, segs, poisoned):
    s_seg = Slab(dev, len(seg), 8, front=4, back=4).fill_input(_t(seg), NAN if poisoned else 0.0)
    s_start = Slab(dev, 1, len(start), front=1, back=1, dtype=torch.int32).fill_input(torch.from_numpy(start), 0x7FFFFFF0 if poisoned else 0)
    s_segs = Slab(dev, 1, len(segs), front=1, back=1, dtype=torch.int32).fill_input(torch.from_numpy(segs), 0x7FFFFFF0 if poisoned else 0)
    return s_seg, s_start, s_segs


@pytest.mark.parametrize('with_dist2', [True, False])
def test_label_points_guards(dev, with_dist2):
    """lm_label_points with the points, the segment table, the two lists and the outputs each between guard slabs: N one past a
    workgroup's share.  Outputs are written only inside their extents, poisoned guards change no output bit, inputs are not written."""
    seg, pts, plain, _ = _scene()
    N = _chunk() + 1
    g, start, segs = ops.line_index_host(seg, lr.HW)
    keep = []

    def run(B, poisoned):
        s_pts = Slab(dev, N, 4, front=8, back=8).fill_input(_t(pts[:N]), NAN if poisoned else 0.0)
        s_seg, s_start, s_segs = _index_slabs(dev, seg, start, segs, poisoned)
        s_line = Slab(dev, 1, N, front=1, back=1, dtype=torch.int32).fill_canary()
        s_d2 = Slab(dev, 1, N, front=1, back=1).fill_canary()
        before = [s.bits().clone() for s in (s_pts, s_seg, s_start, s_segs)]
        rc = lib().lm_label_points(_stream(dev), C.c_void_p(s_pts.ptr()), N, C.c_void_p(s_seg.ptr()), len(seg), C.byref(g),
                                   C.c_void_p(s_start.ptr()), C.c_void_p(s_segs.ptr()), lr.HW, lr.ZTOL, NAN, C.c_void_p(s_line.ptr()),
                                   C.c_void_p(s_d2.ptr()) if with_dist2 else None)
        assert rc == 0, lib().lm_last_error()
        torch.cuda.synchronize()
        for s, b in zip((s_pts, s_seg, s_start, s_segs), before):
            assert torch.equal(s.bits(), b), 'an input was written'
        keep.append(s_d2)
        return {'line': (s_line, 1), **({'dist2': (s_d2, 1)} if with_dist2 else {})}

    got = guarded_runs(run, 'label_points', batch=False)
    assert np.array_equal(got['line'].numpy()[0], plain[0][:N])
    if with_dist2:
        assert np.array_equal(got['dist2'].numpy()[0].view(np.int32), plain[1][:N].view(np.int32))
    else:
        c = keep[0].bits()
        assert bool((c == c[0]).all()), 'dist2 = NULL, yet its buffer was written'


@pytest.mark.parametrize('with_outputs', [True, False])
def test_label_records_guards(dev, tmp_path, with_outputs):
    """lm_las_label_records with records, records_out, line and counts between guard slabs: 257 records of 37 bytes (the last dword of the
    records is padding, the last block holds one record); line and counts given, and both NULL."""
    seg = _scene()[0]
    fmt, extra, n = 7, 1, 257
    rl = RECORD_LEN[fmt] + extra
    rec, flat = _records(tmp_path, fmt, extra, n, seed=7)
    g, start, segs = ops.line_index_host(seg, lr.HW)
    L = g.max_line
    sel = PointFilter(classes=[2], drop_withheld=False)
    want_line = lr.label_f32(lr.decode_f32(rec, SCALE, OFFSET, lr.SHIFT), seg, lr.HW, lr.ZTOL, mask=_passes(rec, fmt, sel))[0]
    want = lr.patch_records(rec, fmt, want_line, 64, True)
    d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])
    st = sel.as_struct()

    def run(B, poisoned):
        s_rec = Slab(dev, 1, len(flat), front=1, back=1, dtype=torch.uint8).fill_input(torch.from_numpy(flat), 0xFF if poisoned else 0)
        s_seg, s_start, s_segs = _index_slabs(dev, seg, start, segs, poisoned)
        s_out = Slab(dev, 1, len(flat), front=1, back=1, dtype=torch.uint8).fill_canary()
        s_line = Slab(dev, 1, n, front=1, back=1, dtype=torch.int32).fill_canary()
        s_cnt = Slab(dev, L + 1, 2, front=8, back=8, dtype=torch.int32).fill_canary()
        before = [s.bits().clone() for s in (s_rec, s_seg, s_start, s_segs)]
        rc = lib().lm_las_label_records(_stream(dev), C.c_void_p(s_rec.ptr()), rl, fmt, n, d3(SCALE), d3(OFFSET), d3(lr.SHIFT), C.byref(st),
                                        C.c_void_p(s_seg.ptr()), len(seg), C.byref(g), C.c_void_p(s_start.ptr()), C.c_void_p(s_segs.ptr()),
                                        lr.HW, lr.ZTOL, NAN, 64, 1, C.c_void_p(s_out.ptr()),
                                        C.c_void_p(s_line.ptr()) if with_outputs else None,
                                        C.c_void_p(s_cnt.ptr()) if with_outputs else None, L)
        assert rc == 0, lib().lm_last_error()
        torch.cuda.synchronize()
        for s, b in zip((s_rec, s_seg, s_start, s_segs), before):
            assert torch.equal(s.bits(), b), 'an input was written'
        if not with_outputs:
            for s in (s_line, s_cnt):
                c = s.bits()
                assert bool((c == c[0]).all()), 'an output given as NULL was written'
        return {'records_out': (s_out, 1), **({'line': (s_line, 1), 'counts': (s_cnt, L + 1)} if with_outputs else {})}

    for attempt in range(2):                                             # the second round: the same bits again
        got = guarded_runs(run, 'las_label_records', batch=False)
        out = got['records_out'].numpy()[0]
        assert np.array_equal(out[:n * rl].reshape(n, rl), want) and np.array_equal(out[n * rl:], flat[n * rl:])
        if with_outputs:
            assert np.array_equal(got['line'].numpy()[0], want_line)
            counts = np.ascontiguousarray(got['counts'].numpy()).view(np.int64)[:, 0]
            assert counts[1:].tolist() == np.bincount(want_line, minlength=L + 1)[1:].tolist()
            assert counts[0] == int((_passes(rec, fmt, sel) & (want_line == 0)).sum())


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_the_argument_and_write_nothing(dev, tmp_path):
    seg = _scene()[0]
    index = ops.line_index(seg, lr.HW, device=dev)
    n = 300
    rec0, flat0 = _records(tmp_path, 1, 0, n, seed=1)
    rec6, flat6 = _records(tmp_path, 6, 0, n, seed=2)
    d0, d6 = torch.from_numpy(flat0).to(dev), torch.from_numpy(flat6).to(dev)
    ok = MarkingLabels(lr.HW, lr.ZTOL)
    L = lib()

    def refused(what, rc, outs):
        torch.cuda.synchronize()
        msg = L.lm_last_error().decode()
        assert rc == 1 and what in msg, f'{what}: rc={rc}, message {msg!r}'
        d_out, line, counts = outs
        assert bool((d_out == 0xA5).all()) and bool((line == 0x7EADBEEF).all()) and bool((counts == -1).all()), f'{what}: an output was written'

    def records(what, d_rec=d0, rl=28, fmt=1, index=index, Ln=5, labels=ok, cls=None, **kw):
        cls = 31 if cls is None and not 0 <= fmt <= 10 else cls
        rc, *outs = _label_call(dev, d_rec, rl, fmt, n, index, Ln, labels, cls=cls, **kw)
        refused(what, rc, outs)

    records('marking_class', cls=32)                                      # formats 0-5 hold five bits
    records('marking_class', d_rec=d6, rl=30, fmt=6, cls=256)
    rc, *outs = _label_call(dev, d6, 30, 6, n, index, 5, ok, cls=255)      # (255 fits format 6)
    assert rc == 0, L.lm_last_error()
    records('write_line_id', Ln=65536)
    rc, *outs = _label_call(dev, d0, 28, 1, n, index, 65536, MarkingLabels(lr.HW, lr.ZTOL, line_ids=False))
    assert rc == 0, L.lm_last_error()
    records('segments', Ln=4)                                             # the segments carry line 5
    records('record_len', rl=27)                                          # format 1 needs 28
    records('record_len', rl=161)
    records('point_format', fmt=11)
    records('point_format', fmt=-1)
    # NaN / negative half_width and z_tol: past the Python class, straight at the entry
    d3 = lambda v: (C.c_double * 3)(*[float(x) for x in v])
    for what, hw, zt in (('half_width', NAN, 0.5), ('half_width', -0.1, 0.5), ('z_tol', lr.HW, NAN), ('z_tol', lr.HW, -1.0)):
        d_out, line, counts = torch.full_like(d0, 0xA5), torch.full((n,), 0x7EADBEEF, dtype=torch.int32, device=dev), torch.full((6,), -1, dtype=torch.int64, device=dev)
        a = list(index.args())
        a[5] = hw
        rc = L.lm_las_label_records(_stream(dev), C.c_void_p(d0.data_ptr()), 28, 1, n, d3(SCALE), d3(OFFSET), d3(lr.SHIFT), None, *a, zt, NAN, 31, 1,
                                    C.c_void_p(d_out.data_ptr()), C.c_void_p(line.data_ptr()), C.c_void_p(counts.data_ptr()), 5)
        refused(what, rc, (d_out, line, counts))
        d_pts = torch.zeros((n, 4), device=dev)
        lp, dp = torch.full((n,), 0x7EADBEEF, dtype=torch.int32, device=dev), torch.full((n,), -7.0, device=dev)
        rc = L.lm_label_points(_stream(dev), C.c_void_p(d_pts.data_ptr()), n, *a, zt, NAN, C.c_void_p(lp.data_ptr()), C.c_void_p(dp.data_ptr()))
        torch.cuda.synchronize()
        assert rc == 1 and what in L.lm_last_error().decode() and bool((lp == 0x7EADBEEF).all()) and bool((dp == -7.0).all()), what
    # misaligned buffers
    d_out, line, counts = torch.full_like(d0, 0xA5), torch.full((n + 1,), 0x7EADBEEF, dtype=torch.int32, device=dev), torch.full((7,), -1, dtype=torch.int64, device=dev)
    base = [_stream(dev), C.c_void_p(d0.data_ptr()), 28, 1, n, d3(SCALE), d3(OFFSET), d3(lr.SHIFT), None, *index.args(), lr.ZTOL, NAN, 31, 1,
            C.c_void_p(d_out.data_ptr()), C.c_void_p(line.data_ptr()), C.c_void_p(counts.data_ptr()), 5]
    # (each message names the one argument that is off: "records is not" does not occur in the message about records_out)
    for pos, what, by in ((1, 'records', 1), (19, 'records_out', 1), (20, 'line', 2), (21, 'counts', 4), (9, 'segments', 4),
                          (12, 'cell_start', 2), (13, 'cell_segs', 1)):
        a = list(base)
        a[pos] = C.c_void_p(a[pos].value + by)
        refused(f'las_label_records: {what} is not', L.lm_las_label_records(*a), (d_out, line[:n], counts[:6]))
    d_pts = torch.zeros((n + 1, 4), device=dev)
    lp, dp = torch.full((n + 1,), 0x7EADBEEF, dtype=torch.int32, device=dev), torch.full((n + 1,), -7.0, device=dev)
    pbase = [_stream(dev), C.c_void_p(d_pts.data_ptr()), n, *index.args(), lr.ZTOL, NAN, C.c_void_p(lp.data_ptr()), C.c_void_p(dp.data_ptr())]
    for pos, what, by in ((1, 'points_xyzi', 4), (11, 'line', 2), (12, 'dist2', 1), (3, 'segments', 8), (6, 'cell_start', 1), (7, 'cell_segs', 2)):
        a = list(pbase)
        a[pos] = C.c_void_p(a[pos].value + by)
        rc = L.lm_label_points(*a)
        torch.cuda.synchronize()
        assert rc == 1 and f'label_points: {what} is not' in L.lm_last_error().decode(), (what, L.lm_last_error())
        assert bool((lp == 0x7EADBEEF).all()) and bool((dp == -7.0).all()), f'{what}: an output was written'
    # a grid built for another table or half width
    other = ops.line_index(seg[:-1], lr.HW, device=dev)
    a = list(base)
    a[11] = C.byref(other.grid)
    refused('grid', L.lm_las_label_records(*a), (d_out, line[:n], counts[:6]))
    wide = ops.line_index(seg, 0.25, device=dev)
    a = list(base)
    a[11] = C.byref(wide.grid)
    refused('half_width', L.lm_las_label_records(*a), (d_out, line[:n], counts[:6]))
    with pytest.raises(ValueError, match='marking_class=32'):
        las_io.label_records(d0, {'point_format': 1, 'record_len': 28, 'n_points': n, 'scale': SCALE, 'offset': OFFSET}, index,
                             MarkingLabels(lr.HW, lr.ZTOL, marking_class=32))
    with pytest.raises(TypeError, match='LineIndex'):
        ops.label_points(torch.zeros((4, 4), device=dev), seg, lr.ZTOL)


# ------------------------------------------------------------------------------------------------ 7. Runner
def test_runner_strip_labels_its_input(dev, net, tmp_path):
    """The strip of tests/test_gpu_drape.py's Runner test (three overlapping 1152 x 1152 tiles over a climbing plane, one point at every
    pixel centre, six painted stripes) through Runner.infer_las_strip_to_map with label=MarkingLabels(): labelled/<name> has the input's
    size and header, its records are the patcher applied with the lines the call returned, params/labels.json agrees; the call without
    label= creates no labelled/ directory and writes the same merged.txt bytes."""
    from lanemapping_amd.runner import Runner
    H = W = 1152
    reso, ele, A, Bs = 0.05, 0.05, 0.075, 0.02
    off = np.array([351200.0, 3433000.0, 12.0])
    step = 1024
    rows = 2 * step + H
    r, c = np.meshgrid(np.arange(rows), np.arange(W), indexing='ij')
    x, y = (r * reso).ravel(), (c * reso).ravel()
    lane_y = [(0.12 + 0.152 * l) * 57.6 + 0.01 * (l - 2.5) * x for l in range(6)]
    paint = np.zeros(len(x), bool)
    for ly in lane_y:
        paint |= np.abs(y - ly) < 0.075
    inten = np.where(paint, 24000.0, 3000.0 + 40.0 * ((r + 3 * c) % 97).ravel())
    world = np.stack([x, y, A * x + Bs * y], axis=1)
    order = np.random.RandomState(3).permutation(len(world))
    las = str(tmp_path / 'strip.las')
    las_ref.write_las(las, world[order] + off, inten[order], point_format=1, offset=tuple(off))
    prm_paths = []
    for t in range(3):
        p = {'coor_las_path': '', 'las_read_offset': list(off), 'las_rotation_trans_quan': [t * step * reso, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0],
             'bev_img_offset': [0.0, 0.0], 'img_reso': [reso, reso], 'local_min_ele': -0.5, 'ele_reso': ele}
        prm_paths.append(str(tmp_path / f'18102{t}_0209.txt'))
        io_utils.save_pc_2_img_transform_paras(prm_paths[t], p)
    rn = Runner.__new__(Runner)
    rn.cfg, rn.device, rn.net = net.cfg, dev, net
    assert rn.cfg.get('las_label') is None
    out = {k: str(tmp_path / k) for k in ('plain', 'label')}
    plain = rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['plain'], batch_size=2)
    labels = MarkingLabels()
    lines3d, merged = rn.infer_las_strip_to_map(las, prm_paths, work_dirs=out['label'], batch_size=2, label=labels)
    # the return value and every other output do not change
    assert sorted(plain[0]) == sorted(lines3d) and len(plain[1]) == len(merged) and all(np.array_equal(a, b) for a, b in zip(plain[1], merged))
    assert not os.path.exists(os.path.join(out['plain'], 'labelled')) and not os.path.exists(os.path.join(out['plain'], 'params', 'labels.json'))
    pc = os.path.join('out_pc_seq_json_dir', 'merged.txt')
    assert open(os.path.join(out['plain'], pc), 'rb').read() == open(os.path.join(out['label'], pc), 'rb').read()
    lines = list(merged) if len(merged) else [l for name in sorted(lines3d) for l in lines3d[name]]
    assert lines, 'the strip yielded no lines'
    data, got = np.fromfile(las, np.uint8), np.fromfile(os.path.join(out['label'], 'labelled', 'strip.las'), np.uint8)
    h = las_io.parse_header(data)
    o, rl, n = h['offset_to_points'], h['record_len'], h['n_points']
    assert len(got) == len(data) and np.array_equal(got[:o], data[:o])
    rec = data[o:o + n * rl].reshape(n, rl)
    seg = las_io.line_segments(lines, off)
    want_line = lr.label_f32_pruned(lr.decode_f32(rec, h['scale'], h['offset'], off), seg, labels.half_width, labels.z_tol)[0]
    assert np.array_equal(got[o:o + n * rl].reshape(n, rl), lr.patch_records(rec, 1, want_line, 31, True)), 'records differ from the patcher'
    assert np.array_equal(got[o + n * rl:], data[o + n * rl:])
    used = json.load(open(os.path.join(out['label'], 'params', 'labels.json')))
    per_line = np.bincount(want_line, minlength=len(lines) + 1)[1:].tolist()
    assert used == {'strip.las': [n, int((want_line > 0).sum()), per_line]}
    print(f'{len(lines)} lines, {len(seg)} segments, {int((want_line > 0).sum())} of {n} records labelled')
    assert (want_line > 0).sum() > 0, 'no record was labelled: the test shows nothing'
