"""GPU: paint thresholds per line and station window (include/lanemap_hip.h: lm_las_line_hist_window_records and the five _local entries;
las_io.hist_window_records / hist_window_files / paint_table, the stage passes with a las_io.PaintTable, Runner `threshold=` with
scope='line' and 'window').

The reference is tests/local_ref.py: the winner of label_ref.label_f32 without a min_intensity, the row from profile_ref.point_terms with
bin = window, the float32 test against thr[row], and the accumulators of the existing references.  Every integer and bit is compared.

The entries take their stream LAST (include/lanemap_hip.h says why), so the harnesses that find entries by a leading stream do not see
them.  Their cases are here: guarded buffers around every operand, table members included (5), poisoned LDS before the record kernels
(5, through guarded_runs), a side stream and graph replay (6)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import colour_ref as co
import cross_ref as cr
import label_ref as lr
import lds_state
import local_ref as lo
import profile_ref as pr
import residue_ref as rr
import test_gpu_cross as tc
import test_gpu_threshold as tt
import threshold_ref as tr
from guards import CANARY, Slab, _signed, guarded_runs
from lanemapping_amd import las_io, ops
from lanemapping_amd._lib import LmPaintTable, lib
from lanemapping_amd.las_io import CrossSection, MarkingLabels, MarkingSurvey, PaintResidue, PaintTable, PaintThreshold, PointFilter

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float('nan')
POISON = -7
HW, ZTOL = lr.HW, lr.ZTOL                       # 0.15625 m, 0.5 m: hq = 160
WINDOW = 8.0                                   # exact in float32, and so is 1 / 8: a station of 8, 16, ... m lies exactly on a seam
BIN, LQ, RQ, SH, BLUE_Q, CLEAR, CELL = 0.25, 32, 32, 6, 768, 0.0625, 0.1
L = 6                                          # label_ref.scene_lines: line 6 has one vertex and no segment
SCALE, OFFSET, ZERO = (1 / 1024, 1 / 1024, 1 / 1024), (0.0, 0.0, 0.0), np.zeros(3)
RECORD_LEN = {0: 20, 6: 30, 7: 36}
ENTRIES = ('label', 'profile', 'colour', 'cross', 'residue', 'hist')
SELECT = PointFilter(classes=[2], drop_withheld=False)


# ------------------------------------------------------------------------------------------------ the scene
@functools.lru_cache(maxsize=None)
def _scene():
    """label_ref's scene (six lines, the zero-length segment of line 5 included; about 3,000 points) with the table's own special points
    in front.  Windows of 8 m: lines 1, 2 and 4 (40 m) own five, line 3 (13.5 m) two, line 5 (4 m, shorter than a window) one, line 6
    none.  -> (lines, seg, pts, stations, win_start, thr, special) with thr [13 + 5] drawn inside the scene's intensities (0 .. 1999)."""
    lines = lr.scene_lines()
    seg = las_io.line_segments(lines, None)
    st, ws = las_io.line_stations(lines, None, WINDOW)
    assert ws.tolist() == [0, 5, 10, 12, 17, 18, 18]
    thr = np.array([300, 1000, 700, 1500, 500,  900, 400, 1999, 0, 1200,  800, 400,  1000, 1000, 1000, 1000, 1000,  650], f32)
    P, special = [], {}

    def add(name, x, y, z, i):
        special[name] = len(P)
        P.append((x, y, z, i))

    # line 1 lies at y = 2 and climbs 1 %; its vertices are 2 m apart, so x = 8, 16, ... are shared vertices: the segment before wins, t = 1
    for k, x in enumerate((8.0, 16.0, 24.0, 32.0)):                        # st = x exactly: the first station of window k + 1
        add(f'seam{k + 1}_eq', x, 2.0, 0.01 * x, float(thr[k + 1]))          # equal to the threshold of the window it opens: passes
        add(f'seam{k + 1}_below', x, 2.0, 0.01 * x, float(thr[k + 1]) - 1.0)
        add(f'before{k + 1}_eq', x - 1 / 1024, 2.0, 0.01 * x, float(thr[k]))  # one lattice step before the seam: the window before
        add(f'before{k + 1}_below', x - 1 / 1024, 2.0, 0.01 * x, float(thr[k]) - 1.0)
    add('end_eq', 40.0, 2.0, 0.4, float(thr[4]))                            # st = 40 = 5 x 8: clamped into the last window, 4
    add('end_below', 40.0, 2.0, 0.4, float(thr[4]) - 1.0)
    add('past_end', 40.0625, 2.0, 0.4, float(thr[4]))                       # t clamped to 1
    add('nan_i', 20.0, 2.0, 0.2, NAN)
    add('short_eq', 31.0, 9.0, 0.31, float(thr[17]))                        # line 5, one window shorter than 8 m
    add('short_below', 31.0, 9.0, 0.31, float(thr[17]) - 1.0)
    add('zero_thr', 6.5, 5.5, 0.065, 0.0)                                   # line 2, window 0 ... thr[5] = 900: fails; see 'zero_row'
    add('zero_row', 25.0, 5.5, 0.25, 0.0)                                   # line 2, window 3: thr[8] = 0, intensity 0 passes
    pts = np.concatenate([np.asarray(P, f32), lr.scene_points(seg)])
    for a in (seg, pts, st, ws, thr):
        a.setflags(write=False)
    return lines, seg, pts, st, ws, thr, special


THR_MIN = 0.0                                  # min(thr) of the scene's table


def _t(a):
    return torch.from_numpy(np.array(a, copy=True))


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def _handle(stream):
    return C.c_void_p(stream.cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


@functools.lru_cache(maxsize=None)
def _finite_points():
    """The scene's points a LAS record can hold: finite coordinates inside the int32 lattice of 1/1024 m and a whole intensity."""
    pts = _scene()[2]
    ok = np.isfinite(pts).all(axis=1) & (np.abs(pts[:, :3]) < 1e5).all(axis=1)
    return np.array(pts[ok], copy=True)


@functools.lru_cache(maxsize=None)
def _records(fmt, extra, n, seed=0):
    """n records of point format fmt, `extra` bytes longer than the format's minimum: the first n storable points of the scene (seed 0) or
    a permutation's (seed > 0) on the 1/1024 m lattice; classification 2 for four records of five and 7 for the fifth; format 7 with a
    colour triple; every other byte a pattern.  -> (rec [n, rl] uint8, the flat copy padded to a multiple of 4 for the device, rgb or None)."""
    src = _finite_points()
    if seed:
        src = src[np.random.RandomState(seed).permutation(len(src))]
    src = src[:n]
    assert len(src) == n
    rl = RECORD_LEN[fmt] + extra
    rec = np.zeros((n, rl), np.uint8)
    rec[:, 14:] = (np.arange(n)[:, None] * 7 + np.arange(rl - 14)[None, :] * 3) % 251
    q = np.round(src[:, :3].astype(np.float64) * 1024).astype('<i4')
    rec[:, 0:12] = q.view(np.uint8).reshape(n, 12)
    rec[:, 12:14] = np.clip(src[:, 3], 0, 65535).astype('<u2').reshape(n, 1).view(np.uint8)
    cls = np.where(np.arange(n) % 5 == 4, 7, 2)
    if fmt >= 6:
        rec[:, 16] = cls
    else:
        rec[:, 15] = (rec[:, 15] & 0xE0) | cls
    rgb = None
    if fmt == 7:
        rng = np.random.RandomState(77 + n + seed)
        rgb = rng.randint(0, 65536, (n, 3))
        rgb[rng.rand(n) < 0.2] = 0                                          # black: no camera saw the point
        rgb[rng.rand(n) < 0.3, 2] //= 4                                     # yellowish
        co.put_rgb(rec, fmt, rgb)
    flat = np.zeros((n * rl + 3) // 4 * 4, np.uint8)
    flat[:n * rl] = rec.reshape(-1)
    rec.setflags(write=False), flat.setflags(write=False)
    return rec, flat, rgb


def _decoded(rec):
    return lr.decode_f32(rec, SCALE, OFFSET, ZERO)


class Ctx:
    """The device tables of the scene: the index, the stations cut per entry (BIN for the tables with station bins, WINDOW for the
    windows), and the paint table."""

    def __init__(self, dev, thr=None, window=WINDOW, thr_min=None):
        lines, seg, _, _, _, scene_thr, _ = _scene()
        self.dev, self.window = dev, window
        self.index = ops.line_index(seg, HW, device=dev)
        self.st_bin = ops.line_stations(*las_io.line_stations(lines, None, BIN), BIN, device=dev)
        self.st_win = ops.line_stations(*las_io.line_stations(lines, None, window), window, device=dev)
        self.ws = self.st_win.bin_start_host
        self.thr = np.asarray(scene_thr if thr is None else thr, f32)
        self.paint_iq = np.array([las_io.paint_iq_of(float(v)) for v in self.thr], np.int32)
        self.rows = ops.paint_rows(self.thr, self.ws, window, self.st_bin.stations, paint_iq=self.paint_iq)
        self.thr_min = float(self.thr.min()) if thr_min is None else thr_min
        self.grid = ops.residue_grid(self.index, CELL)
        self.nl = cr.hq_nl(HW, LQ)[1]
        self.Z, self.NB = tr.shape(HW, RQ, SH)[1:]

    def table(self, cross=False):
        t = self.rows.struct(cross)
        t.thr_min = self.thr_min
        return t


@functools.lru_cache(maxsize=None)
def _ctx(dev):
    return Ctx(dev)


def _out_spec(ctx, entry, n, rl=0):
    """name -> (shape, dtype) of the outputs of an entry for n records (or points)."""
    nb = ctx.st_bin.n_bins
    return {'label': {'records_out': (((n * rl + 3) // 4 * 4,), torch.uint8), 'line': ((n,), torch.int32), 'counts': ((L + 1,), torch.int64)},
            'profile': {'bins': ((nb, 6), torch.int64)},
            'colour': {'bins': ((nb, 6), torch.int64), 'colours': ((nb, 6), torch.int64)},
            'cross': {'cells': ((nb, ctx.nl, 4), torch.int64)},
            'residue': {'key': ((n,), torch.int64), 'iq': ((n,), torch.int32)},
            'hist': {'hist': ((int(ctx.ws[-1]), ctx.Z, ctx.NB), torch.int64)}}[entry]


def _call(ctx, entry, src, rl, fmt, n, select, outs, stream, accumulate=0, table=None, P=None):
    """One call of an entry through the library object.  src: the device records (the residue entry: the device points); outs: name ->
    a C pointer or None; table: an LmPaintTable (default: the scene's); P: pointers replacing the device tables' (guarded slabs).  -> rc."""
    Lb = lib()
    P = P or {}
    ia = list(ctx.index.args())
    for k, pos in (('segments', 0), ('cell_start', 3), ('cell_segs', 4)):
        if k in P:
            ia[pos] = P[k]
    sa = list((ctx.st_win if entry == 'hist' else ctx.st_bin).args())
    if 'stations' in P:
        sa[0] = P['stations']
    if 'bin_start' in P:
        sa[1] = P['bin_start']
    sel = select.as_struct() if select is not None else None
    head = (src, rl, fmt, n, _d3(SCALE), _d3(OFFSET), None, C.byref(sel) if sel is not None else None, *ia)
    t = table if table is not None else ctx.table(cross=entry == 'cross')
    tp = C.byref(t) if t is not False else None
    o = outs
    if entry == 'label':
        return Lb.lm_las_label_records_local(*head, ZTOL, tp, 31 if fmt < 6 else 64, 1, o['records_out'], o['line'], o['counts'], L, stream)
    if entry == 'profile':
        return Lb.lm_las_line_profile_records_local(*head, *sa, ZTOL, tp, accumulate, o['bins'], ctx.st_bin.n_bins, stream)
    if entry == 'colour':
        return Lb.lm_las_line_colour_records_local(*head, *sa, ZTOL, tp, BLUE_Q, accumulate, o['bins'], o['colours'], ctx.st_bin.n_bins, stream)
    if entry == 'cross':
        return Lb.lm_las_line_cross_records_local(*head, *sa, ZTOL, LQ, tp, accumulate, o['cells'], ctx.st_bin.n_bins * ctx.nl, stream)
    if entry == 'residue':
        g = ctx.grid
        return Lb.lm_residue_keys_local(src, n, *ia, ZTOL, tp, L, CLEAR, g['cell'], g['nx'], g['ny'], o['key'], o['iq'], stream)
    R = int(ctx.ws[-1])
    return Lb.lm_las_line_hist_window_records(*head, sa[0], L, ZTOL, RQ, SH, accumulate, o['hist'], R * ctx.Z * ctx.NB,
                                              P.get('win_start', sa[1]), sa[2], ctx.window, stream)


def _want(ctx, entry, rec, fmt, select, pts=None, prev=None, thr=None, thr_min=None, window=None):
    """The brute force of an entry on records (the residue entry: on points): name -> numpy array.  prev: what to add to."""
    _, seg, _, _, _, _, _ = _scene()
    thr = ctx.thr if thr is None else thr
    thr_min = ctx.thr_min if thr_min is None else thr_min
    window = ctx.window if window is None else window
    st = ctx.st_win.stations.cpu().numpy()
    ws, bs = ctx.ws, ctx.st_bin.bin_start_host
    if entry == 'residue':
        key, iq = lo.residue_local(pts, seg, st, ws, window, thr, thr_min, HW, ZTOL, CLEAR, ctx.grid)
        return {'key': key, 'iq': iq}
    dec = _decoded(rec)
    mask = tc._passes(rec, fmt, select)
    prev = prev or {}
    if entry == 'label':
        line = lo.label_local(dec, seg, st, ws, window, thr, thr_min, HW, ZTOL, mask)[0]
        out = lr.patch_records(rec, fmt, line, 31 if fmt < 6 else 64, True)
        flat = np.zeros((out.size + 3) // 4 * 4, np.uint8)
        flat[:out.size] = out.reshape(-1)
        counts = np.bincount(line[line > 0], minlength=L + 1).astype(np.int64)
        counts[0] = int((mask & (line == 0)).sum())
        return {'records_out': flat, 'line': line.astype(np.int32), 'counts': counts}
    if entry == 'profile':
        return {'bins': lo.profile_local(dec, seg, st, bs, BIN, ws, window, thr, thr_min, HW, ZTOL, mask, prev.get('bins'))[0]}
    if entry == 'colour':
        b, c = lo.colour_local(dec, co.get_rgb(rec, fmt), seg, st, bs, BIN, ws, window, thr, thr_min, HW, ZTOL, BLUE_Q, mask, prev.get('bins'),
                               prev.get('colours'))
        return {'bins': b, 'colours': c}
    if entry == 'cross':
        piq = np.array([las_io.paint_iq_of(float(v)) for v in thr], np.int64)
        return {'cells': lo.cross_local(dec, seg, st, bs, BIN, ws, window, piq, HW, ZTOL, LQ, mask, prev.get('cells'))}
    return {'hist': lo.hist_window_f32(dec, seg, st, ws, window, HW, ZTOL, RQ, SH, mask, prev.get('hist'))[0]}


def _poisoned(shape, dt, dev):
    return torch.full(shape, 0xF9 if dt == torch.uint8 else POISON, dtype=dt, device=dev)


def _run(ctx, entry, src, rl, fmt, n, select=None, accumulate=0, into=None, **kw):
    """-> name -> device tensor: the entry run on the current stream into fresh poisoned outputs (or `into`)."""
    outs = into or {k: _poisoned(shape, dt, ctx.dev) for k, (shape, dt) in _out_spec(ctx, entry, n, rl).items()}
    rc = _call(ctx, entry, _ptr(src), rl, fmt, n, select, {k: _ptr(v) for k, v in outs.items()}, _handle(torch.cuda.current_stream(ctx.dev)),
               accumulate, **kw)
    assert rc == 0, lib().lm_last_error()
    return outs


def _same(tag, got, want):
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for k in want:
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else np.asarray(got[k])
        w = np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, f'{tag} [{k}]: {g.dtype} {g.shape}, expected {w.dtype} {w.shape}'
        bad = np.argwhere(g != w)
        assert not len(bad), (f'{tag} [{k}]: {len(bad)} values differ from the brute force; first at {bad[0].tolist()}: '
                              f'{g[tuple(bad[0])]} != {w[tuple(bad[0])]}')


# ------------------------------------------------------------------------------------------------ 0. the scene
def test_the_scene_holds_what_it_is_meant_to_hold():
    """No GPU work: the reference puts the special points where the rule says, so the comparisons below mean what they claim."""
    lines, seg, pts, st, ws, thr, S = _scene()
    line, d2, win, row, ok = lo.label_local(pts, seg, st, ws, WINDOW, thr, THR_MIN, HW, ZTOL)
    plain = lo.winner(pts, seg, HW, ZTOL)[0]
    assert float(f32(1.0 / WINDOW)) == 0.125 and thr.min() == THR_MIN and len(thr) == ws[-1] == 18 and len(seg) == 20 + 20 + 2 + 20 + 3
    terms = pr.point_terms(pts, seg, st, ws, WINDOW, plain, win)
    for k in (1, 2, 3, 4):
        assert plain[S[f'seam{k}_eq']] == 1 and terms['st'][S[f'seam{k}_eq']] == 8.0 * k and row[S[f'seam{k}_eq']] == k, 'on the seam: the window it opens'
        assert ok[S[f'seam{k}_eq']] and not ok[S[f'seam{k}_below']] and row[S[f'seam{k}_below']] == k
        assert row[S[f'before{k}_eq']] == k - 1 and ok[S[f'before{k}_eq']] and not ok[S[f'before{k}_below']]
    assert terms['st'][S['end_eq']] == 40.0 and row[S['end_eq']] == 4 and ok[S['end_eq']] and not ok[S['end_below']], 'the last-window clamp'
    assert terms['t'][S['past_end']] == 1.0 and row[S['past_end']] == 4 and ok[S['past_end']]
    assert plain[S['nan_i']] == 1 and row[S['nan_i']] == 2 and not ok[S['nan_i']] and line[S['nan_i']] == 0, 'a NaN intensity fails'
    assert plain[S['short_eq']] == 5 and row[S['short_eq']] == 17 and ok[S['short_eq']] and not ok[S['short_below']]
    assert plain[S['zero_thr']] == 2 and row[S['zero_thr']] == 5 and not ok[S['zero_thr']]
    assert plain[S['zero_row']] == 2 and row[S['zero_row']] == 8 and ok[S['zero_row']], 'intensity 0 meets a threshold of 0'
    assert set(np.unique(row[row >= 0])) == set(range(18)) - set(), 'every row of the table is hit'
    passed = np.bincount(row[ok], minlength=18)
    failed = np.bincount(row[(row >= 0) & ~ok], minlength=18)
    assert (passed[thr < 1999] > 0).all() and (failed[thr > 0] > 0).all(), 'returns on both sides of every threshold'
    assert (plain > 0).sum() > 300 and 100 < (line > 0).sum() < (plain > 0).sum() - 100
    # a scalar threshold cannot give these labels: whatever T, some row disagrees
    for T in (0.0, 500.0, 1000.0):
        assert (lr.label_f32(pts, seg, HW, ZTOL, T)[0] != line).sum() > 20
    fin = _finite_points()
    assert len(fin) >= 1025 and len(S) < 255, 'the special points are in every file'


# ------------------------------------------------------------------------------------------------ 1. brute force
@pytest.mark.parametrize('entry, fmt, extra', [(e, f, x) for e in ('label', 'profile', 'cross', 'hist') for f, x in ((0, 0), (6, 3), (7, 1))] +
                         [('colour', 7, 1), ('colour', 7, 0)])
def test_record_entries_equal_the_brute_force(dev, entry, fmt, extra):
    """Formats 0, 6 and 7 (the colour entry: 7), an odd record length with extra bytes, with and without a select, 255, 256, 257 and 1025
    records (the block seams)."""
    ctx = _ctx(dev)
    rl = RECORD_LEN[fmt] + extra
    assert rl in (20, 33, 36, 37)
    for n in (255, 256, 257, 1025):
        rec, flat, _ = _records(fmt, extra, n)
        d_rec = _t(flat).to(dev)
        for name, select in (('plain', None), ('class 2 only', SELECT)):
            tag = f'{entry}, format {fmt}, {rl} B, n={n}, {name}'
            before = d_rec.clone()
            got = _run(ctx, entry, d_rec, rl, fmt, n, select)
            want = _want(ctx, entry, rec, fmt, select)
            _same(tag, got, want)
            assert torch.equal(d_rec, before), f'{tag}: the records were written'
            if entry == 'label':
                assert 10 < int((want['line'] > 0).sum()) < n and want['counts'].sum() == tc._passes(rec, fmt, select).sum()


def test_residue_keys_equal_the_brute_force(dev):
    """The points entry on the scene's points, NaN and infinite coordinates and the NaN intensity included, at the block seams."""
    ctx = _ctx(dev)
    pts = _scene()[2]
    for N in (255, 256, 257, 1025, len(pts)):
        got = _run(ctx, 'residue', _t(pts[:N]).to(dev), 0, 0, N)
        want = _want(ctx, 'residue', None, 0, None, pts=pts[:N])
        _same(f'residue_keys_local, N={N}', got, want)
    assert (want['key'] >= 0).sum() > 50 and (rr.keys_f32(pts, _scene()[1], HW, ZTOL, None, CLEAR, ctx.grid)[0] >= 0).sum() > (want['key'] >= 0).sum()
    iq_none = torch.full((len(pts),), POISON, dtype=torch.int64, device=dev)            # iq = NULL is allowed, as in the scalar entry
    rc = _call(ctx, 'residue', _ptr(_t(pts).to(dev)), 0, 0, len(pts), None, {'key': _ptr(iq_none), 'iq': None}, _handle(torch.cuda.current_stream(dev)))
    assert rc == 0 and np.array_equal(iq_none.cpu().numpy(), want['key'])


@pytest.mark.parametrize('entry', ['profile', 'colour', 'cross', 'hist'])
def test_accumulate_over_two_files_in_both_orders(dev, entry):
    ctx = _ctx(dev)
    fmt, extra = 7, 1
    rl = RECORD_LEN[fmt] + extra
    files = [(_records(fmt, extra, 700, seed=s), 700) for s in (3, 4)]
    want = None
    for (rec, _, _), n in files:
        want = _want(ctx, entry, rec, fmt, None, prev=want)
    results = []
    for order in ((0, 1), (1, 0)):
        outs = None
        for j, f in enumerate(order):
            (rec, flat, _), n = files[f]
            outs = _run(ctx, entry, _t(flat).to(dev), rl, fmt, n, None, accumulate=int(j > 0), into=outs)
        _same(f'{entry}, files in order {order}', outs, want)
        results.append(outs)
    first = _want(ctx, entry, files[0][0][0], fmt, None)
    assert any(not np.array_equal(first[k], want[k]) for k in want), 'the second file adds something'


# ------------------------------------------------------------------------------------------------ 2. identities
def _scalar_call(ctx, entry, src, rl, fmt, n, select, outs, T, stream):
    """The scalar entry of a stage with min_intensity (paint_iq) = T, on the same arguments."""
    Lb = lib()
    sel = select.as_struct() if select is not None else None
    head = (stream, src, rl, fmt, n, _d3(SCALE), _d3(OFFSET), None, C.byref(sel) if sel is not None else None, *ctx.index.args())
    sa, o = ctx.st_bin.args(), outs
    if entry == 'label':
        return Lb.lm_las_label_records(*head, ZTOL, T, 31 if fmt < 6 else 64, 1, o['records_out'], o['line'], o['counts'], L)
    if entry == 'profile':
        return Lb.lm_las_line_profile_records(*head, *sa, ZTOL, T, 0, o['bins'], ctx.st_bin.n_bins)
    if entry == 'colour':
        return Lb.lm_las_line_colour_records(*head, *sa, ZTOL, T, BLUE_Q, 0, o['bins'], o['colours'], ctx.st_bin.n_bins)
    if entry == 'cross':
        return Lb.lm_las_line_cross_records(*head, *sa, ZTOL, LQ, las_io.paint_iq_of(T), 0, o['cells'], ctx.st_bin.n_bins * ctx.nl)
    g = ctx.grid
    return Lb.lm_residue_keys(stream, src, n, *ctx.index.args(), ZTOL, T, CLEAR, g['cell'], g['nx'], g['ny'], o['key'], o['iq'])


@pytest.mark.parametrize('entry', ['label', 'profile', 'colour', 'cross', 'residue'])
def test_a_constant_table_equals_the_scalar_entry_bit_for_bit(dev, entry):
    """All rows T and thr_min = T: the scalar entry with min_intensity = T (the cross-sections: paint_iq of T in every row)."""
    fmt, extra, n = 7, 1, 1025
    rl = RECORD_LEN[fmt] + extra
    rec, flat, _ = _records(fmt, extra, n)
    pts = _scene()[2]
    src = _t(pts).to(dev) if entry == 'residue' else _t(flat).to(dev)
    if entry == 'residue':
        n, rl = len(pts), 0
    cur = _handle(torch.cuda.current_stream(dev))
    for T in (500.0, 1000.0, 0.0):
        ctx = Ctx(dev, thr=np.full(18, T, f32))
        for select in (None, SELECT) if entry != 'residue' else (None,):
            got = _run(ctx, entry, src, rl, fmt, n, select)
            ref = {k: _poisoned(shape, dt, dev) for k, (shape, dt) in _out_spec(ctx, entry, n, rl).items()}
            rc = _scalar_call(ctx, entry, _ptr(src), rl, fmt, n, select, {k: _ptr(v) for k, v in ref.items()}, T, cur)
            assert rc == 0, lib().lm_last_error()
            for k in ref:
                lds_state.assert_same_bits(got[k], ref[k], f'{entry} [{k}] with a constant table of {T} against the scalar entry')


def test_one_window_per_line_and_the_windows_summed_equal_the_line_histogram(dev):
    fmt, extra, n = 6, 3, 1025
    rl = RECORD_LEN[fmt] + extra
    rec, flat, _ = _records(fmt, extra, n)
    d_rec = _t(flat).to(dev)
    ctx = _ctx(dev)
    thr = PaintThreshold(half_width=HW, ring=RQ / 1024, inner=RQ / 1024, outer=0.125, z_tol=ZTOL, bin_shift=SH)
    assert (thr.ring_q, thr.rings, thr.n_counts) == (RQ, ctx.Z, ctx.NB)
    header = {'point_format': fmt, 'record_len': rl, 'n_points': n, 'scale': SCALE, 'offset': OFFSET}
    per_line = las_io.hist_records(d_rec, header, ctx.index, ctx.st_bin, thr)
    assert int(per_line.sum()) > 100
    whole = las_io.threshold_window(_scene()[0], None, thr._replace(scope='line'))
    assert whole == 80.0
    one = Ctx(dev, thr=np.zeros(5, f32), window=whole)
    assert one.ws.tolist() == [0, 1, 2, 3, 4, 5, 5]
    got = las_io.hist_window_records(d_rec, header, one.index, one.st_win, thr)
    assert tuple(got.shape) == (5, ctx.Z, ctx.NB)
    lds_state.assert_same_bits(got, per_line[:5], 'one window per line against lm_las_line_hist_records')
    assert not bool(per_line[5].any())
    win = las_io.hist_window_records(d_rec, header, ctx.index, ctx.st_win, thr)
    _same('hist_window_records', {'hist': win}, _want(ctx, 'hist', rec, fmt, None))
    summed = las_io.line_hist_of_windows(win.cpu().numpy(), ctx.ws)
    assert np.array_equal(summed, per_line.cpu().numpy()), 'the windows of a line summed are its histogram'
    again = las_io.hist_window_records(d_rec, header, ctx.index, ctx.st_win, thr, out=win)
    assert again.data_ptr() == win.data_ptr() and np.array_equal(las_io.line_hist_of_windows(again.cpu().numpy(), ctx.ws), 2 * summed)


# ------------------------------------------------------------------------------------------------ 3. edge sizes
@pytest.mark.parametrize('entry', ENTRIES)
def test_edge_sizes_are_ok_after_the_initialisation(dev, entry):
    """n = 0, S = 0 and n_rows = 0 are LM_OK; the accumulating tables read as initialised, every label is 0 and every key -1."""
    ctx = _ctx(dev)
    fmt, extra, n = 7, 1, 300
    rl = RECORD_LEN[fmt] + extra
    rec, flat, _ = _records(fmt, extra, n)
    pts = _scene()[2][:n]
    src = _t(pts).to(dev) if entry == 'residue' else _t(flat).to(dev)
    rl_e = 0 if entry == 'residue' else rl

    def empty(outs, n_out, what):
        for k, v in outs.items():
            v = v.cpu().numpy()
            if k == 'bins':
                assert np.array_equal(v, las_io._empty_bins(ctx.st_bin.bin_start_host)), (what, k)
            elif k == 'key':
                assert (v[:n_out] == -1).all(), (what, k)
            elif k == 'records_out':
                assert np.array_equal(v[:n_out * rl], flat[:n_out * rl]), (what, k)
            elif k == 'counts':
                assert v[1:].sum() == 0 and v[0] == n_out, (what, k)
            elif k in ('line', 'iq'):
                assert not v[:n_out].any(), (what, k)
            else:
                assert not v.any(), (what, k)

    # n = 0
    outs = _run(ctx, entry, src, rl_e, fmt, 0)
    for k, v in outs.items():
        if k in ('records_out', 'line', 'key', 'iq'):
            assert v.numel() == 0
    empty({k: v for k, v in outs.items() if k not in ('records_out', 'line', 'key', 'iq')}, 0, 'n = 0')
    # n_rows = 0: every line without a window - nothing passes; the cross-sections still count every return, none of them paint
    none = Ctx.__new__(Ctx)
    none.__dict__.update(ctx.__dict__)
    none.thr, none.thr_min = np.zeros(0, f32), 0.0
    none.rows = ops.paint_rows(np.zeros(0, f32), np.zeros(L + 1, np.int32), WINDOW, ctx.st_bin.stations, paint_iq=np.zeros(0, np.int32))
    none.ws = none.rows.win_start_host
    if entry == 'hist':
        rc = lib().lm_las_line_hist_window_records(_ptr(src), rl, fmt, n, _d3(SCALE), _d3(OFFSET), None, None, *ctx.index.args(),
                                                   ctx.st_win.args()[0], L, ZTOL, RQ, SH, 0, None, 0, _ptr(none.rows.win_start),
                                                   C.c_void_p(none.ws.ctypes.data), WINDOW, _handle(torch.cuda.current_stream(dev)))
        assert rc == 0, lib().lm_last_error()
    else:
        outs = _run(none, entry, src, rl_e, fmt, n)
        if entry == 'cross':
            scalar = {k: _poisoned(s, dt, dev) for k, (s, dt) in _out_spec(ctx, entry, n, rl).items()}
            rc = lib().lm_las_line_cross_records(_handle(torch.cuda.current_stream(dev)), _ptr(src), rl, fmt, n, _d3(SCALE), _d3(OFFSET), None, None,
                                                 *ctx.index.args(), *ctx.st_bin.args(), ZTOL, LQ, 65536, 0, _ptr(scalar['cells']), ctx.st_bin.n_bins * ctx.nl)
            assert rc == 0 and torch.equal(outs['cells'], scalar['cells']) and int(outs['cells'][..., 0].sum()) > 50 and not bool(outs['cells'][..., 1].any())
        else:
            empty(outs, n, 'n_rows = 0')
    # S = 0: a line of one vertex alone
    lone = [lr.scene_lines()[5]]
    idx0 = ops.line_index(np.zeros((0, 8), f32), HW, device=dev)
    st0 = ops.line_stations(*las_io.line_stations(lone, None, BIN), BIN, device=dev)
    sw0 = ops.line_stations(*las_io.line_stations(lone, None, WINDOW), WINDOW, device=dev)
    assert st0.n_bins == 0 and sw0.bin_start_host.tolist() == [0, 0]
    s0 = Ctx.__new__(Ctx)
    s0.__dict__.update(ctx.__dict__)
    s0.index, s0.st_bin, s0.st_win, s0.ws = idx0, st0, sw0, sw0.bin_start_host
    s0.rows = ops.paint_rows(np.zeros(0, f32), sw0.bin_start_host, WINDOW, st0.stations, paint_iq=np.zeros(0, np.int32))
    s0.grid = ops.residue_grid(idx0, CELL)
    Lb = lib()
    cur = _handle(torch.cuda.current_stream(dev))
    t = s0.table(cross=entry == 'cross')
    sel_head = (_ptr(src), rl, fmt, n, _d3(SCALE), _d3(OFFSET), None, None, *idx0.args())
    if entry == 'label':
        out = {k: _poisoned(s, dt, dev) for k, (s, dt) in _out_spec(ctx, entry, n, rl).items()}
        out['counts'] = torch.full((2,), POISON, dtype=torch.int64, device=dev)
        rc = Lb.lm_las_label_records_local(*sel_head, ZTOL, C.byref(t), 64, 1, _ptr(out['records_out']), _ptr(out['line']), _ptr(out['counts']), 1, cur)
        assert rc == 0, Lb.lm_last_error()
        assert np.array_equal(out['records_out'].cpu().numpy(), flat) and not bool(out['line'].any()) and out['counts'].tolist() == [n, 0]
    elif entry == 'residue':
        out = {k: _poisoned(s, dt, dev) for k, (s, dt) in _out_spec(ctx, entry, n).items()}
        rc = Lb.lm_residue_keys_local(_ptr(src), n, *idx0.args(), ZTOL, C.byref(t), 1, CLEAR, CELL, 0, 0, _ptr(out['key']), _ptr(out['iq']), cur)
        assert rc == 0, Lb.lm_last_error()
        assert bool((out['key'] == -1).all()) and not bool(out['iq'].any())
    elif entry == 'hist':
        rc = Lb.lm_las_line_hist_window_records(*sel_head, None, 1, ZTOL, RQ, SH, 0, None, 0, _ptr(sw0.bin_start), C.c_void_p(s0.ws.ctypes.data), WINDOW, cur)
        assert rc == 0, Lb.lm_last_error()
    else:
        tail = {'profile': (ZTOL, C.byref(t), 0, None, 0, cur), 'colour': (ZTOL, C.byref(t), BLUE_Q, 0, None, None, 0, cur),
                'cross': (ZTOL, LQ, C.byref(t), 0, None, 0, cur)}[entry]
        fn = {'profile': Lb.lm_las_line_profile_records_local, 'colour': Lb.lm_las_line_colour_records_local,
              'cross': Lb.lm_las_line_cross_records_local}[entry]
        assert fn(*sel_head, *st0.args(), *tail) == 0, Lb.lm_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. refusals
@pytest.mark.parametrize('entry', ENTRIES)
def test_refusals_name_the_argument_and_write_nothing(dev, entry):
    """Every refusal of the table's members, by name, with the outputs between guard slabs: no word of them changes."""
    ctx = _ctx(dev)
    fmt, extra, n = 7, 1, 300
    rl = RECORD_LEN[fmt] + extra
    rec, flat, _ = _records(fmt, extra, n)
    src = _t(_scene()[2][:n]).to(dev) if entry == 'residue' else _t(flat).to(dev)
    rl_e = 0 if entry == 'residue' else rl
    cur = _handle(torch.cuda.current_stream(dev))
    W = {torch.int64: (2, torch.int32), torch.int32: (1, torch.int32), torch.uint8: (1, torch.uint8)}
    slabs = {}
    for k, (shape, dt) in _out_spec(ctx, entry, n, rl).items():
        words, sdt = W[dt]
        slabs[k] = Slab(dev, int(np.prod(shape)), words, front=16, back=16, dtype=sdt).fill_canary()
    outs = {k: C.c_void_p(s.ptr()) for k, s in slabs.items()}
    name = {'label': 'las_label_records_local', 'profile': 'las_line_profile_records_local', 'colour': 'las_line_colour_records_local',
            'cross': 'las_line_cross_records_local', 'residue': 'residue_keys_local', 'hist': 'las_line_hist_window_records'}[entry]

    def untouched(what):
        torch.cuda.synchronize()
        for k, s in slabs.items():
            assert bool((s.bits() == _signed(CANARY[s.dtype], s.dtype)).all()), f'{name}, {what}: {k} was written'

    def refused(what, **kw):
        rc = _call(ctx, entry, _ptr(src), rl_e, fmt, n, None, outs, cur, **kw)
        msg = lib().lm_last_error().decode()
        assert rc == 1 and msg.startswith(name + ':') and what in msg, f'{name}, {what}: rc={rc}, message {msg!r}'
        untouched(what)

    if entry == 'hist':
        ws_dev, ws_host = ctx.st_win.bin_start, ctx.ws
        refused('win_start is not 4-byte aligned', P={'win_start': C.c_void_p(ws_dev.data_ptr() + 2)})
        refused('null pointer (win_start)', P={'win_start': None})
        for bad, what in ((np.array([0, 5, 10, 12, 17, 18, 17], np.int32), 'win_start[6]=17 is below'), (np.array([1, 5, 10, 12, 17, 18, 18], np.int32), 'win_start[0]=1'),
                          (np.array([0, 5, 10, 12, 17, 18, 19], np.int32), 'n_hist')):
            saved = ctx.st_win.bin_start_host
            ctx.st_win.bin_start_host = bad
            try:
                refused(what)
            finally:
                ctx.st_win.bin_start_host = saved
        for w, what in ((0.0, 'window=0'), (-1.0, 'window=-1'), (float('inf'), 'window=inf'), (NAN, 'window=nan')):
            saved, ctx.window = ctx.window, w
            try:
                refused(what)
            finally:
                ctx.window = saved
        big = np.array([0, 30000, 60000, 60001, 60002, 60003, 60003], np.int32)      # 60003 x 6 x 1024 > 2^27: refused by n_hist's name
        assert 60003 * ctx.Z * ctx.NB > 1 << 27
        saved = ctx.st_win.bin_start_host
        ctx.st_win.bin_start_host = big
        try:
            refused('at most 2^27')
            assert 'n_hist' in lib().lm_last_error().decode()
        finally:
            ctx.st_win.bin_start_host = saved
        # and the run that is not refused writes the whole table and nothing else
        assert _call(ctx, entry, _ptr(src), rl_e, fmt, n, None, outs, cur) == 0, lib().lm_last_error()
        torch.cuda.synchronize()
        slabs['hist'].check_canary(name)
        return

    def table(**change):
        t = ctx.table(cross=entry == 'cross')
        for k, v in change.items():
            setattr(t, k, v)
        return t

    member = 'paint_iq' if entry == 'cross' else 'thr'
    other = 'thr' if entry == 'cross' else 'paint_iq'
    refused('null pointer (table)', table=False)
    refused(f'null pointer (table.{member})', table=table(**{member: None}))
    refused(f'table.{member} is not 4-byte aligned', table=table(**{member: getattr(ctx.rows, member).data_ptr() + 2}))
    if entry == 'cross':
        refused('null pointer (table.paint_iq): the cross-sections read it', table=table(paint_iq=None))
    else:
        refused('table.paint_iq is given, but only the cross-sections read it', table=table(paint_iq=ctx.rows.paint_iq.data_ptr()))
    refused('null pointer (table.win_start, table.stations)', table=table(win_start=None))
    refused('null pointer (table.win_start, table.stations)', table=table(stations=None))
    refused('table.win_start is not 4-byte aligned', table=table(win_start=ctx.rows.win_start.data_ptr() + 1))
    refused('table.stations is not 16-byte aligned', table=table(stations=ctx.rows.stations.data_ptr() + 8))
    refused('null pointer (table.win_start_host)', table=table(win_start_host=None))
    refused('table.n_rows=17, but table.win_start[L]=18', table=table(n_rows=17))
    refused('table.n_rows=19', table=table(n_rows=19))
    down = np.array([0, 5, 10, 12, 17, 18, 17], np.int32)
    refused('table.win_start[6]=17 is below table.win_start[5]=18', table=table(win_start_host=down.ctypes.data, n_rows=17))
    from1 = np.array([1, 5, 10, 12, 17, 18, 18], np.int32)
    refused('table.win_start[0]=1 must be 0', table=table(win_start_host=from1.ctypes.data))
    for w, what in ((0.0, 'table.window=0'), (-8.0, 'table.window=-8'), (float('inf'), 'table.window=inf'), (NAN, 'table.window=nan')):
        refused(what, table=table(window=w))
    for m, what in ((float('inf'), 'table.thr_min=inf'), (-float('inf'), 'table.thr_min=-inf'), (NAN, 'table.thr_min=nan')):
        refused(what, table=table(thr_min=m))
    if entry == 'colour':
        r0, f0, _ = _records(0, 0, n)
        rc = _call(ctx, entry, _ptr(_t(f0).to(dev)), 20, 0, n, None, outs, cur)
        assert rc == 1 and 'carries no RGB' in lib().lm_last_error().decode()
        untouched('a format without colour')
    # what the scalar entry refuses is still refused, under the new name
    wide = ops.line_index(_scene()[1], 0.25, device=dev)
    saved, ctx.index = ctx.index, ops.LineIndex(wide.segments, wide.cell_start, wide.cell_segs, wide.grid, np.float32(HW))
    try:
        refused('grid was built for half_width=0.25')
    finally:
        ctx.index = saved
    # and the run that is not refused writes all of every output and nothing else
    assert _call(ctx, entry, _ptr(src), rl_e, fmt, n, None, outs, cur) == 0, lib().lm_last_error()
    torch.cuda.synchronize()
    for k, s in slabs.items():
        s.check_canary(f'{name} [{k}]')


# ------------------------------------------------------------------------------------------------ 5. addressing, and LDS state
@pytest.mark.parametrize('entry', ENTRIES)
def test_guards_around_every_operand(dev, entry):
    """Every operand between guard slabs, the table's members included - 257 records of 37 bytes (the last dword of the records is
    padding, the last block holds one record) with a select, or 1025 points: only operands are read (poisoned guards change no output
    bit), only outputs are written (the canaries hold), no input is written; and, through guarded_runs, the same bits after poisoned LDS."""
    ctx = _ctx(dev)
    _, seg, pts, _, _, _, _ = _scene()
    fmt, extra, n = 7, 1, 257
    rl = RECORD_LEN[fmt] + extra
    rec, flat, _ = _records(fmt, extra, n)
    select = None if entry == 'residue' else SELECT
    if entry == 'residue':
        n, rl = 1025, 0
    want = _want(ctx, entry, rec, fmt, select, pts=pts[:n])
    g, start, segs = ops.line_index_host(seg, HW)
    st = ctx.st_win.stations.cpu().numpy()
    bs = ctx.st_bin.bin_start_host
    cur = _handle(torch.cuda.current_stream(dev))
    spec = _out_spec(ctx, entry, n, rl)
    W = {torch.int64: (2, torch.int32), torch.int32: (1, torch.int32), torch.uint8: (1, torch.uint8)}

    def run(B, poisoned):
        big = 0x7FFFFFF0 if poisoned else 0
        if entry == 'residue':
            s_src = Slab(dev, n, 4, front=8, back=8).fill_input(_t(pts[:n]), NAN if poisoned else 0.0)
        else:
            s_src = Slab(dev, 1, len(flat), front=1, back=1, dtype=torch.uint8).fill_input(_t(flat), 0xFF if poisoned else 0)
        s_seg = Slab(dev, len(seg), 8, front=4, back=4).fill_input(_t(seg), NAN if poisoned else 0.0)
        s_start = Slab(dev, 1, len(start), front=1, back=1, dtype=torch.int32).fill_input(torch.from_numpy(start), big)
        s_segs = Slab(dev, 1, len(segs), front=1, back=1, dtype=torch.int32).fill_input(torch.from_numpy(segs), big)
        s_st = Slab(dev, len(st), 4, front=8, back=8).fill_input(_t(st), NAN if poisoned else 0.0)
        s_bs = Slab(dev, 1, len(bs), front=1, back=1, dtype=torch.int32).fill_input(_t(bs), big)
        s_tst = Slab(dev, len(st), 4, front=8, back=8).fill_input(_t(st), NAN if poisoned else 0.0)
        s_ws = Slab(dev, 1, len(ctx.ws), front=1, back=1, dtype=torch.int32).fill_input(_t(ctx.ws), big)
        s_thr = Slab(dev, 1, len(ctx.thr), front=1, back=1).fill_input(_t(ctx.thr), -1e30 if poisoned else 0.0)
        s_iq = Slab(dev, 1, len(ctx.thr), front=1, back=1, dtype=torch.int32).fill_input(_t(ctx.paint_iq), -big)
        ins = (s_src, s_seg, s_start, s_segs, s_st, s_bs, s_tst, s_ws, s_thr, s_iq)
        s_out = {}
        for k, (shape, dt) in spec.items():
            words, sdt = W[dt]
            s_out[k] = Slab(dev, int(np.prod(shape)), words, front=16, back=16, dtype=sdt).fill_canary()
        before = [s.bits().clone() for s in ins]
        t = LmPaintTable()
        t.thr, t.paint_iq = (None, s_iq.ptr()) if entry == 'cross' else (s_thr.ptr(), None)
        t.win_start, t.win_start_host, t.stations = s_ws.ptr(), ctx.ws.ctypes.data, s_tst.ptr()
        t.window, t.thr_min, t.n_rows = WINDOW, ctx.thr_min, len(ctx.thr)
        P = {'segments': C.c_void_p(s_seg.ptr()), 'cell_start': C.c_void_p(s_start.ptr()), 'cell_segs': C.c_void_p(s_segs.ptr()),
             'stations': C.c_void_p(s_st.ptr()), 'bin_start': C.c_void_p(s_bs.ptr()), 'win_start': C.c_void_p(s_ws.ptr())}
        if entry == 'hist':
            del P['bin_start']
        tt._fill_if_poisoned()
        rc = _call(ctx, entry, C.c_void_p(s_src.ptr()), rl, fmt, n, select, {k: C.c_void_p(s.ptr()) for k, s in s_out.items()}, cur, table=t, P=P)
        assert rc == 0, lib().lm_last_error()
        torch.cuda.synchronize()
        for s, b in zip(ins, before):
            assert torch.equal(s.bits(), b), 'an input was written'
        return {k: (s, int(np.prod(spec[k][0]))) for k, s in s_out.items()}

    for attempt in range(2):                                             # the second round: the same bits again
        got = guarded_runs(run, f'{entry}_local', batch=False)
        for k, (shape, dt) in spec.items():
            g_k = np.ascontiguousarray(got[k].numpy()).view({torch.int64: np.int64, torch.int32: np.int32, torch.uint8: np.uint8}[dt]).reshape(shape)
            _same(f'{entry}, guarded', {k: g_k}, {k: want[k]})


# ------------------------------------------------------------------------------------------------ 6. streams
@pytest.mark.parametrize('entry', ENTRIES)
def test_entries_on_a_side_stream_and_in_graph_replay(dev, entry):
    """tests/test_gpu_threshold.py's stream case: on a side stream the bits of the default-stream run; captured into a graph and replayed
    on three data sets over outputs pre-filled with 0xFF, the bits of an eager run.  The outputs of an entry lie in one int64 tensor, one
    after the other without a gap (776 records of 20 bytes; 1024 points)."""
    ctx = _ctx(dev)
    fmt, extra, n = (7, 0, 776) if entry == 'colour' else (0, 0, 776)
    rl = RECORD_LEN[fmt] + extra
    pts = _scene()[2]
    if entry == 'residue':
        n, rl = 1024, 0
        sets = {k: pts[np.random.RandomState(40 + k).permutation(len(pts))[:n]] if k else pts[:n] for k in range(3)}
    else:
        sets = {k: _records(fmt, extra, n, seed=k) for k in range(3)}
    spec = _out_spec(ctx, entry, n, rl)
    sizes = {k: int(np.prod(shape)) * torch.empty((), dtype=dt).element_size() for k, (shape, dt) in spec.items()}
    assert all(v % 8 == 0 for v in sizes.values()), sizes
    total = sum(sizes.values()) // 8

    def views(out):
        flat, at, v = out.view(torch.uint8), 0, {}
        for k, (shape, dt) in spec.items():
            v[k] = flat[at:at + sizes[k]].view(dt).reshape(shape)
            at += sizes[k]
        return v

    @functools.lru_cache(maxsize=None)
    def want_of(k):
        w = _want(ctx, entry, None, fmt, None, pts=sets[k]) if entry == 'residue' else _want(ctx, entry, sets[k][0], fmt, None)
        return np.concatenate([np.ascontiguousarray(w[name]).reshape(-1).view(np.uint8) for name in spec]).view(np.int64)

    assert len(want_of(0)) == total and not np.array_equal(want_of(1), want_of(2)) and not np.array_equal(want_of(0), want_of(1))

    def call(ins, out, s):
        rc = _call(ctx, entry, _ptr(ins[0]), rl, fmt, n, None, {k: _ptr(v) for k, v in views(out).items()}, _handle(s))
        assert rc == 0, lib().lm_last_error()

    tt._stream_case(dev, f'{entry}_local', lambda k: [sets[k] if entry == 'residue' else sets[k][1]], call, want_of)


# ------------------------------------------------------------------------------------------------ 7. the package passes
def test_the_stage_passes_take_the_table(dev, tmp_path):
    """las_io's passes with a PaintTable in the option: label_las, survey_files, survey_colour_files, cross_files and residue_files go
    through the _local entries and give the brute force; hist_window_files gives the windowed table, whole or in chunks."""
    lines, seg, pts, st, ws, thr, _ = _scene()
    ctx = _ctx(dev)
    table = PaintTable(thr, ws, WINDOW)
    n = 1025
    rec, flat, _ = _records(7, 1, n)
    path = str(tmp_path / 'scene.las')
    world = _decoded(rec).astype(np.float64)
    co.write_colour_las(path, world[:, :3], world[:, 3], co.get_rgb(rec, 7), 7, scale=SCALE, offset=OFFSET, extra_bytes=1)
    data = np.fromfile(path, np.uint8)
    h = las_io.parse_header(data)
    o = h['offset_to_points']
    frec = data[o:o + n * h['record_len']].reshape(n, h['record_len'])
    assert h['point_format'] == 7 and np.array_equal(_decoded(frec), _decoded(rec))
    files = [(path, None, None)]
    survey = MarkingSurvey(bin=BIN, half_width=HW, z_tol=ZTOL, min_intensity=table)
    bins, bin_start = las_io.survey_files(files, lines, survey, device=dev)
    want = _want(ctx, 'colour', frec, 7, None)
    assert np.array_equal(bins, want['bins']) and np.array_equal(bin_start, ctx.st_bin.bin_start_host)
    b2, colours, _ = las_io.survey_colour_files(files, lines, survey, las_io.MarkingColour(yellow_ratio=0.75), device=dev, chunk_records=256)
    assert np.array_equal(b2, want['bins']) and np.array_equal(colours, want['colours'])
    cross = CrossSection(table, bin=BIN, half_width=HW, lateral=LQ / 1024, z_tol=ZTOL)
    cells, _ = las_io.cross_files(files, lines, cross, device=dev)
    assert np.array_equal(cells, _want(ctx, 'cross', frec, 7, None)['cells'])
    out = str(tmp_path / 'labelled.las')
    done = las_io.label_las(path, out, lines, MarkingLabels(half_width=HW, z_tol=ZTOL, min_intensity=table), None, device=dev)
    wl = _want(ctx, 'label', frec, 7, None)
    got = np.fromfile(out, np.uint8)
    assert np.array_equal(got[o:o + n * h['record_len']], wl['records_out'][:n * h['record_len']]) and done['per_line'] == wl['counts'][1:].tolist()
    out2 = str(tmp_path / 'labelled_chunks.las')
    las_io.label_las(path, out2, lines, MarkingLabels(half_width=HW, z_tol=ZTOL, min_intensity=table), None, device=dev, chunk_records=512)
    assert open(out, 'rb').read() == open(out2, 'rb').read()
    residue = PaintResidue(table, clear=CLEAR, reach=HW, z_tol=ZTOL, cell=CELL, min_cells=1, min_points=1)
    blobs = las_io.residue_files(files, lines, residue, device=dev)
    rindex = ops.line_index(seg, HW, cell=las_io.residue_index_cell(residue), device=dev)
    key, _ = lo.residue_local(_decoded(frec), seg, st, ws, WINDOW, thr, THR_MIN, HW, ZTOL, CLEAR, ops.residue_grid(rindex, CELL))
    cells_ref = np.unique(key[key >= 0])
    nx = blobs.grid['nx']
    assert np.array_equal(blobs.cells[:, 1].astype(np.int64) * nx + blobs.cells[:, 0], cells_ref) and len(cells_ref) > 20
    assert int(blobs.stats[:, 1].sum()) == int((key >= 0).sum())
    thr_opt = PaintThreshold(half_width=HW, ring=RQ / 1024, inner=RQ / 1024, outer=0.125, z_tol=ZTOL, bin_shift=SH, scope='window', window=WINDOW)
    hw, win_start, window = las_io.hist_window_files(files, lines, thr_opt, device=dev)
    wh = _want(ctx, 'hist', frec, 7, None)['hist']
    assert np.array_equal(hw, wh) and win_start.tolist() == ws.tolist() and window == WINDOW
    hw2, _, _ = las_io.hist_window_files(files, lines, thr_opt, device=dev, chunk_records=256)
    assert np.array_equal(hw2, wh)
    line_scope = las_io.hist_window_files(files, lines, thr_opt._replace(scope='line'), device=dev)
    assert line_scope[1].tolist() == [0, 1, 2, 3, 4, 5, 5] and np.array_equal(line_scope[0], las_io.hist_files(files, lines, thr_opt, device=dev)[:5])
    none = las_io.hist_window_files([], lines, thr_opt, device=dev)
    assert none[0].shape == (18, ctx.Z, ctx.NB) and not none[0].any()
    with pytest.raises(ValueError, match='cut for 2 lines'):
        las_io.survey_files(files, lines, survey._replace(min_intensity=PaintTable([1.0, 2.0], [0, 1, 2], WINDOW)), device=dev)


# ------------------------------------------------------------------------------------------------ 8. Runner
BRIGHT_ASPHALT, BRIGHT_PAINT, DIM_PAINT = 50000, 64000, 42000      # the dim line's paint is darker than the bright lines' asphalt


def test_runner_hands_a_table_to_the_auto_stages(dev, net, tmp_path):
    """tests/test_gpu_threshold.py's Runner test on a strip whose paint differs by line.  The network of the tests carries synthetic weights,
    so the paint is planted where the returned lines are, every return at or above the rasteriser's clip (the tile, and with it the lines,
    stay the same: asserted).  One line - the DIM one, the returned line with the fewest returns in its band among those with at least
    1500 - lies on asphalt of 34000 .. 37840 with paint of 42000; every other line on asphalt of 50000 .. 53840 with paint of 64000, as an
    inner lane under the scanner.  The reference policy (threshold_ref.policy on the brute-force table) puts the strip's threshold above
    the dim paint (asserted), so with scope='strip' the dim line's survey type is 'none' and it gets no labels; with scope='line' and
    scope='window' it has paint runs and labels, and paint_table.npy carries a threshold per line.  With scope='strip' given explicitly
    the files are byte for byte those of a run that leaves the new arguments out."""
    from lanemapping_amd.runner import Runner
    world, inten, prm, off = tt._tile_strip(tmp_path)
    rn = Runner.__new__(Runner)
    rn.cfg, rn.device, rn.net = net.cfg, dev, net
    out = {k: str(tmp_path / k) for k in ('plain', 'default', 'strip', 'line', 'window')}
    bare = str(tmp_path / 'bare' / 'strip.las')
    os.makedirs(os.path.dirname(bare))
    tc.las_ref.write_las(bare, world, inten, point_format=1, offset=tuple(off))
    lines = tt._result_lines(rn.infer_las_strip_to_map(bare, [prm], work_dirs=out['plain'], batch_size=2))
    assert len(lines) >= 2, 'the strip yielded fewer than two lines'
    base = PaintThreshold(min_returns=200)
    cloud = las_io.read_las_raw(bare, dev, shift=off)[0]
    seg = las_io.line_segments(lines, off)
    band = ops.label_points(cloud, ops.line_index(seg, base.half_width, device=dev), base.z_tol).cpu().numpy()
    near = ops.label_points(cloud, ops.line_index(seg, 0.075, device=dev), base.z_tol).cpu().numpy() > 0
    per_line = np.bincount(band, minlength=len(lines) + 1)[1:]
    assert (per_line >= 1500).sum() >= 2, per_line
    dim = int(np.argmin(np.where(per_line >= 1500, per_line, per_line.max() + 1))) + 1
    bright = (band > 0) & (band != dim)
    planted = np.where(bright, inten + (BRIGHT_ASPHALT - tt.ASPHALT), inten)
    planted = np.where(near & bright, BRIGHT_PAINT, np.where(near & (band == dim), DIM_PAINT, planted))
    assert planted.min() >= tt.ASPHALT > tt.CLIP and planted[band == dim].max() == DIM_PAINT < BRIGHT_ASPHALT
    painted = str(tmp_path / 'painted' / 'strip.las')
    os.makedirs(os.path.dirname(painted))
    tc.las_ref.write_las(painted, world, planted, point_format=1, offset=tuple(off))
    stages = dict(label=MarkingLabels(min_intensity='auto'), survey=MarkingSurvey(min_intensity='auto'), cross=CrossSection('auto'),
                  residue=PaintResidue('auto'))
    runs = {'default': base, 'strip': base._replace(scope='strip', window=7.0), 'line': base._replace(scope='line'),
            'window': base._replace(scope='window', window=10.0)}
    par, labels, marks = {}, {}, {}
    for k, threshold in runs.items():
        again = tt._result_lines(rn.infer_las_strip_to_map(painted, [prm], work_dirs=out[k], batch_size=2, threshold=threshold, **stages))
        assert len(again) == len(lines) and all(np.array_equal(a, b) for a, b in zip(again, lines)), 'paint above the clip moved the lines'
        par[k] = os.path.join(out[k], 'params')
        labels[k] = json.load(open(os.path.join(par[k], 'labels.json')))['strip.las'][2]
        marks[k] = json.load(open(os.path.join(par[k], 'markings.json')))
    # the reference: the brute-force table against the returned lines, and the policy on it
    data = np.fromfile(painted, np.uint8)
    h = las_io.parse_header(data)
    o, rl, n = h['offset_to_points'], h['record_len'], h['n_points']
    dec = lr.decode_f32(data[o:o + n * rl].reshape(n, rl), h['scale'], h['offset'], off)
    st, _ = las_io.line_stations(lines, off, las_io.HIST_BIN)
    want = tr.hist_f32(dec, seg, st, len(lines), base.half_width, base.z_tol, base.ring_q, base.bin_shift, pruned=True)[0]
    policy = tr.policy(want, min_returns=200)
    strip_thr = policy['strip']['threshold']
    print(f'{len(lines)} lines, returns per band {per_line.tolist()}, dim line {dim}; strip {policy["strip"]}; dim line {policy["lines"][dim]}')
    assert policy['strip']['supported'] and strip_thr > DIM_PAINT, 'the reference policy: the strip\'s one number leaves the dim line without paint'
    assert policy['lines'][dim]['supported'] and tt.ASPHALT + 3840 < policy['lines'][dim]['threshold'] <= DIM_PAINT
    # scope='strip': what there was - the dim line is lost - and explicit arguments change no byte
    assert labels['default'][dim - 1] == 0 and marks['default'][str(dim)]['type'] == 'none' and sum(labels['default']) > 0
    assert tt._dir_files(out['default']) == tt._dir_files(out['strip'])
    for name in tt._dir_files(out['default']):
        a, b = (open(os.path.join(out[k], name), 'rb').read() for k in ('default', 'strip'))
        assert a == b, f'{name} differs between scope left out and scope=\'strip\''
    assert np.array_equal(np.load(os.path.join(par['default'], 'paint_hist.npy')), want)
    # scope='line' and 'window': the table
    for k in ('line', 'window'):
        assert labels[k][dim - 1] > 0 and marks[k][str(dim)]['type'] != 'none' and marks[k][str(dim)]['runs'], f'{k}: the dim line has no paint'
        for j in range(len(lines)):                                         # a bright line keeps its paint; with one row per line, exactly it
            if j + 1 != dim:
                assert labels[k][j] >= labels['default'][j] and (k == 'window' or labels[k][j] == labels['default'][j]), (k, j + 1)
        assert np.array_equal(np.load(os.path.join(par[k], 'paint_hist.npy')), want), 'the per-line table is the sum of the windows'
        hist_w = np.load(os.path.join(par[k], 'paint_hist_windows.npy'))
        table = las_io.load_paint_table(os.path.join(par[k], 'paint_table.npy'))
        assert np.array_equal(las_io.line_hist_of_windows(hist_w, table.win_start), want)
        thr_ref, src_ref, groups = lo.table_policy(hist_w, table.win_start, min_returns=200)
        assert table.thr.tolist() == [float(f32(v)) for v in thr_ref] and table.source.tolist() == src_ref
        rows_dim = table.thr[table.win_start[dim - 1]:table.win_start[dim]]
        others = np.delete(table.thr, np.arange(table.win_start[dim - 1], table.win_start[dim]))
        # per line the threshold lies between the line's asphalt and its paint.  Per window of 10 m it need not: the asphalt of this strip
        # is a pattern in the plane, and along some windows every inner return is brighter than every outer one, a better separation than
        # the paint's share - the window's threshold then cuts the asphalt.  What holds for both scopes: no row loses its line's paint,
        # and the dim line's rows lie below every other row
        assert len(rows_dim) and (rows_dim <= DIM_PAINT).all() and len(others) and (others <= BRIGHT_PAINT).all()
        assert rows_dim.max() < BRIGHT_ASPHALT <= others.min(), 'a different threshold per line'
        if k == 'line':
            assert (rows_dim > tt.ASPHALT + 3840).all() and (others > BRIGHT_ASPHALT + 3840).all()
        used = json.load(open(os.path.join(par[k], 'paint_threshold.json')))
        assert used['strip'] == json.loads(json.dumps(policy['strip'])) and set(used) == {'strip', 'lines', 'windows'}
        assert [len(v) for v in used['windows'].values()] == np.diff(table.win_start).tolist()
        assert all(len(w) == 6 and w[3] in las_io.SOURCES for v in used['windows'].values() for w in v)
        new = {os.path.join('params', f) for f in ('paint_hist_windows.npy', 'paint_table.npy')}
        assert set(tt._dir_files(out[k])) - set(tt._dir_files(out['default'])) == new
    line_table = las_io.load_paint_table(os.path.join(par['line'], 'paint_table.npy'))
    assert np.diff(line_table.win_start).max() == 1, 'scope=\'line\': one row per line'
    assert np.diff(las_io.load_paint_table(os.path.join(par['window'], 'paint_table.npy')).win_start).max() > 1
