"""Restatement of the paint-table rule (include/lanemap_hip.h: the windows, the windowed histogram, the rule of the stages) for the tests,
in numpy on top of the existing references, which stay as they are: label_ref.label_f32 for the winner, profile_ref.point_terms with
bin = window for the row, and the accumulators of profile_ref, colour_ref, cross_ref, threshold_ref and residue_ref.keys_f32.  The policy
(las_io.paint_table) is restated with plain loops on top of threshold_ref.group.

The float32 expressions round after every operation like the kernels built without contraction."""
import numpy as np

import colour_ref as co
import cross_ref as cr
import label_ref as lr
import profile_ref as pr
import residue_ref as rr
import threshold_ref as tr

f32 = np.float32


def winner(pts, seg, half_width, z_tol, mask=None):
    """Step 1 of the rule: the labelling rule's winner WITHOUT a min_intensity -> (line, d2, win)."""
    return lr.label_f32(pts, seg, half_width, z_tol, None, mask=mask)


def rows(pts, seg, stations, win_start, window, line, win):
    """Step 2: the table row of every point from its label and winning segment, -1 without a label: profile_ref.point_terms' absolute bin
    for bin = window and bin_start = win_start.  A line above the table's L, or one that owns no window, has no row."""
    ws = np.asarray(win_start, np.int64)
    L = len(ws) - 1
    line = np.asarray(line, np.int64)
    inside = (line > 0) & (line <= L)
    owns = np.zeros(len(line), bool)
    owns[inside] = (ws[line[inside]] - ws[line[inside] - 1]) > 0
    ln = np.where(owns, line, 0)
    return np.where(owns, pr.point_terms(pts, seg, stations, ws, window, ln, win)['B'], -1)


def passes(pts, row, thr, thr_min):
    """Step 3: i >= thr_min && i >= thr[row] in float32; a NaN intensity and a point without a row fail."""
    pts = np.asarray(pts, f32)
    thr = np.asarray(thr, f32)
    ok = row >= 0
    with np.errstate(invalid='ignore'):
        ok &= pts[:, 3] >= f32(thr_min)
        ok[ok] &= pts[ok, 3] >= thr[row[ok]]
    return ok


def label_local(pts, seg, stations, win_start, window, thr, thr_min, half_width, z_tol, mask=None):
    """-> (line with 0 where the return does not pass, d2, win, row, ok): what every stage but the cross-sections builds on."""
    line, d2, win = winner(pts, seg, half_width, z_tol, mask)
    row = rows(pts, seg, stations, win_start, window, line, win)
    ok = passes(pts, row, thr, thr_min)
    return np.where(ok, line, 0).astype(line.dtype), d2, win, row, ok


def hist_window_f32(pts, seg, stations, win_start, window, half_width, z_tol, ring_q, bin_shift, mask=None, hist=None):
    """The windowed histogram by brute force: -> (hist [R, Z, NB], cell, row).  threshold_ref.hist_terms' r and ib, the row per window."""
    line, _, win = winner(pts, seg, half_width, z_tol, mask)
    row = rows(pts, seg, stations, win_start, window, line, win)
    terms = tr.hist_terms(pts, seg, stations, half_width, ring_q, bin_shift, line, win)
    _, Z, NB = tr.shape(half_width, ring_q, bin_shift)
    R = int(win_start[-1])
    cell = np.where(row >= 0, (row * Z + terms['r']) * NB + terms['ib'], -1)
    flat = np.zeros(R * Z * NB, np.int64) if hist is None else np.array(hist, np.int64, copy=True).reshape(-1)
    np.add.at(flat, cell[cell >= 0], 1)
    return flat.reshape(R, Z, NB), cell, row


def profile_local(pts, seg, stations, bin_start, bin, win_start, window, thr, thr_min, half_width, z_tol, mask=None, bins=None):
    """-> (bins [n_bins, 6], terms with B = -1 where the return does not pass, line)."""
    line, _, win, _, _ = label_local(pts, seg, stations, win_start, window, thr, thr_min, half_width, z_tol, mask)
    terms = pr.point_terms(pts, seg, stations, bin_start, bin, line, win)
    return pr.accumulate(terms, int(bin_start[-1]), bins), terms, line


def colour_local(pts, rgb, seg, stations, bin_start, bin, win_start, window, thr, thr_min, half_width, z_tol, blue_q, mask=None, bins=None,
                 colours=None):
    """-> (bins, colours)."""
    b, terms, _ = profile_local(pts, seg, stations, bin_start, bin, win_start, window, thr, thr_min, half_width, z_tol, mask, bins)
    return b, co.accumulate(terms['B'], rgb, blue_q, int(bin_start[-1]), colours)


def cross_local(pts, seg, stations, bin_start, bin, win_start, window, paint_iq, half_width, z_tol, lateral_q, mask=None, cells=None):
    """Every finite return counts; it is paint when iq >= paint_iq[row] (a return without a row is none): -> cells [n_bins, nl, 4]."""
    line, _, win = winner(pts, seg, half_width, z_tol, mask)
    row = rows(pts, seg, stations, win_start, window, line, win)
    terms = cr.cross_terms(pts, seg, stations, bin_start, bin, half_width, lateral_q, line, win)
    nl = cr.hq_nl(half_width, lateral_q)[1]
    n_bins = int(bin_start[-1])
    flat = np.zeros((n_bins * nl, 4), np.int64) if cells is None else np.array(cells, np.int64, copy=True).reshape(n_bins * nl, 4)
    on = terms['row'] >= 0
    piq = np.asarray(paint_iq, np.int64)
    paint = np.zeros(len(row), np.int64)
    has = on & (row >= 0)
    paint[has] = terms['iq'][has] >= piq[row[has]]
    np.add.at(flat[:, 0], terms['row'][on], 1)
    np.add.at(flat[:, 1], terms['row'][on], paint[on])
    np.add.at(flat[:, 2], terms['row'][on], terms['iq'][on])
    np.add.at(flat[:, 3], terms['row'][on], terms['zq'][on])
    return flat.reshape(n_bins, nl, 4)


def residue_local(pts, seg, stations, win_start, window, thr, thr_min, reach, z_tol, clear, grid):
    """residue_ref.keys_f32 without a min_intensity, then no residue where the return does not pass: -> (key [N] int64, iq [N] int32)."""
    key, iq = rr.keys_f32(pts, seg, reach, z_tol, None, clear, grid)
    ok = label_local(pts, seg, stations, win_start, window, thr, thr_min, reach, z_tol)[4]
    return np.where(ok, key, -1), np.where(ok, iq, 0).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- the policy
def table_policy(hist_w, win_start, **kw):
    """las_io.paint_table with plain loops: -> (thr list, source list, {'strip', 'lines', 'windows'}); thr None where the strip has no
    support (las_io raises there).  kw: PaintThreshold's arguments as threshold_ref.policy takes them."""
    import inspect
    defaults = {k: v.default for k, v in inspect.signature(tr.policy).parameters.items() if v.default is not inspect.Parameter.empty}
    a = {**defaults, **kw}
    hist_w = np.asarray(hist_w)
    _, Z, inn, out = tr.rings(a['half_width'], a['ring'], a['inner'], a['outer'])
    NB = hist_w.shape[2]

    def of(rs):
        A = [sum(int(hist_w[r, z, b]) for r in rs for z in inn) for b in range(NB)]
        O = [sum(int(hist_w[r, z, b]) for r in rs for z in out) for b in range(NB)]
        return tr.group(A, O, a['bin_shift'], a['min_returns'], a['min_separation'], a['tolerance_shift'])

    L = len(win_start) - 1
    strip = of(range(len(hist_w)))
    lines = {k + 1: of(range(int(win_start[k]), int(win_start[k + 1]))) for k in range(L)}
    windows = {k + 1: [of([r]) for r in range(int(win_start[k]), int(win_start[k + 1]))] for k in range(L)}
    thr, source = [], []
    for k in range(1, L + 1):
        for g in windows[k]:
            if g['supported']:
                thr.append(g['threshold']), source.append(0)
            elif lines[k]['supported']:
                thr.append(lines[k]['threshold']), source.append(1)
            else:
                thr.append(strip['threshold']), source.append(2)
    return thr, source, {'strip': strip, 'lines': lines, 'windows': windows}
