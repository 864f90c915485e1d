"""Numpy restatement of the marking colour rule (include/lanemap_hip.h, csrc/profile.hip: lm_las_line_colour_records) for the tests: which
bin a return lands in is profile_ref's answer (label_ref's winner, profile_ref.point_terms' bin); what it adds to the colour row is
plain integer numpy here; beside it a helper that writes R, G, B into records of a given format, and a plain-loop checker of
las_io.marking_colours.

The rule on a four-point example, worked by hand (blue_q = 768, i.e. yellow_ratio 0.75: yellow when 2048 B < 768 (R + G)):

    return   bin   R      G      B       black?   2048 B     768 (R + G)   yellow?
    a        0     60000  50000  10000   no       20480000   84480000      yes
    b        0     40000  40000  30000   no       61440000   61440000      no: equality is not yellow
    c        0     0      0      0       yes      -          -             -  (adds 1 to n_black, nothing else)
    d        2     40000  40000  29999   no       61437952   61440000      yes: one unit less of B than b

    colours[0] = n_c 2, sum R 100000, sum G 90000, sum B 40000, n_yellow 1, n_black 1
    colours[1] = 0, 0, 0, 0, 0, 0
    colours[2] = n_c 1, sum R 40000, sum G 40000, sum B 29999, n_yellow 1, n_black 0

worked_example() returns these inputs and this table; tests/test_colour_cpu.py holds accumulate() to it."""
from fractions import Fraction

import numpy as np

import profile_ref as pr

RGB_OFFSET = {2: 20, 3: 28, 5: 28, 7: 30, 8: 30, 10: 30}                       # the rule's table, typed again
MIN_LEN = {0: 20, 1: 28, 2: 26, 3: 34, 4: 57, 5: 63, 6: 30, 7: 36, 8: 38, 9: 59, 10: 67}
COLOUR_FORMATS = (2, 3, 5, 7, 8, 10)


def put_rgb(rec, fmt, rgb):
    """rec [n, record_len] uint8, rgb [n, 3] in 0..65535 -> rec, with R, G, B written as u16 little-endian at the format's colour offset."""
    o = RGB_OFFSET[fmt]
    rgb = np.asarray(rgb, np.int64)
    assert rec.ndim == 2 and rec.dtype == np.uint8 and rec.shape[1] >= MIN_LEN[fmt] and rgb.shape == (len(rec), 3)
    assert (rgb >= 0).all() and (rgb <= 65535).all()
    for c in range(3):
        rec[:, o + 2 * c] = rgb[:, c] & 255
        rec[:, o + 2 * c + 1] = rgb[:, c] >> 8
    return rec


def get_rgb(rec, fmt):
    """-> [n, 3] int64: the R, G, B of [n, record_len] uint8 records, byte by byte."""
    o = RGB_OFFSET[fmt]
    r = np.asarray(rec).astype(np.int64)
    return np.stack([r[:, o + 2 * c] + 256 * r[:, o + 2 * c + 1] for c in range(3)], axis=1)


def write_colour_las(path, xyz, intensity, rgb, point_format, scale=(0.001, 0.001, 0.001), offset=(0., 0., 0.), extra_bytes=0):
    """A LAS file of a colour format with the given triples: written by oracle/las_ref.write_las as the nearest format it knows (2, 3 or 6)
    with the record padded to this format's length, then the format byte of the header (104) and the R, G, B of every record patched.
    -> the [n, record_len] records as written."""
    import struct
    from oracle import las_ref
    base = point_format if point_format in las_ref.RECORD_LEN else (3 if point_format <= 5 else 6)
    rl = MIN_LEN[point_format] + extra_bytes
    las_ref.write_las(path, xyz, intensity, point_format=base, version=(1, 4) if point_format >= 6 else (1, 2), scale=scale, offset=offset,
                      extra_bytes=rl - las_ref.RECORD_LEN[base])
    data = np.fromfile(path, np.uint8)
    data[104] = point_format
    off, n = struct.unpack_from('<I', data, 96)[0], len(np.asarray(xyz))
    assert struct.unpack_from('<H', data, 105)[0] == rl and len(data) == off + n * rl
    rec = data[off:].reshape(n, rl)
    put_rgb(rec, point_format, rgb)
    data.tofile(path)
    return rec.copy()


def votes(rgb, blue_q):
    """-> (black, coloured, yellow) boolean [n] of the triples."""
    rgb = np.asarray(rgb, np.int64)
    assert 1 <= int(blue_q) <= 1024
    black = (rgb == 0).all(axis=1)
    yellow = ~black & (2048 * rgb[:, 2] < int(blue_q) * (rgb[:, 0] + rgb[:, 1]))
    return black, ~black, yellow


def accumulate(B, rgb, blue_q, n_bins, colours=None):
    """B [n]: the absolute bin of every return, -1 where it lands in none (profile_ref.point_terms' 'B') -> colours [n_bins, 6] int64 =
    n_c, sum R, sum G, sum B, n_yellow, n_black; colours: what to add to."""
    colours = np.zeros((n_bins, 6), np.int64) if colours is None else np.array(colours, np.int64, copy=True)
    B, rgb = np.asarray(B, np.int64), np.asarray(rgb, np.int64)
    black, col, yellow = votes(rgb, blue_q)
    on = B >= 0
    np.add.at(colours[:, 0], B[on & col], 1)
    for c in range(3):
        np.add.at(colours[:, 1 + c], B[on & col], rgb[on & col, c])
    np.add.at(colours[:, 4], B[on & yellow], 1)
    np.add.at(colours[:, 5], B[on & black], 1)
    return colours


def colour_f32(pts, rgb, seg, stations, bin_start, bin, half_width, z_tol, blue_q, min_intensity=None, mask=None, bins=None, colours=None,
               pruned=False):
    """The whole rule by brute force on decoded rows and their triples: -> (bins, colours, terms, line).  pruned: profile_ref's pruned
    search, for clouds of millions of returns (then nothing can be added to)."""
    if pruned:
        assert bins is None and colours is None
        b, terms, line, _ = pr.profile_f32_pruned(pts, seg, stations, bin_start, bin, half_width, z_tol, min_intensity, mask)
    else:
        b, terms, line, _ = pr.profile_f32(pts, seg, stations, bin_start, bin, half_width, z_tol, min_intensity, mask=mask, bins=bins)
    return b, accumulate(terms['B'], rgb, blue_q, int(bin_start[-1]), colours), terms, line


def worked_example():
    """-> (B, rgb, blue_q, n_bins, the table of the module docstring)."""
    B = np.array([0, 0, 0, 2])
    rgb = np.array([[60000, 50000, 10000], [40000, 40000, 30000], [0, 0, 0], [40000, 40000, 29999]])
    want = np.array([[2, 100000, 90000, 40000, 1, 1], [0, 0, 0, 0, 0, 0], [1, 40000, 40000, 29999, 1, 0]], np.int64)
    return B, rgb, 768, 3, want


def blue_q_of(yellow_ratio):
    """round(1024 yellow_ratio), halves up, at least 1: in exact rationals."""
    return max(1, min(1024, int((Fraction(yellow_ratio) * 1024 + Fraction(1, 2)).__floor__())))


def colours_of(bins, colours, bin_start, bin, min_points, max_gap, yellow_share, min_coloured):
    """What las_io.marking_colours must return, with plain loops and exact rationals: one dict per line."""
    share = Fraction(yellow_share)

    def decide(n_c, n_y):
        if n_c < min_coloured:
            return 'unknown'
        return 'yellow' if Fraction(n_y) >= share * n_c else 'white'

    out = []
    for k in range(len(bin_start) - 1):
        lo, hi = int(bin_start[k]), int(bin_start[k + 1])
        rows = [tuple(int(v) for v in r) for r in np.asarray(bins)[lo:hi]]
        cols = [tuple(int(v) for v in r) for r in np.asarray(colours)[lo:hi]]
        on = [r[0] >= min_points for r in rows]
        runs = []
        for i, o in enumerate(on):                            # maximal runs of painted bins, holes of at most max_gap metres closed
            if not o:
                continue
            if runs and (i - runs[-1][1] - 1) * bin <= max_gap + 1e-9 * bin:
                runs[-1][1] = i
            else:
                runs.append([i, i])
        tot = [sum(c[j] for c, o in zip(cols, on) if o) for j in range(6)]
        per_run = []
        for a, b in runs:
            per_run.append(decide(sum(cols[i][0] for i in range(a, b + 1) if on[i]), sum(cols[i][4] for i in range(a, b + 1) if on[i])))
        out.append({'coloured': tot[0], 'yellow': tot[4], 'black': tot[5], 'rgb': [tot[j] / tot[0] for j in (1, 2, 3)] if tot[0] else None,
                    'colour': decide(tot[0], tot[4]), 'run_colours': per_run})
    return out
