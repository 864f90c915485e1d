"""Vertex heights from the points (csrc/drape.hip) and the back-projection that takes them (csrc/backproject.cpp,
lm_polyline_backproject_z) restated in numpy, for tests/test_drape_cpu.py and tests/test_gpu_drape.py.

The window test and the keys are those of tests/ground_ref.py (float32, every operation rounded on its own), so the GPU results can be
compared bit for bit.
  (a) window_keys    per vertex the smallest key of vz over the tile's points of each pixel of its (2R+1) x (2R+1) window, EMPTY outside
                     the tile and where no point falls
  (b) median         lower median of the non-empty keys, their count; NaN for none
  backproject_z      steps 2 and 4 of the back-projection in float64 for vertices that all carry a height, fit='none'
"""
import math

import numpy as np

import ground_ref as gr

f32 = np.float32
EMPTY = gr.EMPTY


def pixel_keys(pts, p, H, W):
    """One tile: -> keys [H, W] u32, the smallest key of vz per pixel over the points that count for the tile."""
    keys = np.full(H * W, EMPTY, dtype=np.uint32)
    on, row, col, vz = gr.window(pts, p, H, W)
    np.minimum.at(keys, row[on] * W + col[on], gr.key_of(vz[on]))
    return keys.reshape(H, W)


def window_keys(pixel, vertices, R):
    """(a) keys [H, W] of one tile, vertices [n, 2] -> [n, 2R+1, 2R+1] u32; a window pixel outside the tile is EMPTY."""
    H, W = pixel.shape
    padded = np.full((H + 2 * R, W + 2 * R), EMPTY, dtype=np.uint32)
    padded[R:R + H, R:R + W] = pixel
    out = np.full((len(vertices), 2 * R + 1, 2 * R + 1), EMPTY, dtype=np.uint32)
    for n, (vr, vc) in enumerate(vertices):
        out[n] = padded[vr:vr + 2 * R + 1, vc:vc + 2 * R + 1]
    return out


def median(slots):
    """(b) slots [n, ...] u32 -> (z [n] f32, npix [n] int32): element (k - 1) // 2 of the k non-empty keys in ascending order."""
    slots = np.asarray(slots, dtype=np.uint32).reshape(len(slots), -1)
    med = np.full(len(slots), EMPTY, dtype=np.uint32)
    npix = np.zeros(len(slots), dtype=np.int32)
    for n, s in enumerate(slots):
        s = np.sort(s[s != EMPTY])
        npix[n] = len(s)
        if len(s):
            med[n] = s[(len(s) - 1) // 2]
    return gr.keys_to_values(med), npix


def drape_vertices(pts, offs, params, vertices, voffs, H, W, R):
    """-> (z [V] f32, npix [V] int32, pixel_min [V, 2R+1, 2R+1] f32 with NaN = empty) as ops.drape_vertices(want_pixel_min=True) returns
    them."""
    vertices = np.asarray(vertices, dtype=np.int64).reshape(-1, 2)
    slots = np.full((len(vertices), 2 * R + 1, 2 * R + 1), EMPTY, dtype=np.uint32)
    for b, p in enumerate(params):
        if voffs[b + 1] > voffs[b]:
            slots[voffs[b]:voffs[b + 1]] = window_keys(pixel_keys(pts[offs[b]:offs[b + 1]], p, H, W), vertices[voffs[b]:voffs[b + 1]], R)
    z, npix = median(slots)
    return z, npix, gr.keys_to_values(slots)


def _qmul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]


def backproject_z(params, seqs, z):
    """Steps 2 and 4 of lm_polyline_backproject_z in float64, operation by operation, for slots that all take their height from z
    (fit='none'): seqs [..., 2] (row, col), z [...] f32 or f64 -> [..., 3].  params: the dict of load_pc_2_img_transform_paras."""
    seqs = np.asarray(seqs, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)                         # (a float32 height converts exactly, as (double)vertex_z does)
    reso, off = [float(v) for v in params['img_reso'][:2]], [float(v) for v in params['bev_img_offset'][:2]]
    t = [float(v) for v in params['las_rotation_trans_quan'][:7]]
    trans, q = t[0:3], t[3:7]
    shift = [float(v) for v in params['las_read_offset'][:3]]
    qn = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    qinv = [q[0] / qn, (q[1] * -1.0) / qn, (q[2] * -1.0) / qn, (q[3] * -1.0) / qn]
    out = np.zeros(seqs.shape[:-1] + (3,), dtype=np.float64)
    for idx in np.ndindex(*seqs.shape[:-1]):
        r, c = float(seqs[idx][0]), float(seqs[idx][1])
        v = [0.0, r * reso[0] + off[0], c * reso[1] + off[1], float(z[idx])]
        o = _qmul(_qmul(q, v), qinv)
        for a in range(3):
            out[idx][a] = (o[1 + a] + trans[a]) + shift[a]
    return out


def fit_line(z):
    """Step 3 of the back-projection for one line: its heights replaced by their least-squares line over the vertex index, with the
    sequential float64 sums of csrc/backproject.cpp."""
    z = [float(v) for v in z]
    n = len(z)
    sxy, sy, sx, sxx = 0.0, 0.0, 0, 0
    for i in range(n):
        sxy = sxy + float(i) * z[i]
        sy = sy + z[i]
        sx += i
        sxx += i * i
    p = float(n) * sxy - float(sx) * sy
    q = n * sxx - sx * sx
    wgt = 0.0 if abs(float(q)) < 1e-6 else p / float(q)
    sb = 0.0
    for i in range(n):
        sb = sb + (z[i] - wgt * float(i))
    b = sb / float(n)
    return np.array([wgt * float(i) + b for i in range(n)], dtype=np.float64)


# ------------------------------------------------------------------------------------------------ the crest of the accuracy tests
CREST_S, CREST_RESO, CREST_R = 96, 0.0625, 4
CREST_A, CREST_B = 0.1, 0.05


def crest_f(x, y):
    """The surface: a crest across x at x = 3 m that climbs 5 % along y."""
    return -CREST_A * (x - 3.0) ** 2 + CREST_B * y


def crest_case():
    """A noise-free cloud on crest_f, one point at every pixel centre of an axis-aligned 96 x 96 tile of 1/16 m pixels (6 m x 6 m; every
    coordinate is exact in float32), and three straight polylines along x, across the crest, with fractional rows and columns.
    -> (params dict, raster-parameter keywords, points [S*S, 4] f32, seqs [3, 12, 2], lens, g): g bounds |grad f| over the tile:
    |df/dx| <= 2 A * 3 = 0.6, df/dy = B."""
    S, reso = CREST_S, CREST_RESO
    off, trans = (-0.5, 0.25), (8.0, 16.0, 0.0)
    params = {'img_reso': [reso, reso], 'bev_img_offset': list(off), 'ele_reso': 0.05, 'local_min_ele': -2.0,
              'las_read_offset': [0.0, 0.0, 0.0], 'las_rotation_trans_quan': list(trans) + [1.0, 0.0, 0.0, 0.0]}
    kw = dict(trans=trans, bev_img_offset=off, img_reso=(reso, reso), local_min_ele=-2.0, ele_reso=0.05)
    r, c = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    lx, ly = r.ravel() * reso, c.ravel() * reso                  # position inside the tile, 0 .. 6 m
    pts = np.stack([lx + off[0] + trans[0], ly + off[1] + trans[1], crest_f(lx, ly), np.full(S * S, 5000.0)], axis=1).astype(f32)
    lens = [12, 12, 9]
    seqs = np.zeros((3, 12, 2))
    for l, col in enumerate((10.3, 47.75, 90.5)):
        seqs[l, :lens[l], 0] = 2.5 + 8.0 * np.arange(lens[l]) + 0.25 * l
        seqs[l, :lens[l], 1] = col
    g = math.sqrt((2 * CREST_A * 3.0) ** 2 + CREST_B ** 2)
    return params, kw, pts, seqs, lens, g


def crest_error(params, out, lens):
    """|z - f| of every real vertex of a back-projected crest_case (identity rotation, no read offset): -> [n] float64."""
    t, off = params['las_rotation_trans_quan'], params['bev_img_offset']
    err = []
    for l, n in enumerate(lens):
        lx, ly = out[l, :n, 0] - t[0] - off[0], out[l, :n, 1] - t[1] - off[1]
        err.append(np.abs(out[l, :n, 2] - t[2] - crest_f(lx, ly)))
    return np.concatenate(err)


def crest_bound(g):
    """g (R + 1) reso sqrt 2 - the median is the height of a pixel centre within R pixels of the vertex pixel, and the vertex lies less
    than one pixel from that pixel's centre along each axis - plus one float32 ulp of the largest |f| (the points are float32)."""
    return g * (CREST_R + 1) * CREST_RESO * math.sqrt(2.0) + float(np.spacing(f32(CREST_A * 9.0 + CREST_B * 6.0)))
