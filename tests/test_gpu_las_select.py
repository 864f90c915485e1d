"""GPU: decode + select + stable compaction of LAS point records (lm_las_decode_select, las_io.PointFilter).

The reference is a numpy restatement written here: bytes 14-16 of every record are parsed per point format, the boolean mask of the
filter is built from them and from the float32 z of the UNSELECTED decode, and that decode's output is indexed with the mask.  Every
comparison is for equal bits.  Records are random bytes, so classes, flags and return fields take every value."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from guards import Slab, guarded_runs
from lanemapping_amd import io_utils, las_io, ops, synth
from lanemapping_amd._lib import lib
from lanemapping_amd.las_io import PointFilter
from oracle import las_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = W = 1152
SCALE, OFFSET, SHIFT = [1e-3, 2e-3, 5e-4], [100.0, -200.0, 12.5], [96.0, -208.0, 10.0]


def _scan_tile():
    """Elements one workgroup of prim.hip's scan takes: the block counts of more records than 256 of these need a second scan level."""
    text = open(os.path.join(ROOT, 'lanemapping_amd', 'csrc', 'prim.hip')).read()
    return int(re.search(r'constexpr\s+int\s+TILE\s*=\s*(\d+)', text).group(1))


N_BIG = (_scan_tile() + 1) * 256 + 1                 # one block more than a scan tile holds, plus a block of one record
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000, N_BIG]
# (point format, record length): the formats at their minimum length, and one length that is no multiple of 4 for each bit layout
FORMATS = [(0, 20), (1, 28), (3, 34), (6, 30), (7, 36), (10, 67), (0, 23), (6, 37)]


@functools.lru_cache(maxsize=None)
def _pool():
    return np.random.RandomState(20240).randint(0, 256, N_BIG * 67 + 64, dtype=np.uint8)


def _records(n, rl, skip=0):
    """n records of rl random bytes -> ([n, rl] view, the flat copy padded to a multiple of 4 bytes that goes to the device)."""
    nbytes = n * rl
    flat = np.zeros((nbytes + 3) // 4 * 4, np.uint8)
    flat[:nbytes] = _pool()[skip:skip + nbytes]
    return flat[:nbytes].reshape(n, rl), flat


# ------------------------------------------------------------------------------------------------ the numpy restatement
def _fields(rec, fmt):
    """-> return number, number of returns, flags as synthetic 1 | key-point 2 | withheld 4 | overlap 8, classification."""
    b14, b15 = rec[:, 14].astype(np.int64), rec[:, 15].astype(np.int64)
    if fmt >= 6:
        return b14 & 15, b14 >> 4, b15 & 15, rec[:, 16].astype(np.int64)
    return b14 & 7, (b14 >> 3) & 7, b15 >> 5, b15 & 31        # bits 5, 6, 7 of byte 15: no overlap bit in these formats


def _mask(rec, fmt, f, z):
    rn, nr, flags, cls = _fields(rec, fmt)
    keep = np.ones(len(rec), bool) if f.classes is None else np.isin(cls, np.asarray(f.classes, np.int64))
    drop = 1 * f.drop_synthetic | 2 * f.drop_keypoint | 4 * f.drop_withheld | 8 * f.drop_overlap
    keep &= (flags & drop) == 0
    keep &= {'all': np.ones(len(rec), bool), 'first': rn == 1, 'last': rn == nr, 'single': nr == 1}[f.returns]
    if f.z_range is not None:
        assert z.dtype == np.float32
        keep &= (np.float32(f.z_range[0]) <= z) & (z <= np.float32(f.z_range[1]))
    return keep


def _filters(fmt, z):
    """name -> PointFilter; z: the decoded heights, two of which become the bounds of the window."""
    cmax = 256 if fmt >= 6 else 32
    out = {'everything': PointFilter(drop_withheld=False),
           'nothing': PointFilter(classes=[], drop_withheld=False),
           'classes 2, 11': PointFilter(classes=[2, 11], drop_withheld=False),
           'withheld': PointFilter(),
           'first': PointFilter(drop_withheld=False, returns='first'),
           'last': PointFilter(drop_withheld=False, returns='last'),
           'single': PointFilter(drop_withheld=False, returns='single')}
    if len(z):
        zs = np.sort(z)
        lo, hi = float(zs[int(0.3 * (len(zs) - 1))]), float(zs[int(0.7 * (len(zs) - 1))])
        wide = (float(zs[int(0.05 * (len(zs) - 1))]), float(zs[int(0.95 * (len(zs) - 1))]))
    else:
        lo, hi, wide = -1.0, 1.0, (-2.0, 2.0)
    out['z window'] = PointFilter(drop_withheld=False, z_range=(lo, hi))
    out['combined'] = PointFilter(classes=range(0, cmax, 2), drop_withheld=True, drop_overlap=True, returns='last', z_range=wide)
    return out, lo, hi


def _plain(dev, flat, rl, n, normalise=False):
    if n == 0:
        return torch.empty((0, 4), device=dev)
    return las_io.decode_points(torch.from_numpy(flat).to(dev), rl, n, SCALE, OFFSET, SHIFT, normalise)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. kept points and count
@pytest.mark.parametrize('fmt, rl', FORMATS)
def test_selection_equals_the_numpy_selection(dev, fmt, rl):
    for n in SIZES:
        rec, flat = _records(n, rl, skip=n % 61)
        d_rec = torch.from_numpy(flat).to(dev)
        ref = _plain(dev, flat, rl, n)
        z = ref[:, 2].cpu().numpy()
        filters, lo, hi = _filters(fmt, z)
        for name, f in filters.items():
            keep = _mask(rec, fmt, f, z)
            got = las_io.decode_points(d_rec, rl, n, SCALE, OFFSET, SHIFT, False, point_format=fmt, select=f)
            want = ref[torch.from_numpy(keep).to(dev)]
            tag = f'format {fmt}, {rl} B, n={n}, {name}'
            assert got.shape[0] == int(keep.sum()), f'{tag}: {got.shape[0]} kept, the numpy selection keeps {int(keep.sum())}'
            assert got.is_contiguous() and _same_bits(got, want), f'{tag}: kept points differ from the indexed plain decode'
            if name == 'everything':
                assert got.shape[0] == n
            if name == 'nothing':
                assert got.shape[0] == 0
            if name == 'z window' and n:
                # both bounds are heights of records: the ends are inclusive
                assert keep[z == np.float32(lo)].all() and keep[z == np.float32(hi)].all() and (z == np.float32(lo)).any() and (z == np.float32(hi)).any()
                assert bool((got[:, 2] == lo).any()) and bool((got[:, 2] == hi).any())
                if n >= 63:
                    assert 0 < got.shape[0] < n
        if n == 1000:
            counts = {k: int(_mask(rec, fmt, f, z).sum()) for k, f in filters.items()}
            print(f'format {fmt}, {rl} B, n={n}: kept {counts}')
            assert all(0 < counts[k] < n for k in ('classes 2, 11', 'withheld', 'first', 'last', 'single', 'z window')), counts


def test_normalised_intensity_and_out_buffer(dev):
    """read_las's intensity (normalise=True) and a caller's buffer: the rows of the plain decode again, the view is the buffer's head."""
    n, rl, fmt = 1000, 34, 3
    rec, flat = _records(n, rl)
    ref = _plain(dev, flat, rl, n, normalise=True)
    f = PointFilter(classes=range(0, 32, 3), returns='first')
    keep = _mask(rec, fmt, f, ref[:, 2].cpu().numpy())
    buf = torch.full((n, 4), -7.0, device=dev)
    got = las_io.decode_points(torch.from_numpy(flat).to(dev), rl, n, SCALE, OFFSET, SHIFT, True, out=buf, point_format=fmt, select=f)
    assert got.data_ptr() == buf.data_ptr() and got.shape[0] == int(keep.sum()) > 0
    assert _same_bits(got, ref[torch.from_numpy(keep).to(dev)])
    assert bool((buf[got.shape[0]:] == -7.0).all()), 'rows from kept on were written'
    with pytest.raises(ValueError, match='classes'):
        las_io.decode_points(torch.from_numpy(flat).to(dev), rl, n, SCALE, OFFSET, SHIFT, point_format=fmt, select=PointFilter(classes=[40]))


# ------------------------------------------------------------------------------------------------ 2. the overlap bit
@pytest.mark.parametrize('fmt, rl', [(1, 28), (6, 30)])
def test_drop_overlap_exists_from_format_6_on(dev, fmt, rl):
    n = 1000
    rec, flat = _records(n, rl)
    got = las_io.decode_points(torch.from_numpy(flat).to(dev), rl, n, SCALE, OFFSET, SHIFT, False, point_format=fmt,
                               select=PointFilter(drop_withheld=False, drop_overlap=True))
    ref = _plain(dev, flat, rl, n)
    if fmt < 6:
        assert _same_bits(got, ref), 'drop_overlap dropped points of a format that has no overlap bit'
    else:
        keep = (rec[:, 15] & 8) == 0
        assert 0 < keep.sum() < n and _same_bits(got, ref[torch.from_numpy(keep).to(dev)])


# ------------------------------------------------------------------------------------------------ 3. the class histogram
@pytest.mark.parametrize('fmt, rl, n', [(1, 28, 0), (1, 28, 1000), (6, 37, 1000), (0, 20, N_BIG), (6, 30, N_BIG)])
def test_class_histogram_counts_all_records(dev, fmt, rl, n):
    """Kept or not: the histogram is of the file.  N_BIG has more blocks than the count pass has workgroups, so a workgroup walks several."""
    rec, flat = _records(n, rl)
    f = PointFilter(classes=[2, 11])
    pts, hist = las_io.decode_points(torch.from_numpy(flat).to(dev), rl, n, SCALE, OFFSET, SHIFT, False, point_format=fmt, select=f,
                                     return_hist=True)
    cls = _fields(rec, fmt)[3]
    assert hist.dtype == np.int64 and hist.shape == (256,) and np.array_equal(hist, np.bincount(cls, minlength=256))
    assert int(hist.sum()) == n and pts.shape[0] == int(_mask(rec, fmt, f, None).sum())
    again = las_io.decode_points(torch.from_numpy(flat).to(dev), rl, n, SCALE, OFFSET, SHIFT, False, point_format=fmt, select=f)   # NULL histogram
    assert _same_bits(again, pts)


# ------------------------------------------------------------------------------------------------ 4. guarded buffers
def test_select_guards(dev):
    """lm_las_decode_select with records, output, workspace, count and histogram each between guard slabs: n = 257 records of 37 bytes
    (the last dword of the records is padding, the last block holds one record), about half of them kept.  The guards are intact, the
    output rows from `kept` on still hold the canary, poisoned guards change no output bit, and a second run gives the same bits."""
    L = lib()
    n, rl, fmt = 257, 37, 6
    rec, flat = _records(n, rl)
    f = PointFilter(classes=range(0, 256, 2), drop_withheld=False)
    ref = _plain(dev, flat, rl, n)
    keep = _mask(rec, fmt, f, ref[:, 2].cpu().numpy())
    kept = int(keep.sum())
    assert n // 3 < kept < 2 * n // 3
    need = L.lm_las_select_workspace_bytes(n)
    sel = f.as_struct()
    d3 = lambda v: (C.c_double * 3)(*v)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(B, poisoned):
        s_rec = Slab(dev, 1, len(flat), front=1, back=1, dtype=torch.uint8).fill_input(torch.from_numpy(flat), 0xFF if poisoned else 0)
        s_out = Slab(dev, kept, 4, front=64, back=n - kept + 64).fill_canary()          # rows kept .. n-1 are part of the back guard
        s_ws = Slab(dev, 1, need, front=1, back=1, dtype=torch.uint8).fill_canary()
        s_kept = Slab(dev, 1, 2, front=8, back=8, dtype=torch.int32).fill_canary()
        s_hist = Slab(dev, 256, 2, front=8, back=8, dtype=torch.int32).fill_canary()
        rc = L.lm_las_decode_select(stream, C.c_void_p(s_rec.ptr()), rl, fmt, n, d3(SCALE), d3(OFFSET), d3(SHIFT), 800.0, 33000.0, 0,
                                    C.byref(sel), C.c_void_p(s_ws.ptr()), need, C.c_void_p(s_out.ptr()), C.c_void_p(s_kept.ptr()),
                                    C.c_void_p(s_hist.ptr()))
        assert rc == 0, L.lm_last_error()
        return {'out': (s_out, kept), 'workspace': (s_ws, 1), 'kept': (s_kept, 1), 'hist': (s_hist, 256)}

    for attempt in range(2):                                             # the second round: the same bits again
        got = guarded_runs(run, 'las_decode_select', batch=False)
        assert int(got['kept'].numpy().view(np.int64)[0, 0]) == kept
        assert np.array_equal(got['hist'].numpy().view(np.int64)[:, 0], np.bincount(rec[:, 16], minlength=256))
        assert _same_bits(got['out'], ref[torch.from_numpy(keep).to(dev)].cpu())


# ------------------------------------------------------------------------------------------------ 5. end to end
OFF = np.array([351200.0, 3433000.0, 12.0])
ROAD_CLASS = 2


def _write_classified(path, world, inten, cls, withheld):
    """A LAS 1.4 format-6 file whose records carry return 1 of 1, the given classification and withheld flag, no other flag."""
    las_ref.write_las(path, world, inten, point_format=6, version=(1, 4), offset=tuple(OFF))
    data = np.fromfile(path, np.uint8)
    h = las_io.parse_header(data)
    assert h['point_format'] == 6 and h['record_len'] == 30 and h['n_points'] == len(world)
    rec = data[h['offset_to_points']:h['offset_to_points'] + 30 * len(world)].reshape(-1, 30)
    rec[:, 14] = 0x11
    rec[:, 15] = np.where(withheld, 4, 0)
    rec[:, 16] = cls
    data.tofile(path)


def _road_and_clutter(seed, n, trans, k=3000):
    """A synthetic road cloud in the tile frame moved by `trans`, and the same cloud with 3 k points strewn into its file order: k of
    class 7 (noise), k withheld, k sitting 6 m above the road; all with intensity 33000 over the lane-free asphalt at y < 2 m.
    -> (world, intensity) of the clean cloud, (world, intensity, class, withheld) of the dirty one."""
    pts = synth.las_points(seed, n).astype(np.float64)
    rng = np.random.RandomState(seed)
    x, y = rng.uniform(1.0, 56.0, 3 * k), rng.uniform(0.3, 2.0, 3 * k)
    z = 0.02 * x + 0.01 * y
    z[2 * k:] += 6.0
    junk = np.stack([x, y, z, np.full(3 * k, 33000.0)], axis=1)
    cls = np.full(n + 3 * k, ROAD_CLASS)
    cls[n:n + k] = 7
    withheld = np.zeros(n + 3 * k, bool)
    withheld[n + k:n + 2 * k] = True
    both = np.concatenate([pts, junk])
    order = np.argsort(np.concatenate([np.arange(n) + 0.5, rng.uniform(0, n, 3 * k)]), kind='stable')     # clean order kept
    both, cls, withheld = both[order], cls[order], withheld[order]
    move = np.asarray(trans) + OFF
    return (pts[:, :3] + move, pts[:, 3]), (both[:, :3] + move, both[:, 3], cls, withheld)


CLUTTER_FILTER = dict(classes=[c for c in range(256) if c != 7], z_range=(-1.0, 3.0))       # withheld points go by default


def test_filtered_dirty_tile_equals_the_clean_tile(dev, tmp_path):
    """The capability: noise, withheld and overhead returns of full intensity win their pixels in the rasteriser; read through the
    filter, the dirty file gives the tile of the clean one."""
    n = 300_000
    (cw, ci), (dw, di, cls, withheld) = _road_and_clutter(77, n, (0.0, 0.0, 0.0))
    clean, dirty = str(tmp_path / 'clean.las'), str(tmp_path / 'dirty.las')
    _write_classified(clean, cw, ci, np.full(n, ROAD_CLASS), np.zeros(n, bool))
    _write_classified(dirty, dw, di, cls, withheld)
    rpar = [ops.make_raster_params(local_min_ele=-0.5, ele_reso=0.02)]

    def tile(path, select, hist=False):
        pts, h = las_io.read_las_raw(path, dev, shift=OFF, select=select, class_hist=hist)
        _, u8 = ops.bev_raster_batch(pts, [0, pts.shape[0]], rpar, H, W, want_u8=True)
        return u8, pts, h

    want, p_clean, _ = tile(clean, None)
    got, p_sel, h = tile(dirty, PointFilter(**CLUTTER_FILTER), hist=True)
    unfiltered, p_all, h_all = tile(dirty, None)
    assert h['n_points'] == n + 9000 and h['n_kept'] == n and p_all.shape[0] == n + 9000 and 'n_kept' not in h_all
    assert int(h['class_hist'][7]) == 3000 and int(h['class_hist'][ROAD_CLASS]) == n + 6000 and int(h['class_hist'].sum()) == n + 9000
    assert _same_bits(p_sel, p_clean), 'the kept points are not the clean cloud in its file order'
    assert torch.equal(got, want), 'the filtered dirty tile differs from the clean tile'
    assert not torch.equal(unfiltered, want), 'the clutter changed no pixel: the test shows nothing'
    # each kind of clutter on its own reaches the tile too
    for name, kw in (('class 7', dict(drop_withheld=True, z_range=(-1.0, 3.0))), ('withheld', dict(CLUTTER_FILTER, drop_withheld=False)),
                     ('overhead', dict(classes=CLUTTER_FILTER['classes']))):
        part, _, hp = tile(dirty, PointFilter(**kw))
        assert hp['n_kept'] == n + 3000 and not torch.equal(part, want), f'{name} points alone change no pixel'
    with pytest.raises(ValueError, match='only 0 lidar points'):
        las_io.read_las(dirty, dev, shift=OFF, select=PointFilter(classes=[9]))
    assert _same_bits(las_io.read_las(dirty, dev, shift=OFF, select=PointFilter(**CLUTTER_FILTER)), las_io.read_las(clean, dev, shift=OFF))


def test_runner_strip_with_filter_on_dirty_file_equals_clean_file(dev, net, tmp_path):
    """Three overlapping tiles of one strip through Runner.infer_las_strip_to_map: the dirty strip with the filter writes the files of
    the clean strip without one, byte for byte; so does infer_las_to_map on the first tile."""
    from lanemapping_amd.runner import Runner
    n, names, plist = 200_000, [], []
    clean_parts, dirty_parts = [], []
    for t in range(3):
        trans = (3.0 + 40.0 * t, -2.0, 0.5)
        c, d = _road_and_clutter(900 + t, n, trans, k=2000)
        clean_parts.append(c)
        dirty_parts.append(d)
        plist.append({'coor_las_path': '', 'las_read_offset': list(OFF), 'las_rotation_trans_quan': list(trans) + [1.0, 0.0, 0.0, 0.0],
                      'bev_img_offset': [0.0, 0.0], 'img_reso': [0.05, 0.05], 'local_min_ele': -0.5, 'ele_reso': 0.02})
        names.append(f'18101{t}_0209_a')
    (tmp_path / 'clean_in').mkdir(), (tmp_path / 'dirty_in').mkdir()
    clean, dirty = str(tmp_path / 'clean_in' / 'strip_0209.las'), str(tmp_path / 'dirty_in' / 'strip_0209.las')     # (a tile's name comes from it)
    cw, ci = (np.concatenate([p[k] for p in clean_parts]) for k in range(2))
    dw, di, cls, withheld = (np.concatenate([p[k] for p in dirty_parts]) for k in range(4))
    _write_classified(clean, cw, ci, np.full(len(cw), ROAD_CLASS), np.zeros(len(cw), bool))
    _write_classified(dirty, dw, di, cls, withheld)
    prm = []
    for t in range(3):
        prm.append(str(tmp_path / (names[t] + '.txt')))
        io_utils.save_pc_2_img_transform_paras(prm[-1], plist[t])
    z_range = (-0.5, 4.0)                                             # the strip's frame: the tiles sit 0.5 m above the read offset
    sel = PointFilter(classes=CLUTTER_FILTER['classes'], z_range=z_range)
    r = Runner.__new__(Runner)
    r.cfg, r.device, r.net = net.cfg, dev, net
    assert r.cfg.get('las_select') is None
    outs = {k: str(tmp_path / k) for k in ('clean', 'arg', 'tile_clean', 'tile_arg')}
    lines_c, merged_c = r.infer_las_strip_to_map(clean, prm, work_dirs=outs['clean'], batch_size=2)
    lines_a, merged_a = r.infer_las_strip_to_map(dirty, prm, work_dirs=outs['arg'], batch_size=2, select=sel)
    r.infer_las_to_map([(clean, prm[0])], work_dirs=outs['tile_clean'], merge=False)
    r.infer_las_to_map([(dirty, prm[0])], work_dirs=outs['tile_arg'], merge=False, select=sel)
    assert sorted(lines_a) == sorted(lines_c) and len(lines_c) >= 1 and len(merged_a) == len(merged_c)
    for k in lines_c:
        assert len(lines_a[k]) == len(lines_c[k]) and all(np.array_equal(a, b) for a, b in zip(lines_a[k], lines_c[k]))
    assert all(np.array_equal(a, b) for a, b in zip(merged_a, merged_c))

    def tree(root):
        return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), 'rb').read() for d, _, fs in os.walk(root) for f in fs}

    want = tree(outs['clean'])
    assert len(want) >= 4 and tree(outs['arg']) == want
    assert tree(outs['tile_arg']) == tree(outs['tile_clean']) and len(tree(outs['tile_clean'])) >= 1
