"""CPU: the host half of the chunked strip route - las_io.LasChunks (the file's records chunk by chunk, without a device),
las_io.StripStream's argument checks, las_io.tile_groups on hand-made counts, the Runner's refusals, and the header's NOTE."""
import os
import re

import numpy as np
import pytest

from lanemapping_amd import las_io
from lanemapping_amd._lib import SIGNATURES, LanemapHipError
from oracle import las_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write(path, n, point_format=0, extra_bytes=1, vlr_bytes=0, tail=b''):
    rng = np.random.RandomState(n + 7 * point_format)
    xyz = rng.uniform(-50, 50, (n, 3))
    las_ref.write_las(str(path), xyz, rng.randint(0, 60000, n), point_format=point_format, version=(1, 4) if point_format >= 6 else (1, 2),
                      extra_bytes=extra_bytes, vlr_bytes=vlr_bytes)
    if tail:
        with open(path, 'ab') as f:
            f.write(tail)
    return np.fromfile(str(path), dtype=np.uint8)


@pytest.mark.parametrize('point_format,extra', [(0, 1), (6, 1), (0, 0)], ids=['format 0, 21 B', 'format 6, 31 B', 'format 0, 20 B'])
@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 3 * 256])
def test_chunks_are_the_records_of_the_file(tmp_path, n, point_format, extra):
    """Every chunk holds the bytes of its records, zero-padded to four bytes (an odd record length pads most chunks); the chunks are
    consecutive, only the last is short; a second iteration reads the same."""
    data = _write(tmp_path / 'a.las', n, point_format, extra, vlr_bytes=54, tail=b'EVLR-bytes-after-the-records')
    chunks = las_io.LasChunks(tmp_path / 'a.las', 256)
    h = chunks.header
    assert h == las_io.parse_header(data) and h['n_points'] == n and h['record_len'] == las_ref.RECORD_LEN[point_format] + extra
    off, rl = h['offset_to_points'], h['record_len']
    assert len(chunks) == -(-n // 256)
    for again in range(2):
        first_want, seen = 0, 0
        for rec, m, first in chunks:
            assert isinstance(rec, np.ndarray) and rec.dtype == np.uint8
            assert first == first_want and 1 <= m <= 256 and (m == 256 or first + m == n)
            assert len(rec) == (m * rl + 3) // 4 * 4
            assert np.array_equal(rec[:m * rl], data[off + first * rl:off + (first + m) * rl]), f'chunk at record {first}, iteration {again}'
            assert not rec[m * rl:].any(), 'the padding is zero'
            first_want, seen = first + m, seen + 1
        assert first_want == n and seen == len(chunks)
    assert chunks.head_bytes == data[:off].tobytes() and len(chunks.head_bytes) == (375 if point_format >= 6 else 227) + 54
    assert chunks.tail_bytes == b'EVLR-bytes-after-the-records'


def test_a_chunk_size_that_divides_nothing_evenly(tmp_path):
    """chunk_records = 512 over 1300 records of 21 bytes: chunk starts that are no multiple of four bytes in the file."""
    data = _write(tmp_path / 'b.las', 1300, 0, 1)
    chunks = las_io.LasChunks(str(tmp_path / 'b.las'), 512)
    off = chunks.header['offset_to_points']
    got = [(m, first, rec[:m * 21].copy()) for rec, m, first in chunks]
    assert [(m, f) for m, f, _ in got] == [(512, 0), (512, 512), (276, 1024)]
    assert np.array_equal(np.concatenate([r for _, _, r in got]), data[off:off + 1300 * 21])


@pytest.mark.parametrize('bad', [0, -256, 255, 257, 384 + 1, 256.0, True, None, '256'])
def test_chunk_records_must_be_a_positive_multiple_of_256(tmp_path, bad):
    _write(tmp_path / 'c.las', 10)
    with pytest.raises(ValueError, match='chunk_records'):
        las_io.LasChunks(tmp_path / 'c.las', bad)
    with pytest.raises(ValueError, match='chunk_records'):
        las_io.StripStream(chunk_records=bad)


def test_a_truncated_file_is_refused_with_both_byte_counts(tmp_path):
    data = _write(tmp_path / 'd.las', 1000, 0, 1)
    whole = len(data)
    assert whole == 227 + 1000 * 21
    data[:whole - 5].tofile(str(tmp_path / 'short.las'))
    with pytest.raises(LanemapHipError, match=rf'truncated.*{whole} bytes.*{whole - 5}'):
        las_io.LasChunks(tmp_path / 'short.las', 256)
    data[:100].tofile(str(tmp_path / 'stub.las'))
    with pytest.raises(LanemapHipError, match='not a LAS file'):
        las_io.LasChunks(tmp_path / 'stub.las', 256)
    las_io.LasChunks(tmp_path / 'd.las', 256)                      # exactly long enough


def test_more_records_than_one_call_takes_are_accepted(tmp_path, monkeypatch):
    """A LAS 1.4 header that announces 2^31 + 5 records, over a file the file system reports long enough (64 GB are not written here):
    the object is built and its chunks are counted; the same header over the file as it is, is a truncated file."""
    n = (1 << 31) + 5
    _write(tmp_path / 'e.las', 4, 6, 0)
    with open(tmp_path / 'e.las', 'r+b') as f:
        f.seek(247)
        f.write(np.array([n], dtype='<u8').tobytes())
    with pytest.raises(LanemapHipError, match=rf'truncated.*{375 + n * 30} bytes.*{375 + 4 * 30}'):
        las_io.LasChunks(tmp_path / 'e.las', 1 << 24)
    monkeypatch.setattr(las_io.os.path, 'getsize', lambda p: 375 + n * 30)
    chunks = las_io.LasChunks(tmp_path / 'e.las', 1 << 24)
    assert chunks.header['n_points'] == n and len(chunks) == 129 and chunks.record_bytes == n * 30


def test_strip_stream_arguments():
    s = las_io.StripStream()
    assert (s.chunk_records, s.binned_budget) == (1 << 24, None) and s == las_io.StripStream(1 << 24, None)
    assert eval(repr(s), {'StripStream': las_io.StripStream}) == s and hash(s) == hash(las_io.StripStream())
    t = las_io.StripStream(chunk_records=512, binned_budget=1 << 20)
    assert (t.chunk_records, t.binned_budget) == (512, 1 << 20) and t != s and t._replace(binned_budget=None).binned_budget is None
    with pytest.raises(AttributeError, match='StripStream is immutable'):
        t.chunk_records = 256
    for bad in (0, -1, 1.5, True, '1000'):
        with pytest.raises(ValueError, match='binned_budget'):
            las_io.StripStream(binned_budget=bad)
    assert issubclass(las_io.StripStream, las_io._Options)


def test_tile_groups_on_hand_made_counts():
    g = las_io.tile_groups
    counts = [10, 20, 30, 40, 50, 60, 70]
    assert g(counts, 2, None) == [(0, 7)] and g([], 2, 100) == [] and g([], 2, None) == []
    # a budget smaller than any batch: every batch on its own, never a cut inside a batch
    assert g(counts, 2, 16) == [(0, 2), (2, 4), (4, 6), (6, 7)]
    assert g(counts, 3, 1) == [(0, 3), (3, 6), (6, 7)]
    # exactly reached: batches (10 + 20) and (30 + 40) are 16 * 100 bytes together, within a budget of 1600 and not of 1599
    assert g(counts, 2, 1600) == [(0, 4), (4, 6), (6, 7)]
    assert g(counts, 2, 1599) == [(0, 2), (2, 4), (4, 6), (6, 7)]
    assert g(counts, 2, 16 * 280) == [(0, 7)] and g(counts, 2, 16 * 280 - 1) == [(0, 6), (6, 7)]
    # empty tiles cost nothing: they ride along, and an all-empty layout is one group whatever the budget
    assert g([0, 0, 0, 0, 100, 0, 0, 0], 2, 1600) == [(0, 8)]
    assert g([0, 0, 100, 0, 0, 0, 100, 0], 2, 1600) == [(0, 6), (6, 8)]
    assert g([0] * 5, 2, 1) == [(0, 5)]
    # batch 1, and a batch larger than the layout
    assert g([5, 5, 5], 1, 160) == [(0, 2), (2, 3)] and g([5, 5, 5], 8, 1) == [(0, 3)]
    for groups in (g(counts, 2, 16), g(counts, 2, 1600), g([0, 0, 100, 0, 0, 0, 100, 0], 2, 1600)):
        assert groups[0][0] == 0 and all(a[1] == b[0] for a, b in zip(groups, groups[1:])) and all(t0 % 2 == 0 for t0, _ in groups)
    with pytest.raises(ValueError, match='batch'):
        g(counts, 0, 100)


def _runner(cfg=None):
    from lanemapping_amd.runner import Runner
    from lanemapping_amd.config import Config
    r = Runner.__new__(Runner)
    r.cfg, r.device, r.net = Config(dict({'list_img_size_xy': [1152, 1152]}, **(cfg or {}))), 'cpu', None
    return r


def test_the_runner_checks_stream_before_anything_runs(tmp_path):
    r = _runner()
    with pytest.raises(TypeError, match='stream must be a las_io.StripStream'):
        r.infer_las_strip_to_map('none.las', [], stream={'chunk_records': 256})
    with pytest.raises(ValueError, match='chunk_records'):
        _runner({'las_stream': {'chunk_records': 100}}).infer_las_strip_to_map('none.las', [])
    # scope='strip' with a budget and more tiles than one batch: refused by name before any file is opened (none of these exists)
    prm = []
    for t in range(4):
        prm.append(str(tmp_path / f'18103{t}_0209.txt'))
        from lanemapping_amd import io_utils
        io_utils.save_pc_2_img_transform_paras(prm[t], {'coor_las_path': '', 'las_read_offset': [0.0, 0.0, 0.0],
                                                        'las_rotation_trans_quan': [50.0 * t, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], 'bev_img_offset': [0.0, 0.0],
                                                        'img_reso': [0.05, 0.05], 'local_min_ele': -0.5, 'ele_reso': 0.05})
    with pytest.raises(ValueError, match='binned_budget'):
        r.infer_las_strip_to_map(str(tmp_path / 'missing.las'), prm, work_dirs=str(tmp_path / 'out'), batch_size=2,
                                 intensity=las_io.IntensityStretch(scope='strip'), stream=las_io.StripStream(256, binned_budget=1 << 20))


def test_the_header_declares_the_chunk_entries_with_the_stream_last():
    text = open(os.path.join(ROOT, 'include', 'lanemap_hip.h')).read()
    for name, n in (('lm_strip_plan_create', 10), ('lm_strip_bin_count', 7), ('lm_strip_bin_scatter', 10)):
        m = re.search(r'\b' + name + r'\(([^)]*)\);', text)
        params = [' '.join(p.split()) for p in m.group(1).split(',')]
        assert params[-1] == 'void* hip_stream' and len(params) == len(SIGNATURES[name][1]) == n, name
    assert 'NOTE on the place of `hip_stream`' in text[text.index('strip binning, chunk by chunk'):text.index('lm_strip_plan_consts_bytes(int T')]
