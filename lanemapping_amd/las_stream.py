"""A strip larger than memory: LAS files read in chunks, and the plan of the chunked strip route (reached as las_io.LasChunks,
las_io.StripStream, las_io.tile_groups; built on las_io and so imported by it on first use, like threshold.py).

`LasChunks(path, chunk_records, device)` reads the point records of a LAS file as consecutive runs of `chunk_records` records: the
header from the first bytes of the file, the records with readinto() into two alternating buffers on one helper thread that runs one
chunk ahead (pinned buffers and an asynchronous upload when a device is given).  The file is never held whole, and its record count is
not bounded - only a chunk's is.

`StripStream` switches Runner.infer_las_strip_to_map to the chunked route (`stream=`): pass A decodes and counts every chunk
(ops.StripBinner), the tiles are cut into groups whose binned points fit a budget (`tile_groups`), pass B reads the files again and
scatters them for one group at a time; the record passes after the merge go through the files chunk by chunk as well."""
import ctypes as C
import os

import numpy as np
import torch

from . import las_io
from ._lib import lib, check, LmLasHeader, LanemapHipError

HEADER_BYTES = 375                  # the public header block of LAS 1.4, the longest there is
CHUNK_MULTIPLE = 256                # records per workgroup of the record kernels: every chunk but the last is whole workgroups


def _check_chunk_records(who, chunk_records):
    if not las_io._whole(chunk_records) or int(chunk_records) <= 0 or int(chunk_records) % CHUNK_MULTIPLE:
        raise ValueError(f'{who}: chunk_records={chunk_records!r} must be a positive multiple of {CHUNK_MULTIPLE}')
    return int(chunk_records)


class StripStream(las_io._Options):
    """How Runner.infer_las_strip_to_map maps a strip that does not fit in memory (immutable; `stream=`).

      chunk_records   the records read, uploaded, decoded and binned at a time: a positive multiple of 256.  Device memory per chunk is
                      its records, a scratch cloud of 16 bytes per record and the binning's table
      binned_budget   None, or the bytes (whole number > 0) the binned points of one group of tiles may take: the tiles are cut, in layout
                      order and at multiples of the batch size, into groups with 16 * sum(counts) <= binned_budget, and the files are
                      read once more per group.  A batch that alone exceeds the budget is a group of its own.  None: one group
    Both defaults are plain defaults, not tuned values."""
    __slots__ = ('chunk_records', 'binned_budget')

    def __init__(self, chunk_records=1 << 24, binned_budget=None):
        chunk_records = _check_chunk_records('StripStream', chunk_records)
        if binned_budget is not None:
            if not las_io._whole(binned_budget) or int(binned_budget) <= 0:
                raise ValueError(f'StripStream: binned_budget={binned_budget!r} must be None or a whole number of bytes > 0')
            binned_budget = int(binned_budget)
        self._set(chunk_records=chunk_records, binned_budget=binned_budget)


def tile_groups(counts, batch, binned_budget):
    """The tiles of a layout cut into groups for pass B: counts, the points of every tile (pass A); batch, the batch size; -> a list of
    (t0, t1), consecutive runs that cover 0 .. len(counts), every cut at a multiple of `batch`.  A group takes whole batches as long as
    16 * sum(counts) of its tiles stays within binned_budget (reaching it exactly is within); a batch that alone exceeds the budget is a
    group of its own.  binned_budget None: one group.  No tiles: no group."""
    counts = [int(c) for c in counts]
    T, batch = len(counts), int(batch)
    if batch < 1 or any(c < 0 for c in counts):
        raise ValueError(f'tile_groups: batch={batch} must be >= 1 and no count negative')
    if T == 0:
        return []
    if binned_budget is None:
        return [(0, T)]
    groups, t0, size = [], 0, 0
    for b0 in range(0, T, batch):
        need = 16 * sum(counts[b0:b0 + batch])
        if b0 > t0 and size + need > binned_budget:
            groups.append((t0, b0))
            t0, size = b0, 0
        size += need
    groups.append((t0, T))
    return groups


class LasChunks:
    """The point records of the LAS file `path`, `chunk_records` at a time (a positive multiple of 256).

    header          las_io.parse_header's dict, read off the first bytes of the file
    iteration       yields (records, n, first) for consecutive runs of chunk_records records, the last one shorter: records = the n
                    records from number `first` on as uint8, zero-padded to a multiple of four bytes - a tensor on `device` (uploaded
                    asynchronously from a pinned buffer), or with device=None a numpy view of the read buffer, valid until the next chunk
                    is asked for.  A file without records yields nothing.  The object may be iterated again: the file is read again
    head_bytes      the bytes before the records (header, VLRs); tail_bytes: the bytes after them (EVLRs)
    A file shorter than its header says is refused with both byte counts; more than 2^31 - 1 records are accepted."""

    def __init__(self, path, chunk_records, device=None):
        self.chunk_records = _check_chunk_records('LasChunks', chunk_records)
        self.path = os.fspath(path)
        self.device = None if device is None else torch.device(device)
        self.size = os.path.getsize(self.path)
        with open(self.path, 'rb') as f:
            head = f.read(HEADER_BYTES)
        if len(head) < 227 or head[:4] != b'LASF':
            raise LanemapHipError(f'{self.path}: not a LAS file')
        block = np.zeros(HEADER_BYTES, dtype=np.uint8)                          # a shorter header (LAS 1.0 - 1.3: 227 / 235 bytes) is padded
        block[:len(head)] = np.frombuffer(head, dtype=np.uint8)
        h = LmLasHeader()
        # (the length lm_las_parse_header checks the point data against is the file's, checked below with both numbers in the message)
        check(lib().lm_las_parse_header(C.c_void_p(block.ctypes.data), 1 << 62, C.byref(h)))
        self.header = {'version': (h.version_major, h.version_minor), 'point_format': h.point_format, 'record_len': h.record_len,
                       'n_points': h.n_points, 'offset_to_points': h.offset_to_points, 'scale': list(h.scale), 'offset': list(h.offset),
                       'min': list(h.min_xyz), 'max': list(h.max_xyz)}
        self.record_bytes = int(h.n_points) * int(h.record_len)
        expected = int(h.offset_to_points) + self.record_bytes
        if self.size < expected:
            raise LanemapHipError(f'{self.path}: truncated LAS file: {h.n_points} records of {h.record_len} B from byte {h.offset_to_points} '
                                  f'need {expected} bytes, the file has {self.size}')
        self._bufs = None

    def __len__(self):
        """The number of chunks."""
        return -(-int(self.header['n_points']) // self.chunk_records)

    @property
    def head_bytes(self):
        with open(self.path, 'rb') as f:
            return f.read(self.header['offset_to_points'])

    @property
    def tail_bytes(self):
        with open(self.path, 'rb') as f:
            f.seek(self.header['offset_to_points'] + self.record_bytes)
            return f.read()

    def _buffers(self):
        if self._bufs is None:
            cap = (min(self.chunk_records, max(int(self.header['n_points']), 1)) * self.header['record_len'] + 3) // 4 * 4
            pin = self.device is not None and self.device.type == 'cuda'
            self._bufs = [torch.empty(cap, dtype=torch.uint8, pin_memory=pin) for _ in range(2)]
        return self._bufs

    def __iter__(self):
        from concurrent.futures import ThreadPoolExecutor
        n, rl, c = int(self.header['n_points']), int(self.header['record_len']), self.chunk_records
        if n == 0:
            return
        bufs, events = self._buffers(), [None, None]

        def read(f, k):
            """Chunk k into buffer k & 1, once the last upload out of that buffer has finished."""
            slot, m = k & 1, min(c, n - k * c)
            if events[slot] is not None:
                events[slot].synchronize()
            view, nb, at = bufs[slot].numpy(), m * rl, 0
            while at < nb:
                got = f.readinto(memoryview(view)[at:nb])
                if not got:
                    raise LanemapHipError(f'{self.path}: the file ended {nb - at} bytes into chunk {k}')
                at += got
            padded = (nb + 3) // 4 * 4
            view[nb:padded] = 0
            return slot, m, padded

        with open(self.path, 'rb') as f, ThreadPoolExecutor(max_workers=1) as pool:
            f.seek(self.header['offset_to_points'])
            fut = pool.submit(read, f, 0)
            for k in range(len(self)):
                slot, m, padded = fut.result()
                if k + 1 < len(self):
                    fut = pool.submit(read, f, k + 1)
                if self.device is None:
                    yield bufs[slot].numpy()[:padded], m, k * c
                    continue
                rec = bufs[slot][:padded].to(self.device, non_blocking=True)
                if self.device.type == 'cuda':
                    events[slot] = torch.cuda.Event()
                    events[slot].record(torch.cuda.current_stream(self.device))
                yield rec, m, k * c


def empty_records(device):
    """What a file without records hands a record pass: no bytes, on the device."""
    return torch.zeros((0,), dtype=torch.uint8, device=device)
