#!/usr/bin/env python3
"""Micro-bench of the labelling (csrc/label.hip) on the bench's shape: 16 tiles x 4,194,304 synthetic points (synth.las_points, the tiles
laid along x) as [N,4] float32 and as 20- and 34-byte LAS records, eight lines along the strip with a vertex every 0.6 m.

Times, in one process, with HIP events, after a warm-up, over at least 20 repetitions each and alternating in every round:
  lm_label_points            16 N read, 4 N (labels) or 8 N (labels + dist2) written
  lm_las_label_records       2 N record_len (+ 4 N with `line`), with and without a select, in place and out of place
  lm_las_decode_points       N (record_len + 16): the plain decode of the same records
  lm_las_decode_select       2 N record_len + 16 kept: the other entry that reads the records twice
  device-to-device copy      2 N record_len: the copy of the same bytes
and prints the times, the algorithmic GB/s and the ratios; `--out PATH` also writes them to a file (profiles/label.txt holds one)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lanemapping_amd import las_io, ops, synth  # noqa: E402
from lanemapping_amd._lib import lib  # noqa: E402

EXTENT, TILES, N_TILE = 57.6, 16, 4194304


def strip_cloud(dev, tiles, n_tile):
    """-> [tiles * n_tile, 4] f32 on dev: four seeded clouds reused along x like the bench reuses them over its batch."""
    clouds = [torch.from_numpy(synth.las_points(2021 + i, n_tile)).to(dev) for i in range(min(4, tiles))]
    parts = []
    for t in range(tiles):
        c = clouds[t % len(clouds)].clone()
        c[:, 0] += EXTENT * t
        parts.append(c)
    return torch.cat(parts)


def strip_lines(tiles):
    """Eight lines along the strip, a vertex every 0.6 m, on the clouds' surface z = 0.02 (x mod 57.6) + 0.01 y."""
    x = np.arange(0.0, EXTENT * tiles + 0.3, 0.6)
    lines = []
    for l in range(8):
        y = (0.1 + 0.1 * l) * EXTENT + 0.5 * np.sin(x / 40.0 + l)
        lines.append(np.stack([x, y, 0.02 * np.mod(x, EXTENT) + 0.01 * y], axis=1))
    return lines


def records_of(cloud, rl):
    """[N,4] f32 -> N records of rl bytes on the device (padded to 4 bytes): X Y Z int32 at 1 mm, intensity u16, return 1 of 1, class 2
    for three records of four and 7 for the fourth (what a select on class 2 drops)."""
    n = cloud.shape[0]
    rec = torch.zeros((n, rl), dtype=torch.uint8, device=cloud.device)
    q = torch.round(cloud[:, :3].double() / 1e-3).to(torch.int32).contiguous()
    rec[:, 0:12] = q.view(torch.uint8).reshape(n, 12)
    rec[:, 12:14] = cloud[:, 3].clamp(0, 65535).to(torch.int32).to(torch.int16).contiguous().view(torch.uint8).reshape(n, 2)
    rec[:, 14] = 0x11
    rec[:, 15] = torch.where(torch.arange(n, device=cloud.device) % 4 == 3, 7, 2).to(torch.uint8)
    flat = torch.zeros(((n * rl + 3) // 4 * 4,), dtype=torch.uint8, device=cloud.device)
    flat[:n * rl] = rec.reshape(-1)
    return flat


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=TILES)
    ap.add_argument('--points', type=int, default=N_TILE)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=4, help='calls per round and kind: rounds x calls >= 20 repetitions')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.rounds * args.calls >= 20, 'at least 20 repetitions'
    dev = torch.device('cuda:0')
    L = lib()
    cloud = strip_cloud(dev, args.tiles, args.points)
    N = cloud.shape[0]
    lines = strip_lines(args.tiles)
    labels = las_io.MarkingLabels()
    seg = las_io.line_segments(lines)
    index = ops.line_index(seg, labels.half_width, device=dev)
    nl = len(lines)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    d3 = C.c_double * 3
    scale, offset = d3(1e-3, 1e-3, 1e-3), d3(0.0, 0.0, 0.0)
    flt = las_io.PointFilter(classes=[2], drop_withheld=False)
    sel = flt.as_struct()
    out_lines = [f'bench_label: {args.tiles} tiles x {args.points} points = {N} points, {nl} lines, {len(seg)} segments, grid '
                 f'{index.grid.nx} x {index.grid.ny} cells of {index.grid.cell:g} m, {index.grid.n_entries} list entries; '
                 f'{args.rounds} rounds x {args.calls} calls, HIP events, warm']
    line = torch.empty(N, dtype=torch.int32, device=dev)
    dist2 = torch.empty(N, dtype=torch.float32, device=dev)
    pts_out = torch.empty((N, 4), dtype=torch.float32, device=dev)
    counts = torch.empty(nl + 1, dtype=torch.int64, device=dev)
    kinds = {}

    def points(with_d2):
        def fn():
            rc = L.lm_label_points(stream, C.c_void_p(cloud.data_ptr()), N, *index.args(), labels.z_tol, float('nan'), C.c_void_p(line.data_ptr()),
                                   C.c_void_p(dist2.data_ptr()) if with_d2 else None)
            assert rc == 0, L.lm_last_error()
        return fn

    kinds['label_points'] = (points(False), 20 * N)
    kinds['label_points +dist2'] = (points(True), 24 * N)
    for fmt, rl in ((0, 20), (3, 34)):
        rec = records_of(cloud, rl)
        rec_out = torch.empty_like(rec)
        need = L.lm_las_select_workspace_bytes(N)
        ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
        meta = torch.empty(257, dtype=torch.int64, device=dev)

        def label(rec=rec, rec_out=rec_out, rl=rl, fmt=fmt, select=None, want_line=False):
            def fn():
                rc = L.lm_las_label_records(stream, C.c_void_p(rec.data_ptr()), rl, fmt, N, scale, offset, None,
                                            C.byref(select) if select is not None else None, *index.args(), labels.z_tol, float('nan'),
                                            labels.for_format(fmt), 1, C.c_void_p(rec_out.data_ptr()),
                                            C.c_void_p(line.data_ptr()) if want_line else None, C.c_void_p(counts.data_ptr()), nl)
                assert rc == 0, L.lm_last_error()
            return fn

        def decode(rec=rec, rl=rl):
            las_io.decode_points(rec, rl, N, [1e-3] * 3, [0.0] * 3, None, False, out=pts_out)

        def decode_select(rec=rec, rl=rl, fmt=fmt, ws=ws, need=need, meta=meta):
            rc = L.lm_las_decode_select(stream, C.c_void_p(rec.data_ptr()), rl, fmt, N, scale, offset, None, las_io.INTEN_MIN, las_io.INTEN_MAX, 0,
                                        C.byref(sel), C.c_void_p(ws.data_ptr()), need, C.c_void_p(pts_out.data_ptr()), C.c_void_p(meta.data_ptr()),
                                        None)
            assert rc == 0, L.lm_last_error()

        def copy(rec=rec, rec_out=rec_out):
            rec_out.copy_(rec)

        kinds[f'label_records {rl} B'] = (label(), 2 * N * rl)
        kinds[f'label_records {rl} B +select'] = (label(select=sel), 2 * N * rl)
        kinds[f'label_records {rl} B +line'] = (label(want_line=True), 2 * N * rl + 4 * N)
        own = rec.clone()                            # records == records_out: the call patches this copy, the other rows keep `rec`
        kinds[f'label_records {rl} B in place'] = (label(rec=own, rec_out=own), 2 * N * rl)
        kinds[f'decode_points {rl} B'] = (decode, N * (rl + 16))
        kinds[f'decode_select {rl} B'] = (decode_select, 2 * N * rl + 16 * (3 * N // 4))
        kinds[f'copy d2d {rl} B'] = (copy, 2 * N * rl)
    for fn, _ in kinds.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    labelled = int((line > 0).sum())
    out_lines.append(f'labelled points: {labelled} of {N} ({100.0 * labelled / N:.2f} %); counts of the last record call: {counts.cpu().tolist()}')
    ms = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k, (fn, _) in kinds.items():
            ms[k].append(timed(fn, args.calls))
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    out_lines.append(f'{"kind":36s} {"ms":>9s} {"min":>9s} {"max":>9s} {"GB/s":>8s}   (algorithmic bytes)')
    for k, v in ms.items():
        out_lines.append(f'{k:36s} {mean[k]:9.3f} {min(v):9.3f} {max(v):9.3f} {kinds[k][1] / mean[k] / 1e6:8.0f}')
    out_lines.append('ratios of the mean times:')
    for rl in (20, 34):
        lab = mean[f'label_records {rl} B']
        out_lines.append(f'  label_records {rl} B / decode_points {lab / mean[f"decode_points {rl} B"]:.2f}, / copy d2d {lab / mean[f"copy d2d {rl} B"]:.2f}, '
                         f'/ decode_select {lab / mean[f"decode_select {rl} B"]:.2f}; +select / decode_select '
                         f'{mean[f"label_records {rl} B +select"] / mean[f"decode_select {rl} B"]:.2f}')
        out_lines.append(f'  label_points / decode_points {rl} B {mean["label_points"] / mean[f"decode_points {rl} B"]:.2f}, / copy d2d {rl} B '
                         f'{mean["label_points"] / mean[f"copy d2d {rl} B"]:.2f}, / decode_select {rl} B {mean["label_points"] / mean[f"decode_select {rl} B"]:.2f}')
    text = '\n'.join(out_lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
