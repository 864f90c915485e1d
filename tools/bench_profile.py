#!/usr/bin/env python3
"""Micro-bench of the marking profile (csrc/profile.hip) on the bench's shape, beside the labelling it shares its reads and search with:
16 tiles x 4,194,304 synthetic points (tools/bench_label.py's cloud, lines and records), profiled at bin = 0.25 m.

Times, in one process, with HIP events, after a warm-up, over at least 20 repetitions each and alternating in every round:
  lm_label_points               the parent's kernel: the same 16 N read and the same search, 4 N written
  lm_line_profile_points        16 N read, the bins written; fresh (accumulate = 0) and adding (accumulate = 1)
  lm_las_label_records          2 N record_len
  lm_las_line_profile_records   N record_len read
  device-to-device copy         of the cloud (2 x 16 N) and of the records (2 N record_len)
on the cloud as drawn (every wave's 64 points spread over a whole tile) and on the same points in 0.5 m cell order (the points of a wave
are neighbours on the ground, as in a file in acquisition order).  `--out PATH` also writes the table to a file
(profiles/marking_profile.txt holds one)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_label import N_TILE, TILES, records_of, strip_cloud, strip_lines, timed  # noqa: E402
from lanemapping_amd import las_io, ops  # noqa: E402
from lanemapping_amd._lib import lib  # noqa: E402


def cell_order(cloud, n_tile, cell=0.5):
    """The same points, each tile's sorted by the 0.5 m cell they lie in (x-major; the tiles follow each other along x): neighbours in
    memory are neighbours on the ground.  Sorted on the host, tile by tile."""
    host = cloud.cpu().numpy()
    for i in range(0, len(host), n_tile):
        part = host[i:i + n_tile]
        key = np.floor(part[:, 0] / cell).astype(np.int64) * 4096 + np.clip(np.floor(part[:, 1] / cell), 0, 4095).astype(np.int64)
        host[i:i + n_tile] = part[np.argsort(key, kind='stable')]
    return torch.from_numpy(host).to(cloud.device)


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
    survey = las_io.MarkingSurvey()
    lines = strip_lines(args.tiles)
    seg = las_io.line_segments(lines)
    st, bs = las_io.line_stations(lines, None, survey.bin)
    index = ops.line_index(seg, survey.half_width, device=dev)
    stations = ops.line_stations(st, bs, survey.bin, device=dev)
    label_index = ops.line_index(seg, las_io.MarkingLabels().half_width, device=dev)
    clouds = {'as drawn': strip_cloud(dev, args.tiles, args.points)}
    clouds['cell order'] = cell_order(clouds['as drawn'], args.points)
    N = clouds['as drawn'].shape[0]
    nl = len(lines)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    d3 = C.c_double * 3
    scale, offset = d3(1e-3, 1e-3, 1e-3), d3(0.0, 0.0, 0.0)
    nan = float('nan')
    out_lines = [f'bench_profile: {args.tiles} tiles x {args.points} points = {N} points, {nl} lines, {len(seg)} segments, {stations.n_bins} bins of '
                 f'{survey.bin} m, half_width {survey.half_width} m (label rows: {float(label_index.half_width):g} m), grid {index.grid.nx} x '
                 f'{index.grid.ny} cells; {args.rounds} rounds x {args.calls} calls, HIP events, warm']
    line = torch.empty(N, dtype=torch.int32, device=dev)
    bins = stations.new_bins()
    counts = torch.empty(nl + 1, dtype=torch.int64, device=dev)
    kinds = {}

    def label_points(cloud, idx):
        def fn():
            rc = L.lm_label_points(stream, C.c_void_p(cloud.data_ptr()), N, *idx.args(), survey.z_tol, nan, C.c_void_p(line.data_ptr()), None)
            assert rc == 0, L.lm_last_error()
        return fn

    def profile_points(cloud, accumulate):
        def fn():
            rc = L.lm_line_profile_points(stream, C.c_void_p(cloud.data_ptr()), N, *index.args(), *stations.args(), survey.z_tol, nan, accumulate,
                                          C.c_void_p(bins.data_ptr()), stations.n_bins)
            assert rc == 0, L.lm_last_error()
        return fn

    for name, cloud in clouds.items():
        spare = torch.empty_like(cloud)
        kinds[f'label_points, {name}'] = (label_points(cloud, index), 20 * N)
        kinds[f'label_points hw {float(label_index.half_width):g}, {name}'] = (label_points(cloud, label_index), 20 * N)
        kinds[f'line_profile_points, {name}'] = (profile_points(cloud, 0), 16 * N)
        kinds[f'line_profile_points +=, {name}'] = (profile_points(cloud, 1), 16 * N)
        kinds[f'copy d2d cloud, {name}'] = ((lambda cloud=cloud, spare=spare: spare.copy_(cloud)), 32 * N)
        for fmt, rl in ((0, 20), (3, 34)):
            rec = records_of(cloud, rl)
            rec_out = torch.empty_like(rec)

            def label_records(rec=rec, rec_out=rec_out, rl=rl, fmt=fmt):
                rc = L.lm_las_label_records(stream, C.c_void_p(rec.data_ptr()), rl, fmt, N, scale, offset, None, None, *index.args(), survey.z_tol,
                                            nan, 31, 1, C.c_void_p(rec_out.data_ptr()), None, C.c_void_p(counts.data_ptr()), nl)
                assert rc == 0, L.lm_last_error()

            def profile_records(rec=rec, rl=rl, fmt=fmt):
                rc = L.lm_las_line_profile_records(stream, C.c_void_p(rec.data_ptr()), rl, fmt, N, scale, offset, None, None, *index.args(),
                                                   *stations.args(), survey.z_tol, nan, 0, C.c_void_p(bins.data_ptr()), stations.n_bins)
                assert rc == 0, L.lm_last_error()

            kinds[f'label_records {rl} B, {name}'] = (label_records, 2 * N * rl)
            kinds[f'line_profile_records {rl} B, {name}'] = (profile_records, N * rl)
            kinds[f'copy d2d {rl} B, {name}'] = ((lambda rec=rec, rec_out=rec_out: rec_out.copy_(rec)), 2 * N * rl)
    for fn, _ in kinds.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    profile_points(clouds['as drawn'], 0)()
    host = bins.cpu().numpy()
    out_lines.append(f'profiled points: {int(host[:, 0].sum())} of {N} ({100.0 * host[:, 0].sum() / N:.2f} %); bins hit {int((host[:, 0] > 0).sum())} of '
                     f'{len(host)}, at most {int(host[:, 0].max())} points in one')
    ms = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k, (fn, _) in kinds.items():
            ms[k].append(timed(fn, args.calls))
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    out_lines.append(f'{"kind":44s} {"ms":>9s} {"min":>9s} {"max":>9s} {"GB/s":>8s}   (algorithmic bytes)')
    for k, v in ms.items():
        out_lines.append(f'{k:44s} {mean[k]:9.3f} {min(v):9.3f} {max(v):9.3f} {kinds[k][1] / mean[k] / 1e6:8.0f}')
    out_lines.append('ratios of the mean times:')
    for name in clouds:
        lp = mean[f'label_points, {name}']
        out_lines.append(f'  {name}: line_profile_points / label_points {mean[f"line_profile_points, {name}"] / lp:.2f} (adding: '
                         f'{mean[f"line_profile_points +=, {name}"] / lp:.2f}), / copy d2d cloud '
                         f'{mean[f"line_profile_points, {name}"] / mean[f"copy d2d cloud, {name}"]:.2f}')
        for rl in (20, 34):
            pr = mean[f'line_profile_records {rl} B, {name}']
            out_lines.append(f'  {name}: line_profile_records {rl} B / label_records {pr / mean[f"label_records {rl} B, {name}"]:.2f}, / copy d2d '
                             f'{pr / mean[f"copy d2d {rl} B, {name}"]:.2f}, / line_profile_points {pr / mean[f"line_profile_points, {name}"]:.2f}')
    text = '\n'.join(out_lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
