#!/usr/bin/env python3
"""Micro-bench of the paint / asphalt histograms (csrc/profile.hip: lm_line_hist_points, lm_las_line_hist_records) on the bench's shape,
beside the cross-sections they share their reads and their search with: 16 tiles x 4,194,304 synthetic points (tools/bench_label.py's
cloud, lines and records), ONE index built for half_width = 0.625 m (the default of las_io.PaintThreshold and of las_io.CrossSection),
rings of 1/16 m, bins of 64 intensities.

Times, in one process, with HIP events, after a warm-up, over at least 20 repetitions each and alternating in every round:
  lm_line_hist_points           16 N read, the table written (accumulate = 0)
  lm_line_cross_points          the yardstick: the same 16 N read and the same search on the same index, the cells written
  lm_las_line_hist_records      N record_len read
  lm_las_line_cross_records     the same records, the same index
  device-to-device copy         of the cloud (2 x 16 N) and of the records (2 N record_len)
on the cloud as drawn (every wave's 64 points spread over a whole tile) and on the same points in 0.5 m cell order (the points of a wave
are neighbours on the ground, as in a file in acquisition order).

Also printed, per cloud: the share of lanes with a hit, and per wave (64 consecutive points, what one wave of either kernel holds) with
at least one hit the mean number of hit lanes and of DISTINCT table cells among them - what the choice between one atomic add per hit
lane and one per distinct cell rests on.  These statistics are computed here in float64 from the vertex interval a point projects into,
not with the kernel's bits: they describe the load, they are no reference.

The tool times the accumulation the library holds.  The other form was timed with it on a library that held both behind a run-time
switch, which was taken out afterwards; profiles/paint_threshold.txt keeps both tables.
`--out PATH` also writes the table to a file."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_label import N_TILE, TILES, records_of, strip_cloud, strip_lines, timed  # noqa: E402
from bench_profile import cell_order  # noqa: E402
from lanemapping_amd import las_io, ops  # noqa: E402
from lanemapping_amd._lib import lib  # noqa: E402


def wave_load(cloud, lines, index, thr):
    """-> (share of points with a hit, mean hit lanes, mean distinct cells) over the waves of 64 consecutive points with a hit."""
    N = cloud.shape[0]
    label = ops.label_points(cloud, index, thr.z_tol).long()
    hit = torch.nonzero(label > 0)[:, 0]
    if not len(hit):
        return 0.0, 0.0, 0.0
    verts = torch.from_numpy(np.stack(lines)).to(cloud.device)                     # [L, V, 3] float64: every line has the same x grid
    step = float(verts[0, 1, 0] - verts[0, 0, 0])
    p = cloud[hit, :2].double()
    k = label[hit] - 1
    j = torch.clamp(torch.floor(p[:, 0] / step).long(), 0, verts.shape[1] - 2)
    a, d = verts[k, j, :2], verts[k, j + 1, :2] - verts[k, j, :2]
    r = p - a
    q = torch.round((d[:, 0] * r[:, 1] - d[:, 1] * r[:, 0]) / torch.linalg.norm(d, dim=1) * 1024.0).long()
    ring = torch.clamp(q.abs(), max=thr.hq) // thr.ring_q
    iq = torch.clamp(torch.round(torch.nan_to_num(cloud[hit, 3], nan=0.0)), 0, 65535).long()
    cell = (k * thr.rings + ring) * thr.n_counts + (iq >> thr.bin_shift)
    wave = hit // 64
    waves = torch.unique(wave).numel()
    pairs = torch.unique(wave * (1 << 32) + cell).numel()
    return len(hit) / N, len(hit) / waves, pairs / waves


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
    thr = las_io.PaintThreshold()
    cross = las_io.CrossSection(paint_intensity=10000.0)
    assert thr.half_width == cross.half_width and thr.z_tol == cross.z_tol, 'one index, one height band'
    lines = strip_lines(args.tiles)
    seg = las_io.line_segments(lines)
    st, bs = las_io.line_stations(lines, None, cross.bin)
    index = ops.line_index(seg, thr.half_width, device=dev)
    stations = ops.line_stations(st, bs, cross.bin, device=dev)
    clouds = {'as drawn': strip_cloud(dev, args.tiles, args.points)}
    clouds['cell order'] = cell_order(clouds['as drawn'], args.points)
    N = clouds['as drawn'].shape[0]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    d3 = C.c_double * 3
    scale, offset = d3(1e-3, 1e-3, 1e-3), d3(0.0, 0.0, 0.0)
    nl, lq, piq = cross.nl, cross.lateral_q, cross.paint_iq
    n_cells = stations.n_bins * nl
    n_lines, Z, NB, rq, sh = stations.n_lines, thr.rings, thr.n_counts, thr.ring_q, thr.bin_shift
    n_hist = n_lines * Z * NB
    out_lines = [f'bench_threshold: {args.tiles} tiles x {args.points} points = {N} points, {n_lines} lines, {len(seg)} segments, half_width '
                 f'{thr.half_width} m, z_tol {thr.z_tol} m, grid {index.grid.nx} x {index.grid.ny} cells; the histograms: {Z} rings of {rq}/1024 m x '
                 f'{NB} bins of {1 << sh} = {n_hist} counts ({n_hist * 8 / 2 ** 20:.2f} MiB); the cross-sections: {stations.n_bins} station bins x '
                 f'{nl} cells = {n_cells} rows ({n_cells * 32 / 2 ** 20:.1f} MiB); {args.rounds} rounds x {args.calls} calls, HIP events, warm']
    hist = torch.empty((n_lines, Z, NB), dtype=torch.int64, device=dev)
    cells = torch.empty((stations.n_bins, nl, 4), dtype=torch.int64, device=dev)
    kinds = {}

    def hist_points(cloud):
        def fn():
            rc = L.lm_line_hist_points(C.c_void_p(cloud.data_ptr()), N, *index.args(), stations.args()[0], n_lines, thr.z_tol, rq, sh, 0,
                                       C.c_void_p(hist.data_ptr()), n_hist, stream)
            assert rc == 0, L.lm_last_error()
        return fn

    def cross_points(cloud):
        def fn():
            rc = L.lm_line_cross_points(stream, C.c_void_p(cloud.data_ptr()), N, *index.args(), *stations.args(), cross.z_tol, lq, piq, 0,
                                        C.c_void_p(cells.data_ptr()), n_cells)
            assert rc == 0, L.lm_last_error()
        return fn

    for name, cloud in clouds.items():
        spare = torch.empty_like(cloud)
        kinds[f'line_hist_points, {name}'] = (hist_points(cloud), 16 * N)
        kinds[f'line_cross_points, {name}'] = (cross_points(cloud), 16 * N)
        kinds[f'copy d2d cloud, {name}'] = ((lambda cloud=cloud, spare=spare: spare.copy_(cloud)), 32 * N)
        for fmt, rl in ((0, 20), (3, 34)):
            rec = records_of(cloud, rl)
            rec_out = torch.empty_like(rec)

            def hist_records(rec=rec, rl=rl, fmt=fmt):
                rc = L.lm_las_line_hist_records(C.c_void_p(rec.data_ptr()), rl, fmt, N, scale, offset, None, None, *index.args(),
                                                stations.args()[0], n_lines, thr.z_tol, rq, sh, 0, C.c_void_p(hist.data_ptr()), n_hist, stream)
                assert rc == 0, L.lm_last_error()

            def cross_records(rec=rec, rl=rl, fmt=fmt):
                rc = L.lm_las_line_cross_records(stream, C.c_void_p(rec.data_ptr()), rl, fmt, N, scale, offset, None, None, *index.args(),
                                                 *stations.args(), cross.z_tol, lq, piq, 0, C.c_void_p(cells.data_ptr()), n_cells)
                assert rc == 0, L.lm_last_error()

            kinds[f'line_hist_records {rl} B, {name}'] = (hist_records, N * rl)
            kinds[f'line_cross_records {rl} B, {name}'] = (cross_records, N * rl)
            kinds[f'copy d2d {rl} B, {name}'] = ((lambda rec=rec, rec_out=rec_out: rec_out.copy_(rec)), 2 * N * rl)
    for fn, _ in kinds.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    hist_points(clouds['as drawn'])()
    host = hist.cpu().numpy()
    found = las_io.paint_threshold(host, thr)['strip']
    out_lines.append(f'returns in the table: {int(host.sum())} of {N} ({100.0 * host.sum() / N:.2f} %); counts hit {int((host > 0).sum())} of '
                     f'{host.size}, at most {int(host.max())} returns in one; the strip: threshold {found["threshold"]}, separation '
                     f'{found["separation"]:.3f}, {found["inner_returns"]} inner and {found["outer_returns"]} outer returns')
    for name, cloud in clouds.items():
        share, lanes, distinct = wave_load(cloud, lines, index, thr)
        out_lines.append(f'  {name}: {100.0 * share:.2f} % of the lanes hit; per wave with a hit {lanes:.1f} hit lanes in {distinct:.1f} distinct counts')
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
        hp, cp = mean[f'line_hist_points, {name}'], mean[f'line_cross_points, {name}']
        out_lines.append(f'  {name}: line_hist_points / line_cross_points {hp / cp:.2f}, / copy d2d cloud {hp / mean[f"copy d2d cloud, {name}"]:.2f}')
        for rl in (20, 34):
            hr, cr = mean[f'line_hist_records {rl} B, {name}'], mean[f'line_cross_records {rl} B, {name}']
            out_lines.append(f'  {name}: line_hist_records {rl} B / line_cross_records {hr / cr:.2f}, / copy d2d {hr / mean[f"copy d2d {rl} B, {name}"]:.2f}, '
                             f'/ line_hist_points {hr / hp:.2f}')
    text = '\n'.join(out_lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
