#!/usr/bin/env python3
"""Micro-bench of the paint residue (csrc/residue.hip) on the bench's shape: 16 clouds of 4,194,304 synthetic points (synth.las_points, laid
along x as tools/bench_label.py lays them), eight lines along the strip with a vertex every 0.6 m.  The clouds' six painted stripes per tile
lie beside those lines, so they are residue: about a quarter of all points.

Times, in one process, with HIP events, after a warm-up, over at least 20 repetitions each and alternating in every round:
  lm_residue_keys            16 N read, 12 N written (key + iq)
  ops.label_points +dist2    the yardstick: the same points, index and min_intensity, 16 N read, 8 N written
  device-to-device copy      of the same points, 32 N
  the torch plumbing         compaction of the keys >= 0, concatenation, unique cells with counts, the per-cell index_add_ of iq, the dense
                             component ids from the roots
  lm_cell_components         per cell
  lm_residue_stats           per cell
  ops.paint_residue          the whole pipeline over the 16 clouds, its one read-back included
and prints the times and the ratios; `--out PATH` also writes them to a file (profiles/residue.txt holds one)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_label import EXTENT, N_TILE, TILES, strip_lines, timed  # noqa: E402
from lanemapping_amd import las_io, ops, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=TILES)
    ap.add_argument('--points', type=int, default=N_TILE)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=4, help='calls per round and kind: rounds x calls >= 20 repetitions')
    ap.add_argument('--min-intensity', type=float, default=12000.0)
    ap.add_argument('--index-cell', type=float, default=None, help='cell of the line index in metres (default: las_io.residue_index_cell)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.rounds * args.calls >= 20, 'at least 20 repetitions'
    dev = torch.device('cuda:0')
    res = las_io.PaintResidue(min_intensity=args.min_intensity)
    base = [torch.from_numpy(synth.las_points(2021 + i, args.points)).to(dev) for i in range(min(4, args.tiles))]
    clouds = []
    for t in range(args.tiles):
        c = base[t % len(base)].clone()
        c[:, 0] += EXTENT * t
        clouds.append(c)
    del base
    N = sum(int(c.shape[0]) for c in clouds)
    lines = strip_lines(args.tiles)
    seg = las_io.line_segments(lines)
    index = ops.line_index(seg, res.reach, cell=args.index_cell or las_io.residue_index_cell(res), device=dev)
    grid = ops.residue_grid(index, res.cell)
    nx, ny = grid['nx'], grid['ny']
    out_lines = [f'bench_residue: {args.tiles} clouds x {args.points} points = {N} points, {len(lines)} lines, {len(seg)} segments, index grid '
                 f'{index.grid.nx} x {index.grid.ny} cells of {index.grid.cell:g} m, {index.grid.n_entries} list entries; reach {res.reach} m, clear {res.clear} m, min_intensity '
                 f'{res.min_intensity:g}, residue grid {nx} x {ny} cells of {res.cell} m; {args.rounds} rounds x {args.calls} calls, HIP events, warm']
    args_keys = (index, res.z_tol, res.min_intensity, res.clear, grid)
    copy_out = torch.empty_like(clouds[0])

    def keys_all():
        return [ops.residue_keys(c, *args_keys) for c in clouds]

    def label_all():
        for c in clouds:
            ops.label_points(c, index, res.z_tol, res.min_intensity, want_dist2=True)

    def copy_all():
        for c in clouds:
            copy_out.copy_(c)

    pairs = keys_all()

    def plumbing_front():
        ks, qs = [], []
        for key, iq in pairs:
            on = key >= 0
            ks.append(key[on])
            qs.append(iq[on].to(torch.int64))
        keys, iqs = torch.cat(ks), torch.cat(qs)
        cells, inverse, counts = torch.unique(keys, sorted=True, return_inverse=True, return_counts=True)
        cell_iq = torch.zeros((cells.shape[0],), device=dev, dtype=torch.int64).index_add_(0, inverse, iqs)
        return cells, counts, cell_iq, int(keys.shape[0])

    cells, counts, cell_iq, n_res = plumbing_front()
    M = int(cells.shape[0])
    root, err = ops.cell_components(cells, nx, ny, res.connectivity)

    def plumbing_back():
        roots, comp = torch.unique(root, sorted=True, return_inverse=True)
        return comp.to(torch.int32), int(roots.shape[0])

    comp, K = plumbing_back()
    kinds = {'residue_keys': (keys_all, 'point', N), 'label_points +dist2': (label_all, 'point', N), 'copy d2d': (copy_all, 'point', N),
             'torch plumbing, keys -> cells': (plumbing_front, 'point', N), 'cell_components': (lambda: ops.cell_components(cells, nx, ny, res.connectivity), 'cell', M),
             'torch plumbing, roots -> ids': (plumbing_back, 'cell', M),
             'residue_stats': (lambda: ops.residue_stats(comp, cells, nx, ny, counts, cell_iq, K), 'cell', M),
             'paint_residue, all of it': (lambda: ops.paint_residue(clouds, index, res.z_tol, res.min_intensity, res.clear, res.cell, res.connectivity), 'point', N)}
    for fn, _, _ in kinds.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    assert int(err) == 0
    stats = ops.residue_stats(comp, cells, nx, ny, counts, cell_iq, K)
    big = int((stats[:, 0] >= res.min_cells).sum())
    out_lines.append(f'residue points: {n_res} of {N} ({100.0 * n_res / N:.2f} %); occupied cells M = {M}; components K = {K}, '
                     f'{big} of them with at least {res.min_cells} cells; largest {int(stats[:, 0].max()) if K else 0} cells')
    ms = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k, (fn, _, _) in kinds.items():
            ms[k].append(timed(fn, args.calls))
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    out_lines.append(f'{"kind":32s} {"ms":>9s} {"min":>9s} {"max":>9s} {"ns per":>9s}')
    for k, v in ms.items():
        _, unit, n = kinds[k]
        out_lines.append(f'{k:32s} {mean[k]:9.3f} {min(v):9.3f} {max(v):9.3f} {1e6 * mean[k] / max(n, 1):9.3f} {unit}')
    out_lines.append(f'algorithmic GB/s: residue_keys {28 * N / mean["residue_keys"] / 1e6:.0f} (28 B a point), label_points +dist2 '
                     f'{24 * N / mean["label_points +dist2"] / 1e6:.0f} (24 B), copy d2d {32 * N / mean["copy d2d"] / 1e6:.0f} (32 B)')
    out_lines.append(f'ratios of the mean times: residue_keys / label_points +dist2 {mean["residue_keys"] / mean["label_points +dist2"]:.2f} '
                     f'(bytes written 12 : 8, bytes moved 28 : 24 = 1.17), / copy d2d {mean["residue_keys"] / mean["copy d2d"]:.2f}; '
                     f'label_points +dist2 / copy d2d {mean["label_points +dist2"] / mean["copy d2d"]:.2f}')
    text = '\n'.join(out_lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
