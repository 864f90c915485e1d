#!/usr/bin/env python3
"""Micro-bench of the marking colours (csrc/profile.hip: lm_las_line_colour_records) beside the marking profile it shares its kernel with:
16 tiles x 4,194,304 synthetic points (tools/bench_label.py's cloud and lines) as 36-byte records of point format 7, every return with an
R, G, B triple (one in sixteen black), profiled at bin = 0.25 m.

Times, in one process, with HIP events, after a warm-up, over at least 20 repetitions each and alternating in every round:
  lm_las_line_colour_records    N record_len read once; bins and colours written
  lm_las_line_profile_records   N record_len read; bins written - the unchanged entry, on the same buffer
  device-to-device copy         of the same buffer (2 N record_len)
on the cloud as drawn (every wave's 64 points spread over a whole tile) and on the same points in 0.5 m cell order (the points of a wave
are neighbours on the ground, as in a file in acquisition order).  The alternative to the single pass is a colour pass of its own after
the profile, two reads of every record: the colour entry has to stay below twice the profile entry's time.  `--out PATH` also writes the
table to a file (profiles/marking_colour.txt holds one)."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_label import N_TILE, TILES, strip_cloud, strip_lines, timed  # noqa: E402
from bench_profile import cell_order  # noqa: E402
from lanemapping_amd import las_io, ops  # noqa: E402
from lanemapping_amd._lib import lib  # noqa: E402

FMT, RL = 7, 36


def colour_records(cloud):
    """[N,4] f32 -> N format-7 records of 36 bytes on the device (padded to 4 bytes): X Y Z int32 at 1 mm, intensity u16, return 1 of 1,
    class 2, and at byte 30 a triple that depends on the point's index: one in sixteen black, the others spread on both sides of the
    yellow vote."""
    n = cloud.shape[0]
    rec = torch.zeros((n, RL), dtype=torch.uint8, device=cloud.device)
    q = torch.round(cloud[:, :3].double() / 1e-3).to(torch.int32).contiguous()
    rec[:, 0:12] = q.view(torch.uint8).reshape(n, 12)
    rec[:, 12:14] = cloud[:, 3].clamp(0, 65535).to(torch.int32).to(torch.int16).contiguous().view(torch.uint8).reshape(n, 2)
    rec[:, 14], rec[:, 16] = 0x11, 2
    i = torch.arange(n, device=cloud.device, dtype=torch.int64)
    rgb = torch.stack([40000 + i % 20011, 35000 + (i * 7) % 25013, (i * 13) % 60013], dim=1)
    rgb[i % 16 == 5] = 0
    o = las_io.rgb_offset(FMT)
    for c in range(3):
        rec[:, o + 2 * c], rec[:, o + 2 * c + 1] = (rgb[:, c] & 255).to(torch.uint8), (rgb[:, c] >> 8).to(torch.uint8)
    flat = torch.zeros(((n * RL + 3) // 4 * 4,), dtype=torch.uint8, device=cloud.device)
    flat[:n * RL] = rec.reshape(-1)
    return flat


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
    survey, colour = las_io.MarkingSurvey(), las_io.MarkingColour()
    lines = strip_lines(args.tiles)
    seg = las_io.line_segments(lines)
    st, bs = las_io.line_stations(lines, None, survey.bin)
    index = ops.line_index(seg, survey.half_width, device=dev)
    stations = ops.line_stations(st, bs, survey.bin, device=dev)
    cloud = strip_cloud(dev, args.tiles, args.points)
    N = cloud.shape[0]
    recs = {'as drawn': colour_records(cloud)}
    recs['cell order'] = colour_records(cell_order(cloud, args.points))
    del cloud
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    d3 = C.c_double * 3
    scale, offset = d3(1e-3, 1e-3, 1e-3), d3(0.0, 0.0, 0.0)
    nan = float('nan')
    out_lines = [f'bench_colour: {args.tiles} tiles x {args.points} points = {N} records of {RL} B (point format {FMT}), {len(lines)} lines, '
                 f'{len(seg)} segments, {stations.n_bins} bins of {survey.bin} m, half_width {survey.half_width} m, blue_q {colour.blue_q}; '
                 f'{args.rounds} rounds x {args.calls} calls, HIP events, warm']
    bins, colours, plain = stations.new_bins(), stations.new_bins(), stations.new_bins()
    spare = torch.empty_like(recs['as drawn'])
    kinds = {}
    for name, rec in recs.items():
        def colour_call(rec=rec):
            rc = L.lm_las_line_colour_records(stream, C.c_void_p(rec.data_ptr()), RL, FMT, N, scale, offset, None, None, *index.args(),
                                              *stations.args(), survey.z_tol, nan, colour.blue_q, 0, C.c_void_p(bins.data_ptr()),
                                              C.c_void_p(colours.data_ptr()), stations.n_bins)
            assert rc == 0, L.lm_last_error()

        def profile_call(rec=rec):
            rc = L.lm_las_line_profile_records(stream, C.c_void_p(rec.data_ptr()), RL, FMT, N, scale, offset, None, None, *index.args(),
                                               *stations.args(), survey.z_tol, nan, 0, C.c_void_p(plain.data_ptr()), stations.n_bins)
            assert rc == 0, L.lm_last_error()

        kinds[f'line_colour_records {RL} B, {name}'] = (colour_call, N * RL)
        kinds[f'line_profile_records {RL} B, {name}'] = (profile_call, N * RL)
        kinds[f'copy d2d {RL} B, {name}'] = ((lambda rec=rec: spare.copy_(rec)), 2 * N * RL)
    for fn, _ in kinds.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(bins, plain), 'bins differ between the two entries'
    host = torch.stack([bins, colours]).cpu().numpy()
    b, c = host[0], host[1]
    assert ((c[:, 0] + c[:, 5]) == b[:, 0]).all(), 'a profiled return is neither coloured nor black'
    out_lines.append(f'profiled records: {int(b[:, 0].sum())} of {N} ({100.0 * b[:, 0].sum() / N:.2f} %); coloured {int(c[:, 0].sum())}, yellow votes '
                     f'{int(c[:, 4].sum())}, black {int(c[:, 5].sum())}; bins equal lm_las_line_profile_records\' bit for bit')
    ms = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k, (fn, _) in kinds.items():
            ms[k].append(timed(fn, args.calls))
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    out_lines.append(f'{"kind":44s} {"ms":>9s} {"min":>9s} {"max":>9s} {"GB/s":>8s}   (algorithmic bytes)')
    for k, v in ms.items():
        out_lines.append(f'{k:44s} {mean[k]:9.3f} {min(v):9.3f} {max(v):9.3f} {kinds[k][1] / mean[k] / 1e6:8.0f}')
    out_lines.append('ratios of the mean times (the colour entry has to stay below 2.00 x the profile entry, the price of a second pass):')
    for name in recs:
        col, pro = mean[f'line_colour_records {RL} B, {name}'], mean[f'line_profile_records {RL} B, {name}']
        out_lines.append(f'  {name}: line_colour_records / line_profile_records {col / pro:.2f}, / copy d2d {col / mean[f"copy d2d {RL} B, {name}"]:.2f}; '
                         f'line_profile_records / copy d2d {pro / mean[f"copy d2d {RL} B, {name}"]:.2f}')
    text = '\n'.join(out_lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
