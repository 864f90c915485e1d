#!/usr/bin/env python3
"""Micro-bench of lm_las_decode_points (LAS point records resident in HBM -> [N,4] f32): HBM-bound byte work,
algorithmic bytes = N * (record_len + 16).

--select: lm_las_decode_select (decode + select + stable compaction; algorithmic bytes = 2 N record_len + 16 kept) at keep ratios 1.0,
0.5 and 0.05 on 20- and 34-byte records, next to the plain decode of the same buffers in the same process, the two alternating in
every round (device events around 50 calls; mean, fastest and slowest of 5 rounds).  `call`: the C entry alone, nothing read back;
`reader`: las_io.decode_points(select=...), which reads the kept count back after every call."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lanemapping_amd import las_io  # noqa: E402

dev = torch.device('cuda:0')
N = 1 << 24


def _timed(fn, calls=50):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def bench_select():
    from lanemapping_amd._lib import lib
    L = lib()
    d3 = (C.c_double * 3)
    scale, offset = d3(1e-3, 1e-3, 1e-3), d3(0.0, 0.0, 0.0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    need = L.lm_las_select_workspace_bytes(N)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    meta = torch.empty(257, dtype=torch.int64, device=dev)
    out = torch.empty((N, 4), dtype=torch.float32, device=dev)
    flt = las_io.PointFilter(classes=[2], drop_withheld=False)
    sel = flt.as_struct()
    for fmt, rl in ((0, 20), (3, 34)):
        for ratio in (1.0, 0.5, 0.05):
            g = torch.Generator(device=dev).manual_seed(7)
            rec = torch.randint(0, 255, (N, rl), dtype=torch.uint8, device=dev, generator=g)
            rec[:, 15] = torch.where(torch.rand(N, device=dev, generator=g) < ratio, 2, 7).to(torch.uint8)     # class 2 kept, 7 (noise) dropped
            rec = rec.reshape(-1)

            def plain():
                las_io.decode_points(rec, rl, N, [1e-3] * 3, [0.0] * 3, None, False, out=out)

            def call(hist):
                def fn():
                    rc = L.lm_las_decode_select(stream, C.c_void_p(rec.data_ptr()), rl, fmt, N, scale, offset, None, las_io.INTEN_MIN,
                                                las_io.INTEN_MAX, 0, C.byref(sel), C.c_void_p(ws.data_ptr()), need, C.c_void_p(out.data_ptr()),
                                                C.c_void_p(meta.data_ptr()), C.c_void_p(meta.data_ptr() + 8) if hist else None)
                    assert rc == 0, L.lm_last_error()
                return fn

            def reader():
                las_io.decode_points(rec, rl, N, [1e-3] * 3, [0.0] * 3, None, False, out=out, point_format=fmt, select=flt)

            kinds = {'plain': plain, 'call': call(False), 'call_hist': call(True), 'reader': reader}
            for fn in kinds.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            kept = int(meta[0])
            ms = {k: [] for k in kinds}
            for _ in range(5):
                for k, fn in kinds.items():
                    ms[k].append(_timed(fn))
            row = {'record_len': rl, 'points': N, 'keep_ratio': ratio, 'kept': kept}
            for k, v in ms.items():
                nbytes = N * (rl + 16) if k == 'plain' else 2 * N * rl + 16 * kept
                row[k] = {'ms': sum(v) / len(v), 'ms_min': min(v), 'ms_max': max(v), 'GBps': nbytes / (sum(v) / len(v)) / 1e6}
            row['call_over_plain'] = row['call']['ms'] / row['plain']['ms']
            print(json.dumps(row), flush=True)


if '--select' in sys.argv:
    bench_select()
    sys.exit(0)
for rl in (20, 28, 34):
    rec = torch.randint(0, 255, ((N * rl + 3) // 4 * 4,), dtype=torch.uint8, device=dev)
    for _ in range(3):
        las_io.decode_points(rec, rl, N, [1e-3] * 3, [0.0] * 3, None, False)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        las_io.decode_points(rec, rl, N, [1e-3] * 3, [0.0] * 3, None, False)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / 10
    print(json.dumps({'record_len': rl, 'points': N, 'ms': ms, 'GBps': N * (rl + 16) / ms / 1e6, 'frac_of_8TBps': N * (rl + 16) / ms / 1e6 / 8000}))
