"""Stream harness of the GPU tests: an entry uses the stream it was given, and nothing else - off the default stream, and in graph replay.

A CASE is one call on fixed inputs (Case below: name, entries, setup, run, alter).  stream_runs(case, dev) runs it three ways.

1. Reference: on the default stream, synchronised, timed by wall clock (t_case).  Its outputs (`want`) stay alive to the end.
2. Side stream, busy default stream: a bounded blocker (torch.cuda._sleep, calibrated once per process with two events; length
   max(20 ms, 4 x t_case)) is enqueued on the default stream with an event `done` behind it; then run() on a non-blocking side
   stream (the next of torch's pool that runs beside the default stream) whose allocator blocks were pre-filled with 0xA5 bytes.  Required:
   (a) every stream-taking `lm_*` entry called (lds_state.interposed) was given exactly the side stream's handle, and one was called;
   (b) every output has the bits of `want` - work that an entry put on the default stream by mistake runs behind the blocker, after
       the side stream has finished, and the outputs show it;
   (c) the default stream's event is still pending when the side stream has drained: the call waited neither for the default stream
       nor for the whole device.  (c) is one-sided: an entry that waits for the device waits for the blocker whatever its length, so
       the length is no pass threshold, but a call whose honest host-enqueue plus execution time outlasts the blocker fails it.
3. Graph replay, for cases whose entries are all of class 'async' (STREAM_CLASS): run() is captured once on another side stream (one
   stream, a linear capture; the interposer requires the capturing stream's handle), then for data sets k = 1, 2, 0: alter(state, k),
   every captured output and every tensor of state['work'] (the workspaces of the cases that call a raw entry; a workspace that an ops
   wrapper allocates inside run() is out of reach and keeps what the previous replay left) filled with 0xFF bytes, replay, compared
   bit for bit with an eager run() on the same data.  Stale per-replay state (a memset node that does not replay) and values baked in from the host both show.

Known limits: a case proves its entry at the shape it runs - an enqueue that shape does not reach is not seen; (c) is one-sided (above)
and needs a side stream on another hardware queue than the default stream's, which the harness probes for (_stream_beside_default);
work put on a THIRD stream that happens to finish in time is not seen by (b), only a wrong handle at the entry is (a).

STREAM_CLASS says of every stream entry whether it may be captured: 'async' entries launch kernels (the zeroing kernel lm_zero_async
among them) and enqueue device-to-device copies only - no hipMemsetAsync: captured memset nodes were measured to replay wrongly;
'host' entries copy call-local host memory or synchronise the stream and refuse a capturing stream by name (csrc/common.h,
LM_NO_CAPTURE).  tests/test_stream_inventory_cpu.py derives the class from the sources and holds this table to it.
"""
import contextlib
import time

import lds_state
from lds_state import _named, assert_same_bits

# (both tables are literals: tests/test_stream_inventory_cpu.py reads them without importing this file)
STREAM_CLASS = {
    'lm_conv2d_nhwc_mfma_f32': 'async', 'lm_conv2d_nhwc_mfma_resup_f32': 'async', 'lm_conv3x3_winograd44_f32': 'async',
    'lm_conv3x3_winograd44_twin_f32': 'async', 'lm_wino44_split_fragments': 'async', 'lm_conv3x3_winograd44_split_f32': 'async',
    'lm_conv3x3_winograd44_split_twin_f32': 'async', 'lm_conv2d_nhwc_mfma_f32_gnstats': 'async', 'lm_gn_finalize': 'async',
    'lm_gn_finalize_split': 'async', 'lm_stem_conv7x7_bn_relu': 'async', 'lm_stem_conv7x7_bn_relu_u8': 'async',
    'lm_maxpool3x3s2_nhwc': 'async', 'lm_conv2d_nhwc_small': 'async', 'lm_gn_stats': 'async', 'lm_gn_relu_upsample': 'async',
    'lm_gn_relu_upsample_sum': 'async', 'lm_gn_relu_upsample_sum_conv1x1': 'async', 'lm_upsample_bilinear_nhwc': 'async',
    'lm_upsample_bilinear_to_chw': 'async', 'lm_layernorm_rows': 'async', 'lm_unpatchify': 'async', 'lm_token_mix_mfma_f32': 'async',
    'lm_attention_f32': 'async', 'lm_attention_masked_f32': 'async', 'lm_head_tokens': 'async', 'lm_head_tokens_window': 'async',
    'lm_head_stage2': 'async', 'lm_head_proposal_conf': 'async', 'lm_head_endpoint': 'async', 'lm_decode_proposals': 'async',
    'lm_decode_orient': 'async', 'lm_decode_semantic': 'async', 'lm_endp_topk': 'async', 'lm_pack_segments': 'async',
    'lm_bev_raster_batch': 'async', 'lm_bev_raster_batch_scaled': 'async', 'lm_tile_ingest_u8': 'async',
    'lm_strip_bin_points': 'host', 'lm_tile_ground': 'host', 'lm_ground_select': 'host', 'lm_tile_intensity_window': 'host',
    'lm_drape_vertices': 'host',
    'lm_tile_gap_hist': 'async', 'lm_tile_gap_fill': 'async', 'lm_softmax_rows': 'async', 'lm_rowref_select': 'async',
    'lm_rowref_gather': 'async', 'lm_rowref_scatter': 'async', 'lm_rowref_gather_win': 'async', 'lm_rowref_scatter_win': 'async',
    'lm_rowref_decode': 'async', 'lm_exclusive_scan_u32': 'async', 'lm_sort_pairs_u32': 'async', 'lm_voxelize_hard': 'async',
    'lm_sparse_grid_build': 'async', 'lm_sparse_conv_outputs': 'async', 'lm_sparse_rulebook': 'async', 'lm_conv_gather_mfma_f32': 'async',
    'lm_sparse_to_dense_nhwc': 'async', 'lm_upsample_bicubic_nhwc': 'async', 'lm_las_decode_points': 'async',
    'lm_las_decode_select': 'async', 'lm_label_points': 'async', 'lm_las_label_records': 'async', 'lm_line_profile_points': 'async',
    'lm_las_line_profile_records': 'async', 'lm_las_line_colour_records': 'async', 'lm_line_cross_points': 'async',
    'lm_las_line_cross_records': 'async', 'lm_residue_keys': 'async', 'lm_cell_components': 'async', 'lm_residue_stats': 'async',
}
STREAM_EXEMPT = {}

BLOCKER_FLOOR_MS = 20.0
BLOCKER_FACTOR = 4.0
_CYCLES_PER_MS = None
SEEN = {}                                       # entry -> names of the cases that reached it on the side stream


class Case:
    """name; entries: the `lm_*` names the call is expected to reach; setup(dev) -> state: uploads the fixed inputs and preallocates
    what must be static (state['work']: tensors the harness fills with 0xFF before a replay); run(state) -> outs: ONE call of an ops /
    las_io function or of the raw entry, allocating its outputs itself; alter(state, k): overwrites the input tensors IN PLACE with
    fixed data set k (0: the original).  klass: None (from STREAM_CLASS and `entries`) or, for the negative controls, 'async'."""

    def __init__(self, name, entries, setup, run, alter, klass=None):
        self.name, self.entries, self.setup, self.run, self.alter, self.klass = name, tuple(entries), setup, run, alter, klass

    def captured(self):
        return self.klass == 'async' if self.klass else all(STREAM_CLASS[e] == 'async' for e in self.entries)


# ---------------------------------------------------------------------------------------------------- the interposer's second user
class _Watch:
    def __init__(self):
        self.calls = []                         # (entry, raw stream handle)

    def wrap(self, fn, name):
        def entry(stream, *args):
            self.calls.append((name, _raw(stream)))
            return fn(stream, *args)
        entry.__name__ = name
        return entry


_WATCH = None


def _raw(stream):
    v = getattr(stream, 'value', stream)
    return int(v) if v is not None else 0


@contextlib.contextmanager
def watching():
    """Inside the context every call of a stream-taking `lm_*` entry through the library object is recorded with the stream it was given."""
    global _WATCH
    assert _WATCH is None, 'watching() does not nest'
    w = _Watch()
    with lds_state.interposed(w.wrap):
        _WATCH = w
        try:
            yield w
        finally:
            _WATCH = None


def fake_entry(name):
    """What a pure-torch stand-in of an entry (the negative controls) calls first: recorded like an `lm_*` call on the current stream."""
    if _WATCH is not None:
        _WATCH.calls.append((name, _raw(lds_state._stream())))


# ---------------------------------------------------------------------------------------------------- the blocker
def cycles_per_ms(dev):
    """torch.cuda._sleep cycles per millisecond on this device, measured once per process with two events and printed."""
    global _CYCLES_PER_MS
    import torch
    if _CYCLES_PER_MS is None:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize(dev)
        n, ms = 1_000_000, 0.0
        for _ in range(5):                      # grow the probe until it lasts a few milliseconds: launch overhead is then < 1 %
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(n)
            e1.record()
            torch.cuda.synchronize(dev)
            ms = e0.elapsed_time(e1)
            if ms >= 5.0:
                break
            n *= 8
        assert ms >= 1.0, f'torch.cuda._sleep({n}) lasted {ms:.3f} ms: the blocker cannot be calibrated'
        _CYCLES_PER_MS = n / ms
        print(f'stream_state: torch.cuda._sleep runs {_CYCLES_PER_MS:.0f} cycles per ms ({n} cycles in {ms:.2f} ms)')
    return _CYCLES_PER_MS


PROBE_MS = 2.0


def _stream_beside_default(dev, rate):
    """A non-blocking stream whose work demonstrably runs WHILE the default stream is busy.  A process has few hardware queues (4 by
    default) and the runtime deals streams out to them in turn: a stream that shares the default stream's queue runs behind the blocker
    whatever an entry does, and (c) would blame the entry.  torch.cuda.Stream() is no new HIP stream either: it hands out the next of
    a fixed pool of streams, round robin.  So every candidate is probed first - a 2 ms blocker on the default stream, one torch kernel
    on the candidate - and one that waited is passed over: the next call of torch.cuda.Stream() gives the pool's next stream."""
    import torch
    default, probe, waited = torch.cuda.current_stream(dev), torch.zeros(64, device=dev), 0
    torch.cuda.synchronize(dev)
    for _ in range(8):
        s = torch.cuda.Stream(dev)
        done = torch.cuda.Event()
        torch.cuda._sleep(int(PROBE_MS * rate))
        done.record(default)
        with torch.cuda.stream(s):
            probe.add_(1.0)
        s.synchronize()
        beside = not done.query()
        torch.cuda.synchronize(dev)
        if beside:
            return s
        waited += 1
    raise AssertionError(f'none of {waited} streams ran a kernel while the default stream was busy for {PROBE_MS} ms: this device '
                         f'or runtime serialises streams, and the stream tests prove nothing here')


def _ff(t):
    """Every byte of the tensor's storage = 0xFF."""
    import torch
    torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage()).fill_(0xFF)


def _poison_allocator(want, footprint, dev):
    """On the current stream: blocks of the outputs' sizes, one of the call's footprint and 2 MiB of small ones, filled with 0xA5 and
    freed - what torch.empty hands out next on this stream."""
    import torch
    junk = [torch.empty(max(v.untyped_storage().nbytes(), 1), dtype=torch.uint8, device=dev) for v in want.values() if hasattr(v, 'untyped_storage')]
    junk.append(torch.empty(max(int(footprint), 1), dtype=torch.uint8, device=dev))
    junk += [torch.empty(n, dtype=torch.uint8, device=dev) for n in (512, 4096, 65536, 1 << 20) for _ in range(4)]
    for j in junk:
        j.fill_(0xA5)
    del junk


def _same(got, want, what, against):
    try:
        assert_same_bits(got, want, what)
    except AssertionError as e:
        raise AssertionError(str(e).replace('the run after zeroed LDS', against)
                             .replace(': an LDS cell this launch never wrote reaches the output', '')) from None


def _on(calls, handle, what, name):
    assert calls, f'{name}: {what} called no stream-taking lm_* entry through the library object'
    wrong = sorted({(n, hex(s)) for n, s in calls if s != handle})
    assert not wrong, f'{name}: {what}: entries were given a stream other than the current one (0x{handle:x}): {wrong}'


def stream_runs(case, dev):
    """-> the outputs of the side-stream run (CPU copies), for the case's comparison with its reference.  See the module doc."""
    import torch
    name = case.name
    default = torch.cuda.current_stream(dev)
    assert default == torch.cuda.default_stream(dev), 'stream_runs starts on the default stream'
    rate = cycles_per_ms(dev)
    state = case.setup(dev)
    torch.cuda.synchronize(dev)
    # ---- 1. the reference
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    want = _named(case.run(state))
    torch.cuda.synchronize(dev)
    t_case = (time.perf_counter() - t0) * 1e3
    footprint = torch.cuda.max_memory_allocated(dev) - base
    want_cpu = {k: v.detach().cpu().clone() for k, v in want.items()}       # (`want` itself stays alive: its blocks cannot come back)
    # ---- 2. side stream, busy default stream
    side = _stream_beside_default(dev, rate)
    side.wait_stream(default)
    with torch.cuda.stream(side):
        _poison_allocator(want, footprint, dev)
    side.synchronize()
    block_ms = max(BLOCKER_FLOOR_MS, BLOCKER_FACTOR * t_case)
    done = torch.cuda.Event()
    torch.cuda._sleep(int(block_ms * rate))
    done.record(default)
    with watching() as w, torch.cuda.stream(side):
        got = _named(case.run(state))
        side.synchronize()
        still = not done.query()
        torch.cuda.synchronize(dev)
    print(f'stream_state {name}: t_case {t_case:.2f} ms, blocker {block_ms:.1f} ms, footprint {footprint} B, '
          f'entries {sorted({n for n, _ in w.calls})}, default stream still busy after the side stream drained: {still}')
    _on(w.calls, side.cuda_stream, 'the side-stream run', name)
    got_cpu = {k: v.detach().cpu().clone() for k, v in got.items()}
    _same(got_cpu, want_cpu, f'{name} on a side stream beside a busy default stream', 'the run on the default stream')
    assert still, (f'{name}: the default stream\'s {block_ms:.0f} ms blocker had finished when the side-stream call returned and its stream '
                   f'had drained (t_case {t_case:.2f} ms): the call waited for the default stream or for the whole device')
    for n, _ in w.calls:
        SEEN.setdefault(n, set()).add(name)
    # ---- 3. graph replay
    if case.captured():
        cap = torch.cuda.Stream(dev)
        graph = torch.cuda.CUDAGraph()
        with watching() as w:
            with torch.cuda.graph(graph, stream=cap):
                outs = _named(case.run(state))
        _on(w.calls, cap.cuda_stream, 'the captured run', name)
        for k in (1, 2, 0):
            case.alter(state, k)
            for t in list(outs.values()) + list(state.get('work', ())):
                _ff(t)
            torch.cuda.synchronize(dev)
            graph.replay()
            torch.cuda.synchronize(dev)
            replayed = {key: v.detach().cpu().clone() for key, v in outs.items()}
            eager = {key: v.detach().cpu().clone() for key, v in _named(case.run(state)).items()}
            torch.cuda.synchronize(dev)
            _same(replayed, eager, f'{name}, graph replay on data set {k} over outputs pre-filled with 0xFF', 'the eager run on the same data')
        del graph
    return got_cpu if len(got_cpu) > 1 or 'out' not in got_cpu else got_cpu['out']
