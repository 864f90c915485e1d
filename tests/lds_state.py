"""LDS-state harness of the GPU tests: no kernel's result may depend on what LDS held before it was launched.

LDS is not cleared between the dispatches of a process: a kernel that reads a cell it never wrote sees what the previous kernel left
there.  fill(word) stores one 32-bit word into all 160 KB of every CU's LDS (liblanemap_diag.so, built from tests/hip/lds_state.hip
beside the product library and never part of it); probe(word) counts the words that differ from it.  Inside poisoned(word) every call of
a stream-taking `lm_*` entry - made through gpu_common._lib(), lanemapping_amd.ops, torch_ops or any other holder of the library object
of lanemapping_amd._lib.lib() - is preceded by such a fill on the same stream, as the last thing enqueued before the entry.  The context
counts its fills and fails where there was none, so a call that goes round it cannot pass for a poisoned run.

WORDS are the three contents every case runs under: zeros; 0xFFFFFFFF, a NaN as a float and UINT_MAX / -1 / the UNSET, NO_TILE and
NO_BIN sentinels as an integer; 0x7F800000, +Inf as a float and a huge count as an integer.  A padding cell that is multiplied by a zero
weight, or masked after an add, gives the same bits after zeros and after finite floats, and NaN after the other two.

Known limit: the fill precedes the ENTRY, so only the first kernel of an entry that launches several sees the poison; its later kernels
see the LDS its earlier ones left.  An ops function that makes several `lm_*` calls gets a fill before each.
"""
import contextlib
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = (0x00000000, 0xFFFFFFFF, 0x7F800000)
LDS_WORDS = 163840 // 4

_DIAG = None


def stream_entries():
    """Every `lm_*` declaration of include/lanemap_hip.h whose first parameter is the stream: the bounds inventory's `void* stream`
    entries, and the three that call it `hip_stream`."""
    text = open(os.path.join(ROOT, 'include', 'lanemap_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    return frozenset(re.findall(r'\b(lm_\w+)\s*\(\s*void\s*\*\s*(?:hip_)?stream\b', text))


def diag():
    global _DIAG
    if _DIAG is None:
        from lanemapping_amd import _lib
        _lib.lib()                              # first: one HIP runtime per process, the one torch loads
        path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'liblanemap_diag.so')
        assert os.path.exists(path), f'{path} is missing: build it with `python -m lanemapping_amd.build`'
        L = C.CDLL(path)
        for name, args in (('lmd_lds_fill', [C.c_void_p, C.c_uint, C.c_int]),
                           ('lmd_lds_probe', [C.c_void_p, C.c_uint, C.c_void_p, C.c_int]),
                           ('lmd_lds_leaky', [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = C.c_int, args
        L.lm_last_error.restype = C.c_char_p
        _DIAG = L
    return _DIAG


def _chk(code):
    if code != 0:
        raise RuntimeError(f'liblanemap_diag error {code}: {diag().lm_last_error().decode()}')


def _stream():
    from lanemapping_amd import ops
    return ops._stream()


def workgroups():
    """The grid of fill and probe: 4 workgroups per CU, each with a CU's whole LDS."""
    import torch
    return 4 * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def fill(word):
    _chk(diag().lmd_lds_fill(_stream(), word, 0))


def probe(word):
    import torch
    n = torch.zeros(1, dtype=torch.int64, device='cuda')
    _chk(diag().lmd_lds_probe(_stream(), word, n.data_ptr(), 0))
    torch.cuda.synchronize()
    return int(n.item())


def leaky(x):
    """The negative control: y = x + 0 * (an LDS cell the kernel never wrote).  Inside poisoned() it gets the fill an `lm_*` entry gets."""
    import torch
    if _ACTIVE is not None:
        fill(_ACTIVE.word)
        _ACTIVE.fills += 1
    y = torch.empty_like(x)
    _chk(diag().lmd_lds_leaky(_stream(), x.data_ptr(), y.data_ptr(), x.numel()))
    return y


class _Poisoning:
    """The state of one poisoned() context: the word, the fill, and how many fills it has enqueued."""

    def __init__(self, fill_fn, word):
        self.fill_fn, self.word, self.fills = fill_fn, word, 0

    def wrap(self, fn, name):
        def entry(stream, *args):
            cur = _ACTIVE                       # a wrapper that outlives its context is a plain call
            if cur is not None:
                _chk(cur.fill_fn(stream, cur.word, 0))
                cur.fills += 1
            return fn(stream, *args)
        entry.__name__ = name
        return entry


_ACTIVE = None


@contextlib.contextmanager
def interposed(wrap):
    """The one way the test harnesses get in front of the library: every stream-taking `lm_*` attribute of the library object that
    lanemapping_amd._lib.lib() returns is replaced by wrap(fn, name) - on the object itself, so a handle taken before the context is
    interposed like one taken inside it; only an ENTRY bound outside escapes - and put back on exit.  Users: poisoned() below (a fill
    before each entry) and stream_state.watching() (which stream each entry was given)."""
    from lanemapping_amd import _lib
    real = _lib.lib()
    saved = {name: (name in vars(real), getattr(real, name)) for name in stream_entries()}
    for name, (_, fn) in saved.items():
        setattr(real, name, wrap(fn, name))
    try:
        yield real
    finally:
        for name, (had, fn) in saved.items():
            if had:
                setattr(real, name, fn)
            else:
                delattr(real, name)


@contextlib.contextmanager
def poisoned(word):
    """Inside the context every stream-taking `lm_*` attribute of the library object that lanemapping_amd._lib.lib() returns enqueues the
    fill first.  The attributes are replaced on the object itself, so a library handle taken before the context (`L = lib()` at the top
    of a test) is poisoned like one taken inside it; only an ENTRY bound outside (`f = lib().lm_x`) escapes.  That, or a body that calls
    no stream-taking entry at all, is an AssertionError on exit: a poisoned run that enqueued no fill proves nothing.  Yields the state
    (`.fills`).  Nested contexts give one fill per call, with the inner word."""
    global _ACTIVE
    outer = _ACTIVE
    state = _Poisoning(diag().lmd_lds_fill, word)
    with contextlib.ExitStack() as stack:
        if outer is None:
            stack.enter_context(interposed(state.wrap))
        _ACTIVE = state
        try:
            yield state
            assert state.fills > 0, ('no stream-taking lm_* entry was called through the library object inside poisoned(): nothing ran after '
                                     'poisoned LDS (an entry bound outside the context bypasses it)')
        finally:
            _ACTIVE = outer
            if outer is not None:
                outer.fills += state.fills


def _bits(v):
    """One output as a flat numpy array of unsigned words of its element size."""
    if hasattr(v, 'logical_bits'):              # guards.Slab
        v = v.logical_bits()
    a = v.detach().cpu().contiguous().numpy() if hasattr(v, 'detach') else np.ascontiguousarray(v)
    return a.reshape(-1).view(f'u{a.dtype.itemsize}')


def _named(outs):
    if isinstance(outs, dict):
        return outs
    if isinstance(outs, (list, tuple)):
        return {f'out{i}': v for i, v in enumerate(outs)}
    return {'out': outs}


def assert_same_bits(got, want, what):
    got, want = _named(got), _named(want)
    assert got.keys() == want.keys(), (what, sorted(got), sorted(want))
    for k in want:
        a, b = _bits(got[k]), _bits(want[k])
        assert a.shape == b.shape, f'{what} [{k}]: {a.shape} against {b.shape} words'
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (f'{what} [{k}]: {bad.size} of {a.size} output words differ from the run after zeroed LDS, first at flat index '
                               f'{int(bad[0])} (0x{int(a[bad[0]]):x} against 0x{int(b[bad[0]]):x}): an LDS cell this launch never wrote '
                               f'reaches the output')


def lds_state_runs(run, name):
    """run() -> the output tensors or Slabs (one, a sequence or a dict) of one call on fixed inputs.  Runs it with LDS pre-filled with each
    of WORDS and requires every output bit-identical to the run after zeros.  Returns the outputs of the 0xFFFFFFFF run, for the
    comparison with the case's reference."""
    import torch
    res = {}
    for word in WORDS:
        with poisoned(word):                    # (fails on exit if run() enqueued no fill)
            outs = _named(run())
            torch.cuda.synchronize()
        res[word] = {k: (v.logical_bits(), v.view.cpu()) if hasattr(v, 'logical_bits') else (v.detach().cpu().clone(),) * 2
                     for k, v in outs.items()}
    failed = []
    for word in WORDS[1:]:                      # every word is compared, so that the message names each one that changes the result
        try:
            assert_same_bits({k: v[0] for k, v in res[word].items()}, {k: v[0] for k, v in res[WORDS[0]].items()},
                             f'{name} after LDS = 0x{word:08X}')
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, '\n'.join(failed)
    out = {k: v[1] for k, v in res[0xFFFFFFFF].items()}
    return out if len(out) > 1 or 'out' not in out else out['out']
