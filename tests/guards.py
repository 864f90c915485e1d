"""Guarded device buffers for the bounds tests (tests/test_gpu_1_bounds.py).

A Slab is one flat device allocation laid out as  front guard | rows x ld | back guard  (guards in whole rows of `ld` elements), with the
logical operand the [rows, width] view at column `lo` of the middle part.  Everything outside that view - the guards, the `ld` padding and
the columns beside the slice - is either POISON (inputs: a value a stray read cannot cancel) or a CANARY bit pattern (outputs: a stray
write changes it, and a logical element that still holds it was never written).

guarded_runs() runs a case three times - guards benign (0), guards poisoned, and at batch 3 with elements 0 and 2 poisoned - and checks
the canaries of every output after each run, bit-identical logical outputs between the first two, and element 1 of the batch-3 run
bit-identical to the batch-1 run.  It then repeats the benign batch-1 run with every CU's LDS pre-filled with each non-zero word of
lds_state.WORDS (NaN / all ones, +Inf): the canaries hold and the logical outputs keep the bits of the benign run, so no output depends
on an LDS cell the launch did not write itself (tests/lds_state.py).
"""
import torch

from lds_state import WORDS, poisoned as lds_poisoned

NAN = float('nan')
INF = float('inf')
# output canaries: a quiet NaN with a payload no arithmetic produces (fp32 / fp64), and distinctive integer / byte patterns
CANARY = {torch.float32: 0x7FC0BEEF, torch.float64: 0x7FF8BEEFDEADBEEF, torch.int32: 0x7EADBEEF, torch.uint8: 0xA5}
_INT_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int32: torch.int32, torch.uint8: torch.uint8}


class Slab:
    def __init__(self, dev, rows, width, ld=None, lo=0, front=0, back=0, dtype=torch.float32):
        ld = width if ld is None else ld
        assert 0 <= lo and lo + width <= ld and rows >= 0
        self.rows, self.width, self.ld, self.lo, self.front, self.back, self.dtype = rows, width, ld, lo, front, back, dtype
        self.n = (front + rows + back) * ld
        self.flat = torch.empty(self.n, dtype=dtype, device=dev)
        self.view = self.flat.as_strided((rows, width), (ld, 1), front * ld + lo)
        inside = torch.zeros(front + rows + back, ld, dtype=torch.bool)
        inside[front:front + rows, lo:lo + width] = True
        self.inside = inside.reshape(-1)

    def ptr(self):
        return self.view.data_ptr()

    def fill_input(self, data, pad):
        """Everything = pad, then the logical view = data ([rows, width], any shape with that many elements)."""
        self.flat.fill_(pad)
        self.view.copy_(torch.as_tensor(data).reshape(self.rows, self.width).to(self.dtype))
        return self

    def fill_canary(self):
        self.flat.view(_INT_VIEW[self.dtype]).fill_(_signed(CANARY[self.dtype], self.dtype))
        return self

    def bits(self):
        return self.flat.view(_INT_VIEW[self.dtype]).cpu()

    def logical_bits(self):
        return self.bits()[self.inside].reshape(self.rows, self.width)

    def check_canary(self, name):
        """(a) every word outside the logical view still holds the canary; (b) no logical element does (u8 outputs: (a) only)."""
        c = _signed(CANARY[self.dtype], self.dtype)
        b = self.bits()
        bad = (~self.inside) & (b != c)
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            r, col = divmod(i, self.ld)
            where = 'front guard' if r < self.front else 'back guard' if r >= self.front + self.rows else 'ld padding'
            raise AssertionError(f'{name}: {int(bad.sum())} words outside the output changed; first in the {where}, row '
                                 f'{r - self.front} (relative to the first logical row), column {col} (logical columns {self.lo}..'
                                 f'{self.lo + self.width - 1})')
        if self.dtype == torch.uint8:
            return      # (b) needs a pattern no result can hold: every byte value is a legal u8 pixel
        left = (b[self.inside] == c).reshape(self.rows, self.width)
        if bool(left.any()):
            r, col = [int(v) for v in left.nonzero()[0]]
            raise AssertionError(f'{name}: {int(left.sum())} logical output elements were never written (first: row {r}, column {col})')


def _signed(v, dtype):
    bits = {torch.float32: 32, torch.int32: 32, torch.float64: 64, torch.uint8: 8}[dtype]
    if dtype == torch.uint8:
        return v
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


def batched(data, B, poison):
    """Rows of one batch element -> rows of the whole batch: B = 1 -> data; B = 3 -> (poison, data, poison) stacked on dim 0."""
    data = torch.as_tensor(data)
    if B == 1:
        return data
    p = torch.full_like(data, poison)
    return torch.cat([p, data, p])


def guarded_runs(run, name, batch=True):
    """run(B, poisoned) -> {output name: (Slab, logical rows per batch element)}.  Returns {output name: logical contents of the benign
    batch-1 run as a CPU tensor} after the checks described in the module doc."""
    got = {}
    for B, poisoned in [(1, False), (1, True)] + ([(3, True)] if batch else []):
        outs = run(B, poisoned)
        torch.cuda.synchronize()
        for k, (s, _) in outs.items():
            s.check_canary(f'{name} [{k}, B={B}, {"poisoned" if poisoned else "benign"} guards]')
        got[(B, poisoned)] = {k: (s.logical_bits(), rpe, s.view.cpu()) for k, (s, rpe) in outs.items()}
    for k, (bits, rpe, _) in got[(1, False)].items():
        pb = got[(1, True)][k][0]
        assert torch.equal(bits, pb), f'{name} [{k}]: poisoned guards changed {int((bits != pb).sum())} logical output words (a stray read)'
        if batch:
            mid = got[(3, True)][k][0][rpe:2 * rpe]
            assert torch.equal(bits, mid), (f'{name} [{k}]: batch element 1 of 3 (neighbours poisoned) differs from the batch-1 call in '
                                            f'{int((bits != mid).sum())} words')
    for word in WORDS[1:]:
        with lds_poisoned(word) as lds:
            outs = run(1, False)
            torch.cuda.synchronize()
        assert lds.fills > 0, f'{name}: the run after LDS = 0x{word:08X} enqueued no fill'
        for k, (s, _) in outs.items():
            s.check_canary(f'{name} [{k}, B=1, benign guards, LDS pre-filled with 0x{word:08X}]')
            lb, bits = s.logical_bits(), got[(1, False)][k][0]
            diff = (lb != bits).reshape(-1)
            assert not bool(diff.any()), (f'{name} [{k}]: LDS pre-filled with 0x{word:08X} changed {int(diff.sum())} logical output words, first '
                                          f'at flat index {int(diff.nonzero()[0])}: an LDS cell this launch never wrote reaches the output')
    return {k: v[2] for k, v in got[(1, False)].items()}
