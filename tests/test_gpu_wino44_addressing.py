"""GPU tests (-m gpu) of how wino44_kernel addresses its operands: the patch loads go through a buffer resource per image (one 32-bit byte
offset per load and lane, the channel unit in the scalar offset, padding cells refused by the resource's range check) and the K loop is
unrolled over the two patch buffers, with a tail for an odd unit count.

Everything is held to the BITS of the materialising twin (three plain kernels with 64-bit addressing that share the arithmetic helpers):
one, two, an odd number and an odd number above four of 16-channel units; Cout below, at and above the 64-channel N tile; dilation 1-3 at the
smallest image the kernel takes and just above; operands placed so that a padding cell, or a range check that follows the allocation
instead of the operand, meets NaN; inputs beyond 4 GiB; and the image size at which 32-bit offsets end."""
import pytest
import torch

from gpu_common import _close, _g
from guards import NAN, Slab

pytestmark = pytest.mark.gpu

COUTS = (8, 64, 72)


def _smallest(ops, cin, dil):
    """Smallest H and, at that H, smallest W that ops.wino44_supported accepts."""
    H = next(h for h in range(1, 64) if any(ops.wino44_supported(h, w, cin, dil) for w in range(1, 400)))
    W = next(w for w in range(1, 400) if ops.wino44_supported(H, w, cin, dil))
    return H, W


_packed = {}


def _weights(ops, dev, cin, cout):
    """(U, fragments) of a seeded 3x3 weight, packed once per (cin, cout) for the whole file."""
    if (cin, cout) not in _packed:
        w = (torch.randn((cout, cin, 3, 3), generator=_g(100 * cin + cout)) / (cin * 9) ** 0.5).to(dev)
        wu = ops.pack_wino44(w)
        _packed[(cin, cout)] = (w, wu, ops.pack_wino44_fragments(wu))
    return _packed[(cin, cout)]


def _act(ops, dev, B, c, H, W, seed):
    x = ops.new_act(B, c, H, W, dev)
    x.copy_(torch.randn((B, c, H, W), generator=_g(seed)).to(dev))
    return x


@pytest.mark.parametrize('dil', [1, 2, 3])
@pytest.mark.parametrize('cin', [16, 32, 48, 80])
def test_bits_equal_the_twin(dev, cin, dil):
    """B = 2; Cin = 16 (one unit: the tail alone), 32 (two units: one round of the unrolled loop, both patch buffers and nothing else), 48
    (loop + tail), 80 (two rounds + tail); Cout 8 / 64 / 72; the smallest supported H, W for the dilation and those + 1 and + 5."""
    from lanemapping_amd import ops
    H0, W0 = _smallest(ops, cin, dil)
    for d in (0, 1, 5):
        H, W = H0 + d, W0 + d
        assert ops.wino44_supported(H, W, cin, dil)
        x = _act(ops, dev, 2, cin, H, W, 7 * cin + dil + d)
        for cout in COUTS:
            w, wu, wf = _weights(ops, dev, cin, cout)
            y0 = ops.conv_wino44_twin(x, wu, cout, dil)
            y1 = ops.conv_wino44(x, wf, cout, dil)
            assert torch.equal(y0, y1), (cin, cout, dil, H, W, float((y0 - y1).abs().max()))


def test_bits_equal_the_twin_with_epilogue(dev):
    """Scale, shift, residual and ReLU; and the GroupNorm statistics of the epilogue (against the standalone statistics kernel at the
    tolerance of test_conv_winograd44_bit_identical_to_twin)."""
    from lanemapping_amd import ops
    cin, cout, dil = 48, 64, 2
    H0, W0 = _smallest(ops, cin, dil)
    H, W = H0 + 5, W0 + 5
    x = _act(ops, dev, 2, cin, H, W, 1)
    res = _act(ops, dev, 2, cout, H, W, 2)
    g = _g(3)
    sc, sh = (torch.rand(cout, generator=g) + 0.5).to(dev), torch.randn(cout, generator=g).to(dev)
    w, wu, wf = _weights(ops, dev, cin, cout)
    y0 = ops.conv_wino44_twin(x, wu, cout, dil, scale=sc, shift=sh, res=res, act=ops.ACT_RELU)
    y1 = ops.conv_wino44(x, wf, cout, dil, scale=sc, shift=sh, res=res, act=ops.ACT_RELU)
    assert torch.equal(y0, y1), float((y0 - y1).abs().max())
    y2 = ops.conv_wino44_twin(x, wu, cout, dil, shift=sh)
    y3, st = ops.conv_wino44(x, wf, cout, dil, shift=sh, gn_eps=1e-5)
    assert torch.equal(y2, y3)
    _close(st, ops.gn_stats(y3, 1e-5), 2e-5, 'gn stats from the F(4x4) epilogue')


@pytest.mark.parametrize('placement', ['channel_slice', 'end_of_allocation'])
def test_operand_extent(dev, placement):
    """The resource describes the OPERAND.  channel_slice: x = channels 16 .. 16 + Cin of a tensor twice as wide, guard rows before and
    behind; end_of_allocation: x dense, its last byte the last byte of the allocation, guard rows before.  Everything that is not x is NaN: a
    padding cell that read memory (the halo of image 0 lies in the front guard, image 1's in image 0, the right halo in the next row or
    the neighbouring channels) or a cell refused although it exists would change the output bits.  The output is a channel slice between
    canaries."""
    from lanemapping_amd import ops
    B, cin, cout, dil = 2, 48, 72, 2
    H0, W0 = _smallest(ops, cin, dil)
    H, W = H0 + 5, W0 + 5
    P = H * W
    x = torch.randn((B, cin, H, W), generator=_g(11))
    rows = x.permute(0, 2, 3, 1).reshape(B * P, cin)
    guard = (4 * dil + 2) * W + 64
    if placement == 'channel_slice':
        xs = Slab(dev, B * P, cin, 2 * cin, 16, guard, guard)
    else:
        xs = Slab(dev, B * P, cin, cin, 0, guard, 0)
        assert xs.view.data_ptr() + B * P * cin * 4 == xs.flat.data_ptr() + xs.flat.numel() * 4
    xs.fill_input(rows, NAN)
    xv = xs.flat.as_strided((B, cin, H, W), (P * xs.ld, 1, W * xs.ld, xs.ld), xs.front * xs.ld + xs.lo)
    ldy = cout + 8
    ys = Slab(dev, B * P, cout, ldy, 4, guard, guard).fill_canary()
    yv = ys.flat.as_strided((B, cout, H, W), (P * ldy, 1, W * ldy, ldy), ys.front * ldy + ys.lo)
    w, wu, wf = _weights(ops, dev, cin, cout)
    ops.conv_wino44(xv, wf, cout, dil, out=yv)
    torch.cuda.synchronize()
    ys.check_canary(f'wino44 {placement}')
    want = ops.conv_wino44_twin(ops.new_act(B, cin, H, W, dev).copy_(x.to(dev)), wu, cout, dil)
    assert bool(torch.isfinite(want).all())
    assert torch.equal(yv, want), int((yv != want).sum())
    assert torch.equal(xs.view.cpu(), rows)


def test_offsets_beyond_4gib(dev):
    """Cin = Cout = 16 at 288 x 288 with so many images that the input exceeds 4 GiB: the image base is a 64-bit address, only the offset
    inside an image has 32 bits.  The last two images equal a run on those two alone (and that run the twin)."""
    from lanemapping_amd import ops
    c, H, W = 16, 288, 288
    B = (1 << 32) // (H * W * c * 4) + 1
    x = torch.randn((B, H, W, c), device=dev).permute(0, 3, 1, 2)
    assert x.numel() * 4 > 1 << 32
    w, wu, wf = _weights(ops, dev, c, c)
    y = ops.conv_wino44(x, wf, c)
    tail = x[B - 2:]
    yt = ops.conv_wino44(tail, wf, c)
    assert torch.equal(y[B - 2:], yt)
    assert torch.equal(yt, ops.conv_wino44_twin(tail, wu, c))
    del x, y


@pytest.mark.parametrize('over', [0, 64])
def test_image_of_2gib(dev, over):
    """One 64 x 64 image of 32 channels, a slice of a tensor of 2^17 + `over` channels: H W ldx 4 >= 2^31 bytes.  The kernel takes an image
    while the bytes from its first pixel to the end of its last pixel's operand channels stay below 2^31 (over = 0: then the bits are the
    twin's); beyond that the entry point refuses, ops.wino44_supported(..., ldx) says so, and FPNEncoder._c3 gives the layer to the direct
    kernel (over = 64: within 1e-4 of the twin, the tolerance between the two kernels in test_conv_winograd44_random_shapes_vs_twin)."""
    from lanemapping_amd import ops
    from lanemapping_amd.pcencoder import FPNEncoder
    cin, cout, H, W = 32, 64, 64, 64
    ldx = (1 << 17) + over
    assert H * W * ldx * 4 >= 1 << 31
    wide = torch.full((1, H, W, ldx), NAN, device=dev)
    x = torch.randn((1, cin, H, W), generator=_g(21)).to(dev)
    xv = wide.permute(0, 3, 1, 2)[:, 16:16 + cin]
    xv.copy_(x)
    w, wu, wf = _weights(ops, dev, cin, cout)
    want = ops.conv_wino44_twin(xv, wu, cout)
    assert bool(torch.isfinite(want).all())
    fits = ((H * W - 1) * ldx + cin) * 4 < 1 << 31
    assert fits == (over == 0) and ops.wino44_supported(H, W, cin, 1, ldx) == fits and ops.wino44_covers(xv) == fits
    if fits:
        assert torch.equal(ops.conv_wino44(xv, wf, cout), want)
    else:
        with pytest.raises(RuntimeError, match='2\\^31'):
            ops.conv_wino44(xv, wf, cout)
    y = FPNEncoder._c3(xv, {'k': ops.pack_mfma(w), 'kq': wf}, 'k', cout, 1, 1)
    if fits:
        assert torch.equal(y, want)
    else:
        _close(y, want, 1e-4, 'direct kernel on the refused image')
    del wide
