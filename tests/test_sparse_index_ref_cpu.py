"""CPU: the brute-force references of tests/sparse_ref.py against the dense formulation the project already trusts
(oracle/lidar_ref.py::_spconv: conv3d of the active mask with a ones kernel, conv3d of the zero-filled volume), for every geometry,
volume and active set tests/test_gpu_sparse_index.py runs.  A wrong reference cannot then quietly agree with a wrong kernel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_ref as R

CASES = [(g, v, s) for g in R.GEOMETRIES + [R.SUBM] for v in R.VOLUMES for s in R.SETS]
IDS = [f'{R.geom_id(g)}-{v[0]}x{v[1]}x{v[2]}-{s}' for g, v, s in CASES]


def test_grid_ref_by_hand():
    c = np.array([[1, 0, 2, 1], [0, 1, 0, 0], [1, 1, 2, 2]], np.int32)
    g = R.grid_ref(c, 2, (2, 3, 3))
    assert g.shape == (2, 2, 3, 3) and g.dtype == np.int32 and int((g >= 0).sum()) == 3
    assert g[1, 0, 2, 1] == 0 and g[0, 1, 0, 0] == 1 and g[1, 1, 2, 2] == 2
    assert np.all(R.grid_ref(np.zeros((0, 4), np.int32), 1, (1, 2, 2)) == -1)


def test_rulebook_tap_order_by_hand():
    """One output at (0, 1, 1, 1) of a (1, 2, 3) kernel, stride 1, no padding: tap t = ky * 3 + kx reads (z 1, y 1 + ky, x 1 + kx)."""
    inc = np.array([[0, 1, 2, 3], [0, 1, 1, 2], [0, 1, 1, 1], [1, 1, 1, 1]], np.int32)
    nbr = R.rulebook_ref(np.array([[0, 1, 1, 1]], np.int32), inc, (2, 3, 4), (1, 2, 3), (1, 1, 1), (0, 0, 0))
    assert nbr.tolist() == [[2, 1, -1, -1, -1, 0]]


@pytest.mark.parametrize('geom,shape,aset', CASES, ids=IDS)
def test_references_vs_dense_conv3d(geom, shape, aset):
    kernel, stride, padding = geom
    B, inc = R.active_sets(shape)[aset]
    out_shape, oc, og = R.conv_outputs_ref(inc, B, shape, kernel, stride, padding)
    # active mask: lidar_ref._spconv's construction
    mask = torch.zeros((B, 1) + tuple(shape))
    c = torch.from_numpy(inc).long()
    mask[c[:, 0], 0, c[:, 1], c[:, 2], c[:, 3]] = 1.0
    want = (F.conv3d(mask, torch.ones((1, 1) + tuple(kernel)), stride=stride, padding=padding) > 0)[:, 0].numpy()
    assert og.shape == want.shape == (B,) + out_shape
    assert np.array_equal(og >= 0, want)
    assert len(oc) == int(want.sum()) and np.array_equal(oc, np.argwhere(want).astype(np.int32))      # argwhere: ascending (b, z, y, x)
    assert np.array_equal(og[tuple(oc.T)], np.arange(len(oc)))
    # rulebook: the sum over taps is the dense convolution at the active output sites
    if geom == R.SUBM:
        oc = inc                                                                  # submanifold: out == in, in the input's row order
    nbr = R.rulebook_ref(oc, inc, shape, kernel, stride, padding)
    taps = kernel[0] * kernel[1] * kernel[2]
    assert nbr.shape == (len(oc), taps) and nbr.dtype == np.int32
    g = torch.Generator().manual_seed(len(inc) + taps)
    cin, cout = 3, 2
    x = torch.randn(len(inc), cin, generator=g, dtype=torch.float64)
    w = torch.randn(*kernel, cin, cout, generator=g, dtype=torch.float64)
    xe = torch.cat([x, torch.zeros(1, cin, dtype=torch.float64)])
    gath = xe[torch.from_numpy(np.where(nbr < 0, len(inc), nbr)).long()]             # [n_out, taps, cin]
    got = torch.einsum('mtc,tco->mo', gath, w.reshape(taps, cin, cout))
    ref = R.conv3d_rows_ref(x, inc, B, shape, w, kernel, stride, padding, oc)
    assert got.shape == ref.shape == (len(oc), cout)
    if len(oc):                       # the asymmetric geometry reaches no cell of the placed set in the (5, 6, 7) volume: no output at all
        assert float((got - ref).abs().max()) <= 1e-12


def test_placed_set_holds_what_it_claims():
    for shape in R.VOLUMES:
        D, H, W = shape
        B, c = R.active_sets(shape)['placed']
        s = {tuple(int(v) for v in r) for r in c}
        assert B == 4 and len(s) == len(c) and not any(r[0] == 1 for r in s)
        for b in (0, 2, 3):
            assert all((b, z, y, x) in s for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1))
            assert (b, 1, 2, W - 1) in s and (b, 1, 3, 0) in s and (b, 2, H - 1, 3) in s and (b, 3, 0, 3) in s
        assert (2, D - 1, H - 1, W - 1) in s and (3, 0, 0, 0) in s
