"""Brute-force references of the sparse-voxel index kernels (tests/test_gpu_sparse_index.py), plain numpy.

Written from the definitions in the header of csrc/lidar.hip, not from its kernels: an output site (b, oz, oy, ox) of a SparseConv3d
is active iff an active input lies at o * stride - padding + k for some tap k of the kernel; the rulebook lists, per output row and tap
(kz, ky, kx with kx fastest), the input row at that site or -1.  Everything loops over sites and taps; the volumes of the tests hold a
few thousand cells.  tests/test_sparse_index_ref_cpu.py holds these references to the dense conv3d formulation of oracle/lidar_ref.py.

GEOMETRIES / VOLUMES / active_sets() are the cases shared by the CPU and the GPU file."""
import itertools

import numpy as np

# (kernel, stride, padding), each (z, y, x)
GEOMETRIES = [
    ((3, 3, 3), (2, 2, 2), (1, 1, 1)),
    ((3, 3, 3), (2, 2, 2), (0, 1, 1)),
    ((3, 3, 3), (2, 2, 2), (1, 1, 0)),
    ((3, 3, 3), (2, 2, 2), (0, 0, 0)),
    ((3, 1, 1), (2, 1, 1), (0, 0, 0)),      # conv_out of the network
    ((3, 3, 3), (1, 1, 1), (1, 1, 1)),      # a strided-type layer that only dilates the set
    ((2, 2, 2), (2, 2, 2), (0, 0, 0)),
    ((1, 1, 1), (2, 2, 2), (0, 0, 0)),      # stride above kernel: inputs at odd coordinates feed nothing
    ((1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ((3, 1, 2), (2, 1, 3), (1, 0, 2)),      # asymmetric: pins the tap order and the axis order of all three triples
]
SUBM = ((3, 3, 3), (1, 1, 1), (1, 1, 1))
BATCH = 3
VOLUMES = [(5, 6, 7), (4, 9, 8)]            # (D, H, W): (in + 2p - k) % s is zero on some axes and non-zero on others
SETS = ['random', 'full', 'placed']


def geom_id(g):
    return 'k{}{}{}_s{}{}{}_p{}{}{}'.format(*g[0], *g[1], *g[2])


def _raster(coords):
    """Unique rows of an [n,4] list in ascending (b, z, y, x) order."""
    c = np.unique(np.asarray(coords, np.int64).reshape(-1, 4), axis=0)
    return c.astype(np.int32)


def active_sets(shape):
    """{name: (B, coords [n,4] int32 (b, z, y, x), rows in a seeded SHUFFLED order)} for one input volume.  'random' and 'full' have
    B = 3.  'placed' has B = 4: sample 1 is completely empty AND the last cell of one sample meets the first cell of the next
    (samples 2 / 3), which three samples cannot hold at once."""
    D, H, W = shape
    rng = np.random.RandomState(D * 100 + H * 10 + W)
    every = np.array(list(itertools.product(range(BATCH), range(D), range(H), range(W))), np.int32)
    rnd = every[rng.rand(len(every)) < 0.15]
    placed = []
    for b in (0, 2, 3):                                                     # sample 1 stays completely empty
        # the eight corners; (D-1, H-1, W-1) of sample 2 and (0, 0, 0) of sample 3 are neighbours in a linear cell index
        placed += [(b, z, y, x) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)]
        placed += [(b, 1, 2, W - 1), (b, 1, 3, 0)]                          # last cell of a row, first cell of the next row
        placed += [(b, 2, H - 1, 3), (b, 3, 0, 3)]                          # last row of a plane, first row of the next plane
    out = {'random': (BATCH, rnd), 'full': (BATCH, every), 'placed': (4, _raster(placed))}
    return {k: (B, v[rng.permutation(len(v))].copy()) for k, (B, v) in out.items()}


def out_shape_of(in_shape, kernel, stride, padding):
    return tuple((in_shape[a] + 2 * padding[a] - kernel[a]) // stride[a] + 1 for a in range(3))


def grid_ref(coords, B, shape):
    """int32 [B, D, H, W]: -1 everywhere except grid[coords[i]] = i."""
    D, H, W = shape
    grid = np.full((B, D, H, W), -1, np.int32)
    for i, (b, z, y, x) in enumerate(np.asarray(coords).reshape(-1, 4)):
        grid[b, z, y, x] = i
    return grid


def conv_outputs_ref(in_coords, B, in_shape, kernel, stride, padding):
    """-> (out_shape, out_coords [n_out,4] int32 in ascending (b, z, y, x) order, out_grid [B, Do, Ho, Wo] int32 row index or -1)."""
    D, H, W = in_shape
    active = {tuple(int(v) for v in c) for c in np.asarray(in_coords).reshape(-1, 4)}
    Do, Ho, Wo = out_shape = out_shape_of(in_shape, kernel, stride, padding)
    out_grid = np.full((B, Do, Ho, Wo), -1, np.int32)
    out_coords = []
    for b in range(B):
        for oz in range(Do):
            for oy in range(Ho):
                for ox in range(Wo):
                    hit = False
                    for kz in range(kernel[0]):
                        for ky in range(kernel[1]):
                            for kx in range(kernel[2]):
                                site = (b, oz * stride[0] - padding[0] + kz, oy * stride[1] - padding[1] + ky,
                                        ox * stride[2] - padding[2] + kx)
                                hit = hit or site in active
                    if hit:
                        out_grid[b, oz, oy, ox] = len(out_coords)
                        out_coords.append((b, oz, oy, ox))
    return out_shape, np.asarray(out_coords, np.int32).reshape(-1, 4), out_grid


def rulebook_ref(out_coords, in_coords, in_shape, kernel, stride, padding):
    """-> int32 [n_out, kz*ky*kx]: row of the active input at o * s - p + k, taps ordered (kz, ky, kx) with kx fastest, -1 if none."""
    D, H, W = in_shape
    row_of = {tuple(int(v) for v in c): i for i, c in enumerate(np.asarray(in_coords).reshape(-1, 4))}
    out_coords = np.asarray(out_coords).reshape(-1, 4)
    nbr = np.full((len(out_coords), kernel[0] * kernel[1] * kernel[2]), -1, np.int32)
    for m, (b, oz, oy, ox) in enumerate(out_coords):
        t = 0
        for kz in range(kernel[0]):
            for ky in range(kernel[1]):
                for kx in range(kernel[2]):
                    z, y, x = oz * stride[0] - padding[0] + kz, oy * stride[1] - padding[1] + ky, ox * stride[2] - padding[2] + kx
                    if 0 <= z < D and 0 <= y < H and 0 <= x < W:
                        nbr[m, t] = row_of.get((int(b), int(z), int(y), int(x)), -1)
                    t += 1
    return nbr


def dense_volume(feats, coords, B, shape):
    """Zero-filled float64 [B, C, D, H, W] with feats [n, C] at coords."""
    import torch
    D, H, W = shape
    feats = torch.as_tensor(feats, dtype=torch.float64)
    c = torch.as_tensor(np.asarray(coords)).long()
    x = torch.zeros((B, feats.shape[1], D, H, W), dtype=torch.float64)
    x[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = feats
    return x


def conv3d_rows_ref(feats, in_coords, B, in_shape, w, kernel, stride, padding, out_coords):
    """float64 F.conv3d of the zero-filled volume, read at out_coords -> [n_out, Cout].  w: [kD, kH, kW, Cin, Cout]."""
    import torch
    import torch.nn.functional as F
    x = dense_volume(feats, in_coords, B, in_shape)
    y = F.conv3d(x, torch.as_tensor(w, dtype=torch.float64).permute(4, 3, 0, 1, 2).contiguous(), stride=stride, padding=padding)
    c = torch.as_tensor(np.asarray(out_coords)).long()
    return y[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]
