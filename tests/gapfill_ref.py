"""The gap fill of sparse tiles (csrc/gapfill.hip) restated in numpy, for tests/test_gapfill_cpu.py and tests/test_gpu_gapfill.py: a loop
over the offsets of the disc in ascending d2 on a zero-padded copy of the tile.  Integers only; it shares no code with the package and
does not call it.

  value     R << 16 | G << 8 | B of every pixel; 0 = empty
  search    per pixel the gap (the smallest d2 <= R^2 to a non-empty pixel of the same tile; 0 for a non-empty pixel, -1 = far) and the
            largest value at that d2
  hist      [B, Rmax + 2]: non-empty, ring 1 .. Rmax (ring k = the smallest k with k^2 >= gap), far
  fill      the filled tiles for one radius per tile
"""
import numpy as np


def value(tile):
    t = np.asarray(tile)
    assert t.dtype == np.uint8 and t.ndim == 3 and t.shape[2] == 3
    t = t.astype(np.int64)
    return t[..., 0] << 16 | t[..., 1] << 8 | t[..., 2]


def disc(R):
    """The offsets (d2, dr, dc) of the disc of radius R without its centre, ascending in d2."""
    return sorted((dr * dr + dc * dc, dr, dc) for dr in range(-R, R + 1) for dc in range(-R, R + 1) if 0 < dr * dr + dc * dc <= R * R)


def search(tile, R):
    """-> (gap [H, W] int64, best [H, W] int64): for an empty pixel with a non-empty pixel within the disc of radius R the smallest d2
    and the largest value among the pixels at that d2; gap 0 / best 0 for a non-empty pixel, gap -1 / best 0 for a far one."""
    v = value(tile)
    H, W = v.shape
    pad = np.zeros((H + 2 * R, W + 2 * R), np.int64)                # pixels outside the tile do not exist: they are empty
    pad[R:R + H, R:R + W] = v
    gap = np.where(v > 0, 0, -1)
    best = np.zeros((H, W), np.int64)
    for d2, dr, dc in disc(R):
        q = pad[R + dr:R + dr + H, R + dc:R + dc + W]
        # an empty pixel not settled at a smaller d2: the first non-empty q opens the class d2, later ones of the class compete by value
        take = (v == 0) & (q > 0) & ((gap == -1) | ((gap == d2) & (q > best)))
        gap[take] = d2
        best[take] = q[take]
    return gap, best


def ring(d2):
    k = 0
    while k * k < d2:
        k += 1
    return k


def hist(tiles, Rmax):
    tiles = np.asarray(tiles)
    out = np.zeros((tiles.shape[0], Rmax + 2), np.int64)
    for b, t in enumerate(tiles):
        gap, _ = search(t, Rmax)
        out[b, 0] = (gap == 0).sum()
        out[b, Rmax + 1] = (gap == -1).sum()
        for d2 in np.unique(gap[gap > 0]):
            out[b, ring(int(d2))] += (gap == d2).sum()
        assert out[b].sum() == t.shape[0] * t.shape[1]
    return out


def fill(tiles, radii):
    tiles = np.asarray(tiles)
    radii = [int(radii)] * tiles.shape[0] if np.ndim(radii) == 0 else [int(r) for r in radii]
    assert len(radii) == tiles.shape[0]
    out = tiles.copy()
    for b, (t, r) in enumerate(zip(tiles, radii)):
        gap, best = search(t, r)
        m = gap > 0
        out[b][m] = np.stack([best[m] >> 16, (best[m] >> 8) & 255, best[m] & 255], axis=1).astype(np.uint8)
    return out
