"""Plain NumPy references of the sparse-conv kernels (``csrc/kernels/spconv.hip``),
one per kernel, written from the kernels' documented contract and from
``models/second.py`` — sequential semantics, fp64 wherever values are involved.

Conventions: coords are int [N, 4] = (b, z, y, x); ``ksp`` is the 9-tuple
(kz, ky, kx, sz, sy, sx, pz, py, px) the launchers take; a grid is an int array
[B, Z, Y, X] holding the row of each site (negative = no row); the tap index
is ``(kz*KY + ky)*KX + kx``; the device neighbour table is ``nbr[tile][tap][64]``
(64 output rows per tile) with one 32-bit tap mask per tile.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

TILE = 64


def sp_out_dims(in_dims: Sequence[int], ksp: Sequence[int]) -> Tuple[int, int, int]:
    k, s, p = ksp[0:3], ksp[3:6], ksp[6:9]
    return tuple((in_dims[d] + 2 * p[d] - k[d]) // s[d] + 1 for d in range(3))  # type: ignore


def sp_taps(ksp: Sequence[int]) -> np.ndarray:
    """[KT, 3] (kz, ky, kx) in tap-index order."""
    kz, ky, kx = ksp[0:3]
    return np.stack(np.meshgrid(np.arange(kz), np.arange(ky), np.arange(kx), indexing="ij"), -1).reshape(-1, 3)


def sp_out_sites(coords: np.ndarray, ksp: Sequence[int], out_dims: Sequence[int]) -> np.ndarray:
    """Output sites of a strided conv: every (b, o) with ``o*s - p + k == i`` for
    some input site i and tap k, ``0 <= o < out_dim``.  int32 [M, 4], rows sorted."""
    coords = np.asarray(coords, np.int64).reshape(-1, 4)
    s, p = np.asarray(ksp[3:6]), np.asarray(ksp[6:9])
    od = np.asarray(out_dims)
    found = set()
    for k in sp_taps(ksp):
        num = coords[:, 1:] + p - k  # = o * s
        o = num // s
        ok = ((num >= 0) & (o * s == num) & (o < od)).all(1)
        for b, (z, y, x) in zip(coords[ok, 0], o[ok]):
            found.add((int(b), int(z), int(y), int(x)))
    return np.asarray(sorted(found), np.int32).reshape(-1, 4)


def sp_grid(coords: np.ndarray, batch: int, dims: Sequence[int]) -> np.ndarray:
    """[B, Z, Y, X] int32: row of every site of ``coords``, -1 elsewhere."""
    g = np.full((batch, *dims), -1, np.int32)
    c = np.asarray(coords, np.int64).reshape(-1, 4)
    g[c[:, 0], c[:, 1], c[:, 2], c[:, 3]] = np.arange(len(c), dtype=np.int32)
    return g


def sp_neighbour_table(out_coords: np.ndarray, ksp: Sequence[int], in_dims: Sequence[int],
                       in_grid: np.ndarray) -> np.ndarray:
    """nbr [rows, KT] int32: the input row at ``o*s - p + k`` of the same frame, -1
    where that coordinate is out of range or the grid holds no row (any negative value)."""
    oc = np.asarray(out_coords, np.int64).reshape(-1, 4)
    s, p = np.asarray(ksp[3:6]), np.asarray(ksp[6:9])
    taps = sp_taps(ksp)
    g = np.asarray(in_grid).reshape(-1, *in_dims)
    i = oc[:, None, 1:] * s - p + taps[None]  # [rows, KT, 3]
    inside = ((i >= 0) & (i < np.asarray(in_dims))).all(-1)
    j = np.where(inside[..., None], i, 0)
    v = g[oc[:, 0:1], j[..., 0], j[..., 1], j[..., 2]]
    return np.where(inside & (v >= 0), v, -1).astype(np.int32)


def sp_pack_nbr(nbr: np.ndarray, tiles: int | None = None, fill: int = -1) -> np.ndarray:
    """[rows, KT] → the device layout [tiles, KT, 64] (rows past the table = fill)."""
    rows, kt = nbr.shape
    need = (rows + TILE - 1) // TILE
    tiles = need if tiles is None else tiles
    assert tiles >= need
    out = np.full((tiles * TILE, kt), fill, np.int32)
    out[:rows] = nbr
    return np.ascontiguousarray(out.reshape(tiles, TILE, kt).transpose(0, 2, 1))


def sp_unpack_nbr(packed: np.ndarray, rows: int) -> np.ndarray:
    """Device layout [tiles, KT, 64] → [rows, KT]."""
    tiles, kt, _ = packed.shape
    return np.ascontiguousarray(packed.transpose(0, 2, 1).reshape(tiles * TILE, kt)[:rows])


def sp_tap_masks(nbr: np.ndarray) -> np.ndarray:
    """uint32 [ceil(rows / 64)]: bit t of a tile's word = some row of the tile has tap t."""
    rows, kt = nbr.shape
    out = np.zeros(((rows + TILE - 1) // TILE,), np.uint32)
    for i in range(len(out)):
        present = (nbr[i * TILE:(i + 1) * TILE] >= 0).any(0)
        out[i] = sum(1 << t for t in range(kt) if present[t])
    return out


def sp_gather_gemm_ref(inp: np.ndarray, nbr: np.ndarray, w: np.ndarray, bias: np.ndarray, act: int):
    """``out[r, n] = act(sum_{t, c} inp[nbr[r, t], c] * w[n, t, c] + bias[n])`` in fp64
    (absent neighbours contribute zero; act 1 = ReLU), and ``S[r, n] = sum |a||w| + |bias|``,
    the scale of the accumulation's rounding error."""
    x = np.concatenate([np.asarray(inp, np.float64), np.zeros((1, inp.shape[1]))], 0)
    g = x[np.where(nbr >= 0, nbr, len(x) - 1)]  # [rows, KT, Cin]
    w64, b64 = np.asarray(w, np.float64), np.asarray(bias, np.float64)
    out = np.einsum("rtc,ntc->rn", g, w64) + b64
    S = np.einsum("rtc,ntc->rn", np.abs(g), np.abs(w64)) + np.abs(b64)
    if act == 1:
        out = np.maximum(out, 0.0)
    return out, S


def mean_vfe_voxels_ref(voxels: np.ndarray, num_points: np.ndarray):
    """MeanVFE of materialised voxels [V, P, F]: sum of all P slots (padding is zero)
    of the first four features / max(n, 1), fp64.  Also returns sum |x| / max(n, 1)."""
    v = np.asarray(voxels, np.float64)[:, :, :4]
    n = np.maximum(np.asarray(num_points, np.float64), 1.0)[:, None]
    return v.sum(1) / n, np.abs(v).sum(1) / n


def mean_vfe_slots_ref(pts: np.ndarray, slots: np.ndarray, vcount: np.ndarray, max_per_voxel: int):
    """MeanVFE from slot lists: pts [max_pts, >= 4] of one frame, slots [V, P] point
    indices, vcount [V] (clamped to P).  fp64 mean and sum |x| / max(n, 1)."""
    V = len(vcount)
    mean, mag = np.zeros((V, 4)), np.zeros((V, 4))
    for v in range(V):
        m = min(int(vcount[v]), max_per_voxel)
        x = np.asarray(pts[slots[v, :m], :4], np.float64).reshape(m, 4)
        mean[v], mag[v] = x.sum(0) / max(m, 1), np.abs(x).sum(0) / max(m, 1)
    return mean, mag


def sp_edge_sites(rng: np.random.Generator, dims: Sequence[int], n: int | None = None,
                  occupancy: float = 0.1) -> np.ndarray:
    """The site set the kernel tests run on: two frames over ``dims`` (Z, Y, X, each
    >= 9 / 12 / 12) holding, on top of random occupancy (``n`` sites in all if given),

    * the 8 grid corners of both frames — (0, Z-1, Y-1, X-1) and (1, 0, 0, 0) are
      neighbours in the flattened grid, so a missing bounds check links them;
    * one dense 4x4x4 block (frame 0): all 27 taps present;
    * one isolated site (frame 1, nothing within two cells): centre tap only;
    * one sub-block with the same occupancy at the same coordinates in both frames.

    Returns int32 [N, 4] rows (b, z, y, x) in random order."""
    Z, Y, X = dims
    forced = np.zeros((2, Z, Y, X), bool)
    keep_out = np.zeros((2, Z, Y, X), bool)
    for b in range(2):
        for z in (0, Z - 1):
            for y in (0, Y - 1):
                for x in (0, X - 1):
                    forced[b, z, y, x] = True
    forced[0, 2:6, 3:7, 4:8] = True
    forced[1, 4, 3, 3] = True
    keep_out[1, 2:7, 1:6, 1:6] = True
    sub = rng.random((2, 3, 3)) < 0.6
    sub[0, 0, 0] = sub[1, 2, 2] = True
    for b in range(2):
        forced[b, 6:8, 8:11, 9:12] = sub
        keep_out[b, 6:8, 8:11, 9:12] = True
    free = np.flatnonzero(~forced & ~keep_out)
    extra = int(round(occupancy * forced.size)) if n is None else n - int(forced.sum())
    assert 0 <= extra <= len(free)
    mask = forced.copy()
    mask.reshape(-1)[rng.choice(free, extra, replace=False)] = True
    coords = np.argwhere(mask).astype(np.int32)
    return coords[rng.permutation(len(coords))]
