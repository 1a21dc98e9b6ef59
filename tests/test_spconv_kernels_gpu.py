"""csrc/kernels/spconv.hip entry point by entry point against exact (integer) and
fp64 references (ops/spconv_ref.py), on small grids with three distinct extents,
forced edge sites and sentinel-filled guards around every output buffer.

Tolerances (all per element; none is tuned to what the kernels return):

* gather GEMM bf16: ``2^-8 |ref| + 2 K 2^-24 S`` — inputs / weights pre-rounded to bf16,
  K the padded reduction length, S = sum |a||w| + |bias|.  First term: the bf16 output
  rounding (half an ulp is at most 2^-8 of the value); second: fp32 accumulation of K
  terms, doubled for the MFMA's unspecified internal order.
* gather GEMM x3 (fp32 mode): ``(2^-16 + 2 K 2^-24) S`` — hi + lo residuals of both
  operands (2^-18 each) plus the dropped lo*lo term (2^-18) stay under 2^-16 S
  (tca_mfma.h); the test proves on the CPU that a missing cross term exceeds it.
* MeanVFE fp32: ``(P + 1) 2^-24 sum|x| / max(n, 1)`` (P additions and one multiply by
  the rounded reciprocal); bf16: the same plus ``2^-8 |ref|``.
* RoI grid pool: the existing tests' bounds (relative L2 1e-2 bf16, 1e-5 fp32).
* Rescore: ``2^-23 (4 + |x|)`` relative, derived at the test.
* Voxeliser-driven backbone, fp32 mode: the sibling test's bound (relative L2 2e-4).
"""
import ctypes
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

from triton_client_amd.config.lidar import KITTI_SECOND_VOXELS, SecondIoUConfig
from triton_client_amd.ops import spconv_ref as R

DIMS = (9, 12, 14)
BIG_DIMS = (11, 16, 18)  # 10 % occupancy of two frames gives > 600 sites
GUARD = 64               # elements on either side of every output buffer (a multiple of 16 B)
I32_SENT = -1234567
F32_NAN = 0x7FC0ABCD     # NaN bit patterns: compared as integers
BF16_NAN = 0x7FCB

KSP = {
    "subm": (3, 3, 3, 1, 1, 1, 1, 1, 1),
    "s2_p1": (3, 3, 3, 2, 2, 2, 1, 1, 1),
    "s2_p011": (3, 3, 3, 2, 2, 2, 0, 1, 1),
    "k311": (3, 1, 1, 2, 1, 1, 0, 0, 0),
}
STRIDED = ["s2_p1", "s2_p011", "k311"]


def _iarr(v):
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bf16(a):
    """fp32 array rounded to bf16 (round to nearest even), as a torch bf16 tensor."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16)


class Buf:
    """Device output buffer of n elements between two sentinel guards; the body starts
    as the sentinel too unless ``fill`` is given.  kind: i32 / i64 / f32 / bf16."""
    _DT = {"i32": torch.int32, "i64": torch.int64, "f32": torch.int32, "bf16": torch.int16}
    _SENT = {"i32": I32_SENT, "i64": I32_SENT, "f32": F32_NAN, "bf16": BF16_NAN}

    def __init__(self, dev, n, kind, fill=None):
        self.kind, self.n, self.sent = kind, int(n), self._SENT[kind]
        self.t = torch.full((self.n + 2 * GUARD,), self.sent, dtype=self._DT[kind], device=dev)
        if fill is not None:
            self.t[GUARD:GUARD + self.n] = fill
        self.ptr = self.t.data_ptr() + GUARD * self.t.element_size()

    def bits(self):
        """Body as integers; asserts that both guards are untouched."""
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == self.sent).all() and (a[GUARD + self.n:] == self.sent).all(), "guard overwritten"
        return a[GUARD:GUARD + self.n]

    def split(self):
        """(values as fp64, mask of body elements still holding the sentinel)."""
        b = self.bits()
        if self.kind == "bf16":
            v = (b.astype(np.uint16).astype(np.uint32) << 16).view(np.float32)
        else:
            v = b.view(np.float32)
        return v.astype(np.float64), b == self.sent


def _call(name, *args):
    from triton_client_amd import _native
    _native.call(name, *args, _native.stream_ptr())


def _sort_rows(c):
    return c[np.lexsort(c.T[::-1])]


# ------------------------------------------------------------------------------------------ claim
def _claim(dev, coords, n_dev, cap_in, ksp, od, cap_out, batch=2):
    assert cap_in <= len(coords)
    grid = Buf(dev, batch * od[0] * od[1] * od[2], "i32", fill=-1)
    co = Buf(dev, cap_out * 4, "i32")
    cnt = Buf(dev, 1, "i32", fill=0)
    cin, nin = _dev(coords, dev), _dev(np.array([n_dev], np.int32), dev)
    _call("tca_sp_claim", cin.data_ptr(), nin.data_ptr(), cap_in, _iarr(ksp), _iarr(od), grid.ptr, co.ptr, cnt.ptr,
          cap_out)
    torch.cuda.synchronize()
    return grid.bits().reshape(batch, *od), co.bits().reshape(cap_out, 4), int(cnt.bits()[0])


def _check_claim(grid, co, n, ref, od):
    assert n == len(ref)
    rows = co[:n]
    assert np.array_equal(_sort_rows(rows), ref)  # ref rows are unique: so are these
    assert np.array_equal(grid, R.sp_grid(rows, 2, od))  # grid[site(row r)] == r, every other cell -1
    assert (co[n:] == I32_SENT).all()


def _spare_coords(rng, dims, n):
    return np.stack([rng.integers(0, 2, n)] + [rng.integers(0, d, n) for d in dims], 1).astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 640])
@pytest.mark.parametrize("kind", STRIDED)
def test_claim_output_sites(cuda, kind, n):
    ksp = KSP[kind]
    rng = np.random.default_rng(10 + n)
    dims = BIG_DIMS if n > 400 else DIMS
    if n == 1:
        coords = np.array([[0, dims[0] - 1, dims[1] - 1, dims[2] - 1]], np.int32)
    else:
        coords = R.sp_edge_sites(rng, dims, n=n)
    assert len(coords) == n
    od = R.sp_out_dims(dims, ksp)
    ref = R.sp_out_sites(coords, ksp, od)
    # rows past the device count hold valid coordinates: a kernel that ignored the count would claim them
    buf = np.concatenate([coords, _spare_coords(rng, dims, 13)])
    grid, co, got = _claim(cuda, buf, n, len(buf), ksp, od, len(ref) + 20)
    _check_claim(grid, co, got, ref, od)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", STRIDED)
def test_claim_count_above_capacity_uses_cap_in_rows(cuda, kind):
    ksp = KSP[kind]
    coords = R.sp_edge_sites(np.random.default_rng(20), DIMS)
    cap_in = len(coords) - 50
    od = R.sp_out_dims(DIMS, ksp)
    ref = R.sp_out_sites(coords[:cap_in], ksp, od)
    assert len(ref) < len(R.sp_out_sites(coords, ksp, od))
    grid, co, got = _claim(cuda, coords, len(coords) + 100, cap_in, ksp, od, len(ref) + 20)
    _check_claim(grid, co, got, ref, od)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", STRIDED)
def test_claim_capacity_clamp(cuda, kind):
    """cap_out = count - 5: nothing lands past cap_out, exactly 5 sites stay claimed but
    rowless (-2), and a rulebook over that grid treats them as absent."""
    ksp = KSP[kind]
    coords = R.sp_edge_sites(np.random.default_rng(21), DIMS)
    od = R.sp_out_dims(DIMS, ksp)
    ref = R.sp_out_sites(coords, ksp, od)
    cap = len(ref) - 5
    grid, co, got = _claim(cuda, coords, len(coords), len(coords), ksp, od, cap)
    assert got == len(ref)
    want = R.sp_grid(ref, 2, od) >= 0
    assert (grid[~want] == -1).all()
    assert (grid[want] == -2).sum() == 5 and (grid == -2).sum() == 5
    held = grid[want & (grid != -2)]
    assert np.array_equal(np.sort(held), np.arange(cap))  # every row < cap_out, each used once
    c = co.astype(np.int64)
    assert np.array_equal(grid[c[:, 0], c[:, 1], c[:, 2], c[:, 3]], np.arange(cap))
    # SubM rulebook of the output level over this grid: the -2 cells are no neighbours
    sub = KSP["subm"]
    nbr, mask = _rulebook(cuda, co, cap, cap, sub, od, grid)
    exp = R.sp_neighbour_table(co, sub, od, grid)
    got_nbr = R.sp_unpack_nbr(nbr, cap)
    assert np.array_equal(got_nbr >= 0, exp >= 0) and np.array_equal(got_nbr[exp >= 0], exp[exp >= 0])
    assert (got_nbr[exp < 0] < 0).all()
    assert np.array_equal(mask[:len(R.sp_tap_masks(exp))], R.sp_tap_masks(exp))


# --------------------------------------------------------------------------------------- rulebook
def _rulebook(dev, out_coords, n_dev, cap, ksp, in_dims, in_grid):
    """→ (nbr bits [tiles + 1, KT, 64], tap masks uint32 [tiles + 1]); one spare tile each."""
    assert cap <= len(out_coords)
    kt = ksp[0] * ksp[1] * ksp[2]
    tiles = (cap + 63) // 64 + 1
    nbr = Buf(dev, tiles * kt * 64, "i32")
    mask = Buf(dev, tiles, "i32")
    co, nn = _dev(out_coords, dev), _dev(np.array([n_dev], np.int32), dev)
    g = _dev(np.asarray(in_grid, np.int32).reshape(-1), dev)
    _call("tca_sp_rulebook", co.data_ptr(), nn.data_ptr(), cap, _iarr(ksp), _iarr(in_dims), g.data_ptr(), nbr.ptr,
          mask.ptr)
    torch.cuda.synchronize()
    return nbr.bits().reshape(tiles, kt, 64), mask.bits().view(np.uint32)


def _check_rulebook(nbr, mask, n, exp):
    tiles, kt, _ = nbr.shape
    assert np.array_equal(R.sp_unpack_nbr(nbr, n), exp)
    live = (n + 63) // 64
    assert np.array_equal(mask[:live], R.sp_tap_masks(exp))
    flat = nbr.transpose(0, 2, 1).reshape(tiles * 64, kt)
    assert (flat[n:] == I32_SENT).all()  # rest of the last tile and every later tile
    assert (mask[live:] == np.uint32(I32_SENT & 0xFFFFFFFF)).all()


@functools.lru_cache(maxsize=None)
def _rulebook_level(kind):
    """(input coords, input grid, output coords in random order) for a layer kind."""
    ksp = KSP[kind]
    rng = np.random.default_rng(30)
    coords = R.sp_edge_sites(rng, DIMS)
    grid = R.sp_grid(coords, 2, DIMS)
    if kind == "subm":
        return coords, grid, coords
    out = R.sp_out_sites(coords, ksp, R.sp_out_dims(DIMS, ksp))
    return coords, grid, out[rng.permutation(len(out))]


def _full_row_first(out, ksp, grid):
    """The rows with a row that sees every tap moved to the front (so every count covers it)."""
    taps = (R.sp_neighbour_table(out, ksp, DIMS, grid) >= 0).sum(1)
    assert taps.max() == ksp[0] * ksp[1] * ksp[2] and taps.min() == 1
    order = np.arange(len(out))
    order[[0, int(taps.argmax())]] = order[[int(taps.argmax()), 0]]
    return out[order]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("kind", list(KSP))
def test_rulebook_matches_reference(cuda, kind, n):
    ksp = KSP[kind]
    _, grid, out = _rulebook_level(kind)
    out = _full_row_first(out, ksp, grid)
    assert len(out) >= 300
    cap = min(len(out), n + 100)  # rows in [n, cap) hold valid coordinates, and stay unwritten
    nbr, mask = _rulebook(cuda, out[:cap], n, cap, ksp, DIMS, grid)
    _check_rulebook(nbr, mask, n, R.sp_neighbour_table(out[:n], ksp, DIMS, grid))


@pytest.mark.gpu
def test_rulebook_count_above_capacity_uses_cap_rows(cuda):
    ksp = KSP["s2_p011"]
    _, grid, out = _rulebook_level("s2_p011")
    cap = 130
    nbr, mask = _rulebook(cuda, out[:cap], cap + 100, cap, ksp, DIMS, grid)
    _check_rulebook(nbr, mask, cap, R.sp_neighbour_table(out[:cap], ksp, DIMS, grid))


# ------------------------------------------------------------------------------------ gather GEMM
GEMM_SHAPES = [(8, 16, 27), (16, 16, 27), (16, 32, 27), (32, 32, 27), (32, 64, 27), (64, 64, 27), (64, 128, 3),
               (8, 8, 27), (16, 24, 27), (32, 48, 27)]  # the last three: accepted by the contract, sent by no model
N_IN = 150


def _gemm_table(rng, kt, rows_total):
    """Neighbour rows by tile: taps present at p = 0.5 / centre tap only / none / last tap only."""
    nbr = rng.integers(0, N_IN, (rows_total, kt)).astype(np.int32)
    for t in range((rows_total + 63) // 64):
        blk = nbr[t * 64:(t + 1) * 64]
        keep = np.zeros(blk.shape, bool)
        if t % 4 == 0:
            keep = rng.random(blk.shape) < 0.5
        elif t % 4 == 1:
            keep[:, kt // 2] = True
        elif t % 4 == 3:
            keep[:, kt - 1] = True
        blk[~keep] = -1
    return nbr


def _coherent(rng, shape):
    """Positive fp32 values x = hi (1 + e), hi a bf16 number in [0.5, 2), e in 2^-9 [0.5, 0.9]:
    full fp32 mantissas, bf16(x) == hi, and a lo part of one sign and 1e-3 relative size, so
    a dropped hi*lo product shifts every sum the same way instead of averaging out."""
    hi = _bf16(0.5 + 1.5 * rng.random(shape)).float().numpy()
    x = (hi.astype(np.float64) * (1.0 + 2.0 ** -9 * (0.5 + 0.4 * rng.random(shape)))).astype(np.float32)
    assert np.array_equal(_bf16(x).float().numpy(), hi)
    return x


def _gemm_data(rng, cin, cout, kt, x3):
    if x3:
        a = _coherent(rng, (N_IN, cin))
        w = _coherent(rng, (cout, kt, cin)) * np.float32(0.125) * rng.choice([-1.0, 1.0], (cout, 1, 1)).astype(np.float32)
        bias = (rng.standard_normal(cout) * 0.05).astype(np.float32)
    else:
        a = _bf16(rng.standard_normal((N_IN, cin))).float().numpy()
        w = _bf16(rng.standard_normal((cout, kt, cin)) * 0.2).float().numpy()
        bias = rng.standard_normal(cout).astype(np.float32)
    return a, w, bias


def _gemm_weights(dev, w, kp, x3):
    from triton_client_amd.ops.conv import split_pairs
    cout, kt, cin = w.shape
    W = torch.zeros(cout, kp)
    W[:, :kt * cin] = torch.from_numpy(w).reshape(cout, -1)
    return split_pairs(W).to(dev) if x3 else W.to(dev, torch.bfloat16).contiguous()


def _gemm_tol(ref, S, kp, x3):
    if x3:
        return (2.0 ** -16 + 2 * kp * 2.0 ** -24) * S
    return 2.0 ** -8 * np.abs(ref) + 2 * kp * 2.0 ** -24 * S


def _gemm_launch(dev, x3, a_d, cin, nbr, masks, w_d, b_d, cout, kt, kp, count, cap, act, out=None, coords=None,
                 bev=None, bev_hwc=(0, 0, 0)):
    nd = _dev(R.sp_pack_nbr(nbr), dev)
    md = _dev(masks.view(np.int32), dev)
    cd = _dev(np.array([count], np.int32), dev)
    co = _dev(coords, dev) if coords is not None else None
    _call("tca_sp_gemm_x3" if x3 else "tca_sp_gemm", a_d.data_ptr(), cin, nd.data_ptr(), kt, md.data_ptr(),
          w_d.data_ptr(), b_d.data_ptr(), cout, kp, cd.data_ptr(), cap, out.ptr if out is not None else 0,
          co.data_ptr() if co is not None else 0, bev.ptr if bev is not None else 0, *bev_hwc, act)
    torch.cuda.synchronize()


def _masks_for(nbr, live_rows):
    """Tap masks as the rulebook writes them: OR over the live rows; later tiles' words are stale (all ones here)."""
    m = np.full(((len(nbr) + 63) // 64,), 0xFFFFFFFF, np.uint32)
    if live_rows:
        lm = R.sp_tap_masks(nbr[:live_rows])
        m[:len(lm)] = lm
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=lambda s: "%dx%dk%d" % s)
def test_gather_gemm_rows(cuda, shape, x3):
    cin, cout, kt = shape
    kp = (kt * cin + 31) // 32 * 32
    rng = np.random.default_rng(cin * 1000 + cout)
    a, w, bias = _gemm_data(rng, cin, cout, kt, x3)
    a_d = _dev(a, cuda) if x3 else _dev(a, cuda).to(torch.bfloat16)
    w_d, b_d = _gemm_weights(cuda, w, kp, x3), _dev(bias, cuda)
    kind = "f32" if x3 else "bf16"
    worst = 0.0
    for M, cap, count in [(0, 70, 0), (1, 71, 1), (64, 134, 64), (65, 135, 65), (200, 270, 200), (130, 130, 230)]:
        nbr = _gemm_table(rng, kt, (cap + 63) // 64 * 64)  # rows >= M hold valid entries too
        masks = _masks_for(nbr, M)
        for act in (0, 1):
            out = Buf(cuda, cap * cout, kind)
            _gemm_launch(cuda, x3, a_d, cin, nbr, masks, w_d, b_d, cout, kt, kp, count, cap, act, out=out)
            got, untouched = out.split()
            got, untouched = got.reshape(cap, cout), untouched.reshape(cap, cout)
            assert untouched[M:].all() and not untouched[:M].any(), (M, act)
            if M == 0:
                continue
            ref, S = R.sp_gather_gemm_ref(a, nbr[:M], w, bias, act)
            tol = _gemm_tol(ref, S, kp, x3)
            err = np.abs(got[:M] - ref)
            worst = max(worst, float((err / tol).max()))
            assert (err <= tol).all(), (M, act, float((err / tol).max()), np.argwhere(err > tol)[:4])
            if M >= 200:  # the all -1 tile: no K step runs, the output is act(bias)
                assert (nbr[128:192] < 0).all()
                b = bias if x3 else _bf16(bias).float().numpy()
                assert np.array_equal(got[128:192], np.broadcast_to(np.maximum(b, 0) if act else b, (64, cout)))
            if x3 and M == 200 and act == 0:
                # the tolerance is not vacuous: either cross term missing breaks it on this data
                from triton_client_amd.ops.conv import split_bf16
                ah, al = (t.float().numpy() for t in split_bf16(torch.from_numpy(a)))
                wh, wl = (t.float().numpy().reshape(w.shape) for t in split_bf16(torch.from_numpy(w).reshape(cout, -1)))
                zero = np.zeros_like(bias)
                hh = R.sp_gather_gemm_ref(ah, nbr[:M], wh, bias, 0)[0]
                hl = R.sp_gather_gemm_ref(ah, nbr[:M], wl, zero, 0)[0]
                lh = R.sp_gather_gemm_ref(al, nbr[:M], wh, zero, 0)[0]
                assert (np.abs(hh + hl + lh - ref) <= tol).all()  # all three products: inside
                for name, part in (("a_lo*w_hi", hh + hl), ("a_hi*w_lo", hh + lh)):
                    frac = float((np.abs(part - ref) > tol).mean())
                    print(shape, "without", name, ": outside the tolerance in", frac)
                    assert frac > 0.5, (name, frac)
    print(shape, "x3" if x3 else "bf16", "worst err / tol", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
@pytest.mark.parametrize("shape", [(64, 128, 3), (16, 16, 27)], ids=lambda s: "%dx%dk%d" % s)
def test_gather_gemm_bev_scatter(cuda, shape, x3):
    cin, cout, kt = shape
    kp = (kt * cin + 31) // 32 * 32
    B, D, H, W = 2, 2, 5, 6
    C = D * cout
    M, cap = 100, 110
    rng = np.random.default_rng(7 + cin)
    a, w, bias = _gemm_data(rng, cin, cout, kt, x3)
    a_d = _dev(a, cuda) if x3 else _dev(a, cuda).to(torch.bfloat16)
    w_d, b_d = _gemm_weights(cuda, w, kp, x3), _dev(bias, cuda)
    cells = np.argwhere(np.ones((B, D, H, W), bool)).astype(np.int32)  # (b, z, y, x): unique
    coords = cells[rng.permutation(len(cells))][:cap]
    nbr = _gemm_table(rng, kt, 128)
    masks = _masks_for(nbr, M)
    for act in (0, 1):
        bev = Buf(cuda, B * H * W * C, "f32" if x3 else "bf16")
        _gemm_launch(cuda, x3, a_d, cin, nbr, masks, w_d, b_d, cout, kt, kp, M, cap, act, coords=coords, bev=bev,
                     bev_hwc=(H, W, C))
        got, untouched = bev.split()
        got, untouched = got.reshape(B, H, W, D, cout), untouched.reshape(B, H, W, D, cout)
        ref, S = R.sp_gather_gemm_ref(a, nbr[:M], w, bias, act)
        tol = _gemm_tol(ref, S, kp, x3)
        c = coords[:M].astype(np.int64)
        at = (c[:, 0], c[:, 2], c[:, 3], c[:, 1])  # map [b, y, x, z * N + n]
        assert not untouched[at].any()
        err = np.abs(got[at] - ref)
        print(shape, "x3" if x3 else "bf16", "act", act, "bev worst err / tol", float((err / tol).max()))
        assert (err <= tol).all()
        written = np.zeros((B, H, W, D), bool)
        written[at] = True
        assert untouched[~written].all()  # the cells of rows >= M included


# ------------------------------------------------------------------------------- level-0 encoders
def _vfe_check(feats, ref, mag, rows, P, bf16):
    got, untouched = feats.split()
    got, untouched = got.reshape(-1, 8), untouched.reshape(-1, 8)
    assert untouched[rows:].all() and not untouched[:rows].any()
    assert (feats.bits().reshape(-1, 8)[:rows, 4:] == 0).all()  # channels 4..7: exactly +0
    tol = (P + 1) * 2.0 ** -24 * mag
    if bf16:
        tol = tol + 2.0 ** -8 * np.abs(ref)
    err = np.abs(got[:rows, :4] - ref)
    print("vfe", "bf16" if bf16 else "fp32", "rows", rows, "worst err / tol",
          float((err / np.maximum(tol, 1e-300)).max()))
    assert (err <= tol).all()


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("F", [4, 5])
@pytest.mark.parametrize("V", [1, 256, 257])
def test_vfe_from_voxels(cuda, V, F, bf16):
    P, cap = 5, V + 30
    rng = np.random.default_rng(V * 10 + F)
    sites = np.argwhere(np.ones((2, *DIMS), bool)).astype(np.int32)
    coords = sites[rng.permutation(len(sites))][:cap]
    num = rng.integers(0, P + 1, cap).astype(np.int32)
    num[0] = P if V == 1 else 0
    num[V - 1] = P
    vox = (rng.standard_normal((cap, P, F)) * 3).astype(np.float32)
    vox[np.arange(P)[None, :] >= num[:, None]] = 0  # the padding slots are zero
    feats = Buf(cuda, cap * 8, "bf16" if bf16 else "f32")
    co = Buf(cuda, cap * 4, "i32")
    grid = Buf(cuda, 2 * DIMS[0] * DIMS[1] * DIMS[2], "i32", fill=-1)
    vd, nd, cd, cnt = _dev(vox, cuda), _dev(num, cuda), _dev(coords, cuda), _dev(np.array([V], np.int32), cuda)
    _call("tca_sp_vfe_voxels" if bf16 else "tca_sp_vfe_voxels_f32", vd.data_ptr(), cap, P, F, nd.data_ptr(),
          cd.data_ptr(), cnt.data_ptr(), _iarr(DIMS), feats.ptr, co.ptr, grid.ptr)
    torch.cuda.synchronize()
    ref, mag = R.mean_vfe_voxels_ref(vox[:V], num[:V])
    _vfe_check(feats, ref, mag, V, P, bf16)
    cb = co.bits().reshape(cap, 4)
    assert np.array_equal(cb[:V], coords[:V]) and (cb[V:] == I32_SENT).all()
    assert np.array_equal(grid.bits().reshape(2, *DIMS), R.sp_grid(coords[:V], 2, DIMS))


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("pstride", [4, 8])
def test_vfe_from_slots(cuda, pstride, bf16):
    """tca_sp_offsets + tca_sp_vfe_slots[_f32]: three frames, the middle one empty."""
    B, P, max_vox, max_pts = 3, 5, 320, 400
    counts = np.array([5, 0, 300], np.int32)
    total = int(counts.sum())
    rng = np.random.default_rng(40 + pstride)
    pts = (rng.standard_normal((B, max_pts, pstride)) * 3).astype(np.float32)
    pts[:, max_pts - 1] = 1e30  # the point unused slot entries name: reading one shows
    vcount = rng.integers(1, 9, (B, max_vox)).astype(np.int32)  # up to 8 > P: the min() clamp runs
    vcount[2, 0], vcount[2, 1] = 8, 1
    slots = np.full((B, max_vox, P), max_pts - 1, np.int32)
    fill = np.arange(P)[None, None, :] < np.minimum(vcount, P)[..., None]
    slots[fill] = rng.integers(0, max_pts - 1, int(fill.sum()))
    sites = np.argwhere(np.ones(DIMS, bool)).astype(np.int32)
    vco = np.zeros((B, max_vox, 4), np.int32)
    for b in range(B):  # entries past a frame's count name free sites: using one shows in the grid
        vco[b, :, 0] = b
        vco[b, :, 1:] = sites[rng.permutation(len(sites))][:max_vox]
    cap0 = total + 20
    feats = Buf(cuda, cap0 * 8, "bf16" if bf16 else "f32")
    co = Buf(cuda, cap0 * 4, "i32")
    grid = Buf(cuda, B * DIMS[0] * DIMS[1] * DIMS[2], "i32", fill=-1)
    off, tot = Buf(cuda, B, "i32"), Buf(cuda, 1, "i32")
    pd, sd, vd, cd, nd = (_dev(x, cuda) for x in (pts, slots, vcount, vco, counts))
    _call("tca_sp_offsets", nd.data_ptr(), B, off.ptr, tot.ptr)
    _call("tca_sp_vfe_slots" if bf16 else "tca_sp_vfe_slots_f32", pd.data_ptr(), pstride, max_pts, sd.data_ptr(),
          vd.data_ptr(), P, cd.data_ptr(), nd.data_ptr(), B, max_vox, off.ptr, _iarr(DIMS), feats.ptr, co.ptr, grid.ptr)
    torch.cuda.synchronize()
    assert off.bits().tolist() == [0, 5, 5] and int(tot.bits()[0]) == 305
    refs = [R.mean_vfe_slots_ref(pts[b], slots[b, :counts[b]], vcount[b, :counts[b]], P) for b in range(B)]
    ref, mag = np.concatenate([r[0] for r in refs]), np.concatenate([r[1] for r in refs])
    rows = np.concatenate([vco[b, :counts[b]] for b in range(B)])
    _vfe_check(feats, ref, mag, total, P, bf16)
    cb = co.bits().reshape(cap0, 4)
    assert np.array_equal(cb[:total], rows) and (cb[total:] == I32_SENT).all()
    assert np.array_equal(grid.bits().reshape(B, *DIMS), R.sp_grid(rows, B, DIMS))


# ------------------------------------------------------------------------- frame-to-frame state
def _tiny_cfg():
    v = dataclasses.replace(KITTI_SECOND_VOXELS, point_cloud_range=(0.0, -3.2, -3.0, 6.4, 3.2, 1.0), max_voxels=4000)
    return SecondIoUConfig(voxel=v)


@functools.lru_cache(maxsize=None)
def _tiny_model():
    from triton_client_amd.models.common import fuse_model, randomize_bn
    from triton_client_amd.models.second import build_second_iou
    m = build_second_iou(_tiny_cfg(), 0)
    randomize_bn(m, 3)
    for layer in m.backbone3d.layers:
        c = layer.spec.cout
        with torch.no_grad():
            layer.bn.running_mean.copy_(torch.randn(c) * 0.1)
            layer.bn.running_var.copy_(torch.rand(c) * 0.5 + 0.75)
    return fuse_model(m.eval())


def _frame(rng, dims, n, x_lo, x_hi, corners, dev):
    Z, Y, X = dims
    pick = np.zeros((2, Z, Y, X), bool)
    region = np.zeros_like(pick)
    region[..., x_lo:x_hi] = True
    pick.reshape(-1)[rng.choice(np.flatnonzero(region), n, replace=False)] = True
    if corners:
        pick[:, ::Z - 1, ::Y - 1, ::X - 1] = True
    coords = np.argwhere(pick).astype(np.int32)
    coords = coords[rng.permutation(len(coords))]
    V, P = len(coords), 5
    num = rng.integers(1, P + 1, V).astype(np.int32)
    vox = rng.standard_normal((V, P, 4)).astype(np.float32)
    vox[np.arange(P)[None, :] >= num[:, None]] = 0
    return tuple(_dev(x, dev) for x in (vox, num, coords, np.array([V], np.int32)))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_backbone_reset_leaves_no_state(cuda, precision):
    """Frame A, reset, frame B == a fresh backbone on frame B, bit for bit; a last reset
    leaves every grid at -1, the BEV map at zero and the counts at zero."""
    from triton_client_amd.ops.spconv import SparseBackbone
    cfg = _tiny_cfg()
    assert cfg.level_shapes()[0] == (41, 128, 128) and cfg.bev_shape[1:] == (16, 16)
    layers = list(_tiny_model().float().backbone3d.layers)  # CPU modules: the backbone uploads its own copies
    rng = np.random.default_rng(50)
    dims = cfg.level_shapes()[0]
    fa = _frame(rng, dims, 3000, 0, 96, False, cuda)
    fb = _frame(rng, dims, 700, 80, 128, True, cuda)
    used = SparseBackbone(cfg, layers, 2, cuda, precision=precision)
    fresh = SparseBackbone(cfg, layers, 2, cuda, precision=precision)
    used.encode_from_voxels(*fa)
    bev_a = used.forward().clone()
    used.reset()
    used.encode_from_voxels(*fb)
    used.forward()
    fresh.encode_from_voxels(*fb)
    fresh.forward()
    torch.cuda.synchronize()
    assert (bev_a != 0).any() and (fresh.bev != 0).any() and not torch.equal(bev_a, fresh.bev)
    assert torch.equal(used.bev, fresh.bev)
    rows = fresh.level_rows()
    assert used.level_rows() == rows and rows[0] == int(fb[3]) and all(r > 0 for r in rows)
    for lu, lf in zip(used.levels, fresh.levels):
        assert torch.equal(lu.grid >= 0, lf.grid >= 0)
        assert int((lf.grid >= 0).sum()) == rows[lf.count_idx]
    used.reset()
    torch.cuda.synchronize()
    assert all(bool((lev.grid == -1).all()) for lev in used.levels)
    assert not used.bev.view(torch.int32 if precision == "fp32" else torch.int16).any()
    assert used.level_rows() == [0] * len(rows)


@pytest.mark.gpu
def test_backbone_from_voxelizer_slots_fp32_vs_fp64(cuda):
    """The pipeline's level-0 path (Voxelizer.assign → encode_from_slots → finish → forward)
    against the fp64 module on voxelize_np of the same points."""
    from triton_client_amd.models.second import bev_channel_permutation
    from triton_client_amd.ops.lidar import Voxelizer, voxelize_np
    from triton_client_amd.ops.spconv import SparseBackbone
    cfg = _tiny_cfg()
    m = _tiny_model()
    rng = np.random.default_rng(60)
    B, max_pts = 2, 4096
    pts = np.zeros((B, max_pts, 4), np.float32)
    npts = np.array([3000, 2200], np.int32)
    vs, cs, ns = [], [], []
    for b in range(B):
        centres = rng.random((npts[b] // 4, 3)) * [6.4, 6.4, 4.0] + [0.0, -3.2, -3.0]
        p = np.repeat(centres, 4, 0) + rng.standard_normal((npts[b], 3)) * 0.03  # several points per voxel
        pts[b, :npts[b], :3] = p
        pts[b, :npts[b], 3] = rng.random(npts[b])
        v, zyx, num, _ = voxelize_np(pts[b, :npts[b]], cfg.voxel, 4)
        vs.append(v)
        ns.append(num)
        cs.append(np.concatenate([np.full((len(zyx), 1), b, np.int32), zyx], 1))
    vox, num, coords = (torch.from_numpy(np.concatenate(x)) for x in (vs, ns, cs))
    with torch.no_grad():
        ref = m.double().sparse_forward(vox.double(), num.long(), coords, B)
    m.float()
    sp = SparseBackbone(cfg, list(m.backbone3d.layers), B, cuda, precision="fp32")
    vz = Voxelizer(cfg.voxel, B, max_pts, device=cuda, materialize=False)
    pd, nd = _dev(pts, cuda), _dev(npts, cuda)
    sp.reset()
    vz.assign(pd, nd)
    sp.encode_from_slots(pd, vz)
    vz.finish(pd, nd, gather=False)
    bev = sp.forward()
    torch.cuda.synchronize()
    assert sp.level_rows()[0] == len(vox)
    perm = bev_channel_permutation(cfg)
    got = bev.cpu()[..., torch.argsort(perm)].permute(0, 3, 1, 2).double()
    err = ((got - ref).norm() / ref.norm()).item()
    print("slots path fp32 rel L2", err, "voxels", len(vox))
    assert err < 2e-4, err
    assert torch.equal(got.abs().sum(1) > 0, ref.abs().sum(1) > 0)


# -------------------------------------------------------------------------------------- RoI stage
@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
def test_roi_grid_pool_rect_map_channel_window(cuda, f32):
    """H != W, ldc > C, coff > 0; RoIs partly and wholly off the map."""
    from triton_client_amd.models.second import roi_grid_pool_reference
    cfg = _tiny_cfg()
    torch.manual_seed(2)
    B, H, W, C, R_, G = 2, 24, 40, 32, 60, 7
    ldc, coff = C + 16, 8
    v, ds = cfg.voxel, cfg.feature_map_stride
    x0, y0 = float(v.point_cloud_range[0]), float(v.point_cloud_range[1])
    cx, cy = float(v.voxel_size[0] * ds), float(v.voxel_size[1] * ds)
    feat = torch.full((B, H, W, ldc), 1e4)  # a read outside the channel window shows
    feat[..., coff:coff + C] = torch.randn(B, H, W, C)
    if not f32:
        feat = feat.to(torch.bfloat16)
    rois = torch.zeros(B, R_, 7)
    rois[..., 0] = x0 + (torch.rand(B, R_) * 1.3 - 0.15) * W * cx  # centres up to 15 % outside
    rois[..., 1] = y0 + (torch.rand(B, R_) * 1.3 - 0.15) * H * cy
    rois[..., 3:6] = torch.rand(B, R_, 3) * 4 + 0.5
    rois[..., 6] = (torch.rand(B, R_) - 0.5) * 6.3
    rois[:, :4, 0] = x0 + W * cx + 50.0  # wholly off the map
    rois[:, 4:8, 1] = y0 - 50.0
    count = torch.tensor([R_, 23], dtype=torch.int32)
    out = Buf(cuda, B * R_ * G * G * C, "f32" if f32 else "bf16")
    fg, rg, cc = feat.to(cuda), rois.to(cuda), count.to(cuda)
    _call("tca_roi_grid_pool_f32" if f32 else "tca_roi_grid_pool", fg.data_ptr(), B, H, W, C, ldc, coff,
          rg.data_ptr(), 7, cc.data_ptr(), R_, x0, y0, cx, cy, G, out.ptr)
    torch.cuda.synchronize()
    window = feat[..., coff:coff + C].permute(0, 3, 1, 2)
    ref = roi_grid_pool_reference(window.double() if f32 else window.float(), rois.double() if f32 else rois, cfg)
    vals, untouched = out.split()
    assert not untouched.any()
    got = torch.from_numpy(vals).view(B * R_, G, G, C).permute(0, 3, 1, 2)
    valid = torch.cat([torch.arange(R_) < int(c) for c in count])
    off_map = torch.zeros(B, R_, dtype=torch.bool)
    off_map[:, :8] = True
    off_map = off_map.view(-1) & valid
    assert (ref[off_map] == 0).all() and (got[off_map] == 0).all()
    partly = (ref[valid] == 0).view(int(valid.sum()), -1).any(1) & (ref[valid] != 0).view(int(valid.sum()), -1).any(1)
    assert partly.sum() >= 5  # some RoIs straddle the border
    rel = ((got[valid] - ref[valid].double()).norm() / ref[valid].double().norm()).item()
    print("roi pool", "fp32" if f32 else "bf16", "rel L2", rel)
    assert rel < (1e-5 if f32 else 1e-2)
    assert (got[~valid] == 0).all()


@pytest.mark.gpu
def test_roi_rescore_matches_numpy(cuda):
    B, R_, rdim, thresh = 3, 300, 7, 0.3
    counts = np.array([300, 0, 137], np.int32)
    rng = np.random.default_rng(70)
    edge = math.log(thresh / (1 - thresh))
    logit = (rng.standard_normal((B, R_)) * 2.5).astype(np.float32)
    near = np.abs(logit - edge) < 1e-3
    logit[near] = np.float32(edge + 2e-3)  # every logit at least 1e-3 from the threshold
    rois = rng.standard_normal((B, R_, rdim)).astype(np.float32)
    cls = rng.integers(1, 4, (B, R_)).astype(np.int32)
    box, score, ccls = Buf(cuda, B * R_ * rdim, "f32"), Buf(cuda, B * R_, "f32"), Buf(cuda, B * R_, "i32")
    key, cnt = Buf(cuda, B * R_, "i64"), Buf(cuda, B, "i32")
    ld, rd, cd, nd = (_dev(x, cuda) for x in (logit, rois, cls, counts))
    _call("tca_roi_rescore", ld.data_ptr(), rd.data_ptr(), rdim, cd.data_ptr(), nd.data_ptr(), B, R_, thresh,
          box.ptr, score.ptr, ccls.ptr, key.ptr, cnt.ptr)
    torch.cuda.synchronize()
    sig = 1.0 / (1.0 + np.exp(-logit.astype(np.float64)))
    got_n = cnt.bits()
    bb, sb, cb, kb = (box.bits().reshape(B, R_, rdim), score.bits().reshape(B, R_), ccls.bits().reshape(B, R_),
                      key.bits().reshape(B, R_))
    for b in range(B):
        keep = np.flatnonzero((np.arange(R_) < counts[b]) & (sig[b] >= thresh))  # RoI order
        n = len(keep)
        assert got_n[b] == n
        if counts[b] == 300:
            assert (keep < 256).sum() > 20 and (keep >= 256).sum() > 5  # the base carries across chunks
        assert np.array_equal(bb[b, :n], rois[b, keep].view(np.int32))
        assert np.array_equal(cb[b, :n], cls[b, keep])
        # sigmoidf_ = 1 / (1 + __expf(-x)); __expf is v_exp_f32(x * log2 e).  v_exp_f32 is accurate
        # to 1 ulp (CDNA ISA guide); the fp32 product with the rounded constant moves the exponent
        # by at most 2 * 2^-24 |x log2 e|, i.e. the result by ln 2 times that = 2^-23 |x| relative.
        # So exp carries (1 + |x|) 2^-23; d sigma / sigma = -(e / (1 + e)) d e / e is no larger;
        # the add and the divide round once each (2^-24 each; 2.5 ulp allowed for the divide).
        x = np.abs(logit[b, keep].astype(np.float64))
        s = sb[b, :n].view(np.float32).astype(np.float64)
        tol = 2.0 ** -23 * (4.0 + x) * sig[b, keep]
        err = np.abs(s - sig[b, keep])
        if n:
            print("rescore frame", b, "kept", n, "worst err / tol", float((err / tol).max()))
        assert (err <= tol).all()
        # make_score_key: ordered score bits in the high word, ~RoI index in the low word
        u = sb[b, :n].view(np.uint32).astype(np.uint64)
        ordered = np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
        want = (ordered << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - keep.astype(np.uint64))
        assert np.array_equal(kb[b, :n].view(np.uint64), want)
        assert (bb[b, n:] == F32_NAN).all() and (sb[b, n:] == F32_NAN).all()
        assert (cb[b, n:] == I32_SENT).all() and (kb[b, n:] == I32_SENT).all()
