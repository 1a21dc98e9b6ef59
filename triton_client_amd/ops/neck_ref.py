"""CPU references of the fused BEV neck + head kernels (K15, ``csrc/kernels/bev_neck.hip``).

* :func:`neck_head_fp64` — the definition ``head(cat_i relu(deconv_i(x_i)))`` in float64,
  written over the sub-pixel class ``(y mod s, x mod s)`` of a k = s, stride-s transpose conv.
* :func:`neck_head_from_packed` — the same result in float64 from the buffers the kernels are
  handed (:class:`Packed`): deconv rows ``(sy*s + sx)*128 + co``, hi / lo pairs, the 32-chunk
  head permutation, 80 head rows.
* :func:`emulate_fp32` / :func:`emulate_bf16` — the kernels' arithmetic in float32 / bf16.
* :func:`bound_fp32` / :func:`bound_bf16` — element-wise error bounds ``c * u * A`` with
  ``A = |bh| + sum |wh| (|bd| + sum |wd| |x|)`` (derivation: ``docs/precision.md``), and
  :func:`compare`, the comparator of ``tests/test_neck_kernels_gpu.py``.
* :data:`GEOMETRIES`, :func:`make_case`, :func:`pack_case` — the inputs both test files share.

Everything here runs on the CPU; nothing goes through ``FusedConv.__call__``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

CB = 128       # output channels of every branch
NH_PAD = 80    # head rows the kernels read
U_FP32 = 2.0 ** -16   # the three-term split product: 2^-8 squared (bf16 keeps 8 significant bits)
U_BF16 = 2.0 ** -24   # fp32 accumulation; the bf16 kernel is compared with its own bf16 emulation
REL_L2_FP32 = 5e-5    # the project's per-conv budget in fp32 mode


# ------------------------------------------------------------------------------ definition
def _wb(m) -> Tuple[torch.Tensor, torch.Tensor]:
    """An ``nn`` module or a ``(weight, bias)`` pair -> float64 tensors."""
    w, b = (m.weight, m.bias) if isinstance(m, nn.Module) else m
    return w.detach().double(), b.detach().double()


def _by_class(x: torch.Tensor, s: int, per_class) -> torch.Tensor:
    """x [B, Hi, Wi, cin] -> [B, Hi*s, Wi*s, co]: output pixels of class (sy, sx) are
    ``per_class(X [Hi*Wi*B, cin], sy, sx)`` of the input pixel (y // s, x // s)."""
    B, Hi, Wi, cin = x.shape
    X = x.reshape(-1, cin)
    y = None
    for sy in range(s):
        for sx in range(s):
            v = per_class(X, sy, sx)
            if y is None:
                y = v.new_empty(B, Hi * s, Wi * s, v.shape[-1])
            y[:, sy::s, sx::s] = v.reshape(B, Hi, Wi, -1)
    return y


def neck_head_fp64(xs: Sequence[torch.Tensor], strides: Sequence[int], deconvs, head) -> torch.Tensor:
    """xs[i] [B, H/s_i, W/s_i, cin_i] (NHWC values); deconvs[i] a ``ConvTranspose2d(cin_i, 128, s_i,
    s_i)`` or its ``(weight [cin, 128, s, s], bias [128])``; head a 1x1 ``Conv2d`` or ``(weight
    [nh, 128 * nbr(, 1, 1)], bias [nh])``.  Returns [B, H, W, nh] float64."""
    ys = []
    for x, s, d in zip(xs, strides, deconvs):
        w, b = _wb(d)
        assert w.shape[2] == w.shape[3] == s, (w.shape, s)
        ys.append(_by_class(x.double(), s,
                            lambda X, sy, sx: torch.relu(torch.einsum("pc,co->po", X, w[:, :, sy, sx]) + b)))
    wh, bh = _wb(head)
    return torch.einsum("bhwk,nk->bhwn", torch.cat(ys, -1), wh.reshape(wh.shape[0], -1)) + bh


# ------------------------------------------------------------------------------ packed form
def _perm32() -> List[int]:
    """Position 8g + e of a 32-channel chunk holds channel 4g + e (e < 4) or 16 + 4g + e - 4: lane
    group g of the MFMA D layout owns channels 4g .. 4g+3 of two neighbouring 16-channel tiles."""
    return [4 * g + e if e < 4 else 16 + 4 * g + e - 4 for g in range(4) for e in range(8)]


@dataclass
class Packed:
    """The weight buffers one launch is handed (any device).  kind "fp32": w[i] [s*s*128, 2*cin]
    bf16 ({hi 8 | lo 8} per 8 columns), wh [80, 2*128*nbr] bf16; kind "bf16": w[i] [s*s*128, cin],
    wh [80, 128*nbr] bf16.  b[i] [s*s*128] and bh [80] fp32.  wh columns are 32-chunk permuted."""
    kind: str
    strides: List[int]
    cins: List[int]
    w: List[torch.Tensor]
    b: List[torch.Tensor]
    wh: torch.Tensor
    bh: torch.Tensor
    nh: int

    def cpu(self) -> "Packed":
        return Packed(self.kind, self.strides, self.cins, [t.cpu() for t in self.w], [t.cpu() for t in self.b],
                      self.wh.cpu(), self.bh.cpu(), self.nh)


def _halves(t: torch.Tensor, kind: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """A packed weight matrix -> (hi, lo) [N, K] float32 holding bf16 values (lo = 0 for bf16)."""
    assert t.dtype == torch.bfloat16
    if kind == "bf16":
        return t.float(), torch.zeros(t.shape, dtype=torch.float32)
    N, K2 = t.shape
    v = t.float().reshape(N, K2 // 16, 2, 8)
    return v[:, :, 0].reshape(N, K2 // 2).contiguous(), v[:, :, 1].reshape(N, K2 // 2).contiguous()


def _unpermute(wp: torch.Tensor) -> torch.Tensor:
    """Head columns in the kernel's order -> channel order."""
    K = wp.shape[1]
    idx = torch.tensor([c * 32 + p for c in range(K // 32) for p in _perm32()])
    out = torch.empty_like(wp)
    out[:, idx] = wp
    return out


def unpack(p: Packed):
    """-> deconv (hi, lo) [s*s*128, cin] per branch and head (hi, lo) [80, 128*nbr] in channel
    order, float32 holding bf16 values."""
    p = p.cpu()
    dec = []
    for w, s, cin in zip(p.w, p.strides, p.cins):
        hi, lo = _halves(w, p.kind)
        assert hi.shape == (s * s * CB, cin), (hi.shape, s, cin)
        dec.append((hi, lo))
    hh, hl = _halves(p.wh, p.kind)
    assert hh.shape == (NH_PAD, CB * len(p.strides)), hh.shape
    return dec, (_unpermute(hh), _unpermute(hl))


def neck_head_from_packed(xs: Sequence[torch.Tensor], p: Packed) -> torch.Tensor:
    """The result in float64 from the packed buffers: weights hi + lo, rows (sy*s + sx)*128 + co."""
    p = p.cpu()
    dec, (hh, hl) = unpack(p)
    ys = []
    for x, s, (hi, lo), b in zip(xs, p.strides, dec, p.b):
        w, b = hi.double() + lo.double(), b.double()

        def cls(X, sy, sx, w=w, b=b, s=s):
            r = (sy * s + sx) * CB
            return torch.relu(X @ w[r:r + CB].t() + b[r:r + CB])
        ys.append(_by_class(x.double(), s, cls))
    wh = (hh.double() + hl.double())[:p.nh]
    return torch.cat(ys, -1) @ wh.t() + p.bh.double()[:p.nh]


# ------------------------------------------------------------------------------ emulations
def bf16r(t: torch.Tensor) -> torch.Tensor:
    """float32 -> the nearest bf16 (ties to even), as float32."""
    return t.float().to(torch.bfloat16).float()


def split(t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """hi = bf16(t), lo = bf16(t - hi), both as float32 (tca_mfma.h split8)."""
    t = t.float()
    hi = bf16r(t)
    return hi, bf16r(t - hi)


def _mfma3(acc, ah, al, wh, wl, drop_lohi):
    """acc [P, N] += a [P, K] * w [N, K] in 32-deep steps of three fp32-accumulated products, in
    mfma3's order: a_hi w_lo, a_lo w_hi, a_hi w_hi.  drop_lohi leaves a_lo w_hi out (a defect)."""
    for k in range(0, ah.shape[1], 32):
        j = slice(k, k + 32)
        acc = acc + ah[:, j] @ wl[:, j].t()
        if not drop_lohi:
            acc = acc + al[:, j] @ wh[:, j].t()
        acc = acc + ah[:, j] @ wh[:, j].t()
    return acc


def emulate_fp32(xs: Sequence[torch.Tensor], p: Packed, drop_lohi: bool = False) -> torch.Tensor:
    """The fp32 kernel in float32: operands split into bf16 hi + lo, three products per pair, fp32
    accumulation starting at the deconv bias; the ReLU'd branch result is split again for the head
    GEMM, whose bias is added last.  xs are the fp32 values (pair storage holds the same split)."""
    assert p.kind == "fp32"
    p = p.cpu()
    dec, (hh, hl) = unpack(p)
    acc2 = None
    for i, (x, s, (wh, wl), b) in enumerate(zip(xs, p.strides, dec, p.b)):
        xh, xl = split(x.reshape(-1, x.shape[-1]))

        def cls(X, sy, sx, xh=xh, xl=xl, wh=wh, wl=wl, b=b, s=s):
            r = slice((sy * s + sx) * CB, (sy * s + sx + 1) * CB)
            acc = b[r].float().expand(xh.shape[0], CB)
            return torch.relu(_mfma3(acc, xh, xl, wh[r], wl[r], drop_lohi))
        y = _by_class(x.float(), s, cls)
        yh, yl = split(y.reshape(-1, CB))
        if acc2 is None:
            acc2 = torch.zeros(yh.shape[0], NH_PAD)
            shape = y.shape[:3]
        k = slice(i * CB, (i + 1) * CB)
        acc2 = _mfma3(acc2, yh, yl, hh[:, k], hl[:, k], drop_lohi)
    return (acc2 + p.bh.float())[:, :p.nh].reshape(*shape, p.nh)


def emulate_bf16(xs: Sequence[torch.Tensor], p: Packed, exact_acc: bool = False):
    """The bf16 kernel: bf16 inputs and weights, fp32 accumulation, bias and ReLU in fp32, the
    result rounded to bf16 (pack8) for the head GEMM, head bias in fp32.  Returns (e, parts): e the
    fp32 value the kernel rounds to bf16 on store, parts the per-branch fp32 values before the ReLU.
    exact_acc accumulates in float64 and rounds once (another legal accumulation order's limit)."""
    assert p.kind == "bf16"
    p = p.cpu()
    dec, (hh, _) = unpack(p)
    at = torch.float64 if exact_acc else torch.float32

    def gemm(acc, a, w):
        for k in range(0, a.shape[1], 32):
            acc = acc + a[:, k:k + 32].to(at) @ w[:, k:k + 32].to(at).t()
        return acc

    acc2, parts = None, []
    for i, (x, s, (w, _), b) in enumerate(zip(xs, p.strides, dec, p.b)):
        assert torch.equal(bf16r(x), x.float()), "bf16 kernel inputs are bf16 values"

        def cls(X, sy, sx, w=w, b=b, s=s):
            r = slice((sy * s + sx) * CB, (sy * s + sx + 1) * CB)
            acc = gemm(torch.zeros(X.shape[0], CB, dtype=at), X, w[r])
            return acc.float() + b[r].float()
        t = _by_class(x.float(), s, cls)
        parts.append(t)
        z = torch.relu(t)
        if acc2 is None:
            acc2 = torch.zeros(z.numel() // CB, NH_PAD, dtype=at)
        acc2 = gemm(acc2, bf16r(z).reshape(-1, CB), hh[:, i * CB:(i + 1) * CB])
    e = (acc2.float() + p.bh.float())[:, :p.nh].reshape(*parts[0].shape[:3], p.nh)
    return e, parts


# ------------------------------------------------------------------------------ bounds
def magnitude(xs: Sequence[torch.Tensor], p: Packed):
    """A = |bh| + sum |wh| (|bd| + sum |wd| |x|) per output element [B, H, W, nh] in float64, and
    the per-branch inner factors A1 [B, H, W, 128]."""
    p = p.cpu()
    dec, (hh, hl) = unpack(p)
    a1 = []
    for x, s, (hi, lo), b in zip(xs, p.strides, dec, p.b):
        w, b = (hi.double() + lo.double()).abs(), b.double().abs()

        def cls(X, sy, sx, w=w, b=b, s=s):
            r = (sy * s + sx) * CB
            return X @ w[r:r + CB].t() + b[r:r + CB]
        a1.append(_by_class(x.double().abs(), s, cls))
    wh = (hh.double() + hl.double()).abs()[:p.nh]
    return torch.cat(a1, -1) @ wh.t() + p.bh.double().abs()[:p.nh], a1


def c_fp32(cins: Sequence[int]) -> float:
    """The constant of the fp32 kernel's bound, in units of u = 2^-16 (docs/precision.md): 3 per
    GEMM for the split product, and 2^-24 per fp32 addition over n1 = 3 cin + 1 and n2 = 3 * 128 *
    nbr + 1 additions, with 2^-6 of slack for the second-order terms."""
    n1, n2 = 3 * max(cins) + 1, 3 * CB * len(cins) + 1
    return (6 + (n1 + n2) / 256) * (1 + 2.0 ** -6)


def bound_fp32(xs: Sequence[torch.Tensor], p: Packed) -> torch.Tensor:
    """|kernel - fp64| <= c u A per element."""
    return c_fp32(p.cins) * U_FP32 * magnitude(xs, p)[0]


def c_bf16(nbr: int) -> float:
    """fp32 accumulation of the head GEMM on both sides, in units of u = 2^-24: two sums of n2 = 128
    nbr products and a bias, each within n2 u of the exact sum."""
    return 2 * (CB * nbr + 1) * (1 + 2.0 ** -6)


def bound_bf16(xs: Sequence[torch.Tensor], p: Packed, e: torch.Tensor, parts) -> torch.Tensor:
    """|kernel (bf16) - e| per element, e / parts from :func:`emulate_bf16`: the store's rounding
    2^-8 |e|, the head's accumulation order c u A, and one bf16 ulp per intermediate whose fp32
    value lies within the deconv's accumulation-order distance (2 cin u A1) of a rounding tie."""
    p = p.cpu()
    A, a1 = magnitude(xs, p)
    _, (hh, _) = unpack(p)
    flips = []
    for t, a, cin in zip(parts, a1, p.cins):
        t = t.double()
        z = torch.relu(t)
        d = 2 * cin * U_BF16 * a * (1 + 2.0 ** -6)
        ulp = 2.0 ** (torch.floor(torch.log2(z.clamp_min(2.0 ** -126))) - 7)
        frac = z / ulp - torch.floor(z / ulp)            # ties of the rounding sit at frac = 1/2
        near = (((frac - 0.5).abs() * ulp <= d) | (d >= ulp / 4)) & (t >= -d)
        flips.append(torch.where(near, 2.0 ** -7 * (z + d) + d, torch.zeros_like(z)))
    flip = torch.cat(flips, -1).reshape(-1, CB * len(parts)) @ hh.double().abs()[:p.nh].t()
    acc = c_bf16(len(parts)) * U_BF16 * A
    return 2.0 ** -8 * e.double().abs() + (1 + 2.0 ** -8) * (acc + flip.reshape(A.shape))


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def compare(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, rel_l2_max: Optional[float] = None) -> dict:
    """The comparator of the kernel tests: every element finite and |got - ref| <= bound, and (fp32
    kernel) relative L2 below rel_l2_max.  Returns ok, which arms failed and the worst figures."""
    got = got.double().cpu()
    finite = torch.isfinite(got)
    err = torch.where(finite, (got - ref).abs(), torch.zeros_like(ref))
    ratio = err / bound
    r = {"nonfinite": int((~finite).sum()), "worst": ratio.max().item(), "outside": int((err > bound).sum()),
         "rel_l2": rel_l2(torch.where(finite, got, ref), ref)}
    r["failed"] = [k for k, bad in (("finite", r["nonfinite"] > 0), ("bound", r["outside"] > 0),
                                    ("rel_l2", rel_l2_max is not None and not r["rel_l2"] < rel_l2_max)) if bad]
    r["ok"] = not r["failed"]
    return r


# ------------------------------------------------------------------------------ shared inputs
@dataclass(frozen=True)
class Geometry:
    """One row of the shape table.  BM = pixels per tile (256; 128 for fp32 variant 2); the fp32
    kernels tile the np = B * (H/S) * (W/S) pixels of a sub-pixel class, the bf16 kernel those of a
    frame.  cins: fp32 kernel (multiples of 32) / bf16 kernel (multiples of 64)."""
    name: str
    strides: Tuple[int, ...]
    B: int
    H: int
    W: int
    cins32: Tuple[int, ...]
    cins16: Tuple[int, ...]
    nh: int
    ldo_pad: int
    grids: Tuple[int, ...]

    def cins(self, kind):
        return self.cins32 if kind == "fp32" else self.cins16


GEOMETRIES = {g.name: g for g in [
    # 4 pixels per class: 16 tiles with 4 valid rows each; grid 256: most workgroups get no tile
    Geometry("nearly_empty", (1, 2, 4), 1, 8, 8, (64, 128, 256), (64, 128, 256), 72, 8, (8, 256)),
    # np = 105: one partial tile that spans three frames
    Geometry("partial_three_frames", (1, 2, 4), 3, 20, 28, (32, 96, 64), (64, 128, 64), 40, 0, (24,)),
    # np = 1026: 5 tiles of 256 (the last holds 2 pixels) / 9 of 128, frame edges inside tiles;
    # grid 8: 10 tiles per workgroup, the ring wraps across tiles
    Geometry("frame_edges", (1, 2, 4), 3, 72, 76, (64, 128, 256), (64, 128, 256), 72, 0, (8, 24)),
    Geometry("exactly_full", (1, 2, 4), 1, 64, 64, (64, 128, 256), (64, 128, 256), 80, 8, (8,)),      # np = 256
    Geometry("one_past_full", (1, 2, 4), 1, 4, 1028, (32, 96, 128), (64, 128, 256), 8, 8, (24,)),     # np = 257
    Geometry("one_branch_odd", (1,), 2, 5, 7, (32,), (64,), 8, 0, (8,)),                               # 1 tile
    Geometry("second_two_branches", (1, 2), 2, 6, 10, (128, 256), (128, 256), 72, 0, (24,)),           # 4 tiles
    Geometry("no_stride_one", (2, 4), 1, 8, 12, (64, 96), (64, 128), 40, 8, (8,)),
    # batch chunking of the fp32 launcher (chunk = 32767 // (H/S) frames per launch, Yg < 32768):
    # two launches of 3 and 2 frames; one launch with B * H = 32767, the largest legal Yg
    Geometry("chunk_two_launches", (1,), 5, 8192, 2, (32,), (), 8, 0, (24,)),
    Geometry("chunk_largest_yg", (1,), 7, 4681, 2, (32,), (), 8, 0, (24,)),
]}
# every (geometry, kind, nh) the GPU tests launch; nh 4 and 36 go to the entry points directly
GPU_SETS = [(g.name, k, None) for g in GEOMETRIES.values() for k in ("fp32", "bf16") if g.cins(k)] + \
           [("one_branch_odd", k, 4) for k in ("fp32", "bf16")] + \
           [("partial_three_frames", k, 36) for k in ("fp32", "bf16")]


@dataclass
class Case:
    geom: Geometry
    kind: str
    nh: int
    xs: List[torch.Tensor]                       # [B, H/s, W/s, cin] fp32 (bf16 values for kind "bf16")
    deconvs: List[Tuple[torch.Tensor, torch.Tensor]]  # ConvTranspose2d weight [cin, 128, s, s], bias [128]
    head: Tuple[torch.Tensor, torch.Tensor]      # [nh, 128 * nbr], [nh]


def make_inputs(strides, cins, B, H, W, nh, kind, seed):
    g = torch.Generator().manual_seed(seed)
    xs, dec = [], []
    for s, cin in zip(strides, cins):
        x = torch.randn(B, H // s, W // s, cin, generator=g)
        flat = x.view(-1)
        flat[3::37] = 0.0     # exact zeros and negative zeros among the inputs
        flat[5::53] = -0.0
        xs.append(bf16r(x) if kind == "bf16" else x)
        # pre-activation std ~0.5 beside a bias of std 0.3: the ReLU cuts about half the channels
        dec.append((torch.randn(cin, CB, s, s, generator=g) * (0.5 / cin ** 0.5), torch.randn(CB, generator=g) * 0.3))
    head = (torch.randn(nh, CB * len(strides), generator=g) * 0.05, torch.randn(nh, generator=g) * 0.1)
    return xs, dec, head


def make_case(name: str, kind: str, nh: Optional[int] = None) -> Case:
    gm = GEOMETRIES[name]
    nh = nh or gm.nh
    seed = sorted(GEOMETRIES).index(name) * 16 + (kind == "bf16") + 2 * (nh != gm.nh)
    xs, dec, head = make_inputs(gm.strides, gm.cins(kind), gm.B, gm.H, gm.W, nh, kind, seed)
    return Case(gm, kind, nh, xs, dec, head)


def modules(case: Case):
    """The case's weights as ``nn`` modules (float32)."""
    dec = []
    for (w, b), s in zip(case.deconvs, case.geom.strides):
        d = nn.ConvTranspose2d(w.shape[0], CB, s, s)
        d.weight.data.copy_(w)
        d.bias.data.copy_(b)
        dec.append(d)
    w, b = case.head
    h = nn.Conv2d(w.shape[1], w.shape[0], 1)
    h.weight.data.copy_(w.reshape(*w.shape, 1, 1))
    h.bias.data.copy_(b)
    return dec, h


def pack_case(case: Case, device="cpu"):
    """The case's weights packed by the project's host code: ``FusedConv`` for each deconv, and for
    the head ``FusedNeckHead`` where the wrapper takes nh (a multiple of 8), else the same packing
    by hand (``permute_head_weight``, ``split_pairs``): the launcher takes any multiple of 4.
    Returns (Packed on ``device``, the FusedNeckHead or None)."""
    from .conv import FusedConv, split_pairs
    from .neck import FusedNeckHead, permute_head_weight

    strides = list(case.geom.strides)
    dec, h = modules(case)
    ups = [FusedConv(d, act=1, device=device, precision=case.kind) for d in dec]
    neck = None
    if case.nh % 8 == 0:
        neck = FusedNeckHead(ups, strides, FusedConv(h, device=device, precision=case.kind), device, grid=8)
        wh, bh = neck.wh, neck.bh
    else:
        wp = permute_head_weight(case.head[0])
        wh = (split_pairs(wp) if case.kind == "fp32" else wp.to(torch.bfloat16)).to(device).contiguous()
        bh = torch.zeros(NH_PAD)
        bh[:case.nh] = case.head[1]
        bh = bh.to(device)
    return Packed(case.kind, strides, [u.Kp for u in ups], [u.w_gemm for u in ups], [u.b_gemm for u in ups],
                  wh, bh, case.nh), neck


def class_pixel(S: int, B: int, H: int, W: int, cls: int, p: int) -> Tuple[int, int, int]:
    """(b, y, x) of pixel p of sub-pixel class cls in the fp32 kernels' flat (frame, pixel) order."""
    Wq, nq = W // S, (H // S) * (W // S)
    b, q = divmod(p, nq)
    return b, (q // Wq) * S + cls // S, (q % Wq) * S + cls % S
