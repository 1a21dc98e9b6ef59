"""Plain NumPy fp64 references of the LiDAR decode kernels: K11 ``tca_anchor_decode_filter``
(+ ``_keyed`` / ``tca_anchor_topk_threshold``, ``csrc/kernels/anchors.hip``) and K12/K13
``tca_centerhead_decode`` (``csrc/kernels/centerpoint.hip``), written from OpenPCDet's
AnchorHeadSingle + ResidualCoder and det3d's CenterHead decode.  No torch, no GPU.

Conventions: every head is a *logical* NHWC array ``[B, H, W, channels]`` of float32 that
already holds the values of its storage type (``round_storage``), so the reference sees what
the kernel sees; scalars the launchers take as C floats are rounded to fp32 here.  The anchor
index is ``aidx = (y*W + x)*A + a``; head channels are cls ``a*C + c``, box ``a*7 + q``, dir
``a*bins + d``; the anchor table is ``[A][6] = (dxa, dya, dza, za, rot, diag)``.

The error bounds (``*_tol``) are the formulas of ``tests/test_decode_kernels_gpu.py``'s
docstring.  The ``make_*`` generators build that file's inputs: every discontinuity of the
decode (score threshold, dir-bin floor, range filter) is kept clear of every input by a band
wider than the fp32 error, so membership is exact; ``*_band_counts`` report what is left
inside each band (the tests assert zero).  ``_mutate`` applies one deliberate defect, for the
tests that prove the bounds discriminate.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Sequence, Tuple

import numpy as np

EPS = 2.0 ** -23          # fp32 ulp of 1
FLOOR_BAND = 1e-3         # dir-bin floor argument: distance from an integer
RANGE_BAND = 1e-3         # metres from a post-centre-range face
ATAN2_TOL = 4 * 2.0 ** -22  # assumed: 4 ulp of pi (fp32 ulp in [2, 4) is 2^-22), absolute
MAX_LOGIT = 12.0


# ------------------------------------------------------------------------------ number formats
def round_storage(a, dtype: str) -> np.ndarray:
    """``a`` rounded (nearest even) to fp32 / fp16 / bf16 storage, returned as float32."""
    a = np.ascontiguousarray(a, np.float32)
    if dtype == "f32":
        return a
    if dtype == "f16":
        return a.astype(np.float16).astype(np.float32)
    if dtype == "bf16":
        u = a.view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000  # finite inputs only
        return u.astype(np.uint32).view(np.float32).reshape(a.shape)
    raise ValueError(dtype)


def ordered_key(x_f32) -> np.ndarray:
    """uint32 order-preserving map of fp32 (``tca_common.h float_to_ordered``): a negative
    float's bits are inverted, a non-negative one's get the sign bit set."""
    u = np.ascontiguousarray(x_f32, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def sigmoid(m):
    return 1.0 / (1.0 + np.exp(-np.asarray(m, np.float64)))


def score_tol(m, s):
    """|fp32 ``1 / (1 + __expf(-m))`` - s| <= 2^-23 (4 + |m|) s (derived at the rescore test
    of tests/test_spconv_kernels_gpu.py)."""
    return EPS * (4.0 + np.abs(m)) * s


def _f32(v) -> float:
    return float(np.float32(v))


# ------------------------------------------------------------------------------------ K11
@dataclasses.dataclass
class AnchorRef:
    logit: np.ndarray  # [B, N] fp64 max class logit (the first maximum's value)
    score: np.ndarray  # [B, N]
    label: np.ndarray  # [B, N] first argmax + 1
    box: np.ndarray    # [B, N, 7]
    u: np.ndarray      # [B, N] val / period + dir_limit_offset (zeros without a dir head)
    tol: np.ndarray    # [B, N, 7] bound on |kernel - box|


def anchor_decode(cls, box, dir, A, C, bins, table, x0, xs, y0, ys, dir_offset, dir_limit_offset,
                  _mutate: str = "") -> AnchorRef:
    cls = np.asarray(cls, np.float32)
    B, H, W = cls.shape[:3]
    N = H * W * A
    cl = cls.reshape(B, N, C)
    lab0 = np.argmax(cl, -1)  # first maximum
    logit = np.take_along_axis(cl, lab0[..., None], -1)[..., 0].astype(np.float64)
    e = np.asarray(box, np.float32).reshape(B, N, 7).astype(np.float64)
    t = np.tile(np.asarray(table, np.float32).reshape(A, 6).astype(np.float64), (H * W, 1))  # [N, 6]
    dxa, dya, dza, za, ra, diag = (t[:, k] for k in range(6))
    if _mutate == "diag_dxa":
        diag = dxa
    pix = np.arange(N) // A
    xa = _f32(x0) + (pix % W) * _f32(xs)
    ya = _f32(y0) + (pix // W) * _f32(ys)
    out = np.empty((B, N, 7))
    tol = np.empty((B, N, 7))
    for q, (s, c) in enumerate(((diag, xa), (diag, ya), (dza, za))):
        out[..., q] = e[..., q] * s + c
        tol[..., q] = EPS * (np.abs(e[..., q] * s) + np.abs(c))
    for q, s in ((3, dxa), (4, dya), (5, dza)):
        out[..., q] = np.exp(e[..., q]) * s
        tol[..., q] = EPS * (4.0 + np.abs(e[..., q])) * np.abs(out[..., q])
    rg = e[..., 6] + ra
    u = np.zeros((B, N))
    if dir is not None and bins > 0:
        d = np.asarray(dir, np.float32).reshape(B, N, bins)
        dl = np.argmax(d, -1).astype(np.float64)
        period = 2.0 * np.pi / bins
        # the kernel's period: its pi literal and the quotient are rounded to fp32
        period32 = float(np.float32(2.0) * np.float32(3.14159265358979) / np.float32(bins))
        do, dlo = _f32(dir_offset), _f32(dir_limit_offset)
        val = rg - do
        u = val / period + dlo
        fl = np.floor(val / period if _mutate == "no_dlo" else u)
        if _mutate == "dir_shift":
            dl = dl + 1.0
        rg = val - fl * period + do + period * dl
        tol[..., 6] = (EPS * (np.abs(e[..., 6]) + np.abs(ra) + abs(do) + period * (np.abs(fl) + dl))
                       + (np.abs(fl) + dl) * abs(period32 - period))
    else:
        tol[..., 6] = EPS * (np.abs(e[..., 6]) + np.abs(ra))
    out[..., 6] = rg
    return AnchorRef(logit, sigmoid(logit), (lab0 + 1).astype(np.int32), out, u, tol)


@dataclasses.dataclass
class AnchorCase:
    dtype: str
    A: int
    C: int
    bins: int
    cls: np.ndarray            # [B, H, W, A*C]
    box: np.ndarray            # [B, H, W, A*7]
    dir: Optional[np.ndarray]  # [B, H, W, A*bins]
    table: np.ndarray          # [A, 6] float32
    geom: Tuple[float, float, float, float]  # x0, xs, y0, ys
    dir_offset: float
    dir_limit_offset: float
    score_thresh: float

    @property
    def shape(self):
        return self.cls.shape[:3]

    def ref(self, use_dir=True, _mutate="") -> AnchorRef:
        return anchor_decode(self.cls, self.box, self.dir if use_dir else None, self.A, self.C, self.bins,
                             self.table, *self.geom, self.dir_offset, self.dir_limit_offset, _mutate=_mutate)


def anchor_table(A: int) -> np.ndarray:
    a = np.arange(A, dtype=np.float64)
    dxa, dya, dza = 1.5 + 0.37 * a, 0.6 + 0.21 * a, 1.4 + 0.11 * a
    return np.stack([dxa, dya, dza, -1.0 + 0.13 * a, (a % 2) * 1.57, np.sqrt(dxa ** 2 + dya ** 2)], 1).astype(np.float32)


def anchor_band_counts(case: AnchorCase, ref: Optional[AnchorRef] = None) -> Tuple[int, int]:
    """(scores within twice the fp32 score bound of the threshold, floor arguments within
    FLOOR_BAND of an integer)."""
    ref = ref or case.ref()
    n_s = int((np.abs(ref.score - _f32(case.score_thresh)) <= 2 * score_tol(ref.logit, ref.score)).sum())
    n_u = int((np.abs(ref.u - np.rint(ref.u)) < FLOOR_BAND).sum()) if case.dir is not None else 0
    return n_s, n_u


def _nudge_anchor(case: AnchorCase) -> None:
    B, H, W = case.shape
    N = H * W * case.A
    for _ in range(8):
        ref = case.ref()
        bad_s = np.abs(ref.score - _f32(case.score_thresh)) <= 2 * score_tol(ref.logit, ref.score)
        bad_u = np.abs(ref.u - np.rint(ref.u)) < FLOOR_BAND
        if not bad_s.any() and not bad_u.any():
            return
        cl = case.cls.reshape(B, N, case.C)
        cl[bad_s] = round_storage(cl[bad_s] - 0.125, case.dtype)  # the whole anchor: the argmax stays
        bx = case.box.reshape(B, N, 7)
        bx[bad_u, 6] = round_storage(bx[bad_u, 6] + 0.0625, case.dtype)


def make_anchor_case(A=6, C=3, bins=2, dtype="f32", seed=0, H=37, W=41, B=3, dense=False,
                     score_thresh=0.3) -> AnchorCase:
    """Sparse random heads (about a quarter of frame 0's and 2's anchors pass, none of frame
    1's), |logit| <= 12, class ties on frame 0; ``dense``: the first 4096 anchors of frame 0
    all pass.  The anchor origin / stride are dyadic, so xa / ya are exact in fp32 and the
    x / y error is the final multiply-add's alone, as the ``e*s + c`` bound assumes."""
    rng = np.random.default_rng(seed)
    N = H * W * A
    cls = rng.normal(-3.0, 1.6, (B, N, C))
    cls[1] = np.minimum(cls[1], -2.0)
    if C > 1:  # two equal maximal logits: the lower class wins
        for i in rng.choice(N, 64, replace=False):
            c1, c2 = sorted(rng.choice(C, 2, replace=False))
            cls[0, i, :] = -4.0
            cls[0, i, c1] = cls[0, i, c2] = 1.0 + 0.01 * (i % 7)
    if dense:
        cls[0, :4096, 0] = rng.uniform(0.5, 6.0, 4096)
    box = rng.normal(0.0, 0.4, (B, N, 7))
    box[..., 6] *= 4.0  # several periods of yaw residual
    case = AnchorCase(
        dtype, A, C, bins,
        round_storage(np.clip(cls, -MAX_LOGIT, MAX_LOGIT), dtype).reshape(B, H, W, A * C),
        round_storage(box, dtype).reshape(B, H, W, A * 7),
        round_storage(rng.normal(0.0, 1.0, (B, N, bins)), dtype).reshape(B, H, W, A * bins) if bins > 0 else None,
        anchor_table(A), (-5.0, 0.25, -9.5, 0.5), 0.78539, 0.5, score_thresh)
    _nudge_anchor(case)
    return case


def make_tie_anchor_case(dtype="f32") -> AnchorCase:
    """Every class logit is exactly 0 on the even anchors of a small grid and -3 on the odd
    ones; with score_thresh exactly 0.5 the even anchors sit on the threshold."""
    H, W, A, C, B = 5, 7, 6, 3, 1
    rng = np.random.default_rng(5)
    N = H * W * A
    cls = np.where((np.arange(N) % 2 == 0)[None, :, None], 0.0, -3.0) * np.ones((B, N, C))
    case = AnchorCase(dtype, A, C, 2, round_storage(cls, dtype).reshape(B, H, W, A * C),
                      round_storage(rng.normal(0, 0.4, (B, H, W, A * 7)), dtype),
                      round_storage(rng.normal(0, 1.0, (B, H, W, A * 2)), dtype),
                      anchor_table(A), (-5.0, 0.25, -9.5, 0.5), 0.78539, 0.5, 0.5)
    for _ in range(8):
        ref = case.ref()
        bad = np.abs(ref.u - np.rint(ref.u)) < FLOOR_BAND
        if not bad.any():
            break
        bx = case.box.reshape(B, N, 7)
        bx[bad, 6] = round_storage(bx[bad, 6] + 0.0625, dtype)
    return case


# ------------------------------------------------------------------------- top-k threshold
TOPK_KINDS = ("spread", "equal", "tie_straddle", "narrow", "signed_zero")


def make_topk_cls(kind: str, dtype="f32", seed=0, H=37, W=41, A=6, C=3, B=2, k=1024) -> np.ndarray:
    """Class head [B, H, W, A*C] for the top-k threshold cases (two frames, different data).

    spread: logits over +-12, mixed sign, with -0.0 / +0.0 sprinkled in.  equal: one value
    everywhere.  tie_straddle: 300 anchors share the value at rank k.  narrow: every logit in
    [2, 2.2), so the top 12 key bits agree.  signed_zero: 100 positive anchors, 50 whose
    maximum is +0.0, 40 whose classes are (-0.0, +0.0, -1) — the first maximum is -0.0, whose
    key is below +0.0's — and the rest negative; k = 170 must reach into the last group."""
    rng = np.random.default_rng(seed)
    N = H * W * A
    if kind == "spread":
        cls = rng.uniform(-MAX_LOGIT, MAX_LOGIT, (B, N, C))
        z = rng.choice(N, 200, replace=False)
        cls[:, z[:100], :] = -0.0
        cls[:, z[100:], :] = 0.0
    elif kind == "equal":
        cls = np.full((B, N, C), 1.5)
        cls[1] = -2.25
    elif kind == "tie_straddle":
        cls = rng.normal(0.0, 2.0, (B, N, C))
        for b in range(B):
            m = cls[b].max(-1)
            order = np.argsort(-m)
            kk = min(k, N) - 1
            grp = order[max(kk - 150, 0):kk + 150]
            cls[b, grp, :] = m[order[kk]]
    elif kind == "narrow":
        cls = rng.uniform(2.0, 2.2, (B, N, C))
    elif kind == "signed_zero":
        cls = rng.uniform(-MAX_LOGIT, -0.5, (B, N, C))
        z = rng.choice(N, 190, replace=False)
        cls[:, z[:100], 1] = rng.uniform(0.5, 6.0, (B, 100))
        cls[:, z[100:150], :] = [-1.0, 0.0, -0.0][:C] if C == 3 else 0.0
        cls[:, z[150:], :] = [-0.0, 0.0, -1.0][:C] if C == 3 else -0.0
    else:
        raise ValueError(kind)
    return round_storage(np.clip(cls, -MAX_LOGIT, MAX_LOGIT), dtype).reshape(B, H, W, A * C)


def max_logit_keys(cls, A: int, C: int) -> np.ndarray:
    """[B, N] uint32 ordered key of every anchor's max class logit (first maximum)."""
    cls = np.asarray(cls, np.float32)
    B = cls.shape[0]
    cl = cls.reshape(B, -1, C)
    return ordered_key(np.take_along_axis(cl, np.argmax(cl, -1)[..., None], -1)[..., 0])


def topk_threshold_ok(keys: np.ndarray, thr: int, k: int) -> Tuple[bool, bool]:
    """The selection contract for one frame: (count(key >= thr) >= min(k, total),
    count(key >= thr + 256) < k) — the top k plus at most one 256-key bucket."""
    kk = np.asarray(keys, np.uint32).astype(np.int64)
    return bool((kk >= thr).sum() >= min(k, kk.size)), bool((kk >= int(thr) + 256).sum() < k)


# ------------------------------------------------------------------------------ CenterHead
@dataclasses.dataclass
class CenterRef:
    logit: np.ndarray   # [B, T, P] fp64 max heatmap logit
    score: np.ndarray   # [B, T, P]
    label: np.ndarray   # [B, T, P] global label
    box: np.ndarray     # [B, T, P, 9] x, y, z, w, l, h, yaw, vx, vy
    thr: np.ndarray     # [B, T, P] the threshold that applies
    margin: np.ndarray  # [B, T, P, 6] signed distance inside each range face (x, y, z low; x, y, z high)
    keep: np.ndarray    # [B, T, P] bool
    tol: np.ndarray     # [B, T, P, 9]; 0 = bit-equal copy


def centerhead_decode(head, task_info, cls_thresh, score_thresh, range, vsize, osf, pcr,
                      _mutate: str = "") -> CenterRef:
    """task_info: per task (channel offset, classes, first global label); a task's channels are
    [reg 2 | height 1 | dim 3 | rot 2 | vel 2 | hm nc]."""
    head = np.asarray(head, np.float32)
    B, H, W, _ = head.shape
    P, T = H * W, len(task_info)
    st = _f32(score_thresh)
    ix, iy = (np.arange(P) % W).astype(np.float64), (np.arange(P) // W).astype(np.float64)
    sx = (1 if _mutate == "no_osf" else int(osf)) * _f32(vsize[0])
    sy = (1 if _mutate == "no_osf" else int(osf)) * _f32(vsize[1])
    r0, r1 = _f32(range[0]), _f32(range[1])
    pc = [_f32(v) for v in pcr]
    shp = (B, T, P)
    logit, label, thr = np.empty(shp), np.empty(shp, np.int32), np.empty(shp)
    box, tol = np.empty(shp + (9,)), np.zeros(shp + (9,))
    for t, (off, nc, c0) in enumerate(task_info):
        c = head[..., off:off + 10 + nc].reshape(B, P, 10 + nc).astype(np.float64)
        bc = np.argmax(c[..., 10:], -1)
        logit[:, t] = np.take_along_axis(c[..., 10:], bc[..., None], -1)[..., 0]
        lab = c0 + bc + (1 if _mutate == "label_base" else 0)
        label[:, t] = lab
        if cls_thresh is None:
            thr[:, t] = st
        else:
            tab = np.array([max(st, _f32(v)) for v in cls_thresh])
            thr[:, t] = np.where(lab < len(tab), tab[np.minimum(lab, len(tab) - 1)], st)
        for q, (i, s, r) in enumerate(((ix, sx, r0), (iy, sy, r1))):
            es = (i + c[..., q]) * s
            box[:, t, :, q] = es + r
            tol[:, t, :, q] = EPS * (np.abs(es) + abs(r))
        box[:, t, :, 2] = c[..., 2]
        for q in (3, 4, 5):
            box[:, t, :, q] = np.exp(c[..., q])
            tol[:, t, :, q] = EPS * (4.0 + np.abs(c[..., q])) * box[:, t, :, q]
        box[:, t, :, 6] = np.arctan2(c[..., 7], c[..., 6]) if _mutate == "yaw_swap" else np.arctan2(c[..., 6], c[..., 7])
        tol[:, t, :, 6] = ATAN2_TOL
        box[:, t, :, 7:9] = c[..., 8:10]
    score = sigmoid(logit)
    margin = np.stack([box[..., 0] - pc[0], box[..., 1] - pc[1], box[..., 2] - pc[2],
                       pc[3] - box[..., 0], pc[4] - box[..., 1], pc[5] - box[..., 2]], -1)
    above = score >= thr if _mutate == "ge" else score > thr
    return CenterRef(logit, score, label, box, thr, margin, above & (margin >= 0).all(-1), tol)


CENTER_TASKS = (1, 2, 2, 1, 2, 2)  # classes per task (nuScenes)


@dataclasses.dataclass
class CenterCase:
    dtype: str
    head: np.ndarray  # [B, H, W, ldc]
    task_info: List[Tuple[int, int, int]]
    range: Tuple[float, float]
    vsize: Tuple[float, float]
    osf: int
    pcr: Tuple[float, ...]
    face_pixels: List[Tuple[int, int, int]]  # (frame, task, pixel) placed beyond face k

    def ref(self, cls_thresh, score_thresh, _mutate="") -> CenterRef:
        return centerhead_decode(self.head, self.task_info, cls_thresh, score_thresh, self.range, self.vsize,
                                 self.osf, self.pcr, _mutate=_mutate)


def center_band_counts(ref: CenterRef) -> Tuple[int, int]:
    """(scores within twice the fp32 bound of their threshold, range margins of pixels above
    their threshold within RANGE_BAND of a face)."""
    n_s = int((np.abs(ref.score - ref.thr) <= 2 * score_tol(ref.logit, ref.score)).sum())
    n_m = int((np.abs(ref.margin[ref.score > ref.thr]) < RANGE_BAND).sum())
    return n_s, n_m


def make_center_case(dtype="f32", ldc=96, seed=0, H=19, W=23, B=2, thresholds=()) -> CenterCase:
    """Random merged head; the voxel size, out-size factor and range origin are dyadic, so the
    only roundings of x / y are ``pixel + reg`` and the last add.  Frame 0 task 0: pixels 64..127
    never pass and pixels 128..191 all pass (a silent wave beside a full one).  Frame 1 task 3
    has no candidate.  Six pixels of frame 0 task 1 lie beyond one range face each.
    ``thresholds``: every (cls_thresh, score_thresh) pair the case will be run with — all are
    kept out of the score band."""
    rng = np.random.default_rng(seed)
    P = H * W
    info, c0 = [], 0
    for t, nc in enumerate(CENTER_TASKS):
        info.append((16 * t, nc, c0))
        c0 += nc
    head = np.full((B, P, ldc), 11.0)  # gap channels: large, so a misread channel shows
    for off, nc, _ in info:
        head[..., off:off + 2] = rng.uniform(0.0, 1.0, (B, P, 2))
        head[..., off + 2] = rng.normal(0.0, 1.0, (B, P))
        head[..., off + 3:off + 6] = rng.normal(0.0, 0.5, (B, P, 3))
        head[..., off + 6:off + 8] = rng.normal(0.0, 1.0, (B, P, 2))
        head[..., off + 8:off + 10] = rng.normal(0.0, 3.0, (B, P, 2))
        head[..., off + 10:off + 10 + nc] = np.clip(rng.normal(-1.5, 2.0, (B, P, nc)), -MAX_LOGIT, MAX_LOGIT)
    case = CenterCase(dtype, None, info, (-11.5, -19.0), (0.25, 0.5), 4,
                      (-11.25, -18.5, -1.5, 11.0, 18.0, 1.75), [])
    o = info[0][0]
    head[0, 64:128, o + 10] = -8.0
    head[0, 128:192, o + 10] = 4.0
    head[0, 128:192, o:o + 3] = [0.4, 0.5, 0.0]
    o = info[3][0]
    head[1, :, o + 10] = np.minimum(head[1, :, o + 10], -8.0)
    # one pixel beyond each face (x, y, z low; x, y, z high), otherwise well inside and passing
    o = info[1][0]
    mid = (H // 2) * W + W // 2
    spots = [(H // 2) * W, W // 2, mid - 3, (H // 2) * W + W - 1, (H - 1) * W + W // 2, mid + 3]
    for kf, p in enumerate(spots):
        head[0, p, o:o + 3] = [0.5, 0.5, 0.0]
        head[0, p, o + 10:o + 12] = [5.0, -5.0]
        if kf % 3 == 2:
            head[0, p, o + 2] = -2.0 if kf == 2 else 2.25
        else:
            head[0, p, o + kf % 3] = 0.125 if kf < 3 else 0.875
        case.face_pixels.append((0, 1, p))
    case.head = round_storage(head, dtype).reshape(B, H, W, ldc)
    hv = case.head.reshape(B, P, ldc)
    for _ in range(8):
        clean = True
        for ct, st in thresholds:
            ref = case.ref(ct, st)
            bad_s = np.abs(ref.score - ref.thr) <= 2 * score_tol(ref.logit, ref.score)
            bad_m = (np.abs(ref.margin) < RANGE_BAND) & (ref.score > ref.thr)[..., None]
            if not bad_s.any() and not bad_m.any():
                continue
            clean = False
            for t, (off, nc, _) in enumerate(info):
                for b, p in zip(*np.nonzero(bad_s[:, t])):
                    hv[b, p, off + 10:off + 10 + nc] = round_storage(hv[b, p, off + 10:off + 10 + nc] - 0.125, dtype)
                for b, p, f in zip(*np.nonzero(bad_m[:, t])):
                    hv[b, p, off + f % 3] = round_storage(hv[b, p, off + f % 3] + 0.03125, dtype)
        if clean:
            break
    return case


CENTER_THRESH = ("nusc+0.1", "nusc+0.2", "none+0.1")  # per-class table or none + score_thresh


def center_thresholds(name: str, class_table) -> Tuple[Optional[List[float]], float]:
    """(cls_thresh list or None, score_thresh) of a CENTER_THRESH name; ``class_table`` maps the
    global label to its threshold (ops.centerpoint.NUSC_CLASS_THRESH)."""
    tab, st = name.split("+")
    return ([float(class_table[c]) for c in range(sum(CENTER_TASKS))] if tab == "nusc" else None), float(st)


def center_case(dtype: str, ldc: int, class_table) -> CenterCase:
    """The CenterHead test input, clear of the bands of every CENTER_THRESH setting."""
    return make_center_case(dtype, ldc, thresholds=[center_thresholds(n, class_table) for n in CENTER_THRESH])


def make_tie_center_case(dtype="f32") -> CenterCase:
    """One task, one class: heatmap logit exactly 0 on even pixels, -3 on odd ones, every
    centre well inside the range; with score_thresh exactly 0.5 the even pixels tie."""
    H, W, B, ldc = 5, 7, 1, 16
    rng = np.random.default_rng(6)
    P = H * W
    head = rng.normal(0.0, 0.5, (B, P, ldc))
    head[..., 0:2] = 0.5
    head[..., 2] = 0.0
    head[..., 10] = np.where(np.arange(P) % 2 == 0, 0.0, -3.0)
    return CenterCase(dtype, round_storage(head, dtype).reshape(B, H, W, ldc), [(0, 1, 0)], (-11.5, -19.0),
                      (0.25, 0.5), 4, (-11.25, -18.5, -1.5, 11.0, 18.0, 1.75), [])
