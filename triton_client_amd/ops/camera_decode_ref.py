"""Plain NumPy fp64 references of the camera decode kernels: ``tca_yolo_decode_filter`` (K3),
``tca_yolo_decode``, ``tca_yolo_filter_decoded``, ``tca_yolov4_decode`` (``csrc/kernels/yolo.hip``)
and ``tca_retina_decode``, ``tca_fcos_decode``, ``tca_segment_merge``, ``tca_group_norm_nhwc_dt``
(``csrc/kernels/detectron.hip``), written from the operations: the YOLOv5 Detect formulas,
darknet's ``yolo_forward_dynamic``, Detectron2's ``Box2BoxTransform`` with clip, the FCOS
``sqrt(sigmoid(cls) * sigmoid(ctr))`` score, and GroupNorm.  No torch, no GPU.

Conventions (those of ``ops/decode_ref.py``): every head is a *logical* NHWC array of float32
that already holds the values of its storage type (``round_storage``); scalars the launchers
take as C floats are rounded to fp32 here, among them retina's ``logit_thresh =
logf(t / (1 - t))``, which its launcher computes in fp32.  A candidate's identity is the index
its kernel puts in the low key word: K3 ``aidx`` (row of the decoded tensor: level, anchor, y,
x) or ``aidx * nc + c`` in multi-label mode; ``filter_decoded`` the row or ``row * nc + c``;
YOLOv4 the row; retina ``(pix * A + a) * C + k``; FCOS ``pix * C + k``.

The best class is the *first* maximum over the stored logits, which is what the kernels do
(``v > m``) and what is right in fp64.  The fp32 CPU postprocess takes its argmax after
``sigmoid * obj`` in fp32; the two disagree only where two different logits saturate to the
same fp32 sigmoid, so the generators keep |logit| <= 12.  NaN / Inf logits are out of scope.

Error bounds.  E = 2^-23.  One fp32 rounding moves a result v by at most E/2 |v|; a fused
multiply-add only removes roundings, so contraction cannot break a bound.  ``1 / (1 +
__expf(-x))`` is within ``E (4 + |x|)`` relative (derived at the rescore test of
tests/test_spconv_kernels_gpu.py; ``score_tol``), ``__expf(d) * anchor`` within ``E (4 + |d|)``
relative (tests/test_decode_kernels_gpu.py).  fp32 ``/`` and ``sqrtf`` are correctly rounded
(the build passes no fast-math flag).  With s = sigmoid(x) and r(x) = E (4 + |x|):

* YOLOv5 ``c = (2 s - 0.5 + g) * stride``: ``stride (2 s r + E/2 |2 s - 0.5| + E/2 |2 s - 0.5 + g|)
  + E/2 |c|`` (doubling is exact).  ``w = (2 s)^2 * anchor``: ``w (2 r + E)`` (the square and the
  product).  Corners ``c -+ w / 2``: the two bounds (w's halved) + E/2 |corner|.
* scores ``sigmoid(c) * sigmoid(obj)``: relative ``r(c) + r(obj) + E/2``.
* ``filter_decoded``: one fp32 product, E/2 relative; corners ``cx -+ w / 2`` and the kind-1
  scaling one rounding each; kind-1 scores are copies.
* YOLOv4 ``b = (s sxy - 0.5 (sxy - 1) + g) / W``: ``(s sxy (r + E/2) + E/2 |t1| + E/2 |t2|) / W + E/2
  |b|`` with t1, t2 the two partial sums (0.5 (sxy - 1) is exact in fp32 for sxy in [1, 2));
  ``bw = __expf(d) * anchor / W``: ``bw (E (4 + |d|) + E/2)``; ``x1 = b - bw / 2``: the two
  bounds + E/2 |x1|; ``x2 = x1 + bw``: x1's + bw's + E/2 |x2|; candidates ``* img``: scaled + E/2.
* retina ``p = d * a + c``: ``E/2 (|d a| + |p|)``; ``pw = __expf(min(dw, clamp)) * a``:
  ``pw E (4 + |dw|)``; corners ``p -+ pw / 2``: the two bounds + E/2 |corner|; the clip is
  1-Lipschitz.  FCOS corners ``c -+ relu(d) * stride``: ``E/2 (|relu(d) stride| + |corner|)``.
* FCOS enters a class when ``sigmoid(x) > t^2 / max(cs, 1e-12)`` and stores ``sqrtf(p * cs)``.
  The entry test equals the exact ``p cs > t^2`` unless ``|p cs / t^2 - 1| <= r(x) + r(ctr) + E``
  (t*t and the quotient round once each); the stored score is within
  ``score (r(x) + r(ctr) + E/2) / 2 + E/2 score``.  The generators band on both forms.
* GroupNorm: see ``group_norm``.

The ``make_*`` generators keep every input clear of every discontinuity (thresholds, the box
clip at 0 and the image size, retina's ``scale_clamp``, FCOS's relu at 0) by twice the bound that
applies, so membership is exact; ``band counts`` report what is left inside (the tests assert
zero).  Clip-active and clamp-active inputs are placed on purpose.  Strides, anchors and image
sizes are small dyadic numbers, exact in fp32.  ``_mutate`` applies one deliberate defect to
these references only, for the CPU tests that prove the bounds discriminate.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .decode_ref import EPS, MAX_LOGIT, ordered_key, round_storage, score_tol, sigmoid  # noqa: F401

HALF = EPS / 2
RSQRT_ULPS = 2.0  # assumed: rsqrtf within 2 ulp (the HIP math accuracy tables are not installed)
LOGF_ULPS = 4.0   # assumed: the host's logf and NumPy's float32 log within 4 ulp of each other


def _f32(v) -> float:
    return float(np.float32(v))


def _rel(x):
    """Relative bound of the fp32 sigmoid of logit x."""
    return EPS * (4.0 + np.abs(x))


def class_mask_words(nc: int, classes: Sequence[int]) -> np.ndarray:
    """The kernels' class filter: bit c of uint32 word c >> 5."""
    m = np.zeros((nc + 31) // 32, np.uint32)
    for c in classes:
        m[c >> 5] |= np.uint32(1 << (c & 31))
    return m


# ------------------------------------------------------------------------- YOLOv5 (K3, decode)
@dataclasses.dataclass
class YoloCase:
    dtype: str
    na: int
    nc: int
    levels: Tuple[Tuple[int, int], ...]   # (H, W) per level
    strides: Tuple[int, ...]
    anchors: np.ndarray                   # [3, na, 2] float32 (w, h) in pixels
    heads: List[np.ndarray]               # [B, H, W, na * (5 + nc)] per level
    conf: float
    masked_rows: np.ndarray               # rows whose best class is filtered while a lower allowed one passes
    classes: Tuple[int, ...]              # the class filter the case was built for

    @property
    def N(self):
        return sum(self.na * h * w for h, w in self.levels)

    def ref(self, _mutate=""):
        return yolo_decode(self, _mutate)


@dataclasses.dataclass
class YoloRef:
    logit: np.ndarray  # [B, N, 5 + nc] fp64 stored logits in row order
    dec: np.ndarray    # [B, N, 5 + nc] cx, cy, w, h, obj, cls...
    dec_tol: np.ndarray
    box: np.ndarray    # [B, N, 4] x1 y1 x2 y2
    box_tol: np.ndarray


def _yolo_geometry(levels, na, strides, anchors, _mutate=""):
    """Per row of the decoded tensor: (level, anchor, y, x, stride, anchor w, anchor h)."""
    out = []
    for l, (H, W) in enumerate(levels):
        r = np.arange(na * H * W)
        a, yx = (r % na, r // na) if _mutate == "index_order" else (r // (H * W), r % (H * W))
        anc = np.asarray(anchors, np.float32)[l][a].astype(np.float64)
        if _mutate == "wh_swap":
            anc = anc[:, ::-1]
        st = float(strides[0 if _mutate == "level_stride" else l])
        out.append(np.stack([np.full(r.shape, l), a, yx // W, yx % W, np.full(r.shape, st), anc[:, 0], anc[:, 1]], 1))
    return np.concatenate(out)


def _gather_rows(heads, levels, na, no, geo):
    rows, off = [], 0
    for l, (H, W) in enumerate(levels):
        n = na * H * W
        g = geo[off:off + n].astype(np.int64)
        h = np.asarray(heads[l], np.float32)
        rows.append(h.reshape(h.shape[0], H, W, na, no)[:, g[:, 2], g[:, 3], g[:, 1], :])
        off += n
    return np.concatenate(rows, 1).astype(np.float64)


def _yolo_rows(X, geo, _mutate="") -> YoloRef:
    s, r = sigmoid(X), _rel(X)
    half = 0.0 if _mutate == "half_pixel" else 0.5
    st = geo[:, 4][None, :, None]
    g = geo[:, [3, 2]][None]
    t1 = 2 * s[..., 0:2] - half
    t2 = t1 + g
    c = t2 * st
    c_tol = st * (2 * s[..., 0:2] * r[..., 0:2] + HALF * np.abs(t1) + HALF * np.abs(t2)) + HALF * np.abs(c)
    wh = (2 * s[..., 2:4]) ** 2 * geo[:, 5:7][None]
    wh_tol = wh * (2 * r[..., 2:4] + EPS)
    dec = np.concatenate([c, wh, s[..., 4:]], -1)
    dec_tol = np.concatenate([c_tol, wh_tol, s[..., 4:] * r[..., 4:]], -1)
    box = np.concatenate([c - wh / 2, c + wh / 2], -1)
    box_tol = np.concatenate([c_tol + wh_tol / 2] * 2, -1) + HALF * np.abs(box)
    return YoloRef(X, dec, dec_tol, box, box_tol)


def yolo_decode(case: YoloCase, _mutate="") -> YoloRef:
    geo = _yolo_geometry(case.levels, case.na, case.strides, case.anchors, _mutate)
    return _yolo_rows(_gather_rows(case.heads, case.levels, case.na, case.nc + 5, geo), geo, _mutate)


@dataclasses.dataclass
class Filt:
    """Candidates by identity: M = N (single label) or N * nc (multi label)."""
    keep: np.ndarray   # [B, M] bool
    score: np.ndarray  # [B, M]
    tol: np.ndarray    # [B, M]
    cls: np.ndarray    # [B, M]
    row: np.ndarray    # [M] row of the box
    bad_obj: np.ndarray  # [B, N] objectness inside its band
    bad_cls: np.ndarray  # [B, N] (single) / [B, N, nc] (multi) score inside its band, on rows above the obj gate

    def band_counts(self):
        return int(self.bad_obj.sum()), int(self.bad_cls.sum())


def _filter(obj, obj_tol, sc, sc_tol, order, conf, multi_label, classes, _mutate="", obj_gate=True) -> Filt:
    """obj [B, N], sc [B, N, nc] class scores, order [B, N, nc] what the argmax runs over."""
    B, N, nc = sc.shape
    t = _f32(conf)
    allowed = np.ones(nc, bool)
    if classes is not None:
        allowed[:] = False
        allowed[list(classes)] = True
    gate = obj > t if obj_gate else np.ones((B, N), bool)
    bad_obj = np.abs(obj - t) <= 2 * obj_tol if obj_gate else np.zeros((B, N), bool)
    if multi_label:
        keep = gate[..., None] & (sc > t) & allowed
        bad = gate[..., None] & (np.abs(sc - t) <= 2 * sc_tol)
        return Filt(keep.reshape(B, -1), sc.reshape(B, -1), sc_tol.reshape(B, -1),
                    np.tile(np.arange(nc), (B, N)).reshape(B, -1), np.repeat(np.arange(N), nc), bad_obj, bad)
    if _mutate == "filter_before_argmax":
        order = np.where(allowed, order, -np.inf)
    c = np.argmax(order, -1)  # first maximum
    best = np.take_along_axis(sc, c[..., None], -1)[..., 0]
    tol = np.take_along_axis(sc_tol, c[..., None], -1)[..., 0]
    keep = gate & (best > t) & allowed[c]
    return Filt(keep, best, tol, c, np.arange(N), bad_obj, gate & (np.abs(best - t) <= 2 * tol))


def yolo_filter(ref: YoloRef, conf, multi_label=False, classes=None, _mutate="") -> Filt:
    """K3's filter: ``obj > t``, then the best class's ``sigmoid(cls) * obj > t`` with the class
    filter applied *after* the argmax (a row whose best class is filtered is dropped, never
    promoted), or every allowed class above t in multi-label mode."""
    obj, lg = ref.dec[..., 4], ref.logit[..., 5:]
    sc = ref.dec[..., 5:] * obj[..., None]
    sc_tol = sc * (_rel(lg) + _rel(ref.logit[..., 4])[..., None] + HALF)
    return _filter(obj, ref.dec_tol[..., 4], sc, sc_tol, lg, conf, multi_label, classes, _mutate)


def yolo_anchors(na: int) -> np.ndarray:
    a = np.arange(na, dtype=np.float64)
    return np.stack([np.stack([2.0 ** (l + 3) * (1 + a / 2), 2.0 ** (l + 3) * (0.75 + a / 4)], 1)
                     for l in range(3)]).astype(np.float32)


YOLO_LEVELS = ((12, 9), (6, 5), (3, 3))
YOLO_CLASSES = tuple(c for c in range(37) if c % 3 != 1)  # filtered: 1, 4, ..., 34 (both mask words)


def _scatter_rows(X, levels, na, no, geo, dtype):
    heads, off = [], 0
    for l, (H, W) in enumerate(levels):
        n = na * H * W
        g = geo[off:off + n].astype(np.int64)
        h = np.zeros((X.shape[0], H, W, na, no), np.float32)
        h[:, g[:, 2], g[:, 3], g[:, 1], :] = X[:, off:off + n]
        heads.append(round_storage(h.reshape(X.shape[0], H, W, na * no), dtype))
        off += n
    return heads


def make_yolo_case(dtype="f32", na=3, nc=37, B=1, seed=0, conf=0.25, levels=YOLO_LEVELS,
                   classes=YOLO_CLASSES) -> YoloCase:
    """Random heads, |logit| <= 12: roughly a third of the rows pass the objectness gate and
    most of those have several classes above the threshold.  Every 17th row is built so that its
    best class is a filtered one while a lower, allowed class also passes.  Clear of the bands
    of all four filter modes (the multi-label bands contain the single-label ones)."""
    rng = np.random.default_rng(seed)
    no = nc + 5
    strides = (8, 16, 32)
    anchors = yolo_anchors(na)
    geo = _yolo_geometry(levels, na, strides, anchors)
    N = len(geo)
    X = np.concatenate([rng.normal(0.0, 1.5, (B, N, 4)), rng.normal(-1.0, 2.5, (B, N, 1)),
                        rng.normal(-2.0, 2.5, (B, N, nc))], -1)
    masked = np.arange(5, N, 17)
    if classes is not None and nc > 8:
        out = [c for c in range(nc) if c not in classes]
        X[:, masked, 4] = 6.0
        X[:, masked, 5:] = -6.0
        X[:, masked, 5 + out[-1]] = 5.0              # best, filtered (second mask word when nc > 32)
        X[:, masked, 5 + classes[len(classes) // 2]] = 4.0  # allowed, lower, above the threshold
    else:
        masked = masked[:0]
    X = round_storage(np.clip(X, -MAX_LOGIT, MAX_LOGIT), dtype).astype(np.float64)
    for _ in range(8):
        f = yolo_filter(_yolo_rows(X, geo), conf, multi_label=True)
        if not f.bad_obj.any() and not f.bad_cls.any():
            break
        X[..., 4][f.bad_obj] -= 0.125
        X[..., 5:][f.bad_cls] -= 0.125
        X = round_storage(X, dtype).astype(np.float64)
    return YoloCase(dtype, na, nc, tuple(levels), strides, anchors, _scatter_rows(X, levels, na, no, geo, dtype), conf,
                    masked, tuple(classes) if classes is not None else None)


# ------------------------------------------------------------------------------ filter_decoded
@dataclasses.dataclass
class DecodedCase:
    kind: int
    nc: int
    pred: np.ndarray              # kind 0: [B, N, ld] rows (cx, cy, w, h, obj, cls[nc], pad); kind 1: [B, N, 4]
    confs: Optional[np.ndarray]   # kind 1: [B, N, nc]
    conf: float
    img_wh: Tuple[float, float]


def filter_decoded(case: DecodedCase, multi_label=False, classes=None, _mutate=""):
    """→ (Filt, box [B, N, 4], box_tol).  Scores are fp32 products of fp32 inputs (kind 0: one
    rounding) or copies (kind 1: tol 0); the best class is the first maximum of those products,
    so the generator keeps the two largest apart."""
    if case.kind == 0:
        p = np.asarray(case.pred, np.float32).astype(np.float64)
        obj = p[..., 4]
        sc = p[..., 5:5 + case.nc] * obj[..., None]
        c, w = p[..., 0:2], p[..., 2:4]
        box = np.concatenate([c - w / 2, c + w / 2], -1)
        f = _filter(obj, np.zeros_like(obj), sc, HALF * np.abs(sc), sc, case.conf, multi_label, classes, _mutate)
        return f, box, HALF * np.abs(box)
    cf = np.asarray(case.confs, np.float32).astype(np.float64)
    wh = np.array([_f32(case.img_wh[0]), _f32(case.img_wh[1])] * 2)
    if _mutate == "xw_xh":
        wh = wh[[1, 1, 1, 1]]
    box = np.asarray(case.pred, np.float32).astype(np.float64) * wh
    f = _filter(cf.max(-1), np.zeros(cf.shape[:2]), cf, np.zeros_like(cf), cf, case.conf, False, None, obj_gate=False)
    return f, box, HALF * np.abs(box)


def decoded_gap_count(case: DecodedCase) -> int:
    """Rows whose two largest class scores are closer than twice their rounding (kind 0)."""
    if case.kind != 0:
        return 0
    p = np.asarray(case.pred, np.float32).astype(np.float64)
    s = np.sort(p[..., 5:5 + case.nc] * p[..., 4:5], -1)
    return int((s[..., -1] - s[..., -2] <= 2 * EPS * s[..., -1]).sum())


def make_decoded_case(kind=0, nc=37, N=300, B=2, pad=3, seed=0, conf=0.25) -> DecodedCase:
    rng = np.random.default_rng(seed)
    if kind == 0:
        p = np.full((B, N, nc + 5 + pad), 11.0)  # pad columns pass every threshold
        p[..., 0:2] = rng.uniform(0.0, 416.0, (B, N, 2))
        p[..., 2:4] = rng.uniform(2.0, 200.0, (B, N, 2))
        p[..., 4] = rng.uniform(0.0, 1.0, (B, N))
        p[..., 5:5 + nc] = rng.uniform(0.0, 1.0, (B, N, nc)) ** 3
        case = DecodedCase(0, nc, p.astype(np.float32), None, conf, (0.0, 0.0))
        t = _f32(conf)
        for _ in range(8):
            v = case.pred.astype(np.float64)
            sc = v[..., 5:5 + nc] * v[..., 4:5]
            top = np.sort(sc, -1)
            bad = (np.abs(sc - t) <= 2 * HALF * sc) | ((sc == top[..., -1:]) & (top[..., -1:] - top[..., -2:-1] <= 2 * EPS * sc))
            bad |= (v[..., 4:5] == t)
            if not bad.any():
                break
            case.pred[..., 5:5 + nc][bad] *= np.float32(0.96875)
        return case
    boxes = np.sort(rng.uniform(-0.05, 1.05, (B, N, 2, 2)), 2).reshape(B, N, 4)
    confs = rng.uniform(0.0, 1.0, (B, N, nc)) ** 2
    return DecodedCase(1, nc, boxes.astype(np.float32), confs.astype(np.float32), conf, (96.0, 160.0))


# ------------------------------------------------------------------------------------- YOLOv4
@dataclasses.dataclass
class Yolov4Case:
    dtype: str
    nc: int
    levels: Tuple[Tuple[int, int], ...]
    anchors: np.ndarray          # [3, 3, 2] float32, already divided by the level stride
    heads: List[np.ndarray]      # [B, H, W, 3 * (5 + nc)]
    sxy: float
    conf: float
    img_hw: Tuple[int, int]

    def ref(self, _mutate=""):
        return yolov4_decode(self, _mutate)


@dataclasses.dataclass
class Yolov4Ref:
    boxes: np.ndarray   # [B, N, 4] normalised x1 y1 x2 y2 (the served ``boxes`` output)
    boxes_tol: np.ndarray
    confs: np.ndarray   # [B, N, nc]
    confs_tol: np.ndarray
    cand: np.ndarray    # [B, N, 4] boxes in model pixels
    cand_tol: np.ndarray
    filt: Filt


def yolov4_decode(case: Yolov4Case, _mutate="") -> Yolov4Ref:
    geo = _yolo_geometry(case.levels, 3, (0, 0, 0), case.anchors, "wh_swap" if _mutate == "wh_swap" else "")
    X = _gather_rows(case.heads, case.levels, 3, case.nc + 5, geo)
    return _yolov4_rows(X, geo, case, _mutate)


def _yolov4_rows(X, geo, case, _mutate="") -> Yolov4Ref:
    dims = np.array([[w, h] for h, w in case.levels], np.float64)[geo[:, 0].astype(np.int64)]  # [N, (W, H)]
    if _mutate == "xw_xh":
        dims = dims[:, [1, 1]]
    sxy = _f32(case.sxy)
    k = 0.0 if _mutate == "no_sxy_shift" else 0.5 * (sxy - 1.0)
    s, r = sigmoid(X[..., 0:2]), _rel(X[..., 0:2])
    p = s * sxy
    t1 = p - k
    t2 = t1 + geo[:, [3, 2]][None]
    b = t2 / dims
    b_tol = (p * (r + HALF) + HALF * np.abs(t1) + HALF * np.abs(t2)) / dims + HALF * np.abs(b)
    wh = np.exp(X[..., 2:4]) * geo[:, 5:7][None] / dims
    wh_tol = wh * (EPS * (4.0 + np.abs(X[..., 2:4])) + HALF)
    x1 = b - wh / 2
    x1_tol = b_tol + wh_tol / 2 + HALF * np.abs(x1)
    x2 = b + wh / 2
    x2_tol = x1_tol + wh_tol + HALF * np.abs(x2)
    boxes, boxes_tol = np.concatenate([x1, x2], -1), np.concatenate([x1_tol, x2_tol], -1)
    obj = sigmoid(X[..., 4])
    confs = sigmoid(X[..., 5:]) * obj[..., None]
    confs_tol = confs * (_rel(X[..., 5:]) + _rel(X[..., 4])[..., None] + HALF)
    img = np.array([case.img_hw[1], case.img_hw[0]] * 2, np.float64)
    cand = boxes * img
    cand_tol = boxes_tol * img + HALF * np.abs(cand)
    f = _filter(obj, np.zeros_like(obj), confs, confs_tol, X[..., 5:], case.conf, False, None, obj_gate=False)
    return Yolov4Ref(boxes, boxes_tol, confs, confs_tol, cand, cand_tol, f)


def yolov4_anchors() -> np.ndarray:
    """Dyadic (w, h) in grid cells, growing with the level and the anchor."""
    a = np.arange(3, dtype=np.float64)
    return np.stack([np.stack([0.75 * (l + 1) * (1 + a / 2), 0.5 * (l + 1) * (1.5 + a / 4)], 1)
                     for l in range(3)]).astype(np.float32)


def make_yolov4_case(dtype="f32", nc=7, sxy=1.0, B=2, seed=0, conf=0.25, levels=YOLO_LEVELS, img_hw=(96, 160),
                     anchors=None) -> Yolov4Case:
    rng = np.random.default_rng(seed)
    anchors = yolov4_anchors() if anchors is None else np.asarray(anchors, np.float32)
    geo = _yolo_geometry(levels, 3, (0, 0, 0), anchors)
    N = len(geo)
    X = np.concatenate([rng.normal(0.0, 1.5, (B, N, 2)), rng.normal(0.0, 0.7, (B, N, 2)),
                        rng.normal(0.0, 2.5, (B, N, 1)), rng.normal(-1.0, 2.5, (B, N, nc))], -1)
    X = round_storage(np.clip(X, -MAX_LOGIT, MAX_LOGIT), dtype).astype(np.float64)
    case = Yolov4Case(dtype, nc, tuple(levels), anchors, [], sxy, conf, tuple(img_hw))
    for _ in range(8):
        f = _yolov4_rows(X, geo, case).filt
        if not f.bad_cls.any():
            break
        X[..., 5:][f.bad_cls] -= 0.125
        X = round_storage(X, dtype).astype(np.float64)
    case.heads = _scatter_rows(X, levels, 3, nc + 5, geo, dtype)
    return case


# ------------------------------------------------------------------------------ retina / FCOS
def logit_thresh32(t) -> float:
    """The launcher's ``logf(t / (1.f - t))``, every step in fp32."""
    t = np.float32(t)
    return float(np.log(t / (np.float32(1.0) - t), dtype=np.float32))


@dataclasses.dataclass
class LevelRef:
    keep: np.ndarray   # [B, M] by identity
    score: np.ndarray  # [B, M]
    tol: np.ndarray    # [B, M]
    cls: np.ndarray    # [M]
    row: np.ndarray    # [M] row of box
    box: np.ndarray    # [B, R, 4] clipped
    raw: np.ndarray    # [B, R, 4] before the clip
    box_tol: np.ndarray
    bands: Tuple[int, ...]


def _clip(raw, img_h, img_w):
    hi = np.array([_f32(img_w), _f32(img_h)] * 2)
    return np.clip(raw, 0.0, hi), hi


def retina_decode(cls, box, A, C, stride, anchors, score_thresh, scale_clamp, img_h, img_w, _mutate="") -> LevelRef:
    """One level: a class enters when its stored logit exceeds ``logit_thresh32`` (all classes
    of an anchor may); Box2BoxTransform with weights 1 around the anchor centred on
    (x * stride, y * stride), dw / dh clamped at ``scale_clamp``; clip to the image.
    bands: (logits within LOGF_ULPS of the threshold, dw / dh equal to the clamp, corners of
    entered anchors within twice their bound of a clip edge)."""
    cls, box = np.asarray(cls, np.float32), np.asarray(box, np.float32)
    B, H, W = cls.shape[:3]
    R = H * W * A
    ids = np.arange(R)
    a, pix = (ids // (H * W), ids % (H * W)) if _mutate == "index_order" else (ids % A, ids // A)
    v = cls.reshape(B, H * W, A, C)[:, pix, a, :].astype(np.float64)   # [B, R, C]
    d = box.reshape(B, H * W, A, 4)[:, pix, a, :].astype(np.float64)
    anc = np.asarray(anchors, np.float32).reshape(A, 2)[a].astype(np.float64)
    if _mutate == "wh_swap":
        anc = anc[:, ::-1]
    st = float(stride) * (2 if _mutate == "level_stride" else 1)
    ctr = np.stack([(pix % W) * st, (pix // W) * st], 1)[None]
    lt, clamp = logit_thresh32(score_thresh), _f32(scale_clamp)
    keep = v > lt
    s = sigmoid(v)
    p = d[..., 0:2] * anc + ctr
    p_tol = HALF * (np.abs(d[..., 0:2] * anc) + np.abs(p))
    dwh = d[..., 2:4] if _mutate == "no_clamp" else np.minimum(d[..., 2:4], clamp)
    pw = np.exp(dwh) * anc
    pw_tol = pw * EPS * (4.0 + np.abs(dwh))
    raw = np.concatenate([p - pw / 2, p + pw / 2], -1)
    tol = np.concatenate([p_tol + pw_tol / 2] * 2, -1) + HALF * np.abs(raw)
    clipped, hi = _clip(raw, img_h, img_w)
    entered = keep.any(-1)[..., None]
    bands = (int((np.abs(v - lt) <= 2 * LOGF_ULPS * EPS * abs(lt)).sum()), int((d[..., 2:4] == clamp).sum()),
             int((entered & ((np.abs(raw) <= 2 * tol) | (np.abs(raw - hi) <= 2 * tol))).sum()))
    return LevelRef(keep.reshape(B, -1), s.reshape(B, -1), score_tol(v, s).reshape(B, -1), np.tile(np.arange(C), R),
                    np.repeat(ids, C), clipped, raw, tol, bands)


def fcos_decode(cls, box, ctr, stride, score_thresh, img_h, img_w, _mutate="") -> LevelRef:
    """One level: point (x + 0.5, y + 0.5) * stride, ltrb = relu(deltas) * stride, clip; class k
    of a pixel enters when sigmoid(cls) > t^2 / max(sigmoid(ctr), 1e-12), score sqrt(p * cs).
    bands: (entry test, stored score against t, deltas exactly 0, corners near a clip edge)."""
    cls, box, ctr = (np.asarray(t, np.float32) for t in (cls, box, ctr))
    B, H, W, C = cls.shape
    R = H * W
    pix = np.arange(R)
    x, xc = cls.reshape(B, R, C).astype(np.float64), ctr.reshape(B, R).astype(np.float64)
    d = box.reshape(B, R, 4).astype(np.float64)
    t = _f32(score_thresh)
    p, cs = sigmoid(x), sigmoid(xc)[..., None]
    q = p * cs
    keep = p > t * t / np.maximum(cs, 1e-12)
    rel = _rel(x) + _rel(xc)[..., None]
    score = np.sqrt(q)
    tol = score * ((rel + HALF) / 2 + HALF)
    st = float(stride) * (2 if _mutate == "level_stride" else 1)
    half = 0.0 if _mutate == "half_pixel" else 0.5
    c = np.stack([(pix % W + half) * st, (pix // W + half) * st], 1)[None]
    ltrb = np.maximum(d, 0.0) * st
    raw = np.concatenate([c - ltrb[..., 0:2], c + ltrb[..., 2:4]], -1)
    btol = HALF * (np.abs(ltrb) + np.abs(raw))
    clipped, hi = _clip(raw, img_h, img_w)
    entered = keep.any(-1)[..., None]
    bands = (int((np.abs(q / (t * t) - 1.0) <= 2 * (rel + EPS)).sum()), int((np.abs(score - t) <= 2 * tol).sum()),
             int((d == 0).sum()),
             int((entered & ((np.abs(raw) <= 2 * btol) | (np.abs(raw - hi) <= 2 * btol)) & (raw != 0) & (raw != hi)).sum()))
    return LevelRef(keep.reshape(B, -1), score.reshape(B, -1), tol.reshape(B, -1), np.tile(np.arange(C), R),
                    np.repeat(pix, C), clipped, raw, btol, bands)


@dataclasses.dataclass
class DetLevel:
    H: int
    W: int
    stride: int
    cls: np.ndarray
    box: np.ndarray
    ctr: Optional[np.ndarray] = None       # FCOS [B, H, W]
    anchors: Optional[np.ndarray] = None   # retina [A, 2]


@dataclasses.dataclass
class DetCase:
    arch: str
    dtype: str
    A: int
    C: int
    levels: List[DetLevel]
    thresh: float
    scale_clamp: float
    img_hw: Tuple[int, int]
    placed: dict  # name -> (level, frame, row): rows built to clip on each side / to clamp

    def ref(self, l, _mutate="") -> LevelRef:
        L = self.levels[l]
        if self.arch == "retinanet":
            return retina_decode(L.cls, L.box, self.A, self.C, L.stride, L.anchors, self.thresh, self.scale_clamp,
                                 *self.img_hw, _mutate=_mutate)
        return fcos_decode(L.cls, L.box, L.ctr, L.stride, self.thresh, *self.img_hw, _mutate=_mutate)


def retina_anchors(A: int, size: float) -> np.ndarray:
    """A = 3: Detectron2's ratios (0.25, 1, 4) of one dyadic size; otherwise a dyadic ramp."""
    if A == 3:
        return np.array([[2 * size, size / 2], [size, size], [size / 2, 2 * size]], np.float32)
    a = np.arange(A, dtype=np.float64)
    return np.stack([size / 2 + a / 4 * size / 4, 2 * size - a / 4 * size / 4], 1).astype(np.float32)


DET_LEVELS = ((7, 9, 8), (4, 5, 16))


def make_retina_case(dtype="f32", A=3, C=5, B=2, seed=0, levels=DET_LEVELS, thresh=0.25, scale_clamp=0.75,
                     img_hw=(56, 72)) -> DetCase:
    """Random heads; about a sixth of the anchors enter, many with several classes.  On frame 0
    of level 0 four anchors are pushed across the left / top / right / bottom image edge and one
    (unclipped) has dw, dh beyond ``scale_clamp``."""
    rng = np.random.default_rng(seed)
    case = DetCase("retinanet", dtype, A, C, [], thresh, scale_clamp, tuple(img_hw), {})
    lt = logit_thresh32(thresh)
    for l, (H, W, st) in enumerate(levels):
        anc = retina_anchors(A, float(st))
        cls = np.clip(rng.normal(-3.0, 2.5, (B, H * W, A, C)), -MAX_LOGIT, MAX_LOGIT)
        box = rng.normal(0.0, 0.4, (B, H * W, A, 4))
        if l == 0:
            mid = (H // 2) * W + W // 2
            spots = {"left": ((H // 2) * W, 0, (-2.0, 0, 0, 0)), "top": (W // 2, 0, (0, -2.0, 0, 0)),
                     "right": ((H // 2) * W + W - 1, 0, (2.0, 0, 0, 0)), "bottom": ((H - 1) * W + W // 2, 0, (0, 2.0, 0, 0)),
                     "clamp": (mid, 1, (0.125, -0.125, 1.5, 2.0))}
            for name, (pix, a, dl) in spots.items():
                cls[0, pix, a, :] = [3.0, 2.0] + [-6.0] * (C - 2)
                box[0, pix, a, :] = dl
                case.placed[name] = (0, 0, pix * A + a)
        cls, box = round_storage(cls, dtype), round_storage(box, dtype)
        bad = np.abs(cls - lt) <= 2 * LOGF_ULPS * EPS * abs(lt)
        cls[bad] = round_storage(cls[bad] - 0.125, dtype)
        case.levels.append(DetLevel(H, W, st, cls.reshape(B, H, W, A * C), box.reshape(B, H, W, A * 4), None, anc))
        for _ in range(8):
            ref = case.ref(l)
            near = ((np.abs(ref.raw) <= 2 * ref.box_tol) | (np.abs(ref.raw - _clip(ref.raw, *img_hw)[1]) <= 2 * ref.box_tol))
            if not near.any():
                break
            bx = case.levels[l].box.reshape(B, H * W * A, 4)
            for b, r, q in zip(*np.nonzero(near)):
                bx[b, r, q % 2] = round_storage(bx[b, r, q % 2] + 0.03125, dtype)
    return case


def make_fcos_case(dtype="f32", C=5, B=2, seed=0, levels=DET_LEVELS, thresh=0.2, img_hw=(56, 72)) -> DetCase:
    """Random heads with centre-ness logits from -12 up (a fifth pinned at -12: tiny cs, nothing
    enters), half of the deltas negative (relu), and on frame 0 of level 0 four pixels whose
    box crosses one image edge each."""
    rng = np.random.default_rng(seed)
    case = DetCase("fcos", dtype, 1, C, [], thresh, 0.0, tuple(img_hw), {})
    for l, (H, W, st) in enumerate(levels):
        cls = np.clip(rng.normal(-1.0, 2.5, (B, H * W, C)), -MAX_LOGIT, MAX_LOGIT)
        ctr = np.clip(rng.normal(0.0, 3.0, (B, H * W)), -MAX_LOGIT, MAX_LOGIT)
        ctr[:, ::5] = -12.0
        box = rng.normal(0.3, 0.8, (B, H * W, 4))
        box[np.abs(box) < 2.0 ** -6] = 0.25
        if l == 0:
            spots = {"left": ((H // 2) * W + 1, 0), "top": (W + W // 2, 1), "right": ((H // 2) * W + W - 2, 2),
                     "bottom": ((H - 2) * W + W // 2, 3)}
            for name, (pix, q) in spots.items():
                cls[0, pix, :] = [3.0, 2.0] + [-6.0] * (C - 2)
                ctr[0, pix] = 2.0
                box[0, pix, :] = 0.25
                box[0, pix, q] = 2.5
                case.placed[name] = (0, 0, pix)
        cls, ctr, box = round_storage(cls, dtype), round_storage(ctr, dtype), round_storage(box, dtype)
        case.levels.append(DetLevel(H, W, st, cls.reshape(B, H, W, C), box.reshape(B, H, W, 4), ctr.reshape(B, H, W)))
        for _ in range(8):
            ref = case.ref(l)
            x, xc = cls.astype(np.float64), ctr.astype(np.float64)[..., None]
            q = sigmoid(x) * sigmoid(xc)
            t = _f32(thresh)
            rel = _rel(x) + _rel(xc)
            bad = (np.abs(q / (t * t) - 1.0) <= 2 * (rel + EPS)) | (np.abs(np.sqrt(q) - t) <= 2 * ref.tol.reshape(q.shape))
            near = ((np.abs(ref.raw) <= 2 * ref.box_tol) | (np.abs(ref.raw - _clip(ref.raw, *img_hw)[1]) <= 2 * ref.box_tol)) \
                & (ref.raw != 0) & (ref.raw != _clip(ref.raw, *img_hw)[1])
            if not bad.any() and not near.any():
                break
            cls[bad] = round_storage(cls[bad] - 0.125, dtype)
            box[near] = round_storage(box[near] + 0.0625, dtype)
    return case


# -------------------------------------------------------------------------------- segment merge
def segment_merge(box, score, cls, key, order, sorted_n, B, L, cap_out):
    """Concatenate each image's L sorted level lists in level order, first ``cap_out`` only.
    Arrays are bit patterns: box [S, cap_in, D] uint32, score [S, cap_in] uint32, cls int32,
    key uint64; order [S, pre_max], sorted_n [S].  → per image a list of (box, score, cls, key)
    and the count.  The key keeps its high word; the low word becomes 0xffffffff - position."""
    out = []
    for b in range(B):
        rows = []
        for l in range(L):
            s = b * L + l
            for j in range(int(sorted_n[s])):
                o = len(rows)
                if o >= cap_out:
                    break
                src = int(order[s, j])
                k = (int(key[s, src]) & 0xFFFFFFFF00000000) | (0xFFFFFFFF - o)
                rows.append((box[s, src].copy(), score[s, src], cls[s, src], np.uint64(k)))
        out.append((rows, min(sum(int(sorted_n[b * L + l]) for l in range(L)), cap_out)))
    return out


# ---------------------------------------------------------------------------------- GroupNorm
@dataclasses.dataclass
class GnRef:
    y: np.ndarray      # [B, HW, C] fp64
    tol: np.ndarray    # [B, HW, C] bound on |fp32 kernel - y|
    cond: np.ndarray   # [B, G] mean^2 / var of the stored inputs
    two_pass_tol: np.ndarray  # the same bound with the variance's cancellation term left out


def gn_accumulation_factor(HW: int, cg: int, block=256) -> int:
    """Additions an input passes through on its way into the block's sum: its thread's strided
    partial sum (ceil(HW / block) pixels x cg channels), six wave butterfly steps, and the
    serial sum over the block's waves."""
    return -(-HW // block) * cg + 6 + block // 64


def group_norm(x, G, eps, gamma, beta, relu, _mutate="") -> GnRef:
    """GroupNorm over [B, HW, C] (stored values), groups of C / G adjacent channels, biased
    variance, affine, optional ReLU — and the bound of the kernel's fp32 evaluation: one pass
    ``var = SS / n - mean^2`` over per-thread partial sums and a tree.

    With K = ``gn_accumulation_factor``, m1 = mean |x|, m2 = mean x^2 = var + mean^2 and
    h = E/2: an input passes through at most K additions, so |dS| <= K h sum|x| and, with each
    square rounded first, |dSS| <= (K + 1) h sum x^2.  Then
    ``dmean <= K h m1 + h |mean|`` (the division), ``d(SS/n) <= (K + 2) h m2``,
    ``d(mean^2) <= 2 |mean| dmean + h mean^2`` and
    ``dvar <= (K + 2) h m2 + 2 |mean| dmean + h mean^2 + h var  <=  h (3 K + 5) var (1 + mean^2 / var)``:
    the relative error of the variance grows with the conditioning mean^2 / var.  A two-pass
    variance has ``dvar <= h (K + 3) var`` plus second-order terms (``two_pass_tol``).
    ``w = var + eps`` adds h w; ``rsqrtf`` is assumed within RSQRT_ULPS ulp, so rstd is off by at
    most rho = (1 - dw / w)^(-1/2) - 1 + RSQRT_ULPS E relative (infinite when dw >= w).
    ``y = (x - mean) rstd gamma + beta``: d = x - mean carries dmean + h |d|, the two products
    E/2 each, the sum E/2 |y|:
    ``tol = |gamma| rstd (1 + rho) (dmean + h |d|) + |d rstd gamma| (rho + E) + h |y|``."""
    x = np.asarray(x, np.float32).astype(np.float64)
    B, HW, C = x.shape
    cg = C // G
    n = HW * cg
    xg = x.reshape(B, HW, G, cg)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    m1, m2 = np.abs(xg).mean((1, 3)), (xg ** 2).mean((1, 3))
    if _mutate == "unbiased":
        var = var * n / (n - 1)
    e = _f32(eps)
    K, h = gn_accumulation_factor(HW, cg), HALF
    dmean = K * h * m1 + h * np.abs(mean)
    w = var + e

    def rho(dvar):
        dw = dvar + h * w
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(dw < w, (1.0 - np.minimum(dw / w, 1.0 - 1e-16)) ** -0.5 - 1.0, np.inf) + RSQRT_ULPS * EPS

    rho1 = rho((K + 2) * h * m2 + 2 * np.abs(mean) * dmean + h * mean ** 2 + h * var)
    rho2 = rho((K + 3) * h * var)
    rstd = w ** -0.5
    ga = np.asarray(gamma, np.float32).astype(np.float64).reshape(G, cg)
    be = np.asarray(beta, np.float32).astype(np.float64).reshape(G, cg)
    d = xg - mean[:, None, :, None]
    z = d * rstd[:, None, :, None] * ga
    y = z + be
    if relu:
        y = np.maximum(y, 0.0)

    def tol(r):
        r = r[:, None, :, None]
        with np.errstate(invalid="ignore"):
            return (np.abs(ga) * rstd[:, None, :, None] * (1 + r) * (dmean[:, None, :, None] + h * np.abs(d))
                    + np.abs(z) * (r + EPS) + h * np.abs(z + be)).reshape(B, HW, C)

    return GnRef(y.reshape(B, HW, C), tol(rho1), mean ** 2 / var, tol(rho2))


def group_norm_onepass_f32(x, G, eps, gamma, beta, relu, fma=False, block=256) -> np.ndarray:
    """The kernel's arithmetic in NumPy float32: per-thread partial sums over pixels t, t + 256,
    ... and the group's channels in order, a six-step xor butterfly per wave, the waves summed
    in order, ``var = max(SS / n - mean^2, 0)``, then the apply expression.  ``fma``: the square
    enters the running sum unrounded (the compiler may contract ``ss += f * f``)."""
    f32 = np.float32
    x = np.asarray(x, f32)
    B, HW, C = x.shape
    cg = C // G
    xg = x.reshape(B, HW, G, cg)
    rounds = -(-HW // block)
    pad = np.zeros((B, rounds * block, G, cg), f32)
    pad[:, :HW] = xg
    pad = pad.reshape(B, rounds, block, G, cg)
    live = (np.arange(rounds * block).reshape(rounds, block) < HW)
    s, ss = np.zeros((B, block, G), f32), np.zeros((B, block, G), f32)
    for r in range(rounds):
        for k in range(cg):
            f = pad[:, r, :, :, k]
            m = live[r][None, :, None]
            s = np.where(m, s + f, s)
            if fma:
                ss = np.where(m, (ss.astype(np.float64) + f.astype(np.float64) ** 2).astype(f32), ss)
            else:
                ss = np.where(m, ss + f * f, ss)

    def tree(v):
        v = v.reshape(B, block // 64, 64, G)
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, np.arange(64) ^ o, :]
        w = np.zeros((B, G), f32)
        for i in range(block // 64):
            w = w + v[:, i, 0, :]
        return w

    S, SS = tree(s), tree(ss)
    n = f32(HW) * f32(cg)
    mean = S / n
    var = np.maximum(SS / n - mean * mean, f32(0))
    rstd = (f32(1) / np.sqrt((var + f32(eps)).astype(np.float64))).astype(f32)
    ga, be = np.asarray(gamma, f32).reshape(G, cg), np.asarray(beta, f32).reshape(G, cg)
    y = (xg - mean[:, None, :, None]) * rstd[:, None, :, None] * ga + be
    if relu:
        y = np.maximum(y, f32(0))
    return y.reshape(B, HW, C)


def make_gn_input(dtype, B, HW, C, G, ratio, seed=0) -> np.ndarray:
    """[B, HW, C] stored values: unit-variance noise around ``ratio`` (mean / std per group),
    with a per-channel offset of a tenth of a standard deviation so channels differ."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (B, HW, C)) + 0.1 * rng.normal(0.0, 1.0, (1, 1, C)) + ratio
    return round_storage(x, dtype)


def bf16_neighbours(v):
    """(next bf16 below, next above) of bf16 values held in float32."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.int64)
    mag, neg = u & 0x7FFFFFFF, (u >> 31).astype(bool)

    def step(up):
        away = up ^ neg  # moving away from zero grows the magnitude
        m = np.where(away, mag + 0x10000, mag - 0x10000)
        sign = np.where(neg, 0x80000000, 0)
        flip = m < 0  # crossing zero: the smallest value of the other sign
        m = np.where(flip, 0x10000, m)
        sign = np.where(flip, np.where(neg, 0, 0x80000000), sign)
        return (m | sign).astype(np.uint32).view(np.float32)

    return step(False), step(True)


# --------------------------------------------------- the inputs of the GPU tests, built once
YOLO_CONFIGS = (("f32", 3), ("f16", 3), ("bf16", 3), ("f32", 4))                   # dtype, na
YOLOV4_CONFIGS = (("f32", 1.0), ("f32", 1.05), ("bf16", 1.0), ("bf16", 1.05))      # dtype, scale_x_y
DET_SHAPES = {"two": DET_LEVELS, "wide": ((9, 10, 8),), "a16": ((2, 3, 8),)}       # name -> levels
RETINA_CONFIGS = (("f32", "two"), ("bf16", "two"), ("f32", "wide"), ("f32", "a16"))
FCOS_CONFIGS = (("f32", "two"), ("bf16", "two"), ("f32", "wide"))
GN_SHAPES = ((64, 8), (64, 4), (32, 8))   # (C, G): 8, 16 (scalar path), 4 (a vector spans two groups) per group
GN_HW = (5, 273)
GN_RATIOS = (0.0, 3.0, 30.0, 300.0)       # mean / std per group of the conditioning sweep


@functools.lru_cache(maxsize=None)
def yolo_case(dtype="f32", na=3) -> YoloCase:
    return make_yolo_case(dtype, na)


@functools.lru_cache(maxsize=None)
def yolov4_case(dtype="f32", sxy=1.0) -> Yolov4Case:
    return make_yolov4_case(dtype, sxy=sxy)


@functools.lru_cache(maxsize=None)
def retina_case(dtype="f32", shape="two") -> DetCase:
    lv = DET_SHAPES[shape]
    return make_retina_case(dtype, A=16 if shape == "a16" else 3, C=2 if shape == "a16" else 5, levels=lv,
                            img_hw=(lv[0][0] * lv[0][2], lv[0][1] * lv[0][2]))


@functools.lru_cache(maxsize=None)
def fcos_case(dtype="f32", shape="two") -> DetCase:
    lv = DET_SHAPES[shape]
    return make_fcos_case(dtype, levels=lv, img_hw=(lv[0][0] * lv[0][2], lv[0][1] * lv[0][2]))


@functools.lru_cache(maxsize=None)
def decoded_case(kind=0) -> DecodedCase:
    return make_decoded_case(kind, nc=37 if kind == 0 else 7)


def gn_params(C: int, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 1.5, C).astype(np.float32), rng.uniform(-0.2, 0.2, C).astype(np.float32))


def round_bf16(v) -> np.ndarray:
    """fp64 -> bf16 (nearest even, as float32) without the double rounding of a detour through
    fp32: the fp32 route's result is corrected against the exact midpoints to its neighbours."""
    v = np.asarray(v, np.float64)
    r = round_storage(v, "bf16")
    dn, up = bf16_neighbours(r)
    return np.where(v < (r.astype(np.float64) + dn) / 2, dn, np.where(v > (r.astype(np.float64) + up) / 2, up, r))


def gn_bf16_ok(got, ref: GnRef):
    """bf16 output rule → (ok, span).  The kernel rounds an fp32 value within ``ref.tol`` of the
    fp64 result y to bf16, and rounding is monotone, so ``got`` (bf16 values in float32) must
    lie in [bf16(y - tol), bf16(y + tol)].  ``span`` counts the bf16 steps of that interval: 0
    where ``got`` must equal bf16(y); 1 where one rounding tie lies within the fp32 bound of y
    and the result may be the neighbour on that side, by one bf16 ulp; more only where the
    output cancels (x near its group's mean, or the product against beta) to below about 2^9
    times the fp32 bound, so that a bf16 ulp of y is finer than the fp32 error of any
    evaluation, a two-pass one included."""
    lo, hi = round_bf16(ref.y - ref.tol), round_bf16(ref.y + ref.tol)
    got = np.asarray(got, np.float32)
    span = (ordered_key(hi).astype(np.int64) >> 16) - (ordered_key(lo).astype(np.int64) >> 16)
    return (got >= lo) & (got <= hi), span


def gn_cond_limit(HW: int, cg: int) -> float:
    """The conditioning mean^2 / var at which the one-pass variance's cancellation term,
    ``h (3 K + 5) (1 + mean^2 / var)`` relative on var and half of it on rstd, reaches half a bf16
    ulp (2^-9 relative) of the output: beyond it gn_stats_kernel would need a shifted or two-pass
    variance."""
    return 2.0 ** -8 / (HALF * (3 * gn_accumulation_factor(HW, cg) + 5)) - 1.0


GN_TOWER_COND_LIMIT = gn_cond_limit(100 * 168, 8)  # P3 of the default 800 x 1344 input, 8 channels per group
