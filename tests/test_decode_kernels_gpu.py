"""The LiDAR decode kernels entry point by entry point against the fp64 references of
ops/decode_ref.py: K11 ``tca_anchor_decode_filter`` (pixel-major and anchor-major kernels),
``tca_anchor_topk_threshold`` + ``tca_anchor_decode_filter_keyed`` (anchors.hip) and K12/K13
``tca_centerhead_decode`` (centerpoint.hip), called through ``_native.call`` with no
postprocess class, sort or NMS in between.

Every output buffer starts as a sentinel between two sentinel guards.  After each launch:
the guards are intact; no slot at or beyond min(count, cap) was written; slots below it hold
distinct anchor / pixel indices (``0xffffffff - low32(cand_key)``); the key's high word is
``ordered_key`` of the score the kernel wrote in that slot.  Candidates are aligned to the
reference by that index (slot order is not deterministic and is not asserted).

Membership is exact: the generators (ops/decode_ref.py, checked on the CPU by
tests/test_decode_ref.py) leave no score within twice the fp32 score bound of its threshold,
no dir-bin floor argument within 1e-3 of an integer and no centre within 1e-3 m of a range
face, so the kept index set must equal the reference's — no count slack.  Inputs are finite
and |logit| <= 12; NaN logits are out of scope.

Tolerances (per element, fp32 eps = 2^-23; none is tuned to what the kernels return; the
observed error / bound ratios are recorded in docs/precision.md):

* score: ``2^-23 (4 + |x|)`` relative, x the max logit — ``1 / (1 + __expf(-x))``, derived at
  the rescore test of tests/test_spconv_kernels_gpu.py.
* ``e*s + c`` terms (K11 x, y, z; CenterHead x, y): ``2^-23 (|e*s| + |c|)``.  The test geometry
  (anchor origin / stride, voxel size, out-size factor, range origin) is dyadic, so c and s are
  exact in fp32 and the roundings left are the ones this bound counts.
* ``exp`` dims: ``2^-23 (4 + |e|)`` relative (the score's ``__expf`` bound plus the product).
* K11 yaw: ``2^-23 (|e6| + |ra| + |dir_offset| + period (|floor| + dl))`` plus
  ``(|floor| + dl) |period32 - period|``, period32 the kernel's fp32 period (its pi literal
  and the quotient rounded to fp32).  Without a dir head: ``2^-23 (|e6| + |ra|)``.
* CenterHead yaw (``atan2f``): 4 ulp of pi = 2^-20 absolute.  This is an assumption: the HIP
  math accuracy tables are not part of the installed documentation.
* copied values (CenterHead z, vx, vy): bit-equal to the stored input.  Labels: equal.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from triton_client_amd.ops import decode_ref as R

GUARD = 64
I32_SENT = -1234567
F32_NAN = 0x7FC0ABCD
DT_CODE = {"f32": 0, "f16": 1, "bf16": 2}
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
PAD = 11.0  # every channel no head owns: a misread channel passes every threshold


class Buf:
    """Device output buffer of n elements between two sentinel guards (the body starts as the
    sentinel too unless ``fill`` is given); kind i32 / i64 / f32, as in test_spconv_kernels_gpu."""
    _DT = {"i32": torch.int32, "i64": torch.int64, "f32": torch.int32}
    _SENT = {"i32": I32_SENT, "i64": I32_SENT, "f32": F32_NAN}

    def __init__(self, dev, n, kind, fill=None):
        self.kind, self.n, self.sent = kind, int(n), self._SENT[kind]
        self.t = torch.full((self.n + 2 * GUARD,), self.sent, dtype=self._DT[kind], device=dev)
        if fill is not None:
            self.t[GUARD:GUARD + self.n] = fill
        self.ptr = self.t.data_ptr() + GUARD * self.t.element_size()

    def bits(self):
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == self.sent).all() and (a[GUARD + self.n:] == self.sent).all(), "guard overwritten"
        return a[GUARD:GUARD + self.n]


def _call(name, *args):
    from triton_client_amd import _native
    _native.call(name, *args, _native.stream_ptr())


def _farr(v):
    return (ctypes.c_float * len(v))(*[float(x) for x in v])


def _iarr(v):
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def _dev(a, dtype, dev):
    """Values already rounded to ``dtype``: the conversion is exact."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(TORCH_DT[dtype]).to(dev)


class Cand:
    """Guarded candidate buffers of S segments x cap slots x width box values."""

    def __init__(self, dev, S, cap, width):
        self.S, self.cap, self.width = S, cap, width
        self.box, self.score = Buf(dev, S * cap * width, "f32"), Buf(dev, S * cap, "f32")
        self.label, self.key, self.count = Buf(dev, S * cap, "i32"), Buf(dev, S * cap, "i64"), Buf(dev, S, "i32")

    def ptrs(self):
        return self.box.ptr, self.score.ptr, self.label.ptr, self.key.ptr, self.count.ptr

    def untouched(self):
        return all((b.bits() == b.sent).all() for b in (self.box, self.score, self.label, self.key, self.count))

    def read(self):
        """Per segment a dict of the written slots, aligned by recovered index, after the
        structural checks of the module docstring."""
        S, cap, w = self.S, self.cap, self.width
        box, score = self.box.bits().reshape(S, cap, w), self.score.bits().reshape(S, cap)
        label, key, count = self.label.bits().reshape(S, cap), self.key.bits().reshape(S, cap), self.count.bits()
        out = []
        for s in range(S):
            c = int(count[s])
            assert c >= 0
            n = min(c, cap)
            assert (box[s, n:] == F32_NAN).all() and (score[s, n:] == F32_NAN).all(), "slot beyond the count written"
            assert (label[s, n:] == I32_SENT).all() and (key[s, n:] == I32_SENT).all(), "slot beyond the count written"
            k = key[s, :n].view(np.uint64)
            idx = (np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF))).astype(np.int64)
            assert len(np.unique(idx)) == n, "duplicate or missing slot"
            sc = score[s, :n].view(np.float32)
            assert np.array_equal((k >> np.uint64(32)).astype(np.uint32), R.ordered_key(sc)), "key / score mismatch"
            o = np.argsort(idx)
            out.append({"count": c, "idx": idx[o], "score": sc[o], "label": label[s, :n][o],
                        "box": box[s, :n].view(np.float32)[o]})
        return out


RATIOS = {}


def _ratio(name, err, tol):
    if err.size:
        r = float((err / np.maximum(tol, 1e-300)).max())
        RATIOS[name] = max(RATIOS.get(name, 0.0), r)
        print(f"worst err / bound  {name}: {r:.3f}")


def _compare(tag, got, want_idx, cap, logit, score, label, box, tol, exact_cols=()):
    """One segment: ``want_idx`` the reference's kept indices (sorted); the per-index reference
    arrays are indexed by anchor / pixel."""
    assert got["count"] == len(want_idx), (tag, got["count"], len(want_idx))
    if got["count"] <= cap:
        assert np.array_equal(got["idx"], want_idx), tag
    else:
        assert len(got["idx"]) == cap and np.isin(got["idx"], want_idx).all(), tag
    i = got["idx"]
    assert np.array_equal(got["label"], label[i]), tag
    s = got["score"].astype(np.float64)
    err, bound = np.abs(s - score[i]), R.score_tol(logit[i], score[i])
    _ratio(tag + " score", err, bound)
    assert (err <= bound).all(), (tag, "score", float((err / bound).max()))
    b = got["box"].astype(np.float64)
    for q in range(box.shape[-1]):
        if q in exact_cols:
            assert np.array_equal(got["box"][:, q].view(np.uint32), box[i, q].astype(np.float32).view(np.uint32)), (tag, q)
            continue
        err = np.abs(b[:, q] - box[i, q])
        _ratio(f"{tag} box[{q}]", err, tol[i, q])
        assert (err <= tol[i, q]).all(), (tag, "box", q, float((err / tol[i, q]).max()))


# ------------------------------------------------------------------------------------- K11
LAYOUTS = ("nhwc_merged", "nhwc_offset", "nhwc_split", "nchw")


def _pack(case, layout, dev, use_dir=True):
    """→ (tensors to keep alive, cls ptr, box ptr, dir ptr, layout code, ld_cls, ld_box, ld_dir).
    nhwc_merged: one [B, H, W, ld] tensor, ld a multiple of 4, cls at channel 0 (16-B aligned:
    the pixel-major kernel for fp32 A=6 C=3).  nhwc_offset: the same with every head one channel
    further, which breaks the alignment.  nhwc_split: three tensors, each one to three channels
    wider than its head (ld_cls % 4 != 0).  nchw: three contiguous [B, ch, H, W] tensors."""
    B, H, W = case.shape
    heads = [case.cls, case.box] + ([case.dir] if case.dir is not None and use_dir else [])
    es = torch.empty((), dtype=TORCH_DT[case.dtype]).element_size()
    if layout in ("nhwc_merged", "nhwc_offset"):
        first = 1 if layout == "nhwc_offset" else 0
        need = first + sum(h.shape[-1] for h in heads)
        ld = (need + 3) // 4 * 4 + (4 if layout == "nhwc_offset" else 0)
        m = np.full((B, H, W, ld), PAD, np.float32)
        offs, o = [], first
        for h in heads:
            m[..., o:o + h.shape[-1]] = h
            offs.append(o)
            o += h.shape[-1]
        t = _dev(m, case.dtype, dev)
        ptrs = [t.data_ptr() + o * es for o in offs]
        if layout == "nhwc_merged":
            assert ptrs[0] % 16 == 0 and ld % 4 == 0
        else:
            assert ptrs[0] % 16 != 0 or case.dtype != "f32"
        keep, lds, code = [t], [ld] * 3, 1
    elif layout == "nhwc_split":
        keep, ptrs, lds, code = [], [], [], 1
        for h, extra in zip(heads, (1, 3, 1)):
            m = np.full((B, H, W, h.shape[-1] + extra), PAD, np.float32)
            m[..., :h.shape[-1]] = h
            t = _dev(m, case.dtype, dev)
            keep.append(t)
            ptrs.append(t.data_ptr())
            lds.append(m.shape[-1])
        assert lds[0] % 4 != 0
    else:
        keep = [_dev(h.transpose(0, 3, 1, 2), case.dtype, dev) for h in heads]
        ptrs, lds, code = [t.data_ptr() for t in keep], [0, 0, 0], 0
    if len(ptrs) == 2:
        ptrs.append(0)
        lds = lds[:2] + [0]
    return keep, ptrs[0], ptrs[1], ptrs[2], code, lds[0], lds[1], lds[2]


def _run_k11(dev, case, layout, cap, use_dir=True, bins=None, sel_ptr=None):
    B, H, W = case.shape
    keep, pc, pb, pd, code, lc, lb, ld = _pack(case, layout, dev, use_dir)
    cand = Cand(dev, B, cap, 7)
    A = case.A
    head = (pc, pb, pd, DT_CODE[case.dtype], code, B, H, W, A, case.C, case.bins if bins is None else bins, lc, lb, ld,
            _farr(case.table.reshape(-1)), *case.geom, case.dir_offset, case.dir_limit_offset)
    try:
        if sel_ptr is None:
            _call("tca_anchor_decode_filter", *head, float(case.score_thresh), *cand.ptrs(), cap)
        else:
            _call("tca_anchor_decode_filter_keyed", *head, sel_ptr, *cand.ptrs(), cap)
    finally:
        torch.cuda.synchronize()
    return cand


@functools.lru_cache(maxsize=None)
def _anchor(dtype="f32", A=6, C=3, dense=False):
    case = R.make_anchor_case(A, C, 2, dtype, dense=dense)
    ref = case.ref()
    assert R.anchor_band_counts(case, ref) == (0, 0)
    return case, ref, case.ref(use_dir=False)


def _check_k11(tag, cand, case, ref, keep=None):
    if keep is None:
        keep = ref.score >= np.float32(case.score_thresh)
    segs = cand.read()
    for b, got in enumerate(segs):
        _compare(f"{tag} frame {b}", got, np.flatnonzero(keep[b]), cand.cap, ref.logit[b], ref.score[b], ref.label[b],
                 ref.box[b], ref.tol[b])
    return segs


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout", [("f32", "nhwc_merged"), ("f32", "nhwc_offset"), ("f32", "nhwc_split"),
                                          ("f32", "nchw"), ("f16", "nhwc_merged"), ("f16", "nchw"),
                                          ("bf16", "nhwc_merged"), ("bf16", "nchw")])
def test_anchor_decode_filter(cuda, dtype, layout):
    """37 x 41 x 6 anchors, batch 3 (frame 1 empty): the pixel-major kernel (fp32 nhwc_merged:
    6 blocks, ragged last) and the anchor-major one (3 blocks, ragged tail) in every layout
    and storage type; class ties (64 forced, many more in bf16) resolve to the lower class."""
    case, ref, _ = _anchor(dtype)
    B, H, W = case.shape
    segs = _check_k11(f"K11 {dtype} {layout}", _run_k11(cuda, case, layout, H * W * case.A + 7), case, ref)
    assert segs[1]["count"] == 0 and segs[0]["count"] > 500 and segs[2]["count"] > 500


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [False, True])
def test_pixel_major_and_anchor_major_kernels_agree_bitwise(cuda, dense):
    case, ref, _ = _anchor("f32", dense=dense)
    cap = 37 * 41 * 6
    px = _run_k11(cuda, case, "nhwc_merged", cap).read()
    for other in ("nhwc_offset", "nhwc_split", "nchw"):
        an = _run_k11(cuda, case, other, cap).read()
        for g, h in zip(px, an):
            assert g["count"] == h["count"] and np.array_equal(g["idx"], h["idx"])
            assert np.array_equal(g["label"], h["label"])
            assert np.array_equal(g["score"].view(np.uint32), h["score"].view(np.uint32))
            assert np.array_equal(g["box"].view(np.uint32), h["box"].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("A,C,layout", [(2, 1, "nchw"), (2, 1, "nhwc_split"), (8, 5, "nhwc_merged"), (8, 5, "nchw")])
def test_anchor_decode_other_head_shapes(cuda, A, C, layout):
    case, ref, _ = _anchor("f32", A, C)
    _check_k11(f"K11 A={A} C={C} {layout}", _run_k11(cuda, case, layout, 37 * 41 * A), case, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["null_dir", "zero_bins"])
@pytest.mark.parametrize("layout", ["nhwc_merged", "nchw"])
def test_anchor_decode_without_dir_head_returns_raw_angle(cuda, layout, how):
    case, _, raw = _anchor("f32")
    cand = _run_k11(cuda, case, layout, 37 * 41 * 6, use_dir=how != "null_dir", bins=0 if how == "zero_bins" else None)
    _check_k11(f"K11 {how} {layout}", cand, case, raw)


@pytest.mark.gpu
def test_anchor_decode_refuses_nine_anchors(cuda):
    from triton_client_amd._native import NativeError
    case, _, _ = _anchor("f32")
    B, H, W = case.shape
    nine = R.AnchorCase("f32", 9, 2, 2, case.cls, np.concatenate([case.box] * 2, -1)[..., :63],
                        np.concatenate([case.dir] * 2, -1)[..., :18], R.anchor_table(9), case.geom, case.dir_offset,
                        case.dir_limit_offset, 0.0)
    assert nine.cls.shape[-1] == 18
    keep, pc, pb, pd, code, lc, lb, ld = _pack(nine, "nchw", cuda)
    cand = Cand(cuda, B, 64, 7)
    with pytest.raises(NativeError):
        _call("tca_anchor_decode_filter", pc, pb, pd, 0, code, B, H, W, 9, 2, 2, lc, lb, ld, _farr(nine.table.reshape(-1)),
              *nine.geom, nine.dir_offset, nine.dir_limit_offset, 0.0, *cand.ptrs(), 64)
    torch.cuda.synchronize()
    assert cand.untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["nhwc_merged", "nchw"])
def test_anchor_threshold_tie_is_kept(cuda, layout):
    """Max logit exactly 0 with score_thresh exactly 0.5: K11 keeps ``score >= thr``
    (OpenPCDet).  Rests on the device's exp(0) being exactly 1."""
    case = R.make_tie_anchor_case()
    ref = case.ref()
    B, H, W = case.shape
    even = np.arange(H * W * 6) % 2 == 0
    segs = _run_k11(cuda, case, layout, H * W * 6).read()
    got = segs[0]
    assert np.array_equal(got["idx"], np.flatnonzero(even)), ("cand_score held", np.unique(got["score"]))
    assert (got["score"] == np.float32(0.5)).all(), np.unique(got["score"])
    _check_k11(f"K11 tie {layout}", _run_k11(cuda, case, layout, H * W * 6), case, ref, keep=even[None])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["nhwc_merged", "nhwc_offset"])
def test_anchor_decode_dense_block(cuda, layout):
    """All of frame 0's first 4096 anchors pass: in the anchor-major kernel more than 2048
    take global slots one by one; the pixel-major kernel's stage holds its whole block."""
    case, ref, _ = _anchor("f32", dense=True)
    segs = _check_k11(f"K11 dense {layout}", _run_k11(cuda, case, layout, 37 * 41 * 6), case, ref)
    assert (segs[0]["idx"] < 4096).sum() == 4096


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["nhwc_merged", "nhwc_offset"])
@pytest.mark.parametrize("dense", [False, True])
def test_anchor_decode_cap_overflow(cuda, layout, dense):
    """cap below the passing count: the count is still the true one, the first cap slots are
    distinct correct members of the reference set, nothing lands beyond cap."""
    case, ref, _ = _anchor("f32", dense=dense)
    cap = 777
    segs = _check_k11(f"K11 overflow {layout}", _run_k11(cuda, case, layout, cap), case, ref)
    assert segs[0]["count"] > cap and len(segs[0]["idx"]) == cap and segs[1]["count"] == 0


# ------------------------------------------------------------------------- top-k threshold
TOTAL = 37 * 41 * 6


def _topk_case(kind, dtype, k):
    base = R.make_anchor_case(6, 3, 2, dtype, seed=11, B=2)  # box / dir heads: floor band clear on every anchor
    case = R.AnchorCase(dtype, 6, 3, 2, R.make_topk_cls(kind, dtype, k=k), base.box, base.dir, base.table, base.geom,
                        base.dir_offset, base.dir_limit_offset, 0.0)
    ref = case.ref()
    assert R.anchor_band_counts(case, ref)[1] == 0
    return case, ref


def _topk_threshold(dev, case, layout, k, hist, sel):
    keep, pc, _, _, code, lc, _, _ = _pack(case, layout, dev)
    B, H, W = case.shape
    _call("tca_anchor_topk_threshold", pc, DT_CODE[case.dtype], code, B, H, W, case.A, case.C, lc, k, hist.ptr, sel.ptr)
    torch.cuda.synchronize()
    assert (hist.bits() == 0).all(), "histogram not reset"
    return sel.bits().view(np.uint32).reshape(B, 2)[:, 1].astype(np.int64)


def _check_topk(tag, dev, case, ref, layout, k, hist):
    B = case.shape[0]
    sel = Buf(dev, B * 2, "i32")
    thr = _topk_threshold(dev, case, layout, k, hist, sel)
    keys = R.max_logit_keys(case.cls, case.A, case.C)
    assert np.array_equal(keys, R.ordered_key(ref.logit.astype(np.float32)))
    for b in range(B):
        enough, tight = R.topk_threshold_ok(keys[b], thr[b], k)
        n_ge = int((keys[b].astype(np.int64) >= thr[b]).sum())
        assert enough, (tag, b, "thr", hex(thr[b]), "admits", n_ge, "of k", k)
        assert tight, (tag, b, "thr", hex(thr[b]), "admits above the next bucket",
                       int((keys[b].astype(np.int64) >= thr[b] + 256).sum()))
        if k > TOTAL:
            assert thr[b] == 0
    cand = _run_k11(dev, case, layout, TOTAL, sel_ptr=sel.ptr)
    _check_k11(tag, cand, case, ref, keep=keys.astype(np.int64) >= thr[:, None])
    return thr


TOPK_CASES = ([(kind, "f32", k) for kind in ("spread", "equal", "tie_straddle", "narrow")
               for k in (1, 64, 1024, TOTAL, TOTAL + 1)]
              + [("signed_zero", "f32", 170), ("signed_zero", "f32", 120)]
              + [(kind, dt, 1024) for kind in ("spread", "narrow", "tie_straddle") for dt in ("f16", "bf16")])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,dtype,k", TOPK_CASES)
def test_topk_threshold_and_keyed_decode(cuda, kind, dtype, k):
    """sel[b][1] admits the top k and at most one further 256-key bucket; the keyed decode's
    candidate set is exactly {key >= thr} with K11's values.  fp32 runs NHWC (ld 72), the
    16-bit types NCHW."""
    case, ref = _topk_case(kind, dtype, k)
    hist = Buf(cuda, 2 * 4096, "i32", fill=0)
    _check_topk(f"topk {kind} {dtype} k={k}", cuda, case, ref, "nhwc_merged" if dtype == "f32" else "nchw", k, hist)


@pytest.mark.gpu
def test_topk_histogram_resets_itself(cuda):
    """Two selections in a row on different data through one histogram buffer."""
    hist = Buf(cuda, 2 * 4096, "i32", fill=0)
    first = _check_topk("topk reuse 1", cuda, *_topk_case("spread", "f32", 64), "nchw", 64, hist)
    second = _check_topk("topk reuse 2", cuda, *_topk_case("narrow", "f32", 1024), "nchw", 1024, hist)
    assert (first != second).all()


# ------------------------------------------------------------------------------ CenterHead
@functools.lru_cache(maxsize=None)
def _center(dtype, ldc):
    from triton_client_amd.ops.centerpoint import NUSC_CLASS_THRESH
    return R.center_case(dtype, ldc, NUSC_CLASS_THRESH)


def _thresholds(name):
    from triton_client_amd.ops.centerpoint import NUSC_CLASS_THRESH
    return R.center_thresholds(name, NUSC_CLASS_THRESH)


def _run_center(dev, case, cls_thresh, score_thresh, cap, ntask=None, ncls=None):
    B, H, W, ldc = case.head.shape
    T = len(case.task_info) if ntask is None else ntask
    head = _dev(case.head, case.dtype, dev)
    cand = Cand(dev, B * T, cap, 9)
    info = [v for row in case.task_info for v in row]
    info = (info * 3)[:3 * T]
    ct = _farr(cls_thresh) if cls_thresh is not None else None
    n = (len(cls_thresh) if cls_thresh is not None else 0) if ncls is None else ncls
    try:
        _call("tca_centerhead_decode", head.data_ptr(), DT_CODE[case.dtype], ldc, B, H, W, T, _iarr(info), ct, n,
              float(score_thresh), _farr(case.range), _farr(case.vsize), case.osf, _farr(case.pcr), *cand.ptrs(), cap)
    finally:
        torch.cuda.synchronize()
    return cand


def _check_center(tag, cand, case, ref):
    B, T = ref.keep.shape[:2]
    segs = cand.read()
    for b in range(B):
        for t in range(T):
            _compare(f"{tag}", segs[b * T + t], np.flatnonzero(ref.keep[b, t]), cand.cap, ref.logit[b, t],
                     ref.score[b, t], ref.label[b, t], ref.box[b, t], ref.tol[b, t], exact_cols=(2, 7, 8))
    return segs


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,ldc,thresh", [("f32", 96, "nusc+0.1"), ("f32", 96, "nusc+0.2"), ("f32", 96, "none+0.1"),
                                              ("f32", 104, "nusc+0.1"), ("f16", 96, "nusc+0.1"),
                                              ("bf16", 96, "nusc+0.1")])
def test_centerhead_decode(cuda, dtype, ldc, thresh):
    """19 x 23 pixels (two blocks, a 53-lane last wave), six tasks at channel offsets 16 t,
    batch 2: exact per-segment sets under the per-class thresholds (strictly above
    max(score_thresh, cls_thresh[label]); a null table falls back to score_thresh) and the
    post-centre-range filter; labels tcls0[t] + first argmax; box values within the bounds."""
    case = _center(dtype, ldc)
    ct, st = _thresholds(thresh)
    ref = case.ref(ct, st)
    assert R.center_band_counts(ref) == (0, 0)
    segs = _check_center(f"CenterHead {dtype} ldc={ldc} {thresh}", _run_center(cuda, case, ct, st, 19 * 23 + 5), case, ref)
    assert segs[6 + 3]["count"] == 0  # frame 1 task 3
    idx = segs[0]["idx"]  # frame 0 task 0: a silent wave beside a full one
    assert not ((idx >= 64) & (idx < 128)).any() and ((idx >= 128) & (idx < 192)).sum() == 64
    for f, (b, t, p) in enumerate(case.face_pixels):  # above the threshold, beyond face f only
        assert p not in segs[b * 6 + t]["idx"]


@pytest.mark.gpu
def test_centerhead_decode_cap_overflow(cuda):
    case = _center("f32", 96)
    ct, st = _thresholds("none+0.1")
    ref = case.ref(ct, st)
    cap = 50
    segs = _check_center("CenterHead overflow", _run_center(cuda, case, ct, st, cap), case, ref)
    assert sum(s["count"] > cap for s in segs) >= 10 and segs[9]["count"] == 0


@pytest.mark.gpu
def test_centerhead_threshold_tie_is_dropped(cuda):
    """Heatmap logit exactly 0 with score_thresh exactly 0.5: CenterHead keeps ``score > thr``
    (det3d), so the tie is dropped.  Rests on the device's exp(0) being exactly 1."""
    case = R.make_tie_center_case()
    ref = case.ref(None, 0.5)
    assert not ref.keep.any()
    got = _run_center(cuda, case, None, 0.5, 35).read()[0]
    assert got["count"] == 0, ("cand_score held", np.unique(got["score"]))
    # the same input just below the tie keeps exactly the even pixels
    ref = case.ref(None, 0.4999)
    assert ref.keep.sum() == 18 and R.center_band_counts(ref) == (0, 0)
    _check_center("CenterHead tie", _run_center(cuda, case, None, 0.4999, 35), case, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("ntask,ncls", [(9, 10), (6, 33)])
def test_centerhead_decode_refuses_too_many_tasks_or_classes(cuda, ntask, ncls):
    from triton_client_amd._native import NativeError
    case = _center("f32", 96)
    B, H, W, ldc = case.head.shape
    head = _dev(case.head, "f32", cuda)
    cand = Cand(cuda, B * ntask, 16, 9)
    info = ([v for row in case.task_info for v in row] * 3)[:3 * ntask]
    with pytest.raises(NativeError):
        _call("tca_centerhead_decode", head.data_ptr(), 0, ldc, B, H, W, ntask, _iarr(info), _farr([0.1] * 33), ncls,
              0.1, _farr(case.range), _farr(case.vsize), case.osf, _farr(case.pcr), *cand.ptrs(), 16)
    torch.cuda.synchronize()
    assert cand.untouched()
