"""The camera decode kernels entry point by entry point against the fp64 references of
ops/camera_decode_ref.py: ``tca_yolo_decode_filter`` (K3: single-label, multi-label, class
mask, ``decoded`` output), ``tca_yolo_decode``, ``tca_yolo_filter_decoded`` (kind 0 / 1),
``tca_yolov4_decode`` (yolo.hip) and ``tca_retina_decode``, ``tca_fcos_decode``,
``tca_segment_merge``, ``tca_group_norm_nhwc_dt`` (detectron.hip), called through
``_native.call`` with no postprocess class, sort or NMS in between.

The structure is that of tests/test_decode_kernels_gpu.py, whose guarded buffers are reused:
every output starts as a sentinel between sentinel guards; after each launch the guards are
intact, no slot at or beyond min(count, cap) was written, the written slots hold distinct
identities (``0xffffffff - low32(cand_key)``) and the key's high word is ``ordered_key`` of the
score in that slot.  Candidates are aligned to the reference by identity.  Membership is exact:
the generators (checked on the CPU by tests/test_camera_decode_ref.py, re-asserted here) leave
nothing inside a band of twice the applicable bound around any threshold, clip edge or clamp,
so count and kept set must equal the reference's — no slack.  With ``cap`` below the count,
the count is still the full one, exactly ``cap`` slots are written, each a distinct member of
the reference set with its values; which members land is not asserted.

Tolerances are the formulas of ops/camera_decode_ref.py's docstring (fp32 eps, operand
magnitudes, the ``2^-23 (4 + |x|)`` sigmoid bound), none tuned to what the kernels return;
copies, classes and the merged segments are compared bit for bit.  GroupNorm is held to the
bound of ``group_norm``'s docstring, which grows with the conditioning mean^2 / var as the
one-pass variance's cancellation does; in bf16 storage the result is the fp64 value rounded to
bf16, or its neighbour where a rounding tie lies within that bound (``gn_bf16_ok``: outputs
that cancel to below about 2^9 bounds, where a bf16 ulp is finer than any fp32 evaluation's
error, are held to the bound itself).  The observed error /
bound ratios are printed (run with ``-s``) and recorded in docs/precision.md.  Inputs are
finite with |logit| <= 12; NaN / Inf logits are out of scope.
"""
import functools

import numpy as np
import pytest
import torch

from test_decode_kernels_gpu import DT_CODE, F32_NAN, GUARD, I32_SENT, PAD, TORCH_DT, Buf, Cand, _call, _dev, _farr, _iarr
from triton_client_amd.ops import camera_decode_ref as R

RATIOS = {}


def _ratio(name, err, tol):
    if err.size:
        r = float((err / np.maximum(tol, 1e-300)).max())
        RATIOS[name] = max(RATIOS.get(name, 0.0), r)
        print(f"worst err / bound  {name}: {r:.3f}")


def _within(tag, name, got, want, tol):
    err = np.abs(np.asarray(got, np.float64) - want)
    _ratio(f"{tag.split()[0]} {name}", err, tol)
    assert (err <= tol).all(), (tag, name, float((err / np.maximum(tol, 1e-300)).max()))


def _compare(tag, got, cap, keep, score, tol, cls, row, box, box_tol):
    """One segment against the reference arrays indexed by identity (``row`` maps an identity to
    its box)."""
    want = np.flatnonzero(keep)
    assert got["count"] == len(want), (tag, got["count"], len(want))
    if len(want) <= cap:
        assert np.array_equal(got["idx"], want), tag
    else:
        assert len(got["idx"]) == cap and np.isin(got["idx"], want).all(), tag
    i = got["idx"]
    assert np.array_equal(got["label"], cls[i]), tag
    _within(tag, "score", got["score"], score[i], tol[i])
    _within(tag, "box", got["box"], box[row[i]], box_tol[row[i]])


def _nhwc(h, ld, dtype, dev):
    """[B, H, W, C] logical head inside a wider channel stride; the pad passes every threshold."""
    m = np.full(h.shape[:3] + (ld,), PAD, np.float32)
    m[..., :h.shape[3]] = h
    return _dev(m, dtype, dev)


def _sync_call(name, *args):
    try:
        _call(name, *args)
    finally:
        torch.cuda.synchronize()


def _refused(name, *args):
    from triton_client_amd._native import NativeError
    with pytest.raises(NativeError):
        _call(name, *args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ K3 / decode
def _yolo_heads(case, layout, dev):
    no = case.na * (case.nc + 5)
    if layout == "nchw":
        keep = [_dev(h.transpose(0, 3, 1, 2), case.dtype, dev) for h in case.heads]
        return keep, 0, None
    lds = [no + 3, no + 8, no + 1]
    return [_nhwc(h, ld, case.dtype, dev) for h, ld in zip(case.heads, lds)], 1, _iarr(lds)


def _yolo_args(case, layout, dev, na=None):
    keep, code, ldc = _yolo_heads(case, layout, dev)
    B = case.heads[0].shape[0]
    na = na or case.na
    anchors = case.anchors.reshape(-1) if na == case.na else np.resize(case.anchors.reshape(-1), 3 * na * 2)
    return keep, (*[t.data_ptr() for t in keep], DT_CODE[case.dtype], code, B, na, case.nc,
                  _iarr([v for hw in case.levels for v in hw]), _iarr(case.strides), ldc, _farr(anchors))


def _mask(case, dev):
    return torch.from_numpy(R.class_mask_words(case.nc, case.classes).view(np.int32)).to(dev)


def _run_k3(dev, case, layout, multi_label, masked, cap, decoded=None):
    keep, head = _yolo_args(case, layout, dev)
    B = case.heads[0].shape[0]
    cand = Cand(dev, B, cap, 4)
    mask = _mask(case, dev) if masked else None
    _sync_call("tca_yolo_decode_filter", *head, float(case.conf), int(multi_label), mask.data_ptr() if masked else None,
               *cand.ptrs(), cap, decoded.ptr if decoded is not None else None)
    return cand


def _check_k3(tag, cand, case, ref, multi_label, masked):
    f = R.yolo_filter(ref, case.conf, multi_label, case.classes if masked else None)
    assert f.band_counts() == (0, 0)
    segs = cand.read()
    for b, got in enumerate(segs):
        _compare(tag, got, cand.cap, f.keep[b], f.score[b], f.tol[b], f.cls[b], f.row, ref.box[b], ref.box_tol[b])
    return segs, f


@pytest.mark.gpu
@pytest.mark.parametrize("multi_label,masked", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype,na", R.YOLO_CONFIGS)
def test_k3_decode_filter(cuda, dtype, na, layout, multi_label, masked):
    """Levels (12, 9), (6, 5), (3, 3): 441 rows at na = 3 — two blocks, a ragged tail, level
    boundaries inside a block and inside a wave; nc = 37 (the class mask spans two words);
    NCHW, and NHWC with ldc > na (5 + nc) whose pad channels would pass every threshold.  With
    the mask, the rows whose best class is filtered while a lower allowed class passes are
    dropped, not promoted."""
    case = R.yolo_case(dtype, na)
    ref = case.ref()
    cap = case.N * (case.nc if multi_label else 1) + 7
    mode = ("multi" if multi_label else "single") + ("+mask" if masked else "")
    segs, f = _check_k3(f"K3 {dtype} na={na} {layout} {mode}", _run_k3(cuda, case, layout, multi_label, masked, cap), case,
                        ref, multi_label, masked)
    assert segs[0]["count"] > 100
    if masked and not multi_label:
        assert len(case.masked_rows) > 20 and not np.isin(case.masked_rows, segs[0]["idx"]).any()


@pytest.mark.gpu
def test_k3_refuses_five_anchors(cuda):
    case = R.yolo_case("f32", 3)
    keep, head = _yolo_args(case, "nchw", cuda, na=5)
    cand = Cand(cuda, 1, 64, 4)
    dec = Buf(cuda, 64, "f32")
    _refused("tca_yolo_decode_filter", *head, 0.25, 0, None, *cand.ptrs(), 64, None)
    _refused("tca_yolo_decode", *head, dec.ptr)
    assert cand.untouched() and (dec.bits() == F32_NAN).all()


@functools.lru_cache(maxsize=None)
def _yolo_batch2():
    case = R.make_yolo_case("f32", B=2, seed=1)
    assert R.yolo_filter(case.ref(), case.conf, True).band_counts() == (0, 0)
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype,batch", [("f32", 1), ("f16", 1), ("bf16", 1), ("f32", 2)])
def test_yolo_decode_and_k3_decoded_output(cuda, dtype, batch, layout):
    """``tca_yolo_decode`` and K3's ``decoded`` output: every element of every row, rows below
    the threshold included, within the bounds of fp64 and the two bit-equal; guards sit right
    after the last element (batch 1: 18522 floats, a 2-float scalar tail; batch 2: a multiple
    of 4).  K3's candidates are unchanged by the extra output."""
    case = R.yolo_case(dtype, 3) if batch == 1 else _yolo_batch2()
    ref = case.ref()
    n = batch * case.N * (case.nc + 5)
    assert n % 4 == (2 if batch == 1 else 0)
    keep, head = _yolo_args(case, layout, cuda)
    dec = Buf(cuda, n, "f32")
    assert dec.ptr % 16 == 0
    _sync_call("tca_yolo_decode", *head, dec.ptr)
    got = dec.bits().view(np.float32).reshape(ref.dec.shape)
    tag = f"decode {dtype} {layout}"
    _within(tag, "xy", got[..., :2], ref.dec[..., :2], ref.dec_tol[..., :2])
    _within(tag, "wh", got[..., 2:4], ref.dec[..., 2:4], ref.dec_tol[..., 2:4])
    _within(tag, "obj/cls", got[..., 4:], ref.dec[..., 4:], ref.dec_tol[..., 4:])
    dec3 = Buf(cuda, n, "f32")
    cand = _run_k3(cuda, case, layout, False, False, case.N, decoded=dec3)
    assert np.array_equal(dec3.bits(), dec.bits())
    _check_k3(f"K3 decoded {dtype} {layout}", cand, case, ref, False, False)


@pytest.mark.gpu
def test_yolo_decode_refuses_a_misaligned_output(cuda):
    case = R.yolo_case("f32", 3)
    keep, head = _yolo_args(case, "nchw", cuda)
    dec = Buf(cuda, case.N * (case.nc + 5) + 4, "f32")
    _refused("tca_yolo_decode", *head, dec.ptr + 4)
    assert (dec.bits() == F32_NAN).all()


@pytest.mark.gpu
@pytest.mark.parametrize("multi_label,cap", [(False, 50), (True, 300)])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_k3_cap_overflow(cuda, layout, multi_label, cap):
    case = R.yolo_case("f32", 3)
    segs, f = _check_k3(f"K3 overflow {layout}", _run_k3(cuda, case, layout, multi_label, False, cap), case, case.ref(),
                        multi_label, False)
    assert segs[0]["count"] > cap and len(segs[0]["idx"]) == cap


# ---------------------------------------------------------------------------- filter_decoded
def _run_filter_decoded(dev, case, multi_label, masked, cap):
    pred = torch.from_numpy(case.pred).to(dev)
    confs = torch.from_numpy(case.confs).to(dev) if case.confs is not None else None
    B, N, ld = case.pred.shape
    cand = Cand(dev, B, cap, 4)
    mask = torch.from_numpy(R.class_mask_words(case.nc, R.YOLO_CLASSES).view(np.int32)).to(dev) if masked else None
    _sync_call("tca_yolo_filter_decoded", pred.data_ptr(), confs.data_ptr() if confs is not None else None, case.kind, B, N,
               ld, case.nc, float(case.conf), int(multi_label), mask.data_ptr() if masked else None,
               float(case.img_wh[0]), float(case.img_wh[1]), *cand.ptrs(), cap)
    return cand


@pytest.mark.gpu
@pytest.mark.parametrize("kind,multi_label,masked", [(0, False, False), (0, False, True), (0, True, False), (0, True, True),
                                                     (1, False, False)])
def test_filter_decoded(cuda, kind, multi_label, masked):
    """N = 300 rows (two blocks, ragged), batch 2.  Kind 0: rows of ld = nc + 8 floats whose pad
    columns would pass; scores are one fp32 product.  Kind 1: scores are copies, boxes scaled
    by img_w != img_h."""
    case = R.decoded_case(kind)
    f, box, box_tol = R.filter_decoded(case, multi_label, R.YOLO_CLASSES if masked else None)
    assert f.band_counts() == (0, 0) and R.decoded_gap_count(case) == 0
    N = case.pred.shape[1]
    cap = N * (case.nc if multi_label else 1) + 3
    tag = f"filter_decoded kind={kind} multi={multi_label} mask={masked}"
    for b, got in enumerate(_run_filter_decoded(cuda, case, multi_label, masked, cap).read()):
        _compare(tag, got, cap, f.keep[b], f.score[b], f.tol[b], f.cls[b], f.row, box[b], box_tol[b])
        if kind == 1:  # copies
            assert np.array_equal(got["score"], case.confs[b].max(-1)[got["idx"]])
        assert got["count"] > 100


@pytest.mark.gpu
def test_filter_decoded_refused_arguments(cuda):
    case = R.decoded_case(0)
    pred = torch.from_numpy(case.pred).to(cuda)
    B, N, ld = case.pred.shape
    cand = Cand(cuda, B, 16, 4)
    for kind, n, ldx, nc, confs in ((0, N, case.nc + 4, case.nc, None), (1, N, 4, case.nc, None), (2, N, ld, case.nc, None),
                                    (-1, N, ld, case.nc, None), (0, 0, ld, case.nc, None), (0, N, ld, 0, None)):
        _refused("tca_yolo_filter_decoded", pred.data_ptr(), confs, kind, B, n, ldx, nc, 0.25, 0, None, 0.0, 0.0,
                 *cand.ptrs(), 16)
    assert cand.untouched()


# ------------------------------------------------------------------------------------ YOLOv4
def _run_yolov4(dev, case, cap, full=True):
    no = 3 * (case.nc + 5)
    lds = [no + 4, no + 1, no + 7]
    keep = [_nhwc(h, ld, case.dtype, dev) for h, ld in zip(case.heads, lds)]
    B = case.heads[0].shape[0]
    N = sum(3 * h * w for h, w in case.levels)
    cand = Cand(dev, B, cap, 4)
    ob, oc = Buf(dev, B * N * 4, "f32"), Buf(dev, B * N * case.nc, "f32")
    _sync_call("tca_yolov4_decode", *[t.data_ptr() for t in keep], DT_CODE[case.dtype], B, case.nc,
               _iarr([v for hw in case.levels for v in hw]), _iarr(lds), _farr(case.anchors.reshape(-1)), float(case.sxy),
               float(case.conf), case.img_hw[0], case.img_hw[1], ob.ptr if full else None, oc.ptr if full else None,
               *cand.ptrs(), cap)
    return cand, ob, oc


def _check_yolov4(tag, cand, case, ref):
    f = ref.filt
    assert f.band_counts() == (0, 0)
    segs = cand.read()
    for b, got in enumerate(segs):
        _compare(tag, got, cand.cap, f.keep[b], f.score[b], f.tol[b], f.cls[b], f.row, ref.cand[b], ref.cand_tol[b])
    return segs


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,sxy", R.YOLOV4_CONFIGS)
def test_yolov4_decode(cuda, dtype, sxy):
    """The K3 levels (H != W on two of them), nc = 7, padded ldc, img_h != img_w: the full
    ``boxes`` / ``confs`` outputs element by element and the candidates by row."""
    case = R.yolov4_case(dtype, sxy)
    ref = case.ref()
    N = ref.boxes.shape[1]
    cand, ob, oc = _run_yolov4(cuda, case, N + 5)
    tag = f"YOLOv4 {dtype} sxy={sxy}"
    segs = _check_yolov4(tag, cand, case, ref)
    assert min(s["count"] for s in segs) > 100
    _within(tag, "boxes", ob.bits().view(np.float32).reshape(ref.boxes.shape), ref.boxes, ref.boxes_tol)
    _within(tag, "confs", oc.bits().view(np.float32).reshape(ref.confs.shape), ref.confs, ref.confs_tol)


@pytest.mark.gpu
def test_yolov4_cap_overflow_without_full_outputs(cuda):
    case = R.yolov4_case("f32", 1.05)
    cand, ob, oc = _run_yolov4(cuda, case, 40, full=False)
    segs = _check_yolov4("YOLOv4 overflow", cand, case, case.ref())
    assert all(s["count"] > 40 and len(s["idx"]) == 40 for s in segs)
    assert (ob.bits() == F32_NAN).all() and (oc.bits() == F32_NAN).all()


# ----------------------------------------------------------------------------- retina / FCOS
def _run_det(dev, case, cap, A=None, levels=None, zero=None):
    B = case.levels[0].cls.shape[0]
    L = len(case.levels)
    cand = Cand(dev, B * L, cap, 4)
    keep = []
    for l in (range(L) if levels is None else levels):
        lv = case.levels[l]
        z = int(l == 0) if zero is None else zero
        cls = _nhwc(lv.cls, lv.cls.shape[3] + 3, case.dtype, dev)
        box = _nhwc(lv.box, lv.box.shape[3] + 2, case.dtype, dev)
        keep += [cls, box]
        if case.arch == "retinanet":
            _sync_call("tca_retina_decode", cls.data_ptr(), box.data_ptr(), DT_CODE[case.dtype], B, lv.H, lv.W, A or case.A,
                       case.C, cls.shape[3], box.shape[3], lv.stride, _farr(np.resize(lv.anchors.reshape(-1), 2 * (A or case.A))),
                       float(case.thresh), float(case.scale_clamp), float(case.img_hw[0]), float(case.img_hw[1]), l, L,
                       *cand.ptrs(), cap, z)
        else:
            ctr = _nhwc(lv.ctr[..., None], 3, case.dtype, dev)
            keep.append(ctr)
            _sync_call("tca_fcos_decode", cls.data_ptr(), box.data_ptr(), ctr.data_ptr(), DT_CODE[case.dtype], B, lv.H, lv.W,
                       case.C, cls.shape[3], box.shape[3], 3, lv.stride, float(case.thresh), float(case.img_hw[0]),
                       float(case.img_hw[1]), l, L, *cand.ptrs(), cap, z)
    return cand


def _check_det(tag, cand, case):
    B, L = case.levels[0].cls.shape[0], len(case.levels)
    segs = cand.read()
    for l in range(L):
        ref = case.ref(l)
        assert not any(ref.bands), ref.bands
        for b in range(B):
            _compare(f"{tag} level {l}", segs[b * L + l], cand.cap, ref.keep[b], ref.score[b], ref.tol[b], ref.cls,
                     ref.row, ref.box[b], ref.box_tol[b])
    return segs


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,shape", R.RETINA_CONFIGS)
def test_retina_decode(cuda, dtype, shape):
    """two: levels (7, 9) stride 8 and (4, 5) stride 16 with A = 3, C = 5 (189 threads: below a
    block; 60: below a wave), the second launched with zero_counts = 0 onto the first's counts;
    wide: 270 threads, just over a block; a16: the largest anchor count accepted.  ld_cls > A C,
    ld_box > 4 A; several classes per anchor; boxes clipped on each side and deltas beyond
    scale_clamp (placed by the generator, asserted by tests/test_camera_decode_ref.py)."""
    case = R.retina_case(dtype, shape)
    segs = _check_det(f"retina {dtype} {shape}", _run_det(cuda, case, 400), case)
    if shape == "two":
        for name, (l, b, r) in case.placed.items():
            assert r * case.C in segs[b * len(case.levels) + l]["idx"], name


@pytest.mark.gpu
def test_retina_refuses_seventeen_anchors_and_keeps_counts_without_zeroing(cuda):
    case = R.retina_case("f32", "a16")
    cand = Cand(cuda, 2, 400, 4)
    lv = case.levels[0]
    cls, box = _nhwc(lv.cls, 40, "f32", cuda), _nhwc(lv.box, 72, "f32", cuda)
    _refused("tca_retina_decode", cls.data_ptr(), box.data_ptr(), 0, 2, lv.H, lv.W, 17, case.C, 40, 72, lv.stride,
             _farr(np.resize(lv.anchors.reshape(-1), 34)), 0.25, 0.75, 16.0, 24.0, 0, 1, *cand.ptrs(), 400, 1)
    assert cand.untouched()
    # zero_counts = 0 twice on the "two" case's second level alone: its segments' counts double,
    # the first level's segments stay as they were
    case = R.retina_case("f32", "two")
    once = _run_det(cuda, case, 400)
    base = once.count.bits().copy()
    twice = _run_det(cuda, case, 400)
    B, L = 2, 2
    lv = case.levels[1]
    cls, box = _nhwc(lv.cls, lv.cls.shape[3] + 3, "f32", cuda), _nhwc(lv.box, lv.box.shape[3] + 2, "f32", cuda)
    _sync_call("tca_retina_decode", cls.data_ptr(), box.data_ptr(), 0, B, lv.H, lv.W, case.A, case.C, cls.shape[3],
               box.shape[3], lv.stride, _farr(lv.anchors.reshape(-1)), float(case.thresh), float(case.scale_clamp),
               float(case.img_hw[0]), float(case.img_hw[1]), 1, L, *twice.ptrs(), 400, 0)
    got = twice.count.bits()
    assert np.array_equal(got[0::2], base[0::2]) and np.array_equal(got[1::2], 2 * base[1::2])
    for s in (0, 2):  # slot order is free: align the two runs by key
        n = base[s]
        ka, kb = (c.key.bits().reshape(B * L, 400)[s, :n] for c in (once, twice))
        oa, ob = np.argsort(ka), np.argsort(kb)
        assert np.array_equal(ka[oa], kb[ob])
        for buf, w in (("box", 4), ("score", 1), ("label", 1)):
            a, b = (getattr(c, buf).bits().reshape(B * L, 400, w)[s, :n] for c in (once, twice))
            assert np.array_equal(a[oa], b[ob]), buf


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,shape", R.FCOS_CONFIGS)
def test_fcos_decode(cuda, dtype, shape):
    """The retina levels with C = 5, ld_ctr = 3 (the centre-ness stride matters), centre-ness
    logits down to -12, negative deltas (relu), boxes clipped on each side; the entry test
    ``sigmoid(x) > t^2 / cs`` against the exact ``p cs > t^2`` with both forms banded."""
    case = R.fcos_case(dtype, shape)
    segs = _check_det(f"FCOS {dtype} {shape}", _run_det(cuda, case, 300), case)
    if shape == "two":
        for name, (l, b, r) in case.placed.items():
            assert r * case.C in segs[b * len(case.levels) + l]["idx"], name


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["retinanet", "fcos"])
def test_detectron_decode_cap_overflow(cuda, arch):
    case = R.retina_case("f32") if arch == "retinanet" else R.fcos_case("f32")
    segs = _check_det(f"{arch} overflow", _run_det(cuda, case, 37), case)
    assert all(s["count"] > 37 and len(s["idx"]) == 37 for s in segs)


# ----------------------------------------------------------------------------- segment merge
@pytest.mark.gpu
@pytest.mark.parametrize("cap_out", [10, 4])
def test_segment_merge(cuda, cap_out):
    """L = 3 levels, batch 2, D = 4; an empty level, a level with sorted_n = pre_max; cap_out
    above and below the totals (8 and 6).  The output is copied bits in level order; the key
    keeps its high word and takes 0xffffffff - position as its low word."""
    B, L, D, cap_in, pre = 2, 3, 4, 16, 5
    rng = np.random.default_rng(3)
    S = B * L
    box = rng.integers(0, 2 ** 32, (S, cap_in, D), dtype=np.uint64).astype(np.uint32)
    score = rng.integers(0, 2 ** 32, (S, cap_in), dtype=np.uint64).astype(np.uint32)
    cls = rng.integers(0, 80, (S, cap_in)).astype(np.int32)
    key = rng.integers(0, 2 ** 63, (S, cap_in), dtype=np.uint64)
    order = np.stack([rng.permutation(cap_in)[:pre] for _ in range(S)]).astype(np.int32)
    sorted_n = np.array([5, 0, 3, 2, 4, 0], np.int32)
    want = R.segment_merge(box, score, cls, key, order, sorted_n, B, L, cap_out)
    dv = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).to(cuda)  # noqa: E731
    ins = [dv(a) for a in (box, score, cls, key)]
    do, dn = dv(order), dv(sorted_n)
    out = Cand(cuda, B, cap_out, D)
    _sync_call("tca_segment_merge", *[t.data_ptr() for t in ins], D, cap_in, do.data_ptr(), dn.data_ptr(), pre, B, L,
               *out.ptrs(), cap_out)
    obox, oscore = out.box.bits().reshape(B, cap_out, D), out.score.bits().reshape(B, cap_out)
    ocls, okey, ocount = out.label.bits().reshape(B, cap_out), out.key.bits().reshape(B, cap_out), out.count.bits()
    for b, (rows, count) in enumerate(want):
        assert ocount[b] == count == min((8, 6)[b], cap_out)
        for o, (bx, sc, cl, k) in enumerate(rows):
            assert np.array_equal(obox[b, o].view(np.uint32), bx) and oscore[b, o].view(np.uint32) == sc
            assert ocls[b, o] == cl and okey[b, o].view(np.uint64) == k
        assert (obox[b, count:] == F32_NAN).all() and (oscore[b, count:] == F32_NAN).all()
        assert (ocls[b, count:] == I32_SENT).all() and (okey[b, count:] == I32_SENT).all()


# --------------------------------------------------------------------------------- GroupNorm
SENT = -768.0  # exact in bf16


def _run_gn(dev, dtype, x, G, ga, be, relu, in_place):
    """x [B, HW, C] at channel offset 8 of a [B, HW, C + 16] buffer; the output at offset 16 of a
    [B, HW, C + 24] one, or in place.  → (output slice, everything outside it) as float32."""
    B, HW, C = x.shape
    ldc, c_off = C + 16, 8
    ldy, y_off = (ldc, c_off) if in_place else (C + 24, 16)
    xin = np.full((B, HW, ldc), SENT, np.float32)
    xin[..., c_off:c_off + C] = x
    flat = torch.full((2 * GUARD + B * HW * ldc,), SENT, dtype=TORCH_DT[dtype], device=dev)
    flat[GUARD:GUARD + xin.size] = _dev(xin, dtype, dev).reshape(-1)
    es = flat.element_size()
    if in_place:
        yflat = flat
    else:
        yflat = torch.full((2 * GUARD + B * HW * ldy,), SENT, dtype=TORCH_DT[dtype], device=dev)
    stats = Buf(dev, B * G * 2, "f32")
    g, b = torch.from_numpy(ga).to(dev), torch.from_numpy(be).to(dev)
    _sync_call("tca_group_norm_nhwc_dt", flat.data_ptr() + GUARD * es, B, HW, C, ldc, c_off, G, 1e-5, g.data_ptr(),
               b.data_ptr(), int(relu), stats.ptr, yflat.data_ptr() + GUARD * es, ldy, y_off, DT_CODE[dtype])
    stats.bits()
    y = yflat.float().cpu().numpy()
    assert (y[:GUARD] == SENT).all() and (y[-GUARD:] == SENT).all(), "guard overwritten"
    y = y[GUARD:-GUARD].reshape(B, HW, ldy)
    out = y[..., y_off:y_off + C].copy()
    y[..., y_off:y_off + C] = SENT
    assert (y == SENT).all(), "channel outside the slice written"
    if not in_place:
        assert np.array_equal(flat.float().cpu().numpy()[GUARD:-GUARD].reshape(B, HW, ldc), xin), "input changed"
    return out


GN_CASES = ([("f32", C, G, HW, r) for C, G in R.GN_SHAPES for HW in R.GN_HW for r in R.GN_RATIOS]
            + [("bf16", C, G, HW, r) for C, G in R.GN_SHAPES for HW in R.GN_HW for r in (0.0, 3.0)])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,C,G,HW,ratio", GN_CASES)
def test_group_norm(cuda, dtype, C, G, HW, ratio):
    """8, 16 and 4 channels per group (the vector path, the scalar path, a vector across two
    groups), HW below one block and ragged over one, batch 2, a channel slice of a wider
    buffer; out of place with ReLU into another stride / offset, and in place without.  Inputs
    with mean / std per group of 0, 3, 30 and 300 (bf16 storage: 0 and 3, the range the FCOS
    towers present; see docs/precision.md)."""
    x = R.make_gn_input(dtype, 2, HW, C, G, ratio)
    ga, be = R.gn_params(C)
    for relu, in_place in ((True, False), (False, True)):
        ref = R.group_norm(x, G, 1e-5, ga, be, relu)
        assert np.isfinite(ref.tol).all()
        got = _run_gn(cuda, dtype, x, G, ga, be, relu, in_place)
        tag = f"GroupNorm {dtype} C={C} G={G} HW={HW} mean/std={ratio:g}"
        if dtype == "f32":
            err = np.abs(got.astype(np.float64) - ref.y)
            _ratio(f"GroupNorm f32 mean/std={ratio:g}", err, ref.tol)
            _ratio(f"GroupNorm f32 mean/std={ratio:g} (two-pass bound)", err, ref.two_pass_tol)
            assert (err <= ref.tol).all(), (tag, float((err / ref.tol).max()))
        else:
            ok, span = R.gn_bf16_ok(got, ref)
            key = lambda a: R.ordered_key(a).astype(np.int64) >> 16  # noqa: E731
            moved = np.abs(key(got) - key(R.round_bf16(ref.y)))
            print(f"{tag}: bound spans 0 / 1 / more bf16 steps on {(span == 0).mean():.4f} / {(span == 1).mean():.4f} / "
                  f"{(span > 1).mean():.4f} of the outputs; moved by one ulp {int((moved == 1).sum())}, by more "
                  f"{int((moved > 1).sum())}")
            bad = np.argwhere(~ok)
            assert ok.all(), (tag, len(bad), [(ref.y[tuple(i)], ref.tol[tuple(i)], got[tuple(i)]) for i in bad[:4]])
            assert (moved[span == 0] == 0).all() and (moved[span <= 1] <= 1).all(), tag


@pytest.mark.gpu
def test_group_norm_refused_arguments(cuda):
    x = torch.full((2 * 5 * 96,), SENT, device=cuda)
    y = torch.full((2 * 5 * 96,), SENT, device=cuda)
    g = torch.ones(64, device=cuda)
    stats = Buf(cuda, 64, "f32")
    #            C,  ldc, c_off, G, ldy, y_off, dtype
    for C, ldc, c_off, G, ldy, y_off, dt in ((64, 80, 8, 7, 80, 8, 0), (60, 80, 8, 4, 80, 8, 0), (64, 84, 8, 8, 80, 8, 0),
                                              (64, 80, 4, 8, 80, 8, 0), (64, 80, 8, 8, 84, 8, 0), (64, 80, 8, 8, 80, 4, 0),
                                              (64, 80, 8, 8, 80, 8, 1)):
        _refused("tca_group_norm_nhwc_dt", x.data_ptr(), 2, 5, C, ldc, c_off, G, 1e-5, g.data_ptr(), g.data_ptr(), 1,
                 stats.ptr, y.data_ptr(), ldy, y_off, dt)
    assert (y == SENT).all() and (stats.bits() == F32_NAN).all()
