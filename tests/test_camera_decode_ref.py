"""ops/camera_decode_ref.py (the fp64 references of the camera decode kernels) against the
project's independent fp32 CPU implementations, its input generators against their own bands,
each tolerance of tests/test_camera_decode_kernels_gpu.py against a single defect it has to
catch, and the acceptance condition of the GroupNorm bound: the kernel's one-pass arithmetic,
evaluated in NumPy float32 in the kernel's summation order, stays inside the bound at every
conditioning the GPU test sweeps — so a GPU failure there is a kernel finding, not a bound that
is too tight."""
import numpy as np
import pytest
import torch

from triton_client_amd.ops import camera_decode_ref as R


def _nchw(h):
    return torch.from_numpy(np.ascontiguousarray(h.transpose(0, 3, 1, 2)))


def _within(name, got, want, tol):
    err = np.abs(np.asarray(got, np.float64) - want)
    assert (err <= tol).all(), (name, float((err / np.maximum(tol, 1e-300)).max()))


def _match_sets(got, want):
    """got / want: lists of (cls, score, box[4], score tol, box tol[4]) without identities.  Every
    reference candidate pairs with an unused returned one of its class within the bounds."""
    assert len(got) == len(want), (len(got), len(want))
    used = np.zeros(len(got), bool)
    gc, gs, gb = (np.array([g[i] for g in got]) for i in range(3))
    for c, s, b, st, bt in want:
        ok = ~used & (gc == c) & (np.abs(gs - s) <= st) & (np.abs(gb.reshape(-1, 4) - b) <= bt).all(1)
        assert ok.any(), ("no partner for", c, s, b)
        used[np.flatnonzero(ok)[0]] = True


# ------------------------------------------------------------------ against the fp32 decoders
@pytest.mark.parametrize("dtype,na", R.YOLO_CONFIGS)
def test_yolo_reference_matches_decode_cpu(dtype, na):
    from triton_client_amd.models.yolov5 import yolo_decode_reference
    case = R.yolo_case(dtype, na)
    ref = case.ref()
    dec = yolo_decode_reference([_nchw(h) for h in case.heads], torch.from_numpy(case.anchors), case.strides).numpy()
    _within("decoded", dec, ref.dec, ref.dec_tol)


@pytest.mark.parametrize("multi_label", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_yolo_filter_reference_matches_cpu_postprocess(multi_label, masked):
    """YoloPostprocess(device="cpu") on the fp32 decode, NMS switched off (IoU threshold 1):
    the kept set is the reference's, each detection within the bounds."""
    from triton_client_amd.models.yolov5 import yolo_decode_reference
    from triton_client_amd.ops.yolo import YoloPostprocess
    case = R.yolo_case("f32", 3)
    ref = case.ref()
    classes = case.classes if masked else None
    f = R.yolo_filter(ref, case.conf, multi_label, classes)
    assert f.band_counts() == (0, 0)
    pp = YoloPostprocess(case.nc, case.anchors, img_hw=(96, 96), conf_thres=case.conf, iou_thres=1.0, max_det=8192,
                         multi_label=multi_label, classes=classes, device="cpu")
    dec = yolo_decode_reference([_nchw(h) for h in case.heads], torch.from_numpy(case.anchors), case.strides).numpy()
    got = pp.postprocess_decoded(dec).per_image()[0]
    idx = np.flatnonzero(f.keep[0])
    want = [(f.cls[0, i], f.score[0, i], ref.box[0, f.row[i]], f.tol[0, i], ref.box_tol[0, f.row[i]]) for i in idx]
    _match_sets(list(zip(got["cls"], got["score"], got["box"])), want)
    # the same filter on a decoded response (the remote client's path)
    dcase = R.DecodedCase(0, case.nc, dec, None, case.conf, (0.0, 0.0))
    fd, box, _ = R.filter_decoded(dcase, multi_label, classes)
    assert np.array_equal(fd.keep, f.keep)


def test_masked_rows_are_dropped_not_promoted():
    case = R.yolo_case("f32", 3)
    ref = case.ref()
    f = R.yolo_filter(ref, case.conf, False, case.classes)
    free = R.yolo_filter(ref, case.conf, False, None)
    assert len(case.masked_rows) > 20 and free.keep[0, case.masked_rows].all()
    assert not f.keep[0, case.masked_rows].any()
    assert (free.cls[0, case.masked_rows] == 34).all()  # second mask word


@pytest.mark.parametrize("sxy", [1.0, 1.05])
def test_yolov4_reference_matches_decode_cpu(sxy):
    from triton_client_amd.models import yolov4 as M
    anc = np.array([[[M.ANCHORS[2 * m + k] / M.STRIDES[l] for k in range(2)] for m in ms]
                    for l, ms in enumerate(M.MASKS)], np.float32)
    case = R.make_yolov4_case("f32", sxy=sxy, anchors=anc)
    ref = case.ref()
    assert ref.filt.band_counts() == (0, 0)
    boxes, confs = M.decode_reference([_nchw(h) for h in case.heads], case.nc, sxy)
    _within("boxes", boxes.numpy()[:, :, 0], ref.boxes, ref.boxes_tol)
    _within("confs", confs.numpy(), ref.confs, ref.confs_tol)
    keep = confs.numpy().max(2) > case.conf  # post_processing's filter
    assert np.array_equal(keep, ref.filt.keep)
    assert np.array_equal(confs.numpy().argmax(2)[keep], ref.filt.cls[keep])


@pytest.mark.parametrize("arch", ["retinanet", "fcos"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_detectron_reference_matches_decode_cpu(arch, dtype):
    """models.detectron.decode_reference with the top-k, NMS and keep-100 switched off returns
    every entered (anchor, class): the reference's sets, values within the bounds."""
    from triton_client_amd.config.detectron import DetectronConfig
    from triton_client_amd.models.detectron import decode_reference
    case = R.retina_case(dtype) if arch == "retinanet" else R.fcos_case(dtype)
    cfg = DetectronConfig(arch=arch, num_classes=case.C, strides=tuple(L.stride for L in case.levels),
                          anchor_sizes=tuple(float(L.stride) for L in case.levels), anchor_scales=(1.0,),
                          anchor_ratios=(0.25, 1.0, 4.0), score_thresh=case.thresh, topk_per_level=10 ** 6,
                          nms_thresh=1.0, max_detections=10 ** 6, scale_clamp=case.scale_clamp)
    if arch == "retinanet":
        for l, L in enumerate(case.levels):
            np.testing.assert_array_equal(np.array(cfg.anchor_table(l), np.float32), L.anchors)
        outs = [(_nchw(L.cls), _nchw(L.box)) for L in case.levels]
    else:
        outs = [(_nchw(L.cls), _nchw(L.box), _nchw(L.ctr[..., None])) for L in case.levels]
    per = decode_reference(outs, cfg, image_hw=case.img_hw)
    for b, (bx, sc, cl) in enumerate(per):
        want = []
        for l in range(len(case.levels)):
            ref = case.ref(l)
            assert not any(ref.bands), ref.bands
            for i in np.flatnonzero(ref.keep[b]):
                want.append((ref.cls[i], ref.score[b, i], ref.box[b, ref.row[i]], ref.tol[b, i], ref.box_tol[b, ref.row[i]]))
        _match_sets(list(zip(cl, sc, bx)), want)


@pytest.mark.parametrize("C,G", R.GN_SHAPES)
@pytest.mark.parametrize("relu", [False, True])
def test_group_norm_reference_matches_torch_float64(C, G, relu):
    x = R.make_gn_input("f32", 2, 273, C, G, 3.0)
    ga, be = R.gn_params(C)
    ref = R.group_norm(x, G, 1e-5, ga, be, relu)
    y = torch.nn.functional.group_norm(torch.from_numpy(x).double().permute(0, 2, 1), G, torch.from_numpy(ga).double(),
                                       torch.from_numpy(be).double(), float(np.float32(1e-5)))
    y = (torch.relu(y) if relu else y).permute(0, 2, 1).numpy()
    np.testing.assert_allclose(ref.y, y, rtol=1e-12, atol=1e-12)


def test_segment_merge_reference_on_a_hand_case():
    box = np.arange(2 * 3 * 2, dtype=np.uint32).reshape(2, 3, 2)
    score, cls = np.arange(6, dtype=np.uint32).reshape(2, 3) + 100, np.arange(6, dtype=np.int32).reshape(2, 3)
    key = (np.arange(6, dtype=np.uint64).reshape(2, 3) + 7) << np.uint64(32) | np.uint64(5)
    out = R.segment_merge(box, score, cls, key, np.array([[2, 0], [1, 1]]), np.array([2, 1]), 1, 2, 2)
    rows, count = out[0]
    assert count == 2 and [int(r[1]) for r in rows] == [102, 100]
    assert [int(r[3]) for r in rows] == [(9 << 32) | 0xFFFFFFFF, (7 << 32) | 0xFFFFFFFE]


# --------------------------------------------------------------------------------- the bands
def test_every_gpu_case_is_clear_of_its_bands():
    for dtype, na in R.YOLO_CONFIGS:
        case = R.yolo_case(dtype, na)
        ref = case.ref()
        for ml in (False, True):
            for classes in (None, case.classes):
                f = R.yolo_filter(ref, case.conf, ml, classes)
                assert f.band_counts() == (0, 0) and f.keep.sum() > 100
    for dtype, sxy in R.YOLOV4_CONFIGS:
        f = R.yolov4_case(dtype, sxy).ref().filt
        assert f.band_counts() == (0, 0) and f.keep.sum() > 100
    for kind in (0, 1):
        case = R.decoded_case(kind)
        for ml in (False, True):
            f, _, _ = R.filter_decoded(case, ml, R.YOLO_CLASSES if kind == 0 else None)
            assert f.band_counts() == (0, 0) and R.decoded_gap_count(case) == 0 and f.keep.sum() > 100
    for make, configs in ((R.retina_case, R.RETINA_CONFIGS), (R.fcos_case, R.FCOS_CONFIGS)):
        for dtype, shape in configs:
            case = make(dtype, shape)
            for l in range(len(case.levels)):
                ref = case.ref(l)
                assert not any(ref.bands), (dtype, shape, l, ref.bands)
                assert ref.keep.sum() > 30


def test_clip_and_clamp_are_active_where_placed():
    case = R.retina_case("f32")
    ref = case.ref(0)
    hi = (72.0, 56.0)
    for q, name in enumerate(("left", "top", "right", "bottom")):
        _, b, r = case.placed[name]
        assert ref.keep[b, r * case.C] and ref.raw[b, r, q] != ref.box[b, r, q]
        assert ref.box[b, r, q] == (0.0 if q < 2 else hi[q - 2])
    _, b, r = case.placed["clamp"]
    d = case.levels[0].box.reshape(2, -1, 4)[b, r]
    assert (d[2:] > case.scale_clamp).all() and (ref.raw[b, r] == ref.box[b, r]).all()  # clamped, not clipped
    multi = ref.keep.reshape(2, -1, case.C).sum(-1)
    assert (multi > 1).sum() > 20  # several classes of one anchor
    case = R.fcos_case("f32")
    ref = case.ref(0)
    for q, name in enumerate(("left", "top", "right", "bottom")):
        _, b, r = case.placed[name]
        assert ref.keep[b, r * case.C] and ref.raw[b, r, q] != ref.box[b, r, q]
    L = case.levels[0]
    assert (L.ctr == -12.0).sum() > 20 and (L.box < 0).mean() > 0.2
    tiny = (L.ctr == -12.0).reshape(2, -1)
    assert not ref.keep.reshape(2, -1, case.C)[tiny].any()


# ------------------------------------------------------------------------------ the mutations
def _breaks(tol, a, b):
    return bool((np.abs(a - b) > tol).any())


@pytest.mark.parametrize("defect", ["half_pixel", "wh_swap", "index_order", "level_stride"])
def test_yolo_bounds_catch_each_defect(defect):
    case = R.yolo_case("f32", 3)
    ref, bad = case.ref(), case.ref(defect)
    assert _breaks(ref.dec_tol[..., :4], ref.dec[..., :4], bad.dec[..., :4])
    assert _breaks(ref.box_tol, ref.box, bad.box)
    if defect == "index_order":
        assert _breaks(ref.dec_tol[..., 4:], ref.dec[..., 4:], bad.dec[..., 4:])


def test_class_filter_before_argmax_changes_the_kept_set():
    case = R.yolo_case("f32", 3)
    ref = case.ref()
    f, bad = (R.yolo_filter(ref, case.conf, False, case.classes, _mutate=m) for m in ("", "filter_before_argmax"))
    assert bad.keep[0, case.masked_rows].all() and not f.keep[0, case.masked_rows].any()
    d = R.decoded_case(0)
    f, bad = (R.filter_decoded(d, False, R.YOLO_CLASSES, _mutate=m)[0] for m in ("", "filter_before_argmax"))
    assert bad.keep.sum() > f.keep.sum()


@pytest.mark.parametrize("defect", ["xw_xh", "no_sxy_shift", "wh_swap"])
def test_yolov4_bounds_catch_each_defect(defect):
    case = R.yolov4_case("f32", 1.05)
    ref, bad = case.ref(), case.ref(defect)
    assert _breaks(ref.boxes_tol, ref.boxes, bad.boxes) and _breaks(ref.cand_tol, ref.cand, bad.cand)
    d = R.decoded_case(1)
    if defect == "xw_xh":
        (_, box, tol), (_, bbox, _) = R.filter_decoded(d), R.filter_decoded(d, _mutate=defect)
        assert _breaks(tol, box, bbox)


@pytest.mark.parametrize("arch,defect", [("retinanet", "no_clamp"), ("retinanet", "wh_swap"), ("retinanet", "index_order"),
                                         ("retinanet", "level_stride"), ("fcos", "half_pixel"), ("fcos", "level_stride")])
def test_detectron_bounds_catch_each_defect(arch, defect):
    case = R.retina_case("f32") if arch == "retinanet" else R.fcos_case("f32")
    ref, bad = case.ref(0), case.ref(0, defect)
    kept = ref.keep.reshape(ref.keep.shape[0], -1, case.C).any(-1)
    if defect == "index_order":
        assert not np.array_equal(ref.keep, bad.keep)
    else:
        assert _breaks(ref.box_tol[kept], ref.box[kept], bad.box[kept])
    if defect == "no_clamp":  # only the placed anchor moves
        _, b, r = case.placed["clamp"]
        moved = (np.abs(ref.box - bad.box) > ref.box_tol).any(-1)
        assert moved[b, r] and kept[b, r]


@pytest.mark.parametrize("C,G", R.GN_SHAPES)
@pytest.mark.parametrize("HW", R.GN_HW)
def test_group_norm_bound_catches_the_unbiased_variance(C, G, HW):
    x = R.make_gn_input("f32", 2, HW, C, G, 0.0)
    ga, be = R.gn_params(C)
    ref, bad = (R.group_norm(x, G, 1e-5, ga, be, False, _mutate=m) for m in ("", "unbiased"))
    assert _breaks(ref.tol, ref.y, bad.y)


# --------------------------------------------------- the acceptance condition of the GN bound
@pytest.mark.parametrize("C,G", R.GN_SHAPES)
@pytest.mark.parametrize("HW", R.GN_HW)
@pytest.mark.parametrize("ratio", R.GN_RATIOS)
@pytest.mark.parametrize("fma", [False, True])
def test_one_pass_float32_group_norm_stays_inside_the_bound(C, G, HW, ratio, fma):
    x = R.make_gn_input("f32", 2, HW, C, G, ratio)
    ga, be = R.gn_params(C)
    ref = R.group_norm(x, G, 1e-5, ga, be, True)
    assert np.isfinite(ref.tol).all(), "the bound is vacuous at this conditioning"
    got = R.group_norm_onepass_f32(x, G, 1e-5, ga, be, True, fma=fma)
    err = np.abs(got.astype(np.float64) - ref.y)
    print(f"C={C} G={G} HW={HW} mean/std={ratio} fma={fma}: cond {ref.cond.max():.3g} err/bound {(err / ref.tol).max():.3f}"
          f" err/two-pass bound {(err / ref.two_pass_tol).max():.3f}")
    assert (err <= ref.tol).all()


@pytest.mark.parametrize("C,G", R.GN_SHAPES)
@pytest.mark.parametrize("ratio", [0.0, 3.0])
def test_one_pass_group_norm_in_bf16_stays_inside_the_rounded_bound(C, G, ratio):
    """bf16 storage at the conditionings the GPU test runs it at: the float32 evaluation rounded
    to bf16 equals the rounded fp64 value, or its neighbour where a rounding tie lies within the
    fp32 bound.  Outputs that cancel to below about 2^9 bounds, where the bound spans several
    bf16 values, are held to the bound itself; they are a small share of the outputs."""
    HW = 273
    x = R.make_gn_input("bf16", 2, HW, C, G, ratio)
    ga, be = R.gn_params(C)
    ref = R.group_norm(x, G, 1e-5, ga, be, False)
    got = R.round_storage(R.group_norm_onepass_f32(x, G, 1e-5, ga, be, False), "bf16")
    ok, span = R.gn_bf16_ok(got, ref)
    moved = np.abs((R.ordered_key(got).astype(np.int64) >> 16) - (R.ordered_key(R.round_bf16(ref.y)).astype(np.int64) >> 16))
    print(f"C={C} G={G} mean/std={ratio}: span 0 / 1 / more: {(span == 0).mean():.4f} / {(span == 1).mean():.4f} / "
          f"{(span > 1).mean():.4f}; moved by one ulp {(moved == 1).sum()}, by more {(moved > 1).sum()}")
    assert ok.all() and (moved[span <= 1] <= 1).all() and (moved[span == 0] == 0).all()
    assert (span > 1).mean() < 0.02


def test_round_bf16_has_no_double_rounding():
    tie = 1.00390625  # midway between the bf16 values 1.0 and 1.0078125
    v = np.array([tie - 1e-12, tie, tie + 1e-12, -tie + 1e-12, -tie - 1e-12])
    assert R.round_bf16(v).tolist() == [1.0, 1.0, 1.0078125, -1.0, -1.0078125]
    assert R.round_storage(v, "bf16").tolist()[0] == 1.0  # the fp32 detour lands on the tie: to even


def test_fcos_tower_conditioning():
    """mean^2 / var of every GroupNorm input of the FCOS towers of tests/test_detectron.py's model,
    on its input: the figure docs/precision.md records.  The one-pass variance is kept because
    this stays far below the conditioning at which its bound leaves a bf16 ulp (see the docs)."""
    from test_detectron import _model
    m = _model("fcos")
    worst = []
    hooks = [g.register_forward_pre_hook(lambda mod, inp: worst.append(_cond(inp[0], mod.num_groups)))
             for g in m.head.modules() if isinstance(g, torch.nn.GroupNorm)]
    with torch.no_grad():
        m(torch.rand(2, 3, 128, 160, generator=torch.Generator().manual_seed(0)) * 255)
    for h in hooks:
        h.remove()
    assert len(worst) == 8 * 5  # two towers x four GroupNorms x five levels
    print(f"FCOS tower GroupNorm inputs: max mean^2/var {max(worst):.3f}, median {np.median(worst):.3f}")
    assert max(worst) < R.GN_TOWER_COND_LIMIT


def _cond(x, G):
    x = x.double()
    B, C = x.shape[:2]
    g = x.reshape(B, G, -1)
    return float((g.mean(-1) ** 2 / g.var(-1, unbiased=False)).max())
