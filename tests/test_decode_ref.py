"""ops/decode_ref.py (the fp64 references of the LiDAR decode kernels) against the project's
fp32 CPU decoders, its input generators against their own bands, and each tolerance of
tests/test_decode_kernels_gpu.py against a single defect it has to catch."""
import dataclasses

import numpy as np
import pytest
import torch

from triton_client_amd.ops import decode_ref as R

DTYPES = ["f32", "f16", "bf16"]


# ------------------------------------------------------------------------------- ordered_key
def test_ordered_key_is_monotone():
    tiny = np.float32(1e-45)  # the smallest denormal
    x = np.array([-np.inf, -3.0e38, -12.0, -1.0, -1.1754944e-38, -tiny, -0.0, 0.0, tiny, 1.1754944e-38, 0.5, 1.0,
                  12.0, 3.0e38, np.inf], np.float32)
    k = R.ordered_key(x)
    assert k.dtype == np.uint32 and (np.diff(k.astype(np.int64)) > 0).all()  # -0.0 orders below +0.0
    rng = np.random.default_rng(0)
    y = np.concatenate([x, rng.standard_normal(500).astype(np.float32) * 10,
                        (rng.standard_normal(100) * 1e-40).astype(np.float32)])
    rng.shuffle(y)
    by_key = y[np.argsort(R.ordered_key(y), kind="stable")]
    assert np.array_equal(np.sort(y), by_key)  # np.sort treats -0.0 == 0.0; so does array_equal
    assert R.ordered_key(np.float32(0.0)) == 0x80000000 and R.ordered_key(np.float32(-0.0)) == 0x7FFFFFFF


def test_round_storage_matches_torch():
    a = (np.random.default_rng(1).standard_normal(4000) * 7).astype(np.float32)
    a[:4] = [0.0, -0.0, 1.00390625, 1.01171875]  # bf16 ties: to even
    for name, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        want = torch.from_numpy(a).to(dt).float().numpy()
        assert np.array_equal(R.round_storage(a, name).view(np.uint32), want.view(np.uint32))


# ----------------------------------------------------------------- against the fp32 decoders
def test_anchor_reference_matches_decode_cpu():
    from triton_client_amd.config.lidar import PointPillarsConfig
    from triton_client_amd.ops.lidar import AnchorPostprocess
    cfg = PointPillarsConfig()
    ap = AnchorPostprocess(cfg, 2, device="cpu")
    H, W, A, C, bins = 20, 24, ap.A, ap.C, cfg.num_dir_bins
    ap.H, ap.W = H, W
    g = torch.Generator().manual_seed(3)
    cls = torch.randn(2, A * C, H, W, generator=g) * 2
    box = torch.randn(2, A * 7, H, W, generator=g) * 0.5
    dr = torch.randn(2, A * bins, H, W, generator=g)
    out, score, lab = ap.decode_cpu(cls, box, dr)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().numpy()  # noqa: E731
    ref = R.anchor_decode(nhwc(cls), nhwc(box), nhwc(dr), A, C, bins, ap.table, ap.x0, ap.xs, ap.y0, ap.ys,
                          cfg.dir_offset, cfg.dir_limit_offset)
    np.testing.assert_array_equal(lab.numpy(), ref.label)
    np.testing.assert_allclose(score.numpy(), ref.score, rtol=1e-6)
    np.testing.assert_allclose(out[..., :6].numpy(), ref.box[..., :6], rtol=1e-5, atol=1e-5)
    clear = np.abs(ref.u - np.rint(ref.u)) > R.FLOOR_BAND  # away from the floor's jumps
    assert clear.mean() > 0.99
    np.testing.assert_allclose(out[..., 6].numpy()[clear], ref.box[..., 6][clear], rtol=1e-5, atol=1e-5)
    # without a dir head the raw angle comes back
    raw = R.anchor_decode(nhwc(cls), nhwc(box), None, A, C, bins, ap.table, ap.x0, ap.xs, ap.y0, ap.ys,
                          cfg.dir_offset, cfg.dir_limit_offset)
    ra = np.tile(ap.table[:, 4].astype(np.float64), H * W)
    np.testing.assert_array_equal(raw.box[..., 6], nhwc(box).reshape(2, -1, 7)[..., 6].astype(np.float64) + ra)


def _center_cfg():
    from triton_client_amd.config.lidar import NUSC_PILLARS, CenterPointConfig
    v = dataclasses.replace(NUSC_PILLARS, point_cloud_range=(-12.8, -12.8, -5.0, 12.8, 12.8, 3.0), max_voxels=4000)
    return CenterPointConfig(voxel=v)


def test_centerhead_reference_matches_cpu_postprocess():
    """Random heads through models.centerpoint.decode_reference / CenterPointPostprocess.cpu
    (NMS switched off by a huge IoU threshold, so every kept pixel comes back)."""
    from triton_client_amd.models.centerpoint import decode_reference
    from triton_client_amd.ops.centerpoint import NUSC_CLASS_THRESH, CenterPointPostprocess
    cfg = dataclasses.replace(_center_cfg(), nms_iou=2.0, nms_pre_max=100000, nms_post_max=100000,
                              post_center_range=(-10.0, -11.0, -1.0, 11.0, 10.0, 1.2))
    H, W = cfg.feature_map_size
    rng = np.random.default_rng(4)
    ncs = [len(t.class_names) for t in cfg.tasks]
    assert tuple(ncs) == R.CENTER_TASKS
    head = np.zeros((2, H, W, 96), np.float32)
    for t, nc in enumerate(ncs):
        o = 16 * t
        head[..., o:o + 2] = rng.uniform(0, 1, (2, H, W, 2))
        head[..., o + 2:o + 10] = rng.normal(0, 0.7, (2, H, W, 8))
        head[..., o + 10:o + 10 + nc] = rng.normal(-2.0, 1.5, (2, H, W, nc))
    offs = [16 * t for t in range(6)]
    c0 = list(np.cumsum([0] + ncs)[:-1])
    info = list(zip(offs, ncs, c0))
    tabs = (None, NUSC_CLASS_THRESH)
    ths = [None if tb is None else [tb[c] for c in range(sum(ncs))] for tb in tabs]

    def reference(th):
        return R.centerhead_decode(head, info, th, cfg.score_thresh, cfg.voxel.point_cloud_range[:2],
                                   cfg.voxel.voxel_size[:2], cfg.out_size_factor, cfg.post_center_range)

    def borderline(ref):  # where fp32 and fp64 may decide differently
        return (np.abs(ref.score - ref.thr) < 1e-5) | ((ref.score > ref.thr) & (np.abs(ref.margin) < 1e-4).any(-1))

    for th in ths:  # silence the few borderline pixels: both sides then drop them by score
        for b, t, p in zip(*np.nonzero(borderline(reference(th)))):
            head.reshape(2, -1, 96)[b, p, 16 * t + 10:16 * t + 10 + ncs[t]] = -10.0
    outs = [torch.from_numpy(head[..., o:o + 10 + nc]).permute(0, 3, 1, 2) for o, nc in zip(offs, ncs)]
    for table, th in zip(tabs, ths):
        ref = reference(th)
        assert not borderline(ref).any() and ref.keep.sum() > 1000 and ((ref.score > ref.thr) & ~ref.keep).sum() > 100
        pp = CenterPointPostprocess(cfg, 2, offs, device="cpu", class_thresh=table)
        res = pp(torch.from_numpy(head)).per_image()
        for b in range(2):
            keep = ref.keep[b]
            want_box = ref.box[b][keep][:, [0, 1, 2, 3, 4, 5, 7, 8, 6]]  # det3d order
            got = res[b]
            # match by (label, score): the scores are distinct random numbers
            gk = np.lexsort((got["pred_scores"], got["pred_labels"]))
            wk = np.lexsort((ref.score[b][keep], ref.label[b][keep]))
            np.testing.assert_array_equal(got["pred_labels"][gk], ref.label[b][keep][wk])
            np.testing.assert_allclose(got["pred_scores"][gk], ref.score[b][keep][wk], rtol=1e-6)
            np.testing.assert_allclose(got["pred_boxes"][gk], want_box[wk], rtol=1e-5, atol=1e-5)
            # and the per-task decode_reference, the function tests/test_centerpoint.py uses
            for t in range(6):
                bx, sc, lb = decode_reference([outs[t]], cfg, [c0[t]], pp.class_thresh)[b]
                k = ref.keep[b, t]
                o = np.argsort(sc)
                np.testing.assert_allclose(sc[o], np.sort(ref.score[b, t][k]), rtol=1e-6)
                w = np.argsort(ref.score[b, t][k])
                np.testing.assert_array_equal(lb[o], ref.label[b, t][k][w])
                np.testing.assert_allclose(bx[o], ref.box[b, t][k][w][:, [0, 1, 2, 3, 4, 5, 7, 8, 6]], rtol=1e-5,
                                           atol=1e-5)


# ------------------------------------------------------------------ generators and their bands
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("A,C,bins,dense", [(6, 3, 2, False), (6, 3, 2, True), (2, 1, 2, False), (8, 5, 2, False)])
def test_anchor_inputs_clear_of_every_band(dtype, A, C, bins, dense):
    case = R.make_anchor_case(A, C, bins, dtype, dense=dense)
    ref = case.ref()
    assert R.anchor_band_counts(case, ref) == (0, 0)
    assert np.abs(case.cls).max() <= R.MAX_LOGIT
    keep = ref.score >= np.float32(case.score_thresh)
    n = keep.sum(1)
    assert n[1] == 0 and n[0] > 200 and n[2] > 200  # an empty frame between two busy ones
    if dense:
        assert keep[0, :4096].all()  # > 2048 of one block's anchors: the stage overflows
    if C > 1:  # class ties among the kept anchors of frame 0, resolved to the lower class
        cl = case.cls.reshape(3, -1, C)[0]
        tied = (cl == cl.max(-1, keepdims=True)).sum(-1) > 1
        assert (tied & keep[0]).sum() >= 32
        first = np.array([np.flatnonzero(r == r.max())[0] for r in cl[tied]])
        assert np.array_equal(ref.label[0][tied], first + 1)
    fl = np.floor(ref.u[keep])
    assert len(np.unique(fl)) >= 3  # several periods


def test_anchor_tie_input_sits_on_the_threshold():
    case = R.make_tie_anchor_case()
    ref = case.ref()
    even = np.arange(ref.score.shape[1]) % 2 == 0
    assert (ref.score[0, even] == 0.5).all() and case.score_thresh == 0.5 and (ref.score[0, ~even] < 0.4).all()
    assert R.anchor_band_counts(case, ref)[1] == 0
    assert (ref.label[0] == 1).all()  # three equal logits: the first class


CENTER_THRESH = R.CENTER_THRESH


def center_thresholds(name):
    from triton_client_amd.ops.centerpoint import NUSC_CLASS_THRESH
    return R.center_thresholds(name, NUSC_CLASS_THRESH)


def center_case(dtype, ldc):
    from triton_client_amd.ops.centerpoint import NUSC_CLASS_THRESH
    return R.center_case(dtype, ldc, NUSC_CLASS_THRESH)


@pytest.mark.parametrize("dtype,ldc", [("f32", 96), ("f32", 104), ("f16", 96), ("bf16", 96)])
def test_center_inputs_clear_of_every_band(dtype, ldc):
    case = center_case(dtype, ldc)
    for name in CENTER_THRESH:
        ct, st = center_thresholds(name)
        ref = case.ref(ct, st)
        assert R.center_band_counts(ref) == (0, 0)
        n = ref.keep.sum(-1)
        assert n[1, 3] == 0 and (np.delete(n.reshape(-1), 9) > 20).all()  # one empty segment
        assert not ref.keep[0, 0, 64:128].any() and ref.keep[0, 0, 128:192].all()  # silent wave, full wave
        for f, (b, t, p) in enumerate(case.face_pixels):  # dropped by face f alone
            assert ref.score[b, t, p] > ref.thr[b, t, p]
            assert ref.margin[b, t, p, f] < -R.RANGE_BAND and (np.delete(ref.margin[b, t, p], f) > 0).all()
        assert ((ref.score > ref.thr) & ~ref.keep).sum() > 20  # the range filter does work
    # per-class thresholds and the score_thresh floor both decide somewhere
    a, b, c = (case.ref(*center_thresholds(n)).keep.sum() for n in CENTER_THRESH)
    assert c > a > b


def test_center_tie_input_sits_on_the_threshold():
    case = R.make_tie_center_case()
    ref = case.ref(None, 0.5)
    even = np.arange(35) % 2 == 0
    assert (ref.score[0, 0, even] == 0.5).all() and not ref.keep.any()  # '>' drops the ties
    assert (ref.margin > 0.1).all()
    assert case.ref(None, 0.5, _mutate="ge").keep[0, 0, even].all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", R.TOPK_KINDS)
def test_topk_inputs(kind, dtype):
    cls = R.make_topk_cls(kind, dtype, k=1024)
    keys = R.max_logit_keys(cls, 6, 3)
    assert keys.shape == (2, 9102) and np.abs(cls).max() <= R.MAX_LOGIT
    for b in range(2):
        srt = np.sort(keys[b])[::-1].astype(np.int64)
        # the exact k-th key rounded down to its 256-key bucket satisfies the contract
        for k in (1, 64, 1024, 9102):
            thr = srt[k - 1] & ~0xFF
            assert R.topk_threshold_ok(keys[b], thr, k) == (True, True)
            assert R.topk_threshold_ok(keys[b], thr + 256, k)[0] is False or (srt[:k] >= thr + 256).all()
        assert R.topk_threshold_ok(keys[b], 0, 9103) == (True, True)
    if kind == "narrow":
        assert len(np.unique(keys >> 20)) == 1
    if kind == "equal":
        assert len(np.unique(keys[0])) == 1
    if kind == "tie_straddle":
        srt = np.sort(keys[0])[::-1]
        assert srt[1023 - 100] == srt[1023 + 100]
    if kind == "spread":
        assert (keys == 0x80000000).any() and (keys == 0x7FFFFFFF).any() and (keys > 0x80000000).any()
    if kind == "signed_zero":
        for b in range(2):
            assert (keys[b] > 0x80000000).sum() == 100 and (keys[b] == 0x80000000).sum() == 50
            assert (keys[b] == 0x7FFFFFFF).sum() == 40  # k = 170 reaches into the -0.0 group


# ------------------------------------------------------------ each bound catches its defect
def _exceeds(got, ref_box, tol, q):
    return (np.abs(got[..., q] - ref_box[..., q]) > tol[..., q]).any()


@pytest.mark.parametrize("mutation,q", [("diag_dxa", 0), ("diag_dxa", 1), ("dir_shift", 6), ("no_dlo", 6)])
def test_anchor_bounds_catch(mutation, q):
    case = R.make_anchor_case()
    ref, bad = case.ref(), case.ref(_mutate=mutation)
    keep = ref.score >= np.float32(case.score_thresh)
    assert _exceeds(bad.box[keep], ref.box[keep], ref.tol[keep], q)
    assert not _exceeds(ref.box[keep].astype(np.float32).astype(np.float64), ref.box[keep], ref.tol[keep], q)


@pytest.mark.parametrize("mutation,q", [("no_osf", 0), ("no_osf", 1), ("yaw_swap", 6)])
def test_center_bounds_catch(mutation, q):
    case = center_case("f32", 96)
    ct, st = center_thresholds("nusc+0.1")
    ref, bad = case.ref(ct, st), case.ref(ct, st, _mutate=mutation)
    assert _exceeds(bad.box[ref.keep], ref.box[ref.keep], ref.tol[ref.keep], q)
    assert not _exceeds(ref.box[ref.keep].astype(np.float32).astype(np.float64), ref.box[ref.keep],
                        ref.tol[ref.keep], q)


def test_center_label_base_is_caught():
    case = center_case("f32", 96)
    ct, st = center_thresholds("nusc+0.1")
    ref, bad = case.ref(ct, st), case.ref(ct, st, _mutate="label_base")
    assert (bad.label[ref.keep] != ref.label[ref.keep]).any()
    for t, (_, nc, c0) in enumerate(case.task_info):  # every task's base shows among the kept
        assert ref.label[:, t][ref.keep[:, t]].min() == c0
