"""tca_box3d_iou (ragged pairwise rotated BEV / 3D IoU, csrc/kernels/nms.hip) on the
GPU against the golden, the matching decisions it leads to, the 3D evaluator end to
end with the device IoU and with the CPU twin, and graph capture of the launch."""
import numpy as np
import pytest
import torch

from triton_client_amd import _native
from triton_client_amd.ops import box3d
from triton_client_amd.ops._ws import Workspace
from triton_client_amd.utils.evaluation import IOU_THRESHOLDS_3D, DetectionEvaluator3D, match_predictions

from test_evaluation3d import LAYOUT, golden_ragged

pytestmark = pytest.mark.gpu

ATOL = 1e-5  # the window tests/test_ops_gpu.py::_greedy_replay grants the same device function
MATCH_SEED = 1  # with this seed the golden alone has no pair within 1e-5 of a threshold (cap: 2 %)


def borderline(iou, iouv=IOU_THRESHOLDS_3D, eps=ATOL):
    """Pairs whose reference IoU lies within eps of a threshold: a decision there may go either way."""
    return (np.abs(np.asarray(iou, np.float64)[:, None] - np.asarray(iouv)[None]) <= eps).any(1)


@pytest.mark.parametrize("by_class", [False, True])
def test_kernel_matches_golden_on_ragged_layout(cuda, by_class):
    """Five frames (0,3) (4,0) (1,1) (70,9) (130,65): empty frames, the 64-prediction tile
    boundary (70, 130), the 64-box LDS chunk boundary (65), the degenerate pairs."""
    (pred, gt, poff, goff, pair_off, pc, gc), gbev, g3 = golden_ragged()
    cls = (pc, gc) if by_class else (None, None)
    bev, v3, off = box3d.box3d_iou_ragged(pred, gt, poff, goff, *cls, device=cuda)
    assert bev.dtype == v3.dtype == np.float32 and np.array_equal(off, pair_off)
    if by_class:
        same = np.concatenate([(pc[poff[f]:poff[f + 1], None] == gc[None, goff[f]:goff[f + 1]]).ravel()
                               for f in range(len(LAYOUT))])
        assert not bev[~same].any() and not v3[~same].any()  # other classes: exactly 0
        gbev, g3 = np.where(same, gbev, 0.0), np.where(same, g3, 0.0)
    eb, e3 = np.abs(bev - gbev), np.abs(v3 - g3)
    print(f"by_class={by_class}: max |device - golden| BEV {eb.max():.3e} (pair {eb.argmax()}), "
          f"3D {e3.max():.3e} (pair {e3.argmax()}); overlapping pairs {(gbev > 0).sum()}")
    assert eb.max() <= ATOL and e3.max() <= ATOL


def test_matching_decisions_equal_golden(cuda):
    """``correct`` from the device IoU and from the golden IoU, frame by frame, pairs within
    1e-5 of a threshold left out of both (at most 2 % of the overlapping pairs).  The layout
    is the random one: the degenerate pairs' cross products hold hundreds of IoUs of exactly
    1/2, which are borderline by construction and are covered by the test above."""
    (pred, gt, poff, goff, pair_off, pc, gc), gbev, g3 = golden_ragged(MATCH_SEED, degenerate=False)
    bev, v3, _ = box3d.box3d_iou_ragged(pred, gt, poff, goff, device=cuda)
    iouv = np.asarray(IOU_THRESHOLDS_3D)
    for dev_iou, ref in ((bev, gbev), (v3, g3)):
        out = borderline(ref)
        frac = out[ref > 0].mean()
        print(f"left out: {out.sum()} of {(ref > 0).sum()} overlapping pairs ({100 * frac:.2f} %)")
        assert frac <= 0.02
        d, r = np.where(out, 0.0, dev_iou.astype(np.float64)), np.where(out, 0.0, ref)
        for f, (n, m) in enumerate(LAYOUT):
            p6, g6 = np.zeros((n, 6)), np.zeros((m, 6))
            p6[:, 5], g6[:, 5] = pc[poff[f]:poff[f + 1]], gc[goff[f]:goff[f + 1]]
            sl = slice(pair_off[f], pair_off[f + 1])
            got = match_predictions(g6, p6, iouv, iou=d[sl].reshape(n, m).T)
            want = match_predictions(g6, p6, iouv, iou=r[sl].reshape(n, m).T)
            assert np.array_equal(got, want), f
            if (n, m) == LAYOUT[-1]:
                assert want.any()


def test_launcher_refuses_pair_counts_beyond_int32(cuda):
    with pytest.raises(_native.NativeError):  # returns before any launch
        _native.call("tca_box3d_iou", 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2 ** 31, 0, 0, _native.stream_ptr())


def test_launch_captures_and_replays(cuda):
    from triton_client_amd.pipelines import GraphRunner

    (pred, gt, poff, goff, pair_off, pc, gc), _, _ = golden_ragged()
    c = box3d.prepare(Workspace(cuda), pred, gt, poff, goff, pair_off, pc, gc)
    box3d.launch(c)
    torch.cuda.synchronize()
    eager = (c.iou_bev.clone(), c.iou_3d.clone())
    run = GraphRunner(lambda: box3d.launch(c))
    run()
    assert run.graph is not None
    for _ in range(2):
        c.iou_bev.zero_()
        c.iou_3d.zero_()
        run()
        torch.cuda.synchronize()
        assert torch.equal(c.iou_bev, eager[0]) and torch.equal(c.iou_3d, eager[1])
    assert eager[0].count_nonzero() > 100


def test_evaluator_end_to_end_device_and_twin_agree(cuda, tmp_path):
    """PointPillars on 4 synthetic sweeps (32 rings x 1024 columns) through EvaluateInference3D;
    the ground truth is the detector's own ten best boxes of each sweep, jittered, so IoUs
    spread over the thresholds.  The summary from the device IoU equals the one from the
    CPU twin on the same predictions, borderline pairs left out of both."""
    from triton_client_amd.inference import EvaluateInference3D, LocalDetector3D, boxes_to_jsk
    from triton_client_amd.ros import Bag, compat, msgs
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep

    spec = LidarSpec(rings=32, azimuth_steps=1024, sensor_height=3.23)
    clouds = [compat.create_cloud_xyzi(np.frombuffer(lidar_sweep(spec, s).tobytes(), np.float32).reshape(-1, 4),
                                       msgs.Header(seq=s, frame_id="lidar")) for s in range(4)]
    eng = LocalDetector3D(batch=2, device=cuda, max_points=32768)
    first = eng.detect(clouds)
    rng = np.random.default_rng(0)
    params = {"sub_topic": "/points", "gt_topic": "/detections_3d_gt"}
    bag = str(tmp_path / "pp.bag")
    with Bag(bag, "w") as b:
        for c, d in zip(clouds, first):
            k = np.argsort(-d["pred_scores"])
            k = k[(d["pred_boxes"][k, 3:6] >= 0.3).all(1)][:10]  # random weights also give sliver boxes
            assert len(k) > 0
            gb = d["pred_boxes"][k].astype(np.float64)
            gb[:, [0, 1, 2, 6]] += rng.normal(0, 0.08, (len(k), 4))
            gb[:, 3:6] *= rng.uniform(0.9, 1.1, (len(k), 3))  # sizes stay positive
            g = {"pred_boxes": gb.astype(np.float32),
                 "pred_scores": np.ones(len(k), np.float32), "pred_labels": d["pred_labels"][k]}
            b.write(params["sub_topic"], c)
            b.write(params["gt_topic"], boxes_to_jsk(g, np.arange(len(k)), msgs.Header(seq=c.header.seq)))
    for metric in ("bev", "3d"):
        ev = EvaluateInference3D(engine=eng, params=params, metrics_port=None, metric=metric, device=cuda)
        s = ev.evaluate_bag(bag, batch=2)
        assert s.matched_images == 4 and s.ap.max() > 0.0
        frames, dev_iou, off = ev.evaluator.ious()
        twin = DetectionEvaluator3D(metric=metric, device="cpu", preds=ev.evaluator.preds, gts=ev.evaluator.gts)
        _, ref, off2 = twin.ious()
        assert dev_iou.dtype == np.float32 and np.array_equal(off, off2)
        err = np.abs(dev_iou - ref).max()
        out = borderline(ref)
        print(f"{metric}: {len(ref)} pairs, {(ref > 0).sum()} overlapping, max |device - twin| {err:.3e}, "
              f"{out.sum()} borderline")
        w = int(np.abs(dev_iou - ref).argmax())
        k = int(np.searchsorted(off, w, "right")) - 1
        pw, gw = ev.evaluator.preds[frames[k]], ev.evaluator.gts[frames[k]]
        print(f"worst pair {w} (frame {k}): device {dev_iou[w]!r} twin {ref[w]!r}\n pred {pw[(w - off[k]) // len(gw)]}\n"
              f" gt {gw[(w - off[k]) % len(gw)]}")
        assert out[ref > 0].mean() <= 0.02  # (the 1e-5 window itself is asserted on LiDAR-scale boxes above)
        a = ev.evaluator.summary((frames, np.where(out, 0.0, dev_iou), off))
        t = twin.summary((frames, np.where(out, 0.0, ref), off))
        for x, y in ((a.ap, t.ap), (a.precision, t.precision), (a.recall, t.recall), (a.f1, t.f1)):
            np.testing.assert_array_equal(x, y)
        assert a.as_dict(eng.names) == t.as_dict(eng.names)
