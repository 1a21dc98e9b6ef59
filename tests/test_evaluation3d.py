"""3D detection evaluation on the CPU: the golden 3D IoU, the vectorised NumPy
twin of the rotated-IoU kernel, the ragged layout, the evaluator, the
ground-truth messages, and the driver / CLI end to end on synthetic bags."""
import json

import numpy as np
import pytest

from triton_client_amd.ops import golden
from triton_client_amd.ops.box3d import box3d_iou_ragged, boxes7, iou_pairs_np, ragged_offsets, tile_table
from triton_client_amd.utils.evaluation import DetectionEvaluator3D, compute_ap

# The AP of a perfect detector under this project's metric (``compute_ap``: COCO 101-point
# sampling, whose last sample at recall 1 reads the curve's closing point (1, 0)): 0.995,
# the value tests/test_drivers.py asserts for the 2D evaluator.  "AP 1.0" below means this.
PERFECT_AP = compute_ap(np.array([1.0]), np.array([1.0]))[0]
LAYOUT = ((0, 3), (4, 0), (1, 1), (70, 9), (130, 65))  # (predictions, ground truth) per frame


def degenerate_pairs():
    """Identical, contained, edge- and corner-touching boxes, every pairing of yaw
    0 / ±π/2 / π (offset, concentric and square), and a 0.3 m box inside a 5 m box."""
    P, G = [], []
    a = [3.0, -2.0, 0.5, 4.0, 2.0, 1.5, 0.3]
    P.append(a); G.append(a)  # noqa: E702
    P.append([0, 0, 0, 5, 5, 2, 0.7]); G.append([0.5, 0.2, 0.1, 0.3, 0.3, 0.3, -0.4])  # noqa: E702
    P.append([0, 0, 0, 4, 2, 1, 0.0]); G.append([0.5, 0.1, 0, 2, 1, 0.5, 0.0])  # noqa: E702
    P.append([0, 0, 0, 4, 2, 1, 0.0]); G.append([4, 0, 0, 4, 2, 1, 0.0])  # noqa: E702  edge
    P.append([0, 0, 0, 4, 2, 1, 0.0]); G.append([4, 2, 0, 4, 2, 1, 0.0])  # noqa: E702  corner
    for ya in (0.0, np.pi / 2, -np.pi / 2, np.pi):
        for yb in (0.0, np.pi / 2, -np.pi / 2, np.pi):
            P.append([10, 5, 0, 4, 2, 1.5, ya]); G.append([10.5, 5.25, 0.2, 3, 2, 1.5, yb])  # noqa: E702
            P.append([10, 5, 0, 4, 2, 1.5, ya]); G.append([10, 5, 0, 4, 2, 1.5, yb])  # noqa: E702
            P.append([10, 5, 0, 4, 4, 1.5, ya]); G.append([10, 5, 0, 4, 4, 1.5, yb])  # noqa: E702
    return np.array(P, np.float64), np.array(G, np.float64)


def random_pairs(n, seed):
    """LiDAR-scale boxes: centres within ±80 m, sizes 0.3-12 m, any yaw; the partner close enough to overlap."""
    r = np.random.default_rng(seed)
    A, B = np.zeros((n, 7)), np.zeros((n, 7))
    A[:, :2], A[:, 2] = r.uniform(-78, 78, (n, 2)), r.uniform(-2, 2, n)
    A[:, 3:6], A[:, 6] = r.uniform(0.3, 12, (n, 3)), r.uniform(-np.pi, np.pi, n)
    B[:, :2], B[:, 2] = A[:, :2] + r.normal(0, 2.0, (n, 2)).clip(-2, 2), A[:, 2] + r.normal(0, 0.7, n)
    B[:, 3:6], B[:, 6] = r.uniform(0.3, 12, (n, 3)), r.uniform(-np.pi, np.pi, n)
    return A, B


def ragged_case(seed=0, layout=LAYOUT, degenerate=True):
    """The five-frame layout: ground truth spread over the scene, predictions
    around ground-truth boxes (or anywhere, in frames without ground truth), the
    degenerate pairs planted in the last frame (unless ``degenerate`` is off: their
    cross pairs hold many IoUs of exactly 1/2), classes 1-3."""
    r = np.random.default_rng(seed)
    dp, dg = degenerate_pairs()
    P, G = [], []
    for f, (n, m) in enumerate(layout):
        g = random_pairs(m, 100 + seed + f)[0]
        if m:
            src = g[r.integers(0, m, n)]
            p = random_pairs(n, 200 + seed + f)[0]
            p[:, :3] = src[:, :3] + r.normal(0, 1.0, (n, 3))
            half = r.random(n) < 0.5  # half the predictions are near copies of a ground-truth box
            p[half, 3:] = src[half, 3:] + r.normal(0, 0.05, (int(half.sum()), 4))
        else:
            p = random_pairs(n, 200 + seed + f)[0]
        if degenerate and (n, m) == layout[-1]:
            k = min(len(dp), n, m)
            p[:k], g[:k] = dp[:k], dg[:k]
        P.append(p)
        G.append(g)
    poff, goff, pair_off = ragged_offsets([n for n, _ in layout], [m for _, m in layout])
    pred, gt = np.concatenate(P).astype(np.float32).astype(np.float64), np.concatenate(G).astype(np.float32).astype(np.float64)
    return pred, gt, poff, goff, pair_off, r.integers(1, 4, len(pred)), r.integers(1, 4, len(gt))


_GOLDEN = {}


def golden_ragged(seed=0, degenerate=True):
    """(case, golden BEV IoU, golden 3D IoU) of :func:`ragged_case`, computed once."""
    if (seed, degenerate) not in _GOLDEN:
        case = ragged_case(seed, degenerate=degenerate)
        pred, gt, poff, goff, pair_off = case[:5]
        bev, v3 = np.zeros(pair_off[-1]), np.zeros(pair_off[-1])
        for f in range(len(poff) - 1):
            g = gt[goff[f]:goff[f + 1]]
            for i in range(poff[f], poff[f + 1]):
                o = pair_off[f] + (i - poff[f]) * len(g)
                bev[o:o + len(g)] = golden.rotated_iou_bev(pred[i], g)
                v3[o:o + len(g)] = golden.rotated_iou_3d(pred[i], g)
        _GOLDEN[seed, degenerate] = (case, bev, v3)
    return _GOLDEN[seed, degenerate]


# ------------------------------------------------------------------------------- golden
def test_golden_iou3d_hand_cases():
    a = np.array([1.0, 2.0, 0.5, 4.0, 2.0, 1.5, 0.3])
    assert golden.rotated_iou_3d(a, [a])[0] == pytest.approx(1.0, abs=1e-12)
    # shift d along a box of length L: BEV (L - d) / (L + d); same height, so 3D is the same ratio
    L, d = 4.0, 1.0
    b = a.copy()
    b[0] += d * np.cos(a[6])
    b[1] += d * np.sin(a[6])
    assert golden.rotated_iou_bev(a, [b])[0] == pytest.approx((L - d) / (L + d), abs=1e-12)
    assert golden.rotated_iou_3d(a, [b])[0] == pytest.approx((L - d) / (L + d), abs=1e-12)
    # half the height overlaps: the intersection volume halves
    c = a.copy()
    c[2] += a[5] / 2
    v = a[3] * a[4] * a[5]
    assert golden.rotated_iou_3d(a, [c])[0] == pytest.approx((v / 2) / (2 * v - v / 2), abs=1e-12)
    # disjoint in z: no volume, full BEV overlap
    e = a.copy()
    e[2] += 2 * a[5]
    assert golden.rotated_iou_3d(a, [e])[0] == 0.0 and golden.rotated_iou_bev(a, [e])[0] == pytest.approx(1.0)
    # 45-degree square in a square: the octagon 8 (sqrt 2 - 1) of tests/test_ops_cpu.py; equal heights
    s = np.array([0, 0, 0, 2, 2, 1, 0.0])
    r45 = np.array([0, 0, 0, 2, 2, 1, np.pi / 4])
    inter = 8 * (np.sqrt(2) - 1)
    assert golden.rotated_iou_3d(s, [r45])[0] == pytest.approx(inter / (8 - inter), rel=1e-9)
    assert golden.rotated_iou_3d(s, []).shape == (0,)


# ------------------------------------------------------------------------------- NumPy twin
@pytest.mark.parametrize("which", ["random", "degenerate"])
def test_twin_matches_golden(which):
    A, B = random_pairs(400, 0) if which == "random" else degenerate_pairs()
    gb = np.array([golden.rotated_iou_bev(a, b[None])[0] for a, b in zip(A, B)])
    g3 = np.array([golden.rotated_iou_3d(a, b[None])[0] for a, b in zip(A, B)])
    assert (gb > 0).mean() > 0.5  # the pairs do overlap
    bev, v3 = iou_pairs_np(A, B)
    print("max |twin - golden|:", np.abs(bev - gb).max(), np.abs(v3 - g3).max())
    np.testing.assert_allclose(bev, gb, rtol=0, atol=1e-9)
    np.testing.assert_allclose(v3, g3, rtol=0, atol=1e-9)


def test_ragged_layout_and_class_mask():
    (pred, gt, poff, goff, pair_off, pc, gc), gbev, g3 = golden_ragged()
    assert list(np.diff(pair_off)) == [n * m for n, m in LAYOUT]
    frame, first = tile_table(poff, goff)
    assert list(frame) == [2, 3, 3, 4, 4, 4] and list(first) == [0, 0, 64, 0, 64, 128]  # empty frames: no tile
    bev, v3, off = box3d_iou_ragged(pred, gt, poff, goff, device="cpu")
    assert np.array_equal(off, pair_off) and bev.shape == v3.shape == (pair_off[-1],)
    np.testing.assert_allclose(bev, gbev, rtol=0, atol=1e-9)  # offsets and row-major order: element by element
    np.testing.assert_allclose(v3, g3, rtol=0, atol=1e-9)
    assert (gbev > 0).sum() > 500 and (g3 > 0).sum() > 300
    # class arrays: pairs of different classes are 0, the others unchanged
    mb, m3, _ = box3d_iou_ragged(pred, gt, poff, goff, pc, gc, device="cpu")
    same = np.concatenate([(pc[poff[f]:poff[f + 1], None] == gc[None, goff[f]:goff[f + 1]]).ravel()
                           for f in range(len(LAYOUT))])
    assert 0.2 < same.mean() < 0.5
    np.testing.assert_array_equal(mb, np.where(same, bev, 0.0))
    np.testing.assert_array_equal(m3, np.where(same, v3, 0.0))
    with pytest.raises(ValueError):
        box3d_iou_ragged(pred, gt, poff, goff, pc, None, device="cpu")
    with pytest.raises(ValueError):
        box3d_iou_ragged(pred, gt, poff[:-1], goff, device="cpu")
    # a run whose pair count does not fit int32 is refused before anything is allocated
    big = np.zeros((70000, 7))
    with pytest.raises(ValueError, match="int32"):
        box3d_iou_ragged(big, big, [0, 70000], [0, 70000], device="cpu")


# ------------------------------------------------------------------------------- evaluator
def _gt_frames(n_frames=4, per=4, seed=3):
    """Well separated ground truth, one class, [per, 8] per frame."""
    r = np.random.default_rng(seed)
    out = {}
    for s in range(n_frames):
        g = np.zeros((per, 8))
        g[:, 0], g[:, 1] = 10.0 + 15.0 * np.arange(per), r.uniform(-20, 20, per)
        g[:, 2], g[:, 3:6], g[:, 6], g[:, 7] = -1.0, (4.0, 2.0, 1.5), r.uniform(-np.pi, np.pi, per), 1
        out[s] = g
    return out


def _as_pred(g, scores):
    return np.concatenate([g[:, :7], np.asarray(scores, np.float64)[:, None], g[:, 7:8]], 1)


def test_evaluator_perfect_predictions_and_false_positives():
    for metric in ("bev", "3d"):
        ev = DetectionEvaluator3D(metric=metric, device="cpu")
        for s, g in _gt_frames().items():
            fp = np.array([[200.0, 0, -1, 4, 2, 1.5, 0, 0.01, 1]])  # far away, lowest score
            ev.add_prediction(s, np.concatenate([_as_pred(g, 0.9 - 0.1 * np.arange(len(g))), fp]))
            ev.add_ground_truth(s, g)
        s = ev.summary()
        np.testing.assert_allclose(s.ap, PERFECT_AP, atol=1e-12)
        assert s.matched_images == 4 and list(s.map_by_iou) == [0.25, 0.5, 0.7]
        assert s.as_dict(["Car"])["map"] == {k: pytest.approx(PERFECT_AP) for k in ("0.25", "0.5", "0.7")}


def test_evaluator_shifted_boxes_exact_ap():
    """2 frames x 2 ground-truth boxes; in each frame the second prediction is shifted by
    L / 4 along its length, BEV IoU (L - L/4) / (L + L/4) = 0.6: a match at 0.25 and 0.5,
    a miss at 0.7.  Scores 0.9 (exact), 0.8 (shifted), 0.7 (exact), 0.6 (shifted), then
    the two false positives 0.1, 0.05."""
    gts = _gt_frames(2, 2)
    ev = DetectionEvaluator3D(metric="bev", device="cpu")
    for s, g in gts.items():
        p = _as_pred(g, [0.9 - 0.2 * s, 0.8 - 0.2 * s])
        p[1, 0] += 1.0 * np.cos(g[1, 6])
        p[1, 1] += 1.0 * np.sin(g[1, 6])
        fp = np.array([[200.0, 0, -1, 4, 2, 1.5, 0, 0.1 - 0.05 * s, 1]])
        ev.add_prediction(s, np.concatenate([p, fp]))
        ev.add_ground_truth(s, g)
    _, iou, off = ev.ious()
    assert iou[off[0]:off[1]].reshape(3, 2)[1, 1] == pytest.approx(0.6, abs=1e-12)
    tp = ev.stats()[0]
    order = np.argsort(-ev.stats()[1])
    assert tp[order].astype(int).tolist() == [[1, 1, 1], [1, 1, 0], [1, 1, 1], [1, 1, 0], [0, 0, 0], [0, 0, 0]]
    s = ev.summary()
    # at 0.25 / 0.5 the four matches come first: recall 1 at precision 1
    np.testing.assert_allclose(s.ap[0, :2], PERFECT_AP, atol=1e-12)
    # at 0.7, by hand: TP 1 0 1 0 0 0 over 4 ground-truth boxes
    recall = np.array([1, 1, 2, 2, 2, 2]) / 4
    precision = np.array([1, 1, 2, 2, 2, 2]) / np.arange(1, 7)
    assert s.ap[0, 2] == pytest.approx(compute_ap(recall, precision)[0], abs=1e-12)
    assert 0.3 < s.ap[0, 2] < 0.6


def test_evaluator_centerpoint_boxes_and_gt_z_offset():
    g = _gt_frames(1, 3)[0]
    b9 = np.zeros((3, 9))
    b9[:, :6], b9[:, 6:8], b9[:, 8] = g[:, :6], (7.0, -3.0), g[:, 6]  # vx, vy before the yaw
    np.testing.assert_array_equal(boxes7(b9), g[:, :7])
    np.testing.assert_array_equal(boxes7(g[:, :7]), g[:, :7])
    for metric, shifted_ap in (("bev", PERFECT_AP), ("3d", 0.0)):
        for dz, want in ((0.0, PERFECT_AP), (1.5, shifted_ap)):  # a whole box height apart: no volume in common
            ev = DetectionEvaluator3D(metric=metric, device="cpu")
            ev.add_detections(0, {"pred_boxes": b9.astype(np.float32), "pred_scores": np.array([0.9, 0.8, 0.7]),
                                  "pred_labels": np.ones(3, np.int64)})
            gg = g.copy()
            gg[:, 2] += dz
            ev.add_ground_truth(0, gg)
            np.testing.assert_allclose(ev.summary().ap, want, atol=1e-6)


# ------------------------------------------------------------------------------- messages
def test_gt3d_from_msg_round_trips():
    from triton_client_amd.inference import boxes_to_detection3d, boxes_to_jsk, gt3d_from_msg
    from triton_client_amd.ros import msgs

    r = np.random.default_rng(5)
    box = np.concatenate([r.uniform(-50, 50, (6, 3)), r.uniform(0.3, 12, (6, 3)), r.uniform(-np.pi, np.pi, (6, 1))], 1)
    lab = r.integers(1, 4, 6)
    pred = {"pred_boxes": box, "pred_scores": np.ones(6, np.float32), "pred_labels": lab}
    want = np.concatenate([box, lab[:, None]], 1)
    hdr = msgs.Header(seq=7)
    m = boxes_to_jsk(pred, np.arange(6), hdr)
    seq, g = gt3d_from_msg(m)  # from the publisher's columns
    assert seq == 7 and not m.boxes.built
    np.testing.assert_allclose(g, want, rtol=0, atol=1e-12)
    assert m.boxes[0].dimensions.x == box[0, 4]  # the jsk swap is on the wire
    np.testing.assert_allclose(gt3d_from_msg(m)[1], want, rtol=0, atol=1e-12)  # from the built objects
    seq, g = gt3d_from_msg(boxes_to_detection3d(pred, range(6), hdr))
    assert seq == 7
    np.testing.assert_allclose(g, want, rtol=0, atol=1e-12)
    assert gt3d_from_msg(msgs.BoundingBoxArray(header=hdr))[1].shape == (0, 8)


# ------------------------------------------------------------------------------- end to end
class OracleDetector3D:
    """The recorder's ground truth of each sweep as detections, plus one
    low-scored false positive; CenterPoint-style 9-column boxes when asked."""
    names = ["Car", "Pedestrian", "Cyclist"]

    def __init__(self, nine=False):
        self.nine, self.calls = nine, []

    def detect(self, clouds):
        from triton_client_amd.cli.record import synthetic_gt3d

        self.calls.append(len(clouds))
        out = []
        for c in clouds:
            g = synthetic_gt3d(c.header.seq)
            n = len(g["pred_labels"])
            box = np.concatenate([g["pred_boxes"], [[150.0, 0, 0, 2, 2, 2, 0]]]).astype(np.float32)
            if self.nine:
                box = np.concatenate([box[:, :6], np.full((n + 1, 2), 5.0, np.float32), box[:, 6:]], 1)
            out.append({"pred_boxes": box, "pred_scores": np.r_[0.9 - 0.1 * np.arange(n), 0.01].astype(np.float32),
                        "pred_labels": np.r_[g["pred_labels"], 1]})
        return out


PARAMS = {"sub_topic": "/ai_test_field/sensors/os_cloud_node/points", "gt_topic": "/detections_3d_gt"}


@pytest.fixture(scope="module")
def lidar_bag(tmp_path_factory):
    from triton_client_amd.cli import record

    path = str(tmp_path_factory.mktemp("bag3d") / "pc_gt.bag")
    assert record.main([path, "--frames", "5", "--no-camera", "--lidar", "--gt", "--rings", "8", "--columns", "64"]) == 0
    return path


def test_record_writes_gt3d_and_keeps_other_output(lidar_bag, tmp_path):
    from triton_client_amd.cli import record
    from triton_client_amd.inference import gt3d_from_msg
    from triton_client_amd.ros import Bag

    with Bag(lidar_bag) as b:
        ms = list(b.read_messages())
    gt = [m for t, m, _ in ms if t == "/detections_3d_gt"]
    assert len(gt) == 5 and sum(t == PARAMS["sub_topic"] for t, _, _ in ms) == 5
    g = record.synthetic_gt3d(3)
    np.testing.assert_allclose(gt3d_from_msg(gt[3])[1], np.c_[g["pred_boxes"], g["pred_labels"]], atol=1e-12)
    # without --gt the sweeps are written as before: same bytes with and without the new flag's default
    a, c = str(tmp_path / "a.bag"), str(tmp_path / "c.bag")
    args = ["--frames", "2", "--no-camera", "--lidar", "--rings", "8", "--columns", "64"]
    assert record.main([a] + args) == 0 and record.main([c] + args + ["--gt3d-topic", "/other"]) == 0
    assert open(a, "rb").read() == open(c, "rb").read()
    with Bag(a) as b:
        assert {t for t, _, _ in b.read_messages()} == {PARAMS["sub_topic"]}


@pytest.mark.parametrize("nine", [False, True])
def test_evaluate_bag_with_oracle_engine(lidar_bag, nine):
    from triton_client_amd.inference import EvaluateInference3D

    eng = OracleDetector3D(nine)
    ev = EvaluateInference3D(engine=eng, params=PARAMS, metrics_port=None, metric="3d", device="cpu")
    s = ev.evaluate_bag(lidar_bag, batch=2)
    assert eng.calls == [2, 2, 1] and s.matched_images == s.images == 5
    np.testing.assert_allclose(s.ap, PERFECT_AP, atol=1e-6)  # boxes went through fp32: IoU 1 - 1e-7
    assert set(ev.as_dict()["per_class"]) <= {"Car", "Pedestrian", "Cyclist"}
    # ground truth labelled on clouds lifted by a box height and more: no 3D match, BEV unchanged
    for metric, want in (("3d", 0.0), ("bev", PERFECT_AP)):
        ev = EvaluateInference3D(engine=OracleDetector3D(), params=PARAMS, metrics_port=None, metric=metric,
                                 gt_z_offset=3.0, device="cpu")
        np.testing.assert_allclose(ev.evaluate_bag(lidar_bag).ap, want, atol=1e-6)
    # the score floor drops the false positives
    ev = EvaluateInference3D(engine=OracleDetector3D(), params=PARAMS, metrics_port=None, conf_thres=0.05, device="cpu")
    ev.evaluate_bag(lidar_bag)
    assert all((p[:, 7] >= 0.05).all() for p in ev.evaluator.preds.values())


def test_evaluate_live_over_topic_bus(lidar_bag):
    from triton_client_amd.inference import EvaluateInference3D
    from triton_client_amd.ros import Bag, TopicBus

    with Bag(lidar_bag) as b:
        ms = list(b.read_messages())
    clouds = {m.header.seq: m for t, m, _ in ms if t == PARAMS["sub_topic"]}
    gts = {m.header.seq: m for t, m, _ in ms if t == PARAMS["gt_topic"]}
    bus = TopicBus()
    ev = EvaluateInference3D(engine=OracleDetector3D(), params=PARAMS, bus=bus, metrics_port=None, device="cpu")
    ev.start_inference(spin=False)
    for s in (3, 1):  # ground truth before its cloud ...
        bus.publish(PARAMS["gt_topic"], gts[s])
    for s in range(5):
        bus.publish(PARAMS["sub_topic"], clouds[s])
    for s in (0, 4, 2):  # ... and after
        bus.publish(PARAMS["gt_topic"], gts[s])
    bus.publish(PARAMS["sub_topic"], clouds[0])  # the bag loops: done
    bus.publish(PARAMS["gt_topic"], gts[0])
    assert ev.done.wait(30)
    s = ev.finish()
    bus.close()
    assert s.matched_images == 5
    np.testing.assert_allclose(s.ap, PERFECT_AP, atol=1e-6)


def test_cli_evaluate3d_json(lidar_bag, tmp_path):
    from triton_client_amd.cli import evaluate3d

    f = evaluate3d.parse_args([])
    assert (f.model_name, f.metric, f.iou, f.eval_port, f.gt_z_offset) == ("pointpillar_kitti", "bev", "0.25,0.5,0.7", 7658, 0.0)
    assert f.conf_thres < 0.1 and f.params.endswith("client_parameter_3d.yaml")
    js = str(tmp_path / "eval3d.json")
    assert evaluate3d.main(["--bag", lidar_bag, "--engine", "local", "--device", "cpu", "--metric", "3d",
                            "--iou", "0.3,0.6", "--eval-port", "0", "--json", js, "--frames-per-step", "2"]) == 0
    s = json.load(open(js))
    assert s["matched_images"] == 5 and s["metric"] == "3d" and s["iou_thresholds"] == [0.3, 0.6]
    assert set(s["map"]) == {"0.3", "0.6"} and all(0.0 <= v <= 1.0 for v in s["map"].values())
