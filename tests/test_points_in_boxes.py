"""Points in boxes on the host: the float32 definition (ops/points_in_boxes.py) against its
float64 reference, the exact cases, the labelled-cloud message of the 3D drivers and the
evaluator's ``min_gt_points``."""
import json

import numpy as np
import pytest

from triton_client_amd.ops import points_in_boxes as pib
from triton_client_amd.ros import compat, msgs

F = np.float32


# ------------------------------------------------------------ definition vs float64 reference
def _generate(seed, k=64, n=20000):
    """Random boxes (centres in the KITTI range, dims 0.5-12 m, yaw in +-7 rad) and points drawn
    around them (centre +- 0.75 * dims * U(-1, 1))."""
    r = np.random.default_rng(seed)
    box = np.empty((k, 7), F)
    box[:, 0], box[:, 1], box[:, 2] = r.uniform(0, 69.12, k), r.uniform(-39.68, 39.68, k), r.uniform(-3, 1, k)
    box[:, 3:6] = r.uniform(0.5, 12.0, (k, 3))
    box[:, 6] = r.uniform(-7, 7, k)
    j = r.integers(0, k, n)
    pts = (box[j, :3] + 0.75 * box[j, 3:6] * r.uniform(-1, 1, (n, 3))).astype(F)
    return pts, box, r.uniform(0.05, 1, k).astype(F)


def _check_against_ref(inside_fn, seeds):
    """→ (pairs, in-band pairs, inside pairs); asserts agreement on every pair outside the band."""
    pairs = band_n = inside_n = 0
    for seed in seeds:
        pts, box, sc = _generate(seed)
        got = inside_fn(pts, box, sc)
        want, band = pib.points_in_boxes_ref(pts, box, sc)
        bad = (got != want) & ~band
        assert not bad.any(), (seed, int(bad.sum()))
        pairs, band_n, inside_n = pairs + got.size, band_n + int(band.sum()), inside_n + int(want.sum())
    return pairs, band_n, inside_n


def _definition_inside(pts, box, sc):
    return pib.points_in_boxes_numpy(pts, box, sc, return_inside=True)[2]


def test_definition_agrees_with_float64_outside_the_band():
    pairs, band_n, inside_n = _check_against_ref(_definition_inside, range(20))
    print(f"pairs {pairs}, in band {band_n} ({band_n / pairs:.2e}), inside {inside_n}")
    assert pairs == 20 * 64 * 20000 and inside_n > 50000
    assert band_n / pairs <= 1e-4  # a cap, not a measurement: the band must stay too thin to hide a defect


@pytest.mark.parametrize("defect", ["swapped_s_sign", "open_face"])
def test_a_deliberate_defect_breaks_the_check(defect, monkeypatch):
    def col(x, y, z, row):
        ex, ey, ez = x - row[0], y - row[1], z - row[2]
        if defect == "swapped_s_sign":
            lx, ly = (ex * row[6]) - (ey * row[7]), (ey * row[6]) + (ex * row[7])
            return (np.abs(lx) <= row[3]) & (np.abs(ly) <= row[4]) & (np.abs(ez) <= row[5])
        lx, ly = (ex * row[6]) + (ey * row[7]), (ey * row[6]) - (ex * row[7])
        return (np.abs(lx) < row[3]) & (np.abs(ly) < row[4]) & (np.abs(ez) < row[5])

    monkeypatch.setattr(pib, "_inside_column", col)
    if defect == "swapped_s_sign":
        with pytest.raises(AssertionError):
            _check_against_ref(_definition_inside, range(2))
    else:  # an open face shows only on a face: the exact cases catch it
        with pytest.raises(AssertionError):
            test_faces_edges_corners_are_inside_one_ulp_beyond_is_outside()


# ------------------------------------------------------------------------------- exact cases
BOX = np.array([[2.0, -1.0, 0.5, 4.0, 2.0, 1.0, 0.0]], F)  # faces at x 0 / 4, y -2 / 0, z 0 / 1


def _up(v):
    return np.nextafter(F(v), F(np.inf))


def _down(v):
    return np.nextafter(F(v), F(-np.inf))


def test_faces_edges_corners_are_inside_one_ulp_beyond_is_outside():
    inside = np.array([[4.0, -1.0, 0.5], [2.0, 0.0, 0.5], [2.0, -1.0, 1.0],  # faces
                       [4.0, 0.0, 0.5], [0.0, -1.0, 0.0], [2.0, -2.0, 1.0],  # edges
                       [4.0, 0.0, 1.0], [0.0, -2.0, 0.0], [0.0, 0.0, 1.0],  # corners
                       [2.0, -1.0, 0.5]], F)
    outside = np.array([[_up(4.0), -1.0, 0.5], [2.0, -1.0, _up(1.0)], [2.0, _down(-2.0), 0.5],
                        [_up(4.0), 0.0, 1.0], [4.0, 0.0, _up(1.0)]], F)
    owner, count = pib.points_in_boxes_numpy(np.concatenate([inside, outside]), BOX, [0.5])
    assert (owner[:len(inside)] == 0).all() and (owner[len(inside):] == -1).all()
    assert count.tolist() == [len(inside)] and owner.dtype == np.int32 and count.dtype == np.int32
    # all six faces of a box at the origin, where x - cx is the coordinate itself (next to a centre
    # far from 0 the subtraction rounds a point one ulp beyond the face onto it: that is the definition)
    o = np.array([[0.0, 0.0, 0.0, 4.0, 2.0, 1.0, 0.0]], F)
    on = np.array([[2, 0, 0], [-2, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0.5], [0, 0, -0.5], [2, -1, 0.5]], F)
    off = np.array([[_up(2), 0, 0], [_down(-2), 0, 0], [0, _up(1), 0], [0, _down(-1), 0], [0, 0, _up(0.5)],
                    [0, 0, _down(-0.5)], [_up(2), -1, 0.5], [2, -1, _up(0.5)]], F)
    owner, count = pib.points_in_boxes_numpy(np.concatenate([on, off]), o, [0.5])
    assert owner.tolist() == [0] * len(on) + [-1] * len(off) and count.tolist() == [len(on)]


def test_nan_points_bad_boxes_and_empty_inputs():
    pts = np.array([[2.0, -1.0, 0.5], [np.nan, -1.0, 0.5], [2.0, np.nan, 0.5], [2.0, -1.0, np.nan]], F)
    owner, count = pib.points_in_boxes_numpy(pts, BOX, [0.5])
    assert owner.tolist() == [0, -1, -1, -1] and count.tolist() == [1]
    for col, v in [(0, np.nan), (6, np.nan), (3, np.inf), (3, 0.0), (4, -2.0), (5, 0.0)]:
        b = BOX.copy()
        b[0, col] = v
        owner, count = pib.points_in_boxes_numpy(pts, np.concatenate([b, BOX]), [0.9, 0.5])
        assert owner.tolist() == [1, -1, -1, -1] and count.tolist() == [0, 1], (col, v)
        assert np.isnan(pib.box_table(b, [0.9])).all()
    owner, count = pib.points_in_boxes_numpy(pts, np.concatenate([BOX, BOX]), [np.nan, 0.5])  # the score is an entry
    assert owner.tolist() == [1, -1, -1, -1] and count.tolist() == [0, 1]
    owner, count = pib.points_in_boxes_numpy(pts, np.zeros((0, 7), F), [])
    assert owner.tolist() == [-1] * 4 and count.shape == (0,)
    owner, count = pib.points_in_boxes_numpy(np.zeros((0, 3), F), BOX, [0.5])
    assert owner.shape == (0,) and count.tolist() == [0]
    inside, band = pib.points_in_boxes_ref(np.zeros((0, 3), F), np.zeros((0, 7), F))
    assert inside.shape == band.shape == (0, 0)


def test_owner_is_the_best_score_ties_to_the_lowest_index_and_count_counts_all():
    big = np.array([[2.0, -1.0, 0.5, 8.0, 8.0, 8.0, 0.3]], F)
    boxes = np.concatenate([BOX, big, big])
    pts = np.array([[2.0, -1.0, 0.5], [2.0, -1.0, 3.0], [50.0, 0.0, 0.0]], F)
    owner, count = pib.points_in_boxes_numpy(pts, boxes, [0.4, 0.9, 0.2])
    assert owner.tolist() == [1, 1, -1] and count.tolist() == [1, 2, 2]
    owner, _ = pib.points_in_boxes_numpy(pts, boxes, [0.9, 0.4, 0.4])
    assert owner.tolist() == [0, 1, -1]
    owner, _ = pib.points_in_boxes_numpy(pts, boxes, [0.4, 0.4, 0.4])
    assert owner.tolist() == [0, 1, -1]


def test_nine_column_boxes_take_their_yaw_from_column_8():
    yaw = F(np.pi / 2)
    b7 = np.array([[0.0, 0.0, 0.0, 8.0, 1.0, 2.0, yaw]], F)
    b9 = np.array([[0.0, 0.0, 0.0, 8.0, 1.0, 2.0, 0.0, 0.0, yaw]], F)  # (vx, vy) = 0 read as a yaw would fail
    pts = np.array([[0.0, 3.0, 0.0], [3.0, 0.0, 0.0]], F)
    for b in (b7, b9):
        owner, _ = pib.points_in_boxes_numpy(pts, b, [0.5])
        assert owner.tolist() == [0, -1]
    t = pib.box_table(b9, [0.5])[0]
    assert t[6] == F(np.cos(np.float64(yaw))) and t[7] == F(np.sin(np.float64(yaw))) and t[3] == 4.0


# ----------------------------------------------------------------------------------- message
class _Engine:
    """A CPU engine (a Detector3D by duck typing only): boxes around the cloud's own points."""
    names = ["Car", "Pedestrian", "Cyclist"]
    z_offset, normalize, label_base = 1.5, True, 1

    def detect(self, clouds):
        out = []
        for c in clouds:
            p = pib.cloud_xyzi(c)
            p = p[~np.isnan(p).any(1)]
            k = min(6, len(p))
            box = np.zeros((k, 7), F)
            box[:, :3] = p[:: max(1, len(p) // k)][:k, :3]
            box[:, 3:6] = (6.0, 4.0, 3.0)
            box[:, 6] = np.linspace(-1.0, 2.0, k)
            out.append({"pred_boxes": box, "pred_scores": np.linspace(0.2, 0.9, k).astype(F),
                        "pred_labels": (np.arange(k) % 3 + 1).astype(np.int64)})
        return out


def _clouds(n=4):
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep
    out = []
    for s in range(n):
        pts = lidar_sweep(LidarSpec(rings=8, azimuth_steps=128, sensor_height=1.8), s)
        pts = np.frombuffer(pts.tobytes(), F).reshape(-1, 4).copy()
        pts[5, 1] = np.nan  # a NaN point stays in the labelled cloud, in place
        c = compat.create_cloud_xyzi(pts, msgs.Header(seq=s + 1, stamp=msgs.Time(5, s), frame_id="os"))
        c.height, c.width, c.is_dense = 8, c.width // 8, bool(s % 2)
        out.append(c)
    return out


def _drive(clouds, topic, jsk=True, batch=1, workers=1, labels=(2,), score_thresh=0.5):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.ros.bus import TopicBus

    bus = TopicBus()
    order, boxes, pts = [], [], []
    t = msgs.BoundingBoxArray if jsk else msgs.Detection3DArray
    compat.Subscriber("/pc_out", t, lambda m: (order.append(("b", m.header.seq)), boxes.append(m)), bus=bus)
    compat.Subscriber("/pc_pts", msgs.PointCloud2, lambda m: (order.append(("p", m.header.seq)), pts.append(m)),
                      bus=bus)
    drv = RosInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/pc_out"}, bus=bus, jsk=jsk,
                         batch=batch, workers=workers, queue_size=64, labels=labels, score_thresh=score_thresh,
                         **({"points_topic": topic} if topic else {}))
    drv.start_inference(spin=False)
    pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
    for c in clouds:
        pub.publish(c)
    drv.stop()
    bus.close()
    return boxes, pts, order


@pytest.mark.parametrize("jsk", [True, False])
def test_labelled_cloud_message(jsk):
    from triton_client_amd.inference.ros_inference3d import select_boxes
    from triton_client_amd.ros import rosmsg

    clouds = _clouds()
    boxes0, pts0, _ = _drive(clouds, None, jsk, labels=None, score_thresh=0.3)
    boxes, pts, _ = _drive(clouds, "/pc_pts", jsk, labels=None, score_thresh=0.3)
    assert pts0 == [] and len(pts) == len(boxes) == len(clouds)
    assert [rosmsg.serialize(m) for m in boxes0] == [rosmsg.serialize(m) for m in boxes]  # byte-identical
    owned = 0
    for c, bm, pm, pred in zip(clouds, boxes, pts, _Engine().detect(clouds)):
        assert (pm.header.seq, pm.header.stamp, pm.header.frame_id) == (c.header.seq, c.header.stamp, "os")
        assert (pm.height, pm.width, pm.is_dense, pm.point_step, pm.row_step) == (c.height, c.width, c.is_dense, 28,
                                                                                  28 * c.width)
        assert [(f.name, f.offset, f.datatype, f.count) for f in pm.fields] == [
            ("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1), ("intensity", 12, 7, 1), ("label", 16, 5, 1),
            ("instance", 20, 5, 1), ("score", 24, 7, 1)]
        rec = np.frombuffer(pm.data, pib.RECORD_DTYPE)
        src = np.frombuffer(c.data, np.uint32).reshape(-1, 4)
        assert len(rec) == c.width * c.height
        np.testing.assert_array_equal(np.frombuffer(pm.data, np.uint32).reshape(-1, 7)[:, :4], src)  # as sent
        # instance indexes the box message published for the same cloud
        published = bm.boxes if jsk else bm.detections
        idx = select_boxes(pred, None, 0.3)
        assert len(published) == len(idx) and rec["instance"].max() < len(published)
        owner, count = pib.points_in_boxes_numpy(pib.cloud_xyzi(c), pred["pred_boxes"][idx], pred["pred_scores"][idx])
        np.testing.assert_array_equal(rec["instance"], owner)
        has = rec["instance"] >= 0
        owned += int(has.sum())
        for i in np.flatnonzero(has)[:50]:
            b = published[rec["instance"][i]]
            lab, val = (b.label, b.value) if jsk else (b.results[0].id, b.results[0].score)
            assert rec["label"][i] == lab and rec["score"][i] == F(val)
        assert (rec["label"][~has] == 0).all() and (rec["score"][~has] == 0).all() and rec["instance"][5] == -1
        assert count.sum() >= has.sum()
    assert owned > 100
    # the cloud keeps every point also when the box message is empty
    _, pts, _ = _drive(clouds[:1], "/pc_pts", jsk, labels=(99,))
    rec = np.frombuffer(pts[0].data, pib.RECORD_DTYPE)
    assert len(rec) == clouds[0].width * clouds[0].height and (rec["instance"] == -1).all()


def test_micro_batched_driver_publishes_both_topics_in_seq_order():
    clouds = _clouds(6)
    boxes, pts, order = _drive(clouds, "/pc_pts", batch=2, workers=2, labels=None, score_thresh=0.3)
    seqs = [c.header.seq for c in clouds]
    assert [m.header.seq for m in boxes] == seqs and [m.header.seq for m in pts] == seqs
    assert sorted(order) == sorted([(k, s) for s in seqs for k in ("b", "p")])  # (the bus delivers per topic)
    one = _drive(clouds, "/pc_pts", labels=None, score_thresh=0.3)[1]  # the same clouds one at a time
    assert [p.data for p in pts] == [p.data for p in one] and len(one) == len(clouds)


def test_process_tuple_and_layout_fallbacks():
    from triton_client_amd.inference import RosInference3D

    clouds = _clouds(2)
    drv = RosInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, points_topic="/p")
    r = drv.process(clouds)[0]
    assert r.bev is None and isinstance(r.points, msgs.PointCloud2) and r.tracks is None
    plain = RosInference3D(engine=_Engine(), params={}).process(clouds)[0]
    assert (plain.bev, plain.points, plain.tracks, plain.ranged, plain.depth) == (None,) * 5
    # a FLOAT64 cloud without intensity: values cast to float32, intensity 0
    p = pib.cloud_xyzi(clouds[0])[:, :3].astype(np.float64)
    c64 = msgs.PointCloud2(header=msgs.Header(seq=9), height=1, width=len(p),
                           fields=[msgs.PointField("x", 0, 8, 1), msgs.PointField("y", 8, 8, 1),
                                   msgs.PointField("z", 16, 8, 1)], point_step=24, row_step=24 * len(p),
                           data=p.tobytes())
    lay = pib.cloud_layout(c64)
    assert not lay.device_ok and lay.offsets[3] == -1 and pib.cloud_layout(clouds[0]).device_ok
    box = np.array([[p[0, 0], p[0, 1], p[0, 2], 6.0, 6.0, 6.0, 0.2]], F)
    (owner, count, payload), = pib.PointLabeler("cpu").label([c64], [box], [[0.7]], [[3]])
    rec = np.frombuffer(payload, pib.RECORD_DTYPE)
    want, _ = pib.points_in_boxes_numpy(p.astype(F), box, [0.7])
    np.testing.assert_array_equal(owner, want)
    assert owner[0] == 0 and count[0] == (want == 0).sum() and (rec["intensity"] == 0).all()
    assert rec["label"][0] == 3 and rec["score"][0] == F(0.7)
    with pytest.raises(ValueError):
        pib.cloud_layout(msgs.PointCloud2(fields=[msgs.PointField("x", 0, 7, 1)]))


def test_cli_flags_and_bag3d_writes_the_topic(tmp_path):
    from triton_client_amd.cli import bag3d, evaluate3d, main3d, record
    from triton_client_amd.ros import Bag

    assert main3d.parse_args([]).points_topic == "" and main3d.parse_args(["--points-topic", "/p"]).points_topic == "/p"
    assert bag3d.parse_args(["--bag", "x"]).points_topic == ""
    assert evaluate3d.parse_args([]).min_gt_points == 0
    assert evaluate3d.parse_args(["--min-gt-points", "5"]).min_gt_points == 5
    pc = str(tmp_path / "pc.bag")
    assert record.main([pc, "--frames", "2", "--no-camera", "--lidar", "--rings", "8", "--columns", "128"]) == 0
    ob, ob0 = str(tmp_path / "o.bag"), str(tmp_path / "o0.bag")
    common = ["--bag", pc, "--engine", "local", "--device", "cpu", "--labels", "all", "--score-thresh", "0"]
    assert bag3d.main(common + ["--out-bag", ob, "--points-topic", "/labelled"]) == 0
    assert bag3d.main(common + ["--out-bag", ob0]) == 0
    with Bag(ob) as b:
        ms = list(b.read_messages())
    with Bag(ob0) as b:
        ms0 = list(b.read_messages())
    lab = [m for t, m, _ in ms if t == "/labelled"]
    src = [m for t, m, _ in ms if t not in ("/labelled", "/detections_3d")]
    assert len(lab) == 2 and len(ms0) == len(ms) - 2 and {t for t, _, _ in ms0} == {t for t, _, _ in ms} - {"/labelled"}
    for m, c in zip(lab, src):
        assert m.point_step == 28 and m.width * m.height == c.width * c.height and m.header.seq == c.header.seq
        assert len(m.data) == 28 * c.width * c.height


# --------------------------------------------------------------------------------- evaluator
PARAMS = {"sub_topic": "/pc", "gt_topic": "/gt"}
SEEN = np.array([10.0, 0.0, 0.0, 4.0, 2.0, 2.0, 0.3], F)
EMPTY = np.array([40.0, 20.0, 0.0, 4.0, 2.0, 2.0, -0.4], F)  # no point of any cloud inside


class _SeenOnly:
    """Detects the one object the sensor saw, perfectly."""
    names = ["Car"]

    def detect(self, clouds):
        return [{"pred_boxes": SEEN[None].copy(), "pred_scores": np.array([0.9], F),
                 "pred_labels": np.array([1], np.int64)} for _ in clouds]


def _eval_messages(n=3):
    from triton_client_amd.inference import boxes_to_jsk

    r = np.random.default_rng(0)
    out = []
    for s in range(n):
        hdr = msgs.Header(seq=s, frame_id="os")
        pts = np.concatenate([SEEN[:3] + r.uniform(-0.4, 0.4, (7, 3)), r.uniform(-5, 5, (50, 3)) + [-20, 0, 0]])
        cloud = compat.create_cloud_xyzi(np.c_[pts, np.ones(len(pts))].astype(F), hdr)
        gt = {"pred_boxes": np.stack([SEEN, EMPTY]), "pred_scores": np.ones(2, F), "pred_labels": np.array([1, 1])}
        out.append((cloud, boxes_to_jsk(gt, [0, 1], hdr)))
    return out


def _evaluate(order, min_gt_points, bag_path=None):
    from triton_client_amd.inference import EvaluateInference3D
    from triton_client_amd.ros import Bag

    kw = {"min_gt_points": min_gt_points} if min_gt_points is not None else {}
    ev = EvaluateInference3D(engine=_SeenOnly(), params=PARAMS, metrics_port=None, iouv=[0.5], device="cpu", **kw)
    pairs = _eval_messages()
    if order == "bag":
        with Bag(bag_path, "w") as b:
            for k, (c, g) in enumerate(pairs):  # both orders inside one bag
                for t, m in ((("/pc", c), ("/gt", g)) if k % 2 else (("/gt", g), ("/pc", c))):
                    b.write(t, m)
        ev.evaluate_bag(bag_path, batch=2)
    else:
        for c, g in pairs:
            if order == "cloud_first":
                ev.cloud_callback(c), ev.gt_callback(g)
            else:
                ev.gt_callback(g), ev.cloud_callback(c)
        ev.finish()
    return ev


def test_min_gt_points_drops_unseen_ground_truth(tmp_path):
    # by hand (compute_ap: end points (0, 1) and (1, 0), envelope, 101 samples, trapezoid):
    # with the empty box, one true positive of two ground truths per frame: recall 0.5 at precision 1,
    # the curve is 1 on [0, 0.5] and falls linearly to 0 at 1: AP = 0.5 + 0.25 = 0.75;
    # without it recall reaches 1 at precision 1 and only the closing sample at recall 1 reads 0:
    # AP = 1 - 0.5 * 0.01 = 0.995.  The rise is 0.245.
    base = _evaluate("cloud_first", None)
    assert base.summary.ap.shape == (1, 1) and base.summary.ap[0, 0] == pytest.approx(0.75, abs=1e-9)
    zero = _evaluate("cloud_first", 0)
    assert zero.as_dict() == base.as_dict() and "gt_dropped" not in zero.as_dict()  # 0: the parent's summary
    got = {}
    for order in ("cloud_first", "gt_first", "bag"):
        ev = _evaluate(order, 1, str(tmp_path / "e.bag"))
        assert ev.summary.ap[0, 0] == pytest.approx(0.995, abs=1e-9) and ev.summary.matched_images == 3
        assert ev.gt_dropped == 3 and not ev._held_clouds and not ev._held_gts
        got[order] = json.dumps(ev.as_dict(), sort_keys=True)
        assert ev.as_dict()["gt_dropped"] == 3 and ev.as_dict()["min_gt_points"] == 1
    assert got["cloud_first"] == got["gt_first"] == got["bag"]
    assert ev.summary.ap[0, 0] - base.summary.ap[0, 0] == pytest.approx(0.245, abs=1e-9)
    # 7 points lie in the seen box: it survives N = 7 and goes at N = 8
    assert _evaluate("gt_first", 7).gt_dropped == 3 and _evaluate("gt_first", 8).gt_dropped == 6


def test_evaluate3d_cli_min_gt_points(tmp_path):
    from triton_client_amd.cli import evaluate3d, record

    bag = str(tmp_path / "pc_gt.bag")
    assert record.main([bag, "--frames", "2", "--no-camera", "--lidar", "--gt", "--rings", "8", "--columns", "64"]) == 0
    js = str(tmp_path / "e.json")
    args = ["--bag", bag, "--engine", "local", "--device", "cpu", "--eval-port", "0", "--json", js]
    assert evaluate3d.main(args) == 0
    s0 = json.load(open(js))
    assert evaluate3d.main(args + ["--min-gt-points", "1000000"]) == 0
    s = json.load(open(js))
    assert "gt_dropped" not in s0 and s["min_gt_points"] == 1000000 and s["gt_dropped"] > 0 and s["per_class"] == {}
