"""The LiDAR driver's per-cloud record (``CloudResult``) and its table of side outputs: every
option publishes the same bytes whatever else is on, in one order, live and from a bag."""
import functools
import itertools

import numpy as np
import pytest

from test_range2d import AXES, _det_msg
from triton_client_amd.inference.engines import Detector3D
from triton_client_amd.inference.ros_inference3d import SIDE_OUTPUTS, CloudResult, RosInference3D
from triton_client_amd.ops import points_in_boxes as pib
from triton_client_amd.ops.depth_image import DepthOptions
from triton_client_amd.ops.range2d import Calibration
from triton_client_amd.ros import compat, msgs, rosmsg
from triton_client_amd.ros.bus import TopicBus
from triton_client_amd.utils.bev import BevView

F = np.float32
NS = 10 ** 9
NAMES = ("bev", "points", "tracks", "ranged", "depth")  # the publishing order, after the box message
TOPIC = {"box": "/o", "bev": "/bev", "points": "/pts", "tracks": "/trk", "ranged": "/ranged", "depth": "/depth"}
TYPE = {"box": msgs.BoundingBoxArray, "bev": msgs.Image, "points": msgs.PointCloud2, "tracks": msgs.BoundingBoxArray,
        "ranged": msgs.Detection2DArray, "depth": msgs.Image}
SUBSETS = [frozenset(c) for k in range(6) for c in itertools.combinations(NAMES, k)]
SIDE_METHODS = ("render_bev", "label_points", "range_detections", "depth_images", "tracker")

# a 64 x 48 camera looking along the LiDAR's x axis, and a 128 x 64 picture from above
CAL = Calibration(np.array([[40.0, 0, 32, 0], [0, 40.0, 24, 0], [0, 0, 1, 0]]),
                  np.concatenate([np.concatenate([AXES, [[0.0], [-0.08], [-0.27]]], 1), [[0, 0, 0, 1]]], 0))
OPTS = DepthOptions(64, 48)
VIEW = BevView(x_range=(0.0, 25.6), y_range=(-6.4, 6.4), res=0.2)


def _depth_of(seq):
    return 10.0 + 0.2 * seq


class _Engine:
    """A CPU engine by duck typing, with none of the side methods: two boxes on the cloud's wall."""
    names = ["Car", "Pedestrian", "Cyclist"]
    z_offset, normalize, label_base = 0.0, True, 1

    def detect(self, clouds):
        return [{"pred_boxes": np.array([[_depth_of(c.header.seq), y, -0.5, 1.0, 2.0, 1.5, 0.1] for y in (-1.5, 1.5)], F),
                 "pred_scores": np.array([0.9, 0.8], F), "pred_labels": np.array([2, 2])} for c in clouds]


class _OwnLabels(_Engine):
    """An engine that labels the points itself."""
    def __init__(self):
        self.label_calls = []

    def label_points(self, clouds, preds, idx_per_cloud=None):
        self.label_calls.append([c.header.seq for c in clouds])
        return Detector3D.label_points(self, clouds, preds, idx_per_cloud)


def _messages():
    """Four clouds 0.1 s apart, each a wall of 300 points; camera messages 3 ms after clouds 1, 2 and 4
    (cloud 3 finds no partner), each with one box on the wall and one on empty sky."""
    clouds = []
    for s in (1, 2, 3, 4):
        rng = np.random.default_rng(s)
        wall = np.stack([_depth_of(s) + rng.uniform(-0.05, 0.05, 300), rng.uniform(-3, 3, 300),
                         rng.uniform(-1.5, 0.5, 300), rng.uniform(0, 1, 300)], 1).astype(F)
        t = 10 * NS + s * NS // 10
        clouds.append(compat.create_cloud_xyzi(wall, msgs.Header(seq=s, stamp=msgs.Time(t // NS, t % NS),
                                                                 frame_id="os")))
    cams = [_det_msg(10 * NS + s * NS // 10 + 3_000_000, [(32, 26, 16, 6), (32, -40, 8, 8)], seq=100 + s)
            for s in (1, 2, 4)]
    return clouds, cams


def _options(on):
    kw = {}
    if "bev" in on:
        kw.update(bev_topic=TOPIC["bev"], bev_view=VIEW)
    if "points" in on:
        kw.update(points_topic=TOPIC["points"])
    if "tracks" in on:
        kw.update(tracks_topic=TOPIC["tracks"])
    if "ranged" in on:
        kw.update(ranged_topic=TOPIC["ranged"], camera_detections_topic="/cam", calibration=CAL)
    if "depth" in on:
        kw.update(depth_topic=TOPIC["depth"], depth_options=OPTS, depth_frame_id="cam", calibration=CAL)
    return kw


@functools.lru_cache(maxsize=None)
def _drive(on, batched, engine=_Engine):
    """The four clouds through the in-process bus, one message per callback or micro-batched:
    ({name: [serialised message]}, [(name, seq) in the order the driver published], engine)."""
    clouds, cams = _messages()
    bus = TopicBus()
    seen, order = {n: [] for n in TOPIC}, []
    for n in TOPIC:
        compat.Subscriber(TOPIC[n], TYPE[n], lambda m, n=n: seen[n].append(rosmsg.serialize(m)), bus=bus)
    eng = engine()
    drv = RosInference3D(engine=eng, params={"sub_topic": "/pc", "pub_topic": TOPIC["box"]}, bus=bus, queue_size=64,
                         **(dict(batch=2, workers=2) if batched else {}), **_options(on))
    drv.start_inference(spin=False)
    assert set(drv.side_pubs) == set(on)
    for n, p in [("box", drv.pub), *drv.side_pubs.items()]:
        def publish(m, n=n, send=p.publish):
            order.append((n, m.header.seq))
            send(m)
        p.publish = publish
    cam_pub = compat.Publisher("/cam", msgs.Detection2DArray, bus=bus)
    for m in cams:
        cam_pub.publish(m)
    assert bus.wait_idle()  # the camera topic has its own dispatch thread: the pairer holds all three first
    pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
    for c in clouds:
        pub.publish(c)
    runner = drv.runner
    drv.stop()
    bus.close()
    assert (runner is not None) == batched and (runner is None or not runner.errors), runner and runner.errors
    return seen, order, eng


def test_the_table_names_the_record_fields_in_publishing_order():
    assert tuple(n for n, _ in SIDE_OUTPUTS) == NAMES
    assert {n: t for n, t in SIDE_OUTPUTS} == {**{n: TYPE[n] for n in NAMES}, "tracks": None}  # the box message's type
    r = CloudResult("boxes", {"k": 1})
    assert (r.boxes, r.pred) == ("boxes", {"k": 1}) and all(getattr(r, n) is None for n in NAMES)


def test_every_output_of_the_full_run_says_something():
    seen, _, eng = _drive(frozenset(NAMES), False)
    assert not isinstance(eng, Detector3D) and not any(hasattr(eng, n) for n in SIDE_METHODS)
    assert all(len(seen[n]) == 4 for n in ("box", "bev", "points", "tracks", "depth")) and len(seen["ranged"]) == 3
    assert all(len(set(seen[n])) == len(seen[n]) for n in seen)  # every cloud its own bytes
    assert all(len(b) > 200 for n in seen for b in seen[n])


@pytest.mark.parametrize("on", SUBSETS, ids=lambda s: "+".join(n for n in NAMES if n in s) or "none")
@pytest.mark.parametrize("batched", [False, True], ids=["one_by_one", "batch2_workers2"])
def test_each_option_publishes_the_same_bytes_whatever_else_is_on(on, batched):
    seen, order, _ = _drive(on, batched)
    assert seen["box"] == _drive(frozenset(), False)[0]["box"] and len(seen["box"]) == 4
    for n in NAMES:
        assert seen[n] == (_drive(frozenset([n]), False)[0][n] if n in on else []), n
    # per cloud: box, bev, points, tracks, ranged, depth; seqs ascend (cloud 3 has no ranged message, and the
    # others' carry their camera message's header: seq 100 + the cloud's)
    assert order == [(n, 100 + s if n == "ranged" else s) for s in (1, 2, 3, 4) for n in ("box",) + NAMES
                     if n == "box" or (n in on and (n, s) != ("ranged", 3))]


@pytest.mark.parametrize("batched", [False, True])
def test_an_engine_with_its_own_label_points_has_it_called(batched):
    seen, _, eng = _drive(frozenset(NAMES), batched, _OwnLabels)
    assert sorted(s for call in eng.label_calls for s in call) == [1, 2, 3, 4]
    assert seen == _drive(frozenset(NAMES), False)[0]
    rec = np.frombuffer(rosmsg.deserialize(seen["points"][0], "sensor_msgs/PointCloud2").data, pib.RECORD_DTYPE)
    assert (rec["instance"] >= 0).sum() > 10 and (rec["instance"] == -1).sum() > 10


def test_bag_replay_writes_the_union_of_the_single_option_bags(tmp_path):
    from triton_client_amd.inference import BagInference3D
    from triton_client_amd.ros import Bag

    clouds, cams = _messages()
    src = str(tmp_path / "rig.bag")
    with Bag(src, "w") as b:  # the camera messages lie behind their clouds: the first pass finds them
        for c in clouds:
            b.write("/pc", c)
        for m in cams:
            b.write("/cam", m)

    def replay(on):
        out = str(tmp_path / ("_".join(sorted(on)) + ".bag"))
        drv = BagInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": TOPIC["box"]}, bagfile=src,
                             out_bag=out, batch=3, **_options(on))
        assert drv.start_inference() == 4
        per_topic = {}
        with Bag(out) as b:
            for t, m, _ in b.read_messages():
                per_topic.setdefault(t, []).append(rosmsg.serialize(m))
        return per_topic, drv

    full, drv = replay(NAMES)
    union = {}
    for n in NAMES:
        single, _ = replay([n])
        assert set(single) == {"/pc", TOPIC["box"], TOPIC[n]}
        for t, ms in single.items():
            assert union.setdefault(t, ms) == ms  # the clouds and the box messages: the same in every bag
    assert full == union and [len(full[TOPIC[n]]) for n in NAMES] == [4, 4, 4, 3, 4]
    # the bag holds what the live driver publishes
    live = _drive(frozenset(NAMES), False)[0]
    assert all(full[TOPIC[n]] == live[n] for n in TOPIC)
    assert [s for s, _ in drv.results] == [1, 2, 3, 4]
    for s, pred in drv.results:
        assert (pred["ranged"] is None) == (s == 3) and isinstance(pred["depth"], msgs.Image)
        assert len(pred["track_ids"]) == len(pred["track_hits"]) == len(pred["track_vel"]) == 2
        assert (np.asarray(pred["track_ids"]) > 0).all()
