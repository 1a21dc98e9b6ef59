"""The tracker's definition (ops/track3d.py) on crafted cases, its cut invariance, the ordered
stage of the micro-batched driver and the command-line flags.  Every crafted case takes a
tracker factory, so tests/test_track3d_gpu.py runs the same cases through ``tca_track3d``."""
import threading
import time

import numpy as np
import pytest

from triton_client_amd.ops import track3d as T
from triton_client_amd.ros import compat, msgs

F = np.float32
MS = 1_000_000  # nanoseconds


def cpu(**kw):
    gate2 = kw.pop("gate2", None)
    tr = T.Tracker3D(device="cpu", **kw)
    if gate2 is not None:
        tr.max_dist2[:] = gate2
    return tr


def P(xy, labels=1, vel=None):
    """A prediction of boxes centred at ``xy`` ([n, 2]); ``vel`` [n, 2]: 9-d boxes."""
    xy = np.asarray(xy, F).reshape(-1, 2)
    n = len(xy)
    b = np.zeros((n, 7 if vel is None else 9), F)
    b[:, :2] = xy
    b[:, 3:6] = (4.0, 2.0, 1.5)
    if vel is not None:
        b[:, 6:8] = np.asarray(vel, F).reshape(-1, 2)
    return {"pred_boxes": b, "pred_scores": np.full(n, 0.9, F),
            "pred_labels": np.broadcast_to(np.asarray(labels, np.int64), (n,)).copy()}


def ids_of(tr, pred, t_ms):
    return tr.track([pred], None, [int(t_ms) * MS])[0][0].tolist()


def finite_state(st):
    return all(np.isfinite(getattr(st, n)).all() for n, dt in T.FIELDS if dt is F)


# ----------------------------------------------------------------------- crafted cases
def case_crossing_9d(mk):
    """Two objects 0.2 m apart in y cross at 10 m/s each: 1 m per frame, a 0.5 m gate."""
    tr = mk(max_dist=0.5)
    got = []
    for k in range(6):
        a, b = (-2.5 + k, 0.0), (2.5 - k, 0.2)
        pair, vel = [a, b], [(10, 0), (-10, 0)]
        if k % 2:  # the published order changes from frame to frame
            pair, vel = pair[::-1], vel[::-1]
        r = ids_of(tr, P(pair, 1, vel), 100 * k)
        got.append(r[::-1] if k % 2 else r)
    assert got == [[1, 2]] * 6
    st = tr.state()
    assert st.next_id == 3 and st.hits[:2].tolist() == [6, 6]


def case_crossing_7d(mk):
    """7-d boxes: the first step is 0.1 m (dt 10 ms) inside a 0.3 m gate, which gives the
    velocity; every later step is 1 m (dt 100 ms), more than three gates: only the estimated
    velocity keeps the match."""
    gate, speed = 0.3, 10.0
    assert speed * 0.1 > 3 * gate
    tr = mk(max_dist=gate)
    t, xa, xb, got = 0, -2.05, 2.05, []
    for k, dt_ms in enumerate([0, 10, 100, 100, 100, 100]):
        t += dt_ms
        xa, xb = xa + speed * dt_ms * 1e-3, xb - speed * dt_ms * 1e-3
        pair = [(xa, 0.0), (xb, 0.2)]
        r = ids_of(tr, P(pair[::-1] if k % 2 else pair), t)
        got.append(r[::-1] if k % 2 else r)
    assert got == [[1, 2]] * 6
    st = tr.state()
    np.testing.assert_allclose(st.vx[:2], [speed, -speed], rtol=1e-4)
    assert st.next_id == 3


def case_class_mismatch(mk):
    tr = mk()
    assert ids_of(tr, P([(0, 0)], 1), 0) == [1]
    assert ids_of(tr, P([(0, 0)], 2), 100) == [2]  # the same place, another class
    assert ids_of(tr, P([(0, 0), (0, 0)], [2, 1]), 200) == [2, 1]


def case_closed_gate(mk):
    c = F(F(1.5) * F(1.5)) + F(F(0.7) * F(0.7))  # the cost of (1.5, 0.7) against (0, 0)
    assert c.dtype == F
    tr = mk(gate2=c)  # the cost is exactly at the gate
    assert ids_of(tr, P([(0, 0)]), 0) == [1] and ids_of(tr, P([(1.5, 0.7)]), 100) == [1]
    tr = mk(gate2=np.nextafter(c, F(0)))  # the cost is one ulp above the gate
    assert ids_of(tr, P([(0, 0)]), 0) == [1] and ids_of(tr, P([(1.5, 0.7)]), 100) == [2]


def case_greedy_order(mk):
    tr = mk(max_dist=2.0)
    assert ids_of(tr, P([(0, 0)]), 0) == [1]
    # detection 0 takes the track although detection 1 is closer to it
    assert ids_of(tr, P([(1.0, 0), (0.1, 0)]), 100) == [1, 2]


def case_ties(mk):
    tr = mk(max_dist=2.0)
    assert ids_of(tr, P([(-1, 0), (1, 0)]), 0) == [1, 2]
    assert ids_of(tr, P([(0, 0)]), 100) == [1]  # equal cost: the lower slot
    st = tr.state()
    assert st.hits[:2].tolist() == [2, 1] and st.age[:2].tolist() == [0, 1]


def case_max_age(mk):
    for missed, want in ((2, 1), (3, 2)):
        tr = mk(max_age=2)
        assert ids_of(tr, P([(0, 0)]), 0) == [1]
        for k in range(missed):
            assert ids_of(tr, P(np.zeros((0, 2))), 100 * (k + 1)) == []
        assert ids_of(tr, P([(0, 0)]), 100 * (missed + 1)) == [want]


def case_ids_and_slots(mk):
    tr = mk(capacity=2, max_age=0)
    seen = []
    for k in range(5):  # every frame somewhere else: the two slots are freed and taken again
        seen += ids_of(tr, P([(100.0 * k, 0), (100.0 * k, 50)]), 100 * k)
    assert seen == list(range(1, 11))
    st = tr.state()
    assert sorted(st.id.tolist()) == [9, 10] and st.next_id == 11 and st.overflow == 0


def case_overflow(mk):
    tr = mk(capacity=3)
    assert ids_of(tr, P([(10.0 * k, 0) for k in range(4)]), 0) == [1, 2, 3, 0]
    st = tr.state()
    assert st.overflow == 1 and st.next_id == 4
    r = tr.track([P([(10.0 * k, 0) for k in range(4)])], None, [100 * MS])[0]
    assert r[0].tolist() == [1, 2, 3, 0] and r[1].tolist() == [2, 2, 2, 0] and tr.state().overflow == 2


def case_edge_frames(mk):
    tr = mk(max_gap=2.0)
    assert ids_of(tr, P(np.zeros((0, 2))), 0) == []  # an empty first frame
    assert ids_of(tr, P([(0, 0), (5, 5)]), 100) == [1, 2]
    assert ids_of(tr, P([(0.5, 0), (5, 5.5)]), 100) == [1, 2]  # dt == 0: matched with pt == 0
    st = tr.state()
    assert finite_state(st) and (st.vx == 0).all() and (st.pt == 0).all()
    assert ids_of(tr, P([(1.0, 0), (5, 6.0)]), 200) == [1, 2]
    st = tr.state()
    half = F(0.5) * (F(0.5) / F(0.1))  # hits was 2: v = 0 + alpha * (vm - 0)
    assert finite_state(st) and st.vx[0] == half and st.vy[1] == half
    assert ids_of(tr, P([(1.0, 0)]), 150) == [3]  # the stamp goes back: reset, the ids go on
    st = tr.state()
    assert (st.id != 0).sum() == 1 and st.next_id == 4
    assert ids_of(tr, P([(1.0, 0)]), 150 + 2001) == [4]  # a gap above max_gap: reset
    assert ids_of(tr, P([(1.0, 0)]), 150 + 2001 + 2000) == [4]  # a gap of max_gap: none
    # a non-finite centre gets id 0 and leaves the state as an empty frame does
    a, b = mk(), mk()
    for tr_ in (a, b):
        assert ids_of(tr_, P([(0, 0), (3, 3)]), 0) == [1, 2]
    bad = P([(np.nan, 0), (0, np.inf)])
    r = a.track([bad], None, [100 * MS])[0]
    assert r[0].tolist() == [0, 0] and r[1].tolist() == [0, 0] and (r[2] == 0).all()
    assert ids_of(b, P(np.zeros((0, 2))), 100) == []
    assert a.state().same(b.state())
    nanv = P([(0, 0)], 1, [(np.nan, 0)])  # 9-d: a non-finite velocity is invalid too
    assert ids_of(a, nanv, 200) == [0]


CASES = [case_crossing_9d, case_crossing_7d, case_class_mismatch, case_closed_gate, case_greedy_order, case_ties,
         case_max_age, case_ids_and_slots, case_overflow, case_edge_frames]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__[5:])
def test_crafted(case):
    case(cpu)


# ------------------------------------------------------------------------ random scenes
def scene(seed, counts, nine=None, n_obj=160):
    """Frames of a random scene → ``(preds, stamps)``: ``n_obj`` objects of three classes at
    constant velocity plus noise, ``counts[f]`` detections in frame f (objects picked at random:
    dropouts; false positives fill up), in random order; the frames 0..100 ms apart, some dt 0."""
    r = np.random.default_rng(seed)
    nine = bool(seed % 2) if nine is None else nine
    pos = r.uniform(-60, 60, (n_obj, 2))
    vel = r.uniform(-8, 8, (n_obj, 2))
    lab = r.integers(1, 4, n_obj)
    preds, stamps, t = [], [], 1_000 * MS
    for f, n in enumerate(counts):
        dt = int(r.choice([0, 50, 100, 100])) * MS if f not in (0, 3) else 0  # (frame 3: always a dt of 0)
        t += dt
        pos = pos + vel * (dt * 1e-9)
        k = min(n, int(r.integers(n // 2, n + 1))) if n else 0
        pick = r.permutation(n_obj)[:min(k, n_obj)]
        xy = np.concatenate([pos[pick] + r.normal(0, 0.05, (len(pick), 2)), r.uniform(-60, 60, (n - len(pick), 2))])
        lb = np.concatenate([lab[pick], r.integers(1, 4, n - len(pick))])
        v = np.concatenate([vel[pick], np.zeros((n - len(pick), 2))])
        o = r.permutation(n)
        preds.append(P(xy[o], lb[o] if n else 1, v[o] if nine else None))
        stamps.append(t)
    return preds, stamps


def same_results(a, b):
    assert len(a) == len(b)
    for (i, h, v), (wi, wh, wv) in zip(a, b):
        np.testing.assert_array_equal(i, wi)
        np.testing.assert_array_equal(h, wh)
        np.testing.assert_array_equal(v.view(np.uint32), wv.view(np.uint32))


CUTS = ([8], [1] * 8, [3, 5])


def run_cut(tr, preds, stamps, cut):
    out, f = [], 0
    for n in cut:
        out += tr.track(preds[f:f + n], None, stamps[f:f + n])
        f += n
    return out


@pytest.mark.parametrize("nine", [False, True])
def test_cut_invariance(nine):
    preds, stamps = scene(5, [40, 37, 0, 45, 41, 1, 39, 44], nine, n_obj=50)
    runs = []
    for cut in CUTS:
        tr = cpu(capacity=48, max_age=1)
        runs.append((run_cut(tr, preds, stamps, cut), tr.state()))
    for out, st in runs[1:]:
        same_results(out, runs[0][0])
        assert st.same(runs[0][1])
    st = runs[0][1]
    ids = np.concatenate([o[0] for o in runs[0][0]])
    # the scene does what it is for: tracks continue, slots are reused, the capacity overflows
    assert st.overflow > 0 and st.next_id > 48 + 10 and (ids == 0).any()
    assert max(o[1].max() for o in runs[0][0] if len(o[1])) >= 3


def test_track_table_inputs():
    p9 = P([(1, 2), (np.nan, 0), (3, 4)], [1, 2, 3], [(1, 1), (0, 0), (np.inf, 0)])
    b = T.track_table([p9, P([(0, 0)])], [np.array([2, 0]), np.array([0])], [msgs.Time(5, 999_999_999), msgs.Time(6, 1)],
                      prev_ns=None)
    assert b.det_off.tolist() == [0, 2, 3] and b.rows.dtype.itemsize == 32
    assert b.rows["flags"].tolist() == [T.HAS_VEL, T.HAS_VEL | T.VALID, T.VALID]  # inf velocity; fine; 7-d
    assert b.rows["label"].tolist() == [3, 1, 1] and b.rows["x"].tolist() == [3, 1, 0]
    assert b.dt.tolist() == [0, F(np.float64(2) * 1e-9)] and b.reset.tolist() == [0, 0] and b.dt.dtype == F
    b = T.track_table([P([(0, 0)])] * 3, None, [10 * MS, 5 * MS, 2006 * MS], prev_ns=0, max_gap=2.0)
    assert b.reset.tolist() == [0, 1, 1] and b.dt.tolist() == [F(0.01), 0, 0]
    many = T.track_table([P(np.zeros((T.MAX_DETS + 3, 2)))], None, [0])
    assert many.sent == [T.MAX_DETS]
    tr = cpu(capacity=1024)
    ids = tr.track([P(np.arange(2 * (T.MAX_DETS + 3)).reshape(-1, 2) * 10.0)], None, [0])[0][0]
    assert len(ids) == T.MAX_DETS + 3 and (ids[:T.MAX_DETS] > 0).all() and (ids[T.MAX_DETS:] == 0).all()
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            T.Tracker3D(capacity=bad)


# ------------------------------------------------------------------------------ driver
class _Engine:
    """A CPU engine by duck typing: three objects whose places follow the cloud's seq."""
    names = ["Car", "Pedestrian", "Cyclist"]
    z_offset, normalize, label_base = 0.0, True, 1

    def detect(self, clouds):
        out = []
        for c in clouds:
            s = c.header.seq
            if c.header.frame_id == "stale":
                out.append(P([(500.0, 500.0)], 2))
                continue
            xy = [(0.3 * s, 0.0), (10.0 - 0.3 * s, 1.0), (-5.0, 0.2 * s)][: 3 - (s % 5 == 0)]  # (a dropout)
            out.append(P(xy[::-1] if s % 2 else xy, 2))
        return out


def _cloud(seq, frame_id="os"):
    pts = np.zeros((4, 4), F)
    return compat.create_cloud_xyzi(pts, msgs.Header(seq=seq, stamp=msgs.Time(10 + seq // 10, seq % 10 * 10 ** 8),
                                                     frame_id=frame_id))


def _drive(clouds, tracks, jsk=True, batch=1, workers=1, slow=False):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.ros import rosmsg
    from triton_client_amd.ros.bus import TopicBus

    bus = TopicBus()
    t = msgs.BoundingBoxArray if jsk else msgs.Detection3DArray
    boxes, trk, seen = [], [], []
    compat.Subscriber("/o", t, lambda m: boxes.append(rosmsg.serialize(m)), bus=bus)
    compat.Subscriber("/t", t, lambda m: trk.append((m.header.seq, rosmsg.serialize(m))), bus=bus)
    drv = RosInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, jsk=jsk, batch=batch,
                         workers=workers, queue_size=64, tracks_topic="/t" if tracks else None,
                         track_options={"max_dist": {"pedestrian": 1.0}})
    if slow:  # the first ticket finishes last
        process, first = drv.process, threading.Event()

        def slow_process(cs):
            late = not first.is_set()
            first.set()
            r = process(cs)
            if late:
                time.sleep(0.15)
            return r
        drv.process = slow_process
    track = drv.track
    drv.track = lambda rs: (seen.extend((r.boxes.header.seq, r.boxes.header.frame_id) for r in rs), track(rs))[1]
    drv.start_inference(spin=False)
    pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
    for c in clouds:
        pub.publish(c)
        if slow:
            time.sleep(0.002)  # (several tickets, not one)
    runner = drv.runner
    drv.stop()
    bus.close()
    assert runner is None or not runner.errors, runner.errors
    return boxes, trk, seen, drv


@pytest.mark.parametrize("jsk", [True, False])
def test_driver_tracks_in_order_whatever_order_the_batches_finish_in(jsk):
    clean = [_cloud(s) for s in range(1, 17)]
    boxes1, trk1, seen1, drv1 = _drive(clean, True, jsk)
    assert len(boxes1) == len(trk1) == 16 and [s for s, _ in seen1] == list(range(1, 17))
    assert [s for s, _ in trk1] == list(range(1, 17)) and all(a != b for a, (_, b) in zip(boxes1, trk1))
    # a stale cloud (seq 5 again, after seq 9) is dropped by the re-publisher: the tracker never sees it
    dirty = clean[:9] + [_cloud(5, "stale")] + clean[9:]
    boxes4, trk4, seen4, drv4 = _drive(dirty, True, jsk, batch=4, workers=3, slow=True)
    assert [s for s, _ in seen4] == list(range(1, 17)) and all(f == "os" for _, f in seen4)
    assert trk4 == trk1 and boxes4 == boxes1
    assert drv4.tracker().state().same(drv1.tracker().state())
    # the box messages are the same bytes without the topic, and nothing is tracked
    boxes0, trk0, seen0, drv0 = _drive(clean, False, jsk, batch=4, workers=3)
    assert boxes0 == boxes1 and trk0 == [] and seen0 == [] and not hasattr(drv0.engine, "_tracker")


def test_tracked_predictions_and_ids_over_the_run():
    from triton_client_amd.inference import RosInference3D

    drv = RosInference3D(engine=_Engine(), params={}, tracks_topic="/t", labels=None, score_thresh=0.3)
    clouds = [_cloud(s) for s in range(1, 9)]
    res = drv.track(drv.process(clouds))
    by_place = {}
    for c, r in zip(clouds, res):
        assert r.bev is None and r.points is None and isinstance(r.tracks, msgs.BoundingBoxArray)
        assert r.ranged is None and r.depth is None
        pred = r.pred
        assert r.tracks.header.seq == c.header.seq and r.tracks.header.stamp == c.header.stamp
        assert len(pred["track_ids"]) == len(pred["track_hits"]) == len(pred["track_vel"]) == len(r.boxes.boxes)
        assert [b.label for b in r.tracks.boxes] == pred["track_ids"].tolist()
        assert [b.label for b in r.boxes.boxes] == [2] * len(r.boxes.boxes)
        for b0, b1 in zip(r.boxes.boxes, r.tracks.boxes):
            assert b0.pose == b1.pose and b0.dimensions == b1.dimensions and b0.value == b1.value
        for (x, y), i in zip(pred["pred_boxes"][:, :2], pred["track_ids"]):
            key = "a" if y == 0.0 else "b" if y == 1.0 else "c"
            by_place.setdefault(key, set()).add(int(i))
    assert by_place == {"a": {1}, "b": {2}, "c": {3}} or sorted(map(sorted, by_place.values())) == [[1], [2], [3]]
    assert drv.tracker().kind == "host definition" and drv.tracker().frames == 8
    plain = RosInference3D(engine=_Engine(), params={}).process(clouds)[0]  # process() is as before
    assert (plain.bev, plain.points, plain.tracks, plain.ranged, plain.depth) == (None,) * 5


def test_ordered_stage_of_the_republisher():
    from triton_client_amd.inference.batching import OrderedRepublisher

    calls, out = [], []

    def stage(items):
        calls.append(list(items))
        if items and items[0] == "boom":
            raise RuntimeError("boom")
        return [i.upper() for i in items]
    rp = OrderedRepublisher(out.append, stage)
    rp.submit(1, [(3, "c"), (2, "stale"), (4, "d")])
    assert calls == [] and out == []
    rp.submit(0, [(1, "a"), (2, "b")])
    assert calls == [["a", "b"], ["c", "d"]] and out == ["A", "B", "C", "D"] and rp.stale == 1 and rp.published == 4
    rp.submit(2, [(5, "boom")])
    rp.submit(3, [(6, "e")])
    assert out[-1] == "E" and len(rp.errors) == 1 and rp.published == 5
    plain = OrderedRepublisher(out.append)  # without a stage: as before
    plain.submit(0, [(1, "x"), (1, "y")])
    assert out[-1] == "x" and plain.stale == 1


def test_flags_and_gates_by_class_name(tmp_path):
    from triton_client_amd.cli import bag3d, main3d, record
    from triton_client_amd.cli.common import track_options
    from triton_client_amd.inference.engines import Detector3D
    from triton_client_amd.ros import Bag

    f = main3d.parse_args([])
    assert f.tracks_topic == "" and f.track_max_age == 3 and track_options(f) == {"max_age": 3}
    f = main3d.parse_args(["--tracks-topic", "/t", "--track-max-age", "5", "--track-max-dist", "Car=4,Pedestrian=1"])
    assert f.tracks_topic == "/t" and track_options(f) == {"max_age": 5, "max_dist": {"Car": 4.0, "Pedestrian": 1.0}}
    f = bag3d.parse_args(["--bag", "x", "--track-max-dist", "3.5"])
    assert f.tracks_topic == "" and track_options(f)["max_dist"] == 3.5
    with pytest.raises(ValueError):
        T.parse_max_dist("Car=")
    # label_base 1: [unused 0, Car, Pedestrian, Cyclist, every other label]
    g = T.gate_table({"car": 4, "PEDESTRIAN": 1}, ["Car", "Pedestrian", "Cyclist"], 1)
    assert g.dtype == F and g.tolist() == [4, 16, 1, 4, 4]
    assert T.gate_table(1.5, ["a"], 0).tolist() == [2.25, 2.25] and T.gate_table(label_base=0).tolist() == [4.0]
    assert T.gate_table({"a": 0.1}, ["a"], 0)[0] == F(np.float64(0.1) * np.float64(0.1))
    with pytest.raises(ValueError, match="no class"):
        T.gate_table({"tram": 4}, ["Car"], 1)
    tr = Detector3D.tracker(_Engine(), **track_options(main3d.parse_args(["--track-max-dist", "Pedestrian=1"])))
    assert tr.max_dist2.tolist() == [4, 4, 1, 4, 4] and tr.max_age == 3 and tr.capacity == 256

    class Cp(_Engine):  # the CenterPoint family preloads the paper's table; a name overrides it
        family, label_base = "centerpoint", 0
        names = ["car", "truck", "bus", "pedestrian", "traffic_cone", "tram"]
    assert Detector3D.tracker(Cp()).max_dist2.tolist() == [16, 16, 30.25, 1, 1, 4, 4]
    assert Detector3D.tracker(Cp(), max_dist={"Bus": 6}).max_dist2.tolist() == [16, 16, 36, 1, 1, 4, 4]
    assert Detector3D.tracker(Cp(), max_dist=3.0).max_dist2.tolist() == [9] * 7
    e = Cp()
    assert Detector3D.tracker(e) is Detector3D.tracker(e)
    # bag3d --out-bag writes the tracks
    pc, ob = str(tmp_path / "pc.bag"), str(tmp_path / "o.bag")
    assert record.main([pc, "--frames", "3", "--no-camera", "--lidar", "--rings", "8", "--columns", "128"]) == 0
    from triton_client_amd.inference import BagInference3D
    drv = BagInference3D(engine=_Engine(), params={"sub_topic": "/os_cloud_node/points", "pub_topic": "/o"}, bagfile=pc,
                         out_bag=ob, batch=2, tracks_topic="/tracks")
    with Bag(pc) as b:
        topics = {t for t, _, _ in b.read_messages()}
    drv.params["sub_topic"] = sorted(topics)[0]
    assert drv.start_inference() == 3
    with Bag(ob) as b:
        got = [(t, m) for t, m, _ in b.read_messages()]
    tracks = [m for t, m in got if t == "/tracks"]
    assert len(tracks) == 3 and len([1 for t, _ in got if t == "/o"]) == 3
    assert all(len(m.boxes) for m in tracks) and drv.tracker().frames == 3
