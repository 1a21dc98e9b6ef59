"""K26 on the host: the float32 definition of camera ranging against a float64 brute force,
crafted edge cases, stamp pairing, calibration files, the driver over the bus and the flags."""
import numpy as np
import pytest

from triton_client_amd.ops import range2d as R
from triton_client_amd.ros import compat, msgs

F = np.float32
KITTI_P = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791],
                    [0.0, 0.0, 1.0, 0.002745884]])
AXES = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])  # LiDAR x ahead -> camera z ahead


def _rot(a, i):
    c, s = np.cos(a), np.sin(a)
    m = np.eye(3)
    j, k = (i + 1) % 3, (i + 2) % 3
    m[j, j], m[j, k], m[k, j], m[k, k] = c, -s, s, c
    return m


def rig(seed=0):
    """A KITTI-like projection and a slightly rotated LiDAR -> camera transform."""
    ax = np.random.default_rng(1000 + seed).normal(0, 0.02, 3)
    T = np.eye(4)
    T[:3, :3] = _rot(ax[0], 0) @ _rot(ax[1], 1) @ _rot(ax[2], 2) @ AXES
    T[:3, 3] = [0.0, -0.08, -0.27]
    return R.Calibration(KITTI_P, T)


def scene(seed, n=20000, k=40):
    """Seeded points in x -10..80, y +-30, z -2.5..1.5 and k random pixel boxes → (points [n, 3],
    calibration, boxes [k, 4] (cx, cy, sx, sy))."""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-10, 80, n), rng.uniform(-30, 30, n), rng.uniform(-2.5, 1.5, n)], 1).astype(F)
    boxes = np.stack([rng.uniform(0, 1242, k), rng.uniform(100, 375, k), rng.uniform(20, 300, k),
                      rng.uniform(20, 200, k)], 1).astype(F)
    return pts, rig(seed), boxes


SEEDS = range(20)


@pytest.fixture(scope="module")
def scenes():
    out = []
    for s in SEEDS:
        pts, cal, boxes = scene(s)
        rows = R.box_rows(boxes)
        out.append((pts, cal, rows, R.range2d_numpy(pts, rows, cal.M, return_inside=True),
                    R.range2d_ref(pts, rows, cal.M)))
    return out


# ------------------------------------------------------------ definition against float64
def test_definition_equals_the_reference_outside_the_band(scenes):
    pairs = in_band = differ = bin_differ = 0
    for pts, cal, rows, (n, m, c, sums, inside, bins), (rn, rm, rc, rs, rinside, rbins, band, bin_band) in scenes:
        pairs += inside.size
        in_band += int(band.sum())
        differ += int((inside != rinside).sum())
        assert not ((inside != rinside) & ~band).any()
        counted = inside.any(1) | rinside.any(1)
        bin_differ += int(((bins != rbins) & counted).sum())
        assert not ((bins != rbins) & counted & ~bin_band).any()
        # a box none of whose points is in a band has the reference's integers
        clean = ~band.any(0) & ~(bin_band[:, None] & rinside).any(0)
        assert clean.sum() >= 30
        for a, b in ((n, rn), (m, rm), (c, rc), (sums, rs)):
            assert (a[clean] == b[clean]).all()
    print(f"pairs {pairs} band {in_band} float32/float64 disagreements {differ} bins {bin_differ}")
    assert pairs == len(SEEDS) * 20000 * 40
    assert in_band <= pairs // 1000  # the cap on the band: a condition, not a measurement
    assert in_band <= 200 and differ <= in_band  # the band stays far inside the cap


def test_scenes_are_not_vacuous(scenes):
    boxes = ranged = differs = 0
    for _, _, rows, (n, m, c, sums, inside, bins), _ in scenes:
        boxes += len(rows)
        for j in np.nonzero(m >= 0)[0]:
            ranged += 1
            differs += int(bins[inside[:, j]].min() != m[j])
            assert 1 <= c[j] <= n[j]
    print(f"{ranged} of {boxes} boxes ranged, {differs} with a quantile bin past the nearest occupied one")
    assert ranged >= 0.8 * boxes and differs >= 0.5 * ranged


def test_host_finish_gives_the_camera_frame_mean(scenes):
    pts, cal, rows, (n, m, c, sums, inside, bins), _ = scenes[0]
    ok, mean, cam = R.finish(m, c, sums, cal.T)
    assert (ok == (m >= 0)).all() and ok.any() and not ok.all()
    j = int(np.nonzero(ok)[0][0])
    sel = inside[:, j] & (np.abs(bins - m[j]) <= 1)
    want = pts[sel].astype(np.float64).mean(0)
    assert np.abs(mean[j] - want).max() <= 1.0 / 1024  # the fixed point's half step, with room
    assert np.allclose(cam[j], cal.T[:3, :3] @ mean[j] + cal.T[:3, 3], rtol=0, atol=1e-12)
    assert (cam[~ok] == 0).all() and cam[j, 2] >= 0.5 - 0.25


# ------------------------------------------------------------------------ crafted cases
# u = x, v = y, w = z at z = 2 (a = 2x, b = 2y): every product, sum and quotient is exact
M_EXACT = np.array([[2.0, 0, 0, 0], [0, 2.0, 0, 0], [0, 0, 1.0, 0]], F)
BOX = np.array([[10.0, 20.0, 8.0, 4.0]], F)  # shrink 0.5: u in [8, 12], v in [19, 21]


def _below(x):
    return np.nextafter(F(x), F(-np.inf))


def _above(x):
    return np.nextafter(F(x), F(np.inf))


def crafted_cases():
    """name → (points [N, 3], boxes [K, 4], options, expected dict of n / m / c / sums)."""
    cases = {}

    def add(name, pts, boxes=BOX, want=None, shrink=0.5, **opts):
        cases[name] = (np.asarray(pts, F).reshape(-1, 3), np.asarray(boxes, F).reshape(-1, 4), shrink, opts, want)

    edge = [(8, 20, 2), (12, 20, 2), (10, 19, 2), (10, 21, 2), (8, 19, 2), (12, 21, 2)]
    out = [(_below(8), 20, 2), (_above(12), 20, 2), (10, _below(19), 2), (10, _above(21), 2)]
    add("edges_closed", edge + out, want={"n": [6], "m": [8], "c": [6]})
    # w == min_depth is in, one ulp below is out (u = 2x / w: x = 2.5 keeps u = 10)
    add("min_depth", [(2.5, 5, 0.5), (2.5, 5, 0.5), (2.5, 5, 0.5), (2.5, 5, _below(0.5))],
        want={"n": [3], "m": [2], "c": [3]})
    # q just below 512 is in, q at 512 is out (bin_w 0.25: w = 128)
    far = float(_below(128.0))
    add("last_bin", [(5 * far, 10 * far, far)] * 3 + [(640, 1280, 128)], want={"n": [3], "m": [511], "c": [3]})
    nan, inf = np.nan, np.inf
    add("nan_inf_points", [(10, 20, 2)] * 3 + [(nan, 20, 2), (10, nan, 2), (10, 20, nan), (inf, 20, 2), (10, -inf, 2),
                                                (10, 20, inf), (10, 20, -inf)],
        want={"n": [3], "m": [8], "c": [3], "sums": [[3 * 10240, 3 * 20480, 3 * 2048]]})
    add("nan_box_rows", [(10, 20, 2)] * 3,
        boxes=[(10, 20, 8, 4), (nan, 20, 8, 4), (10, 20, inf, 4), (10, 20, 0, 4), (10, 20, 8, -1), (10, inf, 8, 4)],
        want={"n": [3, 0, 0, 0, 0, 0], "m": [8, -1, -1, -1, -1, -1], "c": [3, 0, 0, 0, 0, 0]})
    add("behind_camera", [(10, 20, 2)] * 3 + [(-10, -20, -2)] * 4, want={"n": [3], "m": [8], "c": [3]})
    add("overlap_counts_in_both", [(10, 20, 2)] * 3 + [(13, 20, 2)] * 2, boxes=[(10, 20, 8, 4), (12, 20, 8, 4)],
        want={"n": [3, 5], "m": [8, 8], "c": [3, 5]})
    add("below_min_points", [(10, 20, 2)] * 2, want={"n": [2], "m": [-1], "c": [0], "sums": [[0, 0, 0]]})
    add("at_min_points", [(10, 20, 2)] * 4, min_points=4, want={"n": [4], "m": [8], "c": [4]})
    # 100 points, one per bin 8..107 (w = 2.125 + 0.25 i, u and v stay inside: u = 2x / w)
    ramp = [(5 * w, 10 * w, w) for w in (2.125 + 0.25 * np.arange(100))]
    add("pct_1", ramp, pct=1, want={"n": [100], "m": [8], "c": [2]})
    add("pct_50", ramp, pct=50, want={"n": [100], "m": [57], "c": [3]})
    add("pct_100", ramp, pct=100, want={"n": [100], "m": [107], "c": [2]})
    add("window_0", ramp, window=0, want={"n": [100], "m": [57], "c": [1]})
    add("window_3", ramp, window=3, want={"n": [100], "m": [57], "c": [7]})
    # the fixed point clamps at +-2^30: x = +-2^21 * 1.5 would give +-1.5 * 2^31
    big = float(2 ** 21 * 1.5)
    add("clamp", [(big, 20, 2), (-big, 20, 2), (-big, 20, 2), (1.5 / 1024, 20 + 2.5 / 1024, 2)],
        boxes=[(0, 20, 4e7, 4)], M=np.array([[0, 0, 0, 0], [0, 2.0, 0, 0], [0, 0, 1.0, 0]], F),
        want={"n": [4], "m": [8], "c": [4], "sums": [[-2 ** 30 + 2, 4 * 20480 + 2, 4 * 2048]]})
    return cases


CASES = crafted_cases()


def check_case(name, run):
    """``run(points, rows, M, options)`` → (n, m, c, sums) is compared with the case's expectations."""
    pts, boxes, shrink, opts, want = CASES[name]
    opts = dict(opts)
    M = opts.pop("M", M_EXACT)
    rows = R.box_rows(boxes, shrink)
    n, m, c, sums = run(pts, rows, M, R.RangeOptions(shrink=shrink, **opts))
    got = {"n": n, "m": m, "c": c, "sums": sums}
    for key, val in want.items():
        assert np.asarray(got[key]).tolist() == val, (name, key, np.asarray(got[key]).tolist(), val)
    return got


def _run_numpy(pts, rows, M, o):
    return R.range2d_numpy(pts, rows, M, o.pct, o.min_points, o.bin_w, o.min_depth, o.window)


@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted(name):
    check_case(name, _run_numpy)


def test_box_rows_and_fixed_point():
    b = np.array([[100, 50, 40, 20]], F)
    assert R.box_rows(b).tolist() == [[F(100) - F(20) * F(0.6), F(50) - F(10) * F(0.6), F(100) + F(20) * F(0.6),
                                       F(50) + F(10) * F(0.6)]]
    assert R.box_rows(b, 1.0).tolist() == [[80, 40, 120, 60]]
    assert R.fixed_point(np.array([0.5 / 1024, 1.5 / 1024, 2.5 / 1024, -0.5 / 1024, 1e9, -1e9], F)).tolist() == \
        [0, 2, 2, 0, 2 ** 30, -2 ** 30]  # half to even, the clamp
    for bad in ({"shrink": 0}, {"shrink": 1.5}, {"pct": 0}, {"pct": 101}, {"min_points": 0}, {"window": -1},
                {"bin_w": 0}, {"bin_w": np.inf}, {"min_depth": np.nan}):
        with pytest.raises(ValueError):
            R.RangeOptions(**bad)


# ------------------------------------------------------------------------------ pairing
def _det_msg(t_ns, boxes=(), seq=0, frame="cam"):
    dets = [msgs.Detection2D(results=[msgs.ObjectHypothesisWithPose(id=3 + i, score=0.5 + 0.1 * i)] if i != 1 else [],
                             bbox=msgs.BoundingBox2D(msgs.Pose2D(float(b[0]), float(b[1])), float(b[2]), float(b[3])))
            for i, b in enumerate(boxes)]
    return msgs.Detection2DArray(header=msgs.Header(seq=seq, stamp=msgs.Time(t_ns // 10 ** 9, t_ns % 10 ** 9),
                                                    frame_id=frame), detections=dets)


def test_stamp_pairer():
    s = 10 ** 9
    p = R.StampPairer(capacity=4)
    assert p.nearest(msgs.Time(1, 0)) is None
    held = [_det_msg(t, seq=i) for i, t in enumerate([s, s + 40_000_000, s + 100_000_000])]
    for m in held:
        p.push(m)
    assert p.nearest(msgs.Time(1, 30_000_000)) is held[1]  # 10 ms beats 30 ms
    assert p.nearest(msgs.Time(1, 20_000_000)) is held[0]  # a tie goes to the earlier stamp
    assert p.nearest(msgs.Time(1, 150_000_000)) is held[2]  # |dt| == slop is in
    assert p.nearest(msgs.Time(1, 150_000_001)) is None  # one nanosecond past it is out
    assert p.nearest(msgs.Time(1, 60_000_000), slop=0.01) is None
    assert p.nearest(msgs.Time(0, 960_000_000)) is held[0]
    for i in range(3):  # capacity 4: the two oldest leave
        p.push(_det_msg(5 * s + i, seq=10 + i))
    assert len(p) == 4 and p.nearest(msgs.Time(1, 0)) is None and p.nearest(msgs.Time(1, 40_000_000)) is None
    assert p.nearest(msgs.Time(1, 100_000_000)) is held[2]
    with pytest.raises(ValueError):
        R.StampPairer(0)


# -------------------------------------------------------------------------- calibration
def test_load_calibration_both_formats_and_refusals(tmp_path):
    R0 = _rot(0.01, 0) @ _rot(-0.02, 1)
    Tr = np.concatenate([_rot(0.015, 2) @ AXES, [[0.004], [-0.076], [-0.272]]], 1)
    P2 = KITTI_P

    def line(a):
        return " ".join(repr(float(v)) for v in np.asarray(a).reshape(-1))

    kitti = tmp_path / "000000.txt"
    kitti.write_text(f"P0: {line(P2)}\nP2: {line(P2)}\nR0_rect: {line(R0)}\nTr_velo_to_cam: {line(Tr)}\n"
                     f"Tr_imu_to_velo: {line(Tr)}\n")
    R4 = np.eye(4)
    R4[:3, :3] = R0
    yml = tmp_path / "rig.yaml"
    yml.write_text(f"projection: {(P2 @ R4).tolist()}\nlidar_to_camera: {Tr.tolist()}\n")
    a, b = R.load_calibration(str(kitti)), R.load_calibration(str(yml))
    assert a.M.dtype == F and a.M.shape == (3, 4) and (a.M == b.M).all()
    assert a.T.shape == (4, 4) and (a.T[3] == [0, 0, 0, 1]).all() and np.array_equal(a.T, b.T)
    # 3x3 projection, 4x4 transform
    T4 = np.concatenate([Tr, [[0, 0, 0, 1]]], 0)
    yml.write_text(f"projection: {P2[:, :3].tolist()}\nlidar_to_camera: {T4.tolist()}\n")
    c = R.load_calibration(str(yml))
    assert (c.P[:, 3] == 0).all() and np.array_equal(c.T, T4)

    def refuses(text, key, path=yml):
        path.write_text(text)
        with pytest.raises(ValueError, match=key):
            R.load_calibration(str(path))

    refuses(f"projection: {P2[:2].tolist()}\nlidar_to_camera: {Tr.tolist()}\n", "projection")
    refuses(f"projection: {P2.tolist()}\nlidar_to_camera: {Tr[:, :3].tolist()}\n", "lidar_to_camera")
    refuses(f"projection: {P2.tolist()}\n", "lidar_to_camera")
    refuses(f"lidar_to_camera: {Tr.tolist()}\n", "projection")
    refuses(f"projection: {P2.tolist()}\nlidar_to_camera: {Tr.tolist()}\n".replace("721.5377", ".nan", 1), "projection")
    refuses(f"projection: {P2.tolist()}\nlidar_to_camera: {Tr.tolist()}\n".replace("-0.272", ".inf"), "lidar_to_camera")
    refuses(f"P2: {line(P2)}\nR0_rect: {line(R0)}\n", "Tr_velo_to_cam", kitti)
    refuses(f"P2: {line(P2)}\nTr_velo_to_cam: {line(Tr)}\n", "R0_rect", kitti)
    refuses(f"P2: {line(P2[:, :3])}\nR0_rect: {line(R0)}\nTr_velo_to_cam: {line(Tr)}\n", "P2", kitti)
    refuses(f"P2: {line(P2)}\nR0_rect: {line(R0)}\nTr_velo_to_cam: {line(Tr)} nan\n", "Tr_velo_to_cam", kitti)
    refuses(f"P2: {line(P2)}\nR0_rect: {line(R0).replace(' ', ' inf ', 1)}\nTr_velo_to_cam: {line(Tr)}\n", "R0_rect",
            kitti)


# ------------------------------------------------------------------------------- driver
class _Engine:
    """A CPU engine by duck typing: one box per cloud."""
    names = ["Car", "Pedestrian", "Cyclist"]
    z_offset, normalize, label_base = 0.0, True, 1

    def detect(self, clouds):
        return [{"pred_boxes": np.array([[10.0 + c.header.seq, 0, 0, 4, 2, 1.5, 0.1]], F),
                 "pred_scores": np.array([0.9], F), "pred_labels": np.array([2])} for c in clouds]


CAL = R.Calibration(KITTI_P, np.concatenate([np.concatenate([AXES, [[0.0], [-0.08], [-0.27]]], 1), [[0, 0, 0, 1]]], 0))
NS = 10 ** 9


def _cloud(seq, t_ns, depth):
    """A wall of points `depth` metres ahead (y, z spread) and a few strays."""
    rng = np.random.default_rng(seq)
    wall = np.stack([np.full(300, depth) + rng.uniform(-0.05, 0.05, 300), rng.uniform(-3, 3, 300),
                     rng.uniform(-1.5, 0.5, 300), np.zeros(300)], 1)
    return compat.create_cloud_xyzi(wall.astype(F), msgs.Header(seq=seq, stamp=msgs.Time(t_ns // NS, t_ns % NS),
                                                                frame_id="os"))


def _rig_messages():
    """Clouds 0.1 s apart, walls at 10 + seq metres; camera messages 3 ms after clouds 1, 2 and 4 (none near
    cloud 3), each with a box on the wall, one with no hypothesis, and one on empty sky."""
    clouds = [_cloud(s, 10 * NS + s * NS // 10, 10.0 + s) for s in (1, 2, 3, 4)]
    boxes = [(609, 150, 200, 60), (500, 160, 100, 40), (609, -500, 50, 50)]
    cams = [_det_msg(10 * NS + s * NS // 10 + 3_000_000, boxes, seq=100 + s) for s in (1, 2, 4)]
    return clouds, cams


def _expected_ranged(cloud, cam):
    rows = R.box_rows(R.bbox_array(cam))
    n, m, c, sums = R.range2d_numpy(R.cloud_xyzi(cloud), rows, CAL.M)
    return R.finish(m, c, sums, CAL.T)


def _check_ranged(got, clouds, cams):
    assert [m.header.seq for m in got] == [101, 102, 104]  # cloud 3 found no partner
    for m, cam, cloud in zip(got, cams, [clouds[0], clouds[1], clouds[3]]):
        assert m.header == cam.header and len(m.detections) == 3
        ok, _, pos = _expected_ranged(cloud, cam)
        assert ok.tolist() == [True, True, False]
        for i, (d, d0) in enumerate(zip(m.detections, cam.detections)):
            assert d.bbox == d0.bbox and len(d.results) == max(1, len(d0.results))
            r = d.results[0]
            assert (r.id, r.score) == ((d0.results[0].id, d0.results[0].score) if d0.results else (0, 0.0))
            assert (r.pose.position.x, r.pose.position.y, r.pose.position.z) == tuple(pos[i])
        depth = 10.0 + cloud.header.seq
        assert abs(m.detections[0].results[0].pose.position.z - (depth - 0.27)) < 0.1
        assert m.detections[2].results[0].pose.position == msgs.Point()
        assert not cam.detections[1].results  # the camera message itself is left alone


@pytest.mark.parametrize("batch,workers,tracks", [(1, 1, False), (4, 2, True)])
def test_driver_publishes_ranged_and_keeps_every_other_byte(batch, workers, tracks):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.ros import rosmsg
    from triton_client_amd.ros.bus import TopicBus

    clouds, cams = _rig_messages()

    def drive(ranged):
        bus = TopicBus()
        seen = {t: [] for t in ("/o", "/bev", "/pts", "/trk")}
        got = []
        for t, ty in (("/o", msgs.BoundingBoxArray), ("/bev", msgs.Image), ("/pts", msgs.PointCloud2),
                      ("/trk", msgs.BoundingBoxArray)):
            compat.Subscriber(t, ty, lambda m, t=t: seen[t].append(rosmsg.serialize(m)), bus=bus)
        compat.Subscriber("/ranged", msgs.Detection2DArray, got.append, bus=bus)
        kw = dict(ranged_topic="/ranged", camera_detections_topic="/cam", calibration=CAL) if ranged else {}
        drv = RosInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=batch,
                             workers=workers, queue_size=64, bev_topic="/bev", points_topic="/pts",
                             tracks_topic="/trk" if tracks else None, **kw)
        drv.start_inference(spin=False)
        cam_pub = compat.Publisher("/cam", msgs.Detection2DArray, bus=bus)
        for m in cams:
            cam_pub.publish(m)
        pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
        for c in clouds:
            pub.publish(c)
        runner = drv.runner
        drv.stop()
        bus.close()
        assert runner is None or not runner.errors, runner.errors
        return seen, got, drv

    seen1, got1, drv1 = drive(True)
    _check_ranged(got1, clouds, cams)
    seen0, got0, drv0 = drive(False)
    assert got0 == [] and drv0.pairer is None and not hasattr(drv0.engine, "_ranger")
    assert seen1 == seen0 and len(seen1["/o"]) == len(seen1["/bev"]) == len(seen1["/pts"]) == 4
    assert len(seen1["/trk"]) == (4 if tracks else 0)


def test_process_shapes_and_options():
    from triton_client_amd.inference import RosInference3D

    clouds, cams = _rig_messages()
    drv = RosInference3D(engine=_Engine(), params={}, ranged_topic="/r", camera_detections_topic="/c", calibration=CAL,
                         range_options={"min_points": 1000})
    for m in cams:
        drv.pairer.push(m)
    res = drv.process(clouds)
    # no other side output; the message rides in the prediction too
    assert all((r.bev, r.points, r.tracks, r.depth) == (None,) * 4 for r in res)
    assert [r.pred["ranged"] is not None for r in res] == [True, True, False, True]
    assert all(d.results[0].pose.position == msgs.Point() for d in res[0].pred["ranged"].detections)  # min_points
    assert all(r.ranged is r.pred["ranged"] for r in res)
    off = RosInference3D(engine=_Engine(), params={})
    r0 = off.process(clouds)
    assert all((r.bev, r.points, r.tracks, r.ranged, r.depth) == (None,) * 5 and "ranged" not in r.pred for r in r0)
    assert drv.engine._ranger.gpu is False
    with pytest.raises(ValueError, match="calibration"):
        RosInference3D(engine=_Engine(), params={}, ranged_topic="/r", camera_detections_topic="/c")
    with pytest.raises(ValueError, match="camera_detections_topic"):
        RosInference3D(engine=_Engine(), params={}, ranged_topic="/r", calibration=CAL)
    with pytest.raises(ValueError, match="pct"):
        RosInference3D(engine=_Engine(), params={}, ranged_topic="/r", camera_detections_topic="/c", calibration=CAL,
                       range_options={"pct": 0})


def test_bag_replay_writes_the_ranged_messages(tmp_path):
    from triton_client_amd.inference import BagInference3D
    from triton_client_amd.ros import Bag, rosmsg

    clouds, cams = _rig_messages()
    src = str(tmp_path / "rig.bag")
    with Bag(src, "w") as b:  # the camera messages lie behind their clouds in the bag: the first pass finds them
        for c in clouds:
            b.write("/pc", c)
        for m in cams:
            b.write("/cam", m)

    def replay(out, **kw):
        drv = BagInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bagfile=src,
                             out_bag=out, batch=3, points_topic="/pts", tracks_topic="/trk", **kw)
        assert drv.start_inference() == 4
        with Bag(out) as b:
            return [(t, m) for t, m, _ in b.read_messages()]

    on = replay(str(tmp_path / "on.bag"), ranged_topic="/ranged", camera_detections_topic="/cam", calibration=CAL)
    off = replay(str(tmp_path / "off.bag"))
    _check_ranged([m for t, m in on if t == "/ranged"], clouds, cams)
    rest = [(t, rosmsg.serialize(m)) for t, m in on if t != "/ranged"]
    assert rest == [(t, rosmsg.serialize(m)) for t, m in off] and len(rest) == 16
    assert not [1 for t, _ in off if t == "/ranged"]


def test_flags_and_usage_errors(tmp_path, capsys):
    from triton_client_amd.cli import bag3d, main3d

    calib = tmp_path / "rig.yaml"
    calib.write_text(f"projection: {KITTI_P.tolist()}\nlidar_to_camera: {CAL.T.tolist()}\n")
    f = main3d.parse_args([])
    assert f.ranged_topic == "" and f.calibration is None and f.range_options == {} and f.range_slop == 0.05
    assert (f.range_shrink, f.range_quantile, f.range_min_points, f.range_bin) == (0.6, 50, 3, 0.25)
    args = ["--ranged-topic", "/r", "--camera-detections-topic", "/cam", "--calib", str(calib)]
    for mod, pre in ((main3d, []), (bag3d, ["--bag", "x"])):
        f = mod.parse_args(pre + args + ["--range-slop", "0.02", "--range-shrink", "0.5", "--range-quantile", "30",
                                         "--range-min-points", "5", "--range-bin", "0.5"])
        assert f.ranged_topic == "/r" and f.camera_detections_topic == "/cam" and f.range_slop == 0.02
        assert f.range_options == {"shrink": 0.5, "pct": 30, "min_points": 5, "bin_w": 0.5}
        assert (f.calibration.M == CAL.M).all()
        R.RangeOptions(**f.range_options)
        for bad, word in ((["--ranged-topic", "/r", "--camera-detections-topic", "/cam"], "--calib"),
                          (["--ranged-topic", "/r", "--calib", str(calib)], "--camera-detections-topic"),
                          (args + ["--range-quantile", "0"], "pct"), (args + ["--range-shrink", "2"], "shrink"),
                          (args + ["--range-bin", "0"], "bin_w"), (args + ["--range-min-points", "0"], "min_points"),
                          (args[:-1] + [str(tmp_path / "missing.yaml")], "missing.yaml")):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(pre + bad)
            assert e.value.code == 2 and word in capsys.readouterr().err
