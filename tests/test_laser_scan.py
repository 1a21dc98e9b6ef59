"""K29: the cloud as a 2D LaserScan — the options, the definition against a float64 ``atan2`` brute
force, crafted cases that are exact, the message on the wire and in bags, the driver and the CLI."""
import math
from dataclasses import FrozenInstanceError

import numpy as np
import pytest

from test_range2d import _Engine, _rig_messages
from triton_client_amd.ops import laser_scan as L
from triton_client_amd.ops import range2d as R
from triton_client_amd.ros import compat, msgs, rosmsg

F = np.float32
PI = math.pi
INF = F(np.inf)
# full circle at 1 degree and at 4096 bins, +-1 rad at 0.01, +-pi/2 at half a degree
OPTION_SETS = {"circle_1deg": L.ScanOptions(), "circle_4096": L.ScanOptions(angle_increment=2 * PI / 4096),
               "pm1rad": L.ScanOptions(-1.0, 1.0, 0.01), "front_half_deg": L.ScanOptions(-PI / 2, PI / 2, PI / 360)}
QUARTERS = L.ScanOptions(angle_increment=PI / 2)  # four bins: the table is exactly -2, -1, 0, 1, 2


def scene_points(seed, n=20000):
    """Gaussian points (sigma 20 m in x and y, 1 m in z: a third lie outside the height band) and a
    ring of 2,000 at 30 m (every bin of every option set has a return; many share a bin)."""
    rng = np.random.default_rng(seed)
    g = np.stack([rng.normal(0, 20, n - 2000), rng.normal(0, 20, n - 2000), rng.normal(0, 1.0, n - 2000)], 1)
    a = rng.uniform(-PI, PI, 2000)
    ring = np.stack([30 * np.cos(a), 30 * np.sin(a), rng.uniform(-0.9, 0.9, 2000)], 1)
    return np.concatenate([g, ring]).astype(F)


@pytest.fixture(scope="module")
def scenes():
    """Per option set: the points, the definition's per-point half and ranges, the reference."""
    out = {}
    for k, (name, o) in enumerate(sorted(OPTION_SETS.items())):
        pts = scene_points(k)
        out[name] = (o, pts, L.scan_keys_numpy(pts, o), L.scan_numpy(pts, o), L.scan_ref(pts, o))
    return out


def ulps(a, b):
    """|a - b| in units of the float32 spacing at b (float64 inputs)."""
    return np.abs(a - b) / np.spacing(np.abs(b).astype(F)).astype(np.float64)


# ------------------------------------------------------------------------------ options
def test_options_and_their_refusals():
    o = L.ScanOptions()
    assert (o.angle_min, o.angle_max, o.angle_increment) == (-PI, PI, PI / 180) and o.n == 360
    assert (o.min_height, o.max_height, o.range_min, o.range_max) == (-1.0, 1.0, 0.45, 100.0)
    assert (o.use_inf, o.inf_epsilon, o.scan_time) == (True, 1.0, 1 / 30)
    with pytest.raises(FrozenInstanceError):
        o.range_min = 1.0
    assert L.ScanOptions(angle_increment=2 * PI / 4096).n == 4096
    assert L.ScanOptions(-1.0, 1.0, 0.01).n == 200 and L.ScanOptions(-PI / 2, PI / 2, PI / 360).n == 360
    assert L.ScanOptions(0.0, 1.0, 0.3).n == 4 and L.ScanOptions(0.0, 1.0, 5.0).n == 1  # a last, narrower bin
    assert L.ScanOptions(min_height=-np.inf, max_height=np.inf).limits[:2].tolist() == [-np.inf, np.inf]
    assert L.ScanOptions(min_height=0.5, max_height=0.5).min_height == 0.5 and L.ScanOptions(range_min=0).range_min == 0
    assert L.ScanOptions().empty_bits == L.INF_BITS
    assert L.ScanOptions(use_inf=False, range_max=50.0, inf_epsilon=0.25).empty == F(50.25)
    bad = {"angle_min": [dict(angle_min=-4.0), dict(angle_min=1.0, angle_max=1.0), dict(angle_min=2.0, angle_max=1.0),
                         dict(angle_min=float("nan")), dict(angle_min="0")],
           "angle_max": [dict(angle_max=3.2), dict(angle_max=float("inf")), dict(angle_max=None)],
           "angle_increment": [dict(angle_increment=0.0), dict(angle_increment=-0.1),
                               dict(angle_increment=2 * PI / 4097), dict(angle_increment=float("nan")),
                               dict(angle_increment=float("inf")), dict(angle_increment=True)],
           "min_height": [dict(min_height=1.5), dict(min_height=float("nan"))],
           "max_height": [dict(max_height=float("nan"))],
           "range_min": [dict(range_min=-0.1), dict(range_min=100.0), dict(range_min=200.0),
                         dict(range_min=float("inf")), dict(range_min=1.0, range_max=1.0 + 1e-9)],
           "range_max": [dict(range_max=float("inf")), dict(range_max=float("nan"))],
           "use_inf": [dict(use_inf=1), dict(use_inf=None)],
           "inf_epsilon": [dict(inf_epsilon=0.0), dict(inf_epsilon=-1.0), dict(inf_epsilon=float("inf")),
                           dict(inf_epsilon=1e39)],
           "scan_time": [dict(scan_time=-0.1), dict(scan_time=float("inf")), dict(scan_time=float("nan"))]}
    for field, cases in bad.items():
        for kw in cases:
            with pytest.raises(ValueError, match="^" + field):
                L.ScanOptions(**kw)


def test_the_edge_table():
    assert L.edge_table(QUARTERS).tolist() == [-2.0, -1.0, 0.0, 1.0, 2.0]
    for o in OPTION_SETS.values():
        t = L.edge_table(o)
        assert t.dtype == F and t.shape == (o.n + 1,) and (np.diff(t) > 0).all() and not t.flags.writeable
    assert np.diff(L.edge_table(OPTION_SETS["circle_4096"])).min() > 7e-4  # the smallest step, far above 2**-23
    partial = L.edge_table(L.ScanOptions(0.0, 1.0, 0.3))  # the last edge is angle_max, not angle_min + 4 * 0.3
    assert partial[-1] == F(L.pseudo64(math.cos(1.0), math.sin(1.0)))


# ---------------------------------------------------------------- definition against float64
@pytest.mark.parametrize("name", sorted(OPTION_SETS))
def test_definition_equals_the_reference_outside_the_bands(scenes, name):
    o, pts, (b, valid, r), _, (b64, valid64, r64, edge, gate) = scenes[name]
    clear = ~edge
    assert (b[clear] == b64[clear]).all()
    clear &= ~gate
    assert (valid[clear] == valid64[clear]).all()
    assert ulps(r[valid64].astype(np.float64), r64[valid64]).max() <= 2
    # a test that banded everything away would fail: at most 0.5 % of the points, five times the reference's own
    assert (edge | gate).mean() <= 0.005
    assert 3000 < valid64.sum() < len(pts) - 3000 and (b64 >= 0).sum() > 3000  # and the scene decides something


@pytest.mark.parametrize("name", sorted(OPTION_SETS))
def test_every_bin_is_the_float64_minimum(scenes, name):
    """Per bin the definition's range lies between the float64 minimum over every point that may be in
    the bin (banded ones allowed in: an edge-banded point may also be in a neighbouring bin) and the
    minimum over the points that certainly are, to 2 ulp."""
    o, pts, _, ranges, (b64, valid64, r64, edge, gate) = scenes[name]
    n = o.n
    h0, h1, r0, r1 = (float(v) for v in o.limits)
    z = pts[:, 2].astype(np.float64)
    height = (z >= h0) & (z <= h1)
    in_range = (r64 >= r0) & (r64 <= r1)
    sure = valid64 & ~edge & ~gate
    hi = np.full(n, np.inf)
    np.minimum.at(hi, b64[sure], r64[sure])
    lo = hi.copy()
    maybe = height & (in_range | gate) & ((b64 >= 0) | edge)
    for shift in (-1, 0, 1):
        who = maybe & (edge | (shift == 0))
        bins = np.where(b64 >= 0, b64 + shift, 0 if shift >= 0 else n - 1)  # (outside the scan: its first or last bin)
        who &= (bins >= 0) & (bins < n)
        np.minimum.at(lo, bins[who], r64[who])
    got = ranges.astype(np.float64)
    sp = 2 * np.spacing(ranges[np.isfinite(ranges)].max())
    assert (got >= lo - sp).all() and (got <= hi + sp).all()
    assert np.isfinite(hi).mean() > (0.9 if name != "circle_4096" else 0.5)  # most bins have a certain return
    exact = np.isfinite(hi) & (lo == hi)  # bins no banded point touches: the minimum itself
    assert exact.sum() > n // 3 and ulps(got[exact], hi[exact]).max() <= 2
    assert (ranges[~np.isfinite(got)].view("<u4") == L.INF_BITS).all()


# ------------------------------------------------------------------- crafted, exact, not banded
def crafted_cases():
    """name -> (points [N, 3], options, the expected ranges): every expectation is exact."""
    wide = dict(angle_increment=PI / 2, range_min=0.0)
    full = L.ScanOptions(**wide)
    c = {}

    def bins(n, cells, empty=INF):
        a = np.full(n, empty, F)
        for k, v in cells.items():
            a[k] = v
        return a

    # (1, 0): q = 0, bin 2; (0, 1): q = 1, bin 3; (-1, 0): q = 2 = t_n, kept in bin 3; (-1, -0.0): q = -2, bin 0;
    # (0, -1): q = -1, bin 1
    for name, p, k in (("ahead", (2, 0, 0), 2), ("left", (0, 3, 0), 3), ("behind", (-4, 0, 0), 3),
                       ("behind_minus_zero", (-5, -0.0, 0), 0), ("right", (0, -6, 0), 1)):
        c["axis_" + name] = ([p], full, bins(4, {k: F(max(abs(v) for v in p))}))
    c["y_plus_zero_ahead"] = ([(2, 0.0, 0)], full, bins(4, {2: 2}))
    c["y_minus_zero_ahead"] = ([(2, -0.0, 0)], full, bins(4, {2: 2}))  # q = -0.0 == t_2: still bin 2, as atan2's -0.0
    c["right_of_ahead"] = ([(2, -1, 0)], full, bins(4, {1: np.sqrt(F(5))}))
    up, down = np.nextafter(F(1), F(2)), np.nextafter(F(-1), F(-2))
    c["z_on_both_limits"] = ([(3, 1, 1.0), (-3, -1, -1.0)], full, bins(4, {2: np.sqrt(F(10)), 0: np.sqrt(F(10))}))
    c["z_next_float_outside"] = ([(3, 1, up), (-3, -1, down)], full, bins(4, {}))
    lim = L.ScanOptions(angle_increment=PI / 2, range_min=0.45, range_max=100.0)
    c["r_on_both_limits"] = ([(F(0.45), 0, 0), (0, -100, 0)], lim, bins(4, {2: F(0.45), 1: 100}))
    c["r_next_float_outside"] = ([(np.nextafter(F(0.45), F(0)), 0, 0), (0, -np.nextafter(F(100), F(200)), 0)], lim,
                                 bins(4, {}))
    c["r_is_a_3_4_5_triangle"] = ([(3, 4, 0)], full, bins(4, {2: 5}))
    c["dropped"] = ([(0, 0, 0), (np.nan, 1, 0), (1, np.nan, 0), (1, 1, np.nan), (np.inf, 1, 0), (1, -np.inf, 0),
                     (-np.inf, np.inf, 0), (1, 1, np.inf)], full, bins(4, {}))
    c["infinite_heights_keep_infinite_z"] = ([(1, 1, np.inf), (-2, 2, -np.inf)],
                                             L.ScanOptions(min_height=-np.inf, max_height=np.inf, **wide),
                                             bins(4, {2: np.sqrt(F(2)), 3: np.sqrt(F(8))}))
    c["nearer_wins_far_first"] = ([(9, 1, 0), (4, 1, 0), (6, 1, 0)], full, bins(4, {2: np.sqrt(F(17))}))
    c["nearer_wins_near_first"] = ([(4, 1, 0), (6, 1, 0), (9, 1, 0)], full, bins(4, {2: np.sqrt(F(17))}))
    c["empty_cloud_inf"] = (np.zeros((0, 3), F), full, bins(4, {}))
    c["empty_cloud_no_inf"] = (np.zeros((0, 3), F), L.ScanOptions(use_inf=False, range_max=50.0, inf_epsilon=0.5, **wide),
                               bins(4, {}, F(50.5)))
    c["no_inf_beside_a_return"] = ([(0, 7, 0)], L.ScanOptions(use_inf=False, **wide), bins(4, {3: 7}, F(101)))
    # +-1 rad in two bins: 1.2 rad to the left and to the right fall outside, +-0.5 rad inside
    part = L.ScanOptions(-1.0, 1.0, 1.0, range_min=0.0)
    at = [(5 * math.cos(a), 5 * math.sin(a), 0) for a in (1.2, -1.2, 0.5, -0.5, PI)]
    c["partial_scan_drops_both_sides"] = (at, part, bins(2, {0: np.sqrt(F(at[3][0]) ** 2 + F(at[3][1]) ** 2),
                                                             1: np.sqrt(F(at[2][0]) ** 2 + F(at[2][1]) ** 2)}))
    c["single_wide_bin"] = ([(-3, 0.5, 0), (2, -2, 0), (-1, -1, 0)], L.ScanOptions(angle_increment=7.0, range_min=0.0),
                            bins(1, {0: np.sqrt(F(2))}))
    return c


CASES = crafted_cases()


def check_case(name, run):
    pts, o, want = CASES[name]
    got = run(np.asarray(pts, F).reshape(-1, 3), o)
    assert got.dtype == np.dtype("<f4") and got.shape == (o.n,), name
    np.testing.assert_array_equal(got.view("<u4"), want.view("<u4"), err_msg=name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted(name):
    check_case(name, L.scan_numpy)


def test_pseudo_angle_of_the_axes_and_the_order_of_points():
    pts = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [-1, -0.0, 0], [0, -1, 0]], F)
    b, valid, r = L.scan_keys_numpy(pts, L.ScanOptions(angle_increment=PI / 2, range_min=0.0))
    assert b.tolist() == [2, 3, 3, 0, 1] and valid.all() and (r == 1).all()
    b64 = L.scan_ref(pts, QUARTERS)[0]
    assert b64.tolist() == b.tolist()  # and atan2 agrees, the angle pi itself in the last bin
    o, pts = OPTION_SETS["circle_1deg"], scene_points(9, 5000)
    want = L.scan_numpy(pts, o)
    for seed in (1, 2):
        np.testing.assert_array_equal(L.scan_numpy(pts[np.random.default_rng(seed).permutation(len(pts))], o), want)


# ----------------------------------------------------------------------- message and wire
def _cloud(points, seq=7, t=(12, 345)):
    p = np.concatenate([np.asarray(points, F).reshape(-1, 3), np.zeros((len(points), 1), F)], 1)
    return compat.create_cloud_xyzi(p, msgs.Header(seq=seq, stamp=msgs.Time(*t), frame_id="os"))


def test_md5_and_schema():
    assert rosmsg.md5sum("sensor_msgs/LaserScan") == "90c7ef2dc6895d81024acba2ac42f369"
    assert rosmsg.TYPE_OF[msgs.LaserScan] == "sensor_msgs/LaserScan"
    assert msgs.MSG_TYPES["sensor_msgs/LaserScan"] is msgs.LaserScan
    assert "float32[] ranges" in rosmsg.full_definition("sensor_msgs/LaserScan")


def test_scan_message_and_wire_round_trip():
    o = L.ScanOptions(range_max=60.0, scan_time=0.1)
    pts = scene_points(3, 2300)[:300]  # few enough that many of the 360 rays find nothing
    c = _cloud(pts)
    ranges = L.scan_numpy(pts, o)
    assert np.isinf(ranges).sum() > 100 and np.isfinite(ranges).sum() > 100
    m = L.scan_message(c, ranges, o)
    assert (m.header.seq, m.header.stamp, m.header.frame_id) == (7, msgs.Time(12, 345), "os")
    assert L.scan_message(c, ranges, o, "base_scan").header.frame_id == "base_scan"
    assert (m.angle_min, m.angle_max, m.angle_increment) == (float(F(-PI)), float(F(PI)), float(F(PI / 180)))
    assert (m.time_increment, m.scan_time, m.range_min, m.range_max) == (0.0, float(F(0.1)), float(F(0.45)), 60.0)
    assert m.ranges.dtype == np.dtype("<f4") and m.ranges.tobytes() == ranges.tobytes() and len(m.intensities) == 0
    with pytest.raises(ValueError, match="ranges"):
        L.scan_message(c, ranges[:-1], o)
    wire = rosmsg.serialize(m)
    assert len(wire) == 4 + 8 + 4 + 2 + 7 * 4 + 4 + 4 * 360 + 4  # header, seven floats, two counted arrays
    assert wire[-4 - 4 * 360 - 4:-4 - 4 * 360] == (360).to_bytes(4, "little") and wire[-4:] == b"\0\0\0\0"
    back = rosmsg.deserialize(wire, "sensor_msgs/LaserScan")
    assert isinstance(back, msgs.LaserScan) and back == m and back.ranges.tobytes() == ranges.tobytes()
    assert rosmsg.serialize(back) == wire
    # a list of floats serialises to the same bytes as the array
    listed = msgs.LaserScan(**{**{f: getattr(m, f) for f in m.__dataclass_fields__}, "ranges": ranges.tolist()})
    assert rosmsg.serialize(listed) == wire and listed == m
    assert m != msgs.LaserScan(**{**{f: getattr(m, f) for f in m.__dataclass_fields__}, "ranges": ranges[::-1]})
    with pytest.raises(ValueError):
        rosmsg.deserialize(wire[:-8], "sensor_msgs/LaserScan")


@pytest.mark.parametrize("ext", ["bag", "tcabag"])
def test_bag_write_and_read(tmp_path, ext):
    from triton_client_amd.ros import Bag

    o = L.ScanOptions(use_inf=False)
    pts = scene_points(4, 3000)
    scans = [L.scan_message(_cloud(pts, seq=s, t=(20 + s, 5)), L.scan_numpy(pts * F(s), o), o) for s in (1, 2, 3)]
    path = str(tmp_path / f"scans.{ext}")
    with Bag(path, "w") as b:
        for m in scans:
            b.write("/scan", m)
    with Bag(path) as b:
        got = [(t, m, stamp) for t, m, stamp in b.read_messages()]
    assert [t for t, _, _ in got] == ["/scan"] * 3 and [m for _, m, _ in got] == scans
    assert all(isinstance(m, msgs.LaserScan) and stamp == m.header.stamp for _, m, stamp in got)
    assert [rosmsg.serialize(m) for _, m, _ in got] == [rosmsg.serialize(m) for m in scans]


# ------------------------------------------------------------------------ scanner on the CPU
def test_layouts_the_switch_and_the_scanner_on_the_cpu(monkeypatch):
    from triton_client_amd.ops.cloud_common import CloudLayout

    assert L.layout_device_ok(CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7)))
    assert L.layout_device_ok(CloudLayout(18, (1, 5, 9, -1), (7, 7, 7, 2)))  # the intensity is not read
    assert not L.layout_device_ok(CloudLayout(16, (0, 4, 8, 12), (7, 7, 8, 7)))
    assert not L.layout_device_ok(CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7), True))
    assert not L.layout_device_ok(CloudLayout(12, (0, 4, 10, -1), (7, 7, 7, 7)))
    assert L.device_enabled()
    monkeypatch.setenv("TCA_DEVICE_SCAN", "0")
    assert not L.device_enabled()
    clouds, _ = _rig_messages()
    sc = L.LaserScanner("cpu")
    o = L.ScanOptions(min_height=-2.0)
    got = sc.ranges(clouds, o)
    assert not sc.gpu and len(got) == 4
    for g, c in zip(got, clouds):
        np.testing.assert_array_equal(g.view("<u4"), L.scan_numpy(R.cloud_xyzi(c), o).view("<u4"))
    assert sc.ranges([], o) == []
    # 64 clouds and 2^31 staged bytes to a launch

    class Big:
        data = range(2 ** 29)  # (only its length is asked for)

    assert [len(p) for p in sc._parts(list(range(150)), [clouds[0]] * 150)] == [64, 64, 22]
    assert [len(p) for p in sc._parts(list(range(9)), [Big] * 9)] == [3, 3, 3]


# ----------------------------------------------------------------------- driver, bag, CLI
OPTS = L.ScanOptions(min_height=-2.0, range_max=40.0)


def _expected(cloud, o=OPTS):
    return L.scan_numpy(R.cloud_xyzi(cloud), o).tobytes()


@pytest.mark.parametrize("batch,workers,tracks", [(1, 1, False), (4, 2, True)])
def test_driver_publishes_the_definition_and_keeps_every_other_byte(batch, workers, tracks):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.ros.bus import TopicBus

    clouds, _ = _rig_messages()

    def drive(scan):
        bus = TopicBus()
        seen = {t: [] for t in ("/o", "/bev", "/pts", "/trk")}
        got, order = [], []
        for t, ty in (("/o", msgs.BoundingBoxArray), ("/bev", msgs.Image), ("/pts", msgs.PointCloud2),
                      ("/trk", msgs.BoundingBoxArray)):
            compat.Subscriber(t, ty, lambda m, t=t: seen[t].append(rosmsg.serialize(m)), bus=bus)
        compat.Subscriber("/scan", msgs.LaserScan, got.append, bus=bus)
        kw = dict(scan_topic="/scan", scan_options=OPTS, scan_frame_id="base") if scan else {}
        drv = RosInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=batch,
                             workers=workers, queue_size=64, bev_topic="/bev", points_topic="/pts",
                             tracks_topic="/trk" if tracks else None, **kw)
        drv.start_inference(spin=False)
        for name, p in [("box", drv.pub), *drv.side_pubs.items()]:  # the order the driver publishes in
            def publish(m, name=name, send=p.publish):
                order.append((name, m.header.seq))
                send(m)
            p.publish = publish
        pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
        for c in clouds:
            pub.publish(c)
        runner = drv.runner
        drv.stop()
        bus.close()
        assert runner is None or not runner.errors, runner.errors
        return seen, got, order, drv

    seen1, got1, order, drv1 = drive(True)
    assert [m.header.seq for m in got1] == [1, 2, 3, 4]
    for m, c in zip(got1, clouds):
        assert isinstance(m, msgs.LaserScan) and np.asarray(m.ranges, "<f4").tobytes() == _expected(c)
        assert (m.header.stamp, m.header.frame_id) == (c.header.stamp, "base")
        assert (m.range_max, m.angle_increment, len(m.intensities)) == (40.0, float(F(PI / 180)), 0)
        wall = np.asarray(m.ranges)[np.isfinite(m.ranges)]
        assert len(wall) > 10 and 10 + c.header.seq - 0.1 < wall.min() < 10 + c.header.seq + 0.1  # the wall ahead
    # after the box message and every other output of the same cloud, in published order
    names = ["box", "bev", "points"] + (["tracks"] if tracks else []) + ["scan"]
    assert order == [(k, s) for s in (1, 2, 3, 4) for k in names]
    seen0, got0, _, drv0 = drive(False)
    assert got0 == [] and "scan" not in drv0.side_pubs and not hasattr(drv0.engine, "_laser_scanner")
    assert seen1 == seen0 and len(seen1["/o"]) == len(seen1["/bev"]) == len(seen1["/pts"]) == 4
    assert len(seen1["/trk"]) == (4 if tracks else 0)
    assert drv1.engine._laser_scanner.gpu is False


def test_process_shapes_and_constructor_refusals():
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.inference.ros_inference3d import NAV_OUTPUTS, OUTPUTS, SIDE_OUTPUTS

    class Stages:
        """What the driver's stage timer reports to."""
        def __init__(self):
            self.names = []

        def stage(self, name, seconds):
            self.names.append(name)

        def frame(self, n=1):
            pass

    assert NAV_OUTPUTS == (("scan", msgs.LaserScan),) and OUTPUTS == SIDE_OUTPUTS + NAV_OUTPUTS  # published last
    clouds, _ = _rig_messages()
    metrics = Stages()
    drv = RosInference3D(engine=_Engine(), params={}, scan_topic="/s", metrics=metrics,
                         scan_options={"angle_min": -1.0, "angle_max": 1.0, "min_height": -2.0, "use_inf": False})
    assert drv.scan_options == L.ScanOptions(angle_min=-1.0, angle_max=1.0, min_height=-2.0, use_inf=False)
    for r, c in zip(drv.process(clouds), clouds):
        s = r.pred["scan"]  # the message rides in the prediction too
        assert s.ranges.tobytes() == _expected(c, drv.scan_options) and s.header.frame_id == "os"
        assert r.scan is s and (r.bev, r.points, r.tracks, r.ranged, r.depth) == (None,) * 5
    assert "laser_scan" in metrics.names
    assert RosInference3D(engine=_Engine(), params={}, scan_topic="/s").scan_options == L.ScanOptions()  # the defaults
    off = RosInference3D(engine=_Engine(), params={})
    assert all("scan" not in r.pred and r.scan is None for r in off.process(clouds)) and off.scan_topic is None
    with pytest.raises(ValueError, match="angle_increment"):
        RosInference3D(engine=_Engine(), params={}, scan_topic="/s", scan_options={"angle_increment": 1e-4})
    with pytest.raises(TypeError):
        RosInference3D(engine=_Engine(), params={}, scan_topic="/s", scan_options={"width": 3})


def test_bag_replay_writes_the_scans(tmp_path):
    from triton_client_amd.inference import BagInference3D
    from triton_client_amd.ros import Bag

    clouds, _ = _rig_messages()
    src = str(tmp_path / "rig.bag")
    with Bag(src, "w") as b:
        for c in clouds:
            b.write("/pc", c)

    def replay(out, **kw):
        drv = BagInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bagfile=src,
                             out_bag=out, batch=3, points_topic="/pts", tracks_topic="/trk", **kw)
        assert drv.start_inference() == 4
        with Bag(out) as b:
            return [(t, m) for t, m, _ in b.read_messages()]

    on = replay(str(tmp_path / "on.bag"), scan_topic="/scan", scan_options=OPTS)
    off = replay(str(tmp_path / "off.bag"))
    got = [m for t, m in on if t == "/scan"]
    assert [m.header.seq for m in got] == [1, 2, 3, 4]
    for m, c in zip(got, clouds):
        assert isinstance(m, msgs.LaserScan) and np.asarray(m.ranges, "<f4").tobytes() == _expected(c)
        assert m == L.scan_message(c, L.scan_numpy(R.cloud_xyzi(c), OPTS), OPTS)
    rest = [(t, rosmsg.serialize(m)) for t, m in on if t != "/scan"]
    assert rest == [(t, rosmsg.serialize(m)) for t, m in off] and len(rest) == 16
    assert [t for t, _ in on][:5] == ["/pc", "/o", "/pts", "/trk", "/scan"]  # last of its cloud's messages


def test_flags_and_usage_errors(capsys):
    from triton_client_amd.cli import bag3d, main3d

    f = main3d.parse_args([])
    assert f.scan_topic == "" and f.scan_options is None and not f.scan_frame_id
    for mod, pre in ((main3d, []), (bag3d, ["--bag", "x"])):
        assert mod.parse_args(pre + ["--scan-topic", "/scan"]).scan_options == L.ScanOptions()
        f = mod.parse_args(pre + ["--scan-topic", "/scan", "--scan-angle=-1.5,1.5", "--scan-increment", "0.005",
                                  "--scan-height=-0.5,inf", "--scan-range", "0.2,30", "--scan-no-inf",
                                  "--scan-inf-epsilon", "0.5", "--scan-time", "0.1", "--scan-frame-id", "base"])
        assert f.scan_options == L.ScanOptions(-1.5, 1.5, 0.005, -0.5, math.inf, 0.2, 30.0, False, 0.5, 0.1)
        assert f.scan_frame_id == "base" and f.scan_options.n == 600
        for bad, word in ((["--scan-angle", "0,1"], "--scan-topic"), (["--scan-increment", "0.1"], "--scan-topic"),
                          (["--scan-height", "0,1"], "--scan-topic"), (["--scan-range", "1,2"], "--scan-topic"),
                          (["--scan-no-inf"], "--scan-topic"), (["--scan-inf-epsilon", "1"], "--scan-topic"),
                          (["--scan-time", "0.1"], "--scan-topic"), (["--scan-frame-id", "b"], "--scan-topic"),
                          (["--scan-topic", "/s", "--scan-angle", "0"], "--scan-angle"),
                          (["--scan-topic", "/s", "--scan-angle", "0,x"], "--scan-angle"),
                          (["--scan-topic", "/s", "--scan-angle", "1,0.5"], "--scan-angle"),
                          (["--scan-topic", "/s", "--scan-angle", "0,3.5"], "--scan-angle"),
                          (["--scan-topic", "/s", "--scan-increment", "0.001"], "--scan-increment"),
                          (["--scan-topic", "/s", "--scan-increment", "0"], "--scan-increment"),
                          (["--scan-topic", "/s", "--scan-height", "1,0"], "--scan-height"),
                          (["--scan-topic", "/s", "--scan-range", "5,1"], "--scan-range"),
                          (["--scan-topic", "/s", "--scan-range=-1,5"], "--scan-range"),
                          (["--scan-topic", "/s", "--scan-inf-epsilon", "0"], "--scan-inf-epsilon"),
                          (["--scan-topic", "/s", "--scan-time=-1"], "--scan-time")):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(pre + bad)
            err = capsys.readouterr().err  # a flag without the topic says so; a bad value names its flag
            assert e.value.code == 2 and (f"{bad[0]} needs --scan-topic" if word == "--scan-topic" else
                                          f"error: {word}: ") in err, (bad, err[-200:])
