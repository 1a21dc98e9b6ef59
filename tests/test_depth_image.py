"""K27 on the host: the float32 definition of the depth image against a float64 brute force,
crafted cases with hand-written images, the options, the message, the driver over the bus, bag
replay and the flags."""
from dataclasses import FrozenInstanceError

import numpy as np
import pytest

from test_range2d import CAL, KITTI_P, M_EXACT, _Engine, _above, _below, _rig_messages, rig
from triton_client_amd.ops import depth_image as D
from triton_client_amd.ops import range2d as R
from triton_client_amd.ros import compat, msgs

F = np.float32
NAN_BITS = 0x7FC00000
KITTI_W, KITTI_H = 1242, 375


def scene_points(seed, n=20000):
    """Seeded points in x -10..80, y +-30, z -2.5..1.5: some behind the camera, some past every
    image border, some farther than 65.535 m, and many pixels that get more than one point."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-10, 80, n), rng.uniform(-30, 30, n), rng.uniform(-2.5, 1.5, n)], 1).astype(F)


# (seed, options): both encodings, the two scales the documents name, every splat class
SCENES = [(0, dict()), (1, dict(splat=0)), (2, dict(scale=256.0, splat=4)), (3, dict(encoding="32FC1")),
          (4, dict(min_depth=2.0)), (5, dict(encoding="32FC1", splat=2)), (6, dict()), (7, dict(scale=256.0))]


@pytest.fixture(scope="module")
def scenes():
    out = []
    for seed, kw in SCENES:
        pts, cal = scene_points(seed), rig(seed)
        o = D.DepthOptions(KITTI_W, KITTI_H, **kw)
        out.append((pts, cal, o, D.depth_keys_numpy(pts, cal.M, o), D.depth_ref(pts, cal.M, o)))
    return out


# ------------------------------------------------------------ definition against float64
def test_definition_equals_the_reference_outside_the_band(scenes):
    for pts, cal, o, (px, py, valid, key), (rpx, rpy, rvalid, key16, pixel_band, valid_band) in scenes:
        band = pixel_band | valid_band
        differ = (px != rpx) | (py != rpy) | (valid != rvalid)
        print(f"{o}: band {int(band.sum())} of {len(pts)}, float32/float64 disagreements {int(differ.sum())}")
        assert band.sum() * 100 <= len(pts)  # the cap on the band: a condition, not a measurement
        assert not (differ & ~band).any()
        both = valid & rvalid
        assert both.sum() >= 1000
        if o.encoding == "16UC1":
            assert (np.abs(key[both].astype(np.int64) - key16[both]) <= 1).all()
        else:  # the key is the float32 depth's bits: in output units it is as near the reference's integer
            near = both & (key16 > 0)
            w32 = key[near].view(F).astype(np.float64)
            assert near.sum() >= 1000 and (np.abs(w32 * float(F(o.scale)) - key16[near]) <= 1).all()
            assert (key[both].view(F) >= F(o.min_depth)).all()


def test_scenes_are_not_vacuous(scenes):
    for pts, cal, o, (px, py, valid, key), _ in scenes:
        u, v, w = R.project_uvw(pts, cal.M)
        near = w >= F(o.min_depth)
        assert valid.sum() >= 1000
        assert (~near).sum() > 100  # behind the camera, or nearer than min_depth
        for clause in (u < 0, u >= KITTI_W, v < 0, v >= KITTI_H):
            assert (near & clause).sum() > 10  # past every border of the image
        if o.encoding == "16UC1" and o.scale == 1000.0:  # (scale 256 reaches 256 m: past every point)
            inside = near & (u >= 0) & (u < KITTI_W) & (v >= 0) & (v < KITTI_H)
            assert (inside & ~valid).sum() > 10  # beyond 65535 units: dropped
        flat = py[valid].astype(np.int64) * KITTI_W + px[valid]
        assert (np.bincount(flat) >= 2).sum() >= 1  # a pixel that two points share
        image = D.depth_numpy(pts, cal.M, o)
        lit = (image != 0) if o.encoding == "16UC1" else ~np.isnan(image)
        assert image.shape == (KITTI_H, KITTI_W) and image.dtype == o.dtype
        assert lit.sum() >= min(valid.sum(), 1000) and not lit.all()


def test_the_image_is_the_minimum_over_the_covering_points(scenes):
    """``depth_numpy`` against a per-point loop over the keys of ``depth_keys_numpy``."""
    pts, cal, o, (px, py, valid, key), _ = scenes[2]  # splat 4
    plane = np.full((KITTI_H, KITTI_W), D.EMPTY, np.uint32)
    for x, y, k in zip(px[valid][:3000], py[valid][:3000], key[valid][:3000]):
        y0, y1, x0, x1 = max(y - 4, 0), min(y + 4, KITTI_H - 1), max(x - 4, 0), min(x + 4, KITTI_W - 1)
        plane[y0:y1 + 1, x0:x1 + 1] = np.minimum(plane[y0:y1 + 1, x0:x1 + 1], k)
    sub = pts[np.nonzero(valid)[0][:3000]]
    assert np.array_equal(D.depth_numpy(sub, cal.M, o), D.image_of_keys(plane, o))
    assert np.array_equal(D.depth_numpy(sub[::-1], cal.M, o), D.image_of_keys(plane, o))  # any order


# ------------------------------------------------------------------------ crafted cases
# M_EXACT: u = 2x / z, v = 2y / z, w = z.  at(u, v, w) is the point that lands there exactly when
# u * w / 2 and v * w / 2 are float32 numbers.
def at(u, v, w):
    return (F(u) * F(w) / F(2), F(v) * F(w) / F(2), F(w))


def img16(W, H, cells):
    a = np.zeros((H, W), "<u2")
    for (x, y), d in cells.items():
        a[y, x] = d
    return a


def img32(W, H, cells):
    a = np.full((H, W), NAN_BITS, "<u4")
    for (x, y), d in cells.items():
        a[y, x] = F(d).view(np.uint32)
    return a.view("<f4")


def crafted_cases():
    """name → (points [N, 3], options, expected image)."""
    cases = {}
    nan = np.nan

    def add(name, pts, want, W=8, H=6, **kw):
        kw.setdefault("splat", 0)
        cases[name] = (np.asarray(pts, F).reshape(-1, 3), D.DepthOptions(W, H, **kw), want)

    add("borders", [at(0, 3, 2), at(8, 3, 2), at(3, 0, 2), at(3, 6, 2), at(_below(8), 5, 2), at(5, _below(6), 2),
                    at(_below(0), 1, 2), at(1, _below(0), 2)],
        img16(8, 6, {(0, 3): 2000, (3, 0): 2000, (7, 5): 2000, (5, 5): 2000}))
    add("nan_coordinate", [(nan, 1, 2), (1, nan, 2), (1, 1, nan), at(4, 4, 2)], img16(8, 6, {(4, 4): 2000}))
    add("behind_camera", [(-1, -1, -2), (-3, -2, -2), at(2, 2, 3)], img16(8, 6, {(2, 2): 3000}))
    # w == min_depth is in (pixel 2, 3), one ulp below is out (it would land on pixel 2, 4)
    add("min_depth", [(0.5, 0.75, 0.5), (0.5, 1.0, _below(0.5))], img16(8, 6, {(2, 3): 500}))
    # scale 1024: t = w * 1024 is exact.  65535 is kept; 65535.5 rounds to 65536 and is dropped like
    # 65536 and anything beyond (w = 3e38 at pixel 0, 0: t overflows to inf), never clamped; 65534.5
    # rounds to the even 65534; z = inf makes u a NaN (0 * inf)
    add("range_end", [at(1, 1, 65535 / 1024), at(2, 1, 65535.5 / 1024), at(3, 1, 64.0), at(4, 1, 100.0),
                      at(5, 1, 65534.5 / 1024), (1, 1, np.inf), (1, 1, 3e38)],
        img16(8, 6, {(1, 1): 65535, (5, 1): 65534}), scale=1024.0)
    add("half_to_even", [at(1, 2, 2000.5 / 1024), at(2, 2, 2001.5 / 1024), at(3, 2, 2002.5 / 1024)],
        img16(8, 6, {(1, 2): 2000, (2, 2): 2002, (3, 2): 2002}), scale=1024.0)
    # d = 0 (t = 0.5 rounds to the even 0) is no depth: dropped; t just above 0.5 gives 1
    add("range_start", [at(1, 1, 0.5), at(2, 1, _above(0.5))], img16(8, 6, {(2, 1): 1}), scale=1.0)
    add("nearer_wins", [at(3.5, 2.5, 2), at(3.25, 2.75, 3)], img16(8, 6, {(3, 2): 2000}))
    add("nearer_wins_reversed", [at(3.25, 2.75, 3), at(3.5, 2.5, 2)], img16(8, 6, {(3, 2): 2000}))
    add("scale_256", [at(1, 1, 2), at(2, 2, 10.5)], img16(8, 6, {(1, 1): 512, (2, 2): 2688}), scale=256.0)
    add("empty_16", np.zeros((0, 3)), np.zeros((6, 8), "<u2"))
    add("empty_32", np.zeros((0, 3)), np.full((6, 8), NAN_BITS, "<u4").view("<f4"), encoding="32FC1")
    # 32FC1: the float32 w of the nearest point, bit for bit (2.1 and 3.7 are no float32 numbers;
    # the pixel coordinate is inexact with them, and truncation does not care)
    add("float_bits", [at(3.5, 2.5, F(3.7)), at(3.5, 2.5, F(2.1)), at(6.5, 0.5, F(0.7)), at(1.5, 1.5, 0.25)],
        img32(8, 6, {(3, 2): F(2.1), (6, 0): F(0.7)}), encoding="32FC1")

    # splats on a 12 x 10 image: a corner, an edge and the centre, each square clipped to the image
    def square(rows, cols, d=2000):
        a = np.zeros((10, 12), "<u2")
        a[rows, cols] = d
        return a

    for s, corner, corner2, edge, centre in (
            (0, (slice(0, 1), slice(0, 1)), (slice(9, 10), slice(11, 12)), (slice(0, 1), slice(5, 6)),
             (slice(5, 6), slice(5, 6))),
            (1, (slice(0, 2), slice(0, 2)), (slice(8, 10), slice(10, 12)), (slice(0, 2), slice(4, 7)),
             (slice(4, 7), slice(4, 7))),
            (4, (slice(0, 5), slice(0, 5)), (slice(5, 10), slice(7, 12)), (slice(0, 5), slice(1, 10)),
             (slice(1, 10), slice(1, 10)))):
        add(f"splat{s}_corner", [at(0.5, 0.5, 2)], square(*corner), 12, 10, splat=s)
        add(f"splat{s}_far_corner", [at(11.5, 9.5, 2)], square(*corner2), 12, 10, splat=s)
        add(f"splat{s}_edge", [at(5.5, 0.5, 2)], square(*edge), 12, 10, splat=s)
        add(f"splat{s}_centre", [at(5.5, 5.5, 2)], square(*centre), 12, 10, splat=s)
    # overlapping squares: the nearer point owns the overlap
    a = square(slice(1, 4), slice(1, 4), 3000)
    a[2:5, 2:5] = 2000
    add("splat_overlap", [at(2.5, 2.5, 3), at(3.5, 3.5, 2)], a, 12, 10, splat=1)
    return cases


CASES = crafted_cases()


def check_case(name, run):
    """``run(points, M, options)`` → image is compared with the case's hand-written image, bit for bit."""
    pts, o, want = CASES[name]
    got = run(pts, M_EXACT, o)
    assert got.dtype == want.dtype == o.dtype and got.shape == want.shape == (o.height, o.width), name
    bits = "<u2" if o.encoding == "16UC1" else "<u4"
    np.testing.assert_array_equal(got.view(bits), want.view(bits), err_msg=name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted(name):
    check_case(name, D.depth_numpy)


# ------------------------------------------------------------------- options and message
def test_options_refusals():
    o = D.DepthOptions(1280, 720)
    assert (o.encoding, o.scale, o.min_depth, o.splat) == ("16UC1", 1000.0, 0.5, 1)
    assert o.dtype == np.dtype("<u2") and o.frame_bytes == 1280 * 720 * 2
    assert D.DepthOptions(4096, 1, encoding="32FC1", splat=4).frame_bytes == 4096 * 4
    with pytest.raises(FrozenInstanceError):
        o.width = 3
    for field, bad in (("width", (0, 4097, -1, 2.5, None)), ("height", (0, 4097, "7")),
                       ("encoding", ("mono16", "16uc1", None)), ("scale", (0, -1, np.inf, np.nan, 1e39, "x")),
                       ("min_depth", (0, -0.5, np.inf, np.nan, 1e-50)), ("splat", (-1, 5, 1.5, None))):
        for v in bad:
            kw = {"width": 8, "height": 6, field: v}
            with pytest.raises(ValueError, match=field):
                D.DepthOptions(**kw)


@pytest.mark.parametrize("encoding,size", [("16UC1", 2), ("32FC1", 4)])
def test_depth_message(encoding, size):
    o = D.DepthOptions(37, 23, encoding=encoding)
    cloud = compat.create_cloud_xyzi(np.zeros((0, 4), F), msgs.Header(seq=7, stamp=msgs.Time(12, 34), frame_id="os"))
    im = D.depth_numpy(np.asarray([at(3, 4, 2)], F), M_EXACT, o)
    m = D.depth_message(cloud, im, o)
    assert (m.header.seq, m.header.stamp, m.header.frame_id) == (7, msgs.Time(12, 34), "os")
    assert (m.height, m.width, m.encoding, m.is_bigendian, m.step) == (23, 37, encoding, 0, 37 * size)
    assert len(bytes(m.data)) == 37 * 23 * size and bytes(m.data) == im.tobytes()
    assert D.depth_message(cloud, im, o, "cam0").header.frame_id == "cam0"
    assert cloud.header.frame_id == "os"  # the cloud's header is left alone
    with pytest.raises(ValueError, match="shape"):
        D.depth_message(cloud, im[:-1], o)


def test_layouts_and_the_switch(monkeypatch):
    from triton_client_amd.ops.cloud_common import CloudLayout

    assert D.layout_device_ok(CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7)))
    assert D.layout_device_ok(CloudLayout(13, (1, 5, 9, -1), (7, 7, 7, 7)))
    assert D.layout_device_ok(CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 2)))  # the intensity is not read
    assert not D.layout_device_ok(CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7), True))
    assert not D.layout_device_ok(CloudLayout(32, (0, 8, 16, 24), (8, 8, 8, 7)))
    assert not D.layout_device_ok(CloudLayout(12, (0, 4, 9, -1), (7, 7, 7, 7)))
    monkeypatch.delenv("TCA_DEVICE_DEPTH", raising=False)
    assert D.device_enabled()
    monkeypatch.setenv("TCA_DEVICE_DEPTH", "0")
    assert not D.device_enabled()


def test_imager_on_the_cpu_and_its_parts():
    clouds, _ = _rig_messages()
    o = D.DepthOptions(KITTI_W, KITTI_H)
    im = D.DepthImager("cpu")
    got = im.images(clouds, CAL.M, o)
    assert not im.gpu and len(got) == 4
    for g, c in zip(got, clouds):
        assert np.array_equal(g, D.depth_numpy(R.cloud_xyzi(c), CAL.M, o)) and (g != 0).sum() > 100
    # a launch holds at most 64 clouds and a key plane of at most 256 MiB
    many = [clouds[0]] * 150
    assert [len(p) for p in im._parts(list(range(150)), many, o)] == [64, 64, 22]
    big = D.DepthOptions(4096, 4096)
    parts = list(im._parts(list(range(10)), many, big))
    assert [len(p) for p in parts] == [4, 4, 2] and sum(parts, []) == list(range(10))
    assert all(len(p) * 4096 * 4096 * 4 <= 256 << 20 for p in parts)
    assert [len(p) for p in im._parts([0, 1, 2], many, D.DepthOptions(4096, 4096, encoding="32FC1"))] == [3]


# ------------------------------------------------------------------------------- driver
OPTS = D.DepthOptions(KITTI_W, KITTI_H)


def _expected(cloud, o=OPTS):
    return D.depth_numpy(R.cloud_xyzi(cloud), CAL.M, o).tobytes()


@pytest.mark.parametrize("batch,workers,tracks", [(1, 1, False), (4, 2, True)])
def test_driver_publishes_the_definition_and_keeps_every_other_byte(batch, workers, tracks):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.ros import rosmsg
    from triton_client_amd.ros.bus import TopicBus

    clouds, _ = _rig_messages()

    def drive(depth):
        bus = TopicBus()
        seen = {t: [] for t in ("/o", "/bev", "/pts", "/trk")}
        got, order = [], []
        for t, ty in (("/o", msgs.BoundingBoxArray), ("/bev", msgs.Image), ("/pts", msgs.PointCloud2),
                      ("/trk", msgs.BoundingBoxArray)):
            compat.Subscriber(t, ty, lambda m, t=t: seen[t].append(rosmsg.serialize(m)), bus=bus)
        compat.Subscriber("/depth", msgs.Image, got.append, bus=bus)
        kw = dict(depth_topic="/depth", depth_options=OPTS, depth_frame_id="cam", calibration=CAL) if depth else {}
        drv = RosInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=batch,
                             workers=workers, queue_size=64, bev_topic="/bev", points_topic="/pts",
                             tracks_topic="/trk" if tracks else None, **kw)
        drv.start_inference(spin=False)
        for name, p in (("box", drv.pub), ("depth", drv.side_pubs.get("depth"))):  # the order the driver publishes in
            if p is not None:
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
        assert bytes(m.data) == _expected(c) and (m.header.stamp, m.header.frame_id) == (c.header.stamp, "cam")
        assert (m.height, m.width, m.encoding, m.step, m.is_bigendian) == (KITTI_H, KITTI_W, "16UC1", 2 * KITTI_W, 0)
        assert np.frombuffer(bytes(m.data), "<u2").max() > 10000  # the wall, in millimetres
    # after the box message of the same cloud, in published order
    assert order == [(k, s) for s in (1, 2, 3, 4) for k in ("box", "depth")]
    seen0, got0, _, drv0 = drive(False)
    assert got0 == [] and "depth" not in drv0.side_pubs and not hasattr(drv0.engine, "_depth_imager")
    assert seen1 == seen0 and len(seen1["/o"]) == len(seen1["/bev"]) == len(seen1["/pts"]) == 4
    assert len(seen1["/trk"]) == (4 if tracks else 0)
    assert drv1.engine._depth_imager.gpu is False


def test_process_shapes_and_constructor_refusals():
    from triton_client_amd.inference import RosInference3D

    clouds, cams = _rig_messages()
    drv = RosInference3D(engine=_Engine(), params={}, depth_topic="/d", calibration=CAL,
                         depth_options={"width": 64, "height": 48, "encoding": "32FC1", "splat": 0})
    assert drv.depth_options == D.DepthOptions(64, 48, encoding="32FC1", splat=0)
    res = drv.process(clouds)
    for r, c in zip(res, clouds):
        d = r.pred["depth"]  # the message rides in the prediction too
        assert bytes(d.data) == _expected(c, drv.depth_options) and d.header.frame_id == "os"
        assert r.depth is d and (r.bev, r.points, r.tracks, r.ranged) == (None, None, None, None)
        assert "ranged" not in r.pred
    # with ranging too, one calibration serves both
    both = RosInference3D(engine=_Engine(), params={}, depth_topic="/d", calibration=CAL, depth_options=OPTS,
                          ranged_topic="/r", camera_detections_topic="/c")
    for m in cams:
        both.pairer.push(m)
    r = both.process(clouds)[0]
    assert r.ranged is r.pred["ranged"] is not None and r.depth is r.pred["depth"] is not None
    assert (r.bev, r.points, r.tracks) == (None, None, None)
    off = RosInference3D(engine=_Engine(), params={})
    assert all("depth" not in r.pred and r.depth is None for r in off.process(clouds))
    with pytest.raises(ValueError, match="calibration"):
        RosInference3D(engine=_Engine(), params={}, depth_topic="/d", depth_options=OPTS)
    with pytest.raises(ValueError, match="depth_options"):
        RosInference3D(engine=_Engine(), params={}, depth_topic="/d", calibration=CAL)
    with pytest.raises(ValueError, match="splat"):
        RosInference3D(engine=_Engine(), params={}, depth_topic="/d", calibration=CAL,
                       depth_options={"width": 8, "height": 8, "splat": 9})


def test_bag_replay_writes_the_images_and_the_pngs(tmp_path):
    from PIL import Image as PILImage

    from triton_client_amd.inference import BagInference3D
    from triton_client_amd.ros import Bag, rosmsg

    clouds, _ = _rig_messages()
    src = str(tmp_path / "rig.bag")
    with Bag(src, "w") as b:
        for c in clouds:
            b.write("/pc", c)

    def replay(out, **kw):
        drv = BagInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bagfile=src,
                             out_bag=out, batch=3, points_topic="/pts", tracks_topic="/trk", **kw)
        assert drv.start_inference() == 4
        if not out:
            return []
        with Bag(out) as b:
            return [(t, m) for t, m, _ in b.read_messages()]

    pngs = tmp_path / "depth"
    on = replay(str(tmp_path / "on.bag"), depth_topic="/depth", depth_options=OPTS, calibration=CAL,
                depth_out=str(pngs))
    off = replay(str(tmp_path / "off.bag"))
    got = [m for t, m in on if t == "/depth"]
    assert [m.header.seq for m in got] == [1, 2, 3, 4]
    for i, (m, c) in enumerate(zip(got, clouds)):
        assert bytes(m.data) == _expected(c) and m.encoding == "16UC1" and m.step == 2 * KITTI_W
        png = np.asarray(PILImage.open(pngs / f"{i:04}.png"))
        assert png.shape == (KITTI_H, KITTI_W) and png.astype("<u2").tobytes() == _expected(c)
    assert sorted(p.name for p in pngs.iterdir()) == [f"{i:04}.png" for i in range(4)]
    rest = [(t, rosmsg.serialize(m)) for t, m in on if t != "/depth"]
    assert rest == [(t, rosmsg.serialize(m)) for t, m in off] and len(rest) == 16
    # the PNGs alone: no output bag, the topic gets its default name
    alone = tmp_path / "alone"
    drv = BagInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bagfile=src, out_bag=None,
                         depth_options=OPTS, calibration=CAL, depth_out=str(alone))
    assert drv.start_inference() == 4 and drv.depth_topic == "/o/depth" and len(list(alone.iterdir())) == 4
    with pytest.raises(ValueError, match="16UC1"):
        BagInference3D(engine=_Engine(), params={"pub_topic": "/o"}, bagfile=src, calibration=CAL, depth_out="x",
                       depth_options=D.DepthOptions(8, 8, encoding="32FC1"))


def test_flags_and_usage_errors(tmp_path, capsys):
    from triton_client_amd.cli import bag3d, main3d

    calib = tmp_path / "rig.yaml"
    calib.write_text(f"projection: {KITTI_P.tolist()}\nlidar_to_camera: {CAL.T.tolist()}\n")
    f = main3d.parse_args([])
    assert f.depth_topic == "" and f.depth_options is None and f.calibration is None and not f.depth_frame_id
    args = ["--depth-topic", "/d", "--calib", str(calib), "--depth-size", "1280x720"]
    for mod, pre in ((main3d, []), (bag3d, ["--bag", "x"])):
        f = mod.parse_args(pre + args)  # --calib for depth alone, without --ranged-topic
        assert f.depth_options == D.DepthOptions(1280, 720) and (f.calibration.M == CAL.M).all()
        assert f.ranged_topic == "" and f.range_options == {}
        f = mod.parse_args(pre + args + ["--depth-encoding", "32FC1", "--depth-scale", "256", "--depth-min", "1.5",
                                         "--depth-splat", "0", "--depth-frame-id", "cam0"])
        assert f.depth_options == D.DepthOptions(1280, 720, "32FC1", 256.0, 1.5, 0) and f.depth_frame_id == "cam0"
        f = mod.parse_args(pre + args + ["--ranged-topic", "/r", "--camera-detections-topic", "/cam"])
        assert f.depth_options is not None and f.range_options["pct"] == 50 and (f.calibration.M == CAL.M).all()
        for bad, word in ((["--depth-topic", "/d", "--depth-size", "8x8"], "--calib"),
                          (["--depth-topic", "/d", "--calib", str(calib)], "--depth-size"),
                          (args[:-1] + ["1280"], "WxH"), (args[:-1] + ["0x720"], "width"),
                          (args[:-1] + ["64x5000"], "height"), (args + ["--depth-splat", "5"], "splat"),
                          (args + ["--depth-scale", "0"], "scale"), (args + ["--depth-min", "0"], "min_depth"),
                          (args + ["--depth-encoding", "mono16"], "invalid choice"),
                          (["--depth-size", "8x8"], "--depth-topic"), (["--depth-splat", "2"], "--depth-topic"),
                          (["--depth-encoding", "32FC1"], "--depth-topic"), (["--depth-scale", "256"], "--depth-topic"),
                          (["--depth-min", "1"], "--depth-topic"), (["--depth-frame-id", "c"], "--depth-topic"),
                          (["--depth-topic", "/d", "--depth-size", "8x8", "--calib", str(tmp_path / "missing.yaml")],
                           "missing.yaml")):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(pre + bad)
            assert e.value.code == 2 and word in capsys.readouterr().err, bad
    f = bag3d.parse_args(["--bag", "x", "--depth-out", "d", "--calib", str(calib), "--depth-size", "64x48"])
    assert f.depth_out == "d" and f.depth_topic == "" and f.depth_options == D.DepthOptions(64, 48)
    for bad, word in ((["--depth-out", "d", "--calib", str(calib), "--depth-size", "64x48", "--depth-encoding", "32FC1"],
                       "16UC1"), (["--depth-out", "d", "--depth-size", "64x48"], "--calib")):
        with pytest.raises(SystemExit) as e:
            bag3d.parse_args(["--bag", "x"] + bad)
        assert e.value.code == 2 and word in capsys.readouterr().err
