"""Rectification on the host (``ops/rectify.py``): the map against an independent float64
camera model, the integer definition against the float64 interpolation it rounds (exactly), the
calibration loader, and the 2D driver's ``rectify=`` option on a duck-typed CPU engine."""
import math

import numpy as np
import pytest
import yaml

import rectify_cases as C
from triton_client_amd.inference.ros_inference import RosInference
from triton_client_amd.ops import rectify as R
from triton_client_amd.ros import compat, msgs
from triton_client_amd.ros.bus import TopicBus

H, W = 96, 128


@pytest.fixture(scope="module")
def maps():
    return {n: R.rectify_map(C.model(n, H, W)) for n in C.DISTORTED}


# ------------------------------------------------------------------------------ identity
def test_identity_model_maps_every_pixel_to_itself():
    q = R.rectify_map(C.model("identity", 33, 130))
    u, v = np.meshgrid(np.arange(130), np.arange(33))
    assert q.dtype == np.int32 and q.shape == (33, 130, 2)
    np.testing.assert_array_equal(q[..., 0], 32 * u)
    np.testing.assert_array_equal(q[..., 1], 32 * v)
    frame = np.random.default_rng(1).integers(0, 256, (33, 130, 3), dtype=np.uint8)
    np.testing.assert_array_equal(R.rectify_numpy(frame, q), frame)


# ------------------------------------------------------------- definition against the reference
@pytest.mark.parametrize("name", C.DISTORTED)
def test_definition_is_the_rounded_float64_interpolation(maps, name):
    q = maps[name]
    cov = C.coverage(q)
    assert all(v > 0 for v in cov.values()), cov  # every edge, both clips, ax = ay = 16 and = 31
    rng = np.random.default_rng(len(name))
    for frame in (rng.integers(0, 256, (H, W, 3), dtype=np.uint8), np.full((H, W, 3), 255, np.uint8)):
        got = R.rectify_numpy(frame, q)
        ref = R.rectify_ref(frame, q)
        assert got.dtype == np.uint8 and got.shape == frame.shape
        np.testing.assert_array_equal(got, np.floor(ref + 0.5))
    clipped = (q[..., 0] == R.LOW) | (q[..., 1] == R.LOW) | (q[..., 0] == 32 * (W + 1)) | (q[..., 1] == 32 * (H + 1))
    assert (got[clipped] == 0).all()  # (of the all-white frame): a clipped entry is black


def test_a_frame_of_another_size_is_refused(maps):
    with pytest.raises(ValueError, match="130x33"):
        R.rectify_numpy(np.zeros((33, 130, 3), np.uint8), maps["barrel"])


# --------------------------------------------------------------- map against an independent model
def _forward(m, u, v):
    """Where output pixel (u, v) comes from, one pixel at a time with ``math``: written from the
    camera model's equations (normalise by P, rotate by R^-1, distort, project by K)."""
    fx, fy, cx, cy = m.P[0][0], m.P[1][1], m.P[0][2], m.P[1][2]
    ray = np.linalg.solve(np.array(m.R, np.float64), np.array([(u - cx) / fx, (v - cy) / fy, 1.0]))
    x, y = ray[0] / ray[2], ray[1] / ray[2]
    rr = x * x + y * y
    d = [float(c) for c in m.D]
    if m.model == "equidistant":
        r = math.sqrt(rr)
        th = math.atan(r)
        poly = sum(k * th ** (2 * (i + 1)) for i, k in enumerate(d))
        scale = th * (1.0 + poly) / r if r > 0 else 1.0
        xd, yd = x * scale, y * scale
    else:
        d = d + [0.0] * (8 - len(d))
        k1, k2, p1, p2, k3, k4, k5, k6 = d
        radial = (1 + rr * (k1 + rr * (k2 + rr * k3))) / (1 + rr * (k4 + rr * (k5 + rr * k6)))
        xd = x * radial + 2 * p1 * x * y + p2 * (rr + 2 * x * x)
        yd = y * radial + p1 * (rr + 2 * y * y) + 2 * p2 * x * y
    return m.K[0][0] * xd + m.K[0][2], m.K[1][1] * yd + m.K[1][2]


@pytest.mark.parametrize("name", C.DISTORTED)
def test_map_agrees_with_an_independent_forward_model(maps, name):
    m, q = C.model(name, H, W), maps[name]
    rng = np.random.default_rng(11)
    checked = 0
    for u, v in zip(rng.integers(0, W, 200), rng.integers(0, H, 200)):
        mx, my = _forward(m, int(u), int(v))
        for got, want, side in ((int(q[v, u, 0]), mx, W), (int(q[v, u, 1]), my, H)):
            if R.LOW < got < 32 * (side + 1):
                assert abs(got / 32 - want) <= 1 / 64, (name, u, v)
                checked += 1
            else:  # clipped: the model is at or beyond the clip value
                assert want * 32 <= R.LOW + 0.5 if got == R.LOW else want * 32 >= 32 * (side + 1) - 0.5
    assert checked > 100


def test_principal_point_and_mirror_symmetry():
    K = [[70.0, 0, 31.0], [0, 70.0, 20.0], [0, 0, 1]]
    for kind, D in (("plumb_bob", [-0.3, 0.1, 0.0, 0.0, 0.02]), ("rational_polynomial", [0.5, 0.1, 0, 0, 0, 0.9, 0, 0]),
                    ("equidistant", [0.05, -0.01, 0.0, 0.0])):
        q = R.rectify_map(R.CameraModel(width=63, height=41, K=K, D=D, model=kind))
        assert tuple(q[20, 31]) == (32 * 31, 32 * 20)  # the principal point maps to itself
        # p1 = p2 = 0: mirroring u about cx mirrors qx and keeps qy
        np.testing.assert_array_equal(q[:, ::-1, 0] - 32 * 31, -(q[..., 0] - 32 * 31))
        np.testing.assert_array_equal(q[:, ::-1, 1], q[..., 1])
    assert (R.rectify_map(R.CameraModel(width=8, height=4, K=K, D=[float("1e308")] * 5))[0, 0] == R.LOW).all()


def test_map_agrees_with_opencv_when_it_is_installed(maps):
    cv2 = pytest.importorskip("cv2")
    m = C.model("barrel", H, W)
    mx, my = cv2.initUndistortRectifyMap(m.K, m.D, m.R, m.P[:, :3], (W, H), cv2.CV_32FC1)
    q = maps["barrel"]
    inside = (q[..., 0] > R.LOW) & (q[..., 0] < 32 * (W + 1)) & (q[..., 1] > R.LOW) & (q[..., 1] < 32 * (H + 1))
    assert np.abs(q[..., 0] / 32 - mx)[inside].max() <= 1 / 64 + 1e-3  # (its map is float32)
    assert np.abs(q[..., 1] / 32 - my)[inside].max() <= 1 / 64 + 1e-3


# ----------------------------------------------------------------------- loader and validation
def _ost(m, **drop):
    doc = {"image_width": m.width, "image_height": m.height, "camera_name": "cam",
           "camera_matrix": {"rows": 3, "cols": 3, "data": m.K.reshape(-1).tolist()},
           "distortion_model": m.model,
           "distortion_coefficients": {"rows": 1, "cols": int(m.D.size), "data": m.D.tolist()},
           "rectification_matrix": {"rows": 3, "cols": 3, "data": m.R.reshape(-1).tolist()},
           "projection_matrix": {"rows": 3, "cols": 4, "data": m.P.reshape(-1).tolist()}}
    for k in drop:
        del doc[k]
    return doc


@pytest.mark.parametrize("name", ["barrel", "rational", "equidistant"])
def test_ost_yaml_round_trip(tmp_path, name):
    m = C.model(name, 40, 56)
    path = tmp_path / "ost.yaml"
    path.write_text(yaml.safe_dump(_ost(m)))
    got = R.load_camera_model(str(path))
    assert (got.width, got.height, got.model) == (56, 40, m.model)
    for a in ("K", "D", "R", "P"):
        np.testing.assert_array_equal(getattr(got, a), getattr(m, a))
    np.testing.assert_array_equal(R.rectify_map(got), R.rectify_map(m))
    # R and P are optional: identity and [K | 0]
    path.write_text(yaml.safe_dump(_ost(m, rectification_matrix=1, projection_matrix=1)))
    got = R.load_camera_model(str(path))
    np.testing.assert_array_equal(got.R, np.eye(3))
    np.testing.assert_array_equal(got.P, np.hstack([m.K, np.zeros((3, 1))]))


@pytest.mark.parametrize("key", ["image_width", "image_height", "camera_matrix", "distortion_model",
                                 "distortion_coefficients"])
def test_a_missing_key_is_named(tmp_path, key):
    path = tmp_path / "ost.yaml"
    path.write_text(yaml.safe_dump(_ost(C.model("barrel", 40, 56), **{key: 1})))
    with pytest.raises(ValueError, match=key):
        R.load_camera_model(str(path))


def test_validation():
    K = np.array([[50.0, 0, 20], [0, 50.0, 15], [0, 0, 1]])
    ok = dict(width=40, height=30, K=K, D=[0.1, 0, 0, 0, 0])
    R.CameraModel(**ok)
    R.CameraModel(**{**ok, "D": [0.1, 0, 0, 0]})  # plumb_bob with k3 = 0
    for bad in ({"D": [0.1, 0, 0]}, {"D": [0.0] * 8}, {"D": [0.0] * 5, "model": "equidistant"},
                {"D": [0.0] * 5, "model": "rational_polynomial"}, {"model": "fisheye"},
                {"width": 0}, {"height": 0}, {"width": 4097}, {"height": 4097}, {"width": 40.0}, {"width": True},
                {"K": np.diag([0.0, 50.0, 1.0])}, {"K": np.diag([50.0, 0.0, 1.0])}, {"K": np.eye(2)},
                {"P": np.hstack([np.diag([0.0, 50.0, 1.0]), np.zeros((3, 1))])},
                {"P": np.hstack([np.diag([50.0, 0.0, 1.0]), np.zeros((3, 1))])},
                {"D": [float("nan"), 0, 0, 0, 0]}, {"K": np.full((3, 3), np.inf)}, {"R": np.full((3, 3), np.nan)}):
        with pytest.raises(ValueError):
            R.CameraModel(**{**ok, **bad})


def test_rectifier_on_the_host_is_the_definition(maps):
    m = C.model("barrel", H, W)
    rec = R.Rectifier(m, device="cpu")
    assert rec.kind == "host definition" and not rec.gpu
    frames = [np.random.default_rng(s).integers(0, 256, (H, W, 3), dtype=np.uint8) for s in range(3)]
    for f, g in zip(frames, rec.frames(frames)):
        np.testing.assert_array_equal(g, R.rectify_numpy(f, maps["barrel"]))
    with pytest.raises(ValueError, match="64x48.*128x96"):
        rec.frames([np.zeros((48, 64, 3), np.uint8)])
    for bad in (np.zeros((H, W, 3), np.float32), np.zeros((H, W, 4), np.uint8), np.zeros((H, W), np.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            rec.frames([bad])
    with pytest.raises(ValueError, match="GPU"):
        rec.rectify_(None, None)


# --------------------------------------------------------------------------------- the driver
FH, FW = 40, 56


class _Engine:
    """A CPU engine by duck typing (no ``live``, no ``rectifier``): one box per frame, placed by the
    frame's brightest pixel, so the detections tell which pixels the engine saw."""
    names = ["thing"]

    def __init__(self):
        self.seen = []

    def detect(self, frames):
        out = []
        for f in frames:
            self.seen.append(np.array(f))
            y, x = np.unravel_index(int(np.argmax(f.astype(np.int32).sum(2))), f.shape[:2])
            out.append(np.array([[x, y, x + 4, y + 3, 0.5 + f[y, x, 0] / 1024.0, 0]], np.float32))
        return out


def _frames():
    rng = np.random.default_rng(5)
    out = []
    for s in range(4):
        f = rng.integers(0, 200, (FH, FW, 3), dtype=np.uint8)
        f[8 + 5 * s, 12 + 9 * s] = (255, 250, 251)  # the brightest pixel, well inside the rectified view
        out.append(f)
    return out


def _drive(batched, **kw):
    bus = TopicBus()
    frames, dets = [], []
    bus.subscribe("/out", frames.append)
    bus.subscribe("/out/detections", dets.append)
    eng = _Engine()
    drv = RosInference(engine=eng, params={"sub_topic": "/cam", "pub_topic": "/out"}, bus=bus, draw=False,
                       queue_size=None, **(dict(batch=2, workers=2) if batched else {}), **kw)
    drv.start_inference(spin=False)
    sent = [compat.numpy_to_imgmsg(f, "rgb8", header=msgs.Header(seq=i + 1, frame_id="cam"))
            for i, f in enumerate(_frames())]
    for m in sent:
        bus.publish("/cam", m)
    assert bus.wait_idle(30)
    runner = drv.runner
    drv.stop(drain=True)
    assert bus.wait_idle(30)
    bus.close()
    assert runner is None or not runner.errors, runner.errors
    return sent, frames, dets, eng


@pytest.mark.parametrize("batched", [False, True], ids=["one_per_callback", "batch2_workers2"])
def test_driver_publishes_the_rectified_frame_and_its_detections(batched):
    m = C.model("barrel", FH, FW)
    q = R.rectify_map(m)
    sent, frames, dets, eng = _drive(batched, rectify=m)
    assert [f.header.seq for f in frames] == [1, 2, 3, 4] == [d.header.seq for d in dets]
    want = [R.rectify_numpy(f, q) for f in _frames()]
    assert any((w != f).any() for w, f in zip(want, _frames()))
    seen = sorted(eng.seen, key=lambda a: a.tobytes())
    for a, b in zip(seen, sorted(want, key=lambda a: a.tobytes())):
        np.testing.assert_array_equal(a, b)  # the engine saw the rectified frames, nothing else
    for s, f, d, w in zip(sent, frames, dets, want):
        assert (f.header.seq, f.header.frame_id, f.header.stamp) == (s.header.seq, "cam", s.header.stamp)
        assert (f.encoding, f.height, f.width, f.step) == ("rgb8", FH, FW, 3 * FW)
        np.testing.assert_array_equal(np.frombuffer(f.data, np.uint8).reshape(FH, FW, 3), w)
        np.testing.assert_array_equal(d.detections.columns["dets"], _Engine().detect([w])[0])


def test_driver_takes_a_calibration_file_and_refuses_another_frame_size(tmp_path):
    m = C.model("pincushion", FH, FW)
    path = tmp_path / "ost.yaml"
    path.write_text(yaml.safe_dump(_ost(m)))
    drv = RosInference(engine=_Engine(), params={"sub_topic": "/cam", "pub_topic": "/out"}, draw=False,
                       rectify=str(path))
    f = _frames()[0]
    (im, _, _), = drv.process([compat.numpy_to_imgmsg(f, "rgb8", header=msgs.Header(seq=1))])
    np.testing.assert_array_equal(np.frombuffer(im.data, np.uint8).reshape(FH, FW, 3),
                                  R.rectify_numpy(f, R.rectify_map(m)))
    with pytest.raises(ValueError, match="64x48.*56x40"):
        drv.process([compat.numpy_to_imgmsg(np.zeros((48, 64, 3), np.uint8), "rgb8", header=msgs.Header(seq=2))])
    with pytest.raises(ValueError, match="rectify"):
        RosInference(engine=_Engine(), params={"sub_topic": "/cam", "pub_topic": "/out"}, rectify=3)


def test_option_off_changes_nothing():
    sent, frames, dets, eng = _drive(False)
    _, frames0, dets0, _ = _drive(False, rectify=None)
    assert [bytes(f.data) for f in frames] == [bytes(f.data) for f in frames0] == [bytes(s.data) for s in sent]
    for d, d0 in zip(dets, dets0):
        np.testing.assert_array_equal(d.detections.columns["dets"], d0.detections.columns["dets"])
    for a, f in zip(eng.seen, _frames()):
        np.testing.assert_array_equal(a, f)


def test_ring_engines_refuse_the_option():
    class Ring(_Engine):
        compressed_out = False

    with pytest.raises(ValueError, match="rectify"):
        RosInference(engine=Ring(), params={"sub_topic": "/cam", "pub_topic": "/out"},
                     rectify=C.model("barrel", FH, FW))
    RosInference(engine=Ring(), params={"sub_topic": "/cam", "pub_topic": "/out"})
