"""K27 on the device: ``tca_depth_image`` is bit for bit the definition of ops/depth_image.py."""
import warnings

import numpy as np
import pytest
import torch

from test_depth_image import CASES, KITTI_H, KITTI_W, OPTS, at, check_case
from test_range2d import CAL, M_EXACT, _rig_messages
from triton_client_amd.ops import depth_image as D
from triton_client_amd.ops import range2d as R
from triton_client_amd.ops.cloud_common import CloudLayout, plan_staging
from triton_client_amd.ros import compat, msgs

pytestmark = pytest.mark.gpu

F = np.float32
SENT = 0xA5  # what the output buffer holds before a launch
LAYOUTS = {
    # name: (layout, bytes the payload starts past a 16-byte boundary)
    "record16": (CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7)), 0),  # one 16-byte load per point (path 2)
    "step32": (CloudLayout(32, (4, 8, 12, 16), (7, 7, 7, 7)), 0),  # dword loads (path 1)
    "step13": (CloudLayout(13, (1, 5, 9, -1), (7, 7, 7, 7)), 0),  # byte loads
    "record16_mis4": (CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7)), 4),  # path 2 lowered per frame to dwords
}
SIZES = ((37, 23), (64, 48))  # an odd width: the batch's pixel count is no multiple of four
POINTS = (0, 1, 255, 256, 257, 4099)
SPLATS = (0, 1, 4)
ENCODINGS = ("16UC1", "32FC1")


def payload(points, lay):
    """The points' x, y, z as records of ``lay`` (the other bytes are noise)."""
    p = np.asarray(points, F).reshape(-1, 3)
    raw = np.random.default_rng(len(p)).integers(0, 256, (len(p), lay.point_step), dtype=np.uint8)
    for j in range(3):
        raw[:, lay.offsets[j]:lay.offsets[j] + 4] = np.ascontiguousarray(p[:, j]).view(np.uint8).reshape(-1, 4)
    return raw.tobytes()


def camera(W, H, seed=0):
    """M of a pinhole camera that sees most of :func:`cloud_points` on a W x H image, slightly rotated."""
    e = np.random.default_rng(500 + seed).normal(0, 0.01, (3, 4))
    return (np.array([[W / 2, 0, W / 2, 0], [0, W / 2, H / 2, 0], [0, 0, 1, 0]]) + e).astype(F)


def cloud_points(seed, n):
    """Camera-frame points: x +-30, y +-20, z -1..80 — behind the camera, past every border, beyond
    65.535 m, and on a small image many to a pixel."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-30, 30, n), rng.uniform(-20, 20, n), rng.uniform(-1, 80, n)], 1).astype(F)


def bits(a):
    return np.ascontiguousarray(a).view("<u2" if a.dtype.itemsize == 2 else "<u4")


class Device:
    """One imager for the module: every test launches on the same workspace."""

    def __init__(self, dev):
        self.imager = D.DepthImager(dev)

    def prepare(self, clouds, M, opts, layout="record16"):
        lay, mis = LAYOUTS[layout]
        call = self.imager.prepare([payload(p, lay) for p in clouds], [len(p) for p in clouds], lay, M, opts,
                                   misalign=mis)
        call.out.fill_(SENT)  # the launch owns the pixels of its images, nothing past them
        return call

    @staticmethod
    def read(call):
        torch.cuda.synchronize()
        raw = call.out.cpu().numpy()
        assert (raw[call.out_bytes:] == SENT).all(), "written past the last image"
        return D.images_of(raw, call.batch, call.opts)

    def run(self, clouds, M, opts, layout="record16"):
        call = self.prepare(clouds, M, opts, layout)
        D.launch(call)
        return self.read(call)


@pytest.fixture(scope="module")
def device(cuda):
    return Device(cuda)


def same(got, want, what=""):
    assert len(got) == len(want), what
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, b)
        np.testing.assert_array_equal(bits(g), bits(w), err_msg=f"{what} cloud {b}")


@pytest.fixture(scope="module")
def tables():
    """The clouds of every size and the definition's image per (size, points, splat, encoding): made once."""
    pts = {n: cloud_points(n, n) for n in POINTS}
    Ms = {s: camera(*s) for s in SIZES}
    want = {}
    for (W, H) in SIZES:
        for n in POINTS:
            for s in SPLATS:
                for enc in ENCODINGS:
                    o = D.DepthOptions(W, H, encoding=enc, splat=s)
                    want[(W, H, n, s, enc)] = (o, D.depth_numpy(pts[n], Ms[(W, H)], o))
    lit = bits(want[(64, 48, 4099, 0, "16UC1")][1]) != 0
    assert 1000 < lit.sum() < 64 * 48  # most pixels hold a depth, not all
    return pts, Ms, want


@pytest.mark.parametrize("n", POINTS)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_bit_for_bit_the_definition(device, tables, layout, n):
    pts, Ms, want = tables
    for (W, H, n_, s, enc), (o, image) in want.items():
        if n_ == n:
            same(device.run([pts[n]], Ms[(W, H)], o, layout), [image], f"{layout} {W}x{H} {n} points splat {s} {enc}")


def test_a_camera_sized_image(device):
    pts = cloud_points(77, 4099)
    M = camera(1280, 720, 1)
    o = D.DepthOptions(1280, 720)
    want = D.depth_numpy(pts, M, o)
    assert (want != 0).sum() > 9 * 1000
    same(device.run([pts], M, o), [want], "1280x720")


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_ragged_batches(device, encoding):
    W, H = 37, 23
    M = camera(W, H, 2)
    o = D.DepthOptions(W, H, encoding=encoding)
    for layout, sizes in (("record16", [700, 0, 300]), ("step13", [5 + 3 * b for b in range(64)]),
                          ("record16_mis4", [257, 0, 0, 1])):
        clouds = [cloud_points(100 + b, n) for b, n in enumerate(sizes)]
        want = [D.depth_numpy(p, M, o) for p in clouds]
        got = device.run(clouds, M, o, layout)
        same(got, want, f"{layout} {sizes}")  # no plane leaks into another frame's
        for b in (0, 1, len(sizes) - 1):  # frame b's image is the single-cloud result
            same(device.run([clouds[b]], M, o, layout), [got[b]], f"{layout} alone {b}")
    empty = bits(want[1])
    assert (empty == (0 if encoding == "16UC1" else D.NAN_BITS)).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted_through_the_kernel(device, name):
    check_case(name, lambda pts, M, o: device.run([pts], M, o)[0])


@pytest.mark.parametrize("splat", (0, 4))
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_many_points_on_one_pixel(device, encoding, splat):
    # 4,096 points on pixel (5, 5) of a 12 x 10 image, every depth its own; the nearest is somewhere in the middle
    w = (F(2) + np.arange(4096, dtype=F) / F(64))
    w = w[np.random.default_rng(4).permutation(4096)]
    pts = np.stack([np.asarray(at(5.5, 5.5, d), F) for d in w])
    o = D.DepthOptions(12, 10, encoding=encoding, splat=splat)
    want = D.depth_numpy(pts, M_EXACT, o)
    assert want[5, 5] == (2000 if encoding == "16UC1" else F(2)) and int(np.argmin(w)) not in (0, 4095)
    sq = want[1:10, 1:10] if splat else want[5:6, 5:6]
    assert (sq == want[5, 5]).all() and (bits(want) != bits(want)[5, 5]).sum() == 120 - sq.size
    same(device.run([pts], M_EXACT, o), [want])


def test_relaunch_and_graph_replay(device):
    W, H = 64, 48
    M = camera(W, H, 3)
    o = D.DepthOptions(W, H, splat=1)
    first, second = cloud_points(40, 3000), cloud_points(41, 3000)
    want1, want2 = D.depth_numpy(first, M, o), D.depth_numpy(second, M, o)
    assert (want1 != want2).sum() > 500
    call = device.prepare([first], M, o, "step32")
    D.launch(call)
    same(device.read(call), [want1], "first launch")
    D.launch(call)  # the same plane, not cleaned in between
    same(device.read(call), [want1], "second launch")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.launch(call)
    for i in range(2):
        call.out.fill_(SENT)
        g.replay()
        same(device.read(call), [want1], f"replay {i}")
    # another cloud in the staged payload: the replay resets the plane itself and gives that cloud's image
    lay, mis = LAYOUTS["step32"]
    raw = torch.from_numpy(np.frombuffer(payload(second, lay), np.uint8).copy())
    at0 = plan_staging([3000], lay.point_step, mis, ()).frame_offs[0]
    call.data[at0:at0 + raw.numel()].copy_(raw)
    call.out.fill_(SENT)
    g.replay()
    same(device.read(call), [want2], "replay of another cloud")


def test_launcher_refusals(device):
    from triton_client_amd import _native

    W, H = 37, 23
    M = camera(W, H, 4)
    o = D.DepthOptions(W, H)
    clouds = [cloud_points(50, 300), cloud_points(51, 200)]
    call = device.prepare(clouds, M, o)
    call.plane.fill_(0x5A)
    plane_before = call.plane.clone()
    fn = _native.kernels().tca_depth_image
    p = _native.ptr
    base = dict(data=p(call.data), data_bytes=call.data_bytes, frame_off=p(call.frame_off), frame_n=p(call.frame_n),
                batch=2, max_n=300, step=16, ox=0, oy=4, oz=8, M=call.M.ctypes.data, W=W, H=H, enc=0, scale=1000.0,
                min_depth=0.5, splat=1, plane=p(call.plane), out=p(call.out), stream=_native.stream_ptr())

    def rc(**kw):
        return fn(*{**base, **kw}.values())

    bad = {"null data": dict(data=0), "null frame_off": dict(frame_off=0), "null frame_n": dict(frame_n=0),
           "null M": dict(M=0), "null plane": dict(plane=0), "null out": dict(out=0), "0 frames": dict(batch=0),
           "65 frames": dict(batch=65), "negative batch": dict(batch=-1), "W 0": dict(W=0), "W 4097": dict(W=4097),
           "H 0": dict(H=0), "H 4097": dict(H=4097), "splat -1": dict(splat=-1), "splat 5": dict(splat=5),
           "encoding 2": dict(enc=2), "encoding -1": dict(enc=-1), "min_depth 0": dict(min_depth=0.0),
           "min_depth negative": dict(min_depth=-0.5), "min_depth nan": dict(min_depth=float("nan")),
           "min_depth inf": dict(min_depth=float("inf")), "scale 0": dict(scale=0.0), "scale negative": dict(scale=-1.0),
           "scale nan": dict(scale=float("nan")), "scale inf": dict(scale=float("inf")),
           "a field outside the record": dict(oz=16), "a negative offset": dict(ox=-4),
           "negative data_bytes": dict(data_bytes=-1), "2^31 payload bytes": dict(data_bytes=2 ** 31),
           "negative max_n": dict(max_n=-1), "step 0": dict(step=0), "misaligned plane": dict(plane=p(call.plane) + 4),
           "misaligned out": dict(out=p(call.out) + 2)}
    for what, kw in bad.items():
        assert rc(**kw) != 0, what
    torch.cuda.synchronize()
    assert (call.out == SENT).all() and torch.equal(call.plane, plane_before)  # nothing was launched
    assert rc() == 0
    same(device.read(call), [D.depth_numpy(c, M, o) for c in clouds])


class _GpuEngine:
    """A duck-typed engine on the GPU: one box per cloud."""
    names = ["Car", "Pedestrian", "Cyclist"]
    z_offset, normalize, label_base = 0.0, True, 1
    device = "cuda"

    def detect(self, clouds):
        return [{"pred_boxes": np.array([[10.0 + c.header.seq, 0, 0, 4, 2, 1.5, 0.1]], F),
                 "pred_scores": np.array([0.9], F), "pred_labels": np.array([2])} for c in clouds]


def test_driver_publishes_the_definitions_bytes(cuda, monkeypatch):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.ros.bus import TopicBus

    clouds, _ = _rig_messages()

    def drive(env):
        monkeypatch.setenv("TCA_DEVICE_DEPTH", env)
        bus = TopicBus()
        got = []
        compat.Subscriber("/depth", msgs.Image, lambda m: got.append((m.header.seq, bytes(m.data))), bus=bus)
        drv = RosInference3D(engine=_GpuEngine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=4,
                             workers=2, queue_size=64, depth_topic="/depth", depth_options=OPTS, calibration=CAL)
        drv.start_inference(spin=False)
        pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
        for c in clouds:
            pub.publish(c)
        runner = drv.runner
        drv.stop()
        bus.close()
        assert runner is None or not runner.errors, runner.errors
        return got, drv

    on, drv_on = drive("1")
    off, drv_off = drive("0")
    want = [(c.header.seq, D.depth_numpy(R.cloud_xyzi(c), CAL.M, OPTS).tobytes()) for c in clouds]
    assert on == want and off == want and len(want[0][1]) == 2 * KITTI_W * KITTI_H
    assert drv_on.engine._depth_imager.gpu and drv_on.engine._depth_imager._stream is not None  # the kernel ran
    assert drv_off.engine._depth_imager._stream is None  # TCA_DEVICE_DEPTH=0: the definition, on a GPU engine too


def test_a_big_endian_cloud_goes_to_the_host_with_one_warning(cuda):
    clouds, _ = _rig_messages()
    c = clouds[0]
    swapped = msgs.PointCloud2(header=c.header, height=c.height, width=c.width, fields=c.fields, is_bigendian=True,
                               point_step=16, row_step=c.row_step,
                               data=np.frombuffer(c.data, "<f4").astype(">f4").tobytes(), is_dense=c.is_dense)
    im = D.DepthImager(cuda)
    want = D.depth_numpy(R.cloud_xyzi(c), CAL.M, OPTS)
    with pytest.warns(RuntimeWarning, match="little-endian FLOAT32"):
        got = im.images([c, swapped, clouds[1]], CAL.M, OPTS)
    same(got, [want, want, D.depth_numpy(R.cloud_xyzi(clouds[1]), CAL.M, OPTS)])
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # one warning in the object's life
        same(im.images([swapped], CAL.M, OPTS), [want])


def test_parts_bound_the_key_plane(cuda):
    clouds, _ = _rig_messages()
    im = D.DepthImager(cuda)
    big = D.DepthOptions(4096, 4096)
    parts = list(im._parts(list(range(10)), [clouds[0]] * 10, big))
    assert [len(p) for p in parts] == [4, 4, 2] and sum(parts, []) == list(range(10))
    assert all(4 * len(p) * 4096 * 4096 <= D.MAX_PLANE == 256 << 20 for p in parts)
    assert [len(p) for p in im._parts(list(range(150)), [clouds[0]] * 150, D.DepthOptions(37, 23))] == [64, 64, 22]
    with pytest.raises(ValueError, match="key plane"):  # and a launch that would exceed it is refused before staging
        im.prepare([clouds[0].data] * 5, [300] * 5, LAYOUTS["record16"][0], CAL.M, big)
