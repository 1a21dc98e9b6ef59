"""K26 on the device: ``tca_range2d`` is bit for bit the definition of ops/range2d.py."""
import numpy as np
import pytest
import torch

from test_range2d import CAL, CASES, M_EXACT, _det_msg, _rig_messages, check_case, rig
from triton_client_amd.ops import range2d as R
from triton_client_amd.ops.points_in_boxes import CloudLayout
from triton_client_amd.ros import compat, msgs

pytestmark = pytest.mark.gpu

F = np.float32
SENT = -1234567
LAYOUTS = {
    # name: (layout, bytes the payload starts past a 16-byte boundary)
    "record16": (CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7)), 0),  # one 16-byte load per point
    "step20": (CloudLayout(20, (4, 8, 12, 16), (7, 7, 7, 7)), 0),  # dword loads
    "odd_base": (CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7)), 1),  # byte loads
}
POINTS = (0, 1, 255, 256, 257, 5000)
BOXES = (0, 1, 127, 128, 129, 512)


def payload(points, lay):
    """The points' x, y, z as records of ``lay`` (the other bytes are noise)."""
    p = np.asarray(points, F).reshape(-1, 3)
    raw = np.random.default_rng(len(p)).integers(0, 256, (len(p), lay.point_step), dtype=np.uint8)
    for j in range(3):
        raw[:, lay.offsets[j]:lay.offsets[j] + 4] = np.ascontiguousarray(p[:, j]).view(np.uint8).reshape(-1, 4)
    return raw.tobytes()


def cloud_points(seed, n):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-10, 80, n), rng.uniform(-30, 30, n), rng.uniform(-2.5, 1.5, n)], 1).astype(F)


def pixel_boxes(seed, k):
    rng = np.random.default_rng(7000 + seed)
    b = np.stack([rng.uniform(0, 1242, k), rng.uniform(100, 375, k), rng.uniform(20, 300, k),
                  rng.uniform(20, 200, k)], 1).astype(F)
    if k > 3:
        b[k // 2] = np.nan  # a box that contains nothing, in the middle of the table
    return b


class Device:
    """One ranger for the module: every test launches on the same workspace."""

    def __init__(self, dev):
        self.ranger = R.CameraRanger(dev)

    def prepare(self, clouds, rows, M, opts=None, layout="record16"):
        lay, mis = LAYOUTS[layout]
        call = self.ranger.prepare([payload(p, lay) for p in clouds], [len(p) for p in clouds], lay, rows, M,
                                   opts or R.RangeOptions(), misalign=mis)
        call.out.view(torch.int32).fill_(SENT)  # the launch owns the records of its boxes, nothing past them
        return call

    @staticmethod
    def read(call, rows):
        torch.cuda.synchronize()
        words = call.out.view(torch.int32).cpu().numpy()
        assert (words[R.OUT_INTS * call.n_boxes:] == SENT).all(), "written past the last record"
        if call.n_boxes:
            assert (words[3:R.OUT_INTS * call.n_boxes:R.OUT_INTS] == 0).all()
        n, m, c, sums = R.unpack(words, call.n_boxes)
        out, k0 = [], 0
        for t in rows:
            out.append((n[k0:k0 + len(t)], m[k0:k0 + len(t)], c[k0:k0 + len(t)], sums[k0:k0 + len(t)]))
            k0 += len(t)
        return out

    def run(self, clouds, rows, M, opts=None, layout="record16"):
        call = self.prepare(clouds, rows, M, opts, layout)
        R.launch(call)
        return self.read(call, rows)


@pytest.fixture(scope="module")
def device(cuda):
    return Device(cuda)


def want_of(clouds, rows, M, o=None):
    o = o or R.RangeOptions()
    return [R.range2d_numpy(p, t, M, o.pct, o.min_points, o.bin_w, o.min_depth, o.window) for p, t in zip(clouds, rows)]


def same(got, want, what=""):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        for name, a, e in zip(("n", "m", "c", "sums"), g, w):
            assert a.dtype == e.dtype and a.shape == e.shape, (what, b, name)
            np.testing.assert_array_equal(a, e, err_msg=f"{what} cloud {b} {name}")


@pytest.fixture(scope="module")
def tables():
    """The box rows of every size and the definition's answer per (points, boxes): made once."""
    M = rig(3).M
    rows = {k: R.box_rows(pixel_boxes(k, k)) for k in BOXES}
    pts = {n: cloud_points(n, n) for n in POINTS}
    want = {(n, k): want_of([pts[n]], [rows[k]], M)[0] for n in POINTS for k in BOXES}
    assert (want[(5000, 512)][1] >= 0).sum() > 200 and (want[(257, 129)][0] > 0).sum() > 20
    return M, rows, pts, want


@pytest.mark.parametrize("n", POINTS)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_bit_for_bit_the_definition(device, tables, layout, n):
    M, rows, pts, want = tables
    for k in BOXES:
        same(device.run([pts[n]], [rows[k]], M, layout=layout), [want[(n, k)]], f"{layout} {n} points {k} boxes")


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_ragged_batches(device, layout):
    M = rig(5).M
    sizes = [[(700, 33)], [(300, 0), (0, 5)], [(0, 3), (1000, 140), (513, 0)], [(257, 7), (256, 512), (3000, 1)]]
    for batch in sizes:
        clouds = [cloud_points(10 + i, n) for i, (n, _) in enumerate(batch)]
        rows = [R.box_rows(pixel_boxes(20 + i, k)) for i, (_, k) in enumerate(batch)]
        want = want_of(clouds, rows, M)
        same(device.run(clouds, rows, M, layout=layout), want, f"{layout} {batch}")
    assert sum((w[1] >= 0).sum() for w in want) > 100


@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted_through_the_kernel(device, name):
    got = check_case(name, lambda pts, rows, M, o: device.run([pts], [rows], M, o)[0])
    pts, boxes, shrink, opts, _ = CASES[name]
    opts = dict(opts)
    M = opts.pop("M", M_EXACT)
    o = R.RangeOptions(shrink=shrink, **opts)
    same([tuple(got[k] for k in ("n", "m", "c", "sums"))], want_of([pts], [R.box_rows(boxes, shrink)], M, o), name)


def test_many_points_in_one_box_and_bin(device):
    # 4,096 points 2 m ahead, all in bin 8 of one box, next to a few elsewhere
    rng = np.random.default_rng(1)
    pts = np.stack([rng.uniform(8, 12, 4096), rng.uniform(19, 21, 4096), np.full(4096, 2.0)], 1).astype(F)
    pts = np.concatenate([pts, [[10, 20, 7.3], [10, 20, 2.3], [500, 20, 2]]]).astype(F)
    rows = R.box_rows(np.array([[10, 20, 8, 4], [10, 20, 800, 400]], F), 0.5)
    want = want_of([pts], [rows], M_EXACT)
    assert want[0][0].tolist() == [4096, 4098] and want[0][1].tolist() == [8, 8] and want[0][2].tolist() == [4096, 4097]
    same(device.run([pts], [rows], M_EXACT), want)


def test_relaunch_and_graph_replay(device):
    M = rig(8).M
    clouds = [cloud_points(40, 3000), cloud_points(41, 777)]
    rows = [R.box_rows(pixel_boxes(42, 130)), R.box_rows(pixel_boxes(43, 9))]
    want = want_of(clouds, rows, M)
    call = device.prepare(clouds, rows, M, layout="step20")
    R.launch(call)
    same(device.read(call, rows), want, "first launch")
    R.launch(call)  # the same workspace, not cleaned in between
    same(device.read(call, rows), want, "second launch")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        R.launch(call)
    for i in range(2):
        call.out.view(torch.int32).fill_(SENT)
        g.replay()
        same(device.read(call, rows), want, f"replay {i}")


def test_launcher_refusals(device):
    from triton_client_amd import _native

    M = rig(9).M
    clouds = [cloud_points(50, 300), cloud_points(51, 200)]
    rows = [R.box_rows(pixel_boxes(52, 6)), R.box_rows(pixel_boxes(53, 4))]
    call = device.prepare(clouds, rows, M)
    hist_before = call.hist.clone()
    fn = _native.kernels().tca_range2d
    p = _native.ptr
    base = dict(data=p(call.data), data_bytes=call.data_bytes, frame_off=p(call.frame_off), frame_n=p(call.frame_n),
                batch=2, max_n=300, step=16, ox=0, oy=4, oz=8, box_off=call.box_off.ctypes.data, table=p(call.table),
                M=call.M.ctypes.data, bin_w=0.25, min_depth=0.5, pct=50, min_points=3, window=1, hist=p(call.hist),
                out=p(call.out), stream=_native.stream_ptr())

    def rc(**kw):
        return fn(*{**base, **kw}.values())

    i32 = lambda v: np.asarray(v, np.int32)  # noqa: E731
    many = i32(np.arange(66))
    offs = {"513 boxes in a frame": i32([0, 513, 513]), "unordered offsets": i32([0, 7, 3]),
            "offsets that do not start at 0": i32([1, 6, 10])}
    bad = {"null data": dict(data=0), "null frame_off": dict(frame_off=0), "null frame_n": dict(frame_n=0),
           "null box_off": dict(box_off=0), "null table": dict(table=0), "null M": dict(M=0), "null hist": dict(hist=0),
           "null out": dict(out=0), "65 frames": dict(batch=65, box_off=many.ctypes.data),
           "misaligned table": dict(table=p(call.table) + 4), "pct 0": dict(pct=0), "pct 101": dict(pct=101),
           "min_points 0": dict(min_points=0), "window -1": dict(window=-1), "bin_w 0": dict(bin_w=0.0),
           "bin_w negative": dict(bin_w=-0.25), "bin_w inf": dict(bin_w=float("inf")),
           "bin_w nan": dict(bin_w=float("nan")), "min_depth nan": dict(min_depth=float("nan")),
           "min_depth inf": dict(min_depth=float("inf")), "2^31 payload bytes": dict(data_bytes=2 ** 31),
           "a field outside the record": dict(oz=16), "negative batch": dict(batch=-1)}
    bad.update({k: dict(box_off=v.ctypes.data) for k, v in offs.items()})
    for what, kw in bad.items():
        assert rc(**kw) != 0, what
    torch.cuda.synchronize()
    assert (call.out.view(torch.int32) == SENT).all() and torch.equal(call.hist, hist_before)  # nothing was launched
    assert rc() == 0
    same(device.read(call, rows), want_of(clouds, rows, M))
    assert _native.kernels().tca_range2d_bins() == R.NB


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
    from triton_client_amd.ros import rosmsg
    from triton_client_amd.ros.bus import TopicBus

    clouds, cams = _rig_messages()
    # cloud 3 gets a partner too: a camera message with many boxes
    rng = np.random.default_rng(3)
    wide = np.stack([rng.uniform(0, 1242, 200), rng.uniform(100, 300, 200), rng.uniform(20, 300, 200),
                     rng.uniform(20, 100, 200)], 1)
    cams.append(_det_msg(int(clouds[2].header.stamp.to_nsec()) - 2_000_000, wide, seq=103))

    def drive(env):
        monkeypatch.setenv("TCA_DEVICE_RANGE", env)
        bus = TopicBus()
        got = []
        compat.Subscriber("/ranged", msgs.Detection2DArray, lambda m: got.append(rosmsg.serialize(m)), bus=bus)
        drv = RosInference3D(engine=_GpuEngine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=4,
                             workers=2, queue_size=64, ranged_topic="/ranged", camera_detections_topic="/cam",
                             calibration=CAL)
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
        return got, drv

    on, drv_on = drive("1")
    off, drv_off = drive("0")
    assert len(on) == 4 and on == off
    assert drv_on.engine._ranger.gpu and drv_on.engine._ranger._stream is not None  # the kernel ran
    assert drv_off.engine._ranger._stream is None  # TCA_DEVICE_RANGE=0: the definition, on a GPU engine too
