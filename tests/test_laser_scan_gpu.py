"""K29 on the device: ``tca_laser_scan`` is bit for bit the definition of ops/laser_scan.py."""
import math
import warnings

import numpy as np
import pytest
import torch

from test_laser_scan import CASES, OPTS, check_case, scene_points
from test_range2d import _rig_messages
from triton_client_amd.ops import laser_scan as L
from triton_client_amd.ops import range2d as R
from triton_client_amd.ops.cloud_common import CloudLayout, plan_staging
from triton_client_amd.ros import compat, msgs

pytestmark = pytest.mark.gpu

F = np.float32
PI = math.pi
SENT = 0xA5  # what the output buffer holds before a launch
LAYOUTS = {
    # name: (layout, bytes the payload starts past a 16-byte boundary)
    "record16": (CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7)), 0),  # one 16-byte load per point (path 2)
    "step32": (CloudLayout(32, (4, 12, 20, 28), (7, 7, 7, 7)), 0),  # x, y, z at odd dword positions (path 1)
    "step18": (CloudLayout(18, (1, 5, 9, -1), (7, 7, 7, 7)), 0),  # byte loads
    "record16_mis4": (CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7)), 4),  # path 2 lowered per frame to dwords
    "record16_mis1": (CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7)), 1),  # and to bytes
}
# n = 1: one wide bin; 360; 4096 (k = 32 blocks per workgroup: 5000 points are one workgroup's).  At 360 bins a
# workgroup walks 4 blocks of 256: 5000 points are 20 blocks, five workgroups that flush into the same bins.
BINS = {1: dict(angle_increment=7.0), 360: {}, 4096: dict(angle_increment=2 * PI / 4096)}
POINTS = (0, 1, 255, 256, 257, 5000)


def payload(points, lay):
    """The points' x, y, z as records of ``lay`` (the other bytes are noise)."""
    p = np.asarray(points, F).reshape(-1, 3)
    raw = np.random.default_rng(len(p)).integers(0, 256, (len(p), lay.point_step), dtype=np.uint8)
    for j in range(3):
        raw[:, lay.offsets[j]:lay.offsets[j] + 4] = np.ascontiguousarray(p[:, j]).view(np.uint8).reshape(-1, 4)
    return raw.tobytes()


def cloud_points(seed, n):
    """The CPU file's scene cut to ``n`` points in a seeded order: Gaussian points and the 30 m ring."""
    pts = scene_points(seed, 20000)
    return pts[np.random.default_rng(seed).permutation(len(pts))[:n]]


class Device:
    """One scanner for the module: every test launches on the same workspace."""

    def __init__(self, dev):
        self.scanner = L.LaserScanner(dev)

    def prepare(self, clouds, opts, layout="record16"):
        lay, mis = LAYOUTS[layout]
        call = self.scanner.prepare([payload(p, lay) for p in clouds], [len(p) for p in clouds], lay, opts, misalign=mis)
        call.out.fill_(SENT)  # the launch owns its scans' ranges, nothing past them
        return call

    @staticmethod
    def read(call):
        torch.cuda.synchronize()
        raw = call.out.cpu().numpy()
        assert (raw[call.out_bytes:] == SENT).all(), "written past the last scan"
        return L.ranges_of(raw, call.batch, call.opts)

    def run(self, clouds, opts, layout="record16", privatise=True):
        call = self.prepare(clouds, opts, layout)
        L.launch(call, privatise=privatise)
        return self.read(call)


@pytest.fixture(scope="module")
def device(cuda):
    return Device(cuda)


def same(got, want, what=""):
    assert len(got) == len(want), what
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype == np.dtype("<f4") and g.shape == w.shape, (what, b)
        np.testing.assert_array_equal(g.view("<u4"), w.view("<u4"), err_msg=f"{what} cloud {b}")


@pytest.fixture(scope="module")
def tables():
    """The clouds of every size and the definition's ranges per (bins, points, use_inf): made once."""
    pts = {n: cloud_points(n, n) for n in POINTS}
    want = {}
    for bins, kw in BINS.items():
        for n in POINTS:
            for use_inf in (True, False):
                o = L.ScanOptions(use_inf=use_inf, **kw)
                assert o.n == bins
                want[(bins, n, use_inf)] = (o, L.scan_numpy(pts[n], o))
    full = want[(360, 5000, True)][1]
    assert np.isfinite(full).sum() > 300  # nearly every ray of the 5000-point scan has a return ...
    b, valid, _ = L.scan_keys_numpy(pts[5000], want[(360, 5000, True)][0])
    # ... and the five workgroups (workgroup w walks blocks w, w + 5, ...) flush into the same bins
    owners = [set(b[valid & (np.arange(5000) // 256 % 5 == w)]) for w in range(5)]
    assert len(set.intersection(*owners)) > 100
    assert np.isinf(want[(4096, 5000, True)][1]).sum() > 1000  # at 4096 bins most rays find nothing
    return pts, want


@pytest.mark.parametrize("n", POINTS)
@pytest.mark.parametrize("layout", ["record16", "step32", "step18"])
def test_bit_for_bit_the_definition(device, tables, layout, n):
    pts, want = tables
    for (bins, n_, use_inf), (o, ranges) in want.items():
        if n_ == n:
            same(device.run([pts[n]], o, layout), [ranges], f"{layout} {bins} bins {n} points use_inf {use_inf}")


@pytest.mark.parametrize("bins", sorted(BINS))
def test_global_atomics_alone_give_the_same_bytes(device, tables, bins):
    pts, want = tables
    o, ranges = want[(bins, 5000, True)]
    same(device.run([pts[5000]], o, privatise=False), [ranges], f"{bins} bins")


def test_two_workgroups_at_4096_bins(device):
    # 32 blocks to a workgroup at 4096 bins: 8,500 points are 34 blocks, two workgroups with 16 KiB of bins each
    o = L.ScanOptions(angle_increment=2 * PI / 4096)
    pts = cloud_points(7, 8500)
    b, valid, _ = L.scan_keys_numpy(pts, o)
    blk = np.arange(8500) // 256 % 2
    assert len(set(b[valid & (blk == 0)]) & set(b[valid & (blk == 1)])) > 100
    same(device.run([pts, pts[:300]], o, "step32"), [L.scan_numpy(pts, o), L.scan_numpy(pts[:300], o)])


@pytest.mark.parametrize("layout", ["record16", "record16_mis4", "record16_mis1"])
def test_ragged_batches(device, layout):
    o = L.ScanOptions(range_max=60.0)
    sizes = (0, 1, 257, 3000, 64)
    clouds = [cloud_points(100 + b, n) for b, n in enumerate(sizes)]
    want = [L.scan_numpy(p, o) for p in clouds]
    got = device.run(clouds, o, layout)
    same(got, want, f"{layout} {sizes}")  # no scan leaks into another frame's
    assert (want[0].view("<u4") == L.INF_BITS).all()
    for b in (1, 3):  # frame b's scan is the single-cloud result
        same(device.run([clouds[b]], o, layout), [got[b]], f"{layout} alone {b}")


def test_a_batch_of_64_tiny_clouds(device):
    o = L.ScanOptions(use_inf=False)
    clouds = [cloud_points(200 + b, 5 + 3 * b) for b in range(64)]
    same(device.run(clouds, o, "step18"), [L.scan_numpy(p, o) for p in clouds])


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_many_points_in_one_bin(device, order):
    # 4,096 points along one ray, every range its own; 1-degree bins
    r = F(2) + np.arange(4096, dtype=F) / F(64)
    r = {"ascending": r, "descending": r[::-1], "shuffled": r[np.random.default_rng(4).permutation(4096)]}[order]
    pts = np.stack([r * F(0.8), r * F(0.6), np.zeros(4096, F)], 1)
    o = L.ScanOptions()
    want = L.scan_numpy(pts, o)
    assert np.isfinite(want).sum() == 1 and abs(float(want[np.isfinite(want)][0]) - 2.0) < 1e-6
    same(device.run([pts], o), [want])


def test_one_point_in_every_bin(device):
    # the same 4,096 ranges, one per bin of a 4096-bin scan: at each bin's centre
    o = L.ScanOptions(angle_increment=2 * PI / 4096)
    a = -PI + (np.arange(4096) + 0.5) * (2 * PI / 4096)
    r = 2 + np.random.default_rng(5).permutation(4096) / 64
    pts = np.stack([r * np.cos(a), r * np.sin(a), np.zeros(4096)], 1).astype(F)
    want = L.scan_numpy(pts, o)
    assert np.isfinite(want).all() and len(set(want.tolist())) > 4000
    same(device.run([pts], o), [want])


@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted_through_the_kernel(device, name):
    check_case(name, lambda pts, o: device.run([pts], o)[0])


def test_relaunch_and_graph_replay(device):
    o = L.ScanOptions(range_max=60.0)
    first, second = cloud_points(40, 3000), cloud_points(41, 3000)
    want1, want2 = L.scan_numpy(first, o), L.scan_numpy(second, o)
    assert (want1 != want2).sum() > 200
    call = device.prepare([first], o, "step32")
    L.launch(call)
    same(device.read(call), [want1], "first launch")
    call.plane.fill_(0x11)  # garbage in the plane and in the output: the launch owns its reset
    call.out.fill_(SENT)
    L.launch(call)
    same(device.read(call), [want1], "second launch")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.launch(call)
    for i in range(2):
        call.out.fill_(SENT)
        g.replay()
        same(device.read(call), [want1], f"replay {i}")
    # another cloud in the staged payload: the replay resets the plane itself and gives that cloud's scan
    lay, mis = LAYOUTS["step32"]
    raw = torch.from_numpy(np.frombuffer(payload(second, lay), np.uint8).copy())
    at0 = plan_staging([3000], lay.point_step, mis, ()).frame_offs[0]
    call.data[at0:at0 + raw.numel()].copy_(raw)
    call.out.fill_(SENT)
    g.replay()
    same(device.read(call), [want2], "replay of another cloud")


def test_launcher_refusals(device):
    from triton_client_amd import _native

    o = L.ScanOptions()
    clouds = [cloud_points(50, 300), cloud_points(51, 200)]
    call = device.prepare(clouds, o)
    call.plane.fill_(0x5A)
    plane_before = call.plane.clone()
    fn = _native.kernels().tca_laser_scan
    p = _native.ptr
    nan, inf = float("nan"), float("inf")
    base = dict(data=p(call.data), data_bytes=call.data_bytes, frame_off=p(call.frame_off), frame_n=p(call.frame_n),
                batch=2, max_n=300, step=16, ox=0, oy=4, oz=8, table=p(call.table), n=360, h0=-1.0, h1=1.0, r0=0.45,
                r1=100.0, empty=L.INF_BITS, privatise=1, plane=p(call.plane), out=p(call.out),
                stream=_native.stream_ptr())

    def rc(**kw):
        return fn(*{**base, **kw}.values())

    bad = {"null data": dict(data=0), "null frame_off": dict(frame_off=0), "null frame_n": dict(frame_n=0),
           "null table": dict(table=0), "null plane": dict(plane=0), "null out": dict(out=0), "0 frames": dict(batch=0),
           "65 frames": dict(batch=65), "negative batch": dict(batch=-1), "0 bins": dict(n=0), "4097 bins": dict(n=4097),
           "min_height nan": dict(h0=nan), "max_height nan": dict(h1=nan), "min_height > max_height": dict(h0=1.5),
           "range_min nan": dict(r0=nan), "range_max nan": dict(r1=nan), "range_max inf": dict(r1=inf),
           "range_min inf": dict(r0=inf), "range_min negative": dict(r0=-0.5), "range_min == range_max": dict(r0=100.0),
           "range_min > range_max": dict(r0=200.0), "a field outside the record": dict(oz=16),
           "a negative offset": dict(ox=-4), "negative data_bytes": dict(data_bytes=-1),
           "2^31 payload bytes": dict(data_bytes=2 ** 31), "negative max_n": dict(max_n=-1), "step 0": dict(step=0),
           "privatise 2": dict(privatise=2), "misaligned plane": dict(plane=p(call.plane) + 2),
           "misaligned out": dict(out=p(call.out) + 2), "misaligned table": dict(table=p(call.table) + 1),
           "misaligned frame_off": dict(frame_off=p(call.frame_off) + 4),
           "misaligned frame_n": dict(frame_n=p(call.frame_n) + 2)}
    for what, kw in bad.items():
        assert rc(**kw) == 1, what  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (call.out == SENT).all() and torch.equal(call.plane, plane_before)  # nothing was launched
    assert rc() == 0
    same(device.read(call), [L.scan_numpy(c, o) for c in clouds])
    assert rc(h0=-inf, h1=inf) == 0  # the heights may be infinite
    wide = L.ScanOptions(min_height=-inf, max_height=inf)
    same(device.read(call), [L.scan_numpy(c, wide) for c in clouds])


def test_a_record_past_data_bytes_is_not_read(device):
    o = L.ScanOptions(min_height=-np.inf, max_height=np.inf)
    pts = cloud_points(60, 700)
    pts[-1] = (0.5, 0.01, 0.0)  # the last point is the nearest return of its ray
    assert (L.scan_numpy(pts, o) != L.scan_numpy(pts[:-1], o)).sum() == 1 and L.scan_numpy(pts, o).min() < 0.51
    call = device.prepare([pts], o)
    call.data_bytes = 16 * 700 - 16  # one record short (the staged bytes end 16-byte aligned: 700 * 16)
    L.launch(call)
    same(device.read(call), [L.scan_numpy(pts[:-1], o)])
    call.data_bytes = 16 * 700 - 1  # and a record that only ends past it
    L.launch(call)
    same(device.read(call), [L.scan_numpy(pts[:-1], o)])


# ------------------------------------------------------------------------ through the engine
class _GpuEngine:
    """A duck-typed engine on the GPU: one box per cloud."""
    names = ["Car", "Pedestrian", "Cyclist"]
    z_offset, normalize, label_base = 0.0, True, 1
    device = "cuda"

    def detect(self, clouds):
        return [{"pred_boxes": np.array([[10.0 + c.header.seq, 0, 0, 4, 2, 1.5, 0.1]], F),
                 "pred_scores": np.array([0.9], F), "pred_labels": np.array([2])} for c in clouds]


def _swapped(c):
    return msgs.PointCloud2(header=c.header, height=c.height, width=c.width, fields=c.fields, is_bigendian=True,
                            point_step=16, row_step=c.row_step,
                            data=np.frombuffer(c.data, "<f4").astype(">f4").tobytes(), is_dense=c.is_dense)


def test_engine_scans_equal_the_definitions_messages(cuda, monkeypatch):
    from triton_client_amd.inference.engines import Detector3D

    clouds, _ = _rig_messages()
    want = [L.scan_message(c, L.scan_numpy(R.cloud_xyzi(c), OPTS), OPTS, "base") for c in clouds]
    eng = _GpuEngine()
    assert Detector3D.laser_scans(eng, clouds, OPTS, "base") == want
    sc = Detector3D.laser_scanner(eng)
    assert sc is eng._laser_scanner and sc.gpu and sc._stream is not None  # made once; the kernel ran
    monkeypatch.setenv("TCA_DEVICE_SCAN", "0")
    other = _GpuEngine()
    assert Detector3D.laser_scans(other, clouds, OPTS, "base") == want
    assert other._laser_scanner.gpu and other._laser_scanner._stream is None  # the definition, on a GPU engine too


def test_a_big_endian_cloud_goes_to_the_host_with_one_warning(cuda):
    clouds, _ = _rig_messages()
    c = clouds[0]
    sc = L.LaserScanner(cuda)
    want = L.scan_numpy(R.cloud_xyzi(c), OPTS)
    with pytest.warns(RuntimeWarning, match="little-endian FLOAT32") as rec:
        got = sc.ranges([c, _swapped(c), clouds[1]], OPTS)
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    same(got, [want, want, L.scan_numpy(R.cloud_xyzi(clouds[1]), OPTS)])
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # one warning in the object's life
        same(sc.ranges([_swapped(c)], OPTS), [want])


def test_driver_publishes_the_definitions_bytes(cuda, monkeypatch):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.ros.bus import TopicBus

    clouds, _ = _rig_messages()

    def drive(env):
        monkeypatch.setenv("TCA_DEVICE_SCAN", env)
        bus = TopicBus()
        got = []
        compat.Subscriber("/scan", msgs.LaserScan, lambda m: got.append((m.header.seq, m.ranges.tobytes())), bus=bus)
        drv = RosInference3D(engine=_GpuEngine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=4,
                             workers=2, queue_size=64, scan_topic="/scan", scan_options=OPTS)
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
    want = [(c.header.seq, L.scan_numpy(R.cloud_xyzi(c), OPTS).tobytes()) for c in clouds]
    assert on == want and off == want and len(want[0][1]) == 4 * 360
    assert drv_on.engine._laser_scanner.gpu and drv_on.engine._laser_scanner._stream is not None  # the kernel ran
    assert drv_off.engine._laser_scanner._stream is None  # TCA_DEVICE_SCAN=0: the definition, on a GPU engine too
