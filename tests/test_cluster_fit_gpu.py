"""K32 on the device: ``tca_cluster_fit`` gives, byte for byte, the fit table of the definition of ops/cluster_fit.py,
behind ``tca_cluster`` on what that launch left on the device."""
import numpy as np
import pytest
import torch

from test_cluster import SHAPES, F, grid, place
from test_cluster_gpu import SENT, Device, scene
from test_ground_gpu import cloud_points
from test_laser_scan_gpu import _GpuEngine
from test_range2d import _rig_messages
from triton_client_amd.ops import cluster as C
from triton_client_amd.ops import cluster_fit as K
from triton_client_amd.ops import ground as G

pytestmark = pytest.mark.gpu

N = K.CHUNK
# 320 clusters of 1 to 64 points, then clusters of exactly CHUNK, CHUNK + 1 and 3 * CHUNK + 12 points over a few cells
MANY = [(2 * i, 2 * j, 1 + (7 * i + 13 * j) % 64) for i in range(20) for j in range(16)] + \
    [(60, 10, N // 2), (61, 10, N // 2), (60, 20, N // 2), (61, 21, N // 2 + 1)] + [(70 + i, 40, N // 2 + 2) for i in range(6)]
WIDE = [(i, 3, 2) for i in range(140)] + [(5, 6, 9)]  # 70 m of touching cells: oversize; and one small cluster behind it


@pytest.fixture(scope="module")
def device(cuda):
    return Device(cuda)


def check(device, clouds, o, fo, layout="step16", ground=None, split=True):
    """``tca_cluster`` and ``tca_cluster_fit`` on ``clouds`` → the fit call, its output compared with the definition."""
    res, call = device.run(clouds, o, layout, ground=ground)
    f = K.prepare(device.ex, call, fo)
    f.fit.fill_(SENT)
    K.launch(f, split=split)
    torch.cuda.synchronize()
    rows = f.fit[:f.fit_bytes].cpu().numpy().view(K.FIT_DTYPE).reshape(len(clouds), o.max_clusters)
    for b, (pts, (found, label, table)) in enumerate(zip(clouds, res)):
        pts = C.obstacle_rows(pts, ground) if ground is not None else pts
        want = K.fit_numpy(pts, label, table, fo)
        assert rows[b, :len(table)].tobytes() == want.tobytes(), (b, rows[b, :len(table)], want)
        assert rows[b, len(table):].tobytes() == bytes(K.FIT_ROW * (o.max_clusters - len(table)))  # zero past found
    return f, rows


@pytest.mark.parametrize("angles", [2, 90, 128])
def test_small_and_split_clusters_byte_for_byte(device, angles):
    o, fo = grid(96, 64, min_points=1), K.FitOptions(angles=angles, d0=0.05)
    pts = place(MANY, 3)
    f, rows = check(device, [pts], o, fo)
    n = rows[0]["score"] > 0
    assert n.sum() == 323 and sorted(C.cluster_numpy(pts, o)[2]["n"])[-3:] == [N, N + 1, 3 * N + 12]
    for buf in (f.plan, f.grouped, f.slots, f.work):  # garbage in the workspace: a launch owns what it reads
        buf.fill_(0x33)
    assert check(device, [pts], o, fo)[1].tobytes() == rows.tobytes()  # a relaunch gives the same bytes
    assert check(device, [pts], o, fo, split=False)[1].tobytes() == rows.tobytes()  # one workgroup per cluster too


@pytest.mark.parametrize("layout", ["step32", "step16_mis1"])
def test_a_ragged_batch_sorted_and_shuffled_oversize_and_capped(device, layout):
    o, fo = grid(160, 64, min_points=1), K.FitOptions()
    sorted_pts = place(MANY[:40] + MANY[-6:], 5)
    shuffled = sorted_pts[np.random.default_rng(5).permutation(len(sorted_pts))]
    clouds = [sorted_pts, np.zeros((0, 3), F), shuffled, place(WIDE, 6), place([(1, 1, 257)], 6)]
    _, rows = check(device, clouds, o, fo, layout)
    assert rows[0].tobytes() == rows[2].tobytes() and rows[3]["flags"].tolist()[:2] == [1, 0]
    capped, pts = SHAPES["more_than_max_clusters"]  # found = 7 > max_clusters = 4
    _, rows = check(device, [pts, sorted_pts[:300]], capped, fo, layout)
    assert (rows[0]["score"] > 0).all() and (rows[1][4:]["score"] == 0).all()


def test_chained_behind_the_ground_split(device):
    pts, g, o = scene(), G.GroundOptions(), C.ClusterOptions(min_points=20)
    for layout in ("step16", "step20"):
        f, rows = check(device, [pts, pts[:3000], cloud_points(3, 257)], o, K.FitOptions(), layout, ground=g)
        assert f.cluster.n_stride == 2 and (rows[0][:3]["score"] > 0).all()


def test_launcher_refusals_leave_the_output_untouched(device):
    from triton_client_amd import _native

    o, fo = grid(65, 40), K.FitOptions()
    f, rows = check(device, [place([(3, 3, 9)]), place([(40, 30, 6)])], o, fo)
    c, p = f.cluster, _native.ptr
    f.fit.fill_(SENT)
    trig = f.trig.copy()
    trig[0, 0] = 16385
    base = dict(data=p(c.data), data_bytes=c.data_bytes, frame_off=p(c.frame_off), frame_n=p(c.frame_n), n_stride=1,
                batch=2, max_n=9, step=16, ox=0, oy=4, oz=8, label=p(c.label), table=p(c.out), found=p(c.found),
                max_k=1024, angles=90, d0q=1638, trig=f.trig.ctypes.data, split=1, plan=p(f.plan), grouped=p(f.grouped),
                slots=p(f.slots), slots_bytes=f.slots.numel(), work=p(f.work), work_bytes=f.work.numel(), fit=p(f.fit),
                stream=_native.stream_ptr())
    bad = [dict(data=0), dict(frame_off=0), dict(frame_n=0), dict(label=0), dict(table=0), dict(found=0), dict(trig=0),
           dict(plan=0), dict(grouped=0), dict(slots=0), dict(work=0), dict(fit=0), dict(plan=base["plan"] + 8),
           dict(grouped=base["grouped"] + 4), dict(slots=base["slots"] + 4), dict(work=base["work"] + 2),
           dict(fit=base["fit"] + 4), dict(label=base["label"] + 2), dict(table=base["table"] + 4),
           dict(frame_off=base["frame_off"] + 4), dict(batch=0), dict(batch=65), dict(max_k=0), dict(max_k=4097),
           dict(angles=1), dict(angles=129), dict(d0q=163), dict(d0q=16385), dict(trig=trig.ctypes.data), dict(split=2),
           dict(oz=16), dict(ox=-4), dict(step=0), dict(data_bytes=-1), dict(data_bytes=2 ** 31), dict(max_n=-1),
           dict(n_stride=0), dict(n_stride=3), dict(slots_bytes=32 * 2 * 90 - 1), dict(work_bytes=4 * 2 * 7 - 1)]
    fn = _native.kernels().tca_cluster_fit
    for kw in bad:
        assert fn(*{**base, **kw}.values()) == 1, kw  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (f.fit == SENT).all()  # nothing was launched
    assert fn(*base.values()) == 0
    torch.cuda.synchronize()
    assert f.fit[:f.fit_bytes].cpu().numpy().tobytes() == rows.tobytes()


def test_extractor_engine_and_driver_equal_the_host_path(cuda, monkeypatch):
    from test_ground import OPTS as GROUND
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.inference.engines import Detector3D
    from triton_client_amd.ros import rosmsg

    clouds, _ = _rig_messages()
    o, fo = C.ClusterOptions(min_points=3), K.FitOptions(angles=45)
    host = C.ClusterExtractor("cpu").extract(clouds, o, GROUND, fit=fo)
    assert all(h[0] >= 1 for h in host)
    ex = C.ClusterExtractor(cuda)
    for labels in (True, False):
        for got, want in zip(ex.extract(clouds, o, GROUND, labels=labels, fit=fo), host):
            assert got[0] == want[0] and got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == want[3].tobytes()
            assert np.array_equal(got[1], want[1]) if labels else got[1] is None
    assert "fit_out" in ex.ws._bufs  # the kernel ran
    wire = [rosmsg.serialize(K.fit_boxes(h[2], h[3], c.header, True, fo)) for c, h in zip(clouds, host)]
    engine = _GpuEngine()
    assert [rosmsg.serialize(m) for m in Detector3D.cluster_obstacles(engine, clouds, o, GROUND, fit=fo)] == wire
    assert "fit_out" in engine._cluster_extractor.ws._bufs
    drv = RosInference3D(engine=_GpuEngine(), params={}, clusters_topic="/c", cluster_options=o, ground_options=GROUND,
                         cluster_fit={"angles": 45})
    assert [rosmsg.serialize(r.clusters) for r in drv.process(clouds)] == wire
    assert "fit_out" in drv.engine._cluster_extractor.ws._bufs
    off = RosInference3D(engine=_GpuEngine(), params={}, clusters_topic="/c", cluster_options=o, ground_options=GROUND)
    assert [rosmsg.serialize(r.clusters) for r in off.process(clouds)] == \
        [rosmsg.serialize(C.cluster_boxes(h[2], c.header)) for c, h in zip(clouds, host)]  # option off: today's message
    assert "fit_out" not in off.engine._cluster_extractor.ws._bufs
    monkeypatch.setenv("TCA_DEVICE_CLUSTER_FIT", "0")
    other = _GpuEngine()
    assert [rosmsg.serialize(m) for m in Detector3D.cluster_obstacles(other, clouds, o, GROUND, fit=fo)] == wire
    assert other._cluster_extractor.gpu and "fit_out" not in other._cluster_extractor.ws._bufs  # the definition's fit
