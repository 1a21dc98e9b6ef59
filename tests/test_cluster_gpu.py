"""K31 on the device: ``tca_cluster`` gives, bit for bit, ``found``, the labels and the table of the definition of
ops/cluster.py (and of the float64 flood fill where no point is banded), and never sets ``err``."""
import dataclasses

import numpy as np
import pytest
import torch

from test_cluster import SHAPES, F, grid, place, refs, same  # noqa: F401  (refs: the shared fixture)
from test_ground_gpu import cloud_points
from test_laser_scan_gpu import _GpuEngine, payload
from test_range2d import _rig_messages
from triton_client_amd.ops import cluster as C
from triton_client_amd.ops import ground as G
from triton_client_amd.ops.cloud_common import CloudLayout

pytestmark = pytest.mark.gpu

SENT = 0x5A  # what the output buffer holds before a launch
LAYOUTS = {  # name: (layout, bytes the payload starts past a 16-byte boundary): the three load paths
    "step16": (CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7)), 0), "step20": (CloudLayout(20, (0, 4, 8, -1), (7, 7, 7, 7)), 0),
    "step32": (CloudLayout(32, (4, 12, 20, 28), (7, 7, 7, 7)), 0), "step16_mis1": (CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7)), 1)}


class Device:
    """One extractor for the module: every test launches on the same workspace."""

    def __init__(self, dev):
        self.ex = C.ClusterExtractor(dev)

    def run(self, clouds, opts, layout="step16", aggregate=True, ground=None, call=None):
        """One launch → ``(per cloud (found, label, table), the call)``; ``err`` is asserted to be zero."""
        lay, mis = LAYOUTS[layout]
        call = call or self.ex.prepare([payload(p, lay) for p in clouds], [len(p) for p in clouds], lay, opts, ground,
                                       misalign=mis)
        call.out.fill_(SENT)
        C.launch(call, aggregate=aggregate)
        torch.cuda.synchronize()
        assert call.err.item() == 0
        ns = call.ground.counts.cpu()[:, 0].tolist() if call.ground is not None else call.ns
        return C.results_of(call.out[:call.out_bytes].cpu().numpy(), call, ns, True), call


@pytest.fixture(scope="module")
def device(cuda):
    return Device(cuda)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bit_for_bit_the_definition_and_the_flood_fill(device, refs, name):
    o, pts = SHAPES[name]
    want = C.cluster_numpy(pts, o)
    for aggregate in (True, False):  # one set of atomics per point gives the same bytes
        (got,), call = device.run([pts], o, aggregate=aggregate)
        same(got, want)
        same(got, refs[name][:3])
    for buf in (call.cnt, call.lab, call.pcell, call.blocks):  # garbage in the workspace: a launch owns what it reads
        buf.fill_(0x33)
    same(device.run([pts], o, call=call)[0][0], want)  # a relaunch gives the same bytes


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_a_ragged_batch_in_every_layout_sorted_and_shuffled(device, layout):
    o = grid(65, 40, min_points=3)
    cells = [(x, y, 100) for x, y in ((3, 3), (31, 31), (32, 32), (60, 20))]  # runs of 100 cross the waves' borders
    sorted_pts = place(cells, 5)
    shuffled = sorted_pts[np.random.default_rng(5).permutation(len(sorted_pts))]
    clouds = [sorted_pts, np.zeros((0, 3), F), shuffled, place([(1, 1, 257)], 6)]
    want = [C.cluster_numpy(p, o) for p in clouds]
    assert [w[0] for w in want] == [3, 0, 3, 1] and want[0][2].tobytes() == want[2][2].tobytes()
    got, call = device.run(clouds, o, layout)
    for g, w in zip(got, want):
        same(g, w)
    host = call.out[:call.out_bytes].cpu().numpy()  # rows beyond found stay empty, the pad zero
    rows = host[:call.table_bytes].view(C.TABLE_DTYPE).reshape(4, o.max_clusters)
    assert (rows[1]["n"] == 0).all() and (rows[0][3:]["min_x"] == 2 ** 31 - 1).all() and not rows["pad"].any()


def scene():
    """A ground ring around the sensor 1.8 m up and three objects standing on it."""
    rng = np.random.default_rng(8)
    a, r = rng.uniform(-np.pi, np.pi, 6000), rng.uniform(2.0, 30.0, 6000)
    ring = np.stack([r * np.cos(a), r * np.sin(a), rng.normal(-1.8, 0.01, 6000)], 1)
    objs = [np.stack([rng.uniform(cx - 0.6, cx + 0.6, 300), rng.uniform(cy - 0.4, cy + 0.4, 300),
                      rng.uniform(-1.4, -0.2, 300)], 1) for cx, cy in ((10.3, 0.2), (-0.1, -8.1), (-12.2, 5.3))]
    pts = np.concatenate([ring, *objs]).astype(F)
    return pts[rng.permutation(len(pts))]


def test_chained_behind_the_ground_split(device):
    pts, g, o = scene(), G.GroundOptions(), C.ClusterOptions(min_points=20)
    clouds = [pts, pts[:3000], cloud_points(3, 257)]
    want = [C.cluster_numpy(C.obstacle_rows(p, g), o) for p in clouds]
    assert want[0][0] == 3 and want[0][2]["n"].min() > 250  # the objects, but for the few points their cells' ground took
    for layout in ("step16", "step20"):
        got, call = device.run(clouds, o, layout, ground=g)
        assert call.n_stride == 2 and call.data.data_ptr() == call.ground.out.data_ptr()
        for got_b, want_b in zip(got, want):
            same(got_b, want_b)


def test_launcher_refusals_leave_the_outputs_untouched(device):
    from triton_client_amd import _native

    o = grid(65, 40)
    clouds = [place([(3, 3, 9)]), place([(40, 30, 6)])]
    want = [C.cluster_numpy(p, o) for p in clouds]
    _, call = device.run(clouds, o)
    call.out.fill_(SENT)
    p, nan = _native.ptr, float("nan")
    base = dict(data=p(call.data), data_bytes=call.data_bytes, frame_off=p(call.frame_off), frame_n=p(call.frame_n),
                n_stride=1, batch=2, max_n=9, step=16, ox=0, oy=4, oz=8, x0=0.0, y0=0.0, cell=0.5, W=65, H=40, z0=-512.0,
                z1=512.0, min_cell=1, min_pts=5, max_pts=2 ** 31 - 1, max_k=1024, aggregate=1, cnt=p(call.cnt),
                lab=p(call.lab), pcell=p(call.pcell), blocks=p(call.blocks), label=p(call.label), table=p(call.out),
                found=p(call.found), err=p(call.err), stream=_native.stream_ptr())
    bad = [dict(data=0), dict(frame_off=0), dict(frame_n=0), dict(cnt=0), dict(lab=0), dict(pcell=0), dict(blocks=0),
           dict(label=0), dict(table=0), dict(found=0), dict(err=0), dict(cnt=base["cnt"] + 2), dict(lab=base["lab"] + 1),
           dict(table=base["table"] + 4), dict(label=base["label"] + 2), dict(frame_off=base["frame_off"] + 4),
           dict(batch=0), dict(batch=65), dict(W=0), dict(W=2049), dict(H=0), dict(H=2049), dict(W=2048, H=2048, batch=5),
           dict(max_k=0), dict(max_k=4097), dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(cell=float("inf")),
           dict(x0=nan), dict(z0=nan), dict(z0=1.0, z1=0.0), dict(oz=16), dict(ox=-4), dict(step=0), dict(data_bytes=-1),
           dict(data_bytes=2 ** 31), dict(max_n=-1), dict(n_stride=0), dict(n_stride=3), dict(aggregate=2),
           dict(min_cell=0), dict(min_pts=0), dict(max_pts=4)]
    fn = _native.kernels().tca_cluster
    for kw in bad:
        assert fn(*{**base, **kw}.values()) == 1, kw  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (call.out == SENT).all()  # nothing was launched
    assert fn(*base.values()) == 0
    torch.cuda.synchronize()
    for got, w in zip(C.results_of(call.out[:call.out_bytes].cpu().numpy(), call, call.ns, True), want):
        same(got, w)


def test_extractor_engine_and_driver_equal_the_host_path(cuda, monkeypatch):
    from test_ground import OPTS as GROUND
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.inference.engines import Detector3D
    from triton_client_amd.ros import rosmsg

    clouds, _ = _rig_messages()
    o = C.ClusterOptions(min_points=3)
    ex = C.ClusterExtractor(cuda)
    for opts in (o, dataclasses.replace(o, remove_ground=False)):
        want = [C.cluster_cloud_numpy(c, opts, GROUND) for c in clouds]
        assert all(w[0] >= 1 for w in want)
        for got, w in zip(ex.extract(clouds, opts, GROUND), want):
            same(got, w)
    assert ex._stream is not None and ex.extract([], o) == []  # the kernel ran
    wire = [rosmsg.serialize(C.cluster_boxes(w[2], c.header)) for c, w in zip(clouds, [C.cluster_cloud_numpy(c, o, GROUND)
                                                                                       for c in clouds])]
    drv = RosInference3D(engine=_GpuEngine(), params={}, clusters_topic="/c", cluster_options=o, ground_options=GROUND)
    assert [rosmsg.serialize(r.clusters) for r in drv.process(clouds)] == wire
    assert drv.engine._cluster_extractor.gpu and drv.engine._cluster_extractor._stream is not None
    monkeypatch.setenv("TCA_DEVICE_CLUSTER", "0")
    other = _GpuEngine()
    assert [rosmsg.serialize(m) for m in Detector3D.cluster_obstacles(other, clouds, o, GROUND)] == wire
    assert other._cluster_extractor.gpu and other._cluster_extractor._stream is None  # the definition, on a GPU engine too
