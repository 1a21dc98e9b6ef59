"""``tca_track3d`` against the float32 definition of ops/track3d.py, bit for bit: the outputs
and the whole state, ``next_id`` and ``overflow`` included.  Raw launches go through
``_native.call`` with the state and the outputs between sentinel guards (the structure of
tests/test_points_in_boxes_gpu.py); the crafted cases are those of tests/test_track3d.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_decode_kernels_gpu import I32_SENT, Buf, _call
from test_track3d import CASES, CUTS, run_cut, same_results, scene
from triton_client_amd.ops import track3d as T
from triton_client_amd.ros import compat, msgs

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


class Launch:
    """One guarded launch of a batch against a state (``TrackState``; left as it was)."""

    def __init__(self, dev, batch, state, gate2, max_age=3, alpha=0.5, rows_off=0):
        self.batch, self.cap = batch, state.capacity
        nd, nf = len(batch.rows), len(batch.dt)
        raw = np.zeros(32 * max(nd, 1) + 16, np.uint8)
        raw[rows_off:rows_off + 32 * nd] = batch.rows.view(np.uint8).reshape(-1)
        self.keep = [torch.from_numpy(raw).to(dev)]
        assert self.keep[0].data_ptr() % 16 == 0

        def up(a, dt):
            t = torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1).copy()).to(dev)
            self.keep.append(t)
            return t.data_ptr()

        self.state = Buf(dev, len(state.words()), "i32", fill=torch.from_numpy(state.words()).to(dev))
        self.out = Buf(dev, 4 * nd, "i32")
        assert self.out.ptr % 16 == 0 and self.state.ptr % 4 == 0
        self.off = np.array(batch.det_off, np.int32)  # (a copy: the refusal test changes it)
        self.args = [self.keep[0].data_ptr() + rows_off, self.off.ctypes.data, nf,
                     up(np.r_[batch.dt, F(0)], F), up(np.r_[batch.reset, np.uint8(0)], np.uint8), up(gate2, F),
                     len(gate2), self.state.ptr, self.cap, max_age, float(alpha), self.out.ptr]

    def call(self):
        try:
            _call("tca_track3d", *self.args)
        finally:
            torch.cuda.synchronize()

    def read(self):
        """→ (per frame (ids, hits, vel), TrackState); asserts the guards."""
        w = self.out.bits().reshape(-1, 4)
        out = []
        for f in range(len(self.batch.dt)):
            r = w[self.batch.det_off[f]:self.batch.det_off[f + 1]]
            out.append((r[:, 0].copy(), r[:, 1].copy(), r[:, 2:4].copy().view(F)))
        return out, T.TrackState.from_words(self.state.bits(), self.cap)


def _against_definition(dev, preds, stamps, capacity, max_age=1, gate2=None):
    gate2 = T.gate_table(2.0, ["a", "b", "c"], 1) if gate2 is None else gate2
    batch = T.track_table(preds, None, stamps)
    st = T.TrackState(capacity)
    la = Launch(dev, batch, st, gate2, max_age)
    la.call()
    got, got_state = la.read()
    want = T.track_numpy(st, batch, gate2, max_age, 0.5)
    same_results(got, want)
    assert got_state.same(st), [n for n, _ in T.FIELDS if (getattr(got_state, n).view(np.int32)
                                                           != getattr(st, n).view(np.int32)).any()]
    return want, st


COUNTS = [64, 130, 0, 1, 63, 65, 130, 64]  # one wave, two waves, and their edges


@pytest.mark.parametrize("nine", [False, True], ids=["7d", "9d"])
@pytest.mark.parametrize("capacity", [1, 64, 65, 256])
def test_random_scenes(dev, capacity, nine):
    preds, stamps = scene(capacity + nine, COUNTS, nine)
    assert 0 in np.diff(stamps)[1:]  # a dt of 0 among them
    want, st = _against_definition(dev, preds, stamps, capacity)
    ids = np.concatenate([w[0] for w in want])
    assert st.next_id > capacity + 1 and (st.id != 0).any()  # slots were reused
    assert (st.overflow > 0) == (capacity < 256)
    assert capacity == 1 or max(w[1].max() for w in want if len(w[1])) >= 3  # tracks continue
    assert capacity < 256 or (ids > 0).all()


@pytest.mark.parametrize("frames", [1, 33])
def test_batch_sizes(dev, frames):
    r = np.random.default_rng(frames)
    preds, stamps = scene(frames, [int(n) for n in r.integers(0, 40, frames)], n_obj=30)
    want, st = _against_definition(dev, preds, stamps, 64, max_age=2)
    assert frames == 1 or max(w[1].max() for w in want if len(w[1])) >= 4


class Both:
    """A device tracker and the definition side by side: every call is compared bit for bit."""

    def __init__(self, dev, **kw):
        gate2 = kw.pop("gate2", None)
        self.d, self.h = T.Tracker3D(device=dev, **kw), T.Tracker3D(device="cpu", **kw)
        assert self.d.gpu and self.d.kind == "tca_track3d" and not self.h.gpu
        if gate2 is not None:
            self.d.max_dist2[:] = gate2
            self.h.max_dist2[:] = gate2

    def track(self, preds, idx, stamps):
        got, want = self.d.track(preds, idx, stamps), self.h.track(preds, idx, stamps)
        same_results(got, want)
        self.state()
        return got

    def state(self):
        got, want = self.d.state(), self.h.state()
        assert got.same(want)
        return got


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__[5:])
def test_crafted_cases_through_the_kernel(dev, case):
    case(lambda **kw: Both(dev, **kw))


def test_cut_invariance_on_the_device(dev):
    preds, stamps = scene(5, [40, 37, 0, 45, 41, 1, 39, 44], False, n_obj=50)
    host = T.Tracker3D(capacity=48, max_age=1)
    want = host.track(preds, None, stamps)
    for cut in CUTS:
        tr = T.Tracker3D(capacity=48, max_age=1, device=dev)
        same_results(run_cut(tr, preds, stamps, cut), want)
        assert tr.state().same(host.state())
    assert host.state().overflow > 0


def test_graph_replay(dev):
    preds, stamps = scene(9, [30, 28, 31, 29], True, n_obj=40)
    gate2 = T.gate_table(2.0, ["a", "b", "c"], 1)
    batch = T.track_table(preds, None, stamps)
    st0 = T.TrackState(32)
    p0, s0 = scene(10, [20], True, n_obj=40)
    T.track_numpy(st0, T.track_table(p0, None, s0), gate2, 1)  # a state that is not empty
    la = Launch(dev, batch, st0, gate2, 1)
    la.call()  # warm-up outside the capture
    first = la.read()
    want_state = st0.copy()
    want = T.track_numpy(want_state, batch, gate2, 1, 0.5)
    same_results(first[0], want)
    assert first[1].same(want_state)
    words = torch.from_numpy(st0.words()).to(dev)
    body = la.state.t[64:64 + len(words)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        T.launch(la.args[0], la.off, *la.args[2:])
    for _ in range(2):
        body.copy_(words)  # restore the state
        la.out.t[64:64 + la.out.n] = I32_SENT
        g.replay()
        torch.cuda.synchronize()
        got = la.read()
        same_results(got[0], want)
        assert got[1].same(want_state)


def test_refusals(dev):
    from triton_client_amd._native import NativeError

    preds, stamps = scene(3, [5, 7])
    gate2 = T.gate_table()
    batch = T.track_table(preds, None, stamps)

    def refused(la):
        with pytest.raises(NativeError):
            la.call()
        assert (la.out.bits() == I32_SENT).all() and (la.state.bits() == T.TrackState(la.cap).words()).all()

    for cap in (0, 1025):
        la = Launch(dev, batch, T.TrackState(8), gate2)
        la.args[8] = cap
        refused(la)
    for off in ([0, T.MAX_DETS + 1, T.MAX_DETS + 2], [0, 7, 5]):  # 513 detections in a frame; a decreasing offset
        la = Launch(dev, batch, T.TrackState(8), gate2)
        la.off[:] = off
        refused(la)
    refused(Launch(dev, batch, T.TrackState(8), gate2, rows_off=4))  # the table off 16-byte alignment
    la = Launch(dev, batch, T.TrackState(8), gate2)  # and the same arguments unchanged are taken
    la.call()
    assert (la.read()[0][0][0] > 0).all()


def _sweeps(n):
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep

    out = []
    for s in range(n):
        pts = np.frombuffer(lidar_sweep(LidarSpec(rings=16, azimuth_steps=128, sensor_height=1.8), s % 4).tobytes(),
                            F).reshape(-1, 4)
        out.append(compat.create_cloud_xyzi(pts, msgs.Header(seq=s + 1, stamp=msgs.Time(7, s * 10 ** 8), frame_id="os")))
    return out


def test_engine_and_driver_track_alike_on_the_device_and_the_host(dev, monkeypatch):
    from triton_client_amd.inference import LocalDetector3D, RosInference3D
    from triton_client_amd.ros import rosmsg
    from triton_client_amd.ros.bus import TopicBus

    eng = LocalDetector3D(device=dev)
    clouds = _sweeps(8)
    preds = eng.detect(clouds)
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("TCA_DEVICE_TRACK", mode)
        eng._tracker = None
        tr = eng.tracker(max_age=2)
        assert tr.gpu == (mode == "1") and eng.tracker() is tr
        res = tr.track(preds, None, [c.header.stamp for c in clouds])
        bus = TopicBus()
        got = []
        compat.Subscriber("/t", msgs.BoundingBoxArray, lambda m: got.append((m.header.seq, rosmsg.serialize(m))),
                          bus=bus)
        eng._tracker = None
        drv = RosInference3D(engine=eng, params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=4, workers=2,
                             queue_size=64, labels=None, score_thresh=0.0, tracks_topic="/t")
        drv.start_inference(spin=False)
        pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
        for c in clouds:
            pub.publish(c)
        drv.stop()
        bus.close()
        assert drv.tracker().gpu == (mode == "1") and drv.tracker().frames == 8
        runs[mode] = (res, tr.state(), got)
    same_results(runs["1"][0], runs["0"][0])
    assert runs["1"][1].same(runs["0"][1])
    assert runs["1"][2] == runs["0"][2] and [s for s, _ in runs["1"][2]] == list(range(1, 9))
    assert sum(len(r[0]) for r in runs["1"][0]) > 0 and runs["1"][1].next_id > 1  # something was tracked


def test_driver_bench_reports_the_device_tracker(dev):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "driver_bench.py"), "--camera", "0", "--lidar", "16",
                        "--batch", "4", "--workers", "2", "--tracks", "--timeout", "120"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["lidar"]["tracker"] == "tca_track3d" and out["lidar"]["complete"]
    assert out["lidar"]["tracks"]["frames"] == 16 + 8 and "tracks (tca_track3d)" in out["lidar"]["output"]
