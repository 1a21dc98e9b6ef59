"""``tca_track2d`` against the float32 definition of ops/track2d.py, bit for bit: the outputs
and the whole state, ``next_id`` and ``overflow`` included, in every test.  Raw launches go
through ``_native.call`` with the rows, the state and the outputs between sentinel guards (the
structure of tests/test_track3d_gpu.py); the crafted cases are those of tests/test_track2d.py
and the random scenes those of tests/track2d_scenes.py, whose reference is computed once."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import track2d_scenes as S
from test_decode_kernels_gpu import GUARD, I32_SENT, Buf, _call
from test_track2d import CASES, CUTS, _drive, _Engine, _frame
from triton_client_amd.ops import track2d as T

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = dict(max_age=S.MAX_AGE, min_iou=0.2, min_iou_low=0.5, alpha=0.5, beta=0.5)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


class Launch:
    """One guarded launch of a batch against a state (``TrackState2D``; left as it was)."""

    def __init__(self, dev, batch, state, rows_off=0, **kw):
        p = {**PARAMS, **kw}
        self.batch, self.cap = batch, state.capacity
        nd, nf = len(batch.rows), len(batch.dt)
        self.rows = Buf(dev, 8 * nd + 4, "i32")  # (+ 16 bytes: the refusal test moves the table by 4)
        raw = np.full(32 * nd + 16, 0, np.uint8)
        raw[rows_off:rows_off + 32 * nd] = batch.rows.view(np.uint8).reshape(-1)
        self.rows_words = torch.from_numpy(raw.view(np.int32).copy()).to(dev)
        self.rows.t[GUARD:GUARD + self.rows.n] = self.rows_words
        self.keep = []

        def up(a, dt):
            t = torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1).copy()).to(dev)
            self.keep.append(t)
            return t.data_ptr()

        self.state = Buf(dev, len(state.words()), "i32", fill=torch.from_numpy(state.words()).to(dev))
        self.out = Buf(dev, 4 * nd, "i32")
        assert self.rows.ptr % 16 == 0 and self.out.ptr % 16 == 0 and self.state.ptr % 4 == 0
        self.off = np.array(batch.det_off, np.int32)  # (a copy: the refusal test changes it)
        self.args = [self.rows.ptr + rows_off, self.off.ctypes.data, nf, up(np.r_[batch.dt, F(0)], F),
                     up(np.r_[batch.reset, np.uint8(0)], np.uint8), self.state.ptr, self.cap, int(p["max_age"]),
                     float(F(p["min_iou"])), float(F(p["min_iou_low"])), float(F(p["alpha"])), float(F(p["beta"])),
                     self.out.ptr]

    def call(self):
        try:
            _call("tca_track2d", *self.args)
        finally:
            torch.cuda.synchronize()

    def read(self):
        """→ (per frame (ids, hits, vel) in row order, TrackState2D); asserts the guards of the
        rows, the outputs and the state, and that the rows were not written."""
        assert (self.rows.bits() == self.rows_words.cpu().numpy()).all()
        w = self.out.bits().reshape(-1, 4)
        out = []
        for f in range(len(self.batch.dt)):
            r = w[self.batch.det_off[f]:self.batch.det_off[f + 1]]
            out.append((r[:, 0].copy(), r[:, 1].copy(), r[:, 2:4].copy().view(F)))
        return out, T.TrackState2D.from_words(self.state.bits(), self.cap)


def _same_state(got, want):
    assert got.same(want), [n for n, _ in T.FIELDS if (getattr(got, n).view(np.int32)
                                                       != getattr(want, n).view(np.int32)).any()]


def _against_definition(dev, dets, stamps, state, **kw):
    """One guarded launch of the frames against ``state`` and the definition on a copy of it."""
    p = {**PARAMS, **kw}
    batch = T.track_table(dets, stamps)
    la = Launch(dev, batch, state, **kw)
    la.call()
    got, got_state = la.read()
    st = state.copy()
    want = T.track_numpy(st, batch, p["min_iou"], p["min_iou_low"], p["max_age"], p["alpha"], p["beta"])
    S.same_results(got, want)
    _same_state(got_state, st)
    return want, st


@pytest.mark.parametrize("calls", S.CALLS)
@pytest.mark.parametrize("capacity", S.CAPACITIES)
def test_random_scenes(dev, capacity, calls):
    dets, stamps = S.random_scene(capacity)
    want, want_state, _ = S.reference(capacity)
    assert len(dets) == S.FRAMES == 65 > T.MAX_FRAMES  # in one call: two launches
    tr = T.Tracker2D(capacity=capacity, max_age=S.MAX_AGE, device=dev)
    assert tr.gpu and tr.kind == "tca_track2d"
    S.same_results(S.run_cut(tr, dets, stamps, calls), want)
    _same_state(tr.state(), want_state)
    assert tr.frames == 65 and want_state.next_id > 1


def test_random_scene_between_guards(dev):
    """33 frames of a scene in one guarded launch against a state that is not empty."""
    dets, stamps = S.random_scene(64)
    st0 = T.TrackState2D(64)
    T.track_numpy(st0, T.track_table(dets[:8], stamps[:8]), max_age=S.MAX_AGE)
    assert (st0.id != 0).sum() > 10
    batch = T.track_table(dets[8:41], stamps[8:41], prev_ns=stamps[7])
    la = Launch(dev, batch, st0)
    la.call()
    got, got_state = la.read()
    st, ev = st0.copy(), {}
    S.same_results(got, T.track_numpy(st, batch, max_age=S.MAX_AGE, events=ev))
    _same_state(got_state, st)
    assert all(ev.get(k, 0) > 0 for k in ("high_match", "low_match", "birth", "death", "reset", "tie")), ev


@pytest.mark.parametrize("n,capacity", [(0, 64), (1, 64), (130, 64), (512, 64), (512, 512), (130, 1)])
def test_frame_shapes(dev, n, capacity):
    """Frames of n detections (twice, so that the second matches); 130 at capacity 64: the births
    loop goes round more than once, 512 at 512: every slot and every row."""
    k = np.arange(n)
    d = np.zeros((n, 6), F)
    d[:, 0], d[:, 1] = 40.0 * (k % 25), 40.0 * (k // 25)
    d[:, 2], d[:, 3] = d[:, 0] + 30, d[:, 1] + 30
    d[:, 4], d[:, 5] = 0.25 + (k * 7 % 48) / 64.0, k % 3
    d2 = d.copy()
    d2[:, :4] += 2.25
    st0 = T.TrackState2D(capacity)
    want, st = _against_definition(dev, [d, d2[::-1]], [0, 33 * S.MS], st0, max_age=30)
    born = int((d[:, 4] >= F(0.6)).sum())
    assert st.next_id == min(born, capacity) + 1 and st.overflow == 2 * max(0, born - capacity)
    assert n == 0 or capacity == 1 or (want[1][0] > 0).sum() == min(born, capacity)


class Both:
    """A device tracker and the definition side by side: every call is compared bit for bit."""

    def __init__(self, dev, **kw):
        self.d, self.h = T.Tracker2D(device=dev, **kw), T.Tracker2D(device="cpu", **kw)
        assert self.d.gpu and self.d.kind == "tca_track2d" and not self.h.gpu

    def track(self, dets, stamps):
        got, want = self.d.track(dets, stamps), self.h.track(dets, stamps)
        S.same_results(got, want)
        self.state()
        return got

    def state(self):
        got, want = self.d.state(), self.h.state()
        _same_state(got, want)
        return got


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__[5:])
def test_crafted_cases_through_the_kernel(dev, case):
    case(lambda **kw: Both(dev, **kw))


def test_cut_invariance_on_the_device(dev):
    dets, stamps = S.scene(7, [int(n) for n in np.random.default_rng(7).integers(10, 50, 40)], n_obj=40)
    host = T.Tracker2D(capacity=32, max_age=2)
    want = host.track(dets, stamps)
    for cut in CUTS:
        tr = T.Tracker2D(capacity=32, max_age=2, device=dev)
        S.same_results(S.run_cut(tr, dets, stamps, cut), want)
        _same_state(tr.state(), host.state())
    assert host.state().overflow > 0


def test_graph_replay(dev):
    dets, stamps = S.random_scene(65)
    st0 = T.TrackState2D(65)
    T.track_numpy(st0, T.track_table(dets[:6], stamps[:6]), max_age=S.MAX_AGE)  # a state that is not empty
    batch = T.track_table(dets[6:18], stamps[6:18], prev_ns=stamps[5])
    la = Launch(dev, batch, st0)
    la.call()  # warm-up outside the capture, and the eager result
    first = la.read()
    want_state = st0.copy()
    want = T.track_numpy(want_state, batch, max_age=S.MAX_AGE)
    S.same_results(first[0], want)
    _same_state(first[1], want_state)
    words = torch.from_numpy(st0.words()).to(dev)
    body = la.state.t[GUARD:GUARD + len(words)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        T.launch(la.args[0], la.off, *la.args[2:])
    for _ in range(2):
        body.copy_(words)  # restore the state
        la.out.t[GUARD:GUARD + la.out.n] = I32_SENT
        g.replay()
        torch.cuda.synchronize()
        got = la.read()
        S.same_results(got[0], first[0])
        _same_state(got[1], first[1])


def test_refusals(dev):
    from triton_client_amd._native import NativeError

    dets, stamps = S.scene(3, [5, 7])
    batch = T.track_table(dets, stamps)

    def refused(la):
        with pytest.raises(NativeError):
            la.call()
        assert (la.out.bits() == I32_SENT).all() and (la.state.bits() == T.TrackState2D(la.cap).words()).all()

    def launch(**kw):
        return Launch(dev, batch, T.TrackState2D(8), **kw)

    for cap in (0, 513, -1):
        la = launch()
        la.args[6] = cap
        refused(la)
    for nf in (-1, 65):
        la = launch()
        la.args[2] = nf
        refused(la)
    # 513 detections in a frame; a decreasing offset; a first offset that is not 0
    for off in ([0, T.MAX_DETS + 1, T.MAX_DETS + 2], [0, 7, 5], [1, 5, 12]):
        la = launch()
        la.off[:] = off
        refused(la)
    refused(launch(rows_off=4))  # the table off 16-byte alignment
    la = launch()
    la.args[12] += 4  # out off 16-byte alignment
    refused(la)
    for null in (0, 1, 3, 4, 5, 12):  # rows, det_off, dt, reset, state, out
        la = launch()
        la.args[null] = 0
        refused(la)
    la = launch()
    la.args[7] = -1  # max_age
    refused(la)
    la = launch()  # and the same arguments unchanged are taken
    la.call()
    got, st = la.read()
    assert st.next_id > 1 and sum((g[0] > 0).sum() for g in got) == st.next_id - 1
    la = launch()  # no frames: nothing is launched, nothing written, no error
    la.args[2] = 0
    la.call()
    assert (la.out.bits() == I32_SENT).all() and (la.state.bits() == T.TrackState2D(8).words()).all()


def test_engine_and_driver_track_alike_on_the_device_and_the_host(dev, monkeypatch):
    from triton_client_amd.inference.engines import Detector2D

    class GpuEngine(_Engine, Detector2D):  # the stub detector with a device: its tracker is the kernel
        device = dev

    frames = [_frame(s) for s in range(1, 17)]
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("TCA_DEVICE_TRACK", mode)
        eng = GpuEngine()
        tr = eng.tracker(max_age=5)
        assert tr.gpu == (mode == "1") and eng.tracker() is tr and tr.kind == ("tca_track2d" if tr.gpu else
                                                                                "host definition")
        dets = eng.detect([np.asarray(_img(m)) for m in frames])
        res = tr.track(dets, [m.header.stamp for m in frames])
        monkeypatch.setattr(sys.modules[_drive.__module__], "_Engine", GpuEngine)
        pics, det_msgs, trk, seen, drv = _drive(frames, True, batch=4, workers=2)
        assert drv.tracker().gpu == (mode == "1") and drv.tracker().frames == 16
        runs[mode] = (res, tr.state(), trk, drv.tracker().state(), pics, det_msgs)
    S.same_results(runs["1"][0], runs["0"][0])
    _same_state(runs["1"][1], runs["0"][1])
    _same_state(runs["1"][3], runs["0"][3])
    _same_state(runs["1"][3], runs["1"][1])  # the driver's tracker saw what the direct call saw
    assert runs["1"][2] == runs["0"][2] and [s for s, _ in runs["1"][2]] == list(range(1, 17))
    assert runs["1"][4] == runs["0"][4] and runs["1"][5] == runs["0"][5]
    assert runs["1"][1].next_id == 4 and max(r[1].max() for r in runs["1"][0]) >= 12  # three objects, followed


def _img(m):
    from triton_client_amd.inference.ros_inference import decode_image_msg
    return decode_image_msg(m)


def test_driver_bench_reports_the_device_tracker(dev):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "driver_bench.py"), "--camera", "16", "--lidar", "0",
                        "--batch", "4", "--workers", "2", "--camera-tracks", "--timeout", "120"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["camera"]["tracker"] == "tca_track2d" and out["camera"]["complete"]
    assert out["camera"]["tracks"]["frames"] == 16 + 8 and "tracks (tca_track2d)" in out["camera"]["output"]
