"""The camera tracker's definition (ops/track2d.py) on crafted cases, its cut invariance, the
non-vacuity of the random scenes, the ordered stage of the 2D driver and the command-line flags.
Every crafted case takes a tracker factory, so tests/test_track2d_gpu.py runs the same cases
through ``tca_track2d``."""
import threading
import time

import numpy as np
import pytest

import track2d_scenes as S
from triton_client_amd.ops import track2d as T
from triton_client_amd.ros import compat, msgs

F = np.float32
MS = S.MS
DT = 125  # ms: exact in float32 seconds


def cpu(**kw):
    return T.Tracker2D(device="cpu", **kw)


def D(boxes, scores=0.9, labels=0):
    """Detections [n, 6] of ``boxes`` [n, 4] (x1, y1, x2, y2)."""
    b = np.asarray(boxes, F).reshape(-1, 4)
    d = np.zeros((len(b), 6), F)
    d[:, :4] = b
    d[:, 4] = np.broadcast_to(np.asarray(scores, F), (len(b),))
    d[:, 5] = np.broadcast_to(np.asarray(labels, F), (len(b),))
    return d


def box(cx, cy, w=40.0, h=40.0):
    return (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)


def one(tr, dets, t_ms):
    """One frame → (ids, hits, vel) as lists / array."""
    i, h, v = tr.track([dets], [int(t_ms) * MS])[0]
    return i.tolist(), h.tolist(), v


def ids_of(tr, dets, t_ms):
    return one(tr, dets, t_ms)[0]


def finite_state(st):
    return all(np.isfinite(getattr(st, n)).all() for n, dt in T.FIELDS if dt is F)


# ----------------------------------------------------------------------- crafted cases
def case_constant_velocity(mk):
    """2.5 px per 125 ms: 20 px/s exactly, from the second frame on; the prediction is the place."""
    tr = mk()
    for k in range(6):
        i, h, v = one(tr, D([box(100 + 2.5 * k, 200 - 5.0 * k, 40, 20)]), DT * k)
        assert i == [1] and h == [k + 1]
        assert v.tolist() == ([[0, 0]] if k == 0 else [[20, -40]])
    st = tr.state()
    assert st.next_id == 2 and st.hits[0] == 6 and st.age[0] == 0 and st.pt[0] == 0 and st.label[0] == 0
    assert (st.cx[0], st.cy[0], st.w[0], st.h[0], st.vx[0], st.vy[0]) == (112.5, 175.0, 40, 20, 20, -40)
    assert (st.px[0], st.py[0]) == (112.5, 175.0) and (st.id != 0).sum() == 1
    assert ids_of(tr, D(np.zeros((0, 4))), DT * 6) == []  # a miss: the slot is predicted on
    st = tr.state()
    assert (st.cx[0], st.cy[0], st.pt[0], st.age[0]) == (115.0, 170.0, 0.125, 1)
    assert one(tr, D([box(117.5, 165.0, 40, 20)]), DT * 7)[2].tolist() == [[20, -40]]  # vm over pt = 0.25 s


def case_crossing(mk):
    """Two boxes of one class cross, 10 px apart in y, 8 px per frame each: the velocities keep
    the identities.  The input order and which of the two scores higher change from frame to frame."""
    tr = mk()
    for k in range(13):
        a, b = box(100 + 8 * k, 100), box(196 - 8 * k, 110)
        sa, sb = (0.9, 0.8) if k % 3 else (0.8, 0.9)  # (frame 0: b scores higher and is born first)
        if k % 2:
            i, h, v = one(tr, D([b, a], [sb, sa]), DT * k)
            i, h, v = i[::-1], h[::-1], v[::-1]
        else:
            i, h, v = one(tr, D([a, b], [sa, sb]), DT * k)
        assert i == [2, 1] and h == [k + 1, k + 1], (k, i, h)
        assert v.tolist() == ([[0, 0], [0, 0]] if k == 0 else [[64, 0], [-64, 0]])
    st = tr.state()
    assert st.next_id == 3 and st.vx[:2].tolist() == [-64, 64] and st.hits[:2].tolist() == [13, 13]


def _q_of(det, trk):
    """The definition's q of a detection box and a track box, both (x1, y1, x2, y2), by hand."""
    x1, y1, x2, y2 = (F(v) for v in det)
    a1, b1, a2, b2 = (F(v) for v in trk)
    iw, ih = min(x2, a2) - max(x1, a1), min(y2, b2) - max(y1, b1)
    inter = F(max(iw, F(0)) * max(ih, F(0)))
    u = F(F(F(x2 - x1) * F(y2 - y1)) + F(F(a2 - a1) * F(b2 - b1))) - inter
    return F(inter / u)


def case_closed_gates(mk):
    t0, d1 = (0, 0, 40, 40), (10, 0, 50, 40)
    q = _q_of(d1, t0)
    assert q.dtype == F and q == F(1200) / F(2000)
    up = np.nextafter(q, F(1))
    # high tier: exactly on min_iou matches; one ulp above it does not, and the row is born
    tr = mk(min_iou=q)
    assert ids_of(tr, D([t0]), 0) == [1] and one(tr, D([d1]), 0)[:2] == ([1], [2])
    tr = mk(min_iou=up)
    assert ids_of(tr, D([t0]), 0) == [1] and one(tr, D([d1]), 0)[:2] == ([2], [1])
    # low tier: exactly on min_iou_low keeps the track; one ulp above it does not (and a low row is never born)
    tr = mk(min_iou_low=q)
    assert ids_of(tr, D([t0]), 0) == [1] and one(tr, D([d1], 0.3), 0)[:2] == ([1], [2])
    tr = mk(min_iou_low=up)
    assert ids_of(tr, D([t0]), 0) == [1] and one(tr, D([d1], 0.3), 0)[:2] == ([0], [0])
    st = tr.state()
    assert st.age[0] == 1 and st.next_id == 2 and st.overflow == 0


def case_ties(mk):
    tr = mk()
    assert ids_of(tr, D([(0, 0, 40, 40), (40, 0, 80, 40)]), 0) == [1, 2]
    assert _q_of((20, 0, 60, 40), (0, 0, 40, 40)).view(np.uint32) == _q_of((20, 0, 60, 40), (40, 0, 80, 40)).view(
        np.uint32)
    assert one(tr, D([(20, 0, 60, 40)]), DT)[:2] == ([1], [2])  # bit-equal IoU: the lower slot
    st = tr.state()
    assert st.hits[:2].tolist() == [2, 1] and st.age[:2].tolist() == [0, 1] and st.next_id == 3


def case_score_order(mk):
    tr = mk()
    assert ids_of(tr, D([(0, 0, 40, 40)]), 0) == [1]
    # the second detection scores higher and claims the track although the first is closer to it
    i, h, _ = one(tr, D([(2, 0, 42, 40), (10, 0, 50, 40)], [0.7, 0.9]), DT)
    assert i == [2, 1] and h == [1, 2]
    # equal scores: the caller's order decides
    tr = mk()
    assert ids_of(tr, D([(0, 0, 40, 40)]), 0) == [1]
    assert ids_of(tr, D([(10, 0, 50, 40), (2, 0, 42, 40)], [0.75, 0.75]), DT) == [1, 2]


def case_low_tier(mk):
    tr = mk()
    b = (100, 100, 140, 140)
    assert ids_of(tr, D([b]), 0) == [1]
    assert one(tr, D([b], 0.3), DT)[:2] == ([1], [2])          # matched in the last frame: a low row keeps it
    assert ids_of(tr, D(np.zeros((0, 4))), 2 * DT) == []       # a miss: age 1
    assert one(tr, D([b], 0.3), 3 * DT)[:2] == ([0], [0])      # a low row does not revive it
    st = tr.state()
    assert st.age[0] == 2 and st.hits[0] == 2 and st.next_id == 2
    assert one(tr, D([b], 0.9), 4 * DT)[:2] == ([1], [3])      # a high row does
    # a low row starts nothing, and is no overflow
    assert ids_of(tr, D([b, (500, 500, 540, 540)], [0.9, 0.45]), 5 * DT) == [1, 0]
    st = tr.state()
    assert st.next_id == 2 and st.overflow == 0 and (st.id != 0).sum() == 1


def case_birth_gate(mk):
    tr = mk()
    b = (100, 100, 140, 140)
    assert one(tr, D([b], 0.55), 0)[:2] == ([0], [0])  # high_score <= 0.55 < new_score: not born
    st = tr.state()
    assert (st.id == 0).all() and st.next_id == 1 and st.overflow == 0
    assert ids_of(tr, D([b], 0.6), DT) == [1]          # new_score itself: born
    assert ids_of(tr, D(np.zeros((0, 4))), 2 * DT) == []
    assert one(tr, D([b], 0.55), 3 * DT)[:2] == ([1], [2])  # and 0.55 matches a track with age > 0
    assert ids_of(mk(new_score=0.5), D([b], 0.5), 0) == [1]


def case_labels(mk):
    tr = mk()
    b = (100, 100, 140, 140)
    assert ids_of(tr, D([b], 0.9, 1), 0) == [1]
    assert ids_of(tr, D([b], 0.9, 2), DT) == [2]  # the same place, another class
    assert ids_of(tr, D([b, b], [0.9, 0.8], [2, 1]), 2 * DT) == [2, 1]
    assert tr.state().label[:2].tolist() == [1, 2]


def case_max_age(mk):
    b = (100, 100, 140, 140)
    for missed, want in ((2, 1), (3, 2)):
        tr = mk(max_age=2)
        assert ids_of(tr, D([b]), 0) == [1]
        for k in range(missed):
            assert ids_of(tr, D(np.zeros((0, 4))), DT * (k + 1)) == []
        assert ids_of(tr, D([b]), DT * (missed + 1)) == [want]
        st = tr.state()
        assert (st.id != 0).sum() == 1 and st.next_id == want + 1


def case_size_smoothing(mk):
    for beta, (w, h) in ((0.5, (44, 24)), (0.25, (42, 22))):
        tr = mk(beta=beta)
        assert ids_of(tr, D([box(100, 100, 40, 20)]), 0) == [1]
        assert ids_of(tr, D([box(100, 100, 48, 28)]), DT) == [1]
        st = tr.state()
        assert (st.w[0], st.h[0], st.cx[0], st.cy[0]) == (w, h, 100, 100)


def case_overflow(mk):
    tr = mk(capacity=1)
    two = D([(0, 0, 40, 40), (500, 500, 540, 540)], [0.9, 0.8])
    assert one(tr, two, 0)[:2] == ([1, 0], [1, 0])
    st = tr.state()
    assert st.overflow == 1 and st.next_id == 2
    i, h, v = one(tr, two[::-1], DT)
    assert i == [0, 1] and h == [0, 2] and (v == 0).all() and tr.state().overflow == 2


def case_resets_and_dt0(mk):
    tr = mk(max_gap=2.0)
    a, b = box(100, 100), box(300, 300)
    assert ids_of(tr, D([a, b], [0.9, 0.8]), 1000) == [1, 2]
    assert ids_of(tr, D([box(104, 100), box(300, 304)], [0.9, 0.8]), 1000) == [1, 2]  # dt == 0: matched, pt == 0
    st = tr.state()
    assert finite_state(st) and (st.vx == 0).all() and (st.vy == 0).all() and (st.pt == 0).all()
    assert st.hits[:2].tolist() == [2, 2]
    i, h, v = one(tr, D([box(108, 100), box(300, 308)], [0.9, 0.8]), 1000 + DT)
    half = F(0.5) * (F(4) / F(0.125))  # hits was 2: v = 0 + alpha*(vm - 0)
    assert i == [1, 2] and v.tolist() == [[half, 0], [0, half]] and finite_state(tr.state())
    assert ids_of(tr, D([box(108, 100)]), 900) == [3]  # the stamp goes back: reset, the ids go on
    st = tr.state()
    assert (st.id != 0).sum() == 1 and st.next_id == 4
    assert ids_of(tr, D([box(108, 100)]), 900 + 2001) == [4]         # a gap above max_gap: reset
    assert ids_of(tr, D([box(108, 100)]), 900 + 2001 + 2000) == [4]  # a gap of max_gap: none
    assert tr.state().hits[0] == 2


def case_invalid_rows(mk):
    a, b = mk(), mk()
    good = D([box(100, 100), box(300, 300)], [0.9, 0.8])
    for tr in (a, b):
        assert ids_of(tr, good, 0) == [1, 2]
    bad = D([(np.nan, 80, 120, 120), (80, 80, np.inf, 120), (120, 80, 80, 120), (80, 120, 120, 120), box(100, 100),
             box(300, 300)], [0.9, 0.9, 0.9, 0.9, np.nan, -np.inf])
    i, h, v = one(a, bad, DT)
    assert i == [0] * 6 and h == [0] * 6 and (v == 0).all()
    assert ids_of(b, D(np.zeros((0, 4))), DT) == []
    assert a.state().same(b.state()) and a.state().overflow == 0
    i, h, _ = one(a, np.concatenate([bad[:2], good]), 2 * DT)  # the valid rows among them are tracked
    assert i == [0, 0, 1, 2] and h == [0, 0, 2, 2]


def case_edge_frames(mk):
    tr = mk(capacity=512)
    assert ids_of(tr, D(np.zeros((0, 4))), 0) == []  # an empty first frame
    n = T.MAX_DETS + 8
    k = np.arange(n)
    boxes = np.stack([50.0 * (k % 26), 50.0 * (k // 26), 50.0 * (k % 26) + 40, 50.0 * (k // 26) + 40], 1)
    scores = 0.625 + (k % 5) / 64.0
    i, h, _ = one(tr, D(boxes, scores), DT)
    order = np.argsort(-scores.astype(F), kind="stable")
    want = np.zeros(n, np.int32)
    want[order[:T.MAX_DETS]] = np.arange(1, T.MAX_DETS + 1)  # ids in score order; the 8 lowest: none
    assert i == want.tolist() and (np.asarray(h) == (want > 0)).all()
    st = tr.state()
    assert st.next_id == T.MAX_DETS + 1 and st.overflow == 0 and (st.id != 0).all()
    i2, h2, _ = one(tr, D(boxes, scores), 2 * DT)
    assert i2 == i and (np.asarray(h2) == 2 * (want > 0)).all()


def case_unsorted_input(mk):
    """Outputs are aligned with the caller's order, whatever it is."""
    tr = mk()
    cs = [(100, 100), (300, 100), (500, 100), (100, 400), (300, 400)]
    sc = np.array([0.62, 0.9, 0.3, 0.75, 0.75], F)
    lb = np.array([0, 1, 0, 1, 2])
    i, h, _ = one(tr, D([box(*c) for c in cs], sc, lb), 0)
    assert i == [4, 1, 0, 2, 3] and h == [1, 1, 0, 1, 1]  # born in score order; 0.3 is not
    for k, perm in enumerate(([4, 3, 2, 1, 0], [2, 0, 4, 1, 3], [0, 1, 2, 3, 4]), 1):
        p = np.array(perm)
        d = D([box(cs[j][0] + 2.5 * k, cs[j][1]) for j in p], sc[p], lb[p])
        i, h, v = one(tr, d, DT * k)
        assert i == [[4, 1, 0, 2, 3][j] for j in p]
        assert h == [0 if j == 2 else k + 1 for j in p]
        assert v[:, 0].tolist() == [0 if j == 2 else 20 for j in p]


CASES = [case_constant_velocity, case_crossing, case_closed_gates, case_ties, case_score_order, case_low_tier,
         case_birth_gate, case_labels, case_max_age, case_size_smoothing, case_overflow, case_resets_and_dt0,
         case_invalid_rows, case_edge_frames, case_unsorted_input]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__[5:])
def test_crafted(case):
    case(cpu)


# ------------------------------------------------------------------------ random scenes
CUTS = (40, 1, 7)


def test_cut_invariance():
    dets, stamps = S.scene(7, [int(n) for n in np.random.default_rng(7).integers(10, 50, 40)], n_obj=40)
    runs = []
    for cut in CUTS:
        tr = cpu(capacity=32, max_age=2)
        runs.append((S.run_cut(tr, dets, stamps, cut), tr.state()))
    for out, st in runs[1:]:
        S.same_results(out, runs[0][0])
        assert st.same(runs[0][1])
    st = runs[0][1]
    ids = np.concatenate([o[0] for o in runs[0][0]])
    # the scene does what it is for: tracks continue, slots are reused, the capacity overflows
    assert st.overflow > 0 and st.next_id > 32 + 10 and (ids == 0).any() and (ids > 0).any()
    assert max(o[1].max() for o in runs[0][0] if len(o[1])) >= 5


def test_random_scenes_are_not_vacuous():
    """A condition on the inputs of tests/test_track2d_gpu.py: over its scenes the definition
    takes every path the kernel has."""
    total = {}
    for cap in S.CAPACITIES:
        res, st, ev = S.reference(cap)
        for k, v in ev.items():
            total[k] = total.get(k, 0) + v
        assert ev.get("high_match", 0) > 0 and ev.get("birth", 0) > 0 and ev.get("reset", 0) == 2
        assert (ev.get("overflow", 0) > 0) == (cap < 512) and ev.get("overflow", 0) == st.overflow
        assert ev.get("birth", 0) == st.next_id - 1
        dets, _ = S.random_scene(cap)
        assert [len(r[0]) for r in res] == [len(d) for d in dets] and {0, 1, 90} <= {len(d) for d in dets}
        if cap > 1:
            assert all(ev.get(k, 0) > 0 for k in T.EVENTS if k != "overflow"), ev
    assert all(total.get(k, 0) > 0 for k in T.EVENTS), total
    # exact ties among the scores too (the 1/64 grid): the stable order decides them
    dets, _ = S.random_scene(64)
    assert any(len(np.unique(d[:, 4])) < len(d) for d in dets)


def test_track_table_inputs():
    d = D([(0, 0, 10, 10), (0, 0, np.nan, 10), (5, 5, 9, 9), (1, 1, 3, 3), (2, 2, 2, 8), (0, 0, 4, 4)],
          [0.5, 0.9, 0.6, 0.6, 0.99, 0.25], [3, 1, 2, 7, 1, 0])
    b = T.track_table([d, D([(0, 0, 1, 1)])], [msgs.Time(5, 999_999_999), msgs.Time(6, 1)], prev_ns=None)
    assert b.det_off.tolist() == [0, 6, 7] and b.rows.dtype.itemsize == 32 and b.sent == [6, 1]
    assert b.order[0].tolist() == [2, 3, 0, 5, 1, 4]  # descending score, ties in input order, invalid last
    V, H, B = T.VALID, T.HIGH, T.BIRTH
    assert b.rows["flags"].tolist() == [V | H | B, V | H | B, V | H, V, 0, 0, V | H | B]
    assert b.rows["label"].tolist() == [2, 7, 3, 0, 1, 1, 0] and b.rows["x2"][:4].tolist() == [9, 3, 10, 4]
    assert b.dt.tolist() == [0, F(np.float64(2) * 1e-9)] and b.reset.tolist() == [0, 0] and b.dt.dtype == F
    b = T.track_table([D([(0, 0, 1, 1)])] * 3, [10 * MS, 5 * MS, 2006 * MS], prev_ns=0, max_gap=2.0)
    assert b.reset.tolist() == [0, 1, 1] and b.dt.tolist() == [F(0.01), 0, 0]
    # the comparisons with the score thresholds are float32 comparisons
    s = np.nextafter(F(0.5), F(0))
    assert T.detection_rows(D([(0, 0, 1, 1)] * 2, [s, 0.5]))[0]["flags"].tolist() == [V | H, V]
    assert T.detection_rows(D([(0, 0, 1, 1)], 0.1), high_score=0.1)[0]["flags"].tolist() == [V | H]  # F(0.1) >= F(0.1)
    for bad in (0, 513):
        with pytest.raises(ValueError):
            T.Tracker2D(capacity=bad)
    with pytest.raises(ValueError):
        T.Tracker2D(max_age=-1)
    st = T.TrackState2D(3)
    assert len(st.words()) == 4 + 13 * 3 and st.words()[:2].tolist() == [1, 0]
    assert T.TrackState2D.from_words(st.words(), 3).same(st)


# ------------------------------------------------------------------------------ driver
class _Engine:
    """A CPU engine by duck typing: three objects whose places follow the frame's number, which
    the frame carries in its first pixel (the second: a frame that must never be tracked)."""
    names = ["crop", "weed"]

    def detect(self, frames):
        out = []
        for img in frames:
            s = int(img[0, 0, 0])
            if img[0, 0, 1]:
                out.append(D([box(900, 900)], 0.9, 1))
                continue
            bs = [box(100 + 4.0 * s, 100), box(400 - 4.0 * s, 120), box(250, 300 + 2.0 * s)][: 3 - (s % 5 == 0)]
            sc = [0.9, 0.8, 0.7 if s % 4 else 0.3][: len(bs)]  # (a dropout; a dip into the low tier)
            d = D(bs, sc, [0, 0, 1][: len(bs)])
            out.append(d[::-1].copy() if s % 2 else d)
        return out


def _frame(seq, stale=False):
    img = np.zeros((8, 8, 3), np.uint8)
    img[0, 0, 0], img[0, 0, 1] = seq, int(stale)
    ns = seq * 10 ** 9 // 30
    return compat.numpy_to_imgmsg(img, "rgb8", header=msgs.Header(seq=seq, stamp=msgs.Time(10 + ns // 10 ** 9,
                                                                                             ns % 10 ** 9),
                                                                  frame_id="stale" if stale else "cam"))


def _drive(frames, tracks, batch=1, workers=1, slow=False):
    from triton_client_amd.inference import RosInference
    from triton_client_amd.ros import rosmsg
    from triton_client_amd.ros.bus import TopicBus

    bus = TopicBus()
    pics, dets, trk, seen = [], [], [], []
    compat.Subscriber("/o", msgs.Image, lambda m: pics.append(rosmsg.serialize(m)), bus=bus)
    compat.Subscriber("/o/detections", msgs.Detection2DArray, lambda m: dets.append(rosmsg.serialize(m)), bus=bus)
    compat.Subscriber("/t", msgs.Detection2DArray, lambda m: trk.append((m.header.seq, rosmsg.serialize(m))), bus=bus)
    drv = RosInference(engine=_Engine(), params={"sub_topic": "/cam", "pub_topic": "/o"}, bus=bus, batch=batch,
                       workers=workers, queue_size=64, tracks_topic="/t" if tracks else None,
                       track_options={"max_age": 5})
    if slow:  # the first ticket finishes last
        process, first = drv.process, threading.Event()

        def slow_process(ms):
            late = not first.is_set()
            first.set()
            r = process(ms)
            if late:
                time.sleep(0.15)
            return r
        drv.process = slow_process
    track = drv.track
    drv.track = lambda rs: (seen.extend((r[1].header.seq, r[1].header.frame_id) for r in rs), track(rs))[1]
    drv.start_inference(spin=False)
    pub = compat.Publisher("/cam", msgs.Image, bus=bus)
    for m in frames:
        pub.publish(m)
        if slow:
            time.sleep(0.002)  # (several tickets, not one)
    runner = drv.runner
    drv.stop()
    bus.close()
    assert runner is None or not runner.errors, runner.errors
    return pics, dets, trk, seen, drv


def test_driver_tracks_in_order_whatever_order_the_batches_finish_in():
    clean = [_frame(s) for s in range(1, 17)]
    pics1, dets1, trk1, seen1, drv1 = _drive(clean, True)
    assert len(pics1) == len(dets1) == len(trk1) == 16 and [s for s, _ in seen1] == list(range(1, 17))
    assert [s for s, _ in trk1] == list(range(1, 17)) and all(a != b for a, (_, b) in zip(dets1, trk1))
    # a stale frame (seq 5 again, after seq 9) is dropped by the re-publisher: the tracker never sees it
    dirty = clean[:9] + [_frame(5, stale=True)] + clean[9:]
    pics4, dets4, trk4, seen4, drv4 = _drive(dirty, True, batch=4, workers=3, slow=True)
    assert [s for s, _ in seen4] == list(range(1, 17)) and all(f == "cam" for _, f in seen4)
    assert trk4 == trk1 and dets4 == dets1 and pics4 == pics1
    assert drv4.tracker().state().same(drv1.tracker().state()) and drv4.tracker().frames == 16
    # frame and detections messages are the same bytes without the topic, and nothing is tracked
    for kw in ({}, {"batch": 4, "workers": 3}):
        pics0, dets0, trk0, seen0, drv0 = _drive(clean, False, **kw)
        assert pics0 == pics1 and dets0 == dets1 and trk0 == [] and seen0 == []
        assert not hasattr(drv0.engine, "_tracker")


def test_tracked_results_and_ids_over_the_run():
    from triton_client_amd.inference import RosInference

    drv = RosInference(engine=_Engine(), params={}, tracks_topic="/t")
    frames = [_frame(s) for s in range(1, 13)]
    res = drv.track(drv.process(frames))
    by_place = {}
    for m, r in zip(frames, res):
        assert len(r) == 5 and isinstance(r[3], msgs.Detection2DArray)
        ids, hits, vel = r[4]
        assert r[3].header.seq == m.header.seq and r[3].header.stamp == m.header.stamp
        assert len(ids) == len(hits) == len(vel) == len(r[2]) == len(r[3].detections) == len(r[1].detections)
        assert [d.results[0].id for d in r[3].detections] == ids.tolist()
        assert [d.results[0].id for d in r[1].detections] == r[2][:, 5].astype(int).tolist()
        for d0, d1 in zip(r[1].detections, r[3].detections):
            assert d0.bbox == d1.bbox and d0.results[0].score == d1.results[0].score
        for d, i in zip(r[2], ids):
            key = "a" if d[1] == 80 else "b" if d[1] == 100 else "c"
            by_place.setdefault(key, set()).add(int(i))
    assert sorted(map(sorted, by_place.values())) == [[1], [2], [3]]  # dropouts and the low dips included
    trk = drv.tracker()
    assert trk.kind == "host definition" and trk.frames == 12 and trk.max_age == 30 and trk.state().next_id == 4
    assert len(RosInference(engine=_Engine(), params={}).process(frames)[0]) == 3  # process() is as before


def test_flags_and_bag_driver(tmp_path):
    from triton_client_amd.cli import bag2d, main
    from triton_client_amd.cli.common import track2d_options
    from triton_client_amd.inference import BagInference2D
    from triton_client_amd.inference.engines import Detector2D
    from triton_client_amd.ros import Bag

    f = main.parse_args([])
    assert f.tracks_topic == "" and track2d_options(f) == {"max_age": 30, "high_score": 0.5, "min_iou": 0.2}
    f = main.parse_args(["--tracks-topic", "/t", "--track-max-age", "5", "--track-high-score", "0.4",
                         "--track-min-iou", "0.3"])
    assert f.tracks_topic == "/t" and track2d_options(f) == {"max_age": 5, "high_score": 0.4, "min_iou": 0.3}
    f = bag2d.parse_args(["--bag", "x", "--tracks-topic", "/tracks", "--track-max-age", "7"])
    assert f.tracks_topic == "/tracks" and track2d_options(f)["max_age"] == 7
    e = _Engine()
    tr = Detector2D.tracker(e, **track2d_options(f))
    assert tr.max_age == 7 and tr.capacity == 256 and tr.high_score == F(0.5) and tr.new_score == F(0.6)
    assert tr.min_iou == F(0.2) and tr.min_iou_low == F(0.5) and tr.max_gap == 2.0 and tr.alpha == tr.beta == F(0.5)
    assert Detector2D.tracker(e) is tr and not tr.gpu
    # bag2d --out-bag writes the tracks
    cam, ob = str(tmp_path / "cam.bag"), str(tmp_path / "o.bag")
    with Bag(cam, "w") as b:
        for s in range(1, 6):
            b.write("/cam", _frame(s))
    for topic in ("/tracks", None):
        drv = BagInference2D(engine=_Engine(), params={"sub_topic": "/cam", "pub_topic": "/o"}, bagfile=cam, out_dir=None,
                             save_png=False, out_bag=ob, batch=2, tracks_topic=topic)
        assert drv.start_inference() == 5
        with Bag(ob) as b:
            got = [(t, m) for t, m, _ in b.read_messages()]
        tracks = [m for t, m in got if t == "/tracks"]
        assert len([1 for t, _ in got if t == "/o/detections"]) == 5 and len(tracks) == (5 if topic else 0)
        if topic:
            assert drv.tracker().frames == 5 and [s for s, _ in drv.tracks] == [1, 2, 3, 4, 5]
            assert [[d.results[0].id for d in m.detections] for m in tracks] == [t[0].tolist() for _, t in drv.tracks]
            assert {d.results[0].id for m in tracks for d in m.detections} == {1, 2, 3}
        else:
            assert drv.tracks == [] and not hasattr(drv.engine, "_tracker")
