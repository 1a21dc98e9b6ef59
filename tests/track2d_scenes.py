"""Random camera scenes for the tracker tests (tests/test_track2d.py and
tests/test_track2d_gpu.py import this module, so both see the same frames).

Coordinates lie on a quarter-pixel grid and scores on a 1/64 grid, so that exact ties occur
(equal scores; bit-equal IoUs: every corner, size and area below is exact in float32).  A scene
has a few classes, objects that appear and disappear, dropouts, jitter, score dips into the
low tier, weak objects whose score stays under the birth score, false positives, one frame
whose stamp goes back and one gap above ``max_gap`` (two resets), and *twins*: pairs of
static objects of one class and size, 20 px apart, that some frames answer with a single
detection exactly between them — its IoU with both tracks is the same bits.
"""
from functools import lru_cache

import numpy as np

from triton_client_amd.ops import track2d as T

F = np.float32
MS = 1_000_000  # nanoseconds
SIZE = 1024.0   # the picture: SIZE x SIZE


def _q(a):
    """Onto the quarter-pixel grid."""
    return np.round(np.asarray(a, np.float64) * 4.0) / 4.0


def _score(a):
    """Onto the 1/64 grid."""
    return np.round(np.asarray(a, np.float64) * 64.0) / 64.0


def scene(seed, counts, n_obj=60, n_twins=4, classes=3):
    """Frames of a random scene → ``(dets_per_frame, stamps)``: ``counts[f]`` detections in
    frame f (visible objects first, false positives fill up), in random order."""
    r = np.random.default_rng(seed)
    nf = len(counts)
    pos = _q(r.uniform(60, SIZE - 60, (n_obj, 2)))
    vel = r.uniform(-90, 90, (n_obj, 2))  # pixels per second
    wh = _q(r.uniform(24, 90, (n_obj, 2)))
    lab = r.integers(0, classes, n_obj)
    base = _score(r.uniform(0.65, 0.95, n_obj))
    weak = r.random(n_obj) < 0.12          # never reaches the birth score
    base[weak] = _score(r.uniform(0.5, 0.59, weak.sum()))
    first = r.integers(0, max(1, nf // 2), n_obj)
    first[r.random(n_obj) < 0.5] = 0
    last = first + r.integers(3, nf + 3, n_obj)
    twins = list(range(0, 2 * n_twins, 2))  # objects k, k + 1
    for k in twins:
        pos[k + 1] = pos[k] + (20.0, 0.0)
        wh[k] = wh[k + 1] = _q(r.uniform(40, 60, 2))
        lab[k + 1] = lab[k]
        base[k] = base[k + 1] = 0.875
        first[k] = first[k + 1] = 0
        last[k] = last[k + 1] = nf + 1
    vel[:2 * n_twins] = 0.0
    back, gap = (nf // 2, nf // 2 + 6) if nf >= 16 else (-1, -1)
    dets, stamps, t = [], [], 5_000 * MS
    for f, n in enumerate(counts):
        dt = int(r.choice([0, 33, 33, 33, 66, 125])) * MS if f not in (0, 3) else 0  # (frame 3: always a dt of 0)
        if f == back:
            dt = -500 * MS
        elif f == gap:
            dt = 2_500 * MS
        t += dt
        pos = pos + vel * (max(dt, 0) * 1e-9)
        seen = (first <= f) & (f < last) & (r.random(n_obj) > 0.15)
        seen[:2 * n_twins] = (first[:2 * n_twins] <= f)
        boxes, scores, labels = [], [], []
        merged = [k for k in twins if seen[k] and f > 1 and r.random() < 0.3]
        for k in merged:  # one detection for both twins, exactly between them
            seen[k] = seen[k + 1] = False
            c = _q(pos[k] - wh[k] / 2) + (10.0, 0.0)  # the twins' corners are this -10 and +10
            boxes.append(np.r_[c, c + wh[k]])
            scores.append(0.9375)
            labels.append(lab[k])
        for k in np.flatnonzero(seen):
            c = pos[k] if k < 2 * n_twins else _q(pos[k] + r.normal(0, 1.0, 2))
            boxes.append(np.r_[_q(c - wh[k] / 2), _q(c - wh[k] / 2) + wh[k]])
            s = base[k]
            if k >= 2 * n_twins and r.random() < 0.2:  # a dip into the low tier
                s = _score(r.uniform(0.15, 0.45))
            scores.append(s)
            labels.append(lab[k])
        o = r.permutation(len(boxes))[:n]
        boxes, scores, labels = [boxes[i] for i in o], [scores[i] for i in o], [labels[i] for i in o]
        for _ in range(n - len(boxes)):  # false positives
            c, s = _q(r.uniform(40, SIZE - 40, 2)), _q(r.uniform(16, 70, 2))
            boxes.append(np.r_[c - s / 2, c - s / 2 + s])
            scores.append(_score(r.uniform(0.1, 0.95)))
            labels.append(r.integers(0, classes))
        d = np.zeros((n, 6), F)
        if n:
            o = r.permutation(n)
            d[:, :4], d[:, 4], d[:, 5] = np.asarray(boxes)[o], np.asarray(scores)[o], np.asarray(labels)[o]
        dets.append(d)
        stamps.append(t)
    return dets, stamps


def same_results(a, b):
    assert len(a) == len(b)
    for (i, h, v), (wi, wh, wv) in zip(a, b):
        np.testing.assert_array_equal(i, wi)
        np.testing.assert_array_equal(h, wh)
        np.testing.assert_array_equal(v.view(np.uint32), wv.view(np.uint32))


def run_cut(tr, dets, stamps, cut):
    """The frames through ``tr`` in calls of ``cut`` frames (the last call: what is left)."""
    out = []
    for f in range(0, len(dets), cut):
        out += tr.track(dets[f:f + cut], stamps[f:f + cut])
    return out


# The random scenes of the GPU file: 65 frames (two launches when they go in one call) at these
# capacities, in calls of these many frames.  The counts pass a wave's edges and exceed 64 and 65.
CAPACITIES = (1, 64, 65, 512)
CALLS = (1, 33, 65)
FRAMES = 65
MAX_AGE = 2


def counts_of(capacity):
    r = np.random.default_rng(1000 + capacity)
    c = r.integers(20, 60, FRAMES)
    c[[5, 20, 41]] = (0, 1, 90)
    return [int(v) for v in c]


@lru_cache(maxsize=None)
def random_scene(capacity):
    """→ ``(dets, stamps)`` of the capacity's scene (seed: the capacity)."""
    return scene(capacity, counts_of(capacity))


@lru_cache(maxsize=None)
def reference(capacity):
    """The definition over the capacity's scene in one call → ``(results aligned with the
    caller's order, final state, events)``; computed once, shared, and left unchanged."""
    dets, stamps = random_scene(capacity)
    batch = T.track_table(dets, stamps)
    st, events = T.TrackState2D(capacity), {}
    res = T.unpermute(batch, T.track_numpy(st, batch, max_age=MAX_AGE, events=events))
    return res, st, events
