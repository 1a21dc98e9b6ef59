"""K25 — tracking camera detections from one frame to the next.

:func:`track_numpy` is the definition, bit for bit, in float32 (the pattern of
``ops/track3d.py``); the HIP entry ``tca_track2d`` (``csrc/kernels/track2d.hip``) computes
the same bits on the device, one single-workgroup launch per batch of frames against state
that stays on the device.  The algorithm is ByteTrack's association (Zhang et al., ECCV
2022) made deterministic: detections choose in descending score order, high-score
detections may match any live track, low-score ones may only keep alive a track that was
matched in the previous frame and never start one; a fixed-gain constant-velocity filter
(K24's velocity rule plus a smoothed size) stands in for the Kalman filter, so there are no
covariance matrices to match bit for bit.

**State** (:class:`TrackState2D`): ``capacity`` slots (1..512), each ``id`` int32 (0: free),
``label`` int32, ``cx, cy`` (the centre predicted to the current frame), ``w, h`` (the
smoothed size), ``vx, vy`` (pixels per second), ``px, py`` (the centre at the last match),
``pt`` (the float32 sum of ``dt`` since the last match), ``age`` int32 (frames since the last
match) and ``hits`` int32; plus ``next_id`` int32 (starts at 1) and ``overflow`` int32.

**Per-frame inputs**, all made on the host by :func:`track_table`: one 32-byte row per
detection (:data:`ROW_DTYPE`: ``x1, y1, x2, y2, score`` float32, ``label`` int32, ``flags``
int32, one pad word; flag bit 0 "valid": the five floats are finite, ``x2 > x1`` and ``y2 >
y1``; bit 1 "high": ``score >= high_score``; bit 2 "birth": ``score >= new_score``, both
compared in float32 on the host, so the kernel never compares a score; an invalid row has
no other bit).  The rows of a frame are ordered by descending score
(``np.argsort(-score, kind="stable")``: ties keep the caller's order), invalid rows last;
the permutation stays on the host and every public result is aligned with the caller's
order.  ``dt`` float32 and ``reset`` uint8 are exactly K24's (:func:`stamp_ns`: integer
nanoseconds -> float64 seconds -> float32; a reset on a negative difference or a gap over
``max_gap``).

**One frame**, every operation rounded to float32 on its own (no FMA), in this order:

1. *Reset*: with ``reset`` set every slot is freed; ``next_id`` keeps counting.
2. *Predict*, every live slot: ``cx = cx + vx*dt``, ``cy = cy + vy*dt``, ``pt = pt + dt``;
   ``w`` and ``h`` stay.
3. *Match*: rows in the given order, invalid ones skipped.  The candidates of a row are the
   live, still unclaimed slots of the same label — for a row without the "high" flag only
   those with ``age == 0`` (matched, or born, in the previous frame; ``age`` as it is before
   step 5) — with ``q >= gate`` (``min_iou`` for a high row, ``min_iou_low`` for a low one;
   the gate is closed, a NaN ``q`` compares false).  The maximum ``q`` wins, ties go to the
   lower slot, and the slot is claimed.  ``q``: ``tx1 = cx - 0.5*w``, ``tx2 = cx + 0.5*w``
   (and y); ``iw = min(x2, tx2) - max(x1, tx1)`` (and ``ih``); ``iw = iw > 0 ? iw : 0``;
   ``inter = iw*ih``; ``u = ((x2-x1)*(y2-y1) + (tx2-tx1)*(ty2-ty1)) - inter``;
   ``q = u > 0 ? inter/u : 0`` (IEEE division).  ``min(a, b)`` is ``a < b ? a : b`` and
   ``max(a, b)`` is ``a > b ? a : b`` with the row's value as ``a``: explicit comparisons
   (``np.where`` here), because ``fminf`` and ``np.minimum`` disagree on NaN and a predicted
   centre can overflow.
4. *Update* a matched slot: with ``dcx = (x1 + x2)*0.5`` (and ``dcy``): if ``pt > 0``,
   ``vm = (dc - p)/pt`` and ``v = vm`` when ``hits == 1``, else ``v = v + alpha*(vm - v)``;
   with ``pt == 0`` ``v`` stays (nothing divides by zero).  Then ``cx, cy = dc``,
   ``w = w + beta*((x2-x1) - w)`` (and ``h``), ``p = dc``, ``pt = 0``, ``age = 0``,
   ``hits += 1``.
5. *Age* the unmatched live slots: ``age += 1``, freed when ``age > max_age``.
6. *Births*: the unmatched valid rows with the "birth" flag, in row order, take the lowest
   free slots (those freed in step 5 included): ``id = next_id++``, ``hits = 1``, ``v = 0``,
   ``w, h`` from the row, ``c = p = dc``.  Without a free slot the row gets id 0 and
   ``overflow += 1``; an unmatched row without the flag gets id 0 and is no overflow.

**Outputs** per detection: ``track_id`` int32, ``hits`` int32 and ``vel`` float32[2] (pixels
per second; id 0: zeros).  Ids are never reused, and the result does not depend on how a
run of frames is cut into calls.

**Defaults** — configuration taken from the ByteTrack paper, not measurements:
``high_score = 0.5``, ``new_score = 0.6``, ``min_iou = 0.2``, ``min_iou_low = 0.5``,
``max_age = 30``, ``capacity = 256``, ``max_gap = 2.0`` s, ``alpha = 0.5``, ``beta = 0.5``.
A frame carries at most :data:`MAX_DETS` rows (the highest scores) to the tracker; later
ones get id 0.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .. import _native
from .track_common import (HEADER, MAX_DETS, MAX_FRAMES, TrackerBase, TrackStateBase, device_enabled,  # noqa: F401
                           frame_times, stamp_ns)

MAX_CAPACITY = 512   # kMaxCap in track2d.hip
FIELDS = (("id", np.int32), ("label", np.int32), ("cx", np.float32), ("cy", np.float32), ("w", np.float32),
          ("h", np.float32), ("vx", np.float32), ("vy", np.float32), ("px", np.float32), ("py", np.float32),
          ("pt", np.float32), ("age", np.int32), ("hits", np.int32))  # the order of the device state's arrays
ROW_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("score", "<f4"), ("label", "<i4"),
                      ("flags", "<i4"), ("pad0", "<i4")])
assert ROW_DTYPE.itemsize == 32
VALID, HIGH, BIRTH = 1, 2, 4
EVENTS = ("high_match", "low_match", "low_refused_age", "birth", "birth_refused", "death", "overflow", "reset", "tie")

F = np.float32


# ------------------------------------------------------------------------- definition
class TrackState2D(TrackStateBase):
    """The tracker's state as host arrays (one per entry of :data:`FIELDS`)."""
    FIELDS, MAX_CAPACITY = FIELDS, MAX_CAPACITY


def detection_rows(dets, high_score=0.5, new_score=0.6) -> Tuple[np.ndarray, np.ndarray]:
    """``dets`` [n, 6] (``x1, y1, x2, y2, conf, cls``) → (:data:`ROW_DTYPE` rows in descending
    score order with the invalid ones last, ``order`` [n]: row k is ``dets[order[k]]``)."""
    d = np.asarray(dets, np.float32).reshape(-1, 6)
    n = len(d)
    rows = np.zeros(n, ROW_DTYPE)
    if n == 0:
        return rows, np.zeros(0, np.int64)
    with np.errstate(all="ignore"):
        score = d[:, 4]
        valid = np.isfinite(d[:, :5]).all(axis=1) & (d[:, 2] > d[:, 0]) & (d[:, 3] > d[:, 1])
        good = np.flatnonzero(valid)
        order = np.concatenate([good[np.argsort(-score[good], kind="stable")], np.flatnonzero(~valid)])
        d, valid = d[order], valid[order]
        cls = np.where(np.isfinite(d[:, 5]), d[:, 5], F(0))
        rows["label"] = np.clip(cls, -2.0 ** 31, 2.0 ** 31 - 128).astype(np.int32)
        flags = valid * VALID | (valid & (d[:, 4] >= F(high_score))) * HIGH | (valid & (d[:, 4] >= F(new_score))) * BIRTH
    rows["x1"], rows["y1"], rows["x2"], rows["y2"], rows["score"] = d[:, 0], d[:, 1], d[:, 2], d[:, 3], d[:, 4]
    rows["flags"] = flags.astype(np.int32)
    return rows, order


@dataclass
class TrackBatch2D:
    """What :func:`track_table` makes of a batch of frames."""
    rows: np.ndarray        # ROW_DTYPE [det_off[-1]]
    det_off: np.ndarray     # int32 [F + 1]
    dt: np.ndarray          # float32 [F]
    reset: np.ndarray       # uint8 [F]
    sent: List[int]         # rows of each frame that reach the tracker (the first MAX_DETS)
    order: List[np.ndarray]  # per frame: row k is the caller's detection order[k] (all n of them)
    last_ns: Optional[int]  # the last frame's stamp


def track_table(dets_per_frame: Sequence, stamps: Sequence, prev_ns: Optional[int] = None, max_gap: float = 2.0,
                high_score=0.5, new_score=0.6) -> TrackBatch2D:
    """The per-frame inputs of a batch: ``dets_per_frame[f]`` [n, 6] stamped ``stamps[f]``;
    ``prev_ns``: the stamp of the frame before the batch (None: the first frame ever)."""
    rows, sent, orders = [], [], []
    for f, d in enumerate(dets_per_frame):
        r, order = detection_rows(d, high_score, new_score)
        r = r[:MAX_DETS]
        rows.append(r)
        sent.append(len(r))
        orders.append(order)
    dt, reset, last_ns = frame_times([stamps[f] for f in range(len(rows))], prev_ns, max_gap)
    return TrackBatch2D(rows=np.concatenate(rows) if rows else np.zeros(0, ROW_DTYPE),
                        det_off=np.concatenate([[0], np.cumsum(sent)]).astype(np.int32),
                        dt=dt, reset=reset, sent=sent, order=orders, last_ns=last_ns)


def _count(events: Optional[dict], name: str, n: int = 1) -> None:
    if events is not None and n:
        events[name] = events.get(name, 0) + int(n)


def track_frame(st: TrackState2D, rows: np.ndarray, dt, reset, min_iou=0.2, min_iou_low=0.5, max_age: int = 30,
                alpha=0.5, beta=0.5, events: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The definition for one frame, in place on ``st`` → ``(track_id [n] int32, hits [n] int32,
    vel [n, 2] float32)`` in row order.  ``events``: a dict that gains the counts of
    :data:`EVENTS` (what happened, for the tests' scene generator; no result depends on it)."""
    n = len(rows)
    if n > MAX_DETS:
        raise ValueError(f"{n} detections in a frame: at most {MAX_DETS}")
    dt, alpha, beta, half = F(dt), F(alpha), F(beta), F(0.5)
    gates = (F(min_iou_low), F(min_iou))
    ids, hits, vel = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 2), F)
    with np.errstate(all="ignore"):
        if reset:
            _count(events, "reset")
            st.id[:] = 0
        live = st.id != 0
        st.cx[live] = st.cx[live] + st.vx[live] * dt
        st.cy[live] = st.cy[live] + st.vy[live] * dt
        st.pt[live] = st.pt[live] + dt
        tx1, tx2 = st.cx - half * st.w, st.cx + half * st.w
        ty1, ty2 = st.cy - half * st.h, st.cy + half * st.h
        t_area = (tx2 - tx1) * (ty2 - ty1)
        fresh = st.age == 0
        claimed = np.zeros(st.capacity, bool)
        match = np.full(n, -1, np.int64)
        valid = (rows["flags"] & VALID) != 0
        for i in np.flatnonzero(valid):
            d = rows[i]
            high = bool(d["flags"] & HIGH)
            x1, y1, x2, y2 = d["x1"], d["y1"], d["x2"], d["y2"]
            iw = np.where(x2 < tx2, x2, tx2) - np.where(x1 > tx1, x1, tx1)
            ih = np.where(y2 < ty2, y2, ty2) - np.where(y1 > ty1, y1, ty1)
            iw, ih = np.where(iw > 0, iw, F(0)), np.where(ih > 0, ih, F(0))
            inter = iw * ih
            u = ((x2 - x1) * (y2 - y1) + t_area) - inter
            q = np.where(u > 0, inter / u, F(0)).astype(F)
            near = live & ~claimed & (st.label == d["label"]) & (q >= gates[high])
            ok = near if high else near & fresh
            if events is not None and not high and (near & ~fresh).any():
                _count(events, "low_refused_age")
            if not ok.any():
                continue
            best = ok & (q == q[ok].max())
            _count(events, "tie", best.sum() > 1)
            _count(events, "high_match" if high else "low_match")
            s = int(np.flatnonzero(best)[0])  # ties: the lower slot
            claimed[s] = True
            match[i] = s
        for i in np.flatnonzero(match >= 0):
            d, s = rows[i], int(match[i])
            dcx, dcy = (d["x1"] + d["x2"]) * half, (d["y1"] + d["y2"]) * half
            if st.pt[s] > 0:
                vmx, vmy = (dcx - st.px[s]) / st.pt[s], (dcy - st.py[s]) / st.pt[s]
                if st.hits[s] == 1:
                    st.vx[s], st.vy[s] = vmx, vmy
                else:
                    st.vx[s] = st.vx[s] + alpha * (vmx - st.vx[s])
                    st.vy[s] = st.vy[s] + alpha * (vmy - st.vy[s])
            st.cx[s], st.cy[s], st.px[s], st.py[s] = dcx, dcy, dcx, dcy
            st.w[s] = st.w[s] + beta * ((d["x2"] - d["x1"]) - st.w[s])
            st.h[s] = st.h[s] + beta * ((d["y2"] - d["y1"]) - st.h[s])
            st.pt[s], st.age[s] = 0, 0
            st.hits[s] += 1
            ids[i], hits[i], vel[i] = st.id[s], st.hits[s], (st.vx[s], st.vy[s])
        old = live & ~claimed
        st.age[old] += 1
        dead = old & (st.age > max_age)
        _count(events, "death", dead.sum())
        st.id[dead] = 0
        free = np.flatnonzero(st.id == 0)
        unmatched = valid & (match < 0)
        _count(events, "birth_refused", (unmatched & ((rows["flags"] & BIRTH) == 0)).sum())
        for r, i in enumerate(np.flatnonzero(unmatched & ((rows["flags"] & BIRTH) != 0))):
            if r >= len(free):
                _count(events, "overflow")
                st.overflow = np.int32(st.overflow + 1)
                continue
            _count(events, "birth")
            d, s = rows[i], int(free[r])
            dcx, dcy = (d["x1"] + d["x2"]) * half, (d["y1"] + d["y2"]) * half
            st.id[s], st.label[s] = st.next_id, d["label"]
            st.next_id = np.int32(st.next_id + 1)
            st.cx[s], st.cy[s], st.px[s], st.py[s] = dcx, dcy, dcx, dcy
            st.w[s], st.h[s] = d["x2"] - d["x1"], d["y2"] - d["y1"]
            st.vx[s], st.vy[s] = 0, 0
            st.pt[s], st.age[s], st.hits[s] = 0, 0, 1
            ids[i], hits[i] = st.id[s], 1
    return ids, hits, vel


def track_numpy(st: TrackState2D, batch: TrackBatch2D, min_iou=0.2, min_iou_low=0.5, max_age: int = 30, alpha=0.5,
                beta=0.5, events: Optional[dict] = None) -> List[tuple]:
    """The definition over a batch of frames, in place on ``st`` → per frame ``(track_id, hits,
    vel)`` in row order (:func:`unpermute` aligns them with the caller's order)."""
    out = []
    for f in range(len(batch.dt)):
        rows = batch.rows[batch.det_off[f]:batch.det_off[f + 1]]
        out.append(track_frame(st, rows, batch.dt[f], batch.reset[f], min_iou, min_iou_low, max_age, alpha, beta,
                               events))
    return out


def unpermute(batch: TrackBatch2D, res: Sequence[tuple]) -> List[tuple]:
    """Results in row order → aligned with the caller's detections (those past
    :data:`MAX_DETS` rows: id 0)."""
    out = []
    for order, (ids, hits, vel) in zip(batch.order, res):
        n, k = len(order), len(ids)
        i, h, v = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 2), F)
        i[order[:k]], h[order[:k]], v[order[:k]] = ids, hits, vel
        out.append((i, h, v))
    return out


# --------------------------------------------------------------------------------- GPU
def launch(rows: int, det_off_host, n_frames: int, dt: int, reset: int, state: int, capacity: int, max_age: int,
           min_iou: float, min_iou_low: float, alpha: float, beta: float, out: int, stream=None) -> None:
    """The launch alone, on pointers (``det_off_host``: a host int32 array of ``n_frames + 1``
    offsets, validated by the launcher and passed by value): no allocation, no copy, no sync."""
    off = np.ascontiguousarray(det_off_host, np.int32)
    _native.call("tca_track2d", rows, off.ctypes.data, n_frames, dt, reset, state, capacity, max_age, float(min_iou),
                 float(min_iou_low), float(alpha), float(beta), out, _native.stream_ptr(stream))


class Tracker2D(TrackerBase):
    """Tracks camera detections over frames: on a GPU with ``tca_track2d`` (its own stream,
    pinned staging and device state: one H2D of the rows, ``dt`` and ``reset``, one launch and
    one D2H of the outputs per chunk of up to :data:`MAX_FRAMES` frames), on the CPU and with
    ``TCA_DEVICE_TRACK=0`` with the definition."""
    ENTRY, STATE = "tca_track2d", TrackState2D

    def __init__(self, capacity: int = 256, max_age: int = 30, high_score: float = 0.5, new_score: float = 0.6,
                 min_iou: float = 0.2, min_iou_low: float = 0.5, max_gap: float = 2.0, alpha: float = 0.5,
                 beta: float = 0.5, device="cpu"):
        self.high_score, self.new_score = np.float32(high_score), np.float32(new_score)
        self.min_iou, self.min_iou_low = np.float32(min_iou), np.float32(min_iou_low)
        self.alpha, self.beta = np.float32(alpha), np.float32(beta)
        super().__init__(capacity, max_age, max_gap, device)

    def _launch(self, rows, det_off, n_frames, dt, reset, extra, out) -> None:
        launch(rows, det_off, n_frames, dt, reset, self._state.data_ptr(), self.capacity, self.max_age, self.min_iou,
               self.min_iou_low, self.alpha, self.beta, out, self._stream)

    # ---------------------------------------------------------------------- API
    def track(self, dets_per_frame: Sequence, stamps: Sequence) -> List[tuple]:
        """Frames in order, each ``[n, 6]`` (``x1, y1, x2, y2, conf, cls``) → per frame ``(track_id
        [n] int32, hits [n] int32, vel [n, 2] float32)`` aligned with the frame's detections."""
        with self._lock:
            b = track_table(dets_per_frame, stamps, self.prev_ns, self.max_gap, self.high_score, self.new_score)
            res = self._run_device(b) if self.gpu else track_numpy(self._host, b, self.min_iou, self.min_iou_low,
                                                                   self.max_age, self.alpha, self.beta)
            self.prev_ns = b.last_ns
            self.frames += len(b.dt)
        return unpermute(b, res)
