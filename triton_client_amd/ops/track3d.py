"""K24 — tracking LiDAR detections from one cloud to the next.

:func:`track_numpy` is the definition, bit for bit, in float32 (the pattern of
``ops/points_in_boxes.py``); the HIP entry ``tca_track3d`` (``csrc/kernels/track3d.hip``)
computes the same bits on the device, one single-workgroup launch per batch of clouds
against state that stays on the device.  The algorithm is the tracker of the CenterPoint
paper: greedy closest-centre matching on velocity-compensated positions.

**State** (:class:`TrackState`): ``capacity`` slots (1..1024), each ``id`` int32 (0: free),
``label`` int32, ``x, y`` (the position predicted to the current frame), ``vx, vy``,
``px, py`` (the position at the last match), ``pt`` (the float32 sum of ``dt`` since the
last match), ``age`` int32 (frames since the last match) and ``hits`` int32; plus
``next_id`` int32 (starts at 1) and ``overflow`` int32.

**Per-frame inputs**, all made on the host by :func:`track_table`: one 32-byte row per
detection (:data:`ROW_DTYPE`: ``x, y, vx, vy`` float32, ``label`` int32, ``flags`` int32,
two pad words; flag bit 0 "valid": the centre is finite and so is the velocity when there
is one; flag bit 1 "has velocity": 9-d boxes); ``dt`` float32 = (stamp - previous stamp) in
integer nanoseconds -> float64 seconds -> float32 (0 for the first frame ever, and for a
frame that resets); ``reset`` uint8 = 1 when the integer difference is negative or exceeds
``max_gap`` (a looped bag, a sensor restart); and ``max_dist2``, a float32 table of squared
gates (the metres squared in float64, then rounded) indexed by label, whose last entry
serves every label outside it.

**One frame**, every operation rounded to float32 on its own (no FMA: ``a*b + c`` is two
roundings), in this order:

1. *Reset*: with ``reset`` set every slot is freed; ``next_id`` keeps counting.
2. *Predict*, every live slot: ``x = x + vx*dt``, ``y = y + vy*dt``, ``pt = pt + dt``.
3. *Match*: detections in the given (published) order, invalid ones skipped.  The
   candidates of detection i are the live, still unclaimed slots of the same label with
   ``c = dx*dx + dy*dy <= max_dist2[label]`` (``dx = det.x - slot.x``; the gate is closed,
   a NaN cost compares false).  The minimum ``c`` wins, ties go to the lower slot index,
   and the slot is claimed: a detection does not give way to a later, closer one.
4. *Update* a matched slot: with "has velocity" ``v = det.v``; else if ``pt > 0``,
   ``vm = (det - p) / pt`` (IEEE division) and ``v = vm`` when ``hits == 1``, else
   ``v = v + alpha*(vm - v)``; with ``pt == 0`` ``v`` stays (nothing divides by zero).
   Then ``x, y = det``, ``p = det``, ``pt = 0``, ``age = 0``, ``hits += 1``.
5. *Age* the unmatched live slots: ``age += 1``, freed when ``age > max_age``.
6. *Births*: the unmatched valid detections, in order, take the lowest free slots (those
   freed in step 5 included): ``id = next_id++``, ``hits = 1``, ``v = det.v`` or 0.  Without
   a free slot the detection gets id 0 and ``overflow += 1``.  An invalid detection gets
   id 0 and touches nothing.

**Outputs** per detection: ``track_id`` int32, ``hits`` int32 and ``vel`` float32[2], the
slot's velocity after the update (id 0: hits 0, velocity 0).  Ids are never reused, and the
result does not depend on how a run of frames is cut into calls.

**Defaults** (configuration, not measurements): ``capacity = 256``, ``max_age = 3``,
``max_gap = 2.0`` s, ``alpha = 0.5``, ``max_dist`` 2.0 m for every class unless overridden
by class name; the CenterPoint family preloads the paper's nuScenes table
(:data:`CENTERPOINT_MAX_DIST`).  A frame carries at most :data:`MAX_DETS` detections to
the tracker; later ones get id 0.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from .. import _native
from .track_common import (HEADER, MAX_DETS, MAX_FRAMES, TrackerBase, TrackStateBase, device_enabled,  # noqa: F401
                           frame_times, stamp_ns)

MAX_CAPACITY = 1024  # kMaxCap in track3d.hip
FIELDS = (("id", np.int32), ("label", np.int32), ("x", np.float32), ("y", np.float32), ("vx", np.float32),
          ("vy", np.float32), ("px", np.float32), ("py", np.float32), ("pt", np.float32), ("age", np.int32),
          ("hits", np.int32))  # the order of the device state's arrays
ROW_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("vx", "<f4"), ("vy", "<f4"), ("label", "<i4"), ("flags", "<i4"),
                      ("pad0", "<i4"), ("pad1", "<i4")])
assert ROW_DTYPE.itemsize == 32
VALID, HAS_VEL = 1, 2

# the CenterPoint paper's per-class gates for nuScenes (metres), by class name
CENTERPOINT_MAX_DIST = {"car": 4.0, "truck": 4.0, "bus": 5.5, "trailer": 3.0, "pedestrian": 1.0, "motorcycle": 13.0,
                        "bicycle": 3.0, "barrier": 1.0, "traffic_cone": 1.0, "construction_vehicle": 1.0}
DEFAULT_MAX_DIST = 2.0

F = np.float32


# ------------------------------------------------------------------------- definition
class TrackState(TrackStateBase):
    """The tracker's state as host arrays (one per entry of :data:`FIELDS`)."""
    FIELDS, MAX_CAPACITY = FIELDS, MAX_CAPACITY


def gate_table(max_dist: Union[float, Dict[str, float], None] = None, names: Optional[Sequence[str]] = None,
               label_base: int = 1, default: float = DEFAULT_MAX_DIST) -> np.ndarray:
    """``max_dist2``: float32 squared gates indexed by label; the last entry is the gate of
    every label outside the table.  ``max_dist``: metres for every class, or a dict by class
    name (matched without case; a name that is no class of ``names`` is an error)."""
    names = list(names or [])
    if isinstance(max_dist, dict):
        by = {str(k).lower(): float(v) for k, v in max_dist.items()}
    else:
        by = {}
        default = default if max_dist is None else float(max_dist)
    metres = np.full(max(0, int(label_base)) + len(names) + 1, float(default), np.float64)
    known = {n.lower(): int(label_base) + i for i, n in enumerate(names)}
    for k, v in by.items():
        if k not in known:
            raise ValueError(f"max_dist: no class {k!r} (classes: {names})")
        metres[known[k]] = v
    if not (metres >= 0).all():
        raise ValueError("max_dist: gates are >= 0")
    return (metres * metres).astype(np.float32)


def detection_rows(boxes, labels) -> np.ndarray:
    """:data:`ROW_DTYPE` rows of boxes ``[n, 7]`` or CenterPoint's ``[n, 9]`` (vx, vy at 6, 7)."""
    b = np.asarray(boxes, np.float32)
    n = len(b)
    rows = np.zeros(n, ROW_DTYPE)
    if n == 0:
        return rows
    b = b.reshape(n, -1)
    rows["x"], rows["y"] = b[:, 0], b[:, 1]
    rows["label"] = np.asarray(labels).reshape(-1).astype(np.int32)
    ok = np.isfinite(b[:, 0]) & np.isfinite(b[:, 1])
    flags = np.zeros(n, np.int32)
    if b.shape[1] >= 9:
        rows["vx"], rows["vy"] = b[:, 6], b[:, 7]
        ok &= np.isfinite(b[:, 6]) & np.isfinite(b[:, 7])
        flags |= HAS_VEL
    rows["flags"] = flags | ok.astype(np.int32)
    return rows


@dataclass
class TrackBatch:
    """What :func:`track_table` makes of a batch of frames."""
    rows: np.ndarray     # ROW_DTYPE [det_off[-1]]
    det_off: np.ndarray  # int32 [F + 1]
    dt: np.ndarray       # float32 [F]
    reset: np.ndarray    # uint8 [F]
    sent: List[int]      # detections of each frame that reach the tracker (the first MAX_DETS)
    last_ns: Optional[int]  # the last frame's stamp


def track_table(preds: Sequence[dict], idx: Optional[Sequence], stamps: Sequence, prev_ns: Optional[int] = None,
                max_gap: float = 2.0) -> TrackBatch:
    """The per-frame inputs of a batch: ``preds[f]`` (``pred_boxes``, ``pred_labels``) selected by
    ``idx[f]`` (None: all), stamped ``stamps[f]``; ``prev_ns``: the stamp of the frame before the
    batch (None: the first frame ever)."""
    rows, sent = [], []
    for f, p in enumerate(preds):
        sel = slice(None) if idx is None else np.asarray(idx[f], np.int64)
        r = detection_rows(np.asarray(p["pred_boxes"])[sel], np.asarray(p["pred_labels"])[sel])[:MAX_DETS]
        rows.append(r)
        sent.append(len(r))
    dt, reset, last_ns = frame_times([stamps[f] for f in range(len(rows))], prev_ns, max_gap)
    return TrackBatch(rows=np.concatenate(rows) if rows else np.zeros(0, ROW_DTYPE),
                      det_off=np.concatenate([[0], np.cumsum(sent)]).astype(np.int32),
                      dt=dt, reset=reset, sent=sent, last_ns=last_ns)


def _gate(max_dist2: np.ndarray, label: int) -> np.float32:
    last = len(max_dist2) - 1
    return max_dist2[label if 0 <= label < last else last]


def track_frame(st: TrackState, rows: np.ndarray, dt, reset, max_dist2: np.ndarray, max_age: int = 3,
                alpha=0.5) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The definition for one frame, in place on ``st`` → ``(track_id [n] int32, hits [n] int32,
    vel [n, 2] float32)``."""
    n = len(rows)
    if n > MAX_DETS:
        raise ValueError(f"{n} detections in a frame: at most {MAX_DETS}")
    dt, alpha = F(dt), F(alpha)
    ids, hits, vel = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 2), F)
    with np.errstate(all="ignore"):
        if reset:
            st.id[:] = 0
        live = st.id != 0
        st.x[live] = st.x[live] + st.vx[live] * dt
        st.y[live] = st.y[live] + st.vy[live] * dt
        st.pt[live] = st.pt[live] + dt
        claimed = np.zeros(st.capacity, bool)
        match = np.full(n, -1, np.int64)
        valid = (rows["flags"] & VALID) != 0
        for i in np.flatnonzero(valid):
            d = rows[i]
            dx, dy = d["x"] - st.x, d["y"] - st.y
            c = dx * dx + dy * dy
            ok = live & ~claimed & (st.label == d["label"]) & (c <= _gate(max_dist2, int(d["label"])))
            if not ok.any():
                continue
            s = int(np.flatnonzero(ok & (c == c[ok].min()))[0])  # ties: the lower slot
            claimed[s] = True
            match[i] = s
        for i in np.flatnonzero(match >= 0):
            d, s = rows[i], int(match[i])
            if d["flags"] & HAS_VEL:
                st.vx[s], st.vy[s] = d["vx"], d["vy"]
            elif st.pt[s] > 0:
                vmx, vmy = (d["x"] - st.px[s]) / st.pt[s], (d["y"] - st.py[s]) / st.pt[s]
                if st.hits[s] == 1:
                    st.vx[s], st.vy[s] = vmx, vmy
                else:
                    st.vx[s] = st.vx[s] + alpha * (vmx - st.vx[s])
                    st.vy[s] = st.vy[s] + alpha * (vmy - st.vy[s])
            st.x[s], st.y[s], st.px[s], st.py[s] = d["x"], d["y"], d["x"], d["y"]
            st.pt[s], st.age[s] = 0, 0
            st.hits[s] += 1
            ids[i], hits[i], vel[i] = st.id[s], st.hits[s], (st.vx[s], st.vy[s])
        old = live & ~claimed
        st.age[old] += 1
        st.id[old & (st.age > max_age)] = 0
        free = np.flatnonzero(st.id == 0)
        for r, i in enumerate(np.flatnonzero(valid & (match < 0))):
            if r >= len(free):
                st.overflow = np.int32(st.overflow + 1)
                continue
            d, s = rows[i], int(free[r])
            has = bool(d["flags"] & HAS_VEL)
            st.id[s], st.label[s] = st.next_id, d["label"]
            st.next_id = np.int32(st.next_id + 1)
            st.x[s], st.y[s], st.px[s], st.py[s] = d["x"], d["y"], d["x"], d["y"]
            st.vx[s], st.vy[s] = (d["vx"], d["vy"]) if has else (0, 0)
            st.pt[s], st.age[s], st.hits[s] = 0, 0, 1
            ids[i], hits[i], vel[i] = st.id[s], 1, (st.vx[s], st.vy[s])
    return ids, hits, vel


def track_numpy(st: TrackState, batch: TrackBatch, max_dist2: np.ndarray, max_age: int = 3, alpha=0.5) -> List[tuple]:
    """The definition over a batch of frames, in place on ``st`` → per frame ``(track_id, hits, vel)``."""
    out = []
    for f in range(len(batch.dt)):
        rows = batch.rows[batch.det_off[f]:batch.det_off[f + 1]]
        out.append(track_frame(st, rows, batch.dt[f], batch.reset[f], max_dist2, max_age, alpha))
    return out


# --------------------------------------------------------------------------------- GPU
def launch(rows: int, det_off_host, n_frames: int, dt: int, reset: int, max_dist2: int, n_gates: int, state: int,
           capacity: int, max_age: int, alpha: float, out: int, stream=None) -> None:
    """The launch alone, on pointers (``det_off_host``: a host int32 array of ``n_frames + 1``
    offsets, validated by the launcher and passed by value): no allocation, no copy, no sync."""
    off = np.ascontiguousarray(det_off_host, np.int32)
    _native.call("tca_track3d", rows, off.ctypes.data, n_frames, dt, reset, max_dist2, n_gates, state, capacity,
                 max_age, float(alpha), out, _native.stream_ptr(stream))


class Tracker3D(TrackerBase):
    """Tracks detections over frames: on a GPU with ``tca_track3d`` (its own stream, pinned
    staging and device state: one H2D of the rows, ``dt``, ``reset`` and gates, one launch and
    one D2H of the outputs per batch of up to :data:`MAX_FRAMES` frames), on the CPU and with
    ``TCA_DEVICE_TRACK=0`` with the definition.  ``max_dist``: metres, or a dict by class name
    of ``names`` (``label_base``: the label of ``names[0]``)."""
    ENTRY, STATE = "tca_track3d", TrackState

    def __init__(self, capacity: int = 256, max_age: int = 3, max_dist: Union[float, Dict[str, float], None] = None,
                 max_gap: float = 2.0, alpha: float = 0.5, names: Optional[Sequence[str]] = None,
                 label_base: int = 1, device="cpu"):
        self.alpha = np.float32(alpha)
        self.max_dist2 = gate_table(max_dist, names, label_base)
        super().__init__(capacity, max_age, max_gap, device)

    def _extra_inputs(self) -> List[np.ndarray]:
        return [self.max_dist2]

    def _launch(self, rows, det_off, n_frames, dt, reset, extra, out) -> None:
        launch(rows, det_off, n_frames, dt, reset, extra[0], len(self.max_dist2), self._state.data_ptr(), self.capacity,
               self.max_age, self.alpha, out, self._stream)

    # ---------------------------------------------------------------------- API
    def track(self, preds: Sequence[dict], idx: Optional[Sequence], stamps: Sequence) -> List[tuple]:
        """Frames in order → per frame ``(track_id [n] int32, hits [n] int32, vel [n, 2] float32)``
        aligned with ``preds[f][idx[f]]`` (all of ``preds[f]`` without an index)."""
        with self._lock:
            b = track_table(preds, idx, stamps, self.prev_ns, self.max_gap)
            res = self._run_device(b) if self.gpu else track_numpy(self._host, b, self.max_dist2, self.max_age,
                                                                   self.alpha)
            self.prev_ns = b.last_ns
            self.frames += len(b.dt)
        out = []
        for f, (ids, hits, vel) in enumerate(res):
            n = len(np.asarray(preds[f]["pred_labels"])) if idx is None else len(idx[f])
            if n > len(ids):  # detections past MAX_DETS: id 0
                ids, hits = np.pad(ids, (0, n - len(ids))), np.pad(hits, (0, n - len(hits)))
                vel = np.pad(vel, ((0, n - len(vel)), (0, 0)))
            out.append((ids, hits, vel))
        return out


def parse_max_dist(text: Optional[str]) -> Union[float, Dict[str, float], None]:
    """``--track-max-dist``: ``"3"`` (metres for every class) or ``"Car=4,Pedestrian=1"``."""
    if not text:
        return None
    if "=" not in text:
        return float(text)
    out = {}
    for part in text.split(","):
        k, _, v = part.partition("=")
        if not k.strip() or not v.strip():
            raise ValueError(f"--track-max-dist {text!r}: NAME=METRES[,NAME=METRES...]")
        out[k.strip()] = float(v)
    return out
