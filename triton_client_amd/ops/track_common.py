"""What the LiDAR tracker (``ops/track3d.py``, K24) and the camera tracker (``ops/track2d.py``,
K25) share on the host: the state as host arrays, the stamp -> ``dt`` / ``reset`` arithmetic,
and the device side of a tracker (its stream, pinned staging, the two copies per chunk of
frames and the split of the results per frame).
"""
from __future__ import annotations

import os
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_DETS = 512       # detections per frame: kMaxDets in track2d.hip and track3d.hip
MAX_FRAMES = 64      # frames per launch: kMaxFrames
HEADER = 4           # int32 words in front of the device state: next_id, overflow, 2 pad


def device_enabled() -> bool:
    """``TCA_DEVICE_TRACK=0`` keeps the definition on GPU engines too."""
    return os.environ.get("TCA_DEVICE_TRACK", "1") != "0"


def stamp_ns(stamp) -> int:
    """Integer nanoseconds of a ``Time``, a header, or a number of nanoseconds."""
    stamp = getattr(stamp, "stamp", stamp)
    return int(stamp.to_nsec()) if hasattr(stamp, "to_nsec") else int(stamp)


def frame_times(stamps: Sequence, prev_ns: Optional[int], max_gap: float) -> Tuple[np.ndarray, np.ndarray, Optional[int]]:
    """``(dt float32 [F], reset uint8 [F], the last stamp)`` of frames stamped ``stamps`` after a
    frame at ``prev_ns`` (None: the first frame ever).  ``dt``: the integer difference in
    nanoseconds -> float64 seconds -> float32; a negative difference or one over ``max_gap``
    resets, with ``dt`` 0."""
    gap_ns = int(round(float(max_gap) * 1e9))
    dts, resets = [], []
    for stamp in stamps:
        now = stamp_ns(stamp)
        d = 0 if prev_ns is None else now - prev_ns
        rs = d < 0 or d > gap_ns
        dts.append(np.float32(0.0) if rs else np.float32(np.float64(d) * 1e-9))
        resets.append(1 if rs else 0)
        prev_ns = now
    return np.asarray(dts, np.float32).reshape(-1), np.asarray(resets, np.uint8).reshape(-1), prev_ns


class TrackStateBase:
    """A tracker's state as host arrays, one per entry of the subclass's ``FIELDS`` (the order
    of the device state's arrays), at most ``MAX_CAPACITY`` slots."""
    FIELDS: tuple = ()
    MAX_CAPACITY = 0

    def __init__(self, capacity: int):
        capacity = int(capacity)
        if not 1 <= capacity <= self.MAX_CAPACITY:
            raise ValueError(f"capacity {capacity}: 1..{self.MAX_CAPACITY}")
        self.capacity = capacity
        for name, dt in self.FIELDS:
            setattr(self, name, np.zeros(capacity, dt))
        self.next_id = np.int32(1)
        self.overflow = np.int32(0)

    def words(self) -> np.ndarray:
        """The device layout: int32 ``[HEADER + len(FIELDS) * capacity]``."""
        w = np.zeros(HEADER + len(self.FIELDS) * self.capacity, np.int32)
        w[0], w[1] = self.next_id, self.overflow
        for k, (name, _) in enumerate(self.FIELDS):
            w[HEADER + k * self.capacity: HEADER + (k + 1) * self.capacity] = getattr(self, name).view(np.int32)
        return w

    @classmethod
    def from_words(cls, w: np.ndarray, capacity: int):
        st = cls(capacity)
        w = np.ascontiguousarray(w, np.int32)
        st.next_id, st.overflow = np.int32(w[0]), np.int32(w[1])
        for k, (name, dt) in enumerate(cls.FIELDS):
            setattr(st, name, w[HEADER + k * capacity: HEADER + (k + 1) * capacity].view(dt).copy())
        return st

    def copy(self):
        return type(self).from_words(self.words(), self.capacity)

    def same(self, other) -> bool:
        """Bit for bit, ``next_id`` and ``overflow`` included."""
        return self.capacity == other.capacity and bool((self.words() == other.words()).all())


def _align(n: int, a: int = 16) -> int:
    return (n + a - 1) // a * a


class TrackerBase:
    """The device side of a tracker: its own stream, pinned staging and device state; per chunk
    of up to :data:`MAX_FRAMES` frames one H2D of the inputs, one launch and one D2H of the
    outputs.  A subclass names its kernel entry (``ENTRY``) and state class (``STATE``), and
    makes the launch (:meth:`_launch`); :meth:`_extra_inputs` are arrays it stages after
    ``reset``."""
    ENTRY = ""
    STATE = TrackStateBase

    def __init__(self, capacity: int, max_age: int, max_gap: float, device):
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu") if device in (None, "auto") \
            else torch.device(device)
        self.gpu = self.device.type == "cuda" and device_enabled()
        self.capacity, self.max_age, self.max_gap = int(capacity), int(max_age), float(max_gap)
        if self.max_age < 0:
            raise ValueError("max_age: >= 0")
        self.prev_ns: Optional[int] = None
        self.frames = 0
        self._lock = threading.Lock()
        self._host = self.STATE(self.capacity)  # (validates the capacity)
        self._pin_in = self._pin_out = self._dev_in = self._dev_out = self._stream = None
        self._state = None
        if self.gpu:
            with torch.cuda.device(self.device):
                self._stream = torch.cuda.Stream(self.device)
                with torch.cuda.stream(self._stream):
                    self._state = torch.from_numpy(self._host.words()).to(self.device)
                self._stream.synchronize()

    @property
    def kind(self) -> str:
        return self.ENTRY if self.gpu else "host definition"

    def _buf(self, name: str, nbytes: int, pinned: bool) -> torch.Tensor:
        t = getattr(self, name)
        if t is None or t.numel() < nbytes:
            size = max(4096, 1 << (nbytes - 1).bit_length())
            t = torch.empty((size,), dtype=torch.uint8, pin_memory=True) if pinned \
                else torch.empty((size,), dtype=torch.uint8, device=self.device)
            setattr(self, name, t)
        return t

    def _extra_inputs(self) -> List[np.ndarray]:
        return []

    def _launch(self, rows: int, det_off: np.ndarray, n_frames: int, dt: int, reset: int, extra: List[int],
                out: int) -> None:
        """The launch on the staged pointers (``extra``: those of :meth:`_extra_inputs`)."""
        raise NotImplementedError

    def _run_device(self, b) -> List[tuple]:
        """``b``: a batch with ``rows``, ``det_off``, ``dt`` and ``reset``."""
        out: List[tuple] = []
        extra = [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in self._extra_inputs()]
        with torch.cuda.device(self.device):
            st = self._stream
            for f0 in range(0, len(b.dt), MAX_FRAMES):
                f1 = min(len(b.dt), f0 + MAX_FRAMES)
                n0, n1 = int(b.det_off[f0]), int(b.det_off[f1])
                nf, nd = f1 - f0, n1 - n0
                o_dt = _align(32 * max(nd, 1))
                o_reset = o_dt + _align(4 * nf)
                o_extra, total = [], o_reset + _align(nf)
                for a in extra:
                    o_extra.append(total)
                    total += _align(len(a))
                pin = self._buf("_pin_in", total, True)
                host = pin.numpy()
                host[:32 * nd] = b.rows[n0:n1].view(np.uint8).reshape(-1)
                host[o_dt:o_dt + 4 * nf] = b.dt[f0:f1].view(np.uint8)
                host[o_reset:o_reset + nf] = b.reset[f0:f1]
                for o, a in zip(o_extra, extra):
                    host[o:o + len(a)] = a
                dev = self._buf("_dev_in", total, False)
                res = self._buf("_dev_out", 16 * max(nd, 1), False)
                pout = self._buf("_pin_out", 16 * max(nd, 1), True)
                with torch.cuda.stream(st):
                    dev[:total].copy_(pin[:total], non_blocking=True)
                base = dev.data_ptr()
                self._launch(base, b.det_off[f0:f1 + 1] - b.det_off[f0], nf, base + o_dt, base + o_reset,
                             [base + o for o in o_extra], res.data_ptr())
                with torch.cuda.stream(st):
                    pout[:16 * nd].copy_(res[:16 * nd], non_blocking=True)
                st.synchronize()
                w = pout.numpy()[:16 * nd].view(np.int32).reshape(-1, 4).copy()
                for f in range(f0, f1):
                    r = w[int(b.det_off[f]) - n0:int(b.det_off[f + 1]) - n0]
                    out.append((r[:, 0].copy(), r[:, 1].copy(), r[:, 2:4].copy().view(np.float32)))
        return out

    def state(self):
        """The state as host arrays (a copy)."""
        with self._lock:
            if not self.gpu:
                return self._host.copy()
            with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
                w = self._state.cpu().numpy()
            return self.STATE.from_words(w, self.capacity)
