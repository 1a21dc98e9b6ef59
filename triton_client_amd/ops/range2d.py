"""K26 — range camera detections from the LiDAR cloud.

A camera detection is a pixel box; the cloud that arrives next to it knows how far
away the object is.  :func:`range2d_numpy` is the definition, bit for bit (the pattern
of ``ops/points_in_boxes.py``); the HIP kernel ``tca_range2d``
(``csrc/kernels/range2d.hip``) computes the same integers on the device from the raw
``PointCloud2`` payload, and :func:`range2d_ref` is a float64 brute force that also
marks the decisions float32 may legitimately take differently (``docs/precision.md``).

**Calibration.**  :class:`Calibration` holds ``P`` [3, 4] float64, the camera
projection, and ``T`` [4, 4] float64, LiDAR frame → camera optical frame.
``M = float32(P @ T)`` is made once on the host and is the only thing the per-point
code sees.  :func:`load_calibration` reads a YAML file (``projection`` 3x3 or 3x4,
``lidar_to_camera`` 3x4 or 4x4) or a KITTI ``calib/*.txt`` file (``P2``, ``R0_rect``,
``Tr_velo_to_cam``; P = P2 · R0_rect padded).

**Box table**, made on the host (:func:`box_rows`).  Each row comes from a detection's
``bbox`` as float32 ``(cx, cy, sx, sy)``: ``hw = (sx * 0.5f) * shrink``,
``hh = (sy * 0.5f) * shrink``, the row is ``(cx - hw, cy - hh, cx + hw, cy + hh)``, all
NaN if any entry is non-finite or a size is ``<= 0``.  ``shrink`` in (0, 1], default
0.6, keeps the background around the object out of the statistic.

**Per point** ``(x, y, z)`` as sent, every operation rounded to float32 on its own (no
FMA), ``NB = 512`` bins::

    w = ((M20*x + M21*y) + M22*z) + M23
    a = ((M00*x + M01*y) + M02*z) + M03
    b = ((M10*x + M11*y) + M12*z) + M13
    q = w / bin_w                                        # IEEE division
    visible = (w >= min_depth) and (0 <= q < NB)
    bin = int32(q)                                       # truncation
    u = a / w;  v = b / w
    inside(k) = visible and u0 <= u <= u1 and v0 <= v <= v1   # closed edges

``bin_w`` defaults to 0.25 m (ranging reaches 128 m), ``min_depth`` to 0.5 m.  A NaN
compares false.  (``0 <= q`` holds by itself for a positive ``min_depth``; it keeps the
bin inside the histogram for any other.)  A point may lie in several boxes and counts in
each.

**Per box**, integers only: ``n`` is the number of points inside; ``m`` the smallest bin
with ``cum(0..m) * 100 >= n * pct`` in int64 (``pct`` 1..100, default 50), -1 when
``n < min_points`` (default 3); ``c, sx, sy, sz`` the count and the int64 sums, over the
inside points with ``|bin - m| <= window`` (default 1), of
``int32(rint(clamp(x * 1024f, ±2^30)))`` and the same for y and z (explicit comparisons,
half to even).

**Host finish** (:func:`finish`), shared by both paths: the LiDAR-frame mean is
``(sx, sy, sz) / (1024 * c)`` in float64, the camera-frame position
``T[:3, :3] @ mean + T[:3, 3]``.
"""
from __future__ import annotations

import copy
import os
import threading
from collections import deque
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native
from ..ros import msgs
from .cloud_common import CloudLayout, CloudStager, _align, cloud_bytes, cloud_xyzi, fields_f32, flat, plan_staging

NB = 512  # depth bins: kBins in range2d.hip
MAX_FRAMES = 64  # clouds per launch
MAX_BOXES = 512  # boxes per cloud and launch
OUT_INTS = 10  # ints per output record: n, m, c, 0, then sx, sy, sz as int64
FIX = 1024.0
FIX_LIMIT = 2.0 ** 30
INT31 = 2 ** 31
U = 2.0 ** -24  # unit roundoff of float32


def device_enabled() -> bool:
    """``TCA_DEVICE_RANGE=0`` keeps the definition on GPU engines too."""
    return os.environ.get("TCA_DEVICE_RANGE", "1") != "0"


# ------------------------------------------------------------------------- calibration
def _matrix(v, key: str, shapes) -> np.ndarray:
    try:
        a = np.asarray(v, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"calibration key {key!r}: not a numeric matrix") from None
    for rows, cols in shapes:
        if a.shape == (rows, cols):
            break
        if a.ndim == 1 and a.size == rows * cols:
            a = a.reshape(rows, cols)
            break
    else:
        want = " or ".join(f"{r}x{c}" for r, c in shapes)
        raise ValueError(f"calibration key {key!r}: shape {a.shape}, want {want}")
    if not np.isfinite(a).all():
        raise ValueError(f"calibration key {key!r}: non-finite entry")
    return a


def _pad(a: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """``a`` in the top-left corner of the identity-like [rows, cols] matrix."""
    out = np.eye(max(rows, cols))[:rows, :cols].copy()
    out[:a.shape[0], :a.shape[1]] = a
    return out


@dataclass(frozen=True)
class Calibration:
    """``P`` [3, 4]: camera projection; ``T`` [4, 4]: LiDAR frame → camera optical frame."""
    P: np.ndarray
    T: np.ndarray

    def __post_init__(self):
        P = _matrix(self.P, "projection", [(3, 4), (3, 3)])
        T = _matrix(self.T, "lidar_to_camera", [(4, 4), (3, 4)])
        if P.shape == (3, 3):
            P = np.concatenate([P, np.zeros((3, 1))], 1)
        object.__setattr__(self, "P", P)
        object.__setattr__(self, "T", _pad(T, 4, 4) if T.shape == (3, 4) else T)

    @property
    def M(self) -> np.ndarray:
        """[3, 4] float32: all the per-point code sees."""
        return np.ascontiguousarray((self.P @ self.T).astype(np.float32))


def load_calibration(path: str) -> Calibration:
    """A YAML file with ``projection`` and ``lidar_to_camera``, or a KITTI ``calib/*.txt``
    with ``P2:``, ``R0_rect:`` and ``Tr_velo_to_cam:`` lines.  ``ValueError`` names the key of
    a missing, misshapen or non-finite matrix."""
    with open(path) as f:
        text = f.read()
    kitti = {}
    for line in text.splitlines():
        key, sep, rest = line.partition(":")
        if sep and key.strip() in ("P2", "R0_rect", "Tr_velo_to_cam"):
            try:
                kitti[key.strip()] = [float(t) for t in rest.split()]
            except ValueError:
                raise ValueError(f"calibration key {key.strip()!r}: not numbers") from None
    if "P2" in kitti or "Tr_velo_to_cam" in kitti:
        for key in ("P2", "R0_rect", "Tr_velo_to_cam"):
            if key not in kitti:
                raise ValueError(f"calibration key {key!r} is missing in {path}")
        P2 = _matrix(kitti["P2"], "P2", [(3, 4)])
        R0 = _matrix(kitti["R0_rect"], "R0_rect", [(3, 3)])
        Tr = _matrix(kitti["Tr_velo_to_cam"], "Tr_velo_to_cam", [(3, 4)])
        return Calibration(P2 @ _pad(R0, 4, 4), _pad(Tr, 4, 4))
    import yaml

    doc = yaml.safe_load(text)
    if not isinstance(doc, dict):
        raise ValueError(f"calibration key 'projection' is missing in {path}")
    for key in ("projection", "lidar_to_camera"):
        if key not in doc:
            raise ValueError(f"calibration key {key!r} is missing in {path}")
    P = _matrix(doc["projection"], "projection", [(3, 4), (3, 3)])
    T = _matrix(doc["lidar_to_camera"], "lidar_to_camera", [(4, 4), (3, 4)])
    return Calibration(P, T)


# ----------------------------------------------------------------------------- options
@dataclass(frozen=True)
class RangeOptions:
    shrink: float = 0.6
    pct: int = 50
    min_points: int = 3
    bin_w: float = 0.25
    min_depth: float = 0.5
    window: int = 1

    def __post_init__(self):
        if not (0.0 < float(self.shrink) <= 1.0):
            raise ValueError(f"shrink must lie in (0, 1], got {self.shrink}")
        if int(self.pct) != self.pct or not 1 <= self.pct <= 100:
            raise ValueError(f"pct must be an integer in 1..100, got {self.pct}")
        if int(self.min_points) != self.min_points or self.min_points < 1:
            raise ValueError(f"min_points must be an integer >= 1, got {self.min_points}")
        if int(self.window) != self.window or self.window < 0:
            raise ValueError(f"window must be an integer >= 0, got {self.window}")
        if not (np.isfinite(np.float32(self.bin_w)) and np.float32(self.bin_w) > 0):
            raise ValueError(f"bin_w must be finite and positive, got {self.bin_w}")
        if not np.isfinite(np.float32(self.min_depth)):
            raise ValueError(f"min_depth must be finite, got {self.min_depth}")


# ------------------------------------------------------------------------- definition
def bbox_array(detections) -> np.ndarray:
    """[K, 4] float32 ``(cx, cy, sx, sy)`` of a ``Detection2DArray``'s detections (or of the
    rows of an array given as such)."""
    if isinstance(detections, np.ndarray):
        return np.ascontiguousarray(detections, np.float32).reshape(-1, 4)
    dets = getattr(detections, "detections", detections)
    out = np.zeros((len(dets), 4), np.float32)
    with np.errstate(over="ignore"):
        for i, d in enumerate(dets):
            b = d.bbox
            out[i] = (b.center.x, b.center.y, b.size_x, b.size_y)
    return out


def box_rows(boxes, shrink: float = 0.6) -> np.ndarray:
    """[K, 4] float32 rows ``(u0, v0, u1, v1)`` of boxes [K, 4] ``(cx, cy, sx, sy)``; all NaN
    for a box that contains nothing (a non-finite entry, a size <= 0)."""
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
    s = np.float32(shrink)
    with np.errstate(invalid="ignore", over="ignore"):
        hw = (b[:, 2] * np.float32(0.5)) * s
        hh = (b[:, 3] * np.float32(0.5)) * s
        t = np.stack([b[:, 0] - hw, b[:, 1] - hh, b[:, 0] + hw, b[:, 1] + hh], 1).astype(np.float32)
        bad = ~np.isfinite(b).all(1) | (b[:, 2:] <= 0).any(1)
    t[bad] = np.nan
    return np.ascontiguousarray(t.reshape(-1, 4))


def _xyz(points) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    p = np.asarray(points, np.float32)
    p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)
    return tuple(np.ascontiguousarray(p[:, j]) for j in range(3))


def fixed_point(x: np.ndarray) -> np.ndarray:
    """``int32(rint(clamp(x * 1024f, ±2^30)))`` of float32 ``x`` (finite: the coordinates of an
    inside point always are); a non-finite value gives 0 here and is never summed."""
    x = np.asarray(x, np.float32)
    lim = np.float32(FIX_LIMIT)
    with np.errstate(over="ignore", invalid="ignore"):
        t = x * np.float32(FIX)
        t = np.where(t > lim, lim, np.where(t < -lim, -lim, t)).astype(np.float32)
        t = np.where(np.isfinite(t), t, np.float32(0))
    return np.rint(t).astype(np.int32)


def _reduce(inside: np.ndarray, bins: np.ndarray, fx: np.ndarray, pct: int, min_points: int, window: int):
    """The integer part of the definition, from an [N, K] inside matrix, [N] bins and the
    [N, 3] fixed-point coordinates → ``(n, m, c, sums)``."""
    k = inside.shape[1]
    n = np.zeros(k, np.int32)
    m = np.full(k, -1, np.int32)
    c = np.zeros(k, np.int32)
    sums = np.zeros((k, 3), np.int64)
    fx64 = fx.astype(np.int64)
    for j in range(k):
        idx = np.nonzero(inside[:, j])[0]
        n[j] = len(idx)
        if len(idx) < min_points:
            continue
        bj = bins[idx]
        cum = np.cumsum(np.bincount(bj, minlength=NB).astype(np.int64))
        m[j] = int(np.nonzero(cum * 100 >= np.int64(len(idx)) * np.int64(pct))[0][0])
        near = idx[np.abs(bj.astype(np.int64) - int(m[j])) <= window]
        c[j] = len(near)
        sums[j] = fx64[near].sum(0)
    return n, m, c, sums


def project_uvw(points, M):
    """``(u, v, w)`` of every point, float32 in the definition's operation order (shared with
    ``ops/depth_image.py``)."""
    x, y, z = _xyz(points)
    M = np.asarray(M, np.float32).reshape(3, 4)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = ((M[2, 0] * x + M[2, 1] * y) + M[2, 2] * z) + M[2, 3]
        a = ((M[0, 0] * x + M[0, 1] * y) + M[0, 2] * z) + M[0, 3]
        b = ((M[1, 0] * x + M[1, 1] * y) + M[1, 2] * z) + M[1, 3]
        return a / w, b / w, w


def project_numpy(points, M, bin_w: float = 0.25, min_depth: float = 0.5):
    """The per-point part of the definition → ``(u, v, visible, bin)``."""
    u, v, w = project_uvw(points, M)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = w / np.float32(bin_w)
        visible = (w >= np.float32(min_depth)) & (q >= np.float32(0)) & (q < np.float32(NB))
        bins = np.where(visible, q, np.float32(0)).astype(np.int32)
    return u, v, visible, bins


def range2d_numpy(points, rows, M, pct: int = 50, min_points: int = 3, bin_w: float = 0.25,
                  min_depth: float = 0.5, window: int = 1, return_inside: bool = False):
    """→ ``(n [K] int32, m [K] int32, c [K] int32, sums [K, 3] int64)`` (and the ``[N, K]``
    inside matrix and the ``[N]`` bins): the definition.  ``points`` [N, >=3] (x, y, z);
    ``rows`` [K, 4] from :func:`box_rows`; ``M`` [3, 4] float32."""
    x, y, z = _xyz(points)
    rows = np.asarray(rows, np.float32).reshape(-1, 4)
    u, v, visible, bins = project_numpy(np.stack([x, y, z], 1), M, bin_w, min_depth)
    inside = np.zeros((len(x), len(rows)), bool)
    with np.errstate(invalid="ignore"):
        for j, r in enumerate(rows):
            inside[:, j] = visible & (r[0] <= u) & (u <= r[2]) & (r[1] <= v) & (v <= r[3])
    fx = np.stack([fixed_point(x), fixed_point(y), fixed_point(z)], 1)
    res = _reduce(inside, bins, fx, int(pct), int(min_points), int(window))
    return res + (inside, bins) if return_inside else res


def range2d_ref(points, rows, M, pct: int = 50, min_points: int = 3, bin_w: float = 0.25,
                min_depth: float = 0.5, window: int = 1):
    """Float64 brute force → ``(n, m, c, sums, inside [N, K], bins [N], band [N, K] bool,
    bin_band [N] bool)``.

    ``band`` marks the (point, box) pairs and ``bin_band`` the points whose decision the
    float32 evaluation may legitimately take differently.  With ``S_a`` the sum of the
    absolute terms of ``a`` (``|M00 x| + |M01 y| + |M02 z| + |M03|``; ``S_b``, ``S_w``
    alike), the float32 dot product is within ``4u S`` of the exact one (the first product
    passes four roundings), so ``u = a / w`` is within
    ``eu = 5 * 2**-24 * (S_a + |u| S_w) / |w| + 2 * 2**-24 * |u|`` of the exact pixel (one
    more ``u`` in the factor for the second-order terms, the last term for the division's
    own rounding), ``w`` within ``ew = 5 * 2**-24 * S_w`` and ``q`` within
    ``ew / bin_w + 2**-24 * |q|``.  A pair is in the band when ``u`` or ``v`` is that close
    to an edge of the row, or ``w`` that close to ``min_depth``, or ``q`` to ``NB``; a point's
    bin when ``q`` is that close to an integer.  ``docs/precision.md`` has the derivation.
    The rows and ``M`` are float32 inputs of both evaluations and exact here."""
    x, y, z = (c.astype(np.float64) for c in _xyz(points))
    rows64 = np.asarray(rows, np.float32).reshape(-1, 4).astype(np.float64)
    M64 = np.asarray(M, np.float32).reshape(3, 4).astype(np.float64)
    bw, md = float(np.float32(bin_w)), float(np.float32(min_depth))

    def dot(r):
        t = (M64[r, 0] * x, M64[r, 1] * y, M64[r, 2] * z, M64[r, 3])
        return t[0] + t[1] + t[2] + t[3], np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2]) + np.abs(t[3])

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        (w, Sw), (a, Sa), (b, Sb) = dot(2), dot(0), dot(1)
        q = w / bw
        visible = (w >= md) & (q >= 0) & (q < NB)
        bins = np.where(visible, q, 0.0).astype(np.int32)
        u, v = a / w, b / w
        aw = np.abs(w)
        eu = 5 * U * (Sa + np.abs(u) * Sw) / aw + 2 * U * np.abs(u)
        ev = 5 * U * (Sb + np.abs(v) * Sw) / aw + 2 * U * np.abs(v)
        ew = 5 * U * Sw
        eq = ew / bw + U * np.abs(q)
        vis_band = (np.abs(w - md) <= ew) | (np.abs(q - NB) <= eq) | (np.abs(q) <= eq)
        frac = q - np.floor(q)
        bin_band = (visible | vis_band) & ((frac <= eq) | (1.0 - frac <= eq))
        n_pts, k = len(x), len(rows64)
        inside = np.zeros((n_pts, k), bool)
        band = np.zeros((n_pts, k), bool)
        for j, r in enumerate(rows64):
            if not np.isfinite(r).all():
                continue
            in_u = (r[0] <= u) & (u <= r[2])
            in_v = (r[1] <= v) & (v <= r[3])
            inside[:, j] = visible & in_u & in_v
            near_u = (np.abs(u - r[0]) <= eu) | (np.abs(u - r[2]) <= eu)
            near_v = (np.abs(v - r[1]) <= ev) | (np.abs(v - r[3]) <= ev)
            # near an edge in one axis matters only while the other axis does not already exclude
            band[:, j] = ((visible | vis_band) & ((near_u & (in_v | near_v)) | (near_v & (in_u | near_u)))) \
                | (vis_band & (in_u | near_u) & (in_v | near_v))
    fx = np.stack([fixed_point(c) for c in _xyz(points)], 1)
    n, m, c, sums = _reduce(inside, bins, fx, int(pct), int(min_points), int(window))
    return n, m, c, sums, inside, bins, band, bin_band


def finish(m: np.ndarray, c: np.ndarray, sums: np.ndarray, T: np.ndarray):
    """→ ``(ranged [K] bool, lidar [K, 3] float64, camera [K, 3] float64)``: the LiDAR-frame mean
    ``sums / (1024 * c)`` and its camera-frame position, zeros where the box got no range."""
    m, c = np.asarray(m), np.asarray(c).astype(np.int64)
    ok = (m >= 0) & (c > 0)
    mean = np.zeros((len(m), 3), np.float64)
    mean[ok] = np.asarray(sums, np.int64)[ok].astype(np.float64) / (FIX * c[ok])[:, None]
    T = np.asarray(T, np.float64)
    cam = np.zeros_like(mean)
    cam[ok] = mean[ok] @ T[:3, :3].T + T[:3, 3]
    return ok, mean, cam


def ranged_message(camera_msg, cam: np.ndarray, ok: np.ndarray) -> msgs.Detection2DArray:
    """The camera message with its ranges: the same header, detections, order, bboxes and
    hypotheses; ``results[0].pose.position`` is the camera-frame position (zero without a
    range); a detection without a hypothesis gets one with id 0 and score 0."""
    out = msgs.Detection2DArray(header=camera_msg.header)
    for d, p, good in zip(camera_msg.detections, cam, ok):
        res = [copy.copy(r) for r in d.results] or [msgs.ObjectHypothesisWithPose(id=0, score=0.0)]
        pos = msgs.Point(float(p[0]), float(p[1]), float(p[2])) if good else msgs.Point()
        res[0] = msgs.ObjectHypothesisWithPose(id=res[0].id, score=res[0].score,
                                               pose=msgs.Pose(pos, res[0].pose.orientation))
        out.detections.append(msgs.Detection2D(header=d.header, results=res, bbox=d.bbox, source_img=d.source_img))
    return out


# ----------------------------------------------------------------------------- pairing
def _nsec(stamp) -> int:
    if hasattr(stamp, "to_nsec"):
        return int(stamp.to_nsec())
    if hasattr(stamp, "secs"):
        return int(stamp.secs) * 1_000_000_000 + int(stamp.nsecs)
    return int(round(float(stamp) * 1e9))


class StampPairer:
    """Holds the last ``capacity`` messages of one topic (the oldest arrival leaves first) and
    answers which of them is nearest in time to a stamp."""

    def __init__(self, capacity: int = 64):
        if capacity < 1:
            raise ValueError("capacity must be >= 1")
        self._held = deque(maxlen=int(capacity))
        self._lock = threading.Lock()

    def __len__(self) -> int:
        return len(self._held)

    def push(self, msg) -> None:
        with self._lock:
            self._held.append((_nsec(msg.header.stamp), msg))

    def nearest(self, stamp, slop: float = 0.05):
        """The held message with the smallest ``|Δt| <= slop`` (seconds) to ``stamp``, None
        without one; a tie goes to the earlier stamp."""
        t, lim = _nsec(stamp), int(round(float(slop) * 1e9))
        best = None
        with self._lock:
            for s, m in self._held:
                d = abs(s - t)
                if d <= lim and (best is None or (d, s) < best[:2]):
                    best = (d, s, m)
        return None if best is None else best[2]


# --------------------------------------------------------------------------------- GPU
@dataclass
class RangeCall:
    """One prepared launch: device views of its inputs, workspace and output."""
    data: torch.Tensor
    data_bytes: int
    frame_off: torch.Tensor
    frame_n: torch.Tensor
    table: torch.Tensor
    hist: torch.Tensor
    out: torch.Tensor
    box_off: np.ndarray  # host int32 [B + 1]
    M: np.ndarray  # host float32 [12]
    layout: CloudLayout
    batch: int
    max_n: int
    n_boxes: int
    opts: RangeOptions = field(default_factory=RangeOptions)


def launch(c: RangeCall, stream=None) -> None:
    """The launch alone (workspace zeroing and the three kernels on ``stream``): no
    allocation, no copy, no sync."""
    p = _native.ptr
    o, r = c.layout.offsets, c.opts
    _native.call("tca_range2d", p(c.data), c.data_bytes, p(c.frame_off), p(c.frame_n), c.batch, c.max_n,
                 c.layout.point_step, o[0], o[1], o[2], c.box_off.ctypes.data, p(c.table), c.M.ctypes.data,
                 float(r.bin_w), float(r.min_depth), int(r.pct), int(r.min_points), int(r.window), p(c.hist),
                 p(c.out), _native.stream_ptr(stream))


def unpack(out: np.ndarray, k: int):
    """``(n, m, c, sums)`` of ``k`` output records (host bytes or int32 words)."""
    w = np.ascontiguousarray(out).view(np.int32)[:k * OUT_INTS].reshape(k, OUT_INTS)
    sums = np.ascontiguousarray(w[:, 4:]).view(np.int64).reshape(k, 3)
    return w[:, 0].copy(), w[:, 1].copy(), w[:, 2].copy(), sums.copy()


def layout_device_ok(lay: CloudLayout) -> bool:
    """What ``tca_range2d`` reads in place: little-endian FLOAT32 x, y, z inside the record."""
    return fields_f32(lay, (0, 1, 2))


class CameraRanger(CloudStager):
    """Ranges pixel boxes against clouds: on a GPU with ``tca_range2d`` (its own workspace,
    stream and pinned staging: one H2D of payloads and rows, one launch, one D2H of the
    per-box integers per batch of same-layout clouds), on the CPU — and with
    ``TCA_DEVICE_RANGE=0`` — with the definition.  Clouds the kernel does not take
    (non-FLOAT32 or big-endian fields, more than 512 boxes) run the definition with one
    warning."""

    @staticmethod
    def sections(rows: Sequence[np.ndarray]) -> list:
        """What a batch stages after ``frame_off`` and ``frame_n``."""
        return [("table", flat(rows, np.float32))]

    def prepare(self, payloads: Sequence, ns: Sequence[int], layout: CloudLayout, rows: Sequence[np.ndarray], M,
                opts: Optional[RangeOptions] = None, stream=None, misalign: int = 0) -> RangeCall:
        """Stage one batch (``payloads[b]``: the bytes of ``ns[b]`` points of ``layout``;
        ``rows[b]``: frame b's :func:`box_rows`) in pinned memory and upload it with one H2D
        copy on ``stream``.  ``misalign``: start every payload this many bytes past a 16-byte
        boundary."""
        if not layout_device_ok(layout):
            raise ValueError(f"tca_range2d does not take this layout: {layout}")
        B = len(payloads)
        ns = [int(n) for n in ns]
        nb = [len(t) for t in rows]
        K = sum(nb)
        data_bytes = plan_staging(ns, layout.point_step, misalign, ()).data_bytes  # (refused before any allocation)
        if data_bytes >= INT31:
            raise ValueError(f"{data_bytes} payload bytes do not fit one call: split the batch")
        dev, _, view = self._stage("r2d_in", payloads, ns, layout.point_step, misalign, self.sections(rows), stream)
        hist = self._device_buf("r2d_hist", 4 * NB * max(K, 1))
        out = self._device_buf("r2d_out", 4 * OUT_INTS * max(K, 1))
        return RangeCall(data=dev, data_bytes=data_bytes, frame_off=view("frame_off", B, torch.int64),
                         frame_n=view("frame_n", B, torch.int32), table=view("table", 4 * K, torch.float32),
                         hist=hist.view(torch.int32), out=out, layout=layout, batch=B, max_n=max(ns, default=0),
                         n_boxes=K, box_off=np.concatenate([[0], np.cumsum(nb)]).astype(np.int32),
                         M=np.ascontiguousarray(M, np.float32).reshape(12), opts=opts or RangeOptions())

    launch = staticmethod(launch)

    def _run_device(self, payloads, ns, layout, rows, M, opts):
        """→ per frame ``(n, m, c, sums)``."""
        with torch.cuda.device(self.device):
            st = self._own_stream()
            c = self.prepare(payloads, ns, layout, rows, M, opts, st)
            if c.n_boxes:
                launch(c, st)
                host = self._fetch(c.out, 4 * OUT_INTS * c.n_boxes, st)
            else:  # nothing to range: no launch, no D2H
                st.synchronize()
                host = np.zeros(0, np.int32)
        n, m, cc, sums = unpack(host, c.n_boxes)
        out, ko = [], 0
        for t in rows:
            k = len(t)
            out.append((n[ko:ko + k], m[ko:ko + k], cc[ko:ko + k], sums[ko:ko + k]))
            ko += k
        return out

    def _parts(self, idx, clouds):
        return _launch_groups(idx, [len(clouds[i].data) for i in idx])

    # ---------------------------------------------------------------------- API
    def range(self, clouds: Sequence, rows: Sequence[np.ndarray], M, opts: Optional[RangeOptions] = None) -> List[tuple]:
        """Per cloud ``(n, m, c, sums)`` of its ``rows[b]`` (:func:`box_rows`) under ``M``."""
        opts = opts or RangeOptions()
        return self._per_cloud(
            clouds, lambda i, lay: layout_device_ok(lay) and len(rows[i]) <= MAX_BOXES,
            lambda i, lay: range_numpy(clouds[i], rows[i], M, opts, lay),
            lambda lay, part: (*cloud_bytes(clouds, part), lay, [rows[i] for i in part], M, opts), self._run_device,
            lambda i, lay: f"CameraRanger: tca_range2d takes little-endian FLOAT32 x, y, z and at most {MAX_BOXES} "
                           f"boxes per cloud (got {lay}, {len(rows[i])} boxes); such clouds are ranged on the host",
            device=self.gpu and device_enabled())


def _launch_groups(idx: Sequence[int], nbytes: Sequence[int]):
    """``idx`` cut into runs of at most 64 clouds and less than 2^31 staged bytes."""
    part, size = [], 0
    for i, nb in zip(idx, nbytes):
        nb = _align(nb) + 16
        if part and (len(part) == MAX_FRAMES or size + nb >= INT31):
            yield part
            part, size = [], 0
        part.append(i)
        size += nb
    if part:
        yield part


def range_numpy(cloud, rows, M, opts: Optional[RangeOptions] = None, lay: Optional[CloudLayout] = None) -> tuple:
    """One cloud through the definition → ``(n, m, c, sums)``."""
    o = opts or RangeOptions()
    return range2d_numpy(cloud_xyzi(cloud, lay), rows, M, o.pct, o.min_points, o.bin_w, o.min_depth, o.window)
