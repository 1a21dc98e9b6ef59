"""K29 — the cloud as a 2D ``sensor_msgs/LaserScan``.

The side outputs so far serve perception and visualisation; this one feeds 2D navigation
(``amcl``, ``gmapping``, ``slam_toolbox``, a costmap): per angular bin around the sensor's z axis
the range of the nearest return in a height band, what ROS's ``pointcloud_to_laserscan`` node
computes from the same cloud on a CPU core.  :func:`scan_numpy` is the definition, bit for bit (the
pattern of ``ops/depth_image.py``); the HIP kernel ``tca_laser_scan``
(``csrc/kernels/laser_scan.hip``) computes the same bytes on the device from the raw
``PointCloud2`` payload, and :func:`scan_ref` is a float64 brute force with true ``atan2`` that
also marks the decisions float32 may legitimately take differently (``docs/precision.md``).

:class:`ScanOptions` carries ``pointcloud_to_laserscan``'s parameters under their names and with
their defaults: ``angle_min`` / ``angle_max`` (within [-pi, pi]), ``angle_increment``,
``min_height`` / ``max_height`` (against ``z`` in the cloud's own frame), ``range_min`` /
``range_max``, ``use_inf``, ``inf_epsilon`` and ``scan_time``.  The scan has
``n = ceil((angle_max - angle_min) / angle_increment)`` bins, 1..4096 (float64, with 1e-9 of slack
against a bin born of rounding).

**The bin of a point** needs no ``atan2`` (NumPy's and the device's are not the same function): a
pseudo-angle that is monotone in the true angle and takes one IEEE add, divide and subtract.  In
float32, every operation rounded on its own (no FMA)::

    s = |x| + |y|                      # s == 0 or not finite: the point is dropped
    q = copysign(1 - x / s, y)         # in [-2, 2]: 0 ahead, 1 left, +-2 behind, -1 right

(``y = -0.0`` is "right of behind", as for ``atan2``.)  The host builds the table of bin edges once
per options, in float64: ``e_k = min(angle_min + k * angle_increment, angle_max)`` for
``k = 0..n`` and ``t_k = float32(pseudo64(cos e_k, sin e_k))``, which is non-decreasing.  Then
``bin = searchsorted(t, q, side="right") - 1``; ``q == t_n`` belongs to bin ``n - 1`` (a return
exactly behind the sensor is kept on a full circle), and ``q < t_0`` or ``q > t_n`` has no bin.

**Per point** ``(x, y, z)`` as sent.  The point is valid iff (a NaN compares false)
``min_height <= z <= max_height``, ``range_min <= r <= range_max`` with ``r2 = x * x + y * y`` and
``r = sqrt(r2)`` (correctly rounded), and it has a bin.

**Per bin** the result is the smallest ``r`` over its valid points (positive floats order as
their bits, so an integer minimum does it); nothing depends on the order of the points.  An empty
bin holds ``+inf`` (bits ``0x7F800000``), or ``float32(range_max + inf_epsilon)`` with
``use_inf`` False.  The output is ``<f4 [n]``.

Not here: ``target_frame`` and tf (the scan is in the cloud's frame), ``intensities`` (left empty,
as the ROS node leaves them) and ray-cast free space.
"""
from __future__ import annotations

import functools
import math
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import _native
from ..ros import msgs
from .cloud_common import CloudLayout, CloudStager, _align, cloud_bytes, cloud_xyzi, fields_f32, plan_staging
from .range2d import INT31, U, _xyz

MAX_FRAMES = 64  # clouds per launch
MAX_BINS = 4096
EMPTY = 0xFFFFFFFF  # the key of a bin no point fell into
INF_BITS = 0x7F800000
EDGE_BAND = 8 * U  # scan_ref: how near an edge of its bin a point's pseudo-angle may be taken either way
GATE_BAND = 3 * U  # scan_ref: the same for r against a range limit, relative


def device_enabled() -> bool:
    """``TCA_DEVICE_SCAN=0`` keeps the definition on GPU engines too."""
    return os.environ.get("TCA_DEVICE_SCAN", "1") != "0"


# ----------------------------------------------------------------------------- options
def _number(name, v, finite=True):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, got {v!r}")
    v = float(v)
    if math.isnan(v) or (finite and math.isinf(v)):
        raise ValueError(f"{name} must be {'finite' if finite else 'a number, not NaN'}, got {v!r}")
    return v


@dataclass(frozen=True)
class ScanOptions:
    angle_min: float = -math.pi
    angle_max: float = math.pi
    angle_increment: float = math.pi / 180.0
    min_height: float = -1.0
    max_height: float = 1.0
    range_min: float = 0.45
    range_max: float = 100.0
    use_inf: bool = True
    inf_epsilon: float = 1.0
    scan_time: float = 1.0 / 30.0

    def __post_init__(self):
        lo, hi = _number("angle_min", self.angle_min), _number("angle_max", self.angle_max)
        for name, v in (("angle_min", lo), ("angle_max", hi)):
            if not -math.pi <= v <= math.pi:
                raise ValueError(f"{name} must be within [-pi, pi], got {v!r}")
        if not lo < hi:
            raise ValueError(f"angle_min must be less than angle_max, got {lo!r} >= {hi!r}")
        inc = _number("angle_increment", self.angle_increment)
        if not inc > 0:
            raise ValueError(f"angle_increment must be positive, got {inc!r}")
        n = (hi - lo) / inc
        if not n - 1e-9 <= MAX_BINS:
            raise ValueError(f"angle_increment gives {n:.6g} bins, want 1..{MAX_BINS}")
        h0, h1 = _number("min_height", self.min_height, False), _number("max_height", self.max_height, False)
        if not h0 <= h1:
            raise ValueError(f"min_height must not exceed max_height, got {h0!r} > {h1!r}")
        r0, r1 = _number("range_min", self.range_min), _number("range_max", self.range_max)
        if not r0 >= 0:
            raise ValueError(f"range_min must be >= 0, got {r0!r}")
        with np.errstate(over="ignore"):
            f0, f1 = np.float32(r0), np.float32(r1)
        if not (np.isfinite(f1) and f0 < f1):
            raise ValueError(f"range_min must be less than range_max in float32, got {r0!r} and {r1!r}")
        if not isinstance(self.use_inf, (bool, np.bool_)):
            raise ValueError(f"use_inf must be a bool, got {self.use_inf!r}")
        eps = _number("inf_epsilon", self.inf_epsilon)
        with np.errstate(over="ignore"):
            if not (eps > 0 and np.isfinite(np.float32(r1 + eps))):
                raise ValueError(f"inf_epsilon must be positive and range_max + inf_epsilon finite, got {eps!r}")
        if not _number("scan_time", self.scan_time) >= 0:
            raise ValueError(f"scan_time must be >= 0, got {self.scan_time!r}")

    @property
    def n(self) -> int:
        """The number of bins."""
        return max(1, math.ceil((float(self.angle_max) - float(self.angle_min)) / float(self.angle_increment) - 1e-9))

    @property
    def empty(self) -> np.float32:
        """What a bin without a return holds."""
        return np.float32(np.inf) if self.use_inf else np.float32(float(self.range_max) + float(self.inf_epsilon))

    @property
    def empty_bits(self) -> int:
        return int(np.asarray(self.empty, "<f4").view("<u4"))

    @property
    def limits(self) -> np.ndarray:
        """``float32 [min_height, max_height, range_min, range_max]``: what the per-point code compares with."""
        return np.array([self.min_height, self.max_height, self.range_min, self.range_max], np.float32)


def pseudo64(c, s):
    """The pseudo-angle of direction ``(c, s)`` in float64: ``copysign(1 - c / (|c| + |s|), s)``."""
    c, s = np.asarray(c, np.float64), np.asarray(s, np.float64)
    return np.copysign(1.0 - c / (np.abs(c) + np.abs(s)), s)


def edge_angles(opts: ScanOptions) -> np.ndarray:
    """``e_k`` float64 ``[n + 1]``: the bins' edges as angles."""
    return np.minimum(float(opts.angle_min) + np.arange(opts.n + 1, dtype=np.float64) * float(opts.angle_increment),
                      float(opts.angle_max))


@functools.lru_cache(maxsize=64)
def edge_table(opts: ScanOptions) -> np.ndarray:
    """``t_k`` float32 ``[n + 1]``: the bins' edges as pseudo-angles (made once per options; read-only)."""
    e = edge_angles(opts)
    t = pseudo64(np.cos(e), np.sin(e)).astype(np.float32)
    assert (np.diff(t) >= 0).all(), "the edge table must not decrease"
    t.setflags(write=False)
    return t


# ------------------------------------------------------------------------- definition
def pseudo_bins(x, y, t):
    """The bin rule on float32 ``x``, ``y`` against an edge table ``t`` float32 ``[n + 1]`` →
    ``(bin [N] int64, has [N] bool)``: ``searchsorted(t, q, "right") - 1`` with ``q == t_n`` in bin
    ``n - 1``; ``has`` iff ``s`` is finite and non-zero and ``t_0 <= q <= t_n`` (``bin`` means
    nothing elsewhere).  Shared with the ground splitter's sectors (``ops/ground.py``, K30)."""
    n = len(t) - 1
    one = np.float32(1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = np.abs(x) + np.abs(y)
        ok = np.isfinite(s) & (s != 0)
        q = np.copysign(one - x / np.where(ok, s, one), y).astype(np.float32)
        b = np.searchsorted(t, np.where(ok, q, np.float32(0)), side="right").astype(np.int64) - 1
        b = np.where(q == t[n], n - 1, b)
        has = ok & (q >= t[0]) & (q <= t[n])
    return b, has


def scan_keys_numpy(points, opts: ScanOptions):
    """The per-point half of the definition → ``(bin [N] int32, valid [N] bool, r [N] float32)``;
    ``bin`` is -1 where the point has none."""
    x, y, z = _xyz(points)
    h0, h1, r0, r1 = opts.limits
    b, has = pseudo_bins(x, y, edge_table(opts))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = np.sqrt(x * x + y * y).astype(np.float32)
        valid = has & (z >= h0) & (z <= h1) & (r >= r0) & (r <= r1)
    return np.where(has, b, -1).astype(np.int32), valid, r


def ranges_of_keys(keys: np.ndarray, opts: ScanOptions) -> np.ndarray:
    """The key row (uint32 [n], ``EMPTY`` where nothing fell) as the scan's ranges."""
    return np.where(keys == EMPTY, np.uint32(opts.empty_bits), keys).astype("<u4").view("<f4")


def scan_numpy(points, opts: ScanOptions) -> np.ndarray:
    """→ the scan's ``ranges`` ``<f4 [n]``: the definition.  ``points`` [N, >=3] (x, y, z)."""
    b, valid, r = scan_keys_numpy(points, opts)
    keys = np.full(opts.n, EMPTY, np.uint32)
    np.minimum.at(keys, b[valid], r[valid].view(np.uint32))
    return ranges_of_keys(keys, opts)


def scan_ref(points, opts: ScanOptions):
    """Float64 brute force of the per-point half with true ``atan2`` → ``(bin [N] int32 (-1: none),
    valid [N] bool, r [N] float64, edge_band [N] bool, gate_band [N] bool)``:
    ``bin = floor((atan2(y, x) - angle_min) / angle_increment)`` for an angle in
    ``[angle_min, angle_max]`` (``angle_max`` itself in bin ``n - 1``).

    The bands mark the points whose float32 decision may legitimately differ.  ``edge_band``: the
    point's float64 pseudo-angle lies within ``8 * 2**-24`` of the float64 pseudo-angle of either
    edge of its bin (of either end of the scan for a point outside it): the roundings of ``s``,
    the division, the subtraction and the table entry.  ``gate_band``: ``r`` lies within
    ``3 * 2**-24 * r`` of a range limit; ``z`` is compared exactly on both sides and raises no
    band.  ``docs/precision.md`` has the derivation.  The limits are float32 inputs of both
    evaluations and exact here."""
    x, y, z = (c.astype(np.float64) for c in _xyz(points))
    n = opts.n
    h0, h1, r0, r1 = (float(v) for v in opts.limits)
    lo, hi, inc = float(opts.angle_min), float(opts.angle_max), float(opts.angle_increment)
    e = edge_angles(opts)
    t64 = pseudo64(np.cos(e), np.sin(e))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = np.abs(x) + np.abs(y)
        ok = np.isfinite(s) & (s != 0)
        a = np.arctan2(y, x)
        has = ok & (a >= lo) & (a <= hi)
        b = np.clip(np.floor((np.where(has, a, lo) - lo) / inc), 0, n - 1).astype(np.int64)
        r = np.sqrt(x * x + y * y)
        gate = (z >= h0) & (z <= h1) & (r >= r0) & (r <= r1)
        q = np.where(ok, pseudo64(x, np.where(ok, y, 1.0)), np.nan)
        left, right = np.where(has, t64[b], t64[0]), np.where(has, t64[b + 1], t64[n])
        edge_band = ok & ((np.abs(q - left) <= EDGE_BAND) | (np.abs(q - right) <= EDGE_BAND))
        gate_band = ok & ((np.abs(r - r0) <= GATE_BAND * r) | (np.abs(r - r1) <= GATE_BAND * r))
    return np.where(has, b, -1).astype(np.int32), has & gate, r, edge_band, gate_band


def scan_message(cloud, ranges: np.ndarray, opts: ScanOptions, frame_id: str = "") -> msgs.LaserScan:
    """The ranges as a ``sensor_msgs/LaserScan`` with the cloud's stamp and seq, in frame
    ``frame_id`` (the cloud's when empty); the options as the float32 the wire carries,
    ``angle_max`` as given, ``time_increment`` 0 and no intensities."""
    h = cloud.header
    a = np.ascontiguousarray(ranges, "<f4").reshape(-1)
    if a.shape != (opts.n,):
        raise ValueError(f"{a.shape[0]} ranges, want {opts.n}")

    def f32(v):
        return float(np.float32(v))

    return msgs.LaserScan(header=msgs.Header(seq=h.seq, stamp=h.stamp, frame_id=frame_id or h.frame_id),
                          angle_min=f32(opts.angle_min), angle_max=f32(opts.angle_max),
                          angle_increment=f32(opts.angle_increment), time_increment=0.0,
                          scan_time=f32(opts.scan_time), range_min=f32(opts.range_min), range_max=f32(opts.range_max),
                          ranges=a, intensities=np.zeros(0, "<f4"))


# --------------------------------------------------------------------------------- GPU
@dataclass
class ScanCall:
    """One prepared launch: device views of its inputs, workspace and output."""
    data: torch.Tensor
    data_bytes: int
    frame_off: torch.Tensor
    frame_n: torch.Tensor
    table: torch.Tensor  # float32 [n + 1]
    plane: torch.Tensor  # uint8 view of B * n uint32 keys
    out: torch.Tensor  # uint8, the scans' ranges back to back
    layout: CloudLayout
    batch: int
    max_n: int
    opts: ScanOptions

    @property
    def out_bytes(self) -> int:
        return 4 * self.batch * self.opts.n


def launch(c: ScanCall, stream=None, privatise: bool = True) -> None:
    """The launch alone (the plane's reset and the two kernels on ``stream``): no allocation, no
    copy, no sync.  ``privatise`` False: the points kernel without its LDS bins (measurements)."""
    p = _native.ptr
    o, r = c.layout.offsets, c.opts
    h0, h1, r0, r1 = (float(v) for v in r.limits)
    _native.call("tca_laser_scan", p(c.data), c.data_bytes, p(c.frame_off), p(c.frame_n), c.batch, c.max_n,
                 c.layout.point_step, o[0], o[1], o[2], p(c.table), int(r.n), h0, h1, r0, r1, int(r.empty_bits),
                 1 if privatise else 0, p(c.plane), p(c.out), _native.stream_ptr(stream))


def layout_device_ok(lay: CloudLayout) -> bool:
    """What ``tca_laser_scan`` reads in place: little-endian FLOAT32 x, y, z inside the record."""
    return fields_f32(lay, (0, 1, 2))


def ranges_of(host: np.ndarray, batch: int, opts: ScanOptions) -> List[np.ndarray]:
    """The ``batch`` scans of a launch's output bytes, each its own array."""
    a = np.ascontiguousarray(host).view(np.uint8)[:4 * batch * opts.n].view("<f4").reshape(batch, opts.n)
    return [a[b].copy() for b in range(batch)]


class LaserScanner(CloudStager):
    """Turns clouds into scans: on a GPU with ``tca_laser_scan`` (its own workspace, stream and
    pinned staging: one H2D of the payloads and the edge table, one launch, one D2H of the ranges per
    launch group of same-layout clouds), on the CPU — and with ``TCA_DEVICE_SCAN=0`` — with the
    definition.  Clouds the kernel does not take (non-FLOAT32 or big-endian fields) run the
    definition with one warning."""

    def prepare(self, payloads: Sequence, ns: Sequence[int], layout: CloudLayout, opts: ScanOptions, stream=None,
                misalign: int = 0) -> ScanCall:
        """Stage one batch (``payloads[b]``: the bytes of ``ns[b]`` points of ``layout``) and the
        edge table in pinned memory and upload them with one H2D copy on ``stream``.  ``misalign``:
        start every payload this many bytes past a 16-byte boundary."""
        if not layout_device_ok(layout):
            raise ValueError(f"tca_laser_scan does not take this layout: {layout}")
        B = len(payloads)
        ns = [int(n) for n in ns]
        if not 1 <= B <= MAX_FRAMES:
            raise ValueError(f"{B} clouds do not fit one call (1..{MAX_FRAMES}): split the batch")
        data_bytes = plan_staging(ns, layout.point_step, misalign, ()).data_bytes  # (refused before any allocation)
        if data_bytes >= INT31:
            raise ValueError(f"{data_bytes} payload bytes do not fit one call: split the batch")
        n = opts.n
        dev, _, view = self._stage("scan_in", payloads, ns, layout.point_step, misalign,
                                   [("table", edge_table(opts))], stream)
        plane = self._device_buf("scan_plane", 4 * B * n)
        out = self._device_buf("scan_out", 4 * B * n)
        return ScanCall(data=dev, data_bytes=data_bytes, frame_off=view("frame_off", B, torch.int64),
                        frame_n=view("frame_n", B, torch.int32), table=view("table", n + 1, torch.float32),
                        plane=plane, out=out, layout=layout, batch=B, max_n=max(ns, default=0), opts=opts)

    launch = staticmethod(launch)

    def _run_device(self, payloads, ns, layout, opts):
        """→ per frame its ranges."""
        with torch.cuda.device(self.device):
            st = self._own_stream()
            c = self.prepare(payloads, ns, layout, opts, st)
            launch(c, st)
            host = self._fetch(c.out, c.out_bytes, st)
        return ranges_of(host, c.batch, opts)

    def _parts(self, idx, clouds):
        """``idx`` cut into launches of at most 64 clouds and less than 2^31 staged bytes."""
        part, size = [], 0
        for i in idx:
            nb = _align(len(clouds[i].data)) + 16
            if part and (len(part) == MAX_FRAMES or size + nb >= INT31):
                yield part
                part, size = [], 0
            part.append(i)
            size += nb
        if part:
            yield part

    # ---------------------------------------------------------------------- API
    def ranges(self, clouds: Sequence, opts: ScanOptions) -> List[np.ndarray]:
        """Per cloud its scan's ``ranges`` ``<f4 [n]``, in input order."""
        return self._per_cloud(
            clouds, lambda i, lay: layout_device_ok(lay),
            lambda i, lay: ranges_numpy(clouds[i], opts, lay),
            lambda lay, part: (*cloud_bytes(clouds, part), lay, opts), self._run_device,
            lambda i, lay: f"LaserScanner: tca_laser_scan takes little-endian FLOAT32 x, y, z (got {lay}); such "
                           "clouds are scanned on the host",
            device=self.gpu and device_enabled())


def ranges_numpy(cloud, opts: ScanOptions, lay: Optional[CloudLayout] = None) -> np.ndarray:
    """One cloud through the definition → its ranges."""
    return scan_numpy(cloud_xyzi(cloud, lay), opts)
