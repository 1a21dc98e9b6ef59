"""K30 — the cloud split into ground and obstacles.

Clustering, costmaps and free-space estimation start from a cloud with the ground taken out, what
ROS users run ``ray_ground_filter``, ``linefit_ground_segmentation`` or Patchwork for, on a CPU core
next to the driver.  Here the driver publishes two more ``PointCloud2`` per cloud: ``obstacles``
(the input records that stand above the estimated ground) and ``ground`` (those at or below it),
every kept record copied byte for byte in input order, so ring, time and intensity fields survive.
:func:`split_numpy` is the definition, bit for bit (the pattern of ``ops/laser_scan.py``); the HIP
kernel ``tca_ground_split`` (``csrc/kernels/ground.hip``) computes the same classes from the raw
payload and compacts the records on the device, and :func:`split_ref` is a float64 brute force with
true ``atan2`` that also marks the decisions float32 may legitimately take differently
(``docs/precision.md``).

**The grid** is polar around the sensor's z axis: ``sectors`` angular sectors (the laser scan's
pseudo-angle rule against a table of ``S + 1`` edges, ``e_k = -pi + k * 2 pi / S``, ``e_S = pi``)
times ``nr = ceil(range_max / cell - 1e-9)`` rings ``cell`` metres wide.  Heights are integers in
units of 1/1024 m, so everything after the per-point part is integer arithmetic:
``h0 = -rint(sensor_height * 1024)``, ``slope_q = rint(tan(max_slope) * cell * 1024)``,
``noise_q``, ``thick_q`` and ``top_q`` alike (each clamped to ``2**21``, 2 km, in magnitude;
an infinite ``max_height`` is ``2**21``).

**Per point** ``(x, y, z)`` as sent, in float32, every operation rounded on its own (no FMA), IEEE
division and square root::

    s = |x| + |y|;  q = copysign(1 - x / s, y)      # the sector: laser_scan.pseudo_bins
    r = sqrt(x * x + y * y);  d = r / float32(cell)
    valid = has a sector and r >= float32(range_min) and d < float32(nr) and |z| <= 512
    j = int(d)                                      # the ring (truncation)
    zi = int32(rint(z * 1024))                      # the product is exact, ties to even

(a NaN compares false).  **Per cell** ``M[j][s]`` is the smallest ``zi`` of its valid points,
``EMPTY = INT32_MAX`` without any; nothing depends on the order of the points.  **Per sector** the
rings are walked outwards with ``g = h0`` and ``jg = -1``: an empty cell gets ``G = g``; at any
other, ``allow = noise_q + slope_q * (j - jg)``, and if ``|M - g| <= allow`` the cell has ground
(``g = M``, ``jg = j``); either way ``G[j][s] = g``.  A cell whose lowest point is too high holds
only an obstacle and the ground is carried under it; one whose lowest point is too low is an
outlier and is not adopted; after a real downward step the ground is adopted again once ``allow``
has grown.  **Per valid point** ``h = zi - G``: ground iff ``h <= thick_q``, obstacle iff
``thick_q < h <= top_q``, dropped otherwise — like every point that is not valid.

Not here: tf and ``target_frame``, plane fitting, temporal smoothing of the ground, clustering, and
feeding the obstacle cloud into the ``LaserScan`` (the follow-up this makes possible).
"""
from __future__ import annotations

import functools
import math
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native
from ..ros import msgs
from .cloud_common import CloudLayout, CloudStager, _align, cloud_bytes, cloud_xyzi, fields_f32, plan_staging
from .laser_scan import _number, pseudo64, pseudo_bins
from .range2d import INT31, U, _xyz

MAX_FRAMES = 64  # clouds per launch
MAX_SECTORS = 4096
MAX_RINGS = 512
MAX_CELLS = 2 ** 20  # sectors * rings of one cloud
MAX_PLANE = 2 ** 24  # cells of one launch
EMPTY = 2 ** 31 - 1  # the height of a cell no valid point fell into
Q = 1024  # height units per metre
Z_LIMIT = 512.0  # |z| beyond this is not valid
Q_LIMIT = 2 ** 21  # the integer constants are clamped to this in magnitude
BLOCK = 256  # points per block of the device's counts
DROPPED, GROUND, OBSTACLE = 0, 1, 2
WANT_OBSTACLES, WANT_GROUND = 1, 2
EDGE_BAND = 8 * U  # split_ref: how near a sector edge a point's pseudo-angle may be taken either way
RING_BAND = 3 * U  # split_ref: the same for d against an integer and r against range_min, relative


def device_enabled() -> bool:
    """``TCA_DEVICE_GROUND=0`` keeps the definition on GPU engines too."""
    return os.environ.get("TCA_DEVICE_GROUND", "1") != "0"


# ----------------------------------------------------------------------------- options
def _quant(v: float) -> int:
    """``rint(v * 1024)`` clamped to ``+-2**21`` (an infinity: the clamp)."""
    if math.isinf(v):
        return Q_LIMIT if v > 0 else -Q_LIMIT
    return int(max(-Q_LIMIT, min(Q_LIMIT, np.rint(v * Q))))


@dataclass(frozen=True)
class GroundOptions:
    sectors: int = 360
    cell: float = 0.5
    range_min: float = 0.0
    range_max: float = 80.0
    sensor_height: float = 1.8
    max_slope: float = 10.0
    noise: float = 0.05
    thickness: float = 0.2
    max_height: float = math.inf

    def __post_init__(self):
        s = self.sectors
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 1 <= s <= MAX_SECTORS:
            raise ValueError(f"sectors must be an integer in 1..{MAX_SECTORS}, got {s!r}")
        cell = _number("cell", self.cell)
        if not 0.05 <= cell <= 10.0:
            raise ValueError(f"cell must be within 0.05..10 m, got {cell!r}")
        r0, r1 = _number("range_min", self.range_min), _number("range_max", self.range_max)
        if not r0 >= 0:
            raise ValueError(f"range_min must be >= 0, got {r0!r}")
        if not np.float32(r0) < np.float32(r1):
            raise ValueError(f"range_max must exceed range_min in float32, got {r0!r} and {r1!r}")
        nr = math.ceil(r1 / cell - 1e-9)
        if not 1 <= nr <= MAX_RINGS:
            raise ValueError(f"range_max gives {nr} rings of {cell!r} m, want 1..{MAX_RINGS}")
        if int(s) * nr > MAX_CELLS:
            raise ValueError(f"range_max gives {int(s)} x {nr} cells, want at most {MAX_CELLS}")
        _number("sensor_height", self.sensor_height)
        slope = _number("max_slope", self.max_slope)
        if not 0 <= slope <= 45:
            raise ValueError(f"max_slope must be within 0..45 degrees, got {slope!r}")
        for name in ("noise", "thickness"):
            v = _number(name, getattr(self, name))
            if not v >= 0:
                raise ValueError(f"{name} must be >= 0, got {v!r}")
        top = _number("max_height", self.max_height, False)
        if not top > float(self.thickness):
            raise ValueError(f"max_height must exceed thickness, got {top!r} <= {self.thickness!r}")

    @property
    def nr(self) -> int:
        """The number of rings."""
        return math.ceil(float(self.range_max) / float(self.cell) - 1e-9)

    @property
    def c32(self) -> np.float32:
        return np.float32(self.cell)

    @property
    def r0(self) -> np.float32:
        return np.float32(self.range_min)

    @property
    def h0(self) -> int:
        return -_quant(float(self.sensor_height))

    @property
    def slope_q(self) -> int:
        return _quant(math.tan(math.radians(float(self.max_slope))) * float(self.cell))

    @property
    def noise_q(self) -> int:
        return _quant(float(self.noise))

    @property
    def thick_q(self) -> int:
        return _quant(float(self.thickness))

    @property
    def top_q(self) -> int:
        return _quant(float(self.max_height))


def edge_angles(opts: GroundOptions) -> np.ndarray:
    """``e_k`` float64 ``[S + 1]``: the sectors' edges as angles, the last one ``pi`` itself."""
    S = int(opts.sectors)
    e = -math.pi + np.arange(S + 1, dtype=np.float64) * (2 * math.pi / S)
    e[S] = math.pi
    return e


@functools.lru_cache(maxsize=64)
def edge_table(opts: GroundOptions) -> np.ndarray:
    """``t_k`` float32 ``[S + 1]``: the sectors' edges as pseudo-angles (made once per options; read-only)."""
    e = edge_angles(opts)
    t = pseudo64(np.cos(e), np.sin(e)).astype(np.float32)
    assert (np.diff(t) >= 0).all(), "the edge table must not decrease"
    t.setflags(write=False)
    return t


# ------------------------------------------------------------------------- definition
def cells_numpy(points, opts: GroundOptions):
    """The per-point half of the definition → ``(sector [N] int32, ring [N] int32, zi [N] int32,
    valid [N] bool)``; the first three are 0 where the point is not valid."""
    x, y, z = _xyz(points)
    sec, has = pseudo_bins(x, y, edge_table(opts))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = np.sqrt(x * x + y * y).astype(np.float32)
        d = (r / opts.c32).astype(np.float32)
        valid = has & (r >= opts.r0) & (d < np.float32(opts.nr)) & (np.abs(z) <= np.float32(Z_LIMIT))
    ring = np.where(valid, d, np.float32(0)).astype(np.int32)  # truncation
    zi = np.rint(np.where(valid, z, np.float32(0)) * np.float32(Q)).astype(np.int32)
    return np.where(valid, sec, 0).astype(np.int32), ring, zi, valid


def min_plane(sector, ring, zi, valid, opts: GroundOptions) -> np.ndarray:
    """``M`` int32 ``[nr][S]`` (ring-major, like the device's): per cell the lowest valid ``zi``."""
    plane = np.full((opts.nr, int(opts.sectors)), EMPTY, np.int32)
    np.minimum.at(plane, (ring[valid], sector[valid]), zi[valid])
    return plane


def sweep_numpy(plane: np.ndarray, opts: GroundOptions) -> np.ndarray:
    """``M`` → ``G`` int32 ``[nr][S]``: every sector walked outwards, all sectors at once."""
    nr, S = plane.shape
    g = np.full(S, opts.h0, np.int64)
    jg = np.full(S, -1, np.int64)
    G = np.empty((nr, S), np.int32)
    noise_q, slope_q = opts.noise_q, opts.slope_q
    for j in range(nr):
        m = plane[j].astype(np.int64)
        adopt = (m != EMPTY) & (np.abs(m - g) <= noise_q + slope_q * (j - jg))
        g = np.where(adopt, m, g)
        jg = np.where(adopt, j, jg)
        G[j] = g
    return G


def classes_of(sector, ring, zi, valid, G: np.ndarray, opts: GroundOptions) -> np.ndarray:
    h = zi.astype(np.int64) - G[ring, sector]
    cls = np.where(h <= opts.thick_q, GROUND, np.where(h <= opts.top_q, OBSTACLE, DROPPED))
    return np.where(valid, cls, DROPPED).astype(np.int8)


def ground_numpy(points, opts: GroundOptions) -> np.ndarray:
    """The ground estimate ``G`` int32 ``[nr][S]`` of a cloud."""
    return sweep_numpy(min_plane(*cells_numpy(points, opts), opts), opts)


def split_numpy(points, opts: GroundOptions) -> np.ndarray:
    """→ ``int8 [N]``, per point 0 dropped, 1 ground, 2 obstacle: the definition.  ``points``
    [N, >=3] (x, y, z)."""
    sector, ring, zi, valid = cells_numpy(points, opts)
    G = sweep_numpy(min_plane(sector, ring, zi, valid, opts), opts)
    return classes_of(sector, ring, zi, valid, G, opts)


def split_ref(points, opts: GroundOptions) -> Tuple[np.ndarray, np.ndarray]:
    """Float64 brute force → ``(class [N] int8, band [N] bool)``: the sector is
    ``floor((atan2(y, x) + pi) / (2 pi / S))`` (``pi`` itself in sector ``S - 1``), the ring
    ``floor(r / cell)`` in float64, the heights, the sweep and the classes as in the definition
    (``z * 1024`` is exact on both sides).

    ``band`` marks the points whose float32 decision may legitimately differ: the float64
    pseudo-angle lies within ``8 * 2**-24`` of an edge of the point's sector, ``d`` within
    ``3 * 2**-24 * d`` of an integer (``nr`` among them), or ``r`` within ``3 * 2**-24 * r`` of
    ``range_min``.  ``docs/precision.md`` has the derivation.  ``float32(cell)`` and
    ``float32(range_min)`` are inputs of both evaluations and exact here.  A banded point may
    change its cell's minimum, so the two are compared on clouds without banded points."""
    x, y, z = (c.astype(np.float64) for c in _xyz(points))
    S, nr = int(opts.sectors), opts.nr
    c, r0 = float(opts.c32), float(opts.r0)
    t64 = pseudo64(np.cos(edge_angles(opts)), np.sin(edge_angles(opts)))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = np.abs(x) + np.abs(y)
        ok = np.isfinite(s) & (s != 0)
        a = np.where(ok, np.arctan2(y, x), 0.0)
        sec = np.clip(np.floor((a + math.pi) / (2 * math.pi / S)), 0, S - 1).astype(np.int64)
        r = np.sqrt(x * x + y * y)
        d = r / c
        valid = ok & (r >= r0) & (d < nr) & (np.abs(z) <= Z_LIMIT)
        ring = np.where(valid, np.floor(np.where(valid, d, 0.0)), 0).astype(np.int64)
        zi = np.rint(np.where(valid, z, 0.0) * Q).astype(np.int64)
        q = np.where(ok, pseudo64(x, np.where(ok, y, 1.0)), np.nan)
        band = ok & ((np.abs(q - t64[sec]) <= EDGE_BAND) | (np.abs(q - t64[sec + 1]) <= EDGE_BAND))
        band |= ok & (np.abs(d - np.rint(d)) <= RING_BAND * d)
        band |= ok & (np.abs(r - r0) <= RING_BAND * r)
    sec32, ring32, zi32 = sec.astype(np.int32), ring.astype(np.int32), zi.astype(np.int32)
    G = sweep_numpy(min_plane(sec32, ring32, zi32, valid, opts), opts)
    return classes_of(sec32, ring32, zi32, valid, G, opts), band


# ---------------------------------------------------------------------------- messages
def _check_want(want: int) -> int:
    if isinstance(want, bool) or want not in (1, 2, 3):
        raise ValueError(f"want must be 1 (obstacles), 2 (ground) or 3 (both), got {want!r}")
    return int(want)


def cloud_rows(cloud) -> np.ndarray:
    """The cloud's records as ``uint8 [N][point_step]`` (an organised cloud flattened), a view."""
    n, step = int(cloud.width) * int(cloud.height), int(cloud.point_step)
    return np.frombuffer(cloud.data, np.uint8, n * step).reshape(n, step)


def subset_message(cloud, data, count: int) -> msgs.PointCloud2:
    """``count`` records of ``cloud`` (``data``: their bytes) as an unorganised, dense cloud with
    the input's header, fields, endianness and ``point_step``."""
    step = int(cloud.point_step)
    data = bytes(data)
    if len(data) != count * step:
        raise ValueError(f"{len(data)} bytes, want {count} records of {step}")
    return msgs.PointCloud2(header=cloud.header, height=1, width=count, fields=list(cloud.fields),
                            is_bigendian=cloud.is_bigendian, point_step=step, row_step=count * step, data=data,
                            is_dense=True)


def split_messages(cloud, cls: np.ndarray, want: int = 3):
    """→ ``(obstacles message or None, ground message or None)`` from the per-point classes: the
    rows of ``cloud.data`` of each class, in input order."""
    want = _check_want(want)
    rows = cloud_rows(cloud)
    out = []
    for bit, k in ((WANT_OBSTACLES, OBSTACLE), (WANT_GROUND, GROUND)):
        keep = rows[cls == k] if want & bit else None
        out.append(None if keep is None else subset_message(cloud, keep.tobytes(), len(keep)))
    return tuple(out)


def split_cloud_numpy(cloud, opts: GroundOptions, want: int = 3, lay: Optional[CloudLayout] = None):
    """One cloud through the definition → its two messages."""
    return split_messages(cloud, split_numpy(cloud_xyzi(cloud, lay), opts), want)


# --------------------------------------------------------------------------------- GPU
@dataclass
class GroundCall:
    """One prepared launch: device views of its inputs, workspace and output."""
    data: torch.Tensor
    data_bytes: int  # what the kernels may read records from
    slab_bytes: int  # the staged records' bytes: the output slab's size
    frame_off: torch.Tensor
    frame_n: torch.Tensor
    table: torch.Tensor  # float32 [S + 1]
    plane: torch.Tensor  # uint8 view of B * nr * S int32 heights
    blocks: torch.Tensor  # uint8 view of int32 [B][nblk + 1][2]: per block its counts, then its offsets
    cls: torch.Tensor  # uint8, one class per staged record (the saved-class variant)
    out: torch.Tensor  # uint8: the slab of slab_bytes, then counts int32 [B][2] (obstacles, ground)
    layout: CloudLayout
    batch: int
    max_n: int
    ns: Tuple[int, ...]
    frame_offs: Tuple[int, ...]
    opts: GroundOptions

    @property
    def counts(self) -> torch.Tensor:
        return self.out[self.slab_bytes:self.out_bytes].view(torch.int32).view(self.batch, 2)

    @property
    def out_bytes(self) -> int:
        return self.slab_bytes + 8 * self.batch


def launch(c: GroundCall, want: int = 3, stream=None, saved: bool = True) -> None:
    """The launch alone (six kernels on ``stream``): no allocation, no copy, no sync.  ``saved``:
    the scatter reads the classes the count pass saved; False: it computes them again."""
    p = _native.ptr
    o, r = c.layout.offsets, c.opts
    _native.call("tca_ground_split", p(c.data), c.data_bytes, p(c.frame_off), p(c.frame_n), c.batch, c.max_n,
                 c.layout.point_step, o[0], o[1], o[2], p(c.table), int(r.sectors), r.nr, float(r.c32), float(r.r0),
                 r.h0, r.slope_q, r.noise_q, r.thick_q, r.top_q, _check_want(want), 1 if saved else 0, p(c.plane),
                 p(c.blocks), p(c.cls), p(c.out), c.slab_bytes, p(c.counts), _native.stream_ptr(stream))


def layout_device_ok(lay: CloudLayout) -> bool:
    """What ``tca_ground_split`` reads in place: little-endian FLOAT32 x, y, z inside the record."""
    return fields_f32(lay, (0, 1, 2))


def regions_of(host: np.ndarray, c: GroundCall, want: int) -> List[tuple]:
    """Per cloud ``(obstacle bytes or None, ground bytes or None)`` of a launch's output slab and
    counts (``host``: ``out_bytes`` bytes)."""
    counts = host[c.slab_bytes:c.out_bytes].view("<i4").reshape(c.batch, 2)
    step, res = c.layout.point_step, []
    for b, (n, fo) in enumerate(zip(c.ns, c.frame_offs)):
        n_obs, n_gnd = int(counts[b, 0]), int(counts[b, 1])
        obs = host[fo:fo + n_obs * step].tobytes() if want & WANT_OBSTACLES else None
        gnd = host[fo + (n - n_gnd) * step:fo + n * step].tobytes() if want & WANT_GROUND else None
        res.append((obs, gnd))
    return res


class GroundSplitter(CloudStager):
    """Splits clouds into obstacle and ground clouds: on a GPU with ``tca_ground_split`` (its own
    workspace, stream and pinned staging: one H2D of the payloads and the edge table, one launch and
    the copy back per launch group of same-layout clouds), on the CPU — and with
    ``TCA_DEVICE_GROUND=0`` — with the definition.  Clouds the kernel does not take (non-FLOAT32 or
    big-endian fields) run the definition with one warning.

    ``copy_back``: ``"slab"`` copies the whole output slab and the counts in one D2H with one
    synchronize; ``"counted"`` copies the counts, synchronizes, then copies only the used prefix and
    suffix of every slot; ``"auto"``, the default, takes the slab when both halves are wanted and
    the counted copy for one, which is what measured faster in either case
    (``profiles/ground/README.md``).  ``saved`` False: the launch's slower variant (measurements)."""

    copy_back = "auto"
    saved = True

    def prepare(self, payloads: Sequence, ns: Sequence[int], layout: CloudLayout, opts: GroundOptions, stream=None,
                misalign: int = 0) -> GroundCall:
        """Stage one batch (``payloads[b]``: the bytes of ``ns[b]`` points of ``layout``) and the
        edge table in pinned memory and upload them with one H2D copy on ``stream``.  ``misalign``:
        start every payload this many bytes past a 16-byte boundary."""
        if not layout_device_ok(layout):
            raise ValueError(f"tca_ground_split does not take this layout: {layout}")
        B = len(payloads)
        ns = [int(n) for n in ns]
        if not 1 <= B <= MAX_FRAMES:
            raise ValueError(f"{B} clouds do not fit one call (1..{MAX_FRAMES}): split the batch")
        data_bytes = plan_staging(ns, layout.point_step, misalign, ()).data_bytes  # (refused before any allocation)
        if data_bytes >= INT31:
            raise ValueError(f"{data_bytes} payload bytes do not fit one call: split the batch")
        S, nr = int(opts.sectors), opts.nr
        if B * S * nr > MAX_PLANE:
            raise ValueError(f"{B} clouds of {S} x {nr} cells do not fit one call ({MAX_PLANE}): split the batch")
        dev, plan, view = self._stage("ground_in", payloads, ns, layout.point_step, misalign,
                                      [("table", edge_table(opts))], stream)
        max_n = max(ns, default=0)
        nblk = (max_n + BLOCK - 1) // BLOCK
        return GroundCall(data=dev, data_bytes=data_bytes, slab_bytes=data_bytes,
                          frame_off=view("frame_off", B, torch.int64), frame_n=view("frame_n", B, torch.int32),
                          table=view("table", S + 1, torch.float32),
                          plane=self._device_buf("ground_plane", 4 * B * S * nr),
                          blocks=self._device_buf("ground_blocks", 8 * B * (nblk + 1)),
                          cls=self._device_buf("ground_cls", data_bytes // layout.point_step + 1),
                          out=self._device_buf("ground_out", data_bytes + 8 * B), layout=layout, batch=B, max_n=max_n,
                          ns=tuple(ns), frame_offs=plan.frame_offs, opts=opts)

    launch = staticmethod(launch)

    def _fetch_counted(self, c: GroundCall, want: int, st) -> np.ndarray:
        """The counts, a synchronize, then only the used prefix and suffix of every slot; the host
        bytes are laid out like the slab."""
        pin = self._pinned("_pin_out", c.out_bytes)
        with torch.cuda.stream(st):
            pin[c.slab_bytes:c.out_bytes].copy_(c.out[c.slab_bytes:c.out_bytes], non_blocking=True)
        st.synchronize()
        counts = pin.numpy()[c.slab_bytes:c.out_bytes].view("<i4").reshape(c.batch, 2)
        step = c.layout.point_step
        with torch.cuda.stream(st):
            for b, (n, fo) in enumerate(zip(c.ns, c.frame_offs)):
                spans = []
                if want & WANT_OBSTACLES and counts[b, 0]:
                    spans.append((fo, fo + int(counts[b, 0]) * step))
                if want & WANT_GROUND and counts[b, 1]:
                    spans.append((fo + (n - int(counts[b, 1])) * step, fo + n * step))
                for lo, hi in spans:
                    pin[lo:hi].copy_(c.out[lo:hi], non_blocking=True)
        st.synchronize()
        return pin.numpy()[:c.out_bytes]

    def _run_device(self, payloads, ns, layout, opts, want):
        """→ per frame ``(obstacle bytes or None, ground bytes or None)``."""
        with torch.cuda.device(self.device):
            st = self._own_stream()
            c = self.prepare(payloads, ns, layout, opts, st)
            launch(c, want, st, self.saved)
            how = self.copy_back if self.copy_back != "auto" else "slab" if want == 3 else "counted"
            host = self._fetch_counted(c, want, st) if how == "counted" else self._fetch(c.out, c.out_bytes, st)
            return regions_of(host, c, want)

    def _parts_for(self, opts: GroundOptions):
        """The cut of a layout's clouds into launches of at most 64 clouds, less than 2^31 staged
        bytes and at most 2^24 cells."""
        most = max(1, min(MAX_FRAMES, MAX_PLANE // (int(opts.sectors) * opts.nr)))

        def parts(idx, clouds):
            part, size = [], 0
            for i in idx:
                nb = _align(len(clouds[i].data)) + 16
                if part and (len(part) == most or size + nb >= INT31):
                    yield part
                    part, size = [], 0
                part.append(i)
                size += nb
            if part:
                yield part

        return parts

    def _parts(self, idx, clouds, opts: Optional[GroundOptions] = None):
        return self._parts_for(opts or GroundOptions())(idx, clouds)

    # ---------------------------------------------------------------------- API
    def split(self, clouds: Sequence, opts: GroundOptions, want: int = 3) -> List[tuple]:
        """Per cloud ``(obstacles message or None, ground message or None)``, in input order;
        ``want``: 1 obstacles, 2 ground, 3 both (only what is wanted is written and copied)."""
        want = _check_want(want)

        def on_device(payloads, ns, lay, part):
            res = self._run_device(payloads, ns, lay, opts, want)
            step = lay.point_step
            return [tuple(None if d is None else subset_message(clouds[i], d, len(d) // step) for d in pair)
                    for i, pair in zip(part, res)]

        return self._per_cloud(
            clouds, lambda i, lay: layout_device_ok(lay),
            lambda i, lay: split_cloud_numpy(clouds[i], opts, want, lay),
            lambda lay, part: (*cloud_bytes(clouds, part), lay, part), on_device,
            lambda i, lay: f"GroundSplitter: tca_ground_split takes little-endian FLOAT32 x, y, z (got {lay}); such "
                           "clouds are split on the host",
            device=self.gpu and device_enabled(), parts=self._parts_for(opts))
