"""K32 — an oriented box per obstacle cluster: the search-based L-shape fit in fixed point.

``ops/cluster.py`` (K31) gives every cluster an axis-aligned box; a parked car at 30 degrees to the
sensor axes gets almost twice its footprint and no heading.  What ROS users run Autoware's
``lidar_shape_estimation`` for (the search-based fit of Zhang et al., "Efficient L-shape fitting for
vehicle detection using laser scanners", IV 2017, with the closeness criterion), in one more
subscriber on a CPU core, runs here straight behind ``tca_cluster``: its labels, its table and the
obstacle slab are on the device already, and one more small table comes back.
:func:`fit_numpy` is the definition, bit for bit and in integers only; the HIP kernel
``tca_cluster_fit`` (``csrc/kernels/cluster_fit.hip``) gives the same bytes; :func:`fit_ref` is a
float64 brute force with exact trigonometry, and :func:`fit_band` how far the two may lie apart
(``docs/precision.md``).

**Per cluster** (a row of K31's table) and per point of it, with ``xi, yi`` K31's integers in units
of 1/1024 m::

    cx = (min_x + max_x) >> 1;  cy likewise             # floor
    dx = xi - cx;  dy = yi - cy                          # |dx|, |dy| <= 32768, or the cluster is oversize
    theta_j = j * (pi / 2) / angles,  j = 0 .. angles - 1
    c_j = int(rint(cos(theta_j) * 2**14));  s_j likewise # a host table: the kernel has no trigonometry
    u = dx * c_j + dy * s_j;  v = dy * c_j - dx * s_j    # units of 2^-24 m, |u|, |v| < 2^30
    u_min, u_max, v_min, v_max                           # over the cluster's points, per direction
    d = min(u - u_min, u_max - u, v - v_min, v_max - v) >> 10
    w = (d0q << 16) // max(d, d0q),  d0q = int(rint(d0 * 2**14))       # <= 65536, a 32-bit division
    score_j = sum of w                                   # int64

The largest ``score_j`` wins, among equals the smallest area ``(u_max - u_min) * (v_max - v_min)``
(int64), among those the smallest ``j``; the row of :data:`FIT_DTYPE` holds that ``j``, its bounds
and its score.  A cluster whose x or y side exceeds 65536 units (64 m) is not fitted: ``flags`` bit 0
is set, every other field is 0 and its box stays the axis-aligned one.  Direction 0 is the
axis-aligned box.  Every reduction is an integer minimum, maximum or sum: nothing depends on the
order of the points.

Not here: variance or pure-area criteria, convex hulls or polygons.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import _native
from ..ros import msgs
from . import cluster as C
from .laser_scan import _number
from .range2d import _xyz

CHUNK = 4096  # points of one workgroup: 32 KiB of LDS
MAX_ANGLES = 128
MAX_SIDE = 65536  # units of 1/1024 m: a cluster wider than this is not fitted
OVERSIZE = 1  # flags
FIT_ROW = 32  # bytes
FIT_DTYPE = np.dtype([("j", "<i4"), ("flags", "<i4"), ("u_min", "<i4"), ("u_max", "<i4"), ("v_min", "<i4"),
                      ("v_max", "<i4"), ("score", "<i8")])
assert FIT_DTYPE.itemsize == FIT_ROW
_BLOCK = 8192  # points per block of the definition's sweeps


def device_enabled() -> bool:
    """``TCA_DEVICE_CLUSTER_FIT=0`` keeps the definition on GPU engines too."""
    return os.environ.get("TCA_DEVICE_CLUSTER_FIT", "1") != "0"


@dataclass(frozen=True)
class FitOptions:
    angles: int = 90
    d0: float = 0.1

    def __post_init__(self):
        C._count("angles", self.angles, 2, MAX_ANGLES)
        d0 = _number("d0", self.d0)
        if not 0.01 <= d0 <= 1.0:
            raise ValueError(f"d0 must be within 0.01..1 m, got {d0!r}")
        object.__setattr__(self, "d0", d0)

    @property
    def d0q(self) -> int:
        return int(np.rint(self.d0 * 2 ** 14))


def as_options(v) -> Optional[FitOptions]:
    """``v`` (None, a :class:`FitOptions` or a dict of its fields) as options: a bad one fails here."""
    return v if v is None or isinstance(v, FitOptions) else FitOptions(**v)


def directions(angles: int):
    """``(c, s)`` int32 [angles]: the cosines and sines of the candidate directions, times 2^14."""
    theta = np.arange(angles) * (np.pi / 2) / angles
    return np.rint(np.cos(theta) * 2 ** 14).astype(np.int32), np.rint(np.sin(theta) * 2 ** 14).astype(np.int32)


# ------------------------------------------------------------------------- definition
def _fitted(table) -> np.ndarray:
    side = np.maximum(table["max_x"].astype(np.int64) - table["min_x"], table["max_y"].astype(np.int64) - table["min_y"])
    return side <= MAX_SIDE


def centred(points, label, table):
    """Per table row the ``(dx, dy)`` int64 of its points (None: oversize)."""
    x, y, _ = _xyz(points)
    label = np.asarray(label)
    m = label >= 0
    order = np.argsort(label[m], kind="stable")
    k = label[m][order]
    xi = np.rint(x[m][order] * np.float32(C.Q)).astype(np.int64)
    yi = np.rint(y[m][order] * np.float32(C.Q)).astype(np.int64)
    lo, hi = np.searchsorted(k, np.arange(len(table))), np.searchsorted(k, np.arange(len(table)), "right")
    cx = (table["min_x"].astype(np.int64) + table["max_x"]) >> 1
    cy = (table["min_y"].astype(np.int64) + table["max_y"]) >> 1
    ok = _fitted(table)
    return [(xi[a:b] - cx[r], yi[a:b] - cy[r]) if ok[r] else None for r, (a, b) in enumerate(zip(lo, hi))]


def scores_numpy(dx: np.ndarray, dy: np.ndarray, opts: FitOptions):
    """One cluster's centred points → ``(score [angles] int64, bounds [angles, 4] int64: u_min, u_max,
    v_min, v_max)`` by the rules above."""
    c, s = (t.astype(np.int64) for t in directions(opts.angles))
    big = np.int64(2 ** 62)
    b = np.stack([np.full(opts.angles, big), np.full(opts.angles, -big)] * 2, 1)
    for at in range(0, len(dx), _BLOCK):
        u = np.outer(dx[at:at + _BLOCK], c) + np.outer(dy[at:at + _BLOCK], s)
        v = np.outer(dy[at:at + _BLOCK], c) - np.outer(dx[at:at + _BLOCK], s)
        b[:, 0], b[:, 1] = np.minimum(b[:, 0], u.min(0)), np.maximum(b[:, 1], u.max(0))
        b[:, 2], b[:, 3] = np.minimum(b[:, 2], v.min(0)), np.maximum(b[:, 3], v.max(0))
    score, d0q = np.zeros(opts.angles, np.int64), np.int64(opts.d0q)
    for at in range(0, len(dx), _BLOCK):
        u = np.outer(dx[at:at + _BLOCK], c) + np.outer(dy[at:at + _BLOCK], s)
        v = np.outer(dy[at:at + _BLOCK], c) - np.outer(dx[at:at + _BLOCK], s)
        d = np.minimum(np.minimum(u - b[:, 0], b[:, 1] - u), np.minimum(v - b[:, 2], b[:, 3] - v)) >> 10
        score += ((d0q << 16) // np.maximum(d, d0q)).sum(0)
    return score, b


def fit_numpy(points, label, table, opts: FitOptions) -> np.ndarray:
    """The definition → ``fit`` [len(table)] of :data:`FIT_DTYPE`.  ``points`` [N, >=3], ``label`` [N]
    and ``table``: what ``cluster_numpy`` took and gave."""
    fit = np.zeros(len(table), FIT_DTYPE)
    for r, p in enumerate(centred(points, label, table)):
        if p is None:
            fit[r]["flags"] = OVERSIZE
            continue
        score, b = scores_numpy(*p, opts)
        area = (b[:, 1] - b[:, 0]) * (b[:, 3] - b[:, 2])
        j = np.lexsort((np.arange(opts.angles), area, -score))[0]  # score down, then area up, then j up
        fit[r] = (j, 0, *b[j], score[j])
    return fit


def fit_ref(points, label, table, opts: FitOptions):
    """Float64 brute force → ``(score [rows, angles], bounds [rows, angles, 4] in metres from the
    cluster's centre ``(cx, cy) / 1024``)``, NaN for an oversize row: exact ``cos`` / ``sin`` of
    ``theta_j``, ``d`` in metres, ``score = sum(d0 / max(d, d0))``.  The points are K31's integers
    (``xi / 1024`` is exact in float64), which both evaluations take as their input."""
    theta = np.arange(opts.angles) * (np.pi / 2) / opts.angles
    c, s = np.cos(theta), np.sin(theta)
    score = np.full((len(table), opts.angles), np.nan)
    bounds = np.full((len(table), opts.angles, 4), np.nan)
    for r, p in enumerate(centred(points, label, table)):
        if p is None:
            continue
        x, y = p[0] / C.Q, p[1] / C.Q
        u, v = np.outer(x, c) + np.outer(y, s), np.outer(y, c) - np.outer(x, s)
        bounds[r] = np.stack([u.min(0), u.max(0), v.min(0), v.max(0)], 1)
        d = np.minimum(np.minimum(u - u.min(0), u.max(0) - u), np.minimum(v - v.min(0), v.max(0) - v))
        score[r] = (opts.d0 / np.maximum(d, opts.d0)).sum(0)
    return score, bounds


def fit_band(table, opts: FitOptions):
    """Per table row ``(per point |score_j / 65536 - ref_j| / n, |bound / 2**24 - ref bound| in
    metres)`` at most (``docs/precision.md``): with ``R`` the largest ``|dx| + |dy|`` of the
    cluster in metres, a projection is off by at most ``E = R * 2**-15``, hence ``d`` by ``2 E``
    plus the shift's 2^-14 m, ``d0q`` by 2^-15 m, and the quotient's floor by 2^-16."""
    R = ((table["max_x"].astype(np.float64) - table["min_x"]) + (table["max_y"].astype(np.float64) - table["min_y"])
         + 2) / 2 / C.Q
    E = R * 2.0 ** -15
    return (2 * E + 2.0 ** -14 + 2.0 ** -15) / min(opts.d0, opts.d0q / 2 ** 14) + 2.0 ** -16, E


# ---------------------------------------------------------------------------- messages
def fit_boxes(table: np.ndarray, fit: np.ndarray, header: msgs.Header, jsk: bool = True,
              opts: FitOptions = FitOptions()):
    """The table and its fit as a box message with ``header``: ``cluster_boxes``'s message with, for
    every fitted row, the box of the winning direction, in float64: yaw ``theta = j * pi / (2 *
    angles)``, the centre ``(cx, cy) / 1024`` plus the midpoint of the bounds turned by ``theta``
    and scaled by 2^-24, the extents ``(u_max - u_min) / 2**24`` along ``theta`` and ``(v_max -
    v_min) / 2**24`` across it; where the second is the larger the two are swapped and ``theta +=
    pi / 2``: yaw lies in [0, pi) and the box's x axis is its long side.  z, ``value`` / ``score``
    and ``label`` / ``id`` are ``cluster_boxes``'s; an oversize row keeps its axis-aligned box."""
    from ..inference.ros_inference3d import boxes_to_detection3d, boxes_to_jsk

    n = len(table)
    if len(fit) != n or fit.dtype != FIT_DTYPE:
        raise ValueError(f"fit must hold one row of FIT_DTYPE per table row ({n}), got {len(fit)} of {fit.dtype}")
    if (fit["flags"] & ~OVERSIZE).any() or (fit["j"] < 0).any() or (fit["j"] >= opts.angles).any():
        raise ValueError(f"fit holds a flag other than {OVERSIZE} or a direction outside 0..{opts.angles - 1}")
    b = np.zeros((n, 7), np.float64)
    for j, a in enumerate("xyz"):
        lo, hi = table["min_" + a].astype(np.float64), table["max_" + a].astype(np.float64)
        b[:, j] = (lo + hi) / 2 / C.Q
        b[:, 3 + j] = (hi - lo) / C.Q
    m = fit["flags"] == 0
    f, t = fit[m], table[m]
    theta = f["j"] * np.pi / (2 * opts.angles)
    c, s = np.cos(theta), np.sin(theta)
    u = (f["u_min"].astype(np.float64) + f["u_max"]) / 2 / 2 ** 24
    v = (f["v_min"].astype(np.float64) + f["v_max"]) / 2 / 2 ** 24
    b[m, 0] = ((t["min_x"].astype(np.int64) + t["max_x"]) >> 1) / C.Q + (u * c - v * s)
    b[m, 1] = ((t["min_y"].astype(np.int64) + t["max_y"]) >> 1) / C.Q + (u * s + v * c)
    along = (f["u_max"].astype(np.float64) - f["u_min"]) / 2 ** 24
    across = (f["v_max"].astype(np.float64) - f["v_min"]) / 2 ** 24
    turn = across > along
    b[m, 3], b[m, 4] = np.where(turn, across, along), np.where(turn, along, across)
    b[m, 6] = theta + np.where(turn, np.pi / 2, 0.0)
    if jsk:  # the jsk columns swap the first two dimensions back
        b[:, [3, 4]] = b[:, [4, 3]]
    pred = {"pred_boxes": b, "pred_scores": table["n"].astype(np.float32), "pred_labels": np.arange(n)}
    hdr = msgs.Header(seq=header.seq, stamp=header.stamp, frame_id=header.frame_id)
    return boxes_to_jsk(pred, np.arange(n), hdr) if jsk else boxes_to_detection3d(pred, np.arange(n), hdr)


# --------------------------------------------------------------------------------- GPU
def slots_cap(max_n: int) -> int:
    """How many clusters of more than :data:`CHUNK` points a cloud of ``max_n`` points can hold, plus one."""
    return max_n // CHUNK + 1


@dataclass
class FitCall:
    """One prepared launch behind a :class:`~triton_client_amd.ops.cluster.ClusterCall`."""
    cluster: C.ClusterCall
    opts: FitOptions
    trig: np.ndarray  # int32 [2][angles]: c, s (host: the launcher copies it into the kernels' arguments)
    plan: torch.Tensor  # 16 bytes per table row
    grouped: torch.Tensor  # (dx, dy) int32 per record, grouped by cluster
    slots: torch.Tensor  # 32 bytes per cloud, slot and direction
    work: torch.Tensor  # int32 per cloud: the slot and chunk counts, the slots' clusters, the chunk list
    fit: torch.Tensor  # uint8: [B][max_clusters] rows of FIT_DTYPE

    @property
    def fit_bytes(self) -> int:
        return self.cluster.batch * self.cluster.opts.max_clusters * FIT_ROW


def work_ints(max_n: int) -> int:
    """int32 per cloud of :attr:`FitCall.work`."""
    return 2 + slots_cap(max_n) + 4 * slots_cap(max_n)


def prepare(ex, c: C.ClusterCall, opts: FitOptions) -> FitCall:
    """The fit's buffers for ``c`` from the workspace of ``ex`` (a ``ClusterExtractor``)."""
    cap = slots_cap(c.max_n)
    f = FitCall(cluster=c, opts=opts, trig=np.ascontiguousarray(np.stack(directions(opts.angles))),
                plan=ex._device_buf("fit_plan", 16 * c.batch * c.opts.max_clusters),
                grouped=ex._device_buf("fit_grouped", 8 * c.records),
                slots=ex._device_buf("fit_slots", 32 * c.batch * cap * opts.angles),
                work=ex._device_buf("fit_work", 4 * c.batch * work_ints(c.max_n)), fit=None)
    f.fit = ex._device_buf("fit_out", f.fit_bytes)
    return f


def launch(f: FitCall, stream=None, split: bool = True) -> None:
    """The launch alone, on ``stream`` behind ``tca_cluster``'s (three to six kernels): no allocation,
    no copy, no sync.  ``split`` False: one workgroup per cluster whatever its size (measurements)."""
    p, c = _native.ptr, f.cluster
    o = c.layout.offsets
    _native.call("tca_cluster_fit", p(c.data), c.data_bytes, p(c.frame_off), p(c.frame_n), c.n_stride, c.batch,
                 c.max_n, c.layout.point_step, o[0], o[1], o[2], p(c.label), p(c.out), p(c.found), int(c.opts.max_clusters),
                 int(f.opts.angles), int(f.opts.d0q), f.trig.ctypes.data, 1 if split else 0, p(f.plan), p(f.grouped),
                 p(f.slots), f.slots.numel() * f.slots.element_size(), p(f.work),
                 f.work.numel() * f.work.element_size(), p(f.fit), _native.stream_ptr(stream))


def results_of(host: np.ndarray, f: FitCall, founds) -> list:
    """Per cloud its fit table, of a launch's ``fit_bytes`` bytes."""
    mc = f.cluster.opts.max_clusters
    rows = host.view(FIT_DTYPE).reshape(f.cluster.batch, mc)
    return [rows[b, :min(int(n), mc)].copy() for b, n in enumerate(founds)]
