"""K34 — the cloud thinned on a voxel grid: one centroid per occupied voxel.

Registration, mapping, recording and visualisation all start from a downsampled cloud; ROS users
run ``pcl_ros``'s ``VoxelGrid`` nodelet for it, a sort or a hash of every point on a CPU core in
front of the rest of the chain.  Here the driver publishes it per cloud: a ``PointCloud2`` of x, y,
z, intensity, one record per voxel.  :func:`downsample_numpy` is the definition, bit for bit (the
pattern of ``ops/occupancy_grid.py``); the HIP kernels of ``tca_voxel_downsample``
(``csrc/kernels/voxel_downsample.hip``) compute the same bytes from the raw payload with a hash
table on the device, and :func:`downsample_ref` is a float64 brute force that also names the voxels
float32 may legitimately fill differently (``docs/precision.md``).

All float arithmetic is float32, every operation rounded on its own (no FMA), IEEE division.

**Valid points.**  A point is valid iff x, y and z are finite and ``|v| <= 512`` (``cluster.LIMIT``);
every other point belongs to no voxel.  A cloud of more than 2^24 points is a ``ValueError``.

**Voxel index.**  Per axis ``floor(v / f32(leaf))`` as an integer — ``floor``, not truncation:
-0.05 and +0.05 lie in different voxels.  Its magnitude stays below 2^20 (512 / 0.01), so a voxel
has the 64-bit key ``(iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20)``.

**Sums.**  Integers, so nothing depends on the order of the points: per coordinate
``q = int(rint(v * 65536))`` (the product is exact, ``|q| <= 2^25``) and for the intensity
``qi = int(rint(clamp(i, -65536, 65536) * 4096))``, 0 for a NaN intensity or a cloud without an
intensity field, each summed in int64.  With at most 2^24 points every sum stays below 2^53.

**A kept voxel** has ``n >= min_points`` points (PCL's ``min_points_per_voxel``).  Its centroid
coordinate is ``float32(float64(S) / float64(n * 65536))``: one correctly rounded float64 division,
then one rounding to float32; its intensity the same with 4096.

**Order.**  The kept voxels appear in the order of their first point in the cloud (ascending
smallest point index), not sorted by key: the sensor's scan order survives, and the device compacts
without a sort.

Two departures from PCL's ``VoxelGrid``: PCL sums in float in input order and sorts the output by
voxel index (here: integer sums, first-point order), and every other field (ring, time) is dropped.

**Normals** (``VoxelOptions.normal_radius``, off by default; K35).  With a radius the record grows
by a surface normal and a curvature per voxel, what PCL's ``NormalEstimation`` with a radius search
computes behind a ``VoxelGrid``.  :func:`normals_numpy` is the definition, a function of the
published float32 centroids alone: quantised coordinates, a closed ball in int64, integer moments
about the voxel itself, a float64 covariance rounded to float32 and a fixed number of float32
Jacobi sweeps (``docs/precision.md`` has the rotation's operation order).  ``tca_voxel_normals``
(``csrc/kernels/voxel_normals.hip``) gives its bytes on the device behind ``tca_voxel_downsample``,
and :func:`normals_ref` is a float64 brute force with ``np.linalg.eigh``.

**Outliers** (``VoxelOptions.outlier_radius`` with ``outlier_min_neighbors`` and / or
``outlier_mean_k``, ``outlier_stddev``; off by default; K36).  Between the two, what ``pcl_ros``'s
``RadiusOutlierRemoval`` and ``StatisticalOutlierRemoval`` do behind a ``VoxelGrid``: lone voxels
(rain, dust, ghosts) leave the cloud before the normals are taken, and the kept rows keep their
order.  :func:`outliers_numpy` is the definition — the closed ball of the normals with the voxel
itself left out, a voxel without a neighbour always gone, ``found >= N`` for the radius test, and for
the statistical test the rounded mean of the rounded distances to the ``min(k, found)`` nearest
against ``mean + stddev * sd`` of those means over the cloud (``docs/precision.md``) — and
``tca_voxel_outliers`` (``csrc/kernels/voxel_outliers.hip``) gives its bytes on the device between
the other two entries; :func:`outliers_ref` is a float64 brute force.  Three departures from PCL: the
statistical test searches the ball only, where PCL's k-d tree search is unbounded (a voxel with fewer
than ``k`` neighbours in the ball averages those it has); the query voxel is not its own neighbour
(PCL's radius search counts it, and its SOR asks for ``k + 1`` to skip it); and the arithmetic is
integer (distances in 2^-16 m, rounded), with both tests available at once.

Not here: a radius that grows with range (DROR), filtering the unthinned cloud, averaging or carrying the other fields, ``filter_field_name`` limits and ``leaf_layout``,
feeding the thinned cloud into the detectors or the other side outputs, tf, k-nearest search,
viewpoints other than the origin, normals of the unthinned cloud.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native
from ..ros import msgs
from . import cluster as C
from .cloud_common import CloudLayout, CloudStager, _align, cloud_bytes, cloud_xyzi, fields_f32, plan_staging
from .laser_scan import _number
from .range2d import INT31

MAX_FRAMES = 64  # clouds per launch
MAX_POINTS = 2 ** 24  # of one cloud
MAX_TABLE = 2 ** 30  # bytes of one launch's hash tables
LEAF_MIN, LEAF_MAX = 0.01, 100.0
BIAS = 2 ** 20  # added to a voxel index in the key
QC, QI = 65536, 4096  # units per metre of the coordinate sums, per unit of the intensity sums
I_LIMIT = 65536.0  # an intensity is clamped to this in magnitude
SLOT = 48  # bytes of a table slot: key, four int64 sums, count, first point
BLOCK = 256  # points per block of the device's counts
RECORD = 16  # bytes of an output record, and of a voxel's normal and curvature
RADIUS_MIN, RADIUS_MAX = 0.02, 4.0  # of the normals' ball, metres
RADIUS_LEAVES = 4  # the ball's radius is at most this many of the smallest leaf: at most 10^3 neighbours
SWEEPS = 4  # cyclic Jacobi sweeps of the normals' eigen-solve (docs/precision.md)
CELL_SLOT = 16  # bytes of a slot of the normals' cell table: key, count, start
OUTLIER_NEIGHBORS = 1000  # the most outlier_min_neighbors: what a ball of RADIUS_LEAVES leaves can hold
OUTLIER_K = 16  # the most outlier_mean_k: the squared distances a lane keeps in registers (32 VGPRs)
OUTLIER_STDDEV = 10.0  # the most outlier_stddev
# The launch's variants as they are run (``profiles/voxel_downsample/README.md`` has the measurements).
DEFAULTS = {"wave": True, "lds": True, "saved": True}
NORMALS_DEFAULTS = {"stage": False}  # (``profiles/voxel_normals/README.md``)


def device_enabled() -> bool:
    """``TCA_DEVICE_VOXEL=0`` keeps the definition on GPU engines too."""
    return os.environ.get("TCA_DEVICE_VOXEL", "1") != "0"


# ----------------------------------------------------------------------------- options
@dataclass(frozen=True)
class VoxelOptions:
    leaf: object = 0.2  # one number, or (lx, ly, lz)
    min_points: int = 1
    normal_radius: float = 0.0  # metres; 0: no normals
    outlier_radius: float = 0.0  # metres; 0: no outlier removal.  The ball of both tests below (K36)
    outlier_min_neighbors: int = 0  # the radius test: kept from this many neighbours in the ball; 0: off
    outlier_mean_k: int = 0  # the statistical test over the mean distance to this many nearest neighbours; 0: off
    outlier_stddev: float = 1.0  # ... kept up to this many standard deviations above the cloud's mean

    def _radius(self, name: str, sides) -> float:
        r = _number(name, getattr(self, name))
        if r != 0:
            if not np.float32(RADIUS_MIN) <= np.float32(r) <= np.float32(RADIUS_MAX):
                raise ValueError(f"{name} must be 0 (off) or lie within {RADIUS_MIN}..{RADIUS_MAX:g} m, got {r!r}")
            if not max(self.l32) <= np.float32(r) <= np.float32(RADIUS_LEAVES) * min(self.l32):
                raise ValueError(f"{name} must lie between the largest leaf and {RADIUS_LEAVES} times the smallest "
                                 f"({max(sides):g}..{RADIUS_LEAVES * min(sides):g} m), got {r!r}")
        object.__setattr__(self, name, r)
        return r

    def __post_init__(self):
        v = self.leaf
        if isinstance(v, (tuple, list)):
            if len(v) != 3:
                raise ValueError(f"leaf must be one number or (lx, ly, lz), got {v!r}")
            sides = tuple(_number("leaf", s) for s in v)
        else:
            sides = (_number("leaf", v),) * 3
        for s in sides:
            if not np.float32(LEAF_MIN) <= np.float32(s) <= np.float32(LEAF_MAX):
                raise ValueError(f"leaf must lie within {LEAF_MIN}..{LEAF_MAX:g} m on every axis, got {v!r}")
        object.__setattr__(self, "leaf", sides)
        C._count("min_points", self.min_points, 1, 2 ** 31 - 1)
        self._radius("normal_radius", sides)
        r = self._radius("outlier_radius", sides)
        try:
            n = C._count("outlier_min_neighbors", self.outlier_min_neighbors, 0, OUTLIER_NEIGHBORS)
            k = C._count("outlier_mean_k", self.outlier_mean_k, 0, OUTLIER_K)
        except ValueError as e:
            raise ValueError(f"{e} (0: off)") from None
        a = _number("outlier_stddev", self.outlier_stddev)
        if not 0 <= a <= OUTLIER_STDDEV:
            raise ValueError(f"outlier_stddev must lie within 0..{OUTLIER_STDDEV:g}, got {a!r}")
        object.__setattr__(self, "outlier_stddev", a)
        if r == 0 and (n or k):
            raise ValueError(f"{'outlier_min_neighbors' if n else 'outlier_mean_k'} needs outlier_radius, the ball it searches")
        if r != 0 and not (n or k):
            raise ValueError("outlier_radius needs a test: outlier_min_neighbors or outlier_mean_k")

    @property
    def normals(self) -> bool:
        return self.normal_radius > 0

    @property
    def radius_q(self) -> int:
        """The ball's radius in units of 2^-16 m."""
        return int(np.rint(np.float32(self.normal_radius) * np.float32(QC)))

    @property
    def outliers(self) -> bool:
        return self.outlier_radius > 0

    @property
    def outlier_radius_q(self) -> int:
        """The outlier tests' radius in units of 2^-16 m."""
        return int(np.rint(np.float32(self.outlier_radius) * np.float32(QC)))

    @property
    def l32(self) -> Tuple[np.float32, np.float32, np.float32]:
        return tuple(np.float32(s) for s in self.leaf)


# ------------------------------------------------------------------------- definition
def _columns(points) -> np.ndarray:
    p = np.asarray(points, np.float32)
    p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)
    if len(p) > MAX_POINTS:
        raise ValueError(f"{len(p)} points in a cloud: at most {MAX_POINTS}")
    return p


def _pack(idx: Sequence[np.ndarray]) -> np.ndarray:
    ix, iy, iz = (i.astype(np.int64) + BIAS for i in idx)
    return (iz << 42) | (iy << 21) | ix


def keys_numpy(points, opts: VoxelOptions) -> Tuple[np.ndarray, np.ndarray]:
    """The per-point half of the definition → ``(key [N] int64, valid [N] bool)``; the key is -1
    where the point is not valid."""
    p = _columns(points)
    lim = np.float32(C.LIMIT)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (np.abs(p[:, :3]) <= lim).all(1)  # (a NaN compares false; an infinity is too large)
        idx = [np.floor((np.where(valid, p[:, j], np.float32(0)) / l).astype(np.float32)) for j, l in enumerate(opts.l32)]
    return np.where(valid, _pack(idx), -1), valid


def quantised(points) -> np.ndarray:
    """``int64 [N, 4]``: the integers a point adds to its voxel's sums (an invalid point's are not read)."""
    p = _columns(points)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.zeros((len(p), 4), np.int64)
        ok = np.abs(p[:, :3]) <= np.float32(C.LIMIT)
        q[:, :3] = np.rint(np.where(ok, p[:, :3], np.float32(0)) * np.float32(QC))
        if p.shape[1] >= 4:
            i = np.where(np.isnan(p[:, 3]), np.float32(0), np.clip(p[:, 3], np.float32(-I_LIMIT), np.float32(I_LIMIT)))
            q[:, 3] = np.rint(i.astype(np.float32) * np.float32(QI))
    return q


def _voxels(key: np.ndarray, valid: np.ndarray):
    """→ ``(keys [V], first [V], count [V], order, starts)`` of the distinct valid keys; ``order``
    sorts the valid points by voxel, ``starts`` is where each voxel's run begins in it."""
    at = np.nonzero(valid)[0]
    uniq, inv, count = np.unique(key[at], return_inverse=True, return_counts=True)
    order = np.argsort(inv, kind="stable")
    starts = np.cumsum(count) - count
    return uniq, at[order][starts] if len(uniq) else at[:0], count, at[order], starts


def downsample_numpy(points, opts: VoxelOptions) -> np.ndarray:
    """The definition → ``float32 [K, 4]`` (x, y, z, intensity), one row per kept voxel in the order
    of its first point.  ``points``: [N, >=3 or 4] float32."""
    key, valid = keys_numpy(points, opts)
    uniq, first, count, order, starts = _voxels(key, valid)
    if not len(uniq):
        return np.zeros((0, 4), np.float32)
    sums = np.add.reduceat(quantised(points)[order], starts, axis=0)  # int64: exact
    keep = np.nonzero(count >= opts.min_points)[0]
    keep = keep[np.argsort(first[keep], kind="stable")]
    den = count[keep, None] * np.array([QC, QC, QC, QI], np.int64)
    return (sums[keep].astype(np.float64) / den.astype(np.float64)).astype(np.float32)


def keys_ref(points, opts: VoxelOptions) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Float64, point by point and with nothing of the definition's code → ``(key [N] int64, valid
    [N] bool, odd [N] bool)``: the index is ``floor(float64(v) / float64(f32(leaf)))``; ``odd`` marks
    the valid points whose ``d`` lies within ``cluster.CELL_BAND`` (relative, at least of 1) of an
    integer on any axis."""
    p = np.asarray(points, np.float32)
    rows = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)[:, :3].astype(np.float64).tolist()
    leaf = [float(l) for l in opts.l32]
    key, valid, odd = np.full(len(rows), -1, np.int64), np.zeros(len(rows), bool), np.zeros(len(rows), bool)
    for n, xyz in enumerate(rows):
        if not all(abs(v) <= C.LIMIT for v in xyz):  # (a NaN compares false; an infinity is too large)
            continue
        d = [v / l for v, l in zip(xyz, leaf)]
        ix, iy, iz = (math.floor(t) + BIAS for t in d)
        key[n], valid[n] = iz * 2 ** 42 + iy * 2 ** 21 + ix, True
        odd[n] = any(abs(t - round(t)) <= C.CELL_BAND * max(abs(t), 1.0) for t in d)
    return key, valid, odd


def downsample_ref(points, opts: VoxelOptions):
    """Float64 brute force → ``(centroids float64 [K, 4], keys int64 [K], band int64 [...])``: a
    loop over the points that gathers each voxel's values in a dict (which keeps first-point order)
    and takes plain float64 means of the voxels of ``min_points`` points or more, with the voxels'
    keys.  ``band`` holds the keys of the voxels float32 may legitimately fill differently: every
    voxel that holds, or in float32 holds, an ``odd`` point of :func:`keys_ref`.  ``float32(leaf)``
    is an input of both evaluations."""
    p = np.asarray(points, np.float32)
    p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)
    key, valid, odd = keys_ref(p, opts)
    band = np.unique(np.concatenate([key[odd], keys_numpy(p, opts)[0][odd]]))
    members = {}
    for n, row in enumerate(p.astype(np.float64).tolist()):
        if valid[n]:
            i = row[3] if len(row) >= 4 and not math.isnan(row[3]) else 0.0
            members.setdefault(int(key[n]), []).append(row[:3] + [min(max(i, -I_LIMIT), I_LIMIT)])
    kept = [(k, m) for k, m in members.items() if len(m) >= opts.min_points]
    mean = [[math.fsum(r[j] for r in m) / len(m) for j in range(4)] for _, m in kept]
    return np.array(mean, np.float64).reshape(-1, 4), np.array([k for k, _ in kept], np.int64), band


# ----------------------------------------------------------------------------- normals
NAN_ROW = np.full(4, np.uint32(0x7FC00000)).view(np.float32)  # a voxel with fewer than three neighbours


def _pairs(q: np.ndarray, R: int) -> Tuple[np.ndarray, np.ndarray]:
    """Every ordered pair ``(a, b)`` of rows of ``q`` (int64 [K, 3]) whose cells of side ``R`` touch —
    a superset of the pairs within ``R`` — grouped by ``a``.  The cell index is a floor division."""
    cell = q // R + BIAS
    key = (cell[:, 2] << 42) | (cell[:, 1] << 21) | cell[:, 0]
    order = np.argsort(key, kind="stable")
    sk = key[order]
    a_all, b_all = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                want = key + ((dz << 42) + (dy << 21) + dx)
                lo, hi = np.searchsorted(sk, want, "left"), np.searchsorted(sk, want, "right")
                n = hi - lo
                a = np.repeat(np.arange(len(q)), n)
                a_all.append(a)
                b_all.append(order[np.arange(len(a)) - np.repeat(np.cumsum(n) - n, n) + lo[a]])
    return np.concatenate(a_all), np.concatenate(b_all)


def moments_numpy(rows, opts: VoxelOptions) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The integer half of the normals' definition → ``(m [K], Sd [K, 3], Sdd [K, 6])``, int64: per
    voxel the neighbours of its closed ball (itself included), the sums of their offsets ``d`` and of
    ``d_i d_j`` for ij = xx, xy, xz, yy, yz, zz, in units of 2^-16 m."""
    c = _columns(rows)[:, :3]
    q = np.rint(c * np.float32(QC)).astype(np.int64)
    R = opts.radius_q
    a, b = _pairs(q, R)
    d = q[b] - q[a]
    near = (d * d).sum(1) <= R * R
    a, d = a[near], d[near]
    K = len(q)
    # (float64 weights are exact here: every partial sum is an integer below 2^46)
    tot = lambda w: np.bincount(a, w.astype(np.float64), K).astype(np.int64)
    m = np.bincount(a, minlength=K).astype(np.int64)
    Sd = np.stack([tot(d[:, i]) for i in range(3)], 1).reshape(K, 3)
    Sdd = np.stack([tot(d[:, i] * d[:, j]) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], 1).reshape(K, 6)
    return m, Sd, Sdd


def _rotate(app, aqq, apq, arp, arq, vp, vq):
    """One Jacobi rotation of the pair (p, q) on float32 arrays, every operation rounded on its own
    (``docs/precision.md``); where ``apq`` is exactly 0 nothing changes."""
    one, skip = np.float32(1), apq == 0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (apq + apq)
        t = np.where(theta < 0, -one, one) / (np.abs(theta) + np.sqrt(theta * theta + one))  # 0 for an infinite theta
        c = one / np.sqrt(t * t + one)
        s = t * c
        h = t * apq
        new = [app - h, aqq + h, np.zeros_like(apq), c * arp - s * arq, s * arp + c * arq,
               c[:, None] * vp - s[:, None] * vq, s[:, None] * vp + c[:, None] * vq]
    old = [app, aqq, apq, arp, arq, vp, vq]
    return [np.where(skip if o.ndim == 1 else skip[:, None], o, n) for o, n in zip(old, new)]


def eigen_numpy(cov: np.ndarray, sweeps: int = SWEEPS) -> Tuple[np.ndarray, np.ndarray]:
    """Cyclic Jacobi in float32 on ``cov`` [K, 6] (xx, xy, xz, yy, yz, zz) → ``(diagonal [K, 3],
    vectors [K, 3, 3])``, column j of ``vectors`` belonging to entry j of the diagonal.  The pairs of
    a sweep are (0, 1), (0, 2), (1, 2)."""
    a00, a01, a02, a11, a12, a22 = (cov[:, j].astype(np.float32) for j in range(6))
    K = len(cov)
    v0, v1, v2 = (np.tile(np.eye(3, dtype=np.float32)[j], (K, 1)) for j in range(3))  # the columns
    for _ in range(sweeps):
        a00, a11, a01, a02, a12, v0, v1 = _rotate(a00, a11, a01, a02, a12, v0, v1)
        a00, a22, a02, a01, a12, v0, v2 = _rotate(a00, a22, a02, a01, a12, v0, v2)
        a11, a22, a12, a01, a02, v1, v2 = _rotate(a11, a22, a12, a01, a02, v1, v2)
    return np.stack([a00, a11, a22], 1), np.stack([v0, v1, v2], 2)


def normals_numpy(rows, opts: VoxelOptions, sweeps: int = SWEEPS) -> np.ndarray:
    """The normals' definition → ``float32 [K, 4]`` (normal_x, normal_y, normal_z, curvature) of one
    cloud's rows ``[K, >=3]``; four quiet NaNs for a voxel with fewer than three neighbours."""
    c = np.ascontiguousarray(_columns(rows)[:, :3])
    if not len(c):
        return np.zeros((0, 4), np.float32)
    m, Sd, Sdd = moments_numpy(c, opts)
    fm, fd = m.astype(np.float64), Sd.astype(np.float64)
    ij = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    cov = np.stack([Sdd[:, k].astype(np.float64) - (fd[:, i] * fd[:, j]) / fm for k, (i, j) in enumerate(ij)], 1)
    lam, vec = eigen_numpy(cov.astype(np.float32), sweeps)
    low = np.argmin(lam, 1)  # (the first of equal entries)
    n = vec[np.arange(len(c)), :, low]
    with np.errstate(all="ignore"):
        n = n / np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])[:, None]
        away = n[:, 0] * c[:, 0] + n[:, 1] * c[:, 1] + n[:, 2] * c[:, 2] > 0
        n = np.where(away[:, None], -n, n)
        total = lam[:, 0] + lam[:, 1] + lam[:, 2]
        least = lam[np.arange(len(c)), low]
        least = np.where(least < 0, np.float32(0), least)
        curv = np.where(total > 0, least / total, np.float32(0))
    out = np.concatenate([n, curv[:, None]], 1).astype(np.float32)
    out[m < 3] = NAN_ROW
    return out


def normals_ref(rows, opts: VoxelOptions, g: float = 0.05):
    """Float64 brute force with nothing of the definition's code → ``(normals float64 [K, 4], m int64
    [K], odd bool [K], flat bool [K])``: pairwise distances on ``float64(rows)`` against
    ``float64(float32(r))``, the plain covariance about the neighbours' mean, ``np.linalg.eigh``.
    ``odd``: a pair of the voxel lies within 2^-14 m of the radius (a ``rint`` moves a coordinate by at
    most 2^-17 m, a distance by at most sqrt(3) 2^-16 m), so the quantised ball may hold another set;
    ``flat``: fewer than three neighbours, or ``(l1 - l0) < g l2``: no well-conditioned normal."""
    p = np.asarray(rows, np.float32)
    p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)[:, :3].astype(np.float64)
    r = float(np.float32(opts.normal_radius))
    K = len(p)
    out, m = np.full((K, 4), np.nan), np.zeros(K, np.int64)
    odd, flat = np.zeros(K, bool), np.ones(K, bool)
    for a in range(K):
        dist = np.sqrt(((p - p[a]) ** 2).sum(1))
        odd[a] = (np.abs(dist - r) <= 2.0 ** -14).any()
        nb = p[dist <= r]
        m[a] = len(nb)
        if len(nb) < 3:
            continue
        e = nb - nb.mean(0)
        lam, vec = np.linalg.eigh(e.T @ e)
        n = vec[:, 0] if vec[:, 0] @ p[a] <= 0 else -vec[:, 0]
        out[a] = [*n, max(lam[0], 0.0) / lam.sum() if lam.sum() > 0 else 0.0]
        flat[a] = (lam[1] - lam[0]) < g * lam[2]
    return out, m, odd, flat


# ---------------------------------------------------------------------------- outliers
def outlier_scores_numpy(rows, opts: VoxelOptions) -> Tuple[np.ndarray, np.ndarray, float]:
    """The integer half of the outliers' definition → ``(found int64 [K], mean int64 [K], thr)``: per
    voxel the neighbours of its closed ball (itself excluded) and, with ``outlier_mean_k``, the rounded
    mean of the rounded distances to the ``min(k, found)`` nearest in units of 2^-16 m (0 without a
    neighbour); ``thr`` the statistical test's float64 threshold in the same units, ``inf`` where the
    test is off or fewer than two voxels have a neighbour."""
    c = _columns(rows)[:, :3]
    K, k = len(c), opts.outlier_mean_k
    q = np.rint(c * np.float32(QC)).astype(np.int64)
    R = opts.outlier_radius_q
    a, b = _pairs(q, R)
    d = q[b] - q[a]
    d2 = (d * d).sum(1)
    near = (d2 <= R * R) & (a != b)
    a, d2 = a[near], d2[near]
    found = np.bincount(a, minlength=K).astype(np.int64)
    mean, thr = np.zeros(K, np.int64), math.inf
    if not k:
        return found, mean, thr
    order = np.lexsort((d2, a))  # by voxel, its squared distances ascending: only the values of the first k are used
    a, d2 = a[order], d2[order]
    first = np.arange(len(a)) - (np.cumsum(found) - found)[a] < k  # the rank inside the voxel's run
    e = np.rint(np.sqrt(d2[first].astype(np.float64))).astype(np.int64)  # D^2 < 2^37: exact, the root correctly rounded
    total = np.bincount(a[first], e.astype(np.float64), K)  # (exact: at most 16 * 2^18)
    has = found >= 1
    mean[has] = np.rint(total[has] / np.minimum(k, found[has]).astype(np.float64)).astype(np.int64)
    n = int(has.sum())
    if n >= 2:
        s1, s2, fn = np.float64(int(mean[has].sum())), np.float64(int((mean[has] * mean[has]).sum())), np.float64(n)
        mu = s1 / fn
        var = (s2 - s1 * s1 / fn) / (fn - np.float64(1))  # PCL's sample variance
        thr = float(mu + np.float64(opts.outlier_stddev) * np.sqrt(max(var, np.float64(0))))
    return found, mean, thr


def outliers_numpy(rows, opts: VoxelOptions) -> np.ndarray:
    """The outliers' definition → the keep mask ``bool [K]`` of one cloud's rows ``[K, >=3]``: a voxel
    without a neighbour goes; the radius test keeps ``found >= outlier_min_neighbors``, the statistical
    test ``float64(mean) <= thr``, and with both on a voxel has to pass both."""
    if not len(_columns(rows)):
        return np.zeros(0, bool)
    found, mean, thr = outlier_scores_numpy(rows, opts)
    keep = found >= max(opts.outlier_min_neighbors, 1)
    return keep & (mean.astype(np.float64) <= thr) if opts.outlier_mean_k else keep


# what float64 may legitimately decide differently: a mean within this many metres of the threshold — four times the
# worst |mean - mean_ref| + |thr - thr_ref| measured on the test scenes (docs/precision.md)
OUTLIER_MARGIN = 4 * 2.31e-5


def outlier_scores_ref(rows, opts: VoxelOptions):
    """Float64 brute force with nothing of the definition's code → ``(found int64 [K], mean float64 [K],
    thr, band bool [K])`` in metres: pairwise distances on ``float64(rows)`` against
    ``float64(float32(r))``, ``np.partition`` for the nearest, ``np.std(ddof=1)``; ``band``: a pair of the
    voxel lies within 2^-14 m of the radius."""
    p = np.asarray(rows, np.float32)
    p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)[:, :3].astype(np.float64)
    r, k, K = float(np.float32(opts.outlier_radius)), opts.outlier_mean_k, len(p)
    found, mean, band = np.zeros(K, np.int64), np.zeros(K), np.zeros(K, bool)
    for a in range(K):
        dist = np.delete(np.sqrt(((p - p[a]) ** 2).sum(1)), a)
        band[a] = (np.abs(dist - r) <= 2.0 ** -14).any()
        nb = dist[dist <= r]
        found[a] = len(nb)
        if k and len(nb):
            f = min(k, len(nb))
            mean[a] = np.partition(nb, f - 1)[:f].mean()
    has = found >= 1
    thr = float(mean[has].mean() + opts.outlier_stddev * np.std(mean[has], ddof=1)) if k and has.sum() >= 2 else math.inf
    return found, mean, thr, band


def outliers_ref(rows, opts: VoxelOptions, margin: float = OUTLIER_MARGIN) -> Tuple[np.ndarray, np.ndarray]:
    """→ ``(keep bool [K], odd bool [K])`` of :func:`outlier_scores_ref`; ``odd``: the voxel's ball may
    hold another set after the ``rint`` of its coordinates (``band``), or its mean lies within ``margin``
    of the threshold."""
    found, mean, thr, band = outlier_scores_ref(rows, opts)
    keep = found >= max(opts.outlier_min_neighbors, 1)
    if opts.outlier_mean_k:
        keep &= mean <= thr
        band = band | ((found >= 1) & (np.abs(mean - thr) <= margin))
    return keep, band


# ---------------------------------------------------------------------------- messages
def downsample_message(cloud, rows: np.ndarray) -> msgs.PointCloud2:
    """The rows as an unorganised, little-endian ``PointCloud2`` with the cloud's header.  Rows of
    four columns: 16-byte records, FLOAT32 x, y, z at 0, 4, 8 and, when the input cloud has one,
    ``intensity`` at 12 (the dword is there either way), dense.  Rows of eight (normals on): 32-byte
    records with FLOAT32 ``normal_x``, ``normal_y``, ``normal_z``, ``curvature`` at 16, 20, 24, 28
    behind them, and ``is_dense`` False when a voxel has no normal (NaNs)."""
    a = np.ascontiguousarray(rows, "<f4")
    a = a.reshape(-1, a.shape[-1] if a.ndim > 1 and a.shape[-1] == 8 else 4)
    step = 4 * a.shape[1]
    fields = [msgs.PointField("x", 0, 7, 1), msgs.PointField("y", 4, 7, 1), msgs.PointField("z", 8, 7, 1)]
    if any(f.name == "intensity" for f in cloud.fields):
        fields.append(msgs.PointField("intensity", 12, 7, 1))
    if step > RECORD:
        fields += [msgs.PointField(n, RECORD + 4 * j, 7, 1) for j, n in enumerate(("normal_x", "normal_y", "normal_z", "curvature"))]
    dense = step == RECORD or not bool(np.isnan(a[:, 4:]).any())
    return msgs.PointCloud2(header=cloud.header, height=1, width=len(a), fields=fields, is_bigendian=False,
                            point_step=step, row_step=step * len(a), data=a.tobytes(), is_dense=dense)


def downsample_cloud_numpy(cloud, opts: VoxelOptions, lay: Optional[CloudLayout] = None) -> np.ndarray:
    """One cloud through the definition → its rows, ``[K, 8]`` with normals on; with the outlier filter
    on the kept rows alone, and the normals of those."""
    rows = downsample_numpy(cloud_xyzi(cloud, lay), opts)
    if opts.outliers:
        rows = rows[outliers_numpy(rows, opts)]
    return np.concatenate([rows, normals_numpy(rows, opts)], 1) if opts.normals else rows


# --------------------------------------------------------------------------------- GPU
def slots_for(n: int) -> int:
    """The default table size of a cloud of ``n`` points: the power of two at or above ``2 n``."""
    return max(2, 1 << (2 * int(n) - 1).bit_length()) if n > 0 else 2


def most_clouds(n: int) -> int:
    """How many clouds of ``n`` points fit one launch: 64, and :data:`MAX_TABLE` bytes of tables."""
    return max(1, min(MAX_FRAMES, MAX_TABLE // (SLOT * slots_for(n))))


def parts(idx, clouds):
    """The cut of a layout's clouds into launches of less than 2^31 staged bytes and of at most
    :func:`most_clouds` of the largest cloud among them: 64 clouds, and :data:`MAX_TABLE` bytes of
    default-sized tables (a single cloud is never refused here)."""
    part, size, big = [], 0, 0
    for i in idx:
        nb = _align(len(clouds[i].data)) + 16
        n = int(clouds[i].width) * int(clouds[i].height)
        if part and (len(part) >= most_clouds(max(big, n)) or size + nb >= INT31):
            yield part
            part, size, big = [], 0, 0
        part.append(i)
        size += nb
        big = max(big, n)
    if part:
        yield part


@dataclass
class VoxelCall:
    """One prepared launch: device views of its inputs, workspace and output."""
    data: torch.Tensor
    data_bytes: int
    frame_off: torch.Tensor
    frame_n: torch.Tensor
    table: torch.Tensor  # uint8 view of the clouds' tables, one after the other, 48 bytes a slot
    memo: torch.Tensor  # uint8 view of int32, one per staged point: its slot when it writes its voxel's record, else -1
    blocks: torch.Tensor  # uint8 view of int32 [B][nblk + 1]: per block its writers, then its offset
    out: torch.Tensor  # uint8: cloud b's records from 16 * (points before it), then counts int32 [B]
    layout: CloudLayout
    batch: int
    ns: Tuple[int, ...]
    slots: Tuple[int, ...]
    opts: VoxelOptions
    normals: Optional[torch.Tensor] = None  # uint8, with normals on: 16 bytes per record at the record's index
    kept: Optional[torch.Tensor] = None  # uint8, with the outlier filter on: the kept records, laid out like ``out``'s

    @property
    def records(self) -> torch.Tensor:
        """The buffer that holds the published records: ``kept`` behind the outlier filter, else ``out``."""
        return self.out if self.kept is None else self.kept

    @property
    def table_bytes(self) -> int:
        return SLOT * sum(self.slots)

    @property
    def memo_bytes(self) -> int:
        return 4 * sum(self.ns)

    @property
    def blocks_bytes(self) -> int:
        return 4 * self.batch * ((max(self.ns, default=0) + BLOCK - 1) // BLOCK + 1)

    @property
    def rows_bytes(self) -> int:
        return RECORD * sum(self.ns)

    @property
    def out_bytes(self) -> int:
        return self.rows_bytes + 4 * self.batch

    @property
    def counts(self) -> torch.Tensor:
        return self.out[self.rows_bytes:self.out_bytes].view(torch.int32)


def launch(c: VoxelCall, stream=None, wave: Optional[bool] = None, lds: Optional[bool] = None,
           saved: Optional[bool] = None, stage: Optional[bool] = None) -> None:
    """The launch alone (five kernels on ``stream``, with the outlier filter on the eight of
    ``tca_voxel_outliers`` behind them and with normals on the five of ``tca_voxel_normals`` behind
    those): no allocation, no copy, no sync.  ``wave``:
    runs of equal voxels of a wave are reduced with shuffles first; ``lds``: a workgroup gathers its
    span of points in a table in LDS; ``saved``: the scatter reads the slot the count pass kept
    instead of probing the table again.  None: :data:`DEFAULTS`.  ``stage``: the normals' fit stages
    the candidates of a cell's 27 neighbours through LDS once per cell instead of every lane probing
    and reading for itself (measured slower on the sweep: off); None: :data:`NORMALS_DEFAULTS`."""
    wave, lds, saved = (DEFAULTS[k] if v is None else v for k, v in (("wave", wave), ("lds", lds), ("saved", saved)))
    p = _native.ptr
    o, r = c.layout.offsets, c.opts
    ns, slots = np.asarray(c.ns, np.int32), np.asarray(c.slots, np.int32)
    _native.call("tca_voxel_downsample", p(c.data), c.data_bytes, p(c.frame_off), p(c.frame_n), ns.ctypes.data,
                 slots.ctypes.data, c.batch, c.layout.point_step, o[0], o[1], o[2], o[3], *(float(l) for l in r.l32),
                 int(r.min_points), 1 if wave else 0, 1 if lds else 0, 1 if saved else 0, p(c.table), c.table_bytes,
                 p(c.memo), c.memo_bytes, p(c.blocks), c.blocks_bytes, p(c.out), c.rows_bytes, p(c.counts),
                 _native.stream_ptr(stream))
    if r.outliers:
        launch_outliers(c, stream)
    if r.normals:
        launch_normals(c, stream, stage)


def launch_outliers(c: VoxelCall, stream=None) -> None:
    """``tca_voxel_outliers`` alone, behind a ``tca_voxel_downsample`` of the same call on ``stream``: it
    reads the records and the counts on the device, writes the kept records to ``c.kept`` and the
    survivors of every cloud over its count; the leaf table, the memo and the block counts, all dead
    after the scatter, are its workspace."""
    p, r = _native.ptr, c.opts
    ns, slots = np.asarray(c.ns, np.int32), np.asarray(c.slots, np.int32)
    _native.call("tca_voxel_outliers", p(c.out), c.rows_bytes, p(c.counts), ns.ctypes.data, slots.ctypes.data, c.batch,
                 r.outlier_radius_q, int(r.outlier_min_neighbors), int(r.outlier_mean_k), float(r.outlier_stddev),
                 p(c.table), c.table_bytes, p(c.memo), c.memo_bytes, p(c.blocks), c.blocks_bytes, p(c.kept),
                 c.rows_bytes, _native.stream_ptr(stream))


def launch_normals(c: VoxelCall, stream=None, stage: Optional[bool] = None) -> None:
    """``tca_voxel_normals`` alone, behind a ``tca_voxel_downsample`` (and the outlier filter, when on)
    of the same call on ``stream``: it reads the records and the counts on the device, and the leaf
    table, dead after the scatter, is the cell lists' workspace."""
    stage = NORMALS_DEFAULTS["stage"] if stage is None else stage
    p = _native.ptr
    ns, slots = np.asarray(c.ns, np.int32), np.asarray(c.slots, np.int32)
    _native.call("tca_voxel_normals", p(c.records), c.rows_bytes, p(c.counts), ns.ctypes.data, slots.ctypes.data,
                 c.batch, c.opts.radius_q, 1 if stage else 0, p(c.table), c.table_bytes, p(c.normals), c.rows_bytes,
                 _native.stream_ptr(stream))


def layout_device_ok(lay: CloudLayout) -> bool:
    """What ``tca_voxel_downsample`` reads in place: little-endian FLOAT32 x, y, z inside the
    record, and an intensity that is FLOAT32 too or absent."""
    return fields_f32(lay, (0, 1, 2, 3) if lay.offsets[3] >= 0 else (0, 1, 2))


def rows_of(host: np.ndarray, c: VoxelCall, normals: Optional[np.ndarray] = None,
            kept: Optional[np.ndarray] = None) -> List[np.ndarray]:
    """Per cloud its rows ``float32 [K, 4]`` (copies) of a launch's output bytes (``out_bytes`` of them);
    with the bytes of its normals (``rows_bytes`` of them), ``[K, 8]``.  ``kept``: the bytes of the
    outlier filter's records (``rows_bytes`` of them), read in place of the output's; the counts are the
    output's either way."""
    counts = host[c.rows_bytes:c.out_bytes].view("<i4")
    host = host if kept is None else kept
    res, at = [], 0
    for b, n in enumerate(c.ns):
        k = int(counts[b])
        cut = slice(RECORD * at, RECORD * (at + k))
        rows = host[cut].view("<f4").reshape(k, 4)
        res.append(rows.copy() if normals is None else np.concatenate([rows, normals[cut].view("<f4").reshape(k, 4)], 1))
        at += n
    return res


class VoxelDownsampler(CloudStager):
    """Thins clouds on a voxel grid: on a GPU with ``tca_voxel_downsample`` (its own workspace,
    stream and pinned staging: one H2D of the payloads per launch group of same-layout clouds, one
    launch, the counts back, then only the used part of every cloud's slot), on the CPU — and with
    ``TCA_DEVICE_VOXEL=0`` — with the definition.  Clouds the kernel does not take (non-FLOAT32 or
    big-endian x, y, z, an intensity that is present but not FLOAT32) run the definition with one
    warning.  ``wave``, ``lds``, ``saved``: the launch's variants, None for :data:`DEFAULTS`."""

    wave = lds = saved = stage = None

    def prepare(self, payloads: Sequence, ns: Sequence[int], layout: CloudLayout, opts: VoxelOptions, stream=None,
                misalign: int = 0, slots: Optional[Sequence[int]] = None) -> VoxelCall:
        """Stage one batch (``payloads[b]``: the bytes of ``ns[b]`` points of ``layout``) in pinned
        memory and upload it with one H2D copy on ``stream``.  ``misalign``: start every payload
        this many bytes past a 16-byte boundary; ``slots``: the table size of every cloud (a power
        of two at or above its points) in place of :func:`slots_for`."""
        if not layout_device_ok(layout):
            raise ValueError(f"tca_voxel_downsample does not take this layout: {layout}")
        B = len(payloads)
        ns = [int(n) for n in ns]
        if not 1 <= B <= MAX_FRAMES:
            raise ValueError(f"{B} clouds do not fit one call (1..{MAX_FRAMES}): split the batch")
        if max(ns) > MAX_POINTS:
            raise ValueError(f"{max(ns)} points in a cloud: at most {MAX_POINTS}")
        slots = [slots_for(n) for n in ns] if slots is None else [int(s) for s in slots]
        if len(slots) != B or any(s < max(n, 2) or s & (s - 1) for s, n in zip(slots, ns)):
            raise ValueError(f"slots must be one power of two per cloud, at or above its points: {slots} for {ns}")
        data_bytes = plan_staging(ns, layout.point_step, misalign, ()).data_bytes  # (refused before any allocation)
        if data_bytes >= INT31 or (B > 1 and SLOT * sum(slots) > MAX_TABLE):
            raise ValueError(f"{data_bytes} payload bytes and {SLOT * sum(slots)} table bytes do not fit one call: "
                             "split the batch")
        dev, plan, view = self._stage("voxel_in", payloads, ns, layout.point_step, misalign, [], stream)
        c = VoxelCall(data=dev, data_bytes=data_bytes, frame_off=view("frame_off", B, torch.int64),
                      frame_n=view("frame_n", B, torch.int32), table=None, memo=None, blocks=None, out=None,
                      layout=layout, batch=B, ns=tuple(ns), slots=tuple(slots), opts=opts)
        c.table = self._device_buf("voxel_table", c.table_bytes)
        c.memo = self._device_buf("voxel_memo", c.memo_bytes)
        c.blocks = self._device_buf("voxel_blocks", c.blocks_bytes)
        c.out = self._device_buf("voxel_out", c.out_bytes)
        if opts.normals:
            c.normals = self._device_buf("voxel_normals", c.rows_bytes)
        if opts.outliers:
            c.kept = self._device_buf("voxel_kept", c.rows_bytes)
        return c

    launch = staticmethod(launch)

    def _fetch_counted(self, c: VoxelCall, st) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """The counts (behind the outlier filter the survivors), a synchronize, then only the used
        records of every cloud's slot, and with normals on the same parts of the normals → the host bytes, laid out like the output, and the
        normals' (None when off)."""
        on = c.normals is not None
        pin = self._pinned("_pin_out", _align(c.out_bytes) + c.rows_bytes if on else c.out_bytes)
        side = pin[_align(c.out_bytes):] if on else None
        with torch.cuda.stream(st):
            pin[c.rows_bytes:c.out_bytes].copy_(c.out[c.rows_bytes:c.out_bytes], non_blocking=True)
        st.synchronize()
        counts = pin.numpy()[c.rows_bytes:c.out_bytes].view("<i4")
        with torch.cuda.stream(st):
            at = 0
            for b, n in enumerate(c.ns):
                lo, hi = RECORD * at, RECORD * (at + int(counts[b]))
                if hi > lo:
                    pin[lo:hi].copy_(c.records[lo:hi], non_blocking=True)
                    if on:
                        side[lo:hi].copy_(c.normals[lo:hi], non_blocking=True)
                at += n
        st.synchronize()
        return pin.numpy()[:c.out_bytes], side.numpy()[:c.rows_bytes] if on else None

    def _run_device(self, payloads, ns, layout, opts):
        """→ per frame its rows."""
        with torch.cuda.device(self.device):
            st = self._own_stream()
            c = self.prepare(payloads, ns, layout, opts, st)
            launch(c, st, self.wave, self.lds, self.saved, self.stage)
            host, normals = self._fetch_counted(c, st)
            return rows_of(host, c, normals)

    # ---------------------------------------------------------------------- API
    def downsample(self, clouds: Sequence, opts: VoxelOptions) -> List[np.ndarray]:
        """Per cloud its rows ``float32 [K, 4]``, in input order; ``[K, 8]`` with ``opts.normal_radius``:
        normal x, y, z and curvature behind them (``tca_voxel_normals`` in the same launch group)."""
        return self._per_cloud(
            clouds, lambda i, lay: layout_device_ok(lay),
            lambda i, lay: downsample_cloud_numpy(clouds[i], opts, lay),
            lambda lay, part: (*cloud_bytes(clouds, part), lay, opts), self._run_device,
            lambda i, lay: f"VoxelDownsampler: tca_voxel_downsample takes little-endian FLOAT32 x, y, z and intensity "
                           f"(got {lay}); such clouds are downsampled on the host",
            device=self.gpu and device_enabled(), parts=parts)

    def messages(self, clouds: Sequence, opts: VoxelOptions) -> List[msgs.PointCloud2]:
        """Per cloud its downsampled ``PointCloud2`` message."""
        return [downsample_message(c, a) for c, a in zip(clouds, self.downsample(clouds, opts))]
