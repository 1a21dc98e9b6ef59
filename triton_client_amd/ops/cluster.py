"""K31 — the obstacle clusters of a cloud: one box per connected blob of points.

The detectors report the classes they were trained on; a fallen load, an animal or a barrier is in
the obstacle cloud all the same.  What ROS users run ``euclidean_cluster`` or Autoware's
``voxel_grid_based_euclidean_cluster`` for, on a CPU core next to the driver, the driver does here:
per cloud one box message (``clusters``) with a class-agnostic box per cluster of the obstacle points
(``ops/ground.py``, K30, takes the ground out first unless ``remove_ground`` is off).
:func:`cluster_numpy` is the definition, bit for bit (the pattern of ``ops/ground.py``); the HIP
kernel ``tca_cluster`` (``csrc/kernels/cluster.hip``) computes the same outputs from the raw payload,
straight behind ``tca_ground_split`` on the device, and :func:`cluster_ref` is a float64 brute force
with a plain flood fill that also marks the points float32 may legitimately put into another cell
(``docs/precision.md``).

**The grid** is a bird's-eye one: ``W = ceil((x_max - x_min) / cell - 1e-9)`` columns and ``H`` rows
likewise, cell index ``iy * W + ix``.  **Per point** ``(x, y, z)`` as sent, in float32, every
operation rounded on its own, IEEE division (a NaN compares false)::

    valid = |x| <= 512 and |y| <= 512 and z_min <= z <= z_max and |z| <= 512
    dx = (x - float32(x_min)) / float32(cell);  dy likewise
    valid &= dx >= 0 and dx < float32(W) and dy >= 0 and dy < float32(H)
    ix = int(dx); iy = int(dy)                       # truncation
    xi, yi, zi = int32(rint(v * 1024))               # the products are exact, ties to even

**After that, integers only.**  ``cnt[cell]`` is the number of valid points of the cell; a cell is
occupied iff ``cnt >= min_cell_points``; two occupied cells are connected iff they are 8-neighbours.
A component's root is its smallest cell index and its size the sum of ``cnt`` over its cells; it is
kept iff ``min_points <= size <= max_points``.  Kept components are numbered ``k = 0, 1, ...`` in
ascending root order; ``found`` is their number, and the first ``max_clusters`` are reported: per
point ``label`` (``k``, or -1 for a point that is not valid, an unoccupied cell, a dropped component
or ``k >= max_clusters``) and a table of ``min(found, max_clusters)`` rows of 64 bytes
(:data:`TABLE_DTYPE`: the point count, the root, the integer bounds and the integer sums of the
component's points in units of 1/1024 m).  Nothing depends on the order of the points.

Oriented (L-shape) boxes are ``ops/cluster_fit.py`` (K32), which runs behind this op on request
(``fit``).  Not here: tf, tracking the clusters, merging them with the detections, and a per-point
labelled cluster cloud.
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
from . import ground as G
from .cloud_common import CloudLayout, CloudStager, _align, cloud_bytes, cloud_xyzi, plan_staging
from .laser_scan import _number
from .range2d import INT31, U, _xyz

MAX_FRAMES = 64  # clouds per launch
MAX_SIDE = 2048  # columns, rows
MAX_CELLS = 2 ** 22  # of one cloud
MAX_PLANE = 2 ** 24  # cells of one launch
MAX_CLUSTERS = 4096
LIMIT = 512.0  # |x|, |y|, |z| beyond this are not valid
Q = 1024  # integer units per metre
ROW = 64  # bytes of a table row
CELL_BAND = 3 * U  # cluster_ref: how near an integer dx or dy may be taken either way, relative
TABLE_DTYPE = np.dtype([("n", "<i4"), ("root", "<i4"), ("min_x", "<i4"), ("max_x", "<i4"), ("min_y", "<i4"),
                        ("max_y", "<i4"), ("min_z", "<i4"), ("max_z", "<i4"), ("sum_x", "<i8"), ("sum_y", "<i8"),
                        ("sum_z", "<i8"), ("pad", "<i8")])
assert TABLE_DTYPE.itemsize == ROW


def device_enabled() -> bool:
    """``TCA_DEVICE_CLUSTER=0`` keeps the definition on GPU engines too."""
    return os.environ.get("TCA_DEVICE_CLUSTER", "1") != "0"


# ----------------------------------------------------------------------------- options
def _count(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {v!r}")
    return int(v)


@dataclass(frozen=True)
class ClusterOptions:
    cell: float = 0.4
    x_range: Tuple[float, float] = (-80.0, 80.0)
    y_range: Tuple[float, float] = (-80.0, 80.0)
    z_range: Tuple[float, float] = (-512.0, 512.0)
    min_cell_points: int = 1
    min_points: int = 5
    max_points: int = 2 ** 31 - 1
    max_clusters: int = 1024
    remove_ground: bool = True

    def __post_init__(self):
        cell = _number("cell", self.cell)
        if not 0.05 <= cell <= 10.0:
            raise ValueError(f"cell must be within 0.05..10 m, got {cell!r}")
        for name in ("x_range", "y_range", "z_range"):
            v = getattr(self, name)
            if not isinstance(v, (tuple, list)) or len(v) != 2:
                raise ValueError(f"{name} must be (min, max), got {v!r}")
            lo, hi = _number(name, v[0]), _number(name, v[1])
            if not (-LIMIT <= lo and hi <= LIMIT and np.float32(lo) < np.float32(hi)):
                raise ValueError(f"{name} must lie within +-{LIMIT:g} with min < max in float32, got {v!r}")
            object.__setattr__(self, name, (lo, hi))
        for name, side in (("x_range", self.W), ("y_range", self.H)):
            if not 1 <= side <= MAX_SIDE:
                raise ValueError(f"{name} gives {side} cells of {cell!r} m, want 1..{MAX_SIDE}")
        if self.W * self.H > MAX_CELLS:
            raise ValueError(f"x_range and y_range give {self.W} x {self.H} cells, want at most {MAX_CELLS}")
        _count("min_cell_points", self.min_cell_points, 1, 2 ** 31 - 1)
        lo = _count("min_points", self.min_points, 1, 2 ** 31 - 1)
        _count("max_points", self.max_points, lo, 2 ** 31 - 1)
        _count("max_clusters", self.max_clusters, 1, MAX_CLUSTERS)
        if not isinstance(self.remove_ground, (bool, np.bool_)):
            raise ValueError(f"remove_ground must be a bool, got {self.remove_ground!r}")

    def _side(self, r) -> int:
        return math.ceil((float(r[1]) - float(r[0])) / float(self.cell) - 1e-9)

    @property
    def W(self) -> int:
        return self._side(self.x_range)

    @property
    def H(self) -> int:
        return self._side(self.y_range)

    @property
    def c32(self) -> np.float32:
        return np.float32(self.cell)


# ------------------------------------------------------------------------- definition
def cells_numpy(points, opts: ClusterOptions):
    """The per-point half of the definition → ``(cell [N] int32, -1 where the point is not valid,
    q [N, 3] int32: xi, yi, zi, 0 where it is not)``."""
    x, y, z = _xyz(points)
    lim, W, H = np.float32(LIMIT), opts.W, opts.H
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (np.abs(x) <= lim) & (np.abs(y) <= lim) & (np.abs(z) <= lim)
        valid &= (z >= np.float32(opts.z_range[0])) & (z <= np.float32(opts.z_range[1]))
        dx = ((x - np.float32(opts.x_range[0])).astype(np.float32) / opts.c32).astype(np.float32)
        dy = ((y - np.float32(opts.y_range[0])).astype(np.float32) / opts.c32).astype(np.float32)
        valid &= (dx >= 0) & (dx < np.float32(W)) & (dy >= 0) & (dy < np.float32(H))
    ix = np.where(valid, dx, np.float32(0)).astype(np.int32)  # truncation
    iy = np.where(valid, dy, np.float32(0)).astype(np.int32)
    q = np.stack([np.rint(np.where(valid, v, np.float32(0)) * np.float32(Q)).astype(np.int32) for v in (x, y, z)], 1)
    return np.where(valid, iy * W + ix, -1).astype(np.int32), q


def components_numpy(occupied: np.ndarray, W: int, H: int) -> np.ndarray:
    """``occupied``: ascending cell indices → per occupied cell the smallest cell index of its
    8-connected component: min-propagation over the eight shifts with pointer jumping, on the
    occupied cells alone."""
    K = len(occupied)
    pos = np.full(W * H + 1, K, np.int64)  # cell → its place among the occupied ones, K: none
    pos[occupied] = np.arange(K)
    ix, iy = occupied % W, occupied // W
    nbrs = []
    for sy in (-1, 0, 1):
        for sx in (-1, 0, 1):
            if sx or sy:
                ok = (ix + sx >= 0) & (ix + sx < W) & (iy + sy >= 0) & (iy + sy < H)
                nbrs.append(np.append(pos[np.where(ok, occupied + sy * W + sx, W * H)], K))
    lab = np.arange(K + 1)  # places ascend with the cell indices; lab[K] = K is larger than any
    while True:
        new = lab
        for nb in nbrs:
            new = np.minimum(new, lab[nb])
        new = new[new]
        if (new == lab).all():
            return occupied[lab[:K]]
        lab = new


def _outputs(cell, q, cnt_cells, cnt, roots, opts: ClusterOptions):
    """The integer half after the components: ``cnt_cells`` the cells with points (ascending), ``cnt``
    their counts, ``roots`` per such cell its component's root (-1: not occupied)."""
    occ = roots >= 0
    uniq, inv = np.unique(roots[occ], return_inverse=True)
    size = np.zeros(len(uniq), np.int64)
    np.add.at(size, inv, cnt[occ])
    kept = (size >= opts.min_points) & (size <= opts.max_points)
    found = int(kept.sum())
    k_of = np.where(kept, np.cumsum(kept) - 1, -1)
    k_of[k_of >= opts.max_clusters] = -1
    k_cell = np.full(len(cnt_cells), -1, np.int64)
    k_cell[occ] = k_of[inv]
    at = np.searchsorted(cnt_cells, np.where(cell >= 0, cell, 0))
    label = np.where(cell >= 0, k_cell[np.minimum(at, max(len(cnt_cells) - 1, 0))] if len(cnt_cells) else -1, -1)
    label = label.astype(np.int32)
    rows = min(found, opts.max_clusters)
    table = np.zeros(rows, TABLE_DTYPE)
    table["root"] = uniq[kept][:rows]
    for j, a in enumerate("xyz"):
        table["min_" + a], table["max_" + a] = 2 ** 31 - 1, -2 ** 31
    m = label >= 0
    k, qm = label[m], q[m].astype(np.int64)
    np.add.at(table["n"], k, 1)
    for j, a in enumerate("xyz"):
        np.minimum.at(table["min_" + a], k, q[m][:, j])
        np.maximum.at(table["max_" + a], k, q[m][:, j])
        np.add.at(table["sum_" + a], k, qm[:, j])
    return found, label, table


def cluster_numpy(points, opts: ClusterOptions):
    """The definition → ``(found, label [N] int32, table [min(found, max_clusters)] of
    TABLE_DTYPE)``.  ``points`` [N, >=3] (x, y, z): the points to cluster, the ground already
    taken out."""
    cell, q = cells_numpy(points, opts)
    cnt_cells, cnt = np.unique(cell[cell >= 0], return_counts=True)
    occ = cnt >= opts.min_cell_points
    roots = np.full(len(cnt_cells), -1, np.int64)
    roots[occ] = components_numpy(cnt_cells[occ].astype(np.int64), opts.W, opts.H)
    return _outputs(cell, q, cnt_cells, cnt, roots, opts)


def cluster_ref(points, opts: ClusterOptions):
    """Float64 brute force → ``(found, label, table, band [N] bool)``: the cell is
    ``floor((x - x_min) / cell)`` in float64, the components come from a flood fill in plain Python
    over the dictionary of occupied cells, the rest as in the definition (``v * 1024`` and the
    comparisons with 512 and ``z_range`` are exact on both sides).

    ``band`` marks the points whose float32 cell may legitimately differ: ``dx`` or ``dy`` within
    ``3 * 2**-24 * d`` of an integer from 1 up, ``W`` and ``H`` among them (the difference and the
    quotient are each rounded once; ``docs/precision.md`` has the derivation).  At 0 both agree:
    the sign of a float32 difference is exact.  ``float32(cell)`` and ``float32(x_min)`` are inputs
    of both evaluations.  A banded point may change a cell's occupancy, so the two are compared on
    clouds without banded points."""
    x, y, z = (c.astype(np.float64) for c in _xyz(points))
    W, H, c = opts.W, opts.H, float(opts.c32)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (np.abs(x) <= LIMIT) & (np.abs(y) <= LIMIT) & (np.abs(z) <= LIMIT)
        valid &= (z >= float(np.float32(opts.z_range[0]))) & (z <= float(np.float32(opts.z_range[1])))
        dx = (x - float(np.float32(opts.x_range[0]))) / c
        dy = (y - float(np.float32(opts.y_range[0]))) / c
        band = np.zeros(len(x), bool)
        for d in (dx, dy):
            near = np.rint(d)
            band |= valid & (near >= 1) & (np.abs(d - near) <= CELL_BAND * np.abs(d))
        valid &= (dx >= 0) & (dx < W) & (dy >= 0) & (dy < H)
    ix = np.floor(np.where(valid, dx, 0.0)).astype(np.int64)
    iy = np.floor(np.where(valid, dy, 0.0)).astype(np.int64)
    cell = np.where(valid, iy * W + ix, -1).astype(np.int32)
    q = np.stack([np.rint(np.where(valid, v, 0.0) * Q).astype(np.int32) for v in (x, y, z)], 1)
    cnt_cells, cnt = np.unique(cell[cell >= 0], return_counts=True)
    root_of = {int(cl): -1 for cl, n in zip(cnt_cells, cnt) if n >= opts.min_cell_points}
    for start in sorted(root_of):  # ascending: a component is first met at its smallest cell
        if root_of[start] >= 0:
            continue
        root_of[start], todo = start, [start]
        while todo:
            cl = todo.pop()
            cx, cy = cl % W, cl // W
            for nx in (cx - 1, cx, cx + 1):
                for ny in (cy - 1, cy, cy + 1):
                    nb = ny * W + nx
                    if 0 <= nx < W and 0 <= ny < H and root_of.get(nb, 0) < 0:
                        root_of[nb] = start
                        todo.append(nb)
    roots = np.array([root_of.get(int(cl), -1) for cl in cnt_cells], np.int64)
    return (*_outputs(cell, q, cnt_cells, cnt, roots, opts), band)


def obstacle_rows(points, ground: G.GroundOptions) -> np.ndarray:
    """The rows of ``points`` that ``ops/ground.py`` classifies as obstacles, in input order."""
    return np.asarray(points)[G.split_numpy(points, ground) == G.OBSTACLE]


def cluster_cloud_numpy(cloud, opts: ClusterOptions, ground: Optional[G.GroundOptions] = None,
                        lay: Optional[CloudLayout] = None):
    """One cloud through the definition: with ``remove_ground`` ``split_numpy`` (``ground``: its
    options, the defaults without) and ``cluster_numpy`` on the obstacle rows, whose records the
    labels are reported for."""
    pts = cloud_xyzi(cloud, lay)
    if opts.remove_ground:
        pts = obstacle_rows(pts, ground or G.GroundOptions())
    return cluster_numpy(pts, opts)


# ---------------------------------------------------------------------------- messages
def cluster_boxes(table: np.ndarray, header: msgs.Header, jsk: bool = True):
    """The table as a box message with ``header``, through the driver's column builders: one
    axis-aligned box per row, centre ``((min + max) / 2) / 1024`` and dimensions
    ``(max - min) / 1024`` in float64, identity orientation, ``value`` / ``score`` the point count as
    float32, ``label`` / ``id`` the cluster's number ``k``."""
    from ..inference.ros_inference3d import boxes_to_detection3d, boxes_to_jsk

    n = len(table)
    b = np.zeros((n, 7), np.float64)
    for j, a in enumerate("xyz"):
        lo, hi = table["min_" + a].astype(np.float64), table["max_" + a].astype(np.float64)
        b[:, j] = (lo + hi) / 2 / Q
        b[:, 3 + j] = (hi - lo) / Q
    if jsk:  # the jsk columns swap the first two dimensions back
        b[:, [3, 4]] = b[:, [4, 3]]
    pred = {"pred_boxes": b, "pred_scores": table["n"].astype(np.float32), "pred_labels": np.arange(n)}
    hdr = msgs.Header(seq=header.seq, stamp=header.stamp, frame_id=header.frame_id)
    return boxes_to_jsk(pred, np.arange(n), hdr) if jsk else boxes_to_detection3d(pred, np.arange(n), hdr)


# --------------------------------------------------------------------------------- GPU
@dataclass
class ClusterCall:
    """One prepared launch: device views of its inputs, workspace and outputs."""
    data: torch.Tensor  # the staged records, or K30's output slab
    data_bytes: int
    frame_off: torch.Tensor
    frame_n: torch.Tensor  # int32 [B], or K30's counts int32 [B][2]
    n_stride: int
    cnt: torch.Tensor
    lab: torch.Tensor
    pcell: torch.Tensor
    blocks: torch.Tensor
    out: torch.Tensor  # uint8: table [B][max_clusters] rows, found int32 [B], err int32, then label int32 per record
    layout: CloudLayout
    batch: int
    max_n: int
    ns: Tuple[int, ...]  # the staged clouds' points (with the ground taken out: an upper bound)
    frame_offs: Tuple[int, ...]
    opts: ClusterOptions
    ground: Optional[G.GroundCall] = None

    @property
    def table_bytes(self) -> int:
        return self.batch * self.opts.max_clusters * ROW

    @property
    def head_bytes(self) -> int:
        """The table, ``found`` and ``err``: all the box message needs."""
        return self.table_bytes + 4 * self.batch + 4

    @property
    def records(self) -> int:
        return self.data_bytes // self.layout.point_step + 1

    @property
    def out_bytes(self) -> int:
        return _align(self.head_bytes) + 4 * self.records

    def view(self, lo: int, count: int) -> torch.Tensor:
        return self.out[lo:lo + 4 * count].view(torch.int32)

    @property
    def found(self) -> torch.Tensor:
        return self.view(self.table_bytes, self.batch)

    @property
    def err(self) -> torch.Tensor:
        return self.view(self.table_bytes + 4 * self.batch, 1)

    @property
    def label(self) -> torch.Tensor:
        return self.view(_align(self.head_bytes), self.records)


def launch(c: ClusterCall, stream=None, aggregate: bool = True) -> None:
    """The launch alone (nine kernels on ``stream``, behind the ground split's six when the call has
    one): no allocation, no copy, no sync."""
    p = _native.ptr
    if c.ground is not None:
        G.launch(c.ground, G.WANT_OBSTACLES, stream)
    o, r = c.layout.offsets, c.opts
    _native.call("tca_cluster", p(c.data), c.data_bytes, p(c.frame_off), p(c.frame_n), c.n_stride, c.batch, c.max_n,
                 c.layout.point_step, o[0], o[1], o[2], float(np.float32(r.x_range[0])),
                 float(np.float32(r.y_range[0])), float(r.c32), r.W, r.H, float(np.float32(r.z_range[0])),
                 float(np.float32(r.z_range[1])), int(r.min_cell_points), int(r.min_points), int(r.max_points),
                 int(r.max_clusters), 1 if aggregate else 0, p(c.cnt), p(c.lab), p(c.pcell), p(c.blocks), p(c.label),
                 p(c.out), p(c.found), p(c.err), _native.stream_ptr(stream))


def results_of(host: np.ndarray, c: ClusterCall, ns: Sequence[int], labels: bool) -> List[tuple]:
    """Per cloud ``(found, label or None, table)`` of a launch's output (``host``: ``out_bytes`` bytes,
    or ``head_bytes`` without labels; ``ns``: the clustered records per cloud).  A non-zero ``err``
    raises: a union-find loop of the launch hit its bound."""
    B, mc = c.batch, c.opts.max_clusters
    found = host[c.table_bytes:c.table_bytes + 4 * B].view("<i4")
    if int(host[c.table_bytes + 4 * B:c.head_bytes].view("<i4")[0]) != 0:
        raise _native.NativeError("tca_cluster: a union-find loop did not end within its bound")
    table = host[:c.table_bytes].view(TABLE_DTYPE).reshape(B, mc)
    lab = host[_align(c.head_bytes):].view("<i4") if labels else None
    step, res = c.layout.point_step, []
    for b, (n, fo) in enumerate(zip(ns, c.frame_offs)):
        res.append((int(found[b]), lab[fo // step:fo // step + n].copy() if labels else None,
                    table[b, :min(int(found[b]), mc)].copy()))
    return res


class ClusterExtractor(CloudStager):
    """Clusters clouds: on a GPU with ``tca_cluster`` (its own workspace, stream and pinned staging;
    with ``remove_ground`` a :class:`~triton_client_amd.ops.ground.GroundSplitter` of its own on the
    same workspace stages the clouds, its launch runs first and ``tca_cluster`` reads the obstacle
    slab and the counts where they lie: no byte goes to the host in between), on the CPU — and with
    ``TCA_DEVICE_CLUSTER=0`` — with the definition.  Clouds the kernel does not take (non-FLOAT32 or
    big-endian fields) run the definition with one warning.  ``aggregate`` False: the launch's
    one-atomic-set-per-point variant (measurements)."""

    aggregate = True
    fit_split = True  # False: ``tca_cluster_fit`` gives every cluster one workgroup (measurements)

    def __init__(self, device="auto", ws=None):
        super().__init__(device, ws)
        self.splitter = G.GroundSplitter(self.device, self.ws) if self.gpu else None

    def prepare(self, payloads: Sequence, ns: Sequence[int], layout: CloudLayout, opts: ClusterOptions,
                ground: Optional[G.GroundOptions] = None, stream=None, misalign: int = 0) -> ClusterCall:
        """Stage one batch in pinned memory and upload it with one H2D copy on ``stream``; with
        ``remove_ground`` through the ground splitter's ``prepare`` (``ground``: its options, the
        defaults without)."""
        if not G.layout_device_ok(layout):
            raise ValueError(f"tca_cluster does not take this layout: {layout}")
        B, ns = len(payloads), [int(n) for n in ns]
        if not 1 <= B <= MAX_FRAMES:
            raise ValueError(f"{B} clouds do not fit one call (1..{MAX_FRAMES}): split the batch")
        data_bytes = plan_staging(ns, layout.point_step, misalign, ()).data_bytes  # (refused before any allocation)
        if data_bytes >= INT31:
            raise ValueError(f"{data_bytes} payload bytes do not fit one call: split the batch")
        cells = opts.W * opts.H
        if B * cells > MAX_PLANE:
            raise ValueError(f"{B} clouds of {opts.W} x {opts.H} cells do not fit one call ({MAX_PLANE}): split the "
                             "batch")
        g = None
        if opts.remove_ground:
            g = self.splitter.prepare(payloads, ns, layout, ground or G.GroundOptions(), stream, misalign)
            data, frame_off, frame_n, frame_offs = g.out, g.frame_off, g.counts, g.frame_offs
        else:
            data, plan, view = self._stage("cluster_in", payloads, ns, layout.point_step, misalign, [], stream)
            frame_off, frame_n = view("frame_off", B, torch.int64), view("frame_n", B, torch.int32)
            frame_offs = plan.frame_offs
        c = ClusterCall(data=data, data_bytes=data_bytes, frame_off=frame_off, frame_n=frame_n,
                        n_stride=2 if g is not None else 1, cnt=self._device_buf("cluster_cnt", 4 * B * cells),
                        lab=self._device_buf("cluster_lab", 4 * B * cells), pcell=None, blocks=None, out=None,
                        layout=layout, batch=B, max_n=max(ns, default=0), ns=tuple(ns), frame_offs=frame_offs,
                        opts=opts, ground=g)
        c.pcell = self._device_buf("cluster_pcell", 4 * c.records)
        c.blocks = self._device_buf("cluster_blocks", 4 * B * ((cells + 255) // 256 + 1))
        c.out = self._device_buf("cluster_out", c.out_bytes)
        return c

    launch = staticmethod(launch)

    def _run_device(self, payloads, ns, layout, opts, ground, labels, fit=None):
        from . import cluster_fit as F

        with torch.cuda.device(self.device):
            st = self._own_stream()
            c = self.prepare(payloads, ns, layout, opts, ground, st)
            launch(c, st, self.aggregate)
            f = None
            if fit is not None:  # behind tca_cluster on the same stream: the labels stay on the device
                f = F.prepare(self, c, fit)
                F.launch(f, st, self.fit_split)
            if not labels and f is None:
                return results_of(self._fetch(c.out, c.head_bytes, st), c, ns, False)
            nbytes = c.out_bytes if labels else c.head_bytes
            at_fit = _align(nbytes + 8 * c.batch)
            pin = self._pinned("_pin_out", at_fit + (f.fit_bytes if f is not None else 0))
            with torch.cuda.stream(st):  # one fetch: the copies, then one synchronize
                pin[:nbytes].copy_(c.out[:nbytes], non_blocking=True)
                if labels and c.ground is not None:  # how many records of each slot are obstacles
                    pin[nbytes:nbytes + 8 * c.batch].copy_(c.ground.out[c.ground.slab_bytes:c.ground.out_bytes],
                                                            non_blocking=True)
                if f is not None:
                    pin[at_fit:at_fit + f.fit_bytes].copy_(f.fit[:f.fit_bytes], non_blocking=True)
            st.synchronize()
            host = pin.numpy()
            if labels and c.ground is not None:
                ns = host[nbytes:nbytes + 8 * c.batch].view("<i4")[::2].tolist()
            res = results_of(host[:nbytes], c, ns, labels)
            if f is None:
                return res
            fits = F.results_of(host[at_fit:at_fit + f.fit_bytes], f, [r[0] for r in res])
            return [(*r, t) for r, t in zip(res, fits)]

    def _parts_for(self, opts: ClusterOptions, ground: Optional[G.GroundOptions]):
        """The cut of a layout's clouds into launches: at most 64 clouds, less than 2^31 staged
        bytes, at most 2^24 cells and, with the ground taken out, the ground plane's own limit."""
        most = max(1, min(MAX_FRAMES, MAX_PLANE // (opts.W * opts.H)))
        if opts.remove_ground:
            most = min(most, G.most_clouds(ground or G.GroundOptions()))
        return G.parts_of(most)

    # ---------------------------------------------------------------------- API
    def extract(self, clouds: Sequence, opts: ClusterOptions, ground: Optional[G.GroundOptions] = None,
                labels: bool = True, fit=None) -> List[tuple]:
        """Per cloud ``(found, label, table)``, in input order; ``labels`` False: ``label`` is None
        and is not copied back.  ``fit`` (a :class:`~triton_client_amd.ops.cluster_fit.FitOptions`):
        the oriented fit of every table row as a fourth element (K32: ``tca_cluster_fit`` behind
        ``tca_cluster``; where that one's definition runs, and with ``TCA_DEVICE_CLUSTER_FIT=0``, the cloud
        takes both definitions on the host: the fit's reads the points and labels there)."""
        from . import cluster_fit as F

        def on_host(i, lay):
            if fit is None:
                found, label, table = cluster_cloud_numpy(clouds[i], opts, ground, lay)
                return found, label if labels else None, table
            pts = cloud_xyzi(clouds[i], lay)  # the fit's definition reads the points the labels are for
            if opts.remove_ground:
                pts = obstacle_rows(pts, ground or G.GroundOptions())
            found, label, table = cluster_numpy(pts, opts)
            return found, label if labels else None, table, F.fit_numpy(pts, label, table, fit)

        return self._per_cloud(
            clouds, lambda i, lay: G.layout_device_ok(lay), on_host,
            lambda lay, part: (*cloud_bytes(clouds, part), lay, opts, ground, labels, fit), self._run_device,
            lambda i, lay: f"ClusterExtractor: tca_cluster takes little-endian FLOAT32 x, y, z (got {lay}); such "
                           "clouds are clustered on the host",
            device=self.gpu and device_enabled() and (fit is None or F.device_enabled()),
            parts=self._parts_for(opts, ground))

    def messages(self, clouds: Sequence, opts: ClusterOptions, ground: Optional[G.GroundOptions] = None,
                 jsk: bool = True, fit=None) -> list:
        """Per cloud its box message, with the cloud's header; with ``fit`` the boxes are the oriented
        ones of ``ops/cluster_fit.py``."""
        res = self.extract(clouds, opts, ground, labels=False, fit=fit)
        if fit is None:
            return [cluster_boxes(table, c.header, jsk) for c, (_, _, table) in zip(clouds, res)]
        from .cluster_fit import fit_boxes

        return [fit_boxes(r[2], r[3], c.header, jsk, fit) for c, r in zip(clouds, res)]
