"""K33 — the cloud as a ray-cast ``nav_msgs/OccupancyGrid``: occupied, free and unknown cells.

What a planner or a static costmap layer reads is a grid with **free space**; ROS users get it from
``costmap_2d``'s obstacle layer or Autoware's ``pointcloud_based_occupancy_grid_map``, in one more
subscriber on a CPU core.  Here the driver publishes it per cloud, from the ground / obstacle split
of ``ops/ground.py`` (K30): obstacle returns mark cells occupied, every return, ground or obstacle,
proves its ray free up to the first obstacle in its direction, everything else is unknown.
:func:`grid_numpy` is the definition, bit for bit (the pattern of ``ops/cluster.py``); the HIP
kernel ``tca_occupancy_grid`` (``csrc/kernels/occupancy_grid.hip``) computes the same bytes straight
behind ``tca_ground_split`` on the device, from its output slab and counts where they lie, and
:func:`grid_ref` is a float64 brute force with true ``atan2`` and ``floor`` that also marks the
cells float32 may legitimately decide differently (``docs/precision.md``).

**The grid** is ``W x H`` cells of ``cell`` metres (``ops/cluster.py``'s rule for the sides), cell
index ``iy * W + ix``, the order of ``OccupancyGrid.data``.  Directions are the ``sectors`` angular
sectors of ``ops/ground.py``'s full-circle edge table.  All arithmetic is float32, every operation
rounded on its own (no FMA), IEEE division and square root; a NaN compares false.

**Per point.**  Its cell by ``cluster.cells_numpy`` with ``z_range = +-512``; ``ocnt[cell]`` counts
the valid obstacle points, ``gseen[cell]`` is set by a valid ground point.  Every record with a
sector (``laser_scan.pseudo_bins``), inside the grid or not, and a finite ``r = sqrt(x*x + y*y)``
has the key ``r``'s bits (positive floats order as their bits): ``near[s]`` is the smallest key of
the sector's obstacle records (``0xFFFFFFFF`` without any), ``far[s]`` the largest of its obstacle
and ground records (0 without any).

**Per cell** ``(ix, iy)`` the centre is ``cx = f32(x_min) + (f32(ix) + 0.5f) * f32(cell)`` (the sum
is exact, then one rounded multiply and one rounded add), ``cy`` likewise,
``r_c = sqrt(cx*cx + cy*cy)`` and ``s_c`` the centre's sector (a centre on the sensor has none).
The value is the first that applies: **100** iff ``ocnt >= min_points``; **0** iff ``gseen`` (a cell
that holds a ground return is free whatever stands in front of it), or
``r_c < f32(clear_radius)``, or the centre has a sector and
``key(r_c) < min(near[s_c], far[s_c])``; **-1** otherwise — the shadow behind the first obstacle
and every direction without a return.  Nothing depends on the order of the points.

**Inflation** (K37, ``inflation_radius > 0``; off by default) is ``costmap_2d``'s inflation layer on
that plane, so that a planner can take the topic as it is.  ``Rc = ceil(inflation_radius / cell)``
cells (``cellDistance``, 1..64); :func:`cost_table` holds, per squared distance ``d2`` in cells, the
byte ROS publishes for ``InflationLayer::computeCost`` (100 on the obstacle, 99 within
``inscribed_radius``, then ``252 * exp(-cost_scaling * (dist - inscribed_radius))`` through
``Costmap2DPublisher``'s translation to 1..98, 0 beyond).  It is made on the host in float64 and is an
input of the definition and of the device alike.  :func:`inflate_numpy` is the definition: per cell
``d2`` is the smallest ``dx*dx + dy*dy`` to a cell of value 100 of the same plane (outside the plane
nothing is occupied), ``c = table[d2]`` for ``d2 <= Rc*Rc`` and 0 beyond; 100 stays, 0 becomes ``c``,
-1 becomes ``c`` where ``c >= 99`` (with ``inflate_unknown``: where ``c > 0``) and stays -1
otherwise — the layer's ``NO_INFORMATION`` rule.  Integers only: the kernel ``tca_grid_inflate``
(``csrc/kernels/grid_inflate.hip``) and the brute force :func:`inflate_ref` give equal bytes.

Not here: tf and ``target_frame``, accumulation over time (log-odds), footprints other than a circle,
``inflate_around_unknown``, inflation in the ring engines, and ``map_server`` files.
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
from . import ground as G
from .cloud_common import CloudLayout, CloudStager, _align, cloud_bytes, cloud_xyzi
from .laser_scan import _number, pseudo64, pseudo_bins
from .range2d import U, _xyz

MAX_FRAMES = 64  # clouds per launch
MAX_SECTORS = 4096
MAX_PLANE = 2 ** 24  # cells of one launch
MAX_INFLATION_CELLS = 64  # K37: the halo of a tile
OCCUPIED, FREE, UNKNOWN = 100, 0, -1
NO_KEY = 0xFFFFFFFF  # near[] of a sector without an obstacle record
GROUND_BIT = 0x80000000  # of a cell word; the obstacle count is below it
R_BAND = 3 * U  # grid_ref: how near r_c may lie to near / far / clear_radius, relative


def device_enabled() -> bool:
    """``TCA_DEVICE_GRID=0`` keeps the definition on GPU engines too (``TCA_DEVICE_GROUND=0`` as well)."""
    return os.environ.get("TCA_DEVICE_GRID", "1") != "0" and G.device_enabled()


# ----------------------------------------------------------------------------- options
@dataclass(frozen=True)
class GridOptions:
    cell: float = 0.2
    x_range: Tuple[float, float] = (-40.0, 40.0)
    y_range: Tuple[float, float] = (-40.0, 40.0)
    sectors: int = 720
    min_points: int = 1
    clear_radius: float = 0.0
    inflation_radius: float = 0.0  # metres; 0: off (costmap_2d's inflation_radius)
    inscribed_radius: float = 0.0  # metres: cells this near to an obstacle cost 99
    cost_scaling: float = 10.0  # costmap_2d's cost_scaling_factor
    inflate_unknown: bool = False

    z_range = (-C.LIMIT, C.LIMIT)  # (not a field) what ``cluster.cells_numpy`` reads

    def __post_init__(self):
        cell = _number("cell", self.cell)
        if not 0.05 <= cell <= 10.0:
            raise ValueError(f"cell must be within 0.05..10 m, got {cell!r}")
        for name in ("x_range", "y_range"):
            v = getattr(self, name)
            if not isinstance(v, (tuple, list)) or len(v) != 2:
                raise ValueError(f"{name} must be (min, max), got {v!r}")
            lo, hi = _number(name, v[0]), _number(name, v[1])
            if not (-C.LIMIT <= lo and hi <= C.LIMIT and np.float32(lo) < np.float32(hi)):
                raise ValueError(f"{name} must lie within +-{C.LIMIT:g} with min < max in float32, got {v!r}")
            object.__setattr__(self, name, (lo, hi))
        for name, side in (("x_range", self.W), ("y_range", self.H)):
            if not 1 <= side <= C.MAX_SIDE:
                raise ValueError(f"{name} gives {side} cells of {cell!r} m, want 1..{C.MAX_SIDE}")
        if self.W * self.H > C.MAX_CELLS:
            raise ValueError(f"x_range and y_range give {self.W} x {self.H} cells, want at most {C.MAX_CELLS}")
        C._count("sectors", self.sectors, 1, MAX_SECTORS)
        C._count("min_points", self.min_points, 1, 2 ** 31 - 1)
        if not _number("clear_radius", self.clear_radius) >= 0:
            raise ValueError(f"clear_radius must be >= 0, got {self.clear_radius!r}")
        radius = _number("inflation_radius", self.inflation_radius)
        inscribed = _number("inscribed_radius", self.inscribed_radius)
        scaling = _number("cost_scaling", self.cost_scaling)
        if not isinstance(self.inflate_unknown, (bool, np.bool_)):
            raise ValueError(f"inflate_unknown must be a bool, got {self.inflate_unknown!r}")
        if not radius >= 0:
            raise ValueError(f"inflation_radius must be >= 0, got {radius!r}")
        if not 0 <= scaling <= 100:
            raise ValueError(f"cost_scaling must be within 0..100, got {scaling!r}")
        if radius == 0:
            for name, off in (("inscribed_radius", 0.0), ("cost_scaling", 10.0), ("inflate_unknown", False)):
                if getattr(self, name) != off:
                    raise ValueError(f"{name} needs inflation_radius")
        elif not 1 <= self.inflation_cells <= MAX_INFLATION_CELLS:
            raise ValueError(f"inflation_radius gives {self.inflation_cells} cells of {cell!r} m, want "
                             f"1..{MAX_INFLATION_CELLS}")
        if not 0 <= inscribed <= radius:
            raise ValueError(f"inscribed_radius must be within 0..inflation_radius, got {inscribed!r}")

    _side = C.ClusterOptions._side

    @property
    def W(self) -> int:
        return self._side(self.x_range)

    @property
    def H(self) -> int:
        return self._side(self.y_range)

    @property
    def c32(self) -> np.float32:
        return np.float32(self.cell)

    @property
    def inflation(self) -> bool:
        return self.inflation_radius > 0

    @property
    def inflation_cells(self) -> int:
        """``Rc``: ``costmap_2d``'s ``cellDistance`` of the radius."""
        return int(math.ceil(float(np.float32(self.inflation_radius)) / float(self.c32)))

    @property
    def stride(self) -> int:
        """Bytes from one cloud's plane to the next in the device's output: 16-byte aligned."""
        return _align(self.W * self.H)


# ------------------------------------------------------------------------- definition
def _keys(points, table):
    """→ ``(sector [N] int64, has [N] bool, key [N] uint32)``: ``has`` iff the record has a sector
    and a finite ``r``."""
    x, y, _ = _xyz(points)
    sec, has = pseudo_bins(x, y, table)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.sqrt(x * x + y * y).astype(np.float32)
    return sec, has & np.isfinite(r), r.view(np.uint32)


def centres_numpy(opts: GridOptions):
    """The cells' centres → ``(cx [H * W], cy [H * W])`` float32, in cell order."""
    half = np.float32(0.5)
    cx = np.float32(opts.x_range[0]) + (np.arange(opts.W, dtype=np.float32) + half) * opts.c32
    cy = np.float32(opts.y_range[0]) + (np.arange(opts.H, dtype=np.float32) + half) * opts.c32
    return np.tile(cx, opts.H).astype(np.float32), np.repeat(cy, opts.W).astype(np.float32)


def grid_numpy(obstacles, ground, opts: GridOptions) -> np.ndarray:
    """The definition → ``int8 [H * W]``.  ``obstacles``, ``ground``: [N, >=3] float32 rows
    (x, y, z) as K30 classified them."""
    S, cells = int(opts.sectors), opts.W * opts.H
    table = G.edge_table(opts)
    ocell, _ = C.cells_numpy(obstacles, opts)
    gcell, _ = C.cells_numpy(ground, opts)
    ocnt = np.bincount(ocell[ocell >= 0], minlength=cells)
    gseen = np.zeros(cells, bool)
    gseen[gcell[gcell >= 0]] = True
    near, far = np.full(S, NO_KEY, np.uint32), np.zeros(S, np.uint32)
    sec, has, key = _keys(obstacles, table)
    np.minimum.at(near, sec[has], key[has])
    np.maximum.at(far, sec[has], key[has])
    sec, has, key = _keys(ground, table)
    np.maximum.at(far, sec[has], key[has])

    cx, cy = centres_numpy(opts)
    s_c, has_c = pseudo_bins(cx, cy, table)
    r_c = np.sqrt(cx * cx + cy * cy).astype(np.float32)
    limit = np.minimum(near, far)[np.where(has_c, s_c, 0)]
    free = gseen | (r_c < np.float32(opts.clear_radius)) | (has_c & (r_c.view(np.uint32) < limit))
    return np.where(ocnt >= opts.min_points, OCCUPIED, np.where(free, FREE, UNKNOWN)).astype(np.int8)


def split_rows(points, ground_opts: Optional[G.GroundOptions] = None):
    """``points`` [N, >=3] → ``(obstacle rows, ground rows)`` by ``ops/ground.py``'s definition."""
    pts = np.asarray(points)
    cls = G.split_numpy(pts, ground_opts or G.GroundOptions())
    return pts[cls == G.OBSTACLE], pts[cls == G.GROUND]


def grid_cloud_numpy(cloud, opts: GridOptions, ground_opts: Optional[G.GroundOptions] = None,
                     lay: Optional[CloudLayout] = None) -> np.ndarray:
    """One cloud through the definitions: ``split_numpy`` (``ground_opts``: its options, the
    defaults without), then :func:`grid_numpy` on the two row sets."""
    plane = grid_numpy(*split_rows(cloud_xyzi(cloud, lay), ground_opts), opts)
    return inflate_numpy(plane, opts) if opts.inflation else plane


def grid_ref(obstacles, ground, opts: GridOptions):
    """Float64 brute force → ``(grid int8 [H * W], band bool [H * W])``: cells by
    ``floor((x - x_min) / cell)``, sectors by ``floor((atan2(y, x) + pi) / (2 pi / S))``, ``r`` and
    every comparison in float64.  ``float32(cell)``, ``float32(x_min)``, ``float32(clear_radius)``
    and the float32 centres are inputs of both evaluations.

    ``band`` marks the cells float32 may legitimately decide differently
    (``docs/precision.md``): a cell within one cell of where a point banded by ``cluster_ref``'s
    rule (``CELL_BAND``) falls; a centre whose pseudo-angle lies within ``EDGE_BAND`` of an edge
    of its sector; ``r_c`` within ``3 * 2**-24`` relative of ``clear_radius`` or of
    ``min(near, far)`` of its sector — of the whole interval that value can take when a point that
    is itself within ``EDGE_BAND`` of a sector edge is counted in the sector across that edge, in
    both or in neither."""
    S, W, H = int(opts.sectors), opts.W, opts.H
    c, x0, y0 = float(opts.c32), float(np.float32(opts.x_range[0])), float(np.float32(opts.y_range[0]))
    t64 = pseudo64(np.cos(G.edge_angles(opts)), np.sin(G.edge_angles(opts)))
    band = np.zeros((H, W), bool)

    def cells_of(points):  # the points' cells, -1: none; bands their surroundings
        x, y, z = (v.astype(np.float64) for v in _xyz(points))
        with np.errstate(invalid="ignore", over="ignore"):
            valid = (np.abs(x) <= C.LIMIT) & (np.abs(y) <= C.LIMIT) & (np.abs(z) <= C.LIMIT)
            dx, dy = np.where(valid, (x - x0) / c, -9.0), np.where(valid, (y - y0) / c, -9.0)
            odd = np.zeros(len(x), bool)
            for d in (dx, dy):
                odd |= valid & (np.rint(d) >= 1) & (np.abs(d - np.rint(d)) <= C.CELL_BAND * np.abs(d))
        fx, fy = np.floor(dx).astype(np.int64), np.floor(dy).astype(np.int64)
        for px, py in zip(fx[odd], fy[odd]):
            band[max(py - 1, 0):max(py + 2, 0), max(px - 1, 0):max(px + 2, 0)] = True
        inside = valid & (dx >= 0) & (dx < W) & (dy >= 0) & (dy < H)
        return np.where(inside, fy * W + fx, -1)

    def sectors_of(x, y):  # → (has, sector, the sector across a banded edge or -1, pseudo-angle banded)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            s = np.abs(x) + np.abs(y)
            ok = np.isfinite(s) & (s != 0)
            a = np.where(ok, np.arctan2(y, x), 0.0)
            sec = np.clip(np.floor((a + math.pi) / (2 * math.pi / S)), 0, S - 1).astype(np.int64)
            q = np.where(ok, pseudo64(x, np.where(ok, y, 1.0)), np.nan)
            lo, hi = np.abs(q - t64[sec]) <= G.EDGE_BAND, np.abs(q - t64[sec + 1]) <= G.EDGE_BAND
        other = np.where(lo & (sec > 0), sec - 1, np.where(hi & (sec < S - 1), sec + 1, -1))
        return ok, sec, other, ok & (lo | hi)

    # min(near, far) per sector is monotone in both.  Row 0: the smallest it can be (a banded point lowers near in
    # both sectors it may fall into and raises far in neither), row 1: the largest, row 2: every point in its own.
    near, far = np.full((3, S), np.inf), np.zeros((3, S))

    def keys_of(points, obstacle):
        x, y, _ = (v.astype(np.float64) for v in _xyz(points))
        ok, sec, other, odd = sectors_of(x, y)
        with np.errstate(invalid="ignore", over="ignore"):
            r = np.sqrt(x * x + y * y)
        ok &= np.isfinite(r)
        sure, across = ok & ~odd, ok & odd & (other >= 0)
        wide = (np.concatenate([sec[ok], other[across]]), np.concatenate([r[ok], r[across]]))
        own, narrow = (sec[ok], r[ok]), (sec[sure], r[sure])
        for row, n, f in ((0, wide, narrow), (1, narrow, wide), (2, own, own)):
            if obstacle:
                np.minimum.at(near[row], *n)
            np.maximum.at(far[row], *f)

    ocell, gcell = cells_of(obstacles), cells_of(ground)
    ocnt = np.bincount(ocell[ocell >= 0], minlength=W * H)
    gseen = np.zeros(W * H, bool)
    gseen[gcell[gcell >= 0]] = True
    keys_of(obstacles, True)
    keys_of(ground, False)

    cx, cy = (v.astype(np.float64) for v in centres_numpy(opts))
    has_c, s_c, _, odd_c = sectors_of(cx, cy)
    r_c = np.sqrt(cx * cx + cy * cy)
    clear = float(np.float32(opts.clear_radius))
    t_lo, t_hi, t = (np.minimum(near[k], far[k])[s_c] for k in (0, 1, 2))
    free = gseen | (r_c < clear) | (has_c & (r_c < t))
    flat = band.reshape(-1)
    flat |= odd_c | (np.abs(r_c - clear) <= R_BAND * r_c)
    flat |= has_c & (r_c >= t_lo * (1 - R_BAND)) & (r_c <= t_hi * (1 + R_BAND))
    return np.where(ocnt >= opts.min_points, OCCUPIED, np.where(free, FREE, UNKNOWN)).astype(np.int8), flat


# --------------------------------------------------------------------------- inflation
NO_ROW = 255  # the row distance of a cell with no occupied cell of its row within Rc: 255 * 255 > 64 * 64


def cost_table(opts: GridOptions) -> np.ndarray:
    """The published cost by squared distance in cells → ``int8 [Rc * Rc + 1]``, in float64 on the
    host: ``InflationLayer::computeCost`` (truncated as its ``unsigned char`` cast does), then
    ``Costmap2DPublisher``'s translation table (254 → 100, 253 → 99, 1..252 → 1..98)."""
    Rc, c = opts.inflation_cells, float(opts.c32)
    inscribed, scaling = float(np.float32(opts.inscribed_radius)), float(np.float32(opts.cost_scaling))
    lut = np.zeros(Rc * Rc + 1, np.int8)
    lut[0] = OCCUPIED
    for d2 in range(1, Rc * Rc + 1):
        dist = math.sqrt(float(d2)) * c
        if dist <= inscribed:
            lut[d2] = 99
            continue
        cost = int(252 * math.exp(-scaling * (dist - inscribed)))
        lut[d2] = 0 if cost == 0 else 1 + (97 * (cost - 1)) // 251
    return lut


def _inflated(p: np.ndarray, c: np.ndarray, opts: GridOptions) -> np.ndarray:
    """The value rule: ``p`` the plane's own values, ``c`` the cost of every cell."""
    take = (p == FREE) | ((p == UNKNOWN) & ((c > 0) if opts.inflate_unknown else (c >= 99)))
    return np.where(take, c, p).astype(np.int8)


def inflate_numpy(plane, opts: GridOptions) -> np.ndarray:
    """The definition of K37 → ``int8 [H * W]``: a separable two-pass integer minimum.  ``g`` is the
    distance along the row to the nearest occupied cell within ``Rc`` (``NO_ROW`` without one), then
    ``d2 = min over dy in -Rc..Rc of dy*dy + g*g`` of the row ``dy`` away; rows and columns outside
    the plane hold nothing."""
    W, H, Rc = opts.W, opts.H, opts.inflation_cells
    p = np.ascontiguousarray(plane, np.int8).reshape(H, W)
    occ = np.zeros((H, W + 2 * Rc), bool)
    occ[:, Rc:Rc + W] = p == OCCUPIED
    g = np.full((H + 2 * Rc, W), NO_ROW, np.int64)
    for dx in range(-Rc, Rc + 1):
        np.minimum(g[Rc:Rc + H], np.where(occ[:, Rc + dx:Rc + dx + W], abs(dx), NO_ROW), out=g[Rc:Rc + H])
    g2 = g * g
    d2 = g2[Rc:Rc + H].copy()
    for dy in range(1, Rc + 1):
        np.minimum(d2, dy * dy + np.minimum(g2[Rc - dy:Rc - dy + H], g2[Rc + dy:Rc + dy + H]), out=d2)
    c = np.where(d2 <= Rc * Rc, cost_table(opts)[np.minimum(d2, Rc * Rc)], 0)
    return _inflated(p, c, opts).reshape(-1)


def inflate_ref(plane, opts: GridOptions) -> np.ndarray:
    """A brute force with none of the definition's code: the offsets of the disc in ascending
    ``d2``, each ORing the shifted occupied mask into the plane of the ``d2`` a cell was first
    reached at; then the value rule, cell by cell.  Integers: equal to the definition, no band."""
    W, H, Rc = opts.W, opts.H, opts.inflation_cells
    lut = cost_table(opts)
    p = np.asarray(plane).reshape(H, W)
    first = np.full((H, W), -1, np.int64)
    disc = sorted((dx * dx + dy * dy, dx, dy) for dx in range(-Rc, Rc + 1) for dy in range(-Rc, Rc + 1)
                  if dx * dx + dy * dy <= Rc * Rc)
    for d2, dx, dy in disc:  # cell (y, x) is reached from an occupied (y + dy, x + dx)
        ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
        src = p[max(0, dy):min(H, H + dy), max(0, dx):min(W, W + dx)] == 100
        first[ys, xs] = np.where(src & (first[ys, xs] < 0), d2, first[ys, xs])
    out = np.empty((H, W), np.int8)
    for y in range(H):
        for x in range(W):
            v, c = int(p[y, x]), int(lut[first[y, x]]) if first[y, x] >= 0 else 0
            if v == 0 or (v == -1 and (c >= 99 or (opts.inflate_unknown and c >= 1))):
                v = c
            out[y, x] = v
    return out.reshape(-1)


# ---------------------------------------------------------------------------- messages
def grid_message(cloud, data: np.ndarray, opts: GridOptions, frame_id: str = "") -> msgs.OccupancyGrid:
    """The plane as a ``nav_msgs/OccupancyGrid`` with the cloud's stamp and seq, in frame
    ``frame_id`` (the cloud's when empty): ``map_load_time`` the stamp, the resolution and the
    origin the float32 values the cells were computed with, identity orientation."""
    h = cloud.header
    a = np.ascontiguousarray(data, np.int8).reshape(-1)
    if a.shape != (opts.W * opts.H,):
        raise ValueError(f"{a.shape[0]} cells, want {opts.W * opts.H}")
    origin = msgs.Pose(msgs.Point(float(np.float32(opts.x_range[0])), float(np.float32(opts.y_range[0])), 0.0),
                       msgs.Quaternion())
    info = msgs.MapMetaData(map_load_time=h.stamp, resolution=float(opts.c32), width=opts.W, height=opts.H,
                            origin=origin)
    return msgs.OccupancyGrid(header=msgs.Header(seq=h.seq, stamp=h.stamp, frame_id=frame_id or h.frame_id),
                              info=info, data=a)


# --------------------------------------------------------------------------------- GPU
@dataclass
class GridCall:
    """One prepared launch: the ground split's call and device views of the workspace and output."""
    ground: G.GroundCall
    table: torch.Tensor  # float32 [S + 1]
    cells: torch.Tensor  # uint8 view of B * stride cell words
    keys: torch.Tensor  # uint8 view of uint32 [B][2][S]: near, far
    out: torch.Tensor  # uint8: the planes, ``stride`` bytes apart
    batch: int
    opts: GridOptions
    inflated: Optional[torch.Tensor] = None  # uint8: K37's planes, laid out as ``out`` (with ``opts.inflation``)
    lut: Optional[torch.Tensor] = None  # uint8 view of int8 [Rc * Rc + 1]: the cost table

    @property
    def cells_bytes(self) -> int:
        return 4 * self.batch * self.opts.stride

    @property
    def keys_bytes(self) -> int:
        return 8 * self.batch * int(self.opts.sectors)

    @property
    def out_bytes(self) -> int:
        """The planes' extent: the last one is not padded."""
        return (self.batch - 1) * self.opts.stride + self.opts.W * self.opts.H


def launch(c: GridCall, stream=None, privatise: bool = True, aggregate: bool = True, stage_keys: bool = False,
           skip_empty: bool = True) -> None:
    """The launch alone (the ground split's six kernels, then the reset, the points pass and the
    cell pass on ``stream``, and with ``opts.inflation`` K37 behind them): no allocation, no copy,
    no sync.  ``privatise`` False: no LDS sector keys; ``aggregate`` False: one atomic per point;
    ``stage_keys``: the cell pass stages ``near`` and ``far`` in LDS; ``skip_empty`` False: K37 walks
    the tiles with no obstacle near them too (measurements)."""
    p = _native.ptr
    g, r = c.ground, c.opts
    G.launch(g, G.WANT_OBSTACLES | G.WANT_GROUND, stream)
    o = g.layout.offsets
    _native.call("tca_occupancy_grid", p(g.out), g.slab_bytes, p(g.frame_off), p(g.frame_n), p(g.counts), c.batch,
                 g.max_n, g.layout.point_step, o[0], o[1], o[2], p(c.table), int(r.sectors),
                 float(np.float32(r.x_range[0])), float(np.float32(r.y_range[0])), float(r.c32), r.W, r.H,
                 int(r.min_points), float(np.float32(r.clear_radius)), 1 if privatise else 0, 1 if aggregate else 0,
                 1 if stage_keys else 0, p(c.cells), c.cells_bytes, p(c.keys), c.keys_bytes, p(c.out), c.out_bytes,
                 _native.stream_ptr(stream))
    if r.inflation:
        inflate(c, stream, skip_empty)


def inflate(c: GridCall, stream=None, skip_empty: bool = True) -> None:
    """K37 alone: ``c.out``'s planes → ``c.inflated``."""
    p, r = _native.ptr, c.opts
    Rc = r.inflation_cells
    _native.call("tca_grid_inflate", p(c.out), c.out_bytes, c.batch, r.W, r.H, Rc, p(c.lut), Rc * Rc + 1,
                 1 if r.inflate_unknown else 0, 1 if skip_empty else 0, p(c.inflated), c.out_bytes,
                 _native.stream_ptr(stream))


def planes_of(host: np.ndarray, batch: int, opts: GridOptions) -> List[np.ndarray]:
    """The ``batch`` planes of a launch's output bytes, each its own ``int8 [H * W]``."""
    a = np.ascontiguousarray(host).view(np.int8)
    return [a[b * opts.stride:b * opts.stride + opts.W * opts.H].copy() for b in range(batch)]


def most_clouds(opts: GridOptions, ground_opts: G.GroundOptions) -> int:
    """How many clouds fit one launch: 64, 2^24 cells, and the ground plane's own limit."""
    return max(1, min(MAX_FRAMES, MAX_PLANE // opts.stride, G.most_clouds(ground_opts)))


class GridMapper(CloudStager):
    """Turns clouds into occupancy grids: on a GPU a :class:`~triton_client_amd.ops.ground.GroundSplitter`
    of its own on the same workspace stages the clouds, its launch runs first and
    ``tca_occupancy_grid`` reads the slab and the counts where they lie (no byte goes to the host
    in between; one D2H of ``H * W`` bytes per cloud; with ``opts.inflation`` ``tca_grid_inflate``
    runs behind it and its planes are the ones fetched); on the CPU — and with ``TCA_DEVICE_GRID=0``
    or ``TCA_DEVICE_GROUND=0`` — the definitions.  Clouds the kernels do not take (non-FLOAT32 or
    big-endian fields) run the definitions with one warning.  ``privatise``, ``aggregate``,
    ``stage_keys``: the launch's variants (measurements)."""

    privatise, aggregate, stage_keys = True, True, False

    def __init__(self, device="auto", ws=None):
        super().__init__(device, ws)
        self.splitter = G.GroundSplitter(self.device, self.ws) if self.gpu else None

    def prepare(self, payloads: Sequence, ns: Sequence[int], layout: CloudLayout, opts: GridOptions,
                ground: Optional[G.GroundOptions] = None, stream=None, misalign: int = 0) -> GridCall:
        """Stage one batch through the ground splitter's ``prepare`` (``ground``: its options, the
        defaults without) and upload the grid's own edge table behind it on ``stream``."""
        B, S = len(payloads), int(opts.sectors)
        if not 1 <= B <= MAX_FRAMES:
            raise ValueError(f"{B} clouds do not fit one call (1..{MAX_FRAMES}): split the batch")
        if B * opts.stride > MAX_PLANE:
            raise ValueError(f"{B} clouds of {opts.W} x {opts.H} cells do not fit one call ({MAX_PLANE}): split the "
                             "batch")
        g = self.splitter.prepare(payloads, ns, layout, ground or G.GroundOptions(), stream, misalign)
        costs = cost_table(opts).view(np.uint8) if opts.inflation else np.zeros(0, np.uint8)
        at = _align(4 * (S + 1))  # the cost table's place in the pinned bytes, behind the edges
        pin = self._pinned("_pin_in", at + len(costs) if opts.inflation else 4 * (S + 1))
        pin.numpy()[:4 * (S + 1)] = G.edge_table(opts).view(np.uint8)
        pin.numpy()[at:at + len(costs)] = costs
        table = self._device_buf("grid_table", 4 * (S + 1))
        lut = self._device_buf("grid_lut", len(costs)) if opts.inflation else None
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            table[:4 * (S + 1)].copy_(pin[:4 * (S + 1)], non_blocking=True)
            if lut is not None:
                lut[:len(costs)].copy_(pin[at:at + len(costs)], non_blocking=True)
        c = GridCall(ground=g, table=table, cells=None, keys=None, out=None, batch=B, opts=opts, lut=lut)
        c.cells = self._device_buf("grid_cells", c.cells_bytes)
        c.keys = self._device_buf("grid_keys", c.keys_bytes)
        c.out = self._device_buf("grid_out", c.out_bytes)
        if opts.inflation:
            c.inflated = self._device_buf("grid_inflated", c.out_bytes)
        return c

    launch = staticmethod(launch)

    def _run_device(self, payloads, ns, layout, opts, ground):
        """→ per frame its plane."""
        with torch.cuda.device(self.device):
            st = self._own_stream()
            c = self.prepare(payloads, ns, layout, opts, ground, st)
            launch(c, st, self.privatise, self.aggregate, self.stage_keys)
            return planes_of(self._fetch(c.inflated if opts.inflation else c.out, c.out_bytes, st), c.batch, opts)

    def _parts_for(self, opts: GridOptions, ground: Optional[G.GroundOptions]):
        """The cut of a layout's clouds into launches (:func:`most_clouds`, less than 2^31 staged bytes)."""
        return G.parts_of(most_clouds(opts, ground or G.GroundOptions()))

    # ---------------------------------------------------------------------- API
    def grids(self, clouds: Sequence, opts: GridOptions, ground: Optional[G.GroundOptions] = None) -> List[np.ndarray]:
        """Per cloud its plane ``int8 [H * W]``, in input order."""
        return self._per_cloud(
            clouds, lambda i, lay: G.layout_device_ok(lay),
            lambda i, lay: grid_cloud_numpy(clouds[i], opts, ground, lay),
            lambda lay, part: (*cloud_bytes(clouds, part), lay, opts, ground), self._run_device,
            lambda i, lay: f"GridMapper: tca_occupancy_grid takes little-endian FLOAT32 x, y, z (got {lay}); such "
                           "clouds are mapped on the host",
            device=self.gpu and device_enabled(), parts=self._parts_for(opts, ground))

    def messages(self, clouds: Sequence, opts: GridOptions, ground: Optional[G.GroundOptions] = None,
                 frame_id: str = "") -> List[msgs.OccupancyGrid]:
        """Per cloud its ``OccupancyGrid`` message."""
        return [grid_message(c, a, opts, frame_id) for c, a in zip(clouds, self.grids(clouds, opts, ground))]
