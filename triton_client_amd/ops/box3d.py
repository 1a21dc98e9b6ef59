"""K14r — ragged pairwise rotated IoU (BEV and 3D) for the LiDAR evaluator.

Boxes are ``(x, y, z, dx, dy, dz, yaw)`` with z the box centre.  All frames of
an evaluation run go through one call: frame ``f`` owns predictions
``pred_off[f]:pred_off[f + 1]`` and ground truth ``gt_off[f]:gt_off[f + 1]``,
and its ``[np_f, ng_f]`` row-major IoU block starts at ``pair_off[f]`` in both
outputs.  With class arrays, pairs of different classes are 0 in both outputs
and are not evaluated.

GPU: ``tca_box3d_iou`` (``csrc/kernels/nms.hip``), fp32, one launch.  CPU: the
same Green's-theorem edge clipping in float64 over all pairs at once
(:func:`overlap_pairs_np`); :func:`golden.rotated_iou_bev` /
:func:`golden.rotated_iou_3d` are the per-pair specification of both.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _native
from ._ws import Workspace

TILE = 64  # predictions per workgroup: kIouTile in nms.hip
INT32_MAX = 2 ** 31 - 1


def boxes7(b: np.ndarray) -> np.ndarray:
    """[n, >=7] detector boxes → [n, 7]: CenterPoint's 9 columns carry (vx, vy)
    before the yaw, the rule of ``ros_inference3d`` (yaw at 8 if dim >= 9 else 6)."""
    b = np.asarray(b)
    if b.ndim != 2:
        b = b.reshape(-1, 7)
    return b[:, [0, 1, 2, 3, 4, 5, 8 if b.shape[1] >= 9 else 6]]


def ragged_offsets(np_f, ng_f) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Per-frame counts → (pred_off, gt_off, pair_off), each [F + 1] int64."""
    np_f, ng_f = np.asarray(np_f, np.int64).reshape(-1), np.asarray(ng_f, np.int64).reshape(-1)
    z = np.zeros(1, np.int64)
    return (np.concatenate([z, np.cumsum(np_f)]), np.concatenate([z, np.cumsum(ng_f)]),
            np.concatenate([z, np.cumsum(np_f * ng_f)]))


def tile_table(pred_off: np.ndarray, gt_off: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(frame, first prediction within the frame) of every tile of 64 predictions;
    frames without predictions or without ground truth get no tile."""
    np_f, ng_f = np.diff(pred_off), np.diff(gt_off)
    tiles = np.where(ng_f > 0, (np_f + TILE - 1) // TILE, 0)
    frame = np.repeat(np.arange(len(np_f)), tiles)
    first = (np.arange(int(tiles.sum())) - np.repeat(np.cumsum(tiles) - tiles, tiles)) * TILE
    return frame.astype(np.int32), first.astype(np.int32)


# ------------------------------------------------------------------------------- CPU
def _cross(ax, ay, bx, by):
    return ax * by - ay * bx


def overlap_pairs_np(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """BEV intersection area of box A[k] with box B[k], float64 [K].

    By Green's theorem the CCW boundary of A∩B is the part of A's edges inside B
    plus the part of B's edges inside A, so 2·area = Σ cross(p0, p1) over the
    clipped edges.  In A's frame (A axis-aligned at the origin) B's edges are
    clipped to A's box (Liang–Barsky, open) and A's edges by B's four half-planes
    (Cyrus–Beck, closed), so coincident edges count once — the device function
    ``rotated_overlap`` of ``nms.hip``, vectorised over pairs."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    K = len(A)
    if K == 0:
        return np.zeros(0)
    ca, sa, cb, sb = np.cos(A[:, 6]), np.sin(A[:, 6]), np.cos(B[:, 6]), np.sin(B[:, 6])
    ddx, ddy = B[:, 0] - A[:, 0], B[:, 1] - A[:, 1]
    cr, sr = (cb * ca + sb * sa)[:, None], (sb * ca - cb * sa)[:, None]
    bx, by = (ca * ddx + sa * ddy)[:, None], (-sa * ddx + ca * ddy)[:, None]
    ahx, ahy = 0.5 * A[:, 3, None], 0.5 * A[:, 4, None]
    bhx, bhy = 0.5 * B[:, 3, None], 0.5 * B[:, 4, None]
    sx, sy = np.array([[-1.0, 1.0, 1.0, -1.0]]), np.array([[-1.0, -1.0, 1.0, 1.0]])
    qx = bx + cr * (bhx * sx) - sr * (bhy * sy)  # B's corners in A's frame, CCW  [K, 4]
    qy = by + sr * (bhx * sx) + cr * (bhy * sy)
    ex, ey = np.roll(qx, -1, 1) - qx, np.roll(qy, -1, 1) - qy  # B's edges
    inf = np.inf
    # B's edges clipped to A's box (open)
    pp = np.stack([-ex, ex, -ey, ey], -1)  # [K, edge, constraint]
    qq = np.stack([qx + ahx, ahx - qx, qy + ahy, ahy - qy], -1)
    par = pp == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = qq / np.where(par, 1.0, pp)
    empty = (par & (qq <= 0.0)).any(-1)
    t0 = np.maximum(0.0, np.where(~par & (pp < 0.0), r, -inf).max(-1))
    t1 = np.minimum(1.0, np.where(~par & (pp > 0.0), r, inf).min(-1))
    ok = ~empty & (t0 < t1)
    area2 = np.where(ok, _cross(qx + t0 * ex, qy + t0 * ey, qx + t1 * ex, qy + t1 * ey), 0.0).sum(1)
    # A's edges clipped by B's half-planes (closed)
    ax, ay = ahx * sx, ahy * sy  # A's corners  [K, 4]
    dx, dy = np.roll(ax, -1, 1) - ax, np.roll(ay, -1, 1) - ay
    px, py, qx2, qy2 = ax[:, :, None], ay[:, :, None], np.roll(ax, -1, 1)[:, :, None], np.roll(ay, -1, 1)[:, :, None]
    jx, jy, ejx, ejy = qx[:, None, :], qy[:, None, :], ex[:, None, :], ey[:, None, :]  # [K, edge of A, plane of B]
    sp = _cross(ejx, ejy, px - jx, py - jy)
    sq = _cross(ejx, ejy, qx2 - jx, qy2 - jy)
    out = (sp < 0.0) & (sq < 0.0)
    col = (sp == 0.0) & (sq == 0.0)  # collinear with B's edge: boundary of A∩B only if both run the same way
    empty = (out | (col & (ejx * (qx2 - px) + ejy * (qy2 - py) < 0.0))).any(-1)
    cut = ~out & ~col
    with np.errstate(divide="ignore", invalid="ignore"):
        t = sp / np.where(sp == sq, 1.0, sp - sq)
    t0 = np.maximum(0.0, np.where(cut & (sp < 0.0), t, -inf).max(-1))
    t1 = np.minimum(1.0, np.where(cut & (sp >= 0.0) & (sq < 0.0), t, inf).min(-1))
    ok = ~empty & (t0 < t1)
    area2 += np.where(ok, _cross(ax + t0 * dx, ay + t0 * dy, ax + t1 * dx, ay + t1 * dy), 0.0).sum(1)
    return np.maximum(0.5 * area2, 0.0)


def iou_pairs_np(A: np.ndarray, B: np.ndarray, block: int = 1 << 16) -> Tuple[np.ndarray, np.ndarray]:
    """(BEV IoU, 3D IoU) of A[k] with B[k], float64 [K] each.  Pairs whose
    bounding circles do not meet are 0 without being clipped (exact)."""
    A, B = np.asarray(A, np.float64).reshape(-1, 7), np.asarray(B, np.float64).reshape(-1, 7)
    bev, v3 = np.zeros(len(A)), np.zeros(len(A))
    rs = 0.5 * (np.hypot(A[:, 3], A[:, 4]) + np.hypot(B[:, 3], B[:, 4]))
    near = np.flatnonzero(np.hypot(B[:, 0] - A[:, 0], B[:, 1] - A[:, 1]) <= rs)
    for s in range(0, len(near), block):
        k = near[s:s + block]
        a, b = A[k], B[k]
        ov = overlap_pairs_np(a, b)
        bev[k] = ov / np.maximum(a[:, 3] * a[:, 4] + b[:, 3] * b[:, 4] - ov, 1e-8)
        h = np.maximum(0.0, np.minimum(a[:, 2] + a[:, 5] / 2, b[:, 2] + b[:, 5] / 2)
                       - np.maximum(a[:, 2] - a[:, 5] / 2, b[:, 2] - b[:, 5] / 2))
        inter = ov * h
        v3[k] = inter / np.maximum(a[:, 3] * a[:, 4] * a[:, 5] + b[:, 3] * b[:, 4] * b[:, 5] - inter, 1e-8)
    return bev, v3


def pair_indices(pred_off: np.ndarray, gt_off: np.ndarray, pair_off: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(prediction index, ground-truth index) of every output element."""
    n_pairs = np.diff(pair_off)
    f = np.repeat(np.arange(len(n_pairs)), n_pairs)
    local = np.arange(int(pair_off[-1])) - pair_off[f]
    ng = np.diff(gt_off)[f]
    return pred_off[f] + local // np.maximum(ng, 1), gt_off[f] + local % np.maximum(ng, 1)


def _box3d_iou_ragged_cpu(pred, gt, pred_off, gt_off, pair_off, pred_cls, gt_cls):
    pi, gi = pair_indices(pred_off, gt_off, pair_off)
    total = len(pi)
    bev, v3 = np.zeros(total), np.zeros(total)
    sel = np.arange(total) if pred_cls is None else np.flatnonzero(pred_cls[pi] == gt_cls[gi])
    bev[sel], v3[sel] = iou_pairs_np(pred[pi[sel]], gt[gi[sel]])
    return bev, v3


# ------------------------------------------------------------------------------- GPU
@dataclass
class RaggedIoU:
    """One prepared call: its inputs, tables and outputs in workspace buffers."""
    pred: torch.Tensor
    gt: torch.Tensor
    pred_cls: Optional[torch.Tensor]
    gt_cls: Optional[torch.Tensor]
    pred_off: torch.Tensor
    gt_off: torch.Tensor
    pair_off: torch.Tensor
    tile_frame: torch.Tensor
    tile_first: torch.Tensor
    iou_bev: torch.Tensor
    iou_3d: torch.Tensor
    n_tiles: int
    total: int


def _upload(ws: Workspace, name: str, a: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    t = ws.get(name, a.shape if a.size else (1,) + a.shape[1:], dtype)
    if a.size:
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dtype))
    return t


def prepare(ws: Workspace, pred, gt, pred_off, gt_off, pair_off, pred_cls=None, gt_cls=None,
            prefix: str = "iou3d_") -> RaggedIoU:
    """Upload one call's boxes, offsets and tile table into ``ws`` and size its
    outputs (every pair belongs to a frame with predictions and ground truth, so
    the tiles cover every output element)."""
    frame, first = tile_table(pred_off, gt_off)
    total = int(pair_off[-1])
    up = lambda n, a, dt: _upload(ws, prefix + n, a, dt)  # noqa: E731
    return RaggedIoU(up("pred", pred.astype(np.float32), torch.float32), up("gt", gt.astype(np.float32), torch.float32),
                     None if pred_cls is None else up("pred_cls", pred_cls.astype(np.int32), torch.int32),
                     None if gt_cls is None else up("gt_cls", gt_cls.astype(np.int32), torch.int32),
                     up("pred_off", pred_off.astype(np.int32), torch.int32),
                     up("gt_off", gt_off.astype(np.int32), torch.int32),
                     up("pair_off", pair_off.astype(np.int32), torch.int32),
                     up("tile_frame", frame, torch.int32), up("tile_first", first, torch.int32),
                     ws.get(prefix + "bev", (max(total, 1),), torch.float32),
                     ws.get(prefix + "3d", (max(total, 1),), torch.float32), len(frame), total)


def launch(c: RaggedIoU, stream=None) -> None:
    """The kernel launch alone: no allocation, no copy, no sync (graph-capturable)."""
    p = _native.ptr
    _native.call("tca_box3d_iou", p(c.pred), p(c.gt), p(c.pred_cls), p(c.gt_cls), p(c.pred_off), p(c.gt_off),
                 p(c.pair_off), p(c.tile_frame), p(c.tile_first), c.n_tiles, c.total, p(c.iou_bev), p(c.iou_3d),
                 _native.stream_ptr(stream))


def box3d_iou_ragged(pred, gt, pred_off, gt_off, pred_cls=None, gt_cls=None, device="auto",
                     ws: Optional[Workspace] = None):
    """→ ``(iou_bev, iou_3d, pair_off)``: both IoUs of every (prediction, ground
    truth) pair of every frame, flat, frame ``f``'s ``[np_f, ng_f]`` block
    row-major at ``pair_off[f]`` (int64 [F + 1]).

    ``pred`` [NP, 7] / ``gt`` [NG, 7]; ``pred_off`` / ``gt_off`` [F + 1];
    ``pred_cls`` / ``gt_cls`` both or neither.  On a GPU the HIP kernel computes
    in fp32 (results float32); on the CPU the float64 NumPy twin runs."""
    pred = np.asarray(pred, np.float64).reshape(-1, 7)
    gt = np.asarray(gt, np.float64).reshape(-1, 7)
    pred_off, gt_off = np.asarray(pred_off, np.int64).reshape(-1), np.asarray(gt_off, np.int64).reshape(-1)
    if len(pred_off) != len(gt_off) or len(pred_off) < 1:
        raise ValueError("pred_off and gt_off must both have F + 1 entries")
    if pred_off[0] != 0 or gt_off[0] != 0 or pred_off[-1] != len(pred) or gt_off[-1] != len(gt) \
            or (np.diff(pred_off) < 0).any() or (np.diff(gt_off) < 0).any():
        raise ValueError("offsets must start at 0, not decrease, and end at the number of boxes")
    if (pred_cls is None) != (gt_cls is None):
        raise ValueError("pred_cls and gt_cls: give both or neither")
    if pred_cls is not None:
        pred_cls, gt_cls = np.asarray(pred_cls).reshape(-1).astype(np.int64), np.asarray(gt_cls).reshape(-1).astype(np.int64)
        if len(pred_cls) != len(pred) or len(gt_cls) != len(gt):
            raise ValueError("one class per box")
    pair_off = np.concatenate([np.zeros(1, np.int64), np.cumsum(np.diff(pred_off) * np.diff(gt_off))])
    if int(pair_off[-1]) > INT32_MAX:
        raise ValueError(f"{int(pair_off[-1])} pairs do not fit the int32 offsets of one call: split the run")
    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu") if device in (None, "auto") \
        else torch.device(device)
    if dev.type != "cuda":
        bev, v3 = _box3d_iou_ragged_cpu(pred, gt, pred_off, gt_off, pair_off, pred_cls, gt_cls)
        return bev, v3, pair_off
    total = int(pair_off[-1])
    if total == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.float32), pair_off
    with torch.cuda.device(dev):
        c = prepare(ws if ws is not None else Workspace(dev), pred, gt, pred_off, gt_off, pair_off, pred_cls, gt_cls)
        launch(c)
        return c.iou_bev[:total].cpu().numpy(), c.iou_3d[:total].cpu().numpy(), pair_off
