"""K22 — points in boxes: which detection owns which LiDAR point.

:func:`points_in_boxes_numpy` is the definition, bit for bit, in float32 (the
pattern of ``utils/bev.py`` and ``ops/jpeg_encode.py::encode_numpy``); the HIP
kernel ``tca_points_in_boxes`` (``csrc/kernels/points_in_boxes.hip``) computes
the same bits on the device, and :func:`points_in_boxes_ref` is a float64
brute-force reference that also marks the pairs too close to a face for float32
to decide (``docs/precision.md``).

Points are the message's own ``(x, y, z)`` float32, boxes are
``boxes7(pred_boxes)`` = ``(cx, cy, cz, dx, dy, dz, yaw)`` with z the centre, in
the sensor frame (the engines remove their ``z_offset`` from the boxes they
return), one float32 score per box.  The host prepares the box table
(:func:`box_table`): ``hx = dx * 0.5f`` (exact), ``c = float32(cos(float64(yaw)))``,
``s = float32(sin(float64(yaw)))`` — no transcendental runs on the device.  Per
point and box, every operation rounded to float32 on its own (no FMA)::

    ex = x - cx;  ey = y - cy;  ez = z - cz
    lx = (ex * c) + (ey * s)
    ly = (ey * c) - (ex * s)
    inside = |lx| <= hx and |ly| <= hy and |ez| <= hz        # closed faces

A NaN compares false (the point is outside); a box with a non-finite entry
(its score included) or a dimension ``<= 0`` contains nothing: its table row is
all NaN.  ``owner[i]`` is the containing box with the highest score (ties: the
lowest index), -1 for none; ``count[k]`` is the number of points box ``k``
contains, owners or not.

The labelled cloud is a 28-byte record per point, the payload of the published
``PointCloud2`` (:data:`LABEL_FIELDS`): x, y, z, intensity as sent (0 without
an intensity field), ``label`` int32 (the owner's class, 0 for background),
``instance`` int32 (the owner's index, -1) and ``score`` float32 (0).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native
from ..ros import msgs
from .box3d import boxes7
from .cloud_common import (_PF_NP, CloudLayout, CloudStager, _align, cloud_bytes, cloud_layout,  # noqa: F401
                           cloud_xyzi, flat)

CHUNK = 128  # boxes per LDS stage: kChunk in points_in_boxes.hip
RECORD = 28  # bytes per labelled point
INT32_MAX = 2 ** 31 - 1
U = 2.0 ** -24  # unit roundoff of float32

LABEL_FIELDS = [msgs.PointField("x", 0, 7, 1), msgs.PointField("y", 4, 7, 1), msgs.PointField("z", 8, 7, 1),
                msgs.PointField("intensity", 12, 7, 1), msgs.PointField("label", 16, 5, 1),
                msgs.PointField("instance", 20, 5, 1), msgs.PointField("score", 24, 7, 1)]
RECORD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("label", "<i4"),
                         ("instance", "<i4"), ("score", "<f4")])
assert RECORD_DTYPE.itemsize == RECORD


# ------------------------------------------------------------------------- definition
def _boxes_scores(boxes, scores) -> Tuple[np.ndarray, np.ndarray]:
    b = np.asarray(boxes, np.float32)
    b = boxes7(b) if b.size else np.zeros((0, 7), np.float32)
    s = np.asarray(scores, np.float32).reshape(-1)
    if len(s) != len(b):
        raise ValueError(f"{len(b)} boxes but {len(s)} scores")
    return np.ascontiguousarray(b, np.float32), s


def box_table(boxes, scores) -> np.ndarray:
    """[K, 8] float32 rows ``(cx, cy, cz, hx, hy, hz, c, s)``; all NaN for a box that
    contains nothing (a non-finite entry or score, a dimension <= 0)."""
    b, sc = _boxes_scores(boxes, scores)
    t = np.empty((len(b), 8), np.float32)
    t[:, :3] = b[:, :3]
    t[:, 3:6] = b[:, 3:6] * np.float32(0.5)
    yaw = b[:, 6].astype(np.float64)
    with np.errstate(invalid="ignore"):
        t[:, 6] = np.cos(yaw).astype(np.float32)
        t[:, 7] = np.sin(yaw).astype(np.float32)
        bad = ~np.isfinite(b).all(1) | ~np.isfinite(sc) | (b[:, 3:6] <= 0).any(1)
    t[bad] = np.nan
    return t


def _inside_column(x, y, z, row) -> np.ndarray:
    """The definition for one table row over all points: float32, one rounding per operation."""
    with np.errstate(invalid="ignore"):
        ex, ey, ez = x - row[0], y - row[1], z - row[2]
        lx = (ex * row[6]) + (ey * row[7])
        ly = (ey * row[6]) - (ex * row[7])
        return (np.abs(lx) <= row[3]) & (np.abs(ly) <= row[4]) & (np.abs(ez) <= row[5])


def points_in_boxes_numpy(points, boxes, scores, return_inside: bool = False):
    """→ ``(owner [N] int32, count [K] int32)`` (and the ``[N, K]`` inside matrix):
    the definition.  ``points`` [N, >=3] (x, y, z); ``boxes`` [K, 7] or CenterPoint's
    [K, 9] (yaw at column 8); ``scores`` [K]."""
    p = np.asarray(points, np.float32)
    p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)
    x, y, z = (np.ascontiguousarray(p[:, j]) for j in range(3))
    _, sc = _boxes_scores(boxes, scores)
    tab = box_table(boxes, scores)
    n, k = len(p), len(tab)
    owner = np.full(n, -1, np.int32)
    best = np.zeros(n, np.float32)
    count = np.zeros(k, np.int32)
    inside = np.zeros((n, k), bool) if return_inside else None
    for j in range(k):
        m = _inside_column(x, y, z, tab[j])
        count[j] = m.sum()
        take = m & ((owner < 0) | (sc[j] > best))  # ascending j: a tie keeps the lower index
        owner[take] = j
        best[take] = sc[j]
        if inside is not None:
            inside[:, j] = m
    return (owner, count, inside) if return_inside else (owner, count)


def points_in_boxes_ref(points, boxes, scores=None, chunk: int = 8192):
    """Float64 brute force → ``(inside [N, K] bool, band [N, K] bool)``.

    ``band`` marks the pairs whose distance to a face is within the rounding bound
    of the float32 evaluation, where the definition may legitimately differ from
    ``inside``: ``5 * 2**-24 * (|ex| + |ey|)`` for the two rotated coordinates (one
    rounding each for the subtraction, for c or s, for the product and for the sum:
    at most ``4u`` of ``|ex||c| + |ey||s|``, one more ``u`` of slack for the second-
    order terms) and ``2**-24 * |ez|`` for z (the one subtraction).  The half sizes
    are exact.  ``docs/precision.md`` has the derivation."""
    p = np.asarray(points, np.float32).astype(np.float64)
    p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)
    b = np.asarray(boxes, np.float32)
    b = (boxes7(b) if b.size else np.zeros((0, 7), np.float32)).astype(np.float64)
    k = len(b)
    sc = np.zeros(k) if scores is None else np.asarray(scores, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(b).all(1) & np.isfinite(sc) & (b[:, 3:6] > 0).all(1)
        c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
    hx, hy, hz = 0.5 * b[:, 3], 0.5 * b[:, 4], 0.5 * b[:, 5]
    inside = np.zeros((len(p), k), bool)
    band = np.zeros((len(p), k), bool)
    with np.errstate(invalid="ignore"):
        for s0 in range(0, len(p), chunk):
            q = p[s0:s0 + chunk]
            ex, ey, ez = q[:, 0:1] - b[:, 0], q[:, 1:2] - b[:, 1], q[:, 2:3] - b[:, 2]
            lx, ly = ex * c + ey * s, ey * c - ex * s
            bxy = 5.0 * U * (np.abs(ex) + np.abs(ey))
            bz = U * np.abs(ez)
            inside[s0:s0 + chunk] = ok & (np.abs(lx) <= hx) & (np.abs(ly) <= hy) & (np.abs(ez) <= hz)
            band[s0:s0 + chunk] = ok & ((np.abs(np.abs(lx) - hx) <= bxy) | (np.abs(np.abs(ly) - hy) <= bxy)
                                        | (np.abs(np.abs(ez) - hz) <= bz))
    return inside, band


def pack_records(xyzi: np.ndarray, owner: np.ndarray, scores, labels) -> np.ndarray:
    """The labelled cloud's records (:data:`RECORD_DTYPE`) of points ``[N, 4]`` float32
    (x, y, z, intensity: bits kept) and their owners."""
    xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    owner = np.asarray(owner, np.int32).reshape(-1)
    sc = np.asarray(scores, np.float32).reshape(-1)
    lb = np.asarray(labels).reshape(-1).astype(np.int32)
    rec = np.zeros(len(owner), RECORD_DTYPE)
    raw = rec.view(np.uint32).reshape(-1, 7)
    raw[:, :4] = xyzi.view(np.uint32)
    has = owner >= 0
    o = owner[has]
    rec["instance"] = owner
    rec["label"][has] = lb[o]
    rec["score"][has] = sc[o]
    return rec


def labelled_cloud(cloud, payload) -> msgs.PointCloud2:
    """The published message: the cloud's header, height, width and is_dense, 28-byte records."""
    return msgs.PointCloud2(header=cloud.header, height=cloud.height, width=cloud.width, fields=list(LABEL_FIELDS),
                            is_bigendian=False, point_step=RECORD, row_step=RECORD * int(cloud.width),
                            data=payload, is_dense=cloud.is_dense)


# --------------------------------------------------------------------------------- GPU
@dataclass
class LabelCall:
    """One prepared launch: device views of its inputs and outputs."""
    data: torch.Tensor
    frame_off: torch.Tensor
    frame_n: torch.Tensor
    box_off: torch.Tensor
    pt_off: torch.Tensor
    table: torch.Tensor
    score: torch.Tensor
    label: torch.Tensor
    owner: torch.Tensor
    count: torch.Tensor
    record: Optional[torch.Tensor]
    layout: CloudLayout
    batch: int
    max_n: int
    n_boxes: int
    total: int
    out: torch.Tensor  # owner | count | record, one device buffer (one D2H)
    out_sections: Tuple[int, int, int]  # byte offsets of owner, count, record in ``out``


def launch(c: LabelCall, stream=None) -> None:
    """The launch alone (the count zeroing and the kernel on ``stream``): no allocation,
    no copy, no sync."""
    p = _native.ptr
    o = c.layout.offsets
    _native.call("tca_points_in_boxes", p(c.data), p(c.frame_off), p(c.frame_n), c.batch, c.max_n,
                 c.layout.point_step, o[0], o[1], o[2], o[3], p(c.box_off), p(c.table), p(c.score), p(c.label),
                 c.n_boxes, p(c.pt_off), p(c.owner), p(c.count), p(c.record), _native.stream_ptr(stream))


def out_sections(total: int, n_boxes: int) -> Tuple[int, int, int]:
    """Byte offsets of owner, count and record in the output buffer of ``total`` points."""
    o_count = _align(4 * max(total, 1))
    return 0, o_count, o_count + _align(4 * max(n_boxes, 1))


class PointLabeler(CloudStager):
    """Labels clouds against boxes: on a GPU with ``tca_points_in_boxes`` (its own
    workspace, stream and pinned staging: one H2D of payloads and tables, one launch,
    one D2H of owners, counts and records per batch of same-layout clouds), on the CPU
    with the definition.  Clouds the kernel does not take (non-FLOAT32 or big-endian
    fields) run the definition with one warning."""

    @staticmethod
    def sections(ns: Sequence[int], tables: Sequence, scores: Sequence, labels: Sequence) -> list:
        """What a batch stages after ``frame_off`` and ``frame_n``, in order."""
        return [("box_off", np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int32)),
                ("pt_off", np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)),
                ("table", flat(tables, np.float32)), ("score", flat(scores, np.float32)),
                ("label", flat(labels, np.int32))]

    def prepare(self, payloads: Sequence, ns: Sequence[int], layout: CloudLayout, tables: Sequence[np.ndarray],
                scores: Sequence[np.ndarray], labels: Sequence[np.ndarray], records: bool = True,
                stream=None, misalign: int = 0) -> LabelCall:
        """Stage one batch (``payloads[b]``: the bytes of ``ns[b]`` points of ``layout``;
        ``tables[b]`` / ``scores[b]`` / ``labels[b]``: frame b's :func:`box_table` rows, scores
        and int labels) in pinned memory and upload it with one H2D copy on ``stream``.
        ``misalign``: start every payload this many bytes past a 16-byte boundary."""
        if not layout.device_ok:
            raise ValueError(f"tca_points_in_boxes does not take this layout: {layout}")
        B = len(payloads)
        ns = [int(n) for n in ns]
        K, total = sum(len(t) for t in tables), sum(ns)
        if total > INT32_MAX // RECORD:
            raise ValueError(f"{total} points do not fit the int32 offsets of one call: split the batch")
        dev, _, view = self._stage("pib_in", payloads, ns, layout.point_step, misalign,
                                   self.sections(ns, tables, scores, labels), stream)
        o_owner, o_count, o_rec = out_sections(total, K)
        out = self._device_buf("pib_out", o_rec + (RECORD * max(total, 1) if records else 0))
        i32, f32, i64 = torch.int32, torch.float32, torch.int64
        return LabelCall(
            data=dev, frame_off=view("frame_off", B, i64), frame_n=view("frame_n", B, i32),
            box_off=view("box_off", B + 1, i32), pt_off=view("pt_off", B + 1, i32), table=view("table", 8 * K, f32),
            score=view("score", K, f32), label=view("label", K, i32),
            owner=out[o_owner:o_owner + 4 * max(total, 1)].view(i32),
            count=out[o_count:o_count + 4 * max(K, 1)].view(i32),
            record=out[o_rec:o_rec + RECORD * max(total, 1)] if records else None,
            layout=layout, batch=B, max_n=max(ns, default=0), n_boxes=K, total=total, out=out,
            out_sections=(o_owner, o_count, o_rec))

    launch = staticmethod(launch)

    def _run_device(self, payloads, ns, layout, tables, scores, labels):
        """→ per frame (owner, count, payload bytes)."""
        with torch.cuda.device(self.device):
            st = self._own_stream()
            c = self.prepare(payloads, ns, layout, tables, scores, labels, True, st)
            launch(c, st)
            host = self._fetch(c.out, c.out_sections[2] + RECORD * c.total, st)
        owner = host[:4 * c.total].view(np.int32)
        count = host[c.out_sections[1]:c.out_sections[1] + 4 * c.n_boxes].view(np.int32)
        rec = host[c.out_sections[2]:c.out_sections[2] + RECORD * c.total]
        out, po, ko = [], 0, 0
        for n, t in zip(ns, tables):
            out.append((owner[po:po + n].copy(), count[ko:ko + len(t)].copy(),
                        rec[RECORD * po:RECORD * (po + n)].tobytes()))
            po, ko = po + n, ko + len(t)
        return out

    # ---------------------------------------------------------------------- API
    def label(self, clouds: Sequence, boxes: Sequence, scores: Sequence, labels: Sequence) -> List[tuple]:
        """Per cloud ``(owner [N] int32, count [K] int32, payload)``: ``payload`` is the bytes of
        the labelled cloud's 28-byte records (:func:`labelled_cloud`).  ``boxes[b]`` [K, 7 or 9],
        ``scores[b]`` [K] and ``labels[b]`` [K] belong to ``clouds[b]``."""
        def group_args(lay, idx):
            return (*cloud_bytes(clouds, idx), lay, [box_table(boxes[i], scores[i]) for i in idx],
                    [np.asarray(scores[i], np.float32).reshape(-1) for i in idx],
                    [np.asarray(labels[i]).reshape(-1) for i in idx])

        return self._per_cloud(
            clouds, lambda i, lay: lay.device_ok,
            lambda i, lay: label_numpy(clouds[i], boxes[i], scores[i], labels[i], lay), group_args, self._run_device,
            lambda i, lay: f"PointLabeler: tca_points_in_boxes takes little-endian FLOAT32 x, y, z and intensity "
                           f"only (got {lay}); such clouds are labelled on the host")

    def count_points(self, cloud, boxes) -> np.ndarray:
        """Points of ``cloud`` inside each of ``boxes`` [K, 7] (every box scores 0)."""
        k = len(boxes)
        return self.label([cloud], [boxes], [np.zeros(k, np.float32)], [np.zeros(k, np.int32)])[0][1]


def label_numpy(cloud, boxes, scores, labels, lay: Optional[CloudLayout] = None) -> tuple:
    """One cloud through the definition → ``(owner, count, payload)``."""
    xyzi = cloud_xyzi(cloud, lay)
    owner, count = points_in_boxes_numpy(xyzi, boxes, scores)
    return owner, count, pack_records(xyzi, owner, scores, labels).tobytes()


def xyz_cloud(points: np.ndarray, header=None) -> msgs.PointCloud2:
    """A PointCloud2 of bare FLOAT32 x, y, z records (``point_step`` 12): what the
    evaluator keeps of a cloud that waits for its ground truth."""
    p = np.ascontiguousarray(np.asarray(points, np.float32)[:, :3])
    return msgs.PointCloud2(header=header or msgs.Header(), height=1, width=len(p),
                            fields=[msgs.PointField("x", 0, 7, 1), msgs.PointField("y", 4, 7, 1),
                                    msgs.PointField("z", 8, 7, 1)],
                            is_bigendian=False, point_step=12, row_step=12 * len(p), data=p.tobytes(), is_dense=False)
