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

import contextlib
import threading
import warnings
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native
from ..ros import msgs
from ._ws import Workspace
from .box3d import boxes7

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


# ------------------------------------------------------------------------------ clouds
_PF_NP = {1: "i1", 2: "u1", 3: "<i2", 4: "<u2", 5: "<i4", 6: "<u4", 7: "<f4", 8: "<f8"}


@dataclass(frozen=True)
class CloudLayout:
    """Where x, y, z and intensity (offset -1: none) lie in a point record."""
    point_step: int
    offsets: Tuple[int, int, int, int]
    dtypes: Tuple[int, int, int, int]
    bigendian: bool = False

    @property
    def device_ok(self) -> bool:
        """What ``tca_points_in_boxes`` takes: little-endian FLOAT32 fields inside the record."""
        if self.bigendian or self.point_step <= 0:
            return False
        for j, (o, d) in enumerate(zip(self.offsets, self.dtypes)):
            if j == 3 and o < 0:
                continue
            if d != 7 or o < 0 or o + 4 > self.point_step:
                return False
        return True


def cloud_layout(msg) -> CloudLayout:
    by = {f.name: f for f in msg.fields}
    missing = [n for n in ("x", "y", "z") if n not in by]
    if missing:
        raise ValueError(f"PointCloud2 lacks fields {missing}")
    f = [by["x"], by["y"], by["z"], by.get("intensity")]
    return CloudLayout(int(msg.point_step), tuple(-1 if g is None else int(g.offset) for g in f),
                       tuple(7 if g is None else int(g.datatype) for g in f), bool(msg.is_bigendian))


def cloud_xyzi(msg, lay: Optional[CloudLayout] = None) -> np.ndarray:
    """[N, 4] float32 x, y, z, intensity of every point of the message, in input order, NaN
    points included (FLOAT32 fields keep their bits; 0 without an intensity field)."""
    lay = lay or cloud_layout(msg)
    n = int(msg.width) * int(msg.height)
    out = np.zeros((n, 4), np.float32)
    if n == 0:
        return out
    use = [j for j in range(4) if lay.offsets[j] >= 0]
    fmt = [_PF_NP[lay.dtypes[j]] for j in use]
    if lay.bigendian:
        fmt = [f.replace("<", ">") for f in fmt]
    dt = np.dtype({"names": [str(j) for j in use], "formats": fmt, "offsets": [lay.offsets[j] for j in use],
                   "itemsize": lay.point_step})
    rec = np.frombuffer(msg.data, dtype=dt, count=n)
    for j in use:
        col = rec[str(j)]
        if lay.dtypes[j] == 7 and not lay.bigendian:
            out.view(np.uint32)[:, j] = col.view(np.uint32)
        else:
            out[:, j] = col
    return out


def labelled_cloud(cloud, payload) -> msgs.PointCloud2:
    """The published message: the cloud's header, height, width and is_dense, 28-byte records."""
    return msgs.PointCloud2(header=cloud.header, height=cloud.height, width=cloud.width, fields=list(LABEL_FIELDS),
                            is_bigendian=False, point_step=RECORD, row_step=RECORD * int(cloud.width),
                            data=payload, is_dense=cloud.is_dense)


# --------------------------------------------------------------------------------- GPU
def _align(n: int, a: int = 16) -> int:
    return (n + a - 1) // a * a


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


class PointLabeler:
    """Labels clouds against boxes: on a GPU with ``tca_points_in_boxes`` (its own
    workspace, stream and pinned staging: one H2D of payloads and tables, one launch,
    one D2H of owners, counts and records per batch of same-layout clouds), on the CPU
    with the definition.  Clouds the kernel does not take (non-FLOAT32 or big-endian
    fields) run the definition with one warning."""

    def __init__(self, device="auto", ws: Optional[Workspace] = None):
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu") if device in (None, "auto") \
            else torch.device(device)
        self.gpu = self.device.type == "cuda"
        self.ws = ws if ws is not None else (Workspace(self.device) if self.gpu else None)
        self._lock = threading.Lock()
        self._pin_in = self._pin_out = None
        self._stream = None
        self._warned = False

    # ------------------------------------------------------------------ staging
    def _pinned(self, name: str, nbytes: int) -> torch.Tensor:
        t = getattr(self, name)
        if t is None or t.numel() < nbytes:
            t = torch.empty((max(4096, 1 << (nbytes - 1).bit_length()),), dtype=torch.uint8, pin_memory=True)
            setattr(self, name, t)
        return t

    def _device_buf(self, name: str, nbytes: int) -> torch.Tensor:
        cur = self.ws._bufs.get(name)
        if cur is not None and cur.numel() >= nbytes:
            return cur
        return self.ws.get(name, (max(4096, 1 << (nbytes - 1).bit_length()),), torch.uint8)

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
        nb = [len(t) for t in tables]
        K, total = sum(nb), sum(ns)
        if total > INT32_MAX // RECORD:
            raise ValueError(f"{total} points do not fit the int32 offsets of one call: split the batch")
        step = layout.point_step
        off, frame_off = 0, []
        for n in ns:
            frame_off.append(off + misalign)
            off = _align(off + misalign + n * step)
        sec = {}
        for name, nbytes in (("frame_off", 8 * B), ("frame_n", 4 * B), ("box_off", 4 * (B + 1)),
                             ("pt_off", 4 * (B + 1)), ("table", 32 * K), ("score", 4 * K), ("label", 4 * K)):
            sec[name] = off
            off = _align(off + max(nbytes, 4))
        pin = self._pinned("_pin_in", off)
        host = pin.numpy()
        for pl, n, fo in zip(payloads, ns, frame_off):
            if n:
                host[fo:fo + n * step] = np.frombuffer(pl, np.uint8, n * step)

        def put(name, a, dt):
            a = np.ascontiguousarray(a, dt).reshape(-1)
            host[sec[name]:sec[name] + a.nbytes] = a.view(np.uint8)

        put("frame_off", frame_off, np.int64)
        put("frame_n", ns, np.int32)
        put("box_off", np.concatenate([[0], np.cumsum(nb)]), np.int32)
        put("pt_off", np.concatenate([[0], np.cumsum(ns)]), np.int32)
        if K:
            put("table", np.concatenate([np.asarray(t, np.float32).reshape(-1, 8) for t in tables]), np.float32)
            put("score", np.concatenate([np.asarray(s, np.float32).reshape(-1) for s in scores]), np.float32)
            put("label", np.concatenate([np.asarray(v).reshape(-1).astype(np.int32) for v in labels]), np.int32)
        dev = self._device_buf("pib_in", off)
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            dev[:off].copy_(pin[:off], non_blocking=True)

        def view(name, count, dt):
            return dev[sec[name]:sec[name] + max(count, 1) * dt.itemsize].view(dt)

        o_owner = 0
        o_count = _align(4 * max(total, 1))
        o_rec = o_count + _align(4 * max(K, 1))
        out_bytes = o_rec + (RECORD * max(total, 1) if records else 0)
        out = self._device_buf("pib_out", out_bytes)
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
            if self._stream is None:
                self._stream = torch.cuda.Stream(self.device)
            st = self._stream
            c = self.prepare(payloads, ns, layout, tables, scores, labels, True, st)
            launch(c, st)
            nbytes = c.out_sections[2] + RECORD * c.total
            pin = self._pinned("_pin_out", nbytes)
            with torch.cuda.stream(st):
                pin[:nbytes].copy_(c.out[:nbytes], non_blocking=True)
            st.synchronize()
        host = pin.numpy()
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
        lays = [cloud_layout(c) for c in clouds]
        out: List[Optional[tuple]] = [None] * len(clouds)
        groups = {}
        for i, lay in enumerate(lays):
            if self.gpu and lay.device_ok:
                groups.setdefault(lay, []).append(i)
                continue
            if self.gpu and not self._warned:
                self._warned = True
                warnings.warn(f"PointLabeler: tca_points_in_boxes takes little-endian FLOAT32 x, y, z and intensity "
                              f"only (got {lay}); such clouds are labelled on the host", RuntimeWarning,
                              stacklevel=2)
            out[i] = label_numpy(clouds[i], boxes[i], scores[i], labels[i], lay)
        for lay, idx in groups.items():
            tabs = [box_table(boxes[i], scores[i]) for i in idx]
            with self._lock:
                res = self._run_device([clouds[i].data for i in idx],
                                       [int(clouds[i].width) * int(clouds[i].height) for i in idx], lay, tabs,
                                       [np.asarray(scores[i], np.float32).reshape(-1) for i in idx],
                                       [np.asarray(labels[i]).reshape(-1) for i in idx])
            for i, r in zip(idx, res):
                out[i] = r
        return out

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
