"""K23 — the bird's-eye-view picture of a batch of LiDAR frames and their detections.

:func:`triton_client_amd.utils.bev.render_bev_frame` is the definition, bit for bit; the
HIP entry ``tca_bev_render`` (``csrc/kernels/bev_render.hip``) paints the same bytes on the
device.  CPU tensors and ``BevRenderer("cpu")`` run the definition frame by frame.

The box table is made on the host (:func:`bev_box_table`): the definition takes NumPy's fp32
``cos`` / ``sin`` of the yaw, which no device routine is bound to reproduce, and the
predictions are host arrays in every driver anyway.  One row of 12 int32 per box::

    0..7   the four corners (col, row) of utils.bev.box_corners_px (0 for a box that is not drawn)
    8      valid: 0 for a box with a NaN corner
    9      the label colour, r | g << 8 | b << 16
    10,11  byte offset and length of the box's label in the text buffer; length 0 for a box
           that gets no label (not valid, or every corner outside the image)

and one ragged buffer of ASCII text (``draw.label_text``).  No transcendental and no text
formatting runs on the device.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np
import torch

from .. import _native
from ..utils.bev import HEADING_COLOR, BevView, box_corners_px, label_color, render_bev_frame
from ..utils.draw import label_text
from ._ws import Workspace
from .cloud_common import CloudLayout, CloudStager, _align, cloud_bytes, fields_f32

ROW = 12  # int32 per box table row: kRow in bev_render.hip
INT32_MAX = 2 ** 31 - 1
assert HEADING_COLOR == (255, 80, 40)  # kHeading in bev_render.hip


def device_enabled() -> bool:
    """``TCA_DEVICE_BEV=0`` keeps the host painter on GPU engines too."""
    return os.environ.get("TCA_DEVICE_BEV", "1") != "0"


def device_takes(lay: CloudLayout) -> bool:
    """What ``tca_bev_render`` reads in place: little-endian FLOAT32 x, y, z and intensity
    inside the record (the painter's NaN-row rule needs the intensity field)."""
    return fields_f32(lay, (0, 1, 2, 3))


def plane_words(view: BevView) -> int:
    """int32 words of level-plane workspace per frame: four pixels per word, rows padded."""
    return view.H * ((view.W + 3) // 4)


def bev_box_table(boxes, scores, labels, count, view: BevView, names=None) -> Tuple[np.ndarray, bytes]:
    """→ ``(table int32 [k, 12], text)`` of boxes ``0..k-1``, ``k = min(count, len(boxes))``
    (``count`` None: all); the row layout is in the module docstring.  Built from
    ``box_corners_px``, ``label_color`` and ``label_text`` alone."""
    if boxes is None or len(boxes) == 0:
        return np.zeros((0, ROW), np.int32), b""
    boxes = np.asarray(boxes, np.float32)
    if boxes.ndim != 2 or boxes.shape[1] < 7:
        raise ValueError(f"boxes {boxes.shape}: [K, >= 7] rows")
    k = len(boxes) if count is None else max(0, min(int(count), len(boxes)))
    labels = np.asarray(labels).astype(np.int64)
    tab = np.zeros((k, ROW), np.int32)
    text = bytearray()
    H, W = view.H, view.W
    for i in range(k):
        cor = box_corners_px(boxes[i], view)
        r, g, b = label_color(labels[i])
        tab[i, 9] = r | (g << 8) | (b << 16)
        tab[i, 10] = len(text)
        if cor is None:
            continue
        tab[i, :8] = cor.reshape(-1)
        tab[i, 8] = 1
        if ((cor[:, 0] >= 0) & (cor[:, 0] < W) & (cor[:, 1] >= 0) & (cor[:, 1] < H)).any():
            t = label_text(int(labels[i]), scores[i], names).encode("ascii", "replace")
            tab[i, 11] = len(t)
            text += t
    return tab, bytes(text)


# --------------------------------------------------------------------------------- GPU
@dataclass
class BevCall:
    """One prepared launch: device views of its inputs, workspace and output."""
    data: torch.Tensor          # uint8: the payloads (frame b's records start at byte frame_offs[b]) and tables
    data_bytes: int             # bytes of ``data`` the kernel may read records from
    frame_off: torch.Tensor
    frame_n: torch.Tensor
    box_off: torch.Tensor
    table: torch.Tensor
    text: torch.Tensor
    plane: torch.Tensor
    out: torch.Tensor           # uint8 [B, H, W, 3]
    layout: CloudLayout         # offsets[3] == -1: dense rows
    consts: Tuple[float, ...]   # x1, y1, inv_res, z0, zscale, z_offset as Python floats of the fp32 values
    batch: int
    max_n: int
    n_boxes: int
    text_bytes: int
    frame_offs: Tuple[int, ...]


def launch(c: BevCall, stream=None) -> None:
    """The launch alone (the plane zeroing and the three kernels on ``stream``): no
    allocation, no copy, no sync, so it can be captured in a graph."""
    p = _native.ptr
    o = c.layout.offsets
    B, H, W, _ = c.out.shape
    _native.call("tca_bev_render", p(c.data), c.data_bytes, p(c.frame_off), p(c.frame_n), c.batch, c.max_n,
                 c.layout.point_step, o[0], o[1], o[2], o[3], *c.consts, H, W, p(c.plane), p(c.box_off), p(c.table),
                 c.n_boxes, p(c.text), c.text_bytes, p(c.out), c.out.stride(0) if B > 1 else H * c.out.stride(1),
                 c.out.stride(1), _native.stream_ptr(stream))


def _consts(view: BevView, z_offset: float) -> Tuple[float, ...]:
    return tuple(float(v) for v in (*view.constants(), np.float32(z_offset)))


def _concat_tables(tables: Sequence[np.ndarray], texts: Sequence[bytes]) -> Tuple[np.ndarray, bytes, np.ndarray]:
    """Frames' tables as one (text offsets rebased) → (table [K, 12], text, box_off [B + 1])."""
    out, to = [], 0
    for t, s in zip(tables, texts):
        t = np.array(t, np.int32).reshape(-1, ROW)
        t[:, 10] += to
        to += len(s)
        out.append(t)
    tab = np.concatenate(out) if out else np.zeros((0, ROW), np.int32)
    return tab, b"".join(texts), np.concatenate([[0], np.cumsum([len(t) for t in out])]).astype(np.int32)


class BevRenderer(CloudStager):
    """Paints clouds and their predictions: on a GPU with ``tca_bev_render`` (its own
    workspace, stream and pinned staging: one H2D of payloads and tables, one launch, one
    D2H of the pictures per batch of same-layout clouds), on the CPU with the definition.
    Clouds the kernel does not take (non-FLOAT32 or big-endian fields, no intensity field)
    go to the host painter with one warning."""

    @staticmethod
    def sections(tab: np.ndarray, text: bytes, box_off: np.ndarray) -> list:
        """What a batch stages after ``frame_off`` and ``frame_n``, in order (the arguments:
        :func:`_concat_tables`)."""
        return [("box_off", np.asarray(box_off, np.int32)), ("table", np.asarray(tab, np.int32)),
                ("text", np.frombuffer(text, np.uint8))]

    def prepare(self, payloads: Sequence, ns: Sequence[int], layout: CloudLayout, tables: Sequence[np.ndarray],
                texts: Sequence[bytes], view: BevView, z_offset: float = 0.0, stream=None,
                misalign: int = 0) -> BevCall:
        """Stage one batch (``payloads[b]``: the bytes of ``ns[b]`` points of ``layout``;
        ``tables[b]`` / ``texts[b]``: frame b's :func:`bev_box_table`) in pinned memory and
        upload it with one H2D copy on ``stream``.  ``misalign``: start every payload this many
        bytes past a 16-byte boundary."""
        if not device_takes(layout):
            raise ValueError(f"tca_bev_render does not take this layout: {layout}")
        B = len(payloads)
        ns = [int(n) for n in ns]
        tab, text, box_off = _concat_tables(tables, texts)
        K = len(tab)
        if B * plane_words(view) > INT32_MAX:
            raise ValueError(f"{B} pictures of {view.W}x{view.H} do not fit one call: split the batch")
        dev, plan, dview = self._stage("bev_in", payloads, ns, layout.point_step, misalign,
                                       self.sections(tab, text, box_off), stream)
        H, W = view.H, view.W
        words = max(B, 1) * plane_words(view)
        plane = self._device_buf("bev_plane", 4 * words)[:4 * words].view(torch.int32)
        out = self._device_buf("bev_out", max(B, 1) * H * W * 3)[:B * H * W * 3].view(B, H, W, 3)
        return BevCall(data=dev, data_bytes=plan.data_bytes, frame_off=dview("frame_off", B, torch.int64),
                       frame_n=dview("frame_n", B, torch.int32), box_off=dview("box_off", B + 1, torch.int32),
                       table=dview("table", ROW * K, torch.int32), text=dview("text", len(text), torch.uint8),
                       plane=plane, out=out, layout=layout, consts=_consts(view, z_offset), batch=B,
                       max_n=max(ns, default=0), n_boxes=K, text_bytes=len(text), frame_offs=plan.frame_offs)

    launch = staticmethod(launch)

    def _run_device(self, payloads, ns, layout, tables, texts, view, z_offset) -> List[np.ndarray]:
        with torch.cuda.device(self.device):
            st = self._own_stream()
            c = self.prepare(payloads, ns, layout, tables, texts, view, z_offset, st)
            launch(c, st)
            host = self._fetch(c.out.reshape(-1), c.out.numel(), st).reshape(c.out.shape)
        return [host[b].copy() for b in range(c.batch)]

    # ---------------------------------------------------------------------- API
    def render(self, clouds: Sequence, preds: Sequence[dict], view: BevView, names=None,
               z_offset: float = 0.0) -> List[np.ndarray]:
        """Per cloud the uint8 [H, W, 3] picture of ``cloud_to_numpy(cloud, z_offset=z_offset)``
        and ``preds[b]`` (``pred_boxes``, ``pred_scores``, ``pred_labels``) — what
        ``render_bev_frame(..., view, names, z_offset)`` paints."""
        def group_args(lay, idx):
            tt = [bev_box_table(preds[i]["pred_boxes"], preds[i]["pred_scores"], preds[i]["pred_labels"], None, view,
                                names) for i in idx]
            return (*cloud_bytes(clouds, idx), lay, [t for t, _ in tt], [s for _, s in tt], view, z_offset)

        return self._per_cloud(
            clouds, lambda i, lay: device_takes(lay),
            lambda i, lay: render_host(clouds[i], preds[i], view, names, z_offset), group_args, self._run_device,
            lambda i, lay: f"BevRenderer: tca_bev_render takes little-endian FLOAT32 x, y, z and intensity only "
                           f"(got {lay}); such clouds are painted on the host", host_layouts=False)


def render_host(cloud, pred: dict, view: BevView, names=None, z_offset: float = 0.0) -> np.ndarray:
    """One cloud through the definition."""
    from ..ros.compat import cloud_to_numpy

    pts = cloud_to_numpy(cloud, z_offset=z_offset)
    return render_bev_frame(pts, None, pred["pred_boxes"], pred["pred_scores"], pred["pred_labels"], None, view,
                            names, z_offset)


_OP_WS = {}  # device -> the workspace of render_bev_ on GPU tensors (the level plane)


def _render_device(out, points, n, box, score, label, count, view, names, z_offset) -> None:
    B, H, W, _ = out.shape
    maxp, F = points.shape[1], points.shape[2]
    ld = box.shape[1]
    # the one synchronising copy of this op: the predictions come to the host for the box table
    bh, sh, lh, ch = (t.cpu().numpy() for t in (box, score, label, count))
    tt = [bev_box_table(bh[b], sh[b], lh[b], max(0, min(int(ch[b]), ld)), view, names) for b in range(B)]
    tab, text, box_off = _concat_tables([t for t, _ in tt], [s for _, s in tt])
    sec, off = {}, 0
    for name, nbytes in (("box_off", box_off.nbytes), ("table", tab.nbytes), ("text", len(text))):
        sec[name] = off
        off = _align(off + max(nbytes, 4))
    host = np.zeros(off, np.uint8)
    host[sec["box_off"]:sec["box_off"] + box_off.nbytes] = box_off.view(np.uint8)
    host[sec["table"]:sec["table"] + tab.nbytes] = tab.reshape(-1).view(np.uint8)
    host[sec["text"]:sec["text"] + len(text)] = np.frombuffer(text, np.uint8)
    dev = torch.from_numpy(host).to(out.device)
    ws = _OP_WS.get(out.device)
    if ws is None:
        ws = _OP_WS[out.device] = Workspace(out.device)
    words = B * plane_words(view)
    if words > INT32_MAX:
        raise ValueError(f"{B} pictures of {W}x{H} do not fit one call: split the batch")
    plane = ws.get("bev_plane", (max(words, 1),), torch.int32)
    step = 4 * F
    c = BevCall(data=points, data_bytes=points.numel() * 4,
                frame_off=torch.arange(B, dtype=torch.int64, device=out.device) * (maxp * step),
                frame_n=n.clamp(0, maxp).contiguous(), box_off=dev[sec["box_off"]:sec["table"]].view(torch.int32),
                table=dev[sec["table"]:sec["text"]].view(torch.int32), text=dev[sec["text"]:], plane=plane, out=out,
                layout=CloudLayout(step, (0, 4, 8, -1), (7, 7, 7, 7)), consts=_consts(view, z_offset), batch=B,
                max_n=maxp, n_boxes=len(tab), text_bytes=len(text), frame_offs=())
    launch(c)


def render_bev_(out: torch.Tensor, points: torch.Tensor, n: torch.Tensor, box: torch.Tensor, score: torch.Tensor,
                label: torch.Tensor, count: torch.Tensor, view: BevView, names=None,
                z_offset: float = 0.0) -> torch.Tensor:
    """Fill ``out`` uint8 [B, H, W, 3] (rows ``out.stride(1) >= 3 * W`` bytes apart)
    with the picture of each frame.

    points [B, max_points, F >= 3] fp32 with n [B] int32 (z carries ``z_offset``
    on top of the frame ``view.z_range`` is given in); box [B, ld, D >= 7] fp32
    (yaw at index 8 when D >= 9), score [B, ld] fp32, label [B, ld] int32,
    count [B] int32; ``names[label]`` is a label's text.

    CPU tensors run the host painter.  With ``out`` on a GPU, ``points`` and ``n`` are on
    that GPU and ``tca_bev_render`` reads the points in place (dense mode) and writes into
    ``out`` on the current stream; ``box``, ``score``, ``label`` and ``count`` may be CPU or
    GPU tensors, and GPU ones are brought to the host with one synchronising copy, since the
    box table is made there (module docstring).  So this op allocates and synchronises and
    cannot be captured in a graph; :func:`launch` of a prepared :class:`BevCall` can."""
    if out.dim() != 4 or out.dtype != torch.uint8 or out.shape[3] != 3 or out.stride(3) != 1 or out.stride(2) != 3:
        raise ValueError("out must be uint8 [B, H, W, 3] with packed pixels")
    B, H, W, _ = out.shape
    if (H, W) != (view.H, view.W):
        raise ValueError(f"out is {W}x{H}, the view {view.W}x{view.H}")
    if out.stride(1) < 3 * W or (B > 1 and out.stride(0) < H * out.stride(1)):
        raise ValueError(f"out rows {out.stride(1)} B apart (< {3 * W}) or overlapping frames")
    if points.dim() != 3 or points.shape[0] != B or points.shape[2] < 3 or points.dtype != torch.float32 \
            or not points.is_contiguous():
        raise ValueError("points must be contiguous fp32 [B, max_points, >= 3]")
    if tuple(n.shape) != (B,) or n.dtype != torch.int32:
        raise ValueError("n must be int32 [B]")
    if box.dim() != 3 or box.shape[0] != B or box.shape[2] < 7 or box.dtype != torch.float32 \
            or not box.is_contiguous():
        raise ValueError("box must be contiguous fp32 [B, ld, >= 7]")
    ld = box.shape[1]
    if (tuple(score.shape) != (B, ld) or score.dtype != torch.float32 or tuple(label.shape) != (B, ld)
            or label.dtype != torch.int32 or tuple(count.shape) != (B,) or count.dtype != torch.int32
            or not score.is_contiguous() or not label.is_contiguous()):
        raise ValueError("score [B, ld] fp32, label [B, ld] int32 (contiguous) and count [B] int32")
    if out.is_cuda:
        if points.device != out.device or n.device != out.device:
            raise ValueError("out, points and n must be on one device")
        if any(t.device != out.device and t.is_cuda for t in (box, score, label, count)):
            raise ValueError("box, score, label and count must be on out's device or on the host")
        if B:
            _render_device(out, points, n, box, score, label, count, view, names, z_offset)
        return out
    if any(t.device != out.device for t in (points, n, box, score, label, count)):
        raise ValueError("out, points, n, box, score, label and count must be on one device")
    nh, ch = n.numpy(), count.numpy()
    for b in range(B):
        k = max(0, min(int(ch[b]), ld))
        img = render_bev_frame(points[b].numpy(), max(0, min(int(nh[b]), points.shape[1])), box[b, :k].numpy(),
                               score[b, :k].numpy(), label[b, :k].numpy(), k, view, names, z_offset)
        out[b].copy_(torch.from_numpy(img))
    return out
