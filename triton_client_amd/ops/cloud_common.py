"""What the ops that read raw ``PointCloud2`` payloads in place share on the host — the point
labeler (``ops/points_in_boxes.py``, K22), the bird's-eye-view painter (``ops/bev.py``, K23) and
the camera ranger (``ops/range2d.py``, K26), the depth imager (``ops/depth_image.py``, K27), the
laser scanner (``ops/laser_scan.py``, K29) and the ground splitter (``ops/ground.py``, K30): where
a cloud's fields lie (:class:`CloudLayout`), which of them a kernel can read in place
(:func:`fields_f32`), the byte layout of one staged batch (:func:`plan_staging`,
:func:`fill_staging`: no torch in either), and the device side of such an op
(:class:`CloudStager`).

One staged batch is one buffer: frame b's records at ``frame_offs[b]`` (16-byte aligned, plus
``misalign``), then ``frame_off`` int64 [B], ``frame_n`` int32 [B] and the op's own sections,
each 16-byte aligned and at least 4 bytes long.
"""
from __future__ import annotations

import contextlib
import threading
import warnings
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._ws import Workspace

# ------------------------------------------------------------------------------ clouds
_PF_NP = {1: "i1", 2: "u1", 3: "<i2", 4: "<u2", 5: "<i4", 6: "<u4", 7: "<f4", 8: "<f8"}


def fields_f32(lay: "CloudLayout", js: Sequence[int]) -> bool:
    """Are fields ``js`` (0: x, 1: y, 2: z, 3: intensity) little-endian FLOAT32 inside the record?"""
    if lay.bigendian or lay.point_step <= 0:
        return False
    return all(lay.dtypes[j] == 7 and 0 <= lay.offsets[j] and lay.offsets[j] + 4 <= lay.point_step for j in js)


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
        return fields_f32(self, (0, 1, 2, 3) if self.offsets[3] >= 0 else (0, 1, 2))


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


# ----------------------------------------------------------------------------- staging
def _align(n: int, a: int = 16) -> int:
    return (n + a - 1) // a * a


@dataclass(frozen=True)
class StagePlan:
    """Byte offsets of one staged batch."""
    frame_offs: Tuple[int, ...]  # where each frame's records start
    data_bytes: int              # the records end here: what a kernel may read records from
    sections: Dict[str, int]     # where each section starts
    total: int


def plan_staging(ns: Sequence[int], point_step: int, misalign: int,
                 sections: Sequence[Tuple[str, int]]) -> StagePlan:
    """Frames of ``ns[b]`` records of ``point_step`` bytes, each started ``misalign`` bytes past a
    16-byte boundary, then ``sections`` ``(name, nbytes)`` in their order."""
    off, frame_offs = 0, []
    for n in ns:
        frame_offs.append(off + misalign)
        off = _align(off + misalign + int(n) * point_step)
    data_bytes, sec = off, {}
    for name, nbytes in sections:
        sec[name] = off
        off = _align(off + max(nbytes, 4))
    return StagePlan(tuple(frame_offs), data_bytes, sec, off)


def batch_sections(ns: Sequence[int], arrays: Sequence[Tuple[str, np.ndarray]]) -> List[Tuple[str, int]]:
    """The section list of a batch whose op stages ``arrays`` ``(name, array)``: ``frame_off``
    and ``frame_n`` come first."""
    return [("frame_off", 8 * len(ns)), ("frame_n", 4 * len(ns))] + [(name, a.nbytes) for name, a in arrays]


def fill_staging(host: np.ndarray, plan: StagePlan, payloads: Sequence, ns: Sequence[int], point_step: int,
                 arrays: Sequence[Tuple[str, np.ndarray]]) -> None:
    """Write the batch into ``host`` (uint8): the payloads, ``frame_off``, ``frame_n`` and the
    op's ``arrays``, each as its own dtype's bytes.  No other byte of ``host`` is touched."""
    for pl, n, fo in zip(payloads, ns, plan.frame_offs):
        if n:
            host[fo:fo + n * point_step] = np.frombuffer(pl, np.uint8, n * point_step)
    for name, a in (("frame_off", np.asarray(plan.frame_offs, np.int64)), ("frame_n", np.asarray(ns, np.int32)),
                    *arrays):
        a = np.ascontiguousarray(a).reshape(-1)
        host[plan.sections[name]:plan.sections[name] + a.nbytes] = a.view(np.uint8)


def flat(parts: Sequence, dt) -> np.ndarray:
    """``parts`` as one flat array of ``dt`` (empty without parts)."""
    return np.concatenate([np.zeros(0, dt)] + [np.asarray(p).reshape(-1).astype(dt, copy=False) for p in parts])


def cloud_bytes(clouds: Sequence, idx: Sequence[int]) -> Tuple[list, List[int]]:
    """``(payloads, ns)`` of ``clouds[i]`` for ``i`` in ``idx``."""
    return [clouds[i].data for i in idx], [int(clouds[i].width) * int(clouds[i].height) for i in idx]


class CloudStager:
    """The device side of a cloud-reading op: its own workspace, stream and pinned staging; per
    batch of same-layout clouds one H2D copy (:meth:`_stage`), the subclass's launch, one D2H copy
    and one synchronize (:meth:`_fetch`), all on that stream; :meth:`_per_cloud` sends each cloud
    to the device or to the definition.  A batch is cut into several launches (:meth:`_parts`)
    by ``CameraRanger``, ``DepthImager`` (``ops/depth_image.py``, K27, whose cut also bounds the
    key plane), ``LaserScanner`` (``ops/laser_scan.py``, K29) and ``GroundSplitter``
    (``ops/ground.py``, K30, whose cut also bounds the cell plane): ``tca_range2d``,
    ``tca_depth_image``, ``tca_laser_scan`` and ``tca_ground_split`` refuse more than 64 frames or
    2^31 record bytes, while ``tca_points_in_boxes`` checks neither (64-bit frame offsets; its int32 point offsets are
    refused in ``prepare``) and ``tca_bev_render`` takes 65535 frames and a 64-bit byte count."""

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

    def _own_stream(self):
        if self._stream is None:
            self._stream = torch.cuda.Stream(self.device)
        return self._stream

    def _stage(self, buf: str, payloads: Sequence, ns: Sequence[int], point_step: int, misalign: int,
               arrays: Sequence[Tuple[str, np.ndarray]], stream=None):
        """Plan the batch, fill pinned memory and upload it into workspace buffer ``buf`` with one
        H2D copy on ``stream`` → ``(dev, plan, view)``; ``view(name, count, dtype)`` is section
        ``name`` as ``max(count, 1)`` elements of a torch dtype."""
        plan = plan_staging(ns, point_step, misalign, batch_sections(ns, arrays))
        pin = self._pinned("_pin_in", plan.total)
        fill_staging(pin.numpy(), plan, payloads, ns, point_step, arrays)
        dev = self._device_buf(buf, plan.total)
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            dev[:plan.total].copy_(pin[:plan.total], non_blocking=True)

        def view(name, count, dt):
            return dev[plan.sections[name]:plan.sections[name] + max(count, 1) * dt.itemsize].view(dt)

        return dev, plan, view

    def _fetch(self, src: torch.Tensor, nbytes: int, stream) -> np.ndarray:
        """The first ``nbytes`` of ``src`` (flat uint8 on the device) as host bytes: one D2H copy
        into pinned memory on ``stream`` and its synchronize."""
        pin = self._pinned("_pin_out", nbytes)
        with torch.cuda.stream(stream):
            pin[:nbytes].copy_(src[:nbytes], non_blocking=True)
        stream.synchronize()
        return pin.numpy()[:nbytes]

    # -------------------------------------------------------------------- clouds
    def _parts(self, idx: List[int], clouds: Sequence):
        """``idx`` (clouds of one layout) cut into launches: one."""
        return [idx]

    def _per_cloud(self, clouds: Sequence, takes: Callable, on_host: Callable, group_args: Callable,
                   on_device: Callable, warning: Callable, device: Optional[bool] = None,
                   host_layouts: bool = True, parts: Optional[Callable] = None) -> list:
        """One result per cloud, in input order.  With ``device`` (default: ``self.gpu``), cloud
        ``i`` of layout ``lay`` goes to the device when ``takes(i, lay)``: for clouds ``part``, all
        of one layout, ``on_device(*group_args(lay, part))`` returns their results; it alone runs
        under the lock.  Every other cloud is ``on_host(i, lay)``, with one ``warning(i, lay)`` in
        this object's life if there is a device.  ``host_layouts`` False: no layout is computed
        without a device.  ``parts``: cuts a layout's clouds into launches in place of
        :meth:`_parts` (a cut that depends on the call's options)."""
        device = self.gpu if device is None else device
        lays = [cloud_layout(c) for c in clouds] if device or host_layouts else [None] * len(clouds)
        out: List[Optional[object]] = [None] * len(clouds)
        groups = {}
        for i, lay in enumerate(lays):
            if device and takes(i, lay):
                groups.setdefault(lay, []).append(i)
                continue
            if device and not self._warned:
                self._warned = True
                warnings.warn(warning(i, lay), RuntimeWarning, stacklevel=3)
            out[i] = on_host(i, lay)
        for lay, idx in groups.items():
            for part in (parts or self._parts)(idx, clouds):
                args = group_args(lay, part)
                with self._lock:
                    res = on_device(*args)
                for i, r in zip(part, res):
                    out[i] = r
        return out
