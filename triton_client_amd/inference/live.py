"""The live drivers' device path: sensor messages in, publishable results out.

The reference's product is its subscriber callback — one message, decode,
preprocess, one blocking ``ModelInfer``, NMS, draw, publish
(``communicator/ros_inference.py:117-175``; ``communicator/ros_inference3d.py:120-213``).
Here :class:`~triton_client_amd.inference.ros_inference.RosInference` /
:class:`~triton_client_amd.inference.ros_inference3d.RosInference3D` hand
micro-batches of messages to these executors, which keep the frames on the
device from ingest to the one D2H copy the publisher needs:

camera (:class:`LiveCamera`)
    ``CompressedImage`` JPEG: C++ Huffman decode (``csrc/runtime/jpeg_entropy.cpp``,
    host threads, no GIL) straight into a pinned slot -> H2D -> HIP IDCT +
    colour (``csrc/kernels/jpeg.hip``) into the pipeline's frame buffer.  Raw
    ``Image`` rgb8: the rows are gathered into the pinned slot by C++ threads
    (``csrc/runtime/host_copy.cpp``).  Every other raw ``Image`` encoding (bgr8 /
    rgba8 / bgra8, mono8 / mono16, YUV 4:2:2, 8-bit Bayer, rgb8 with padded rows):
    the payload as the sensor sent it is gathered into the pinned slot -> H2D ->
    HIP conversion to rgb8 (``csrc/kernels/encodings.hip``) into the frame buffer
    (``TCA_DEVICE_ENCODINGS=0``: converted on the host instead).  Then the
    captured YOLOv5 / YOLOv4 / Detectron step, and boxes + labels drawn on the resident frames
    (``csrc/kernels/draw.hip``); with ``process(..., rectify=Rectifier)`` the frames are
    rectified from the camera's calibration on the device first (``csrc/kernels/rectify.hip``,
    the last step before the captured one); the annotated frames and the detections come
    back in one D2H into pinned memory that the published ``Image`` wraps
    without a copy.  With ``process(..., compressed=JpegOptions(...))`` the step
    also encodes the annotated frames (``csrc/kernels/jpeg_encode.hip``) and
    the files come back instead of the frames, a quarter of the bytes, each
    wrapped by a ``CompressedImage``.
LiDAR (:class:`LiveLidar`)
    ``PointCloud2`` payload bytes gathered into a pinned slot -> H2D -> the
    captured unpack / voxelise / network / NMS step -> one D2H of the result
    rows; the jsk ``BoundingBoxArray`` is built from those columns.

Both run on :class:`~triton_client_amd.pipelines.stream.StreamExecutor`: two
input sets, one captured graph per set, separate H2D / compute / D2H streams.
There is no engine-wide lock: several driver workers stage, submit and
collect batches concurrently; only the enqueue itself is serialised.
"""
from __future__ import annotations

import ctypes
import logging
import os
import threading
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native
from ..ops import golden
from ..ops.image import image_frame_bytes, image_to_rgb8
from ..ops.jpeg import GEOM_FIELDS, JpegGeometry, decode_pil, probe
from ..pipelines.stream import PinnedSlots, StreamExecutor
from ..ros import msgs

log = logging.getLogger("triton_client_amd.live")


def _threads() -> int:
    return max(1, min(16, os.cpu_count() or 1))


def _buffers(bufs: Sequence) -> Tuple[ctypes.Array, list]:
    """void* array over bytes-like objects (no copy) + the views keeping them alive."""
    views = [np.frombuffer(b, np.uint8) for b in bufs]
    return (ctypes.c_void_p * len(views))(*[v.ctypes.data for v in views]), views


def gather_copy(dst_ptrs: Sequence[int], srcs: Sequence, sizes: Sequence[int], threads: int) -> None:
    """dst_ptrs[i] <- srcs[i][:sizes[i]] on C++ threads (GIL released)."""
    n = len(srcs)
    if n == 0:
        return
    sp, keep = _buffers(srcs)
    dp = (ctypes.c_void_p * n)(*dst_ptrs)
    nb = (ctypes.c_int64 * n)(*sizes)
    rc = _native.runtime().tca_host_gather_copy(n, dp, sp, nb, threads)
    del keep
    if rc:
        raise ValueError("tca_host_gather_copy: bad arguments")


# ============================================================================ camera
def _is_compressed(m) -> bool:
    return isinstance(m, msgs.CompressedImage) or (hasattr(m, "format") and not hasattr(m, "encoding"))


class _CameraEngine:
    """One frame geometry + input kind: a calibrated pipeline, its two captured
    graphs and a pool of pinned staging slots."""

    def __init__(self, live: "LiveCamera", kind: str, hw: Tuple[int, int], geo, draw: bool, names: Tuple[str, ...],
                 sample: np.ndarray, compressed=None, rectify=None):
        """geo: the :class:`JpegGeometry` of a ``"jpeg"`` engine, (encoding, step, is_bigendian)
        of a ``"raw"`` one, else None.  compressed: :class:`~triton_client_amd.ops.jpeg_encode.JpegOptions`
        -- the step also encodes the annotated frames, and they leave as ``CompressedImage``.
        rectify: a :class:`~triton_client_amd.ops.rectify.Rectifier` on the detector's GPU -- the
        frames as the sensor sent them land in a buffer of their own (``unrect_dev``), and the last
        step of ``pre`` rectifies them into the pipeline's frame buffer (``tca_rectify``)."""
        det = live.det
        self.live, self.kind, self.hw, self.draw = live, kind, hw, draw
        self.compressed, self.names, self.jenc, self.warned = compressed, names, None, False
        self.rectify = rectify
        raw = geo if kind == "raw" else None
        self.geo = geo = geo if kind == "jpeg" else None
        self.B, dev = det.B, det.device
        H, W = hw
        if raw is not None:
            self.enc, self.step, self.be = raw
            self.raw_bytes = image_frame_bytes(H, W, self.step, self.enc)  # ValueError: a geometry it refuses
            self.raw_stride = (self.raw_bytes + 15) // 16 * 16
        self.p = det._calibrated_pipeline(hw, sample)
        self.names_dev = None
        if draw and names:
            from ..utils.draw import names_table
            self.names_dev = torch.from_numpy(names_table(names)).to(dev)
        inputs = [(self.p, "frames")]
        if compressed is not None:  # the files and their lengths are per set, like the frames they replace
            from ..ops.jpeg_encode import JpegBatchEncoder
            self.jenc = JpegBatchEncoder(self.B, hw, dev, compressed.quality, compressed.subsampling,
                                         compressed.restart, compressed.cap)
            self.jfiles, self.jlens = self.jenc.buffers()
            inputs += [(self, "jfiles"), (self, "jlens")]
        self.ex = StreamExecutor(self._step, inputs, dev, graph=det.graph)
        if rectify is not None:  # per set, like the frames they become
            self.unrect_dev = [torch.empty((self.B, H, W, 3), dtype=torch.uint8, device=dev)
                               for _ in range(self.ex.sets)]
        if raw is not None:
            self.raw_dev = [torch.empty((self.B, self.raw_stride), dtype=torch.uint8, device=dev)
                            for _ in range(self.ex.sets)]
        if geo is not None:
            self.geom_rec = np.array([geo.width, geo.height, geo.nc, geo.hmax, geo.vmax, geo.mcux, geo.mcuy,
                                      *[v for hv in geo.sampling for v in hv], geo.nblocks, 0, 0], np.int32)
            self.coef_dev = [torch.empty((self.B, geo.nblocks, 64), dtype=torch.int16, device=dev)
                             for _ in range(self.ex.sets)]
            self.q_dev = [torch.empty((self.B, 192), dtype=torch.float32, device=dev) for _ in range(self.ex.sets)]
            self.planes = torch.empty((self.B, geo.plane_bytes), dtype=torch.uint8, device=dev)

        def make_slot():
            if raw is not None:  # the payloads as the sensor sent them
                return SimpleNamespace(raw=torch.empty((self.B, self.raw_stride), dtype=torch.uint8).pin_memory())
            s = SimpleNamespace(frames=torch.empty((self.B, H, W, 3), dtype=torch.uint8).pin_memory())
            s.frames_np = s.frames.numpy()
            if geo is not None:
                s.coef = torch.empty((self.B, geo.nblocks, 64), dtype=torch.int16).pin_memory()
                s.q = torch.empty((self.B, 192), dtype=torch.float32).pin_memory()
                s.geoms = np.zeros((self.B, GEOM_FIELDS), np.int32)
                s.status = np.zeros((self.B,), np.int32)
            return s
        self.slots = PinnedSlots(live.slots, make_slot)

    def _step(self):
        """Capture-safe: the pipeline step, then boxes + labels onto the frames."""
        res = self.p.step()
        if self.draw:
            from ..ops.image import draw_annotations_
            draw_annotations_(self.p.frames, res.box, res.score, res.cls, res.count, self.names_dev,
                              thickness=self.live.thickness)
        if self.jenc is not None:
            # all B frames, whatever the batch holds: the captured step's grids are fixed
            self.jenc.encode_(self.p.frames, self.jfiles, self.jlens, stream=torch.cuda.current_stream())
        return res

    def _sensor_frames(self, k: int) -> torch.Tensor:
        """Where set k's frames land as the sensor sent them: the pipeline's frame buffer, or with
        ``rectify`` the buffer :meth:`_rectify` reads."""
        return self.ex.inputs[k][0] if self.rectify is None else self.unrect_dev[k]

    def _rectify(self, k: int, n: int) -> None:
        """The last step of ``pre``: set k's first n sensor frames, rectified, into the pipeline's
        frame buffer."""
        if self.rectify is not None:
            self.rectify.rectify_(self.unrect_dev[k], self.ex.inputs[k][0], n, torch.cuda.current_stream())

    # ------------------------------------------------------------------ host staging
    def _stage_jpeg(self, s, datas: List) -> List[int]:
        n, g = len(datas), self.geo
        ptrs, keep = _buffers(datas)
        lens = (ctypes.c_int64 * n)(*[len(v) for v in keep])
        failed = _native.runtime().tca_jpeg_decode_batch(
            ptrs, lens, n, s.coef.data_ptr(), g.nblocks, s.q.data_ptr(), s.geoms.ctypes.data, s.status.ctypes.data,
            self.live.threads)
        fb = []
        for i in range(n):
            if (failed and s.status[i]) or not np.array_equal(s.geoms[i], self.geom_rec):
                s.frames_np[i] = self.live.host_rgb(datas[i], self.hw)
                fb.append(i)
        return fb

    def _stage_frames(self, s, batch: Sequence) -> None:
        H, W = self.hw
        direct, srcs = [], []
        for i, m in enumerate(batch):
            if (not _is_compressed(m) and m.encoding == "rgb8" and m.step == 3 * W
                    and len(m.data) >= H * W * 3):
                direct.append(i)
                srcs.append(m.data)
            else:
                s.frames_np[i] = self.live.host_rgb(m, self.hw)
        frame = H * W * 3
        gather_copy([s.frames.data_ptr() + i * frame for i in direct], srcs, [frame] * len(direct),
                    self.live.threads)

    def _stage_raw(self, s, batch: Sequence) -> None:
        gather_copy([s.raw.data_ptr() + i * self.raw_stride for i in range(len(batch))], [m.data for m in batch],
                    [self.raw_bytes] * len(batch), self.live.threads)

    # ------------------------------------------------------------------ one batch
    def submit(self, batch: Sequence, out_frames: Optional[Sequence[torch.Tensor]] = None):
        """Stage ``batch`` (<= B messages of this engine's kind and geometry) and
        enqueue its device work; returns the pending batch for :meth:`finish`.
        ``out_frames``: page-locked [H, W, 3] host tensors (one per message) the
        annotated frames are copied into instead of a fresh pinned buffer."""
        n = len(batch)
        if not 0 < n <= self.B:
            raise ValueError(f"{n} frames for a batch of {self.B}")
        if self.kind == "raw":
            for m in batch:  # a short payload: the host path's ValueError, before anything is staged
                if len(m.data) < self.raw_bytes:
                    self.live.host_rgb(m, self.hw)
                    raise ValueError(f"{self.enc!r} image: {len(m.data)} B of data, {self.raw_bytes} B needed")
        s = self.slots.acquire()
        ticket = None
        try:
            fb: List[int] = []
            if self.kind == "jpeg":
                fb = self._stage_jpeg(s, [m.data for m in batch])
            elif self.kind == "raw":
                self._stage_raw(s, batch)
            else:
                self._stage_frames(s, batch)
            if self.kind == "raw":
                def copies(k):
                    return [(self.raw_dev[k], s.raw[:n])]

                def pre(k):
                    H, W = self.hw
                    image_to_rgb8(self.raw_dev[k], H, W, self.step, self.enc, self.be, out=self._sensor_frames(k), n=n,
                                  stream=torch.cuda.current_stream())
                    self._rectify(k, n)
            elif self.kind == "jpeg":
                def copies(k):
                    return [(self.coef_dev[k], s.coef[:n]), (self.q_dev[k], s.q[:n])]

                def pre(k):
                    g, st = self.geo, _native.stream_ptr(torch.cuda.current_stream())
                    out = self._sensor_frames(k)
                    _native.call("tca_jpeg_idct", self.coef_dev[k].data_ptr(), self.q_dev[k].data_ptr(),
                                 self.planes.data_ptr(), self.geom_rec.ctypes.data, g.nblocks, g.plane_bytes, n, st)
                    _native.call("tca_jpeg_color", self.planes.data_ptr(), out.data_ptr(), self.geom_rec.ctypes.data,
                                 g.plane_bytes, g.height * g.width * 3, n, st)
                    for i in fb:  # frames the entropy decoder handed to the host decoder
                        out[i].copy_(s.frames[i], non_blocking=True)
                    self._rectify(k, n)
            else:
                def copies(k):
                    return [(self._sensor_frames(k), s.frames[:n])]
                pre = None if self.rectify is None else (lambda k: self._rectify(k, n))
            if self.jenc is not None:
                if out_frames is not None:
                    raise ValueError("compressed output has no caller-provided frame buffers")
                ticket = self.ex.submit(copies, pre, lambda k: [self.ex.inputs[k][1][:n], self.ex.inputs[k][2][:n]])
            elif out_frames is not None:
                ticket = self.ex.submit(copies, pre, lambda k: [self.ex.inputs[k][0][i] for i in range(n)],
                                        extras_dst=list(out_frames))
            else:
                ticket = self.ex.submit(copies, pre, lambda k: [self.ex.inputs[k][0][:n]])
        finally:
            # the slot is read by the H2D (and the host-decoded frames by pre() on the compute
            # stream): free once the batch's last device work is done
            self.slots.release(s, ticket.done if ticket is not None else None)
        return SimpleNamespace(batch=batch, ticket=ticket, out_frames=out_frames)

    def finish(self, pend) -> List[tuple]:
        """-> [(Image, dets [n, 6])] of a submitted batch (waits for its D2H); with
        compressed output the first of each pair is a ``CompressedImage``."""
        ticket, batch = pend.ticket.wait(), pend.batch
        res = ticket.result()
        cnt = res.count.numpy()
        box, score, cls = res.box.numpy(), res.score.numpy(), res.cls.numpy()
        H, W = self.hw
        if self.jenc is not None:
            files, lens = ticket.extras[0].numpy(), ticket.extras[1].numpy()
        else:
            frames = [f.numpy() for f in ticket.extras] if pend.out_frames is not None else ticket.extras[0].numpy()
        out = []
        for j, m in enumerate(batch):
            c = int(min(cnt[j], box.shape[1]))
            d = np.empty((c, 6), np.float32)
            d[:, :4] = box[j, :c, :4]
            d[:, 4] = score[j, :c]
            d[:, 5] = cls[j, :c]
            if self.jenc is not None:
                from ..ops.jpeg_encode import FORMAT
                if lens[j] > 0:  # zero-copy view of the pinned D2H buffer
                    data = memoryview(files[j, :int(lens[j])])
                else:
                    data = self._host_file(m, d, int(-lens[j]))
                out.append((msgs.CompressedImage(header=m.header, format=FORMAT, data=data), d))
                continue
            im = msgs.Image(header=m.header, height=H, width=W, encoding="rgb8", is_bigendian=0, step=3 * W,
                            data=memoryview(frames[j].reshape(-1)))  # zero-copy view of the pinned D2H buffer
            out.append((im, d))
        return out

    def _host_file(self, m, dets: np.ndarray, needed: int) -> bytes:
        """A frame whose file did not fit the device buffer: decoded, rectified (with ``rectify``),
        drawn and encoded on the host."""
        from ..ops.jpeg_encode import encode_pil
        from ..utils.draw import draw_detections
        if not self.warned:
            self.warned = True
            log.warning("a %dx%d frame needs %d B as JPEG, the device buffer holds %d B per frame: such frames "
                        "are encoded on the host (raise the cap)", self.hw[1], self.hw[0], needed, self.jenc.cap)
        rgb = np.array(self.live.host_rgb(m, self.hw))
        if self.rectify is not None:  # the detections are in rectified pixels: so is the frame
            from ..ops.rectify import rectify_numpy
            rgb = rectify_numpy(np.ascontiguousarray(rgb), self.rectify.map)
        if self.draw:
            draw_detections(rgb, dets, list(self.names) or None, thickness=self.live.thickness)
        return encode_pil(rgb, self.compressed.quality, self.compressed.subsampling)

    def run(self, batch: Sequence) -> List[tuple]:
        return self.finish(self.submit(batch))

    def zero_stage(self) -> List[torch.Tensor]:
        """Result-shaped device zeros (an empty shard's part of a gather)."""
        if getattr(self, "_zero", None) is None:
            self._zero = [torch.zeros_like(t) for t in self.ex.stage[0]]
        return self._zero


class LiveCamera:
    """Camera messages -> (annotated ``Image``, detections [n, 6]) per message,
    for a :class:`~triton_client_amd.inference.engines.LocalDetector2D` on the GPU."""

    def __init__(self, det, slots: int = 4, threads: Optional[int] = None, thickness: int = 2):
        self.det, self.slots, self.thickness = det, slots, thickness
        self.threads = threads or _threads()
        self.engines: Dict[tuple, _CameraEngine] = {}
        self.lock = threading.Lock()

    @staticmethod
    def host_rgb(msg_or_data, hw: Optional[Tuple[int, int]] = None) -> np.ndarray:
        """Host decode for what the device path does not take (progressive JPEG, PNG, JPEGs
        the entropy decoder rejects), for an engine's calibration sample, and, with
        ``TCA_DEVICE_ENCODINGS=0``, for every raw ``Image`` that is not packed rgb8 (bgr8 /
        rgba8 / bgra8, mono8 / mono16, YUV 4:2:2, 8-bit Bayer, padded rows): HxWx3 uint8 RGB.
        ValueError for an ``Image`` encoding ``ops.golden.image_to_rgb8`` does not know."""
        from ..ros import compat
        if isinstance(msg_or_data, (bytes, bytearray, memoryview)):
            try:
                rgb = decode_pil(bytes(msg_or_data))
            except Exception as e:  # noqa: BLE001 - a corrupt frame must not end the stream
                log.warning("undecodable camera frame (%s): publishing it black", e)
                return np.zeros((*hw, 3), np.uint8)
        elif _is_compressed(msg_or_data):
            return LiveCamera.host_rgb(msg_or_data.data, hw)
        else:
            rgb = compat.imgmsg_to_numpy(msg_or_data, "rgb8")
        if hw is not None and rgb.shape[:2] != tuple(hw):
            raise ValueError(f"frame {rgb.shape[1]}x{rgb.shape[0]} in a {hw[1]}x{hw[0]} batch")
        return rgb

    def _key(self, m):
        if _is_compressed(m):
            try:
                geo = probe(m.data if isinstance(m.data, bytes) else bytes(m.data))
            except ValueError:
                geo = None
            if geo is not None and geo.gpu_ok:
                return ("jpeg", (geo.height, geo.width), geo)
            rgb = self.host_rgb(m)
            return ("frames", rgb.shape[:2], None)
        H, W, enc = int(m.height), int(m.width), m.encoding
        # a raw Image the device converts: any known encoding but packed rgb8 (TCA_DEVICE_ENCODINGS=0:
        # the host converts them all, as it does the encodings it alone refuses by name)
        if (enc in golden.IMAGE_ENCODINGS and not (enc == "rgb8" and m.step == 3 * W)
                and os.environ.get("TCA_DEVICE_ENCODINGS", "1") != "0"):
            return ("raw", (H, W), (enc, int(m.step), int(bool(m.is_bigendian)) if enc == "mono16" else 0))
        return ("frames", (H, W), None)

    compressed_out = True  # process() takes compressed= (the drivers ask before passing it)
    rectify_in = True      # ... and rectify=

    def _engine(self, key, draw: bool, names: Tuple[str, ...], sample_msg, compressed=None,
                rectify=None) -> _CameraEngine:
        k = (key, draw, names, compressed, rectify)
        eng = self.engines.get(k)
        if eng is None:
            with self.lock:
                eng = self.engines.get(k)
                if eng is None:
                    kind, hw, geo = key
                    sample = self.host_rgb(sample_msg, hw) if self.det.calibrate_target is not None else None
                    if rectify is not None:
                        want = self.det.device.index  # (None: the current GPU)
                        if rectify.map_dev is None or want not in (None, rectify.map_dev.device.index):
                            raise ValueError(f"rectify: a Rectifier on {self.det.device} (the engine's "
                                             f"rectifier()), got one on {rectify.device}")
                        if sample is not None:  # the detector is calibrated on what it will see
                            from ..ops.rectify import rectify_numpy
                            sample = rectify_numpy(np.ascontiguousarray(sample), rectify.map)
                    eng = self.engines[k] = _CameraEngine(self, kind, hw, geo, draw, names, sample, compressed,
                                                          rectify)
        return eng

    def process(self, messages: Sequence, draw: bool = True, names: Optional[Sequence[str]] = None,
                compressed=None, rectify=None) -> List[tuple]:
        """-> [(Image, dets [n, 6] x1,y1,x2,y2,conf,cls in frame pixels)] in message order.
        compressed: :class:`~triton_client_amd.ops.jpeg_encode.JpegOptions`; the annotated frames are
        encoded on the device and come back as ``CompressedImage`` (JPEG) instead.
        rectify: a :class:`~triton_client_amd.ops.rectify.Rectifier` on the detector's GPU
        (``det.rectifier(model)``); every frame is rectified on the device before the detector sees
        it, and frame and detections come back in rectified pixels.  ValueError for a frame that is
        not of the camera model's size."""
        names = tuple(names or ())
        groups: Dict[tuple, List[int]] = {}
        for i, m in enumerate(messages):
            groups.setdefault(self._key(m), []).append(i)
        out: List[Optional[tuple]] = [None] * len(messages)
        B = self.det.B
        for key in groups:
            if rectify is not None and tuple(key[1]) != rectify.hw:
                raise ValueError(f"rectify: frame {key[1][1]}x{key[1][0]}, the camera model is "
                                 f"{rectify.hw[1]}x{rectify.hw[0]}")
        for key, idx in groups.items():
            eng = self._engine(key, draw, names, messages[idx[0]], compressed, rectify)
            for s in range(0, len(idx), B):
                chunk = idx[s:s + B]
                for i, r in zip(chunk, eng.run([messages[i] for i in chunk])):
                    out[i] = r
        return out


# ============================================================================ LiDAR
class _LidarEngine:
    def __init__(self, live: "LiveLidar", layout, max_points: int, sample):
        det = live.det
        self.live, self.layout = live, layout
        self.B, dev = det.B, det.device
        self.p = det._calibrated_pipeline(layout, max_points, sample)
        self.max_points, self.fb = self.p.max_points, self.p.frame_bytes
        self.ex = StreamExecutor(self.p.step, [(self.p, "data"), (self.p, "frame_n")], dev, graph=det.graph)

        def make_slot():
            s = SimpleNamespace(data=torch.empty((self.B * self.fb,), dtype=torch.uint8).pin_memory(),
                                n=torch.zeros((self.B,), dtype=torch.int32).pin_memory())
            s.n_np = s.n.numpy()
            return s
        self.slots = PinnedSlots(live.slots, make_slot)

    def submit(self, clouds: Sequence[msgs.PointCloud2]):
        n, fb, step = len(clouds), self.fb, self.layout.point_step
        if not 0 < n <= self.B:
            raise ValueError(f"{n} clouds for a batch of {self.B}")
        counts = [int(c.width * c.height) for c in clouds]
        sizes = [k * step for k in counts]
        for c, sz in zip(clouds, sizes):
            if len(c.data) < sz or sz > fb:
                raise ValueError(f"PointCloud2 of {c.width}x{c.height} points x {step} B has {len(c.data)} B of data "
                                 f"(slot {fb} B)")
        s = self.slots.acquire()
        ticket = None
        try:
            gather_copy([s.data.data_ptr() + j * fb for j in range(n)], [c.data for c in clouds], sizes,
                        self.live.threads)
            s.n_np[:] = 0
            s.n_np[:n] = counts

            def copies(k):
                d, nd = self.ex.inputs[k]
                return [(d[j * fb:j * fb + sz], s.data[j * fb:j * fb + sz]) for j, sz in enumerate(sizes) if sz] + \
                    [(nd, s.n)]
            ticket = self.ex.submit(copies)
        finally:
            self.slots.release(s, ticket.uploaded if ticket is not None else None)
        return SimpleNamespace(n=n, ticket=ticket)

    def finish(self, pend) -> List[dict]:
        return self.live.det._frames_out(pend.ticket.wait().result())[:pend.n]

    def run(self, clouds: Sequence[msgs.PointCloud2]) -> List[dict]:
        return self.finish(self.submit(clouds))

    def zero_stage(self) -> List[torch.Tensor]:
        if getattr(self, "_zero", None) is None:
            self._zero = [torch.zeros_like(t) for t in self.ex.stage[0]]
        return self._zero


class LiveLidar:
    """PointCloud2 messages -> per-cloud {pred_boxes, pred_scores, pred_labels}
    (sensor frame) for a :class:`~triton_client_amd.inference.engines.LocalDetector3D`
    on the GPU."""

    def __init__(self, det, slots: int = 4, threads: Optional[int] = None):
        self.det, self.slots = det, slots
        self.threads = threads or _threads()
        self.engines: Dict[tuple, _LidarEngine] = {}
        self.lock = threading.Lock()

    def _engine(self, layout, npts: int, sample) -> _LidarEngine:
        key = (layout.point_step, layout.offsets, layout.dtypes)
        eng = self.engines.get(key)
        if eng is None or eng.max_points < npts:
            with self.lock:
                eng = self.engines.get(key)
                if eng is None or eng.max_points < npts:
                    maxp = self.det.max_points
                    while maxp < npts:
                        maxp *= 2
                    eng = self.engines[key] = _LidarEngine(self, layout, maxp, sample)
        return eng

    def process(self, clouds: Sequence[msgs.PointCloud2]) -> List[dict]:
        from ..ros.compat import cloud_layout

        groups: Dict[tuple, List[int]] = {}
        lays = {}
        for i, c in enumerate(clouds):
            lay = cloud_layout(c)
            k = (lay.point_step, lay.offsets, lay.dtypes)
            lays[k] = lay
            groups.setdefault(k, []).append(i)
        out: List[Optional[dict]] = [None] * len(clouds)
        B = self.det.B
        for k, idx in groups.items():
            npts = max(clouds[i].width * clouds[i].height for i in idx)
            eng = self._engine(lays[k], npts, clouds[idx[0]])
            for s in range(0, len(idx), B):
                chunk = idx[s:s + B]
                for i, r in zip(chunk, eng.run([clouds[i] for i in chunk])):
                    out[i] = r
        return out
