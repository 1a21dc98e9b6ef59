"""Live 2D inference driver (reference ``communicator/ros_inference.py:25-175``).

Subscribes to the camera topic (``CompressedImage`` JPEG or raw ``Image``,
SURVEY Appendix A3), runs the engine (local MI355X pipeline or remote KServe
server), draws the boxes and publishes an annotated ``Image`` (rgb8) carrying
the *input* header (A4) — plus a ``vision_msgs/Detection2DArray`` on
``<pub_topic>/detections`` (the intent of ``utils/pred2ros_msg.py:21-52``).
An empty detection set still publishes the frame (fixes A5).

``batch > 1`` (or ``workers > 1``): the callback only enqueues; frames are
run as micro-batches (one engine call — one graph replay, or one DP scatter
over the node's GPUs — per batch) from a latest-wins window, and results are
re-published in ``header.seq`` order (:mod:`.batching`).

``compressed=JpegOptions(...)``: the annotated frame is published as a
``CompressedImage`` (JPEG) on ``<pub_topic>/compressed`` *instead of* the raw
``Image`` -- about a thirteenth of the bytes.  The local GPU engine encodes on the
device inside its captured step (``ops/jpeg_encode.py``); every other engine encodes
the annotated array with PIL on the host.  The data-parallel ring engines refuse it.

``rectify=CameraModel`` (or the path of a ``camera_calibration`` YAML): every frame is
rectified from the camera's calibration (``ops/rectify.py``) between decode and detector, so
the annotated frame is the rectified frame and the detections and tracks messages are in
rectified pixels, the image the calibration's ``projection_matrix`` describes (give that
matrix to the LiDAR driver's ``--calib`` as ``projection``).  The local GPU engine rectifies
on the device (``tca_rectify``, the last step before its captured one); every other engine,
and ``TCA_DEVICE_RECTIFY=0``, through the engine's ``rectifier(model).frames``.  Headers are
unchanged; a frame that is not of the model's size is a ``ValueError``.  The data-parallel
ring engines refuse it.

``tracks_topic``: also publish, per frame and with the frame's header, one more
``Detection2DArray`` with the same detections in the same order whose ``results[0].id``
holds the detection's track id instead of its class (the convention of the 3D tracks
message; id 0: not tracked).  The tracker (``ops/track2d.py``: ByteTrack's association
on the IoU of predicted boxes, ``tca_track2d`` on an engine's GPU) sees the frames in
published order: :meth:`RosInference.track` is the ordered stage of the micro-batched
driver, and a frame the re-publisher drops never reaches it.  The annotated frame and
the detections message are the same bytes with the option on or off; track ids are
not drawn on the frame (the drawing happens in the engine's step, before the ordered
stage).
"""
from __future__ import annotations

import time
from typing import List, Optional, Sequence

import numpy as np

from ..ros import compat, msgs
from ..utils.draw import draw_detections
from ..utils.metrics import StageTimer
from .base_inference import BaseInference
from .engines import Detector2D, RemoteDetector2D


def decode_image_msg(msg) -> np.ndarray:
    """CompressedImage (jpeg/png) or Image → HxWx3 uint8 RGB (reference :119-133)."""
    if isinstance(msg, msgs.CompressedImage) or (hasattr(msg, "format") and not hasattr(msg, "encoding")):
        if "compressed" in msg.format or msg.format.lower() in ("jpeg", "jpg", "png"):
            return compat.jpeg_decode_rgb(msg.data)
    return compat.imgmsg_to_numpy(msg, "rgb8")


def detections_to_msg(dets: np.ndarray, header: msgs.Header, source: Optional[msgs.Image] = None,
                      ids=None) -> msgs.Detection2DArray:
    """Detection2DArray over dets [n, 6]; the Detection2D objects are built only
    if a subscriber reads ``detections`` (:class:`~triton_client_amd.ros.msgs.ArrayList`,
    columns ``{"dets": dets}``).  ``ids`` [n]: these values instead of the classes in
    ``results[0].id`` (the tracks message's ids; one more column ``"ids"``)."""
    dets = np.asarray(dets, np.float32).reshape(-1, 6)
    cols = {"dets": dets}
    if ids is not None:
        cols["ids"] = ids = np.asarray(ids, np.int32).reshape(-1)

    def build():
        src = msgs.Image(header=header) if source is None else source
        out = []
        for k, (x1, y1, x2, y2, conf, c) in enumerate(dets.tolist()):
            out.append(msgs.Detection2D(
                header=header, results=[msgs.ObjectHypothesisWithPose(id=int(c if ids is None else ids[k]),
                                                                      score=conf)],
                bbox=msgs.BoundingBox2D(center=msgs.Pose2D((x1 + x2) / 2, (y1 + y2) / 2, 0.0), size_x=x2 - x1,
                                        size_y=y2 - y1),
                source_img=src))
        return out
    return msgs.Detection2DArray(header=header, detections=msgs.ArrayList(len(dets), build, cols))


class RosInference(BaseInference):
    def __init__(self, channel=None, client=None, engine: Optional[Detector2D] = None, params: Optional[dict] = None,
                 bus=None, letterbox: bool = False, conf_thres: float = 0.3, draw: bool = True,
                 publish_detections: bool = True, queue_size: Optional[int] = 1, metrics=None, mode: str = "sync",
                 wire: str = "raw", batch: int = 1, workers: int = 1, compressed=None,
                 tracks_topic: Optional[str] = None, track_options: Optional[dict] = None, rectify=None):
        super().__init__(channel, client)
        if compressed is not None and not getattr(engine, "compressed_out", True):
            raise ValueError(f"{type(engine).__name__} does not publish compressed frames: the data-parallel ring "
                             "engines move raw frames between ranks; run without --publish-compressed")
        if rectify is not None and not getattr(engine, "compressed_out", True):
            raise ValueError(f"{type(engine).__name__} does not rectify frames: the data-parallel ring engines "
                             "move the sensor's frames between ranks; run without --rectify")
        self.compressed = compressed
        if rectify is not None:
            from ..ops.rectify import as_camera_model
            rectify = as_camera_model(rectify)
        self.rectify = rectify
        self._params = params or {}
        self.engine = engine or RemoteDetector2D(channel, client, letterbox=letterbox, conf_thres=conf_thres,
                                                 mode=mode, wire=wire)
        self.class_names = list(getattr(self.engine, "names", []) or [])
        self.bus, self.draw, self.publish_detections = bus, draw, publish_detections
        self.queue_size, self.metrics = queue_size, metrics
        self.frames = 0
        self.sub = self.pub = self.det_pub = None
        self.tracks_topic, self.tracks_pub = tracks_topic or None, None
        self.track_options = dict(track_options or {})
        self.batch, self.workers = max(1, batch), max(1, workers)
        self.runner = None
        if self.rectify is not None:
            self.rectifier()  # made here, once, before any worker asks for it

    # ------------------------------------------------------------------ run
    def start_inference(self, spin: bool = True, timeout: Optional[float] = None):
        p = self.params
        if self.compressed is not None:  # instead of the raw Image, not beside it
            self.pub = compat.Publisher(p["pub_topic"] + "/compressed", msgs.CompressedImage, queue_size=10,
                                        bus=self.bus)
        else:
            self.pub = compat.Publisher(p["pub_topic"], msgs.Image, queue_size=10, bus=self.bus)
        if self.publish_detections:
            self.det_pub = compat.Publisher(p["pub_topic"] + "/detections", msgs.Detection2DArray, queue_size=10,
                                            bus=self.bus)
        if self.tracks_topic:
            self.tracks_pub = compat.Publisher(self.tracks_topic, msgs.Detection2DArray, queue_size=10, bus=self.bus)
        cb, qs = self._callback, self.queue_size
        if self.batch > 1 or self.workers > 1:
            from .batching import MicroBatchRunner
            cap = max(self.queue_size or 0, 2 * self.batch * self.workers)
            if self.tracks_topic:  # the workers hand over whole results; the ordered stage tracks them
                self.runner = MicroBatchRunner(self.process, lambda r: self._publish((r[0], r[1], r[3])),
                                               batch=self.batch, workers=self.workers, capacity=cap,
                                               ordered_fn=self.track)
            else:
                self.runner = MicroBatchRunner(lambda ms: [(im, det) for im, det, _ in self.process(ms)],
                                               self._publish, batch=self.batch, workers=self.workers, capacity=cap)
            cb, qs = self.runner.push, None  # the window is the (latest-wins) queue
        self.sub = compat.Subscriber(p["sub_topic"], msgs.CompressedImage, cb, queue_size=qs, bus=self.bus,
                                     ingest=getattr(self.engine, "ingest_buffer", None))
        if spin:
            compat.spin(self.bus, timeout)

    def stop(self, drain: bool = True):
        if self.sub is not None:
            self.sub.unregister()
            self.sub = None
        if self.runner is not None:
            self.runner.close(drain=drain)
            self.runner = None

    def _publish(self, item) -> None:
        """item: (frame, detections message[, tracks message])."""
        im, det = item[0], item[1]
        self.pub.publish(im)
        if self.det_pub is not None:
            self.det_pub.publish(det)
        if len(item) > 2 and self.tracks_pub is not None:
            self.tracks_pub.publish(item[2])

    # ------------------------------------------------------------------ work
    def _live(self):
        """The engine's streaming device path (LocalDetector2D on a GPU), else None."""
        if not hasattr(self, "_live_exec"):
            fn = getattr(self.engine, "live", None)
            self._live_exec = fn() if callable(fn) else None
        return self._live_exec

    @property
    def out_topic(self) -> str:
        """Where the annotated frame goes."""
        return self.params["pub_topic"] + ("/compressed" if self.compressed is not None else "")

    def _compress(self, im) -> msgs.CompressedImage:
        """An annotated rgb8 ``Image`` -> JPEG ``CompressedImage`` on the host (PIL)."""
        from ..ops.jpeg_encode import FORMAT, encode_pil
        c = self.compressed
        return msgs.CompressedImage(header=im.header, format=FORMAT,
                                    data=encode_pil(compat.imgmsg_to_numpy(im, "rgb8"), c.quality, c.subsampling))

    def process(self, images: Sequence) -> List[tuple]:
        """Messages → [(annotated Image msg, Detection2DArray, dets [n,6])]; with ``compressed`` the
        first of each triple is a JPEG ``CompressedImage``."""
        t0 = time.perf_counter()
        timer = StageTimer(self.metrics)
        live = self._live()
        if live is not None:  # device path: GPU decode, graph step, GPU annotation, zero-copy Image
            kw = {}
            if self.rectify is not None:
                rec = self.rectifier()
                if getattr(live, "rectify_in", False) and rec.gpu:
                    kw["rectify"] = rec  # rectified on the device, between decode and detector
                else:  # a device path without the step (the remote client's), or TCA_DEVICE_RECTIFY=0
                    with timer("rectify"):
                        rgb = rec.frames([decode_image_msg(m) for m in images])
                        images = [compat.numpy_to_imgmsg(f, "rgb8", header=m.header) for m, f in zip(images, rgb)]
            with timer("device"):
                if self.compressed is not None and getattr(live, "compressed_out", False):
                    res = live.process(images, draw=self.draw, names=self.class_names, compressed=self.compressed,
                                       **kw)
                else:
                    res = live.process(images, draw=self.draw, names=self.class_names, **kw)
                    if self.compressed is not None:  # a device path without the encoder (the remote client's)
                        res = [(self._compress(im), d) for im, d in res]
            with timer("messages"):
                out = [(im, detections_to_msg(d, m.header), d) for m, (im, d) in zip(images, res)]
            self.frames += len(images)
            if self.metrics is not None:
                self.metrics.stage("frame", (time.perf_counter() - t0) / max(len(images), 1))
                self.metrics.frame(len(images))
            return out
        with timer("decode"):
            rgb = [decode_image_msg(m) for m in images]
        if self.rectify is not None:
            with timer("rectify"):
                rgb = self.rectifier().frames(rgb)
        gpu_draw = self.draw and hasattr(self.engine, "detect_annotated") and \
            getattr(getattr(self.engine, "device", None), "type", "cpu") == "cuda"
        with timer("detect"):
            if gpu_draw:  # rectangles drawn on the GPU (K15), labels below
                dets, drawn = self.engine.detect_annotated(rgb)
            else:
                dets, drawn = self.engine.detect(rgb), None
        out = []
        with timer("draw_publish"):
            for j, (m, img, d) in enumerate(zip(images, rgb, dets)):
                if drawn is not None:
                    img = draw_detections(drawn[j], d, self.class_names, rects=False)
                elif self.draw:
                    img = draw_detections(img.copy(), d, self.class_names)
                im = compat.numpy_to_imgmsg(img, "rgb8", header=m.header)
                if self.compressed is not None:
                    im = self._compress(im)
                out.append((im, detections_to_msg(d, m.header), d))
        self.frames += len(images)
        if self.metrics is not None:
            self.metrics.stage("frame", (time.perf_counter() - t0) / max(len(images), 1))
            self.metrics.frame(len(images))
        return out

    def tracker(self):
        """The engine's tracker, made with ``track_options`` on first use."""
        fn = getattr(self.engine, "tracker", None)  # (an engine that is no Detector2D subclass)
        return fn(**self.track_options) if fn is not None else Detector2D.tracker(self.engine, **self.track_options)

    def rectifier(self):
        """The engine's :class:`~triton_client_amd.ops.rectify.Rectifier` of the ``rectify`` model."""
        fn = getattr(self.engine, "rectifier", None)  # (an engine that is no Detector2D subclass)
        return fn(self.rectify) if fn is not None else Detector2D.rectifier(self.engine, self.rectify)

    def track(self, results: Sequence[tuple]) -> List[tuple]:
        """The ordered stage: ``process`` results of consecutive frames, in published order →
        each as ``(frame, detections message, dets [n, 6], tracks message, (track_id [n], hits
        [n], vel [n, 2]))``, aligned with the frame's detections.  One tracker call per batch."""
        results = list(results)
        if not results:
            return []
        timer = StageTimer(self.metrics)
        with timer("track2d"):
            res = self.tracker().track([r[2] for r in results], [r[1].header.stamp for r in results])
            return [(r[0], r[1], r[2], detections_to_msg(r[2], r[1].header, ids=t[0]), t) for r, t in zip(results, res)]

    def _callback(self, msg):
        res = self.process([msg])
        if self.tracks_topic:
            for r in self.track(res):
                self._publish((r[0], r[1], r[3]))
            return
        for im, det, _ in res:
            self.pub.publish(im)
            if self.det_pub is not None:
                self.det_pub.publish(det)
