"""Live 3D inference driver (reference ``communicator/ros_inference3d.py:44-213``).

PointCloud2 in → boxes out as a jsk ``BoundingBoxArray`` (default) or a
``vision_msgs/Detection3DArray``, header stamp/frame_id copied from the
cloud.  Reference behaviours kept as configurable defaults:
z offset +1.5 before voxelising (removed from the output boxes), intensity
normalised by its max, only label 2 (Pedestrian) with score > 0.5 published,
jsk dimensions swapped (x = dy, y = dx).  Fixed: the Detection3DArray yaw is
taken from the box's own dimension (index 6 for 7-d boxes, 8 for 9-d; A8).

``bev_topic``: also publish, per cloud and with the cloud's header, an rgb8
``Image`` of the frame from above — points grey by height, every detection the
engine returned (whatever ``labels`` / ``score_thresh`` keep in the box
message) as a labelled box.  ``utils/bev.py`` defines the picture; an engine
with a GPU paints the same bytes with ``tca_bev_render`` (``ops/bev.py``;
``TCA_DEVICE_BEV=0``: the host painter).

``points_topic``: also publish, per cloud, the cloud itself with its labels — a
``PointCloud2`` with the cloud's header, height, width and is_dense, every point
in input order as a 28-byte record (x, y, z, intensity as sent; ``label`` int32:
the owner's class, 0 for background; ``instance`` int32: the owner's position in
the ``boxes`` / ``detections`` array of the box message of the same cloud, -1 for
none; ``score`` float32, 0 for none).  The owner of a point is the published box
with the highest score that contains it (``ops/points_in_boxes.py``).

``tracks_topic``: also publish, per cloud and with the cloud's header, a message of
the box message's type with the same boxes in the same order whose class field
(``label``, or ``results[0].id``) holds the box's track id instead — the convention
rviz's jsk display colours by; id 0: not tracked.  The tracker (``ops/track3d.py``:
greedy closest-centre matching on velocity-compensated positions, ``tca_track3d`` on
an engine's GPU) sees the clouds in published order: :meth:`RosInference3D.track` is
the ordered stage of the micro-batched driver, and a cloud the re-publisher drops
never reaches it.  The box message is the same bytes with the option on or off.

``ranged_topic`` (with ``camera_detections_topic`` and ``calibration``): the driver also
subscribes a camera's ``Detection2DArray`` topic into a ``StampPairer`` and, per batch,
pairs every cloud with the held camera message nearest in time within ``range_slop``
seconds (default 0.05) and ranges them in one call (``ops/range2d.py``: ``tca_range2d``
on an engine's GPU).  A cloud that found a partner publishes one ``Detection2DArray``
with the camera message's header and its detections in order, bbox and hypotheses kept,
``results[0].pose.position`` the camera-frame position of the points the shrunken box
sees; a detection without a range keeps a zero position (``z = 0`` is no ranged value:
only points at least ``min_depth`` ahead count), one without a hypothesis gets one with
id 0 and score 0.  Live pairing is best effort: a camera message that arrives after its
cloud was processed is missed (bag replay reads the camera topic first and misses none).
The message rides in the prediction as ``pred["ranged"]``; every other message keeps its
bytes, and with the option off nothing changes.

``depth_topic`` (with ``calibration`` — the one ranging uses — and ``depth_options``, a
``DepthOptions`` or a dict of its fields): the driver also publishes, per cloud, the cloud seen
from the camera (``ops/depth_image.py``: ``tca_depth_image`` on an engine's GPU): an ``Image``
of ``depth_options.encoding`` (REP 118 ``16UC1``, or ``32FC1``) registered to the camera's
pixels, with the cloud's stamp and seq, in frame ``depth_frame_id`` (the cloud's when empty).
It is published after the box message of the same cloud, in published order, and rides in the
prediction as ``pred["depth"]``; every other message keeps its bytes.

``scan_topic`` (with ``scan_options``, a ``ScanOptions`` or a dict of its fields —
``pointcloud_to_laserscan``'s parameters): the driver also publishes, per cloud, a
``sensor_msgs/LaserScan`` for 2D navigation (``ops/laser_scan.py``: ``tca_laser_scan`` on an
engine's GPU): per angular bin the nearest return in the height band, with the cloud's stamp and
seq, in frame ``scan_frame_id`` (the cloud's when empty).  No calibration is involved.  It is
published last of the cloud's messages and rides in the prediction as ``pred["scan"]``; every
other message keeps its bytes.

Whatever is on, one cloud makes one :class:`CloudResult`: the box message, the prediction and
one field per option above, None where the option is off (or, for ``ranged``, where the cloud
found no partner).  :data:`ALL_OUTPUTS` names those fields in the order they are published in,
after the box message: :data:`OUTPUTS` (the perception and visualisation outputs of
:data:`SIDE_OUTPUTS`, then the navigation outputs of :data:`NAV_OUTPUTS`), then the split clouds of
:data:`CLOUD_OUTPUTS`.
"""
from __future__ import annotations

import dataclasses
import time
from typing import List, Optional, Sequence

import numpy as np

from ..ros import compat, msgs
from ..utils.metrics import StageTimer
from .base_inference import BaseInference
from .engines import Detector3D, RemoteDetector3D


def select_boxes(pred: dict, labels: Optional[Sequence[int]] = (2,), score_thresh: float = 0.5) -> np.ndarray:
    """Indices kept for publishing (reference :156 keeps label==2 & score>0.5)."""
    s, l_ = pred["pred_scores"], pred["pred_labels"]
    keep = s > score_thresh
    if labels is not None:
        keep &= np.isin(l_, np.asarray(labels))
    return np.nonzero(keep)[0]


def jsk_columns(pred: dict, idx, label=None) -> dict:
    """The published fields of the selected boxes as columns (float64 like the
    message): position [n, 3], orientation [n, 4] (yaw about +z, reference
    ``yaw2quaternion`` :117-118), dimensions [n, 3] with the reference's x/y
    swap (:169-171), value [n] fp32, label [n] uint32 (``label``: these values instead
    of the classes, aligned with ``idx``: the tracks message's ids)."""
    idx = np.asarray(idx, np.int64)
    b = np.asarray(pred["pred_boxes"])[idx].astype(np.float64)
    yaw = b[:, 8 if b.shape[-1] >= 9 else 6] if len(b) else np.zeros((0,))
    quat = np.zeros((len(b), 4))
    quat[:, 2], quat[:, 3] = np.sin(yaw / 2), np.cos(yaw / 2)
    return {"position": b[:, :3], "orientation": quat, "dimensions": b[:, [4, 3, 5]] if len(b) else np.zeros((0, 3)),
            "value": np.asarray(pred["pred_scores"])[idx].astype(np.float32),
            "label": (np.asarray(pred["pred_labels"])[idx] if label is None else np.asarray(label)).astype(np.uint32)}


def boxes_to_jsk(pred: dict, idx, header: msgs.Header, label=None) -> msgs.BoundingBoxArray:
    """jsk BoundingBoxArray of the selected boxes, built from columns: the
    BoundingBox objects are made only if a subscriber reads ``boxes``
    (:class:`~triton_client_amd.ros.msgs.ArrayList`); serialisation packs the
    columns directly (``ros.rosmsg``)."""
    cols = jsk_columns(pred, idx, label)

    def build():
        P, Q, D = cols["position"].tolist(), cols["orientation"].tolist(), cols["dimensions"].tolist()
        V, L = cols["value"].tolist(), cols["label"].tolist()
        return [msgs.BoundingBox(header=header, pose=msgs.Pose(msgs.Point(*p), msgs.Quaternion(*q)),
                                 dimensions=msgs.Vector3(*d), value=v, label=lb)
                for p, q, d, v, lb in zip(P, Q, D, V, L)]
    return msgs.BoundingBoxArray(header=header, boxes=msgs.ArrayList(len(cols["value"]), build, cols))


def boxes_to_detection3d(pred: dict, idx, header: msgs.Header, ids=None) -> msgs.Detection3DArray:
    """``ids``: these values instead of the classes in ``results[0].id``, aligned with ``idx``."""
    arr = msgs.Detection3DArray(header=header)
    b = pred["pred_boxes"]
    yaw_i = 8 if b.shape[-1] >= 9 else 6
    for k, i in enumerate(idx):
        x = b[i]
        arr.detections.append(msgs.Detection3D(
            header=header,
            results=[msgs.ObjectHypothesisWithPose(id=int(pred["pred_labels"][i] if ids is None else ids[k]),
                                                   score=float(pred["pred_scores"][i]))],
            bbox=msgs.BoundingBox3D(
                center=msgs.Pose(msgs.Point(float(x[0]), float(x[1]), float(x[2])),
                                 compat.yaw2quaternion(float(x[yaw_i]))),
                size=msgs.Vector3(float(x[3]), float(x[4]), float(x[5])))))
    return arr


@dataclasses.dataclass
class CloudResult:
    """What the driver made of one cloud.  ``ranged``, ``depth``, ``scan``, ``obstacles`` and
    ``ground`` are the objects that also ride in ``pred`` under those keys."""
    boxes: object  # BoundingBoxArray, or Detection3DArray
    pred: dict
    bev: Optional[msgs.Image] = None
    points: Optional[msgs.PointCloud2] = None
    tracks: object = None  # a message of the box message's type
    ranged: Optional[msgs.Detection2DArray] = None
    depth: Optional[msgs.Image] = None
    scan: Optional[msgs.LaserScan] = None
    obstacles: Optional[msgs.PointCloud2] = None
    ground: Optional[msgs.PointCloud2] = None


# The side outputs in publishing order: (CloudResult field, message type; None: the box message's).
# The driver's ``<name>_topic`` attribute holds the topic, None when the option is off.
SIDE_OUTPUTS = (("bev", msgs.Image), ("points", msgs.PointCloud2), ("tracks", None),
                ("ranged", msgs.Detection2DArray), ("depth", msgs.Image))
# What feeds 2D navigation rather than perception: published after the side outputs.
NAV_OUTPUTS = (("scan", msgs.LaserScan),)
OUTPUTS = SIDE_OUTPUTS + NAV_OUTPUTS
# The cloud split at its estimated ground: published after everything else.
CLOUD_OUTPUTS = (("obstacles", msgs.PointCloud2), ("ground", msgs.PointCloud2))
ALL_OUTPUTS = OUTPUTS + CLOUD_OUTPUTS  # what the publishers, ``_publish`` and the bag writer loop over


class RosInference3D(BaseInference):
    def __init__(self, channel=None, client=None, engine: Optional[Detector3D] = None, params: Optional[dict] = None,
                 bus=None, jsk: bool = True, labels: Optional[Sequence[int]] = (2,), score_thresh: float = 0.5,
                 z_offset: float = 1.5, queue_size: Optional[int] = 50, metrics=None, mode: str = "sync",
                 wire: str = "raw", batch: int = 1, workers: int = 1, bev_topic: Optional[str] = None,
                 bev_view=None, points_topic: Optional[str] = None, tracks_topic: Optional[str] = None,
                 track_options: Optional[dict] = None, ranged_topic: Optional[str] = None,
                 camera_detections_topic: Optional[str] = None, calibration=None,
                 range_options: Optional[dict] = None, range_slop: float = 0.05, depth_topic: Optional[str] = None,
                 depth_options=None, depth_frame_id: str = "", scan_topic: Optional[str] = None,
                 scan_options=None, scan_frame_id: str = "", obstacles_topic: Optional[str] = None,
                 ground_topic: Optional[str] = None, ground_options=None):
        super().__init__(channel, client)
        self._params = params or {}
        self.engine = engine or RemoteDetector3D(channel, client, z_offset=z_offset, mode=mode, wire=wire)
        self.bev_topic, self.bev_view = None, None
        if bev_topic:
            self.enable_bev(bev_topic, bev_view)
        self.points_topic, self.tracks_topic = points_topic or None, tracks_topic or None
        self.track_options = dict(track_options or {})
        self.ranged_topic, self.camera_sub = ranged_topic or None, None
        self.camera_detections_topic, self.calibration = camera_detections_topic or None, calibration
        self.range_options, self.range_slop = dict(range_options or {}), float(range_slop)
        self.pairer = None
        if self.ranged_topic:
            from ..ops.range2d import RangeOptions, StampPairer

            if calibration is None or not self.camera_detections_topic:
                raise ValueError("ranged_topic needs calibration and camera_detections_topic")
            RangeOptions(**self.range_options)  # a bad option fails here, not in the first batch
            # holds a camera message for as long as its cloud may wait in the driver's window
            self.pairer = StampPairer(max(64, queue_size or 0, 2 * max(1, batch) * max(1, workers)))
        self.depth_topic, self.depth_frame_id = depth_topic or None, depth_frame_id or ""
        self.depth_options = depth_options
        if self.depth_topic:
            from ..ops.depth_image import DepthOptions

            if calibration is None or depth_options is None:
                raise ValueError("depth_topic needs calibration and depth_options")
            if not isinstance(depth_options, DepthOptions):
                self.depth_options = DepthOptions(**depth_options)  # a bad option fails here
        self.scan_topic, self.scan_frame_id = scan_topic or None, scan_frame_id or ""
        self.scan_options = scan_options
        if self.scan_topic:
            from ..ops.laser_scan import ScanOptions

            if not isinstance(scan_options, ScanOptions):
                self.scan_options = ScanOptions(**(scan_options or {}))  # a bad option fails here
        self.obstacles_topic, self.ground_topic = obstacles_topic or None, ground_topic or None
        self.ground_options = ground_options
        if self.obstacles_topic or self.ground_topic:
            from ..ops.ground import GroundOptions

            if not isinstance(ground_options, GroundOptions):
                self.ground_options = GroundOptions(**(ground_options or {}))  # a bad option fails here
        self.bus, self.jsk, self.labels, self.score_thresh = bus, jsk, labels, score_thresh
        self.queue_size, self.metrics = queue_size, metrics
        self.frames = 0
        self.sub = self.pub = None
        self.side_pubs = {}  # the publishers of the side outputs that are on, by ALL_OUTPUTS name
        # batch > 1: the reference's queue of 50 becomes a latest-wins window
        # drained as micro-batches (one engine call per batch), re-published in
        # header.seq order (see .batching)
        self.batch, self.workers = max(1, batch), max(1, workers)
        self.runner = None

    def start_inference(self, spin: bool = True, timeout: Optional[float] = None):
        p = self.params
        t = msgs.BoundingBoxArray if self.jsk else msgs.Detection3DArray
        self.pub = compat.Publisher(p["pub_topic"], t, queue_size=1, bus=self.bus)
        self.side_pubs = {name: compat.Publisher(self.side_topic(name), mtype or t, queue_size=1, bus=self.bus)
                          for name, mtype in ALL_OUTPUTS if self.side_topic(name)}
        if self.ranged_topic:
            self.camera_sub = compat.Subscriber(self.camera_detections_topic, msgs.Detection2DArray,
                                                self.pairer.push, queue_size=None, bus=self.bus)
        cb, qs = self._pc_callback, self.queue_size
        if self.batch > 1 or self.workers > 1:
            from .batching import MicroBatchRunner
            # the workers hand over whole results; the tracker is the stage that sees them in published order
            self.runner = MicroBatchRunner(self.process, self._publish, batch=self.batch, workers=self.workers,
                                           capacity=max(self.queue_size or 0, 2 * self.batch * self.workers),
                                           ordered_fn=self.track if self.tracks_topic else None)
            cb, qs = self.runner.push, None
        self.sub = compat.Subscriber(p["sub_topic"], msgs.PointCloud2, cb, queue_size=qs, bus=self.bus,
                                     ingest=getattr(self.engine, "ingest_buffer", None))
        if spin:
            compat.spin(self.bus, timeout)

    def stop(self, drain: bool = True):
        if self.sub is not None:
            self.sub.unregister()
            self.sub = None
        if self.camera_sub is not None:
            self.camera_sub.unregister()
            self.camera_sub = None
        if self.runner is not None:
            self.runner.close(drain=drain)
            self.runner = None

    def enable_bev(self, topic: str, view=None) -> None:
        """Publish the bird's-eye-view picture on ``topic``; ``view``: a ``BevView`` (default:
        the engine's point-cloud range at 0.1 m per pixel, else the KITTI range)."""
        from ..utils.bev import BevView

        cfg = getattr(self.engine, "cfg", None)
        self.bev_topic = topic
        self.bev_view = view or (BevView.for_model(cfg) if getattr(cfg, "voxel", None) is not None else BevView())

    def side_topic(self, name: str) -> Optional[str]:
        """The topic of the side output ``name`` of :data:`ALL_OUTPUTS`, None when it is off."""
        return getattr(self, name + "_topic")

    def _engine(self, name: str, *args, **kw):
        """The engine's own ``name`` method; an engine that is no Detector3D subclass and has none
        gets ``Detector3D``'s, with itself as ``self``."""
        fn = getattr(self.engine, name, None)
        return fn(*args, **kw) if fn is not None else getattr(Detector3D, name)(self.engine, *args, **kw)

    def _publish(self, r: CloudResult) -> None:
        """One cloud's messages: the box message, then every side output it has, in
        :data:`ALL_OUTPUTS` order."""
        self.pub.publish(r.boxes)
        for name, _ in ALL_OUTPUTS:
            m = getattr(r, name)
            if m is not None:
                self.side_pubs[name].publish(m)

    def to_msg(self, pred: dict, header: msgs.Header):
        idx = select_boxes(pred, self.labels, self.score_thresh)
        hdr = msgs.Header(seq=header.seq, stamp=header.stamp, frame_id=header.frame_id)
        return boxes_to_jsk(pred, idx, hdr) if self.jsk else boxes_to_detection3d(pred, idx, hdr)

    def _live(self):
        """The engine's streaming device path (LocalDetector3D on a GPU), else None."""
        if not hasattr(self, "_live_exec"):
            fn = getattr(self.engine, "live", None)
            self._live_exec = fn() if callable(fn) else None
        return self._live_exec

    def process(self, clouds: Sequence[msgs.PointCloud2]) -> List[CloudResult]:
        """One :class:`CloudResult` per cloud, in order: the box message, the prediction and the
        side output of every option that is on except ``tracks``, which :meth:`track` fills.  One
        engine call per stage for the whole batch; safe to call from several workers."""
        t0 = time.perf_counter()
        timer = StageTimer(self.metrics)
        live = self._live()
        view, pics = self.bev_view, None
        with timer("detect3d"):
            preds = live.process(clouds) if live is not None else self.engine.detect(clouds)
        if view is not None:
            with timer("bev_render"):
                pics = self._engine("render_bev", clouds, preds, view)
        with timer("boxes_publish"):
            out = [CloudResult(self.to_msg(p, c.header), p) for c, p in zip(clouds, preds)]
            for r, c, f in zip(out, clouds, pics if pics is not None else ()):
                r.bev = msgs.Image(header=c.header, height=view.H, width=view.W, encoding="rgb8", is_bigendian=0,
                                   step=3 * view.W, data=memoryview(np.ascontiguousarray(f).reshape(-1)))
        if self.points_topic:
            with timer("points_label"):
                self._points(clouds, out)
        if self.ranged_topic:
            with timer("range2d"):
                self._range(clouds, out)
        if self.depth_topic:
            with timer("depth_image"):
                self._depth(clouds, out)
        if self.scan_topic:
            with timer("laser_scan"):
                self._scan(clouds, out)
        if self.obstacles_topic or self.ground_topic:
            with timer("ground_split"):
                self._ground(clouds, out)
        self.frames += len(clouds)
        if self.metrics is not None:
            self.metrics.stage("frame3d", (time.perf_counter() - t0) / max(len(clouds), 1))
            self.metrics.frame(len(clouds))
        return out

    def _points(self, clouds, out: List[CloudResult]) -> None:
        """``points`` of every result: the cloud labelled against the boxes the box message
        carries, so ``instance`` indexes that message."""
        from ..ops.points_in_boxes import labelled_cloud

        preds = [r.pred for r in out]
        idx = [select_boxes(p, self.labels, self.score_thresh) for p in preds]
        for r, c, (_, _, payload) in zip(out, clouds, self._engine("label_points", clouds, preds, idx)):
            r.points = labelled_cloud(c, payload)

    def _range(self, clouds, out: List[CloudResult]) -> None:
        """``ranged`` and ``pred["ranged"]`` of every result: the cloud's nearest camera message
        with ranges, None without a partner within the slop.  One ranging call per batch."""
        partners = [self.pairer.nearest(c.header.stamp, self.range_slop) for c in clouds]
        res = self._engine("range_detections", clouds, partners, self.calibration, **self.range_options)
        for r, m in zip(out, res):
            r.ranged = r.pred["ranged"] = m

    def _depth(self, clouds, out: List[CloudResult]) -> None:
        """``depth`` and ``pred["depth"]`` of every result: the cloud's depth image message.  One
        call per batch."""
        res = self._engine("depth_images", clouds, self.calibration, self.depth_options, self.depth_frame_id)
        for r, m in zip(out, res):
            r.depth = r.pred["depth"] = m

    def _scan(self, clouds, out: List[CloudResult]) -> None:
        """``scan`` and ``pred["scan"]`` of every result: the cloud's LaserScan message.  One call
        per batch."""
        res = self._engine("laser_scans", clouds, self.scan_options, self.scan_frame_id)
        for r, m in zip(out, res):
            r.scan = r.pred["scan"] = m

    def _ground(self, clouds, out: List[CloudResult]) -> None:
        """``obstacles`` / ``ground`` and ``pred[...]`` of every result, for the topics that are on:
        the cloud's records above, and at or below, its estimated ground.  One call per batch."""
        want = (1 if self.obstacles_topic else 0) | (2 if self.ground_topic else 0)
        for r, (obs, gnd) in zip(out, self._engine("split_ground", clouds, self.ground_options, want)):
            if obs is not None:
                r.obstacles = r.pred["obstacles"] = obs
            if gnd is not None:
                r.ground = r.pred["ground"] = gnd

    def tracker(self):
        """The engine's tracker, made with ``track_options`` on first use."""
        return self._engine("tracker", **self.track_options)

    def track(self, results: Sequence[CloudResult]) -> List[CloudResult]:
        """The ordered stage: :meth:`process` results of consecutive clouds, in published order →
        the same results with ``tracks`` filled.  One tracker call per batch; each prediction
        gains ``track_ids``, ``track_hits`` and ``track_vel``, aligned with the published
        selection."""
        results = list(results)
        if not results:
            return []
        timer = StageTimer(self.metrics)
        with timer("track3d"):
            preds = [r.pred for r in results]
            idx = [select_boxes(p, self.labels, self.score_thresh) for p in preds]
            res = self.tracker().track(preds, idx, [r.boxes.header.stamp for r in results])
            for r, p, ix, (ids, hits, vel) in zip(results, preds, idx, res):
                p["track_ids"], p["track_hits"], p["track_vel"] = ids, hits, vel
                h = r.boxes.header
                r.tracks = boxes_to_jsk(p, ix, h, ids) if self.jsk else boxes_to_detection3d(p, ix, h, ids)
        return results

    def _pc_callback(self, msg):
        res = self.process([msg])
        for r in (self.track(res) if self.tracks_topic else res):
            self._publish(r)
