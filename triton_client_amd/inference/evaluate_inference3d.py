"""Accuracy evaluation of the LiDAR detectors, the 3D counterpart of
:mod:`.evaluate_inference` (the reference evaluates only its camera models).

Subscribes to the PointCloud2 topic (``sub_topic``) and the ground-truth topic
(``gt_topic``, ``data/client_parameter_3d.yaml``: ``/detections_3d_gt``), runs
the detector on every cloud, and scores its boxes against the ground truth by
rotated BEV or 3D IoU (:class:`..utils.evaluation.DetectionEvaluator3D`; the IoU
of the whole run is one ``tca_box3d_iou`` launch on a GPU).  Predictions and
ground truth are joined on ``header.seq``; the run finishes when a seq repeats
on both topics (the bag looped), on :meth:`finish`, or at the end of
:meth:`evaluate_bag`.  The Prometheus metrics have the names and the port of the
2D evaluator (``precision``, ``recall``, ``ap``, ``fone``, ``ap_class`` on 7658).

Ground truth is a jsk ``BoundingBoxArray`` (``label`` = class) or a
``vision_msgs/Detection3DArray`` (``results[0].id`` = class), i.e. what the live
driver publishes: :func:`gt3d_from_msg` inverts ``jsk_columns`` /
``boxes_to_detection3d``.

``min_gt_points=N`` (default 0: nothing changes) leaves out ground truth the sensor
did not see, the nuScenes rule (``filter_eval_boxes`` drops boxes without LiDAR
points; OpenPCDet's configs carry ``filter_by_min_points``): a ground-truth box
that contains fewer than N points of its cloud is dropped before it reaches the
evaluator; predictions are not filtered.  The counts come from
:class:`..ops.points_in_boxes.PointLabeler` on the boxes after ``gt_z_offset``.
Cloud and ground truth of a seq arrive in either order: whichever comes first is
held (of a cloud only x, y, z) until the other is known.
"""
from __future__ import annotations

import threading
from typing import Optional, Sequence

import numpy as np

from ..ros import compat, msgs
from ..ros.bag import Bag
from ..utils.evaluation import IOU_THRESHOLDS_3D, DetectionEvaluator3D, EvalSummary3D
from .base_inference import BaseInference
from .engines import Detector3D, RemoteDetector3D


def _yaw(qz, qw):
    return 2.0 * np.arctan2(qz, qw)


def gt3d_from_msg(msg) -> tuple:
    """→ (seq, [m, 8] x, y, z, dx, dy, dz, yaw, cls) of a jsk BoundingBoxArray
    (whose dimensions carry the reference's x/y swap: x = dy, y = dx) or a
    Detection3DArray."""
    seq = msg.header.seq
    if hasattr(msg, "boxes"):
        cols = getattr(msg.boxes, "columns", None)
        if cols is not None and not msg.boxes.built:  # still the publisher's columns: no objects are made
            q, d = np.asarray(cols["orientation"], np.float64), np.asarray(cols["dimensions"], np.float64)
            g = np.concatenate([np.asarray(cols["position"], np.float64).reshape(-1, 3), d.reshape(-1, 3)[:, [1, 0, 2]],
                                _yaw(q.reshape(-1, 4)[:, 2], q.reshape(-1, 4)[:, 3])[:, None],
                                np.asarray(cols["label"], np.float64).reshape(-1, 1)], 1)
            return seq, g
        g = np.zeros((len(msg.boxes), 8), np.float64)
        for i, b in enumerate(msg.boxes):
            p, q, d = b.pose.position, b.pose.orientation, b.dimensions
            g[i] = [p.x, p.y, p.z, d.y, d.x, d.z, _yaw(q.z, q.w), b.label]
        return seq, g
    g = np.zeros((len(msg.detections), 8), np.float64)
    for i, det in enumerate(msg.detections):
        p, q, s = det.bbox.center.position, det.bbox.center.orientation, det.bbox.size
        g[i] = [p.x, p.y, p.z, s.x, s.y, s.z, _yaw(q.z, q.w), det.results[0].id if det.results else 0]
    return seq, g


class EvaluateInference3D(BaseInference):
    """``gt_z_offset`` is added to the ground truth's z before the comparison.
    The engines publish boxes in the sensor frame (the ``z_offset`` they add
    before voxelising is taken out of their results), so ground truth recorded
    in the sensor frame needs 0, the default; ground truth labelled on clouds
    that already carry the reference's ``z += 1.5`` needs ``-1.5``.  Only
    ``metric="3d"`` depends on it.  Predictions below ``conf_thres`` are dropped."""

    def __init__(self, channel=None, client=None, engine: Optional[Detector3D] = None, params: Optional[dict] = None,
                 bus=None, metrics_port: Optional[int] = 7658, metric: str = "bev",
                 iouv: Sequence[float] = IOU_THRESHOLDS_3D, conf_thres: float = 0.0, z_offset: float = 1.5,
                 gt_z_offset: float = 0.0, gt_type: str = "jsk", device="auto", class_names=None,
                 min_gt_points: int = 0):
        super().__init__(channel, client)
        self._params = params or {}
        self.engine = engine or RemoteDetector3D(channel, client, z_offset=z_offset)
        self.class_names = class_names or list(getattr(self.engine, "names", []) or [])
        self.label_base = getattr(self.engine, "label_base", 1)
        self.bus, self.conf_thres, self.gt_z_offset = bus, conf_thres, float(gt_z_offset)
        if gt_type not in ("jsk", "detection3d"):
            raise ValueError(f"gt_type {gt_type!r}: 'jsk' or 'detection3d'")
        self.gt_msg_type = msgs.BoundingBoxArray if gt_type == "jsk" else msgs.Detection3DArray
        self.evaluator = DetectionEvaluator3D(metric=metric, iouv=np.asarray(iouv, np.float64), device=device)
        self.min_gt_points, self.gt_dropped = max(0, int(min_gt_points)), 0
        self._labeler, self._device = None, device
        self._held_clouds, self._held_gts = {}, {}  # seq -> xyz cloud / ground truth waiting for the other
        self.metrics = None
        if metrics_port is not None:
            from ..utils.metrics import EvalMetrics

            self.metrics = EvalMetrics(metrics_port)
        self.pc_processed = self.gt_processed = False
        self.done = threading.Event()
        self._lock = threading.Lock()
        self.summary: Optional[EvalSummary3D] = None
        self.pc_sub = self.gt_sub = None

    # ------------------------------------------------------------------ live
    def start_inference(self, spin: bool = True, timeout: Optional[float] = None):
        p = self.params
        self.pc_sub = compat.Subscriber(p["sub_topic"], msgs.PointCloud2, self.cloud_callback, queue_size=None,
                                        bus=self.bus)
        self.gt_sub = compat.Subscriber(p["gt_topic"], self.gt_msg_type, self.gt_callback, queue_size=None,
                                        bus=self.bus)
        if spin:
            self.done.wait(timeout)
            return self.finish()

    def cloud_callback(self, msg):
        seq = msg.header.seq
        with self._lock:
            if seq in self.evaluator.preds:  # bag looped: clouds are complete
                self.pc_processed = True
                self._maybe_done()
                return
        d = self.engine.detect([msg])[0]
        with self._lock:
            self.evaluator.add_detections(seq, d, self.conf_thres)
            if self.min_gt_points:
                self._cloud_known(msg)

    def _add_gt(self, msg):
        seq, g = gt3d_from_msg(msg)
        g[:, 2] += self.gt_z_offset
        if not self.min_gt_points:
            self.evaluator.add_ground_truth(seq, g)
        elif seq in self._held_clouds:
            self._add_seen_gt(seq, g, self._held_clouds.pop(seq))
        else:
            self._held_gts[seq] = g

    def _cloud_known(self, msg):
        """The cloud of a seq has arrived: filter its waiting ground truth, or keep its x, y, z."""
        from ..ops.points_in_boxes import cloud_xyzi, xyz_cloud

        seq = msg.header.seq
        if seq in self._held_gts:
            self._add_seen_gt(seq, self._held_gts.pop(seq), msg)
        elif seq not in self.evaluator.gts:
            self._held_clouds[seq] = xyz_cloud(cloud_xyzi(msg), msg.header)

    def _add_seen_gt(self, seq, g, cloud):
        """Ground truth with at least ``min_gt_points`` points of its cloud inside → the evaluator."""
        if self._labeler is None:
            from ..ops.points_in_boxes import PointLabeler

            self._labeler = PointLabeler(self._device)
        keep = self._labeler.count_points(cloud, g[:, :7]) >= self.min_gt_points
        self.gt_dropped += int((~keep).sum())
        self.evaluator.add_ground_truth(seq, g[keep])

    def gt_callback(self, msg):
        with self._lock:
            if msg.header.seq in self.evaluator.gts or msg.header.seq in self._held_gts:
                self.gt_processed = True
                self._maybe_done()
                return
            self._add_gt(msg)

    def _maybe_done(self):
        if self.pc_processed and self.gt_processed:
            self.done.set()

    # ------------------------------------------------------------------ offline
    def evaluate_bag(self, bagfile: str, batch: int = 8) -> EvalSummary3D:
        """Evaluate the cloud + ground-truth topics of a bag, ``batch`` clouds per engine call."""
        p = self.params
        pending = []
        with Bag(bagfile) as bag:
            for topic, m, _ in bag.read_messages(topics=[p["sub_topic"], p["gt_topic"]]):
                if topic == p["gt_topic"]:
                    self._add_gt(m)
                    continue
                pending.append(m)
                if len(pending) == batch:
                    self._run(pending)
                    pending = []
        if pending:
            self._run(pending)
        return self.finish()

    def _run(self, clouds):
        for m, d in zip(clouds, self.engine.detect(clouds)):
            self.evaluator.add_detections(m.header.seq, d, self.conf_thres)
            if self.min_gt_points:
                self._cloud_known(m)

    # ------------------------------------------------------------------ metrics
    def calculate_metrics(self) -> EvalSummary3D:
        with self._lock:
            s = self.evaluator.summary()
        if self.metrics is not None and getattr(self.metrics, "reg", None) is not None:
            k = int(np.argmin(np.abs(s.iouv - 0.5)))  # `ap`: the column at (or nearest) IoU 0.5, as in 2D
            for v in s.precision:
                self.metrics.p_summary.observe(float(v))
            for v in s.recall:
                self.metrics.r_summary.observe(float(v))
            for v in s.ap[:, k] if len(s.ap) else []:
                self.metrics.ap_summary.observe(float(v))
            for v in s.f1:
                self.metrics.f1_summary.observe(float(v))
            for v in s.classes:
                self.metrics.ap_class_summary.observe(float(v))
        return s

    def finish(self) -> EvalSummary3D:
        for sub in (self.pc_sub, self.gt_sub):
            if sub is not None:
                sub.unregister()
        self.pc_sub = self.gt_sub = None
        with self._lock:  # ground truth whose cloud never came: no prediction to score it against, kept as it is
            for seq, g in self._held_gts.items():
                self.evaluator.add_ground_truth(seq, g)
            self._held_gts, self._held_clouds = {}, {}
        self.summary = self.calculate_metrics()
        return self.summary

    def as_dict(self) -> dict:
        d = self.summary.as_dict(self.class_names or None, self.label_base)
        if self.min_gt_points:
            d["min_gt_points"], d["gt_dropped"] = self.min_gt_points, self.gt_dropped
        return d
