"""3D accuracy evaluation (``EvaluateInference3D``): PointCloud2 + ground-truth boxes
(jsk BoundingBoxArray or Detection3DArray) → P/R/AP/F1 by rotated BEV or 3D IoU,
exported to Prometheus :7658."""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys

from .common import DATA, add_framework_flags, add_reference_flags, load_params, play_bag, setup_logging
from .engines import engine_3d, lidar_family

EVAL_CONF = 0.05  # default --conf-thres: low on purpose, so the PR curve reaches high recall


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__)
    add_reference_flags(p, "pointpillar_kitti")
    add_framework_flags(p, os.path.join(DATA, "client_parameter_3d.yaml"), three_d=True)
    p.add_argument("--bag", default=None, help="evaluate this bag offline (cloud + gt topics)")
    p.add_argument("--metric", choices=["bev", "3d"], default="bev", help="rotated BEV IoU or 3D IoU")
    p.add_argument("--iou", default="0.25,0.5,0.7", help="IoU thresholds, ascending (comma list)")
    p.add_argument("--conf-thres", type=float, default=EVAL_CONF,
                   help="keep predictions from this score up (the local engine's score threshold is lowered to it; "
                        "a remote server applies its own first)")
    p.add_argument("--gt-z-offset", type=float, default=0.0,
                   help="added to the ground truth's z (0: ground truth in the sensor frame, like the engines' "
                        "boxes; only --metric 3d depends on it)")
    p.add_argument("--min-gt-points", type=int, default=0, metavar="N",
                   help="drop ground-truth boxes that contain fewer than N points of their cloud (the nuScenes rule; "
                        "0: keep all)")
    p.add_argument("--eval-port", type=int, default=7658, help="Prometheus port (reference 7658; 0 = off)")
    p.add_argument("--json", default=None, help="write the summary here")
    return p.parse_args(argv)


def _engine(flags, params):
    """The 3D engine of the flags; a local one scores down to ``--conf-thres``."""
    if flags.engine != "local":
        return engine_3d(flags, params)
    from ..config.lidar import LIDAR_FAMILIES
    from ..inference import LocalDetector3D

    family = lidar_family(flags.model_name)
    cfg = LIDAR_FAMILIES[family].config()
    cfg = dataclasses.replace(cfg, score_thresh=min(cfg.score_thresh, flags.conf_thres))
    return LocalDetector3D(cfg=cfg, batch=max(1, flags.frames_per_step), device=flags.device, weights=flags.weights,
                           z_offset=flags.z_offset, family=family), None, None


def main(argv=None) -> int:
    flags = parse_args(argv)
    setup_logging(flags.verbose)
    from ..inference import EvaluateInference3D
    from ..ros import compat, default_bus

    compat.init_node("ros_evaluate_3d")
    params = load_params(flags.params, flags.server)
    engine, channel, client = _engine(flags, params)
    ev =EvaluateInference3D(channel, client, engine=engine, params=params, metrics_port=flags.eval_port or None,
                             bus=default_bus(), metric=flags.metric, iouv=[float(v) for v in flags.iou.split(",")],
                             conf_thres=flags.conf_thres, gt_z_offset=flags.gt_z_offset,
                             gt_type="detection3d" if flags.detection3d else "jsk", device=flags.device,
                             min_gt_points=flags.min_gt_points)
    if flags.bag:
        ev.evaluate_bag(flags.bag, batch=max(1, flags.frames_per_step))
    else:
        if flags.play:
            play_bag(flags.play, default_bus(), topics=[params["sub_topic"], params["gt_topic"]], shutdown=False)
        ev.start_inference(spin=True, timeout=flags.spin_timeout)
    if hasattr(engine, "release_transport"):
        engine.release_transport()
    out = ev.as_dict()
    print(json.dumps(out, indent=1))
    if flags.json:
        with open(flags.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
