"""3D live inference (reference ``main3d.py``): PointCloud2 topic → 3D boxes."""
from __future__ import annotations

import argparse
import os
import sys

from .common import (DATA, add_depth_flags, add_framework_flags, add_ground_flags, add_range_flags,
                     add_reference_flags, add_scan_flags, add_track_flags, bev_view, depth_options, ground_options,
                     labels_arg, load_params, play_bag, range_options, scan_options, setup_logging, track_options)
from .engines import engine_3d, export_if_asked, maybe_data_parallel


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__)
    add_reference_flags(p, "pointpillar_kitti")
    add_framework_flags(p, os.path.join(DATA, "client_parameter_3d.yaml"), three_d=True)
    p.add_argument("--bev-topic", default="", metavar="TOPIC",
                   help="also publish an rgb8 Image of every cloud from above (points + all detections) here")
    p.add_argument("--bev-res", type=float, default=0.1, metavar="M", help="metres per pixel of --bev-topic")
    p.add_argument("--points-topic", default="", metavar="TOPIC",
                   help="also publish every cloud with its labels here: a PointCloud2 of x, y, z, intensity, label, "
                        "instance (index into the box message), score per point")
    add_track_flags(p, "also publish the boxes of every cloud here with their track ids in place of their classes")
    add_range_flags(p, "also publish, per cloud, the nearest camera Detection2DArray of --camera-detections-topic here "
                       "with each detection's camera-frame position from the LiDAR points (needs --calib)")
    add_depth_flags(p, "also publish every cloud here as a depth Image registered to the camera's pixels (needs "
                       "--calib and --depth-size)")
    add_scan_flags(p, "also publish every cloud here as a sensor_msgs/LaserScan for 2D navigation: per angular bin the "
                      "nearest return in the height band (pointcloud_to_laserscan's parameters)")
    add_ground_flags(p, "also publish here, per cloud, the input records that stand above the estimated ground (a "
                        "PointCloud2 with the input's fields, in input order)",
                     "also publish here, per cloud, the input records at or below the estimated ground")
    flags = p.parse_args(argv)
    flags.calibration, flags.range_options = range_options(flags, p.error)  # a usage error ends here
    flags.calibration, flags.depth_options = depth_options(flags, p.error)
    flags.scan_options = scan_options(flags, p.error)
    flags.ground_options = ground_options(flags, p.error)
    return flags


def main(argv=None) -> int:
    flags = parse_args(argv)
    setup_logging(flags.verbose)
    from ..inference import RosInference3D
    from ..ros import compat, default_bus

    compat.init_node("ros_infer_3d")
    params = load_params(flags.params, flags.server)
    engine, channel, client = engine_3d(flags, params)
    info = None
    if flags.engine == "local":  # under torchrun: shard every micro-batch over the node's GPUs
        engine, info = maybe_data_parallel(engine, three_d=True)
        if info is not None and not info.is_main:
            engine.serve()
            from ..parallel.dp import shutdown
            shutdown(info)
            return 0
    bus = default_bus() if (flags.play or not compat.HAVE_ROSPY) else None
    drv = RosInference3D(channel, client, engine=engine, params=params, bus=bus, jsk=not flags.detection3d,
                         labels=labels_arg(flags.labels), score_thresh=flags.score_thresh,
                         queue_size=None if flags.play else 50,
                         batch=flags.live_batch, workers=flags.live_workers, bev_topic=flags.bev_topic or None,
                         bev_view=bev_view(engine, flags.bev_res, flags.bev_topic),
                         points_topic=flags.points_topic or None, tracks_topic=flags.tracks_topic or None,
                         track_options=track_options(flags), ranged_topic=flags.ranged_topic or None,
                         camera_detections_topic=flags.camera_detections_topic or None,
                         calibration=flags.calibration, range_options=flags.range_options,
                         range_slop=flags.range_slop, depth_topic=flags.depth_topic or None,
                         depth_options=flags.depth_options, depth_frame_id=flags.depth_frame_id or "",
                         scan_topic=flags.scan_topic or None, scan_options=flags.scan_options,
                         scan_frame_id=flags.scan_frame_id or "",
                         obstacles_topic=flags.obstacles_topic or None, ground_topic=flags.ground_topic or None,
                         ground_options=flags.ground_options)
    if flags.play:
        play_bag(flags.play, bus, topics=[params["sub_topic"]] + ([flags.camera_detections_topic]
                                                                  if flags.ranged_topic else []))
    drv.start_inference(spin=True, timeout=flags.spin_timeout)
    drv.stop()
    if hasattr(engine, "release_transport"):  # a remote client's shared-memory regions
        engine.release_transport()
    export_if_asked(flags, engine)
    if info is not None:
        engine.close()
        from ..parallel.dp import shutdown
        shutdown(info)
    print(f"processed {drv.frames} clouds", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
