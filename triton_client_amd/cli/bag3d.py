"""Offline 3D bag replay (reference ``bag3d.py``): bag → <bag>_output.bag with boxes."""
from __future__ import annotations

import argparse
import os
import sys

from .common import (DATA, add_depth_flags, add_framework_flags, add_ground_flags, add_range_flags,
                     add_reference_flags, add_scan_flags, add_track_flags, bev_view, depth_options, ground_options,
                     labels_arg, load_params, range_options, scan_options, setup_logging, track_options)
from .engines import engine_3d, export_if_asked, maybe_data_parallel


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__)
    add_reference_flags(p, "pointpillar_kitti")
    add_framework_flags(p, os.path.join(DATA, "client_parameter_3d.yaml"), three_d=True)
    p.add_argument("--bag", required=True, help="input bag")
    p.add_argument("--out-bag", default="", help="output bag (default <bag>_output.bag, 'none' to skip)")
    p.add_argument("--start-seq", type=int, default=0)
    p.add_argument("--max-frames", type=int, default=None)
    p.add_argument("--bev-out", default="", metavar="DIR",
                   help="save every cloud's bird's-eye-view picture (points + all detections) as DIR/NNNN.png")
    p.add_argument("--bev-res", type=float, default=0.1, metavar="M", help="metres per pixel of --bev-out")
    p.add_argument("--points-topic", default="", metavar="TOPIC",
                   help="write every cloud with its labels (x, y, z, intensity, label, instance, score per point) to "
                        "the output bag on this topic")
    add_track_flags(p, "write the boxes of every cloud, with their track ids in place of their classes, to the "
                       "output bag on this topic")
    add_range_flags(p, "write, per cloud, the nearest camera Detection2DArray of --camera-detections-topic (read from "
                       "the bag in a first pass) to the output bag on this topic, with each detection's "
                       "camera-frame position from the LiDAR points (needs --calib)")
    add_depth_flags(p, "write every cloud as a depth Image registered to the camera's pixels to the output bag on this "
                       "topic (needs --calib and --depth-size)")
    p.add_argument("--depth-out", default="", metavar="DIR",
                   help="save every cloud's 16UC1 depth image as the 16-bit greyscale DIR/NNNN.png (the numbering of "
                        "--bev-out)")
    add_scan_flags(p, "write every cloud as a sensor_msgs/LaserScan (per angular bin the nearest return in the height "
                      "band; pointcloud_to_laserscan's parameters) to the output bag on this topic")
    add_ground_flags(p, "write, per cloud, the input records that stand above the estimated ground (a PointCloud2 with "
                        "the input's fields, in input order) to the output bag on this topic",
                     "write, per cloud, the input records at or below the estimated ground to the output bag on this "
                     "topic")
    flags = p.parse_args(argv)
    flags.calibration, flags.range_options = range_options(flags, p.error)  # a usage error ends here
    flags.calibration, flags.depth_options = depth_options(flags, p.error)
    flags.scan_options = scan_options(flags, p.error)
    flags.ground_options = ground_options(flags, p.error)
    return flags


def main(argv=None) -> int:
    flags = parse_args(argv)
    setup_logging(flags.verbose)
    from ..inference import BagInference3D

    params = load_params(flags.params, flags.server)
    engine, channel, client = engine_3d(flags, params)
    info = None
    if flags.engine == "local":
        engine, info = maybe_data_parallel(engine, three_d=True)
        if info is not None and not info.is_main:  # worker rank: serve shards until rank 0 is done
            engine.serve()
            from ..parallel.dp import shutdown
            shutdown(info)
            return 0
    drv = BagInference3D(channel, client, engine=engine, params=params, bagfile=flags.bag,
                         out_bag=None if flags.out_bag == "none" else flags.out_bag,
                         batch=max(1, flags.frames_per_step), start_seq=flags.start_seq,
                         max_frames=flags.max_frames, verbose=flags.verbose, jsk=not flags.detection3d,
                         labels=labels_arg(flags.labels), score_thresh=flags.score_thresh,
                         bev_out=flags.bev_out or None, bev_view=bev_view(engine, flags.bev_res, flags.bev_out),
                         points_topic=flags.points_topic or None, tracks_topic=flags.tracks_topic or None,
                         track_options=track_options(flags), ranged_topic=flags.ranged_topic or None,
                         camera_detections_topic=flags.camera_detections_topic or None,
                         calibration=flags.calibration, range_options=flags.range_options,
                         range_slop=flags.range_slop, depth_topic=flags.depth_topic or None,
                         depth_options=flags.depth_options, depth_frame_id=flags.depth_frame_id or "",
                         depth_out=flags.depth_out or None, scan_topic=flags.scan_topic or None,
                         scan_options=flags.scan_options, scan_frame_id=flags.scan_frame_id or "",
                         obstacles_topic=flags.obstacles_topic or None, ground_topic=flags.ground_topic or None,
                         ground_options=flags.ground_options)
    n = drv.start_inference()
    export_if_asked(flags, engine)
    if info is not None:
        engine.close()
        from ..parallel.dp import shutdown
        shutdown(info)
    fps = n / drv.elapsed if drv.elapsed > 0 else 0.0
    print(f"processed {n} clouds in {drv.elapsed:.2f}s ({fps:.1f} FPS)", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
