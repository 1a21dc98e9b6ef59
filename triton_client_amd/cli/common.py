"""Shared command-line surface of the entry points.

The reference's flags are kept with the same names and defaults
(``main.py:51-113``; identical in ``main3d.py``, ``bag2d.py``,
``bag3d.py``): ``-v``, ``-a/--async``, ``--streaming``, ``-m``, ``-x``,
``-b``, ``-c``, ``-s``, ``-i``.  Additions are listed in ``--help``:

* the engine — ``remote`` (a KServe/Triton server, as in the reference) or
  ``local`` (in-process MI355X pipeline);
* the client parameter file.  The reference read it through the rosparam
  ``client_parameter_file`` (``main.py:119-121``);
* the bag paths.  The reference hard-coded them;
* ``--client``, which picks the client by model family.  The reference
  always used YOLOv5 (A1).
"""
from __future__ import annotations

import argparse
import logging
import os
from typing import Optional

import yaml

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "data")


def add_reference_flags(p: argparse.ArgumentParser, default_model: str = "YOLOv5n") -> None:
    p.add_argument("-v", "--verbose", action="store_true", default=False, help="Enable verbose output")
    p.add_argument("-a", "--async", dest="async_set", action="store_true", default=False,
                   help="Use asynchronous inference API")
    p.add_argument("--streaming", action="store_true", default=False, help="Use streaming inference API")
    p.add_argument("-m", "--model-name", type=str, default=default_model, help="Name of model")
    p.add_argument("-x", "--model-version", type=str, default="",
                   help="Version of model. Default is to use latest version.")
    p.add_argument("-b", "--batch-size", type=int, default=1, help="Batch size. Default is 1.")
    p.add_argument("-c", "--classes", type=int, default=80, help="Number of class results to report.")
    p.add_argument("-s", "--scaling", type=str, choices=["NONE", "INCEPTION", "VGG", "COCO"], default="COCO",
                   help="Type of scaling to apply to image pixels.")
    p.add_argument("-i", "--image-src", type=str, choices=["ros", "local"], default="ros",
                   help="Source of input: the ROS topic (or a replayed bag) or local image files")


def add_framework_flags(p: argparse.ArgumentParser, params_default: str, three_d: bool = False) -> None:
    g = p.add_argument_group("triton_client_amd")
    g.add_argument("--params", default=params_default, help="client parameter YAML (grpc_channel, topics)")
    g.add_argument("--engine", choices=["remote", "local"], default="remote",
                   help="remote: KServe/Triton server at grpc_channel; local: in-process MI355X pipeline")
    g.add_argument("--client", choices=["auto", "yolov5", "fcos", "pointpillars"], default="auto",
                   help="model-family client (auto: from the model's config)")
    g.add_argument("--server", default=None, help="override grpc_channel host:port")
    g.add_argument("--device", default="auto",
                   help="where the engine runs: the local pipeline, or the remote client's decode / preprocess / "
                        "postprocess HIP kernels (auto: the first GPU if there is one; cuda:N; cpu)")
    g.add_argument("--frames-per-step", type=int, default=8, help="micro-batch for bag replay / local engine")
    g.add_argument("--live-batch", type=int, default=1,
                   help="live topic: run up to N pending frames per engine call (latest-wins window, "
                        "re-published in header.seq order); 1 = the reference's one frame per callback")
    g.add_argument("--live-workers", type=int, default=1,
                   help="live topic: micro-batches in flight (host work of one overlaps another's GPU work)")
    g.add_argument("--wire", choices=["raw", "proto", "shm", "devshm"], default="raw",
                   help="raw: C++ zero-copy KServe codec; proto: reference-style protobuf request; shm: KServe "
                        "system shared memory (server on the same host; tensors stay in a /dev/shm region); "
                        "devshm: KServe device shared memory (server on the same GPU node; the model input and "
                        "outputs stay in a GPU allocation the server maps by HIP IPC handle -- needs --device cuda)")
    g.add_argument("--timeout", type=float, default=None, help="per-RPC deadline (s); default none")
    g.add_argument("--retries", type=int, default=2, help="retries on UNAVAILABLE/DEADLINE_EXCEEDED")
    g.add_argument("--weights", default=None, help="state_dict for the local engine: path, file://, http(s):// or s3:// URI (loaded with torch.load weights_only)")
    g.add_argument("--export-weights", default=None,
                   help="local engine: after the run, save its fused, calibrated weights here (reload with --weights "
                        "to reproduce them exactly, e.g. on every rank or host of a deployment)")
    g.add_argument("--play", default=None, help="replay this bag onto the in-process topic bus (no rospy)")
    g.add_argument("--spin-timeout", type=float, default=None, help="stop spinning after N seconds")
    g.add_argument("--metrics-port", type=int, default=None, help="Prometheus exporter port for client metrics")
    if three_d:
        g.add_argument("--detection3d", action="store_true", help="publish vision_msgs/Detection3DArray, not jsk")
        g.add_argument("--labels", default="2", help="labels to publish (comma list, 'all'); reference: 2")
        g.add_argument("--score-thresh", type=float, default=0.5, help="publish threshold (reference 0.5)")
        g.add_argument("--z-offset", type=float, default=1.5, help="z added before voxelising (reference 1.5)")
    else:
        g.add_argument("--letterbox", action="store_true", help="letterbox instead of the reference's stretch")
        g.add_argument("--conf-thres", type=float, default=0.3, help="reference: 0.3")
        g.add_argument("--images", default=None, help="directory of images for -i local")
        g.add_argument("--publish-compressed", action="store_true", default=False,
                       help="publish the annotated frame as a JPEG CompressedImage on <pub_topic>/compressed instead of "
                            "the raw Image (local GPU engine: encoded on the device; not with data-parallel ranks)")
        g.add_argument("--jpeg-quality", type=int, default=90, help="--publish-compressed: JPEG quality 1..100")
        g.add_argument("--jpeg-subsampling", choices=["4:2:0", "4:2:2", "4:4:4"], default="4:2:0",
                       help="--publish-compressed: chroma subsampling")
        g.add_argument("--rectify", default="", metavar="CAMERA.yaml",
                       help="rectify every frame from this camera_calibration YAML before detection: the annotated "
                            "frame, the detections and the tracks are in rectified pixels (local GPU engine: on the "
                            "device; not with data-parallel ranks)")


def load_params(path: Optional[str], server: Optional[str] = None) -> dict:
    from ..ros import compat

    path = compat.get_param("client_parameter_file", path) or path
    with open(path) as f:
        params = yaml.safe_load(f)
    if server:
        params["grpc_channel"] = server
    return params


def setup_logging(verbose: bool) -> None:
    logging.basicConfig(level=logging.DEBUG if verbose else logging.INFO,
                        format="%(asctime)s %(levelname)s %(name)s: %(message)s")


def make_channel(params: dict, flags):
    from ..channel.grpc_channel import GRPCChannel

    return GRPCChannel(params, flags, timeout_s=getattr(flags, "timeout", None), retries=getattr(flags, "retries", 2))


def resolve_device(flag: Optional[str]) -> str:
    """``--device``: "auto" is the first visible GPU when there is one, else the CPU
    (config 1, the CPU-only client); anything else is taken as given."""
    if flag in (None, "", "auto"):
        import torch

        return "cuda" if torch.cuda.is_available() else "cpu"
    return flag


def make_client(flags, channel=None):
    """The model-family client, its pre/postprocess on ``--device`` (the remote
    engine's HIP path on a GPU client)."""
    from ..clients import FCOS_client, Pointpillars_client, Yolov5client, client_for_model

    dev = resolve_device(getattr(flags, "device", "cpu"))
    c = getattr(flags, "client", "auto")
    if c == "yolov5":
        return Yolov5client(dev)
    if c == "fcos":
        return FCOS_client(dev)
    if c == "pointpillars":
        return Pointpillars_client(dev)
    cfg = None
    if channel is not None:
        cr = channel.get_metadata().get("config_response")
        cfg = getattr(cr, "config", cr)
    return client_for_model(flags.model_name, cfg, dev)


def rpc_mode(flags) -> str:
    return "stream" if flags.streaming else "async" if flags.async_set else "sync"


def jpeg_options(flags):
    """The drivers' ``compressed=`` option of --publish-compressed / --jpeg-*; None when off."""
    if not getattr(flags, "publish_compressed", False):
        return None
    from ..ops.jpeg_encode import JpegOptions

    return JpegOptions(quality=flags.jpeg_quality, subsampling=flags.jpeg_subsampling)


def rectify_model(flags):
    """The drivers' ``rectify=`` option of --rectify; None when off."""
    path = getattr(flags, "rectify", "")
    if not path:
        return None
    from ..ops.rectify import load_camera_model

    return load_camera_model(path)


def labels_arg(s: str):
    return None if s in ("all", "", "none") else tuple(int(v) for v in s.split(","))


def add_track_flags(p: argparse.ArgumentParser, topic_help: str) -> None:
    """--tracks-topic, --track-max-age, --track-max-dist (``ops/track3d.py``)."""
    p.add_argument("--tracks-topic", default="", metavar="TOPIC", help=topic_help)
    p.add_argument("--track-max-age", type=int, default=3, metavar="FRAMES",
                   help="a track missed this many clouds in a row still comes back with its id")
    p.add_argument("--track-max-dist", default="", metavar="M | NAME=M,...",
                   help="association gate in metres: one number for every class, or by class name (Car=4,"
                        "Pedestrian=1; default 2, CenterPoint: the paper's nuScenes table)")


def track_options(flags) -> dict:
    """The ``track_options`` of the --track-* flags."""
    from ..ops.track3d import parse_max_dist

    opts = {"max_age": flags.track_max_age}
    md = parse_max_dist(flags.track_max_dist)
    if md is not None:
        opts["max_dist"] = md
    return opts


def add_track2d_flags(p: argparse.ArgumentParser, topic_help: str) -> None:
    """--tracks-topic, --track-max-age, --track-high-score, --track-min-iou (``ops/track2d.py``)."""
    p.add_argument("--tracks-topic", default="", metavar="TOPIC", help=topic_help)
    p.add_argument("--track-max-age", type=int, default=30, metavar="FRAMES",
                   help="a track missed this many frames in a row still comes back with its id")
    p.add_argument("--track-high-score", type=float, default=0.5, metavar="SCORE",
                   help="detections scoring at least this may match any live track; lower ones only keep alive a "
                        "track matched in the previous frame")
    p.add_argument("--track-min-iou", type=float, default=0.2, metavar="IOU",
                   help="association gate of the high-score detections: IoU with the track's predicted box")


def track2d_options(flags) -> dict:
    """The ``track_options`` of the 2D --track-* flags."""
    return {"max_age": flags.track_max_age, "high_score": flags.track_high_score, "min_iou": flags.track_min_iou}


def add_range_flags(p: argparse.ArgumentParser, topic_help: str) -> None:
    """--ranged-topic, --camera-detections-topic, --calib and --range-* (``ops/range2d.py``)."""
    p.add_argument("--ranged-topic", default="", metavar="TOPIC", help=topic_help)
    p.add_argument("--camera-detections-topic", default="", metavar="TOPIC",
                   help="the camera's vision_msgs/Detection2DArray topic that --ranged-topic ranges")
    p.add_argument("--calib", default="", metavar="FILE",
                   help="camera-LiDAR calibration: YAML with projection (3x3 or 3x4) and lidar_to_camera (3x4 or "
                        "4x4), or a KITTI calib/*.txt (P2, R0_rect, Tr_velo_to_cam)")
    p.add_argument("--range-slop", type=float, default=0.05, metavar="S",
                   help="a cloud pairs with the camera message nearest in time within this many seconds")
    p.add_argument("--range-shrink", type=float, default=0.6, metavar="F",
                   help="the pixel box is shrunk about its centre by this factor, in (0, 1], before points count")
    p.add_argument("--range-quantile", type=int, default=50, metavar="PCT",
                   help="the depth quantile that picks the object's depth bin, 1..100")
    p.add_argument("--range-min-points", type=int, default=3, metavar="N",
                   help="a box with fewer points inside gets no range")
    p.add_argument("--range-bin", type=float, default=0.25, metavar="M",
                   help="depth bin width in metres (512 bins: 0.25 reaches 128 m)")


def range_options(flags, error=None):
    """``(calibration, range_options)`` of the --calib / --range-* flags, ``(None, {})`` without
    --ranged-topic.  A ranged topic without a calibration or a detections topic, a calibration
    that does not load and an option out of range are usage errors: ``error`` (an
    ``ArgumentParser.error``) is called with the message, else ``ValueError`` is raised."""
    if not getattr(flags, "ranged_topic", ""):
        return None, {}
    from ..ops.range2d import RangeOptions, load_calibration

    def fail(msg):
        if error is not None:
            error(msg)
        raise ValueError(msg)

    if not flags.calib:
        fail("--ranged-topic needs --calib FILE")
    if not flags.camera_detections_topic:
        fail("--ranged-topic needs --camera-detections-topic TOPIC")
    if not (flags.range_slop >= 0):
        fail("--range-slop must be >= 0")
    opts = {"shrink": flags.range_shrink, "pct": flags.range_quantile, "min_points": flags.range_min_points,
            "bin_w": flags.range_bin}
    try:
        RangeOptions(**opts)
        cal = load_calibration(flags.calib)
    except (ValueError, OSError) as e:
        fail(f"--ranged-topic: {e}")
    return cal, opts


_DEPTH_FLAGS = ("depth_size", "depth_encoding", "depth_scale", "depth_min", "depth_splat", "depth_frame_id")


def add_depth_flags(p: argparse.ArgumentParser, topic_help: str) -> None:
    """--depth-topic, --depth-size and --depth-* (``ops/depth_image.py``); --calib is the range
    flags' own.  The option flags default to None so that one given without a topic is seen."""
    p.add_argument("--depth-topic", default="", metavar="TOPIC", help=topic_help)
    p.add_argument("--depth-size", default=None, metavar="WxH", help="the camera's image size in pixels, e.g. 1280x720")
    p.add_argument("--depth-encoding", default=None, choices=["16UC1", "32FC1"],
                   help="16UC1 (default): depth in 1/--depth-scale metres, 0 for no return (REP 118); 32FC1: metres, "
                        "NaN for no return")
    p.add_argument("--depth-scale", type=float, default=None, metavar="S",
                   help="16UC1 units per metre (default 1000: millimetres; 256: the KITTI depth-PNG convention)")
    p.add_argument("--depth-min", type=float, default=None, metavar="M",
                   help="points nearer than this many metres in front of the camera are left out (default 0.5)")
    p.add_argument("--depth-splat", type=int, default=None, metavar="R",
                   help="a point covers the (2R+1)^2 pixels around its own, 0..4 (default 1)")
    p.add_argument("--depth-frame-id", default=None, metavar="FRAME",
                   help="frame_id of the depth images (default: the cloud's)")


def depth_options(flags, error=None):
    """``(calibration, depth_options)`` of the --depth-* flags: ``flags.calibration`` (loaded
    from --calib when ranging has not) and a ``DepthOptions``, or ``(flags.calibration, None)``
    without --depth-topic / --depth-out.  A depth topic without --calib or --depth-size, a
    --depth-* flag without a topic, --depth-out with 32FC1 and an option out of range are usage
    errors: ``error`` (an ``ArgumentParser.error``) is called with the message, else
    ``ValueError`` is raised."""
    def fail(msg):
        if error is not None:
            error(msg)
        raise ValueError(msg)

    cal = getattr(flags, "calibration", None)
    out_dir = getattr(flags, "depth_out", "")
    if not (flags.depth_topic or out_dir):
        given = [f for f in _DEPTH_FLAGS if getattr(flags, f) is not None]
        if given:
            fail(f"--{given[0].replace('_', '-')} needs --depth-topic TOPIC" + (" or --depth-out DIR" if hasattr(
                flags, "depth_out") else ""))
        return cal, None
    from ..ops.depth_image import DepthOptions
    from ..ops.range2d import load_calibration

    what = "--depth-topic" if flags.depth_topic else "--depth-out"
    if not flags.calib:
        fail(f"{what} needs --calib FILE")
    if not flags.depth_size:
        fail(f"{what} needs --depth-size WxH")
    try:
        w, h = (int(v) for v in flags.depth_size.lower().split("x"))
    except ValueError:
        fail(f"--depth-size: want WxH, e.g. 1280x720, got {flags.depth_size!r}")
    if out_dir and flags.depth_encoding == "32FC1":
        fail("--depth-out writes 16-bit PNGs: it needs --depth-encoding 16UC1")
    kw = {k: v for k, v in (("encoding", flags.depth_encoding), ("scale", flags.depth_scale),
                            ("min_depth", flags.depth_min), ("splat", flags.depth_splat)) if v is not None}
    try:
        opts = DepthOptions(width=w, height=h, **kw)
        cal = cal if cal is not None else load_calibration(flags.calib)
    except (ValueError, OSError) as e:
        fail(f"{what}: {e}")
    return cal, opts


_SCAN_FLAGS = ("scan_angle", "scan_increment", "scan_height", "scan_range", "scan_no_inf", "scan_inf_epsilon",
               "scan_time", "scan_frame_id")


def add_scan_flags(p: argparse.ArgumentParser, topic_help: str) -> None:
    """--scan-topic and --scan-* (``ops/laser_scan.py``: ``pointcloud_to_laserscan``'s parameters).
    The option flags default to None so that one given without a topic is seen."""
    p.add_argument("--scan-topic", default="", metavar="TOPIC", help=topic_help)
    p.add_argument("--scan-angle", default=None, metavar="MIN,MAX",
                   help="the scan's first and last angle in radians, within [-pi, pi] (default the full circle); a pair "
                        "that starts with a minus sign is written with '=': --scan-angle=-1.57,1.57")
    p.add_argument("--scan-increment", type=float, default=None, metavar="RAD",
                   help="angle between two rays in radians (default pi/180; at most 4096 rays)")
    p.add_argument("--scan-height", default=None, metavar="MIN,MAX",
                   help="only points with z in this band, in metres in the cloud's frame, count (default -1,1; inf "
                        "allowed)")
    p.add_argument("--scan-range", default=None, metavar="MIN,MAX",
                   help="only returns within these ranges in metres count (default 0.45,100)")
    p.add_argument("--scan-no-inf", action="store_const", const=True, default=None,
                   help="a ray without a return reports range_max + --scan-inf-epsilon, not +inf")
    p.add_argument("--scan-inf-epsilon", type=float, default=None, metavar="M", help="(default 1.0)")
    p.add_argument("--scan-time", type=float, default=None, metavar="S",
                   help="the message's scan_time in seconds (default 1/30)")
    p.add_argument("--scan-frame-id", default=None, metavar="FRAME", help="frame_id of the scans (default: the cloud's)")


def scan_options(flags, error=None):
    """The ``ScanOptions`` of the --scan-* flags, None without --scan-topic.  A --scan-* flag
    without a topic, a pair that is no ``MIN,MAX`` and an option out of range are usage errors that
    name the flag: ``error`` (an ``ArgumentParser.error``) is called with the message, else
    ``ValueError`` is raised."""
    def fail(msg):
        if error is not None:
            error(msg)
        raise ValueError(msg)

    if not flags.scan_topic:
        given = [f for f in _SCAN_FLAGS if getattr(flags, f) is not None]
        if given:
            fail(f"--{given[0].replace('_', '-')} needs --scan-topic TOPIC")
        return None
    from ..ops.laser_scan import ScanOptions

    def pair(flag, text):
        try:
            lo, hi = (float(v) for v in text.split(","))
        except ValueError:
            fail(f"{flag}: want MIN,MAX, e.g. -1.57,1.57, got {text!r}")
        return lo, hi

    kw, flag_of = {}, {}
    for flag, names in (("--scan-angle", ("angle_min", "angle_max")), ("--scan-height", ("min_height", "max_height")),
                        ("--scan-range", ("range_min", "range_max"))):
        text = getattr(flags, flag[2:].replace("-", "_"))
        if text is not None:
            kw.update(zip(names, pair(flag, text)))
        flag_of.update({n: flag for n in names})
    for flag, name in (("--scan-increment", "angle_increment"), ("--scan-inf-epsilon", "inf_epsilon"),
                       ("--scan-time", "scan_time")):
        v = getattr(flags, flag[2:].replace("-", "_"))
        if v is not None:
            kw[name] = v
        flag_of[name] = flag
    if flags.scan_no_inf:
        kw["use_inf"] = False
    try:
        return ScanOptions(**kw)
    except ValueError as e:
        field = str(e).split()[0]
        fail(f"{flag_of.get(field, '--scan-topic')}: {e}")


_GROUND_FLAGS = (("ground_sectors", "sectors"), ("ground_cell", "cell"), ("ground_range", None),
                 ("ground_sensor_height", "sensor_height"), ("ground_slope", "max_slope"), ("ground_noise", "noise"),
                 ("ground_thickness", "thickness"), ("ground_max_height", "max_height"))


def add_ground_flags(p: argparse.ArgumentParser, obstacles_help: str, ground_help: str) -> None:
    """--obstacles-topic, --ground-topic and --ground-* (``ops/ground.py``).  The option flags
    default to None so that one given without a topic is seen."""
    p.add_argument("--obstacles-topic", default="", metavar="TOPIC", help=obstacles_help)
    p.add_argument("--ground-topic", default="", metavar="TOPIC", help=ground_help)
    p.add_argument("--ground-sectors", type=int, default=None, metavar="N",
                   help="angular sectors of the polar grid around z (default 360; 1..4096)")
    p.add_argument("--ground-cell", type=float, default=None, metavar="M",
                   help="radial width of a grid ring in metres (default 0.5; 0.05..10)")
    p.add_argument("--ground-range", default=None, metavar="MIN,MAX",
                   help="only points at these distances from the z axis, in metres, count (default 0,80; at most 512 "
                        "rings of --ground-cell)")
    p.add_argument("--ground-sensor-height", type=float, default=None, metavar="M",
                   help="the ground is expected at z = -M under the sensor (default 1.8)")
    p.add_argument("--ground-slope", type=float, default=None, metavar="DEG",
                   help="slope the ground may take from ring to ring, in degrees (default 10; 0..45)")
    p.add_argument("--ground-noise", type=float, default=None, metavar="M",
                   help="allowance for measurement noise in metres (default 0.05)")
    p.add_argument("--ground-thickness", type=float, default=None, metavar="M",
                   help="how far above the ground estimate a point is still ground (default 0.2)")
    p.add_argument("--ground-max-height", type=float, default=None, metavar="M",
                   help="points higher above the ground than this are dropped (default inf)")


def ground_options(flags, error=None):
    """The ``GroundOptions`` of the --ground-* flags, None without --obstacles-topic and
    --ground-topic.  A --ground-* flag without either topic, a range that is no ``MIN,MAX`` and an
    option out of range are usage errors that name the flag: ``error`` (an
    ``ArgumentParser.error``) is called with the message, else ``ValueError`` is raised."""
    def fail(msg):
        if error is not None:
            error(msg)
        raise ValueError(msg)

    def flag(attr):
        return "--" + attr.replace("_", "-")

    if not (flags.obstacles_topic or flags.ground_topic):
        given = [a for a, _ in _GROUND_FLAGS if getattr(flags, a) is not None]
        if given:
            fail(f"{flag(given[0])} needs --obstacles-topic TOPIC or --ground-topic TOPIC")
        return None
    from ..ops.ground import GroundOptions

    kw, flag_of = {}, {"range_min": "--ground-range", "range_max": "--ground-range"}
    for attr, name in _GROUND_FLAGS:
        v = getattr(flags, attr)
        if name is None:
            if v is not None:
                try:
                    kw["range_min"], kw["range_max"] = (float(t) for t in v.split(","))
                except ValueError:
                    fail(f"--ground-range: want MIN,MAX, e.g. 2,60, got {v!r}")
            continue
        flag_of[name] = flag(attr)
        if v is not None:
            kw[name] = v
    try:
        return GroundOptions(**kw)
    except ValueError as e:
        fail(f"{flag_of.get(str(e).split()[0], '--ground-topic')}: {e}")


def bev_view(engine, res: float, enabled):
    """The ``BevView`` of the --bev-* flags: the engine's point-cloud range (the KITTI
    range for an engine that does not know its model's) at ``res`` metres per pixel; None
    when the flag that turns the picture on is empty."""
    if not enabled:
        return None
    from ..utils.bev import BevView

    cfg = getattr(engine, "cfg", None)
    if getattr(cfg, "voxel", None) is not None:
        return BevView.for_model(cfg, res)
    d = BevView()
    return BevView(d.x_range, d.y_range, float(res), d.z_range)


def play_bag(path: str, bus, topics=None, rate: Optional[float] = None, shutdown: bool = True):
    """rosbag-play equivalent onto the in-process bus (background thread)."""
    import threading
    import time

    from ..ros.bag import Bag

    def run():
        t_prev = None
        with Bag(path) as bag:
            for topic, msg, t in bag.read_messages(topics=topics):
                if rate and t_prev is not None:
                    time.sleep(max(0.0, (t.to_sec() - t_prev) / rate))
                t_prev = t.to_sec()
                bus.publish(topic, msg)
        bus.wait_idle(600)
        if shutdown:
            bus.shutdown_event.set()

    th = threading.Thread(target=run, daemon=True, name="bag-play")
    th.start()
    return th


def image_files(d: str):
    exts = (".png", ".jpg", ".jpeg", ".bmp")
    return sorted(os.path.join(d, f) for f in os.listdir(d) if f.lower().endswith(exts))
