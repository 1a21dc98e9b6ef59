"""Live-driver GPU bench: the reference's actual loop, message in -> message published.

The reference's product is the subscriber callback: CompressedImage -> decode ->
preprocess -> ModelInfer -> NMS -> draw -> publish ``Image``
(``communicator/ros_inference.py:117-175``), and PointCloud2 -> ``read_points`` ->
voxelise -> ModelInfer -> filter -> jsk ``BoundingBoxArray`` -> publish
(``communicator/ros_inference3d.py:120-213``).  ``bench.py`` times the device step
from raw pinned bytes to device detections; this tool times the drivers
(:class:`RosInference` / :class:`RosInference3D`) with the local GPU engines over
the in-process topic bus, including JPEG decode, micro-batching, the ordered
re-publisher, GPU annotation and building the published messages.

    python tools/driver_bench.py [--camera N] [--lidar N] [--batch B] [--workers W] [--gpus N]

``--gpus N`` (N > 1) runs the drivers data-parallel the way ``torchrun main.py
--engine local`` does (``parallel/ring_dp.py``): rank 0 subscribes and publishes, the
node batch goes through the shared host ring, every rank decodes / detects its shard
on its own GPU.  Launched without torchrun it starts ``torch.distributed.run`` as a
child process; ``TCA_DIST_BACKEND=gloo`` rehearses N ranks on one GPU.

Messages are published paced so the latest-wins windows never drop (every
message is detected and published); throughput = messages / wall time from the
first publish to the last published result.  Prints one JSON line.
"""
import argparse
import io
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, ".")


class _Stages:
    """ClientMetrics stand-in: per-stage sums (StageTimer calls .stage / .frame)."""

    def __init__(self):
        self.sum, self.n, self.lock = {}, {}, threading.Lock()

    def stage(self, name, seconds):
        with self.lock:
            self.sum[name] = self.sum.get(name, 0.0) + seconds
            self.n[name] = self.n.get(name, 0) + 1

    def frame(self, n=1):
        pass

    def bytes(self, n):
        pass

    def summary(self):
        return {k: {"calls": self.n[k], "ms_per_call": round(1e3 * v / self.n[k], 3)} for k, v in self.sum.items()}


def _run(bus, pub_topic, out_topic, out_type, messages, window, timeout, published=None, side=None):
    """published: a list that receives the payload bytes of every output message.  side: (topic,
    messages) published one by one, each just before the input message of the same index."""
    from triton_client_amd.ros import compat

    got = []
    done = threading.Event()

    def on_out(m):
        got.append(time.perf_counter())
        if published is not None:
            published.append(len(m.data))
        if len(got) >= len(messages):
            done.set()
    sub = compat.Subscriber(out_topic, out_type, on_out, bus=bus)
    pub = compat.Publisher(pub_topic, type(messages[0]), bus=bus)
    side_pub = compat.Publisher(side[0], type(side[1][0]), bus=bus) if side else None
    t0 = time.perf_counter()
    for i, m in enumerate(messages):
        while i - len(got) >= window:  # pace: never more than `window` messages in flight
            time.sleep(0.0002)
        if side_pub is not None:
            side_pub.publish(side[1][i])
        pub.publish(m)
    ok = done.wait(timeout)
    t1 = time.perf_counter()
    sub.unregister()
    return len(got), (t1 - t0), ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--camera", type=int, default=512, help="CompressedImage messages (0: skip)")
    ap.add_argument("--camera-encoding", default=None, metavar="NAME",
                    help="publish raw sensor_msgs/Image messages in this encoding (rgb8, bgr8, rgba8, bgra8, mono8, "
                         "mono16, yuv422, yuv422_yuy2, bayer_rggb8, ...) instead of JPEG CompressedImage")
    ap.add_argument("--compressed-out", action="store_true",
                    help="camera side: publish the annotated frame as a JPEG CompressedImage on <pub_topic>/compressed "
                         "(RosInference compressed=; encoded on the GPU) instead of the raw Image")
    ap.add_argument("--jpeg-quality", type=int, default=90)
    ap.add_argument("--jpeg-subsampling", default="4:2:0", choices=["4:2:0", "4:2:2", "4:4:4"])
    ap.add_argument("--camera-tracks", action="store_true",
                    help="camera side: also track the detections and publish them with their track ids "
                         "(RosInference tracks_topic; the frames are stamped 1/30 s apart)")
    ap.add_argument("--rectify", action="store_true",
                    help="camera side: rectify every frame under a synthetic barrel-distortion camera model of the "
                         "frame's size (RosInference rectify=; on the GPU unless TCA_DEVICE_RECTIFY=0)")
    ap.add_argument("--lidar", type=int, default=512, help="PointCloud2 messages (0: skip)")
    ap.add_argument("--bev", action="store_true",
                    help="LiDAR side: also publish the bird's-eye-view Image of every cloud (RosInference3D bev_topic)")
    ap.add_argument("--points", action="store_true",
                    help="LiDAR side: also publish every cloud with its per-point labels (RosInference3D points_topic)")
    ap.add_argument("--tracks", action="store_true",
                    help="LiDAR side: also track the detections and publish the boxes with their track ids "
                         "(RosInference3D tracks_topic; the clouds are stamped 0.1 s apart)")
    ap.add_argument("--ranged", action="store_true",
                    help="LiDAR side: also range 64 synthetic camera detections per cloud, stamped like the cloud, "
                         "under a fixed KITTI-like calibration (RosInference3D ranged_topic)")
    ap.add_argument("--depth", action="store_true",
                    help="LiDAR side: also publish every cloud as a 16UC1 depth Image of --depth-size pixels under a "
                         "fixed KITTI-like calibration rescaled to that size (RosInference3D depth_topic)")
    ap.add_argument("--depth-size", default="1280x720", metavar="WxH")
    ap.add_argument("--scan", action="store_true",
                    help="LiDAR side: also publish every cloud as a LaserScan of --scan-bins rays over the full circle, "
                         "the other options at their defaults (RosInference3D scan_topic)")
    ap.add_argument("--scan-bins", type=int, default=360, metavar="N")
    ap.add_argument("--ground", action="store_true",
                    help="LiDAR side: also publish every cloud's obstacle and ground clouds, the sensor height the "
                         "synthetic sweep's and the other options at their defaults (RosInference3D obstacles_topic and "
                         "ground_topic)")
    ap.add_argument("--ground-only", choices=("obstacles", "ground"), default=None,
                    help="--ground: publish this one of the two clouds alone")
    ap.add_argument("--ground-copy", choices=("slab", "counted"), default=None,
                    help="how --ground copies the split clouds back (default: the splitter's own)")
    ap.add_argument("--ground-recompute", action="store_true",
                    help="--ground: the scatter computes the classes again instead of reading the saved ones")
    ap.add_argument("--batch", type=int, default=32, help="micro-batch per engine call")
    ap.add_argument("--workers", type=int, default=2, help="driver worker threads (host || device overlap)")
    ap.add_argument("--hw", default="720,1280")
    ap.add_argument("--timeout", type=float, default=240.0)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--gpus", type=int, default=1, help="data-parallel ranks (one process per GPU)")
    ap.add_argument("--engine", choices=["local", "remote"], default="local",
                    help="remote: the reference's architecture -- the drivers are KServe clients (RemoteDetector2D / "
                         "3D with their HIP pre/post on this GPU, main.py's default) of a server process started here "
                         "with YOLOv5nCOCO + pointpillar_kitti on the same GPU")
    ap.add_argument("--mode", choices=["sync", "async"], default="sync",
                    help="remote: RPC mode (sync = the reference's blocking ModelInfer; async = -a)")
    ap.add_argument("--wire", choices=["raw", "proto", "shm", "devshm"], default="raw",
                    help="remote: request codec / transport (shm, devshm: shared-memory regions, server on this node)")
    a = ap.parse_args()
    if a.depth and a.ranged:
        ap.error("--depth rescales the calibration that --ranged uses as it is: run them apart")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:  # self-launch (a child: nothing has touched the GPU)
        import socket
        import subprocess
        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
        sk.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
               "--master-addr=127.0.0.1", f"--master-port={port}", __file__] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))

    import torch
    from PIL import Image

    from triton_client_amd.inference.engines import LocalDetector2D, LocalDetector3D
    from triton_client_amd.inference.ros_inference import RosInference
    from triton_client_amd.inference.ros_inference3d import RosInference3D
    from triton_client_amd.ros import compat, msgs
    from triton_client_amd.ros.bus import TopicBus
    from triton_client_amd.utils.synthetic import LidarSpec, camera_frame, lidar_sweep

    from triton_client_amd.cli.engines import maybe_data_parallel

    H, W = (int(v) for v in a.hw.split(","))
    if a.engine == "remote":
        return _remote(a, H, W)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.device == "cuda" and world > 1:
        a.device = f"cuda:{int(os.environ.get('LOCAL_RANK', '0')) % max(1, torch.cuda.device_count())}"
    os.environ.setdefault("TCA_DP_HEARTBEAT", "0")
    # every rank builds both engines (and their DP wrappers) in the same order
    eng2, info = maybe_data_parallel(LocalDetector2D(batch=a.batch, device=a.device, letterbox=True)) \
        if a.camera else (None, None)
    eng3, info3 = maybe_data_parallel(LocalDetector3D(batch=a.batch, device=a.device), three_d=True) \
        if a.lidar else (None, None)
    info = info or info3
    if info is not None and not info.is_main:  # worker rank: serve shards until rank 0 is done
        for e in (eng2, eng3):
            if e is not None:
                e.serve()
        from triton_client_amd.parallel.dp import shutdown
        shutdown(info)
        return
    out = {"tool": "driver_bench", "batch": a.batch, "workers": a.workers, "gpus": world,
           "device": torch.cuda.get_device_name(0) if a.device.startswith("cuda") else a.device}
    bus = TopicBus()
    window = 2 * a.batch * a.workers
    if a.camera:
        # header.seq strictly increasing over warm-up + run: the re-publisher drops a seq that is
        # not newer than the last one it published
        warm = 2 * a.batch
        msgs_in = _camera_messages(H, W, warm + a.camera, a.camera_encoding)
        st = _Stages()
        opts = None
        if a.compressed_out:
            from triton_client_amd.ops.jpeg_encode import JpegOptions
            opts = JpegOptions(quality=a.jpeg_quality, subsampling=a.jpeg_subsampling)
        drv = RosInference(engine=eng2, params={"sub_topic": "/cam", "pub_topic": "/cam_out"}, bus=bus,
                           batch=a.batch, workers=a.workers, metrics=st, queue_size=window, compressed=opts,
                           **({"rectify": _barrel_model(H, W)} if a.rectify else {}),
                           **({"tracks_topic": "/cam_tracks"} if a.camera_tracks else {}))
        drv.start_inference(spin=False)
        out_type = msgs.CompressedImage if opts is not None else msgs.Image
        _run(bus, "/cam", drv.out_topic, out_type, msgs_in[:warm], window, a.timeout)  # warm-up + graphs
        st.sum.clear(), st.n.clear()
        sizes = []
        n, dt, ok = _run(bus, "/cam", drv.out_topic, out_type, msgs_in[warm:], window, a.timeout, published=sizes)
        drv.stop()
        if info is not None:
            eng2.close()
        out["camera"] = {"messages": n, "complete": ok, "seconds": round(dt, 3), "msgs_per_s": round(n / dt, 1),
                         "input": _camera_input(H, W, a.camera_encoding),
                         "output": (f"annotated CompressedImage JPEG q{a.jpeg_quality} {a.jpeg_subsampling}"
                                    if opts is not None else "annotated Image") + " + Detection2DArray",
                         "published_bytes_per_frame": round(sum(sizes) / max(1, len(sizes))), "stages": st.summary()}
        if a.rectify:
            out["camera"]["output"] += f", rectified ({drv.rectifier().kind})"
            out["camera"]["rectifier"] = drv.rectifier().kind
        if a.camera_tracks:
            trk = drv.tracker()
            ts = trk.state()
            out["camera"]["output"] += f" + tracks ({trk.kind})"
            out["camera"]["tracker"] = trk.kind
            out["camera"]["tracks"] = {"frames": trk.frames, "ids_given": int(ts.next_id) - 1,
                                       "live": int((ts.id != 0).sum()), "overflow": int(ts.overflow)}
    if a.lidar:
        spec = LidarSpec(sensor_height=3.23)
        clouds = [compat.create_cloud_xyzi(np.frombuffer(lidar_sweep(spec, s).tobytes(), np.float32).reshape(-1, 4))
                  for s in range(8)]
        warm = 2 * a.batch
        msgs_in = []
        for i in range(warm + a.lidar):
            c = clouds[i % 8]
            msgs_in.append(msgs.PointCloud2(header=msgs.Header(seq=i + 1, stamp=msgs.Time(100 + i // 10, i % 10 * 10 ** 8),
                                                               frame_id="os"), height=c.height,
                                            width=c.width, fields=c.fields, is_bigendian=False,
                                            point_step=c.point_step, row_step=c.row_step, data=c.data,
                                            is_dense=True))
        st = _Stages()
        drv = RosInference3D(engine=eng3, params={"sub_topic": "/pc", "pub_topic": "/pc_out"}, bus=bus,
                             batch=a.batch, workers=a.workers, metrics=st, queue_size=window,
                             bev_topic="/pc_bev" if a.bev else None,
                             **({"points_topic": "/pc_points"} if a.points else {}),
                             **({"tracks_topic": "/pc_tracks"} if a.tracks else {}),
                             **({"ranged_topic": "/cam_ranged", "camera_detections_topic": "/cam_det",
                                 "calibration": _kitti_like_calibration()} if a.ranged else {}),
                             **(_depth_arguments(a) if a.depth else {}),
                             **(_scan_arguments(a) if a.scan else {}),
                             **({**{k + "_topic": "/pc_" + k for k in ("obstacles", "ground")
                                    if a.ground_only in (None, k)},
                                 "ground_options": {"sensor_height": spec.sensor_height}} if a.ground else {}))
        if a.ground:
            from triton_client_amd.inference.engines import Detector3D
            splitter = Detector3D.ground_splitter(eng3)
            splitter.copy_back = a.ground_copy or splitter.copy_back
            splitter.saved = not a.ground_recompute
        dets = _detection_messages(msgs_in) if a.ranged else None
        ranged = []
        rsub = compat.Subscriber("/cam_ranged", msgs.Detection2DArray, ranged.append, bus=bus) if a.ranged else None
        depth = []
        dsub = compat.Subscriber("/pc_depth", msgs.Image, lambda m: depth.append(len(m.data)), bus=bus) \
            if a.depth else None
        scans = []
        ssub = compat.Subscriber("/pc_scan", msgs.LaserScan, lambda m: scans.append(len(m.ranges)), bus=bus) \
            if a.scan else None
        split = {"/pc_obstacles": [], "/pc_ground": []}
        gsubs = [compat.Subscriber(t, msgs.PointCloud2, lambda m, t=t: split[t].append(m.width), bus=bus)
                 for t in split] if a.ground else []
        drv.start_inference(spin=False)
        _run(bus, "/pc", "/pc_out", msgs.BoundingBoxArray, msgs_in[:warm], window, a.timeout,
             side=("/cam_det", dets[:warm]) if dets else None)
        st.sum.clear(), st.n.clear()
        del ranged[:]
        del depth[:]
        del scans[:]
        for v in split.values():
            del v[:]
        n, dt, ok = _run(bus, "/pc", "/pc_out", msgs.BoundingBoxArray, msgs_in[warm:], window, a.timeout,
                         side=("/cam_det", dets[warm:]) if dets else None)
        drv.stop()
        if rsub is not None:
            rsub.unregister()
        if dsub is not None:
            dsub.unregister()
        if ssub is not None:
            ssub.unregister()
        for g in gsubs:
            g.unregister()
        if info is not None:
            eng3.close()
        out["lidar"] = {"messages": n, "complete": ok, "seconds": round(dt, 3), "msgs_per_s": round(n / dt, 1),
                        "input": f"PointCloud2 {clouds[0].width} points x {clouds[0].point_step} B",
                        "output": "jsk BoundingBoxArray (label 2, score > 0.5)", "stages": st.summary()}
        if a.bev:
            v = drv.bev_view
            from triton_client_amd.inference.engines import Detector3D
            painter = {"device": "tca_bev_render", "host": "host painter"}[Detector3D.bev_painter(eng3)]
            out["lidar"]["output"] += f" + bev Image {v.W}x{v.H} ({painter})"
            out["lidar"]["bev_painter"] = painter
        if a.points:
            out["lidar"]["output"] += " + labelled PointCloud2 (28 B per point)"
        if a.ranged:
            from triton_client_amd.inference.engines import Detector3D
            from triton_client_amd.ops.range2d import device_enabled
            kind = "tca_range2d" if Detector3D.ranger(eng3).gpu and device_enabled() else "host definition"
            got = sum(1 for m in ranged for d in m.detections if d.results[0].pose.position.z != 0.0)
            out["lidar"]["output"] += f" + ranged Detection2DArray ({kind})"
            out["lidar"]["ranger"] = kind
            out["lidar"]["ranged"] = {"messages": len(ranged), "detections": sum(len(m.detections) for m in ranged),
                                      "with_range": got}
        if a.depth:
            from triton_client_amd.inference.engines import Detector3D
            from triton_client_amd.ops.depth_image import device_enabled
            kind = "tca_depth_image" if Detector3D.depth_imager(eng3).gpu and device_enabled() else "host definition"
            o = drv.depth_options
            print(f"depth images: {kind}", file=sys.stderr)
            out["lidar"]["output"] += f" + depth Image {o.encoding} {o.width}x{o.height} ({kind})"
            out["lidar"]["depth_imager"] = kind
            out["lidar"]["depth"] = {"messages": len(depth), "bytes_per_image": round(sum(depth) / max(1, len(depth)))}
        if a.scan:
            from triton_client_amd.inference.engines import Detector3D
            from triton_client_amd.ops.laser_scan import device_enabled
            kind = "tca_laser_scan" if Detector3D.laser_scanner(eng3).gpu and device_enabled() else "host definition"
            print(f"laser scans: {kind}", file=sys.stderr)
            out["lidar"]["output"] += f" + LaserScan {drv.scan_options.n} rays ({kind})"
            out["lidar"]["laser_scanner"] = kind
            out["lidar"]["scan"] = {"messages": len(scans), "rays_per_scan": round(sum(scans) / max(1, len(scans)))}
        if a.ground:
            from triton_client_amd.ops.ground import device_enabled
            kind = "tca_ground_split" if splitter.gpu and device_enabled() else "host definition"
            print(f"ground split: {kind}", file=sys.stderr)
            out["lidar"]["output"] += f" + obstacle and ground PointCloud2 ({kind})"
            out["lidar"]["ground_splitter"] = kind
            out["lidar"]["ground"] = {"copy_back": splitter.copy_back, "saved_classes": splitter.saved,
                                      **{t[4:]: {"messages": len(v), "points_per_cloud": round(sum(v) / max(1, len(v)))}
                                         for t, v in split.items()}}
        if a.tracks:
            trk = drv.tracker()
            ts = trk.state()
            out["lidar"]["output"] += f" + tracks ({trk.kind})"
            out["lidar"]["tracker"] = trk.kind
            out["lidar"]["tracks"] = {"frames": trk.frames, "ids_given": int(ts.next_id) - 1,
                                      "live": int((ts.id != 0).sum()), "overflow": int(ts.overflow)}
    bus.close()
    print(json.dumps(out), flush=True)
    if info is not None:
        from triton_client_amd.parallel.dp import shutdown
        shutdown(info)


def _camera_input(H, W, encoding):
    return f"CompressedImage JPEG {W}x{H} q90" if encoding is None else f"Image {encoding} {W}x{H}"


def _camera_messages(H, W, n, encoding=None):
    """n camera messages over 8 synthetic frames, stamped 1/30 s apart: JPEG CompressedImage, or raw
    Image in ``encoding``."""
    from PIL import Image

    from triton_client_amd.ros import msgs
    from triton_client_amd.utils.synthetic import camera_frame

    def header(i):
        ns = i * 10 ** 9 // 30
        return msgs.Header(seq=i + 1, stamp=msgs.Time(100 + ns // 10 ** 9, ns % 10 ** 9), frame_id="cam")

    if encoding is not None:
        from triton_client_amd.ops.golden import image_packed_row, rgb8_to_encoding

        raws = [rgb8_to_encoding(camera_frame(H, W, s), encoding) for s in range(8)]
        return [msgs.Image(header=header(i), height=H, width=W, encoding=encoding,
                           is_bigendian=0, step=image_packed_row(W, encoding), data=raws[i % 8]) for i in range(n)]
    jpegs = []
    for s in range(8):
        buf = io.BytesIO()
        Image.fromarray(camera_frame(H, W, s)).save(buf, format="JPEG", quality=90)
        jpegs.append(buf.getvalue())
    return [msgs.CompressedImage(header=header(i), format="jpeg", data=jpegs[i % 8])
            for i in range(n)]


def _barrel_model(H, W):
    """A wide-angle lens of the frame's size: focal length 0.6 W, barrel distortion that moves the
    corners over a hundred pixels at 1280 x 720, a little tangential distortion."""
    from triton_client_amd.ops.rectify import CameraModel

    f = 0.6 * W
    K = [[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]]
    return CameraModel(width=W, height=H, K=K, D=[-0.28, 0.07, 0.0005, -0.0003, 0.0], model="plumb_bob")


def _kitti_like_calibration():
    """A fixed rig: KITTI's colour-camera projection, the LiDAR looking along the camera's axis
    from 8 cm above and 27 cm behind it."""
    from triton_client_amd.ops.range2d import Calibration

    P = [[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]]
    T = [[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, -0.08], [1.0, 0.0, 0.0, -0.27], [0.0, 0.0, 0.0, 1.0]]
    return Calibration(np.array(P), np.array(T))


def _depth_arguments(a):
    """The driver's depth arguments: the KITTI-like rig with its 1242 x 375 projection rescaled to
    --depth-size, the default options."""
    from triton_client_amd.ops.depth_image import DepthOptions
    from triton_client_amd.ops.range2d import Calibration

    w, h = (int(v) for v in a.depth_size.lower().split("x"))
    cal = _kitti_like_calibration()
    P = np.diag([w / 1242.0, h / 375.0, 1.0]) @ cal.P
    return {"depth_topic": "/pc_depth", "depth_options": DepthOptions(w, h), "calibration": Calibration(P, cal.T)}


def _scan_arguments(a):
    """The driver's scan arguments: --scan-bins rays over the full circle, the default options."""
    import math

    from triton_client_amd.ops.laser_scan import ScanOptions

    return {"scan_topic": "/pc_scan", "scan_options": ScanOptions(angle_increment=2 * math.pi / a.scan_bins)}


def _detection_messages(clouds, per_cloud=64):
    """One Detection2DArray per cloud, stamped like it: ``per_cloud`` seeded boxes on a 1242 x 375 image."""
    from triton_client_amd.ros import msgs

    out = []
    for i, c in enumerate(clouds):
        rng = np.random.default_rng(i % 8)
        box = np.stack([rng.uniform(0, 1242, per_cloud), rng.uniform(120, 375, per_cloud),
                        rng.uniform(20, 300, per_cloud), rng.uniform(20, 200, per_cloud)], 1)
        dets = [msgs.Detection2D(results=[msgs.ObjectHypothesisWithPose(id=1 + k % 3, score=0.9)],
                                 bbox=msgs.BoundingBox2D(msgs.Pose2D(float(b[0]), float(b[1])), float(b[2]), float(b[3])))
                for k, b in enumerate(box)]
        out.append(msgs.Detection2DArray(header=msgs.Header(seq=c.header.seq, stamp=c.header.stamp, frame_id="cam"),
                                         detections=dets))
    return out


def _cloud_messages(n):
    from triton_client_amd.ros import compat, msgs
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep

    spec = LidarSpec(sensor_height=3.23)
    clouds = [compat.create_cloud_xyzi(np.frombuffer(lidar_sweep(spec, s).tobytes(), np.float32).reshape(-1, 4))
              for s in range(8)]
    out = []
    for i in range(n):
        c = clouds[i % 8]
        out.append(msgs.PointCloud2(header=msgs.Header(seq=i + 1, frame_id="os"), height=c.height, width=c.width,
                                    fields=c.fields, is_bigendian=False, point_step=c.point_step, row_step=c.row_step,
                                    data=c.data, is_dense=True))
    return out


def _remote(a, H, W):
    """--engine remote: a KServe server process on this GPU; the drivers as its clients
    (RemoteDetector2D / RemoteDetector3D on the GPU: main.py / main3d.py's default path)."""
    import socket
    import subprocess
    from types import SimpleNamespace

    import torch

    from triton_client_amd.channel.grpc_channel import GRPCChannel
    from triton_client_amd.clients import client_for_model
    from triton_client_amd.inference.engines import RemoteDetector2D, RemoteDetector3D
    from triton_client_amd.inference.ros_inference import RosInference
    from triton_client_amd.inference.ros_inference3d import RosInference3D
    from triton_client_amd.ros import msgs
    from triton_client_amd.ros.bus import TopicBus

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    target = f"127.0.0.1:{port}"
    proc = subprocess.Popen([sys.executable, "-m", "triton_client_amd.server", "--host", "127.0.0.1", "--port",
                             str(port), "--metrics-port", "0", "--models", "YOLOv5nCOCO,pointpillar_kitti"])
    out = {"tool": "driver_bench", "engine": "remote", "mode": a.mode, "wire": a.wire, "batch": a.batch,
           "workers": a.workers, "device": torch.cuda.get_device_name(0) if a.device.startswith("cuda") else a.device,
           "server": "separate process, same GPU: YOLOv5nCOCO + pointpillar_kitti (fp32)"}
    try:
        def channel(model):
            f = SimpleNamespace(model_name=model, model_version="", batch_size=1, verbose=False)
            return GRPCChannel({"grpc_channel": target}, f, wait_ready_s=600.0)

        bus = TopicBus()
        window = 2 * a.batch * a.workers
        if a.camera:
            ch = channel("YOLOv5nCOCO")
            cr = ch.get_metadata()["config_response"]
            client = client_for_model("YOLOv5nCOCO", getattr(cr, "config", cr), a.device)
            eng = RemoteDetector2D(ch, client, letterbox=False, conf_thres=0.3, mode=a.mode, wire=a.wire,
                                   device=a.device)
            warm = 2 * a.batch
            ms = _camera_messages(H, W, warm + a.camera, a.camera_encoding)
            st = _Stages()
            drv = RosInference(None, client, engine=eng, params={"sub_topic": "/cam", "pub_topic": "/cam_out"},
                               bus=bus, batch=a.batch, workers=a.workers, metrics=st, queue_size=window)
            drv.start_inference(spin=False)
            _run(bus, "/cam", "/cam_out", msgs.Image, ms[:warm], window, a.timeout)
            st.sum.clear(), st.n.clear()
            n, dt, ok = _run(bus, "/cam", "/cam_out", msgs.Image, ms[warm:], window, a.timeout)
            drv.stop()
            live = eng.live()
            eng.release_transport()
            out["camera"] = {"messages": n, "complete": ok, "seconds": round(dt, 3), "msgs_per_s": round(n / dt, 1),
                             "device_path": live is not None and live.stats["frames"] > 0,
                             "input": _camera_input(H, W, a.camera_encoding),
                             "output": "annotated Image + Detection2DArray", "stages": st.summary()}
            ch.close()
        if a.lidar:
            ch = channel("pointpillar_kitti")
            cr = ch.get_metadata()["config_response"]
            client = client_for_model("pointpillar_kitti", getattr(cr, "config", cr), a.device)
            eng = RemoteDetector3D(ch, client, z_offset=1.5, mode=a.mode, wire=a.wire, device=a.device)
            warm = 2 * a.batch
            ms = _cloud_messages(warm + a.lidar)
            st = _Stages()
            drv = RosInference3D(None, client, engine=eng, params={"sub_topic": "/pc", "pub_topic": "/pc_out"},
                                 bus=bus, batch=a.batch, workers=a.workers, metrics=st, queue_size=window)
            drv.start_inference(spin=False)
            _run(bus, "/pc", "/pc_out", msgs.BoundingBoxArray, ms[:warm], window, a.timeout)
            st.sum.clear(), st.n.clear()
            n, dt, ok = _run(bus, "/pc", "/pc_out", msgs.BoundingBoxArray, ms[warm:], window, a.timeout)
            drv.stop()
            eng.release_transport()
            out["lidar"] = {"messages": n, "complete": ok, "seconds": round(dt, 3), "msgs_per_s": round(n / dt, 1),
                            "device_voxeliser": str(getattr(eng.pre, "device", "cpu")),
                            "input": f"PointCloud2 {ms[0].width} points x {ms[0].point_step} B",
                            "output": "jsk BoundingBoxArray (label 2, score > 0.5)", "stages": st.summary()}
            ch.close()
        bus.close()
        print(json.dumps(out), flush=True)
    finally:
        proc.terminate()
        try:
            proc.wait(60)
        except subprocess.TimeoutExpired:
            proc.kill()


if __name__ == "__main__":
    main()
