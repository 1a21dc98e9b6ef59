#!/usr/bin/env python3
"""End-to-end sensor → detection throughput, YOLOv5n-640 + PointPillars, 1..8 MI355X.

Metric (BASELINE.json): "end-to-end FPS (sensor->detection) YOLOv5n-640 +
PointPillars at 1/2/4/8 GPU".  One *frame* = one camera image (uint8 RGB,
default 1280x720) AND one LiDAR sweep (PointCloud2 payload, 64 beams x 1875
columns ≈ 120k points x 16 B) turned into 2D detections (YOLOv5n @640,
letterbox, conf 0.3 / IoU 0.45 / max_det 300 — reference
``communicator/ros_inference.py:148``) and 3D boxes (PointPillars KITTI, score 0.1,
rotated NMS 0.01, 4096 → 500 — ``data/pointpillar.yaml:130-142``).

Each timed step, on every rank: B new frames enter from pinned host memory
(``--ingest local``: each GPU over its own PCIe link; ``--ingest rccl``: all
through rank 0, then a grouped RCCL scatter over xGMI), the captured
camera + LiDAR hipGraph runs, and the detections of all ranks are gathered to
rank 0 over RCCL and copied to its host.  Weak scaling: B frames per GPU per
step.  Data: synthetic sensors, random-init weights (no datasets/checkpoints
reachable); compute precision per ``--precision`` below (fp32 by default).

Launch: ``python bench.py`` (1 GPU), ``python bench.py --gpus N`` (the script
starts N rank processes itself, before any GPU call) or ``torchrun
--nproc-per-node N bench.py --gpus N``.  The run fails — it never silently
measures fewer GPUs — when the ranks that come up, the visible devices or the
ranks RCCL built its communicator over differ from ``--gpus``.

Precision: ``--precision fp32`` (default) is the reference's serving precision
(``examples/YOLOv5/config.pbtxt:7,16``, ``examples/pointpillar_kitti/config.pbtxt:33,54``
TYPE_FP32): fp32 activations, split-product MFMA convs, detection parity with
the fp32 models gated in ``tests/test_fp32_mode_gpu.py``.  ``--precision bf16``
is a secondary, labelled number.

A plain run sets up, warms up, times ``--steps`` steps and prints the result line.
``--dump-outputs DIR`` also writes the last timed step's detections as ``DIR/*.npy``
(the same arrays in every run with the same arguments); ``--full`` adds the secondary
measurements that take runs of their own after the timed steps.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from triton_client_amd.parallel.dp import (FrameExchange, allreduce_max, barrier, init_distributed,  # noqa: E402
                                           shutdown)

METRIC = "end-to-end FPS (sensor->detection) YOLOv5n-640 + PointPillars at 1/2/4/8 GPU"
# Reference-equivalent FPS: tools/reference_equivalent.py on an MI355X box (the
# reference client's per-frame logic — batch 1, sync KServe RPC, struct-loop
# response decode, Python read_points — for the same camera + LiDAR frame pair,
# models served on the same GPU).  profiles/reference_equivalent_r1.json, BASELINE.md.
REFERENCE_EQUIVALENT_FPS = 3.2319


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32, help="frames per GPU per step (32: +11%% frames/s over 16 at 5.8 ms per step, profiles/batch_sweep_r1.md)")
    ap.add_argument("--cam", default="720x1280", help="camera HxW")
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--columns", type=int, default=1875)
    ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic frames per rank")
    ap.add_argument("--ingest", choices=["local", "rccl"], default="local")
    ap.add_argument("--comm", choices=["torch", "native"], default="native",
                    help="DP scatter/gather: the C++ RCCL communicator (default) or torch batch_isend_irecv")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-prefetch", action="store_true", help="serial H2D ingest (no copy-stream prefetch)")
    ap.add_argument("--unfused-detect", action="store_true",
                    help="YOLOv5 Detect convs + tca_yolo_decode_filter instead of the fused kernel "
                         "(models/fast.py DETECT_FUSED; A/B)")
    ap.add_argument("--dense-bev", action="store_true",
                    help="PointPillars first block without uniform-tile skipping (models/fast.py BEV_UNIFORM; A/B)")
    ap.add_argument("--lidar-pipeline", type=int, default=5, choices=[0, 1, 2, 3, 4, 5],
                    help="LiDAR software pipeline over two LidarPipelines sharing one model (double-buffered "
                         "graphs only; every step still runs one full batch through every stage, results come "
                         "out one step later). 0: off. 1: network + NMS of batch t beside preprocessing of "
                         "batch t+1. 2: preprocessing + network of batch t beside decode + NMS of batch t-1. "
                         "3: preprocessing + down blocks of batch t beside the fused neck + head + "
                         "decode + NMS of batch t-1 (7.27-7.44 vs 8.0 ms per step off; profiles/r3/lpipe/). "
                         "4: as 3 with the last down block in the back half too (bit-identical; 3241-3267 vs "
                         "4699-4792 frame pairs/s: its convs starve the camera, profiles/r5/split4/). 5 "
                         "(default since round 6): the down blocks of batch t alone beside the fused neck + head + "
                         "decode + NMS of batch t-1 and then the preprocessing (unpack, voxeliser, PillarVFE) of "
                         "batch t+1: the front leaves the critical stream, +0.9%% over 3 on two boxes "
                         "(profiles/r6/knobs/); detections come out two steps after ingest")
    ap.add_argument("--single-input-set", action="store_true",
                    help="one set of graph inputs (prefetch into landing buffers + a D2D copy per step) instead "
                         "of two captured graphs alternating over two input sets")
    ap.add_argument("--serial", action="store_true", help="camera and LiDAR branches on one stream")
    ap.add_argument("--graph-mode", choices=["split", "fork"], default="fork",
                    help="split: one hipGraph per branch, replayed on two streams; fork: one graph with two "
                         "forked branches")
    ap.add_argument("--lidar-priority", type=int, default=0, help="1: LiDAR branch on a high-priority stream")
    ap.add_argument("--only", choices=["both", "camera", "lidar"], default="both")
    ap.add_argument("--camera-model", choices=["yolov5n", "yolov4", "retinanet", "fcos"], default="yolov5n",
                    help="2D detector: YOLOv5n-640 (headline) or Detectron2 RetinaNet / FCOS R50-FPN at 800x1344")
    ap.add_argument("--lidar-model", choices=["pointpillars", "centerpoint", "second_iou"], default="pointpillars",
                    help="3D detector: PointPillars KITTI (headline), CenterPoint-PP nuScenes or SECOND-IoU KITTI "
                         "(sparse 3D conv backbone + RoI head)")
    ap.add_argument("--sweeps", type=int, default=1,
                    help="CenterPoint: LiDAR sweeps merged per frame (det3d nuScenes '10sweep': 10; device ring, "
                         "time lag as the 5th point feature)")
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32",
                    help="fp32 (default): the reference's serving precision — fp32 activations, split-product "
                         "MFMA convs; bf16: bf16 activations (secondary, labelled)")
    ap.add_argument("--camera-input", choices=["raw", "jpeg"], default="raw",
                    help="raw: uint8 RGB frames (sensor_msgs/Image); jpeg: CompressedImage JPEGs decoded every step "
                         "(C++ Huffman decode into pinned staging on --decode-threads host threads, overlapped with "
                         "the previous step's GPU work; IDCT + upsample + colour on the GPU)")
    ap.add_argument("--decode-threads", type=int, default=16, help="host threads of the JPEG entropy decoder")
    ap.add_argument("--jpeg-quality", type=int, default=90)
    ap.add_argument("--check-launch", action="store_true",
                    help="launch/rendezvous check only: every rank joins, the ranks are counted with an all-reduce, "
                         "rank 0 prints them (no GPU work; used by the CPU tests with TCA_DIST_BACKEND=gloo)")
    ap.add_argument("--json-out", default=None)
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the detections of the last timed step as they reach rank 0's "
                         "host (what a caller of the step receives) to DIR/<branch>_<box|score|cls|count>.npy in "
                         "float32, rows past each frame's count zeroed; the inputs are seeded, so two builds run "
                         "with the same arguments can be compared output for output")
    ap.add_argument("--full", action="store_true",
                    help="also take the secondary measurements that need runs of their own after the timed steps: "
                         "the DP gather / scatter alone (config.dp_comm_us_per_step, N > 1) and the GPU half of the "
                         "JPEG decode alone (config.jpeg.gpu_idct_color_us_per_frame, --camera-input jpeg); a plain "
                         "run times the steps and nothing else")
    ap.add_argument("--target-2d", type=float, default=100.0, help="candidates/frame reaching 2D NMS (calibration)")
    ap.add_argument("--target-3d", type=float, default=2000.0, help="anchors/frame reaching 3D NMS (calibration)")
    return ap.parse_args()


def _free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(n: int) -> int:
    """``--gpus N`` without a launcher: start N rank processes (RANK /
    LOCAL_RANK / WORLD_SIZE / MASTER_* set, rendezvous on 127.0.0.1) and
    return the worst exit code.  Runs before anything initialises the GPU in
    this process (spawned children, never an exec)."""
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), TCA_SELF_LAUNCHED="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    try:
        for p in procs:
            code = p.wait()
            if code != 0 and rc == 0:
                rc = code
                for q in procs:  # one rank failed: the others would block in a collective
                    if q.poll() is None:
                        q.terminate()
    finally:
        for q in procs:
            if q.poll() is None:
                q.kill()
    return rc


class _Split:
    """--graph-mode split: one step graph per branch, replayed on two streams."""

    def __init__(self, fn):
        self.fn = fn

    def __call__(self):
        return self.fn()


@contextlib.contextmanager
def _reproducible_calibration():
    """The head calibration runs the PyTorch modules once, before the steps.  Through MIOpen the
    convolution algorithm, and with it the rounding of the calibrated weights, follows the tuning
    records MIOpen keeps per user between runs: two runs with the same arguments gave camera scores
    3.5e-5 apart.  PyTorch's own convolutions without atomic accumulation give every run the same
    weights, so the timed path gets the same inputs and ``--dump-outputs`` the same arrays."""
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        with torch.backends.cudnn.flags(enabled=False):  # the switch that also governs MIOpen
            yield
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path: str, per_rank, branches) -> dict:
    """``--dump-outputs``: the last timed step's detections on rank 0's host (``per_rank[r]``: the flat
    ``outputs()`` list of rank r, four tensors per branch) as ``<branch>_<box|score|cls|count>.npy``,
    float32 (class ids and counts are small integers: exact), the ranks' frames concatenated in rank
    order.  Rows past a frame's count are not results (the buffers keep earlier steps' rows there) and
    are written as zeros.  Above ``DUMP_LIMIT_BYTES`` in all, a fixed seeded sample of the frames is
    written and ``frames.npy`` names them."""
    arrays = {}
    for j, br in enumerate(branches):
        box, score, cls, count = (np.concatenate([np.asarray(per_rank[r][4 * j + i].numpy(), dtype=np.float32)
                                                  for r in range(len(per_rank))]) for i in range(4))
        if count.ndim == 1 and score.ndim == 2 and score.shape[0] == count.shape[0]:
            live = np.arange(score.shape[1])[None, :] < count[:, None]
            box, score, cls = np.where(live[..., None], box, 0), np.where(live, score, 0), np.where(live, cls, 0)
        arrays.update({f"{br}_box": box, f"{br}_score": score, f"{br}_cls": cls, f"{br}_count": count})
    total = sum(a.nbytes for a in arrays.values())
    frames = min(a.shape[0] for a in arrays.values())
    if total > DUMP_LIMIT_BYTES and all(a.shape[0] == frames for a in arrays.values()):
        keep = max(1, int(frames * DUMP_LIMIT_BYTES // total) - 1)
        pick = np.sort(np.random.default_rng(0).choice(frames, keep, replace=False))
        arrays = {k: a[pick] for k, a in arrays.items()}
        arrays["frames"] = pick.astype(np.float32)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), np.ascontiguousarray(a, dtype=np.float32))
    return {"dir": path, "arrays": sorted(arrays), "bytes": total}


def _preflight(info, dev, rccl_ranks: int, comm_used: str) -> dict:
    """Before the first step on N GPUs: every rank's peer access to every other visible GPU
    (``hipDeviceCanAccessPeer``: RCCL's xGMI p2p path), the communicator's rank count, and
    every rank's NUMA placement (``parallel/numa.py`` describe + the CPUs it runs on), gathered
    to rank 0 and printed into the result's ``config``."""
    from triton_client_amd.parallel import numa

    n = torch.cuda.device_count()
    me = dev.index if dev.index is not None else 0
    peers = {j: bool(torch.cuda.can_device_access_peer(me, j)) for j in range(n) if j != me}
    d = numa.describe(info.local_rank)
    mine = {"rank": info.rank, "device": me, "gpu_pci": d["gpu_pci"], "numa_node": d["numa_node"],
            "cpus_allowed": len(os.sched_getaffinity(0)), "gpu_local_cpus": d["local_cpus"],
            "binding": d["reason"], "peer_access": peers}
    every = [mine]
    if info.world > 1:
        import torch.distributed as dist
        every = [None] * info.world
        dist.all_gather_object(every, mine)
    ranks_dev = sorted({e["device"] for e in every})
    pairs = [(e["device"], j) for e in every for j in ranks_dev if j != e["device"]]
    ok = all(e["peer_access"].get(j, False) for e in every for j in ranks_dev if j != e["device"])
    return {"ranks": every, "peer_pairs_checked": len(pairs), "peer_access_all_pairs": ok if pairs else None,
            "rccl_comm_ranks": rccl_ranks, "comm": comm_used}


def main():
    args = parse()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args.gpus))
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if world_env != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started {world_env} rank(s): refusing to report a "
                         f"number under the wrong GPU count")
    gloo_rehearsal = os.environ.get("TCA_DIST_BACKEND") == "gloo"
    if args.gpus > 1 and not gloo_rehearsal and torch.cuda.device_count() < args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but only {torch.cuda.device_count()} GPU(s) are visible")
    info = init_distributed()
    dev = info.device
    if info.world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but {info.world} ranks joined the process group")
    if args.check_launch:
        import torch.distributed as dist
        seen = torch.zeros(args.gpus, dtype=torch.int64)
        seen[info.rank] = 1
        if info.world > 1:
            dist.all_reduce(seen)
        if info.is_main:
            print(json.dumps({"check_launch": True, "world": info.world, "ranks_seen": int(seen.sum()),
                              "self_launched": os.environ.get("TCA_SELF_LAUNCHED") == "1"}), flush=True)
        shutdown(info)
        return
    if dev.type != "cuda":
        raise SystemExit("bench.py needs a GPU")
    from triton_client_amd.pipelines import CameraPipeline, GraphRunner, LidarPipeline
    from triton_client_amd.utils.synthetic import LidarSpec, camera_frame, lidar_sweep
    import triton_client_amd.models.fast as fast_plans
    if args.dense_bev:
        fast_plans.BEV_UNIFORM = False
    if args.unfused_detect:
        fast_plans.DETECT_FUSED = False

    B = args.batch
    H0, W0 = (int(v) for v in args.cam.split("x"))
    # sensor mounted 3.23 m up; the reference's +1.5 m z offset (ros_inference3d.py:123-128)
    # brings the ground to the KITTI frame's -1.73 m.
    cp = args.lidar_model == "centerpoint"
    # nuScenes LiDAR frame: sensor ~1.8 m up, no z shift; KITTI PointPillars: see above
    spec = LidarSpec(rings=args.rings, azimuth_steps=args.columns, sensor_height=1.8 if cp else 3.23)
    max_points = ((spec.points_per_sweep + 1023) // 1024) * 1024
    use_cam = args.only in ("both", "camera")
    use_lid = args.only in ("both", "lidar")

    torch.manual_seed(0)
    det2 = args.camera_model in ("retinanet", "fcos")
    S = 1  # frames per branch run as one pipeline (sub-batched multistream variants measured slower, removed)
    if use_cam and args.camera_model == "yolov4":
        from triton_client_amd.pipelines import Yolov4Pipeline

        def make_cam(b, m):
            return Yolov4Pipeline(model=m, batch=b, src_hw=(H0, W0), img=512, device=dev, precision=args.precision)
    elif use_cam and det2:
        from triton_client_amd.config.detectron import DetectronConfig
        from triton_client_amd.pipelines import DetectronPipeline

        def make_cam(b, m):
            return DetectronPipeline(model=m, batch=b, src_hw=(H0, W0), cfg=DetectronConfig(arch=args.camera_model),
                                     device=dev, precision=args.precision)
    else:
        def make_cam(b, m):
            return CameraPipeline(model=m, batch=b, src_hw=(H0, W0), device=dev, precision=args.precision)
    sec = args.lidar_model == "second_iou"
    if args.sweeps > 1 and not (use_lid and cp):
        raise SystemExit("--sweeps needs --lidar-model centerpoint")
    if use_lid and cp:
        from triton_client_amd.pipelines import CenterPointPipeline

        def make_lid(b, m):
            return CenterPointPipeline(model=m, batch=b, max_points=max_points, device=dev, precision=args.precision,
                                       nsweeps=args.sweeps)
    elif use_lid and sec:
        from triton_client_amd.pipelines import SecondPipeline

        def make_lid(b, m):
            return SecondPipeline(model=m, batch=b, max_points=max_points, device=dev, z_offset=1.5,
                                  precision=args.precision)
    else:
        def make_lid(b, m):
            return LidarPipeline(model=m, batch=b, max_points=max_points, device=dev, z_offset=1.5,
                                 precision=args.precision)
    cam = make_cam(B, None) if use_cam else None
    lid = make_lid(B, None) if use_lid else None

    # ---------------- synthetic sensor data in pinned host memory
    shards = info.world if (args.ingest == "rccl" and info.is_main) else 1
    have_host = args.ingest == "local" or info.is_main
    nd = max(1, min(args.distinct, B))
    step_bytes = 0
    if have_host:
        seed0 = 1000 * info.rank
        cams = [camera_frame(H0, W0, seed0 + i) for i in range(nd)] if use_cam else []
        clouds = [lidar_sweep(spec, seed0 + 500 + i) for i in range(nd)] if use_lid else []
        jpegs = None
        if use_cam and args.camera_input == "jpeg":
            import io

            from PIL import Image
            jpegs = []
            for f in cams:
                buf = io.BytesIO()
                Image.fromarray(f).save(buf, format="JPEG", quality=args.jpeg_quality)
                jpegs.append(buf.getvalue())
        if use_cam:
            cam_host = torch.empty((shards, B, H0, W0, 3), dtype=torch.uint8).pin_memory()
            for s in range(shards):
                for b in range(B):
                    cam_host[s, b].copy_(torch.from_numpy(cams[(s * B + b) % nd]))
            step_bytes += cam_host[0].numel()
        if use_lid:
            fb = lid.frame_bytes
            pc_host = torch.zeros((shards, B * fb), dtype=torch.uint8).pin_memory()
            n_host = torch.zeros((shards, B), dtype=torch.int32).pin_memory()
            for s in range(shards):
                for b in range(B):
                    c = clouds[(s * B + b) % nd]
                    raw = torch.from_numpy(c.view(np.uint8).reshape(-1))
                    pc_host[s, b * fb:b * fb + raw.numel()].copy_(raw)
                    n_host[s, b] = c.shape[0]
            step_bytes += pc_host[0].numel()
    node = None
    if args.ingest == "rccl" and info.is_main:
        node = {}
        if use_cam:
            node["cam"] = torch.empty((info.world, B, H0, W0, 3), dtype=torch.uint8, device=dev)
        if use_lid:
            node["pc"] = torch.empty((info.world, B * lid.frame_bytes), dtype=torch.uint8, device=dev)
            node["n"] = torch.empty((info.world, B), dtype=torch.int32, device=dev)

    # ---------------- calibrate detection density on the first batch (see pipelines/*.calibrate_*)
    calib = {}
    if have_host or args.ingest == "rccl":
        if args.ingest == "local" or info.is_main:
            if use_cam:
                cam.frames.copy_(cam_host[0])
            if use_lid:
                lid.data.copy_(pc_host[0])
                lid.frame_n.copy_(n_host[0])
    if args.ingest == "local" or info.is_main:
        with _reproducible_calibration():
            if use_cam:
                calib["detectron_logit_shift" if det2 else "yolo_logit_shift"] = cam.calibrate_detection_density(
                    min(args.target_2d, 300.0) if det2 else args.target_2d)
            if use_lid:
                key = "centerpoint_hm_shift" if cp else ("second_iou_shift" if sec else "pp_logit_shift")
                # SECOND-IoU: the target is RoIs (of the 100 proposals) passing the final score threshold
                calib[key] = lid.calibrate_detection_density(min(args.target_3d, 60.0) if sec else args.target_3d)
    if info.world > 1:
        # every GPU must run the same model: rank 0's calibrated weights win
        from triton_client_amd.models.common import broadcast_parameters
        if use_cam:
            broadcast_parameters(cam.model)
        if use_lid:
            broadcast_parameters(lid.model)
    torch.cuda.synchronize()

    # the LiDAR branch is the critical path: its stream gets the higher HW-queue
    # priority so its kernels are dispatched first and the camera branch fills in
    side = (torch.cuda.Stream(priority=-1 if args.lidar_priority else 0)
            if (use_cam and use_lid and not args.serial) else None)

    def pipeline_step():
        """Camera and LiDAR branches on forked streams: under capture this is one
        graph with two parallel branches, so each branch's low-occupancy phases
        (sort / NMS reduce / unpack) overlap the other's convolutions."""
        if side is None:
            r2 = cam.step() if use_cam else None
            r3 = lid.step() if use_lid else None
            return r2, r3
        main = torch.cuda.current_stream()
        side.wait_stream(main)
        with torch.cuda.stream(side):
            r3 = lid.step()
        r2 = cam.step()
        main.wait_stream(side)
        return r2, r3

    if side is not None and args.graph_mode == "split" and not args.no_graph:
        # one graph per branch, each replayed on its own stream (its own HW queue):
        # the overlap no longer depends on how the runtime maps a forked graph's
        # branches onto queues
        cam_runner = GraphRunner(cam.step)
        lid_runner = GraphRunner(lid.step)

        def split_step():
            main = torch.cuda.current_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                r3 = lid_runner()
            r2 = cam_runner()
            main.wait_stream(side)
            return r2, r3

        runner = _Split(split_step)
    else:
        runner = GraphRunner(pipeline_step, enabled=not args.no_graph)
    native = None
    comm_used = "torch" if info.world > 1 else "none"
    rccl_ranks = 1
    selftest = None
    if args.comm == "native" and info.world > 1 and not gloo_rehearsal:
        from triton_client_amd.parallel.rccl import NativeComm

        try:
            native = NativeComm.from_info(info)
            rccl_ranks = native.count()
            comm_used = "native"
        except Exception as e:  # noqa: BLE001 - the process group's own RCCL communicator still serves
            print(f"[bench] rank {info.rank}: native RCCL communicator unavailable ({e}); "
                  f"using torch.distributed p2p", file=sys.stderr, flush=True)
            native = None
        if native is not None:
            # the step's gather pattern, eager and in two alternately replayed graphs, under a time
            # limit: a communicator that cannot run it is aborted and the process group serves instead
            from triton_client_amd.parallel.rccl import native_selftest
            ok_, why = native_selftest(native, info.rank, info.world)
            selftest = why
            print(f"[bench] rank {info.rank}: native RCCL self-test: {why}", file=sys.stderr, flush=True)
            if not ok_:
                native = None
        import torch.distributed as dist
        ok = torch.tensor([1 if native is not None else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)  # every rank takes the same path
        if int(ok.item()) == 0:
            native = None
            comm_used = "torch"
    if native is None and info.world > 1:
        import torch.distributed as dist
        rccl_ranks = dist.get_world_size() if dist.get_backend() == "nccl" else 0
    if info.world > 1 and not gloo_rehearsal and rccl_ranks != args.gpus:
        raise SystemExit(f"RCCL communicator spans {rccl_ranks} ranks, expected --gpus {args.gpus}")
    preflight = _preflight(info, dev, rccl_ranks, comm_used)
    preflight["native_selftest"] = selftest
    ex = FrameExchange(info, native=native)
    # with the native RCCL communicator the detection gather (grouped send / recv of fixed-shape
    # result buffers) is stream work: it is captured inside the step graph(s), so a step is one
    # replay.  With the double-buffered graphs (the default) each of the two captures holds its own
    # copy of the grouped plan over the one communicator, gathering into that set's receive buffers
    # (tests/test_rccl.py: two graphs replaying one communicator's plan, alternately)
    will_db = (args.ingest == "local" and not args.no_prefetch and not (use_cam and args.camera_input == "jpeg")
               and not args.single_input_set and isinstance(runner, GraphRunner) and runner.enabled)
    gather_in_graph = (native is not None and isinstance(runner, GraphRunner) and runner.enabled
                       and args.ingest == "local")
    gbuf = {}
    if gather_in_graph and not will_db:
        def step_and_gather():
            r2, r3 = pipeline_step()
            src = outputs(r2, r3)
            if "dst" not in gbuf:  # allocated in the eager warm-up, before capture
                gbuf["dst"] = ([list(src)] + [[torch.empty_like(t) for t in src] for _ in range(1, info.world)]
                               if info.is_main else None)
            ex.gather(src, gbuf["dst"])
            return r2, r3
        runner = GraphRunner(step_and_gather)

    jdec = None
    if use_cam and args.camera_input == "jpeg":
        if args.ingest != "local":
            raise SystemExit("--camera-input jpeg needs --ingest local")
        from triton_client_amd.ops.jpeg import JpegBatchDecoder
        jdec = JpegBatchDecoder(B, dev, threads=args.decode_threads)
        jpeg_copy = torch.cuda.Stream()
        jstep = [0]

        def stage_next_jpegs():
            """Host entropy decode of the next step's B JPEGs (C++ threads),
            then their H2D on a copy stream — runs while the GPU computes."""
            j0 = jstep[0]
            jstep[0] += 1
            jdec.upload(jdec.stage([jpegs[(j0 * B + b) % nd] for b in range(B)]), jpeg_copy)

        stage_next_jpegs()
    dsts = [t for t in ((cam.frames,) if use_cam and jdec is None else ()) +
            ((lid.data, lid.frame_n) if use_lid else ())]
    # ---------------- ingest: local mode prefetches step t+1's frames (H2D on a copy
    # stream into landing buffers) while step t computes
    prefetch = args.ingest == "local" and not args.no_prefetch
    if prefetch:
        copy_stream = torch.cuda.Stream()
        landing = [torch.empty_like(t) for t in dsts]
        host_src = [t for t in ((cam_host[0],) if use_cam and jdec is None else ()) +
                    ((pc_host[0], n_host[0]) if use_lid else ())]
        h2d_done = torch.cuda.Event()
        consumed = torch.cuda.Event()

        def issue_h2d():
            copy_stream.wait_event(consumed)
            with torch.cuda.stream(copy_stream):
                for d, h in zip(landing, host_src):
                    d.copy_(h, non_blocking=True)
                h2d_done.record(copy_stream)

        consumed.record()
        issue_h2d()

    # two captured graphs over two input sets: the prefetch writes straight into the set the next
    # replay reads, so no per-step D2D copy from landing buffers (BEV / camera frames: ~60 us)
    d2h_stage = None
    piped = post_split = front_next = False
    front_after = 0
    # (not with the RCCL gather captured in the step graph: two graphs replaying the same
    # communicator's p2p have not run on a multi-GPU node yet, so that path keeps one graph)
    # (split mode keeps one input set: double-buffering its two per-branch graphs measured slower,
    # 8.92-8.98 vs 8.45 ms, profiles/r3/sched_ab.txt)
    db = will_db and prefetch and jdec is None
    assert db == will_db, (db, will_db)
    if db:
        owners = ([(cam, "frames")] if use_cam else []) + ([(lid, "data"), (lid, "frame_n")] if use_lid else [])
        in_sets = [list(dsts), [torch.empty_like(t) for t in dsts]]
        # the step graph is captured twice, once per input set, with its results copied into a
        # per-capture D2H stage
        piped = bool(args.lidar_pipeline) and use_lid and not cp and not sec
        post_split = piped and args.lidar_pipeline >= 2
        if piped:
            # two LiDAR pipelines over one model: graph k finishes pipeline k's batch (network + NMS)
            # and preprocesses the next batch into pipeline 1-k, whose own data buffer is its input set
            lids = [lid, make_lid(B, lid.model)]
            for lp in lids:
                lp.build_fast()
            blocks_front = len(lids[0].fast.bb.blocks) - 1 if args.lidar_pipeline == 4 else None
            front_next = args.lidar_pipeline == 5
            # mode 5: the next batch's front waits until lside has issued the first TCA_FRONT_AFTER
            # down blocks (default 1: the voxeliser chain runs beside blocks 2-3, not beside block 1's
            # hx3 convs; +1.7% median on one box, profiles/r6/knobs/ sweep 16); 0: right after the
            # neck / NMS
            front_after = int(os.environ.get("TCA_FRONT_AFTER", "1")) if front_next else 0
            # (TCA_FRONT_AFTER_CONVS: the gate after that many convs instead of whole blocks)
            front_convs = (int(os.environ.get("TCA_FRONT_AFTER_CONVS", "0"))
                           or lids[0].fast.bb.convs_before(front_after)) if front_after else 0
            front_ev = [torch.cuda.Event(), torch.cuda.Event()]
            side2 = torch.cuda.Stream()
            lside = side if side is not None else torch.cuda.Stream()
            # (the canvas clear moved from the front into the back half: 7.60 vs 7.60 ms, not kept;
            # the back half starts with the step: held until the front's VFE is done, so that the neck
            # runs beside the backbone convs instead, 9.55 vs 7.43-7.54 ms; a 128 / 64-workgroup neck
            # grid 7.44-7.72 / 8.01-8.06 vs 7.38-7.60; the front on a high-priority stream 9.7 ms)

            def piped_fn(k):
                def fn():
                    main = torch.cuda.current_stream()
                    lside.wait_stream(main)
                    side2.wait_stream(main)
                    if front_next:  # graph k: pipeline k's blocks beside pipeline 1-k's neck / NMS + next front
                        with torch.cuda.stream(lside):
                            lids[k].step_blocks(mark=(front_convs, front_ev[k]) if front_after else None)
                        with torch.cuda.stream(side2):
                            r3 = lids[1 - k].step_back()
                            if front_after:
                                side2.wait_event(front_ev[k])
                            lids[1 - k].step_pre()
                    elif post_split:  # graph k: pipeline k's front beside pipeline 1-k's decode / NMS
                        with torch.cuda.stream(lside):
                            lids[k].step_front(neck_back=args.lidar_pipeline >= 3, blocks_front=blocks_front)
                        with torch.cuda.stream(side2):
                            r3 = lids[1 - k].step_back()
                    else:  # graph k: pipeline k's network / NMS beside pipeline 1-k's preprocessing
                        with torch.cuda.stream(lside):
                            r3 = lids[k].step_post()
                        with torch.cuda.stream(side2):
                            lids[1 - k].step_pre()
                    r2 = cam.step() if use_cam else None
                    main.wait_stream(lside)
                    main.wait_stream(side2)
                    return r2, r3
                return fn
            owners = [(cam, "frames")] if use_cam else []
            in_sets = [in_sets[0][:len(owners)], in_sets[1][:len(owners)]]
            base_fns = [piped_fn(0), piped_fn(1)]
        else:
            base_fns = [runner.fn, runner.fn]
        units = [("all", None, lambda r: outputs(*r))]
        stages = {name: [None, None] for name, _, _ in units}

        def h2d_pairs(k):  # (device, host) pairs of the inputs graph k reads
            if not piped:
                return list(zip(in_sets[k], host_src))
            pairs = [(in_sets[k][0], host_src[0])] if use_cam else []
            p = k if post_split and not front_next else 1 - k  # the pipeline whose preprocessing graph k runs
            return pairs + [(lids[p].data, pc_host[0]), (lids[p].frame_n, n_host[0])]

        def stage_copy(dst_, src_):
            # every result tensor into the stage with ONE batched copy kernel (a graph node per
            # tensor cost ~11 us each at the end of the step: 9 copyBuffer nodes, ~100 us)
            from triton_client_amd import _native
            pairs = [(d, t) for d, t in zip(dst_, src_) if t.numel()]
            if not all(d.is_contiguous() and t.is_contiguous() for d, t in pairs):
                for d, t in pairs:
                    d.copy_(t, non_blocking=True)
                return
            dp, sp, nb = (np.asarray(v, np.int64) for v in (
                [d.data_ptr() for d, _ in pairs], [t.data_ptr() for _, t in pairs],
                [t.numel() * t.element_size() for _, t in pairs]))
            _native.call("tca_copy_segments", len(pairs), dp.ctypes.data, sp.ctypes.data, nb.ctypes.data,
                         _native.stream_ptr(torch.cuda.current_stream()))

        def bound(name, _unused, outs_of, k):
            base_fn = base_fns[k]

            def fn():
                for (o, attr), t in zip(owners, in_sets[k]):
                    setattr(o, attr, t)
                try:
                    res = base_fn()
                finally:
                    for (o, attr), t in zip(owners, in_sets[0]):
                        setattr(o, attr, t)
                if info.world == 1:  # results -> this capture's D2H stage (device copies inside the graph)
                    src_ = outs_of(res)
                    if stages[name][k] is None:  # allocated in the eager warm-up, before capture
                        stages[name][k] = [torch.empty_like(t) for t in src_]
                    stage_copy(stages[name][k], src_)
                elif gather_in_graph:  # the grouped RCCL gather into this set's receive buffers
                    src_ = outs_of(res)
                    if stages[name][k] is None:
                        stages[name][k] = ([[torch.empty_like(t) for t in src_] for _ in range(info.world)]
                                           if info.is_main else [])
                    ex.gather(src_, stages[name][k] if info.is_main else None)
                return res
            return fn
        unit_runners = {name: [GraphRunner(bound(name, fn, of, k)) for k in (0, 1)] for name, fn, of in units}
        d2h_stream = torch.cuda.Stream()
        d2h_free = [torch.cuda.Event(), torch.cuda.Event()]
        db_done = [torch.cuda.Event(), torch.cuda.Event()]
        db_free = [torch.cuda.Event(), torch.cuda.Event()]

        def db_replay(k):
            return unit_runners["all"][k]()

        def db_h2d(k):
            copy_stream.wait_event(db_free[k])
            with torch.cuda.stream(copy_stream):
                for d, h in h2d_pairs(k):
                    d.copy_(h, non_blocking=True)
                db_done[k].record(copy_stream)

        torch.cuda.synchronize()  # the landing-buffer prefetch issued above is not used
        for k in (0, 1):
            db_free[k].record()
            db_h2d(k)  # both sets hold valid frames before either graph's eager warm-up reads them
        torch.cuda.synchronize()
        if piped:  # prologue: graph 0's first replay finishes a batch of pipeline 0 (mode 1) / 1 (mode 2)
            if front_next:  # mode 5: pipeline 0's canvas and pipeline 1's down blocks
                lids[0].step_pre()
                lids[1].step_front(neck_back=True)
            elif post_split:
                lids[1].step_front(neck_back=args.lidar_pipeline >= 3, blocks_front=blocks_front)
            else:
                lids[0].step_pre()
            torch.cuda.synchronize()

        class _DoubleBuffered:
            t = 0

            def __call__(self):
                nonlocal d2h_stage
                if self.t == 0:  # capture every graph (the first warm-up step); both input sets hold frames
                    for rs in unit_runners.values():
                        for r_ in rs:
                            r_.capture()
                    o = [outputs(*unit_runners["all"][k].out) for k in (0, 1)]
                    if not piped and [t.data_ptr() for t in o[0]] != [t.data_ptr() for t in o[1]]:
                        raise SystemExit("double-buffered graphs: the two captures return different result buffers")
                    if info.world == 1 or gather_in_graph:
                        d2h_stage = [stages["all"][k] for k in (0, 1)]
                k = self.t % 2
                cur = torch.cuda.current_stream()
                cur.wait_event(db_done[k])
                if self.t >= 2:
                    cur.wait_event(d2h_free[k])  # stage[k]'s D2H (two steps ago) is done
                out = db_replay(k)
                db_free[k].record(cur)
                db_h2d(1 - k)  # the other set (read by the previous step) streams in the next frames
                self.t += 1
                return out

        runner = _DoubleBuffered()

    def ingest():
        if jdec is not None:
            jdec.reconstruct(cam.frames)  # this step's JPEGs, staged during the previous step
        if db:
            return  # the double-buffered runner orders its own H2D
        if prefetch:
            cur = torch.cuda.current_stream()
            cur.wait_event(h2d_done)
            for d, l_ in zip(dsts, landing):
                d.copy_(l_, non_blocking=True)
            consumed.record(cur)
            issue_h2d()  # next step's frames stream in while this step computes
            return
        if args.ingest == "local":
            if use_cam and jdec is None:
                cam.frames.copy_(cam_host[0], non_blocking=True)
            if use_lid:
                lid.data.copy_(pc_host[0], non_blocking=True)
                lid.frame_n.copy_(n_host[0], non_blocking=True)
            return
        if info.is_main:
            if use_cam:
                node["cam"].copy_(cam_host, non_blocking=True)
            if use_lid:
                node["pc"].copy_(pc_host, non_blocking=True)
                node["n"].copy_(n_host, non_blocking=True)
        ex.scatter(scatter_src(), dsts)

    def scatter_src():
        if not info.is_main:
            return None
        return [[t for t in ((node["cam"][r],) if use_cam else ()) + ((node["pc"][r], node["n"][r]) if use_lid else ())]
                for r in range(info.world)]

    gather_dst = None
    last_src = [None]
    host_out = None  # [2][world][k]: double-buffered so step t's D2H overlaps step t+1
    out_ready = [torch.cuda.Event(), torch.cuda.Event()]
    it = [0]

    def outputs(r2, r3):
        """Flat list of result tensors; with sub-batches r2 / r3 are lists of
        per-sub-pipeline results, laid out camera subs then LiDAR subs."""
        o = []
        for r in (r2 if isinstance(r2, list) else [r2]):
            if r is not None:
                o += [r.box, r.score, r.cls, r.count]
        for r in (r3 if isinstance(r3, list) else [r3]):
            if r is not None:
                n3 = getattr(r, "nms", r)  # CenterPoint: per (frame, task) segments
                o += [n3.box, n3.score, n3.cls, n3.count]
        return o

    def step():
        nonlocal gather_dst, host_out
        ingest()
        r2, r3 = runner()
        if jdec is not None:
            stage_next_jpegs()  # host decode overlaps this step's GPU work
        src = outputs(r2, r3)
        last_src[0] = src
        if gather_dst is None and info.is_main:
            # rank 0's own detections are D2H-copied straight from the graph's result
            # buffers (stream order keeps the next replay behind that copy)
            own = [torch.empty_like(t) for t in src] if piped else list(src)  # piped: results alternate buffers
            gather_dst = (gbuf["dst"] if (gather_in_graph and not db) else
                          [own] + [[torch.empty_like(t) for t in src] for _ in range(1, info.world)])
            host_out = [[[torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in src] for _ in range(info.world)]
                        for _ in range(2)]
        staged = db and d2h_stage is not None and (info.world == 1 or gather_in_graph)
        if not gather_in_graph and not staged:  # (one rank with a staged D2H: nothing to gather)
            ex.gather(src, gather_dst if info.is_main else None)
        k = it[0] % 2
        if info.is_main:
            if staged:
                # the replay already copied (one rank) or gathered (RCCL, in the graph) its results into
                # stage[j]: the D2H runs on the copy stream beside the next replay, which writes the other
                j = (runner.t - 1) % 2
                d2h_stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(d2h_stream):
                    per_rank = [d2h_stage[j]] if info.world == 1 else d2h_stage[j]
                    for r, stage_r in enumerate(per_rank):
                        for h, d in zip(host_out[k][r], stage_r):
                            h.copy_(d, non_blocking=True)
                    out_ready[k].record(d2h_stream)
                    d2h_free[j].record(d2h_stream)
            else:
                for r in range(info.world):
                    for h, d in zip(host_out[k][r], gather_dst[r]):
                        h.copy_(d, non_blocking=True)
                out_ready[k].record()
        else:
            out_ready[k].record()
            if staged:
                d2h_free[(runner.t - 1) % 2].record()  # (workers: the gather's sends are in the replay)
        # detections of the previous step are on rank 0's host now; this step's
        # D2H completes while the next step is issued
        if it[0] > 0:
            out_ready[1 - k].synchronize()
        it[0] += 1

    t_setup = time.perf_counter()
    for _ in range(args.warmup):
        step()
    barrier(info)
    torch.cuda.synchronize()
    if jdec is not None:
        jdec.stats.update(frames=0, host_s=0.0)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    barrier(info)
    elapsed = time.perf_counter() - t0
    elapsed = allreduce_max(info, elapsed)
    dumped = None
    if args.dump_outputs and info.is_main:
        if host_out is None:
            raise SystemExit("--dump-outputs needs at least one step")
        # the synchronize above completed the last step's D2H into host_out[(it - 1) % 2]
        dumped = dump_outputs(args.dump_outputs, host_out[(it[0] - 1) % 2],
                              (["cam"] if use_cam else []) + (["lidar"] if use_lid else []))
    # --full: DP communication alone, after the timed run (every rank takes part): the
    # detection gather (captured in the step graph when gather_in_graph) and the
    # --ingest rccl frame scatter, µs per step, max over ranks
    comm_us = None
    if info.world > 1 and args.full:
        def _time_us(fn, reps=10):
            barrier(info)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return allreduce_max(info, 1e3 * e0.elapsed_time(e1) / reps)
        comm_us = {"gather": round(_time_us(lambda: ex.gather(last_src[0], gather_dst if info.is_main else None)), 1)
                   if not (gather_in_graph and db) else None,
                   "gather_bytes_per_rank": int(sum(t.numel() * t.element_size() for t in last_src[0])),
                   "gather_in_graph": gather_in_graph}
        if args.ingest == "rccl":
            comm_us["scatter"] = round(_time_us(lambda: ex.scatter(scatter_src(), dsts)), 1)
            comm_us["scatter_bytes_per_rank"] = int(sum(t.numel() * t.element_size() for t in dsts))
    jpeg_info = None
    if jdec is not None:
        host_us = jdec.host_us_per_frame()
        gpu_us = None
        if args.full:
            # GPU half alone (IDCT + colour kernels), timed after the run
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            reps = 10
            e0.record()
            for _ in range(reps):
                jdec.pending = 0
                jdec.reconstruct(cam.frames)
            e1.record()
            torch.cuda.synchronize()
            gpu_us = round(1e3 * e0.elapsed_time(e1) / reps / B, 2)
        jpeg_info = {"decode_threads": args.decode_threads, "quality": args.jpeg_quality,
                     "avg_jpeg_bytes": int(np.mean([len(j) for j in jpegs])),
                     "host_entropy_decode_wall_us_per_frame": round(host_us, 1),
                     "gpu_idct_color_us_per_frame": gpu_us,
                     "fallback_frames": jdec.stats["fallback"]}

    cam_name = {"yolov5n": "YOLOv5n-640 (COCO, 80 cls)", "yolov4": "YOLOv4-512 (COCO, 80 cls)",
                "retinanet": "RetinaNet R50-FPN 800x1344 (COCO)",
                "fcos": "FCOS R50-FPN 800x1344 (COCO)"}[args.camera_model]
    if info.is_main:
        frames = info.world * B * args.steps
        fps = frames / elapsed
        det2 = det3 = None
        k = 0
        last = (it[0] - 1) % 2
        ncs = S if use_cam else 0
        if use_cam:
            det2 = float(np.mean([host_out[last][r][4 * j + 3].float().mean().item()
                                  for r in range(info.world) for j in range(ncs)]))
        if use_lid:
            det3 = float(np.mean([sum(host_out[last][r][4 * (ncs + j) + 3].float().sum().item() for j in range(S)) / B
                                  for r in range(info.world)]))
        res = {
            "metric": METRIC,
            "value": round(fps, 2),
            "unit": "frames/s",
            "n_gpus": info.world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            # BASELINE.json publishes no reference number: nothing to divide by
            "vs_baseline": None,
            # families with an fp32 mode report the mode; the others run bf16 only
            "dtype": args.precision if (args.camera_model in ("yolov5n", "yolov4", "retinanet", "fcos") or not use_cam)
            and (args.lidar_model in ("pointpillars", "centerpoint", "second_iou") or not use_lid) else "bf16",
            "data": (f"synthetic: {nd} distinct {W0}x{H0} "
                     + (f"JPEG (q{args.jpeg_quality}, decoded every step)" if jdec is not None else "uint8 RGB")
                     + f" camera frames + {nd} distinct "
                     f"{spec.rings}x{spec.azimuth_steps} LiDAR sweeps per rank, re-sent every step "
                     f"(PointCloud2 16 B/pt, ~2% NaN dropouts); random-init weights (He-normal + LSUV rescaling on "
                     f"sample frames), detection-head bias offset calibrated so ~{args.target_2d:g} 2D / ~{args.target_3d:g} 3D candidates per frame reach NMS"),
            "config": {
                "model": ({"both": cam_name + " + ", "camera": cam_name, "lidar": ""}[args.only]
                          + ("" if args.only == "camera" else
                             (f"CenterPoint-PP (nuScenes, 10 cls, {args.sweeps} sweep{'s' if args.sweeps > 1 else ''}/frame)" if cp else
                              ("SECOND-IoU (KITTI, 3 cls)" if sec else "PointPillars (KITTI, 3 cls)")))),
                "global_batch": info.world * B,
                "seq_len": None,
                "parallelism": f"dp{info.world}",
                "frames_per_gpu_per_step": B,
                "precision": args.precision,
                "lidar_sweeps_per_frame": args.sweeps if (use_lid and cp) else None,
                "distinct_frames_per_rank": nd,
                "rccl_ranks": rccl_ranks,
                "preflight": preflight,
                "vs_reference_equivalent_emulation": round(fps / REFERENCE_EQUIVALENT_FPS, 2),
                "ingest": args.ingest,
                "camera_input": args.camera_input if use_cam else None,
                "jpeg": jpeg_info,
                "comm": comm_used,
                "hipgraph": not args.no_graph,
                "ingest_prefetch": prefetch,
                "branch_streams": (3 if piped else 2) if side is not None else 1,
                "graph_mode": args.graph_mode if side is not None else "single",
                "graph_input_sets": 2 if db else 1,
                "lidar_pipelined": (["off", "pre", "post", "neck", "block3", "neck+next_front"][args.lidar_pipeline]
                                    if piped else "off"),
                "lidar_pipeline_note": (("two LiDAR pipelines alternate: each timed step runs one full batch "
                                         "through every stage: batch t's down blocks beside batch t-1's neck, "
                                         "head, decode and NMS followed by batch t+1's preprocessing"
                                         + (f" (which waits until batch t's first {front_after} down block(s) are "
                                            "issued)" if front_after else "")
                                         + "; detections leave two steps after ingest") if piped and front_next else
                                        ("two LiDAR pipelines alternate: each timed step runs one full batch through "
                                         "every stage, one batch's first half beside the previous batch's second "
                                         "half (split point: lidar_pipelined); detections leave one step later")
                                        if piped else None),
                "host_bytes_per_gpu_per_step": step_bytes,
                "dp_comm_us_per_step": comm_us,
                "avg_2d_dets_per_frame": det2,
                "avg_3d_dets_per_frame": det3,
                "setup_plus_warmup_s": round(t0 - t_setup, 1),
                "full": args.full,
                "dumped_outputs": dumped,
                "head_bias_calibration": {k: round(v, 3) for k, v in calib.items()},
                "nms_candidates_target_per_frame": {"2d": args.target_2d, "3d": args.target_3d},
            },
        }
        line = json.dumps(res)
        print(line, flush=True)
        if args.json_out:
            with open(args.json_out, "w") as f:
                f.write(line + "\n")
    shutdown(info)
    if native is not None:
        # the step graphs hold RCCL work over the native communicator: leave without running
        # their destructors against it at interpreter exit (GraphRunner.release documents the
        # teardown order; the OS reclaims the communicator and the graphs together)
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)


if __name__ == "__main__":
    main()
