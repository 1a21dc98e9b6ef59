"""CenterPoint-PP (det3d, nuScenes): model, fast plan, decode/NMS, kernels."""
import dataclasses

import numpy as np
import pytest
import torch

from triton_client_amd.config.lidar import NUSC_PILLARS, CenterPointConfig
from triton_client_amd.models.centerpoint import (build_centerpoint, decode_reference, merged_task_outputs,
                                                  pfn_point_features)
from triton_client_amd.models.common import fuse_model, randomize_bn
from triton_client_amd.ops.conv import NHWC
from triton_client_amd.ops.lidar import voxelize_np
from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep


def _small_cfg(**kw):
    v = dataclasses.replace(NUSC_PILLARS, point_cloud_range=(-12.8, -12.8, -5.0, 12.8, 12.8, 3.0), max_voxels=4000)
    return CenterPointConfig(voxel=v, **kw)


def _model(cfg, seed=0):
    m = build_centerpoint(cfg, seed)
    randomize_bn(m, 3)
    m = fuse_model(m.eval())
    with torch.no_grad():  # tame the random regression heads (exp(dim)) like the pipeline calibration
        for t in m.head.tasks:
            for n, c in t.out.items():
                s = 0.05 if n != "hm" else 0.3
                c.weight.mul_(s)
                c.bias.mul_(s)
    return m


def _cloud(cfg, seed=0):
    pts = lidar_sweep(LidarSpec(rings=16, azimuth_steps=512, sensor_height=1.8), seed)
    p = np.frombuffer(pts.tobytes(), np.float32).reshape(-1, 4)
    p = p[~np.isnan(p).any(1)]
    return np.concatenate([p, np.zeros((len(p), 1), np.float32)], 1)


def test_fast_centerpoint_cpu_matches_module():
    from triton_client_amd.models.fast import FastCenterPoint
    cfg = _small_cfg()
    m = _model(cfg)
    nx, ny, _ = cfg.voxel.grid_size
    canvas = torch.zeros(2, ny, nx, 64)
    canvas[:, ::3, ::2] = torch.rand(2, (ny + 2) // 3, (nx + 1) // 2, 64)
    with torch.no_grad():
        ref = merged_task_outputs(m.bev_forward(canvas.permute(0, 3, 1, 2)))
        f = FastCenterPoint(m, 2, device="cpu")
        out = f.forward(NHWC(canvas)).t
    for t, r in enumerate(ref):
        o = out[..., f.task_offsets[t]:f.task_offsets[t] + r.shape[1]].permute(0, 3, 1, 2)
        torch.testing.assert_close(o, r, rtol=1e-4, atol=1e-4)


def test_pfn_features_and_model_forward_shapes():
    cfg = _small_cfg()
    m = _model(cfg)
    p5 = _cloud(cfg)
    v, zyx, num, _ = voxelize_np(p5, cfg.voxel, 5)
    coords = torch.from_numpy(np.pad(zyx, ((0, 0), (1, 0))).astype(np.int32))
    f = pfn_point_features(torch.from_numpy(v), torch.from_numpy(num.astype(np.int64)), coords, cfg.voxel)
    assert f.shape == (len(v), cfg.voxel.max_points_per_voxel, 10)
    assert (f[torch.arange(20).view(1, -1).expand(len(v), -1) >= torch.from_numpy(num).view(-1, 1)] == 0).all()
    with torch.no_grad():
        out = m(torch.from_numpy(v), torch.from_numpy(num.astype(np.int64)), coords, 1)
    H, W = cfg.feature_map_size
    assert len(out) == 6 and out[0]["hm"].shape == (1, 1, H, W) and out[1]["hm"].shape == (1, 2, H, W)


def test_postprocess_cpu_and_class_thresholds():
    from triton_client_amd.ops.centerpoint import NUSC_CLASS_THRESH, CenterPointPostprocess
    cfg = _small_cfg()
    m = _model(cfg)
    H, W = cfg.feature_map_size
    with torch.no_grad():
        canvas = torch.rand(1, 64, *[s * cfg.out_size_factor for s in (H, W)])
        mo = merged_task_outputs(m.bev_forward(canvas))
    head = torch.zeros(1, H, W, 96)
    for t, o in enumerate(mo):
        head[..., 16 * t:16 * t + o.shape[1]] = o.permute(0, 2, 3, 1)
    pp = CenterPointPostprocess(cfg, 1, [16 * t for t in range(6)], device="cpu")
    res = pp(head).per_image()[0]
    offs = [0, 1, 3, 5, 6, 8]
    ref = decode_reference(mo, cfg, offs)[0]
    np.testing.assert_allclose(np.sort(res["pred_scores"]), np.sort(ref[1]), rtol=1e-6)
    assert res["pred_boxes"].shape[1] == 9
    assert len(res["pred_scores"]) > 0
    pp2 = CenterPointPostprocess(cfg, 1, [16 * t for t in range(6)], device="cpu", class_thresh=NUSC_CLASS_THRESH)
    r2 = pp2(head).per_image()[0]
    for c, th in NUSC_CLASS_THRESH.items():
        assert (r2["pred_scores"][r2["pred_labels"] == c] > th).all()


# ---------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_pfn2_kernel_vs_fp32(cuda):
    from triton_client_amd.ops.centerpoint import PFNEncoder
    cfg = _small_cfg()
    m = _model(cfg)
    p5 = _cloud(cfg, 1)
    v, zyx, num, _ = voxelize_np(p5, cfg.voxel, 5)
    V = len(v)
    coords = np.pad(zyx, ((0, 0), (1, 0))).astype(np.int32)
    enc = PFNEncoder(cfg.voxel, m.pfn, 1, device=cuda)
    feat = torch.zeros((1, cfg.voxel.max_voxels, 64), dtype=torch.float32, device=cuda)
    vox = torch.zeros((1, cfg.voxel.max_voxels, 20, 5), device=cuda)
    vox[0, :V] = torch.from_numpy(v).to(cuda)
    nump = torch.zeros((1, cfg.voxel.max_voxels), dtype=torch.int32, device=cuda)
    nump[0, :V] = torch.from_numpy(num).to(cuda)
    co = torch.zeros((1, cfg.voxel.max_voxels, 4), dtype=torch.int32, device=cuda)
    co[0, :V] = torch.from_numpy(coords).to(cuda)
    vc = torch.tensor([V], dtype=torch.int32, device=cuda)
    enc.encode_from_voxels(vox, nump, co, vc, feat_out=feat)
    torch.cuda.synchronize()
    with torch.no_grad():
        f = pfn_point_features(torch.from_numpy(v), torch.from_numpy(num.astype(np.int64)),
                               torch.from_numpy(coords), cfg.voxel)
        ref = m.pfn.float()(f)
    got = feat[0, :V].cpu()
    err = (got - ref).abs().max().item()
    assert err < 0.02 * max(1.0, ref.abs().max().item()), err
    # the canvas holds the same features (bf16) at each pillar's cell
    cv = enc.canvas[0].float().cpu()
    np.testing.assert_allclose(cv[coords[:, 2], coords[:, 3]].numpy(), got.numpy(), rtol=0.02, atol=0.02)


@pytest.mark.gpu
def test_centerhead_decode_gpu_matches_cpu(cuda):
    from triton_client_amd.ops.centerpoint import CenterPointPostprocess
    cfg = _small_cfg()
    m = _model(cfg)
    H, W = cfg.feature_map_size
    with torch.no_grad():
        canvas = torch.rand(2, 64, H * 4, W * 4)
        mo = merged_task_outputs(m.bev_forward(canvas))
    head = torch.zeros(2, H, W, 96)
    for t, o in enumerate(mo):
        head[..., 16 * t:16 * t + o.shape[1]] = o.permute(0, 2, 3, 1)
    offs = [16 * t for t in range(6)]
    ref = CenterPointPostprocess(cfg, 2, offs, device="cpu")(head).per_image()
    got = CenterPointPostprocess(cfg, 2, offs, device=cuda)(head.to(cuda)).per_image()
    for r, g in zip(ref, got):
        assert abs(len(r["pred_scores"]) - len(g["pred_scores"])) <= 2
        k = min(20, len(r["pred_scores"]))
        np.testing.assert_allclose(np.sort(g["pred_scores"])[::-1][:k], np.sort(r["pred_scores"])[::-1][:k],
                                   rtol=1e-5)


@pytest.mark.gpu
def test_centerpoint_pipeline_graph(cuda):
    from triton_client_amd.pipelines import CenterPointPipeline, GraphRunner
    pipe = CenterPointPipeline(batch=2, max_points=32768, device=cuda)
    for b in range(2):
        c = lidar_sweep(LidarSpec(rings=32, azimuth_steps=1024, sensor_height=1.8), b)
        raw = torch.from_numpy(c.view(np.uint8).reshape(-1))
        pipe.data[b * pipe.frame_bytes: b * pipe.frame_bytes + raw.numel()].copy_(raw)
        pipe.frame_n[b] = c.shape[0]
    d = pipe.calibrate_detection_density(300.0)
    assert -30 < d < 30
    eager = pipe.step()
    torch.cuda.synchronize()
    e = eager.per_image()
    run = GraphRunner(pipe.step)
    g = run().per_image()
    g2 = run().per_image()
    assert all(len(x["pred_scores"]) > 0 for x in e)
    for a, b, c in zip(e, g, g2):
        np.testing.assert_array_equal(b["pred_boxes"], c["pred_boxes"])
        assert a["pred_boxes"].shape[1] == 9 and len(a["pred_scores"]) <= 6 * 83


def _rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


@pytest.mark.gpu
def test_pfn2_fp32_mode_vs_fp64(cuda):
    """fp32 mode PFN (both layers split-product, fp32 canvas) against an fp64
    evaluation of the module: relative L2 at the fp32 plans' bound (2e-4; the
    bf16 PFN's second layer alone sits near 2e-3)."""
    from triton_client_amd.ops.centerpoint import PFNEncoder
    cfg = _small_cfg()
    m = _model(cfg)
    p5 = _cloud(cfg, 1)
    v, zyx, num, _ = voxelize_np(p5, cfg.voxel, 5)
    V = len(v)
    coords = np.pad(zyx, ((0, 0), (1, 0))).astype(np.int32)
    Vm = cfg.voxel.max_voxels
    vox = torch.zeros((1, Vm, 20, 5), device=cuda)
    vox[0, :V] = torch.from_numpy(v).to(cuda)
    nump = torch.zeros((1, Vm), dtype=torch.int32, device=cuda)
    nump[0, :V] = torch.from_numpy(num).to(cuda)
    co = torch.zeros((1, Vm, 4), dtype=torch.int32, device=cuda)
    co[0, :V] = torch.from_numpy(coords).to(cuda)
    vc = torch.tensor([V], dtype=torch.int32, device=cuda)
    with torch.no_grad():
        f = pfn_point_features(torch.from_numpy(v).double(), torch.from_numpy(num.astype(np.int64)),
                               torch.from_numpy(coords), cfg.voxel)
        ref = m.pfn.double()(f)
    m.pfn.float()
    errs = {}
    for precision in ("fp32", "bf16"):
        enc = PFNEncoder(cfg.voxel, m.pfn, 1, device=cuda, precision=precision)
        feat = torch.zeros((1, Vm, 64), dtype=torch.float32, device=cuda)
        enc.encode_from_voxels(vox, nump, co, vc, feat_out=feat)
        torch.cuda.synchronize()
        errs[precision] = _rel_l2(feat[0, :V], ref)
        cv = enc.canvas[0].float().cpu()
        assert enc.canvas.dtype == (torch.float32 if precision == "fp32" else torch.bfloat16)
        if precision == "fp32":  # the canvas holds exactly the features
            torch.testing.assert_close(cv[coords[:, 2], coords[:, 3]], feat[0, :V].cpu(), rtol=0, atol=0)
    print("pfn rel L2", errs)
    assert errs["fp32"] < 2e-4 and errs["fp32"] < errs["bf16"], errs


@pytest.mark.gpu
def test_fast_centerpoint_fp32_vs_fp64_module(cuda):
    """fp32 mode RPN + CenterHead plan against an fp64 evaluation of the fused
    module, per task: relative L2 below the fp32 plans' bound (2e-4)."""
    from triton_client_amd.models.fast import FastCenterPoint
    cfg = _small_cfg()
    m = _model(cfg)
    nx, ny, _ = cfg.voxel.grid_size
    canvas = torch.zeros(2, ny, nx, 64)
    canvas[:, ::3, ::2] = torch.rand(2, (ny + 2) // 3, (nx + 1) // 2, 64)
    with torch.no_grad():
        ref = merged_task_outputs(m.double().bev_forward(canvas.double().permute(0, 3, 1, 2)))
    f = FastCenterPoint(m.float(), 2, device=cuda, precision="fp32")
    out = f.forward(NHWC(canvas.to(cuda))).t
    torch.cuda.synchronize()
    assert out.dtype == torch.float32
    errs = [_rel_l2(out[..., f.task_offsets[t]:f.task_offsets[t] + r.shape[1]].permute(0, 3, 1, 2), r)
            for t, r in enumerate(ref)]
    print("centerpoint fp32 rel L2", errs)
    assert max(errs) < 2e-4, errs


@pytest.mark.gpu
def test_centerpoint_pipeline_fp32_matches_bf16_kept_set(cuda):
    """Same weights, same sweeps: the fp32 pipeline's detections and the bf16
    pipeline's agree on the strong boxes (bf16 is the secondary mode)."""
    from triton_client_amd.pipelines import CenterPointPipeline
    res = {}
    base = None
    for precision in ("fp32", "bf16"):
        import copy
        pipe = CenterPointPipeline(model=None if base is None else copy.deepcopy(base), batch=2, max_points=32768,
                                   device=cuda, precision=precision)
        for b in range(2):
            c = lidar_sweep(LidarSpec(rings=32, azimuth_steps=1024, sensor_height=1.8), b)
            raw = torch.from_numpy(c.view(np.uint8).reshape(-1))
            pipe.data[b * pipe.frame_bytes: b * pipe.frame_bytes + raw.numel()].copy_(raw)
            pipe.frame_n[b] = c.shape[0]
        if base is None:
            pipe.calibrate_detection_density(300.0)
            base = pipe.model
        res[precision] = pipe.step().per_image()
        torch.cuda.synchronize()
    for a, b in zip(res["fp32"], res["bf16"]):
        assert len(a["pred_scores"]) > 0
        k = min(10, len(a["pred_scores"]), len(b["pred_scores"]))
        np.testing.assert_allclose(np.sort(a["pred_scores"])[::-1][:k], np.sort(b["pred_scores"])[::-1][:k],
                                   rtol=0.05, atol=0.02)


def _pose(yaw, tx, ty, tz):
    import math
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([c, -s, 0, tx, s, c, 0, ty, 0, 0, 1, tz], np.float32)


def test_merge_sweeps_reference_cpu():
    """A static world point seen from two sensor poses lands on the same current-frame
    coordinates after the merge; lags are t_cur - t_k; the current sweep comes first."""
    from triton_client_amd.ops.lidar import merge_sweeps_np

    T0, T1 = _pose(0.3, 1.0, -2.0, 0.1), _pose(0.5, 2.5, -1.0, 0.1)
    world = np.array([[5.0, 3.0, -1.0]])

    def to_sensor(T, w):
        Tm = T.reshape(3, 4).astype(np.float64)
        return (w - Tm[:, 3]) @ Tm[:, :3]
    p_prev = np.concatenate([to_sensor(T0, world), [[0.7]]], 1).astype(np.float32)
    p_cur = np.concatenate([to_sensor(T1, world), [[0.2]]], 1).astype(np.float32)
    m = merge_sweeps_np(p_cur, [(p_prev, 0.95, T0)], 1.0, T1)
    assert m.shape == (2, 5)
    np.testing.assert_allclose(m[1, :3], m[0, :3], atol=1e-5)
    np.testing.assert_allclose(m[:, 3:], [[0.2, 0.0], [0.7, 0.05]], atol=1e-6)


@pytest.mark.gpu
def test_sweep_ring_gpu_matches_reference(cuda):
    """tca_sweep_step over several steps (ring wrap-around, partial history at the
    start, per-frame counts, moving poses and clocks) == merge_sweeps_np."""
    from triton_client_amd.ops.lidar import SweepAccumulator, merge_sweeps_np

    rng = np.random.default_rng(0)
    B, maxp, S = 3, 700, 4
    acc = SweepAccumulator(S, B, maxp, cuda, dt=0.0)
    hist = [[] for _ in range(B)]
    for step in range(7):
        pts = rng.standard_normal((B, maxp, 4)).astype(np.float32)
        n = rng.integers(0, maxp + 1, B).astype(np.int32)
        t = (0.05 * step + 0.01 * np.arange(B)).astype(np.float32)
        poses = np.stack([_pose(0.1 * step + b, 0.5 * step, -0.2 * b, 0.0) for b in range(B)])
        acc.clock.copy_(torch.from_numpy(t))
        acc.pose.copy_(torch.from_numpy(poses))
        out, cnt = acc(torch.from_numpy(pts).to(cuda), torch.from_numpy(n).to(cuda))
        torch.cuda.synchronize()
        for b in range(B):
            want = merge_sweeps_np(pts[b, :n[b]], hist[b][::-1][:S - 1], float(t[b]), poses[b])
            k = int(cnt[b])
            assert k == len(want), (step, b, k, len(want))
            np.testing.assert_allclose(out[b, :k].cpu().numpy(), want, rtol=1e-5, atol=1e-5)
            hist[b].append((pts[b, :n[b]].copy(), float(t[b]), poses[b].copy()))


@pytest.mark.gpu
def test_sweep_ring_epoch_clock_keeps_ms_lags(cuda):
    """Message stamps in epoch seconds (~1.7e9 s) and an auto-advanced clock after
    hours of streaming: the time-lag feature stays exact to well under a ms (the
    ring's stamps are fp64; fp32 stamps would quantise them to 128 s)."""
    from triton_client_amd.ops.lidar import SweepAccumulator

    B, maxp, S = 2, 64, 3
    pts = torch.ones((B, maxp, 4), device=cuda)
    n = torch.full((B,), maxp, dtype=torch.int32, device=cuda)
    acc = SweepAccumulator(S, B, maxp, cuda, dt=0.0)
    t0 = 1.7e9 + 0.123
    for step in range(3):
        acc.clock.fill_(t0 + 0.05 * step)
        out, cnt = acc(pts, n)
    torch.cuda.synchronize()
    lags = out[0, :S * maxp, 4].cpu().numpy().reshape(S, maxp)[:, 0]
    np.testing.assert_allclose(lags, [0.0, 0.05, 0.1], atol=1e-6)
    auto = SweepAccumulator(S, B, maxp, cuda, dt=0.05)
    auto.clock.fill_(3600.0 * 5)  # five hours in
    for _ in range(3):
        out, cnt = auto(pts, n)
    torch.cuda.synchronize()
    lags = out[1, :S * maxp, 4].cpu().numpy().reshape(S, maxp)[:, 0]
    np.testing.assert_allclose(lags, [0.0, 0.05, 0.1], atol=1e-6)


@pytest.mark.gpu
def test_centerpoint_pipeline_multisweep_graph(cuda):
    """nsweeps = 3: the merged point list feeds the voxeliser and the PFN (time lag
    as the 5th feature); the ring advances inside the captured graph, so the first
    replays see a growing history and detections stay finite."""
    from triton_client_amd.pipelines.centerpoint import CenterPointPipeline
    from triton_client_amd.pipelines.graph import GraphRunner
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep

    spec = LidarSpec(rings=32, azimuth_steps=1024, sensor_height=1.8)
    p = CenterPointPipeline(batch=2, max_points=32768, device=cuda, nsweeps=3)
    for b in range(2):
        c = lidar_sweep(spec, b)
        raw = torch.from_numpy(c.view(np.uint8).reshape(-1))
        p.data[b * p.frame_bytes: b * p.frame_bytes + raw.numel()].copy_(raw)
        p.frame_n[b] = c.shape[0]
    p.calibrate_detection_density(300.0)
    p.sweeps.reset()
    run = GraphRunner(p.step)
    counts = []
    for _ in range(4):
        r = run()
        torch.cuda.synchronize()
        counts.append(int(p.sweeps.out_n[0]))
        d = r.per_image()[0]
        assert len(d["pred_scores"]) > 0 and np.isfinite(d["pred_boxes"]).all()
    n0 = int(p.frame_n[0])  # the eager warm-up filled the 2-sweep history: 3 sweeps merged per replay
    assert len(set(counts)) == 1 and 2.5 * n0 < counts[0] <= 3 * n0, (counts, n0)


@pytest.mark.gpu
def test_centerpoint_served_model_gpu(cuda):
    """The served centerpoint_pp model on the GPU path (PFN from received voxels over the
    full 512 x 512 canvas): 9-d finite boxes, 0-based nuScenes labels, and the same bytes
    from a second execute (the canvas cells of a request are cleared before the next)."""
    from triton_client_amd.server.models import CenterPointModel
    m = CenterPointModel("centerpoint_pp", device="cuda")
    m.load()
    p = lidar_sweep(LidarSpec(rings=32, azimuth_steps=1024, sensor_height=1.8), 7)
    p = p[~np.isnan(p).any(1)]
    v, zyx, num, _ = voxelize_np(p, m.cfg.voxel, 4)
    coords = np.concatenate([np.zeros((len(zyx), 1), np.int32), zyx], 1)
    req = {"voxels": v, "voxel_coords": coords, "voxel_num_points": num.astype(np.int32)}
    out = m.execute(req, None)
    n = len(out["pred_scores"])
    assert out["pred_boxes"].shape == (n, 9) and n > 0 and np.isfinite(out["pred_boxes"]).all()
    assert out["pred_labels"].dtype == np.int64 and set(np.unique(out["pred_labels"])) <= set(range(10))
    out2 = m.execute(req, None)
    for k in ("pred_boxes", "pred_scores", "pred_labels"):
        np.testing.assert_array_equal(out[k], out2[k])
