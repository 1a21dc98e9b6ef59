"""K32 measurements: `tca_cluster_fit` behind `tca_ground_split` + `tca_cluster` on clouds of the synthetic sweep.

    python tools/bench_cluster_fit.py --clouds 32 --reps 20            # device events, the host definition, the checks
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_cluster_fit.py --reps 20 --no-host

`--wall N` appends to every cloud a 60 m wall of N points 0.5 m in front of nothing else: one cluster of N points, the
long tail the split path is for.  Every configuration's fit bytes are compared with the definition on the first cloud,
and split against unsplit on all of them.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--wall", type=int, default=0, help="points of a 60 m wall added to every cloud")
    ap.add_argument("--no-host", action="store_true", help="skip timing the host definition")
    a = ap.parse_args()
    from triton_client_amd.ops import cluster as C
    from triton_client_amd.ops import cluster_fit as F
    from triton_client_amd.ops import ground as G
    from triton_client_amd.ops.cloud_common import CloudLayout
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep

    spec = LidarSpec(sensor_height=3.23)
    rng = np.random.default_rng(0)
    clouds = []
    for s in range(a.clouds):
        p = np.frombuffer(lidar_sweep(spec, s).tobytes(), np.float32).reshape(-1, 4).copy()
        if a.wall:  # 30 degrees to the axes, 1.5 m high, 5 cm thick
            t, th = rng.uniform(-30, 30, a.wall), np.deg2rad(30)
            w = np.stack([t * np.cos(th) - 20 * np.sin(th),
                          t * np.sin(th) + 20 * np.cos(th), rng.uniform(-2.5, -1.0, a.wall), np.ones(a.wall)], 1)
            w[:, :2] += rng.normal(0, 0.02, (a.wall, 2))
            p = np.concatenate([p, w.astype(np.float32)])
        clouds.append(p)
    lay = CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7))
    o, g, fo = C.ClusterOptions(), G.GroundOptions(sensor_height=spec.sensor_height), F.FitOptions()
    ex = C.ClusterExtractor("cuda")
    call = ex.prepare([c.tobytes() for c in clouds], [len(c) for c in clouds], lay, o, g)
    C.launch(call)
    f = F.prepare(ex, call, fo)
    out, times = {}, {}
    for name, split in (("split", True), ("unsplit", False)):
        for _ in range(3):
            F.launch(f, split=split)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            F.launch(f, split=split)
            e1.record()
        torch.cuda.synchronize()
        times[name] = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
        out[name] = f.fit[:f.fit_bytes].cpu().numpy().copy()
    for _ in range(a.reps):  # the launches in front, for the trace
        C.launch(call)
    torch.cuda.synchronize()
    assert call.err.item() == 0 and out["split"].tobytes() == out["unsplit"].tobytes()
    ns = call.ground.counts.cpu()[:, 0].tolist()
    res = C.results_of(call.out[:call.out_bytes].cpu().numpy(), call, ns, True)
    fits = F.results_of(out["split"], f, [r[0] for r in res])
    pts = [C.obstacle_rows(c, g) for c in clouds]
    assert fits[0].tobytes() == F.fit_numpy(pts[0], res[0][1], res[0][2], fo).tobytes()
    host = None
    if not a.no_host:
        t0 = time.perf_counter()
        for p, r in zip(pts, res):
            F.fit_numpy(p, r[1], r[2], fo)
        host = round((time.perf_counter() - t0) * 1e3, 1)
    sizes = np.concatenate([r[2]["n"] for r in res])
    print(json.dumps({"clouds": a.clouds, "points_per_cloud": len(clouds[0]), "wall": a.wall,
                      "obstacle_records_per_cloud": round(float(np.mean(ns))),
                      "clusters_per_cloud": round(len(sizes) / a.clouds, 1), "largest_cluster": int(sizes.max()),
                      "clusters_over_chunk": int((sizes > F.CHUNK).sum()),
                      **{f"fit_{k}_us": {"median": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1)}
                         for k, v in times.items()},
                      "fit_numpy_ms_all_clouds": host}))


if __name__ == "__main__":
    main()
