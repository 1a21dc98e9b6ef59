"""K34 measurements: `tca_voxel_downsample` on clouds of the synthetic sweep.

    python tools/bench_voxel_downsample.py --clouds 32 --reps 20        # device events per leaf and variant, the checks
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_voxel_downsample.py --reps 20 --leaves 0.2 --variants default

    python tools/bench_voxel_downsample.py --leaves 0.2 --variants default --outlier-radius 0.6 --outlier-neighbors 3 --outlier-mean-k 5,16

Every variant's rows are compared with the first variant's on all clouds, and those with the definition on the first
cloud.  The figure of a variant is its whole launch (five kernels), the median of `--reps` event-timed launches.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = {"default": {}, "wave_on": {"wave": True}, "wave_off": {"wave": False}, "lds_on": {"lds": True},
            "lds_off": {"lds": False}, "saved_on": {"saved": True}, "saved_off": {"saved": False},
            "all_off": {"wave": False, "lds": False, "saved": False}}


def timed(fn, reps):
    """Sorted microseconds of `reps` event-timed calls of `fn`, after three warm-ups."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--leaves", default="0.1,0.2,0.5")
    ap.add_argument("--variants", default=",".join(VARIANTS), help="comma-separated, of " + ", ".join(VARIANTS))
    ap.add_argument("--no-host", action="store_true", help="skip timing the host definition")
    ap.add_argument("--normals", type=float, default=0.0, metavar="R",
                    help="also time tca_voxel_normals alone at this radius, stage on and off, and check its bytes")
    ap.add_argument("--outlier-radius", type=float, default=0.0, metavar="R",
                    help="also time tca_voxel_outliers behind the downsample at this radius and check its bytes")
    ap.add_argument("--outlier-neighbors", type=int, default=0, metavar="N")
    ap.add_argument("--outlier-mean-k", default="", metavar="K[,K...]", help="one timing per K")
    ap.add_argument("--outlier-stddev", type=float, default=1.0, metavar="A")
    a = ap.parse_args()
    from triton_client_amd.ops import voxel_downsample as V
    from triton_client_amd.ops.cloud_common import CloudLayout
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep

    spec = LidarSpec(sensor_height=3.23)
    clouds = [np.frombuffer(lidar_sweep(spec, s).tobytes(), np.float32).reshape(-1, 4).copy() for s in range(a.clouds)]
    lay = CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7))
    op = V.VoxelDownsampler("cuda")
    out = {"clouds": a.clouds, "points_per_cloud": len(clouds[0]), "defaults": V.DEFAULTS}
    for leaf in (float(t) for t in a.leaves.split(",")):
        o = V.VoxelOptions(leaf=leaf, normal_radius=a.normals)
        call = op.prepare([c.tobytes() for c in clouds], [len(c) for c in clouds], lay, o)
        times, rows = {}, {}
        for name in a.variants.split(","):
            times[name] = timed(lambda: V.launch(call, **VARIANTS[name]), a.reps)
            rows[name] = V.rows_of(call.out[:call.out_bytes].cpu().numpy(), call)
        first = next(iter(rows))
        assert all(x.tobytes() == y.tobytes() for r in rows.values() for x, y in zip(r, rows[first])), "the variants differ"
        t0 = time.perf_counter()
        want = V.downsample_numpy(clouds[0], o)
        host = None if a.no_host else round((time.perf_counter() - t0) * 1e3 * a.clouds, 1)
        assert rows[first][0].tobytes() == want.tobytes(), "not the definition's bytes"
        out[f"leaf_{leaf:g}"] = {"voxels_per_cloud": round(float(np.mean([len(r) for r in rows[first]]))),
                                 "table_bytes": call.table_bytes, "d2h_bytes": 16 * sum(len(r) for r in rows[first]),
                                 **{f"{k}_us": {"median": round(v[len(v) // 2], 1), "min": round(v[0], 1),
                                                "max": round(v[-1], 1)} for k, v in times.items()},
                                 "numpy_ms_all_clouds_from_cloud0": host}
        if a.normals:  # (the times above are of both entries; these of the second alone, on the records of the last launch)
            alone, got = {}, {}
            for stage in (True, False):
                alone[stage] = timed(lambda: V.launch_normals(call, stage=stage), a.reps)
                got[stage] = call.normals[:call.rows_bytes].cpu().numpy()
            rows8 = V.rows_of(call.out[:call.out_bytes].cpu().numpy(), call, got[True])
            assert all(x.tobytes() == y.tobytes() for x, y in zip(rows8, V.rows_of(call.out[:call.out_bytes].cpu().numpy(), call, got[False]))), "stage on and off differ"
            t0 = time.perf_counter()
            want = V.normals_numpy(rows8[0][:, :4], o)
            assert rows8[0][:, 4:].tobytes() == want.tobytes(), "not the normals' definition's bytes"
            out[f"leaf_{leaf:g}"]["normals"] = {
                "radius": a.normals, "numpy_ms_all_clouds_from_cloud0": round((time.perf_counter() - t0) * 1e3 * a.clouds, 1),
                "no_normal_share": round(float(np.mean([np.isnan(r[:, 4]).mean() for r in rows8 if len(r)])), 4),
                **{f"stage_{'on' if s else 'off'}_us": {"median": round(v[len(v) // 2], 1), "min": round(v[0], 1),
                                                         "max": round(v[-1], 1)} for s, v in alone.items()}}
        if a.outlier_radius:  # (the filter rewrites the counts, so it is timed behind a downsample: the difference is its own)
            thin = V.downsample_numpy(clouds[0], V.VoxelOptions(leaf=leaf))
            plain = timed(lambda: V.launch(V.VoxelCall(**{**call.__dict__, "opts": V.VoxelOptions(leaf=leaf)})), a.reps)
            res = {"radius": a.outlier_radius, "downsample_alone_us": round(plain[len(plain) // 2], 1)}
            for k in [int(t) for t in a.outlier_mean_k.split(",") if t] or [0]:
                f = V.VoxelOptions(leaf=leaf, outlier_radius=a.outlier_radius, outlier_min_neighbors=a.outlier_neighbors,
                                   outlier_mean_k=k, outlier_stddev=a.outlier_stddev)
                both = op.prepare([c.tobytes() for c in clouds], [len(c) for c in clouds], lay, f)
                t = timed(lambda: V.launch(both), a.reps)
                got = V.rows_of(both.out[:both.out_bytes].cpu().numpy(), both, kept=both.kept[:both.rows_bytes].cpu().numpy())
                t0 = time.perf_counter()
                keep = V.outliers_numpy(thin, f)
                host = round((time.perf_counter() - t0) * 1e3 * a.clouds, 1)
                assert got[0].tobytes() == thin[keep].tobytes(), "not the outliers' definition's bytes"
                res[f"k_{k}"] = {"with_downsample_us": {"median": round(t[len(t) // 2], 1), "min": round(t[0], 1), "max": round(t[-1], 1)},
                                 "filter_us": round(t[len(t) // 2] - plain[len(plain) // 2], 1),
                                 "removed_share": round(1 - sum(len(r) for r in got) / sum(len(r) for r in rows[first]), 4),
                                 "numpy_ms_all_clouds_from_cloud0": host}
            out[f"leaf_{leaf:g}"]["outliers"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
