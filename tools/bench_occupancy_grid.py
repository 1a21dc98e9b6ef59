"""K33 measurements: `tca_occupancy_grid` behind `tca_ground_split` on clouds of the synthetic sweep.

    python tools/bench_occupancy_grid.py --clouds 32 --reps 20          # device events per variant, the checks
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_occupancy_grid.py --reps 20 --variants default

Every variant's planes are compared with the default's on all clouds, and the default's with the definition on the
first cloud.  The event-timed figure of a variant is its whole launch (ground split + grid) less the ground split
alone, both as medians of `--reps` launches.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = {"default": {}, "no_lds_keys": {"privatise": False}, "atomic_per_point": {"aggregate": False},
            "keys_staged_in_lds": {"stage_keys": True}}


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
    ap.add_argument("--sectors", type=int, default=720)
    ap.add_argument("--variants", default=",".join(VARIANTS), help="comma-separated, of " + ", ".join(VARIANTS))
    ap.add_argument("--no-host", action="store_true", help="skip timing the host definition")
    a = ap.parse_args()
    from triton_client_amd.ops import ground as G
    from triton_client_amd.ops import occupancy_grid as O
    from triton_client_amd.ops.cloud_common import CloudLayout
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep

    spec = LidarSpec(sensor_height=3.23)
    clouds = [np.frombuffer(lidar_sweep(spec, s).tobytes(), np.float32).reshape(-1, 4).copy() for s in range(a.clouds)]
    lay = CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7))
    o, g = O.GridOptions(sectors=a.sectors), G.GroundOptions(sensor_height=spec.sensor_height)
    mapper = O.GridMapper("cuda")
    call = mapper.prepare([c.tobytes() for c in clouds], [len(c) for c in clouds], lay, o, g)
    split = timed(lambda: G.launch(call.ground, 3), a.reps)
    times, planes = {}, {}
    for name in a.variants.split(","):
        times[name] = timed(lambda: O.launch(call, **VARIANTS[name]), a.reps)
        planes[name] = call.out[:call.out_bytes].cpu().numpy().copy()
    first = next(iter(planes))
    assert all(p.tobytes() == planes[first].tobytes() for p in planes.values()), "the variants differ"
    want = O.grid_numpy(*O.split_rows(clouds[0], g), o)
    assert O.planes_of(planes[first], a.clouds, o)[0].tobytes() == want.tobytes(), "not the definition's bytes"
    host = None
    if not a.no_host:
        t0 = time.perf_counter()
        for c in clouds:
            O.grid_numpy(*O.split_rows(c, g), o)
        host = round((time.perf_counter() - t0) * 1e3, 1)
    counts = call.ground.counts.cpu().numpy()
    share = [round(float((want == v).mean()), 3) for v in (O.OCCUPIED, O.FREE, O.UNKNOWN)]

    def stats(v):
        return {"median": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1)}

    print(json.dumps({"clouds": a.clouds, "points_per_cloud": len(clouds[0]), "grid": f"{o.W}x{o.H}", "sectors": a.sectors,
                      "obstacle_records_per_cloud": round(float(counts[:, 0].mean())),
                      "ground_records_per_cloud": round(float(counts[:, 1].mean())),
                      "occupied_free_unknown_share_cloud0": share, "ground_split_us": stats(split),
                      **{f"split_and_grid_{k}_us": stats(v) for k, v in times.items()},
                      **{f"grid_{k}_us_less_split": round(v[len(v) // 2] - split[len(split) // 2], 1)
                         for k, v in times.items()},
                      "d2h_bytes": call.out_bytes, "split_and_grid_numpy_ms_all_clouds": host}))


if __name__ == "__main__":
    main()
