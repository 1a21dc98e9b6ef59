"""K37 measurements: `tca_grid_inflate` alone on the planes `tca_occupancy_grid` made of the synthetic sweep's clouds.

    python tools/bench_grid_inflate.py --clouds 32 --reps 20            # device events per radius, the checks
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_grid_inflate.py --reps 20 --cells 3 --no-host

Per radius (`--cells`, in cells of the default 0.2 m grid) the entry is event-timed with `skip_empty` on and off, its
planes are compared between the two on all clouds and with the definition on the first, and the definition is timed
on the host.  The grid's own kernels (whole launch less the ground split, as `tools/bench_occupancy_grid.py` takes
it) are timed in the same run.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_occupancy_grid import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cells", default="3,16,64", help="comma-separated inflation radii in cells (1..64)")
    ap.add_argument("--no-host", action="store_true", help="skip timing the host definition")
    a = ap.parse_args()
    from triton_client_amd.ops import ground as G
    from triton_client_amd.ops import occupancy_grid as O
    from triton_client_amd.ops.cloud_common import CloudLayout
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep

    spec = LidarSpec(sensor_height=3.23)
    clouds = [np.frombuffer(lidar_sweep(spec, s).tobytes(), np.float32).reshape(-1, 4).copy() for s in range(a.clouds)]
    lay = CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7))
    g = G.GroundOptions(sensor_height=spec.sensor_height)
    mapper = O.GridMapper("cuda")

    def stats(v):
        return {"median": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1)}

    out = {"clouds": a.clouds, "points_per_cloud": len(clouds[0])}
    for cells in (int(t) for t in a.cells.split(",")):
        o = O.GridOptions(inflation_radius=0.2 * cells - 0.05, inscribed_radius=0.3, cost_scaling=10.0 if cells < 16 else 1.0)
        assert o.inflation_cells == cells, (o.inflation_cells, cells)
        call = mapper.prepare([c.tobytes() for c in clouds], [len(c) for c in clouds], lay, o, g)
        if "grid" not in out:
            plain = O.GridCall(**{**call.__dict__, "opts": O.GridOptions()})  # the same buffers, K37 not launched
            split = timed(lambda: G.launch(call.ground, 3), a.reps)
            both = timed(lambda: O.launch(plain), a.reps)
            out.update({"grid": f"{o.W}x{o.H}", "ground_split_us": stats(split), "split_and_grid_us": stats(both),
                        "grid_us_less_split": round(both[len(both) // 2] - split[len(split) // 2], 1)})
        O.launch(call)  # the planes K37 reads
        row, planes = {}, {}
        for skip in (True, False):
            row["skip_empty" if skip else "every_tile"] = stats(timed(lambda: O.inflate(call, None, skip), a.reps))
            planes[skip] = call.inflated[:call.out_bytes].cpu().numpy().copy()
        assert planes[True].tobytes() == planes[False].tobytes(), "skip_empty changes the bytes"
        plane0 = O.planes_of(call.out[:call.out_bytes].cpu().numpy(), a.clouds, o)[0]
        want = O.inflate_numpy(plane0, o)
        assert O.planes_of(planes[True], a.clouds, o)[0].tobytes() == want.tobytes(), "not the definition's bytes"
        tiles = [(plane0.reshape(o.H, o.W)[max(0, y - cells):y + 32 + cells, max(0, x - cells):x + 64 + cells] == 100).any()
                 for y in range(0, o.H, 32) for x in range(0, o.W, 64)]
        row["tiles_with_an_obstacle_near_cloud0"] = f"{sum(tiles)}/{len(tiles)}"
        row["cells_with_a_cost_cloud0"] = int(((want > 0) & (want < 100) & (plane0 != want)).sum())
        if not a.no_host:
            t0 = time.perf_counter()
            for p in O.planes_of(call.out[:call.out_bytes].cpu().numpy(), a.clouds, o):
                O.inflate_numpy(p, o)
            row["inflate_numpy_ms_all_clouds"] = round((time.perf_counter() - t0) * 1e3, 1)
        out[f"inflate_{cells}_cells_us"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
