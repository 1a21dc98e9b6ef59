"""K38 measurements: `tca_depth_fill` alone on the key planes `tca_depth_image` made of the synthetic sweep's clouds.

    python tools/bench_depth_fill.py --clouds 32 --reps 20              # device events per radius set, the checks
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_depth_fill.py --reps 20 --sets defaults --no-host

Per encoding and radius set the entry is event-timed in its variants: two launches through the scratch plane
(`split`), one launch (`fused`), and `split` with the early exit of empty tiles off (`every_tile`).  The variants'
images are compared on all clouds, and `split`'s with the definition on the first.  The kernels of `tca_depth_image`
are timed in the same run, and the definition on the host.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_occupancy_grid import timed  # noqa: E402
from tools.driver_bench import _kitti_like_calibration  # noqa: E402

SETS = {"defaults": (2, 3, 15, 2), "no_large": (2, 3, 0, 2), "maximum": (4, 7, 15, 2)}
VARIANTS = {"split": (False, True), "fused": (True, True), "every_tile": (False, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", default="1280x720", metavar="WxH")
    ap.add_argument("--sets", default=",".join(SETS), help="comma-separated, of " + ", ".join(SETS))
    ap.add_argument("--encodings", default="16UC1,32FC1")
    ap.add_argument("--no-host", action="store_true", help="skip timing the host definition")
    a = ap.parse_args()
    from triton_client_amd.ops import depth_image as D
    from triton_client_amd.ops.cloud_common import CloudLayout
    from triton_client_amd.ops.range2d import Calibration
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep

    W, H = (int(v) for v in a.size.lower().split("x"))
    cal = _kitti_like_calibration()
    M = Calibration(np.diag([W / 1242.0, H / 375.0, 1.0]) @ cal.P, cal.T).M
    spec = LidarSpec(sensor_height=3.23)
    clouds = [np.frombuffer(lidar_sweep(spec, s).tobytes(), np.float32).reshape(-1, 4).copy() for s in range(a.clouds)]
    lay = CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7))
    imager = D.DepthImager("cuda")

    def stats(v):
        return {"median": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1)}

    out = {"clouds": a.clouds, "points_per_cloud": len(clouds[0]), "image": f"{W}x{H}"}
    for enc in a.encodings.split(","):
        for name in a.sets.split(","):
            k, h, g, m = SETS[name]
            o = D.DepthOptions(W, H, enc, fill=k, fill_hole=h, fill_large=g, fill_median=m)
            call = imager.prepare([c.tobytes() for c in clouds], [len(c) for c in clouds], lay, M, o)
            plain = D.DepthCall(**{**call.__dict__, "opts": D.DepthOptions(W, H, enc)})  # the same buffers, K38 not launched
            row = {}
            if f"depth_image_{enc}_us" not in out:
                out[f"depth_image_{enc}_us"] = stats(timed(lambda: D.launch(plain), a.reps))
            D.launch(plain)  # the keys K38 reads
            images = {}
            for variant, (fused, skip) in VARIANTS.items():
                row[variant] = stats(timed(lambda: D.fill(call, None, fused, skip), a.reps))
                images[variant] = call.out[:call.out_bytes].cpu().numpy().copy()
            assert all(im.tobytes() == images["split"].tobytes() for im in images.values()), "a variant changes the bytes"
            keys0 = call.plane[:4 * W * H].cpu().numpy().view(np.uint32).reshape(H, W)
            want = D.image_of_keys(D.fill_numpy(keys0, o), o)
            assert D.images_of(images["split"], a.clouds, o)[0].tobytes() == want.tobytes(), "not the definition's bytes"
            empty = np.uint32(D.EMPTY)
            row["pixels_with_a_depth_cloud0"] = {"before": int((keys0 != empty).sum()),
                                                 "after": int((D.fill_numpy(keys0, o) != empty).sum())}
            if not a.no_host:
                planes = call.plane[:4 * a.clouds * W * H].cpu().numpy().view(np.uint32).reshape(a.clouds, H, W)
                t0 = time.perf_counter()
                for p in planes:
                    D.fill_numpy(p, o)
                row["fill_numpy_ms_all_clouds"] = round((time.perf_counter() - t0) * 1e3, 1)
            out[f"fill_{enc}_{name}_us"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
