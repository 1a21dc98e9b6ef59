#!/usr/bin/env python
"""K28 ``tca_rectify`` alone, on resident frames (``profiles/rectify/README.md``).

Default: every variant of ``tca_rectify_variant`` (frames per read of a map entry x store path)
on ``--frames`` frames of ``--hw`` under ``driver_bench.py``'s synthetic wide-angle model, timed
with events around ``--reps`` back-to-back launches, ``--rounds`` interleaved rounds of all
variants in one process; beside them a device-to-device copy of the same frames and the shipped
kernel under an identity map (perfectly local gathers).  Prints one JSON line.

``--trace``: 50 launches of the shipped entry and nothing else, for a kernel trace taken in a run
of its own::

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/rectify_bench.py --trace
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path[:0] = [".", os.path.dirname(os.path.abspath(__file__))]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hw", default="720,1280")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--trace", action="store_true", help="50 launches of tca_rectify, no timing")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()

    import torch

    from driver_bench import _barrel_model
    from triton_client_amd.ops import rectify as R

    H, W = (int(v) for v in a.hw.split(","))
    B = a.frames
    dev = torch.device("cuda")
    rec = R.Rectifier(_barrel_model(H, W), device=dev)
    src = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    dst = torch.empty_like(src)
    if a.trace:
        for _ in range(50):
            rec.rectify_(src, dst)
        torch.cuda.synchronize()
        return

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        s.record()
        for _ in range(a.reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.reps * 1e3  # us per launch

    ident = R.Rectifier(R.CameraModel(width=W, height=H, K=[[0.6 * W, 0, (W - 1) / 2], [0, 0.6 * W, (H - 1) / 2],
                                                            [0, 0, 1]], D=[0.0] * 5), device=dev)
    runs = {f"chunk{c}_{'byte' if b else 'dword'}": (lambda c=c, b=b: R.rectify_(src, dst, rec.map_dev, variant=(c, b)))
            for b in (0, 1) for c in (1, 2, 4, 8, 16, 32)}
    runs["shipped"] = lambda: rec.rectify_(src, dst)
    runs["shipped_identity_map"] = lambda: ident.rectify_(src, dst)
    runs["copy"] = lambda: dst.copy_(src)
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    out = {"tool": "rectify_bench", "device": torch.cuda.get_device_name(0), "shape": [B, H, W, 3],
           "frames_MB": round(B * H * W * 3 / 1e6, 1), "map_MB": round(H * W * 8 / 1e6, 1), "reps": a.reps,
           "rounds": a.rounds,
           "us_per_launch": {k: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1)}
                             for k, v in times.items()}}
    line = json.dumps(out)
    print(line)
    if a.json_out:
        with open(a.json_out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
