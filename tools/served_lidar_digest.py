#!/usr/bin/env python3
"""Digests of what the three served LiDAR models answer to fixed requests.

Builds ``pointpillar_kitti``, ``second_iou`` and ``centerpoint_pp`` from the repository's
factories (default config, default seed), voxelises fixed synthetic sweeps with
``voxelize_np`` and sends them through ``execute``; ``pointpillar_kitti`` also answers
three requests through ``execute_batch``.  Writes one JSON with the sha256 of every output
array and of each model's ``config.pbtxt`` text, so that two trees can be compared for
equal answers (``profiles/lidar_families/``).

    python tools/served_lidar_digest.py --device cuda --out digest.json
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name -> (sweep rings, azimuth steps, sensor height, z offset, request seeds)
REQUESTS = {
    "pointpillar_kitti": (32, 1024, 3.23, 1.5, (11, 12, 13)),
    "second_iou": (32, 1024, 3.23, 1.5, (21, 22)),
    "centerpoint_pp": (32, 1024, 1.8, 0.0, (31, 32)),
}


def _sha(a) -> str:
    a = np.ascontiguousarray(np.asarray(a))
    return hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()


def _request(cfg, rings, steps, height, zoff, seed, features):
    from triton_client_amd.ops.lidar import voxelize_np
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep

    p = lidar_sweep(LidarSpec(rings=rings, azimuth_steps=steps, sensor_height=height), seed)
    p = p[~np.isnan(p).any(1)]
    p[:, 2] += zoff
    v, zyx, num, _ = voxelize_np(p, cfg.voxel, 4)
    if features > 4:  # the time-lag column of a single sweep
        v = np.concatenate([v, np.zeros(v.shape[:2] + (features - 4,), v.dtype)], 2)
    coords = np.concatenate([np.zeros((len(zyx), 1), np.int32), zyx.astype(np.int32)], 1)
    return {"voxels": v, "voxel_coords": coords, "voxel_num_points": num.astype(np.int32)}


def _digest(out) -> dict:
    return {"n": int(len(out["pred_scores"])), **{k: _sha(out[k]) for k in sorted(out)}}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=None)
    ap.add_argument("--models", default=",".join(REQUESTS))
    flags = ap.parse_args(argv)

    from google.protobuf import text_format

    from triton_client_amd.server.repository import FACTORIES

    res = {"device": flags.device, "models": {}}
    for name in flags.models.split(","):
        rings, steps, height, zoff, seeds = REQUESTS[name]
        m = FACTORIES[name](device=flags.device)
        m.load()
        width = int(m.config().input[0].dims[-1])
        # the last CenterPoint request keeps the voxeliser's 4 columns (accepted: the lag reads as zero)
        reqs = [_request(m.cfg, rings, steps, height, zoff, s, width if i == 0 else 4) for i, s in enumerate(seeds)]
        entry = {"config_sha256": hashlib.sha256(text_format.MessageToString(m.config()).encode()).hexdigest(),
                 "voxels": [int(len(r["voxels"])) for r in reqs],
                 "execute": [_digest(m.execute(r, None)) for r in reqs]}
        if name == "pointpillar_kitti":
            entry["execute_batch"] = [_digest(o) for o in m.execute_batch(reqs, None)]
        res["models"][name] = entry
        print(name, json.dumps(entry["execute"]), flush=True)
    text = json.dumps(res, indent=1, sort_keys=True)
    if flags.out:
        os.makedirs(os.path.dirname(os.path.abspath(flags.out)), exist_ok=True)
        with open(flags.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
