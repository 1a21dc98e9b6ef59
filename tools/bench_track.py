"""Standalone time of the tracker kernels ``tca_track2d`` (K25) and ``tca_track3d`` (K24): one
launch per batch of 32 frames x 64 detections against a state that already holds the tracks of
one pass over the batch (restored on the device before every timed launch), between two
device events; 10 warm-up launches, then 50 timed.  The last launch's ids, hits, velocities
and state are compared with the definition (``track_numpy``), bit for bit.

The 2D scene is the generator of ``tests/track2d_scenes.py``; the 3D scene is the generator of
``tests/test_track3d.py`` (copied: that module needs pytest), with 7-d and 9-d boxes.

    python tools/bench_track.py [--entry 2d|3d|both] [--launches 50] [--warmup 10]

``TCA_KERNELS_LIB`` times another build of the kernel library.  One JSON object on stdout.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES, DETS, OBJECTS = 32, 64, 80
MS = 1_000_000


def scene3d(seed, nine):
    """``tests/test_track3d.py scene``: objects of three classes at constant velocity plus noise,
    dropouts, false positives, frames 0..100 ms apart → ``(preds, stamps)``."""
    r = np.random.default_rng(seed)
    pos, vel = r.uniform(-60, 60, (OBJECTS, 2)), r.uniform(-8, 8, (OBJECTS, 2))
    lab = r.integers(1, 4, OBJECTS)
    preds, stamps, t = [], [], 1_000 * MS
    for f in range(FRAMES):
        dt = int(r.choice([0, 50, 100, 100])) * MS if f not in (0, 3) else 0
        t += dt
        pos = pos + vel * (dt * 1e-9)
        pick = r.permutation(OBJECTS)[:min(DETS, int(r.integers(DETS // 2, DETS + 1)))]
        fill = DETS - len(pick)
        xy = np.concatenate([pos[pick] + r.normal(0, 0.05, (len(pick), 2)), r.uniform(-60, 60, (fill, 2))])
        lb = np.concatenate([lab[pick], r.integers(1, 4, fill)])
        v = np.concatenate([vel[pick], np.zeros((fill, 2))])
        o = r.permutation(DETS)
        b = np.zeros((DETS, 9 if nine else 7), np.float32)
        b[:, :2], b[:, 3:6] = xy[o], (4.0, 2.0, 1.5)
        if nine:
            b[:, 6:8] = v[o]
        preds.append({"pred_boxes": b, "pred_labels": lb[o].astype(np.int64)})
        stamps.append(t)
    return preds, stamps


def time_entry(torch, state_cls, batch, capacity, define, launch, launches, warmup):
    """``define(state, batch)``: the definition in place; ``launch(dev, state_ptr, out_ptr)``: the
    entry on the uploaded batch ``dev`` (rows, dt, reset)."""
    st0 = state_cls(capacity)
    define(st0, batch)  # one pass: the tracks the timed launch meets
    want_state = st0.copy()
    want = define(want_state, batch)
    nd = int(batch.det_off[-1])
    dev = {"rows": torch.from_numpy(batch.rows.view(np.uint8).reshape(-1).copy()).cuda(),
           "dt": torch.from_numpy(batch.dt).cuda(), "reset": torch.from_numpy(batch.reset).cuda()}
    state0 = torch.from_numpy(st0.words()).cuda()
    state, out = torch.empty_like(state0), torch.zeros((nd, 4), dtype=torch.int32, device="cuda")
    times = []
    for i in range(warmup + launches):
        state.copy_(state0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch(dev, state.data_ptr(), out.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1) * 1e3)
    got = out.cpu().numpy()
    got_state = state_cls.from_words(state.cpu().numpy(), capacity)
    ids = np.concatenate([w[0] for w in want])
    hits = np.concatenate([w[1] for w in want])
    vel = np.concatenate([w[2] for w in want]).view(np.int32)
    same = bool((got[:, 0] == ids).all() and (got[:, 1] == hits).all() and (got[:, 2:4] == vel).all()
                and got_state.same(want_state))
    return {"kernel_us_median": round(float(np.median(times)), 1), "kernel_us_min": round(float(np.min(times)), 1),
            "kernel_us_max": round(float(np.max(times)), 1), "launches": launches,
            "live_tracks": int((want_state.id != 0).sum()), "same_as_definition": same}


def main() -> int:
    global FRAMES, DETS
    ap = argparse.ArgumentParser()
    ap.add_argument("--entry", choices=("2d", "3d", "both"), default="both")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=FRAMES, help="frames per batch (at most 64)")
    ap.add_argument("--dets", type=int, default=DETS, help="detections per frame (at most 512)")
    a = ap.parse_args()
    FRAMES, DETS = a.frames, a.dets

    import torch

    from triton_client_amd import _native
    from triton_client_amd.ops import track2d as T2
    from triton_client_amd.ops import track3d as T3

    _native.kernels()
    runs = {}
    if a.entry in ("2d", "both"):
        import track2d_scenes as S

        batch = T2.track_table(*S.scene(7, [DETS] * FRAMES, n_obj=OBJECTS))
        for cap in (64, 256, 512):
            runs[f"track2d, capacity {cap}"] = time_entry(
                torch, T2.TrackState2D, batch, cap, lambda st, b: T2.track_numpy(st, b),
                lambda d, state, out: T2.launch(d["rows"].data_ptr(), batch.det_off, FRAMES, d["dt"].data_ptr(),
                                                d["reset"].data_ptr(), state, cap, 30, 0.2, 0.5, 0.5, 0.5, out),
                a.launches, a.warmup)
    if a.entry in ("3d", "both"):
        gates = T3.gate_table(None, ["a", "b", "c"])
        dgates = torch.from_numpy(gates).cuda()
        for nine in (False, True):
            preds, stamps = scene3d(7, nine)
            batch = T3.track_table(preds, None, stamps)
            for cap in (64, 256, 1024):
                runs[f"track3d, capacity {cap}, {'9-d' if nine else '7-d'}"] = time_entry(
                    torch, T3.TrackState, batch, cap, lambda st, b: T3.track_numpy(st, b, gates),
                    lambda d, state, out: T3.launch(d["rows"].data_ptr(), batch.det_off, FRAMES, d["dt"].data_ptr(),
                                                    d["reset"].data_ptr(), dgates.data_ptr(), len(gates), state, cap,
                                                    3, 0.5, out),
                    a.launches, a.warmup)
    out = {"what": f"one launch per batch of {FRAMES} frames x {DETS} detections, device events",
           "device": torch.cuda.get_device_name(0), "kernels_lib": os.environ.get("TCA_KERNELS_LIB", "in-tree"),
           "runs": runs}
    print(json.dumps(out, indent=1), flush=True)
    return 0 if all(r["same_as_definition"] for r in runs.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
