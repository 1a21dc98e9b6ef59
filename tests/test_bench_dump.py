"""bench.py --dump-outputs: the writer alone on host tensors (no GPU): names, float32, rows past
each frame's count zeroed, ranks concatenated, and the seeded frame sample above the size limit."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _result(B, M, D, seed):
    g = torch.Generator().manual_seed(seed)
    count = torch.randint(0, M + 1, (B,), generator=g, dtype=torch.int32)
    return [torch.randn(B, M, D, generator=g), torch.rand(B, M, generator=g),
            torch.randint(1, 80, (B, M), generator=g, dtype=torch.int32), count]


def test_dump_outputs_names_masking_and_ranks(tmp_path):
    r0 = _result(3, 5, 4, 0) + _result(3, 7, 7, 1)
    r1 = _result(3, 5, 4, 2) + _result(3, 7, 7, 3)
    r0[0][0, 4, :] = float("nan")  # a stale row past the count must not leak
    r0[3][0] = 2
    info = bench.dump_outputs(str(tmp_path / "o"), [r0, r1], ["cam", "lidar"])
    names = sorted(f"{b}_{k}" for b in ("cam", "lidar") for k in ("box", "score", "cls", "count"))
    assert info["arrays"] == names
    assert sorted(os.listdir(tmp_path / "o")) == [n + ".npy" for n in names]
    got = {n: np.load(tmp_path / "o" / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["cam_box"].shape == (6, 5, 4) and got["lidar_box"].shape == (6, 7, 7)
    for j, br in enumerate(("cam", "lidar")):
        for r, res in enumerate((r0, r1)):
            box, score, cls, count = (t.numpy() for t in res[4 * j:4 * j + 4])
            for b in range(3):
                n = int(count[b])
                f = 3 * r + b
                assert got[f"{br}_count"][f] == n
                np.testing.assert_array_equal(got[f"{br}_box"][f, :n], box[b, :n])
                np.testing.assert_array_equal(got[f"{br}_score"][f, :n], score[b, :n])
                np.testing.assert_array_equal(got[f"{br}_cls"][f, :n], cls[b, :n].astype(np.float32))
                assert not got[f"{br}_box"][f, n:].any() and not got[f"{br}_score"][f, n:].any()
                assert not got[f"{br}_cls"][f, n:].any()


def test_dump_outputs_samples_frames_above_the_limit(tmp_path, monkeypatch):
    res = _result(16, 8, 4, 0)
    full = sum(t.numel() * 4 for t in res)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", full // 2)
    picks = []
    for d in ("a", "b"):
        info = bench.dump_outputs(str(tmp_path / d), [res], ["cam"])
        assert info["bytes"] <= full // 2
        picks.append(np.load(tmp_path / d / "frames.npy"))
    np.testing.assert_array_equal(picks[0], picks[1])  # the same frames every run
    idx = picks[0].astype(int)
    assert 1 <= len(idx) < 16 and len(set(idx)) == len(idx)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "cam_count.npy"), res[3].numpy()[idx])
