"""The device JPEG encoder (csrc/kernels/jpeg_encode.hip) against its definition
(ops/jpeg_encode.py encode_numpy): coefficients and files byte for byte, overflow, graph
replay, and the live camera path's compressed output."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from test_jpeg_encode import cases, corner_frame, frame
from triton_client_amd.ops import jpeg_encode as je
from triton_client_amd.ros import msgs

pytestmark = pytest.mark.gpu
PATTERN = 0xA5


def batch(hw, seeds=(1, 2)):
    """B = 3 frames of different content: a camera frame, noise, a flat dark frame."""
    H, W = hw
    return np.stack([frame("camera", H, W, seeds[0]), frame("noise", H, W, seeds[1]), np.full((H, W, 3), 7, np.uint8)])


def run(enc, frames, cap=None):
    out = torch.full((enc.B, cap or enc.cap), PATTERN, dtype=torch.uint8, device=enc.device)
    lens = torch.zeros((enc.B,), dtype=torch.int32, device=enc.device)
    enc.encode_(torch.from_numpy(frames).to(enc.device), out, lens)
    torch.cuda.synchronize()
    return out.cpu().numpy(), lens.cpu().numpy(), enc.coef.cpu().numpy()


def check_exact(frames, quality, subsampling, restart, cuda):
    H, W = frames.shape[1:3]  # room for any content: the default cap is sized for camera pictures, not noise
    enc = je.JpegBatchEncoder(len(frames), (H, W), cuda, quality, subsampling, restart, cap=4 * H * W * 3 + 4096)
    out, lens, coef = run(enc, frames)
    for b, f in enumerate(frames):
        want, _, geo = je.quantized_coefficients(f, quality, subsampling, restart)
        np.testing.assert_array_equal(coef[b], want, err_msg=f"coefficients of frame {b}")
        data = je.encode_coefficients(want, geo, quality, subsampling, restart)
        assert lens[b] == len(data)
        assert bytes(out[b, :lens[b]]) == data, f"file of frame {b}"
        assert (out[b, lens[b]:] == PATTERN).all(), f"bytes after frame {b}'s file were written"


@pytest.mark.parametrize("subsampling,hw", cases())
def test_kernels_match_the_definition(cuda, subsampling, hw):
    check_exact(batch(hw), 90, subsampling, 4, cuda)


@pytest.mark.parametrize("subsampling,restart", [("4:4:4", 1), ("4:2:0", 1), ("4:2:2", 3)])
def test_entropy_corner_cases_on_the_device(cuda, subsampling, restart):
    """Quality 100 full-scale patterns: ZRL, blocks without EOB, DC category 11, AC category 10,
    stuffed 0xFF (asserted to occur in test_jpeg_encode.py's token counts)."""
    c = corner_frame()
    check_exact(np.stack([c, c[::-1].copy(), 255 - c]), 100, subsampling, restart, cuda)


@pytest.mark.parametrize("restart", [1, 5, 7])
def test_restart_intervals_on_the_device(cuda, restart):
    """48x64 4:2:0, 12 MCUs: 12 intervals (the RST counter wraps) and shorter last intervals."""
    check_exact(batch((48, 64), (5, 6)), 90, "4:2:0", restart, cuda)


def test_more_intervals_than_one_workgroup_of_lanes(cuda):
    """136x200 4:4:4, restart 1: 425 intervals per frame span several 64-lane workgroups of the
    entropy kernels and two rounds of the 256-wide scan."""
    check_exact(batch((136, 200), (8, 9)), 75, "4:4:4", 1, cuda)


def test_overflow_reports_needed_and_spares_the_others(cuda):
    frames = batch((48, 64))
    want = [je.encode_numpy(f, 90, "4:2:0", 4) for f in frames]
    need = [len(w) for w in want]
    assert need[1] > need[0] > need[2]  # noise is the largest
    cap = need[0] + 3  # the camera and the flat frame fit, the noise frame does not
    enc = je.JpegBatchEncoder(3, (48, 64), cuda, 90, "4:2:0", 4, cap=cap)
    assert enc.cap == cap
    out, lens, _ = run(enc, frames)
    assert out.shape == (3, cap)  # nothing exists past cap
    assert lens.tolist() == [need[0], -need[1], need[2]]
    assert (out[1] == PATTERN).all()
    for b in (0, 2):
        assert bytes(out[b, :need[b]]) == want[b] and (out[b, need[b]:] == PATTERN).all()


def test_graph_replay_over_two_batches(cuda):
    from triton_client_amd.pipelines.graph import GraphRunner

    hw = (40, 56)
    enc = je.JpegBatchEncoder(3, hw, cuda, 90, "4:2:0", 4, cap=16384)
    frames = torch.zeros((3, *hw, 3), dtype=torch.uint8, device=cuda)
    out, lens = enc.buffers()
    runner = GraphRunner(lambda: enc.encode_(frames, out, lens, stream=torch.cuda.current_stream()))
    runner.capture()
    assert runner.graph is not None
    for k, seeds in enumerate(((1, 2), (3, 4))):
        b = batch(hw, seeds)
        if k:
            b[2] = frame("noise", *hw, seed=11)  # every length changes between the replays
        frames.copy_(torch.from_numpy(b))
        runner()
        torch.cuda.synchronize()
        o, n = out.cpu().numpy(), lens.cpu().numpy()
        for i, f in enumerate(b):
            want = je.encode_numpy(f, 90, "4:2:0", 4)
            assert n[i] == len(want) and bytes(o[i, :n[i]]) == want


def _jpeg(img, q=90):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=q)
    return buf.getvalue()


def test_live_camera_publishes_the_definitions_file(cuda, caplog):
    from triton_client_amd.inference import LocalDetector2D
    from triton_client_amd.ros import compat

    H, W = 72, 104
    eng = LocalDetector2D(batch=4, device=cuda, letterbox=True, calibrate_target=100.0)
    rgb = [frame("camera", H, W, s) for s in range(3)]
    eng.detect(rgb[:1])  # calibrates the shared model once
    names = [f"c{i}" for i in range(80)]
    cm = [msgs.CompressedImage(header=msgs.Header(seq=i + 1), format="jpeg", data=_jpeg(f)) for i, f in enumerate(rgb)]
    live = eng.live()
    plain = live.process(cm, draw=True, names=names)
    opts = je.JpegOptions(quality=85, subsampling="4:2:0")
    got = live.process(cm, draw=True, names=names, compressed=opts)
    assert sum(len(d) for _, d in plain) > 0
    for m, (im, d0), (c, d1) in zip(cm, plain, got):
        np.testing.assert_array_equal(d1, d0)
        assert isinstance(c, msgs.CompressedImage) and c.header is m.header and c.format == je.FORMAT
        assert bytes(c.data) == je.encode_numpy(compat.imgmsg_to_numpy(im, "rgb8"), 85, "4:2:0", opts.restart)
    # raw Image topics the device converts (their engine keeps its encoding beside the encoder's buffers)
    from triton_client_amd.ops.golden import image_packed_row, rgb8_to_encoding
    for enc in ("bgr8", "yuv422"):
        raw = [msgs.Image(header=msgs.Header(seq=i + 1), height=H, width=W, encoding=enc, is_bigendian=0,
                          step=image_packed_row(W, enc), data=rgb8_to_encoding(f, enc)) for i, f in enumerate(rgb)]
        off = live.process(raw, draw=True, names=names)
        on = live.process(raw, draw=True, names=names, compressed=opts)
        for m, (im, d0), (c, d1) in zip(raw, off, on):
            np.testing.assert_array_equal(d1, d0)
            assert isinstance(c, msgs.CompressedImage) and c.header is m.header
            assert bytes(c.data) == je.encode_numpy(compat.imgmsg_to_numpy(im, "rgb8"), 85, "4:2:0", opts.restart)
    short = msgs.Image(header=msgs.Header(seq=9), height=H, width=W, encoding="bgr8", is_bigendian=0, step=3 * W,
                       data=bytes(10))
    with pytest.raises(ValueError):  # a short payload is still refused before anything is staged
        live.process([short], draw=True, names=names, compressed=opts)
    again = live.process(cm, draw=True, names=names)  # the engine without the option is untouched
    for (im, d0), (im2, d2) in zip(plain, again):
        np.testing.assert_array_equal(d2, d0)
        assert bytes(im2.data) == bytes(im.data)
    # a cap no frame fits (the header alone is over 600 B): the host encodes, once warned
    tiny = je.JpegOptions(quality=85, subsampling="4:2:0", cap=640)
    with caplog.at_level("WARNING", logger="triton_client_amd.live"):
        fb = live.process(cm, draw=True, names=names, compressed=tiny)
    assert sum("encoded on the host" in r.message for r in caplog.records) == 1
    for (c, d1), (_, d0) in zip(fb, plain):
        np.testing.assert_array_equal(d1, d0)
        im = Image.open(io.BytesIO(bytes(c.data)))
        im.load()
        assert im.format == "JPEG" and im.size == (W, H)
