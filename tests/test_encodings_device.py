"""The raw-``Image`` conversion op (``ops.image.image_to_rgb8``) on CPU tensors -- the twin of
the HIP kernel, ``golden.image_to_rgb8`` frame by frame -- its argument checks, and which
messages the live camera engine keys for the device conversion."""
import numpy as np
import pytest
import torch

from triton_client_amd.inference.live import LiveCamera
from triton_client_amd.ops import golden
from triton_client_amd.ops.image import image_frame_bytes, image_to_rgb8
from triton_client_amd.ros import msgs


def _payloads(enc, h, w, pad, batch, seed=0):
    """[batch, frame_stride] uint8 random payloads (stride: the frame's bytes rounded up to 16)."""
    step = golden.image_packed_row(w, enc) + pad
    need = image_frame_bytes(h, w, step, enc)
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (batch, (need + 15) // 16 * 16), dtype=np.uint8)
    return src, step, need


@pytest.mark.parametrize("enc", sorted(golden.IMAGE_ENCODINGS))
def test_cpu_op_is_golden_per_frame(enc):
    h, w, pad = 5, 6, 5
    src, step, need = _payloads(enc, h, w, pad, 3)
    for big in ((0, 1) if enc == "mono16" else (0,)):
        out = torch.full((3, h, w, 3), 0x5A, dtype=torch.uint8)
        got = image_to_rgb8(torch.from_numpy(src), h, w, step, enc, big, out=out, n=2)
        assert got is out
        for f in range(2):
            np.testing.assert_array_equal(out[f].numpy(), golden.image_to_rgb8(src[f, :need], h, w, step, enc, big))
        assert (out[2] == 0x5A).all()  # row n is left as it was
    full = image_to_rgb8(torch.from_numpy(src), h, w, step, enc)
    assert full.shape == (3, h, w, 3) and full.dtype == torch.uint8
    np.testing.assert_array_equal(full[2].numpy(), golden.image_to_rgb8(src[2, :need], h, w, step, enc))


def test_op_refuses_what_the_specification_refuses():
    src = torch.zeros((2, 256), dtype=torch.uint8)
    with pytest.raises(ValueError, match="yuv422_yuy2"):
        image_to_rgb8(src, 2, 3, 6, "yuv422_yuy2")       # odd width
    with pytest.raises(ValueError, match="bayer_grbg8"):
        image_to_rgb8(src, 1, 8, 8, "bayer_grbg8")       # one row
    with pytest.raises(ValueError, match="bgr8.*step"):
        image_to_rgb8(src, 2, 4, 11, "bgr8")             # step below the packed row
    for enc in ("rgb16", "nv12", "32FC1"):
        with pytest.raises(ValueError, match=repr(enc)):
            image_to_rgb8(src, 2, 2, 16, enc)
    with pytest.raises(ValueError, match="mono8.*data"):
        image_to_rgb8(src, 20, 20, 20, "mono8")          # frames of 400 B in rows of 256 B


def _image(enc, h, w, pad=0, big=0):
    step = golden.image_packed_row(w, enc) + pad
    return msgs.Image(height=h, width=w, encoding=enc, is_bigendian=big, step=step, data=bytes(h * step))


def test_ring_payload_is_the_message_as_sent_and_file_sharding_finds_it(tmp_path, monkeypatch):
    """Rank 0 of a device-path node hands the ring the payload unconverted under a KIND_RAW key;
    when the payload is a view of a mapped bag, the ring records its file offset like any other."""
    import mmap
    from types import SimpleNamespace

    from triton_client_amd.parallel import dp  # noqa: F401  (ring_dp is imported through it)
    from triton_client_amd.parallel import ring_dp
    from triton_client_amd.parallel.host_ring import FileMaps

    monkeypatch.delenv("TCA_DEVICE_ENCODINGS", raising=False)
    h, w, enc, step = 4, 6, "yuv422", 15
    need = image_frame_bytes(h, w, step, enc)
    body = np.random.default_rng(5).integers(0, 256, h * step, dtype=np.uint8).tobytes()
    path = tmp_path / "payloads.bin"
    path.write_bytes(bytes(100) + body + bytes(7))
    with open(path, "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    FileMaps.register(str(path), mm)
    try:
        m = msgs.Image(height=h, width=w, encoding=enc, step=step, data=memoryview(mm)[100:100 + h * step])
        node = SimpleNamespace(gpu=True, local=SimpleNamespace(live=lambda: LiveCamera.__new__(LiveCamera)))
        key, payload, same = ring_dp.DataParallelDetector2D._prepare(node, m)
        assert same is m and key == (ring_dp.KIND_RAW, h, w, golden.IMAGE_ENCODINGS[enc], step, 0)
        assert bytes(payload) == body[:need] and len(payload) == need == h * step - 3
        assert FileMaps.locate(payload, len(payload)) == (str(path), 100)
        short = msgs.Image(height=h, width=w, encoding=enc, step=step, data=body[:need - 1])
        with pytest.raises(ValueError, match=enc):
            ring_dp.DataParallelDetector2D._prepare(node, short)
        # a host-engine rank 0 keeps the rgb8-rows path
        node.gpu = False
        key, payload, _ = ring_dp.DataParallelDetector2D._prepare(node, m)
        assert key == (ring_dp.KIND_FRAMES, h, w)
        np.testing.assert_array_equal(payload, golden.image_to_rgb8(body, h, w, step, enc))
    finally:
        FileMaps.unregister(mm)


def test_live_camera_key(monkeypatch):
    monkeypatch.delenv("TCA_DEVICE_ENCODINGS", raising=False)
    live = LiveCamera.__new__(LiveCamera)  # _key needs no detector
    assert live._key(_image("bayer_rggb8", 4, 6, pad=2, big=1)) == ("raw", (4, 6), ("bayer_rggb8", 8, 0))
    assert live._key(_image("rgb8", 4, 6, pad=3)) == ("raw", (4, 6), ("rgb8", 21, 0))
    assert live._key(_image("mono16", 4, 6, big=1)) == ("raw", (4, 6), ("mono16", 12, 1))
    assert live._key(_image("bgr8", 4, 6)) == ("raw", (4, 6), ("bgr8", 18, 0))
    assert live._key(_image("rgb8", 4, 6)) == ("frames", (4, 6), None)
    # an encoding the specification does not know stays on the host path, which refuses it by name
    unknown = msgs.Image(height=4, width=6, encoding="rgb16", step=36, data=bytes(144))
    assert live._key(unknown) == ("frames", (4, 6), None)
    with pytest.raises(ValueError, match="'rgb16'"):
        LiveCamera.host_rgb(unknown, (4, 6))
    monkeypatch.setenv("TCA_DEVICE_ENCODINGS", "0")
    for m in (_image("bayer_rggb8", 4, 6, pad=2), _image("rgb8", 4, 6, pad=3), _image("mono16", 4, 6, big=1),
              _image("rgb8", 4, 6)):
        assert live._key(m) == ("frames", (4, 6), None)
