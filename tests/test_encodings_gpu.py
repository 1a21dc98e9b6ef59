"""Raw ``Image`` encodings on MI355X: the HIP conversion kernel (``csrc/kernels/encodings.hip``)
against its specification ``golden.image_to_rgb8``, byte for byte, and the live engines that
upload a payload as the sensor sent it and convert it on the device."""
import numpy as np
import pytest
import torch

from triton_client_amd import _native
from triton_client_amd.ops import golden
from triton_client_amd.ops.image import image_frame_bytes, image_to_rgb8
from triton_client_amd.ros import msgs
from triton_client_amd.utils.synthetic import camera_frame

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
# (encoding, is_bigendian): mono16 in both byte orders
CASES = [(e, 0) for e in sorted(golden.IMAGE_ENCODINGS)] + [("mono16", 1)]


def _geometries(enc):
    """2x2; an odd width (even for YUV); a multiple of the 4 pixels a thread makes; a ragged
    tail (non-YUV: 19 = 4 * 4 + 3); more than one block of 256 threads with a ragged tail."""
    yuv = enc.startswith("yuv")
    return [(2, 2), (3, 6) if yuv else (3, 5), (6, 8)] + ([] if yuv else [(5, 19)]) + [(33, 130)]


def _random_frames(rng, n, need):
    src = rng.integers(0, 256, (n, need), dtype=np.uint8)
    src[:, 0], src[:, -1] = 0, 255       # the extremes at the first and last sample of a frame
    src[-1, 0], src[-1, -1] = 255, 0
    return src


def _yuv_by_hand(enc):
    """The macropixels tests/test_encodings.py::test_yuv422 works by hand: both clamps of R and
    (Y0, U, Y1, V) = (50, 100, 180, 200) -> (154, 0, 0), (255, 143, 134); as a 2 x 6 image."""
    mp = [(255, 128, 255, 255), (0, 128, 0, 0), (50, 100, 180, 200)] * 2
    order = (lambda y0, u, y1, v: (u, y0, v, y1)) if enc == "yuv422" else (lambda y0, u, y1, v: (y0, u, y1, v))
    return np.array([order(*m) for m in mp], np.uint8).reshape(2, 12)


@pytest.mark.parametrize("enc,big", CASES)
def test_kernel_is_the_specification(cuda, enc, big):
    rng = np.random.default_rng(golden.IMAGE_ENCODINGS[enc] + 100 * big)
    for (h, w) in _geometries(enc):
        for pad in (0, 5):  # 5: every row but the first starts at an odd address
            step = golden.image_packed_row(w, enc) + pad
            need = image_frame_bytes(h, w, step, enc)
            stride = (need + 15) // 16 * 16
            src = np.full((3, stride), 0xEE, np.uint8)
            src[:, :need] = _random_frames(rng, 3, need)
            got = image_to_rgb8(torch.from_numpy(src).to(cuda), h, w, step, enc, big)
            got = got.cpu().numpy()
            for f in range(3):
                np.testing.assert_array_equal(got[f], golden.image_to_rgb8(src[f, :need], h, w, step, enc, big),
                                              err_msg=f"{enc} {w}x{h} pad {pad} frame {f}")
    if enc.startswith("yuv"):
        body = _yuv_by_hand(enc)
        got = image_to_rgb8(torch.from_numpy(body.reshape(1, -1)).to(cuda), 2, 6, 12, enc).cpu().numpy()[0]
        for row in got:
            assert row[:4, 0].tolist() == [255, 255, 0, 0]  # both clamps of R
            assert row[4:].tolist() == [[154, 0, 0], [255, 143, 134]]
        np.testing.assert_array_equal(got, golden.image_to_rgb8(body.tobytes(), 2, 6, 12, enc))


@pytest.mark.parametrize("enc,big", CASES)
def test_source_exactly_sized_and_sentinel_intact(cuda, enc, big):
    """Frames lie back to back with nothing after a frame's last row, and the source tensor ends
    with the last frame's last sample: a load past a frame has nowhere legal to go.  The
    destination is a view at an odd offset of a larger buffer that must keep its sentinel."""
    rng = np.random.default_rng(7 + golden.IMAGE_ENCODINGS[enc])
    n = 3
    for (h, w) in _geometries(enc):
        step = golden.image_packed_row(w, enc) + 5
        need = image_frame_bytes(h, w, step, enc)
        src = _random_frames(rng, n, need)
        dev_src = torch.from_numpy(src).to(cuda)
        assert dev_src.numel() == n * need and dev_src.stride(0) == need
        frame = h * w * 3
        for lead in (16, 13):  # a dword-aligned and an odd destination
            big_buf = torch.full((lead + n * frame + 19,), SENTINEL, dtype=torch.uint8, device=cuda)
            out = big_buf[lead:lead + n * frame].view(n, h, w, 3)
            image_to_rgb8(dev_src, h, w, step, enc, big, out=out)
            host = big_buf.cpu().numpy()
            assert (host[:lead] == SENTINEL).all() and (host[lead + n * frame:] == SENTINEL).all()
            for f in range(n):
                np.testing.assert_array_equal(host[lead + f * frame:lead + (f + 1) * frame].reshape(h, w, 3),
                                              golden.image_to_rgb8(src[f], h, w, step, enc, big),
                                              err_msg=f"{enc} {w}x{h} lead {lead} frame {f}")


def test_only_n_frames_are_written(cuda):
    h, w, enc = 6, 8, "bgr8"
    src = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (3, h * w * 3), dtype=np.uint8)).to(cuda)
    out = torch.full((3, h, w, 3), SENTINEL, dtype=torch.uint8, device=cuda)
    image_to_rgb8(src, h, w, w * 3, enc, out=out, n=2)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:2], src[:2].cpu().numpy().reshape(2, h, w, 3)[..., ::-1])
    assert (got[2] == SENTINEL).all()


def test_bad_arguments_launch_nothing(cuda):
    src = torch.zeros((2, 4096), dtype=torch.uint8, device=cuda)
    out = torch.full((2, 4, 6, 3), SENTINEL, dtype=torch.uint8, device=cuda)
    for h, w, step, enc in [(4, 6, 64, "rgb16"), (4, 5, 10, "yuv422"), (1, 6, 6, "bayer_rggb8"), (4, 6, 17, "bgr8")]:
        with pytest.raises(ValueError, match=enc):
            image_to_rgb8(src, h, w, step, enc, out=out)
    # the launcher itself: nonzero, and no kernel runs
    fn = _native.kernels().tca_image_to_rgb8
    st = _native.stream_ptr(torch.cuda.current_stream())
    bad = [(12, 4, 6, 64), (-1, 4, 6, 64),  # unknown code
           (6, 4, 5, 10), (7, 4, 5, 10),    # odd-width YUV
           (8, 1, 6, 6), (11, 4, 1, 1),     # Bayer under 2x2
           (1, 4, 6, 17), (5, 4, 6, 11)]    # step below the packed row
    for code, h, w, step in bad:
        assert fn(src.data_ptr(), 4096, step, h, w, code, 0, out.data_ptr(), 72, 2, st) != 0, (code, h, w, step)
    assert fn(src.data_ptr(), 1 << 30, 18, 4, 6, 1, 0, out.data_ptr(), 1 << 30, 2, st) != 0  # 2 * 2^30 B: 32-bit indices
    assert fn(src.data_ptr(), 4096, 18, 4, 6, 1, 0, out.data_ptr(), 71, 2, st) != 0          # output frames overlap
    torch.cuda.synchronize()
    assert (out.cpu() == SENTINEL).all()


# ------------------------------------------------------------------------------------ live engines
H, W, PAD, B = 48, 64, 4, 4


def _messages(enc, seeds, pad=PAD):
    out = []
    for i, s in enumerate(seeds):
        step = golden.image_packed_row(W, enc) + pad
        data = golden.rgb8_to_encoding(camera_frame(H, W, s), enc, step)
        out.append(msgs.Image(header=msgs.Header(seq=i + 1), height=H, width=W, encoding=enc, step=step, data=data))
    return out


def _spec(m):
    return golden.image_to_rgb8(m.data, m.height, m.width, m.step, m.encoding, m.is_bigendian)


def _packed(rgb, seq=0):
    return msgs.Image(header=msgs.Header(seq=seq), height=H, width=W, encoding="rgb8", step=3 * W,
                      data=np.ascontiguousarray(rgb).tobytes())


def _frame(img_msg):
    assert (img_msg.encoding, img_msg.height, img_msg.width, img_msg.step) == ("rgb8", H, W, 3 * W)
    return np.frombuffer(img_msg.data, np.uint8).reshape(H, W, 3)


@pytest.fixture(scope="module")
def det(cuda):
    from triton_client_amd.inference import LocalDetector2D
    return LocalDetector2D(batch=B, device=cuda, img=320, letterbox=True, calibrate_target=100.0)


def _count_host_rgb(monkeypatch):
    from triton_client_amd.inference.live import LiveCamera
    calls, orig = [], LiveCamera.host_rgb

    def counted(m, hw=None):
        calls.append(m)
        return orig(m, hw)
    monkeypatch.setattr(LiveCamera, "host_rgb", staticmethod(counted))
    return calls


def test_live_camera_converts_on_the_device(det, monkeypatch):
    monkeypatch.delenv("TCA_DEVICE_ENCODINGS", raising=False)
    live = det.live()
    for enc in ("bayer_grbg8", "yuv422"):
        ms = _messages(enc, range(10, 13))  # n = 3 < B
        calibrating = det.calibrate_target is not None
        with monkeypatch.context() as mp:
            calls = _count_host_rgb(mp)
            got = live.process(ms, draw=False)
        # the calibration sample of the first engine built on random-init weights, nothing else
        assert len(calls) == (1 if calibrating else 0), (enc, len(calls))
        assert det.calibrate_target is None
        want_rgb = [_spec(m) for m in ms]
        for (im, _), m, w in zip(got, ms, want_rgb):
            assert im.header is m.header
            np.testing.assert_array_equal(_frame(im), w)
        ref = live.process([_packed(w, i) for i, w in enumerate(want_rgb)], draw=False)
        for (_, d), (_, r) in zip(got, ref):
            np.testing.assert_array_equal(d, r)
        if calibrating:
            assert sum(len(d) for _, d in got) > 0


def test_mixed_batch_keeps_message_order_and_host_switch_agrees(det, monkeypatch):
    monkeypatch.delenv("TCA_DEVICE_ENCODINGS", raising=False)
    live = det.live()
    ms = [_packed(camera_frame(H, W, 20), 1), _messages("bgr8", [21])[0], _messages("mono8", [22])[0],
          _messages("bgr8", [23], pad=0)[0], _packed(camera_frame(H, W, 24), 5), _messages("mono8", [25])[0]]
    got = live.process(ms, draw=False)
    kinds = {live._key(m)[0] for m in ms}
    assert kinds == {"frames", "raw"}
    for (im, d), m in zip(got, ms):
        assert im.header is m.header
        np.testing.assert_array_equal(_frame(im), _spec(m))
        (im1, d1), = live.process([m], draw=False)
        np.testing.assert_array_equal(_frame(im1), _frame(im))
        np.testing.assert_array_equal(d1, d)
    # the host conversion, switched on: the same frames and detections
    monkeypatch.setenv("TCA_DEVICE_ENCODINGS", "0")
    assert {live._key(m)[0] for m in ms} == {"frames"}
    calls = _count_host_rgb(monkeypatch)
    host = live.process(ms, draw=False)
    assert len(calls) == 4
    for (im, d), (imh, dh) in zip(got, host):
        np.testing.assert_array_equal(_frame(imh), _frame(im))
        np.testing.assert_array_equal(dh, d)


def test_short_payload_is_refused_before_staging(det, monkeypatch):
    monkeypatch.delenv("TCA_DEVICE_ENCODINGS", raising=False)
    m = _messages("bgr8", [30])[0]
    m.data = m.data[:len(m.data) - PAD - 1]  # one byte short of the last row's last pixel
    with pytest.raises(ValueError, match="bgr8"):
        det.live().process([m], draw=False)
    ok = _messages("bgr8", [30])[0]
    ok.data = ok.data[:len(ok.data) - PAD]   # the last row's padding need not exist
    (im, _), = det.live().process([ok], draw=False)
    np.testing.assert_array_equal(_frame(im), _spec(ok))


def test_slot_rotation_keeps_every_batch_exact(det, monkeypatch):
    """2 x slots + 1 batches of different content, submitted back to back through one "raw"
    engine and only then collected: a staging slot or an input set released before its H2D and
    conversion were done would show another batch's pixels."""
    monkeypatch.delenv("TCA_DEVICE_ENCODINGS", raising=False)
    live = det.live()
    first = _messages("bayer_grbg8", [40])
    eng = live._engine(live._key(first[0]), False, (), first[0])
    assert eng.kind == "raw"
    batches = [_messages("bayer_grbg8", range(50 + 10 * b, 50 + 10 * b + 1 + b % B)) for b in range(2 * live.slots + 1)]
    pending = [eng.submit(b) for b in batches]
    for b, p in zip(batches, pending):
        for (im, _), m in zip(eng.finish(p), b):
            np.testing.assert_array_equal(_frame(im), _spec(m))


def test_remote_ingest_converts_on_the_device(cuda):
    from triton_client_amd.inference.remote_live import _Ingest
    ms = _messages("bayer_bggr8", range(60, 63))
    ing = _Ingest("raw", (H, W), ("bayer_bggr8", ms[0].step, 0), cuda, 2)
    frames = ing(ms)
    torch.cuda.synchronize()
    assert frames.is_cuda and tuple(frames.shape) == (3, H, W, 3)
    for f, m in zip(frames.cpu().numpy(), ms):
        np.testing.assert_array_equal(f, _spec(m))
