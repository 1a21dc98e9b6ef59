"""Rectification on MI355X: the HIP kernel ``tca_rectify`` (``csrc/kernels/rectify.hip``) against
its specification ``ops.rectify.rectify_numpy``, byte for byte; its argument checks;
``Rectifier.frames``; and the live camera engines that rectify between decode and detector."""
import io

import numpy as np
import pytest
import torch

import rectify_cases as C
from triton_client_amd import _native
from triton_client_amd.ops import golden
from triton_client_amd.ops import rectify as R
from triton_client_amd.ros import msgs
from triton_client_amd.utils.synthetic import camera_frame

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
MODELS = C.DISTORTED + ("identity",)


def _hostile_map(rng, H, W):
    """Entries no camera model gives: anywhere in int32, the extremes included.  Every tap is
    clamped into the frame by the kernel, so this only reads ``src``."""
    q = rng.integers(-2 ** 31, 2 ** 31, (H, W, 2), dtype=np.int64).astype(np.int32)
    near = rng.integers(-70, 32 * (max(H, W) + 2), (H, W, 2)).astype(np.int32)
    q = np.where(rng.random((H, W, 1)) < 0.5, q, near).astype(np.int32)
    ext = np.array([-2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31], np.int32)[:q.size]
    q.reshape(-1)[:ext.size] = ext
    return q


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (33, 130), (48, 64)])
def test_kernel_is_the_specification(cuda, H, W):
    """5 x 7: a frame of 105 bytes, so frame 1 starts misaligned and every fourth pixel group
    straddles rows; 33 x 130: a ragged last group (4290 = 4 * 1072 + 2) and more than one block."""
    rng = np.random.default_rng(H * 1000 + W)
    frame = H * W * 3
    src3 = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    src3[0, 0, 0], src3[-1, -1, -1] = 255, 255  # the extremes at the first and last pixel
    maps = {name: R.rectify_map(C.model(name, H, W)) for name in MODELS}
    maps["hostile"] = _hostile_map(rng, H, W)
    for name, q in maps.items():
        want = [R.rectify_numpy(f, q) for f in src3]  # once per map, shared by every launch below
        qd = torch.from_numpy(q).to(cuda)
        for B in (1, 3):
            for lead in (1, 2, 3):
                sbuf = torch.full((lead + B * frame + 5,), 0xEE, dtype=torch.uint8, device=cuda)
                src = sbuf[lead:lead + B * frame].view(B, H, W, 3)
                src.copy_(torch.from_numpy(src3[:B]).to(cuda))
                for n in (B, B - 1):
                    dbuf = torch.full((lead + B * frame + 19,), SENTINEL, dtype=torch.uint8, device=cuda)
                    dst = dbuf[lead:lead + B * frame].view(B, H, W, 3)
                    R.rectify_(src, dst, qd, n)
                    host = dbuf.cpu().numpy()
                    what = f"{name} {W}x{H} B {B} n {n} lead {lead}"
                    assert (host[:lead] == SENTINEL).all() and (host[lead + n * frame:] == SENTINEL).all(), what
                    for f in range(n):
                        np.testing.assert_array_equal(
                            host[lead + f * frame:lead + (f + 1) * frame].reshape(H, W, 3), want[f],
                            err_msg=f"{what} frame {f}")


def test_aligned_frames_every_chunk_length_and_both_store_paths_agree(cuda):
    """The dword-store path at its best alignment, and ``tca_rectify_variant`` with chunks shorter
    than, equal to and longer than the batch and with byte stores only: the same bytes."""
    H, W, B = 33, 130, 5
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    q = R.rectify_map(C.model("rational", H, W))
    want = np.stack([R.rectify_numpy(f, q) for f in src])
    sd, qd = torch.from_numpy(src).to(cuda), torch.from_numpy(q).to(cuda)
    for variant in (None, (1, 0), (2, 0), (4, 0), (5, 0), (8, 0), (64, 0), (2, 1), (8, 1)):
        dst = torch.full((B, H, W, 3), SENTINEL, dtype=torch.uint8, device=cuda)
        R.rectify_(sd, dst, qd, variant=variant)
        np.testing.assert_array_equal(dst.cpu().numpy(), want, err_msg=f"variant {variant}")
    dst = torch.full((B, H, W, 3), SENTINEL, dtype=torch.uint8, device=cuda)
    with pytest.raises(_native.NativeError):  # chunk < 1 is refused like any bad argument
        R.rectify_(sd, dst, qd, variant=(0, 0))
    torch.cuda.synchronize()
    assert (dst.cpu() == SENTINEL).all()


def test_bad_arguments_launch_nothing(cuda):
    H, W = 6, 8
    src = torch.zeros((2, H, W, 3), dtype=torch.uint8, device=cuda)
    dst = torch.full((2, H, W, 3), SENTINEL, dtype=torch.uint8, device=cuda)
    qbuf = torch.zeros((H * W * 2 + 4,), dtype=torch.int32, device=cuda)
    q = qbuf[:H * W * 2].view(H, W, 2)
    fn = _native.kernels().tca_rectify
    st = _native.stream_ptr(torch.cuda.current_stream())
    s, d, m = src.data_ptr(), dst.data_ptr(), q.data_ptr()
    for args in [(s, d, m, 0, W, 2), (s, d, m, H, 0, 2), (s, d, m, 4097, W, 2), (s, d, m, H, 4097, 2),
                 (s, d, m, -1, W, 2), (s, d, m, H, W, -1),       # sizes and n
                 (0, d, m, H, W, 2), (s, 0, m, H, W, 2), (s, d, 0, H, W, 2),  # null pointers
                 (d, d, m, H, W, 2),                              # src == dst
                 (s, d, m + 4, H, W, 2)]:                         # a map that is not 16-byte aligned
        assert fn(*args, st) != 0, args
    assert fn(s, d, m, H, W, 0, st) == 0  # no frames: nothing to do
    torch.cuda.synchronize()
    assert (dst.cpu() == SENTINEL).all()
    # the Python wrapper refuses what it can see before the launcher does
    with pytest.raises(ValueError, match="same buffer"):
        R.rectify_(dst, dst, q)
    with pytest.raises(ValueError, match="n = 3"):
        R.rectify_(src, dst, q, 3)
    with pytest.raises(ValueError, match="dst"):
        R.rectify_(src, dst[:, :, :4], q)
    with pytest.raises(_native.NativeError):
        R.rectify_(src, dst, qbuf[1:H * W * 2 + 1].view(H, W, 2))
    torch.cuda.synchronize()
    assert (dst.cpu() == SENTINEL).all()


def test_rectifier_frames_on_the_device_and_with_the_host_switch(cuda, monkeypatch):
    monkeypatch.delenv("TCA_DEVICE_RECTIFY", raising=False)
    H, W = 33, 130
    m = C.model("equidistant", H, W)
    rec = R.Rectifier(m, device=cuda)
    assert rec.gpu and rec.kind == "tca_rectify"
    frames = [np.random.default_rng(s).integers(0, 256, (H, W, 3), dtype=np.uint8) for s in range(R.CHUNK + 3)]
    want = [R.rectify_numpy(f, rec.map) for f in frames]
    for got in (rec.frames(frames), rec.frames(frames[:2])):  # two chunks, then a short one in the same buffers
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
    assert rec.frames([]) == []
    with pytest.raises(ValueError, match="64x48.*130x33"):
        rec.frames([np.zeros((48, 64, 3), np.uint8)])
    for bad in (np.zeros((H, W, 3), np.float32), np.zeros((H, W, 4), np.uint8), np.zeros((H, W), np.uint8)):
        with pytest.raises(ValueError, match="uint8"):  # as the definition refuses them, never cast or cut
            rec.frames([bad])
    monkeypatch.setenv("TCA_DEVICE_RECTIFY", "0")
    assert not rec.gpu and rec.kind == "host definition"
    for g, w in zip(rec.frames(frames[:3]), want):
        np.testing.assert_array_equal(g, w)


# ------------------------------------------------------------------------------------ live engines
H, W, B = 48, 64, 4  # the frame size tests/test_encodings_gpu.py runs the camera pipeline at


def _jpeg(img, q=90):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=q)
    return buf.getvalue()


def _packed(rgb, seq=0):
    return msgs.Image(header=msgs.Header(seq=seq), height=H, width=W, encoding="rgb8", step=3 * W,
                      data=np.ascontiguousarray(rgb).tobytes())


def _messages(kind, seeds):
    out = []
    for i, s in enumerate(seeds):
        rgb, hdr = camera_frame(H, W, s), msgs.Header(seq=i + 1)
        if kind == "rgb8":
            out.append(_packed(rgb, i + 1))
        elif kind == "bgr8":
            step = golden.image_packed_row(W, "bgr8") + 4
            out.append(msgs.Image(header=hdr, height=H, width=W, encoding="bgr8", step=step,
                                  data=golden.rgb8_to_encoding(rgb, "bgr8", step)))
        else:
            out.append(msgs.CompressedImage(header=hdr, format="jpeg", data=_jpeg(rgb)))
    return out


def _frame(img_msg):
    assert (img_msg.encoding, img_msg.height, img_msg.width, img_msg.step) == ("rgb8", H, W, 3 * W)
    return np.frombuffer(img_msg.data, np.uint8).reshape(H, W, 3).copy()


@pytest.fixture(scope="module")
def det(cuda):
    from triton_client_amd.inference import LocalDetector2D
    return LocalDetector2D(batch=B, device=cuda, img=320, letterbox=True, calibrate_target=100.0)


@pytest.mark.parametrize("kind,engine_kind", [("rgb8", "frames"), ("bgr8", "raw"), ("jpeg", "jpeg")])
def test_live_camera_rectifies_between_decode_and_detector(det, monkeypatch, kind, engine_kind):
    monkeypatch.delenv("TCA_DEVICE_ENCODINGS", raising=False)
    monkeypatch.delenv("TCA_DEVICE_RECTIFY", raising=False)
    live = det.live()
    assert live.rectify_in
    model = C.model("barrel", H, W)
    rec = det.rectifier(model)
    assert rec is det.rectifier(model) and rec.gpu and rec.map_dev.device.type == "cuda"
    ms = _messages(kind, range(70, 73))  # n = 3 < B
    assert live._key(ms[0])[0] == engine_kind
    plain = live.process(ms, draw=False)  # what the engine sees without the option
    want = [R.rectify_numpy(_frame(im), rec.map) for im, _ in plain]
    assert any((w != _frame(im)).any() for w, (im, _) in zip(want, plain))
    ref = live.process([_packed(w, i + 1) for i, w in enumerate(want)], draw=False)  # fed pre-rectified
    for rep in range(2):  # the second batch replays the captured graph
        got = live.process(ms, draw=False, rectify=rec)
        for m, (im, d), w, (_, r) in zip(ms, got, want, ref):
            assert im.header is m.header
            np.testing.assert_array_equal(_frame(im), w, err_msg=f"{kind} run {rep}")
            np.testing.assert_array_equal(d, r, err_msg=f"{kind} run {rep}")
    assert sum(len(d) for _, d in ref) > 0
    again = live.process(ms, draw=False)  # the engine without the option is untouched
    for (im, d), (im0, d0) in zip(again, plain):
        np.testing.assert_array_equal(_frame(im), _frame(im0))
        np.testing.assert_array_equal(d, d0)


def test_live_camera_refuses_a_frame_of_another_size(det):
    rec = det.rectifier(C.model("barrel", 33, 130))
    with pytest.raises(ValueError, match="64x48.*130x33"):
        det.live().process(_messages("rgb8", [1]), draw=False, rectify=rec)


def test_rectified_frames_leave_as_jpeg_from_the_device_and_from_the_host_fallback(det, monkeypatch, caplog):
    """``rectify`` with ``compressed``: the file is the encoder's definition of the rectified frame;
    with a cap no frame fits, the host encodes -- the rectified frame too, not the sensor's."""
    from triton_client_amd.ops import jpeg_encode as je

    monkeypatch.delenv("TCA_DEVICE_RECTIFY", raising=False)
    live = det.live()
    rec = det.rectifier(C.model("pincushion", H, W))
    names = [f"c{i}" for i in range(80)]
    ms = _messages("rgb8", range(80, 83))  # (raw frames: host and device see the same sensor pixels)
    want = [R.rectify_numpy(camera_frame(H, W, s), rec.map) for s in range(80, 83)]
    plain = live.process(ms, draw=False, rectify=rec)
    opts = je.JpegOptions(quality=85, subsampling="4:2:0", cap=16384)  # room for any 48 x 64 file
    for (c, d), (_, d0), w, m in zip(live.process(ms, draw=False, rectify=rec, compressed=opts), plain, want, ms):
        assert isinstance(c, msgs.CompressedImage) and c.header is m.header
        np.testing.assert_array_equal(d, d0)
        assert bytes(c.data) == je.encode_numpy(w, 85, "4:2:0", opts.restart)
    tiny = je.JpegOptions(quality=85, subsampling="4:2:0", cap=640)  # the header alone is over 600 B
    for draw in (False, True):
        with caplog.at_level("WARNING", logger="triton_client_amd.live"):
            got = live.process(ms, draw=draw, names=names, rectify=rec, compressed=tiny)
        for (c, d), (_, d0), w in zip(got, plain, want):
            np.testing.assert_array_equal(d, d0)
            rgb = w.copy()
            if draw:
                from triton_client_amd.utils.draw import draw_detections
                draw_detections(rgb, d, names, thickness=live.thickness)
            assert bytes(c.data) == je.encode_pil(rgb, 85, "4:2:0")
    assert any("encoded on the host" in r.message for r in caplog.records)
