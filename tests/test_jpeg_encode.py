"""The JPEG encoder's definition (ops/jpeg_encode.py) on the CPU: round trips through the
project's own entropy decoder, entropy corner cases counted in the token stream, equality
with libjpeg (PIL) on MCU-multiple sizes, and the drivers' compressed output on the CPU engine."""
import io
import os

import numpy as np
import pytest
from PIL import Image

from triton_client_amd.ops import jpeg_encode as je
from triton_client_amd.ops.jpeg import decode_coefficients
from triton_client_amd.ros import Bag, msgs
from triton_client_amd.utils.synthetic import camera_frame

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "ros1_sensors.bag")
SIZES = [(16, 16), (8, 8), (24, 40), (17, 33), (48, 64)]  # H x W; 8x8 with 4:4:4 only


def frame(kind: str, H: int, W: int, seed: int = 0) -> np.ndarray:
    if kind == "camera":  # camera_frame needs >= 27 pixels a side: crop a larger one
        return np.ascontiguousarray(camera_frame(max(H, 64), max(W, 64), seed)[:H, :W])
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def cases():
    return [(ss, hw) for ss in je.SUBSAMPLINGS for hw in SIZES if hw != (8, 8) or ss == "4:4:4"]


def corner_frame() -> np.ndarray:
    """32x16 grey frame of full-scale patterns: at quality 100 it holds a +-full-scale (4,4)
    checkerboard (AC category 10), white next to black blocks (DC difference category 11), the
    finest checkerboard (coefficient 63 non-zero, no EOB) and long zero runs (ZRL)."""
    y, x = np.mgrid[0:8, 0:8]
    chk = np.sign(np.cos((2 * x + 1) * 4 * np.pi / 16)) * np.sign(np.cos((2 * y + 1) * 4 * np.pi / 16)) > 0
    a = np.where(chk, 255, 0).astype(np.uint8)
    img = np.zeros((16, 32), np.uint8)
    img[:8, :8], img[:8, 8:16], img[:8, 16:24], img[:8, 24:] = a, 255, 0, 255 - a
    img[8:, :8] = ((x + y) & 1) * 255
    img[8:, 8:16] = np.where(x == 7, 255, 0)
    return np.repeat(img[..., None], 3, 2)


def entropy_stats(rgb, quality, subsampling, restart):
    coef, _, geo = je.quantized_coefficients(rgb, quality, subsampling, restart)
    segs = je.scan_tokens(coef, geo, restart)
    toks = [t for s in segs for t in s]
    data = je.encode_numpy(rgb, quality, subsampling, restart)
    body = data[len(je.header_bytes(geo.width, geo.height, quality, subsampling, restart)):]
    return dict(zrl=sum(t[0] in (1, 3) and t[1] == 0xF0 for t in toks),
                dc11=sum(t[0] in (0, 2) and t[1] == 11 for t in toks),
                ac10=sum(t[0] in (1, 3) and (t[1] & 15) == 10 for t in toks),
                coef63=int((coef[:, 63] != 0).sum()), nseg=len(segs), stuffed=body.count(b"\xff\x00"),
                blocks=[sum(1 for t in s if t[0] in (0, 2)) for s in segs], data=data, coef=coef, geo=geo)


def assert_round_trip(rgb, quality=90, subsampling="4:2:0", restart=4):
    data = je.encode_numpy(rgb, quality, subsampling, restart)
    want, q, geo = je.quantized_coefficients(rgb, quality, subsampling, restart)
    got, gq, ggeo = decode_coefficients(data)
    assert ggeo == geo and geo.gpu_ok
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(gq[:2].astype(np.int32), q)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == "RGB" and im.size == (rgb.shape[1], rgb.shape[0])
    return data


@pytest.mark.parametrize("kind", ["camera", "noise"])
@pytest.mark.parametrize("subsampling,hw", cases())
def test_round_trip_through_the_projects_decoder(subsampling, hw, kind):
    assert_round_trip(frame(kind, *hw, seed=3), 90, subsampling, 4)


def test_header_depends_on_its_five_values_only():
    a, b = frame("camera", 24, 40, 1), frame("noise", 24, 40, 2)
    h = je.header_bytes(40, 24, 75, "4:2:2", 3)
    assert je.encode_numpy(a, 75, "4:2:2", 3).startswith(h) and je.encode_numpy(b, 75, "4:2:2", 3).startswith(h)
    assert h[:4] == b"\xff\xd8\xff\xe0" and h[6:11] == b"JFIF\x00"
    markers, i = [], 2
    while i < len(h):
        markers.append(h[i + 1])
        i += 2 + int.from_bytes(h[i + 2:i + 4], "big")
    assert markers == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA] and i == len(h)
    for bad in (dict(quality=0), dict(quality=101), dict(subsampling="4:1:1"), dict(restart=0)):
        with pytest.raises(ValueError):
            je.header_bytes(40, 24, **bad)


def test_huffman_tables_are_the_standard_ones_libjpeg_writes():
    def dht(data):
        out, i = b"", 2
        while data[i + 1] != 0xDA:
            n = int.from_bytes(data[i + 2:i + 4], "big")
            if data[i + 1] == 0xC4:
                out += data[i + 4:i + 2 + n]
            i += 2 + n
        return out
    rgb = frame("camera", 32, 32)
    assert dht(je.encode_numpy(rgb)) == dht(je.encode_pil(rgb)) and len(dht(je.encode_numpy(rgb))) == 416


@pytest.mark.parametrize("subsampling", ["4:4:4", "4:2:0"])
def test_entropy_corner_cases_occur_and_round_trip(subsampling):
    rgb = corner_frame()
    s = entropy_stats(rgb, 100, subsampling, 1)
    assert s["zrl"] > 0, "no run of >= 16 zeros"
    assert s["coef63"] > 0, "no block ending without EOB"
    assert s["dc11"] > 0 and s["ac10"] > 0, "no DC category 11 / AC category 10"
    assert s["stuffed"] > 0, "no stuffed 0xFF"
    assert_round_trip(rgb, 100, subsampling, 1)
    if subsampling == "4:4:4":
        assert s["nseg"] == 8  # RST0..RST6, then the last interval: below the wrap


@pytest.mark.parametrize("restart,nseg,last", [(1, 12, 6), (4, 3, 24), (5, 3, 12), (7, 2, 30)])
def test_restart_intervals(restart, nseg, last):
    """48x64 4:2:0 is 12 MCUs of 6 blocks: more than 8 intervals (the RST counter wraps), an
    interval that divides the MCU count, and two that leave a shorter last interval."""
    rgb = frame("noise", 48, 64, 5)
    s = entropy_stats(rgb, 90, "4:2:0", restart)
    assert s["nseg"] == nseg and s["blocks"][-1] == last and s["stuffed"] > 0
    if restart in (5, 7):
        assert s["blocks"][-1] < s["blocks"][0]
    data = s["data"]
    marks = [data[i + 1] for i in range(len(je.header_bytes(64, 48, 90, "4:2:0", restart)), len(data) - 2)
             if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert marks == [0xD0 + (i & 7) for i in range(nseg - 1)]
    assert_round_trip(rgb, 90, "4:2:0", restart)


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("quality", [50, 90])
@pytest.mark.parametrize("subsampling", list(je.SUBSAMPLINGS))
@pytest.mark.parametrize("kind,hw", [("camera", (32, 48)), ("noise", (32, 48)), ("camera", (64, 64)), ("noise", (64, 64))])
def test_coefficients_equal_libjpeg(kind, hw, subsampling, quality):
    """The definition copies libjpeg's integer path: on MCU-multiple sizes its quantised
    coefficients and tables equal those of PIL's file exactly (measured: 0 of 146432 coefficients
    differ over these cases), so the decoded pictures have the same PSNR (gap 0)."""
    rgb = frame(kind, *hw, seed=7)
    pil = je.encode_pil(rgb, quality, subsampling)
    want, wq, wgeo = decode_coefficients(pil)
    got, q, geo = je.quantized_coefficients(rgb, quality, subsampling)
    assert geo == wgeo
    np.testing.assert_array_equal(wq[:2].astype(np.int32), q)
    np.testing.assert_array_equal(got, want)
    ours = np.asarray(Image.open(io.BytesIO(je.encode_numpy(rgb, quality, subsampling))).convert("RGB"))
    theirs = np.asarray(Image.open(io.BytesIO(pil)).convert("RGB"))
    assert psnr(ours, rgb) >= psnr(theirs, rgb)  # gap 0: the coefficients are equal


def test_encoder_op_refuses_the_cpu():
    import torch

    with pytest.raises(ValueError, match="GPU"):
        je.JpegBatchEncoder(1, (16, 16), torch.device("cpu"))


# ---------------------------------------------------------------------------- drivers, CPU engine
class _Engine:
    names = ["a", "b"]

    def detect(self, frames):
        return [np.array([[1, 2, 10, 12, 0.5 + float(f[0, 0, 0]) / 512, 1]], np.float32) for f in frames]


def _drive(compressed, n=5):
    from triton_client_amd.inference import RosInference
    from triton_client_amd.ros import compat
    from triton_client_amd.ros.bus import TopicBus

    bus = TopicBus()
    got = {"/det": [], "/det/compressed": [], "/det/detections": []}
    for t in got:
        bus.subscribe(t, got[t].append)
    drv = RosInference(engine=_Engine(), params={"sub_topic": "/cam", "pub_topic": "/det"}, bus=bus, queue_size=None,
                       compressed=compressed)
    drv.start_inference(spin=False)
    sent = [compat.numpy_to_imgmsg(frame("camera", 40, 56, s), "rgb8", header=msgs.Header(seq=s + 1, frame_id="cam"))
            for s in range(n)]
    for m in sent:
        bus.publish("/cam", m)
    bus.wait_idle(30)
    drv.stop(drain=True)
    bus.wait_idle(30)
    bus.close()
    return sent, got


def test_ros_driver_publishes_compressed_instead_of_raw():
    from triton_client_amd.utils.draw import draw_detections

    opts = je.JpegOptions(quality=80, subsampling="4:2:2")
    sent, got = _drive(opts)
    _, plain = _drive(None)
    assert got["/det"] == [] and len(plain["/det"]) == len(sent) and plain["/det/compressed"] == []
    assert len(got["/det/compressed"]) == len(sent)
    for m, c in zip(sent, got["/det/compressed"]):
        assert isinstance(c, msgs.CompressedImage) and c.header is m.header and c.format == je.FORMAT
        rgb = np.frombuffer(m.data, np.uint8).reshape(40, 56, 3)
        want = draw_detections(rgb.copy(), _Engine().detect([rgb])[0], _Engine.names)
        assert bytes(c.data) == je.encode_pil(want, 80, "4:2:2")
        assert Image.open(io.BytesIO(bytes(c.data))).size == (56, 40)
    a = [(d.header.seq, [(x.results[0].id, x.results[0].score, x.bbox.size_x) for x in d.detections])
         for d in got["/det/detections"]]
    b = [(d.header.seq, [(x.results[0].id, x.results[0].score, x.bbox.size_x) for x in d.detections])
         for d in plain["/det/detections"]]
    assert a == b and len(a) == len(sent)


def test_bag2d_writes_decodable_compressed_messages(tmp_path):
    from triton_client_amd.cli import bag2d

    ob = str(tmp_path / "cam_out.bag")
    assert bag2d.main(["--bag", FIX, "--engine", "local", "--device", "cpu", "--out", "", "--out-bag", ob,
                       "--frames-per-step", "2", "--publish-compressed", "--jpeg-quality", "85"]) == 0
    with Bag(ob) as b:
        info = b.get_type_and_topic_info()
        out = [m for _, m, _ in b.read_messages(topics=["/aver_01/camera_color/detection/compressed"])]
        src = [m for _, m, _ in b.read_messages(topics=["/camera/color/image_raw"])]
    assert "/aver_01/camera_color/detection" not in info
    assert info["/aver_01/camera_color/detection/compressed"]["type"] == "sensor_msgs/CompressedImage"
    assert len(out) == len(src) == 3
    for m, s in zip(out, src):
        im = Image.open(io.BytesIO(bytes(m.data)))
        im.load()
        assert im.format == "JPEG" and im.size == Image.open(io.BytesIO(bytes(s.data))).size
        assert m.header.seq == s.header.seq


def test_flags_parse_and_default_to_off():
    from triton_client_amd.cli import bag2d, main as main2d, main3d
    from triton_client_amd.cli.common import jpeg_options

    for mod, base in ((main2d, []), (bag2d, ["--bag", "x.bag"])):
        f = mod.parse_args(base)
        assert f.publish_compressed is False and (f.jpeg_quality, f.jpeg_subsampling) == (90, "4:2:0")
        assert jpeg_options(f) is None
        f = mod.parse_args(base + ["--publish-compressed", "--jpeg-quality", "70", "--jpeg-subsampling", "4:4:4"])
        assert jpeg_options(f) == je.JpegOptions(quality=70, subsampling="4:4:4")
    assert not hasattr(main3d.parse_args([]), "publish_compressed")  # the 2D group only
    with pytest.raises(SystemExit):
        main3d.parse_args(["--publish-compressed"])


def test_ring_engine_refuses_the_option():
    from triton_client_amd.inference import RosInference
    from triton_client_amd.parallel.dp import DataParallelDetector2D

    ring = DataParallelDetector2D.__new__(DataParallelDetector2D)  # the class decides; no ranks are started
    params = {"sub_topic": "/cam", "pub_topic": "/det"}
    with pytest.raises(ValueError, match="compressed"):
        RosInference(engine=ring, params=params, compressed=je.JpegOptions())
    RosInference(engine=ring, params=params)  # without the option it builds as before
