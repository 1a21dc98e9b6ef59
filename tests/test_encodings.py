"""sensor_msgs/Image encodings -> rgb8 on the host: the NumPy specification
(``ops.golden.image_to_rgb8``), ``compat.imgmsg_to_numpy`` over it, the synthetic
inverse and the recorder's ``--encoding``."""
import numpy as np
import pytest

from triton_client_amd.ops import golden
from triton_client_amd.ros import compat, msgs

BAYER = ("bayer_rggb8", "bayer_bggr8", "bayer_gbrg8", "bayer_grbg8")
# colours of pixels (0,0), (0,1), (1,0), (1,1) as channel indices, spelled out from the ROS names
BAYER_TILE = {"bayer_rggb8": ((0, 1), (1, 2)), "bayer_bggr8": ((2, 1), (1, 0)),
              "bayer_gbrg8": ((1, 2), (0, 1)), "bayer_grbg8": ((1, 0), (2, 1))}


def _msg(data, h, w, step, enc, big=0):
    return msgs.Image(height=h, width=w, encoding=enc, is_bigendian=big, step=step, data=bytes(data))


def _rows(body: np.ndarray, pad: int) -> bytes:
    """[H, packed] uint8 -> payload with ``pad`` junk bytes after every row."""
    h = body.shape[0]
    return np.concatenate([body, np.full((h, pad), 0xEE, np.uint8)], axis=1).tobytes()


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("enc", ["rgb8", "bgr8", "rgba8", "bgra8", "mono8"])
def test_legacy_encodings(enc, pad):
    h, w = 5, 7
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    alpha = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    if enc == "rgb8":
        body, want = rgb, rgb
    elif enc == "bgr8":
        body, want = rgb[..., ::-1], rgb
    elif enc == "rgba8":
        body, want = np.concatenate([rgb, alpha], 2), rgb
    elif enc == "bgra8":
        body, want = np.concatenate([rgb[..., ::-1], alpha], 2), rgb
    else:
        body = rgb[..., :1]
        want = np.concatenate([body, body, body], 2)
    body = np.ascontiguousarray(body).reshape(h, -1)
    step = body.shape[1] + pad
    data = _rows(body, pad)
    np.testing.assert_array_equal(compat.imgmsg_to_numpy(_msg(data, h, w, step, enc), "rgb8"), want)
    np.testing.assert_array_equal(golden.image_to_rgb8(data, h, w, step, enc), want)
    np.testing.assert_array_equal(compat.imgmsg_to_numpy(_msg(data, h, w, step, enc), "bgr8"), want[..., ::-1])


@pytest.mark.parametrize("hw", [(2, 2), (3, 5), (6, 8)])
@pytest.mark.parametrize("enc", BAYER)
def test_bayer_constant_colour_and_own_site(enc, hw):
    h, w = hw
    colour = np.array([201, 37, 118], np.uint8)
    flat = np.broadcast_to(colour, (h, w, 3))
    out = golden.image_to_rgb8(golden.rgb8_to_encoding(flat, enc), h, w, w, enc)
    np.testing.assert_array_equal(out, flat)
    # every site's own colour passes through
    cfa = np.random.default_rng(2).integers(0, 256, (h, w), dtype=np.uint8)
    cfa[0, 0], cfa[-1, -1] = 0, 255
    out = golden.image_to_rgb8(cfa.tobytes(), h, w, w, enc)
    tile = BAYER_TILE[enc]
    for y in range(h):
        for x in range(w):
            assert out[y, x, tile[y & 1][x & 1]] == cfa[y, x], (y, x)


def test_bayer_rggb_worked_by_hand():
    cfa = np.array([[10, 200, 31, 7],       # R G R G
                    [90, 60, 255, 80],      # G B G B
                    [0, 101, 110, 33],      # R G R G
                    [130, 17, 150, 255]],   # G B G B
                   np.uint8)
    out = golden.image_to_rgb8(cfa.tobytes(), 4, 4, 4, "bayer_rggb8")
    # (0,0) corner, R: G = (90+90+200+200+2)>>2, B = (4*60+2)>>2 (row -1 is row 1, column -1 is column 1)
    assert out[0, 0].tolist() == [10, 145, 60]
    # (0,1) top edge, G on a red row: R = (10+31+1)>>1, B = (60+60+1)>>1
    assert out[0, 1].tolist() == [21, 200, 60]
    # (1,1) interior, B: G = (200+101+90+255+2)>>2, R = (10+31+0+110+2)>>2
    assert out[1, 1].tolist() == [38, 162, 60]
    # (1,2) interior, G on a blue row: B = (60+80+1)>>1, R = (31+110+1)>>1
    assert out[1, 2].tolist() == [71, 255, 70]
    # (2,2) interior, R: G = (255+150+101+33+2)>>2, B = (60+80+17+255+2)>>2
    assert out[2, 2].tolist() == [110, 135, 103]
    # (3,0) left/bottom edge, G on a blue row: B = (17+17+1)>>1, R = (0+0+1)>>1 (row 4 is row 2)
    assert out[3, 0].tolist() == [0, 130, 17]
    # (3,3) corner, B: G = (33+33+150+150+2)>>2, R = (4*110+2)>>2
    assert out[3, 3].tolist() == [110, 92, 255]


def _macropixels(enc, y0, u, y1, v):
    order = (u, y0, v, y1) if enc == "yuv422" else (y0, u, y1, v)
    return np.stack([np.asarray(a, np.uint8) for a in order], axis=-1)


@pytest.mark.parametrize("enc", ["yuv422", "yuv422_yuy2"])
def test_yuv422(enc):
    # grey ramp: U = V = 128, all 256 luma values
    ys = np.arange(256)
    mp = _macropixels(enc, ys[0::2], np.full(128, 128), ys[1::2], np.full(128, 128))
    out = golden.image_to_rgb8(mp.tobytes(), 1, 256, 512, enc)
    want = [min(255, (max(y - 16, 0) * 1220542 + 524288) >> 20) for y in range(256)]
    assert want[16] == 0 and want[235] == 255 and want[0] == 0 and want[255] == 255
    for c in range(3):
        assert out[0, :, c].tolist() == want
    # both clamps of R
    hi = golden.image_to_rgb8(_macropixels(enc, [255], [128], [255], [255]).tobytes(), 1, 2, 4, enc)
    lo = golden.image_to_rgb8(_macropixels(enc, [0], [128], [0], [0]).tobytes(), 1, 2, 4, enc)
    assert hi[0, :, 0].tolist() == [255, 255] and lo[0, :, 0].tolist() == [0, 0]
    # one macropixel by hand: U = 100, V = 200 (u = -28, v = 72), Y0 = 50, Y1 = 180
    #   y0 = 34 * 1220542 = 41498428, y1 = 164 * 1220542 = 200168888
    #   R: + 1673527 * 72 = 120493944; G: - 852492 * 72 + 409993 * 28 = -49899620; B: - 2116026 * 28 = -59248728
    #   pixel 0: (162516660, -7876904, -17226012) >> 20 = (154, -8, -17) -> (154, 0, 0)
    #   pixel 1: (321187120, 150793556, 141444448) >> 20 = (306, 143, 134) -> (255, 143, 134)
    one = golden.image_to_rgb8(_macropixels(enc, [50], [100], [180], [200]).tobytes(), 1, 2, 4, enc)
    assert one[0].tolist() == [[154, 0, 0], [255, 143, 134]]
    with pytest.raises(ValueError, match=enc):
        golden.image_to_rgb8(bytes(6), 1, 3, 6, enc)
    with pytest.raises(ValueError, match=enc):
        compat.imgmsg_to_numpy(_msg(bytes(6), 1, 3, 6, enc))


@pytest.mark.parametrize("big", [0, 1])
def test_mono16(big):
    vals = [0, 65535, 128, 129, 257, 32768]
    data = np.array(vals, ">u2" if big else "<u2").tobytes()
    out = golden.image_to_rgb8(data, 1, len(vals), 2 * len(vals), "mono16", big)
    want = [0, 255, 0, 1, 1, (32768 + 128) // 257]
    for c in range(3):
        assert out[0, :, c].tolist() == want
    np.testing.assert_array_equal(compat.imgmsg_to_numpy(_msg(data, 1, len(vals), 2 * len(vals), "mono16", big)), out)


@pytest.mark.parametrize("enc", ["rgb16", "32FC1", "bayer_rggb16", "nv12", ""])
def test_unknown_encoding_is_a_value_error_naming_it(enc):
    with pytest.raises(ValueError, match=repr(enc)):
        compat.imgmsg_to_numpy(_msg(bytes(64), 2, 2, 16, enc))
    with pytest.raises(ValueError, match=repr(enc)):
        golden.image_to_rgb8(bytes(64), 2, 2, 16, enc)


def test_rejected_geometries():
    with pytest.raises(ValueError, match="bayer_gbrg8"):
        golden.image_to_rgb8(bytes(8), 1, 8, 8, "bayer_gbrg8")
    with pytest.raises(ValueError, match="bayer_gbrg8"):
        golden.image_to_rgb8(bytes(8), 8, 1, 1, "bayer_gbrg8")
    with pytest.raises(ValueError, match="step"):
        golden.image_to_rgb8(bytes(64), 2, 4, 11, "bgr8")
    with pytest.raises(ValueError, match="data"):
        golden.image_to_rgb8(bytes(20), 2, 4, 12, "bgr8")


@pytest.mark.parametrize("enc", sorted(golden.IMAGE_ENCODINGS))
def test_synthetic_inverse_round_trip(enc):
    """rgb8_to_encoding writes H * step bytes image_to_rgb8 reads back: exactly for the byte
    permutations, at the own-colour sites for Bayer, as a grey image for mono and close to the
    source for a smooth YUV frame (it is a data generator, so the YUV bound is loose)."""
    from triton_client_amd.utils.synthetic import camera_frame

    h, w = 6, 8
    rgb = camera_frame(48, 64, 3)[10:10 + h, 20:20 + w]
    step = golden.image_packed_row(w, enc) + 3
    data = golden.rgb8_to_encoding(rgb, enc, step=step, is_bigendian=1)
    assert len(data) == h * step
    out = golden.image_to_rgb8(data, h, w, step, enc, 1)
    if enc in ("rgb8", "bgr8", "rgba8", "bgra8"):
        np.testing.assert_array_equal(out, rgb)
    elif enc.startswith("bayer"):
        tile = BAYER_TILE[enc]
        for y in range(h):
            for x in range(w):
                c = tile[y & 1][x & 1]
                assert out[y, x, c] == rgb[y, x, c]
    elif enc.startswith("mono"):
        c = rgb.astype(int)
        grey = (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8
        np.testing.assert_array_equal(out, np.repeat(grey[..., None], 3, 2))
    else:
        flat = np.broadcast_to(np.array([90, 140, 60], np.uint8), (h, w, 3))
        back = golden.image_to_rgb8(golden.rgb8_to_encoding(flat, enc), h, w, 2 * w, enc)
        assert np.abs(back.astype(int) - flat).max() <= 3


def test_recorder_writes_encoded_bag(tmp_path):
    from triton_client_amd.cli import record
    from triton_client_amd.ros import Bag
    from triton_client_amd.utils.synthetic import camera_frame

    path = str(tmp_path / "bayer.bag")
    assert record.main([path, "--encoding", "bayer_rggb8", "--cam", "48x64", "--frames", "3", "--row-pad", "4"]) == 0
    with Bag(path) as bag:
        got = [m for _, m, _ in bag.read_messages()]
    assert len(got) == 3
    tile = BAYER_TILE["bayer_rggb8"]
    sel = np.array([[tile[y & 1][x & 1] for x in range(64)] for y in range(48)])
    for s, m in enumerate(got):
        assert (m.encoding, m.height, m.width, m.step) == ("bayer_rggb8", 48, 64, 68)
        rgb = compat.imgmsg_to_numpy(m)
        np.testing.assert_array_equal(rgb, golden.image_to_rgb8(m.data, 48, 64, 68, "bayer_rggb8"))
        src = camera_frame(48, 64, s)
        np.testing.assert_array_equal(np.take_along_axis(rgb, sel[..., None], 2),
                                      np.take_along_axis(src, sel[..., None], 2))
