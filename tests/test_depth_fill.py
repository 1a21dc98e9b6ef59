"""K38, the definition: ``fill_numpy`` (ops/depth_image.py) against its brute force, by hand, and through the driver."""
import numpy as np
import pytest

from test_depth_image import KITTI_H, KITTI_W
from test_range2d import CAL, KITTI_P, _Engine, _rig_messages
from triton_client_amd.ops import depth_image as D
from triton_client_amd.ops import range2d as R
from triton_client_amd.ros import compat, msgs

E = D.EMPTY
RADII = {"defaults": (2, 3, 15, 2), "maximum": (4, 7, 15, 2), "no hole": (2, 0, 15, 2), "no large": (2, 3, 0, 2),
         "no median": (2, 3, 15, 0), "k 1": (1, 3, 15, 2)}


def options(W, H, enc="16UC1", radii=RADII["defaults"]):
    k, h, g, m = radii
    return D.DepthOptions(W, H, enc, fill=k, fill_hole=h, fill_large=g, fill_median=m)


def keys(rng, W, H, enc, density=0.05):
    vals = rng.integers(1, 65536, (H, W)).astype(np.uint32) if enc == "16UC1" else \
        rng.uniform(0.5, 80.0, (H, W)).astype(np.float32).view(np.uint32)
    return np.where(rng.random((H, W)) < density, vals, np.uint32(E)).astype(np.uint32)


@pytest.mark.parametrize("radii", sorted(RADII))
@pytest.mark.parametrize("encoding", ("16UC1", "32FC1"))
def test_definition_equals_the_brute_force(encoding, radii):
    rng = np.random.default_rng(len(radii))
    for W, H, density in ((1, 1, 1.0), (5, 3, 0.3), (41, 37, 0.05)):
        o = options(W, H, encoding, RADII[radii])
        plane = keys(rng, W, H, encoding, density)
        got = D.fill_numpy(plane, o)
        assert got.dtype == np.uint32 and got.shape == (H, W) and (got == D.fill_ref(plane, o)).all(), f"{W}x{H}"
        # a stage selects, never computes: every output key is an input key within the halo
        halo = 3 * o.fill + o.fill_hole + o.fill_large + o.fill_median
        for y, x in zip(*np.nonzero(got != E)):
            assert got[y, x] in plane[max(0, y - halo):y + halo + 1, max(0, x - halo):x + halo + 1]
        assert (D.fill_numpy(np.full((H, W), E, np.uint32), o) == E).all()  # an empty plane stays empty


def test_a_single_key_by_hand():
    plane = np.full((41, 41), E, np.uint32)
    plane[20, 20] = 7
    for k in (1, 2, 4):
        dx, dy = np.meshgrid(np.arange(41) - 20, np.arange(41) - 20)
        diamond = np.abs(dx) + np.abs(dy) <= k
        # stage 1 makes the diamond; the closing leaves it: every pixel outside it lies in a square that misses it
        got = D.fill_numpy(plane, options(41, 41, radii=(k, 0, 0, 0)))
        assert ((got == 7) == diamond).all() and ((got == E) | (got == 7)).all()
        # the small-hole fill grows it by the square h: extents k + h both ways, corners cut as the diamond's are
        got = D.fill_numpy(plane, options(41, 41, radii=(k, 3, 0, 0)))
        ys, xs = np.nonzero(got == 7)
        assert (ys.min(), ys.max(), xs.min(), xs.max()) == (17 - k, 23 + k, 17 - k, 23 + k)
        assert got[17 - k, 20 - 3:20 + 4].tolist() == [7] * 7 and got[17 - k, 20 - 4] == E


def test_the_large_fill_reaches_exactly_g():
    g = 5
    o = options(40, 9, radii=(1, 0, g, 0))
    plane = np.full((9, 40), E, np.uint32)
    plane[3:6, 3:6] = 9  # closed, this block stays a block with the diamond's tips: its last column is 6
    got = D.fill_numpy(plane, o)
    assert got[4, 6] == 9 and got[4, 6 + g] == 9 and got[4, 6 + g + 1] == E


def test_option_refusals_and_fill_off():
    o = D.DepthOptions(8, 6)
    assert (o.fill, o.fill_hole, o.fill_large, o.fill_median) == (0, 3, 15, 2)
    for field, bad in (("fill", (-1, 5, 1.5, None, True)), ("fill_hole", (-1, 8, "3")), ("fill_large", (-1, 16, 2.0)),
                       ("fill_median", (-1, 3, None))):
        for v in bad:
            with pytest.raises(ValueError, match=field):
                D.DepthOptions(8, 6, **{field: v})
    # fill = 0: the other radii are not read, and the image is the unfilled one
    clouds, _ = _rig_messages()
    six = D.DepthOptions(KITTI_W, KITTI_H, "16UC1", 1000.0, 0.5, 1)
    off = D.DepthOptions(KITTI_W, KITTI_H, fill=0, fill_hole=0, fill_large=0, fill_median=0)
    pts = R.cloud_xyzi(clouds[0])
    assert D.depth_numpy(pts, CAL.M, off).tobytes() == D.depth_numpy(pts, CAL.M, six).tobytes()
    im = D.DepthImager("cpu")  # two planes a launch with fill on: the cut halves, and stays where it was with it off
    many = [clouds[0]] * 10
    assert [len(p) for p in im._parts(list(range(10)), many, D.DepthOptions(4096, 4096))] == [4, 4, 2]
    assert [len(p) for p in im._parts(list(range(10)), many, D.DepthOptions(4096, 4096, fill=2))] == [2] * 5


@pytest.mark.parametrize("fill", (0, 2))
def test_driver_publishes_the_filled_image(fill):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.ros.bus import TopicBus

    clouds, _ = _rig_messages()
    o = D.DepthOptions(KITTI_W, KITTI_H, fill=fill)
    bus = TopicBus()
    got = []
    compat.Subscriber("/depth", msgs.Image, lambda m: got.append((m.header.seq, bytes(m.data))), bus=bus)
    drv = RosInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=4, workers=2,
                         queue_size=64, depth_topic="/depth", depth_options=o, calibration=CAL)
    drv.start_inference(spin=False)
    pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
    for c in clouds:
        pub.publish(c)
    drv.stop()
    bus.close()
    plain = D.DepthOptions(KITTI_W, KITTI_H)  # the first six fields alone
    want = []
    for c in clouds:
        image = D.depth_numpy(R.cloud_xyzi(c), CAL.M, plain)
        if fill:  # depth_message(fill_numpy(...)): the fill on the unfilled image's keys
            plane = np.where(image == 0, np.uint32(E), image.astype(np.uint32))
            image = D.image_of_keys(D.fill_numpy(plane, o), o)
            assert (image != 0).sum() > 2 * (plane != E).sum()
        want.append((c.header.seq, bytes(D.depth_message(c, image, o).data)))
    assert got == want


def test_flags_and_usage_errors(tmp_path, capsys):
    from triton_client_amd.cli import bag3d, main3d

    calib = tmp_path / "rig.yaml"
    calib.write_text(f"projection: {KITTI_P.tolist()}\nlidar_to_camera: {CAL.T.tolist()}\n")
    args = ["--depth-topic", "/d", "--calib", str(calib), "--depth-size", "64x48"]
    for mod, pre in ((main3d, []), (bag3d, ["--bag", "x"])):
        assert mod.parse_args(pre + args).depth_options == D.DepthOptions(64, 48)
        assert mod.parse_args(pre + args + ["--depth-fill", "2"]).depth_options == D.DepthOptions(64, 48, fill=2)
        every = "--depth-fill 1 --depth-fill-hole 0 --depth-fill-large 7 --depth-fill-median 1".split()
        assert mod.parse_args(pre + args + every).depth_options == options(64, 48, radii=(1, 0, 7, 1))
        for bad, word in (("--depth-fill 2", "--depth-topic"), ("+ --depth-fill-hole 2", "--depth-fill K"),
                          ("+ --depth-fill-large 2", "--depth-fill K"), ("+ --depth-fill-median 1", "--depth-fill K"),
                          ("+ --depth-fill 0 --depth-fill-median 1", "--depth-fill K"), ("+ --depth-fill 5", "fill"),
                          ("+ --depth-fill 2 --depth-fill-large 16", "fill_large")):
            with pytest.raises(SystemExit) as e:  # ("+": behind the depth topic's own flags)
                mod.parse_args(pre + (args + bad.split()[1:] if bad[0] == "+" else bad.split()))
            assert e.value.code == 2 and word in capsys.readouterr().err, bad
