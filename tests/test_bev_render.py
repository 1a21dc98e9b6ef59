"""The bird's-eye-view host painter (utils/bev.py, the definition of the picture), the
batched op ops.bev.render_bev_, and the picture topic of the 3D drivers and CLIs."""
import os

import numpy as np
import pytest
import torch

from triton_client_amd.ros import compat, msgs
from triton_client_amd.utils import bev
from triton_client_amd.utils.bev import BevView, edge_pixels, render_bev_frame
from triton_client_amd.utils.draw import text_mask

VIEW = BevView((0.0, 6.4), (-2.4, 2.4), 0.1, (-2.0, 2.0))  # 64 rows x 48 columns, 50 levels per metre


def _pts(rows):
    return np.asarray(rows, np.float32).reshape(-1, 4)


def _paint(points=None, boxes=None, scores=None, labels=None, view=VIEW, names=None, z_offset=0.0, n=None,
           count=None):
    k = 0 if boxes is None else len(boxes)
    scores = np.full(k, 0.5, np.float32) if scores is None else scores
    labels = np.ones(k, np.int64) if labels is None else labels
    return render_bev_frame(points, n, boxes, scores, labels, count, view, names, z_offset)


def test_view_geometry():
    assert (VIEW.H, VIEW.W) == (64, 48)
    v = BevView.for_model([0, -39.68, -3, 69.12, 39.68, 1])
    assert (v.H, v.W, v.res, v.z_range) == (691, 794, 0.1, (-3.0, 1.0))
    from triton_client_amd.config.lidar import CenterPointConfig, PointPillarsConfig
    assert BevView.for_model(PointPillarsConfig()) == v
    r = CenterPointConfig().voxel.point_cloud_range
    assert BevView.for_model(CenterPointConfig(), 0.2).H == int(round((r[3] - r[0]) / 0.2))
    with pytest.raises(ValueError):
        BevView((0, 0), (0, 1), 0.1, (0, 1))


def test_points_layer_mapping_levels_and_max():
    # +x up, +y left: (x1, y1) is pixel (0, 0); level = 55 + floor((z - z0) * 50) clamped to 0..200
    img = _paint(_pts([[6.35, 2.35, -2.0, 0], [0.05, -2.35, 0.5, 0], [3.25, 0.05, 5.0, 0], [3.25, 0.05, -9.0, 0],
                       [1.05, 1.05, -1.0, 0], [1.05, 1.05, 1.0, 0], [1.05, 1.05, 0.0, 0]]))
    assert tuple(img[0, 0]) == (55, 55, 55)                       # z0 -> level 55 (not black)
    assert tuple(img[63, 47]) == (180, 180, 180)                  # 55 + floor(2.5 * 50)
    assert tuple(img[31, 23]) == (255, 255, 255)                  # above the range: clamped; max over below
    assert tuple(img[53, 13]) == (205, 205, 205)                  # three points: the maximum level wins
    assert (img.reshape(-1, 3).any(1)).sum() == 4                 # untouched pixels are black


def test_points_shuffle_invariant():
    g = np.random.default_rng(0)
    p = np.c_[g.uniform(-1, 7, 4000), g.uniform(-3, 3, 4000), g.uniform(-3, 3, 4000), g.uniform(0, 1, 4000)]
    p = p.astype(np.float32)
    p[:600, :2] = (3.21, 0.33)  # hundreds in one pixel
    a = _paint(p)
    for s in range(3):
        np.testing.assert_array_equal(_paint(p[np.random.default_rng(s).permutation(len(p))]), a)
    assert a.any()


def test_points_edges_nan_and_out_of_range():
    x0, x1, y0, y1 = 0.0, 6.4, -2.4, 2.4
    f32 = np.float32
    # exactly x1 / y1: row / column 0; exactly x0 / y0: fr = (x1 - x0) * inv_res in fp32, inside only below H / W
    img = _paint(_pts([[x1, y1, 0, 0]]))
    assert img[0, 0, 0] == 155 and img.reshape(-1, 3).any(1).sum() == 1
    fr = (f32(x1) - f32(x0)) * f32(1 / 0.1)
    fc = (f32(y1) - f32(y0)) * f32(1 / 0.1)
    img = _paint(_pts([[x0, 0.05, 0, 0], [3.05, y0, 0, 0]]))
    assert img.reshape(-1, 3).any(1).sum() == int(fr < 64) + int(fc < 48)
    # just outside, NaN and infinite coordinates: skipped
    bad = _pts([[6.45, 0, 0, 0], [-0.05, 0, 0, 0], [3, 2.45, 0, 0], [3, -2.45, 0, 0], [np.nan, 0, 0, 0],
                [3, np.nan, 0, 0], [3, 0, np.nan, 0], [np.inf, 0, 0, 0], [3, -np.inf, 0, 0], [3, 0, np.inf, 0],
                [3, 0, -np.inf, 0], [1e30, 1e30, 0, 0]])
    assert not _paint(bad).any()
    # a NaN in a column the painter does not read does not matter
    assert _paint(_pts([[3, 0, 0, np.nan]])).any()


def test_z_offset_is_removed_in_fp32():
    z = np.float32(0.337)
    p = _pts([[3.05, 0.05, z + np.float32(1.5), 0]])
    want = 55 + int(np.floor(((p[0, 2] - np.float32(1.5)) - np.float32(-2.0)) * np.float32(200 / 4.0)))
    assert _paint(p, z_offset=1.5)[33, 23, 0] == want
    assert _paint(p)[33, 23, 0] != want  # per view, not per frame: nothing is normalised by the frame's points


def test_n_and_count_zero():
    p = _pts([[3.05, 0.05, 0, 0], [1.05, 1.05, 0, 0]])
    b = np.array([[3.2, 0.0, 0, 2.0, 1.0, 1, 0.3]], np.float32)
    assert not _paint(p, n=0).any() and not _paint(None).any() and not _paint(np.zeros((0, 4), np.float32)).any()
    assert _paint(p, n=1).reshape(-1, 3).any(1).sum() == 1
    np.testing.assert_array_equal(_paint(p, b, count=0), _paint(p))          # points only
    np.testing.assert_array_equal(_paint(p, np.zeros((0, 7), np.float32)), _paint(p))
    assert (_paint(None, b) != 0).any() and not _paint(None, b, count=0).any()


def test_edge_rule_is_symmetric_connected_and_integer():
    g = np.random.default_rng(1)
    for _ in range(300):
        ax, ay, bx, by = (int(v) for v in g.integers(-40, 40, 4))
        a, b = edge_pixels(ax, ay, bx, by), edge_pixels(bx, by, ax, ay)
        np.testing.assert_array_equal(a, b)
        n = max(abs(bx - ax), abs(by - ay))
        assert len(a) == n + 1 and a.dtype == np.int64
        ends = {tuple(a[0]), tuple(a[-1])}
        assert ends == {(ax, ay), (bx, by)}
        assert (np.abs(np.diff(a, axis=0)).max(initial=0) <= 1)
    np.testing.assert_array_equal(edge_pixels(2, 3, 2, 3), [[2, 3]])
    np.testing.assert_array_equal(edge_pixels(0, 0, 4, 2), [[0, 0], [1, 1], [2, 1], [3, 2], [4, 2]])  # halves round up


def test_box_edges_colours_and_later_box_wins():
    # yaw 0: corners (+,+) (+,-) (-,-) (-,+) -> the heading side is the top edge (x = cx + dx / 2)
    b = np.array([[3.2, 0.0, 0, 2.0, 1.0, 1, 0.0]], np.float32)
    cor = bev.box_corners_px(b[0], VIEW)
    np.testing.assert_array_equal(cor, [[19, 22], [29, 22], [29, 42], [19, 42]])
    img = np.zeros((64, 48, 3), np.uint8)
    img[:] = _paint(None, b, labels=np.array([2]), count=1)
    lab = bev.label_color(2)
    assert lab == (0, 255, 255) and bev.label_color(12) == lab and bev.label_color(-8) == lab
    assert all(tuple(img[22, c]) == bev.HEADING_COLOR for c in range(19, 30))  # drawn last: it owns its corners
    assert all(tuple(img[42, c]) == lab for c in range(19, 30))
    assert all(tuple(img[r, 19]) == lab and tuple(img[r, 29]) == lab for r in range(23, 43))
    assert not img[23:42, 20:29].any()
    # two overlapping boxes with different labels: the later one wins where their edges cross
    two = np.array([[3.2, 0.0, 0, 2.0, 1.0, 1, 0.0], [3.7, 0.5, 0, 2.0, 1.0, 1, 0.0]], np.float32)
    a = _paint(None, two, labels=np.array([2, 3]), names=["", "", "", ""])
    second = _paint(None, two[1:], labels=np.array([3]), names=["", "", "", ""])
    m = second.any(2)
    np.testing.assert_array_equal(a[m], second[m])
    rev = _paint(None, two[::-1].copy(), labels=np.array([3, 2]), names=["", "", "", ""])
    assert (a != rev).any()


def test_box_outside_is_clipped_never_wrapped_or_clamped():
    # half outside on the right (y < y0) and the top (x > x1)
    b = np.array([[6.2, -2.2, 0, 1.0, 1.0, 1, 0.0]], np.float32)
    cor = bev.box_corners_px(b[0], VIEW)
    assert cor[:, 0].max() >= 48 and cor[:, 1].min() < 0
    img = _paint(None, b, names=[""] * 4)
    want = np.zeros_like(img)
    for e, col in ((1, bev.label_color(1)), (2, bev.label_color(1)), (3, bev.label_color(1)), (0, bev.HEADING_COLOR)):
        for x, y in edge_pixels(*cor[e], *cor[(e + 1) % 4]):
            if 0 <= x < 48 and 0 <= y < 64:
                want[y, x] = col
    np.testing.assert_array_equal(img, want)  # (the names are empty and 0.50 starts right of the image)
    assert not img[:, 0].any() and not img[63].any()  # nothing wrapped to the far side
    assert not (img[:, 47].any(1) & ~want[:, 47].any(1)).any()  # nothing clamped onto the border column
    # wholly outside: nothing at all, label included; NaN box: nothing
    for row in ([20.0, 0.0, 0, 2.0, 1.0, 1, 0.3], [np.nan, 0.0, 0, 2.0, 1.0, 1, 0.3], [3, 0, 0, 2, 1, 1, np.inf]):
        assert not _paint(None, np.array([row], np.float32)).any()
    # absurd sizes neither fail nor hang
    assert _paint(None, np.array([[3.2, 0, 0, 1e30, 1e30, 1, 0.3]], np.float32)).shape == (64, 48, 3)


def test_nine_d_rows_equal_their_seven_d_equivalents():
    g = np.random.default_rng(2)
    b7 = np.c_[g.uniform(1, 5, 6), g.uniform(-2, 2, 6), g.uniform(-1, 1, 6), g.uniform(0.5, 3, (6, 3)),
               g.uniform(-3.2, 3.2, 6)].astype(np.float32)
    b9 = np.c_[b7[:, :6], g.normal(0, 3, (6, 2)), b7[:, 6]].astype(np.float32)
    s, l_ = g.uniform(0, 1, 6).astype(np.float32), g.integers(0, 12, 6)
    a = _paint(None, b7, s, l_, names=["car", "bus"])
    assert a.any()
    np.testing.assert_array_equal(_paint(None, b9, s, l_, names=["car", "bus"]), a)


def test_label_text_position_and_clipping():
    b = np.array([[3.2, 0.0, 0, 2.0, 1.0, 1, 0.0]], np.float32)  # corners cols 19..29, rows 22..42
    names = ["-", "Car", "Pedestrian"]
    img = _paint(None, b, np.array([0.995], np.float32), np.array([1]), names=names)
    from triton_client_amd.utils.draw import label_text
    txt = label_text(1, np.float32(0.995), names)
    m = text_mask(txt)
    x0, y0 = 19 + 2, 22 - 11
    reg = img[y0:y0 + 11, x0:x0 + m.shape[1]]
    w = min(m.shape[1], 48 - x0)
    assert (reg[:, :w][m[:, :w]] == bev.label_color(1)).all()
    assert not reg[:, :w][~m[:, :w]].any()  # the cell is above the box: nothing else there
    assert m.shape[1] > w                    # and this one already runs off the right edge: clipped
    # scores: half-even from the exact value; ids outside the table print as numbers
    for sc, lab, want in ((0.005, 1, "Car 0.00"), (1.0, 2, "Pedestrian 1.00"), (0.125, 7, "7 0.12"),
                          (0.5, -3, "-3 0.50")):
        assert label_text(lab, np.float32(sc), names) == want
    # off the top edge: the cell origin is clamped to row 0 and drawn over the box
    top = np.array([[6.1, 1.5, 0, 0.4, 0.4, 1, 0.0]], np.float32)
    cor = bev.box_corners_px(top[0], VIEW)
    assert 0 <= cor[:, 1].min() < 11
    img = _paint(None, top, names=names)
    m = text_mask(label_text(1, np.float32(0.5), names))
    x0 = int(cor[:, 0].min()) + 2
    w = min(m.shape[1], 48 - x0)
    assert (img[0:11, x0:x0 + w][m[:, :w]] == bev.label_color(1)).all()
    # a min corner left of the image: the text is clipped on the left as well
    left = np.array([[3.2, 2.6, 0, 1.0, 1.0, 1, 0.0]], np.float32)
    cor = bev.box_corners_px(left[0], VIEW)
    assert cor[:, 0].min() < -2 and (cor[:, 0] >= 0).any()
    img = _paint(None, left, names=names)
    x0, y0 = int(cor[:, 0].min()) + 2, int(cor[:, 1].min()) - 11
    assert (img[y0:y0 + 11, 0:m.shape[1] + x0][m[:, -x0:]] == bev.label_color(1)).all()


def test_render_bev_op_cpu_path_and_validation():
    from triton_client_amd.ops.bev import render_bev_

    g = np.random.default_rng(3)
    B, N, K = 2, 200, 4
    pts = np.c_[g.uniform(0, 6.4, (B * N)), g.uniform(-2.4, 2.4, B * N), g.uniform(-2, 2, B * N),
                g.uniform(0, 1, B * N)].astype(np.float32).reshape(B, N, 4)
    n = np.array([N, 17], np.int32)
    box = np.tile(np.array([3.2, 0.0, 0, 2.0, 1.0, 1, 0.4], np.float32), (B, K, 1))
    box[:, :, 0] += np.arange(K, dtype=np.float32)[None] * 0.6
    score = g.uniform(0, 1, (B, K)).astype(np.float32)
    label = g.integers(0, 5, (B, K)).astype(np.int32)
    count = np.array([K, 2], np.int32)
    t = [torch.from_numpy(a) for a in (pts, n, box, score, label, count)]
    out = torch.full((B, 64, 48, 3), 7, dtype=torch.uint8)
    assert render_bev_(out, *t, VIEW, names=["a", "b"], z_offset=0.25) is out
    for b in range(B):
        np.testing.assert_array_equal(out[b].numpy(), render_bev_frame(pts[b], n[b], box[b], score[b], label[b],
                                                                       count[b], VIEW, ["a", "b"], 0.25))
    # a padded row stride
    wide = torch.zeros((B, 64, 50, 3), dtype=torch.uint8)
    render_bev_(wide[:, :, :48], *t, VIEW, names=["a", "b"], z_offset=0.25)
    assert torch.equal(wide[:, :, :48], out) and not wide[:, :, 48:].any()
    bad = [
        (torch.zeros((B, 64, 40, 3), dtype=torch.uint8), t),                           # not the view's size
        (torch.zeros((B, 64, 48, 3), dtype=torch.float32), t),
        (out, [t[0][:, :, :2].contiguous()] + t[1:]),                                  # F < 3
        (out, [t[0], t[1], t[2][:, :, :6].contiguous()] + t[3:]),                      # D < 7
        (out, [t[0], t[1].long()] + t[2:]),
        (out, t[:4] + [t[4].long(), t[5]]),
        (out, t[:3] + [t[3][:, :2], t[4], t[5]]),
        (torch.zeros((B, 64, 96, 3), dtype=torch.uint8)[:, :, ::2], t),                # pixels not packed
    ]
    for o, args in bad:
        with pytest.raises(ValueError):
            render_bev_(o, *args, VIEW)


# ------------------------------------------------------------------ driver and CLI
class _Engine:
    """A CPU engine: deterministic boxes from the cloud's own points (all labels, all scores)."""
    from triton_client_amd.config.lidar import PointPillarsConfig
    cfg = PointPillarsConfig()
    names = list(cfg.class_names)
    z_offset, normalize, label_base = 1.5, True, 1

    def detect(self, clouds):
        out = []
        for c in clouds:
            p = compat.cloud_to_numpy(c)
            k = min(6, len(p))
            box = np.zeros((k, 7), np.float32)
            box[:, 0] = 4.0 + 2.0 * np.arange(k) + np.float32(abs(p[0, 0]) % 1.0)  # in view, cloud dependent
            box[:, 1] = -6.0 + 2.0 * np.arange(k)
            box[:, 3:6] = (3.9, 1.6, 1.5)
            box[:, 6] = np.linspace(-1.0, 2.0, k)
            out.append({"pred_boxes": box, "pred_scores": np.linspace(0.2, 0.9, k).astype(np.float32),
                        "pred_labels": (np.arange(k) % 3 + 1).astype(np.int64)})
        return out


def _clouds(n=3):
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep
    out = []
    for s in range(n):
        pts = lidar_sweep(LidarSpec(rings=8, azimuth_steps=128, sensor_height=1.8), s)
        out.append(compat.create_cloud_xyzi(np.frombuffer(pts.tobytes(), np.float32).reshape(-1, 4),
                                            msgs.Header(seq=s + 1, stamp=msgs.Time(5, s), frame_id="os")))
    return out


@pytest.mark.parametrize("batch,workers", [(1, 1), (2, 2)])
def test_driver_publishes_one_picture_per_cloud(batch, workers):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.inference.engines import Detector3D
    from triton_client_amd.utils.bev import label_names
    from triton_client_amd.ros import rosmsg
    from triton_client_amd.ros.bus import TopicBus

    clouds = _clouds(4)
    view = BevView((0.0, 20.0), (-10.0, 10.0), 0.25, (-3.0, 1.0))
    runs = {}
    for topic in (None, "/pc_bev"):
        bus, eng = TopicBus(), _Engine()
        boxes, pics = [], []
        compat.Subscriber("/pc_out", msgs.BoundingBoxArray, boxes.append, bus=bus)
        compat.Subscriber("/pc_bev", msgs.Image, pics.append, bus=bus)
        drv = RosInference3D(engine=eng, params={"sub_topic": "/pc", "pub_topic": "/pc_out"}, bus=bus, batch=batch,
                             workers=workers, queue_size=64, bev_topic=topic, bev_view=view)
        drv.start_inference(spin=False)
        pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
        for c in clouds:
            pub.publish(c)
        drv.stop()
        bus.close()
        runs[topic] = ([rosmsg.serialize(m) for m in boxes], pics)
        assert len(boxes) == len(clouds)
    assert runs[None][1] == [] and runs[None][0] == runs["/pc_bev"][0]  # the box message: byte-identical
    pics = runs["/pc_bev"][1]
    assert [p.header.seq for p in pics] == [c.header.seq for c in clouds]
    eng = _Engine()
    names = label_names(eng.names, 1)
    assert names == ["-", "Car", "Pedestrian", "Cyclist"]
    for p, c, pred in zip(pics, clouds, eng.detect(clouds)):
        assert p.header is c.header or (p.header.stamp, p.header.frame_id) == (c.header.stamp, c.header.frame_id)
        assert (p.height, p.width, p.encoding, p.step) == (view.H, view.W, "rgb8", 3 * view.W)
        pts = compat.cloud_to_numpy(c, normalize_intensity=True, z_offset=1.5)
        want = render_bev_frame(pts, None, pred["pred_boxes"], pred["pred_scores"], pred["pred_labels"], None, view,
                                names, 1.5)
        got = compat.imgmsg_to_numpy(p, "rgb8")
        np.testing.assert_array_equal(got, want)
        assert (got == bev.HEADING_COLOR).all(2).any() and (got == bev.label_color(3)).all(2).any()  # every label
        np.testing.assert_array_equal(Detector3D.render_bev(eng, [c], [pred], view)[0], want)


def test_cli_flags_and_bag3d_bev_out(tmp_path):
    from triton_client_amd.cli import bag3d, main3d, record
    from triton_client_amd.ros import Bag

    f = main3d.parse_args([])
    assert f.bev_topic == "" and f.bev_res == 0.1
    f = main3d.parse_args(["--bev-topic", "/bev", "--bev-res", "0.2"])
    assert (f.bev_topic, f.bev_res) == ("/bev", 0.2)
    assert bag3d.parse_args(["--bag", "x"]).bev_out == ""
    assert bag3d.parse_args(["--bag", "x", "--bev-out", "d", "--bev-res", "0.5"]).bev_out == "d"
    pc = str(tmp_path / "pc.bag")
    assert record.main([pc, "--frames", "3", "--no-camera", "--lidar", "--rings", "16", "--columns", "256"]) == 0
    out, ob = str(tmp_path / "bev"), str(tmp_path / "o.bag")
    assert bag3d.main(["--bag", pc, "--engine", "local", "--device", "cpu", "--out-bag", ob, "--labels", "all",
                       "--score-thresh", "0", "--bev-out", out, "--bev-res", "0.2"]) == 0
    assert sorted(os.listdir(out)) == ["0000.png", "0001.png", "0002.png"]
    from PIL import Image
    img = np.asarray(Image.open(os.path.join(out, "0001.png")))
    assert img.shape == (346, 397, 3) and img.any()
    with Bag(ob) as b:
        pics = [m for _, m, _ in b.read_messages(topics=["/detections_3d/bev"])]
    assert len(pics) == 3 and (pics[1].height, pics[1].width) == (346, 397)
    np.testing.assert_array_equal(compat.imgmsg_to_numpy(pics[1], "rgb8"), img)
    # off by default: no directory, no topic
    ob2 = str(tmp_path / "o2.bag")
    assert bag3d.main(["--bag", pc, "--engine", "local", "--device", "cpu", "--out-bag", ob2, "--max-frames", "1"]) == 0
    with Bag(ob2) as b:
        assert not [1 for _ in b.read_messages(topics=["/detections_3d/bev"])]
