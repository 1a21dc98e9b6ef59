"""The host half of the device bird's-eye-view renderer (ops/bev.py): the box table the kernel
draws from, the CPU renderer, the layouts the kernel takes and the TCA_DEVICE_BEV switch."""
import warnings

import numpy as np
import pytest

from triton_client_amd.ops import bev as obev
from triton_client_amd.ops.points_in_boxes import CloudLayout, cloud_layout
from triton_client_amd.ros import compat, msgs
from triton_client_amd.utils import bev
from triton_client_amd.utils.bev import BevView
from triton_client_amd.utils.draw import label_text

VIEW = BevView((0.0, 6.4), (-2.4, 2.4), 0.1, (-2.0, 2.0))  # 64 rows x 48 columns
F = np.float32


def _check_table(boxes, scores, labels, count, names):
    tab, text = obev.bev_box_table(boxes, scores, labels, count, VIEW, names)
    k = len(boxes) if count is None else min(count, len(boxes))
    assert tab.shape == (k, obev.ROW) and tab.dtype == np.int32 and isinstance(text, bytes)
    end = 0
    for i in range(k):
        cor = bev.box_corners_px(boxes[i], VIEW)
        r, g, b = bev.label_color(labels[i])
        assert tab[i, 9] == r | (g << 8) | (b << 16)
        assert tab[i, 8] == (cor is not None)
        if cor is None:
            assert tab[i, 11] == 0 and not tab[i, :8].any()
            continue
        np.testing.assert_array_equal(tab[i, :8].reshape(4, 2), cor)
        inside = ((cor[:, 0] >= 0) & (cor[:, 0] < VIEW.W) & (cor[:, 1] >= 0) & (cor[:, 1] < VIEW.H)).any()
        want = label_text(int(labels[i]), scores[i], names) if inside else ""
        assert text[tab[i, 10]:tab[i, 10] + tab[i, 11]].decode("ascii") == want
        assert tab[i, 10] == end  # the texts follow each other in box order
        end += tab[i, 11]
    assert end == len(text)
    return tab, text


def test_box_table_rows():
    b7 = np.array([[3.2, 0.0, 0, 2.0, 1.0, 1, 0.4],       # inside
                   [np.nan, 0.0, 0, 2.0, 1.0, 1, 0.3],    # a NaN corner: not valid
                   [20.0, 0.0, 0, 2.0, 1.0, 1, 0.3],      # every corner outside: no text
                   [6.2, -2.2, 0, 1.0, 1.0, 1, 0.0],      # crosses two borders: still labelled
                   [1.0, 1.0, 0, 0.5, 0.5, 1, -2.0]], F)
    sc = np.array([0.99, 0.5, 0.7, 0.125, 0.005], F)
    lab = np.array([1, 2, 1, 7, -3])                       # 7 and -3 are outside names: the decimal id
    names = ["-", "Car", "Pedestrian"]
    tab, text = _check_table(b7, sc, lab, None, names)
    assert tab[:, 8].tolist() == [1, 0, 1, 1, 1] and tab[2, 11] == 0 and tab[1, 11] == 0
    assert text == b"Car 0.997 0.12-3 0.00"
    # 9-d rows (yaw at index 8) equal their 7-d equivalents
    b9 = np.c_[b7[:, :6], np.full((5, 2), 9.0, F), b7[:, 6]].astype(F)
    t9, x9 = _check_table(b9, sc, lab, None, names)
    np.testing.assert_array_equal(t9, tab)
    assert x9 == text
    # count < K, count 0, no boxes, no names
    t3, x3 = _check_table(b7, sc, lab, 3, names)
    np.testing.assert_array_equal(t3, tab[:3])
    assert x3 == b"Car 0.99"
    assert obev.bev_box_table(b7, sc, lab, 0, VIEW, names)[0].shape == (0, 12)
    assert obev.bev_box_table(np.zeros((0, 7), F), [], [], None, VIEW)[1] == b""
    assert obev.bev_box_table(None, None, None, None, VIEW)[0].shape == (0, 12)
    assert _check_table(b7, sc, lab, None, None)[1].startswith(b"1 0.99")
    with pytest.raises(ValueError):
        obev.bev_box_table(np.zeros((2, 6), F), [0, 0], [0, 0], None, VIEW)
    # a name outside the font reaches the buffer as one '?' per character
    assert obev.bev_box_table(b7[:1], sc[:1], [1], None, VIEW, ["-", "Vélo\x7f"])[1] == b"V?lo? 0.99"


def test_giant_box_corners_are_clamped_in_the_table():
    b = np.array([[3.2, 0.0, 0, 1.0, 10000.0, 1, 0.01]], F)
    tab, text = obev.bev_box_table(b, [0.5], [1], None, VIEW, ["-", "Car"])
    assert tab[0, 8] == 1 and tab[0, :8].min() == -32768 and tab[0, :8].max() == 32767 and text == b""


class _Engine:
    """A CPU engine without ``device``: deterministic boxes, all labels."""
    names = ["Car", "Pedestrian", "Cyclist"]
    z_offset, normalize, label_base = 1.5, True, 1


def _clouds(n=3):
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep
    out = []
    for s in range(n):
        pts = lidar_sweep(LidarSpec(rings=8, azimuth_steps=128, sensor_height=1.8), s)
        out.append(compat.create_cloud_xyzi(np.frombuffer(pts.tobytes(), F).reshape(-1, 4), msgs.Header(seq=s + 1)))
    return out


def _preds(n):
    out = []
    for s in range(n):
        k = 5
        box = np.zeros((k, 7), F)
        box[:, 0], box[:, 1] = 4.0 + 2.5 * np.arange(k) + 0.3 * s, -6.0 + 2.0 * np.arange(k)
        box[:, 3:6], box[:, 6] = (3.9, 1.6, 1.5), np.linspace(-1.0, 2.0, k)
        out.append({"pred_boxes": box, "pred_scores": np.linspace(0.2, 0.9, k).astype(F),
                    "pred_labels": (np.arange(k) % 3 + 1).astype(np.int64)})
    return out


BIG = BevView((0.0, 20.0), (-10.0, 10.0), 0.25, (-3.0, 1.0))


def test_cpu_renderer_is_the_host_painter():
    from triton_client_amd.inference.engines import Detector3D

    clouds, preds = _clouds(), _preds(3)
    eng = _Engine()
    assert Detector3D.bev_painter(eng) == "host"
    want = Detector3D.render_bev(eng, clouds, preds, BIG)
    ren = obev.BevRenderer("cpu")
    assert not ren.gpu and ren.ws is None
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the CPU renderer has nothing to warn about
        got = ren.render(clouds, preds, BIG, bev.label_names(eng.names, 1), 1.5)
    assert len(got) == 3
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
        assert (w == bev.HEADING_COLOR).all(2).any() and (w[..., 0] == w[..., 1]).any() and w.any()
    assert Detector3D.bev_renderer(eng) is Detector3D.bev_renderer(eng) and not Detector3D.bev_renderer(eng).gpu


def test_layouts_the_kernel_takes():
    c = _clouds(1)[0]
    assert obev.device_takes(cloud_layout(c))
    assert obev.device_takes(CloudLayout(21, (1, 5, 9, 13), (7, 7, 7, 7)))
    assert not obev.device_takes(CloudLayout(16, (0, 4, 8, -1), (7, 7, 7, 7)))          # no intensity field
    assert not obev.device_takes(CloudLayout(24, (0, 8, 12, 16), (8, 7, 7, 7)))         # FLOAT64 x
    assert not obev.device_takes(CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 2)))          # UINT8 intensity
    assert not obev.device_takes(CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7), True))    # big-endian
    assert not obev.device_takes(CloudLayout(16, (0, 4, 8, 14), (7, 7, 7, 7)))          # past the record
    assert obev.plane_words(VIEW) == 64 * 12 and obev.plane_words(BevView()) == 691 * 199


def test_device_bev_switch(monkeypatch):
    from triton_client_amd.inference.engines import Detector3D

    class Gpu(_Engine):
        device = "cuda"

    class Remote(_Engine):
        device, label_device = None, "cuda:0"

    monkeypatch.delenv("TCA_DEVICE_BEV", raising=False)
    assert obev.device_enabled()
    assert Detector3D.bev_painter(Gpu()) == "device" and Detector3D.bev_painter(Remote()) == "device"
    monkeypatch.setenv("TCA_DEVICE_BEV", "0")
    assert not obev.device_enabled()
    assert Detector3D.bev_painter(Gpu()) == "host" and Detector3D.bev_painter(Remote()) == "host"
    # switched off, a GPU engine paints on the host: no renderer is made, the pictures are the definition's
    eng = Gpu()
    clouds, preds = _clouds(2), _preds(2)
    got = Detector3D.render_bev(eng, clouds, preds, BIG)
    assert getattr(eng, "_bev_renderer", None) is None
    for g, w in zip(got, Detector3D.render_bev(_Engine(), clouds, preds, BIG)):
        np.testing.assert_array_equal(g, w)
    monkeypatch.setenv("TCA_DEVICE_BEV", "1")
    assert Detector3D.bev_painter(Gpu()) == "device"
