"""The host side the cloud-reading ops share (ops/cloud_common.py): the byte layout of a staged
batch against offsets derived by hand, the fill, the layout predicate and the per-cloud loop."""
import warnings

import numpy as np
import pytest

from triton_client_amd.ops import bev as obev
from triton_client_amd.ops import cloud_common as cc
from triton_client_amd.ops import points_in_boxes as pib
from triton_client_amd.ops import range2d as R
from triton_client_amd.ops.cloud_common import CloudLayout
from triton_client_amd.ros import compat

# The batch of every test here and in test_cloud_common_gpu.py: 20-byte records, 3 / 0 / 5 points,
# 3 boxes split 2 / 0 / 1.  The rule, by hand: fo = off + misalign; off = align16(fo + n * 20);
# then each section at off, off = align16(off + max(nbytes, 4)).
STEP, NS, NB = 20, [3, 0, 5], [2, 0, 1]
LAY = CloudLayout(STEP, (0, 4, 8, 12), (7, 7, 7, 7))
FRAMES = {0: ((0, 64, 64), 176), 1: ((1, 65, 81), 192)}  # misalign: (frame offsets, data_bytes)
TEXTS = [b"Car 0.99Van 0.5", b"", b"Pe"]  # 17 bytes


def payloads():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, n * STEP, dtype=np.uint8).tobytes() for n in NS]


def op_arrays(nb=NB):
    """Each op's sections for boxes split ``nb``, from the subclass."""
    rng = np.random.default_rng(6)
    tabs = [rng.standard_normal((k, 8)).astype(np.float32) for k in nb]
    scores = [rng.random(k).astype(np.float32) for k in nb]
    labels = [rng.integers(0, 9, k) for k in nb]
    btabs = [rng.integers(0, 99, (k, obev.ROW)).astype(np.int32) for k in nb]
    rows = [rng.random((k, 4)).astype(np.float32) for k in nb]
    return {"K22": (pib.PointLabeler.sections(NS, tabs, scores, labels), (tabs, scores, labels)),
            "K23": (obev.BevRenderer.sections(*obev._concat_tables(btabs, TEXTS)), (btabs, TEXTS)),
            "K26": (R.CameraRanger.sections(rows), (rows,))}


def staged_bytes(arrays, misalign, fill=0xAA):
    """The batch as the CPU fill writes it into a buffer of ``fill`` bytes → (bytes, plan)."""
    plan = cc.plan_staging(NS, STEP, misalign, cc.batch_sections(NS, arrays))
    host = np.full(plan.total, fill, np.uint8)
    cc.fill_staging(host, plan, payloads(), NS, STEP, arrays)
    return host, plan


@pytest.mark.parametrize("misalign", [0, 1])
def test_frame_offsets_by_hand(misalign):
    plan = cc.plan_staging(NS, STEP, misalign, [])
    assert (plan.frame_offs, plan.data_bytes) == FRAMES[misalign]
    assert plan.total == plan.data_bytes and plan.sections == {}


def test_sections_of_each_op_by_hand():
    want = {"K22": ({"frame_off": 176, "frame_n": 208, "box_off": 224, "pt_off": 240, "table": 256, "score": 352,
                     "label": 368}, 384),
            "K23": ({"frame_off": 176, "frame_n": 208, "box_off": 224, "table": 240, "text": 384}, 416),
            "K26": ({"frame_off": 176, "frame_n": 208, "table": 224}, 272)}
    for op, (arrays, _) in op_arrays().items():
        plan = cc.plan_staging(NS, STEP, 0, cc.batch_sections(NS, arrays))
        assert (plan.sections, plan.total) == want[op], op
        assert list(plan.sections) == list(want[op][0]), op  # the order too
    assert pib.out_sections(8, 3) == (0, 32, 48)
    # an empty section still advances by 16
    arrays = op_arrays([0, 0, 0])["K26"][0]
    plan = cc.plan_staging(NS, STEP, 0, cc.batch_sections(NS, arrays))
    assert arrays[0][1].nbytes == 0 and plan.sections["table"] == 224 and plan.total == 240


@pytest.mark.parametrize("misalign", [0, 1])
def test_fill_writes_the_batch_and_nothing_else(misalign):
    for op, (arrays, _) in op_arrays().items():
        host, plan = staged_bytes(arrays, misalign)
        touched = np.zeros(plan.total, bool)

        def check(at, want):
            want = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
            np.testing.assert_array_equal(host[at:at + len(want)], want, err_msg=op)
            touched[at:at + len(want)] = True

        for pl, fo in zip(payloads(), plan.frame_offs):
            check(fo, np.frombuffer(pl, np.uint8))
        check(plan.sections["frame_off"], np.array(FRAMES[misalign][0], np.int64))
        check(plan.sections["frame_n"], np.array(NS, np.int32))
        for name, a in arrays:
            check(plan.sections[name], a)
        assert (host[~touched] == 0xAA).all(), op
    arrays = dict(op_arrays()["K22"][0])
    assert arrays["box_off"].tolist() == [0, 2, 2, 3] and arrays["pt_off"].tolist() == [0, 3, 3, 8]
    assert [arrays[k].dtype for k in ("box_off", "pt_off", "table", "score", "label")] == \
        [np.int32, np.int32, np.float32, np.float32, np.int32]


def test_one_predicate_three_rules():
    xyzi = compat.create_cloud_xyzi(np.zeros((3, 4), np.float32))
    cases = [  # layout, device_ok (K22), device_takes (K23), layout_device_ok (K26)
        (cc.cloud_layout(xyzi), True, True, True),
        (CloudLayout(21, (1, 5, 9, 13), (7, 7, 7, 7)), True, True, True),
        (CloudLayout(16, (0, 4, 8, -1), (7, 7, 7, 7)), True, False, True),          # no intensity field
        (CloudLayout(24, (0, 8, 12, 16), (8, 7, 7, 7)), False, False, False),       # FLOAT64 x
        (CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 2)), False, False, True),         # UINT8 intensity
        (CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7), True), False, False, False),  # big-endian
        (CloudLayout(16, (0, 4, 8, 14), (7, 7, 7, 7)), False, False, True),         # intensity past the record
        (CloudLayout(0, (0, 4, 8, 12), (7, 7, 7, 7)), False, False, False),         # no record
    ]
    for lay, k22, k23, k26 in cases:
        assert (lay.device_ok, obev.device_takes(lay), R.layout_device_ok(lay)) == (k22, k23, k26), lay
    assert cc.fields_f32(cases[4][0], (0, 1, 2)) and not cc.fields_f32(cases[4][0], (3,))
    assert pib.CloudLayout is CloudLayout and pib.cloud_layout is cc.cloud_layout and R.cloud_xyzi is cc.cloud_xyzi


def _clouds():
    f32 = compat.create_cloud_xyzi(np.zeros((2, 4), np.float32))
    big = compat.create_cloud_xyzi(np.zeros((2, 4), np.float32))
    big.is_bigendian = True
    return [f32, big, f32, big, f32]


def test_per_cloud_keeps_the_order_and_warns_once(monkeypatch):
    st = cc.CloudStager("cpu")
    assert not st.gpu and st.ws is None
    st.gpu = True  # the callables below are stubs: nothing touches a device
    clouds, calls = _clouds(), []

    def on_device(lay, part, tag):
        assert st._lock.locked() and lay.device_ok
        calls.append(list(part))
        return [(tag, i) for i in part]

    def run():
        return st._per_cloud(clouds, lambda i, lay: lay.device_ok, lambda i, lay: ("host", i),
                             lambda lay, part: (lay, part, "dev"), on_device, lambda i, lay: f"cloud {i}: {lay}")

    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert run() == [("dev", 0), ("host", 1), ("dev", 2), ("host", 3), ("dev", 4)]
        assert run()[1] == ("host", 1)
    assert calls == [[0, 2, 4], [0, 2, 4]] and not st._lock.locked()
    assert len(seen) == 1 and seen[0].category is RuntimeWarning and str(seen[0].message).startswith("cloud 1: ")
    # a subclass may cut a group into several launches
    monkeypatch.setattr(st, "_parts", lambda idx, clouds: [idx[:2], idx[2:]])
    del calls[:]
    assert [r[0] for r in run()] == ["dev", "host", "dev", "host", "dev"] and calls == [[0, 2], [4]]
    # device=False: everything on the host, without a warning
    st._warned = False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = st._per_cloud(clouds, lambda i, lay: True, lambda i, lay: ("host", i, lay.bigendian), None, None, None,
                            device=False)
    assert got == [("host", i, i % 2 == 1) for i in range(5)]


def test_no_layout_without_a_device_for_the_bev_variant(monkeypatch):
    def no_layout(msg):
        raise AssertionError("a layout was computed")

    monkeypatch.setattr(cc, "cloud_layout", no_layout)
    st = cc.CloudStager("cpu")
    got = st._per_cloud(_clouds(), None, lambda i, lay: (i, lay), None, None, None, host_layouts=False)
    assert got == [(i, None) for i in range(5)]
    with pytest.raises(AssertionError, match="a layout was computed"):
        st._per_cloud(_clouds(), None, lambda i, lay: (i, lay), None, None, None)
