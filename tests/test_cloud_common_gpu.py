"""What the three cloud-reading ops upload is, byte for byte, what ops/cloud_common.py's CPU fill
writes; and staging a smaller batch afterwards moves no buffer."""
import numpy as np
import pytest
import torch

from test_cloud_common import FRAMES, LAY, NS, STEP, op_arrays, payloads, staged_bytes
from triton_client_amd.ops import bev as obev
from triton_client_amd.ops import points_in_boxes as pib
from triton_client_amd.ops import range2d as R
from triton_client_amd.utils.bev import BevView

pytestmark = pytest.mark.gpu

VIEW = BevView((0.0, 6.4), (-2.4, 2.4), 0.1, (-2.0, 2.0))  # 64 rows x 48 columns
FILL = 0xAA
OPS = {"K22": (pib.PointLabeler, ()), "K23": (obev.BevRenderer, (VIEW,)), "K26": (R.CameraRanger, (np.eye(3, 4),))}


def _prepare(obj, op, args, frames, misalign):
    """``prepare()`` of the first ``frames`` frames of the batch."""
    ns = NS[:frames]
    pls = [p[:n * STEP] for p, n in zip(payloads(), ns)]
    return obj.prepare(pls, ns, LAY, *(a[:frames] for a in args), *OPS[op][1], misalign=misalign)


@pytest.mark.parametrize("misalign", [0, 1])
@pytest.mark.parametrize("op", list(OPS))
def test_prepare_uploads_the_cpu_fill(op, misalign):
    arrays, args = op_arrays()[op]
    want, plan = staged_bytes(arrays, misalign, FILL)
    obj = OPS[op][0](torch.device("cuda"))
    obj._pinned("_pin_in", plan.total).fill_(FILL)  # so the bytes the fill does not write are known
    call = _prepare(obj, op, args, 3, misalign)
    torch.cuda.synchronize()
    got = call.data[:plan.total].cpu().numpy()
    np.testing.assert_array_equal(got, want)
    for pl, n, fo in zip(payloads(), NS, FRAMES[misalign][0]):  # the payloads, against the inputs
        assert got[fo:fo + n * STEP].tobytes() == pl
    assert tuple(call.frame_off.cpu().tolist()) == FRAMES[misalign][0]
    if op != "K22":
        assert call.data_bytes == FRAMES[misalign][1]
    if op == "K23":
        assert call.frame_offs == FRAMES[misalign][0] and call.text_bytes == 17
    assert (call.n_boxes, call.batch, call.max_n) == (3, 3, 5)
    assert call.table.data_ptr() == call.data.data_ptr() + plan.sections["table"]

    # a smaller batch afterwards: no regrowth, the same addresses (what a captured graph replays on)
    bufs = {k: v.data_ptr() for k, v in obj.ws._bufs.items()}
    pin = obj._pin_in.data_ptr()
    small = _prepare(obj, op, args, 1, misalign)
    torch.cuda.synchronize()
    assert (small.batch, small.n_boxes, small.max_n) == (1, 2, 3)
    assert small.data.data_ptr() == call.data.data_ptr() and obj._pin_in.data_ptr() == pin
    assert {k: v.data_ptr() for k, v in obj.ws._bufs.items()} == bufs
