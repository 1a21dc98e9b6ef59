"""K38 on the device: ``tca_depth_fill`` gives the bytes of ``image_of_keys(fill_numpy(keys))``."""
import numpy as np
import pytest
import torch

from test_depth_fill import keys, options
from test_range2d import CAL, _rig_messages
from triton_client_amd import _native
from triton_client_amd.ops import depth_image as D
from triton_client_amd.ops import range2d as R

pytestmark = pytest.mark.gpu

SENT, GUARD = 0xA5, 64  # what `out` and its guards hold before a launch; bytes of guard on either side
ENCODINGS = ("16UC1", "32FC1")
SIZES = ((1, 1), (5, 3), (67, 35), (130, 70))  # below any halo; one tile and a ragged edge; tiles both ways
RADII = {"defaults": (2, 3, 15, 2), "maximum": (4, 7, 15, 2), "stages off": (2, 0, 0, 0), "small": (1, 1, 2, 1)}


def run(cuda, planes, o, fused=0, skip_empty=1, **bad):
    """``tca_depth_fill`` on ``planes`` [B, H, W] → (its return code, the images, whether only the images' bytes
    were written)."""
    planes = np.ascontiguousarray(planes, np.uint32)
    B, n = len(planes), planes.size
    dev_keys = torch.from_numpy(planes.view(np.int32)).to(cuda)
    scratch = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=cuda)
    out = torch.full((2 * GUARD + B * o.frame_bytes,), SENT, dtype=torch.uint8, device=cuda)
    p = _native.ptr
    args = dict(keys=p(dev_keys), keys_bytes=4 * n, B=B, W=o.width, H=o.height, enc=D.ENCODINGS[o.encoding], k=o.fill,
                h=o.fill_hole, g=o.fill_large, m=o.fill_median, fused=fused, skip=skip_empty, scratch=p(scratch),
                scratch_bytes=4 * n, out=p(out) + GUARD, out_bytes=B * o.frame_bytes, stream=_native.stream_ptr())
    rc = _native.kernels().tca_depth_fill(*{**args, **bad}.values())
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    clean = (raw[:GUARD] == SENT).all() and (raw[-GUARD:] == SENT).all() and \
        torch.equal(dev_keys.cpu(), torch.from_numpy(planes.view(np.int32)))
    return rc, raw[GUARD:-GUARD].view(o.dtype).reshape(B, o.height, o.width), clean


def check(cuda, planes, o, what):
    want = np.stack([D.image_of_keys(D.fill_numpy(p, o), o) for p in planes])
    for fused, skip in ((0, 1), (1, 1), (0, 0)):  # two launches, one launch, and no early exit of empty tiles
        rc, got, clean = run(cuda, planes, o, fused, skip)
        assert rc == 0 and clean, (what, fused, skip)
        np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg=f"{what} {fused} {skip}")
    return want


@pytest.mark.parametrize("radii", sorted(RADII))
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_byte_for_byte_the_definition(cuda, encoding, size, radii):
    o = options(*size, encoding, RADII[radii])
    plane = keys(np.random.default_rng(size[0]), *size, encoding, density=0.05 if size[0] > 60 else 0.3)
    want = check(cuda, [plane], o, f"{encoding} {size} {radii}")
    if size == (130, 70):  # not vacuous: filled where it was empty, and not everywhere the same
        assert (D.image_of_keys(plane, o).view(np.uint8) != want[0].view(np.uint8)).sum() > 1000


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_three_frames_and_corner_keys(cuda, encoding):
    rng = np.random.default_rng(3)
    W, H = 67, 35
    o = options(W, H, encoding, RADII["defaults"])
    full = keys(rng, W, H, encoding, density=2.0)
    empty = np.full((H, W), D.EMPTY, np.uint32)
    want = check(cuda, [keys(rng, W, H, encoding), empty, full], o, "three frames")  # the frame stride
    assert (want[1].view(np.uint8) == D.image_of_keys(empty, o).view(np.uint8)).all()
    corners = np.full((70, 130), D.EMPTY, np.uint32)
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = keys(rng, 4, 1, encoding, density=2.0)[0]
    check(cuda, [corners], options(130, 70, encoding, RADII["maximum"]), "corners")


def test_refusals_launch_nothing(cuda):
    o = options(67, 35, "16UC1", RADII["defaults"])
    plane = keys(np.random.default_rng(5), 67, 35, "16UC1")
    bad = {"k 0": dict(k=0), "k 5": dict(k=5), "hole 8": dict(h=8), "hole -1": dict(h=-1), "large 16": dict(g=16),
           "median 3": dict(m=3), "encoding 2": dict(enc=2), "0 frames": dict(B=0), "65 frames": dict(B=65),
           "W 0": dict(W=0), "H 4097": dict(H=4097), "null keys": dict(keys=0), "null out": dict(out=0),
           "null scratch": dict(scratch=0), "short keys": dict(keys_bytes=4 * 67 * 35 - 1),
           "short scratch": dict(scratch_bytes=4 * 67 * 35 - 1), "short out": dict(out_bytes=2 * 67 * 35 - 1),
           "fused 2": dict(fused=2), "skip_empty 2": dict(skip=2)}
    for what, kw in bad.items():
        rc, got, clean = run(cuda, [plane], o, **kw)
        assert rc != 0 and clean and (got.view(np.uint8) == SENT).all(), what


def test_the_imager_fills_on_the_device_and_on_the_host(cuda, monkeypatch):
    clouds, _ = _rig_messages()
    o = D.DepthOptions(1242, 375, fill=2)
    want = [D.depth_numpy(R.cloud_xyzi(c), CAL.M, o) for c in clouds]
    plain = D.depth_numpy(R.cloud_xyzi(clouds[0]), CAL.M, D.DepthOptions(1242, 375))
    assert (want[0] != 0).sum() > 2 * (plain != 0).sum()
    for env, device in (("1", True), ("0", False)):
        monkeypatch.setenv("TCA_DEVICE_DEPTH", env)
        im = D.DepthImager(cuda)
        got = im.images(clouds, CAL.M, o)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)) and len(got) == len(want)
        assert im.gpu and (im._stream is not None) == device  # TCA_DEVICE_DEPTH=0: the definition, on the host
