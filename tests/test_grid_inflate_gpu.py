"""K37 on the device: ``tca_grid_inflate`` is byte for byte ``inflate_numpy``, on planes uploaded as they are."""
import dataclasses

import numpy as np
import pytest
import torch

from test_grid_inflate import opts_of, random_plane
from test_ground import OPTS as GROUND
from test_occupancy_grid import RIG
from test_range2d import _rig_messages
from triton_client_amd import _native
from triton_client_amd.ops import occupancy_grid as O

pytestmark = pytest.mark.gpu

SENT = 0x5A  # what the output buffer holds before a launch
TILE = (64, 32)  # a workgroup's cells: 130 x 70 has three tiles in each axis, 67 x 35 two


def planes_for(W, H):
    # no obstacle, only obstacles, one on every corner and edge, one on the first cell of the second tile, two random
    empty = np.where(np.arange(W * H) % 3 == 0, -1, 0).astype(np.int8)
    edges = np.where(np.arange(W * H) % 5 == 0, -1, 0).astype(np.int8).reshape(H, W)
    edges[np.ix_([0, H // 2, H - 1], [0, W // 2, W - 1])] = 100
    edges[H // 2, W // 2] = 0
    corner = np.where(np.arange(W * H) % 2 == 0, -1, 0).astype(np.int8).reshape(H, W)
    corner[min(TILE[1], H - 1), min(TILE[0], W - 1)] = 100
    return [empty, np.full(W * H, 100, np.int8), edges.reshape(-1), corner.reshape(-1), random_plane(W, H, 1),
            random_plane(W, H, 2)]


def run(dev, planes, o, skip_empty=True):
    # planes laid out as tca_occupancy_grid leaves them → the output's planes; the padding keeps the sentinel
    B, cells = len(planes), o.W * o.H
    host = np.full(B * o.stride + 64, 0x33, np.uint8)
    for b, p in enumerate(planes):
        host[b * o.stride:b * o.stride + cells] = p.view(np.uint8)
    lut = O.cost_table(o).view(np.uint8)
    c = O.GridCall(ground=None, table=None, cells=None, keys=None, out=torch.from_numpy(host).to(dev), batch=B, opts=o,
                   inflated=torch.full((len(host),), SENT, dtype=torch.uint8, device=dev),
                   lut=torch.from_numpy(lut.copy()).to(dev))
    O.inflate(c, skip_empty=skip_empty)
    torch.cuda.synchronize()
    raw = c.inflated.cpu().numpy()
    assert (raw[c.out_bytes:] == SENT).all(), "written past the last plane"
    for b in range(B):
        assert (raw[b * o.stride + cells:min((b + 1) * o.stride, c.out_bytes)] == SENT).all(), "padding written"
    return O.planes_of(raw, B, o)


@pytest.mark.parametrize("unknown", [False, True])
@pytest.mark.parametrize("Rc", [1, 7, 64])  # 64: the halo is wider than a tile and reaches two tiles up and down
@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (67, 35), (130, 70)])
def test_byte_for_byte_the_definition(cuda, shape, Rc, unknown):
    o = opts_of(*shape, Rc, inflate_unknown=unknown)
    planes = planes_for(*shape)
    want = [O.inflate_numpy(p, o) for p in planes]
    for skip in (True, False):
        got = run(cuda, planes, o, skip)
        for b in range(len(planes)):
            np.testing.assert_array_equal(got[b], want[b], err_msg=f"plane {b}, skip_empty {skip}")


def test_the_rim_across_a_tile_corner(cuda):
    # 3, 4, 5: the first cell of tile (1, 1) is exactly Rc from cells of tile (0, 0), along the axes and on a diagonal
    o = opts_of(130, 70, 5)
    p = np.zeros((70, 130), np.int8)
    p[32, 64] = 100
    want = O.inflate_numpy(p.reshape(-1), o).reshape(70, 130)
    rim = int(O.cost_table(o)[25])
    assert 0 < rim < 99 and want[28, 61] == want[29, 60] == want[32, 59] == want[27, 64] == rim
    assert want[28, 60] == want[32, 58] == want[26, 64] == want[27, 63] == 0
    for skip in (True, False):
        np.testing.assert_array_equal(run(cuda, [p.reshape(-1)], o, skip)[0], want.reshape(-1))


def test_the_mapper_gives_the_inflated_definition(cuda):
    clouds = _rig_messages()[0][:2]
    o = dataclasses.replace(RIG, inflation_radius=1.2, inscribed_radius=0.5, cost_scaling=2.0)
    got = O.GridMapper(cuda).grids(clouds, o, GROUND)
    for g, c in zip(got, clouds):
        want = O.grid_cloud_numpy(c, o, GROUND)
        assert ((want > 0) & (want < 99)).sum() > 20
        np.testing.assert_array_equal(g, want)


REFUSED = {"radius 0": lambda a: dict(R=0), "radius 65": lambda a: dict(R=65), "a short table": lambda a: dict(lut_bytes=49),
           "short planes": lambda a: dict(in_bytes=a["in_bytes"] - 1), "short out": lambda a: dict(out_bytes=a["out_bytes"] - 1),
           "a second plane in the same buffers": lambda a: dict(batch=2), "65 planes": lambda a: dict(batch=65),
           "W 0": lambda a: dict(W=0), "H 2049": lambda a: dict(H=2049), "null planes": lambda a: dict(planes=0),
           "null table": lambda a: dict(lut=0), "misaligned planes": lambda a: dict(planes=a["planes"] + 4),
           "misaligned out": lambda a: dict(out=a["out"] + 4), "out is planes": lambda a: dict(out=a["planes"]),
           "inflate_unknown 2": lambda a: dict(unknown=2), "skip_empty -1": lambda a: dict(skip=-1)}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_launcher_refusals(cuda, what):
    o = opts_of(67, 35, 7)
    src = torch.zeros(o.W * o.H + 16, dtype=torch.uint8, device=cuda)
    dst = torch.full((o.W * o.H + 16,), SENT, dtype=torch.uint8, device=cuda)
    lut = torch.from_numpy(O.cost_table(o).view(np.uint8).copy()).to(cuda)
    p = _native.ptr
    a = dict(planes=p(src), in_bytes=o.W * o.H, batch=1, W=67, H=35, R=7, lut=p(lut), lut_bytes=50, unknown=0, skip=1,
             out=p(dst), out_bytes=o.W * o.H, stream=_native.stream_ptr())
    fn = _native.kernels().tca_grid_inflate
    assert fn(*{**a, **REFUSED[what](a)}.values()) == 1, what  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (dst == SENT).all()  # nothing was launched
