"""K30 on the device: ``tca_ground_split`` gives, bit for bit, the records the definition of ops/ground.py
selects, in input order, and writes nothing else."""
import warnings

import numpy as np
import pytest
import torch

from test_ground import OPTS, gaussian_cloud
from test_laser_scan_gpu import LAYOUTS, _GpuEngine, _swapped, payload
from test_range2d import _rig_messages
from triton_client_amd.ops import ground as G

pytestmark = pytest.mark.gpu

F = np.float32
SENT = 0xA5  # what the output buffer holds before a launch
# one cell; the defaults; 4096 sectors (32 blocks to a workgroup) over a short range; 512 rings of 5 cm
GRIDS = {"one_cell": dict(sectors=1, cell=10.0, range_max=10.0), "default": {},
         "sectors4096": dict(sectors=4096, range_max=20.0), "rings512": dict(cell=0.05, range_max=25.6)}
POINTS = (0, 1, 255, 256, 257, 5000)  # 5000 points are 20 blocks: the scan and the offsets across blocks matter


def cloud_points(seed, n):
    """Gaussian points, sigma 12 m around the sensor and 0.6 m around z = -1.5: every grid sees ground, obstacles
    and points outside it."""
    return (gaussian_cloud(seed, max(n, 1)) * F([0.4, 0.4, 1.0]))[:n]


class Device:
    """One splitter for the module: every test launches on the same workspace."""

    def __init__(self, dev):
        self.splitter = G.GroundSplitter(dev)

    def prepare(self, clouds, opts, layout="record16"):
        lay, mis = LAYOUTS[layout]
        raws = [payload(p, lay) for p in clouds]
        call = self.splitter.prepare(raws, [len(p) for p in clouds], lay, opts, misalign=mis)
        call.out.fill_(SENT)  # the launch owns its regions and counts, nothing else
        return call, raws

    @staticmethod
    def expected(call, raws, classes, want):
        """The whole output buffer as it must be after a launch on the sentinel."""
        step = call.layout.point_step
        buf = np.full(call.out.numel(), SENT, np.uint8)
        counts = buf[call.slab_bytes:call.out_bytes].view("<i4").reshape(call.batch, 2)
        for b, (raw, cls, fo) in enumerate(zip(raws, classes, call.frame_offs)):
            rows = np.frombuffer(raw, np.uint8).reshape(-1, step)
            obs, gnd = rows[cls == 2].reshape(-1), rows[cls == 1].reshape(-1)
            if want & 1:
                buf[fo:fo + len(obs)] = obs
                counts[b, 0] = len(obs) // step
            if want & 2:
                end = fo + len(rows) * step
                buf[end - len(gnd):end] = gnd
                counts[b, 1] = len(gnd) // step
        return buf

    def check(self, clouds, opts, classes, layout="record16", wants=(1, 2, 3), saved=True, what=""):
        call, raws = self.prepare(clouds, opts, layout)
        for want in wants:
            call.out.fill_(SENT)
            G.launch(call, want, saved=saved)
            torch.cuda.synchronize()
            got = call.out.cpu().numpy()
            want_buf = self.expected(call, raws, classes, want)
            # counts, both regions, the gap, the unwanted region and count, and everything past the last slot
            np.testing.assert_array_equal(got, want_buf, err_msg=f"{what} {layout} want {want} saved {saved}")
        return call, raws


@pytest.fixture(scope="module")
def device(cuda):
    return Device(cuda)


@pytest.fixture(scope="module")
def tables():
    """The clouds of every size and the definition's classes per (grid, points): made once."""
    pts = {n: cloud_points(n, n) for n in POINTS}
    opts = {g: G.GroundOptions(**kw) for g, kw in GRIDS.items()}
    assert (opts["one_cell"].nr, opts["sectors4096"].nr, opts["rings512"].nr) == (1, 40, 512)
    want = {(g, n): G.split_numpy(pts[n], o) for g, o in opts.items() for n in POINTS}
    for g in GRIDS:  # every grid decides something: ground and obstacles in every block, and dropped points
        cls = want[(g, 5000)]
        if g == "one_cell":  # the lowest point within 10 m is the ground; nearly everything else stands above it
            assert (cls == 1).sum() >= 5 and (cls == 2).sum() > 1000 and (cls == 0).sum() > 1000
            continue
        assert min((cls == k).sum() for k in (1, 2)) > 400 and ((cls == 0).sum() > 400 or g == "default"), g
        assert all((cls[i:i + 256] == k).any() for i in range(0, 5000, 256) for k in (1, 2)), g
    return pts, opts, want


@pytest.mark.parametrize("n", POINTS)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_bit_for_bit_the_definitions_records(device, tables, layout, n):
    pts, opts, want = tables
    for g, o in opts.items():
        device.check([pts[n]], o, [want[(g, n)]], layout, what=f"{g} {n} points")


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_computing_the_classes_again_gives_the_same_bytes(device, tables, grid):
    pts, opts, want = tables
    device.check([pts[5000]], opts[grid], [want[(grid, 5000)]], "step32", saved=False, what=grid)
    device.check([pts[257]], opts[grid], [want[(grid, 257)]], "step18", saved=False, what=grid)


@pytest.mark.parametrize("layout", ["record16", "record16_mis4", "record16_mis1", "step18"])
def test_ragged_batches_and_a_second_launch(device, layout):
    o = G.GroundOptions(range_max=40.0)
    sizes = (3000, 0, 257)
    clouds = [cloud_points(100 + b, n) for b, n in enumerate(sizes)]
    classes = [G.split_numpy(p, o) for p in clouds]
    assert (classes[0] == 1).sum() > 500 and (classes[0] == 2).sum() > 500
    call, raws = device.check(clouds, o, classes, layout, what=str(sizes))  # no cloud leaks into another's slot
    first = call.out.cpu().numpy()
    call.plane.fill_(0x11)  # garbage in the workspace: a launch owns everything it reads
    call.blocks.fill_(0x22)
    call.cls.fill_(0x33)
    G.launch(call, 3)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(call.out.cpu().numpy(), first)
    np.testing.assert_array_equal(call.counts.cpu().numpy(),
                                  [[(c == 2).sum(), (c == 1).sum()] for c in classes])


def test_a_batch_of_64_tiny_clouds(device):
    o = G.GroundOptions(sectors=90, range_max=30.0)
    clouds = [cloud_points(200 + b, 5 + 9 * b) for b in range(64)]
    device.check(clouds, o, [G.split_numpy(p, o) for p in clouds], "step18", wants=(3,))


def test_every_point_in_one_cell_keeps_its_order(device):
    # 4,096 points along one ray in one cell, alternating ground and obstacle: the ranks alone order them
    z = np.where(np.arange(4096) % 3 == 0, F(-1.8), F(-0.5)) + np.arange(4096, dtype=F) / F(65536)
    pts = np.stack([np.full(4096, F(4.1)), np.full(4096, F(0.3)), z], 1)
    o = G.GroundOptions()
    cls = G.split_numpy(pts, o)
    assert (cls == 1).sum() == 1366 and (cls == 2).sum() == 2730
    device.check([pts], o, [cls])


def test_a_record_past_data_bytes_is_not_read(device):
    o = G.GroundOptions()
    pts = cloud_points(60, 700)
    pts[-1] = (5.0, 0.1, -1.8)  # the last point is ground
    cls_all, cls_short = G.split_numpy(pts, o), G.split_numpy(pts[:-1], o)
    assert cls_all[-1] == 1 and (cls_all[:-1] == cls_short).all()
    call, raws = device.prepare([pts], o)
    rows = np.frombuffer(raws[0], np.uint8).reshape(-1, 16)[:-1]
    obs, gnd = rows[cls_short == 2].reshape(-1), rows[cls_short == 1].reshape(-1)
    end = 16 * 700  # (the staged bytes end 16-byte aligned: 700 * 16)
    assert call.data_bytes == end
    for nbytes in (end - 16, end - 1):  # one record short; a record that only ends past it
        call.data_bytes = nbytes
        call.out.fill_(SENT)
        G.launch(call, 3)
        torch.cuda.synchronize()
        got = call.out.cpu().numpy()
        assert call.counts.cpu().numpy().tolist() == [[len(obs) // 16, len(gnd) // 16]]  # without the last point
        np.testing.assert_array_equal(got[:len(obs)], obs)
        np.testing.assert_array_equal(got[end - len(gnd):end], gnd)  # the ground region ends the slot of 700 records
        assert (got[len(obs):end - len(gnd)] == SENT).all()


def test_launcher_refusals(device):
    from triton_client_amd import _native

    o = G.GroundOptions()
    clouds = [cloud_points(50, 300), cloud_points(51, 200)]
    call, raws = device.prepare(clouds, o)
    call.plane.fill_(0x5A)
    plane_before = call.plane.clone()
    fn = _native.kernels().tca_ground_split
    p = _native.ptr
    nan, inf = float("nan"), float("inf")
    base = dict(data=p(call.data), data_bytes=call.data_bytes, frame_off=p(call.frame_off), frame_n=p(call.frame_n),
                batch=2, max_n=300, step=16, ox=0, oy=4, oz=8, table=p(call.table), S=360, nr=160, cell=0.5, r0=0.0,
                h0=o.h0, slope_q=o.slope_q, noise_q=o.noise_q, thick_q=o.thick_q, top_q=o.top_q, want=3, saved=1,
                plane=p(call.plane), blocks=p(call.blocks), cls=p(call.cls), out=p(call.out), out_bytes=call.slab_bytes,
                counts=p(call.counts),
                stream=_native.stream_ptr())

    def rc(**kw):
        return fn(*{**base, **kw}.values())

    bad = {"null data": dict(data=0), "null frame_off": dict(frame_off=0), "null frame_n": dict(frame_n=0),
           "null table": dict(table=0), "null plane": dict(plane=0), "null blocks": dict(blocks=0),
           "null cls": dict(cls=0), "null out": dict(out=0), "null counts": dict(counts=0),
           "out is data": dict(out=p(call.data)), "0 frames": dict(batch=0), "65 frames": dict(batch=65),
           "negative batch": dict(batch=-1), "negative data_bytes": dict(data_bytes=-1),
           "2^31 payload bytes": dict(data_bytes=2 ** 31), "negative out_bytes": dict(out_bytes=-1),
           "2^31 output bytes": dict(out_bytes=2 ** 31), "negative max_n": dict(max_n=-1), "step 0": dict(step=0),
           "0 sectors": dict(S=0), "4097 sectors": dict(S=4097), "0 rings": dict(nr=0), "513 rings": dict(nr=513),
           "more than 2^24 cells": dict(S=4096, nr=512, batch=9), "cell 0": dict(cell=0.0), "cell nan": dict(cell=nan),
           "cell inf": dict(cell=inf), "range_min negative": dict(r0=-1.0), "range_min nan": dict(r0=nan),
           "range_min inf": dict(r0=inf), "h0 too low": dict(h0=-2 ** 21 - 1), "h0 too high": dict(h0=2 ** 21 + 1),
           "slope_q negative": dict(slope_q=-1), "noise_q negative": dict(noise_q=-1),
           "thick_q negative": dict(thick_q=-1), "top_q too high": dict(top_q=2 ** 21 + 1), "want 0": dict(want=0),
           "want 4": dict(want=4), "saved 2": dict(saved=2), "a field outside the record": dict(oz=16),
           "a negative offset": dict(ox=-4), "misaligned plane": dict(plane=p(call.plane) + 2),
           "misaligned blocks": dict(blocks=p(call.blocks) + 2), "misaligned counts": dict(counts=p(call.counts) + 2),
           "misaligned table": dict(table=p(call.table) + 1), "misaligned frame_off": dict(frame_off=p(call.frame_off) + 4),
           "misaligned frame_n": dict(frame_n=p(call.frame_n) + 2)}
    for what, kw in bad.items():
        assert rc(**kw) == 1, what  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (call.out == SENT).all() and torch.equal(call.plane, plane_before)  # nothing was launched
    assert rc() == 0
    torch.cuda.synchronize()
    classes = [G.split_numpy(c, o) for c in clouds]
    np.testing.assert_array_equal(call.out.cpu().numpy(), Device.expected(call, raws, classes, 3))


# ------------------------------------------------------------------------ through the splitter
def test_splitter_equals_the_host_path_with_either_copy_back(cuda):
    clouds, _ = _rig_messages()
    want = [G.split_cloud_numpy(c, OPTS) for c in clouds]
    assert all(obs.width > 50 and gnd.width > 10 for obs, gnd in want)
    sp = G.GroundSplitter(cuda)
    assert sp.copy_back == "auto" and sp.split(clouds, OPTS) == want and sp._stream is not None  # the kernel ran
    assert sp.split(clouds, OPTS, 1) == [(o, None) for o, _ in want]
    assert sp.split(clouds, OPTS, 2) == [(None, g) for _, g in want]
    sp.copy_back = "counted"
    for w in (1, 2, 3):
        assert sp.split(clouds, OPTS, w) == [(o if w & 1 else None, g if w & 2 else None) for o, g in want]
    sp.saved = False
    assert sp.split(clouds, OPTS) == want
    assert sp.split([], OPTS) == []


def test_a_big_endian_cloud_goes_to_the_host_with_one_warning(cuda):
    clouds, _ = _rig_messages()
    c = clouds[0]
    sp = G.GroundSplitter(cuda)
    want, swapped = G.split_cloud_numpy(c, OPTS), G.split_cloud_numpy(_swapped(c), OPTS)
    assert swapped[0].width == want[0].width and swapped[0].is_bigendian and swapped[0].data != want[0].data
    with pytest.warns(RuntimeWarning, match="little-endian FLOAT32") as rec:
        got = sp.split([c, _swapped(c), clouds[1]], OPTS)
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert got == [want, swapped, G.split_cloud_numpy(clouds[1], OPTS)]
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # one warning in the object's life
        assert sp.split([_swapped(c)], OPTS) == [swapped]


def test_engine_and_driver_publish_the_definitions_bytes(cuda, monkeypatch):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.inference.engines import Detector3D

    clouds, _ = _rig_messages()
    want = [G.split_cloud_numpy(c, OPTS) for c in clouds]
    eng = _GpuEngine()
    assert Detector3D.split_ground(eng, clouds, OPTS) == want
    sp = Detector3D.ground_splitter(eng)
    assert sp is eng._ground_splitter and sp.gpu and sp._stream is not None  # made once; the kernel ran
    drv = RosInference3D(engine=_GpuEngine(), params={}, obstacles_topic="/obs", ground_options=OPTS)
    res = drv.process(clouds)
    assert [(r.obstacles, r.ground) for r in res] == [(o, None) for o, _ in want]
    assert drv.engine._ground_splitter._stream is not None
    monkeypatch.setenv("TCA_DEVICE_GROUND", "0")
    other = _GpuEngine()
    assert Detector3D.split_ground(other, clouds, OPTS, 2) == [(None, g) for _, g in want]
    assert other._ground_splitter.gpu and other._ground_splitter._stream is None  # the definition, on a GPU engine too
