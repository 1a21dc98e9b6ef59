"""K33 on the device: ``tca_occupancy_grid`` behind ``tca_ground_split`` is bit for bit ``grid_cloud_numpy``."""
import dataclasses

import numpy as np
import pytest
import torch

from test_ground import OPTS as GROUND
from test_laser_scan_gpu import LAYOUTS, _GpuEngine, payload
from test_occupancy_grid import OPTS, RIG, F, _wanted, scene
from test_range2d import _rig_messages
from triton_client_amd.ops import ground as G
from triton_client_amd.ops import occupancy_grid as O
from triton_client_amd.ops.laser_scan import pseudo_bins
from triton_client_amd.ros import compat, msgs

pytestmark = pytest.mark.gpu

SENT = 0x5A  # what the output buffer holds before a launch
POINTS = (0, 1, 255, 256, 257, 5000)
SHAPES = {"1x1": dict(cell=10.0, x_range=(-5, 5), y_range=(-5, 5)),
          "5x3": dict(cell=3.0, x_range=(-7.5, 7.5), y_range=(-4.5, 4.5), min_points=150),  # (some cells stay below it)
          "64x48": dict(cell=0.25, x_range=(-8, 8), y_range=(-6, 6))}
VARIANTS = {"no_lds_keys": dict(privatise=False), "atomic_per_point": dict(aggregate=False),
            "keys_staged_in_lds": dict(stage_keys=True), "none_of_them": dict(privatise=False, aggregate=False)}


def cloud(seed, n):
    """The CPU file's scene, twice as dense, cut to ``n`` points of its seeded order."""
    return np.concatenate([scene(seed), scene(seed + 100)])[:n]


def want_of(pts, opts):
    return O.grid_numpy(*O.split_rows(pts), opts)


class Device:
    """One mapper for the module: every test launches on the same workspace."""

    def __init__(self, dev):
        self.mapper = O.GridMapper(dev)

    def run(self, clouds, opts, layout="record16", **variant):
        lay, mis = LAYOUTS[layout]
        call = self.mapper.prepare([payload(p, lay) for p in clouds], [len(p) for p in clouds], lay, opts, misalign=mis)
        call.out.fill_(SENT)  # the launch owns its planes' cells, nothing between or past them
        call.cells.fill_(0x33)  # garbage in the workspace: the reset belongs to the launch
        call.keys.fill_(0x33)
        O.launch(call, **variant)
        torch.cuda.synchronize()
        raw = call.out.cpu().numpy()
        cells = opts.W * opts.H
        assert (raw[call.out_bytes:] == SENT).all(), "written past the last plane"
        for b in range(call.batch):
            assert (raw[b * opts.stride + cells:min((b + 1) * opts.stride, call.out_bytes)] == SENT).all(), "padding written"
        return O.planes_of(raw, call.batch, opts), call


@pytest.fixture(scope="module")
def device(cuda):
    return Device(cuda)


def same(got, want, what=""):
    assert len(got) == len(want) and all(g.dtype == np.int8 for g in got), what
    for b, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg=f"{what} cloud {b}")


def test_the_data_makes_workgroups_meet():
    # 90 sectors: a workgroup walks 4 blocks of 256 records of the slab (obstacles, then ground): 5000 are 20 blocks,
    # five workgroups (workgroup w walks blocks w, w + 5, ...) that flush into the same sector bins and cells
    obs, gnd = O.split_rows(cloud(5000, 5000))
    slab = np.concatenate([obs, gnd])
    assert len(slab) == 5000 and len(obs) > 1500 and len(gnd) > 1000
    sec, has = pseudo_bins(slab[:, 0].copy(), slab[:, 1].copy(), G.edge_table(OPTS))
    cell, _ = O.C.cells_numpy(slab, OPTS)
    group = np.arange(5000) // 256 % 5
    assert len(set.intersection(*[set(sec[has & (group == w)]) for w in range(5)])) > 60
    assert len(set.intersection(*[set(cell[(cell >= 0) & (group == w)]) for w in range(5)])) > 50


@pytest.mark.parametrize("n", POINTS)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_bit_for_bit_the_definition(device, layout, n):
    pts = cloud(n, n)
    same(device.run([pts], OPTS, layout)[0], [want_of(pts, OPTS)], f"{layout} {n} points")


@pytest.mark.parametrize("sectors", [1, 90, 4096])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_grid_shapes_and_sectors(device, shape, sectors):
    o = O.GridOptions(sectors=sectors, clear_radius=0.4, **SHAPES[shape])
    assert f"{o.W}x{o.H}" == shape
    clouds = [cloud(7, 5000), cloud(8, 700)]  # (5 x 3: 15 cells, a bytewise tail, the second plane 16 bytes on)
    same(device.run(clouds, o, "step32")[0], [want_of(p, o) for p in clouds], f"{shape} {sectors} sectors")


def test_a_ragged_batch_and_a_relaunch_with_another(device):
    ground_only = cloud(11, 1500)
    ground_only = ground_only[ground_only[:, 2] < -1.7]
    first = [cloud(10, 3000), np.zeros((0, 3), F), ground_only]
    want = [want_of(p, OPTS) for p in first]
    assert len(O.split_rows(ground_only)[0]) == 0 and (want[1] == O.UNKNOWN).all() and (want[2] == O.OCCUPIED).sum() == 0
    same(device.run(first, OPTS, "record16_mis4")[0], want, "first batch")
    second = [cloud(12, 257), cloud(13, 4000)]  # the same workspace, filled by the first batch (and then with garbage)
    same(device.run(second, OPTS, "record16_mis4")[0], [want_of(p, OPTS) for p in second], "second batch")


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_the_variants_give_the_same_bytes(device, variant):
    clouds = [cloud(20, 5000), cloud(21, 300)]
    for sectors in (90, 4096):
        o = dataclasses.replace(OPTS, sectors=sectors, min_points=2)
        same(device.run(clouds, o, **VARIANTS[variant])[0], [want_of(p, o) for p in clouds], f"{variant} {sectors}")


def test_the_device_agrees_with_the_float64_reference(device):
    pts = cloud(40, 5000)
    ref, band = O.grid_ref(*O.split_rows(pts), OPTS)
    (got,), _ = device.run([pts], OPTS)
    assert band.mean() <= 0.01
    np.testing.assert_array_equal(got[~band], ref[~band])


def test_launcher_refusals(device):
    from triton_client_amd import _native

    pts = cloud(50, 300)
    (want,), c = device.run([pts], OPTS)
    c.out.fill_(SENT)
    p, g, o = _native.ptr, c.ground, c.ground.layout.offsets
    base = dict(data=p(g.out), data_bytes=g.slab_bytes, frame_off=p(g.frame_off), frame_n=p(g.frame_n), counts=p(g.counts),
                batch=1, max_n=300, step=16, ox=o[0], oy=o[1], oz=o[2], table=p(c.table), S=90, x0=-8.0, y0=-6.0, cell=0.25,
                W=64, H=48, min_points=1, clear=0.0, privatise=1, aggregate=1, stage=0, cells=p(c.cells),
                cells_bytes=c.cells_bytes, keys=p(c.keys), keys_bytes=c.keys_bytes, out=p(c.out), out_bytes=c.out_bytes,
                stream=_native.stream_ptr())
    fn = _native.kernels().tca_occupancy_grid
    bad = {"short cells": dict(cells_bytes=c.cells_bytes - 1), "short keys": dict(keys_bytes=c.keys_bytes - 1),
           "short out": dict(out_bytes=c.out_bytes - 1), "a second cloud in the same buffers": dict(batch=2),
           "65 clouds": dict(batch=65), "4097 sectors": dict(S=4097), "H 2049": dict(H=2049), "cell nan": dict(cell=float("nan")),
           "clear negative": dict(clear=-1.0), "min_points 0": dict(min_points=0), "null counts": dict(counts=0),
           "misaligned out": dict(out=p(c.out) + 4), "misaligned cells": dict(cells=p(c.cells) + 4),
           "a field outside the record": dict(oz=16), "2^31 bytes": dict(data_bytes=2 ** 31), "stage 2": dict(stage=2)}
    for what, kw in bad.items():
        assert fn(*{**base, **kw}.values()) == 1, what  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (c.out == SENT).all()  # nothing was launched
    assert fn(*base.values()) == 0
    torch.cuda.synchronize()
    same(O.planes_of(c.out.cpu().numpy(), 1, OPTS), [want])


# ------------------------------------------------------------------------ through the engine
def test_mapper_engine_and_driver_give_the_definitions_messages(cuda, monkeypatch):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.inference.engines import Detector3D
    from triton_client_amd.ros.bus import TopicBus

    clouds, _ = _rig_messages()
    want = _wanted(clouds)
    same(O.GridMapper(cuda).grids(clouds, RIG, GROUND), [w.data for w in want])

    def drive(env):
        monkeypatch.setenv("TCA_DEVICE_GRID", env)
        eng = _GpuEngine()
        assert Detector3D.occupancy_grids(eng, clouds, RIG, GROUND, "map") == want
        assert Detector3D.grid_mapper(eng) is eng._grid_mapper and eng._grid_mapper.gpu  # made once
        bus, got = TopicBus(), []
        compat.Subscriber("/grid", msgs.OccupancyGrid, got.append, bus=bus)
        drv = RosInference3D(engine=eng, params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=4, workers=2,
                             queue_size=64, grid_topic="/grid", grid_options=RIG, grid_frame_id="map", ground_options=GROUND)
        drv.start_inference(spin=False)
        pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
        for c in clouds:
            pub.publish(c)
        runner = drv.runner
        drv.stop()
        bus.close()
        assert not runner.errors, runner.errors
        assert got == want
        return eng._grid_mapper

    assert drive("1")._stream is not None  # the kernel ran
    assert drive("0")._stream is None  # TCA_DEVICE_GRID=0: the definition, on a GPU engine too
