"""K34 on the device: ``tca_voxel_downsample`` is bit for bit ``downsample_numpy``."""
import numpy as np
import pytest
import torch

from test_laser_scan_gpu import LAYOUTS, _GpuEngine, payload
from test_occupancy_grid import scene
from test_range2d import _rig_messages
from test_voxel_downsample import RIG, _wanted
from triton_client_amd.ops import voxel_downsample as V
from triton_client_amd.ros import compat, msgs

pytestmark = pytest.mark.gpu

F = np.float32
SENT = 0x5A  # what the output and the whole workspace hold before a launch
OPTS = V.VoxelOptions(leaf=0.2)
POINTS = (0, 1, 63, 64, 65, 255, 256, 257, 5000)
VARIANTS = {"no_wave_runs": dict(wave=False), "lds_table": dict(lds=True), "no_lds_table": dict(lds=False),
            "probe_again": dict(saved=False), "all_on": dict(wave=True, lds=True, saved=True),
            "all_off": dict(wave=False, lds=False, saved=False)}


def cloud(seed, n):
    """The CPU file's scene, twice as dense, cut to ``n`` points of its seeded order."""
    return np.concatenate([scene(seed), scene(seed + 100)])[:n]


def staged(pl, lay, n):
    """The x, y, z, intensity the kernel reads out of a payload (the intensity is the payload's noise)."""
    raw = np.frombuffer(pl, np.uint8).reshape(n, lay.point_step)
    return np.stack([raw[:, o:o + 4].copy().view("<f4")[:, 0] for o in lay.offsets], 1) if n else np.zeros((0, 4), F)


class Device:
    """One downsampler for the module: every test launches on the same workspace."""

    def __init__(self, dev):
        self.op = V.VoxelDownsampler(dev)

    def run(self, clouds, opts, layout="record16", slots=None, **variant):
        """→ (the device's rows, the definition's rows of the same staged bytes, the call)."""
        lay, mis = LAYOUTS[layout]
        pls = [payload(p, lay) for p in clouds]
        call = self.op.prepare(pls, [len(p) for p in clouds], lay, opts, misalign=mis, slots=slots)
        for t in (call.out, call.table, call.memo, call.blocks):
            t.fill_(SENT)  # the launch owns its reset, and nothing past the used records and the counts
        V.launch(call, **variant)
        torch.cuda.synchronize()
        raw = call.out.cpu().numpy()
        got = V.rows_of(raw, call)
        assert (raw[call.out_bytes:] == SENT).all(), "written past the counts"
        at = 0
        for rows, n in zip(got, call.ns):
            assert (raw[16 * (at + len(rows)):16 * (at + n)] == SENT).all(), "written past the used records"
            at += n
        return got, [V.downsample_numpy(staged(pl, lay, len(p)), opts) for pl, p in zip(pls, clouds)], call


@pytest.fixture(scope="module")
def device(cuda):
    return Device(cuda)


def same(got, want, what=""):
    assert len(got) == len(want), what
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype == F and g.shape == w.shape, (what, b, g.shape, w.shape)
        np.testing.assert_array_equal(g.view("<u4"), w.view("<u4"), err_msg=f"{what} cloud {b}")


@pytest.mark.parametrize("n", POINTS)
@pytest.mark.parametrize("layout", ["record16", "step32", "record16_mis4"])
def test_bit_for_bit_the_definition(device, layout, n):
    got, want, _ = device.run([cloud(n, n)], OPTS, layout)
    assert len(want[0]) >= n // 4  # (the noise intensities, NaNs and infinities among them, are clamped alike)
    same(got, want, f"{layout} {n} points")


@pytest.mark.parametrize("min_points", [1, 3])
@pytest.mark.parametrize("leaf", [0.01, (0.5, 0.25, 1.0), 100])
def test_leaves_and_min_points(device, leaf, min_points):
    # 0.01: nearly every point its own voxel, the table at its highest load; 100: seven voxels, contention
    got, want, _ = device.run([cloud(7, 5000), cloud(8, 700)], V.VoxelOptions(leaf=leaf, min_points=min_points), "step32")
    assert len(want[0]) == {(0.01, 1): 5000, (0.01, 3): 0, (100, 1): 7, (100, 3): 7}.get((leaf, min_points), len(want[0]))
    same(got, want, f"leaf {leaf} min_points {min_points}")


def test_a_full_table_gives_the_same_bytes(device):
    pts, o = cloud(9, 4096), V.VoxelOptions(leaf=0.01)
    full, want, call = device.run([pts], o, slots=[4096])  # 100 % load: probe chains that wrap
    assert call.slots == (4096,) and len(want[0]) >= 4090
    same(full, want, "slots == points")
    same(device.run([pts], o)[0], want, "the default size")


def test_a_ragged_batch_and_a_relaunch_with_another(device):
    junk = np.array([[np.nan, 1, 1], [1, np.inf, 1], [600, 0, 0], [0, -513, 0], [1, 1, np.nan]], F).repeat(60, 0)
    got, want, _ = device.run([cloud(10, 3000), np.zeros((0, 3), F), junk], OPTS, "record16_mis4")
    assert [len(w) > 0 for w in want] == [True, False, False]
    same(got, want, "first batch")
    got, want, _ = device.run([cloud(12, 257), cloud(13, 4000)], OPTS, "record16_mis4")  # the same, dirtied workspace
    same(got, want, "second batch")


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_the_variants_give_the_same_bytes(device, variant):
    for leaf in (0.2, 100):
        got, want, _ = device.run([cloud(20, 5000), cloud(21, 300)], V.VoxelOptions(leaf=leaf, min_points=2), **VARIANTS[variant])
        same(got, want, f"{variant} leaf {leaf}")


def test_launcher_refusals(device):
    from triton_client_amd import _native

    (_,), (want,), c = device.run([cloud(50, 300)], OPTS)
    c.out.fill_(SENT)
    p, o = _native.ptr, c.layout.offsets
    ns, slots = np.array([300], np.int32), np.array([1024], np.int32)
    base = dict(data=p(c.data), data_bytes=c.data_bytes, frame_off=p(c.frame_off), frame_n=p(c.frame_n), ns=ns.ctypes.data,
                slots=slots.ctypes.data, batch=1, step=16, ox=o[0], oy=o[1], oz=o[2], oi=o[3], lx=0.2, ly=0.2, lz=0.2,
                min_points=1, wave=1, lds=1, saved=1, table=p(c.table), table_bytes=c.table_bytes, memo=p(c.memo),
                memo_bytes=c.memo_bytes, blocks=p(c.blocks), blocks_bytes=c.blocks_bytes, out=p(c.out),
                out_bytes=c.rows_bytes, counts=p(c.counts), stream=_native.stream_ptr())
    small, odd, two = np.array([256], np.int32), np.array([768], np.int32), np.array([300, 300], np.int32)
    fn = _native.kernels().tca_voxel_downsample
    bad = {"short table": dict(table_bytes=c.table_bytes - 1), "short memo": dict(memo_bytes=c.memo_bytes - 1),
           "short blocks": dict(blocks_bytes=c.blocks_bytes - 1), "short out": dict(out_bytes=c.rows_bytes - 1),
           "misaligned table": dict(table=p(c.table) + 8), "misaligned out": dict(out=p(c.out) + 4),
           "misaligned memo": dict(memo=p(c.memo) + 2), "a field outside the record": dict(oz=16),
           "an intensity outside the record": dict(oi=14), "leaf nan": dict(ly=float("nan")), "leaf 0.001": dict(lx=0.001),
           "leaf 101": dict(lz=101.0), "min_points 0": dict(min_points=0), "65 clouds": dict(batch=65),
           "2^31 bytes": dict(data_bytes=2 ** 31), "fewer slots than points": dict(slots=small.ctypes.data),
           "slots no power of two": dict(slots=odd.ctypes.data), "points past the records": dict(ns=two.ctypes.data, batch=2),
           "null counts": dict(counts=0), "lds 2": dict(lds=2)}
    for what, kw in bad.items():
        assert fn(*{**base, **kw}.values()) == 1, what  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (c.out == SENT).all()  # nothing was launched
    assert fn(*base.values()) == 0
    torch.cuda.synchronize()
    same(V.rows_of(c.out.cpu().numpy(), c), [want])


# ------------------------------------------------------------------------ through the engine
def test_downsampler_engine_and_driver_give_the_definitions_messages(cuda, monkeypatch):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.inference.engines import Detector3D
    from triton_client_amd.ros.bus import TopicBus

    clouds, _ = _rig_messages()
    want = _wanted(clouds)
    same(V.VoxelDownsampler(cuda).downsample(clouds, RIG), [np.frombuffer(w.data, F).reshape(-1, 4) for w in want])

    def drive(env):
        monkeypatch.setenv("TCA_DEVICE_VOXEL", env)
        eng = _GpuEngine()
        assert Detector3D.downsample_clouds(eng, clouds, RIG) == want
        assert Detector3D.voxel_downsampler(eng) is eng._voxel_downsampler and eng._voxel_downsampler.gpu  # made once
        bus, got = TopicBus(), []
        compat.Subscriber("/vox", msgs.PointCloud2, got.append, bus=bus)
        drv = RosInference3D(engine=eng, params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=4, workers=2,
                             queue_size=64, voxel_topic="/vox", voxel_options=RIG)
        drv.start_inference(spin=False)
        pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
        for c in clouds:
            pub.publish(c)
        runner = drv.runner
        drv.stop()
        bus.close()
        assert not runner.errors, runner.errors
        assert got == want
        return eng._voxel_downsampler

    assert drive("1")._stream is not None  # the kernel ran
    assert drive("0")._stream is None  # TCA_DEVICE_VOXEL=0: the definition, on a GPU engine too
