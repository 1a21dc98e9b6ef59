"""K35 on the device: ``tca_voxel_normals`` behind ``tca_voxel_downsample`` is bit for bit ``normals_numpy``."""
import numpy as np
import pytest
import torch

from test_laser_scan_gpu import LAYOUTS, _GpuEngine, payload
from test_range2d import _rig_messages
from test_voxel_downsample_gpu import SENT, same, staged
from test_voxel_normals import ANGLE, CURV, OPTS, SCENES, F, angle, planes
from triton_client_amd.ops import voxel_downsample as V

pytestmark = pytest.mark.gpu

FINE = V.VoxelOptions(leaf=0.125, normal_radius=0.5)  # r = 4 leaves: the most neighbours a voxel can have
GRID = (np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), -1).reshape(-1, 3) - 5.5).astype(F) * F(0.125)
CORNERS = np.array([[x, y, z] for x in (-0.05, 0.05) for y in (-0.05, 0.05) for z in (-0.05, 0.05)], F)


@pytest.fixture(scope="module")
def op(cuda):
    return V.VoxelDownsampler(cuda)  # every test launches on the same workspace


def run(op, clouds, opts, layout="record16", slots=None, stage=None):
    """→ (the device's rows [K, 8], the definition's of the same staged bytes, the call)."""
    lay, mis = LAYOUTS[layout]
    pls = [payload(p, lay) for p in clouds]
    call = op.prepare(pls, [len(p) for p in clouds], lay, opts, misalign=mis, slots=slots)
    for t in (call.out, call.table, call.memo, call.blocks, call.normals):
        t.fill_(SENT)  # the launch owns its resets
    V.launch(call, stage=stage)
    torch.cuda.synchronize()
    nrm, at = call.normals.cpu().numpy(), 0
    got = V.rows_of(call.out.cpu().numpy(), call, nrm)
    for rows, n in zip(got, call.ns):
        assert (nrm[16 * (at + len(rows)):16 * (at + n)] == SENT).all(), "normals written past the used records"
        at += n
    assert (nrm[call.rows_bytes:] == SENT).all()
    want = [V.downsample_numpy(staged(pl, lay, len(p)), opts) for pl, p in zip(pls, clouds)]
    return got, [np.concatenate([w, V.normals_numpy(w, opts)], 1) for w in want], call


@pytest.mark.parametrize("stage", [True, False])
def test_a_ragged_batch_across_zero_and_a_relaunch(op, stage):
    wide = planes([(0.3, -0.2, 1.0)], [0.0], 0.01, n=5000, side=6.0) - np.array([1, 2, 0], F)  # both signs on every axis
    junk, few = np.full((70, 3), np.nan, F), np.array([[1, 1, 1], [1.01, 1, 1], [-3, 2, 1]], F)
    got, want, _ = run(op, [wide, junk, few], OPTS, "record16_mis4", stage=stage)
    assert [len(w) for w in want[1:]] == [0, 2] and np.isnan(want[2]).sum() == 8 and not np.isnan(want[0]).all()
    same(got, want, "first batch")
    got, want, _ = run(op, [few, planes(*SCENES["edge"][:3], n=4000)], OPTS, "step32", stage=stage)  # the dirtied workspace
    same(got, want, "second batch")


@pytest.mark.parametrize("stage", [True, False])
def test_cells_diagonal_full_and_wrapping(op, stage):
    # every voxel alone in its cell, its seven neighbours in the cells across a face, an edge or the corner
    got, want, _ = run(op, [CORNERS + F(0.5), CORNERS, CORNERS - F(0.5)], FINE, stage=stage)
    assert all(len(w) == 8 and not np.isnan(w).any() for w in want)
    same(got, want, "diagonal cells")
    # a filled block: 64 rows a cell, 27 cells of candidates (more than one LDS tile), up to 257 neighbours
    got, want, _ = run(op, [GRID], FINE, stage=stage)
    assert len(want[0]) == 1728 and V.moments_numpy(want[0], FINE)[0].max() == 257
    same(got, want, "12 x 12 x 12 block")
    far = (np.arange(24, dtype=F).reshape(8, 3) - 12) * F(7)  # eight cells in a table of eight slots: probes wrap
    got, want, call = run(op, [far], FINE, slots=[8], stage=stage)
    assert call.slots == (8,) and len(want[0]) == 8 and (want[0][:, 4:].view("<u4") == 0x7FC00000).all()
    same(got, want, "a full cell table")


def test_device_against_the_reference(op):
    nrm, off, noise, o, _ = SCENES["off_origin"]
    (got,), _, _ = run(op, [planes(nrm, off, noise)], o)
    ref, m, odd, flat = V.normals_ref(got[:, :4], o)
    ok = ~(odd | flat)
    assert ok.mean() >= 0.95 and angle(got[ok, 4:7].astype(np.float64), ref[ok, :3]).max() <= ANGLE
    assert np.abs(got[ok, 7] - ref[ok, 3]).max() <= CURV and (V.moments_numpy(got, o)[0][~odd] == m[~odd]).all()


def test_launcher_refusals_and_the_engine(op, cuda, monkeypatch):
    from triton_client_amd import _native
    from triton_client_amd.inference.engines import Detector3D
    (_,), (want,), c = run(op, [GRID[:300]], FINE)
    c.normals.fill_(SENT)
    p = _native.ptr
    ns, slots = np.array(c.ns, np.int32), np.array(c.slots, np.int32)
    base = dict(rows=p(c.out), rows_bytes=c.rows_bytes, counts=p(c.counts), ns=ns.ctypes.data, slots=slots.ctypes.data, batch=1,
                radius=FINE.radius_q, stage=1, table=p(c.table), table_bytes=c.table_bytes, normals=p(c.normals),
                normals_bytes=c.rows_bytes, stream=_native.stream_ptr())
    fn = _native.kernels().tca_voxel_normals
    for what, kw in {"short table": dict(table_bytes=c.table_bytes - 1), "short normals": dict(normals_bytes=c.rows_bytes - 1),
                     "short rows": dict(rows_bytes=c.rows_bytes - 1), "misaligned normals": dict(normals=p(c.normals) + 4),
                     "misaligned table": dict(table=p(c.table) + 8), "radius 0": dict(radius=0), "radius 4.1": dict(radius=268698),
                     "stage 2": dict(stage=2), "65 clouds": dict(batch=65), "null counts": dict(counts=0)}.items():
        assert fn(*{**base, **kw}.values()) == 1, what  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (c.normals == SENT).all()  # nothing was launched
    assert fn(*base.values()) == 0
    torch.cuda.synchronize()
    same(V.rows_of(c.out.cpu().numpy(), c, c.normals.cpu().numpy()), [want])
    clouds, _ = _rig_messages()
    on = V.VoxelOptions(leaf=(0.5, 0.25, 1.0), min_points=2, normal_radius=1.0)
    wanted = [V.downsample_message(m, V.downsample_cloud_numpy(m, on)) for m in clouds]
    for env in ("1", "0"):  # the kernels, then the definition on a GPU engine
        monkeypatch.setenv("TCA_DEVICE_VOXEL", env)
        eng = _GpuEngine()
        assert Detector3D.downsample_clouds(eng, clouds, on) == wanted and wanted[0].point_step == 32
        assert (eng._voxel_downsampler._stream is not None) == (env == "1")
