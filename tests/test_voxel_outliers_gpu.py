"""K36 on the device: ``tca_voxel_outliers`` between ``tca_voxel_downsample`` and ``tca_voxel_normals`` is bit for bit
``outliers_numpy``: the counts, the kept records in their order and the normals of the filtered cloud."""
import numpy as np
import pytest
import torch

from test_laser_scan_gpu import LAYOUTS, payload
from test_range2d import _rig_messages
from test_voxel_downsample_gpu import SENT, same, staged
from triton_client_amd.ops import voxel_downsample as V

pytestmark = pytest.mark.gpu

F = np.float32
# leaf 0.25, the ball 0.5; "ror" runs without the normals behind it
MODES = {"sor1": dict(outlier_mean_k=1, normal_radius=0.5), "sor5": dict(outlier_mean_k=5, normal_radius=0.5),
         "sor16": dict(outlier_mean_k=16, outlier_stddev=0.5, normal_radius=0.5), "ror": dict(outlier_min_neighbors=3),
         "both": dict(outlier_min_neighbors=3, outlier_mean_k=5, normal_radius=0.5)}
FAR = np.array([[40, 0, 0], [0, 40, 0], [0, 0, 40], [-40, 0, 0], [0, -40, 0], [0, 0, -40]], F)  # nobody's neighbours
EMPTY = np.zeros((0, 3), F)
FIVE = np.array([[0.125, 0.125, 0.125], [0.375, 0.125, 0.125], [0.125, 0.375, 0.125], [0.375, 0.375, 0.125], [9, 9, 9]], F)
LINE = np.stack([F(0.3) * np.arange(40, dtype=F) + F(0.1), np.full(40, 1.1, F), np.full(40, -2.1, F)], 1)  # found = 2 < k
SHEET = (np.stack(np.meshgrid(np.arange(27), np.arange(26), [3], indexing="ij"), -1).reshape(-1, 3).astype(F) + F(0.5)) * F(0.25)
SHEET[[100, 255, 256, 300, 511, 600]] = FAR  # 702 voxels; the survivors' ranks shift across the blocks' ends at 256 and 512
CUBE = (np.stack(np.meshgrid(*[np.arange(-4, 4)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F) + F(0.5)) * F(0.25)


def opts_of(mode):
    return V.VoxelOptions(leaf=0.25, outlier_radius=0.5, **MODES[mode])


@pytest.fixture(scope="module")
def op(cuda):
    return V.VoxelDownsampler(cuda)  # every test launches on the same workspace


def fetch(call):
    """→ (the rows per cloud, the used bytes of the counts, the kept records and the normals)."""
    torch.cuda.synchronize()
    out, kept = call.out.cpu().numpy(), call.kept.cpu().numpy()
    nrm = None if call.normals is None else call.normals.cpu().numpy()
    got, at, used = V.rows_of(out, call, nrm, kept), 0, [out[call.rows_bytes:call.out_bytes].tobytes()]
    for rows, n in zip(got, call.ns):
        for buf in (kept,) if nrm is None else (kept, nrm):
            assert (buf[16 * (at + len(rows)):16 * (at + n)] == SENT).all(), "written past the used records"
            used.append(buf[16 * at:16 * (at + len(rows))].tobytes())
        at += n
    assert (kept[call.rows_bytes:] == SENT).all() and (nrm is None or (nrm[call.rows_bytes:] == SENT).all())
    return got, used


def run(op, clouds, opts, layout="record16", slots=None):
    """→ (the device's rows, the definition's of the same staged bytes, the used bytes, the call)."""
    lay, mis = LAYOUTS[layout]
    pls = [payload(p, lay) for p in clouds]
    call = op.prepare(pls, [len(p) for p in clouds], lay, opts, misalign=mis, slots=slots)
    for t in (call.out, call.table, call.memo, call.blocks, call.kept, call.normals):
        if t is not None:
            t.fill_(SENT)  # the launch owns its resets
    V.launch(call)
    got, used = fetch(call)
    want = [V.downsample_numpy(staged(pl, lay, len(p)), opts) for pl, p in zip(pls, clouds)]
    want = [w[V.outliers_numpy(w, opts)] for w in want]
    return got, [np.concatenate([w, V.normals_numpy(w, opts)], 1) if opts.normals else w for w in want], used, call


@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_ragged_batch_and_a_relaunch(op, mode):
    o = opts_of(mode)
    got, want, used, call = run(op, [EMPTY, FIVE, LINE, SHEET], o, "record16_mis4")
    kept = [len(w) for w in want]
    assert kept[:2] == [0, 4] and (kept[2] > 0) == (not o.outlier_min_neighbors) and 500 <= kept[3] <= 696
    assert not V.outliers_numpy(SHEET, o)[[100, 255, 256, 300, 511, 600]].any()  # gone on both sides of both ends
    same(got, want, "first launch")
    V.launch(call)  # the workspace as the first launch left it
    again, used_again = fetch(call)
    same(again, want, "relaunch")
    assert used_again == used


@pytest.mark.parametrize("mode", ["sor5", "both"])
def test_all_isolated_then_ties_across_zero(op, mode):
    o = opts_of(mode)
    lone = np.concatenate([FAR * F(k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)]) / F(4)  # 72 voxels, 10 m apart
    got, want, _, call = run(op, [lone, FIVE[4:]], o)  # fetch() has seen every byte of kept and of the normals untouched
    assert [len(w) for w in want] == [0, 0] and call.counts.cpu().tolist() == [0, 0]
    same(got, want, "every voxel isolated")
    # a filled cube about the origin: cells on both sides of zero on every axis (floor, not truncation), 26 equal
    # distances around an inner voxel; FAR behind it and a cell table of as many slots as points
    got, want, _, call = run(op, [np.concatenate([CUBE, FAR]), CUBE[:8]], o, "step32", slots=[1024, 8])
    assert call.slots == (1024, 8) and len(want[0]) in range(300, 513) and V.outlier_scores_numpy(CUBE, o)[0].max() == 32
    same(got, want, "the cube")


def test_launcher_refusals_and_downsample(op, cuda):
    from triton_client_amd import _native
    o = opts_of("both")
    _, want, _, c = run(op, [SHEET[:300]], o)
    c.kept.fill_(SENT), c.normals.fill_(SENT)
    V.launch(V.VoxelCall(**{**c.__dict__, "opts": V.VoxelOptions(leaf=0.25)}))  # the records and counts before the filter
    before = c.counts.cpu().tolist()
    p = _native.ptr
    ns, slots = np.array(c.ns, np.int32), np.array(c.slots, np.int32)
    base = dict(rows=p(c.out), rows_bytes=c.rows_bytes, counts=p(c.counts), ns=ns.ctypes.data, slots=slots.ctypes.data, batch=1,
                radius=o.outlier_radius_q, min_neighbors=3, mean_k=5, stddev=1.0, table=p(c.table), table_bytes=c.table_bytes,
                memo=p(c.memo), memo_bytes=c.memo_bytes, blocks=p(c.blocks), blocks_bytes=c.blocks_bytes, kept=p(c.kept),
                kept_bytes=c.rows_bytes, stream=_native.stream_ptr())
    fn = _native.kernels().tca_voxel_outliers
    for what, kw in {"short table": dict(table_bytes=c.table_bytes - 1), "short kept": dict(kept_bytes=c.rows_bytes - 1),
                     "short rows": dict(rows_bytes=c.rows_bytes - 1), "short memo": dict(memo_bytes=c.memo_bytes - 1),
                     "short blocks": dict(blocks_bytes=c.blocks_bytes - 1), "misaligned kept": dict(kept=p(c.kept) + 4),
                     "misaligned table": dict(table=p(c.table) + 8), "kept is rows": dict(kept=p(c.out)), "radius 0": dict(radius=0),
                     "radius 4.1": dict(radius=268698), "no test": dict(min_neighbors=0, mean_k=0), "k 17": dict(mean_k=17),
                     "N 1001": dict(min_neighbors=1001), "stddev nan": dict(stddev=float("nan")), "stddev 11": dict(stddev=11.0),
                     "65 clouds": dict(batch=65), "null counts": dict(counts=0)}.items():
        assert fn(*{**base, **kw}.values()) == 1, what  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (c.kept == SENT).all() and c.counts.cpu().tolist() == before  # nothing was launched
    assert fn(*base.values()) == 0
    V.launch_normals(c)
    same(fetch(c)[0], want)
    clouds, _ = _rig_messages()
    on = V.VoxelOptions(leaf=(0.5, 0.25, 1.0), min_points=2, normal_radius=1.0, outlier_radius=1.0, outlier_min_neighbors=4, outlier_mean_k=3)
    wanted = [V.downsample_cloud_numpy(m, on) for m in clouds]
    assert all(0 < len(w) < len(V.downsample_cloud_numpy(m, V.VoxelOptions(leaf=on.leaf, min_points=2))) for w, m in zip(wanted, clouds))
    same(V.VoxelDownsampler(cuda).downsample(clouds, on), wanted, "downsample")
