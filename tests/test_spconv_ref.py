"""The NumPy references of the sparse-conv kernels (ops/spconv_ref.py) against the
project's trusted CPU layer, models.second.SparseConv3d (itself tested against a
dense conv3d in test_second.py), on the four layer kinds of voxel_backbone_8x."""
import numpy as np
import pytest
import torch

from triton_client_amd.config.lidar import SparseConvSpec
from triton_client_amd.models.second import SparseConv3d
from triton_client_amd.ops import spconv_ref as R

DIMS = (9, 12, 14)  # three distinct extents: an axis swap cannot cancel

KINDS = {
    "subm": SparseConvSpec(8, 16),
    "s2_p1": SparseConvSpec(8, 16, False, stride=(2, 2, 2)),
    "s2_p011": SparseConvSpec(8, 16, False, stride=(2, 2, 2), padding=(0, 1, 1)),
    "k311": SparseConvSpec(8, 16, False, kernel=(3, 1, 1), stride=(2, 1, 1), padding=(0, 0, 0)),
}


def _ksp(spec):
    return tuple(spec.kernel) + tuple(spec.stride) + tuple(spec.padding)


def test_edge_sites_hold_the_forced_cases():
    c = R.sp_edge_sites(np.random.default_rng(0), DIMS)
    Z, Y, X = DIMS
    g = R.sp_grid(c, 2, DIMS) >= 0
    assert len(np.unique(c, axis=0)) == len(c) and 0.08 < (len(c) - g[:, 2:6, 3:7, 4:8].sum()) / g.size < 0.2
    assert g[0, Z - 1, Y - 1, X - 1] and g[1, 0, 0, 0] and g[:, ::Z - 1, ::Y - 1, ::X - 1].all()
    assert g[0, 2:6, 3:7, 4:8].all()
    assert g[1, 2:7, 1:6, 1:6].sum() == 1 and g[1, 4, 3, 3]
    assert g[0, 6:8, 8:11, 9:12].sum() >= 2 and (g[0, 6:8, 8:11, 9:12] == g[1, 6:8, 8:11, 9:12]).all()
    n = R.sp_neighbour_table(c, _ksp(KINDS["subm"]), DIMS, R.sp_grid(c, 2, DIMS))
    taps = (n >= 0).sum(1)
    assert taps.max() == 27 and taps.min() == 1  # all 27 taps / the centre tap only
    lone = np.flatnonzero(taps == 1)
    assert (n[lone, 13] == lone).all()


def test_pack_unpack_and_masks():
    rng = np.random.default_rng(1)
    nbr = rng.integers(-1, 50, (150, 27)).astype(np.int32)
    nbr[64:128] = -1
    nbr[128:, :26] = -1
    nbr[128, 26] = 3
    p = R.sp_pack_nbr(nbr, tiles=4, fill=-9)
    assert p.shape == (4, 27, 64)
    assert p[1, 5, 7] == nbr[64 + 7, 5] and p[2, 26, 0] == 3 and (p[3] == -9).all() and (p[2, :, 22:] == -9).all()
    assert np.array_equal(R.sp_unpack_nbr(p, 150), nbr)
    m = R.sp_tap_masks(nbr)
    assert m.dtype == np.uint32 and m[1] == 0 and m[2] == 1 << 26
    assert m[0] == sum(1 << t for t in range(27) if (nbr[:64, t] >= 0).any())


@pytest.mark.parametrize("kind", list(KINDS))
def test_reference_matches_sparse_conv_module(kind):
    spec = KINDS[kind]
    ksp = _ksp(spec)
    torch.manual_seed(3)
    coords = R.sp_edge_sites(np.random.default_rng(2), DIMS)
    feats = torch.randn(len(coords), spec.cin)
    layer = SparseConv3d(spec).eval()
    with torch.no_grad():
        layer.bn.running_mean.copy_(torch.randn(spec.cout) * 0.1)
        layer.bn.running_var.copy_(torch.rand(spec.cout) * 0.5 + 0.75)
        layer.bn.bias.copy_(torch.randn(spec.cout) * 0.3)
    layer.fuse_bn()
    with torch.no_grad():
        y, co, shp = layer(feats, torch.from_numpy(coords), DIMS)
    od = R.sp_out_dims(DIMS, ksp)
    assert tuple(shp) == od
    if spec.subm:
        assert od == DIMS
        out_sites = coords
    else:
        out_sites = R.sp_out_sites(coords, ksp, od)
    assert np.array_equal(out_sites, co.numpy())  # same site set, same (sorted) order
    nbr = R.sp_neighbour_table(out_sites, ksp, DIMS, R.sp_grid(coords, 2, DIMS))
    w = layer.weight.detach().reshape(spec.cout, spec.taps, spec.cin).numpy()
    ref, S = R.sp_gather_gemm_ref(feats.numpy(), nbr, w, layer.bias.detach().numpy(), 1)
    err = np.abs(ref - y.numpy().astype(np.float64)).max()
    print(kind, "rows", len(out_sites), "max |ref - module|", err)
    assert err < 1e-5
    assert (ref > 0).any() and (ref == 0).any() and (S >= np.abs(ref)).all()
    # and without the ReLU: the module's pre-activation sign survives
    lin, _ = R.sp_gather_gemm_ref(feats.numpy(), nbr, w, layer.bias.detach().numpy(), 0)
    assert np.array_equal(np.maximum(lin, 0.0), ref) and (lin < 0).any()


def test_mean_vfe_references_agree():
    from triton_client_amd.models.second import mean_vfe
    rng = np.random.default_rng(4)
    P = 5
    pts = rng.standard_normal((40, 8)).astype(np.float32)
    vcount = np.array([0, 1, 3, 5, 9], np.int32)
    slots = rng.integers(0, 40, (5, P)).astype(np.int32)
    vox = np.zeros((5, P, 4), np.float32)
    for v in range(5):
        m = min(vcount[v], P)
        vox[v, :m] = pts[slots[v, :m], :4]
    num = np.minimum(vcount, P)
    a, ma = R.mean_vfe_slots_ref(pts, slots, vcount, P)
    b, mb = R.mean_vfe_voxels_ref(vox, num)
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-15)
    np.testing.assert_allclose(ma, mb, rtol=0, atol=1e-15)
    ref = mean_vfe(torch.from_numpy(vox), torch.from_numpy(num.astype(np.int64))).numpy()
    np.testing.assert_allclose(a, ref, rtol=0, atol=1e-6)
    assert (a[0] == 0).all()
