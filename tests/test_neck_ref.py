"""ops/neck_ref.py (the references of the fused BEV neck + head kernels, K15): the float64
definition against ``torch.nn``, the packed-buffer evaluation against the definition, both
emulations of the kernels' arithmetic against the element-wise bounds on every input set of
tests/test_neck_kernels_gpu.py, and the comparator against the defects it has to catch."""
import functools

import pytest
import torch
import torch.nn.functional as F

from triton_client_amd.ops import neck_ref as R


@functools.lru_cache(maxsize=None)
def _set(name, kind, nh=None):
    """case, packed buffers, fp64 definition, and the kernel's comparison target + bound."""
    case = R.make_case(name, kind, nh)
    p, _ = R.pack_case(case, "cpu")
    ref = R.neck_head_fp64(case.xs, case.geom.strides, case.deconvs, case.head)
    if kind == "fp32":
        return case, p, ref, ref, R.bound_fp32(case.xs, p)
    e, parts = R.emulate_bf16(case.xs, p)
    return case, p, ref, e.double(), R.bound_bf16(case.xs, p, e, parts)


def _ids(sets):
    return [f"{n}-{k}" + (f"-nh{h}" if h else "") for n, k, h in sets]


# --------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("name", ["one_branch_odd", "second_two_branches", "partial_three_frames", "no_stride_one"])
def test_fp64_definition_matches_torch_modules(name):
    """strides [1], [1, 2], [1, 2, 4], [2, 4] against ConvTranspose2d / Conv2d in float64."""
    case = R.make_case(name, "fp32")
    dec, head = R.modules(case)
    with torch.no_grad():
        cat = torch.cat([F.relu(d.double()(x.double().permute(0, 3, 1, 2))) for d, x in zip(dec, case.xs)], 1)
        want = head.double()(cat).permute(0, 2, 3, 1)
    got = R.neck_head_fp64(case.xs, case.geom.strides, case.deconvs, case.head)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-13)
    # modules and raw weights are the same thing to it
    assert torch.equal(got, R.neck_head_fp64(case.xs, case.geom.strides, dec, head))


# --------------------------------------------------------------------------- the host packing
_SMALL = [t for t in R.GPU_SETS if not t[0].startswith("chunk_")]  # the chunking sets repeat one_branch_odd's packing


@pytest.mark.parametrize("name,kind,nh", _SMALL, ids=_ids(_SMALL))
def test_packed_buffers_evaluate_to_the_definition(name, kind, nh):
    """hi + lo keeps 16 significant bits of a weight (|w - hi - lo| <= 2^-16 |w|; bf16 alone 2^-8),
    so the float64 evaluation of the packed buffers is within 2 w_u A of the definition: w_u A1 from
    the deconv weights carried through the head, w_u A from the head's own (second order: 2^-7)."""
    case, p, ref, _, _ = _set(name, kind, nh)
    wu = 2.0 ** -16 if kind == "fp32" else 2.0 ** -8
    dec, (hh, hl) = R.unpack(p)
    for (hi, lo), (w, b), s, pb in zip(dec, case.deconvs, case.geom.strides, p.b):
        want = w.permute(2, 3, 1, 0).reshape(s * s * R.CB, -1).double()  # row (sy*s + sx)*128 + co
        assert ((hi.double() + lo.double() - want).abs() <= wu * want.abs()).all()
        assert torch.equal(pb, b.repeat(s * s))
    want = case.head[0].double()
    assert ((hh.double() + hl.double())[:case.nh] - want).abs().le(wu * want.abs()).all()
    assert hh[case.nh:].abs().sum() == 0 and hl[case.nh:].abs().sum() == 0 and p.bh[case.nh:].abs().sum() == 0
    assert p.wh.shape == (80, (2 if kind == "fp32" else 1) * 128 * len(case.xs)) and p.bh.shape == (80,)
    got = R.neck_head_from_packed(case.xs, p)
    A, _ = R.magnitude(case.xs, p)
    err = (got - ref).abs()
    assert (err <= 2 * wu * (1 + 2.0 ** -7) * A).all(), (err / (wu * A)).max().item()
    if kind == "fp32":
        assert R.rel_l2(got, ref) < 2.0 ** -16


# --------------------------------------------------------------------------- emulations vs bounds
@pytest.mark.parametrize("name,kind,nh", R.GPU_SETS, ids=_ids(R.GPU_SETS))
def test_emulation_is_inside_the_bound(name, kind, nh):
    """The acceptance condition of the bounds, set before any GPU run: the kernels' arithmetic on
    the CPU sits inside them on every input set the GPU tests use."""
    case, p, ref, target, bound = _set(name, kind, nh)
    if kind == "fp32":
        r = R.compare(R.emulate_fp32(case.xs, p), target, bound, R.REL_L2_FP32)
    else:
        # another accumulation order (its limit: exact sums rounded once), stored as bf16
        e2, _ = R.emulate_bf16(case.xs, p, exact_acc=True)
        r = R.compare(R.bf16r(e2), target, bound)
        # and the bf16 arithmetic is the definition to bf16 accuracy: three roundings (input given,
        # weights, intermediate) on each path through A
        A, _ = R.magnitude(case.xs, p)
        assert ((target - ref).abs() <= 4 * 2.0 ** -8 * A).all()
    print(name, kind, nh, r)
    assert r["ok"], r
    assert r["worst"] < 1.0


# --------------------------------------------------------------------------- the comparator rejects
def _exact(name, kind):
    case, p, ref, target, bound = _set(name, kind)
    got = target.float() if kind == "fp32" else R.bf16r(target.float())
    l2 = R.REL_L2_FP32 if kind == "fp32" else None
    assert R.compare(got, target, bound, l2)["ok"]
    return case, p, got, target, bound, l2


@pytest.mark.parametrize("name", ["frame_edges", "one_past_full", "second_two_branches", "one_branch_odd"])
def test_comparator_rejects_one_element_off(name):
    """2^-12 A on one element (16 u A; c is below 14 for every case)."""
    case, p, got, target, bound, l2 = _exact(name, "fp32")
    A, _ = R.magnitude(case.xs, p)
    assert R.c_fp32(case.geom.cins32) < 14
    for idx in [(0, 0, 0, 0), tuple(d - 1 for d in got.shape)]:
        bad = got.clone()
        bad[idx] += (2.0 ** -12 * A[idx]).float()
        r = R.compare(bad, target, bound, l2)
        assert "bound" in r["failed"] and r["outside"] == 1, r


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["frame_edges", "one_past_full", "partial_three_frames"])
def test_comparator_rejects_a_pixel_left_at_its_fill_value(name, kind):
    """The last valid pixel of the partial tile of the last class keeps the NaN fill."""
    case, p, got, target, bound, l2 = _exact(name, kind)
    g = case.geom
    S = max(g.strides)
    nq = (g.H // S) * (g.W // S)
    b, y, x = R.class_pixel(S, g.B, g.H, g.W, S * S - 1, g.B * nq - 1)
    assert (b, y, x) == (g.B - 1, g.H - 1, g.W - 1)
    bad = got.clone()
    bad[b, y, x] = float("nan")
    r = R.compare(bad, target, bound, l2)
    assert r["failed"] == ["finite"] and r["nonfinite"] == case.nh, r


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["nearly_empty", "second_two_branches", "no_stride_one"])
def test_comparator_rejects_exchanged_subpixel_classes(name, kind):
    case, p, got, target, bound, l2 = _exact(name, kind)
    S = max(case.geom.strides)
    bad = got.clone()
    bad[:, 0::S, 0::S], bad[:, 0::S, 1::S] = got[:, 0::S, 1::S], got[:, 0::S, 0::S]
    r = R.compare(bad, target, bound, l2)
    assert "bound" in r["failed"] and r["worst"] > 10, r


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["frame_edges", "one_branch_odd"])
def test_comparator_rejects_an_unpermuted_head_chunk(name, kind):
    """One 32-channel chunk of the head contraction pairs accumulator position q with weight column
    q instead of perm(q)."""
    case, p, got, target, bound, l2 = _exact(name, kind)
    perm = torch.tensor(R._perm32())
    w = case.head[0].clone()
    c = w.shape[1] // 32 - 1
    w[:, c * 32:(c + 1) * 32] = case.head[0][:, c * 32 + perm]
    bad = R.neck_head_fp64(case.xs, case.geom.strides, case.deconvs, (w, case.head[1])).float()
    r = R.compare(bad if kind == "fp32" else R.bf16r(bad), target, bound, l2)
    assert "bound" in r["failed"] and r["worst"] > 10, r


@pytest.mark.parametrize("name", ["frame_edges", "one_branch_odd", "second_two_branches", "partial_three_frames"])
def test_comparator_rejects_a_dropped_lo_hi_term(name):
    """Without x_lo * w_hi a product keeps 8 bits of x.  The errors of a sum's terms have random
    signs, so against A (a sum of magnitudes) the element-wise arm need not see it; the relative
    L2 arm does, by more than an order of magnitude."""
    case, p, got, target, bound, l2 = _exact(name, "fp32")
    r = R.compare(R.emulate_fp32(case.xs, p, drop_lohi=True), target, bound, l2)
    print(name, r)
    assert not r["ok"] and "rel_l2" in r["failed"] and r["rel_l2"] > 10 * R.REL_L2_FP32, r
