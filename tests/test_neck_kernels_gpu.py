"""The fused BEV neck + head kernels (K15, csrc/kernels/bev_neck.hip) one by one against
ops/neck_ref.py: the bf16 kernel ``tca_bev_neck_head`` against its bf16 emulation, the fp32 kernel
``tca_bev_neck_head_x3v`` (plain-fp32 and pair input, tilings 0 / 1 / 2) against the float64
definition, each inside the element-wise bound of docs/precision.md ("Fused BEV neck + head");
the three tilings, the two input storages and a repeated launch must agree bit for bit.

Every input buffer is NaN outside its channel slice, every output is NaN in [0, nh) and a
sentinel in [nh, ldo) before the launch.  Shapes and inputs: ``neck_ref.GEOMETRIES`` (shared
with tests/test_neck_ref.py, which holds the emulations to the same bounds on the CPU).
Each test prints ``NECK_RATIO`` lines: the worst |err| / bound and |err| / (u A) it saw."""
import ctypes
import functools

import pytest
import torch

from triton_client_amd.ops import neck_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -1024.0
GEOMS = [n for n in R.GEOMETRIES if not n.startswith("chunk_")]


@functools.lru_cache(maxsize=None)
def _prepared(name, kind, nh=None):
    """case, packed buffers on the GPU (and the wrapper where it takes nh), comparison target,
    bound and u * A on the CPU: computed once per input set."""
    case = R.make_case(name, kind, nh)
    p, neck = R.pack_case(case, "cuda")
    A, _ = R.magnitude(case.xs, p)
    if kind == "fp32":
        target = R.neck_head_fp64(case.xs, case.geom.strides, case.deconvs, case.head)
        return case, p, neck, target, R.bound_fp32(case.xs, p), R.U_FP32 * A
    e, parts = R.emulate_bf16(case.xs, p)
    return case, p, neck, e.double(), R.bound_bf16(case.xs, p, e, parts), R.U_BF16 * A


def _input_buffers(case, pair, offx, pad):
    """[B, H/s, W/s, cin + pad] buffers, NaN everywhere but channels [offx, offx + cin)."""
    from triton_client_amd.ops.conv import to_pairs
    bufs = []
    for x in case.xs:
        cin = x.shape[-1]
        if case.kind == "bf16":
            t = torch.full((*x.shape[:3], cin + pad), float("nan"), dtype=torch.bfloat16)
            t[..., offx:offx + cin] = x.to(torch.bfloat16)
        else:
            # NaN in both bf16 halves of every word, so a stray pair read cannot see zeros either
            t = torch.full((*x.shape[:3], 2 * (cin + pad)), float("nan"), dtype=torch.bfloat16).view(torch.float32)
            t[..., offx:offx + cin] = to_pairs(x) if pair else x
        bufs.append(t.cuda())
    return bufs


def _output(case, ldo_pad, dtype):
    g = case.geom
    out = torch.full((g.B, g.H, g.W, case.nh + ldo_pad), SENTINEL, dtype=dtype, device="cuda")
    out[..., :case.nh] = float("nan")
    return out


def _launch(kind, p, bufs, offx, out, B, H, W, grid, pair=0, variant=0, cins=None, strides=None, nh=None):
    """The entry point itself.  cins / strides / nh override what the launcher is told (refusals)."""
    from triton_client_amd import _native
    n = len(strides or p.strides)
    ints = lambda v: (ctypes.c_int * n)(*v)  # noqa: E731
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
    args = (n, ptrs(bufs[:n]), ints([b.shape[-1] for b in bufs[:n]]), ints([offx] * n), ints(cins or p.cins),
            ints(strides or p.strides), ptrs(p.w[:n]), ptrs(p.b[:n]), _native.ptr(p.wh), _native.ptr(p.bh),
            nh or p.nh, _native.ptr(out), out.shape[-1], B, H, W, grid)
    if kind == "fp32":
        _native.call("tca_bev_neck_head_x3v", *args, pair, variant, _native.stream_ptr())
    else:
        _native.call("tca_bev_neck_head", *args, _native.stream_ptr())


def _run(case, p, neck, grid, pair=0, variant=0, offx=None, pad=None, ldo_pad=None):
    """One launch into fresh buffers: through ``FusedNeckHead`` where it exists (nh % 8 == 0), else
    the entry point.  Returns the whole output buffer on the CPU."""
    from triton_client_amd.ops.conv import NHWC
    fp32 = case.kind == "fp32"
    offx = offx if offx is not None else (8 if pair or not fp32 else 4)
    pad = pad if pad is not None else (32 if not fp32 else 16 if pair else 12)
    ldo_pad = case.geom.ldo_pad if ldo_pad is None else ldo_pad
    bufs = _input_buffers(case, pair, offx, pad)
    out = _output(case, ldo_pad, torch.float32 if fp32 else torch.bfloat16)
    g = case.geom
    if neck is not None:
        neck.grid, neck.variant = grid, variant
        neck([NHWC(b, offx, x.shape[-1], pair=bool(pair)) for b, x in zip(bufs, case.xs)], NHWC(out))
    else:
        _launch(case.kind, p, bufs, offx, out, g.B, g.H, g.W, grid, pair, variant)
    torch.cuda.synchronize()
    return out.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _check(tag, out, nh, target, bound, ua, l2=None):
    assert (out[..., nh:] == SENTINEL).all(), f"{tag}: channels [nh, ldo) were written"
    got = out[..., :nh]
    r = R.compare(got, target, bound, l2)
    fin = torch.isfinite(got)
    ua_ratio = (torch.where(fin, (got.double() - target).abs(), torch.zeros_like(target)) / ua).max().item()
    print(f"NECK_RATIO {tag} err/bound {r['worst']:.4g} err/(uA) {ua_ratio:.4g} rel_l2 {r['rel_l2']:.3g}")
    assert r["ok"], (tag, r)
    return r


def _fp32_all_ways(name, nh=None):
    case, p, neck, target, bound, ua = _prepared(name, "fp32", nh)
    first = None
    for grid in case.geom.grids:
        for pair in (0, 1):
            for variant in (0, 1, 2):
                tag = f"{name} nh{case.nh} fp32 {'pair' if pair else 'plain'} v{variant} grid{grid}"
                out = _run(case, p, neck, grid, pair, variant)
                _check(tag, out, case.nh, target, bound, ua, R.REL_L2_FP32)
                if first is None:
                    first = out
                # tilings, input storages and grids: the same bits
                assert torch.equal(_bits(out), _bits(first)), f"{tag}: differs from plain v0 grid{case.geom.grids[0]}"
    again = _run(case, p, neck, case.geom.grids[0], 0, 0)
    assert torch.equal(_bits(again), _bits(first)), f"{name}: a repeated launch differs (no atomics: a race)"


def _bf16_all_ways(name, nh=None):
    case, p, neck, target, bound, ua = _prepared(name, "bf16", nh)
    first = None
    for grid in case.geom.grids:
        for offx in (8, 32):
            tag = f"{name} nh{case.nh} bf16 offx{offx} grid{grid}"
            out = _run(case, p, neck, grid, offx=offx)
            _check(tag, out, case.nh, target, bound, ua)
            if first is None:
                first = out
            assert torch.equal(_bits(out), _bits(first)), f"{tag}: differs from offx8 grid{case.geom.grids[0]}"
    again = _run(case, p, neck, case.geom.grids[0], offx=8)
    assert torch.equal(_bits(again), _bits(first)), f"{name}: a repeated launch differs (no atomics: a race)"


@pytest.mark.parametrize("name", GEOMS)
def test_fp32_kernel_vs_fp64(cuda, name):
    """Plain and pair input, tilings 0 / 1 / 2, the geometry's grids; nh 8 / 40 / 72 / 80 through
    FusedNeckHead, ldo = nh or nh + 8, offx 4 (plain, ldx = cin + 12) or 8 (pair, ldx = cin + 16)."""
    _fp32_all_ways(name)


@pytest.mark.parametrize("name", GEOMS)
def test_bf16_kernel_vs_emulation(cuda, name):
    """offx 8 and 32 in buffers of ldx = cin + 32, the geometry's grids."""
    _bf16_all_ways(name)


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
@pytest.mark.parametrize("name,nh", [("one_branch_odd", 4), ("partial_three_frames", 36)])
def test_nh_multiple_of_4_at_the_entry_point(cuda, name, nh, kind):
    """The launchers take nh % 4 == 0 (the wrapper asks for 8): hand-packed wh / bh."""
    assert _prepared(name, kind, nh)[2] is None
    (_fp32_all_ways if kind == "fp32" else _bf16_all_ways)(name, nh)


@pytest.mark.parametrize("name", ["chunk_two_launches", "chunk_largest_yg"])
def test_fp32_batch_chunking(cuda, name):
    """chunk = 32767 // (H/S): H 8192, B 5 runs as launches of 3 and 2 frames; H 4681, B 7 as one
    launch whose last q-grid row is Yg = 32766.  Against fp64, and the chunked batch against
    per-frame launches bit for bit."""
    case, p, neck, target, bound, ua = _prepared(name, "fp32")
    g = case.geom
    assert 32767 // g.H == (3 if name == "chunk_two_launches" else 7)
    outs = []
    for pair, variant in ((0, 2), (1, 0), (0, 1)):
        out = _run(case, p, neck, g.grids[0], pair, variant)
        _check(f"{name} fp32 pair{pair} v{variant}", out, case.nh, target, bound, ua, R.REL_L2_FP32)
        outs.append(out)
    assert all(torch.equal(_bits(o), _bits(outs[0])) for o in outs[1:])
    if name == "chunk_two_launches":
        bufs = _input_buffers(case, 0, 4, 12)
        per_frame = _output(case, g.ldo_pad, torch.float32)
        for b in range(g.B):
            _launch("fp32", p, [t[b:b + 1] for t in bufs], 4, per_frame[b:b + 1], 1, g.H, g.W, g.grids[0], 0, 2)
        torch.cuda.synchronize()
        assert torch.equal(_bits(per_frame.cpu()), _bits(outs[0]))


REFUSALS = [  # (id, kinds, geometry, launcher arguments that break the contract)
    ("grid_12", ("fp32", "bf16"), "second_two_branches", dict(grid=12)),
    ("stride_not_dividing", ("fp32", "bf16"), "second_two_branches", dict(strides=[2, 3], H=6, W=12)),
    ("H_not_multiple_of_S", ("fp32", "bf16"), "second_two_branches", dict(H=5)),
    ("cin_48", ("fp32",), "one_branch_odd", dict(cins=[48])),
    ("cin_96", ("bf16",), "no_stride_one", dict(cins=[64, 96])),
    ("nh_84", ("fp32", "bf16"), "one_branch_odd", dict(nh=84)),
    ("nh_6", ("fp32", "bf16"), "one_branch_odd", dict(nh=6)),
    ("variant_3", ("fp32",), "one_branch_odd", dict(variant=3)),
    ("pair_offx_4", ("fp32",), "one_branch_odd", dict(pair=1, offx=4)),
]


@pytest.mark.parametrize("rid,kind,name,bad", [(r, k, n, b) for r, ks, n, b in REFUSALS for k in ks],
                         ids=[f"{r}-{k}" for r, ks, _, _ in REFUSALS for k in ks])
def test_launcher_refuses(cuda, rid, kind, name, bad):
    """hipErrorInvalidValue from the launcher, nothing launched: the output keeps its fill.  The
    buffers are those of a legal call, so nothing here could reach a kernel outside its contract."""
    from triton_client_amd import _native
    case, p, _, _, _, _ = _prepared(name, kind)
    g = case.geom
    bad = dict(bad)
    offx = bad.pop("offx", 8)
    bufs = _input_buffers(case, bad.get("pair", 0), 8, 32 if kind == "bf16" else 16)
    out = _output(case, 8, torch.float32 if kind == "fp32" else torch.bfloat16)
    before = out.clone()
    kw = dict(B=g.B, H=g.H, W=g.W, grid=8)
    kw.update(bad)
    with pytest.raises(_native.NativeError, match=r"invalid argument \(1\)"):
        _launch(kind, p, bufs, offx, out, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(before))
