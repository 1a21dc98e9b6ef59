"""Which kernel takes a FusedConv call (ops/conv.py FusedConv.route), without a GPU: route() itself
as a table, __call__ driven with stand-in tensors and recorded native calls (the launch methods
pass what route decided), and the questions the BEV plans ask on the PointPillars backbone's layers.
Every expected value was recorded from the nested chain this function replaced."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from triton_client_amd import _native
from triton_client_amd.models import fast
from triton_client_amd.models.common import ACT_RELU, ACT_SILU
from triton_client_amd.ops import conv as conv_mod
from triton_client_amd.ops.conv import NHWC, PAIR_TILES, FusedConv, Route

SWITCHES = dict(WINO=True, HX3=True, HX3S2=True, S2SP=False, S2SP_TILE=0, WINO_MIN_N=128, HX3_TILE_AUTO=0,
                HX3S2_TILE_AUTO=0, WINO_TILE_AUTO=0)
H, W = 20, 64  # wino_tile(20, 64, 128) == 1, wino_tile(20, 64, 64) == 3


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    """The documented defaults, whatever the environment set at import."""
    for k, v in SWITCHES.items():
        monkeypatch.setattr(conv_mod, k, v)
    monkeypatch.setattr(fast, "WINO_F32_CHAIN", True)


_CONVS = {}


def layer(cin=64, n=128, k=3, s=1, act=ACT_RELU, precision="fp32", transpose=False) -> FusedConv:
    key = (cin, n, k, s, act, precision, transpose)
    if key not in _CONVS:
        m = nn.ConvTranspose2d(cin, n, s, s) if transpose else nn.Conv2d(cin, n, k, s, k // 2)
        _CONVS[key] = FusedConv(m, act=act, device="cpu", precision=precision)
    return _CONVS[key]


S1 = dict(n=128)  # 3x3 s1, Cin 64, N 128, ReLU
S1N = dict(n=64)
S2 = dict(n=64, s=2)  # 3x3 s2, Cin 64, N 64
PP = dict(x_pair=True, out_pair=True)  # pair in, pair out
R = Route
# (layer, route arguments, switches set for the case, expected)
ROUTES = [
    (dict(precision="bf16"), dict(x_pair=False, out_pair=False), {}, R("bf16", 0)),
    (dict(precision="bf16"), dict(x_pair=False, out_pair=False, tile=130), {}, R("bf16", 130)),
    (dict(precision="bf16", k=1), dict(x_pair=False, out_pair=False, res="fp32", tile=5), {}, R("bf16", 5)),
    (dict(n=32, cin=16), dict(x_pair=False, out_pair=False), {}, R("x3", 0)),
    (dict(n=32, cin=16), dict(x_pair=False, out_pair=False, tile=60), {}, R("x3", 60)),
    (S1, dict(x_pair=False, out_pair=False, res="fp32"), {}, R("x3", 0)),
    (S1, dict(x_pair=False, out_pair=False, occ=True, tile=81), {}, R("x3", 81)),
    # pair in, pair out, 3x3 s1
    (S1, PP, {}, R("wino", 1)),
    (S1, PP, dict(WINO=False), R("hx3", 0)),
    (S1, PP, dict(WINO=False, HX3=False), R("x3p", 0)),
    (S1N, PP, {}, R("hx3", 0)),
    (S1N, PP, dict(WINO_MIN_N=64), R("wino", 3)),
    (S1N, PP, dict(WINO_MIN_N=64, WINO_TILE_AUTO=4), R("wino", 4)),
    (S1, dict(PP, res="pair"), {}, R("hx3", 0)),
    (S1, dict(PP, res="pair", tile=130), {}, R("x3p", 0)),
    (S1, dict(PP, res="pair"), dict(HX3=False), R("x3p", 0)),
    (S1, dict(PP, occ=True), {}, R("x3p_occ", 0, gated=True)),
    (S1, dict(PP, occ=True, tile=130), {}, R("x3p_occ", 0, gated=True)),
    (S1, dict(PP, occ=True, tile=110), {}, R("x3p_occ", 0, gated=True)),
    (S1, dict(PP, uni=True), {}, R("wino", 1)),
    (S1, dict(PP, uni=True), dict(WINO=False), R("hx3_uni", 0)),
    (S1, dict(PP, uni=True, res="pair"), {}, R("hx3", 0)),
    (S1, dict(PP, uni=True), dict(WINO=False, HX3_TILE_AUTO=5), R("hx3_uni", 5)),
    (dict(n=128, act=ACT_SILU), PP, {}, R("hx3", 0)),  # F(2,3): ReLU or no activation only
    # the F(2,3) kernel reads and writes either storage; hx3 writes pairs only
    (S1, dict(x_pair=True, out_pair=False), {}, R("wino", 1, out_fp32=True)),
    (S1, dict(x_pair=False, out_pair=True), {}, R("wino", 1)),
    (S1, dict(x_pair=False, out_pair=False), {}, R("wino", 1, out_fp32=True)),
    (S1, dict(x_pair=False, out_pair=False), dict(WINO=False), R("x3", 0)),
    (S1, dict(x_pair=True, out_pair=False), dict(WINO=False), R("x3p", 0)),
    (S1, dict(x_pair=True, out_pair=False, tile=110), {}, R("x3p", 0)),
    # 3x3 s2, pair in
    (S2, PP, {}, R("hx3s2", 0)),
    (S2, dict(x_pair=True, out_pair=False), {}, R("hx3s2", 0, out_fp32=True)),
    (S2, dict(PP, occ=True), {}, R("hx3s2", 0, gated=True)),
    (S2, dict(PP, occ=True), dict(S2SP=True), R("s2sp", 0, gated=True)),
    (S2, dict(PP, occ=True), dict(S2SP=True, S2SP_TILE=2), R("s2sp", 2, gated=True)),
    (S2, dict(x_pair=True, out_pair=False, occ=True), dict(S2SP=True), R("s2sp", 0, out_fp32=True, gated=True)),
    (S2, PP, dict(S2SP=True), R("hx3s2", 0)),  # s2sp only over an occupancy-marked canvas
    (S2, dict(PP, occ=True, res="pair"), dict(S2SP=True), R("hx3s2", 0, gated=True)),  # nor with a residual
    (S2, dict(PP, res="pair"), {}, R("hx3s2", 0)),
    (S2, dict(x_pair=True, out_pair=False, res="fp32"), {}, R("x3p", 0)),  # hx3s2: fp32 out only without residual
    (S2, PP, dict(HX3S2=False), R("x3p", 0)),
    (S2, dict(PP, occ=True), dict(HX3S2=False), R("x3p_occ", 0, gated=True)),
    (S2, PP, dict(HX3S2_TILE_AUTO=3), R("hx3s2", 3)),
    (dict(n=128, s=2), dict(PP, occ=True, tile=140), {}, R("x3p_occ", 0, gated=True)),  # s2sp: N == 64 only
    # an explicit tile of a family the layer cannot take falls through
    (S2, dict(PP, tile=130), {}, R("x3p", 0)),
    (S2, dict(PP, tile=110), {}, R("x3p", 0)),
    (S1, dict(PP, tile=120), {}, R("x3p", 0)),
    (S2, dict(PP, tile=140), {}, R("x3p", 0)),  # no occupancy
    (dict(n=128, k=1), dict(PP, tile=111), {}, R("x3p", 0)),
    (dict(n=128, k=1), dict(PP, occ=True), {}, R("x3p_occ", 0, gated=True)),
    (dict(cin=8, n=64, k=7), dict(PP, occ=True), {}, R("x3p_occ", 0)),  # 49 taps: the launcher drops occ
    # a transpose conv (k = s = 2) over pairs
    (dict(n=128, s=2, transpose=True), PP, {}, R("x3p", 0)),
    (dict(n=128, s=2, transpose=True), dict(PP, occ=True, tile=41), {}, R("x3p", 41)),
    (dict(n=128, s=2, transpose=True), dict(x_pair=False, out_pair=False), {}, R("x3", 0)),
]
# every explicit public tile -> the launcher's own number, on a layer its family takes
ROUTES += [(S1, dict(PP, tile=110 + t), {}, R("hx3", t)) for t in range(7)]
ROUTES += [(S2, dict(PP, tile=120 + t), {}, R("hx3s2", t)) for t in range(5)]
ROUTES += [(S1, dict(PP, tile=130 + t), dict(WINO=False), R("wino", t or 1)) for t in range(5)]
ROUTES += [(S2, dict(PP, occ=True, tile=140 + t), {}, R("s2sp", t, gated=True)) for t in range(3)]
ROUTES += [(S1, dict(PP, tile=t), {}, R("x3p", t)) for t in PAIR_TILES]
ROUTES += [(S1, dict(PP, tile=t), {}, R("x3p", 0)) for t in (5, 60, 81, 98, 117, 125, 135, 143)]  # no pair tiles


def _id(case):
    lay, args, sw, exp = case
    return "-".join(f"{k}={v}" for d in (lay, args, sw) for k, v in d.items()) or "default"


@pytest.mark.parametrize("case", ROUTES, ids=_id)
def test_route_table(case, monkeypatch):
    lay, args, sw, exp = case
    for k, v in sw.items():
        monkeypatch.setattr(conv_mod, k, v)
    assert layer(**lay).route(**args, H=H, W=W) == exp


def test_route_wino_tile_orientation():
    """As tests/test_wino_gpu.py test_wino_tile_orientation, through route."""
    for (h, w, n), t in {(248, 216, 128): 2, (124, 108, 128): 2, (62, 54, 256): 2, (20, 64, 128): 1,
                         (20, 64, 192): 3, (248, 216, 192): 4}.items():
        assert layer(n=n).route(True, True, H=h, W=w).tile == t
        assert layer(n=n).route(True, True, tile=130, H=h, W=w).tile == t


def test_route_reads_switches_at_call(monkeypatch):
    fc = layer(**S1)
    assert fc.route(True, True, H=H, W=W).family == "wino"
    monkeypatch.setattr(conv_mod, "WINO", False)
    assert fc.route(True, True, H=H, W=W).family == "hx3"


@pytest.mark.parametrize("lay,args", [
    (S1, dict(x_pair=False, out_pair=True, occ=True)),  # pairs out of plain fp32 (the F(2,3) kernel aside)
    (S2, dict(x_pair=False, out_pair=True)),
    (dict(n=128, k=1), dict(x_pair=False, out_pair=True)),
    (S1, dict(x_pair=True, out_pair=True, res="fp32")),  # residual storage != output storage
    (S1, dict(x_pair=True, out_pair=False, res="pair")),
    (dict(precision="bf16"), dict(x_pair=True, out_pair=True)),  # bf16 convs take no pairs
    (dict(precision="bf16"), dict(x_pair=True, out_pair=False)),
])
def test_route_refuses_storage(lay, args):
    with pytest.raises(TypeError):
        layer(**lay).route(**args, H=H, W=W)


# ---- __call__ end to end: stand-in tensors, recorded native calls


class _T:
    """What __call__ reads of a tensor on its way to the launch."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype, self.device = tuple(shape), dtype, SimpleNamespace(type="cuda")

    def numel(self):
        return int(torch.Size(self.shape).numel())


_PTR = object()


@pytest.fixture
def calls(monkeypatch):
    rec = []
    monkeypatch.setattr(_native, "call", lambda name, *a: rec.append((name, tuple(v for v in a if v is not _PTR))))
    monkeypatch.setattr(_native, "ptr", lambda t: _PTR)
    monkeypatch.setattr(_native, "stream_ptr", lambda s=None: _PTR)
    return rec


def run(fc, x_pair, out_pair, res=None, occ=False, uni=False, tile=0, B=2):
    Ho, Wo = fc.out_hw(H, W)
    dt = fc.dtype
    x = NHWC(_T((B, H, W, fc.cin_p + 8), dt), 8, fc.cin_p, pair=x_pair, occ=_T((B, H, W), torch.uint8) if occ else None)
    out = NHWC(_T((B, Ho, Wo, fc.out_channels() + 16), dt), 16, fc.out_channels(), pair=out_pair)
    r = None if res is None else NHWC(_T((B, Ho, Wo, fc.out_channels() + 24), dt), 24, fc.out_channels(), pair=res == "pair")
    u = (_T((B, Ho, Wo), torch.uint8), 3, _T((fc.N,), torch.float32)) if uni else None
    assert fc(x, out=out, res=r, tile=tile, uni=u) is out


# B, H, W, Cin, ldi, ci_off lead every entry; the rest per entry, pointers left out:
#   tca_conv_nhwc / _x3:  N, KH, KW, S, P, Kp, gh, gw, ldo, co_off, act, ldr, r_off, shuffle, tile
#   _x3p (_occ):          the same, then out_pair
#   tca_conv_hx3p:        N, ldo, co_off, act, ldr, r_off, tile      _uni: N, ldo, co_off, act, uni_min, tile
#   tca_conv_hx3s2p:      N, ldo, co_off, act (| 32: fp32 out), ldr, r_off, uni_min, tile
#   tca_conv_wino:        x_pair, N, ldo, co_off, out_pair, act, uni_min, tile
#   tca_conv_s2sp:        N, ldo, co_off, act (| 32), tile
IN = (2, 20, 64, 64, 72, 8)
CALLS = [
    (dict(precision="bf16"), dict(x_pair=False, out_pair=False, tile=2), {},
     ("tca_conv_nhwc", IN + (128, 3, 3, 1, 1, 576, 20, 64, 144, 16, 1, 0, 0, 0, 2))),
    (dict(n=32, cin=64, act=ACT_SILU), dict(x_pair=False, out_pair=False, res="fp32"), {},
     ("tca_conv_nhwc_x3", IN + (32, 3, 3, 1, 1, 576, 20, 64, 48, 16, 2, 56, 24, 0, 0))),
    (dict(n=128, s=2, transpose=True), dict(PP, occ=True, tile=41), {},
     ("tca_conv_nhwc_x3p", IN + (512, 1, 1, 1, 0, 64, 20, 64, 144, 16, 1, 0, 0, 2, 41, 1))),
    (S1, dict(x_pair=True, out_pair=False, tile=110), {},
     ("tca_conv_nhwc_x3p", IN + (128, 3, 3, 1, 1, 576, 20, 64, 144, 16, 1, 0, 0, 0, 0, 0))),
    (S1, dict(PP, occ=True, res="pair", tile=97), {},
     ("tca_conv_nhwc_x3p_occ", IN + (128, 3, 3, 1, 1, 576, 20, 64, 144, 16, 1, 152, 24, 0, 97, 1))),
    (S1N, dict(PP, res="pair"), dict(HX3_TILE_AUTO=4), ("tca_conv_hx3p", IN + (64, 80, 16, 1, 88, 24, 4))),
    (S1N, dict(PP, tile=116), dict(HX3_TILE_AUTO=4), ("tca_conv_hx3p", IN + (64, 80, 16, 1, 0, 0, 6))),
    (S1N, dict(PP, uni=True), {}, ("tca_conv_hx3p_uni", IN + (64, 80, 16, 1, 3, 0))),
    (S2, dict(x_pair=True, out_pair=False, occ=True, uni=True, tile=122), {},
     ("tca_conv_hx3s2p", IN + (64, 80, 16, 1 | 32, 0, 0, 3, 2))),
    (S2, dict(PP, res="pair", uni=True), {}, ("tca_conv_hx3s2p", IN + (64, 80, 16, 1, 88, 24, 0, 0))),
    (S1, dict(x_pair=True, out_pair=False, uni=True), {}, ("tca_conv_wino", IN + (1, 128, 144, 16, 0, 1, 3, 1))),
    (S1, dict(x_pair=False, out_pair=True, tile=134), dict(WINO=False),
     ("tca_conv_wino", IN + (0, 128, 144, 16, 1, 1, 0, 4))),
    (S2, dict(x_pair=True, out_pair=False, occ=True, tile=141), {}, ("tca_conv_s2sp", IN + (64, 80, 16, 1 | 32, 1))),
    (S2, dict(PP, occ=True), dict(S2SP=True, S2SP_TILE=2), ("tca_conv_s2sp", IN + (64, 80, 16, 1, 2))),
]


@pytest.mark.parametrize("case", CALLS, ids=_id)
def test_call_launches_what_route_decided(case, calls, monkeypatch):
    lay, args, sw, exp = case
    for k, v in sw.items():
        monkeypatch.setattr(conv_mod, k, v)
    run(layer(**lay), **args)
    assert calls == [exp]


def test_call_post_res_flag(calls):
    """act | 16 (activation after the residual) only with a residual."""
    fc = FusedConv(nn.Conv2d(64, 64, 3, 1, 1), act=ACT_RELU, device="cpu", precision="fp32", post_res=True)
    run(fc, True, True, res="pair")
    run(fc, True, True)
    assert [(n, a[9]) for n, a in calls] == [("tca_conv_hx3p", 1 | 16), ("tca_conv_hx3p", 1)]


def test_call_refusals(calls):
    with pytest.raises(TypeError):
        run(layer(**S2), False, True)
    with pytest.raises(TypeError):
        run(layer(**S1), True, True, res="fp32")
    with pytest.raises(TypeError):  # fp32 tensors into a bf16 conv: the dtype check, before any routing
        x = NHWC(_T((1, H, W, 64), torch.float32))
        layer(precision="bf16")(x, out=NHWC(_T((1, H, W, 128), torch.float32)))
    assert calls == []


# ---- the plans' questions on the PointPillars backbone (64 -> 64 s2 + 3, 64 -> 128 s2 + 5, 128 -> 256 s2 + 5)


def pp_blocks():
    spec = [(64, 64, 3), (64, 128, 5), (128, 256, 5)]
    return [[layer(cin, n, s=2)] + [layer(n, n)] * m for cin, n, m in spec]


def out_pairs():
    return [[fast.bev_out_pair(convs, i) for i in range(len(convs))] for convs in pp_blocks()]


ALL_PAIRS = [[True] * 4, [True] * 6, [True] * 6]


def test_plan_out_pair_pattern(monkeypatch):
    # block 1 (N = 64: hx3) all pairs; blocks 2 and 3 fp32 between the convs, pairs at the block's end
    assert out_pairs() == [[True] * 4, [False] * 5 + [True], [False] * 5 + [True]]
    monkeypatch.setattr(conv_mod, "WINO_MIN_N", 64)
    assert out_pairs() == [[False] * 3 + [True], [False] * 5 + [True], [False] * 5 + [True]]
    monkeypatch.setattr(conv_mod, "HX3S2", False)  # the stride-2 conv falls to x3p: pairs in front of F(2,3)
    assert out_pairs() == [[True] + [False] * 2 + [True], [True] + [False] * 4 + [True], [True] + [False] * 4 + [True]]


def test_plan_out_pair_all_pairs_without_wino(monkeypatch):
    monkeypatch.setattr(conv_mod, "WINO", False)
    assert out_pairs() == ALL_PAIRS


def test_plan_out_pair_all_pairs_without_f32_chain(monkeypatch):
    monkeypatch.setattr(fast, "WINO_F32_CHAIN", False)
    assert out_pairs() == ALL_PAIRS


def test_plan_first_conv_gated(monkeypatch):
    first = pp_blocks()[0][0]
    assert fast.bev_first_conv_gated(first) is True
    monkeypatch.setattr(conv_mod, "S2SP", True)
    assert fast.bev_first_conv_gated(first) is True
    monkeypatch.setattr(conv_mod, "HX3S2", False)
    monkeypatch.setattr(conv_mod, "S2SP", False)
    assert fast.bev_first_conv_gated(first) is True  # x3p_occ
    assert fast.bev_first_conv_gated(layer(64, 64, k=1)) is True
    assert fast.bev_first_conv_gated(layer(8, 64, k=7)) is False  # 49 taps
    assert fast.bev_first_conv_gated(layer(64, 64, s=2, transpose=True)) is False


def test_plan_uniform_eligible(monkeypatch):
    blocks = pp_blocks()
    assert [fast.bev_uniform_eligible(b) for b in blocks] == [True, True, True]
    assert fast.bev_uniform_eligible(blocks[0][:1]) is False  # needs a stride-1 conv behind the stride-2 one
    assert fast.bev_uniform_eligible(blocks[0][1:]) is False  # starts at stride 1
    assert fast.bev_uniform_eligible([blocks[0][0]] + blocks[0][1:] * 3) is False  # more than 8 convs
    assert fast.bev_uniform_eligible([blocks[0][0], layer(64, 64, k=1)]) is False
    monkeypatch.setattr(conv_mod, "WINO", False)
    monkeypatch.setattr(conv_mod, "S2SP", True)
    assert [fast.bev_uniform_eligible(b) for b in blocks] == [True, True, True]
