"""K37: inflation of the occupancy grid — the options, the cost table, the definition against the brute force, the
driver and the CLI."""
import dataclasses

import numpy as np
import pytest

from test_ground import OPTS as GROUND
from test_occupancy_grid import RIG
from test_range2d import _Engine, _rig_messages
from triton_client_amd.ops import occupancy_grid as O
from triton_client_amd.ros import rosmsg

KNOWN = dict(cell=0.2, inflation_radius=0.55, inscribed_radius=0.3, cost_scaling=10.0)
KNOWN_TABLE = [100, 99, 99, 61, 36, 22, 14, 10, 7, 5]


def opts_of(W, H, Rc, **kw):
    """A ``W x H`` grid of 1 m cells that inflates by ``Rc`` cells, costs falling slowly enough to reach the rim."""
    o = O.GridOptions(cell=1.0, x_range=(0, W), y_range=(0, H), inflation_radius=float(Rc),
                      inscribed_radius=min(1.2, Rc), cost_scaling=2.0 / Rc, **kw)
    assert (o.W, o.H, o.inflation_cells) == (W, H, Rc)
    return o


def random_plane(W, H, seed=0):
    u = np.random.default_rng(seed).random(W * H)
    return np.where(u < 0.02, 100, np.where(u < 0.35, -1, 0)).astype(np.int8)


def test_options():
    o = O.GridOptions()  # unchanged
    assert not o.inflation and (o.inflation_radius, o.inscribed_radius, o.cost_scaling, o.inflate_unknown) == (0, 0, 10, False)
    assert O.GridOptions(**KNOWN).inflation_cells == 3 and O.GridOptions(**KNOWN).inflation
    assert O.GridOptions(cell=0.2, inflation_radius=0.6).inflation_cells == 4  # float32(0.6) is above 3 * float32(0.2)
    assert O.GridOptions(cell=0.25, x_range=(-8, 8), y_range=(-8, 8), inflation_radius=16.0).inflation_cells == 64


@pytest.mark.parametrize("kw,word", [
    (dict(cell=0.25, inflation_radius=16.1), "inflation_radius gives 65 cells"), (dict(inflation_radius=-1.0), "inflation_radius"),
    (dict(inflation_radius=float("nan")), "inflation_radius"), (dict(inflation_radius=0.5, inscribed_radius=0.6), "inscribed_radius"),
    (dict(inscribed_radius=0.1), "inscribed_radius needs inflation_radius"), (dict(cost_scaling=5.0), "cost_scaling needs inflation_radius"),
    (dict(inflate_unknown=True), "inflate_unknown needs inflation_radius"), (dict(inflation_radius=1.0, cost_scaling=101.0), "cost_scaling"),
    (dict(inflation_radius=1.0, cost_scaling=float("inf")), "cost_scaling"), (dict(inflation_radius=1.0, inflate_unknown=1), "inflate_unknown")])
def test_options_refuse(kw, word):
    with pytest.raises(ValueError, match=word):
        O.GridOptions(**kw)


def test_cost_table_known_answers():
    assert O.cost_table(O.GridOptions(**KNOWN)).tolist() == KNOWN_TABLE
    fine = O.GridOptions(cell=0.05, x_range=(-5, 5), y_range=(-5, 5), inflation_radius=0.55)
    assert fine.inflation_cells == 12 and O.cost_table(fine)[:8].tolist() == [100, 59, 48, 41, 36, 32, 29, 26]
    wide = O.GridOptions(cell=0.2, inflation_radius=12.8, inscribed_radius=0.5, cost_scaling=1.0)
    t = O.cost_table(wide)
    assert wide.inflation_cells == 64 and t.dtype == np.int8 and len(t) == 4097 and (np.diff(t.astype(int)) <= 0).all()


PLANES = {"empty": lambda W, H: np.where(np.arange(W * H) % 3 == 0, -1, 0).astype(np.int8),
          "full": lambda W, H: np.full(W * H, 100, np.int8), "random": random_plane,
          "corner": lambda W, H: np.where(np.arange(W * H) == 0, 100, np.where(np.arange(W * H) % 2, -1, 0)).astype(np.int8)}


@pytest.mark.parametrize("unknown", [False, True])
@pytest.mark.parametrize("Rc", [1, 3, 12])
@pytest.mark.parametrize("plane", sorted(PLANES))
def test_definition_equals_the_brute_force(plane, Rc, unknown):
    o = opts_of(67, 35, Rc, inflate_unknown=unknown)
    p = PLANES[plane](67, 35)
    got = O.inflate_numpy(p, o)
    assert got.dtype == np.int8 and got.shape == p.shape
    np.testing.assert_array_equal(got, O.inflate_ref(p, o))
    if plane in ("empty", "full"):
        np.testing.assert_array_equal(got, p)


def test_one_obstacle_gives_the_table_by_squared_distance():
    o = O.GridOptions(x_range=(0, 1.8), y_range=(0, 1.8), **KNOWN)
    p = np.zeros(81, np.int8)
    p[4 * 9 + 4] = 100
    yy, xx = np.mgrid[0:9, 0:9]
    d2 = ((yy - 4) ** 2 + (xx - 4) ** 2).reshape(-1)
    want = np.where(d2 <= 9, np.array(KNOWN_TABLE + [0] * 30)[d2], 0)
    np.testing.assert_array_equal(O.inflate_numpy(p, o), want)


def test_driver_makes_the_inflated_grid_and_the_same_bytes_with_it_off():
    from triton_client_amd.inference import RosInference3D

    clouds, _ = _rig_messages()
    on = dataclasses.replace(RIG, inflation_radius=1.2, inscribed_radius=0.5, cost_scaling=2.0)

    def drive(grid_options):
        drv = RosInference3D(engine=_Engine(), params={}, grid_topic="/grid", grid_options=grid_options, grid_frame_id="map",
                             ground_options=GROUND)
        return [r.grid for r in drv.process(clouds)]

    plain = [O.grid_cloud_numpy(c, RIG, GROUND) for c in clouds]
    want = [O.grid_message(c, O.inflate_numpy(p, on), on, "map") for c, p in zip(clouds, plain)]
    assert drive(dataclasses.asdict(on)) == want and all(((w.data > 0) & (w.data < 99)).sum() > 20 for w in want)
    old = {f.name: getattr(RIG, f.name) for f in dataclasses.fields(RIG)[:6]}  # the fields before this feature
    assert [rosmsg.serialize(m) for m in drive(RIG)] == [rosmsg.serialize(m) for m in drive(old)] == \
        [rosmsg.serialize(O.grid_message(c, p, RIG, "map")) for c, p in zip(clouds, plain)]


def test_flags_and_usage_errors(capsys):
    from triton_client_amd.cli import bag3d, main3d

    for mod, pre in ((main3d, []), (bag3d, ["--bag", "x"])):
        f = mod.parse_args(pre + ["--grid-topic", "/g", "--grid-inflation-radius", "0.55", "--grid-inscribed-radius", "0.3",
                                  "--grid-cost-scaling", "5", "--grid-inflate-unknown"])
        assert f.grid_options == O.GridOptions(inflation_radius=0.55, inscribed_radius=0.3, cost_scaling=5.0,
                                               inflate_unknown=True)
        assert mod.parse_args(pre + ["--grid-topic", "/g"]).grid_options == O.GridOptions()
        for bad, word in ((["--grid-inflation-radius", "1"], "--grid-inflation-radius needs --grid-topic TOPIC"),
                          (["--grid-inflate-unknown"], "--grid-inflate-unknown needs --grid-topic TOPIC"),
                          (["--grid-topic", "/g", "--grid-inflation-radius", "13"], "error: --grid-inflation-radius: "),
                          (["--grid-topic", "/g", "--grid-inflation-radius", "1", "--grid-inscribed-radius", "2"],
                           "error: --grid-inscribed-radius: "),
                          (["--grid-topic", "/g", "--grid-cost-scaling", "3"], "error: --grid-cost-scaling: "),
                          (["--grid-topic", "/g", "--grid-inflate-unknown"], "error: --grid-inflate-unknown: ")):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(pre + bad)
            assert e.value.code == 2 and word in capsys.readouterr().err, bad
