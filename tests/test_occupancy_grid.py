"""K33: the ray-cast occupancy grid — the definition against a float64 brute force, hand-made facts, the options,
the two nav_msgs types, the drivers and the CLI."""
import dataclasses

import numpy as np
import pytest

from test_ground import OPTS as GROUND
from test_range2d import _Engine, _rig_messages
from triton_client_amd.ops import ground as G
from triton_client_amd.ops import occupancy_grid as O
from triton_client_amd.ros import compat, msgs, rosmsg

F = np.float32
OPTS = O.GridOptions(cell=0.25, x_range=(-8, 8), y_range=(-6, 6), sectors=90)  # 64 x 48 cells
RIG = O.GridOptions(cell=0.5, x_range=(-5, 20), y_range=(-10, 10), sectors=180, clear_radius=1.0)


def scene(seed):
    """A ground plane at z = -1.8 with 2 cm of noise and no return between 100 and 140 degrees, two walls, a box
    near the sensor and a low obstacle with the plane's returns beyond it, in a seeded order."""
    rng = np.random.default_rng(seed)
    g = np.stack([rng.uniform(-8, 8, 1200), rng.uniform(-6, 6, 1200), -1.8 + rng.normal(0, 0.02, 1200)], 1)
    a = np.degrees(np.arctan2(g[:, 1], g[:, 0]))

    def slab(x, y, z, n):
        return np.stack([rng.uniform(*x, n), rng.uniform(*y, n), rng.uniform(*z, n)], 1)

    pts = np.concatenate([g[~((a > 100) & (a < 140))], slab((4.8, 5.6), (-4, 4), (-1.6, 0.5), 900),
                          slab((-6, 3), (-5.0, -4.3), (-1.6, 0.5), 900), slab((1, 2.2), (1, 2.2), (-1.5, -0.5), 400),
                          slab((-3.5, -3.0), (-0.6, 0.6), (-1.5, -1.3), 150)]).astype(F)
    return pts[rng.permutation(len(pts))]


@pytest.fixture(scope="module")
def scenes():
    """Per seed the split rows, the definition's grid and the reference's grid and band: made once."""
    out = []
    for seed in range(4):
        obs, gnd = O.split_rows(scene(seed))
        out.append((obs, gnd, O.grid_numpy(obs, gnd, OPTS), *O.grid_ref(obs, gnd, OPTS)))
    return out


def at(x, y, o=OPTS):  # the cell index of the point (x, y)
    return int((y - o.y_range[0]) / o.cell) * o.W + int((x - o.x_range[0]) / o.cell)


# ------------------------------------------------------------------------------ options
@pytest.mark.parametrize("kw,word", [
    (dict(cell=0.01), "cell"), (dict(cell=float("nan")), "cell"), (dict(cell=True), "cell"),
    (dict(x_range=(5, 5)), "x_range"), (dict(x_range=(-600, 0)), "x_range"), (dict(y_range=(0, 1, 2)), "y_range"),
    (dict(cell=0.05, x_range=(-60, 60)), "x_range"), (dict(cell=0.05, y_range=(-60, 60)), "y_range"),
    (dict(sectors=0), "sectors"), (dict(sectors=4097), "sectors"), (dict(sectors=90.0), "sectors"),
    (dict(min_points=0), "min_points"), (dict(clear_radius=-1.0), "clear_radius"),
    (dict(clear_radius=float("inf")), "clear_radius")])
def test_options_refuse(kw, word):
    with pytest.raises(ValueError, match=word):
        O.GridOptions(**kw)


# ------------------------------------------------------------ definition against float64
def test_definition_equals_the_reference_outside_the_band(scenes):
    for obs, gnd, grid, ref, band in scenes:
        assert grid.dtype == ref.dtype == np.int8 and grid.shape == ref.shape == band.shape == (64 * 48,)
        assert band.mean() <= 0.01  # a condition on the reference: the band may leave out at most 1 % of the cells
        np.testing.assert_array_equal(grid[~band], ref[~band])
        for value in (O.OCCUPIED, O.FREE, O.UNKNOWN):
            assert (grid == value).mean() > 0.05, value
        # ground rows too high to have a cell still cast their rays: what differs is free only through gseen
        lifted = gnd.copy()
        lifted[:, 2] = 600.0
        shadowed = (grid == O.FREE) & (O.grid_numpy(obs, lifted, OPTS) == O.UNKNOWN)
        assert shadowed.sum() >= 1
        order = np.random.default_rng(9).permutation(len(obs))
        np.testing.assert_array_equal(O.grid_numpy(obs[order], gnd[::-1], OPTS), grid)  # no order matters


def test_hand_made_facts():
    assert (O.GridOptions().W, O.GridOptions().H, O.GridOptions().stride, OPTS.W, OPTS.H) == (400, 400, 160000, 64, 48)
    assert O.GridOptions(cell=1.0, x_range=(0, 5), y_range=(0, 3)).stride == 16  # planes start 16-byte aligned
    assert O.most_clouds(O.GridOptions(cell=0.05), G.GroundOptions()) == 6 and len(G.edge_table(OPTS)) == 91
    one = np.array([[5.1, 0.1, 0.0]], F)
    none = np.zeros((0, 3), F)
    g = O.grid_numpy(one, none, OPTS)
    ahead = [at(x, 0.1) for x in np.arange(2.05, 8, 0.25)]  # the obstacle's row of cells where its 4-degree sector holds them
    hit = ahead.index(at(5.1, 0.1))
    assert g[at(5.1, 0.1)] == O.OCCUPIED and (g == O.OCCUPIED).sum() == 1
    assert (g[ahead[:hit]] == O.FREE).all() and (g[ahead[hit + 1:]] == O.UNKNOWN).all()
    assert g[at(-5.1, 0.1)] == O.UNKNOWN and g[at(0.1, 3.1)] == O.UNKNOWN  # other directions have no return
    assert (g == O.FREE).sum() < 64  # one sector of 4 degrees
    near = dataclasses.replace(OPTS, clear_radius=1.0)
    cleared = O.grid_numpy(one, none, near)
    assert cleared[at(-0.6, 0.1)] == cleared[at(0.1, -0.6)] == O.FREE and cleared[at(-1.1, 0.1)] == O.UNKNOWN
    two = dataclasses.replace(OPTS, min_points=2)
    assert O.grid_numpy(one, none, two)[at(5.1, 0.1)] == O.UNKNOWN  # its own ray ends at its r, short of the centre ...
    assert O.grid_numpy(np.array([[5.24, 0.1, 0.0]], F), none, two)[at(5.24, 0.1)] == O.FREE  # ... or past it
    assert O.grid_numpy(np.repeat(one, 2, 0), none, two)[at(5.1, 0.1)] == O.OCCUPIED
    gnd = np.array([[7.1, 0.1, -1.8], [-3.1, 2.1, -1.8]], F)
    g = O.grid_numpy(one, gnd, OPTS)
    assert g[at(7.1, 0.1)] == O.FREE and g[at(6.6, 0.1)] == O.UNKNOWN  # free behind the obstacle only where seen
    assert g[at(-1.6, 1.1)] == O.FREE  # a ground return alone frees its ray
    odd = np.array([[np.nan, 1, 0], [0, 0, 0], [1e30, 1e30, 0], [600, 0.1, 0], [3.1, 0.1, 600]], F)
    g = O.grid_numpy(odd, none, OPTS)  # NaN, r = inf: nothing; the sensor itself: a cell, no ray; outside or too high: a ray
    assert g[at(0, 0)] == O.OCCUPIED and (g == O.OCCUPIED).sum() == 1
    assert g[at(2.6, 0.1)] == O.FREE and g[at(3.4, 0.1)] == O.UNKNOWN


# ---------------------------------------------------------------------------- messages
def test_message_types_and_the_grid_message():
    assert rosmsg.md5sum("nav_msgs/OccupancyGrid") == "3381f2d731d4076ec5c71b0759edbe4e"
    assert rosmsg.md5sum("nav_msgs/MapMetaData") == "10cfc8a2818024d3248802c00c95f11b"
    cloud = _rig_messages()[0][0]
    data = O.grid_cloud_numpy(cloud, RIG, GROUND)
    m = O.grid_message(cloud, data, RIG, "map")
    h = cloud.header
    assert m.header == msgs.Header(seq=h.seq, stamp=h.stamp, frame_id="map")
    assert O.grid_message(cloud, data, RIG).header.frame_id == h.frame_id
    assert m.info == msgs.MapMetaData(h.stamp, 0.5, 50, 40, msgs.Pose(msgs.Point(-5.0, -10.0, 0.0), msgs.Quaternion(0, 0, 0, 1)))
    assert m.data.dtype == np.int8 and m.data.tobytes() == data.tobytes()
    wire = rosmsg.serialize(m)
    assert wire[-2000:] == data.tobytes() and rosmsg.deserialize(wire, "nav_msgs/OccupancyGrid") == m
    info = rosmsg.serialize(m.info)
    assert len(info) == 8 + 4 + 4 + 4 + 56 and rosmsg.deserialize(info, "nav_msgs/MapMetaData") == m.info
    with pytest.raises(ValueError, match="cells"):
        O.grid_message(cloud, data[:-1], RIG)


# ----------------------------------------------------------------------------- drivers
def _wanted(clouds):
    return [O.grid_message(c, O.grid_cloud_numpy(c, RIG, GROUND), RIG, "map") for c in clouds]


def test_driver_publishes_the_grid_last_and_keeps_every_other_byte(monkeypatch):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.inference import ros_inference3d as M
    from triton_client_amd.ros.bus import TopicBus

    assert M.MAP_OUTPUTS == (("grid", msgs.OccupancyGrid),) and M.EVERY_OUTPUT == M.PUBLISHED + M.MAP_OUTPUTS
    clouds, _ = _rig_messages()
    want = _wanted(clouds)
    assert all((w.data == v).sum() > 20 for w in want for v in (100, 0, -1))  # the rig's grids hold all three values

    def drive(grid):
        bus, seen, order = TopicBus(), {"/o": [], "/clusters": [], "/gnd": []}, []
        for t, ty in (("/o", msgs.BoundingBoxArray), ("/clusters", msgs.BoundingBoxArray), ("/gnd", msgs.PointCloud2)):
            compat.Subscriber(t, ty, lambda m, t=t: seen[t].append(rosmsg.serialize(m)), bus=bus)
        got = []
        compat.Subscriber("/grid", msgs.OccupancyGrid, got.append, bus=bus)
        kw = dict(grid_topic="/grid", grid_options=dataclasses.asdict(RIG), grid_frame_id="map") if grid else {}
        drv = RosInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=4,
                             workers=2, queue_size=64, ground_topic="/gnd", ground_options=GROUND,
                             clusters_topic="/clusters", **kw)
        drv.start_inference(spin=False)
        for name, p in drv.side_pubs.items():
            monkeypatch.setattr(p, "publish", lambda m, name=name, send=p.publish: (order.append(name), send(m)))
        pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
        for c in clouds:
            pub.publish(c)
        runner = drv.runner
        drv.stop()
        bus.close()
        assert not runner.errors, runner.errors
        return seen, got, order, drv

    seen, got, order, drv = drive(True)
    assert got == want and drv.grid_options == RIG
    assert order == ["ground", "clusters", "grid"] * 4  # last of every cloud's messages
    off_seen, off_got, _, _ = drive(False)
    assert off_got == [] and off_seen == seen  # with the option off, and on, every other message keeps its bytes
    assert all(r.grid is None and "grid" not in r.pred for r in RosInference3D(engine=_Engine(), params={}).process(clouds))
    alone = RosInference3D(engine=_Engine(), params={}, grid_topic="/g")  # the defaults of both option sets
    assert (alone.grid_options, alone.ground_options) == (O.GridOptions(), G.GroundOptions())
    with pytest.raises(ValueError, match="sectors"):
        RosInference3D(engine=_Engine(), params={}, grid_topic="/g", grid_options={"sectors": 0})


def test_bag_driver_writes_the_grids(tmp_path):
    from triton_client_amd.inference import BagInference3D
    from triton_client_amd.ros.bag import Bag

    clouds, _ = _rig_messages()
    src, dst = str(tmp_path / "in.bag"), str(tmp_path / "out.bag")
    with Bag(src, "w") as bag:
        for c in clouds:
            bag.write("/pc", c)
    drv = BagInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bagfile=src, out_bag=dst,
                         batch=3, grid_topic="/grid", grid_options=RIG, grid_frame_id="map", ground_options=GROUND)
    assert drv.start_inference() == 4
    with Bag(dst) as bag:
        topics = [t for t, _, _ in bag.read_messages()]
        got = [m for _, m, _ in bag.read_messages(topics=["/grid"])]
    assert topics == ["/pc", "/o", "/grid"] * 4 and got == _wanted(clouds)


def test_flags_and_usage_errors(capsys):
    from triton_client_amd.cli import bag3d, main3d

    for mod, pre in ((main3d, []), (bag3d, ["--bag", "x"])):
        f = mod.parse_args(pre)
        assert f.grid_topic == "" and f.grid_options is None and f.ground_options is None
        f = mod.parse_args(pre + ["--grid-topic", "/g", "--ground-sensor-height", "2.1"])  # legal with this topic alone
        assert f.grid_options == O.GridOptions() and f.ground_options == G.GroundOptions(sensor_height=2.1)
        f = mod.parse_args(pre + ["--grid-topic", "/g", "--grid-cell", "0.25", "--grid-x-range=-8,8", "--grid-y-range=-6,6",
                                  "--grid-sectors", "90", "--grid-min-points", "2", "--grid-clear-radius", "1.5",
                                  "--grid-frame-id", "map"])
        assert f.grid_options == dataclasses.replace(OPTS, min_points=2, clear_radius=1.5) and f.grid_frame_id == "map"
        for bad, word in ((["--grid-cell", "1"], "--grid-cell needs --grid-topic TOPIC"),
                          (["--grid-frame-id", "map"], "--grid-frame-id needs --grid-topic TOPIC"),
                          (["--grid-topic", "/g", "--grid-cell", "0.01"], "error: --grid-cell: "),
                          (["--grid-topic", "/g", "--grid-x-range", "5"], "error: --grid-x-range: "),
                          (["--grid-topic", "/g", "--ground-cell", "0.01"], "error: --ground-cell: ")):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(pre + bad)
            assert e.value.code == 2 and word in capsys.readouterr().err, bad
