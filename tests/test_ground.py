"""K30: the cloud split into ground and obstacles — the options, crafted cases that are exact, a
tilted scene with objects, the definition against a float64 ``atan2`` brute force, the messages,
the driver, bag replay and the CLI."""
import math
from dataclasses import FrozenInstanceError

import numpy as np
import pytest

from test_range2d import _Engine, _rig_messages
from triton_client_amd.ops import ground as G
from triton_client_amd.ops import laser_scan as L
from triton_client_amd.ops import range2d as R
from triton_client_amd.ros import compat, msgs, rosmsg

F = np.float32
PI = math.pi
INF = math.inf
NAN = math.nan
QUARTERS = dict(sectors=4)  # the edge table is exactly -2, -1, 0, 1, 2


# ------------------------------------------------------------------------------ options
def test_options_and_their_refusals():
    o = G.GroundOptions()
    assert (o.sectors, o.cell, o.range_min, o.range_max, o.sensor_height) == (360, 0.5, 0.0, 80.0, 1.8)
    assert (o.max_slope, o.noise, o.thickness, o.max_height) == (10.0, 0.05, 0.2, INF)
    assert o.nr == 160 and (o.h0, o.slope_q, o.noise_q, o.thick_q, o.top_q) == (-1843, 90, 51, 205, 2 ** 21)
    assert o.c32 == F(0.5) and o.r0 == F(0) and o.c32.dtype == F
    with pytest.raises(FrozenInstanceError):
        o.cell = 1.0
    assert G.GroundOptions(cell=0.05, range_max=25.6).nr == 512 and G.GroundOptions(sectors=1, range_max=0.4).nr == 1
    assert G.GroundOptions(range_max=80.2).nr == 161 and G.GroundOptions(cell=0.1, range_max=0.3).nr == 3
    assert G.GroundOptions(sectors=4096, range_max=128.0).nr == 256  # 2**20 cells
    assert G.GroundOptions(max_height=3.0).top_q == 3072 and G.GroundOptions(max_height=1e9).top_q == 2 ** 21
    assert G.GroundOptions(sensor_height=-2.0).h0 == 2048 and G.GroundOptions(sensor_height=1e9).h0 == -2 ** 21
    assert G.GroundOptions(max_slope=0).slope_q == 0 and G.GroundOptions(max_slope=45, cell=10, range_max=100).slope_q == 10240
    bad = {"sectors": [dict(sectors=0), dict(sectors=4097), dict(sectors=360.0), dict(sectors=True), dict(sectors="4")],
           "cell": [dict(cell=0.04), dict(cell=10.5), dict(cell=NAN), dict(cell=INF), dict(cell=None)],
           "range_min": [dict(range_min=-0.1), dict(range_min=NAN), dict(range_min=INF)],
           "range_max": [dict(range_max=INF), dict(range_max=NAN), dict(range_max=0.0), dict(range_min=5.0, range_max=5.0),
                         dict(range_min=9.0, range_max=5.0), dict(range_max=256.5), dict(cell=0.05, range_max=25.7),
                         dict(sectors=4096, range_max=128.5)],
           "sensor_height": [dict(sensor_height=NAN), dict(sensor_height=INF), dict(sensor_height="1")],
           "max_slope": [dict(max_slope=-1), dict(max_slope=45.5), dict(max_slope=NAN)],
           "noise": [dict(noise=-0.01), dict(noise=INF), dict(noise=NAN)],
           "thickness": [dict(thickness=-0.01), dict(thickness=INF), dict(thickness=NAN)],
           "max_height": [dict(max_height=0.2), dict(max_height=0.1), dict(max_height=-INF), dict(max_height=NAN),
                          dict(thickness=1.0, max_height=0.5)]}
    for field, cases in bad.items():
        for kw in cases:
            with pytest.raises(ValueError, match="^" + field):
                G.GroundOptions(**kw)


def test_the_edge_table():
    assert G.edge_table(G.GroundOptions(**QUARTERS)).tolist() == [-2.0, -1.0, 0.0, 1.0, 2.0]
    assert G.edge_table(G.GroundOptions(sectors=1)).tolist() == [-2.0, 2.0]
    for S in (1, 2, 3, 360, 4096):
        o = G.GroundOptions(sectors=S, range_max=20.0)
        t = G.edge_table(o)
        assert t.dtype == F and t.shape == (S + 1,) and (np.diff(t) >= 0).all() and not t.flags.writeable
        assert (t[0], t[-1]) == (-2.0, 2.0) and G.edge_angles(o)[-1] == PI
    # the laser scan's full-circle table of as many bins, but for the last edge's own rounding
    a, b = G.edge_table(G.GroundOptions()), L.edge_table(L.ScanOptions())
    assert np.abs(a.astype(np.float64) - b).max() <= 2 ** -22


# ------------------------------------------------------------------------ crafted, exact
def classes(points, **kw):
    return G.split_numpy(np.asarray(points, F).reshape(-1, 3), G.GroundOptions(**kw)).tolist()


def test_sector_edges_and_the_axis_behind():
    pts = np.array([[1, 0, -1.8], [0, 1, -1.8], [-1, 0.0, -1.8], [-1, -0.0, -1.8], [0, -1, -1.8], [2, -0.0, -1.8]], F)
    o = G.GroundOptions(**QUARTERS)
    sector, ring, zi, valid = G.cells_numpy(pts, o)
    assert sector.tolist() == [2, 3, 3, 0, 1, 2] and valid.all()  # +pi in the last sector, -pi in the first
    assert ring.tolist() == [2, 2, 2, 2, 2, 4] and (zi == -1843).all()
    cls, band = G.split_ref(pts, o)
    assert cls.tolist() == [1] * 6 and band.all()  # atan2 agrees; every one of them is on an edge
    assert G.split_numpy(pts, o).tolist() == [1] * 6


def test_rings_and_the_limits_of_validity():
    z = -1.8
    below = lambda v: float(np.nextafter(F(v), F(0)))  # noqa: E731
    above = lambda v: float(np.nextafter(F(v), F(1e9) if v > 0 else F(-1e9)))  # noqa: E731
    o = G.GroundOptions(range_min=2.0, range_max=10.0, **QUARTERS)
    assert o.nr == 20
    pts = np.array([[1.5, 0, z], [2.0, 0, z], [below(2.0), 0, z], [0, 2.5, z], [0, below(2.5), z], [10.0, 0, z],
                    [below(10.0), 0, z], [3, 4, z], [6, 8, z], [0, 0, z]], F)
    sector, ring, zi, valid = G.cells_numpy(pts, o)
    #                        < r_min  == r_min  below it  r = 5 cells  below   d == nr  below  3-4-5  d == nr  s == 0
    assert valid.tolist() == [False, True, False, True, True, False, True, True, False, False]
    assert ring[valid].tolist() == [4, 5, 4, 19, 10]
    hi = np.array([[3, 1, 512.0], [3, 1, -512.0], [3, 1, above(512.0)], [3, 1, above(-512.0)]], F)
    sector, ring, zi, valid = G.cells_numpy(hi, o)
    assert valid.tolist() == [True, True, False, False] and zi[:2].tolist() == [2 ** 19, -2 ** 19]
    # heights round half to even in 1/1024 m: 0.5 / 1024 -> 0, 1.5 / 1024 -> 2, -2.5 / 1024 -> -2
    half = np.array([[3, 1, 0.5 / 1024], [3, 1, 1.5 / 1024], [3, 1, -2.5 / 1024], [3, 1, 1.25 / 1024]], F)
    assert G.cells_numpy(half, o)[2].tolist() == [0, 2, -2, 1]


def test_not_finite_points_are_dropped():
    bad = [(NAN, 1, -1.8), (1, NAN, -1.8), (1, 1, NAN), (INF, 1, -1.8), (1, -INF, -1.8), (1, 1, INF), (1, 1, -INF),
           (-INF, INF, -1.8), (1e30, 1e30, -1.8), (0, 0, -1.8)]
    assert classes(bad + [(3, 1, -1.8)]) == [0] * len(bad) + [1]
    assert G.split_ref(np.asarray(bad + [(3, 1, -1.8)], F), G.GroundOptions())[0].tolist() == [0] * len(bad) + [1]


# one sector's rings, 1 m wide, the sensor 1 m up: ring -> the heights of its points.  slope_q = 181, noise_q = 51.
PROFILE = {0: [-1.0, 0.0],      # |-1024 - h0| = 0 <= 51 + 181: adopted; the point 1 m above it is an obstacle
           # ring 1 is empty: the ground is carried
           2: [0.5, 1.0],       # lowest 1536 above g, allow = 51 + 181 * 2: only an obstacle, the ground is carried
           3: [-1.1, -0.95],    # -1126: 102 below g, allow 594: adopted; -0.95 is 153 above it, within thick_q = 205
           4: [-3.0],           # 1946 below g, allow 232: an outlier, not adopted (below the ground: ground all the same)
           5: [-1.15, -0.9],    # -1178: allow = 51 + 181 * 2: adopted; -0.9 is 256 above it: an obstacle
           # a real step down of 1 m (1024): allow is 232, 413, 594, 775, 956 at rings 6..10 and 1137 at ring 11
           6: [-2.15], 7: [-2.15], 8: [-2.15], 9: [-2.15], 10: [-2.15, -0.5], 11: [-2.15, -1.9, -1.0]}
PROFILE_G = [-1024, -1024, -1024, -1126, -1126, -1178, -1178, -1178, -1178, -1178, -1178, -2202]
PROFILE_CLASSES = {0: [1, 2], 2: [2, 2], 3: [1, 1], 4: [1], 5: [1, 2], 6: [1], 7: [1], 8: [1], 9: [1], 10: [1, 2],
                   11: [1, 2, 2]}


def test_one_sectors_ring_profile():
    o = G.GroundOptions(sectors=4, cell=1.0, range_max=12.0, sensor_height=1.0)
    assert (o.nr, o.h0, o.slope_q, o.noise_q, o.thick_q) == (12, -1024, 181, 51, 205)
    pts = np.array([(j + 0.5, 0.1, z) for j, zs in PROFILE.items() for z in zs], F)
    want = [c for j in PROFILE for c in PROFILE_CLASSES[j]]
    ground = G.ground_numpy(pts, o)
    assert ground.shape == (12, 4) and ground.dtype == np.int32
    assert ground[:, 2].tolist() == PROFILE_G
    assert (ground[:, [0, 1, 3]] == -1024).all()  # the sectors without a point keep h0
    assert G.split_numpy(pts, o).tolist() == want
    assert G.split_ref(pts, o)[0].tolist() == want
    # max_height = 1.75 (top_q = 1792): of ring 2's points above the carried ground, z = 0.5 (1536) stays, z = 1.0 (2048) goes
    low = G.GroundOptions(sectors=4, cell=1.0, range_max=12.0, sensor_height=1.0, max_height=1.75)
    got = G.split_numpy(pts, low).tolist()
    assert got[2:4] == [2, 0] and got[:2] + got[4:] == want[:2] + want[4:]


# --------------------------------------------------------------------------------- scene
TILT = math.tan(math.radians(3.0))


def plane_z(x):
    """The tilted plane through (0, 0, -sensor_height)."""
    return -1.8 + TILT * x


def scene():
    """→ ``(points [N, 3] float32, kind [N]: 0 plane, 1 car, 2 wall, 3 pole, 4 slab, above [N]: metres above the
    plane)``.  The plane is sampled twice in every cell of the default grid from 2 to 60 m (away from the cells'
    edges in angle), with +-2 cm of noise; the objects stand within 30 m, where a cell is at most 0.53 m wide."""
    rng = np.random.default_rng(30)
    S, rings = 360, np.arange(4, 120)
    sec, ring = (a.reshape(-1) for a in np.meshgrid(np.arange(S), rings, indexing="ij"))
    sec, ring = np.repeat(sec, 2), np.repeat(ring, 2)
    a = -PI + (sec + rng.uniform(0.2, 0.8, len(sec))) * (2 * PI / S)
    r = (ring + rng.uniform(0.1, 0.9, len(ring))) * 0.5
    x, y = r * np.cos(a), r * np.sin(a)
    parts = [(x, y, np.zeros(len(x)) + rng.uniform(-0.02, 0.02, len(x)), 0)]

    def add(x, y, up, kind):
        parts.append((np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(up, np.float64), kind))

    for cx, cy, yaw in ((10, 3, 0.2), (-15, -6, 1.3), (4, -20, 2.0), (-8, 22, 0.7)):  # cars: 4 x 2 x 1.5 m, their sides
        n = 600
        u, side = rng.uniform(-1, 1, n), rng.integers(0, 4, n)
        lx = np.where(side < 2, u * 2.0, np.where(side == 2, 2.0, -2.0))
        ly = np.where(side < 2, np.where(side == 0, 1.0, -1.0), u * 1.0)
        add(cx + lx * math.cos(yaw) - ly * math.sin(yaw), cy + lx * math.sin(yaw) + ly * math.cos(yaw),
            rng.uniform(0.05, 1.5, n), 1)
    n = 2000  # a wall 12 m long and 2.5 m high
    add(rng.uniform(12, 24, n), np.full(n, -9.0) + rng.uniform(-0.02, 0.02, n), rng.uniform(0.05, 2.5, n), 2)
    for px, py in ((6, 6), (-5, 9), (14, -3), (-20, -14), (3, 25)):  # poles 5 cm thin, 2.8 m high
        n = 120
        add(px + rng.uniform(-0.025, 0.025, n), py + rng.uniform(-0.025, 0.025, n), rng.uniform(0.05, 2.8, n), 3)
    n = 1500  # a slab 4 m up, 6 x 6 m
    add(rng.uniform(-18, -12, n), rng.uniform(8, 14, n), np.full(n, 4.0) + rng.uniform(0, 0.05, n), 4)
    x, y, up = (np.concatenate([p[k] for p in parts]) for k in range(3))
    kind = np.concatenate([np.full(len(p[0]), p[3]) for p in parts])
    pts = np.stack([x, y, plane_z(x) + up], 1).astype(F)
    order = rng.permutation(len(pts))  # the objects are not the cloud's last points
    return pts[order], kind[order], up[order]


def gaussian_cloud(seed=31, n=20000):
    rng = np.random.default_rng(seed)
    return np.stack([rng.normal(0, 30, n), rng.normal(0, 30, n), rng.normal(-1.5, 0.6, n)], 1).astype(F)


@pytest.fixture(scope="module")
def scenes():
    """The scene and the Gaussian cloud, with the definition's classes and the reference's: made once."""
    o = G.GroundOptions()
    pts, kind, up = scene()
    g = gaussian_cloud()
    return {"scene": (pts, kind, up, G.split_numpy(pts, o), G.split_ref(pts, o)),
            "gauss": (g, None, None, G.split_numpy(g, o), G.split_ref(g, o))}


def test_scene_plane_is_ground_and_objects_are_obstacles(scenes):
    pts, kind, up, cls, _ = scenes["scene"]
    assert len(pts) == 2 * 360 * 116 + 2400 + 2000 + 600 + 1500
    assert (cls[kind == 0] == G.GROUND).all()  # every plane point
    high = (kind > 0) & (up > 0.2 + 0.1)
    assert high.sum() > 5000 and (cls[high] == G.OBSTACLE).all()  # every object point well above the plane
    assert (cls[kind == 4] == G.OBSTACLE).all() and (kind == 4).sum() == 1500
    # neighbouring cell minima differ by far less than the sweep allows: the ground follows the plane everywhere
    ground = G.ground_numpy(pts, G.GroundOptions())
    assert np.abs(np.diff(ground[4:120].astype(np.int64), axis=0)).max() <= 51 + 90
    low = G.split_numpy(pts, G.GroundOptions(max_height=3.0))
    assert (low[kind == 4] == G.DROPPED).all() and (low[kind != 4] == cls[kind != 4]).all()  # only the slab goes


@pytest.mark.parametrize("name", ["scene", "gauss"])
def test_definition_equals_the_reference_outside_the_bands(scenes, name):
    pts, _, _, cls, (cls64, band) = scenes[name]
    o = G.GroundOptions()
    assert band.mean() < 1e-3  # a test that banded everything away would fail
    rest = pts[~band]
    assert not G.split_ref(rest, o)[1].any()  # flags are per point: the remainder has none
    got, want = G.split_numpy(rest, o), G.split_ref(rest, o)[0]
    np.testing.assert_array_equal(got, want)
    assert min((want == k).sum() for k in (1, 2)) > 1000  # and the cloud decides something
    if name == "gauss":
        assert (want == 0).sum() > 10  # beyond 80 m


def test_points_on_cell_edges_are_banded():
    o = G.GroundOptions(range_min=2.0)
    a = -PI + 17 * (2 * PI / 360)  # a sector edge
    pts = np.array([[7 * math.cos(a), 7 * math.sin(a), -1.8],  # on a sector edge
                    [3.0, 0.3, -1.8], [6.5 * 0.8, 6.5 * 0.6, -1.8],  # d == 13 exactly
                    [2 * 0.6, 2 * 0.8, -1.8],  # r == range_min
                    [80 * 0.6, 80 * 0.8, -1.8],  # d == nr
                    [3.1, 0.3, -1.8]], F)
    assert G.split_ref(pts, o)[1].tolist() == [True, False, True, True, True, False]


# ---------------------------------------------------------------------------- invariants
def test_the_order_of_points_does_not_matter(scenes):
    pts, _, _, cls, _ = scenes["gauss"]
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(len(pts))
        np.testing.assert_array_equal(G.split_numpy(pts[perm], G.GroundOptions()), cls[perm])


def make_cloud(points, step=16, offsets=(0, 4, 8), seq=7, height=1, seed=0):
    """The points as a PointCloud2 of ``step``-byte records, x, y, z at ``offsets``, every other byte noise."""
    p = np.asarray(points, F).reshape(-1, 3)
    raw = np.random.default_rng(seed + len(p)).integers(0, 256, (len(p), step), dtype=np.uint8)
    for j in range(3):
        raw[:, offsets[j]:offsets[j] + 4] = np.ascontiguousarray(p[:, j]).view(np.uint8).reshape(-1, 4)
    fields = [msgs.PointField(n, o, 7, 1) for n, o in zip("xyz", offsets)]
    if step >= 16 and offsets == (0, 4, 8):
        fields.append(msgs.PointField("intensity", 12, 7, 1))
    assert len(p) % height == 0
    return msgs.PointCloud2(header=msgs.Header(seq=seq, stamp=msgs.Time(12, 345), frame_id="os"), height=height,
                            width=len(p) // height, fields=fields, is_bigendian=False, point_step=step,
                            row_step=step * (len(p) // height), data=raw.tobytes(), is_dense=False)


@pytest.mark.parametrize("step,offsets", [(16, (0, 4, 8)), (18, (1, 5, 9)), (32, (4, 12, 20))])
def test_messages_are_rows_of_the_input(step, offsets):
    o = G.GroundOptions()
    pts = gaussian_cloud(5, 3000)
    c = make_cloud(pts, step, offsets)
    np.testing.assert_array_equal(R.cloud_xyzi(c)[:, :3].view(np.uint32), pts.view(np.uint32))
    cls = G.split_numpy(pts, o)
    rows = np.frombuffer(c.data, np.uint8).reshape(-1, step)
    obs, gnd = G.split_cloud_numpy(c, o)
    for m, k in ((obs, 2), (gnd, 1)):
        n = int((cls == k).sum())
        assert n > 300 and m.data == rows[cls == k].tobytes() and isinstance(m.data, bytes)
        assert (m.height, m.width, m.point_step, m.row_step, m.is_dense) == (1, n, step, n * step, True)
        assert m.header == c.header and m.fields == c.fields and m.is_bigendian is False
        assert rosmsg.deserialize(rosmsg.serialize(m), "sensor_msgs/PointCloud2").data == m.data
    assert (cls == 0).sum() > 10 and obs.width + gnd.width == len(pts) - (cls == 0).sum()
    assert G.split_cloud_numpy(c, o, 1) == (obs, None) and G.split_cloud_numpy(c, o, 2) == (None, gnd)
    with pytest.raises(ValueError, match="want"):
        G.split_cloud_numpy(c, o, 0)
    with pytest.raises(ValueError, match="want"):
        G.GroundSplitter("cpu").split([c], o, 4)


def test_organised_and_empty_clouds():
    o = G.GroundOptions()
    pts = gaussian_cloud(6, 1200)
    flat, grid = make_cloud(pts), make_cloud(pts, height=4)
    assert (grid.height, grid.width) == (4, 300) and grid.data == flat.data
    a, b = G.split_cloud_numpy(grid, o), G.split_cloud_numpy(flat, o)
    assert a == b and a[0].height == 1 and a[0].width + a[1].width > 1000
    empty = make_cloud(np.zeros((0, 3), F))
    obs, gnd = G.split_cloud_numpy(empty, o)
    assert obs == gnd and (obs.width, obs.row_step, obs.data, obs.fields) == (0, 0, b"", empty.fields)
    assert G.split_numpy(np.zeros((0, 3), F), o).shape == (0,)


def test_layouts_the_switch_and_the_splitter_on_the_cpu(monkeypatch):
    from triton_client_amd.ops.cloud_common import CloudLayout

    assert G.layout_device_ok(CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7)))
    assert G.layout_device_ok(CloudLayout(18, (1, 5, 9, -1), (7, 7, 7, 2)))  # the intensity is not read
    assert not G.layout_device_ok(CloudLayout(16, (0, 4, 8, 12), (7, 7, 8, 7)))
    assert not G.layout_device_ok(CloudLayout(16, (0, 4, 8, 12), (7, 7, 7, 7), True))
    assert G.device_enabled()
    monkeypatch.setenv("TCA_DEVICE_GROUND", "0")
    assert not G.device_enabled()
    clouds, _ = _rig_messages()
    sp = G.GroundSplitter("cpu")
    got = sp.split(clouds, OPTS)
    assert not sp.gpu and got == [G.split_cloud_numpy(c, OPTS) for c in clouds] and sp.split([], OPTS) == []
    # 64 clouds, 2^31 staged bytes and 2^24 cells to a launch

    class Big:
        data = range(2 ** 29)  # (only its length is asked for)

    assert [len(p) for p in sp._parts(list(range(150)), [clouds[0]] * 150)] == [64, 64, 22]
    assert [len(p) for p in sp._parts(list(range(9)), [Big] * 9)] == [3, 3, 3]
    wide = G.GroundOptions(sectors=4096, range_max=128.0)  # 2^20 cells a cloud
    assert [len(p) for p in sp._parts_for(wide)(list(range(40)), [clouds[0]] * 40)] == [16, 16, 8]


# ----------------------------------------------------------------------- driver, bag, CLI
OPTS = G.GroundOptions(range_max=40.0, sensor_height=1.5)  # the rig's walls span z = -1.5 .. 0.5


def _expected(cloud, o=OPTS):
    return G.split_cloud_numpy(cloud, o)


def test_the_rig_has_both_classes():
    clouds, _ = _rig_messages()
    for c in clouds:
        obs, gnd = _expected(c)
        assert obs.width > 50 and gnd.width > 10 and obs.width + gnd.width == 300


@pytest.mark.parametrize("topics", [("obstacles",), ("ground",), ("obstacles", "ground")])
@pytest.mark.parametrize("batch,workers", [(1, 1), (4, 2)])
def test_driver_publishes_the_definition_and_keeps_every_other_byte(batch, workers, topics):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.ros.bus import TopicBus

    clouds, _ = _rig_messages()

    def drive(on):
        bus = TopicBus()
        seen = {t: [] for t in ("/o", "/bev", "/pts", "/trk", "/scan")}
        got, order = {"obstacles": [], "ground": []}, []
        for t, ty in (("/o", msgs.BoundingBoxArray), ("/bev", msgs.Image), ("/pts", msgs.PointCloud2),
                      ("/trk", msgs.BoundingBoxArray), ("/scan", msgs.LaserScan)):
            compat.Subscriber(t, ty, lambda m, t=t: seen[t].append(rosmsg.serialize(m)), bus=bus)
        for name in got:
            compat.Subscriber("/" + name, msgs.PointCloud2, got[name].append, bus=bus)
        kw = dict(ground_options=OPTS, **{name + "_topic": "/" + name for name in topics}) if on else {}
        drv = RosInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=batch,
                             workers=workers, queue_size=64, bev_topic="/bev", points_topic="/pts", tracks_topic="/trk",
                             scan_topic="/scan", **kw)
        drv.start_inference(spin=False)
        for name, p in [("box", drv.pub), *drv.side_pubs.items()]:  # the order the driver publishes in
            def publish(m, name=name, send=p.publish):
                order.append((name, m.header.seq))
                send(m)
            p.publish = publish
        pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
        for c in clouds:
            pub.publish(c)
        runner = drv.runner
        drv.stop()
        bus.close()
        assert runner is None or not runner.errors, runner.errors
        return seen, got, order, drv

    seen1, got1, order, drv1 = drive(True)
    for k, name in enumerate(("obstacles", "ground")):
        if name in topics:
            assert got1[name] == [_expected(c)[k] for c in clouds] and got1[name][0].header == clouds[0].header
        else:
            assert got1[name] == [] and name not in drv1.side_pubs
    # after the box message and every other output of the same cloud, the scan among them
    names = ["box", "bev", "points", "tracks", "scan"] + [n for n in ("obstacles", "ground") if n in topics]
    assert order == [(k, s) for s in (1, 2, 3, 4) for k in names]
    seen0, got0, _, drv0 = drive(False)
    assert got0 == {"obstacles": [], "ground": []} and not hasattr(drv0.engine, "_ground_splitter")
    assert seen1 == seen0 and all(len(v) == 4 for v in seen1.values())
    assert drv1.engine._ground_splitter.gpu is False


def test_process_shapes_and_constructor_refusals():
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.inference import ros_inference3d as M

    class Stages:
        """What the driver's stage timer reports to."""
        def __init__(self):
            self.names = []

        def stage(self, name, seconds):
            self.names.append(name)

        def frame(self, n=1):
            pass

    # the pinned tables are as they were; the split clouds follow them
    assert [n for n, _ in M.SIDE_OUTPUTS] == ["bev", "points", "tracks", "ranged", "depth"]
    assert M.NAV_OUTPUTS == (("scan", msgs.LaserScan),) and M.OUTPUTS == M.SIDE_OUTPUTS + M.NAV_OUTPUTS
    assert M.CLOUD_OUTPUTS == (("obstacles", msgs.PointCloud2), ("ground", msgs.PointCloud2))
    assert M.ALL_OUTPUTS == M.OUTPUTS + M.CLOUD_OUTPUTS
    fields = [f.name for f in __import__("dataclasses").fields(M.CloudResult)]
    assert fields[-3:] == ["scan", "obstacles", "ground"] and fields[:2] == ["boxes", "pred"]
    clouds, _ = _rig_messages()
    metrics = Stages()
    drv = RosInference3D(engine=_Engine(), params={}, obstacles_topic="/obs", ground_topic="/gnd", metrics=metrics,
                         ground_options={"range_max": 40.0, "sensor_height": 1.5})
    assert drv.ground_options == OPTS
    for r, c in zip(drv.process(clouds), clouds):
        obs, gnd = _expected(c)
        assert r.pred["obstacles"] is r.obstacles and r.pred["ground"] is r.ground  # they ride in the prediction too
        assert (r.obstacles, r.ground) == (obs, gnd) and r.scan is None and r.bev is None
    assert "ground_split" in metrics.names
    one = RosInference3D(engine=_Engine(), params={}, ground_topic="/gnd")
    assert one.ground_options == G.GroundOptions() and one.obstacles_topic is None  # the defaults
    for r, c in zip(one.process(clouds), clouds):
        assert r.obstacles is None and "obstacles" not in r.pred and r.ground == G.split_cloud_numpy(c, G.GroundOptions())[1]
    off = RosInference3D(engine=_Engine(), params={})
    assert all("ground" not in r.pred and r.ground is None and r.obstacles is None for r in off.process(clouds))
    assert off.ground_topic is None and off.obstacles_topic is None
    with pytest.raises(ValueError, match="cell"):
        RosInference3D(engine=_Engine(), params={}, ground_topic="/g", ground_options={"cell": 0.01})
    with pytest.raises(TypeError):
        RosInference3D(engine=_Engine(), params={}, obstacles_topic="/o", ground_options={"width": 3})


def test_bag_replay_writes_the_clouds(tmp_path):
    from triton_client_amd.inference import BagInference3D
    from triton_client_amd.ros import Bag

    clouds, _ = _rig_messages()
    src = str(tmp_path / "rig.bag")
    with Bag(src, "w") as b:
        for c in clouds:
            b.write("/pc", c)

    def replay(out, **kw):
        drv = BagInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bagfile=src,
                             out_bag=out, batch=3, points_topic="/pts", scan_topic="/scan", **kw)
        assert drv.start_inference() == 4
        with Bag(out) as b:
            return [(t, m) for t, m, _ in b.read_messages()]

    on = replay(str(tmp_path / "on.bag"), obstacles_topic="/obs", ground_topic="/gnd", ground_options=OPTS)
    off = replay(str(tmp_path / "off.bag"))
    for k, topic in enumerate(("/obs", "/gnd")):
        got = [m for t, m in on if t == topic]
        assert got == [_expected(c)[k] for c in clouds] and [m.header.seq for m in got] == [1, 2, 3, 4]
    rest = [(t, rosmsg.serialize(m)) for t, m in on if t not in ("/obs", "/gnd")]
    assert rest == [(t, rosmsg.serialize(m)) for t, m in off] and len(rest) == 16
    assert [t for t, _ in on][:6] == ["/pc", "/o", "/pts", "/scan", "/obs", "/gnd"]  # after the scan
    only = replay(str(tmp_path / "one.bag"), obstacles_topic="/obs")  # the default options, one half
    assert [t for t, _ in only][:5] == ["/pc", "/o", "/pts", "/scan", "/obs"] and "/gnd" not in {t for t, _ in only}


def test_flags_and_usage_errors(capsys):
    from triton_client_amd.cli import bag3d, main3d

    f = main3d.parse_args([])
    assert f.obstacles_topic == "" and f.ground_topic == "" and f.ground_options is None
    for mod, pre in ((main3d, []), (bag3d, ["--bag", "x"])):
        assert mod.parse_args(pre + ["--obstacles-topic", "/obs"]).ground_options == G.GroundOptions()
        assert mod.parse_args(pre + ["--ground-topic", "/gnd"]).ground_options == G.GroundOptions()
        f = mod.parse_args(pre + ["--obstacles-topic", "/obs", "--ground-topic", "/gnd", "--ground-sectors", "720",
                                  "--ground-cell", "0.25", "--ground-range", "1.5,60", "--ground-sensor-height", "2.1",
                                  "--ground-slope", "7.5", "--ground-noise", "0.03", "--ground-thickness", "0.15",
                                  "--ground-max-height", "3"])
        assert f.ground_options == G.GroundOptions(720, 0.25, 1.5, 60.0, 2.1, 7.5, 0.03, 0.15, 3.0)
        assert (f.obstacles_topic, f.ground_topic, f.ground_options.nr) == ("/obs", "/gnd", 240)
        topic = "--obstacles-topic"
        for bad, word in ((["--ground-sectors", "90"], topic), (["--ground-cell", "1"], topic),
                          (["--ground-range", "0,50"], topic), (["--ground-sensor-height", "2"], topic),
                          (["--ground-slope", "5"], topic), (["--ground-noise", "0.1"], topic),
                          (["--ground-thickness", "0.1"], topic), (["--ground-max-height", "2"], topic),
                          (["--ground-topic", "/g", "--ground-sectors", "0"], "--ground-sectors"),
                          (["--ground-topic", "/g", "--ground-sectors", "5000"], "--ground-sectors"),
                          (["--ground-topic", "/g", "--ground-cell", "0.01"], "--ground-cell"),
                          (["--ground-topic", "/g", "--ground-range", "5"], "--ground-range"),
                          (["--ground-topic", "/g", "--ground-range", "0,x"], "--ground-range"),
                          (["--ground-topic", "/g", "--ground-range", "9,5"], "--ground-range"),
                          (["--ground-topic", "/g", "--ground-range", "0,300"], "--ground-range"),
                          (["--ground-topic", "/g", "--ground-range=-1,50"], "--ground-range"),
                          (["--obstacles-topic", "/o", "--ground-slope", "60"], "--ground-slope"),
                          (["--obstacles-topic", "/o", "--ground-noise=-1"], "--ground-noise"),
                          (["--obstacles-topic", "/o", "--ground-thickness=-1"], "--ground-thickness"),
                          (["--obstacles-topic", "/o", "--ground-max-height", "0.1"], "--ground-max-height"),
                          (["--obstacles-topic", "/o", "--ground-sensor-height", "nan"], "--ground-sensor-height")):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(pre + bad)
            err = capsys.readouterr().err  # a flag without a topic says so; a bad value names its flag
            assert e.value.code == 2 and (f"{bad[0]} needs --obstacles-topic TOPIC or --ground-topic TOPIC"
                                          if word == topic else f"error: {word}: ") in err, (bad, err[-200:])
