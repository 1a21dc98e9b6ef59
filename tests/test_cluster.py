"""K31: the obstacle clusters — the definition against a float64 flood fill on the shapes a labelling kernel can
get wrong, the options, the box message, the driver, the CLI and the host chain behind the ground split."""
import dataclasses

import numpy as np
import pytest

from test_ground import OPTS as GROUND
from test_range2d import _Engine, _rig_messages
from triton_client_amd.ops import cluster as C
from triton_client_amd.ops import ground as G
from triton_client_amd.ros import msgs, rosmsg

F = np.float32


def grid(W, H, **kw):
    """A grid of ``W x H`` cells of 0.5 m from the origin; the ground stays in."""
    return C.ClusterOptions(cell=0.5, x_range=(0.0, W / 2), y_range=(0.0, H / 2), remove_ground=False, **kw)


def place(cells, seed=0):
    """The one helper that places points: ``cells`` (ix, iy, count) → points at the cells' centres (0.5 m cells from
    the origin) with a jitter of at most 0.3 cell, z within +-1 m."""
    rng = np.random.default_rng(seed)
    c = np.repeat(np.asarray(cells, np.int64).reshape(-1, 3), np.asarray(cells, np.int64).reshape(-1, 3)[:, 2], 0)
    xy = (c[:, :2] + 0.5 + rng.uniform(-0.3, 0.3, (len(c), 2))) * 0.5
    return np.concatenate([xy, rng.uniform(-1, 1, (len(c), 1))], 1).astype(F)


def blobs(W, H, seed):
    """Random occupancy of about a third of the cells, one to three points each: components of every size."""
    rng = np.random.default_rng(seed)
    on = np.argwhere(rng.random((W, H)) < 0.34)
    return [(x, y, rng.integers(1, 4)) for x, y in on]


def spiral(x0, y0, n=32):
    """A one-cell-wide square spiral that fills an ``n x n`` block of cells: one component, one long chain."""
    seen, x, y, dx, dy = {(0, 0)}, 0, 0, 1, 0
    while True:
        for _ in range(2):  # straight on while the cell after the next is free, else one turn
            ahead, after = (x + dx, y + dy), (x + 2 * dx, y + 2 * dy)
            if 0 <= ahead[0] < n and 0 <= ahead[1] < n and ahead not in seen and after not in seen:
                break
            dx, dy = -dy, dx
        else:
            return [(x0 + cx, y0 + cy, 1) for cx, cy in seen]
        x, y = ahead
        seen.add(ahead)


SPIRAL = spiral(32, 32)
COMB = [(x, 0, 1) for x in range(96)] + [(x, y, 1) for x in range(0, 96, 2) for y in range(1, 31)]
U_SHAPE = [(x, y, 1) for x in range(20, 33) for y in (5, 9)] + [(33, y, 1) for y in range(5, 10)]
ISLANDS = [(3 * i + 1, 2, 5) for i in range(7)]
OUTSIDE = np.array([[-0.1, 1.1, 0], [1.1, -0.1, 0], [15.6, 1.1, 0], [1.1, 16.6, 0], [600, 1.1, 0], [1.1, -600, 0],
                    [1.1, 1.1, 3.0], [1.1, 1.1, -3.0], [np.inf, 1.1, 0], [1.1, 1.1, np.nan], [1e30, 1e30, 0]]
                   + [[1.2, 1.3, 0.5]] * 6, F)
# name → (options, points): the smallest shapes at which a labelling kernel can go wrong
SHAPES = {
    "one_cell": (grid(1, 1), place([(0, 0, 7)])),
    "31x33": (grid(31, 33), place(blobs(31, 33, 1), 1)),
    "33x31": (grid(33, 31), place(blobs(33, 31, 2), 2)),
    "64x64": (grid(64, 64), place(blobs(64, 64, 3), 3)),
    "65x40": (grid(65, 40), place(blobs(65, 40, 4), 4)),
    # across a tile border sideways, upwards, and only diagonally where four tiles meet, in both directions
    "borders": (grid(96, 64), place([(30, 5, 2), (31, 5, 2), (32, 5, 2), (5, 30, 2), (5, 31, 2), (5, 32, 2),
                                    (31, 31, 3), (32, 32, 3), (64, 31, 3), (63, 32, 3)])),
    "diagonal_of_a_third": (grid(31, 33), place([(10, 10, 3), (11, 11, 3), (12, 10, 3)])),
    "spiral": (grid(64, 64), place(SPIRAL)),
    "comb": (grid(96, 32), place(COMB)),
    "u_joined_in_the_next_tile": (grid(64, 32), place(U_SHAPE)),
    "sizes": (grid(31, 33, min_points=5, max_points=9), place([(1, 1, 5), (4, 1, 4), (7, 1, 9), (10, 1, 10)])),
    "bridge": (grid(31, 33, min_cell_points=2, min_points=3), place([(3, 3, 3), (4, 3, 1), (5, 3, 3)])),
    "more_than_max_clusters": (grid(31, 33, max_clusters=4), place(ISLANDS)),
    "all_nan": (grid(31, 33), np.full((300, 3), np.nan, F)),
    "outside": (grid(31, 33, z_range=(-2.0, 2.0)), OUTSIDE),
    **{f"{n}_points": (grid(65, 40, min_points=1), place(blobs(65, 40, 9), 9)[:n]) for n in (0, 1, 255, 256, 257)},
}
# what the crafted shapes must give: found, and the sizes of the reported clusters in root order
EXPECT = {"one_cell": (1, [7]), "borders": (4, [6, 6, 6, 6]), "diagonal_of_a_third": (1, [9]), "spiral": (1, [len(SPIRAL)]),
          "comb": (1, [96 + 48 * 30]), "u_joined_in_the_next_tile": (1, [31]), "sizes": (2, [5, 9]),
          "bridge": (2, [3, 3]), "more_than_max_clusters": (7, [5, 5, 5, 5]), "all_nan": (0, []), "outside": (1, [6]),
          "0_points": (0, []), "1_points": (1, [1])}


def same(a, b):
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes()


@pytest.fixture(scope="module")
def refs():
    """The float64 flood fill of every shape, made once (``test_cluster_gpu.py`` shares it)."""
    return {name: C.cluster_ref(pts, o) for name, (o, pts) in SHAPES.items()}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_definition_equals_the_flood_fill(refs, name):
    o, pts = SHAPES[name]
    *ref, band = refs[name]
    assert not band.any()  # 0.2 cell from every edge is orders of magnitude wider than the band
    got = C.cluster_numpy(pts, o)
    same(got, ref)
    found, label, table = got
    assert label.dtype == np.int32 and label.shape == (len(pts),) and table.dtype == C.TABLE_DTYPE
    assert len(table) == min(found, o.max_clusters) and table["n"].sum() == (label >= 0).sum()
    if name in EXPECT:
        assert (found, table["n"].tolist()) == EXPECT[name]
    else:
        assert found > 3 and (np.diff(table["root"]) > 0).all()
    same(C.cluster_numpy(pts[::-1], o), (found, label[::-1], table))  # nothing depends on the order of the points


def test_labels_bounds_and_sums_of_a_crafted_cloud():
    o, pts = SHAPES["more_than_max_clusters"]
    found, label, table = C.cluster_numpy(pts, o)
    assert label.tolist() == [k for k in (0, 1, 2, 3) for _ in range(5)] + [-1] * 15  # -1 beyond the cap
    assert table["root"].tolist() == [2 * 31 + 3 * i + 1 for i in range(4)] and not table["pad"].any()
    q = np.rint(pts[:5].astype(np.float64) * 1024).astype(np.int64)
    row = table[0]
    assert [row["min_x"], row["max_y"], row["sum_z"]] == [q[:, 0].min(), q[:, 1].max(), q[:, 2].sum()]
    edge = np.array([[0.5, 0.25, 0.5 / 1024], [15.49, 16.49, 1.5 / 1024]], F)  # truncation; ties to even
    cell, qq = C.cells_numpy(edge, grid(31, 33))
    assert cell.tolist() == [1, 32 * 31 + 30] and qq[:, 2].tolist() == [0, 2]


def test_options_and_their_refusals():
    o = C.ClusterOptions()
    assert (o.cell, o.x_range, o.y_range, o.z_range) == (0.4, (-80.0, 80.0), (-80.0, 80.0), (-512.0, 512.0))
    assert (o.min_cell_points, o.min_points, o.max_points, o.max_clusters, o.remove_ground) == (1, 5, 2 ** 31 - 1, 1024, True)
    assert (o.W, o.H) == (400, 400) and C.ClusterOptions(cell=0.25, x_range=[-256, 256]).W == 2048
    with pytest.raises(dataclasses.FrozenInstanceError):
        o.cell = 1.0
    bad = {"cell": [dict(cell=0.04), dict(cell=11), dict(cell=np.nan), dict(cell=None)],
           "x_range": [dict(x_range=(5, 5)), dict(x_range=(-513, 0)), dict(x_range=(0, np.inf)), dict(x_range=3),
                       dict(cell=0.05, x_range=(-80, 80))],
           "y_range": [dict(y_range=(9, 5)), dict(y_range=(0, 600)), dict(cell=0.05, x_range=(0, 102.4))],
           "z_range": [dict(z_range=(1, 1)), dict(z_range=(-600, 0))],
           "min_cell_points": [dict(min_cell_points=0), dict(min_cell_points=1.0)],
           "min_points": [dict(min_points=0), dict(min_points=True)], "max_points": [dict(max_points=4)],
           "max_clusters": [dict(max_clusters=0), dict(max_clusters=4097)], "remove_ground": [dict(remove_ground=1)]}
    for field, cases in bad.items():
        for kw in cases:
            with pytest.raises(ValueError, match="^" + field):
                C.ClusterOptions(**kw)


@pytest.mark.parametrize("jsk", [True, False])
def test_box_message_of_a_hand_made_table(jsk):
    table = np.zeros(2, C.TABLE_DTYPE)
    table[0] = (7, 40, 1024, 3072, -2048, -1024, 0, 512, 0, 0, 0, 0)
    table[1] = (300, 90, -5, 6, 10, 10, -1024, 1024, 0, 0, 0, 0)
    hdr = msgs.Header(seq=9, stamp=msgs.Time(3, 4), frame_id="os")
    m = C.cluster_boxes(table, hdr, jsk)
    assert m.header == hdr and type(m) is (msgs.BoundingBoxArray if jsk else msgs.Detection3DArray)
    boxes = m.boxes if jsk else m.detections
    pose = [b.pose if jsk else b.bbox.center for b in boxes]
    size = [b.dimensions if jsk else b.bbox.size for b in boxes]
    assert [(p.position.x, p.position.y, p.position.z) for p in pose] == [(2.0, -1.5, 0.25), (0.5 / 1024, 10 / 1024, 0.0)]
    assert [(s.x, s.y, s.z) for s in size] == [(2.0, 1.0, 0.5), (11 / 1024, 0.0, 2.0)]
    assert all((p.orientation.x, p.orientation.y, p.orientation.z, p.orientation.w) == (0, 0, 0, 1) for p in pose)
    assert [(b.value, b.label) if jsk else (b.results[0].score, b.results[0].id) for b in boxes] == [(7.0, 0), (300.0, 1)]
    assert len(C.cluster_boxes(table[:0], hdr, jsk).boxes if jsk else C.cluster_boxes(table[:0], hdr, jsk).detections) == 0


def test_the_host_chain_clusters_the_obstacle_rows():
    clouds, _ = _rig_messages()
    o = C.ClusterOptions()
    for c in clouds:
        pts = C.cloud_xyzi(c)
        rows = pts[G.split_numpy(pts, GROUND) == G.OBSTACLE]
        got = C.cluster_cloud_numpy(c, o, GROUND)
        same(got, C.cluster_numpy(rows, o))
        assert got[0] >= 1 and len(got[1]) == len(rows) < len(pts)  # labels per obstacle record
    kept = dataclasses.replace(o, remove_ground=False)
    same(C.cluster_cloud_numpy(clouds[0], kept), C.cluster_numpy(C.cloud_xyzi(clouds[0]), kept))
    ex = C.ClusterExtractor("cpu")
    assert not ex.gpu and ex.extract([], o) == []
    same(ex.extract(clouds[:1], o, GROUND)[0], C.cluster_cloud_numpy(clouds[0], o, GROUND))
    assert [len(p) for p in ex._parts_for(C.ClusterOptions(cell=0.1), None)(list(range(9)), clouds[:1] * 9)] == [6, 3]


def test_driver_publishes_the_clusters_last(monkeypatch):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.inference import ros_inference3d as M
    from triton_client_amd.ros import compat
    from triton_client_amd.ros.bus import TopicBus

    assert [n for n, _ in M.SIDE_OUTPUTS] == ["bev", "points", "tracks", "ranged", "depth"]  # the pinned tables
    assert M.ALL_OUTPUTS == M.SIDE_OUTPUTS + M.NAV_OUTPUTS + M.CLOUD_OUTPUTS and M.OBJECT_OUTPUTS == (("clusters", None),)
    assert M.PUBLISHED == M.ALL_OUTPUTS + M.OBJECT_OUTPUTS
    fields = [f.name for f in dataclasses.fields(M.CloudResult)]
    assert fields[:2] == ["boxes", "pred"] and fields[-4:] == ["clusters", "scan", "obstacles", "ground"]
    clouds, _ = _rig_messages()
    stages, order, bus = [], [], TopicBus()
    metrics = type("Stages", (), {"stage": lambda self, name, s: stages.append(name), "frame": lambda self, n=1: None})()
    drv = RosInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, metrics=metrics,
                         ground_topic="/gnd", ground_options=GROUND, clusters_topic="/clusters",
                         cluster_options={"min_points": 3})
    o = C.ClusterOptions(min_points=3)
    assert drv.cluster_options == o and drv.ground_options == GROUND
    for r, c in zip(drv.process(clouds), clouds):
        want = C.cluster_boxes(C.cluster_cloud_numpy(c, o, GROUND)[2], c.header)
        assert r.pred["clusters"] is r.clusters and rosmsg.serialize(r.clusters) == rosmsg.serialize(want)
        assert len(r.clusters.boxes) >= 1 and r.clusters.header == c.header
    assert stages.index("cluster") > stages.index("ground_split")
    drv.start_inference(spin=False)
    for name, p in drv.side_pubs.items():
        monkeypatch.setattr(p, "publish", lambda m, name=name: order.append(name))
    compat.Publisher("/pc", msgs.PointCloud2, bus=bus).publish(clouds[0])
    drv.stop()
    bus.close()
    assert order == ["ground", "clusters"]  # after the ground cloud: last of the cloud's messages
    alone = RosInference3D(engine=_Engine(), params={}, clusters_topic="/c")  # the defaults of both option sets
    assert (alone.cluster_options, alone.ground_options) == (C.ClusterOptions(), G.GroundOptions())
    assert all(r.clusters is None and "clusters" not in r.pred
               for r in RosInference3D(engine=_Engine(), params={}).process(clouds))
    with pytest.raises(ValueError, match="cell"):
        RosInference3D(engine=_Engine(), params={}, clusters_topic="/c", cluster_options={"cell": 0.01})


def test_flags_and_usage_errors(capsys):
    from triton_client_amd.cli import bag3d, main3d

    for mod, pre in ((main3d, []), (bag3d, ["--bag", "x"])):
        f = mod.parse_args(pre)
        assert f.clusters_topic == "" and f.cluster_options is None and f.ground_options is None
        f = mod.parse_args(pre + ["--clusters-topic", "/c", "--ground-sensor-height", "2.1"])  # legal with this topic alone
        assert f.cluster_options == C.ClusterOptions() and f.ground_options == G.GroundOptions(sensor_height=2.1)
        f = mod.parse_args(pre + ["--clusters-topic", "/c", "--cluster-cell", "0.25", "--cluster-x-range=-20,60",
                                  "--cluster-y-range=-30,30", "--cluster-z-range=-2,3", "--cluster-min-points", "8",
                                  "--cluster-max-points", "5000", "--cluster-min-cell-points", "2", "--cluster-max", "64",
                                  "--cluster-keep-ground"])
        assert f.cluster_options == C.ClusterOptions(0.25, (-20, 60), (-30, 30), (-2, 3), 2, 8, 5000, 64, False)
        for bad, word in ((["--cluster-cell", "1"], "--cluster-cell needs --clusters-topic TOPIC"),
                          (["--cluster-keep-ground"], "--cluster-keep-ground needs --clusters-topic TOPIC"),
                          (["--ground-slope", "5"], "--ground-slope needs --obstacles-topic TOPIC or --ground-topic TOPIC"),
                          (["--clusters-topic", "/c", "--cluster-cell", "0.01"], "error: --cluster-cell: "),
                          (["--clusters-topic", "/c", "--cluster-x-range", "5"], "error: --cluster-x-range: "),
                          (["--clusters-topic", "/c", "--cluster-y-range=9,5"], "error: --cluster-y-range: "),
                          (["--clusters-topic", "/c", "--cluster-max", "5000"], "error: --cluster-max: "),
                          (["--clusters-topic", "/c", "--cluster-min-points", "9", "--cluster-max-points", "3"],
                           "error: --cluster-max-points: "),
                          (["--clusters-topic", "/c", "--ground-cell", "0.01"], "error: --ground-cell: ")):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(pre + bad)
            assert e.value.code == 2 and word in capsys.readouterr().err, bad
