"""K34: the voxel-grid downsample — the options, hand-made facts, the definition against a float64 brute force, the
message, the drivers and the CLI."""
import numpy as np
import pytest

from test_occupancy_grid import scene
from test_range2d import _Engine, _rig_messages
from triton_client_amd.ops import voxel_downsample as V
from triton_client_amd.ros import compat, msgs, rosmsg

F = np.float32
LEAVES = (0.01, 0.2, (0.5, 0.25, 1.0), 100)
RIG = V.VoxelOptions(leaf=(0.5, 0.25, 1.0), min_points=2)


def cloud(seed, n):
    """Two of the grid test's scenes joined, cut to ``n`` points, with a seeded intensity."""
    pts = np.concatenate([scene(seed), scene(seed + 100)])[:n]
    return np.concatenate([pts, np.random.default_rng(seed).uniform(0, 255, (len(pts), 1)).astype(F)], 1)


@pytest.mark.parametrize("kw", [dict(leaf=0.001), dict(leaf=101), dict(leaf=float("nan")), dict(leaf=True), dict(leaf="0.2"),
                                dict(leaf=(0.2, 0.2)), dict(leaf=(0.2, 0.2, 0.2, 0.2)), dict(leaf=(0.2, 0.001, 0.2)),
                                dict(min_points=0), dict(min_points=1.5)])
def test_options_refuse(kw):
    with pytest.raises(ValueError, match="leaf" if "leaf" in kw else "min_points"):
        V.VoxelOptions(**kw)


def test_hand_made_facts():
    o = V.VoxelOptions()
    assert o.leaf == (0.2, 0.2, 0.2) and V.VoxelOptions(leaf=[1, 2, 3]).leaf == (1.0, 2.0, 3.0)
    assert (V.slots_for(0), V.slots_for(1), V.slots_for(4096), V.slots_for(120000)) == (2, 2, 8192, 262144)
    assert V.most_clouds(120000) == 64 and V.most_clouds(2 ** 20) == 10
    pts = np.array([[-0.0625, 0.125, 0.125, 10], [0.0625, 0.125, 0.125, 20]], F)  # floor, not truncation: two voxels
    np.testing.assert_array_equal(V.downsample_numpy(pts, o), pts)  # (multiples of 2^-16 come back as they are)
    assert abs(float(V.downsample_numpy(np.array([[0.05, 0, 0]], F), o)[0, 0]) - 0.05) <= 2.0 ** -17
    edge = np.array([[3 * F(0.2), 0.1, 0.1, 1], [3 * F(0.2) - F(1e-6), 0.1, 0.1, 3]], F)  # exactly k * leaf: voxel k
    key, valid = V.keys_numpy(edge, o)
    assert valid.all() and ((key & (2 ** 21 - 1)) - V.BIAS).tolist() == [3, 2]
    odd = np.array([[np.nan, 0, 0, 1], [600, 0, 0, 1], [0, -np.inf, 0, 1], [0, 0, 512.5, 1], [512, -512, 0.125, np.nan],
                    [512, -512, 0.125, 7]], F)  # NaN, out of range: no voxel; a NaN intensity counts as 0
    np.testing.assert_array_equal(V.downsample_numpy(odd, o), np.array([[512, -512, 0.125, 3.5]], F))
    assert V.downsample_numpy(odd[:4], o).shape == (0, 4) and V.downsample_numpy(np.zeros((0, 3), F), o).shape == (0, 4)
    assert V.downsample_numpy(odd[4:, :3], o)[0, 3] == 0  # no intensity column
    pair = np.array([[5.015625, 0, 0, 1], [1.015625, 1.25, 1.25, 1], [5.046875, 0, 0, 3], [1.03125, 1.25, 1.25, 1],
                     [1.0625, 1.25, 1.25, 1], [-3.015625, 0, 0, 9]], F)
    three = V.downsample_numpy(pair, V.VoxelOptions(min_points=3))  # the pair at x = 5 and the single point are dropped
    np.testing.assert_array_equal(three, np.array([[F(3.109375 / 3), 1.25, 1.25, 1]], F))  # one float64 division, one rounding
    rows = V.downsample_numpy(pair, o)  # in the order of the voxels' first points, not of their keys
    assert rows[:, 0].tolist() == [5.03125, float(F(3.109375 / 3)), -3.015625] and rows[0, 3] == 2
    with pytest.raises(ValueError, match="points"):
        V.downsample_numpy(np.zeros((2 ** 24 + 1, 3), F), o)


@pytest.mark.parametrize("leaf", LEAVES)
def test_definition_against_the_reference(leaf):
    pts, o = cloud(40, 5000), V.VoxelOptions(leaf=leaf)
    assert len(pts) == 5000
    rows = V.downsample_numpy(pts, o)
    ref, keys, band = V.downsample_ref(pts, o)
    assert ref.shape == (len(keys), 4) and ref.dtype == np.float64
    got_keys, got_n = np.unique(V.keys_numpy(pts, o)[0], return_counts=True)
    ref_keys, ref_n = np.unique(V.keys_ref(pts, o)[0], return_counts=True)
    clean = ~np.isin(keys, band)
    assert (~clean).mean() <= 0.01  # a condition on the reference: the band may leave out at most 1 % of the voxels
    a, b = ~np.isin(got_keys, band), ~np.isin(ref_keys, band)
    np.testing.assert_array_equal(got_keys[a], ref_keys[b])
    np.testing.assert_array_equal(got_n[a], ref_n[b])
    key, valid = V.keys_numpy(pts, o)
    uniq, first = np.unique(key[valid], return_index=True)
    _, i, j = np.intersect1d(uniq[np.argsort(first)], keys[clean], return_indices=True)  # the rows' keys, in their order
    assert rows.dtype == F and len(rows) == len(uniq) and len(i) == clean.sum() > 0
    ref = ref[clean][j]
    half_ulp = np.spacing(np.abs(ref).astype(F)).astype(np.float64) / 2
    tol = np.array([2.0 ** -17] * 3 + [2.0 ** -13]) + half_ulp  # the quantisation's half unit, then the final rounding
    assert (np.abs(rows[i].astype(np.float64) - ref) <= tol).all()
    order = np.random.default_rng(3).permutation(len(pts))  # no sum depends on the order of the points
    shuffled = V.downsample_numpy(pts[order], o)
    np.testing.assert_array_equal(shuffled[np.lexsort(shuffled.T)], rows[np.lexsort(rows.T)])
    assert len(rows) == {0.01: 4999, 100: 7}.get(leaf, len(rows))


def test_the_message():
    c = _rig_messages()[0][0]
    rows = V.downsample_cloud_numpy(c, RIG)
    m = V.downsample_message(c, rows)
    assert 0 < len(rows) < 300 and m.header == c.header and (m.height, m.width, m.point_step, m.row_step) == (1, len(rows), 16, 16 * len(rows))
    assert [(f.name, f.offset, f.datatype, f.count) for f in m.fields] == [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1), ("intensity", 12, 7, 1)]
    assert m.data == rows.tobytes() and m.is_dense and not m.is_bigendian
    bare = msgs.PointCloud2(header=c.header, height=1, width=c.width, fields=[f for f in c.fields if f.name != "intensity"],
                            is_bigendian=False, point_step=16, row_step=c.row_step, data=c.data, is_dense=True)
    thin = V.downsample_message(bare, V.downsample_cloud_numpy(bare, RIG))  # the dword is there, the field is not
    assert [f.name for f in thin.fields] == ["x", "y", "z"] and thin.point_step == 16 and len(thin.data) == len(m.data)
    assert rosmsg.deserialize(rosmsg.serialize(m), "sensor_msgs/PointCloud2") == m


def _wanted(clouds, opts=RIG):
    return [V.downsample_message(c, V.downsample_cloud_numpy(c, opts)) for c in clouds]


def test_driver_publishes_the_voxels_last_and_keeps_every_other_byte(monkeypatch, tmp_path):
    from triton_client_amd.inference import BagInference3D, RosInference3D
    from triton_client_amd.inference import ros_inference3d as M
    from triton_client_amd.parallel.dp import DataParallelDetector3D
    from triton_client_amd.ros.bag import Bag
    from triton_client_amd.ros.bus import TopicBus

    assert M.EVERY_MESSAGE == M.EVERY_OUTPUT + M.FILTERED_OUTPUTS == M.EVERY_OUTPUT + (("voxels", msgs.PointCloud2),)
    clouds, _ = _rig_messages()
    want = _wanted(clouds)

    def drive(on):
        bus, seen, order, got = TopicBus(), {"/o": [], "/grid": [], "/gnd": []}, [], []
        for t, ty in (("/o", msgs.BoundingBoxArray), ("/grid", msgs.OccupancyGrid), ("/gnd", msgs.PointCloud2)):
            compat.Subscriber(t, ty, lambda m, t=t: seen[t].append(rosmsg.serialize(m)), bus=bus)
        compat.Subscriber("/vox", msgs.PointCloud2, got.append, bus=bus)
        kw = dict(voxel_topic="/vox", voxel_options=dict(leaf=RIG.leaf, min_points=2)) if on else {}
        drv = RosInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=4, workers=2,
                             queue_size=64, ground_topic="/gnd", grid_topic="/grid", **kw)
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
    assert got == want and drv.voxel_options == RIG and order == ["ground", "grid", "voxels"] * 4
    off_seen, off_got, _, _ = drive(False)
    assert off_got == [] and off_seen == seen  # every other message keeps its bytes
    res = RosInference3D(engine=_Engine(), params={}).process(clouds)
    assert all(r.voxels is None and "voxels" not in r.pred for r in res)
    assert RosInference3D(engine=_Engine(), params={}, voxel_topic="/v").voxel_options == V.VoxelOptions()
    with pytest.raises(ValueError, match="leaf"):
        RosInference3D(engine=_Engine(), params={}, voxel_topic="/v", voxel_options={"leaf": 0})
    ring = object.__new__(DataParallelDetector3D)  # (no ranks are started: the refusal reads a class attribute)
    with pytest.raises(ValueError, match="ring"):
        RosInference3D(engine=ring, params={}, voxel_topic="/v")

    src, dst = str(tmp_path / "in.bag"), str(tmp_path / "out.bag")
    with Bag(src, "w") as bag:
        for c in clouds:
            bag.write("/pc", c)
    bagged = BagInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bagfile=src, out_bag=dst, batch=3,
                            voxel_topic="/vox", voxel_options=RIG)
    assert bagged.start_inference() == 4
    with Bag(dst) as bag:
        assert [t for t, _, _ in bag.read_messages()] == ["/pc", "/o", "/vox"] * 4
        assert [m for _, m, _ in bag.read_messages(topics=["/vox"])] == want


def test_flags_and_usage_errors(capsys):
    from triton_client_amd.cli import bag3d, main3d

    for mod, pre in ((main3d, []), (bag3d, ["--bag", "x"])):
        f = mod.parse_args(pre)
        assert f.voxel_topic == "" and f.voxel_options is None
        assert mod.parse_args(pre + ["--voxel-topic", "/v"]).voxel_options == V.VoxelOptions()
        f = mod.parse_args(pre + ["--voxel-topic", "/v", "--voxel-leaf", "0.5,0.25,1", "--voxel-min-points", "2"])
        assert f.voxel_options == RIG and mod.parse_args(pre + ["--voxel-topic", "/v", "--voxel-leaf", "0.1"]).voxel_options.leaf == (0.1,) * 3
        for bad, word in ((["--voxel-leaf", "1"], "--voxel-leaf needs --voxel-topic TOPIC"),
                          (["--voxel-min-points", "2"], "--voxel-min-points needs --voxel-topic TOPIC"),
                          (["--voxel-topic", "/v", "--voxel-leaf", "1,2"], "error: --voxel-leaf: want L or LX,LY,LZ"),
                          (["--voxel-topic", "/v", "--voxel-leaf", "0.001"], "error: --voxel-leaf: "),
                          (["--voxel-topic", "/v", "--voxel-min-points", "0"], "error: --voxel-min-points: ")):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(pre + bad)
            assert e.value.code == 2 and word in capsys.readouterr().err, bad
