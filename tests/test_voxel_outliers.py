"""K36: outlier removal on the thinned cloud — the options, known answers, the definition against a float64 brute
force, the message, the driver and the flags."""
import numpy as np
import pytest

from test_range2d import _Engine, _rig_messages
from test_voxel_downsample import RIG
from triton_client_amd.ops import voxel_downsample as V
from triton_client_amd.ros import compat, msgs, rosmsg

F = np.float32
ROR = dict(outlier_radius=0.5, outlier_min_neighbors=3)
# name -> (leaf, radius, what is added to every coordinate)
SCENES = {"plain": (0.2, 0.5, (0.0, 0.0, 0.1)), "negative_anisotropic": ((0.2, 0.25, 0.15), 0.6, (-10.0, -7.0, -2.9))}
TESTS = {"ror3": dict(outlier_min_neighbors=3), "sor1": dict(outlier_mean_k=1), "sor5": dict(outlier_mean_k=5),
         "sor16": dict(outlier_mean_k=16), "both": dict(outlier_min_neighbors=3, outlier_mean_k=5)}


def scene(shift, seed=11, n=9000):
    """A ground plane of 8 m x 8 m with 2 cm of noise, a wall of 4 m x 2 m on it and 3 % of the points uniform in
    the box around both."""
    rng = np.random.default_rng(seed)
    ground = np.concatenate([rng.uniform(-4, 4, (n, 2)), rng.normal(0, 0.02, (n, 1))], 1)
    wall = np.stack([np.full(n // 6, 3.0) + rng.normal(0, 0.02, n // 6), rng.uniform(-2, 2, n // 6), rng.uniform(0, 2, n // 6)], 1)
    noise = rng.uniform((-4, -4, -1), (4, 4, 3), (3 * (n + n // 6) // 100, 3))
    return (rng.permutation(np.concatenate([ground, wall, noise])) + np.asarray(shift)).astype(F)


@pytest.fixture(scope="module")
def solved():
    """Per scene and test: the rows, the options, the definition's scores and the reference's, computed once."""
    res = {}
    for name, (leaf, r, shift) in SCENES.items():
        rows = V.downsample_numpy(scene(shift), V.VoxelOptions(leaf=leaf))
        for t, kw in TESTS.items():
            o = V.VoxelOptions(leaf=leaf, outlier_radius=r, **kw)
            res[name, t] = (rows, o, V.outlier_scores_numpy(rows, o), V.outlier_scores_ref(rows, o))
    return res


@pytest.mark.parametrize("t", sorted(TESTS))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_definition_against_the_reference(solved, name, t):
    rows, o, (found, mean, thr), (rfound, rmean, rthr, band) = solved[name, t]
    keep, (ref, odd) = V.outliers_numpy(rows, o), V.outliers_ref(rows, o)
    assert 1800 <= len(rows) <= 2400 and odd.mean() <= 0.05  # a condition on the reference
    np.testing.assert_array_equal(found[~band], rfound[~band])
    if o.outlier_mean_k:  # what docs/precision.md records, in metres
        print(name, t, "mean", np.abs(mean / V.QC - rmean)[~band].max(), "thr", abs(thr / V.QC - rthr), "odd", odd.mean())
        assert np.abs(mean / V.QC - rmean)[~band].max() + abs(thr / V.QC - rthr) <= V.OUTLIER_MARGIN / 4
    np.testing.assert_array_equal(keep[~odd], ref[~odd])
    assert 0.01 <= (~keep).mean() <= 0.2  # the noise goes, the surfaces stay


def test_known_answers():
    slab = np.stack(np.meshgrid(np.arange(5), np.arange(5), [0], indexing="ij"), -1).reshape(-1, 3).astype(F) * F(0.25)
    rows = np.concatenate([slab, [[9, 9, 9]], [[1.25, 0, 0]]]).astype(F)  # a far voxel, and one next to the corner (1, 0, 0)
    o = lambda **kw: V.VoxelOptions(leaf=0.25, outlier_radius=0.25, **kw)
    found, _, _ = V.outlier_scores_numpy(rows, o(outlier_min_neighbors=1))
    assert found.tolist() == [2, 3, 3, 3, 2, 3, 4, 4, 4, 3, 3, 4, 4, 4, 3, 3, 4, 4, 4, 3, 3, 3, 3, 3, 2, 0, 1]  # a closed ball
    assert np.nonzero(~V.outliers_numpy(rows, o(outlier_min_neighbors=1)))[0].tolist() == [25]
    assert np.nonzero(~V.outliers_numpy(rows, o(outlier_min_neighbors=2)))[0].tolist() == [25, 26]
    # every nearest neighbour at 0.25 m exactly: no variance, the threshold is the mean, only the far voxel goes
    found, mean, thr = V.outlier_scores_numpy(rows, o(outlier_mean_k=1, outlier_stddev=0.0))
    assert mean.tolist() == [16384] * 25 + [0, 16384] and thr == 16384.0
    assert np.nonzero(~V.outliers_numpy(rows, o(outlier_mean_k=1, outlier_stddev=0.0)))[0].tolist() == [25]
    pair = np.array([[0, 0, 0], [0.25, 0.125, 0]], F)  # n = 2: both means equal, both kept; then n = 1 and n = 0
    k1 = o(outlier_mean_k=1, outlier_stddev=0.0)
    assert V.outliers_numpy(pair * F(0.8), k1).tolist() == [True, True] and V.outlier_scores_numpy(pair * F(0.8), k1)[2] < np.inf
    assert V.outliers_numpy(pair, k1).tolist() == [False, False] and V.outliers_numpy(pair[:1], k1).tolist() == [False]
    three = np.array([[0, 0, 0], [0.25, 0, 0], [9, 9, 9]], F)
    assert V.outlier_scores_numpy(three, k1)[2] < np.inf and V.outliers_numpy(three, k1).tolist() == [True, True, False]
    assert V.outliers_numpy(np.zeros((0, 4), F), k1).shape == (0,)


BAD = [("outlier_radius", dict(outlier_radius=0.5)), ("outlier_min_neighbors", dict(outlier_min_neighbors=2)),
       ("outlier_mean_k", dict(outlier_mean_k=5)), ("outlier_radius", dict(outlier_radius=0.19, outlier_mean_k=5)),
       ("outlier_radius", dict(outlier_radius=0.81, outlier_mean_k=5)), ("outlier_radius", dict(outlier_radius=-1, outlier_mean_k=5)),
       ("outlier_radius", dict(outlier_radius=4.5, leaf=2, outlier_mean_k=5)), ("outlier_radius", dict(outlier_radius="0.5")),
       ("outlier_min_neighbors", dict(outlier_radius=0.5, outlier_min_neighbors=1001)),
       ("outlier_min_neighbors", dict(outlier_radius=0.5, outlier_min_neighbors=-1)),
       ("outlier_min_neighbors", dict(outlier_radius=0.5, outlier_min_neighbors=2.0)),
       ("outlier_mean_k", dict(outlier_radius=0.5, outlier_mean_k=17)), ("outlier_mean_k", dict(outlier_radius=0.5, outlier_mean_k=True)),
       ("outlier_stddev", dict(outlier_radius=0.5, outlier_mean_k=5, outlier_stddev=-0.1)),
       ("outlier_stddev", dict(outlier_radius=0.5, outlier_mean_k=5, outlier_stddev=10.5)),
       ("outlier_stddev", dict(outlier_stddev=float("nan")))]


@pytest.mark.parametrize("field,kw", BAD)
def test_options_refuse(field, kw):
    with pytest.raises(ValueError, match="^" + field + " "):
        V.VoxelOptions(**kw)


def test_options_message_and_driver():
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.ros.bus import TopicBus

    off = V.VoxelOptions()
    assert (off.outlier_radius, off.outlier_min_neighbors, off.outlier_mean_k, off.outlier_stddev) == (0, 0, 0, 1.0)
    assert not off.outliers and off == V.VoxelOptions(leaf=0.2, min_points=1, normal_radius=0.0)
    assert V.VoxelOptions(**ROR).outliers and V.VoxelOptions(**ROR).outlier_radius_q == 32768
    clouds, _ = _rig_messages()
    kw = dict(leaf=RIG.leaf, min_points=2, normal_radius=1.0, outlier_radius=1.0, outlier_min_neighbors=4, outlier_mean_k=3)
    on, op = V.VoxelOptions(**kw), V.VoxelDownsampler("cpu")
    rows, plain = op.downsample(clouds, on), V.downsample_cloud_numpy(clouds[0], RIG)
    keep = V.outliers_numpy(plain, on)
    assert 0 < keep.sum() < len(plain) and rows[0][:, :4].tobytes() == plain[keep].tobytes()
    assert rows[0][:, 4:].tobytes() == V.normals_numpy(plain[keep], on).tobytes()  # the normals of the filtered cloud
    wanted = [V.downsample_message(c, r) for c, r in zip(clouds, rows)]
    assert wanted[0].point_step == 32 and wanted[0].width == keep.sum() and op.messages(clouds, on) == wanted

    def drive(voxel_options):
        bus, got = TopicBus(), {"/o": [], "/grid": [], "/gnd": [], "/vox": []}
        for t, ty in (("/o", msgs.BoundingBoxArray), ("/grid", msgs.OccupancyGrid), ("/gnd", msgs.PointCloud2), ("/vox", msgs.PointCloud2)):
            compat.Subscriber(t, ty, lambda m, t=t: got[t].append(m if t == "/vox" else rosmsg.serialize(m)), bus=bus)
        drv = RosInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=4, workers=2,
                             queue_size=64, ground_topic="/gnd", grid_topic="/grid", voxel_topic="/vox", voxel_options=voxel_options)
        drv.start_inference(spin=False)
        pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
        for c in clouds:
            pub.publish(c)
        runner = drv.runner
        drv.stop(), bus.close()
        assert not runner.errors and drv.voxel_options == V.VoxelOptions(**voxel_options)
        return got

    filtered, unfiltered = drive(kw), drive(dict(leaf=RIG.leaf, min_points=2, normal_radius=1.0))
    assert filtered["/vox"] == wanted and filtered["/vox"] != unfiltered["/vox"]
    assert all(len(filtered[t]) == len(clouds) and filtered[t] == unfiltered[t] for t in ("/o", "/grid", "/gnd"))  # every other topic


def test_flags_and_usage_errors(capsys):
    from triton_client_amd.cli import bag3d, main3d

    flags = ["--voxel-outlier-radius", "0.5", "--voxel-outlier-neighbors", "3", "--voxel-outlier-mean-k", "5", "--voxel-outlier-stddev", "2"]
    want = V.VoxelOptions(outlier_radius=0.5, outlier_min_neighbors=3, outlier_mean_k=5, outlier_stddev=2.0)
    for mod, pre in ((main3d, []), (bag3d, ["--bag", "x"])):
        assert mod.parse_args(pre + ["--voxel-topic", "/v"] + flags).voxel_options == want
        errors = [(flags[2 * j:2 * j + 2], flags[2 * j] + " needs --voxel-topic TOPIC") for j in range(4)] + [
            (["--voxel-topic", "/v"] + flags[:2], "error: --voxel-outlier-radius: outlier_radius needs a test"),
            (["--voxel-topic", "/v"] + flags[2:4], "error: --voxel-outlier-neighbors: outlier_min_neighbors needs outlier_radius"),
            (["--voxel-topic", "/v"] + flags[4:6], "error: --voxel-outlier-mean-k: outlier_mean_k needs outlier_radius"),
            (["--voxel-topic", "/v", "--voxel-outlier-radius", "0.1"] + flags[2:4], "error: --voxel-outlier-radius: outlier_radius must lie between"),
            (["--voxel-topic", "/v"] + flags[:2] + ["--voxel-outlier-mean-k", "17"], "error: --voxel-outlier-mean-k: outlier_mean_k must be an integer in 0..16"),
            (["--voxel-topic", "/v"] + flags[:6] + ["--voxel-outlier-stddev", "11"], "error: --voxel-outlier-stddev: outlier_stddev must lie within 0..10")]
        for bad, word in errors:
            with pytest.raises(SystemExit) as e:
                mod.parse_args(pre + bad)
            assert e.value.code == 2 and word in capsys.readouterr().err, bad
