"""K35: normals and curvature of the thinned cloud — the definition against a float64 brute force, known answers, the
edge cases, the message, the driver and the flags."""
import numpy as np
import pytest

from test_range2d import _Engine, _rig_messages
from test_voxel_downsample import RIG, _wanted
from triton_client_amd.ops import voxel_downsample as V
from triton_client_amd.ros import compat, msgs, rosmsg

F = np.float32
OPTS = V.VoxelOptions(leaf=0.2, normal_radius=0.5)
ANGLE, CURV = 4 * 2.7e-5, 4 * 2.7e-6  # radians, curvature: four times the worst measured here (docs/precision.md)
# name -> (plane normals, offsets along them, noise, options, the share of voxels ``odd | flat`` may leave out)
SCENES = {"through_origin": ([(0.3, -0.2, 1.0)], [0.0], 0.01, OPTS, 0.05),
          "off_origin": ([(0.5, 0.4, 1.0)], [-2.0], 0.01, OPTS, 0.05),
          "anisotropic": ([(-0.2, 1.0, 0.3)], [3.0], 0.01, V.VoxelOptions(leaf=(0.2, 0.15, 0.25), normal_radius=0.6), 0.05),
          "edge": ([(0.0, 0.1, 1.0), (1.0, 0.0, 0.2)], [-1.5, 2.0], 0.01, OPTS, 0.25)}


def planes(normals, offsets, noise, seed=5, n=6000, side=4.0):
    """``n`` points of square patches of the planes ``n . p = offset`` around (1, 2, 0), with Gaussian noise
    along the normal; two planes are cut at their edge, each to the side where it is the lower."""
    rng, out = np.random.default_rng(seed), []
    for nrm, off in zip(normals, offsets):
        nrm = np.asarray(nrm, np.float64) / np.linalg.norm(nrm)
        u = np.cross(nrm, [1.0, 0.0, 0.0] if abs(nrm[0]) < 0.9 else [0.0, 1.0, 0.0])
        u /= np.linalg.norm(u)
        st = rng.uniform(-side / 2, side / 2, (n // len(normals), 2))
        base = np.array([1.0, 2.0, 0.0])
        base = base + (off - nrm @ base) * nrm
        out.append(base + st[:, :1] * u + st[:, 1:] * np.cross(nrm, u) + rng.normal(0, noise, (len(st), 1)) * nrm)
    if len(out) == 2:
        (na, oa), (nb, ob) = ((np.asarray(v, np.float64) / np.linalg.norm(v), o) for v, o in zip(normals, offsets))
        out = [out[0][out[0] @ nb <= ob], out[1][out[1] @ na <= oa]]
    return np.concatenate(out).astype(F)


@pytest.fixture(scope="module")
def solved():
    """Per scene: the rows, the definition's normals and the reference's answer, computed once."""
    res = {}
    for name, (nrm, off, noise, o, _) in SCENES.items():
        rows = V.downsample_numpy(planes(nrm, off, noise), o)
        res[name] = (rows, V.normals_numpy(rows, o), V.normals_ref(rows, o))
    return res


def angle(a, b):  # radians, row by row
    return np.arccos(np.clip((a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)), -1, 1))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_definition_against_the_reference(solved, name):
    rows, got, (ref, m, odd, flat) = solved[name]
    o, share = SCENES[name][3], SCENES[name][4]
    assert len(rows) > 300 and (odd | flat).mean() <= share  # a condition on the reference
    np.testing.assert_array_equal(V.moments_numpy(rows, o)[0][~odd], m[~odd])
    ok = ~(odd | flat)
    worst = angle(got[ok, :3].astype(np.float64), ref[ok, :3]).max(), np.abs(got[ok, 3] - ref[ok, 3]).max()
    print(name, "voxels", len(rows), "left out", (odd | flat).mean(), "angle", worst[0], "curvature", worst[1])
    assert worst[0] <= ANGLE and worst[1] <= CURV
    one_more = V.normals_numpy(rows, o, sweeps=V.SWEEPS + 1)  # the sweep count: one more changes no bit
    np.testing.assert_array_equal(one_more.view("<u4"), got.view("<u4"))


@pytest.mark.parametrize("nrm,off", [((0.3, -0.2, 1.0), 1.0), ((1.0, 0.0, 0.0), -3.0), ((0.0, 0.0, 1.0), 0.0)])
def test_a_noise_free_plane(nrm, off):
    rows = V.downsample_numpy(planes([nrm], [off], 0.0, n=3000, side=3.0), OPTS)
    got, (_, _, _, flat) = V.normals_numpy(rows, OPTS), V.normals_ref(rows, OPTS)
    unit = np.asarray(nrm, np.float64) / np.linalg.norm(nrm)
    n = got[~flat, :3].astype(np.float64)
    assert (~flat).sum() > 100 and (np.minimum(angle(n, unit[None]), angle(n, -unit[None])) <= ANGLE).all()
    assert ((n * rows[~flat, :3]).sum(1) <= 0).all() and (got[~flat, 3] <= CURV).all()  # towards the origin; flat


def test_edge_cases():
    lone = np.array([[0, 0, 0], [0.125, 0, 0], [5, 5, 5], [5.125, 5, 5], [5, 5.125, 5]], F)  # two neighbours, then three
    o = V.VoxelOptions(leaf=0.125, normal_radius=0.5)
    got, none = V.normals_numpy(lone, o), V.normals_numpy(np.zeros((0, 4), F), o)
    assert (got[:2].view("<u4") == 0x7FC00000).all() and not np.isnan(got[2:]).any() and none.shape == (0, 4)
    np.testing.assert_array_equal(got[2:], np.array([[0, 0, -1, 0]] * 3, F))  # the plane z = 5, seen from below
    ring = np.array([[0, 0, 0], [0.5, 0, 0], [0, -0.5, 0], [0, 0, 0.5], [0.375, 0.375, 0], [0.5, 0.125, 0]], F)
    assert V.moments_numpy(ring, o)[0].tolist() == [4, 4, 2, 2, 3, 3]  # the ball is closed: a pair at exactly R counts
    lam, vec = V.eigen_numpy(np.array([[1.0, 1e-30, 0.0, 3e30, 0.0, 2.0]], F))  # an infinite theta: t = 0, never a NaN
    assert lam.tolist() == [[1.0, float(F(3e30)), 2.0]] and (vec[0] == np.eye(3)).all()
    pts = planes(*SCENES["edge"][:3], n=3000)
    rows, mixed = V.downsample_numpy(pts, OPTS), V.downsample_numpy(pts[np.random.default_rng(1).permutation(len(pts))], OPTS)
    a, b = (np.concatenate([r, V.normals_numpy(r, OPTS)], 1) for r in (rows, mixed))  # no row's bytes depend on the order
    np.testing.assert_array_equal(a[np.lexsort(a[:, :3].T)].view("<u4"), b[np.lexsort(b[:, :3].T)].view("<u4"))


@pytest.mark.parametrize("kw", [dict(normal_radius=0.01, leaf=0.01), dict(normal_radius=4.5, leaf=2), dict(normal_radius=0.19),
                                dict(normal_radius=0.81), dict(normal_radius=0.5, leaf=(0.1, 0.2, 0.2)),
                                dict(normal_radius=0.5, leaf=(0.2, 0.6, 0.2)), dict(normal_radius=float("nan")),
                                dict(normal_radius=-0.5), dict(normal_radius="0.5"), dict(normal_radius=True)])
def test_options_refuse(kw):
    with pytest.raises(ValueError, match="normal_radius"):
        V.VoxelOptions(**kw)


def test_options_message_and_driver():
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.ros.bus import TopicBus

    assert V.VoxelOptions().normal_radius == 0 and not V.VoxelOptions().normals and OPTS.normals and OPTS.radius_q == 32768
    assert all(V.VoxelOptions(**ok).normals for ok in (dict(normal_radius=0.2), dict(normal_radius=0.8), dict(leaf=RIG.leaf, normal_radius=1)))
    clouds, _ = _rig_messages()
    on = V.VoxelOptions(leaf=RIG.leaf, min_points=2, normal_radius=1.0)
    op = V.VoxelDownsampler("cpu")
    assert op.messages(clouds, RIG) == _wanted(clouds)  # off: today's bytes
    rows = op.downsample(clouds, on)
    plain = V.downsample_cloud_numpy(clouds[0], RIG)
    assert rows[0].shape == (len(plain), 8) and rows[0][:, :4].tobytes() == plain.tobytes()
    assert rows[0][:, 4:].tobytes() == V.normals_numpy(plain, on).tobytes()
    m = V.downsample_message(clouds[0], rows[0])
    assert (m.point_step, m.row_step, m.width, m.data) == (32, 32 * len(plain), len(plain), rows[0].tobytes())
    assert [(f.name, f.offset, f.datatype, f.count) for f in m.fields[3:]] == [
        ("intensity", 12, 7, 1), ("normal_x", 16, 7, 1), ("normal_y", 20, 7, 1), ("normal_z", 24, 7, 1), ("curvature", 28, 7, 1)]
    assert m.is_dense == (not np.isnan(rows[0]).any()) and rosmsg.deserialize(rosmsg.serialize(m), "sensor_msgs/PointCloud2") == m
    assert not V.downsample_message(clouds[0], np.concatenate([plain[:2], np.tile(V.NAN_ROW, (2, 1))], 1)).is_dense

    bus, got = TopicBus(), []
    compat.Subscriber("/vox", msgs.PointCloud2, got.append, bus=bus)
    drv = RosInference3D(engine=_Engine(), params={"sub_topic": "/pc", "pub_topic": "/o"}, bus=bus, batch=4, workers=2,
                         queue_size=64, voxel_topic="/vox", voxel_options=dict(leaf=RIG.leaf, min_points=2, normal_radius=1.0))
    drv.start_inference(spin=False)
    pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
    for c in clouds:
        pub.publish(c)
    runner = drv.runner
    drv.stop(), bus.close()
    assert not runner.errors and got == [V.downsample_message(c, r) for c, r in zip(clouds, rows)] and drv.voxel_options == on


def test_flags_and_usage_errors(capsys):
    from triton_client_amd.cli import bag3d, main3d

    for mod, pre in ((main3d, []), (bag3d, ["--bag", "x"])):
        assert mod.parse_args(pre + ["--voxel-topic", "/v", "--voxel-normals", "0.5"]).voxel_options == OPTS
        for bad, word in ((["--voxel-normals", "0.5"], "--voxel-normals needs --voxel-topic TOPIC"),
                          (["--voxel-topic", "/v", "--voxel-normals", "0.1"], "error: --voxel-normals: normal_radius must lie between"),
                          (["--voxel-topic", "/v", "--voxel-leaf", "2", "--voxel-normals", "5"], "error: --voxel-normals: ")):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(pre + bad)
            assert e.value.code == 2 and word in capsys.readouterr().err, bad
