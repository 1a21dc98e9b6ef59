"""K32: the oriented fit — the integer definition against a float64 brute force within its derived band on L-shaped
and full-outline objects, the rules of the definition, the box message, the options, the extractor and the engine."""
import dataclasses

import numpy as np
import pytest

from test_cluster import F as F32, GROUND, _Engine, _rig_messages, grid, place
from triton_client_amd.ops import cluster as C
from triton_client_amd.ops import cluster_fit as F
from triton_client_amd.ros import msgs, rosmsg

OPTS = C.ClusterOptions(remove_ground=False, min_points=1)
FIT = F.FitOptions(angles=90, d0=0.02)
CENTRE = (12.3, -7.1)
HDR = msgs.Header(seq=9, stamp=msgs.Time(3, 4), frame_id="os")


def outline(n, yaw_deg, full, seed=7):
    """The one input maker: a 4.2 x 1.8 m object at ``CENTRE``, its long side along the yaw: two edges (an L) or all
    four, ``n`` points evenly along them, 3 mm noise."""
    rng = np.random.default_rng(seed)
    corners = np.array([[2.1, -0.9], [-2.1, -0.9], [-2.1, 0.9], [2.1, 0.9], [2.1, -0.9]])[:5 if full else 3]
    at = np.concatenate([[0], np.cumsum(np.hypot(*np.diff(corners, axis=0).T))])
    t = (np.arange(n) + 0.5) / n * at[-1]
    p = np.stack([np.interp(t, at, corners[:, a]) for a in (0, 1)], 1) + rng.normal(0, 0.003, (n, 2))
    c, s = np.cos(np.deg2rad(yaw_deg)), np.sin(np.deg2rad(yaw_deg))
    p = p @ np.array([[c, s], [-s, c]]) + CENTRE
    return np.concatenate([p, rng.uniform(-1, 0.5, (n, 1))], 1).astype(F32)


def clustered(pts, opts=OPTS):
    found, label, table = C.cluster_numpy(pts, opts)
    return label, table


@pytest.mark.parametrize("yaw", [0, 1, 17, 44, 45, 89])
@pytest.mark.parametrize("n", [64, 300, 2500])
@pytest.mark.parametrize("full", [False, True], ids=["L", "outline"])
def test_definition_within_its_band_of_the_float64_brute_force(full, n, yaw):
    pts = outline(n, yaw, full)
    label, table = clustered(pts)
    assert len(table) == 1 and table["n"][0] == n
    score, bounds = F.scores_numpy(*F.centred(pts, label, table)[0], FIT)
    (ref,), (ref_bounds,) = F.fit_ref(pts, label, table, FIT)
    (band,), (edge,) = F.fit_band(table, FIT)
    assert (np.abs(score / 65536 - ref) <= n * band).all()
    assert (np.abs(bounds / 2 ** 24 - ref_bounds) <= edge).all()
    top = np.sort(ref)
    assert top[-1] - top[-2] > 2 * n * band  # the reference alone decides: the band cannot turn the order
    (row,) = F.fit_numpy(pts, label, table, FIT)
    assert row["j"] == np.argmax(ref) == yaw and row["flags"] == 0
    assert (row["score"], *(row[f] for f in ("u_min", "u_max", "v_min", "v_max"))) == (score[yaw], *bounds[yaw])
    assert F.fit_numpy(pts[::-1], label[::-1], table, FIT).tobytes() == row.tobytes()  # no order dependence


def test_a_point_a_line_and_an_oversize_cluster():
    o = grid(400, 40, min_points=1)
    line = np.stack([np.linspace(3, 6, 30), np.full(30, 7.2), np.zeros(30)], 1).astype(F32)
    wide = np.stack([np.linspace(10, 75.1, 218), np.full(218, 15.1), np.zeros(218)], 1).astype(F32)
    pts = np.concatenate([np.array([[1.2, 1.3, 0.5]], F32), line, wide])
    label, table = clustered(pts, o)
    assert table["n"].tolist() == [1, 30, 218] and table["max_x"][2] - table["min_x"][2] > F.MAX_SIDE
    fit = F.fit_numpy(pts, label, table, F.FitOptions())
    assert fit["j"].tolist() == [0, 0, 0] and fit["flags"].tolist() == [0, 0, F.OVERSIZE]
    assert fit[2].tobytes() == np.array([(0, 1, 0, 0, 0, 0, 0)], F.FIT_DTYPE).tobytes()
    assert fit["u_min"][0] == fit["u_max"][0] and fit["score"].tolist()[:2] == [65536, 30 * 65536]
    assert np.isnan(F.fit_ref(pts, label, table, F.FitOptions())[0][2]).all()
    for jsk in (True, False):  # an oversize row keeps the axis-aligned box, byte for byte
        assert rosmsg.serialize(F.fit_boxes(table[2:], fit[2:], HDR, jsk)) == \
            rosmsg.serialize(C.cluster_boxes(table[2:], HDR, jsk))


@pytest.mark.parametrize("pts", [place([(3, 3, 5)], 2) * F32(0.3), np.array([[5, 5, 0], [5.1, 5, 0], [5, 5.1, 0],
                                                                             [5.1, 5.1, 0]], F32)],
                         ids=["blob", "square"])
def test_saturated_scores_pick_the_smallest_area_then_the_smallest_direction(pts):
    o = F.FitOptions(angles=90, d0=0.1)
    label, table = clustered(pts)
    (row,) = F.fit_numpy(pts, label, table, o)
    (dx, dy), (c, s) = F.centred(pts, label, table)[0], F.directions(90)
    best = None
    for j in range(90):  # the rules in plain Python integers
        u = [int(x) * int(c[j]) + int(y) * int(s[j]) for x, y in zip(dx, dy)]
        v = [int(y) * int(c[j]) - int(x) * int(s[j]) for x, y in zip(dx, dy)]
        score = sum((o.d0q << 16) // max(min(a - min(u), max(u) - a, b - min(v), max(v) - b) >> 10, o.d0q)
                    for a, b in zip(u, v))
        key = (-score, (max(u) - min(u)) * (max(v) - min(v)), j)
        best = min(best or key, key)
        saturated = score == len(u) * 65536
        assert saturated or j  # direction 0 is saturated, and so are several others
    r = {f: int(row[f]) for f in F.FIT_DTYPE.names}
    assert (-r["score"], (r["u_max"] - r["u_min"]) * (r["v_max"] - r["v_min"]), r["j"]) == best
    assert row["score"] == len(pts) * 65536


@pytest.mark.parametrize("jsk", [True, False])
@pytest.mark.parametrize("full,yaw", [(False, 17), (True, 44), (False, 89), (True, 0)])
def test_box_message_has_the_objects_yaw_centre_and_extents(full, yaw, jsk):
    pts = outline(300, yaw, full)
    label, table = clustered(pts)
    fit = F.fit_numpy(pts, label, table, FIT)
    m = F.fit_boxes(table, fit, HDR, jsk, FIT)
    ref = C.cluster_boxes(table, HDR, jsk)
    assert m.header == HDR and type(m) is type(ref)
    (b,), (r,) = (m.boxes, ref.boxes) if jsk else (m.detections, ref.detections)
    pose, size = (b.pose, b.dimensions) if jsk else (b.bbox.center, b.bbox.size)
    got_yaw = 2 * np.arctan2(pose.orientation.z, pose.orientation.w)
    assert abs(got_yaw - np.deg2rad(yaw)) <= np.pi / 180 + 1e-12 and 0 <= got_yaw < np.pi
    assert abs(pose.position.x - CENTRE[0]) <= 0.02 and abs(pose.position.y - CENTRE[1]) <= 0.02
    assert abs(size.x - 4.2) <= 0.02 and abs(size.y - 1.8) <= 0.02  # the long side lies along the yaw
    rpose, rsize = (r.pose, r.dimensions) if jsk else (r.bbox.center, r.bbox.size)
    assert (pose.position.z, size.z) == (rpose.position.z, rsize.z)
    assert ((b.value, b.label) if jsk else (b.results[0].score, b.results[0].id)) == (300.0, 0)


def test_a_box_wider_than_long_is_turned_and_bad_tables_are_refused():
    table = np.zeros(1, C.TABLE_DTYPE)
    table[0] = (7, 40, 1024, 3073, -2048, -1024, 0, 512, 0, 0, 0, 0)  # cx = 2048 (floor), cy = -1536
    fit = np.array([(30, 0, -2 ** 24, 2 ** 24, -2 ** 25, 2 ** 26, 5)], F.FIT_DTYPE)
    (b,) = F.fit_boxes(table, fit, HDR, False, F.FitOptions(angles=90)).detections
    yaw = 2 * np.arctan2(b.bbox.center.orientation.z, b.bbox.center.orientation.w)
    assert np.isclose(yaw, np.pi / 6 + np.pi / 2) and (b.bbox.size.x, b.bbox.size.y) == (6.0, 2.0)
    assert np.allclose((b.bbox.center.position.x, b.bbox.center.position.y),
                       (2.0 - np.sin(np.pi / 6), -1.5 + np.cos(np.pi / 6)))
    for bad in (fit[:0], fit.astype([(n, "<i8") for n in F.FIT_DTYPE.names]), np.array([(90, 0, 0, 0, 0, 0, 0)], F.FIT_DTYPE),
                np.array([(0, 2, 0, 0, 0, 0, 0)], F.FIT_DTYPE), np.array([(-1, 0, 0, 0, 0, 0, 0)], F.FIT_DTYPE)):
        with pytest.raises(ValueError, match="^fit "):
            F.fit_boxes(table, bad, HDR, True, F.FitOptions(angles=90))


def test_options_and_their_refusals():
    o = F.FitOptions()
    assert (o.angles, o.d0, o.d0q) == (90, 0.1, 1638) and F.FitOptions(d0=1).d0q == 16384
    assert F.as_options(None) is None and F.as_options(o) is o and F.as_options({"angles": 45}) == F.FitOptions(45)
    c, s = F.directions(128)
    assert (c[0], s[0], c.dtype) == (16384, 0, np.int32) and c[64] == s[64] == 11585
    with pytest.raises(dataclasses.FrozenInstanceError):
        o.d0 = 1.0
    bad = {"angles": [dict(angles=1), dict(angles=129), dict(angles=90.0), dict(angles=True)],
           "d0": [dict(d0=0.009), dict(d0=1.01), dict(d0=np.nan), dict(d0=None)]}
    for field, cases in bad.items():
        for kw in cases:
            with pytest.raises(ValueError, match="^" + field):
                F.FitOptions(**kw)


def test_extractor_engine_and_driver_take_the_option():
    from triton_client_amd.inference import BagInference3D, RosInference3D
    from triton_client_amd.inference.engines import Detector3D

    clouds, _ = _rig_messages()
    o, fo = C.ClusterOptions(min_points=3), F.FitOptions(angles=30)
    ex = C.ClusterExtractor("cpu")
    want = []
    for c, got in zip(clouds, ex.extract(clouds, o, GROUND, fit=fo)):
        pts = C.obstacle_rows(C.cloud_xyzi(c), GROUND)
        found, label, table = C.cluster_numpy(pts, o)
        assert len(got) == 4 and got[3].tobytes() == F.fit_numpy(pts, label, table, fo).tobytes() and found >= 1
        want.append(rosmsg.serialize(F.fit_boxes(table, got[3], c.header, True, fo)))
    assert [len(r) for r in ex.extract(clouds, o, GROUND)] == [3] * len(clouds)  # without the option nothing changes
    assert [rosmsg.serialize(m) for m in ex.messages(clouds, o, GROUND, fit=fo)] == want
    assert [rosmsg.serialize(m) for m in Detector3D.cluster_obstacles(_Engine(), clouds, o, GROUND, fit=fo)] == want
    plain = [rosmsg.serialize(m) for m in Detector3D.cluster_obstacles(_Engine(), clouds, o, GROUND)]
    assert plain == [rosmsg.serialize(m) for m in ex.messages(clouds, o, GROUND)] and plain != want
    kw = dict(engine=_Engine(), params={}, clusters_topic="/c", cluster_options=o, ground_options=GROUND)
    for drv in (RosInference3D(cluster_fit={"angles": 30}, **kw), BagInference3D(cluster_fit=fo, **kw)):
        assert drv.cluster_fit == fo and [rosmsg.serialize(r.clusters) for r in drv.process(clouds)] == want
    off = RosInference3D(**kw)
    assert off.cluster_fit is None and [rosmsg.serialize(r.clusters) for r in off.process(clouds)] == plain
    for cls in (RosInference3D, BagInference3D):  # a bad option fails in the constructor
        with pytest.raises(ValueError, match="^angles"):
            cls(cluster_fit={"angles": 1}, **kw)
        with pytest.raises(ValueError, match="needs clusters_topic"):
            cls(engine=_Engine(), params={}, cluster_fit=fo)


def test_flags_and_usage_errors(capsys):
    from triton_client_amd.cli import bag3d, main3d

    for mod, pre in ((main3d, []), (bag3d, ["--bag", "x"])):
        assert mod.parse_args(pre + ["--clusters-topic", "/c"]).cluster_fit is None
        assert mod.parse_args(pre + ["--clusters-topic", "/c", "--cluster-oriented"]).cluster_fit == F.FitOptions()
        f = mod.parse_args(pre + ["--clusters-topic", "/c", "--cluster-oriented", "--cluster-fit-angles", "45",
                                  "--cluster-fit-d0", "0.05"])
        assert f.cluster_fit == F.FitOptions(45, 0.05)
        for bad, word in ((["--cluster-oriented"], "error: --cluster-oriented needs --clusters-topic"),
                          (["--clusters-topic", "/c", "--cluster-fit-angles", "45"],
                           "error: --cluster-fit-angles needs --cluster-oriented"),
                          (["--clusters-topic", "/c", "--cluster-fit-d0", "0.05"],
                           "error: --cluster-fit-d0 needs --cluster-oriented"),
                          (["--clusters-topic", "/c", "--cluster-oriented", "--cluster-fit-angles", "129"],
                           "error: --cluster-fit-angles: "),
                          (["--clusters-topic", "/c", "--cluster-oriented", "--cluster-fit-d0", "2"],
                           "error: --cluster-fit-d0: ")):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(pre + bad)
            assert e.value.code == 2 and word in capsys.readouterr().err, bad
