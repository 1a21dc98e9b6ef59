"""The LiDAR family table (config/lidar.py LIDAR_FAMILIES) against its readers: the served
voxel models, the local engine, the name matcher, and the request check all three served
models share."""
import dataclasses
import os

import numpy as np
import pytest
from google.protobuf import text_format

from triton_client_amd.config.lidar import (KITTI_SECOND_VOXELS, LIDAR_FAMILIES, NUSC_PILLARS, CenterPointConfig,
                                            SecondIoUConfig, lidar_family)
from triton_client_amd.ops.lidar import voxelize_np
from triton_client_amd.server.model import InferError
from triton_client_amd.server.models import VOXEL_MODELS, CenterPointModel, SecondIoUModel
from triton_client_amd.server.repository import FACTORIES, _family
from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def test_table_names_the_three_families():
    assert sorted(LIDAR_FAMILIES) == ["centerpoint", "pointpillars", "second_iou"] == sorted(VOXEL_MODELS)
    assert [(f.box_dim, f.label_base, f.point_features) for f in map(LIDAR_FAMILIES.get, (
        "pointpillars", "second_iou", "centerpoint"))] == [(7, 1, 4), (7, 1, 4), (9, 0, 5)]


@pytest.mark.parametrize("family", sorted(LIDAR_FAMILIES))
def test_table_matches_its_readers(family):
    from triton_client_amd.inference import LocalDetector3D

    fam = LIDAR_FAMILIES[family]
    assert fam.config().voxel.num_point_features == fam.point_features
    m = VOXEL_MODELS[family](device="cpu")
    assert type(m.cfg) is fam.config
    dims = {t.name: list(t.dims) for t in m.outputs() + m.inputs()}
    assert dims["pred_boxes"] == [-1, fam.box_dim]
    assert dims["voxels"] == [-1, m.cfg.voxel.max_points_per_voxel, fam.point_features]
    eng = LocalDetector3D(family=family, device="cpu")
    assert (eng.box_dim, eng.label_base, eng.z_offset) == (fam.box_dim, fam.label_base, fam.z_offset)
    assert eng.family == family and type(eng.cfg) is fam.config and eng.names == list(eng.cfg.class_names)
    assert eng.calibrate_target == fam.calibrate_target == m.calibrate_target
    # the shared load() passes the record's z offset: it is the pipeline constructor's own default
    import inspect
    assert inspect.signature(fam.pipeline_cls().__init__).parameters["z_offset"].default == fam.z_offset


def test_local_pointpillars_cpu_keeps_its_results():
    """The local PointPillars engine on the CPU (voxeliser, CPU head calibration, the served
    model's CPU path) against its results from before every family went through the served
    class: same boxes, scores within fp32 rounding of another host's BLAS."""
    from triton_client_amd.config.lidar import KITTI_PILLARS, PointPillarsConfig
    from triton_client_amd.inference import LocalDetector3D
    from triton_client_amd.ros import compat

    want = np.load(os.path.join(GOLDEN, "local_pointpillars_cpu.npz"))
    v = dataclasses.replace(KITTI_PILLARS, point_cloud_range=(0.0, -12.8, -3.0, 25.6, 12.8, 1.0), max_voxels=4000)
    eng = LocalDetector3D(cfg=PointPillarsConfig(voxel=v), device="cpu", calibrate_target=200.0)
    for seed in (1, 2):
        pts = lidar_sweep(LidarSpec(rings=16, azimuth_steps=256, sensor_height=3.23), seed)
        p = eng.detect([compat.create_cloud_xyzi(np.frombuffer(pts.tobytes(), np.float32).reshape(-1, 4))])[0]
        assert p["pred_boxes"].shape == want[f"pred_boxes_{seed}"].shape and len(p["pred_scores"]) > 10
        np.testing.assert_array_equal(p["pred_labels"], want[f"pred_labels_{seed}"])
        np.testing.assert_allclose(p["pred_scores"], want[f"pred_scores_{seed}"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(p["pred_boxes"], want[f"pred_boxes_{seed}"], rtol=1e-5, atol=1e-5)
    assert eng.calibrate_target is None  # calibrated once, on the first cloud


def test_unknown_family_is_refused_with_the_list():
    from triton_client_amd.inference import LocalDetector3D

    with pytest.raises(ValueError, match=r"\['centerpoint', 'pointpillars', 'second_iou'\]"):
        LocalDetector3D(family="voxelnet", device="cpu")


NAMES = [  # (model name, family): every LiDAR name in FACTORIES, the reference's -m values, a nuScenes name
    ("pointpillar_kitti", "pointpillars"), ("pointpillar_python", "pointpillars"), ("centerpoint_pp", "centerpoint"),
    ("centerpoint", "centerpoint"), ("second_iou", "second_iou"), ("SECOND_IoU", "second_iou"),
    ("nusc_pp_10sweep", "centerpoint"), ("my_pillars", "pointpillars"),
]


def test_name_resolution():
    for name, family in NAMES:
        assert lidar_family(name) == family and lidar_family(name, default=None) == family, name
        assert _family(name) == family, name
    lidar = {n for n in FACTORIES if lidar_family(n, default=None)}
    assert lidar == {"pointpillar_kitti", "pointpillar_python", "centerpoint_pp", "centerpoint", "second_iou"}
    assert lidar <= {n for n, _ in NAMES}
    for n in lidar:
        assert type(FACTORIES[n](device="cpu")) is VOXEL_MODELS[lidar_family(n)]
    # a camera name is no LiDAR family; the repository's camera rules come first
    assert lidar_family("YOLOv5nCOCO", default=None) is None and _family("YOLOv5nCOCO") == "yolo"
    assert _family("test_model") == "detectron" and _family("YOLOv4") == "yolov4"
    # an unknown name: the CLIs' default family, or the caller's
    assert lidar_family("voxelnet") == "pointpillars"
    assert lidar_family("voxelnet", default=None) is None and _family("voxelnet") is None
    assert lidar_family("voxelnet", default="second_iou") == "second_iou"
    from triton_client_amd.cli import engines
    assert engines.lidar_family is lidar_family


@pytest.mark.parametrize("name", ["pointpillar_kitti", "second_iou", "centerpoint_pp"])
def test_served_config_keeps_its_bytes(name):
    """config.pbtxt text of the served models as written before the models shared a base."""
    with open(os.path.join(GOLDEN, f"served_config_{name}.pbtxt")) as f:
        want = f.read()
    assert text_format.MessageToString(FACTORIES[name](device="cpu").config()) == want


# ------------------------------------------------------------------ refused requests
def _centerpoint():
    v = dataclasses.replace(NUSC_PILLARS, point_cloud_range=(-12.8, -12.8, -5.0, 12.8, 12.8, 3.0), max_voxels=4000)
    cfg = CenterPointConfig(voxel=v, score_thresh=0.0, nms_pre_max=16, nms_post_max=4)
    return CenterPointModel("centerpoint_pp", cfg=cfg, device="cpu"), LidarSpec(rings=16, azimuth_steps=256,
                                                                                 sensor_height=1.8), 0.0


def _second():
    v = dataclasses.replace(KITTI_SECOND_VOXELS, point_cloud_range=(0.0, -12.8, -3.0, 25.6, 12.8, 1.0),
                            max_voxels=16000)
    cfg = SecondIoUConfig(voxel=v, score_thresh=0.0)
    return SecondIoUModel("second_iou", cfg=cfg, device="cpu"), LidarSpec(rings=16, azimuth_steps=256,
                                                                          sensor_height=3.23), 1.5


@pytest.fixture(scope="module", params=[_centerpoint, _second], ids=["centerpoint", "second_iou"])
def served(request):
    """(loaded CPU model, one well-formed request): built once per family, never modified."""
    m, spec, zoff = request.param()
    m.load()
    p = lidar_sweep(spec, 3)
    p = p[~np.isnan(p).any(1)]
    p[:, 2] += zoff
    v, zyx, num, _ = voxelize_np(p, m.cfg.voxel, 4)
    coords = np.concatenate([np.zeros((len(zyx), 1), np.int32), zyx.astype(np.int32)], 1)
    return m, {"voxels": v, "voxel_coords": coords, "voxel_num_points": num.astype(np.int32)}


def test_well_formed_request_is_answered(served):
    m, ok = served
    out = m.execute(ok, None)
    n = len(out["pred_scores"])
    assert n > 0 and out["pred_boxes"].shape == (n, m.fam.box_dim) and out["pred_labels"].shape == (n,)


def test_malformed_requests_are_refused(served):
    """The corruptions of test_check_voxel_inputs_rejects_out_of_range_cells and a coordinate
    row too few, through execute: the check runs before the device branch, so the CPU model
    passes the line that guards the GPU path's canvas writes."""
    m, ok = served
    nx, ny, nz = m.cfg.voxel.grid_size
    P = m.cfg.voxel.max_points_per_voxel
    assert len(ok["voxels"]) > 4 and (nz == 1 or type(m) is SecondIoUModel)
    for key, idx, val in (("voxel_coords", (2, 3), nx), ("voxel_coords", (1, 2), -1), ("voxel_coords", (0, 1), nz),
                          ("voxel_num_points", (3,), 0), ("voxel_num_points", (4,), P + 1)):
        bad = {k: v.copy() for k, v in ok.items()}
        bad[key][idx] = val
        with pytest.raises(InferError):
            m.execute(bad, None)
    short = dict(ok, voxel_coords=ok["voxel_coords"][:-1])
    with pytest.raises(InferError, match="voxel_coords must be"):
        m.execute(short, None)
