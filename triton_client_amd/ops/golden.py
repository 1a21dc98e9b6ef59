"""Golden (sequential, obviously-correct) NumPy references for every per-frame
op.  They re-state the reference's semantics — not its code — and are what
the HIP kernels and the vectorised CPU paths are tested against:

* ``resize_bilinear_u8``     — OpenCV INTER_LINEAR pixel-centre convention
  (reference ``communicator/ros_inference.py:140``, cv2 is not installed here,
  so bit-exactness with cv2's fixed point is "parity unpinned"; we match the
  float formula and round to uint8 like cv2's u8 output).
* ``letterbox_params``       — YOLOv5 letterbox geometry.
* ``nms_greedy``             — torchvision.ops.nms semantics (score-desc,
  suppress IoU > thr), class-aware like the reference's class-offset trick.
* ``voxelize_sequential``    — spconv ``points_to_voxel`` loop.
* ``rotated_iou_bev``        — polygon clipping IoU (OpenPCDet iou_bev).
* ``pc2_read_points``        — ``sensor_msgs.point_cloud2.read_points(skip_nans)``.
"""
from __future__ import annotations

import math
import struct
from typing import List, Sequence, Tuple

import numpy as np


# ----------------------------------------------------------------------------- image
def _axis_coords(n_dst: int, n_src: int):
    scale = np.float32(n_src) / np.float32(n_dst)  # fp32 like the kernel
    f = (np.arange(n_dst, dtype=np.float32) + np.float32(0.5)) * scale - np.float32(0.5)
    s = np.floor(f).astype(np.int64)
    a = f - s.astype(np.float32)
    a = np.where(s < 0, 0.0, a)
    s = np.where(s < 0, 0, s)
    hi = s >= n_src - 1
    a = np.where(hi, 0.0, a)
    s = np.where(hi, n_src - 1, s)
    s1 = np.minimum(s + 1, n_src - 1)
    return s, s1, a.astype(np.float32)


def resize_bilinear_u8(img: np.ndarray, out_h: int, out_w: int, quantize: bool = True) -> np.ndarray:
    """img [H, W, C] uint8 → [out_h, out_w, C] (uint8 if quantize else float32)."""
    H, W = img.shape[:2]
    y0, y1, ay = _axis_coords(out_h, H)
    x0, x1, ax = _axis_coords(out_w, W)
    f = img.astype(np.float32)
    ax_ = ax[None, :, None]
    top = f[y0][:, x0] + ax_ * (f[y0][:, x1] - f[y0][:, x0])
    bot = f[y1][:, x0] + ax_ * (f[y1][:, x1] - f[y1][:, x0])
    out = top + ay[:, None, None] * (bot - top)
    if quantize:
        return np.clip(np.rint(out), 0, 255).astype(np.uint8)
    return out


def letterbox_params(src_hw: Tuple[int, int], dst_hw: Tuple[int, int], mode: str = "letterbox"):
    """Returns (reg_top, reg_left, reg_h, reg_w, gain_x, gain_y).

    stretch  : the whole dst is the resized region (reference behaviour,
               ``cv2.resize(img, (W, H))``).
    letterbox: keep aspect ratio, centre, pad 114 (YOLOv5 ``letterbox``).
    """
    h0, w0 = src_hw
    H, W = dst_hw
    if mode == "stretch":
        return 0, 0, H, W, W / w0, H / h0
    r = min(H / h0, W / w0)
    nw, nh = int(round(w0 * r)), int(round(h0 * r))
    dw, dh = (W - nw) / 2.0, (H - nh) / 2.0
    top, left = int(round(dh - 0.1)), int(round(dw - 0.1))
    return top, left, nh, nw, nw / w0, nh / h0


def preprocess_image(img: np.ndarray, dst_hw, mode="stretch", scale=(1 / 255.0,) * 3, bias=(0.0,) * 3,
                     swap_rb=False, pad=114.0, layout="NCHW") -> np.ndarray:
    H, W = dst_hw
    top, left, nh, nw, _, _ = letterbox_params(img.shape[:2], dst_hw, mode)
    canvas = np.full((H, W, 3), pad, np.float32)
    canvas[top:top + nh, left:left + nw] = resize_bilinear_u8(img[..., :3], nh, nw).astype(np.float32)
    if swap_rb:
        canvas = canvas[..., ::-1]
    out = canvas * np.asarray(scale, np.float32) + np.asarray(bias, np.float32)
    return out.transpose(2, 0, 1).copy() if layout == "NCHW" else out


# ----------------------------------------------------------------------------- sensor_msgs/Image -> rgb8
# the encodings image_to_rgb8 takes (the values: stable codes for a device launcher)
IMAGE_ENCODINGS = {"rgb8": 0, "bgr8": 1, "rgba8": 2, "bgra8": 3, "mono8": 4, "mono16": 5, "yuv422": 6,
                   "yuv422_yuy2": 7, "bayer_rggb8": 8, "bayer_bggr8": 9, "bayer_gbrg8": 10, "bayer_grbg8": 11}
_ENC_BPP = {"rgb8": 3, "bgr8": 3, "rgba8": 4, "bgra8": 4, "mono8": 1, "mono16": 2, "yuv422": 2, "yuv422_yuy2": 2,
            "bayer_rggb8": 1, "bayer_bggr8": 1, "bayer_gbrg8": 1, "bayer_grbg8": 1}
# (row, column) of the red sample inside the 2x2 colour-filter tile: the ROS name spells the
# colours of pixels (0,0), (0,1), (1,0), (1,1)
_BAYER_RED = {"bayer_rggb8": (0, 0), "bayer_grbg8": (0, 1), "bayer_gbrg8": (1, 0), "bayer_bggr8": (1, 1)}
# BT.601 limited range, 20-bit fixed point (OpenCV's COLOR_YUV2RGB_UYVY constants)
_YUV_SHIFT, _YUV_CY, _YUV_CVR, _YUV_CVG, _YUV_CUG, _YUV_CUB = 20, 1220542, 1673527, -852492, -409993, 2116026


def image_packed_row(width: int, encoding: str) -> int:
    """Bytes of one row without padding; ValueError for an encoding ``image_to_rgb8`` does not take."""
    if encoding not in _ENC_BPP:
        raise ValueError(f"unsupported image encoding {encoding!r}")
    return int(width) * _ENC_BPP[encoding]


def check_image_geometry(height: int, width: int, step: int, encoding: str) -> int:
    """The geometry checks of ``image_to_rgb8``; -> packed row bytes."""
    packed = image_packed_row(width, encoding)
    if height < 1 or width < 1:
        raise ValueError(f"{encoding!r} image of {width}x{height}")
    if encoding.startswith("yuv422") and width % 2:
        raise ValueError(f"{encoding!r} needs an even width, not {width}")
    if encoding.startswith("bayer") and (height < 2 or width < 2):
        raise ValueError(f"{encoding!r} needs at least 2x2 pixels, not {width}x{height}")
    if step < packed:
        raise ValueError(f"{encoding!r} step {step} below the {packed} B of a {width}-pixel row")
    return packed


def image_to_rgb8(data, height: int, width: int, step: int, encoding: str, is_bigendian: int = 0) -> np.ndarray:
    """What ``cv_bridge.imgmsg_to_cv2(msg, 'rgb8')`` makes of a raw ``sensor_msgs/Image``
    payload: uint8 [H, W, 3].  Integer arithmetic throughout, so it can serve as the bit-exact
    specification of a device kernel.  Bytes of a row past its packed size are ignored."""
    H, W, step = int(height), int(width), int(step)
    packed = check_image_geometry(H, W, step, encoding)
    buf = np.frombuffer(data, np.uint8)
    if buf.size < (H - 1) * step + packed:
        raise ValueError(f"{encoding!r} image {W}x{H} step {step}: {buf.size} B of data")
    rows = np.lib.stride_tricks.as_strided(buf, (H, packed), (step, 1))
    if encoding in ("rgb8", "bgr8", "rgba8", "bgra8"):
        a = rows.reshape(H, W, _ENC_BPP[encoding])[..., :3]
        return np.ascontiguousarray(a[..., ::-1] if encoding.startswith("bgr") else a)
    if encoding == "mono8":
        return np.repeat(rows.reshape(H, W, 1), 3, axis=2)
    if encoding == "mono16":
        b = rows.reshape(H, W, 2).astype(np.int32)
        v = (b[..., 0] << 8 | b[..., 1]) if is_bigendian else (b[..., 1] << 8 | b[..., 0])
        g = ((v + 128) // 257).astype(np.uint8)
        return np.repeat(g[..., None], 3, axis=2)
    if encoding in ("yuv422", "yuv422_yuy2"):
        m = rows.reshape(H, W // 2, 4).astype(np.int32)
        if encoding == "yuv422":  # U0 Y0 V0 Y1
            u, y0, v, y1 = (m[..., k] for k in range(4))
        else:                     # Y0 U0 Y1 V0
            y0, u, y1, v = (m[..., k] for k in range(4))
        y = np.stack([y0, y1], axis=2).reshape(H, W)
        u = np.repeat(u, 2, axis=1) - 128
        v = np.repeat(v, 2, axis=1) - 128
        yy = np.maximum(y - 16, 0) * _YUV_CY + (1 << (_YUV_SHIFT - 1))
        out = np.empty((H, W, 3), np.uint8)
        out[..., 0] = np.clip((yy + _YUV_CVR * v) >> _YUV_SHIFT, 0, 255)
        out[..., 1] = np.clip((yy + _YUV_CVG * v + _YUV_CUG * u) >> _YUV_SHIFT, 0, 255)
        out[..., 2] = np.clip((yy + _YUV_CUB * u) >> _YUV_SHIFT, 0, 255)
        return out
    # Bayer, bilinear, colour-filter plane extended by reflect-101 (keeps the colour parity)
    p = np.pad(rows.astype(np.int32), 1, mode="reflect")
    c = p[1:-1, 1:-1]
    n, s, w, e = p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]
    cross = (n + s + w + e + 2) >> 2
    diag = (p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:] + 2) >> 2
    horiz, vert = (w + e + 1) >> 1, (n + s + 1) >> 1
    ry, rx = _BAYER_RED[encoding]
    yy, xx = np.mgrid[0:H, 0:W]
    red_row, red_col = ((yy ^ ry) & 1) == 0, ((xx ^ rx) & 1) == 0
    at_r, at_b = red_row & red_col, ~red_row & ~red_col
    r = np.where(at_r, c, np.where(at_b, diag, np.where(red_row, horiz, vert)))
    b = np.where(at_b, c, np.where(at_r, diag, np.where(red_row, vert, horiz)))
    g = np.where(at_r | at_b, cross, c)
    return np.stack([r, g, b], axis=2).astype(np.uint8)


def rgb8_to_encoding(rgb: np.ndarray, encoding: str, step=None, is_bigendian: int = 0) -> bytes:
    """Synthetic sensor data: an rgb8 frame [H, W, 3] as the ``H * step`` payload bytes of
    ``encoding`` (mosaicked, chroma averaged over the pixel pair, or bytes permuted; padding
    bytes are 0xA5).  A data generator, not a specification: ``image_to_rgb8`` of the result
    is the original only where the encoding keeps it."""
    rgb = np.asarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    packed = image_packed_row(W, encoding)
    step = packed if step is None else int(step)
    check_image_geometry(H, W, step, encoding)
    c = rgb.astype(np.int32)
    R, G, B = c[..., 0], c[..., 1], c[..., 2]
    if encoding in ("rgb8", "bgr8"):
        body = rgb if encoding == "rgb8" else rgb[..., ::-1]
    elif encoding in ("rgba8", "bgra8"):
        body = np.full((H, W, 4), 255, np.uint8)
        body[..., :3] = rgb if encoding == "rgba8" else rgb[..., ::-1]
    elif encoding in ("mono8", "mono16"):
        gray = (77 * R + 150 * G + 29 * B + 128) >> 8
        if encoding == "mono8":
            body = gray.astype(np.uint8)
        else:
            body = (gray * 257).astype(">u2" if is_bigendian else "<u2").view(np.uint8)
    elif encoding in ("yuv422", "yuv422_yuy2"):
        y = np.clip(((66 * R + 129 * G + 25 * B + 128) >> 8) + 16, 16, 235)
        u = np.clip(((-38 * R - 74 * G + 112 * B + 128) >> 8) + 128, 16, 240)
        v = np.clip(((112 * R - 94 * G - 18 * B + 128) >> 8) + 128, 16, 240)
        u = (u[:, 0::2] + u[:, 1::2] + 1) >> 1
        v = (v[:, 0::2] + v[:, 1::2] + 1) >> 1
        order = (u, y[:, 0::2], v, y[:, 1::2]) if encoding == "yuv422" else (y[:, 0::2], u, y[:, 1::2], v)
        body = np.stack(order, axis=2).astype(np.uint8)
    else:
        ry, rx = _BAYER_RED[encoding]
        yy, xx = np.mgrid[0:H, 0:W]
        ch = (((yy ^ ry) & 1) + ((xx ^ rx) & 1))  # 0 at red, 1 at green, 2 at blue sites
        body = np.take_along_axis(rgb, ch[..., None], axis=2)
    out = np.full((H, step), 0xA5, np.uint8)
    out[:, :packed] = np.ascontiguousarray(body).reshape(H, packed)
    return out.tobytes()


# ----------------------------------------------------------------------------- 2D NMS
def box_iou_np(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    ix1 = np.maximum(a[:, None, 0], b[None, :, 0])
    iy1 = np.maximum(a[:, None, 1], b[None, :, 1])
    ix2 = np.minimum(a[:, None, 2], b[None, :, 2])
    iy2 = np.minimum(a[:, None, 3], b[None, :, 3])
    inter = np.clip(ix2 - ix1, 0, None) * np.clip(iy2 - iy1, 0, None)
    aa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (aa[:, None] + ab[None, :] - inter)


def nms_greedy(boxes: np.ndarray, scores: np.ndarray, thr: float, classes=None, order_key=None,
               iou_fn=None, max_out: int | None = None) -> List[int]:
    """Greedy NMS; returns kept indices in score order.

    order_key: optional int array used to break score ties (ascending), the
    same (score desc, index asc) order the GPU sort uses."""
    n = len(scores)
    if n == 0:
        return []
    if order_key is None:
        order_key = np.arange(n)
    order = np.lexsort((order_key, -scores.astype(np.float64)))
    iou_fn = iou_fn or (lambda a, b: box_iou_np(a[None], b)[0])
    removed = np.zeros(n, bool)
    keep = []
    for oi, i in enumerate(order):
        if removed[i]:
            continue
        keep.append(int(i))
        if max_out is not None and len(keep) >= max_out:
            break
        rest = order[oi + 1:]
        rest = rest[~removed[rest]]
        if len(rest) == 0:
            continue
        ious = iou_fn(boxes[i], boxes[rest])
        sup = ious > thr
        if classes is not None:
            sup &= classes[rest] == classes[i]
        removed[rest[sup]] = True
    return keep


# ----------------------------------------------------------------------------- rotated IoU
def _corners(b):
    c, s = math.cos(b[6]), math.sin(b[6])
    hx, hy = b[3] / 2, b[4] / 2
    pts = []
    for ox, oy in ((-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy)):
        pts.append((b[0] + c * ox - s * oy, b[1] + s * ox + c * oy))
    return pts


def _clip(poly, a, b):
    out = []
    n = len(poly)
    def side(p):
        return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
    for i in range(n):
        cur, nxt = poly[i], poly[(i + 1) % n]
        dc, dn = side(cur), side(nxt)
        if dc >= 0:
            out.append(cur)
        if (dc >= 0) != (dn >= 0):
            t = dc / (dc - dn)
            out.append((cur[0] + t * (nxt[0] - cur[0]), cur[1] + t * (nxt[1] - cur[1])))
    return out


def rotated_overlap(a, b) -> float:
    poly = _corners(a)
    cb = _corners(b)
    for i in range(4):
        if not poly:
            break
        poly = _clip(poly, cb[i], cb[(i + 1) % 4])
    if len(poly) < 3:
        return 0.0
    area = 0.0
    for i in range(len(poly)):
        p, q = poly[i], poly[(i + 1) % len(poly)]
        area += p[0] * q[1] - q[0] * p[1]
    return abs(area) / 2


def rotated_iou_bev(a, bs) -> np.ndarray:
    out = np.zeros(len(bs), np.float64)
    if len(bs) == 0:
        return out
    bs_ = np.asarray(bs, np.float64)
    # exact prefilter: boxes whose bounding circles do not meet have no overlap (IoU 0)
    ra = 0.5 * math.hypot(a[3], a[4])
    rb = 0.5 * np.hypot(bs_[:, 3], bs_[:, 4])
    near = np.hypot(bs_[:, 0] - a[0], bs_[:, 1] - a[1]) <= ra + rb
    for k in np.nonzero(near)[0]:
        b = bs_[k]
        ov = rotated_overlap(a, b)
        out[k] = ov / max(a[3] * a[4] + b[3] * b[4] - ov, 1e-8)
    return out


def rotated_iou_3d(a, bs) -> np.ndarray:
    """3D IoU of box ``a`` with each of ``bs`` (x, y, z, dx, dy, dz, yaw; z the
    centre), OpenPCDet ``boxes_iou3d_gpu``: the rotated BEV overlap times the
    common height, over the union of the volumes."""
    out = np.zeros(len(bs), np.float64)
    for k, b in enumerate(np.asarray(bs, np.float64).reshape(-1, len(a)) if len(bs) else ()):
        h = max(0.0, min(a[2] + a[5] / 2, b[2] + b[5] / 2) - max(a[2] - a[5] / 2, b[2] - b[5] / 2))
        if h <= 0.0:
            continue
        inter = rotated_overlap(a, b) * h
        out[k] = inter / max(a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - inter, 1e-8)
    return out


# ----------------------------------------------------------------------------- point clouds
PF_FMT = {1: "b", 2: "B", 3: "h", 4: "H", 5: "i", 6: "I", 7: "f", 8: "d"}


def pc2_read_points(data: bytes, n: int, point_step: int, offsets: Sequence[int], dtypes: Sequence[int]):
    """Sequential read_points(skip_nans=True) over 4 fields → [M, 4] float32."""
    out = []
    for i in range(n):
        rec = i * point_step
        vals = [struct.unpack_from("<" + PF_FMT[dt], data, rec + off)[0] for off, dt in zip(offsets, dtypes)]
        if any(isinstance(v, float) and math.isnan(v) for v in vals):
            continue
        out.append(vals)
    return np.asarray(out, np.float32).reshape(-1, 4)


def voxelize_sequential(points: np.ndarray, pc_range, voxel_size, max_points: int, max_voxels: int):
    """spconv points_to_voxel loop (continue-on-full semantics).

    Returns voxels [V, P, F], coords [V, 3] (z, y, x), num_points [V]."""
    r = np.asarray(pc_range, np.float32)
    vs = np.asarray(voxel_size, np.float32)
    grid = np.round((r[3:] - r[:3]) / vs).astype(np.int64)
    F = points.shape[1]
    coor_to_vid = {}
    voxels, coords, num = [], [], []
    for i in range(points.shape[0]):
        p = points[i]
        c = np.floor((p[:3] - r[:3]) / vs).astype(np.int64)
        if np.any(c < 0) or np.any(c >= grid):
            continue
        key = (int(c[2]), int(c[1]), int(c[0]))
        vid = coor_to_vid.get(key, -1)
        if vid == -1:
            if len(voxels) >= max_voxels:
                continue
            vid = len(voxels)
            coor_to_vid[key] = vid
            voxels.append(np.zeros((max_points, F), np.float32))
            coords.append(key)
            num.append(0)
        if num[vid] < max_points:
            voxels[vid][num[vid]] = p
            num[vid] += 1
    if not voxels:
        return np.zeros((0, max_points, F), np.float32), np.zeros((0, 3), np.int32), np.zeros((0,), np.int32)
    return np.stack(voxels), np.asarray(coords, np.int32), np.asarray(num, np.int32)
