"""Bird's-eye-view picture of a LiDAR frame and its detections: the host painter.

This file is the bit-exact definition of the picture, written so that a device
renderer can reproduce it pixel for pixel (the role :mod:`.draw` plays for
``draw.hip``): fp32 pixel mapping with a fixed operation order, integer
arithmetic after it.  The reference showed its 3D results in rviz / Open3D /
Mayavi windows; a headless client publishes this picture
instead (:class:`~triton_client_amd.inference.ros_inference3d.RosInference3D`
``bev_topic``).

The view (:class:`BevView`) is fixed: +x up, +y left, ``res`` metres per pixel,
``H = round((x1 - x0) / res)`` rows and ``W = round((y1 - y0) / res)`` columns,
and a height range ``z_range`` in the sensor frame that does not depend on the
frame's points, so grey levels are comparable between frames.

Every step after the fp32 pixel mapping is integer arithmetic.

Points layer
    ``fr = (x1 - x) * inv_res`` and ``fc = (y1 - y) * inv_res`` in fp32 (one
    subtract, one multiply by ``inv_res = float32(1 / res)``), pixel =
    ``(floor(fr), floor(fc))``.  A point is skipped unless ``0 <= fr < H`` and
    ``0 <= fc < W`` and z is finite (so NaN and infinite coordinates never
    draw).  ``level = 55 + clamp(floor(((z - z_offset) - z0) * zscale), 0, 200)``
    with ``zscale = float32(200 / (z1 - z0))``; a pixel takes the maximum level
    of its points (order independent) and is painted ``(level, level, level)``.
    Untouched pixels are black.

Boxes layer
    Boxes ``0..count-1`` in result order, over the points; a later box wins.
    Rows are ``(x, y, z, dx, dy, dz, yaw)`` or 9-d det3d rows (yaw at index 8).
    The BEV corners, in :func:`~.visualize.boxes_to_corners_3d`'s order
    ``(+,+) (+,-) (-,-) (-,+)`` of ``(dx, dy) / 2``, are computed in fp32 with
    separately rounded operations: ``wx = (lx * c - ly * s) + x``,
    ``wy = (lx * s + ly * c) + y``; mapped to pixel coordinates like the points;
    clamped to ``[-32768, 32767]`` and rounded half-even to integers.  A box
    with a NaN corner is not drawn.  Edge ``i`` joins corners ``i`` and
    ``(i + 1) % 4``; edges 1, 2, 3 are drawn in ``visualize.label_colors(label)``,
    then edge 0, the heading side, in ``(255, 80, 40)`` on top.
    :func:`edge_pixels` is the integer line rule.  Pixels outside the image are
    dropped, never clamped onto the border.

Labels layer
    After all boxes, again in result order: ``"<name> <score:.2f>"`` (the text
    of :func:`.draw.label_text`: score rounded half-even from its exact value,
    the decimal class id for a label outside ``names``) in the 6x11 cell font,
    in the box's label colour, cell origin ``(min corner col + 2,
    max(min corner row - 11, 0))``, clipped at the image edges.  A box with
    every corner outside the image gets no label.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import font6x11
from .draw import label_text, text_mask
from .visualize import BOX_COLORS

HEADING_COLOR = (255, 80, 40)
LEVEL_BASE, LEVEL_SPAN = 55, 200
PX_LIMIT = 32768  # corner pixel coordinates are clamped to [-PX_LIMIT, PX_LIMIT - 1]
# boxes_to_corners_3d's bottom-face order
CORNER_SIGNS = ((1.0, 1.0), (1.0, -1.0), (-1.0, -1.0), (-1.0, 1.0))


@dataclass(frozen=True)
class BevView:
    x_range: Tuple[float, float] = (0.0, 69.12)
    y_range: Tuple[float, float] = (-39.68, 39.68)
    res: float = 0.1
    z_range: Tuple[float, float] = (-3.0, 1.0)

    def __post_init__(self):
        (x0, x1), (y0, y1), (z0, z1) = self.x_range, self.y_range, self.z_range
        if not (self.res > 0 and x1 > x0 and y1 > y0 and z1 > z0):
            raise ValueError(f"empty view: x {self.x_range}, y {self.y_range}, z {self.z_range}, res {self.res}")
        if self.H < 1 or self.W < 1 or self.H >= PX_LIMIT or self.W >= PX_LIMIT:
            raise ValueError(f"view of {self.W}x{self.H} pixels")

    @property
    def H(self) -> int:
        return int(round((self.x_range[1] - self.x_range[0]) / self.res))

    @property
    def W(self) -> int:
        return int(round((self.y_range[1] - self.y_range[0]) / self.res))

    @staticmethod
    def for_model(cfg, res: float = 0.1) -> "BevView":
        """The model's point-cloud range (``cfg.voxel.point_cloud_range`` or a
        6-vector ``x0, y0, z0, x1, y1, z1``) at ``res`` metres per pixel."""
        r = getattr(getattr(cfg, "voxel", cfg), "point_cloud_range", cfg)
        x0, y0, z0, x1, y1, z1 = (float(v) for v in r)
        return BevView((x0, x1), (y0, y1), float(res), (z0, z1))

    def constants(self) -> Tuple[np.float32, np.float32, np.float32, np.float32, np.float32]:
        """(x1, y1, inv_res, z0, zscale) as the fp32 values both painters use."""
        return (np.float32(self.x_range[1]), np.float32(self.y_range[1]), np.float32(1.0 / self.res),
                np.float32(self.z_range[0]), np.float32(LEVEL_SPAN / (self.z_range[1] - self.z_range[0])))


def label_names(class_names: Sequence[str], label_base: int) -> list:
    """The painter's ``names[label]`` table for labels that start at ``label_base``
    (OpenPCDet labels start at 1, det3d's at 0)."""
    return ["-"] * label_base + [str(n) for n in class_names]


def label_color(label: int) -> Tuple[int, int, int]:
    """``visualize.label_colors`` of one label."""
    return tuple(int(v) for v in BOX_COLORS[int(label) % len(BOX_COLORS)])


def level_plane(points: np.ndarray, view: BevView, z_offset: float = 0.0) -> np.ndarray:
    """[H, W] uint8: 0 where no point lands, else the maximum level (55..255)."""
    H, W = view.H, view.W
    plane = np.zeros((H, W), np.uint8)
    p = np.asarray(points, np.float32)
    if p.size == 0:
        return plane
    x1, y1, inv, z0, zs = view.constants()
    with np.errstate(invalid="ignore", over="ignore"):
        fr = (x1 - p[:, 0]) * inv
        fc = (y1 - p[:, 1]) * inv
        z = p[:, 2]
        ok = (fr >= 0) & (fr < np.float32(H)) & (fc >= 0) & (fc < np.float32(W)) & np.isfinite(z)
        fr, fc, z = fr[ok], fc[ok], z[ok]
        t = ((z - np.float32(z_offset)) - z0) * zs
    lv = np.where(t >= np.float32(LEVEL_SPAN), np.float32(LEVEL_SPAN), np.where(t > 0, np.floor(t), np.float32(0)))
    lv = (lv.astype(np.int64) + LEVEL_BASE).astype(np.uint8)
    np.maximum.at(plane, (np.floor(fr).astype(np.int64), np.floor(fc).astype(np.int64)), lv)
    return plane


def box_corners_px(box: np.ndarray, view: BevView) -> Optional[np.ndarray]:
    """Integer (col, row) of the four BEV corners of one box row, [4, 2] int64;
    None if a corner is NaN (the box is not drawn)."""
    b = np.asarray(box, np.float32)
    yaw = b[8] if b.shape[0] >= 9 else b[6]
    x1, y1, inv, _, _ = view.constants()
    out = np.empty((4, 2), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        c, s = np.cos(yaw), np.sin(yaw)  # fp32
        hx, hy = np.float32(0.5) * b[3], np.float32(0.5) * b[4]
        for i, (sx, sy) in enumerate(CORNER_SIGNS):
            lx, ly = np.float32(sx) * hx, np.float32(sy) * hy
            wx = (lx * c - ly * s) + b[0]
            wy = (lx * s + ly * c) + b[1]
            fc, fr = (y1 - wy) * inv, (x1 - wx) * inv
            if np.isnan(fc) or np.isnan(fr):
                return None
            out[i, 0] = int(np.rint(np.clip(fc, -PX_LIMIT, PX_LIMIT - 1)))
            out[i, 1] = int(np.rint(np.clip(fr, -PX_LIMIT, PX_LIMIT - 1)))
    return out


def edge_pixels(ax: int, ay: int, bx: int, by: int) -> np.ndarray:
    """The integer line rule, [n + 1, 2] (x, y) samples.  The ends are put in
    lexicographic order first, so a to b and b to a give the same pixels; with
    ``n = max(|dx|, |dy|)``, sample ``i`` of ``0..n`` is
    ``a + floor((2 * i * d + n) / (2 * n))`` per coordinate (a division rounded
    half up, in integers)."""
    ax, ay, bx, by = int(ax), int(ay), int(bx), int(by)
    if (bx, by) < (ax, ay):
        ax, ay, bx, by = bx, by, ax, ay
    dx, dy = bx - ax, by - ay
    n = max(abs(dx), abs(dy))
    if n == 0:
        return np.array([[ax, ay]], np.int64)
    i = np.arange(n + 1, dtype=np.int64)
    return np.stack([ax + (2 * i * dx + n) // (2 * n), ay + (2 * i * dy + n) // (2 * n)], 1)


def _draw_edge(img: np.ndarray, a, b, color) -> None:
    H, W = img.shape[:2]
    px = edge_pixels(a[0], a[1], b[0], b[1])
    ok = (px[:, 0] >= 0) & (px[:, 0] < W) & (px[:, 1] >= 0) & (px[:, 1] < H)
    img[px[ok, 1], px[ok, 0]] = color


def _draw_label(img: np.ndarray, cor: np.ndarray, text: str, color) -> None:
    H, W = img.shape[:2]
    inside = (cor[:, 0] >= 0) & (cor[:, 0] < W) & (cor[:, 1] >= 0) & (cor[:, 1] < H)
    if not inside.any():
        return
    m = text_mask(text)
    x0, y0 = int(cor[:, 0].min()) + 2, max(int(cor[:, 1].min()) - font6x11.H, 0)
    xa, ya = max(x0, 0), max(y0, 0)
    xb, yb = min(x0 + m.shape[1], W), min(y0 + m.shape[0], H)
    if xb <= xa or yb <= ya:
        return
    img[ya:yb, xa:xb][m[ya - y0:yb - y0, xa - x0:xb - x0]] = color


def render_bev_frame(points, n, boxes, scores, labels, count, view: BevView,
                     names: Optional[Sequence[str]] = None, z_offset: float = 0.0) -> np.ndarray:
    """One frame's picture, uint8 [H, W, 3].

    points [N, F >= 3] fp32 (rows 0..n-1 are drawn; ``n`` None: all), in the
    frame the view's z range is given in plus ``z_offset``; boxes [K, 7 | 9]
    with scores [K] and labels [K] (rows 0..count-1; ``count`` None: all; None
    boxes: points only); ``names[label]`` is a label's text."""
    if points is None:
        pts = np.zeros((0, 3), np.float32)
    else:
        pts = np.asarray(points, np.float32).reshape(-1, np.shape(points)[-1] if np.ndim(points) > 1 else 3)
        pts = pts[:len(pts) if n is None else max(0, min(int(n), len(pts)))]
    plane = level_plane(pts, view, z_offset)
    img = np.repeat(plane[:, :, None], 3, 2)
    if boxes is None or len(boxes) == 0:
        return img
    boxes = np.asarray(boxes, np.float32)
    if boxes.ndim != 2 or boxes.shape[1] < 7:
        raise ValueError(f"boxes {boxes.shape}: [K, >= 7] rows")
    k = len(boxes) if count is None else max(0, min(int(count), len(boxes)))
    labels = np.asarray(labels).astype(np.int64)
    cors = [box_corners_px(boxes[i], view) for i in range(k)]
    for i, cor in enumerate(cors):
        if cor is None:
            continue
        col = label_color(labels[i])
        for e in (1, 2, 3):
            _draw_edge(img, cor[e], cor[(e + 1) % 4], col)
        _draw_edge(img, cor[0], cor[1], HEADING_COLOR)
    for i, cor in enumerate(cors):
        if cor is not None:
            _draw_label(img, cor, label_text(int(labels[i]), scores[i], names), label_color(labels[i]))
    return img
