"""K27 — the cloud as a camera-frame depth image.

Ranging (``ops/range2d.py``) gives one depth per camera detection; this gives the whole cloud
seen from the camera: a ``sensor_msgs/Image`` of depths registered to the camera's pixels (REP
118 ``16UC1`` in millimetres, the KITTI depth-PNG convention with ``scale = 256``, or
``32FC1`` in metres).  :func:`depth_numpy` is the definition, bit for bit (the pattern of
``ops/range2d.py``); the HIP kernel ``tca_depth_image`` (``csrc/kernels/depth_image.hip``)
computes the same bytes on the device from the raw ``PointCloud2`` payload, and
:func:`depth_ref` is a float64 brute force that also marks the decisions float32 may
legitimately take differently (``docs/precision.md``).

``M = float32(P @ T)`` [3, 4] of a :class:`~triton_client_amd.ops.range2d.Calibration` is all
the per-point code sees.  :class:`DepthOptions`: ``width`` ``W`` and ``height`` ``H`` (1..4096),
``encoding`` (``"16UC1"`` or ``"32FC1"``), ``scale`` (output units per metre of ``16UC1``:
1000 gives millimetres, 256 the KITTI depth PNG), ``min_depth`` (> 0) and ``splat`` (0..4).

**Per point** ``(x, y, z)`` as sent, every operation rounded to float32 on its own (no FMA);
``w``, ``a``, ``b``, ``u = a / w`` and ``v = b / w`` are those of ``ops/range2d.py``
(:func:`~triton_client_amd.ops.range2d.project_uvw`)::

    visible = (w >= min_depth) and (0 <= u < W) and (0 <= v < H)    # float compares; a NaN is false
    px = int32(u); py = int32(v)                                     # truncation, which is floor here
    16UC1:  t = w * scale; d = int32(rint(min(t, 65536f)))           # half to even
            valid = visible and 1 <= d <= 65535                      # beyond the range: dropped, never clamped
            key = uint32(d)
    32FC1:  valid = visible; key = the bits of w as uint32           # positive floats order as their bits

**Per pixel** the value is the smallest key over all valid points whose splat square — the
``(2 splat + 1)^2`` pixels around ``(px, py)``, clipped to the image — covers the pixel.  A pixel
no point covers holds 0 in ``16UC1`` and the quiet NaN with bits ``0x7FC00000`` in ``32FC1``.  The
output is ``[H, W]`` ``<u2`` or ``<f4``.  The minimum is commutative: nothing depends on the
order of the points.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import _native
from ..ros import msgs
from .cloud_common import CloudLayout, CloudStager, _align, cloud_bytes, cloud_xyzi, fields_f32, plan_staging
from .range2d import INT31, U, _xyz, project_uvw

MAX_FRAMES = 64  # clouds per launch
MAX_SIDE = 4096  # pixels per image side
MAX_SPLAT = 4
MAX_PLANE = 256 << 20  # bytes of key plane per launch
EMPTY = 0xFFFFFFFF  # the key of a pixel no point covers
NAN_BITS = 0x7FC00000  # what such a pixel holds in 32FC1
ENCODINGS = {"16UC1": 0, "32FC1": 1}  # the kernel's codes
_DTYPES = {"16UC1": np.dtype("<u2"), "32FC1": np.dtype("<f4")}


def device_enabled() -> bool:
    """``TCA_DEVICE_DEPTH=0`` keeps the definition on GPU engines too."""
    return os.environ.get("TCA_DEVICE_DEPTH", "1") != "0"


# ----------------------------------------------------------------------------- options
@dataclass(frozen=True)
class DepthOptions:
    width: int
    height: int
    encoding: str = "16UC1"
    scale: float = 1000.0
    min_depth: float = 0.5
    splat: int = 1

    def __post_init__(self):
        for name in ("width", "height"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= MAX_SIDE:
                raise ValueError(f"{name} must be an integer in 1..{MAX_SIDE}, got {v!r}")
        if self.encoding not in ENCODINGS:
            raise ValueError(f"encoding must be one of {sorted(ENCODINGS)}, got {self.encoding!r}")
        for name in ("scale", "min_depth"):
            try:
                with np.errstate(over="ignore"):
                    v = np.float32(getattr(self, name))
            except (TypeError, ValueError):
                raise ValueError(f"{name} must be a number, got {getattr(self, name)!r}") from None
            if not (np.isfinite(v) and v > 0):
                raise ValueError(f"{name} must be finite and positive in float32, got {getattr(self, name)!r}")
        s = self.splat
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= s <= MAX_SPLAT:
            raise ValueError(f"splat must be an integer in 0..{MAX_SPLAT}, got {s!r}")

    @property
    def dtype(self) -> np.dtype:
        return _DTYPES[self.encoding]

    @property
    def frame_bytes(self) -> int:
        return self.width * self.height * self.dtype.itemsize


# ------------------------------------------------------------------------- definition
def depth_keys_numpy(points, M, opts: DepthOptions):
    """The per-point half of the definition → ``(px [N] int32, py [N] int32, valid [N] bool,
    key [N] uint32)``; ``px``, ``py`` and ``key`` are 0 where the point is not visible."""
    u, v, w = project_uvw(points, M)
    W, H = np.float32(opts.width), np.float32(opts.height)
    with np.errstate(invalid="ignore", over="ignore"):
        visible = (w >= np.float32(opts.min_depth)) & (u >= np.float32(0)) & (u < W) & (v >= np.float32(0)) & (v < H)
        px = np.where(visible, u, np.float32(0)).astype(np.int32)
        py = np.where(visible, v, np.float32(0)).astype(np.int32)
        if opts.encoding == "16UC1":
            t = np.where(visible, w, np.float32(0)) * np.float32(opts.scale)
            d = np.rint(np.minimum(t, np.float32(65536.0))).astype(np.int32)
            valid = visible & (d >= 1) & (d <= 65535)
            key = d.astype(np.uint32)
        else:
            valid = visible
            key = np.where(visible, w, np.float32(0)).astype(np.float32).view(np.uint32)
    return px, py, valid, np.where(valid, key, np.uint32(0)).astype(np.uint32)


def image_of_keys(plane: np.ndarray, opts: DepthOptions) -> np.ndarray:
    """The key plane (uint32 [H, W], ``EMPTY`` where nothing landed) as the output image."""
    if opts.encoding == "16UC1":
        return np.where(plane == EMPTY, 0, plane).astype("<u2")
    return np.where(plane == EMPTY, np.uint32(NAN_BITS), plane).astype("<u4").view("<f4")


def depth_numpy(points, M, opts: DepthOptions) -> np.ndarray:
    """→ the ``[H, W]`` depth image (``<u2`` or ``<f4``): the definition.  ``points`` [N, >=3]
    (x, y, z); ``M`` [3, 4] float32."""
    px, py, valid, key = depth_keys_numpy(points, M, opts)
    W, H, s = opts.width, opts.height, int(opts.splat)
    plane = np.full((H, W), EMPTY, np.uint32)
    px, py, key = px[valid].astype(np.int64), py[valid].astype(np.int64), key[valid]
    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            xx, yy = px + dx, py + dy
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)  # the square is clipped to the image
            np.minimum.at(plane, (yy[ok], xx[ok]), key[ok])
    return image_of_keys(plane, opts)


def depth_ref(points, M, opts: DepthOptions):
    """Float64 brute force of the per-point half → ``(px, py, valid, key16, pixel_band [N] bool,
    valid_band [N] bool)``; ``key16`` is the ``16UC1`` key (``int32(rint(min(w * scale, 65536)))``
    whatever the encoding), 0 where the point is not valid.

    The bands mark the points whose decision the float32 evaluation may legitimately take
    differently, with the bounds of :func:`~triton_client_amd.ops.range2d.range2d_ref`: with
    ``S_a`` the sum of the absolute terms of ``a`` (``S_b``, ``S_w`` alike), ``u`` is within
    ``eu = 5 * 2**-24 * (S_a + |u| S_w) / |w| + 2 * 2**-24 * |u|`` of the exact pixel coordinate,
    ``w`` within ``ew = 5 * 2**-24 * S_w`` and ``t = w * scale`` within ``et = ew * scale +
    2**-24 * |t|``.  ``pixel_band``: ``u`` or ``v`` lies within ``eu`` / ``ev`` of an integer (the
    image edges 0, W and H are integers).  ``valid_band``: ``w`` lies within ``ew`` of
    ``min_depth``, or (``16UC1``) ``t`` within ``et`` of 0.5 or 65535.5.  Both are raised only
    for points that are not clearly nearer than ``min_depth``: such a point is invalid on both
    sides whatever its pixel.  ``docs/precision.md`` has the derivation.  ``M``, ``scale`` and
    ``min_depth`` are float32 inputs of both evaluations and exact here."""
    x, y, z = (c.astype(np.float64) for c in _xyz(points))
    M64 = np.asarray(M, np.float32).reshape(3, 4).astype(np.float64)
    md, sc = float(np.float32(opts.min_depth)), float(np.float32(opts.scale))
    W, H = float(opts.width), float(opts.height)

    def dot(r):
        t = (M64[r, 0] * x, M64[r, 1] * y, M64[r, 2] * z, M64[r, 3])
        return t[0] + t[1] + t[2] + t[3], np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2]) + np.abs(t[3])

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        (w, Sw), (a, Sa), (b, Sb) = dot(2), dot(0), dot(1)
        u, v = a / w, b / w
        visible = (w >= md) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        px = np.where(visible, u, 0.0).astype(np.int32)
        py = np.where(visible, v, 0.0).astype(np.int32)
        t = w * sc
        d = np.rint(np.minimum(np.where(visible, t, 0.0), 65536.0)).astype(np.int32)
        in_range = (d >= 1) & (d <= 65535)
        valid = visible & in_range if opts.encoding == "16UC1" else visible
        aw = np.abs(w)
        eu = 5 * U * (Sa + np.abs(u) * Sw) / aw + 2 * U * np.abs(u)
        ev = 5 * U * (Sb + np.abs(v) * Sw) / aw + 2 * U * np.abs(v)
        ew = 5 * U * Sw
        et = ew * sc + U * np.abs(t)
        maybe = w >= md - ew  # (a NaN is false: such a point is in no band)
        fu, fv = u - np.floor(u), v - np.floor(v)
        pixel_band = maybe & ((fu <= eu) | (1.0 - fu <= eu) | (fv <= ev) | (1.0 - fv <= ev))
        valid_band = maybe & (np.abs(w - md) <= ew)
        if opts.encoding == "16UC1":
            valid_band |= maybe & ((np.abs(t - 0.5) <= et) | (np.abs(t - 65535.5) <= et))
    return px, py, valid, np.where(visible & in_range, d, 0).astype(np.int32), pixel_band, valid_band


def depth_message(cloud, image: np.ndarray, opts: DepthOptions, frame_id: str = "") -> msgs.Image:
    """The image as a ``sensor_msgs/Image`` with the cloud's stamp and seq, in frame ``frame_id``
    (the cloud's when empty)."""
    h = cloud.header
    a = np.ascontiguousarray(image, opts.dtype)
    if a.shape != (opts.height, opts.width):
        raise ValueError(f"image shape {a.shape}, want {(opts.height, opts.width)}")
    return msgs.Image(header=msgs.Header(seq=h.seq, stamp=h.stamp, frame_id=frame_id or h.frame_id),
                      height=opts.height, width=opts.width, encoding=opts.encoding, is_bigendian=0,
                      step=opts.width * opts.dtype.itemsize, data=memoryview(a.view(np.uint8).reshape(-1)))


# --------------------------------------------------------------------------------- GPU
@dataclass
class DepthCall:
    """One prepared launch: device views of its inputs, workspace and output."""
    data: torch.Tensor
    data_bytes: int
    frame_off: torch.Tensor
    frame_n: torch.Tensor
    plane: torch.Tensor  # uint8 view of B * H * W uint32 keys
    out: torch.Tensor  # uint8, the images back to back
    M: np.ndarray  # host float32 [12]
    layout: CloudLayout
    batch: int
    max_n: int
    opts: DepthOptions

    @property
    def out_bytes(self) -> int:
        return self.batch * self.opts.frame_bytes


def launch(c: DepthCall, stream=None) -> None:
    """The launch alone (the plane's reset and the two kernels on ``stream``): no allocation,
    no copy, no sync."""
    p = _native.ptr
    o, r = c.layout.offsets, c.opts
    _native.call("tca_depth_image", p(c.data), c.data_bytes, p(c.frame_off), p(c.frame_n), c.batch, c.max_n,
                 c.layout.point_step, o[0], o[1], o[2], c.M.ctypes.data, int(r.width), int(r.height),
                 ENCODINGS[r.encoding], float(r.scale), float(r.min_depth), int(r.splat), p(c.plane), p(c.out),
                 _native.stream_ptr(stream))


def layout_device_ok(lay: CloudLayout) -> bool:
    """What ``tca_depth_image`` reads in place: little-endian FLOAT32 x, y, z inside the record."""
    return fields_f32(lay, (0, 1, 2))


def images_of(host: np.ndarray, batch: int, opts: DepthOptions) -> List[np.ndarray]:
    """The ``batch`` images of a launch's output bytes, each its own array."""
    a = np.ascontiguousarray(host).view(np.uint8)[:batch * opts.frame_bytes]
    a = a.view(opts.dtype).reshape(batch, opts.height, opts.width)
    return [a[b].copy() for b in range(batch)]


class DepthImager(CloudStager):
    """Turns clouds into camera-frame depth images: on a GPU with ``tca_depth_image`` (its own
    workspace, stream and pinned staging: one H2D of the payloads, one launch, one D2H of the
    images per launch group of same-layout clouds), on the CPU — and with ``TCA_DEVICE_DEPTH=0``
    — with the definition.  Clouds the kernel does not take (non-FLOAT32 or big-endian fields)
    run the definition with one warning."""

    def prepare(self, payloads: Sequence, ns: Sequence[int], layout: CloudLayout, M, opts: DepthOptions,
                stream=None, misalign: int = 0) -> DepthCall:
        """Stage one batch (``payloads[b]``: the bytes of ``ns[b]`` points of ``layout``) in pinned
        memory and upload it with one H2D copy on ``stream``.  ``misalign``: start every payload
        this many bytes past a 16-byte boundary."""
        if not layout_device_ok(layout):
            raise ValueError(f"tca_depth_image does not take this layout: {layout}")
        B = len(payloads)
        ns = [int(n) for n in ns]
        if not 1 <= B <= MAX_FRAMES:
            raise ValueError(f"{B} clouds do not fit one call (1..{MAX_FRAMES}): split the batch")
        data_bytes = plan_staging(ns, layout.point_step, misalign, ()).data_bytes  # (refused before any allocation)
        if data_bytes >= INT31:
            raise ValueError(f"{data_bytes} payload bytes do not fit one call: split the batch")
        n_px = B * opts.width * opts.height
        if 4 * n_px > MAX_PLANE:
            raise ValueError(f"a key plane of {4 * n_px} bytes does not fit one call: split the batch")
        dev, _, view = self._stage("dep_in", payloads, ns, layout.point_step, misalign, (), stream)
        plane = self._device_buf("dep_plane", 4 * n_px)
        out = self._device_buf("dep_out", B * opts.frame_bytes)
        return DepthCall(data=dev, data_bytes=data_bytes, frame_off=view("frame_off", B, torch.int64),
                         frame_n=view("frame_n", B, torch.int32), plane=plane, out=out,
                         M=np.ascontiguousarray(M, np.float32).reshape(12), layout=layout, batch=B,
                         max_n=max(ns, default=0), opts=opts)

    launch = staticmethod(launch)

    def _run_device(self, payloads, ns, layout, M, opts):
        """→ per frame its image."""
        with torch.cuda.device(self.device):
            st = self._own_stream()
            c = self.prepare(payloads, ns, layout, M, opts, st)
            launch(c, st)
            host = self._fetch(c.out, c.out_bytes, st)
        return images_of(host, c.batch, opts)

    def _parts(self, idx, clouds, opts: Optional[DepthOptions] = None):
        """``idx`` cut into launches of at most 64 clouds, less than 2^31 staged bytes and, with
        ``opts``, a key plane of at most 256 MiB."""
        most = MAX_FRAMES if opts is None else max(1, min(MAX_FRAMES, MAX_PLANE // (4 * opts.width * opts.height)))
        part, size = [], 0
        for i in idx:
            nb = _align(len(clouds[i].data)) + 16
            if part and (len(part) == most or size + nb >= INT31):
                yield part
                part, size = [], 0
            part.append(i)
            size += nb
        if part:
            yield part

    # ---------------------------------------------------------------------- API
    def images(self, clouds: Sequence, M, opts: DepthOptions) -> List[np.ndarray]:
        """Per cloud its ``[H, W]`` depth image under ``M``, in input order."""
        return self._per_cloud(
            clouds, lambda i, lay: layout_device_ok(lay),
            lambda i, lay: image_numpy(clouds[i], M, opts, lay),
            lambda lay, part: (*cloud_bytes(clouds, part), lay, M, opts), self._run_device,
            lambda i, lay: f"DepthImager: tca_depth_image takes little-endian FLOAT32 x, y, z (got {lay}); such "
                           "clouds are imaged on the host",
            device=self.gpu and device_enabled(), parts=lambda idx, cl: self._parts(idx, cl, opts))


def image_numpy(cloud, M, opts: DepthOptions, lay: Optional[CloudLayout] = None) -> np.ndarray:
    """One cloud through the definition → its image."""
    return depth_numpy(cloud_xyzi(cloud, lay), M, opts)
