"""K28 — camera frames rectified from a camera calibration (``image_proc/rectify``).

The LiDAR side places camera detections in space with the pinhole projection ``P`` of a
calibration (``ops/range2d.py``, ``ops/depth_image.py``); that only meets the camera chain
where the camera chain works in the rectified image ``P`` describes.  A :class:`CameraModel`
(``K``, ``D``, ``R``, ``P`` of a ``camera_calibration`` YAML, :func:`load_camera_model`) gives
:func:`rectify_map`, a fixed-point source position per output pixel, built once on the host
in float64 — libm never reaches the per-frame code (the division of labour of the box table
of ``tca_bev_render``).  :func:`rectify_numpy` is the per-frame definition, in integers only;
the HIP kernel ``tca_rectify`` (``csrc/kernels/rectify.hip``) makes the same bytes on the
device, and :func:`rectify_ref` is the float64 bilinear interpolation the definition rounds
(``docs/precision.md``).  The output has the size of the input, the model's ``width x height``.

**The map**, for each output pixel ``(u, v)``::

    x = (u - P[0,2]) / P[0,0];  y = (v - P[1,2]) / P[1,1]          # P's 4th column is not used
    (X, Y, Wc) = R^T (x, y, 1);  x' = X / Wc;  y' = Y / Wc
    plumb_bob / rational_polynomial:  r2 = x'^2 + y'^2
        g   = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3)
        x'' = x' g + 2 p1 x' y' + p2 (r2 + 2 x'^2);  y'' = y' g + p1 (r2 + 2 y'^2) + 2 p2 x' y'
    equidistant:  r = sqrt(r2);  th = atan(r)
        s   = th (1 + k1 th^2 + k2 th^4 + k3 th^6 + k4 th^8) / r   (s = 1 at r = 0)
        x'' = x' s;  y'' = y' s
    mx = K[0,0] x'' + K[0,2];  my = K[1,1] y'' + K[1,2]
    qx = clip(rint(32 mx), -64, 32 (W + 1));  qy = clip(rint(32 my), -64, 32 (H + 1))

``rint`` rounds half to even and a non-finite position becomes -64.  Five fractional bits;
at both clip ends all four taps lie outside the frame, so a clipped entry is black.  ``D`` is
``(k1, k2, p1, p2, k3[, k4, k5, k6])`` for the polynomial models (OpenCV's order) and ``(k1, k2,
k3, k4)`` for the equidistant one.

**Per frame** (``src`` [H, W, 3] uint8), per output pixel and channel::

    ix = qx >> 5 (arithmetic);  ax = qx & 31;  iy, ay alike
    s00 = src[iy, ix], s01 = src[iy, ix+1], s10 = src[iy+1, ix], s11 = src[iy+1, ix+1]   # outside: 0
    out = ((32-ax)(32-ay) s00 + ax (32-ay) s01 + (32-ax) ay s10 + ax ay s11 + 512) >> 10
"""
from __future__ import annotations

import os
import threading
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import _native

MAX_SIDE = 4096  # pixels per image side
FRAC_BITS = 5
ONE = 1 << FRAC_BITS  # 32 map units per pixel
LOW = -2 * ONE  # the low clip: taps -2 and -1, both outside
MODELS = {"plumb_bob": (4, 5), "rational_polynomial": (8,), "equidistant": (4,)}  # coefficient counts
CHUNK = 32  # frames per launch of Rectifier.frames


def device_enabled() -> bool:
    """``TCA_DEVICE_RECTIFY=0`` keeps the definition on GPU engines too."""
    return os.environ.get("TCA_DEVICE_RECTIFY", "1") != "0"


# ------------------------------------------------------------------------------- model
def _matrix(v, name: str, shape) -> np.ndarray:
    try:
        a = np.array(v, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: not numbers") from None
    if a.size != shape[0] * shape[1]:
        raise ValueError(f"{name}: {a.size} numbers, want {shape[0]} x {shape[1]}")
    a = a.reshape(shape)
    if not np.isfinite(a).all():
        raise ValueError(f"{name}: not finite")
    a.setflags(write=False)
    return a


@dataclass(frozen=True, eq=False)
class CameraModel:
    """One camera's calibration (the fields of ``sensor_msgs/CameraInfo``)."""
    width: int
    height: int
    K: np.ndarray
    D: np.ndarray
    model: str = "plumb_bob"
    R: Optional[np.ndarray] = None  # identity
    P: Optional[np.ndarray] = field(default=None)  # [K | 0]

    def __post_init__(self):
        for name in ("width", "height"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= MAX_SIDE:
                raise ValueError(f"{name} must be an integer in 1..{MAX_SIDE}, got {v!r}")
        if self.model not in MODELS:
            raise ValueError(f"model must be one of {sorted(MODELS)}, got {self.model!r}")
        set_ = object.__setattr__
        set_(self, "K", _matrix(self.K, "K", (3, 3)))
        try:
            D = np.array(self.D, np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError("D: not numbers") from None
        if D.size not in MODELS[self.model]:
            want = " or ".join(str(c) for c in MODELS[self.model])
            raise ValueError(f"D: {D.size} coefficients, {self.model} takes {want}")
        if not np.isfinite(D).all():
            raise ValueError("D: not finite")
        D.setflags(write=False)
        set_(self, "D", D)
        set_(self, "R", _matrix(np.eye(3) if self.R is None else self.R, "R", (3, 3)))
        P = np.hstack([self.K, np.zeros((3, 1))]) if self.P is None else self.P
        set_(self, "P", _matrix(P, "P", (3, 4)))
        for name, m in (("K", self.K), ("P", self.P)):
            for i in (0, 1):
                if m[i, i] == 0:
                    raise ValueError(f"{name}[{i},{i}] (a focal length) must not be zero")


def load_camera_model(path: str) -> CameraModel:
    """The YAML ``camera_calibration`` writes and ``camera_info_manager`` reads ("ost.yaml"):
    ``image_width``, ``image_height``, ``camera_matrix.data``, ``distortion_model``,
    ``distortion_coefficients.data`` and, optional, ``rectification_matrix.data`` (identity)
    and ``projection_matrix.data`` (``[K | 0]``).  ``ValueError`` names the key of what is
    missing or wrong."""
    import yaml

    with open(path) as f:
        doc = yaml.safe_load(f)
    if not isinstance(doc, dict):
        raise ValueError(f"camera model key 'image_width' is missing in {path}")

    def data(key, required=True):
        if key not in doc:
            if required:
                raise ValueError(f"camera model key {key!r} is missing in {path}")
            return None
        v = doc[key]
        if not isinstance(v, dict) or "data" not in v:
            raise ValueError(f"camera model key '{key}.data' is missing in {path}")
        return v["data"]

    for key in ("image_width", "image_height", "distortion_model"):
        if key not in doc:
            raise ValueError(f"camera model key {key!r} is missing in {path}")
    try:
        return CameraModel(width=doc["image_width"], height=doc["image_height"], K=data("camera_matrix"),
                           D=data("distortion_coefficients"), model=doc["distortion_model"],
                           R=data("rectification_matrix", False), P=data("projection_matrix", False))
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None


def as_camera_model(m) -> Optional[CameraModel]:
    """A :class:`CameraModel`, or the path of a file :func:`load_camera_model` reads; None stays None."""
    if m is None or isinstance(m, CameraModel):
        return m
    if isinstance(m, (str, os.PathLike)):
        return load_camera_model(os.fspath(m))
    raise ValueError(f"rectify: a CameraModel or the path of a camera calibration YAML, got {type(m).__name__}")


# -------------------------------------------------------------------------- definition
def rectify_map(model: CameraModel) -> np.ndarray:
    """→ int32 [H, W, 2] ``(qx, qy)``: where in the sensor's frame, in 1/32 pixel, each pixel of
    the rectified frame comes from (the module docstring has the formulas)."""
    W, H = int(model.width), int(model.height)
    K, P, D = model.K, model.P, model.D
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    with np.errstate(all="ignore"):
        x = (u - P[0, 2]) / P[0, 0]
        y = (v - P[1, 2]) / P[1, 1]
        Rt = model.R.T
        X = Rt[0, 0] * x + Rt[0, 1] * y + Rt[0, 2]
        Y = Rt[1, 0] * x + Rt[1, 1] * y + Rt[1, 2]
        Wc = Rt[2, 0] * x + Rt[2, 1] * y + Rt[2, 2]
        x, y = X / Wc, Y / Wc
        r2 = x * x + y * y
        if model.model == "equidistant":
            k1, k2, k3, k4 = D
            r = np.sqrt(r2)
            th = np.arctan(r)
            t2 = th * th
            s = th * (1 + k1 * t2 + k2 * t2 ** 2 + k3 * t2 ** 3 + k4 * t2 ** 4) / r
            s = np.where(r == 0, 1.0, s)
            xd, yd = x * s, y * s
        else:
            k1, k2, p1, p2 = D[:4]
            k3 = D[4] if D.size > 4 else 0.0
            k4, k5, k6 = D[5:8] if D.size == 8 else (0.0, 0.0, 0.0)
            g = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
            xd = x * g + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            yd = y * g + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        mx = K[0, 0] * xd + K[0, 2]
        my = K[1, 1] * yd + K[1, 2]
        out = np.empty((H, W, 2), np.int32)
        for c, (m, side) in enumerate(((mx, W), (my, H))):
            q = np.clip(np.rint(ONE * m), LOW, ONE * (side + 1))
            out[..., c] = np.where(np.isfinite(m), q, LOW).astype(np.int32)
    return out


def _check(frame: np.ndarray, qmap: np.ndarray):
    frame, qmap = np.asarray(frame), np.asarray(qmap)
    if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
        raise ValueError(f"frame: uint8 [H, W, 3], got {frame.dtype} {frame.shape}")
    if qmap.shape != (*frame.shape[:2], 2):
        raise ValueError(f"frame {frame.shape[1]}x{frame.shape[0]} under a map for "
                         f"{qmap.shape[1]}x{qmap.shape[0]}")
    return frame, qmap.astype(np.int32, copy=False)


def rectify_numpy(frame: np.ndarray, qmap: np.ndarray) -> np.ndarray:
    """→ the rectified frame [H, W, 3] uint8: the definition, integers only.  Not bit-equal to
    ``cv2.remap``, whose bilinear weight table rounds differently (and the project does not
    depend on OpenCV); it is exactly ``floor(rectify_ref + 0.5)``."""
    frame, qmap = _check(frame, qmap)
    H, W = frame.shape[:2]
    qx, qy = qmap[..., 0], qmap[..., 1]
    ix, iy = qx >> FRAC_BITS, qy >> FRAC_BITS
    ax, ay = (qx & (ONE - 1))[..., None], (qy & (ONE - 1))[..., None]

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        s = frame[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int32)
        return np.where(ok[..., None], s, 0)

    acc = ((ONE - ax) * (ONE - ay) * tap(iy, ix) + ax * (ONE - ay) * tap(iy, ix + 1)
           + (ONE - ax) * ay * tap(iy + 1, ix) + ax * ay * tap(iy + 1, ix + 1) + (1 << (2 * FRAC_BITS - 1)))
    return (acc >> (2 * FRAC_BITS)).astype(np.uint8)


def rectify_ref(frame: np.ndarray, qmap: np.ndarray) -> np.ndarray:
    """→ float64 [H, W, 3]: bilinear interpolation of ``frame``, zero outside it, at the map's
    positions ``(qx / 32, qy / 32)``.  Every term is a dyadic rational far inside float64, so
    this is exact, and :func:`rectify_numpy` is its ``floor(. + 0.5)``."""
    frame, qmap = _check(frame, qmap)
    H, W = frame.shape[:2]
    x, y = qmap[..., 0] / float(ONE), qmap[..., 1] / float(ONE)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    padded = np.zeros((H + 2, W + 2, 3), np.float64)  # one ring of zeros
    padded[1:-1, 1:-1] = frame
    xi = np.clip(x0.astype(np.int64) + 1, 0, W)  # so that xi + 1 <= W + 1; further out is zero anyway
    yi = np.clip(y0.astype(np.int64) + 1, 0, H)
    far = ((x0 < -1) | (x0 > W - 1) | (y0 < -1) | (y0 > H - 1))[..., None]
    val = ((1 - fx) * (1 - fy) * padded[yi, xi] + fx * (1 - fy) * padded[yi, xi + 1]
           + (1 - fx) * fy * padded[yi + 1, xi] + fx * fy * padded[yi + 1, xi + 1])
    return np.where(far, 0.0, val)


# --------------------------------------------------------------------------------- GPU
def rectify_(src: torch.Tensor, dst: torch.Tensor, qmap: torch.Tensor, n: Optional[int] = None, stream=None,
             variant=None) -> None:
    """``dst[:n] <- rectified src[:n]`` with ``tca_rectify``: the launch alone (no allocation,
    copy or sync).  ``src``, ``dst``: uint8 [B, H, W, 3] on the map's GPU, contiguous, not the same
    buffer; ``qmap``: int32 [H, W, 2].  Frames ``n..B-1`` of ``dst`` are untouched.  ``variant``
    ``(chunk, byte_stores)``: the same bytes through ``tca_rectify_variant`` (measurements, tests)."""
    B, H, W = int(src.shape[0]), int(qmap.shape[0]), int(qmap.shape[1])
    n = B if n is None else int(n)
    for name, t in (("src", src), ("dst", dst)):
        if t.dtype != torch.uint8 or tuple(t.shape[1:]) != (H, W, 3) or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"{name}: contiguous uint8 [B, {H}, {W}, 3] on the GPU, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    if not 0 <= n <= min(B, int(dst.shape[0])):
        raise ValueError(f"n = {n} frames of {B} (dst holds {int(dst.shape[0])})")
    if src.data_ptr() == dst.data_ptr():
        raise ValueError("rectify_: src and dst are the same buffer")
    if qmap.dtype != torch.int32 or not qmap.is_contiguous() or qmap.device != src.device or dst.device != src.device:
        raise ValueError("rectify_: the map is contiguous int32 [H, W, 2] on the frames' GPU")
    if variant is not None:
        _native.call("tca_rectify_variant", src.data_ptr(), dst.data_ptr(), qmap.data_ptr(), H, W, n, int(variant[0]),
                     int(bool(variant[1])), _native.stream_ptr(stream))
        return
    _native.call("tca_rectify", src.data_ptr(), dst.data_ptr(), qmap.data_ptr(), H, W, n, _native.stream_ptr(stream))


class Rectifier:
    """Rectifies frames of one :class:`CameraModel`: holds its map on the host and, with a GPU,
    on the device.  :meth:`rectify_` is the launch alone, for a caller's resident frames;
    :meth:`frames` takes host arrays — one H2D, one launch and one D2H per chunk on the GPU, the
    definition on the CPU and with ``TCA_DEVICE_RECTIFY=0``."""

    def __init__(self, model: CameraModel, device="auto"):
        self.model = as_camera_model(model)
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu") if device in (None, "auto") \
            else torch.device(device)
        self.hw = (int(self.model.height), int(self.model.width))
        self.map = rectify_map(self.model)
        self.map_dev = self._stream = self._pin = self._dev = None
        self._lock = threading.Lock()
        if self.device.type == "cuda":
            self.map_dev = torch.from_numpy(self.map).to(self.device)

    @property
    def gpu(self) -> bool:
        return self.map_dev is not None and device_enabled()

    @property
    def kind(self) -> str:
        return "tca_rectify" if self.gpu else "host definition"

    def rectify_(self, src: torch.Tensor, dst: torch.Tensor, n: Optional[int] = None, stream=None) -> None:
        """The launch alone (safe inside graph capture): see :func:`rectify_`."""
        if self.map_dev is None:
            raise ValueError("Rectifier.rectify_ needs a GPU (this one is on the host: use frames())")
        rectify_(src, dst, self.map_dev, n, stream)

    def check(self, frame) -> None:
        """``ValueError`` for a frame that is not uint8 [H, W, 3] of the model's size."""
        if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
            raise ValueError(f"rectify: a frame is uint8 [H, W, 3], got {frame.dtype} {tuple(frame.shape)}")
        h, w = frame.shape[:2]
        if (h, w) != self.hw:
            raise ValueError(f"rectify: frame {w}x{h}, the camera model is {self.hw[1]}x{self.hw[0]}")

    def frames(self, frames: Sequence[np.ndarray]) -> List[np.ndarray]:
        """Per frame ([H, W, 3] uint8) its rectified frame, in input order."""
        frames = [np.asarray(f) for f in frames]
        for f in frames:
            self.check(f)
        if not self.gpu:
            return [rectify_numpy(np.ascontiguousarray(f, np.uint8), self.map) for f in frames]
        out: List[np.ndarray] = []
        H, W = self.hw
        with self._lock, torch.cuda.device(self.device):
            if self._stream is None:
                c = min(CHUNK, max(1, (256 << 20) // (H * W * 3)))
                self._stream = torch.cuda.Stream(self.device)
                self._pin = torch.empty((2, c, H, W, 3), dtype=torch.uint8).pin_memory()
                self._dev = torch.empty((2, c, H, W, 3), dtype=torch.uint8, device=self.device)
            st, pin, dev = self._stream, self._pin, self._dev
            c = pin.shape[1]
            for s in range(0, len(frames), c):
                part = frames[s:s + c]
                k = len(part)
                for j, f in enumerate(part):
                    pin[0, j].numpy()[...] = f
                with torch.cuda.stream(st):
                    dev[0, :k].copy_(pin[0, :k], non_blocking=True)
                    rectify_(dev[0], dev[1], self.map_dev, k, st)
                    pin[1, :k].copy_(dev[1, :k], non_blocking=True)
                st.synchronize()
                out += [pin[1, j].numpy().copy() for j in range(k)]
        return out
