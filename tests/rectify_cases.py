"""Camera models shared by the rectification tests (``test_rectify.py``, ``test_rectify_gpu.py``).

Every distorted model's rectified view is wider than the sensor's (``P``'s focal length is below
``K``'s), so its map leaves the frame on all four sides: it holds entries whose taps straddle each
edge and entries at both clip values (``coverage`` counts them, and the tests assert on it)."""
import numpy as np

from triton_client_amd.ops.rectify import LOW, ONE, CameraModel

_D = {
    "barrel": ("plumb_bob", [-0.32, 0.09, 0.002, -0.001, -0.01]),
    "pincushion": ("plumb_bob", [0.21, 0.05, -0.001, 0.0015]),  # four coefficients: k3 = 0
    "rational": ("rational_polynomial", [0.9, -0.4, 0.001, -0.002, 0.05, 1.2, -0.3, 0.02]),
    "equidistant": ("equidistant", [-0.04, 0.006, -0.002, 0.0004]),
}
DISTORTED = tuple(_D)


def model(name: str, H: int, W: int) -> CameraModel:
    """``name``: one of :data:`DISTORTED`, or ``"identity"`` (no distortion, ``R = I``, ``P = [K|0]``)."""
    f = 0.62 * W
    cx, cy = 0.48 * (W - 1) + 0.37, 0.53 * (H - 1) - 0.21
    K = np.array([[f, 0, cx], [0, 1.03 * f, cy], [0, 0, 1]])
    if name == "identity":
        return CameraModel(width=W, height=H, K=K, D=[0, 0, 0, 0, 0])
    kind, D = _D[name]
    a, b = np.deg2rad(1.3), np.deg2rad(-0.8)  # a small rectifying rotation about x, then y
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    P = np.array([[0.55 * f, 0, (W - 1) / 2 + 0.3, 0], [0, 0.57 * f, (H - 1) / 2 - 0.4, 0], [0, 0, 1, 0]])
    return CameraModel(width=W, height=H, K=K, D=D, model=kind, R=Ry @ Rx, P=P)


def coverage(qmap: np.ndarray) -> dict:
    """How many entries of a map exercise each special case of the definition."""
    H, W = qmap.shape[:2]
    qx, qy = qmap[..., 0].astype(np.int64), qmap[..., 1].astype(np.int64)
    ix, iy, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
    in_x, in_y = (ix >= 0) & (ix < W), (iy >= 0) & (iy < H)
    return {"left": int(((ix == -1) & (ax > 0) & in_y).sum()), "right": int(((ix == W - 1) & (ax > 0) & in_y).sum()),
            "top": int(((iy == -1) & (ay > 0) & in_x).sum()), "bottom": int(((iy == H - 1) & (ay > 0) & in_x).sum()),
            "clip_low": int(((qx == LOW) | (qy == LOW)).sum()),
            "clip_high": int(((qx == ONE * (W + 1)) | (qy == ONE * (H + 1))).sum()),
            "half": int(((ax == 16) & (ay == 16) & in_x & in_y).sum()),
            "last": int(((ax == 31) & (ay == 31) & in_x & in_y).sum())}
