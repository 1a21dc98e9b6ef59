"""The bird's-eye-view picture of a batch of LiDAR frames and their detections.

CPU tensors run the host painter :func:`triton_client_amd.utils.bev.render_bev_frame`
frame by frame.  There is no device renderer yet: GPU tensors raise
:class:`~triton_client_amd._native.NativeError` (never a silent copy to the host).
"""
from __future__ import annotations

import torch

from .. import _native
from ..utils.bev import BevView, render_bev_frame


def render_bev_(out: torch.Tensor, points: torch.Tensor, n: torch.Tensor, box: torch.Tensor, score: torch.Tensor,
                label: torch.Tensor, count: torch.Tensor, view: BevView, names=None,
                z_offset: float = 0.0) -> torch.Tensor:
    """Fill ``out`` uint8 [B, H, W, 3] (rows ``out.stride(1) >= 3 * W`` bytes apart)
    with the picture of each frame.

    points [B, max_points, F >= 3] fp32 with n [B] int32 (z carries ``z_offset``
    on top of the frame ``view.z_range`` is given in); box [B, ld, D >= 7] fp32
    (yaw at index 8 when D >= 9), score [B, ld] fp32, label [B, ld] int32,
    count [B] int32; ``names[label]`` is a label's text."""
    if out.dim() != 4 or out.dtype != torch.uint8 or out.shape[3] != 3 or out.stride(3) != 1 or out.stride(2) != 3:
        raise ValueError("out must be uint8 [B, H, W, 3] with packed pixels")
    B, H, W, _ = out.shape
    if (H, W) != (view.H, view.W):
        raise ValueError(f"out is {W}x{H}, the view {view.W}x{view.H}")
    if out.stride(1) < 3 * W or (B > 1 and out.stride(0) < H * out.stride(1)):
        raise ValueError(f"out rows {out.stride(1)} B apart (< {3 * W}) or overlapping frames")
    if points.dim() != 3 or points.shape[0] != B or points.shape[2] < 3 or points.dtype != torch.float32 \
            or not points.is_contiguous():
        raise ValueError("points must be contiguous fp32 [B, max_points, >= 3]")
    if tuple(n.shape) != (B,) or n.dtype != torch.int32:
        raise ValueError("n must be int32 [B]")
    if box.dim() != 3 or box.shape[0] != B or box.shape[2] < 7 or box.dtype != torch.float32 \
            or not box.is_contiguous():
        raise ValueError("box must be contiguous fp32 [B, ld, >= 7]")
    ld = box.shape[1]
    if (tuple(score.shape) != (B, ld) or score.dtype != torch.float32 or tuple(label.shape) != (B, ld)
            or label.dtype != torch.int32 or tuple(count.shape) != (B,) or count.dtype != torch.int32
            or not score.is_contiguous() or not label.is_contiguous()):
        raise ValueError("score [B, ld] fp32, label [B, ld] int32 (contiguous) and count [B] int32")
    if any(t.device != out.device for t in (points, n, box, score, label, count)):
        raise ValueError("out, points, n, box, score, label and count must be on one device")
    if out.is_cuda:
        raise _native.NativeError("render_bev_: no device renderer; pass CPU tensors")
    nh, ch = n.numpy(), count.numpy()
    for b in range(B):
        k = max(0, min(int(ch[b]), ld))
        img = render_bev_frame(points[b].numpy(), max(0, min(int(nh[b]), points.shape[1])), box[b, :k].numpy(),
                               score[b, :k].numpy(), label[b, :k].numpy(), k, view, names, z_offset)
        out[b].copy_(torch.from_numpy(img))
    return out
