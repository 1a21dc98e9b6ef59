"""3D LiDAR pipeline on one GPU: raw PointCloud2 payloads → 3D boxes.

    PointCloud2 bytes ─K6 unpack (skip NaN, i/=max, z+=offset)→ points
    ─K7 voxelise (spconv order)→ sorted slot lists ─K8/K9 MFMA PillarVFE +
    scatter→ NHWC BEV canvas ─BEV backbone + anchor head (channels_last)→
    cls/box/dir maps ─K11 decode/filter→ candidates ─K10 top-4096 +
    rotated-IoU NMS→ boxes [B,500,7], scores, labels, counts

``precision="fp32"`` (default; the reference serves PointPillars in fp32,
``examples/pointpillar_kitti/config.pbtxt:33,54``): fp32 canvas and
activations, split-product MFMA convs and fused neck; ``"bf16"``: bf16.

The reference splits this across a client (``communicator/ros_inference3d.py:120-213``:
138 ms Python ``read_points``, OpenPCDet/spconv CPU voxeliser, three
``tobytes`` copies, gRPC) and a Triton Python-backend server running
OpenPCDet on the CPU (``examples/pointpillar_kitti/config.pbtxt:73`` KIND_CPU).
Here it is one captured hipGraph; the [V,32,4] voxel tensor is never
materialised (the VFE kernel gathers from the voxeliser's slot lists).
"""
from __future__ import annotations

import os

from typing import Optional

import torch

from ..config.lidar import PointPillarsConfig
from ..models.common import fuse_model, lsuv_rescale
from ..models.pointpillars import PointPillars, build_pointpillars
from ..ops._ws import Workspace
from ..ops.conv import act_dtype
from ..ops.lidar import AnchorPostprocess, PillarEncoder, PointLayout, Voxelizer, pc2_unpack

# the per-frame canvas clear resets only the previous frame's occupancy bytes when the fast plan's
# first conv gates its loads on them (TCA_LAZY_CANVAS=0: clear the features too, for A/B runs)
LAZY_CANVAS_CLEAR = os.environ.get("TCA_LAZY_CANVAS", "1") != "0"


def calibrate_on_cloud(pipe, payload: torch.Tensor, npoints: int, target: float) -> None:
    """Set a random-init head prior from one cloud: its payload bytes (uint8) go into every
    frame slot of ``pipe`` (any of the LiDAR families' pipelines), then
    ``calibrate_detection_density(target)`` runs on them."""
    raw = payload[:min(payload.numel(), pipe.frame_bytes)]
    for b in range(pipe.B):
        pipe.data[b * pipe.frame_bytes: b * pipe.frame_bytes + raw.numel()].copy_(raw)
    pipe.frame_n.fill_(min(npoints, pipe.max_points))
    pipe.calibrate_detection_density(target)


class LidarPipeline:
    def __init__(self, model: Optional[PointPillars] = None, batch: int = 16, max_points: int = 131072,
                 layout: Optional[PointLayout] = None, z_offset: float = 1.5, normalize_intensity: bool = True,
                 precision: str = "fp32", device="cuda", cfg: Optional[PointPillarsConfig] = None,
                 seed: int = 0, fast: bool = True):
        self.device = torch.device(device)
        self.precision = precision
        dtype = act_dtype(precision)
        self.B, self.max_points, self.dtype = batch, max_points, dtype
        self.layout = layout or PointLayout.xyzi_f32()
        self.z_offset, self.normalize = z_offset, normalize_intensity
        if model is None:
            model = build_pointpillars(cfg, seed)
        model = fuse_model(model.eval())
        self.cfg = model.cfg
        self.model = model.to(device=self.device, dtype=dtype, memory_format=torch.channels_last)
        self.frame_bytes = max_points * self.layout.point_step
        # static inputs: B payload slots of frame_bytes each + per-frame point counts
        self.data = torch.zeros(batch * self.frame_bytes, dtype=torch.uint8, device=self.device)
        self.frame_off = torch.arange(batch, dtype=torch.int64, device=self.device) * self.frame_bytes
        self.frame_n = torch.zeros(batch, dtype=torch.int32, device=self.device)
        self.ws = Workspace(self.device)
        v = self.cfg.voxel
        self.vox = Voxelizer(v, batch, max_points, device=self.device, materialize=False)
        self.enc = PillarEncoder(v, model.vfe.fused_weight.float(), model.vfe.fused_bias.float(), batch,
                                 device=self.device, channels=self.cfg.vfe_filters, dtype=dtype)
        self.post = AnchorPostprocess(self.cfg, batch, device=self.device)
        self.use_fast = fast and self.device.type == "cuda"
        self.fast = None

    def build_fast(self):
        from ..models.fast import FastBEV
        self.fast = FastBEV(self.model, self.B, self.device, precision=self.precision)
        # fp32 mode: the scatter writes the pair storage the plan reads; the plan's first conv
        # gates its canvas loads on the occupancy bytes, so a frame's clear resets only those
        self.enc.set_pair(self.fast.pair)
        self.enc.set_occ_gated(LAZY_CANVAS_CLEAR and self.fast.first_conv_gated())
        return self.fast

    @torch.no_grad()
    def calibrate_detection_density(self, target_per_frame: float = 2000.0, lsuv: bool = True) -> float:
        """Shift the class-logit bias so ~target anchors per frame reach the
        score filter (>= SCORE_THRESH) on the current sweeps — what a trained
        detector typically hands to the 4096-pre / 500-post rotated NMS.
        Random-init weights otherwise leave every score near the 0.01 prior
        and the NMS stage idle.  Returns the shift."""
        pts, cnt = pc2_unpack(self.ws, self.data, self.frame_off, self.frame_n, self.layout, self.max_points,
                              self.normalize, self.z_offset)
        self.enc.clear(self.vox)
        self.vox.assign(pts, cnt)
        pair = self.enc.pair
        self.enc.set_pair(False)  # the PyTorch module reads plain fp32
        canvas = self.enc.encode_from_slots(pts, self.vox)
        self.vox.finish(pts, cnt, gather=False)
        self.enc.set_pair(pair)  # (the next frame's scatter; its clear zeroes these cells)
        if lsuv:
            h = self.model.head
            lsuv_rescale(self.model, lambda: self.model.bev_forward(canvas), head_modules=[h.conv_cls, h.conv_dir])
            h.conv_cls.bias.fill_(-4.59)  # restore the 0.01 prior; the shift below sets the density
        cls, _, _ = self.model.bev_forward(canvas)
        B = cls.shape[0]
        C = self.cfg.num_classes
        m = cls.float().permute(0, 2, 3, 1).reshape(B, -1, C).max(-1).values
        t = self.cfg.score_thresh

        def count(d):
            return (torch.sigmoid(m + d) >= t).float().sum(1).mean().item()

        lo, hi = -30.0, 30.0
        for _ in range(50):
            mid = 0.5 * (lo + hi)
            if count(mid) > target_per_frame:
                hi = mid
            else:
                lo = mid
        d = 0.5 * (lo + hi)
        self.model.head.conv_cls.bias += d
        self.calibration_shift = d
        return d

    @torch.no_grad()
    def step(self):
        canvas = self.step_pre()
        return self.step_post(canvas)

    @torch.no_grad()
    def step_pre(self):
        """Unpack + voxelise + PillarVFE scatter into this pipeline's canvas (capture-safe).
        The two halves let a caller run the next batch's preprocessing beside this one's
        network (bench.py --lidar-pipeline: two pipelines alternating)."""
        if self.use_fast and self.fast is None:
            self.build_fast()  # sets the canvas storage first
        pts, cnt = pc2_unpack(self.ws, self.data, self.frame_off, self.frame_n, self.layout, self.max_points,
                              self.normalize, self.z_offset)
        self.enc.clear(self.vox)  # previous frame's pillars (coords still hold them)
        self.vox.assign(pts, cnt)
        canvas = self.enc.encode_from_slots(pts, self.vox)
        self.vox.finish(pts, cnt, gather=False)
        return canvas

    @torch.no_grad()
    def step_front(self, neck_back: bool = False, blocks_front: Optional[int] = None):
        """Preprocessing + BEV network; the head maps stay in this pipeline's plan buffers
        for step_back (bench.py --lidar-pipeline 2: the decode / rotated NMS of one batch,
        a few low-occupancy kernels, runs beside the next batch's network).  neck_back
        (--lidar-pipeline 3): stop after the down blocks; step_back runs the fused neck +
        head as well.  blocks_front (--lidar-pipeline 4): only the first blocks_front down
        blocks here; step_back runs the rest before the neck."""
        self.step_pre()
        self.step_blocks(neck_back, blocks_front)

    @torch.no_grad()
    def step_blocks(self, neck_back: bool = True, blocks_front: Optional[int] = None,
                    mark: Optional[tuple] = None):
        """The BEV network over the canvas the last step_pre filled (the down blocks only with
        neck_back; step_back finishes the batch).  bench.py --lidar-pipeline 5 runs it alone on the
        critical stream: this pipeline's next step_pre then runs after its step_back, beside the
        other pipeline's blocks.  mark = (n, event): record the event on the current stream once
        the first n convs of the down blocks are issued (the other pipeline's next front waits for it, so that
        the voxeliser runs beside blocks 2-3 instead of block 1's full-register-file convs;
        ``self.fast.bb.convs_before(blocks)`` gives n for whole blocks)."""
        self._blocks = self._head = None
        if self.use_fast and neck_back and self.fast.neck is not None:
            self._blocks = self.fast.forward_blocks(self.enc.canvas_nhwc(), blocks_front, mark=mark)
        elif self.use_fast:
            self._head = self.fast.forward(self.enc.canvas_nhwc())
        else:
            self._head = self.model.bev_forward(self.enc.canvas_nchw())

    @torch.no_grad()
    def step_back(self):
        """(Neck + head, then) decode + rotated NMS of what the last step_front left."""
        head = self._head if self._blocks is None else self.fast.forward_neck(self._blocks)
        return self.post(*head)

    @torch.no_grad()
    def step_post(self, canvas=None):
        """BEV network + decode + rotated NMS over the canvas step_pre filled."""
        if self.use_fast:
            f = self.fast or self.build_fast()
            return self.post(*f.forward(self.enc.canvas_nhwc()))
        cls, box, dir_ = self.model.bev_forward(canvas if canvas is not None else self.enc.canvas_nchw())
        return self.post(cls, box, dir_)
