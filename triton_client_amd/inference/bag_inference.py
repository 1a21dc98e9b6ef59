"""Offline bag replay (reference ``communicator/bag_inference2d.py:22-160`` and
``communicator/bag_inference3d.py:46-184``).

Reads the sensor topic from a bag and runs the same per-frame body as the
live drivers, but ``batch`` frames at a time (one local graph replay or a
window of remote RPCs per micro-batch) instead of one blocking RPC per frame.
2D: annotated PNGs to ``out_dir/NNNN.png`` and, if ``out_bag`` is given, the
input image + annotated image + Detection2DArray written to it (the
reference opened ``output.bag`` but never wrote); with ``compressed=`` the annotated
image is a JPEG ``CompressedImage`` on ``<pub_topic>/compressed``; with ``rectify=`` every frame is
rectified from the camera's calibration first, as in the live driver; with ``tracks_topic=`` the
frames are tracked in bag order and the tracks message is written to that topic.  3D: the input cloud and
the BoundingBoxArray are written to ``<bag>_output.bag`` like the
reference.  Bag path and output dir are arguments (fixes A14);
``start_seq`` resumes a replay.
"""
from __future__ import annotations

import os
import time
from typing import Optional

from ..ros.bag import Bag
from .ros_inference import RosInference
from .ros_inference3d import ALL_OUTPUTS, RosInference3D


def _ingest(engine):
    """The data-parallel engine's ingest arena allocator (payloads deserialised
    straight into the node's host ring), or None."""
    return getattr(engine, "ingest_buffer", None)


def _readers(engine) -> int:
    """Threads reading the bag's chunks ahead into the ingest arena (with an arena only)."""
    return 8 if getattr(engine, "ingest_buffer", None) is not None else 0


def _read_kw(engine) -> dict:
    """How the bag is read for this engine: a data-parallel engine that shards by file
    (``ring_dp.file_sharding``) gets messages whose payloads stay in the mapped bag -- rank 0
    reads record headers and message prefixes, every rank reads its own shard's payloads --
    else payloads are deserialised into the ingest arena by reader threads."""
    if getattr(engine, "file_sharding", False):
        return {"mapped": True}
    return {"alloc": _ingest(engine), "readers": _readers(engine)}


def _batches(it, n):
    buf = []
    for item in it:
        buf.append(item)
        if len(buf) == n:
            yield buf
            buf = []
    if buf:
        yield buf


class BagInference2D(RosInference):
    def __init__(self, channel=None, client=None, bagfile: str = "", out_dir: Optional[str] = "./output_data",
                 out_bag: Optional[str] = None, batch: int = 8, save_png: bool = True, start_seq: int = 0,
                 max_frames: Optional[int] = None, **kw):
        super().__init__(channel, client, **kw)
        self.bagfile, self.out_dir, self.out_bag = bagfile, out_dir, out_bag
        self.batch, self.save_png, self.start_seq, self.max_frames = batch, save_png, start_seq, max_frames
        self.results = []
        self.tracks = []  # with tracks_topic: (seq, (track_id, hits, vel)) per frame
        self.elapsed = 0.0

    def start_inference(self, spin: bool = False, timeout: Optional[float] = None):
        if self.save_png and self.out_dir:
            os.makedirs(self.out_dir, exist_ok=True)
        ob = Bag(self.out_bag, "w") if self.out_bag else None
        p = self.params
        count = 0
        t0 = time.perf_counter()
        with Bag(self.bagfile) as bag:
            it = (m for _, m, _ in bag.read_messages(topics=[p["sub_topic"]], start_seq=self.start_seq,
                                                     **_read_kw(self.engine)))
            for chunk in _batches(it, self.batch):
                if self.max_frames is not None:
                    chunk = chunk[: max(0, self.max_frames - count)]
                    if not chunk:
                        break
                res = self.process(chunk)
                if self.tracks_topic:  # the frames are tracked in bag order
                    res = self.track(res)
                for m, (im, det, d, *trk) in zip(chunk, res):
                    if self.save_png and self.out_dir:
                        _save_png(os.path.join(self.out_dir, f"{count:04}.png"), im)
                    if ob is not None:
                        ob.write(p["sub_topic"], m)
                        ob.write(self.out_topic, im)  # <pub_topic>, or <pub_topic>/compressed (JPEG)
                        ob.write(p["pub_topic"] + "/detections", det)
                        if trk:
                            ob.write(self.tracks_topic, trk[0])
                    self.results.append((m.header.seq, d))
                    if trk:
                        self.tracks.append((m.header.seq, trk[1]))
                    count += 1
        self.elapsed = time.perf_counter() - t0
        if ob is not None:
            ob.close()
        return count


def _save_png(path, im) -> None:
    from PIL import Image as PILImage

    from .ros_inference import decode_image_msg

    PILImage.fromarray(decode_image_msg(im)).save(path)


def _save_depth_png(path, im) -> None:
    """A ``16UC1`` Image as a 16-bit greyscale PNG (the KITTI depth-PNG container)."""
    import numpy as np
    from PIL import Image as PILImage

    a = np.frombuffer(im.data, "<u2").reshape(im.height, im.width)
    PILImage.fromarray(a.astype(np.uint16)).save(path)


class BagInference3D(RosInference3D):
    def __init__(self, channel=None, client=None, bagfile: str = "", out_bag: Optional[str] = "", batch: int = 8,
                 start_seq: int = 0, max_frames: Optional[int] = None, verbose: bool = False,
                 bev_out: Optional[str] = None, depth_out: Optional[str] = None, **kw):
        """bev_out: a directory; every cloud's bird's-eye-view picture is saved there as
        ``NNNN.png`` (the naming of the 2D replay's ``out_dir``) and, with an output bag,
        written to it on ``bev_topic`` (default ``<pub_topic>/bev``).  With ``points_topic`` the
        labelled cloud of every input cloud is written to the output bag on that topic, and with
        ``tracks_topic`` the tracks message (the clouds are tracked in bag order).  With
        ``ranged_topic`` the bag's ``camera_detections_topic`` is read in a first pass, so the
        pairing is deterministic, and the ranged message of every cloud that has a partner is
        written on that topic.  With ``depth_topic`` every cloud's depth image is written on that
        topic; ``depth_out``: a directory where it is also saved as a 16-bit greyscale
        ``NNNN.png`` (``16UC1`` only; the topic defaults to ``<pub_topic>/depth``).  With
        ``scan_topic`` every cloud's ``LaserScan`` is written on that topic, with ``obstacles_topic``
        / ``ground_topic`` its obstacle and ground clouds."""
        if depth_out and not kw.get("depth_topic"):
            kw["depth_topic"] = ((kw.get("params") or {}).get("pub_topic") or "") + "/depth"
        super().__init__(channel, client, **kw)
        self.depth_out = depth_out or None
        if self.depth_out and self.depth_options.encoding != "16UC1":
            raise ValueError("depth_out writes 16-bit PNGs: it needs the 16UC1 encoding")
        self.bev_out = bev_out or None
        if self.bev_out and not self.bev_topic:
            self.enable_bev(self.params["pub_topic"] + "/bev", kw.get("bev_view"))
        self.bagfile, self.batch, self.start_seq, self.max_frames = bagfile, batch, start_seq, max_frames
        self.out_bag = (os.path.splitext(bagfile)[0] + "_output.bag") if out_bag == "" else out_bag
        self.verbose = verbose
        self.results = []
        self.elapsed = 0.0

    def start_inference(self, spin: bool = False, timeout: Optional[float] = None):
        p = self.params
        if self.bev_out:
            os.makedirs(self.bev_out, exist_ok=True)
        if self.depth_out:
            os.makedirs(self.depth_out, exist_ok=True)
        ob = Bag(self.out_bag, "w") if self.out_bag else None
        count = 0
        t0 = time.perf_counter()
        if self.ranged_topic:  # a first pass holds every camera message: replay misses no partner
            from ..ops.range2d import StampPairer

            with Bag(self.bagfile) as bag:
                held = [m for _, m, _ in bag.read_messages(topics=[self.camera_detections_topic])]
            self.pairer = StampPairer(capacity=max(1, len(held)))
            for m in held:
                self.pairer.push(m)
        with Bag(self.bagfile) as bag:
            it = (m for _, m, _ in bag.read_messages(topics=[p["sub_topic"]], start_seq=self.start_seq,
                                                     **_read_kw(self.engine)))
            for chunk in _batches(it, self.batch):
                if self.max_frames is not None:
                    chunk = chunk[: max(0, self.max_frames - count)]
                    if not chunk:
                        break
                res = self.process(chunk)
                if self.tracks_topic:
                    res = self.track(res)
                for m, r in zip(chunk, res):
                    if r.bev is not None and self.bev_out:
                        _save_png(os.path.join(self.bev_out, f"{count:04}.png"), r.bev)
                    if ob is not None:
                        ob.write(p["sub_topic"], m)
                        ob.write(p["pub_topic"], r.boxes)
                        for name, _ in ALL_OUTPUTS:
                            if getattr(r, name) is not None:
                                ob.write(self.side_topic(name), getattr(r, name))
                    if self.depth_out:
                        _save_depth_png(os.path.join(self.depth_out, f"{count:04}.png"), r.depth)
                    if self.verbose:
                        print(m.header.seq)
                    self.results.append((m.header.seq, r.pred))
                    count += 1
        self.elapsed = time.perf_counter() - t0
        if ob is not None:
            ob.close()
        return count
