"""``tca_points_in_boxes`` against the float32 definition of ops/points_in_boxes.py, called
through ``_native.call`` with guarded buffers (the structure of
tests/test_camera_decode_kernels_gpu.py): owner, count and every byte of the 28-byte records
equal the definition exactly — the arithmetic is the same, so no band applies."""
import warnings

import numpy as np
import pytest
import torch

from test_decode_kernels_gpu import I32_SENT, Buf, _call
from triton_client_amd.ops import points_in_boxes as pib
from triton_client_amd.ros import msgs

pytestmark = pytest.mark.gpu
F = np.float32
NS = (0, 1, 63, 64, 65, 255, 256, 257, 4097)
XYZI = (16, (0, 4, 8, 12))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _boxes(r, k):
    """k boxes in a 40 m square, many overlapping; the first is axis-aligned with dyadic faces,
    one is NaN and one has a zero dimension (they contain nothing)."""
    b = np.empty((k, 7), F)
    b[:, 0], b[:, 1], b[:, 2] = r.uniform(0, 40, k), r.uniform(-20, 20, k), r.uniform(-2, 0, k)
    b[:, 3:6] = r.uniform(0.5, 12.0, (k, 3))
    b[:, 6] = r.uniform(-7, 7, k)
    if k:
        b[0] = (8.0, -4.0, -1.0, 4.0, 2.0, 1.0, 0.0)
    if k > 3:
        b[2, 1] = np.nan
        b[3, 4] = 0.0
    sc = r.uniform(0.05, 1, k).astype(F)
    if k > 5:
        sc[5] = sc[4]  # a tie
    return b, sc, r.integers(0, 10, k).astype(np.int32)


def _points(r, n, boxes):
    """n points (x, y, z, intensity) around the boxes, some on the faces of box 0, some NaN."""
    p = np.empty((n, 4), F)
    p[:, :3] = r.uniform((0, -20, -3), (40, 20, 1), (n, 3))
    ok = np.flatnonzero(np.isfinite(boxes).all(1)) if len(boxes) else []
    if len(ok) and n:
        j = ok[r.integers(0, len(ok), n)]
        near = (boxes[j, :3] + 0.75 * boxes[j, 3:6] * r.uniform(-1, 1, (n, 3))).astype(F)
        m = r.random(n) < 0.7
        p[m, :3] = near[m]
        if n > 8:
            p[1, :3], p[2, :3], p[3, :3] = (10.0, -4.0, -1.0), (10.0, -3.0, -0.5), (np.nextafter(F(10), F(99)), -4, -1)
    p[:, 3] = r.uniform(0, 255, n)
    if n > 8:
        p[5, 0] = p[6, 2] = np.nan
        p.view(np.uint32)[7, 3] = 0x7FC12345  # a NaN payload is copied, not canonicalised
    return p


def _cloud(p, step, offs, seed=0):
    """PointCloud2 of points p in the given record layout (intensity offset -1: no such field),
    the bytes between the fields random."""
    raw = np.random.default_rng(seed).integers(0, 256, (len(p), step), dtype=np.uint8)
    fields = []
    for j, name in enumerate(("x", "y", "z", "intensity")):
        if offs[j] < 0:
            continue
        raw[:, offs[j]:offs[j] + 4] = np.ascontiguousarray(p[:, j]).view(np.uint8).reshape(-1, 4)
        fields.append(msgs.PointField(name, offs[j], 7, 1))
    return msgs.PointCloud2(header=msgs.Header(), height=1, width=len(p), fields=fields, point_step=step,
                            row_step=step * len(p), data=raw.tobytes())


def _want(clouds, boxes):
    return [pib.label_numpy(c, b, s, lb) for c, (b, s, lb) in zip(clouds, boxes)]


class Launch:
    """One guarded launch over same-layout clouds.  ``frame_mis``: bytes every frame starts past a
    16-byte boundary; ``base_mis``: bytes the data pointer lies past one."""

    def __init__(self, dev, clouds, boxes, frame_mis=0, base_mis=0):
        lay = pib.cloud_layout(clouds[0])
        step, ns = lay.point_step, [c.width * c.height for c in clouds]
        off, foff = 0, []
        for n in ns:
            foff.append(off + frame_mis)
            off = (off + frame_mis + n * step + 15) // 16 * 16
        host = np.zeros(off + 64, np.uint8)
        for c, n, fo in zip(clouds, ns, foff):
            host[base_mis + fo: base_mis + fo + n * step] = np.frombuffer(c.data, np.uint8)
        self.keep = [torch.from_numpy(host).to(dev)]
        assert self.keep[0].data_ptr() % 16 == 0
        nb = [len(b) for b, _, _ in boxes]
        self.ns, self.nb, self.K, self.total = ns, nb, sum(nb), sum(ns)

        def up(a, dt):
            t = torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1)).to(dev)
            self.keep.append(t)
            return t.data_ptr()

        tab = np.concatenate([pib.box_table(b, s) for b, s, _ in boxes] + [np.zeros((1, 8), F)])
        self.owner, self.count = Buf(dev, self.total, "i32"), Buf(dev, self.K, "i32")
        self.rec = Buf(dev, 7 * self.total, "i32")
        o = lay.offsets
        self.args = (self.keep[0].data_ptr() + base_mis, up(foff, np.int64), up(ns, np.int32), len(clouds),
                     max(ns, default=0), step, o[0], o[1], o[2], o[3], up(np.r_[0, np.cumsum(nb)], np.int32),
                     up(tab, F), up(np.concatenate([s for _, s, _ in boxes] + [np.zeros(1, F)]), F),
                     up(np.concatenate([lb for _, _, lb in boxes] + [np.zeros(1, np.int32)]), np.int32), self.K,
                     up(np.r_[0, np.cumsum(ns)], np.int32), self.owner.ptr, self.count.ptr, self.rec.ptr)

    def run(self):
        try:
            _call("tca_points_in_boxes", *self.args)
        finally:
            torch.cuda.synchronize()
        owner, count, rec = self.owner.bits(), self.count.bits(), self.rec.bits()  # (asserts the guards)
        out, po, ko = [], 0, 0
        for n, k in zip(self.ns, self.nb):
            out.append((owner[po:po + n], count[ko:ko + k], rec[7 * po:7 * (po + n)].tobytes()))
            po, ko = po + n, ko + k
        return out


def _same(got, want, tag=""):
    assert len(got) == len(want)
    for f, ((o, c, p), (wo, wc, wp)) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(o, wo, err_msg=f"owner {tag} frame {f}")
        np.testing.assert_array_equal(c, wc, err_msg=f"count {tag} frame {f}")
        assert p == wp, f"payload {tag} frame {f}"


@pytest.fixture(scope="module")
def chunk():
    from triton_client_amd import _native
    c = _native.kernels().tca_points_in_boxes_chunk()
    assert c == pib.CHUNK
    return c


@pytest.mark.parametrize("kind", ["0", "1", "2", "chunk-1", "chunk", "chunk+1"])
def test_every_n_against_the_definition(dev, chunk, kind):
    k = {"0": 0, "1": 1, "2": 2, "chunk-1": chunk - 1, "chunk": chunk, "chunk+1": chunk + 1}[kind]
    r = np.random.default_rng(k)
    boxes = [_boxes(r, k) for _ in NS]
    clouds = [_cloud(_points(r, n, b[0]), *XYZI) for n, b in zip(NS, boxes)]
    want = _want(clouds, boxes)
    got = Launch(dev, clouds, boxes).run()
    _same(got, want, f"K={k}")
    if k >= 2:
        big = want[-1]
        # the generator's own sanity: 70 % of the points lie within +-0.75 dims of a box, (2/3)^3 of them inside
        assert (big[0] >= 0).sum() > 400 and big[0][1] >= 0 and big[0][2] >= 0  # (points 1, 2: a face, an edge)
        assert k < 100 or big[1].sum() > (big[0] >= 0).sum()  # many boxes overlap: count counts non-owners too


def test_ragged_batch_with_an_empty_frame_and_a_frame_without_boxes(dev, chunk):
    r = np.random.default_rng(7)
    boxes = [_boxes(r, chunk + 40), _boxes(r, 9), _boxes(r, 0), _boxes(r, 3)]
    ns = [700, 0, 300, 129]
    clouds = [_cloud(_points(r, n, boxes[0][0]), *XYZI) for n in ns]
    want = _want(clouds, boxes)
    got = Launch(dev, clouds, boxes).run()
    _same(got, want)
    assert (got[2][0] == -1).all() and len(got[2][2]) == 28 * 300 and got[1][1].tolist() == [0] * 9
    # the labeler (one pinned upload, own stream and workspace) gives the same, and so a second time
    lab = pib.PointLabeler(dev)
    for _ in range(2):
        res = lab.label(clouds, *[[b[j] for b in boxes] for j in range(3)])
        _same([(o, c, p) for o, c, p in res], want, "PointLabeler")


LAYOUTS = {"16 xyzi": (16, (0, 4, 8, 12)), "20 shuffled": (20, (8, 12, 4, 0)), "32 shuffled": (32, (16, 4, 24, 8)),
           "16 no intensity": (16, (0, 4, 8, -1)), "18 unaligned fields": (18, (1, 6, 10, 14))}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layouts_and_alignments_give_the_same_bytes(dev, name):
    step, offs = LAYOUTS[name]
    r = np.random.default_rng(step)
    boxes = [_boxes(r, 20), _boxes(r, 7)]
    pts = [_points(r, n, boxes[0][0]) for n in (513, 64)]
    clouds = [_cloud(p, step, offs, seed=k) for k, p in enumerate(pts)]
    want = _want(clouds, boxes)
    if offs[3] < 0:
        assert all((np.frombuffer(w[2], pib.RECORD_DTYPE)["intensity"] == 0).all() for w in want)
    # 16-byte aligned, 4-byte aligned and 1-byte misaligned frame offsets; a misaligned base pointer
    for frame_mis, base_mis in ((0, 0), (4, 0), (1, 0), (0, 1), (15, 1), (0, 4)):
        _same(Launch(dev, clouds, boxes, frame_mis, base_mis).run(), want, f"{name} +{frame_mis} base +{base_mis}")


def test_second_launch_on_the_same_buffers_gives_the_same_counts(dev):
    r = np.random.default_rng(3)
    boxes = [_boxes(r, 30)]
    clouds = [_cloud(_points(r, 3000, boxes[0][0]), *XYZI)]
    la = Launch(dev, clouds, boxes)
    first = la.run()
    assert first[0][1].sum() > 1000
    _same(la.run(), first, "second launch")  # zeroed per launch, not accumulated
    _same(first, _want(clouds, boxes))


def test_refused_layouts(dev):
    from triton_client_amd._native import NativeError

    r = np.random.default_rng(4)
    boxes = [_boxes(r, 4)]
    clouds = [_cloud(_points(r, 100, boxes[0][0]), *XYZI)]
    for pos, bad in ((5, 0), (6, -1), (8, 14), (9, -2)):  # step 0, x absent, z past the record, intensity -2
        la = Launch(dev, clouds, boxes)
        la.args = la.args[:pos] + (bad,) + la.args[pos + 1:]
        with pytest.raises(NativeError):
            _call("tca_points_in_boxes", *la.args)
        torch.cuda.synchronize()
        assert (la.owner.bits() == I32_SENT).all() and (la.rec.bits() == I32_SENT).all()
    # FLOAT64 x: the labeler falls back to the definition and says so, once
    p = _points(r, 200, boxes[0][0])
    raw = np.zeros((200, 24), np.uint8)
    raw[:, :8] = p[:, 0].astype(np.float64).view(np.uint8).reshape(-1, 8)
    for j, o in ((1, 8), (2, 12), (3, 16)):
        raw[:, o:o + 4] = np.ascontiguousarray(p[:, j]).view(np.uint8).reshape(-1, 4)
    c64 = msgs.PointCloud2(height=1, width=200, point_step=24, row_step=4800, data=raw.tobytes(),
                           fields=[msgs.PointField("x", 0, 8, 1), msgs.PointField("y", 8, 7, 1),
                                   msgs.PointField("z", 12, 7, 1), msgs.PointField("intensity", 16, 7, 1)])
    lab = pib.PointLabeler(dev)
    args = ([c64], [boxes[0][0]], [boxes[0][1]], [boxes[0][2]])
    with pytest.warns(RuntimeWarning, match="labelled on the host"):
        res = lab.label(*args)
    _same(res, _want([c64], boxes))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _same(lab.label(*args), _want([c64], boxes))


def test_engine_label_points_equals_the_cpu_engine(dev):
    from triton_client_amd.inference import LocalDetector3D
    from triton_client_amd.ros import compat
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep

    pts = np.frombuffer(lidar_sweep(LidarSpec(rings=16, azimuth_steps=128, sensor_height=1.8), 0).tobytes(),
                        F).reshape(-1, 4)
    assert len(pts) == 2048
    cloud = compat.create_cloud_xyzi(pts, msgs.Header(seq=1))
    ok = pts[~np.isnan(pts).any(1)]
    box = np.zeros((12, 7), F)
    box[:, :3] = ok[::len(ok) // 12][:12, :3]
    box[:, 3:6], box[:, 6] = (5.0, 3.0, 2.5), np.linspace(-3, 3, 12)
    pred = {"pred_boxes": box, "pred_scores": np.linspace(0.1, 0.9, 12).astype(F),
            "pred_labels": (np.arange(12) % 3 + 1).astype(np.int64)}
    idx = [np.arange(2, 12)]
    gpu, cpu = LocalDetector3D(device=dev), LocalDetector3D(device="cpu")
    assert gpu.point_labeler().gpu and not cpu.point_labeler().gpu
    got, want = gpu.label_points([cloud], [pred], idx), cpu.label_points([cloud], [pred], idx)
    _same(got, want)
    assert (want[0][0] >= 0).sum() > 50 and want[0][0].max() < 10
