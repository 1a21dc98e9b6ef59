"""``tca_bev_render`` (K23) against the definition of the picture, utils/bev.py render_bev_frame:
every comparison is exact equality of every byte, no tolerance and no case left out.  The entry
point is called through ``_native.call`` with guarded buffers (the structure of
tests/test_points_in_boxes_gpu.py): ``out`` is the 48-pixel-wide view of a 50-pixel-wide parent
buffer that starts as a sentinel, so the row padding, the bytes around the frames and the guards
of the level plane must come back untouched.  Each case also asserts that the definition itself
draws what the case is about, so none passes by being empty."""
import warnings

import numpy as np
import pytest
import torch

from test_decode_kernels_gpu import I32_SENT, Buf, _call
from triton_client_amd.ops import bev as obev
from triton_client_amd.ops.points_in_boxes import cloud_layout
from triton_client_amd.ros import compat, msgs
from triton_client_amd.utils import bev
from triton_client_amd.utils.bev import BevView, render_bev_frame

pytestmark = pytest.mark.gpu
F = np.float32
VIEW = BevView((0.0, 6.4), (-2.4, 2.4), 0.1, (-2.0, 2.0))  # 64 rows x 48 columns
SHORT = BevView((0.0, 0.8), (-2.4, 2.4), 0.1, (-2.0, 2.0))  # 8 rows: lower than a glyph
WP = 50  # pixels per row of the parent buffer
NS = (0, 1, 63, 64, 65, 255, 256, 257, 4097)
LAYOUTS = {"16 xyzi": (16, (0, 4, 8, 12)), "32 dwords": (32, (4, 8, 12, 16)), "21 bytes": (21, (1, 5, 9, 13)),
           "dense": None}
NAMES = ["-", "Car", "Pedestrian", "Cyclist"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


# ------------------------------------------------------------------------------ inputs
def _bits(v):
    return int(np.array(v, F).view(np.uint32))


def _last_inside(limit, lo, hi, f):
    """The float32 t in [lo, hi] (0 < lo) with the largest f(t) < limit, f non-decreasing, and its
    successor (f >= limit): a bisection over the bit patterns."""
    a, b = _bits(lo), _bits(hi)
    assert f(np.array(a, np.uint32).view(F)) < limit <= f(np.array(b, np.uint32).view(F))
    while b - a > 1:
        m = (a + b) // 2
        if f(np.array(m, np.uint32).view(F)) < limit:
            a = m
        else:
            b = m
    return np.array(a, np.uint32).view(F)[()], np.array(b, np.uint32).view(F)[()]


def _edge_points(view=VIEW):
    """(drawn, not drawn) points (x, y, z, intensity) at the borders of the view."""
    x1, y1, inv, _, _ = view.constants()
    H, W = F(view.H), F(view.W)
    xm, ym = F(3.05), F(0.05)
    # fr = (x1 - x) * inv just below H and at H: x = x1 - t
    t_in, t_out = _last_inside(H, F(1.0), F(2 * view.H / float(inv)), lambda t: (x1 - (x1 - t)) * inv)
    u_in, u_out = _last_inside(W, F(1.0), F(2 * view.W / float(inv)), lambda t: (y1 - (y1 - t)) * inv)
    drawn = [(x1, ym, 0.5, 1), (xm, y1, 0.25, 1), (x1 - t_in, ym, 0.0, 1), (xm, y1 - u_in, -0.5, 1),
             (xm, ym, -5.0, 1), (F(1.05), F(1.05), 5.0, 1)]           # below z0: 55; above z1: 255
    out = [(np.nextafter(x1, F(np.inf)), ym, 0, 1), (xm, np.nextafter(y1, F(np.inf)), 0, 1), (x1 - t_out, ym, 0, 1),
           (xm, y1 - u_out, 0, 1), (np.nan, ym, 0, 1), (xm, np.nan, 0, 1), (F(2.05), ym, np.nan, 1),
           (F(2.05), ym, np.inf, 1), (F(2.05), ym, -np.inf, 1)]
    return np.array(drawn, F), np.array(out, F)


def test_the_edge_points_are_what_they_say():
    drawn, out = _edge_points()
    for zo in (0.0, 0.25, 1.5):
        p = drawn.copy()
        p[:, 2] += F(zo)
        plane = bev.level_plane(p, VIEW, zo)
        assert (plane > 0).sum() == len(drawn) and plane[0, 23] > 0 and plane[33, 0] > 0
        assert plane[63, 23] > 0 and plane[33, 47] > 0 and plane[33, 23] == 55 and plane[53, 13] == 255
        assert not bev.level_plane(out, VIEW, zo).any()


def _points(r, n):
    """n points in and around VIEW; with room, the border points and a NaN in every column."""
    p = np.empty((n, 4), F)
    p[:, :3] = r.uniform((-0.5, -2.9, -3), (6.9, 2.9, 3), (n, 3))
    p[:, 3] = r.uniform(0, 255, n)
    if n >= 63:
        drawn, out = _edge_points()
        p[:len(drawn)] = drawn
        p[10:10 + len(out)] = out
        p[30] = (F(4.05), F(-1.05), F(1.0), np.nan)  # dropped from a cloud, drawn from dense rows
        p[31:40, :2] = (F(5.05), F(-2.05))           # nine points on one pixel
    return p


def _cloud(p, step, offs, seed=0):
    raw = np.random.default_rng(seed).integers(0, 256, (len(p), step), dtype=np.uint8)
    fields = []
    for j, name in enumerate(("x", "y", "z", "intensity")):
        raw[:, offs[j]:offs[j] + 4] = np.ascontiguousarray(p[:, j]).view(np.uint8).reshape(-1, 4)
        fields.append(msgs.PointField(name, offs[j], 7, 1))
    return msgs.PointCloud2(header=msgs.Header(), height=1, width=len(p), fields=fields, point_step=step,
                            row_step=step * len(p), data=raw.tobytes())


def _pred(boxes, scores=None, labels=None):
    boxes = np.asarray(boxes, F).reshape(-1, 7) if len(boxes) else np.zeros((0, 7), F)
    k = len(boxes)
    return {"pred_boxes": boxes, "pred_scores": np.full(k, 0.5, F) if scores is None else np.asarray(scores, F),
            "pred_labels": np.ones(k, np.int64) if labels is None else np.asarray(labels, np.int64)}


NO_BOXES = _pred([])


def _want(pts, pred, view, zo, count=None, names=NAMES):
    """The definition: ``pts`` as the painter gets them (z carries zo)."""
    return render_bev_frame(pts, None, pred["pred_boxes"], pred["pred_scores"], pred["pred_labels"], count, view,
                            names, zo)


def _want_cloud(cloud, pred, view, zo, count=None, names=NAMES):
    return _want(compat.cloud_to_numpy(cloud, z_offset=zo), pred, view, zo, count, names)


# ------------------------------------------------------------------------------ launch
class Launch:
    """One guarded launch.  ``frames``: per frame the record bytes and the point count; ``layout``:
    (step, offsets), offsets[3] == -1 for dense rows; ``tables``: per frame (table, text).
    ``frame_mis``: bytes every frame starts past a 16-byte boundary; ``out_mis``: bytes the picture
    starts past a 4-byte boundary."""

    def __init__(self, dev, frames, layout, tables, view, zo, frame_mis=0, out_mis=0):
        step, offs = layout
        ns = [n for _, n in frames]
        off, foff = 0, []
        for n in ns:
            foff.append(off + frame_mis)
            off = (off + frame_mis + n * step + 15) // 16 * 16
        host = np.zeros(off + 16, np.uint8)
        for (raw, n), fo in zip(frames, foff):
            if n:
                host[fo:fo + n * step] = np.frombuffer(raw, np.uint8, n * step)
        self.keep = [torch.from_numpy(host).to(dev)]
        assert self.keep[0].data_ptr() % 16 == 0

        def up(a, dt):
            t = torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1)).to(dev)
            self.keep.append(t)
            return t.data_ptr()

        tab, text, box_off = obev._concat_tables([t for t, _ in tables], [s for _, s in tables])
        self.B, self.H, self.W = len(frames), view.H, view.W
        self.rs, self.out_mis = 3 * WP, out_mis
        self.fs = self.H * self.rs
        assert (self.B * self.fs) % 4 == 0
        self.out = Buf(dev, self.B * self.fs // 4 + 1, "i32")
        self.plane = Buf(dev, self.B * obev.plane_words(view), "i32")
        self.text = np.frombuffer(text, np.uint8).copy()
        self.args = [self.keep[0].data_ptr(), off, up(foff, np.int64), up(ns, np.int32), self.B, max(ns, default=0),
                     step, offs[0], offs[1], offs[2], offs[3], *obev._consts(view, zo), self.H, self.W,
                     self.plane.ptr, up(box_off, np.int32), up(np.r_[tab.reshape(-1), np.zeros(12, np.int32)], np.int32),
                     len(tab), up(np.r_[self.text, np.zeros(4, np.uint8)], np.uint8), len(text),
                     self.out.ptr + out_mis, self.fs, self.rs]

    def raw(self):
        return np.ascontiguousarray(self.out.bits()).view(np.uint8)  # (asserts the guards)

    def run(self):
        try:
            _call("tca_bev_render", *self.args)
        finally:
            torch.cuda.synchronize()
        self.plane.bits()  # the workspace stays inside its guards
        raw = self.raw()
        sent = np.full(len(raw) // 4, I32_SENT, np.int32).view(np.uint8)
        a, b = self.out_mis, self.out_mis + self.B * self.fs
        assert (raw[:a] == sent[:a]).all() and (raw[b:] == sent[b:]).all(), "bytes around the frames written"
        pic = raw[a:b].reshape(self.B, self.H, WP, 3)
        pad = sent[a:b].reshape(self.B, self.H, WP, 3)
        assert (pic[:, :, self.W:] == pad[:, :, self.W:]).all(), "row padding written"
        return [pic[b, :, :self.W] for b in range(self.B)]


def _same(got, want, tag=""):
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg=f"{tag} frame {f}")


def _tables(preds, view, counts=None, names=NAMES):
    return [obev.bev_box_table(p["pred_boxes"], p["pred_scores"], p["pred_labels"],
                               None if counts is None else counts[i], view, names) for i, p in enumerate(preds)]


def _dense(p, zo):
    rows = p.copy()
    rows[:, 2] += F(zo)
    return rows


# ------------------------------------------------------------------------------ points
@pytest.fixture(scope="module")
def ragged():
    r = np.random.default_rng(11)
    return [_points(r, n) for n in NS]


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_points_every_layout_alignment_and_offset(dev, ragged, name):
    tables = _tables([NO_BOXES] * len(NS), VIEW)
    for zo in (0.0, 0.25, 1.5):
        if LAYOUTS[name] is None:  # dense rows of 4 and of 5 floats: z carries zo, no NaN-row rule
            for width in (4, 5):
                rows = [np.ascontiguousarray(np.c_[_dense(p, zo), np.zeros((len(p), width - 4), F)]) for p in ragged]
                want = [_want(q, NO_BOXES, VIEW, zo) for q in rows]
                assert want[2][23, 34, 0] > 0  # the row with a NaN intensity is drawn
                for mis in (0, 4):
                    got = Launch(dev, [(q.tobytes(), len(q)) for q in rows], (4 * width, (0, 4, 8, -1)), tables, VIEW,
                                 zo, mis, mis // 4).run()
                    _same(got, want, f"dense {width} zo {zo} +{mis}")
            continue
        step, offs = LAYOUTS[name]
        clouds = [_cloud(p, step, offs, seed=k) for k, p in enumerate(ragged)]
        want = [_want_cloud(c, NO_BOXES, VIEW, zo) for c in clouds]
        assert not want[0].any() and want[-1].any(2).sum() > 1500
        assert want[2][0, 23, 0] > 0 and want[2][63, 23, 0] > 0 and want[2][33, 0, 0] > 0 and want[2][33, 47, 0] > 0
        assert want[2][33, 23, 0] == 55 and want[2][53, 13, 0] == 255 and want[2][23, 34, 0] == 0
        for mis in (0, 4, 1):
            got = Launch(dev, [(c.data, c.width) for c in clouds], (step, offs), tables, VIEW, zo, mis, mis % 4).run()
            _same(got, want, f"{name} zo {zo} +{mis}")


def test_points_contending_for_one_packed_word(dev):
    r = np.random.default_rng(5)
    n = 4097
    p = np.empty((n, 4), F)
    col = r.integers(20, 24, n)  # columns 20..23 of row 30: one word of the plane
    p[:, 0], p[:, 1] = F(3.35), (F(2.4) - (col + 0.5) * 0.1).astype(F)
    p[:, 2], p[:, 3] = np.linspace(-2.0, 1.9, n).astype(F)[r.permutation(n)], 1.0
    plane = bev.level_plane(p, VIEW)
    assert (plane > 0).sum() == 4 and (plane[30, 20:24] > 0).all()
    t = np.floor((p[:, 2].astype(np.float64) + 2.0) * 50.0)
    assert len(np.unique(t)) > 190  # nearly every level occurs
    for c in range(20, 24):  # the pixel carries its points' maximum
        assert abs(int(plane[30, c]) - (55 + int(t[col == c].max()))) <= 1 and plane[30, c] > 240
    want = [_want(p, NO_BOXES, VIEW, 0.0)]
    tables = _tables([NO_BOXES], VIEW)
    _same(Launch(dev, [(_cloud(p, 16, (0, 4, 8, 12)).data, n)], (16, (0, 4, 8, 12)), tables, VIEW, 0.0).run(), want)
    for s in range(2):  # the same cloud shuffled: the same bytes
        q = p[np.random.default_rng(s).permutation(n)]
        _same(Launch(dev, [(_cloud(q, 16, (0, 4, 8, 12)).data, n)], (16, (0, 4, 8, 12)), tables, VIEW, 0.0).run(),
              want, f"shuffle {s}")
    asc = p[np.argsort(p[:, 2])]  # ascending levels: every point raises its pixel
    _same(Launch(dev, [(_cloud(asc, 16, (0, 4, 8, 12)).data, n)], (16, (0, 4, 8, 12)), tables, VIEW, 0.0).run(), want)


# ------------------------------------------------------------------------------- boxes
GIANT = [3.2, 0.0, 0, 1.0, 10000.0, 1, 0.01]
FEATURE_BOXES = np.array([
    [3.2, 0.0, 0, 2.0, 1.0, 1, 0.0],      # horizontal and vertical edges
    [3.2, 0.0, 0, 3.0, 1.5, 1, 0.3],      # shallow and steep edges
    [1.5, -1.0, 0, 1.0, 2.0, 1, -1.1],
    [4.0, 1.0, 0, 0.0, 0.0, 1, 0.7],      # zero size: one pixel
    [6.3, 0.0, 0, 1.0, 1.0, 1, 0.2],      # over the top border
    [0.1, 0.5, 0, 1.0, 1.0, 1, 0.5],      # the bottom
    [3.0, 2.3, 0, 1.0, 1.0, 1, 0.9],      # the left
    [2.0, -2.4, 0, 1.0, 1.0, 1, 2.0],     # the right
    [5.0, 0.5, 0, 1.0, 1.0, 1, 0.0],      # drawn,
    [np.nan, 0.5, 0, 1.0, 1.0, 1, 0.0],   # not drawn,
    [4.8, 0.3, 0, 1.0, 1.0, 1, 0.0],      # drawn over it: another label
    GIANT], F)
FEATURE_LABELS = np.array([1, 2, 3, 1, 2, 3, 1, 2, 2, 1, 3, 1])


def test_the_box_cases_are_what_they_say():
    cors = [bev.box_corners_px(b, VIEW) for b in FEATURE_BOXES]
    assert cors[9] is None and all(c is not None for i, c in enumerate(cors) if i != 9)
    kinds = set()
    neg_dy = False
    for c in cors[:3]:
        for e in range(4):
            (ax, ay), (bx, by) = sorted([tuple(c[e]), tuple(c[(e + 1) % 4])])
            dx, dy = bx - ax, by - ay
            neg_dy |= dy < 0
            kinds.add("h" if dy == 0 else "v" if dx == 0 else "shallow" if abs(dx) > abs(dy) else "steep")
    assert kinds == {"h", "v", "shallow", "steep"} and neg_dy
    assert len({tuple(p) for p in cors[3]}) == 1
    assert cors[4][:, 1].min() < 0 and cors[5][:, 1].max() >= 64 and cors[6][:, 0].min() < 0 and cors[7][:, 0].max() >= 48
    g = cors[11]
    assert g.min() == -32768 and g.max() == 32767
    n = max(abs(g[1] - g[0]))
    assert 2 * n * n > 2 ** 31  # the line rule's 2 i d term leaves 32 bits
    pic = _want(None, _pred([GIANT]), VIEW, 0.0)
    # its long sides cross the whole picture
    assert (pic == bev.label_color(1)).all(2).sum() >= 48 and (pic == bev.HEADING_COLOR).all(2).sum() >= 48
    # later colour on top, the heading colour on top of its own box
    two = _want(None, _pred(FEATURE_BOXES[[8, 10]], labels=[2, 3]), VIEW, 0.0, names=[""] * 4)
    a, b = cors[8], cors[10]
    assert tuple(two[b[0][1], b[0][0]]) == bev.HEADING_COLOR and (two == bev.label_color(2)).all(2).any()
    only_b = _want(None, _pred(FEATURE_BOXES[[10]], labels=[3]), VIEW, 0.0, names=[""] * 4)
    assert (two[only_b.any(2)] == only_b[only_b.any(2)]).all() and a is not None


def _box_frames():
    r = np.random.default_rng(21)
    many = np.c_[r.uniform(-0.5, 7, 300), r.uniform(-3, 3, 300), np.zeros(300), r.uniform(0, 2.5, (300, 2)),
                 np.ones(300), r.uniform(-7, 7, 300)].astype(F)
    many[::37, 0] = np.nan
    preds = [_pred(FEATURE_BOXES, np.linspace(0.05, 0.95, 12), FEATURE_LABELS),
             _pred(many, r.uniform(0, 1, 300), r.integers(-2, 14, 300)),
             _pred(FEATURE_BOXES[:4], labels=[1, 2, 3, 1]),             # count 0
             _pred(many[:8], r.uniform(0, 1, 8), r.integers(0, 4, 8))]  # count 5 < 8
    return preds, [None, None, 0, 5], [_points(r, n) for n in (65, 300, 64, 0)]


def test_boxes_and_labels_over_points(dev):
    preds, counts, pts = _box_frames()
    clouds = [_cloud(p, 16, (0, 4, 8, 12), seed=k) for k, p in enumerate(pts)]
    want = [_want_cloud(c, p, VIEW, 0.25, k) for c, p, k in zip(clouds, preds, counts)]
    assert (want[0] == bev.HEADING_COLOR).all(2).any() and (want[1] == bev.HEADING_COLOR).all(2).sum() > 20
    np.testing.assert_array_equal(want[2], _want_cloud(clouds[2], NO_BOXES, VIEW, 0.25))
    assert (want[3] != _want_cloud(clouds[3], preds[3], VIEW, 0.25)).any()  # boxes 5..7 would show
    tables = _tables(preds, VIEW, counts)
    assert [len(t) for t, _ in tables] == [12, 300, 0, 5]
    for out_mis in (0, 1, 3):
        got = Launch(dev, [(c.data, c.width) for c in clouds], (16, (0, 4, 8, 12)), tables, VIEW, 0.25,
                     out_mis=out_mis).run()
        _same(got, want, f"out +{out_mis}")
    # the boxes alone, one launch per box of the first frame: every edge kind on its own
    for k in range(len(FEATURE_BOXES)):
        p = _pred(FEATURE_BOXES[[k]], labels=FEATURE_LABELS[[k]])
        w = _want(None, p, VIEW, 0.0)
        assert w.any() == (k != 9)
        got = Launch(dev, [(b"", 0)], (16, (0, 4, 8, 12)), _tables([p], VIEW), VIEW, 0.0).run()
        _same(got, [w], f"box {k}")


def test_labels_clipped_on_every_side(dev):
    names = ["-", "Car", "Pedestrian", "C\x07r\xe9"]
    cases = {
        "left": _pred([[3.2, 2.6, 0, 1.0, 1.0, 1, 0.0]]),                      # origin column negative
        "right": _pred([[3.2, -1.9, 0, 1.0, 0.8, 1, 0.0]], labels=[2]),        # runs off the right edge
        "top": _pred([[6.1, 1.5, 0, 0.4, 0.4, 1, 0.0]]),                       # origin row clamped to 0
        "font": _pred([[3.2, 1.0, 0, 1.0, 1.0, 1, 0.0]], labels=[3]),          # characters outside the font
        "over": _pred([[3.2, 1.0, 0, 1.0, 1.0, 1, 0.0]] * 2, [0.25, 0.75], [1, 2]),
    }
    preds = list(cases.values())
    cor = {k: bev.box_corners_px(p["pred_boxes"][0], VIEW) for k, p in cases.items()}
    assert cor["left"][:, 0].min() + 2 < 0 and (cor["left"][:, 0] >= 0).any()
    assert cor["right"][:, 0].min() + 2 + 6 * len("Pedestrian 0.50") > 48 and 0 <= cor["top"][:, 1].min() < 11
    want = [_want(None, p, VIEW, 0.0, names=names) for p in preds]
    for k, w, p in zip(cases, want, preds):  # the label adds pixels to the boxes alone
        assert (w != _want(None, p, VIEW, 0.0, names=[""] * 4)).any() or k == "over", k
    assert (want[4] == bev.label_color(1)).all(2).any() and (want[4] == bev.label_color(2)).all(2).any()
    tables = _tables(preds, VIEW, names=names)
    assert tables[3][1] == b"C?r? 0.50"
    la = Launch(dev, [(b"", 0)] * 5, (16, (0, 4, 8, 12)), tables, VIEW, 0.0)
    _same(la.run(), want)
    # the same text with the raw bytes: the kernel prints '?' for codes outside the font
    at = sum(len(s) for _, s in tables[:3])
    raw = [(t, s) for t, s in tables]
    raw[3] = (raw[3][0], b"C\x07r\xe9 0.50")
    assert len(raw[3][1]) == len(tables[3][1]) and la.text[at:at + 4].tobytes() == b"C?r?"
    _same(Launch(dev, [(b"", 0)] * 5, (16, (0, 4, 8, 12)), raw, VIEW, 0.0).run(), want, "raw bytes")
    # a picture lower than a glyph: clipped at the bottom (and the right)
    low = [_pred([[0.5, -1.5, 0, 0.4, 1.0, 1, 0.3]], labels=[2]), _pred([[0.4, 2.0, 0, 0.2, 0.2, 1, 0.0]])]
    want = [_want(None, p, SHORT, 0.0) for p in low]
    for w, p in zip(want, low):
        assert (w[7] != _want(None, p, SHORT, 0.0, names=[""] * 4)[7]).any()  # text in the last row
    _same(Launch(dev, [(b"", 0)] * 2, (16, (0, 4, 8, 12)), _tables(low, SHORT), SHORT, 0.0).run(), want, "short view")


def test_invalid_arguments_are_refused_before_any_launch(dev):
    from triton_client_amd._native import NativeError

    r = np.random.default_rng(4)
    p = _points(r, 100)
    preds = [_pred(FEATURE_BOXES[:2])]
    # positions in the argument list: row stride, intensity offset, x offset, H, W, point step, frame stride
    for pos, bad in ((27, 3 * 48 - 1), (10, 13), (7, -1), (17, 0), (18, 32768), (6, 0), (26, 64 * 150 - 1), (10, -2)):
        la = Launch(dev, [(_cloud(p, 16, (0, 4, 8, 12)).data, 100)], (16, (0, 4, 8, 12)), _tables(preds, VIEW), VIEW, 0.0)
        la.args[pos] = bad
        with pytest.raises(NativeError):
            _call("tca_bev_render", *la.args)
        torch.cuda.synchronize()
        assert (la.out.bits() == I32_SENT).all() and (la.plane.bits() == I32_SENT).all(), (pos, bad)


# --------------------------------------------------------------------------------- op
def _op_batch():
    g = np.random.default_rng(3)
    B, N, K = 2, 200, 4
    pts = np.c_[g.uniform(0, 6.4, (B * N)), g.uniform(-2.4, 2.4, B * N), g.uniform(-2, 2, B * N),
                g.uniform(0, 1, B * N)].astype(F).reshape(B, N, 4)
    n = np.array([N, 17], np.int32)
    box = np.tile(np.array([3.2, 0.0, 0, 2.0, 1.0, 1, 0.4], F), (B, K, 1))
    box[:, :, 0] += np.arange(K, dtype=F)[None] * 0.6
    score = g.uniform(0, 1, (B, K)).astype(F)
    label = g.integers(0, 5, (B, K)).astype(np.int32)
    return [torch.from_numpy(a) for a in (pts, n, box, score, label, np.array([K, 2], np.int32))]


def test_render_bev_op_on_gpu_tensors_equals_the_cpu_op(dev):
    from triton_client_amd.ops.bev import render_bev_

    t = _op_batch()
    want = render_bev_(torch.full((2, 64, 48, 3), 7, dtype=torch.uint8), *t, VIEW, names=["a", "b"], z_offset=0.25)
    assert (want.numpy() == bev.HEADING_COLOR).all(3).any() and (want[1] != want[0]).any()
    g = [a.to(dev) for a in t]
    out = torch.full((2, 64, 48, 3), 7, dtype=torch.uint8, device=dev)
    assert render_bev_(out, *g, VIEW, names=["a", "b"], z_offset=0.25) is out
    assert torch.equal(out.cpu(), want)
    # a padded row stride; the predictions may stay on the host; n beyond max_points is clamped
    wide = torch.full((2, 64, WP, 3), 9, dtype=torch.uint8, device=dev)
    render_bev_(wide[:, :, :48], g[0], g[1], *t[2:], VIEW, names=["a", "b"], z_offset=0.25)
    assert torch.equal(wide[:, :, :48].cpu(), want) and (wide[:, :, 48:] == 9).all()
    big = torch.tensor([10 ** 6, 17], dtype=torch.int32)
    w2 = render_bev_(torch.zeros((2, 64, 48, 3), dtype=torch.uint8), t[0], big, *t[2:], VIEW, z_offset=0.25)
    o2 = render_bev_(torch.zeros((2, 64, 48, 3), dtype=torch.uint8, device=dev), g[0], big.to(dev), *g[2:], VIEW,
                     z_offset=0.25)
    assert torch.equal(o2.cpu(), w2)
    with pytest.raises(ValueError):
        render_bev_(out, t[0], *g[1:], VIEW)  # the points on another device


# ------------------------------------------------------------------- engine and driver
class _GpuEngine:
    """An engine stub with a GPU: deterministic boxes from the cloud's own points."""
    from triton_client_amd.config.lidar import PointPillarsConfig
    cfg = PointPillarsConfig()
    names = list(cfg.class_names)
    z_offset, normalize, label_base = 1.5, True, 1
    device = "cuda"

    def detect(self, clouds):
        out = []
        for c in clouds:
            p = compat.cloud_to_numpy(c)
            k = min(6, len(p))
            box = np.zeros((k, 7), F)
            box[:, 0] = 4.0 + 2.0 * np.arange(k) + F(abs(p[0, 0]) % 1.0)
            box[:, 1] = -6.0 + 2.0 * np.arange(k)
            box[:, 3:6] = (3.9, 1.6, 1.5)
            box[:, 6] = np.linspace(-1.0, 2.0, k)
            out.append({"pred_boxes": box, "pred_scores": np.linspace(0.2, 0.9, k).astype(F),
                        "pred_labels": (np.arange(k) % 3 + 1).astype(np.int64)})
        return out


class _CpuEngine(_GpuEngine):
    device = None


def _sweeps(shapes=((8, 128), (16, 128), (8, 64), (4, 64))):
    from triton_client_amd.utils.synthetic import LidarSpec, lidar_sweep
    out = []
    for s, (rings, az) in enumerate(shapes):
        pts = lidar_sweep(LidarSpec(rings=rings, azimuth_steps=az, sensor_height=1.8), s)
        out.append(compat.create_cloud_xyzi(np.frombuffer(pts.tobytes(), F).reshape(-1, 4),
                                            msgs.Header(seq=s + 1, stamp=msgs.Time(5, s), frame_id="os")))
    return out


BIG = BevView((0.0, 20.0), (-10.0, 10.0), 0.25, (-3.0, 1.0))


def test_engine_render_bev_equals_the_host_painter(dev, monkeypatch):
    from triton_client_amd.inference.engines import Detector3D

    monkeypatch.delenv("TCA_DEVICE_BEV", raising=False)
    clouds = _sweeps()
    assert len({c.width for c in clouds}) == 4
    gpu, cpu = _GpuEngine(), _CpuEngine()
    preds = gpu.detect(clouds)
    assert Detector3D.bev_painter(gpu) == "device" and Detector3D.bev_painter(cpu) == "host"
    want = Detector3D.render_bev(cpu, clouds, preds, BIG)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for _ in range(2):  # and so a second time, on the same buffers
            _same(Detector3D.render_bev(gpu, clouds, preds, BIG), want)
    assert Detector3D.bev_renderer(gpu).gpu and all((w == bev.HEADING_COLOR).all(2).any() for w in want)
    assert all((w[..., 0] == w[..., 2]).sum() > 200 and w.any(2).sum() > 200 for w in want)
    # a FLOAT64 x field: that cloud is painted on the host, with one warning
    p = np.frombuffer(clouds[0].data, F).reshape(-1, 4)
    raw = np.zeros((len(p), 24), np.uint8)
    raw[:, :8] = p[:, 0].astype(np.float64).view(np.uint8).reshape(-1, 8)
    for j, o in ((1, 8), (2, 12), (3, 16)):
        raw[:, o:o + 4] = np.ascontiguousarray(p[:, j]).view(np.uint8).reshape(-1, 4)
    c64 = msgs.PointCloud2(header=msgs.Header(seq=9), height=1, width=len(p), point_step=24, row_step=24 * len(p),
                           data=raw.tobytes(), fields=[msgs.PointField("x", 0, 8, 1), msgs.PointField("y", 8, 7, 1),
                                                       msgs.PointField("z", 12, 7, 1),
                                                       msgs.PointField("intensity", 16, 7, 1)])
    assert not obev.device_takes(cloud_layout(c64))
    mixed, mp = clouds + [c64], preds + preds[:1]
    with pytest.warns(RuntimeWarning, match="painted on the host") as rec:
        got = Detector3D.render_bev(gpu, mixed, mp, BIG)
    assert len([w for w in rec if "painted on the host" in str(w.message)]) == 1
    _same(got, want + want[:1])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _same(Detector3D.render_bev(gpu, mixed, mp, BIG), want + want[:1])


@pytest.mark.parametrize("batch,workers", [(1, 1), (2, 2)])
def test_driver_publishes_the_same_images_with_either_painter(dev, monkeypatch, batch, workers):
    from triton_client_amd.inference import RosInference3D
    from triton_client_amd.ros.bus import TopicBus

    clouds = _sweeps()
    runs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("TCA_DEVICE_BEV", mode)
        bus, eng, pics = TopicBus(), _GpuEngine(), []
        compat.Subscriber("/pc_bev", msgs.Image, pics.append, bus=bus)
        drv = RosInference3D(engine=eng, params={"sub_topic": "/pc", "pub_topic": "/pc_out"}, bus=bus, batch=batch,
                             workers=workers, queue_size=64, bev_topic="/pc_bev", bev_view=BIG)
        drv.start_inference(spin=False)
        pub = compat.Publisher("/pc", msgs.PointCloud2, bus=bus)
        for c in clouds:
            pub.publish(c)
        drv.stop()
        bus.close()
        assert (getattr(eng, "_bev_renderer", None) is not None) == (mode == "1")
        runs[mode] = [(p.header.seq, p.height, p.width, p.encoding, p.step, bytes(p.data)) for p in pics]
    assert [r[0] for r in runs["1"]] == [c.header.seq for c in clouds] and runs["1"] == runs["0"]
    assert runs["1"][0][1:5] == (BIG.H, BIG.W, "rgb8", 3 * BIG.W) and any(runs["1"][0][5])


def test_launch_replayed_in_a_graph_repaints_from_a_zeroed_plane(dev):
    r = np.random.default_rng(8)
    n = 600
    sets = [_points(r, n) for _ in range(4)]
    for k, p in enumerate(sets):  # each set in its own quarter: a plane that is not re-zeroed keeps the others
        p[:, 0] = (p[:, 0] % F(1.5)) + F(1.6 * k)
    pred = _pred(FEATURE_BOXES[:3], labels=[1, 2, 3])
    tt = obev.bev_box_table(pred["pred_boxes"], pred["pred_scores"], pred["pred_labels"], None, VIEW, NAMES)
    clouds = [_cloud(p, 16, (0, 4, 8, 12), seed=k) for k, p in enumerate(sets)]
    want = [_want_cloud(c, pred, VIEW, 0.25) for c in clouds]
    assert all((want[0] != w).any() for w in want[1:])
    ren = obev.BevRenderer(dev)
    lay = cloud_layout(clouds[0])
    call = ren.prepare([clouds[0].data], [n], lay, [tt[0]], [tt[1]], VIEW, 0.25)
    obev.launch(call)  # warm-up outside the capture
    torch.cuda.synchronize()
    np.testing.assert_array_equal(call.out[0].cpu().numpy(), want[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        obev.launch(call)
    for k in (1, 2, 3):
        new = torch.from_numpy(np.frombuffer(clouds[k].data, np.uint8).copy()).to(dev)
        call.data[call.frame_offs[0]:call.frame_offs[0] + new.numel()].copy_(new)
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(call.out[0].cpu().numpy(), want[k], err_msg=f"replay {k}")
