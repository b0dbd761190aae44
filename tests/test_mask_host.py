"""Human and text masks, host side: the restatement of tests/mask_reference.py held to hand-worked cases (strict thresholds, ties, class
offsets, 0 / 0, the ratio threshold, NumPy's slice rules), its rescale pinned to torch's in-place ops, the letterbox geometry, the host
logic of storygen_amd.mask on emulated ops, and the refusals of ops and of the C entry points (nothing is launched, nothing written)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import mask_reference as R
from tests.mask_ops_emulation import patched_mask_ops

F = np.float32


def _cand(rows):
    """(x1, y1, x2, y2, conf, cls) rows already in score order."""
    return np.asarray(rows, dtype=F).reshape(-1, 6)


def _pred(rows, nc):
    """(x1, y1, x2, y2, obj, best class, class score) -> a [A, 5 + nc] prediction in xywh."""
    p = np.zeros((len(rows), 5 + nc), F)
    for a, (x1, y1, x2, y2, obj, cls, score) in enumerate(rows):
        p[a, :5] = ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, obj)
        p[a, 5 + cls] = score
    return p


# ------------------------------------------------------------------------------------------------------------------ NMS, by hand
def test_iou_exactly_at_the_threshold_keeps_both_and_just_above_drops_the_lower_score():
    # [0, 4] x [0, 3] and [2, 6] x [0, 3]: inter 6, union 12 + 12 - 6 = 18 ... use 2/3 overlap: [0, 3] and [1, 4] wide, 1 high: inter 2, union 4
    c = _cand([[0, 0, 3, 1, 0.9, 0], [1, 0, 4, 1, 0.8, 0]])
    assert R.nms(c, 0.5).tolist() == [0, 1]                          # 2 / 4 = 0.5 exactly, `>` is strict
    assert R.nms(c, float(np.nextafter(F(0.5), F(0)))).tolist() == [0]
    c2 = _cand([[0, 0, 4, 1, 0.9, 0], [1, 0, 4, 1, 0.8, 0]])          # inter 3, union 4: 0.75
    assert R.nms(c2, 0.5).tolist() == [0]


def test_equal_scores_keep_anchor_order():
    p = _pred([(0, 0, 4, 4, 0.9, 0, 1.0), (100, 100, 104, 104, 0.9, 0, 1.0), (1, 0, 5, 4, 0.9, 0, 1.0)], nc=2)
    cand = R.select(p, 0.5)
    assert cand[:, 0].tolist() == [0.0, 100.0, 1.0]                  # all 0.9: anchor order
    assert R.nms(cand, 0.5).tolist() == [0, 1]                       # the third overlaps the first (12 / 20) and came later


def test_classes_do_not_suppress_each_other_unless_agnostic():
    c = _cand([[0, 0, 4, 4, 0.9, 0], [0, 0, 4, 4, 0.8, 1]])
    assert R.nms(c, 0.5).tolist() == [0, 1]
    assert R.nms(c, 0.5, agnostic=True).tolist() == [0]


def test_two_empty_boxes_divide_zero_by_zero_and_both_stay():
    c = _cand([[5, 5, 5, 5, 0.9, 0], [5, 5, 5, 5, 0.8, 0]])
    assert R.nms(c, 0.0).tolist() == [0, 1]


def test_max_det_cuts_the_kept_list():
    c = _cand([[10 * k, 0, 10 * k + 5, 5, 1.0 - 0.01 * k, 0] for k in range(7)])
    assert R.nms(c, 0.5, max_det=3).tolist() == [0, 1, 2]


# ------------------------------------------------------------------------------------------------------------------ select, by hand
def test_single_class_uses_obj_and_best_class_tie_takes_the_first():
    p1 = np.array([[10, 10, 4, 4, 0.7, 0.1], [10, 10, 4, 4, 0.4, 0.9]], F)
    c = R.select(p1, 0.5)
    assert c.shape == (1, 6) and c[0, 4] == F(0.7) and c[0, 5] == 0 and c[0, :4].tolist() == [8, 8, 12, 12]
    p3 = np.array([[10, 10, 4, 4, 1.0, 0.2, 0.8, 0.8]], F)
    assert R.select(p3, 0.5)[0, 5] == 1
    assert len(R.select(p3, 0.5, classes=(2,))) == 0 and len(R.select(p3, 0.5, classes=(1, 2))) == 1


def test_select_thresholds_are_strict_and_nan_drops():
    p = np.array([[1, 1, 2, 2, 0.5, 1.0, 0.0],                       # obj == conf_thres: out
                  [1, 1, 2, 2, 1.0, 0.5, 0.0],                       # conf == conf_thres: out
                  [1, 1, 2, 2, np.nan, 1.0, 0.0],
                  [1, 1, 2, 2, 1.0, np.nan, 0.9],
                  [np.nan, 1, 2, 2, 1.0, 0.9, 0.0]], F)              # a NaN box passes the filter
    c = R.select(p, 0.5)
    assert len(c) == 1 and np.isnan(c[0, 0]) and np.isnan(c[0, 2]) and c[0, 1] == 0 and c[0, 3] == 2


def test_max_nms_keeps_the_best_scores():
    p = _pred([(0, 0, 1, 1, 1.0, 0, 0.6 + 0.01 * (k % 5)) for k in range(12)], nc=1 + 1)
    c = R.select(p, 0.5, max_nms=4)
    assert len(c) == 4 and c[:, 4].tolist() == [F(0.6 + 0.01 * 4)] * 2 + [F(0.6 + 0.01 * 3)] * 2


# ------------------------------------------------------------------------------------------------------------------ rescale, pinned
GEOMETRIES = [((384, 640), (720, 1280)), ((640, 384), (1280, 720)), ((384, 640), (480, 854))]


@pytest.mark.parametrize("input_shape,frame_shape", GEOMETRIES)
def test_rescale_is_torchs_inplace_arithmetic_and_the_fp32_formula(input_shape, frame_shape):
    """R.rescale runs torch's own `-=`, `/=`, clamp_, round on the CPU; the kernels' formula — subtract fp32(pad), divide by fp32(gain), clamp,
    round half to even — gives the same bits on 200 000 values, and the multiply-by-reciprocal form does not."""
    rng = np.random.default_rng(3)
    v = (rng.random((50000, 4)) * 800 - 80).astype(F)
    want = R.rescale(v, input_shape, frame_shape)
    pad_x, pad_y, gain = (F(t) for t in R.scale_geometry(input_shape, frame_shape))
    h0, w0 = frame_shape
    got, recip = np.empty_like(v), np.empty_like(v)
    for k, (pad, hi) in enumerate(((pad_x, w0), (pad_y, h0), (pad_x, w0), (pad_y, h0))):
        got[:, k] = np.rint(np.clip((v[:, k] - pad) / gain, 0, hi))
        recip[:, k] = (v[:, k] - pad) * (F(1) / gain)
    assert got.tobytes() == want.tobytes()
    unrounded = np.stack([(v[:, k] - (pad_x, pad_y)[k % 2]) / gain for k in range(4)], 1)
    if np.frexp(gain)[0] != 0.5:                                     # (a power-of-two gain has an exact reciprocal)
        assert (recip != unrounded).mean() > 0.01
    # half to even, the clamp edges, NaN -> 0
    g = ((640, 640), (1280, 1280))                                   # gain 0.5, pad 0: quotients land on .5
    e = R.rescale(np.array([[0.25, 0.75, 1.25, 1.75], [-3, 640, 641, np.nan], [np.inf, -np.inf, 639.75, 320.25]], F), *g)
    assert e.tolist() == [[0, 2, 2, 4], [0, 1280, 1280, 0], [1280, 0, 1280, 640]]


# ------------------------------------------------------------------------------------------------------------------ painter, by hand
def test_ratio_exactly_at_the_threshold_is_not_removed():
    p20 = _pred([(0, 0, 10, 2, 0.9, 0, 1.0)], nc=2)
    m, det, ratio, removed = R.human_text_mask(p20, (10, 10), (10, 10))
    assert ratio == 0.2 and not removed and m is not None and int(m.sum()) == 20 * 3 * 255 and det[0, :4].tolist() == [0, 0, 10, 2]
    p21 = _pred([(0, 0, 10, 2, 0.9, 0, 1.0), (0, 5, 1, 6, 0.8, 0, 1.0)], nc=2)
    m, det, ratio, removed = R.human_text_mask(p21, (10, 10), (10, 10))
    assert ratio == 0.21 and removed and m is None and len(det) == 2


def test_text_rectangles_follow_numpy_slicing():
    rects = [(-3, -2, 7, 5), (6, 1, 2, 4), (-100, 0, 3, 3), (2, 2, 100, 100), (-1, -1, -5, -5), (0, 0, 0, 0), (4, -1, -1, 1)]
    for h0, w0 in ((5, 7), (1, 1), (9, 4)):
        m, covered = R.paint(h0, w0, None, rects)
        want = np.zeros((h0, w0, 3), np.uint8)
        for x1, y1, x2, y2 in rects:
            want[y1:y2, x1:x2] = 255
        assert covered == 0 and (m == want).all() and set(np.unique(m)) <= {0, 255}
    m, covered = R.paint(6, 6, _cand([[0, 0, 4, 4, 1, 0], [2, 2, 6, 6, 1, 0]]), [(0, 5, 2, 6)])
    assert covered == 28 and int((m[..., 0] == 255).sum()) == 30     # the union, not the sum; text is not counted


# ------------------------------------------------------------------------------------------------------------------ letterbox geometry
def test_letterbox_shape_and_check_img_size():
    from storygen_amd.mask import check_img_size, letterbox_shape, scale_geometry
    assert [check_img_size(s, 32) for s in (640, 641, 1, 32, 100)] == [640, 672, 32, 32, 128]
    assert check_img_size(640, 64) == 640 and check_img_size(700, 64) == 704
    # 1280 x 720: r = 0.5 -> 640 x 360, pad 24 rows -> 384; 854 x 480: r = 0.7494 -> 640 x 360 again; a square frame fills the square;
    # a small frame is scaled UP (scaleup=True): 100 x 50 -> 640 x 320
    assert letterbox_shape(720, 1280) == (384, 640)
    assert letterbox_shape(1280, 720) == (640, 384)
    assert letterbox_shape(480, 854) == (384, 640)
    assert letterbox_shape(500, 500) == (640, 640)
    assert letterbox_shape(50, 100) == (320, 640)
    assert letterbox_shape(333, 1000) == (224, 640)                  # 213 rows + np.mod(427, 32) = 11 -> 5 + 6
    assert letterbox_shape(720, 1280, 1280, 64) == (768, 1280)
    assert scale_geometry((384, 640), (720, 1280)) == R.scale_geometry((384, 640), (720, 1280)) == (0.0, 12.0, 0.5)


# ------------------------------------------------------------------------------------------------------------------ HumanTextMasker on emulated ops
def _scene(seed, A, nc, input_shape):
    rng = np.random.default_rng(seed)
    h1, w1 = input_shape
    p = np.zeros((A, 5 + nc), F)
    p[:, 0], p[:, 1] = rng.integers(0, w1, A), rng.integers(0, h1, A)
    p[:, 2], p[:, 3] = rng.integers(4, w1 // 3, A), rng.integers(4, h1 // 3, A)
    p[:, 4] = rng.random(A)
    p[:, 5:] = rng.random((A, nc))
    return p


def test_masker_end_to_end_on_emulated_ops():
    from storygen_amd.mask import HumanTextMasker
    input_shape, frames = (96, 160), [(90, 160), (180, 320), (45, 80)]
    pred = np.stack([_scene(s, 120, 3, input_shape) for s in range(3)])
    easyocr = [([[3.7, 4.2], [30.2, 4.2], [30.9, 12.8], [3.1, 12.1]], "text", 0.9), ([[-4.5, 60.0], [20, 60], [20.5, 70.9], [-4, 70]], "t", 0.5)]
    texts = [easyocr, [(10, 10, 50, 30), (-20, -10, 400, 400)], None]
    m = HumanTextMasker(conf_thres=0.3, iou_thres=0.45, classes=(0, 2))
    with patched_mask_ops() as calls:
        got = m.mask(torch.from_numpy(pred), input_shape, frames, texts)
    assert [c[0] for c in calls] == ["det_select", "det_nms", "box_mask", "box_mask", "box_mask"]
    assert [c[3] for c in calls[2:]] == [2, 2, 0]
    rect0 = [(3, 4, 30, 12), (-4, 60, 20, 70)]                       # int() truncates towards zero
    for b, g in enumerate(got):
        wm, wdet, wratio, wrem = R.human_text_mask(pred[b], input_shape, frames[b], [rect0, texts[1], None][b], 0.3, 0.45, 0.2, (0, 2))
        assert g.removed == wrem and g.human_ratio == wratio and g.detections.numpy().tobytes() == wdet.tobytes() and len(wdet) > 0
        assert (g.mask is None) == wrem and (wrem or (g.mask.numpy() == wm).all())
    # the threshold itself: exactly a fifth stays, one pixel more goes, and the mask of a removed frame is None
    p = np.stack([_pred([(0, 0, 10, 2, 0.9, 0, 1.0), (0, 5, 1, 6, 0.4, 0, 1.0)], 2), _pred([(0, 0, 10, 2, 0.9, 0, 1.0), (0, 5, 1, 6, 0.8, 0, 1.0)], 2)])
    with patched_mask_ops():
        a, b = HumanTextMasker().mask(torch.from_numpy(p), (10, 10), [(10, 10), (10, 10)])
    assert a.human_ratio == 0.2 and not a.removed and a.mask is not None and b.human_ratio == 0.21 and b.removed and b.mask is None
    assert len(a.detections) == 1 and len(b.detections) == 2


def test_masker_refuses_bad_arguments():
    from storygen_amd.mask import HumanTextMasker, text_rectangles
    m = HumanTextMasker()
    pred = torch.zeros(2, 4, 7)
    with patched_mask_ops() as calls:
        for bad in (lambda: m.mask(pred, (64, 64), [(10, 10)]), lambda: m.mask(pred[0], (64, 64), [(10, 10)]),
                    lambda: m.mask(pred, (64, 64), [(10, 10), (0, 10)]), lambda: m.mask(pred, (64, 64), [(10, 10), (10, 16385)]),
                    lambda: m.mask(pred, (64, 64), [(10, 10), (10, 10)], [[]]), lambda: m.mask(pred, (64, 64), [(10, 10)] * 2, [[(1, 2, 3)], []]),
                    lambda: m.mask(pred, (64, 64), [(10, 10)] * 2, [[(0, 0, 1, 1)] * 1025, []])):
            with pytest.raises(ValueError):
                bad()
        assert not calls
    for kw in (dict(conf_thres=float("nan")), dict(max_det=0), dict(max_det=1025), dict(max_nms=30001), dict(classes=(-1,))):
        with pytest.raises(ValueError):
            HumanTextMasker(**kw)
    assert HumanTextMasker(classes=None).classes == () and HumanTextMasker(classes=0).classes == (0,)
    assert text_rectangles([(2 ** 40, -2 ** 40, 1.9, -1.9)]).tolist() == [[2 ** 31 - 1, -2 ** 31, 1, -1]]


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from storygen_amd import ops
    pred = torch.zeros(1, 8, 7)
    with pytest.raises(TypeError):
        ops.det_select(pred)
    with pytest.raises(TypeError):
        ops.det_nms(torch.zeros(1, 4, 6), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 5))
    with pytest.raises(TypeError):
        ops.box_mask(4, 4, det=torch.zeros(4, 6), count=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError):
        ops.box_mask(4, 4, text=torch.zeros(1, 4, dtype=torch.int32))
    for bad in (lambda: ops.box_mask(0, 4, text=torch.zeros(1, 4, dtype=torch.int32)), lambda: ops.box_mask(4, 16385, text=torch.zeros(1, 4, dtype=torch.int32)),
                lambda: ops.box_mask(4, 4), lambda: ops.box_mask(4, 4, det=torch.zeros(4, 6)),
                lambda: ops.check_det_sides("t", 1, 2 ** 20 + 1, 1, 1, 1), lambda: ops.check_det_sides("t", 1, 1, 1025, 1, 1),
                lambda: ops.check_det_sides("t", 1, 1, 1, 30001, 1), lambda: ops.check_det_sides("t", 1, 1, 1, 1, 1025),
                lambda: ops.check_det_sides("t", 0, 1, 1, 1, 1)):
        with pytest.raises(ValueError):
            bad()
    ops.check_det_sides("t", 1, 2 ** 20, 1024, 30000, 1024)
    assert (ops.DET_MAX_BATCH, ops.DET_MAX_ANCHORS, ops.DET_MAX_NC, ops.DET_MAX_NMS, ops.DET_MAX_DET, ops.MASK_MAX_SIDE, ops.MASK_MAX_TEXT) == \
        (4096, 1 << 20, 1024, 30000, 1024, 16384, 1024)


def test_c_entry_points_refuse_on_the_host():
    """SG_EINVAL (-1) with a message, before any launch: the calls run on fake pointers on a box without a GPU."""
    from storygen_amd import _lib
    lib = _lib.load()
    P, Q, W, G = 0x10000, 0x2000000, 0x4000000, 0x8000000
    ws = lib.sg_det_select_workspace_bytes(1, 100)
    assert ws == 100 * 24 + 4 and lib.sg_det_select_workspace_bytes(2, 2 ** 20) == 2 * 2 ** 20 * 24 + 8
    assert lib.sg_det_select_workspace_bytes(0, 100) == 0 and lib.sg_det_select_workspace_bytes(1, 2 ** 20 + 1) == 0
    cl = (C.c_int32 * 2)(0, 3)

    def select(pred=P, f16=0, bsp=100 * 7, ldp=7, B=1, A=100, nc=2, thr=0.5, classes=cl, ncl=2, max_nms=100, cand=Q, ncand=Q + 0x100000, w=W, wb=ws):
        return lib.sg_det_select(pred, f16, bsp, ldp, B, A, nc, thr, classes, ncl, max_nms, cand, ncand, w, wb, None)

    for kw, word in ((dict(pred=None), b"null"), (dict(cand=None), b"null"), (dict(w=None), b"null"), (dict(f16=2), b"pred_f16"), (dict(B=0), b"B = 0"),
                     (dict(B=4097, bsp=700), b"B = 4097"), (dict(A=0), b"A = 0"), (dict(A=2 ** 20 + 1), b"A ="), (dict(nc=0), b"nc = 0"),
                     (dict(nc=1025), b"nc = 1025"), (dict(max_nms=0), b"max_nms"), (dict(max_nms=30001), b"max_nms"), (dict(ldp=6), b"row stride"),
                     (dict(bsp=699), b"batch stride"), (dict(thr=float("nan")), b"NaN"), (dict(classes=None), b"classes"), (dict(ncl=-1), b"classes"),
                     (dict(classes=(C.c_int32 * 2)(0, -1)), b"negative"), (dict(wb=ws - 1), b"workspace"), (dict(w=W + 2), b"aligned"),
                     (dict(ncand=Q + 8), b"overlap"), (dict(w=Q + 16), b"overlap")):
        assert select(**kw) == -1 and word in lib.sg_last_error(), (kw, lib.sg_last_error())

    def nms(cand=P, ncand=Q, B=1, max_nms=100, thr=0.6, agnostic=0, max_det=300, geom=G, det=W, count=W + 0x100000):
        return lib.sg_det_nms(cand, ncand, B, max_nms, thr, agnostic, max_det, geom, det, count, None)

    for kw, word in ((dict(cand=None), b"null"), (dict(geom=None), b"null"), (dict(count=None), b"null"), (dict(B=0), b"B = 0"), (dict(max_nms=30001), b"max_nms"),
                     (dict(max_det=0), b"max_det"), (dict(max_det=1025), b"max_det"), (dict(thr=float("nan")), b"NaN"), (dict(agnostic=2), b"agnostic"),
                     (dict(count=W + 24), b"overlap")):
        assert nms(**kw) == -1 and word in lib.sg_last_error(), (kw, lib.sg_last_error())

    def paint(mask=P, ldm=30, h0=10, w0=10, det=Q, count=W, max_det=300, text=G, n_text=2, covered=G + 0x1000):
        return lib.sg_box_mask_u8(mask, ldm, h0, w0, det, count, max_det, text, n_text, covered, None)

    for kw, word in ((dict(mask=None), b"null"), (dict(covered=None), b"null"), (dict(h0=0), b"frame"), (dict(w0=16385, ldm=3 * 16385), b"frame"),
                     (dict(ldm=29), b"row stride"), (dict(count=None), b"go together"), (dict(det=None), b"go together"), (dict(max_det=0), b"max_det"),
                     (dict(max_det=1025), b"max_det"), (dict(det=None, count=None), b"max_det"), (dict(text=None), b"text"), (dict(n_text=1025), b"text"),
                     (dict(n_text=-1), b"text"), (dict(covered=G + 0x1002), b"aligned"), (dict(covered=P + 8), b"overlap")):
        assert paint(**kw) == -1 and word in lib.sg_last_error(), (kw, lib.sg_last_error())
