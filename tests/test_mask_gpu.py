"""Human and text masks on the GPU: sg_det_select, sg_det_nms and sg_box_mask_u8 against the fp32 restatement of tests/mask_reference.py (held
to hand-worked cases and to torch's in-place arithmetic by tests/test_mask_host.py), and HumanTextMasker end to end.  Every comparison is
exact: fp32 bit patterns, bytes, integers.  Inputs are windows of NaN-filled buffers, outputs windows of buffers filled with a NaN of a
payload no computation produces, and every case checks that nothing but the expected elements changed."""
import numpy as np
import pytest
import torch

from tests import mask_reference as R

pytestmark = pytest.mark.gpu
F = np.float32
PAT32, PAT8, PATI = 0x7FC0BEEF, 0xA5, -77


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def _same(got_bits, want):
    """Bit for bit; a NaN equals a NaN (its payload and sign are not part of the result)."""
    want = np.ascontiguousarray(want, dtype=F)
    return bool(((got_bits == want.view(np.int32)) | (np.isnan(got_bits.view(F)) & np.isnan(want))).all())


def _pat_f32(n, gpu):
    return torch.full((n,), PAT32, dtype=torch.int32, device=gpu).view(torch.float32)


# ------------------------------------------------------------------------------------------------------------------ select
def _scene(seed, B, A, nc, kind="random"):
    rng = np.random.default_rng(1000 * A + 10 * nc + seed)
    p = np.empty((B, A, 5 + nc), F)
    p[..., 0:2] = rng.integers(0, 640, (B, A, 2))
    p[..., 2:4] = rng.integers(1, 200, (B, A, 2)) / 4
    p[..., 4] = np.round(rng.random((B, A)), 2)                     # two decimals: equal scores occur
    p[..., 5:] = np.round(rng.random((B, A, nc)), 1)                # one decimal: best-class ties occur
    if kind == "none":
        p[..., 4] = 0.25
    elif kind == "all":
        p[..., 4] = 1.0
        p[..., 5:] = 0.75
    elif kind == "nan":
        for b in range(B):
            idx = rng.permutation(A)
            p[b, idx[0::7], 4] = np.nan
            p[b, idx[1::7], 5 + (A % nc)] = np.nan
            p[b, idx[2::7], A % 4] = np.nan
    return p


def _select(gpu, p, dtype, strided, conf_thres=0.5, classes=(), max_nms=100):
    from storygen_amd import ops
    B, A, C = p.shape
    ldp, off = (C + 3, 3) if strided else (C, 0)
    bsp = A * ldp + (5 if strided else 0)
    buf = torch.full((B * bsp + 8,), float("nan"), dtype=dtype, device=gpu)
    pred = buf[off:].as_strided((B, A, C), (bsp, ldp, 1))
    pred.copy_(torch.from_numpy(p))
    before = buf.clone()
    cbuf, nbuf = _pat_f32(B * max_nms * 6 + 16, gpu), torch.full((B + 8,), PATI, dtype=torch.int32, device=gpu)
    cand, ncand = ops.det_select(pred, conf_thres, classes, max_nms, cand=cbuf[5:5 + B * max_nms * 6].view(B, max_nms, 6), ncand=nbuf[3:3 + B])
    assert cand.data_ptr() == cbuf.data_ptr() + 20 and ncand.data_ptr() == nbuf.data_ptr() + 12
    assert torch.equal(buf.view(torch.int16 if dtype == torch.float16 else torch.int32), before.view(torch.int16 if dtype == torch.float16 else torch.int32))
    cb, nb = cbuf.view(torch.int32).cpu().numpy(), nbuf.cpu().numpy()
    assert (cb[:5] == PAT32).all() and (cb[5 + B * max_nms * 6:] == PAT32).all() and (nb[:3] == PATI).all() and (nb[3 + B:] == PATI).all()
    got = cb[5:5 + B * max_nms * 6].reshape(B, max_nms, 6)
    src = pred.cpu().float().numpy()                                 # what the kernel read, after the fp16 rounding
    total = 0
    for b in range(B):
        want = R.select(src[b], conf_thres, classes, max_nms)
        assert nb[3 + b] == len(want), (b, nb[3 + b], len(want))
        assert _same(got[b, :len(want)], want), f"image {b}: candidates differ"
        assert (got[b, len(want):] == PAT32).all(), f"image {b}: rows beyond ncand written"
        total += len(want)
    return total


@pytest.mark.parametrize("A", [1, 63, 64, 65, 257, 2049])
@pytest.mark.parametrize("nc", [1, 2, 80])
def test_select_anchor_counts_and_class_counts(gpu, A, nc):
    dtype, strided, B = (torch.float16, True, 3) if (A + nc) % 2 else (torch.float32, False, 1)
    n = _select(gpu, _scene(0, B, A, nc), dtype, strided, max_nms=3000)
    assert A < 63 or n > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("strided,B", [(False, 3), (True, 1), (True, 3)])
def test_select_layouts(gpu, dtype, strided, B):
    assert _select(gpu, _scene(1, B, 257, 4), dtype, strided, max_nms=300) > 0


@pytest.mark.parametrize("kind", ["none", "all", "nan"])
def test_select_contents(gpu, kind):
    n = _select(gpu, _scene(2, 2, 257, 3, kind), torch.float32, True, max_nms=600)
    assert (n == 0) if kind == "none" else (n == 2 * 257) if kind == "all" else (0 < n < 2 * 257)


@pytest.mark.parametrize("classes", [(), (0,), (1, 3)])
def test_select_class_filter(gpu, classes):
    assert _select(gpu, _scene(3, 2, 257, 5), torch.float16, False, classes=classes, max_nms=300) > 0


def test_select_more_candidates_than_max_nms(gpu):
    p = _scene(4, 2, 300, 2)
    p[..., 4] = 1.0
    p[..., 5] = np.round(0.6 + 0.3 * np.random.default_rng(0).random((2, 300)), 2)       # 150+ pass per image, many equal scores
    assert _select(gpu, p, torch.float32, False, max_nms=100) == 200
    assert _select(gpu, p, torch.float32, False, conf_thres=0.75, max_nms=100) == 200


def test_select_hand_worked(gpu):
    p3 = np.array([[[10, 10, 4, 4, 1.0, 0.2, 0.8, 0.8], [10, 10, 4, 4, 0.5, 1.0, 0, 0], [10, 10, 4, 4, 1.0, 0.5, 0, 0]]], F)
    assert _select(gpu, p3, torch.float32, False) == 1               # the tie takes class 1; obj == thr and conf == thr are out
    p1 = np.array([[[10, 10, 4, 4, 0.7, 0.1], [10, 10, 4, 4, 0.4, 0.9]]], F)
    assert _select(gpu, p1, torch.float32, True) == 1                # nc == 1: conf = obj


# ------------------------------------------------------------------------------------------------------------------ NMS + rescale
GEOMETRIES = [((384, 640), (720, 1280)), ((640, 384), (1280, 720)), ((384, 640), (480, 854))]


def _nms(gpu, cands, geoms, iou_thres=0.6, agnostic=False, max_det=300, max_nms=None):
    """cands: per image fp32 [n, 6] in score order; geoms: per image (input_shape, frame_shape)."""
    from storygen_amd import ops
    from storygen_amd.mask import scale_geometry
    B = len(cands)
    max_nms = max_nms or max(1, max(len(c) for c in cands)) + 3
    cin = torch.full((B, max_nms, 6), float("nan"), dtype=torch.float32, device=gpu)
    for b, c in enumerate(cands):
        cin[b, :len(c)] = torch.from_numpy(np.asarray(c, F).reshape(-1, 6)).to(gpu)
    ncand = torch.tensor([len(c) for c in cands], dtype=torch.int32, device=gpu)
    geom = torch.tensor([[*scale_geometry(i, f), f[1], f[0]] for i, f in geoms], dtype=torch.float64).float().to(gpu)
    dbuf, nbuf = _pat_f32(B * max_det * 6 + 16, gpu), torch.full((B + 8,), PATI, dtype=torch.int32, device=gpu)
    before = cin.clone()
    det, count = ops.det_nms(cin, ncand, geom, iou_thres, agnostic, max_det, det=dbuf[7:7 + B * max_det * 6].view(B, max_det, 6), count=nbuf[2:2 + B])
    assert torch.equal(cin.view(torch.int32), before.view(torch.int32))
    db, nb = dbuf.view(torch.int32).cpu().numpy(), nbuf.cpu().numpy()
    assert (db[:7] == PAT32).all() and (db[7 + B * max_det * 6:] == PAT32).all() and (nb[:2] == PATI).all() and (nb[2 + B:] == PATI).all()
    got = db[7:7 + B * max_det * 6].reshape(B, max_det, 6)
    counts = []
    for b, c in enumerate(cands):
        c = np.asarray(c, F).reshape(-1, 6)
        want = c[R.nms(c, iou_thres, agnostic, max_det)].copy()
        if len(want):
            want[:, :4] = R.rescale(want[:, :4], *geoms[b])
        assert nb[2 + b] == len(want), (b, nb[2 + b], len(want))
        assert _same(got[b, :len(want)], want), f"image {b}: detections differ"
        assert (got[b, len(want):] == PAT32).all(), f"image {b}: rows beyond count written"
        counts.append(len(want))
    return counts


def _boxes(seed, n, integer=False, ncls=1, spread=300):
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2)) * spread
    wh = 8 + rng.random((n, 2)) * 60
    if integer:
        xy, wh = np.floor(xy / 8) * 8, np.floor(wh / 8) * 8
    conf = np.sort(np.round(rng.random(n), 2))[::-1]
    return np.concatenate([xy, xy + wh, conf[:, None], rng.integers(0, ncls, (n, 1))], 1).astype(F)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129])
def test_nms_bitmap_word_edges(gpu, n):
    counts = _nms(gpu, [_boxes(n, n), _boxes(n + 7, n, integer=True)], [GEOMETRIES[0], GEOMETRIES[2]], iou_thres=0.3)
    assert n < 63 or all(0 < c < n for c in counts)


def test_nms_hand_worked(gpu):
    g = ((640, 640), (640, 640))
    at = [[0, 0, 3, 1, 0.9, 0], [1, 0, 4, 1, 0.8, 0]]               # IoU 2 / 4: exactly the threshold
    assert _nms(gpu, [at, at], [g, g], iou_thres=0.5) == [2, 2]
    assert _nms(gpu, [at], [g], iou_thres=float(np.nextafter(F(0.5), F(0)))) == [1]
    assert _nms(gpu, [[[0, 0, 4, 1, 0.9, 0], [1, 0, 4, 1, 0.8, 0]]], [g], iou_thres=0.5) == [1]
    tie = [[0, 0, 4, 4, 0.9, 0], [100, 100, 104, 104, 0.9, 0], [1, 0, 5, 4, 0.9, 0]]
    assert _nms(gpu, [tie], [g], iou_thres=0.5) == [2]
    two = [[0, 0, 4, 4, 0.9, 0], [0, 0, 4, 4, 0.8, 1]]
    assert _nms(gpu, [two], [g], iou_thres=0.5) == [2] and _nms(gpu, [two], [g], iou_thres=0.5, agnostic=True) == [1]
    empty = [[5, 5, 5, 5, 0.9, 0], [5, 5, 5, 5, 0.8, 0]]
    assert _nms(gpu, [empty], [g], iou_thres=0.0) == [2]             # 0 / 0 suppresses nothing


def test_nms_max_det_and_heavy_overlap(gpu):
    grid = np.array([[40 * (k % 20), 40 * (k // 20), 40 * (k % 20) + 30, 40 * (k // 20) + 30, 1.0 - k / 1000, 0] for k in range(400)], F)
    pile = np.array([[100 + k % 3, 100 + k % 2, 300 + k % 3, 300 + k % 2, 1.0 - k / 1000, 0] for k in range(200)], F)
    g = ((800, 800), (800, 800))
    assert _nms(gpu, [grid, pile], [g, g]) == [300, 1]
    assert _nms(gpu, [grid[:70]], [g], max_det=64) == [64]


@pytest.mark.parametrize("agnostic", [False, True])
def test_nms_class_offsets_and_integer_ties(gpu, agnostic):
    counts = _nms(gpu, [_boxes(5, 129, integer=True, ncls=3, spread=120), _boxes(6, 100, ncls=80, spread=80)], GEOMETRIES[:2], iou_thres=0.45, agnostic=agnostic)
    assert all(1 < c < 129 for c in counts)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_rescale_edges_and_half_to_even(gpu, geometry):
    (h1, w1), (h0, w0) = geometry
    pad_x, pad_y, gain = R.scale_geometry(*geometry)
    rows = []
    for k, q in enumerate([0.5, 1.5, 2.5, 3.5, w0 - 0.5, w0 + 0.5, -0.5, h0 - 1.5, h0 + 2.5]):     # quotients on .5 (where fp32 holds them)
        x, y = q * gain + pad_x, q * gain + pad_y
        rows.append([x, y, x + 1000 * (k + 1), y + 1000 * (k + 1), 0.9 - 0.01 * k, k])            # far apart through the class offset
    edge = [[-50, -50, 0, 0, 0.5, 20], [w1 + 50, h1 + 50, w1 + 60, h1 + 60, 0.4, 21], [pad_x, pad_y, w1 - pad_x, h1 - pad_y, 0.3, 22],
            [np.nan, 5, np.inf, -np.inf, 0.2, 23]]
    assert _nms(gpu, [np.array(rows + edge, F)], [geometry]) == [len(rows) + len(edge)]
    rng = np.random.default_rng(9)
    v = rng.random((256, 2)) * [w1, h1]
    many = np.concatenate([v, v + rng.random((256, 2)) * 3, np.linspace(0.99, 0.5, 256)[:, None], np.arange(256)[:, None]], 1).astype(F)
    assert _nms(gpu, [many], [geometry]) == [256]


# ------------------------------------------------------------------------------------------------------------------ painter
EDGE_RECTS = [(-3, -2, 7, 5), (6, 1, 2, 4), (-100, 0, 3, 3), (2, 2, 100, 100), (-1, -1, -5, -5), (0, 0, 0, 0), (4, -1, -1, 1), (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 1)]


def _paint(gpu, h0, w0, det=None, text=None, max_det=8):
    """Both layouts: rows 16-byte aligned (the 16-byte stores) and rows of an odd pitch at an odd address (byte stores)."""
    from storygen_amd import ops
    want, want_cov = R.paint(h0, w0, det, text)
    for ldm, off in (((3 * w0 + 15) // 16 * 16 + 16, 16), (3 * w0 + 5, 1)):
        buf = torch.full((off + h0 * ldm + 16,), PAT8, dtype=torch.uint8, device=gpu)
        out = buf[off:off + h0 * ldm].view(h0, ldm)[:, :3 * w0].unflatten(1, (w0, 3))
        assert out.data_ptr() % 16 == off % 16
        kw = {}
        if det is not None:
            d = torch.full((max_det, 6), float("nan"), dtype=torch.float32, device=gpu)
            d[:len(det)] = torch.from_numpy(np.asarray(det, F).reshape(-1, 6)).to(gpu)
            kw = dict(det=d, count=torch.tensor([len(det)], dtype=torch.int32, device=gpu))
        if text is not None:
            kw["text"] = torch.tensor(text, dtype=torch.int32, device=gpu).view(-1, 4)
        cbuf = torch.full((5,), PATI, dtype=torch.int32, device=gpu)
        m, cov = ops.box_mask(h0, w0, out=out, covered=cbuf[2:3], **kw)
        assert m.data_ptr() == out.data_ptr() and cbuf.cpu().tolist() == [PATI, PATI, want_cov, PATI, PATI]
        host = buf.cpu().numpy()
        rows = host[off:off + h0 * ldm].reshape(h0, ldm)
        assert (host[:off] == PAT8).all() and (host[off + h0 * ldm:] == PAT8).all() and (rows[:, 3 * w0:] == PAT8).all(), "written outside the window"
        assert (rows[:, :3 * w0].reshape(h0, w0, 3) == want).all(), (h0, w0, ldm)
    return want_cov


@pytest.mark.parametrize("h0,w0", [(1, 1), (7, 5), (64, 64), (65, 63)])
def test_paint_frames_and_rectangle_sources(gpu, h0, w0):
    persons = np.array([[0, 0, w0 // 2 + 1, h0 // 2 + 1, 0.9, 0], [w0 // 3, h0 // 3, w0, h0 - h0 // 4, 0.8, 0], [w0, 0, 0, h0, 0.7, 0]], F)
    union = np.zeros((h0, w0), bool)
    for x1, y1, x2, y2 in persons[:, :4].astype(int):
        union[y1:y2, x1:x2] = True
    assert _paint(gpu, h0, w0, persons, EDGE_RECTS) == int(union.sum())        # the union, not the sum; text is not counted
    assert _paint(gpu, h0, w0, persons, None) == int(union.sum())
    assert _paint(gpu, h0, w0, None, EDGE_RECTS) == 0
    assert _paint(gpu, h0, w0, None, [(0, 0, 0, 0)]) == 0                       # nothing covered
    assert _paint(gpu, h0, w0, np.zeros((0, 6), F), None) == 0                  # a det of no rows
    assert _paint(gpu, h0, w0, np.array([[0, 0, w0, h0, 1, 0]], F), [(0, 0, w0, h0)]) == h0 * w0


def test_paint_a_video_frame(gpu):
    rng = np.random.default_rng(2)
    persons = np.concatenate([rng.integers(0, 640, (6, 2)), rng.integers(640, 1281, (6, 1)), rng.integers(360, 721, (6, 1)), np.ones((6, 2))], 1).astype(F)
    persons[:, [1, 3]] = np.minimum(persons[:, [1, 3]], 720)
    text = [(int(x), int(y), int(x) + 90, int(y) + 25) for x, y in rng.integers(-40, 1260, (20, 2))]
    assert _paint(gpu, 720, 1280, persons[:, [0, 1, 2, 3, 4, 5]], text) > 0


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_masker_end_to_end(gpu):
    from storygen_amd.mask import HumanTextMasker
    input_shape, frames = (96, 160), [(90, 160), (180, 320), (45, 80)]
    rng = np.random.default_rng(11)
    A, nc = 300, 3
    pred = np.zeros((3, A, 5 + nc), F)
    pred[..., 0], pred[..., 1] = rng.integers(0, 160, (3, A)), rng.integers(0, 96, (3, A))
    pred[..., 2], pred[..., 3] = rng.integers(4, 30, (3, A)), rng.integers(4, 20, (3, A))
    pred[..., 4] = np.round(rng.random((3, A)), 2)
    pred[..., 5:] = np.round(rng.random((3, A, nc)), 1)
    pred[0] = 0                                                      # frame 0: one box over exactly a fifth of 90 x 160 (gain 1, pad (0, 3))
    pred[0, 17] = [80, 12, 160, 18, 0.9, 1.0, 0, 0]
    pred[2, 40:, 4] = 0                                              # frame 2: a few people, kept; frame 1: a crowd, removed
    easyocr = [([[3.7, 4.2], [30.2, 4.2], [30.9, 12.8], [3.1, 12.1]], "text", 0.9), ([[-4.5, 60.0], [20, 60], [20.5, 70.9], [-4, 70]], "t", 0.5)]
    texts = [easyocr, [(10, 10, 50, 30), (-20, -10, 400, 400), (300, 100, 100, 150)], None]
    plain = [[(3, 4, 30, 12), (-4, 60, 20, 70)], texts[1], None]
    for dtype in (torch.float32, torch.float16):
        p = torch.from_numpy(pred).to(dtype)
        got = HumanTextMasker(conf_thres=0.4, iou_thres=0.45, classes=(0, 2)).mask(p.to(gpu), input_shape, frames, texts)
        removed = []
        for b, g in enumerate(got):
            wm, wdet, wratio, wrem = R.human_text_mask(p[b].float().numpy(), input_shape, frames[b], plain[b], 0.4, 0.45, 0.2, (0, 2))
            assert g.removed == wrem and g.human_ratio == wratio, (b, g.human_ratio, wratio)
            assert _bits(g.detections.cpu().numpy()).tobytes() == _bits(wdet).tobytes() and len(wdet) > 0
            assert (g.mask is None) == wrem and (wrem or (g.mask.cpu().numpy() == wm).all())
            removed.append(wrem)
        assert got[0].human_ratio == 0.2 and removed == [False, True, False]
