"""Frame / narration alignment on the GPU: sg_dtw_path_f64 and sg_align_cost_f64 against the NumPy float64 restatement of
tests/align_reference.py (held to hand-worked cases by tests/test_align_host.py), and FrameAligner end to end.

sg_dtw_path_f64: path, path_len, codes and acc equal the restatement BIT FOR BIT — each cell is one float64 add and two comparisons on
the same operands in the same order, so there is nothing to tolerate.  The kernel's workgroup has 256 threads and keeps at most 2048
cells of a diagonal, so the shapes sit on and either side of 64 (a wave), 256 and 2048.

sg_align_cost_f64: elementwise within a DERIVED bar.  u = 2^-53.  Products of fp32 values are exact in float64, so each of the three sums
(dot, |f|^2, |s|^2) errs by at most g = (dim - 1) u times the sum of its terms' magnitudes, whatever the order of the additions.  With
q = dot / (sqrt(nf) sqrt(ns) + 1e-9):  the numerator's error g sum|f s| is at most g times the denominator (Cauchy-Schwarz), i.e. g on q;
the two sums under the roots move the denominator by a relative g / 2 each, i.e. g |q| <= g on q; the two roots, their product, the
+ 1e-9, the division and the 1 - q each round once, 6 u on quantities <= 1 (|q| <= 1, |1 - q| <= 2), counted twice over for a device
sqrt / division that is within one unit in the last place instead of half: 12 u; the final + floor(dt / 60) rounds to u |cost|.  One
side: (2 (dim - 1) + 12 + |cost|) u.  Kernel and restatement both err like that, so the bar per cell is twice it (cost_bar below).
floor(dt / 60) itself is exact on both sides: dt is one exact-operand subtraction and the division is correctly rounded.
What this bar holds and what it does not: it is a worst-case bound and grows with dim, so at dim 512 / 513 the measured error is a few
thousandths of it (profiles/r25a_align.txt); there it catches a dropped element, a wrong tail of the lane-strided loop or a wrong stride
(each moves a cost by about 1e-3 or more, ten orders above the bar), not a last-bit change of the arithmetic.  The arithmetic itself is
held tightly by the dim 1 and dim 8 cases (bar 3e-15 to 7e-15, a handful of units in the last place) and exactly by two checks without
a tolerance: the zero feature row (cost = 1 + whole minutes, bit for bit) and the cells whose times are exactly 60 s and 120 s apart.

End to end: the path of FrameAligner.align equals the restatement's path on the restatement's own cost matrix; the test asserts the
decision margin that makes this independent of the engines' fp16-level deviation.  One case at ViT-B/16's token geometry (197 tokens,
heads of 64, one layer) holds the image feature to 2 x the deviation of the fp16-rounded CPU restatement from the fp32 one, the bar of
tests/test_pick_score_gpu.py for its towers and for its reason (that file's docstring); measured values: profiles/r25a_align.txt."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from tests import align_reference as A
from tests import pick_score_reference as P

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = 2.0 ** -53
THREADS, MAX_SHORT = 256, 2048
PATTERN64 = 0x7FF8DEADBEEF0001          # a NaN with a payload no computation produces
PATTERN32, PATTERN8 = 0x5A5A5A5A, 0xA5


# ---------------------------------------------------------------------------------------------------------------- sg_dtw_path_f64
def _content(kind, r, c, seed=0):
    rng = np.random.default_rng(1000 * r + c + seed)
    if kind == "random":
        return rng.random((r, c)) * 2.0
    if kind == "ints":                                   # exact ties in most cells: the order diagonal, up, left is what is tested
        return rng.integers(0, 3, (r, c)).astype(np.float64)
    if kind == "equal":
        return np.full((r, c), 0.75)
    assert kind == "nonfinite"
    M = rng.random((r, c))
    M[rng.random((r, c)) < 0.15] = np.inf
    M[rng.random((r, c)) < 0.10] = np.nan
    M[rng.random((r, c)) < 0.05] = -np.inf
    return M


def _filled(n, dtype, pattern, gpu):
    return torch.full((n,), pattern, dtype=dtype, device=gpu)


def _run_dtw(gpu, M, strided=False, with_acc=True):
    """Launches on pattern-filled outputs with guard elements behind (and, for acc, around) them; returns the outputs on the host after
    checking that nothing but path[:path_len], path_len and the [r, c] windows changed."""
    from storygen_amd import ops
    r, c = M.shape
    if strided:                                          # a window of a larger NaN-filled buffer
        big = torch.full((r + 2, c + 5), float("nan"), dtype=F64, device=gpu)
        cost = big[1:r + 1, 3:c + 3]
        cost.copy_(torch.from_numpy(M))
        assert cost.stride(0) == c + 5
    else:
        cost = torch.from_numpy(M).to(gpu)
    n = r + c - 1
    pbuf, lbuf, cbuf = _filled(2 * n + 16, torch.int32, PATTERN32, gpu), _filled(4, torch.int32, PATTERN32, gpu), _filled(r * c + 64, torch.uint8, PATTERN8, gpu)
    abuf = _filled((r + 2) * (c + 3), torch.int64, PATTERN64, gpu).view(F64).view(r + 2, c + 3)
    acc = abuf[1:r + 1, 2:c + 2] if with_acc else None
    out = ops.dtw_path(cost, path=pbuf[:2 * n].view(n, 2), path_len=lbuf[:1], codes=cbuf[:r * c].view(r, c), acc=acc)
    assert len(out) == (4 if with_acc else 3)
    pbuf, lbuf, cbuf, abuf = pbuf.cpu().numpy(), lbuf.cpu().numpy(), cbuf.cpu().numpy(), abuf.cpu().view(torch.int64).numpy().copy()
    L = int(lbuf[0])
    assert 1 <= L <= n, (L, n)
    assert (pbuf[2 * L:] == PATTERN32).all(), "path written beyond path_len"
    assert (lbuf[1:] == PATTERN32).all() and (cbuf[r * c:] == PATTERN8).all(), "guard elements written"
    window = np.zeros_like(abuf, bool)
    if with_acc:
        window[1:r + 1, 2:c + 2] = True
    assert (abuf[~window] == np.int64(PATTERN64)).all(), "acc written outside its window"
    if strided:
        assert bool(torch.isnan(big[0]).all() and torch.isnan(big[-1]).all() and torch.isnan(big[:, :3]).all() and torch.isnan(big[:, c + 3:]).all())
    path = [tuple(p) for p in pbuf[:2 * L].reshape(L, 2).tolist()]
    return path, cbuf[:r * c].reshape(r, c), (abuf[1:r + 1, 2:c + 2] if with_acc else None)


def _check_dtw(gpu, M, **kw):
    path, codes, acc = _run_dtw(gpu, M, **kw)
    want_path, want_acc, want_codes = A.dtw(M)
    assert np.array_equal(codes, want_codes), f"{int((codes != want_codes).sum())} codes differ"
    if acc is not None:
        assert np.array_equal(acc, want_acc.view(np.int64)), f"{int((acc != want_acc.view(np.int64)).sum())} accumulated values differ in bits"
    assert path == want_path
    return path


# 1 x 1, a single row / column, 2 x 2; a wave (64) and the workgroup (256) bracketed in either orientation and hit exactly; 300 x 500: both
# sides beyond the workgroup and unequal; the largest admitted shorter side with the other side one longer, in either orientation
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (63, 65), (65, 63), (64, 64), (255, 257), (257, 255), (256, 256), (300, 500)]
LARGEST = [(MAX_SHORT, MAX_SHORT + 1, "random"), (MAX_SHORT + 1, MAX_SHORT, "ints")]


@pytest.mark.parametrize("kind", ["random", "ints", "equal"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_dtw_path_is_the_restatement_bit_for_bit(gpu, shape, kind):
    path = _check_dtw(gpu, _content(kind, *shape))
    if kind == "equal":                                  # the pure diagonal from the far corner, then the forced moves along a border
        r, c = shape
        n = min(r, c)
        assert path[-n:] == [(r - n + k, c - n + k) for k in range(n)]
        assert path[:len(path) - n] == ([(0, j) for j in range(c - n)] if c > r else [(i, 0) for i in range(r - n)])
        assert len(path) == max(r, c)


@pytest.mark.parametrize("case", LARGEST, ids=lambda s: "%dx%d_%s" % s)
def test_dtw_path_at_the_largest_shorter_side(gpu, case):
    r, c, kind = case
    _check_dtw(gpu, _content(kind, r, c))


@pytest.mark.parametrize("shape", [(2, 2), (65, 63), (257, 255), (300, 500)], ids=lambda s: "%dx%d" % s)
def test_dtw_path_on_a_strided_cost_window_and_without_acc(gpu, shape):
    M = _content("ints", *shape, seed=5)
    a = _check_dtw(gpu, M, strided=True)
    assert _check_dtw(gpu, M, with_acc=False) == a


@pytest.mark.parametrize("shape", [(1, 7), (7, 1), (2, 2), (64, 64), (65, 63), (257, 255), (300, 500)], ids=lambda s: "%dx%d" % s)
def test_dtw_path_with_nonfinite_costs_stays_inside_and_ends(gpu, shape):
    """+inf, -inf and NaN cells: the path may be anything, but it is a walk inside the matrix of at most r + c - 1 entries (path_len and
    the guards are checked by _run_dtw), from (0, 0) to (r - 1, c - 1) by the three moves — the borders are left one way only."""
    r, c = shape
    for seed in (0, 1):
        M = _content("nonfinite", r, c, seed)
        if seed:
            M[0, :], M[:, 0] = np.inf, np.nan           # whole borders non-finite
        path, codes, _ = _run_dtw(gpu, M)
        assert all(0 <= i < r and 0 <= j < c for i, j in path) and codes.max() <= 2
        assert path[0] == (0, 0) and path[-1] == (r - 1, c - 1)
        assert {(b[0] - a[0], b[1] - a[1]) for a, b in zip(path, path[1:])} <= {(1, 1), (1, 0), (0, 1)}


def test_dtw_path_is_deterministic_and_refuses_beyond_its_limits(gpu):
    from storygen_amd import ops
    M = _content("ints", 300, 500, seed=9)
    a, b = _run_dtw(gpu, M), _run_dtw(gpu, M)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    with pytest.raises(ValueError, match="shorter side"):
        ops.dtw_path(torch.zeros(MAX_SHORT + 1, MAX_SHORT + 1, dtype=F64, device=gpu))
    with pytest.raises(TypeError):
        ops.dtw_path(torch.zeros(4, 4, dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError, match="path must be"):
        ops.dtw_path(torch.zeros(4, 4, dtype=F64, device=gpu), path=torch.zeros(6, 2, dtype=torch.int32, device=gpu))


# ---------------------------------------------------------------------------------------------------------------- sg_align_cost_f64
def cost_bar(dim, cost):
    """Per cell: 2 sides x (2 (dim - 1) + 12 + |cost|) u — derived in the module docstring."""
    return 2.0 * (2.0 * (dim - 1) + 12.0 + np.abs(cost)) * U


def _times(n, rng, other=None):
    """Times in [0, 400) s on a grid of 1 / 8 s (sums and differences are exact); with `other`, entry k is put exactly 60 s or 120 s away
    from other[k % len(other)] so that the boundaries of the penalty are met exactly on the cells (k, k % len)."""
    t = rng.integers(0, 3200, n) / 8.0
    if other is not None:
        for k in range(n):
            t[k] = other[k % len(other)] + (60.0, 120.0, -60.0, -120.0)[k % 4]
    return t


COST_CASES = [(1, 1, 1), (1, 65, 8), (63, 1, 513), (63, 65, 1), (65, 63, 8), (63, 63, 512), (65, 65, 513), (5, 7, 512), (17, 33, 513)]


@pytest.mark.parametrize("case", COST_CASES, ids=lambda s: "r%d_c%d_dim%d" % s)
def test_align_cost_against_the_restatement(gpu, case):
    from storygen_amd import ops
    r, c, dim = case
    rng = np.random.default_rng(r * 10007 + c * 101 + dim)
    f, s = rng.standard_normal((r, dim)).astype(np.float32), rng.standard_normal((c, dim)).astype(np.float32)
    f[r // 2] = 0.0                                       # a zero feature row: the 1e-9 keeps the quotient finite, cd = 1
    if c > 2:
        s[1] = f[0] if r > 1 else s[1]                    # identical vectors (cd about 1e-9) ...
        s[2] = -3.0 * s[1]                                # ... and opposite ones (cd about 2)
    ts = _times(c, rng)
    tf = _times(r, rng, other=ts)
    want = A.cost_matrix(f, s, tf, ts)
    assert np.isfinite(want).all()
    if r > 1:
        k = np.arange(r)
        assert set(np.abs(tf - ts[k % c]).tolist()) <= {60.0, 120.0}       # met exactly: 60 adds nothing, 120 adds 2
    # frames as a window with a row stride; the output as a window of a NaN-filled buffer
    fbuf = torch.full((r, dim + 3), float("nan"), dtype=torch.float32, device=gpu)
    fbuf[:, :dim] = torch.from_numpy(f)
    obuf = torch.full((r + 2, c + 4), float("nan"), dtype=F64, device=gpu)
    out = ops.align_cost(fbuf[:, :dim], torch.from_numpy(s).to(gpu), torch.from_numpy(tf).to(gpu), torch.from_numpy(ts).to(gpu), out=obuf[1:r + 1, 1:c + 1])
    got = out.cpu().numpy()
    guard = obuf.clone()
    guard[1:r + 1, 1:c + 1] = float("nan")
    assert bool(torch.isnan(guard).all()), "cost written outside its window"
    err, bar = np.abs(got - want), cost_bar(dim, want)
    worst = float((err / bar).max())
    print(f"align_cost r{r} c{c} dim{dim}: max |kernel - restatement| {err.max():.3e}, worst error / bar {worst:.3f} (bar at that cell "
          f"{bar.flat[(err / bar).argmax()]:.3e})")
    assert (err <= bar).all(), f"{int((err > bar).sum())} cells beyond the bar; worst error / bar {worst:.3f}"
    assert np.array_equal(got[r // 2], want[r // 2]) and np.all(want[r // 2] % 1.0 == 0.0)        # the zero row: 1 + whole minutes, exactly
    # contiguous everything, allocated output: the same bits
    again = ops.align_cost(torch.from_numpy(f).to(gpu), torch.from_numpy(s).to(gpu), torch.from_numpy(tf).to(gpu), torch.from_numpy(ts).to(gpu))
    assert np.array_equal(again.cpu().numpy().view(np.int64), got.view(np.int64))


def test_align_cost_wrapper_refusals(gpu):
    from storygen_amd import ops
    f, s = torch.zeros(3, 8, device=gpu), torch.zeros(4, 8, device=gpu)
    t3, t4 = torch.zeros(3, dtype=F64, device=gpu), torch.zeros(4, dtype=F64, device=gpu)
    assert tuple(ops.align_cost(f, s, t3, t4).shape) == (3, 4)
    for args in ((f, s[:, :7], t3, t4), (f, s, t4, t4), (f, s, t3, t3), (f, s.t().contiguous().t(), t3, t4), (f[:0], s, t3[:0], t4)):
        with pytest.raises(ValueError):
            ops.align_cost(*args)
    with pytest.raises(TypeError):
        ops.align_cost(f, s, t3.float(), t4)
    with pytest.raises(ValueError, match="out must be"):
        ops.align_cost(f, s, t3, t4, out=torch.zeros(4, 3, dtype=F64, device=gpu))


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_frame_aligner_end_to_end(gpu):
    """5 frames of mixed sizes (PIL, arrays, a tensor), 7 sentences, two frames replaced by their OCR text, stamps as strings."""
    from PIL import Image
    from storygen_amd.align import FrameAligner, align_features
    SEED = A.STORY_SEED
    cfg = A.b16_config()
    sd = P.tiny_state(SEED, cfg)
    frames, fstamps, ids, sstamps, ocr = A.story_inputs(SEED)
    f, s = A.story_features(sd, cfg, frames, ids, ocr)
    ft, st = [A.timestamp_seconds(v) for v in fstamps], [A.timestamp_seconds(v) for v in sstamps]
    want_M = A.cost_matrix(f, s, ft, st)
    want_path, want_acc, _ = A.dtw(want_M)
    margin = A.decision_margin(want_acc)
    al = FrameAligner(sd, cfg, device=gpu)
    mixed = [frames[0], Image.fromarray(frames[1]), torch.from_numpy(frames[2]), frames[3], Image.fromarray(frames[4])]
    out = al.align(mixed, fstamps, torch.from_numpy(ids), sstamps, ocr_ids=ocr)
    assert out.cost.is_cuda and out.cost.dtype == F64 and tuple(out.cost.shape) == (5, 7)
    moved = float(np.abs(out.cost.cpu().numpy() - want_M).max())
    feats = al.frame_features(frames, ocr)
    print(f"FrameAligner: decision margin {margin:.3e}; the engines' features move a cost by at most {moved:.3e}; frame features rel-L2 "
          f"{rel_l2(feats.cpu(), torch.from_numpy(f)):.2e}, sentence features rel-L2 {rel_l2(al.text_features(torch.from_numpy(ids)).cpu(), torch.from_numpy(s)):.2e}; "
          f"path {out.path}")
    assert margin > 1e-6, "a bad seed: some cell's best and second-best predecessor are too close for a path comparison"
    assert margin > 4 * (5 + 7 - 1) * moved, "the engines' deviation could flip a decision"
    assert out.path == want_path and out.groups == A.groups(want_path)
    assert {i for i, _ in out.groups} == set(range(5)) and sorted(j for _, js in out.groups for j in set(js)) == list(range(7))
    # the same features in hand, with times as float64 seconds: the same alignment, and the cost is the kernel's on those features
    again = align_features(feats, al.text_features(torch.from_numpy(ids)), np.array(ft), torch.tensor(st, dtype=F64))
    assert again.path == out.path and torch.equal(again.cost, out.cost)
    # an OCR frame's feature is the text feature of its ids, any other frame's the image feature
    assert torch.equal(feats[[1, 3]], al.text_features(torch.from_numpy(np.stack([ocr[1], ocr[3]]))))
    assert torch.equal(feats[[0, 2, 4]], al.image_features([frames[0], frames[2], frames[4]]))


def test_image_feature_at_vit_b16_token_geometry(gpu):
    """Image 224, patch 16: 197 tokens, heads of 64 (sg_attn_enc_f16), one layer, hidden 256: what ViT-B/16 asks of the kernels that the
    small config does not.  Bar: 2 x the deviation of the fp16-rounded CPU restatement from the fp32 one (module docstring)."""
    from storygen_amd.align import FrameAligner
    from tests import clip_u8_reference as U8
    cfg = A.b16_config(image=224, vision_hidden=256, layers=1)
    sd = P.tiny_state(5, cfg)
    frames = [U8.content("random", 240, 260, seed=1), U8.content("checker", 224, 224, seed=2)]
    px = U8.pixel_values(frames, 224, "torchvision")
    want, rounded = P.image_features(sd, cfg, px), P.image_features(sd, cfg, px, round_operands=True)
    dev = rel_l2(rounded, want)
    al = FrameAligner(sd, cfg, device=gpu)
    assert (al.vision.T, al.vision.C // al.vision.heads) == (197, 64)
    got = al.image_features(frames)
    err = rel_l2(got.cpu(), want)
    print(f"ViT-B/16 token geometry, 1 layer: image feature rel-L2 {err:.2e} (fp16-rounded CPU restatement {dev:.2e}, bar {2 * dev:.2e})")
    assert tuple(got.shape) == (2, 32) and bool(torch.isfinite(got).all())
    assert 1e-5 < dev < 1e-3
    assert err < 2 * dev
    assert torch.equal(al.image_features(frames), got)
