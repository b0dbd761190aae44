"""Near-duplicate keyframe removal on the GPU: sg_adjacent_cosine_f64 against the float64 restatement of tests/dedup_reference.py (pinned to
torch.cosine_similarity and to the script's loop by tests/test_dedup_host.py), DinoVitEngine against the restated tower, the drop-in, and
KeyframeDeduper end to end.

sg_adjacent_cosine_f64: `sim` within a DERIVED bar.  u = 2^-53.  Products of fp32 values are exact in float64, so each of the three sums
(dot, |f|^2, |g|^2) errs by at most e = (dim - 1) u times the sum of its terms' magnitudes, whatever the order of the additions.  With
q = dot / (max(|f|, eps) max(|g|, eps)): the numerator's error e sum|f g| is at most e |f| |g| (Cauchy-Schwarz), which is at most e times the
denominator: e on q; the two sums under the roots move the denominator by a relative e / 2 each (not at all where the clamp holds): e |q| <= e
on q; the two roots, their product and the division round once each, 4 u on a quantity |q| <= 1, counted twice over for a device sqrt /
division that is within one unit in the last place instead of half: 8 u.  One side: (2 (dim - 1) + 8) u.  Kernel and restatement both err
like that, so the bar is twice it (sim_bar below): 3.6e-15 at dim 1, 3.4e-13 at dim 768 — a dropped element, a wrong tail of either loop
or a wrong stride moves a similarity by 1e-3 or more.  `drop` must equal the restatement's wherever |sim - threshold| exceeds the bar, and
the test asserts that this covers at least 95 % of its pairs (the inputs are built on the CPU so that the restatement alone says so).
Without any tolerance: integer-valued vectors (every sum exact in any order; the remaining operations are correctly rounded IEEE ones),
the 0.75 tie, identical rows, zero rows, a NaN row, N = 1.

Engine: at a small geometry that still takes the MFMA attention (145 tokens) the patch rows equal the restatement's pixels bit for bit, and
the features are held to 2 x the deviation of the fp16-rounded CPU restatement from the fp32 one — the bar of tests/test_pick_score_gpu.py,
for its reason (that file's docstring): the engine rounds where that restatement rounds, the rest is summation order.  One case at
dino_vitb8's token geometry (785 tokens, 12 heads of 64, width 768) with 2 layers.  End to end the decisions of KeyframeDeduper.dedup equal
the restatement's; the test asserts the gap that makes this independent of the engine's fp16-level deviation.  Measured values:
profiles/r26a_dedup.txt."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from tests import dedup_reference as D

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = 2.0 ** -53
HEADS = D.TINY["num_heads"]
PATTERN64, PATTERN8 = 0x7FF8DEADBEEF0001, 0xA5          # a NaN with a payload no computation produces


def sim_bar(dim):
    """2 sides x (2 (dim - 1) + 8) u — derived in the module docstring."""
    return 2.0 * (2.0 * (dim - 1) + 8.0) * U


# ------------------------------------------------------------------------------------------------------- sg_adjacent_cosine_f64
def _chain(N, dim, seed):
    """fp32 [N, dim]: row i = cos(t) row i-1 + sin(t) fresh, t random per row, so that the similarities spread over (0, 1) on either side
    of 0.75 (at dim 1 they are +-1); rows rescaled by random powers of two (the cosine does not care)."""
    rng = np.random.default_rng(100003 * N + dim + seed)
    f = np.empty((N, dim))
    f[0] = rng.standard_normal(dim)
    for i in range(1, N):
        t = rng.random() * 1.5
        f[i] = np.cos(t) * f[i - 1] + np.sin(t) * rng.standard_normal(dim) * (np.linalg.norm(f[i - 1]) / np.sqrt(dim))
    return (f * 2.0 ** rng.integers(-3, 4, (N, 1))).astype(np.float32)


def _layout(gpu, f, kind):
    """The features on the device as `kind` lays them out; returns the [N, dim] view handed to the wrapper."""
    N, dim = f.shape
    t = torch.from_numpy(f)
    if kind == "contiguous":
        return t.to(gpu)
    ldf = {"ld4": (dim + 7) & ~3, "ld5": dim + 5, "offset1": dim + 3}[kind]       # ld4: rows stay 16-byte aligned with any dim
    off = 1 if kind == "offset1" else 0                                          # offset1: the base is 4 bytes past an aligned address
    flat = torch.full((N * ldf + 4,), float("nan"), dtype=torch.float32, device=gpu)
    view = flat[off:off + N * ldf].view(N, ldf)[:, :dim]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * off and (view.stride(0) == ldf or N == 1)
    return view


def _run(gpu, feats, threshold=0.75, eps=1e-8):
    """Launches on windows of pattern-filled buffers; returns (sim float64 [N], drop bool [N]) on the host after checking that nothing
    outside the windows changed and that drop holds only 0 and 1."""
    from storygen_amd import ops
    N = feats.shape[0]
    sbuf = torch.full((N + 8,), PATTERN64, dtype=torch.int64, device=gpu)
    dbuf = torch.full((N + 16,), PATTERN8, dtype=torch.uint8, device=gpu)
    sim, drop = ops.adjacent_cosine(feats, threshold, eps, sim=sbuf.view(F64)[3:3 + N], drop=dbuf[5:5 + N])
    assert sim.data_ptr() == sbuf.data_ptr() + 24 and drop.data_ptr() == dbuf.data_ptr() + 5
    sb, db = sbuf.cpu().numpy(), dbuf.cpu().numpy()
    assert (sb[:3] == np.int64(PATTERN64)).all() and (sb[3 + N:] == np.int64(PATTERN64)).all(), "sim written outside its window"
    assert (db[:5] == PATTERN8).all() and (db[5 + N:] == PATTERN8).all(), "drop written outside its window"
    assert set(db[5:5 + N].tolist()) <= {0, 1}
    return sb[3:3 + N].view(np.float64).copy(), db[5:5 + N].astype(bool)


NS = (1, 2, 3, 4, 5, 63, 64, 65, 257)
DIMS = (1, 3, 4, 7, 8, 64, 255, 256, 257, 768)
WORST = [0.0]                                            # largest error / bar of the cases run so far, for the printed summary


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("N", NS)
def test_adjacent_cosine_against_the_restatement(gpu, N, dim):
    f = _chain(N, dim, 0)
    want_sim, want_drop = D.adjacent_cosine(f)
    bar = sim_bar(dim)
    decided = np.abs(want_sim[1:] - 0.75) > bar                          # pairs whose decision the bar does not touch
    first, worst = None, 0.0
    for kind in ("contiguous", "ld4", "ld5", "offset1"):
        sim, drop = _run(gpu, _layout(gpu, f, kind))
        err = np.abs(sim - want_sim)
        assert sim[0] == 0.0 and not np.signbit(sim[0]) and not drop[-1]
        assert err.max() <= bar, f"{kind}: worst error / bar {err.max() / bar:.3f}"
        assert np.array_equal(drop[:-1][decided], want_drop[:-1][decided]), kind
        worst = max(worst, float(err.max() / bar))
        # the two 16-byte layouts add in one order, the two scalar layouts (where dim % 4, or ldf % 4, or the base rule out 16-byte loads)
        # in another: within a path the bits do not depend on the stride
        if kind == "contiguous":
            first = sim
        elif kind == "ld4" and dim % 4 == 0:
            assert np.array_equal(sim.view(np.int64), first.view(np.int64))
    WORST[0] = max(WORST[0], worst)
    if N >= 63:
        assert 0 < want_drop.sum() < N - 1                               # both decisions occur
    print(f"adjacent_cosine N{N} dim{dim}: worst error / bar over the four layouts {worst:.3f} (bar {bar:.2e}), {int(want_drop.sum())} of {N - 1} pairs drop")


def test_adjacent_cosine_decisions_cover_the_pairs(gpu):
    """The restatement alone: at least 95 % of all pairs of the cases above lie further from the threshold than the bar (all of them, in fact,
    unless a similarity of the random chains falls within 1e-13 of 0.75), so the exact comparison of `drop` there is not vacuous."""
    pairs = decided = 0
    for N in NS:
        for dim in DIMS:
            s, _ = D.adjacent_cosine(_chain(N, dim, 0))
            pairs += N - 1
            decided += int((np.abs(s[1:] - 0.75) > sim_bar(dim)).sum())
    print(f"adjacent_cosine: {decided} of {pairs} pairs are decided beyond the bar; worst measured error / bar so far {WORST[0]:.3f}")
    assert decided >= 0.95 * pairs


@pytest.mark.parametrize("shape", [(65, 257), (257, 256), (5, 768), (64, 7)], ids=lambda s: "N%d_dim%d" % s)
def test_adjacent_cosine_integer_vectors_bit_for_bit(gpu, shape):
    """Entries in [-8, 8]: products and sums are small integers, exact in any order; sqrt, product and division are single correctly rounded
    operations on equal operands, so kernel and restatement agree in every bit of sim and in every decision."""
    N, dim = shape
    f = np.random.default_rng(N * 1000 + dim).integers(-8, 9, (N, dim)).astype(np.float32)
    f[N // 2] = f[N // 2 - 1]                                            # identical rows
    want_sim, want_drop = D.adjacent_cosine(f, 0.1)
    for kind in ("contiguous", "ld5", "offset1"):
        sim, drop = _run(gpu, _layout(gpu, f, kind), threshold=0.1)
        assert np.array_equal(sim.view(np.int64), want_sim.view(np.int64)), f"{kind}: {int((sim != want_sim).sum())} similarities differ in bits"
        assert np.array_equal(drop, want_drop)
    assert 0 < want_drop.sum() < N - 1


def test_adjacent_cosine_exact_cases(gpu):
    tie = np.array([[1, 0, 0, 0, 0], [3, 2, 1, 1, 1]], np.float32)      # 3 / (1 * 4): exactly the threshold, and a tie drops
    sim, drop = _run(gpu, torch.from_numpy(tie).to(gpu))
    assert sim.tolist() == [0.0, 0.75] and drop.tolist() == [True, False]
    sim, drop = _run(gpu, torch.from_numpy(tie).to(gpu), threshold=float(np.nextafter(0.75, 1.0)))
    assert sim.tolist() == [0.0, 0.75] and drop.tolist() == [False, False]
    # identical rows of norm 2^k: exactly 1; opposite rows: exactly -1; a zero row next to a non-zero one and two zero rows: exactly +0
    f = np.zeros((9, 16), np.float32)
    f[0] = f[1] = 0.5
    f[2] = -2.0 * f[1]
    f[5] = 3.0
    f[8] = np.arange(16)
    sim, drop = _run(gpu, torch.from_numpy(f).to(gpu))
    assert sim.tolist() == [0.0, 1.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0] and not np.signbit(sim[3:]).any()
    assert drop.tolist() == [True] + [False] * 8
    want_sim, want_drop = D.adjacent_cosine(f)
    assert np.array_equal(sim, want_sim) and np.array_equal(drop, want_drop)
    # eps = 0 is admitted: two zero rows are then 0 / 0 = NaN, kept
    sim, drop = _run(gpu, torch.from_numpy(f).to(gpu), eps=0.0)
    assert np.isnan(sim[4]) and np.isnan(sim[7]) and sim[1] == 1.0 and drop.tolist() == [True] + [False] * 8
    # a NaN or an infinite entry: the two pairs it belongs to are NaN and kept, whatever the threshold; the others do not see it
    g = np.ones((6, 260), np.float32)
    g[2, 259] = np.nan
    g[4, 3] = np.inf
    for thr in (0.75, -2.0):
        sim, drop = _run(gpu, torch.from_numpy(g).to(gpu), threshold=thr)
        assert np.isnan(sim[[2, 3, 4, 5]]).all() and sim[0] == 0.0 and abs(sim[1] - 1.0) <= sim_bar(260)
        assert drop.tolist() == [True, False, False, False, False, False]
    # N = 1: one similarity, nothing to drop
    sim, drop = _run(gpu, torch.ones(1, 768, device=gpu))
    assert sim.tolist() == [0.0] and drop.tolist() == [False]
    sim, drop = _run(gpu, torch.ones(4, 768, device=gpu)[2:3, :5], threshold=-1.0)
    assert sim.tolist() == [0.0] and drop.tolist() == [False]


def test_adjacent_cosine_wrapper_refusals(gpu):
    from storygen_amd import ops
    f = torch.ones(5, 8, device=gpu)
    sim, drop = ops.adjacent_cosine(f)
    assert sim.dtype == F64 and drop.dtype == torch.uint8 and tuple(sim.shape) == tuple(drop.shape) == (5,) and sim.device == f.device
    assert drop.tolist() == [1, 1, 1, 1, 0]
    for bad in (f[0], f[:0], f[:, :0], f.t(), f.expand(3, 5, 8)):
        with pytest.raises(ValueError):
            ops.adjacent_cosine(bad)
    with pytest.raises(ValueError, match="overlap"):
        ops.adjacent_cosine(f[:1].expand(5, 8))
    for eps in (-1e-8, float("nan")):
        with pytest.raises(ValueError, match="eps"):
            ops.adjacent_cosine(f, eps=eps)
    with pytest.raises(TypeError):
        ops.adjacent_cosine(f.double())
    with pytest.raises(TypeError):
        ops.adjacent_cosine(f, sim=torch.zeros(5, device=gpu))
    with pytest.raises(TypeError):
        ops.adjacent_cosine(f, drop=torch.zeros(5, dtype=torch.bool, device=gpu))
    with pytest.raises(ValueError, match="sim must be"):
        ops.adjacent_cosine(f, sim=torch.zeros(6, dtype=F64, device=gpu))
    with pytest.raises(ValueError, match="drop must be"):
        ops.adjacent_cosine(f, drop=torch.zeros(10, dtype=torch.uint8, device=gpu)[::2])
    raw = torch.zeros(64, dtype=torch.uint8, device=gpu)                 # sim and drop carved from one buffer so that they overlap
    with pytest.raises(RuntimeError, match="overlap"):
        ops.adjacent_cosine(f, sim=raw[:40].view(F64), drop=raw[39:44])


# ------------------------------------------------------------------------------------------------------------------ the engine
def _mixed_frames():
    """A landscape, a portrait, one whose shorter side already equals the resize (112: its vertical pass is skipped), a square at the
    resize (both passes skipped), and a second landscape of the first one's size (two frames in one launch)."""
    from tests import clip_u8_reference as U8
    return [U8.content("random", 120, 150, seed=1), U8.content("checker", 200, 130, seed=2), U8.content("random", 112, 140, seed=3),
            U8.content("ramp", 112, 112, seed=4), U8.content("random", 120, 150, seed=5), D.block_image(6, 300, 227), D.block_image(7, 113, 115)]


@pytest.fixture(scope="module")
def tiny(gpu):
    from storygen_amd.dino import DinoVitEngine
    sd = D.tiny_state(0)
    frames = _mixed_frames()
    px = D.pixel_values(frames, 96, 112)
    want, rounded = D.dino_forward(sd, px, HEADS), D.dino_forward(sd, px, HEADS, round_operands=True)
    return sd, frames, px, want, rounded, DinoVitEngine(sd, gpu, heads=HEADS, resize=112)


def test_engine_patch_rows_are_the_transforms_pixels_bit_for_bit(gpu, tiny):
    from PIL import Image
    _, frames, px, _, _, eng = tiny
    assert (eng.T, eng.S, eng.ps, eng.C // eng.heads) == (145, 96, 8, 32)
    mixed = [frames[0], Image.fromarray(frames[1]), torch.from_numpy(frames[2]), frames[3], Image.fromarray(frames[4]), frames[5], frames[6]]
    rows = eng.patch_rows_u8(mixed).cpu().numpy()
    want = D.patch_rows_u8(frames, 96, 8, 112)
    assert rows.shape == want.shape == (7 * 144, 192)
    assert np.array_equal(rows.view(np.uint16), want.view(np.uint16)), f"{int((rows.view(np.uint16) != want.view(np.uint16)).sum())} fp16 values differ"
    # the same pixels, handed over as the transform's float output, give the same features
    assert torch.equal(eng(mixed), eng.encode_pixels(px))


def test_engine_features_against_the_restatement(gpu, tiny):
    _, frames, _, want, rounded, eng = tiny
    dev = rel_l2(rounded, want)
    got = eng(frames)
    err = rel_l2(got.cpu(), want)
    print(f"DinoVitEngine 145 tokens, 2 heads of 32, 2 layers: feature rel-L2 {err:.2e} (fp16-rounded CPU restatement {dev:.2e}, bar {2 * dev:.2e})")
    assert tuple(got.shape) == (7, 64) and got.dtype == torch.float32 and got.device == gpu and bool(torch.isfinite(got).all())
    assert torch.equal(got, got.half().float())                          # the final LayerNorm writes fp16
    assert 1e-5 < dev < 1e-3
    assert err < 2 * dev


def test_engine_batches_give_the_same_bits(gpu, tiny):
    _, frames, _, _, _, eng = tiny
    whole = eng(frames, batch=16)
    assert torch.equal(eng(frames, batch=3), whole)
    assert torch.equal(eng(np.stack([frames[0], frames[4]]), batch=1), whole[[0, 4]])


def test_engine_at_dino_vitb8_token_geometry(gpu):
    """Patch 8, crop 224, width 768: 785 tokens, 12 heads of 64, K = 192 in the patch GEMM — what dino_vitb8 asks of the kernels — with 2
    layers and the script's resize of 256.  Bar: 2 x the deviation of the fp16-rounded CPU restatement from the fp32 one."""
    from storygen_amd.dino import DinoVitEngine
    from tests import clip_u8_reference as U8
    sd = D.tiny_state(5, embed_dim=768, depth=2, img_size=224)
    frames = [U8.content("random", 300, 400, seed=1), D.block_image(2, 256, 256)]
    px = D.pixel_values(frames)
    want, rounded = D.dino_forward(sd, px, 12), D.dino_forward(sd, px, 12, round_operands=True)
    dev = rel_l2(rounded, want)
    eng = DinoVitEngine(sd, gpu)
    assert (eng.T, eng.S, eng.C // eng.heads, eng.kpad, eng.resize) == (785, 224, 64, 192, 256)
    got = eng(frames)
    err = rel_l2(got.cpu(), want)
    print(f"dino_vitb8 token geometry, 2 layers: feature rel-L2 {err:.2e} (fp16-rounded CPU restatement {dev:.2e}, bar {2 * dev:.2e})")
    assert tuple(got.shape) == (2, 768) and bool(torch.isfinite(got).all())
    assert 1e-5 < dev < 2e-3
    assert err < 2 * dev
    assert torch.equal(eng(frames), got)


def test_drop_in_forward_is_the_engines_encode_pixels(gpu, tiny):
    from storygen_amd.model import DinoVisionTransformer
    sd, _, px, _, _, eng = tiny
    m = DinoVisionTransformer(img_size=96, patch_size=8, embed_dim=64, depth=2, num_heads=HEADS)
    m.load_state_dict(sd)
    assert m.cuda() is m and m.device.type == "cuda" and m.eval() is m
    with torch.no_grad():
        out = m(px.to(gpu))
    assert tuple(out.shape) == (7, 64) and out.dtype == torch.float32 and out.is_cuda
    assert torch.equal(out, eng.encode_pixels(px))
    assert rel_l2(m(px[:1]).cpu(), out[:1].cpu()) < 1e-3                 # one image, as the script calls it
    back = m.to("cpu").state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(ValueError, match="native token grid"):
        m(torch.zeros(1, 3, 104, 104))


# ------------------------------------------------------------------------------------------------------------------ end to end
THRESHOLD = 0.75          # the script's; chosen on the CPU with the weights: tables at scale 1 put near-copies above 0.999, other shots below 0.66


def test_keyframe_deduper_end_to_end(gpu):
    """Eight frames in four shots.  A randomly initialised ViT can map every image to almost one class feature (with the position table
    at 10 x its scale unrelated images reach 0.85); with the tables at scale 1 the restatement's similarities fall into two groups either
    side of the script's threshold.  The gap on either side must be at least 20 x the largest change of a similarity between the
    fp16-rounded and the fp32 restatement, which is the size of what the engine may do to it."""
    from PIL import Image
    from storygen_amd.dedup import KeyframeDeduper, dedup_features
    sd = D.tiny_state(0, table_scale=1.0)
    frames = D.keyframes()
    px = D.pixel_values(frames, 96, 256)
    f32, f16 = D.dino_forward(sd, px, HEADS).numpy(), D.dino_forward(sd, px, HEADS, round_operands=True).numpy()
    want_sim, want_drop = D.adjacent_cosine(f32, THRESHOLD)
    moved = float(np.abs(D.adjacent_cosine(f16, THRESHOLD)[0] - want_sim).max())
    gap = float(np.abs(want_sim[1:] - THRESHOLD).min())
    assert want_drop.tolist() == [True, True, False, True, False, False, True, False]
    assert want_sim[1:][want_drop[:-1]].min() > THRESHOLD > want_sim[1:][~want_drop[:-1]].max()      # two groups
    assert gap >= 20 * moved, (gap, moved)
    dd = KeyframeDeduper(sd, device=gpu, threshold=THRESHOLD, heads=HEADS)
    mixed = [Image.fromarray(a) if i % 2 else a for i, a in enumerate(frames)]
    out = dd.dedup(mixed, batch=3)
    got_moved = float(np.abs(out.similarity - want_sim).max())
    print(f"KeyframeDeduper: similarities {np.round(out.similarity, 4).tolist()}; gap to the threshold {gap:.3e}; the fp16-rounded restatement "
          f"moves a similarity by at most {moved:.3e} ({gap / moved:.0f} x), the engine by {got_moved:.3e}")
    assert out.similarity.dtype == np.float64 and out.similarity[0] == 0.0 and got_moved < gap
    assert out.drop.tolist() == want_drop.tolist() and out.keep.tolist() == (~want_drop).tolist()
    # features in hand: the kernel's similarities on the engine's features, the same decisions
    feats = dd.features(frames, batch=3)
    again = dedup_features(feats, THRESHOLD)
    assert np.array_equal(again.similarity, out.similarity) and np.array_equal(again.drop, out.drop)
    s, d = D.adjacent_cosine(feats.cpu().numpy(), THRESHOLD)
    assert np.abs(s - out.similarity).max() <= sim_bar(64) and np.array_equal(d, out.drop)
