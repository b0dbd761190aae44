"""CLIP-I / CLIP-T scoring on the GPU: sg_clip_patchify_f16, ClipVisionEngine, ClipScorer and the unchanged ClipTextEngine against the CPU
restatements of tests/clip_vision_reference.py (pinned to torch / transformers by tests/test_clip_vision_reference.py).

Bars.  Patchify: the normalised values lie in about [-2.2, 2.7], where fp16 spacing is 2^-9, so half a spacing plus fp32 reassociation slack =
1.0e-3 absolute.  Hidden state: the relative bar tests/test_encoders_gpu.py applies to the text tower's hidden state on its tiny model, 3e-3.
Projected embedding and cosine have no counterpart there: their bars are 2x the larger of (a) the deviation from the fp32 restatement of a CPU
run of the restatement with fp16 rounding at the engine's rounding points and (b) the GPU's measured deviation from the fp32 restatement; both
are listed per case in EMBED_DEV / COSINE_DEV below and in profiles/r14a_clip_score.txt (one MI355X, one run)."""
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from oracle import encoders_oracle as eo
from tests import clip_vision_reference as R
from tests.test_clip_score_host import tiny_states

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F16, F32 = torch.float16, torch.float32
HIDDEN_BAR = 3e-3

# (B, H, W, S, ps)
PATCHIFY_CASES = [(1, 32, 32, 32, 8),        # identity
                  (3, 73, 73, 32, 8),        # non-integer downscale, 7 taps per axis
                  (1, 20, 20, 32, 8),        # upscale: support stays 2
                  (3, 81, 48, 32, 8),        # non-square, odd crop offset (11)
                  (1, 48, 80, 32, 8),        # crop offset 10.5 -> 10, along the other axis
                  (2, 512, 512, 224, 32)]    # the real geometry: 11 taps per axis, 49 patches of 3072 columns


def _image(B, H, W, lo, hi):
    g = torch.Generator().manual_seed(1000 * H + W)
    return torch.rand(B, 3, H, W, generator=g) * (hi - lo) + lo


def _patchify(gpu, x, S, ps, in_scale, in_shift):
    from storygen_amd import ops
    rows = x.shape[0] * (S // ps) ** 2
    out = torch.full((rows, 3 * ps * ps), float("nan"), dtype=F16, device=gpu)       # an element the kernel skips stays NaN
    ops.clip_patchify(x.to(gpu), out, S, ps, R.CLIP_MEAN, R.CLIP_STD, in_scale, in_shift)
    return out.cpu()


@pytest.mark.parametrize("affine", [(1.0, 0.0, 0.0, 1.0), (0.5, 0.5, -1.0, 1.0)], ids=["unit", "signed"])
@pytest.mark.parametrize("case", PATCHIFY_CASES, ids=lambda c: "B%d_%dx%d_to%d_ps%d" % c)
def test_patchify_kernel_vs_restatement(gpu, case, affine):
    B, H, W, S, ps = case
    in_scale, in_shift, lo, hi = affine
    x = _image(B, H, W, lo, hi)
    got = _patchify(gpu, x, S, ps, in_scale, in_shift)
    pre = R.preprocess(x, S, in_scale, in_shift)
    want = R.patch_rows(pre, ps)
    assert tuple(got.shape) == tuple(want.shape) == (B * (S // ps) ** 2, 3 * ps * ps)
    assert bool(torch.isfinite(got).all())
    err = float((got.float() - want).abs().max())
    print(f"patchify {case} affine {affine[:2]}: max abs error {err:.2e}, values in [{float(want.min()):.2f}, {float(want.max()):.2f}]")
    assert err < 1.0e-3
    if (H, W) == (S, S):
        m, s = torch.tensor(R.CLIP_MEAN).view(1, 3, 1, 1), torch.tensor(R.CLIP_STD).view(1, 3, 1, 1)
        exact = R.patch_rows(((x * in_scale + in_shift) - m) / s, ps).to(F16)
        ulp = torch.exp2(torch.floor(torch.log2(exact.float().abs().clamp_min(2.0 ** -14))) - 10)
        assert bool(((got.float() - exact.float()).abs() <= ulp).all())


@pytest.mark.parametrize("case", [(2, 81, 48, 32, 8), (1, 300, 260, 224, 32)], ids=lambda c: "B%d_%dx%d_to%d_ps%d" % c)
def test_patchify_columns_are_the_convolution_operand(gpu, case):
    """The patch GEMM of the kernel's rows against a random [C, 3*ps*ps] weight is the stride-ps convolution of the preprocessed image: a
    (c, dy, dx) mix-up would leave every value in place for the elementwise test's sorted eye, but not here.  Both operands carry one fp16
    rounding (relative 2^-11 each) and the sum is fp32: rel-L2 stays below 2 * 2^-11 = 1e-3; a wrong order gives O(1)."""
    from storygen_amd import ops
    B, H, W, S, ps = case
    Cc = 64
    x = _image(B, H, W, 0.0, 1.0)
    w = torch.randn(Cc, 3 * ps * ps, generator=torch.Generator().manual_seed(7)).half()
    rows = _patchify(gpu, x, S, ps, 1.0, 0.0).to(gpu)
    out = torch.empty(rows.shape[0], Cc, dtype=F32, device=gpu)
    ops.gemm(rows, w.to(gpu), out)
    want = F.conv2d(R.preprocess(x, S), w.float().view(Cc, 3, ps, ps), stride=ps).flatten(2).transpose(1, 2).reshape(-1, Cc)
    err = rel_l2(out.cpu(), want)
    print(f"patch GEMM vs conv2d {case}: rel-L2 {err:.2e}")
    assert err < 1e-3


def test_embed_patches_kernel(gpu):
    from storygen_amd import ops
    g = torch.Generator().manual_seed(0)
    B, T, Cc = 3, 17, 72
    buf = torch.randn(B * (T - 1), 80, generator=g).to(gpu)
    patches = buf[:, :Cc]                                                   # row-strided input
    cls, pos = torch.randn(Cc, generator=g).to(gpu), torch.randn(T, Cc, generator=g).to(gpu)
    out = torch.full((B * T, Cc), float("nan"), device=gpu)
    ops.clip_embed_patches(patches, cls, pos, out, T)
    want = torch.cat([cls.expand(B, 1, Cc), patches.reshape(B, T - 1, Cc)], 1) + pos[None]
    assert torch.equal(out.view(B, T, Cc), want)


# -------------------------------------------------------------------------------------------------------------- vision engine
# name: (hidden, heads, image, patch, input H x W).  All: 2 layers, quick_gelu, projection_dim 32.
ENGINE_CASES = {"d32_t17": (64, 2, 32, 8, (40, 56)),           # D = 32
                "d64_t65": (128, 2, 64, 8, (70, 90)),          # D = 64, the attention kernel's limit
                "d32_t122": (64, 2, 88, 8, (100, 96)),         # 121 patches: near the T = 128 limit
                "d32_t50_k3072": (64, 2, 224, 32, (256, 300))}  # ViT-B/32 geometry: K = 3072 in the patch GEMM
# rel-L2 deviation of image_embeds from the fp32 restatement: (CPU restatement with fp16 rounding points, GPU measured)
EMBED_DEV = {"d32_t17": (2.86e-4, 2.57e-4), "d64_t65": (2.62e-4, 2.74e-4), "d32_t122": (3.37e-4, 3.76e-4), "d32_t50_k3072": (3.18e-4, 3.03e-4)}


def _engine_case(name):
    hidden, heads, image, patch, hw = ENGINE_CASES[name]
    vsd, _ = tiny_states(seed=len(name), hidden=hidden, heads=heads, image=image, patch=patch)
    x = _image(2, hw[0], hw[1], 0.0, 1.0)
    px = R.preprocess(x, image)
    return vsd, heads, x, R.vision_forward(vsd, px, heads), R.vision_forward(vsd, px, heads, round_operands=True)


def embed_bar(name):
    cpu16, gpu_dev = EMBED_DEV[name]
    return 2 * max(cpu16, gpu_dev)


@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_vision_engine_vs_restatement(gpu, name):
    from storygen_amd.encoders import ClipVisionEngine
    vsd, heads, x, (want_e, want_h), (r_e, r_h) = _engine_case(name)
    eng = ClipVisionEngine(vsd, gpu, heads=heads)
    embeds, hidden = eng(x)
    assert tuple(hidden.shape) == tuple(want_h.shape) and tuple(embeds.shape) == tuple(want_e.shape) and hidden.dtype == F32
    eh, ee = rel_l2(hidden.cpu(), want_h), rel_l2(embeds.cpu(), want_e)
    print(f"vision engine {name}: hidden rel-L2 {eh:.2e} (fp16-rounded CPU restatement {rel_l2(r_h, want_h):.2e}, bar {HIDDEN_BAR:.1e}); "
          f"image_embeds rel-L2 {ee:.2e} (fp16-rounded CPU restatement {rel_l2(r_e, want_e):.2e}, bar {embed_bar(name):.1e})")
    assert eh < HIDDEN_BAR
    assert ee < embed_bar(name)
    e2, h2 = eng(x)
    assert torch.equal(e2, embeds) and torch.equal(h2, hidden)


def test_dropin_vision_model_forward(gpu):
    from storygen_amd.model import CLIPVisionModelWithProjection
    cfg = dict(hidden_size=64, intermediate_size=128, projection_dim=32, num_hidden_layers=2, num_attention_heads=2, image_size=32, patch_size=8)
    m = CLIPVisionModelWithProjection(cfg, seed=6)
    m.load_state_dict(tiny_states(seed=7)[0])
    m = m.to(gpu)
    px = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(8))
    out = m(px.to(gpu))
    want_e, want_h = R.vision_forward({k: v.cpu() for k, v in m.state_dict().items()}, px, heads=2)
    assert out.image_embeds.dtype == F32 and tuple(out.image_embeds.shape) == (2, 32) and tuple(out.last_hidden_state.shape) == (2, 17, 64)
    assert rel_l2(out.last_hidden_state.cpu(), want_h) < HIDDEN_BAR and rel_l2(out.image_embeds.cpu(), want_e) < embed_bar("d32_t17")


# --------------------------------------------------------------------------------------------------------------------- scorer
# max abs deviation of the CLIP-I / CLIP-T cosines of test_clip_scorer_end_to_end from the fp32 restatement's: (CPU run with fp16 rounding at
# the engines' rounding points — both engines over tests/clip_ops_emulation.py, CLIP-T being the larger of the two —, GPU measured)
COSINE_DEV = (1.20e-4, 6.82e-5)


def test_clip_scorer_end_to_end(gpu):
    from storygen_amd.clip_score import ClipScorer
    bar = 2 * max(COSINE_DEV)
    vsd, tsd = tiny_states(seed=5)
    vcfg = dict(hidden_size=64, num_attention_heads=2, image_size=32, patch_size=8)
    tcfg = dict(hidden_size=64, num_attention_heads=2)
    g = torch.Generator().manual_seed(9)
    a, b = torch.rand(3, 40, 56, 3, generator=g).numpy(), torch.rand(3, 40, 56, 3, generator=g).numpy()
    ids = torch.randint(0, 95, (3, 77), generator=g)
    ids[:, 20] = 95
    nchw = lambda t: torch.from_numpy(t).permute(0, 3, 1, 2)   # noqa: E731
    pa, pb = R.preprocess(nchw(a), 32), R.preprocess(nchw(b), 32)
    fa, fb = R.vision_forward(vsd, pa, 2)[0], R.vision_forward(vsd, pb, 2)[0]
    ft = eo.clip_text_forward(tsd, ids, heads=2)[1] @ tsd["text_projection.weight"].t()
    ra, rb = R.vision_forward(vsd, pa, 2, round_operands=True)[0], R.vision_forward(vsd, pb, 2, round_operands=True)[0]
    sc = ClipScorer(vsd, vcfg, tsd, tcfg, device=gpu)
    ci, ct, same = sc.clip_i(a, b), sc.clip_t(a, ids), sc.clip_i(a, a)
    assert ci.dtype == F32 and ci.is_cuda and tuple(ci.shape) == (3,) and tuple(ct.shape) == (3,)
    di, dt = float((ci.cpu() - R.cosine(fa, fb)).abs().max()), float((ct.cpu() - R.cosine(fa, ft)).abs().max())
    print(f"scorer: CLIP-I {ci.tolist()} max abs deviation {di:.2e} (fp16-rounded CPU restatement {float((R.cosine(ra, rb) - R.cosine(fa, fb)).abs().max()):.2e}); "
          f"CLIP-T {ct.tolist()} max abs deviation {dt:.2e}; bar {bar:.1e}")
    assert float((same.cpu() - 1).abs().max()) < bar
    assert di < bar and dt < bar
    assert torch.equal(sc.clip_i(nchw(a), nchw(b)), ci)                      # the NCHW tensor and the numpy array are the same input
    signed = ClipScorer(vsd, vcfg, device=gpu, in_scale=0.5, in_shift=0.5)
    assert float((signed.clip_i(nchw(a) * 2 - 1, nchw(b) * 2 - 1).cpu() - R.cosine(fa, fb)).abs().max()) < bar
    # rejected on the host, before anything is launched (nothing of these state dicts is ever read)
    with pytest.raises(ValueError, match="257 tokens"):
        ClipScorer({}, dict(hidden_size=1024, num_attention_heads=16, image_size=224, patch_size=14), device=gpu)
    with pytest.raises(ValueError, match="head dim"):
        ClipScorer({}, dict(hidden_size=1280, num_attention_heads=16, image_size=224, patch_size=32), device=gpu)


# ----------------------------------------------------------------------------------------------------------------- text tower
def test_clip_text_engine_bits_unchanged(gpu):
    """tests/golden/clip_text_bitexact.pt holds ClipTextEngine's output as the commit before the layer loop was shared with the image tower
    produced it on an MI355X (tools/make_clip_text_bitexact.py): the refactored engine must give the same bits."""
    from storygen_amd.encoders import ClipTextEngine
    gold = torch.load(os.path.join(GOLDEN, "clip_text_bitexact.pt"), weights_only=True)
    eng = ClipTextEngine(gold["state_dict"], gpu, heads=gold["heads"])
    hidden, pooled = eng(gold["input_ids"])
    assert torch.equal(hidden.cpu(), gold["hidden"]) and torch.equal(pooled.cpu(), gold["pooled"])
    hm, pm = eng(gold["input_ids"][:1, :24], attention_mask=gold["mask"])
    assert torch.equal(hm.cpu(), gold["hidden_masked"]) and torch.equal(pm.cpu(), gold["pooled_masked"])
    with pytest.raises(KeyError):
        eng.project(pooled)                                                    # this checkpoint has no text_projection
