"""PickScore on the GPU: sg_attn_enc_f16, sg_clip_patchify_padk_f16, ClipVisionEngine(wide=True), PickScorer and the drop-in CLIPModel against
float64 torch and the CPU restatements of tests/pick_score_reference.py (pinned to transformers by tests/test_pick_score_reference.py).

Bars.  Attention: rel-L2 < 1.5e-3 against float64 — the bar tests/test_kernels_gpu.py::test_attention_small applies to the same contract with
the same fp16 output.  The kernel streams keys in tiles of KEY_TILE = 64 and gives each workgroup 128 queries, so the shapes sit on and either
side of 64 and 128.  Patchify: the existing 1.0e-3 absolute (half an fp16 spacing at |x| < 4 plus slack); patch GEMM vs conv2d: the existing
1e-3 rel-L2.  Hidden state: HIDDEN_BAR = 3e-3 as in tests/test_clip_score_gpu.py.  Projected embedding, cosine and score: 2 x the larger of (a)
the deviation from the fp32 restatement of the CPU restatement with fp16 rounding at the engines' rounding points and (b) the GPU's measured
deviation; both are listed per case in EMBED_DEV / COSINE_DEV / FEATURE_DEV below and in profiles/r16a_pick_score.txt.  STATE OF (b): None = not yet
measured — no MI355X could be reached when these tests were written, so the bars below stand on (a) alone (tests/test_clip_score_gpu.py, same
method, same engines: the GPU's deviation was 0.9 - 1.1 x the CPU-rounded one in all four of its cases).  Fill (b) in from the printed figures
of the first hardware run (`-s`)."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from tests import clip_vision_reference as R
from tests import pick_score_reference as P

pytestmark = pytest.mark.gpu
F16, F32 = torch.float16, torch.float32
ATTN_BAR = 1.5e-3
HIDDEN_BAR = 3e-3
KEY_TILE = 64
FMIN = torch.finfo(torch.float32).min


# ---------------------------------------------------------------------------------------------------------------- attention kernel
def _bias(kind, B, T):
    if kind is None:
        return None
    kb = torch.zeros(B, T)
    if kind == "tail":                 # the trailing quarter of the keys: a padding mask
        kb[:, T - T // 4:] = FMIN
    elif kind == "tile":               # one whole key tile in the middle
        kb[:, KEY_TILE:2 * KEY_TILE] = FMIN
    elif kind == "first":              # everything except key 0: every later tile is masked in full
        kb[:, 1:] = FMIN
    elif kind == "ragged":             # a different number of live keys per batch row, plus a finite bias on the live ones
        kb = 0.5 * torch.randn(B, T, generator=torch.Generator().manual_seed(T))
        for b in range(B):
            kb[b, T - 1 - 7 * b - T // 5:] = FMIN
    return kb


def _reference(q, k, v, heads, scale, causal, kb):
    B, T, C = q.shape
    D = C // heads
    qh, kh, vh = (t.double().view(B, T, heads, D).transpose(1, 2) for t in (q, k, v))
    s = (qh @ kh.transpose(-1, -2)) * scale
    if kb is not None:
        s = s + kb.double()[:, None, None, :]
    if causal:
        s = s + torch.full((T, T), float("-inf"), dtype=torch.float64).triu(1)
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, T, C)


def _run_enc(gpu, qkv, heads, scale, causal, kb, separate=False):
    """q, k, v = slices of one fused [B, T, 3 * H * D] buffer (or, separate=True, three buffers with distinct batch strides); the output has a
    token stride of H * D + 16 and is NaN-prefilled."""
    from storygen_amd import ops
    B, T, C3 = qkv.shape
    C = C3 // 3
    dq = qkv.to(gpu)
    q, k, v = dq[:, :, :C], dq[:, :, C:2 * C], dq[:, :, 2 * C:]
    if separate:
        kbuf = torch.zeros(B, T + 3, C + 8, dtype=F16, device=gpu)
        vbuf = torch.zeros(B, T + 5, C, dtype=F16, device=gpu)
        kbuf[:, :T, :C], vbuf[:, :T] = k, v
        k, v = kbuf[:, :T, :C], vbuf[:, :T]
        assert len({q.stride(0), k.stride(0), v.stride(0)}) == 3
    obuf = torch.full((B, T, C + 16), float("nan"), dtype=F16, device=gpu)
    out = obuf[:, :, :C]
    ops.attention_enc(q, k, v, out, heads, scale, causal, None if kb is None else kb.to(gpu))
    return out, obuf, (q, k, v)


def _check_enc(gpu, B, H, T, D, causal=False, bias=None, separate=False, gain=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * T + D)
    qkv = torch.randn(B, T, 3 * H * D, generator=g)
    qkv[:, :, :2 * H * D] *= gain
    qkv = qkv.half()
    C = H * D
    kb = _bias(bias, B, T)
    scale = D ** -0.5
    out, obuf, _ = _run_enc(gpu, qkv, H, scale, causal, kb, separate)
    got = out.cpu()
    assert bool(torch.isfinite(got).all()), "non-finite output"
    assert bool(torch.isnan(obuf[:, :, C:]).all()), "guard columns written"
    want = _reference(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], H, scale, causal, kb)
    err = rel_l2(got, want)
    print(f"attention_enc B{B} H{H} T{T} D{D} causal={causal} bias={bias} gain={gain}: rel-L2 {err:.2e} (bar {ATTN_BAR:.1e})")
    assert err < ATTN_BAR
    return qkv, kb, got


# T in {1, 63, 64, 65, 129, 257, 1024} x D in {8, 40, 64, 72, 80, 128}: every T and every D at least once, the key tile (64) and the query
# block (128) each with +-1 / +1, every padded head-dim class (32, 64, 96, 128) at more than one tile of keys
SHAPES = [(2, 2, 1, 8), (1, 3, 1, 80), (2, 3, 63, 40), (2, 2, 64, 64), (2, 2, 65, 72), (3, 2, 65, 8), (1, 2, 129, 128), (2, 2, 129, 40),
          (2, 4, 257, 80), (1, 2, 257, 64), (1, 1, 1024, 80), (1, 1, 1024, 128), (1, 2, 1024, 8)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_H%d_T%d_D%d" % s)
def test_attention_enc_shapes(gpu, shape):
    _check_enc(gpu, *shape)


@pytest.mark.parametrize("shape", [(2, 16, 77, 64), (2, 4, 257, 80)], ids=lambda s: "B%d_H%d_T%d_D%d" % s)
def test_attention_enc_causal(gpu, shape):
    _check_enc(gpu, *shape, causal=True)


@pytest.mark.parametrize("bias,causal", [("tail", False), ("tile", False), ("first", False), ("ragged", False), ("tail", True), ("tile", True)])
def test_attention_enc_key_bias(gpu, bias, causal):
    """A key bias of finfo(float32).min (ClipTextEngine's padding mask): a trailing quarter, one whole key tile in the middle (no NaN, the
    running maximum undisturbed), everything but key 0, and with the causal mask on top."""
    _check_enc(gpu, 2, 4, 257, 80, causal=causal, bias=bias)


def test_attention_enc_first_key_only_is_exact(gpu):
    """Every row attends to key 0 only: P is exactly (1, 0, 0, ...), so the output is V[0] of the head bit for bit."""
    qkv, _, got = _check_enc(gpu, 2, 4, 257, 80, bias="first", seed=3)
    v0 = qkv[:, :1, 2 * 320:]
    assert torch.equal(got, v0.expand_as(got))


def test_attention_enc_distinct_batch_strides(gpu):
    _check_enc(gpu, 3, 2, 129, 80, separate=True)
    _check_enc(gpu, 3, 2, 77, 64, causal=True, bias="ragged", separate=True)


def test_attention_enc_large_logits(gpu):
    """q and k scaled so that scale * q.k reaches about +-60: without the subtraction of the running maximum exp overflows fp16 P / fp32 sums."""
    D, gain = 80, 4.2        # std of scale * q.k = gain^2 = 17.6; the extremes over 257 keys are beyond 3 sigma, about +-60
    g = torch.Generator().manual_seed(1)
    qk = torch.randn(2, 257, 2 * 2 * D, generator=g) * gain
    smax = float(((qk[:, :, :D].double() @ qk[:, :, 2 * D:3 * D].double().transpose(1, 2)) * D ** -0.5).abs().max())
    assert 45.0 < smax < 120.0, smax
    _check_enc(gpu, 2, 2, 257, D, gain=gain)
    _check_enc(gpu, 2, 2, 257, D, gain=gain, causal=True)


@pytest.mark.parametrize("shape,causal,bias", [((2, 12, 77, 64), True, "ragged"), ((2, 2, 128, 64), False, None), ((3, 2, 65, 40), False, "tail"),
                                                ((2, 3, 17, 32), False, None)])
def test_attention_enc_agrees_with_attention_small(gpu, shape, causal, bias):
    from storygen_amd import ops
    B, H, T, D = shape
    qkv, kb, got = _check_enc(gpu, B, H, T, D, causal=causal, bias=bias)
    dq = qkv.to(gpu)
    C = H * D
    small = torch.empty(B, T, C, dtype=F16, device=gpu)
    ops.attention_small(dq[:, :, :C], dq[:, :, C:2 * C], dq[:, :, 2 * C:], small, H, D ** -0.5, causal, None if kb is None else kb.to(gpu))
    err = rel_l2(got, small.cpu())
    print(f"attention_enc vs attention_small {shape}: rel-L2 {err:.2e}")
    assert err < 2 * ATTN_BAR


def test_attention_enc_is_deterministic(gpu):
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(2, 257, 3 * 4 * 80, generator=g).half()
    kb = _bias("tail", 2, 257)
    a, _, _ = _run_enc(gpu, qkv, 4, 80 ** -0.5, True, kb)
    b, _, _ = _run_enc(gpu, qkv, 4, 80 ** -0.5, True, kb)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- padded patchify
def _image(B, H, W):
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(1000 * H + W))


@pytest.mark.parametrize("case", [(2, 70, 90, 28, 14), (2, 512, 512, 224, 14)], ids=lambda c: "B%d_%dx%d_to%d_ps%d" % c)
def test_padded_patchify(gpu, case):
    from storygen_amd import ops
    B, H, W, S, ps = case
    K, Kpad = 3 * ps * ps, (3 * ps * ps + 7) & ~7
    assert (K, Kpad) == (588, 592)
    x = _image(B, H, W)
    rows = B * (S // ps) ** 2
    out = torch.full((rows, Kpad + 8), float("nan"), dtype=F16, device=gpu)
    ops.clip_patchify(x.to(gpu), out, S, ps, R.CLIP_MEAN, R.CLIP_STD, kpad=Kpad)
    got = out.cpu()
    want = R.patch_rows(R.preprocess(x, S), ps)
    err = float((got[:, :K].float() - want).abs().max())
    print(f"padded patchify {case}: max abs error {err:.2e}")
    assert err < 1.0e-3
    assert bool((got[:, K:Kpad] == 0).all()) and bool(torch.isnan(got[:, Kpad:]).all())
    # the patch GEMM against a weight with zero columns appended is the stride-14 convolution
    Cc = 64
    w = torch.randn(Cc, K, generator=torch.Generator().manual_seed(7)).half()
    a = out[:, :Kpad].contiguous()
    y = torch.empty(rows, Cc, dtype=F32, device=gpu)
    ops.gemm(a, F.pad(w, (0, Kpad - K)).to(gpu), y)
    conv = F.conv2d(R.preprocess(x, S), w.float().view(Cc, 3, ps, ps), stride=ps).flatten(2).transpose(1, 2).reshape(-1, Cc)
    e2 = rel_l2(y.cpu(), conv)
    print(f"padded patch GEMM vs conv2d {case}: rel-L2 {e2:.2e}")
    assert e2 < 1e-3


# ---------------------------------------------------------------------------------------------------------------- vision engine
# name: (hidden, heads, image, patch, input H x W).  All: 2 layers, gelu, projection_dim 32, batch 2.
ENGINE_CASES = {"d80_t82": (160, 2, 126, 14, (150, 170)),       # head dim 80, ps 14 (K 588 -> 592), two key tiles
                "d80_t257": (160, 2, 224, 14, (256, 300)),      # the real token count
                "d64_t257": (128, 2, 224, 14, (240, 240))}      # ViT-L/14's head dim at 257 tokens
# rel-L2 deviation of image_embeds from the fp32 restatement: (CPU restatement with fp16 rounding points, GPU measured)
EMBED_DEV = {"d80_t82": (2.43e-4, None), "d80_t257": (3.09e-4, None), "d64_t257": (3.75e-4, None)}


def dev_bar(dev):
    """2 x max(CPU-rounded deviation, GPU-measured deviation); a figure not yet measured (None) does not enter."""
    return 2 * max(v for v in dev if v is not None)


def _engine_case(name):
    hidden, heads, image, patch, hw = ENGINE_CASES[name]
    cfg = P.tiny_config(vision_hidden=hidden, vision_heads=heads, image=image, patch=patch)
    sd = P.tiny_state(seed=len(name) + image, config=cfg)
    x = _image(2, *hw)
    px = R.preprocess(x, image)
    want = R.vision_forward(sd, px, heads, hidden_act="gelu")
    rounded = R.vision_forward(sd, px, heads, hidden_act="gelu", round_operands=True)
    return sd, heads, x, want, rounded


@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_wide_vision_engine_vs_restatement(gpu, name):
    from storygen_amd.encoders import ClipVisionEngine
    sd, heads, x, (want_e, want_h), (r_e, r_h) = _engine_case(name)
    eng = ClipVisionEngine(sd, gpu, heads=heads, hidden_act="gelu", wide=True)
    embeds, hidden = eng(x)
    assert tuple(hidden.shape) == tuple(want_h.shape) and tuple(embeds.shape) == tuple(want_e.shape) and hidden.dtype == F32
    eh, ee = rel_l2(hidden.cpu(), want_h), rel_l2(embeds.cpu(), want_e)
    bar = dev_bar(EMBED_DEV[name])
    print(f"wide vision engine {name}: hidden rel-L2 {eh:.2e} (fp16-rounded CPU restatement {rel_l2(r_h, want_h):.2e}, bar {HIDDEN_BAR:.1e}); "
          f"image_embeds rel-L2 {ee:.2e} (fp16-rounded CPU restatement {rel_l2(r_e, want_e):.2e}, bar {bar:.1e})")
    assert eh < HIDDEN_BAR
    assert ee < bar
    e2, h2 = eng(x)
    assert torch.equal(e2, embeds) and torch.equal(h2, hidden)


def test_wide_engine_on_a_small_tower_is_the_default_engine(gpu):
    """D = 32, T = 17: wide=True changes neither the attention entry point nor the patch rows, so the bits are the default engine's."""
    from storygen_amd.encoders import ClipVisionEngine
    from tests.test_clip_score_host import tiny_states
    vsd, _ = tiny_states(seed=7)
    x = _image(2, 40, 56)
    e0, h0 = ClipVisionEngine(vsd, gpu, heads=2)(x)
    e1, h1 = ClipVisionEngine(vsd, gpu, heads=2, wide=True)(x)
    assert torch.equal(e0, e1) and torch.equal(h0, h1)


# ------------------------------------------------------------------------------------------------------------------- PickScorer
SCORER_SEEDS = (2, 13)         # (state seed, input seed): tests/test_pick_score_reference.py asserts the top-two score gap for these
# max abs deviation of the 5 cosines from the fp32 restatement's: (CPU restatement with fp16 rounding points, GPU measured)
COSINE_DEV = (1.046e-4, None)
# rel-L2 deviation of (image features, text features) from the fp32 restatement: (CPU rounded, GPU measured)
FEATURE_DEV = {"image": (3.18e-4, None), "text": (2.47e-4, None)}


def cosine_bar():
    return dev_bar(COSINE_DEV)


def test_pick_scorer_end_to_end(gpu):
    from storygen_amd.model import CLIPModel
    from storygen_amd.pick_score import PickScorer
    cfg = P.tiny_config()
    sd = P.tiny_state(SCORER_SEEDS[0], cfg)
    frames, ids = P.tiny_inputs(SCORER_SEEDS[1])
    px = P.preprocess_frames(frames, cfg["vision_config"]["image_size"])
    want_i, want_t = P.image_features(sd, cfg, px), P.text_features(sd, cfg, ids)
    want_s = P.scores(sd, cfg, ids, px)
    want_cos = P.cosines(want_t, want_i)
    r_cos = P.cosines(P.text_features(sd, cfg, ids, round_operands=True), P.image_features(sd, cfg, px, round_operands=True))
    scale = float(sd["logit_scale"].exp())
    sc = PickScorer(sd, cfg, device=gpu)
    fi, ft = sc.image_features(frames), sc.text_features(ids)
    assert fi.dtype == F32 and fi.is_cuda and tuple(fi.shape) == (5, 32) and tuple(ft.shape) == (1, 32)
    s = sc.scores(ids, frames)
    assert tuple(s.shape) == (1, 5) and s.dtype == F32
    dcos = float((s.cpu() / scale - want_cos).abs().max())
    dscore = float((s.cpu() - want_s).abs().max())
    print(f"PickScorer: image features rel-L2 {rel_l2(fi.cpu(), want_i):.2e}, text features rel-L2 {rel_l2(ft.cpu(), want_t):.2e}; cosine max abs "
          f"deviation {dcos:.2e} (fp16-rounded CPU restatement {float((r_cos - want_cos).abs().max()):.2e}, bar {cosine_bar():.1e}); score max abs "
          f"deviation {dscore:.2e} (bar {scale * cosine_bar():.2e}); scores {s.cpu().tolist()} want {want_s.tolist()}")
    assert rel_l2(fi.cpu(), want_i) < dev_bar(FEATURE_DEV["image"]) and rel_l2(ft.cpu(), want_t) < dev_bar(FEATURE_DEV["text"])
    assert dcos < cosine_bar()
    assert dscore < scale * cosine_bar()
    p = sc.probs(ids, frames)
    assert abs(float(p.sum()) - 1.0) < 1e-5 and float((p.cpu() - torch.softmax(want_s, -1)).abs().max()) < scale * cosine_bar()
    idx, pb = sc.best_of(ids, frames)
    assert idx == int(want_s[0].argmax()) and torch.equal(pb, p[0])
    nchw = torch.from_numpy(frames).permute(0, 3, 1, 2)
    assert torch.equal(sc.scores(ids, nchw), s)                              # the NCHW tensor and the numpy array are the same input
    with pytest.raises(ValueError, match="one prompt"):
        sc.best_of(torch.cat([ids, ids]), frames)
    # the drop-in CLIPModel, fed what a CLIPImageProcessor returns, gives the scorer's features
    m = CLIPModel(cfg)
    m.load_state_dict(sd)
    m = m.to(gpu)
    gi = m.get_image_features(pixel_values=px.to(gpu))
    gt = m.get_text_features(input_ids=ids.to(gpu), attention_mask=torch.ones_like(ids).to(gpu))
    assert rel_l2(gi.cpu(), want_i) < dev_bar(FEATURE_DEV["image"]) and rel_l2(gi.cpu(), fi.cpu()) < 1.0e-3
    assert torch.equal(gt, ft)                                               # an all-ones mask adds an exact zero to every score
    assert abs(float(m.logit_scale.exp()) - scale) < 1e-3 * scale


# ------------------------------------------------------------------------------------------------------------- the real geometry
def test_vit_h14_geometry_two_layers(gpu):
    """ViT-H/14's widths (hidden 1280, 16 heads of 80, MLP 5120, patch 14, image 224: 257 tokens) with 2 layers: the only place the 1280-wide
    GEMM shapes meet the new attention kernel."""
    from storygen_amd.encoders import ClipVisionEngine, clip_vision_param_shapes, init_state
    sd = init_state(clip_vision_param_shapes(1280, 5120, 2, 224, 14, 1024), seed=3)
    g = torch.Generator().manual_seed(4)
    for k in sd:
        if "norm" in k:
            sd[k] = sd[k] + 0.2 * torch.randn(sd[k].shape, generator=g)
        if "embedding" in k:
            sd[k] = sd[k] * 10
        sd[k] = sd[k].half().float()
    x = _image(2, 256, 256)
    want_e, want_h = R.vision_forward(sd, R.preprocess(x, 224), 16, hidden_act="gelu")
    eng = ClipVisionEngine(sd, gpu, heads=16, hidden_act="gelu", image_size=224, wide=True)
    embeds, hidden = eng(x)
    assert tuple(hidden.shape) == (2, 257, 1280) and tuple(embeds.shape) == (2, 1024)
    assert bool(torch.isfinite(hidden).all()) and bool(torch.isfinite(embeds).all())
    eh = rel_l2(hidden.cpu(), want_h)
    print(f"ViT-H/14 widths, 2 layers: hidden rel-L2 {eh:.2e} (bar {HIDDEN_BAR:.1e}), image_embeds rel-L2 {rel_l2(embeds.cpu(), want_e):.2e}")
    assert eh < HIDDEN_BAR
    e2, h2 = eng(x)
    assert torch.equal(e2, embeds) and torch.equal(h2, hidden)
