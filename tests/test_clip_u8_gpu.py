"""Scoring 8-bit frames on the GPU: sg_clip_patchify_u8 (ops.clip_patchify_u8) and everything above it against the restatement of
tests/clip_u8_reference.py (PIL's resize, crop, fp32 normalisation, patch rows), which tests/test_clip_u8_host.py pins to transformers'
PIL image processor.  Every comparison is exact — the uint8 bytes of the cropped image and the fp16 bit patterns of the patch rows — so
there are no tolerances.  Geometries are written width x height; arrays are [h, w, 3]."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_story_gpu import PROMPTS, SIZE, _pipeline, rig  # noqa: F401  (rig: that module's fixture, built once for this one too)
from tests import clip_u8_reference as U
from tests import pick_score_reference as P

pytestmark = pytest.mark.gpu
F16, I16 = torch.float16, torch.int16
TOWERS = [(32, 8), (28, 14), (64, 32)]           # (S, ps): K = 192 (no padding), 588 -> 592, 3072


def _pattern(n, gpu):
    """fp16 bit patterns that no result equals by accident (NaNs among them), to be found untouched around the output window."""
    return (torch.arange(n, device=gpu) % 2039 + 0x7C01).to(I16).view(F16)


def _check(gpu, a, S, ps, crop="torchvision", geom=None, kpad=None, what=""):
    """a uint8 [N,h,w,3] on the host -> both outputs of one launch equal the restatement; the row buffer is 8 columns wider than kpad."""
    from storygen_amd import ops
    N, K = a.shape[0], 3 * ps * ps
    kpad = (K + 7) & ~7 if kpad is None else kpad
    rows = N * (S // ps) ** 2
    buf = _pattern(rows * (kpad + 8), gpu).view(rows, kpad + 8)
    guard = buf[:, kpad:].clone()
    u8 = torch.full((N, S, S, 3), 0xA5, dtype=torch.uint8, device=gpu)
    got = ops.clip_patchify_u8(torch.from_numpy(a).to(gpu), buf[:, :kpad], S, ps, U.CLIP_MEAN, U.CLIP_STD, geometry=geom, crop=crop, kpad=kpad,
                               out_u8=u8)
    want_u8, want_rows = U.reference(list(a), S, ps, crop, geom, kpad)
    assert got.data_ptr() == buf.data_ptr() and want_rows.shape == (rows, kpad) and not want_rows[:, K:].any()
    bad = int((u8.cpu().numpy() != want_u8).sum()), int((buf[:, :kpad].cpu().view(I16).numpy() != want_rows.view(np.int16)).sum())
    assert bad == (0, 0), f"{what} {a.shape} -> S {S} ps {ps} {crop} {geom}: {bad[0]} uint8 and {bad[1]} fp16 mismatches of {want_u8.size}"
    assert torch.equal(buf[:, kpad:].view(I16), guard.view(I16)), f"{what}: columns >= Kpad written"
    return want_u8, want_rows


# h x w sources: 70 x 50 and 33 x 90 (width x height) and an upscale (20 x 13)
SOURCES = [(50, 70), (90, 33), (13, 20)]


@pytest.mark.parametrize("tower", TOWERS, ids=lambda t: "S%d_ps%d" % t)
@pytest.mark.parametrize("hw", SOURCES, ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_geometries_towers_and_contents(gpu, hw, tower):
    """Random bytes, the 0 / 255 checkerboard of 3-pixel cells (Pillow's clip acts at both ends, in both passes) and constant 255, under
    both crop rules, N = 2."""
    (h, w), (S, ps) = hw, tower
    for kind in ("random", "checker", "white"):
        for crop in U.CROPS if kind != "white" else U.CROPS[:1]:
            _check(gpu, U.content(kind, h, w, seed=S, n=2), S, ps, crop, what=kind)


@pytest.mark.parametrize("side,tower,rows", [(1000, (32, 8), 7), (896, (28, 14), 7), (976, (32, 8), 8)], ids=["1000_to_32", "896_to_28", "976_to_32"])
def test_shrink_ratio_at_its_limit(gpu, side, tower, rows):
    """1000 x 1000 -> 32 (ratio 31.25, 127 taps) and 896 x 896 -> 28 (32 exactly, 129 taps: the largest kernel): the rows per tile are
    lowered to 7 so that the staged rows fit the LDS budget.  976 -> 32 (30.5): 8 rows per tile stage 337 input rows, 64 704 bytes, which
    fit the budget alone (sg_image_resize_u8 takes 8) and not beside the 1 536 bytes of the normalisation table (this launch takes 7)."""
    from storygen_amd import ops
    assert ops.image_resize_tile_rows(side, tower[0], 3) == rows
    _check(gpu, U.content("random", side, side, seed=1, n=1), *tower, what="ratio")


@pytest.mark.parametrize("tower", TOWERS, ids=lambda t: "S%d_ps%d" % t)
def test_crop_offsets_where_the_rules_differ_and_where_they_agree(gpu, tower):
    """size - S = 5 (1 mod 4: both rules give 2) and 7 (3 mod 4: torchvision 4, floor 3), on either axis, with the short side at S (one
    pass skipped) and at 2 S (both passes)."""
    S, ps = tower
    for h, w, d in ((S + 5, S, 5), (S, S + 7, 7), (2 * S + 10, 2 * S, 5), (2 * S, 2 * S + 14, 7)):
        tv, fl = U.geometry(h, w, S, "torchvision"), U.geometry(h, w, S, "floor")
        assert max(tv[0], tv[1]) == S + d and (tv != fl) == (d == 7)
        a = U.content("random", h, w, seed=d, n=2)
        got = [_check(gpu, a, S, ps, crop, what=f"offset d={d}")[0] for crop in U.CROPS]
        assert np.array_equal(got[0], got[1]) == (d == 5)


def test_both_passes_skipped_cover_every_byte_in_every_channel(gpu):
    """Short side == S on a square image: nothing is resampled, the crop is the image, and an image holding all 256 byte values in each
    channel exercises all 768 (byte, channel) results of the normalisation."""
    for S, ps in TOWERS:
        a = U.content("ramp", S, S, n=2)
        u8, rows = _check(gpu, a, S, ps, what="identity")
        assert np.array_equal(u8, a)
        assert all(len(np.unique(rows[:, c * ps * ps:(c + 1) * ps * ps].view(np.int16))) == 256 for c in range(3))


@pytest.mark.parametrize("geom", [(50, 39, 11, 5), (40, 70, 3, 20), (31, 45, 2, 9), (50, 70, 22, 42), (28, 28, 0, 0), (100, 28, 72, 0)],
                         ids=lambda g: "%dx%d_at_%d_%d" % (g[1], g[0], g[2], g[3]))
def test_explicit_geometry_one_pass_only_and_any_window(gpu, geom):
    """Hr, Wr, top, left through the ABI on a 70 x 50 source, S = 28: the vertical pass skipped (Hr == 50), the horizontal one skipped
    (Wr == 70), a resize that keeps no aspect ratio, no pass with an off-centre window in its last rows and columns, both axes shrunk to S,
    and an upscaled height with the window at the bottom."""
    for kind in ("random", "checker"):
        _check(gpu, U.content(kind, 50, 70, seed=9, n=2), 28, 14, geom=geom, what=kind)
    _check(gpu, U.content("random", 50, 70, seed=2, n=1), 28, 7, geom=geom, kpad=160, what="Kpad 13 columns above 3 ps^2")


@pytest.mark.parametrize("kind,crop", [("random", "floor"), ("checker", "floor"), ("random", "torchvision")])
def test_real_tile_case(gpu, kind, crop):
    """S = 224, ps = 14, N = 2 from a 256 x 300 source: 3.5 output tiles per row, patches that straddle tile edges in both directions."""
    u8, rows = _check(gpu, U.content(kind, 300, 256, seed=4, n=2), 224, 14, crop, what="ViT-H/14 rows")
    assert rows.shape == (512, 592)


@pytest.mark.parametrize("offset", [0, 1, 3], ids=lambda o: f"byte{o}")
@pytest.mark.parametrize("case", [((50, 70), 28, 14, None), ((90, 33), 32, 8, None), ((28, 28), 28, 14, None), ((50, 70), 28, 14, (50, 39, 11, 5)),
                                  ((40, 70), 28, 14, (40, 70, 12, 42))], ids=["both", "both_tall", "none", "horizontal", "no_pass_window"])
def test_windows_batches_and_unaligned_bases(gpu, case, offset):
    """N = 3.  Input = a window (batch and row stride) of a larger buffer that starts `offset` bytes past an aligned address; the patch rows
    = a window (ldo > Kpad, `offset` elements past an aligned address) of a buffer pre-filled with a bit pattern, the uint8 output likewise:
    every element outside the windows, columns >= Kpad included, must stay as it was.  Then the patch rows alone."""
    from storygen_amd import ops
    (h, w), S, ps, geom = case
    N, K = 3, 3 * ps * ps
    kpad, rows = (K + 7) & ~7, N * (S // ps) ** 2
    a = U.content("random", h, w, seed=offset, n=N)
    want_u8, want_rows = U.reference(list(a), S, ps, "floor", geom)
    wb, ldo, sb = w + 5, kpad + 24, S + 4
    for with_u8 in (True, False):
        xflat = torch.full((offset + N * (h + 2) * wb * 3,), 0x5A, dtype=torch.uint8, device=gpu)
        xbuf = xflat[offset:].view(N, h + 2, wb, 3)
        xbuf[:, 1:1 + h, 2:2 + w] = torch.from_numpy(a).to(gpu)
        xin = xbuf[:, 1:1 + h, 2:2 + w]
        oflat = _pattern(offset + (rows + 2) * ldo, gpu)
        uflat = (torch.arange(offset + N * (S + 2) * sb * 3, device=gpu) * 7 % 251).to(torch.uint8)
        o0, u0 = oflat.clone(), uflat.clone()
        out = oflat[offset:].view(rows + 2, ldo)[1:1 + rows, 8:8 + kpad]
        uout = uflat[offset:].view(N, S + 2, sb, 3)[:, 1:1 + S, 3:3 + S]
        assert not xin.is_contiguous() and out.stride(0) == ldo
        ops.clip_patchify_u8(xin, out, S, ps, U.CLIP_MEAN, U.CLIP_STD, geometry=geom, crop="floor", out_u8=uout if with_u8 else None)
        o0[offset:].view(rows + 2, ldo)[1:1 + rows, 8:8 + kpad] = torch.from_numpy(want_rows).to(gpu)
        if with_u8:
            u0[offset:].view(N, S + 2, sb, 3)[:, 1:1 + S, 3:3 + S] = torch.from_numpy(want_u8).to(gpu)
        assert torch.equal(oflat.view(I16), o0.view(I16)), f"u8={with_u8}: patch rows or the elements around their window"
        assert torch.equal(uflat, u0), f"u8={with_u8}: uint8 window or its guard elements"


def test_ops_rejections(gpu):
    from storygen_amd import ops
    from test_clip_u8_host import test_clip_patchify_u8_rejects_on_the_host
    test_clip_patchify_u8_rejects_on_the_host()
    x = torch.zeros(1, 50, 70, 3, dtype=torch.uint8, device=gpu)
    out = torch.zeros(4, 592, dtype=F16, device=gpu)
    M, Sd = U.CLIP_MEAN, U.CLIP_STD
    with pytest.raises(TypeError):
        ops.clip_patchify_u8(x, out.float(), 28, 14, M, Sd)
    with pytest.raises(ValueError, match=r"\[N,h,w,3\]"):
        ops.clip_patchify_u8(x[..., :1], out, 28, 14, M, Sd)
    with pytest.raises(ValueError, match="multiple of patch size"):
        ops.clip_patchify_u8(x, out, 30, 14, M, Sd)
    with pytest.raises(ValueError, match="out must be"):
        ops.clip_patchify_u8(x, out[:3], 28, 14, M, Sd)
    with pytest.raises(ValueError, match="out must be"):
        ops.clip_patchify_u8(x, out[:, :584], 28, 14, M, Sd)
    with pytest.raises(ValueError, match="out_u8 must be"):
        ops.clip_patchify_u8(x, out, 28, 14, M, Sd, out_u8=torch.zeros(1, 28, 29, 3, dtype=torch.uint8, device=gpu))
    with pytest.raises(ValueError, match="contiguous pixels"):
        ops.clip_patchify_u8(x.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3), out, 28, 14, M, Sd)
    with pytest.raises(ValueError, match="crop must be"):
        ops.clip_patchify_u8(x, out, 28, 14, M, Sd, crop="center")
    with pytest.raises(RuntimeError, match="crop window"):
        ops.clip_patchify_u8(x, out, 28, 14, M, Sd, geometry=(28, 39, 0, 12))
    with pytest.raises(RuntimeError, match="zero std"):
        ops.clip_patchify_u8(x, out, 28, 14, M, (0.5, 0.0, 0.5))
    with pytest.raises(RuntimeError, match="in / out <= 32"):
        ops.clip_patchify_u8(torch.zeros(1, 40, 1000, 3, dtype=torch.uint8, device=gpu), out, 28, 14, M, Sd, geometry=(28, 28, 0, 0))
    assert not out.any()


# ------------------------------------------------------------------------------------------------------ through the layers
def _mixed_frames(S):
    """Five frames of three sizes, interleaved; the second size has resized size - S = 7 (3 mod 4) on its long axis."""
    big = (2 * S, 2 * S + 14) if S < 100 else (140, 148)
    sizes = [(S + 20, S + 40), big, (S + 20, S + 40), big[::-1], (S + 20, S + 40)]
    return [U.content("random" if i != 2 else "checker", h, w, seed=i) for i, (h, w) in enumerate(sizes)]


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_engine_on_uint8_frames_equals_encode_pixels_of_the_reference(gpu, wide):
    """engine(8-bit frames) == engine.encode_pixels(the restatement's pixel_values), bit for bit, for the attention path of the ViT-B/32
    class (17 tokens, head dim 32) and for wide=True (82 tokens, head dim 80, patch rows 588 -> 592); lists of mixed sizes, PIL images,
    one uint8 tensor on either device."""
    from PIL import Image
    from storygen_amd.encoders import ClipVisionEngine
    if wide:
        cfg = P.tiny_config()
        eng, S = ClipVisionEngine(P.tiny_state(2, cfg), gpu, heads=2, hidden_act="gelu", wide=True), 126
    else:
        from tests.test_clip_score_host import tiny_states
        eng, S = ClipVisionEngine(tiny_states(seed=7)[0], gpu, heads=2), 32
    frames = _mixed_frames(S)
    for crop in U.CROPS:
        want_e, want_h = eng.encode_pixels(U.pixel_values(frames, S, crop))
        mixed = [frames[0], Image.fromarray(frames[1]), torch.from_numpy(frames[2]).to(gpu), frames[3], frames[4]]
        e, h = eng(mixed, crop=crop)
        assert e.dtype == torch.float32 and tuple(e.shape) == (5, 32) and bool(torch.isfinite(e).all())
        assert torch.equal(e, want_e) and torch.equal(h, want_h)
    assert not torch.equal(eng(frames, crop="floor")[0][1], eng(frames, crop="torchvision")[0][1])
    same = np.stack([frames[0], frames[2], frames[4]])
    want = eng.encode_pixels(U.pixel_values(same, S, "torchvision"))[0]
    for form in (same, torch.from_numpy(same), torch.from_numpy(same).to(gpu)):
        assert torch.equal(eng(form)[0], want)


def test_scorers_on_uint8_frames_equal_the_reference_pixel_values(gpu):
    from storygen_amd.clip_score import ClipScorer
    from storygen_amd.pick_score import PickScorer
    from tests.test_clip_score_host import tiny_states
    cfg = P.tiny_config()
    pick = PickScorer(P.tiny_state(2, cfg), cfg, device=gpu)
    _, ids = P.tiny_inputs(13)
    frames = _mixed_frames(126)
    idx, probs = pick.best_of(ids, frames)
    want = torch.softmax(pick._scores(pick.text_features(ids), pick.pixel_features(U.pixel_values(frames, 126, "floor"))), -1)[0]
    assert torch.equal(probs, want) and idx == int(want.argmax()) and abs(float(probs.sum()) - 1) < 1e-5
    other = torch.softmax(pick._scores(pick.text_features(ids), pick.pixel_features(U.pixel_values(frames, 126, "torchvision"))), -1)[0]
    assert not torch.equal(probs, other)                                          # the scorer's default is the processor's crop
    vsd, tsd = tiny_states(seed=5)
    vcfg, tcfg = dict(hidden_size=64, num_attention_heads=2, image_size=32, patch_size=8), dict(hidden_size=64, num_attention_heads=2)
    clip = ClipScorer({**vsd, **tsd}, vcfg, {**vsd, **tsd}, tcfg, device=gpu)
    small, ids5 = _mixed_frames(32), torch.randint(0, 95, (5, 77), generator=torch.Generator().manual_seed(9))
    ids5[:, 20] = 95
    feats = clip.vision.encode_pixels(U.pixel_values(small, 32, "torchvision"))[0]
    ci, ct = clip.clip_i(small, small[::-1]), clip.clip_t(small, ids5)
    assert torch.equal(ci, clip.cosine(feats, feats.flip(0))) and torch.equal(ct, clip.cosine(feats, clip.text_features(ids5)))
    assert bool(torch.isfinite(ci).all()) and float(ci[2]) == pytest.approx(1.0, abs=1e-6)


def test_story_scores_uint8_frames_when_asked(gpu, rig):  # noqa: F811
    """3 frames x 3 samples.  score_uint8=True: the kept sample is the argmax of the scorer's probabilities on the restatement's
    pixel_values of the saved frames, and those probabilities are the ones returned.  score_uint8=False: the scorer sees uint8 / 255 as
    float, as before."""
    from storygen_amd.pick_score import PickScorer
    from storygen_amd.story import StoryGenerator
    pipe = _pipeline(rig)
    cfg = P.tiny_config()
    scorer = PickScorer(P.tiny_state(2, cfg), cfg, device=gpu)
    ids = {p: P.tiny_inputs(20 + i)[1] for i, p in enumerate(PROMPTS)}
    tok = lambda prompt, **kw: SimpleNamespace(input_ids=ids[prompt])      # noqa: E731
    decoded = []
    real = pipe._decode_device
    pipe._decode_device = lambda lat: decoded.append(real(lat)) or decoded[-1]
    for flag in (True, False):
        del decoded[:]
        torch.manual_seed(3)
        out = StoryGenerator(pipe, scorer, tok).generate(PROMPTS[1:4], context_frames=2, samples_per_frame=3, num_inference_steps=3, height=SIZE,
                                                         width=SIZE, generator=[torch.Generator(device=gpu).manual_seed(s) for s in (11, 12, 13)],
                                                         output_type="uint8", score_uint8=flag)
        assert len(decoded) == 3
        for j, (u8, _) in enumerate(decoded):
            t = scorer.text_features(ids[PROMPTS[1 + j]])
            if flag:
                i = scorer.pixel_features(U.pixel_values(u8.cpu().numpy(), 126, "floor"))
            else:
                i = scorer.image_features(u8.permute(0, 3, 1, 2).float() / 255.0)
            want = torch.softmax(scorer._scores(t, i), -1)[0].cpu()
            print(f"score_uint8={flag} frame {j}: probabilities {out.scores[j]} kept {out.chosen[j]}")
            assert out.scores[j] == want.tolist() and out.chosen[j] == int(np.argmax(want.numpy()))
            assert np.array_equal(out.frames[j], u8[out.chosen[j]].cpu().numpy())
