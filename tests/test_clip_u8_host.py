"""Scoring 8-bit frames, on the host (no GPU): the restatement of tests/clip_u8_reference.py pinned to transformers' PIL image processor
and to the NumPy restatement of Pillow's resize, the crop geometry under both rules, the host-side rejections of sg_clip_patchify_u8, and the
uint8 dispatch of ClipVisionEngine, ClipScorer, PickScorer and StoryGenerator over the emulated op of tests/clip_u8_ops_emulation.py."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import clip_u8_reference as U
from tests import image_reference as IR
from tests import pick_score_reference as P
from tests.clip_u8_ops_emulation import patched_u8_ops

# height x width of the source, crop size: size - S = 0, 1, 2, 3 (mod 4) on the long axis, either axis long, up- and downscaled
SOURCES = [((50, 70), 28), ((90, 33), 28), ((28, 28), 28), ((28, 31), 28), ((33, 28), 28), ((13, 20), 32), ((227, 224), 224), ((256, 300), 224)]


# ------------------------------------------------------------------------------------------------- the restatement is the reference's
@pytest.mark.parametrize("kind", ["random", "checker", "white"])
@pytest.mark.parametrize("source", SOURCES, ids=lambda s: "%dx%d_to%d" % (s[0][1], s[0][0], s[1]))
def test_restatement_equals_transformers_pil_processor(source, kind):
    """pixel_values of CLIPImageProcessorPil (shortest-edge resize with resample = 3, centre crop, rescale, normalise) against the
    restatement with the "floor" crop: equal after the fp16 rounding; in fp32 within 1e-6 absolute, which covers a build that rescales by
    * (1 / 255) instead of / 255 (two relative roundings of 2^-24 on values <= 1, divided by std >= 0.26)."""
    transformers = pytest.importorskip("transformers")
    if not hasattr(transformers, "CLIPImageProcessorPil"):
        pytest.skip("this transformers has no CLIPImageProcessorPil")
    from PIL import Image
    (h, w), S = source
    a = U.content(kind, h, w, seed=3)
    proc = transformers.CLIPImageProcessorPil(size={"shortest_edge": S}, crop_size={"height": S, "width": S})
    want = proc(images=[Image.fromarray(a)], return_tensors="np")["pixel_values"]
    u8, got = U.preprocess([a], S, "floor")
    assert want.dtype == np.float32 and want.shape == got.shape == (1, 3, S, S)
    err = float(np.abs(got - want).max())
    print(f"{kind} {w}x{h} -> {S}: max |restatement - CLIPImageProcessorPil| = {err:.3e}")
    assert err <= 1e-6
    assert np.array_equal(got.astype(np.float16).view(np.int16), want.astype(np.float16).view(np.int16))


@pytest.mark.parametrize("source", SOURCES[:6], ids=lambda s: "%dx%d_to%d" % (s[0][1], s[0][0], s[1]))
def test_restatement_resize_equals_the_numpy_restatement_of_pillow(source):
    """PIL's BICUBIC is the default filter tests/image_reference.py restates (and the kernel's tables implement), clip included."""
    (h, w), S = source
    for kind in ("random", "checker"):
        a = U.content(kind, h, w, seed=1)
        for crop in U.CROPS:
            Hr, Wr, top, left = U.geometry(h, w, S, crop)
            assert np.array_equal(U.resize_crop(a, (Hr, Wr, top, left), S), IR.resize_reference(a, (Wr, Hr))[top:top + S, left:left + S])


def test_checker_content_reaches_both_clips_and_ramp_every_byte():
    a = U.content("checker", 50, 70).astype(np.int64)
    coef, bounds = IR.table(70, 39)
    ss = np.array([(1 << 21) + (a[:, b[0]:b[0] + b[1]] * k[:b[1], None]).sum(1) for k, b in zip(coef.astype(np.int64), bounds)])
    assert (ss >> 22).min() < 0 and (ss >> 22).max() > 255
    r = U.content("ramp", 32, 40, n=2)
    assert all(set(r[i, :, :, c].flatten().tolist()) == set(range(256)) for i in range(2) for c in range(3))
    px = U.normalise(r)
    assert len({(c, v) for c in range(3) for v in px[:, c].flatten().tolist()}) == 768


def test_patch_rows_layout():
    px = np.arange(2 * 3 * 28 * 28, dtype=np.float32).reshape(2, 3, 28, 28) % 2039
    rows = U.patch_rows(px, 14)
    assert rows.shape == (8, 592) and rows.dtype == np.float16 and not rows[:, 588:].any()
    for n, y, x, c in ((0, 0, 0, 0), (1, 13, 14, 2), (1, 27, 27, 1), (0, 14, 13, 0)):
        assert rows[n * 4 + (y // 14) * 2 + x // 14, c * 196 + (y % 14) * 14 + x % 14] == np.float16(px[n, c, y, x])
    from tests.clip_vision_reference import patch_rows
    assert np.array_equal(rows[:, :588], patch_rows(torch.from_numpy(px), 14).numpy().astype(np.float16))


# ------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("S", [28, 224])
def test_crop_geometry_under_both_rules(S):
    """size - S = 0 .. 7 on either axis (every residue mod 4 twice): "torchvision" is int(round((size - S) / 2.0)) with halves to the even
    integer and what sg_clip_resize_geometry gives, "floor" is (size - S) // 2; they differ exactly where size - S = 3 (mod 4)."""
    from storygen_amd import ops
    seen = set()
    for d in range(8):
        for tall in (False, True):
            # the short side is S already, so the resize keeps the size: int(S * (S + d) / S) == S + d
            h, w = (S + d, S) if tall else (S, S + d)
            tv, fl = ops.clip_u8_geometry(h, w, S, "torchvision"), ops.clip_u8_geometry(h, w, S, "floor")
            assert tv == U.geometry(h, w, S, "torchvision") == ops.clip_resize_geometry(h, w, S)
            assert fl == U.geometry(h, w, S, "floor")
            assert tv[:2] == fl[:2] == (h, w)
            off_tv, off_fl = (tv[2], fl[2]) if tall else (tv[3], fl[3])
            assert off_fl == d // 2 and off_tv == int(round(d / 2.0))
            assert ((tv[3], fl[3]) if tall else (tv[2], fl[2])) == (0, 0)
            assert (off_tv != off_fl) == (d % 4 == 3) and off_tv - off_fl in (0, 1)
            seen.add((d % 4, tall))
    assert len(seen) == 8
    # a 224 x 227 (width x height) image: transformers crops from row 1, torchvision's formula from row 2
    assert ops.clip_u8_geometry(227, 224, 224, "floor") == (227, 224, 1, 0) and ops.clip_u8_geometry(227, 224, 224, "torchvision") == (227, 224, 2, 0)
    # resized sizes: both rules resize alike
    for h, w in ((50, 70), (90, 33), (13, 20), (1000, 1000), (300, 517), (375, 500)):
        for crop in U.CROPS:
            assert ops.clip_u8_geometry(h, w, S, crop) == U.geometry(h, w, S, crop)
    with pytest.raises(ValueError, match="crop must be"):
        ops.clip_u8_geometry(50, 70, 28, "center")


# ------------------------------------------------------------------------------------------------- the entry point's host checks
def test_clip_patchify_u8_rejects_on_the_host():
    """sg_clip_patchify_u8 validates before it launches: these return SG_EINVAL without a device (fake pointers)."""
    from storygen_amd import _lib, ops
    lib = _lib.load()
    X, O, U8, T = 0x100000, 0x200000, 0x300000, 0x400000
    m, z = (C.c_float * 3)(0.5, 0.4, 0.3), (C.c_float * 3)(0.5, 0.0, 0.5)

    def call(x=X, out=O, u8=U8, mean=m, std=m, N=1, Hin=50, Win=70, Hr=28, Wr=39, top=0, left=5, S=28, ps=14, Kpad=592, ldo=592, sx=None,
             su=None, h=(T, T + 0x1000), v=(T + 0x2000, T + 0x3000)):
        sx = sx or (Hin * Win * 3, Win * 3)
        su = su or (S * S * 3, S * 3)
        return lib.sg_clip_patchify_u8(x, *sx, N, Hin, Win, Hr, Wr, top, left, mean, std, S, ps, Kpad, out, ldo, u8, *su, *h, *v, None)
    none = (None, None)
    for kw, msg in ((dict(x=None), b"null"), (dict(out=None), b"null"), (dict(mean=None), b"null"), (dict(std=None), b"null"),
                    (dict(N=0), b"N = 0"), (dict(N=65536), b"N = 65536"), (dict(Hin=0), b"sizes must be positive"),
                    (dict(Win=-1), b"sizes must be positive"), (dict(Hr=0), b"sizes must be positive"), (dict(Wr=0), b"sizes must be positive"),
                    (dict(Win=16385), b"above 16384"), (dict(Hr=16385), b"above 16384"),
                    (dict(Win=39 * 32 + 1), b"more than 32"), (dict(Hin=28 * 32 + 1), b"more than 32"),
                    (dict(S=0), b"bad crop size"), (dict(ps=0), b"bad crop size"), (dict(ps=-14), b"bad crop size"),
                    (dict(S=27, ps=14), b"multiple of the patch size"), (dict(ps=8, Kpad=192, ldo=192), b"multiple of the patch size"),
                    (dict(Kpad=588), b"Kpad"), (dict(Kpad=590, ldo=600), b"Kpad"), (dict(Kpad=584), b"Kpad"), (dict(Kpad=0), b"Kpad"),
                    (dict(Kpad=600), b"below Kpad"), (dict(ldo=591), b"below Kpad"),
                    (dict(top=1), b"crop window"), (dict(left=12), b"crop window"), (dict(top=-1), b"crop window"), (dict(left=-1), b"crop window"),
                    (dict(Hr=27), b"crop window"), (dict(Wr=32), b"crop window"),
                    (dict(std=z), b"zero std"),
                    (dict(sx=(50 * 210, 209)), b"input strides"), (dict(N=2, sx=(50 * 210 - 1, 210)), b"input strides"),
                    (dict(su=(28 * 84, 83)), b"uint8 output strides"), (dict(N=2, su=(28 * 84 - 1, 84)), b"uint8 output strides"),
                    (dict(u8=O + 100), b"outputs overlap"), (dict(out=U8 + 2), b"outputs overlap"), (dict(out=X + 4), b"overlaps the input"),
                    (dict(u8=X + 10), b"overlaps the input"), (dict(u8=None, out=X + 50 * 210 - 2), b"overlaps the input"),
                    (dict(h=none), b"horizontal tables are missing"), (dict(h=(T, None)), b"horizontal tables are missing"),
                    (dict(v=none), b"vertical tables are missing"), (dict(v=(None, T)), b"vertical tables are missing"),
                    (dict(Win=39), b"horizontal tables are given"), (dict(Hin=28), b"vertical tables are given"),
                    (dict(Win=39, h=(None, T)), b"horizontal tables are given"), (dict(Hin=28, Win=39, h=none), b"vertical tables are given")):
        assert call(**kw) == -1, kw
        assert msg in lib.sg_last_error(), (kw, lib.sg_last_error())
    # ops refuses what is not on the device or not uint8, like every other op
    x, out = torch.zeros(1, 50, 70, 3, dtype=torch.uint8), torch.zeros(4, 592, dtype=torch.float16)
    with pytest.raises(TypeError, match="CUDA/HIP uint8"):
        ops.clip_patchify_u8(x, out, 28, 14, U.CLIP_MEAN, U.CLIP_STD)
    with pytest.raises(TypeError, match="CUDA/HIP uint8"):
        ops.clip_patchify_u8(x.float(), out, 28, 14, U.CLIP_MEAN, U.CLIP_STD)


# ------------------------------------------------------------------------------------------------- dispatch of engines and scorers
def _frames():
    """Five frames of three sizes, interleaved; 140 x 148 becomes 126 x 133 at S = 126: size - S = 7 = 3 (mod 4), where the crop rules differ."""
    sizes = [(150, 170), (148, 140), (150, 170), (140, 148), (150, 170)]
    return [U.content("random", h, w, seed=i) for i, (h, w) in enumerate(sizes)]


def test_vision_engine_dispatches_on_dtype_and_groups_sizes():
    from PIL import Image
    from storygen_amd.encoders import ClipVisionEngine, is_uint8_images
    cfg = P.tiny_config()
    sd = P.tiny_state(2, cfg)
    frames = _frames()
    S = 126
    with patched_u8_ops() as (u8_calls, calls):
        eng = ClipVisionEngine(sd, "cpu", heads=2, hidden_act="gelu", wide=True)
        for crop in U.CROPS:
            del u8_calls[:]
            mixed = [frames[0], Image.fromarray(frames[1]), torch.from_numpy(frames[2]), frames[3], Image.fromarray(frames[4])]
            e, h = eng(mixed, crop=crop)
            # one launch per size, first appearance first, with that size's geometry under the rule asked for
            assert u8_calls == [((3, 150, 170, 3), U.geometry(150, 170, S, crop), 592), ((1, 148, 140, 3), U.geometry(148, 140, S, crop), 592),
                                ((1, 140, 148, 3), U.geometry(140, 148, S, crop), 592)]
            want_e, want_h = eng.encode_pixels(U.pixel_values(frames, S, crop))
            assert tuple(e.shape) == (5, 32) and torch.equal(e, want_e) and torch.equal(h, want_h)           # order kept
        assert U.geometry(148, 140, S, "floor") != U.geometry(148, 140, S, "torchvision")
        # a [N,h,w,3] array or tensor: one launch, in_scale / in_shift not applied
        same = np.stack([frames[0], frames[2], frames[4]])
        want = eng.encode_pixels(U.pixel_values(same, S, "torchvision"))[0]
        for form in (same, torch.from_numpy(same), list(same)):
            del u8_calls[:], calls[:]
            assert torch.equal(eng(form, in_scale=0.5, in_shift=0.5)[0], want)
            assert len(u8_calls) == 1 and u8_calls[0][0] == (3, 150, 170, 3)
            assert not [c for c in calls if c[0].startswith("clip_patchify")]
        # float input keeps the float path
        del u8_calls[:], calls[:]
        eng(torch.rand(1, 3, 150, 170))
        assert u8_calls == [] and ("clip_patchify_padk", 588, 592) in calls
        for bad in (same[..., :2], np.zeros((0, 8, 8, 3), np.uint8), [frames[0][..., :1]], [Image.new("RGBA", (8, 8))], [Image.new("L", (8, 8))],
                    torch.zeros(8, 8, 3, dtype=torch.uint8)):
            with pytest.raises(ValueError):
                eng(bad)
        with pytest.raises(ValueError, match="crop must be"):
            eng(same, crop="center")
    assert is_uint8_images(same) and is_uint8_images([Image.new("RGB", (4, 4))]) and is_uint8_images((torch.zeros(4, 4, 3, dtype=torch.uint8),))
    assert not is_uint8_images(same.astype(np.float32)) and not is_uint8_images(torch.zeros(1, 3, 4, 4)) and not is_uint8_images([])


def test_scorers_default_crop_and_dtype_dispatch():
    from storygen_amd.clip_score import ClipScorer
    from storygen_amd.pick_score import PickScorer
    from tests.test_clip_score_host import tiny_states
    cfg = P.tiny_config()
    sd = P.tiny_state(2, cfg)
    _, ids = P.tiny_inputs(13)
    frames = _frames()
    vsd, tsd = tiny_states(seed=5)
    vcfg, tcfg = dict(hidden_size=64, num_attention_heads=2, image_size=32, patch_size=8), dict(hidden_size=64, num_attention_heads=2)
    ids3 = torch.randint(0, 95, (5, 77), generator=torch.Generator().manual_seed(9))
    ids3[:, 20] = 95
    with patched_u8_ops() as (u8_calls, calls):
        pick = PickScorer(sd, cfg, device="cpu", in_scale=0.5, in_shift=0.5)
        assert pick.crop == "floor"
        idx, probs = pick.best_of(ids, frames)
        assert [c[1] for c in u8_calls] == [U.geometry(h, w, 126, "floor") for h, w in ((150, 170), (148, 140), (140, 148))]
        px = U.pixel_values(frames, 126, "floor")
        want = torch.softmax(pick._scores(pick.text_features(ids), pick.pixel_features(px)), -1)[0]
        assert torch.equal(probs, want) and idx == int(want.argmax())
        tv = PickScorer(sd, cfg, device="cpu", crop="torchvision")
        assert torch.equal(tv.image_features(frames), tv.pixel_features(U.pixel_values(frames, 126, "torchvision")))
        assert not torch.equal(tv.image_features(frames), pick.image_features(frames))          # 140 x 148: the rules differ by a pixel
        # float frames: today's path, in_scale / in_shift applied, no uint8 launch
        del u8_calls[:], calls[:]
        f = torch.rand(2, 3, 150, 170)
        assert torch.equal(pick.image_features(f * 2 - 1), pick.vision(f * 2 - 1, 0.5, 0.5)[0])
        assert u8_calls == [] and ("clip_patchify_padk", 588, 592) in calls
        with pytest.raises(ValueError, match="crop must be"):
            PickScorer(sd, cfg, device="cpu", crop="round")

        clip = ClipScorer({**vsd, **tsd}, vcfg, {**vsd, **tsd}, tcfg, device="cpu")
        assert clip.crop == "torchvision"
        small = [U.content("random", h, w, seed=i) for i, (h, w) in enumerate([(40, 56), (39, 32), (40, 56), (32, 39), (40, 56)])]
        del u8_calls[:]
        ci, ct = clip.clip_i(small, small[::-1]), clip.clip_t(small, ids3)
        assert [c[1] for c in u8_calls[:3]] == [U.geometry(h, w, 32, "torchvision") for h, w in ((40, 56), (39, 32), (32, 39))]
        assert all(c[2] == 192 for c in u8_calls) and len(u8_calls) == 9
        feats = clip.vision.encode_pixels(U.pixel_values(small, 32, "torchvision"))[0]
        assert torch.equal(ci, clip.cosine(feats, feats.flip(0))) and torch.equal(ct, clip.cosine(feats, clip.text_features(ids3)))
        fl = ClipScorer(vsd, vcfg, device="cpu", crop="floor")
        assert torch.equal(fl.image_features(small), fl.vision.encode_pixels(U.pixel_values(small, 32, "floor"))[0])
        assert not torch.equal(fl.image_features(small), clip.image_features(small))
        with pytest.raises(ValueError, match="crop must be"):
            ClipScorer(vsd, vcfg, device="cpu", crop="round")


def test_story_generator_hands_uint8_frames_to_the_scorer_only_when_asked():
    from test_story_host import FakePipeline, H, W
    from storygen_amd.story import StoryGenerator

    class Scorer:
        def __init__(self):
            self.seen = []

        def best_of(self, ids, images):
            self.seen.append(images)
            p = torch.softmax(images.float().mean(dim=(1, 2, 3)) * (100.0 if images.dtype == torch.uint8 else 25500.0), 0)
            return int(p.argmax()), p

    tok = lambda prompt, **kw: SimpleNamespace(input_ids=torch.zeros(1, 4, dtype=torch.long))      # noqa: E731
    runs = {}
    for flag in (False, True, None):
        pipe, sc = FakePipeline(), Scorer()
        kw = {} if flag is None else dict(score_uint8=flag)
        out = StoryGenerator(pipe, sc, tok).generate(["a", "b"], samples_per_frame=3, height=H, width=W, num_inference_steps=3, output_type="uint8", **kw)
        runs[flag] = (out, sc.seen, pipe.decoded)
    for flag, (out, seen, decoded) in runs.items():
        assert len(seen) == 2
        for images, (u8, _) in zip(seen, decoded):
            if flag:
                assert images is u8 and images.dtype == torch.uint8 and tuple(images.shape) == (3, H, W, 3)
            else:
                assert images.dtype == torch.float32 and torch.equal(images, u8.permute(0, 3, 1, 2).float() / 255.0)
    assert runs[None][0].chosen == runs[False][0].chosen and np.array_equal(runs[None][0].frames, runs[False][0].frames)
