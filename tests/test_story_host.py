"""Story generation on the host (no GPU): the NumPy restatement of the frame hand-off pinned to the pipeline's own chain, the context
schedule, first frames, the selection rule, the pipeline's sampler cache and the rejected arguments.  The pipeline stand-in records
every call and decodes through tests/story_reference.handoff_reference, so what is checked is the loop of storygen_amd/story.py."""
import ctypes as C
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import story_reference as SR

H = W = 16


# ------------------------------------------------------------------------------------------------- the restatement is the host chain
def test_handoff_restatement_equals_decode_latents_numpy_to_pil_and_reload_on_every_fp16_pattern():
    from storygen_amd.model import StableDiffusionPipeline
    x, n = SR.as_image(SR.all_fp16_patterns())
    assert n == 65536
    vae = SimpleNamespace(config=None, decode=lambda z: SimpleNamespace(sample=x.clone()))
    pipe = StableDiffusionPipeline(vae=vae, text_encoder=None, tokenizer=None, unet=None, scheduler=None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # numpy: NaN -> uint8 is an invalid cast (those patterns are compared below)
        pil = pipe.numpy_to_pil(pipe.decode_latents(torch.zeros(1, 4, 2, 2)))
    want_u8 = torch.from_numpy(np.asarray(pil[0]).copy())[None]                                   # [1,S,S,3]
    want_f16 = (torch.from_numpy(np.asarray(pil[0]).copy()) / 255).permute(2, 0, 1).half()[None]  # inference.py:86-92, then the pipeline's cast
    got_u8, got_f16 = SR.handoff_reference(x)
    nan = torch.isnan(x)
    assert int(nan.sum()) == SR.NAN_PATTERNS
    nan_hwc = nan.permute(0, 2, 3, 1)
    assert torch.equal(got_u8[~nan_hwc], want_u8[~nan_hwc])
    assert torch.equal(got_f16[~nan].view(torch.int16), want_f16[~nan].view(torch.int16))
    assert int(got_u8[nan_hwc].max()) == 0 and int(got_f16[nan].view(torch.int16).abs().max()) == 0      # the documented value
    assert set(got_u8.flatten().tolist()) == set(range(256))                                      # every byte, hence every reload value
    # +-inf clamp like any large value
    inf = torch.tensor([float("inf"), float("-inf"), 65504.0, -65504.0], dtype=torch.float16)
    u, y = SR.handoff_reference(torch.cat([inf, torch.zeros(8, dtype=torch.float16)]).view(1, 3, 2, 2))
    assert u.permute(0, 3, 1, 2).flatten()[:4].tolist() == [255, 0, 255, 0] and y.flatten()[:4].tolist() == [1.0, 0.0, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------- a recording pipeline stand-in
class FakePipeline:
    """Records every call; call i, sample s decodes to a frame that depends on i, s and the mean of the context it was given."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls, self.decoded = [], []

    def __call__(self, **kw):
        self.calls.append(kw)
        S = kw["num_images_per_prompt"]
        ctx = float(kw["image_prompt"].float().mean())
        lat = torch.tensor([len(self.calls) * 0.37 + s * 0.11 + ctx for s in range(S)]).view(S, 1, 1, 1).expand(S, 4, H // 8, W // 8)
        return SimpleNamespace(images=lat.clone())

    def _decode_device(self, latents):
        S = latents.shape[0]
        ramp = torch.linspace(-1.2, 1.2, 3 * H * W).view(1, 3, H, W)
        x = (torch.sin(latents[:, :1, :1, :1] * 5.0) * 0.5 + ramp).half()
        assert tuple(x.shape) == (S, 3, H, W)
        out = SR.handoff_reference(x)
        self.decoded.append(out)
        return out


def _story(prompts, **kw):
    from storygen_amd.story import StoryGenerator
    pipe = FakePipeline()
    gen = StoryGenerator(pipe, kw.pop("scorer", None), kw.pop("tokenizer", None))
    out = gen.generate(prompts, height=H, width=W, num_inference_steps=3, **kw)
    return pipe, gen, out


@pytest.mark.parametrize("context_frames", [1, 2, 3])
@pytest.mark.parametrize("n_frames", [1, 2, 5])
def test_context_schedule(context_frames, n_frames):
    from storygen_amd.story import context_schedule
    prompts = [f"p{j}" for j in range(n_frames)]
    pipe, gen, out = _story(prompts, context_frames=context_frames, output_type="uint8")
    assert len(pipe.calls) == n_frames and out.chosen == [0] * n_frames and out.scores == [None] * n_frames
    assert out.frames.dtype == np.uint8 and out.frames.shape == (n_frames, H, W, 3)
    for j, kw in enumerate(pipe.calls):
        want = list(range(max(0, j - context_frames), j))                                  # the last min(j, context_frames), oldest first
        assert context_schedule(n_frames, context_frames)[j] == want
        assert kw["prompt"] == prompts[j] and kw["output_type"] == "latent" and kw["num_images_per_prompt"] == 1
        assert (kw["height"], kw["width"], kw["num_inference_steps"], kw["guidance_scale"], kw["image_guidance_scale"], kw["eta"]) == \
            (H, W, 3, 7.0, 3.5, 0.0)
        ip = kw["image_prompt"]
        assert ip.dtype == torch.float16
        if not want:      # no prior frame: the text-only stage, on the one zero frame and prompt the call shape still needs
            assert kw["stage"] == "no" and tuple(ip.shape) == (1, 1, 3, H, W) and not ip.any() and kw["prev_prompt"] == [prompts[j]]
        else:
            assert kw["stage"] == "auto-regressive" and tuple(ip.shape) == (1, len(want), 3, H, W)
            assert kw["prev_prompt"] == [prompts[i] for i in want]
            for slot, i in enumerate(want):
                assert torch.equal(ip[0, slot], pipe.decoded[i][1][0])                     # output (b) of frame i, untouched
        assert np.array_equal(out.frames[j], pipe.decoded[j][0][0].numpy())                # output (a) of frame j
    kept = list(range(max(0, n_frames - context_frames), n_frames))
    assert gen.context_prompts == [prompts[i] for i in kept]
    assert all(torch.equal(f, pipe.decoded[i][1][0]) for f, i in zip(gen.context, kept))


def test_output_types_and_stage_passthrough():
    pipe, _, pil = _story(["a", "b"], output_type="pil", stage="multi-image-condition")
    assert pipe.calls[0]["stage"] == "no" and pipe.calls[1]["stage"] == "multi-image-condition"
    _, _, u8 = _story(["a", "b"], output_type="uint8")
    _, _, f32 = _story(["a", "b"], output_type="np")
    assert [np.asarray(im).shape for im in pil.frames] == [(H, W, 3)] * 2
    assert all(np.array_equal(np.asarray(im), f) for im, f in zip(pil.frames, u8.frames))
    assert f32.frames.dtype == np.float32 and np.array_equal(f32.frames, u8.frames.astype(np.float32) / 255.0)


def test_first_frames_seed_the_context():
    first = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(0))
    pipe, gen, _ = _story(["g0", "g1", "g2"], context_frames=3, first_frames=first, first_prompts=["f0", "f1"])
    f16 = first.half()
    g = [d[1][0] for d in pipe.decoded]
    want = [([f16[0], f16[1]], ["f0", "f1"]), ([f16[0], f16[1], g[0]], ["f0", "f1", "g0"]), ([f16[1], g[0], g[1]], ["f1", "g0", "g1"])]
    for kw, (frames, prev) in zip(pipe.calls, want):
        assert kw["stage"] == "auto-regressive" and kw["prev_prompt"] == prev
        assert torch.equal(kw["image_prompt"], torch.stack(frames)[None])
    assert gen.context_prompts == ["g0", "g1", "g2"]
    # more first frames than the context holds: the last context_frames of them
    pipe, _, _ = _story(["g0"], context_frames=1, first_frames=first, first_prompts=["f0", "f1"])
    assert pipe.calls[0]["prev_prompt"] == ["f1"] and torch.equal(pipe.calls[0]["image_prompt"][0, 0], f16[1])


class StubScorer:
    def __init__(self, table):
        self.table, self.seen = table, []

    def best_of(self, input_ids, images):
        self.seen.append((input_ids, images))
        p = torch.tensor(self.table[len(self.seen) - 1])
        return 0, p                       # the index a scorer reports is not what decides: np.argmax of the probabilities is


def test_selection_keeps_the_argmax_and_only_it_becomes_context():
    table = [[0.2, 0.5, 0.3], [0.1, 0.45, 0.45], [0.6, 0.3, 0.1]]          # frame 1 is a tie: the first of equals, as np.argmax
    scorer = StubScorer(table)
    tok = lambda prompt, **kw: SimpleNamespace(input_ids=torch.tensor([[len(prompt)]]), kw=kw)      # noqa: E731
    gens = [torch.Generator().manual_seed(s) for s in range(3)]
    pipe, gen, out = _story(["one", "three", "eleven"], context_frames=2, samples_per_frame=3, scorer=scorer, tokenizer=tok, generator=gens,
                            output_type="uint8")
    assert out.chosen == [1, 1, 0] == [int(np.argmax(t)) for t in table]
    assert np.allclose(np.array(out.scores), np.array(table))
    for j, kw in enumerate(pipe.calls):
        assert kw["num_images_per_prompt"] == 3 and kw["generator"] == gens
        ids, images = scorer.seen[j]
        assert ids.tolist() == [[len(kw["prompt"])]]
        u8 = pipe.decoded[j][0]
        assert images.dtype == torch.float32 and torch.equal(images, u8.permute(0, 3, 1, 2).float() / 255.0)     # the uint8 frames
        assert np.array_equal(out.frames[j], u8[out.chosen[j]].numpy())
    assert torch.equal(pipe.calls[1]["image_prompt"][0, 0], pipe.decoded[0][1][1])
    assert torch.equal(pipe.calls[2]["image_prompt"][0], torch.stack([pipe.decoded[0][1][1], pipe.decoded[1][1][1]]))
    # without a scorer sample 0 is kept and nothing is scored
    _, _, plain = _story(["a", "b"], samples_per_frame=3)
    assert plain.chosen == [0, 0] and plain.scores == [None, None]


def test_rejected_arguments():
    from storygen_amd.story import StoryGenerator
    with pytest.raises(ValueError, match="tokenizer"):
        StoryGenerator(FakePipeline(), scorer=StubScorer([]))
    gen = StoryGenerator(FakePipeline())
    first = torch.rand(1, 3, H, W)
    for bad, match in ((dict(prompts=[]), "non-empty"), (dict(prompts="a prompt"), "non-empty"), (dict(prompts=["a"], context_frames=0), "context_frames"),
                       (dict(prompts=["a"], first_frames=first), "go together"), (dict(prompts=["a"], first_prompts=["f"]), "go together"),
                       (dict(prompts=["a"], first_frames=first, first_prompts=["f", "g"]), "first prompts"),
                       (dict(prompts=["a"], first_frames=first[:, :, :8], first_prompts=["f"]), "first_frames must be"),
                       (dict(prompts=["a"], samples_per_frame=0), "samples_per_frame"), (dict(prompts=["a"], output_type="latent"), "output_type"),
                       (dict(prompts=["a"], samples_per_frame=2, generator=[torch.Generator()]), "generators")):
        with pytest.raises(ValueError, match=match):
            gen.generate(height=H, width=W, **bad)
    assert gen.pipeline.calls == []


# ------------------------------------------------------------------------------------------------- the pipeline's sampler cache
class FakeSampler:
    built = 0

    def __init__(self, arch, sd, device, n, h, w, R, S, schedule=None, weights=None, ref_ahead=1):
        type(self).built += 1
        self.R, self.G, self.timesteps = R, ref_ahead, []
        self.latents = torch.zeros(n, 4, h, w)

    def prepare(self, inputs, steps, stage, *a, **k):
        self.stage = stage
        self.timesteps = list(range(steps))

    def step(self, i):
        pass

    def check_guards(self):
        pass


def _cpu_pipeline(monkeypatch):
    import storygen_amd.model.pipeline as PL
    from storygen_amd.scheduler import DDIMSchedule
    monkeypatch.setattr(PL, "StoryGenSampler", FakeSampler)
    FakeSampler.built = 0
    wts = object()
    unet = SimpleNamespace(device=torch.device("cpu"), in_channels=4, config=SimpleNamespace(sample_size=2), _arch=None,
                           _engine_weights=lambda: wts)
    tok = lambda prompts, **kw: SimpleNamespace(input_ids=torch.zeros(len(prompts), 7, dtype=torch.long),      # noqa: E731
                                                attention_mask=torch.ones(len(prompts), 7, dtype=torch.long))
    tok.model_max_length = 7
    text = lambda ids, attention_mask=None: (torch.zeros(ids.shape[0], 7, 8),)      # noqa: E731
    vae = SimpleNamespace(config=None, encode=lambda f: SimpleNamespace(latent_dist=SimpleNamespace(sample=lambda: torch.zeros(f.shape[0], 4, 2, 2))))
    pipe = PL.StableDiffusionPipeline(vae=vae, text_encoder=text, tokenizer=tok, unet=unet, scheduler=DDIMSchedule())
    pipe.set_progress_bar_config(disable=True)

    def call(R, stage="auto-regressive", steps=3):
        return pipe(stage=stage, prompt="p", image_prompt=torch.zeros(1, R, 3, 16, 16), prev_prompt=["q"] * R, height=16, width=16,
                    num_inference_steps=steps, output_type="latent")
    return pipe, call, PL


def test_sampler_cache_hits_evicts_the_oldest_of_five_and_repeats_give_the_same_object(monkeypatch):
    pipe, call, PL = _cpu_pipeline(monkeypatch)
    assert PL.SAMPLER_CACHE_ENTRIES == 4 and pipe._sampler is None
    call(1)
    first = pipe._sampler
    call(1)
    assert pipe._sampler is first and FakeSampler.built == 1                 # a single-call user: same key, same sampler object
    call(1, stage="no")                                                      # the text-only stage has an entry of its own
    no = pipe._sampler
    assert no is not first and no.stage == "no" and FakeSampler.built == 2
    seen = {1: first}
    for R in (2, 3):
        call(R)
        seen[R] = pipe._sampler
    assert FakeSampler.built == 4 and len(pipe._samplers) == 4
    for R in (3, 1, 2, 3, 3):                                                # a story's steady state and head again: hits only
        call(R)
        assert pipe._sampler is seen[R]
    call(1, stage="no")
    assert pipe._sampler is no and FakeSampler.built == 4
    call(4)                                                                  # a fifth key: the oldest entry (R = 1) goes
    assert FakeSampler.built == 5 and len(pipe._samplers) == 4 and first not in pipe._samplers.values()
    assert pipe._sampler.R == 4 and no in pipe._samplers.values() and seen[2] in pipe._samplers.values()
    call(1)                                                                  # ... and is rebuilt when asked for again
    assert FakeSampler.built == 6 and pipe._sampler is not first and pipe._sampler.R == 1
    call(5, steps=5)                                                         # G = 5 is part of the key as before
    assert pipe._sampler.G == 5 and FakeSampler.built == 7


def test_story_on_the_pipeline_builds_one_sampler_per_distinct_key(monkeypatch):
    """A 5-frame story at context_frames = 3 asks for R = 1 (stage "no"), 1, 2, 3, 3, 3: four keys, four samplers; a second story none."""
    from storygen_amd.story import StoryGenerator
    pipe, _, _ = _cpu_pipeline(monkeypatch)
    pipe._decode_device = lambda lat: SR.handoff_reference(torch.zeros(lat.shape[0], 3, 16, 16, dtype=torch.float16))
    gen = StoryGenerator(pipe)
    gen.generate(["a", "b", "c", "d", "e"], height=16, width=16, num_inference_steps=3, output_type="uint8")
    assert FakeSampler.built == 4 and [s.R for s in pipe._samplers.values()] == [1, 1, 2, 3]
    gen.generate(["a", "b", "c", "d", "e"], height=16, width=16, num_inference_steps=3, output_type="uint8")
    assert FakeSampler.built == 4


# ------------------------------------------------------------------------------------------------- the entry point's host checks
def test_frame_handoff_rejects_on_the_host():
    """sg_frame_handoff_f16 validates before it launches: these return SG_EINVAL without a device."""
    from storygen_amd import _lib
    lib = _lib.load()
    X, U, Y = 0x100000, 0x200000, 0x300000

    def call(x=X, u=U, y=Y, N=1, H=4, W=8, sx=None, su=None, sy=None):
        sx = sx or (3 * H * W, H * W, W)
        su = su or (3 * H * W, 3 * W)
        sy = sy or (3 * H * W, H * W, W)
        return lib.sg_frame_handoff_f16(x, *sx, u, *su, y, *sy, N, H, W, None)
    for kw, msg in ((dict(x=None), b"null"), (dict(u=None), b"null"), (dict(y=None), b"null"), (dict(N=0), b"N = 0"), (dict(N=-1), b"N = -1"),
                    (dict(H=0), b"H * W == 0"), (dict(W=0), b"H * W == 0"), (dict(u=Y + 10), b"outputs overlap"), (dict(y=U + 8), b"outputs overlap"),
                    (dict(y=X), b"overlaps the input"), (dict(u=X + 2), b"overlaps the input"), (dict(sx=(96, 32, 7)), b"input strides"),
                    (dict(sy=(96, 31, 8)), b"fp16 output strides"), (dict(su=(96, 23)), b"uint8 output strides"),
                    (dict(N=2, sy=(95, 32, 8)), b"fp16 output strides"), (dict(N=2, su=(95, 24)), b"uint8 output strides")):
        assert call(**kw) == -1, kw
        assert msg in lib.sg_last_error(), (kw, lib.sg_last_error())
    assert C.sizeof(C.c_void_p) == 8
