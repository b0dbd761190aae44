"""Story generation on the GPU: sg_frame_handoff_f16 on every fp16 bit pattern and at its shape / stride / grid edges against the host
chain it replaces, a story against the same frames as chained pipeline calls with the host round trip (bit for bit), the best-of-N
selection with a small PickScorer, and sampler reuse across the frames of a story.

The story tests run the 2-level UNet of tests/test_dropin_gpu.py::test_pipeline_sees_new_unet_weights_between_calls at a 16 x 16 latent
with the HIP AutoencoderKL (two blocks: 32 x 32 frames) in fp16 and that file's table stand-ins for tokenizer and text encoder."""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_dropin_gpu import _Enc, _Tok
from tests import pick_score_reference as P
from tests import story_reference as SR

pytestmark = pytest.mark.gpu
F16 = torch.float16


# ------------------------------------------------------------------------------------------------------ the hand-off kernel
def test_handoff_every_fp16_bit_pattern_equals_the_host_chain(gpu):
    """All 65 536 patterns as one [1,3,148,148] image (zero-padded).  (a) = numpy_to_pil(decode_latents(.)), the pipeline's own methods
    with the clamp evaluated on the device in fp16 as in a real call; (b) = fp16(fp32(u8) / 255).  The 2 046 NaN patterns (a property of
    the format) give the documented 0; no other pattern is excluded."""
    from storygen_amd import ops
    from storygen_amd.model import StableDiffusionPipeline
    x, n = SR.as_image(SR.all_fp16_patterns())
    xg = x.to(gpu)
    u8, y = ops.frame_handoff(xg)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (1, 148, 148, 3) and y.dtype == F16 and tuple(y.shape) == (1, 3, 148, 148)
    pipe = StableDiffusionPipeline(vae=SimpleNamespace(config=None, decode=lambda z: SimpleNamespace(sample=xg.clone())), text_encoder=None,
                                   tokenizer=None, unet=None, scheduler=None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # numpy: NaN -> uint8 is an invalid cast (compared with the documented value)
        pil = pipe.numpy_to_pil(pipe.decode_latents(torch.zeros(1, 4, 2, 2, device=gpu, dtype=F16)))
    want_u8 = torch.from_numpy(np.asarray(pil[0]).copy())[None]
    want_y = (torch.from_numpy(np.asarray(pil[0]).copy()) / 255).permute(2, 0, 1).half()[None]
    nan = torch.isnan(x)
    assert n == 65536 and int(nan.sum()) == SR.NAN_PATTERNS
    nan_hwc = nan.permute(0, 2, 3, 1)
    got_u8, got_y = u8.cpu(), y.cpu()
    bad = int((got_u8[~nan_hwc] != want_u8[~nan_hwc]).sum()), int((got_y[~nan].view(torch.int16) != want_y[~nan].view(torch.int16)).sum())
    print(f"frame_handoff, 65536 patterns: {bad[0]} uint8 and {bad[1]} fp16 mismatches outside the {int(nan.sum())} NaN patterns")
    assert bad == (0, 0)
    assert int(got_u8[nan_hwc].max()) == 0 and int(got_y[nan].view(torch.int16).abs().max()) == 0
    ref_u8, ref_y = SR.handoff_reference(x)                  # and the NumPy restatement agrees everywhere, NaN included
    assert torch.equal(got_u8, ref_u8) and torch.equal(got_y.view(torch.int16), ref_y.view(torch.int16))


def _values(shape, seed):
    g = torch.Generator().manual_seed(seed)
    v = (torch.randn(shape, generator=g) * 1.2).half()
    flat = v.view(-1)
    special = torch.tensor([float("inf"), float("-inf"), float("nan"), -0.0, 1.0, -1.0, 6e-8, 65504.0], dtype=F16)
    k = min(flat.numel(), special.numel())
    flat[torch.randperm(flat.numel(), generator=g)[:k]] = special[:k]
    return v


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (3, 5), (8, 8), (17, 9), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_handoff_windows_of_larger_buffers(gpu, hw, N, aligned):
    """Input = a window (nonzero batch, channel and row stride) of a NaN-filled buffer; both outputs = windows of bit-pattern-filled
    buffers whose other elements must stay as they were.  aligned: column offset 8 in buffers 8-element-multiple wide (the 16-byte /
    8-byte vector path with its scalar tail where W % 8 != 0); unaligned: column offset 3 in odd-width buffers (element by element)."""
    from storygen_amd import ops
    H, W = hw
    off, Wb = (8, (W + 7) // 8 * 8 + 16) if aligned else (3, W + 7 + (W % 2 == 0))
    x = _values((N, 3, H, W), 1000 * H + 10 * W + N)
    xbuf = torch.full((N, 3, H + 2, Wb), float("nan"), dtype=F16, device=gpu)
    xbuf[:, :, 1:1 + H, off:off + W] = x.to(gpu)
    ubuf = (torch.arange(N * (H + 2) * Wb * 3, device=gpu) * 7 % 251).to(torch.uint8).view(N, H + 2, Wb, 3)
    ybuf = (torch.arange(N * 3 * (H + 2) * Wb, device=gpu) % 2039 - 1000).to(torch.int16).view(F16).view(N, 3, H + 2, Wb)
    u0, y0 = ubuf.clone(), ybuf.clone()
    xin, uout, yout = xbuf[:, :, 1:1 + H, off:off + W], ubuf[:, 1:1 + H, off:off + W], ybuf[:, :, 1:1 + H, off:off + W]
    assert (xin.data_ptr() % 16 == 0 and xin.stride(2) % 8 == 0 and uout.data_ptr() % 8 == 0) == aligned
    got = ops.frame_handoff(xin, uout, yout)
    assert got[0] is uout and got[1] is yout
    want_u8, want_y = SR.handoff_reference(x)
    u0[:, 1:1 + H, off:off + W], y0[:, :, 1:1 + H, off:off + W] = want_u8.to(gpu), want_y.to(gpu)
    assert torch.equal(ubuf, u0), "uint8 window or its guard elements"
    assert torch.equal(ybuf.view(torch.int16), y0.view(torch.int16)), "fp16 window or its guard elements"


@pytest.mark.parametrize("W", [1, 8], ids=["scalar", "vector"])
def test_handoff_grid_stride_loop_wraps(gpu, W):
    """The launch has at most FRAME_HANDOFF_MAX_BLOCKS workgroups of 256 work items (a pixel, or 8 pixels of a row on the vector path): one
    item more than that is the smallest size at which the grid-stride loop takes a second turn."""
    from storygen_amd import ops
    H = ops.FRAME_HANDOFF_MAX_BLOCKS * 256 + 1
    x = _values((1, 3, H, W), W)
    u8, y = ops.frame_handoff(x.to(gpu))
    want_u8, want_y = SR.handoff_reference(x)
    assert torch.equal(u8.cpu(), want_u8) and torch.equal(y.cpu().view(torch.int16), want_y.view(torch.int16))


def test_handoff_rejections(gpu):
    from storygen_amd import ops
    from test_story_host import test_frame_handoff_rejects_on_the_host
    test_frame_handoff_rejects_on_the_host()
    x = torch.zeros(1, 3, 4, 8, dtype=F16, device=gpu)
    with pytest.raises(TypeError):
        ops.frame_handoff(x.float())
    with pytest.raises(TypeError):
        ops.frame_handoff(x.cpu())
    with pytest.raises(ValueError, match=r"\[N,3,H,W\]"):
        ops.frame_handoff(x[:, :2])
    with pytest.raises(ValueError, match="outputs must be"):
        ops.frame_handoff(x, torch.zeros(1, 4, 8, 4, dtype=torch.uint8, device=gpu))
    with pytest.raises(ValueError, match="pixel stride"):
        ops.frame_handoff(x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2))
    both = torch.zeros(1024, dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError, match="outputs overlap"):
        ops.frame_handoff(x, both[:96].view(1, 4, 8, 3), both[64:64 + 192].view(F16).view(1, 3, 4, 8))
    with pytest.raises(RuntimeError, match="overlaps the input"):
        ops.frame_handoff(x, out_f16=x)
    with pytest.raises(RuntimeError):
        ops.frame_handoff(torch.zeros(1, 3, 0, 8, dtype=F16, device=gpu))
    with pytest.raises(RuntimeError):
        ops.frame_handoff(torch.zeros(0, 3, 4, 8, dtype=F16, device=gpu))


# ------------------------------------------------------------------------------------------------------ stories
CFG = dict(block_out_channels=(320, 640), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
           up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), cross_attention_dim=768, attention_head_dim=8, sample_size=128)
PROMPTS = ["", "p0", "p1", "p2", "p3", "p4"]
SIZE = 32                                   # frames: the two-block VAE halves once, the latent is 16 x 16


@pytest.fixture(scope="module")
def rig(gpu):
    from storygen_amd.arch import build_arch, load_config
    from storygen_amd.model import AutoencoderKL, UNet2DConditionModel
    from storygen_amd.synth import synthetic_inputs, synthetic_state_dict
    unet = UNet2DConditionModel.from_config(CFG)
    unet.load_state_dict(synthetic_state_dict(build_arch(load_config(CFG)), 1))
    unet = unet.to(gpu, F16).eval()
    vae = AutoencoderKL(block_out_channels=(64, 128), down_block_types=("DownEncoderBlock2D",) * 2, up_block_types=("UpDecoderBlock2D",) * 2,
                        seed=3).to(gpu, F16)
    table = torch.stack([synthetic_inputs(1, 1, 16, 16, 40 + i, 768)["text"][0] for i in range(len(PROMPTS))]).to(gpu, F16)
    return unet, vae, table


def _pipeline(rig):
    from storygen_amd.model import StableDiffusionPipeline
    from storygen_amd.scheduler import DDIMSchedule
    unet, vae, table = rig
    pipe = StableDiffusionPipeline(vae=vae, text_encoder=_Enc(table), tokenizer=_Tok(PROMPTS), unet=unet, scheduler=DDIMSchedule())
    pipe.set_progress_bar_config(disable=True)
    return pipe


def _chained(pipe, prompts, context_frames, steps, generator):
    """The story as a user of the reference's inference.py builds it: one pipeline call per frame with output_type="pil", each fed from
    the earlier calls' PIL images through the host round trip of inference.py:86-92."""
    pil = []
    for j, p in enumerate(prompts):
        prior = list(range(max(0, j - context_frames), j))
        if prior:
            stage, frames, prev = "auto-regressive", SR.host_round_trip([pil[i] for i in prior]).unsqueeze(0), [prompts[i] for i in prior]
        else:
            stage, frames, prev = "no", torch.zeros(1, 1, 3, SIZE, SIZE), [p]
        pil.append(pipe(stage=stage, prompt=p, image_prompt=frames, prev_prompt=prev, height=SIZE, width=SIZE, num_inference_steps=steps,
                        guidance_scale=7.0, image_guidance_scale=3.5, generator=generator, output_type="pil").images[0])
    return np.stack([np.asarray(im) for im in pil])


def test_story_equals_chained_calls_with_the_host_round_trip(gpu, rig):
    """3 frames, context_frames = 2, one sample per frame, 5 DDIM steps (a multiple of 5: the group schedule of the default 40).  Both runs
    start from the same global RNG state (the pipeline draws its shared noise with randn_like and the HIP VAE's latent_dist.sample() from
    it) and the same generator seed, and make the same calls in the same order, so the state is the same before every call — checked at
    the end.  The uint8 frames are identical."""
    from storygen_amd.story import StoryGenerator
    pipe = _pipeline(rig)
    prompts = PROMPTS[1:4]
    torch.manual_seed(77)
    story = StoryGenerator(pipe).generate(prompts, context_frames=2, num_inference_steps=5, height=SIZE, width=SIZE,
                                          generator=torch.Generator(device=gpu).manual_seed(5), output_type="uint8")
    state_story = torch.cuda.get_rng_state(gpu)
    torch.manual_seed(77)
    chained = _chained(pipe, prompts, 2, 5, torch.Generator(device=gpu).manual_seed(5))
    assert torch.equal(torch.cuda.get_rng_state(gpu), state_story)
    diff = int((story.frames != chained).sum())
    print(f"story vs chained calls: {diff} of {chained.size} bytes differ; distinct byte values per frame "
          f"{[len(np.unique(f)) for f in chained]}; frame 1 vs frame 2 differ in {int((chained[1] != chained[2]).sum())} bytes")
    assert story.frames.shape == (3, SIZE, SIZE, 3) and story.chosen == [0, 0, 0] and story.scores == [None] * 3
    assert all(len(np.unique(f)) > 16 for f in chained) and (chained[0] != chained[1]).any() and (chained[1] != chained[2]).any()
    assert diff == 0


def test_story_selection_keeps_the_scorers_argmax(gpu, rig):
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
    gen = StoryGenerator(pipe, scorer, tok)
    torch.manual_seed(3)
    out = gen.generate(PROMPTS[1:4], context_frames=2, samples_per_frame=3, num_inference_steps=3, height=SIZE, width=SIZE,
                       generator=[torch.Generator(device=gpu).manual_seed(s) for s in (11, 12, 13)], output_type="uint8")
    assert len(decoded) == 3
    for j, (u8, nxt) in enumerate(decoded):
        assert tuple(u8.shape) == (3, SIZE, SIZE, 3) and tuple(nxt.shape) == (3, 3, SIZE, SIZE)
        s = scorer.scores(ids[PROMPTS[1 + j]], u8.permute(0, 3, 1, 2).float() / 255.0)[0]
        print(f"frame {j}: scores {s.tolist()} probabilities {out.scores[j]} kept {out.chosen[j]}")
        assert out.chosen[j] == int(s.argmax()) and len(out.scores[j]) == 3 and abs(sum(out.scores[j]) - 1.0) < 1e-5
        assert np.array_equal(out.frames[j], u8[out.chosen[j]].cpu().numpy())
    # only the kept samples became context: the ring holds output (b) of the kept sample of the last two frames
    assert gen.context_prompts == PROMPTS[2:4] and len(gen.context) == 2
    for f, j in zip(gen.context, (1, 2)):
        assert torch.equal(f.view(torch.int16), decoded[j][1][out.chosen[j]].view(torch.int16))


def test_story_builds_one_sampler_per_distinct_key(gpu, rig, monkeypatch):
    """5 frames at context_frames = 3: R = 1 (stage "no"), 1, 2, 3, 3 -> four keys, four samplers; the second story builds none and
    gives the same frames."""
    import storygen_amd.model.pipeline as PL
    from storygen_amd.story import StoryGenerator
    built = []

    class Counting(PL.StoryGenSampler):
        def __init__(self, *a, **k):
            built.append(a[6])
            super().__init__(*a, **k)
    monkeypatch.setattr(PL, "StoryGenSampler", Counting)
    pipe = _pipeline(rig)
    gen = StoryGenerator(pipe)
    runs = []
    for _ in range(2):
        torch.manual_seed(9)
        runs.append(gen.generate(PROMPTS[1:6], context_frames=3, num_inference_steps=3, height=SIZE, width=SIZE,
                                 generator=torch.Generator(device=gpu).manual_seed(1), output_type="uint8").frames)
        assert built == [1, 1, 2, 3] and len(pipe._samplers) == 4
    assert np.array_equal(runs[0], runs[1])
