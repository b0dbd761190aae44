"""Story generation: consecutive frames, each conditioned on the frames generated before it and on their prompts — what the
reference's default `auto-regressive` stage and its Visual-Language Context module exist for, and what a user of its inference.py
builds by hand around the pipeline call: decode the frame, bring it to the host, quantise it to 8 bits, save a PNG, reload it, run
ToTensor, upload it, call again with one more prior frame (inference.py:84-92,103-120), with the best-of-N PickScore selection of
inference_COCO_val.py:143-148 in between.

    story = StoryGenerator(pipeline, scorer, tokenizer).generate(["A cat.", "The cat sleeps.", "The cat wakes up."], samples_per_frame=10,
                                                                 generator=[torch.Generator("cuda").manual_seed(s) for s in seeds])
    story.frames      # one image per prompt
    story.chosen      # which of the samples of each frame was kept
    story.scores      # the scorer's probabilities per frame (None without a scorer)

Between frames nothing leaves the device: the decoder's output goes through ONE kernel (sg_frame_handoff_f16, ops.frame_handoff) that
writes both the frame as it would have been saved (uint8, bit for bit numpy_to_pil(decode_latents(.))) and the tensor the reload of that
file would have produced (fp16 in [0, 1]); the latter of the kept sample joins a ring of context frames on the device, the former goes
to the scorer and, once, at the end, to the host.  The frames are the ones the chained calls with the host round trip give.

Convention of the context frames: values in [0, 1].  inference.py:90-91 (`for ref_image in ref_images: ref_image = ref_image * 2. - 1.`)
rebinds its loop variable, so the `* 2 - 1` never reaches the tensor the pipeline gets; that convention is kept, for `first_frames` too.

First frames the caller brings may be raw 8-bit images of any size (PIL images, uint8 arrays, a uint8 [K,h,w,3] tensor): they are resized
on the device exactly as Pillow's `.resize((width, height))` and ToTensor would (storygen_amd/image.py, sg_image_resize_u8).

Out of scope: reading / writing / converting image files (the caller passes decoded RGB images or [K,3,H,W] tensors), multi-GPU stories
(independent: the data-parallel launcher applies unchanged)."""
from __future__ import annotations

from collections import deque, namedtuple
from typing import List, Optional

import numpy as np
import torch

StoryOutput = namedtuple("StoryOutput", ["frames", "chosen", "scores"])
OUTPUT_TYPES = ("pil", "np", "uint8")


def context_schedule(n_frames: int, context_frames: int, n_first: int = 0):
    """Which story positions frame j is conditioned on, oldest first: the last min(j + n_first, context_frames) of the story so far.
    Positions count the caller's first frames too (0 .. n_first - 1), generated frame j sits at n_first + j."""
    return [list(range(max(0, n_first + j - context_frames), n_first + j)) for j in range(n_frames)]


class StoryGenerator:
    def __init__(self, pipeline, scorer=None, tokenizer=None):
        """pipeline: a storygen_amd.model.StableDiffusionPipeline running in fp16 (the reference's mixed_precision).  scorer: a
        storygen_amd.pick_score.PickScorer (or anything with its `best_of`) choosing among the samples of a frame; it needs `tokenizer`,
        the scorer's own (PickScore's processor, inference_COCO_val.py:27-33), called as tokenizer(prompt, padding=True, truncation=True,
        max_length=77, return_tensors="pt")."""
        if scorer is not None and tokenizer is None:
            raise ValueError("StoryGenerator: a scorer needs its tokenizer")
        self.pipeline, self.scorer, self.tokenizer = pipeline, scorer, tokenizer
        self.context: List[torch.Tensor] = []           # the ring after the last generate(): fp16 [3,H,W] device tensors, oldest first
        self.context_prompts: List[str] = []

    @torch.no_grad()
    def generate(self, prompts: List[str], *, context_frames: int = 3, stage: str = "auto-regressive", samples_per_frame: int = 1,
                 first_frames=None, first_prompts: Optional[List[str]] = None, num_inference_steps: int = 40,
                 guidance_scale: float = 7.0, image_guidance_scale: float = 3.5, eta: float = 0.0, generator=None, height: int = 512,
                 width: int = 512, output_type: str = "pil", score_uint8: bool = False) -> StoryOutput:
        """One frame per prompt.  Frame j is one pipeline call conditioned on the last min(j + len(first_frames), context_frames) frames
        of the story so far — the caller's `first_frames` (a float [K,3,H,W] tensor in [0, 1], or raw 8-bit images of any size: a list of
        PIL images / uint8 [h,w,3] arrays or a uint8 [K,h,w,3] tensor, resized as Pillow's `.resize((width, height))` + ToTensor by
        image.load_reference_images; with `first_prompts`), then the kept generated frames —
        oldest first, with their prompts as `prev_prompt` (the order of the reference's `ref_image` / `ref_prompt` lists).  A frame with
        no prior frame runs stage "no", the reference's text-only path; the call still wants one `image_prompt` frame and prompt
        (pipeline.py encodes them before the stage is looked at, and the sampler is sized for at least one): a zero frame and the
        frame's own prompt, neither of which that stage reads.

        samples_per_frame > 1: every frame is one call with num_images_per_prompt = samples_per_frame (`generator`: one per sample, as
        inference.py:97-101 builds them; they keep advancing from frame to frame).  The frame kept is np.argmax of
        scorer.best_of(input_ids, frames)'s probabilities on the uint8 frames (inference_COCO_val.py:143-147; the first of equals) —
        sample 0 without a scorer.  Only the kept frame becomes context.  score_uint8=True hands the scorer the uint8 frames as they are
        (a PickScorer then preprocesses them exactly as the script's processor preprocesses the saved images); the default converts them to
        float [S,3,H,W] = uint8 / 255 first, which the scorer resamples in floating point.

        output_type: "pil" (list of PIL images), "uint8" (numpy [F,H,W,3]) or "np" (float32 [F,H,W,3] = uint8 / 255: the SAVED frames,
        unlike the pipeline's "np", which is not quantised).  Returns StoryOutput(frames, chosen, scores): chosen[j] the kept sample of
        frame j, scores[j] the probabilities of its samples (None where nothing was scored)."""
        prompts = list(prompts) if isinstance(prompts, (list, tuple)) else None
        if not prompts or not all(isinstance(p, str) for p in prompts):
            raise ValueError("StoryGenerator.generate: prompts must be a non-empty list of strings")
        if not isinstance(context_frames, int) or context_frames < 1:
            raise ValueError(f"StoryGenerator.generate: context_frames must be >= 1, got {context_frames!r}")
        if not isinstance(samples_per_frame, int) or samples_per_frame < 1:
            raise ValueError(f"StoryGenerator.generate: samples_per_frame must be >= 1, got {samples_per_frame!r}")
        if output_type not in OUTPUT_TYPES:
            raise ValueError(f"StoryGenerator.generate: output_type must be one of {OUTPUT_TYPES}, got {output_type!r}")
        if isinstance(generator, (list, tuple)) and len(generator) != samples_per_frame:
            raise ValueError(f"StoryGenerator.generate: {len(generator)} generators for {samples_per_frame} samples per frame")
        if (first_frames is None) != (first_prompts is None):
            raise ValueError("StoryGenerator.generate: first_frames and first_prompts go together")
        pipe = self.pipeline
        dev = pipe.device
        ring = deque(maxlen=context_frames)              # (fp16 [3,H,W] on the device, prompt), oldest first
        if first_frames is not None:
            if isinstance(first_frames, (list, tuple)) or (isinstance(first_frames, torch.Tensor) and first_frames.dtype == torch.uint8):
                from .image import load_reference_images
                first_frames = load_reference_images(first_frames, size=(width, height), device=dev)
            if first_frames.dim() != 4 or tuple(first_frames.shape[1:]) != (3, height, width) or not first_frames.is_floating_point():
                raise ValueError(f"StoryGenerator.generate: first_frames must be a float [K,3,{height},{width}] tensor in [0, 1], got "
                                 f"{first_frames.dtype} {tuple(first_frames.shape)}")
            if len(first_prompts) != first_frames.shape[0]:
                raise ValueError(f"StoryGenerator.generate: {first_frames.shape[0]} first frames but {len(first_prompts)} first prompts")
            for f, p in zip(first_frames.to(dev, torch.float16), first_prompts):
                ring.append((f, p))
        kept, chosen, scores = [], [], []
        for prompt in prompts:
            if ring:
                frame_stage, ctx, ctx_prompts = stage, torch.stack([f for f, _ in ring]), [p for _, p in ring]
            else:
                frame_stage, ctx, ctx_prompts = "no", torch.zeros(1, 3, height, width, dtype=torch.float16, device=dev), [prompt]
            latents = pipe(stage=frame_stage, prompt=prompt, image_prompt=ctx.unsqueeze(0), prev_prompt=ctx_prompts, height=height,
                           width=width, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                           image_guidance_scale=image_guidance_scale, num_images_per_prompt=samples_per_frame, eta=eta,
                           generator=list(generator) if isinstance(generator, (list, tuple)) else generator, output_type="latent").images
            u8, nxt = pipe._decode_device(latents)       # uint8 [S,H,W,3] as saved | fp16 [S,3,H,W] as reloaded, both on the device
            k, probs = 0, None
            if self.scorer is not None and samples_per_frame > 1:
                ids = self.tokenizer(prompt, padding=True, truncation=True, max_length=77, return_tensors="pt").input_ids
                _, probs = self.scorer.best_of(ids, u8 if score_uint8 else u8.permute(0, 3, 1, 2).float() / 255.0)
                probs = probs.detach().float().cpu()
                k = int(np.argmax(probs.numpy()))        # inference_COCO_val.py:147
            chosen.append(k)
            scores.append(None if probs is None else probs.tolist())
            kept.append(u8[k])
            ring.append((nxt[k].clone(), prompt))
        self.context, self.context_prompts = [f for f, _ in ring], [p for _, p in ring]
        frames = torch.stack(kept).cpu().numpy()         # the one device-to-host copy of the story
        if output_type == "pil":
            from PIL import Image
            frames = [Image.fromarray(f) for f in frames]
        elif output_type == "np":
            frames = frames.astype(np.float32) / 255.0
        return StoryOutput(frames=frames, chosen=chosen, scores=scores)
