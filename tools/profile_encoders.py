#!/usr/bin/env python
"""Timing of the networks either side of the loop on the HIP kernels, at the sizes one pipeline call uses them:
CLIP text encoder on [uncond, prompt] + 3 previous prompts (model/pipeline.py:359-362), VAE encode of the zero image and 3 prior frames
at 512x512 (:390-404), VAE decode of one 64x64 latent (:198-205); and the CLIP-I / CLIP-T scorer (storygen_amd/clip_score.py) at ViT-B/32
geometry on 4 generated 512x512 frames against 4 ground-truth frames and 4 prompts.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel
table (profiles/r02j_*).  Random weights of the reference's configurations."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from storygen_amd.clip_score import ClipScorer  # noqa: E402
from storygen_amd.encoders import (ClipTextEngine, VaeEngine, clip_text_param_shapes, clip_vision_param_shapes, init_state,  # noqa: E402
                                   vae_param_shapes)

dev = torch.device("cuda:0")


def timed(fn, n=5):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    vae = VaeEngine(init_state(vae_param_shapes(), 0), dev)
    clip = ClipTextEngine(init_state(clip_text_param_shapes(), 1), dev, heads=12)
    ids = torch.randint(0, 49407, (5, 77))
    frames = torch.rand(4, 3, 512, 512, device=dev)
    z = torch.randn(1, 4, 64, 64, device=dev)
    out = dict(clip_text_5x77_ms=round(timed(lambda: clip(ids)), 3),
               vae_encode_4x512x512_ms=round(timed(lambda: vae.encode(frames)), 3),
               vae_encode_1x512x512_ms=round(timed(lambda: vae.encode(frames[:1])), 3),
               vae_decode_1x64x64_ms=round(timed(lambda: vae.decode(z)), 3))
    # convolution + attention work of AutoencoderKL at 512x512 (2*MAC): decode 1.24 TFLOP, encode 0.57 TFLOP per image
    out["vae_decode_tflops"] = round(1.24 / out["vae_decode_1x64x64_ms"] * 1e3, 1)
    out["vae_encode_tflops"] = round(4 * 0.566 / out["vae_encode_4x512x512_ms"] * 1e3, 1)
    # ViT-B/32 (openai/clip-vit-base-patch32): image tower 12 x 768, 12 heads, 50 tokens; text tower 12 x 512, 8 heads, 77 tokens; 512-d joint space
    tsh = clip_text_param_shapes(hidden_size=512, intermediate_size=2048)
    tsh["text_projection.weight"] = (512, 512)
    scorer = ClipScorer(init_state(clip_vision_param_shapes(), 2), dict(hidden_size=768, num_attention_heads=12, image_size=224, patch_size=32),
                        init_state(tsh, 3), dict(hidden_size=512, num_attention_heads=8), device=dev)
    gen, gt = torch.rand(4, 3, 512, 512, device=dev), torch.rand(4, 3, 512, 512, device=dev)
    out["clip_image_features_4x512x512_ms"] = round(timed(lambda: scorer.image_features(gen), 20), 3)
    out["clip_i_4_pairs_ms"] = round(timed(lambda: scorer.clip_i(gen, gt), 20), 3)
    out["clip_t_4_pairs_ms"] = round(timed(lambda: scorer.clip_t(gen, ids[:4]), 20), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
