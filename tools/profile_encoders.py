#!/usr/bin/env python
"""Timing of the networks either side of the loop on the HIP kernels, at the sizes one pipeline call uses them:
CLIP text encoder on [uncond, prompt] + 3 previous prompts (model/pipeline.py:359-362), VAE encode of the zero image and 3 prior frames
at 512x512 (:390-404), VAE decode of one 64x64 latent (:198-205); and the CLIP-I / CLIP-T scorer (storygen_amd/clip_score.py) at ViT-B/32
geometry on 4 generated 512x512 frames against 4 ground-truth frames and 4 prompts.  `--pick` instead runs the PickScore block
(storygen_amd/pick_score.py at CLIP ViT-H/14 geometry: 10 frames of 512x512 and one prompt, inference_COCO_val.py's best-of-ten) and the
attention A/B at its shape (sg_attn_enc_f16 against sg_transpose_batched_f16 + sg_attn_fwd_f16).  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel
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


def pick_score_block():
    """PickScore at the real geometry with init_state weights: vision 32 x 1280 (16 heads of 80, MLP 5120, patch 14, image 224, gelu), text
    24 x 1024 (16 heads of 64, MLP 4096, gelu), projection 1024; ms for 10 frames of 512 x 512 plus one prompt."""
    from storygen_amd.pick_score import PickScorer
    vc = dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16, image_size=224, patch_size=14, hidden_act="gelu")
    tc = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, hidden_act="gelu")
    sd = init_state(clip_vision_param_shapes(1280, 5120, 32, 224, 14, 1024), 4)
    tsh = clip_text_param_shapes(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24)
    tsh["text_projection.weight"] = (1024, 1024)
    sd.update(init_state(tsh, 5))
    sd["logit_scale"] = torch.tensor(4.6052)
    scorer = PickScorer(sd, dict(vision_config=vc, text_config=tc), device=dev)
    frames = torch.rand(10, 3, 512, 512, device=dev)
    ids = torch.randint(0, 49407, (1, 77))
    return dict(pick_image_tower_10x512x512_ms=round(timed(lambda: scorer.image_features(frames), 10), 3),
                pick_text_tower_1x77_ms=round(timed(lambda: scorer.text_features(ids), 10), 3),
                pick_best_of_10_ms=round(timed(lambda: scorer.best_of(ids, frames), 10), 3))


def attention_ab(B=10, H=16, T=257, D=80, rounds=7):
    """sg_attn_enc_f16 against the only composition the previous kernels offer for that shape: sg_transpose_batched_f16 (V -> V^T, token count
    padded to a multiple of 8) followed by sg_attn_fwd_f16.  One untimed pass over both sides, then `rounds` alternating rounds in this process;
    every figure is a loop of >= 0.1 s of kernel time between two events."""
    from storygen_amd import ops
    C, Tp = H * D, (T + 7) & ~7
    g = torch.Generator().manual_seed(0)
    qkv = torch.zeros(B, Tp, 3 * C, dtype=torch.float16, device=dev)
    qkv[:, :T] = torch.randn(B, T, 3 * C, generator=g).half().to(dev)
    q, k, v = qkv[:, :T, :C], qkv[:, :T, C:2 * C], qkv[:, :T, 2 * C:]
    vt = torch.zeros(B, C, Tp, dtype=torch.float16, device=dev)
    o_new, o_old = torch.empty(B, T, C, dtype=torch.float16, device=dev), torch.empty(B, T, C, dtype=torch.float16, device=dev)
    scale = D ** -0.5

    def new():
        ops.attention_enc(q, k, v, o_new, H, scale, False)

    def old():
        ops.transpose_batched(qkv[:, :, 2 * C:], vt)
        ops.attention(q, k, vt, o_old, H, scale, nk=T)

    def loop(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1e3        # us per call

    new(), old()
    torch.cuda.synchronize()
    agree = float((o_new.float() - o_old.float()).norm() / o_old.float().norm())
    n = max(200, int(0.1e6 / min(loop(new, 50), loop(old, 50))) + 1)
    t_new, t_old = [], []
    for _ in range(rounds):
        t_new.append(loop(new, n))
        t_old.append(loop(old, n))
    med = lambda x: sorted(x)[len(x) // 2]   # noqa: E731
    return dict(attn_ab_shape=f"B{B} H{H} T{T} D{D}", attn_ab_calls_per_figure=n, attn_ab_outputs_rel_l2=round(agree, 6),
                attn_enc_us_median=round(med(t_new), 2), attn_enc_us_min=round(min(t_new), 2),
                transpose_plus_attention_us_median=round(med(t_old), 2), transpose_plus_attention_us_min=round(min(t_old), 2),
                attn_ab_ratio_median=round(med(t_new) / med(t_old), 3), attn_ab_goal="<= 1.03")


def main():
    if "--pick" in sys.argv:
        out = attention_ab()
        out.update(pick_score_block())
        print(json.dumps(out))
        return
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
