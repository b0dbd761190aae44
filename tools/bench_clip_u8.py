"""Times the preprocessing of 8-bit frames for the PickScore tower, on the GPU: 10 uint8 frames of 512 x 512 to ViT-H/14 patch rows
[10 * 256, 592] through sg_clip_patchify_u8 (one launch), beside the float path the scorers used for such frames before
(u8.permute(0, 3, 1, 2).float() / 255, then sg_clip_patchify_padk_f16), alternating in one process.  Also the largest
|score(uint8 path) - score(float path)| over those frames with a random tiny PickScore-like tower.

    python tools/bench_clip_u8.py [--out FILE]

An untimed pass first; every figure is the median over rounds of device-event time, the rounds of a figure together hold about 0.2 s of kernel time (>= 0.1 s)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_u8: needs the GPU (no CPU path)")
    from storygen_amd import ops
    dev = torch.device("cuda:0")
    N, S, ps, kpad = 10, 224, 14, 592
    g = torch.Generator().manual_seed(0)
    # textured frames: a smooth field plus noise, like decoded images (pure noise would overstate the difference between the resamplers)
    base = torch.nn.functional.interpolate(torch.rand(N, 3, 32, 32, generator=g), size=(512, 512), mode="bicubic", align_corners=False)
    u8 = ((base + 0.08 * torch.randn(N, 3, 512, 512, generator=g)).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev)
    rows_u8 = torch.empty(N * 256, kpad, dtype=torch.float16, device=dev)
    rows_f = torch.empty(N * 256, kpad, dtype=torch.float16, device=dev)

    def new():
        ops.clip_patchify_u8(u8, rows_u8, S, ps, MEAN, STD, crop="floor", kpad=kpad)

    def old():
        ops.clip_patchify((u8.permute(0, 3, 1, 2).float() / 255.0).contiguous(), rows_f, S, ps, MEAN, STD, kpad=kpad)      # as the engine feeds it

    new(), old()
    torch.cuda.synchronize()
    reps = {}
    for name, fn in (("new", new), ("old", old)):
        once = timed(fn, 20)
        reps[name] = max(20, int(200.0 / max(once, 1e-3)) // args.rounds + 1)       # rounds * reps * once ~ 0.2 s of kernel time per figure
    t = {"new": [], "old": []}
    for _ in range(args.rounds):
        for name, fn in (("new", new), ("old", old)):
            t[name].append(timed(fn, reps[name]))
    total = {k: sum(v) * reps[k] / 1e3 for k, v in t.items()}
    lines = [f"10 uint8 frames 512x512 -> ViT-H/14 patch rows [2560, 592], {args.rounds} alternating rounds, device events",
             f"  sg_clip_patchify_u8 (one launch)                          median {statistics.median(t['new']) * 1e3:8.1f} us  "
             f"(min {min(t['new']) * 1e3:.1f}, max {max(t['new']) * 1e3:.1f}; {reps['new']} launches per round)",
             f"  permute + float / 255 + sg_clip_patchify_padk_f16         median {statistics.median(t['old']) * 1e3:8.1f} us  "
             f"(min {min(t['old']) * 1e3:.1f}, max {max(t['old']) * 1e3:.1f}; {reps['old']} launches per round)"]
    lines.append(f"  timed kernel time in all: {total['new']:.3f} s and {total['old']:.3f} s")
    d = (rows_u8[:, :588].float() - rows_f[:, :588].float()).abs()
    lines.append(f"  patch rows, uint8 path vs float path: max |difference| {float(d.max()):.4f}, mean {float(d.mean()):.5f} "
                 f"(one 8-bit level is {1 / 255 / max(STD):.4f} .. {1 / 255 / min(STD):.4f} after Normalize)")
    # a random tiny tower at ViT-H/14's image and patch size
    from storygen_amd.encoders import clip_text_param_shapes, clip_vision_param_shapes, init_state
    from storygen_amd.pick_score import PickScorer
    vc = dict(hidden_size=160, intermediate_size=320, num_hidden_layers=2, num_attention_heads=2, image_size=224, patch_size=14, hidden_act="gelu")
    tc = dict(vocab_size=96, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
              hidden_act="gelu")
    tshapes = clip_text_param_shapes(96, 64, 128, 2, 77)
    tshapes["text_projection.weight"] = (32, 64)
    sd = {**init_state(clip_vision_param_shapes(160, 320, 2, 224, 14, 32), 1), **init_state(tshapes, 2)}
    for k in sd:
        if "embedding" in k:
            sd[k] = sd[k] * 10
    sd["logit_scale"] = torch.tensor(4.6052)
    scorer = PickScorer(sd, dict(vision_config=vc, text_config=tc), device=dev)
    ids = torch.randint(2, 94, (1, 24), generator=g)
    ids[:, 0], ids[:, 10], ids[:, 11:] = 0, 95, 1
    s_u8 = scorer.scores(ids, u8)[0]
    s_f = scorer.scores(ids, u8.permute(0, 3, 1, 2).float() / 255.0)[0]
    lines.append(f"  random tiny tower (2 layers, hidden 160, exp(logit_scale) = 100): scores {[round(v, 3) for v in s_u8.tolist()]}")
    lines.append(f"  largest |score(uint8 path) - score(float path)| = {float((s_u8 - s_f).abs().max()):.4f}; "
                 f"argmax uint8 {int(s_u8.argmax())}, float {int(s_f.argmax())}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
