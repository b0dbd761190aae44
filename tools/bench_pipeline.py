#!/usr/bin/env python
"""End-to-end latency of one `StableDiffusionPipeline.__call__` in the reference's default inference setting (inference.py:58-64,103-115,
127-131: 40 DDIM steps, 512x512, guidance 7.0 / 3.5, 3 prior frames) with every network on the HIP kernels: CLIP text encoder on the
prompts, VAE encode of the prior frames, the denoising loop, VAE decode.  Random weights of the reference's configs (no checkpoints here),
a stand-in tokenizer (token ids are irrelevant for timing).  Prints one JSON line; non-contract (bench.py is the contract).

    python tools/bench_pipeline.py [STEPS] [--scheduler ddim|dpm] [--eta E]     one configuration (default: 40 DDIM steps, eta 0)
    python tools/bench_pipeline.py --compare ddim:40,ddim:50,dpm:20,dpm:25,ddim:40:0.5 [--rounds 5]      (a third field = eta)
        several configurations in one process (one pipeline each, sharing the networks), timed in alternation round by round so that
        drift of the machine spreads over all of them; one JSON line per configuration with every sample.
dpm = DPM-Solver++(2M), diffusers' DPMSolverMultistepScheduler defaults (storygen_amd.scheduler.DPMSolverMultistepSchedule)."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from storygen_amd.arch import SD15_CONFIG  # noqa: E402
from storygen_amd.model import AutoencoderKL, CLIPTextModel, StableDiffusionPipeline, UNet2DConditionModel  # noqa: E402
from storygen_amd.scheduler import DDIMSchedule, DPMSolverMultistepSchedule  # noqa: E402

SCHEDULERS = {"ddim": ("DDIM", DDIMSchedule), "dpm": ("DPM-Solver++(2M)", DPMSolverMultistepSchedule)}


class Tok:
    model_max_length = 77

    def __call__(self, prompt, padding=None, max_length=None, truncation=None, return_tensors=None):
        n = 1 if isinstance(prompt, str) else len(prompt)
        g = torch.Generator().manual_seed(n)
        ids = torch.randint(1, 49000, (n, 77), generator=g)
        return SimpleNamespace(input_ids=ids, attention_mask=torch.ones_like(ids))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=40)
    ap.add_argument("--scheduler", choices=sorted(SCHEDULERS), default="ddim")
    ap.add_argument("--eta", type=float, default=0.0, help="DDIM's eta (> 0: stochastic DDIM, the variance noise drawn from a seeded "
                                                           "generator inside the timed call, as a user's call draws it)")
    ap.add_argument("--compare", default="", help="comma-separated scheduler:steps[:eta] list, timed in alternation")
    ap.add_argument("--rounds", type=int, default=3, help="timed calls per configuration")
    args = ap.parse_args()
    def parse(c):
        f = c.split(":")
        return f[0], int(f[1]), float(f[2]) if len(f) > 2 else 0.0
    configs = [parse(c) for c in args.compare.split(",")] if args.compare else [(args.scheduler, args.steps, args.eta)]
    for name, _, _ in configs:
        if name not in SCHEDULERS:
            raise SystemExit(f"unknown scheduler {name!r} (choose from {sorted(SCHEDULERS)})")
    dev, f16 = torch.device("cuda:0"), torch.float16
    unet = UNet2DConditionModel.from_config(SD15_CONFIG).to(dev, f16).eval()
    vae = AutoencoderKL(block_out_channels=(128, 256, 512, 512), down_block_types=("DownEncoderBlock2D",) * 4,
                        up_block_types=("UpDecoderBlock2D",) * 4, layers_per_block=2).to(dev, f16)
    clip = CLIPTextModel(dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12)).to(dev, f16)
    frames = torch.rand(1, 3, 3, 512, 512)
    pipes = []
    for name, steps, _ in configs:          # one pipeline (hence one cached sampler and its graphs) per configuration
        pipe = StableDiffusionPipeline(vae=vae, text_encoder=clip, tokenizer=Tok(), unet=unet, scheduler=SCHEDULERS[name][1]())
        pipe.set_progress_bar_config(disable=True)
        pipes.append(pipe)

    def call(i):
        return pipes[i](stage="multi-image-condition", prompt="a", image_prompt=frames, prev_prompt=["b", "c", "d"], height=512,
                        width=512, num_inference_steps=configs[i][1], guidance_scale=7.0, image_guidance_scale=3.5,
                        eta=configs[i][2], generator=torch.Generator(device=dev).manual_seed(0) if configs[i][2] > 0 else None,
                        output_type="np").images

    imgs = []
    for i in range(len(configs)):
        imgs.append(call(i))                  # builds the sampler, captures the graphs
    torch.cuda.synchronize()
    ts = [[] for _ in configs]
    for _ in range(args.rounds):
        for i in range(len(configs)):
            t0 = time.perf_counter()
            imgs[i] = call(i)
            torch.cuda.synchronize()
            ts[i].append(time.perf_counter() - t0)
    for (name, steps, eta), samples, img in zip(configs, ts, imgs):
        srt = sorted(samples)
        med = srt[len(srt) // 2]
        print(json.dumps({"workload": f"one pipeline call: {steps} {SCHEDULERS[name][0]} steps, 512x512, 3 prior frames, CFG, HIP CLIP + "
                                      "VAE + UNet, fp16",
                          "scheduler": name, "steps": steps, "eta": eta, "seconds_per_image_median": round(med, 4), "seconds_min": round(srt[0], 4),
                          "seconds_max": round(srt[-1], 4), "seconds_all": [round(v, 4) for v in samples],
                          "ms_per_step_incl_everything": round(med / steps * 1e3, 2), "image_shape": list(img.shape),
                          "finite": bool(torch.isfinite(torch.as_tensor(img)).all())}))


if __name__ == "__main__":
    main()
