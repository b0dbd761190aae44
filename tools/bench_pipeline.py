#!/usr/bin/env python
"""End-to-end latency of one `StableDiffusionPipeline.__call__` in the reference's default inference setting (inference.py:58-64,103-115,
127-131: 40 DDIM steps, 512x512, guidance 7.0 / 3.5, 3 prior frames) with every network on the HIP kernels: CLIP text encoder on the
prompts, VAE encode of the prior frames, the denoising loop, VAE decode.  Random weights of the reference's configs (no checkpoints here),
a stand-in tokenizer (token ids are irrelevant for timing).  Prints one JSON line; non-contract (bench.py is the contract).

    python tools/bench_pipeline.py [STEPS] [--scheduler ddim|dpm] [--eta E]     one configuration (default: 40 DDIM steps, eta 0)
    python tools/bench_pipeline.py --compare ddim:40,ddim:50,dpm:20,dpm:25,ddim:40:0.5 [--rounds 5]      (a third field = eta)
        several configurations in one process (one pipeline each, sharing the networks), timed in alternation round by round so that
        drift of the machine spreads over all of them; one JSON line per configuration with every sample.
    python tools/bench_pipeline.py --story K [STEPS] [--rounds 3]
        a K-frame story (storygen_amd.story.StoryGenerator, context_frames 3, one sample per frame, no scorer) against the same K frames
        as chained pipeline calls with the host round trip of inference.py (PIL image, PNG in memory, reload, ToTensor, upload), timed in
        alternation; one JSON line with both totals, the per-frame times, and the story's split into encode (text encoder + VAE
        encoder), loop, decode, hand-off and scoring from one extra run with a device synchronisation around each part.
    python tools/bench_pipeline.py --ingest K WxH [--rounds 5]
        K reference frames of W x H pixels (decoded RGB PIL images, random content) to the pipeline's fp16 [K,3,512,512] on the device:
        storygen_amd.image.load_reference_images (upload of the raw bytes + sg_image_resize_u8) against the host chain it replaces
        (PIL resize, ToTensor, cast to fp16, upload), timed in alternation after an untimed pass over both, and the kernel alone on
        resident bytes (device events); one JSON line.  No network is built.
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
    ap.add_argument("--story", type=int, default=0, metavar="K", help="time a K-frame story against K chained calls with the host round trip")
    ap.add_argument("--ingest", nargs=2, metavar=("K", "WxH"), help="time the ingest of K raw W x H frames against the host chain")
    args = ap.parse_args()
    if args.ingest:
        return ingest(args)
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
    if args.story:
        return story(args, unet, vae, clip, dev)
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


def ingest(args):
    import numpy as np
    from PIL import Image
    from storygen_amd import ops
    from storygen_amd.image import load_reference_images
    K, (W, H) = int(args.ingest[0]), (int(v) for v in args.ingest[1].lower().split("x"))
    dev, size = torch.device("cuda:0"), (512, 512)
    rng = np.random.default_rng(0)
    images = [Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)) for _ in range(K)]

    def host_chain():      # inference.py:84-89 on decoded images, then the pipeline's cast and upload
        frames = [torch.from_numpy(np.asarray(im.resize(size)).copy()).permute(2, 0, 1).float().div(255) for im in images]
        return torch.stack(frames).half().to(dev)

    def device_chain():
        return load_reference_images(images, size=size, device=dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0
    a, b = timed(host_chain)[0], timed(device_chain)[0]          # untimed pass: allocator, coefficient tables
    res = {"host": [], "device": []}
    for _ in range(args.rounds):
        for name, fn in (("host", host_chain), ("device", device_chain)):
            res[name].append(timed(fn)[1])
    resident = torch.stack([torch.from_numpy(np.array(im)) for im in images]).to(dev)
    out_f16 = torch.empty(K, 3, size[1], size[0], dtype=torch.float16, device=dev)
    ops.image_resize(resident, size, out_u8=False, out_f16=out_f16)
    kernel = []
    for _ in range(max(args.rounds, 5)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.image_resize(resident, size, out_u8=False, out_f16=out_f16)
        e1.record()
        torch.cuda.synchronize()
        kernel.append(e0.elapsed_time(e1) * 1e-3)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    print(json.dumps({"workload": f"{K} decoded RGB frames of {W}x{H} -> fp16 [{K},3,512,512] on the device; host = PIL resize + ToTensor + "
                                  "fp16 + upload, device = upload of the bytes + sg_image_resize_u8 (load_reference_images)",
                      "frames": K, "source": [W, H], "bits_identical": bool(torch.equal(a.view(torch.int16), b.view(torch.int16))),
                      "host_chain_seconds_median": round(med(res["host"]), 6), "device_chain_seconds_median": round(med(res["device"]), 6),
                      "kernel_alone_seconds_median": round(med(kernel), 6), "host_chain_seconds_all": [round(t, 6) for t in res["host"]],
                      "device_chain_seconds_all": [round(t, 6) for t in res["device"]], "kernel_alone_seconds_all": [round(t, 6) for t in kernel]}))


def story(args, unet, vae, clip, dev):
    import io

    import numpy as np
    from PIL import Image

    from storygen_amd import ops
    from storygen_amd.story import StoryGenerator
    K, steps, cf = args.story, args.steps, 3
    prompts = [f"frame {j}" for j in range(K)]
    pipe = StableDiffusionPipeline(vae=vae, text_encoder=clip, tokenizer=Tok(), unet=unet, scheduler=SCHEDULERS[args.scheduler][1]())
    pipe.set_progress_bar_config(disable=True)
    gen = StoryGenerator(pipe)
    kw = dict(num_inference_steps=steps, guidance_scale=7.0, image_guidance_scale=3.5, height=512, width=512)
    marks, mem = [], []

    def run_story():
        torch.manual_seed(0)
        marks.clear()
        real = pipe._decode_device

        def decode(lat):                       # per-frame times: the host reaches this point once per frame
            out = real(lat)
            torch.cuda.synchronize()
            marks.append(time.perf_counter())
            mem.append(torch.cuda.memory_allocated())
            return out
        pipe._decode_device = decode
        try:
            return gen.generate(prompts, context_frames=cf, generator=torch.Generator(device=dev).manual_seed(1), output_type="uint8", **kw).frames
        finally:
            del pipe._decode_device

    def run_chained():
        torch.manual_seed(0)
        marks.clear()
        g, pil = torch.Generator(device=dev).manual_seed(1), []
        for j, p in enumerate(prompts):
            prior = list(range(max(0, j - cf), j))
            if prior:
                reloaded = []
                for i in prior:                # inference.py:86-92 on the saved file (here a PNG in memory)
                    buf = io.BytesIO()
                    pil[i].save(buf, format="PNG")
                    buf.seek(0)
                    reloaded.append(torch.from_numpy(np.asarray(Image.open(buf).convert("RGB")).copy()).permute(2, 0, 1).float() / 255)
                stage, ip, prev = "auto-regressive", torch.stack(reloaded).unsqueeze(0), [prompts[i] for i in prior]
            else:
                stage, ip, prev = "no", torch.zeros(1, 1, 3, 512, 512), [p]
            pil.append(pipe(stage=stage, prompt=p, image_prompt=ip, prev_prompt=prev, generator=g, output_type="pil", **kw).images[0])
            marks.append(time.perf_counter())
        return np.stack([np.asarray(im) for im in pil])

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0, [round(b - a, 4) for a, b in zip([t0] + marks[:-1], marks)]

    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, first_story_s, _ = timed(run_story)               # builds the samplers, captures the graphs
    held = torch.cuda.memory_allocated() - base
    grown = [m - n for m, n in zip(mem, [base] + mem[:-1])]      # frame 0: repacked UNet weights + the stage-"no" sampler; then one new sampler per frame
    b, _, _ = timed(run_chained)
    res = {"story": [], "chained": []}
    for _ in range(args.rounds):
        for name, fn in (("story", run_story), ("chained", run_chained)):
            _, t, per = timed(fn)
            res[name].append((t, per))
    # the split: one more story with a synchronisation around each part (not one of the timed runs)
    split = {"encode": 0.0, "decode": 0.0, "handoff": 0.0, "scoring": 0.0}

    def part(name, fn):
        def wrapped(*a_, **k_):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a_, **k_)
            torch.cuda.synchronize()
            split[name] += time.perf_counter() - t0
            return out
        return wrapped
    real_handoff = ops.frame_handoff
    pipe._encode_prompt, vae.encode, vae.decode = part("encode", pipe._encode_prompt), part("encode", vae.encode), part("decode", vae.decode)
    ops.frame_handoff = part("handoff", real_handoff)
    try:
        _, total, _ = timed(run_story)
    finally:
        ops.frame_handoff = real_handoff
        del pipe._encode_prompt, vae.encode, vae.decode
    split["loop"] = total - sum(split.values())
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    out = {"workload": f"{K}-frame story, {steps} {SCHEDULERS[args.scheduler][0]} steps per frame, 512x512, context_frames {cf}, one sample per "
                       "frame, no scorer, HIP CLIP + VAE + UNet, fp16; chained = the same frames as pipeline calls with the host round trip "
                       "(PIL, PNG in memory, reload, ToTensor, upload)",
           "frames": K, "steps": steps, "frames_identical": bool(np.array_equal(a, b)),
           "story_seconds_median": round(med([t for t, _ in res["story"]]), 4), "chained_seconds_median": round(med([t for t, _ in res["chained"]]), 4),
           "story_seconds_all": [round(t, 4) for t, _ in res["story"]], "chained_seconds_all": [round(t, 4) for t, _ in res["chained"]],
           "story_seconds_per_frame": res["story"][-1][1], "chained_seconds_per_frame": res["chained"][-1][1],
           "story_split_seconds_synchronised": {k: round(v, 4) for k, v in split.items()}, "story_split_total": round(total, 4),
           "first_story_seconds_incl_sampler_construction": round(first_story_s, 2), "samplers_cached": len(pipe._samplers),
           "device_bytes_held_after_first_story": int(held), "device_bytes_grown_per_frame_of_first_story": grown[:K], "device_peak_bytes": int(torch.cuda.max_memory_allocated())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
