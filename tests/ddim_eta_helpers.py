"""TEST INFRASTRUCTURE for tests/test_ddim_eta.py and tests/test_ddim_eta_gpu.py: the clean-room shim's DDIMScheduler (the
restatement of diffusers 0.13.1 `DDIMScheduler.step` the oracle itself steps with) as the reference of the eta / clip_sample path,
the variance noise drawn in the reference's order by an implementation of its own, and a stand-in sampler that records what the
drop-in pipeline hands to `prepare`."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

SD_BETAS = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
S_IMG, S_TXT = 3.5, 7.5


def shim_ddim(n_steps=None, **kw):
    """oracle/diffusers_shim's DDIMScheduler on SD-1.5's betas (steps_offset 1 and set_alpha_to_one False unless overridden, as
    inference.py:48 loads it), with `set_timesteps(n_steps)` applied when given."""
    shim = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "diffusers_shim")
    sys.path.insert(0, shim)
    try:
        from diffusers.schedulers import DDIMScheduler
    finally:
        sys.path.remove(shim)
    cfg = dict(SD_BETAS, steps_offset=1, set_alpha_to_one=False, clip_sample=False)
    cfg.update(kw)
    s = DDIMScheduler(**cfg)
    if n_steps is not None:
        s.set_timesteps(n_steps)
    return s


def ulp32(v) -> float:
    """Spacing of fp32 at |v|."""
    return float(np.spacing(np.float32(abs(float(v)))))


def guided(eps3: torch.Tensor, n: int) -> torch.Tensor:
    """The 3-way guidance combine of pipeline.py:457-458 in torch (fp32 when eps3 is)."""
    eu, ei, ea = eps3[:n], eps3[n:2 * n], eps3[2 * n:]
    return eu + S_IMG * (ei - eu) + S_TXT * (ea - ei)


def reference_order_noise(seeds, steps: int, shape, dtype=torch.float32, device="cpu") -> torch.Tensor:
    """What `scheduler.step(..., eta > 0, generator=generator)` draws over `steps` steps from FRESH generators seeded `seeds` (an
    int: one generator, one [N, 4, h, w] draw per step; a list: one [1, 4, h, w] draw per generator per step, concatenated).
    -> [steps, N, 4, h, w]."""
    if isinstance(seeds, int):
        g = torch.Generator(device=device).manual_seed(seeds)
        return torch.stack([torch.randn(tuple(shape), generator=g, device=device, dtype=dtype) for _ in range(steps)])
    gens = [torch.Generator(device=device).manual_seed(s) for s in seeds]
    rows = []
    for _ in range(steps):
        rows.append(torch.cat([torch.randn((1,) + tuple(shape[1:]), generator=g, device=device, dtype=dtype) for g in gens]))
    return torch.stack(rows)


class RecordingSampler:
    """Stands in for StoryGenSampler inside storygen_amd.model.pipeline: keeps the arguments of every `prepare`, steps nothing."""
    made = []

    def __init__(self, arch, state_dict, device, n, h, w, R, S, schedule=None, weights=None, ref_ahead=1):
        self.schedule, self.G = schedule, ref_ahead
        self.prepared = []
        self.latents = torch.zeros(n, 4, h, w)
        RecordingSampler.made.append(self)

    def prepare(self, inputs, steps, stage, guidance_scale, image_guidance_scale, **kw):
        self.prepared.append(dict(kw, steps=steps))
        self.timesteps = self.schedule.timesteps(steps)
        self.latents = inputs["latents"].float().clone()

    def step(self, k):
        pass

    def check_guards(self):
        pass


class _Tok:
    model_max_length = 77

    def __call__(self, prompt, padding=None, max_length=None, truncation=None, return_tensors=None):
        n = 1 if isinstance(prompt, str) else len(prompt)
        ids = torch.zeros(n, 77, dtype=torch.long)
        return SimpleNamespace(input_ids=ids, attention_mask=torch.ones_like(ids))


class _Enc:
    config = SimpleNamespace()

    def __init__(self, dtype):
        self.dtype = dtype

    def __call__(self, input_ids, attention_mask=None):
        return (torch.zeros(input_ids.shape[0], 77, 8, dtype=self.dtype),)


class _Vae:
    config = SimpleNamespace(block_out_channels=(128, 256, 512, 512))

    def encode(self, x):
        lat = torch.zeros(x.shape[0], 4, x.shape[-2] // 8, x.shape[-1] // 8, dtype=x.dtype)
        return SimpleNamespace(latent_dist=SimpleNamespace(sample=lambda: lat))


def cpu_pipeline(monkeypatch, schedule, dtype=torch.float32):
    """A StableDiffusionPipeline on the CPU whose networks are constants and whose sampler is a RecordingSampler: everything around
    the loop runs as shipped (prepare_latents, the noise draws, the sampler cache), nothing needs a GPU."""
    import storygen_amd.model.pipeline as P
    monkeypatch.setattr(P, "StoryGenSampler", RecordingSampler)
    RecordingSampler.made = []
    unet = SimpleNamespace(device=torch.device("cpu"), in_channels=4, config=SimpleNamespace(sample_size=8), _arch=None,
                           _engine_weights=lambda w=object(): w)
    pipe = P.StableDiffusionPipeline(vae=_Vae(), text_encoder=_Enc(dtype), tokenizer=_Tok(), unet=unet, scheduler=schedule)
    pipe.set_progress_bar_config(disable=True)
    return pipe


def cpu_call(pipe, n_prompts: int, steps: int, **kw):
    prompt = "a" if n_prompts == 1 else ["a"] * n_prompts
    prev = ["b", "c"] if n_prompts == 1 else [["b"] * n_prompts, ["c"] * n_prompts]
    return pipe(stage="multi-image-condition", prompt=prompt, image_prompt=torch.zeros(n_prompts, 2, 3, 64, 64), prev_prompt=prev,
                height=64, width=64, num_inference_steps=steps, output_type="latent", **kw)


def cfg_ddim_var_step(eps3, latents, latents3, noise, coef):
    """sg_cfg_ddim_var_step_f32 in torch on the CPU (for sampler tests on tests/stub_engine.py's stand-in engine)."""
    c = [float(v) for v in coef]
    eps = guided(eps3, latents.shape[0])
    x0 = (latents - c[3] * eps) / c[2]
    if c[7] != 0.0:
        x0 = x0.clamp(-1, 1)
    xp = c[4] * x0 + c[5] * eps
    if c[6] != 0.0:
        xp = xp + c[6] * noise
    latents.copy_(xp)
    if latents3 is not None:
        latents3.copy_(torch.cat([latents] * 3))
    return latents
