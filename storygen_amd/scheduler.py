"""Schedule tables for the sampling loop (host side, fp32).

DDIMSchedule: computed exactly as diffusers' DDIMScheduler does for the scheduler the reference's inference.py builds
(inference.py:48: scaled-linear betas 0.00085..0.012, 1000 train steps, steps_offset=1, set_alpha_to_one=False,
clip_sample=False, eta=0).  PNDMSchedule: the class the shipped ckpt/stable-diffusion-v1-5/scheduler/scheduler_config.json
names (`_class_name: PNDMScheduler`, skip_prk_steps=true) — the PLMS linear-multistep rule of diffusers 0.13.1
(`PNDMScheduler.step_plms` / `_get_prev_sample`), restated from the published algorithm (diffusers is not installed here).
DPMSolverMultistepSchedule: DPM-Solver / DPM-Solver++ multistep (diffusers 0.13.1 `DPMSolverMultistepScheduler`, which
model/pipeline.py:7-16 also accepts), restated from the published formulas (Lu et al. 2022, "DPM-Solver" and "DPM-Solver++").
Reference call sites: model/pipeline.py:7-16,47-75 (accepted scheduler classes), :366-367 (set_timesteps), :420-424
(add_noise), :461 (step).

A schedule is the numbers; what the sampler does with them each step is its UpdateRule (`schedule.update_rule(eta)`): the one `ops`
entry point it launches, the scalars of a table row, and the fp32 buffers that kernel keeps between steps."""
from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Optional

import torch


class UpdateRule:
    """All the sampling loop knows about a scheduler's `step`.  This one is plain DDIM (sg_cfg_ddim_step_f32): no state, the row is
    the schedule's own `step_row`; the others override what differs."""
    key = "ddim"                 # hashable: rules with equal keys launch the same kernel on rows of the same length
    needs_noise = False          # the kernel adds std * noise (the sampler stages the step's variance noise for it)
    eta = 0.0

    def __init__(self, schedule: "DDIMSchedule"):
        self.schedule = schedule
        self.row_len = schedule.row_len          # scalars of a table row after the two guidance scales

    def row(self, k: int, ts: List[int], n: int) -> List[float]:
        return self.schedule.step_row(k, ts, n)

    def state(self, shape, device) -> Dict[str, torch.Tensor]:
        """The buffers the kernel keeps between the steps of a loop over latents of `shape`."""
        return {}

    def launch(self, ops, eps3, latents, latents3, state, noise, coef):
        ops.cfg_ddim_step(eps3, latents, latents3, coef)


class DDIMVarRule(UpdateRule):
    """DDIM with eta > 0 and / or clip_sample (sg_cfg_ddim_var_step_f32): row = (sa, sb, sap, dir, std, clip)."""
    key = "ddim-var"
    needs_noise = True

    def __init__(self, schedule: "DDIMSchedule", eta: float):
        self.schedule, self.eta, self.row_len = schedule, float(eta), 6

    def row(self, k, ts, n):
        return [*self.schedule.var_step_coef(int(ts[k]), n, self.eta), float(self.schedule.clip_sample)]

    def launch(self, ops, eps3, latents, latents3, state, noise, coef):
        ops.cfg_ddim_var_step(eps3, latents, latents3, noise, coef)


def _zeros(shape, device) -> torch.Tensor:
    return torch.zeros(tuple(shape), dtype=torch.float32, device=device)


class PLMSRule(UpdateRule):
    """PNDM / PLMS (sg_cfg_plms_step_f32): a ring of the last 4 guided epsilons and the sample kept by the first call."""
    key = "plms"

    def state(self, shape, device):
        return {"history": _zeros((4, *shape), device), "kept": _zeros(shape, device)}

    def launch(self, ops, eps3, latents, latents3, state, noise, coef):
        ops.cfg_plms_step(eps3, latents, latents3, state["history"], state["kept"], coef)


class DPMRule(UpdateRule):
    """Multistep DPM-Solver (sg_cfg_dpm_step_f32): a ring of the last 3 converted model outputs (fp32: x0 = (x - sigma e) / alpha)."""
    key = "dpm"

    def state(self, shape, device):
        return {"history": _zeros((3, *shape), device)}

    def launch(self, ops, eps3, latents, latents3, state, noise, coef):
        ops.cfg_dpm_step(eps3, latents, latents3, state["history"], coef)


# keys of a compatible scheduler's config that do not change the DDIM / PLMS arithmetic (diffusers ignores them the same way
# when inference.py:48 loads the shipped PNDM scheduler_config.json into a DDIMScheduler)
_IGNORED_KEYS = ("_class_name", "_diffusers_version", "_name_or_path", "_use_default_values", "skip_prk_steps")


class DDIMSchedule:
    kind = "ddim"          # the family of the update rule (update_rule() hands out the rule itself)
    row_len = 4            # floats step_row() contributes to a row of the sampler's per-step table

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", steps_offset: int = 1, set_alpha_to_one: bool = False,
                 clip_sample: bool = False, trained_betas=None, prediction_type: str = "epsilon", **unknown):
        unknown = {k: v for k, v in unknown.items() if k not in _IGNORED_KEYS}
        if unknown:
            raise NotImplementedError(f"{type(self).__name__}: unsupported scheduler config keys {sorted(unknown)}")
        if prediction_type != "epsilon":
            raise NotImplementedError(f"prediction_type={prediction_type!r}: only epsilon prediction is on the StoryGen path")
        self._config = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                            beta_schedule=beta_schedule, steps_offset=steps_offset, set_alpha_to_one=set_alpha_to_one,
                            trained_betas=None if trained_betas is None else [float(b) for b in trained_betas],
                            prediction_type=prediction_type,
                            # written out explicitly: diffusers' DDIMScheduler DEFAULTS clip_sample to True, so a saved config
                            # without the key would make the reference's inference.py:48
                            # (`DDIMScheduler.from_pretrained(ckpt, subfolder="scheduler")`) clip x0 on a checkpoint written here
                            clip_sample=bool(clip_sample))
        if trained_betas is not None:
            betas = torch.tensor([float(b) for b in trained_betas], dtype=torch.float32)
            if betas.numel() != num_train_timesteps:
                raise ValueError(f"trained_betas has {betas.numel()} entries for {num_train_timesteps} train timesteps")
        elif beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise NotImplementedError(f"{beta_schedule} is not implemented for DDIMSchedule")
        # x0 clamped to [-1, 1] in every step (diffusers' DDIMScheduler default; PNDM / DPM-Solver have no such key and drop it)
        self.clip_sample = bool(clip_sample)
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.num_train_timesteps = num_train_timesteps
        self.steps_offset = steps_offset
        self.init_noise_sigma = 1.0

    @classmethod
    def from_pretrained(cls, path: str, subfolder: Optional[str] = "scheduler") -> "DDIMSchedule":
        with open(os.path.join(path, subfolder or "", "scheduler_config.json")) as f:
            return cls(**{k: v for k, v in json.load(f).items() if not k.startswith("_")})

    @property
    def config(self) -> dict:
        return dict(self._config, _class_name=self.diffusers_name)

    diffusers_name = "DDIMScheduler"

    def save_pretrained(self, save_directory: str):
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, "scheduler_config.json"), "w") as f:
            json.dump(dict(self.config, _diffusers_version="0.13.1"), f, indent=2)

    save_config = save_pretrained

    def key(self) -> tuple:
        """Hashable identity of the schedule (cache key of the pipeline's sampler)."""
        c = self._config
        return (type(self).__name__,) + tuple((k, tuple(v) if isinstance(v, list) else v) for k, v in sorted(c.items()))

    def update_rule(self, eta: Optional[float] = 0.0) -> UpdateRule:
        """What the loop launches each step at diffusers' `eta` (pipeline.py:208-221,461 hands it to DDIM only: PNDM and DPM-Solver
        ignore it).  eta = None: the plain rule whatever clip_sample says (the schedule's own step_row)."""
        if eta is None or (eta == 0 and not self.clip_sample):
            return UpdateRule(self)
        return DDIMVarRule(self, eta)

    def step_row(self, k: int, ts: List[int], n: int) -> List[float]:
        """The scalars the update kernel needs at loop index k (timesteps `ts` = self.timesteps(n))."""
        return list(self.step_coef(int(ts[k]), n))

    def timesteps(self, n: int) -> List[int]:
        ratio = self.num_train_timesteps // n
        return [int(round(i * ratio)) + self.steps_offset for i in reversed(range(n))]

    def add_noise_coef(self, t: int):
        """(sqrt(abar_t), sqrt(1 - abar_t)) as fp32 python floats (memoised per timestep: a sampler's step table asks for the same few
        hundred values a thousand times per prepare(), ~10 us of tensor indexing each)."""
        memo = self.__dict__.setdefault("_add_noise_memo", {})
        t = int(t)
        v = memo.get(t)
        if v is None:
            a = self.alphas_cumprod[t]
            v = memo[t] = (float(a ** 0.5), float((1 - a) ** 0.5))
        return v

    def step_coef(self, t: int, n: int):
        """(sqrt(abar_t), sqrt(1-abar_t), sqrt(abar_prev), sqrt(1-abar_prev)) for x_t -> x_{t - T/n}, eta = 0."""
        memo = self.__dict__.setdefault("_step_coef_memo", {})
        v = memo.get((int(t), int(n)))
        if v is None:
            prev = t - self.num_train_timesteps // n
            a_t = self.alphas_cumprod[t]
            a_p = self.alphas_cumprod[prev] if prev >= 0 else self.final_alpha_cumprod
            v = memo[(int(t), int(n))] = (float(a_t ** 0.5), float((1 - a_t) ** 0.5), float(a_p ** 0.5), float((1 - a_p) ** 0.5))
        return v

    def var_step_coef(self, t: int, n: int, eta: float):
        """(sqrt(abar_t), sqrt(1-abar_t), sqrt(abar_prev), dir, std) for x_t -> x_{t - T/n} with diffusers' eta
        (`DDIMScheduler.step` / `_get_variance`, the same fp32 tensor arithmetic): std = eta sqrt(variance), variance =
        (1 - abar_prev) / (1 - abar_t) (1 - abar_t / abar_prev), dir = sqrt(1 - abar_prev - std^2).  eta = 0 gives step_coef(t, n)
        and std = 0."""
        memo = self.__dict__.setdefault("_var_step_coef_memo", {})
        key = (int(t), int(n), float(eta))
        v = memo.get(key)
        if v is None:
            prev = t - self.num_train_timesteps // n
            a_t = self.alphas_cumprod[t]
            a_p = self.alphas_cumprod[prev] if prev >= 0 else self.final_alpha_cumprod
            variance = ((1 - a_p) / (1 - a_t)) * (1 - a_t / a_p)
            std = float(eta) * variance ** 0.5
            v = memo[key] = (float(a_t ** 0.5), float((1 - a_t) ** 0.5), float(a_p ** 0.5), float((1 - a_p - std ** 2) ** 0.5),
                             float(std))
        return v


class PNDMSchedule(DDIMSchedule):
    """diffusers 0.13.1 PNDMScheduler with skip_prk_steps=True (the SD-1.5 default): pseudo linear multistep (PLMS).

    n inference steps make n + 1 UNet evaluations: timesteps = [s_{n-1}, s_{n-2}, s_{n-2}, s_{n-3}, ..., s_0]
    (`set_timesteps`).  With e_c the (guided) epsilon of call c and `ets` the history of calls c != 1:
        c = 0 : e' = e_0,                               x <- prev(x, t, t - r, e'),  the incoming sample is kept
        c = 1 : e' = (e_1 + e_0) / 2,                   x <- prev(kept sample, t + r, t, e')      (e_1 is not stored)
        c = 2 : e' = (3 e_2 - e_0) / 2
        c = 3 : e' = (23 e_3 - 16 e_2 + 5 e_0) / 12
        c >= 4: e' = (55 e_c - 59 ets[-2] + 37 ets[-3] - 9 ets[-4]) / 24
    prev(x, t, p, e) = sqrt(a_p / a_t) x - (a_p - a_t) e / (a_t sqrt(1 - a_p) + sqrt(a_t (1 - a_t) a_p))   (`_get_prev_sample`).
    step_row() encodes one call as [A, Bc, w0..w3, slot_cur, slot1..slot3, push, use_kept, keep]: the update kernel computes
    e' = w0 e + sum_i w_i hist[slot_i], optionally stores e in hist[slot_cur] first (a 4-deep ring), and applies
    x <- A x_src - Bc e' with x_src = the kept sample (use_kept) or the current latents."""
    kind = "plms"
    row_len = 13
    diffusers_name = "PNDMScheduler"

    def __init__(self, skip_prk_steps: bool = False, **kw):
        if not skip_prk_steps:
            raise NotImplementedError("PNDM with Runge-Kutta warm-up steps (skip_prk_steps=false) is not on the StoryGen path; the "
                                      "shipped scheduler_config.json sets skip_prk_steps=true")
        kw.pop("clip_sample", None)                      # not a PNDMScheduler key: diffusers drops it the same way
        super().__init__(**kw)
        self._config["skip_prk_steps"] = True
        self._config.pop("set_alpha_to_one", None)
        self._config.pop("clip_sample", None)            # not a PNDMScheduler key
        self._config["set_alpha_to_one"] = kw.get("set_alpha_to_one", False)

    def update_rule(self, eta: Optional[float] = 0.0) -> UpdateRule:
        return PLMSRule(self)

    def timesteps(self, n: int) -> List[int]:
        ratio = self.num_train_timesteps // n
        base = [int(round(i * ratio)) + self.steps_offset for i in range(n)]
        return (base[:-1] + base[-2:-1] + base[-1:])[::-1]

    def _prev_coef(self, t: int, prev: int):
        a_t = float(self.alphas_cumprod[t])
        a_p = float(self.alphas_cumprod[prev]) if prev >= 0 else float(self.final_alpha_cumprod)
        A = (a_p / a_t) ** 0.5
        denom = a_t * (1.0 - a_p) ** 0.5 + (a_t * (1.0 - a_t) * a_p) ** 0.5
        return A, (a_p - a_t) / denom

    def step_row(self, k: int, ts: List[int], n: int) -> List[float]:
        ratio = self.num_train_timesteps // n
        t = int(ts[k])
        if k == 1:
            A, Bc = self._prev_coef(t + ratio, t)
        else:
            A, Bc = self._prev_coef(t, t - ratio)
        pushes = k if k < 2 else k - 1             # history entries stored BEFORE this call (call 1 stores nothing)
        push = 0 if k == 1 else 1
        cur = pushes % 4                           # ring slot this call's epsilon goes to (if pushed)
        n_hist = pushes + push                     # len(ets) after the append
        back = lambda j: (cur - j) % 4 if push else (pushes - j) % 4      # noqa: E731  slot of ets[-1-j] (push) / ets[-j] (no push)
        if k == 0:
            w, sl = [1.0, 0.0, 0.0, 0.0], [0, 0, 0]
        elif k == 1:
            w, sl = [0.5, 0.5, 0.0, 0.0], [back(1), 0, 0]
        elif n_hist == 2:
            w, sl = [1.5, -0.5, 0.0, 0.0], [back(1), 0, 0]
        elif n_hist == 3:
            w, sl = [23.0 / 12.0, -16.0 / 12.0, 5.0 / 12.0, 0.0], [back(1), back(2), 0]
        else:
            w, sl = [55.0 / 24.0, -59.0 / 24.0, 37.0 / 24.0, -9.0 / 24.0], [back(1), back(2), back(3)]
        return [A, Bc, *w, float(cur), *map(float, sl), float(push), float(k == 1), float(k == 0)]


# keys of a DDIM / PNDM config that do not apply to DPM-Solver: diffusers ignores them the same way in
# `DPMSolverMultistepScheduler.from_config(ddim.config)`, the usual way of switching schedulers
_DPM_IGNORED_KEYS = _IGNORED_KEYS + ("steps_offset", "set_alpha_to_one", "clip_sample")


class DPMSolverMultistepSchedule(DDIMSchedule):
    """diffusers 0.13.1 DPMSolverMultistepScheduler (epsilon prediction, no thresholding), the multistep DPM-Solver of
    Lu et al. 2022: "DPM-Solver++(2M)" with the defaults solver_order=2, algorithm_type="dpmsolver++".

    Timesteps: linspace(0, T - 1, n + 1).round()[::-1][:-1] (n UNet evaluations, 999, 949, .. for n = 20, T = 1000); the step
    after the last one goes to timestep 0 (alphas_cumprod[0]).  With alpha = sqrt(abar), sigma = sqrt(1 - abar),
    lambda = log alpha - log sigma, h = lambda_t - lambda_s0 (s0 = this call's timestep, t = the next one), and m_j the
    converted model output of the call j steps back (`convert_model_output`: x0 = (x - sigma_s e) / alpha_s for dpmsolver++,
    e itself for dpmsolver), one call of `step` is
        first order  (`dpm_solver_first_order_update`):   x' = A x + c D0
        second order (`multistep_dpm_solver_second_order_update`, r0 = h_0 / h):
                     D1 = (m0 - m1) / r0,  x' = A x + c D0 + b D1          (midpoint: b = c / 2)
        third order  (`multistep_dpm_solver_third_order_update`, r1 = h_1 / h):
                     D1_0 = (m0 - m1) / r0,  D1_1 = (m1 - m2) / r1,  D1 = D1_0 + r0 / (r0 + r1) (D1_0 - D1_1),
                     D2 = (D1_0 - D1_1) / (r0 + r1),  x' = A x + c D0 + b D1 + d D2
    with, for dpmsolver++: A = sigma_t / sigma_s0, c = -alpha_t (e^-h - 1), b (heun, 3rd order) = alpha_t ((e^-h - 1) / h + 1),
    d = -alpha_t ((e^-h - 1 + h) / h^2 - 0.5); for dpmsolver: A = alpha_t / alpha_s0, c = -sigma_t (e^h - 1),
    b (heun, 3rd order) = -sigma_t ((e^h - 1) / h - 1), d = -sigma_t ((e^h - 1 - h) / h^2 - 0.5).  Call k runs the order
    min(solver_order, k + 1), except that with lower_order_final and fewer than 15 timesteps the last call is first order and
    (order 3) the last but one second order.
    Every case is linear in (x, m0, m1, m2): step_row() encodes call k as [cx, ce, A, w0, w1, w2, slot_cur, slot1, slot2, push]
    and the update kernel computes m = cx x + ce e, x' = A x + w0 m + w1 hist[slot1] + w2 hist[slot2], hist[slot_cur] = m
    (a 3-deep ring of converted model outputs, fp32).  The scalars are computed in float64 from the fp32 alphas_cumprod (diffusers
    keeps alpha / sigma / lambda as fp32 tensors: ~1e-7 relative apart)."""
    kind = "dpm"
    row_len = 10
    diffusers_name = "DPMSolverMultistepScheduler"

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", trained_betas=None, solver_order: int = 2,
                 prediction_type: str = "epsilon", thresholding: bool = False, dynamic_thresholding_ratio: float = 0.995,
                 sample_max_value: float = 1.0, algorithm_type: str = "dpmsolver++", solver_type: str = "midpoint",
                 lower_order_final: bool = True, **unknown):
        unknown = {k: v for k, v in unknown.items() if k not in _DPM_IGNORED_KEYS}
        if unknown:
            raise NotImplementedError(f"{type(self).__name__}: unsupported scheduler config keys {sorted(unknown)}")
        if thresholding:
            raise NotImplementedError("thresholding=True (dynamic thresholding) is not on the StoryGen path")
        if solver_order not in (1, 2, 3):
            raise NotImplementedError(f"solver_order={solver_order!r}: DPMSolverMultistepScheduler implements orders 1, 2 and 3")
        if algorithm_type not in ("dpmsolver++", "dpmsolver"):
            raise NotImplementedError(f"algorithm_type={algorithm_type!r}: only dpmsolver++ and dpmsolver exist")
        if solver_type not in ("midpoint", "heun"):
            raise NotImplementedError(f"solver_type={solver_type!r}: only midpoint and heun exist")
        super().__init__(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                         beta_schedule=beta_schedule, trained_betas=trained_betas, prediction_type=prediction_type)
        self.solver_order, self.algorithm_type, self.solver_type = int(solver_order), algorithm_type, solver_type
        self.lower_order_final = bool(lower_order_final)
        self._config = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                            beta_schedule=beta_schedule, trained_betas=self._config["trained_betas"], solver_order=int(solver_order),
                            prediction_type=prediction_type, thresholding=False,
                            dynamic_thresholding_ratio=float(dynamic_thresholding_ratio), sample_max_value=float(sample_max_value),
                            algorithm_type=algorithm_type, solver_type=solver_type, lower_order_final=bool(lower_order_final))

    @classmethod
    def from_config(cls, config, **kwargs) -> "DPMSolverMultistepSchedule":
        """The diffusers idiom `DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)`: a dict-like config of this or
        a DDIM / PNDM scheduler (their DDIM-only keys are ignored); keyword arguments override its entries."""
        cfg = dict(config) if isinstance(config, dict) else dict(vars(config))
        cfg.update(kwargs)
        return cls(**{k: v for k, v in cfg.items() if not k.startswith("_")})

    def update_rule(self, eta: Optional[float] = 0.0) -> UpdateRule:
        return DPMRule(self)

    def timesteps(self, n: int) -> List[int]:
        import numpy as np          # numpy's linspace + round-half-to-even, exactly as `set_timesteps` computes them
        T = self.num_train_timesteps
        return [int(t) for t in np.linspace(0, T - 1, n + 1).round()[::-1][:-1].astype(np.int64)]

    def _als(self, t: int):
        """(alpha, sigma, lambda) of timestep t in float64 from the fp32 alphas_cumprod."""
        a = float(self.alphas_cumprod[t])
        alpha, sigma = math.sqrt(a), math.sqrt(1.0 - a)
        return alpha, sigma, math.log(alpha) - math.log(sigma)

    def order_at(self, k: int, n_ts: int) -> int:
        """The order of call k of a loop over n_ts timesteps (diffusers' lower_order_nums / lower_order_final logic)."""
        lof = self.lower_order_final and n_ts < 15
        if self.solver_order == 1 or k == 0 or (lof and k == n_ts - 1):
            return 1
        if self.solver_order == 2 or k == 1 or (lof and k == n_ts - 2):
            return 2
        return 3

    def step_row(self, k: int, ts: List[int], n: int) -> List[float]:
        T = len(ts)
        s0 = int(ts[k])
        t = int(ts[k + 1]) if k + 1 < T else 0
        al_t, sg_t, lam_t = self._als(t)
        al_0, sg_0, lam_0 = self._als(s0)
        h = lam_t - lam_0
        if self.algorithm_type == "dpmsolver++":
            cx, ce = 1.0 / al_0, -sg_0 / al_0
            A = sg_t / sg_0
            em = math.expm1(-h)                                  # e^-h - 1
            c = -al_t * em
            b_heun = al_t * (em / h + 1.0)
            d = -al_t * ((em + h) / (h * h) - 0.5)
        else:
            cx, ce = 0.0, 1.0
            A = al_t / al_0
            ep = math.expm1(h)                                   # e^h - 1
            c = -sg_t * ep
            b_heun = -sg_t * (ep / h - 1.0)
            d = -sg_t * ((ep - h) / (h * h) - 0.5)
        order = self.order_at(k, T)
        w = [c, 0.0, 0.0]
        if order == 2:
            r0 = (lam_0 - self._als(int(ts[k - 1]))[2]) / h
            b = 0.5 * c if self.solver_type == "midpoint" else b_heun
            w = [c + b / r0, -b / r0, 0.0]
        elif order == 3:
            lam_1, lam_2 = self._als(int(ts[k - 1]))[2], self._als(int(ts[k - 2]))[2]
            r0, r1 = (lam_0 - lam_1) / h, (lam_1 - lam_2) / h
            b = b_heun                                           # the third-order update has no midpoint form
            g = (b * r0 + d) / (r0 + r1)                         # weight of D1_0 - D1_1 in b D1 + d D2
            w = [c + b / r0 + g / r0, -b / r0 - g * (1.0 / r0 + 1.0 / r1), g / r1]
        cur = k % 3                                              # ring slot of m0; m1 / m2 sit one / two slots back
        return [cx, ce, A, *w, float(cur), float((k - 1) % 3), float((k - 2) % 3), 1.0]


def schedule_from_config(cfg, class_name: str = "") -> DDIMSchedule:
    """A diffusers scheduler `.config` (dict, FrozenDict or attribute object) -> DDIMSchedule / PNDMSchedule /
    DPMSolverMultistepSchedule; raises NotImplementedError for every other scheduler class instead of silently running DDIM.
    Euler, EulerAncestral and LMS stay out: their add_noise looks the reference pass's timestep (t / 10, pipeline.py:414-424) up
    in their own timestep table, where it never is, so they cannot run the context stages."""
    def get(k, default=None):
        if isinstance(cfg, dict):
            return cfg.get(k, default)
        return getattr(cfg, k, default)
    name = get("_class_name") or class_name
    keys = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "steps_offset", "set_alpha_to_one", "clip_sample",
            "trained_betas", "prediction_type", "skip_prk_steps")
    kw = {k: get(k) for k in keys if get(k) is not None}
    if name in ("DPMSolverMultistepScheduler", "DPMSolverMultistepSchedule"):
        dpm_keys = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "trained_betas", "solver_order",
                    "prediction_type", "thresholding", "dynamic_thresholding_ratio", "sample_max_value", "algorithm_type",
                    "solver_type", "lower_order_final")
        return DPMSolverMultistepSchedule(**{k: get(k) for k in dpm_keys if get(k) is not None})
    if "PNDM" in name:
        kw.pop("clip_sample", None)
        return PNDMSchedule(**kw)
    if "DDIM" in name or name in ("", "DDIMSchedule"):
        kw.pop("skip_prk_steps", None)
        return DDIMSchedule(**kw)
    raise NotImplementedError(f"scheduler {name!r}: the HIP loop implements DDIM (any eta, clip_sample), PNDM/PLMS (skip_prk_steps) and "
                              "DPMSolverMultistepScheduler (DPM-Solver / DPM-Solver++)")
