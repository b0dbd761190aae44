"""A stateful restatement of diffusers 0.13.1 `DPMSolverMultistepScheduler` (epsilon prediction, no thresholding) for the tests,
written the way the library writes it — a list of past converted model outputs and `lower_order_nums`, one update function per
order — and independent of the per-call table of storygen_amd.scheduler.DPMSolverMultistepSchedule.

Parity UNPINNED against diffusers itself (not installed): the formulas are the published DPM-Solver / DPM-Solver++ multistep
updates (Lu et al. 2022) as diffusers states them in `convert_model_output`, `dpm_solver_first_order_update` and
`multistep_dpm_solver_{second,third}_order_update`.  Its only pin to the reference's own output is order 1, which is DDIM (eta = 0):
tests/test_dpm_solver_gpu.py runs that against the latents of the reference's own 50-step loop.

It has the interface oracle.storygen_oracle.denoise_step drives (`add_noise(x, noise, t)`, `step(eps, t, x, n)`).  alpha / sigma /
lambda are float64 from the fp32 alphas_cumprod (diffusers keeps them as fp32 tensors: ~1e-7 relative apart); the update runs in
float64 and returns the sample's dtype."""
import numpy as np
import torch

from oracle import storygen_oracle as O


class DPMSolverMultistep:
    def __init__(self, solver_order=2, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                 timesteps=None):
        self.base = O.DDIM()
        ac = self.base.alphas_cumprod.double()
        self.alpha_t, self.sigma_t = ac.sqrt(), (1 - ac).sqrt()
        self.lambda_t = self.alpha_t.log() - self.sigma_t.log()
        self.solver_order, self.algorithm_type, self.solver_type = solver_order, algorithm_type, solver_type
        self.lower_order_final = lower_order_final
        self._timesteps_fn = timesteps
        self._ts = None

    def timesteps(self, n):
        if self._timesteps_fn is not None:
            return list(self._timesteps_fn(n))
        return [int(t) for t in np.linspace(0, 999, n + 1).round()[::-1][:-1].astype(np.int64)]      # set_timesteps

    def add_noise(self, x, noise, t):
        return self.base.add_noise(x, noise, t)

    # ------------------------------------------------------------------------------------------ diffusers' methods
    def convert_model_output(self, eps, t, x):
        if self.algorithm_type == "dpmsolver++":
            return (x - self.sigma_t[t] * eps) / self.alpha_t[t]
        return eps

    def first_order_update(self, m, s, t, x):
        lt, ls = self.lambda_t[t], self.lambda_t[s]
        at, as_ = self.alpha_t[t], self.alpha_t[s]
        st, ss = self.sigma_t[t], self.sigma_t[s]
        h = lt - ls
        if self.algorithm_type == "dpmsolver++":
            return (st / ss) * x - (at * (torch.exp(-h) - 1.0)) * m
        return (at / as_) * x - (st * (torch.exp(h) - 1.0)) * m

    def second_order_update(self, ms, tl, t, x):
        s0, s1 = tl[-1], tl[-2]
        m0, m1 = ms[-1], ms[-2]
        lt, l0, l1 = self.lambda_t[t], self.lambda_t[s0], self.lambda_t[s1]
        at, a0 = self.alpha_t[t], self.alpha_t[s0]
        st, s0_ = self.sigma_t[t], self.sigma_t[s0]
        h, h0 = lt - l0, l0 - l1
        r0 = h0 / h
        D0, D1 = m0, (1.0 / r0) * (m0 - m1)
        if self.algorithm_type == "dpmsolver++":
            if self.solver_type == "midpoint":
                return (st / s0_) * x - (at * (torch.exp(-h) - 1.0)) * D0 - 0.5 * (at * (torch.exp(-h) - 1.0)) * D1
            return (st / s0_) * x - (at * (torch.exp(-h) - 1.0)) * D0 + (at * ((torch.exp(-h) - 1.0) / h + 1.0)) * D1
        if self.solver_type == "midpoint":
            return (at / a0) * x - (st * (torch.exp(h) - 1.0)) * D0 - 0.5 * (st * (torch.exp(h) - 1.0)) * D1
        return (at / a0) * x - (st * (torch.exp(h) - 1.0)) * D0 - (st * ((torch.exp(h) - 1.0) / h - 1.0)) * D1

    def third_order_update(self, ms, tl, t, x):
        s0, s1, s2 = tl[-1], tl[-2], tl[-3]
        m0, m1, m2 = ms[-1], ms[-2], ms[-3]
        lt, l0, l1, l2 = self.lambda_t[t], self.lambda_t[s0], self.lambda_t[s1], self.lambda_t[s2]
        at, a0 = self.alpha_t[t], self.alpha_t[s0]
        st, s0_ = self.sigma_t[t], self.sigma_t[s0]
        h, h0, h1 = lt - l0, l0 - l1, l1 - l2
        r0, r1 = h0 / h, h1 / h
        D0 = m0
        D1_0, D1_1 = (1.0 / r0) * (m0 - m1), (1.0 / r1) * (m1 - m2)
        D1 = D1_0 + (r0 / (r0 + r1)) * (D1_0 - D1_1)
        D2 = (1.0 / (r0 + r1)) * (D1_0 - D1_1)
        if self.algorithm_type == "dpmsolver++":
            return ((st / s0_) * x - (at * (torch.exp(-h) - 1.0)) * D0 + (at * ((torch.exp(-h) - 1.0) / h + 1.0)) * D1
                    - (at * ((torch.exp(-h) - 1.0 + h) / h ** 2 - 0.5)) * D2)
        return ((at / a0) * x - (st * (torch.exp(h) - 1.0)) * D0 - (st * ((torch.exp(h) - 1.0) / h - 1.0)) * D1
                - (st * ((torch.exp(h) - 1.0 - h) / h ** 2 - 0.5)) * D2)

    def step(self, eps, t, x, n):
        if self._ts is None:                                   # set_timesteps(n) before the loop
            self._ts = self.timesteps(n)
            self.model_outputs = [None] * self.solver_order
            self.lower_order_nums = 0
        ts = self._ts
        dtype = x.dtype
        eps, x = eps.double(), x.double()
        i = ts.index(int(t))
        prev = 0 if i == len(ts) - 1 else ts[i + 1]
        lof = i == len(ts) - 1 and self.lower_order_final and len(ts) < 15
        los = i == len(ts) - 2 and self.lower_order_final and len(ts) < 15
        m = self.convert_model_output(eps, t, x)
        for j in range(self.solver_order - 1):
            self.model_outputs[j] = self.model_outputs[j + 1]
        self.model_outputs[-1] = m
        if self.solver_order == 1 or self.lower_order_nums < 1 or lof:
            out = self.first_order_update(m, t, prev, x)
        elif self.solver_order == 2 or self.lower_order_nums < 2 or los:
            out = self.second_order_update(self.model_outputs, [ts[i - 1], t], prev, x)
        else:
            out = self.third_order_update(self.model_outputs, [ts[i - 2], ts[i - 1], t], prev, x)
        if self.lower_order_nums < self.solver_order:
            self.lower_order_nums += 1
        return out.to(dtype)


def apply_row(row, e, x, hist):
    """One call of sg_cfg_dpm_step_f32 on an already guided epsilon, in the dtype of the inputs (hist: [3, ...], updated in
    place); `row` = DPMSolverMultistepSchedule.step_row(...)."""
    cx, ce, A, w0, w1, w2, cur, s1, s2, push = row
    m = cx * x + ce * e
    xp = A * x + w0 * m
    if w1 != 0.0:
        xp = xp + w1 * hist[int(s1)]
    if w2 != 0.0:
        xp = xp + w2 * hist[int(s2)]
    if push:
        hist[int(cur)] = m
    return xp


def dpm_on_ddim_timesteps(**kw):
    """Order-1 DPM-Solver++ (storygen_amd's schedule) forced onto DDIM's timestep list (981, 961, .., 1 for 50 steps): DDIM itself."""
    from storygen_amd.scheduler import DDIMSchedule, DPMSolverMultistepSchedule

    class DPMOnDDIMTimesteps(DPMSolverMultistepSchedule):
        def timesteps(self, n):
            return DDIMSchedule().timesteps(n)
    return DPMOnDDIMTimesteps(solver_order=1, **kw)
