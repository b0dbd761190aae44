"""TEST INFRASTRUCTURE for tests/test_update_rules.py and oracle/make_golden_step_tables.py: the cases of
tests/golden/step_tables.json, how a case's step table is made, and a recorder of the `ops` calls a sampler's loop makes
(tests/stub_engine.py's engine, tests/fake_ops.py's update rules, CPU)."""
import types

import torch

UNITS0 = [(0, 0, 0), (1, 0, 0), (1, 1, 0)]
R, B, S_IMG, S_TXT = 2, 3, 3.5, 7.5
MIC, AR = "multi-image-condition", "auto-regressive"

_DPM2 = dict(solver_order=2, algorithm_type="dpmsolver++", solver_type="midpoint")      # n = 10 < 15: lower_order_final applies
_DPM3 = dict(solver_order=3, algorithm_type="dpmsolver", solver_type="heun")
# name -> (schedule class, its keywords, inference steps, G, overlap, stage, eta); eta None = step_table's default
TABLES = {
    "ddim_g1_overlap": ("DDIMSchedule", {}, 10, 1, True, MIC, None),
    "ddim_g1_serial": ("DDIMSchedule", {}, 10, 1, False, MIC, None),
    "ddim_g5_overlap": ("DDIMSchedule", {}, 10, 5, True, MIC, None),
    "ddim_g5_serial": ("DDIMSchedule", {}, 10, 5, False, MIC, None),
    "ddim_g5_autoregressive": ("DDIMSchedule", {}, 10, 5, True, AR, None),
    "ddim_clip_eta0_g5": ("DDIMSchedule", {"clip_sample": True}, 10, 5, True, MIC, 0.0),
    "ddim_clip_eta05_g5": ("DDIMSchedule", {"clip_sample": True}, 10, 5, True, MIC, 0.5),
    "pndm_g1": ("PNDMSchedule", {"skip_prk_steps": True}, 9, 1, True, MIC, None),
    "pndm_g5": ("PNDMSchedule", {"skip_prk_steps": True}, 9, 5, True, MIC, None),
    "pndm_g1_autoregressive": ("PNDMSchedule", {"skip_prk_steps": True}, 9, 1, True, AR, None),
    "dpmpp2m_n10_g5": ("DPMSolverMultistepSchedule", _DPM2, 10, 5, True, MIC, None),
    "dpm3_heun_n20_g5": ("DPMSolverMultistepSchedule", _DPM3, 20, 5, True, MIC, None),
    "dpm3_heun_n20_g1_autoregressive": ("DPMSolverMultistepSchedule", _DPM3, 20, 1, True, AR, None),
}
# name -> (schedule class, its keywords, inference steps (10 UNet evaluations each), eta)
LOOPS = {
    "ddim": ("DDIMSchedule", {}, 10, 0.0),
    "ddim_eta_clip": ("DDIMSchedule", {"clip_sample": True}, 10, 0.5),
    "plms": ("PNDMSchedule", {"skip_prk_steps": True}, 9, 0.0),
    "dpm": ("DPMSolverMultistepSchedule", _DPM3, 10, 0.0),
}


def make_schedule(cls: str, kw: dict):
    import storygen_amd.scheduler as sch
    return getattr(sch, cls)(**kw)


def table_of(case):
    from storygen_amd.sampler import step_table
    cls, kw, n, G, overlap, stage, eta = case
    s = make_schedule(cls, kw)
    extra = {} if eta is None else {"eta": eta}
    rows, row0 = step_table(s, s.timesteps(n), n, UNITS0, R, stage, B, G, overlap, S_IMG, S_TXT, **extra)
    return {"rows": rows, "row0": row0}


def host_arithmetic_fingerprint() -> str:
    """sha256 over the schedules' numeric API on this machine (every add_noise_coef, the step / var_step coefficients and the PLMS /
    DPM-Solver rows of the cases' timesteps).  torch's vectorised fp32 CPU kernels (linspace, cumprod) round differently on CPUs
    with other vector units: 1 ulp in alphas_cumprod, measured between two x86 hosts.  A golden of floats is exact only on
    arithmetic with its recorder's fingerprint, so the file keeps one recording per fingerprint."""
    import hashlib
    vals = []
    for cls, kw, n, *_ in list(TABLES.values()):
        s = make_schedule(cls, kw)
        ts = s.timesteps(n)
        vals += [s.add_noise_coef(t) for t in range(s.num_train_timesteps)] + [s.step_row(k, ts, n) for k in range(len(ts))]
        if cls == "DDIMSchedule":
            vals += [s.var_step_coef(t, n, 0.5) for t in ts]
    return hashlib.sha256(repr(vals).encode()).hexdigest()


def table_from_api(case, golden):
    """The case's table assembled from the schedule's numeric API on this machine, in the layout and with the (integer, so
    machine-independent) timesteps of the golden one: what the golden holds on a machine whose fp32 host arithmetic rounds otherwise."""
    cls, kw, n, G, overlap, stage, eta = case
    s = make_schedule(cls, kw)
    ts, U = s.timesteps(n), G * len(UNITS0)

    def assemble(row, tail):
        tt = row[:U + B]
        assert all(float(t).is_integer() for t in tt)
        cc = [c for t in tt[:U] for c in s.add_noise_coef(int(t))]
        return tt + cc + tail
    var = eta is not None and (eta > 0 or s.clip_sample)
    tails = [[S_IMG, S_TXT] + ([*s.var_step_coef(ts[k], n, eta), float(s.clip_sample)] if var else s.step_row(k, ts, n)) for k in range(len(ts))]
    rows = [assemble(r, t) for r, t in zip(golden["rows"], tails)]
    return {"rows": rows, "row0": assemble(golden["row0"], [0.0] * len(tails[0]))}


def _state_buffers(smp) -> dict:
    """The fp32 buffers the sampler keeps for its update rule, by the rule's names for them."""
    state = getattr(smp, "rule_state", None)
    if state is None:        # the sampler before it held an UpdateRule (the commit tests/golden/step_tables.json was recorded from)
        state = {"history": getattr(smp, "eps_history", getattr(smp, "model_outputs", None)), "kept": getattr(smp, "kept_sample", None)}
    return {k: v for k, v in state.items() if v is not None}


def record_calls(case, G: int, patch=setattr):
    """The update-rule calls of one whole loop, [op name, *which buffer each rule-specific tensor argument is] per UNet
    evaluation, and the final latents (fp32 values as Python floats).  `patch(object, name, value)`: how storygen_amd.sampler is pointed at the stand-ins (a test passes
    monkeypatch.setattr)."""
    import fake_ops
    import stub_engine
    import storygen_amd.sampler as S
    from storygen_amd.arch import SD15_CONFIG, build_arch
    cls, kw, n, eta = case
    calls, smp = [], None

    def recorder(name):
        def call(eps3, latents, latents3, *rest):
            assert latents is smp.latents and latents3 is smp.latents3
            named = {v.data_ptr(): k for k, v in _state_buffers(smp).items()}
            if smp.var_noise is not None:
                named.update({smp.var_noise[g].data_ptr(): f"noise[{g}]" for g in range(smp.var_noise.shape[0])})
            calls.append([name] + [named[t.data_ptr()] for t in rest[:-1]])
            return getattr(fake_ops, name)(eps3, latents, latents3, *rest)
        return call

    patch(S, "UNetEngine", stub_engine.StubEngine)
    patch(S, "ops", types.SimpleNamespace(add_noise=stub_engine.add_noise, **{f: recorder(f) for f in
                                          ("cfg_ddim_step", "cfg_ddim_var_step", "cfg_plms_step", "cfg_dpm_step")}))
    N, hw, seq = 2, 4, 5
    g = torch.Generator().manual_seed(0)
    r = lambda *sh: torch.randn(*sh, generator=g)                                         # noqa: E731
    inp = dict(latents=r(N, 4, hw, hw), noise=r(N, 4, hw, hw), image_prompts=r(R, N, 4, hw, hw), zero_prompt=r(N, 4, hw, hw),
               text=r(N, seq, 8), uncond=r(N, seq, 8), prev_text=r(R, N, seq, 8), prev_uncond=r(1, N, seq, 8).expand(R, N, seq, 8).clone())
    smp = S.StoryGenSampler(build_arch(SD15_CONFIG), None, "cpu", N, hw, hw, R, seq, use_graph=False, weights=object(),
                            time_tables=False, ref_ahead=G, schedule=make_schedule(cls, kw))
    evals = len(smp.schedule.timesteps(n))
    noise = torch.randn(evals, N, 4, hw, hw, generator=g) if eta > 0 else None
    smp.prepare(inp, n, MIC, S_TXT, S_IMG, eta=eta, variance_noise=noise)
    smp.run()
    assert len(calls) == evals == 10 and torch.isfinite(smp.latents).all()
    return {"calls": calls, "latents": smp.latents.flatten().tolist()}


# ------------------------------------------------------------------------------------------------ the kernels (tests/test_update_rules_gpu.py)
KERNEL_TOTALS = (252, 512, 307200)      # N * n: not a multiple of the block; two blocks; more than 1024 x 256 threads (the loop wraps)
KERNEL_N = 2


def kernel_coef(rule: str) -> torch.Tensor:
    """One mid-trajectory row per rule behind the two guidance scales: PLMS with all four weights and a push, DPM-Solver at order 3,
    the eta rule with std != 0 and clipping on."""
    from storygen_amd.scheduler import DDIMSchedule
    if rule in ("ddim", "ddim_var"):
        s = DDIMSchedule(clip_sample=rule == "ddim_var")
        t = s.timesteps(10)[5]
        row = list(s.step_coef(t, 10)) if rule == "ddim" else [*s.var_step_coef(t, 10, 0.5), 1.0]
        assert rule == "ddim" or row[4] != 0.0
    elif rule == "plms":
        s = make_schedule("PNDMSchedule", {"skip_prk_steps": True})
        row = s.step_row(6, s.timesteps(9), 9)
        assert all(w != 0.0 for w in row[2:6]) and row[10] == 1.0
    else:
        s = make_schedule("DPMSolverMultistepSchedule", _DPM3)
        row = s.step_row(5, s.timesteps(20), 20)
        assert s.order_at(5, 20) == 3 and all(w != 0.0 for w in row[3:6])
    return torch.tensor([S_IMG, S_TXT, *row], dtype=torch.float32)


_BASE = {}


def kernel_case(total: int) -> dict:
    """Seeded fp32 inputs of `total` elements per tensor: the first `total` of ONE draw, whatever the size (made once, on the CPU)."""
    if not _BASE:
        g = torch.Generator().manual_seed(12)
        m = max(KERNEL_TOTALS)
        for name, k in (("eps3", 3), ("latents", 1), ("noise", 1), ("history", 4), ("kept", 1)):
            _BASE[name] = torch.randn(k, m, generator=g)
    return {k: v[:, :total].clone() for k, v in _BASE.items()}


def run_kernel(ops, rule: str, total: int, with_lat3: bool, device) -> dict:
    """One call of the rule's wrapper on kernel_case(total); returns every tensor the kernel may write, on the CPU."""
    c = {k: v.to(device) for k, v in kernel_case(total).items()}
    n = total // KERNEL_N
    lat = c["latents"].view(KERNEL_N, n)
    eps3 = c["eps3"].view(3 * KERNEL_N, n)
    lat3 = torch.zeros(3 * KERNEL_N, n, device=device) if with_lat3 else None
    coef = kernel_coef(rule).to(device)
    out = {"latents": lat}
    if rule == "ddim":
        ops.cfg_ddim_step(eps3, lat, lat3, coef)
    elif rule == "ddim_var":
        ops.cfg_ddim_var_step(eps3, lat, lat3, c["noise"].view(KERNEL_N, n), coef)
    elif rule == "plms":
        hist, kept = c["history"].view(4, KERNEL_N, n), c["kept"].view(KERNEL_N, n)
        ops.cfg_plms_step(eps3, lat, lat3, hist, kept, coef)
        out.update(history=hist, kept=kept)
    else:
        hist = c["history"][:3].contiguous().view(3, KERNEL_N, n)
        ops.cfg_dpm_step(eps3, lat, lat3, hist, coef)
        out["history"] = hist
    if with_lat3:
        out["latents3"] = lat3
    return {k: v.cpu() for k, v in out.items()}
