"""Stochastic (eta > 0) and clipped DDIM, host side: DDIMSchedule.var_step_coef against the clean-room shim's DDIMScheduler (the
restatement of diffusers 0.13.1 the oracle steps with), the clip_sample config round trip, and the order in which the drop-in
pipeline draws the variance noise (the reference's `scheduler.step(..., eta=eta, generator=generator)`, pipeline.py:461)."""
import json

import pytest
import torch

from ddim_eta_helpers import RecordingSampler, cpu_call, cpu_pipeline, reference_order_noise, shim_ddim, ulp32


# ------------------------------------------------------------------------------------------------ the coefficients
@pytest.mark.parametrize("alpha_to_one", [False, True])
@pytest.mark.parametrize("n", [50, 20, 7])
def test_var_step_coef_vs_shim_scheduler(n, alpha_to_one):
    """Every step of the n-step schedule, eta in {0, 0.3, 1}: std = eta sqrt(_get_variance) and dir = sqrt(1 - abar_prev - std^2) as
    the shim computes them, within 2 fp32 ulp (both are the same fp32 tensor formula; measured: 0 ulp).  eta = 0 is step_coef, exactly,
    with std = 0; the first three scalars never depend on eta."""
    from storygen_amd.scheduler import DDIMSchedule
    s = DDIMSchedule(set_alpha_to_one=alpha_to_one)
    ref = shim_ddim(n, set_alpha_to_one=alpha_to_one)
    ts = s.timesteps(n)
    assert ts == ref.timesteps.tolist()
    worst = 0.0
    for eta in (0.0, 0.3, 1.0):
        for t in ts:
            prev = t - 1000 // n
            a_p = ref.alphas_cumprod[prev] if prev >= 0 else ref.final_alpha_cumprod
            std_ref = eta * ref._get_variance(t, prev) ** 0.5
            dir_ref = (1 - a_p - std_ref ** 2) ** 0.5
            sa, sb, sap, dirc, std = s.var_step_coef(t, n, eta)
            assert (sa, sb, sap) == s.step_coef(t, n)[:3]
            for got, want in ((std, float(std_ref)), (dirc, float(dir_ref))):
                assert got == got and want == want, (n, eta, t)
                gap = abs(got - want) / ulp32(max(abs(want), 1e-30))
                worst = max(worst, gap)
                assert gap <= 2.0, (n, eta, t, got, want)
            if eta == 0.0:
                assert (sa, sb, sap, dirc) == s.step_coef(t, n) and std == 0.0
            else:
                assert std > 0.0 or (alpha_to_one and prev < 0)       # the last step onto abar = 1 has zero variance
    print(f"var_step_coef vs shim, n = {n}, set_alpha_to_one = {alpha_to_one}: worst gap {worst} ulp")
    assert s.var_step_coef(ts[0], n, 0.3) is s.var_step_coef(ts[0], n, 0.3)        # memoised like step_coef


# ------------------------------------------------------------------------------------------------ the config
def test_clip_sample_config_round_trip(tmp_path):
    from storygen_amd.scheduler import DDIMSchedule, schedule_from_config
    s = DDIMSchedule(clip_sample=True)
    assert s.clip_sample is True and s.config["clip_sample"] is True and s.key() != DDIMSchedule().key()
    s.save_pretrained(str(tmp_path))
    saved = json.loads((tmp_path / "scheduler_config.json").read_text())
    assert saved["_class_name"] == "DDIMScheduler" and saved["clip_sample"] is True
    back = DDIMSchedule.from_pretrained(str(tmp_path), subfolder=None)
    assert back.clip_sample is True and back.key() == s.key()
    assert DDIMSchedule().clip_sample is False and DDIMSchedule().config["clip_sample"] is False


def test_stock_diffusers_ddim_config_loads():
    """A scheduler_config.json written by stock diffusers' DDIMScheduler (clip_sample defaults to true there) is what
    inference.py:48 loads; the same keys must give the clipping schedule here, as a dict and as an attribute object."""
    from types import SimpleNamespace
    from storygen_amd.scheduler import DDIMSchedule, PNDMSchedule, schedule_from_config
    cfg = {"_class_name": "DDIMScheduler", "_diffusers_version": "0.13.1", "beta_end": 0.012, "beta_schedule": "scaled_linear",
           "beta_start": 0.00085, "clip_sample": True, "num_train_timesteps": 1000, "prediction_type": "epsilon",
           "set_alpha_to_one": False, "steps_offset": 1, "trained_betas": None}
    for c in (cfg, SimpleNamespace(**cfg)):
        s = schedule_from_config(c)
        assert type(s) is DDIMSchedule and s.clip_sample is True and s.key() == DDIMSchedule(clip_sample=True).key()
    # PNDM has no such key: the shipped PNDM config read as PNDM stays unclipped
    p = schedule_from_config(dict(cfg, _class_name="PNDMScheduler", skip_prk_steps=True))
    assert type(p) is PNDMSchedule and p.clip_sample is False and "clip_sample" not in p.config


def test_step_table_rows_of_the_eta_path():
    """step_table(eta=...) rows end in [s_img, s_txt, sa, sb, sap, dir, std, clip]; without eta they are what they were."""
    from storygen_amd.sampler import step_table
    from storygen_amd.scheduler import DDIMSchedule
    units0 = [(0, 0, 0), (1, 0, 0), (1, 1, 0)]
    for clip in (False, True):
        s = DDIMSchedule(clip_sample=clip)
        ts = s.timesteps(10)
        base, base0 = step_table(s, ts, 10, units0, 2, "multi-image-condition", 3, 5, True, 3.5, 7.5)
        rows, row0 = step_table(s, ts, 10, units0, 2, "multi-image-condition", 3, 5, True, 3.5, 7.5, eta=0.5)
        assert len(rows) == 10 and all(len(r) == len(base[0]) + 2 for r in rows) and len(row0) == len(base0) + 2
        for k, (r, b) in enumerate(zip(rows, base)):
            assert r[:-8] == b[:-6] and r[-8:-6] == [3.5, 7.5]
            assert tuple(r[-6:-1]) == s.var_step_coef(ts[k], 10, 0.5) and r[-1] == float(clip)
            assert tuple(b[-4:]) == s.step_coef(ts[k], 10)


# ------------------------------------------------------------------------------------------------ the pipeline's draws
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_pipeline_draws_variance_noise_in_reference_order_one_generator(monkeypatch, dtype):
    from storygen_amd.scheduler import DDIMSchedule
    pipe = cpu_pipeline(monkeypatch, DDIMSchedule(), dtype)
    g = torch.Generator().manual_seed(1234)
    cpu_call(pipe, 1, 10, eta=0.7, generator=g)
    (smp,) = RecordingSampler.made
    (kw,) = smp.prepared
    assert kw["eta"] == 0.7 and smp.G == 5
    # the reference: prepare_latents draws [1, 4, 8, 8] first, then every step one more of the same shape
    want = reference_order_noise(1234, 11, (1, 4, 8, 8), dtype)
    assert kw["variance_noise"].dtype == dtype and torch.equal(kw["variance_noise"], want[1:])
    assert torch.equal(smp.latents, want[0].float())
    fresh = torch.Generator().manual_seed(1234)
    for _ in range(11):
        torch.randn((1, 4, 8, 8), generator=fresh, dtype=dtype)
    assert torch.equal(g.get_state(), fresh.get_state())


def test_pipeline_draws_variance_noise_in_reference_order_generator_list(monkeypatch):
    from storygen_amd.scheduler import DDIMSchedule
    pipe = cpu_pipeline(monkeypatch, DDIMSchedule())
    gens = [torch.Generator().manual_seed(7), torch.Generator().manual_seed(8)]
    cpu_call(pipe, 2, 5, eta=1.0, generator=gens)
    (kw,) = RecordingSampler.made[0].prepared
    want = reference_order_noise([7, 8], 6, (2, 4, 8, 8))
    assert kw["variance_noise"].shape == (5, 2, 4, 8, 8) and torch.equal(kw["variance_noise"], want[1:])
    # not one [steps, ...] draw per generator: Philox / mt19937 streams give other values for that
    assert torch.equal(RecordingSampler.made[0].latents, want[0])


def test_pipeline_eta_zero_and_pndm_draw_nothing(monkeypatch):
    """eta = 0 consumes the generator exactly as before the eta path existed (prepare_latents' one draw) and hands prepare() eta = 0
    and no noise; PNDM and DPM-Solver ignore eta (prepare_extra_step_kwargs forwards it only to schedulers whose step takes it)."""
    from storygen_amd.scheduler import DDIMSchedule, DPMSolverMultistepSchedule, PNDMSchedule
    after_latents = torch.Generator().manual_seed(99)
    torch.randn((1, 4, 8, 8), generator=after_latents)
    for sched, eta, steps in ((DDIMSchedule(), 0.0, 10), (PNDMSchedule(skip_prk_steps=True), 0.5, 9),
                              (DPMSolverMultistepSchedule(), 0.5, 10)):
        pipe = cpu_pipeline(monkeypatch, sched)
        g = torch.Generator().manual_seed(99)
        cpu_call(pipe, 1, steps, eta=eta, generator=g)
        (kw,) = RecordingSampler.made[0].prepared
        assert kw == {"steps": steps, "eta": 0.0, "variance_noise": None}, (type(sched).__name__, kw)
        assert torch.equal(g.get_state(), after_latents.get_state()), type(sched).__name__


def test_pipeline_sampler_cache_key_has_eta_and_clip_sample(monkeypatch):
    from storygen_amd.scheduler import DDIMSchedule
    pipe = cpu_pipeline(monkeypatch, DDIMSchedule())
    g = torch.Generator().manual_seed(0)
    cpu_call(pipe, 1, 5, generator=g)
    cpu_call(pipe, 1, 5, generator=g)
    assert len(RecordingSampler.made) == 1
    cpu_call(pipe, 1, 5, eta=0.5, generator=g)
    cpu_call(pipe, 1, 5, eta=0.5, generator=g)
    assert len(RecordingSampler.made) == 2
    cpu_call(pipe, 1, 5, eta=0.25, generator=g)
    assert len(RecordingSampler.made) == 3
    pipe.scheduler = DDIMSchedule(clip_sample=True)
    cpu_call(pipe, 1, 5, generator=g)
    assert len(RecordingSampler.made) == 4
    (kw,) = RecordingSampler.made[3].prepared
    assert kw["eta"] == 0.0 and kw["variance_noise"] is None      # the clipping schedule runs the eta path's kernel without noise


# ------------------------------------------------------------------------------------------------ the sampler's schedules
def _stub_inputs(N, R, hw=4, S=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *sh: torch.randn(*sh, generator=g)                                         # noqa: E731
    return dict(latents=r(N, 4, hw, hw), noise=r(N, 4, hw, hw), image_prompts=r(R, N, 4, hw, hw), zero_prompt=r(N, 4, hw, hw),
                text=r(N, S, 8), uncond=r(N, S, 8), prev_text=r(R, N, S, 8), prev_uncond=r(1, N, S, 8).expand(R, N, S, 8).clone())


@pytest.mark.parametrize("clip", [False, True])
def test_sampler_eta_path_on_the_stand_in_engine(monkeypatch, clip):
    """The sampler's bookkeeping of the eta path without a GPU (tests/stub_engine.py's engine, the update rule in torch): every step
    of the group schedule (G = 5) gets the noise and the table row the step-by-step loop gives it — latents bit-identical after
    every step —; another variance_noise on the same sampler changes the trajectory; eta = 0 without clipping never reaches the new
    op (the stand-in ops namespace of the default path has no such entry) and leaves the default trajectory as it is."""
    import stub_engine
    from ddim_eta_helpers import cfg_ddim_var_step
    from storygen_amd.arch import build_arch
    from storygen_amd.scheduler import DDIMSchedule, PNDMSchedule
    from test_oracle_golden import _load
    S = stub_engine.install(monkeypatch)
    calls = []

    def var_step(eps3, latents, latents3, noise, coef):
        calls.append((noise.clone(), coef.clone()))
        return cfg_ddim_var_step(eps3, latents, latents3, noise, coef)

    arch = build_arch(_load("tiny")["config"])
    N, R, T = 2, 2, 10
    inp = _stub_inputs(N, R)
    noise = reference_order_noise(3, T, (N, 4, 4, 4))

    def run(smp, **kw):
        smp.prepare(inp, T, "multi-image-condition", 7.5, 3.5, **kw)
        tr = []
        smp.run(trace=tr)
        return tr

    def make(G, sched=None):
        return S.StoryGenSampler(arch, None, "cpu", N, 4, 4, R, 5, use_graph=False, weights=object(), time_tables=False, ref_ahead=G,
                                 schedule=sched or DDIMSchedule(clip_sample=clip))

    step, group = make(1), make(5)
    if not clip:
        default = run(step)                                   # no cfg_ddim_var_step in the namespace yet: reaching it would raise
        assert all(torch.equal(a, b) for a, b in zip(run(step, eta=0.0), default)) and step.var is False
    monkeypatch.setattr(S.ops, "cfg_ddim_var_step", var_step, raising=False)
    want = run(step, eta=0.5, variance_noise=noise)
    assert step.var and len(calls) == T
    sched = step.schedule
    for k, (z, c) in enumerate(calls):
        assert torch.equal(z, noise[k]) and c[-1] == float(clip)
        assert [float(v) for v in c[2:7]] == [float(torch.tensor(v, dtype=torch.float32)) for v in
                                              sched.var_step_coef(step.timesteps[k], T, 0.5)]
    got = run(group, eta=0.5, variance_noise=noise)
    assert group.group and len(got) == T and all(torch.equal(a, b) for a, b in zip(got, want))
    other = run(group, eta=0.5, variance_noise=reference_order_noise(4, T, (N, 4, 4, 4)))
    assert not torch.equal(other[0], want[0]) and not torch.equal(other[-1], want[-1])
    assert all(torch.equal(a, b) for a, b in zip(run(group, eta=0.5, variance_noise=noise), want))
    with pytest.raises(ValueError, match="variance_noise"):
        step.prepare(inp, T, "multi-image-condition", 7.5, 3.5, eta=0.5)
    with pytest.raises(ValueError, match="variance_noise"):
        step.prepare(inp, T, "multi-image-condition", 7.5, 3.5, eta=0.5, variance_noise=noise[:-1])
    with pytest.raises(ValueError, match="eta"):
        step.prepare(inp, T, "multi-image-condition", 7.5, 3.5, eta=-0.1)
    if clip:                                                  # the clipping schedule takes the new kernel at eta = 0 too, std = 0
        calls.clear()
        run(step)
        assert len(calls) == T and all(float(c[6]) == 0.0 and float(c[7]) == 1.0 for _, c in calls)
    # PNDM ignores eta, as the reference's prepare_extra_step_kwargs does
    monkeypatch.setattr(S.ops, "cfg_plms_step", lambda eps3, lat, lat3, hist, kept, coef: lat, raising=False)
    p = make(1, PNDMSchedule(skip_prk_steps=True))
    p.prepare(inp, 9, "multi-image-condition", 7.5, 3.5, eta=0.5)
    assert p.var is False and p.eta == 0.0
