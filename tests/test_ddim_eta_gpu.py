"""Stochastic (eta > 0) and clipped DDIM on the GPU: the update kernel sg_cfg_ddim_var_step_f32 against the clean-room shim's
`DDIMScheduler.step` (diffusers 0.13.1 restated; fp32 on the CPU, variance noise passed explicitly), the sampler's step-by-step and
group schedules on it, and the drop-in pipeline's `eta` / a clipping scheduler.

Bars (set before the first GPU run, figures in profiles/r11a_ddim_eta.txt):
  * kernel: max abs error <= 4 fp32 ulp of the largest term.  "Term" = every addend of the update carried to the output's scale:
    with g = max(|dir|, sap sb / sa) the gain of the guided epsilon, the terms are g |e_u|, g |s_img (e_i - e_u)|, g |s_txt (e_a - e_i)|,
    (sap / sa) |x|, (sap sb / sa) |eps|, |dir eps| and |std noise|; the bar is 4 ulp of the largest of them over the tensor.
  * group path (G = 5) against one graph per step at eta = 0.5: 2 x the deviation the PARENT commit shows between the same two
    paths at eta = 0 on the same inputs (the two schedules tile the batched reference pass differently; the variance term adds the
    same noise to both).
  * step trace: every x_{t-1} within 1e-6 (max abs error over max abs value) of the shim's step on the recorded (eps, x_t, noise_k).
Measured on MI355X: kernel 2.38 ulp at worst, group against step path 1.609e-3 (parent at eta = 0: 1.4953e-3, bar 2.99e-3), step trace
2.2e-7 at worst."""
import pytest
import torch

from conftest import max_rel, rel_l2
from ddim_eta_helpers import S_IMG, S_TXT, guided, reference_order_noise, shim_ddim, ulp32

pytestmark = pytest.mark.gpu

STAGE, GUIDANCE, STEPS = "multi-image-condition", (7.5, 3.5), 10
# rel-L2 between the G = 5 and the one-graph-per-step trajectories (worst of the 10 steps) of the PARENT commit at eta = 0, on
# this file's inputs (profiles/r11a_ddim_eta.txt)
PARENT_GROUP_VS_STEP = 1.4953e-3
SIZES = [(1, 1), (1, 255), (1, 256), (1, 257), (2, 1024 * 256 + 3), (3, 4 * 32 * 32)]


# ------------------------------------------------------------------------------------------------ the kernel
def _kernel_case(N, n, t, eta, clip, seed):
    """Inputs, coefficients and the shim's result for one launch.  In the clipped cases the inputs are scaled so that the median
    |x0| is 1 (x0 is linear in (x, eps)): half the elements clamp.  A single element cannot be half clamped: N x n = 1 x 1 runs
    once clamped (|x0| = 2) and once not (|x0| = 0.5), chosen by the seed's parity."""
    from storygen_amd.scheduler import DDIMSchedule
    g = torch.Generator().manual_seed(seed)
    eps3, x, noise = torch.randn(3 * N, n, generator=g), torch.randn(N, n, generator=g), torch.randn(N, n, generator=g)
    ref = shim_ddim(50, clip_sample=bool(clip))
    sa, sb, sap, dirc, std = DDIMSchedule(clip_sample=bool(clip)).var_step_coef(t, 50, eta)
    if clip:
        x0 = (x - sb * guided(eps3, N)) / sa
        scale = 1.0 / float(x0.abs().median()) if N * n > 1 else (2.0 if seed % 2 else 0.5) / float(x0.abs())
        eps3, x = eps3 * scale, x * scale
    eps = guided(eps3, N)
    x0 = (x - sb * eps) / sa
    want = ref.step(eps, t, x, eta=eta, variance_noise=noise if eta > 0 else None).prev_sample
    gain = max(abs(dirc), sap * sb / sa)
    eu, ei, ea = eps3.chunk(3)
    terms = [gain * eu.abs().max(), gain * (S_IMG * (ei - eu)).abs().max(), gain * (S_TXT * (ea - ei)).abs().max(),
             sap / sa * x.abs().max(), sap * sb / sa * eps.abs().max(), (dirc * eps).abs().max(), (std * noise).abs().max()]
    coef = torch.tensor([S_IMG, S_TXT, sa, sb, sap, dirc, std, float(clip)], dtype=torch.float32)
    return eps3, x, noise, coef, want, float(max(terms)), float((x0.abs() > 1).float().mean())


@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("N,n", SIZES)
def test_cfg_ddim_var_step_kernel_vs_shim_step(gpu, N, n, eta, clip):
    """ops.cfg_ddim_var_step against the shim's DDIMScheduler.step at the first, a middle and the last timestep of the 50-step
    schedule (the last one steps onto final_alpha_cumprod), with latents3 null and non-null."""
    from storygen_amd import ops
    worst = 0.0
    for j, t in enumerate((981, 481, 1)):
        eps3, x, noise, coef, want, largest, frac = _kernel_case(N, n, t, eta, clip, seed=17 * n + j)
        if clip and N * n > 1:
            assert 0.2 <= frac <= 0.8, (t, frac)
        elif clip:
            assert frac == float((17 * n + j) % 2)
        bar = 4.0 * ulp32(largest)
        for with_lat3 in (False, True):
            lat = x.to(gpu)
            lat3 = torch.full((3 * N, n), -7.0, device=gpu) if with_lat3 else None
            ops.cfg_ddim_var_step(eps3.to(gpu), lat, lat3, noise.to(gpu), coef.to(gpu))
            torch.cuda.synchronize()
            got = lat.cpu()
            err = float((got - want).abs().max())
            worst = max(worst, err / ulp32(largest))
            assert torch.isfinite(got).all() and err <= bar, (t, with_lat3, err, bar)
            if with_lat3:
                assert torch.equal(lat3.cpu().view(torch.int32), torch.cat([got] * 3).view(torch.int32))
    print(f"cfg_ddim_var_step N={N} n={n} eta={eta} clip={clip}: worst error {worst:.2f} ulp of the largest term")


@pytest.mark.parametrize("N,n", SIZES)
def test_cfg_ddim_var_step_is_cfg_ddim_step_at_eta0_unclipped(gpu, N, n):
    """std = 0, clip = 0: bit for bit sg_cfg_ddim_step_f32 on the same inputs (with and without a noise tensor)."""
    from storygen_amd import ops
    from storygen_amd.scheduler import DDIMSchedule
    s = DDIMSchedule()
    for j, t in enumerate((981, 481, 1)):
        eps3, x, noise, coef, _, _, _ = _kernel_case(N, n, t, 0.0, 0, seed=5 * n + j)
        assert tuple(float(v) for v in coef[2:6]) == tuple(float(torch.tensor(v, dtype=torch.float32)) for v in s.step_coef(t, 50))
        a, a3 = x.to(gpu), torch.zeros(3 * N, n, device=gpu)
        ops.cfg_ddim_step(eps3.to(gpu), a, a3, coef[:6].contiguous().to(gpu))
        for z in (noise.to(gpu), None):
            b, b3 = x.to(gpu), torch.zeros(3 * N, n, device=gpu)
            ops.cfg_ddim_var_step(eps3.to(gpu), b, b3, z, coef.to(gpu))
            torch.cuda.synchronize()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a3.view(torch.int32), b3.view(torch.int32))


def test_cfg_ddim_var_step_refuses_null_noise_with_std(gpu):
    """A null noise pointer with std > 0 is SG_EINVAL before anything is launched (the latents stay untouched); so are null tensors
    and empty shapes."""
    from storygen_amd import _lib, ops
    lib = _lib.load()
    eps3, x, noise, coef, _, _, _ = _kernel_case(1, 256, 481, 0.5, 0, seed=1)
    e, lat, c = eps3.to(gpu), x.to(gpu), coef.to(gpu)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.sg_cfg_ddim_var_step_f32(e.data_ptr(), lat.data_ptr(), None, None, c.data_ptr(), 1, 256, st) == -1
    assert b"noise is null" in lib.sg_last_error()
    torch.cuda.synchronize()
    assert torch.equal(lat.cpu(), x)
    with pytest.raises(Exception, match="noise is null"):
        ops.cfg_ddim_var_step(e, lat, None, None, c)
    z = noise.to(gpu)
    assert lib.sg_cfg_ddim_var_step_f32(None, lat.data_ptr(), None, z.data_ptr(), c.data_ptr(), 1, 256, st) == -1
    assert lib.sg_cfg_ddim_var_step_f32(e.data_ptr(), None, None, z.data_ptr(), c.data_ptr(), 1, 256, st) == -1
    assert lib.sg_cfg_ddim_var_step_f32(e.data_ptr(), lat.data_ptr(), None, z.data_ptr(), None, 1, 256, st) == -1
    assert lib.sg_cfg_ddim_var_step_f32(e.data_ptr(), lat.data_ptr(), None, z.data_ptr(), c.data_ptr(), 0, 256, st) == -1
    assert lib.sg_cfg_ddim_var_step_f32(e.data_ptr(), lat.data_ptr(), None, z.data_ptr(), c.data_ptr(), 1, 0, st) == -1
    with pytest.raises(ValueError):
        ops.cfg_ddim_var_step(e, lat, None, z, c[:6].contiguous())
    with pytest.raises(ValueError):
        ops.cfg_ddim_var_step(e, lat, None, z[:, :255].contiguous(), c)
    torch.cuda.synchronize()
    assert torch.equal(lat.cpu(), x)


# ------------------------------------------------------------------------------------------------ the sampler
@pytest.fixture(scope="module")
def model(gpu):
    from storygen_amd.arch import SD15_CONFIG, build_arch
    from storygen_amd.model import UNet2DConditionModel
    from storygen_amd.synth import synthetic_state_dict
    arch = build_arch(SD15_CONFIG)
    m = UNet2DConditionModel.from_config(SD15_CONFIG)
    m.load_state_dict(synthetic_state_dict(arch, 0))
    return m.to(gpu, torch.float16).eval(), arch


@pytest.fixture(scope="module")
def inputs32():
    from storygen_amd.synth import synthetic_inputs
    return synthetic_inputs(1, 2, 32, 32, 9, 768)


def _sampler(model, gpu, G, schedule=None):
    from storygen_amd.sampler import StoryGenSampler
    unet, arch = model
    return StoryGenSampler(arch, None, gpu, 1, 32, 32, 2, schedule=schedule, weights=unet._engine_weights(), ref_ahead=G)


@pytest.fixture(scope="module")
def sampler_runs(gpu, model, inputs32):
    """Every sampler run the tests below look at (32x32 latent, R = 2, 10 steps, SD-1.5 UNet with synthetic weights), made once."""
    r = {}
    noise = reference_order_noise(41, STEPS, (1, 4, 32, 32))
    noise2 = reference_order_noise(42, STEPS, (1, 4, 32, 32))
    step = _sampler(model, gpu, 1)
    step.prepare(inputs32, STEPS, STAGE, *GUIDANCE)
    r["default"] = step.run().cpu()
    step.prepare(inputs32, STEPS, STAGE, *GUIDANCE, eta=0.0)
    r["eta0"] = step.run().cpu()
    r["eta0_var"] = step.var
    # one graph per step at eta = 0.5, recording (x_t, eps3, x_{t-1}) of every step
    step.prepare(inputs32, STEPS, STAGE, *GUIDANCE, eta=0.5, variance_noise=noise)
    trace = []
    for k in range(STEPS):
        x_t = step.latents.clone()
        step.step(k)
        trace.append((x_t.cpu(), step.main.eps_out.clone().cpu(), step.latents.clone().cpu()))
    torch.cuda.synchronize()
    r["trace"] = trace
    step.check_guards()
    group = _sampler(model, gpu, 5)
    group.prepare(inputs32, STEPS, STAGE, *GUIDANCE, eta=0.5, variance_noise=noise)
    got = []
    group.run(trace=got)
    r["group"] = [g.cpu() for g in got]
    r["group_is_group"] = group.group and bool(group.graphs)
    graphs = list(group.graphs)
    group.prepare(inputs32, STEPS, STAGE, *GUIDANCE, eta=0.5, variance_noise=noise2)
    r["graphs_kept"] = len(graphs) == len(group.graphs) and all(a is b for a, b in zip(graphs, group.graphs))
    r["group_noise2"] = group.run().cpu()
    group.check_guards()
    fresh = _sampler(model, gpu, 5)
    fresh.prepare(inputs32, STEPS, STAGE, *GUIDANCE, eta=0.5, variance_noise=noise2)
    r["fresh_noise2"] = fresh.run().cpu()
    r["noise"] = noise
    return r


def test_sampler_eta0_is_the_default_path(sampler_runs):
    """prepare(eta=0.0) on the unclipped schedule is prepare(): the same kernel, table and graphs, bit-identical latents."""
    assert sampler_runs["eta0_var"] is False
    assert torch.equal(sampler_runs["default"].view(torch.int32), sampler_runs["eta0"].view(torch.int32))


def test_sampler_group_path_vs_step_path_at_eta_half(sampler_runs):
    """G = 5 (one graph per group, five update launches reading five rows of the staged noise) against one graph per step, the same
    variance noise: worst rel-L2 over the 10 steps within 2 x what the parent commit's two paths differ by at eta = 0."""
    r = sampler_runs
    assert r["group_is_group"] and len(r["group"]) == STEPS
    errs = [rel_l2(g, t[2]) for g, t in zip(r["group"], r["trace"])]
    print(f"group vs step at eta = 0.5: worst {max(errs):.3e}, final {errs[-1]:.3e}; parent at eta = 0: {PARENT_GROUP_VS_STEP:.3e}")
    assert max(errs) <= 2.0 * PARENT_GROUP_VS_STEP, errs


def test_sampler_step_trace_vs_shim_step(sampler_runs):
    """Every step of the one-graph-per-step run: the shim's DDIMScheduler.step on the recorded guided epsilon, x_t and the step's
    noise gives the recorded x_{t-1} within 1e-6 relative (fp32 elementwise arithmetic, compared per step)."""
    r = sampler_runs
    ref = shim_ddim(STEPS)
    errs = []
    for k, (x_t, eps3, x_next) in enumerate(r["trace"]):
        t = int(ref.timesteps[k])
        want = ref.step(guided(eps3, 1), t, x_t, eta=0.5, variance_noise=r["noise"][k]).prev_sample
        errs.append(max_rel(x_next, want))
    print("step trace vs shim step, max abs error / max abs value per step:", [f"{e:.1e}" for e in errs])
    assert len(errs) == STEPS and max(errs) <= 1e-6, errs
    assert not torch.equal(r["trace"][-1][2], r["eta0"])            # and the noise did move the trajectory


def test_sampler_prepare_with_other_noise_replays_the_same_graphs(sampler_runs):
    """A second prepare() with another variance_noise keeps the captured graphs (they read the persistent staging buffer) and runs
    on the new noise: other latents than the first run, the latents of a fresh sampler given that noise."""
    r = sampler_runs
    assert r["graphs_kept"]
    assert not torch.equal(r["group_noise2"], r["group"][-1])
    assert torch.equal(r["group_noise2"].view(torch.int32), r["fresh_noise2"].view(torch.int32))


# ------------------------------------------------------------------------------------------------ the drop-in pipeline
@pytest.fixture(scope="module")
def pipeline_runs(gpu, model, inputs32):
    from test_dropin_gpu import _call, _table_pipeline
    from storygen_amd.scheduler import DDIMSchedule
    unet, arch = model
    R, hw = 2, 32
    r = {}

    def run(pipe, vae, **kw):
        vae.queue = [inputs32["zero_prompt"].to(gpu)] + [inputs32["image_prompts"][i].to(gpu) for i in range(R)]
        return _call(pipe, inputs32, R, hw, STEPS, GUIDANCE, STAGE, inputs32["latents"].to(gpu), **kw).images.float().cpu()

    pipe, vae = _table_pipeline(unet, inputs32, R, gpu, DDIMSchedule(), torch.float32)
    pipe.set_progress_bar_config(disable=True)
    r["eta07_a"] = run(pipe, vae, eta=0.7, generator=torch.Generator().manual_seed(5))
    r["G"] = pipe._sampler.G
    r["eta07_b"] = run(pipe, vae, eta=0.7, generator=torch.Generator().manual_seed(5))
    r["eta07_other_seed"] = run(pipe, vae, eta=0.7, generator=torch.Generator().manual_seed(6))
    r["eta0"] = run(pipe, vae, generator=torch.Generator().manual_seed(5))
    # what the pipeline hands its sampler: the stand-in VAE's latents went through `/ 0.18215` and `* 0.18215` on the device
    seen = dict(inputs32, zero_prompt=(inputs32["zero_prompt"].to(gpu) / 0.18215) * 0.18215,
                image_prompts=torch.stack([(inputs32["image_prompts"][i].to(gpu) / 0.18215) * 0.18215 for i in range(R)]))
    direct = _sampler(model, gpu, 5)
    # `latents=` is given, so prepare_latents draws nothing: the generator's first draws are the variance noise
    direct.prepare(seen, STEPS, STAGE, *GUIDANCE, eta=0.7, variance_noise=reference_order_noise(5, STEPS, (1, 4, hw, hw)))
    r["direct"] = direct.run().float().cpu()
    clip_pipe, clip_vae = _table_pipeline(unet, inputs32, R, gpu, DDIMSchedule(clip_sample=True), torch.float32)
    clip_pipe.set_progress_bar_config(disable=True)
    r["clip"] = run(clip_pipe, clip_vae)
    r["clip_var"] = clip_pipe._sampler.var
    return r


def test_pipeline_eta_runs_reproducibly_and_matches_the_sampler(pipeline_runs):
    r = pipeline_runs
    assert r["G"] == 5 and torch.isfinite(r["eta07_a"]).all()
    assert torch.equal(r["eta07_a"], r["eta07_b"])                    # same seed
    assert not torch.equal(r["eta07_a"], r["eta07_other_seed"])
    assert not torch.equal(r["eta07_a"], r["eta0"])
    assert torch.equal(r["eta07_a"].view(torch.int32), r["direct"].view(torch.int32))


def test_pipeline_with_a_clipping_ddim_schedule(pipeline_runs):
    r = pipeline_runs
    assert r["clip_var"] is True and torch.isfinite(r["clip"]).all()
    assert not torch.equal(r["clip"], r["eta0"])
