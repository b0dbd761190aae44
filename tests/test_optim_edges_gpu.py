"""The three kernels of storygen_amd/csrc/optim.hip (sg_sumsq_f32, sg_adamw_f32, sg_adamw8bit) at their block, clip, scale and step
edges, against the float64 reference of tests/optim_reference.py (pinned on the CPU by tests/test_optim_reference.py) and
oracle/optim_oracle.py.  The fp32 bars are not constants: each case runs torch.optim.AdamW (or the oracle pinned to it) in fp32 on
the CPU on the same inputs and allows the kernel 4x that implementation's distance from float64, floored at 2 ulp of the largest
parameter — room for fused multiply-adds and sqrtf / division rounding between two correct fp32 implementations."""
import ctypes as C
import functools

import pytest
import torch

import optim_reference as R
from conftest import rel_l2
from oracle import optim_oracle as oo

pytestmark = pytest.mark.gpu
F32 = torch.float32
DEFAULT_HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
HP_SETS = {
    "reference": dict(R.REFERENCE_HP),
    "b.5_.9_eps1e-6_wd0": dict(lr=1e-3, betas=(0.5, 0.9), eps=1e-6, weight_decay=0.0),
    "beta1_0": dict(lr=1e-3, betas=(0.0, 0.999), eps=1e-8, weight_decay=1e-2),
    "wd_only": dict(DEFAULT_HP),                          # run with a zero gradient: only the decoupled weight decay moves p
}
GRID_STRIDE_N = 4_194_304 + 1000                         # 4096 blocks x 256 threads x 4: above it every thread of adamw_kernel loops


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _bar(dist_fp32_cpu: float, pmax: float) -> float:
    return max(4.0 * dist_fp32_cpu, 2.0 * R.ulp32(pmax))


def _norm_bar(norm: float) -> float:
    """Bar on the total norm clip_grad_norm_ returns.  The sum of squares is formed in fp32: a product, at most 8 additions per thread,
    6 in the wave, 2 in the block, then 4 + 6 + 2 over the block partials and one addition per tensor — about 30 roundings on the
    longest path, each 2^-24 relative in the worst case.  The square root halves that and adds its own; the scale is a power of two.
    (30 / 2 + 1) x 2^-24 relative is at most 16 ulp of the result."""
    return 16.0 * R.ulp32(norm)


def _dist(a: torch.Tensor, b64: torch.Tensor) -> float:
    return float((a.detach().cpu().double().flatten() - b64.flatten()).abs().max())


# ---------------------------------------------------------------------------------------------------------------- sg_sumsq_f32
def _sumsq(x: torch.Tensor) -> torch.Tensor:
    from storygen_amd import optim
    out = torch.zeros(2, device=x.device)
    scratch = torch.empty(optim.lib.sg_sumsq_scratch_floats(), device=x.device)
    for slot in (0, 1):
        optim.check(optim.lib.sg_sumsq_f32(x.data_ptr(), x.numel(), out[slot:].data_ptr(), scratch.data_ptr(), _stream()), "sg_sumsq_f32")
    return out.cpu()


@pytest.mark.parametrize("pattern", ["ones", "alternating"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2047, 2048, 2049, 2_097_151, 2_097_152, 2_097_153, 3_000_001, 1 << 24])
def test_sumsq_counts_every_element_exactly_once(gpu, n, pattern):
    """Every element is +1 or -1, so every square is 1 and every partial sum the kernel can form — per thread, per wave, per block,
    the final one — is an integer no larger than n <= 2^24, which fp32 holds exactly whatever the order of the additions.  The result
    must EQUAL n: one dropped or double-counted element, at a tail or where the grid stops growing (n = 1024 x 256 x 8 = 2,097,152),
    changes it by one.  Two output slots from two calls must agree bit for bit (no atomics)."""
    x = torch.ones(n, device=gpu)
    if pattern == "alternating":
        x[1::2] = -1.0
    out = _sumsq(x)
    assert float(out[0]) == float(out[1])
    assert float(out[0]) == float(n), (n, float(out[0]) - n)


def test_sumsq_wide_range_against_float64(gpu):
    """One element at 1e4 among 1e-2 values, n = 100,003: squares 1e8 and 1e-4, 12 decades apart.  Bar: 4x the error of
    torch.sum(x * x) in fp32 on the CPU against the float64 sum, floored at 1 ulp of the result."""
    n = 100_003
    x = torch.full((n,), 1e-2)
    x[77_777] = 1e4
    want = float((x.double() ** 2).sum())
    cpu_err = abs(float(torch.sum(x * x)) - want)
    bar = max(4.0 * cpu_err, R.ulp32(want))
    out = _sumsq(x.to(gpu))
    print(f"sumsq wide range: kernel error {abs(float(out[0]) - want):.3g}, fp32 CPU error {cpu_err:.3g}, bar {bar:.3g}")
    assert float(out[0]) == float(out[1])
    assert abs(float(out[0]) - want) <= bar


# ---------------------------------------------------------------------------------------------------------------- sg_adamw_f32
@functools.lru_cache(maxsize=None)
def _data(n: int, steps: int = 4):
    """(p0, gradients of `steps` steps, seeded exp_avg, seeded exp_avg_sq) on the CPU, made once per size and never modified."""
    gen = torch.Generator().manual_seed(1000 + n % 9973)
    p0 = torch.randn(n, generator=gen)
    grads = tuple(torch.randn(n, generator=gen) * (10.0 ** -(s % 3)) for s in range(steps))
    m0 = 0.1 * torch.randn(n, generator=gen)
    v0 = 0.01 * torch.rand(n, generator=gen) + 1e-6
    return p0, grads, m0, v0


def _run_f32(gpu, label, params0, per_step, hp, start=0, states0=None, grad_scale=1.0, max_norm=None, via="set_grads"):
    """Step storygen_amd.optim.AdamW, torch.optim.AdamW (fp32, CPU) and the float64 reference over the same RAW gradients
    (per_step[s][i], None = no gradient; still multiplied by 1 / grad_scale) and hold the kernel to the bar after every step.
    Returns the optimizer under test."""
    from storygen_amd.optim import AdamW
    names = [f"p{i}" for i in range(len(params0))]
    ref = R.AdamW64(params0, **hp)
    tps = [torch.nn.Parameter(p.clone()) for p in params0]
    topt = torch.optim.AdamW(tps, foreach=False, fused=False, **hp)
    mine = {k: torch.nn.Parameter(p.clone().to(gpu)) for k, p in zip(names, params0)}
    opt = AdamW(mine, **hp)
    if start:
        ref.steps = [start] * len(params0)
        state = {}
        for i, (m0, v0) in enumerate(states0):
            ref.m[i], ref.v[i] = m0.double().flatten().clone(), v0.double().flatten().clone()
            topt.state[tps[i]] = dict(step=torch.tensor(float(start)), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
            state[names[i]] = dict(bits=32, step=start, exp_avg=m0.clone(), exp_avg_sq=v0.clone())
        opt.load_state_dict(dict(step=start, param_groups=[{}], names=names, state=state))
    worst = []
    for s, raw in enumerate(per_step, 1):
        for tp, g in zip(tps, raw):
            tp.grad = None if g is None else (g * grad_scale).reshape(tp.shape).clone()
        if max_norm is not None:
            want_norm32 = float(torch.nn.utils.clip_grad_norm_(tps, max_norm))
        topt.step()
        want_norm = ref.step(raw, grad_scale, max_norm)
        if via == "set_grads":
            opt.set_grads({k: None if g is None else g.to(gpu) for k, g in zip(names, raw)})
        else:
            for k, g in zip(names, raw):
                mine[k].grad = None if g is None else g.to(gpu)
        if max_norm is not None:
            got_norm = float(opt.clip_grad_norm_(max_norm, grad_scale=grad_scale))
            nbar = _norm_bar(want_norm)
            assert abs(want_norm32 - want_norm) <= nbar                                # torch's own fp32 norm meets it too
            print(f"{label} step {s}: total norm {got_norm:.8g} (float64 {want_norm:.8g}), off by {abs(got_norm - want_norm):.3g}, bar {nbar:.3g}")
            assert abs(got_norm - want_norm) <= nbar
        opt.step(grad_scale) if max_norm is None else opt.step()
        opt.zero_grad()
        for i, k in enumerate(names):
            d_gpu, d_cpu = _dist(mine[k], ref.p[i]), _dist(tps[i], ref.p[i])
            bar = _bar(d_cpu, float(ref.p[i].abs().max()))
            worst.append((d_gpu / bar, s, k, d_gpu, d_cpu, bar))
    ratio, s, k, d_gpu, d_cpu, bar = max(worst)
    print(f"{label}: worst {k} step {s}: kernel {d_gpu:.3g} from float64, torch fp32 CPU {d_cpu:.3g}, bar {bar:.3g} (ratio {ratio:.2f})")
    assert ratio <= 1.0, (label, k, s, d_gpu, d_cpu, bar)
    # the moments, by the same rule plus one term: Adam's update hardly depends on the SCALE of the gradients (only through eps), the
    # moments do — a lost grad_scale or clip factor shows here first.  The descriptor carries the betas as fp32 and the kernel forms
    # 1 - beta from that value (exactly), so it runs Adam with beta rounded to fp32: 1 - beta is off by up to half an ulp of beta,
    # 2^-25 beta / (1 - beta) relative (3e-5 at 0.999, where torch rounds 1 - beta itself), and the moment by that times its size.
    for i, tp in enumerate(tps):
        if i not in opt.state:
            continue
        for key, want, beta in (("exp_avg", ref.m[i], hp["betas"][0]), ("exp_avg_sq", ref.v[i], hp["betas"][1])):
            d_gpu, d_cpu = _dist(opt.state[i][key], want), _dist(topt.state[tp][key], want)
            wmax = max(float(want.abs().max()), 1e-38)
            bar = _bar(d_cpu, wmax) + 2.0 ** -25 * beta / (1.0 - beta) * wmax
            assert d_gpu <= bar, (label, names[i], key, d_gpu, d_cpu, bar)
    assert opt.step_count == start + len(per_step)
    return opt, mine, ref, tps


def _f32_cases():
    for n in (1, 255, 257, 1023, 1025, GRID_STRIDE_N):
        for hp in HP_SETS:
            for start in (0, 99_999):
                # the grid-stride loop does not depend on the hyper-parameters: the 4M-element tensor runs every set from step 1 and
                # the reference's set from step 100,000 — five cases of half a second of CPU reference instead of eight
                if n == GRID_STRIDE_N and start and hp != "reference":
                    continue
                yield pytest.param(n, hp, start, id=f"n{n}-{hp}-step{start + 1}")


@pytest.mark.parametrize("n,hp_name,start", list(_f32_cases()))
def test_adamw_f32_sizes_hyperparameters_and_step_numbers(gpu, n, hp_name, start):
    """4 steps per case.  Sizes around the 256-thread block and the 1024-element grid step, and 4,194,304 + 1000 where the grid is
    capped at 4096 blocks and every thread loops; step numbers from 1 and from 100,000 (both bias corrections round to 1 in fp32),
    the latter with seeded states and the step number passed through load_state_dict."""
    p0, grads, m0, v0 = _data(n)
    per_step = [[torch.zeros(n) if hp_name == "wd_only" else g] for g in grads]
    _run_f32(gpu, f"adamw_f32 n={n} {hp_name} from step {start + 1}", [p0], per_step, HP_SETS[hp_name], start=start, states0=[(m0, v0)])


@pytest.mark.parametrize("clip", ["none", "active", "inactive"])
@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 65536, 0.25])
def test_adamw_f32_unscales_then_clips(gpu, grad_scale, clip):
    """step(grad_scale) multiplies the gradients by grad_scale; clip_grad_norm_(1.0, grad_scale) clips on — and returns — the norm
    of the UNSCALED gradients, what torch.nn.utils.clip_grad_norm_ gives after GradScaler.unscale_.  The raw gradients are the
    intended ones divided by grad_scale, so the same clip is active (norm ~ 36) or inactive (~ 0.036) at every scale."""
    sizes = (1025, 257)
    size = 1e-3 if clip == "inactive" else 1.0
    per_step = [[_data(n)[1][s] * size / grad_scale for n in sizes] for s in range(4)]
    opt, *_ = _run_f32(gpu, f"adamw_f32 grad_scale={grad_scale:g} clip {clip}", [_data(n)[0] for n in sizes], per_step, DEFAULT_HP,
                       grad_scale=grad_scale, max_norm=None if clip == "none" else 1.0)
    opt.set_grads({"p0": torch.ones(1025, device=gpu), "p1": torch.ones(257, device=gpu)})
    opt.clip_grad_norm_(1.0, grad_scale=0.5)
    with pytest.raises(ValueError):
        opt.step(0.25)                                   # not the scale the returned norm was computed with


def test_adamw_f32_takes_a_transposed_gradient_view(gpu):
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(33, 65, generator=gen)
    per_step = [[torch.randn(65, 33, generator=gen).t()] for _ in range(4)]
    assert not per_step[0][0].is_contiguous()
    _run_f32(gpu, "adamw_f32 transposed gradient", [p0], per_step, DEFAULT_HP)


# -------------------------------------------------------------------------------------------- first gradient on a later step
LATE_SIZES = (257, 1025, 300)


@pytest.mark.parametrize("via", ["p.grad", "set_grads"])
def test_adamw_f32_first_gradient_on_step_3_is_torch_adamw(gpu, via):
    """Tensor 1 has no gradient on steps 1-2.  torch.optim.AdamW creates its state["step"] when the gradient first arrives, so its
    step 3 is bias-corrected with 1 - beta^1; the number of step() calls would give 1 - beta^3 and a first update 2.7x too small at
    beta1 = 0.9.  Through p.grad = None and through a set_grads dict that carries None for it."""
    per_step = [[None if (i == 1 and s < 2) else _data(n, 5)[1][s] for i, n in enumerate(LATE_SIZES)] for s in range(5)]
    opt, mine, ref, tps = _run_f32(gpu, f"adamw_f32 late gradient via {via}", [_data(n, 5)[0] for n in LATE_SIZES], per_step, DEFAULT_HP, via=via)
    assert [opt.state[i]["step"] for i in range(3)] == [5, 3, 5] == ref.steps and opt.step_count == 5
    sd = opt.state_dict()
    assert sd["step"] == 5 and [sd["state"][f"p{i}"]["step"] for i in range(3)] == [5, 3, 5]


# ---------------------------------------------------------------------------------------------------------------- sg_adamw8bit
GUARD_CODE, GUARD_F = 0xA5, -7.0


def _guarded_8bit(opt, gpu):
    """Move every 8-bit state of `opt` into a buffer with a sentinel tail: codes up to the end of the last 2048-block and beyond,
    one absmax entry past the last block.  Returns the buffers for _guards_intact."""
    keep = []
    for i, p in enumerate(opt.params):
        st = opt._state(i)
        if st["bits"] != 8:
            continue
        n, nb = p.numel(), st["absmax1"].numel()
        for k in ("code1", "code2"):
            big = torch.full((nb * oo.BLOCK + 256,), GUARD_CODE, dtype=torch.uint8, device=gpu)
            big[:n] = st[k]
            st[k] = big[:n]
            keep.append((big, n, GUARD_CODE))
        for k in ("absmax1", "absmax2"):
            big = torch.full((nb + 1,), GUARD_F, device=gpu)
            big[:nb] = st[k]
            st[k] = big[:nb]
            keep.append((big, nb, GUARD_F))
    return keep


def _guards_intact(keep) -> bool:
    return all(bool((big[n:] == val).all()) for big, n, val in keep)


def _run_8bit(gpu, label, params0, per_step, hp, grad_scale=1.0, max_norm=None, zero_blocks=(), tight=False, via="set_grads"):
    """AdamW8bit over `params0` (tensors of >= 4096 elements get 8-bit states, smaller ones fp32) against ONE step of the references
    from the kernel's own previous states, re-synchronised after every step as tests/test_optim_gpu.py does: the 8-bit step of
    oracle/optim_oracle.py on the scaled and clipped gradient; for an fp32 tensor the float64 step, with the bar of _bar."""
    from storygen_amd.optim import AdamW8bit
    names = [f"w{i}" for i in range(len(params0))]
    bufs = [torch.full((p.numel() + 64,), GUARD_F, device=gpu) for p in params0]          # parameters with a sentinel tail too
    mine = {}
    for k, p, b in zip(names, params0, bufs):
        b[:p.numel()] = p.to(gpu)
        mine[k] = torch.nn.Parameter(b[:p.numel()])
    opt = AdamW8bit(mine, **hp)
    keep = _guarded_8bit(opt, gpu) + [(b, p.numel(), GUARD_F) for b, p in zip(bufs, params0)]
    z1, z2 = opt._zero1, opt._zero2
    steps = [0] * len(params0)
    cpu = []                                                  # the kernel's states as of the previous step, on the CPU
    for i, p in enumerate(params0):
        n = p.numel()
        cpu.append(dict(p=p.clone(), s=list(oo.adamw8bit_state(n))) if n >= 4096 else dict(p=p.clone(), s=[torch.zeros(n), torch.zeros(n)]))
    for s, raw in enumerate(per_step, 1):
        factor, want_norm = R.grad_factor64(raw, grad_scale, max_norm)
        if via == "set_grads":
            opt.set_grads({k: None if g is None else g.to(gpu) for k, g in zip(names, raw)})
        else:
            for k, g in zip(names, raw):
                mine[k].grad = None if g is None else g.to(gpu)
        if max_norm is not None:
            got_norm = float(opt.clip_grad_norm_(max_norm, grad_scale=grad_scale))
            assert abs(got_norm - want_norm) <= _norm_bar(want_norm), (got_norm, want_norm)
            opt.step()
        else:
            opt.step(grad_scale)
        opt.zero_grad()
        for i, (k, g) in enumerate(zip(names, raw)):
            st, c, got_p = opt.state.get(i), cpu[i], mine[k].detach().cpu()
            if g is None:
                assert torch.equal(got_p, c["p"]) and (st is None or st["step"] == steps[i])
                continue
            steps[i] += 1
            assert st["step"] == steps[i]
            f32_factor = torch.tensor(factor, dtype=F32)
            if st["bits"] == 32:
                assert g.numel() < opt.min_8bit_size
                p64, m64, v64 = c["p"].double(), c["s"][0].double(), c["s"][1].double()
                R.adamw_step64(p64, g, m64, v64, steps[i], factor=factor, **hp)
                oo.adamw_step(c["p"], g * f32_factor, c["s"][0], c["s"][1], steps[i], **hp)
                d_gpu, bar = _dist(got_p, p64), _bar(_dist(c["p"], p64), float(p64.abs().max()))
                print(f"{label} step {s} {k} (fp32 states): kernel {d_gpu:.3g} from float64, bar {bar:.3g}")
                assert d_gpu <= bar
                c["p"].copy_(got_p), c["s"][0].copy_(st["exp_avg"].cpu()), c["s"][1].copy_(st["exp_avg_sq"].cpu())
                continue
            assert g.numel() >= opt.min_8bit_size
            p, (c1, c2, a1, a2) = c["p"], c["s"]
            if tight:
                p64 = R.adamw8bit_step_f64_moments(p.clone(), g * f32_factor, c1.clone(), c2.clone(), a1.clone(), a2.clone(), steps[i], **hp)
            R.adamw8bit_step_scaled(p, g, c1, c2, a1, a2, steps[i], factor=factor, **hp)
            d_gpu, bar = float((got_p - p).abs().max()), 1e-5
            if tight:                   # lr = 1e-5: an update is an ulp or so of the parameter, 1e-5 would let it be missing altogether
                d_gpu, bar = _dist(got_p, p64), min(1e-5, _bar(_dist(p, p64), float(p64.abs().max())))
            g1, g2, ga1, ga2 = st["code1"].cpu(), st["code2"].cpu(), st["absmax1"].cpu(), st["absmax2"].cpu()
            d1, d2 = (g1.int() - c1.int()).abs(), (g2.int() - c2.int()).abs()
            f1, f2 = float((d1 > 0).float().mean()), float((d2 > 0).float().mean())
            print(f"{label} step {s} {k}: parameters {d_gpu:.3g} (bar {bar:.3g}), codes differing {f1:.2%} / {f2:.2%}, "
                  f"absmax rel-L2 {rel_l2(ga1, a1):.2e} / {rel_l2(ga2, a2):.2e}")
            assert d_gpu <= bar
            assert rel_l2(ga1, a1) < 1e-4 and rel_l2(ga2, a2) < 1e-4
            assert int(d1.max()) <= 1 and int(d2.max()) <= 1
            assert f1 < 0.01 and f2 < 0.01
            for b in zero_blocks:                             # a block whose moments are all zero: the zero code, absmax exactly 0
                sl = slice(b * oo.BLOCK, (b + 1) * oo.BLOCK)
                assert bool((g1[sl] == z1).all()) and bool((g2[sl] == z2).all()) and float(ga1[b]) == 0.0 and float(ga2[b]) == 0.0
            c1.copy_(g1), c2.copy_(g2), a1.copy_(ga1), a2.copy_(ga2), p.copy_(got_p)
        assert _guards_intact(keep), f"{label} step {s}: something was written past the end of a tensor"
    return opt


@pytest.mark.parametrize("name", list(R.EIGHT_BIT_CASES))
def test_adamw8bit_blocks_contents_rates_and_clip_against_the_oracle(gpu, name):
    """3 steps per case (tests/optim_reference.py::EIGHT_BIT_CASES; tests/test_optim_reference.py keeps every one of them well inside
    the 1 % cap on the CPU): n = 4096 (the min_8bit_size threshold, >=), 4097 (a block with ONE live element), exact multiples of
    2048, one short of and one past a multiple; a block whose gradient is zero from step 1 (absmax 0 -> reciprocal 0) and stays zero
    while its neighbours move; a block with one outlier 1e4 times the rest; the reference's lr = 1e-5, where the bar tightens from
    1e-5 to 4x the fp32 oracle's distance from its float64 form (floor 2 ulp); an active clip together with grad_scale = 0.25 and a
    4095-element tensor in the same optimizer, which keeps fp32 states and shares the clip total."""
    params0, per_step, hp, grad_scale, max_norm = R.eight_bit_inputs(name)
    content = R.EIGHT_BIT_CASES[name][1]
    opt = _run_8bit(gpu, f"adamw8bit {name}", params0, per_step, hp, grad_scale, max_norm, zero_blocks=(0,) if content == "zero_block" else (),
                    tight=hp["lr"] == 1e-5)
    assert opt.state[0]["bits"] == 8
    if len(params0) > 1:
        assert opt.state[1]["bits"] == 32 and params0[1].numel() == 4095
    if max_norm is not None:                                  # the case must have had the clip both active and inactive
        norms = [R.total_norm64(raw, grad_scale) for raw in per_step]
        assert max(norms) > max_norm > min(norms)


@pytest.mark.parametrize("via", ["p.grad", "set_grads"])
def test_adamw8bit_first_gradient_on_step_3(gpu, via):
    sizes = (4097, 2 * 2048, 300)
    cases = [R.eight_bit_case(n, "normal", seed=23) for n in sizes]
    per_step = [[None if (i == 1 and s < 2) else cases[i][1][s] for i in range(3)] for s in range(3)]
    per_step += [[c[1][s] * 0.5 for c in cases] for s in range(2)]                    # two more steps: 5 in all, 3 for tensor 1
    opt = _run_8bit(gpu, f"adamw8bit late gradient via {via}", [c[0] for c in cases], per_step, R.HP_8BIT, via=via)
    assert [opt.state[i]["step"] for i in range(3)] == [5, 3, 5] and opt.step_count == 5
    assert [opt.state[i]["bits"] for i in range(3)] == [8, 8, 32]


def test_adamw8bit_a_non_finite_gradient_stays_in_its_block(gpu):
    """One inf in block 1 of a 3-block tensor, no clip: blocks 0 and 2 — parameters, codes, absmax — equal the run without it bit
    for bit, and the poisoned element's parameter is non-finite (inf / inf).  Nothing else is asserted about block 1: what its absmax
    becomes is undefined today, because fmaxf drops a NaN operand and the block maximum then depends on the reduction order."""
    from storygen_amd.optim import AdamW8bit
    n, bad = 3 * oo.BLOCK, oo.BLOCK + 100
    p0, grads = R.eight_bit_case(n, "normal", seed=31)
    runs = []
    for poison in (False, True):
        w = {"w": p0.clone().to(gpu)}
        opt = AdamW8bit(w, **R.HP_8BIT)
        for s, g in enumerate(grads[:2]):
            g = g.clone()
            if poison and s == 0:
                g[bad] = float("inf")
            opt.set_grads({"w": g.to(gpu)})
            opt.step()
        runs.append((w["w"].cpu(), {k: v.cpu() for k, v in opt.state[0].items() if torch.is_tensor(v)}))
    (p_ok, st_ok), (p_bad, st_bad) = runs
    for blk in (0, 2):
        sl = slice(blk * oo.BLOCK, (blk + 1) * oo.BLOCK)
        assert torch.equal(p_ok[sl], p_bad[sl])
        assert torch.equal(st_ok["code1"][sl], st_bad["code1"][sl]) and torch.equal(st_ok["code2"][sl], st_bad["code2"][sl])
        assert float(st_ok["absmax1"][blk]) == float(st_bad["absmax1"][blk]) and float(st_ok["absmax2"][blk]) == float(st_bad["absmax2"][blk])
    assert not bool(torch.isfinite(p_bad[bad])) and bool(torch.isfinite(p_ok).all())


# ---------------------------------------------------------------------------------------------------------------- ABI level
def _desc(p, g, hp, step=1, grad_scale=1.0):
    from storygen_amd._lib import AdamWDesc
    d = AdamWDesc()
    d.param, d.grad, d.n = p.data_ptr(), g.data_ptr(), p.numel()
    d.lr, (d.beta1, d.beta2), d.eps, d.weight_decay = hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"]
    d.step, d.grad_scale = step, grad_scale
    return d


def _f32_call(gpu, p0, g, m0, v0, hp, sums, max_norm, grad_scale, step):
    from storygen_amd import optim
    p, m, v = p0.clone().to(gpu), m0.clone().to(gpu), v0.clone().to(gpu)
    gg, ss = g.to(gpu), sums.to(gpu)
    d = _desc(p, gg, hp, step, grad_scale)
    d.exp_avg, d.exp_avg_sq = m.data_ptr(), v.data_ptr()
    d.sumsq, d.n_sumsq, d.max_norm = ss.data_ptr(), ss.numel(), max_norm
    optim.check(optim.lib.sg_adamw_f32(C.byref(d), _stream()), "sg_adamw_f32")
    torch.cuda.synchronize()
    return p.cpu()


def _eight_bit_call(gpu, p0, g, states, hp, sums, max_norm, grad_scale, step):
    from storygen_amd import optim
    c1, c2, a1, a2 = (t.clone().to(gpu) for t in states)
    q1, q2 = optim.create_dynamic_map(True).to(gpu), optim.create_dynamic_map(False).to(gpu)
    p, gg, ss = p0.clone().to(gpu), g.to(gpu), sums.to(gpu)
    d = _desc(p, gg, hp, step, grad_scale)
    d.code1, d.code2, d.absmax1, d.absmax2 = c1.data_ptr(), c2.data_ptr(), a1.data_ptr(), a2.data_ptr()
    d.q_code1, d.q_code2 = q1.data_ptr(), q2.data_ptr()
    d.sumsq, d.n_sumsq, d.max_norm = ss.data_ptr(), ss.numel(), max_norm
    optim.check(optim.lib.sg_adamw8bit(C.byref(d), _stream()), "sg_adamw8bit")
    torch.cuda.synchronize()
    return p.cpu(), c1.cpu(), c2.cpu(), a1.cpu(), a2.cpu()


@pytest.mark.parametrize("n_sums", [3, 4096])
def test_per_tensor_sums_of_squares_at_abi_level(gpu, n_sums):
    """The descriptor's `sumsq` may point at up to 4096 per-tensor sums that the kernel adds itself; storygen_amd.optim always passes
    one pre-summed total, so this path has no caller.  Both forms must give the float64 step with the float64 total of the same
    sums (the order of the additions differs), under the fp32 bar, and for the 8-bit kernel the oracle's step under its bars."""
    gen = torch.Generator().manual_seed(40 + n_sums)
    sums = torch.rand(n_sums, generator=gen) * (40.0 / n_sums) + 1e-3                      # total ~ 20: norm ~ 4.5, the clip is active
    total = sums.sum(dim=0, keepdim=True)
    grad_scale, max_norm, hp = 0.25, 1.0, DEFAULT_HP
    norm = grad_scale * float(sums.double().sum()) ** 0.5
    factor = grad_scale * min(1.0, max_norm / (norm + 1e-6))
    assert factor < grad_scale
    # step 5 from non-zero moments: Adam's FIRST step is lr * sign(g) whatever the clip factor, a later one is not
    p0, grads, m0, v0 = _data(1025)
    p64, m64, v64 = p0.double(), m0.double(), v0.double()
    R.adamw_step64(p64, grads[0], m64, v64, 5, factor=factor, **hp)
    unclipped = p0.double()
    R.adamw_step64(unclipped, grads[0], m0.double(), v0.double(), 5, factor=grad_scale, **hp)
    p32, m32, v32 = p0.clone(), m0.clone(), v0.clone()
    oo.adamw_step(p32, grads[0] * torch.tensor(factor, dtype=F32), m32, v32, 5, **hp)
    bar = _bar(_dist(p32, p64), float(p64.abs().max()))
    assert _dist(unclipped, p64) > 100 * bar                                           # ignoring the sums would not pass
    for label, ss in (("per-tensor sums", sums), ("one total", total)):
        got = _f32_call(gpu, p0, grads[0], m0, v0, hp, ss, max_norm, grad_scale, 5)
        print(f"sg_adamw_f32 n_sumsq={ss.numel()} ({label}): {_dist(got, p64):.3g} from float64, bar {bar:.3g}")
        assert _dist(got, p64) <= bar
    q0, qgrads = R.eight_bit_case(4097, "normal", seed=41)
    p, c1, c2, a1, a2 = [q0.clone(), *oo.adamw8bit_state(4097)]
    oo.adamw8bit_step(p, qgrads[0], c1, c2, a1, a2, 1, **R.HP_8BIT)                     # step 1 on the CPU: non-zero states for step 2
    q1, states = p.clone(), [t.clone() for t in (c1, c2, a1, a2)]
    R.adamw8bit_step_scaled(p, qgrads[1], c1, c2, a1, a2, 2, factor=factor, **R.HP_8BIT)
    for label, ss in (("per-tensor sums", sums), ("one total", total)):
        gp, g1, g2, ga1, ga2 = _eight_bit_call(gpu, q1, qgrads[1], states, R.HP_8BIT, ss, max_norm, grad_scale, 2)
        d1, d2 = (g1.int() - c1.int()).abs(), (g2.int() - c2.int()).abs()
        print(f"sg_adamw8bit n_sumsq={ss.numel()} ({label}): parameters {float((gp - p).abs().max()):.3g}, codes differing "
              f"{float((d1 > 0).float().mean()):.2%} / {float((d2 > 0).float().mean()):.2%}")
        assert float((gp - p).abs().max()) <= 1e-5
        assert rel_l2(ga1, a1) < 1e-4 and rel_l2(ga2, a2) < 1e-4
        assert int(d1.max()) <= 1 and int(d2.max()) <= 1
        assert float((d1 > 0).float().mean()) < 0.01 and float((d2 > 0).float().mean()) < 0.01


def _bad_descriptors():
    def clip(n_sumsq, max_norm):
        def f(d, sums):
            d.sumsq, d.n_sumsq, d.max_norm = sums.data_ptr(), n_sumsq, max_norm
        return f
    both = [("step=0", lambda d, s: setattr(d, "step", 0), "step counts from 1"),
            ("beta1=1", lambda d, s: setattr(d, "beta1", 1.0), "bad hyper-parameters"),
            ("lr<0", lambda d, s: setattr(d, "lr", -1e-3), "bad hyper-parameters"),
            ("sumsq_with_n_sumsq=0", clip(0, 1.0), "clipping needs 1..4096 sums of squares"),
            ("n_sumsq=4097", clip(4097, 1.0), "clipping needs 1..4096 sums of squares"),
            ("max_norm=0", clip(1, 0.0), "clipping needs 1..4096 sums of squares"),
            ("n=0", lambda d, s: setattr(d, "n", 0), "null param / grad or empty tensor")]
    for kernel in ("sg_adamw_f32", "sg_adamw8bit"):
        for name, mutate, text in both:
            yield pytest.param(kernel, mutate, text, id=f"{kernel}-{name}")
    yield pytest.param("sg_adamw_f32", lambda d, s: setattr(d, "exp_avg", None), "sg_adamw_f32: null state", id="sg_adamw_f32-null_exp_avg")
    yield pytest.param("sg_adamw8bit", lambda d, s: setattr(d, "code1", None), "sg_adamw8bit: null 8-bit state", id="sg_adamw8bit-null_code1")


@pytest.mark.parametrize("kernel,mutate,text", list(_bad_descriptors()))
def test_rejected_descriptors_raise_and_write_nothing(gpu, kernel, mutate, text):
    """Every one of these returns from the argument checks, before any launch: a RuntimeError with the check's own text, and the
    parameter is as it was."""
    from storygen_amd import optim
    n = 4097
    p0 = _data(n)[0]
    p, g, sums = p0.clone().to(gpu), torch.ones(n, device=gpu), torch.ones(4097, device=gpu)
    m, v = torch.zeros(n, device=gpu), torch.zeros(n, device=gpu)
    c1, c2, a1, a2 = (t.to(gpu) for t in oo.adamw8bit_state(n))
    q1, q2 = optim.create_dynamic_map(True).to(gpu), optim.create_dynamic_map(False).to(gpu)
    d = _desc(p, g, DEFAULT_HP)
    d.exp_avg, d.exp_avg_sq = m.data_ptr(), v.data_ptr()
    d.code1, d.code2, d.absmax1, d.absmax2 = c1.data_ptr(), c2.data_ptr(), a1.data_ptr(), a2.data_ptr()
    d.q_code1, d.q_code2 = q1.data_ptr(), q2.data_ptr()
    mutate(d, sums)
    with pytest.raises(RuntimeError) as err:
        optim.check(getattr(optim.lib, kernel)(C.byref(d), _stream()), kernel)
    assert text in str(err.value) and kernel in str(err.value)
    torch.cuda.synchronize()
    assert torch.equal(p.cpu(), p0) and not bool(m.any()) and not bool(v.any())


# ---------------------------------------------------------------------------------------------------------------- resume
@pytest.mark.parametrize("kind", ["adamw", "adamw8bit", "mixed"])
def test_a_resumed_trajectory_is_the_uninterrupted_one(gpu, kind):
    """3 steps, state_dict(), a new optimizer over cloned parameters, load_state_dict(), 3 more steps == 6 uninterrupted steps, bit
    for bit: parameters and every state tensor (absmax included) and every per-parameter step number.  In the mixed set the small
    tensor has no gradient on step 1, so its step number differs from step_count and must come back from the state dict."""
    from storygen_amd.optim import AdamW, AdamW8bit
    cls = AdamW if kind == "adamw" else AdamW8bit
    sizes = dict(adamw=(1025, 300), adamw8bit=(4097, 3 * 2048), mixed=(4097, 300))[kind]
    gen = torch.Generator().manual_seed(50)
    p0 = {f"w{i}": torch.randn(n, generator=gen) for i, n in enumerate(sizes)}
    grads = [{k: torch.randn(p.numel(), generator=gen).to(gpu) for k, p in p0.items()} for _ in range(6)]
    if kind == "mixed":
        grads[0]["w1"] = None

    def advance(opt, steps):
        for s in steps:
            opt.set_grads(grads[s])
            opt.clip_grad_norm_(1.0)
            opt.step()
            opt.zero_grad()

    straight = {k: v.clone().to(gpu) for k, v in p0.items()}
    o1 = cls(straight, **DEFAULT_HP)
    advance(o1, range(6))
    first = {k: v.clone().to(gpu) for k, v in p0.items()}
    o2 = cls(first, **DEFAULT_HP)
    advance(o2, range(3))
    sd = o2.state_dict()
    resumed = {k: v.clone() for k, v in first.items()}
    o3 = cls(resumed, **DEFAULT_HP)
    o3.load_state_dict(sd)
    assert o3.step_count == 3 and [o3.state[i]["step"] for i in range(2)] == [o2.state[i]["step"] for i in range(2)]
    advance(o3, range(3, 6))
    assert o3.step_count == o1.step_count == 6
    for k in p0:
        assert torch.equal(resumed[k], straight[k]), k
    for i in range(2):
        a, b = o1.state[i], o3.state[i]
        assert a.keys() == b.keys() and a["bits"] == b["bits"] and a["step"] == b["step"] == (5 if (kind == "mixed" and i == 1) else 6)
        assert all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k])), (i, [k for k in a if torch.is_tensor(a[k]) and not torch.equal(a[k], b[k])])
    if kind == "mixed":
        assert [o1.state[i]["bits"] for i in range(2)] == [8, 32]
    # a state dict written before the per-parameter step numbers existed: every tensor takes step_count
    old = {"step": sd["step"], "param_groups": sd["param_groups"], "names": sd["names"],
           "state": {k: {kk: vv for kk, vv in st.items() if kk != "step"} for k, st in sd["state"].items()}}
    o4 = cls({k: v.clone() for k, v in first.items()}, **DEFAULT_HP)
    o4.load_state_dict(old)
    assert o4.step_count == 3 and all(o4.state[i]["step"] == 3 for i in range(2))
