"""CPU: the float64 optimizer reference of tests/optim_reference.py (what tests/test_optim_edges_gpu.py measures the kernels
against) pinned three ways — to torch.optim.AdamW + torch.nn.utils.clip_grad_norm_, to oracle/optim_oracle.py, and on a parameter
whose first gradient arrives at step 3 — and the inputs of the 8-bit GPU comparison shown to leave the oracle itself well inside the
GPU test's cap on differing codes."""
import pytest
import torch

import optim_reference as R
from oracle import optim_oracle as oo

HPS = [dict(R.REFERENCE_HP), dict(lr=1e-3, betas=(0.5, 0.9), eps=1e-6, weight_decay=0.0), dict(lr=1e-3, betas=(0.0, 0.999), eps=1e-8, weight_decay=1e-2)]
SHAPES = [(300,), (17, 5), (1,)]


def _close(p32: torch.Tensor, p64: torch.Tensor, steps: int) -> bool:
    """An fp32 AdamW step rounds the parameter twice (decay, update) and its update carries ~1e-6 relative error of at most lr-sized
    terms: after `steps` steps an fp32 implementation is within 2 ulp per step of the float64 value, taken at the largest |p|."""
    return float((p32.double().flatten() - p64).abs().max()) <= 2 * steps * R.ulp32(float(p64.abs().max()))


@pytest.mark.parametrize("hp", HPS, ids=["reference", "b.5_.9", "beta1_0"])
@pytest.mark.parametrize("grad_scale,max_norm", [(1.0, None), (1.0, 1.0), (1.0 / 65536, 1.0), (0.25, None), (0.25, 1.0)])
def test_reference_is_torch_adamw_after_unscale_and_clip(hp, grad_scale, max_norm):
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
    ref = R.AdamW64(ps, **hp)
    opt = torch.optim.AdamW(ps, foreach=False, fused=False, **hp)
    gmax = [0.0] * len(ps)
    for step in range(1, 6):
        size = 3.0 if step % 2 else 0.003                                 # the clip is active on the odd steps only
        raw = [torch.randn(s) * size / grad_scale for s in SHAPES]         # what the optimizer is handed: still loss-scaled
        for p, g in zip(ps, raw):
            p.grad = g * grad_scale
        want_norm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm)) if max_norm is not None else None
        gmax = [max(a, float(p.grad.abs().max())) for a, p in zip(gmax, ps)]      # after the clip: what enters the moments
        opt.step()
        norm = ref.step(raw, grad_scale, max_norm)
        if want_norm is not None:
            assert norm == pytest.approx(want_norm, rel=1e-6)
            assert (norm > max_norm) == bool(step % 2)
        for p, q in zip(ps, ref.p):
            assert _close(p.detach(), q, step)
    for i, p in enumerate(ps):
        st = opt.state[p]
        assert int(st["step"]) == ref.steps[i] == 5
        # a moment is a decaying sum of five gradient terms of either sign: a few fp32 roundings of the largest term
        assert float((st["exp_avg"].flatten().double() - ref.m[i]).abs().max()) <= 1e-6 * gmax[i]
        assert float((st["exp_avg_sq"].flatten().double() - ref.v[i]).abs().max()) <= 1e-6 * gmax[i] ** 2


def test_reference_is_the_optimizer_oracle():
    torch.manual_seed(1)
    n, hp = 2000, dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    p0 = [torch.randn(n), torch.randn(77)]
    ref = R.AdamW64(p0, **hp)
    p = [x.clone() for x in p0]
    m, v = [torch.zeros_like(x) for x in p0], [torch.zeros_like(x) for x in p0]
    for step in range(1, 5):
        gs = [torch.randn_like(x) * (5.0 if step % 2 else 0.01) for x in p0]
        c = oo.clip_coef(gs, 1.0)
        factor, _ = R.grad_factor64(gs, 1.0, 1.0)
        assert factor == pytest.approx(c, rel=1e-6) and (c < 1.0) == bool(step % 2)
        ref.step(gs, 1.0, 1.0)
        for i in range(2):
            oo.adamw_step(p[i], gs[i] * c, m[i], v[i], step, **hp)
            assert _close(p[i], ref.p[i], step)


@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_a_parameter_whose_first_gradient_arrives_at_step_3_starts_at_step_1(max_norm):
    """torch.optim.AdamW creates state["step"] when a parameter first has a gradient: its first update is bias-corrected with
    1 - beta^1 whatever the number of step() calls before it.  With weight decay off that first update is lr * sign(g) (Adam's first
    step); a global step number would make it (1 - 0.9) / (1 - 0.9^3) = 0.369 of that, about 2.7 times too small."""
    torch.manual_seed(2)
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    ps = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
    ref = R.AdamW64(ps, **hp)
    opt = torch.optim.AdamW(ps, foreach=False, fused=False, **hp)
    late = 1
    for step in range(1, 6):
        grads = [torch.randn(s) for s in SHAPES]
        if step < 3:
            grads[late] = None
        before = ps[late].detach().clone()
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        ref.step(grads, 1.0, max_norm)
        for p, q in zip(ps, ref.p):
            assert _close(p.detach(), q, step)
        moved = (ps[late].detach() - before).abs()
        if step < 3:
            assert float(moved.max()) == 0.0
        elif step == 3:
            assert float((moved / hp["lr"] - 1.0).abs().max()) < 1e-3          # lr * sign(g), not 0.369 of it
    assert ref.steps == [5, 3, 5] and [int(opt.state[p]["step"]) for p in ps] == [5, 3, 5]


@pytest.mark.parametrize("name", list(R.EIGHT_BIT_CASES))
def test_eight_bit_inputs_leave_the_oracle_well_inside_the_code_cap(name):
    """tests/test_optim_edges_gpu.py allows the kernel's codes to differ from oo.adamw8bit_step's by one on fewer than 1 % of the
    entries: an fp32 rounding (a fused multiply-add, a reciprocal) may carry a moment across a bin boundary.  That cap is a condition on
    the inputs, so they are kept only while the oracle itself is far from it: against the same step with float64 moments it differs
    on at most 0.5 % of the codes and by at most one.  Both trajectories restart from the oracle's states after every step, as the
    GPU test restarts from the kernel's."""
    params, per_step, hp, grad_scale, max_norm = R.eight_bit_inputs(name)
    n = params[0].numel()
    p = params[0].clone()
    c1, c2, a1, a2 = oo.adamw8bit_state(n)
    for step, raw in enumerate(per_step, 1):
        factor, _ = R.grad_factor64(raw, grad_scale, max_norm)
        q, d1, d2, b1, b2 = p.clone(), c1.clone(), c2.clone(), a1.clone(), a2.clone()
        g = raw[0] * torch.tensor(factor, dtype=torch.float32)
        R.adamw8bit_step_scaled(p, raw[0], c1, c2, a1, a2, step, factor=factor, **hp)
        R.adamw8bit_step_f64_moments(q, g, d1, d2, b1, b2, step, **hp)
        for mine, other in ((c1, d1), (c2, d2)):
            diff = (mine.int() - other.int()).abs()
            assert int(diff.max()) <= 1 and float((diff > 0).float().mean()) <= 0.005, (name, step)
        assert torch.allclose(a1, b1, rtol=1e-6, atol=0) and torch.allclose(a2, b2, rtol=1e-6, atol=0)
        assert float((p - q).abs().max()) <= 1e-6                              # a tenth of the GPU test's 1e-5
    if R.EIGHT_BIT_CASES[name][1] == "zero_block":
        z1, z2 = int((oo.dynamic_map(True) == 0).nonzero()[0]), int((oo.dynamic_map(False) == 0).nonzero()[0])
        assert bool((c1[:oo.BLOCK] == z1).all()) and bool((c2[:oo.BLOCK] == z2).all()) and float(a1[0]) == 0.0 and float(a2[0]) == 0.0
        assert float(a1[1]) > 0.0
