"""tests/attention_bwd_model.py (the reference and the rounding yardstick of tests/test_attention_backward_edges_gpu.py) checked on the CPU:
its `exact` against the hand-written oracle and against torch.autograd, and its `rounded` against the project's bars on every input family
of the GPU test — a correct kernel CAN meet them, shown before any GPU time is spent."""
import pytest
import torch

import attention_bwd_model as M

H = 8
SHAPES = [(40, 2, 72, 77), (80, 1, 40, 129), (160, 3, 24, 33), (40, 1, 8, 1)]


def _close(a, b, tol=1e-12):
    scale = max(float(b.abs().max()), 1e-300)
    return float((a - b).abs().max()) <= tol * max(scale, 1.0)


@pytest.mark.parametrize("D,B,Nq,Nk", SHAPES)
def test_exact_is_the_oracle_in_float64(D, B, Nq, Nk):
    from oracle import storygen_backward as O
    q, k, v, do = M.make_inputs("normal", B, H, D, Nq, Nk, seed=3)
    ex = M.exact(q, k, v, do, H)
    qd, kd, vd, dod = (t.double() for t in (q, k, v, do))
    o, lse = O.attention_core(qd, kd, vd, H)
    dq, dk, dv = O.attention_core_bwd(qd, kd, vd, o, lse, dod, H)
    assert _close(ex["o"], o) and _close(ex["lse2"], lse * M.LOG2E)
    assert _close(ex["dq"], dq) and _close(ex["dk"], dk) and _close(ex["dv"], dv)
    assert _close(ex["delta"], (dod * o).reshape(B, Nq, H, D).sum(-1).transpose(1, 2))


@pytest.mark.parametrize("D,B,Nq,Nk", SHAPES)
def test_exact_is_autograd_through_a_float64_softmax_attention(D, B, Nq, Nk):
    q, k, v, do = M.make_inputs("normal", B, H, D, Nq, Nk, seed=4)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    hd = lambda t: t.reshape(t.shape[0], t.shape[1], H, D).transpose(1, 2)                      # noqa: E731
    o = (torch.softmax(hd(qd) @ hd(kd).transpose(-1, -2) * D ** -0.5, dim=-1) @ hd(vd)).transpose(1, 2).reshape(B, Nq, H * D)
    dq, dk, dv = torch.autograd.grad(o, (qd, kd, vd), do.double())
    ex = M.exact(q, k, v, do, H)
    assert _close(ex["o"], o.detach())
    assert _close(ex["dq"], dq) and _close(ex["dk"], dk) and _close(ex["dv"], dv)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("D,B,Nq,Nk", M.RANGE_SHAPES)
@pytest.mark.parametrize("family", M.FAMILIES)
def test_the_documented_roundings_alone_stay_inside_the_bars(family, D, B, Nq, Nk, seed):
    """o 2e-3, lse2 2e-3 absolute, delta / dq / dk / dv 5e-3 aggregate rel-L2 (tests/test_backward_gpu.py::test_attention_backward) with
    the kernel's documented roundings and nothing else, at the shapes and on the inputs the GPU test runs (seed 0 is the GPU test's)."""
    q, k, v, do = M.make_inputs(family, B, H, D, Nq, Nk, seed)
    ex, rd = M.exact(q, k, v, do, H), M.rounded(q, k, v, do, H)
    errs = {n: M.rel_l2(rd[n], ex[n]) for n in ("o", "delta", "dq", "dk", "dv")}
    rows = {n: M.max_row_error(rd[n], ex[n], H) for n in ("dq", "dk", "dv")}
    print(f"{family} D{D} B{B} Nq{Nq} Nk{Nk} seed{seed}: aggregate " + " ".join(f"{n} {e:.1e}" for n, e in errs.items()) +
          " | worst row " + " ".join(f"{n} {e:.1e}" for n, e in rows.items()))
    assert all(bool(torch.isfinite(rd[n]).all()) for n in rd)
    assert float((rd["lse2"] - ex["lse2"]).abs().max()) <= 2e-3
    assert errs["o"] <= 2e-3 and errs["delta"] <= 5e-3
    assert max(errs["dq"], errs["dk"], errs["dv"]) <= 5e-3


def test_row_metric_sees_one_wrong_row_that_the_aggregate_misses():
    """The reason for the per-row bar: one key row of dK replaced by 1.1 x itself at Nk = 776 moves the aggregate by ~0.1 / sqrt(776)
    = 3.6e-3 < 5e-3, and the row metric by ~0.1."""
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(1, 776, H * 40, generator=g, dtype=torch.float64)
    got = ref.clone()
    got[0, 400] *= 1.1
    assert M.rel_l2(got, ref) < 5e-3
    assert M.max_row_error(got, ref, H) > 0.05
