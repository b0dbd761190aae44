"""The four update kernels behind their shared wrapper path (storygen_amd.ops._cfg_step) on the GPU: no tolerance anywhere — the
kernels are elementwise, so every comparison is bitwise."""
import pytest
import torch

import update_rule_helpers as H

RULES = ("ddim", "ddim_var", "plms", "dpm")


@pytest.fixture(scope="module")
def runs(gpu):
    """Every (rule, total, with latents3) run, made once."""
    from storygen_amd import ops
    out = {(r, t, w): H.run_kernel(ops, r, t, w, gpu) for r in RULES for t in H.KERNEL_TOTALS for w in (True, False)}
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("total", H.KERNEL_TOTALS)
@pytest.mark.parametrize("rule", RULES)
def test_copies_and_optional_latents3(runs, rule, total):
    """The three latents3 copies are the new latents; without latents3 the latents and the rule's state come out the same."""
    a, b = runs[rule, total, True], runs[rule, total, False]
    x = a["latents"]
    assert torch.isfinite(x).all() and not torch.equal(x.flatten(), H.kernel_case(total)["latents"].flatten())
    assert torch.equal(a["latents3"].view(3, -1), x.reshape(1, -1).expand(3, -1))
    assert set(b) == set(a) - {"latents3"}
    for k in b:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULES)
def test_elements_do_not_depend_on_the_launch_size(runs, rule):
    """Element i of a run is a function of element i of its inputs alone: the first 252 elements of the 307 200-element run (a
    grid-stride loop that wraps) and of the 512-element run are the 252-element run."""
    small = runs[rule, 252, True]
    for total in (512, 307200):
        big = runs[rule, total, True]
        for k, v in small.items():
            rows = v.reshape(-1, 252) if k in ("history", "latents3") else v.reshape(1, 252)
            assert torch.equal(big[k].reshape(rows.shape[0], -1)[:, :252], rows), (total, k)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULES)
def test_malformed_calls_raise_before_the_library(gpu, rule):
    from storygen_amd import ops
    n = 128
    x, e3, l3 = torch.zeros(2, n, device=gpu), torch.zeros(6, n, device=gpu), torch.zeros(6, n, device=gpu)
    coef = H.kernel_coef(rule).to(gpu)
    mid = {"ddim": (), "ddim_var": (torch.zeros(2, n, device=gpu),), "plms": (torch.zeros(4, 2, n, device=gpu), torch.zeros(2, n, device=gpu)),
           "dpm": (torch.zeros(3, 2, n, device=gpu),)}[rule]
    fn = getattr(ops, {"ddim": "cfg_ddim_step", "ddim_var": "cfg_ddim_var_step", "plms": "cfg_plms_step", "dpm": "cfg_dpm_step"}[rule])
    with pytest.raises(ValueError):
        fn(e3, x, l3, *mid, coef[:-1].contiguous())
    with pytest.raises(ValueError):
        fn(e3, x, l3, *mid, torch.cat([coef, coef[:1]]))
    with pytest.raises(ValueError):
        fn(e3[:5].contiguous(), x, l3, *mid, coef)
    with pytest.raises(ValueError):
        fn(e3, x, l3.half(), *mid, coef)
    with pytest.raises(ValueError):
        fn(e3, x, l3[:3].contiguous(), *mid, coef)
    torch.cuda.synchronize()
    assert not x.any() and not l3.any()
    fn(e3, x, l3, *mid, coef)                      # the well-formed call goes through
    torch.cuda.synchronize()
