"""The tests' CPU stand-ins of storygen_amd.ops held to the real kernels (cases: tests/standin_cases.py).  Host logic — engine layouts,
weight folds, the training tape, the sampler's update rules — is checked on machines without a GPU against tests/fake_ops.py and
tests/ops_emulation.py (and, through it, the CLIP and PickScore emulations); a stand-in that drifts from its kernel lets wrong host
code pass there.  Per case and stand-in, the real op runs on device copies of the very same bits, with the same view structure:
  (a) the same elements are written: isnan of every backing buffer is identical on the two sides, guards around in-place operands intact;
  (b) kernel and stand-in agree within the project's bar for that op (torch.equal for copies, transposes and gathers);
  (c) each side is inside the same bar against a float64 evaluation of the expression, so a failure of (b) names the wrong side;
  (d) both return the same argument, and mutated state (history rings, kept, loss, lse2, ld2) follows (a) - (c) like any output.
Argument sets a stand-in refuses are refused by the real op with a ValueError before any launch.
Measured errors of the first hardware run: profiles/r27a_standin_conformance.txt (pytest -s prints them)."""
import pytest
import torch

import standin_cases as S
from conftest import max_rel, rel_l2
from test_standin_signatures import _standins

pytestmark = pytest.mark.gpu


def _agree(got, ref, bar):
    """(b): the kernel's tensor against the stand-in's, on the elements both wrote."""
    m = ~torch.isnan(ref.float())
    a, b = got[m], ref[m]
    if bar[0] == "equal":
        return bool(torch.equal(a, b)), "equal" if torch.equal(a, b) else "NOT equal"
    if bar[0] == "abs":
        e = float((a.double() - b.double()).abs().max())
        return e <= bar[1], f"max-abs {e:.1e}"
    e2, em = rel_l2(a, b), max_rel(a, b)
    return e2 <= bar[1] and (bar[2] is None or em <= bar[2]), f"rel-L2 {e2:.1e} max-rel {em:.1e}"


@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_standin_conforms_to_the_kernel(gpu, case):
    from storygen_amd import ops
    for module, fn in _standins(case):
        call = case.build(S.gen_for(case))
        want = call.ref()
        cache = {}
        g_args, g_kwargs, g_outs = (S.mirror(o, gpu, cache) for o in (call.args, call.kwargs, call.outs))
        c_ret = S.returned(fn(*call.args, **call.kwargs), call.args)
        g_ret = S.returned(getattr(ops, case.op)(*g_args, **g_kwargs), g_args)
        torch.cuda.synchronize()
        fails = []
        # (a) the same elements written, buffer by buffer
        for names, views in S.by_storage(call.outs):
            c_nan, g_nan = torch.isnan(S.backing(views[0]).float()), torch.isnan(S.backing(g_outs[names[0]]).float()).cpu()
            if not torch.equal(c_nan, g_nan):
                fails.append(f"(a) {' / '.join(names)}: the kernel wrote {int((~g_nan).sum())} elements of the buffer, {module} {int((~c_nan).sum())}")
        # (c) each side against float64 (guards and NaN pattern included), (d) the returned argument
        h_outs = S.mirror(g_outs, "cpu", {})
        lines = []
        for who, outs, ret in ((module, call.outs, c_ret), ("kernel", h_outs, g_ret)):
            ln, fl = S.check_side(who, call, outs, want, ret)
            lines += ln
            fails += [f"(c) {f}" for f in fl]
        # (b) kernel against stand-in
        for n, v in call.outs.items():
            ok, text = _agree(h_outs[n], v, call.bars[n])
            lines.append(f"kernel vs {module} {n}: {text}")
            if not ok:
                fails.append(f"(b) {n}: kernel vs {module} {text} outside {call.bars[n]}")
        print(f"CONFORM {case.name}: " + "; ".join(lines))
        assert not fails, f"{case.name} [{module}]: " + "; ".join(fails)


@pytest.mark.parametrize("case", S.REFUSED, ids=repr)
def test_refused_by_both(gpu, case):
    from storygen_amd import ops
    for module, fn in _standins(case):
        call = case.build(S.gen_for(case))
        cache = {}
        g_args, g_kwargs, g_outs = (S.mirror(o, gpu, cache) for o in (call.args, call.kwargs, call.outs))
        with pytest.raises((AssertionError, ValueError)):
            fn(*call.args, **call.kwargs)
        with pytest.raises(ValueError):
            getattr(ops, case.op)(*g_args, **g_kwargs)
        torch.cuda.synchronize()
        for n, v in g_outs.items():
            assert bool(torch.isnan(S.backing(v).float()).all()), f"{case.name}: the refused call wrote into {n}"
