"""The CPU half of the stand-in conformance (tests/standin_cases.py; the hardware half is tests/test_standin_conformance_gpu.py):
  - every public entry point of the hand-written stand-in modules takes what the real storygen_amd.ops entry point takes: the same
    positional parameters, no keyword the real op lacks, the same defaults, and every keyword of the real op it does NOT take listed in
    NOT_EMULATED — a new keyword on the real op fails here until someone decides what the stand-in does with it;
  - every case of the table runs through its stand-ins here and lands inside the op's bar against float64, with the NaN guards intact
    and the expected elements written, so the table is well-formed before it reaches a card;
  - the table names every public entry point of the four modules; the refused argument sets are refused by the stand-ins."""
import importlib
import inspect

import pytest
import torch

import standin_cases as S
from storygen_amd import ops

# keywords of the real op that a stand-in does not accept (launch selection, fused producers / consumers nobody emulates on the CPU)
NOT_EMULATED = {
    ("fake_ops", "gemm"): {"ln", "ln_out", "guard"},
    ("ops_emulation", "gemm"): {"ln", "ln_out", "guard"},
    ("fake_ops", "conv3x3"): {"defer_reduce"},
    ("ops_emulation", "conv3x3"): {"defer_reduce"},
    ("fake_ops", "groupnorm"): {"split"},
    ("ops_emulation", "groupnorm"): {"split"},
    ("clip_ops_emulation", "clip_patchify"): {"kpad"},
}
# host-only size queries the trainer calls beside the ops: a stand-in returns a placeholder size, there is no kernel to conform to
HOST_QUERIES = {"gemm_workspace_bytes", "groupnorm_workspace_bytes", "groupnorm_bwd_workspace_bytes"}
DESC = {"gemm": ops._gemm_desc, "conv3x3": ops._conv_desc}            # the **kw wrappers take their keywords here


def entry_points(module):
    m = importlib.import_module("tests." + module)
    return {n: f for n, f in vars(m).items() if inspect.isfunction(f) and not n.startswith("_") and hasattr(ops, n)}


PAIRS = [(m, n) for m in S.MODULES for n in sorted(entry_points(m))]


def _split(fn):
    ps = inspect.signature(fn).parameters.values()
    assert not any(p.kind in (p.VAR_POSITIONAL, p.VAR_KEYWORD) for p in ps), f"{fn.__name__} takes * / **"
    return [p.name for p in ps if p.default is p.empty], {p.name: p.default for p in ps if p.default is not p.empty}


@pytest.mark.parametrize("module,name", PAIRS)
def test_signature_matches_the_real_op(module, name):
    pos, kw = _split(entry_points(module)[name])
    real_pos, real_kw = _split(DESC.get(name, getattr(ops, name)))
    assert pos == real_pos, f"{module}.{name}: positional parameters {pos}, ops.{name} takes {real_pos}"
    for k, default in kw.items():
        assert k in real_kw, f"{module}.{name} accepts {k}=, ops.{name} does not"
        assert default == real_kw[k] and type(default) is type(real_kw[k]), f"{module}.{name}: {k}={default!r}, ops.{name} has {real_kw[k]!r}"
    assert set(real_kw) - set(kw) == NOT_EMULATED.get((module, name), set()), \
        f"{module}.{name}: keywords of ops.{name} it does not take {sorted(set(real_kw) - set(kw))} != NOT_EMULATED {sorted(NOT_EMULATED.get((module, name), set()))}"


def test_not_emulated_holds_no_stale_entry():
    assert set(NOT_EMULATED) <= set(PAIRS)
    assert all(NOT_EMULATED.values())


def test_every_entry_point_has_a_case():
    named = {(m, c.op) for c in S.CASES for m in c.modules}
    missing = [p for p in PAIRS if p not in named and p[1] not in HOST_QUERIES]
    assert not missing, f"no conformance case for {missing}"
    for c in S.CASES + S.REFUSED:
        for m in c.modules:
            assert c.op in entry_points(m), f"{c.name}: {m} has no {c.op}"
    assert len({c.name for c in S.CASES + S.REFUSED}) == len(S.CASES + S.REFUSED)


def _standins(case):
    """(module, function) per distinct body: a module that re-exports another's function is the same stand-in."""
    seen, out = set(), []
    for m in case.modules:
        fn = S.standin(m, case.op)
        if fn not in seen:
            seen.add(fn)
            out.append((m, fn))
    return out


@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_standin_agrees_with_float64(case):
    for module, fn in _standins(case):
        call = case.build(S.gen_for(case))
        want = call.ref()
        for n, v in call.outs.items():             # the case itself: outputs start as NaN, in-place operands finite
            assert bool(torch.isnan(v.float()).all()) != (n in call.inplace), f"{case.name}: {n} prefill"
        ret = S.returned(fn(*call.args, **call.kwargs), call.args)
        lines, fails = S.check_side(module, call, call.outs, want, ret)
        print(f"STANDIN {case.name}: " + "; ".join(lines))
        assert not fails, f"{case.name}: " + "; ".join(fails)


@pytest.mark.parametrize("case", S.REFUSED, ids=repr)
def test_standin_refuses(case):
    for module, fn in _standins(case):
        call = case.build(S.gen_for(case))
        with pytest.raises((AssertionError, ValueError)):
            fn(*call.args, **call.kwargs)
        assert all(bool(torch.isnan(S.backing(v).float()).all()) for v in call.outs.values()), f"{module}: wrote before refusing"
