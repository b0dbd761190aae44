"""The update rules of the denoising loop, host side: every schedule's UpdateRule reproduces the step tables and the sequence of
`ops` calls recorded in tests/golden/step_tables.json (oracle/make_golden_step_tables.py) — exactly: it is the same host arithmetic."""
import json
import os

import pytest
import torch

import update_rule_helpers as H

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_tables.json")) as f:
    RECORDINGS = json.load(f)["recordings"]
# One recording per host arithmetic (1 ulp apart, see the helper), each made by the commit before the rules: this CPU's own is
# compared float for float.  On a CPU none was made on, the floats on file are not this machine's, and the same `==` is asked of the
# table re-assembled from the schedule's numeric API in a recording's layout
SAME_HOST_ARITHMETIC = H.host_arithmetic_fingerprint() in RECORDINGS
GOLDEN = RECORDINGS[H.host_arithmetic_fingerprint() if SAME_HOST_ARITHMETIC else min(RECORDINGS)]


def test_golden_covers_the_cases():
    for rec in RECORDINGS.values():
        assert set(rec["tables"]) == set(GOLDEN["tables"]) and set(rec["loops"]) == set(GOLDEN["loops"])
        assert all(rec["loops"][k]["calls"] == v["calls"] for k, v in GOLDEN["loops"].items())      # no float in these
    assert set(GOLDEN["tables"]) == set(H.TABLES) and set(GOLDEN["loops"]) == {f"{n}_g{G}" for n in H.LOOPS for G in (1, 5)}


@pytest.mark.parametrize("name", sorted(H.TABLES))
def test_step_table_equals_golden(name):
    got, want = H.table_of(H.TABLES[name]), GOLDEN["tables"][name]
    if not SAME_HOST_ARITHMETIC:       # this CPU rounds alphas_cumprod otherwise: the golden's layout and timesteps, this machine's scalars
        want = H.table_from_api(H.TABLES[name], want)
    assert got["row0"] == want["row0"] and len(got["rows"]) == len(want["rows"])
    for k, (g, w) in enumerate(zip(got["rows"], want["rows"])):
        assert g == w, (name, k)


@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("name", sorted(H.LOOPS))
def test_loop_makes_the_recorded_ops_calls(monkeypatch, name, G):
    got, want = H.record_calls(H.LOOPS[name], G, monkeypatch.setattr), GOLDEN["loops"][f"{name}_g{G}"]
    assert got["calls"] == want["calls"]
    if SAME_HOST_ARITHMETIC:           # the latents are fp32 arithmetic on the table's scalars
        assert got["latents"] == want["latents"]


@pytest.mark.parametrize("name", sorted(H.LOOPS))
def test_rule_is_what_the_loop_needs_to_know(name):
    """row_len / row / state / needs_noise / key of each schedule's rule, against the schedule's own numeric API."""
    cls, kw, n, eta = H.LOOPS[name]
    s = H.make_schedule(cls, kw)
    rule, ts = s.update_rule(eta), s.timesteps(n)
    var = name == "ddim_eta_clip"
    assert rule.needs_noise is var and rule.row_len == (6 if var else s.row_len) == {"ddim": 4, "ddim_eta_clip": 6, "plms": 13, "dpm": 10}[name]
    for k in range(len(ts)):
        want = [*s.var_step_coef(ts[k], n, eta), float(s.clip_sample)] if var else s.step_row(k, ts, n)
        assert rule.row(k, ts, n) == want and len(want) == rule.row_len
    state = rule.state((2, 4, 8, 8), "cpu")
    shapes = {k: tuple(v.shape) for k, v in state.items()}
    assert shapes == {"ddim": {}, "ddim_eta_clip": {}, "plms": {"history": (4, 2, 4, 8, 8), "kept": (2, 4, 8, 8)},
                      "dpm": {"history": (3, 2, 4, 8, 8)}}[name]
    assert all(v.dtype == torch.float32 and not v.any() for v in state.values())
    assert hash(rule.key) == hash(s.update_rule(eta).key) and rule.key == s.update_rule(eta).key


def test_rule_keys_tell_the_kernels_apart():
    from storygen_amd.scheduler import DDIMSchedule, DPMSolverMultistepSchedule, PNDMSchedule
    plain, clip = DDIMSchedule(), DDIMSchedule(clip_sample=True)
    assert plain.update_rule().key == plain.update_rule(0.0).key != plain.update_rule(0.5).key
    assert plain.update_rule(0.5).key == plain.update_rule(0.25).key == clip.update_rule().key      # one kernel, one row length
    pndm, dpm = PNDMSchedule(skip_prk_steps=True), DPMSolverMultistepSchedule()
    for s in (pndm, dpm):                      # eta reaches DDIM only
        assert s.update_rule(0.5).key == s.update_rule().key and not s.update_rule(0.5).needs_noise
    assert len({plain.update_rule().key, clip.update_rule().key, pndm.update_rule().key, dpm.update_rule().key}) == 4
