"""Multistep DPM-Solver (diffusers 0.13.1 DPMSolverMultistepScheduler) on the host, no GPU: config handling, the timestep rule, the
per-call table the update kernel consumes (storygen_amd.scheduler.DPMSolverMultistepSchedule.step_row) against the stateful
restatement in tests/dpm_restatement.py (parity unpinned against diffusers, see there), order 1 against DDIM, and the host-side
validation of the C entry point."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dpm_restatement import DPMSolverMultistep, apply_row, dpm_on_ddim_timesteps

NS = (1, 2, 5, 14, 15, 20, 25, 50)
SD_CFG = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", trained_betas=None)


# ------------------------------------------------------------------------------------------------ config handling
def test_schedule_from_config_builds_dpm_solver():
    from storygen_amd.scheduler import DPMSolverMultistepSchedule, schedule_from_config
    s = schedule_from_config(dict(SD_CFG, _class_name="DPMSolverMultistepScheduler", solver_order=3, algorithm_type="dpmsolver",
                                  solver_type="heun", lower_order_final=False, thresholding=False, prediction_type="epsilon"))
    assert type(s) is DPMSolverMultistepSchedule and s.kind == "dpm" and s.row_len == 10
    assert (s.solver_order, s.algorithm_type, s.solver_type, s.lower_order_final) == (3, "dpmsolver", "heun", False)
    # attribute-style config, class named by the object (the pipeline passes type(scheduler).__name__)
    s2 = schedule_from_config(SimpleNamespace(**SD_CFG), "DPMSolverMultistepScheduler")
    assert type(s2) is DPMSolverMultistepSchedule and s2.key() == DPMSolverMultistepSchedule().key()
    assert (s2.solver_order, s2.algorithm_type, s2.solver_type, s2.lower_order_final) == (2, "dpmsolver++", "midpoint", True)
    assert torch.equal(s2.alphas_cumprod, DPMSolverMultistepSchedule().alphas_cumprod)


def test_dpm_from_config_of_a_ddim_or_pndm_config():
    """`DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)`: the DDIM / PNDM-only keys are ignored."""
    from storygen_amd.scheduler import DDIMSchedule, DPMSolverMultistepSchedule, PNDMSchedule
    for src in (DDIMSchedule().config, PNDMSchedule(skip_prk_steps=True).config):
        s = DPMSolverMultistepSchedule.from_config(src)
        assert s.key() == DPMSolverMultistepSchedule().key()
        assert not {"steps_offset", "set_alpha_to_one", "clip_sample", "skip_prk_steps"} & set(s.config)
    s = DPMSolverMultistepSchedule.from_config(DDIMSchedule().config, solver_order=3)
    assert s.solver_order == 3 and s.config["solver_order"] == 3


def test_dpm_rejects_what_it_does_not_implement():
    from storygen_amd.scheduler import DPMSolverMultistepSchedule, schedule_from_config
    with pytest.raises(NotImplementedError, match="thresholding"):
        DPMSolverMultistepSchedule(thresholding=True)
    with pytest.raises(NotImplementedError, match="thresholding"):
        schedule_from_config(dict(SD_CFG, _class_name="DPMSolverMultistepScheduler", thresholding=True))
    with pytest.raises(NotImplementedError, match="prediction_type"):
        DPMSolverMultistepSchedule(prediction_type="v_prediction")
    with pytest.raises(NotImplementedError, match="unsupported scheduler config keys"):
        DPMSolverMultistepSchedule(use_karras_sigmas=True)
    with pytest.raises(NotImplementedError):
        DPMSolverMultistepSchedule(solver_order=4)
    with pytest.raises(NotImplementedError):
        DPMSolverMultistepSchedule(algorithm_type="sde-dpmsolver++")
    with pytest.raises(NotImplementedError):
        DPMSolverMultistepSchedule(solver_type="bh2")
    for name in ("EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler", "LMSDiscreteScheduler", "DPMSolverSinglestepScheduler"):
        with pytest.raises(NotImplementedError, match=name):
            schedule_from_config(dict(SD_CFG, _class_name=name))


def test_dpm_save_pretrained_round_trip(tmp_path):
    from storygen_amd.scheduler import DPMSolverMultistepSchedule
    s = DPMSolverMultistepSchedule(solver_order=3, solver_type="heun", trained_betas=torch.linspace(1e-4, 2e-2, 1000).tolist())
    s.save_pretrained(str(tmp_path / "scheduler"))
    cfg = json.loads((tmp_path / "scheduler" / "scheduler_config.json").read_text())
    assert cfg["_class_name"] == "DPMSolverMultistepScheduler" and cfg["thresholding"] is False and cfg["solver_order"] == 3
    assert not {"steps_offset", "set_alpha_to_one", "clip_sample", "skip_prk_steps"} & set(cfg)
    back = DPMSolverMultistepSchedule.from_pretrained(str(tmp_path))
    assert back.key() == s.key() and torch.equal(back.alphas_cumprod, s.alphas_cumprod)
    assert back.key() != DPMSolverMultistepSchedule().key()


# ------------------------------------------------------------------------------------------------ timesteps
def test_dpm_timesteps_are_the_linspace_rule():
    from storygen_amd.scheduler import DPMSolverMultistepSchedule
    s = DPMSolverMultistepSchedule()
    for n in NS:
        want = np.linspace(0, 999, n + 1).round()[::-1][:-1].astype(np.int64).tolist()
        assert s.timesteps(n) == want and len(want) == n, n
    assert s.timesteps(20)[:3] == [999, 949, 899] and s.timesteps(20)[-1] == 50
    assert s.timesteps(2) == [999, 500]                                        # round half to even (499.5)


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("algo", ["dpmsolver++", "dpmsolver"])
@pytest.mark.parametrize("solver_type", ["midpoint", "heun"])
@pytest.mark.parametrize("lower_order_final", [True, False])
def test_dpm_table_reproduces_the_stateful_rule(order, algo, solver_type, lower_order_final):
    """Each step_row, executed in float64 exactly as sg_cfg_dpm_step_f32 executes it (3-slot ring of converted model outputs),
    against the stateful restatement of DPMSolverMultistepScheduler.step over random epsilon sequences."""
    from storygen_amd.scheduler import DPMSolverMultistepSchedule
    kw = dict(solver_order=order, algorithm_type=algo, solver_type=solver_type, lower_order_final=lower_order_final)
    g = torch.Generator().manual_seed(order * 7 + len(algo) + len(solver_type) + lower_order_final)
    for n in NS:
        s, ref = DPMSolverMultistepSchedule(**kw), DPMSolverMultistep(**kw)
        ts = s.timesteps(n)
        x = torch.randn(4, 8, generator=g, dtype=torch.float64)
        xr = x.clone()
        hist = torch.full((3, 4, 8), float("nan"), dtype=torch.float64)        # unread slots must not matter
        orders = []
        for k, t in enumerate(ts):
            e = torch.randn(4, 8, generator=g, dtype=torch.float64)
            orders.append(s.order_at(k, len(ts)))
            x = apply_row(s.step_row(k, ts, n), e, x, hist)
            xr = ref.step(e, t, xr, n)
            err = float((x - xr).norm() / xr.norm())
            assert err <= 1e-5, (n, k, err)
            assert torch.isfinite(x).all()
        lof = lower_order_final and len(ts) < 15
        want = [1] + [min(order, k + 1) for k in range(1, len(ts))]
        if lof:
            want[-1] = 1
            if order == 3 and len(ts) >= 2:
                want[-2] = min(want[-2], 2)
        assert orders == want, (n, orders)


def test_dpm_rows_are_linear_and_keep_the_ring_disjoint():
    from storygen_amd.scheduler import DPMSolverMultistepSchedule
    s = DPMSolverMultistepSchedule(solver_order=3)
    ts = s.timesteps(25)
    for k in range(len(ts)):
        row = s.step_row(k, ts, 25)
        assert len(row) == s.row_len and all(np.isfinite(row))
        cur, s1, s2 = int(row[6]), int(row[7]), int(row[8])
        assert cur == k % 3 and cur not in (s1, s2) and s1 != s2 and row[9] == 1.0
        assert (row[4] != 0.0) == (k >= 1) and (row[5] != 0.0) == (k >= 2)   # history weights exist only where history does


def test_order_one_dpm_solver_pp_is_ddim():
    """First-order DPM-Solver++ is DDIM (eta = 0): on DDIM's timesteps the order-1 rows give DDIM's update, the last step
    included (to alphas_cumprod[0], which is DDIM's final_alpha_cumprod with set_alpha_to_one = false)."""
    from storygen_amd.scheduler import DDIMSchedule
    ddim = DDIMSchedule()
    for n in (1, 2, 5, 20, 50):
        s = dpm_on_ddim_timesteps()
        ts = s.timesteps(n)
        g = torch.Generator().manual_seed(n)
        x = torch.randn(4, 8, generator=g, dtype=torch.float64)
        xd = x.clone()
        hist = torch.zeros(3, 4, 8, dtype=torch.float64)
        for k, t in enumerate(ts):
            e = torch.randn(4, 8, generator=g, dtype=torch.float64)
            row = s.step_row(k, ts, n)
            assert row[4] == 0.0 and row[5] == 0.0
            x = apply_row(row, e, x, hist)
            sa, sb, pa, pb = ddim.step_coef(t, n)
            xd = pa * ((xd - sb * e) / sa) + pb * e
            err = float((x - xd).norm() / xd.norm())
            assert err <= 1e-6, (n, k, err)
    assert ddim.step_coef(1, 50)[2] == pytest.approx(float(ddim.alphas_cumprod[0] ** 0.5))


def test_sampler_table_rows_carry_the_dpm_row():
    from storygen_amd.sampler import step_table
    from storygen_amd.scheduler import DPMSolverMultistepSchedule
    s = DPMSolverMultistepSchedule()
    ts = s.timesteps(20)
    units0 = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 2, 0)]
    rows, row0 = step_table(s, ts, 20, units0, 3, "multi-image-condition", 3, 5, True, 3.5, 7.5)
    U = 5 * len(units0)
    assert len(rows) == 20 and all(len(r) == len(row0) == 3 * U + 3 + 2 + 10 for r in rows)
    for k, r in enumerate(rows):
        assert r[3 * U + 3:3 * U + 5] == [3.5, 7.5] and r[3 * U + 5:] == s.step_row(k, ts, 20)
        assert r[U] == float(ts[k])
    assert row0[:len(units0)] == [99.0] * len(units0)                          # ref_t = (999 / 10).long()


def test_dpm_entry_point_validates_on_the_host():
    """sg_cfg_dpm_step_f32 refuses null pointers and empty shapes with SG_EINVAL before anything is launched."""
    from storygen_amd import _lib
    from storygen_amd.build import build
    build(force=False, verbose=False)
    lib = _lib.load()
    P = 0x10000
    assert lib.sg_cfg_dpm_step_f32(None, P, P, P, P, 1, 256, None) == -1
    assert b"sg_cfg_dpm_step" in lib.sg_last_error()
    assert lib.sg_cfg_dpm_step_f32(P, None, P, P, P, 1, 256, None) == -1
    assert lib.sg_cfg_dpm_step_f32(P, P, P, None, P, 1, 256, None) == -1
    assert lib.sg_cfg_dpm_step_f32(P, P, P, P, None, 1, 256, None) == -1
    assert lib.sg_cfg_dpm_step_f32(P, P, P, P, P, 0, 256, None) == -1
    assert lib.sg_cfg_dpm_step_f32(P, P, P, P, P, -1, 256, None) == -1
    assert lib.sg_cfg_dpm_step_f32(P, P, P, P, P, 1, 0, None) == -1


def test_dpm_ops_wrapper_checks_before_the_library():
    from storygen_amd import ops
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(TypeError):
        ops.cfg_dpm_step(torch.zeros(3, 4, 8, 8), x, None, torch.zeros(3, 1, 4, 8, 8), torch.zeros(12))
