"""UNetEngine, StoryGenSampler and UNetTrainer on NON-SQUARE latents, against the oracle run live on the host.

Every other GPU test that builds one of the three uses a square latent, where a swap of H and W anywhere in the wiring (hw per level,
the zero-bordered [B, H+2, W+2, C] conv inputs, the NCHW ends, stride-2 / nearest-2x convolutions, the harvest plan and the flat
context buffers, _spread of the shared CFG head, the trainer's zero_stuff / sum2x2 / pad_cast) changes nothing, and where — 96x96
excepted — every level is a power of two, so the shape-dependent dispatch of engine.py always takes the same branch.  Shapes
(SD-1.5 architecture: H and W divisible by 8, (H/8)(W/8) a multiple of 8; tokens per level after the arrow):

    16x32 -> 512, 128, 32, 8      smallest non-square; deepest level 2x4
    32x16 -> 512, 128, 32, 8      the same counts transposed: a bug that only swaps H and W passes exactly one of the two
    16x96 -> 1536, 384, 96, 24    no power of two; batch 3: M = 4608, 1152, 288, 72, M % 128 = 32 and 72 at the two deepest levels
    48x32 -> 1536, 384, 96, 24    the same counts with H > W

No tolerance is new: TOL_EPS / TOL_LATENT are test_unet_gpu's, the ref_ahead and shared-head relations are those of
test_ref_ahead_batches_reference_passes_of_G_steps / test_shared_cfg_head_is_the_same_main_pass (twice the latent bar between two fp16
realisations of one trajectory), the trainer's bars those of test_backward_gpu.test_training_step_vs_oracle.  The refusals of latents
the layouts cannot hold need no device: tests/test_host_logic.py.

Measured on MI355X (first hardware run, every figure per case): profiles/r24a_unet_nonsquare_tests.txt."""
import pytest
import torch

from conftest import rel_l2
from test_unet_gpu import TOL_EPS, TOL_LATENT, _ref_and_main_inputs

pytestmark = pytest.mark.gpu

F16 = torch.float16
SHAPES = [(16, 32), (32, 16), (16, 96), (48, 32)]
GUARD = 64            # NaN rows in front of and behind every buffer the test owns


@pytest.fixture(scope="module")
def sd15(gpu):
    """(arch, state dict, the weights repacked once on the device: every engine of this file shares them)."""
    from storygen_amd.arch import SD15_CONFIG, build_arch
    from storygen_amd.engine import EngineWeights
    from storygen_amd.synth import synthetic_state_dict
    arch = build_arch(SD15_CONFIG)
    sd = synthetic_state_dict(arch, 0)
    return arch, sd, EngineWeights(arch, sd, gpu)


# ------------------------------------------------------------------------------------------------ 1, 2: engine passes and what they chose
_CHOSEN = {}          # (H, W) -> what the batch-3 engine of that shape chose (filled by the parity test; _chosen() fills what is missing)


def _record(eng, deferred):
    emit = {k: v.pstats[0][1] for k, v in eng._stats_site.items() if v.pstats}
    cannot = sorted(k for k, v in eng._stats_site.items() if not v.pstats and not v.split)
    return dict(hw=list(eng.hw), emit=emit, cannot=cannot, deferred=sorted({s for s, n in deferred if n > 1}),
                undeferred=sorted({s for s, n in deferred if n <= 1}), gn_sites=sorted(set(eng.padded) | {(0, eng.cfg["block_out_channels"][0])}))


def _watch_defer(eng):
    """Log what UNetEngine._defer_splits answers (site, K slices or 0); changes nothing."""
    log, inner = [], eng._defer_splits

    def watched(site, lvl, cout, query):
        n = inner(site, lvl, cout, query)
        log.append((site, n))
        return n
    eng._defer_splits = watched
    return log


def _chosen(gpu, sd15, H, W):
    if (H, W) not in _CHOSEN:       # run alone: the two passes on the synthetic inputs, no oracle
        from storygen_amd.engine import UNetEngine
        from storygen_amd.synth import synthetic_inputs
        arch, _, wts = sd15
        inputs = synthetic_inputs(1, 2, H, W, 1, arch.config["cross_attention_dim"])
        eng = UNetEngine(arch, None, gpu, 3, H, W, 2, weights=wts)
        log = _watch_defer(eng)
        eng.set_inputs(torch.cat([inputs["latents"]] * 3), 500, torch.cat([inputs["text"]] * 3))
        eng.forward(harvest_slot=0)
        eng.forward(harvest_slot=1)
        eng.forward(consume=True)
        torch.cuda.synchronize()
        _CHOSEN[H, W] = _record(eng, log)
    return _CHOSEN[H, W]


@pytest.mark.parametrize("H,W", SHAPES)
def test_unet_passes_vs_oracle_nonsquare(gpu, sd15, H, W):
    """test_unet_passes_vs_oracle_32x32 at HxW: 3 samples, R = 2; harvest pass (eps and all 16 features), then the main pass on the
    ORACLE's features (two distinct frames [v, 0.5 v]), each against oracle.unet_forward.  Bar: every error <= TOL_EPS."""
    from oracle import storygen_oracle as O
    from storygen_amd.engine import UNetEngine
    from storygen_amd.synth import synthetic_inputs
    arch, sd, wts = sd15
    cfg, R = arch.config, 2
    inputs = synthetic_inputs(1, R, H, W, 1, cfg["cross_attention_dim"])
    sched = O.DDIM()
    t_main = sched.timesteps(5)[0]
    ref_t, x, e, xm, em = _ref_and_main_inputs(inputs, sched, t_main)
    with torch.no_grad():
        o_eps, o_feats = O.unet_forward(sd, cfg, x, ref_t, e, None)
        ctx = {k: torch.cat([v, 0.5 * v], dim=1) for k, v in o_feats.items()}      # two distinct "frames"
        o_main, _ = O.unet_forward(sd, cfg, xm, t_main, em, ctx)
    assert tuple(o_eps.shape) == (3, 4, H, W)
    eng = UNetEngine(arch, None, gpu, 3, H, W, R, weights=wts)
    log = _watch_defer(eng)
    eng.set_inputs(x, ref_t, e)
    eps = eng.forward(harvest_slot=0).clone()
    torch.cuda.synchronize()
    errs = {"eps(ref)": rel_l2(eps.cpu(), o_eps)}
    feats = eng.features(0)
    assert len(feats) == len(o_feats) == 16
    for k, v in feats.items():
        errs[k] = rel_l2(v.float().cpu(), o_feats[k])
    for k, v in ctx.items():
        eng.ctx[k].copy_(v.to(gpu, F16))
    eng.set_inputs(xm, t_main, em)
    eps_m = eng.forward(consume=True)
    torch.cuda.synchronize()
    errs["eps(main)"] = rel_l2(eps_m.cpu(), o_main)
    assert eng.check_ln_guard() == 0
    _CHOSEN[H, W] = _record(eng, log)
    print(f"{H}x{W}", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL_EPS, errs


def test_the_shapes_reach_the_fallbacks(gpu, sd15):
    """What the engines of the four shapes chose (host-side: UNetEngine._stats_site, ops.groupnorm_plan): over the case set both
    outcomes of the producer-statistics question occur, and every GroupNorm variant the square 32x32 case runs is run here too."""
    from storygen_amd import ops
    arch, _, _ = sd15
    groups = arch.config["norm_num_groups"]
    chosen = {s: _chosen(gpu, sd15, *s) for s in SHAPES}
    for s, c in chosen.items():
        rows = sorted(set(c["emit"].values()))
        print(f"{s[0]}x{s[1]} tokens {c['hw']}: {len(c['emit'])} sites emit GroupNorm statistics (rows per partial {rows}), cannot: {c['cannot']}; "
              f"split-K reduction left to the GroupNorm at {len(c['deferred'])} sites, not at {len(c['undeferred'])}")
    # statistics wanted, launch cannot emit them -> the consumer makes its own pass: the stride-2 convolution into level 2 (640 channels
    # feeding a 960-wide concat GroupNorm) at every shape here — 16x32 / 32x16: 32 tokens per image, 16x96 / 48x32: 96; a statistics tile
    # is at least 64 rows and must divide the image.  (At 32x32 and 64x64 no site takes this branch: 64 and 256 tokens there.)
    assert any(c["cannot"] for c in chosen.values()), chosen
    assert all("down_blocks.1.downsamplers.0.conv" in c["cannot"] for c in chosen.values())
    # ... and sites that do emit them: levels 0 and 1 of every shape (512 / 128 and 1536 / 384 tokens: multiples of 64)
    assert all(c["emit"] for c in chosen.values()), chosen

    def variants(hw, sites, B=3):
        return {ops.groupnorm_plan(hw[l], ch, groups, B, True)[0] for l, ch in sites}
    sites = chosen[SHAPES[0]]["gn_sites"]
    square = variants([1024, 256, 64, 16], sites)
    print("GroupNorm variants at 32x32:", sorted(square), "here:", {s: sorted(variants(c["hw"], c["gn_sites"])) for s, c in chosen.items()})
    assert square == {"wide", "one_launch"}
    # "wide": level 0 of every shape (and every 320- / 960-channel GroupNorm: 10 / 30 channels per group); "one_launch": the 1280-channel
    # GroupNorms of levels 2 and 3 of every shape — each shape on its own runs both
    for s, c in chosen.items():
        assert c["gn_sites"] == sites and variants(c["hw"], c["gn_sites"]) >= square, s


# ------------------------------------------------------------------------------------------------ 3: batch 1, harvest-only engine
def _guarded(rows, cols, dev):
    buf = torch.full((rows + 2 * GUARD, cols), float("nan"), dtype=F16, device=dev)
    return buf, buf[GUARD:GUARD + rows]


def test_batch_1_harvest_engine_16x32_vs_oracle(gpu, sd15):
    """UNetEngine(batch 1, n_ref 0) at 16x32: M = 32 and 8 at the two deepest levels, so UNetEngine._produce meets M // 64 == 0 at the
    stride-2 convolution into level 2 (statistics wanted there: 640 channels).  On its first hardware run the forward raised there: the
    statistics buffer of (M // 64) * 2 * n_out floats is empty, an empty tensor has no address and sg_conv3x3_stats_tile_rows refuses
    a descriptor without one; _produce no longer asks where no 64-row tile can exist.  A full pass harvesting in place (HarvestPlan.direct, the
    sampler's default) into NaN-guarded buffers of the test's own: eps and the 16 features against the oracle, guards untouched; then
    a harvest_only pass whose plan copies the one sample into both frame slots of another engine's context buffers (the sampler's
    shared zero-image row as written)."""
    from oracle import storygen_oracle as O
    from storygen_amd.arch import feature_shapes
    from storygen_amd.engine import HarvestPlan, UNetEngine
    from storygen_amd.synth import synthetic_inputs
    arch, sd, wts = sd15
    cfg, H, W = arch.config, 16, 32
    inputs = synthetic_inputs(1, 2, H, W, 3, cfg["cross_attention_dim"])
    sched = O.DDIM()
    ref_t = sched.timesteps(5)[0] // 10
    x, e = sched.add_noise(inputs["image_prompts"][0], inputs["noise"], ref_t), inputs["prev_text"][0]
    with torch.no_grad():
        o_eps, o_feats = O.unet_forward(sd, cfg, x, ref_t, e, None)
    eng = UNetEngine(arch, None, gpu, 1, H, W, 0, weights=wts)
    assert eng.hw == [512, 128, 32, 8]
    bufs, ctx = {}, {}
    for k, (n, c) in feature_shapes(arch, H, W).items():
        bufs[k], view = _guarded(n, c, gpu)
        ctx[k] = view.view(1, n, c)
    plan = HarvestPlan(ctx, [(0, 0, 0, 0, 1)], slots_per_row=1, direct=True)
    assert plan.is_direct(1, 1)
    eng.set_inputs(x, ref_t, e)
    eps = eng.forward(harvest=plan).clone()
    torch.cuda.synchronize()
    assert eng.check_ln_guard() == 0
    errs = {"eps": rel_l2(eps.cpu(), o_eps)}
    for k, v in ctx.items():
        errs[k] = rel_l2(v.float().cpu(), o_feats[k])
        assert bool(torch.isnan(bufs[k][:GUARD]).all()) and bool(torch.isnan(bufs[k][-GUARD:]).all()), f"{k}: rows outside the context buffer were written"
    # whatever _produce did where M < 64, it recorded an answer for that site and handed the GroupNorm no statistics
    feed = eng._stats_site["down_blocks.1.downsamplers.0.conv"]
    assert not feed.pstats and not feed.split
    # as the sampler's reference engine does it: harvest_only, into the main engine's buffers, one sample -> both frame slots (copies)
    main = UNetEngine(arch, None, gpu, 1, H, W, 2, weights=wts)
    for v in main.ctx.values():
        v.fill_(float("nan"))
    assert eng.forward(harvest=HarvestPlan(main.ctx, [(0, 0, 0, 0, 2)]), harvest_only=True) is None
    torch.cuda.synchronize()
    for slot in (0, 1):
        for k, v in main.features(slot).items():
            errs[f"{k} slot {slot}"] = rel_l2(v.float().cpu(), o_feats[k])
    assert all(torch.equal(a, b) for a, b in zip(main.features(0).values(), main.features(1).values()))
    print("16x32 batch 1", {k: f"{v:.2e}" for k, v in errs.items()})
    assert len(errs) == 1 + 3 * 16 and max(errs.values()) <= TOL_EPS, errs


# ------------------------------------------------------------------------------------------------ 4: sampler loop
@pytest.mark.parametrize("stage", ["multi-image-condition", "auto-regressive"])
@pytest.mark.parametrize("H,W", [(16, 32), (32, 16)])
def test_loop_vs_oracle_nonsquare(gpu, sd15, H, W, stage):
    """test_loop_vs_oracle_both_stages_32x32 at HxW: R = 2, the first 2 steps of the 50-step schedule, captured graphs.  Bar: TOL_LATENT."""
    from oracle import storygen_oracle as O
    from storygen_amd.sampler import StoryGenSampler
    from storygen_amd.synth import synthetic_inputs
    arch, sd, wts = sd15
    inputs = synthetic_inputs(1, 2, H, W, 7, arch.config["cross_attention_dim"])
    want = []
    O.sample_loop(sd, arch.config, inputs, 50, stage, 7.5, 3.5, max_steps=2, trace=want)
    smp = StoryGenSampler(arch, None, gpu, 1, H, W, 2, use_graph=True, weights=wts)
    smp.prepare(inputs, 50, stage, 7.5, 3.5)
    got = []
    smp.run(max_steps=2, trace=got)
    torch.cuda.synchronize()
    smp.check_guards()
    assert len(got) == len(want) == 2 and tuple(got[0].shape) == (1, 4, H, W)
    errs = [rel_l2(a.cpu(), b) for a, b in zip(got, want)]
    print(f"{H}x{W}", stage, [f"{e:.2e}" for e in errs])
    assert max(errs) <= TOL_LATENT, (stage, errs)


def test_graph_replay_matches_eager_16x32(gpu, sd15):
    """The captured step and the eager step are the same kernels on the same buffers: bit-identical latents (test_graph_replay_matches_eager)."""
    from storygen_amd.sampler import StoryGenSampler
    from storygen_amd.synth import synthetic_inputs
    arch, _, wts = sd15
    inputs = synthetic_inputs(1, 2, 16, 32, 5, arch.config["cross_attention_dim"])
    outs = []
    for use_graph in (False, True):
        smp = StoryGenSampler(arch, None, gpu, 1, 16, 32, 2, use_graph=use_graph, weights=wts)
        smp.prepare(inputs, 4, "auto-regressive", 7.5, 3.5)
        outs.append(smp.run().clone())
        torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_ref_ahead_2_is_the_same_trajectory_16x32(gpu, sd15):
    """ref_ahead = 2 against the step-by-step schedule over three groups, under the relation of
    test_ref_ahead_batches_reference_passes_of_G_steps: the batched reference pass has other tile / split-K plans, so the two are two fp16
    realisations of one trajectory — every latent within twice the latent bar of the other's."""
    from storygen_amd.sampler import StoryGenSampler
    from storygen_amd.synth import synthetic_inputs
    arch, _, wts = sd15
    inputs = synthetic_inputs(1, 2, 16, 32, 13, arch.config["cross_attention_dim"])
    G, traces = 2, []
    n = 3 * G
    for g in (1, G):
        smp = StoryGenSampler(arch, None, gpu, 1, 16, 32, 2, use_graph=True, weights=wts, ref_ahead=g)
        smp.prepare(inputs, 50, "multi-image-condition", 7.5, 3.5)
        assert smp.U == g * smp.U0 and len(smp.ctx_sets) == 2 * g
        assert smp.group == (g > 1) and (not smp.group or (smp.group_direct and len(smp.graphs) == 2))
        tr = []
        smp.run(max_steps=n, trace=tr)
        torch.cuda.synchronize()
        smp.check_guards()
        assert len(tr) == n
        traces.append([t.cpu() for t in tr])
    errs = [rel_l2(a, b) for a, b in zip(traces[1], traces[0])]
    print("16x32 ref_ahead=2 vs step-by-step, per step:", [f"{e:.1e}" for e in errs])
    assert max(errs) <= 2 * TOL_LATENT, errs


# ------------------------------------------------------------------------------------------------ 5: shared CFG head
@pytest.mark.parametrize("stage", ["multi-image-condition", "auto-regressive"])
def test_shared_cfg_head_is_the_same_main_pass_16x32(gpu, sd15, stage):
    """test_shared_cfg_head_is_the_same_main_pass at 16x32 (UNetEngine._spread with rows = n * hw[0] on a non-square level 0): the pass
    that runs the head once against the batch-3 pass, under that test's relation — twice the latent bar over three steps — and with
    fewer FLOPs executed."""
    from storygen_amd import ops
    from storygen_amd.sampler import StoryGenSampler
    from storygen_amd.synth import synthetic_inputs
    arch, _, wts = sd15
    inputs = synthetic_inputs(1, 2, 16, 32, 29, arch.config["cross_attention_dim"])
    traces, flops = [], []
    for head in (False, True):
        smp = StoryGenSampler(arch, None, gpu, 1, 16, 32, 2, use_graph=True, weights=wts, shared_head=head)
        smp.prepare(inputs, 50, stage, 7.5, 3.5)
        assert smp.main.cfg_shared_head == head
        tr = []
        smp.run(max_steps=3, trace=tr)
        torch.cuda.synchronize()
        traces.append([t.cpu() for t in tr])
        sink = []
        ops.PROFILE_SINK = sink
        try:
            smp._main_pass(0)
            torch.cuda.synchronize()
        finally:
            ops.PROFILE_SINK = None
        flops.append(sum(f for _, f, _, _, _ in sink))
        smp.check_guards()
    errs = [rel_l2(a, b) for a, b in zip(traces[1], traces[0])]
    print("16x32", stage, "shared head vs batch 3, per step:", [f"{e:.1e}" for e in errs], f"main-pass GFLOP {flops[0] / 1e9:.2f} -> {flops[1] / 1e9:.2f}")
    assert all(torch.isfinite(t).all() for t in traces[1])
    assert max(errs) <= 2 * TOL_LATENT, errs
    assert flops[1] < flops[0]


# ------------------------------------------------------------------------------------------------ 6: trainer
def _two_level():
    from storygen_amd.arch import build_arch, load_config
    cfg = load_config(dict(block_out_channels=(320, 640), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
                           up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), cross_attention_dim=768, attention_head_dim=8,
                           sample_size=128))
    return cfg, build_arch(cfg)


def _train_batch(H, W, seed):
    """synthetic_train_batch draws squares: the HxW batch is the top-left window of the 24x24 one (latents, noises and the loss mask)."""
    from storygen_amd.synth import synthetic_train_batch
    spatial = ("latents", "ref_latents", "noise", "ref_noise", "mask")
    return {k: (v[..., :H, :W].contiguous() if k in spatial else v) for k, v in synthetic_train_batch(2, 24, 768, seed).items()}


def _check_step(loss, grads, want_loss, want, tag):
    from test_backward_gpu import rel
    errs = {k: rel(grads[k].cpu(), want[k]) for k in want if k in grads}
    print(tag, f"loss {float(loss):.6f} vs {float(want_loss):.6f}; worst gradients:", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    assert abs(float(loss) - float(want_loss)) <= 2e-3 * abs(float(want_loss))
    assert set(grads) == set(want)
    assert max(errs.values()) < 1e-2


@pytest.mark.parametrize("H,W", [(16, 24), (24, 16)])
def test_training_step_vs_oracle_nonsquare(gpu, H, W):
    """test_training_step_vs_oracle (2-level UNet, batch 2, three reference frames) at HxW — 384 and 96 tokens: the batched reference
    pass, the main pass and the backward walk (_down / _down_bwd / _up / _up_bwd: zero_stuff, sum2x2, pad_cast) with H != W."""
    from oracle import storygen_oracle as O
    from storygen_amd.synth import synthetic_state_dict
    from storygen_amd.train import UNetTrainer
    cfg, arch = _two_level()
    sd = synthetic_state_dict(arch, 7)
    batch = _train_batch(H, W, 7)
    want_loss, want = O.train_step(sd, cfg, batch, (0, 1, 2))
    tr = UNetTrainer(arch, sd, gpu, 2, H, W, n_ref=3)
    loss, grads = tr.train_step(batch, (0, 1, 2))
    torch.cuda.synchronize()
    assert all(".attn3." in k for k in grads)
    _check_step(loss, grads, want_loss, want, f"{H}x{W} stage 2,")


def test_stage1_training_step_vs_oracle_16x24(gpu):
    """test_stage1_training_step_vs_oracle at 16x24: no reference pass, no image context, the attn1 gradients."""
    from oracle import storygen_oracle as O
    from storygen_amd.synth import synthetic_state_dict
    from storygen_amd.train import UNetTrainer
    cfg, arch = _two_level()
    sd = synthetic_state_dict(arch, 7)
    batch = {k: v for k, v in _train_batch(16, 24, 7).items() if k not in ("ref_latents", "ref_noise", "prev_text")}
    want_loss, want = O.train_step(sd, cfg, batch, (), trainable="attn1")
    tr = UNetTrainer(arch, sd, gpu, 2, 16, 24, n_ref=0, trainable="attn1")
    loss, grads = tr.train_step(batch, ())
    torch.cuda.synchronize()
    assert all(".attn1." in k for k in grads)
    _check_step(loss, grads, want_loss, want, "16x24 stage 1,")
