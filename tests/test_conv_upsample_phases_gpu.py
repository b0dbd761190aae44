"""The phase form of the upsampling convolution (sg_conv3x3_desc.upsample2x = 2, mma_phase_kernel): nearest-2x upsampling + 3x3
convolution computed as four 2x2 convolutions of the input-resolution image on packed tap sums (repack.upsample_phase_pack).

Yardstick of the kernel tests: the same four 2x2 convolutions in float64 on the SAME fp16 input and the SAME packed fp16 weights — the
operands are identical and only the accumulation differs, so the bars are those tests/test_kernels_gpu.py holds the upsampling entries
of CONV_CASES to (fp32 output: rel-L2 2e-6 / max-rel 2e-5, test_conv3x3_padded_input_all_tiles; fp16 output: 1e-3 / 3e-3).  Shapes: the
smallest that reach the tap / channel-block wrap (two channel blocks), a partial 128-wide column tile, the sample boundary, one 64-row
tile per phase and sample (8x8), a 256-row tile that is exactly one phase image (16x16) and a non-square image."""
import pytest
import torch

from conftest import rel_l2
from test_kernels_gpu import check, rnd
from test_upsample_phase_pack import phase_conv

pytestmark = pytest.mark.gpu

F32_BAR = dict(l2=2e-6, mx=2e-5)        # test_conv3x3_padded_input_all_tiles

# B, H, W, Cin, Cout, tile
PHASE_CASES = [
    (2, 8, 8, 128, 192, (64, 128)),     # H W = 64: one 64-row tile per phase and sample; 2 channel blocks; columns 128 + 64; 2 samples
    (2, 8, 8, 128, 192, None),          # the planner's own tile
    (1, 16, 16, 64, 64, (256, 128)),    # H W = BM exactly
    (1, 8, 16, 64, 64, (128, 128)),     # non-square: a phase image is one 128-row tile
    (1, 8, 16, 64, 72, (64, 64)),       # ... and two 64-row tiles, Cout no multiple of 64
]


def _problem(gpu, B, H, W, Cin, Cout, exact=False):
    x = rnd((B, H, W, Cin), gpu, seed=1)
    if exact:       # small multiples of 2^-6: every tap sum is an fp16 number, the pack loses nothing against the 3x3 weights
        g = torch.Generator().manual_seed(2)
        w = (torch.randint(-3, 4, (Cout, Cin, 3, 3), generator=g).float() / 64).to(torch.float16).to(gpu)
    else:
        w = rnd((Cout, Cin, 3, 3), gpu, (9 * Cin) ** -0.5, seed=2)
    bias = rnd((Cout,), gpu, seed=3) + 2.0
    from storygen_amd import ops, repack
    xp = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.float16, device=gpu)
    ops.pad_cast(x, xp)
    wp = repack.upsample_phase_pack(w)
    ref = phase_conv(x.permute(0, 3, 1, 2).double().cpu(), wp.double().cpu()) + bias.double().cpu()[None, :, None, None]
    return xp, w.permute(0, 2, 3, 1).contiguous(), wp, bias, ref            # ref [B, Cout, 2H, 2W] float64


def _check_everywhere(out_nhwc, ref, what, **bar):
    """The whole image, each of the four parities, and the one-pixel frame (where the taps read the zero border)."""
    o = out_nhwc.permute(0, 3, 1, 2).float().cpu()
    check(o, ref, what, **bar)
    for a in range(2):
        for b in range(2):
            check(o[:, :, a::2, b::2], ref[:, :, a::2, b::2], f"{what}, parity ({a}, {b})", **bar)
    frame = torch.ones(ref.shape[2], ref.shape[3], dtype=torch.bool)
    frame[1:-1, 1:-1] = False
    check(o[:, :, frame], ref[:, :, frame], f"{what}, frame", **bar)
    for cy in (0, -1):
        for cx in (0, -1):
            check(o[:, :, cy, cx], ref[:, :, cy, cx], f"{what}, corner ({cy}, {cx})", **bar)


@pytest.mark.parametrize("B,H,W,Cin,Cout,tile", PHASE_CASES)
def test_phase_form_fp32_output(gpu, B, H, W, Cin, Cout, tile):
    from storygen_amd import ops
    xp, _, wp, bias, ref = _problem(gpu, B, H, W, Cin, Cout)
    out = torch.full((B, 2 * H, 2 * W, Cout), float("nan"), dtype=torch.float32, device=gpu)
    kw = dict(bias=bias, x_padded=True, tile=tile)
    assert ops.conv3x3_phases_fit(xp, wp, out, **kw)
    bm = ops.conv3x3_launch_plan(xp, wp, out, upsample2x=2, **kw)[0]
    assert (H * W) % bm == 0 and (tile is None or bm == tile[0])
    ops.conv3x3(xp, wp, out, upsample2x=2, **kw)
    _check_everywhere(out, ref, f"phase form {B}x{H}x{W} {Cin}->{Cout} tile {tile}", **F32_BAR)


def test_phase_form_fp16_output_without_bias(gpu):
    from storygen_amd import ops
    B, H, W, Cin, Cout = 2, 8, 8, 128, 192
    xp, _, wp, bias, ref = _problem(gpu, B, H, W, Cin, Cout)
    out = torch.full((B, 2 * H, 2 * W, Cout), float("nan"), dtype=torch.float16, device=gpu)
    ops.conv3x3(xp, wp, out, upsample2x=2, x_padded=True)
    _check_everywhere(out, ref - bias.double().cpu()[None, :, None, None], "phase form, fp16 output")


@pytest.mark.parametrize("B,H,W,Cin,Cout,tile,split", [(2, 8, 8, 128, 192, (64, 128), 1), (1, 16, 16, 64, 64, (256, 128), 1),
                                                       (2, 8, 8, 128, 128, (64, 128), 2)])
def test_groupnorm_partials_of_the_phase_form(gpu, B, H, W, Cin, Cout, tile, split):
    """Per sample and channel, the merged partials (sum, sum of squares) are the column sums of the launch's own fp32 output (the bar
    test_groupnorm_statistics_from_producer_epilogues holds partials to, rel-L2 1e-6), in the count the consumer expects (4 H W / rows per
    sample, sample-major); and on weights whose tap sums are exact in fp16 — both forms then compute the same products — they are
    those of the upsample2x = 1 launch on the same data to the same bar.  split = 2: from the split-K second pass."""
    from storygen_amd import ops
    xp, w3, wp, bias, _ = _problem(gpu, B, H, W, Cin, Cout, exact=True)
    HWo, M = 4 * H * W, 4 * B * H * W
    ws = torch.empty(max(16, ops.gemm_workspace_bytes(M, Cout, 4)), dtype=torch.uint8, device=gpu)
    merged, outs = [], []
    for mode, w in ((2, wp), (True, w3)):
        out = torch.full((B, 2 * H, 2 * W, Cout), float("nan"), dtype=torch.float32, device=gpu)
        st = torch.full((M // 64 * 2 * Cout,), float("nan"), dtype=torch.float32, device=gpu)
        kw = dict(bias=bias, x_padded=True, upsample2x=mode, workspace=ws, tile=tile if mode == 2 else None, split_k=split if mode == 2 else 0)
        rows = ops.conv3x3_stats_rows(xp, w, out, stats=st, **kw)
        assert rows in (64, 128, 256) and HWo % rows == 0
        if mode == 2:
            assert ops.conv3x3_planned_splits(xp, w, out, **kw) == split
        ops.conv3x3(xp, w, out, stats=st, **kw)
        torch.cuda.synchronize()
        got = st[: M // rows * 2 * Cout].view(B, HWo // rows, 2, Cout).double().sum(1)            # the consumer's merge: per sample
        y = out.view(B, HWo, Cout).double()
        own = torch.stack([y.sum(1), (y * y).sum(1)], 1)
        e = rel_l2(got[:, 0], own[:, 0]), rel_l2(got[:, 1], own[:, 1])
        print(f"mode {mode}: rows {rows}, partials vs own output: sum {e[0]:.2e}, squares {e[1]:.2e}")
        assert max(e) < 1e-6
        merged.append(got)
        outs.append(out)
    check(outs[0], outs[1], "phase form vs 3x3 form on exactly packed weights", **F32_BAR)
    e = rel_l2(merged[0][:, 0], merged[1][:, 0]), rel_l2(merged[0][:, 1], merged[1][:, 1])
    print(f"merged partials, phase form vs upsample2x = 1: sum {e[0]:.2e}, squares {e[1]:.2e}")
    assert max(e) < 1e-6


def test_split_k_and_deferred_reduction(gpu):
    """Split-K forced through the tile hint: the second pass sees the partial tiles in output-pixel order like any other convolution's;
    with defer_reduce the slices left in the workspace, added in slice order plus the bias, are that output bit for bit."""
    from storygen_amd import ops
    B, H, W, Cin, Cout, split = 2, 8, 8, 128, 192, 2
    xp, _, wp, bias, ref = _problem(gpu, B, H, W, Cin, Cout)
    M = 4 * B * H * W
    ws = torch.full((ops.gemm_workspace_bytes(M, Cout, split) // 4,), float("nan"), dtype=torch.float32, device=gpu)
    kw = dict(bias=bias, x_padded=True, upsample2x=2, tile=(64, 128), split_k=split, workspace=ws.view(torch.uint8))
    out = torch.full((B, 2 * H, 2 * W, Cout), float("nan"), dtype=torch.float32, device=gpu)
    assert ops.conv3x3_planned_splits(xp, wp, out, **kw) == split
    ops.conv3x3(xp, wp, out, **kw)
    _check_everywhere(out, ref, "phase form, split-K", **F32_BAR)
    ws.fill_(float("nan"))
    ghost = torch.full_like(out, float("nan"))
    ops.conv3x3(xp, wp, ghost, defer_reduce=True, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ghost).all()), "a deferred launch writes no output"
    parts = ws[: split * M * Cout].view(split, M, Cout)
    assert bool(torch.isfinite(parts).all())
    v = torch.zeros(M, Cout, dtype=torch.float32, device=gpu)
    for z in range(split):
        v = v + parts[z]
    v = v + bias.float()[None]
    assert torch.equal(v.view_as(out), out)


@pytest.mark.parametrize("B,H,W,tile", [(1, 8, 8, (256, 128)), (1, 8, 12, None), (2, 4, 4, None)])
def test_launch_the_form_does_not_fit_takes_todays_path(gpu, B, H, W, tile):
    """No row tile inside one phase image (the hinted 256 rows against H W = 64; H W = 96 or 16, which no tile divides): the library
    answers SG_EUNSUP from the query and from the launch without writing, and conv3x3_upsample is the upsample2x = 1 launch bit for bit."""
    from storygen_amd import ops
    from storygen_amd._lib import InvalidArgument
    Cin, Cout = 64, 64
    xp, w3, wp, bias, _ = _problem(gpu, B, H, W, Cin, Cout)
    kw = dict(bias=bias, x_padded=True, tile=tile)
    out = torch.full((B, 2 * H, 2 * W, Cout), float("nan"), dtype=torch.float32, device=gpu)
    assert not ops.conv3x3_phases_fit(xp, wp, out, **kw)
    with pytest.raises(InvalidArgument, match=r"\(-2\)"):
        ops.conv3x3(xp, wp, out, upsample2x=2, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    want = torch.empty_like(out)
    ops.conv3x3(xp, w3, want, upsample2x=True, **kw)
    ops.conv3x3_upsample(xp, w3, wp, out, **kw)
    assert torch.equal(out, want)


def test_descriptor_rejections(gpu):
    """Refused on the host with SG_EINVAL (-1), nothing launched, nothing written: an unpadded input, Cin % 64 != 0, stride 2 together
    with the mode, and the row-addressed epilogue inputs the form does not take."""
    from storygen_amd import ops
    from storygen_amd._lib import InvalidArgument
    B, H, W, Cin, Cout = 1, 8, 8, 64, 64
    xp, _, wp, bias, _ = _problem(gpu, B, H, W, Cin, Cout)
    out = torch.full((B, 2 * H, 2 * W, Cout), float("nan"), dtype=torch.float32, device=gpu)
    x_unpadded = xp[:, 1:-1, 1:-1].contiguous()
    x32 = torch.zeros(B, H + 2, W + 2, 32, dtype=torch.float16, device=gpu)
    wp32 = torch.zeros(4, Cout, 2, 2, 32, dtype=torch.float16, device=gpu)
    half = torch.full((B, H, W, Cout), float("nan"), dtype=torch.float32, device=gpu)
    res = torch.zeros_like(out)
    rb = torch.zeros(B, Cout, dtype=torch.float32, device=gpu)
    for what, args, kw in (("unpadded input", (x_unpadded, wp, out), dict(x_padded=False)),
                           ("Cin % 64", (x32, wp32, out), dict(x_padded=True)),
                           ("stride 2", (xp, wp, half), dict(x_padded=True, stride=2)),
                           ("res1", (xp, wp, out), dict(x_padded=True, res1=res)),
                           ("rowbias", (xp, wp, out), dict(x_padded=True, rowbias=rb))):
        for fn in (ops.conv3x3, ops.conv3x3_launch_plan, ops.conv3x3_planned_splits):
            with pytest.raises(InvalidArgument, match=r"\(-1\)"):
                fn(*args, upsample2x=2, bias=bias, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(half).all())


# the two-level UNet of the other engine tests (head dim 40): its one Upsample2D runs at 640 channels, 16x16 -> 32x32 on the 32x32
# latent (H W = 256: the 128- / 256-row tiles; 3 072 output rows at batch 3) and 8x8 -> 16x16 on the 16x16 latent (H W = 64: the 64-row
# tiles; 4 096 rows at batch 16) — both above engine.UPSAMPLE_PHASES_MIN_ROWS
SMALL = dict(block_out_channels=(320, 640), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
             up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), cross_attention_dim=768, attention_head_dim=8, sample_size=128)


@pytest.mark.parametrize("batch,hw", [(3, 32), (16, 16)])
def test_engine_passes_with_and_without_the_phase_form(gpu, batch, hw):
    """engine.UPSAMPLE_PHASES on against off on a small UNet: a reference pass with harvest and a main pass that consumes the harvested
    context, at batch 3 on a 32x32 latent (the main pass) and at batch 16 on a 16x16 latent (a batched reference pass: the
    largest batch whose time embedding set_inputs() can run without a sampler's time table; the loop's own is 20).  Bar: that of
    test_unet_gpu.test_ff2_and_proj_out_as_one_gemm_is_the_same_pass_32x32 between its two forms (one pass, epsilon)."""
    from storygen_amd import engine as E
    from storygen_amd.arch import build_arch, load_config
    from storygen_amd.synth import synthetic_state_dict
    from test_unet_gpu import TOL_EPS
    arch = build_arch(load_config(SMALL))
    sd = synthetic_state_dict(arch, 0)
    R, S = 2, 7
    g = torch.Generator().manual_seed(5)
    x = torch.randn(batch, 4, hw, hw, generator=g)
    t = torch.full((batch,), 400.0)
    e = torch.randn(batch, S, arch.config["cross_attention_dim"], generator=g)
    got, modes = {}, {}
    real = E.ops.conv3x3
    try:
        for on in (True, False):
            E.UPSAMPLE_PHASES = on
            seen = modes.setdefault(on, [])

            def spy(*a, _seen=seen, **kw):
                _seen.append(kw.get("upsample2x", False))
                return real(*a, **kw)
            E.ops.conv3x3 = spy
            eng = E.UNetEngine(arch, sd, gpu, batch, hw, hw, R, seq_len=S)
            for v in eng.ctx.values():
                v.zero_()
            eng.set_inputs(x, t, e)
            eps_r = eng.forward(harvest_slot=0).clone().cpu()
            ctx = {k: v.clone().cpu() for k, v in eng.ctx.items()}
            eps_m = eng.forward(consume=True).clone().cpu()
            got[on] = (eps_r, eps_m, ctx)
            del eng
    finally:
        E.UPSAMPLE_PHASES = True
        E.ops.conv3x3 = real
    assert 2 in modes[True] and True not in [m for m in modes[True] if m is True], modes[True]
    assert 2 not in modes[False] and any(m is True for m in modes[False]), modes[False]
    errs = {"reference pass": rel_l2(got[True][0], got[False][0]), "main pass": rel_l2(got[True][1], got[False][1])}
    for k in got[True][2]:
        errs[f"harvested {k}"] = rel_l2(got[True][2][k].float(), got[False][2][k].float())
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert all(torch.isfinite(v).all() for v in got[True][:2])
    assert max(errs.values()) <= TOL_EPS, errs
