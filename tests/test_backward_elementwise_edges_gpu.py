"""The bandwidth-bound backward kernels (csrc/backward.hip, the GroupNorm backward of csrc/norm.hip) at their shape, type, stride and
range edges, against float64 on the CPU (oracle/storygen_backward.py or the definition in include/storygen_hip.h).
Bars: the existing ones of tests/test_backward_gpu.py (rel-L2: fp32 outputs 1e-5 LayerNorm / 1e-4 GroupNorm, fp16 outputs 1e-3) plus
check()'s max-abs bar, 3e-3 of the output range.  Every strided output lives in a sentinel-filled buffer that must stay untouched
outside the view.  Measured conditioning numbers: profiles/r10a_backward_edge_tests.txt."""
import pytest
import torch
import torch.nn.functional as F

from conftest import max_rel, rel_l2

pytestmark = pytest.mark.gpu

SENT = -7.0
F16, F32 = torch.float16, torch.float32


def rnd(shape, scale=1.0, seed=0, dtype=F16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def inside(t, dev, pad=8, fill=SENT, row_pad=0):
    """A copy of the CPU tensor t [..., rows, cols] on the device as a column (and optionally row) slice of a wider `fill`-filled buffer.
    Returns (view, buffer)."""
    shape = list(t.shape)
    shape[-1] += 2 * pad
    shape[-2] += row_pad
    buf = torch.full(shape, fill, dtype=t.dtype, device=dev)
    view = buf[..., :t.shape[-2], pad:pad + t.shape[-1]]
    view.copy_(t)
    return view, buf


def untouched(buf, view_shape, pad=8, fill=SENT):
    rows, cols = view_shape[-2], view_shape[-1]
    return bool((buf[..., :pad] == fill).all()) and bool((buf[..., pad + cols:] == fill).all()) and bool((buf[..., rows:, :] == fill).all())


def close(out, want, what, l2, mx=3e-3):
    out, want = out.detach().cpu(), want.detach().cpu()
    assert bool(torch.isfinite(out.float()).all()), f"{what}: non-finite output"
    e2, em = rel_l2(out, want), max_rel(out, want)
    assert e2 <= l2 and em <= mx, f"{what}: rel-L2 {e2:.2e} (bar {l2:.0e}), max-abs / range {em:.2e} (bar {mx:.0e})"


# ------------------------------------------------------------------------------------------------ LayerNorm backward
# NV = ceil(C / 512) registers-per-lane instantiations: both sides of every boundary, the smallest row, the largest.  Each C with one
# (x fp32, dy fp32, dual) combination and its complement, so every C meets both values of each flag and all 8 combinations occur.
LN_CASES = [(C, bool(c & 4), bool(c & 2), bool(c & 1)) for i, C in enumerate((64, 512, 520, 1024, 1032, 1536, 1544, 2048)) for c in (i, 7 - i)]


@pytest.mark.parametrize("C,x32,dy32,dual", LN_CASES)
def test_layernorm_bwd_register_boundaries_types_and_views(gpu, C, x32, dy32, dual):
    from oracle import storygen_backward as B
    from storygen_amd import ops
    for M in (1, 3, 5, 77):                                   # a workgroup is 4 rows: fewer than one, a ragged last one
        x = rnd((M, C), 2.0, 1, F32 if x32 else F16) + 0.5
        dy1, dy2 = rnd((M, C), 1.0, 2, F32 if dy32 else F16), rnd((M, C), 1.0, 3, F32 if dy32 else F16)
        g1, g2, res = rnd((C,), 1.0, 4), rnd((C,), 1.0, 5), rnd((M, C), 1.0, 6, F32)
        want = 2.0 * res.double() + B.layer_norm_bwd(x.double(), g1.double(), dy1.double())
        if dual:
            want = want + B.layer_norm_bwd(x.double(), g2.double(), dy2.double())
        (xv, _), (d1v, _), (d2v, _), (rv, _) = (inside(t, gpu, row_pad=2) for t in (x, dy1, dy2, res))
        ov, obuf = inside(torch.full((M, C), SENT, dtype=F32), gpu, row_pad=2)
        ops.layernorm_bwd(xv, d1v, g1.to(gpu), ov, 1e-5, d2v if dual else None, g2.to(gpu) if dual else None, rv, 2.0)
        close(ov, want, f"layernorm_bwd M{M} C{C}", 1e-5)
        assert untouched(obuf, (M, C)), f"layernorm_bwd M{M} C{C}: wrote outside its view"


def test_layernorm_bwd_rejects_rows_wider_than_its_registers(gpu):
    from storygen_amd import ops
    x, dy, g = torch.zeros(4, 2056, device=gpu), torch.zeros(4, 2056, dtype=F16, device=gpu), torch.ones(2056, dtype=F16, device=gpu)
    out = torch.full((4, 2056), SENT, device=gpu)
    with pytest.raises(RuntimeError, match="C=2056 must be a multiple of 8, <= 2048"):
        ops.layernorm_bwd(x, dy, g, out)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


def test_layernorm_bwd_of_rows_far_from_zero(gpu):
    """fp32 x with |mean| = 1e3 sigma: the bar is measured, not assumed — 4 x the error of torch's own fp32 LayerNorm autograd on the CPU
    against float64 on the same input, or the usual 1e-5, whichever is larger (an fp32 x at 1e3 sigma carries ~6e-5 sigma of rounding
    in x - mean whatever the algorithm)."""
    from oracle import storygen_backward as B
    from storygen_amd import ops
    M, C = 77, 1280
    x = rnd((M, C), 1.0, 1, F32) + 1000.0
    dy, g = rnd((M, C), 1.0, 2), rnd((C,), 1.0, 3) + 1.0
    want = B.layer_norm_bwd(x.double(), g.double(), dy.double())
    xt = x.clone().requires_grad_(True)
    F.layer_norm(xt, (C,), g.float(), None, 1e-5).backward(dy.float())
    e_torch = rel_l2(xt.grad, want)
    out = torch.empty(M, C, device=gpu)
    ops.layernorm_bwd(x.to(gpu), dy.to(gpu), g.to(gpu), out)
    e_kernel = rel_l2(out.cpu(), want)
    print(f"COND layernorm_bwd |mean| = 1e3 sigma: kernel {e_kernel:.2e}, torch fp32 CPU autograd {e_torch:.2e}")
    assert e_kernel <= max(4.0 * e_torch, 1e-5)


# ------------------------------------------------------------------------------------------------ GEGLU backward
@pytest.mark.parametrize("N8", [64, 2560, 10240])
@pytest.mark.parametrize("M", [1, 200])
def test_geglu_bwd_both_gelu_tails_and_views(gpu, M, N8):
    """Gates spread over [-12, 12] (both tails of gelu' : __expf underflows, erff saturates).  |du * val * gelu'| stays far below 6e4:
    fp16 saturation of the outputs is outside the kernel's contract."""
    from oracle import storygen_backward as B
    from storygen_amd import ops
    N4 = N8 // 2
    val, du = rnd((M, N4), 1.5, 1), rnd((M, N4), 1.0, 3)
    gate = (torch.linspace(-12.0, 12.0, M * N4).reshape(M, N4)[:, torch.randperm(N4, generator=torch.Generator().manual_seed(2))]).to(F16)
    il = lambda a, b: torch.stack([a.view(M, -1, 32), b.view(M, -1, 32)], dim=2).reshape(M, 2 * N4)   # noqa: E731
    (pv, _), (dv, _) = inside(il(val, gate), gpu, row_pad=1), inside(du, gpu, row_pad=1)
    ov, obuf = inside(torch.full((M, N8), SENT, dtype=F16), gpu, row_pad=1)
    ops.geglu_bwd(pv, dv, ov)
    dval = du.double() * F.gelu(gate.double())
    dgate = B.gelu_bwd(gate.double(), du.double() * val.double())
    close(ov, il(dval, dgate), f"geglu_bwd M{M} N8 {N8}", 1e-3)
    close(ov.cpu().reshape(M, -1, 2, 32)[:, :, 1], dgate.view(M, -1, 32), f"geglu_bwd M{M} N8 {N8}: dgate alone", 1e-3)
    assert untouched(obuf, (M, N8))


# ------------------------------------------------------------------------------------------------ GroupNorm backward
def _gn_want(x, dy, g, b, silu, H, W):
    from oracle import storygen_backward as B
    B_, HW, C = x.shape
    xi = x.double().transpose(1, 2).reshape(B_, C, H, W)
    dyi = dy.double().transpose(1, 2).reshape(B_, C, H, W)
    if silu:
        dyi = B.silu_bwd(F.group_norm(xi, 32, g.double(), b.double(), 1e-5), dyi)
    return B.group_norm_bwd(xi, g.double(), dyi, 32, 1e-5).reshape(B_, C, HW).transpose(1, 2)


# C = 256: 8 channels per group, the minimum; 2560: the limit (1024 threads = 3 pixel rows of 320 vectors + 64 idle threads); HW = 64:
# rows_per_chunk below one pass of the thread rows; (5, 9, 7): nothing divides anything; 64 x 64: many chunks.  Output mode and types
# cycle so that each of {fp32 + res, fp16, padded fp16} meets each of the four (x, dy) type pairs, SiLU and not.
GN_SHAPES = [(1, 8, 8, 256), (4, 8, 8, 1280), (2, 8, 8, 2560), (2, 16, 16, 1920), (5, 9, 7, 320), (1, 64, 64, 320)]
GN_CASES = [(*s, bool(j & 1), ("f32res", "f16", "f16pad")[j % 3], bool((j // 3) & 1), bool((j // 3) & 2))
            for j, s in enumerate(sh for sh in GN_SHAPES for _ in (0, 1))]


@pytest.mark.parametrize("B_,H,W,C,silu,mode,x32,dy32", GN_CASES)
def test_groupnorm_bwd_channel_limits_small_images_types_and_views(gpu, B_, H, W, C, silu, mode, x32, dy32):
    from storygen_amd import ops
    HW = H * W
    x = rnd((B_, HW, C), 2.0, 1, F32 if x32 else F16) + 1.0
    dy = rnd((B_, HW, C), 1.0, 2, F32 if dy32 else F16)
    g, b = rnd((C,), 1.0, 3) + 1.0, rnd((C,), 0.5, 4)
    want = _gn_want(x, dy, g, b, silu, H, W)
    ws = torch.empty(ops.groupnorm_bwd_workspace_bytes(B_, 32), dtype=torch.uint8, device=gpu)
    strided = lambda t: inside(t.reshape(B_ * HW, C), gpu)[0].unflatten(0, (B_, HW))         # noqa: E731
    xv, dyv = strided(x), strided(dy)
    what = f"groupnorm_bwd B{B_} {H}x{W} C{C} silu{int(silu)} {mode}"
    if mode == "f32res":
        res = rnd((B_, HW, C), 1.0, 5, F32)
        ov, obuf = inside(torch.full((B_ * HW, C), SENT, dtype=F32), gpu)
        ops.groupnorm_bwd(xv, dyv, g.to(gpu), b.to(gpu), ov.unflatten(0, (B_, HW)), 32, 1e-5, silu, ws, res=strided(res))
        close(ov.unflatten(0, (B_, HW)), want + res.double(), what, 1e-4)
        assert untouched(obuf, (B_ * HW, C))
    elif mode == "f16":
        ov, obuf = inside(torch.full((B_ * HW, C), SENT, dtype=F16), gpu)
        ops.groupnorm_bwd(xv, dyv, g.to(gpu), b.to(gpu), ov.unflatten(0, (B_, HW)), 32, 1e-5, silu, ws)
        close(ov.unflatten(0, (B_, HW)), want, what, 1e-3)
        assert untouched(obuf, (B_ * HW, C))
    else:
        out = torch.zeros(B_, H + 2, W + 2, C, dtype=F16, device=gpu)
        ops.groupnorm_bwd(xv, dyv, g.to(gpu), b.to(gpu), out, 32, 1e-5, silu, ws)
        close(out[:, 1:-1, 1:-1].reshape(B_, HW, C), want, what, 1e-3)
        for name, border in (("top", out[:, 0]), ("bottom", out[:, -1]), ("left", out[:, :, 0]), ("right", out[:, :, -1])):
            assert float(border.abs().max()) == 0.0, f"{what}: {name} border written"


@pytest.mark.parametrize("C", [128, 2592])
def test_groupnorm_bwd_unsupported_channel_counts(gpu, C):
    from storygen_amd import ops
    x, dy = torch.zeros(1, 64, C, device=gpu), torch.zeros(1, 64, C, dtype=F16, device=gpu)
    g = torch.ones(C, dtype=F16, device=gpu)
    out = torch.full((1, 64, C), SENT, device=gpu)
    ws = torch.empty(ops.groupnorm_bwd_workspace_bytes(1, 32), dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError, match=r"needs >= 8 channels per group and C <= 2560"):
        ops.groupnorm_bwd(x, dy, g, g, out, 32 if C == 128 else 16, 1e-5, False, ws)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


@pytest.mark.parametrize("kind", ["common_offset", "pivot_outlier"])
def test_groupnorm_bwd_conditioning(gpu, kind):
    """~30 sigma offsets.  common_offset: every value of x carries +30.  pivot_outlier: pixel 0 of each group's first channel — the pivot
    gnw_group_stats subtracts before it forms q / n - md^2 — sits 30 sigma out, so every OTHER value is 30 sigma from the pivot.
    Bar: 4 x torch's fp32 CPU GroupNorm autograd against float64 on the same input, or the usual 1e-4, whichever is larger.
    Measured on MI355X (profiles/r10a_backward_edge_tests.txt): common_offset kernel 8.6e-8 (torch 1.36e-4): the pivot does its job.
    pivot_outlier: 1.05e-4 while gnw_group_stats formed q / n - md^2 over the whole image (a 900 : 1 cancellation in fp32: this test's
    finding), 9.9e-6 since it merges the chunk partials Chan-style (torch 9.72e-8)."""
    from storygen_amd import ops
    B_, H, W, C = 2, 32, 32, 320
    HW = H * W
    x = rnd((B_, HW, C), 1.0, 1, F32)
    if kind == "common_offset":
        x += 30.0
    else:
        x[:, 0, ::C // 32] += 30.0
    dy, g, b = rnd((B_, HW, C), 1.0, 2), rnd((C,), 1.0, 3) + 1.0, rnd((C,), 0.5, 4)
    want = _gn_want(x, dy, g, b, False, H, W)
    xt = x.transpose(1, 2).reshape(B_, C, H, W).clone().requires_grad_(True)
    F.group_norm(xt, 32, g.float(), b.float(), 1e-5).backward(dy.float().transpose(1, 2).reshape(B_, C, H, W))
    e_torch = rel_l2(xt.grad.reshape(B_, C, HW).transpose(1, 2), want)
    ws = torch.empty(ops.groupnorm_bwd_workspace_bytes(B_, 32), dtype=torch.uint8, device=gpu)
    out = torch.empty(B_, HW, C, device=gpu)
    ops.groupnorm_bwd(x.to(gpu), dy.to(gpu), g.to(gpu), b.to(gpu), out, 32, 1e-5, False, ws)
    e_kernel = rel_l2(out.cpu(), want)
    print(f"COND groupnorm_bwd {kind}: kernel {e_kernel:.2e}, torch fp32 CPU autograd {e_torch:.2e}")
    assert e_kernel <= max(4.0 * e_torch, 1e-4)


# ------------------------------------------------------------------------------------------------ conv dgrad helpers
@pytest.mark.parametrize("B_,H,W,C", [(1, 1, 1, 4), (2, 5, 3, 4), (2, 5, 3, 72), (1, 16, 16, 320)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_sum2x2_accumulate_and_pixel_strides(gpu, B_, H, W, C, accumulate):
    """Bit-exact against the four-term fp32 sum in the kernel's order ((0 + a00 + a01 + a10 + a11) + dx); accumulate = False must
    overwrite (a NaN-filled dx), accumulate = True must add to what is there."""
    from storygen_amd import ops
    du = rnd((B_, 2 * H, 2 * W, C), 1.0, 1, F32)
    old = rnd((B_, H, W, C), 3.0, 2, F32) if accumulate else torch.full((B_, H, W, C), float("nan"))
    duv, _ = inside(du.reshape(-1, C), gpu, pad=4)
    dxv, dxbuf = inside(old.reshape(-1, C), gpu, pad=4)
    ops.sum2x2(duv.unflatten(0, (B_, 2 * H, 2 * W)), dxv.unflatten(0, (B_, H, W)), accumulate=accumulate)
    want = ((du[:, 0::2, 0::2] + du[:, 0::2, 1::2]) + du[:, 1::2, 0::2]) + du[:, 1::2, 1::2]
    if accumulate:
        want = want + old
    assert torch.equal(dxv.cpu().unflatten(0, (B_, H, W)), want)
    assert untouched(dxbuf, (B_ * H * W, C), pad=4)


@pytest.mark.parametrize("B_,Ho,Wo,C", [(1, 1, 1, 8), (2, 5, 3, 72), (1, 8, 8, 320)])
@pytest.mark.parametrize("dy32", [False, True])
def test_zero_stuff_against_its_definition(gpu, B_, Ho, Wo, C, dy32):
    """y[b, 1 + 2i, 1 + 2j] = dy[b, i, j], every other interior pixel 0 — the whole interior overwritten (it starts as NaN), the border
    left alone (it starts, and must stay, zero)."""
    from storygen_amd import ops
    dy = rnd((B_, Ho, Wo, C), 1.0, 1, F32 if dy32 else F16)
    dyv, _ = inside(dy.reshape(-1, C), gpu)
    y = torch.zeros(B_, 2 * Ho + 2, 2 * Wo + 2, C, dtype=F16, device=gpu)
    y[:, 1:-1, 1:-1] = float("nan")
    ops.zero_stuff(dyv.unflatten(0, (B_, Ho, Wo)), y)
    want = torch.zeros(B_, 2 * Ho + 2, 2 * Wo + 2, C, dtype=F16)
    want[:, 1:-1:2, 1:-1:2] = dy.half()
    assert torch.equal(y.cpu(), want)


@pytest.mark.parametrize("n", [288, 1024, 1025, 65536 + 7])
def test_mse_grad_ragged_sizes_and_trivial_masks(gpu, n):
    from storygen_amd import ops
    pred, noise = rnd((n,), 1.0, 1, F32), rnd((n,), 1.0, 2, F32)
    for name, mask in (("random", (rnd((n,), 1.0, 3, F32) > 0.5).float()), ("zeros", torch.zeros(n)), ("ones", torch.ones(n))):
        d, loss = torch.full((n,), float("nan"), device=gpu), torch.full((1,), float("nan"), device=gpu)
        ops.mse_grad(pred.to(gpu), noise.to(gpu), mask.to(gpu), d, loss)
        keep = 1.0 - mask.double()
        diff = (pred.double() - noise.double()) * keep
        want_loss, want_d = float((diff * diff).mean()), 2.0 * diff * keep / n
        if name == "ones":
            assert float(loss) == 0.0 and float(d.abs().max()) == 0.0
        else:
            assert abs(float(loss) - want_loss) <= 1e-6 * want_loss, (name, float(loss), want_loss)
            assert rel_l2(d.cpu(), want_d) <= 1e-6


# ------------------------------------------------------------------------------------------------ transposes
@pytest.mark.parametrize("M,C,f32", [(8, 8, False), (8, 8, True), (72, 200, True), (200, 72, True), (72, 72, False)])
def test_transpose_minimum_and_ragged_fp32_views(gpu, M, C, f32):
    from storygen_amd import ops
    src = rnd((M, C), 1.0, 1, F32 if f32 else F16)
    sv, _ = inside(src, gpu, row_pad=3)
    dv, dbuf = inside(torch.full((C, M), SENT, dtype=F16), gpu, row_pad=3)
    ops.transpose(sv, dv)
    assert torch.equal(dv.cpu(), src.half().t())
    assert untouched(dbuf, (C, M))
    B_ = 3
    src = rnd((B_, M, C), 1.0, 2, F32 if f32 else F16)
    sv, _ = inside(src, gpu, row_pad=3)
    dv, dbuf = inside(torch.full((B_, C, M), SENT, dtype=F16), gpu, row_pad=3)
    ops.transpose_batched(sv, dv)
    assert torch.equal(dv.cpu(), src.half().transpose(1, 2))
    assert untouched(dbuf, (C, M))
