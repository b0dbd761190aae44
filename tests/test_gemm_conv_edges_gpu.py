"""storygen_amd/csrc/gemm_conv.hip at its split, tile and offset edges: sg_gemm_f16 and sg_conv3x3_nhwc_f16 on every kernel family (the
LDS-DMA pipeline on its six tiles, the 32x32-per-wave latency kernel, the eight-wave fat kernel, the register-staged generic kernel) and the
two split-K second passes behind them.

1. Forced K slices: every split_k of 2..16, 24 and 64 — values the cost model never enumerates, more slices than 64-deep K slabs (clamped),
   slices that own no slab (they contribute zeros) — with every epilogue term, bit-identical over three repeats, on the slice count the
   launch-plan query reports and on a workspace of exactly that many partial tiles, NaN-filled before every launch (an unwritten partial
   tile cannot pass for zeros).  Also the GEGLU second pass, sg_gemm_pair_f16, and a fat-kernel hint (which does not split K).
2. Nothing outside the views: every output is an interior window of a buffer prefilled with a fixed bit pattern (compared as bits
   afterwards), every input a window of a NaN-filled buffer, the workspace has sentinel bands on both sides.
3. The 32-bit byte offsets of the LDS-DMA operands: operands that end just inside 4 GiB from their base pointer compute the right
   rows at both ends; the first inadmissible size is rejected by the descriptor check before anything is launched.

Reference for every case: float64 torch on the same fp16-rounded operands (the convolution as an explicit im2col product, which also
gives sum |a||w|).

Bar, per output element and for ANY summation order (u = 2^-24):  |err| <= gamma_K * sum_k |a_mk||w_nk|, gamma_K = K u / (1 - K u), plus
u |term| per fp32 epilogue term added, plus one output rounding (2^-24 |ref| for fp32 outputs, 2^-11 |ref| for fp16 outputs and the fp16
copy).  It is derived, not measured, and carries no factor.  On this CPU-only check, done once when the bar was written: torch's own fp32
`a.float() @ w.float().t()` stays inside it against the float64 reference at every (M, N, K) used below (158 shapes, worst |err| / bar 0.09).
GroupNorm partials: a sum of T fp32 values in any order, gamma_T * sum |v| (gamma_(T+1) * sum v^2 for the squares, one fma each).

Every case prints its worst ratio to the bar (`-s`); the figures of the first hardware run are in profiles/r18a_gemm_conv_edge_tests.txt."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
F16, F32, F64 = torch.float16, torch.float32, torch.float64
U = 2.0 ** -24
SENT32 = 0x7FC5A5A5          # a quiet NaN with a recognisable payload (fp32 buffers, as int32)
SENT16 = 0x7C7C              # an fp16 NaN (as int16)
SENT8 = 0xA5                 # workspace bands
WS_FILL = 0xFF               # workspace interior: 0xFFFFFFFF is an fp32 NaN, so a partial tile that no slice wrote makes the result non-finite
GR, GC = 3, 8                # guard rows above / below, guard columns left / right of every 2-D window (ld = N + 16)
BAND = 4096                  # bytes of sentinel in front of and behind a workspace
FORCED = list(range(2, 17)) + [24, 64]
PIPE_TILES = [(256, 128), (128, 128), (256, 64), (128, 64), (64, 128), (64, 64)]
# (family, forced split) combinations a family cannot serve: none.  In particular the register-staged kernel serves every split_k.
UNSERVED = []


# ------------------------------------------------------------------------------------------------------------------------- helpers
def _gamma(n):
    return n * U / (1.0 - n * U)


def _randn(shape, dev, seed, dtype=F16, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def _sent(shape, dtype, dev):
    """A buffer of `dtype` whose every element is the sentinel bit pattern."""
    if dtype == F16:
        return torch.full(shape, SENT16, dtype=torch.int16, device=dev).view(F16)
    return torch.full(shape, SENT32, dtype=torch.int32, device=dev).view(F32)


def _bits(buf):
    return buf.view(torch.int16) if buf.dtype == F16 else buf.view(torch.int32)


def _guards_intact(what, buf, index):
    """Everything of buf outside buf[index] is still the sentinel, bit for bit."""
    ok = _bits(buf) == (SENT16 if buf.dtype == F16 else SENT32)
    ok[index] = True
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} guard elements outside the view were written, first at {tuple(int(v) for v in (~ok).nonzero()[0])}"


def _untouched(what, buf):
    assert bool((_bits(buf) == (SENT16 if buf.dtype == F16 else SENT32)).all()), f"{what}: written by a launch that must fail before it starts"


def _nan_window(data):
    """data as the interior of a NaN-filled buffer: guard rows and columns for 2-D [rows, cols], guard images and channels for [B, H, W, C]."""
    if data.dim() == 2:
        buf = torch.full((data.shape[0] + 2 * GR, data.shape[1] + 2 * GC), float("nan"), dtype=data.dtype, device=data.device)
        view = buf[GR:GR + data.shape[0], GC:GC + data.shape[1]]
    else:
        # (the descriptor carries ONE pixel stride, so the images of a batch are adjacent by contract and a window in H or W cannot be
        # expressed: a row read above image b >= 1 lands in image b - 1's random data and shows as an error far above the bar, not as NaN)
        B, H, W, Cc = data.shape
        buf = torch.full((B + 2, H, W, Cc + 2 * GC), float("nan"), dtype=data.dtype, device=data.device)
        view = buf[1:B + 1, :, :, GC:GC + Cc]
    view.copy_(data)
    return view


def _nan_fenced(data):
    """An exact-size contiguous tensor with NaN-filled memory directly in front of and behind it."""
    n = data.numel()
    buf = torch.full((n + 128,), float("nan"), dtype=data.dtype, device=data.device)
    view = buf[64:64 + n].view(data.shape)
    view.copy_(data)
    return view


def _out_window(shape, dtype, dev):
    """(buffer, view, index): a sentinel-filled output window, 2-D [M, N] or [B, Ho, Wo, C]."""
    if len(shape) == 2:
        buf = _sent((shape[0] + 2 * GR, shape[1] + 2 * GC), dtype, dev)
        idx = (slice(GR, GR + shape[0]), slice(GC, GC + shape[1]))
    else:
        buf = _sent((shape[0] + 2, shape[1], shape[2], shape[3] + 2 * GC), dtype, dev)
        idx = (slice(1, shape[0] + 1), slice(None), slice(None), slice(GC, GC + shape[3]))
    return buf, buf[idx], idx


def _flat_window(n, dev):
    """(buffer, view, index) of n contiguous fp32 values with 64 sentinel floats on both sides."""
    buf = _sent((n + 128,), F32, dev)
    return buf, buf[64:64 + n], (slice(64, 64 + n),)


def _workspace(nbytes, dev):
    """(buffer, workspace view of exactly nbytes) with a sentinel band on both sides.  The interior is NaN as fp32 (a real workspace holds
    garbage): every partial tile the second pass or the consumer reads must have been written by its slice, an empty slice's zeros included."""
    buf = torch.full((nbytes + 2 * BAND,), SENT8, dtype=torch.uint8, device=dev)
    buf[BAND:BAND + nbytes] = WS_FILL
    return buf, buf[BAND:BAND + nbytes]


def _workspace_untouched(what, wsbuf, nbytes):
    _bands_intact(what, wsbuf, nbytes)
    assert bool((wsbuf[BAND:BAND + nbytes] == WS_FILL).all()), f"{what}: the workspace was written by a launch that must fail before it starts"


def _bands_intact(what, wsbuf, nbytes):
    assert bool((wsbuf[:BAND] == SENT8).all()) and bool((wsbuf[BAND + nbytes:] == SENT8).all()), f"{what}: written outside the {nbytes}-byte workspace"


def _assert_bar(what, out, ref, bar, plan, K):
    """Element-wise |out - ref| <= bar; names the worst element, its tile and the K slicing of the launch."""
    out2, ref2, bar2 = out.reshape(-1, out.shape[-1]).double(), ref.reshape(-1, ref.shape[-1]), bar.reshape(-1, bar.shape[-1])
    assert bool(torch.isfinite(out2).all()), f"{what}: non-finite output (a read outside an operand's view leaked, or a sentinel was left in place)"
    ratio = (out2 - ref2).abs() / bar2
    worst = int(ratio.argmax())
    r, c = divmod(worst, ratio.shape[1])
    bm, bn, splits = plan[0], plan[1], plan[2]
    kt = -(-K // 64)
    msg = (f"{what}: worst |err| / bar {float(ratio[r, c]):.3f} at row {r}, column {c} = tile ({r // bm}, {c // bn}) of {bm}x{bn}; "
           f"{splits} K slice(s) of {-(-kt // splits)} slab(s) over {kt} slabs; got {float(out2[r, c]):.6g}, reference {float(ref2[r, c]):.6g}")
    print(msg)
    assert float(ratio[r, c]) <= 1.0, msg


def _plan_matches(what, plan, want_split, K):
    kt = -(-K // 64)
    if want_split >= 1:
        assert plan[2] == min(want_split, kt), f"{what}: the plan reports {plan[2]} K slices for split_k = {want_split} over {kt} slabs"


# --------------------------------------------------------------------------------------------------------------------------- GEMM
@functools.lru_cache(maxsize=None)
def _gemm_problem(M, N, K):
    """Operands (in NaN-surrounded windows), the float64 reference and the three parts of the bar; shared by every case of one shape."""
    dev = torch.device("cuda:0")
    a, w = _randn((M, K), dev, 3), _randn((N, K), dev, 4, scale=K ** -0.5)
    rpb = max(1, M // 3)
    bias, rb = _randn((N,), dev, 5), _randn((-(-M // rpb), N), dev, 8, F32)
    r1, r2 = _randn((M, N), dev, 6, F32), _randn((M, N), dev, 7)
    rows = torch.arange(M, device=dev) // rpb
    terms = [bias.double().expand(M, N), rb.double()[rows], r1.double(), r2.double()]
    acc = a.double() @ w.double().t()
    ref = acc + terms[0] + terms[1] + terms[2] + terms[3]
    core = _gamma(K) * (a.double().abs() @ w.double().abs().t()) + U * sum(t.abs() for t in terms)
    ops_in = dict(a=_nan_window(a), w=_nan_window(w), bias=_nan_fenced(bias), rowbias=_nan_fenced(rb), rows_per_batch=rpb,
                  res1=_nan_window(r1), res2=_nan_window(r2))
    return ops_in, ref, core


def _run_gemm(what, M, N, K, *, split_k, tile=None, out_f32=True, ws_bytes=None, repeats=1, ln_out=False, stats=False):
    """One sg_gemm_f16 case with every term, every buffer a window; returns the plan.  ws_bytes None: M N 4 bytes per reported slice."""
    from storygen_amd import ops
    dev = torch.device("cuda:0")
    p, ref, core = _gemm_problem(M, N, K)
    cbuf, c, cidx = _out_window((M, N), F32 if out_f32 else F16, dev)
    c2buf, c2, c2idx = _out_window((M, N), F16, dev)
    kw = dict(bias=p["bias"], rowbias=p["rowbias"], rows_per_batch=p["rows_per_batch"], res1=p["res1"], res2=p["res2"], out2=c2,
              split_k=split_k, tile=tile, use_table=False)
    nblk = (N // 64 + 1) & ~1
    if ln_out:
        lbuf, lview, lidx = _flat_window(M * nblk * 2, dev)
        kw["ln_out"] = lview.view(M, nblk, 2)
    # the plan is a function of the workspace the launch is given: query it with the largest the case could use, then size the real one
    if ws_bytes is None:
        big = torch.empty(M * N * 4 * 64, dtype=torch.uint8, device=dev)
        plan = ops.gemm_launch_plan(p["a"], p["w"], c, workspace=big, **kw)
        ws_bytes = M * N * 4 * plan[2] if plan[2] > 1 else 0
        del big
    wsbuf, ws = _workspace(ws_bytes, dev) if ws_bytes else (None, None)
    kw["workspace"] = ws
    plan = ops.gemm_launch_plan(p["a"], p["w"], c, **kw)
    _plan_matches(what, plan, split_k, K)
    if split_k == 0 and ws_bytes:
        assert plan[2] <= max(1, ws_bytes // (M * N * 4)), f"{what}: {plan[2]} slices planned into a workspace of {ws_bytes} bytes"
    if stats:
        T = M            # one image = the whole problem: partials exist where a row tile divides M
        sb_probe = _sent((16,), F32, dev)
        rows = ops.gemm_stats_rows(p["a"], p["w"], c, stats=(sb_probe, T), **kw)
        if rows == 0:
            with pytest.raises(RuntimeError, match="statistics"):
                ops.gemm(p["a"], p["w"], c, stats=(sb_probe, T), **kw)
            torch.cuda.synchronize()
            for name, b in (("C", cbuf), ("C2", c2buf), ("stats", sb_probe)) + ((("ln_stats_out", lbuf),) if ln_out else ()):
                _untouched(f"{what}: {name} after the rejected statistics launch", b)
            if wsbuf is not None:
                _workspace_untouched(f"{what}: rejected statistics launch", wsbuf, ws_bytes)
        else:
            sbuf, sview, sidx = _flat_window((M // rows) * 2 * N, dev)
            kw["stats"] = (sview, T)
    first = None
    for _ in range(repeats):
        _bits(cbuf).fill_(SENT32 if out_f32 else SENT16)
        if ws is not None:
            ws.fill_(WS_FILL)
        ops.gemm(p["a"], p["w"], c, **kw)
        torch.cuda.synchronize()
        got = (_bits(c).clone(), _bits(c2).clone())
        if first is None:
            first = got
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]), f"{what}: repeats differ bit-wise"
    _guards_intact(f"{what}: C", cbuf, cidx)
    _guards_intact(f"{what}: C2", c2buf, c2idx)
    if wsbuf is not None:
        _bands_intact(what, wsbuf, ws_bytes)
    _assert_bar(f"{what}: C", c, ref, core + (U if out_f32 else 2.0 ** -11) * ref.abs(), plan, K)
    _assert_bar(f"{what}: C2", c2, ref, core + 2.0 ** -11 * ref.abs(), plan, K)
    if "stats" in kw and out_f32:
        rows = M // (sview.numel() // (2 * N))
        _guards_intact(f"{what}: stats", sbuf, sidx)
        v = c.double().view(M // rows, rows, N)
        got = sview.view(M // rows, 2, N)
        _assert_bar(f"{what}: stats sums", got[:, 0], v.sum(1), _gamma(rows) * v.abs().sum(1) + 1e-300, plan, K)
        _assert_bar(f"{what}: stats squares", got[:, 1], (v * v).sum(1), _gamma(rows + 1) * (v * v).sum(1) + 1e-300, plan, K)
    if ln_out and out_f32:
        # per token and 64-column block (sum, M2 about the block mean) of the final fp32 values: the sum in any order gamma_64 sum |v|;
        # M2 = sum (v - m)^2 with the ROUNDED mean m = M2_true + 64 (m - mean)^2 exactly, each difference and the 64 fmas one rounding
        _guards_intact(f"{what}: ln_stats_out", lbuf, lidx)
        v = c.double().view(M, N // 64, 64)
        got = lview.view(M, nblk, 2)[:, :N // 64]
        s_bar = _gamma(64) * v.abs().sum(2)
        em = s_bar / 64 + U * v.mean(2).abs()
        m2 = ((v - v.mean(2, keepdim=True)) ** 2).sum(2)
        _assert_bar(f"{what}: ln sums", got[..., 0], v.sum(2), s_bar + 1e-300, plan, K)
        _assert_bar(f"{what}: ln M2", got[..., 1], m2, _gamma(66) * (m2 + 64 * em * em) + 64 * em * em + 1e-300, plan, K)
    return plan


class _tile_forced:
    """debug_set_tile for the body, the automatic choice back afterwards (also when the body fails)."""
    def __init__(self, bm, bn, generic=False):
        self.t = (bm, bn, generic)

    def __enter__(self):
        from storygen_amd import ops
        ops.debug_set_tile(*self.t)

    def __exit__(self, *exc):
        from storygen_amd import ops
        ops.debug_set_tile(0, 0, False)
        ops.debug_set_option("reset", 0)
        return False


# ---------------------------------------------------------------------------------------------------- 1. forced K slices
# pipelined: KT = 10 and KT = 3; generic (K % 64 != 0): KT = 3 with a partial last slab, and KT = 2
SPLIT_GEMMS = [(100, 72, 640), (130, 200, 192), (100, 72, 136), (64, 64, 72)]
HINTS = {"auto": None, "lat64x64": (64, 64, 4), "lat64x128": (64, 128, 8)}


@pytest.mark.parametrize("split", FORCED)
@pytest.mark.parametrize("hint", list(HINTS))
@pytest.mark.parametrize("M,N,K", SPLIT_GEMMS)
def test_gemm_forced_split_every_value(gpu, M, N, K, hint, split):
    """split_k = 7, 9, 11, ... and split_k > KT on the pipelined, the latency and the generic kernel.  The hints do not apply to K % 64 != 0:
    those launches must stay on the generic kernel's one tile, which is all the 2 shapes x 2 hints x 17 = 68 hinted generic cases add to
    their 'auto' twins (same kernel, same plan).  KT = 10 at split 7, 8, 9: ceil(10 / s) = 2 slabs a slice, slices 5 and up own no slab."""
    assert ("gemm", hint, split) not in UNSERVED
    plan = _run_gemm(f"gemm {M}x{N}x{K} {hint} split_k={split}", M, N, K, split_k=split, tile=HINTS[hint], repeats=3)
    if K % 64:
        assert plan[:2] == (128, 128) and plan[5] == 0, f"the generic kernel was handed tile {plan[:2]}"
    elif HINTS[hint]:
        assert plan[:2] == HINTS[hint][:2] and plan[5] >= 16, f"forced split_k = {split} changed the hinted kernel: plan {plan}"


@pytest.mark.parametrize("bm,bn", PIPE_TILES)
@pytest.mark.parametrize("M,N,K", SPLIT_GEMMS[:2])
def test_gemm_forced_split_keeps_the_tile(gpu, M, N, K, bm, bn):
    """split_k = 7 (never enumerated by the cost model; KT = 10: two empty slices, KT = 3: clamped) under each pipeline tile."""
    with _tile_forced(bm, bn):
        plan = _run_gemm(f"gemm {M}x{N}x{K} tile {bm}x{bn} split_k=7", M, N, K, split_k=7, repeats=3)
        assert plan[:2] == (bm, bn) and plan[5] == 1, f"forced split_k = 7 changed the tile: plan {plan}"


@pytest.mark.parametrize("fat", [(512, 128, 8), (256, 256, 8)])
@pytest.mark.parametrize("M,N,K", SPLIT_GEMMS[:2])
def test_gemm_fat_hint_with_a_forced_split_leaves_the_fat_kernel(gpu, M, N, K, fat):
    """The one documented exception to "a forced split keeps the tile": the eight-wave fat kernel does not split K, so its hint together with
    split_k > 1 is answered as if no tile had been asked for (a pipeline tile or the latency kernel, by size) on the forced slice count —
    never by an unsplit fat launch."""
    plan = _run_gemm(f"gemm {M}x{N}x{K} hint {fat} split_k=3", M, N, K, split_k=3, tile=fat, repeats=3)
    assert (plan[5] == 1 or plan[5] >= 16) and plan[2] == 3 and plan[:2] in PIPE_TILES, f"fat hint + split_k = 3: plan {plan}"


# GEGLU: bias only, fp16 [M, N / 2]; the erf polynomial is outside the derived bound, so the bars of tests/test_kernels_gpu.py::check, per ROW
GEGLU_L2, GEGLU_MAX = 1.0e-3, 3.0e-3


@pytest.mark.parametrize("split", [3, 7, 64])
@pytest.mark.parametrize("K,generic", [(640, False), (136, True)], ids=["pipe-K640", "generic-K136"])
def test_geglu_forced_split(gpu, K, generic, split):
    """The GEGLU form of the split-K second pass (16 interleaved columns per thread) behind the pipeline and the generic kernel, with empty
    slices (KT = 10, split 7) and more slices than slabs."""
    import torch.nn.functional as F
    from storygen_amd import ops
    from storygen_amd.repack import interleave_geglu
    M, inner = 100, 64
    a, w, b = _randn((M, K), gpu, 21), _randn((2 * inner, K), gpu, 22, scale=K ** -0.5), _randn((2 * inner,), gpu, 23)
    proj = a.double() @ w.double().t() + b.double()
    ref = proj[:, :inner] * F.gelu(proj[:, inner:])
    wi, bi = interleave_geglu(w, b)
    av, wv, bv = _nan_window(a), _nan_window(wi.contiguous()), _nan_fenced(bi.contiguous())
    n = min(split, -(-K // 64))
    first = None
    for _ in range(3):
        obuf, out, oidx = _out_window((M, inner), F16, gpu)
        wsbuf, ws = _workspace(M * 2 * inner * 4 * n, gpu)
        kw = dict(bias=bv, epilogue=ops.EPI_GEGLU, split_k=split, workspace=ws, use_table=False)
        plan = ops.gemm_launch_plan(av, wv, out, **kw)
        assert plan[2] == n and (plan[5] == 0) == generic, f"GEGLU K={K} split_k={split}: plan {plan}"
        ops.gemm(av, wv, out, **kw)
        torch.cuda.synchronize()
        _guards_intact("GEGLU out", obuf, oidx)
        _bands_intact("GEGLU", wsbuf, M * 2 * inner * 4 * n)
        first = _bits(out).clone() if first is None else first
        assert torch.equal(_bits(out), first), "GEGLU: repeats differ bit-wise"
    assert bool(torch.isfinite(out).all()), "GEGLU: non-finite output"
    err = out.double() - ref
    l2 = (err.norm(dim=1) / ref.norm(dim=1)).max()
    mx = (err.abs().amax(1) / ref.abs().amax(1)).max()
    print(f"GEGLU K={K} split_k={split}: worst row rel-L2 {float(l2):.2e} (bar {GEGLU_L2:.0e}), worst row max-rel {float(mx):.2e} (bar {GEGLU_MAX:.0e})")
    assert float(l2) <= GEGLU_L2 and float(mx) <= GEGLU_MAX


@pytest.mark.parametrize("split", [7, 64])
@pytest.mark.parametrize("shapes", [((100, 72, 640), (130, 200, 192)), ((100, 72, 136), (64, 64, 72))], ids=["one-launch", "generic-fallback"])
def test_gemm_pair_forced_split(gpu, shapes, split):
    """sg_gemm_pair_f16 with a forced split on both problems: one launch on the first problem's tile (the latency kernel here), two generic
    launches for K % 64 != 0; every term, windows and NaN workspaces as everywhere else."""
    from storygen_amd import ops
    args, outs = [], []
    for M, N, K in shapes:
        p, ref, core = _gemm_problem(M, N, K)
        cbuf, c, cidx = _out_window((M, N), F32, gpu)
        n = min(split, -(-K // 64))
        wsbuf, ws = _workspace(M * N * 4 * n, gpu)
        kw = dict(bias=p["bias"], rowbias=p["rowbias"], rows_per_batch=p["rows_per_batch"], res1=p["res1"], res2=p["res2"], split_k=split, workspace=ws)
        args.append(((p["a"], p["w"], c), kw))
        outs.append((cbuf, c, cidx, wsbuf, M * N * 4 * n, ref, core, (64, 64, n), K))
    first = None
    for _ in range(3):
        for o in outs:
            _bits(o[0]).fill_(SENT32)
            o[3][BAND:BAND + o[4]] = WS_FILL
        ops.gemm_pair(args[0], args[1])
        torch.cuda.synchronize()
        got = [_bits(o[1]).clone() for o in outs]
        first = got if first is None else first
        assert all(torch.equal(g, f) for g, f in zip(got, first)), "pair: repeats differ bit-wise"
    for i, (cbuf, c, cidx, wsbuf, nbytes, ref, core, plan, K) in enumerate(outs):
        _guards_intact(f"pair[{i}] C", cbuf, cidx)
        _bands_intact(f"pair[{i}]", wsbuf, nbytes)
        _assert_bar(f"pair[{i}] {shapes[i]} split_k={split}: C", c, ref, core + U * ref.abs(), plan, K)


# ---------------------------------------------------------------------------------------------------------------------- convolution
@functools.lru_cache(maxsize=None)
def _conv_problem(B, H, W, Cin, Cout, stride, ups):
    dev = torch.device("cuda:0")
    x = _randn((B, H, W, Cin), dev, 1)
    w = _randn((Cout, 3, 3, Cin), dev, 2, scale=(9 * Cin) ** -0.5)
    xin = x.repeat_interleave(2, 1).repeat_interleave(2, 2) if ups else x
    hin, win = xin.shape[1], xin.shape[2]
    Ho, Wo = (hin - 1) // stride + 1, (win - 1) // stride + 1
    xz = torch.zeros(B, hin + 2, win + 2, Cin, dtype=F16, device=dev)
    xz[:, 1:-1, 1:-1] = xin
    # im2col in the weights' (ky, kx, ci) order: tap (ky, kx) of output (oy, ox) is bordered pixel (oy stride + ky, ox stride + kx)
    cols = torch.cat([xz[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] for ky in range(3) for kx in range(3)], 3)
    cols = cols.reshape(B * Ho * Wo, 9 * Cin).double()
    wm = w.reshape(Cout, 9 * Cin).double()
    bias, rb = _randn((Cout,), dev, 3), _randn((B, Cout), dev, 4, F32)
    r1 = _randn((B, Ho, Wo, Cout), dev, 5, F32)
    M = B * Ho * Wo
    rows = torch.arange(M, device=dev) // (Ho * Wo)
    terms = [bias.double().expand(M, Cout), rb.double()[rows], r1.double().reshape(M, Cout)]
    acc = cols @ wm.t()
    ref = acc + terms[0] + terms[1] + terms[2]
    core_acc = _gamma(9 * Cin) * (cols.abs() @ wm.abs().t())
    core = core_acc + U * sum(t.abs() for t in terms)
    xpad = torch.zeros(B, H + 2, W + 2, Cin, dtype=F16, device=dev)
    xpad[:, 1:-1, 1:-1] = x
    ops_in = dict(x=_nan_window(x), xpad=_nan_window(xpad), w=_nan_fenced(w), bias=_nan_fenced(bias), rowbias=_nan_fenced(rb), res1=_nan_window(r1))
    return ops_in, (B, Ho, Wo, Cout), ref, core, acc, core_acc


def _run_conv(what, geom, *, padded, split_k, tile=None, out_f32=True, ws_bytes=None, repeats=1, stats=False):
    from storygen_amd import ops
    dev = torch.device("cuda:0")
    B, H, W, Cin, Cout, stride, ups = geom
    p, oshape, ref, core, _, _ = _conv_problem(*geom)
    M, K = oshape[0] * oshape[1] * oshape[2], 9 * Cin
    ybuf, y, yidx = _out_window(oshape, F32 if out_f32 else F16, dev)
    x = p["xpad"] if padded else p["x"]
    kw = dict(stride=stride, upsample2x=ups, bias=p["bias"], rowbias=p["rowbias"], res1=p["res1"], split_k=split_k, x_padded=padded, tile=tile)
    if ws_bytes is None:
        big = torch.empty(M * Cout * 4 * 64, dtype=torch.uint8, device=dev)
        ws_bytes = M * Cout * 4 * ops.conv3x3_planned_splits(x, p["w"], y, workspace=big, **kw)
        ws_bytes = ws_bytes if ws_bytes > M * Cout * 4 else 0
        del big
    wsbuf, ws = _workspace(ws_bytes, dev) if ws_bytes else (None, None)
    kw["workspace"] = ws
    plan = ops.conv3x3_launch_plan(x, p["w"], y, **kw)
    assert plan[2] == ops.conv3x3_planned_splits(x, p["w"], y, **kw)
    _plan_matches(what, plan, split_k, K)
    if split_k == 0 and ws_bytes:
        assert plan[2] <= max(1, ws_bytes // (M * Cout * 4)), f"{what}: {plan[2]} slices planned into a workspace of {ws_bytes} bytes"
    if stats:
        sb_probe = _sent((16,), F32, dev)
        rows = ops.conv3x3_stats_rows(x, p["w"], y, stats=sb_probe, **kw)
        if rows == 0:
            with pytest.raises(RuntimeError, match="statistics"):
                ops.conv3x3(x, p["w"], y, stats=sb_probe, **kw)
            torch.cuda.synchronize()
            _untouched(f"{what}: y after the rejected statistics launch", ybuf)
            _untouched(f"{what}: stats after the rejected statistics launch", sb_probe)
            if wsbuf is not None:
                _workspace_untouched(f"{what}: rejected statistics launch", wsbuf, ws_bytes)
        else:
            sbuf, sview, sidx = _flat_window((M // rows) * 2 * Cout, dev)
            kw["stats"] = sview
    first = None
    for _ in range(repeats):
        _bits(ybuf).fill_(SENT32 if out_f32 else SENT16)
        if ws is not None:
            ws.fill_(WS_FILL)
        ops.conv3x3(x, p["w"], y, **kw)
        torch.cuda.synchronize()
        got = _bits(y).clone()
        first = got if first is None else first
        assert torch.equal(got, first), f"{what}: repeats differ bit-wise"
    _guards_intact(f"{what}: y", ybuf, yidx)
    if wsbuf is not None:
        _bands_intact(what, wsbuf, ws_bytes)
    _assert_bar(f"{what}: y", y.reshape(M, Cout), ref, core + (U if out_f32 else 2.0 ** -11) * ref.abs(), plan, K)
    if "stats" in kw and out_f32:
        rows = M // (sview.numel() // (2 * Cout))
        _guards_intact(f"{what}: stats", sbuf, sidx)
        v = y.reshape(M, Cout).double().view(M // rows, rows, Cout)
        got = sview.view(M // rows, 2, Cout)
        _assert_bar(f"{what}: stats sums", got[:, 0], v.sum(1), _gamma(rows) * v.abs().sum(1) + 1e-300, plan, K)
        _assert_bar(f"{what}: stats squares", got[:, 1], (v * v).sum(1), _gamma(rows + 1) * (v * v).sum(1) + 1e-300, plan, K)
    return plan


# B, H, W, Cin, Cout, stride, upsample2x:  KT = 9;  stride 2 and the nearest-2x gather at KT = 18
SPLIT_CONVS = [(1, 12, 20, 64, 72, 1, False), (2, 8, 8, 128, 64, 2, False), (2, 8, 8, 128, 64, 1, True)]


@pytest.mark.parametrize("split", FORCED)
@pytest.mark.parametrize("padded", [True, False], ids=["padded", "unpadded"])
@pytest.mark.parametrize("geom", SPLIT_CONVS, ids=lambda g: "x".join(str(int(v)) for v in g))
def test_conv_forced_split_every_value(gpu, geom, padded, split):
    """x_padded = 1: the LDS-DMA pipeline; x_padded = 0: the register-staged kernel, which has the 128x128 tile only."""
    assert ("conv", padded, split) not in UNSERVED
    plan = _run_conv(f"conv {geom} {'padded' if padded else 'unpadded'} split_k={split}", geom, padded=padded, split_k=split, repeats=3)
    if not padded:
        assert plan[:2] == (128, 128) and plan[5] == 0, f"the generic kernel was handed tile {plan[:2]}"


@pytest.mark.parametrize("bm,bn", PIPE_TILES)
def test_conv_forced_split_keeps_the_tile(gpu, bm, bn):
    with _tile_forced(bm, bn):
        plan = _run_conv(f"conv tile {bm}x{bn} split_k=7", SPLIT_CONVS[0], padded=True, split_k=7, repeats=3)
        assert plan[:2] == (bm, bn) and plan[5] == 1, f"forced split_k = 7 changed the tile: plan {plan}"


@pytest.mark.parametrize("padded", [True, False], ids=["padded", "unpadded"])
@pytest.mark.parametrize("split", [16, 64])
def test_conv_deferred_reduce_with_more_slices_than_slabs(gpu, split, padded):
    """defer_reduce with split_k above KT = 9: the launch defers with the slice count sg_conv3x3_planned_splits reports (9), writes that
    many raw partial tiles and nothing else; their sum in slice order is the plain product."""
    from storygen_amd import ops
    geom = SPLIT_CONVS[0]
    p, oshape, _, _, acc, core_acc = _conv_problem(*geom)
    M, Cout = acc.shape
    x = p["xpad"] if padded else p["x"]
    ybuf, y, _ = _out_window(oshape, F32, gpu)
    wsbuf, ws = _workspace(M * Cout * 4 * 9, gpu)
    kw = dict(bias=p["bias"], rowbias=p["rowbias"], res1=p["res1"], split_k=split, x_padded=padded, workspace=ws)
    n = ops.conv3x3_planned_splits(x, p["w"], y, **kw)
    assert n == 9
    ops.conv3x3(x, p["w"], y, defer_reduce=True, **kw)
    torch.cuda.synchronize()
    _untouched("y of a deferred launch", ybuf)
    _bands_intact("deferred launch", wsbuf, M * Cout * 4 * n)
    parts = ws.view(F32).view(n, M, Cout)
    assert bool(torch.isfinite(parts).all()), "a partial tile of the deferred launch was not written (the workspace was NaN before)"
    total = parts[0].clone()
    for z in range(1, n):
        total += parts[z]
    _assert_bar(f"deferred conv split_k={split}: sum of the {n} partial tiles", total, acc, core_acc + U * acc.abs(), (64, 64, n), 9 * geom[3])
    # a launch that does not split cannot defer: the documented error, consistently with the query
    kw["split_k"] = 1
    assert ops.conv3x3_planned_splits(x, p["w"], y, **kw) == 1
    with pytest.raises(RuntimeError, match="needs a split-K launch"):
        ops.conv3x3(x, p["w"], y, defer_reduce=True, **kw)


# ------------------------------------------------------------------------------------- 2. nothing outside the views
# family -> (tile height bm, K, debug tile or None, tile hint or None, forced split).  The pipeline families run K = 192 (KT = 3); the
# generic kernel K = 136 and K = 200 (a partial last slab: its zero-fill predicates); split 3 runs both second passes' producers.
FAMILIES = {
    **{f"pipe{bm}x{bn}": (bm, 192, (bm, bn, False), None, 1) for bm, bn in PIPE_TILES},
    "generic-K136": (128, 136, (128, 128, True), None, 1),
    "generic-K200": (128, 200, (128, 128, True), None, 1),
    "lat64x64": (64, 192, None, (64, 64, 4), 1),
    "lat64x128": (64, 192, None, (64, 128, 8), 1),
    "fat512x128": (512, 192, None, (512, 128, 8), 1),
    "fat256x256": (256, 192, None, (256, 256, 8), 1),
    "split3-pipe": (128, 192, None, (0, 0, -1), 3),
    "split3-generic": (128, 136, (128, 128, True), None, 3),
    "split3-lat": (64, 192, None, (64, 64, 4), 3),
    "auto-oddws": (64, 2048, None, None, 0),         # split_k = 0 with 2.5 partial tiles of workspace: at most two slices (KT = 32)
}
M_EDGES = ["1", "63", "65", "bm-1", "bm+1", "2bm"]      # 2bm: whole row tiles, where the epilogue statistics exist (T > 0)
N_EDGES = [8, 72, 136, 200, 128]                        # 128: N % 64 == 0, where ln_stats_out and the split-K statistics exist


def _assert_family(what, family, plan, padded=True):
    """The launch runs on the kernel family (and tile) its parameter names: plan[5] = 0 register-staged, 1 LDS-DMA pipeline, 2 fat waves,
    16 + ring depth the latency kernel."""
    if not padded or "generic" in family:
        want = plan[:2] == (128, 128) and plan[5] == 0
    elif family.startswith("pipe"):
        want = plan[5] == 1 and f"pipe{plan[0]}x{plan[1]}" == family
    elif family.startswith("fat"):
        want = plan[5] == 2 and f"fat{plan[0]}x{plan[1]}" == family
    elif "lat" in family:
        want = plan[5] >= 16 and plan[:2] == ((64, 128) if family.endswith("128") else (64, 64))
    elif family == "split3-pipe":
        want = plan[5] == 1
    else:                       # auto, split3, auto-oddws: the cost model's tile on one of the LDS-DMA kernels
        want = plan[5] != 0
    assert want, f"{what}: planned as {plan}, not on the family the case names"


def _m_of(edge, bm):
    return {"1": 1, "63": 63, "65": 65, "bm-1": bm - 1, "bm+1": bm + 1, "2bm": 2 * bm}[edge]


@pytest.mark.parametrize("N", N_EDGES)
@pytest.mark.parametrize("edge", M_EDGES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_gemm_stays_inside_its_views(gpu, family, edge, N):
    from storygen_amd import ops
    bm, K, dbg, hint, split = FAMILIES[family]
    M = _m_of(edge, bm)
    ws_bytes = ops.gemm_workspace_bytes(M, N, split) if split > 1 else (10 * M * N if split == 0 else 0)
    with _tile_forced(*(dbg or (0, 0, False))):
        for out_f32 in (True, False):
            what = f"gemm {family} M={M} N={N} K={K} {'fp32' if out_f32 else 'fp16'} out"
            plan = _run_gemm(what, M, N, K, split_k=split, tile=hint, out_f32=out_f32, ws_bytes=ws_bytes, ln_out=N % 64 == 0, stats=out_f32)
            _assert_family(what, family, plan)


VIEW_CONVS = [(1, 1, 1, 1, False), (1, 3, 5, 1, False), (2, 7, 9, 2, False), (1, 4, 4, 1, True)]
VIEW_CHANNELS = [(64, 8), (64, 72), (128, 136)]
CONV_FAMILIES = {"auto": (None, None, 1), "split3": (None, None, 3), "auto-oddws": (None, None, 0),
                 **{f"pipe{bm}x{bn}": ((bm, bn, False), None, 1) for bm, bn in PIPE_TILES},
                 "lat64x64": (None, (64, 64, 4), 1), "fat512x128": (None, (512, 128, 8), 1)}


# x_padded = 0 is the register-staged kernel whatever tile is asked for: the tile families would only repeat it
CONV_FAMILY_CASES = [(f, True) for f in CONV_FAMILIES] + [(f, False) for f, v in CONV_FAMILIES.items() if not (v[0] or v[1])]


@pytest.mark.parametrize("family,padded", CONV_FAMILY_CASES, ids=[f"{f}-{'padded' if q else 'unpadded'}" for f, q in CONV_FAMILY_CASES])
@pytest.mark.parametrize("Cin,Cout", VIEW_CHANNELS)
@pytest.mark.parametrize("B,H,W,stride,ups", VIEW_CONVS)
def test_conv_stays_inside_its_views(gpu, B, H, W, stride, ups, Cin, Cout, padded, family):
    from storygen_amd import ops
    dbg, hint, split = CONV_FAMILIES[family]
    geom = (B, H, W, Cin, Cout, stride, ups)
    oshape = _conv_problem(*geom)[1]
    M = oshape[0] * oshape[1] * oshape[2]
    ws_bytes = ops.gemm_workspace_bytes(M, Cout, split) if split > 1 else (10 * M * Cout if split == 0 else 0)
    with _tile_forced(*(dbg or (0, 0, False))):
        for out_f32 in (True, False):
            what = f"conv {family} {geom} {'padded' if padded else 'unpadded'} {'fp32' if out_f32 else 'fp16'} out"
            plan = _run_conv(what, geom, padded=padded, split_k=split, tile=hint, out_f32=out_f32, ws_bytes=ws_bytes, stats=out_f32)
            _assert_family(what, family, plan, padded)


# ------------------------------------------------------------------------------------------- 3. the 32-bit offset bound
LD_BIG = 65536


def _ends_check(what, out, a_rows, w_rows, K, plan):
    """out rows against float64 for the given operand rows, with the bar of section 1 (no epilogue term, fp32 output)."""
    ref = a_rows.double() @ w_rows.double().t()
    bar = _gamma(K) * (a_rows.double().abs() @ w_rows.double().abs().t()) + U * ref.abs()
    _assert_bar(what, out, ref, bar, plan, K)


def test_gemm_a_operand_ends_just_inside_4_gib(gpu):
    """(M - 1) lda + K <= 2^31 elements with lda = 65536, K = 64: M = 32768 is the largest admitted; its last row starts 4 GiB - 128 KiB
    from the base.  M = 32769 (row 32768 would wrap to row 0) is rejected by the descriptor check: nothing is launched."""
    from storygen_amd import ops
    K, N, M = 64, 64, (2 ** 31 - 64) // LD_BIG + 1
    assert (M - 1) * LD_BIG + K <= 2 ** 31 < M * LD_BIG + K
    buf = torch.empty((M + 1, LD_BIG), dtype=F16, device=gpu)          # 4 GiB + 128 KiB, never filled
    try:
        a = buf[:M, :K]
        a.copy_(_randn((M, K), gpu, 11))
        w = _randn((N, K), gpu, 12, scale=K ** -0.5)
        out = torch.empty(M, N, dtype=F32, device=gpu)
        plan = ops.gemm_launch_plan(a, w, out, split_k=1, use_table=False)
        assert plan[5] != 0, "the LDS-DMA kernels are what the bound is about"
        ops.gemm(a, w, out, split_k=1, use_table=False)
        _ends_check("A just inside: first 128 rows", out[:128], a[:128], w, K, plan)
        _ends_check("A just inside: last 128 rows", out[-128:], a[-128:], w, K, plan)
        sbuf, sview, _ = _out_window((M + 1, N), F32, gpu)
        with pytest.raises(RuntimeError, match=r"operand A spans .*2\^31 elements"):
            ops.gemm(buf[:M + 1, :K], w, sview, split_k=1, use_table=False)
        torch.cuda.synchronize()
        _untouched("output of the rejected launch", sbuf)
    finally:
        del buf
        torch.cuda.empty_cache()


def test_gemm_w_operand_ends_just_inside_4_gib(gpu):
    """The roles swapped: W row-strided with ldw = 65536, N = 32768 the largest admitted, N + 8 (the next valid N) rejected."""
    from storygen_amd import ops
    K, M, N = 64, 64, (2 ** 31 - 64) // LD_BIG + 1
    assert N % 8 == 0 and (N - 1) * LD_BIG + K <= 2 ** 31 < (N + 7) * LD_BIG + K
    buf = torch.empty((N + 8, LD_BIG), dtype=F16, device=gpu)
    try:
        w = buf[:N, :K]
        w.copy_(_randn((N, K), gpu, 13, scale=K ** -0.5))
        a = _randn((M, K), gpu, 14)
        out = torch.empty(M, N, dtype=F32, device=gpu)
        plan = ops.gemm_launch_plan(a, w, out, split_k=1, use_table=False)
        assert plan[5] != 0
        ops.gemm(a, w, out, split_k=1, use_table=False)
        _ends_check("W just inside: first 128 columns", out[:, :128], a, w[:128], K, plan)
        _ends_check("W just inside: last 128 columns", out[:, -128:], a, w[-128:], K, plan)
        sbuf, sview, _ = _out_window((M, N + 8), F32, gpu)
        with pytest.raises(RuntimeError, match=r"operand W spans .*2\^31 elements"):
            ops.gemm(a, buf[:N + 8, :K], sview, split_k=1, use_table=False)
        torch.cuda.synchronize()
        _untouched("output of the rejected launch", sbuf)
    finally:
        del buf
        torch.cuda.empty_cache()


def test_conv_padded_input_ends_just_inside_4_gib(gpu):
    """A 64-channel window of pixels 4 194 296 elements apart (W + 2 = 4 pixels a row: the row pitch stays below 2^24): B (H+2) (W+2) = 512
    pixels end inside 2^31 elements, H = 127 (516 pixels) does not."""
    from storygen_amd import ops
    Cin, Cout, W, ldx = 64, 64, 2, 2 ** 22 - 8
    H = 126
    assert ((H + 2) * (W + 2) - 1) * ldx + Cin <= 2 ** 31 < ((H + 3) * (W + 2) - 1) * ldx + Cin
    buf = torch.empty(((H + 3) * (W + 2) * ldx,), dtype=F16, device=gpu)       # 4.03 GiB, never filled
    try:
        x = _randn((1, H, W, Cin), gpu, 15)
        xp = buf[:(H + 2) * (W + 2) * ldx].view(1, H + 2, W + 2, ldx)[..., :Cin]
        xp.zero_()
        xp[:, 1:-1, 1:-1] = x
        w = _randn((Cout, 3, 3, Cin), gpu, 16, scale=(9 * Cin) ** -0.5)
        out = torch.empty(1, H, W, Cout, dtype=F32, device=gpu)
        plan = ops.conv3x3_launch_plan(xp, w, out, split_k=1, x_padded=True)
        assert plan[5] != 0
        ops.conv3x3(xp, w, out, split_k=1, x_padded=True)
        xz = xp.contiguous()
        cols = torch.cat([xz[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], 3).reshape(H * W, 9 * Cin)
        o = out.reshape(H * W, Cout)
        _ends_check("x just inside: first 128 pixels", o[:128], cols[:128], w.reshape(Cout, -1), 9 * Cin, plan)
        _ends_check("x just inside: last 128 pixels", o[-128:], cols[-128:], w.reshape(Cout, -1), 9 * Cin, plan)
        sbuf, sview, _ = _out_window((1, H + 1, W, Cout), F32, gpu)
        with pytest.raises(RuntimeError, match=r"input x spans .*2\^31 elements"):
            ops.conv3x3(buf.view(1, H + 3, W + 2, ldx)[..., :Cin], w, sview, split_k=1, x_padded=True)
        torch.cuda.synchronize()
        _untouched("output of the rejected launch", sbuf)
    finally:
        del buf
        torch.cuda.empty_cache()
