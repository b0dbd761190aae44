"""Per-kernel parity: every C-ABI entry point vs a plain PyTorch fp32 reference of the same op on the same
fp16-rounded inputs (tolerance: fp16 output rounding, rel-L2 <= 1e-3, max-abs <= 3e-3 of the output range)."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import max_rel, rel_l2

pytestmark = pytest.mark.gpu

TOL_L2 = 1.0e-3
TOL_MAX = 3.0e-3


def rnd(shape, dev, scale=1.0, seed=0, dtype=torch.float16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def check(out, ref, what, l2=TOL_L2, mx=TOL_MAX):
    assert torch.isfinite(out.float()).all(), f"{what}: non-finite output"
    e2, em = rel_l2(out.float().cpu(), ref.float().cpu()), max_rel(out.float().cpu(), ref.float().cpu())
    assert e2 <= l2 and em <= mx, f"{what}: rel-L2 {e2:.2e} (tol {l2:.0e}), max-rel {em:.2e} (tol {mx:.0e})"


def test_mfma_fragment_layout(gpu):
    """Pins the v_mfma_f32_32x32x16_f16 operand/result lane maps every MFMA kernel here assumes:
    A[i=l&31][k=8(l>>5)+j], B[k][n=l&31], D[row=(r&3)+8(r>>2)+4(l>>5)][col=l&31] (asymmetric operands)."""
    from storygen_amd import ops
    a = rnd((32, 16), gpu, seed=1)
    b = rnd((16, 32), gpu, seed=2)
    raw = ops.debug_mfma(a.contiguous(), b.contiguous()).cpu()
    ref = (a.float() @ b.float()).cpu()
    got = torch.empty(32, 32)
    for lane in range(64):
        for r in range(16):
            got[(r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), lane & 31] = raw[lane, r]
    check(got, ref, "mfma layout", l2=1e-5, mx=1e-5)


TILES = [(0, 0, False), (256, 128, False), (128, 128, False), (256, 64, False), (128, 64, False), (64, 128, False), (64, 64, False),
         (128, 128, True)]


@pytest.fixture(params=TILES, ids=lambda t: f"tile{t[0]}x{t[1]}{'-generic' if t[2] else ''}")
def tile(request, gpu):
    """Runs the test once per GEMM/conv tile shape and kernel family (LDS-DMA pipeline vs generic)."""
    from storygen_amd import ops
    ops.debug_set_tile(*request.param)
    yield request.param
    ops.debug_set_tile(0, 0, False)


GEMM_SHAPES = [
    # M, N, K            (tails in M and N, K not a multiple of 64, tiny, SD-1.5 layer shapes)
    (128, 128, 64), (256, 320, 320), (200, 72, 136), (12, 320, 1280), (3072, 640, 640), (768, 1280, 2560),
    (4096, 960, 320), (231, 2560, 768), (64, 1280, 11520 // 4),
]


@pytest.mark.parametrize("M,N,K", [(256, 320, 320), (200, 72, 128), (3072, 640, 640), (300, 1280, 1920)])
def test_gemm_all_tiles_fp32_stream(gpu, tile, M, N, K):
    """Every tile shape / kernel family; fp32 output, fp32 + fp16 residuals, second fp16 copy of the output."""
    from storygen_amd import ops
    a, w = rnd((M, K), gpu, seed=3), rnd((N, K), gpu, 1 / math.sqrt(K), seed=4)
    bias, r1 = rnd((N,), gpu, seed=5), rnd((M, N), gpu, seed=6, dtype=torch.float32)
    r2 = rnd((M, N), gpu, seed=7)
    ref = a.float() @ w.float().t() + bias.float() + r1 + r2.float()
    out = torch.empty(M, N, dtype=torch.float32, device=gpu)
    out16 = torch.empty(M, N, dtype=torch.float16, device=gpu)
    ops.gemm(a, w, out, bias=bias, res1=r1, res2=r2, split_k=1, out2=out16)
    check(out, ref, "fp32 out", l2=2e-6, mx=2e-5)
    check(out16, ref, "fp16 copy")
    ops.gemm(a, w, out16, bias=bias, res1=r2, res2=r1, split_k=1)
    check(out16, ref, "fp16 out, swapped residual dtypes")


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_linear_epilogues(gpu, M, N, K):
    from storygen_amd import ops
    a, w = rnd((M, K), gpu, seed=3), rnd((N, K), gpu, 1 / math.sqrt(K), seed=4)
    bias, r1, r2 = rnd((N,), gpu, seed=5), rnd((M, N), gpu, seed=6), rnd((M, N), gpu, seed=7)
    rpb = max(1, M // 3)
    rb = rnd((-(-M // rpb), N), gpu, seed=8, dtype=torch.float32)
    acc = a.float() @ w.float().t()
    out = torch.empty(M, N, dtype=torch.float16, device=gpu)
    ops.gemm(a, w, out, split_k=1)
    check(out, acc, "plain")
    ops.gemm(a, w, out, bias=bias, res1=r1, res2=r2, rowbias=rb, rows_per_batch=rpb, split_k=1)
    ref = acc + bias.float() + r1.float() + r2.float() + rb.repeat_interleave(rpb, 0)[:M]
    check(out, ref, "bias+rowbias+res1+res2")


@pytest.mark.parametrize("M,N,K,split", [(192, 1280, 1280, 4), (768, 1280, 11520, 6), (100, 72, 640, 3), (64, 640, 5120, 0)])
def test_gemm_split_k(gpu, M, N, K, split):
    from storygen_amd import ops
    a, w = rnd((M, K), gpu, seed=3), rnd((N, K), gpu, 1 / math.sqrt(K), seed=4)
    bias, r1 = rnd((N,), gpu, seed=5), rnd((M, N), gpu, seed=6)
    ws = torch.empty(ops.gemm_workspace_bytes(M, N, split), dtype=torch.uint8, device=gpu)
    out = torch.empty(M, N, dtype=torch.float16, device=gpu)
    ops.gemm(a, w, out, bias=bias, res1=r1, split_k=split, workspace=ws)
    check(out, a.float() @ w.float().t() + bias.float() + r1.float(), f"split_k={split}")


def test_tile_waves_hint_is_validated(gpu):
    """Every wave owns a 64x64 sub-tile (the 128x64-per-wave variants of round 1 were 12-25 % slower and are gone): tile_waves
    accepts 0 or the tile's own wave count, anything else is an error."""
    from storygen_amd import ops
    a, w = rnd((256, 128), gpu, seed=1), rnd((128, 128), gpu, 128 ** -0.5, seed=2)
    out = torch.empty(256, 128, dtype=torch.float32, device=gpu)
    ops.gemm(a, w, out, tile=(128, 128, 4))
    check(out, a.float() @ w.float().t(), "tile_waves = natural count", l2=2e-6, mx=2e-5)
    with pytest.raises(RuntimeError, match="tile_waves"):
        ops.gemm(a, w, out, tile=(128, 128, 2))


@pytest.mark.parametrize("M,C,split", [(4096, 320, 1), (1000, 640, 1), (768, 1280, 4), (192, 1280, 0), (64, 64, 1)])
def test_gemm_layernorm_fold(gpu, M, C, split):
    """LayerNorm folded into the consuming GEMM (sg_gemm_desc.ln_*; model/attention.py:250,268,283,298): a producer GEMM writes the
    fp32 stream x, its fp16 copy and the per-token (sum, M2) partials per 64-channel block (fused epilogue or split-K reduce); the
    consumers run on the raw copy with gamma-scaled weights and normalise in their epilogues — rows-are-tokens (q | k), the
    transposed V^T product (columns are tokens) and GEGLU.  Reference: torch LayerNorm -> Linear in fp32 on the fp32 stream.
    The stream carries a large common offset (|mean| = 3 sigma) so a cancellation in the fold would show."""
    from storygen_amd import ops
    from storygen_amd.repack import fold_layernorm, interleave_geglu
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=gpu)
    a0, w0 = rnd((M, C), gpu, 1.0, 1), rnd((C, C), gpu, C ** -0.5, 2)
    res = rnd((M, C), gpu, 1.0, 3, torch.float32) + 3.0
    x = torch.empty(M, C, dtype=torch.float32, device=gpu)
    x16 = torch.empty(M, C, dtype=torch.float16, device=gpu)
    P = C // 64
    st = torch.full((M, (P + 1) & ~1, 2), float("nan"), dtype=torch.float32, device=gpu)      # padded to an even number of blocks
    ops.gemm(a0, w0, x, bias=rnd((C,), gpu, 1.0, 4), res1=res, out2=x16, ln_out=st, split_k=split, workspace=ws)
    blocks = x.view(M, P, 64).double()
    check(st[:, :P, 0], blocks.sum(-1), "block sums", l2=1e-6, mx=1e-4)
    check(st[:, :P, 1], ((blocks - blocks.mean(-1, keepdim=True)) ** 2).sum(-1), "block M2", l2=1e-5, mx=1e-3)
    gamma, beta = rnd((C,), gpu, 0.3, 5) + 1.0, rnd((C,), gpu, 0.3, 6)
    ln = F.layer_norm(x, (C,), gamma.float(), beta.float(), 1e-5)
    # rows are tokens: a q | k style projection with a bias
    wq, bq = rnd((2 * C, C), gpu, C ** -0.5, 7), rnd((2 * C,), gpu, 1.0, 8)
    wf, c, d = fold_layernorm(wq, bq, gamma, beta)
    out = torch.full((M, 2 * C), float("nan"), dtype=torch.float16, device=gpu)
    ops.gemm(x16, wf, out, ln=(1, st, c, d, 1e-5))
    check(out, ln @ wq.float().t() + bq.float(), "LayerNorm fold, rows = tokens", l2=1.5e-3, mx=2e-2)
    # columns are tokens: V^T = W_v LN(x)^T
    wv = rnd((C, C), gpu, C ** -0.5, 9)
    wvf, cv, dv = fold_layernorm(wv, None, gamma, beta)
    Mp = (M + 7) & ~7
    vt = torch.full((C, Mp), float("nan"), dtype=torch.float16, device=gpu)[:, :M]
    ops.gemm(wvf, x16, vt, ln=(2, st, cv, dv, 1e-5))
    check(vt, wv.float() @ ln.t(), "LayerNorm fold, columns = tokens", l2=1.5e-3, mx=2e-2)
    # GEGLU on the folded LayerNorm
    wg, bg = rnd((8 * C, C), gpu, C ** -0.5, 10), rnd((8 * C,), gpu, 1.0, 11)
    wi, bi = interleave_geglu(wg, bg)
    wif, ci, di = fold_layernorm(wi, bi, gamma, beta)
    og = torch.full((M, 4 * C), float("nan"), dtype=torch.float16, device=gpu)
    ops.gemm(x16, wif, og, epilogue=ops.EPI_GEGLU, ln=(1, st, ci, di, 1e-5))
    val, gate = (ln @ wg.float().t() + bg.float()).chunk(2, dim=-1)
    check(og, val * F.gelu(gate), "LayerNorm fold + GEGLU", l2=2e-3, mx=3e-2)
    # both consumers of one LayerNorm in one launch
    o1, o2 = torch.empty_like(out), torch.empty_like(vt)
    ops.gemm_pair(((x16, wf, o1), dict(ln=(1, st, c, d, 1e-5))), ((wvf, x16, o2), dict(ln=(2, st, cv, dv, 1e-5))))
    assert torch.equal(o1, out) and torch.equal(o2, vt)
    with pytest.raises(RuntimeError, match="split"):
        ops.gemm(x16, wf, out, ln=(1, st, c, d, 1e-5), split_k=2, workspace=ws)


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("case", ["in-range", "offset", "range"])
def test_layernorm_fold_guard_and_saturation(gpu, case, split):
    """The two assumptions of the LayerNorm fold, and what the library does when one fails (the reference's
    LayerNorm reads an fp32 tensor and has neither limit, model/attention.py:250,268,283,298):
      offset: a stream whose tokens sit at |mean| = 1e3 sigma — the fp16 copy keeps ~2^-11 |x| = 0.5 sigma of rounding, the folded
              LayerNorm is wrong by O(1), and the consumer raises SG_LN_GUARD_OFFSET;
      range:  |x| ~ 1e5 > 65504 — the fp16 copy is SATURATED (finite everywhere, never inf), the producer raises SG_LN_GUARD_RANGE;
      in-range (|mean| = 3 sigma): no flag, results within the kernel bar.
    In both failing cases the fp32 stream itself is exact, so the unfused LayerNorm launch on it (engine.LN_FOLD = False) is."""
    from storygen_amd import ops
    from storygen_amd.repack import fold_layernorm
    M, C = 512, 320
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=gpu)
    a0, w0 = rnd((M, C), gpu, 1.0, 1), rnd((C, C), gpu, C ** -0.5, 2)
    off = {"in-range": 3.0, "offset": 1.0e3, "range": 1.0e5}[case]
    res = rnd((M, C), gpu, 1.0, 3, torch.float32) + off
    x = torch.empty(M, C, dtype=torch.float32, device=gpu)
    x16 = torch.empty(M, C, dtype=torch.float16, device=gpu)
    P = C // 64
    st = torch.zeros((M, (P + 1) & ~1, 2), dtype=torch.float32, device=gpu)
    guard = torch.zeros(1, dtype=torch.int32, device=gpu)
    ops.gemm(a0, w0, x, res1=res, out2=x16, ln_out=st, guard=guard, split_k=split, workspace=ws)
    want_x = a0.float() @ w0.float().t() + res
    check(x, want_x, "fp32 stream", l2=1e-6, mx=1e-2 if case == "range" else 1e-3)           # exact whatever the magnitude
    assert torch.isfinite(x16).all(), "the fp16 copy must saturate, not overflow"
    if case == "range":
        assert float(x16.float().abs().max()) == 65504.0 and int(guard.item()) & ops.LN_GUARD_RANGE
    else:
        assert not int(guard.item()) & ops.LN_GUARD_RANGE
        check(x16, want_x, "fp16 copy", l2=6e-4, mx=off * 1e-3 + 1e-2)
    gamma, beta = rnd((C,), gpu, 0.3, 5) + 1.0, rnd((C,), gpu, 0.3, 6)
    wq, bq = rnd((2 * C, C), gpu, C ** -0.5, 7), rnd((2 * C,), gpu, 1.0, 8)
    wf, c, d = fold_layernorm(wq, bq, gamma, beta)
    out = torch.full((M, 2 * C), float("nan"), dtype=torch.float16, device=gpu)
    guard.zero_()
    ops.gemm(x16, wf, out, ln=(1, st, c, d, 1e-5), guard=guard)
    want = F.layer_norm(x, (C,), gamma.float(), beta.float(), 1e-5) @ wq.float().t() + bq.float()
    err = float((out.float() - want).norm() / want.norm())
    flags = int(guard.item())
    print(f"LayerNorm fold, |mean| = {off:g} sigma: rel-L2 {err:.2e}, guard flags {flags}")
    assert case == "range" or torch.isfinite(out).all()        # (range: the fp16 OUTPUT of the consumer may overflow like any fp16 GEMM's)
    if case == "in-range":
        assert flags == 0 and err <= 1.5e-3
    else:
        assert flags & ops.LN_GUARD_OFFSET, "a token with |mean| / sigma > 16 must be reported"
        assert not err <= 1e-2, "if the fold were accurate here the guard would be needless"
        # the remedy: the LayerNorm launch on the fp32 stream (what engine.LN_FOLD = False runs) is within the kernel bar
        y = torch.empty(M, C, dtype=torch.float16, device=gpu)
        ops.layernorm(x, gamma, beta, y)
        o2 = torch.empty_like(out)
        ops.gemm(y, wq, o2, bias=bq, workspace=ws)
        # (looser than the in-range bar: at |mean| = 1e3 sigma an fp32 LayerNorm itself keeps ~1e3 x 2^-24 of relative noise per element,
        # on either side of this comparison — measured 2.9e-3)
        check(o2, want, "unfused LayerNorm -> GEMM on the same stream", l2=6e-3, mx=5e-2)


def test_gemm_strided_views(gpu):
    """lda/ldc/ldr larger than the logical widths: operands are column slices of wider buffers."""
    from storygen_amd import ops
    M, N, K = 300, 320, 640
    abuf, cbuf, rbuf = rnd((M, K + 64), gpu, seed=1), torch.zeros(M, N + 128, dtype=torch.float16, device=gpu), rnd((M, 2 * N), gpu, seed=2)
    w = rnd((N, K), gpu, 1 / math.sqrt(K), seed=3)
    a, out, res = abuf[:, 64:], cbuf[:, 64:64 + N], rbuf[:, N:]
    ops.gemm(a, w, out, res1=res, split_k=1)
    check(out, a.float() @ w.float().t() + res.float(), "strided")
    assert float(cbuf[:, :64].abs().max()) == 0 and float(cbuf[:, 64 + N:].abs().max()) == 0, "wrote outside the view"


@pytest.mark.parametrize("M,C", [(4096, 320), (768, 1280), (192, 1280), (1000, 640)])
def test_gemm_pair_is_two_gemms_in_one_launch(gpu, M, C):
    """sg_gemm_pair_f16 on the pairs the engine issues: q|k (token-major, N = 2C) with V^T = Wv . X^T (swapped operands), and two
    plain projections with different inputs, residual / bias epilogues included; split-K (small M) with two workspaces."""
    from storygen_amd import ops
    x, x4 = rnd((M, C), gpu, 1.0, 1), rnd((M, C), gpu, 1.0, 2)
    wqk, wv, wq3 = rnd((2 * C, C), gpu, C ** -0.5, 3), rnd((C, C), gpu, C ** -0.5, 4), rnd((C, C), gpu, C ** -0.5, 5)
    bias, res = rnd((C,), gpu, 1.0, 6), rnd((M, C), gpu, 1.0, 7, torch.float32)
    ws0, ws1 = (torch.empty(64 << 20, dtype=torch.uint8, device=gpu) for _ in range(2))
    qk, vt = torch.empty(M, 2 * C, dtype=torch.float16, device=gpu), torch.empty(C, M, dtype=torch.float16, device=gpu)
    ops.gemm_pair(((x, wqk, qk), dict(workspace=ws0)), ((wv, x, vt), dict(workspace=ws1)))
    check(qk, x.float() @ wqk.float().t(), "pair: q|k")
    check(vt, wv.float() @ x.float().t(), "pair: V^T")
    o0, o1 = torch.empty(M, C, dtype=torch.float32, device=gpu), torch.empty(M, C, dtype=torch.float16, device=gpu)
    ops.gemm_pair(((x, wv, o0), dict(workspace=ws0, bias=bias, res1=res)), ((x4, wq3, o1), dict(workspace=ws1)))
    check(o0, x.float() @ wv.float().t() + bias.float() + res, "pair: bias + fp32 residual")
    check(o1, x4.float() @ wq3.float().t(), "pair: second input")
    with pytest.raises(RuntimeError, match="disjoint"):
        ops.gemm_pair(((x, wv, o0), dict(workspace=ws0)), ((x4, wq3, o1), dict(workspace=ws0)))
    # K % 64 != 0 -> generic kernel -> the pair falls back to two launches, same results
    xk, wk = rnd((M, 72), gpu, 1.0, 8), rnd((C, 72), gpu, 72 ** -0.5, 9)
    ops.gemm_pair(((xk, wk, o1), {}), ((x, wv, o0), {}))
    check(o1, xk.float() @ wk.float().t(), "pair fallback: K = 72")
    check(o0, x.float() @ wv.float().t(), "pair fallback: second")


def test_split_k_is_deterministic_and_its_workspace_reusable(gpu):
    """Split-K partial tiles are summed in slice order by the reduce pass: bit-identical from run to run, one workspace for any
    sequence of shapes / split factors."""
    from storygen_amd import ops
    ws = torch.full((ops.gemm_workspace_bytes(768, 1280, 8),), 0xFF, dtype=torch.uint8, device=gpu)
    ref = {}
    for rep in range(3):
        for M, N, K, split in [(192, 1280, 1280, 4), (768, 1280, 2560, 8), (100, 72, 640, 3), (768, 640, 5120, 0)]:
            a, w, bias = rnd((M, K), gpu, 1.0, 11), rnd((N, K), gpu, K ** -0.5, 12), rnd((N,), gpu, 1.0, 13)
            r1 = rnd((M, N), gpu, 1.0, 14, torch.float32)
            out = torch.empty(M, N, dtype=torch.float32, device=gpu)
            ops.gemm(a, w, out, bias=bias, res1=r1, split_k=split, workspace=ws)
            if rep == 0:
                check(out, a.float() @ w.float().t() + bias.float() + r1, f"split_k={split}")
                ref[(M, N, K)] = out.clone()
            else:
                assert torch.equal(out, ref[(M, N, K)]), (rep, M, N, K)


@pytest.mark.parametrize("M", [128, 4096 * 3, 1000])
def test_fused_geglu_feed_forward(gpu, M):
    """Round 4: sg_ff_geglu_fused_f16 — LayerNorm -> Linear(C, 8C) -> a gelu(g) -> Linear(4C, C)
    -> + x in one launch (C = 320) — against torch fp32 on the same fp16-rounded weights (model/attention.py:298-300,381-393), and
    against the two-launch path it replaces (LayerNorm-folded GEGLU GEMM + second GEMM).  M = 1000: a ragged last workgroup."""
    from storygen_amd import ops
    from storygen_amd.repack import ff_fused_pack, fold_layernorm, interleave_geglu
    C = 320
    assert ops.ff_fused_supported(C) and not ops.ff_fused_supported(640)
    xbig = rnd((M, 2 * C), gpu, 1.5, 1, torch.float32) + 0.4
    x = xbig[:, C // 2: C // 2 + C]                                   # row-strided view of the fp32 stream
    w1, b1 = rnd((8 * C, C), gpu, C ** -0.5, 2), rnd((8 * C,), gpu, 0.5, 3)
    w2, b2 = rnd((C, 4 * C), gpu, (4 * C) ** -0.5, 4), rnd((C,), gpu, 0.5, 5)
    gamma, beta = rnd((C,), gpu, 0.2, 6) + 1.0, rnd((C,), gpu, 0.2, 7)
    w1i, b1i = interleave_geglu(w1, b1)
    w1f, c1, d1 = fold_layernorm(w1i, b1i, gamma, beta)
    pack = ff_fused_pack(w1f.contiguous(), d1.contiguous(), w2)
    out = torch.full((M, C), float("nan"), dtype=torch.float16, device=gpu)
    ops.ff_fused(x, pack, b2, out, 1e-5)
    h = F.layer_norm(x.float(), (C,), gamma.float(), beta.float(), 1e-5) @ w1.float().t() + b1.float()
    ref = (h[:, : 4 * C] * F.gelu(h[:, 4 * C:])) @ w2.float().t() + b2.float() + x
    check(out, ref, "fused GEGLU feed-forward vs torch")
    # the two-launch path on the same operands
    raw, lnst = torch.empty(M, C, dtype=torch.float16, device=gpu), torch.zeros(M, (C // 64 + 1) & ~1, 2, dtype=torch.float32, device=gpu)
    xc = x.contiguous()
    blocks = xc.view(M, C // 64, 64)
    raw.copy_(xc)
    lnst[:, : C // 64, 0] = blocks.sum(-1)
    lnst[:, : C // 64, 1] = ((blocks - blocks.mean(-1, keepdim=True)) ** 2).sum(-1)
    ffi = torch.empty(M, 4 * C, dtype=torch.float16, device=gpu)
    ops.gemm(raw, w1f.contiguous(), ffi, epilogue=ops.EPI_GEGLU, ln=(1, lnst, c1.contiguous(), d1.contiguous(), 1e-5))
    two = torch.empty(M, C, dtype=torch.float16, device=gpu)
    ops.gemm(ffi, w2, two, bias=b2, res1=xc)
    check(two, ref, "two-launch feed-forward vs torch")
    assert rel_l2(out.float().cpu(), two.float().cpu()) < 1e-3
    # the schedule variants (development option ff_variant) compute the same values in the same order
    try:
        for var in (1, 2, 3):
            ops.debug_set_option("ff_variant", var)
            o = torch.full((M, C), float("nan"), dtype=torch.float16, device=gpu)
            ops.ff_fused(x, pack, b2, o, 1e-5)
            torch.cuda.synchronize()
            assert torch.equal(o, out), f"ff_variant {var}"
    finally:
        ops.debug_set_option("ff_variant", 3)
    # hidden split (round 5, sg_ff_desc.hidden_split): two workgroups per 128 tokens, each over half of the hidden units; the first half's
    # sum + b2 + x in columns [0, C), the second half's partial sum in [C, 2C) — their sum is the result, and the consumer gets it for
    # free by contracting [y_a | y_b] with [W | W] (what the engine's proj_out does)
    sp = torch.full((M, 2 * C), float("nan"), dtype=torch.float16, device=gpu)
    ops.ff_fused(x, pack, b2, sp, 1e-5, split=True)
    check(sp[:, :C].float() + sp[:, C:].float(), ref, "hidden-split feed-forward, sum of the halves, vs torch")
    wo, bo = rnd((C, C), gpu, C ** -0.5, 8), rnd((C,), gpu, 0.5, 9)
    y1, y2 = torch.empty(M, C, dtype=torch.float32, device=gpu), torch.empty(M, C, dtype=torch.float32, device=gpu)
    ops.gemm(out, wo, y1, bias=bo, res1=xc)
    ops.gemm(sp, torch.cat([wo, wo], dim=1).contiguous(), y2, bias=bo, res1=xc)
    check(y2, ref @ wo.float().t() + bo.float() + xc, "proj_out over the two halves vs torch")
    assert rel_l2(y2.cpu(), y1.cpu()) < 6e-4


@pytest.mark.parametrize("M,C,split", [(256, 320, 1), (100, 64, 1), (192, 1280, 3)])
def test_gemm_geglu(gpu, M, C, split):
    """GEGLU.proj + gelu gate (model/attention.py:381-393) with the 32/32 value/gate row interleave."""
    from storygen_amd import ops
    from storygen_amd.repack import interleave_geglu
    K, inner = C, 4 * C
    a = rnd((M, K), gpu, seed=1)
    w = rnd((2 * inner, K), gpu, 1 / math.sqrt(K), seed=2)
    b = rnd((2 * inner,), gpu, seed=3)
    proj = a.float() @ w.float().t() + b.float()
    ref = proj[:, :inner] * F.gelu(proj[:, inner:])
    wi, bi = interleave_geglu(w, b)
    out = torch.empty(M, inner, dtype=torch.float16, device=gpu)
    ws = torch.empty(ops.gemm_workspace_bytes(M, 2 * inner, split), dtype=torch.uint8, device=gpu) if split > 1 else None
    ops.gemm(a, wi, out, bias=bi, epilogue=ops.EPI_GEGLU, split_k=split, workspace=ws)
    check(out, ref, "geglu")


CONV_CASES = [
    # B, H, W, Cin, Cout, stride, ups, split
    (2, 16, 16, 64, 64, 1, False, 1), (3, 8, 8, 128, 320, 1, False, 1), (1, 12, 20, 64, 72, 1, False, 1),
    (2, 16, 16, 64, 128, 2, False, 1), (2, 8, 8, 128, 64, 1, True, 1), (3, 8, 8, 1280, 1280, 1, False, 0),
    (1, 10, 6, 192, 136, 2, False, 1), (3, 16, 16, 640, 640, 1, False, 4),
]


@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,ups,split", CONV_CASES)
def test_conv3x3(gpu, B, H, W, Cin, Cout, stride, ups, split):
    """3x3 pad-1 conv (stride 1/2, fused nearest-2x upsample) with bias + per-batch channel bias + residual."""
    from storygen_amd import ops
    x = rnd((B, Cin, H, W), gpu, seed=1)
    w = rnd((Cout, Cin, 3, 3), gpu, 1 / math.sqrt(9 * Cin), seed=2)
    bias = rnd((Cout,), gpu, seed=3)
    rb = rnd((B, Cout), gpu, seed=4, dtype=torch.float32)
    xin = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if ups else x.float()
    ref = F.conv2d(xin, w.float(), bias.float(), stride=stride, padding=1) + rb[:, :, None, None]
    res = rnd(tuple(ref.shape), gpu, seed=5)
    ref = ref + res.float()
    x_nhwc = x.permute(0, 2, 3, 1).contiguous()
    w_krsc = w.permute(0, 2, 3, 1).contiguous()
    res_nhwc = res.permute(0, 2, 3, 1).contiguous()
    out = torch.empty(B, ref.shape[2], ref.shape[3], Cout, dtype=torch.float16, device=gpu)
    M = B * ref.shape[2] * ref.shape[3]
    ws = torch.empty(max(16, ops.gemm_workspace_bytes(M, Cout, split)), dtype=torch.uint8, device=gpu)
    ops.conv3x3(x_nhwc, w_krsc, out, stride=stride, upsample2x=ups, bias=bias, rowbias=rb, res1=res_nhwc, split_k=split,
                workspace=ws)
    check(out.permute(0, 3, 1, 2), ref, "conv3x3")


@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,ups,split", CONV_CASES)
def test_conv3x3_padded_input_all_tiles(gpu, tile, B, H, W, Cin, Cout, stride, ups, split):
    """Zero-bordered input (LDS-DMA pipelined kernel when the tile is not '-generic'), fp32 output + fp32 residual."""
    from storygen_amd import ops
    x = rnd((B, Cin, H, W), gpu, seed=1)
    w = rnd((Cout, Cin, 3, 3), gpu, 1 / math.sqrt(9 * Cin), seed=2)
    bias = rnd((Cout,), gpu, seed=3)
    rb = rnd((B, Cout), gpu, seed=4, dtype=torch.float32)
    xin = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if ups else x.float()
    ref = F.conv2d(xin, w.float(), bias.float(), stride=stride, padding=1) + rb[:, :, None, None]
    res = rnd(tuple(ref.shape), gpu, seed=5, dtype=torch.float32)
    ref = ref + res
    xp = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.float16, device=gpu)
    ops.pad_cast(x.permute(0, 2, 3, 1).contiguous(), xp)
    assert float(xp[:, 0].abs().max()) == 0 and float(xp[:, :, -1].abs().max()) == 0
    out = torch.empty(B, ref.shape[2], ref.shape[3], Cout, dtype=torch.float32, device=gpu)
    M = B * ref.shape[2] * ref.shape[3]
    ws = torch.empty(max(16, ops.gemm_workspace_bytes(M, Cout, split)), dtype=torch.uint8, device=gpu)
    ops.conv3x3(xp, w.permute(0, 2, 3, 1).contiguous(), out, stride=stride, upsample2x=ups, bias=bias, rowbias=rb,
                res1=res.permute(0, 2, 3, 1).contiguous(), split_k=split, workspace=ws, x_padded=True)
    check(out.permute(0, 3, 1, 2), ref, "conv3x3 padded", l2=2e-6, mx=2e-5)


@pytest.mark.parametrize("B,Bk,Nq,Nk", [(2, 2, 256, 320), (1, 1, 200, 77), (3, 2, 1024, 3000), (2, 2, 4096, 4096), (1, 1, 96, 1)])
def test_attention_fp8_d40(gpu, B, Bk, Nq, Nk):
    """sg_attn_f8_pack + sg_attn_fwd_f8_d40 (e4m3 Q / K / V / P, fp32 softmax; BASELINE config 5's attention path) against the
    fp32 softmax reference on the same fp16 operands, and against the fp16 kernel.  Stated bound: e4m3 keeps 3 mantissa bits
    (relative rounding error up to 2^-4 per element), which leaves 2-4e-2 rel-L2 on the attention output for unit-variance
    operands (measured 5.0-5.6e-2) — 8e-2 is asserted; the fp16 kernel sits at ~3e-4 on the same inputs.  Also: shared K/V batches (kv_batches < B),
    ragged key tails, a single key."""
    from storygen_amd import ops
    H, D = 8, 40
    C = H * D
    q, k, v = rnd((B, Nq, C), gpu, 1.0, 1), rnd((Bk, Nk, C), gpu, 1.0, 2), rnd((Bk, Nk, C), gpu, 1.0, 3)
    vt = _vt(v)
    scale = D ** -0.5
    kmap = [b if b < Bk else b - (B - Bk) for b in range(B)]
    qh = q.float().view(B, Nq, H, D).permute(0, 2, 1, 3)
    kh = k.float().view(Bk, Nk, H, D).permute(0, 2, 1, 3)[kmap]
    vh = v.float().view(Bk, Nk, H, D).permute(0, 2, 1, 3)[kmap]
    ref = (torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1) @ vh).permute(0, 2, 1, 3).reshape(B, Nq, C)
    nbytes = (ops.attention_f8_bytes(B, H, Nq, False) + ops.attention_f8_bytes(Bk, H, Nk, False) + ops.attention_f8_bytes(Bk, H, Nk, True) + 4096)
    scratch = torch.full((nbytes,), 0x7F, dtype=torch.uint8, device=gpu)          # 0x7F = NaN in e4m3: padding must not leak
    out8 = torch.full((B, Nq, C), float("nan"), dtype=torch.float16, device=gpu)
    ops.attention_f8(q, k, vt, out8, H, scale, scratch)
    out16 = torch.empty_like(out8)
    ops.attention(q, k, vt, out16, H, scale)
    torch.cuda.synchronize()
    e8, e16 = rel_l2(out8.float(), ref), rel_l2(out16.float(), ref)
    print(f"fp8 attention rel-L2 {e8:.2e} (fp16 kernel {e16:.2e})")
    assert torch.isfinite(out8).all() and e16 < 2e-3 and e8 < 8e-2          # measured 2.7e-2 .. 5.6e-2 (round 2, MI355X)


@pytest.mark.parametrize("outlier", ["first-channel", "first-tile", "one-row"])
def test_groupnorm_merge_of_producer_statistics_with_an_outlier_entry(gpu, outlier):
    """the merge of the producers' per-(tile, channel) partials must not lose digits when the FIRST entry of a group — the
    one a single-pivot formula would centre everything on — is an outlier by ~1e3 standard deviations (a channel with a huge bias, a
    tile with a huge offset).  The two-level Chan merge of gn_apply_wide_kernel is compared with the self-contained statistics pass
    and with torch in fp64 on the channels that are NOT outliers."""
    from storygen_amd import ops
    B, H, W, C = 2, 32, 32, 320
    HW, M = H * W, B * H * W
    a, w = rnd((M, 320), gpu, 1.0, 1), rnd((C, 320), gpu, 320 ** -0.5, 2)
    bias = torch.zeros(C, dtype=torch.float16, device=gpu)
    res = torch.zeros(M, C, dtype=torch.float32, device=gpu)
    if outlier == "first-channel":
        bias[0::10] = 1000.0                         # the first channel of every 10-channel group
    elif outlier == "first-tile":
        res.view(B, HW, C)[:, :64] += 1000.0         # the first row tile of every image, all channels
    else:
        res.view(B, HW, C)[:, 5, 0::10] = 30000.0    # one pixel of the first channel (not pixel 0: that one is the pivot of the
                                                     # kernel's OWN statistics pass, which is not the subject here)
    y = torch.empty(M, C, dtype=torch.float32, device=gpu)
    st = torch.zeros(M // 64 * 2 * C, dtype=torch.float32, device=gpu)
    ws = torch.empty(16 << 20, dtype=torch.uint8, device=gpu)
    rows = ops.gemm_stats_rows(a, w, y, bias=bias, res1=res, stats=(st, HW), workspace=ws)
    assert rows > 0
    ops.gemm(a, w, y, bias=bias, res1=res, stats=(st, HW), workspace=ws)
    gamma, beta = rnd((C,), gpu, 0.2, 3) + 1.0, rnd((C,), gpu, 0.2, 4)
    wsg = torch.empty(ops.groupnorm_workspace_bytes(B, 32), dtype=torch.uint8, device=gpu)
    outs = []
    for pst in ([(st, rows, C)], None):
        o = torch.full((B, HW, C), float("nan"), dtype=torch.float16, device=gpu)
        ops.groupnorm(y.view(B, HW, C), gamma, beta, o, 32, 1e-5, False, wsg, pstats=pst)
        outs.append(o.float().cpu())
    want = F.group_norm(y.view(B, HW, C).permute(0, 2, 1).double().cpu(), 32, gamma.double().cpu(), beta.double().cpu(), 1e-5).permute(0, 2, 1)
    for o, what in zip(outs, ("producer statistics", "own statistics pass")):
        err = (o.double() - want).abs().max() / want.abs().max()
        assert float(err) < 2e-3, f"{what}: max error {float(err):.2e} of the output range"
    assert float((outs[0] - outs[1]).abs().max()) <= 2e-3 * float(want.abs().max())


@pytest.mark.parametrize("B,H,W,C1,C2", [(3, 64, 64, 320, 320), (2, 32, 32, 640, 320), (2, 32, 32, 320, 640)])
def test_groupnorm_statistics_from_producer_epilogues(gpu, B, H, W, C1, C2):
    """North-star: GroupNorm as an epilogue.  (i) a conv3x3 and a GEMM write per-(row tile, channel) sums of their final outputs
    (bias / row bias / residual included) — checked against torch column sums; (ii) sg_groupnorm_nhwc_f16 fed with those
    partials (one source, and two sources for a channel concat [conv output | GEMM output]) matches torch's GroupNorm+SiLU like the
    self-contained kernel does; (iii) a launch that cannot emit statistics (split-K) reports 0 rows and refuses them."""
    from storygen_amd import ops
    HW, M = H * W, B * H * W
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=gpu)
    # producer 1: conv3x3 (+ bias, temb row bias, fp32 residual) -> fp32 [M, C1]
    xp = torch.zeros(B, H + 2, W + 2, 64, dtype=torch.float16, device=gpu)
    xp[:, 1:-1, 1:-1] = rnd((B, H, W, 64), gpu, 1.0, 1)
    wk, bias, rb = rnd((C1, 3, 3, 64), gpu, 0.05, 2), rnd((C1,), gpu, 1.0, 3), rnd((B, C1), gpu, 1.0, 4, torch.float32)
    res = rnd((B, H, W, C1), gpu, 1.0, 5, torch.float32) + 2.0                     # a large mean: the cancellation case
    cat = torch.empty(M, C1 + C2, dtype=torch.float32, device=gpu)               # [conv output | GEMM output]
    y1 = cat[:, :C1]
    st1 = torch.full((M // 64 * 2 * C1,), float("nan"), dtype=torch.float32, device=gpu)
    kw1 = dict(bias=bias, rowbias=rb, res1=res, workspace=ws, x_padded=True)
    rows1 = ops.conv3x3_stats_rows(xp, wk, y1.view(B, H, W, C1), stats=st1, **kw1)
    assert rows1 in (64, 128, 256)
    ops.conv3x3(xp, wk, y1.view(B, H, W, C1), stats=st1, **kw1)
    # producer 2: GEMM (+ bias, fp32 residual) -> fp32 [M, C2]
    a, w2 = rnd((M, 320), gpu, 1.0, 6), rnd((C2, 320), gpu, 320 ** -0.5, 7)
    y2 = cat[:, C1:]
    st2 = torch.full((M // 64 * 2 * C2,), float("nan"), dtype=torch.float32, device=gpu)
    kw2 = dict(bias=rnd((C2,), gpu, 1.0, 8), res1=rnd((M, C2), gpu, 1.0, 9, torch.float32), workspace=ws)
    rows2 = ops.gemm_stats_rows(a, w2, y2, stats=(st2, HW), **kw2)
    assert rows2 in (64, 128, 256)
    ops.gemm(a, w2, y2, stats=(st2, HW), **kw2)
    torch.cuda.synchronize()
    for y, st, rows, C in ((y1, st1, rows1, C1), (y2, st2, rows2, C2)):
        got = st[: M // rows * 2 * C].view(M // rows, 2, C)
        tiles = y.reshape(M // rows, rows, C).double()
        assert rel_l2(got[:, 0].double(), tiles.sum(1)) < 1e-6 and rel_l2(got[:, 1].double(), (tiles * tiles).sum(1)) < 1e-6
    # consumers
    wsg = torch.empty(ops.groupnorm_workspace_bytes(B, 32), dtype=torch.uint8, device=gpu)
    for x, pst in ((y1, [(st1, rows1, C1)]), (cat, [(st1, rows1, C1), (st2, rows2, C2)])):
        C = x.shape[1]
        assert ops.groupnorm_uses_pstats(HW, C, 32)
        gamma, beta = rnd((C,), gpu, 1.0, 10) + 1.0, rnd((C,), gpu, 1.0, 11)
        xc = x.contiguous()
        want = F.silu(F.group_norm(xc.view(B, HW, C).permute(0, 2, 1).float(), 32, gamma.float(), beta.float(), 1e-5)).permute(0, 2, 1)
        outs = []
        for p in (pst, None):
            o = torch.full((B, HW, C), float("nan"), dtype=torch.float16, device=gpu)
            ops.groupnorm(x.view(B, HW, C), gamma, beta, o, 32, 1e-5, True, wsg, pstats=p)
            outs.append(o)
        check(outs[0], want, "groupnorm from epilogue statistics")
        check(outs[1], want, "groupnorm, own statistics")
        assert rel_l2(outs[0].float(), outs[1].float()) < 3e-4
    # a launch that cannot emit statistics says so and refuses them: split-K needs N % 64 == 0 (its second pass works on 64-column blocks)
    a3, w3 = rnd((768, 5120), gpu, 1.0, 12), rnd((72, 5120), gpu, 0.01, 13)
    o3, st3 = torch.empty(768, 72, dtype=torch.float32, device=gpu), torch.zeros(768 // 64 * 2 * 72, dtype=torch.float32, device=gpu)
    assert ops.gemm_stats_rows(a3, w3, o3, stats=(st3, 256), split_k=4, workspace=ws) == 0
    with pytest.raises(RuntimeError, match="statistics"):
        ops.gemm(a3, w3, o3, stats=(st3, 256), split_k=4, workspace=ws)


@pytest.mark.parametrize("B,H,W,C1,C2,split", [(2, 32, 32, 640, 640, 3), (3, 16, 16, 1280, 1280, 5), (4, 16, 16, 1280, 640, 2),
                                               (1, 64, 64, 320, 320, 2)])
def test_groupnorm_statistics_from_the_split_k_second_pass(gpu, B, H, W, C1, C2, split):
    """Round 3: a split-K conv / GEMM emits the GroupNorm partials from its reduction pass
    (splitk_reduce_stats_kernel), so the 32x32 / 16x16 levels stop paying a statistics launch.  (i) the outputs are bit-identical to
    the plain second pass; (ii) the partials equal torch's per-tile column sums; (iii) GroupNorm fed with them (one source and the
    [conv | GEMM] channel concat) matches torch and the self-contained statistics."""
    from storygen_amd import ops
    HW, M = H * W, B * H * W
    ws = torch.empty(128 << 20, dtype=torch.uint8, device=gpu)
    xp = torch.zeros(B, H + 2, W + 2, 128, dtype=torch.float16, device=gpu)
    xp[:, 1:-1, 1:-1] = rnd((B, H, W, 128), gpu, 1.0, 1)
    wk, bias, rb = rnd((C1, 3, 3, 128), gpu, 0.04, 2), rnd((C1,), gpu, 1.0, 3), rnd((B, C1), gpu, 1.0, 4, torch.float32)
    res = rnd((B, H, W, C1), gpu, 1.0, 5, torch.float32) + 2.0
    cat = torch.empty(M, C1 + C2, dtype=torch.float32, device=gpu)
    y1, y2 = cat[:, :C1], cat[:, C1:]
    st1 = torch.full((M // 64 * 2 * C1,), float("nan"), dtype=torch.float32, device=gpu)
    kw1 = dict(bias=bias, rowbias=rb, res1=res, workspace=ws, x_padded=True, split_k=split)
    rows1 = ops.conv3x3_stats_rows(xp, wk, y1.view(B, H, W, C1), stats=st1, **kw1)
    assert rows1 in (64, 128, 256) and HW % rows1 == 0
    ops.conv3x3(xp, wk, y1.view(B, H, W, C1), stats=st1, **kw1)
    plain1 = torch.empty(M, C1, dtype=torch.float32, device=gpu)
    ops.conv3x3(xp, wk, plain1.view(B, H, W, C1), **kw1)
    a, w2 = rnd((M, 1280), gpu, 1.0, 6), rnd((C2, 1280), gpu, 1280 ** -0.5, 7)
    st2 = torch.full((M // 64 * 2 * C2,), float("nan"), dtype=torch.float32, device=gpu)
    kw2 = dict(bias=rnd((C2,), gpu, 1.0, 8), res1=rnd((M, C2), gpu, 1.0, 9, torch.float32), workspace=ws, split_k=split)
    rows2 = ops.gemm_stats_rows(a, w2, y2, stats=(st2, HW), **kw2)
    assert rows2 in (64, 128, 256) and HW % rows2 == 0
    ops.gemm(a, w2, y2, stats=(st2, HW), **kw2)
    plain2 = torch.empty(M, C2, dtype=torch.float32, device=gpu)
    ops.gemm(a, w2, plain2, **kw2)
    torch.cuda.synchronize()
    assert torch.equal(y1, plain1) and torch.equal(y2, plain2)
    for y, st, rows, C in ((y1, st1, rows1, C1), (y2, st2, rows2, C2)):
        got = st[: M // rows * 2 * C].view(M // rows, 2, C)
        tiles = y.reshape(M // rows, rows, C).double()
        assert rel_l2(got[:, 0].double(), tiles.sum(1)) < 1e-6 and rel_l2(got[:, 1].double(), (tiles * tiles).sum(1)) < 1e-6
    wsg = torch.empty(ops.groupnorm_workspace_bytes(B, 32), dtype=torch.uint8, device=gpu)
    for x, pst in ((y1, [(st1, rows1, C1)]), (cat, [(st1, rows1, C1), (st2, rows2, C2)])):
        C = x.shape[1]
        if not ops.groupnorm_uses_pstats(HW, C, 32):
            continue                                    # e.g. 16x16 x 1280: the one-launch kernel has its own statistics
        gamma, beta = rnd((C,), gpu, 1.0, 10) + 1.0, rnd((C,), gpu, 1.0, 11)
        xc = x.contiguous()
        want = F.silu(F.group_norm(xc.view(B, HW, C).permute(0, 2, 1).float(), 32, gamma.float(), beta.float(), 1e-5)).permute(0, 2, 1)
        outs = []
        for p in (pst, None):
            o = torch.full((B, HW, C), float("nan"), dtype=torch.float16, device=gpu)
            ops.groupnorm(x.view(B, HW, C), gamma, beta, o, 32, 1e-5, True, wsg, pstats=p)
            outs.append(o)
        check(outs[0], want, "groupnorm from second-pass statistics")
        assert rel_l2(outs[0].float(), outs[1].float()) < 3e-4


@pytest.mark.parametrize("B,H,W,Cin,C,split,out_f32,use_res", [(3, 8, 8, 1280, 1280, 6, False, False), (4, 16, 16, 640, 1280, 4, True, True),
                                                                (2, 16, 16, 128, 640, 3, False, True), (3, 8, 8, 256, 2560, 2, True, True)])
def test_groupnorm_sums_the_k_slices_of_a_deferred_split_k_convolution(gpu, B, H, W, Cin, C, split, out_f32, use_res):
    """Round 4: sg_conv3x3_desc.defer_reduce + sg_groupnorm_desc.split_*.  A split-K convolution stops after its
    partial tiles; the one-launch GroupNorm sums them in slice order with bias / temb row / residual while it loads its slab.  Both
    the normalised output and the (optionally stored) reduced tensor are BIT-IDENTICAL to reduce-then-normalise."""
    from storygen_amd import ops
    HW, M = H * W, B * H * W
    assert ops.groupnorm_is_fused(HW, C, 32)
    ws = torch.empty(128 << 20, dtype=torch.uint8, device=gpu)
    xp = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.float16, device=gpu)
    xp[:, 1:-1, 1:-1] = rnd((B, H, W, Cin), gpu, 1.0, 1)
    wk, bias, rb = rnd((C, 3, 3, Cin), gpu, (9 * Cin) ** -0.5, 2), rnd((C,), gpu, 1.0, 3), rnd((B, 2 * C), gpu, 1.0, 4, torch.float32)[:, C // 2: C // 2 + C]
    res = (rnd((B, H, W, C), gpu, 1.0, 5, torch.float32) + 2.0) if use_res else None
    gamma, beta = rnd((C,), gpu, 1.0, 6) + 1.0, rnd((C,), gpu, 1.0, 7)
    wsg = torch.empty(ops.groupnorm_workspace_bytes(B, 32), dtype=torch.uint8, device=gpu)
    odt = torch.float32 if out_f32 else torch.float16
    kw = dict(bias=bias, rowbias=rb, res1=res, workspace=ws, x_padded=True, split_k=split)
    # reference order: convolution with its own second pass, then GroupNorm of the stored tensor
    y_ref = torch.full((B, H, W, C), float("nan"), dtype=odt, device=gpu)
    ops.conv3x3(xp, wk, y_ref, **kw)
    n_ref = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float16, device=gpu)
    ops.groupnorm(y_ref.view(B, HW, C), gamma, beta, n_ref, 32, 1e-5, True, wsg)
    assert ops.conv3x3_planned_splits(xp, wk, y_ref, **kw) == split
    for store in (True, False):
        y = torch.full((B, H, W, C), float("nan"), dtype=odt, device=gpu)
        n = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float16, device=gpu)
        ops.conv3x3(xp, wk, y, defer_reduce=True, **kw)
        ops.groupnorm(y.view(B, HW, C), gamma, beta, n, 32, 1e-5, True, wsg,
                      split=dict(ws=ws, splits=split, bias=bias, rowbias=rb, res1=None if res is None else res.view(B, HW, C), store=store))
        torch.cuda.synchronize()
        assert torch.equal(n, n_ref), f"normalised output differs (store={store})"
        if store:
            assert torch.equal(y, y_ref), "reduced tensor differs"
        else:
            assert torch.isnan(y.float()).all(), "the reduced tensor must not be written without store"
    want = F.silu(F.group_norm(y_ref.view(B, HW, C).permute(0, 2, 1).float(), 32, gamma.float(), beta.float(), 1e-5)).permute(0, 2, 1)
    check(n[:, 1:-1, 1:-1].reshape(B, HW, C), want, "groupnorm over deferred split-K slices")
    # a launch that does not split cannot defer
    with pytest.raises(RuntimeError):
        ops.conv3x3(xp, wk, y_ref, defer_reduce=True, **dict(kw, split_k=1))


@pytest.mark.parametrize("tile", [(128, 128), (256, 64)])
def test_two_stage_ring_computes_the_same_values(gpu, tile):
    """Development option pipe_stages = 2 (round 4): the 128x128 and 256x64 tiles on a 2-stage LDS ring (74 / 80 KB: two workgroups
    per CU) — same slabs, same MFMA order, so GEMM (1, 2, odd slab counts, split-K) and convolution outputs are bit-identical."""
    from storygen_amd import ops
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=gpu)

    def run_all():
        outs = []
        for M, N, K, split in [(1024, 320, 64, 1), (4096, 320, 320, 1), (768, 1280, 1280, 4), (300, 640, 2560, 0), (640, 256, 128, 1)]:
            a, w = rnd((M, K), gpu, 1.0, 1), rnd((N, K), gpu, K ** -0.5, 2)
            o = torch.full((M, N), float("nan"), dtype=torch.float32, device=gpu)
            ops.gemm(a, w, o, bias=rnd((N,), gpu, 1.0, 3), res1=rnd((M, N), gpu, 1.0, 4, torch.float32), split_k=split, workspace=ws, tile=tile)
            outs.append(o)
        xp = torch.zeros(2, 34, 34, 320, dtype=torch.float16, device=gpu)
        xp[:, 1:-1, 1:-1] = rnd((2, 32, 32, 320), gpu, 1.0, 5)
        o = torch.full((2, 32, 32, 320), float("nan"), dtype=torch.float32, device=gpu)
        ops.conv3x3(xp, rnd((320, 3, 3, 320), gpu, 0.02, 6), o, bias=rnd((320,), gpu, 1.0, 7), workspace=ws, x_padded=True, tile=tile)
        outs.append(o)
        torch.cuda.synchronize()
        return outs
    ref = run_all()
    try:
        ops.debug_set_option("pipe_stages", 2)
        two = run_all()
    finally:
        ops.debug_set_option("pipe_stages", 3)
    for a, b in zip(ref, two):
        assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("tile", [(256, 128), (256, 64), (128, 128), (128, 64), (64, 128), (64, 64), (64, 64, 4)])
def test_register_epilogue_every_tile_every_mode(gpu, tile):
    """The round-3 epilogue (transposed accumulators + half-wave register swap, residual requested under the last K slab, no LDS
    staging) on every tile shape against fp32 references: GEMM with bias + fp32 residual (1, 5 and odd slab counts, ragged M and N),
    GEGLU, split-K partial tiles, 3x3 convolution incl. stride 2 and the upsampled gather, epilogue statistics."""
    from storygen_amd import ops
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=gpu)

    def run_all():
        outs = []
        for M, N, K, split in [(4096, 320, 320, 1), (768, 1280, 1280, 4), (300, 640, 2560, 0), (512, 256, 64, 1), (1024, 1280, 704, 1)]:
            a, w = rnd((M, K), gpu, 1.0, 1), rnd((N, K), gpu, K ** -0.5, 2)
            o = torch.full((M, N), float("nan"), dtype=torch.float32, device=gpu)
            ops.gemm(a, w, o, bias=rnd((N,), gpu, 1.0, 3), res1=rnd((M, N), gpu, 1.0, 4, torch.float32), split_k=split, workspace=ws, tile=tile)
            outs.append((o, a.float() @ w.float().t() + rnd((N,), gpu, 1.0, 3).float() + rnd((M, N), gpu, 1.0, 4, torch.float32)))
        a, w = rnd((1024, 640), gpu, 1.0, 5), rnd((5120, 640), gpu, 640 ** -0.5, 6)
        o = torch.full((1024, 2560), float("nan"), dtype=torch.float16, device=gpu)
        ops.gemm(a, w, o, bias=rnd((5120,), gpu, 1.0, 7), epilogue=ops.EPI_GEGLU, workspace=ws, tile=tile)
        wv, wg = w.view(-1, 2, 32, 640)[:, 0].reshape(-1, 640).float(), w.view(-1, 2, 32, 640)[:, 1].reshape(-1, 640).float()
        bfull = rnd((5120,), gpu, 1.0, 7).float().view(-1, 2, 32)
        outs.append((o, (a.float() @ wv.t() + bfull[:, 0].reshape(-1)) * F.gelu(a.float() @ wg.t() + bfull[:, 1].reshape(-1))))
        for B, H, W, Ci, Co, stride, ups in [(2, 32, 32, 320, 320, 1, False), (2, 16, 16, 640, 128, 2, False), (1, 16, 16, 128, 192, 1, True)]:
            x = rnd((B, Ci, H, W), gpu, 1.0, 8)
            xp = torch.zeros(B, H + 2, W + 2, Ci, dtype=torch.float16, device=gpu)
            xp[:, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
            wk = rnd((Co, Ci, 3, 3), gpu, (9 * Ci) ** -0.5, 9)
            xin = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if ups else x.float()
            ref = F.conv2d(xin, wk.float(), rnd((Co,), gpu, 1.0, 10).float(), stride=stride, padding=1)
            o = torch.full((B, ref.shape[2], ref.shape[3], Co), float("nan"), dtype=torch.float32, device=gpu)
            ops.conv3x3(xp, wk.permute(0, 2, 3, 1).contiguous(), o, stride=stride, upsample2x=ups, bias=rnd((Co,), gpu, 1.0, 10),
                        workspace=ws, x_padded=True, tile=tile)
            outs.append((o, ref.permute(0, 2, 3, 1)))
        # epilogue statistics (half-wave butterfly + LDS across the wave rows)
        a, w = rnd((4096, 320), gpu, 1.0, 11), rnd((320, 320), gpu, 320 ** -0.5, 12)
        o = torch.empty(4096, 320, dtype=torch.float32, device=gpu)
        st = torch.zeros(4096 // 64 * 2 * 320, dtype=torch.float32, device=gpu)
        rows = ops.gemm_stats_rows(a, w, o, stats=(st, 1024), workspace=ws, tile=tile)
        if rows:
            ops.gemm(a, w, o, stats=(st, 1024), workspace=ws, tile=tile)
            t = o.view(4096 // rows, rows, 320).double()
            got = st[: 4096 // rows * 2 * 320].view(4096 // rows, 2, 320).double()
            assert rel_l2(got[:, 0], t.sum(1)) < 1e-6 and rel_l2(got[:, 1], (t * t).sum(1)) < 1e-6
        torch.cuda.synchronize()
        return outs
    for o, ref in run_all():
        assert torch.isfinite(o.float()).all()
        if o.dtype == torch.float32:
            check(o, ref, "register epilogue vs fp32 reference", l2=2e-6, mx=2e-5)
        else:
            check(o, ref, "register epilogue (fp16 output) vs fp32 reference")


@pytest.mark.parametrize("stages,lat", [(0, (64, 64, 4)), (4, (64, 64, 4)), (8, (64, 64, 4)), (0, (64, 128, 8))])
def test_latency_kernel_every_mode(gpu, stages, lat):
    """The 32x32-per-wave deep-ring kernel (mma_lat_kernel, round 6: tile 64x64 = four waves, 4 / 8 LDS stages) on the shapes of the
    batch-3 main pass it serves, against fp32 references and against the 64x64-per-wave kernels on the same operands: every term of
    the linear epilogue at once, ragged M / N, 1 ... 80 K slabs (fewer than the ring is deep, not a multiple of it), split-K partial
    tiles — also on the 64x128-tile / eight-wave / 6-stage weight-streaming form of the 8x8 level (tile hint (64, 128, 8)) —, the LayerNorm fold on both sides (producer partials, rows-are-tokens and columns-are-tokens consumers), GroupNorm
    partials, paired launches, and the 3x3 convolution gather."""
    from storygen_amd import ops
    from storygen_amd.repack import fold_layernorm
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=gpu)
    try:
        ops.debug_set_option("lat_stages", stages)
        for M, N, K, split in [(768, 1280, 1280, 1), (3072, 640, 640, 1), (192, 1280, 2560, 0), (192, 1280, 1280, 3), (300, 200, 64, 1),
                               (1000, 72, 448, 1), (768, 1280, 5120, 1), (64, 64, 192, 1), (130, 1288, 576, 2)]:
            a, w = rnd((M, K), gpu, 1.0, 1), rnd((N, K), gpu, K ** -0.5, 2)
            bias, r1, r2 = rnd((N,), gpu, 1.0, 3), rnd((M, N), gpu, 1.0, 4, torch.float32), rnd((M, N), gpu, 1.0, 5)
            rpb = max(1, M // 3)
            rb = rnd((-(-M // rpb), N), gpu, 1.0, 6, torch.float32)
            ref = a.float() @ w.float().t() + bias.float() + r1 + r2.float() + rb.repeat_interleave(rpb, 0)[:M]
            o = torch.full((M, N), float("nan"), dtype=torch.float32, device=gpu)
            o16 = torch.full((M, N), float("nan"), dtype=torch.float16, device=gpu)
            ops.gemm(a, w, o, bias=bias, res1=r1, res2=r2, rowbias=rb, rows_per_batch=rpb, out2=o16, split_k=split, workspace=ws, tile=lat)
            check(o, ref, f"lat M{M} N{N} K{K} split {split}: fp32 out", l2=2e-6, mx=2e-5)
            check(o16, ref, "fp16 copy")
            ops.gemm(a, w, o16, bias=bias, res1=r2, split_k=split, workspace=ws, tile=lat)
            check(o16, a.float() @ w.float().t() + bias.float() + r2.float(), "fp16 out + fp16 residual")
            # (a2 + h) + (a3 + h): one tensor as both residuals
            ops.gemm(a, w, o, bias=bias, res1=r1, res2=r1, split_k=split, workspace=ws, tile=lat)
            check(o, a.float() @ w.float().t() + bias.float() + 2.0 * r1, "res1 == res2", l2=2e-6, mx=2e-5)
        # LayerNorm fold: producer (fp32 stream + raw copy + partials) -> consumers in both orientations, all on the latency kernel
        for M, C in [(768, 1280), (3072, 640), (200, 320)]:
            a0, w0 = rnd((M, C), gpu, 1.0, 1), rnd((C, C), gpu, C ** -0.5, 2)
            res = rnd((M, C), gpu, 1.0, 3, torch.float32) + 3.0
            x = torch.empty(M, C, dtype=torch.float32, device=gpu)
            x16 = torch.empty(M, C, dtype=torch.float16, device=gpu)
            st = torch.zeros(M, (C // 64 + 1) & ~1, 2, dtype=torch.float32, device=gpu)
            guard = torch.zeros(1, dtype=torch.int32, device=gpu)
            ops.gemm(a0, w0, x, res1=res, out2=x16, ln_out=st, guard=guard, tile=lat, workspace=ws)
            xr = a0.float() @ w0.float().t() + res
            check(x, xr, "producer stream", l2=2e-6, mx=2e-5)
            blk = xr.view(M, C // 64, 64).double()
            got = st[:, : C // 64].double()
            assert rel_l2(got[..., 0].cpu(), blk.sum(-1).cpu()) < 1e-5
            assert rel_l2(got[..., 1].cpu(), ((blk - blk.mean(-1, keepdim=True)) ** 2).sum(-1).cpu()) < 1e-4
            g, b = rnd((C,), gpu, 0.2, 7, torch.float32) + 1.0, rnd((C,), gpu, 0.1, 8, torch.float32)
            wq = rnd((2 * C, C), gpu, C ** -0.5, 9)
            wf, cq, dq = fold_layernorm(wq, None, g, b)
            y = torch.empty(M, 2 * C, dtype=torch.float16, device=gpu)
            ops.gemm(x16, wf, y, ln=(1, st, cq, dq, 1e-5), guard=guard, tile=lat)
            lnx = F.layer_norm(xr, (C,), g, b, 1e-5)
            check(y, lnx @ wq.float().t(), "folded consumer, rows are tokens", l2=1.5e-3, mx=2e-2)
            wv = rnd((C, C), gpu, C ** -0.5, 10)
            wvf, cv, dv = fold_layernorm(wv, None, g, b)
            yt = torch.empty(C, M, dtype=torch.float16, device=gpu)
            ops.gemm(wvf, x16, yt, ln=(2, st, cv, dv, 1e-5), guard=guard, tile=lat)
            check(yt, wv.float() @ lnx.t(), "folded consumer, columns are tokens", l2=1.5e-3, mx=2e-2)
            # the same two as one paired launch: bit-identical
            y2, yt2 = torch.empty_like(y), torch.empty_like(yt)
            ops.gemm_pair(((x16, wf, y2), dict(ln=(1, st, cq, dq, 1e-5), guard=guard, tile=lat)),
                          ((wvf, x16, yt2), dict(ln=(2, st, cv, dv, 1e-5), guard=guard)))
            assert torch.equal(y, y2) and torch.equal(yt, yt2)
            assert int(guard.item()) == 0
        # GroupNorm partials from the epilogue (one per 64-row tile)
        a, w = rnd((3072, 2560), gpu, 1.0, 11), rnd((640, 2560), gpu, 2560 ** -0.5, 12)
        o = torch.empty(3072, 640, dtype=torch.float32, device=gpu)
        stt = torch.zeros(3072 // 64 * 2 * 640, dtype=torch.float32, device=gpu)
        rows = ops.gemm_stats_rows(a, w, o, stats=(stt, 1024), workspace=ws, tile=lat)
        assert rows == 64
        ops.gemm(a, w, o, stats=(stt, 1024), workspace=ws, tile=lat)
        t = o.view(3072 // rows, rows, 640).double()
        got = stt.view(3072 // rows, 2, 640).double()
        assert rel_l2(got[:, 0].cpu(), t.sum(1).cpu()) < 1e-6 and rel_l2(got[:, 1].cpu(), (t * t).sum(1).cpu()) < 1e-6
        # 3x3 convolution on the same mainloop (implicit-GEMM gather, stride 2, nearest-2x upsample, split-K)
        for B, H, W, Ci, Co, stride, ups, split in [(3, 8, 8, 1280, 1280, 1, False, 0), (2, 16, 16, 640, 128, 2, False, 1), (1, 16, 16, 128, 192, 1, True, 1),
                                                     (3, 16, 16, 640, 200, 1, False, 2)]:
            xx = rnd((B, Ci, H, W), gpu, 1.0, 8)
            xp = torch.zeros(B, H + 2, W + 2, Ci, dtype=torch.float16, device=gpu)
            xp[:, 1:-1, 1:-1] = xx.permute(0, 2, 3, 1)
            wk = rnd((Co, Ci, 3, 3), gpu, (9 * Ci) ** -0.5, 9)
            xin = F.interpolate(xx.float(), scale_factor=2.0, mode="nearest") if ups else xx.float()
            ref = F.conv2d(xin, wk.float(), rnd((Co,), gpu, 1.0, 10).float(), stride=stride, padding=1)
            oc = torch.full((B, ref.shape[2], ref.shape[3], Co), float("nan"), dtype=torch.float32, device=gpu)
            ops.conv3x3(xp, wk.permute(0, 2, 3, 1).contiguous(), oc, stride=stride, upsample2x=ups, bias=rnd((Co,), gpu, 1.0, 10),
                        split_k=split, workspace=ws, x_padded=True, tile=lat)
            check(oc, ref.permute(0, 2, 3, 1), f"lat conv {B}x{H}x{W} {Ci}->{Co}", l2=2e-6, mx=2e-5)
        # automatic selection (no hint) against the 64x64-per-wave kernels: same sums in a different order
        a, w = rnd((768, 1280), gpu, 1.0, 13), rnd((1280, 1280), gpu, 1280 ** -0.5, 14)
        o1, o2 = torch.empty(768, 1280, dtype=torch.float32, device=gpu), torch.empty(768, 1280, dtype=torch.float32, device=gpu)
        ops.gemm(a, w, o1, workspace=ws, use_table=False)
        ops.debug_set_option("lat_tiles", 0)
        ops.gemm(a, w, o2, workspace=ws, use_table=False)
        check(o1, o2, "auto-selected latency kernel vs 64x64-per-wave kernel", l2=1e-6, mx=1e-5)
    finally:
        ops.debug_set_option("reset", 0)


@pytest.mark.parametrize("fat", [(512, 128, 8), (256, 256, 8)])
def test_fat_wave_kernel_every_mode(gpu, fat):
    """Eight waves of 128x64 on a 2-stage ring (mma_fat_kernel, round 6: tiles 512x128 / 256x256 by tile hint) against fp32 references:
    every term of the linear epilogue at once on ragged M / N and 1 ... 90 K slabs, GEGLU, GroupNorm partials (one per tile height),
    the LayerNorm fold on both sides, and the 3x3 convolution gather (stride 1, stride 2, nearest-2x) with the GroupNorm partials of a
    batch of images — plus the automatic selection for large convolutions (development option fat_m)."""
    from storygen_amd import ops
    from storygen_amd.repack import fold_layernorm
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=gpu)
    bm = fat[0]
    try:
        for M, N, K in [(2048, 640, 640), (1000, 328, 128), (5120, 1280, 64), (700, 200, 1280), (4096, 320, 5760)]:
            a, w = rnd((M, K), gpu, 1.0, 1), rnd((N, K), gpu, K ** -0.5, 2)
            bias, r1, r2 = rnd((N,), gpu, 1.0, 3), rnd((M, N), gpu, 1.0, 4, torch.float32), rnd((M, N), gpu, 1.0, 5)
            rpb = max(1, M // 3)
            rb = rnd((-(-M // rpb), N), gpu, 1.0, 6, torch.float32)
            ref = a.float() @ w.float().t() + bias.float() + r1 + r2.float() + rb.repeat_interleave(rpb, 0)[:M]
            o = torch.full((M, N), float("nan"), dtype=torch.float32, device=gpu)
            o16 = torch.full((M, N), float("nan"), dtype=torch.float16, device=gpu)
            ops.gemm(a, w, o, bias=bias, res1=r1, res2=r2, rowbias=rb, rows_per_batch=rpb, out2=o16, workspace=ws, tile=fat)
            check(o, ref, f"fat M{M} N{N} K{K}: fp32 out", l2=2e-6, mx=2e-5)
            check(o16, ref, "fp16 copy")
            ops.gemm(a, w, o16, bias=bias, res1=r2, tile=fat)
            check(o16, a.float() @ w.float().t() + bias.float() + r2.float(), "fp16 out + fp16 residual")
            ops.gemm(a, w, o, bias=bias, res1=r1, res2=r1, tile=fat)
            check(o, a.float() @ w.float().t() + bias.float() + 2.0 * r1, "res1 == res2", l2=2e-6, mx=2e-5)
        # the launch really is the 128x64-per-wave kernel
        d, _, _ = ops._gemm_desc(a, w, o, tile=fat)
        assert ops._plan_of(ops.lib.sg_gemm_launch_plan, d)[:2] == [fat[0], fat[1]] and ops._plan_of(ops.lib.sg_gemm_launch_plan, d)[5] == 2
        # GEGLU (interleaved weight rows) against the heuristic tile: the same products, the same epilogue arithmetic
        M, C = 2048, 320
        a, w = rnd((M, C), gpu, 1.0, 21), rnd((8 * C, C), gpu, C ** -0.5, 22)
        bias = rnd((8 * C,), gpu, 1.0, 23)
        g1, g2 = torch.empty(M, 4 * C, dtype=torch.float16, device=gpu), torch.empty(M, 4 * C, dtype=torch.float16, device=gpu)
        ops.gemm(a, w, g1, bias=bias, epilogue=ops.EPI_GEGLU, tile=fat)
        ops.gemm(a, w, g2, bias=bias, epilogue=ops.EPI_GEGLU, use_table=False)
        check(g1, g2.float(), "GEGLU on the fat tile vs the heuristic tile", l2=1e-3, mx=2e-2)
        # LayerNorm fold: producer partials and both consumer orientations
        M, C = 2048, 640
        a0, w0 = rnd((M, C), gpu, 1.0, 1), rnd((C, C), gpu, C ** -0.5, 2)
        res = rnd((M, C), gpu, 1.0, 3, torch.float32) + 3.0
        x, x16 = torch.empty(M, C, dtype=torch.float32, device=gpu), torch.empty(M, C, dtype=torch.float16, device=gpu)
        st = torch.zeros(M, (C // 64 + 1) & ~1, 2, dtype=torch.float32, device=gpu)
        guard = torch.zeros(1, dtype=torch.int32, device=gpu)
        ops.gemm(a0, w0, x, res1=res, out2=x16, ln_out=st, guard=guard, tile=fat)
        xr = a0.float() @ w0.float().t() + res
        check(x, xr, "producer stream", l2=2e-6, mx=2e-5)
        blk = xr.view(M, C // 64, 64).double()
        got = st[:, : C // 64].double()
        assert rel_l2(got[..., 0].cpu(), blk.sum(-1).cpu()) < 1e-5
        assert rel_l2(got[..., 1].cpu(), ((blk - blk.mean(-1, keepdim=True)) ** 2).sum(-1).cpu()) < 1e-4
        g, b = rnd((C,), gpu, 0.2, 7, torch.float32) + 1.0, rnd((C,), gpu, 0.1, 8, torch.float32)
        wq = rnd((2 * C, C), gpu, C ** -0.5, 9)
        wf, cq, dq = fold_layernorm(wq, None, g, b)
        y = torch.empty(M, 2 * C, dtype=torch.float16, device=gpu)
        ops.gemm(x16, wf, y, ln=(1, st, cq, dq, 1e-5), guard=guard, tile=fat)
        lnx = F.layer_norm(xr, (C,), g, b, 1e-5)
        check(y, lnx @ wq.float().t(), "folded consumer, rows are tokens", l2=1.5e-3, mx=2e-2)
        wv = rnd((C, C), gpu, C ** -0.5, 10)
        wvf, cv, dv = fold_layernorm(wv, None, g, b)
        yt = torch.empty(C, M, dtype=torch.float16, device=gpu)
        ops.gemm(wvf, x16, yt, ln=(2, st, cv, dv, 1e-5), guard=guard, tile=fat)
        check(yt, wv.float() @ lnx.t(), "folded consumer, columns are tokens", l2=1.5e-3, mx=2e-2)
        assert int(guard.item()) == 0
        # GroupNorm partials from the epilogue: one per tile height
        a, w = rnd((4096, 1280), gpu, 1.0, 11), rnd((640, 1280), gpu, 1280 ** -0.5, 12)
        o = torch.empty(4096, 640, dtype=torch.float32, device=gpu)
        stt = torch.zeros(4096 // bm * 2 * 640, dtype=torch.float32, device=gpu)
        rows = ops.gemm_stats_rows(a, w, o, stats=(stt, 1024), tile=fat)
        assert rows == bm
        ops.gemm(a, w, o, stats=(stt, 1024), tile=fat)
        t = o.view(4096 // rows, rows, 640).double()
        got = stt.view(4096 // rows, 2, 640).double()
        assert rel_l2(got[:, 0].cpu(), t.sum(1).cpu()) < 1e-6 and rel_l2(got[:, 1].cpu(), (t * t).sum(1).cpu()) < 1e-6
        # 3x3 convolution: bias + temb row + fp32 residual + GroupNorm partials; stride 2; nearest-2x
        for B, H, W, Ci, Co, stride, ups in [(4, 32, 32, 128, 320, 1, False), (2, 64, 64, 64, 128, 2, False), (2, 16, 16, 128, 256, 1, True),
                                             (3, 32, 16, 192, 200, 1, False)]:
            xx = rnd((B, Ci, H, W), gpu, 1.0, 8)
            xp = torch.zeros(B, H + 2, W + 2, Ci, dtype=torch.float16, device=gpu)
            xp[:, 1:-1, 1:-1] = xx.permute(0, 2, 3, 1)
            wk = rnd((Co, Ci, 3, 3), gpu, (9 * Ci) ** -0.5, 9)
            bias, rb = rnd((Co,), gpu, 1.0, 10), rnd((B, Co), gpu, 1.0, 11, torch.float32)
            xin = F.interpolate(xx.float(), scale_factor=2.0, mode="nearest") if ups else xx.float()
            ref = F.conv2d(xin, wk.float(), bias.float(), stride=stride, padding=1) + rb[:, :, None, None]
            Ho, Wo = ref.shape[2], ref.shape[3]
            res = rnd((B, Ho, Wo, Co), gpu, 1.0, 12, torch.float32)
            ref = ref.permute(0, 2, 3, 1) + res
            oc = torch.full((B, Ho, Wo, Co), float("nan"), dtype=torch.float32, device=gpu)
            kw = dict(stride=stride, upsample2x=ups, bias=bias, rowbias=rb, res1=res, x_padded=True, tile=fat)
            wkr = wk.permute(0, 2, 3, 1).contiguous()
            hw = Ho * Wo
            if hw % bm == 0 and Co % 64 == 0:
                stc = torch.zeros(B * hw // bm * 2 * Co, dtype=torch.float32, device=gpu)
                assert ops.conv3x3_stats_rows(xp, wkr, oc, stats=stc, **kw) == bm
                ops.conv3x3(xp, wkr, oc, stats=stc, **kw)
                t = oc.view(B * hw // bm, bm, Co).double()
                got = stc.view(B * hw // bm, 2, Co).double()
                assert rel_l2(got[:, 0].cpu(), t.sum(1).cpu()) < 1e-6 and rel_l2(got[:, 1].cpu(), (t * t).sum(1).cpu()) < 1e-6
            else:
                ops.conv3x3(xp, wkr, oc, **kw)
            check(oc, ref, f"fat conv {B}x{H}x{W} {Ci}->{Co} stride {stride} ups {ups}", l2=2e-6, mx=2e-5)
        # automatic selection (development option fat_m): the same values as the heuristic tile up to summation order
        xx = rnd((8, 64, 32, 32), gpu, 1.0, 31)
        xp = torch.zeros(8, 34, 34, 64, dtype=torch.float16, device=gpu)
        xp[:, 1:-1, 1:-1] = xx.permute(0, 2, 3, 1)
        wkr = rnd((640, 3, 3, 64), gpu, (9 * 64) ** -0.5, 32)
        o1, o2 = (torch.empty(8, 32, 32, 640, dtype=torch.float32, device=gpu) for _ in range(2))
        ops.conv3x3(xp, wkr, o1, x_padded=True)
        ops.debug_set_option("fat_m", 4096)
        d, _, _ = ops._conv_desc(xp, wkr, o2, x_padded=True)
        assert ops._plan_of(ops.lib.sg_conv3x3_launch_plan, d)[5] == 2
        ops.conv3x3(xp, wkr, o2, x_padded=True)
        check(o2, o1, "automatically selected fat tile vs heuristic tile", l2=1e-6, mx=1e-5)
    finally:
        ops.debug_set_option("reset", 0)


PATCH_CASES = [
    # B, H, W, Cin, Cout, split, tile
    (3, 64, 64, 320, 320, 0, None), (3, 64, 64, 320, 320, 1, (256, 128)), (2, 64, 64, 128, 64, 1, (128, 64)), (1, 64, 64, 64, 72, 1, (64, 64)),
    (2, 32, 32, 640, 320, 0, None), (2, 32, 32, 192, 128, 3, (256, 64)), (4, 16, 16, 1280, 640, 0, None), (2, 16, 16, 256, 136, 2, (128, 128)),
    (3, 8, 8, 1280, 1280, 0, None), (2, 8, 8, 320, 64, 5, (64, 128)), (1, 32, 16, 128, 128, 1, (64, 64)), (2, 16, 32, 64, 64, 1, (128, 128)),
]


@pytest.mark.parametrize("B,H,W,Cin,Cout,split,tile", PATCH_CASES)
def test_conv3x3_every_epilogue_term(gpu, B, H, W, Cin, Cout, split, tile):
    """3x3 convolution with bias + temb row-bias + fp32 residual at once against the fp32 reference: every tile shape, split-K,
    non-square images, Cout not a multiple of the tile."""
    from storygen_amd import ops
    x = rnd((B, Cin, H, W), gpu, seed=1)
    w = rnd((Cout, Cin, 3, 3), gpu, 1 / math.sqrt(9 * Cin), seed=2)
    bias, rb = rnd((Cout,), gpu, seed=3), rnd((B, Cout), gpu, seed=4, dtype=torch.float32)
    res = rnd((B, Cout, H, W), gpu, seed=5, dtype=torch.float32)
    ref = F.conv2d(x.float(), w.float(), bias.float(), padding=1) + rb[:, :, None, None] + res
    xp = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.float16, device=gpu)
    ops.pad_cast(x.permute(0, 2, 3, 1).contiguous(), xp)
    wk, resn = w.permute(0, 2, 3, 1).contiguous(), res.permute(0, 2, 3, 1).contiguous()
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=gpu)
    out = torch.full((B, H, W, Cout), float("nan"), dtype=torch.float32, device=gpu)
    ops.conv3x3(xp, wk, out, bias=bias, rowbias=rb, res1=resn, split_k=split, workspace=ws, x_padded=True, tile=tile)
    check(out.permute(0, 3, 1, 2), ref, "conv3x3, all epilogue terms", l2=2e-6, mx=2e-5)


def _vt(v):
    """[B, Nk, C] -> the kernel's V^T operand [B, C, Nk rounded up to 8] (zero padding, as the engine's GEMM produces)."""
    B, Nk, C = v.shape
    vt = torch.zeros(B, C, (Nk + 7) & ~7, dtype=v.dtype, device=v.device)
    vt[:, :, :Nk] = v.transpose(1, 2)
    return vt


ATTN_CASES = [
    # B, H, Nq, Nk, D
    (2, 8, 256, 256, 40), (1, 8, 200, 77, 40), (3, 8, 64, 192, 160), (2, 8, 256, 768, 80), (1, 8, 1024, 1024, 80),
    (1, 2, 130, 65, 160), (3, 8, 4096, 77, 40), (1, 8, 1024, 3072, 40), (1, 4, 33, 1, 80),
    (2, 8, 4096, 705, 40), (2, 8, 4096, 320, 40),      # big grids: the 4-wave kernels, ragged last tile / odd tile count
    # D = 160 at Nq <= 256: the key-split workgroups (round 5) — 12 / 4 / 2 tiles for 4 waves, ragged queries and keys; (20, 8, 256, 256) has
    # 1 280 workgroups of 32 queries, more than the 256 the key split is chosen for, and (2, 8, 64, 64) a single tile: both run the query-split kernel
    (3, 8, 256, 768, 160), (3, 8, 256, 256, 160), (3, 8, 256, 77, 160), (1, 8, 250, 330, 160), (20, 8, 256, 256, 160), (2, 8, 64, 64, 160),
]


@pytest.mark.parametrize("B,H,Nq,Nk,D", ATTN_CASES)
def test_attention(gpu, B, H, Nq, Nk, D):
    from storygen_amd import ops
    C = H * D
    # q/k/v as column slices of fused projection buffers, like the engine lays them out
    qkv = rnd((B, Nq, 3 * C), gpu, 1.5, seed=1)
    kv = rnd((B, Nk, 2 * C), gpu, 1.5, seed=2)
    q, k, v = qkv[:, :, :C], kv[:, :, :C], kv[:, :, C:]
    scale = D ** -0.5
    out = torch.empty(B, Nq, C, dtype=torch.float16, device=gpu)
    ops.attention(q, k, _vt(v), out, H, scale, nk=Nk)

    def heads(t):
        return t.float().view(t.shape[0], t.shape[1], H, D).transpose(1, 2)
    att = torch.softmax(heads(q) @ heads(k).transpose(-1, -2) * scale, dim=-1) @ heads(v)
    ref = att.transpose(1, 2).reshape(B, Nq, C)
    check(out, ref, "attention")


def test_attention_online_softmax_rescale(gpu):
    """Forces the running-max rescale: one key in a *late* tile dominates one query row (guide §5.4 rule 26)."""
    from storygen_amd import ops
    B, H, Nq, Nk, D = 1, 8, 128, 512, 40
    C = H * D
    q, k, v = rnd((B, Nq, C), gpu, seed=1), rnd((B, Nk, C), gpu, seed=2), rnd((B, Nk, C), gpu, seed=3)
    k[0, 300] = q[0, 5] * 6.0          # spike: raw q.k is ~40 * 6 vs O(6) elsewhere
    k[0, 450] = q[0, 77] * 8.0
    out = torch.empty(B, Nq, C, dtype=torch.float16, device=gpu)
    ops.attention(q, k, _vt(v), out, H, D ** -0.5)

    def heads(t):
        return t.float().view(B, -1, H, D).transpose(1, 2)
    ref = (torch.softmax(heads(q) @ heads(k).transpose(-1, -2) * D ** -0.5, -1) @ heads(v)).transpose(1, 2).reshape(B, Nq, C)
    check(out, ref, "attention rescale")


def test_attention_deferred_rescale_threshold(gpu):
    """Row maxima that creep up by less than the rescale threshold per tile (so the kernel keeps a stale running max
    and P exceeds 1) and then jump far above it."""
    from storygen_amd import ops
    B, H, Nq, Nk, D = 1, 8, 64, 640, 40
    C = H * D
    q, k, v = rnd((B, Nq, C), gpu, seed=4), rnd((B, Nk, C), gpu, 0.2, seed=5), rnd((B, Nk, C), gpu, seed=6)
    qh = q.view(B, Nq, H, D)
    for tile in range(1, 10):                   # key tile*64 + 3 aligned with query 7: score grows ~ +2.5 log2 units per tile
        k.view(B, Nk, H, D)[0, tile * 64 + 3] = qh[0, 7] * (0.28 * tile)
    out = torch.empty(B, Nq, C, dtype=torch.float16, device=gpu)
    ops.attention(q, k, _vt(v), out, H, D ** -0.5)

    def heads(t):
        return t.float().view(B, -1, H, D).transpose(1, 2)
    ref = (torch.softmax(heads(q) @ heads(k).transpose(-1, -2) * D ** -0.5, -1) @ heads(v)).transpose(1, 2).reshape(B, Nq, C)
    check(out, ref, "attention deferred rescale")


def test_attention_key_split_d160_rescale_and_variants(gpu):
    """The key-split D = 160 kernel (attn_fwd_ksplit_kernel: four waves on one 32-query block, each on every fourth 64-key tile, partial
    (max, sum, O^T) merged through LDS): row maxima that sit in DIFFERENT waves' tiles — a dominant key in a late tile of wave 2, another in
    wave 0's first tile, rows whose keys are all tiny in three of the four waves — against fp32 softmax, and against the query-split
    instantiation (option attn_d160 = 3) on the same operands."""
    from storygen_amd import ops
    B, H, Nq, Nk, D = 2, 8, 256, 768, 160
    C = H * D
    q, k, v = rnd((B, Nq, C), gpu, seed=1), rnd((B, Nk, C), gpu, 0.3, seed=2), rnd((B, Nk, C), gpu, seed=3)
    kh, qh = k.view(B, Nk, H, D), q.view(B, Nq, H, D)
    kh[0, 64 * 6 + 5] = qh[0, 9] * 2.0            # tile 6 -> wave 2: dominates query 9 of every head
    kh[0, 3] = qh[0, 40] * 2.5                    # tile 0 -> wave 0
    kh[1, 64 * 11 + 63] = qh[1, 255] * 3.0        # the very last key -> wave 3
    out = torch.empty(B, Nq, C, dtype=torch.float16, device=gpu)
    ops.attention(q, k, _vt(v), out, H, D ** -0.5)

    def heads(t):
        return t.float().view(B, -1, H, D).transpose(1, 2)
    ref = (torch.softmax(heads(q) @ heads(k).transpose(-1, -2) * D ** -0.5, -1) @ heads(v)).transpose(1, 2).reshape(B, Nq, C)
    check(out, ref, "key-split attention")
    ops.debug_set_option("attn_d160", 3)
    try:
        old = torch.empty_like(out)
        ops.attention(q, k, _vt(v), old, H, D ** -0.5)
    finally:
        ops.debug_set_option("attn_d160", 4)
    check(old, ref, "query-split attention")
    check(out, old, "key-split vs query-split", l2=6e-4, mx=2e-2)


@pytest.mark.parametrize("D,Nq,Nk", [(40, 4096, 640), (80, 200, 77), (160, 64, 192)])
def test_attention_shared_kv_batches(gpu, D, Nq, Nk):
    """Query batches [u/zero, u/img, t/img] over context rows [zero, img]: batch 2 reads K/V row 1 (kv_batches = 2)."""
    from storygen_amd import ops
    H = 8
    C = H * D
    q, k, v = rnd((3, Nq, C), gpu, 1.5, seed=1), rnd((2, Nk, C), gpu, 1.5, seed=2), rnd((2, Nk, C), gpu, seed=3)
    out = torch.empty(3, Nq, C, dtype=torch.float16, device=gpu)
    ops.attention(q, k, _vt(v), out, H, D ** -0.5, nk=Nk)
    idx = [0, 1, 1]

    def heads(t):
        return t.float().view(t.shape[0], t.shape[1], H, D).transpose(1, 2)
    att = torch.softmax(heads(q) @ heads(k[idx]).transpose(-1, -2) * D ** -0.5, dim=-1) @ heads(v[idx])
    check(out, att.transpose(1, 2).reshape(3, Nq, C), "attention shared kv")


@pytest.mark.parametrize("D,Nq,hw,R", [(40, 4096, 256, 3), (40, 320, 64, 5), (80, 1024, 128, 3), (160, 256, 72, 2)])
def test_attention_short_kv_rows(gpu, D, Nq, hw, R):
    """sg_attn_desc.k2 (round 4): query batches [u/zero, u/img, t/img] over K/V rows [zero (hw keys) | frames (R hw keys)] laid out
    back to back in ONE flat projection output, as the main pass lays them out — against torch on the same rows, and against the
    as-written form of the zero-image branch (R copies of its hw keys: softmax over R copies of the same keys is softmax over one)."""
    from storygen_amd import ops
    H = 8
    C = H * D
    T = hw + R * hw
    q = rnd((3, Nq, C), gpu, 1.5, seed=1)
    kflat, vflat = rnd((T, C), gpu, 1.5, seed=2), rnd((T, C), gpu, 1.0, seed=3)
    vt = vflat.t().contiguous()                                        # [C, T]
    k_s, k_l = kflat[:hw].view(1, hw, C), kflat[hw:].view(1, R * hw, C)
    vt_s = vt[:, :hw].unflatten(1, (1, hw)).permute(1, 0, 2)
    vt_l = vt[:, hw:].unflatten(1, (1, R * hw)).permute(1, 0, 2)
    out = torch.full((3, Nq, C), float("nan"), dtype=torch.float16, device=gpu)
    ops.attention(q, k_l, vt_l, out, H, D ** -0.5, short=(k_s, vt_s))

    def heads(t):
        return t.float().view(t.shape[0], t.shape[1], H, D).transpose(1, 2)

    def ref(qq, kk, vv):
        return (torch.softmax(heads(qq) @ heads(kk).transpose(-1, -2) * D ** -0.5, -1) @ heads(vv)).transpose(1, 2).reshape(qq.shape[0], Nq, C)
    v_s, v_l = vflat[:hw].view(1, hw, C), vflat[hw:].view(1, R * hw, C)
    check(out[:1], ref(q[:1], k_s, v_s), "short row")
    check(out[1:], ref(q[1:], k_l.expand(2, -1, -1), v_l.expand(2, -1, -1)), "long rows")
    # the as-written zero-image branch: R copies of the same keys
    rep = torch.full((1, Nq, C), float("nan"), dtype=torch.float16, device=gpu)
    k_rep, v_rep = k_s.repeat(1, R, 1), v_s.repeat(1, R, 1)
    ops.attention(q[:1], k_rep, _vt(v_rep), rep, H, D ** -0.5)
    check(out[:1], rep, "one copy of the keys vs R copies", l2=3e-4, mx=2e-3)


@pytest.mark.parametrize("shift", [-40.0, 25.0])
def test_attention_d40_fast_path_extreme_maxima(gpu, shift):
    """The D = 40 path keeps the running maximum in two fp16 contraction slots (hi + lo) and starts from a placeholder of 0: rows whose
    scores are all far below zero (exp2 of the raw first tile underflows) or far above it (the maximum needs both halves), with the
    maximum moving between tiles, must come out like torch's softmax."""
    from storygen_amd import ops
    B, H, Nq, Nk, D = 1, 8, 256, 448, 40
    C = H * D
    q, k, v = rnd((B, Nq, C), gpu, 1.0, seed=7), rnd((B, Nk, C), gpu, 1.0, seed=8), rnd((B, Nk, C), gpu, seed=9)
    qh, kh = q.view(B, Nq, H, D), k.view(B, Nk, H, D)
    # a common component along one direction shifts every score of a row by `shift` * |row scale| (log2 units: x 1.44 / sqrt(40))
    qh[..., 0] = 8.0
    kh[..., 0] = shift
    kh[0, 200:, :, 0] = shift * 1.5 if shift > 0 else shift * 0.5      # later tiles: higher maximum -> rescale with a large delta
    out = torch.empty(B, Nq, C, dtype=torch.float16, device=gpu)
    ops.attention(q, k, _vt(v), out, H, D ** -0.5)

    def heads(t):
        return t.float().view(B, -1, H, D).transpose(1, 2)
    ref = (torch.softmax(heads(q) @ heads(k).transpose(-1, -2) * D ** -0.5, -1) @ heads(v)).transpose(1, 2).reshape(B, Nq, C)
    check(out, ref, "attention extreme maxima", l2=2e-3, mx=6e-3)


def test_attention_d40_fast_path_vs_general_path(gpu):
    """Development switch attn_d40_general: the round-3 softmax (exponent FMA, row-sum adds) and the round-4 fast path (both in the
    MFMAs) on the same operands."""
    from storygen_amd import ops
    B, H, Nq, Nk, D = 2, 8, 4096, 1000, 40
    C = H * D
    q, k, v = rnd((B, Nq, C), gpu, 1.5, seed=1), rnd((B, Nk, C), gpu, 1.5, seed=2), rnd((B, Nk, C), gpu, seed=3)
    outs = []
    try:
        for general, lean in ((1, 0), (0, 0), (0, 1)):
            ops.debug_set_option("attn_d40_general", general)
            ops.debug_set_option("attn_lean", lean)
            o = torch.empty(B, Nq, C, dtype=torch.float16, device=gpu)
            ops.attention(q, k, _vt(v), o, H, D ** -0.5, nk=Nk)
            outs.append(o)
    finally:
        ops.debug_set_option("attn_d40_general", 0)
        ops.debug_set_option("attn_lean", 0)
    check(outs[1], outs[0], "fast vs general", l2=1e-3, mx=3e-3)      # (two fp16-rounded results of the same fp32 values)
    assert torch.equal(outs[1], outs[2]), "the lean instantiation computes the same values in the same order"


@pytest.mark.parametrize("D,Nq,Nk_img,Bk", [(40, 4096, 1024, 2), (40, 1024, 3072, 3), (80, 1024, 640, 2), (160, 256, 768, 3), (160, 64, 192, 2)])
def test_attention_pair_text_and_image_in_one_launch(gpu, D, Nq, Nk_img, Bk):
    """sg_attn_fwd_pair_f16: the text (77 keys, one K/V row per query batch) and the image cross-attention
    (R * HW keys, context rows shared between CFG batches) of one block in one grid — bit-identical to the two separate launches
    and equal to torch; a pair with different query geometry falls back to two launches."""
    from storygen_amd import ops
    H, B, S = 8, 3, 77
    C = H * D
    scale = D ** -0.5
    q2, q3 = rnd((B, Nq, C), gpu, 1.5, seed=1), rnd((B, Nq, C), gpu, 1.5, seed=2)
    kt, vt_ = rnd((B, 80, C), gpu, 1.5, seed=3), rnd((B, 80, C), gpu, 1.0, seed=4)
    ki, vi = rnd((Bk, Nk_img, C), gpu, 1.5, seed=5), rnd((Bk, Nk_img, C), gpu, 1.0, seed=6)
    vtt, vti = _vt(vt_), _vt(vi)
    both = torch.full((B, Nq, 2 * C), float("nan"), dtype=torch.float16, device=gpu)       # the engine's [a2 | a3] buffer
    a2, a3 = both[:, :, :C], both[:, :, C:]
    ops.attention_pair((q3, ki, vti, a3, None), (q2, kt, vtt, a2, S), H, scale)
    s2, s3 = torch.empty(B, Nq, C, dtype=torch.float16, device=gpu), torch.empty(B, Nq, C, dtype=torch.float16, device=gpu)
    # (the paired launch runs the query-split instantiation: at D = 160 select it for the single launches too — their default there is the
    # key-split kernel of round 5, equal up to the order of the fp32 sums)
    ops.debug_set_option("attn_d160", 3)
    try:
        ops.attention(q2, kt, vtt, s2, H, scale, nk=S)
        ops.attention(q3, ki, vti, s3, H, scale)
    finally:
        ops.debug_set_option("attn_d160", 4)
    torch.cuda.synchronize()
    assert torch.equal(a2, s2) and torch.equal(a3, s3)
    idx = [b if b < Bk else b - (B - Bk) for b in range(B)]

    def heads(t):
        return t.float().view(t.shape[0], t.shape[1], H, D).transpose(1, 2)
    ref3 = (torch.softmax(heads(q3) @ heads(ki[idx]).transpose(-1, -2) * scale, -1) @ heads(vi[idx])).transpose(1, 2).reshape(B, Nq, C)
    ref2 = (torch.softmax(heads(q2) @ heads(kt[:, :S]).transpose(-1, -2) * scale, -1) @ heads(vt_[:, :S])).transpose(1, 2).reshape(B, Nq, C)
    check(a3, ref3, "paired image attention")
    check(a2, ref2, "paired text attention")
    # different query counts: served as two launches, same results
    o2 = torch.full((B, Nq // 2, C), float("nan"), dtype=torch.float16, device=gpu)
    o3 = torch.full((B, Nq, C), float("nan"), dtype=torch.float16, device=gpu)
    ops.debug_set_option("attn_d160", 3)          # (the two launches it falls back to: the same instantiation as s2 / s3 above)
    try:
        ops.attention_pair((q3, ki, vti, o3, None), (q2[:, : Nq // 2], kt, vtt, o2, S), H, scale)
    finally:
        ops.debug_set_option("attn_d160", 4)
    torch.cuda.synchronize()
    assert torch.equal(o3, s3) and torch.equal(o2, s2[:, : Nq // 2])


@pytest.mark.parametrize("B,HW,C,silu,eps", [(3, 256, 320, True, 1e-5), (2, 64, 1920, True, 1e-5), (1, 100, 2560, False, 1e-6),
                                            (3, 4096, 320, False, 1e-6), (2, 1024, 960, True, 1e-5), (1, 7, 64, True, 1e-5),
                                            (4, 256, 1280, True, 1e-5), (2, 256, 2560, False, 1e-6), (3, 64, 640, True, 1e-5),
                                            (4, 4096, 640, True, 1e-5), (1, 4000, 960, False, 1e-5), (3, 1024, 1920, True, 1e-5),
                                            (2, 1000, 1280, True, 1e-6), (5, 520, 2560, True, 1e-5)])
def test_groupnorm(gpu, B, HW, C, silu, eps):
    from storygen_amd import ops
    x = (rnd((B, HW, C), gpu, 2.0, seed=1).float() + 3.0).half()      # non-zero mean
    g, b = rnd((C,), gpu, seed=2), rnd((C,), gpu, seed=3)
    out = torch.empty_like(x)
    ws = torch.empty(ops.groupnorm_workspace_bytes(B, 32), dtype=torch.uint8, device=gpu)
    ops.groupnorm(x, g, b, out, 32, eps, silu, ws)
    ref = F.group_norm(x.float().transpose(1, 2), 32, g.float(), b.float(), eps)
    ref = (F.silu(ref) if silu else ref).transpose(1, 2)
    check(out, ref, "groupnorm")


@pytest.mark.parametrize("B,H,W,C", [(3, 16, 16, 320), (2, 8, 12, 1920), (1, 4, 4, 2560), (4, 64, 64, 320), (3, 63, 64, 960),
                                     (2, 32, 32, 1280)])
def test_groupnorm_fp32_in_padded_out_rawcopy(gpu, B, H, W, C):
    """The resnet flavour: fp32 residual-stream input, SiLU, output into the zero-bordered conv input, raw fp16 copy."""
    from storygen_amd import ops
    x = rnd((B, H * W, C), gpu, 2.0, seed=1, dtype=torch.float32) + 1.5
    g, b = rnd((C,), gpu, seed=2), rnd((C,), gpu, seed=3)
    yp = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float16, device=gpu)
    xc = torch.empty(B, H * W, C, dtype=torch.float16, device=gpu)
    ws = torch.empty(ops.groupnorm_workspace_bytes(B, 32), dtype=torch.uint8, device=gpu)
    ops.groupnorm(x, g, b, yp, 32, 1e-5, True, ws, xcopy=xc)
    ref = F.silu(F.group_norm(x.transpose(1, 2), 32, g.float(), b.float(), 1e-5)).transpose(1, 2)
    check(yp[:, 1:-1, 1:-1].reshape(B, H * W, C), ref, "groupnorm padded")
    assert float(yp[:, 0].abs().max()) == 0 and float(yp[:, -1].abs().max()) == 0
    assert float(yp[:, :, 0].abs().max()) == 0 and float(yp[:, :, -1].abs().max()) == 0
    assert torch.equal(xc, x.half())


def test_groupnorm_row_strided_input(gpu):
    """Input rows that are a channel window of a wider buffer (ldx > C) through the wide two-pass kernels."""
    from storygen_amd import ops
    B, HW, C, LD = 2, 2048, 640, 960
    big = rnd((B, HW, LD), gpu, 2.0, seed=1, dtype=torch.float32) - 0.7
    x = big[:, :, 320:]
    g, b = rnd((C,), gpu, seed=2), rnd((C,), gpu, seed=3)
    out = torch.empty(B, HW, C, dtype=torch.float16, device=gpu)
    ws = torch.empty(ops.groupnorm_workspace_bytes(B, 32), dtype=torch.uint8, device=gpu)
    ops.groupnorm(x, g, b, out, 32, 1e-5, False, ws)
    check(out, F.group_norm(x.transpose(1, 2), 32, g.float(), b.float(), 1e-5).transpose(1, 2), "groupnorm strided")


def test_layernorm_fp32_input(gpu):
    from storygen_amd import ops
    x = rnd((300, 640), gpu, 2.0, seed=1, dtype=torch.float32) + 1.0
    g, b = rnd((640,), gpu, seed=2), rnd((640,), gpu, seed=3)
    y = torch.empty(300, 640, dtype=torch.float16, device=gpu)
    ops.layernorm(x, g, b, y)
    check(y, F.layer_norm(x, (640,), g.float(), b.float(), 1e-5), "layernorm fp32 in")


@pytest.mark.parametrize("M,C", [(1024, 320), (300, 640), (77, 1280), (5, 64)])
def test_layernorm_dual(gpu, M, C):
    from storygen_amd import ops
    x = (rnd((M, C), gpu, 2.0, seed=1).float() + 1.0).half()
    g1, b1, g2, b2 = (rnd((C,), gpu, seed=s) for s in (2, 3, 4, 5))
    y1, y2 = torch.empty_like(x), torch.empty_like(x)
    ops.layernorm(x, g1, b1, y1, 1e-5, g2, b2, y2)
    check(y1, F.layer_norm(x.float(), (C,), g1.float(), b1.float(), 1e-5), "layernorm 1")
    check(y2, F.layer_norm(x.float(), (C,), g2.float(), b2.float(), 1e-5), "layernorm 2")
    ops.layernorm(x, g2, b2, y1, 1e-5)
    check(y1, F.layer_norm(x.float(), (C,), g2.float(), b2.float(), 1e-5), "layernorm single")


def test_time_embedding_path(gpu):
    """Timesteps -> linear_1 -> SiLU -> linear_2, then SiLU -> time_emb_proj (unet_2d_condition.py:392-398)."""
    from storygen_amd import ops
    B, dim, temb = 3, 320, 1280
    t = torch.tensor([981.0, 98.0, 1.0], device=gpu)
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half).to(gpu)
    emb = torch.empty(B, dim, device=gpu)
    ops.timestep_embed(t, freqs, emb, True)
    e = t[:, None] * freqs[None]
    check(emb, torch.cat([torch.cos(e), torch.sin(e)], -1), "timestep embed", l2=1e-5, mx=1e-4)
    w1, b1 = rnd((temb, dim), gpu, 0.05, seed=1), rnd((temb,), gpu, seed=2)
    w2, b2 = rnd((960, temb), gpu, 0.03, seed=3), rnd((960,), gpu, seed=4)
    h = torch.empty(B, temb, device=gpu)
    ops.linear_rows(emb, w1, b1, h, act_out=True)
    ref_h = F.silu(emb @ w1.float().t() + b1.float())
    check(h, ref_h, "linear_rows silu-out", l2=1e-5, mx=1e-4)
    y = torch.empty(B, 960, device=gpu)
    ops.linear_rows(h, w2, b2, y, act_in=True)
    check(y, F.silu(ref_h) @ w2.float().t() + b2.float(), "linear_rows silu-in", l2=1e-5, mx=1e-4)


def test_conv_in_out(gpu):
    from storygen_amd import ops
    B, H, W, C = 3, 16, 24, 320
    x = rnd((B, 4, H, W), gpu, seed=1, dtype=torch.float32)
    w = rnd((C, 4, 3, 3), gpu, 1 / 6, seed=2)
    b = rnd((C,), gpu, seed=3)
    y = torch.empty(B, H, W, C, dtype=torch.float16, device=gpu)
    ops.conv_in(x, w.permute(2, 3, 1, 0).reshape(36, C).contiguous(), b, y)
    check(y.permute(0, 3, 1, 2), F.conv2d(x, w.float(), b.float(), padding=1), "conv_in")
    y32 = torch.empty(B, H, W, C, dtype=torch.float32, device=gpu)
    ops.conv_in(x, w.permute(2, 3, 1, 0).reshape(36, C).contiguous(), b, y32)
    check(y32.permute(0, 3, 1, 2), F.conv2d(x, w.float(), b.float(), padding=1), "conv_in fp32", l2=1e-5, mx=1e-4)
    wo = rnd((4, C, 3, 3), gpu, 1 / math.sqrt(9 * C), seed=4)
    bo = rnd((4,), gpu, seed=5)
    out = torch.empty(B, 4, H, W, device=gpu)
    ops.conv_out(y, wo.permute(0, 2, 3, 1).contiguous(), bo, out)
    check(out, F.conv2d(y.permute(0, 3, 1, 2).float(), wo.float(), bo.float(), padding=1), "conv_out", l2=1e-5, mx=1e-4)


def test_sampling_elementwise(gpu):
    from storygen_amd import ops
    N, shape = 2, (2, 4, 16, 16)
    zero, img, noise, lat = (rnd(shape, gpu, seed=s, dtype=torch.float32) for s in (1, 2, 3, 4))
    coef = torch.tensor([[0.9, 0.43], [0.9, 0.43], [0.7, 0.71], [0.5, 0.86]], device=gpu)   # per-sample timesteps
    src = torch.cat([zero, img])
    out4 = torch.empty(2 * N, 4, 16, 16, device=gpu)
    ops.add_noise(src, noise, coef, out4)
    ref = torch.stack([coef[u, 0] * src[u] + coef[u, 1] * noise[u % N] for u in range(2 * N)])
    check(out4, ref, "add_noise", l2=1e-6, mx=1e-6)
    eps3 = rnd((3 * N, 4, 16, 16), gpu, seed=5, dtype=torch.float32)
    c = torch.tensor([3.5, 7.5, 0.8, 0.6, 0.85, 0.5267], device=gpu)
    eu, ei, ea = eps3.chunk(3)
    eps = eu + 3.5 * (ei - eu) + 7.5 * (ea - ei)
    ref = 0.85 * (lat - 0.6 * eps) / 0.8 + 0.5267 * eps
    lat3 = torch.empty(3 * N, 4, 16, 16, device=gpu)
    ops.cfg_ddim_step(eps3, lat, lat3, c)
    check(lat, ref, "cfg+ddim", l2=1e-6, mx=1e-5)
    check(lat3, torch.cat([ref] * 3), "cfg+ddim replicate", l2=1e-6, mx=1e-5)


def test_copy_rows(gpu):
    from storygen_amd import ops
    src = rnd((3, 50, 640), gpu, seed=1)
    dst = torch.zeros(3, 150, 960, dtype=torch.float16, device=gpu)
    ops.copy_rows(dst[:, 50:100, 320:], src)
    assert torch.equal(dst[:, 50:100, 320:], src) and float(dst[:, :50].abs().max()) == 0 and float(dst[:, :, :320].abs().max()) == 0
    src32 = rnd((2, 33, 64), gpu, seed=2, dtype=torch.float32)
    d32 = torch.zeros(2, 40, 128, device=gpu)
    ops.copy_rows(d32[:, 3:36, 64:], src32)
    assert torch.equal(d32[:, 3:36, 64:], src32)
    d16 = torch.zeros(2, 33, 64, dtype=torch.float16, device=gpu)
    ops.copy_rows(d16, src32)
    assert torch.equal(d16, src32.half())


def test_abi_rejects_bad_arguments(gpu):
    """Errors are reported through the return code + sg_last_error(), mirrored as RuntimeError (SURVEY §8b Errors)."""
    from storygen_amd import ops
    a, w = rnd((64, 60), gpu), rnd((64, 60), gpu)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ops.gemm(a, w, torch.empty(64, 64, dtype=torch.float16, device=gpu))
    q = rnd((1, 64, 8 * 48), gpu)
    with pytest.raises(RuntimeError, match="head dim"):
        ops.attention(q, q, q.transpose(1, 2).contiguous(), torch.empty_like(q), 8, 1.0)
