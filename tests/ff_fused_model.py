"""CPU model of the fused GEGLU feed-forward (sg_ff_geglu_fused_f16) and of its weight stream, written from the comment blocks of
csrc/ff_fused.hip and of storygen_amd/repack.py (ff_fused_pack, fold_layernorm, interleave_geglu).  Plain torch, float64.

Operands, everywhere: x [M, C] fp32; w1 [8C, C] (rows [0, 4C) values, [4C, 8C) gates: ff.net.0.proj.weight), b1 [8C]; gamma, beta [C]
(norm3); w2 [C, 4C] fp16 (ff.net.2.weight), b2 [C]; eps.  All CPU tensors; the values they hold are taken as given (fp16 or fp32).

  exact(x, w1, b1, gamma, beta, w2, b2, eps, halves=False)
        float64 LayerNorm -> Linear(C, 8C) -> a * gelu_erf(g) -> Linear(4C, C) -> + b2 + x: the REFERENCE of
        the GPU edge module (below).  halves=True: the two outputs of the hidden split (sg_ff_desc.hidden_split = 2) —
        hidden units [0, 2C) + b2 + x, and hidden units [2C, 4C) alone.
  rounded(...)   the same computation with the kernel's DOCUMENTED roundings and nothing else:
        xhat = (x - mean) rstd               -> fp16 (the B-operand fragments of GEMM1)
        gamma (.) W1                         -> fp16 (repack.fold_layernorm)
        d1 = W1 beta + b1 (fp32)             -> fp16(d1) + fp16(d1 - fp16(d1))   (the (hi, lo) k-step of the pack)
        a * 2 gelu(g)                        -> fp16, INCLUDING the overflow to inf from 65520 on, times fp16(W2 / 2)
        y                                    -> fp16 (each half on its own under the split)
        Sums are exact (float64).  Not modelled: the order of the fp32 sums, the fp32 LayerNorm statistics, v_rcp_f32 / v_exp_f32
        and the Abramowitz-Stegun erf (|error| <= 1.5e-7).  It is the yardstick of the per-row bar: what a correct kernel cannot avoid.
  max_row_error(got, ref)   max over the rows of ||got_row - ref_row|| / RMS over the rows of ||ref_row|| (the metric of
                            tests/attention_fwd_model.py, one "head" of width C).
  unpack(stream, C)   inverse of the weight stream, written from the KERNEL's address formulas (w1v / w1g / w2o / dvo / dgo of
                      ff_fused_kernel) and the MFMA fragment maps pinned by tests/test_kernels_gpu.py::test_mfma_fragment_layout —
                      not from repack.py: -> (w1f [8C, C] fp16 in interleaved row order, d1 [8C] float64 = hi + lo, W2 / 2 [C, 4C] fp16
                      as stored).
Also here: the inputs of the GPU edge module, each maker asserting the condition the GPU bar relies on.

The GPU edge module itself (row counts, position, layout, hidden-unit probe, LayerNorm edges, isolation, range, refusals) is not in the
tree: it passed on an MI355X (profiles/r23a_ff_fused_edge_tests.txt), then a run of the GPU suite that contained it aborted and the cause
was not found.  It comes back when that cause is known; this model, its inputs and tests/test_ff_fused_model.py are what it stands on."""
import math

import torch

from attention_bwd_model import rel_l2  # noqa: F401  (re-exported)

C = 320                       # the one width the kernel is built for
F16_MAX = 65504.0
HIDDEN_LIMIT = F16_MAX / 2    # |a gelu(g)| above which fp16(a * 2 gelu(g)) may stop being finite (it does from 32760 on)


def _f16(t):
    return t.to(torch.float16).double()


def gelu_erf(g):
    """g Phi(g) in float64, without the cancellation of 1 + erf for negative g."""
    g = g.double()
    return 0.5 * g * torch.special.erfc(-g / math.sqrt(2.0))


def _layernorm_hat(x, eps):
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    var = (xd - mean).pow(2).mean(-1, keepdim=True)
    return (xd - mean) / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))      # eps as the float the C ABI carries


def _model(x, w1, b1, gamma, beta, w2, b2, eps, halves, rnd):
    Cc = x.shape[-1]
    xhat = _layernorm_hat(x, eps)
    if rnd:
        xhat = _f16(xhat)
        w1f = (w1.float() * gamma.float()[None]).to(torch.float16).double()
        d1 = (w1.double() @ beta.double() + b1.double()).to(torch.float32)
        hi = d1.to(torch.float16)
        d = hi.double() + (d1 - hi.float()).to(torch.float16).double()
        h = xhat @ w1f.t() + d
    else:
        h = (xhat * gamma.double() + beta.double()) @ w1.double().t() + b1.double()
    a, g = h[:, : 4 * Cc], h[:, 4 * Cc:]
    if rnd:
        act = _f16(a * (2.0 * gelu_erf(g)))                   # fp16: +-inf from 65520 on
        w2d = (w2.to(torch.float16) * 0.5).double()           # the pack's halved W2 (exact down to the subnormals)
    else:
        act, w2d = a * gelu_erf(g), w2.double()
    first = act[:, : 2 * Cc] @ w2d[:, : 2 * Cc].t() + b2.double() + x.double()
    second = act[:, 2 * Cc:] @ w2d[:, 2 * Cc:].t()
    if halves:
        return (_f16(first), _f16(second)) if rnd else (first, second)
    return _f16(first + second) if rnd else first + second


def exact(x, w1, b1, gamma, beta, w2, b2, eps=1e-5, halves=False):
    return _model(x, w1, b1, gamma, beta, w2, b2, eps, halves, False)


def rounded(x, w1, b1, gamma, beta, w2, b2, eps=1e-5, halves=False):
    return _model(x, w1, b1, gamma, beta, w2, b2, eps, halves, True)


def row_errors(got, ref):
    """e_row = ||got_row - ref_row|| / RMS over the rows of ||ref_row||; [M].  A zero error is 0 whatever the reference."""
    got, ref = got.double(), ref.double()
    err = (got - ref).norm(dim=-1)
    rms = ref.norm(dim=-1).pow(2).mean().sqrt()
    return torch.where(err == 0, torch.zeros_like(err), err / rms)


def max_row_error(got, ref):
    return float(row_errors(got, ref).max())


# ------------------------------------------------------------------------------------------------ the weight stream
def _rho(p):
    """MFMA row of a chunk's hidden unit p.  GEMM1's result register r of lane (token, hi) is tile row (r & 3) + 8 (r >> 2) + 4 hi; GEGLU
    keeps it in place and GEMM2's B fragment of k-step ks takes registers 8 ks + j as k = 8 hi + j, i.e. hidden unit 16 ks + 8 hi + j."""
    ks, hi, j = p >> 4, (p >> 3) & 1, p & 7
    r = 8 * ks + j
    return (r & 3) + 8 * (r >> 2) + 4 * hi


def stream_sizes(Cc):
    """(chunks, W1_IMG, W1_PART, W2_PART, CHUNK) as ff_fused_kernel's constexprs give them."""
    ks = Cc // 64
    w1_img = ks * 8192
    w1_part = w1_img + 64 * 32
    w2_part = Cc * 64
    return 4 * Cc // 32, w1_img, w1_part, w2_part, w1_part + w2_part


def unpack(stream, Cc=C, pad=False):
    """See the module docstring.  pad=True: also the 14 halves per d1 row that the constant fragment (1, 1, 0, ...) multiplies by zero
    ([chunks, 64, 14] fp16: they must be zero — a NaN there would still poison the accumulator)."""
    nch, w1_img, w1_part, _, chunk = stream_sizes(Cc)
    assert stream.dtype == torch.uint8 and stream.numel() == nch * chunk
    halves = stream.cpu().contiguous().view(torch.float16)              # the stream as fp16 elements; byte b = element b / 2
    c = torch.arange(nch).view(nch, 1, 1, 1)
    p = torch.arange(32).view(1, 32, 1, 1)
    row = torch.tensor([_rho(i) for i in range(32)]).view(1, 32, 1, 1)
    # GEMM1: lane (l31 = tile row, hi) reads, for k-step s, 16 bytes at slab (s >> 2) * 8192 + w1v / w1g[s & 3] as A[i = l31][k = 8 hi + j]
    # against the xhat fragment of columns 16 s + 8 hi + j
    k = torch.arange(Cc).view(1, 1, Cc, 1)
    s, hi, j = k >> 4, (k >> 3) & 1, k & 7
    tiles = []
    for t in range(2):                                                   # w1v: rows l31; w1g: rows 32 + l31
        r = 32 * t + row
        byte = c * chunk + (s >> 2) * 8192 + r * 128 + ((((s & 3) * 2 + hi) ^ ((r >> 1) & 7)) << 4) + 2 * j
        tiles.append(halves[(byte >> 1).reshape(-1)].view(nch, 32, Cc))
    w1f = torch.stack(tiles, dim=1).reshape(8 * Cc, Cc)                  # interleaved row 64 c + 32 t + p
    # d1: dvo / dgo = W1_IMG + row * 32 (+ hi * 16); the activation side is (1, 1, 0, ...): elements 0 and 1 of the row are summed
    r64 = torch.cat([row.view(32), 32 + row.view(32)]).view(1, 64)
    base = (torch.arange(nch).view(nch, 1) * chunk + w1_img + r64 * 32) >> 1
    d1 = (halves[base.reshape(-1)].double() + halves[(base + 1).reshape(-1)].double()).view(8 * Cc)
    # GEMM2: lane (l31, hi) reads 16 bytes at ct * 2048 + w2o[ks] as A[i = l31][k = 8 hi + j]: output column ct * 32 + l31, hidden unit
    # 16 ks + 8 hi + j of the chunk
    n = torch.arange(Cc).view(1, Cc, 1)
    ct, l31 = n >> 5, n & 31
    pp = torch.arange(32).view(1, 1, 32)
    ks2, hi2, j2 = pp >> 4, (pp >> 3) & 1, pp & 7
    byte = torch.arange(nch).view(nch, 1, 1) * chunk + w1_part + ct * 2048 + l31 * 64 + (((ks2 * 2 + hi2) ^ ((l31 >> 2) & 3)) << 4) + 2 * j2
    w2 = halves[(byte >> 1).reshape(-1)].view(nch, Cc, 32).permute(1, 0, 2).reshape(Cc, 4 * Cc)
    if not pad:
        return w1f, d1, w2
    rest = (base.view(nch, 64, 1) + torch.arange(2, 16).view(1, 1, 14)).reshape(-1)
    return w1f, d1, w2, halves[rest].view(nch, 64, 14)


# ------------------------------------------------------------------------------------------------ inputs
def _r(shape, seed, scale=1.0, dtype=torch.float16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def weights(seed=0, Cc=C):
    """The weight set of tests/test_kernels_gpu.py::test_fused_geglu_feed_forward at another seed: fp16 CPU tensors."""
    s = 100 * seed
    return dict(w1=_r((8 * Cc, Cc), s + 2, Cc ** -0.5), b1=_r((8 * Cc,), s + 3, 0.5), gamma=_r((Cc,), s + 6, 0.2) + 1.0,
                beta=_r((Cc,), s + 7, 0.2), w2=_r((Cc, 4 * Cc), s + 4, (4 * Cc) ** -0.5), b2=_r((Cc,), s + 5, 0.5))


def ff_term(x, w, eps=1e-5):
    """Linear2(a gelu(g)) alone, float64: the part of y that the GEMMs compute."""
    return exact(x, w["w1"], w["b1"], w["gamma"], w["beta"], w["w2"], w["b2"], eps) - w["b2"].double() - x.double()


def small_residual(M, w, seed=0):
    """x ~ 0.04 N(0, 1) + 0.01 (fp32): LayerNorm sees the same rows as at any other scale, and the residual is small against the
    feed-forward term, so that an aggregate bar on y measures the GEMMs: ||FF|| >= 10 ||x|| (asserted)."""
    x = _r((M, w["w2"].shape[0]), 1000 + seed, 0.04, torch.float32) + 0.01
    ff = ff_term(x, w)
    assert float(ff.norm()) >= 10.0 * float(x.double().norm()), "small_residual: the feed-forward term must dominate x"
    return x


def layernorm_edge(kind, w, M=40, seed=0):
    """fp32 x [M, C] for the LayerNorm edges:
      constant   every row one value (0, 0.75, -3, 0.4137, 100.3, cycled): variance 0
      mean1e4    N(0, 1) + 1e4: the two-pass statistics must not cancel
      tiny_var   0.25 + 1e-4 N(0, 1): variance 1e-8, far below eps = 1e-5
      outlier    small_residual rows; row 7 is N(0, 1) with one element 1e4: |xhat| of that element is near sqrt(C)"""
    Cc = w["w2"].shape[0]
    if kind == "constant":
        vals = torch.tensor([0.0, 0.75, -3.0, 0.4137, 100.3], dtype=torch.float32)
        x = vals[torch.arange(M) % vals.numel()].view(M, 1).expand(M, Cc).contiguous()
        assert float(x.double().var(-1, unbiased=False).max()) == 0.0
    elif kind == "mean1e4":
        x = _r((M, Cc), 2000 + seed, 1.0, torch.float32) + 1.0e4
        sd = x.double().std(-1)
        assert float((x.double().mean(-1) - 1.0e4).abs().max()) < 1.0 and 0.8 < float(sd.min()) and float(sd.max()) < 1.2
    elif kind == "tiny_var":
        x = _r((M, Cc), 2100 + seed, 1.0e-4, torch.float32) + 0.25
        assert float(x.double().var(-1, unbiased=False).max()) < 1.0e-2 * 1.0e-5
    elif kind == "outlier":
        x = small_residual(M, w, 2200 + seed)
        x[7] = _r((Cc,), 2300 + seed, 1.0, torch.float32)
        x[7, 123] = 1.0e4
        xh = _layernorm_hat(x[7:8], 1e-5)
        assert float(xh[0, 123]) > 0.99 * math.sqrt(Cc - 1)
    else:
        raise ValueError(kind)
    return x


def f16_ulp(v):
    """Spacing of fp16 at |v| (float64 tensor): 2^(floor(log2 |v|) - 10), 2^-24 in the subnormal range."""
    e = torch.floor(torch.log2(v.double().abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


# Gates every sweep must hold (the issue's list), then gates in [-4, -2) whose fp16 (hi, lo) split has a lo half near half an ulp of hi: there
# gelu is steep relative to its value, and a dropped lo half moves the result by more than the probe's tolerance.
GATES_REQUIRED = (0.0, -0.0, 1e-4, -1e-4, -5.5, -8.0, 8.0, 1.0, -1.0, 10.0, -10.0)
GATES_NEED_LO = tuple(-(2.0 + 2.0 ** -9 * (i + 0.45)) for i in range(0, 512, 23))
VALUES_SECOND = (0.5, -0.5, 3.0, -3.0, 100.0, -100.0, 1000.123, -1000.123, 0.333251953125 + 2.0 ** -14, 77.7777)


def probe_d1(sweep):
    """(a, g) fp32 [4C] each — hidden unit j's value and gate term of the hidden-unit probe (x = 0, W1 = 0, so h = d1 exactly).
      sweep "gate"    a_j = 1; g_j sweeps [-10, 10]: the required gates, the lo-half gates, then an even grid
      sweep "value"   a_j cycles through +-{0.5, 3, 100} and values that need the lo half of the (hi, lo) split (1000.123, ...);
                      g_j as in "gate" but shifted by 7 units, so that every value meets many gates
    Every expected a_j gelu(g_j) is finite and below the hidden range limit (asserted)."""
    n = 4 * C
    fixed = torch.tensor(GATES_REQUIRED + GATES_NEED_LO, dtype=torch.float32)
    grid = torch.linspace(-10.0, 10.0, n - fixed.numel(), dtype=torch.float64).to(torch.float32)
    g = torch.cat([fixed, grid])
    g = g[(torch.arange(n) * 37) % n]                                  # 37 is coprime to 1280: neighbours in j are far apart in g
    if sweep == "gate":
        a = torch.ones(n, dtype=torch.float32)
    elif sweep == "value":
        vals = torch.tensor(VALUES_SECOND, dtype=torch.float32)
        a = vals[torch.arange(n) % vals.numel()]
        g = torch.roll(g, 7)
    else:
        raise ValueError(sweep)
    want = a.double() * gelu_erf(g)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) < HIDDEN_LIMIT, "probe_d1: expected values must be finite and in range"
    return a, g


def probe_weights(a, g, quarter, ones=1.0):
    """The weight set of one probe launch: W1 = 0, gamma = 1, beta = 0, b1 = [a | g] (fp32), b2 = 0, and W2 one-hot — hidden unit j of
    [320 quarter, 320 quarter + 320) feeds column j mod 320, every other hidden unit nothing.  With x = 0: y[:, j mod 320] = a_j gelu(g_j)."""
    w2 = torch.zeros(C, 4 * C, dtype=torch.float16)
    j = torch.arange(C * quarter, C * quarter + C)
    w2[j % C, j] = ones
    return dict(w1=torch.zeros(8 * C, C, dtype=torch.float16), b1=torch.cat([a, g]).to(torch.float32), gamma=torch.ones(C, dtype=torch.float16),
                beta=torch.zeros(C, dtype=torch.float16), w2=w2, b2=torch.zeros(C, dtype=torch.float16))


def probe_tolerance(a, g):
    """One fp16 ulp of the expected value (the fp16 roundings of a * 2 gelu(g) and of y) + 1e-6 |a g| (the fp32 erf of the kernel,
    4.7e-7, doubled for v_rcp_f32 / v_exp_f32)."""
    return f16_ulp(a.double() * gelu_erf(g)) + 1.0e-6 * (a.double() * g.double()).abs()


RANGE_GATE = 8.0       # 2 gelu(8) = 16 (1 - 6e-16): 16 exactly in fp32, so a * 2 gelu(g) = 16 a with no rounding at all


def range_d1(level, hot=()):
    """(a, g) of the range case: every hidden unit of quarter 0 at a_j gelu(g_j) = 30000 (a = 3750, g = 8), the units `hot` at `level`
    (a = level / 8; level / 8 must be an fp16 value so that the (hi, lo) split is exact).  Asserts where the inputs sit."""
    a = torch.zeros(4 * C, dtype=torch.float32)
    g = torch.full((4 * C,), RANGE_GATE, dtype=torch.float32)
    a[:C] = 30000.0 / RANGE_GATE
    for j in hot:
        a[j] = level / RANGE_GATE
    assert bool((a.to(torch.float16).float() == a).all()), "range_d1: a must be exact in fp16"
    want = a.double() * gelu_erf(g)
    assert float((want[:C] - a[:C].double() * RANGE_GATE).abs().max()) < 1e-9
    assert all(abs(float(want[j]) - level) < 1e-9 for j in hot)
    return a, g
