"""Float64 model of the CONSUMER side of the LayerNorm fold (storygen_amd/csrc/gemm_conv.hip: ln_token_coeffs and the ln_mode branches of
epi_finish), with a derived per-element error bar and the guard flags the kernel must raise.  Plain torch, no kernel, no GPU.

The operation.  A GEMM on the raw fp16 tokens x16 [tokens, K] with the folded fp16 weight W' [rows, K], then per output element
    mode 1 (tokens are the rows of the product):     out[t, n] = r_t (x16 W'^T)[t, n] - (m_t r_t) c_n + d_n + bias_n
    mode 2 (tokens are the columns, V^T = W' X^T):   out[n, t] = r_t (W' x16^T)[n, t] - (m_t r_t) c_n + d_n + bias_t
    GEGLU (mode 1, interleaved layout of repack.interleave_geglu: columns 64 u .. 64 u + 31 are values, 64 u + 32 .. 64 u + 63 their gates):
                                                     out[t, 32 u + i] = val[t, 64 u + i] * gelu_erf(val[t, 64 u + 32 + i])
m_t and r_t = 1 / sqrt(var_t + eps) come from the fp32 table AS THE KERNEL READS IT — per token and 64-channel block (sum, M2 about the block
mean) — merged in float64 with Chan's formula: m = sum_q s_q / (64 P), M2 = sum_q [M2_q + 64 (s_q / 64 - m)^2], var = M2 / (64 P).  eps is
rounded to fp32 first (the descriptor carries a float).  The padding block of an odd P is never read by the model.

The bar, per output element, u = 2^-24, gamma_n = n u / (1 - n u).  Nothing in it is fitted: every term is an operation count of the kernel source
times the magnitude that operation acts on.
 1. Accumulation, any summation order:  |acc^ - acc| <= gamma_K sum_k |x16_tk| |w'_nk|; it reaches the output multiplied by r^.
 2. ln_token_coeffs, from its operations on the fp32 table entries s_q, M2_q:
      tot = P additions, mean = one division:             e_m  = gamma_(P+1) sum_q |s_q| / (64 P)
      dm_q = s_q / 64 - mean^ (s_q / 64 is exact):         e_dm = e_m (1 + u) + u |dm_q|
      t_q = fma(64 dm_q, dm_q, M2_q), then P additions:   e_M2 = (1 + gamma_(P+1)) sum_q (128 |dm_q| e_dm + 64 e_dm^2) + gamma_(P+1) sum_q t_q
      var = M2 / (64 P) (one division), v = var + eps (one addition):   e_v = e_M2 / (64 P) + u var^ + u v^
      r = rsqrt(v): the one constant the source cannot give.  v_rsq_f32 is specified to 1 ULP (AMD Instinct CDNA3 / CDNA4 ISA reference
      guide, "V_RSQ_F32 ... 1ULP accuracy"; the ROCm HIP math API lists rsqrtf with a maximum error of 1 ULP), i.e. a relative 2^-23:
                                                          e_r  = r ((1 + 2^-23) (1 + rho / (2 (1 - rho))) - 1),   rho = e_v / v
      mr = mean^ r^ (one multiplication):                 e_mr = (|m| + e_m)(r + e_r) - |m| r + u (|m| + e_m)(r + e_r)
    They reach the output as |acc| e_r + |c| e_mr.
 3. One u per fp32 operation of the epilogue `fma(r, acc, d + bias) - mr c`, on the magnitude it acts on: the addition d + bias (|d| + |bias|, only
    with a bias), the fma (|r acc| + |d| + |bias|), the product (|mr c|), the subtraction (|r acc| + |mr c| + |d| + |bias|).  These are ABSOLUTE:
    r acc and mr c cancel when |mean| / sigma is large and the bar must not shrink with the result.
 4. One output rounding: 2^-24 |value| for fp32 outputs, 2^-11 |value| (2^-25 absolute below the fp16 normal range) for fp16 outputs.
 5. GEGLU: value and gate each carry 1..3 as e_val, e_gate; the product val * G, G = gelu_erf(gate), is off by at most
      e_val (|G| + e_G) + |val| e_G + u |val G|,   e_G = L e_gate + e_gelu,
    L = max |gelu_erf'| = Phi(sqrt 2) + sqrt 2 phi(sqrt 2) < 1.13 (the Lipschitz bound), and e_gelu the kernel's own evaluation error of
    0.5 (g + |g| E(|g|)): E is Abramowitz-Stegun 7.1.26 (|E - erf| <= 1.5e-7, their stated bound) evaluated with v_rcp_f32 and v_exp_f32 (1 ULP
    each, same ISA guide): t = rcp(fma(..)) relative 4 u; the five-term Horner form gamma_10 sum |a_i| + sum i |a_i| 4 u = (44.8 + 64.8) u;
    exp2(-zs^2) absolute 4 u; E = fma(-q, e, 1) one more u: 115 u in all, so e_gelu = 0.5 |g| (1.5e-7 + 115 u) + u |g|.

guard_flags: the documented rule of SG_LN_GUARD_OFFSET — set iff some token t < tokens has |m_t| r_t > 16; the consumer never sets RANGE.

CPU figure (tests/test_ln_fold_model.py, torch fp32 evaluating the same formula with a sequential fp32 merge, at every shape of the GPU file):
worst |err| / bar 0.037 (linear) and 0.010 (GEGLU) on fp32 outputs; 0.96 and 0.69 on fp16 outputs, where the largest term of the bar is the half-ulp
fp16 rounding 2^-11 |value| — a bound that is attained, so a ratio near 1 there is that rounding and not a thin derivation (the fp32 figures are
the derivation's).  On the MI355X: profiles/r28a_layernorm_fold_edge_tests.txt.

The case tables of tests/test_layernorm_fold_edges_gpu.py live here so that the CPU tests run at exactly the shapes the GPU file uses."""
import math

import torch

F64 = torch.float64
U = 2.0 ** -24
RSQ_REL = 2.0 ** -23              # v_rsq_f32: 1 ULP (ISA reference guide)
GELU_LIP = 1.13                   # max |gelu_erf'| = 1.12890...
GELU_EVAL = 1.5e-7 + 115 * U      # Abramowitz-Stegun 7.1.26 plus the arithmetic of its evaluation
GUARD_RATIO, GUARD_OFFSET = 16.0, 2

# ---------------------------------------------------------------------------------------------------- case tables of the GPU file
PIPE_TILES = [(256, 128), (128, 128), (256, 64), (128, 64), (64, 128), (64, 64)]
LAT_TILES = [(64, 64, 4), (64, 128, 8)]
FAT_TILES = [(512, 128, 8), (256, 256, 8)]
ALL_TILES = [t + (0,) for t in PIPE_TILES] + LAT_TILES + FAT_TILES       # (bm, bn, tile_waves): 0 = the 64x64-per-wave pipeline
K_A = 320                                                               # P = 5: odd, one padding block


def shapes_a(bm, bn, mode):
    """Group A: (M, N) of the product.  Mode 1: tokens = M; mode 2: tokens = N."""
    if mode == 1:
        return [(M, N) for M in (1, bm - 1, bm + 1) for N in (8, 72, bn + 8)]
    return [(M, N) for N in (8, 72, bn + 8) for M in (8, 72, bm + 8)]


PARTS_B = [1, 2, 3, 19, 20]
MN_B = (65, 72)
GEGLU_M, GEGLU_N = (1, 63, 65), (128, 192)
MN_E = (136, 136, 72)             # tokens, N of the q|k problem, rows of the V^T problem
MN_H = (200, 320)


def all_shapes():
    """Every (M, N, K, mode, geglu) the GPU file launches with ln=."""
    out = set()
    for bm, bn, _ in ALL_TILES:
        for mode in (1, 2):
            out |= {(M, N, K_A, mode, False) for M, N in shapes_a(bm, bn, mode)}
    out |= {(MN_B[0], MN_B[1], 64 * P, 1, False) for P in PARTS_B}
    out |= {(M, N, K_A, 1, True) for M in GEGLU_M for N in GEGLU_N}
    out |= {(MN_E[0], MN_E[1], K_A, 1, False), (MN_E[2], MN_E[0], K_A, 2, False)}
    out |= {(MN_H[0], 2 * MN_H[1], MN_H[1], 1, False)}
    return sorted(out)


# ------------------------------------------------------------------------------------------------------------------ inputs
def gamma_n(n):
    return n * U / (1.0 - n * U)


def make_tokens(tokens, K, seed, block_means=None, block_sigmas=None):
    """float64 [tokens, K]: every 64-channel block of every token has a mean and a spread of its own (uniform in [-3, 3] and [0.5, 2] unless
    given as [tokens, P] / broadcastable), so a swapped, repeated or dropped block moves the token's statistics by O(1)."""
    g = torch.Generator().manual_seed(seed)
    P = K // 64
    z = torch.randn(tokens, P, 64, generator=g, dtype=F64)
    mu = torch.rand(tokens, P, 1, generator=g, dtype=F64) * 6.0 - 3.0
    sg = torch.rand(tokens, P, 1, generator=g, dtype=F64) * 1.5 + 0.5
    if block_means is not None:
        mu = torch.as_tensor(block_means, dtype=F64).expand(tokens, P).reshape(tokens, P, 1)
    if block_sigmas is not None:
        sg = torch.as_tensor(block_sigmas, dtype=F64).expand(tokens, P).reshape(tokens, P, 1)
    return (mu + sg * z).reshape(tokens, K)


def table_from_x(x, pad=float("nan")):
    """The producer's table of x [tokens, K] in float64: [tokens, P rounded up to even, 2] = (sum, M2 about the block mean) per 64-channel block;
    the padding block of an odd P holds `pad`.  `.float()` rounds it to what the kernel reads."""
    tokens, K = x.shape
    P = K // 64
    b = x.to(F64).reshape(tokens, P, 64)
    t = torch.full((tokens, (P + 1) & ~1, 2), pad, dtype=F64, device=x.device)
    t[:, :P, 0] = b.sum(2)
    t[:, :P, 1] = ((b - b.mean(2, keepdim=True)) ** 2).sum(2)
    return t


def handmade_table(tokens, P, mean, ratio, eps, spread=0.0, pad=float("nan")):
    """float64 table whose every token merges to exactly `mean` and to |mean| r = `ratio` (r = 1 / sqrt(var + fp32(eps))), with no x behind it:
    block q sits at mean + spread * (q - (P - 1) / 2) (the offsets sum to zero) and the blocks share the remaining M2 equally.  ratio = None
    with mean = 0: variance 1."""
    eps = float(torch.tensor(eps, dtype=torch.float32))
    var = 1.0 if ratio is None else (mean / ratio) ** 2 - eps
    off = spread * (torch.arange(P, dtype=F64) - (P - 1) / 2.0)
    within = 64.0 * P * var - float((64.0 * off * off).sum())
    assert var > 0 and within >= 0, "the block spread alone exceeds the variance asked for"
    t = torch.full((tokens, (P + 1) & ~1, 2), pad, dtype=F64)
    t[:, :P, 0] = 64.0 * (mean + off)
    t[:, :P, 1] = within / P
    return t


def merge(table, P, eps):
    """(m, r) per token: the float64 Chan merge of the first P blocks of `table` (any float dtype), eps rounded to fp32."""
    s, q = table[:, :P, 0].to(F64), table[:, :P, 1].to(F64)
    n = 64.0 * P
    m = s.sum(1) / n
    dm = s / 64.0 - m[:, None]
    var = (q + 64.0 * dm * dm).sum(1) / n
    return m, (var + float(torch.tensor(eps, dtype=torch.float32))).rsqrt()


def guard_flags(table, P, eps, tokens):
    """The flags a consumer launch over the first `tokens` rows of the table must raise."""
    m, r = merge(table[:tokens], P, eps)
    return GUARD_OFFSET if bool(((m * r).abs() > GUARD_RATIO).any()) else 0


def _coeff_bars(table, P, eps):
    """(m, r, e_m, e_r, e_mr) per token: section 2 of the derivation."""
    s, q = table[:, :P, 0].to(F64), table[:, :P, 1].to(F64)
    n, g1 = 64.0 * P, gamma_n(P + 1)
    m, r = merge(table, P, eps)
    e_m = g1 * s.abs().sum(1) / n
    dm = (s / 64.0 - m[:, None]).abs()
    e_dm = e_m[:, None] * (1 + U) + U * dm
    t = 64.0 * dm * dm + q
    e_M2 = (1 + g1) * (128.0 * dm * e_dm + 64.0 * e_dm * e_dm).sum(1) + g1 * t.sum(1)
    v = r ** -2
    var = t.sum(1) / n
    e_var = e_M2 / n + U * (var + e_M2 / n)
    e_v = e_var + U * (v + e_var)
    rho = e_v / v
    e_r = r * ((1 + RSQ_REL) * (1 + rho / (2 * (1 - rho))) - 1)
    mr_hi = (m.abs() + e_m) * (r + e_r)
    e_mr = mr_hi - m.abs() * r + U * mr_hi
    return m, r, e_m, e_r, e_mr


def _linear(x, w, c, d, bias, table, eps, mode):
    """(value, bar before the output rounding) in the token-major layout [tokens, rows of w]; bias is [rows] in mode 1, [tokens] in mode 2."""
    x, w, c, d = x.to(F64), w.to(F64), c.to(F64), d.to(F64)
    K = x.shape[1]
    m, r, _, e_r, e_mr = _coeff_bars(table, K // 64, eps)
    m, r, e_r, e_mr = m[:, None], r[:, None], e_r[:, None], e_mr[:, None]
    acc = x @ w.t()
    e_acc = gamma_n(K) * (x.abs() @ w.abs().t())
    b = torch.zeros((), dtype=F64, device=x.device) if bias is None else (bias.to(F64)[None, :] if mode == 1 else bias.to(F64)[:, None])
    val = r * acc - (m * r) * c[None, :] + d[None, :] + b
    racc, mrc, db = (r + e_r) * (acc.abs() + e_acc), (m.abs() * r + e_mr) * c.abs()[None, :], d.abs()[None, :] + b.abs()
    bar = (r + e_r) * e_acc + acc.abs() * e_r + c.abs()[None, :] * e_mr
    bar = bar + U * ((db if bias is not None else 0.0) + (racc + db) + mrc + (racc + mrc + db))
    return val, bar


def _round_bar(val, bar, out_f32):
    mag = val.abs() + bar
    return bar + (U * mag if out_f32 else torch.clamp(2.0 ** -11 * mag, min=2.0 ** -25))


def geglu_columns(N, device=None):
    """(value columns, gate columns) of the interleaved layout, in output-column order."""
    j = torch.arange(N // 2, device=device)
    v = (j // 32) * 64 + j % 32
    return v, v + 32


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def fold_model(x, w, c, d, bias, table, eps, mode, geglu=False, out_f32=False):
    """(ref, bar), both float64 in the layout of the kernel's output: [tokens, N] (mode 1), [rows, tokens] (mode 2), [tokens, N / 2] (GEGLU).
    x [tokens, K] and w [rows, K] are the operands as the MFMAs see them (fp16 in the GPU tests; float64 x and unrounded weights make `ref` the
    LayerNorm -> Linear itself), c, d [rows], bias [N] or None, table [>= tokens, P rounded up to even, 2] as the kernel reads it."""
    assert mode in (1, 2) and not (geglu and mode == 2)
    val, bar = _linear(x, w, c, d, bias, table[:x.shape[0]], eps, mode)
    if geglu:
        iv, ig = geglu_columns(w.shape[0], x.device)
        v, g, e_v, e_g = val[:, iv], val[:, ig], bar[:, iv], bar[:, ig]
        G = gelu_erf(g)
        e_G = GELU_LIP * e_g + 0.5 * (g.abs() + e_g) * GELU_EVAL + U * (g.abs() + e_g)
        val = v * G
        bar = e_v * (G.abs() + e_G) + v.abs() * e_G + U * (v.abs() + e_v) * (G.abs() + e_G)
    bar = _round_bar(val, bar, out_f32)
    return (val, bar) if mode == 1 else (val.t(), bar.t())


# ------------------------------------------------------------------------------- the same formula in fp32 (the CPU emulation of the kernel)
def coeffs_fp32(table, P, eps):
    """(mean * rstd, rstd) per token in fp32 with the operation order of ln_token_coeffs: sequential sum, division, fma-free Chan terms."""
    f = torch.float32
    t = table.to(f)
    n = torch.tensor(64.0 * P, dtype=f)
    tot = torch.zeros(t.shape[0], dtype=f)
    for q in range(P):
        tot = tot + t[:, q, 0]
    mean = tot / n
    m2 = torch.zeros_like(tot)
    for q in range(P):
        dm = t[:, q, 0] * f32(1.0 / 64.0) - mean
        m2 = m2 + ((64.0 * dm) * dm + t[:, q, 1])
    r = torch.rsqrt(m2 / n + f32(eps))
    return mean * r, r


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def eval_fp32(x16, w16, c, d, bias, table, eps, mode, geglu=False, out_f32=False):
    """The kernel's arithmetic in torch fp32: fp32 matmul of the fp16 operands, coeffs_fp32, the epilogue's operation order, one output rounding."""
    f = torch.float32
    mr, r = coeffs_fp32(table[:x16.shape[0]], x16.shape[1] // 64, eps)
    acc = x16.to(f) @ w16.to(f).t()
    b = 0.0 if bias is None else (bias.to(f)[None, :] if mode == 1 else bias.to(f)[:, None])
    val = (r[:, None] * acc + (d.to(f)[None, :] + b)) - mr[:, None] * c.to(f)[None, :]
    if geglu:
        iv, ig = geglu_columns(w16.shape[0])
        val = val[:, iv] * torch.nn.functional.gelu(val[:, ig])
    val = val if out_f32 else val.to(torch.float16)
    return val if mode == 1 else val.t()
