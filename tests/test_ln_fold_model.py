"""tests/ln_fold_model.py checked against itself, without a GPU, at every (M, N, K, mode) tests/test_layernorm_fold_edges_gpu.py launches:
the formula is the operation (float64 LayerNorm -> Linear to 1e-12), an fp32 evaluation of it stays inside the derived bar, and the helper
behind the hand-made tables delivers the mean and sigma it is asked for."""
import pytest
import torch
import torch.nn.functional as F

import ln_fold_model as L

F16, F32, F64 = torch.float16, torch.float32, torch.float64
SHAPES = L.all_shapes()
WORST = {False: 0.0, True: 0.0}


def _operands(M, N, K, mode, seed=0):
    """x [tokens, K], w [rows, K], gamma, beta, linear bias [rows] in float64."""
    g = torch.Generator().manual_seed(seed)
    tokens, rows = (M, N) if mode == 1 else (N, M)
    x = L.make_tokens(tokens, K, seed + 1)
    w = torch.randn(rows, K, generator=g, dtype=F64) * K ** -0.5
    gamma = 1.0 + 0.3 * torch.randn(K, generator=g, dtype=F64)
    beta = 0.3 * torch.randn(K, generator=g, dtype=F64)
    b = torch.randn(rows, generator=g, dtype=F64)
    return x, w, gamma, beta, b, tokens


def test_the_shape_list_is_what_the_issue_names():
    assert len(SHAPES) == len(set(SHAPES)) and all(K % 64 == 0 and N % 8 == 0 for _, N, K, _, _ in SHAPES)
    assert {(M, N) for M, N, K, mode, g in SHAPES if g} == {(M, N) for M in (1, 63, 65) for N in (128, 192)}
    assert {K // 64 for M, N, K, mode, g in SHAPES if (M, N) == (65, 72)} >= {1, 2, 3, 19, 20}
    for bm, bn, _ in L.ALL_TILES:
        assert (bm + 1, bn + 8, 320, 1, False) in SHAPES and (bm + 8, bn + 8, 320, 2, False) in SHAPES and (1, 8, 320, 1, False) in SHAPES


@pytest.mark.parametrize("M,N,K,mode,geglu", SHAPES)
def test_model_is_layernorm_then_linear(M, N, K, mode, geglu):
    """Float64 x, unrounded gamma (.) W, exact c and d, the exact table: `ref` is F.layer_norm -> linear (-> GEGLU) to 1e-12."""
    x, w, gamma, beta, b, tokens = _operands(M, N, K, mode)
    eps = 1e-5
    eps32 = float(torch.tensor(eps, dtype=F32))                 # the model rounds eps to fp32 as the descriptor does
    wf = w * gamma[None]
    ref, _ = L.fold_model(x, wf, wf.sum(1), w @ beta + b, None, L.table_from_x(x), eps, mode, geglu=geglu, out_f32=True)
    want = F.layer_norm(x, (K,), gamma, beta, eps32) @ w.t() + b
    if geglu:
        iv, ig = L.geglu_columns(N)
        want = want[:, iv] * F.gelu(want[:, ig])
    want = want if mode == 1 else want.t()
    assert ref.shape == want.shape
    assert float((ref - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("M,N,K,mode,geglu", SHAPES)
def test_fp32_evaluation_stays_inside_the_bar(M, N, K, mode, geglu):
    """fp16 operands, the fp32-rounded table, torch fp32 for the matmul, the merge and the epilogue: inside `bar` for both output types."""
    x, w, gamma, beta, b, tokens = _operands(M, N, K, mode, seed=7)
    x16, wf = x.to(F16), (w * gamma[None]).to(F16)
    c, d = wf.float().sum(1), (w @ beta + b).float()
    table = L.table_from_x(x16).float()
    bias = torch.randn(N, generator=torch.Generator().manual_seed(3)).to(F16) if (M + N) % 16 else None
    for out_f32 in (True, False):
        ref, bar = L.fold_model(x16, wf, c, d, bias, table, 1e-5, mode, geglu=geglu, out_f32=out_f32)
        got = L.eval_fp32(x16, wf, c, d, bias, table, 1e-5, mode, geglu=geglu, out_f32=out_f32)
        ratio = float(((got.double() - ref).abs() / bar).max())
        WORST[geglu] = max(WORST[geglu], ratio)
        print(f"M={M} N={N} K={K} mode {mode}{' GEGLU' if geglu else ''} {'fp32' if out_f32 else 'fp16'} out: worst |err| / bar {ratio:.3f}"
              f"   (so far: linear {WORST[False]:.3f}, GEGLU {WORST[True]:.3f})")
        assert ratio <= 1.0


@pytest.mark.parametrize("P", L.PARTS_B)
@pytest.mark.parametrize("mean,ratio,spread", [(15.5, 15.5, 0.0), (-16.5, 16.5, 0.0), (3.0, 15.5, 0.01), (1000.0, 1000.0, 0.0), (0.0, None, 0.05)])
@pytest.mark.parametrize("eps", [1e-5, 1e-6, 1e-3])
def test_handmade_table_has_the_mean_and_sigma_asked_for(P, mean, ratio, spread, eps):
    t = L.handmade_table(3, P, mean, ratio, eps, spread)
    m, r = L.merge(t, P, eps)
    eps32 = float(torch.tensor(eps, dtype=F32))
    want = (1.0 + eps32) ** 0.5 if ratio is None else abs(mean) / ratio          # 1 / r = sqrt(sigma^2 + eps)
    assert float((m - mean).abs().max()) <= 1e-12 * max(1.0, abs(mean)) and float((1.0 / r - want).abs().max()) <= 1e-12 * want
    # rounded to fp32 (what the kernel reads) the ratio moves by a few 2^-24, far inside the 3 % the guard cases keep from the threshold
    m32, r32 = L.merge(t.float(), P, eps)
    if ratio is not None:
        assert float(((m32 * r32).abs() / ratio - 1).abs().max()) <= 1e-5
        assert L.guard_flags(t.float(), P, eps, 3) == (L.GUARD_OFFSET if ratio > L.GUARD_RATIO else 0)
    assert P % 2 == 0 or bool(torch.isnan(t[:, P:]).all())


def test_table_from_x_and_block_means_far_apart():
    """table_from_x is the two-pass definition; the +-100 tokens of the GPU file's group C: the between-block term is ~100x the within-block one."""
    P = 5
    x = L.make_tokens(4, 64 * P, 5, block_means=[100.0, -100.0, 100.0, -100.0, 100.0], block_sigmas=1.0).to(F16)
    t = L.table_from_x(x)
    m, r = L.merge(t, P, 1e-5)
    xd = x.double()
    assert float((m - xd.mean(1)).abs().max()) <= 1e-12 * 100 and float((r - (xd.var(1, unbiased=False) + float(torch.tensor(1e-5))).rsqrt()).abs().max()) <= 1e-12
    within = t[:, :P, 1].sum(1)
    assert float((64 * P / r ** 2 / within).min()) > 50


def test_guard_flags_looks_at_the_first_tokens_only():
    t = torch.cat([L.handmade_table(4, 5, 15.5, 15.5, 1e-5), L.handmade_table(2, 5, 1000.0, 1000.0, 1e-5)]).float()
    assert L.guard_flags(t, 5, 1e-5, 4) == 0 and L.guard_flags(t, 5, 1e-5, 5) == L.GUARD_OFFSET
