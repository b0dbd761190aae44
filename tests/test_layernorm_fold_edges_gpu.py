"""The CONSUMER side of the LayerNorm fold (sg_gemm_desc.ln_mode; ln_token_coeffs and the ln branches of epi_finish in
storygen_amd/csrc/gemm_conv.hip) on every tile of every kernel family and at its guard edges.  tests/test_gemm_conv_edges_gpu.py holds the
producer side (ln_stats_out); here every launch passes ln=.

Reference and bar: tests/ln_fold_model.py — float64 on the same fp16 operands and on the fp32 table as the kernel reads it, with a derived
per-element bar (its docstring; nothing in it is fitted to a kernel's output) and the guard flags the documented rule gives.

Every case: `a`, `w` and the output are interior windows of NaN- / sentinel-filled buffers (helpers of tests/test_gemm_conv_edges_gpu.py), the
stats table — contiguous by contract — sits between a sentinel band and 512 rows of |mean| / sigma = 1e3 entries (a token index that escapes
the clamp raises SG_LN_GUARD_OFFSET), the padding block of an odd ln_parts is NaN, use_table=False, the plan query must name the hinted
family and tile, three launches must agree bit for bit, and the worst ratio to the bar is printed (`-s`).

 A  every tile (six pipeline, two latency, two fat), both modes, tails in M and N, K = 320 (P = 5), bias on half, fp16 and fp32 outputs
 B  ln_parts 1, 2, 3, 19, 20 on the 64x64 pipeline and latency tiles
 C  tables of hand-made tokens: block means +-100, an all-zero token (= the rounding of d + bias, bit for bit), two identical tokens in
    different tiles and strips (equal bits), eps 1e-5 / 1e-6 / 1e-3
 D  GEGLU on the fold: six pipeline and two fat tiles; the latency hint falls back to the heuristic
 E  gemm_pair (mode 1 q|k problem + mode 2 V^T problem) = the two single launches, bit for bit, in ONE launch
 F  the guard: |mean| / sigma = 15.5 / 16.5 at token 0 and at the last token of a tail tile, on all four epilogue forms; sticky; never RANGE
 G  refusals before any launch
 H  producer -> consumer chains (fused and split-K producer; pipeline and latency consumer) against float64 LayerNorm -> Linear

Figures of the first hardware run: profiles/r28a_layernorm_fold_edge_tests.txt."""
import functools

import pytest
import torch
import torch.nn.functional as F

import ln_fold_model as L
from conftest import max_rel, rel_l2
from test_gemm_conv_edges_gpu import (F16, F32, SENT16, SENT32, _assert_bar, _bits, _guards_intact, _nan_fenced, _nan_window, _out_window, _randn,
                                      _sent, _untouched, _workspace)

pytestmark = pytest.mark.gpu
AFTER = 512                      # table rows behind the last token: at least one tile height of any family
BEFORE = 4
RANGE, OFFSET = 1, 2


# ------------------------------------------------------------------------------------------------------------------------- helpers
def _hint(tile):
    return tile[:2] if tile[2] == 0 else tile


def _assert_plan(what, plan, tile):
    bm, bn, waves = tile
    family = plan[5] == 1 if waves == 0 else plan[5] >= 16 if tile in L.LAT_TILES else plan[5] == 2
    assert family and plan[:2] == (bm, bn) and plan[2] == 1, f"{what}: planned as {plan}, not on the hinted tile {tile}"


def _table_buffer(table, dev):
    """(buffer, view): the fp32 table [tokens, P2, 2] behind BEFORE sentinel rows and in front of AFTER rows of |mean| / sigma = 1e3 entries."""
    tokens, P2, _ = table.shape
    after = torch.empty(AFTER, P2, 2, dtype=F32)
    after[..., 0], after[..., 1] = 64.0e3, 64.0
    buf = torch.cat([_sent((BEFORE, P2, 2), F32, "cpu"), table.to(F32).cpu(), after]).to(dev)
    return buf, buf[BEFORE:BEFORE + tokens]


class _Problem:
    """Operands of one folded GEMM, each in its window; the float64 model is evaluated on demand (bias, eps and output type vary per case)."""
    def __init__(self, tokens, rows, K, mode, geglu=False, x=None, table=None, seed=0):
        dev = torch.device("cuda:0")
        self.tokens, self.rows, self.K, self.mode, self.geglu = tokens, rows, K, mode, geglu
        x = L.make_tokens(tokens, K, 100 + seed) if x is None else x
        self.x = x.to(F16).to(dev)
        self.w = _randn((rows, K), dev, 200 + seed, scale=K ** -0.5)
        self.c = self.w.float().sum(1)
        self.d = _randn((rows,), dev, 300 + seed, F32)
        self.N = rows if mode == 1 else tokens
        self.M = tokens if mode == 1 else rows
        self.bias = _randn((self.N,), dev, 400 + seed)
        self.table = (L.table_from_x(self.x.cpu()) if table is None else table).float()
        self.tbuf, self.tview = _table_buffer(self.table, dev)
        self.tbits = _bits(self.tbuf).clone()
        self.xv, self.wv, self.cv, self.dv, self.bv = _nan_window(self.x), _nan_window(self.w), _nan_fenced(self.c), _nan_fenced(self.d), _nan_fenced(self.bias)
        self.a, self.b = (self.xv, self.wv) if mode == 1 else (self.wv, self.xv)

    @functools.lru_cache(maxsize=None)
    def model(self, bias, eps, out_f32):
        return L.fold_model(self.x, self.w, self.c, self.d, self.bias if bias else None, self.table.to(self.x.device), eps, self.mode,
                            geglu=self.geglu, out_f32=out_f32)

    def out_shape(self):
        return (self.M, self.N // 2 if self.geglu else self.N)

    def kwargs(self, bias, eps, tile, guard):
        from storygen_amd import ops
        kw = dict(ln=(self.mode, self.tview, self.cv, self.dv, eps), use_table=False, guard=guard)
        if tile is not None:
            kw["tile"] = _hint(tile)
        if bias:
            kw["bias"] = self.bv
        if self.geglu:
            kw["epilogue"] = ops.EPI_GEGLU
        return kw


@functools.lru_cache(maxsize=None)
def _problem(tokens, rows, K, mode, geglu=False):
    return _Problem(tokens, rows, K, mode, geglu)


def _run_fold(what, p, tile, *, bias=False, out_f32=False, eps=1e-5, guard_init=0, use_guard=True, want_plan=True, want_flags=None):
    """Three launches of one folded GEMM; checks the plan, the windows, the table, repeatability, the bar and the guard flags.  Returns
    (output view, plan)."""
    from storygen_amd import ops
    dev = p.x.device
    obuf, out, oidx = _out_window(p.out_shape(), F32 if out_f32 else F16, dev)
    guard = torch.full((1,), guard_init, dtype=torch.int32, device=dev) if use_guard else None
    kw = p.kwargs(bias, eps, tile, guard)
    plan = ops.gemm_launch_plan(p.a, p.b, out, **kw)
    if want_plan:
        _assert_plan(what, plan, tile)
    first = None
    for _ in range(3):
        _bits(obuf).fill_(SENT32 if out_f32 else SENT16)
        ops.gemm(p.a, p.b, out, **kw)
        torch.cuda.synchronize()
        got = _bits(out).clone()
        first = got if first is None else first
        assert torch.equal(got, first), f"{what}: repeats differ bit-wise"
    _guards_intact(f"{what}: out", obuf, oidx)
    assert torch.equal(_bits(p.tbuf), p.tbits), f"{what}: the stats table or its bands were written"
    ref, bar = p.model(bias, eps, out_f32)
    _assert_bar(what, out, ref, bar, plan, p.K)
    if use_guard:
        want = L.guard_flags(p.table, p.K // 64, eps, p.tokens) if want_flags is None else want_flags
        flags = int(guard.item())
        assert flags == (guard_init | want), f"{what}: guard flags {flags}, expected {guard_init | want} (before the launch: {guard_init})"
    return out, plan


# -------------------------------------------------------------------------------------------------- A. every tile, both modes, tails
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("tile", L.ALL_TILES, ids=lambda t: f"{t[0]}x{t[1]}w{t[2]}")
def test_every_tile_both_modes_tails(gpu, tile, mode):
    for i, (M, N) in enumerate(L.shapes_a(tile[0], tile[1], mode)):
        tokens, rows = (M, N) if mode == 1 else (N, M)
        what = f"A tile {tile} mode {mode} M={M} N={N} {'fp32' if i % 2 == 0 else 'fp16'} out{', bias' if (i // 2) % 2 == 0 else ''}"
        _run_fold(what, _problem(tokens, rows, L.K_A, mode), tile, bias=(i // 2) % 2 == 0, out_f32=i % 2 == 0)


# ------------------------------------------------------------------------------------------------------------- B. ln_parts sweep
@pytest.mark.parametrize("P", L.PARTS_B)
@pytest.mark.parametrize("tile", [(64, 64, 0), (64, 64, 4)], ids=["pipe64x64", "lat64x64"])
def test_ln_parts_sweep(gpu, tile, P):
    M, N = L.MN_B
    for out_f32 in (True, False):
        _run_fold(f"B tile {tile} P={P} {'fp32' if out_f32 else 'fp16'} out", _problem(M, N, 64 * P, 1), tile, bias=not out_f32, out_f32=out_f32)


# ------------------------------------------------------------------------------------------------------------ C. hand-made tokens
C_TILES = [(64, 64, 0), (64, 64, 4), (512, 128, 8)]


@functools.lru_cache(maxsize=None)
def _far_apart_problem(mode):
    x = L.make_tokens(72, L.K_A, 11, block_means=[100.0, -100.0, 100.0, -100.0, 100.0], block_sigmas=1.0)
    return _Problem(72, 72, L.K_A, mode, x=x, seed=11)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("tile", C_TILES, ids=lambda t: f"{t[0]}x{t[1]}w{t[2]}")
def test_block_means_far_apart(gpu, tile, mode):
    """Blocks at +-100 with sigma 1 inside: the token's variance is the between-block term 64 dm^2 almost alone."""
    for out_f32 in (True, False):
        _run_fold(f"C far-apart tile {tile} mode {mode} {'fp32' if out_f32 else 'fp16'} out", _far_apart_problem(mode), tile, bias=out_f32, out_f32=out_f32)


ZERO_ROWS, TWIN = (7, 128), (5, 101)         # 128: alone in the tail tile of a 64- or 128-row tiling; 5 / 101: strips 0 and 2 of tiles 0 and 1


@functools.lru_cache(maxsize=None)
def _special_problem():
    x = L.make_tokens(130, L.K_A, 12)
    x[list(ZERO_ROWS)] = 0.0
    x[TWIN[1]] = x[TWIN[0]]
    return _Problem(130, 72, L.K_A, 1, x=x, seed=12)


@pytest.mark.parametrize("tile", C_TILES + [(128, 64, 0)], ids=lambda t: f"{t[0]}x{t[1]}w{t[2]}")
def test_zero_token_and_identical_tokens(gpu, tile):
    p = _special_problem()
    for out_f32 in (True, False):
        for bias in (True, False):
            what = f"C special tile {tile} {'fp32' if out_f32 else 'fp16'} out{', bias' if bias else ''}"
            out, _ = _run_fold(what, p, tile, bias=bias, out_f32=out_f32)
            # acc = 0, mean = 0: fma(r, 0, d + bias) - 0 c is the fp32 sum d + bias itself, then the one output rounding
            want = (p.d + (p.bias.float() if bias else 0.0)).to(out.dtype)
            for r in ZERO_ROWS:
                assert torch.equal(_bits(out[r]), _bits(want)), f"{what}: the all-zero token {r} is not the rounding of d + bias"
            assert torch.equal(_bits(out[TWIN[0]]), _bits(out[TWIN[1]])), f"{what}: identical tokens {TWIN} differ"


@pytest.mark.parametrize("eps", [1e-5, 1e-6, 1e-3])
@pytest.mark.parametrize("tile", C_TILES[:2], ids=["pipe64x64", "lat64x64"])
def test_eps(gpu, tile, eps):
    for mode in (1, 2):
        p = _special_problem() if mode == 1 else _problem(72, 72, L.K_A, 2)
        _run_fold(f"C eps={eps:g} tile {tile} mode {mode}", p, tile, bias=True, out_f32=True, eps=eps)


# ------------------------------------------------------------------------------------------------------------ D. GEGLU on the fold
@pytest.mark.parametrize("tile", [t + (0,) for t in L.PIPE_TILES] + L.FAT_TILES, ids=lambda t: f"{t[0]}x{t[1]}w{t[2]}")
def test_geglu_on_the_fold(gpu, tile):
    i = 0
    for N in L.GEGLU_N:
        for M in L.GEGLU_M:
            _run_fold(f"D GEGLU tile {tile} M={M} N={N} {'fp32' if i % 3 == 0 else 'fp16'} out", _problem(M, N, L.K_A, 1, True), tile, bias=i % 2 == 0, out_f32=i % 3 == 0)
            i += 1


@pytest.mark.parametrize("lat", L.LAT_TILES, ids=["lat64x64", "lat64x128"])
def test_geglu_latency_hint_falls_back_to_the_heuristic(gpu, lat):
    """The latency kernel has the linear epilogue only: its hint on a GEGLU launch is answered as if no tile had been asked for."""
    from storygen_amd import ops
    for N in L.GEGLU_N:
        for M in L.GEGLU_M:
            p = _problem(M, N, L.K_A, 1, True)
            out, plan = _run_fold(f"D GEGLU hint {lat} M={M} N={N}", p, lat, bias=True, want_plan=False)
            unhinted = ops.gemm_launch_plan(p.a, p.b, out, **p.kwargs(True, 1e-5, None, None))
            assert plan == unhinted and plan[5] == 1, f"latency hint on GEGLU: plan {plan}, without a hint {unhinted}"


# ---------------------------------------------------------------------------------------------------------------- E. gemm_pair
@pytest.mark.parametrize("tile", [(64, 64, 0), (128, 64, 0), (64, 64, 4)], ids=["pipe64x64", "pipe128x64", "lat64x64"])
def test_pair_is_the_two_single_launches(gpu, tile):
    from storygen_amd import ops
    tokens, nqk, rows = L.MN_E
    x = L.make_tokens(tokens, L.K_A, 13)
    p0, p1 = _Problem(tokens, nqk, L.K_A, 1, x=x, seed=13), _Problem(tokens, rows, L.K_A, 2, x=x, seed=14)
    singles = [_run_fold(f"E single[{i}] tile {tile}", p, tile, bias=i == 0)[0] for i, p in enumerate((p0, p1))]
    outs = [_out_window(p.out_shape(), F16, gpu) for p in (p0, p1)]
    guard = torch.zeros(1, dtype=torch.int32, device=gpu)
    kw0, kw1 = p0.kwargs(True, 1e-5, tile, guard), p1.kwargs(False, 1e-5, None, guard)
    kw0.pop("use_table"), kw1.pop("use_table")
    args = ((p0.a, p0.b, outs[0][1]), kw0), ((p1.a, p1.b, outs[1][1]), kw1)
    pplan = ops.gemm_pair_launch_plan(*args)
    assert pplan[0] == 1 and pplan[1:3] == pplan[7:9] == tile[:2] and pplan[6] == pplan[12], f"pair on tile {tile}: not one launch, plan {pplan}"
    assert (pplan[6] >= 16) == (tile[2] == 4)
    for _ in range(3):
        for obuf, _, _ in outs:
            _bits(obuf).fill_(SENT16)
        ops.gemm_pair(*args)
        torch.cuda.synchronize()
        for i, (obuf, out, oidx) in enumerate(outs):
            _guards_intact(f"E pair[{i}] tile {tile}", obuf, oidx)
            assert torch.equal(_bits(out), _bits(singles[i])), f"E pair[{i}] tile {tile}: differs from the single launch"
    assert int(guard.item()) == 0


# -------------------------------------------------------------------------------------------------------------------- F. the guard
# form -> (tile, mode, GEGLU): the row-quad form, the GEGLU branch, the 16-row strips, the two 64-row halves
FORMS = {"pipe64x64-m1": ((64, 64, 0), 1, False), "pipe64x64-m2": ((64, 64, 0), 2, False), "geglu128x64": ((128, 64, 0), 1, True),
         "lat64x64-m1": ((64, 64, 4), 1, False), "lat64x64-m2": ((64, 64, 4), 2, False), "fat512x128-m1": ((512, 128, 8), 1, False),
         "fat512x128-m2": ((512, 128, 8), 2, False)}


def _guard_problem(form, where, ratio):
    """tokens = one tile and a tail; every token at |mean| / sigma = 4 but the one at `where` (0 or the last)."""
    tile, mode, geglu = FORMS[form]
    tokens = tile[0] + 1 if mode == 1 else tile[1] + 8
    rows = 128 if geglu else 72
    table = L.handmade_table(tokens, 5, 4.0, 4.0, 1e-5, spread=0.1)
    at = 0 if where == "first" else tokens - 1
    table[at] = L.handmade_table(1, 5, -ratio if where == "first" else ratio, ratio, 1e-5, spread=0.1)[0]
    return _Problem(tokens, rows, L.K_A, mode, geglu, table=table, seed=15), tile


@pytest.mark.parametrize("ratio", [15.5, 16.5])
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("form", list(FORMS))
def test_guard_threshold(gpu, form, where, ratio):
    """3 % either side of SG_LN_GUARD_RATIO = 16, far beyond any fp32 or rsqrt rounding; the 1e3 rows behind the table must not be seen; a RANGE
    bit set before the launch survives and the consumer sets none."""
    p, tile = _guard_problem(form, where, ratio)
    want = OFFSET if ratio > 16 else 0
    assert L.guard_flags(p.table, 5, 1e-5, p.tokens) == want
    _run_fold(f"F {form} {where} token at ratio {ratio}", p, tile, bias=True, want_flags=want)
    _run_fold(f"F {form} {where} token at ratio {ratio}, RANGE set before", p, tile, guard_init=RANGE, want_flags=want)


@pytest.mark.parametrize("form", list(FORMS))
def test_guard_is_sticky_optional_and_sees_a_constant_token(gpu, form):
    tile, mode, geglu = FORMS[form]
    clean, _ = _guard_problem(form, "last", 15.5)
    _run_fold(f"F {form} clean launch on set flags", clean, tile, guard_init=RANGE | OFFSET, want_flags=0)
    _run_fold(f"F {form} without a guard", clean, tile, use_guard=False)
    _run_fold(f"F {form} without a guard, offending token", _guard_problem(form, "last", 16.5)[0], tile, use_guard=False)
    x = L.make_tokens(clean.tokens, L.K_A, 16)
    x[clean.tokens - 1] = 2.0                   # constant, non-zero: sigma = 0, |mean| r = 2 / sqrt(eps)
    p = _Problem(clean.tokens, clean.rows, L.K_A, mode, geglu, x=x, seed=16)
    _run_fold(f"F {form} constant token", p, tile, want_flags=OFFSET)


# -------------------------------------------------------------------------------------------------------------------- G. refusals
def _refused(what, match, p, out_shape=None, **over):
    from storygen_amd import ops
    dev = p.x.device
    obuf, out, _ = _out_window(out_shape or p.out_shape(), F16, dev)
    guard = torch.zeros(1, dtype=torch.int32, device=dev)
    kw = p.kwargs(False, 1e-5, None, guard)
    a, b = over.pop("a", p.a), over.pop("b", p.b)
    kw.update(over)
    with pytest.raises(RuntimeError, match=match):
        ops.gemm(a, b, out, **kw)
    torch.cuda.synchronize()
    _untouched(f"{what}: output", obuf)
    assert torch.equal(_bits(p.tbuf), p.tbits) and int(guard.item()) == 0, f"{what}: table or guard written by a refused launch"


def test_refusals_before_any_launch(gpu):
    from storygen_amd import ops
    M, N = 72, 72
    p = _problem(M, N, L.K_A, 1)
    wsbuf, ws = _workspace(ops.gemm_workspace_bytes(M, N, 2), gpu)
    _refused("P = 21", "ln_parts", _problem(M, N, 64 * 21, 1))
    _refused("split_k = 2", "does not split K", p, split_k=2, workspace=ws)
    assert bool((ws == 0xFF).all())
    sbuf = _sent((2 * N,), F32, gpu)
    _refused("stats", "excludes stats", p, stats=(sbuf, M))
    _untouched("stats buffer", sbuf)
    _refused("rowbias", "excludes stats, rowbias", p, rowbias=_randn((1, N), gpu, 1, F32), rows_per_batch=M)
    _refused("res1", "excludes stats, rowbias and residuals", p, res1=_randn((M, N), gpu, 2))
    _refused("res2", "excludes stats, rowbias and residuals", p, res2=_randn((M, N), gpu, 3, F32))
    p2 = _problem(128, 72, L.K_A, 2)                                         # tokens N = 128 = N % 64 == 0, as GEGLU demands
    _refused("mode 2 + GEGLU", "ln_mode 2 needs the linear epilogue", p2, out_shape=(72, 64), epilogue=ops.EPI_GEGLU)
    cbuf = torch.zeros(N + 8, dtype=F32, device=gpu)
    _refused("ln_c + 4 bytes", "alignment", p, ln=(1, p.tview, cbuf[1:1 + N], p.dv, 1e-5))
    _refused("ln_d + 4 bytes", "alignment", p, ln=(1, p.tview, p.cv, cbuf[1:1 + N], 1e-5))
    p4 = _Problem(12, 72, L.K_A, 2)                                          # tokens = N = 12: the first N the multiple-of-8 check turns away
    obuf = _sent((72 + 6, 32), F16, gpu)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ops.gemm(p4.a, p4.b, obuf[3:75, 8:20], ln=(2, p4.tview, p4.cv, p4.dv, 1e-5), use_table=False)
    torch.cuda.synchronize()
    _untouched("N = 12", obuf)


def test_first_token_count_beyond_the_32_bit_offsets_is_refused(gpu):
    """Mode 2: the tokens are the rows of W.  With ldw = 65536 the last admitted N is 32768 ((N - 1) ldw + K <= 2^31); N = 32776, the next valid
    one, is turned away by the descriptor check with the table, the output and the guard untouched."""
    from storygen_amd import ops
    K, M, ldw = 64, 8, 65536
    N = (2 ** 31 - K) // ldw + 1 + 8
    assert (N - 9) * ldw + K <= 2 ** 31 < (N - 1) * ldw + K
    buf = torch.empty((N, ldw), dtype=F16, device=gpu)                      # 4 GiB + 1 MiB, never filled nor read
    try:
        tbuf = _sent((N, 2, 2), F32, gpu)
        obuf, out, _ = _out_window((M, N), F16, gpu)
        guard = torch.zeros(1, dtype=torch.int32, device=gpu)
        w, cd = _randn((M, K), gpu, 1), torch.zeros(M, dtype=F32, device=gpu)
        with pytest.raises(RuntimeError, match=r"operand W spans .*2\^31 elements"):
            ops.gemm(w, buf[:, :K], out, ln=(2, tbuf, cd, cd, 1e-5), guard=guard, use_table=False)
        torch.cuda.synchronize()
        _untouched("output", obuf), _untouched("table", tbuf)
        assert int(guard.item()) == 0
    finally:
        del buf
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ H. one chain per producer kind
H_L2, H_MAX = 1.5e-3, 2.0e-2        # tests/test_kernels_gpu.py::test_gemm_layernorm_fold's own bar (it carries the fp16 rounding of x)


@pytest.mark.parametrize("tile", [(64, 64, 0), (64, 64, 4)], ids=["pipe-consumer", "lat-consumer"])
@pytest.mark.parametrize("split", [1, 2], ids=["fused-producer", "splitk2-producer"])
def test_chain_producer_to_consumer(gpu, split, tile):
    from storygen_amd import ops
    from storygen_amd.repack import fold_layernorm
    M, C = L.MN_H
    P = C // 64
    a0, w0 = _randn((M, C), gpu, 21), _randn((C, C), gpu, 22, scale=C ** -0.5)
    res = _randn((M, C), gpu, 23, F32) + 3.0
    x, x16 = torch.empty(M, C, dtype=F32, device=gpu), torch.empty(M, C, dtype=F16, device=gpu)
    st = torch.full((M, (P + 1) & ~1, 2), float("nan"), dtype=F32, device=gpu)
    ws = torch.empty(ops.gemm_workspace_bytes(M, C, 2), dtype=torch.uint8, device=gpu)
    plan = ops.gemm_launch_plan(a0, w0, x, bias=_randn((C,), gpu, 24), res1=res, out2=x16, ln_out=st, split_k=split, workspace=ws, use_table=False)
    assert plan[2] == split
    ops.gemm(a0, w0, x, bias=_randn((C,), gpu, 24), res1=res, out2=x16, ln_out=st, split_k=split, workspace=ws, use_table=False)
    assert bool(torch.isnan(st[:, P:]).all()) and bool(torch.isfinite(st[:, :P]).all()), "the producer fills P blocks and leaves the padding block alone"
    gamma, beta = _randn((C,), gpu, 25, scale=0.3) + 1.0, _randn((C,), gpu, 26, scale=0.3)
    wq, bq = _randn((2 * C, C), gpu, 27, scale=C ** -0.5), _randn((2 * C,), gpu, 28)
    wf, c, d = fold_layernorm(wq, bq, gamma, beta)
    out = torch.full((M, 2 * C), float("nan"), dtype=F16, device=gpu)
    guard = torch.zeros(1, dtype=torch.int32, device=gpu)
    kw = dict(ln=(1, st, c, d, 1e-5), guard=guard, tile=_hint(tile), use_table=False)
    _assert_plan("H consumer", ops.gemm_launch_plan(x16, wf, out, **kw), tile)
    ops.gemm(x16, wf, out, **kw)
    want = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5) @ wq.double().t() + bq.double()
    assert bool(torch.isfinite(out).all()) and int(guard.item()) == 0
    l2, mx = rel_l2(out.cpu(), want.cpu()), max_rel(out.cpu(), want.cpu())
    print(f"H split_k={split} consumer tile {tile}: rel-L2 {l2:.2e} (bar {H_L2:.1e}), max-rel {mx:.2e} (bar {H_MAX:.0e})")
    assert l2 <= H_L2 and mx <= H_MAX
