"""The forward norm, head/tail and encoder glue kernels at their edges: the second half of storygen_amd/csrc/norm.hip (the narrow GroupNorm
pair, the one-launch GroupNorm's 256-thread instantiation, the branches behind the gn_* development options, LayerNorm up to C = 2048),
storygen_amd/csrc/misc.hip (linear_rows, timestep_embed, lookup_rows, the two thin convolutions, add_noise, copy_rows, pad_cast) and the small
kernels of storygen_amd/csrc/encoders.hip (softmax_rows, attn_small, act_rows, embed_tokens, clip_embed_patches, gaussian_sample), plus the
"every key biased away = uniform average" contract of attention_enc.hip.

Reference for every case: the same operation in plain torch, in float64, on the same fp16-rounded or fp32 inputs.

Bars (all the project's own): fp16 outputs TOL_L2 = 1e-3 / TOL_MAX = 3e-3 of tests/test_kernels_gpu.py::check; fp32 outputs of misc.hip rel-L2 1e-5 /
max 1e-4 (test_time_embedding_path) and 1e-6 for add_noise (test_sampling_elementwise); two GroupNorm paths on the same input rel-L2 < 3e-4
(test_groupnorm_statistics_from_producer_epilogues); attn_small 1.5e-3 (test_attention_small); attention_enc ATTN_BAR of
tests/test_pick_score_gpu.py; gaussian_sample 1e-5 and act_rows 1e-3 (test_act_embed_and_gaussian_kernels); copies, gathers and lookups torch.equal.

Every output that is a view of a wider buffer sits in a NaN-prefilled buffer (a finite sentinel for the in-place act_rows and for lookup_rows,
whose miss rows are NaN themselves) and everything outside the view must come back untouched.  Only shapes are chosen here: the smallest that
reach each branch; the comment next to each parameter list says which.  Every case prints its measured error (`-s`); the figures of the first
hardware run are in profiles/r17a_forward_edge_tests.txt."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import max_rel, rel_l2
from test_kernels_gpu import TOL_L2, TOL_MAX
from test_pick_score_gpu import ATTN_BAR

pytestmark = pytest.mark.gpu
F16, F32, F64 = torch.float16, torch.float32, torch.float64
FMIN = torch.finfo(torch.float32).min
F32_L2, F32_MAX = 1e-5, 1e-4        # fp32 outputs of misc.hip (test_time_embedding_path, test_conv_in_out)
GN_PATHS_L2 = 3e-4                  # two GroupNorm paths on the same input (test_groupnorm_statistics_from_producer_epilogues)
ATTN_SMALL_BAR = 1.5e-3             # test_attention_small
GN_DEFAULTS = dict(gn_no_fused=0, gn_wide=1, gn_fused_nt=1024, gn_fused_max=-1, gn_chunks=0)


# ------------------------------------------------------------------------------------------------------------------------- helpers
def _randn(shape, dev, seed, dtype=F32, scale=1.0, shift=0.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=dev) * scale + shift).to(dtype)


def _nan(shape, dev, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _check(what, out, ref, l2=TOL_L2, mx=TOL_MAX):
    assert bool(torch.isfinite(out.float()).all()), f"{what}: non-finite output"
    e2, em = rel_l2(out, ref), max_rel(out, ref)
    print(f"{what}: rel-L2 {e2:.2e} (bar {l2:.0e}), max-rel {em:.2e} (bar {mx:.0e})")
    assert e2 <= l2 and em <= mx, f"{what}: rel-L2 {e2:.2e} (bar {l2:.0e}), max-rel {em:.2e} (bar {mx:.0e})"


def _agree(what, a, b, bar=GN_PATHS_L2):
    e = rel_l2(a, b)
    print(f"{what}: rel-L2 between the two paths {e:.2e} (bar {bar:.0e})")
    assert e < bar, f"{what}: {e:.2e}"


def _guards_are(buf, view_index, value=None):
    """Everything of buf outside buf[view_index] still holds the prefill (NaN when value is None)."""
    ok = torch.isnan(buf) if value is None else buf == value
    ok[view_index] = True
    assert bool(ok.all()), "guard elements outside the view were written"


@contextlib.contextmanager
def _options(**kw):
    """Development options for the body; the defaults are back afterwards, also when the body fails."""
    from storygen_amd import ops
    try:
        for name, value in kw.items():
            ops.debug_set_option(name, value)
        yield
    finally:
        for name in kw:
            ops.debug_set_option(name, GN_DEFAULTS[name])


def _silu64(x):
    return x * torch.sigmoid(x)


# ------------------------------------------------------------------------------------------------------------------------- GroupNorm
def _gn_ref(x, g, b, groups, eps, silu):
    B, HW, C = x.shape
    xd = x.double().reshape(B, HW, groups, C // groups)
    mean = xd.mean((1, 3), keepdim=True)
    var = ((xd - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((xd - mean) / torch.sqrt(var + eps)).reshape(B, HW, C) * g.double() + b.double()
    return _silu64(y) if silu else y


def _gn_run(x, g, b, out, silu, eps=1e-5, xcopy=None, groups=32):
    from storygen_amd import ops
    ws = torch.empty(ops.groupnorm_workspace_bytes(x.shape[0], groups), dtype=torch.uint8, device=x.device)
    ops.groupnorm(x, g, b, out, groups, eps, silu, ws, xcopy=xcopy)
    return out


def _gn_params(C, dev):
    return _randn((C,), dev, 2, F16), _randn((C,), dev, 3, F16)


# (B, H, W, C), 32 groups; the geometry is the narrow pair's in gn_plan (tw = min(C/8, 256) threads per pixel row, rpp = 256 / tw rows per pass)
NARROW = [
    (2, 64, 64, 128),    # cpg 4, slab 16384 (the VAE's outer level): rpp 16, 32 chunks of 128 rows = two trips of the 4-row loop, no remainder
    (3, 25, 40, 64),     # cpg 2: rpp 32, 4 chunks of 250 rows: 4-row loop, then 0 to 3 remainder rows depending on the thread row
    (3, 7, 143, 64),     # cpg 2, HW = 1001: 4 chunks of 251 rows, a ragged last chunk of 248 (statistics) and of 118 rows (fp32 apply)
    (1, 42, 50, 192),    # cpg 6: C/8 = 24 does not divide 256 (16 idle threads, rpp 10); 27 chunks of 78 rows, the last one 72
    (1, 96, 96, 128),    # HW / (8 rpp) = 72 chunks wanted: the GN_MAX_CHUNKS = 64 cap
    (16, 64, 72, 128),   # 36 chunks wanted: the 512 / B = 32 cap
]


def _assert_narrow(HW, C, groups=32):
    from storygen_amd import ops
    assert ops.groupnorm_is_fused(HW, C, groups) == 0 and ops.groupnorm_uses_pstats(HW, C, groups) == 0, "no longer the narrow pair"
    assert ops.groupnorm_plan(HW, C, groups)[:2] == ("narrow", 256)


@pytest.mark.parametrize("flavour", ["f16", "resnet"])
@pytest.mark.parametrize("B,H,W,C", NARROW, ids=lambda v: str(v))
def test_groupnorm_narrow_pair(gpu, B, H, W, C, flavour):
    """gn_stats_kernel + gn_apply_kernel under the default options: (f16) fp16 in, fp16 out, no SiLU; (resnet) fp32 in, SiLU, zero-bordered
    output, raw fp16 copy — the flavour of test_groupnorm_fp32_in_padded_out_rawcopy."""
    HW = H * W
    _assert_narrow(HW, C)
    g, b = _gn_params(C, gpu)
    if flavour == "f16":
        x = _randn((B, HW, C), gpu, 1, F16, 2.0, 3.0)
        out = _gn_run(x, g, b, torch.empty_like(x), False, 1e-6)
        _check(f"groupnorm narrow f16 {(B, HW, C)}", out, _gn_ref(x, g, b, 32, 1e-6, False))
        return
    x = _randn((B, HW, C), gpu, 1, F32, 2.0, 1.5)
    yp = torch.zeros(B, H + 2, W + 2, C, dtype=F16, device=gpu)
    xc = _nan((B, HW, C), gpu, F16)
    _gn_run(x, g, b, yp, True, 1e-5, xcopy=xc)
    _check(f"groupnorm narrow resnet {(B, HW, C)}", yp[:, 1:-1, 1:-1].reshape(B, HW, C), _gn_ref(x, g, b, 32, 1e-5, True))
    assert float(yp[:, 0].abs().max()) == 0 and float(yp[:, -1].abs().max()) == 0
    assert float(yp[:, :, 0].abs().max()) == 0 and float(yp[:, :, -1].abs().max()) == 0
    assert torch.equal(xc, x.half())


def test_groupnorm_narrow_pair_row_strided(gpu):
    """x a channel window of a wider buffer (ldx = 192 > C), the output a window of another (ldy = 144)."""
    B, HW, C = 2, 4096, 128
    _assert_narrow(HW, C)
    big = _randn((B, HW, 192), gpu, 1, F16, 2.0, -0.7)
    x = big[:, :, 64:]
    g, b = _gn_params(C, gpu)
    obuf = _nan((B, HW, 144), gpu, F16)
    out = _gn_run(x, g, b, obuf[:, :, 8:8 + C], True)
    _check("groupnorm narrow strided", out, _gn_ref(x, g, b, 32, 1e-5, True))
    _guards_are(obuf, (slice(None), slice(None), slice(8, 8 + C)))


def _gn_case(gpu, B, HW, C, silu=True, eps=1e-5):
    x = _randn((B, HW, C), gpu, 1, F16, 2.0, 3.0)
    g, b = _gn_params(C, gpu)
    return x, g, b, _gn_ref(x, g, b, 32, eps, silu), silu, eps


# gn_wide = 0 sends what the wide pair serves by default to the narrow pair
@pytest.mark.parametrize("B,HW,C", [(2, 256, 2560),     # C/8 = 320 > 256: the column loop (two trips, the second with 64 live columns), rpp 1
                                    (2, 1024, 320)])    # cpg 10: an 8-channel vector straddles two groups, C/8 = 40 leaves 16 idle threads
def test_groupnorm_narrow_pair_behind_gn_wide(gpu, B, HW, C):
    from storygen_amd import ops
    x, g, b, ref, silu, eps = _gn_case(gpu, B, HW, C)
    assert ops.groupnorm_uses_pstats(HW, C, 32) == 1, "default: the wide pair"
    assert ops.groupnorm_plan(HW, C, 32, B=B)[:2] == ("wide", 1024)
    default = _gn_run(x, g, b, torch.empty_like(x), silu, eps)
    with _options(gn_wide=0):
        _assert_narrow(HW, C)
        out = _gn_run(x, g, b, torch.empty_like(x), silu, eps)
    _check(f"groupnorm gn_wide=0 {(B, HW, C)}", out, ref)
    _agree(f"groupnorm gn_wide=0 vs wide pair {(B, HW, C)}", out, default)


# gn_no_fused = 1 sends what the one-launch kernel serves by default to the wide pair
@pytest.mark.parametrize("B,HW,C", [(4, 256, 1280),     # cpg 40, rpp 6: rows_per_chunk raised to rpp, 43 chunks, the last one 4 rows
                                    (3, 64, 640)])      # cpg 20, rpp 12: 6 chunks, the last one 4 rows
def test_groupnorm_wide_pair_behind_gn_no_fused(gpu, B, HW, C):
    from storygen_amd import ops
    x, g, b, ref, silu, eps = _gn_case(gpu, B, HW, C)
    assert ops.groupnorm_is_fused(HW, C, 32) == 1, "default: the one-launch kernel"
    fused = _gn_run(x, g, b, torch.empty_like(x), silu, eps)
    with _options(gn_no_fused=1):
        assert ops.groupnorm_is_fused(HW, C, 32) == 0 and ops.groupnorm_uses_pstats(HW, C, 32) == 1
        assert ops.groupnorm_plan(HW, C, 32, B=B)[:2] == ("wide", 1024)
        out = _gn_run(x, g, b, torch.empty_like(x), silu, eps)
    _check(f"groupnorm gn_no_fused=1 {(B, HW, C)}", out, ref)
    _agree(f"groupnorm gn_no_fused=1 vs one-launch {(B, HW, C)}", out, fused)


# gn_fused_nt = 256: gn_fused_kernel<false, 256, GNF_MAXI> (the default 1024-thread instantiation also accepts these three)
@pytest.mark.parametrize("B,HW,C", [(3, 64, 640),       # slab 1280: 320 items, only the first two of the 24 item slots, the second partly
                                    (1, 100, 2560),     # slab 8000: 2000 items, 20 per pixel
                                    (4, 256, 1280)])    # slab 10240 = the default threshold: 2560 items, ten full item slots
def test_groupnorm_one_launch_256_threads(gpu, B, HW, C):
    from storygen_amd import ops
    x, g, b, ref, silu, eps = _gn_case(gpu, B, HW, C)
    assert ops.groupnorm_is_fused(HW, C, 32) == 1
    nt1024 = _gn_run(x, g, b, torch.empty_like(x), silu, eps)
    assert ops.groupnorm_plan(HW, C, 32, B=B)[:2] == ("one_launch", 1024)
    with _options(gn_fused_nt=256):
        assert ops.groupnorm_is_fused(HW, C, 32) == 1
        assert ops.groupnorm_plan(HW, C, 32, B=B)[:2] == ("one_launch", 256)
        out = _gn_run(x, g, b, torch.empty_like(x), silu, eps)
    _check(f"groupnorm gn_fused_nt=256 {(B, HW, C)}", out, ref)
    _agree(f"groupnorm 256 vs 1024 threads {(B, HW, C)}", out, nt1024)


# ... and with gn_fused_max = 24576 the slabs only that instantiation can hold (above the 1024-thread kernel's 16384)
@pytest.mark.parametrize("B,HW,C,fused", [(1, 256, 2560, True),     # slab 20480: 5120 items, 20 of the 24 item slots
                                          (2, 384, 2048, True),     # slab exactly 24576 = 256 x 24 x 4: every slot of every thread
                                          (1, 385, 2048, False)])   # slab 24640: one pixel too many, must not be fused (wide pair)
def test_groupnorm_one_launch_256_threads_large_slabs(gpu, B, HW, C, fused):
    from storygen_amd import ops
    x, g, b, ref, silu, eps = _gn_case(gpu, B, HW, C, silu=not fused)
    with _options(gn_fused_nt=256, gn_fused_max=24576):
        assert ops.groupnorm_is_fused(HW, C, 32) == int(fused)
        assert ops.groupnorm_plan(HW, C, 32, B=B)[:2] == (("one_launch", 256) if fused else ("wide", 1024))
        out = _gn_run(x, g, b, torch.empty_like(x), silu, eps)
    assert ops.groupnorm_is_fused(HW, C, 32) == 0, "options not restored"
    _check(f"groupnorm gn_fused_max=24576 {(B, HW, C)}", out, ref)


def test_groupnorm_wide_pair_gn_chunks(gpu):
    """gn_chunks = 64 (64 chunks of 64 rows) against the default 256 / B = 85 wanted (84 chunks of 49 rows, the last one 29)."""
    from storygen_amd import ops
    B, HW, C = 3, 4096, 320
    x, g, b, ref, silu, eps = _gn_case(gpu, B, HW, C)
    default = _gn_run(x, g, b, torch.empty_like(x), silu, eps)
    assert ops.groupnorm_plan(HW, C, 32, B=B)[:5] == ("wide", 1024, 2, 84, 49)
    with _options(gn_chunks=64):
        assert ops.groupnorm_plan(HW, C, 32, B=B)[:5] == ("wide", 1024, 2, 64, 64)
        out = _gn_run(x, g, b, torch.empty_like(x), silu, eps)
    _check("groupnorm gn_chunks=64", out, ref)
    _check("groupnorm default chunking", default, ref)
    _agree("groupnorm gn_chunks=64 vs default chunking", out, default)


# ------------------------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_ref(x, g, b, eps=1e-5):
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    return (xd - mean) / torch.sqrt(var + eps) * g.double() + b.double()


# C = 8: one live lane; 768: second vector of layernorm_kernel<2> half filled (CLIP text tower); 1024: exactly filled (ViT-L); 1536: <3> exactly
# filled; 1544: the first lane of <4>'s fourth vector; 2048: <4> full.  M = 1: three of the block's four waves leave at once; 6: a second block
@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("M", [1, 6])
@pytest.mark.parametrize("C", [8, 768, 1024, 1536, 1544, 2048])
def test_layernorm_widths(gpu, C, M, dtype):
    from storygen_amd import ops
    x = _randn((M, C), gpu, 1, dtype, 2.0, 1.0)
    g1, b1, g2, b2 = (_randn((C,), gpu, s, F16) for s in (2, 3, 4, 5))
    y1, y2 = _nan((M, C), gpu, F16), _nan((M, C), gpu, F16)
    ops.layernorm(x, g1, b1, y1, 1e-5, g2, b2, y2)
    _check(f"layernorm dual M{M} C{C} {dtype} y1", y1, _ln_ref(x, g1, b1))
    _check(f"layernorm dual M{M} C{C} {dtype} y2", y2, _ln_ref(x, g2, b2))
    ys = _nan((M, C), gpu, F16)
    ops.layernorm(x, g2, b2, ys, 1e-5)
    _check(f"layernorm single M{M} C{C} {dtype}", ys, _ln_ref(x, g2, b2))


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_layernorm_column_windows(gpu, dtype):
    """x, y1 and y2 are column windows of three wider buffers with three different row strides."""
    from storygen_amd import ops
    M, C = 6, 1544
    xbuf = _randn((M, C + 16), gpu, 1, dtype, 2.0, 1.0)
    x = xbuf[:, 8:8 + C]
    g1, b1, g2, b2 = (_randn((C,), gpu, s, F16) for s in (2, 3, 4, 5))
    y1buf, y2buf = _nan((M, C + 24), gpu, F16), _nan((M, C + 8), gpu, F16)
    y1, y2 = y1buf[:, 16:16 + C], y2buf[:, :C]
    ops.layernorm(x, g1, b1, y1, 1e-5, g2, b2, y2)
    _check(f"layernorm windows {dtype} y1", y1, _ln_ref(x, g1, b1))
    _check(f"layernorm windows {dtype} y2", y2, _ln_ref(x, g2, b2))
    _guards_are(y1buf, (slice(None), slice(16, 16 + C)))
    _guards_are(y2buf, (slice(None), slice(0, C)))


def test_layernorm_large_mean(gpu):
    """fp32 rows with mean 1000 and sigma 1: E[x^2] - E[x]^2 in fp32 would lose every digit; the exact two-pass kernel keeps the normal bar."""
    from storygen_amd import ops
    M, C = 6, 2048
    x = _randn((M, C), gpu, 1, F32, 1.0, 1000.0)
    g, b = _randn((C,), gpu, 2, F16), _randn((C,), gpu, 3, F16)
    y = _nan((M, C), gpu, F16)
    ops.layernorm(x, g, b, y)
    _check("layernorm mean 1000 sigma 1", y, _ln_ref(x, g, b))


def test_layernorm_rejects_rows_wider_than_2048(gpu):
    from storygen_amd import ops
    x = _randn((2, 2056), gpu, 1, F16)
    g = _randn((2056,), gpu, 2, F16)
    with pytest.raises(RuntimeError, match="<= 2048"):
        ops.layernorm(x, g, g, torch.empty_like(x))


# ------------------------------------------------------------------------------------------------------------------------- misc.hip
# (B, N, K, bias, act_in, act_out, strided).  B <= 4: linear_rows_kernel<4>, 5..8: <8>, 9..16: <16>; N = 6 and 1282 leave two idle waves in the
# last block; K = 8: one live lane; 1288 = 2 x 512 + 264: a third, partial trip of the k loop; 320: lanes 40..63 never enter it
LINEAR = [(1, 4, 8, True, False, False, False), (4, 6, 320, False, True, False, False), (5, 1282, 8, True, False, True, False),
          (8, 6, 1288, True, True, True, True), (9, 4, 320, False, False, True, True), (16, 1282, 1288, True, False, False, True),
          (16, 6, 8, True, True, False, False)]


@pytest.mark.parametrize("B,N,K,bias,act_in,act_out,strided", LINEAR)
def test_linear_rows(gpu, B, N, K, bias, act_in, act_out, strided):
    from storygen_amd import ops
    w = _randn((N, K), gpu, 1, F16, 1.0 / math.sqrt(K))
    bs = _randn((N,), gpu, 2, F16) if bias else None
    xbuf = _randn((B, K + 8), gpu, 3, F32, 1.5)
    x = xbuf[:, 4:4 + K] if strided else xbuf[:, :K].contiguous()
    obuf = _nan((B, N + 5), gpu, F32)
    out = obuf[:, 2:2 + N] if strided else obuf[:, :N]
    ops.linear_rows(x, w, bs, out, act_in=act_in, act_out=act_out)
    xd = _silu64(x.double()) if act_in else x.double()
    ref = xd @ w.double().t() + (bs.double() if bias else 0.0)
    ref = _silu64(ref) if act_out else ref
    _check(f"linear_rows B{B} N{N} K{K} bias={bias} act_in={act_in} act_out={act_out} strided={strided}", out, ref, F32_L2, F32_MAX)
    _guards_are(obuf, (slice(None), slice(2, 2 + N) if strided else slice(0, N)))


def test_linear_rows_rejects_17_rows(gpu):
    from storygen_amd import ops
    x, w = _randn((17, 8), gpu, 1), _randn((4, 8), gpu, 2, F16)
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.linear_rows(x, w, None, torch.empty(17, 4, device=gpu))


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("B,dim", [(3, 34),      # 51 threads of one block; an odd half dimension
                                   (5, 320)])    # 800 threads: four blocks, the last one partly
def test_timestep_embed(gpu, B, dim, flip):
    from storygen_amd import ops
    half = dim // 2
    t = torch.tensor([0.0, 0.5, 999.0, 1.0, 517.0][:B], device=gpu)
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F32) / half).to(gpu)
    out = _nan((B, dim), gpu, F32)
    ops.timestep_embed(t, freqs, out, flip)
    e = (t[:, None] * freqs[None]).double()          # the fp32 product the kernel forms, then float64 sin / cos
    ref = torch.cat([torch.cos(e), torch.sin(e)], -1) if flip else torch.cat([torch.sin(e), torch.cos(e)], -1)
    _check(f"timestep_embed B{B} dim{dim} flip={flip}", out, ref, F32_L2, F32_MAX)


# N = 4: one live thread; 1024: one full block; 1028: one thread of a second block; 2052: a third.  T = 1: no scan; 37: the duplicate and a late hit
@pytest.mark.parametrize("T", [1, 37])
@pytest.mark.parametrize("N", [4, 1024, 1028, 2052])
def test_lookup_rows(gpu, N, T):
    from storygen_amd import ops
    tkeys = torch.arange(T, dtype=F32, device=gpu) * 1.5 + 0.25
    if T > 20:
        tkeys[20] = tkeys[5]                              # a duplicated key: the first match (row 5) wins
    tbuf = _randn((T, N + 8), gpu, 1)
    table = tbuf[:, 4:4 + N]
    want_rows = [0, -1] if T == 1 else [T - 1, 5, -1, 0, 19]      # -1: a key the table does not hold
    keys = torch.tensor([12345.0 if r < 0 else float(tkeys[r]) for r in want_rows], device=gpu)
    Bq = len(want_rows)
    obuf = torch.full((Bq, N + 12), 7.0, device=gpu)      # finite sentinel: a miss row is NaN, and must be told from an untouched one
    out = obuf[:, 8:8 + N]
    ops.lookup_rows(keys, tkeys, table, out)
    for i, r in enumerate(want_rows):
        if r < 0:
            assert bool(torch.isnan(out[i]).all()), "a miss must give an all-NaN row"
        else:
            assert torch.equal(out[i], table[r]), f"row {i} is not table row {r}"
    _guards_are(obuf, (slice(None), slice(8, 8 + N)), value=7.0)
    print(f"lookup_rows N{N} T{T}: {Bq} rows exact")


HW_EDGES = [(1, 1), (1, 7), (5, 1), (9, 6)]     # one pixel (only the centre tap), one row, one column, and a shape with an interior


@pytest.mark.parametrize("out_f32", [False, True], ids=["f16", "f32"])
@pytest.mark.parametrize("H,W", HW_EDGES)
def test_conv_in_edges(gpu, H, W, out_f32):
    """Cin in {1, 4, 8} x Cout in {8 (one channel group per pixel), 320}; the output is a channel window of a wider NHWC buffer."""
    from storygen_amd import ops
    B = 2
    for Cin in (1, 4, 8):
        for Cout in (8, 320):
            x = _randn((B, Cin, H, W), gpu, 1)
            w = _randn((Cout, Cin, 3, 3), gpu, 2, F16, 1.0 / math.sqrt(9 * Cin))
            b = _randn((Cout,), gpu, 3, F16)
            ybuf = _nan((B, H, W, Cout + 16), gpu, F32 if out_f32 else F16)
            y = ybuf[..., 8:8 + Cout]
            ops.conv_in(x, w.permute(2, 3, 1, 0).reshape(9 * Cin, Cout).contiguous(), b, y)
            ref = F.conv2d(x.cpu().double(), w.cpu().double(), b.cpu().double(), padding=1)
            l2, mx = (F32_L2, F32_MAX) if out_f32 else (TOL_L2, TOL_MAX)
            _check(f"conv_in {H}x{W} Cin{Cin} Cout{Cout} {'f32' if out_f32 else 'f16'}", y.permute(0, 3, 1, 2).cpu(), ref, l2, mx)
            _guards_are(ybuf, (Ellipsis, slice(8, 8 + Cout)))


@pytest.mark.parametrize("H,W", HW_EDGES)
def test_conv_out_edges(gpu, H, W):
    """Cout in {1, 3, 4} x Cin in {8, 72, 520}: 9, 81 and 585 input chunks over 64 lanes (idle lanes; a second, partial trip; ten trips, the last
    one partial); x is a channel window whose neighbours are NaN."""
    from storygen_amd import ops
    B = 2
    for Cout in (1, 3, 4):
        for Cin in (8, 72, 520):
            xbuf = _nan((B, H, W, Cin + 16), gpu, F16)
            x = xbuf[..., 8:8 + Cin]
            x.copy_(_randn((B, H, W, Cin), gpu, 1, F16))
            w = _randn((Cout, Cin, 3, 3), gpu, 2, F16, 1.0 / math.sqrt(9 * Cin))
            b = _randn((Cout,), gpu, 3, F16)
            out = _nan((B, Cout, H, W), gpu, F32)
            ops.conv_out(x, w.permute(0, 2, 3, 1).contiguous(), b, out)
            ref = F.conv2d(x.permute(0, 3, 1, 2).cpu().double(), w.cpu().double(), b.cpu().double(), padding=1)
            _check(f"conv_out {H}x{W} Cin{Cin} Cout{Cout}", out.cpu(), ref, F32_L2, F32_MAX)


def test_thin_convs_reject_too_many_channels(gpu):
    from storygen_amd import ops
    x = _randn((1, 9, 4, 4), gpu, 1)
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.conv_in(x, _randn((81, 8), gpu, 2, F16), _randn((8,), gpu, 3, F16), torch.empty(1, 4, 4, 8, dtype=F16, device=gpu))
    xo = _randn((1, 4, 4, 8), gpu, 1, F16)
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.conv_out(xo, _randn((5, 3, 3, 8), gpu, 2, F16), _randn((5,), gpu, 3, F16), torch.empty(1, 5, 4, 4, device=gpu))


@pytest.mark.parametrize("n", [70001,     # 274 blocks wanted, 256 launched per sample: the loop wraps, the second trip ends mid-block
                               1])
def test_add_noise_grid_wrap(gpu, n):
    from storygen_amd import ops
    U, N = 4, 2
    src, noise = _randn((U, n), gpu, 1), _randn((N, n), gpu, 2)
    coef = torch.tensor([[0.9, 0.43], [0.95, 0.31], [0.7, 0.71], [0.5, 0.86]], device=gpu)
    out = _nan((U, n), gpu, F32)
    ops.add_noise(src, noise, coef, out)
    cd = coef.double()
    ref = torch.stack([cd[u, 0] * src[u].double() + cd[u, 1] * noise[u % N].double() for u in range(U)])
    _check(f"add_noise n={n}", out, ref, 1e-6, 1e-6)


@pytest.mark.parametrize("Bn,rows,cols", [(4, 4100, 264),     # 541200 vectors > 2048 x 256: every thread loops, the second trip is partial
                                          (1, 1, 8)])         # one vector
def test_copy_rows_grid_wrap(gpu, Bn, rows, cols):
    """All three modes, source and destination both windows (rows and columns) of larger buffers; the results are exact."""
    from storygen_amd import ops
    win_s = (slice(None), slice(0, rows), slice(8, 8 + cols))
    win_d = (slice(None), slice(1, 1 + rows), slice(16, 16 + cols))
    for mode, (sdt, ddt) in enumerate([(F16, F16), (F32, F32), (F32, F16)]):
        sbuf = _randn((Bn, rows + 1, cols + 8), gpu, 1 + mode, sdt)
        dbuf = _nan((Bn, rows + 2, cols + 16), gpu, ddt)
        ops.copy_rows(dbuf[win_d], sbuf[win_s])
        assert torch.equal(dbuf[win_d], sbuf[win_s].to(ddt)), f"copy_rows mode {mode}"
        _guards_are(dbuf, win_d)
        print(f"copy_rows {(Bn, rows, cols)} mode {mode}: exact, guards untouched")


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_pad_cast_grid_wrap(gpu, dtype):
    """679380 vectors > 2048 x 256; x is a channel window (pixel stride 424 > C = 416)."""
    from storygen_amd import ops
    B, H, W, C = 3, 65, 67, 416
    x = _randn((B, H, W, C + 8), gpu, 1, dtype)[..., 8:]
    out = torch.zeros(B, H + 2, W + 2, C, dtype=F16, device=gpu)
    ops.pad_cast(x, out)
    assert torch.equal(out[:, 1:-1, 1:-1], x.half())
    assert float(out[:, 0].abs().max()) == 0 and float(out[:, -1].abs().max()) == 0
    assert float(out[:, :, 0].abs().max()) == 0 and float(out[:, :, -1].abs().max()) == 0
    print(f"pad_cast {(B, H, W, C)} {dtype}: interior exact, border zero")


# ------------------------------------------------------------------------------------------------------------------------- encoders.hip
def _softmax_run(gpu, s_view, scale):
    from storygen_amd import ops
    M, N = s_view.shape
    N8 = (N + 7) & ~7
    pbuf = _nan((M, N8 + 16), gpu, F16)
    p = pbuf[:, 8:8 + N8]
    ops.softmax_rows(s_view, p, scale)
    _guards_are(pbuf, (slice(None), slice(8, 8 + N8)))
    if N8 > N:
        assert float(p[:, N:].abs().max()) == 0.0, "padding columns must be zero"
    return p[:, :N]


# N = 1: one live thread, 7 padding columns; 7: less than a wave; 255 / 256 / 257: one thread short of, exactly, and one past one trip
@pytest.mark.parametrize("N", [1, 7, 255, 256, 257])
def test_softmax_rows_below_and_around_one_trip(gpu, N):
    M = 3
    sbuf = _randn((M, N + 5), gpu, N, F32, 6.0)
    s = sbuf[:, 2:2 + N]                                   # strided scores
    p = _softmax_run(gpu, s, 0.37)
    _check(f"softmax_rows N{N}", p, torch.softmax(s.double() * 0.37, -1))
    # scores of magnitude 3e4 at scale 1: exp(s) overflows, exp(s - max) does not
    sign = torch.where(_randn((M, N), gpu, N + 1) < 0, -1.0, 1.0)
    sign[:, 0] = 1.0
    big = (sign * 3.0e4 + _randn((M, N), gpu, N + 2)).contiguous()
    p = _softmax_run(gpu, big, 1.0)
    _check(f"softmax_rows N{N} |s| = 3e4", p, torch.softmax(big.double(), -1))
    # a constant row: exactly uniform
    p = _softmax_run(gpu, torch.full((M, N), 5.0, device=gpu), 1.0)
    assert torch.equal(p, torch.full((M, N), 1.0 / N, dtype=F64, device=gpu).half()), "a constant row must be exactly uniform"
    print(f"softmax_rows N{N} constant row: exactly {float(p[0, 0])}")


def _attn_inputs(gpu, B, H, T, D, seed):
    """q, k, v in three buffers with distinct token and batch strides; a finite random key bias, the last batch row biased away entirely."""
    C = H * D
    qbuf, kbuf, vbuf = _randn((B, T + 1, C + 8), gpu, seed, F16), _randn((B, T + 3, C + 16), gpu, seed + 1, F16), _randn((B, T + 5, C), gpu, seed + 2, F16)
    q, k, v = qbuf[:, :T, :C], kbuf[:, :T, 8:8 + C], vbuf[:, :T]
    assert len({q.stride(0), k.stride(0), v.stride(0)}) == 3
    kb = _randn((B, T), gpu, seed + 3, F32, 0.5)
    kb[B - 1] = FMIN
    return q, k, v, kb


def _attn_ref(q, k, v, H, scale, causal, kb):
    B, T, C = q.shape
    D = C // H
    qh, kh, vh = (t.double().reshape(B, T, H, D).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * scale + kb.double()[:, None, None, :]
    if causal:
        s = s + torch.full((T, T), float("-inf"), device=q.device, dtype=F64).triu(1)
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, T, C)


def _uniform_average(v, causal):
    """What a batch row with every key biased away must give: the mean of V over all keys (over keys <= i when causal)."""
    vd = v.double()
    T = vd.shape[0]
    if not causal:
        return vd.mean(0, keepdim=True).expand_as(vd)
    return vd.cumsum(0) / torch.arange(1, T + 1, device=v.device, dtype=F64)[:, None]


def _attn_check(gpu, fn, name, B, H, T, D, causal, bar):
    q, k, v, kb = _attn_inputs(gpu, B, H, T, D, 100 * T + D)
    C = H * D
    obuf = _nan((B, T, C + 16), gpu, F16)
    out = obuf[:, :, 8:8 + C]
    fn(q, k, v, out, H, D ** -0.5, causal, kb)
    assert bool(torch.isfinite(out).all()), f"{name}: non-finite output"
    _guards_are(obuf, (slice(None), slice(None), slice(8, 8 + C)))
    err = rel_l2(out, _attn_ref(q, k, v, H, D ** -0.5, causal, kb))
    eu = rel_l2(out[B - 1], _uniform_average(v[B - 1], causal))
    print(f"{name} B{B} H{H} T{T} D{D} causal={causal}: rel-L2 {err:.2e}, all-keys-biased row vs uniform average {eu:.2e} (bar {bar:.1e})")
    assert err < bar and eu < bar


# T = 16 / 17: one row chunk / one row into a second; 64 / 65: lane j's second key (j + 64) unused / used once; 127 / 128: the last key absent /
# the limit.  D = 4, 20: partial head dims (lanes >= D idle); 64: the limit.  T = 128 with D = 64 fills the LDS tiles.
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,H,T,D", [(2, 2, 16, 4), (2, 3, 17, 20), (2, 1, 64, 64), (2, 2, 65, 4), (3, 2, 127, 20), (2, 2, 128, 64)])
def test_attention_small_limits(gpu, B, H, T, D, causal):
    from storygen_amd import ops
    _attn_check(gpu, ops.attention_small, "attention_small", B, H, T, D, causal, ATTN_SMALL_BAR)


def test_attention_small_rejects_beyond_its_limits(gpu):
    from storygen_amd import ops
    for T, D in ((129, 8), (8, 65)):
        q = _randn((1, T, D), gpu, 1, F16)
        with pytest.raises(RuntimeError, match="needs T <= 128 and D <= 64"):
            ops.attention_small(q, q, q, torch.empty_like(q), 1, 1.0, False)


@pytest.mark.parametrize("causal", [False, True])
def test_attention_enc_all_keys_biased_row(gpu, causal):
    """T = 130: three key tiles of 64, the last with two live keys; two query blocks of 128."""
    from storygen_amd import ops
    _attn_check(gpu, ops.attention_enc, "attention_enc", 2, 2, 130, 40, causal, ATTN_BAR)


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_act_rows_special_values(gpu, act):
    """A (5, 40) view; +-0, the smallest and the largest fp16 subnormal, +-65504 among ordinary values."""
    from storygen_amd import ops
    special = [0.0, -0.0, 2.0 ** -24, -(2.0 ** -24), 1023 * 2.0 ** -24, -1023 * 2.0 ** -24, 65504.0, -65504.0]
    vals = _randn((5, 40), gpu, 1, F16, 3.0)
    vals.view(-1)[: len(special)] = torch.tensor(special, dtype=F64).half().to(gpu)
    buf = torch.full((5, 56), 3.0, dtype=F16, device=gpu)
    view = buf[:, 8:48]
    view.copy_(vals)
    ops.act_rows(view, ops.ACT_QUICK_GELU if act == "quick_gelu" else ops.ACT_GELU)
    xd = vals.double()
    ref = xd * torch.sigmoid(1.702 * xd) if act == "quick_gelu" else 0.5 * xd * (1.0 + torch.erf(xd / math.sqrt(2.0)))
    assert bool(torch.isfinite(view).all()), "non-finite output"
    _guards_are(buf, (slice(None), slice(8, 48)), value=3.0)
    e_all = rel_l2(view, ref)
    ordinary = vals.abs().flatten() < 100.0                     # without +-65504, which alone would carry the norm
    e_ord = rel_l2(view.flatten()[ordinary], ref.flatten()[ordinary])
    print(f"act_rows {act}: rel-L2 {e_all:.2e}, without +-65504 {e_ord:.2e} (bar 1e-03)")
    assert e_all < 1e-3 and e_ord < 1e-3


@pytest.mark.parametrize("rows,T,C,vocab", [(7, 3, 4, 5),           # one float4 per row, 7 threads
                                            (154, 77, 772, 1000)])  # 29722 vectors: 117 blocks, the last one partial
def test_embed_tokens_edges(gpu, rows, T, C, vocab):
    from storygen_amd import ops
    tok, pos = _randn((vocab, C), gpu, 1), _randn((T, C), gpu, 2)
    ids = torch.randint(0, vocab, (rows,), generator=torch.Generator().manual_seed(3)).to(gpu)
    ids[0], ids[rows - 1], ids[rows // 2] = 0, vocab - 1, vocab - 1
    ids[1] = 0
    obuf = _nan((rows, C + 8), gpu, F32)
    out = obuf[:, 4:4 + C]
    ops.embed_tokens(ids, tok, pos, out, T)
    assert torch.equal(out, tok[ids] + pos[torch.arange(rows, device=gpu) % T])
    _guards_are(obuf, (slice(None), slice(4, 4 + C)))
    print(f"embed_tokens rows{rows} T{T} C{C}: exact, guards untouched")


@pytest.mark.parametrize("B,T,C", [(1, 2, 4),         # the minimum: one class row, one patch row, one float4 each
                                   (3, 5, 132)])      # 495 vectors: two blocks
def test_clip_embed_patches_edges(gpu, B, T, C):
    from storygen_amd import ops
    pbuf = _randn((B * (T - 1), C + 8), gpu, 1)
    patches = pbuf[:, 4:4 + C]
    cls, pos = _randn((C,), gpu, 2), _randn((T, C), gpu, 3)
    obuf = _nan((B * T, C + 12), gpu, F32)
    out = obuf[:, 8:8 + C]
    ops.clip_embed_patches(patches, cls, pos, out, T)
    want = torch.cat([torch.cat([cls[None], patches[b * (T - 1):(b + 1) * (T - 1)]]) + pos for b in range(B)])
    assert torch.equal(out, want)
    _guards_are(obuf, (slice(None), slice(8, 8 + C)))
    print(f"clip_embed_patches B{B} T{T} C{C}: exact, guards untouched")


@pytest.mark.parametrize("n", [1100003,      # > 4096 x 256 = 1048576: the grid wraps, the second trip is partial
                               1])
def test_gaussian_sample_grid_wrap_and_clamp_bounds(gpu, n):
    from storygen_amd import ops
    mean, noise = _randn((n,), gpu, 1), _randn((n,), gpu, 2)
    logvar = _randn((n,), gpu, 3, F32, 20.0)
    edge = torch.tensor([100.0, -30.0, 20.0, -100.0], device=gpu)      # the clamp bounds exactly, and far beyond them
    logvar[: min(n, 4)] = edge[: min(n, 4)]
    out = _nan((n,), gpu, F32)
    ops.gaussian_sample(mean, logvar, noise, out, 0.18215)
    ref = (mean.double() + torch.exp(0.5 * logvar.double().clamp(-30.0, 20.0)) * noise.double()) * 0.18215
    assert bool(torch.isfinite(out).all()), "non-finite (or unwritten) output"
    err, e4 = rel_l2(out, ref), rel_l2(out[:4], ref[:4])
    print(f"gaussian_sample n={n}: rel-L2 {err:.2e}, the clamp-bound elements {e4:.2e} (bar 1e-05)")
    assert err < 1e-5 and e4 < 1e-5
