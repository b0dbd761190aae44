"""Forward attention (sg_attn_fwd_f16, sg_attn_fwd_pair_f16, sg_attn_fwd_lse_f16, sg_attn_f8_pack + sg_attn_fwd_f8_d40) at its dispatch,
tile, window and range edges, against the float64 `exact` of tests/attention_fwd_model.py.

Every launch of this module (see _launch) reads its operands through windows of NaN buffers — q and k as column windows of [B, N + 2, 3C] /
[Bk, Nk + 3, 2C] buffers (the other columns, the query rows at or beyond Nq and the key rows [Nk, Nk + 3) NaN, the batch stride not the
dense one), V^T as the first round8(Nk) columns of rows 16 columns longer (NaN beyond) — and writes through a window of a buffer
pre-filled with a NaN bit pattern whose every other element must come back untouched.  Every case asserts the kernel family, waves,
stages and workgroups it ran on through the plan wrappers of ops (the expectation restated here from the three dispatch thresholds),
and prints its measured errors on one line.

Bars of the fp16 kernels (per case): output finite; check() at 1e-3 rel-L2 / 3e-3 max against `exact` (2e-3 / 6e-3 for the D = 40 fast
path under a common logit offset: the bar of tests/test_kernels_gpu.py::test_attention_d40_fast_path_extreme_maxima, which defines that
input); and PER ROW
    e_row = ||got_row - exact_row|| / RMS over the rows of ||exact_row||   per (batch, head)
    max e_row(kernel) <= ROW_FACTOR x max e_row(rounded model) on the same inputs,
the rounded model being the reference plus the kernel's documented roundings (never the kernel).  fp8: 8e-2 aggregate and the row bar
against the "f8" model.  Where two launches are the same computation they must be bit-identical.
Measured ratios, per family: profiles/r20a_attention_forward_edge_tests.txt."""
import pytest
import torch

import attention_fwd_model as M
from test_kernels_gpu import check

pytestmark = pytest.mark.gpu

# The factor covers what the model leaves out: fp32 accumulation order, v_exp_f32, the deferred rescale (the value of
# tests/test_attention_backward_edges_gpu.py, for the same reason).
ROW_FACTOR = 4.0
PATTERN = 0x7E5A          # an fp16 NaN: an unwritten output element is not finite, a written guard element is not this pattern
NAN = float("nan")


def _r8(n):
    return (n + 7) & ~7


def kv_map_of(B, Bk):
    return [b if b < Bk else b - (B - Bk) for b in range(B)]


def expected_plan(D, B, H, Nq, Nk, mode="attn", opts=()):
    """(family, waves, stages, workgroups) from the dispatch rules: 4 waves x 3 stages at D = 40 when cdiv(Nq, 128) H B >= 512, else
    2 x 2; D = 160 splits the keys when Nq <= 256, Nk > 64 and cdiv(Nq, 32) H B <= 256."""
    cd = lambda a, b: -(-a // b)                                                                # noqa: E731
    big = cd(Nq, 128) * H * B >= 512
    if mode == "f8":
        return ("f8", 4, 3, cd(Nq, 128) * H * B) if big else ("f8", 2, 3, cd(Nq, 64) * H * B)
    if mode == "lse":
        return ("lse", 4, 3, cd(Nq, 128) * H * B)
    if D == 40:
        if big and "attn_d40_general" in opts:
            return ("general", 4, 3, cd(Nq, 128) * H * B)
        if big and "attn_lean" in opts:
            return ("lean", 4, 3, cd(Nq, 128) * H * B)
        fam = "shared_body" if "attn_d40_loop" in opts else "d40_loop"
        return (fam, 4, 3, cd(Nq, 128) * H * B) if big else (fam, 2, 2, cd(Nq, 64) * H * B)
    if D == 160 and "attn_d160" not in opts and Nq <= 256 and Nk > 64 and cd(Nq, 32) * H * B <= 256:
        return ("ksplit", 4, 1, cd(Nq, 32) * H * B)
    return ("general", 4, 3, cd(Nq, 128) * H * B)


class _Options:
    """Development options for the duration of a with block: names -> 1, except attn_d160 -> 3 (always the query-split kernel)."""

    def __init__(self, *names):
        self.names = names

    def __enter__(self):
        from storygen_amd import ops
        for n in self.names:
            ops.debug_set_option(n, 3 if n == "attn_d160" else 1)

    def __exit__(self, *exc):
        from storygen_amd import ops
        ops.debug_set_option("reset", 0)


# ------------------------------------------------------------------------------------------------ operands as windows
def _q_window(q, dev):
    B, Nq, C = q.shape
    buf = torch.full((B, Nq + 2, 3 * C), NAN, dtype=torch.float16, device=dev)
    buf[:, :Nq, C:2 * C] = q.to(dev)
    return buf[:, :Nq, C:2 * C]


def _k_window(k, dev):
    """[Bk, Nk + 3, C] view (pass nk = Nk): rows [Nk, Nk + 3) and the other columns of the [.., 2C] buffer NaN."""
    Bk, Nk, C = k.shape
    buf = torch.full((Bk, Nk + 3, 2 * C), NAN, dtype=torch.float16, device=dev)
    buf[:, :Nk, C:] = k.to(dev)
    return buf[:, :, C:]


def _vt_window(v, dev, junk=False, layout="bcn"):
    """[Bk, C, round8(Nk)] view of rows 16 columns longer; columns [Nk, round8(Nk)) zero, or +-60000 (junk: read, multiplied by an exact
    0), columns beyond NaN.  layout "cbn": the buffer is [C, Bk, .] permuted (model/attention_processor.py: batch stride < row stride)."""
    Bk, Nk, C = v.shape
    n8 = _r8(Nk)
    if layout == "cbn":
        buf = torch.full((C, Bk, n8 + 16), NAN, dtype=torch.float16, device=dev).permute(1, 0, 2)
    else:
        buf = torch.full((Bk, C, n8 + 16), NAN, dtype=torch.float16, device=dev)
    buf[:, :, :Nk] = v.to(dev).transpose(1, 2)
    buf[:, :, Nk:n8] = 0.0
    if junk and n8 > Nk:
        buf[:, 0::2, Nk:n8] = 60000.0
        buf[:, 1::2, Nk:n8] = -60000.0
    return buf[:, :, :n8]


class _Out:
    """Output window of a pattern-filled [B, Nq + 1, ldo] buffer: ldo = C + 4 (columns [0, C): rows 8-byte aligned only) or 2C (the
    column window [C, 2C))."""

    def __init__(self, B, Nq, C, dev, ldo=None):
        ldo = C + 4 if ldo is None else ldo
        self.raw = torch.full((B, Nq + 1, ldo), PATTERN, dtype=torch.int16, device=dev)
        off = 0 if ldo < 2 * C else C
        self.win = self.raw.view(torch.float16)[:, :Nq, off:off + C]
        self.mask = torch.ones_like(self.raw, dtype=torch.bool)
        self.mask[:, :Nq, off:off + C] = False

    def result(self, what):
        torch.cuda.synchronize()
        assert bool((self.raw[self.mask] == PATTERN).all()), f"{what}: wrote outside its output window"
        return self.win.contiguous()


def _launch(q, k, v, H, dev, *, mode="attn", opts=(), ldo=None, junk=False, layout="bcn", what=""):
    """One launch on windowed operands; q [B, Nq, C], k, v [Bk, Nk, C] CPU fp16.  Asserts the plan.  Returns the output [B, Nq, C] (GPU)."""
    from storygen_amd import ops
    B, Nq, C = q.shape
    Bk, Nk, D = k.shape[0], k.shape[1], C // H
    scale = D ** -0.5
    qw, kw, vw = _q_window(q, dev), _k_window(k, dev), _vt_window(v, dev, junk, layout)
    out = _Out(B, Nq, C, dev, ldo)
    want = expected_plan(D, B, H, Nq, Nk, mode, opts)
    with _Options(*opts):
        if mode == "f8":
            assert ops.attention_f8_plan(B, H, Nq) == want, (what, ops.attention_f8_plan(B, H, Nq), want)
            nbytes = ops.attention_f8_bytes(B, H, Nq, False) + ops.attention_f8_bytes(Bk, H, Nk, False) + ops.attention_f8_bytes(Bk, H, Nk, True) + 4096
            scratch = torch.full((nbytes,), 0x7F, dtype=torch.uint8, device=dev)          # 0x7F = NaN in e4m3: padding must not leak
            ops.attention_f8(qw, kw, vw, out.win, H, scale, scratch, nk=Nk)
        elif mode == "lse":
            got = ops.attention_plan(qw, kw, vw, out.win, H, scale, nk=Nk, lse=True)
            assert got == want, (what, got, want)
            lse2 = torch.full((B, H, Nq), NAN, dtype=torch.float32, device=dev)
            ops.attention_lse(qw, kw, vw, out.win, lse2, H, scale, nk=Nk)
            assert bool(torch.isfinite(lse2).all()), f"{what}: lse2"
        else:
            got = ops.attention_plan(qw, kw, vw, out.win, H, scale, nk=Nk)
            assert got == want, (what, got, want)
            ops.attention(qw, kw, vw, out.win, H, scale, nk=Nk)
    return out.result(what)


def _assert_bars(got, q, k, v, H, what, *, family, kv_map=None, nk=None, bar=(1e-3, 3e-3)):
    """Every assertion of the module docstring on one output; prints the case's line; returns kernel / model row ratio."""
    D = q.shape[-1] // H
    got = got.cpu()
    ex = M.exact(q, k, v, H, D ** -0.5, kv_map=kv_map, nk=nk)
    rd = M.rounded(q, k, v, H, D ** -0.5, kv_map=kv_map, nk=nk, path=M.path_of(family, D))
    assert bool(torch.isfinite(got.float()).all()), f"{what}: output not finite"
    l2 = M.rel_l2(got, ex)
    mx = float((got.double() - ex).abs().max() / ex.abs().max())
    rk, rm = M.max_row_error(got.double(), ex, H), M.max_row_error(rd, ex, H)
    ratio = rk / rm if rm > 0 else (0.0 if rk == 0 else float("inf"))
    print(f"FWD-EDGE {what} [{family}]: rel-L2 {l2:.1e} (model {M.rel_l2(rd, ex):.1e}) max {mx:.1e} row {rk:.1e} / model {rm:.1e} = {ratio:.2f}")
    if family == "f8":
        assert l2 <= 8e-2, f"{what}: fp8 aggregate {l2:.2e} > 8e-2"
    else:
        check(got, ex, what, l2=bar[0], mx=bar[1])
    assert rk <= ROW_FACTOR * rm, f"{what}: worst row {rk:.2e} > {ROW_FACTOR:g} x the rounded model's {rm:.2e}"
    return ratio


def _case(q, k, v, H, dev, what, *, bar=(1e-3, 3e-3), **kw):
    B, Bk = q.shape[0], k.shape[0]
    D, Nq, Nk = q.shape[-1] // H, q.shape[1], k.shape[1]
    family = expected_plan(D, B, H, Nq, Nk, kw.get("mode", "attn"), kw.get("opts", ()))[0]
    got = _launch(q, k, v, H, dev, what=what, **kw)
    _assert_bars(got, q, k, v, H, what, family=family, kv_map=kv_map_of(B, Bk), bar=bar)
    return got


# ------------------------------------------------------------------------------------------------ A. tile counts, ragged tails, dispatch
NKS = [1, 7, 63, 64, 65, 72, 127, 128, 129, 191, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 512, 513, 577]
NQS = [7, 32, 33, 130, 256, 257]
# pairwise: every head dim meets every Nk and every Nq; H 8 / 3 and the batch counts alternate (B 5 with the small query counts only)
TILE_CASES = [(D, (1, 2, 5)[(i + di) % 3] if NQS[(i + 2 * di) % 6] <= 33 else (1, 2)[(i + di) % 2], (8, 3)[(i + di) % 2], NQS[(i + 2 * di) % 6], nk)
              for di, D in enumerate((80, 160)) for i, nk in enumerate(NKS)]
# D = 160: one more key-split case per tile count that the pairwise list ran on the query-split kernel, and 12 tiles
TILE_CASES += [(160, 2, 3, 33, nk) for nk in (129, 193, 257, 321, 385, 449, 513, 577, 768)]
assert all({c[3] for c in TILE_CASES if c[0] == D} == set(NQS) and {c[4] for c in TILE_CASES if c[0] == D} >= set(NKS) for D in (80, 160))
assert {-(-c[4] // 64) for c in TILE_CASES if expected_plan(*c)[0] == "ksplit"} >= set(range(2, 10)) | {12}
assert any(c[3] < 32 and expected_plan(*c)[0] == "ksplit" for c in TILE_CASES)


@pytest.mark.parametrize("D,B,H,Nq,Nk", TILE_CASES)
def test_tile_counts_and_ragged_tails(gpu, D, B, H, Nq, Nk):
    q, k, v = M.make_inputs("normal", B, H, D, Nq, Nk)
    _case(q, k, v, H, gpu, f"normal D{D} B{B} H{H} Nq{Nq} Nk{Nk}")


# each dispatch threshold on both sides: Nk 64 / 65, Nq 256 / 257, 256 workgroups / more (D = 160); 512 workgroups of 4 waves (D = 40)
THRESHOLDS = [(160, 4, 8, 256, 64, "general"), (160, 4, 8, 256, 65, "ksplit"), (160, 1, 8, 256, 130, "ksplit"), (160, 1, 8, 257, 130, "general"),
              (160, 5, 8, 256, 65, "general"), (160, 20, 8, 256, 256, "general"),
              (40, 16, 8, 512, 130, "d40_loop"), (40, 16, 8, 384, 130, "d40_loop"), (40, 16, 8, 390, 130, "d40_loop")]


@pytest.mark.parametrize("D,B,H,Nq,Nk,family", THRESHOLDS)
def test_both_sides_of_every_dispatch_threshold(gpu, D, B, H, Nq, Nk, family):
    plan = expected_plan(D, B, H, Nq, Nk)
    assert plan[0] == family
    if D == 40:
        assert plan[1:3] == ((2, 2) if Nq == 384 else (4, 3))          # Nq 390: waves 1..3 of the last workgroup own no query
    q, k, v = M.make_inputs("normal", B, H, D, Nq, Nk, seed=1)
    _case(q, k, v, H, gpu, f"threshold D{D} B{B} H{H} Nq{Nq} Nk{Nk}")


# ------------------------------------------------------------------------------------------------ B. pairs
def _pair_problem(q, k, v, dev, nk, short=None):
    """(operand tuple for ops.attention_pair / ops.attention, _Out)"""
    B, Nq, C = q.shape
    out = _Out(B, Nq, C, dev, 2 * C)
    if short is not None:                       # the flat [C, T] layout: short rows in front of the long ones (ops.attention's `short`)
        ks, vs = short
        hw, T = ks.shape[1], ks.shape[1] + k.shape[1]
        kflat = torch.cat([ks[0], k[0]]).to(dev)
        vt = torch.cat([vs[0], v[0]]).to(dev).t().contiguous()
        k_s, k_l = kflat[:hw].view(1, hw, C), kflat[hw:].view(1, T - hw, C)
        vt_s = vt[:, :hw].unflatten(1, (1, hw)).permute(1, 0, 2)
        vt_l = vt[:, hw:].unflatten(1, (1, T - hw)).permute(1, 0, 2)
        return (_q_window(q, dev), k_l, vt_l, out.win, None, (k_s, vt_s)), out
    return (_q_window(q, dev), _k_window(k, dev), _vt_window(v, dev), out.win, nk), out


# D, H, B, Nq, (Nk, Bk) of problem 0, (Nk, Bk) of problem 1, short rows in problem 0.  na % 8 != 0 (H 3 / 5); equal Nk; the short problem
# passed first; different kv_batches per problem; short rows (k2); D = 160 whose singles would split the keys
PAIRS = [(40, 3, 3, 200, (77, 3), (130, 2), 0), (40, 5, 2, 72, (129, 2), (129, 1), 0), (40, 8, 16, 512, (130, 8), (77, 16), 0),
         (80, 3, 3, 130, (77, 3), (320, 2), 0), (80, 5, 1, 33, (65, 1), (65, 1), 0), (80, 8, 3, 200, (144, 2), (77, 3), 72),
         (160, 3, 3, 64, (192, 2), (77, 3), 0), (160, 5, 2, 33, (77, 2), (257, 1), 0), (160, 8, 3, 40, (80, 2), (77, 3), 40),
         (40, 8, 3, 96, (160, 2), (77, 3), 40)]


@pytest.mark.parametrize("D,H,B,Nq,p0,p1,hw", PAIRS)
def test_pairs_are_their_two_launches_bit_for_bit(gpu, D, H, B, Nq, p0, p1, hw):
    from storygen_amd import ops
    scale = D ** -0.5
    probs = []
    for i, (Nk, Bk) in enumerate((p0, p1)):
        q, k, v = M.make_inputs("normal", B, H, D, Nq, Nk, seed=10 + i, Bk=Bk)
        short = None
        if hw and i == 0:                       # K/V rows [short (hw keys) | long (Nk keys)]: Bk = 2
            ks, vs = M.make_inputs("normal", 1, H, D, 1, hw, seed=20)[1:]
            short, k, v = (ks, vs), k[:1], v[:1]
        probs.append((q, k, v, short))
    args = [_pair_problem(q, k, v, gpu, k.shape[1], short) for q, k, v, short in probs]
    shared, first, pl0, pl1, wgs = ops.attention_pair_plan(args[0][0], args[1][0], H, scale)
    big = -(-Nq // 128) * H * B >= 512
    fam = ("d40_loop", 4, 3) if D == 40 and big else ("d40_loop", 2, 2) if D == 40 else ("general", 4, 3)
    sub = -(-Nq // (32 * fam[1])) * H * B
    assert (shared, first, pl0, pl1, wgs) == (True, 0 if p0[0] >= p1[0] else 1, fam + (sub,), fam + (sub,), 2 * sub)
    ops.attention_pair(args[0][0], args[1][0], H, scale)
    paired = [o.result("pair") for _, o in args]
    for i, (q, k, v, short) in enumerate(probs):
        a, o = _pair_problem(q, k, v, gpu, k.shape[1], short)
        with _Options("attn_d160"):             # the shared grid runs the query-split kernel: the singles' default at D = 160 may split the keys
            ops.attention(*a[:4], H, scale, nk=a[4], short=a[5] if len(a) > 5 else None)
        single = o.result("single")
        assert torch.equal(paired[i].view(torch.int16), single.view(torch.int16)), f"problem {i} differs from its own launch"
        if short is None:
            _assert_bars(paired[i], q, k, v, H, f"pair D{D} H{H} B{B} Nq{Nq} problem {i} Nk{k.shape[1]} Bk{k.shape[0]}", family=fam[0],
                         kv_map=kv_map_of(B, k.shape[0]))
        else:
            _assert_bars(paired[i], q, [short[0][0], k[0]], [short[1][0], v[0]], H, f"pair D{D} H{H} B{B} Nq{Nq} problem {i} Nk{hw}|{k.shape[1]}",
                         family=fam[0], kv_map=kv_map_of(B, 2))


@pytest.mark.parametrize("D", [40, 80, 160])
def test_a_pair_of_different_query_counts_is_two_launches(gpu, D):
    from storygen_amd import ops
    H, B, scale = 3, 2, D ** -0.5
    pa = M.make_inputs("normal", B, H, D, 72, 130, seed=30)
    pb = M.make_inputs("normal", B, H, D, 40, 77, seed=31)
    (a, oa), (b, ob) = _pair_problem(*pa, gpu, 130), _pair_problem(*pb, gpu, 77)
    plan = ops.attention_pair_plan(a, b, H, scale)
    assert plan == (False, 0, expected_plan(D, B, H, 72, 130), expected_plan(D, B, H, 40, 77), 0)
    ops.attention_pair(a, b, H, scale)
    got = [oa.result("a"), ob.result("b")]
    for g, (q, k, v) in zip(got, (pa, pb)):
        single = _launch(q, k, v, H, gpu, ldo=2 * H * D)
        assert torch.equal(g.view(torch.int16), single.view(torch.int16))
        _assert_bars(g, q, k, v, H, f"two launches D{D} Nq{q.shape[1]}", family=expected_plan(D, B, H, q.shape[1], k.shape[1])[0])


# ------------------------------------------------------------------------------------------------ C. windows and poison
# every family: (D, B, H, Nq, mode, options); the big D = 40 grid for the 4-wave kernels
FAMILY_RUNS = [(40, 2, 3, 72, "attn", ()), (40, 2, 3, 72, "attn", ("attn_d40_loop",)), (40, 16, 8, 512, "attn", ()),
               (40, 16, 8, 512, "attn", ("attn_d40_loop",)), (40, 16, 8, 512, "attn", ("attn_lean",)), (40, 16, 8, 512, "attn", ("attn_d40_general",)),
               (80, 2, 3, 72, "attn", ()), (160, 2, 3, 72, "attn", ("attn_d160",)), (160, 2, 3, 72, "attn", ()),
               (40, 2, 3, 72, "lse", ()), (80, 2, 3, 72, "lse", ()), (160, 2, 3, 72, "lse", ()), (40, 2, 3, 72, "f8", ()), (40, 16, 8, 512, "f8", ())]


@pytest.mark.parametrize("Nk", [77, 65, 1, 129])
@pytest.mark.parametrize("D,B,H,Nq,mode,opts", FAMILY_RUNS)
def test_finite_junk_in_the_padding_columns_and_nan_everywhere_else(gpu, D, B, H, Nq, mode, opts, Nk):
    """V^T columns [Nk, round8(Nk)) at +-60000 (read as part of a 16-byte chunk and multiplied by an exact 0): bit-identical to zero padding;
    the [C, B, Nkp]-permuted V^T and the output as a column window (ldo = 2C) as well.  All NaN windows of _launch apply."""
    q, k, v = M.make_inputs("normal", B, H, D, Nq, Nk, seed=2, Bk=B if B == 2 else 8)
    what = f"windows D{D} B{B} H{H} Nq{Nq} Nk{Nk} {mode} {' '.join(opts)}"
    base = _case(q, k, v, H, gpu, what, mode=mode, opts=opts)
    junk = _launch(q, k, v, H, gpu, mode=mode, opts=opts, junk=True, layout="cbn", ldo=2 * H * D, what=what)
    assert torch.equal(base.view(torch.int16), junk.view(torch.int16)), f"{what}: junk padding / permuted V^T / column window changed the result"


@pytest.mark.parametrize("hw,R", [(64, 3), (40, 2), (72, 2)])
@pytest.mark.parametrize("D,opts", [(40, ()), (80, ()), (160, ()), (160, ("attn_d160",))])
def test_short_rows_in_the_flat_layout(gpu, D, opts, hw, R):
    """sg_attn_desc.k2 with K/V rows [short (hw keys) | long (R hw keys)] back to back in one flat [C, T] V^T: Nk2 <= 64 < Nk (a key-split
    workgroup whose waves 1..3 own no tile), and Nk2 not a multiple of 64."""
    from storygen_amd import ops
    H, B, Nq = 3, 3, 72
    q = M.make_inputs("normal", B, H, D, Nq, 8, seed=3)[0]
    ks, vs = M.make_inputs("normal", 1, H, D, 1, hw, seed=4)[1:]
    kl, vl = M.make_inputs("normal", 1, H, D, 1, R * hw, seed=5)[1:]
    a, out = _pair_problem(q, kl, vl, gpu, None, (ks, vs))
    want = expected_plan(D, B, H, Nq, R * hw, "attn", opts)
    with _Options(*opts):
        assert ops.attention_plan(*a[:4], H, D ** -0.5, nk=None, short=a[5]) == want
        ops.attention(*a[:4], H, D ** -0.5, short=a[5])
    _assert_bars(out.result("short rows"), q, [ks[0], kl[0]], [vs[0], vl[0]], H, f"short rows D{D} {hw}|{R * hw} {' '.join(opts)}",
                 family=want[0], kv_map=kv_map_of(B, 2))


# ------------------------------------------------------------------------------------------------ D. exact selection
SELECT_RUNS = [(40, 3, 3, 96, [130, 77], "attn", ()), (40, 3, 3, 96, [130, 77], "attn", ("attn_d40_loop",)), (40, 16, 8, 512, [193] * 8, "attn", ()),
               (40, 16, 8, 512, [193] * 8, "attn", ("attn_d40_loop",)), (40, 16, 8, 512, [193] * 8, "attn", ("attn_lean",)),
               (40, 16, 8, 512, [193] * 8, "attn", ("attn_d40_general",)), (80, 3, 8, 136, [321, 65], "attn", ()),
               (160, 3, 3, 136, [577, 72], "attn", ("attn_d160",)), (160, 3, 3, 136, [577, 72], "attn", ()), (160, 2, 3, 7, [577, 129], "attn", ()),
               (40, 3, 3, 96, [130, 77], "lse", ()), (80, 3, 3, 96, [130, 77], "lse", ()), (160, 3, 3, 96, [130, 77], "lse", ()),
               (40, 3, 3, 96, [130, 77], "f8", ()), (40, 16, 8, 512, [193] * 8, "f8", ()), (40, 1, 8, 40, [1], "attn", ())]


@pytest.mark.parametrize("D,B,H,Nq,nks,mode,opts", SELECT_RUNS)
def test_one_hot_rows_select_their_value_row_bit_for_bit(gpu, D, B, H, Nq, nks, mode, opts):
    """Key indexing, the in-tile permutations, tail masking and the K/V-row map, bit for bit (inputs: M.selector_inputs).  Why exact: the
    selected logit exceeds every other by >= 29 log2 units, so every other P is <= 2^-29 of it — 0 after the fp16 / e4m3(128 P) cast where it
    is computed against the final maximum, and where it was accumulated against an earlier (stale or per-wave) maximum, rescaled in fp32 to
    at most Nk * 2^-29 * max|V| / min|V| = 768 * 2^-29 * 15 = 2e-5 of the selected value.  The selected P is exp2 of at most 2^-22 |m|
    (the fp32 / fp16 hi + lo maximum), which rounds to 1 in fp16 and to 128 in e4m3; V * P is exact in fp32; 1 / l carries the same 1e-5.  All
    of it is below the 2^-12 = 2.4e-4 that rounds back to the fp16 V (the CPU rounded model returns V bit for bit on every path).  K rows
    [Nk, Nk + 3) are NaN (_k_window): a key read past the end would win.  One launch per distinct key count of `nks`, every K/V row of
    it with that count (rows of different length in one launch: test_short_rows_select)."""
    Bk = len(nks)
    kvm = kv_map_of(B, Bk)
    for n in sorted(set(nks), reverse=True):
        q, ks, vs, t = M.selector_inputs(B, H, D, Nq, [n] * Bk, kvm, seed=n)
        got = _launch(q, torch.stack(ks), torch.stack(vs), H, gpu, mode=mode, opts=opts, what=f"select D{D} Nk{n}")
        want = M.selected_values(vs, t, kvm).to(gpu)
        bad = (got.view(torch.int16) != want.view(torch.int16)).any(-1).nonzero()
        print(f"FWD-EDGE select D{D} B{B} H{H} Nq{Nq} Nk{n} {mode} {' '.join(opts)} [{expected_plan(D, B, H, Nq, n, mode, opts)[0]}]: "
              f"{bad.shape[0]} wrong rows")
        assert bad.shape[0] == 0, f"rows (batch, query) {bad[:8].tolist()} are not the selected V row (targets {[int(t[b, i]) for b, i in bad[:8].tolist()]})"


@pytest.mark.parametrize("D,opts", [(40, ()), (80, ()), (160, ()), (160, ("attn_d160",))])
def test_short_rows_select(gpu, D, opts):
    from storygen_amd import ops
    H, B, Nq, nks = 3, 3, 96, [40, 136]
    kvm = kv_map_of(B, 2)
    q, ks, vs, t = M.selector_inputs(B, H, D, Nq, nks, kvm, seed=9)
    a, out = _pair_problem(q, ks[1][None], vs[1][None], gpu, None, (ks[0][None], vs[0][None]))
    with _Options(*opts):
        assert ops.attention_plan(*a[:4], H, D ** -0.5, nk=None, short=a[5]) == expected_plan(D, B, H, Nq, 136, "attn", opts)
        ops.attention(*a[:4], H, D ** -0.5, short=a[5])
    assert torch.equal(out.result("short select").view(torch.int16), M.selected_values(vs, t, kvm).to(gpu).view(torch.int16))


# ------------------------------------------------------------------------------------------------ E. range edges beyond D = 40
RANGE_RUNS = [(80, 2, 64, 320, ()), (160, 2, 64, 640, ("attn_d160",)), (160, 2, 64, 640, ())]


@pytest.mark.parametrize("family", ["late_key", "wave_keys", "creep", "offset_neg", "offset_pos"])
@pytest.mark.parametrize("D,B,Nq,Nk,opts", RANGE_RUNS)
def test_range_families(gpu, family, D, B, Nq, Nk, opts):
    """A dominating key in every late tile (key-split: in each wave's tile of every round, wave 0's first tile included, rows whose keys are
    tiny in three waves), maxima creeping by under 6 log2 units per tile and then jumping, common logit shifts of -40 / +25 whose maximum
    moves at a tile boundary: the general softmax keeps an fp32 maximum and holds the default bars."""
    q, k, v = M.make_inputs(family, B, 8, D, Nq, Nk)
    _case(q, k, v, 8, gpu, f"{family} D{D} B{B} Nq{Nq} Nk{Nk} {' '.join(opts)}", opts=opts)


@pytest.mark.parametrize("family", ["late_key", "wave_keys", "creep", "offset_neg", "offset_pos"])
@pytest.mark.parametrize("D,Nk", [(40, 448), (80, 320), (160, 640)])
def test_range_families_in_a_paired_launch(gpu, family, D, Nk):
    """The same inputs as problem 0 of a pair (problem 1: 77 text keys).  D = 40 runs the fast path: 2e-3 / 6e-3 under the logit offsets."""
    from storygen_amd import ops
    H, B, Nq = 8, 2, 64
    q, k, v = M.make_inputs(family, B, H, D, Nq, Nk)
    qt, kt, vt = M.make_inputs("normal", B, H, D, Nq, 77, seed=40)
    (a, oa), (b, ob) = _pair_problem(q, k, v, gpu, Nk), _pair_problem(qt, kt, vt, gpu, 77)
    assert ops.attention_pair_plan(a, b, H, D ** -0.5)[:2] == (True, 0)
    ops.attention_pair(a, b, H, D ** -0.5)
    fam = "d40_loop" if D == 40 else "general"
    bar = (2e-3, 6e-3) if D == 40 and family.startswith("offset") else (1e-3, 3e-3)
    _assert_bars(oa.result("a"), q, k, v, H, f"pair {family} D{D} Nk{Nk}", family=fam, bar=bar)
    _assert_bars(ob.result("b"), qt, kt, vt, H, f"pair {family} D{D} text", family=fam)


# ------------------------------------------------------------------------------------------------ F. fp8
F8_NKS = [1, 63, 64, 65, 127, 129, 257, 449]
F8_CASES = [((1, 1), (3, 2), (2, 2))[i % 3] + ((8, 3)[i % 2], (7, 64, 65, 200)[i % 4], nk) for i, nk in enumerate(F8_NKS)] + [(16, 8, 8, 512, 129)]


@pytest.mark.parametrize("B,Bk,H,Nq,Nk", F8_CASES)
def test_fp8_tiles_tails_and_shared_rows(gpu, B, Bk, H, Nq, Nk):
    q, k, v = M.make_inputs("normal", B, H, 40, Nq, Nk, seed=6, Bk=Bk)
    q, k = (q.float() / 1.5).to(torch.float16), (k.float() / 1.5).to(torch.float16)          # unit variance, as test_attention_fp8_d40
    _case(q, k, v, H, gpu, f"fp8 B{B} Bk{Bk} H{H} Nq{Nq} Nk{Nk}", mode="f8")
