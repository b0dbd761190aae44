"""Host tests of the fused GEGLU feed-forward's weight stream (storygen_amd.repack.ff_fused_pack) and of the CPU model the GPU edge
module measures against (tests/ff_fused_model.py).  No GPU.

  * pack round trip: ff_fused_model.unpack — the stream read back through the KERNEL's address formulas — returns what was packed, for
    random weights and for index-coded ones (a misplaced row, slot, slab or chunk names itself);
  * the model against the fp32 torch reference of tests/test_kernels_gpu.py::test_fused_geglu_feed_forward on that test's inputs;
  * ff_fused_pack refuses a d1 that is not finite in fp16;
  * every input maker of the GPU edge module (see tests/ff_fused_model.py) runs here (each asserts the condition the GPU bar relies on), and the rounded
    model — a correct kernel's unavoidable error — meets the GPU module's aggregate bars on those inputs."""
import pytest
import torch
import torch.nn.functional as F

import ff_fused_model as FM
from conftest import max_rel
from storygen_amd.repack import ff_fused_layout, ff_fused_pack, fold_layernorm, interleave_geglu

C = FM.C
D1_REL = 2.0 ** -21            # hi + lo against d1
D1_FLOOR = 2.0 ** -25          # half the fp16 subnormal spacing: all a (hi, lo) pair of fp16 values can do once lo is subnormal,
D1_FLOOR_BELOW = 2.0 ** -4     # which it is for |d1| < 2^-3 (ulp(hi) <= 2^-14); D1_FLOOR <= D1_REL |d1| from |d1| = 2^-4 on


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_d1(got, d1, what):
    err, mag = (got - d1.double()).abs(), d1.double().abs()
    big = mag >= D1_FLOOR_BELOW
    assert bool((err[big] <= D1_REL * mag[big]).all()), f"{what}: hi + lo misses d1 by more than 2^-21 relative"
    assert bool((err[~big] <= D1_FLOOR).all()), f"{what}: hi + lo misses a small d1 by more than 2^-25"


def _folded(w):
    w1i, b1i = interleave_geglu(w["w1"], w["b1"])
    w1f, _, d1 = fold_layernorm(w1i, b1i, w["gamma"], w["beta"])
    return w1f.contiguous(), d1.contiguous()


def _coded(shape, code):
    """fp16 tensor whose element (r, c) has the bit pattern 0x0C00 + code(r, c): positive normal numbers >= 2^-12 — distinct codes are
    distinct values, and halving them is exact."""
    r = torch.arange(shape[0]).view(-1, 1).expand(shape)
    c = torch.arange(shape[1]).view(1, -1).expand(shape)
    v = code(r, c) + 0x0C00
    assert int(v.max()) < 0x7C00
    return v.to(torch.int16).contiguous().view(torch.float16)


def _weight_sets():
    w = FM.weights(0)
    w1f, d1 = _folded(w)
    yield "random", w1f, d1, w["w2"]
    # fp16 has fewer values than W1 has elements: two codings, one naming the row (chunk, tile, permuted row), one the position in the
    # row together with the row inside its chunk — an element in the wrong place is wrong in at least one of them
    d1c = ((torch.arange(8 * C, dtype=torch.float64) + 1.0) * 1.0001).to(torch.float32)           # distinct, >= 1, every lo half non-zero
    yield "coded by row", _coded((8 * C, C), lambda r, c: r), d1c, _coded((C, 4 * C), lambda r, c: c)
    yield "coded by column", _coded((8 * C, C), lambda r, c: c + C * (r % 64)), -d1c.flip(0), _coded((C, 4 * C), lambda r, c: r + C * (c % 32))


@pytest.mark.parametrize("name", ["random", "coded by row", "coded by column"], ids=lambda v: v.replace(" ", "_"))
def test_pack_round_trip(name):
    w1f, d1, w2 = next(s[1:] for s in _weight_sets() if s[0] == name)
    stream = ff_fused_pack(w1f, d1, w2)
    L = ff_fused_layout(C)
    assert stream.dtype == torch.uint8 and stream.dim() == 1
    assert stream.numel() == L["chunks"] * L["chunk"]
    assert stream.numel() == (4 * C // 32) * ((C // 64) * 8192 + 64 * 32 + C * 64)               # sg_ff_fused_pack_bytes(320)
    assert FM.stream_sizes(C) == (L["chunks"], L["w1_img"], L["w1_part"], L["w2_part"], L["chunk"])
    g1, gd, g2, pad = FM.unpack(stream, C, pad=True)
    bad = (_bits(g1) != _bits(w1f)).nonzero()
    assert bad.numel() == 0, f"{name}: W1f differs first at interleaved (row, column) {bad[0].tolist()} of {bad.shape[0]} elements"
    half = (w2 * 0.5).half()
    bad = (_bits(g2) != _bits(half)).nonzero()
    assert bad.numel() == 0, f"{name}: W2 / 2 differs first at (column, hidden unit) {bad[0].tolist()} of {bad.shape[0]} elements"
    _assert_d1(gd, d1, name)
    assert bool((_bits(pad) == 0).all()), f"{name}: the zero padding of the d1 k-step is not zero"
    if name != "random":
        assert bool((gd != d1.to(torch.float16).double()).all()), "the coded d1 is meant to need its lo half"


def test_model_matches_the_fp32_reference_of_the_gpu_test():
    """tests/test_kernels_gpu.py::test_fused_geglu_feed_forward's inputs (M = 128) and its torch fp32 reference, on the CPU."""
    def rnd(shape, scale=1.0, seed=0, dtype=torch.float16):
        g = torch.Generator().manual_seed(seed)
        return (torch.randn(shape, generator=g) * scale).to(dtype)
    M = 128
    xbig = rnd((M, 2 * C), 1.5, 1, torch.float32) + 0.4
    x = xbig[:, C // 2: C // 2 + C]
    w1, b1 = rnd((8 * C, C), C ** -0.5, 2), rnd((8 * C,), 0.5, 3)
    w2, b2 = rnd((C, 4 * C), (4 * C) ** -0.5, 4), rnd((C,), 0.5, 5)
    gamma, beta = rnd((C,), 0.2, 6) + 1.0, rnd((C,), 0.2, 7)
    h = F.layer_norm(x.float(), (C,), gamma.float(), beta.float(), 1e-5) @ w1.float().t() + b1.float()
    ref = (h[:, : 4 * C] * F.gelu(h[:, 4 * C:])) @ w2.float().t() + b2.float() + x
    ex = FM.exact(x, w1, b1, gamma, beta, w2, b2, 1e-5)
    rd = FM.rounded(x, w1, b1, gamma, beta, w2, b2, 1e-5)
    assert FM.rel_l2(ref, ex) <= 1e-6 and max_rel(ref, ex) <= 1e-5                   # fp32 arithmetic against float64
    assert FM.rel_l2(rd, ex) <= 1e-3 and max_rel(rd, ex) <= 3e-3                     # the GPU test's bar is reachable
    a, b = FM.exact(x, w1, b1, gamma, beta, w2, b2, 1e-5, halves=True)
    assert FM.rel_l2(a + b, ex) <= 1e-14
    ra, rb = FM.rounded(x, w1, b1, gamma, beta, w2, b2, 1e-5, halves=True)
    assert FM.rel_l2(ra, a) <= 1e-3 and FM.rel_l2(rb, b) <= 1e-3
    # the second half carries neither bias nor residual: with W2's second half zeroed it is zero, and the first is the whole result
    w2z = w2.clone()
    w2z[:, 2 * C:] = 0
    a0, b0 = FM.exact(x, w1, b1, gamma, beta, w2z, b2, 1e-5, halves=True)
    assert float(b0.abs().max()) == 0.0 and FM.rel_l2(a0, a) <= 1e-14


@pytest.mark.parametrize("bad", [65520.0, -65520.0, 7.0e4, float("inf"), float("-inf"), float("nan")])
def test_pack_refuses_d1_beyond_fp16(bad):
    w = FM.weights(1)
    w1f, d1 = _folded(w)
    d1[1234] = bad
    with pytest.raises(ValueError, match=r"ff_fused_pack: d1 .* must be finite in fp16"):
        ff_fused_pack(w1f, d1, w["w2"])


def test_pack_keeps_d1_just_below_the_limit():
    w = FM.weights(1)
    w1f, d1 = _folded(w)
    edge = torch.nextafter(torch.tensor(65520.0), torch.tensor(0.0))
    d1[0], d1[77], d1[8 * C - 1] = edge, -edge, 65504.0
    got = FM.unpack(ff_fused_pack(w1f, d1, w["w2"]), C)[1]
    assert bool(torch.isfinite(got).all())
    _assert_d1(got, d1, "just below 65520")
    for i in (0, 77, 8 * C - 1):
        assert abs(float(got[i]) - float(d1[i])) <= D1_REL * abs(float(d1[i]))


# ------------------------------------------------------------------------------------------------ the inputs of the GPU module
def _bars(x, w, eps=1e-5):
    args = (x, w["w1"], w["b1"], w["gamma"], w["beta"], w["w2"], w["b2"], eps)
    ex, rd = FM.exact(*args), FM.rounded(*args)
    assert bool(torch.isfinite(rd).all())
    assert FM.rel_l2(rd, ex) <= 1e-3 and max_rel(rd, ex) <= 1e-2
    for e, r in zip(FM.exact(*args, halves=True), FM.rounded(*args, halves=True)):
        assert FM.rel_l2(r, e) <= 1e-3 and max_rel(r, e) <= 1e-2
    return ex


def test_small_residual_inputs():
    w = FM.weights(0)
    x = FM.small_residual(1024, w)                                   # asserts ||FF|| >= 10 ||x||
    ff = FM.ff_term(x, w)
    assert float(ff.norm()) >= 10.0 * float(x.double().norm())
    assert float(ff[:1].norm()) >= 5.0 * float(x[:1].double().norm())           # M = 1 is a prefix: its one row, too, is mostly FF
    _bars(x, w)
    assert len({tuple(r.tolist()) for r in x[:160]}) == 160                     # position independence wants distinct rows


@pytest.mark.parametrize("kind", ["constant", "mean1e4", "tiny_var", "outlier"])
def test_layernorm_edge_inputs(kind):
    w = FM.weights(0)
    _bars(FM.layernorm_edge(kind, w), w)


@pytest.mark.parametrize("eps", [1e-12, 1e-5, 1e-2, 1.0])
def test_eps_inputs(eps):
    w = FM.weights(0)
    _bars(FM.small_residual(40, w), w, eps)


@pytest.mark.parametrize("sweep", ["gate", "value"])
def test_probe_inputs(sweep):
    a, g = FM.probe_d1(sweep)                                        # asserts finite, in range
    for req in FM.GATES_REQUIRED:
        assert bool(((g == req) & (torch.signbit(g) == (str(req)[0] == "-"))).any()), req
    assert float(g.min()) == -10.0 and float(g.max()) == 10.0
    if sweep == "value":
        for v in (0.5, 3.0, 100.0):
            assert bool((a == v).any()) and bool((a == -v).any())
        assert bool((a.to(torch.float16).float() != a).any())        # some values need the lo half
    want = a.double() * FM.gelu_erf(g)
    tol = FM.probe_tolerance(a, g)
    x = torch.zeros(32, C, dtype=torch.float32)
    caught_lo = 0
    for quarter in range(4):
        w = FM.probe_weights(a, g, quarter)
        j = torch.arange(C * quarter, C * quarter + C)
        args = (w["w1"], w["b1"], w["gamma"], w["beta"], w["w2"], w["b2"], 1e-5)
        ex, rd = FM.exact(x, *args), FM.rounded(x, *args)
        assert bool((ex[0] - want[j]).abs().max() <= 1e-12)          # column j mod 320 is hidden unit j
        assert bool(((rd - want[j]).abs() <= tol[j]).all()), "the probe's tolerance must hold for the rounded model"
        # a pack without the lo half of d1 is out of tolerance somewhere in every quarter
        hi = dict(w, b1=w["b1"].to(torch.float16).float())
        miss = (FM.rounded(x, hi["w1"], hi["b1"], *args[2:])[0] - want[j]).abs() > tol[j]
        caught_lo += int(miss.sum())
        assert bool(miss.any()), f"quarter {quarter}: the probe cannot see a dropped lo half"
    print(f"probe {sweep}: {caught_lo} of {4 * C} hidden units out of tolerance without the lo half of d1")


def test_range_inputs():
    x = torch.zeros(32, C, dtype=torch.float32)
    a, g = FM.range_d1(30000.0)
    w = FM.probe_weights(a, g, 0)
    args = (w["w1"], w["b1"], w["gamma"], w["beta"], w["w2"], w["b2"], 1e-5)
    assert 30000.0 < FM.HIDDEN_LIMIT == 32752.0 < 40000.0
    rd = FM.rounded(x, *args)
    assert bool((rd == 30000.0).all()) and FM.rel_l2(rd, FM.exact(x, *args)) <= 1e-12
    for level, finite in ((32752.0, True), (32768.0, False), (40000.0, False)):
        a, g = FM.range_d1(level, hot=(7,))
        w = FM.probe_weights(a, g, 0)
        args = (w["w1"], w["b1"], w["gamma"], w["beta"], w["w2"], w["b2"], 1e-5)
        ex, rd = FM.exact(x, *args), FM.rounded(x, *args)
        assert abs(float(ex[0, 7]) - level) < 1e-9 and bool(torch.isfinite(ex).all())
        assert bool(torch.isfinite(rd).all()) == finite, level
        if finite:
            assert float(rd[0, 7]) == level
        else:
            assert bool(torch.isinf(rd[:, 7]).all()) and bool(torch.isnan(rd[:, :7]).all()) and bool(torch.isnan(rd[:, 8:]).all())
