"""The attention training pipeline at its shape, stride and range edges: ops.attention_lse -> attention_bwd_prep -> attention_bwd_dq ->
attention_bwd_dkv, the transposed operands from ops.transpose_batched on inputs padded to a multiple of 8 (train_blocks._tr_batched),
against the float64 `exact` of tests/attention_bwd_model.py.

Bars (per case): everything finite; o at the forward bar (check(): rel-L2 1e-3, max 3e-3); max |lse2 - exact| <= 2e-3; ld2[..., 0]
bit-equal to lse2; delta, dq, dk, dv aggregate rel-L2 <= 5e-3 (all as tests/test_backward_gpu.py::test_attention_backward) — and PER ROW:
    e_row = ||got_row - exact_row|| / RMS over the rows of ||exact_row||   per (batch, head); rows = queries for dq, keys for dk / dv
    max e_row(kernel) <= ROW_FACTOR x max e_row(rounded model) on the same inputs,
the rounded model being the reference plus the kernel's documented roundings (never the kernel).  An aggregate over [B, N, C] does not
see a few wrong rows (tests/test_attention_bwd_model.py::test_row_metric_sees_one_wrong_row_that_the_aggregate_misses).
Measured ratios, per family: profiles/r10a_backward_edge_tests.txt."""
import pytest
import torch

import attention_bwd_model as M
from test_kernels_gpu import check

pytestmark = pytest.mark.gpu

H = 8
# The factor covers what the model leaves out: fp32 MFMA accumulation order, v_exp_f32, the fp16 rounding of scale * acc.
ROW_FACTOR = 4.0


def _pad8(x, fill=0.0):
    B, N, C = x.shape
    Np = (N + 7) // 8 * 8
    if Np == N:
        return x
    xp = torch.full((B, Np, C), fill, dtype=x.dtype, device=x.device)
    xp[:, :N] = x
    return xp


def _tr(x, extra=0, beyond=0.0):
    """[B, N, C] -> the transposed operand [B, C, N rounded up to 8] (zero padded), as train_blocks._tr_batched makes it; extra > 0: as a
    view of a [B, C, N8 + extra] buffer whose other columns hold `beyond`."""
    from storygen_amd import ops
    xp = _pad8(x)
    B, Np, C = xp.shape
    buf = torch.full((B, C, Np + extra), beyond, dtype=torch.float16, device=x.device)
    ops.transpose_batched(xp, buf[:, :, :Np])
    return buf[:, :, :Np]


def _pipeline(q, k, v, do, *, dkv=True, kt=None, vt=None, qt=None, dot=None, dq=None, dkt=None, dvt=None):
    """The trainer's four launches.  Returns o, lse2, ld2, dq and (dkv) dkt, dvt."""
    from storygen_amd import ops
    B, Nq, C = q.shape
    Nk, D = k.shape[1], C // H
    scale = D ** -0.5
    dev = q.device
    kt = _tr(k) if kt is None else kt
    vt = _tr(v) if vt is None else vt
    r = {}
    r["o"] = torch.full((B, Nq, C), float("nan"), dtype=torch.float16, device=dev)
    r["lse2"] = torch.full((B, H, Nq), float("nan"), dtype=torch.float32, device=dev)
    ops.attention_lse(q, k, vt, r["o"], r["lse2"], H, scale, nk=Nk)
    r["ld2"] = torch.full((B, H, Nq, 2), float("nan"), dtype=torch.float32, device=dev)
    ops.attention_bwd_prep(r["o"], do, r["lse2"], r["ld2"], H)
    r["dq"] = torch.full((B, Nq, C), float("nan"), dtype=torch.float16, device=dev) if dq is None else dq
    ops.attention_bwd_dq(q, k, kt, v, do, r["ld2"], r["dq"], H, scale)
    if dkv:
        qt = _tr(q) if qt is None else qt
        dot = _tr(do) if dot is None else dot
        r["dkt"] = torch.full((B, C, Nk), float("nan"), dtype=torch.float16, device=dev) if dkt is None else dkt
        r["dvt"] = torch.full((B, C, Nk), float("nan"), dtype=torch.float16, device=dev) if dvt is None else dvt
        ops.attention_bwd_dkv(q, qt, k, v, do, dot, r["ld2"], r["dkt"], r["dvt"], H, scale)
    torch.cuda.synchronize()
    return r


def _same(a, b, what):
    """bit-identical, NaNs included (none are expected; a NaN must not compare equal to a number by accident)"""
    for n in a:
        assert torch.equal(a[n].view(torch.int16 if a[n].dtype == torch.float16 else torch.int32),
                           b[n].view(torch.int16 if b[n].dtype == torch.float16 else torch.int32)), f"{what}: {n} differs"


def _assert_case(r, cpu_inputs, what, *, dkv=True, aggregate=True, o_bar=(1e-3, 3e-3)):
    """Every assertion of the module docstring for one run of the pipeline.  Returns the per-row kernel / model ratios."""
    q, k, v, do = cpu_inputs
    B, Nq, C = q.shape
    Nk, D = k.shape[1], C // H
    ex, rd = M.exact(q, k, v, do, H), M.rounded(q, k, v, do, H)
    got = {"o": r["o"], "lse2": r["lse2"], "delta": r["ld2"][..., 1], "dq": r["dq"]}
    if dkv:
        got["dk"], got["dv"] = r["dkt"].transpose(1, 2), r["dvt"].transpose(1, 2)
    got = {n: t.cpu() for n, t in got.items()}
    for n, t in got.items():
        assert bool(torch.isfinite(t.float()).all()), f"{what}: {n} is not finite"
    check(got["o"], ex["o"], f"{what}: o", l2=o_bar[0], mx=o_bar[1])
    e_lse = float((got["lse2"].double() - ex["lse2"]).abs().max())
    assert torch.equal(r["ld2"][..., 0], r["lse2"]), f"{what}: ld2[..., 0] is not lse2"
    e_delta = M.rel_l2(got["delta"], ex["delta"])
    line = f"EDGE {what}: lse2 {e_lse:.1e} delta {e_delta:.1e}"
    assert e_lse <= 2e-3 and e_delta <= 5e-3, line
    ratios, fails = {}, []
    for n in ("dq", "dk", "dv") if dkv else ("dq",):
        zero_ref = float(ex[n].abs().max()) < 1e-12            # Nk = 1: P = 1, dP = delta, so dQ = dK = 0 identically
        if zero_ref:
            # The kernel's value is the fp32 cancellation residue of dP - delta (two sums of D products in different orders):
            # |dS| <= 2 D 2^-24 sum_d |dO_d V_d|, then |dq| <= scale |dS| |K|, |dk| <= scale sum_q |dS_q| |Q_q|.  Bar: that bound.
            doh, vh = M.heads_of(do, H), M.heads_of(v, H)
            ds = 2.0 * D * 2.0 ** -24 * (doh.abs() * vh.abs()).sum(-1)                      # [B, H, Nq]
            lim = D ** -0.5 * (ds.max() * M.heads_of(k, H).abs().max() if n == "dq" else (ds * M.heads_of(q, H).abs().amax(-1)).sum(-1).max())
            worst = float(got[n].double().abs().max())
            line += f" | {n} (exact 0) max {worst:.1e} bound {float(lim):.1e}"
            if worst > float(lim) + 6e-8:
                fails.append(f"{n}: |value| {worst:.2e} above the cancellation bound {float(lim):.2e}")
            continue
        agg = M.rel_l2(got[n], ex[n])
        rk, rm = M.max_row_error(got[n], ex[n], H), M.max_row_error(rd[n], ex[n], H)
        ratios[n] = rk / rm
        line += f" | {n} agg {agg:.1e} (model {M.rel_l2(rd[n], ex[n]):.1e}) row {rk:.1e} / model {rm:.1e} = {rk / rm:.2f}"
        if aggregate and agg > 5e-3:
            fails.append(f"{n}: aggregate rel-L2 {agg:.2e} > 5e-3")
        if rk > ROW_FACTOR * rm:
            fails.append(f"{n}: worst row {rk:.2e} > {ROW_FACTOR:g} x the rounded model's {rm:.2e}")
    print(line)
    assert not fails, f"{what}: " + "; ".join(fails)
    return ratios


def _gpu(inputs, dev):
    return tuple(t.to(dev) for t in inputs)


# ------------------------------------------------------------------------------------------------ shape families
# Nq: streamed by the dK/dV pass (1 .. 4 tiles with and without a partial last one, + 264 = 4 full + partial) and owned by the dQ pass
# (fewer than 32 rows, one wave of four, a ragged last wave).  Nk: streamed by dQ (the same tile counts + 1, 7, 65, 77, 127, 129: not
# multiples of 8) and owned by dK/dV.  Pairwise: every head dim meets every Nq and every Nk in both passes, not every (Nq, Nk) pair.
NQS = [8, 24, 32, 40, 56, 64, 72, 128, 136, 192, 200, 264]
NKS = [1, 7, 8, 31, 33, 56, 64, 65, 72, 77, 127, 128, 129, 136, 192, 200, 264, 320]
SHAPES = [(D, 1 + 2 * ((i + di) % 2), NQS[(5 * i + 4 * di) % len(NQS)], nk)
          for di, D in enumerate((40, 80, 160)) for i, nk in enumerate(NKS)]
assert all({s[2] for s in SHAPES if s[0] == D} == set(NQS) for D in (40, 80, 160))


@pytest.mark.parametrize("D,B,Nq,Nk", SHAPES)
def test_tile_counts_owned_tails_and_ragged_keys(gpu, D, B, Nq, Nk):
    cpu = M.make_inputs("normal", B, H, D, Nq, Nk)
    _assert_case(_pipeline(*_gpu(cpu, gpu)), cpu, f"normal D{D} B{B} Nq{Nq} Nk{Nk}")


@pytest.mark.parametrize("D", [40, 80, 160])
@pytest.mark.parametrize("B,Nq", [(1, 264), (3, 40)])
def test_text_keys_dq_only(gpu, D, B, Nq):
    """Nk = 77 (the text path: frozen K / V, only dQ is asked for) at every head dim."""
    cpu = M.make_inputs("normal", B, H, D, Nq, 77, seed=1)
    _assert_case(_pipeline(*_gpu(cpu, gpu), dkv=False), cpu, f"text D{D} B{B} Nq{Nq} Nk77 dq-only", dkv=False)


# ------------------------------------------------------------------------------------------------ contract and isolation
@pytest.mark.parametrize("D", [40, 80, 160])
def test_padding_the_contract_lets_the_kernels_read_may_hold_anything_finite(gpu, D):
    """K^T / V^T columns [Nk, Nk rounded up to 8) hold +-6e4 instead of zeros: every result bit-identical (the columns are read — whole
    16-byte chunks — and multiplied by an exact zero)."""
    B, Nq, Nk = 2, 136, 77
    cpu = M.make_inputs("normal", B, H, D, Nq, Nk, seed=2)
    q, k, v, do = _gpu(cpu, gpu)
    base = _pipeline(q, k, v, do)
    kt, vt = _tr(k).clone(), _tr(v).clone()
    kt[:, :, Nk:], vt[:, :, Nk:] = 6.0e4, -6.0e4
    kt[:, ::2, Nk:] *= -1
    _same(base, _pipeline(q, k, v, do, kt=kt, vt=vt), "finite padding")
    _assert_case(base, cpu, f"padding D{D}")


@pytest.mark.parametrize("D", [40, 80, 160])
@pytest.mark.parametrize("Nq,Nk", [(136, 77), (72, 200)])
def test_memory_beyond_the_rounded_up_row_is_never_read(gpu, D, Nq, Nk):
    """K^T, V^T, Q^T, dO^T as views of wider buffers (ld = N8 + 16) whose columns beyond N rounded up to 8 hold NaN."""
    B = 2
    cpu = M.make_inputs("normal", B, H, D, Nq, Nk, seed=3)
    q, k, v, do = _gpu(cpu, gpu)
    base = _pipeline(q, k, v, do)
    nan = float("nan")
    wide = _pipeline(q, k, v, do, kt=_tr(k, 16, nan), vt=_tr(v, 16, nan), qt=_tr(q, 16, nan), dot=_tr(do, 16, nan))
    for n, t in wide.items():
        assert bool(torch.isfinite(t.float()).all()), n
    _same(base, wide, "NaN beyond the rows")


@pytest.mark.parametrize("D", [40, 80, 160])
def test_strided_views_and_untouched_surroundings(gpu, D):
    """Self-attention layout: q and k are the two halves of one [B, N, 2C] buffer; v and dout column slices of wider buffers with gaps
    between the batch rows; dq into a column slice, dkt / dvt into column ranges of sentinel-filled buffers."""
    B, N, C = 3, 200, H * D
    cpu = M.make_inputs("normal", B, H, D, N, N, seed=4)
    q, k, v, do = _gpu(cpu, gpu)
    base = _pipeline(q, k, v, do)
    qk = torch.cat([q, k], dim=2)
    vbuf = torch.full((B, N + 3, C + 64), 3.0, dtype=torch.float16, device=gpu)
    dobuf = torch.full((B, N + 5, C + 32), 3.0, dtype=torch.float16, device=gpu)
    vbuf[:, :N, 32:32 + C], dobuf[:, :N, 8:8 + C] = v, do
    SENT = -7.0
    dqbuf = torch.full((B, N, C + 48), SENT, dtype=torch.float16, device=gpu)
    dkbuf, dvbuf = (torch.full((B, C, N + 24), SENT, dtype=torch.float16, device=gpu) for _ in range(2))
    got = _pipeline(qk[:, :, :C], qk[:, :, C:], vbuf[:, :N, 32:32 + C], dobuf[:, :N, 8:8 + C],
                    dq=dqbuf[:, :, 16:16 + C], dkt=dkbuf[:, :, 8:8 + N], dvt=dvbuf[:, :, 8:8 + N])
    _same(base, {n: t.contiguous() for n, t in got.items()}, "views")
    assert bool((dqbuf[:, :, :16] == SENT).all()) and bool((dqbuf[:, :, 16 + C:] == SENT).all()), "dq wrote outside its columns"
    for n, buf in (("dkt", dkbuf), ("dvt", dvbuf)):
        assert bool((buf[:, :, :8] == SENT).all()) and bool((buf[:, :, 8 + N:] == SENT).all()), f"{n} wrote outside [0, Nk)"
    _assert_case(base, cpu, f"views D{D}")


# ------------------------------------------------------------------------------------------------ range
@pytest.mark.parametrize("D,B,Nq,Nk", M.RANGE_SHAPES)
@pytest.mark.parametrize("family", ["late_key", "offset_neg", "offset_pos", "do_2p10"])
def test_range_families(gpu, family, D, B, Nq, Nk):
    """A late dominating key, a large common logit offset (o at the bar of the forward test that defines that input, 2e-3 / 6e-3:
    tests/test_attention_d40_loop_gpu.py::test_extreme_maxima_and_the_clamp), dO at the loss scale 2^10."""
    cpu = M.make_inputs(family, B, H, D, Nq, Nk)
    _assert_case(_pipeline(*_gpu(cpu, gpu)), cpu, f"{family} D{D} B{B} Nq{Nq} Nk{Nk}",
                 o_bar=(2e-3, 6e-3) if family.startswith("offset") else (1e-3, 3e-3))


@pytest.mark.parametrize("D,B,Nq,Nk", M.RANGE_SHAPES)
def test_gradients_in_the_fp16_subnormal_range(gpu, D, B, Nq, Nk):
    """dO scaled by 2^-12: dS is an fp16 subnormal.  Only the model-relative bars apply (the aggregate is printed: it is the price of
    training without a loss scale, 0.7e-3 .. 2.0e-3 in the model against 0.3e-3 for scaled gradients)."""
    cpu = M.make_inputs("do_2m12", B, H, D, Nq, Nk)
    _assert_case(_pipeline(*_gpu(cpu, gpu)), cpu, f"do_2m12 D{D} B{B} Nq{Nq} Nk{Nk}", aggregate=False)


# ------------------------------------------------------------------------------------------------ rejections
def test_rejections_launch_nothing(gpu):
    from storygen_amd import ops
    D, B, Nq, Nk = 40, 1, 64, 77
    C = H * D
    q, k, v, do = _gpu(M.make_inputs("normal", B, H, D, Nq, Nk), gpu)
    r = _pipeline(q, k, v, do)
    kt, qt, dot, ld2 = _tr(k), _tr(q), _tr(do), r["ld2"]
    SENT = -7.0
    dq = torch.full((B, Nq, C), SENT, dtype=torch.float16, device=gpu)
    dkt, dvt = (torch.full((B, C, Nk), SENT, dtype=torch.float16, device=gpu) for _ in range(2))
    scale = D ** -0.5

    with pytest.raises(RuntimeError, match="Nq=60 must be a multiple of 8"):
        ops.attention_bwd_dkv(q[:, :60], qt[:, :, :64], k, v, do[:, :60], dot[:, :, :64], ld2, dkt, dvt, H, scale)
    with pytest.raises(RuntimeError, match="ldkt must cover Nk rounded up to 8"):
        ops.attention_bwd_dq(q, k, torch.zeros(B, C, 72, dtype=torch.float16, device=gpu), v, do, ld2, dq, H, scale)
    q64 = torch.zeros(B, Nq, 8 * 64, dtype=torch.float16, device=gpu)
    k64 = torch.zeros(B, 80, 8 * 64, dtype=torch.float16, device=gpu)
    with pytest.raises(RuntimeError, match="head dim 64 not in"):
        ops.attention_bwd_dq(q64, k64, k64.transpose(1, 2).contiguous(), k64, q64, ld2, torch.empty_like(q64), H, 0.125)
    with pytest.raises(RuntimeError, match="head dim 64 not in"):
        ops.attention_bwd_dkv(q64, q64.transpose(1, 2).contiguous(), k64, k64, q64, q64.transpose(1, 2).contiguous(), ld2,
                              k64.transpose(1, 2).contiguous(), k64.transpose(1, 2).contiguous(), H, 0.125)
    flat = torch.zeros(ld2.numel() + 4, dtype=torch.float32, device=gpu)
    odd = flat[2:2 + ld2.numel()].view_as(ld2)                                  # 8-byte aligned only
    with pytest.raises(RuntimeError, match="16-byte alignment"):
        ops.attention_bwd_dq(q, k, kt, v, do, odd, dq, H, scale)
    with pytest.raises(RuntimeError, match="16-byte alignment"):
        ops.attention_bwd_dkv(q, qt, k, v, do, dot, odd, dkt, dvt, H, scale)
    with pytest.raises(RuntimeError, match="transposed outputs"):
        ops.attention_bwd_dkv(q, qt, k, v, do, dot, ld2, torch.full((B, C, 72), SENT, dtype=torch.float16, device=gpu), dvt, H, scale)
    torch.cuda.synchronize()
    assert bool((dq == SENT).all()) and bool((dkt == SENT).all()) and bool((dvt == SENT).all()), "a rejected call wrote its output"
