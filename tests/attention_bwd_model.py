"""CPU model of the attention training pipeline (sg_attn_fwd_lse_f16 -> sg_attn_bwd_prep_f32 -> sg_attn_bwd_dq_f16 / sg_attn_bwd_dkv_f16),
written from oracle/storygen_backward.py::attention_core_bwd and the comment block at the top of csrc/attention_bwd.hip.  Plain torch.

  exact(q, k, v, do, heads)    float64 from the fp16-valued inputs: the REFERENCE of tests/test_attention_backward_edges_gpu.py.
  rounded(q, k, v, do, heads)  the same formulas with the kernels' DOCUMENTED roundings and nothing else: O stored fp16; lse2 and delta
                               fp32; delta from the fp16 O; P and dS cast to fp16 before the second contraction; outputs fp16.  Everything
                               else float64.  It is the yardstick of the per-row bar: what a correct kernel cannot avoid losing.

Both return a dict: o, dq [B, Nq, C]; dk, dv [B, Nk, C]; lse2 (log2 domain), delta [B, H, Nq] — float64 tensors.
Also here: the input families of the edge tests (so that the CPU test shows the bars reachable on exactly the inputs the GPU test uses) and
the row metric."""
import torch

LOG2E = 1.4426950408889634


def heads_of(t, heads):
    """[B, N, H*D] -> [B, H, N, D] float64."""
    b, n, c = t.shape
    return t.double().reshape(b, n, heads, c // heads).transpose(1, 2)


def _back(t):
    b, h, n, d = t.shape
    return t.transpose(1, 2).reshape(b, n, h * d)


def _f16(t):
    return t.to(torch.float16).double()


def _f32(t):
    return t.to(torch.float32).double()


def _model(q, k, v, do, heads, rnd):
    d = q.shape[-1] // heads
    scale = d ** -0.5
    qh, kh, vh, doh = (heads_of(t, heads) for t in (q, k, v, do))
    s2 = (qh @ kh.transpose(-1, -2)) * (scale * LOG2E)                     # log2-domain scores
    m = s2.max(-1, keepdim=True).values
    lse2 = (m + torch.log2(torch.exp2(s2 - m).sum(-1, keepdim=True)))
    o = torch.exp2(s2 - lse2) @ vh
    if rnd:
        o, lse2 = _f16(o), _f32(lse2)
    p = torch.exp2(s2 - lse2)                                              # recomputed from the STORED lse2, as the kernel does
    delta = (doh * o).sum(-1, keepdim=True)
    if rnd:
        delta = _f32(delta)
    ds = p * (doh @ vh.transpose(-1, -2) - delta)
    if rnd:
        p, ds = _f16(p), _f16(ds)
    dv = p.transpose(-1, -2) @ doh
    dq = (ds @ kh) * scale
    dk = (ds.transpose(-1, -2) @ qh) * scale
    out = dict(o=_back(o), dq=_back(dq), dk=_back(dk), dv=_back(dv), lse2=lse2[..., 0], delta=delta[..., 0])
    if rnd:
        for n in ("dq", "dk", "dv"):
            out[n] = _f16(out[n])
    return out


def exact(q, k, v, do, heads):
    return _model(q, k, v, do, heads, False)


def rounded(q, k, v, do, heads):
    return _model(q, k, v, do, heads, True)


def row_errors(got, ref, heads):
    """e_row = ||got_row - ref_row|| / RMS over the rows of ||ref_row||, per (batch, head); [B, H, N].  A (batch, head) whose reference
    rows are all zero (Nk = 1: dQ = dK = 0 identically) yields inf for a non-zero row and 0 otherwise."""
    g, r = heads_of(got, heads), heads_of(ref, heads)
    err = (g - r).norm(dim=-1)
    rms = r.norm(dim=-1).pow(2).mean(-1, keepdim=True).sqrt()
    return torch.where(err == 0, torch.zeros_like(err), err / rms)


def max_row_error(got, ref, heads):
    return float(row_errors(got, ref, heads).max())


# ------------------------------------------------------------------------------------------------ input families
FAMILIES = ("normal", "late_key", "offset_neg", "offset_pos", "do_2p10", "do_2m12")


def _r(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.float16)


def make_inputs(family, B, heads, D, Nq, Nk, seed=0):
    """fp16 CPU tensors q [B, Nq, C], k, v [B, Nk, C], do [B, Nq, C].
      normal      N(0, 1)
      late_key    the LAST key of every batch row is 24 x one query row (tests/test_attention_d40_loop_gpu.py::
                  test_late_dominating_key_forces_the_rescale, pushed to the end of the key axis): in that query row its log2-domain logit
                  exceeds every other by more than 2^6 in every head (asserted), so the online softmax rescales at the very last key
      offset_*    the construction of test_extreme_maxima_and_the_clamp: q[..., 0] = 8 and k[..., 0] = shift in every head, the second
                  half of batch row 0's keys at 1.5 x / 0.5 x the shift — a large common logit offset with a step in the middle
      do_2p10     N(0, 1) with dO scaled by 2^10 (the trainer's loss scale)
      do_2m12     ... by 2^-12: dS lands in the fp16 subnormal range (what running without a loss scale costs)"""
    C = heads * D
    q, k, v, do = _r((B, Nq, C), 4 * seed + 1), _r((B, Nk, C), 4 * seed + 2), _r((B, Nk, C), 4 * seed + 3), _r((B, Nq, C), 4 * seed + 4)
    if family == "late_key":
        row = Nq // 3
        k[:, Nk - 1] = (q[:, row].float() * 24.0).to(torch.float16)
        if Nk > 1:
            s2 = (heads_of(q[:, row:row + 1], heads) @ heads_of(k, heads).transpose(-1, -2))[:, :, 0] * (D ** -0.5 * LOG2E)
            assert float((s2[..., -1:] - s2[..., :-1]).min()) > 64.0, "late_key: the last key must dominate by more than 2^6"
    elif family in ("offset_neg", "offset_pos"):
        shift = -40.0 if family == "offset_neg" else 25.0
        qh, kh = q.view(B, Nq, heads, D), k.view(B, Nk, heads, D)
        qh[..., 0] = 8.0
        kh[..., 0] = shift
        kh[0, Nk // 2:, :, 0] = shift * 1.5 if shift > 0 else shift * 0.5
    elif family == "do_2p10":
        do = (do.float() * 1024.0).to(torch.float16)
    elif family == "do_2m12":
        do = (do.float() * 2.0 ** -12).to(torch.float16)
    elif family != "normal":
        raise ValueError(family)
    return q, k, v, do


# the (D, B, Nq, Nk) each range family runs at, on the GPU and in the CPU test: one shape per head dim, both axes with a partial last tile
RANGE_SHAPES = [(40, 2, 200, 264), (80, 1, 136, 200), (160, 2, 72, 136)]


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))

