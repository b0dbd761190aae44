"""CPU model of the forward attention kernels (sg_attn_fwd_f16, sg_attn_fwd_pair_f16, sg_attn_f8_pack + sg_attn_fwd_f8_d40), written from the
comment blocks at the top of csrc/attention.hip, csrc/attention_kernel.h and csrc/attention_f8.hip.  Plain torch.

  exact(q, k, v, heads, scale, kv_map, nk)          float64 from the fp16-valued inputs: the REFERENCE of
                                                    tests/test_attention_forward_edges_gpu.py.
  rounded(q, k, v, heads, scale, kv_map, nk, path)  the same formula with the kernels' DOCUMENTED roundings and nothing else; everything
                                                    else float64.  It is the yardstick of the per-row bar: what a correct kernel cannot
                                                    avoid losing.
      path "general"  P cast to fp16 before P V (the row sum from the unrounded P), O stored fp16: attn_fwd_kernel at D = 80 / 160, the
                      key-split kernel, the training forward, D = 40 under option attn_d40_general;
      path "f40"      also q * scale * log2(e) rounded to fp16 (fp32 product), and the row sum taken of the fp16 P (the row of ones of
                      the padded head dimension sums exactly the values that multiply V): the D = 40 fast path in all its bodies;
      path "f8"       Q / K / V to e4m3 clamped at +-448, P to e4m3(128 P), the row sum from the unquantised 128 P, O stored fp16.
  Not modelled: the order of the fp32 sums, v_exp_f32, the deferred rescale (P relative to a stale maximum), the fp16 hi + lo maximum of
  the D = 40 fast path.

Operands: q [B, Nq, H*D]; k, v either [Bk, Nk', H*D] tensors or lists of [Nk_j, H*D] tensors, one per K/V row (rows of different length:
sg_attn_desc.k2); kv_map[b] = the K/V row of query batch b (default: b); nk = valid keys, an int or one per K/V row (default: all).
Returns [B, Nq, H*D] float64.  `scale` is taken as the float32 the C ABI carries.
Also here: the input families of the GPU module, so that the CPU test shows the bars reachable on exactly those inputs; the row metric is
tests/attention_bwd_model.py's."""
import math

import torch

from attention_bwd_model import heads_of, max_row_error, rel_l2, row_errors  # noqa: F401  (re-exported)

LOG2E = 1.4426950408889634
PATHS = ("general", "f40", "f8")


def _f16(t):
    return t.to(torch.float16).double()


def _e4m3_by_hand(t):
    """Round to nearest even onto OCP e4m3 (3 mantissa bits, exponents 2^-6 .. 2^8, subnormals down to 2^-9); |t| <= 448 expected."""
    a = t.double().abs()
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -20))).clamp(-6, 8)
    step = torch.exp2(e - 3)
    return torch.sign(t.double()) * torch.round(a / step) * step          # torch.round: half to even


def _torch_converts_e4m3():
    try:
        x = torch.tensor([0.3, -447.0, 2.0 ** -9, 17.0, 0.0], dtype=torch.float32)
        return bool(torch.equal(x.to(torch.float8_e4m3fn).to(torch.float64), _e4m3_by_hand(x)))
    except (AttributeError, RuntimeError, TypeError):
        return False


TORCH_E4M3 = _torch_converts_e4m3()


def e4m3(t):
    """float64 values of e4m3(clamp(t, +-448)), as v_cvt_pk_fp8_f32 of the clamped fp32 value gives them."""
    t = t.to(torch.float32).clamp(-448.0, 448.0)
    return t.to(torch.float8_e4m3fn).to(torch.float64) if TORCH_E4M3 else _e4m3_by_hand(t)


def _rows(k, v, nk):
    """-> lists of [nk_j, C] tensors, one per K/V row."""
    ks = list(k) if isinstance(k, (list, tuple)) else [k[j] for j in range(k.shape[0])]
    vs = list(v) if isinstance(v, (list, tuple)) else [v[j] for j in range(v.shape[0])]
    nks = [nk] * len(ks) if nk is None or isinstance(nk, int) else list(nk)
    nks = [kk.shape[0] if n is None else n for kk, n in zip(ks, nks)]
    return [kk[:n] for kk, n in zip(ks, nks)], [vv[:n] for vv, n in zip(vs, nks)]


def _h(t, heads):
    """[N, H*D] -> [H, N, D] float64"""
    return t.double().reshape(t.shape[0], heads, -1).transpose(0, 1)


def _model(q, k, v, heads, scale, kv_map, nk, path):
    B, Nq, C = q.shape
    ks, vs = _rows(k, v, nk)
    kv_map = list(range(B)) if kv_map is None else list(kv_map)
    s32 = torch.tensor(scale, dtype=torch.float32)
    c32 = s32 * torch.tensor(1.44269504088896340736, dtype=torch.float32)        # scale_log2 as attn_params computes it
    c = float(c32)
    out = torch.empty(B, Nq, C, dtype=torch.float64)
    for b in range(B):
        qh, kh, vh = _h(q[b], heads), _h(ks[kv_map[b]], heads), _h(vs[kv_map[b]], heads)
        if path == "f8":
            qh, kh, vh = e4m3(qh), e4m3(kh), e4m3(vh)
        if path == "f40":
            qh = (qh.to(torch.float32) * c32).to(torch.float16).double()
            s2 = qh @ kh.transpose(-1, -2)
        elif path is None:
            s2 = (qh @ kh.transpose(-1, -2)) * (float(s32) * LOG2E)
        else:
            s2 = (qh @ kh.transpose(-1, -2)) * c
        p = torch.exp2(s2 - s2.max(-1, keepdim=True).values)
        if path is None:
            o = (p @ vh) / p.sum(-1, keepdim=True)
        elif path == "general":
            o = _f16((_f16(p) @ vh) / p.sum(-1, keepdim=True))
        elif path == "f40":
            p = _f16(p)
            o = _f16((p @ vh) / p.sum(-1, keepdim=True))
        elif path == "f8":
            o = _f16((e4m3(128.0 * p) @ vh) / (128.0 * p).sum(-1, keepdim=True))
        else:
            raise ValueError(path)
        out[b] = o.transpose(0, 1).reshape(Nq, C)
    return out


def exact(q, k, v, heads, scale, kv_map=None, nk=None):
    return _model(q, k, v, heads, scale, kv_map, nk, None)


def rounded(q, k, v, heads, scale, kv_map=None, nk=None, path="general"):
    if path not in PATHS:
        raise ValueError(path)
    return _model(q, k, v, heads, scale, kv_map, nk, path)


def path_of(family, D):
    """The rounded model of a plan family (ops.ATTN_FAMILIES) at head dim D."""
    if family == "f8":
        return "f8"
    return "f40" if D == 40 and family in ("d40_loop", "shared_body", "lean") else "general"


# ------------------------------------------------------------------------------------------------ input families
FAMILIES = ("normal", "late_key", "wave_keys", "creep", "offset_neg", "offset_pos")


def _r(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.float16)


def make_inputs(family, B, heads, D, Nq, Nk, seed=0, Bk=None):
    """fp16 CPU tensors q [B, Nq, C], k, v [Bk, Nk, C] (Bk = B unless given).
      normal      q, k ~ 1.5 N(0, 1), v ~ N(0, 1) (tests/test_kernels_gpu.py::test_attention)
      late_key    N(0, 1); key 64 t + 5 of K/V row 0 is a multiple of query row 3 t + 1, for every tile t >= 1 in turn, and the very LAST key of
                  the last K/V row a multiple of the last query row: a dominating key in every late tile (the online softmax rescales there)
      wave_keys   test_attention_key_split_d160_rescale_and_variants: k ~ 0.3 N(0, 1), so that a row's keys are tiny everywhere but in the
                  tile of its dominating key — one such key per tile t (query row 7 t + 2, key 64 t + (5 t) % 64), i.e. in each wave's tile of
                  every round of a key-split group, wave 0's first tile included, and the last key for the last query row
      creep       test_attention_deferred_rescale_threshold: k ~ 0.2 N(0, 1), key 64 t + 3 = 0.28 t x query row 7 (t >= 1) — the row's maximum
                  grows by under 6 log2 units per tile (the kernels keep a stale maximum and P exceeds 1), then the last key jumps far above
      offset_*    test_attention_d40_fast_path_extreme_maxima: q[..., 0] = 8, k[..., 0] = shift (-40 / +25) in every head, the keys of K/V
                  row 0 from the first tile boundary past Nk / 2 on at 0.5 x / 1.5 x the shift: a large common logit offset whose maximum moves
                  at a tile boundary"""
    C = heads * D
    Bk = B if Bk is None else Bk
    ntiles = (Nk + 63) // 64
    if family == "normal":
        return _r((B, Nq, C), 3 * seed + 1, 1.5), _r((Bk, Nk, C), 3 * seed + 2, 1.5), _r((Bk, Nk, C), 3 * seed + 3)
    kscale = {"wave_keys": 0.3, "creep": 0.2}.get(family, 1.0)
    q, k, v = _r((B, Nq, C), 3 * seed + 1), _r((Bk, Nk, C), 3 * seed + 2, kscale), _r((Bk, Nk, C), 3 * seed + 3)
    qf = q.float()
    if family == "late_key":
        for t in range(1, ntiles):
            k[0, min(64 * t + 5, Nk - 1)] = (qf[0, (3 * t + 1) % Nq] * 6.0).to(torch.float16)
        k[Bk - 1, Nk - 1] = (qf[B - 1, Nq - 1] * 7.0).to(torch.float16)
    elif family == "wave_keys":
        for t in range(ntiles):
            k[0, min(64 * t + (5 * t) % 64, Nk - 1)] = (qf[0, (7 * t + 2) % Nq] * 2.0).to(torch.float16)
        k[Bk - 1, Nk - 1] = (qf[B - 1, Nq - 1] * 3.0).to(torch.float16)
    elif family == "creep":
        for t in range(1, ntiles):
            k[0, min(64 * t + 3, Nk - 2)] = (qf[0, 7 % Nq] * (0.28 * t)).to(torch.float16)
        k[0, Nk - 1] = (qf[0, 7 % Nq] * 6.0).to(torch.float16)
    elif family in ("offset_neg", "offset_pos"):
        shift = -40.0 if family == "offset_neg" else 25.0
        qh, kh = q.view(B, Nq, heads, D), k.view(Bk, Nk, heads, D)
        qh[..., 0] = 8.0
        kh[..., 0] = shift
        kh[0, ((Nk // 2 + 63) // 64) * 64:, :, 0] = shift * 1.5 if shift > 0 else shift * 0.5
    else:
        raise ValueError(family)
    return q, k, v


# ------------------------------------------------------------------------------------------------ exact selection
SELECT_GAIN = 16.0          # q = 16 x the target key's code: exact in fp16 and in e4m3
SELECT_GAP = 29.0           # log2 units between the selected score and every other


def min_distance(D):
    """Hamming distance between key codes that gives SELECT_GAP: scores differ by 2 * SELECT_GAIN * distance * D^-0.5 * log2(e)."""
    return max(4, math.ceil(SELECT_GAP / (2.0 * SELECT_GAIN * D ** -0.5 * LOG2E)))


def _codes(n, D, seed):
    """n codes of +-1 with pairwise Hamming distance >= min_distance(D), built greedily from a seeded stream of candidates."""
    g = torch.Generator().manual_seed(seed)
    dmin = min_distance(D)
    kept = torch.empty(n, D)
    have = 0
    while have < n:
        cand = torch.randint(0, 2, (4 * n, D), generator=g).float() * 2 - 1
        for c in cand:
            if have == 0 or float(((D - kept[:have] @ c) / 2).min()) >= dmin:      # Hamming distance = (D - dot) / 2
                kept[have] = c
                have += 1
                if have == n:
                    break
    return kept


def _value_table():
    """The 64 values +-(1 + m / 8) 2^e, m < 8, e in {-1, 0, 1, 2}: exact in e4m3 and in fp16, all within a factor 15 of one another."""
    vals = [s * (1 + m / 8) * 2.0 ** e for s in (1, -1) for m in range(8) for e in (-1, 0, 1, 2)]
    return torch.tensor(vals, dtype=torch.float32)


def targets(Nq, n, offset=0):
    """The target key of each query row of one batch, for a K/V row of n keys: all 64 in-tile positions (tile 0, and the last full tile),
    the first and the last valid key, both sides of every tile boundary, the first key of the ragged tail — cycled over the queries,
    starting `offset` entries in."""
    want = list(range(min(64, n)))
    for t in range(1, (n + 63) // 64):
        want += [64 * t - 1, 64 * t]
    want += [0, n - 1, (n - 1) // 64 * 64, max(n - 2, 0)]
    last_full = n // 64 - 1
    if last_full > 0:
        want += list(range(64 * last_full, 64 * last_full + 64))
    return [want[(i + offset) % len(want)] for i in range(Nq)]


def selector_inputs(B, heads, D, Nq, nks, kv_map=None, seed=0):
    """Inputs whose softmax is a one-hot row up to rounding: q [B, Nq, C], ks, vs (lists of [nk_j, C], one per K/V row), t [B, Nq] (the
    selected key of every query row, the same in every head), all fp16-exact float16 tensors.
      K rows   per (K/V row, head) a set of +-1 codes with pairwise Hamming distance >= min_distance(D) (one greedy set, the head dimension
               permuted and sign-flipped per K/V row and head: distances are kept)
      q        SELECT_GAIN x the code of the target key, per head
      V        v[j][key, h * D + d] = table[a seeded draw per (K/V row j, key, h, d)], table = _value_table(): few-bit values exact in e4m3;
               the D values of a (K/V row, key, head) identify it (the CPU test checks that no two are equal)
    The selected score then exceeds every other by >= SELECT_GAP log2 units (checked by the CPU test on the scores themselves)."""
    C = heads * D
    kv_map = list(range(B)) if kv_map is None else list(kv_map)
    base = _codes(max(nks), D, 1000 + seed)
    g = torch.Generator().manual_seed(77 + seed)
    table = _value_table()
    ks, vs = [], []
    for j, n in enumerate(nks):
        kk = torch.empty(n, heads, D)
        for h in range(heads):
            perm = torch.randperm(D, generator=g)
            sign = torch.randint(0, 2, (D,), generator=g).float() * 2 - 1
            kk[:, h] = base[:n][:, perm] * sign
        idx = torch.randint(0, table.numel(), (n, heads, D), generator=torch.Generator().manual_seed(5000 + 97 * seed + j))
        ks.append(kk.reshape(n, C).to(torch.float16))
        vs.append(table[idx].reshape(n, C).to(torch.float16))
    t = torch.tensor([targets(Nq, nks[kv_map[b]], 37 * b) for b in range(B)])
    q = torch.stack([ks[kv_map[b]][t[b]].float() * SELECT_GAIN for b in range(B)]).to(torch.float16)
    return q, ks, vs, t


def selected_values(vs, t, kv_map=None):
    """[B, Nq, C] float16: the V row of every query's target key."""
    kv_map = list(range(t.shape[0])) if kv_map is None else list(kv_map)
    return torch.stack([vs[kv_map[b]][t[b]] for b in range(t.shape[0])])
