"""tests/attention_fwd_model.py (the reference and the rounding yardstick of tests/test_attention_forward_edges_gpu.py) checked on the CPU:
`exact` against torch's softmax attention, `rounded` against the project's forward bars on every input family of the GPU module — a correct
kernel CAN meet them, shown before any GPU time is spent —, the row metric against three defects an aggregate bar can miss, and the
exact-selection inputs against their gap condition."""
import pytest
import torch

import attention_fwd_model as M

H = 8
ROW_FACTOR = 4.0        # tests/test_attention_forward_edges_gpu.py


def _torch_reference(q, k, v, heads, scale):
    B, Nq, C = q.shape
    hd = lambda t: t.double().reshape(t.shape[0], t.shape[1], heads, -1).transpose(1, 2)                      # noqa: E731
    return (torch.softmax(hd(q) @ hd(k).transpose(-1, -2) * scale, -1) @ hd(v)).transpose(1, 2).reshape(B, Nq, C)


@pytest.mark.parametrize("D,B,Nq,Nk", [(40, 2, 72, 77), (80, 1, 40, 129), (160, 3, 24, 33), (40, 1, 8, 1)])
def test_exact_is_a_float64_softmax_attention(D, B, Nq, Nk):
    q, k, v = M.make_inputs("normal", B, H, D, Nq, Nk, seed=3)
    scale = float(torch.tensor(D ** -0.5, dtype=torch.float32))
    ref = _torch_reference(q, k, v, H, scale)
    assert float((M.exact(q, k, v, H, D ** -0.5) - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    # K/V row map, per-row key counts and rows of different length
    ex = M.exact(q[:1].expand(3, -1, -1), [k[0], k[0, :5]], [v[0], v[0, :5]], H, D ** -0.5, kv_map=[0, 1, 1], nk=[max(Nk - 1, 1), None])
    n0 = max(Nk - 1, 1)
    assert float((ex[:1] - _torch_reference(q[:1], k[:1, :n0], v[:1, :n0], H, scale)).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    assert torch.equal(ex[1], ex[2])
    assert float((ex[1:2] - _torch_reference(q[:1], k[:1, :5], v[:1, :5], H, scale)).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_the_e4m3_quantiser():
    """The hand-written quantiser on every e4m3 value and on the midpoints between neighbours (ties to even), subnormals included; where
    this torch converts float8_e4m3fn on the CPU the two agree on a dense sweep."""
    vals = sorted({(1 + m / 8) * 2.0 ** e for m in range(8) for e in range(-6, 9) if (1 + m / 8) * 2.0 ** e <= 448} | {m * 2.0 ** -9 for m in range(8)})
    x = torch.tensor(vals, dtype=torch.float64)
    assert len(vals) == 127 and torch.equal(M._e4m3_by_hand(x), x) and torch.equal(M._e4m3_by_hand(-x), -x)
    mid = (x[1:] + x[:-1]) / 2
    even = torch.where((torch.arange(len(vals) - 1) % 2) == 0, x[:-1], x[1:])       # codes alternate even / odd mantissa from 0 on
    assert torch.equal(M._e4m3_by_hand(mid), even)
    assert torch.equal(M.e4m3(torch.tensor([1e4, -1e4, 460.0])), torch.tensor([448.0, -448.0, 448.0], dtype=torch.float64))
    if M.TORCH_E4M3:
        sweep = torch.linspace(-448, 448, 200001, dtype=torch.float32)
        assert torch.equal(sweep.to(torch.float8_e4m3fn).double(), M._e4m3_by_hand(sweep))


@pytest.mark.parametrize("family", M.FAMILIES)
@pytest.mark.parametrize("D,B,Nq,Nk", [(40, 1, 64, 448), (80, 2, 64, 320), (160, 2, 64, 640)])
def test_the_documented_roundings_alone_stay_inside_the_bars(family, D, B, Nq, Nk):
    """check()'s 1e-3 rel-L2 / 3e-3 max over the global max (2e-3 / 6e-3 for the D = 40 fast path under a common logit offset, the bar of
    the test that defines that input) with the kernels' documented roundings and nothing else; the fp8 path at 8e-2 aggregate."""
    q, k, v = M.make_inputs(family, B, H, D, Nq, Nk)
    ex = M.exact(q, k, v, H, D ** -0.5)
    paths = ("general", "f40", "f8") if D == 40 else ("general",)
    for path in paths:
        rd = M.rounded(q, k, v, H, D ** -0.5, path=path)
        l2, mx = M.rel_l2(rd, ex), float((rd - ex).abs().max() / ex.abs().max())
        row = M.max_row_error(rd, ex, H)
        print(f"{family} D{D} B{B} Nq{Nq} Nk{Nk} {path}: rel-L2 {l2:.1e} max {mx:.1e} worst row {row:.1e}")
        assert bool(torch.isfinite(rd).all())
        if path == "f8":
            assert l2 <= 8e-2
        elif path == "f40" and family.startswith("offset"):
            assert l2 <= 2e-3 and mx <= 6e-3
        else:
            assert l2 <= 1e-3 and mx <= 3e-3


def test_row_metric_sees_what_an_aggregate_can_miss():
    """On the largest case of the GPU module (D 160, B 3, Nq 256, Nk 768): one dropped key, one extra key (mask off by one) and one
    query row computed against the wrong K/V row each exceed ROW_FACTOR x the rounded model's own worst row error."""
    D, B, Nq, Nk = 160, 3, 256, 768
    q, k, v = M.make_inputs("normal", B, H, D, Nq, Nk + 1)
    ex = M.exact(q, k, v, H, D ** -0.5, nk=Nk)
    bar = ROW_FACTOR * M.max_row_error(M.rounded(q, k, v, H, D ** -0.5, nk=Nk), ex, H)
    dropped = M.exact(q, k, v, H, D ** -0.5, nk=Nk - 1)
    extra = M.exact(q, k, v, H, D ** -0.5, nk=Nk + 1)
    wrong = ex.clone()
    wrong[2, 100] = M.exact(q[2:3, 100:101], k[1:2], v[1:2], H, D ** -0.5, nk=Nk)[0, 0]
    for what, got in (("dropped key", dropped), ("extra key", extra), ("wrong K/V row", wrong)):
        row, agg = M.max_row_error(got, ex, H), M.rel_l2(got, ex)
        print(f"{what}: worst row {row:.1e} (bar {bar:.1e}), aggregate {agg:.1e}")
        assert row > bar, what


SELECT_CASES = [(40, 2, 3, 96, [130, 77], [0, 1]), (80, 3, 8, 72, [193, 65], [0, 1, 1]), (160, 2, 3, 96, [577], [0, 0]), (40, 1, 8, 40, [1], [0])]


@pytest.mark.parametrize("D,B,heads,Nq,nks,kv_map", SELECT_CASES)
def test_selector_inputs_meet_their_gap_and_the_model_selects_bit_for_bit(D, B, heads, Nq, nks, kv_map):
    q, ks, vs, t = M.selector_inputs(B, heads, D, Nq, nks, kv_map)
    c = float(torch.tensor(D ** -0.5, dtype=torch.float32)) * M.LOG2E
    for b in range(B):
        kk, n = ks[kv_map[b]], nks[kv_map[b]]
        if n >= 64:
            assert set(range(64)) <= {int(x) % 64 for x in t[b]}, "every in-tile position"
        assert {0, n - 1} <= {int(x) for x in t[b]}
        for tile in range(1, (n + 63) // 64):
            assert {64 * tile - 1, 64 * tile} <= {int(x) for x in t[b]}, "both sides of every tile boundary"
        s2 = (M._h(q[b], heads) @ M._h(kk, heads).transpose(-1, -2)) * c                    # [H, Nq, n]
        sel = s2.gather(-1, t[b].view(1, Nq, 1).expand(heads, Nq, 1))
        others = s2.scatter(-1, t[b].view(1, Nq, 1).expand(heads, Nq, 1), float("-inf"))
        if n > 1:
            assert float((sel - others.max(-1, keepdim=True).values).min()) >= M.SELECT_GAP
        # distinct V rows: a wrong key, head or K/V row cannot give the right answer
        for j, vv in enumerate(vs):
            rows = vv.view(nks[j] * heads, D)
            assert len({tuple(r.tolist()) for r in rows}) == rows.shape[0]
    for vv in vs:
        assert torch.equal(M.e4m3(vv), vv.double()), "V is exact in e4m3"
    assert torch.equal(M.e4m3(q), q.double()) and all(torch.equal(M.e4m3(kk), kk.double()) for kk in ks)
    want = M.selected_values(vs, t, kv_map)
    for path in M.PATHS if D == 40 else ("general",):
        got = M.rounded(q, ks, vs, heads, D ** -0.5, kv_map=kv_map, path=path)
        assert torch.equal(got, want.double()), path
