"""D = 40 attention: the tile loop cut into tile 0 / branch-free steady state / drain (attn_d40_body) against
  (a) the fp32 softmax(Q K^T scale) V reference with the bar of test_kernels_gpu.py::test_attention, and
  (b) the shared tile loop it replaces (development option attn_d40_loop = 1), BIT FOR BIT: the split changes no arithmetic.
Shapes: what the split can break — tile 0 that is also the ragged tail, exact multiples of the tile, Nk = 1 and 63 mod 64, Nk not a multiple
of 8 (V^T padding), every tile count mod 3 (the 3-stage unroll) and mod 2 (the 2-stage one) below and above the point where the steady-state
loop starts (6 / 4 full tiles), ragged and tiny query counts, both instantiations (4 waves x 3 stages on big grids, 2 x 2 otherwise)."""
import pytest
import torch

from test_kernels_gpu import _vt, check, rnd

pytestmark = pytest.mark.gpu

H, D = 8, 40
C = H * D
SCALE = D ** -0.5


def _ref(q, k, v):
    """fp32 reference, one query batch at a time (the contract shapes hold 1.6 G scores per batch)."""
    def heads(t):
        return t.float().view(t.shape[0], t.shape[1], H, D).transpose(1, 2)
    out = []
    for b in range(q.shape[0]):
        att = torch.softmax(heads(q[b:b + 1]) @ heads(k[b:b + 1]).transpose(-1, -2) * SCALE, dim=-1) @ heads(v[b:b + 1])
        out.append(att.transpose(1, 2).reshape(1, q.shape[1], C))
    return torch.cat(out)


def _new_and_old(launch):
    """launch() -> output tensor; runs it on the default body and on the previous one."""
    from storygen_amd import ops
    new = launch()
    ops.debug_set_option("attn_d40_loop", 1)
    try:
        old = launch()
    finally:
        ops.debug_set_option("attn_d40_loop", 0)
    torch.cuda.synchronize()
    return new, old


NKS = [1, 37, 63, 64, 65, 127, 128, 129, 191, 192, 256, 257, 320, 383, 384, 385, 448, 449, 511, 512, 576, 577, 639, 1000, 1217]
# B, Nq: 4 waves x 3 stages (ceil(Nq / 128) * H * B >= 512) with and without a ragged last query block | 2 waves x 2 stages, Nq % 128 != 0, Nq < 32
CASES = ([(B, Nq, Nk) for B, Nq in [(2, 4096), (1, 200), (1, 20)] for Nk in NKS] +
         [(2, 4000, Nk) for Nk in (37, 128, 385, 577, 1000)])


@pytest.mark.parametrize("B,Nq,Nk", CASES)
def test_tile_counts_and_ragged_tails(gpu, B, Nq, Nk):
    from storygen_amd import ops
    q, k, v = rnd((B, Nq, C), gpu, 1.5, seed=1), rnd((B, Nk, C), gpu, 1.5, seed=2), rnd((B, Nk, C), gpu, seed=3)
    vt = _vt(v)

    def launch():
        out = torch.full((B, Nq, C), float("nan"), dtype=torch.float16, device=gpu)
        ops.attention(q, k, vt, out, H, SCALE, nk=Nk)
        return out
    new, old = _new_and_old(launch)
    assert torch.equal(new, old), "attn_d40_body differs from the shared tile loop"
    check(new, _ref(q, k, v), f"attention D=40 B{B} Nq{Nq} Nk{Nk}")


@pytest.mark.parametrize("Nq,Nk", [(4096, 640), (4096, 449), (200, 705)])
def test_shared_kv_batches(gpu, Nq, Nk):
    """kv_batches < B: query batches [0, 1, 2] read K/V rows [0, 1, 1]."""
    from storygen_amd import ops
    q, k, v = rnd((3, Nq, C), gpu, 1.5, seed=1), rnd((2, Nk, C), gpu, 1.5, seed=2), rnd((2, Nk, C), gpu, seed=3)
    vt = _vt(v)

    def launch():
        out = torch.full((3, Nq, C), float("nan"), dtype=torch.float16, device=gpu)
        ops.attention(q, k, vt, out, H, SCALE, nk=Nk)
        return out
    new, old = _new_and_old(launch)
    assert torch.equal(new, old)
    idx = [0, 1, 1]
    check(new, _ref(q, k[idx], v[idx]), "shared K/V rows")


def _short_rows(gpu, Nq, hw, R):
    """The main pass's layout: K/V rows [zero image (hw keys) | frames (R hw keys)] back to back in one flat projection output."""
    T = hw + R * hw
    q = rnd((3, Nq, C), gpu, 1.5, seed=1)
    kflat, vflat = rnd((T, C), gpu, 1.5, seed=2), rnd((T, C), gpu, 1.0, seed=3)
    vt = vflat.t().contiguous()
    k_s, k_l = kflat[:hw].view(1, hw, C), kflat[hw:].view(1, R * hw, C)
    vt_s = vt[:, :hw].unflatten(1, (1, hw)).permute(1, 0, 2)
    vt_l = vt[:, hw:].unflatten(1, (1, R * hw)).permute(1, 0, 2)
    return q, (k_s, vt_s, vflat[:hw].view(1, hw, C)), (k_l, vt_l, vflat[hw:].view(1, R * hw, C))


@pytest.mark.parametrize("Nq,hw,R", [(4096, 4096, 3), (4096, 200, 3), (320, 64, 5)])
def test_short_kv_rows(gpu, Nq, hw, R):
    """sg_attn_desc.k2: one short K/V row (hw keys) beside the long ones (R hw keys) — (4096, 4096, 3) is the contract step's main-pass
    launch, B3 H8 Nq4096 Nk12288 with one 4 096-key row."""
    from storygen_amd import ops
    q, (k_s, vt_s, v_s), (k_l, vt_l, v_l) = _short_rows(gpu, Nq, hw, R)

    def launch():
        out = torch.full((3, Nq, C), float("nan"), dtype=torch.float16, device=gpu)
        ops.attention(q, k_l, vt_l, out, H, SCALE, short=(k_s, vt_s))
        return out
    new, old = _new_and_old(launch)
    assert torch.equal(new, old)
    check(new[:1], _ref(q[:1], k_s, v_s), "short row")
    check(new[1:], _ref(q[1:], k_l.expand(2, -1, -1), v_l.expand(2, -1, -1)), "long rows")


def test_reference_pass_shape(gpu):
    """The contract step's batched reference pass: B20 H8 Nq4096 Nk4096."""
    from storygen_amd import ops
    B, N = 20, 4096
    q, k, v = rnd((B, N, C), gpu, 1.5, seed=1), rnd((B, N, C), gpu, 1.5, seed=2), rnd((B, N, C), gpu, seed=3)
    vt = _vt(v)

    def launch():
        out = torch.full((B, N, C), float("nan"), dtype=torch.float16, device=gpu)
        ops.attention(q, k, vt, out, H, SCALE)
        return out
    new, old = _new_and_old(launch)
    assert torch.equal(new, old)
    check(new, _ref(q, k, v), "reference-pass attention")


@pytest.mark.parametrize("Nq,Nk_img,Bk", [(4096, 1024, 2), (4096, 449, 3), (1024, 3072, 3), (200, 130, 2)])
def test_paired_text_and_image_launch(gpu, Nq, Nk_img, Bk):
    """sg_attn_fwd_pair_f16 on attn_d40_body against the two launches of the shared tile loop."""
    from storygen_amd import ops
    B, S = 3, 77
    q2, q3 = rnd((B, Nq, C), gpu, 1.5, seed=1), rnd((B, Nq, C), gpu, 1.5, seed=2)
    kt, vt_ = rnd((B, 80, C), gpu, 1.5, seed=3), rnd((B, 80, C), gpu, 1.0, seed=4)
    ki, vi = rnd((Bk, Nk_img, C), gpu, 1.5, seed=5), rnd((Bk, Nk_img, C), gpu, 1.0, seed=6)
    vtt, vti = _vt(vt_), _vt(vi)

    def launch():
        both = torch.full((B, Nq, 2 * C), float("nan"), dtype=torch.float16, device=gpu)
        ops.attention_pair((q3, ki, vti, both[:, :, C:], None), (q2, kt, vtt, both[:, :, :C], S), H, SCALE)
        return both
    new, old = _new_and_old(launch)
    assert torch.equal(new, old)
    idx = [b if b < Bk else b - (B - Bk) for b in range(B)]
    check(new[:, :, C:], _ref(q3, ki[idx], vi[idx]), "paired image attention")
    check(new[:, :, :C], _ref(q2, kt[:, :S], vt_[:, :S]), "paired text attention")


@pytest.mark.parametrize("B,Nq", [(2, 4096), (1, 128)])
def test_late_dominating_key_forces_the_rescale(gpu, B, Nq):
    """One key of a late tile dominates a row — in the steady-state loop (tile 4 of 11; tile 7 too on the 2-stage ring) and in the drain (the last tile)."""
    from storygen_amd import ops
    Nk = 700
    q, k, v = rnd((B, Nq, C), gpu, seed=1), rnd((B, Nk, C), gpu, seed=2), rnd((B, Nk, C), gpu, seed=3)
    k[0, 300] = q[0, 5] * 6.0
    k[0, 450] = q[0, 77] * 8.0
    k[B - 1, 699] = q[B - 1, 100] * 7.0
    vt = _vt(v)

    def launch():
        out = torch.full((B, Nq, C), float("nan"), dtype=torch.float16, device=gpu)
        ops.attention(q, k, vt, out, H, SCALE)
        return out
    new, old = _new_and_old(launch)
    assert torch.equal(new, old)
    check(new, _ref(q, k, v), "late dominating key")


@pytest.mark.parametrize("shift", [-40.0, 25.0])
@pytest.mark.parametrize("B,Nq", [(2, 4096), (1, 256)])
def test_extreme_maxima_and_the_clamp(gpu, B, Nq, shift):
    """The inputs of test_attention_d40_fast_path_extreme_maxima (row maxima far from the placeholder 0, the +-60 000 clamp of the fp16
    hi / lo split, a large delta between tiles) at 7 and at 11 tiles: bit-identical to the shared loop; against fp32 with THAT test's bar
    (2e-3 / 6e-3: the case is defined there, with the precision its two-fp16 maximum has at |m| ~ 1e3)."""
    from storygen_amd import ops
    for Nk in (448, 700):
        q, k, v = rnd((B, Nq, C), gpu, 1.0, seed=7), rnd((B, Nk, C), gpu, 1.0, seed=8), rnd((B, Nk, C), gpu, seed=9)
        qh, kh = q.view(B, Nq, H, D), k.view(B, Nk, H, D)
        qh[..., 0] = 8.0
        kh[..., 0] = shift
        kh[0, 200:, :, 0] = shift * 1.5 if shift > 0 else shift * 0.5
        vt = _vt(v)

        def launch():
            out = torch.full((B, Nq, C), float("nan"), dtype=torch.float16, device=gpu)
            ops.attention(q, k, vt, out, H, SCALE)
            return out
        new, old = _new_and_old(launch)
        assert torch.equal(new, old)
        check(new, _ref(q, k, v), f"extreme maxima Nk{Nk}", l2=2e-3, mx=6e-3)
