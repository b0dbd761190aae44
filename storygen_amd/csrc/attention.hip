// Fused (flash-style) attention forward for gfx950: O = softmax(scale * Q K^T) V, fp16 in/out, fp32 softmax.
//
// Serves the three attentions of StoryGen's BasicTransformerBlock (model/attention.py:255-260 self, :271-276 text,
// :285-290 image / Visual-Language Context) — head dim D = C/8 in {40, 80, 160}, Nk = HW, 77 or R*HW.
//
// Operands: Q and K token-major ([B, N, H*D], heads interleaved in the channel dimension exactly as
// head_to_batch_dim expects) and V *transposed*: VT[b][h*D + d][key].  The V projection is a GEMM anyway, so the host
// simply computes it with swapped operands (VT = Wv . X^T) — the attention kernel then needs no in-kernel transpose
// and every LDS tile it consumes is a plain 16-byte-chunk copy of global memory, which is what LDS-DMA wants.
//
// Work decomposition: one workgroup = NW wave64, each wave owns 32 queries of one (batch, head); K / VT are streamed in
// tiles of 64 keys through an S-stage LDS ring filled by LDS-DMA (global_load_lds, 16 B per lane, no VGPR staging),
// counted vmcnt waits and ONE raw s_barrier per tile (same pipeline as the GEMM mainloop).
//
// MFMA formulation (v_mfma_f32_32x32x16_f16), chosen so that softmax never leaves registers:
//   S^T[key, q] = sum_d K[key, d] Q[q, d]      A = K fragment (LDS, ds_read_b128), B = Q^T fragment (registers)
//     The A rows are fed in a permuted order (row i of the MFMA reads key pi(i), pi = swap of bits 2 and 3), so that
//     accumulator register r of lane (q = l & 31, hi = l >> 5) holds key 16 (r >> 3) + 8 hi + (r & 7): the 8 registers
//     of a 16-key step are 8 CONSECUTIVE keys.  Row max / row sum are in-lane reductions plus ONE exchange with l^32.
//   O^T[d, q] = sum_key VT[d, key] P^T[key, q]  A = VT fragment (LDS, one ds_read_b128 of 8 consecutive keys),
//     B = P^T = the lane's own accumulator registers converted to fp16.  P never moves across lanes or through LDS.
//   Head dim 40 is zero-padded to 48 on the contraction side (the Q fragment of chunk 5 is zero; the K fragment reads
//   the first 16 bytes of the next LDS row, finite data) and to 64 on the O^T rows (rows >= D are never stored).
// LDS images (both filled by LDS-DMA, so linear in lane order; the swizzles are applied on the SOURCE address and again
// on the read, guide §5.4 rule 21):
//   K tile  [64 keys][D halves], row stride 2D bytes, chunk c of row k at slot c ^ kswz(k): conflict-free ds_read_b128
//           (kswz = 0 for D=40 whose 80-byte stride already spreads 16 rows over 16 slots, (k>>3)&1 for D=80,
//           (k>>2)&3 for D=160).
//   VT tile [D rows][64 keys], row stride 128 bytes, chunk c of row d at slot c ^ ((d>>1)&7).
// Online softmax runs in the log2 domain with the scale folded into the exponent's FMA, and rescales the accumulators
// only when some row's running max grows by more than 2^6 (wave-uniform branch; P <= 64 stays exact enough in fp16
// and the row sums are fp32).
#include "attention_kernel.h"
#include <float.h>

using namespace sgattn;


// Validates a descriptor and translates it into kernel parameters.
//
// 32-bit arithmetic of the kernels (attention_kernel.h) and what bounds it here:
//   row * (int)ldk + col    K-side DMA offsets, `unsigned` in attn_fwd_body, `int` in attn_d40_body: row <= 63, col < D <= 160 <= ldk, so
//                           the value is < 64 ldk — the check 64 ldk < 2^31 below (which also makes (int)ldk exact);
//   d * (int)ldvt + col     V^T-side DMA offsets: d <= D - 1, col <= 56, so the value is <= D ldvt - ldvt + 56 — the check D ldvt < 2^31
//                           (an ldvt <= 56 is nowhere near it; the check also makes (int)ldvt exact);
//   (qb NW + wave) 32, tile 64 + ..., (tile + 1) 64, (Nk + 7) & ~7, (Nk + 63) / 64
//                           query / key indices rounded up to a block: < N + 128 — the check Nq, Nk <= 2^30;
//   nqb * H * B             the grid (an `int` product in the launchers, and HIP's own limit) — planned in 64 bits and checked < 2^31;
//   work / nqb, bh / B, b - (B - kv_batches), h * D
//                           indices below the grid size, the batch or H D <= ldq.
// Everything else (batch, token and head offsets into the operands, the lse2 index) is computed in `long`.
static int attn_params(const sg_attn_desc* d, AttnParams& p, const char* who) {
    SG_REQUIRE(d != nullptr, "%s: null descriptor", who);
    SG_REQUIRE(d->q && d->k && d->vt && d->o, "%s: null q/k/vt/o", who);
    SG_REQUIRE(d->B > 0 && d->H > 0 && d->Nq > 0 && d->Nk > 0, "%s: bad shape", who);
    if (d->D != 40 && d->D != 80 && d->D != 160)
        return sg_set_error(SG_EUNSUP, "%s: head dim %d not in {40, 80, 160}", who, d->D);
    SG_REQUIRE(d->Nq <= (1 << 30) && d->Nk <= (1 << 30), "%s: Nq and Nk must not exceed 2^30", who);
    // the general softmax takes the row maximum of the RAW scores and scales it afterwards, and masks the key tail with -inf before the
    // multiplication: a negative scale would pick the minimum, scale = 0 would make the tail 0 * -inf = NaN (the D = 40 fast path
    // pre-multiplies Q and would answer differently): one contract for every head dim
    SG_REQUIRE(d->scale > 0.f && d->scale <= FLT_MAX, "%s: scale must be finite and > 0", who);
    SG_REQUIRE(d->kv_batches >= 0 && d->kv_batches <= d->B, "%s: kv_batches must be in [0, B]", who);
    // query batch b >= kv_batches reads K/V row b - (B - kv_batches): negative (a read in front of the operand) unless 2 kv_batches >= B
    SG_REQUIRE(d->kv_batches == 0 || 2 * (int64_t)d->kv_batches >= d->B, "%s: kv_batches must be 0 or at least B / 2", who);
    SG_REQUIRE(d->ldq % 8 == 0 && d->ldk % 8 == 0 && d->ldvt % 8 == 0 && d->ldo % 4 == 0, "%s: row strides", who);
    SG_REQUIRE(d->bsq % 8 == 0 && d->bsk % 8 == 0 && d->bsvt % 8 == 0 && d->bso % 4 == 0, "%s: batch strides", who);
    SG_REQUIRE(sg_aligned16(d->q) && sg_aligned16(d->k) && sg_aligned16(d->vt) && sg_aligned16(d->o), "%s: 16-byte alignment", who);
    const int64_t hd = (int64_t)d->H * d->D;
    SG_REQUIRE(d->ldq >= hd && d->ldk >= hd && d->ldo >= hd, "%s: token stride smaller than H*D", who);
    SG_REQUIRE(d->ldvt >= ((d->Nk + 7) & ~7), "%s: ldvt must cover Nk rounded up to 8 keys", who);
    SG_REQUIRE((int64_t)d->D * d->ldvt < (1ll << 31), "%s: VT head slab too large for 32-bit offsets", who);
    SG_REQUIRE(d->ldk < (1ll << 25), "%s: K tile (64 ldk) too large for 32-bit offsets", who);
    p = AttnParams{};
    p.q = reinterpret_cast<const f16*>(d->q); p.ldq = d->ldq; p.bsq = d->bsq;
    p.k = reinterpret_cast<const f16*>(d->k); p.ldk = d->ldk; p.bsk = d->bsk;
    p.vt = reinterpret_cast<const f16*>(d->vt); p.ldvt = d->ldvt; p.bsvt = d->bsvt;
    p.o = reinterpret_cast<f16*>(d->o); p.ldo = d->ldo; p.bso = d->bso;
    p.B = d->B; p.H = d->H; p.Nq = d->Nq; p.Nk = d->Nk;
    p.kv_batches = d->kv_batches > 0 ? d->kv_batches : d->B;
    p.scale_log2 = d->scale * 1.44269504088896340736f;
    if (d->kv2_batches > 0) {      // leading K/V rows with their own key count (same token / row strides)
        SG_REQUIRE(d->k2 && d->vt2 && d->Nk2 > 0 && d->kv2_batches <= p.kv_batches, "%s: kv2_batches needs k2, vt2, Nk2 and at most kv_batches rows", who);
        SG_REQUIRE(d->bsk2 % 8 == 0 && d->bsvt2 % 8 == 0 && sg_aligned16(d->k2) && sg_aligned16(d->vt2), "%s: k2 / vt2 strides and alignment", who);
        SG_REQUIRE(d->ldvt >= ((d->Nk2 + 7) & ~7), "%s: ldvt must cover Nk2 rounded up to 8 keys", who);
        p.k2 = reinterpret_cast<const f16*>(d->k2); p.bsk2 = d->bsk2;
        p.vt2 = reinterpret_cast<const f16*>(d->vt2); p.bsvt2 = d->bsvt2;
        p.Nk2 = d->Nk2; p.kv2 = d->kv2_batches;
    }
    return SG_OK;
}

// ---- the launch plan: which kernel serves a descriptor, as a value (sg_attn_plan).  attn_plan alone decides, attn_launch alone maps a
// plan to an instantiation; sg_attn_fwd_plan / sg_attn_fwd_pair_plan answer from the same two functions the launches go through.

// 4-wave workgroups with a 3-deep ring when that still gives the chip >= 2 workgroups per CU (a property of the queries only)
static bool attn_big(const sg_attn_desc* d) { return (long)sg_cdiv(d->Nq, 128) * d->H * d->B >= 512; }

static int attn_plan_grid(sg_attn_plan& pl, const sg_attn_desc* d, int family, int waves, int stages, const char* who) {
    const int64_t wgs = (int64_t)sg_cdiv(d->Nq, family == SG_ATTN_KSPLIT ? 32 : 32 * waves) * d->H * d->B;
    SG_REQUIRE(wgs < (1ll << 31), "%s: %lld workgroups do not fit a grid", who, (long long)wgs);
    pl.family = family; pl.waves = waves; pl.stages = stages; pl.workgroups = (int32_t)wgs;
    return SG_OK;
}

// d has passed attn_params
static int attn_plan(const sg_attn_desc* d, bool lse, sg_attn_plan& pl, const char* who) {
    // training forward (sg_attn_fwd_lse_f16): the default instantiations with the log-sum-exp rows stored.
    // D = 40: the GENERAL softmax (fp32 scores, fp32 running maximum), not the padded-head-dimension fast path — that one rounds
    // scale * log2(e) * Q to fp16 and keeps the maximum as two fp16 values, which costs lse2 ~|lse2| * 2^-12: 4e-4 .. 8e-4 on N(0, 1)
    // inputs and 1.3e-2 at a common logit offset of ~70 (tests/test_attention_backward_edges_gpu.py, bar 2e-3; the other head
    // dims: 1e-6).  The backward recomputes every P from lse2, so the training forward pays the ~66 VALU instructions per tile.
    if (lse) return attn_plan_grid(pl, d, SG_ATTN_LSE, 4, 3, who);
    const bool big = attn_big(d);
    const SgOptions& opt = sg_options();          // development options (sg_debug_set_option), defaults in common.h
    // Every head dim runs 4 waves on a 3-deep ring where the grid allows it (measured against 2 waves and 2 stages at D = 80 / 160: HISTORY.md §5.1).
    if (d->D == 40) {
        if (big && opt.attn_d40_general) return attn_plan_grid(pl, d, SG_ATTN_GENERAL, 4, 3, who);   // round-3 softmax (A/B)
        if (big && opt.attn_lean) return attn_plan_grid(pl, d, SG_ATTN_LEAN, 4, 3, who);   // V^T fragments per k-step: fewer VGPRs
        // round 7: tile 0 / branch-free steady state / drain (attn_d40_body, bit-identical); option attn_d40_loop = 1: the shared body
        return attn_plan_grid(pl, d, opt.attn_d40_loop == 1 ? SG_ATTN_SHARED_BODY : SG_ATTN_D40_LOOP, big ? 4 : 2, big ? 3 : 2, who);
    }
    // D = 160, round 5: at Nq <= 256 (the 16x16 / 8x8 levels) the four waves of a workgroup split the KEYS of one 32-query block instead
    // of taking 32 queries each (attn_fwd_ksplit_kernel) — only where it wins: one round of workgroups (a 160 KB workgroup owns its CU)
    // and at least two tiles of keys; batch 20 of the batched reference pass, 1 280 workgroups, measured 42.7 vs 27.4 us.
    // option attn_d160 = 4 (default); 3 = always the query-split kernel (what the parity tests compare against)
    if (d->D == 160 && opt.attn_d160 == 4 && d->Nq <= 256 && d->Nk > KVBLK && (long)sg_cdiv(d->Nq, 32) * d->H * d->B <= 256)
        return attn_plan_grid(pl, d, SG_ATTN_KSPLIT, 4, 1, who);
    return attn_plan_grid(pl, d, SG_ATTN_GENERAL, 4, 3, who);
}

static int attn_launch(const AttnParams& p, int D, const sg_attn_plan& pl, hipStream_t st) {
    const bool big = pl.waves == 4;
    switch (pl.family) {
    case SG_ATTN_LSE:
        if (D == 40) launch_attn<40, 4, 3, true, false, true>(p, st);
        else if (D == 80) launch_attn<80, 4, 3, true>(p, st);
        else launch_attn<160, 4, 3, true>(p, st);
        return SG_OK;
    case SG_ATTN_D40_LOOP: big ? launch_attn_d40<4, 3>(p, st) : launch_attn_d40<2, 2>(p, st); return SG_OK;
    case SG_ATTN_SHARED_BODY: big ? launch_attn<40, 4, 3>(p, st) : launch_attn<40, 2, 2>(p, st); return SG_OK;
    case SG_ATTN_LEAN: launch_attn<40, 4, 3, false, true>(p, st); return SG_OK;
    case SG_ATTN_KSPLIT: launch_attn_ksplit<160, 4>(p, st); return SG_OK;
    case SG_ATTN_GENERAL:
        if (D == 40) launch_attn<40, 4, 3, false, false, true>(p, st);
        else if (D == 80) launch_attn<80, 4, 3>(p, st);
        else launch_attn<160, 4, 3>(p, st);
        return SG_OK;
    }
    return sg_set_error(SG_EINVAL, "attention: internal: no kernel for plan family %d", pl.family);
}

static int attn_fwd(const sg_attn_desc* d, float* lse2, sg_stream_t stream) {
    const char* who = lse2 ? "sg_attn_fwd_lse_f16" : "sg_attn_fwd_f16";
    AttnParams p;
    sg_attn_plan pl;
    if (int rc = attn_params(d, p, "sg_attn_fwd_f16")) return rc;
    if (int rc = attn_plan(d, lse2 != nullptr, pl, "sg_attn_fwd_f16")) return rc;
    p.lse2 = lse2;
    if (int rc = attn_launch(p, d->D, pl, (hipStream_t)stream)) return rc;
    SG_CHECK_LAUNCH(who);
    return SG_OK;
}

extern "C" int sg_attn_fwd_f16(const sg_attn_desc* d, sg_stream_t stream) { return attn_fwd(d, nullptr, stream); }

extern "C" int sg_attn_fwd_plan(const sg_attn_desc* d, int32_t lse, sg_attn_plan* out) {
    SG_REQUIRE(out != nullptr, "sg_attn_fwd_plan: null plan");
    AttnParams p;
    if (int rc = attn_params(d, p, "sg_attn_fwd_plan")) return rc;
    return attn_plan(d, lse != 0, *out, "sg_attn_fwd_plan");
}

// Two attentions over the same query geometry (B, H, Nq, D) in one launch — the text and the image cross-attention of one
// BasicTransformerBlock.  The longer key loop is numbered first.  Pairs that the default instantiation table would not serve with
// one kernel (development options set, different query geometry) are simply launched one after the other.
static int attn_pair_plan(const sg_attn_desc* d0, const sg_attn_desc* d1, sg_attn_pair_plan& pr, const char* who) {
    const SgOptions& opt = sg_options();
    const bool same = d0->D == d1->D && d0->B == d1->B && d0->H == d1->H && d0->Nq == d1->Nq;   // (short K/V rows: either problem)
    const bool defaults = !(d0->D == 40 && opt.attn_d40_loop == 1);
    pr = sg_attn_pair_plan{};
    if (!same || !defaults) {
        if (int rc = attn_plan(d0, false, pr.p0, who)) return rc;
        return attn_plan(d1, false, pr.p1, who);
    }
    const bool big = d0->D != 40 || attn_big(d0);
    const int family = d0->D == 40 ? SG_ATTN_D40_LOOP : SG_ATTN_GENERAL;
    if (int rc = attn_plan_grid(pr.p0, d0, family, big ? 4 : 2, big ? 3 : 2, who)) return rc;
    pr.p1 = pr.p0;                                 // same query geometry: same sub-grid
    SG_REQUIRE((int64_t)pr.p0.workgroups * 2 < (1ll << 31), "%s: the shared grid does not fit", who);
    pr.shared = 1;
    pr.first = d0->Nk >= d1->Nk ? 0 : 1;
    pr.workgroups = 2 * pr.p0.workgroups;
    return SG_OK;
}

extern "C" int sg_attn_fwd_pair_plan(const sg_attn_desc* d0, const sg_attn_desc* d1, sg_attn_pair_plan* out) {
    SG_REQUIRE(out != nullptr, "sg_attn_fwd_pair_plan: null plan");
    AttnParams p0, p1;
    if (int rc = attn_params(d0, p0, "sg_attn_fwd_pair_plan[0]")) return rc;
    if (int rc = attn_params(d1, p1, "sg_attn_fwd_pair_plan[1]")) return rc;
    return attn_pair_plan(d0, d1, *out, "sg_attn_fwd_pair_plan");
}

extern "C" int sg_attn_fwd_pair_f16(const sg_attn_desc* d0, const sg_attn_desc* d1, sg_stream_t stream) {
    AttnParams p0, p1;
    sg_attn_pair_plan pr;
    if (int rc = attn_params(d0, p0, "sg_attn_fwd_pair_f16[0]")) return rc;
    if (int rc = attn_params(d1, p1, "sg_attn_fwd_pair_f16[1]")) return rc;
    if (int rc = attn_pair_plan(d0, d1, pr, "sg_attn_fwd_pair_f16")) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!pr.shared) {
        if (int rc = attn_launch(p0, d0->D, pr.p0, st)) return rc;
        SG_CHECK_LAUNCH("sg_attn_fwd_pair_f16[0]");
        if (int rc = attn_launch(p1, d1->D, pr.p1, st)) return rc;
        SG_CHECK_LAUNCH("sg_attn_fwd_pair_f16[1]");
        return SG_OK;
    }
    const AttnParams& a = pr.first == 0 ? p0 : p1;
    const AttnParams& b = pr.first == 0 ? p1 : p0;
    if (d0->D == 40) {
        if (pr.p0.waves == 4) launch_attn_d40_pair<4, 3>(a, b, st);
        else launch_attn_d40_pair<2, 2>(a, b, st);
    } else if (d0->D == 80) launch_attn_pair<80, 4, 3>(a, b, st);
    else launch_attn_pair<160, 4, 3>(a, b, st);
    SG_CHECK_LAUNCH("sg_attn_fwd_pair_f16");
    return SG_OK;
}

extern "C" int sg_attn_fwd_lse_f16(const sg_attn_desc* d, float* lse2, sg_stream_t stream) {
    SG_REQUIRE(lse2 != nullptr, "sg_attn_fwd_lse_f16: null lse2");
    return attn_fwd(d, lse2, stream);
}
