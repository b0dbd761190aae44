// Encoder-class attention for gfx950: O[b,i,h*D+:] = softmax_j(scale * Q.K + key_bias[b,j], j <= i when causal) . V — the contract of
// sg_attn_small_f16 (encoders.hip) for the sequences that kernel cannot hold: up to 1024 tokens, head dim up to 128 (CLIP ViT-H/14, the
// image tower of PickScore: 257 tokens x 16 heads of 80; ViT-L/14 257 x 64, ViT-L/14@336 577 tokens).
//
// Operands: Q, K, V and O token-major [B, T, H*D] views (slices of the fused qkv GEMM's output), V NOT transposed.
//
// Work decomposition: grid (heads, batches, ceil(T / 128)); one workgroup = 4 wave64, each wave owns 32 queries.  K and V are streamed in
// tiles of EA_KT = 64 keys through ONE LDS image each ([64 keys][DP + 8 halves], DP = D rounded up to 32, zero-filled beyond D and beyond
// T), register-staged: the global loads of tile t + 1 are issued before the MFMAs of tile t and written after the barrier that retires
// tile t's reads.  LDS use is 2 * 64 * (DP + 8) * 2 + 256 bytes whatever T is.
//
// MFMA formulation (v_mfma_f32_32x32x16_f16), the one of attention.hip, so that a query's softmax row never leaves its lane pair:
//   S^T[key, q] = sum_d K[key, d] Q[q, d]     A = K rows (ds_read_b128 of 8 consecutive halves), B = Q^T fragments (registers, loaded once)
//     accumulator register r of lane (q = l & 31, hi = l >> 5) holds key (r & 3) + 8 (r >> 2) + 4 hi of the 32-key block.
//   O^T[d, q]   = sum_key V^T[d, key] P^T[key, q]    B = the lane's own P registers 8 s .. 8 s + 7 converted to fp16 (k-step s: its element j
//     is key 16 s + 8 (j >> 2) + 4 hi + (j & 3)), A = V^T in that same key order, read from the token-major V image with the transposing
//     LDS read (ds_read_b64_tr_b16: per 16 lanes a block of 4 keys x 16 channels, lane i receives channel i of the 4 keys).  Every lane
//     supplies an in-bounds, 8-byte-aligned address and no lane is masked when the reads issue (the tile is padded instead).
// Softmax: fp32, log2 domain (scale * log2(e) folded into one FMA with the bias), online over the key tiles; the row maximum needs one
// exchange with lane l ^ 32 per tile, the row sum one at the end.  Masked scores are -inf (keys >= T, causal); a key bias of
// finfo(float32).min stays finite (clamped to -FLT_MAX after the log2(e) factor), so a tile whose keys are all biased away contributes
// exp2(-FLT_MAX - m) = 0 and leaves the running maximum alone, and a row with every key biased away is the uniform average, as in
// sg_attn_small_f16.
#include <float.h>

#include "common.h"

namespace {

constexpr int EA_KT = 64;      // keys per tile
constexpr int EA_QB = 128;     // queries per workgroup (4 waves x 32)

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

union H4x2 {
    f16x8 v;
    s16x4 h[2];
};

struct EncParams {
    const f16 *q, *k, *v;
    f16* o;
    long ldq, bsq, ldk, bsk, ldv, bsv, ldo, bso;
    const float* key_bias;
    int T, D, causal;
    float scale_log2;
};

template <int NB>      // head dim padded to DP = 32 * NB channels
__global__ __launch_bounds__(256) void attn_enc_kernel(EncParams p) {
    constexpr int DP = 32 * NB, LD = DP + 8, CPR = DP / 8;      // LD: 16-byte chunks per row is odd -> row reads spread over the banks
    __shared__ __attribute__((aligned(16))) f16 sK[EA_KT * LD];
    __shared__ __attribute__((aligned(16))) f16 sV[EA_KT * LD];
    __shared__ __attribute__((aligned(16))) float sB[EA_KT];

    const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, hi = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int h = blockIdx.x, b = blockIdx.y, q0 = blockIdx.z * EA_QB;
    const int T = p.T, D = p.D;
    const int qw = q0 + 32 * w, qi = qw + l31;
    const int Tk = p.causal ? min(T, q0 + EA_QB) : T;            // keys this workgroup can see
    const int ntiles = (Tk + EA_KT - 1) / EA_KT;

    // ---- Q^T fragments: element j of k-step st = Q[qi][16 st + 8 hi + j]; zero beyond D and for rows >= T
    f16x8 qf[2 * NB];
    {
        const f16* qp = p.q + (long)b * p.bsq + (long)qi * p.ldq + h * D;
#pragma unroll
        for (int st = 0; st < 2 * NB; ++st) {
            const int d = 16 * st + 8 * hi;
            H8 x;
            x.u = make_uint4(0u, 0u, 0u, 0u);
            if (qi < T && d < D) x.u = ldg16(qp + d);
            qf[st] = x.v;
        }
    }

    // ---- staging: thread t moves chunks t + 256 i (i < NB) of the [64][CPR] chunk grid of K and of V
    const f16* kbase = p.k + (long)b * p.bsk + h * D;
    const f16* vbase = p.v + (long)b * p.bsv + h * D;
    uint4 kreg[NB], vreg[NB];
    float breg = 0.f;
    auto load_tile = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = t + 256 * i, row = idx / CPR, c = idx - row * CPR, key = k0 + row;
            kreg[i] = make_uint4(0u, 0u, 0u, 0u);
            vreg[i] = make_uint4(0u, 0u, 0u, 0u);
            if (key < T && c * 8 < D) {                      // never reads a key >= T
                kreg[i] = ldg16(kbase + (long)key * p.ldk + c * 8);
                vreg[i] = ldg16(vbase + (long)key * p.ldv + c * 8);
            }
        }
        if (t < EA_KT) {
            const int key = k0 + t;
            breg = -INFINITY;
            if (key < T) breg = p.key_bias ? fmaxf(p.key_bias[(long)b * T + key] * 1.44269504088896340736f, -FLT_MAX) : 0.f;
        }
    };
    auto write_tile = [&]() {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = t + 256 * i, row = idx / CPR, c = idx - row * CPR;
            *reinterpret_cast<uint4*>(sK + row * LD + c * 8) = kreg[i];
            *reinterpret_cast<uint4*>(sV + row * LD + c * 8) = vreg[i];
        }
        if (t < EA_KT) sB[t] = breg;
    };

    // lane addresses: K row read (row l31 of a 32-key block, 8 halves at 8 hi of a k-step); transposing V read (16-lane group g: keys
    // 4 hi + (0..3), channels 16 (g & 1) + (0..15); lane 4 r + c of the group supplies key 4 hi + r, channels 16 (g & 1) + 4 c ..)
    const f16* kread = sK + l31 * LD + 8 * hi;
    const f16* vread = sV + (4 * hi + ((lane >> 2) & 3)) * LD + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);

    f32x16 oacc[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    load_tile(0);
    for (int tile = 0; tile < ntiles; ++tile) {
        const int k0 = tile * EA_KT;
        __syncthreads();                       // the previous tile's LDS reads are done
        write_tile();
        __syncthreads();
        if (tile + 1 < ntiles) load_tile(k0 + EA_KT);
        // wave-uniform: waves without a live query, or (causal) entirely above the diagonal, only help staging
        if (qw >= T || (p.causal && k0 > qw + 31)) continue;

        // ---- S^T = K Q^T, two blocks of 32 keys
        f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
#pragma unroll
            for (int st = 0; st < 2 * NB; ++st) {
                if (16 * st < D) {             // (uniform) the k-steps that hold only padding are skipped
                    const f16x8 kf = *reinterpret_cast<const f16x8*>(kread + (32 * kb) * LD + 16 * st);
                    s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[st], s[kb], 0, 0, 0);
                }
            }
        }

        // ---- scores in the log2 domain, masks, running maximum
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 bias = *reinterpret_cast<const float4*>(sB + 32 * kb + 8 * g + 4 * hi);
                s[kb][4 * g + 0] = fmaf(s[kb][4 * g + 0], p.scale_log2, bias.x);
                s[kb][4 * g + 1] = fmaf(s[kb][4 * g + 1], p.scale_log2, bias.y);
                s[kb][4 * g + 2] = fmaf(s[kb][4 * g + 2], p.scale_log2, bias.z);
                s[kb][4 * g + 3] = fmaf(s[kb][4 * g + 3], p.scale_log2, bias.w);
            }
        if (p.causal && k0 + EA_KT - 1 > qw) {          // (wave-uniform) only the tiles that touch the diagonal pay for the mask
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (k0 + 32 * kb + (r & 3) + 8 * (r >> 2) + 4 * hi > qi) s[kb][r] = -INFINITY;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_ref = m_new == -INFINITY ? 0.f : m_new;       // a row with nothing to see yet: every exp2 below is exp2(-inf) = 0
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_ref);  // 0 on the first tile
        m_run = m_new;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
        }
        float psum = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = __builtin_amdgcn_exp2f(s[kb][r] - m_ref);
                s[kb][r] = e;
                psum += e;
            }
        l_run = fmaf(l_run, alpha, psum);

        // ---- O^T += V^T P^T: 4 k-steps of 16 keys
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            f16x8 pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = (f16)s[ks >> 1][(ks & 1) * 8 + j];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                if (32 * i < D) {
                    H4x2 vf;
                    vf.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(vread + (16 * ks) * LD + 32 * i));
                    vf.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(vread + (16 * ks + 8) * LD + 32 * i));
                    oacc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf.v, pf, oacc[i], 0, 0, 0);
                }
            }
        }
    }

    // ---- epilogue: lane (q, hi) holds channels 32 i + 8 g + 4 hi + (0..3) of query q in registers 4 g .. 4 g + 3: one 8-byte store each
    const float l = l_run + __shfl_xor(l_run, 32, 64);
    if (qi < T) {
        const float inv = 1.0f / l;
        f16* op = p.o + (long)b * p.bso + (long)qi * p.ldo + h * D;
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = 32 * i + 8 * g + 4 * hi;
                if (d < D) {
                    f16x4 ov;
#pragma unroll
                    for (int e = 0; e < 4; ++e) ov[e] = (f16)(oacc[i][4 * g + e] * inv);
                    *reinterpret_cast<f16x4*>(op + d) = ov;
                }
            }
    }
}

}  // namespace

extern "C" int sg_attn_enc_f16(const sg_half* q, int64_t ldq, int64_t bsq, const sg_half* k, int64_t ldk, int64_t bsk, const sg_half* v,
                               int64_t ldv, int64_t bsv, sg_half* o, int64_t ldo, int64_t bso, const float* key_bias, int32_t B,
                               int32_t H, int32_t T, int32_t D, float scale, int32_t causal, sg_stream_t stream) {
    SG_REQUIRE(q && k && v && o, "sg_attn_enc: null pointer");
    SG_REQUIRE(B > 0 && B <= 65535 && H > 0, "sg_attn_enc: bad shape B=%d H=%d", B, H);
    SG_REQUIRE(T >= 1 && T <= 1024, "sg_attn_enc: needs 1 <= T <= 1024 (got T=%d)", T);
    SG_REQUIRE(D >= 8 && D <= 128 && D % 8 == 0, "sg_attn_enc: head dim must be a multiple of 8 in [8, 128] (got D=%d)", D);
    const int64_t hd = (int64_t)H * D;
    SG_REQUIRE(ldq >= hd && ldk >= hd && ldv >= hd && ldo >= hd, "sg_attn_enc: token stride below H*D");
    SG_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0 && bsq % 8 == 0 && bsk % 8 == 0 && bsv % 8 == 0 && bso % 8 == 0,
               "sg_attn_enc: token and batch strides must be multiples of 8 elements");
    SG_REQUIRE(sg_aligned16(q) && sg_aligned16(k) && sg_aligned16(v) && sg_aligned16(o), "sg_attn_enc: 16-byte alignment");
    SG_REQUIRE(key_bias == nullptr || (reinterpret_cast<uintptr_t>(key_bias) & 3u) == 0, "sg_attn_enc: key_bias alignment");
    SG_REQUIRE(causal == 0 || causal == 1, "sg_attn_enc: causal must be 0 or 1");
    EncParams p;
    p.q = reinterpret_cast<const f16*>(q), p.k = reinterpret_cast<const f16*>(k), p.v = reinterpret_cast<const f16*>(v);
    p.o = reinterpret_cast<f16*>(o);
    p.ldq = ldq, p.bsq = bsq, p.ldk = ldk, p.bsk = bsk, p.ldv = ldv, p.bsv = bsv, p.ldo = ldo, p.bso = bso;
    p.key_bias = key_bias;
    p.T = T, p.D = D, p.causal = causal;
    p.scale_log2 = scale * 1.44269504088896340736f;
    const dim3 grid(H, B, (T + EA_QB - 1) / EA_QB);
    hipStream_t st = (hipStream_t)stream;
    switch ((D + 31) / 32) {
        case 1: hipLaunchKernelGGL(attn_enc_kernel<1>, grid, dim3(256), 0, st, p); break;
        case 2: hipLaunchKernelGGL(attn_enc_kernel<2>, grid, dim3(256), 0, st, p); break;
        case 3: hipLaunchKernelGGL(attn_enc_kernel<3>, grid, dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL(attn_enc_kernel<4>, grid, dim3(256), 0, st, p); break;
    }
    SG_CHECK_LAUNCH("sg_attn_enc_f16");
    return SG_OK;
}
