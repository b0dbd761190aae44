// fp8 (OCP e4m3) attention forward for head dim 40 on gfx950 — BASELINE config 5 ("768x768 latent, 5 prior-frame context,
// fp8 MFMA attention path"): the D = 40 self- and image-cross-attention of the 96x96 level, whose 46 080-key context
// dominates that configuration (model/attention.py:255-260, 285-290).
//
// Two entry points:
//   sg_attn_f8_pack    fp16 Q / K / V^T operands (exactly what the projection GEMMs produce for sg_attn_fwd_f16) -> e4m3 operand
//                      images, one per (batch, head), rows padded to 64 bytes:
//                        Q8 / K8 [B][H][N][64]        row = token, byte d < 40 = e4m3(x), bytes 40..63 = 0
//                        VT8     [B][H][64][Nkp]      row = d (rows >= 40 zero), Nkp = Nk rounded up to 64, keys PERMUTED inside
//                                                     every 64-key tile (below); keys >= Nk are zero
//   sg_attn_fwd_f8_d40 the attention itself on those images; output fp16 [B, Nq, H*40] like the fp16 kernel.
//
// MFMA formulation — v_mfma_scale_f32_32x32x64_f8f6f4 with unit scales, operand map established on the device by
// tools/probe_mfma_f8.py (round 2: the natural map, lane = row/col + 32 (k / 32), byte = k % 32, confirmed to 1.3e-5):
//   S^T[key, q] = sum_d K[key, d] Q[q, d]     ONE MFMA per 32-key block (k = d padded 40 -> 64): A = K8 rows, 32 bytes per lane
//                                              (two ds_read_b128), B = Q8 row of the lane's query (registers)
//   O^T[d, q]  += sum_kk VT[d, kk] P^T[kk, q]  ONE MFMA per 32-row d-tile per 64-key tile (k = the whole tile): B = the lane's own
//                                              32 probabilities as e4m3 — accumulator register r of block kb (key kb*32 + (r&3) +
//                                              8 (r>>2) + 4 hi) becomes byte kb*16 + r, i.e. contraction index kk = 32 hi + 16 kb + r.
//                                              VT8 is stored with exactly that permutation of the keys inside each 64-key tile, so the
//                                              A fragment is again 32 contiguous bytes.  P never leaves the lane.
// 4 MFMAs of 64 cycles per 64-key tile and wave instead of 14 of 32 (fp16 kernel): 256 vs 448 matrix-pipe cycles.
// Softmax: fp32, log2 domain, deferred rescale as in the fp16 kernel but with a threshold of 2x (P <= 2 between rescales).
// P is stored as e4m3(128 P) — the factor is folded into the exponent — representable down to 2^-16 of the running max
// instead of 2^-9; the row sums are accumulated from the UNQUANTISED fp32 values (128 P as well, so O' / l needs no correction).
// LDS images (LDS-DMA, 1 KiB segments of 16 rows x 64 B): 16-byte slot c of row r is stored at slot c ^ ((r >> 2) & 3) —
// 16 consecutive rows read the same logical slot conflict-free (4 rows per 256-byte bank row x 4 distinct slots).
#include "common.h"
#include <float.h>

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
constexpr int KV = 64;                    // keys per tile
constexpr float RESCALE_THR = 1.0f;       // log2 units: P <= 2 between rescales, so 128 P <= 256 fits e4m3 (max 448)
constexpr int UNIT_SCALE = 0x7F7F7F7F;    // E8M0 127 = 2^0 in every byte lane of the scale operand

__device__ __forceinline__ void glds16b(const void* g, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ int pack4_fp8(float a, float b, float c, float d) {
    int v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    return __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
}
__device__ __forceinline__ float clamp448(float x) { return fminf(fmaxf(x, -448.f), 448.f); }

// ------------------------------------------------------------------------------------------------ operand packing
struct PackParams {
    const f16* src; long ld, bs;          // Q / K: [B, N, H*40] (ld = token stride); VT: [B, H*40, Nk''] (ld = row stride)
    unsigned char* dst;
    int B, H, N, Nkp, mode;               // mode 0: token-major rows (Q, K); 1: VT with the in-tile key permutation
};

__global__ __launch_bounds__(256) void attn_f8_pack_kernel(const PackParams p) {
    if (p.mode == 0) {
        // one thread = 16 output bytes (a quarter row): items [B*H*N*4]
        const long total = (long)p.B * p.H * p.N * 4;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
            const int c = (int)(i & 3);
            const long row = i >> 2;
            const int n = (int)(row % p.N);
            const long bh = row / p.N;
            const int h = (int)(bh % p.H), b = (int)(bh / p.H);
            int4 out = make_int4(0, 0, 0, 0);
            if (c * 16 < 40) {
                const f16* s = p.src + (long)b * p.bs + (long)n * p.ld + h * 40 + c * 16;
                float v[16];
                H8 x0; x0.u = ldg16(s);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = clamp448((float)x0.h[j]);
                if (c < 2) {
                    H8 x1; x1.u = ldg16(s + 8);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[8 + j] = clamp448((float)x1.h[j]);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[8 + j] = 0.f;          // d = 40..47
                }
                out = make_int4(pack4_fp8(v[0], v[1], v[2], v[3]), pack4_fp8(v[4], v[5], v[6], v[7]),
                                pack4_fp8(v[8], v[9], v[10], v[11]), pack4_fp8(v[12], v[13], v[14], v[15]));
            }
            *reinterpret_cast<int4*>(p.dst + row * 64 + c * 16) = out;
        }
    } else {
        // VT: one thread = 16 output bytes = contraction indices kk0 .. kk0+15 of one (b, h, d, tile): kk = 32 hi + 16 kb + r
        // <-> key = 32 kb + (r & 3) + 8 (r >> 2) + 4 hi, i.e. four groups of 4 consecutive keys.  items [B*H*64*(Nkp/16)]
        const int tpr = p.Nkp / 16;
        const long total = (long)p.B * p.H * 64 * tpr;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
            const int q16 = (int)(i % tpr);
            const long rowi = i / tpr;
            const int d = (int)(rowi & 63);
            const long bh = rowi >> 6;
            const int h = (int)(bh % p.H), b = (int)(bh / p.H);
            int4 out = make_int4(0, 0, 0, 0);
            if (d < 40) {
                const int tile = q16 >> 2, sub = q16 & 3;             // sub = 2 hi + kb
                const int hi = sub >> 1, kb = sub & 1;
                const f16* s = p.src + (long)b * p.bs + (long)(h * 40 + d) * p.ld + tile * 64 + kb * 32 + 4 * hi;
                int w[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {                          // r = 4 g .. 4 g + 3 -> keys 8 g .. 8 g + 3 (+ 32 kb + 4 hi)
                    float v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int key = tile * 64 + kb * 32 + 4 * hi + 8 * g + j;
                        v[j] = key < p.N ? clamp448((float)s[8 * g + j]) : 0.f;
                    }
                    w[g] = pack4_fp8(v[0], v[1], v[2], v[3]);
                }
                out = make_int4(w[0], w[1], w[2], w[3]);
            }
            *reinterpret_cast<int4*>(p.dst + rowi * p.Nkp + q16 * 16) = out;
        }
    }
}

// ------------------------------------------------------------------------------------------------ attention
struct F8Params {
    const unsigned char* q8; const unsigned char* k8; const unsigned char* vt8;
    f16* o; long ldo, bso;
    int B, H, Nq, Nk, Nkp, kv_batches, nqb;
    float scale_log2;
};

template <int NW, int S>
__global__ __launch_bounds__(64 * NW) void attn_fwd_f8_kernel(const F8Params p) {
    constexpr int K_SEG = 4, V_SEG = 3, NSEG = K_SEG + V_SEG;        // 1 KiB segments per tile: 64 keys x 64 B, 48 d-rows x 64 B
    constexpr int TSTAGE = 8192;                                     // K image 4 KiB + V image 4 KiB (rows 48..63 never loaded/used)
    constexpr int MAXL = (NSEG + NW - 1) / NW, REM = NSEG % NW;
    static_assert(S == 2 || S == 3, "2 or 3 stages");
    __shared__ __attribute__((aligned(16))) char smem[S * TSTAGE];

    const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int work = xcd_remap(blockIdx.x, gridDim.x);               // head-major: an XCD works on one head at a time
    const int bh = work / p.nqb, qb = work - bh * p.nqb;
    const int h = bh / p.B, b = bh - h * p.B;
    const int kvb = b < p.kv_batches ? b : b - (p.B - p.kv_batches);
    const int q0 = (qb * NW + wave) * 32;
    const unsigned char* Q8 = p.q8 + ((long)b * p.H + h) * p.Nq * 64;
    const unsigned char* K8 = p.k8 + ((long)kvb * p.H + h) * (long)p.Nk * 64;
    const unsigned char* VT8 = p.vt8 + ((long)kvb * p.H + h) * 64 * (long)p.Nkp;
    const int ntiles = (p.Nk + KV - 1) / KV;

    // DMA: segment g covers rows 16 (g % 4) .. +15 of the K (g < 4) or V image; lane = (row & 15) * 4 + stored slot
    auto issue_tile = [&](int tile, char* base) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < MAXL; ++i) {
            const int g = i * NW + wave;                             // wave-uniform
            if (g >= NSEG) continue;
            const int row = (g & 3) * 16 + (lane >> 2);
            const int slot = (lane & 3) ^ ((row >> 2) & 3);          // logical 16-byte slot this lane fetches
            if (g < K_SEG) {
                const int key = min(tile * KV + row, p.Nk - 1);      // tail rows: duplicates (finite; masked by the softmax)
                glds16b(K8 + (long)key * 64 + slot * 16, base + g * 1024);
            } else {
                glds16b(VT8 + (long)row * p.Nkp + tile * KV + slot * 16, base + g * 1024);
            }
        }
    };

    // Q fragment: the lane's query row, bytes [32 hi, 32 hi + 32)
    v8i qf;
    {
        const int qi = min(q0 + l31, p.Nq - 1);
        const int4 a = *reinterpret_cast<const int4*>(Q8 + (long)qi * 64 + hi * 32);
        const int4 c = *reinterpret_cast<const int4*>(Q8 + (long)qi * 64 + hi * 32 + 16);
        qf[0] = a.x; qf[1] = a.y; qf[2] = a.z; qf[3] = a.w; qf[4] = c.x; qf[5] = c.y; qf[6] = c.z; qf[7] = c.w;
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): only the LDS-DMA ring may be in flight inside the tile loop

    f32x16 oacc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

#pragma unroll
    for (int s = 0; s < S - 1; ++s)
        if (s < ntiles) issue_tile(s, smem + s * TSTAGE);

    // fragment read offsets: row r, bytes [32 hi, 32 hi + 32) = logical slots 2 hi, 2 hi + 1
    auto frag = [&](const char* img, int row) __attribute__((always_inline)) {
        const int sw = (row >> 2) & 3;
        const int4 a = *reinterpret_cast<const int4*>(img + row * 64 + (((2 * hi) ^ sw) << 4));
        const int4 c = *reinterpret_cast<const int4*>(img + row * 64 + (((2 * hi + 1) ^ sw) << 4));
        v8i f;
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = c.x; f[5] = c.y; f[6] = c.z; f[7] = c.w;
        return f;
    };
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    int stage = 0;
    for (int tile = 0; tile < ntiles; ++tile) {
        if (S == 3 && tile + 1 < ntiles) {
            if (REM == 0 || wave < REM) wait_vm<MAXL>();
            else wait_vm<(MAXL > 1 ? MAXL - 1 : 0)>();
        } else {
            wait_vm<0>();
        }
        __builtin_amdgcn_s_barrier();
        if (tile + S - 1 < ntiles) {
            int st = stage + S - 1;
            if (st >= S) st -= S;
            issue_tile(tile + S - 1, smem + st * TSTAGE);
        }
        const char* sK = smem + stage * TSTAGE;
        const char* sV = sK + 4096;
        // ---- S^T = K Q^T: one MFMA per 32-key block
        const v8i k0 = frag(sK, l31), k1 = frag(sK, 32 + l31);
        const v8i v0 = frag(sV, l31), v1 = frag(sV, min(32 + l31, 47));          // d rows 48..63: duplicates, never stored
        f32x16 s[2];
        s[0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(k0, qf, zero16, 0, 0, 0, UNIT_SCALE, 0, UNIT_SCALE);
        s[1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(k1, qf, zero16, 0, 0, 0, UNIT_SCALE, 0, UNIT_SCALE);
        // ---- online softmax (log2 domain); register r of block kb <-> key 64 tile + 32 kb + (r & 3) + 8 (r >> 2) + 4 hi
        if ((tile + 1) * KV > p.Nk) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (tile * KV + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi >= p.Nk) s[kb][r] = -INFINITY;
        }
        float mx = s[0][0];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * p.scale_log2;
        if (__builtin_amdgcn_ballot_w64(mx - m_run > RESCALE_THR) != 0) {
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
        }
        // e = 128 P: the factor rides in the exponent (m_run - 7), so quantisation needs no multiply, and P <= 2^RESCALE_THR = 2
        // between rescales keeps 128 P <= 256 < 448 (e4m3 max) without a clamp.  l_run accumulates the same 128 P, so O / l is
        // unchanged.
        const float m_off = 7.0f - m_run;
        float psum = 0.f;
        v8i pf;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    e[j] = __builtin_amdgcn_exp2f(fmaf(s[kb][4 * g + j], p.scale_log2, m_off));
                    psum += e[j];
                }
                pf[kb * 4 + g] = pack4_fp8(e[0], e[1], e[2], e[3]);
            }
        l_run += psum;
        // ---- O^T += VT P^T: one MFMA per 32-row d-tile
        oacc[0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(v0, pf, oacc[0], 0, 0, 0, UNIT_SCALE, 0, UNIT_SCALE);
        oacc[1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(v1, pf, oacc[1], 0, 0, 0, UNIT_SCALE, 0, UNIT_SCALE);
        if (++stage == S) stage = 0;
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;            // O' and l carry the same factor 128
    const int qi = q0 + l31;
    if (qi < p.Nq) {
        f16* O = p.o + (long)b * p.bso + (long)qi * p.ldo + (long)h * 40;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d0 = i * 32 + 8 * g + 4 * hi;
                if (d0 < 40) {
                    f16x4 w = {(f16)(oacc[i][4 * g + 0] * inv), (f16)(oacc[i][4 * g + 1] * inv),
                               (f16)(oacc[i][4 * g + 2] * inv), (f16)(oacc[i][4 * g + 3] * inv)};
                    *reinterpret_cast<f16x4*>(O + d0) = w;
                }
            }
    }
}

}  // namespace

extern "C" size_t sg_attn_f8_bytes(int32_t B, int32_t H, int32_t N, int32_t transposed) {
    const size_t np = transposed ? (size_t)((N + 63) & ~63) : (size_t)N;
    return (size_t)B * (size_t)H * 64u * np;
}

extern "C" int sg_attn_f8_pack(const sg_half* src, int64_t ld, int64_t bs, void* dst, int32_t B, int32_t H, int32_t N,
                               int32_t transposed, sg_stream_t stream) {
    SG_REQUIRE(src && dst && B > 0 && H > 0 && N > 0, "sg_attn_f8_pack: bad arguments");
    SG_REQUIRE(transposed == 0 || transposed == 1, "sg_attn_f8_pack: transposed must be 0 (Q / K rows) or 1 (V^T)");
    SG_REQUIRE(sg_aligned16(src) && sg_aligned16(dst) && ld % 8 == 0 && bs % 8 == 0, "sg_attn_f8_pack: 16-byte alignment / strides");
    SG_REQUIRE(transposed ? ld >= ((N + 7) & ~7) : ld >= (int64_t)H * 40, "sg_attn_f8_pack: row stride too small");
    PackParams p{};
    p.src = reinterpret_cast<const f16*>(src); p.ld = ld; p.bs = bs;
    p.dst = reinterpret_cast<unsigned char*>(dst);
    p.B = B; p.H = H; p.N = N; p.Nkp = (N + 63) & ~63; p.mode = transposed;
    const long items = transposed ? (long)B * H * 64 * (p.Nkp / 16) : (long)B * H * N * 4;
    hipLaunchKernelGGL(attn_f8_pack_kernel, dim3((int)min((long)8192, (items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    SG_CHECK_LAUNCH("sg_attn_f8_pack");
    return SG_OK;
}

// The launch shape of sg_attn_fwd_f8_d40: 4 waves where that still gives the chip >= 2 workgroups per CU, else 2; both on a 3-deep ring.
static int attn_f8_plan(int32_t B, int32_t H, int32_t Nq, sg_attn_plan& pl, const char* who) {
    SG_REQUIRE(B > 0 && H > 0 && Nq > 0, "%s: bad arguments", who);
    const int waves = (int64_t)sg_cdiv(Nq, 128) * H * B >= 512 ? 4 : 2;
    const int64_t wgs = (int64_t)sg_cdiv(Nq, 32 * waves) * H * B;
    SG_REQUIRE(wgs < (1ll << 31), "%s: %lld workgroups do not fit a grid", who, (long long)wgs);
    pl.family = SG_ATTN_F8; pl.waves = waves; pl.stages = 3; pl.workgroups = (int32_t)wgs;
    return SG_OK;
}

extern "C" int sg_attn_fwd_f8_plan(int32_t B, int32_t H, int32_t Nq, sg_attn_plan* out) {
    SG_REQUIRE(out != nullptr, "sg_attn_fwd_f8_plan: null plan");
    return attn_f8_plan(B, H, Nq, *out, "sg_attn_fwd_f8_plan");
}

// 32-bit arithmetic of attn_fwd_f8_kernel / attn_f8_pack_kernel: key and query indices rounded up to a tile (tile * 64 + row, (tile + 1) * 64,
// (qb NW + wave) * 32, Nkp = Nk rounded up to 64) stay below N + 128 — the check Nq, Nk <= 2^30 —, the grid is planned in 64 bits and checked
// (attn_f8_plan); every offset into an image (row * 64, row * Nkp, (b H + h) * N * 64) is computed in `long`.
extern "C" int sg_attn_fwd_f8_d40(const void* q8, const void* k8, const void* vt8, sg_half* o, int64_t ldo, int64_t bso, int32_t B,
                                  int32_t H, int32_t Nq, int32_t Nk, int32_t kv_batches, float scale, sg_stream_t stream) {
    SG_REQUIRE(q8 && k8 && vt8 && o && B > 0 && H > 0 && Nq > 0 && Nk > 0, "sg_attn_fwd_f8_d40: bad arguments");
    SG_REQUIRE(Nq <= (1 << 30) && Nk <= (1 << 30), "sg_attn_fwd_f8_d40: Nq and Nk must not exceed 2^30");
    // (the row maximum is taken of the raw scores and the key tail masked with -inf before the multiplication: see attention.hip)
    SG_REQUIRE(scale > 0.f && scale <= FLT_MAX, "sg_attn_fwd_f8_d40: scale must be finite and > 0");
    SG_REQUIRE(kv_batches >= 0 && kv_batches <= B, "sg_attn_fwd_f8_d40: kv_batches must be in [0, B]");
    SG_REQUIRE(kv_batches == 0 || 2 * (int64_t)kv_batches >= B, "sg_attn_fwd_f8_d40: kv_batches must be 0 or at least B / 2");
    SG_REQUIRE(sg_aligned16(q8) && sg_aligned16(k8) && sg_aligned16(vt8) && (reinterpret_cast<uintptr_t>(o) & 7u) == 0 && ldo % 4 == 0 &&
               bso % 4 == 0 && ldo >= (int64_t)H * 40, "sg_attn_fwd_f8_d40: alignment / strides");
    sg_attn_plan pl;
    if (int rc = attn_f8_plan(B, H, Nq, pl, "sg_attn_fwd_f8_d40")) return rc;
    F8Params p{};
    p.q8 = reinterpret_cast<const unsigned char*>(q8);
    p.k8 = reinterpret_cast<const unsigned char*>(k8);
    p.vt8 = reinterpret_cast<const unsigned char*>(vt8);
    p.o = reinterpret_cast<f16*>(o); p.ldo = ldo; p.bso = bso;
    p.B = B; p.H = H; p.Nq = Nq; p.Nk = Nk; p.Nkp = (Nk + 63) & ~63;
    p.kv_batches = kv_batches > 0 ? kv_batches : B;
    p.scale_log2 = scale * 1.44269504088896340736f;
    p.nqb = sg_cdiv(Nq, 32 * pl.waves);
    if (pl.waves == 4) hipLaunchKernelGGL((attn_fwd_f8_kernel<4, 3>), dim3(pl.workgroups), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((attn_fwd_f8_kernel<2, 3>), dim3(pl.workgroups), dim3(128), 0, (hipStream_t)stream, p);
    SG_CHECK_LAUNCH("sg_attn_fwd_f8_d40");
    return SG_OK;
}
