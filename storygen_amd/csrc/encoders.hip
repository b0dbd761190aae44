// Small kernels of the two networks either side of the denoising loop: the CLIP text encoder
// (/root/reference/model/pipeline.py:137,183) and the AutoencoderKL (:198-205,392,401).  Their GEMMs, convolutions, GroupNorms and
// LayerNorms are the UNet's kernels (gemm_conv.hip, norm.hip); what is left is bandwidth- or latency-bound glue:
//   softmax_rows_kernel   the VAE mid-block AttentionBlock (ONE head of 512 channels: QK^T and PV are plain GEMMs, fp32 scores)
//   attn_small_kernel     CLIP's causal self-attention (77 tokens, 12 heads of 64): K/V of one (batch, head) live in LDS
//   act_rows_kernel       quick_gelu / gelu between CLIP's fc1 and fc2
//   embed_tokens_kernel   token + position embedding gather into the fp32 residual stream
//   gaussian_sample_kernel  DiagonalGaussianDistribution.sample() * scaling factor
// and the front of the CLIP image tower (CLIP-I / CLIP-T scoring of generated frames):
//   clip_patchify_kernel       antialiased bicubic resize + centre crop + normalise + patch gather, float image -> fp16 GEMM rows
//                              (optionally zero-padded to a K that is a multiple of 8: patch size 14, sg_clip_patchify_padk_f16)
//   clip_embed_patches_kernel  class token + patch rows + position embedding into the fp32 residual stream
#include "common.h"

namespace {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// p[row, j] = softmax_j(scale * s[row, j]), j < N; columns [N, Npad) are written as zeros (the PV GEMM's K dimension is Npad).
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* s, long lds, f16* p, long ldp, int N, int Npad, float scale) {
    __shared__ float red[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const float* sr = s + (long)blockIdx.x * lds;
    f16* pr = p + (long)blockIdx.x * ldp;
    float m = -INFINITY;
    for (int j = t; j < N; j += 256) m = fmaxf(m, sr[j]);
    m = wave_max(m);
    if (lane == 0) red[w] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int j = t; j < N; j += 256) sum += expf(scale * (sr[j] - m));
    sum = wave_sum(sum);
    if (lane == 0) red[w] = sum;
    __syncthreads();
    sum = (red[0] + red[1]) + (red[2] + red[3]);
    const float inv = 1.0f / sum;
    for (int j = t; j < Npad; j += 256) pr[j] = j < N ? (f16)(expf(scale * (sr[j] - m)) * inv) : (f16)0.f;
}

constexpr int AS_MAXT = 128, AS_MAXD = 64, AS_LD = AS_MAXD + 2;   // +2 halfs: a row is 33 dwords, lane-per-row reads spread over banks

constexpr int AS_ROWS = 16;     // query rows per workgroup (4 per wave): CLIP's 77 tokens x 12 heads x B spread over 60 B workgroups

// grid (heads, batches, row chunks); one wave per query row at a time, lane j owns keys j and j + 64.  A causal chunk only needs the
// keys up to its last row.
__global__ __launch_bounds__(256) void attn_small_kernel(const f16* q, long ldq, long bsq, const f16* k, long ldk, long bsk,
                                                         const f16* v, long ldv, long bsv, f16* o, long ldo, long bso,
                                                         const float* key_bias, int T, int D, float scale, int causal) {
    __shared__ f16 sK[AS_MAXT][AS_LD], sV[AS_MAXT][AS_LD];
    __shared__ float sQ[4][AS_MAXD], sP[4][AS_MAXT];
    const int h = blockIdx.x, b = blockIdx.y, r0 = blockIdx.z * AS_ROWS, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int Tk = causal ? min(T, r0 + AS_ROWS) : T;             // keys this chunk can see
    const f16* kb = k + (long)b * bsk + h * D;
    const f16* vb = v + (long)b * bsv + h * D;
    for (int idx = t; idx < Tk * D; idx += 256) {
        const int j = idx / D, d = idx - j * D;
        sK[j][d] = kb[(long)j * ldk + d];
        sV[j][d] = vb[(long)j * ldv + d];
    }
    __syncthreads();
    for (int r = 0; r < AS_ROWS / 4; ++r) {
        const int i = r0 + r * 4 + w;
        const bool live = i < T;
        if (live && lane < D) sQ[w][lane] = (float)q[(long)b * bsq + (long)i * ldq + h * D + lane] * scale;
        __syncthreads();
        float s0 = -INFINITY, s1 = -INFINITY;
        if (live) {
            const int j0 = lane, j1 = lane + 64;
            if (j0 < Tk && !(causal && j0 > i)) {
                float a = 0.f;
                for (int d = 0; d < D; ++d) a += sQ[w][d] * (float)sK[j0][d];
                s0 = a + (key_bias ? key_bias[(long)b * T + j0] : 0.f);
            }
            if (j1 < Tk && !(causal && j1 > i)) {
                float a = 0.f;
                for (int d = 0; d < D; ++d) a += sQ[w][d] * (float)sK[j1][d];
                s1 = a + (key_bias ? key_bias[(long)b * T + j1] : 0.f);
            }
        }
        const float m = wave_max(fmaxf(s0, s1));
        const float e0 = s0 == -INFINITY ? 0.f : expf(s0 - m), e1 = s1 == -INFINITY ? 0.f : expf(s1 - m);
        const float sum = wave_sum(e0 + e1);
        sP[w][lane] = e0;
        sP[w][lane + 64] = e1;
        __syncthreads();
        if (live && lane < D) {
            const int jn = causal ? min(Tk, i + 1) : Tk;
            float acc = 0.f;
            for (int j = 0; j < jn; ++j) acc += sP[w][j] * (float)sV[j][lane];
            o[(long)b * bso + (long)i * ldo + h * D + lane] = (f16)(acc / sum);
        }
        __syncthreads();
    }
}

// in place: x = x * sigmoid(1.702 x) (act 0, CLIP "quick_gelu") or the erf GELU (act 1)
__global__ __launch_bounds__(256) void act_rows_kernel(f16* x, long ldx, int M, int N, int act) {
    const int vpr = N / 8;
    const long total = (long)M * vpr;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / vpr;
        const int c = (int)(idx - r * vpr);
        f16* px = x + r * ldx + c * 8;
        H8 v; v.u = ldg16(px);
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float a = (float)v.h[j];
            o[j] = act == 0 ? a / (1.0f + expf(-1.702f * a)) : gelu_erf_f(a);
        }
        store8h(px, o);
    }
}

// out[r, :] = tok[ids[r], :] + pos[r % T, :]   (fp32 tables, fp32 residual stream)
__global__ __launch_bounds__(256) void embed_tokens_kernel(const long long* ids, const float* tok, const float* pos, float* out, long ldo,
                                                           int rows, int T, int C) {
    const int vpr = C / 4;
    const long total = (long)rows * vpr;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / vpr;
        const int c = (int)(idx - r * vpr) * 4;
        const float4 a = *reinterpret_cast<const float4*>(tok + (long)ids[r] * C + c);
        const float4 p = *reinterpret_cast<const float4*>(pos + (long)(r % T) * C + c);
        *reinterpret_cast<float4*>(out + r * ldo + c) = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
    }
}

__global__ __launch_bounds__(256) void gaussian_sample_kernel(const float* mean, const float* logvar, const float* noise, float* out,
                                                              float scale, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float v = mean[i];
        if (noise) v += expf(0.5f * fminf(fmaxf(logvar[i], -30.0f), 20.0f)) * noise[i];
        out[i] = v * scale;
    }
}

// ---- CLIP image tower front end (the `clip` package's preprocessing = torchvision Resize(S, BICUBIC) + CenterCrop(S) + Normalize, then
// the patch gather of CLIPVisionEmbeddings' stride-ps convolution), one launch.
// Keys cubic, a = -0.5
__device__ __forceinline__ float keys_cubic(float x) {
    x = fabsf(x);
    if (x < 1.0f) return ((1.5f * x - 2.5f) * x) * x + 1.0f;
    if (x < 2.0f) return (((x - 5.0f) * x + 8.0f) * x - 4.0f) * -0.5f;
    return 0.0f;
}

// Antialiased window of output index i along an axis of `in` input pixels (scale = in / out, half-pixel centres): taps [lo, lo + n) lie
// inside the image by construction (the window is truncated at the edges and the weights renormalised by their sum).
__device__ __forceinline__ void aa_window(int i, int in, float scale, int& lo, int& n, float& center, float& inv) {
    const float support = scale >= 1.0f ? 2.0f * scale : 2.0f;
    center = scale * ((float)i + 0.5f);
    inv = scale >= 1.0f ? 1.0f / scale : 1.0f;
    lo = max((int)(center - support + 0.5f), 0);
    n = max(min((int)(center + support + 0.5f), in) - lo, 0);
}

struct PatchifyArgs {
    int B, H, W, S, ps, RH, RW, top, left;      // input size, crop size, patch size, resized size, crop offset in the resized image
    float sy, sx;                               // H / RH, W / RW
    float in_scale, in_shift, mean[3], std[3];
};

// One resampled, normalised value: image b, output column col = (c * ps + dy) * ps + dx of the patch at (py, px).
__device__ __forceinline__ float patchify_value(const float* x, const PatchifyArgs& a, int b, int py, int px, int col) {
    const int c = col / (a.ps * a.ps), rem = col - c * a.ps * a.ps;
    const int dy = rem / a.ps, dx = rem - dy * a.ps;
    int ylo, ny, xlo, nx;
    float cy, iy, cx, ix;
    aa_window(a.top + py * a.ps + dy, a.H, a.sy, ylo, ny, cy, iy);
    aa_window(a.left + px * a.ps + dx, a.W, a.sx, xlo, nx, cx, ix);
    float ty = 0.f, tx = 0.f;
    for (int j = 0; j < ny; ++j) ty += keys_cubic(((float)(ylo + j) - cy + 0.5f) * iy);
    for (int k = 0; k < nx; ++k) tx += keys_cubic(((float)(xlo + k) - cx + 0.5f) * ix);
    const float* src = x + ((long)b * 3 + c) * a.H * a.W;
    float acc = 0.f;
    for (int j = 0; j < ny; ++j) {
        const float* r = src + (long)(ylo + j) * a.W + xlo;
        float s = 0.f;
        for (int k = 0; k < nx; ++k) s += keys_cubic(((float)(xlo + k) - cx + 0.5f) * ix) * r[k];
        acc += keys_cubic(((float)(ylo + j) - cy + 0.5f) * iy) * s;
    }
    const float t = ty * tx;
    if (t != 0.f) acc /= t;
    // the input affine commutes with the resampling (the normalised weights sum to one), so it is applied once here
    const float v = acc * a.in_scale + a.in_shift;
    const float m = c == 0 ? a.mean[0] : (c == 1 ? a.mean[1] : a.mean[2]);
    const float sd = c == 0 ? a.std[0] : (c == 1 ? a.std[1] : a.std[2]);
    return (v - m) / sd;
}

// One thread per 8 consecutive columns of one output row (one 16-byte store).  Row = b * P + patch (row-major patches), column =
// (c * ps + dy) * ps + dx: the layout of patch_embedding.weight.view(C, 3 * ps * ps).  The separable weights are evaluated per output
// value (<= 11 x 11 taps at 512 -> 224): no intermediate image, fp32 throughout.  Columns [3 * ps * ps, Kpad) are written as zeros (the patch GEMM's
// K dimension when 3 * ps * ps is no multiple of 8: patch size 14); sg_clip_patchify_f16 passes Kpad = 3 * ps * ps.
__global__ __launch_bounds__(256) void clip_patchify_kernel(const float* x, f16* out, long ldo, PatchifyArgs a, int Kpad) {
    const int K = 3 * a.ps * a.ps, vpr = Kpad / 8, G = a.S / a.ps, P = G * G;
    const long total = (long)a.B * P * vpr;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long row = idx / vpr;
        const int col0 = (int)(idx - row * vpr) * 8;
        const int b = (int)(row / P), p = (int)(row - (long)b * P);
        const int py = p / G, px = p - py * G;
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = col0 + e < K ? patchify_value(x, a, b, py, px, col0 + e) : 0.f;
        store8h(out + row * ldo + col0, o);
    }
}

// CLIPVisionEmbeddings: out[b*T + 0, :] = cls + pos[0], out[b*T + t, :] = patches[b*(T-1) + t-1, :] + pos[t]   (fp32)
__global__ __launch_bounds__(256) void clip_embed_patches_kernel(const float* patches, long ldp, const float* cls, const float* pos, float* out,
                                                                 long ldo, int rows, int T, int C) {
    const int vpr = C / 4;
    const long total = (long)rows * vpr;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / vpr;
        const int c = (int)(idx - r * vpr) * 4;
        const long b = r / T;
        const int t = (int)(r - b * T);
        const float4 a = *reinterpret_cast<const float4*>(t == 0 ? cls + c : patches + (b * (T - 1) + t - 1) * ldp + c);
        const float4 p = *reinterpret_cast<const float4*>(pos + (long)t * C + c);
        *reinterpret_cast<float4*>(out + r * ldo + c) = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
    }
}

}  // namespace

extern "C" int sg_softmax_rows_f16(const float* s, int64_t lds, sg_half* p, int64_t ldp, int32_t M, int32_t N, float scale,
                                   sg_stream_t stream) {
    SG_REQUIRE(s && p, "sg_softmax_rows: null pointer");
    const int Npad = (N + 7) & ~7;
    SG_REQUIRE(M > 0 && N > 0 && lds >= N && ldp >= Npad, "sg_softmax_rows: bad shape M=%d N=%d lds=%lld ldp=%lld", M, N, (long long)lds,
               (long long)ldp);
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, s, (long)lds, reinterpret_cast<f16*>(p), (long)ldp, N,
                       Npad, scale);
    SG_CHECK_LAUNCH("sg_softmax_rows_f16");
    return SG_OK;
}

extern "C" int sg_attn_small_f16(const sg_half* q, int64_t ldq, int64_t bsq, const sg_half* k, int64_t ldk, int64_t bsk, const sg_half* v,
                                 int64_t ldv, int64_t bsv, sg_half* o, int64_t ldo, int64_t bso, const float* key_bias, int32_t B,
                                 int32_t H, int32_t T, int32_t D, float scale, int32_t causal, sg_stream_t stream) {
    SG_REQUIRE(q && k && v && o, "sg_attn_small: null pointer");
    SG_REQUIRE(B > 0 && H > 0 && T > 0 && T <= AS_MAXT && D > 0 && D <= AS_MAXD, "sg_attn_small: needs T <= %d and D <= %d (got T=%d D=%d)",
               AS_MAXT, AS_MAXD, T, D);
    SG_REQUIRE(ldq >= (int64_t)H * D && ldk >= (int64_t)H * D && ldv >= (int64_t)H * D && ldo >= (int64_t)H * D, "sg_attn_small: token stride below H*D");
    SG_REQUIRE(causal == 0 || causal == 1, "sg_attn_small: causal must be 0 or 1");
    hipLaunchKernelGGL(attn_small_kernel, dim3(H, B, (T + AS_ROWS - 1) / AS_ROWS), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const f16*>(q), (long)ldq, (long)bsq,
                       reinterpret_cast<const f16*>(k), (long)ldk, (long)bsk, reinterpret_cast<const f16*>(v), (long)ldv, (long)bsv,
                       reinterpret_cast<f16*>(o), (long)ldo, (long)bso, key_bias, T, D, scale, causal);
    SG_CHECK_LAUNCH("sg_attn_small_f16");
    return SG_OK;
}

extern "C" int sg_act_rows_f16(sg_half* x, int64_t ldx, int32_t M, int32_t N, int32_t act, sg_stream_t stream) {
    SG_REQUIRE(x, "sg_act_rows: null pointer");
    SG_REQUIRE(M > 0 && N > 0 && N % 8 == 0 && ldx % 8 == 0 && ldx >= N && sg_aligned16(x), "sg_act_rows: N and ldx must be multiples of 8, x 16-byte aligned");
    SG_REQUIRE(act == SG_ACT_QUICK_GELU || act == SG_ACT_GELU, "sg_act_rows: unknown activation %d", act);
    const long total = (long)M * (N / 8);
    const int blocks = (int)(total / 256 + 1 < 65536 ? total / 256 + 1 : 65536);
    hipLaunchKernelGGL(act_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<f16*>(x), (long)ldx, M, N, act);
    SG_CHECK_LAUNCH("sg_act_rows_f16");
    return SG_OK;
}

extern "C" int sg_embed_tokens_f32(const int64_t* ids, const float* tok, const float* pos, float* out, int64_t ldo, int32_t rows, int32_t T,
                                   int32_t C, sg_stream_t stream) {
    SG_REQUIRE(ids && tok && pos && out, "sg_embed_tokens: null pointer");
    SG_REQUIRE(rows > 0 && T > 0 && C > 0 && C % 4 == 0 && ldo % 4 == 0 && ldo >= C, "sg_embed_tokens: bad shape rows=%d T=%d C=%d", rows, T, C);
    SG_REQUIRE(sg_aligned16(tok) && sg_aligned16(pos) && sg_aligned16(out), "sg_embed_tokens: 16-byte alignment");
    const long total = (long)rows * (C / 4);
    const int blocks = (int)(total / 256 + 1 < 65536 ? total / 256 + 1 : 65536);
    hipLaunchKernelGGL(embed_tokens_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const long long*>(ids), tok, pos, out,
                       (long)ldo, rows, T, C);
    SG_CHECK_LAUNCH("sg_embed_tokens_f32");
    return SG_OK;
}

extern "C" int sg_gaussian_sample_f32(const float* mean, const float* logvar, const float* noise, float* out, float scale, int64_t n,
                                      sg_stream_t stream) {
    SG_REQUIRE(mean && out && (noise == nullptr || logvar != nullptr), "sg_gaussian_sample: null pointer");
    SG_REQUIRE(n > 0, "sg_gaussian_sample: empty");
    const int blocks = (int)(n / 256 + 1 < 4096 ? n / 256 + 1 : 4096);
    hipLaunchKernelGGL(gaussian_sample_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, mean, logvar, noise, out, scale, (long)n);
    SG_CHECK_LAUNCH("sg_gaussian_sample_f32");
    return SG_OK;
}

// torchvision's Resize(S) (shorter side -> S, longer side -> int(S * long / short)) followed by CenterCrop(S) (offset
// int(round((size - S) / 2.0)), Python's round: halves go to the even integer).  geom = {resized H, resized W, top, left}.
extern "C" int sg_clip_resize_geometry(int32_t H, int32_t W, int32_t S, int32_t* geom) {
    SG_REQUIRE(geom, "sg_clip_resize_geometry: null pointer");
    SG_REQUIRE(H > 0 && W > 0 && S > 0 && H <= (1 << 15) && W <= (1 << 15) && S <= (1 << 15), "sg_clip_resize_geometry: bad size H=%d W=%d S=%d", H, W, S);
    const int shortside = W <= H ? W : H, longside = W <= H ? H : W;
    const int rl = (int)((double)((long)S * longside) / (double)shortside);
    const int RH = W <= H ? rl : S, RW = W <= H ? S : rl;
    const int dh = RH - S, dw = RW - S;
    geom[0] = RH;
    geom[1] = RW;
    geom[2] = (dh >> 1) + ((dh & 1) & (dh >> 1));      // k + 1/2 rounds to the even one of k, k + 1
    geom[3] = (dw >> 1) + ((dw & 1) & (dw >> 1));
    return SG_OK;
}

// The shared tail of the two patchify entry points: geometry, arguments, launch.  Kpad = row width written (>= 3 * ps * ps, multiple of 8).
static int clip_patchify_launch(const char* who, const float* x, int32_t B, int32_t H, int32_t W, float in_scale, float in_shift, const float* mean,
                                const float* std, int32_t S, int32_t ps, int32_t Kpad, sg_half* out, int64_t ldo, sg_stream_t stream) {
    int32_t g[4];
    if (int e = sg_clip_resize_geometry(H, W, S, g)) return e;
    PatchifyArgs a;
    a.B = B, a.H = H, a.W = W, a.S = S, a.ps = ps, a.RH = g[0], a.RW = g[1], a.top = g[2], a.left = g[3];
    a.sy = (float)H / (float)a.RH, a.sx = (float)W / (float)a.RW;
    a.in_scale = in_scale, a.in_shift = in_shift;
    for (int c = 0; c < 3; ++c) a.mean[c] = mean[c], a.std[c] = std[c];
    const long total = (long)B * (S / ps) * (S / ps) * (Kpad / 8);
    const int blocks = (int)(total / 256 + 1 < 65536 ? total / 256 + 1 : 65536);
    hipLaunchKernelGGL(clip_patchify_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, reinterpret_cast<f16*>(out), (long)ldo, a, Kpad);
    SG_CHECK_LAUNCH(who);
    return SG_OK;
}

extern "C" int sg_clip_patchify_f16(const float* x, int32_t B, int32_t H, int32_t W, float in_scale, float in_shift, const float* mean,
                                    const float* std, int32_t S, int32_t ps, sg_half* out, int64_t ldo, sg_stream_t stream) {
    SG_REQUIRE(x && mean && std && out, "sg_clip_patchify: null pointer");
    SG_REQUIRE(B > 0 && H > 0 && W > 0 && S > 0 && ps > 0 && H <= (1 << 15) && W <= (1 << 15) && S <= (1 << 15),
               "sg_clip_patchify: bad size B=%d H=%d W=%d S=%d ps=%d", B, H, W, S, ps);
    SG_REQUIRE(S % ps == 0, "sg_clip_patchify: the crop size %d is not a multiple of the patch size %d", S, ps);
    SG_REQUIRE((3 * ps * ps) % 8 == 0, "sg_clip_patchify: 3 * ps * ps (%d) must be a multiple of 8", 3 * ps * ps);
    SG_REQUIRE(ldo % 8 == 0 && ldo >= 3 * ps * ps && sg_aligned16(out), "sg_clip_patchify: output row stride / alignment");
    SG_REQUIRE(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "sg_clip_patchify: zero std");
    return clip_patchify_launch("sg_clip_patchify_f16", x, B, H, W, in_scale, in_shift, mean, std, S, ps, 3 * ps * ps, out, ldo, stream);
}

extern "C" int sg_clip_patchify_padk_f16(const float* x, int32_t B, int32_t H, int32_t W, float in_scale, float in_shift, const float* mean,
                                         const float* std, int32_t S, int32_t ps, int32_t Kpad, sg_half* out, int64_t ldo, sg_stream_t stream) {
    SG_REQUIRE(x && mean && std && out, "sg_clip_patchify_padk: null pointer");
    SG_REQUIRE(B > 0 && H > 0 && W > 0 && S > 0 && ps > 0 && ps <= 256 && H <= (1 << 15) && W <= (1 << 15) && S <= (1 << 15),
               "sg_clip_patchify_padk: bad size B=%d H=%d W=%d S=%d ps=%d", B, H, W, S, ps);
    SG_REQUIRE(S % ps == 0, "sg_clip_patchify_padk: the crop size %d is not a multiple of the patch size %d", S, ps);
    SG_REQUIRE((3 * ps * ps) % 4 == 0, "sg_clip_patchify_padk: 3 * ps * ps (%d) must be a multiple of 4", 3 * ps * ps);
    SG_REQUIRE(Kpad % 8 == 0 && Kpad >= 3 * ps * ps, "sg_clip_patchify_padk: Kpad (%d) must be a multiple of 8 and at least 3 * ps * ps (%d)", Kpad,
               3 * ps * ps);
    SG_REQUIRE(ldo % 8 == 0 && ldo >= Kpad && sg_aligned16(out), "sg_clip_patchify_padk: output row stride %lld below Kpad %d / alignment",
               (long long)ldo, Kpad);
    SG_REQUIRE(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "sg_clip_patchify_padk: zero std");
    return clip_patchify_launch("sg_clip_patchify_padk_f16", x, B, H, W, in_scale, in_shift, mean, std, S, ps, Kpad, out, ldo, stream);
}

extern "C" int sg_clip_embed_patches_f32(const float* patches, int64_t ldp, const float* cls, const float* pos, float* out, int64_t ldo,
                                         int32_t B, int32_t T, int32_t C, sg_stream_t stream) {
    SG_REQUIRE(patches && cls && pos && out, "sg_clip_embed_patches: null pointer");
    SG_REQUIRE(B > 0 && T > 1 && C > 0 && C % 4 == 0 && ldp % 4 == 0 && ldp >= C && ldo % 4 == 0 && ldo >= C,
               "sg_clip_embed_patches: bad shape B=%d T=%d C=%d", B, T, C);
    SG_REQUIRE(sg_aligned16(patches) && sg_aligned16(cls) && sg_aligned16(pos) && sg_aligned16(out), "sg_clip_embed_patches: 16-byte alignment");
    const long total = (long)B * T * (C / 4);
    const int blocks = (int)(total / 256 + 1 < 65536 ? total / 256 + 1 : 65536);
    hipLaunchKernelGGL(clip_embed_patches_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, patches, (long)ldp, cls, pos, out, (long)ldo,
                       B * T, T, C);
    SG_CHECK_LAUNCH("sg_clip_embed_patches_f32");
    return SG_OK;
}
