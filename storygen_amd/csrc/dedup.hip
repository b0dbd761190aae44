// Near-duplicate keyframe removal (data_process/dup_remove.py:21-46): the cosine similarity of every frame feature with the one before it
// and the script's decision on each pair, in one launch.  The arithmetic is written out in include/storygen_hip.h.
#include "common.h"

namespace {

constexpr int DEDUP_THREADS = 256, DEDUP_WAVES = DEDUP_THREADS / 64;
static_assert(SG_DEDUP_MAX_FRAMES / DEDUP_WAVES < (1 << 30), "the grid fits an int");

// A fixed butterfly: lane l adds what lane l ^ o holds, o = 32 .. 1; every lane ends with the same sum, whatever the inputs' order in time.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per frame i, DEDUP_WAVES frames per workgroup; lanes stride over dim.  VEC: rows are 16-byte aligned (base and ldf), a lane
// takes four consecutive floats per step and adds them in index order; the up to three last columns go to lanes 0 .. 2 one by one.
// The product of two fp32 values is exact in float64, so every rounding of the three sums is one of the float64 additions.
// Lane 0 writes sim[i], drop[i - 1] (i >= 1) and, for the last frame, drop[i] = 0: each element once, nothing else.
template <bool VEC>
__global__ __launch_bounds__(DEDUP_THREADS) void adjacent_cosine_kernel(const float* feats, long ldf, int N, int dim, double eps, double threshold,
                                                                        double* sim, uint8_t* drop) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * DEDUP_WAVES + wave;
    if (i >= N) return;                                              // wave-uniform: whole waves leave
    double s = 0.0;                                                  // frame 0 meets the script's zero feature: exactly 0
    if (i > 0) {
        const float* f = feats + i * ldf;
        const float* g = f - ldf;
        double dot = 0.0, nf = 0.0, ng = 0.0;
        int k0 = 0;
        if (VEC) {
            const int dim4 = dim & ~3;
            for (int k = lane * 4; k < dim4; k += 256) {
                const float4 a = *reinterpret_cast<const float4*>(f + k), b = *reinterpret_cast<const float4*>(g + k);
                const double a0 = a.x, a1 = a.y, a2 = a.z, a3 = a.w, b0 = b.x, b1 = b.y, b2 = b.z, b3 = b.w;
                dot += a0 * b0; dot += a1 * b1; dot += a2 * b2; dot += a3 * b3;
                nf += a0 * a0; nf += a1 * a1; nf += a2 * a2; nf += a3 * a3;
                ng += b0 * b0; ng += b1 * b1; ng += b2 * b2; ng += b3 * b3;
            }
            k0 = dim4;
        }
        for (int k = k0 + lane; k < dim; k += 64) {
            const double a = (double)f[k], b = (double)g[k];
            dot += a * b;
            nf += a * a;
            ng += b * b;
        }
        dot = wave_sum_f64(dot);
        nf = wave_sum_f64(nf);
        ng = wave_sum_f64(ng);
        // torch.cosine_similarity's clamp of each norm; fmax returns eps for a NaN norm, and dot is NaN there, so s stays NaN
        s = dot / (fmax(sqrt(nf), eps) * fmax(sqrt(ng), eps));
    }
    if (lane == 0) {
        sim[i] = s;
        if (i > 0) drop[i - 1] = s >= threshold ? 1 : 0;             // false for NaN: the frame is kept
        if (i == N - 1) drop[i] = 0;
    }
}

}  // namespace

extern "C" int sg_adjacent_cosine_f64(const float* feats, int64_t ldf, int32_t N, int32_t dim, double eps, double threshold, double* sim,
                                      uint8_t* drop, sg_stream_t stream) {
    SG_REQUIRE(feats && sim && drop, "sg_adjacent_cosine: null pointer");
    SG_REQUIRE(N >= 1 && N <= SG_DEDUP_MAX_FRAMES, "sg_adjacent_cosine: N = %d is outside [1, %d]", N, SG_DEDUP_MAX_FRAMES);
    SG_REQUIRE(dim >= 1 && dim <= SG_DEDUP_MAX_DIM, "sg_adjacent_cosine: dim = %d is outside [1, %d]", dim, SG_DEDUP_MAX_DIM);
    SG_REQUIRE(ldf >= dim, "sg_adjacent_cosine: feature row stride %lld below dim %d", (long long)ldf, dim);
    SG_REQUIRE(ldf <= ((int64_t)1 << 40), "sg_adjacent_cosine: feature row stride %lld exceeds 2^40", (long long)ldf);
    SG_REQUIRE(eps >= 0.0, "sg_adjacent_cosine: eps = %g must be a number >= 0", eps);                 // (false for NaN)
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(sim), d0 = reinterpret_cast<uintptr_t>(drop);
    SG_REQUIRE(s0 + (uintptr_t)N * sizeof(double) <= d0 || d0 + (uintptr_t)N <= s0, "sg_adjacent_cosine: sim and drop overlap");
    const dim3 grid((unsigned)sg_cdiv(N, DEDUP_WAVES)), block(DEDUP_THREADS);
    if (sg_aligned16(feats) && ldf % 4 == 0)
        hipLaunchKernelGGL(adjacent_cosine_kernel<true>, grid, block, 0, (hipStream_t)stream, feats, (long)ldf, N, dim, eps, threshold, sim, drop);
    else
        hipLaunchKernelGGL(adjacent_cosine_kernel<false>, grid, block, 0, (hipStream_t)stream, feats, (long)ldf, N, dim, eps, threshold, sim, drop);
    SG_CHECK_LAUNCH("sg_adjacent_cosine_f64");
    return SG_OK;
}
