// Frame / narration alignment (data_process/align.py): the cost matrix of cosine distance plus time penalty, and dynamic time warping
// with its backtrace, each in one launch.  The arithmetic is written out in include/storygen_hip.h.
#include "common.h"

namespace {

constexpr int COST_THREADS = 256, COST_WAVES = COST_THREADS / 64;
constexpr int COST_TILE = 16;                          // sentences per workgroup: COST_TILE / COST_WAVES per wave

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One workgroup: frame row i x COST_TILE consecutive sentences; one wave per (i, j), lanes stride over dim.  The product of two fp32
// values is exact in float64, so every rounding is one of the float64 additions (63 lane-local chains, then the butterfly).
__global__ __launch_bounds__(COST_THREADS) void align_cost_kernel(const float* frames, long ldf, const float* sents, const double* ft,
                                                                  const double* st, double* cost, long ldo, int r, int c, int dim, int jtiles) {
    const int i = blockIdx.x / jtiles, j0 = (blockIdx.x % jtiles) * COST_TILE;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* f = frames + i * ldf;
    double nf = 0.0;
    for (int k = lane; k < dim; k += 64) {
        const double a = (double)f[k];
        nf += a * a;
    }
    nf = wave_sum_f64(nf);
    const double tf = ft[i];
    for (int j = j0 + wave; j < min(j0 + COST_TILE, c); j += COST_WAVES) {
        const float* s = sents + (long)j * dim;
        double dot = 0.0, ns = 0.0;
        for (int k = lane; k < dim; k += 64) {
            const double a = (double)f[k], b = (double)s[k];
            dot += a * b;
            ns += b * b;
        }
        dot = wave_sum_f64(dot);
        ns = wave_sum_f64(ns);
        if (lane == 0) {
            const double cd = 1.0 - dot / (sqrt(nf) * sqrt(ns) + 1e-9);
            const double dt = fabs(tf - st[j]);
            cost[i * ldo + j] = dt <= 60.0 ? cd : floor(dt / 60.0) + cd;
        }
    }
}

constexpr int DTW_THREADS = SG_DTW_THREADS, DTW_SHORT = SG_DTW_MAX_SHORT, DTW_PER_THREAD = DTW_SHORT / DTW_THREADS;
constexpr int DTW_WORDS = (SG_DTW_MAX_SIDE + DTW_SHORT - 1 + 15) / 16;      // 16 two-bit moves per word over the longest walk
static_assert(DTW_SHORT % DTW_THREADS == 0, "cells of a diagonal per thread");
static_assert(3 * (DTW_SHORT + 1) * sizeof(double) >= 2 * DTW_WORDS * sizeof(uint32_t), "the walk reuses the diagonals' LDS");
static_assert(SG_DTW_MAX_SIDE <= 65535, "a walk position packs into two 16-bit halves");

// One workgroup.  Fill: anti-diagonal d = i + j holds the cells i in [max(0, d - (c - 1)), min(r - 1, d)]; threads stride over them.  A cell
// is kept in LDS under its coordinate along the shorter side (+ 1, so that slot 0 stands for coordinate -1 and is never read): the
// diagonals d - 1 and d - 2 are read, d is written, three buffers in rotation, one barrier per diagonal.
// Walk: thread 0 follows the codes back from (r - 1, c - 1), packing its moves 16 to a word and noting where each word starts; then every
// thread replays one word at a time and stores its up to 16 positions, last one first, so that path[] runs from (0, 0).
__global__ __launch_bounds__(DTW_THREADS) void dtw_path_kernel(const double* cost, long ldc, int r, int c, uint8_t* codes, double* acc, long lda,
                                                               int* path, int* path_len) {
    __shared__ double ring[3][DTW_SHORT + 1];
    __shared__ int walk_len;
    const int tid = threadIdx.x;
    const bool by_j = c <= r;
    const int nd = r + c - 1;
    const double inf = __builtin_huge_val();
    double *cur = ring[0], *p1 = ring[1], *p2 = ring[2];
    for (int d = 0; d < nd; ++d) {
        const int i_lo = max(0, d - (c - 1)), n = min(r - 1, d) - i_lo + 1;
        double cst[DTW_PER_THREAD];
#pragma unroll
        for (int u = 0; u < DTW_PER_THREAD; ++u) {
            const int t = tid + u * DTW_THREADS;
            if (t < n) cst[u] = cost[(i_lo + t) * ldc + (d - i_lo - t)];
        }
#pragma unroll
        for (int u = 0; u < DTW_PER_THREAD; ++u) {
            const int t = tid + u * DTW_THREADS;
            if (t < n) {
                const int i = i_lo + t, j = d - i;
                const int slot = (by_j ? j : i) + 1;
                const double dg = (i > 0 && j > 0) ? p2[slot - 1] : ((i | j) == 0 ? 0.0 : inf);
                const double up = i > 0 ? p1[by_j ? slot : slot - 1] : inf;
                const double lf = j > 0 ? p1[by_j ? slot - 1 : slot] : inf;
                double m = dg;                                       // first minimum wins: diagonal, up, left
                int code = 0;
                if (up < m) { m = up; code = 1; }
                if (lf < m) { m = lf; code = 2; }
                if (i == 0) code = j > 0 ? 2 : 0;                    // the borders leave one way, whatever the values say
                else if (j == 0) code = 1;
                const double a = cst[u] + m;
                cur[slot] = a;
                codes[(long)i * c + j] = (uint8_t)code;
                if (acc) acc[i * lda + j] = a;
            }
        }
        __syncthreads();
        double* t3 = p2;
        p2 = p1;
        p1 = cur;
        cur = t3;
    }
    // The barrier that ended the last diagonal (__syncthreads(): a workgroup-scope release / acquire that covers global memory too) makes
    // every code visible to thread 0.  That is all the walk needs BECAUSE the launch is one workgroup and a workgroup lives on one CU,
    // behind one vector L1 (the library builds no threadgroup-split code objects); another workgroup would need agent scope.
    // It also frees the diagonals' LDS, reused below as uint32 words (sized by the static_assert above).
    uint32_t* moves = reinterpret_cast<uint32_t*>(&ring[0][0]);
    uint32_t* starts = moves + DTW_WORDS;
    if (tid == 0) {
        int i = r - 1, j = c - 1, k = 0;                             // k moves made: the walk stands on its entry k
        uint32_t w = 0;
        starts[0] = ((uint32_t)i << 16) | (uint32_t)j;
        while ((i > 0 || j > 0) && k < nd - 1) {
            const int mv = i == 0 ? 2 : (j == 0 ? 1 : min((int)codes[(long)i * c + j], 2));
            if (mv == 0) { --i; --j; }
            else if (mv == 1) --i;
            else --j;
            w |= (uint32_t)mv << (2 * (k & 15));
            ++k;
            if ((k & 15) == 0) {
                moves[(k >> 4) - 1] = w;
                w = 0;
                starts[k >> 4] = ((uint32_t)i << 16) | (uint32_t)j;
            }
        }
        moves[k >> 4] = w;
        walk_len = k + 1;
        path_len[0] = k + 1;
    }
    __syncthreads();
    const int L = walk_len;
    for (int wd = tid; wd * 16 < L; wd += DTW_THREADS) {
        const uint32_t s = starts[wd];
        uint32_t w = moves[wd];
        int i = (int)(s >> 16), j = (int)(s & 0xFFFFu);
        for (int e = wd * 16; e < min(wd * 16 + 16, L); ++e, w >>= 2) {
            path[2 * (L - 1 - e)] = i;
            path[2 * (L - 1 - e) + 1] = j;
            const int mv = (int)(w & 3u);
            if (mv == 0) { --i; --j; }
            else if (mv == 1) --i;
            else --j;
        }
    }
}

static int check_sides(const char* who, int32_t r, int32_t c) {
    SG_REQUIRE(r >= 1 && c >= 1, "%s: r = %d, c = %d (both at least 1)", who, r, c);
    SG_REQUIRE(r <= SG_DTW_MAX_SIDE && c <= SG_DTW_MAX_SIDE, "%s: r = %d, c = %d exceed %d", who, r, c, SG_DTW_MAX_SIDE);
    SG_REQUIRE((int64_t)r * c < ((int64_t)1 << 31), "%s: r * c = %lld is not below 2^31", who, (long long)r * c);
    return SG_OK;
}

}  // namespace

extern "C" int sg_align_cost_f64(const float* frames, int64_t ldf, const float* sents, const double* frame_times, const double* sent_times,
                                 double* cost, int64_t ldo, int32_t r, int32_t c, int32_t dim, sg_stream_t stream) {
    SG_REQUIRE(frames && sents && frame_times && sent_times && cost, "sg_align_cost: null pointer");
    if (int e = check_sides("sg_align_cost", r, c)) return e;
    SG_REQUIRE(dim >= 1, "sg_align_cost: dim = %d (at least 1)", dim);
    SG_REQUIRE(ldf >= dim, "sg_align_cost: frame row stride %lld below dim %d", (long long)ldf, dim);
    SG_REQUIRE(ldo >= c, "sg_align_cost: cost row stride %lld below c = %d", (long long)ldo, c);
    const int jtiles = sg_cdiv(c, COST_TILE);
    hipLaunchKernelGGL(align_cost_kernel, dim3((unsigned)((int64_t)r * jtiles)), dim3(COST_THREADS), 0, (hipStream_t)stream, frames, (long)ldf, sents,
                       frame_times, sent_times, cost, (long)ldo, r, c, dim, jtiles);
    SG_CHECK_LAUNCH("sg_align_cost_f64");
    return SG_OK;
}

extern "C" int sg_dtw_path_f64(const double* cost, int64_t ldc, int32_t r, int32_t c, uint8_t* codes, double* acc, int64_t lda, int32_t* path,
                               int32_t* path_len, sg_stream_t stream) {
    SG_REQUIRE(cost && codes && path && path_len, "sg_dtw_path: null pointer");
    if (int e = check_sides("sg_dtw_path", r, c)) return e;
    SG_REQUIRE(min(r, c) <= SG_DTW_MAX_SHORT, "sg_dtw_path: the shorter side min(%d, %d) exceeds %d", r, c, SG_DTW_MAX_SHORT);
    SG_REQUIRE(ldc >= c, "sg_dtw_path: cost row stride %lld below c = %d", (long long)ldc, c);
    SG_REQUIRE(!acc || lda >= c, "sg_dtw_path: acc row stride %lld below c = %d", (long long)lda, c);
    hipLaunchKernelGGL(dtw_path_kernel, dim3(1), dim3(DTW_THREADS), 0, (hipStream_t)stream, cost, (long)ldc, r, c, codes, acc, (long)lda,
                       reinterpret_cast<int*>(path), reinterpret_cast<int*>(path_len));
    SG_CHECK_LAUNCH("sg_dtw_path_f64");
    return SG_OK;
}
