// Human and text masks from a detector's output (data_process/yolov7/human_ocr_mask.py:34-70 with utils/general.py's non_max_suppression
// and scale_coords): candidates per image, greedy NMS with the rescale to the frame, and the mask painter.  Every step is written out in
// include/storygen_hip.h.  All arithmetic is fp32, one rounding per operation: the file is built with fp contraction off and spells the
// operations whose fusion would change a decision with the __f*_rn intrinsics as well.
#include "common.h"

namespace {

constexpr int SEL_THREADS = 1024, SEL_WAVES = SEL_THREADS / 64;
constexpr int RANK_THREADS = 256;
constexpr int NMS_THREADS = 1024, NMS_WAVES = NMS_THREADS / 64;
constexpr int NMS_WORDS = (SG_DET_MAX_NMS + 63) / 64;
constexpr int PAINT_THREADS = 256;
constexpr float MAX_WH = 4096.0f;                                    // non_max_suppression's class offset

struct ClassMask { uint32_t w[SG_DET_MAX_NC / 32]; };

template <bool F16>
__device__ __forceinline__ float ld_pred(const void* p, long i) {
    return F16 ? (float)reinterpret_cast<const f16*>(p)[i] : reinterpret_cast<const float*>(p)[i];
}

// One workgroup per image walks the anchors SEL_THREADS at a time, a thread per anchor, and appends the survivors to comp[b] in anchor
// order: a ballot gives the position inside the wave, the waves' totals (LDS) the position of the wave, `run` the chunk's.  No atomics.
template <bool F16>
__global__ __launch_bounds__(SEL_THREADS) void det_candidates_kernel(const void* pred, long bsp, long ldp, int A, int nc, float conf_thres,
                                                                     ClassMask classes, int any_class, float* comp, int* ncomp) {
    __shared__ int wave_total[SEL_WAVES];
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* out = comp + (long)b * A * 6;
    int run = 0;
    for (int base = 0; base < A; base += SEL_THREADS) {
        const int a = base + threadIdx.x;
        bool keep = false;
        float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, conf = 0.f;
        int cls = 0;
        if (a < A) {
            const long row = b * bsp + a * ldp;
            const float obj = ld_pred<F16>(pred, row + 4);
            if (obj > conf_thres) {                                  // (false for NaN)
                bool nan = false;
                if (nc == 1) {
                    conf = obj;
                } else {
                    conf = __fmul_rn(ld_pred<F16>(pred, row + 5), obj);
                    nan = conf != conf;
                    for (int c = 1; c < nc; ++c) {
                        const float v = __fmul_rn(ld_pred<F16>(pred, row + 5 + c), obj);
                        nan |= v != v;                                // torch.max hands a NaN on: the anchor goes
                        if (v > conf) { conf = v; cls = c; }          // strict: the first maximum stays
                    }
                }
                keep = !nan && conf > conf_thres && (any_class || ((classes.w[cls >> 5] >> (cls & 31)) & 1u));
                if (keep) {
                    const float x = ld_pred<F16>(pred, row), y = ld_pred<F16>(pred, row + 1);
                    const float hw = __fdiv_rn(ld_pred<F16>(pred, row + 2), 2.0f), hh = __fdiv_rn(ld_pred<F16>(pred, row + 3), 2.0f);
                    x1 = __fsub_rn(x, hw); y1 = __fsub_rn(y, hh); x2 = __fadd_rn(x, hw); y2 = __fadd_rn(y, hh);
                }
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_total[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < SEL_WAVES; ++w) {
            const int t = wave_total[w];
            before += w < wave ? t : 0;
            total += t;
        }
        if (keep) {
            float* o = out + (long)(run + before + __popcll(m & ((1ull << lane) - 1ull))) * 6;
            o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2; o[4] = conf; o[5] = (float)cls;
        }
        run += total;
        __syncthreads();                                             // wave_total is rewritten by the next chunk
    }
    if (threadIdx.x == 0) ncomp[b] = run;
}

// Counting rank: survivor i goes to position #{j : conf_j > conf_i, or conf_j == conf_i and j < i}, score descending and anchor order among
// equal scores; positions at and beyond max_nms are not written.  The scores pass through LDS RANK_THREADS at a time.
__global__ __launch_bounds__(RANK_THREADS) void det_rank_kernel(const float* comp, const int* ncomp, int A, int max_nms, float* cand, int* ncand) {
    __shared__ float tile[RANK_THREADS];
    const int b = blockIdx.y, n = ncomp[b];
    if (blockIdx.x == 0 && threadIdx.x == 0) ncand[b] = n < max_nms ? n : max_nms;
    if ((int)(blockIdx.x * RANK_THREADS) >= n) return;              // uniform: whole workgroups leave
    const float* in = comp + (long)b * A * 6;
    const int i = blockIdx.x * RANK_THREADS + threadIdx.x;
    const float ci = i < n ? in[(long)i * 6 + 4] : 0.f;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += RANK_THREADS) {
        const int j = j0 + threadIdx.x;
        tile[threadIdx.x] = j < n ? in[(long)j * 6 + 4] : 0.f;
        __syncthreads();
        const int lim = n - j0 < RANK_THREADS ? n - j0 : RANK_THREADS;
        for (int k = 0; k < lim; ++k) {
            const float cj = tile[k];
            rank += (cj > ci || (cj == ci && j0 + k < i)) ? 1 : 0;
        }
        __syncthreads();
    }
    if (i < n && rank < max_nms) {
        const float* s = in + (long)i * 6;
        float* o = cand + ((long)b * max_nms + rank) * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = s[k];
    }
}

// torchvision's CPU kernel, operation by operation: std::max / std::min (a NaN on the left stays, one on the right is passed over), a
// strict comparison of the ratio (false for NaN).
__device__ __forceinline__ float tv_max(float a, float b) { return a < b ? b : a; }
__device__ __forceinline__ float tv_min(float a, float b) { return b < a ? b : a; }

// scale_coords' -= pad, /= gain, clamp, then .round(): fmaxf passes a NaN over, so a NaN coordinate ends as 0.
__device__ __forceinline__ float rescale(float v, float pad, float gain, float hi) {
    return rintf(fminf(fmaxf(__fdiv_rn(__fsub_rn(v, pad), gain), 0.0f), hi));
}

// One workgroup per image.  removed[] (LDS) holds one bit per sorted candidate.  All threads walk it together to the next candidate that
// is still in; it is kept (thread 0 writes its row), then every wave sweeps whole 64-bit words of later candidates, a lane per candidate,
// and lane 0 stores the word with the ballot of the suppressed ones: a word has one writer.  The walk ends after max_det kept boxes.
__global__ __launch_bounds__(NMS_THREADS) void det_nms_kernel(const float* cand, const int* ncand, int max_nms, float iou_thres, int agnostic,
                                                              int max_det, const float* geom, float* det, int* count) {
    __shared__ unsigned long long removed[NMS_WORDS];
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int n = ncand[b];
    n = n < 0 ? 0 : (n > max_nms ? max_nms : n);
    const int nwords = (n + 63) >> 6;
    const float* in = cand + (long)b * max_nms * 6;
    const float pad_x = geom[b * 5], pad_y = geom[b * 5 + 1], gain = geom[b * 5 + 2], w0 = geom[b * 5 + 3], h0 = geom[b * 5 + 4];
    for (int w = threadIdx.x; w < nwords; w += NMS_THREADS)
        removed[w] = (w == nwords - 1 && (n & 63)) ? ~0ull << (n & 63) : 0ull;       // the bits past n are out from the start
    __syncthreads();
    int kept = 0, i = 0;
    while (kept < max_det) {
        int found = -1;
        for (int w = i >> 6; w < nwords; ++w) {
            const unsigned long long in_bits = ~removed[w] & (w == (i >> 6) ? ~0ull << (i & 63) : ~0ull);
            if (in_bits) { found = (w << 6) + __ffsll((long long)in_bits) - 1; break; }
        }
        if (found < 0) break;
        i = found;
        __syncthreads();                                             // everyone has read the words before the sweep rewrites them
        const float* bi = in + (long)i * 6;
        const float rx1 = bi[0], ry1 = bi[1], rx2 = bi[2], ry2 = bi[3], cls_i = bi[5];
        if (threadIdx.x == 0) {
            float* o = det + ((long)b * max_det + kept) * 6;
            o[0] = rescale(rx1, pad_x, gain, w0); o[1] = rescale(ry1, pad_y, gain, h0);
            o[2] = rescale(rx2, pad_x, gain, w0); o[3] = rescale(ry2, pad_y, gain, h0);
            o[4] = bi[4]; o[5] = cls_i;
        }
        const float oi = agnostic ? 0.0f : __fmul_rn(cls_i, MAX_WH);
        const float ix1 = agnostic ? rx1 : __fadd_rn(rx1, oi), iy1 = agnostic ? ry1 : __fadd_rn(ry1, oi);
        const float ix2 = agnostic ? rx2 : __fadd_rn(rx2, oi), iy2 = agnostic ? ry2 : __fadd_rn(ry2, oi);
        const float iarea = __fmul_rn(__fsub_rn(ix2, ix1), __fsub_rn(iy2, iy1));
        for (int w = (i >> 6) + wave; w < nwords; w += NMS_WAVES) {
            const unsigned long long word = removed[w];
            const int j = (w << 6) + lane;
            bool sup = false;
            if (j > i && j < n && !((word >> lane) & 1ull)) {
                const float* bj = in + (long)j * 6;
                const float oj = agnostic ? 0.0f : __fmul_rn(bj[5], MAX_WH);
                const float jx1 = agnostic ? bj[0] : __fadd_rn(bj[0], oj), jy1 = agnostic ? bj[1] : __fadd_rn(bj[1], oj);
                const float jx2 = agnostic ? bj[2] : __fadd_rn(bj[2], oj), jy2 = agnostic ? bj[3] : __fadd_rn(bj[3], oj);
                const float jarea = __fmul_rn(__fsub_rn(jx2, jx1), __fsub_rn(jy2, jy1));
                const float xx1 = tv_max(ix1, jx1), yy1 = tv_max(iy1, jy1), xx2 = tv_min(ix2, jx2), yy2 = tv_min(iy2, jy2);
                const float iw = tv_max(0.0f, __fsub_rn(xx2, xx1)), ih = tv_max(0.0f, __fsub_rn(yy2, yy1));
                const float inter = __fmul_rn(iw, ih);
                sup = __fdiv_rn(inter, __fsub_rn(__fadd_rn(iarea, jarea), inter)) > iou_thres;
            }
            const unsigned long long m = __ballot(sup);
            if (lane == 0 && m) removed[w] = word | m;
        }
        __syncthreads();
        ++kept;
        ++i;
    }
    if (threadIdx.x == 0) count[b] = kept;
}

// mask[y1:y2, x1:x2] as NumPy reads the two ends of a slice over `size` elements: a negative end wraps once, then both are clamped.
__device__ __forceinline__ int slice_end(int v, int size) {
    if (v < 0) v += size;
    return v < 0 ? 0 : (v > size ? size : v);
}
__device__ __forceinline__ int det_int(float v) {                    // int() of a rounded coordinate; a NaN counts as 0
    return v != v ? 0 : (int)fminf(fmaxf(v, -1073741824.0f), 1073741824.0f);
}

// One workgroup per row y.  The rectangles that cover the row are gathered in LDS as [x1, x2) pairs, the persons' first; then a thread
// takes 16 bytes of the row (VEC: one store) or one pixel (three byte stores).  Pixels under a person rectangle are counted where their
// first byte lies; one integer atomic per workgroup adds the row's count to *covered.
template <bool VEC>
__global__ __launch_bounds__(PAINT_THREADS) void box_mask_kernel(uint8_t* mask, long ldm, int h0, int w0, const float* det, const int* count,
                                                                 int max_det, const int* text, int n_text, int* covered) {
    __shared__ int2 persons[SG_DET_MAX_DET], texts[SG_MASK_MAX_TEXT];
    __shared__ int n_persons, n_texts, row_count;
    const int y = blockIdx.x;
    if (threadIdx.x == 0) { n_persons = 0; n_texts = 0; row_count = 0; }
    __syncthreads();
    int nd = det ? *count : 0;
    nd = nd < 0 ? 0 : (nd > max_det ? max_det : nd);
    for (int r = threadIdx.x; r < nd + n_text; r += PAINT_THREADS) {
        int x1, y1, x2, y2;
        if (r < nd) {
            const float* d = det + (long)r * 6;
            x1 = det_int(d[0]); y1 = det_int(d[1]); x2 = det_int(d[2]); y2 = det_int(d[3]);
        } else {
            const int* t = text + (long)(r - nd) * 4;
            x1 = t[0]; y1 = t[1]; x2 = t[2]; y2 = t[3];
        }
        x1 = slice_end(x1, w0); x2 = slice_end(x2, w0); y1 = slice_end(y1, h0); y2 = slice_end(y2, h0);
        if (y1 <= y && y < y2 && x1 < x2) {
            if (r < nd) persons[atomicAdd(&n_persons, 1)] = make_int2(x1, x2);
            else texts[atomicAdd(&n_texts, 1)] = make_int2(x1, x2);
        }
    }
    __syncthreads();
    const int np = n_persons, nt = n_texts;
    uint8_t* row = mask + y * ldm;
    int mine = 0;
    auto pixel = [&](int x, bool& person) -> bool {
        person = false;
        for (int k = 0; k < np; ++k) person |= persons[k].x <= x && x < persons[k].y;
        bool on = person;
        for (int k = 0; k < nt && !on; ++k) on = texts[k].x <= x && x < texts[k].y;
        return on;
    };
    if (VEC) {
        const int nbytes = 3 * w0;
        for (int c0 = threadIdx.x * 16; c0 < nbytes; c0 += PAINT_THREADS * 16) {
            unsigned long long lo = 0ull, hi = 0ull;                 // bytes 0 .. 7 and 8 .. 15 of the chunk
            const int xa = c0 / 3, c1 = (c0 + 16 < nbytes ? c0 + 16 : nbytes), xb = (c1 - 1) / 3;
            for (int x = xa; x <= xb; ++x) {
                bool person;
                const bool on = pixel(x, person);
                if (person && 3 * x >= c0) ++mine;
                if (on)
                    for (int c = 3 * x; c < 3 * x + 3; ++c) {
                        const int k = c - c0;
                        if (k >= 0 && k < 8) lo |= 0xFFull << (k * 8);
                        else if (k >= 8 && k < 16) hi |= 0xFFull << ((k - 8) * 8);
                    }
            }
            if (c1 - c0 == 16) {
                stg16(row + c0, make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)));
            } else {
                for (int c = c0; c < c1; ++c) {
                    const int k = c - c0;
                    row[c] = (uint8_t)(k < 8 ? lo >> (k * 8) : hi >> ((k - 8) * 8));
                }
            }
        }
    } else {
        for (int x = threadIdx.x; x < w0; x += PAINT_THREADS) {
            bool person;
            const uint8_t v = pixel(x, person) ? 255 : 0;
            mine += person ? 1 : 0;
            row[3 * x] = v; row[3 * x + 1] = v; row[3 * x + 2] = v;
        }
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&row_count, mine);
    __syncthreads();
    if (threadIdx.x == 0 && row_count) atomicAdd(covered, row_count);
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" size_t sg_det_select_workspace_bytes(int32_t B, int32_t A) {
    if (B < 1 || B > SG_DET_MAX_BATCH || A < 1 || A > SG_DET_MAX_ANCHORS) return 0;
    return (size_t)B * A * 6 * sizeof(float) + (size_t)B * sizeof(int32_t);
}

extern "C" int sg_det_select(const void* pred, int32_t pred_f16, int64_t bsp, int64_t ldp, int32_t B, int32_t A, int32_t nc, float conf_thres,
                             const int32_t* classes, int32_t n_classes, int32_t max_nms, float* cand, int32_t* ncand, void* workspace,
                             size_t workspace_bytes, sg_stream_t stream) {
    SG_REQUIRE(pred && cand && ncand && workspace, "sg_det_select: null pointer");
    SG_REQUIRE(pred_f16 == 0 || pred_f16 == 1, "sg_det_select: pred_f16 = %d is neither 0 nor 1", pred_f16);
    SG_REQUIRE(B >= 1 && B <= SG_DET_MAX_BATCH, "sg_det_select: B = %d is outside [1, %d]", B, SG_DET_MAX_BATCH);
    SG_REQUIRE(A >= 1 && A <= SG_DET_MAX_ANCHORS, "sg_det_select: A = %d is outside [1, %d]", A, SG_DET_MAX_ANCHORS);
    SG_REQUIRE(nc >= 1 && nc <= SG_DET_MAX_NC, "sg_det_select: nc = %d is outside [1, %d]", nc, SG_DET_MAX_NC);
    SG_REQUIRE(max_nms >= 1 && max_nms <= SG_DET_MAX_NMS, "sg_det_select: max_nms = %d is outside [1, %d]", max_nms, SG_DET_MAX_NMS);
    SG_REQUIRE(ldp >= 5 + nc && ldp <= ((int64_t)1 << 32), "sg_det_select: row stride %lld is outside [5 + nc = %d, 2^32]", (long long)ldp, 5 + nc);
    SG_REQUIRE(bsp >= (int64_t)A * ldp && bsp <= ((int64_t)1 << 52), "sg_det_select: batch stride %lld is below A * row stride or beyond 2^52", (long long)bsp);
    SG_REQUIRE(conf_thres == conf_thres, "sg_det_select: conf_thres is NaN");
    SG_REQUIRE(n_classes >= 0 && n_classes <= SG_DET_MAX_NC && (n_classes == 0 || classes), "sg_det_select: %d classes without a list, or more than %d",
               n_classes, SG_DET_MAX_NC);
    ClassMask cm = {};
    for (int k = 0; k < n_classes; ++k) {
        SG_REQUIRE(classes[k] >= 0, "sg_det_select: class %d is negative", classes[k]);
        if (classes[k] < SG_DET_MAX_NC) cm.w[classes[k] >> 5] |= 1u << (classes[k] & 31);       // (a class beyond nc matches nothing)
    }
    SG_REQUIRE(workspace_bytes >= sg_det_select_workspace_bytes(B, A), "sg_det_select: workspace of %zu bytes, %zu needed", workspace_bytes,
               sg_det_select_workspace_bytes(B, A));
    SG_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, "sg_det_select: workspace must be 4-byte aligned");
    const size_t cand_bytes = (size_t)B * max_nms * 6 * sizeof(float), nc_bytes = (size_t)B * sizeof(int32_t);
    SG_REQUIRE(!overlap(cand, cand_bytes, ncand, nc_bytes) && !overlap(cand, cand_bytes, workspace, workspace_bytes) &&
               !overlap(ncand, nc_bytes, workspace, workspace_bytes), "sg_det_select: cand, ncand and workspace overlap");
    float* comp = reinterpret_cast<float*>(workspace);
    int* ncomp = reinterpret_cast<int*>(comp + (size_t)B * A * 6);
    if (pred_f16)
        hipLaunchKernelGGL(det_candidates_kernel<true>, dim3(B), dim3(SEL_THREADS), 0, (hipStream_t)stream, pred, (long)bsp, (long)ldp, A, nc,
                           conf_thres, cm, n_classes == 0 ? 1 : 0, comp, ncomp);
    else
        hipLaunchKernelGGL(det_candidates_kernel<false>, dim3(B), dim3(SEL_THREADS), 0, (hipStream_t)stream, pred, (long)bsp, (long)ldp, A, nc,
                           conf_thres, cm, n_classes == 0 ? 1 : 0, comp, ncomp);
    SG_CHECK_LAUNCH("sg_det_select (candidates)");
    hipLaunchKernelGGL(det_rank_kernel, dim3(sg_cdiv(A, RANK_THREADS), B), dim3(RANK_THREADS), 0, (hipStream_t)stream, comp, ncomp, A, max_nms,
                       cand, ncand);
    SG_CHECK_LAUNCH("sg_det_select (rank)");
    return SG_OK;
}

extern "C" int sg_det_nms(const float* cand, const int32_t* ncand, int32_t B, int32_t max_nms, float iou_thres, int32_t agnostic, int32_t max_det,
                          const float* geom, float* det, int32_t* count, sg_stream_t stream) {
    SG_REQUIRE(cand && ncand && geom && det && count, "sg_det_nms: null pointer");
    SG_REQUIRE(B >= 1 && B <= SG_DET_MAX_BATCH, "sg_det_nms: B = %d is outside [1, %d]", B, SG_DET_MAX_BATCH);
    SG_REQUIRE(max_nms >= 1 && max_nms <= SG_DET_MAX_NMS, "sg_det_nms: max_nms = %d is outside [1, %d]", max_nms, SG_DET_MAX_NMS);
    SG_REQUIRE(max_det >= 1 && max_det <= SG_DET_MAX_DET, "sg_det_nms: max_det = %d is outside [1, %d]", max_det, SG_DET_MAX_DET);
    SG_REQUIRE(iou_thres == iou_thres, "sg_det_nms: iou_thres is NaN");
    SG_REQUIRE(agnostic == 0 || agnostic == 1, "sg_det_nms: agnostic = %d is neither 0 nor 1", agnostic);
    SG_REQUIRE(!overlap(det, (size_t)B * max_det * 6 * sizeof(float), count, (size_t)B * sizeof(int32_t)), "sg_det_nms: det and count overlap");
    hipLaunchKernelGGL(det_nms_kernel, dim3(B), dim3(NMS_THREADS), 0, (hipStream_t)stream, cand, ncand, max_nms, iou_thres, agnostic, max_det, geom,
                       det, count);
    SG_CHECK_LAUNCH("sg_det_nms");
    return SG_OK;
}

extern "C" int sg_box_mask_u8(uint8_t* mask, int64_t ldm, int32_t h0, int32_t w0, const float* det, const int32_t* count, int32_t max_det,
                              const int32_t* text, int32_t n_text, int32_t* covered, sg_stream_t stream) {
    SG_REQUIRE(mask && covered, "sg_box_mask_u8: null pointer");
    SG_REQUIRE(h0 >= 1 && h0 <= SG_MASK_MAX_SIDE && w0 >= 1 && w0 <= SG_MASK_MAX_SIDE, "sg_box_mask_u8: a %d x %d frame is outside [1, %d] per side", h0,
               w0, SG_MASK_MAX_SIDE);
    SG_REQUIRE(ldm >= 3 * (int64_t)w0 && ldm <= ((int64_t)1 << 32), "sg_box_mask_u8: row stride %lld is outside [3 w0 = %d, 2^32]", (long long)ldm, 3 * w0);
    SG_REQUIRE((det == nullptr) == (count == nullptr), "sg_box_mask_u8: det and count go together");
    SG_REQUIRE(det ? (max_det >= 1 && max_det <= SG_DET_MAX_DET) : max_det == 0, "sg_box_mask_u8: max_det = %d is outside [1, %d] (0 without det)", max_det,
               SG_DET_MAX_DET);
    SG_REQUIRE(n_text >= 0 && n_text <= SG_MASK_MAX_TEXT && (n_text == 0 || text), "sg_box_mask_u8: %d text rectangles without a list, or more than %d",
               n_text, SG_MASK_MAX_TEXT);
    SG_REQUIRE((reinterpret_cast<uintptr_t>(covered) & 3u) == 0, "sg_box_mask_u8: covered must be 4-byte aligned");
    SG_REQUIRE(!overlap(mask, (size_t)(h0 - 1) * ldm + 3 * (size_t)w0, covered, sizeof(int32_t)), "sg_box_mask_u8: mask and covered overlap");
    if (hipMemsetAsync(covered, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return sg_set_error(SG_ELAUNCH, "sg_box_mask_u8: clearing covered failed");
    if (sg_aligned16(mask) && ldm % 16 == 0)
        hipLaunchKernelGGL(box_mask_kernel<true>, dim3(h0), dim3(PAINT_THREADS), 0, (hipStream_t)stream, mask, (long)ldm, h0, w0, det, count, max_det, text,
                           n_text, covered);
    else
        hipLaunchKernelGGL(box_mask_kernel<false>, dim3(h0), dim3(PAINT_THREADS), 0, (hipStream_t)stream, mask, (long)ldm, h0, w0, det, count, max_det,
                           text, n_text, covered);
    SG_CHECK_LAUNCH("sg_box_mask_u8");
    return SG_OK;
}
