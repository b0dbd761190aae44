// Pillow's 8-bit resampling, the pieces image.hip (sg_image_resize_u8) and clip_u8.hip (sg_clip_patchify_u8) share: the device side of one
// fixed-point tap sum and the host side of the launch geometry and the overlap checks.  Each unit gets its own copy (anonymous namespace).
#pragma once
#include "common.h"
#include <math.h>

namespace {

constexpr int PRECISION_BITS = 22;      // Pillow's: 32 - 8 - 2

struct Taps { int first, n; };
// (first sample, taps) of one output sample, forced inside the input extent and the table row whatever the table says
__device__ __forceinline__ Taps taps_of(const int32_t* bounds, int i, int in, int ks) {
    const int first = min(max(bounds[2 * i], 0), in);
    return {first, min(max(bounds[2 * i + 1], 0), min(ks, in - first))};
}
__device__ __forceinline__ int clip8(int ss) { return min(max(ss >> PRECISION_BITS, 0), 255); }

// ---------------------------------------------------------------------------------------------------------- host: the launch geometry
// operation by operation in double: a fused multiply-add would round once where the C code rounds twice
#pragma clang fp contract(off)
struct Axis { double scale, filterscale, support; int ksize; };
Axis axis_of(int in, int out) {
    Axis ax;
    ax.scale = (double)in / out;
    ax.filterscale = ax.scale < 1.0 ? 1.0 : ax.scale;
    ax.support = 2.0 * ax.filterscale;
    ax.ksize = 2 * (int)ceil(ax.support) + 1;
    return ax;
}
bool axis_admitted(int in, int out) {
    return in > 0 && out > 0 && in <= SG_IMAGE_MAX_SIDE && out <= SG_IMAGE_MAX_SIDE && (int64_t)in <= (int64_t)SG_IMAGE_MAX_RATIO * out;
}

// Input rows that th consecutive output rows read at most: last tap of the last row - first tap of the first row
// <= (c + (th - 1) scale + support + 0.5) - (c - support + 0.5 - 1).
int staged_rows(const Axis& ax, int in, int th) {
    const int bound = (int)floor((th - 1) * ax.scale + 2.0 * ax.support) + 2;
    return bound < in ? bound : in;
}
int tile_rows(int in, int out, int C) {
    if (in == out) return SG_IMAGE_TILE_H;
    const Axis ax = axis_of(in, out);
    int th = SG_IMAGE_TILE_H;
    while (th > 1 && (int64_t)staged_rows(ax, in, th) * SG_IMAGE_TILE_W * C > SG_IMAGE_LDS_BYTES) --th;
    return th;
}

struct Span { uintptr_t lo, hi; };
Span span_of(const void* p, int64_t bs, int64_t cs, int64_t ld, int N, int chans, int H, int64_t inner, int esz) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return {lo, lo + (uintptr_t)(((int64_t)(N - 1) * bs + (int64_t)(chans - 1) * cs + (int64_t)(H - 1) * ld + inner) * esz)};
}
bool overlap(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace
