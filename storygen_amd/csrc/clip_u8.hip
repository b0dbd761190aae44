// CLIP preprocessing of 8-bit frames as the reference's evaluation scripts run it: Pillow's bicubic Image.resize (image_resample.h), the
// centre crop, ToTensor + Normalize and the patch rows of the patch GEMM, in one launch.
#include "image_resample.h"

namespace {

constexpr int LUT_BYTES = 3 * 256 * (int)sizeof(f16);      // the 768 normalised values, ahead of the staged image in LDS

struct PatchU8Args {
    const uint8_t* x; long bsx, ldx;                      // uint8 [N,Hin,Win,3]
    f16* out; long ldo;                                   // fp16 [N * P, >= Kpad]
    uint8_t* u8; long bsu, ldu;                           // uint8 [N,S,S,3] or null
    const int32_t *hcoef, *hbounds, *vcoef, *vbounds;     // null for a skipped pass
    int Hin, Win, top, left, S, ps, Kpad, hks, vks, th, lds_rows;
    float mean[3], std[3];
};

// A workgroup (4 waves) owns th rows x SG_IMAGE_TILE_W columns of the S x S crop window of one resized image, the scheme of
// image_resize_kernel: the horizontal pass of the input rows [lo, lo + rows) that the tile's vertical taps read goes to LDS as uint8 (what
// Pillow's intermediate image holds), the vertical pass reads it from there; one pass alone reads global memory.  Every byte then becomes
// one fp16 of its patch row through a table of the 768 (channel, byte) results; lanes walk a row channel by channel, so neighbouring
// lanes store neighbouring columns of a patch row.  The patch whose top-left pixel a thread holds gets its zero columns from that thread.
__global__ __launch_bounds__(256) void clip_patchify_u8_kernel(const PatchU8Args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    f16* lut = reinterpret_cast<f16*>(lds);
    uint8_t* img = lds + LUT_BYTES;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * SG_IMAGE_TILE_W, tw = min(SG_IMAGE_TILE_W, a.S - x0), rowe = tw * 3;
    const int y0 = blockIdx.y * a.th, trows = min(a.th, a.S - y0);
    const int c0 = (a.left + x0) * 3;                     // byte of the tile's first column in a row of the resized image
    const uint8_t* src = a.x + blockIdx.z * a.bsx;

    // ToTensor, then Normalize: three fp32 roundings (contraction is off in this unit), then the cast to fp16
#pragma unroll
    for (int c = 0; c < 3; ++c) lut[c * 256 + threadIdx.x] = (f16)(((float)threadIdx.x / 255.0f - a.mean[c]) / a.std[c]);

    // byte e of the tile's columns in input row `row` after the horizontal pass
    auto hpass = [&](int row, int e) -> int {
        const uint8_t* p = src + row * a.ldx;
        if (!a.hcoef) return p[c0 + e];
        const int col = a.left + x0 + e / 3, ch = e % 3;
        const Taps t = taps_of(a.hbounds, col, a.Win, a.hks);
        const int32_t* k = a.hcoef + (long)col * a.hks;
        p += t.first * 3 + ch;
        int ss = 1 << (PRECISION_BITS - 1);
        for (int i = 0; i < t.n; ++i) ss += (int)p[i * 3] * k[i];
        return clip8(ss);
    };

    const bool staged = a.hcoef && a.vcoef;
    int lo = 0, rows = a.Hin;
    if (staged) {       // the input rows this tile's vertical taps read, cut to what the LDS image holds
        int hi = 0;
        lo = a.Hin;
        for (int r = 0; r < trows; ++r) {
            const Taps t = taps_of(a.vbounds, a.top + y0 + r, a.Hin, a.vks);
            lo = min(lo, t.first);
            hi = max(hi, t.first + t.n);
        }
        rows = min(max(hi - lo, 0), a.lds_rows);
        for (int r = wave; r < rows; r += 4)
            for (int e = lane; e < rowe; e += 64) img[r * rowe + e] = (uint8_t)hpass(lo + r, e);
    }
    __syncthreads();

    const int G = a.S / a.ps, pp = a.ps * a.ps;
    for (int r = wave; r < trows; r += 4) {
        const int cy = y0 + r, yy = a.top + cy;           // row of the crop window | of the resized image
        const int py = cy / a.ps, dy = cy - py * a.ps;
        Taps t = {0, 0};
        const int32_t* k = nullptr;
        if (a.vcoef) {
            t = taps_of(a.vbounds, yy, a.Hin, a.vks);
            t.first = min(max(t.first, lo), lo + rows);
            t.n = min(t.n, lo + rows - t.first);
            k = a.vcoef + (long)yy * a.vks;
        }
        for (int j = lane; j < rowe; j += 64) {
            const int ch = j / tw, xl = j - ch * tw, e = xl * 3 + ch;
            int b;
            if (!a.vcoef) {
                b = hpass(yy, e);
            } else {
                int ss = 1 << (PRECISION_BITS - 1);
                if (staged) {
                    const uint8_t* p = img + (t.first - lo) * rowe + e;
                    for (int i = 0; i < t.n; ++i) ss += (int)p[i * rowe] * k[i];
                } else {
                    const uint8_t* p = src + t.first * a.ldx + c0 + e;
                    for (int i = 0; i < t.n; ++i) ss += (int)p[i * a.ldx] * k[i];
                }
                b = clip8(ss);
            }
            const int cx = x0 + xl, px = cx / a.ps, dx = cx - px * a.ps;
            f16* o = a.out + ((long)blockIdx.z * G * G + py * G + px) * a.ldo;
            o[ch * pp + dy * a.ps + dx] = lut[ch * 256 + b];
            if (ch == 0 && dy == 0 && dx == 0)
                for (int z = 3 * pp; z < a.Kpad; ++z) o[z] = (f16)0.0f;
            if (a.u8) a.u8[blockIdx.z * a.bsu + cy * a.ldu + cx * 3 + ch] = (uint8_t)b;
        }
    }
}

}  // namespace

extern "C" int sg_clip_patchify_u8(const uint8_t* x, int64_t bsx, int64_t ldx, int32_t N, int32_t Hin, int32_t Win, int32_t Hr, int32_t Wr,
                                   int32_t top, int32_t left, const float* mean, const float* std, int32_t S, int32_t ps, int32_t Kpad,
                                   sg_half* out, int64_t ldo, uint8_t* u8, int64_t bsu, int64_t ldu, const int32_t* hcoef,
                                   const int32_t* hbounds, const int32_t* vcoef, const int32_t* vbounds, sg_stream_t stream) {
    SG_REQUIRE(x && mean && std && out, "sg_clip_patchify_u8: null pointer");
    SG_REQUIRE(N > 0 && N <= 65535, "sg_clip_patchify_u8: N = %d (1 .. 65535)", N);
    SG_REQUIRE(Hin > 0 && Win > 0 && Hr > 0 && Wr > 0, "sg_clip_patchify_u8: sizes must be positive (%d x %d -> %d x %d)", Win, Hin, Wr, Hr);
    SG_REQUIRE(Hin <= SG_IMAGE_MAX_SIDE && Win <= SG_IMAGE_MAX_SIDE && Hr <= SG_IMAGE_MAX_SIDE && Wr <= SG_IMAGE_MAX_SIDE,
               "sg_clip_patchify_u8: a side of %d x %d -> %d x %d is above %d", Win, Hin, Wr, Hr, SG_IMAGE_MAX_SIDE);
    SG_REQUIRE(axis_admitted(Win, Wr) && axis_admitted(Hin, Hr), "sg_clip_patchify_u8: %d x %d -> %d x %d shrinks an axis by more than %d", Win,
               Hin, Wr, Hr, SG_IMAGE_MAX_RATIO);
    SG_REQUIRE(S > 0 && ps > 0 && ps <= S, "sg_clip_patchify_u8: bad crop size %d / patch size %d", S, ps);
    SG_REQUIRE(S % ps == 0, "sg_clip_patchify_u8: the crop size %d is not a multiple of the patch size %d", S, ps);
    const int64_t K = (int64_t)3 * ps * ps;
    SG_REQUIRE(Kpad % 8 == 0 && Kpad >= K, "sg_clip_patchify_u8: Kpad (%d) must be a multiple of 8 and at least 3 * ps * ps (%lld)", Kpad,
               (long long)K);
    SG_REQUIRE(ldo >= Kpad, "sg_clip_patchify_u8: output row stride %lld below Kpad %d", (long long)ldo, Kpad);
    SG_REQUIRE(top >= 0 && left >= 0 && (int64_t)top + S <= Hr && (int64_t)left + S <= Wr, "sg_clip_patchify_u8: the %d x %d crop window at "
               "(top %d, left %d) leaves the %d x %d resized image", S, S, top, left, Wr, Hr);
    SG_REQUIRE(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "sg_clip_patchify_u8: zero std");
    // every tensor is laid out pixel inside row inside image, without self-overlap
    const int64_t row_x = (int64_t)Win * 3, row_u = (int64_t)S * 3, rows_o = (int64_t)N * (S / ps) * (S / ps);
    SG_REQUIRE(ldx >= row_x && (N == 1 || bsx >= (int64_t)(Hin - 1) * ldx + row_x), "sg_clip_patchify_u8: input strides (batch %lld, row %lld) "
               "do not describe [N,%d,%d,3]", (long long)bsx, (long long)ldx, Hin, Win);
    SG_REQUIRE(!u8 || (ldu >= row_u && (N == 1 || bsu >= (int64_t)(S - 1) * ldu + row_u)), "sg_clip_patchify_u8: uint8 output strides (batch "
               "%lld, row %lld) do not describe [N,%d,%d,3]", (long long)bsu, (long long)ldu, S, S);
    const Span sx = span_of(x, bsx, 0, ldx, N, 1, Hin, row_x, 1);
    const Span su = u8 ? span_of(u8, bsu, 0, ldu, N, 1, S, row_u, 1) : Span{0, 0};
    const uintptr_t o_lo = reinterpret_cast<uintptr_t>(out);
    const Span so = {o_lo, o_lo + (uintptr_t)(((rows_o - 1) * ldo + Kpad) * 2)};
    SG_REQUIRE(!u8 || !overlap(su, so), "sg_clip_patchify_u8: the two outputs overlap");
    SG_REQUIRE(!overlap(sx, so) && !(u8 && overlap(sx, su)), "sg_clip_patchify_u8: an output overlaps the input");
    const bool need_h = Win != Wr, need_v = Hin != Hr;
    SG_REQUIRE(need_h ? (hcoef && hbounds) : (!hcoef && !hbounds), "sg_clip_patchify_u8: the horizontal tables are %s (%d -> %d columns)",
               need_h ? "missing" : "given for a pass that is skipped", Win, Wr);
    SG_REQUIRE(need_v ? (vcoef && vbounds) : (!vcoef && !vbounds), "sg_clip_patchify_u8: the vertical tables are %s (%d -> %d rows)",
               need_v ? "missing" : "given for a pass that is skipped", Hin, Hr);

    PatchU8Args a;
    a.x = x, a.bsx = (long)bsx, a.ldx = (long)ldx;
    a.out = reinterpret_cast<f16*>(out), a.ldo = (long)ldo;
    a.u8 = u8, a.bsu = (long)bsu, a.ldu = (long)ldu;
    a.hcoef = hcoef, a.hbounds = hbounds, a.vcoef = vcoef, a.vbounds = vbounds;
    a.Hin = Hin, a.Win = Win, a.top = top, a.left = left, a.S = S, a.ps = ps, a.Kpad = Kpad;
    a.hks = need_h ? axis_of(Win, Wr).ksize : 0;
    a.vks = need_v ? axis_of(Hin, Hr).ksize : 0;
    a.th = tile_rows(Hin, Hr, 3);
    if (need_h && need_v)       // the table shares the LDS budget with the staged rows: up to one row per tile fewer than sg_image_resize_u8
        while (a.th > 1 && (int64_t)staged_rows(axis_of(Hin, Hr), Hin, a.th) * SG_IMAGE_TILE_W * 3 + LUT_BYTES > SG_IMAGE_LDS_BYTES) --a.th;
    a.lds_rows = need_h && need_v ? staged_rows(axis_of(Hin, Hr), Hin, a.th) : 0;
    for (int c = 0; c < 3; ++c) a.mean[c] = mean[c], a.std[c] = std[c];
    const size_t img_bytes = (size_t)a.lds_rows * SG_IMAGE_TILE_W * 3;
    SG_REQUIRE(LUT_BYTES + img_bytes <= SG_IMAGE_LDS_BYTES, "sg_clip_patchify_u8: internal: %zu bytes of LDS for %d staged rows", img_bytes,
               a.lds_rows);
    const dim3 grid((S + SG_IMAGE_TILE_W - 1) / SG_IMAGE_TILE_W, (S + a.th - 1) / a.th, N);
    hipLaunchKernelGGL(clip_patchify_u8_kernel, grid, dim3(256), LUT_BYTES + img_bytes, (hipStream_t)stream, a);
    SG_CHECK_LAUNCH("sg_clip_patchify_u8");
    return SG_OK;
}
