// Image ingest: Pillow's 8-bit bicubic Image.resize (two fixed-point passes with a rounding to uint8 in between) and ToTensor, in one launch.
#include "image_resample.h"

namespace {

struct ResizeArgs {
    const uint8_t* x; long bsx, ldx;                      // uint8 [N,Hin,Win,C]
    uint8_t* u8; long bsu, ldu;                           // uint8 [N,Hout,Wout,C] or null
    f16* y; long bsy, csy, ldy;                           // fp16 [N,C,Hout,Wout] or null
    const int32_t *hcoef, *hbounds, *vcoef, *vbounds;     // null for a skipped pass
    int Hin, Win, Hout, Wout, hks, vks, th, lds_rows, flip;
};

// A workgroup (4 waves) owns th output rows x SG_IMAGE_TILE_W output columns of one image; a wave takes a row at a time, its lanes the
// row's tw * C bytes.  Both passes needed: the horizontal pass of the input rows [lo, lo + rows) that the tile's vertical taps read goes
// to LDS as uint8 (what Pillow's intermediate image holds), the vertical pass reads it from there.  One pass: it reads global memory.
template <int C>
__global__ __launch_bounds__(256) void image_resize_kernel(const ResizeArgs a) {
    extern __shared__ uint8_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * SG_IMAGE_TILE_W, tw = min(SG_IMAGE_TILE_W, a.Wout - x0), rowe = tw * C;
    const int y0 = blockIdx.y * a.th, trows = min(a.th, a.Hout - y0);
    const uint8_t* src = a.x + blockIdx.z * a.bsx;

    // byte e of the tile's columns in input row `row` after the horizontal pass
    auto hpass = [&](int row, int e) -> int {
        const uint8_t* p = src + row * a.ldx;
        if (!a.hcoef) return p[x0 * C + e];
        const int col = x0 + e / C, ch = e % C;
        const Taps t = taps_of(a.hbounds, col, a.Win, a.hks);
        const int32_t* k = a.hcoef + (long)col * a.hks;
        p += t.first * C + ch;
        int ss = 1 << (PRECISION_BITS - 1);
        for (int i = 0; i < t.n; ++i) ss += (int)p[i * C] * k[i];
        return clip8(ss);
    };
    auto store = [&](int yy, int e, int b) {
        const int col = x0 + e / C, ch = e % C, oc = a.flip ? a.Wout - 1 - col : col;
        if (a.u8) a.u8[blockIdx.z * a.bsu + yy * a.ldu + oc * C + ch] = (uint8_t)b;
        if (a.y) a.y[blockIdx.z * a.bsy + ch * a.csy + yy * a.ldy + oc] = (f16)((float)b / 255.0f);      // ToTensor, then the cast to fp16
    };

    if (!a.vcoef) {
        for (int r = wave; r < trows; r += 4)
            for (int e = lane; e < rowe; e += 64) store(y0 + r, e, hpass(y0 + r, e));
        return;
    }
    const bool staged = a.hcoef != nullptr;
    int lo = 0, rows = a.Hin;
    if (staged) {       // the input rows this tile's vertical taps read, cut to what the LDS image holds
        int hi = 0;
        lo = a.Hin;
        for (int r = 0; r < trows; ++r) {
            const Taps t = taps_of(a.vbounds, y0 + r, a.Hin, a.vks);
            lo = min(lo, t.first);
            hi = max(hi, t.first + t.n);
        }
        rows = min(max(hi - lo, 0), a.lds_rows);
        for (int r = wave; r < rows; r += 4)
            for (int e = lane; e < rowe; e += 64) lds[r * rowe + e] = (uint8_t)hpass(lo + r, e);
        __syncthreads();
    }
    for (int r = wave; r < trows; r += 4) {
        const int yy = y0 + r;
        Taps t = taps_of(a.vbounds, yy, a.Hin, a.vks);
        t.first = min(max(t.first, lo), lo + rows);
        t.n = min(t.n, lo + rows - t.first);
        const int32_t* k = a.vcoef + (long)yy * a.vks;
        for (int e = lane; e < rowe; e += 64) {
            int ss = 1 << (PRECISION_BITS - 1);
            if (staged) {
                const uint8_t* p = lds + (t.first - lo) * rowe + e;
                for (int i = 0; i < t.n; ++i) ss += (int)p[i * rowe] * k[i];
            } else {
                const uint8_t* p = src + t.first * a.ldx + x0 * C + e;
                for (int i = 0; i < t.n; ++i) ss += (int)p[i * a.ldx] * k[i];
            }
            store(yy, e, clip8(ss));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- host: the tables
// Pillow's precompute_coeffs / normalize_coeffs_8bpc for its bicubic filter, operation by operation in double: a fused multiply-add
// would round once where the C code rounds twice.
#pragma clang fp contract(off)
double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

void fill_table(int in, int out, int32_t* coef, int32_t* bounds) {
    const Axis ax = axis_of(in, out);
    double w[SG_IMAGE_MAX_KSIZE];
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * ax.scale;
        int xmin = (int)(center - ax.support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + ax.support + 0.5);
        if (xmax > in) xmax = in;
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            w[x] = bicubic_filter((x + xmin - center + 0.5) / ax.filterscale);
            ww += w[x];
        }
        int32_t* k = coef + (int64_t)xx * ax.ksize;
        for (int x = 0; x < ax.ksize; ++x) {
            if (x >= n) {
                k[x] = 0;
                continue;
            }
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = n;
    }
}

}  // namespace

extern "C" int sg_image_resample_ksize(int32_t in, int32_t out) {
    SG_REQUIRE(axis_admitted(in, out), "sg_image_resample_ksize: %d -> %d samples: sides are 1 .. %d and in / out <= %d", in, out,
               SG_IMAGE_MAX_SIDE, SG_IMAGE_MAX_RATIO);
    return axis_of(in, out).ksize;
}

extern "C" int sg_image_resample_table(int32_t in, int32_t out, int32_t* coef, int32_t* bounds) {
    SG_REQUIRE(coef && bounds, "sg_image_resample_table: null pointer");
    SG_REQUIRE(axis_admitted(in, out), "sg_image_resample_table: %d -> %d samples: sides are 1 .. %d and in / out <= %d", in, out,
               SG_IMAGE_MAX_SIDE, SG_IMAGE_MAX_RATIO);
    fill_table(in, out, coef, bounds);
    return SG_OK;
}

extern "C" int sg_image_resize_tile_rows(int32_t in_h, int32_t out_h, int32_t C) {
    SG_REQUIRE(C == 1 || C == 3, "sg_image_resize_tile_rows: C = %d (1 or 3)", C);
    SG_REQUIRE(axis_admitted(in_h, out_h), "sg_image_resize_tile_rows: %d -> %d rows: sides are 1 .. %d and in / out <= %d", in_h, out_h,
               SG_IMAGE_MAX_SIDE, SG_IMAGE_MAX_RATIO);
    return tile_rows(in_h, out_h, C);
}

extern "C" int sg_image_resize_u8(const uint8_t* x, int64_t bsx, int64_t ldx, int32_t N, int32_t Hin, int32_t Win, int32_t C, uint8_t* u8,
                                  int64_t bsu, int64_t ldu, sg_half* y, int64_t bsy, int64_t csy, int64_t ldy, int32_t Hout, int32_t Wout,
                                  const int32_t* hcoef, const int32_t* hbounds, const int32_t* vcoef, const int32_t* vbounds, int32_t flip,
                                  sg_stream_t stream) {
    SG_REQUIRE(x, "sg_image_resize: null input pointer");
    SG_REQUIRE(u8 || y, "sg_image_resize: both outputs are null");
    SG_REQUIRE(N > 0 && N <= 65535, "sg_image_resize: N = %d (1 .. 65535)", N);
    SG_REQUIRE(Hin > 0 && Win > 0 && Hout > 0 && Wout > 0, "sg_image_resize: sizes must be positive (%d x %d -> %d x %d)", Win, Hin, Wout, Hout);
    SG_REQUIRE(C == 1 || C == 3, "sg_image_resize: C = %d (1 or 3)", C);
    SG_REQUIRE(flip == 0 || flip == 1, "sg_image_resize: flip = %d (0 or 1)", flip);
    SG_REQUIRE(Hin <= SG_IMAGE_MAX_SIDE && Win <= SG_IMAGE_MAX_SIDE && Hout <= SG_IMAGE_MAX_SIDE && Wout <= SG_IMAGE_MAX_SIDE,
               "sg_image_resize: a side of %d x %d -> %d x %d is above %d", Win, Hin, Wout, Hout, SG_IMAGE_MAX_SIDE);
    SG_REQUIRE(axis_admitted(Win, Wout) && axis_admitted(Hin, Hout), "sg_image_resize: %d x %d -> %d x %d shrinks an axis by more than %d", Win,
               Hin, Wout, Hout, SG_IMAGE_MAX_RATIO);
    // every tensor is laid out pixel inside row inside image, without self-overlap
    const int64_t row_x = (int64_t)Win * C, row_o = (int64_t)Wout * C;
    SG_REQUIRE(ldx >= row_x && (N == 1 || bsx >= (int64_t)(Hin - 1) * ldx + row_x), "sg_image_resize: input strides (batch %lld, row %lld) do "
               "not describe [N,%d,%d,%d]", (long long)bsx, (long long)ldx, Hin, Win, C);
    SG_REQUIRE(!u8 || (ldu >= row_o && (N == 1 || bsu >= (int64_t)(Hout - 1) * ldu + row_o)), "sg_image_resize: uint8 output strides (batch "
               "%lld, row %lld) do not describe [N,%d,%d,%d]", (long long)bsu, (long long)ldu, Hout, Wout, C);
    const int64_t plane_y = (int64_t)(Hout - 1) * ldy + Wout;
    SG_REQUIRE(!y || (ldy >= Wout && (C == 1 || csy >= plane_y) && (N == 1 || bsy >= (int64_t)(C - 1) * csy + plane_y)), "sg_image_resize: fp16 "
               "output strides (batch %lld, channel %lld, row %lld) do not describe [N,%d,%d,%d]", (long long)bsy, (long long)csy,
               (long long)ldy, C, Hout, Wout);
    const Span sx = span_of(x, bsx, 0, ldx, N, 1, Hin, row_x, 1);
    const Span su = u8 ? span_of(u8, bsu, 0, ldu, N, 1, Hout, row_o, 1) : Span{0, 0};
    const Span sy = y ? span_of(y, bsy, csy, ldy, N, C, Hout, Wout, 2) : Span{0, 0};
    SG_REQUIRE(!(u8 && y) || !overlap(su, sy), "sg_image_resize: the two outputs overlap");
    SG_REQUIRE(!(u8 && overlap(sx, su)) && !(y && overlap(sx, sy)), "sg_image_resize: an output overlaps the input");
    const bool need_h = Win != Wout, need_v = Hin != Hout;
    SG_REQUIRE(need_h ? (hcoef && hbounds) : (!hcoef && !hbounds), "sg_image_resize: the horizontal tables are %s (%d -> %d columns)",
               need_h ? "missing" : "given for a pass that is skipped", Win, Wout);
    SG_REQUIRE(need_v ? (vcoef && vbounds) : (!vcoef && !vbounds), "sg_image_resize: the vertical tables are %s (%d -> %d rows)",
               need_v ? "missing" : "given for a pass that is skipped", Hin, Hout);

    ResizeArgs a;
    a.x = x, a.bsx = (long)bsx, a.ldx = (long)ldx;
    a.u8 = u8, a.bsu = (long)bsu, a.ldu = (long)ldu;
    a.y = reinterpret_cast<f16*>(y), a.bsy = (long)bsy, a.csy = (long)csy, a.ldy = (long)ldy;
    a.hcoef = hcoef, a.hbounds = hbounds, a.vcoef = vcoef, a.vbounds = vbounds;
    a.Hin = Hin, a.Win = Win, a.Hout = Hout, a.Wout = Wout, a.flip = flip;
    a.hks = need_h ? axis_of(Win, Wout).ksize : 0;
    a.vks = need_v ? axis_of(Hin, Hout).ksize : 0;
    a.th = tile_rows(Hin, Hout, C);
    a.lds_rows = need_h && need_v ? staged_rows(axis_of(Hin, Hout), Hin, a.th) : 0;
    const size_t lds_bytes = (size_t)a.lds_rows * SG_IMAGE_TILE_W * C;
    SG_REQUIRE(lds_bytes <= SG_IMAGE_LDS_BYTES, "sg_image_resize: internal: %zu bytes of LDS for %d staged rows", lds_bytes, a.lds_rows);
    const dim3 grid((Wout + SG_IMAGE_TILE_W - 1) / SG_IMAGE_TILE_W, (Hout + a.th - 1) / a.th, N);
    if (C == 3) hipLaunchKernelGGL(image_resize_kernel<3>, grid, dim3(256), lds_bytes, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(image_resize_kernel<1>, grid, dim3(256), lds_bytes, (hipStream_t)stream, a);
    SG_CHECK_LAUNCH("sg_image_resize_u8");
    return SG_OK;
}
