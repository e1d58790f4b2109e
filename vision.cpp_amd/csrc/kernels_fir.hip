// The two kernels of MI-GAN's node groups that the graph layer lowers onto (csrc/lower_migan.cpp), for any channel count that is a multiple of 8:
//
// vx_upfirdn2x_f16 -- interpolate(x2, NEAREST) -> mul(filter_const) -> conv_2d_depthwise(4x4, pad 2) -> slice -> cont (migan.cpp:32-51) with filter_const the
// tile [[1, 0], [0, 0]] is zero insertion followed by a FIR: out[Y, X] = sum_{i,j} f[i][j] z[Y + i - 2, X + j - 2], z[2a, 2b] = x[a, b], zero elsewhere. Of the 16
// taps only those with Y + i and X + j even meet a sample, so per output parity 2 x 2 input pixels and 4 taps remain:
//   Y = 2a:     i = 0 reads row a - 1, i = 2 row a          X = 2b:     j = 0 reads column b - 1, j = 2 column b
//   Y = 2a + 1: i = 1 reads row a,     i = 3 row a + 1      X = 2b + 1: j = 1 reads column b,     j = 3 column b + 1
// The shape of dwconv_kernel / pool_kernel: one thread owns 8 channels x P input columns of one input row a, i.e. the 2 x 2P output pixels of the row pair
// (2a, 2a + 1). Per input row a - 1, a, a + 1 it loads the P + 2 pixels that feed them once (16-byte loads) and the four taps of each output row that row
// meets; every loaded pixel serves its four outputs. Lanes run over the channel groups first, so a load / store instruction covers whole pixels. No LDS, no
// scratch, no x2 intermediate in memory: the map is read once (re-reads of the neighbours hit the caches) and the result written once. Accumulation and the
// epilogue (+ noise plane, lrelu_agc, + residual map; separable_conv_2d and synthesis_block's order, migan.cpp:66-80, 116-124) are f32, one f16 rounding.
//
// vx_dwconv_agc_f16 -- kernels_dwconv.hip's kernel with lrelu_agc (migan.cpp:17-26) as its tail: a kernel of its own with a copy of the source. Sharing the body
// through a header (the tail as a functor) was tried: kernels_dwconv.hip's device assembly sum (tools/device_asm_sums.sh) moved, so the existing kernel stays as it is.
#include "vx_common.h"

namespace {

__device__ __forceinline__ long xcd_block(long nwg, long b) { // XCD-aware block order (blocks b and b + 8 share an XCD and its L2), as dwconv_kernel
    const long q = nwg >> 3, rem = nwg & 7, xcd = b & 7;
    return (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (b >> 3);
}

__device__ __forceinline__ float lrelu_agc(float v, float slope, float gain, float clamp) {
    v = (v > 0.0f ? v : v * slope) * gain;
    if (clamp > 0.0f) v = v < -clamp ? -clamp : (v > clamp ? clamp : v);
    return v;
}

template <int P>
__global__ __launch_bounds__(256) void upfirdn2x_kernel(const f16* __restrict__ x, long x_pix, const f16* __restrict__ fir, f16* __restrict__ y, long y_pix,
                                                        const float* __restrict__ plane, const f16* __restrict__ res, long res_pix, int agc, float gain, float clamp,
                                                        int B, int h, int w, int C) {
    const int c8n = C >> 3, strips = (w + P - 1) / P;
    const long n = (long)B * h * strips * c8n;
    const long i = xcd_block(gridDim.x, blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c8 = (int)(i % c8n);
    long q = i / c8n;
    const int b0 = (int)(q % strips) * P;
    q /= strips;
    const int a = (int)(q % h), img = (int)(q / h);
    float acc[2][2 * P][8];
#pragma unroll
    for (int oy = 0; oy < 2; ++oy)
#pragma unroll
        for (int p = 0; p < 2 * P; ++p)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[oy][p][j] = 0.0f;
#pragma unroll
    for (int dr = -1; dr <= 1; ++dr) {
        const int r = a + dr;
        if ((unsigned)r >= (unsigned)h) continue;
        const f16* row = x + ((long)img * h + r) * w * x_pix + c8 * 8;
        f16x8 col[P + 2];
#pragma unroll
        for (int t = 0; t < P + 2; ++t) {
            const int c = b0 - 1 + t;
            if ((unsigned)c < (unsigned)w) col[t] = *reinterpret_cast<const f16x8*>(row + (long)c * x_pix);
            else col[t] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int oy = 0; oy < 2; ++oy) {
            // the tap row of output row 2a + oy that meets input row a + dr: 2 (dr + 1) - oy, where that is one of 0..3 and of the parity's two
            const int ti = dr == -1 ? (oy == 0 ? 0 : -1) : (dr == 0 ? (oy == 0 ? 2 : 1) : (oy == 1 ? 3 : -1));
            if (ti < 0) continue;
            f16x8 wv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) wv[j] = *reinterpret_cast<const f16x8*>(fir + (long)(ti * 4 + j) * C + c8 * 8);
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    // input column b0 + p is col[p + 1]
                    acc[oy][2 * p][j] = fmaf((float)col[p][j], (float)wv[0][j], acc[oy][2 * p][j]);
                    acc[oy][2 * p][j] = fmaf((float)col[p + 1][j], (float)wv[2][j], acc[oy][2 * p][j]);
                    acc[oy][2 * p + 1][j] = fmaf((float)col[p + 1][j], (float)wv[1][j], acc[oy][2 * p + 1][j]);
                    acc[oy][2 * p + 1][j] = fmaf((float)col[p + 2][j], (float)wv[3][j], acc[oy][2 * p + 1][j]);
                }
        }
    }
    const int W2 = 2 * w;
#pragma unroll
    for (int oy = 0; oy < 2; ++oy) {
        const long prow = ((long)img * 2 * h + 2 * a + oy) * W2; // first pixel of the output row, over the batch
#pragma unroll
        for (int p = 0; p < 2 * P; ++p) {
            const int X = 2 * b0 + p;
            if (X >= W2) break;
            const float nz = plane ? plane[(long)(2 * a + oy) * W2 + X] : 0.0f;
            f16x8 rv = {0, 0, 0, 0, 0, 0, 0, 0};
            if (res) rv = *reinterpret_cast<const f16x8*>(res + (prow + X) * res_pix + c8 * 8);
            f16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float v = acc[oy][p][j] + nz;
                if (agc) v = lrelu_agc(v, 0.2f, gain, clamp);
                o[j] = (f16)(v + (float)rv[j]);
            }
            *reinterpret_cast<f16x8*>(y + (prow + X) * y_pix + c8 * 8) = o;
        }
    }
}

// dwconv_kernel (kernels_dwconv.hip) with the lrelu_agc tail
template <int K, int S, int P>
__global__ __launch_bounds__(256) void dwconv_agc_kernel(const f16* __restrict__ x, const f16* __restrict__ w, const float* __restrict__ bias, f16* __restrict__ y,
                                                         int B, int H, int W, int C, int OH, int OW, int pad, float slope, float gain, float clamp) {
    constexpr int NC = (P - 1) * S + K, ROWS_UNROLLED = K <= 3 ? K : 1;
    const int c8n = C >> 3, strips = (OW + P - 1) / P;
    const long n = (long)B * OH * strips * c8n;
    const long i = xcd_block(gridDim.x, blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c8 = (int)(i % c8n);
    long q = i / c8n;
    const int ox0 = (int)(q % strips) * P;
    q /= strips;
    const int oy = (int)(q % OH), b = (int)(q / OH);
    float acc[P][8];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[p][j] = 0.0f;
    const int ix0 = ox0 * S - pad;
#pragma unroll ROWS_UNROLLED
    for (int ky = 0; ky < K; ++ky) {
        const int iy = oy * S - pad + ky;
        if ((unsigned)iy >= (unsigned)H) continue;
        f16x8 wv[K];
#pragma unroll
        for (int kx = 0; kx < K; ++kx) wv[kx] = *reinterpret_cast<const f16x8*>(w + (long)(ky * K + kx) * C + c8 * 8);
        const f16* row = x + ((long)b * H + iy) * W * C + c8 * 8;
        f16x8 col[NC];
#pragma unroll
        for (int t = 0; t < NC; ++t) {
            const int ix = ix0 + t;
            if ((unsigned)ix < (unsigned)W) col[t] = *reinterpret_cast<const f16x8*>(row + (long)ix * C);
            else col[t] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int kx = 0; kx < K; ++kx)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[p][j] = fmaf((float)col[p * S + kx][j], (float)wv[kx][j], acc[p][j]);
    }
    float bv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = bias ? bias[c8 * 8 + j] : 0.0f;
    f16* out = y + (((long)b * OH + oy) * OW + ox0) * C + c8 * 8;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        if (ox0 + p >= OW) break;
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)lrelu_agc(acc[p][j] + bv[j], slope, gain, clamp);
        *reinterpret_cast<f16x8*>(out + (long)p * C) = o;
    }
}

// output pixels per thread, as kernels_dwconv.hip chooses them
template <int K, int S>
constexpr int strip_of() { return S == 1 && K <= 5 ? 8 : 4; }

template <int K, int S>
void launch_agc(const f16* x, const f16* w, const float* bias, f16* y, int B, int H, int W, int C, int OH, int OW, int pad, float slope, float gain, float clamp, hipStream_t st) {
    constexpr int P = strip_of<K, S>();
    const long n = (long)B * OH * ((OW + P - 1) / P) * (C / 8);
    hipLaunchKernelGGL((dwconv_agc_kernel<K, S, P>), dim3(blocks_for(n)), dim3(256), 0, st, x, w, bias, y, B, H, W, C, OH, OW, pad, slope, gain, clamp);
}

constexpr int UP_P = 2; // input columns per thread: 2 x 4 output pixels, 64 f32 accumulators (DESIGN.md section 18 has the register count)

} // namespace

extern "C" int vx_upfirdn2x_f16(const void* x, int64_t x_pix, const void* fir, void* y, int64_t y_pix, const float* plane, const void* res, int64_t res_pix, int agc,
                                float gain, float clamp, int B, int h, int w, int C, void* stream) {
    VX_REQUIRE(x && fir && y && B > 0 && h > 0 && w > 0 && C > 0, "vx_upfirdn2x_f16: bad operands");
    VX_REQUIRE(C % 8 == 0, "vx_upfirdn2x_f16: C = %d must be a multiple of 8", C);
    VX_REQUIRE(x_pix >= C && y_pix >= C && x_pix % 8 == 0 && y_pix % 8 == 0, "vx_upfirdn2x_f16: pixel strides %ld / %ld (multiples of 8, at least C = %d)", (long)x_pix, (long)y_pix, C);
    VX_REQUIRE(!res || (res_pix >= C && res_pix % 8 == 0), "vx_upfirdn2x_f16: residual pixel stride %ld (a multiple of 8, at least C = %d)", (long)res_pix, C);
    VX_REQUIRE(aligned16(x) && aligned16(fir) && aligned16(y) && aligned16(res), "vx_upfirdn2x_f16: operands must be 16-byte aligned");
    // an input may share the output's buffer only as another channel slice of the same pixels (equal pixel strides, disjoint channel ranges)
    auto clear_of_y = [&](const void* a, int64_t a_pix, int64_t a_pixels) {
        const char *ab = static_cast<const char*>(a), *yb = static_cast<const char*>(y);
        const int64_t a_span = ((a_pixels - 1) * a_pix + C) * 2, y_span = (((int64_t)B * 4 * h * w - 1) * y_pix + C) * 2;
        if (!a || ab + a_span <= yb || yb + y_span <= ab) return true;
        if (a_pix != y_pix) return false;
        const int64_t d = (((ab - yb) / 2) % y_pix + y_pix) % y_pix;
        return d >= C && d <= y_pix - C;
    };
    VX_REQUIRE(clear_of_y(x, x_pix, (int64_t)B * h * w) && clear_of_y(res, res_pix, (int64_t)B * 4 * h * w), "vx_upfirdn2x_f16: the output may not alias or overlap an input");
    VX_REQUIRE(!agc || (gain - gain == 0.0f && clamp >= 0.0f && clamp - clamp == 0.0f), "vx_upfirdn2x_f16: gain %g, clamp %g (finite; clamp >= 0, 0 for none)", (double)gain, (double)clamp);
    const long n = (long)B * h * ((w + UP_P - 1) / UP_P) * (C / 8);
    VX_REQUIRE((n + 255) / 256 < (1L << 31), "vx_upfirdn2x_f16: the map is too large for one launch");
    hipLaunchKernelGGL((upfirdn2x_kernel<UP_P>), dim3(blocks_for(n)), dim3(256), 0, as_stream(stream), reinterpret_cast<const f16*>(x), (long)x_pix, reinterpret_cast<const f16*>(fir),
                       reinterpret_cast<f16*>(y), (long)y_pix, plane, reinterpret_cast<const f16*>(res), (long)res_pix, agc, gain, clamp, B, h, w, C);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_dwconv_agc_f16(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int k, int stride, int pad, float slope, float gain,
                                 float clamp, void* stream) {
    VX_REQUIRE(x && w && y && B > 0 && H > 0 && W > 0 && C > 0, "vx_dwconv_agc_f16: bad operands");
    VX_REQUIRE(C % 8 == 0, "vx_dwconv_agc_f16: C = %d must be a multiple of 8", C);
    VX_REQUIRE(k >= 1 && k <= 7 && (stride == 1 || stride == 2), "vx_dwconv_agc_f16: kernel %d, stride %d (kernels 1..7, stride 1 or 2)", k, stride);
    VX_REQUIRE(pad >= 0 && pad <= k - 1, "vx_dwconv_agc_f16: pad %d with a %dx%d kernel (0 .. k - 1)", pad, k, k);
    VX_REQUIRE(slope - slope == 0.0f && gain - gain == 0.0f && clamp >= 0.0f && clamp - clamp == 0.0f, "vx_dwconv_agc_f16: slope %g, gain %g, clamp %g (finite; clamp >= 0, 0 for none)",
               (double)slope, (double)gain, (double)clamp);
    VX_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y), "vx_dwconv_agc_f16: operands must be 16-byte aligned");
    VX_REQUIRE(H + 2 * pad >= k && W + 2 * pad >= k, "vx_dwconv_agc_f16: a %dx%d kernel at pad %d does not fit a %dx%d map", k, k, pad, W, H);
    const int OH = (H + 2 * pad - k) / stride + 1, OW = (W + 2 * pad - k) / stride + 1;
    const int P = stride == 1 && k <= 5 ? 8 : 4; // strip_of<k, stride>()
    const long blocks = ((long)B * OH * ((OW + P - 1) / P) * (C / 8) + 255) / 256;
    VX_REQUIRE(blocks < (1L << 31), "vx_dwconv_agc_f16: the map is too large for one launch");
    const f16 *xp = reinterpret_cast<const f16*>(x), *wp = reinterpret_cast<const f16*>(w);
    f16* yp = reinterpret_cast<f16*>(y);
    hipStream_t st = as_stream(stream);
#define VX_DW(K_)                                                                                          \
    case K_:                                                                                               \
        if (stride == 1) launch_agc<K_, 1>(xp, wp, bias, yp, B, H, W, C, OH, OW, pad, slope, gain, clamp, st); \
        else launch_agc<K_, 2>(xp, wp, bias, yp, B, H, W, C, OH, OW, pad, slope, gain, clamp, st);         \
        break;
    switch (k) {
        VX_DW(1) VX_DW(2) VX_DW(3) VX_DW(4) VX_DW(5) VX_DW(6) VX_DW(7)
    }
#undef VX_DW
    VX_LAUNCH_CHECK();
    return 1;
}
