// Depthwise convolution of any square kernel up to 7x7, stride 1 or 2, any pad below the kernel size (conv_2d_depthwise + add_bias_2d,
// nn.cpp:102-115): the graph layer's VISP_OP_CONV_2D_DEPTHWISE. TinyViT's mb_conv / patch_merging / local_conv are 3x3 pad 1
// (mobile-sam.cpp:84, 101, 155), MI-GAN's filters 3x3 and 4x4 at pad 1 and 2, stride 1 and 2 (migan.cpp:28-57).
//
// The shape of tv_dwconv3x3_kernel (kernels_tinyvit.hip), templated on (k, stride): one thread owns 8 channels x P consecutive output
// pixels of one row. Per kernel row it loads the (P - 1) S + K input pixels that feed all P outputs once, as 16-byte loads, and ONE row of
// K weight vectors -- a 7x7 kernel held whole would be 49 x 4 = 196 VGPRs, a row of it is 28. Accumulation is f32. Lanes run over the
// channel groups first, so a load / store instruction covers whole pixels (C * 2 contiguous bytes); blocks are numbered so that every XCD
// gets a contiguous run of the row-major sequence and the K output rows that read one input row fetch it through one L2.
// The kernel is memory bound: loads per output are K ((P - 1) S + K) / P instead of K^2 (3.75 instead of 9 at 3x3 / P = 8).
// Taps outside the map are zeros; a strip's tail past OW is computed and not stored.
// kernels_fir.hip holds a copy of this kernel with another tail (dwconv_agc_kernel: lrelu_agc): a change to the loop here belongs there as well.
#include "vx_common.h"

namespace {

template <int K, int S, int P>
__global__ __launch_bounds__(256) void dwconv_kernel(const f16* __restrict__ x, const f16* __restrict__ w, const float* __restrict__ bias, f16* __restrict__ y,
                                                     int B, int H, int W, int C, int OH, int OW, int pad, int act, float act_param) {
    constexpr int NC = (P - 1) * S + K, ROWS_UNROLLED = K <= 3 ? K : 1;
    const int c8n = C >> 3, strips = (OW + P - 1) / P;
    const long n = (long)B * OH * strips * c8n;
    long blk;
    { // XCD-aware block order (blocks b and b + 8 share an XCD and its L2)
        const long nwg = gridDim.x, b = blockIdx.x;
        const long q = nwg >> 3, rem = nwg & 7, xcd = b & 7;
        blk = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (b >> 3);
    }
    const long i = blk * blockDim.x + threadIdx.x;
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
    // kernels above 3x3: rows not unrolled, one row of weights and one row segment live at a time. Up to 3x3 the rows are unrolled (36 VGPRs of weights at
    // most): the compiler may then start a row's loads before the products of the row above it are done
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
        for (int j = 0; j < 8; ++j) {
            float v = acc[p][j] + bv[j];
            if (act == 1) v = gelu_tanh(v);
            else if (act == 2) v = v > 0.0f ? v : v * act_param;
            o[j] = (f16)v;
        }
        *reinterpret_cast<f16x8*>(out + (long)p * C) = o;
    }
}

// output pixels per thread: 8 at stride 1 up to 5x5, 4 beyond and at stride 2 -- the row segment (P - 1) S + K stays at 13 pixels (52 VGPRs) at most
template <int K, int S>
constexpr int strip_of() { return S == 1 && K <= 5 ? 8 : 4; }

template <int K, int S>
void launch(const f16* x, const f16* w, const float* bias, f16* y, int B, int H, int W, int C, int OH, int OW, int pad, int act, float act_param, hipStream_t st) {
    constexpr int P = strip_of<K, S>();
    const long n = (long)B * OH * ((OW + P - 1) / P) * (C / 8);
    hipLaunchKernelGGL((dwconv_kernel<K, S, P>), dim3(blocks_for(n)), dim3(256), 0, st, x, w, bias, y, B, H, W, C, OH, OW, pad, act, act_param);
}

} // namespace

extern "C" int vx_dwconv_f16(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int k, int stride, int pad, int act, float act_param,
                             void* stream) {
    VX_REQUIRE(x && w && y && B > 0 && H > 0 && W > 0 && C > 0, "vx_dwconv_f16: bad operands");
    VX_REQUIRE(C % 8 == 0, "vx_dwconv_f16: C = %d must be a multiple of 8", C);
    VX_REQUIRE(k >= 1 && k <= 7 && (stride == 1 || stride == 2), "vx_dwconv_f16: kernel %d, stride %d (kernels 1..7, stride 1 or 2)", k, stride);
    VX_REQUIRE(pad >= 0 && pad <= k - 1, "vx_dwconv_f16: pad %d with a %dx%d kernel (0 .. k - 1)", pad, k, k);
    VX_REQUIRE(act >= 0 && act <= 2, "vx_dwconv_f16: activation %d (0 none, 1 gelu, 2 leaky relu)", act);
    VX_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y), "vx_dwconv_f16: operands must be 16-byte aligned");
    VX_REQUIRE(H + 2 * pad >= k && W + 2 * pad >= k, "vx_dwconv_f16: a %dx%d kernel at pad %d does not fit a %dx%d map", k, k, pad, W, H);
    const int OH = (H + 2 * pad - k) / stride + 1, OW = (W + 2 * pad - k) / stride + 1;
    const long blocks = ((long)B * OH * ((OW + 3) / 4) * (C / 8) + 255) / 256;
    VX_REQUIRE(blocks < (1L << 31), "vx_dwconv_f16: the map is too large for one launch");
    const f16 *xp = reinterpret_cast<const f16*>(x), *wp = reinterpret_cast<const f16*>(w);
    f16* yp = reinterpret_cast<f16*>(y);
    hipStream_t st = as_stream(stream);
#define VX_DW(K_)                                                                                  \
    case K_:                                                                                       \
        if (stride == 1) launch<K_, 1>(xp, wp, bias, yp, B, H, W, C, OH, OW, pad, act, act_param, st); \
        else launch<K_, 2>(xp, wp, bias, yp, B, H, W, C, OH, OW, pad, act, act_param, st);         \
        break;
    switch (k) {
        VX_DW(1) VX_DW(2) VX_DW(3) VX_DW(4) VX_DW(5) VX_DW(6) VX_DW(7)
    }
#undef VX_DW
    VX_LAUNCH_CHECK();
    return 1;
}
