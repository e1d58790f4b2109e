// MI-GAN inpainting generator (reference src/visp/arch/migan.cpp): the non-GEMM stages of separable_conv_2d, the
// image path and the pre / post processing. All activations NHWC f16 with f32 arithmetic; the 1x1 convolutions run on
// the GEMM family (kernels_gemm.hip, epilogue VX_EPI_LRELU_AGC).
//
// Per-channel filters come from the file: depthwise 3x3 as f16 [9][C] (tap-major), the 4x4 down / up FIR as f32 [16][C].
// The upsample is written polyphase: the zero-insertion x2 map (nearest x2 times the [[1,0],[0,0]] filter_const tile,
// migan.cpp:34-51) is never formed; output row Y = 2m + py reads input rows m - 1 + py and m + py through FIR taps
// py and py + 2 (same for columns).
#include "vx_common.h"

namespace {

__device__ __forceinline__ float lrelu_agc(float v) { // migan.cpp:17-26 with alpha 0.2, gain sqrt2, clamp 256
    return fminf(fmaxf((v < 0.0f ? 0.2f * v : v) * 1.41421356f, -256.0f), 256.0f);
}

__device__ __forceinline__ void load8(const f16* p, float v[8]) {
    const f16x8 h = *reinterpret_cast<const f16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
}

__device__ __forceinline__ void store8(f16* p, const float v[8]) {
    f16x8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = (f16)v[j];
    *reinterpret_cast<f16x8*>(p) = h;
}

// activated depthwise 3x3 (zero padding 1) of 8 channels at (y, x) of image b
__device__ __forceinline__ void dw_at(const f16* __restrict__ x, const f16* __restrict__ w, const float* __restrict__ bias, int b, int y, int xx,
                                      int H, int W, int C, int c0, float out[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = bias[c0 + j];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = y + ky - 1;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = xx + kx - 1;
            if (ix < 0 || ix >= W) continue;
            float v[8], k[8];
            load8(x + (((int64_t)b * H + iy) * W + ix) * C + c0, v);
            load8(w + (ky * 3 + kx) * C + c0, k);
#pragma unroll
            for (int j = 0; j < 8; ++j) out[j] = fmaf(v[j], k[j], out[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = lrelu_agc(out[j]);
}

// y = lrelu_agc(dw3x3(x) + bias), same extent; one thread = one pixel x 8 channels
__global__ __launch_bounds__(256) void migan_dw3x3_agc_kernel(const f16* __restrict__ x, const f16* __restrict__ w, const float* __restrict__ bias,
                                                              f16* __restrict__ y, int B, int H, int W, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int G = C / 8;
    if (i >= (int64_t)B * H * W * G) return;
    const int c0 = (int)(i % G) * 8;
    const int64_t pix = i / G;
    const int xx = (int)(pix % W), yy = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
    float v[8];
    dw_at(x, w, bias, b, yy, xx, H, W, C, c0, v);
    store8(y + pix * C + c0, v);
}

// y = FIR4x4_stride2_pad1(lrelu_agc(dw3x3(x) + bias)) at half extent (migan.cpp:28-30, 53-66). A block owns an 8 x 8 tile of
// outputs x 32 channels: the 18 x 18 activated depthwise values under it (halo included, zeros outside the map = the FIR's
// zero padding) are computed once into LDS, then each output reads its 16 taps from there.
constexpr int DT = 8, DS = 2 * DT + 2, DC = 32;
__global__ __launch_bounds__(256) void migan_dw3x3_agc_down_kernel(const f16* __restrict__ x, const f16* __restrict__ w, const float* __restrict__ bias,
                                                                   const float* __restrict__ fir, f16* __restrict__ y, int B, int H, int W, int C) {
    __shared__ float s[DS * DS * DC];
    const int OH = H / 2, OW = W / 2;
    const int tiles_x = (OW + DT - 1) / DT;
    const int ty0 = (blockIdx.y / tiles_x) * DT, tx0 = (blockIdx.y % tiles_x) * DT;
    const int cb = blockIdx.x * DC, b = blockIdx.z;
    const int tid = threadIdx.x;
    for (int i = tid; i < DS * DS * (DC / 8); i += 256) {
        const int pos = i / (DC / 8), cg = (i % (DC / 8)) * 8;
        const int fy = pos / DS, fx = pos % DS;
        const int Y = 2 * ty0 - 1 + fy, X = 2 * tx0 - 1 + fx;
        float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (Y >= 0 && Y < H && X >= 0 && X < W) dw_at(x, w, bias, b, Y, X, H, W, C, cb + cg, v);
        float4* d = reinterpret_cast<float4*>(s + pos * DC + cg);
        d[0] = make_float4(v[0], v[1], v[2], v[3]);
        d[1] = make_float4(v[4], v[5], v[6], v[7]);
    }
    __syncthreads();
    const int op = tid / (DC / 8), cg = (tid % (DC / 8)) * 8;
    const int oy = op / DT, ox = op % DT;
    if (ty0 + oy >= OH || tx0 + ox >= OW) return;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int ky = 0; ky < 4; ++ky)
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) {
            const float* a = s + ((2 * oy + ky) * DS + 2 * ox + kx) * DC + cg;
            const float* f = fir + (ky * 4 + kx) * C + cb + cg;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf(a[j], f[j], acc[j]);
        }
    store8(y + (((int64_t)b * OH + ty0 + oy) * OW + tx0 + ox) * C + cb + cg, acc);
}

// out = lrelu_agc(upFIR(y) + noise[pixel]) + feat at twice the extent of y (synthesis conv1 after its 1x1, migan.cpp:67-80, 119-120)
__global__ __launch_bounds__(256) void migan_upsample_agc_kernel(const f16* __restrict__ yin, const float* __restrict__ fir, const float* __restrict__ noise,
                                                                 const f16* __restrict__ feat, f16* __restrict__ out, int B, int h, int w, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int G = C / 8, H = 2 * h, W = 2 * w;
    if (i >= (int64_t)B * H * W * G) return;
    const int c0 = (int)(i % G) * 8;
    const int64_t pix = i / G;
    const int X = (int)(pix % W), Y = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
    const int py = Y & 1, px = X & 1, my = Y >> 1, mx = X >> 1;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int ty = 0; ty < 2; ++ty) {
        const int iy = my - 1 + py + ty, ky = py + 2 * ty;
        if (iy < 0 || iy >= h) continue;
#pragma unroll
        for (int tx = 0; tx < 2; ++tx) {
            const int ix = mx - 1 + px + tx, kx = px + 2 * tx;
            if (ix < 0 || ix >= w) continue;
            float v[8];
            load8(yin + (((int64_t)b * h + iy) * w + ix) * C + c0, v);
            const float* f = fir + (ky * 4 + kx) * C + c0;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf(v[j], f[j], acc[j]);
        }
    }
    const float nz = noise ? noise[(int64_t)Y * W + X] : 0.0f;
    float fv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (feat) load8(feat + pix * C + c0, fv);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = lrelu_agc(acc[j] + nz) + fv[j];
    store8(out + pix * C + c0, acc);
}

// img = upFIR(img_prev) + torgb(x) + bias, 3 channels f32 (synthesis_block's image path, migan.cpp:122-129); one thread = one pixel
__global__ __launch_bounds__(256) void migan_torgb_kernel(const f16* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ bias,
                                                          const float* __restrict__ prev, const float* __restrict__ fir, float* __restrict__ img,
                                                          int B, int H, int W, int C) {
    __shared__ float sw[3 * 512];
    for (int i = threadIdx.x; i < 3 * C; i += 256) sw[i] = wt[i];
    __syncthreads();
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (int64_t)B * H * W) return;
    float o[3] = {bias[0], bias[1], bias[2]};
    const f16* xp = x + pix * C;
    for (int c = 0; c < C; c += 8) {
        float v[8];
        load8(xp + c, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            o[0] = fmaf(v[j], sw[c + j], o[0]);
            o[1] = fmaf(v[j], sw[C + c + j], o[1]);
            o[2] = fmaf(v[j], sw[2 * C + c + j], o[2]);
        }
    }
    if (prev) {
        const int X = (int)(pix % W), Y = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
        const int h = H / 2, w = W / 2, py = Y & 1, px = X & 1, my = Y >> 1, mx = X >> 1;
#pragma unroll
        for (int ty = 0; ty < 2; ++ty) {
            const int iy = my - 1 + py + ty, ky = py + 2 * ty;
            if (iy < 0 || iy >= h) continue;
#pragma unroll
            for (int tx = 0; tx < 2; ++tx) {
                const int ix = mx - 1 + px + tx, kx = px + 2 * tx;
                if (ix < 0 || ix >= w) continue;
                const float* pv = prev + (((int64_t)b * h + iy) * w + ix) * 3;
                const float* f = fir + (ky * 4 + kx) * 3;
#pragma unroll
                for (int j = 0; j < 3; ++j) o[j] = fmaf(pv[j], f[j], o[j]);
            }
        }
    }
    img[pix * 3 + 0] = o[0];
    img[pix * 3 + 1] = o[1];
    img[pix * 3 + 2] = o[2];
}

// migan_process_input's pixel (migan.cpp:142-159, mask inverted) -- or a given f32 4-channel input -- then fromrgb (1x1, 4 -> C,
// bias) and lrelu_agc (migan.cpp:84-89); one thread = one pixel x 8 output channels
__global__ __launch_bounds__(256) void migan_preprocess_kernel(const uint8_t* __restrict__ img, int img_ch, const uint8_t* __restrict__ mask,
                                                               const float* __restrict__ in4, const float* __restrict__ wt, const float* __restrict__ bias,
                                                               f16* __restrict__ out, int64_t n_pix, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int G = C / 8;
    if (i >= n_pix * G) return;
    const int c0 = (int)(i % G) * 8;
    const int64_t pix = i / G;
    float p[4];
    if (in4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = in4[pix * 4 + j];
    } else {
        const float a = 1.0f - (float)mask[pix] / 255.0f;
        const uint8_t* q = img + pix * img_ch;
        p[0] = a - 0.5f;
#pragma unroll
        for (int j = 0; j < 3; ++j) p[1 + j] = a * ((float)q[j] / 255.0f * 2.0f - 1.0f);
    }
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float* wr = wt + (c0 + j) * 4;
        float t = bias[c0 + j];
#pragma unroll
        for (int k = 0; k < 4; ++k) t = fmaf(p[k], wr[k], t);
        v[j] = lrelu_agc(t);
    }
    store8(out + pix * C + c0, v);
}

// rgb f32 -> rgba_u8 with x * 0.5 + 0.5 truncated as image_f32_to_u8 does, alpha = the (un-inverted) mask (migan.cpp:198-206)
__global__ __launch_bounds__(256) void migan_postprocess_kernel(const float* __restrict__ img, const uint8_t* __restrict__ mask, uint8_t* __restrict__ rgba,
                                                                int64_t n_pix) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= n_pix) return;
    uchar4 o;
    uint8_t* op = reinterpret_cast<uint8_t*>(&o);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float t = __fadd_rn(__fmul_rn(img[pix * 3 + j], 0.5f), 0.5f);
        op[j] = (uint8_t)__fmul_rn(fminf(fmaxf(t, 0.0f), 1.0f), 255.0f);
    }
    op[3] = mask[pix];
    reinterpret_cast<uchar4*>(rgba)[pix] = o;
}

} // namespace

extern "C" {

VX_API int vx_migan_dwconv_f16(const void* x, const void* w, const float* bias, const float* down_fir, void* y, int B, int H, int W, int C,
                               void* stream) {
    VX_REQUIRE(x && w && bias && y, "vx_migan_dwconv_f16: null pointer");
    VX_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y), "vx_migan_dwconv_f16: x, w and y must be 16-byte aligned");
    VX_REQUIRE(B > 0 && H >= 2 && W >= 2, "vx_migan_dwconv_f16: bad extent B=%d H=%d W=%d", B, H, W);
    VX_REQUIRE(C > 0 && C % 64 == 0, "vx_migan_dwconv_f16: C=%d must be a positive multiple of 64", C);
    if (down_fir) {
        VX_REQUIRE(H % 2 == 0 && W % 2 == 0, "vx_migan_dwconv_f16: downsample needs an even extent (%dx%d)", W, H);
        const int OH = H / 2, OW = W / 2;
        const dim3 grid((unsigned)(C / DC), (unsigned)(((OH + DT - 1) / DT) * ((OW + DT - 1) / DT)), (unsigned)B);
        VX_REQUIRE(B <= 65535, "vx_migan_dwconv_f16: batch %d too large", B);
        hipLaunchKernelGGL(migan_dw3x3_agc_down_kernel, grid, dim3(256), 0, as_stream(stream), static_cast<const f16*>(x), static_cast<const f16*>(w), bias,
                           down_fir, static_cast<f16*>(y), B, H, W, C);
    } else {
        hipLaunchKernelGGL(migan_dw3x3_agc_kernel, dim3(blocks_for((int64_t)B * H * W * (C / 8))), dim3(256), 0, as_stream(stream),
                           static_cast<const f16*>(x), static_cast<const f16*>(w), bias, static_cast<f16*>(y), B, H, W, C);
    }
    VX_LAUNCH_CHECK();
    return 1;
}

VX_API int vx_migan_upsample_f16(const void* y, const float* fir, const float* noise, const void* feat, void* out, int B, int h, int w, int C,
                                 void* stream) {
    VX_REQUIRE(y && fir && out, "vx_migan_upsample_f16: null pointer");
    VX_REQUIRE(aligned16(y) && aligned16(feat) && aligned16(out), "vx_migan_upsample_f16: y, feat and out must be 16-byte aligned");
    VX_REQUIRE(B > 0 && h > 0 && w > 0, "vx_migan_upsample_f16: bad extent B=%d h=%d w=%d", B, h, w);
    VX_REQUIRE(C > 0 && C % 8 == 0, "vx_migan_upsample_f16: C=%d must be a positive multiple of 8", C);
    hipLaunchKernelGGL(migan_upsample_agc_kernel, dim3(blocks_for((int64_t)B * 4 * h * w * (C / 8))), dim3(256), 0, as_stream(stream),
                       static_cast<const f16*>(y), fir, noise, static_cast<const f16*>(feat), static_cast<f16*>(out), B, h, w, C);
    VX_LAUNCH_CHECK();
    return 1;
}

VX_API int vx_migan_torgb(const void* x, const float* w, const float* bias, const float* img_prev, const float* fir, float* img, int B, int H, int W,
                          int C, void* stream) {
    VX_REQUIRE(x && w && bias && img, "vx_migan_torgb: null pointer");
    VX_REQUIRE(aligned16(x), "vx_migan_torgb: x must be 16-byte aligned");
    VX_REQUIRE(!img_prev || (fir && H % 2 == 0 && W % 2 == 0), "vx_migan_torgb: the image path needs its FIR and an even extent");
    VX_REQUIRE(B > 0 && H > 0 && W > 0, "vx_migan_torgb: bad extent B=%d H=%d W=%d", B, H, W);
    VX_REQUIRE(C > 0 && C % 8 == 0 && C <= 512, "vx_migan_torgb: C=%d must be a multiple of 8 in [8, 512]", C);
    hipLaunchKernelGGL(migan_torgb_kernel, dim3(blocks_for((int64_t)B * H * W)), dim3(256), 0, as_stream(stream), static_cast<const f16*>(x), w, bias,
                       img_prev, fir, img, B, H, W, C);
    VX_LAUNCH_CHECK();
    return 1;
}

VX_API int vx_migan_preprocess(const uint8_t* img, int img_channels, const uint8_t* mask, const float* in4, const float* w, const float* bias,
                               void* out, int64_t n_pixels, int C, void* stream) {
    VX_REQUIRE(w && bias && out, "vx_migan_preprocess: null pointer");
    VX_REQUIRE(aligned16(out), "vx_migan_preprocess: out must be 16-byte aligned");
    VX_REQUIRE(in4 || (img && mask && (img_channels == 3 || img_channels == 4)), "vx_migan_preprocess: need an f32 input or a 3/4-channel u8 image and a mask");
    VX_REQUIRE(n_pixels > 0 && C > 0 && C % 8 == 0, "vx_migan_preprocess: bad shape pixels=%lld C=%d", (long long)n_pixels, C);
    hipLaunchKernelGGL(migan_preprocess_kernel, dim3(blocks_for(n_pixels * (C / 8))), dim3(256), 0, as_stream(stream), img, img_channels, mask, in4, w,
                       bias, static_cast<f16*>(out), n_pixels, C);
    VX_LAUNCH_CHECK();
    return 1;
}

VX_API int vx_migan_postprocess(const float* img, const uint8_t* mask, uint8_t* rgba, int64_t n_pixels, void* stream) {
    VX_REQUIRE(img && mask && rgba && n_pixels > 0, "vx_migan_postprocess: null pointer or empty image");
    hipLaunchKernelGGL(migan_postprocess_kernel, dim3(blocks_for(n_pixels)), dim3(256), 0, as_stream(stream), img, mask, rgba, n_pixels);
    VX_LAUNCH_CHECK();
    return 1;
}

} // extern "C"
