// YOLOv9t detector (reference src/visp/arch/yolov9t.cpp): the stages between its convolutions. Every conv (Conv = conv + bias +
// SiLU, the folded RepConv, the detect head's plain 1x1) runs on the GEMM family (kernels_gemm.hip, epilogues VX_EPI_SILU and
// VX_EPI_F16). Maps are NHWC f16 with f32 arithmetic; a map may be a channel slice of a wider concat buffer (x_pix / y_pix =
// elements between pixels), so no concat is ever copied.
#include "vx_common.h"

namespace {

__global__ __launch_bounds__(256) void preprocess_kernel(const uint8_t* __restrict__ img, int channels, const float* __restrict__ f32,
                                                         f16* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v[3];
    if (img) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (float)img[i * channels + c] / 255.0f;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = f32[i * 3 + c];
    }
    f16x8 o = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f};
    *reinterpret_cast<f16x8*>(out + i * 8) = o;
}

// one thread per 8 channels of an output pixel
__global__ __launch_bounds__(256) void avgpool2_kernel(const f16* __restrict__ x, long x_pix, f16* __restrict__ y, int B, int H, int W, int C) {
    const int c8 = C / 8, OH = H - 1, OW = W - 1;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * OH * OW * c8) return;
    const int c = (int)(i % c8) * 8;
    long p = i / c8;
    const int ox = (int)(p % OW);
    p /= OW;
    const int oy = (int)(p % OH);
    const int b = (int)(p / OH);
    const f16* src = x + (((long)b * H + oy) * W + ox) * x_pix + c;
    const f16x8 a = *reinterpret_cast<const f16x8*>(src), bb = *reinterpret_cast<const f16x8*>(src + x_pix);
    const f16x8 cc = *reinterpret_cast<const f16x8*>(src + (long)W * x_pix), d = *reinterpret_cast<const f16x8*>(src + (long)(W + 1) * x_pix);
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)(((float)a[j] + (float)bb[j] + (float)cc[j] + (float)d[j]) * 0.25f);
    *reinterpret_cast<f16x8*>(y + i * 8) = o;
}

__global__ __launch_bounds__(256) void spp_kernel(f16* __restrict__ buf, long pix, int B, int H, int W, int C) {
    const int c8 = C / 8;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * H * W * c8) return;
    const int c = (int)(i % c8) * 8;
    long p = i / c8;
    const int x = (int)(p % W);
    p /= W;
    const int y = (int)(p % H);
    const int b = (int)(p / H);
    const f16* img = buf + (long)b * H * W * pix + c;
    f16x8 m5 = *reinterpret_cast<const f16x8*>(img + ((long)y * W + x) * pix); // the centre lies in every window
    f16x8 m9 = m5, m13 = m5;
    for (int dy = -6; dy <= 6; ++dy) {
        const int iy = y + dy;
        if (iy < 0 || iy >= H) continue;
        for (int dx = -6; dx <= 6; ++dx) {
            const int ix = x + dx;
            if (ix < 0 || ix >= W) continue;
            const f16x8 v = *reinterpret_cast<const f16x8*>(img + ((long)iy * W + ix) * pix);
            const int r = max(abs(dy), abs(dx));
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                m13[j] = v[j] > m13[j] ? v[j] : m13[j];
                if (r <= 4) m9[j] = v[j] > m9[j] ? v[j] : m9[j];
                if (r <= 2) m5[j] = v[j] > m5[j] ? v[j] : m5[j];
            }
        }
    }
    f16* o = buf + (((long)b * H + y) * W + x) * pix + c;
    *reinterpret_cast<f16x8*>(o + C) = m5;
    *reinterpret_cast<f16x8*>(o + 2 * C) = m9;
    *reinterpret_cast<f16x8*>(o + 3 * C) = m13;
}

__global__ __launch_bounds__(256) void upsample2_kernel(const f16* __restrict__ x, long x_pix, f16* __restrict__ y, long y_pix, int B, int h, int w, int C) {
    const int c8 = C / 8, OH = 2 * h, OW = 2 * w;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * OH * OW * c8) return;
    const int c = (int)(i % c8) * 8;
    long p = i / c8;
    const int ox = (int)(p % OW);
    p /= OW;
    const int oy = (int)(p % OH);
    const int b = (int)(p / OH);
    *reinterpret_cast<f16x8*>(y + (((long)b * OH + oy) * OW + ox) * y_pix + c) =
        *reinterpret_cast<const f16x8*>(x + (((long)b * h + (oy >> 1)) * w + (ox >> 1)) * x_pix + c);
}

// one thread per (image, anchor, item): items 0..3 are the four box sides (DFL + dist2bbox), item 4 + g the classes 8g..8g+7.
// Candidates are appended with one atomic per wave: a wave prefix-sums its lanes' counts and its last lane reserves the whole range
// (a wave that straddles two images falls back to one atomic per lane)
__global__ __launch_bounds__(256) void decode_kernel(const f16* __restrict__ raw0, const f16* __restrict__ raw1, const f16* __restrict__ raw2, int B, int S,
                                                     int nc, float* __restrict__ boxes, float* __restrict__ scores, float conf, int* __restrict__ cand_count,
                                                     int* __restrict__ cand_idx, float* __restrict__ cand_score) {
    const int J = 4 + nc / 8;
    const int g0 = S / 8, g1 = S / 16, g2 = S / 32;
    const int A0 = g0 * g0, A1 = g1 * g1, A = A0 + A1 + g2 * g2;
    const long total = (long)B * A * J;
    const long i0 = (long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i0 < total; // no early return: every lane takes part in the wave scan below
    const long i = valid ? i0 : total - 1;
    const int j = (int)(i % J);
    const long ba = i / J;
    const int a = (int)(ba % A), b = (int)(ba / A);
    const f16* raw;
    int g, cell;
    float stride;
    if (a < A0) { raw = raw0; g = g0; cell = a; stride = 8.0f; }
    else if (a < A0 + A1) { raw = raw1; g = g1; cell = a - A0; stride = 16.0f; }
    else { raw = raw2; g = g2; cell = a - A0 - A1; stride = 32.0f; }
    const f16* px = raw + ((long)b * g * g + cell) * (64 + nc);
    float s[8];
    int n = 0, c0 = 0;
    unsigned pass = 0;
    if (j < 4) {
        const f16x8 h0 = *reinterpret_cast<const f16x8*>(px + j * 16), h1 = *reinterpret_cast<const f16x8*>(px + j * 16 + 8);
        float v[16];
#pragma unroll
        for (int k = 0; k < 8; ++k) { v[k] = (float)h0[k]; v[k + 8] = (float)h1[k]; }
        float m = v[0];
#pragma unroll
        for (int k = 1; k < 16; ++k) m = fmaxf(m, v[k]);
        float sum = 0.0f, wsum = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float e = expf(v[k] - m);
            sum += e;
            wsum += e * (float)k;
        }
        const float d = wsum / sum;
        const float anchor = (j & 1) ? (float)(cell / g) + 0.5f : (float)(cell % g) + 0.5f; // sides 0, 2: x; 1, 3: y
        if (valid) boxes[ba * 4 + j] = (j < 2 ? anchor - d : anchor + d) * stride;
    } else {
        c0 = (j - 4) * 8;
        const f16x8 h = *reinterpret_cast<const f16x8*>(px + 64 + c0);
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = 1.0f / (1.0f + expf(-(float)h[k]));
        if (valid) {
            float* dst = scores + ba * nc + c0;
            *reinterpret_cast<float4*>(dst) = make_float4(s[0], s[1], s[2], s[3]);
            *reinterpret_cast<float4*>(dst + 4) = make_float4(s[4], s[5], s[6], s[7]);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (s[k] >= conf) { pass |= 1u << k; ++n; }
        }
    }
    if (!cand_count) return; // kernel-uniform
    const int lane = threadIdx.x & 63;
    int incl = n; // inclusive prefix sum of the lanes' counts
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    const int wave_total = __shfl(incl, 63, 64);
    const int b_first = __shfl(b, 0, 64);
    int base;
    if (__all(n == 0 || b == b_first)) {
        int got = 0;
        if (lane == 63 && wave_total > 0) got = atomicAdd(cand_count + b_first, wave_total);
        base = __shfl(got, 63, 64) + incl - n;
    } else {
        base = n > 0 ? atomicAdd(cand_count + b, n) : 0;
    }
    if (n > 0) {
        const long o = (long)b * A * nc + base;
        int q = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (pass >> k & 1u) {
                cand_idx[o + q] = a * nc + c0 + k;
                cand_score[o + q] = s[k];
                ++q;
            }
    }
}

} // namespace

extern "C" int vx_yolo_preprocess(const uint8_t* img_u8, int channels, const float* img_f32, void* out8, int64_t n_pixels, void* stream) {
    VX_REQUIRE(out8 && (img_u8 != nullptr) != (img_f32 != nullptr), "vx_yolo_preprocess: exactly one of the u8 and f32 inputs, and an output");
    VX_REQUIRE(!img_u8 || channels == 3 || channels == 4, "vx_yolo_preprocess: %d channels (3 or 4)", channels);
    VX_REQUIRE(n_pixels > 0 && aligned16(out8), "vx_yolo_preprocess: empty or misaligned");
    hipLaunchKernelGGL(preprocess_kernel, dim3(blocks_for(n_pixels)), dim3(256), 0, as_stream(stream), img_u8, channels, img_f32, static_cast<f16*>(out8), (long)n_pixels);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_yolo_avgpool2_f16(const void* x, int64_t x_pix, void* y, int B, int H, int W, int C, void* stream) {
    VX_REQUIRE(x && y && B > 0 && H >= 2 && W >= 2 && C > 0 && C % 8 == 0 && x_pix >= C && x_pix % 8 == 0 && aligned16(x) && aligned16(y),
               "vx_yolo_avgpool2_f16: bad shape B=%d H=%d W=%d C=%d pix=%ld", B, H, W, C, (long)x_pix);
    hipLaunchKernelGGL(avgpool2_kernel, dim3(blocks_for((long)B * (H - 1) * (W - 1) * (C / 8))), dim3(256), 0, as_stream(stream), static_cast<const f16*>(x),
                       (long)x_pix, static_cast<f16*>(y), B, H, W, C);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_yolo_spp_f16(void* buf, int64_t pix, int B, int H, int W, int C, void* stream) {
    VX_REQUIRE(buf && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && pix >= 4 * C && pix % 8 == 0 && aligned16(buf),
               "vx_yolo_spp_f16: bad shape B=%d H=%d W=%d C=%d pix=%ld", B, H, W, C, (long)pix);
    hipLaunchKernelGGL(spp_kernel, dim3(blocks_for((long)B * H * W * (C / 8))), dim3(256), 0, as_stream(stream), static_cast<f16*>(buf), (long)pix, B, H, W, C);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_yolo_upsample2_f16(const void* x, int64_t x_pix, void* y, int64_t y_pix, int B, int h, int w, int C, void* stream) {
    VX_REQUIRE(x && y && B > 0 && h > 0 && w > 0 && C > 0 && C % 8 == 0 && x_pix >= C && y_pix >= C && x_pix % 8 == 0 && y_pix % 8 == 0 && aligned16(x) &&
                   aligned16(y),
               "vx_yolo_upsample2_f16: bad shape B=%d h=%d w=%d C=%d", B, h, w, C);
    hipLaunchKernelGGL(upsample2_kernel, dim3(blocks_for((long)B * 4 * h * w * (C / 8))), dim3(256), 0, as_stream(stream), static_cast<const f16*>(x), (long)x_pix,
                       static_cast<f16*>(y), (long)y_pix, B, h, w, C);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_yolo_decode(const void* raw0, const void* raw1, const void* raw2, int B, int S, int nc, float* boxes, float* scores, float conf,
                              int* cand_count, int* cand_idx, float* cand_score, void* stream) {
    VX_REQUIRE(raw0 && raw1 && raw2 && boxes && scores && aligned16(raw0) && aligned16(raw1) && aligned16(raw2) && aligned16(scores),
               "vx_yolo_decode: null or misaligned operand");
    VX_REQUIRE(B > 0 && S >= 32 && S % 32 == 0 && nc > 0 && nc % 8 == 0, "vx_yolo_decode: bad shape B=%d S=%d nc=%d", B, S, nc);
    VX_REQUIRE((cand_count != nullptr) == (cand_idx != nullptr) && (cand_idx != nullptr) == (cand_score != nullptr),
               "vx_yolo_decode: the candidate list needs count, index and score buffers");
    const long A = (long)(S / 8) * (S / 8) + (long)(S / 16) * (S / 16) + (long)(S / 32) * (S / 32);
    hipLaunchKernelGGL(decode_kernel, dim3(blocks_for((long)B * A * (4 + nc / 8))), dim3(256), 0, as_stream(stream), static_cast<const f16*>(raw0),
                       static_cast<const f16*>(raw1), static_cast<const f16*>(raw2), B, S, nc, boxes, scores, conf, cand_count, cand_idx, cand_score);
    VX_LAUNCH_CHECK();
    return 1;
}
