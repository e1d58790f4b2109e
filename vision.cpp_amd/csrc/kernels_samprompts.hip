// Kernels of the batched MobileSAM decode (many prompts per encoded image; csrc/sam_decoder.cpp sam_compute_batch_device): what the single-prompt
// path does on the host between its launches, here on the device so that a chunk of prompts never waits for the host.
//   vx_sam_iou_head_f32     iou_prediction_head (mobile-sam.cpp:476-481) on the iou token of each prompt, f32 weights and sums, and the choice of
//                           vision.cpp:80-82: the best of the first three predictions, the first index on ties
//   vx_sam_process_masks    sam_process_mask (mobile-sam.cpp:556-583) for P prompts, each on the logit plane its `chosen` entry names: two launches
//                           with the arithmetic of tv_sam_interp_kernel (kernels_tinyvit.hip), bit for bit
//   vx_sam_tile_rows_f16    dst[b][i] = src[i]: the image-side operands every prompt shares in layer 0, laid out per prompt
// No scratch, no atomics; every value leaves through a vector store.
#include "vx_common.h"

namespace {

constexpr int IOU_MAX_WIDTH = 1024, IOU_MAX_OUT = 64;

// y[n] = act(b[n] + sum_k w[n][k] x[k]) for n < N: wave w of the block takes rows w, w + 4, ..; its lanes walk the row 64 apart (coalesced), each a
// sequential f32 chain with k ascending, then a butterfly over the wave. The same order on every run.
__device__ __forceinline__ void iou_linear(const float* __restrict__ w, const float* __restrict__ b, const float* x, float* y, int N, int K, bool relu) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int n = wave; n < N; n += 4) {
        const float* wr = w + (long)n * K;
        float acc = 0.0f;
        for (int k = lane; k < K; k += 64) acc = fmaf(wr[k], x[k], acc);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) {
            acc += b[n];
            y[n] = relu ? fmaxf(acc, 0.0f) : acc;
        }
    }
}

// one block of 256 threads per prompt; the two hidden vectors live in LDS
__global__ __launch_bounds__(256) void sam_iou_head_kernel(const f16* __restrict__ tokens, long row_stride, const float* __restrict__ w0, const float* __restrict__ b0,
                                                           const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                           const float* __restrict__ b2, int K0, int N0, int N1, int N2, float* __restrict__ iou,
                                                           int* __restrict__ chosen) {
    __shared__ float xa[IOU_MAX_WIDTH], xb[IOU_MAX_WIDTH], yo[IOU_MAX_OUT];
    const long p = blockIdx.x;
    const f16* t = tokens + p * row_stride;
    for (int k = threadIdx.x; k < K0; k += 256) xa[k] = (float)t[k];
    __syncthreads();
    iou_linear(w0, b0, xa, xb, N0, K0, true);
    __syncthreads();
    iou_linear(w1, b1, xb, xa, N1, N0, true);
    __syncthreads();
    iou_linear(w2, b2, xa, yo, N2, N1, false);
    __syncthreads();
    if (threadIdx.x < N2) iou[p * N2 + threadIdx.x] = yo[threadIdx.x];
    if (threadIdx.x == 0 && chosen) { // std::max_element over the first three: a later one wins only when it is strictly larger
        int best = 0;
        if (yo[1] > yo[best]) best = 1;
        if (yo[2] > yo[best]) best = 2;
        chosen[p] = best;
    }
}

// The body of tv_sam_interp_kernel (kernels_tinyvit.hip) with the prompt on blockIdx.y. Contraction is off so the coordinates round as in the
// reference's C++ and as in the single-prompt kernel.
template <typename TS>
__device__ __forceinline__ void sam_interp_one(const TS* __restrict__ src, int sw, int sh, int sstride, int step, void* __restrict__ dst, int dw, int dh, int out_u8) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dw * dh) return;
    const int x = i % dw, y = i / dw;
    const float scale_x = (float)sw / (float)dw, scale_y = (float)sh / (float)dh;
    const float sxf = fmaxf(((float)x + 0.5f) * scale_x - 0.5f, 0.0f), syf = fmaxf(((float)y + 0.5f) * scale_y - 0.5f, 0.0f);
    const int x0 = (int)sxf, y0 = (int)syf;
    const int x1 = min(x0 + 1, sw - 1), y1 = min(y0 + 1, sh - 1);
    const float v00 = (float)src[((long)y0 * sstride + x0) * step], v01 = (float)src[((long)y0 * sstride + x1) * step];
    const float v10 = (float)src[((long)y1 * sstride + x0) * step], v11 = (float)src[((long)y1 * sstride + x1) * step];
    const float wx = sxf - (float)x0, wy = syf - (float)y0;
    const float v0 = (1 - wx) * v00 + wx * v01, v1 = (1 - wx) * v10 + wx * v11;
    const float v = (1 - wy) * v0 + wy * v1;
    if (out_u8) reinterpret_cast<uint8_t*>(dst)[i] = v > 0.0f ? 255 : 0;
    else reinterpret_cast<float*>(dst)[i] = v;
}

// step 1: plane chosen[p] of prompt p (mask_size^2 f16 logits, element (x, y) at (y mask_size + x) step) -> scaled f32 [p][image_size^2]
__global__ __launch_bounds__(256) void sam_masks_upscale_kernel(const f16* __restrict__ planes, long prompt_stride, long plane_stride, int step, int mask_size,
                                                                const int* __restrict__ chosen, int n_planes, float* __restrict__ scaled, int image_size) {
    const long p = blockIdx.y;
    const int c = min(max(chosen[p], 0), n_planes - 1); // a value outside the planes reads the nearest one, never beyond the buffer
    sam_interp_one<f16>(planes + p * prompt_stride + c * plane_stride, mask_size, mask_size, mask_size, step, scaled + p * (long)image_size * image_size, image_size,
                        image_size, 0);
}

// step 2: the top-left sw x sh of scaled[p] -> u8 [p][dh][dw], thresholded at 0
__global__ __launch_bounds__(256) void sam_masks_crop_kernel(const float* __restrict__ scaled, int image_size, int sw, int sh, uint8_t* __restrict__ out, int dw, int dh) {
    const long p = blockIdx.y;
    sam_interp_one<float>(scaled + p * (long)image_size * image_size, sw, sh, image_size, 1, out + p * (long)dw * dh, dw, dh, 1);
}

__global__ __launch_bounds__(256) void sam_tile_rows_kernel(const f16x8* __restrict__ src, f16x8* __restrict__ dst, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n8) dst[(long)blockIdx.y * n8 + i] = src[i];
}

} // namespace

extern "C" int vx_sam_iou_head_f32(const void* tokens, int64_t row_stride, int P, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                                   const float* b2, int K0, int N0, int N1, int N2, float* iou, int32_t* chosen, void* stream) {
    VX_REQUIRE(tokens && w0 && b0 && w1 && b1 && w2 && b2 && iou && P > 0, "vx_sam_iou_head_f32: bad operands");
    VX_REQUIRE(K0 > 0 && N0 > 0 && N1 > 0 && K0 <= IOU_MAX_WIDTH && N0 <= IOU_MAX_WIDTH && N1 <= IOU_MAX_WIDTH, "vx_sam_iou_head_f32: widths %d -> %d -> %d (1 .. %d)", K0,
               N0, N1, IOU_MAX_WIDTH);
    VX_REQUIRE(N2 >= 3 && N2 <= IOU_MAX_OUT, "vx_sam_iou_head_f32: %d predictions (3 .. %d: the choice is among the first three)", N2, IOU_MAX_OUT);
    VX_REQUIRE(row_stride >= K0, "vx_sam_iou_head_f32: row stride %lld below the token width %d", (long long)row_stride, K0);
    hipLaunchKernelGGL(sam_iou_head_kernel, dim3((unsigned)P), dim3(256), 0, as_stream(stream), reinterpret_cast<const f16*>(tokens), (long)row_stride, w0, b0, w1, b1, w2,
                       b2, K0, N0, N1, N2, iou, chosen);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_sam_process_masks(const void* planes, int64_t prompt_stride, int64_t plane_stride, int step, int mask_size, int n_planes, const int32_t* chosen,
                                    float* scaled, int image_size, int sw, int sh, uint8_t* out, int dw, int dh, int P, void* stream) {
    VX_REQUIRE(planes && chosen && scaled && out && P > 0 && P <= 65535, "vx_sam_process_masks: bad operands (1 .. 65535 prompts)");
    VX_REQUIRE(mask_size > 0 && n_planes > 0 && step > 0 && plane_stride > 0 && prompt_stride > 0 && image_size > 0, "vx_sam_process_masks: bad plane layout");
    VX_REQUIRE(sw > 0 && sh > 0 && sw <= image_size && sh <= image_size && dw > 0 && dh > 0, "vx_sam_process_masks: crop %d x %d of a %d^2 map, target %d x %d", sw, sh,
               image_size, dw, dh);
    VX_REQUIRE((long)image_size * image_size <= (1L << 31) - 256 && (long)dw * dh <= (1L << 31) - 256, "vx_sam_process_masks: map too large"); // the last block's thread index stays an int
    hipLaunchKernelGGL(sam_masks_upscale_kernel, dim3(blocks_for((long)image_size * image_size), (unsigned)P), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const f16*>(planes), (long)prompt_stride, (long)plane_stride, step, mask_size, chosen, n_planes, scaled, image_size);
    VX_LAUNCH_CHECK();
    hipLaunchKernelGGL(sam_masks_crop_kernel, dim3(blocks_for((long)dw * dh), (unsigned)P), dim3(256), 0, as_stream(stream), scaled, image_size, sw, sh, out, dw, dh);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_sam_tile_rows_f16(const void* src, int64_t n, void* dst, int B, void* stream) {
    VX_REQUIRE(src && dst && n > 0 && n % 8 == 0 && B > 0 && B <= 65535, "vx_sam_tile_rows_f16: n a positive multiple of 8, 1 .. 65535 copies");
    VX_REQUIRE(aligned16(src) && aligned16(dst), "vx_sam_tile_rows_f16: operands must be 16-byte aligned");
    VX_REQUIRE((n / 8 + 255) / 256 < (1L << 31), "vx_sam_tile_rows_f16: too many blocks");
    hipLaunchKernelGGL(sam_tile_rows_kernel, dim3(blocks_for(n / 8), (unsigned)B), dim3(256), 0, as_stream(stream), reinterpret_cast<const f16x8*>(src),
                       reinterpret_cast<f16x8*>(dst), (long)(n / 8));
    VX_LAUNCH_CHECK();
    return 1;
}
