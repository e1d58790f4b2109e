// SAM's mask-input prompt (PromptEncoder._embed_masks) fused with the decoder's first add: one kernel from a prompt's low-resolution logits to the two
// image-side operands of the decoder's first layer.
//   vx_sam_dense_prompt_f16   mask f32 [n][4 res][4 res] -> conv 2x2 s2 (1 -> 4), LayerNorm2d, GELU, conv 2x2 s2 (4 -> 16), LayerNorm2d, GELU, conv 1x1 (16 -> dim),
//                             + image embedding -> K f16 [n][res^2][dim], and k1 = K + dense positional embedding
//   vx_sam_gather_plane_f32   plane chosen[p] of each prompt's f16 logits as f32: the low_res_logits a caller feeds back as the next mask input
//   vx_sam_fix_plane_i32      chosen[p] = plane: a caller's fixed plane in place of the iou head's choice
//
// The dense prompt. An output pixel depends on one 4 x 4 patch of its prompt's mask and on nothing else, so a pixel never leaves its lane's registers until the last
// product: no LDS, no scratch, no barrier. One wave (= one block) owns tiles of 16 consecutive output rows (row = prompt * res^2 + pixel). Lane l = 16 g + p works on
// row p of the tile, as one of the four lanes (g = 0 .. 3) of that row:
//   load     the patch, four 16-byte loads (the four lanes of a row ask for the same addresses: one fetch)
//   stage 1  4 positions x 4 channels, 64 MACs, LayerNorm over the 4 channels of a position, erf GELU: computed by all four lanes of the row alike (f32)
//   stage 2  lane g computes channels 4 g .. 4 g + 3 of the 16: 64 MACs with its own 64 weights, held in registers for the whole kernel. The LayerNorm over the
//            16 channels is two butterflies over the row's four lanes (__shfl_xor 16, 32): the mean, then the mean of the squared distances from it (f32)
//   product  the four activations, rounded to f16 once, ARE the lane's slice of v_mfma_f32_16x16x16_f16's B operand (k = 4 g .. 4 g + 3, column = row p). The A
//            operand is a 16-channel tile of the 1x1 conv's weight, [channel][k]: every tile's fragment (2 VGPRs) stays in registers for the whole kernel, up to
//            16 tiles (dim 256, the 8 KB weight, 32 VGPRs); wider maps run the channel groups of 256 on blockIdx.y. The product is the transposed one, D[channel][row],
//            so a lane's four accumulators are channels 16 t + 4 g .. + 3 of row p: the bias, the embedding and the positional embedding are read, and K and k1
//            stored, as four consecutive channels (8 bytes of f16, 16 bytes of an f32 embedding)
// Rows at and behind n res^2 compute on a zero patch (the butterflies need every lane) and neither read nor store anything.
// Roundings: stage-2 activations to f16 (the MFMA operand), K to f16, and k1 = f16(K as stored + pe). Everything before is f32; the 1x1 weight is f16 as packed.
#include "vx_common.h"

namespace {

constexpr int SD_MAX_TILES = 16; // channel tiles of 16 whose weight fragments a wave keeps: 256 channels per blockIdx.y

struct sam_dense_params {
    const float* mask; long mask_prompt_stride; int mask_row_stride; // elements
    const float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2;            // stage 1: [4][1][2][2], [4] x 3; stage 2: [16][4][2][2], [16] x 3
    const f16* w3; const float* b3;                                  // [dim][16], [dim]
    const void* embed; const f16* pe;                                // [res^2][dim] f16 or f32; pe nullable
    f16 *K, *k1;                                                     // [n][res^2][dim]
    long rows;                                                       // n res^2
    int res, dim;
    float eps;
};

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

template <bool EMBED_F32>
__global__ __launch_bounds__(64) void sam_dense_prompt_kernel(sam_dense_params p) {
    const int lane = threadIdx.x, g = lane >> 4, col = lane & 15;
    const int ch0 = blockIdx.y * (SD_MAX_TILES * 16);
    const int n_tiles = min(SD_MAX_TILES, (p.dim - ch0) / 16);

    // ---- what the wave keeps for all its tiles: the 1x1 conv's fragments, this lane's stage-2 weights and the small tables
    f16x4 wf[SD_MAX_TILES];
#pragma unroll
    for (int t = 0; t < SD_MAX_TILES; ++t) {
        wf[t] = f16x4{0, 0, 0, 0};
        if (t < n_tiles) wf[t] = *reinterpret_cast<const f16x4*>(p.w3 + (long)(ch0 + t * 16 + col) * 16 + 4 * g);
    }
    float w2[4][16], b2[4], g2[4], be2[4]; // [own channel][c1 * 4 + ky * 2 + kx]
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int i = 0; i < 16; ++i) w2[c][i] = p.w2[(4 * g + c) * 16 + i];
        b2[c] = p.b2[4 * g + c];
        g2[c] = p.g2[4 * g + c];
        be2[c] = p.be2[4 * g + c];
    }
    float w1[4][4], b1[4], g1[4], be1[4]; // [channel][ky * 2 + kx]: wave-uniform
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) w1[c][i] = p.w1[c * 4 + i];
        b1[c] = p.b1[c];
        g1[c] = p.g1[c];
        be1[c] = p.be1[c];
    }

    const long px_per_prompt = (long)p.res * p.res;
    const long n_row_tiles = (p.rows + 15) / 16;
    for (long tile = blockIdx.x; tile < n_row_tiles; tile += gridDim.x) {
        const long row = tile * 16 + col;
        const bool live = row < p.rows;
        float patch[4][4] = {};
        if (live) {
            const long b = row / px_per_prompt;
            const int pix = (int)(row - b * px_per_prompt), y = pix / p.res, x = pix - y * p.res;
            const float* src = p.mask + b * p.mask_prompt_stride + (long)(4 * y) * p.mask_row_stride + 4 * x;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(src + (long)r * p.mask_row_stride);
                patch[r][0] = v[0]; patch[r][1] = v[1]; patch[r][2] = v[2]; patch[r][3] = v[3];
            }
        }
        // stage 1: position (py, px) of the 2 x 2 map, channels 0 .. 3 -> s1[c * 4 + py * 2 + px], the order of stage 2's weights
        float s1[16];
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px) {
                float a[4], mean = 0.0f, var = 0.0f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    a[c] = b1[c];
#pragma unroll
                    for (int ky = 0; ky < 2; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 2; ++kx) a[c] = fmaf(w1[c][ky * 2 + kx], patch[2 * py + ky][2 * px + kx], a[c]);
                    mean += a[c];
                }
                mean *= 0.25f;
#pragma unroll
                for (int c = 0; c < 4; ++c) var = fmaf(a[c] - mean, a[c] - mean, var);
                const float rstd = 1.0f / sqrtf(var * 0.25f + p.eps);
#pragma unroll
                for (int c = 0; c < 4; ++c) s1[c * 4 + py * 2 + px] = gelu_erf(fmaf((a[c] - mean) * rstd, g1[c], be1[c]));
            }
        // stage 2: this lane's four of the sixteen channels; the LayerNorm's sums cross the row's four lanes
        float a2[4], part = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            a2[c] = b2[c];
#pragma unroll
            for (int i = 0; i < 16; ++i) a2[c] = fmaf(w2[c][i], s1[i], a2[c]);
            part += a2[c];
        }
        part += __shfl_xor(part, 16, 64);
        part += __shfl_xor(part, 32, 64);
        const float mean2 = part * 0.0625f;
        float sq = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) sq = fmaf(a2[c] - mean2, a2[c] - mean2, sq);
        sq += __shfl_xor(sq, 16, 64);
        sq += __shfl_xor(sq, 32, 64);
        const float rstd2 = 1.0f / sqrtf(sq * 0.0625f + p.eps);
        f16x4 act;
#pragma unroll
        for (int c = 0; c < 4; ++c) act[c] = (f16)gelu_erf(fmaf((a2[c] - mean2) * rstd2, g2[c], be2[c]));

        // the 1x1 conv, transposed: D[channel 16 t + 4 g + r][row col]; then bias + embedding, K, and k1 = K + pe
        const long pix_off = (row % px_per_prompt) * p.dim;
#pragma unroll
        for (int t = 0; t < SD_MAX_TILES; ++t) {
            if (t >= n_tiles) continue; // wave-uniform
            const f32x4 d = __builtin_amdgcn_mfma_f32_16x16x16f16(wf[t], act, f32x4{0, 0, 0, 0}, 0, 0, 0);
            if (!live) continue; // a row behind the end: nothing read, nothing stored
            const int ch = ch0 + t * 16 + 4 * g;
            const f32x4 bias = *reinterpret_cast<const f32x4*>(p.b3 + ch);
            f32x4 e;
            if (EMBED_F32) e = *reinterpret_cast<const f32x4*>(static_cast<const float*>(p.embed) + pix_off + ch);
            else {
                const f16x4 eh = *reinterpret_cast<const f16x4*>(static_cast<const f16*>(p.embed) + pix_off + ch);
                e = f32x4{(float)eh[0], (float)eh[1], (float)eh[2], (float)eh[3]};
            }
            f16x4 k;
#pragma unroll
            for (int r = 0; r < 4; ++r) k[r] = (f16)((d[r] + bias[r]) + e[r]);
            *reinterpret_cast<f16x4*>(p.K + row * p.dim + ch) = k;
            if (p.pe) {
                const f16x4 pe = *reinterpret_cast<const f16x4*>(p.pe + pix_off + ch);
                f16x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (f16)((float)k[r] + (float)pe[r]);
                *reinterpret_cast<f16x4*>(p.k1 + row * p.dim + ch) = o;
            }
        }
    }
}

__global__ __launch_bounds__(256) void sam_gather_plane_kernel(const f16* __restrict__ planes, long prompt_stride, long plane_stride, long n_px, int n_planes,
                                                               const int* __restrict__ chosen, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (i >= n_px) return;
    const int c = min(max(chosen[p], 0), n_planes - 1); // as vx_sam_process_masks: a value outside the planes reads the nearest one
    out[p * n_px + i] = (float)planes[p * prompt_stride + c * plane_stride + i];
}

__global__ __launch_bounds__(256) void sam_fix_plane_kernel(int* __restrict__ chosen, int plane, int P) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < P) chosen[i] = plane;
}

} // namespace

extern "C" int vx_sam_dense_prompt_f16(const float* mask, int64_t mask_prompt_stride, int mask_row_stride, const float* w1, const float* b1, const float* ln1_w,
                                       const float* ln1_b, int c1, const float* w2, const float* b2, const float* ln2_w, const float* ln2_b, int c2, const void* w3,
                                       const float* b3, const void* embed, int embed_is_f32, const void* pe, void* K, void* k1, int n, int res, int dim, float eps,
                                       void* stream) {
    VX_REQUIRE(mask && w1 && b1 && ln1_w && ln1_b && w2 && b2 && ln2_w && ln2_b && w3 && b3 && embed && K, "vx_sam_dense_prompt_f16: null operand");
    VX_REQUIRE(c1 == 4 && c2 == 16, "vx_sam_dense_prompt_f16: mask_downscaling widths %d -> %d (built for 4 -> 16: one 16x16x16 MFMA step per tile)", c1, c2);
    VX_REQUIRE(n > 0 && res > 0 && res <= 4096 && dim > 0 && dim % 16 == 0, "vx_sam_dense_prompt_f16: n = %d, res = %d, dim = %d (dim a multiple of 16)", n, res, dim);
    VX_REQUIRE((pe == nullptr) == (k1 == nullptr), "vx_sam_dense_prompt_f16: pe and k1 come together");
    VX_REQUIRE(mask_row_stride >= 4 * res && mask_row_stride % 4 == 0 && mask_prompt_stride >= (int64_t)mask_row_stride * 4 * res && mask_prompt_stride % 4 == 0,
               "vx_sam_dense_prompt_f16: mask strides %d / %lld for a %d^2 mask (multiples of 4, rows and prompts apart)", mask_row_stride,
               (long long)mask_prompt_stride, 4 * res);
    VX_REQUIRE(aligned16(mask) && aligned16(b3) && aligned16(embed) && (reinterpret_cast<uintptr_t>(w3) & 7) == 0 && (reinterpret_cast<uintptr_t>(K) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(pe) & 7) == 0 && (reinterpret_cast<uintptr_t>(k1) & 7) == 0,
               "vx_sam_dense_prompt_f16: mask, b3 and the embedding must be 16-byte aligned, w3, pe, K and k1 8-byte aligned");
    sam_dense_params p;
    p.mask = mask; p.mask_prompt_stride = (long)mask_prompt_stride; p.mask_row_stride = mask_row_stride;
    p.w1 = w1; p.b1 = b1; p.g1 = ln1_w; p.be1 = ln1_b; p.w2 = w2; p.b2 = b2; p.g2 = ln2_w; p.be2 = ln2_b;
    p.w3 = reinterpret_cast<const f16*>(w3); p.b3 = b3;
    p.embed = embed; p.pe = reinterpret_cast<const f16*>(pe);
    p.K = reinterpret_cast<f16*>(K); p.k1 = reinterpret_cast<f16*>(k1);
    p.rows = (long)n * res * res;
    p.res = res; p.dim = dim; p.eps = eps;
    const long row_tiles = (p.rows + 15) / 16;
    const dim3 grid((unsigned)(row_tiles < 2048 ? row_tiles : 2048), (unsigned)((dim + SD_MAX_TILES * 16 - 1) / (SD_MAX_TILES * 16))); // 8 waves per CU at most
    if (embed_is_f32) hipLaunchKernelGGL(sam_dense_prompt_kernel<true>, grid, dim3(64), 0, as_stream(stream), p);
    else hipLaunchKernelGGL(sam_dense_prompt_kernel<false>, grid, dim3(64), 0, as_stream(stream), p);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_sam_gather_plane_f32(const void* planes, int64_t prompt_stride, int64_t plane_stride, int64_t n_px, int n_planes, const int32_t* chosen, float* out,
                                       int P, void* stream) {
    VX_REQUIRE(planes && chosen && out && P > 0 && P <= 65535, "vx_sam_gather_plane_f32: bad operands (1 .. 65535 prompts)");
    VX_REQUIRE(n_px > 0 && n_px <= (1L << 31) - 256 && n_planes > 0 && plane_stride >= n_px && prompt_stride >= plane_stride * n_planes,
               "vx_sam_gather_plane_f32: bad plane layout (%lld logits, %d planes %lld apart, prompts %lld apart)", (long long)n_px, n_planes, (long long)plane_stride,
               (long long)prompt_stride);
    hipLaunchKernelGGL(sam_gather_plane_kernel, dim3(blocks_for(n_px), (unsigned)P), dim3(256), 0, as_stream(stream), reinterpret_cast<const f16*>(planes),
                       (long)prompt_stride, (long)plane_stride, (long)n_px, n_planes, chosen, out);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_sam_fix_plane_i32(int32_t* chosen, int plane, int P, void* stream) {
    VX_REQUIRE(chosen && P > 0 && plane >= 0, "vx_sam_fix_plane_i32: bad operands");
    hipLaunchKernelGGL(sam_fix_plane_kernel, dim3(blocks_for(P)), dim3(256), 0, as_stream(stream), chosen, plane, P);
    VX_LAUNCH_CHECK();
    return 1;
}
