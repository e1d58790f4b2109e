// The graph layer's image ops and pixel gates for BiRefNet written against it (birefnet.cpp:20-73, 147-260) on gfx950. All of them are memory-bound
// passes without atomics: the same bits on every launch.
//
//  * image_bilinear_ac      bilinear | align_corners resize of an f32 image [N, H, W, C <= 4] (downscale_by of the input image, birefnet.cpp:36-41)
//  * image_patches          image_to_patches (birefnet.cpp:153-162) of an f32 image as an f16 map: the naive form, and the form that walks image rows
//  * pixel_gate             p * sigmoid(conv 1x1 to one channel) per pixel (the gdt gate, birefnet.cpp:189-192)
//  * bilinear_ac_pix        vx_bilinear_ac_f16 (kernels_misc.hip) with pixel strides on both sides: a resize that writes its slice of a concat's buffer
//  * layernorm_pix          LayerNorm of f16 rows with an output row stride: swin_encode's last norms write their slice of encode_concat's buffers
#include "vx_common.h"

namespace {

constexpr int GRID_CAP = 256 * 64; // at most 64 blocks per CU, grid-stride beyond

// One thread per output element. The source coordinate is o * (in - 1) / (out - 1), the factor made on the host (0 where out is 1); both taps are
// clamped; horizontal lerp, then vertical: the arithmetic of bf_preprocess_half_kernel (kernels_birefnet.hip).
__global__ __launch_bounds__(256) void image_bilinear_ac_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int C, int OH, int OW, float sy, float sx, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C);
        long p = i / C;
        const int ox = (int)(p % OW);
        p /= OW;
        const int oy = (int)(p % OH);
        const long b = p / OH;
        const float fy = (float)oy * sy, fx = (float)ox * sx;
        int y0 = (int)fy, x0 = (int)fx;
        if (y0 > H - 1) y0 = H - 1;
        if (x0 > W - 1) x0 = W - 1;
        const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
        const float ty = fy - (float)y0, tx = fx - (float)x0;
        const float* s = x + b * (long)H * W * C + c;
        const float v00 = s[((long)y0 * W + x0) * C], v01 = s[((long)y0 * W + x1) * C], v10 = s[((long)y1 * W + x0) * C], v11 = s[((long)y1 * W + x1) * C];
        const float top = v00 + (v01 - v00) * tx, bot = v10 + (v11 - v10) * tx;
        y[i] = top + (bot - top) * ty;
    }
}

// image_to_patches, naive form: one thread per 8 output channels. Channel ch = gx + gw (gy + gh c) of pixel (py, px) is image (gy h + py, gx w + px, c), so
// the eight loads of a thread are w pixels apart and the loads of a wave touch 64 different lines each. Kept to be measured against (tools/bench_birefnet_graph.py).
__global__ __launch_bounds__(256) void image_patches_naive_kernel(const float* __restrict__ x, f16* __restrict__ y, int IH, int IW, int C, int h, int w, long n8) {
    const int gw = IW / w, gh = IH / h, CP = gw * gh * C, c8 = CP / 8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        const int ch0 = (int)(i % c8) * 8;
        const long pix = i / c8;
        const int px = (int)(pix % w), py = (int)((pix / w) % h);
        const long b = pix / ((long)w * h);
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ch = ch0 + j, gx = ch % gw, gy = (ch / gw) % gh, c = ch / (gw * gh);
            o[j] = (f16)x[((b * IH + (long)gy * h + py) * IW + (long)gx * w + px) * C + c];
        }
        *reinterpret_cast<f16x8*>(y + pix * CP + ch0) = o;
    }
}

// image_to_patches through LDS: a block makes TP consecutive pixels of one output row. It reads, for every (gy, gx), the TP * C consecutive floats of image row
// gy h + py that those pixels come from -- consecutive lanes read consecutive floats -- and stores them, rounded to f16, where the output wants them: LDS holds the
// TP output pixels as they will lie in memory, each padded by 8 halves so that neighbouring pixels start 4 banks apart. Then the block writes those TP * CP halves,
// which are contiguous in the output, 16 bytes per lane.
__global__ __launch_bounds__(256) void image_patches_rows_kernel(const float* __restrict__ x, f16* __restrict__ y, int IH, int IW, int C, int h, int w, int TP) {
    extern __shared__ __attribute__((aligned(16))) f16 tile[];
    const int gw = IW / w, gh = IH / h, CP = gw * gh * C, CPp = CP + 8;
    const int tiles = (w + TP - 1) / TP;
    const int px0 = (int)(blockIdx.x % tiles) * TP, py = (int)((blockIdx.x / tiles) % h);
    const long b = blockIdx.x / ((long)tiles * h);
    const int valid = min(TP, w - px0), seg = valid * C, total = gw * gh * seg;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int s = e / seg, r = e - s * seg, gy = s / gw, gx = s - gy * gw, pl = r / C, c = r - pl * C;
        const float v = x[((b * IH + (long)gy * h + py) * IW + (long)gx * w + px0) * C + r];
        tile[pl * CPp + gx + gw * (gy + gh * c)] = (f16)v;
    }
    __syncthreads();
    const int c8 = CP / 8;
    f16* out = y + ((b * h + py) * (long)w + px0) * CP;
    for (int e = threadIdx.x; e < valid * c8; e += 256) {
        const int pl = e / c8, k = e - pl * c8;
        *reinterpret_cast<f16x8*>(out + (long)pl * CP + k * 8) = *reinterpret_cast<const f16x8*>(tile + pl * CPp + k * 8);
    }
}

// y[p, 0:C] = p[p, 0:C] * f16(sigmoid(bias + sum_k a[p, k] w[k])): one thread per 8 channels of p; every thread of a pixel sums the pixel's Cg gate channels
// itself (f32, k ascending; the row is a few cache lines that the pixel's threads share). g is rounded to f16 before the product, as bf_mul_sigmoid_kernel's
// operand is one (the per-node graph stores it as f16 too).
__global__ __launch_bounds__(256) void pixel_gate_kernel(const f16* __restrict__ p, long ldp, const f16* __restrict__ a, long lda, const float* __restrict__ w, float bias,
                                                         f16* __restrict__ y, long ldy, int C8, int Cg8, long n8) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        const int k = (int)(i % C8);
        const long row = i / C8;
        const f16* ar = a + row * lda;
        float s = 0.0f;
        for (int q = 0; q < Cg8; ++q) {
            const f16x8 av = *reinterpret_cast<const f16x8*>(ar + q * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += (float)av[j] * w[q * 8 + j];
        }
        const float g = (float)(f16)(1.0f / (1.0f + __expf(-(s + bias))));
        const f16x8 v = *reinterpret_cast<const f16x8*>(p + row * ldp + k * 8);
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)((float)v[j] * g);
        *reinterpret_cast<f16x8*>(y + row * ldy + k * 8) = o;
    }
}

// bilinear_ac_kernel of kernels_misc.hip, its arithmetic to the letter, with x_pix / y_pix elements between the pixels of source and destination
__global__ __launch_bounds__(256) void bilinear_ac_pix_kernel(const f16* __restrict__ x, long x_pix, f16* __restrict__ y, long y_pix, int H, int W, int c8n, int OH, int OW, float sfy,
                                                              float sfx) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= OW * c8n) return;
    const int ox = t / c8n, c8 = t - ox * c8n;
    const int oy = blockIdx.y, b = blockIdx.z;
    const float sy = (float)oy / sfy, sx = (float)ox / sfx;
    int y0 = (int)floorf(sy), x0 = (int)floorf(sx);
    int y1 = y0 + 1, x1 = x0 + 1;
    y0 = max(0, min(y0, H - 1)); y1 = max(0, min(y1, H - 1));
    x0 = max(0, min(x0, W - 1)); x1 = max(0, min(x1, W - 1));
    const float dy = fminf(fmaxf(sy - (float)y0, 0.0f), 1.0f), dx = fminf(fmaxf(sx - (float)x0, 0.0f), 1.0f);
    const f16* base = x + (long)b * H * W * x_pix + c8 * 8;
    const f16x8 a = *reinterpret_cast<const f16x8*>(base + ((long)y0 * W + x0) * x_pix);
    const f16x8 bb = *reinterpret_cast<const f16x8*>(base + ((long)y0 * W + x1) * x_pix);
    const f16x8 c = *reinterpret_cast<const f16x8*>(base + ((long)y1 * W + x0) * x_pix);
    const f16x8 d = *reinterpret_cast<const f16x8*>(base + ((long)y1 * W + x1) * x_pix);
    const float w00 = (1 - dx) * (1 - dy), w01 = dx * (1 - dy), w10 = (1 - dx) * dy, w11 = dx * dy;
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        o[j] = (f16)((float)a[j] * w00 + (float)bb[j] * w01 + (float)c[j] * w10 + (float)d[j] * w11);
    *reinterpret_cast<f16x8*>(y + (((long)b * OH + oy) * OW + ox) * y_pix + c8 * 8) = o;
}

// LayerNorm of contiguous f16 rows, written y_pix elements apart: LANES lanes per row (a wave holds 64 / LANES rows), a lane holds CHUNKS chunks of 8 channels,
// chunk `lane + LANES q`. Mean, then the mean of the squared deviations (two passes over registers), both summed across the row's lanes by butterflies: every lane of
// a row ends with the same f32 sums. The launcher picks the narrowest form that covers C, so that rows of few channels do not leave most of a wave idle.
template <int LANES, int CHUNKS>
__global__ __launch_bounds__(256) void layernorm_pix_kernel(const f16* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, f16* __restrict__ y, long y_pix, long rows,
                                                            int C, float eps) {
    const long row = ((long)blockIdx.x * 256 + threadIdx.x) / LANES;
    if (row >= rows) return; // (the lanes of a row leave together, and no barrier follows)
    const int lane = threadIdx.x % LANES, c8 = C / 8;
    float v[CHUNKS][8];
    float s = 0.0f;
#pragma unroll
    for (int q = 0; q < CHUNKS; ++q) {
        const int k = lane + LANES * q;
        f16x8 in = {0, 0, 0, 0, 0, 0, 0, 0};
        if (k < c8) in = *reinterpret_cast<const f16x8*>(x + row * C + k * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) { v[q][j] = (float)in[j]; s += v[q][j]; }
    }
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / (float)C;
    float d2 = 0.0f;
#pragma unroll
    for (int q = 0; q < CHUNKS; ++q)
        if (lane + LANES * q < c8)
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float d = v[q][j] - mean; d2 += d * d; }
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) d2 += __shfl_xor(d2, o, 64);
    const float rstd = 1.0f / sqrtf(d2 / (float)C + eps);
#pragma unroll
    for (int q = 0; q < CHUNKS; ++q) {
        const int k = lane + LANES * q;
        if (k >= c8) continue;
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)((v[q][j] - mean) * rstd * w[k * 8 + j] + b[k * 8 + j]);
        *reinterpret_cast<f16x8*>(y + row * y_pix + k * 8) = o;
    }
}

} // namespace

extern "C" {

int vx_layernorm_pix_f16(const void* x, const float* w, const float* b, void* y, int64_t y_pix, int64_t rows, int C, float eps, void* stream) {
    VX_REQUIRE(x && w && b && y && rows > 0 && C > 0 && C <= 1024 && C % 8 == 0, "vx_layernorm_pix_f16: bad operands (C = %d: a multiple of 8, at most 1024)", C);
    VX_REQUIRE(y_pix >= C && y_pix % 8 == 0 && aligned16(x) && aligned16(y), "vx_layernorm_pix_f16: output rows %ld elements apart (a multiple of 8, at least C = %d; operands 16-byte aligned)",
               (long)y_pix, C);
    const f16* xp = reinterpret_cast<const f16*>(x);
    f16* yp = reinterpret_cast<f16*>(y);
    hipStream_t s = as_stream(stream);
    if (C <= 64) hipLaunchKernelGGL((layernorm_pix_kernel<8, 1>), dim3(blocks_for((long)rows, 32)), dim3(256), 0, s, xp, w, b, yp, (long)y_pix, (long)rows, C, eps);
    else if (C <= 128) hipLaunchKernelGGL((layernorm_pix_kernel<16, 1>), dim3(blocks_for((long)rows, 16)), dim3(256), 0, s, xp, w, b, yp, (long)y_pix, (long)rows, C, eps);
    else if (C <= 256) hipLaunchKernelGGL((layernorm_pix_kernel<32, 1>), dim3(blocks_for((long)rows, 8)), dim3(256), 0, s, xp, w, b, yp, (long)y_pix, (long)rows, C, eps);
    else if (C <= 512) hipLaunchKernelGGL((layernorm_pix_kernel<64, 1>), dim3(blocks_for((long)rows, 4)), dim3(256), 0, s, xp, w, b, yp, (long)y_pix, (long)rows, C, eps);
    else hipLaunchKernelGGL((layernorm_pix_kernel<64, 2>), dim3(blocks_for((long)rows, 4)), dim3(256), 0, s, xp, w, b, yp, (long)y_pix, (long)rows, C, eps);
    VX_LAUNCH_CHECK();
    return 1;
}

int vx_image_bilinear_ac_f32(const float* x, float* y, int B, int H, int W, int C, int OH, int OW, void* stream) {
    VX_REQUIRE(x && y, "vx_image_bilinear_ac_f32: null operand");
    VX_REQUIRE(B > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "vx_image_bilinear_ac_f32: empty extent");
    VX_REQUIRE(C >= 1 && C <= 4, "vx_image_bilinear_ac_f32: C = %d; an image has 1..4 channels", C);
    const float sy = OH > 1 ? (float)(H - 1) / (float)(OH - 1) : 0.0f, sx = OW > 1 ? (float)(W - 1) / (float)(OW - 1) : 0.0f;
    const long n = (long)B * OH * OW * C;
    hipLaunchKernelGGL(image_bilinear_ac_kernel, dim3(grid_stride_blocks(n, GRID_CAP)), dim3(256), 0, as_stream(stream), x, y, H, W, C, OH, OW, sy, sx, n);
    VX_LAUNCH_CHECK();
    return 1;
}

int vx_image_patches_tile(int channels) { // output pixels per block of the row-walking form: the largest power of two whose tile fits 56 KiB of LDS (below the 64 KiB a launch gets without an attribute), at most 64; 0: none fits
    int tp = 64;
    while (tp > 0 && (long)tp * (channels + 8) * 2 > 56 * 1024) tp /= 2;
    return tp;
}

int vx_image_patches_f16(const float* x, void* y, int B, int IH, int IW, int C, int h, int w, int form, void* stream) {
    VX_REQUIRE(x && y && B > 0 && IH > 0 && IW > 0 && h > 0 && w > 0, "vx_image_patches_f16: bad operands");
    VX_REQUIRE(C >= 1 && C <= 4, "vx_image_patches_f16: C = %d; an image has 1..4 channels", C);
    VX_REQUIRE(IW % w == 0 && IH % h == 0, "vx_image_patches_f16: Grid must divide image size (image %dx%d, patches %dx%d)", IW, IH, w, h);
    const long CP = (long)(IW / w) * (IH / h) * C;
    VX_REQUIRE(CP % 8 == 0 && CP < (1L << 24), "vx_image_patches_f16: %ld channels (grid %dx%d x %d; a multiple of 8)", CP, IW / w, IH / h, C);
    VX_REQUIRE(aligned16(y), "vx_image_patches_f16: the output must be 16-byte aligned");
    VX_REQUIRE(form >= 0 && form <= 2, "vx_image_patches_f16: form %d (0 chosen by shape, 1 naive, 2 image rows through LDS)", form);
    const int tp = vx_image_patches_tile((int)CP);
    const long blocks = (long)B * h * ((w + (tp > 0 ? tp : 1) - 1) / (tp > 0 ? tp : 1));
    VX_REQUIRE(form != 2 || (tp > 0 && blocks < (1L << 31)), "vx_image_patches_f16: %ld channels do not fit the LDS tile of the row form", CP);
    // form 0: the row form where it was measured faster (tools/bench_birefnet_graph.py: 72 against 121 us at 3072 channels, a tie at 768, 69 against 57 us at 192 and
    // 48, where a thread's eight loads fall into few image rows) -- tiles below 32 pixels, that is more than 888 channels
    if (form == 2 || (form == 0 && tp > 0 && tp < 32 && blocks < (1L << 31))) {
        hipLaunchKernelGGL(image_patches_rows_kernel, dim3((unsigned)blocks), dim3(256), (size_t)tp * (CP + 8) * 2, as_stream(stream), x, reinterpret_cast<f16*>(y), IH, IW, C, h, w, tp);
    } else {
        const long n8 = (long)B * h * w * (CP / 8);
        hipLaunchKernelGGL(image_patches_naive_kernel, dim3(grid_stride_blocks(n8, GRID_CAP)), dim3(256), 0, as_stream(stream), x, reinterpret_cast<f16*>(y), IH, IW, C, h, w, n8);
    }
    VX_LAUNCH_CHECK();
    return 1;
}

int vx_pixel_gate_f16(const void* p, int64_t ldp, const void* a, int64_t lda, const float* w, float bias, void* y, int64_t ldy, int64_t rows, int C, int Cg, void* stream) {
    VX_REQUIRE(p && a && w && y && rows > 0, "vx_pixel_gate_f16: bad operands");
    VX_REQUIRE(C > 0 && C % 8 == 0 && Cg > 0 && Cg % 8 == 0, "vx_pixel_gate_f16: C = %d, Cg = %d (multiples of 8)", C, Cg);
    VX_REQUIRE(ldp >= C && ldy >= C && lda >= Cg && ldp % 8 == 0 && ldy % 8 == 0 && lda % 8 == 0 && aligned16(p) && aligned16(a) && aligned16(y),
               "vx_pixel_gate_f16: leading dimensions %ld / %ld / %ld (multiples of 8, at least C = %d and Cg = %d; operands 16-byte aligned)", (long)ldp, (long)lda, (long)ldy, C, Cg);
    const long n8 = (long)rows * (C / 8);
    hipLaunchKernelGGL(pixel_gate_kernel, dim3(grid_stride_blocks(n8, GRID_CAP)), dim3(256), 0, as_stream(stream), reinterpret_cast<const f16*>(p), (long)ldp, reinterpret_cast<const f16*>(a),
                       (long)lda, w, bias, reinterpret_cast<f16*>(y), (long)ldy, C / 8, Cg / 8, n8);
    VX_LAUNCH_CHECK();
    return 1;
}

int vx_bilinear_ac_pix_f16(const void* x, int64_t x_pix, void* y, int64_t y_pix, int B, int H, int W, int C, int OH, int OW, void* stream) {
    VX_REQUIRE(x && y, "vx_bilinear_ac_pix_f16: null operand");
    VX_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && OH > 0 && OW > 0, "vx_bilinear_ac_pix_f16: empty extent");
    VX_REQUIRE(C % 8 == 0, "vx_bilinear_ac_pix_f16: C=%d must be a multiple of 8", C);
    VX_REQUIRE(x_pix >= C && y_pix >= C && x_pix % 8 == 0 && y_pix % 8 == 0 && aligned16(x) && aligned16(y),
               "vx_bilinear_ac_pix_f16: pixel strides %ld / %ld (multiples of 8, at least C = %d; operands 16-byte aligned)", (long)x_pix, (long)y_pix, C);
    VX_REQUIRE(OH <= 65535 && B <= 65535, "vx_bilinear_ac_pix_f16: %d rows x %d images do not fit the grid (65535 each)", OH, B);
    const float sfy = (OH > 1 && H > 1) ? (float)(OH - 1) / (float)(H - 1) : (float)OH / (float)H;
    const float sfx = (OW > 1 && W > 1) ? (float)(OW - 1) / (float)(W - 1) : (float)OW / (float)W;
    const int c8n = C / 8;
    hipLaunchKernelGGL(bilinear_ac_pix_kernel, dim3((OW * c8n + 255) / 256, OH, B), dim3(256), 0, as_stream(stream), reinterpret_cast<const f16*>(x), (long)x_pix, reinterpret_cast<f16*>(y),
                       (long)y_pix, H, W, c8n, OH, OW, sfy, sfx);
    VX_LAUNCH_CHECK();
    return 1;
}

} // extern "C"
