// 2D pooling, row softmax, the softmax expectation of a DFL box decode and row sums: the graph layer's VISP_OP_POOL_2D, VISP_OP_SOFT_MAX and
// VISP_OP_SUM_ROWS (ggml_pool_2d, ggml_soft_max, ggml_sum_rows as yolov9t.cpp:165-185, 449-483, 657-691 call them).
//
// pool_kernel has the shape of dwconv_kernel (kernels_dwconv.hip), templated on (k, stride, kind): one thread owns 8 channels x P consecutive output
// pixels of one row and loads, per kernel row, the (P - 1) S + K input pixels that feed all P outputs once, as 16-byte loads. Lanes run over the channel
// groups first. Input and output carry a pixel stride of their own, so the kernel reads a channel slice of a wider map and writes into a slice of a
// concat's buffer. Max is taken in f16 (exact: the maximum of f16 values is one of them), positions outside the map never win; average sums in f32
// and rounds once (no padding: the divisor is k * k). A strip's tail past OW is computed and not stored. No LDS, no scratch.
#include "vx_common.h"

namespace {

template <int K, int S, int KIND, int P>
__global__ __launch_bounds__(256) void pool_kernel(const f16* __restrict__ x, long x_pix, f16* __restrict__ y, long y_pix, int B, int H, int W, int C, int OH, int OW, int pad) {
    constexpr int NC = (P - 1) * S + K, ROWS_UNROLLED = K <= 3 ? K : 1;
    const int c8n = C >> 3, strips = (OW + P - 1) / P;
    const long n = (long)B * OH * strips * c8n;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c8 = (int)(i % c8n);
    long q = i / c8n;
    const int ox0 = (int)(q % strips) * P;
    q /= strips;
    const int oy = (int)(q % OH), b = (int)(q / OH);
    const f16 lowest = (f16)(-__builtin_huge_valf());
    f16x8 best[P];
    float acc[P][8];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        best[p] = f16x8{lowest, lowest, lowest, lowest, lowest, lowest, lowest, lowest};
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[p][j] = 0.0f;
    }
    const int ix0 = ox0 * S - pad;
#pragma unroll ROWS_UNROLLED
    for (int ky = 0; ky < K; ++ky) {
        const int iy = oy * S - pad + ky;
        if ((unsigned)iy >= (unsigned)H) continue;
        const f16* row = x + ((long)b * H + iy) * W * x_pix + c8 * 8;
        f16x8 col[NC];
#pragma unroll
        for (int t = 0; t < NC; ++t) {
            const int ix = ix0 + t;
            if ((unsigned)ix < (unsigned)W) col[t] = *reinterpret_cast<const f16x8*>(row + (long)ix * x_pix);
            else if (KIND == 0) col[t] = f16x8{lowest, lowest, lowest, lowest, lowest, lowest, lowest, lowest};
            else col[t] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                if (KIND == 0) best[p] = __builtin_elementwise_max(best[p], col[p * S + kx]);
                else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[p][j] += (float)col[p * S + kx][j];
                }
            }
    }
    f16* out = y + (((long)b * OH + oy) * OW + ox0) * y_pix + c8 * 8;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        if (ox0 + p >= OW) break;
        f16x8 o = best[p];
        if (KIND == 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (f16)(acc[p][j] * (1.0f / (float)(K * K)));
        }
        *reinterpret_cast<f16x8*>(out + (long)p * y_pix) = o;
    }
}

// output pixels per thread: 8 at stride 1 up to 5x5, 4 beyond and at stride 2 (the row segment stays at 19 pixels = 76 VGPRs at 13x13 / stride 2)
template <int K, int S>
constexpr int strip_of() { return S == 1 && K <= 5 ? 8 : 4; }

template <int K, int S>
void launch_pool(int kind, const f16* x, long x_pix, f16* y, long y_pix, int B, int H, int W, int C, int OH, int OW, int pad, hipStream_t st) {
    constexpr int P = strip_of<K, S>();
    const long n = (long)B * OH * ((OW + P - 1) / P) * (C / 8);
    if (kind == 0) hipLaunchKernelGGL((pool_kernel<K, S, 0, P>), dim3(blocks_for(n)), dim3(256), 0, st, x, x_pix, y, y_pix, B, H, W, C, OH, OW, pad);
    else hipLaunchKernelGGL((pool_kernel<K, S, 1, P>), dim3(blocks_for(n)), dim3(256), 0, st, x, x_pix, y, y_pix, B, H, W, C, OH, OW, pad);
}

// ---- softmax over rows of n f16 (n % 8 == 0, n <= 1024): f32 arithmetic, the row maximum subtracted, so logits at the f16 limit give neither inf nor NaN

// one wave per row: lane l holds the 8-element chunks l and l + 64
__global__ __launch_bounds__(256) void softmax_wave_kernel(const f16* __restrict__ x, long x_ld, f16* __restrict__ y, long y_ld, long rows, int n) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63, chunks = n >> 3;
    float v[2][8];
    float m = -__builtin_huge_valf();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = lane + h * 64;
        if (c < chunks) {
            const f16x8 t = *reinterpret_cast<const f16x8*>(x + r * x_ld + c * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) { v[h][j] = (float)t[j]; m = fmaxf(m, v[h][j]); }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[h][j] = -__builtin_huge_valf();
        }
    }
    m = wave_max(m);
    float s = 0.0f;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 8; ++j) { v[h][j] = __expf(v[h][j] - m); s += v[h][j]; } // exp(-inf) = 0 for the chunks that do not exist
    s = wave_sum(s);
    const float inv = 1.0f / s;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = lane + h * 64;
        if (c >= chunks) continue;
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)(v[h][j] * inv);
        *reinterpret_cast<f16x8*>(y + r * y_ld + c * 8) = o;
    }
}
// n = 8 or 16: one thread per row
template <int N8>
__global__ __launch_bounds__(256) void softmax_thread_kernel(const f16* __restrict__ x, long x_ld, f16* __restrict__ y, long y_ld, long rows) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float v[N8 * 8];
    float m = -__builtin_huge_valf();
#pragma unroll
    for (int c = 0; c < N8; ++c) {
        const f16x8 t = *reinterpret_cast<const f16x8*>(x + r * x_ld + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) { v[c * 8 + j] = (float)t[j]; m = fmaxf(m, v[c * 8 + j]); }
    }
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < N8 * 8; ++j) { v[j] = __expf(v[j] - m); s += v[j]; }
    const float inv = 1.0f / s;
#pragma unroll
    for (int c = 0; c < N8; ++c) {
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)(v[c * 8 + j] * inv);
        *reinterpret_cast<f16x8*>(y + r * y_ld + c * 8) = o;
    }
}

// y[r, g] = sum_i softmax(x[r, g n .. g n + n))_i * proj_i: the DFL decode (dfl_forward, yolov9t.cpp:657-691) in one pass over the box logits where they
// lie; one thread per (row, group), two passes over n <= 64 logits (the second one hits the cache)
__global__ __launch_bounds__(256) void softmax_expect_kernel(const f16* __restrict__ x, long x_ld, int group, const float* __restrict__ proj, f16* __restrict__ y, long rows, int n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * group) return;
    const long r = i / group;
    const int gi = (int)(i % group);
    const f16* p = x + r * x_ld + (long)gi * n;
    float m = -__builtin_huge_valf();
    for (int c = 0; c < n; c += 8) {
        const f16x8 t = *reinterpret_cast<const f16x8*>(p + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) m = fmaxf(m, (float)t[j]);
    }
    float s = 0.0f, e = 0.0f;
    for (int c = 0; c < n; c += 8) {
        const f16x8 t = *reinterpret_cast<const f16x8*>(p + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float w = __expf((float)t[j] - m);
            s += w;
            e = fmaf(w, proj[c + j], e);
        }
    }
    y[i] = (f16)(e / s);
}

// y[r] = sum of the n elements of row r, f32, left to right (one thread per row, scalar loads: not a hot-path kernel -- the fused DFL decode does not use it)
__global__ __launch_bounds__(256) void sum_rows_kernel(const f16* __restrict__ x, f16* __restrict__ y, long rows, int n) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const f16* p = x + r * n;
    float s = 0.0f;
    for (int c = 0; c < n; ++c) s += (float)p[c];
    y[r] = (f16)s;
}

} // namespace

extern "C" int vx_pool2d_f16(const void* x, int64_t x_pix, void* y, int64_t y_pix, int B, int H, int W, int C, int kind, int k, int stride, int pad, void* stream) {
    VX_REQUIRE(x && y && B > 0 && H > 0 && W > 0 && C > 0, "vx_pool2d_f16: bad operands");
    VX_REQUIRE(C % 8 == 0, "vx_pool2d_f16: C = %d must be a multiple of 8", C);
    VX_REQUIRE(kind == 0 || kind == 1, "vx_pool2d_f16: kind %d (0 max, 1 average)", kind);
    VX_REQUIRE(k >= 1 && k <= 13 && (stride == 1 || stride == 2), "vx_pool2d_f16: kernel %d, stride %d (kernels 1..13, stride 1 or 2)", k, stride);
    VX_REQUIRE(pad >= 0 && pad <= k / 2, "vx_pool2d_f16: pad %d with a %dx%d kernel (0 .. k / 2)", pad, k, k);
    VX_REQUIRE(kind == 0 || pad == 0, "vx_pool2d_f16: average pooling with padding is not built");
    VX_REQUIRE(x_pix >= C && y_pix >= C && x_pix % 8 == 0 && y_pix % 8 == 0, "vx_pool2d_f16: pixel strides %ld / %ld (multiples of 8, at least C = %d)", (long)x_pix, (long)y_pix, C);
    VX_REQUIRE(aligned16(x) && aligned16(y), "vx_pool2d_f16: operands must be 16-byte aligned");
    VX_REQUIRE(H + 2 * pad >= k && W + 2 * pad >= k, "vx_pool2d_f16: a %dx%d kernel at pad %d does not fit a %dx%d map", k, k, pad, W, H);
    const int OH = (H + 2 * pad - k) / stride + 1, OW = (W + 2 * pad - k) / stride + 1;
    const long blocks = ((long)B * OH * ((OW + 3) / 4) * (C / 8) + 255) / 256;
    VX_REQUIRE(blocks < (1L << 31), "vx_pool2d_f16: the map is too large for one launch");
    const f16* xp = reinterpret_cast<const f16*>(x);
    f16* yp = reinterpret_cast<f16*>(y);
    hipStream_t st = as_stream(stream);
#define VX_POOL(K_)                                                                                  \
    case K_:                                                                                         \
        if (stride == 1) launch_pool<K_, 1>(kind, xp, (long)x_pix, yp, (long)y_pix, B, H, W, C, OH, OW, pad, st); \
        else launch_pool<K_, 2>(kind, xp, (long)x_pix, yp, (long)y_pix, B, H, W, C, OH, OW, pad, st);             \
        break;
    switch (k) {
        VX_POOL(1) VX_POOL(2) VX_POOL(3) VX_POOL(4) VX_POOL(5) VX_POOL(6) VX_POOL(7) VX_POOL(8) VX_POOL(9) VX_POOL(10) VX_POOL(11) VX_POOL(12) VX_POOL(13)
    }
#undef VX_POOL
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_softmax_rows_f16(const void* x, int64_t x_ld, void* y, int64_t y_ld, int64_t rows, int n, void* stream) {
    VX_REQUIRE(x && y && rows > 0, "vx_softmax_rows_f16: bad operands");
    VX_REQUIRE(n >= 8 && n <= 1024 && n % 8 == 0, "vx_softmax_rows_f16: n = %d (a multiple of 8, at most 1024)", n);
    VX_REQUIRE(x_ld >= n && y_ld >= n && x_ld % 8 == 0 && y_ld % 8 == 0 && aligned16(x) && aligned16(y), "vx_softmax_rows_f16: row strides are multiples of 8 and at least n; operands 16-byte aligned");
    VX_REQUIRE(rows < (1L << 32), "vx_softmax_rows_f16: too many rows for one launch");
    hipStream_t st = as_stream(stream);
    const f16* xp = reinterpret_cast<const f16*>(x);
    f16* yp = reinterpret_cast<f16*>(y);
    if (n == 8) hipLaunchKernelGGL(softmax_thread_kernel<1>, dim3(blocks_for(rows)), dim3(256), 0, st, xp, (long)x_ld, yp, (long)y_ld, (long)rows);
    else if (n == 16) hipLaunchKernelGGL(softmax_thread_kernel<2>, dim3(blocks_for(rows)), dim3(256), 0, st, xp, (long)x_ld, yp, (long)y_ld, (long)rows);
    else hipLaunchKernelGGL(softmax_wave_kernel, dim3(blocks_for(rows, 4)), dim3(256), 0, st, xp, (long)x_ld, yp, (long)y_ld, (long)rows, n);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_softmax_expect_f16(const void* x, int64_t x_ld, int group, const float* proj, void* y, int64_t rows, int n, void* stream) {
    VX_REQUIRE(x && y && proj && rows > 0 && group > 0, "vx_softmax_expect_f16: bad operands");
    VX_REQUIRE(n >= 8 && n <= 64 && n % 8 == 0, "vx_softmax_expect_f16: n = %d (a multiple of 8, at most 64)", n);
    VX_REQUIRE(x_ld >= (int64_t)group * n && x_ld % 8 == 0 && aligned16(x), "vx_softmax_expect_f16: the row stride is a multiple of 8 and at least group * n; x 16-byte aligned");
    VX_REQUIRE(rows * group < (1L << 39), "vx_softmax_expect_f16: too many rows for one launch");
    hipLaunchKernelGGL(softmax_expect_kernel, dim3(blocks_for(rows * group)), dim3(256), 0, as_stream(stream), reinterpret_cast<const f16*>(x), (long)x_ld, group, proj,
                       reinterpret_cast<f16*>(y), (long)rows, n);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_sum_rows_f16(const void* x, void* y, int64_t rows, int n, void* stream) {
    VX_REQUIRE(x && y && rows > 0 && n > 0, "vx_sum_rows_f16: bad operands");
    VX_REQUIRE(rows < (1L << 39), "vx_sum_rows_f16: too many rows for one launch");
    hipLaunchKernelGGL(sum_rows_kernel, dim3(blocks_for(rows)), dim3(256), 0, as_stream(stream), reinterpret_cast<const f16*>(x), reinterpret_cast<f16*>(y), (long)rows, n);
    VX_LAUNCH_CHECK();
    return 1;
}
