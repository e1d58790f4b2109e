// The element-wise and small-product kernels of the SAM prompt encoder and mask decoder (mobile-sam.cpp:238-248, 471) for the graph layer:
//   vx_mul_mat_f16            ggml_mul_mat of two f16 activations, a [Ba][M][K], b [B][N][K] -> out [B][N][M] (out[b][n][m] = sum_k a[b % Ba.. ][m][k] b[b][n][k])
//   vx_sincos_f16             ggml_sin / ggml_cos, element-wise, f32 inside
//   vx_fourier_features_f32   position_embedding_random: f32 coordinates x the [2, F] gaussian matrix -> f16 sin | cos of 2 pi (x g0 + y g1)
#include "vx_common.h"

namespace {

constexpr int MM_MAX_K = 256, MM_MAX_N = 16;
constexpr float INV_2PI = 0.15915494309189533577f;

// One thread per row m of a. The N columns of b (zero-padded to a multiple of 4) sit in LDS as f16 and are read as broadcasts; the thread walks its row
// in 16-byte pieces once per group of four columns (N <= 4: once) with four f32 chains, k ascending. Plane n of the output is written by
// consecutive threads: coalesced.
__global__ __launch_bounds__(256) void mul_mat_kernel(const f16* __restrict__ A, const f16* __restrict__ Bm, f16* __restrict__ out, long M, int N, int K, int Ba) {
    __shared__ __attribute__((aligned(16))) f16 sb[MM_MAX_N * MM_MAX_K];
    const int b = blockIdx.y, n_pad = (N + 3) & ~3;
    const f16* bb = Bm + (long)b * N * K;
    for (int i = threadIdx.x; i < n_pad * K; i += 256) sb[i] = i < N * K ? bb[i] : (f16)0;
    __syncthreads();
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const f16* arow = A + ((long)(Ba == 1 ? 0 : b) * M + m) * K;
    f16* o = out + (long)b * N * M + m;
    for (int n0 = 0; n0 < N; n0 += 4) {
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int kc = 0; kc < K; kc += 8) {
            const f16x8 av = *reinterpret_cast<const f16x8*>(arow + kc);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f16x8 bv = *reinterpret_cast<const f16x8*>(sb + (n0 + j) * K + kc);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[j] = fmaf((float)av[e], (float)bv[e], acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (n0 + j < N) o[(long)(n0 + j) * M] = (f16)acc[j];
    }
}

// sin / cos of x radians: x / (2 pi) in f32, reduced to [-0.5, 0.5] revolutions, then the hardware sine / cosine (their operand is in revolutions)
__device__ __forceinline__ float sincos_rev(float rev, int mode) {
    rev -= rintf(rev);
    return mode ? __builtin_amdgcn_cosf(rev) : __builtin_amdgcn_sinf(rev);
}

__global__ __launch_bounds__(256) void sincos_kernel(const f16* __restrict__ x, f16* __restrict__ y, long n, int mode) {
    const long n8 = n / 8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i <= n8; i += (long)gridDim.x * 256) {
        if (i < n8) {
            const f16x8 v = *reinterpret_cast<const f16x8*>(x + i * 8);
            f16x8 r;
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = (f16)sincos_rev((float)v[e] * INV_2PI, mode);
            *reinterpret_cast<f16x8*>(y + i * 8) = r;
        } else {
            for (long j = n8 * 8; j < n; ++j) y[j] = (f16)sincos_rev((float)x[j] * INV_2PI, mode); // the tail behind the last whole piece
        }
    }
}

// one thread per (point, frequency): t = x g0 + y g1 IS the argument in revolutions (2 pi t radians), so product, scale and reduction stay in f32
__global__ __launch_bounds__(256) void fourier_kernel(const float* __restrict__ coords, const float* __restrict__ gauss, f16* __restrict__ out, long n_points, int F) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_points * F) return;
    const long p = i / F;
    const int f = (int)(i - p * F);
    const float t = fmaf(coords[2 * p + 1], gauss[2 * f + 1], coords[2 * p] * gauss[2 * f]);
    out[p * 2 * F + f] = (f16)sincos_rev(t, 0);
    out[p * 2 * F + F + f] = (f16)sincos_rev(t, 1);
}

} // namespace

extern "C" int vx_mul_mat_f16(const void* a, const void* b, void* out, int64_t M, int N, int K, int B, int Ba, void* stream) {
    VX_REQUIRE(a && b && out && M > 0 && N > 0 && K > 0 && B > 0, "vx_mul_mat_f16: empty problem");
    VX_REQUIRE(K % 8 == 0 && K <= MM_MAX_K, "vx_mul_mat_f16: K = %d (a multiple of 8, at most %d)", K, MM_MAX_K);
    VX_REQUIRE(N <= MM_MAX_N, "vx_mul_mat_f16: N = %d (at most %d columns)", N, MM_MAX_N);
    VX_REQUIRE(Ba == 1 || Ba == B, "vx_mul_mat_f16: the first operand's batch %d is neither 1 nor %d", Ba, B);
    VX_REQUIRE(aligned16(a), "vx_mul_mat_f16: the first operand must be 16-byte aligned");
    VX_REQUIRE(B <= 65535 && (M + 255) / 256 < (1L << 31), "vx_mul_mat_f16: too many blocks");
    hipLaunchKernelGGL(mul_mat_kernel, dim3(blocks_for(M), (unsigned)B), dim3(256), 0, as_stream(stream), reinterpret_cast<const f16*>(a), reinterpret_cast<const f16*>(b),
                       reinterpret_cast<f16*>(out), (long)M, N, K, Ba);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_sincos_f16(int mode, const void* x, void* y, int64_t n, void* stream) {
    VX_REQUIRE(x && y && n > 0, "vx_sincos_f16: bad operands");
    VX_REQUIRE(mode == 0 || mode == 1, "vx_sincos_f16: mode %d (0 sin, 1 cos)", mode);
    VX_REQUIRE(aligned16(x) && aligned16(y), "vx_sincos_f16: operands must be 16-byte aligned");
    hipLaunchKernelGGL(sincos_kernel, dim3(grid_stride_blocks(n / 8 + 1, 4096)), dim3(256), 0, as_stream(stream), reinterpret_cast<const f16*>(x), reinterpret_cast<f16*>(y), (long)n, mode);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_fourier_features_f32(const float* coords, const float* gauss, void* out, int64_t n_points, int F, void* stream) {
    VX_REQUIRE(coords && gauss && out && n_points > 0 && F > 0, "vx_fourier_features_f32: bad operands");
    VX_REQUIRE((n_points * F + 255) / 256 < (1L << 31), "vx_fourier_features_f32: too many blocks");
    hipLaunchKernelGGL(fourier_kernel, dim3(blocks_for(n_points * F)), dim3(256), 0, as_stream(stream), coords, gauss, reinterpret_cast<f16*>(out), (long)n_points, F);
    VX_LAUNCH_CHECK();
    return 1;
}
