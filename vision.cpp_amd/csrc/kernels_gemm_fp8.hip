// OCP e4m3 GEMM on the block-scaled matrix instruction of gfx950 (v_mfma_scale_f32_16x16x128_f8f6f4: twice the f16 MFMA rate), opt-in -- BASELINE.json
// configs[4] asks for "fp8 GGUF weights on CDNA4 fp8 MFMA". The reference has no fp8 tensor type (scripts/convert.py:543, 551 offers f16 only), so the
// format is this backend's own: e4m3 values with ONE f32 scale per row -- per output channel for a weight, per token for an activation --
//   C[m, n] = act( sA[m] * sW[n] * sum_k A8[m, k] * W8[n, k] + bias[n] ),   K padded to a multiple of 128 with zeros
// replaces linear() (nn.cpp:6-12) with its bias / GELU epilogue on the MLP shapes of the TinyViT stages. The instruction's own e8m0 block scales
// are left at 2^0: a row scale commutes with the product and keeps f32 precision of the scale. Accuracy is the caller's decision
// (tests/test_fp8_decision.py: rejected for MobileSAM masks); this file only has to be exact for what it is given.
//
// Structure: 128 x 128 output tile, 4 waves of 64 x 64, k-step 128 (= 128 bytes per row); both operands global -> LDS by LDS-DMA
// (global_load_lds_dwordx4, 8 rows of 128 B per wave instruction) into a 2-stage ring; 16-byte chunks XOR-swizzled by (row & 7) on the source
// address and on the fragment reads (a lane's 32 operand bytes are two ds_read_b128); swapped operands (D^T = W A^T) so that a lane owns one
// output row and 4 consecutive columns of every 16 x 16 tile; the f16 tile is staged through LDS and leaves as 16-byte stores of whole 128-byte segments,
// with an optional residual map added on the way out.
#include "vx_common.h"

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int BM = 128, BN = 128, BKB = 128; // tile rows (tokens), tile columns (features), k bytes per step
constexpr int STAGE = (BM + BN) * BKB;       // 32 KiB

template <int ACT>
__global__ __launch_bounds__(256) void gemm_fp8_kernel(const vx_gemm_fp8_args p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1; // 2 x 2 waves: rows wr * 64, columns wc * 64
    const int i16 = lane & 15, g = lane >> 4;

    // XCD-aware tile order (blocks b and b + 8 share an L2): contiguous runs of the (row panel major) tile sequence per XCD
    const int tiles_n = p.N / BN;
    int tile;
    {
        const int nwg = gridDim.x, b = blockIdx.x, q = nwg >> 3, rem = nwg & 7, xcd = b & 7;
        tile = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (b >> 3);
    }
    const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
    const int nk = p.Kp / BKB;

    const unsigned char* __restrict__ Ag = static_cast<const unsigned char*>(p.A);
    const unsigned char* __restrict__ Wg = static_cast<const unsigned char*>(p.W);
    // LDS-DMA: wave w fills rows 32 w .. 32 w + 31 of each operand tile, 8 rows per instruction; lane l lands at row l >> 3, physical chunk l & 7
    // and therefore fetches logical chunk (l & 7) ^ (row & 7). Rows past M read row M - 1 again (their results are not stored).
    const int l_row = lane >> 3, l_chunk = lane & 7;
    auto issue = [&](int kt, int stage) {
        unsigned char* sa = smem + stage * STAGE;
        unsigned char* sw = sa + BM * BKB;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wave * 32 + i * 8 + l_row, chunk = l_chunk ^ (row & 7);
            const int am = min(m0 + row, p.M - 1);
            __builtin_amdgcn_global_load_lds((gptr_t)(Ag + (size_t)am * p.Kp + (size_t)kt * BKB + chunk * 16), (lptr_t)(sa + (wave * 32 + i * 8) * BKB), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)(Wg + (size_t)(n0 + row) * p.Kp + (size_t)kt * BKB + chunk * 16), (lptr_t)(sw + (wave * 32 + i * 8) * BKB), 16, 0, 0);
        }
    };
    // a lane's 32 operand bytes of tile row `row`: k bytes 32 g .. 32 g + 31 = chunks 2 g, 2 g + 1
    auto frag = [&](const unsigned char* base, int row) -> v8i {
        const unsigned char* r = base + row * BKB;
        const v4i lo = *reinterpret_cast<const v4i*>(r + (((2 * g) ^ (row & 7)) << 4));
        const v4i hi = *reinterpret_cast<const v4i*>(r + (((2 * g + 1) ^ (row & 7)) << 4));
        v8i f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return f;
    };

    f32x4 acc[4][4]; // [feature tile][token tile]: D^T[16 features, 16 tokens]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    issue(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        const int st = kt & 1;
        wait_vmcnt<0>();
        __syncthreads(); // k-tile kt landed; every wave is done with the other stage
        if (kt + 1 < nk) issue(kt + 1, st ^ 1);
        const unsigned char* sa = smem + st * STAGE;
        const unsigned char* sw = sa + BM * BKB;
        v8i fa[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) fa[b] = frag(sa, wr * 64 + b * 16 + i16);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const v8i fw = frag(sw, wc * 64 + a * 16 + i16);
#pragma unroll
            for (int b = 0; b < 4; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fa[b], acc[a][b], 0, 0, 0, 127, 0, 127); // e4m3 x e4m3, block scales 2^0
        }
    }

    // ---- epilogue: lane (token i16 of tile b, features 4 g .. 4 g + 3 of tile a). Scales, bias and activation on the accumulators; the wave's 64 x 64
    // f16 tile goes through LDS (its own 8 KiB of the finished ring; 16-byte chunks swizzled by the row) so that a row leaves as 16-byte stores of
    // 8 consecutive lanes = whole 128-byte segments; the optional residual map is added on the way out with 16-byte loads.
    __syncthreads(); // every wave is done reading the last k-tile
    unsigned char* otile = smem + wave * (64 * 128);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int row = b * 16 + i16, m = m0 + wr * 64 + row;
        const float sa_m = m < p.M ? p.a_scale[m] : 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int n = n0 + wc * 64 + a * 16 + 4 * g;
            const float4 sw4 = *reinterpret_cast<const float4*>(p.w_scale + n);
            float4 b4 = {0.f, 0.f, 0.f, 0.f};
            if (p.bias) b4 = *reinterpret_cast<const float4*>(p.bias + n);
            float v[4] = {fmaf(acc[a][b][0], sa_m * sw4.x, b4.x), fmaf(acc[a][b][1], sa_m * sw4.y, b4.y), fmaf(acc[a][b][2], sa_m * sw4.z, b4.z),
                          fmaf(acc[a][b][3], sa_m * sw4.w, b4.w)};
            if constexpr (ACT == 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = gelu_tanh(v[j]);
            }
            const f16x4 o = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
            const int chunk = (2 * a + (g >> 1)) ^ (row & 7);
            *reinterpret_cast<f16x4*>(otile + row * 128 + chunk * 16 + (g & 1) * 8) = o;
        }
    }
    // (a wave reads back only what it wrote: no barrier)
    const f16* res = static_cast<const f16*>(p.res);
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int row = it * 8 + (lane >> 3), c = lane & 7;
        const int m = m0 + wr * 64 + row, n = n0 + wc * 64 + c * 8;
        f16x8 o = *reinterpret_cast<const f16x8*>(otile + row * 128 + ((c ^ (row & 7)) << 4));
        if (m < p.M && n < p.n_valid) { // n_valid % 8 == 0
            if (res) o = o + *reinterpret_cast<const f16x8*>(res + (size_t)m * p.ldo + n);
            *reinterpret_cast<f16x8*>(static_cast<f16*>(p.out) + (size_t)m * p.ldo + n) = o;
        }
    }
}

// f16 rows -> e4m3 rows + one f32 scale per row (scale = absmax / 448, the largest e4m3 magnitude); one wave per row, K <= 8192
__global__ __launch_bounds__(256) void quantize_rows_kernel(const f16* __restrict__ x, int64_t ldx, unsigned char* __restrict__ q, float* __restrict__ scale, int M, int K, int Kp) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const f16* xr = x + (size_t)row * ldx;
    float amax = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
        const f16x8 v = *reinterpret_cast<const f16x8*>(xr + k);
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf((float)v[j]));
    }
    amax = wave_max(amax);
    const float s = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f, inv = 1.0f / s;
    if (lane == 0) scale[row] = s;
    unsigned char* qr = q + (size_t)row * Kp;
    for (int k = lane * 8; k < Kp; k += 512) {
        float v[8];
        if (k < K) {
            const f16x8 h = *reinterpret_cast<const f16x8*>(xr + k);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (float)h[j] * inv;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.f;
        }
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], hi, true);
        *reinterpret_cast<int2*>(qr + k) = int2{lo, hi};
    }
}

// host: round to nearest even OCP e4m3fn (bias 7, 3 mantissa bits, max 448, no infinities; NaN = 0x7f)
unsigned char e4m3_from_f32(float f) {
    if (f != f) return 0x7f;
    const unsigned char sign = f < 0 ? 0x80 : 0;
    float a = f < 0 ? -f : f;
    if (a >= 464.0f) return sign | 0x7e;         // saturate (464 = midpoint above 448 rounds up out of range)
    if (a < 0.0009765625f) return sign;          // below half of the smallest subnormal 2^-9
    int e;
    const float mant = std::frexp(a, &e);        // a = mant * 2^e, mant in [0.5, 1)
    int exp = e - 1;                             // a = (2 mant) * 2^exp
    if (exp < -6) {                              // subnormal: units of 2^-9
        const float u = a * 512.0f;
        int q = (int)u;
        const float r = u - (float)q;
        if (r > 0.5f || (r == 0.5f && (q & 1))) ++q;
        return sign | (unsigned char)q;          // q == 8 carries into the first normal
    }
    const float m8 = (2.0f * mant - 1.0f) * 8.0f; // mantissa in eighths
    int q = (int)m8;
    const float r = m8 - (float)q;
    if (r > 0.5f || (r == 0.5f && (q & 1))) ++q;
    if (q == 8) { q = 0; ++exp; }
    if (exp > 8 || (exp == 8 && q > 6)) return sign | 0x7e;
    return sign | (unsigned char)(((exp + 7) << 3) | q);
}

} // namespace

extern "C" {

int vx_gemm_fp8_supported(int N, int K) { return N > 0 && N % BN == 0 && K > 0; }

int vx_quantize_rows_e4m3(const void* x_f16, int64_t ldx, void* q, float* scale, int M, int K, int Kp, void* stream) {
    VX_REQUIRE(x_f16 && q && scale && M > 0 && K > 0 && K % 8 == 0 && Kp % 128 == 0 && Kp >= K && ldx >= K, "vx_quantize_rows_e4m3: bad arguments (K %% 8 == 0, Kp a multiple of 128 >= K)");
    hipLaunchKernelGGL(quantize_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, as_stream(stream), static_cast<const f16*>(x_f16), ldx, static_cast<unsigned char*>(q), scale, M, K, Kp);
    VX_LAUNCH_CHECK();
    return 1;
}

int vx_quantize_rows_e4m3_host(const float* w, int N, int K, int Kp, void* q_out, float* scale_out) {
    VX_REQUIRE(w && q_out && scale_out && N > 0 && K > 0 && Kp >= K && Kp % 128 == 0, "vx_quantize_rows_e4m3_host: bad arguments");
    unsigned char* q = static_cast<unsigned char*>(q_out);
    for (int n = 0; n < N; ++n) {
        float amax = 0.f;
        for (int k = 0; k < K; ++k) amax = std::fmax(amax, std::fabs(w[(size_t)n * K + k]));
        const float s = amax > 0.f ? amax / 448.0f : 1.0f;
        scale_out[n] = s;
        for (int k = 0; k < Kp; ++k) q[(size_t)n * Kp + k] = k < K ? e4m3_from_f32(w[(size_t)n * K + k] / s) : 0;
    }
    return 1;
}

int vx_gemm_fp8(const vx_gemm_fp8_args* args, void* stream) {
    const vx_gemm_fp8_args& a = *args;
    VX_REQUIRE(a.A && a.W && a.a_scale && a.w_scale && a.out, "vx_gemm_fp8: null operand");
    VX_REQUIRE(a.M > 0 && a.N % BN == 0 && a.Kp % BKB == 0 && a.Kp > 0, "vx_gemm_fp8: N = %d must be a multiple of %d and Kp = %d a multiple of %d", a.N, BN, a.Kp, BKB);
    VX_REQUIRE(a.n_valid > 0 && a.n_valid <= a.N && a.n_valid % 8 == 0 && a.ldo >= a.n_valid && a.ldo % 8 == 0, "vx_gemm_fp8: n_valid = %d, ldo = %lld (multiples of 8, n_valid at most N)", a.n_valid, (long long)a.ldo);
    VX_REQUIRE(a.act == 0 || a.act == 1, "vx_gemm_fp8: act %d (0 none, 1 gelu)", a.act);
    const int tiles = ((a.M + BM - 1) / BM) * (a.N / BN);
    const int lds = 2 * STAGE;
    if (a.act == 1) {
        VX_CHECK(vx_ensure_dynamic_lds(reinterpret_cast<const void*>(gemm_fp8_kernel<1>), lds));
        hipLaunchKernelGGL(gemm_fp8_kernel<1>, dim3(tiles), dim3(256), lds, as_stream(stream), a);
    } else {
        VX_CHECK(vx_ensure_dynamic_lds(reinterpret_cast<const void*>(gemm_fp8_kernel<0>), lds));
        hipLaunchKernelGGL(gemm_fp8_kernel<0>, dim3(tiles), dim3(256), lds, as_stream(stream), a);
    }
    VX_LAUNCH_CHECK();
    return 1;
}

} // extern "C"
