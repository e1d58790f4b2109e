// Device-side helpers shared by the kernel files (included through vx_common.h). The numerics the parity with the reference rests
// on (ggml's gelu, the value + residue input pixel) and the LDS swizzle a tile's writers and readers must agree on are defined here once.
#pragma once

typedef __attribute__((address_space(1))) const void* gptr_t; // global / LDS operands of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(3))) void* lptr_t;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float gelu_tanh(float x) { // ggml_gelu (tanh form), the reference's activation everywhere
    // 0.5 x (1 + tanh(u)), u = sqrt(2/pi) x (1 + 0.044715 x^2), = x * sigmoid(2u) = x / (1 + exp2(x * w)): exp2 -> inf gives -0,
    // exp2 -> 0 gives x (no inf/inf); v_rcp instead of an IEEE division (a dozen VALU ops per element: the depthwise kernels were
    // VALU bound on it). 5 VALU + v_exp + v_rcp.
    const float c1 = -2.0f * 0.79788456080286535588f * 1.44269504088896340736f; // -2 sqrt(2/pi) log2(e)
    const float c3 = c1 * 0.044715f;
    const float w = fmaf(x * x, c3, c1);
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * w));
}

__device__ __forceinline__ float silu(float x) { // x * sigmoid(x) = x / (1 + exp(-x)); exp2 of a large argument gives inf and x * 0
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896340736f));
}

// max(x, 0) as ONE instruction: fmaxf() on an MFMA result costs a canonicalising v_max_f32 x, x, x first (IEEE mode), and the depth
// head's epilogue is 32 of them per tile in a kernel bound by VALU issue. Signed-integer max with 0 (same order as floats for non-NaN
// values, -0.0 and negatives -> +0), NOT an inline-asm v_max_f32: the hazard recogniser does not look into inline asm, and one placed
// right behind an accumulator's last MFMA reads it before the matrix pipe has written it (kernels_headconv.hip met exactly that in
// its first parity run: every wave's first row off by a few per cent).
__device__ __forceinline__ float relu1(float x) { return __int_as_float(max(__float_as_int(x), 0)); }

// value held by the same lane of the other 32-lane half (in the 32x32 MFMA layouts lanes l and l+32 own the same column)
__device__ __forceinline__ float other_half(float v) {
    const unsigned u = __float_as_uint(v);
    auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    // after the swap r[0] = {low: own low, high: low half's values}, r[1] = {low: high half's values, high: own high}
    return __uint_as_float((threadIdx.x & 32) ? r[0] : r[1]);
}

// 16-byte chunk of a 128-byte LDS row after the swizzle (a tile's writer and its readers both go through it): the rows of
// 16 consecutive lanes alternate between the two 128-byte halves of the bank row and take 8 different chunks inside each
__device__ __forceinline__ int swz128(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

// counted waits the compiler does not know it needs (LDS-DMA copies, hand-ordered ring stages)
template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void wait_lgkmcnt0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// the 8-channel input pixel of a first conv: channels 0..2 = f16(v), 3..5 = f16(v - f16(v)) (the rounding residue; the conv's weights
// are duplicated on channels 3..5, so the f32 input value is reconstructed inside the f32 accumulator), 6..7 zero
__device__ __forceinline__ f16x8 residue_pixel(const float (&v)[3]) {
    f16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const f16 hi = (f16)v[c];
        o[c] = hi;
        o[3 + c] = (f16)(v[c] - (float)hi);
    }
    return o;
}
