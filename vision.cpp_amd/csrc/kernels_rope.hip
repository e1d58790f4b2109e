// Rotary position embedding and the token gather of the SAM3 encoders (sam3.h:221-231, 413-438) for the graph layer:
//   vx_rope_f16      ggml_rope_ext (GGML_ROPE_TYPE_NORMAL) on rows of n channels: pair i of a row at token t is rotated by the angle whose cosine and
//                    sine the host put into table[t][i] and table[t][n / 2 + i]
//   vx_rope2d_f16    apply_rope_2d on whole heads: channels [0, hd / 2) from table x, [hd / 2, hd) from table y, on one or two tensors (q and k) per launch
//   vx_get_rows_f16  ggml_get_rows with an index that is known at run time only: out[j] = table[idx[j]], a row of zeros for an index outside the table
// All three are copies with a little arithmetic: memory-bound, 16 bytes per lane and access, consecutive lanes on consecutive 16-byte pieces of a row. A
// lane reads and writes the SAME four pairs, so a rotation may run in place. No LDS, no scratch, no transcendentals: the angles come from the host.
#include "vx_common.h"

namespace {

struct rope_args {
    const f16* x[2];
    f16* out[2];
    const float* tab[2]; // per half of a row: f32 [T][n], cos in [0, n / 2), sin in [n / 2, n)
    float scale[2];      // per tensor: multiplied into the rotated values (q_scale on tensor 0)
    int n, halves, heads, T, B;
    int si[3], so[3];    // element strides of (head, token, batch), in and out
    int total;           // lanes per tensor: B * T * heads * halves * n / 8
};

__global__ __launch_bounds__(256) void rope_kernel(rope_args a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.total) return;
    const int which = blockIdx.y;
    const int per_row = a.halves * a.n / 8;
    const int c8 = i % per_row, r = i / per_row;
    const int h = r % a.heads, r2 = r / a.heads;
    const int t = r2 % a.T, b = r2 / a.T;
    const int c = c8 * 8, half = c >= a.n ? 1 : 0, cc = c - half * a.n; // n % 8 == 0: a lane's eight channels lie in one half
    const float* tab = a.tab[half] + t * a.n + cc / 2;
    const f32x4 co = *reinterpret_cast<const f32x4*>(tab), sn = *reinterpret_cast<const f32x4*>(tab + a.n / 2);
    const f16x8 v = *reinterpret_cast<const f16x8*>(a.x[which] + h * a.si[0] + t * a.si[1] + b * a.si[2] + c);
    const float s = a.scale[which];
    f16x8 o;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float x0 = (float)v[2 * p], x1 = (float)v[2 * p + 1];
        o[2 * p] = (f16)(fmaf(-x1, sn[p], x0 * co[p]) * s);
        o[2 * p + 1] = (f16)(fmaf(x1, co[p], x0 * sn[p]) * s);
    }
    *reinterpret_cast<f16x8*>(a.out[which] + h * a.so[0] + t * a.so[1] + b * a.so[2] + c) = o;
}

__global__ __launch_bounds__(256) void get_rows_kernel(const f16* __restrict__ table, const int* __restrict__ idx, f16* __restrict__ out, int rows, int C8, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int j = i / C8, c8 = i - j * C8;
    const int row = idx[j];
    f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (row >= 0 && row < rows) v = *reinterpret_cast<const f16x8*>(table + ((long)row * C8 + c8) * 8); // an index outside the table never reads
    *reinterpret_cast<f16x8*>(out + (long)i * 8) = v;
}

// what the launcher needs of a problem besides its pointers; null: fine, else the reason
const char* rope_shape_error(int row, int heads, int T, int B, const int64_t si[3], const int64_t so[3], int64_t* span_in = nullptr, int64_t* span_out = nullptr) {
    if (row <= 0 || heads <= 0 || T <= 0 || B <= 0) return "empty problem";
    const int64_t ext[3] = {heads, T, B};
    int64_t last_in = row, last_out = row; // elements from the first of a tensor to behind its last
    for (int d = 0; d < 3; ++d) {
        if (si[d] < 0 || so[d] < 0 || si[d] % 8 || so[d] % 8) return "strides must be non-negative multiples of 8 elements (16-byte rows)";
        last_in += (ext[d] - 1) * si[d];
        last_out += (ext[d] - 1) * so[d];
    }
    const int64_t lim = (int64_t)1 << 31;
    if (last_in >= lim || last_out >= lim || (int64_t)heads * T * B * (row / 8) >= lim || (int64_t)T * row >= lim) return "extents overflow the kernel's 32-bit indexing";
    if (span_in) *span_in = last_in;
    if (span_out) *span_out = last_out;
    return nullptr;
}

int rope_launch(const char* who, const void* x0, void* out0, const void* x1, void* out1, const float* tx, const float* ty, int n, int halves, int heads, int T, int B,
                const int64_t si[3], const int64_t so[3], float q_scale, void* stream) {
    VX_REQUIRE(x0 && out0 && tx && (halves == 1 || ty) && (!x1) == (!out1), "%s: null operand", who);
    VX_REQUIRE(n > 0 && n % 8 == 0, "%s: n = %d rotated channels per table (a positive multiple of 8)", who, n);
    int64_t span_in = 0, span_out = 0;
    const char* why = rope_shape_error(n * halves, heads, T, B, si, so, &span_in, &span_out);
    VX_REQUIRE(!why, "%s: %s", who, why);
    VX_REQUIRE(aligned16(x0) && aligned16(out0) && aligned16(x1) && aligned16(out1) && aligned16(tx) && aligned16(ty), "%s: operands must be 16-byte aligned", who);
    const bool same = si[0] == so[0] && si[1] == so[1] && si[2] == so[2];
    const bool in_place = x0 == out0 || (x1 && x1 == out1); // legal because a lane reads and writes the same pairs -- at the same address only
    VX_REQUIRE(!in_place || same, "%s: in place needs equal strides in and out", who);
    // an output may share memory with an input only as that input's own in-place pass; two outputs never share any
    const uintptr_t xs[2] = {reinterpret_cast<uintptr_t>(x0), reinterpret_cast<uintptr_t>(x1)}, os[2] = {reinterpret_cast<uintptr_t>(out0), reinterpret_cast<uintptr_t>(out1)};
    const uintptr_t bytes_in = (uintptr_t)span_in * 2, bytes_out = (uintptr_t)span_out * 2;
    for (int o = 0; o < (x1 ? 2 : 1); ++o) {
        for (int i = 0; i < (x1 ? 2 : 1); ++i)
            VX_REQUIRE((o == i && os[o] == xs[i]) || os[o] + bytes_out <= xs[i] || xs[i] + bytes_in <= os[o], "%s: output %d overlaps input %d without being the same buffer", who, o, i);
        VX_REQUIRE(o == 0 || os[1] + bytes_out <= os[0] || os[0] + bytes_out <= os[1], "%s: the two outputs overlap", who);
    }
    rope_args a;
    a.x[0] = reinterpret_cast<const f16*>(x0); a.x[1] = reinterpret_cast<const f16*>(x1);
    a.out[0] = reinterpret_cast<f16*>(out0); a.out[1] = reinterpret_cast<f16*>(out1);
    a.tab[0] = tx; a.tab[1] = halves == 2 ? ty : tx;
    a.scale[0] = q_scale; a.scale[1] = 1.0f;
    a.n = n; a.halves = halves; a.heads = heads; a.T = T; a.B = B;
    for (int d = 0; d < 3; ++d) { a.si[d] = (int)si[d]; a.so[d] = (int)so[d]; }
    a.total = B * T * heads * (halves * n / 8);
    hipLaunchKernelGGL(rope_kernel, dim3(blocks_for(a.total), x1 ? 2 : 1), dim3(256), 0, as_stream(stream), a);
    VX_LAUNCH_CHECK();
    return 1;
}

} // namespace

extern "C" int vx_rope_supported(int n, int heads, int T, int B, const int64_t strides_in[3], const int64_t strides_out[3]) {
    return n > 0 && n % 8 == 0 && strides_in && strides_out && !rope_shape_error(n, heads, T, B, strides_in, strides_out);
}

extern "C" int vx_rope2d_supported(int head_dim, int heads, int T, int B, const int64_t strides_in[3], const int64_t strides_out[3]) {
    return head_dim > 0 && head_dim % 16 == 0 && strides_in && strides_out && !rope_shape_error(head_dim, heads, T, B, strides_in, strides_out);
}

extern "C" int vx_rope_f16(const void* x, void* out, const float* table, int n, int heads, int T, int B, const int64_t strides_in[3], const int64_t strides_out[3], float q_scale,
                           void* stream) {
    VX_REQUIRE(strides_in && strides_out, "vx_rope_f16: null strides");
    return rope_launch("vx_rope_f16", x, out, nullptr, nullptr, table, nullptr, n, 1, heads, T, B, strides_in, strides_out, q_scale, stream);
}

extern "C" int vx_rope2d_f16(const void* q, void* q_out, const void* k, void* k_out, const float* table_x, const float* table_y, int head_dim, int heads, int T, int B,
                             const int64_t strides_in[3], const int64_t strides_out[3], float q_scale, void* stream) {
    VX_REQUIRE(strides_in && strides_out, "vx_rope2d_f16: null strides");
    VX_REQUIRE(head_dim > 0 && head_dim % 16 == 0, "vx_rope2d_f16: head_dim %d (a positive multiple of 16: two halves of n % 8 == 0 channels)", head_dim);
    return rope_launch("vx_rope2d_f16", q, q_out, k, k_out, table_x, table_y, head_dim / 2, 2, heads, T, B, strides_in, strides_out, q_scale, stream);
}

extern "C" int vx_get_rows_f16(const void* table, const int32_t* idx, void* out, int64_t rows, int C, int64_t n_idx, void* stream) {
    VX_REQUIRE(table && idx && out && rows > 0 && C > 0 && n_idx > 0, "vx_get_rows_f16: empty problem");
    VX_REQUIRE(C % 8 == 0, "vx_get_rows_f16: C = %d (a multiple of 8)", C);
    VX_REQUIRE(aligned16(table) && aligned16(out) && (reinterpret_cast<uintptr_t>(idx) & 3) == 0, "vx_get_rows_f16: table and out must be 16-byte aligned, idx 4-byte aligned");
    VX_REQUIRE(rows < ((int64_t)1 << 31) && n_idx * (C / 8) < ((int64_t)1 << 31), "vx_get_rows_f16: extents overflow the kernel's 32-bit indexing");
    const int total = (int)(n_idx * (C / 8));
    hipLaunchKernelGGL(get_rows_kernel, dim3(blocks_for(total)), dim3(256), 0, as_stream(stream), reinterpret_cast<const f16*>(table), idx, reinterpret_cast<f16*>(out), (int)rows, C / 8,
                       total);
    VX_LAUNCH_CHECK();
    return 1;
}
