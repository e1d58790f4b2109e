// Multi-head attention without a mask for any number of queries and keys, head_dim 16, 32 and 64, on the matrix cores of gfx950:
// softmax(scale * q k^T) v -- the graph layer's ATTENTION_CROSS op (reference src/visp/nn.cpp:210-244 with mask == nullptr, as
// mobile-sam.cpp:307-319 calls it for the mask decoder: 7 x 7 self-attention at head_dim 32, 7 x 4096 and 4096 x 7 cross attention at 16).
//
// q f16 [B][T_q][H][HD], k and v f16 [B][T_k][H][HD] -- token-major rows of H * HD, where the graph has them: no head-major copies in front.
// out f16 [B][T_q][H * HD]. The kernel multiplies the f32 scores by scale * log2(e) itself (q is NOT pre-scaled).
// The orientation is that of kernels_attn_mask.hip: one block = NW wave64 = 32 NW queries of one (batch, head); S^T = K Q^T on
// v_mfma_f32_32x32x16_f16 (head_dim 16 is exactly one k-step), so a lane owns ONE query column (lane & 31) and 16 keys of the 32-key block
// in its accumulator registers (key = 8 (e >> 2) + 4 (lane >> 5) + (e & 3)); online softmax over the 32-key blocks in the exp2 domain with
// the finite running-maximum floor (-1e30: a block that is all -inf while nothing has been seen gives exp2(-inf + 1e30) = 0, never NaN);
// P^T feeds O^T = V^T P^T straight from the accumulators, V^T fragments come from ds_read_b64_tr_b16. At head_dim 16 the transposed reads
// of lanes 16..31 of a half fetch d = 0..15 again: rows 16..31 of O^T are computed and never stored.
//   * keys at or beyond the end of the block's key range score -inf (P exactly 0); queries >= T_q are computed on a clamped row, not stored.
//
// Key splitting. With T_q <= 32 there is one block per (batch, head): 8 blocks at the decoder's 7 x 4096. From CX_SPLIT_MIN keys on, the keys
// are cut into parts of CX_SPLIT_KEYS; block (bh, part) writes its unnormalised f32 triple (m, l, O) per query into `partial`
// ([B * H][parts][32][HD + 2]: m, l, O[0 .. HD)), and attention_cross_combine_kernel, a second small launch, folds the parts IN PART ORDER:
// m = max m_i, l = sum l_i 2^(m_i - m), O = sum O_i 2^(m_i - m), every sum a sequential f32 chain from part 0 upwards. No atomics: the
// same bits on every run. The few-keys side (T_k <= 32, many queries) is one key block per wave tile: one staging step, no ring.
#include "vx_common.h"

namespace {

constexpr float CX_LOG2E = 1.44269504088896340736f;
constexpr int CX_SPLIT_KEYS = 128; // keys per part (a multiple of 32)
constexpr int CX_SPLIT_MIN = 256;  // fewer keys than this: one part

typedef __fp16 hv4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

template <int HD>
__device__ __forceinline__ int cx_k_swz(int row, int chunk) { return HD == 64 ? chunk ^ ((row >> 1) & 7) : (HD == 32 ? chunk ^ ((row >> 2) & 3) : chunk); }
template <int HD>
__device__ __forceinline__ int cx_v_swz(int row, int chunk) { return HD == 64 ? chunk ^ (((row >> 1) & 1) << 2) : chunk; }

template <int HD, int NW>
__global__ __launch_bounds__(64 * NW) void attention_cross_kernel(const f16* __restrict__ Q, const f16* __restrict__ K, const f16* __restrict__ V, f16* __restrict__ O,
                                                                  float* __restrict__ partial, int H, int Tq, int Tk, int n_split, float qs) {
    constexpr int ROW = HD * 2;           // bytes per K / V row in LDS
    constexpr int CH = HD / 8;            // 16-byte chunks per row
    constexpr int N_CH = 32 * CH;         // chunks per 32-key block
    constexpr int THREADS = 64 * NW;
    constexpr int PER = (N_CH + THREADS - 1) / THREADS;
    constexpr int DS = HD / 16;           // d-steps of the score product
    constexpr int DB = HD == 64 ? 2 : 1;  // 32-row blocks of O^T
    constexpr int G_OUT = HD == 16 ? 2 : 4; // groups of four accumulator rows that hold real d
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 32 * ROW];
    unsigned char* const sk = smem;
    unsigned char* const sv = smem + 32 * ROW;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int n_qblk = (Tq + 32 * NW - 1) / (32 * NW);
    const int per_bh = n_qblk * n_split;  // (n_split > 1 only with n_qblk == 1)
    const int bh = blockIdx.x / per_bh;   // b * H + head
    const int rem = blockIdx.x - bh * per_bh;
    const int part = n_split > 1 ? rem : 0;
    const int q0 = (n_split > 1 ? 0 : rem) * (32 * NW) + wave * 32;
    const int b = bh / H, head = bh - b * H;
    const bool active = q0 < Tq;          // wave-uniform: a wave without queries only stages K / V and keeps the barriers
    const int k_begin = n_split > 1 ? part * CX_SPLIT_KEYS : 0;
    const int k_end = n_split > 1 ? min(Tk, k_begin + CX_SPLIT_KEYS) : Tk;
    const long ld = (long)H * HD;         // elements between token rows

    const f16* Qb = Q + (long)b * Tq * ld + head * HD;
    const f16* Kb = K + (long)b * Tk * ld + head * HD;
    const f16* Vb = V + (long)b * Tk * ld + head * HD;

    const int q = q0 + r;
    const int qc = q < Tq ? q : Tq - 1;
    f16x8 qf[DS];
#pragma unroll
    for (int s = 0; s < DS; ++s) qf[s] = *reinterpret_cast<const f16x8*>(Qb + (long)qc * ld + 16 * s + 8 * h);

    // ---- staging: chunk cid = tid + i * THREADS of the block is row cid / CH, 16-byte chunk cid % CH
    f16x8 kreg[PER], vreg[PER];
    auto load_block = [&](int k0) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int cid = tid + i * THREADS, row = cid / CH, c = cid - row * CH, key = k0 + row;
            f16x8 z = {(f16)0, (f16)0, (f16)0, (f16)0, (f16)0, (f16)0, (f16)0, (f16)0};
            kreg[i] = z;
            vreg[i] = z;
            if (cid < N_CH && key < k_end) {
                kreg[i] = *reinterpret_cast<const f16x8*>(Kb + (long)key * ld + c * 8);
                vreg[i] = *reinterpret_cast<const f16x8*>(Vb + (long)key * ld + c * 8);
            }
        }
    };
    auto store_block = [&]() {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int cid = tid + i * THREADS, row = cid / CH, c = cid - row * CH;
            if (cid < N_CH) {
                *reinterpret_cast<f16x8*>(sk + row * ROW + cx_k_swz<HD>(row, c) * 16) = kreg[i];
                *reinterpret_cast<f16x8*>(sv + row * ROW + cx_v_swz<HD>(row, c) * 16) = vreg[i];
            }
        }
    };

    // loop-invariant LDS offsets: K fragment of d-step s = row r, chunk 2 s + h; V^T transposed reads as in kernels_attn_mask.hip (16-lane
    // group g covers d = 16 (g & 1) .. +15 of key half g >> 1 == h; lane 4 t + p of the group supplies key row t, columns 4 p .. +3)
    int k_off[DS], v_off[DB];
#pragma unroll
    for (int s = 0; s < DS; ++s) k_off[s] = r * ROW + cx_k_swz<HD>(r, 2 * s + h) * 16;
    {
        const int key = 4 * h + ((lane & 15) >> 2), dd = ((16 * ((lane >> 4) & 1)) & (HD - 1)) + 4 * (lane & 3);
#pragma unroll
        for (int db = 0; db < DB; ++db) v_off[db] = key * ROW + cx_v_swz<HD>(key, (dd + 32 * db) >> 3) * 16 + (dd & 7) * 2;
    }

    f32x16 o[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[db][e] = 0.0f;
    float m_run = -1e30f, l_run = 0.0f; // finite floor: see the header
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    const int n_blocks = (k_end - k_begin + 31) / 32;
    load_block(k_begin);
    for (int kb = 0; kb < n_blocks; ++kb) {
        const int k0 = k_begin + kb * 32;
        __syncthreads(); // every wave is done with block kb - 1
        store_block();
        __syncthreads();
        if (kb + 1 < n_blocks) load_block(k0 + 32);
        if (!active) continue;

        f32x16 s = zero;
#pragma unroll
        for (int st = 0; st < DS; ++st) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(sk + k_off[st]), qf[st], s, 0, 0, 0);

        float mloc = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int key = k0 + 8 * (e >> 2) + 4 * h + (e & 3);
            const float v = key < k_end ? s[e] * qs : -INFINITY;
            s[e] = v;
            mloc = fmaxf(mloc, v);
        }
        mloc = fmaxf(mloc, other_half(mloc)); // lanes l and l + 32 own the same query
        const float m_new = fmaxf(m_run, mloc);
        if (__any(m_new > m_run)) {
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            l_run *= alpha;
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int e = 0; e < 16; ++e) o[db][e] *= alpha;
            m_run = m_new;
        }
        float psum = 0.0f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float p = __builtin_amdgcn_exp2f(s[e] - m_run);
            s[e] = p;
            psum += p;
        }
        l_run += psum;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) { // element j of the k-step <-> key k0 + 16 ks + 8 (j >> 2) + 4 h + (j & 3)
            f16x8 pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = (f16)s[8 * ks + j];
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                const unsigned char* vrow = sv + v_off[db] + ks * 16 * ROW;
                hv4 va = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) hv4*)(vrow));
                hv4 vb = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) hv4*)(vrow + 8 * ROW));
                f16x8 vf = {(f16)va[0], (f16)va[1], (f16)va[2], (f16)va[3], (f16)vb[0], (f16)vb[1], (f16)vb[2], (f16)vb[3]};
                o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o[db], 0, 0, 0);
            }
        }
    }

    if (!active || q >= Tq) return;
    const float l_tot = l_run + other_half(l_run);
    if (n_split > 1) { // the unnormalised triple of this part: accumulator rows d = 32 db + 8 g + 4 h + j
        float* prow = partial + (((long)bh * n_split + part) * 32 + q) * (HD + 2);
        if (h == 0) { prow[0] = m_run; prow[1] = l_tot; }
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int g = 0; g < G_OUT; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) prow[2 + db * 32 + 8 * g + 4 * h + j] = o[db][g * 4 + j];
        return;
    }
    const float inv = 1.0f / l_tot;
    f16* orow = O + ((long)b * Tq + q) * ld + head * HD;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int g = 0; g < G_OUT; ++g) {
            f16x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (f16)(o[db][g * 4 + j] * inv);
            *reinterpret_cast<f16x4*>(orow + db * 32 + 8 * g + 4 * h) = v;
        }
}

// one thread per (query, d) of one (batch, head): the parts in part order, every sum one sequential f32 chain
template <int HD>
__global__ __launch_bounds__(256) void attention_cross_combine_kernel(const float* __restrict__ partial, f16* __restrict__ O, int H, int Tq, int n_split) {
    const int bh = blockIdx.x, b = bh / H, head = bh - b * H;
    const float* base = partial + (long)bh * n_split * 32 * (HD + 2);
    for (int idx = threadIdx.x; idx < Tq * HD; idx += 256) {
        const int q = idx / HD, d = idx - q * HD;
        const float* p = base + (long)q * (HD + 2);
        float m = -1e30f;
        for (int i = 0; i < n_split; ++i) m = fmaxf(m, p[(long)i * 32 * (HD + 2)]);
        float l = 0.0f, acc = 0.0f;
        for (int i = 0; i < n_split; ++i) {
            const float* pi = p + (long)i * 32 * (HD + 2);
            const float w = __builtin_amdgcn_exp2f(pi[0] - m);
            l = fmaf(pi[1], w, l);
            acc = fmaf(pi[2 + d], w, acc);
        }
        O[((long)b * Tq + q) * ((long)H * HD) + head * HD + d] = (f16)(acc * (1.0f / l));
    }
}

int cx_parts(int Tq, int Tk) { return Tq <= 32 && Tk >= CX_SPLIT_MIN ? (Tk + CX_SPLIT_KEYS - 1) / CX_SPLIT_KEYS : 1; }

template <int HD>
void launch_cross(const f16* q, const f16* k, const f16* v, f16* out, float* partial, int B, int H, int Tq, int Tk, float qs, int steps, hipStream_t s) {
    const int n_split = cx_parts(Tq, Tk);
    if (steps & 1) {
    const int qblocks = (Tq + 31) / 32, nw = qblocks >= 3 ? 4 : qblocks; // few queries: a block per 32 / 64 of them
    const dim3 grid((unsigned)((Tq + 32 * nw - 1) / (32 * nw)) * B * H * n_split);
    switch (nw) {
        case 1: hipLaunchKernelGGL((attention_cross_kernel<HD, 1>), grid, dim3(64), 0, s, q, k, v, out, partial, H, Tq, Tk, n_split, qs); break;
        case 2: hipLaunchKernelGGL((attention_cross_kernel<HD, 2>), grid, dim3(128), 0, s, q, k, v, out, partial, H, Tq, Tk, n_split, qs); break;
        default: hipLaunchKernelGGL((attention_cross_kernel<HD, 4>), grid, dim3(256), 0, s, q, k, v, out, partial, H, Tq, Tk, n_split, qs); break;
    }
    }
    if (n_split > 1 && (steps & 2)) hipLaunchKernelGGL((attention_cross_combine_kernel<HD>), dim3((unsigned)(B * H)), dim3(256), 0, s, partial, out, H, Tq, n_split);
}

} // namespace

extern "C" int vx_attention_cross_parts(int Tq, int Tk) { return Tq > 0 && Tk > 0 ? cx_parts(Tq, Tk) : 0; }

extern "C" size_t vx_attention_cross_partial_bytes(int B, int H, int Tq, int Tk, int head_dim) {
    if (B <= 0 || H <= 0 || Tq <= 0 || Tk <= 0 || head_dim <= 0) return 0;
    const int parts = cx_parts(Tq, Tk);
    return parts > 1 ? (size_t)B * H * parts * 32 * (head_dim + 2) * sizeof(float) : 0;
}

// steps: 1 = the attention launch (which writes `out` itself when there is one part), 2 = the combine launch of a split, 3 = both
static int attention_cross_steps(const void* q, const void* k, const void* v, void* out, void* partial, size_t partial_bytes, int B, int H, int Tq, int Tk, int head_dim,
                                 float scale, int steps, void* stream) {
    VX_REQUIRE(q && k && v && out && B > 0 && H > 0 && Tq > 0 && Tk > 0, "vx_attention_cross_f16: empty problem");
    VX_REQUIRE(head_dim == 16 || head_dim == 32 || head_dim == 64, "vx_attention_cross_f16: head_dim %d (16, 32 and 64 are built)", head_dim);
    VX_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && ((reinterpret_cast<uintptr_t>(out) & 7) == 0), "vx_attention_cross_f16: q, k, v must be 16-byte aligned, out 8-byte aligned");
    const size_t need = vx_attention_cross_partial_bytes(B, H, Tq, Tk, head_dim);
    VX_REQUIRE(need == 0 || (partial && partial_bytes >= need && (reinterpret_cast<uintptr_t>(partial) & 3) == 0),
               "vx_attention_cross_f16: %d queries on %d keys split the keys into %d parts and need %zu bytes of partial results (vx_attention_cross_partial_bytes), got %zu", Tq, Tk,
               cx_parts(Tq, Tk), need, partial ? partial_bytes : (size_t)0);
    VX_REQUIRE((long)((Tq + 31) / 32) * B * H * cx_parts(Tq, Tk) < (1L << 31), "vx_attention_cross_f16: too many blocks");
    const f16 *qp = reinterpret_cast<const f16*>(q), *kp = reinterpret_cast<const f16*>(k), *vp = reinterpret_cast<const f16*>(v);
    f16* op = reinterpret_cast<f16*>(out);
    float* pp = reinterpret_cast<float*>(partial);
    const float qs = scale * CX_LOG2E;
    if (head_dim == 16) launch_cross<16>(qp, kp, vp, op, pp, B, H, Tq, Tk, qs, steps, as_stream(stream));
    else if (head_dim == 32) launch_cross<32>(qp, kp, vp, op, pp, B, H, Tq, Tk, qs, steps, as_stream(stream));
    else launch_cross<64>(qp, kp, vp, op, pp, B, H, Tq, Tk, qs, steps, as_stream(stream));
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_attention_cross_f16(const void* q, const void* k, const void* v, void* out, void* partial, size_t partial_bytes, int B, int H, int Tq, int Tk,
                                      int head_dim, float scale, void* stream) {
    return attention_cross_steps(q, k, v, out, partial, partial_bytes, B, H, Tq, Tk, head_dim, scale, 3, stream);
}
extern "C" int vx_attention_cross_step_f16(int step, const void* q, const void* k, const void* v, void* out, void* partial, size_t partial_bytes, int B, int H, int Tq,
                                           int Tk, int head_dim, float scale, void* stream) {
    VX_REQUIRE(step == 1 || step == 2, "vx_attention_cross_step_f16: step %d (1 the attention launch, 2 the combine launch)", step);
    return attention_cross_steps(q, k, v, out, partial, partial_bytes, B, H, Tq, Tk, head_dim, scale, step, stream);
}
