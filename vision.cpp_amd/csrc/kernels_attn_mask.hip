// Multi-head self-attention with an additive mask, head_dim 32 and 64, any number of tokens, on the matrix cores of gfx950:
// softmax(scale * q k^T + mask) v -- the graph layer's ATTENTION_MASKED op (reference src/visp/nn.cpp:210-244 with a mask, as
// swin::window_attention calls it, src/visp/arch/swin.cpp:69-97: mask = relative position bias [+ the shifted-window mask]).
//
// q, k, v f16 head-major [B * H][T][HD], q already multiplied by scale * log2(e) (VX_ATTN_Q_SCALE, as for vx_attention_f16);
// mask f16 or f32 [Bm][Hm][T queries][T keys] (keys contiguous), Hm in {1, H}, batch b reads image b % Bm; out f16 [B][T][H * HD].
// One block = NW wave64 = 32 NW queries of one (batch, head); the same "swapped" formulation as kernels_attn.hip and
// kernels_winattn.hip: S^T = K Q^T on v_mfma_f32_32x32x16_f16, so a lane owns ONE query column (lane & 31) and holds 16 keys of
// the 32-key block in its accumulator registers (key = 8 (e >> 2) + 4 (lane >> 5) + (e & 3)): runs of four consecutive keys, so
// the mask row of the lane's query loads as four 8-byte (f16) / 16-byte (f32) pieces per key block when T is a multiple of 4
// (rows are then aligned), element by element otherwise. The softmax is online over the 32-key blocks in the exp2 domain, P^T
// feeds O^T = V^T P^T straight from the accumulators, V^T fragments come from ds_read_b64_tr_b16.
// K and V blocks (32 keys x HD) go through registers into LDS (zero rows behind T), the next block's global loads in flight
// while the current one is computed; the LDS images are swizzled as in the two kernels above (K: 16-byte chunk ^ row bits, so
// the ds_read_b128 of 32 rows spread over the banks; V at HD 64: chunk ^ 4 on odd row pairs for the transposed reads).
//   * keys >= T score -inf (P exactly 0), queries >= T are computed on a clamped row and not stored;
//   * the running maximum starts at a finite floor (-1e30), not -inf: a 32-key block that is all -inf for a query while nothing
//     has been seen yet gives exp2(-inf - (-1e30)) = 0, never exp2(-inf - (-inf)) = NaN;
//   * a query whose mask is -inf on EVERY key has l = 0: its output row is unspecified (the reference gives NaN).
#include "vx_common.h"

namespace {

constexpr float AM_LOG2E = 1.44269504088896340736f;

typedef __fp16 hv4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

template <int HD>
__device__ __forceinline__ int am_k_swz(int row, int chunk) { return HD == 64 ? chunk ^ ((row >> 1) & 7) : chunk ^ ((row >> 2) & 3); }
template <int HD>
__device__ __forceinline__ int am_v_swz(int row, int chunk) { return HD == 64 ? chunk ^ (((row >> 1) & 1) << 2) : chunk; }

template <int HD, int NW>
__global__ __launch_bounds__(64 * NW) void attention_masked_kernel(const f16* __restrict__ Q, const f16* __restrict__ K, const f16* __restrict__ V,
                                                                   const void* __restrict__ mask, f16* __restrict__ O, int H, int T, int Hm, int Bm,
                                                                   int mask_f32) {
    constexpr int ROW = HD * 2;           // bytes per K / V row in LDS
    constexpr int CH = HD / 8;            // 16-byte chunks per row
    constexpr int N_CH = 32 * CH;         // chunks per 32-key block
    constexpr int THREADS = 64 * NW;
    constexpr int PER = (N_CH + THREADS - 1) / THREADS;
    constexpr int DS = HD / 16;           // d-steps of the score product
    constexpr int DB = HD / 32;           // 32-row blocks of O^T
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 32 * ROW];
    unsigned char* const sk = smem;
    unsigned char* const sv = smem + 32 * ROW;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int n_qblk = (T + 32 * NW - 1) / (32 * NW);
    const int bh = blockIdx.x / n_qblk;   // b * H + head
    const int q0 = (blockIdx.x - bh * n_qblk) * (32 * NW) + wave * 32;
    const int b = bh / H, head = bh - b * H;
    const bool active = q0 < T;           // wave-uniform: a wave without queries only stages K / V and keeps the barriers

    const f16* Qb = Q + (long)bh * T * HD;
    const f16* Kb = K + (long)bh * T * HD;
    const f16* Vb = V + (long)bh * T * HD;

    const int q = q0 + r;
    const int qc = q < T ? q : T - 1;
    f16x8 qf[DS];
#pragma unroll
    for (int s = 0; s < DS; ++s) qf[s] = *reinterpret_cast<const f16x8*>(Qb + (long)qc * HD + 16 * s + 8 * h);

    // the mask row of this lane's query
    const long mrow = (((long)(b % Bm) * Hm + (Hm == 1 ? 0 : head)) * T + qc) * (long)T;
    const f16* m16 = reinterpret_cast<const f16*>(mask) + mrow;
    const float* m32 = reinterpret_cast<const float*>(mask) + mrow;
    const bool vec = (T & 3) == 0;        // rows start aligned and a run of four keys is wholly inside or outside T

    // ---- staging: chunk cid = tid + i * THREADS of the block is row cid / CH, 16-byte chunk cid % CH
    f16x8 kreg[PER], vreg[PER];
    auto load_block = [&](int k0) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int cid = tid + i * THREADS, row = cid / CH, c = cid - row * CH, key = k0 + row;
            f16x8 z = {(f16)0, (f16)0, (f16)0, (f16)0, (f16)0, (f16)0, (f16)0, (f16)0};
            kreg[i] = z;
            vreg[i] = z;
            if (cid < N_CH && key < T) {
                kreg[i] = *reinterpret_cast<const f16x8*>(Kb + (long)key * HD + c * 8);
                vreg[i] = *reinterpret_cast<const f16x8*>(Vb + (long)key * HD + c * 8);
            }
        }
    };
    auto store_block = [&]() {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int cid = tid + i * THREADS, row = cid / CH, c = cid - row * CH;
            if (cid < N_CH) {
                *reinterpret_cast<f16x8*>(sk + row * ROW + am_k_swz<HD>(row, c) * 16) = kreg[i];
                *reinterpret_cast<f16x8*>(sv + row * ROW + am_v_swz<HD>(row, c) * 16) = vreg[i];
            }
        }
    };

    // loop-invariant LDS offsets: K fragment of d-step s = row r, chunk 2 s + h; V^T transposed reads as in kernels_attn.hip (16-lane
    // group g covers d = 16 (g & 1) .. +15 of key half g >> 1 == h; lane 4 t + p of the group supplies key row t, columns 4 p .. +3)
    int k_off[DS], v_off[DB];
#pragma unroll
    for (int s = 0; s < DS; ++s) k_off[s] = r * ROW + am_k_swz<HD>(r, 2 * s + h) * 16;
    {
        const int key = 4 * h + ((lane & 15) >> 2), dd = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
#pragma unroll
        for (int db = 0; db < DB; ++db) v_off[db] = key * ROW + am_v_swz<HD>(key, (dd + 32 * db) >> 3) * 16 + (dd & 7) * 2;
    }

    f32x16 o[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[db][e] = 0.0f;
    float m_run = -1e30f, l_run = 0.0f; // finite floor: see the header
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    const int n_blocks = (T + 31) / 32;
    load_block(0);
    for (int kb = 0; kb < n_blocks; ++kb) {
        const int k0 = kb * 32;
        __syncthreads(); // every wave is done with block kb - 1
        store_block();
        __syncthreads();
        if (kb + 1 < n_blocks) load_block(k0 + 32);
        if (!active) continue;

        f32x16 s = zero;
#pragma unroll
        for (int st = 0; st < DS; ++st) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(sk + k_off[st]), qf[st], s, 0, 0, 0);

        // + mask * log2(e); -inf behind T
        float mloc = -INFINITY;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int key = k0 + 8 * g + 4 * h;
            float mv[4];
            if (vec) {
                if (key < T) {
                    if (mask_f32) {
                        const f32x4 t4 = *reinterpret_cast<const f32x4*>(m32 + key);
#pragma unroll
                        for (int j = 0; j < 4; ++j) mv[j] = t4[j];
                    } else {
                        const f16x4 t4 = *reinterpret_cast<const f16x4*>(m16 + key);
#pragma unroll
                        for (int j = 0; j < 4; ++j) mv[j] = (float)t4[j];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) mv[j] = -INFINITY;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) mv[j] = key + j < T ? (mask_f32 ? m32[key + j] : (float)m16[key + j]) : -INFINITY;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = fmaf(mv[j], AM_LOG2E, s[4 * g + j]);
                s[4 * g + j] = v;
                mloc = fmaxf(mloc, v);
            }
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

    if (!active || q >= T) return;
    const float inv = 1.0f / (l_run + other_half(l_run));
    f16* orow = O + ((long)b * T + q) * (H * HD) + head * HD;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) { // accumulator rows d = 32 db + 8 g + 4 h + j
            f16x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (f16)(o[db][g * 4 + j] * inv);
            *reinterpret_cast<f16x4*>(orow + db * 32 + 8 * g + 4 * h) = v;
        }
}

template <int HD>
void launch_masked(const f16* q, const f16* k, const f16* v, const void* mask, f16* out, int B, int H, int T, int Hm, int Bm, int mask_f32, hipStream_t s) {
    const int qblocks = (T + 31) / 32, nw = qblocks >= 3 ? 4 : qblocks; // short windows: a block per 32 / 64 queries
    const dim3 grid((unsigned)((T + 32 * nw - 1) / (32 * nw)) * B * H);
    switch (nw) {
        case 1: hipLaunchKernelGGL((attention_masked_kernel<HD, 1>), grid, dim3(64), 0, s, q, k, v, mask, out, H, T, Hm, Bm, mask_f32); break;
        case 2: hipLaunchKernelGGL((attention_masked_kernel<HD, 2>), grid, dim3(128), 0, s, q, k, v, mask, out, H, T, Hm, Bm, mask_f32); break;
        default: hipLaunchKernelGGL((attention_masked_kernel<HD, 4>), grid, dim3(256), 0, s, q, k, v, mask, out, H, T, Hm, Bm, mask_f32); break;
    }
}

} // namespace

extern "C" int vx_attention_masked_f16(const void* q, const void* k, const void* v, const void* mask, void* out, int B, int H, int T, int head_dim, int Hm,
                                       int Bm, int mask_is_f32, void* stream) {
    VX_REQUIRE(q && k && v && mask && out && B > 0 && H > 0 && T > 0, "vx_attention_masked_f16: empty problem");
    VX_REQUIRE(head_dim == 32 || head_dim == 64, "vx_attention_masked_f16: head_dim %d (32 and 64 are built)", head_dim);
    VX_REQUIRE(Hm == 1 || Hm == H, "vx_attention_masked_f16: the mask has %d heads (1 or %d)", Hm, H);
    VX_REQUIRE(Bm > 0 && B % Bm == 0, "vx_attention_masked_f16: the mask's batch %d does not divide %d", Bm, B);
    VX_REQUIRE((long)((T + 127) / 128) * B * H < (1L << 31), "vx_attention_masked_f16: too many blocks");
    const f16 *qp = reinterpret_cast<const f16*>(q), *kp = reinterpret_cast<const f16*>(k), *vp = reinterpret_cast<const f16*>(v);
    if (head_dim == 32) launch_masked<32>(qp, kp, vp, mask, reinterpret_cast<f16*>(out), B, H, T, Hm, Bm, mask_is_f32 ? 1 : 0, as_stream(stream));
    else launch_masked<64>(qp, kp, vp, mask, reinterpret_cast<f16*>(out), B, H, T, Hm, Bm, mask_is_f32 ? 1 : 0, as_stream(stream));
    VX_LAUNCH_CHECK();
    return 1;
}
