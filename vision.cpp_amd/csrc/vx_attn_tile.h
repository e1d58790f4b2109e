// The 32-key block step of the MFMA flash-attention kernels that stage K / V through registers into LDS: kernels_attn_mask.hip,
// kernels_attn_cross.hip and kernels_attn_relpos.hip (include after vx_common.h). What a tile's writers and readers must agree on is
// defined here once; a kernel keeps how it addresses its operands and what it adds to a score.
//
// Orientation. One block = NW wave64 = 32 NW queries of one (batch, head); a wave owns 32 queries. "Swapped" product, as in
// kernels_attn.hip and kernels_winattn.hip: S^T = K Q^T on v_mfma_f32_32x32x16_f16 (HD / 16 d-steps; head_dim 16 is exactly one), so
//   * a lane owns ONE query column r = lane & 31, and lanes l and l + 32 own the same query (other_half() joins their maxima and sums);
//   * accumulator element e of half h = lane >> 5 is key attn_key_of(e, h) = 8 (e >> 2) + 4 h + (e & 3) of the 32-key block: 16 keys
//     per lane in runs of four consecutive keys.
// The softmax is online over the 32-key blocks in the exp2 domain (scores arrive already multiplied by log2 e). P^T feeds
// O^T = V^T P^T straight from the accumulators: element j of k-step ks is key 16 ks + 8 (j >> 2) + 4 h + (j & 3), and the V^T
// fragments come from ds_read_b64_tr_b16 (16-lane group g covers d = 16 (g & 1) .. +15 of key half g >> 1 == h; lane 4 t + p of the
// group supplies key row t, columns 4 p .. +3). Accumulator row g * 4 + j of O^T block db is d = 32 db + 8 g + 4 h + j.
//   * At head_dim 16 the transposed reads of lanes 16..31 of a half fetch d = 0..15 again: rows 16..31 of O^T are computed and never
//     stored (G_OUT = 2 row groups instead of 4).
//   * The running maximum starts at a finite floor (ATTN_M_FLOOR = -1e30), not -inf: a 32-key block that is all -inf for a query while
//     nothing has been seen yet gives exp2(-inf - (-1e30)) = 0, never exp2(-inf - (-inf)) = NaN.
//
// The LDS tile. K and V blocks (32 keys x HD f16, rows of ROW = 2 HD bytes, CH = HD / 8 16-byte chunks each) go through registers
// into one K tile and one V tile shared by the block; rows at or behind the end key are zeros (their P is exactly 0, and 0 * 0 is not
// NaN). The next block's global loads are issued right after the tile is written and stay in flight under the MFMAs. Both images are
// swizzled: K by 16-byte chunk ^ row bits, so the ds_read_b128 of 32 rows spread over the banks (swz128 at head_dim 64); V at
// head_dim 64 by chunk ^ 4 on odd row pairs, for the transposed reads.
#pragma once

constexpr float ATTN_LOG2E = 1.44269504088896340736f;
constexpr float ATTN_M_FLOOR = -1e30f;

typedef __fp16 hv4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

template <int HD>
struct attn_tile {
    static_assert(HD == 16 || HD == 32 || HD == 64, "head_dim 16, 32 and 64 are built");
    static constexpr int ROW = HD * 2;            // bytes per K / V row in LDS
    static constexpr int CH = HD / 8;             // 16-byte chunks per row
    static constexpr int N_CH = 32 * CH;          // chunks per 32-key block
    static constexpr int BYTES = 32 * ROW;        // one K (or V) tile
    static constexpr int DS = HD / 16;            // d-steps of a product with Q
    static constexpr int DB = HD == 64 ? 2 : 1;   // 32-row blocks of O^T
    static constexpr int G_OUT = HD == 16 ? 2 : 4; // groups of four accumulator rows that hold real d
};

template <int HD>
__device__ __forceinline__ int attn_k_swz(int row, int chunk) { return HD == 64 ? swz128(row, chunk) : (HD == 32 ? chunk ^ ((row >> 2) & 3) : chunk); }
template <int HD>
__device__ __forceinline__ int attn_v_swz(int row, int chunk) { return HD == 64 ? chunk ^ (((row >> 1) & 1) << 2) : chunk; }

// accumulator element e of half h -> key within a 32-block
__device__ __forceinline__ int attn_key_of(int e, int h) { return 8 * (e >> 2) + 4 * h + (e & 3); }

// ---- K / V staging: chunk cid = tid + i * 64 NW of the block is row cid / CH, 16-byte chunk cid % CH; PER chunks of K and of V per thread.
// With more threads than chunks (head_dim 16 / 32 at 256 threads) cid needs its test; otherwise the test is compiled out.
template <int HD, int NW>
struct attn_stage {
    static constexpr int THREADS = 64 * NW;
    static constexpr int PER = (attn_tile<HD>::N_CH + THREADS - 1) / THREADS;
    static constexpr bool RAGGED = attn_tile<HD>::N_CH % THREADS != 0;
};

// keys k0 .. k0 + 31 into registers, zeros from k_end on; ld = elements between key rows
template <int HD, int NW>
__device__ __forceinline__ void attn_kv_load(const int& tid, f16x8 (&kreg)[attn_stage<HD, NW>::PER], f16x8 (&vreg)[attn_stage<HD, NW>::PER], const f16* Kb, const f16* Vb,
                                             long ld, int k0, int k_end) {
    using S = attn_stage<HD, NW>;
    constexpr int CH = attn_tile<HD>::CH;
#pragma unroll
    for (int i = 0; i < S::PER; ++i) {
        const int cid = tid + i * S::THREADS, row = cid / CH, c = cid - row * CH, key = k0 + row;
        f16x8 z = {(f16)0, (f16)0, (f16)0, (f16)0, (f16)0, (f16)0, (f16)0, (f16)0};
        kreg[i] = z;
        vreg[i] = z;
        if ((!S::RAGGED || cid < attn_tile<HD>::N_CH) && key < k_end) {
            kreg[i] = *reinterpret_cast<const f16x8*>(Kb + (long)key * ld + c * 8);
            vreg[i] = *reinterpret_cast<const f16x8*>(Vb + (long)key * ld + c * 8);
        }
    }
}

// the staged block into the swizzled tiles, between the two block-wide barriers of a step: every thread of the block calls it
template <int HD, int NW>
__device__ __forceinline__ void attn_kv_store_sync(const int& tid, const f16x8 (&kreg)[attn_stage<HD, NW>::PER], const f16x8 (&vreg)[attn_stage<HD, NW>::PER],
                                                   unsigned char* sk, unsigned char* sv) {
    using S = attn_stage<HD, NW>;
    constexpr int CH = attn_tile<HD>::CH, ROW = attn_tile<HD>::ROW;
    __syncthreads(); // every wave is done with the previous block
#pragma unroll
    for (int i = 0; i < S::PER; ++i) {
        const int cid = tid + i * S::THREADS, row = cid / CH, c = cid - row * CH;
        if (!S::RAGGED || cid < attn_tile<HD>::N_CH) {
            *reinterpret_cast<f16x8*>(sk + row * ROW + attn_k_swz<HD>(row, c) * 16) = kreg[i];
            *reinterpret_cast<f16x8*>(sv + row * ROW + attn_v_swz<HD>(row, c) * 16) = vreg[i];
        }
    }
    __syncthreads();
}

// S^T = K Q^T of the staged block
template <int HD>
__device__ __forceinline__ f32x16 attn_scores(const unsigned char* sk, const int (&k_off)[attn_tile<HD>::DS], const f16x8 (&qf)[attn_tile<HD>::DS]) {
    f32x16 s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < attn_tile<HD>::DS; ++st) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(sk + k_off[st]), qf[st], s, 0, 0, 0);
    return s;
}

// online softmax update and O^T += V^T P^T for the adjusted scores s (exp2 domain; -inf where there is no key) and the lane's own maximum of them
template <int HD>
__device__ __forceinline__ void attn_softmax_pv(f32x16& s, float mloc, float& m_run, float& l_run, f32x16 (&o)[attn_tile<HD>::DB], unsigned char* const& sv,
                                                const int (&v_off)[attn_tile<HD>::DB]) {
    using G = attn_tile<HD>;
    mloc = fmaxf(mloc, other_half(mloc)); // lanes l and l + 32 own the same query
    const float m_new = fmaxf(m_run, mloc);
    if (__any(m_new > m_run)) {
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        l_run *= alpha;
#pragma unroll
        for (int db = 0; db < G::DB; ++db)
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
    for (int ks = 0; ks < 2; ++ks) {
        f16x8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[j] = (f16)s[8 * ks + j];
#pragma unroll
        for (int db = 0; db < G::DB; ++db) {
            const unsigned char* vrow = sv + v_off[db] + ks * 16 * G::ROW;
            hv4 va = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) hv4*)(vrow));
            hv4 vb = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) hv4*)(vrow + 8 * G::ROW));
            f16x8 vf = {(f16)va[0], (f16)va[1], (f16)va[2], (f16)va[3], (f16)vb[0], (f16)vb[1], (f16)vb[2], (f16)vb[3]};
            o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o[db], 0, 0, 0);
        }
    }
}
