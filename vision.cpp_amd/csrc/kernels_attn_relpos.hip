// Multi-head self-attention with SAM's decomposed relative-position bias, head_dim 64, on the matrix cores of gfx950 -- the graph layer's
// ATTENTION_REL_POS op (transformers' SamVisionAttention / get_decomposed_rel_pos; segment-anything's add_decomposed_rel_pos):
//   out = softmax(scale q k^T + bias) v,   bias[(qy, qx), (ky, kx)] = q . rel_h[qy - ky + gh - 1] + q . rel_w[qx - kx + gw - 1]
// over the T = gw * gh tokens of a grid in row-major order, the bias from the UNSCALED q. Nothing of size T x T exists outside registers.
//
// q, k, v f16 [B][T][H][64] -- token-major rows of H * 64, where the graph has them; rel_h f16 [2 gh - 1][64], rel_w f16 [2 gw - 1][64], shared by all heads;
// out f16 [B][T][H * 64]. The orientation is that of kernels_attn_cross.hip: one block = NW wave64 = 32 NW queries of one (batch, head), S^T = K Q^T on
// v_mfma_f32_32x32x16_f16, so a lane owns ONE query column r = lane & 31 and 16 keys of a 32-key block (key = 8 (e >> 2) + 4 (lane >> 5) + (e & 3)); online
// softmax in the exp2 domain with the finite running-maximum floor; P^T feeds O^T = V^T P^T from the accumulators, V^T through ds_read_b64_tr_b16.
//
// The bias. It is the sum of a part that depends on (query, key ROW) and a part that depends on (query, key COLUMN): per query only gh + gw numbers, not T.
// Before the key loop every wave makes them for its 32 queries with the matrix cores and keeps them in its own slice of LDS:
//   * D^T = Rel Q^T: the A operand is a 32-row slab of a table read straight from global memory (rows past the table's end clamp to its last row and are never
//     used), the B operand the Q fragments the score product uses anyway. A lane gets q . rel[j] for its query and 16 table rows j per slab; at most four
//     slabs per table cover the 2 g - 1 <= 127 rows: 32 MFMAs per wave once, against 8 per key block in the loop.
//   * the skew is undone on the way INTO LDS: entry j of query position p belongs to key position kk = p + g - 1 - j, and the lane stores it (times log2 e, in
//     f32: no second number format) at RH[r][kk] / RW[r][kk] if 0 <= kk < g. Every (query, kk) is written exactly once. Rows are padded to an odd number of
//     floats (g | 1), so the 32 query rows of a wave fall into 32 different banks whichever kk they ask for.
// In the loop a score is  acc * (scale log2 e) + (RH[r][ky] + RW[r][kx])  -- one add, one fma. Two forms, chosen by the launcher:
//   generic   any gw, gh in 1..64 (SAM's 14 x 14 windows, every small or non-square grid): key blocks straddle grid rows, so each of the 16 keys of a lane looks
//             up (ky, kx) = (key / gw, key % gw) -- the division as one f32 multiply, exact for key < 4096 -- and reads its two floats from LDS.
//   aligned   gw == 64 (the global layers of a 1024^2 image, 64 x 64): a 32-key block is half a grid row. ky is the same for the whole block: ONE LDS read per
//             lane per block. kx is 32 (block & 1) + the lane's 16 offsets: the RW part is loop-invariant, read out of LDS once into 2 x 16 registers in the
//             accumulator's own layout; the loop is unrolled by the two phases so the register file is indexed statically.
// K / V staging is the cross kernel's: 32-key blocks through registers into one swizzled LDS tile, the next block's global loads in flight under the MFMAs.
// No atomics, no workspace; the same bits on every run.
#include "vx_common.h"

#include <type_traits>

namespace {

constexpr float RP_LOG2E = 1.44269504088896340736f;
constexpr int RP_HD = 64;
constexpr int RP_ROW = RP_HD * 2;      // bytes per K / V row in LDS
constexpr int RP_TILE = 32 * RP_ROW;   // bytes of one 32-key K (or V) tile

typedef __fp16 hv4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

__device__ __forceinline__ int rp_k_swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }
__device__ __forceinline__ int rp_v_swz(int row, int chunk) { return chunk ^ (((row >> 1) & 1) << 2); }
__device__ __forceinline__ int rp_key_of(int e, int h) { return 8 * (e >> 2) + 4 * h + (e & 3); } // accumulator element e of half h -> key (table row) within a 32-block

__host__ __device__ constexpr int rp_stride(int g) { return g | 1; } // floats per query row of a bias table in LDS: odd, so rows land in different banks

template <bool ALIGNED, int NW>
__global__ __launch_bounds__(64 * NW) void attention_relpos_kernel(const f16* __restrict__ Q, const f16* __restrict__ K, const f16* __restrict__ V,
                                                                   const f16* __restrict__ RelH, const f16* __restrict__ RelW, f16* __restrict__ O, int H, int gw,
                                                                   int gh, float qs) {
    constexpr int CH = RP_HD / 8;          // 16-byte chunks per row
    constexpr int N_CH = 32 * CH;          // chunks per 32-key block
    constexpr int THREADS = 64 * NW;
    constexpr int PER = N_CH / THREADS;    // 4, 2, 1
    constexpr int DS = RP_HD / 16;         // d-steps of a product with Q
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const sk = smem;
    unsigned char* const sv = smem + RP_TILE;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int T = gw * gh;
    const int n_qblk = (T + 32 * NW - 1) / (32 * NW);
    const int bh = blockIdx.x / n_qblk;    // b * H + head
    const int q0 = (blockIdx.x - bh * n_qblk) * (32 * NW) + wave * 32;
    const int b = bh / H, head = bh - b * H;
    const bool active = q0 < T;            // wave-uniform: a wave without queries only stages K / V and keeps the barriers
    const long ld = (long)H * RP_HD;       // elements between token rows
    const int SH = rp_stride(gh), SW = rp_stride(gw);
    float* const rh_row = reinterpret_cast<float*>(smem + 2 * RP_TILE) + (wave * 32 + r) * (SH + SW); // this lane's query: RH[0 .. gh) then RW[0 .. gw)
    float* const rw_row = rh_row + SH;

    const f16* Qb = Q + (long)b * T * ld + head * RP_HD;
    const f16* Kb = K + (long)b * T * ld + head * RP_HD;
    const f16* Vb = V + (long)b * T * ld + head * RP_HD;

    const int q = q0 + r;
    const int qc = q < T ? q : T - 1;      // (an inactive wave never dereferences it)
    f16x8 qf[DS];
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float rw_reg[2][16]; // ALIGNED: the loop-invariant RW part of the two half-row phases, in the accumulator's layout

    if (active) {
#pragma unroll
        for (int s = 0; s < DS; ++s) qf[s] = *reinterpret_cast<const f16x8*>(Qb + (long)qc * ld + 16 * s + 8 * h);
        // ---- the bias tables of this wave's 32 queries: D^T = Rel Q^T per 32-row slab, stored de-skewed
        const int qy = qc / gw, qx = qc - qy * gw;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const f16* rel = t == 0 ? RelH : RelW;
            const int g = t == 0 ? gh : gw, pos = t == 0 ? qy : qx;
            float* const dst = t == 0 ? rh_row : rw_row;
            const int n_rows = 2 * g - 1;
            for (int j0 = 0; j0 < n_rows; j0 += 32) {
                const int row = min(j0 + r, n_rows - 1);
                f32x16 d = zero;
#pragma unroll
                for (int s = 0; s < DS; ++s)
                    d = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(rel + row * RP_HD + 16 * s + 8 * h), qf[s], d, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int kk = pos + g - 1 - (j0 + rp_key_of(e, h)); // >= 0 implies the table row exists
                    if (kk >= 0 && kk < g) dst[kk] = d[e] * RP_LOG2E;
                }
            }
        }
        if (ALIGNED) { // the stores above are this wave's own and LDS serves a wave in program order: no barrier between them and these reads
#pragma unroll
            for (int ph = 0; ph < 2; ++ph)
#pragma unroll
                for (int e = 0; e < 16; ++e) rw_reg[ph][e] = rw_row[32 * ph + rp_key_of(e, h)];
        }
    }

    // ---- staging: chunk cid = tid + i * THREADS of the block is row cid / CH, 16-byte chunk cid % CH
    f16x8 kreg[PER], vreg[PER];
    auto load_block = [&](int k0) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int cid = tid + i * THREADS, row = cid / CH, c = cid - row * CH, key = k0 + row;
            f16x8 z = {(f16)0, (f16)0, (f16)0, (f16)0, (f16)0, (f16)0, (f16)0, (f16)0};
            kreg[i] = z;
            vreg[i] = z;
            if (key < T) {
                kreg[i] = *reinterpret_cast<const f16x8*>(Kb + (long)key * ld + c * 8);
                vreg[i] = *reinterpret_cast<const f16x8*>(Vb + (long)key * ld + c * 8);
            }
        }
    };
    auto store_block = [&]() {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int cid = tid + i * THREADS, row = cid / CH, c = cid - row * CH;
            *reinterpret_cast<f16x8*>(sk + row * RP_ROW + rp_k_swz(row, c) * 16) = kreg[i];
            *reinterpret_cast<f16x8*>(sv + row * RP_ROW + rp_v_swz(row, c) * 16) = vreg[i];
        }
    };

    // loop-invariant LDS offsets: K fragment of d-step s = row r, chunk 2 s + h; V^T transposed reads as in kernels_attn_cross.hip
    int k_off[DS], v_off[2];
#pragma unroll
    for (int s = 0; s < DS; ++s) k_off[s] = r * RP_ROW + rp_k_swz(r, 2 * s + h) * 16;
    {
        const int key = 4 * h + ((lane & 15) >> 2), dd = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
#pragma unroll
        for (int db = 0; db < 2; ++db) v_off[db] = key * RP_ROW + rp_v_swz(key, (dd + 32 * db) >> 3) * 16 + (dd & 7) * 2;
    }

    f32x16 o[2] = {zero, zero};
    float m_run = -1e30f, l_run = 0.0f; // finite floor: a block that is all -inf while nothing has been seen gives exp2(-inf + 1e30) = 0, never NaN
    const float inv_gw = 1.0f / (float)gw;

    // one 32-key block: stage, scores, bias, online softmax, PV. PH: the half-row phase (ALIGNED; 0 otherwise)
    const int n_blocks = (T + 31) / 32;
    auto step = [&](int kb, auto phase) {
        constexpr int PH = decltype(phase)::value;
        const int k0 = kb * 32;
        __syncthreads(); // every wave is done with block kb - 1
        store_block();
        __syncthreads();
        if (kb + 1 < n_blocks) load_block(k0 + 32);
        if (!active) return;

        f32x16 s = zero;
#pragma unroll
        for (int st = 0; st < DS; ++st) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(sk + k_off[st]), qf[st], s, 0, 0, 0);

        float mloc = -INFINITY;
        const float rh_blk = ALIGNED ? rh_row[kb >> 1] : 0.0f; // ALIGNED: the block lies in grid row kb / 2
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int key = k0 + rp_key_of(e, h);
            float bias;
            if (ALIGNED) bias = rh_blk + rw_reg[PH][e];
            else {
                const int kc = min(key, T - 1);
                const int ky = (int)(((float)kc + 0.5f) * inv_gw); // exact: (kc + 0.5) / gw is at least 1 / 128 away from an integer, the f32 error below 1e-5
                bias = rh_row[ky] + rw_row[kc - ky * gw];
            }
            const float v = key < T ? fmaf(s[e], qs, bias) : -INFINITY;
            s[e] = v;
            mloc = fmaxf(mloc, v);
        }
        mloc = fmaxf(mloc, other_half(mloc)); // lanes l and l + 32 own the same query
        const float m_new = fmaxf(m_run, mloc);
        if (__any(m_new > m_run)) {
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            l_run *= alpha;
#pragma unroll
            for (int db = 0; db < 2; ++db)
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
            for (int db = 0; db < 2; ++db) {
                const unsigned char* vrow = sv + v_off[db] + ks * 16 * RP_ROW;
                hv4 va = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) hv4*)(vrow));
                hv4 vb = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) hv4*)(vrow + 8 * RP_ROW));
                f16x8 vf = {(f16)va[0], (f16)va[1], (f16)va[2], (f16)va[3], (f16)vb[0], (f16)vb[1], (f16)vb[2], (f16)vb[3]};
                o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o[db], 0, 0, 0);
            }
        }
    };

    load_block(0);
    if (ALIGNED) { // T = 64 gh: an even number of blocks
        for (int kb = 0; kb < n_blocks; kb += 2) {
            step(kb, std::integral_constant<int, 0>{});
            step(kb + 1, std::integral_constant<int, 1>{});
        }
    } else {
        for (int kb = 0; kb < n_blocks; ++kb) step(kb, std::integral_constant<int, 0>{});
    }

    if (!active || q >= T) return;
    const float inv = 1.0f / (l_run + other_half(l_run));
    f16* orow = O + ((long)b * T + q) * ld + head * RP_HD; // accumulator rows d = 32 db + 8 g + 4 h + j
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f16x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (f16)(o[db][g * 4 + j] * inv);
            *reinterpret_cast<f16x4*>(orow + db * 32 + 8 * g + 4 * h) = v;
        }
}

int rp_waves(int T) { const int qblocks = (T + 31) / 32; return qblocks >= 3 ? 4 : qblocks; } // few queries: a block per 32 / 64 of them
size_t rp_lds_bytes(int nw, int gw, int gh) { return 2 * RP_TILE + (size_t)nw * 32 * (rp_stride(gh) + rp_stride(gw)) * sizeof(float); }

template <bool ALIGNED, int NW>
int launch_relpos(const f16* q, const f16* k, const f16* v, const f16* rel_h, const f16* rel_w, f16* out, int B, int H, int gw, int gh, float qs, hipStream_t s) {
    const int T = gw * gh;
    const size_t lds = rp_lds_bytes(NW, gw, gh);
    VX_CHECK(vx_ensure_dynamic_lds(reinterpret_cast<const void*>(&attention_relpos_kernel<ALIGNED, NW>), (int)lds));
    const dim3 grid((unsigned)((T + 32 * NW - 1) / (32 * NW)) * B * H);
    hipLaunchKernelGGL((attention_relpos_kernel<ALIGNED, NW>), grid, dim3(64 * NW), lds, s, q, k, v, rel_h, rel_w, out, H, gw, gh, qs);
    return 1;
}

} // namespace

extern "C" int vx_attention_relpos_aligned(int gw, int gh) { return gw == 64 && gh >= 1 && gh <= 64 ? 1 : 0; }

extern "C" int vx_attention_relpos_f16(const void* q, const void* k, const void* v, const void* rel_h, const void* rel_w, void* out, int B, int H, int gw, int gh,
                                       int head_dim, float scale, void* stream) {
    VX_REQUIRE(q && k && v && rel_h && rel_w && out && B > 0 && H > 0, "vx_attention_relpos_f16: empty problem");
    VX_REQUIRE(head_dim == 64, "vx_attention_relpos_f16: head_dim %d (64 is built: ViT-B and ViT-L; ViT-H's 80 is not)", head_dim);
    VX_REQUIRE(gw >= 1 && gw <= 64 && gh >= 1 && gh <= 64, "vx_attention_relpos_f16: grid %d x %d (1..64 each way)", gw, gh);
    VX_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(rel_h) && aligned16(rel_w) && ((reinterpret_cast<uintptr_t>(out) & 7) == 0),
               "vx_attention_relpos_f16: q, k, v and the tables must be 16-byte aligned, out 8-byte aligned");
    const int T = gw * gh, nw = vx_attention_relpos_aligned(gw, gh) ? 4 : rp_waves(T);
    VX_REQUIRE((long)((T + 32 * nw - 1) / (32 * nw)) * B * H < (1L << 31), "vx_attention_relpos_f16: too many blocks");
    const f16 *qp = reinterpret_cast<const f16*>(q), *kp = reinterpret_cast<const f16*>(k), *vp = reinterpret_cast<const f16*>(v);
    const f16 *hp = reinterpret_cast<const f16*>(rel_h), *wp = reinterpret_cast<const f16*>(rel_w);
    f16* op = reinterpret_cast<f16*>(out);
    const float qs = scale * RP_LOG2E;
    hipStream_t s = as_stream(stream);
    int ok;
    if (vx_attention_relpos_aligned(gw, gh)) ok = launch_relpos<true, 4>(qp, kp, vp, hp, wp, op, B, H, gw, gh, qs, s); // T >= 64: gh == 1 has two query tiles
    else if (nw == 1) ok = launch_relpos<false, 1>(qp, kp, vp, hp, wp, op, B, H, gw, gh, qs, s);
    else if (nw == 2) ok = launch_relpos<false, 2>(qp, kp, vp, hp, wp, op, B, H, gw, gh, qs, s);
    else ok = launch_relpos<false, 4>(qp, kp, vp, hp, wp, op, B, H, gw, gh, qs, s);
    if (!ok) return 0;
    VX_LAUNCH_CHECK();
    return 1;
}
