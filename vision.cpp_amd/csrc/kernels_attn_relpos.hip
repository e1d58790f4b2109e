// Multi-head self-attention with SAM's decomposed relative-position bias, head_dim 64, on the matrix cores of gfx950 -- the graph layer's
// ATTENTION_REL_POS op (transformers' SamVisionAttention / get_decomposed_rel_pos; segment-anything's add_decomposed_rel_pos):
//   out = softmax(scale q k^T + bias) v,   bias[(qy, qx), (ky, kx)] = q . rel_h[qy - ky + gh - 1] + q . rel_w[qx - kx + gw - 1]
// over the T = gw * gh tokens of a grid in row-major order, the bias from the UNSCALED q. Nothing of size T x T exists outside registers.
//
// q, k, v f16 [B][T][H][64] -- token-major rows of H * 64, where the graph has them; rel_h f16 [2 gh - 1][64], rel_w f16 [2 gw - 1][64], shared by all heads;
// out f16 [B][T][H * 64]. The 32-key block step -- orientation, accumulator layout, LDS tile, online softmax -- is vx_attn_tile.h's: a lane owns ONE query
// column r = lane & 31 and the 16 keys attn_key_of(e, h) of a 32-key block.
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
// No atomics, no workspace; the same bits on every run.
#include "vx_common.h"
#include "vx_attn_tile.h"

#include <type_traits>

namespace {

constexpr int RP_HD = 64;
constexpr int RP_TILE = attn_tile<RP_HD>::BYTES; // one 32-key K (or V) tile

__host__ __device__ constexpr int rp_stride(int g) { return g | 1; } // floats per query row of a bias table in LDS: odd, so rows land in different banks

template <bool ALIGNED, int NW>
__global__ __launch_bounds__(64 * NW) void attention_relpos_kernel(const f16* __restrict__ Q, const f16* __restrict__ K, const f16* __restrict__ V,
                                                                   const f16* __restrict__ RelH, const f16* __restrict__ RelW, f16* __restrict__ O, int H, int gw,
                                                                   int gh, float qs) {
    using G = attn_tile<RP_HD>;
    constexpr int DS = G::DS;
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
                    const int kk = pos + g - 1 - (j0 + attn_key_of(e, h)); // >= 0 implies the table row exists
                    if (kk >= 0 && kk < g) dst[kk] = d[e] * ATTN_LOG2E;
                }
            }
        }
        if (ALIGNED) { // the stores above are this wave's own and LDS serves a wave in program order: no barrier between them and these reads
#pragma unroll
            for (int ph = 0; ph < 2; ++ph)
#pragma unroll
                for (int e = 0; e < 16; ++e) rw_reg[ph][e] = rw_row[32 * ph + attn_key_of(e, h)];
        }
    }

    f16x8 kreg[attn_stage<RP_HD, NW>::PER], vreg[attn_stage<RP_HD, NW>::PER];
    // loop-invariant LDS offsets: K fragment of d-step s = row r, chunk 2 s + h; V^T transposed reads of O^T block db, k-step 0 (vx_attn_tile.h)
    int k_off[G::DS], v_off[G::DB];
#pragma unroll
    for (int s = 0; s < G::DS; ++s) k_off[s] = r * G::ROW + attn_k_swz<RP_HD>(r, 2 * s + h) * 16;
    {
        const int key = 4 * h + ((lane & 15) >> 2), dd = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
#pragma unroll
        for (int db = 0; db < G::DB; ++db) v_off[db] = key * G::ROW + attn_v_swz<RP_HD>(key, (dd + 32 * db) >> 3) * 16 + (dd & 7) * 2;
    }
    f32x16 o[G::DB] = {zero, zero};
    float m_run = ATTN_M_FLOOR, l_run = 0.0f;
    const float inv_gw = 1.0f / (float)gw;

    // one 32-key block: stage, scores, bias, online softmax, PV. PH: the half-row phase (ALIGNED; 0 otherwise)
    const int n_blocks = (T + 31) / 32;
    auto step = [&](int kb, auto phase) {
        constexpr int PH = decltype(phase)::value;
        const int k0 = kb * 32;
        attn_kv_store_sync<RP_HD, NW>(tid, kreg, vreg, sk, sv);
        if (kb + 1 < n_blocks) attn_kv_load<RP_HD, NW>(tid, kreg, vreg, Kb, Vb, ld, k0 + 32, T);
        if (!active) return;

        f32x16 s = attn_scores<RP_HD>(sk, k_off, qf);
        float mloc = -INFINITY;
        const float rh_blk = ALIGNED ? rh_row[kb >> 1] : 0.0f; // ALIGNED: the block lies in grid row kb / 2
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int key = k0 + attn_key_of(e, h);
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
        attn_softmax_pv<RP_HD>(s, mloc, m_run, l_run, o, sv, v_off);
    };

    attn_kv_load<RP_HD, NW>(tid, kreg, vreg, Kb, Vb, ld, 0, T);
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
    f16* orow = O + ((long)b * T + q) * ld + head * RP_HD;
#pragma unroll
    for (int db = 0; db < G::DB; ++db)
#pragma unroll
        for (int g = 0; g < G::G_OUT; ++g) { // accumulator rows d = 32 db + 8 g + 4 h + j
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
    const float qs = scale * ATTN_LOG2E;
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
