// Multi-head self-attention with an additive mask, head_dim 32 and 64, any number of tokens, on the matrix cores of gfx950:
// softmax(scale * q k^T + mask) v -- the graph layer's ATTENTION_MASKED op (reference src/visp/nn.cpp:210-244 with a mask, as
// swin::window_attention calls it, src/visp/arch/swin.cpp:69-97: mask = relative position bias [+ the shifted-window mask]).
//
// q, k, v f16 head-major [B * H][T][HD], q already multiplied by scale * log2(e) (VX_ATTN_Q_SCALE, as for vx_attention_f16);
// mask f16 or f32 [Bm][Hm][T queries][T keys] (keys contiguous), Hm in {1, H}, batch b reads image b % Bm; out f16 [B][T][H * HD].
// The 32-key block step -- orientation, accumulator layout, LDS tile, online softmax -- is vx_attn_tile.h's. A lane's 16 keys of a
// block are runs of four consecutive keys, so the mask row of the lane's query loads as four 8-byte (f16) / 16-byte (f32) pieces per
// key block when T is a multiple of 4 (rows are then aligned), element by element otherwise.
//   * keys >= T score -inf (P exactly 0), queries >= T are computed on a clamped row and not stored;
//   * the shift masks make whole 32-key blocks -inf for a query before it has seen anything: the finite floor of the running maximum
//     (vx_attn_tile.h) is what keeps those from NaN;
//   * a query whose mask is -inf on EVERY key has l = 0: its output row is unspecified (the reference gives NaN).
#include "vx_common.h"
#include "vx_attn_tile.h"

namespace {

template <int HD, int NW>
__global__ __launch_bounds__(64 * NW) void attention_masked_kernel(const f16* __restrict__ Q, const f16* __restrict__ K, const f16* __restrict__ V,
                                                                   const void* __restrict__ mask, f16* __restrict__ O, int H, int T, int Hm, int Bm,
                                                                   int mask_f32) {
    using G = attn_tile<HD>;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * G::BYTES];
    unsigned char* const sk = smem;
    unsigned char* const sv = smem + G::BYTES;

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
    f16x8 qf[G::DS];
#pragma unroll
    for (int s = 0; s < G::DS; ++s) qf[s] = *reinterpret_cast<const f16x8*>(Qb + (long)qc * HD + 16 * s + 8 * h);

    // the mask row of this lane's query
    const long mrow = (((long)(b % Bm) * Hm + (Hm == 1 ? 0 : head)) * T + qc) * (long)T;
    const f16* m16 = reinterpret_cast<const f16*>(mask) + mrow;
    const float* m32 = reinterpret_cast<const float*>(mask) + mrow;
    const bool vec = (T & 3) == 0;        // rows start aligned and a run of four keys is wholly inside or outside T

    f16x8 kreg[attn_stage<HD, NW>::PER], vreg[attn_stage<HD, NW>::PER];
    // loop-invariant LDS offsets: K fragment of d-step s = row r, chunk 2 s + h; V^T transposed reads of O^T block db, k-step 0 (vx_attn_tile.h)
    int k_off[G::DS], v_off[G::DB];
#pragma unroll
    for (int s = 0; s < G::DS; ++s) k_off[s] = r * G::ROW + attn_k_swz<HD>(r, 2 * s + h) * 16;
    {
        const int key = 4 * h + ((lane & 15) >> 2), dd = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
#pragma unroll
        for (int db = 0; db < G::DB; ++db) v_off[db] = key * G::ROW + attn_v_swz<HD>(key, (dd + 32 * db) >> 3) * 16 + (dd & 7) * 2;
    }
    f32x16 o[G::DB];
#pragma unroll
    for (int db = 0; db < G::DB; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[db][e] = 0.0f;
    float m_run = ATTN_M_FLOOR, l_run = 0.0f;

    const int n_blocks = (T + 31) / 32;
    attn_kv_load<HD, NW>(tid, kreg, vreg, Kb, Vb, HD, 0, T);
    for (int kb = 0; kb < n_blocks; ++kb) {
        const int k0 = kb * 32;
        attn_kv_store_sync<HD, NW>(tid, kreg, vreg, sk, sv);
        if (kb + 1 < n_blocks) attn_kv_load<HD, NW>(tid, kreg, vreg, Kb, Vb, HD, k0 + 32, T);
        if (!active) continue;

        f32x16 s = attn_scores<HD>(sk, k_off, qf);

        // + mask * log2(e); -inf behind T
        float mloc = -INFINITY;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int key = k0 + attn_key_of(4 * g, h);
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
                const float v = fmaf(mv[j], ATTN_LOG2E, s[4 * g + j]);
                s[4 * g + j] = v;
                mloc = fmaxf(mloc, v);
            }
        }
        attn_softmax_pv<HD>(s, mloc, m_run, l_run, o, sv, v_off);
    }

    if (!active || q >= T) return;
    const float inv = 1.0f / (l_run + other_half(l_run));
    f16* orow = O + ((long)b * T + q) * (H * HD) + head * HD;
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
