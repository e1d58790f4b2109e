// YOLOv9t's non_max_suppression on the device (csrc/yolov9t.cpp nms_candidates is the host statement it owes its decisions to, bit for bit):
// multi-label candidates as vx_yolo_decode leaves them, in any order, -> at most max_det visp_detection rows per image and their count.
//   yolo_nms_rank_kernel   rank by counting. (score bits, idx) is one 64-bit key: scores are non-negative, so their bit patterns order as the
//                          values do, and idx is unique in a list, so the keys are distinct and "the keys above mine" IS the rank in
//                          (score descending, idx ascending). A block stages a tile of the image's keys in LDS and every thread counts the
//                          keys that precede its own candidate: any n, no sort network, the same ranks for every order of the list. Ranks
//                          below min(n, max_nms) scatter the box with its class offset, the score and idx to the ranked workspace.
//   yolo_nms_scan_kernel   the greedy pass, one block per image. The kept boxes live in LDS (at most max_det float4, read by all lanes at one
//                          address: a broadcast). A round takes 256 ranked candidates, one per lane: every lane tests its box against the
//                          kept list, then the four waves resolve in rank order -- against what the earlier waves of the round appended, then
//                          inside the wave through 64-bit suppression words (lane broadcast + ballot) resolved on the scalar side with
//                          readlane, no memory in the chain. The block leaves once max_det rows are kept or the ranked list ends: at most
//                          n * max_det IoUs, never n^2.
// The IoU keeps the host's float32 operations in the host's order: contraction off, IEEE division, std::min / std::max spelled out, and this
// object is built without the packed f32 forms (csrc/Makefile). No atomics, no scratch; every result leaves through a vector store.
#include "vx_common.h"

namespace {

constexpr int NMS_MAX_DET = 4096; // rows of the kept list in LDS: 4096 float4 = 64 KiB
constexpr int RANK_TILE = 1024;   // keys staged per LDS tile (8 KiB)
constexpr int RANK_BLOCKS = 128;  // blocks per image of the rank grid; each strides over the 256-candidate groups of its image

typedef unsigned long long u64;

struct nms_ws {
    float4* rbox;  // [B][M] ranked boxes, class offset applied
    float2* rmeta; // [B][M] {score, idx as bits}
};
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline long ranked_rows(int A, int nc, int max_nms) { return (long)A * nc < (long)max_nms ? (long)A * nc : (long)max_nms; }
inline size_t nms_ws_layout(int B, long M, nms_ws* w, uint8_t* base) {
    const size_t o_meta = up256((size_t)B * M * 16);
    if (w) *w = {reinterpret_cast<float4*>(base), reinterpret_cast<float2*>(base + o_meta)};
    return o_meta + up256((size_t)B * M * 8);
}

__device__ __forceinline__ int list_length(const int* __restrict__ cand_count, int b, int cap) { return min(max(cand_count[b], 0), cap); }
__device__ __forceinline__ u64 rank_key(float score, int idx) { return ((u64)__float_as_uint(score) << 32) | (0xffffffffu - (unsigned)idx); }

// grid (RANK_BLOCKS, B). Candidate c of image b is preceded by every candidate of b with a larger key; a tile slot behind the list holds key 0, which
// is above nobody (a real key is at least 1: idx < 2^32 - 1).
__global__ __launch_bounds__(256) void yolo_nms_rank_kernel(const float* __restrict__ boxes, const int* __restrict__ cand_count, const int* __restrict__ cand_idx,
                                                            const float* __restrict__ cand_score, int A, int nc, int max_nms, int max_wh, long M,
                                                            float4* __restrict__ rbox, float2* __restrict__ rmeta) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) u64 tile[RANK_TILE];
    const int b = blockIdx.y, tid = threadIdx.x, cap = A * nc, n = list_length(cand_count, b, cap), kept_ranks = min(n, max_nms);
    const int* idx_b = cand_idx + (long)b * cap;
    const float* score_b = cand_score + (long)b * cap;
    for (int c0 = blockIdx.x * 256; c0 < n; c0 += RANK_BLOCKS * 256) { // block-uniform
        const int c = c0 + tid;
        const bool mine = c < n;
        const int idx = mine ? idx_b[c] : 0;
        const float score = mine ? score_b[c] : 0.0f;
        const u64 key = mine ? rank_key(score, idx) : ~0ull;
        int before = 0;
        for (int t0 = 0; t0 < n; t0 += RANK_TILE) {
            __syncthreads(); // the tile of the round before is read out
            for (int j = tid; j < RANK_TILE; j += 256) tile[j] = t0 + j < n ? rank_key(score_b[t0 + j], idx_b[t0 + j]) : 0ull;
            __syncthreads();
            const int len = min(RANK_TILE, (n - t0 + 1) & ~1); // whole pairs: the slot behind an odd list is a zero key
            for (int j = 0; j < len; j += 2) {                 // all lanes at one address: two keys per 16-byte LDS read
                const ulonglong2 k = *reinterpret_cast<const ulonglong2*>(&tile[j]);
                before += (k.x > key) + (k.y > key);
            }
        }
        if (mine && before < kept_ranks) {
            const int anchor = min((int)((unsigned)idx / (unsigned)nc), A - 1), cls = (int)((unsigned)idx % (unsigned)nc); // an idx outside the list's range reads in bounds
            const float4 bx = reinterpret_cast<const float4*>(boxes)[(long)b * A + anchor];
            const float off = (float)(cls * max_wh);
            rbox[b * M + before] = make_float4(bx.x + off, bx.y, bx.z + off, bx.w);
            rmeta[b * M + before] = make_float2(score, __int_as_float(idx));
        }
    }
}

// overlap_ratio of nms_candidates: a = the earlier (kept) box, b = the later one
__device__ __forceinline__ float host_max(float a, float b) { return a < b ? b : a; } // std::max
__device__ __forceinline__ float host_min(float a, float b) { return b < a ? b : a; } // std::min
__device__ __forceinline__ bool suppresses(float4 a, float4 b, float iou) {
#pragma clang fp contract(off)
    const float ow = host_max(0.0f, host_min(a.z, b.z) - host_max(a.x, b.x));
    const float oh = host_max(0.0f, host_min(a.w, b.w) - host_max(a.y, b.y));
    const float common = ow * oh;
    const float both = (a.z - a.x) * (a.w - a.y) + (b.z - b.x) * (b.w - b.y) - common;
    const float ratio = both > 0.0f ? common / both : 0.0f;
    return ratio > iou;
}

// whether a candidate that is still alive stays so against kept rows [k0, k1). Four independent IoUs are in flight per step: the block runs one wave per
// SIMD, so nothing else hides the latency of the LDS read and the division chain. A wave with no lane alive leaves early.
__device__ __forceinline__ bool survives(const float4* kept_box, int k0, int k1, float4 mine, float iou, bool alive) {
    int k = k0;
    for (; k + 4 <= k1 && __ballot(alive) != 0; k += 4) {
        const int hits = (int)suppresses(kept_box[k], mine, iou) + (int)suppresses(kept_box[k + 1], mine, iou) + (int)suppresses(kept_box[k + 2], mine, iou) +
                         (int)suppresses(kept_box[k + 3], mine, iou); // all four are evaluated: no short circuit
        alive = alive && hits == 0;
    }
    for (; k < k1 && __ballot(alive) != 0; ++k) alive = alive && !suppresses(kept_box[k], mine, iou);
    return alive;
}

__device__ __forceinline__ float lane_value(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// grid (B), 256 threads, dynamic LDS: max_det float4
__global__ __launch_bounds__(256) void yolo_nms_scan_kernel(const float* __restrict__ boxes, const int* __restrict__ cand_count, const float4* __restrict__ rbox,
                                                            const float2* __restrict__ rmeta, int A, int nc, float iou, int max_det, int max_nms, long M,
                                                            int* __restrict__ out, int* __restrict__ counts) {
    extern __shared__ float4 kept_box[];
    __shared__ int kept_after[4]; // the count behind wave w's turn; a slot is rewritten a round later, three barriers behind its last read
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = min(list_length(cand_count, b, A * nc), max_nms);
    rbox += b * M;
    rmeta += b * M;
    int kept = 0; // block-uniform: rows of the kept list as of the last barrier
    for (int base = 0; base < m && kept < max_det; base += 256) {
        const int i = base + tid;
        const float4 mine = i < m ? rbox[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        bool alive = i < m;
        const int round_start = kept;
        alive = survives(kept_box, 0, round_start, mine, iou, alive);
        for (int w = 0; w < 4 && kept < max_det; ++w) { // the waves in rank order; `kept` moves at the barrier below
            if (wave == w) {
                alive = survives(kept_box, round_start, kept, mine, iou, alive);
                // word of lane l: the later lanes of this wave that l would suppress. Rows of dead lanes are never asked for.
                const u64 alive_mask = __ballot(alive);
                u64 word = 0;
                for (u64 rows = alive_mask; rows != 0; rows &= rows - 1) {
                    const int l = __builtin_ctzll(rows);
                    const float4 row = make_float4(lane_value(mine.x, l), lane_value(mine.y, l), lane_value(mine.z, l), lane_value(mine.w, l));
                    const u64 hits = __ballot(alive && lane > l && suppresses(row, mine, iou));
                    if (lane == l) word = hits;
                }
                // the greedy pass over the wave, scalar: the first open lane is kept and closes what its word names
                const unsigned lo = (unsigned)word, hi = (unsigned)(word >> 32);
                u64 keep_mask = 0;
                int room = max_det - kept;
                for (u64 open = alive_mask; open != 0 && room > 0; --room) {
                    const int l = __builtin_ctzll(open);
                    const u64 closes = ((u64)(unsigned)__builtin_amdgcn_readlane((int)hi, l) << 32) | (unsigned)__builtin_amdgcn_readlane((int)lo, l);
                    keep_mask |= 1ull << l;
                    open &= ~(closes | (1ull << l));
                }
                if ((keep_mask >> lane) & 1) {
                    const int pos = kept + __popcll(keep_mask & ((1ull << lane) - 1)); // < max_det: keep_mask has at most `room` bits
                    kept_box[pos] = mine;
                    const float2 meta = rmeta[i];
                    const int idx = __float_as_int(meta.y);
                    const int anchor = min((int)((unsigned)idx / (unsigned)nc), A - 1), cls = (int)((unsigned)idx % (unsigned)nc);
                    const float4 raw = reinterpret_cast<const float4*>(boxes)[(long)b * A + anchor];
                    int* o = out + ((long)b * max_det + pos) * 7;
                    o[0] = __float_as_int(raw.x);
                    o[1] = __float_as_int(raw.y);
                    o[2] = __float_as_int(raw.z);
                    o[3] = __float_as_int(raw.w);
                    o[4] = __float_as_int(meta.x);
                    o[5] = cls;
                    o[6] = __float_as_int(meta.x);
                }
                if (lane == 0) kept_after[w] = kept + __popcll(keep_mask);
            }
            __syncthreads();
            kept = kept_after[w];
        }
    }
    if (tid == 0) counts[b] = kept;
}

} // namespace

extern "C" size_t vx_yolo_nms_workspace_bytes(int B, int A, int nc, int max_nms) {
    if (B < 1 || A < 1 || nc < 1 || max_nms < 1 || (long)A * nc > INT32_MAX) return 0;
    return nms_ws_layout(B, ranked_rows(A, nc, max_nms), nullptr, nullptr);
}

extern "C" int vx_yolo_nms(const float* boxes, const int* cand_count, const int* cand_idx, const float* cand_score, int B, int A, int nc, float iou, int max_det,
                           int max_nms, int max_wh, void* workspace, size_t workspace_bytes, void* out, int* counts, void* stream) {
    VX_REQUIRE(boxes && cand_count && cand_idx && cand_score && workspace && out && counts, "vx_yolo_nms: null operand");
    VX_REQUIRE(B >= 1 && B <= 65535 && A >= 1 && nc >= 1 && (long)A * nc <= INT32_MAX, "vx_yolo_nms: batch %d (1 .. 65535), %d anchors x %d classes", B, A, nc);
    VX_REQUIRE(max_det >= 1 && max_det <= NMS_MAX_DET, "vx_yolo_nms: max_det %d (1 .. %d, the kept list lives in LDS)", max_det, NMS_MAX_DET);
    VX_REQUIRE(max_nms >= 1, "vx_yolo_nms: max_nms %d below 1", max_nms);
    VX_REQUIRE(iou >= 0.0f && iou <= 1.0f, "vx_yolo_nms: iou %g outside [0, 1]", (double)iou);
    auto aligned4 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; };
    VX_REQUIRE(aligned16(boxes) && aligned4(cand_count) && aligned4(cand_idx) && aligned4(cand_score) && aligned4(out) && aligned4(counts),
               "vx_yolo_nms: misaligned operand (boxes 16 bytes, the others 4)");
    VX_REQUIRE(aligned16(workspace) && workspace_bytes >= vx_yolo_nms_workspace_bytes(B, A, nc, max_nms), "vx_yolo_nms: workspace of %zu bytes (16-byte aligned, at least %zu)",
               workspace_bytes, vx_yolo_nms_workspace_bytes(B, A, nc, max_nms));
    const long M = ranked_rows(A, nc, max_nms);
    nms_ws w;
    nms_ws_layout(B, M, &w, static_cast<uint8_t*>(workspace));
    const int lds = max_det * (int)sizeof(float4);
    VX_CHECK(vx_ensure_dynamic_lds(reinterpret_cast<const void*>(yolo_nms_scan_kernel), lds));
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(yolo_nms_rank_kernel, dim3(RANK_BLOCKS, B), dim3(256), 0, s, boxes, cand_count, cand_idx, cand_score, A, nc, max_nms, max_wh, M, w.rbox, w.rmeta);
    VX_LAUNCH_CHECK();
    hipLaunchKernelGGL(yolo_nms_scan_kernel, dim3(B), dim3(256), lds, s, boxes, cand_count, w.rbox, w.rmeta, A, nc, iou, max_det, max_nms, M, static_cast<int*>(out), counts);
    VX_LAUNCH_CHECK();
    return 1;
}
