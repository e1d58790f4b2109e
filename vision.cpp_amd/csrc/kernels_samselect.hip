// Kernels of MobileSAM's automatic mask generation (csrc/sam_generate.cpp sam_generate_masks_device): the selection stage between the logit planes of a
// batched decode and the masks a caller gets -- SAM's automatic mask generator on the device, so that a "segment everything" pass never waits for the host.
//   vx_sam_score_planes_f16        per candidate (prompt, plane): the counts behind the stability score and the box of the positive logits, over the
//                                  part of the plane the image occupies
//   vx_sam_rank_nms                the filters, the rank by predicted iou (by counting), the suppression bit matrix of the ranked survivors (one wave
//                                  ballot per 64 columns) and the greedy scan over it (one block, a 64-row tile at a time)
//   vx_sam_process_masks_indexed   the body of vx_sam_process_masks with the plane of output mask k named by keep_idx[k]
//   vx_sam_mask_stats_u8           area and box of the u8 masks that come out, and the info rows of the public entry
// Every decision is an integer comparison or a float32 comparison of a product (no division, no sum of products: nothing to contract), so a numpy
// restatement takes the same decisions bit for bit (tests/sam_select_ref.py). No scratch, no atomics; every value leaves through a vector store.
// Integer sums, minima and maxima do not depend on the order they are taken in: the same bytes on every run.
#include "vx_common.h"

#include <climits>

namespace {

constexpr int RANK_MAX = 16384; // candidates per vx_sam_rank_nms call: 256 words of 64 columns, the scan's `removed` set is 2 KiB of LDS

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// {sum, sum, min, max, min, max} of six per-thread values over a block of 256 threads: a butterfly in each wave, then wave 0 .. 3 in that order by thread 0.
// On return thread 0 holds the block's values in v[].
__device__ __forceinline__ void block_reduce6(int (&v)[6], int (*part)[6]) {
    v[0] = wave_sum_i(v[0]);
    v[1] = wave_sum_i(v[1]);
    v[2] = wave_min_i(v[2]);
    v[3] = wave_max_i(v[3]);
    v[4] = wave_min_i(v[4]);
    v[5] = wave_max_i(v[5]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int i = 0; i < 6; ++i) part[wave][i] = v[i];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) {
            v[0] += part[w][0];
            v[1] += part[w][1];
            v[2] = min(v[2], part[w][2]);
            v[3] = max(v[3], part[w][3]);
            v[4] = min(v[4], part[w][4]);
            v[5] = max(v[5], part[w][5]);
        }
}

struct score_acc {
    int inter = 0, uni = 0, x0 = INT_MAX, x1 = -1, y0 = INT_MAX, y1 = -1;
    __device__ __forceinline__ void take(float v, int x, int y, float off) {
        inter += v > off;
        uni += v > -off;
        if (v > 0.0f) {
            x0 = min(x0, x);
            x1 = max(x1, x);
            y0 = min(y0, y);
            y1 = max(y1, y);
        }
    }
};

// one block per candidate c = prompt * n_planes + plane. The region's rows are cut into units of 8 logits: a unit that lies inside the region is one
// 16-byte load (vec: every row of the plane starts 16-byte aligned), the last unit of a row whose width is no multiple of 8 is a scalar tail.
__global__ __launch_bounds__(256) void sam_score_planes_kernel(const f16* __restrict__ planes, long prompt_stride, long plane_stride, int mask_size, int n_planes,
                                                               int cw, int ch, float off, int vec, int* __restrict__ table, float* __restrict__ stability) {
    __shared__ int part[4][6];
    const int plane = blockIdx.x, prompt = blockIdx.y;
    const long c = (long)prompt * n_planes + plane;
    const f16* src = planes + prompt * prompt_stride + plane * plane_stride;
    const int per_row = (cw + 7) >> 3, units = per_row * ch;
    score_acc a;
    for (int u = threadIdx.x; u < units; u += 256) {
        const int y = u / per_row, x = (u - y * per_row) << 3;
        const f16* row = src + (long)y * mask_size + x;
        if (vec && x + 8 <= cw) {
            const f16x8 v = *reinterpret_cast<const f16x8*>(row);
#pragma unroll
            for (int i = 0; i < 8; ++i) a.take((float)v[i], x + i, y, off);
        } else {
            const int n = min(8, cw - x);
            for (int i = 0; i < n; ++i) a.take((float)row[i], x + i, y, off);
        }
    }
    int v[6] = {a.inter, a.uni, a.x0, a.x1, a.y0, a.y1};
    block_reduce6(v, part);
    if (threadIdx.x == 0) {
        const bool any = v[3] >= 0;
        int* t = table + c * 6;
        t[0] = v[0];
        t[1] = v[1];
        t[2] = any ? v[2] : 0;
        t[3] = any ? v[4] : 0;
        t[4] = any ? v[3] : 0;
        t[5] = any ? v[5] : 0;
        stability[c] = v[1] > 0 ? (float)v[0] / (float)v[1] : 0.0f;
    }
}

// ---- rank + NMS ---------------------------------------------------------------------------------------------------------------------------------------
// workspace of one call (vx_sam_rank_nms_workspace_bytes): key f32 [N] | order i32 [N] | boxes i32 [N][4] in rank order | survivors i32 | matrix u64 [N][words]
struct rank_ws {
    float* key;
    int* order;
    int4* rbox;
    int* n_surv;
    unsigned long long* matrix;
};
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t rank_ws_layout(long N, rank_ws* w, uint8_t* base) {
    const size_t o_key = 0, o_order = o_key + up256((size_t)N * 4), o_box = o_order + up256((size_t)N * 4), o_n = o_box + up256((size_t)N * 16);
    const size_t o_mat = o_n + 256, words = (size_t)(N + 63) / 64;
    if (w) *w = {reinterpret_cast<float*>(base + o_key), reinterpret_cast<int*>(base + o_order), reinterpret_cast<int4*>(base + o_box),
                 reinterpret_cast<int*>(base + o_n), reinterpret_cast<unsigned long long*>(base + o_mat)};
    return o_mat + (size_t)N * words * 8;
}

// the filters, one thread per candidate: flag, and key = the predicted iou of a survivor, NaN for the others (a NaN precedes nobody and counts nowhere)
__global__ __launch_bounds__(256) void sam_filter_kernel(const int* __restrict__ table, const float* __restrict__ iou, int n_planes, int iou_stride, int N, float iou_thresh,
                                                         float stab_thresh, int* __restrict__ flags, float* __restrict__ key) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    const float p = iou[(long)(c / n_planes) * iou_stride + c % n_planes];
    const int inter = table[(long)c * 6], uni = table[(long)c * 6 + 1];
    const bool pass = p > iou_thresh && uni > 0 && (float)inter >= stab_thresh * (float)uni;
    flags[c] = pass;
    key[c] = pass ? p : __builtin_nanf("");
}

// rank by counting: candidate c is preceded by every survivor with a larger key, and by those with an equal key and a smaller index. Every thread walks
// all N keys (the address is the same in all lanes). Survivors scatter their index and box to their rank; candidate 0's thread also counts the survivors.
__global__ __launch_bounds__(256) void sam_rank_kernel(const float* __restrict__ key, const int* __restrict__ table, int N, int* __restrict__ rank, int* __restrict__ order,
                                                       int4* __restrict__ rbox, int* __restrict__ n_surv) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    const float k = key[c];
    const bool pass = k == k;
    if (!pass) rank[c] = -1;
    if (!pass && c != 0) return;
    int before = 0, total = 0;
    for (int j = 0; j < N; ++j) {
        const float kj = key[j];
        total += kj == kj;
        before += (kj > k) | ((kj == k) & (j < c));
    }
    if (c == 0) *n_surv = total;
    if (pass) {
        rank[c] = before;
        order[before] = c;
        const int* t = table + (long)c * 6;
        rbox[before] = make_int4(t[2], t[3], t[4], t[5]);
    }
}

// torchvision's box IoU on inclusive integer coordinates, decided without a division
__device__ __forceinline__ bool sam_suppresses(int4 a, int4 b, float thresh) {
#pragma clang fp contract(off)
    const int area_a = (a.z - a.x) * (a.w - a.y), area_b = (b.z - b.x) * (b.w - b.y);
    const int iw = max(0, min(a.z, b.z) - max(a.x, b.x)), ih = max(0, min(a.w, b.w) - max(a.y, b.y));
    const int inter = iw * ih, uni = area_a + area_b - inter;
    return (float)inter > thresh * (float)uni;
}

// bit j of word w of row i = ranked survivor i suppresses ranked survivor j (j > i). Block (bx, by): rows 64 by .. 64 by + 63, words 4 bx .. 4 bx + 3, one word per
// wave; a lane keeps its column's box and the wave walks the rows, one ballot each. Words left of the diagonal are never read by the scan and are not written.
__global__ __launch_bounds__(256) void sam_nms_matrix_kernel(const int4* __restrict__ rbox, const int* __restrict__ n_surv, int words_per_row, float thresh,
                                                             unsigned long long* __restrict__ matrix) {
    const int M = *n_surv, lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6), tile = blockIdx.y;
    if (tile * 64 >= M || w * 64 >= M || w < tile) return; // wave-uniform
    const int j = w * 64 + lane;
    const int4 bj = j < M ? rbox[j] : make_int4(0, 0, 0, 0);
    const int rows = min(64, M - tile * 64);
    for (int r = 0; r < rows; ++r) {
        const int i = tile * 64 + r;
        const int4 bi = rbox[i];
        const unsigned long long word = __ballot(j < M && j > i && sam_suppresses(bi, bj, thresh));
        if (lane == 0) matrix[(long)i * words_per_row + w] = word;
    }
}

// The greedy scan, one block of 256 threads. `removed` (one bit per ranked survivor) lives in LDS. Per 64-row tile: wave 0 loads the tile's 64 diagonal words,
// one per lane, and resolves the tile in registers (64 steps of readlane, no memory in the chain); its kept rows get their output slots; then every thread
// ORs the kept rows' words of the columns it owns into `removed` (independent loads, coalesced along a row).
__global__ __launch_bounds__(256) void sam_nms_scan_kernel(const unsigned long long* __restrict__ matrix, const int* __restrict__ order, const int* __restrict__ n_surv,
                                                           int words_per_row, int capacity, int* __restrict__ keep_idx, int* __restrict__ counts) {
    __shared__ unsigned long long removed[RANK_MAX / 64];
    __shared__ unsigned long long kept_mask;
    const int M = *n_surv, W = (M + 63) / 64, tid = threadIdx.x;
    for (int w = tid; w < W; w += 256) removed[w] = 0;
    __syncthreads();
    int kept = 0;
    for (int t = 0; t < W; ++t) {
        if (tid < 64) {
            const int row = t * 64 + tid;
            const unsigned long long diag = row < M ? matrix[(long)row * words_per_row + t] : 0ull;
            const unsigned lo = (unsigned)diag, hi = (unsigned)(diag >> 32);
            unsigned long long rem = removed[t];
#pragma unroll
            for (int l = 0; l < 64; ++l) {
                const unsigned long long d = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)hi, l) << 32) | (unsigned)__builtin_amdgcn_readlane((int)lo, l);
                if (!((rem >> l) & 1)) rem |= d;
            }
            const int rows = min(64, M - t * 64);
            const unsigned long long valid = rows == 64 ? ~0ull : ((1ull << rows) - 1);
            const unsigned long long km = ~rem & valid;
            if ((km >> tid) & 1) {
                const int pos = kept + __popcll(km & ((1ull << tid) - 1));
                if (pos < capacity) keep_idx[pos] = order[row];
            }
            if (tid == 0) kept_mask = km;
        }
        __syncthreads();
        const unsigned long long km = kept_mask;
        kept += __popcll(km);
        for (int w = t + 1 + tid; w < W; w += 256) {
            unsigned long long acc = 0;
            for (int l = 0; l < 64; ++l)
                if ((km >> l) & 1) acc |= matrix[(long)(t * 64 + l) * words_per_row + w];
            removed[w] |= acc;
        }
        __syncthreads();
    }
    if (tid == 0) {
        counts[0] = min(kept, capacity);
        counts[1] = kept;
    }
}

// ---- the masks that come out ------------------------------------------------------------------------------------------------------------------------------
// sam_interp_one of kernels_samprompts.hip, restated: the same expressions in the same order with contraction off, so the same bytes.
template <typename TS>
__device__ __forceinline__ void sam_interp_one(const TS* __restrict__ src, int sw, int sh, int sstride, int step, void* __restrict__ dst, int dw, int dh, int out_u8) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dw * dh) return;
    const int x = i % dw, y = i / dw;
    const float scale_x = (float)sw / (float)dw, scale_y = (float)sh / (float)dh;
    const float sxf = fmaxf(((float)x + 0.5f) * scale_x - 0.5f, 0.0f), syf = fmaxf(((float)y + 0.5f) * scale_y - 0.5f, 0.0f);
    const int x0 = (int)sxf, y0 = (int)syf;
    const int x1 = min(x0 + 1, sw - 1), y1 = min(y0 + 1, sh - 1);
    const float v00 = (float)src[((long)y0 * sstride + x0) * step], v01 = (float)src[((long)y0 * sstride + x1) * step];
    const float v10 = (float)src[((long)y1 * sstride + x0) * step], v11 = (float)src[((long)y1 * sstride + x1) * step];
    const float wx = sxf - (float)x0, wy = syf - (float)y0;
    const float v0 = (1 - wx) * v00 + wx * v01, v1 = (1 - wx) * v10 + wx * v11;
    const float v = (1 - wy) * v0 + wy * v1;
    if (out_u8) reinterpret_cast<uint8_t*>(dst)[i] = v > 0.0f ? 255 : 0;
    else reinterpret_cast<float*>(dst)[i] = v;
}

// output mask k = k0 + blockIdx.y reads candidate keep_idx[k] = prompt * n_scored + plane; masks at and behind counts[0] are neither read nor written
__global__ __launch_bounds__(256) void sam_indexed_upscale_kernel(const f16* __restrict__ planes, long prompt_stride, long plane_stride, int step, int mask_size,
                                                                  int n_scored, int n_prompts, const int* __restrict__ keep_idx, const int* __restrict__ counts, int k0,
                                                                  float* __restrict__ scaled, int image_size) {
    const int k = k0 + blockIdx.y;
    if (k >= counts[0]) return;
    const int c = min(max(keep_idx[k], 0), n_prompts * n_scored - 1); // an index outside the candidates reads the nearest one, never beyond the buffer
    sam_interp_one<f16>(planes + (long)(c / n_scored) * prompt_stride + (c % n_scored) * plane_stride, mask_size, mask_size, mask_size, step,
                        scaled + (long)blockIdx.y * image_size * image_size, image_size, image_size, 0);
}

__global__ __launch_bounds__(256) void sam_indexed_crop_kernel(const float* __restrict__ scaled, int image_size, int sw, int sh, const int* __restrict__ counts, int k0,
                                                               uint8_t* __restrict__ out, int dw, int dh) {
    const int k = k0 + blockIdx.y;
    if (k >= counts[0]) return;
    sam_interp_one<float>(scaled + (long)blockIdx.y * image_size * image_size, sw, sh, image_size, 1, out + (long)k * dw * dh, dw, dh, 1);
}

// one block per mask: area = pixels that are 255, box of them. 16 bytes per load from the first 16-byte aligned pixel on, single bytes before and behind.
__global__ __launch_bounds__(256) void sam_mask_stats_kernel(const uint8_t* __restrict__ masks, int w, int h, const int* __restrict__ keep_idx, const int* __restrict__ counts,
                                                             int n_scored, int n_prompts, const float* __restrict__ iou, int iou_stride, const float* __restrict__ stability,
                                                             int* __restrict__ info_i32, float* __restrict__ info_f32) {
    __shared__ int part[4][6];
    const int k = blockIdx.x;
    if (k >= counts[0]) return;
    const long n = (long)w * h;
    const uint8_t* m = masks + k * n;
    int area = 0, x0 = INT_MAX, x1 = -1, y0 = INT_MAX, y1 = -1;
    auto take = [&](long i) {
        const int y = (int)(i / w), x = (int)(i - (long)y * w);
        ++area;
        x0 = min(x0, x);
        x1 = max(x1, x);
        y0 = min(y0, y);
        y1 = max(y1, y);
    };
    const long head = min(n, (long)((16 - (reinterpret_cast<uintptr_t>(m) & 15)) & 15)), n16 = (n - head) / 16, tail = head + n16 * 16;
    for (long i = threadIdx.x; i < head; i += 256)
        if (m[i] == 255) take(i);
    const uint4* mv = reinterpret_cast<const uint4*>(m + head);
    for (long q = threadIdx.x; q < n16; q += 256) {
        const uint4 v = mv[q];
        if ((v.x | v.y | v.z | v.w) == 0) continue;
        const unsigned word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int b = 0; b < 16; ++b)
            if (((word[b >> 2] >> ((b & 3) * 8)) & 255u) == 255u) take(head + q * 16 + b);
    }
    for (long i = tail + threadIdx.x; i < n; i += 256)
        if (m[i] == 255) take(i);
    int v[6] = {area, 0, x0, x1, y0, y1};
    block_reduce6(v, part);
    if (threadIdx.x == 0) {
        const bool any = v[0] > 0;
        const int c = min(max(keep_idx[k], 0), n_prompts * n_scored - 1); // as the indexed mask pass reads it: never beyond the tables
        int* r = info_i32 + (long)k * 8;
        r[0] = c / n_scored;
        r[1] = c % n_scored;
        r[2] = any ? v[2] : 0;
        r[3] = any ? v[4] : 0;
        r[4] = any ? v[3] - v[2] + 1 : 0;
        r[5] = any ? v[5] - v[4] + 1 : 0;
        r[6] = v[0];
        r[7] = 0;
        if (info_f32) {
            info_f32[(long)k * 2] = iou[(long)(c / n_scored) * iou_stride + c % n_scored];
            info_f32[(long)k * 2 + 1] = stability[c];
        }
    }
}

} // namespace

extern "C" int vx_sam_score_planes_f16(const void* planes, int64_t prompt_stride, int64_t plane_stride, int mask_size, int n_planes, int cw, int ch, float offset,
                                       int32_t* table, float* stability, int P, void* stream) {
    VX_REQUIRE(planes && table && stability && P > 0 && P <= 65535, "vx_sam_score_planes_f16: bad operands (1 .. 65535 prompts)");
    VX_REQUIRE(mask_size > 0 && mask_size <= 32768 && n_planes > 0 && n_planes <= 65535, "vx_sam_score_planes_f16: bad plane layout");
    VX_REQUIRE(plane_stride >= (int64_t)mask_size * mask_size && prompt_stride >= plane_stride * n_planes,
               "vx_sam_score_planes_f16: strides %lld / %lld below %d planes of %d^2", (long long)prompt_stride, (long long)plane_stride, n_planes, mask_size);
    VX_REQUIRE(cw > 0 && ch > 0 && cw <= mask_size && ch <= mask_size, "vx_sam_score_planes_f16: region %d x %d of a %d^2 plane", cw, ch, mask_size);
    VX_REQUIRE(offset >= 0.0f, "vx_sam_score_planes_f16: the stability offset must be 0 or above"); // a NaN fails too
    const int vec = aligned16(planes) && mask_size % 8 == 0 && plane_stride % 8 == 0 && prompt_stride % 8 == 0;
    hipLaunchKernelGGL(sam_score_planes_kernel, dim3((unsigned)n_planes, (unsigned)P), dim3(256), 0, as_stream(stream), reinterpret_cast<const f16*>(planes),
                       (long)prompt_stride, (long)plane_stride, mask_size, n_planes, cw, ch, offset, vec, table, stability);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" size_t vx_sam_rank_nms_workspace_bytes(int N) { return N < 1 || N > RANK_MAX ? 0 : rank_ws_layout(N, nullptr, nullptr); }

extern "C" int vx_sam_rank_nms(const int32_t* table, const float* iou, int n_planes, int iou_stride, int N, float pred_iou_thresh, float stability_thresh,
                               float nms_iou_thresh, int capacity, void* workspace, size_t workspace_bytes, int32_t* flags, int32_t* rank, int32_t* keep_idx,
                               int32_t* counts, void* stream) {
    VX_REQUIRE(table && iou && workspace && flags && rank && keep_idx && counts, "vx_sam_rank_nms: null operand");
    VX_REQUIRE(N >= 1 && N <= RANK_MAX, "vx_sam_rank_nms: %d candidates (1 .. %d)", N, RANK_MAX);
    VX_REQUIRE(n_planes >= 1 && iou_stride >= n_planes && N % n_planes == 0, "vx_sam_rank_nms: %d candidates in groups of %d with iou stride %d", N, n_planes, iou_stride);
    VX_REQUIRE(pred_iou_thresh == pred_iou_thresh && stability_thresh == stability_thresh && nms_iou_thresh == nms_iou_thresh, "vx_sam_rank_nms: a threshold is NaN");
    VX_REQUIRE(nms_iou_thresh >= 0.0f && nms_iou_thresh <= 1.0f, "vx_sam_rank_nms: nms_iou_thresh %g outside [0, 1]", (double)nms_iou_thresh);
    VX_REQUIRE(capacity >= 1, "vx_sam_rank_nms: capacity %d below 1", capacity);
    VX_REQUIRE(aligned16(workspace) && workspace_bytes >= vx_sam_rank_nms_workspace_bytes(N), "vx_sam_rank_nms: workspace of %zu bytes (16-byte aligned, at least %zu)",
               workspace_bytes, vx_sam_rank_nms_workspace_bytes(N));
    rank_ws w;
    rank_ws_layout(N, &w, static_cast<uint8_t*>(workspace));
    const int words = (N + 63) / 64;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(sam_filter_kernel, dim3(blocks_for(N)), dim3(256), 0, s, table, iou, n_planes, iou_stride, N, pred_iou_thresh, stability_thresh, flags, w.key);
    VX_LAUNCH_CHECK();
    hipLaunchKernelGGL(sam_rank_kernel, dim3(blocks_for(N)), dim3(256), 0, s, w.key, table, N, rank, w.order, w.rbox, w.n_surv);
    VX_LAUNCH_CHECK();
    hipLaunchKernelGGL(sam_nms_matrix_kernel, dim3((unsigned)((words + 3) / 4), (unsigned)words), dim3(256), 0, s, w.rbox, w.n_surv, words, nms_iou_thresh, w.matrix);
    VX_LAUNCH_CHECK();
    hipLaunchKernelGGL(sam_nms_scan_kernel, dim3(1), dim3(256), 0, s, w.matrix, w.order, w.n_surv, words, capacity, keep_idx, counts);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_sam_process_masks_indexed(const void* planes, int64_t prompt_stride, int64_t plane_stride, int step, int mask_size, int n_scored, int n_prompts,
                                            const int32_t* keep_idx, const int32_t* counts, int capacity, int group, float* scaled, int image_size, int sw, int sh,
                                            uint8_t* out, int dw, int dh, void* stream) {
    VX_REQUIRE(planes && keep_idx && counts && scaled && out, "vx_sam_process_masks_indexed: null operand");
    VX_REQUIRE(capacity > 0 && group > 0 && group <= 65535, "vx_sam_process_masks_indexed: capacity %d in groups of %d (1 .. 65535)", capacity, group);
    VX_REQUIRE(mask_size > 0 && n_scored > 0 && n_prompts > 0 && (int64_t)n_scored * n_prompts <= RANK_MAX && step > 0 && plane_stride > 0 && prompt_stride > 0 && image_size > 0,
               "vx_sam_process_masks_indexed: bad plane layout");
    VX_REQUIRE(sw > 0 && sh > 0 && sw <= image_size && sh <= image_size && dw > 0 && dh > 0, "vx_sam_process_masks_indexed: crop %d x %d of a %d^2 map, target %d x %d", sw,
               sh, image_size, dw, dh);
    VX_REQUIRE((long)image_size * image_size <= (1L << 31) - 256 && (long)dw * dh <= (1L << 31) - 256, "vx_sam_process_masks_indexed: map too large");
    for (int k0 = 0; k0 < capacity; k0 += group) { // `scaled` holds `group` maps: the masks go through it a group at a time
        const unsigned g = (unsigned)(capacity - k0 < group ? capacity - k0 : group);
        hipLaunchKernelGGL(sam_indexed_upscale_kernel, dim3(blocks_for((long)image_size * image_size), g), dim3(256), 0, as_stream(stream),
                           reinterpret_cast<const f16*>(planes), (long)prompt_stride, (long)plane_stride, step, mask_size, n_scored, n_prompts, keep_idx, counts, k0, scaled,
                           image_size);
        VX_LAUNCH_CHECK();
        hipLaunchKernelGGL(sam_indexed_crop_kernel, dim3(blocks_for((long)dw * dh), g), dim3(256), 0, as_stream(stream), scaled, image_size, sw, sh, counts, k0, out, dw, dh);
        VX_LAUNCH_CHECK();
    }
    return 1;
}

extern "C" int vx_sam_mask_stats_u8(const uint8_t* masks, int w, int h, const int32_t* keep_idx, const int32_t* counts, int capacity, int n_scored, int n_prompts,
                                    const float* iou, int iou_stride, const float* stability, int32_t* info_i32, float* info_f32, void* stream) {
    VX_REQUIRE(masks && keep_idx && counts && info_i32, "vx_sam_mask_stats_u8: null operand");
    VX_REQUIRE(!info_f32 || (iou && stability), "vx_sam_mask_stats_u8: the f32 rows need the iou predictions and the stability scores");
    VX_REQUIRE(w > 0 && h > 0 && (long)w * h <= (1L << 31) - 256, "vx_sam_mask_stats_u8: extent %d x %d", w, h);
    VX_REQUIRE(capacity > 0 && n_scored > 0 && n_prompts > 0 && (int64_t)n_scored * n_prompts <= RANK_MAX && iou_stride >= (info_f32 ? n_scored : 0),
               "vx_sam_mask_stats_u8: capacity %d, %d prompts of %d planes with iou stride %d", capacity, n_prompts, n_scored, iou_stride);
    hipLaunchKernelGGL(sam_mask_stats_kernel, dim3((unsigned)capacity), dim3(256), 0, as_stream(stream), masks, w, h, keep_idx, counts, n_scored, n_prompts, iou, iou_stride,
                       stability, info_i32, info_f32);
    VX_LAUNCH_CHECK();
    return 1;
}
