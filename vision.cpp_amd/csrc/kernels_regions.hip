// Connected-component labelling of u8 masks on the device, and SAM's remove_small_regions on top of it: small holes (background components) are filled,
// small islands (foreground components) are removed, 8-connectivity, a component is small iff it has fewer than min_area pixels.
//   vx_mask_regions_workspace_bytes      bytes of workspace for `group` masks of w x h in flight
//   vx_mask_remove_small_regions_u8      the batched pass: per group of masks and per step (holes, then islands) five or six launches
//     tile     a 32 x 32 tile is labelled in LDS by union-find (a label = the smallest row-major pixel index of its component in the tile); labels[p] = the
//              tile root of pixel p as a pixel index of the mask (-1 outside the set being labelled), areas[p] = the tile component's pixel count at a tile
//              root, 0 elsewhere
//     merge    ONE block per mask unites the labels across every tile border, so no block reads a word that another block of the launch writes: the block's own
//              reads of the labels are agent-scope loads (served by L2, where its atomicMin lands), and a stale parent would still be an ancestor
//     areas    every tile root that is no final root adds its count to its final root's (integer atomicAdd)
//     best     (islands only) per mask the maximum over the final roots of (area, then smallest root), one 64-bit atomicMax each
//     decide   every pixel of a small component is flipped (a plain byte store of 0 or 255, nothing else is written) and `changed` is raised (atomicMax)
//   vx_sam_clean_nms_inputs              the records of cleaned masks as the table and keys that vx_sam_rank_nms takes: SAM's second NMS, scores 1 / 0
//   vx_sam_gather_clean_masks            the survivors of that NMS, masks and records, from the staging buffer to the caller's in final order
// Parents only ever decrease (a root is linked to a smaller root by atomicMin), so every find and every union loop ends by construction; nothing waits for
// another thread. Integer min / add / max atomics only: their final values do not depend on the order of arrival, the same bytes on every run. The launches
// behind the merge only read the labels; the areas a launch adds to are read by later launches only.
#include "vx_common.h"

namespace {

constexpr int T = 32, TP = T * T; // tile edge; pixels of a tile, four per thread of a block of 256

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// the root of x: parents decrease, so the walk ends at the latest at the set's smallest index
__device__ __forceinline__ int find_lds(const int* lab, int x) {
    for (int q; (q = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != x;) x = q;
    return x;
}
__device__ __forceinline__ int find_l2(const int* lab, int x) { // past this CU's L1, to where the atomics of the same block land
    for (int q; (q = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x;) x = q;
    return x;
}
__device__ __forceinline__ int find_plain(const int* __restrict__ lab, int x) { // labels written by earlier launches only
    for (int q; (q = lab[x]) != x;) x = q;
    return x;
}

// Unite the sets of a and b: the larger root is linked to the smaller one by atomicMin. Where the larger one had a parent already (old != a) the loop goes on with
// that parent, so no link is lost; max(a, b) decreases with every round.
template <bool LDS>
__device__ __forceinline__ void unite(int* lab, int a, int b) {
    for (;;) {
        a = LDS ? find_lds(lab, a) : find_l2(lab, a);
        b = LDS ? find_lds(lab, b) : find_l2(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(lab + a, b);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ bool skipped(const int* __restrict__ counts, int m) { return counts && m >= counts[0]; }

__global__ __launch_bounds__(256) void regions_init_kernel(const int* __restrict__ counts, int n, int* __restrict__ changed) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m < n && !skipped(counts, m)) changed[m] = 0;
}

// block (tile, mask of the group). `fg` = 1 labels the non-zero pixels, 0 the zero ones.
__global__ __launch_bounds__(256) void regions_tile_kernel(const uint8_t* __restrict__ masks, int w, int h, int tiles_x, const int* __restrict__ counts, int k0, int fg,
                                                           int* __restrict__ labels, int* __restrict__ areas, unsigned long long* __restrict__ best) {
    __shared__ int lab[TP];
    __shared__ int cnt[TP];
    const int j = blockIdx.y, m = k0 + j, tid = threadIdx.x;
    if (skipped(counts, m)) return;
    const long px = (long)w * h;
    const uint8_t* src = masks + m * px;
    const int x0 = (blockIdx.x % tiles_x) * T, y0 = (blockIdx.x / tiles_x) * T;
    if (blockIdx.x == 0 && tid == 0) best[j] = 0;
    bool member[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = tid + 256 * k, x = x0 + (i & (T - 1)), y = y0 + (i >> 5);
        member[k] = x < w && y < h && (src[(long)y * w + x] != 0) == (fg != 0);
        lab[i] = member[k] ? i : -1;
        cnt[i] = 0;
    }
    __syncthreads();
    // west, and north; north-west and north-east only without a north neighbour, which would join both (they are its west and its east's west)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = tid + 256 * k, lx = i & (T - 1), ly = i >> 5;
        if (!member[k]) continue;
        if (lx > 0 && lab[i - 1] >= 0) unite<true>(lab, i, i - 1);
        if (ly > 0) {
            if (lab[i - T] >= 0) unite<true>(lab, i, i - T);
            else {
                if (lx > 0 && lab[i - T - 1] >= 0) unite<true>(lab, i, i - T - 1);
                if (lx < T - 1 && lab[i - T + 1] >= 0) unite<true>(lab, i, i - T + 1);
            }
        }
    }
    __syncthreads();
    int root[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        root[k] = member[k] ? find_lds(lab, tid + 256 * k) : -1;
        if (member[k]) atomicAdd(cnt + root[k], 1);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = tid + 256 * k, x = x0 + (i & (T - 1)), y = y0 + (i >> 5);
        if (x >= w || y >= h) continue;
        const long p = (long)y * w + x;
        labels[j * px + p] = member[k] ? (y0 + (root[k] >> 5)) * w + x0 + (root[k] & (T - 1)) : -1;
        areas[j * px + p] = member[k] && root[k] == i ? cnt[i] : 0;
    }
}

// one block per mask: every pair of neighbours that a tile border separates. Item it < nh: the pixel (x, y) of the first row of a tile row with its three
// neighbours above; the others: the pixel of the first column of a tile column with its three neighbours to the left. The diagonal pair across a tile corner is
// in both lists. As in the tile: the diagonal neighbours only where the straight one is missing.
__global__ __launch_bounds__(1024) void regions_merge_kernel(int w, int h, int tiles_x, int tiles_y, const int* __restrict__ counts, int k0, int* __restrict__ labels) {
    const int j = blockIdx.x, m = k0 + j;
    if (skipped(counts, m)) return;
    int* lab = labels + (long)j * w * h;
    auto in = [&](int p) { return __hip_atomic_load(lab + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0; };
    const long nh = (long)(tiles_y - 1) * w, nv = (long)(tiles_x - 1) * h;
    for (long it = threadIdx.x; it < nh + nv; it += 1024) {
        if (it < nh) {
            const int y = (int)(it / w + 1) * T, x = (int)(it % w), p = y * w + x, q = p - w;
            if (!in(p)) continue;
            if (in(q)) unite<false>(lab, p, q);
            else {
                if (x > 0 && in(q - 1)) unite<false>(lab, p, q - 1);
                if (x < w - 1 && in(q + 1)) unite<false>(lab, p, q + 1);
            }
        } else {
            const long iv = it - nh;
            const int x = (int)(iv / h + 1) * T, y = (int)(iv % h), p = y * w + x, q = p - 1;
            if (!in(p)) continue;
            if (in(q)) unite<false>(lab, p, q);
            else {
                if (y > 0 && in(q - w)) unite<false>(lab, p, q - w);
                if (y < h - 1 && in(q + w)) unite<false>(lab, p, q + w);
            }
        }
    }
}

// a tile root whose parent is another pixel is no final root: nobody adds to its count, which moves to its final root
__global__ __launch_bounds__(256) void regions_areas_kernel(long px, const int* __restrict__ counts, int k0, const int* __restrict__ labels, int* __restrict__ areas) {
    const int j = blockIdx.y;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (skipped(counts, k0 + j) || p >= px) return;
    const int* lab = labels + j * px;
    const int v = lab[p];
    if (v < 0 || v == p) return;
    const int a = areas[j * px + p];
    if (a == 0) return;
    atomicAdd(areas + j * px + find_plain(lab, v), a);
}

// best[j] = max over the final roots of area << 32 | (INT_MAX - root): the largest component, of equal ones the one whose first pixel comes first
__global__ __launch_bounds__(256) void regions_best_kernel(long px, const int* __restrict__ counts, int k0, const int* __restrict__ labels, const int* __restrict__ areas,
                                                           unsigned long long* __restrict__ best) {
    const int j = blockIdx.y;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (skipped(counts, k0 + j) || p >= px) return;
    if (labels[j * px + p] != (int)p) return;
    atomicMax(best + j, ((unsigned long long)(unsigned)areas[j * px + p] << 32) | (unsigned)(0x7fffffff - (int)p));
}

__global__ __launch_bounds__(256) void regions_decide_kernel(uint8_t* __restrict__ masks, long px, const int* __restrict__ counts, int k0, int fg, int min_area,
                                                             const int* __restrict__ labels, const int* __restrict__ areas, const unsigned long long* __restrict__ best,
                                                             int* __restrict__ changed) {
    const int j = blockIdx.y, m = k0 + j;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (skipped(counts, m)) return;
    bool flip = false;
    if (p < px) {
        const int* lab = labels + j * px;
        const int v = lab[p];
        if (v >= 0) {
            const int r = find_plain(lab, v);
            flip = areas[j * px + r] < min_area;
            if (flip && fg) { // where every island is small the largest one stays
                const unsigned long long b = best[j];
                flip = !((int)(b >> 32) < min_area && r == 0x7fffffff - (int)(unsigned)b);
            }
            if (flip) masks[m * px + p] = fg ? 0 : 255;
        }
    }
    if (changed && __ballot(flip) != 0 && (threadIdx.x & 63) == 0) atomicMax(changed + m, 1);
}

// ---- the second NMS of SAM's postprocess_small_regions, fed to vx_sam_rank_nms, and the gather of its survivors ---------------------------------------------------
// row k of the records of the cleaned masks -> a table row whose counts pass every stability threshold with the mask's inclusive box, and the key: 1 for an
// unchanged mask, 0 for a changed one, NaN (which the filter refuses) at and behind the count
__global__ __launch_bounds__(256) void clean_nms_inputs_kernel(const int* __restrict__ info, const int* __restrict__ changed, const int* __restrict__ counts, int N,
                                                               int* __restrict__ table, float* __restrict__ key) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= N) return;
    const bool live = k < counts[0];
    const int* r = info + (long)k * 8;
    const bool any = live && r[6] > 0;
    int* t = table + (long)k * 6;
    t[0] = t[1] = 1;
    t[2] = any ? r[2] : 0;
    t[3] = any ? r[3] : 0;
    t[4] = any ? r[2] + r[4] - 1 : 0;
    t[5] = any ? r[3] + r[5] - 1 : 0;
    key[k] = live ? (changed[k] ? 0.0f : 1.0f) : __builtin_nanf("");
}

// block (part, output mask i): mask keep[i] of the staged ones to place i, its records with the changed flag in column 7; block (0, 0) writes the counts
__global__ __launch_bounds__(256) void clean_gather_kernel(const uint8_t* __restrict__ masks, long px, int vec, const int* __restrict__ info, const float* __restrict__ info_f,
                                                           const int* __restrict__ changed, const int* __restrict__ keep, const int* __restrict__ first,
                                                           const int* __restrict__ second, int N, uint8_t* __restrict__ out, int* __restrict__ out_info,
                                                           float* __restrict__ out_info_f, int* __restrict__ out_counts) {
    const int i = blockIdx.y, n_out = min(second[0], N), tid = threadIdx.x;
    if (blockIdx.x == 0 && i == 0 && tid == 0) {
        int n_changed = 0;
        for (int q = 0; q < n_out; ++q) n_changed += changed[min(max(keep[q], 0), N - 1)] != 0;
        out_counts[0] = n_out;
        out_counts[1] = first[1];
        out_counts[2] = n_changed;
        out_counts[3] = min(first[0], N) - second[1];
    }
    if (i >= n_out) return;
    const int src = min(max(keep[i], 0), N - 1); // never beyond the staged masks
    if (blockIdx.x == 0 && tid < 8) out_info[(long)i * 8 + tid] = tid == 7 ? (changed[src] != 0) : info[(long)src * 8 + tid];
    if (blockIdx.x == 0 && tid >= 8 && tid < 10) out_info_f[(long)i * 2 + tid - 8] = info_f[(long)src * 2 + tid - 8];
    const uint8_t* s = masks + src * px;
    uint8_t* d = out + i * px;
    if (vec) {
        const long q = (long)blockIdx.x * 256 + tid;
        if (q < px / 16) reinterpret_cast<uint4*>(d)[q] = reinterpret_cast<const uint4*>(s)[q];
    } else {
        const long b0 = ((long)blockIdx.x * 256 + tid) * 16, b1 = min(b0 + 16, px);
        for (long b = b0; b < b1; ++b) d[b] = s[b];
    }
}

} // namespace

extern "C" size_t vx_mask_regions_workspace_bytes(int w, int h, int group) {
    if (w < 1 || h < 1 || group < 1 || group > 65535 || (long)w * h > (1L << 31) - 256) return 0;
    return 2 * up256((size_t)group * w * h * 4) + up256((size_t)group * 8);
}

extern "C" int vx_mask_remove_small_regions_u8(uint8_t* masks, int w, int h, int n, const int32_t* counts, int min_area, int mode, int32_t* changed, void* workspace,
                                               size_t workspace_bytes, int group, void* stream) {
    VX_REQUIRE(masks && workspace, "vx_mask_remove_small_regions_u8: null operand");
    VX_REQUIRE(w > 0 && h > 0 && (long)w * h <= (1L << 31) - 256, "vx_mask_remove_small_regions_u8: extent %d x %d", w, h);
    VX_REQUIRE(n > 0 && group > 0 && group <= 65535, "vx_mask_remove_small_regions_u8: %d masks in groups of %d (1 .. 65535)", n, group);
    VX_REQUIRE(min_area >= 0, "vx_mask_remove_small_regions_u8: min_area %d below 0", min_area);
    VX_REQUIRE(mode >= VX_REGIONS_HOLES && mode <= VX_REGIONS_BOTH, "vx_mask_remove_small_regions_u8: unknown mode %d (1 holes, 2 islands, 3 both)", mode);
    VX_REQUIRE(aligned16(workspace) && workspace_bytes >= vx_mask_regions_workspace_bytes(w, h, group),
               "vx_mask_remove_small_regions_u8: workspace of %zu bytes (16-byte aligned, at least %zu)", workspace_bytes, vx_mask_regions_workspace_bytes(w, h, group));
    hipStream_t s = as_stream(stream);
    if (changed) {
        hipLaunchKernelGGL(regions_init_kernel, dim3(blocks_for(n)), dim3(256), 0, s, counts, n, changed);
        VX_LAUNCH_CHECK();
    }
    if (min_area <= 1) return 1; // no component has fewer than one pixel: nothing can change, no mask byte is read or written
    const long px = (long)w * h;
    const size_t plane = up256((size_t)group * px * 4);
    int* labels = static_cast<int*>(workspace);
    int* areas = reinterpret_cast<int*>(static_cast<uint8_t*>(workspace) + plane);
    unsigned long long* best = reinterpret_cast<unsigned long long*>(static_cast<uint8_t*>(workspace) + 2 * plane);
    const int tiles_x = (w + T - 1) / T, tiles_y = (h + T - 1) / T;
    for (int k0 = 0; k0 < n; k0 += group) {
        const unsigned g = (unsigned)(n - k0 < group ? n - k0 : group);
        for (int fg = 0; fg < 2; ++fg) { // SAM's order: the holes, then the islands of what that left
            if (!(mode & (fg ? VX_REGIONS_ISLANDS : VX_REGIONS_HOLES))) continue;
            hipLaunchKernelGGL(regions_tile_kernel, dim3((unsigned)(tiles_x * tiles_y), g), dim3(256), 0, s, masks, w, h, tiles_x, counts, k0, fg, labels, areas, best);
            VX_LAUNCH_CHECK();
            if (tiles_x * tiles_y > 1) {
                hipLaunchKernelGGL(regions_merge_kernel, dim3(g), dim3(1024), 0, s, w, h, tiles_x, tiles_y, counts, k0, labels);
                VX_LAUNCH_CHECK();
                hipLaunchKernelGGL(regions_areas_kernel, dim3(blocks_for(px), g), dim3(256), 0, s, px, counts, k0, labels, areas);
                VX_LAUNCH_CHECK();
            }
            if (fg) {
                hipLaunchKernelGGL(regions_best_kernel, dim3(blocks_for(px), g), dim3(256), 0, s, px, counts, k0, labels, areas, best);
                VX_LAUNCH_CHECK();
            }
            hipLaunchKernelGGL(regions_decide_kernel, dim3(blocks_for(px), g), dim3(256), 0, s, masks, px, counts, k0, fg, min_area, labels, areas, best, changed);
            VX_LAUNCH_CHECK();
        }
    }
    return 1;
}

extern "C" int vx_sam_clean_nms_inputs(const int32_t* info_i32, const int32_t* changed, const int32_t* counts, int N, int32_t* table, float* key, void* stream) {
    VX_REQUIRE(info_i32 && changed && counts && table && key, "vx_sam_clean_nms_inputs: null operand");
    VX_REQUIRE(N >= 1, "vx_sam_clean_nms_inputs: %d rows", N);
    hipLaunchKernelGGL(clean_nms_inputs_kernel, dim3(blocks_for(N)), dim3(256), 0, as_stream(stream), info_i32, changed, counts, N, table, key);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_sam_gather_clean_masks(const uint8_t* masks, int w, int h, const int32_t* info_i32, const float* info_f32, const int32_t* changed, const int32_t* keep_idx,
                                         const int32_t* first_counts, const int32_t* second_counts, int N, uint8_t* out_masks, int32_t* out_info_i32, float* out_info_f32,
                                         int32_t* out_counts, void* stream) {
    VX_REQUIRE(masks && info_i32 && info_f32 && changed && keep_idx && first_counts && second_counts && out_masks && out_info_i32 && out_info_f32 && out_counts,
               "vx_sam_gather_clean_masks: null operand");
    VX_REQUIRE(w > 0 && h > 0 && (long)w * h <= (1L << 31) - 256, "vx_sam_gather_clean_masks: extent %d x %d", w, h);
    VX_REQUIRE(N >= 1 && N <= 65535, "vx_sam_gather_clean_masks: %d masks (1 .. 65535)", N);
    const long px = (long)w * h;
    const int vec = aligned16(masks) && aligned16(out_masks) && px % 16 == 0;
    hipLaunchKernelGGL(clean_gather_kernel, dim3(blocks_for((px + 15) / 16), (unsigned)N), dim3(256), 0, as_stream(stream), masks, px, vec, info_i32, info_f32, changed, keep_idx,
                       first_counts, second_counts, N, out_masks, out_info_i32, out_info_f32, out_counts);
    VX_LAUNCH_CHECK();
    return 1;
}
