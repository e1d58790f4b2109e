// The way back from COCO's uncompressed RLE (kernels_rle.hip writes it), and what both forms of a mask meet in: one bit per pixel in the encoder's own word layout.
// Word (x, s) of a mask sits at x * S + s, S = ceil(h / 64); bit r is pixel (64 s + r, x); bits at and behind row h are zero. A mask's words are in the order of
// p = x * h + y, which is the order of its runs, and masks lie vx_mask_rle_workspace_bytes(w, h, 1) bytes apart, as the encoder's boundary words do.
//   vx_rle_to_bits      CSR rows of runs -> words, per mask two launches:
//     positions  one block of 16 waves per mask scans the runs, 1024 per round: a wave's inclusive scan (cross-lane shifts), the waves' totals through LDS, one
//                carried sum from round to round. Run k's start, cut at h w, goes to the workspace as an i32 (R + 1 entries per mask: the last one is where
//                the last run ends). The sums are i64, so a long row cannot wrap. The same pass gives area (odd runs, each cut at h w) and status.
//     words      one lane per word, a wave 64 consecutive words: 512 contiguous bytes per store. A word covers p0 .. p0 + len of one column. The run that holds p0
//                is found by a binary search over the positions: all lanes first search for the wave's first and last p0 (one address per step, a broadcast
//                load), which brackets each lane's own search. The word starts as that run's parity and takes ~0 << (b - p0) for every boundary b inside
//                it: at most 64 of them in a row without empty runs. A word behind the last run of a short row is background.
//   vx_bits_to_mask_u8  words -> row-major u8 [n][h][w], the encoder's tile step backwards: lane x holds column x's word of a 64 x 64 tile.
//                Byte path: row r of the tile is bit r of every lane, one 64-byte store per row of the wave.
//                16-byte path (16-byte aligned masks, w a multiple of 16): six masked-swap stages across lanes transpose the tile, lane r then holds row r. The
//                rows pass through LDS once so that lane l takes the 16 bits of row 16 k + l / 4, columns 16 (l % 4) ..: four lanes cover a 64-byte row piece,
//                a wave's store 16 rows of them. 4 bits become 4 bytes by one multiplication (bit i to bit 8 i), times the foreground value.
//   vx_mask_to_bits_u8  u8 masks -> words: the encoder's tile pass (kernels_rle.hip, rle_tiles_kernel) stopped before its boundary step.
//   vx_bitmask_iou      na x nb pairs of masks in words: areas first (a wave per mask sums popcounts), then a wave per 4 x 4 tile of pairs, four waves a block
//                of 8 x 8: lanes stride the words, 8 loads feed 16 AND + popcount sums in registers, a cross-lane butterfly folds them, lanes 0 .. 15 write one
//                pair each. No LDS, no atomics; integer sums, the same bits on every run whatever the order.
// transpose64 and nonzero_bytes are the encoder's, restated: its translation unit and device code stay as they are.
#include "vx_common.h"

namespace {

typedef unsigned long long u64;

constexpr int TILE_WAVES = 4;  // waves of a tile block: four consecutive 64-row segments of one strip of 64 columns
constexpr int SCAN_WAVES = 16; // waves of a positions block: 1024 runs per round
constexpr int PAIR = 4;        // a wave's register tile of the IoU matrix: PAIR x PAIR pairs

inline long segments(int h) { return ((long)h + 63) / 64; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline bool extent_ok(int w, int h) { return w > 0 && h > 0 && (long)w * h < (1L << 31) - 1; }

__device__ __forceinline__ bool skipped(const int* __restrict__ counts, int m) { return counts && m >= counts[0]; }

// bit k = byte k of d is non-zero
__device__ __forceinline__ unsigned nonzero_bytes(unsigned d) {
    const unsigned t = (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u;
    return ((t >> 7) * 0x10204080u) >> 28;
}

// byte k = value where bit k of the low four bits of b is set: bit i goes to bit 8 i (i + 7 j are sixteen different positions, no carry)
__device__ __forceinline__ unsigned spread4(unsigned b, unsigned value) { return (((b & 15u) * 0x00204081u) & 0x01010101u) * value; }

// lane r holds row r of a 64 x 64 bit matrix; returns its transpose's row: recursive swap of the off-diagonal blocks of size j
__device__ __forceinline__ u64 transpose64(u64 r, int lane) {
    constexpr u64 low[6] = {0x00000000ffffffffull, 0x0000ffff0000ffffull, 0x00ff00ff00ff00ffull, 0x0f0f0f0f0f0f0f0full, 0x3333333333333333ull, 0x5555555555555555ull};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int j = 32 >> k;
        const u64 m = low[k], t = __shfl_xor(r, j);
        r = (lane & j) ? ((r & ~m) | ((t & ~m) >> j)) : ((r & m) | ((t & m) << j));
    }
    return r;
}

// Row m of the CSR: its runs at runs + offsets[m], R of them, its positions at pos + (offsets[m] - offsets[0]) + m. A row that does not lie inside the total_runs
// the workspace was sized for has R = -1: it is read and written nowhere (the host entries refuse such offsets before any launch).
struct csr_row { long rel, R; };
__device__ __forceinline__ csr_row row_of(const long* __restrict__ offsets, int m, long total_runs) {
    const long rel = offsets[m] - offsets[0], R = offsets[m + 1] - offsets[m];
    const bool ok = rel >= 0 && R >= 0 && rel <= total_runs && R <= total_runs - rel;
    return {ok ? rel : 0, ok ? R : -1};
}

// one block per mask
__global__ __launch_bounds__(64 * SCAN_WAVES) void rle_positions_kernel(const uint32_t* __restrict__ runs, const long* __restrict__ offsets, long total_runs, int w, int h,
                                                                         const int* __restrict__ counts, int first, int* __restrict__ pos, long* __restrict__ area,
                                                                         int* __restrict__ status) {
    __shared__ long wave_sum[SCAN_WAVES];
    const int m = blockIdx.x;
    if (skipped(counts, first + m)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const csr_row row = row_of(offsets, m, total_runs);
    const long hw = (long)w * h, R = row.R;
    if (R < 0) {
        if (tid == 0 && status) status[m] = 1;
        if (tid == 0 && area) area[m] = 0;
        return;
    }
    const uint32_t* src = runs + offsets[m];
    int* out = pos + row.rel + m;
    long carry = 0, fg = 0; // the runs before this round; this thread's foreground pixels
    for (long base = 0; base < R; base += 64 * SCAN_WAVES) {
        const long i = base + tid;
        const long v = i < R ? (long)src[i] : 0;
        long incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        const long T = __shfl(incl, 63);
        if (lane == 0) wave_sum[wave] = T;
        __syncthreads();
        long before = 0, round_total = 0;
#pragma unroll
        for (int u = 0; u < SCAN_WAVES; ++u) {
            const long t = wave_sum[u];
            if (u < wave) before += t;
            round_total += t;
        }
        __syncthreads();
        const long end = carry + before + incl, start = end - v;
        const long cs = start < hw ? start : hw, ce = end < hw ? end : hw;
        if (i < R) out[i] = (int)cs;
        if (i & 1) fg += ce - cs; // v is 0 behind R
        carry += round_total;
    }
    if (tid == 0) {
        out[R] = (int)(carry < hw ? carry : hw);
        if (status) status[m] = carry == hw ? 0 : carry < hw ? 1 : 2;
    }
    if (!area) return;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) fg += __shfl_xor(fg, d);
    if (lane == 0) wave_sum[wave] = fg;
    __syncthreads();
    if (tid == 0) {
        long total = 0;
#pragma unroll
        for (int u = 0; u < SCAN_WAVES; ++u) total += wave_sum[u];
        area[m] = total;
    }
}

// the number of j in 1 .. R with P[j] <= p, known to lie in lo .. hi
__device__ __forceinline__ long runs_up_to(const int* __restrict__ P, long lo, long hi, int p) {
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (P[mid + 1] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// block: 256 consecutive words of mask blockIdx.y, a wave 64 of them
__global__ __launch_bounds__(256) void rle_words_kernel(const long* __restrict__ offsets, long total_runs, int w, int h, int S, const int* __restrict__ counts, int first,
                                                         const int* __restrict__ pos, u64* __restrict__ words, long words_per_mask) {
    const int m = blockIdx.y;
    if (skipped(counts, first + m)) return;
    const int lane = threadIdx.x & 63;
    const long nw = (long)w * S, i = (long)blockIdx.x * 256 + threadIdx.x, i0 = i - lane;
    if (i0 >= nw) return; // the whole wave
    const csr_row row = row_of(offsets, m, total_runs);
    const long R = row.R < 0 ? 0 : row.R;
    const int* P = pos + row.rel + m;
    const unsigned uS = (unsigned)S, uh = (unsigned)h;
    auto p_of = [&](long word) { // p of the word's bit 0; w * S <= w * h, below 2^31
        const unsigned u = (unsigned)word;
        return (int)((u / uS) * uh + (u % uS) * 64u);
    };
    const long i1 = i0 + 63 < nw ? i0 + 63 : nw - 1, mine = i < nw ? i : i1;
    const long k_lo = row.R < 0 ? 0 : runs_up_to(P, 0, R, p_of(i0));
    const long k_hi = row.R < 0 ? 0 : runs_up_to(P, k_lo, R, p_of(i1));
    const int p0 = p_of(mine), len = min(64, h - (int)((unsigned)mine % uS) * 64);
    const long k = runs_up_to(P, k_lo, k_hi, p0); // run k holds p0; k == R: p0 lies behind the last run
    u64 word = (k < R && (k & 1)) ? ~0ull : 0ull;
    for (long j = k + 1; j <= R; ++j) {
        const int b = P[j]; // above p0
        if (b >= p0 + len) break;
        if (j < R || !(R & 1)) word ^= ~0ull << (b - p0); // the end of the last run is a boundary only behind foreground
    }
    if (len < 64) word &= ((u64)1 << len) - 1;
    if (i < nw) words[m * words_per_mask + i] = word;
}

// block (strip of 64 columns x group of four segments, mask blockIdx.y); wave v: segment 4 * group + v
template <bool VEC>
__global__ __launch_bounds__(64 * TILE_WAVES) void bits_to_mask_kernel(const u64* __restrict__ words, long words_per_mask, int w, int h, int S, int seg_groups,
                                                                        const int* __restrict__ counts, int first, unsigned value, uint8_t* __restrict__ masks) {
    __shared__ u64 cw[TILE_WAVES][64];
    __shared__ __attribute__((aligned(16))) u64 rows[TILE_WAVES][64];
    const int m = blockIdx.y;
    if (skipped(counts, first + m)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int strip = blockIdx.x / seg_groups, s0 = (blockIdx.x % seg_groups) * TILE_WAVES, s = s0 + wave;
    const int x0 = strip * 64, y0 = s * 64, x = x0 + lane;
    uint8_t* dst = masks + (long)m * w * h;
    const bool live = s < S; // a wave without a segment still meets the barriers
    const int xo = x0 + (tid >> 2), so = s0 + (tid & 3); // the four segments of a column are 32 contiguous bytes
    cw[tid & 3][tid >> 2] = (xo < w && so < S) ? words[m * words_per_mask + (long)xo * S + so] : 0;
    __syncthreads();
    const u64 c = cw[wave][lane];
    if (VEC) {
        rows[wave][lane] = transpose64(c, lane);
        __syncthreads();
        const uint16_t* pieces = reinterpret_cast<const uint16_t*>(rows[wave]); // pieces 4 r .. 4 r + 3 are row r, left to right
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int row = y0 + 16 * k + (lane >> 2), col = x0 + 16 * (lane & 3);
            const unsigned b = pieces[64 * k + lane];
            const uint4 v = make_uint4(spread4(b, value), spread4(b >> 4, value), spread4(b >> 8, value), spread4(b >> 12, value));
            if (live && row < h && col < w) *reinterpret_cast<uint4*>(dst + (long)row * w + col) = v; // w is a multiple of 16: a piece is inside or outside
        }
    } else if (live && x < w) {
        const int n_rows = min(64, h - y0);
        for (int r = 0; r < n_rows; ++r) dst[(long)(y0 + r) * w + x] = (uint8_t)(((c >> r) & 1) ? value : 0u);
    }
}

// the same block shape, the other way: kernels_rle.hip's rle_tiles_kernel without its boundary step
template <bool VEC>
__global__ __launch_bounds__(64 * TILE_WAVES) void mask_to_bits_kernel(const uint8_t* __restrict__ masks, int w, int h, int S, int seg_groups, const int* __restrict__ counts,
                                                                        int first, u64* __restrict__ words, long words_per_mask) {
    __shared__ u64 cw[TILE_WAVES][64];
    __shared__ __attribute__((aligned(16))) uint16_t pieces[TILE_WAVES][256];
    const int m = blockIdx.y;
    if (skipped(counts, first + m)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int strip = blockIdx.x / seg_groups, s0 = (blockIdx.x % seg_groups) * TILE_WAVES, s = s0 + wave;
    const int x0 = strip * 64, y0 = s * 64, x = x0 + lane;
    const uint8_t* src = masks + (long)m * w * h;
    const bool live = s < S;
    u64 c = 0;
    if (VEC) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int row = y0 + 16 * k + (lane >> 2), col = x0 + 16 * (lane & 3);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (live && row < h && col < w) v = *reinterpret_cast<const uint4*>(src + (long)row * w + col);
            pieces[wave][64 * k + lane] = (uint16_t)(nonzero_bytes(v.x) | nonzero_bytes(v.y) << 4 | nonzero_bytes(v.z) << 8 | nonzero_bytes(v.w) << 12);
        }
        __syncthreads();
        c = transpose64(reinterpret_cast<const u64*>(pieces[wave])[lane], lane);
    } else if (live && x < w) {
        const int n_rows = min(64, h - y0);
        for (int r = 0; r < n_rows; ++r) c |= (u64)(src[(long)(y0 + r) * w + x] != 0) << r;
    }
    cw[wave][lane] = c;
    __syncthreads();
    const int xo = x0 + (tid >> 2), so = s0 + (tid & 3);
    if (xo < w && so < S) words[m * words_per_mask + (long)xo * S + so] = cw[tid & 3][tid >> 2];
}

// a wave per mask, four masks a block
__global__ __launch_bounds__(256) void bits_area_kernel(const u64* __restrict__ words, long words_per_mask, long nw, int n, const int* __restrict__ counts,
                                                         long* __restrict__ area) {
    const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= n || skipped(counts, m)) return;
    const u64* src = words + m * words_per_mask;
    long sum = 0;
    for (long t = lane; t < nw; t += 64) sum += __popcll(src[t]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if (lane == 0) area[m] = sum;
}

// block: 8 x 8 pairs, wave (wave >> 1, wave & 1) its 4 x 4 quarter
__global__ __launch_bounds__(256) void bitmask_iou_kernel(const u64* __restrict__ a, int na, const u64* __restrict__ b, int nb, long words_per_mask, long nw,
                                                           const int* __restrict__ counts_a, const int* __restrict__ counts_b, const long* __restrict__ area_a,
                                                           const long* __restrict__ area_b, const uint8_t* __restrict__ iscrowd, int* __restrict__ inter,
                                                           float* __restrict__ iou) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int live_a = counts_a ? max(0, min(na, counts_a[0])) : na, live_b = counts_b ? max(0, min(nb, counts_b[0])) : nb;
    const int i0 = blockIdx.y * (2 * PAIR) + (wave >> 1) * PAIR, j0 = blockIdx.x * (2 * PAIR) + (wave & 1) * PAIR;
    if (i0 >= live_a || j0 >= live_b) return; // the whole wave
    const u64 *pa[PAIR], *pb[PAIR]; // a row or column behind the live ones repeats the last live one: summed, never stored
#pragma unroll
    for (int r = 0; r < PAIR; ++r) {
        pa[r] = a + min(i0 + r, live_a - 1) * words_per_mask;
        pb[r] = b + min(j0 + r, live_b - 1) * words_per_mask;
    }
    int acc[PAIR * PAIR] = {};
    for (long t = lane; t < nw; t += 64) {
        u64 x[PAIR], y[PAIR];
#pragma unroll
        for (int r = 0; r < PAIR; ++r) {
            x[r] = pa[r][t];
            y[r] = pb[r][t];
        }
#pragma unroll
        for (int q = 0; q < PAIR * PAIR; ++q) acc[q] += __popcll(x[q / PAIR] & y[q % PAIR]);
    }
    int mine = 0; // lane q keeps pair q of the tile
#pragma unroll
    for (int q = 0; q < PAIR * PAIR; ++q) {
        int v = acc[q];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        if (lane == q) mine = v;
    }
    const int i = i0 + lane / PAIR, j = j0 + lane % PAIR;
    if (lane >= PAIR * PAIR || i >= live_a || j >= live_b) return;
    const long den = (iscrowd && iscrowd[j]) ? area_a[i] : area_a[i] + area_b[j] - mine;
    const long at = (long)i * nb + j;
    if (inter) inter[at] = mine;
    iou[at] = den ? (float)mine / (float)den : 0.0f;
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline long words_per_mask_of(int w, int h) { return (long)(vx_mask_rle_workspace_bytes(w, h, 1) / 8); }

} // namespace

extern "C" size_t vx_rle_to_bits_workspace_bytes(int64_t total_runs, int n) {
    if (total_runs < 0 || n < 1 || n > 65535) return 0;
    return up256(((size_t)total_runs + (size_t)n) * 4);
}

extern "C" int vx_rle_to_bits(const uint32_t* runs, const int64_t* offsets, int64_t total_runs, int n, int w, int h, const int32_t* counts, int first, void* words,
                              int64_t* area, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    VX_REQUIRE(runs && offsets && words && workspace, "vx_rle_to_bits: null operand");
    VX_REQUIRE(extent_ok(w, h), "vx_rle_to_bits: extent %d x %d (w, h >= 1, w * h below 2^31 - 1)", w, h);
    VX_REQUIRE(n > 0 && n <= 65535 && first >= 0 && total_runs >= 0, "vx_rle_to_bits: %d masks (1 .. 65535) from %d, %lld runs", n, first, (long long)total_runs);
    VX_REQUIRE(aligned8(words) && aligned16(workspace) && workspace_bytes >= vx_rle_to_bits_workspace_bytes(total_runs, n),
               "vx_rle_to_bits: words 8-byte aligned, workspace of %zu bytes (16-byte aligned, at least %zu)", workspace_bytes, vx_rle_to_bits_workspace_bytes(total_runs, n));
    static_assert(sizeof(long) == sizeof(int64_t), "offsets and areas are read as long");
    hipStream_t s = as_stream(stream);
    const int S = (int)segments(h);
    const long* off = reinterpret_cast<const long*>(offsets);
    int* pos = static_cast<int*>(workspace);
    hipLaunchKernelGGL(rle_positions_kernel, dim3((unsigned)n), dim3(64 * SCAN_WAVES), 0, s, runs, off, (long)total_runs, w, h, counts, first, pos,
                       reinterpret_cast<long*>(area), status);
    VX_LAUNCH_CHECK();
    hipLaunchKernelGGL(rle_words_kernel, dim3(blocks_for((long)w * S), (unsigned)n), dim3(256), 0, s, off, (long)total_runs, w, h, S, counts, first, pos,
                       static_cast<u64*>(words), words_per_mask_of(w, h));
    VX_LAUNCH_CHECK();
    return 1;
}

namespace {

// the grid of the two tile kernels: (strips x groups of four segments, masks)
bool tile_grid(int w, int h, int n, dim3* grid, int* S, int* seg_groups) {
    *S = (int)segments(h);
    *seg_groups = (*S + TILE_WAVES - 1) / TILE_WAVES;
    const long strips = ((long)w + 63) / 64;
    if (strips * *seg_groups >= (1L << 31)) return false;
    *grid = dim3((unsigned)(strips * *seg_groups), (unsigned)n);
    return true;
}

} // namespace

extern "C" int vx_bits_to_mask_u8(const void* words, int n, int w, int h, const int32_t* counts, int first, int value, uint8_t* masks, void* stream) {
    VX_REQUIRE(words && masks && aligned8(words), "vx_bits_to_mask_u8: null operand, or words not 8-byte aligned");
    VX_REQUIRE(extent_ok(w, h), "vx_bits_to_mask_u8: extent %d x %d (w, h >= 1, w * h below 2^31 - 1)", w, h);
    VX_REQUIRE(n > 0 && n <= 65535 && first >= 0, "vx_bits_to_mask_u8: %d masks (1 .. 65535) from %d", n, first);
    VX_REQUIRE(value >= 1 && value <= 255, "vx_bits_to_mask_u8: foreground value %d (1 .. 255)", value);
    dim3 grid;
    int S, seg_groups;
    VX_REQUIRE(tile_grid(w, h, n, &grid, &S, &seg_groups), "vx_bits_to_mask_u8: extent %d x %d", w, h);
    const u64* src = static_cast<const u64*>(words);
    if (aligned16(masks) && w % 16 == 0)
        hipLaunchKernelGGL(bits_to_mask_kernel<true>, grid, dim3(64 * TILE_WAVES), 0, as_stream(stream), src, words_per_mask_of(w, h), w, h, S, seg_groups, counts, first,
                           (unsigned)value, masks);
    else
        hipLaunchKernelGGL(bits_to_mask_kernel<false>, grid, dim3(64 * TILE_WAVES), 0, as_stream(stream), src, words_per_mask_of(w, h), w, h, S, seg_groups, counts, first,
                           (unsigned)value, masks);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_mask_to_bits_u8(const uint8_t* masks, int n, int w, int h, const int32_t* counts, int first, void* words, void* stream) {
    VX_REQUIRE(words && masks && aligned8(words), "vx_mask_to_bits_u8: null operand, or words not 8-byte aligned");
    VX_REQUIRE(extent_ok(w, h), "vx_mask_to_bits_u8: extent %d x %d (w, h >= 1, w * h below 2^31 - 1)", w, h);
    VX_REQUIRE(n > 0 && n <= 65535 && first >= 0, "vx_mask_to_bits_u8: %d masks (1 .. 65535) from %d", n, first);
    dim3 grid;
    int S, seg_groups;
    VX_REQUIRE(tile_grid(w, h, n, &grid, &S, &seg_groups), "vx_mask_to_bits_u8: extent %d x %d", w, h);
    u64* dst = static_cast<u64*>(words);
    if (aligned16(masks) && w % 16 == 0)
        hipLaunchKernelGGL(mask_to_bits_kernel<true>, grid, dim3(64 * TILE_WAVES), 0, as_stream(stream), masks, w, h, S, seg_groups, counts, first, dst, words_per_mask_of(w, h));
    else
        hipLaunchKernelGGL(mask_to_bits_kernel<false>, grid, dim3(64 * TILE_WAVES), 0, as_stream(stream), masks, w, h, S, seg_groups, counts, first, dst, words_per_mask_of(w, h));
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" size_t vx_bitmask_iou_workspace_bytes(int na, int nb) {
    if (na < 1 || nb < 1 || na > 65535 || nb > 65535) return 0;
    return up256(((size_t)na + (size_t)nb) * 8);
}

extern "C" int vx_bitmask_iou(const void* a_words, int na, const void* b_words, int nb, int w, int h, const int32_t* counts_a, const int32_t* counts_b,
                              const uint8_t* iscrowd, int32_t* inter, float* iou, void* workspace, size_t workspace_bytes, void* stream) {
    VX_REQUIRE(a_words && b_words && iou && workspace, "vx_bitmask_iou: null operand");
    VX_REQUIRE(extent_ok(w, h), "vx_bitmask_iou: extent %d x %d (w, h >= 1, w * h below 2^31 - 1)", w, h);
    VX_REQUIRE(na > 0 && nb > 0 && na <= 65535 && nb <= 65535, "vx_bitmask_iou: %d x %d masks (1 .. 65535 each)", na, nb);
    VX_REQUIRE(aligned8(a_words) && aligned8(b_words) && aligned16(workspace) && workspace_bytes >= vx_bitmask_iou_workspace_bytes(na, nb),
               "vx_bitmask_iou: words 8-byte aligned, workspace of %zu bytes (16-byte aligned, at least %zu)", workspace_bytes, vx_bitmask_iou_workspace_bytes(na, nb));
    hipStream_t s = as_stream(stream);
    const long wpm = words_per_mask_of(w, h), nw = (long)w * segments(h);
    const u64 *a = static_cast<const u64*>(a_words), *b = static_cast<const u64*>(b_words);
    long *area_a = static_cast<long*>(workspace), *area_b = area_a + na;
    hipLaunchKernelGGL(bits_area_kernel, dim3(blocks_for(na, 4)), dim3(256), 0, s, a, wpm, nw, na, counts_a, area_a);
    VX_LAUNCH_CHECK();
    hipLaunchKernelGGL(bits_area_kernel, dim3(blocks_for(nb, 4)), dim3(256), 0, s, b, wpm, nw, nb, counts_b, area_b);
    VX_LAUNCH_CHECK();
    hipLaunchKernelGGL(bitmask_iou_kernel, dim3(blocks_for(nb, 2 * PAIR), blocks_for(na, 2 * PAIR)), dim3(256), 0, s, a, na, b, nb, wpm, nw, counts_a, counts_b, area_a, area_b,
                       iscrowd, inter, iou);
    VX_LAUNCH_CHECK();
    return 1;
}
