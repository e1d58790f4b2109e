// COCO's uncompressed run-length encoding of u8 masks on the device, as SAM's mask_to_rle_pytorch writes it: pixels in column-major order p = x * h + y,
// counts[0] the leading background run (0 when pixel 0 is foreground), runs alternating from there and continuing across column ends.
//   vx_mask_rle_workspace_bytes    bytes of workspace for `group` masks of w x h in flight: the boundary words, one bit per pixel
//   vx_mask_rle_packed_u8          vx_mask_rle_u8 with mask b's runs at runs + offsets[b], of offsets[b + 1] - offsets[b] entries: rows of their own lengths (CSR)
//   vx_mask_rle_u8                 per group of masks two launches:
//     tiles    a wave turns one 64 x 64 tile of the row-major mask into 64 COLUMN words (bit r of lane x's word = pixel (y0 + r, x0 + x) != 0) and from them the
//              boundary words b = c ^ ((c << 1) | carry): bit r is set iff pixel p differs from pixel p - 1. carry is the pixel above the tile, for row 0 the last
//              pixel of the column before, for p = 0 background; it is read from the mask, so no tile waits for another. Rows behind h and columns behind w are
//              masked out of b. The words go to the workspace in the order of p: word (x, s) at x * S + s, S = ceil(h / 64), four waves of a block writing the four
//              consecutive segments of their columns as 32-byte pieces.
//              Where the masks are 16-byte aligned and w is a multiple of 16 the tile is read as four 16-byte loads per lane (lane l: row 16 k + l / 4, bytes
//              16 (l % 4) ..), each reduced to 16 bits in registers; the pieces pass through LDS once so that lane r holds row r's 64-bit word, and six
//              exchange stages across lanes (partner lane ^ 32, 16, .. 1, a masked swap of half the bits each) transpose the 64 x 64 bit matrix.
//              Otherwise lane x reads its column's 64 bytes row by row (each row of the wave one 64-byte piece) and shifts them into its column word directly.
//     scan     one block of 16 waves per mask walks the words in order, 1024 per round. A wave's inclusive scan of popc(b) (cross-lane shifts) ranks its 64 words,
//              the waves' totals and last boundary positions meet in LDS, and two running values carry from round to round: boundaries so far, and the position
//              of the last one (positions only grow, so "last so far" is a maximum). A wave then writes its boundaries 64 ranks at a time: lane q finds the word
//              that holds rank q by a binary search over the wave's scan (six cross-lane reads), picks the bit by a binary search over popc, and takes the
//              position before it from lane q - 1 (lane 0: the carried one). run[rank] = position - previous position, consecutive ranks in consecutive
//              lanes: coalesced stores, cut by a comparison of the rank with run_stride. Thread 0 writes the last run, h w - last position, and n_runs.
//              Without runs to write (the count-only form) the scan is a sum.
// Keeping the boundary words costs 1/8 of the mask's bytes written and read again; deriving them a second time in the scan would read the mask twice.
// Integers only, no atomics: every output is a function of the mask alone, the same bytes on every run.
#include "vx_common.h"

namespace {

typedef unsigned long long u64;

constexpr int TILE_WAVES = 4;   // waves of a tiles block: four consecutive 64-row segments of one strip of 64 columns
constexpr int SCAN_WAVES = 16;  // waves of a scan block: 1024 words per round

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline long segments(int h) { return ((long)h + 63) / 64; }

__device__ __forceinline__ bool skipped(const int* __restrict__ counts, int m) { return counts && m >= counts[0]; }

// bit k = byte k of d is non-zero
__device__ __forceinline__ unsigned nonzero_bytes(unsigned d) {
    const unsigned t = (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u;
    return ((t >> 7) * 0x10204080u) >> 28;
}

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

// block (strip of 64 columns x group of four segments, mask of the launch's group); wave v: segment 4 * group + v
template <bool VEC>
__global__ __launch_bounds__(64 * TILE_WAVES) void rle_tiles_kernel(const uint8_t* __restrict__ masks, int w, int h, int S, int seg_groups, const int* __restrict__ counts,
                                                                     int k0, u64* __restrict__ words, long words_per_mask) {
    __shared__ u64 bw[TILE_WAVES][64];
    __shared__ __attribute__((aligned(16))) uint16_t pieces[TILE_WAVES][256];
    const int j = blockIdx.y, m = k0 + j;
    if (skipped(counts, m)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int strip = blockIdx.x / seg_groups, s0 = (blockIdx.x % seg_groups) * TILE_WAVES, s = s0 + wave;
    const int x0 = strip * 64, y0 = s * 64, x = x0 + lane;
    const uint8_t* src = masks + (long)m * w * h;
    const bool live = s < S; // a wave without a segment still meets the barriers
    u64 c = 0;
    if (VEC) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int row = y0 + 16 * k + (lane >> 2), col = x0 + 16 * (lane & 3);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (live && row < h && col < w) v = *reinterpret_cast<const uint4*>(src + (long)row * w + col); // w is a multiple of 16: a piece is inside or outside
            pieces[wave][64 * k + lane] = (uint16_t)(nonzero_bytes(v.x) | nonzero_bytes(v.y) << 4 | nonzero_bytes(v.z) << 8 | nonzero_bytes(v.w) << 12);
        }
        __syncthreads();
        c = transpose64(reinterpret_cast<const u64*>(pieces[wave])[lane], lane); // pieces 4 r .. 4 r + 3 are row r, left to right
    } else if (live && x < w) {
        const int rows = min(64, h - y0);
        for (int r = 0; r < rows; ++r) c |= (u64)(src[(long)(y0 + r) * w + x] != 0) << r;
    }
    u64 b = 0;
    if (live && x < w) {
        unsigned above = 0; // the pixel before the tile's first one of this column in the order of p
        if (y0 > 0) above = src[(long)(y0 - 1) * w + x] != 0;
        else if (x > 0) above = src[(long)(h - 1) * w + x - 1] != 0;
        b = c ^ ((c << 1) | above);
        if (h - y0 < 64) b &= ((u64)1 << (h - y0)) - 1;
    }
    bw[wave][lane] = b;
    __syncthreads();
    const int xo = x0 + (tid >> 2), so = s0 + (tid & 3);
    if (xo < w && so < S) words[j * words_per_mask + (long)xo * S + so] = bw[tid & 3][tid >> 2];
}

// position in the word of its r-th set bit (0-based, r below its popc)
__device__ __forceinline__ int select_bit(u64 word, int r) {
    unsigned v = (unsigned)word;
    int pos = 0, c = __popc(v);
    if (r >= c) {
        r -= c;
        pos = 32;
        v = (unsigned)(word >> 32);
    }
#pragma unroll
    for (int width = 16; width >= 1; width >>= 1) {
        c = __popc(v & ((1u << width) - 1));
        if (r >= c) {
            r -= c;
            v >>= width;
            pos += width;
        }
    }
    return pos;
}

// one block per mask of the launch's group
template <bool WRITE>
__global__ __launch_bounds__(64 * SCAN_WAVES) void rle_scan_kernel(const u64* __restrict__ words, long words_per_mask, int w, int h, int S, const int* __restrict__ counts,
                                                                    int k0, uint32_t* __restrict__ runs, long run_stride, const long* __restrict__ offsets,
                                                                    int* __restrict__ n_runs) {
    __shared__ int wave_total[SCAN_WAVES];
    __shared__ unsigned wave_last[SCAN_WAVES];
    const int j = blockIdx.x, m = k0 + j;
    if (skipped(counts, m)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64* src = words + j * words_per_mask;
    const long nw = (long)w * S;
    // mask m's row: runs + m * run_stride of run_stride entries, or with offsets (the packed form) runs + offsets[m] of offsets[m + 1] - offsets[m]
    uint32_t* out = !WRITE ? nullptr : offsets ? runs + offsets[m] : runs + (long)m * run_stride;
    if (WRITE && offsets) run_stride = offsets[m + 1] - offsets[m];
    int total = 0;      // boundaries before this round
    unsigned last = 0;  // position of the last of them; 0 without one, which is what the first run subtracts
    for (long base = 0; base < nw; base += 64 * SCAN_WAVES) {
        const long i = base + tid;
        const u64 word = i < nw ? src[i] : 0;
        const int c = __popcll(word);
        if (!WRITE) { // the count alone: every thread sums its own words
            total += c;
            continue;
        }
        const unsigned iu = (unsigned)i; // w * S <= w * h, below 2^31
        const unsigned pos0 = i < nw ? (iu / (unsigned)S) * (unsigned)h + (iu % (unsigned)S) * 64u : 0; // p of the word's bit 0
        int incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        const int T = __shfl(incl, 63);
        const u64 holders = __ballot(c > 0);
        const unsigned mine = c ? pos0 + 63 - __clzll(word) : 0;
        const unsigned wl = holders ? __shfl(mine, 63 - __clzll(holders)) : 0;
        if (lane == 0) {
            wave_total[wave] = T;
            wave_last[wave] = wl;
        }
        __syncthreads();
        int before = 0, round_total = 0;
        unsigned carried = last, round_last = last;
#pragma unroll
        for (int u = 0; u < SCAN_WAVES; ++u) {
            const int t = wave_total[u];
            const unsigned l = wave_last[u];
            if (u < wave) {
                before += t;
                carried = max(carried, l);
            }
            round_total += t;
            round_last = max(round_last, l);
        }
        __syncthreads();
        // the wave's T boundaries, 64 ranks at a time
        const int excl = incl - c;
        const long rank0 = (long)total + before;
        for (int q0 = 0; q0 < T && rank0 + q0 < run_stride; q0 += 64) {
            const int q = q0 + lane;
            int L = 0; // the largest lane whose exclusive scan is at most q: its word holds rank q
#pragma unroll
            for (int step = 32; step >= 1; step >>= 1) {
                const int e = __shfl(excl, L + step);
                if (e <= q) L += step;
            }
            const u64 wL = __shfl(word, L);
            const int eL = __shfl(excl, L);
            const unsigned pL = __shfl(pos0, L);
            const unsigned P = q < T ? pL + select_bit(wL, q - eL) : 0;
            unsigned prev = __shfl_up(P, 1);
            if (lane == 0) prev = carried;
            carried = __shfl(P, 63);
            if (q < T && rank0 + q < run_stride) out[rank0 + q] = P - prev;
        }
        total += round_total;
        last = round_last;
    }
    if (!WRITE) { // block sum of the threads' counts
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) total += __shfl_xor(total, d);
        if (lane == 0) wave_total[wave] = total;
        __syncthreads();
        total = 0;
#pragma unroll
        for (int u = 0; u < SCAN_WAVES; ++u) total += wave_total[u];
    }
    if (tid == 0) {
        n_runs[m] = total + 1;
        if (WRITE && total < run_stride) out[total] = (unsigned)((long)w * h) - last;
    }
}

} // namespace

extern "C" size_t vx_mask_rle_workspace_bytes(int w, int h, int group) {
    if (w < 1 || h < 1 || group < 1 || group > 65535 || (long)w * h >= (1L << 31) - 1) return 0;
    return (size_t)group * up256((size_t)w * segments(h) * 8);
}

namespace {

int rle_launch(const char* who, const uint8_t* masks, int w, int h, int n, const int32_t* counts, uint32_t* runs, int64_t run_stride, const int64_t* offsets, int32_t* n_runs,
               void* workspace, size_t workspace_bytes, int group, void* stream) {
    VX_REQUIRE(masks && n_runs && workspace, "%s: null operand", who);
    VX_REQUIRE(w > 0 && h > 0 && (long)w * h < (1L << 31) - 1, "%s: extent %d x %d (w, h >= 1, w * h below 2^31 - 1)", who, w, h);
    VX_REQUIRE(n > 0 && group > 0 && group <= 65535, "%s: %d masks in groups of %d (1 .. 65535)", who, n, group);
    VX_REQUIRE(run_stride >= 0, "%s: run_stride %lld below 0", who, (long long)run_stride);
    VX_REQUIRE(aligned16(workspace) && workspace_bytes >= vx_mask_rle_workspace_bytes(w, h, group), "%s: workspace of %zu bytes (16-byte aligned, at least %zu)", who,
               workspace_bytes, vx_mask_rle_workspace_bytes(w, h, group));
    hipStream_t s = as_stream(stream);
    const int S = (int)segments(h);
    const long words_per_mask = (long)(up256((size_t)w * S * 8) / 8);
    const int strips = (w + 63) / 64, seg_groups = (S + TILE_WAVES - 1) / TILE_WAVES;
    VX_REQUIRE((long)strips * seg_groups < (1L << 31), "%s: extent %d x %d", who, w, h);
    const bool vec = aligned16(masks) && w % 16 == 0, write = runs && (offsets || run_stride > 0);
    u64* words = static_cast<u64*>(workspace);
    static_assert(sizeof(long) == sizeof(int64_t), "offsets are read as long");
    for (int k0 = 0; k0 < n; k0 += group) {
        const unsigned g = (unsigned)(n - k0 < group ? n - k0 : group);
        const dim3 grid((unsigned)(strips * seg_groups), g);
        if (vec) hipLaunchKernelGGL(rle_tiles_kernel<true>, grid, dim3(64 * TILE_WAVES), 0, s, masks, w, h, S, seg_groups, counts, k0, words, words_per_mask);
        else hipLaunchKernelGGL(rle_tiles_kernel<false>, grid, dim3(64 * TILE_WAVES), 0, s, masks, w, h, S, seg_groups, counts, k0, words, words_per_mask);
        VX_LAUNCH_CHECK();
        if (write)
            hipLaunchKernelGGL(rle_scan_kernel<true>, dim3(g), dim3(64 * SCAN_WAVES), 0, s, words, words_per_mask, w, h, S, counts, k0, runs, (long)run_stride,
                               reinterpret_cast<const long*>(offsets), n_runs);
        else hipLaunchKernelGGL(rle_scan_kernel<false>, dim3(g), dim3(64 * SCAN_WAVES), 0, s, words, words_per_mask, w, h, S, counts, k0, runs, 0L, nullptr, n_runs);
        VX_LAUNCH_CHECK();
    }
    return 1;
}

} // namespace

extern "C" int vx_mask_rle_u8(const uint8_t* masks, int w, int h, int n, const int32_t* counts, uint32_t* runs, int64_t run_stride, int32_t* n_runs, void* workspace,
                              size_t workspace_bytes, int group, void* stream) {
    return rle_launch("vx_mask_rle_u8", masks, w, h, n, counts, runs, run_stride, nullptr, n_runs, workspace, workspace_bytes, group, stream);
}

extern "C" int vx_mask_rle_packed_u8(const uint8_t* masks, int w, int h, int n, const int64_t* offsets, uint32_t* runs, int32_t* n_runs, void* workspace,
                                     size_t workspace_bytes, int group, void* stream) {
    VX_REQUIRE(offsets && runs, "vx_mask_rle_packed_u8: null operand");
    return rle_launch("vx_mask_rle_packed_u8", masks, w, h, n, nullptr, runs, 0, offsets, n_runs, workspace, workspace_bytes, group, stream);
}
