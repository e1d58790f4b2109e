// COCO's compressed counts string (pycocotools' rleToString / rleFrString) on the device, both ways, on CSR rows: runs u32 + offsets i64 [n + 1] as the encoder's
// packed call writes them, strings u8 + byte_offsets i64 [n + 1]. Run i of a record is coded as x = c[i] (i <= 2) or c[i] - c[i - 2] (i > 2), a signed value cut
// into 5-bit groups from the least significant one: byte = group + 48, bit 5 of the group = "more follow"; the last group's bit 4 is the sign of what is above it.
//   vx_rle_compress    one lane per run, a block of four waves 256 runs a round, a CHUNK of 1024 runs (four rounds) per block and grid step: a record of R runs is
//                ceil(R / 1024) chunks, grid (chunks of the longest record, capped; records), a block strides over its record's chunks. Three launches:
//     sums       each chunk's bytes: c[i - 2] comes from two lanes back (a cross-lane shift), for a wave's first two lanes from the previous wave's last two through
//                LDS, for a round's first two from the previous round's (LDS, double-buffered by the round's parity), for a chunk's first two by ONE two-lane load
//                per chunk. The length of x is (37 - clz(x < 0 ? ~x : x)) / 5: the bits up to the highest significant one, plus the sign, in groups of five.
//     prefix     a wave per record turns its chunks' sums into their running sum in place (wave scan, a carried sum) and writes the record's size.
//     bytes      the lengths again, a wave scan + the waves' totals + the carried sum of the rounds + the chunk's running sum = each value's place in the string.
//                A round's bytes (at most 1792) are assembled in LDS at the string's own phase modulo 16, and leave as 16-byte stores for every aligned piece
//                that lies wholly inside the round, byte stores for the ragged ends: no byte outside the round's range is touched, whatever the row's base.
//   vx_rle_decompress  one lane per byte, one block of 8 waves per record, 512 bytes a round, ONE launch (a record is not split: a long string takes rounds).
//                A byte without bit 5 ends a value: ballot + popcount below the lane + the waves' counts + the carried count = the value's index. The lane at
//                a value's last byte walks back over at most six more bytes in LDS (the round's bytes behind an 8-byte halo of the round before), and puts the
//                value at its index in LDS. Then one lane per VALUE: c[i] = x[i] + c[i - 2] is two interleaved prefix sums, so the wave scan steps 2, 4 .. 32 lanes,
//                lanes 62 and 63 hold the wave's two chain totals, and a pair of i64 sums is carried from round to round by the value index's parity; c[0]
//                stays out of both chains. Consecutive values leave from consecutive lanes.
// Integers only, no atomics, no scratch; the same bytes on every run. Every store is held below the capacity of its own row (offsets[m + 1] - offsets[m]).
#include "vx_common.h"

namespace {

typedef unsigned long long u64;

constexpr int CW = 4;         // waves of a compress block
constexpr int CT = 64 * CW;   // runs of a round
constexpr int CHUNK = 4 * CT; // runs of a chunk
constexpr int MAX_GRID_X = 1024;
constexpr int DW = 8;         // waves of a decompress block
constexpr int DT = 64 * DW;   // bytes of a round
constexpr int HALO = 8;       // bytes of the round before kept in front of a round's: a value has at most 7, one more shows an eighth

__device__ __forceinline__ bool skipped(const int* __restrict__ counts, int m) { return counts && m >= counts[0]; }

// Row m of the run CSR, as kernels_rle_decode.hip reads it: rel = its first run behind offsets[0]; a row outside total_runs has R = -1 and is touched nowhere
struct csr_row { long rel, R; };
__device__ __forceinline__ csr_row row_of(const long* __restrict__ offsets, int m, long total_runs) {
    const long rel = offsets[m] - offsets[0], R = offsets[m + 1] - offsets[m];
    const bool ok = rel >= 0 && R >= 0 && rel <= total_runs && R <= total_runs - rel;
    return {ok ? rel : 0, ok ? R : -1};
}

// bytes of x: the smallest k with -2^(5k - 1) <= x < 2^(5k - 1); 1 .. 7
__device__ __forceinline__ int value_bytes(int x) { return (37 - __clz(x < 0 ? ~x : x)) / 5; }

// WRITE = false: chunk c's bytes -> chunk_ws[c]. WRITE = true: chunk_ws[c] holds the record's bytes before chunk c; the chunk's bytes are written.
template <bool WRITE>
__global__ __launch_bounds__(CT) void rle_compress_kernel(const uint32_t* __restrict__ runs, const long* __restrict__ offsets, long total_runs, const int* __restrict__ counts,
                                                          int first, int* __restrict__ chunk_ws, uint8_t* __restrict__ bytes, const long* __restrict__ byte_offsets) {
    __shared__ uint32_t seam[2][CW + 1][2]; // [round parity][wave]: the two runs in front of the wave's
    __shared__ int wave_sum[CW];
    __shared__ __attribute__((aligned(16))) uint8_t stage[16 + 7 * CT + 16];
    const int m = blockIdx.y;
    if (skipped(counts, first + m)) return;
    const csr_row row = row_of(offsets, m, total_runs);
    if (row.R <= 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t* src = runs + offsets[m];
    int* ws = chunk_ws + row.rel / CHUNK + m; // chunks of the rows before: at most rel / CHUNK + m
    const long n_chunks = (row.R + CHUNK - 1) / CHUNK;
    long cap = 0;
    uint8_t* dst = nullptr;
    if (WRITE) {
        cap = byte_offsets[m + 1] - byte_offsets[m];
        dst = bytes + byte_offsets[m];
    }
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const long i0 = c * CHUNK, i1 = min(row.R, i0 + (long)CHUNK);
        if (tid < 2) seam[0][0][tid] = i0 >= 2 ? src[i0 - 2 + tid] : 0u; // the chunk seam
        long at = WRITE ? (long)ws[c] : 0; // the record's bytes in front of the round
        int mine = 0, q = 0;
        for (long base = i0; base < i1; base += CT, q ^= 1) {
            const long i = base + tid;
            const bool live = i < i1;
            const uint32_t v = live ? src[i] : 0u;
            if (lane >= 62) {
                if (wave < CW - 1) seam[q][wave + 1][lane - 62] = v;
                else seam[q ^ 1][0][lane - 62] = v; // the round seam
            }
            __syncthreads();
            uint32_t p = __shfl_up(v, 2);
            if (lane < 2) p = seam[q][wave][lane];
            const int x = (int)(i > 2 ? v - p : v);
            const int len = live ? value_bytes(x) : 0;
            if (!WRITE) {
                mine += len;
                __syncthreads(); // the next round writes the seams this one read
                continue;
            }
            int incl = len;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            if (lane == 63) wave_sum[wave] = incl;
            __syncthreads();
            int before = 0, round_total = 0;
#pragma unroll
            for (int u = 0; u < CW; ++u) {
                const int t = wave_sum[u];
                if (u < wave) before += t;
                round_total += t;
            }
            uint8_t* out = dst + at; // the round's first byte
            const int shift = (int)(reinterpret_cast<uintptr_t>(out) & 15);
            const int s = shift + before + incl - len;
#pragma unroll
            for (int k = 0; k < 7; ++k)
                if (k < len) stage[s + k] = (uint8_t)(((x >> (5 * k)) & 31) + (k + 1 < len ? 32 : 0) + 48);
            __syncthreads();
            // piece t: the 16 bytes at out - shift + 16 t, bytes lo .. lo + 16 of the round
            const int lo = 16 * tid - shift;
            const long room = min((long)round_total, cap - at); // bytes of the round the row has room for
            if (lo + 16 > 0 && lo < room) {
                if (lo >= 0 && lo + 16 <= room) {
                    *reinterpret_cast<uint4*>(out + lo) = *reinterpret_cast<const uint4*>(stage + 16 * tid);
                } else {
#pragma unroll
                    for (int k = 0; k < 16; ++k)
                        if (lo + k >= 0 && lo + k < room) out[lo + k] = stage[16 * tid + k];
                }
            }
            at += round_total;
            __syncthreads(); // stage, wave_sum and the seams are free again
        }
        if (!WRITE) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
            if (lane == 0) wave_sum[wave] = mine;
            __syncthreads();
            if (tid == 0) {
                int total = 0;
#pragma unroll
                for (int u = 0; u < CW; ++u) total += wave_sum[u];
                ws[c] = total;
            }
            __syncthreads();
        }
    }
}

// a wave per record, four records a block: the chunks' sums -> the sum of the chunks before each, in place; the record's size
__global__ __launch_bounds__(256) void rle_chunk_prefix_kernel(const long* __restrict__ offsets, long total_runs, int n, const int* __restrict__ counts, int first,
                                                                int* __restrict__ chunk_ws, int* __restrict__ sizes) {
    const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= n || skipped(counts, first + m)) return;
    const csr_row row = row_of(offsets, m, total_runs);
    int* ws = chunk_ws + row.rel / CHUNK + m;
    const long n_chunks = row.R < 0 ? 0 : (row.R + CHUNK - 1) / CHUNK;
    int carry = 0;
    for (long base = 0; base < n_chunks; base += 64) {
        const long c = base + lane;
        const int v = c < n_chunks ? ws[c] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        if (c < n_chunks) ws[c] = carry + incl - v;
        carry += __shfl(incl, 63);
    }
    if (lane == 0 && sizes) sizes[m] = carry;
}

// one block per record; runs == nullptr: sizes and status only
__global__ __launch_bounds__(DT) void rle_decompress_kernel(const uint8_t* __restrict__ bytes, const long* __restrict__ byte_offsets, const int* __restrict__ counts, int first,
                                                            uint32_t* __restrict__ runs, const long* __restrict__ offsets, int* __restrict__ sizes, int* __restrict__ status) {
    __shared__ uint8_t stage[2][HALO + DT]; // [round parity]: the last HALO bytes of the round before, then the round's
    __shared__ long vals[DT];               // the round's values by index
    __shared__ long pair_total[DW][2];      // a wave's two chain sums
    __shared__ int wave_count[DW];
    const int m = blockIdx.x;
    if (skipped(counts, first + m)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long B = max(0L, byte_offsets[m + 1] - byte_offsets[m]);
    const uint8_t* src = bytes + byte_offsets[m];
    long cap = 0;
    uint32_t* dst = nullptr;
    if (runs) {
        cap = offsets[m + 1] - offsets[m];
        dst = runs + offsets[m];
    }
    long rank_base = 0, chain[2] = {0, 0}; // values before the round; the sums of the even chain (from c[2]) and the odd chain (from c[1])
    int flags = 0, q = 0;                  // bit k: status k + 1 was met
    for (long base = 0; base < B; base += DT, q ^= 1) {
        const long pos = base + tid;
        const bool live = pos < B;
        const int b = live ? src[pos] : 48;
        stage[q][HALO + tid] = (uint8_t)b;
        if (tid >= DT - HALO) stage[q ^ 1][tid - (DT - HALO)] = (uint8_t)b;
        const int g = b - 48;
        const bool ends = live && !(g & 32);
        if (b < 48 || b > 111) flags |= 1;
        if (live && pos == B - 1 && (g & 32)) flags |= 2;
        const u64 ballot = __ballot(ends);
        if (lane == 0) wave_count[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, n_values = 0;
#pragma unroll
        for (int u = 0; u < DW; ++u) {
            const int t = wave_count[u];
            if (u < wave) before += t;
            n_values += t;
        }
        if (ends) {
            const uint8_t* at = &stage[q][HALO + tid];
            long x = g & 31;
            int len = 1;
            bool open = true; // no earlier value's end and not the string's start met yet
#pragma unroll
            for (int k = 1; k < 7; ++k) {
                const int e = at[-k] - 48;
                open = open && pos - k >= 0 && (e & 32);
                if (open) {
                    x = (x << 5) | (e & 31);
                    ++len;
                }
            }
            if (open && pos - 7 >= 0 && ((at[-7] - 48) & 32)) flags |= 4;
            if (g & 16) x |= ~0L << (5 * len);
            vals[before + __popcll(ballot & (((u64)1 << lane) - 1))] = x;
        }
        __syncthreads();
        const long i = rank_base + tid; // one lane per value from here
        const bool mine = tid < n_values;
        const long x = mine ? vals[tid] : 0;
        long y = i == 0 ? 0 : x;
#pragma unroll
        for (int d = 2; d < 64; d <<= 1) {
            const long t = __shfl_up(y, d);
            if (lane >= d) y += t;
        }
        if (lane >= 62) pair_total[wave][lane - 62] = y;
        __syncthreads();
        long ahead = 0, total[2] = {0, 0};
#pragma unroll
        for (int u = 0; u < DW; ++u) {
            const long t0 = pair_total[u][0], t1 = pair_total[u][1];
            if (u < wave) ahead += (lane & 1) ? t1 : t0;
            total[0] += t0;
            total[1] += t1;
        }
        const bool swap = rank_base & 1; // the round's lane parity against the value index's
        const long c = i == 0 ? x : ((i & 1) ? chain[1] : chain[0]) + ahead + y;
        if (mine) {
            if (c < 0 || c > 0x7fffffffL) flags |= 8;
            if (i < cap) dst[i] = (uint32_t)c;
        }
        chain[0] += swap ? total[1] : total[0];
        chain[1] += swap ? total[0] : total[1];
        rank_base += n_values;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) flags |= __shfl_xor(flags, d);
    __syncthreads();
    if (lane == 0) wave_count[wave] = flags;
    __syncthreads();
    if (tid == 0) {
        int all = 0;
#pragma unroll
        for (int u = 0; u < DW; ++u) all |= wave_count[u];
        const int st = all ? __ffs(all) : 0; // the lowest status met
        if (sizes) sizes[m] = st ? 0 : (int)min(rank_base, 0x7fffffffL);
        if (status) status[m] = st;
    }
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr int64_t MAX_TOTAL_RUNS = ((int64_t(1) << 31) - 1) / 7; // a record's size is an i32

} // namespace

extern "C" size_t vx_rle_compress_workspace_bytes(int64_t total_runs, int n) {
    if (total_runs < 0 || total_runs > MAX_TOTAL_RUNS || n < 1 || n > 65535) return 0;
    return up256(((size_t)(total_runs / CHUNK) + (size_t)n + 1) * 4);
}

extern "C" int vx_rle_compress(const uint32_t* runs, const int64_t* offsets, int64_t total_runs, int64_t max_runs, int n, const int32_t* counts, int first, uint8_t* bytes,
                               const int64_t* byte_offsets, int32_t* sizes, void* workspace, size_t workspace_bytes, void* stream) {
    VX_REQUIRE(runs && offsets && workspace && (bytes ? byte_offsets != nullptr : sizes != nullptr),
               "vx_rle_compress: null operand (runs, offsets, workspace; sizes without bytes, byte_offsets with them)");
    VX_REQUIRE(n > 0 && n <= 65535 && first >= 0 && total_runs >= 0 && total_runs <= MAX_TOTAL_RUNS && max_runs >= 0,
               "vx_rle_compress: %d records (1 .. 65535) from %d, %lld runs (0 .. %lld), the longest %lld", n, first, (long long)total_runs, (long long)MAX_TOTAL_RUNS,
               (long long)max_runs);
    VX_REQUIRE(aligned16(workspace) && workspace_bytes >= vx_rle_compress_workspace_bytes(total_runs, n),
               "vx_rle_compress: workspace of %zu bytes (16-byte aligned, at least %zu)", workspace_bytes, vx_rle_compress_workspace_bytes(total_runs, n));
    static_assert(sizeof(long) == sizeof(int64_t), "offsets are read as long");
    hipStream_t s = as_stream(stream);
    const long* off = reinterpret_cast<const long*>(offsets);
    int* ws = static_cast<int*>(workspace);
    const long longest = max_runs < total_runs ? max_runs : total_runs;
    const dim3 grid((unsigned)grid_stride_blocks(longest, MAX_GRID_X, CHUNK), (unsigned)n);
    hipLaunchKernelGGL(rle_compress_kernel<false>, grid, dim3(CT), 0, s, runs, off, (long)total_runs, counts, first, ws, (uint8_t*)nullptr, (const long*)nullptr);
    VX_LAUNCH_CHECK();
    hipLaunchKernelGGL(rle_chunk_prefix_kernel, dim3(blocks_for(n, 4)), dim3(256), 0, s, off, (long)total_runs, n, counts, first, ws, sizes);
    VX_LAUNCH_CHECK();
    if (!bytes) return 1;
    hipLaunchKernelGGL(rle_compress_kernel<true>, grid, dim3(CT), 0, s, runs, off, (long)total_runs, counts, first, ws, bytes, reinterpret_cast<const long*>(byte_offsets));
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_rle_decompress(const uint8_t* bytes, const int64_t* byte_offsets, int n, const int32_t* counts, int first, uint32_t* runs, const int64_t* offsets,
                                 int32_t* sizes, int32_t* status, void* stream) {
    VX_REQUIRE(bytes && byte_offsets && (runs ? offsets != nullptr : sizes != nullptr),
               "vx_rle_decompress: null operand (bytes, byte_offsets; sizes without runs, offsets with them)");
    VX_REQUIRE(n > 0 && n <= 65535 && first >= 0, "vx_rle_decompress: %d records (1 .. 65535) from %d", n, first);
    hipLaunchKernelGGL(rle_decompress_kernel, dim3((unsigned)n), dim3(DT), 0, as_stream(stream), bytes, reinterpret_cast<const long*>(byte_offsets), counts, first, runs,
                       reinterpret_cast<const long*>(offsets), sizes, status);
    VX_LAUNCH_CHECK();
    return 1;
}
