// Polygons to COCO's uncompressed RLE (pycocotools' rleFrPoly), the union / intersection of records and their boxes, on the device. Polygons are a CSR: xy f64
// [total_vertices][2], poly_offsets i64 [n + 1]; records are the encoder's CSR rows (runs u32, offsets i64 [n + 1], alternating from background, p = x * h + y).
//   vx_poly_rle  rleFrPoly as it reads: vertices upsampled by 5 with a truncating cast, every edge walked along its longer axis, a boundary key x * h + y for
//                every walked point that enters a new column at a pixel centre, the keys and h w sorted, equal keys cancelled in pairs, differences = runs.
//     edges      one block per polygon, a lane per edge: both ends upsampled, the edge's slope, an inclusive scan of max(dx, dy) + 1 (cross-lane shifts, the
//                waves' totals through LDS, a carried i64) = the edge's first point index and the polygon's M. 32 bytes an edge go to the workspace.
//     points     a lane per point index j, never stored: the owning edge by a binary search over the edge starts (in LDS up to 1024 edges, in the table
//                beyond), point j a closed form of j - start, point j - 1 the same edge's previous point or the last point of the edge before. A polygon's M
//                points are cut into chunks of 4096; the grid's x blocks of a polygon take contiguous ranges of chunks, so one long outline spreads over
//                blocks and a block's keys are one contiguous piece of the polygon's key row. Pass one counts the kept keys per block, a wave per polygon
//                turns the blocks' counts into offsets and K, one block turns the K + 1 into key rows, pass two writes the keys (ballot + popcount within
//                a wave, the waves' counts through LDS). The order of a row's keys does not matter: they are sorted next.
//     runs       one block of 16 waves per polygon: the keys and h w, padded with ~0 to a power of two, through a bitonic network: in LDS up to 8192 keys,
//                in the key row itself beyond (the same code on a global pointer; slower). Then a round per 1024 sorted keys: group heads by a compare with
//                the neighbour, each key's group head by a max-scan of head indices, so the LAST key of a group knows the group's size; it survives when
//                that is odd, or when it is h w. Survivors are ranked by a sum-scan, the survivor before each by a max-scan of values (they ascend):
//                run = survivor - the one before, stored at its rank below the row's capacity.
//   vx_bits_merge  a lane per output word in the bit-word layout of kernels_rle_decode.hip, OR or AND over the group's members, contiguous stores.
//   vx_rle_bbox  one block per record: the run starts by the scan of rle_positions_kernel (restated; kernels_rle_decode.hip stays as it is), a foreground
//                run cut at h w gives columns p0 / h .. (p1 - 1) / h and rows p0 % h .. (p1 - 1) % h, or every row when it crosses a column end; min / max
//                by a butterfly, the waves' through LDS.
// Doubles only in edges and points, written as the loop writes them and built without contraction (csrc/Makefile); integers elsewhere. No atomics, no scratch;
// the same bytes on every run.
#include "vx_common.h"

namespace {

typedef unsigned long long u64;

constexpr int EW = 4, ET = 64 * EW;     // waves and edges a round of an edges block
constexpr int PW = 4, PT = 64 * PW;     // waves and points a round of a points block
constexpr int CHUNK = 16 * PT;          // points of a chunk
constexpr int STAGE_EDGES = 1024;       // edge starts held in LDS
constexpr int MAX_GRID_X = 1024, DEFAULT_GRID_X = 16;
constexpr int RW = 16, RT = 64 * RW;    // waves and keys a round of a runs block
constexpr int SORT_CAP = 8192;          // keys sorted in LDS (32 KB: two blocks of 16 waves fill a CU's wave slots before its LDS)
constexpr int BW = 4, BT = 64 * BW;     // waves and runs a round of a bbox block
constexpr double COORD_LIMIT = 1048576.0;
constexpr uint32_t PAD_KEY = 0xffffffffu; // above every key: h w is below 2^31

// an edge after the loop's swap: its first end, its points - 1 along the longer axis, bit 0 flip, bit 1 x is the longer axis, the slope, its first point's index
struct edge_rec { int xs, ys, n, flags; double s; long start; };
static_assert(sizeof(edge_rec) == 32, "the workspace is sized by 32 bytes an edge");

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline long segments(int h) { return ((long)h + 63) / 64; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline bool extent_ok(int w, int h) { return w > 0 && h > 0 && (long)w * h < (1L << 31) - 1; }
inline int grid_x_of(int64_t max_points) { return max_points <= 0 ? DEFAULT_GRID_X : grid_stride_blocks(max_points, MAX_GRID_X, CHUNK); }

__host__ __device__ inline long key_row_of(long N) { // entries of a key row of N = K + 1 keys: the sort beyond LDS pads in place
    if (N <= SORT_CAP) return N < 0 ? 0 : N;
    long r = SORT_CAP;
    while (r < N) r <<= 1;
    return r;
}

__device__ __forceinline__ bool skipped(const int* __restrict__ counts, int m) { return counts && m >= counts[0]; }

// polygon m of the CSR: rel = its first vertex behind poly_offsets[0], k vertices; k = -1: no vertex, or outside total_vertices
struct csr_row { long rel, k; };
__device__ __forceinline__ csr_row poly_of(const long* __restrict__ poly_offsets, int m, long total_vertices) {
    const long rel = poly_offsets[m] - poly_offsets[0], k = poly_offsets[m + 1] - poly_offsets[m];
    const bool ok = rel >= 0 && k >= 1 && rel <= total_vertices && k <= total_vertices - rel;
    return {ok ? rel : 0, ok ? k : -1};
}

__device__ __forceinline__ int upsample(double c) { return (int)(5.0 * c + 0.5); }

// one block per polygon
__global__ __launch_bounds__(ET) void poly_edges_kernel(const double* __restrict__ xy, const long* __restrict__ poly_offsets, long total_vertices, const int* __restrict__ counts,
                                                        int first, edge_rec* __restrict__ edges, long* __restrict__ points, int* __restrict__ st_ws, int* __restrict__ status) {
    __shared__ long wave_sum[EW];
    const int m = blockIdx.x;
    if (skipped(counts, first + m)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const csr_row row = poly_of(poly_offsets, m, total_vertices);
    if (row.k < 0) {
        if (tid == 0) {
            points[m] = 0;
            st_ws[m] = 1;
            if (status) status[m] = 1;
        }
        return;
    }
    const double* src = xy + 2 * poly_offsets[m];
    edge_rec* out = edges + row.rel;
    long carry = 0;
    int bad = 0;
    for (long base = 0; base < row.k; base += ET) {
        const long j = base + tid;
        const bool live = j < row.k;
        edge_rec e = {0, 0, 0, 0, 0.0, 0};
        long cnt = 0;
        if (live) {
            const long j1 = j + 1 < row.k ? j + 1 : 0;
            const double X0 = src[2 * j], Y0 = src[2 * j + 1], X1 = src[2 * j1], Y1 = src[2 * j1 + 1];
            const bool fine = fabs(X0) <= COORD_LIMIT && fabs(Y0) <= COORD_LIMIT && fabs(X1) <= COORD_LIMIT && fabs(Y1) <= COORD_LIMIT; // false for a NaN
            cnt = 1;
            if (!fine) {
                bad = 1;
            } else {
                int xs = upsample(X0), ys = upsample(Y0), xe = upsample(X1), ye = upsample(Y1);
                const int dx = abs(xe - xs), dy = abs(ys - ye);
                const bool xmajor = dx >= dy, flip = xmajor ? xs > xe : ys > ye;
                if (flip) {
                    int t = xs; xs = xe; xe = t;
                    t = ys; ys = ye; ye = t;
                }
                e.xs = xs;
                e.ys = ys;
                e.n = xmajor ? dx : dy;
                e.flags = (flip ? 1 : 0) | (xmajor ? 2 : 0);
                e.s = e.n == 0 ? 0.0 : xmajor ? (double)(ye - ys) / dx : (double)(xe - xs) / dy;
                cnt = (long)e.n + 1;
            }
        }
        long incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        long before = 0, round_total = 0;
#pragma unroll
        for (int u = 0; u < EW; ++u) {
            const long t = wave_sum[u];
            if (u < wave) before += t;
            round_total += t;
        }
        __syncthreads();
        if (live) {
            e.start = carry + before + incl - cnt;
            out[j] = e;
        }
        carry += round_total;
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) {
        const int st = bad ? 2 : carry >= (1L << 31) ? 3 : 0;
        points[m] = st ? 0 : carry;
        st_ws[m] = st;
        if (status) status[m] = st;
    }
}

// point d of an edge; a single-point edge has no slope and is its first end
__device__ __forceinline__ void point_of(const edge_rec& e, int d, int& u, int& v) {
    const int t = (e.flags & 1) ? e.n - d : d;
    if (e.n == 0) {
        u = e.xs;
        v = e.ys;
    } else if (e.flags & 2) {
        u = t + e.xs;
        v = (int)(e.ys + e.s * t + 0.5);
    } else {
        v = t + e.ys;
        u = (int)(e.xs + e.s * t + 0.5);
    }
}

// the loop's step 3 on point (u, v) behind point (pu, pv)
__device__ __forceinline__ bool boundary_key(int u, int v, int pu, int pv, int w, int h, uint32_t& key) {
    if (u == pu) return false;
    double xd = (double)(u < pu ? u : u - 1);
    xd = (xd + 0.5) / 5.0 - 0.5;
    if (floor(xd) != xd || xd < 0 || xd > w - 1) return false;
    double yd = (double)(v < pv ? v : pv);
    yd = (yd + 0.5) / 5.0 - 0.5;
    if (yd < 0) yd = 0;
    else if (yd > h) yd = h;
    yd = ceil(yd);
    key = (uint32_t)((int)xd * h + (int)yd);
    return true;
}

// grid (blocks of a polygon, polygons). WRITE = false: the block's kept keys -> partial[m][block]. WRITE = true: partial holds the keys of the blocks before.
template <bool WRITE>
__global__ __launch_bounds__(PT) void poly_points_kernel(const long* __restrict__ poly_offsets, long total_vertices, const int* __restrict__ counts, int first,
                                                         const edge_rec* __restrict__ edges, const long* __restrict__ points, const int* __restrict__ st_ws, int w, int h,
                                                         int* __restrict__ partial, const long* __restrict__ key_off, uint32_t* __restrict__ keys, long total_keys) {
    __shared__ int starts[STAGE_EDGES];
    __shared__ int wave_cnt[PW];
    const int m = blockIdx.y;
    if (skipped(counts, first + m) || st_ws[m]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long M = points[m], n_chunks = (M + CHUNK - 1) / CHUNK, per = (n_chunks + gridDim.x - 1) / gridDim.x;
    const long c0 = min(n_chunks, (long)blockIdx.x * per), c1 = min(n_chunks, c0 + per);
    int* slot = partial + (long)m * gridDim.x + blockIdx.x;
    if (c0 >= c1) {
        if (!WRITE && tid == 0) *slot = 0;
        return;
    }
    const csr_row row = poly_of(poly_offsets, m, total_vertices); // st_ws[m] == 0: k >= 1
    const edge_rec* E = edges + row.rel;
    const bool staged = row.k <= STAGE_EDGES;
    if (staged) {
        for (int i = tid; i < row.k; i += PT) starts[i] = (int)E[i].start; // M is below 2^31
        __syncthreads();
    }
    long at = 0, row_end = 0;
    if (WRITE) {
        at = key_off[m] + *slot;
        row_end = min(key_off[m + 1], total_keys);
    }
    const long j_end = min(M, c1 * CHUNK);
    int mine = 0;
    for (long base = c0 * CHUNK; base < j_end; base += PT) {
        const long j = base + tid;
        bool keep = false;
        uint32_t key = 0;
        if (j >= 1 && j < j_end) {
            long lo = 0, hi = row.k - 1; // the last edge that starts at or before j
            while (lo < hi) {
                const long mid = (lo + hi + 1) >> 1;
                const long s = staged ? (long)starts[mid] : E[mid].start;
                if (s <= j) lo = mid;
                else hi = mid - 1;
            }
            const edge_rec e = E[lo];
            const int d = (int)(j - e.start);
            int u, v, pu, pv;
            point_of(e, d, u, v);
            if (d > 0) {
                point_of(e, d - 1, pu, pv);
            } else { // j >= 1: an edge lies before this one
                const edge_rec p = E[lo - 1];
                point_of(p, p.n, pu, pv);
            }
            keep = boundary_key(u, v, pu, pv, w, h, key);
        }
        if (!WRITE) {
            mine += keep;
            continue;
        }
        const u64 ballot = __ballot(keep);
        if (lane == 0) wave_cnt[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, round_total = 0;
#pragma unroll
        for (int u = 0; u < PW; ++u) {
            const int t = wave_cnt[u];
            if (u < wave) before += t;
            round_total += t;
        }
        if (keep) {
            const long p = at + before + __popcll(ballot & (((u64)1 << lane) - 1));
            if (p < row_end) keys[p] = key;
        }
        at += round_total;
        __syncthreads();
    }
    if (!WRITE) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
        if (lane == 0) wave_cnt[wave] = mine;
        __syncthreads();
        if (tid == 0) {
            int total = 0;
#pragma unroll
            for (int u = 0; u < PW; ++u) total += wave_cnt[u];
            *slot = total;
        }
    }
}

// a wave per polygon, four a block: the blocks' counts -> the keys of the blocks before each, in place; K; mk = {M, K + 1}, {0, 0} for a refused polygon
__global__ __launch_bounds__(256) void poly_block_prefix_kernel(int n, int grid_x, const int* __restrict__ counts, int first, const long* __restrict__ points,
                                                                const int* __restrict__ st_ws, int* __restrict__ partial, int* __restrict__ n_keys, long* __restrict__ mk) {
    const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= n || skipped(counts, first + m)) return;
    long carry = 0;
    if (!st_ws[m]) {
        int* ws = partial + (long)m * grid_x;
        for (int base = 0; base < grid_x; base += 64) {
            const int c = base + lane;
            const int v = c < grid_x ? ws[c] : 0;
            long incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const long t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            if (c < grid_x) ws[c] = (int)(carry + incl - v);
            carry += __shfl(incl, 63);
        }
    }
    if (lane == 0) {
        n_keys[m] = (int)carry; // at most M - 1
        if (mk) {
            mk[2 * m] = points[m];
            mk[2 * m + 1] = st_ws[m] ? 0 : carry + 1;
        }
    }
}

// one block: the key rows' sizes -> key_off [n + 1]; a row that does not fit into total_keys gets status 4
__global__ __launch_bounds__(RT) void poly_key_rows_kernel(int n, const int* __restrict__ counts, int first, const int* __restrict__ n_keys, int* __restrict__ st_ws,
                                                           int* __restrict__ status, long total_keys, long* __restrict__ key_off) {
    __shared__ long wave_sum[RW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long carry = 0;
    for (int base = 0; base < n; base += RT) {
        const int m = base + tid;
        const bool live = m < n && !skipped(counts, first + m) && !st_ws[m];
        const long v = live ? key_row_of((long)n_keys[m] + 1) : 0;
        long incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        long before = 0, round_total = 0;
#pragma unroll
        for (int u = 0; u < RW; ++u) {
            const long t = wave_sum[u];
            if (u < wave) before += t;
            round_total += t;
        }
        __syncthreads();
        const long end = carry + before + incl;
        if (m < n) key_off[m] = end - v;
        if (live && end > total_keys) {
            st_ws[m] = 4;
            if (status) status[m] = 4;
        }
        carry += round_total;
    }
    if (tid == 0) key_off[n] = carry;
}

// the network on n2 keys (a power of two, at least 64) in LDS or in global memory, all RT threads
template <class Keys>
__device__ __forceinline__ void bitonic_sort(Keys s, long n2, int tid) {
    for (long k = 2; k <= n2; k <<= 1) {
        for (long j = k >> 1; j > 0; j >>= 1) {
            for (long t = tid; t < n2 / 2; t += RT) {
                const long i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint32_t a = s[i], b = s[l];
                if ((a > b) == !(i & k)) {
                    s[i] = b;
                    s[l] = a;
                }
            }
            __syncthreads();
        }
    }
}

// N sorted keys -> the runs of their odd groups (and of h w's), at most cap of them to dst; returns their number
template <class Keys>
__device__ __forceinline__ long emit_runs(Keys s, long N, uint32_t hw, uint32_t* __restrict__ dst, long cap, int tid, long* wave_a, long* wave_b, uint32_t* wave_c) {
    const int lane = tid & 63, wave = tid >> 6;
    long head_carry = -1, rank_carry = 0; // the last group head's index, the survivors, the last survivor's key: of the rounds before
    uint32_t prev_carry = 0;
    for (long base = 0; base < N; base += RT) {
        const long i = base + tid;
        const bool live = i < N;
        const uint32_t key = live ? s[i] : PAD_KEY;
        const bool head = live && (i == 0 || s[i - 1] != key), last = live && (i == N - 1 || s[i + 1] != key);
        long hidx = head ? i : -1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long t = __shfl_up(hidx, d);
            if (lane >= d) hidx = max(hidx, t);
        }
        if (lane == 63) wave_a[wave] = hidx;
        __syncthreads();
        long round_head = head_carry;
#pragma unroll
        for (int u = 0; u < RW; ++u) {
            const long t = wave_a[u];
            if (u < wave) hidx = max(hidx, t);
            round_head = max(round_head, t);
        }
        hidx = max(hidx, head_carry);
        const bool survive = last && (((i - hidx + 1) & 1) || key == hw);
        long rank = survive ? 1 : 0;
        uint32_t top = survive ? key : 0u; // the largest surviving key up to this lane
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long t = __shfl_up(rank, d);
            const uint32_t v = __shfl_up(top, d);
            if (lane >= d) {
                rank += t;
                top = max(top, v);
            }
        }
        uint32_t below = __shfl_up(top, 1); // ... below this lane
        if (lane == 0) below = 0u;
        if (lane == 63) {
            wave_b[wave] = rank;
            wave_c[wave] = top;
        }
        __syncthreads();
        long before = 0, round_total = 0;
        uint32_t round_top = prev_carry;
#pragma unroll
        for (int u = 0; u < RW; ++u) {
            const long t = wave_b[u];
            const uint32_t v = wave_c[u];
            if (u < wave) {
                before += t;
                below = max(below, v);
            }
            round_total += t;
            round_top = max(round_top, v);
        }
        below = max(below, prev_carry);
        if (survive) {
            const long q = rank_carry + before + rank - 1;
            if (dst && q < cap) dst[q] = key - below;
        }
        head_carry = round_head;
        rank_carry += round_total;
        prev_carry = round_top;
        __syncthreads(); // the waves' slots are free again
    }
    return rank_carry;
}

// one block per polygon
__global__ __launch_bounds__(RT) void poly_runs_kernel(const int* __restrict__ counts, int first, const int* __restrict__ n_keys, const int* __restrict__ st_ws,
                                                       const long* __restrict__ key_off, uint32_t* __restrict__ keys, int w, int h, uint32_t* __restrict__ runs,
                                                       const long* __restrict__ offsets, int* __restrict__ sizes) {
    __shared__ uint32_t lds_keys[SORT_CAP];
    __shared__ long wave_a[RW], wave_b[RW];
    __shared__ uint32_t wave_c[RW];
    const int m = blockIdx.x, tid = threadIdx.x;
    if (skipped(counts, first + m)) return;
    if (st_ws[m]) {
        if (tid == 0 && sizes) sizes[m] = 0;
        return;
    }
    const long N = (long)n_keys[m] + 1;
    const uint32_t hw = (uint32_t)((long)w * h);
    uint32_t* row = keys + key_off[m];
    long n2 = 64;
    while (n2 < N) n2 <<= 1;
    long cap = 0;
    uint32_t* dst = nullptr;
    if (runs) {
        cap = offsets[m + 1] - offsets[m];
        dst = runs + offsets[m];
    }
    long total;
    if (n2 <= SORT_CAP) {
        for (long i = tid; i < n2; i += RT) lds_keys[i] = i < N - 1 ? row[i] : i == N - 1 ? hw : PAD_KEY;
        __syncthreads();
        bitonic_sort(lds_keys, n2, tid);
        total = emit_runs(lds_keys, N, hw, dst, cap, tid, wave_a, wave_b, wave_c);
    } else { // the row has n2 entries (key_row_of)
        for (long i = N - 1 + tid; i < n2; i += RT) row[i] = i == N - 1 ? hw : PAD_KEY;
        __syncthreads();
        bitonic_sort(row, n2, tid);
        total = emit_runs(row, N, hw, dst, cap, tid, wave_a, wave_b, wave_c);
    }
    if (tid == 0 && sizes) sizes[m] = (int)min(total, 0x7fffffffL);
}

// grid (256 words, groups): word i of group g = the OR / AND of word i of its members; an empty group, and a member outside 0 .. n - 1, give nothing
__global__ __launch_bounds__(256) void bits_merge_kernel(const u64* __restrict__ words, int n, const long* __restrict__ group_offsets, long nw, long words_per_mask,
                                                         int intersect, u64* __restrict__ out) {
    const int g = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nw) return;
    const long b0 = max(0L, group_offsets[g]), b1 = min((long)n, group_offsets[g + 1]);
    u64 acc = (intersect && b0 < b1) ? ~0ull : 0ull;
    for (long b = b0; b < b1; ++b) {
        const u64 v = words[b * words_per_mask + i];
        acc = intersect ? acc & v : acc | v;
    }
    out[g * words_per_mask + i] = acc;
}

// one block per record
__global__ __launch_bounds__(BT) void rle_bbox_kernel(const uint32_t* __restrict__ runs, const long* __restrict__ offsets, long total_runs, int w, int h,
                                                      const int* __restrict__ counts, int first, int* __restrict__ boxes) {
    __shared__ long wave_sum[BW];
    __shared__ int wave_box[BW][4];
    const int m = blockIdx.x;
    if (skipped(counts, first + m)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long rel = offsets[m] - offsets[0], Rr = offsets[m + 1] - offsets[m];
    const bool ok = rel >= 0 && Rr >= 0 && rel <= total_runs && Rr <= total_runs - rel;
    const long R = ok ? Rr : 0, hw = (long)w * h;
    const uint32_t* src = runs + offsets[m];
    int x0 = w, y0 = h, x1 = -1, y1 = -1;
    long carry = 0;
    for (long base = 0; base < R; base += BT) {
        const long i = base + tid;
        const long v = i < R ? (long)src[i] : 0;
        long incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        long before = 0, round_total = 0;
#pragma unroll
        for (int u = 0; u < BW; ++u) {
            const long t = wave_sum[u];
            if (u < wave) before += t;
            round_total += t;
        }
        __syncthreads();
        const long end = carry + before + incl, start = end - v;
        const long p0 = min(start, hw), p1 = min(end, hw);
        if ((i & 1) && p0 < p1) { // v is 0 behind R
            const int c0 = (int)(p0 / h), c1 = (int)((p1 - 1) / h);
            x0 = min(x0, c0);
            x1 = max(x1, c1);
            y0 = min(y0, c0 == c1 ? (int)(p0 % h) : 0);
            y1 = max(y1, c0 == c1 ? (int)((p1 - 1) % h) : h - 1);
        }
        carry += round_total;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        x0 = min(x0, __shfl_xor(x0, d));
        y0 = min(y0, __shfl_xor(y0, d));
        x1 = max(x1, __shfl_xor(x1, d));
        y1 = max(y1, __shfl_xor(y1, d));
    }
    if (lane == 0) {
        wave_box[wave][0] = x0;
        wave_box[wave][1] = y0;
        wave_box[wave][2] = x1;
        wave_box[wave][3] = y1;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int u = 1; u < BW; ++u) {
            x0 = min(x0, wave_box[u][0]);
            y0 = min(y0, wave_box[u][1]);
            x1 = max(x1, wave_box[u][2]);
            y1 = max(y1, wave_box[u][3]);
        }
        int* out = boxes + 4 * (long)m;
        const bool any = x1 >= 0;
        out[0] = any ? x0 : 0;
        out[1] = any ? y0 : 0;
        out[2] = any ? x1 - x0 + 1 : 0;
        out[3] = any ? y1 - y0 + 1 : 0;
    }
}

// the workspace of vx_poly_rle: edges, M i64 [n], K i32 [n], status i32 [n], the blocks' counts i32 [n][grid_x], key_off i64 [n + 1]
struct poly_ws {
    size_t edges, points, n_keys, st, partial, key_off, total;
    poly_ws(int64_t total_vertices, int n, int grid_x) {
        size_t at = 0;
        auto take = [&](size_t bytes) {
            const size_t o = at;
            at += up256(bytes);
            return o;
        };
        edges = take((size_t)total_vertices * sizeof(edge_rec));
        points = take((size_t)n * 8);
        n_keys = take((size_t)n * 4);
        st = take((size_t)n * 4);
        partial = take((size_t)n * grid_x * 4);
        key_off = take(((size_t)n + 1) * 8);
        total = at;
    }
};

} // namespace

extern "C" int64_t vx_poly_rle_key_row(int64_t keys) { return key_row_of(keys); }

extern "C" size_t vx_poly_rle_workspace_bytes(int64_t total_vertices, int n, int64_t max_points) {
    if (total_vertices < 1 || total_vertices > (int64_t(1) << 40) || n < 1 || n > 65535) return 0;
    return poly_ws(total_vertices, n, grid_x_of(max_points)).total;
}

extern "C" int vx_poly_rle(const double* xy, const int64_t* poly_offsets, int64_t total_vertices, int64_t max_points, int n, int w, int h, const int32_t* counts, int first,
                           uint32_t* keys, int64_t total_keys, uint32_t* runs, const int64_t* offsets, int32_t* sizes, int64_t* mk, int32_t* status, void* workspace,
                           size_t workspace_bytes, void* stream) {
    VX_REQUIRE(xy && poly_offsets && workspace && (keys ? (runs ? offsets != nullptr : sizes != nullptr) : mk != nullptr),
               "vx_poly_rle: null operand (xy, poly_offsets, workspace; mk without keys; with keys sizes without runs, offsets with them)");
    VX_REQUIRE(extent_ok(w, h), "vx_poly_rle: extent %d x %d (w, h >= 1, w * h below 2^31 - 1)", w, h);
    VX_REQUIRE(n > 0 && n <= 65535 && first >= 0 && total_vertices >= 1 && total_keys >= 0, "vx_poly_rle: %d polygons (1 .. 65535) from %d, %lld vertices, %lld keys", n, first,
               (long long)total_vertices, (long long)total_keys);
    VX_REQUIRE(aligned16(workspace) && aligned8(xy) && workspace_bytes >= vx_poly_rle_workspace_bytes(total_vertices, n, max_points) && workspace_bytes > 0,
               "vx_poly_rle: workspace of %zu bytes (16-byte aligned, at least %zu)", workspace_bytes, vx_poly_rle_workspace_bytes(total_vertices, n, max_points));
    static_assert(sizeof(long) == sizeof(int64_t), "offsets are read as long");
    hipStream_t s = as_stream(stream);
    const int grid_x = grid_x_of(max_points);
    const poly_ws lay(total_vertices, n, grid_x);
    uint8_t* base = static_cast<uint8_t*>(workspace);
    edge_rec* edges = reinterpret_cast<edge_rec*>(base + lay.edges);
    long* points = reinterpret_cast<long*>(base + lay.points);
    int* n_keys = reinterpret_cast<int*>(base + lay.n_keys);
    int* st_ws = reinterpret_cast<int*>(base + lay.st);
    int* partial = reinterpret_cast<int*>(base + lay.partial);
    long* key_off = reinterpret_cast<long*>(base + lay.key_off);
    const long* poff = reinterpret_cast<const long*>(poly_offsets);
    const dim3 grid((unsigned)grid_x, (unsigned)n);
    hipLaunchKernelGGL(poly_edges_kernel, dim3((unsigned)n), dim3(ET), 0, s, xy, poff, (long)total_vertices, counts, first, edges, points, st_ws, status);
    VX_LAUNCH_CHECK();
    hipLaunchKernelGGL(poly_points_kernel<false>, grid, dim3(PT), 0, s, poff, (long)total_vertices, counts, first, edges, points, st_ws, w, h, partial, (const long*)nullptr,
                       (uint32_t*)nullptr, 0L);
    VX_LAUNCH_CHECK();
    hipLaunchKernelGGL(poly_block_prefix_kernel, dim3(blocks_for(n, 4)), dim3(256), 0, s, n, grid_x, counts, first, points, st_ws, partial, n_keys, reinterpret_cast<long*>(mk));
    VX_LAUNCH_CHECK();
    if (!keys) return 1;
    hipLaunchKernelGGL(poly_key_rows_kernel, dim3(1), dim3(RT), 0, s, n, counts, first, n_keys, st_ws, status, (long)total_keys, key_off);
    VX_LAUNCH_CHECK();
    hipLaunchKernelGGL(poly_points_kernel<true>, grid, dim3(PT), 0, s, poff, (long)total_vertices, counts, first, edges, points, st_ws, w, h, partial, key_off, keys,
                       (long)total_keys);
    VX_LAUNCH_CHECK();
    hipLaunchKernelGGL(poly_runs_kernel, dim3((unsigned)n), dim3(RT), 0, s, counts, first, n_keys, st_ws, key_off, keys, w, h, runs, reinterpret_cast<const long*>(offsets), sizes);
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_bits_merge(const void* words, int n, const int64_t* group_offsets, int groups, int w, int h, int intersect, void* out_words, void* stream) {
    VX_REQUIRE(words && group_offsets && out_words && aligned8(words) && aligned8(out_words), "vx_bits_merge: null operand, or words not 8-byte aligned");
    VX_REQUIRE(extent_ok(w, h), "vx_bits_merge: extent %d x %d (w, h >= 1, w * h below 2^31 - 1)", w, h);
    VX_REQUIRE(n > 0 && n <= 65535 && groups > 0 && groups <= 65535, "vx_bits_merge: %d masks in %d groups (1 .. 65535 each)", n, groups);
    const long nw = (long)w * segments(h), wpm = (long)(vx_mask_rle_workspace_bytes(w, h, 1) / 8);
    hipLaunchKernelGGL(bits_merge_kernel, dim3(blocks_for(nw), (unsigned)groups), dim3(256), 0, as_stream(stream), static_cast<const u64*>(words), n,
                       reinterpret_cast<const long*>(group_offsets), nw, wpm, intersect, static_cast<u64*>(out_words));
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_rle_bbox(const uint32_t* runs, const int64_t* offsets, int64_t total_runs, int n, int w, int h, const int32_t* counts, int first, int32_t* boxes, void* stream) {
    VX_REQUIRE(runs && offsets && boxes, "vx_rle_bbox: null operand");
    VX_REQUIRE(extent_ok(w, h), "vx_rle_bbox: extent %d x %d (w, h >= 1, w * h below 2^31 - 1)", w, h);
    VX_REQUIRE(n > 0 && n <= 65535 && first >= 0 && total_runs >= 0, "vx_rle_bbox: %d records (1 .. 65535) from %d, %lld runs", n, first, (long long)total_runs);
    hipLaunchKernelGGL(rle_bbox_kernel, dim3((unsigned)n), dim3(BT), 0, as_stream(stream), runs, reinterpret_cast<const long*>(offsets), (long)total_runs, w, h, counts, first,
                       boxes);
    VX_LAUNCH_CHECK();
    return 1;
}
