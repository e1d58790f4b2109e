// image_scale (image_resize.cpp: stb_image_resize v0.97 as the reference calls it) on the device: both passes in one launch, for a batch of images of one
// extent and format, with the bits of the host function.
//
// Work split. A block owns TW x TH outputs of one image. Its 64 x ch threads are (column, channel) with the channel as the fast index, so thread t
// stores element t of a tile row: consecutive addresses. A thread keeps TH vertical accumulators in registers and never sees another thread's
// arithmetic, except the alpha of its own pixel at the very end.
//
// Data movement. The block walks the source rows of its band -- the union of its rows' vertical taps, UNCLAMPED, so a row past the edge is its
// clamped neighbour once more, exactly as often and in the same place of the sum as on the host -- in ascending order. A row's span (the columns the
// tile's horizontal taps reach, clamped column by column) is staged in LDS decoded: table lookup, alpha + 2^-80, premultiplied. Two buffers: row
// v + 1 is loaded and decoded into the other one while row v is filtered, one barrier per row. Every thread filters its column from LDS in
// ascending tap order (zero weights inside a tap run included: they are in the table), then adds h * wy into the accumulators of the output rows
// whose taps hold this source row; the test is uniform over the block, so it is a scalar branch. The per-tile tables (horizontal weights tap-major,
// vertical weights, the u8 lookup tables) are copied into LDS once per block.
//
// Arithmetic. f32, every product and every sum rounded on its own (contraction off for the whole file; the packed f32 VALU forms are disabled for
// this object in the Makefile), accumulators start at zero, divisions are IEEE (hipcc's default). No scratch, no atomics, nothing of one image
// reaches another: the bits do not depend on the batch or on the tile width.
#include "vx_common.h"

#include "image_scale_tables.h"

#pragma clang fp contract(off)

namespace {

using namespace visp_scale;

struct scale_args {
    const void* src;
    void* dst;
    const uint32_t* tables;
    table_layout lay;
    int B, h, w, oh, ow;
    int ac;                          // alpha channel, -1 without one
    int tile_w, taps_x, taps_y, span; // span: words of a row buffer / ch
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// image_resize.cpp's linear_to_srgb_u8 with its table in LDS
__device__ __forceinline__ uint8_t encode_srgb(float in, const uint32_t* tab) {
    const uint32_t min_u = (127u - 13u) << 23;
    const float min_f = __uint_as_float(min_u), almost_one = __uint_as_float(0x3f7fffffu);
    if (!(in > min_f)) in = min_f;
    if (in > almost_one) in = almost_one;
    const uint32_t u = __float_as_uint(in);
    const uint32_t t = tab[(u - min_u) >> 20];
    const uint32_t bias = (t >> 16) << 9, scale = t & 0xffff;
    return (uint8_t)((bias + scale * ((u >> 12) & 0xff)) >> 16);
}
// round half up of the clamped value, with std::max's and std::min's choice of operand
__device__ __forceinline__ uint8_t encode_alpha(float p) {
    const float lo = p < 0.0f ? 0.0f : p, v = 1.0f < lo ? 1.0f : lo;
    return (uint8_t)(int)(v * 255.0f + 0.5f);
}

// one source pixel, decoded as image_scale's first loop does, into ch words of LDS
template <int CH, bool F32>
__device__ __forceinline__ void decode_pixel(const void* row, int sx, int ac, const float* lut_srgb, const float* lut_alpha, float* out) {
    float p[CH];
    if constexpr (F32) {
        if constexpr (CH == 4) {
            const f32x4 v = static_cast<const f32x4*>(row)[sx];
#pragma unroll
            for (int c = 0; c < 4; ++c) p[c] = v[c];
        } else {
            const float* s = static_cast<const float*>(row) + (long)sx * CH;
#pragma unroll
            for (int c = 0; c < CH; ++c) p[c] = s[c];
        }
        if (CH > 1 && ac >= 0) {
            const float a = p[CH - 1]; // rgba_f32: the only float format with colour and alpha
#pragma unroll
            for (int c = 0; c < CH - 1; ++c) p[c] = p[c] * a;
        }
    } else {
        uint8_t u[CH];
        if constexpr (CH == 4) {
            const uint32_t v = static_cast<const uint32_t*>(row)[sx];
#pragma unroll
            for (int c = 0; c < CH; ++c) u[c] = (uint8_t)(v >> (8 * c));
        } else {
            const uint8_t* s = static_cast<const uint8_t*>(row) + (long)sx * CH;
#pragma unroll
            for (int c = 0; c < CH; ++c) u[c] = s[c];
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) p[c] = c == ac ? lut_alpha[u[c]] : lut_srgb[u[c]];
        if (ac >= 0) {
            const float a = (ac == 0 ? p[0] : p[CH - 1]) + 0x1p-80f;
#pragma unroll
            for (int c = 0; c < CH; ++c) p[c] = c == ac ? a : p[c] * a;
        }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) out[c] = p[c];
}

template <int CH, bool F32>
__global__ __launch_bounds__(64 * CH) void image_scale_kernel(const scale_args a) {
    extern __shared__ float lds[];
    constexpr int NT = 64 * CH;
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % a.lay.tiles_x, ty = (blockIdx.x / a.lay.tiles_x) % a.lay.tiles_y;
    const long b = blockIdx.x / (a.lay.tiles_x * a.lay.tiles_y);
    const int x0 = tx * a.tile_w, y0 = ty * TH;
    const int col = tid / CH, c = tid - col * CH;
    const bool live = col < a.tile_w && x0 + col < a.ow;
    const int TWE = a.tile_w, NX = a.taps_x, NY = a.taps_y;

    // the block's LDS, in lds_words' order
    const float* lut_srgb = lds;
    const float* lut_alpha = lds + 256;
    const uint32_t* lut_enc = reinterpret_cast<const uint32_t*>(lds + 512);
    float* at = lds + (F32 ? 0 : LUT_WORDS);
    int* ymeta = reinterpret_cast<int*>(at);
    float* ytab = at + 2 * TH;
    float* xtab = ytab + TH * NY;
    float* alpha_of = xtab + NX * TWE;
    float* buf = alpha_of + TH * TWE; // two of span * CH words

    const uint32_t* T = a.tables;
    if (!F32)
        for (int i = tid; i < LUT_WORDS; i += NT) reinterpret_cast<uint32_t*>(lds)[i] = T[i];
    for (int i = tid; i < TH; i += NT) {
        const bool in = y0 + i < a.oh;
        ymeta[i] = in ? (int)T[a.lay.yfirst + y0 + i] : 0;
        ymeta[TH + i] = in ? min((int)T[a.lay.ycount + y0 + i], NY) : 0;
    }
    for (int r = 0; r < TH; ++r) {
        const bool in = y0 + r < a.oh;
        const uint32_t* g = T + a.lay.yw + (size_t)(in ? y0 + r : 0) * NY;
        for (int i = tid; i < NY; i += NT) ytab[r * NY + i] = in ? __uint_as_float(g[i]) : 0.0f;
    }
    {
        const uint32_t* g = T + a.lay.xw + (size_t)tx * NX * TWE;
        for (int i = tid; i < NX * TWE; i += NT) xtab[i] = __uint_as_float(g[i]);
    }
    // (tables that do not fit the launch's sizes filter nothing: no index below leaves the block's LDS)
    const int xlo = (int)T[a.lay.tile_xlo + tx], span = min((int)T[a.lay.tile_span + tx], a.span);
    const int vlo = (int)T[a.lay.band_lo + ty], nv = (int)T[a.lay.band_n + ty];
    const int off = live ? (int)T[a.lay.xfirst + x0 + col] - xlo : 0;
    const int n_taps = live ? (int)T[a.lay.xcount + x0 + col] : 0;
    const int cnt = off >= 0 && n_taps <= NX && off + n_taps <= span ? n_taps : 0;

    const size_t px = F32 ? 4 * CH : CH; // bytes of a pixel
    const uint8_t* image = static_cast<const uint8_t*>(a.src) + (size_t)b * a.h * a.w * px;
    auto stage = [&](float* dstbuf, int v) {
        const uint8_t* row = image + (size_t)clampi(v, a.h - 1) * a.w * px;
        for (int j = tid; j < span; j += NT) decode_pixel<CH, F32>(row, clampi(xlo + j, a.w - 1), a.ac, lut_srgb, lut_alpha, dstbuf + j * CH);
    };

    __syncthreads(); // the lookup tables are read by the first stage
    stage(buf, vlo);
    __syncthreads();
    int yf[TH], yc[TH];
    float acc[TH];
#pragma unroll
    for (int r = 0; r < TH; ++r) {
        yf[r] = ymeta[r];
        yc[r] = ymeta[TH + r];
        acc[r] = 0.0f;
    }
    const int bufw = a.span * CH;
    for (int k = 0; k < nv; ++k) {
        const float* cur = buf + (k & 1) * bufw;
        if (k + 1 < nv) stage(buf + ((k + 1) & 1) * bufw, vlo + k + 1);
        float hval = 0.0f;
        const float* p = cur + off * CH + c;
        const float* wx = xtab + col;
        for (int i = 0; i < cnt; ++i) hval = hval + p[i * CH] * wx[i * TWE];
        const int v = vlo + k;
#pragma unroll
        for (int r = 0; r < TH; ++r) {
            const int i = v - yf[r];
            if (i >= 0 && i < yc[r]) acc[r] = acc[r] + hval * ytab[r * NY + i];
        }
        __syncthreads();
    }

    const bool unpremultiply = CH > 1 && a.ac >= 0;
    if (unpremultiply) {
        if (live && c == a.ac) {
#pragma unroll
            for (int r = 0; r < TH; ++r) alpha_of[r * TWE + col] = acc[r];
        }
        __syncthreads();
    }
    if (!live) return;
#pragma unroll
    for (int r = 0; r < TH; ++r) {
        if (y0 + r >= a.oh) break;
        float p = acc[r];
        if (unpremultiply && c != a.ac) {
            const float al = alpha_of[r * TWE + col], ra = al != 0.0f ? 1.0f / al : 0.0f;
            p = p * ra;
        }
        const size_t o = ((((size_t)b * a.oh + y0 + r) * a.ow) + x0 + col) * CH + c;
        if (F32) static_cast<float*>(a.dst)[o] = p;
        else static_cast<uint8_t*>(a.dst)[o] = c == a.ac ? encode_alpha(p) : encode_srgb(p, lut_enc);
    }
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + nb && pb < pa + na;
}

template <int CH, bool F32>
void launch(const scale_args& a, size_t lds_bytes, hipStream_t st) {
    const unsigned blocks = (unsigned)((long)a.B * a.lay.tiles_x * a.lay.tiles_y);
    hipLaunchKernelGGL((image_scale_kernel<CH, F32>), dim3(blocks), dim3(64 * CH), lds_bytes, st, a);
}

} // namespace

extern "C" int vx_image_scale(const void* src, int format, int B, int h, int w, void* dst, int oh, int ow, const void* tables, size_t table_bytes, int tile_w, int taps_x,
                              int taps_y, int span, void* stream) {
    const char* who = "vx_image_scale";
    VX_REQUIRE(src && dst && tables, "%s: null pointer", who);
    VX_REQUIRE(format >= 0 && format <= 7, "%s: image format %d", who, format);
    // visp_image_format: rgba_u8, bgra_u8, argb_u8, rgb_u8, alpha_u8, rgba_f32, rgb_f32, alpha_f32
    static const int channels[8] = {4, 4, 4, 3, 1, 4, 3, 1}, alpha[8] = {3, 3, 0, -1, 0, 3, -1, 0};
    const int ch = channels[format], f32 = format >= 5;
    VX_REQUIRE(B > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "%s: batch %d, %dx%d to %dx%d must be positive", who, B, w, h, ow, oh);
    VX_REQUIRE((int64_t)h * w * ch < (1LL << 31) && (int64_t)oh * ow * ch < (1LL << 31), "%s: an image of %dx%d or %dx%d passes 32-bit indexing", who, w, h, ow, oh);
    VX_REQUIRE(tile_w >= 1 && tile_w <= TW && taps_x >= 1 && taps_x <= MAX_TAPS && taps_y >= 1 && taps_y <= MAX_TAPS && span >= 1,
               "%s: tile of %d columns, %d x %d taps, span %d (at most %d columns and %d taps)", who, tile_w, taps_x, taps_y, span, TW, MAX_TAPS);
    const table_layout lay = layout(ow, oh, tile_w, taps_x, taps_y);
    VX_REQUIRE(table_bytes == lay.total * 4, "%s: %zu bytes of tables, the layout of this shape has %zu", who, table_bytes, lay.total * 4);
    const size_t lds_bytes = lds_words(ch, f32, tile_w, taps_x, taps_y, span) * 4;
    VX_REQUIRE(lds_bytes <= (size_t)LDS_BUDGET, "%s: the tile needs %zu bytes of LDS (at most %d)", who, lds_bytes, LDS_BUDGET);
    VX_REQUIRE((int64_t)B * lay.tiles_x * lay.tiles_y < (1LL << 31), "%s: %d images of %d x %d tiles pass the grid", who, B, lay.tiles_x, lay.tiles_y);
    const size_t px = f32 ? 4 * ch : ch, align = ch == 4 ? px : (f32 ? 4 : 1); // four-channel pixels are read as one word / one float4
    VX_REQUIRE(reinterpret_cast<uintptr_t>(src) % align == 0 && reinterpret_cast<uintptr_t>(dst) % (f32 ? 4 : 1) == 0 && reinterpret_cast<uintptr_t>(tables) % 4 == 0,
               "%s: misaligned pointer (%zu-byte pixels)", who, px);
    VX_REQUIRE(!overlap(src, (size_t)B * h * w * px, dst, (size_t)B * oh * ow * px), "%s: the output overlaps the input", who);
    const scale_args a = {src, dst, static_cast<const uint32_t*>(tables), lay, B, h, w, oh, ow, alpha[format], tile_w, taps_x, taps_y, span};
    hipStream_t st = as_stream(stream);
    if (f32) {
        if (ch == 4) launch<4, true>(a, lds_bytes, st);
        else if (ch == 3) launch<3, true>(a, lds_bytes, st);
        else launch<1, true>(a, lds_bytes, st);
    } else {
        if (ch == 4) launch<4, false>(a, lds_bytes, st);
        else if (ch == 3) launch<3, false>(a, lds_bytes, st);
        else launch<1, false>(a, lds_bytes, st);
    }
    VX_LAUNCH_CHECK();
    return 1;
}
