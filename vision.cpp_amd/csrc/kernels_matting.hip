// The matting image ops of the reference's image.h on the device (src/visp/image.cpp:358-535): box blur, erosion, the blur-fusion
// foreground estimator ("Approximate Fast Foreground Colour Estimation") and the u8 alpha composite.
//
// Summation order. The reference's blur keeps ONE f32 running sum along a whole row / column (add the entering pixel, subtract the
// leaving one), so the error of an output scales with everything the sum has passed. Here every output is the sum of its OWN window,
// added left to right (top to bottom) into an accumulator that starts at the first term: n = 2r + 1 terms, n - 1 additions, one
// multiplication by fl(1 / n). Nothing outside the window ever enters an output.
//   horizontal pass: one thread per output, lanes along x, the window read from the cache (a wave's loads are 64 consecutive pixels)
//   vertical pass:   one thread per column and strip of RUN rows, lanes along x (coalesced); a loaded value is added to the accumulators
//                    of the strip whose windows hold it -- to the others 0.0f is added, which is exact -- so RUN outputs cost
//                    RUN + 2r loads instead of RUN (2r + 1)
// The estimator's launches use the same strips along x and y from radius 8 on (launch_stage). Short sliding runs re-seeded from a direct
// sum were not taken: a run that slides past a bright region carries its rounding into the outputs behind it.
// No atomics, no scratch, 1 KiB of LDS in one kernel (the u8 -> f32 table); a thread's result depends on its own image only, so bits do not
// depend on the batch. Registers per kernel: DESIGN.md section 21.
#include "vx_common.h"

namespace {

constexpr int RUN = 4; // outputs per thread along the summed axis: rows in the vertical passes, columns in the estimator's horizontal pass

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <typename T> __device__ __forceinline__ T zero_of();
template <> __device__ __forceinline__ float zero_of<float>() { return 0.0f; }
template <> __device__ __forceinline__ f32x4 zero_of<f32x4>() { return f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }

// t [rows, w] (contiguous) = horizontal window means of x (rows of x_row elements of T); rows = B * h
template <typename T>
__global__ __launch_bounds__(256) void blur_h_kernel(const T* __restrict__ x, long x_row, T* __restrict__ t, int w, int r, float wgt, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int xx = (int)(i % w);
    const T* p = x + (i / w) * x_row;
    T s = p[clampi(xx - r, w - 1)];
    for (int k = 1 - r; k <= r; ++k) s += p[clampi(xx + k, w - 1)];
    t[i] = s * wgt;
}

// y (rows of y_row elements of T) = vertical window means of t [B, h, w]
template <typename T>
__global__ __launch_bounds__(256) void blur_v_kernel(const T* __restrict__ t, T* __restrict__ y, long y_row, int h, int w, int r, float wgt, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int strips = (h + RUN - 1) / RUN;
    const int xx = (int)(i % w);
    const long q = i / w;
    const int y0 = (int)(q % strips) * RUN;
    const long b = q / strips;
    const T* p = t + b * h * w + xx;
    T acc[RUN];
#pragma unroll
    for (int u = 0; u < RUN; ++u) acc[u] = zero_of<T>();
    const int n = 2 * r;
    for (int j = 0; j < RUN + n; ++j) { // row y0 - r + j is term j - u of output u
        const T v = p[(long)clampi(y0 - r + j, h - 1) * w];
        if (j >= RUN - 1 && j <= n) {
#pragma unroll
            for (int u = 0; u < RUN; ++u) acc[u] += v;
        } else {
#pragma unroll
            for (int u = 0; u < RUN; ++u) acc[u] += (j >= u && j - u <= n) ? v : zero_of<T>();
        }
    }
#pragma unroll
    for (int u = 0; u < RUN; ++u)
        if (y0 + u < h) y[(b * h + y0 + u) * y_row + xx] = acc[u] * wgt;
}

// minimum over the clamped (2r + 1)^2 neighbourhood, started at the format's one as erosion<T> does (image.cpp:509-525); the comparison
// is std::min's (the neighbour wins only when it is smaller), so the bits are the reference's
template <typename T>
__global__ __launch_bounds__(256) void erode_kernel(const T* __restrict__ x, long x_row, T* __restrict__ y, long y_row, int h, int w, int r, T one, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int xx = (int)(i % w);
    const long q = i / w;
    const int yy = (int)(q % h);
    const long b = q / h;
    const T* p = x + b * h * x_row;
    T val = one;
    for (int dy = -r; dy <= r; ++dy) {
        const T* row = p + (long)clampi(yy + dy, h - 1) * x_row;
        for (int dx = -r; dx <= r; ++dx) {
            const T v = row[clampi(xx + dx, w - 1)];
            val = v < val ? v : val;
        }
    }
    y[(b * h + yy) * y_row + xx] = val;
}

// ---- the estimator ----------------------------------------------------------------------------------------------------------
enum { FMT_RGBA_U8 = 0, FMT_RGB_U8 = 3, FMT_RGBA_F32 = 5 }; // visp_image_format's values

template <int FMT>
__device__ __forceinline__ f32x4 load_rgb(const void* img, long i) { // image_load (image-impl.h:22-32, 53-55); the alpha is never used
    if (FMT == FMT_RGBA_F32) return static_cast<const f32x4*>(img)[i];
    if (FMT == FMT_RGBA_U8) {
        const uchar4 u = static_cast<const uchar4*>(img)[i];
        return f32x4{float(u.x) / 255.0f, float(u.y) / 255.0f, float(u.z) / 255.0f, 0.0f};
    }
    const uint8_t* u = static_cast<const uint8_t*>(img) + 3 * i;
    return f32x4{float(u[0]) / 255.0f, float(u[1]) / 255.0f, float(u[2]) / 255.0f, 0.0f};
}

// the same pixel with the 256 quotients u / 255.0f read from a table (LDS) instead of divided again: the same bits, a dozen instructions fewer per channel
template <int FMT>
__device__ __forceinline__ f32x4 load_rgb(const void* img, long i, const float* lut) {
    if (FMT == FMT_RGBA_F32) return static_cast<const f32x4*>(img)[i];
    if (FMT == FMT_RGBA_U8) {
        const uchar4 u = static_cast<const uchar4*>(img)[i];
        return f32x4{lut[u.x], lut[u.y], lut[u.z], 0.0f};
    }
    const uint8_t* u = static_cast<const uint8_t*>(img) + 3 * i;
    return f32x4{lut[u[0]], lut[u[1]], lut[u[2]], 0.0f};
}

// planes [B, h, w][2] f32x4 = horizontal window means of {m, fg m} and {bg (1 - m), -}. STAGE2: fg and bg are rgba_f32 maps; otherwise
// both are the image. The products exist in registers only. One thread per row and strip of R columns, the vertical passes' scheme turned
// by 90 degrees: a tap is loaded (and converted) once for the R outputs whose windows hold it, R + 2r taps instead of R (2r + 1). A wave's
// loads cover 64 R consecutive pixels of a row. R = 1 is the plain form, one coalesced load per tap: the launcher takes it for small radii,
// where the strip saves little and its strided float4 loads cost more (profiles/matting_bench.txt).
template <int FMT, bool STAGE2, int R>
__global__ __launch_bounds__(256) void fg_h_kernel(const void* __restrict__ img, const f32x4* __restrict__ fg, const f32x4* __restrict__ bg, const float* __restrict__ mask,
                                                   f32x4* __restrict__ planes, int w, int r, float wgt, long total) {
    __shared__ float lut[256];
    if (!STAGE2 && FMT != FMT_RGBA_F32) {
        lut[threadIdx.x] = float(threadIdx.x) / 255.0f;
        __syncthreads();
    }
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int strips = (w + R - 1) / R;
    const int x0 = (int)(i % strips) * R;
    const long base = (i / strips) * w; // first pixel of the row
    f32x4 a[R], c[R];
#pragma unroll
    for (int u = 0; u < R; ++u) a[u] = c[u] = zero_of<f32x4>();
    const int n = 2 * r;
    for (int t = 0; t < R + n; ++t) { // column x0 - r + t is term t - u of output u
        const long j = base + clampi(x0 - r + t, w - 1);
        const float m = mask[j];
        f32x4 F, G;
        if (STAGE2) {
            F = fg[j];
            G = bg[j];
        } else {
            F = G = load_rgb<FMT>(img, j, lut);
        }
        const f32x4 va = f32x4{m, F[0] * m, F[1] * m, F[2] * m}, vc = G * (1.0f - m);
        if (t >= R - 1 && t <= n) {
#pragma unroll
            for (int u = 0; u < R; ++u) {
                a[u] += va;
                c[u] += vc;
            }
        } else {
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const bool in = t >= u && t - u <= n;
                a[u] += in ? va : zero_of<f32x4>();
                c[u] += in ? vc : zero_of<f32x4>();
            }
        }
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
        if (x0 + u >= w) break;
        planes[2 * (base + x0 + u)] = a[u] * wgt;
        planes[2 * (base + x0 + u) + 1] = c[u] * wgt;
    }
}

// vertical window means of the planes, then the combine (image.cpp:448-467): bf = blur(fg m) / (bm + 1e-5), bb = blur(bg (1 - m)) /
// (1 - bm + 1e-5), f = clamp(bf + m (img - m bf - (1 - m) bb), 0, 1), alpha = clamp(m, 0, 1). out: rgba_f32, or rgba_u8 by image_store's
// truncation; bg_out (nullable): bb as rgba_f32 (alpha 0: the next stage never reads it)
template <int FMT, int R>
__global__ __launch_bounds__(256) void fg_v_kernel(const f32x4* __restrict__ planes, const void* __restrict__ img, const float* __restrict__ mask, void* __restrict__ out,
                                                   int out_u8, f32x4* __restrict__ bg_out, int h, int w, int r, float wgt, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int strips = (h + R - 1) / R;
    const int xx = (int)(i % w);
    const long q = i / w;
    const int y0 = (int)(q % strips) * R;
    const long b = q / strips;
    const f32x4* p = planes + 2 * (b * h * w + xx);
    f32x4 a[R], c[R];
#pragma unroll
    for (int u = 0; u < R; ++u) a[u] = c[u] = zero_of<f32x4>();
    const int n = 2 * r;
    for (int j = 0; j < R + n; ++j) {
        const f32x4* s = p + 2 * ((long)clampi(y0 - r + j, h - 1) * w);
        const f32x4 va = s[0], vc = s[1];
        if (j >= R - 1 && j <= n) {
#pragma unroll
            for (int u = 0; u < R; ++u) {
                a[u] += va;
                c[u] += vc;
            }
        } else {
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const bool in = j >= u && j - u <= n;
                a[u] += in ? va : zero_of<f32x4>();
                c[u] += in ? vc : zero_of<f32x4>();
            }
        }
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
        if (y0 + u >= h) break;
        const long o = (b * h + y0 + u) * w + xx;
        const f32x4 sa = a[u] * wgt, sc = c[u] * wgt;
        const float m = mask[o], bm = sa[0];
        const f32x4 I = load_rgb<FMT>(img, o);
        const float df = bm + 1e-5f, db = (1.0f - bm) + 1e-5f;
        f32x4 f, bb;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float bf = sa[1 + ch] / df;
            bb[ch] = sc[ch] / db;
            const float v = bf + m * (I[ch] - m * bf - (1.0f - m) * bb[ch]);
            f[ch] = fminf(fmaxf(v, 0.0f), 1.0f);
        }
        f[3] = fminf(fmaxf(m, 0.0f), 1.0f);
        bb[3] = 0.0f;
        if (bg_out) bg_out[o] = bb;
        if (out_u8) static_cast<uchar4*>(out)[o] = make_uchar4((uint8_t)(f[0] * 255.0f), (uint8_t)(f[1] * 255.0f), (uint8_t)(f[2] * 255.0f), (uint8_t)(f[3] * 255.0f));
        else static_cast<f32x4*>(out)[o] = f;
    }
}

// alpha_composite (image.cpp:478-489): w fg + (1 - w) bg in f32 with every product and sum rounded on its own (no fused multiply-add: the
// host code this restates has none), stored by image_store's truncation
__global__ __launch_bounds__(256) void composite_kernel(const uchar4* __restrict__ fg, const uint8_t* __restrict__ bg, int bg_channels, const uint8_t* __restrict__ mask,
                                                        uchar4* __restrict__ out, long total) {
#pragma clang fp contract(off) // __fmul_rn / __fadd_rn are plain operators in HIP's headers: only this keeps the compiler from fusing them
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float wt = float(mask[i]) / 255.0f, wb = 1.0f - wt;
    const uchar4 f = fg[i];
    const uint8_t* g = bg + i * bg_channels;
    const float fv[3] = {float(f.x) / 255.0f, float(f.y) / 255.0f, float(f.z) / 255.0f};
    uint8_t o[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float a = wt * fv[ch], b = wb * (float(g[ch]) / 255.0f);
        const float v = a + b;
        o[ch] = (uint8_t)(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f);
    }
    out[i] = make_uchar4(o[0], o[1], o[2], 255);
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + nb && pb < pa + na;
}
bool aligned(const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
// elements an image batch of rows `row` elements apart spans
size_t span(int B, int h, int w, int64_t row) { return ((size_t)B * h - 1) * (size_t)row + (size_t)w; }

// what every launcher here refuses: extents that are not positive or whose element count passes 32-bit indexing
int check_extent(const char* who, int B, int h, int w, int C, int64_t row_in, int64_t row_out) {
    VX_REQUIRE(B > 0 && h > 0 && w > 0, "%s: batch %d, extent %dx%d must be positive", who, B, w, h);
    VX_REQUIRE(row_in >= (int64_t)w * C && row_out >= (int64_t)w * C, "%s: row strides %ld / %ld are shorter than a row of %d elements", who, (long)row_in, (long)row_out, w * C);
    const int64_t row = row_in > row_out ? row_in : row_out;
    VX_REQUIRE(row < (1LL << 31) && (int64_t)B * h * row < (1LL << 31), "%s: %d images of %dx%d (row stride %ld) pass 32-bit indexing", who, B, w, h, (long)row);
    return 1;
}
int check_radius(const char* who, int radius, int h, int w) {
    VX_REQUIRE(radius >= 1, "%s: radius %d must be at least 1", who, radius);
    VX_REQUIRE(radius <= w / 2 && radius <= h / 2, "%s: radius %d exceeds half the extent %dx%d", who, radius, w, h);
    return 1;
}

template <typename T>
int launch_blur(const T* x, long x_row, T* tmp, T* y, long y_row, int B, int h, int w, int radius, hipStream_t st) {
    const float wgt = 1.0f / float(2 * radius + 1);
    const long n_h = (long)B * h * w, n_v = (long)B * ((h + RUN - 1) / RUN) * w;
    hipLaunchKernelGGL(blur_h_kernel<T>, dim3(blocks_for(n_h)), dim3(256), 0, st, x, x_row, tmp, w, radius, wgt, n_h);
    hipLaunchKernelGGL(blur_v_kernel<T>, dim3(blocks_for(n_v)), dim3(256), 0, st, static_cast<const T*>(tmp), y, y_row, h, w, radius, wgt, n_v);
    VX_LAUNCH_CHECK();
    return 1;
}

template <typename T>
int launch_erode(const char* who, const T* x, int64_t x_row, T* y, int64_t y_row, int B, int h, int w, int radius, T one, void* stream) {
    VX_REQUIRE(x && y, "%s: null pointer", who);
    VX_REQUIRE(aligned(x, sizeof(T)) && aligned(y, sizeof(T)), "%s: misaligned pointer", who);
    if (!check_extent(who, B, h, w, 1, x_row, y_row)) return 0;
    VX_REQUIRE(radius >= 1, "%s: radius %d must be at least 1", who, radius);
    VX_REQUIRE(radius <= 64, "%s: radius %d is not built (at most 64: the neighbourhood is visited directly)", who, radius);
    VX_REQUIRE(!overlap(x, span(B, h, w, x_row) * sizeof(T), y, span(B, h, w, y_row) * sizeof(T)), "%s: the output overlaps the input", who);
    const long total = (long)B * h * w;
    hipLaunchKernelGGL(erode_kernel<T>, dim3(blocks_for(total)), dim3(256), 0, as_stream(stream), x, (long)x_row, y, (long)y_row, h, w, radius, one, total);
    VX_LAUNCH_CHECK();
    return 1;
}

// From this radius on a thread makes a strip of outputs along the summed axis (RUN columns in the horizontal launch, RUN_LONG rows in the vertical one);
// below it the horizontal launch is the plain one-output form and the vertical one keeps RUN rows (measured: profiles/matting_bench.txt).
constexpr int STRIP_RADIUS = 8;
constexpr int RUN_LONG = 8;
struct stage_args {
    const void* img;
    const f32x4 *fg, *bg;
    const float* mask;
    f32x4* planes;
    void* out;
    int out_u8;
    f32x4* bg_out;
    int B, h, w, radius;
    float wgt;
    int passes;
    hipStream_t st;
};
template <int FMT, bool STAGE2, int R>
void launch_stage_h(stage_args const& a) {
    const long n = (long)a.B * a.h * ((a.w + R - 1) / R);
    hipLaunchKernelGGL((fg_h_kernel<FMT, STAGE2, R>), dim3(blocks_for(n)), dim3(256), 0, a.st, a.img, a.fg, a.bg, a.mask, a.planes, a.w, a.radius, a.wgt, n);
}
template <int FMT, int R>
void launch_stage_v(stage_args const& a) {
    const long n = (long)a.B * ((a.h + R - 1) / R) * a.w;
    hipLaunchKernelGGL((fg_v_kernel<FMT, R>), dim3(blocks_for(n)), dim3(256), 0, a.st, static_cast<const f32x4*>(a.planes), a.img, a.mask, a.out, a.out_u8, a.bg_out, a.h, a.w,
                       a.radius, a.wgt, n);
}
template <int FMT>
void launch_stage(stage_args const& a) {
    const bool strip = a.radius >= STRIP_RADIUS;
    if (a.passes & 1) {
        if (a.fg) strip ? launch_stage_h<FMT, true, RUN>(a) : launch_stage_h<FMT, true, 1>(a);
        else strip ? launch_stage_h<FMT, false, RUN>(a) : launch_stage_h<FMT, false, 1>(a);
    }
    if (a.passes & 2) strip ? launch_stage_v<FMT, RUN_LONG>(a) : launch_stage_v<FMT, RUN>(a);
}

} // namespace

extern "C" int vx_box_blur_f32(const float* x, int64_t x_row, float* tmp, float* y, int64_t y_row, int B, int h, int w, int C, int radius, void* stream) {
    VX_REQUIRE(x && tmp && y, "vx_box_blur_f32: null pointer");
    VX_REQUIRE(C == 1 || C == 4, "vx_box_blur_f32: %d channels (1 or 4)", C);
    const size_t al = C == 4 ? 16 : 4;
    VX_REQUIRE(aligned(x, al) && aligned(tmp, al) && aligned(y, al) && x_row % C == 0 && y_row % C == 0, "vx_box_blur_f32: misaligned pointer or row stride (%d-byte pixels)", 4 * C);
    if (!check_extent("vx_box_blur_f32", B, h, w, C, x_row, y_row) || !check_radius("vx_box_blur_f32", radius, h, w)) return 0;
    const size_t nx = span(B, h, w * C, x_row) * 4, ny = span(B, h, w * C, y_row) * 4, nt = (size_t)B * h * w * C * 4;
    VX_REQUIRE(!overlap(x, nx, y, ny) && !overlap(x, nx, tmp, nt) && !overlap(tmp, nt, y, ny), "vx_box_blur_f32: input, workspace and output overlap");
    hipStream_t st = as_stream(stream);
    if (C == 1) return launch_blur<float>(x, (long)x_row, tmp, y, (long)y_row, B, h, w, radius, st);
    return launch_blur<f32x4>(reinterpret_cast<const f32x4*>(x), (long)(x_row / 4), reinterpret_cast<f32x4*>(tmp), reinterpret_cast<f32x4*>(y), (long)(y_row / 4), B, h, w, radius, st);
}

extern "C" int vx_erode_f32(const float* x, int64_t x_row, float* y, int64_t y_row, int B, int h, int w, int radius, void* stream) {
    return launch_erode<float>("vx_erode_f32", x, x_row, y, y_row, B, h, w, radius, 1.0f, stream);
}

extern "C" int vx_erode_u8(const uint8_t* x, int64_t x_row, uint8_t* y, int64_t y_row, int B, int h, int w, int radius, void* stream) {
    return launch_erode<uint8_t>("vx_erode_u8", x, x_row, y, y_row, B, h, w, radius, (uint8_t)255, stream);
}

extern "C" int vx_foreground_stage(const void* img, int img_format, const float* fg, const float* bg, const float* mask, float* planes, void* out, int out_format,
                                   float* bg_out, int B, int h, int w, int radius, int passes, void* stream) {
    const char* who = "vx_foreground_stage";
    VX_REQUIRE(passes >= 1 && passes <= 3, "%s: passes %d (1 horizontal, 2 vertical, 3 both)", who, passes);
    VX_REQUIRE(img && mask && planes && out, "%s: null pointer", who);
    VX_REQUIRE((fg == nullptr) == (bg == nullptr), "%s: fg and bg are given together (stage two) or not at all (stage one)", who);
    VX_REQUIRE(img_format == FMT_RGBA_U8 || img_format == FMT_RGB_U8 || img_format == FMT_RGBA_F32, "%s: image format %d (rgba_u8, rgb_u8 or rgba_f32)", who, img_format);
    VX_REQUIRE(out_format == FMT_RGBA_U8 || out_format == FMT_RGBA_F32, "%s: output format %d (rgba_u8 or rgba_f32)", who, out_format);
    const int img_px = img_format == FMT_RGBA_F32 ? 16 : (img_format == FMT_RGBA_U8 ? 4 : 3), out_px = out_format == FMT_RGBA_F32 ? 16 : 4;
    VX_REQUIRE(aligned(img, img_px == 3 ? 1 : img_px) && aligned(mask, 4) && aligned(planes, 16) && aligned(out, out_px) && (!fg || (aligned(fg, 16) && aligned(bg, 16))) &&
                   (!bg_out || aligned(bg_out, 16)),
               "%s: misaligned pointer", who);
    if (!check_extent(who, B, h, w, 8, (int64_t)w * 8, (int64_t)w * 8) || !check_radius(who, radius, h, w)) return 0;
    const size_t n = (size_t)B * h * w;
    const void* ins[4] = {img, mask, fg, bg};
    const size_t in_bytes[4] = {n * img_px, n * 4, n * 16, n * 16};
    void* outs[3] = {planes, out, bg_out};
    const size_t out_bytes[3] = {n * 32, n * out_px, n * 16};
    for (int o = 0; o < 3; ++o) {
        if (!outs[o]) continue;
        for (int i = 0; i < 4; ++i) VX_REQUIRE(!ins[i] || !overlap(ins[i], in_bytes[i], outs[o], out_bytes[o]), "%s: an output overlaps an input", who);
        for (int p = o + 1; p < 3; ++p) VX_REQUIRE(!outs[p] || !overlap(outs[p], out_bytes[p], outs[o], out_bytes[o]), "%s: outputs overlap", who);
    }
    hipStream_t st = as_stream(stream);
    const float wgt = 1.0f / float(2 * radius + 1);
    const stage_args sa = {img, reinterpret_cast<const f32x4*>(fg), reinterpret_cast<const f32x4*>(bg), mask, reinterpret_cast<f32x4*>(planes), out, out_format == FMT_RGBA_U8,
                           reinterpret_cast<f32x4*>(bg_out), B, h, w, radius, wgt, passes, st};
    switch (img_format) {
        case FMT_RGBA_U8: launch_stage<FMT_RGBA_U8>(sa); break;
        case FMT_RGB_U8: launch_stage<FMT_RGB_U8>(sa); break;
        case FMT_RGBA_F32: launch_stage<FMT_RGBA_F32>(sa); break;
    }
    VX_LAUNCH_CHECK();
    return 1;
}

extern "C" int vx_alpha_composite_u8(const uint8_t* fg_rgba, const uint8_t* bg, int bg_channels, const uint8_t* mask, uint8_t* out_rgba, int64_t n_pixels, void* stream) {
    const char* who = "vx_alpha_composite_u8";
    VX_REQUIRE(fg_rgba && bg && mask && out_rgba, "%s: null pointer", who);
    VX_REQUIRE(bg_channels == 3 || bg_channels == 4, "%s: background of %d channels (3 or 4)", who, bg_channels);
    VX_REQUIRE(aligned(fg_rgba, 4) && aligned(out_rgba, 4), "%s: misaligned pointer (rgba pixels are read as 4 bytes)", who);
    VX_REQUIRE(n_pixels > 0 && n_pixels * 4 < (1LL << 31), "%s: %ld pixels (positive, within 32-bit indexing)", who, (long)n_pixels);
    const size_t n = (size_t)n_pixels;
    VX_REQUIRE(!overlap(out_rgba, n * 4, fg_rgba, n * 4) && !overlap(out_rgba, n * 4, bg, n * bg_channels) && !overlap(out_rgba, n * 4, mask, n), "%s: the output overlaps an input", who);
    hipLaunchKernelGGL(composite_kernel, dim3(blocks_for((long)n_pixels)), dim3(256), 0, as_stream(stream), reinterpret_cast<const uchar4*>(fg_rgba), bg, bg_channels, mask,
                       reinterpret_cast<uchar4*>(out_rgba), (long)n_pixels);
    VX_LAUNCH_CHECK();
    return 1;
}
