// visp/vision.h -- the source-level C++ API of the MI355X backend, shaped like the reference's public header
// (reference include/visp/vision.h:124-347, include/visp/image.h:17-110, include/visp/ml.h:32-64): same namespace, type and
// function names, argument meaning and error behaviour (exceptions carrying the library's message), so that a C++ caller of
// the reference's high-level API -- scripts/pkg-check/main.cpp:22-44 is the model -- builds against this backend unchanged.
// Header-only over the binary-stable C ABI (include/visp_c_api.h, lib/libvisioncpp.so): link with -lvisioncpp.
//
// Covered: backend_init / backend_device, image_view / image_data / image_alloc / image_clear / image_scale / image_u8_to_f32 /
// image_normalize / image_span / image_to_mask / image_set_alpha / image_blur / image_erosion / image_estimate_foreground /
// image_alpha_composite, birefnet_cutout, per family *_load_model + *_compute for depth_anything, esrgan, birefnet and sam (sam_encode + sam_compute with a
// point or a box), and the Depth-Anything pipeline pieces depthany_params / depthany_detect_params / depthany_image_extent /
// depthany_process_input / depthany_process_output (vision.h:236-252).
// The ml.h layer -- model_file, model_weights, compute_graph, model_ref, tensor, transfer_* -- is visp/ml.h, the nn.h builders visp/nn.h.
// The graph builders of the reference's arch sources (dino::*, dpt::*, depthany_predict) are DECLARED in visp/builders.h and defined by
// those sources themselves: src/visp/arch/dino.cpp and depth-anything.cpp compile unmodified against these headers with
// -DVISP_GGML_NAMES -DVISP_ARCH_FROM_SOURCE (tests/test_reference_sources_compile.py). With VISP_ARCH_FROM_SOURCE the pipeline pieces
// the reference defines in depth-anything.cpp (image_extent / process_input / process_output) are declared here, not defined.
// Not covered: the *_predict builders of the other families (hand schedules only). migan_* loads through visp_migan_load and
// yolov9t::* through visp_yolov9t_load (visp_model_load refuses both).
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <exception>
#include <memory>
#include <span>
#include <string>
#include <utility>
#include <vector>

#include "../visp_c_api.h"

namespace visp {
using std::byte;
using std::span;
using f32x4 = std::array<float, 4>; // per-channel offset / scale of image_u8_to_f32 (arithmetic: util/math.h)

struct exception : std::exception { // reference src/util/... visp::exception: what() = the library's message
    std::string message;
    explicit exception(std::string m) : message(std::move(m)) {}
    char const* what() const noexcept override { return message.c_str(); }
};
namespace detail {
inline void check(int32_t ok) {
    if (!ok) throw exception(visp_get_last_error());
}
} // namespace detail

//
// images (include/visp/image.h)

struct i32x2 {
    int32_t v[2] = {0, 0};
    constexpr i32x2() = default;
    constexpr i32x2(int32_t x, int32_t y) : v{x, y} {}
    constexpr int32_t& operator[](int i) { return v[i]; }
    constexpr int32_t operator[](int i) const { return v[i]; }
    friend constexpr bool operator==(i32x2 a, i32x2 b) { return a.v[0] == b.v[0] && a.v[1] == b.v[1]; }
    friend constexpr bool operator!=(i32x2 a, i32x2 b) { return !(a == b); }
};
struct box_2d { i32x2 top_left, bottom_right; }; // sam_compute box prompt (vision.h:139-160)

enum class image_format : int32_t { rgba_u8, bgra_u8, argb_u8, rgb_u8, alpha_u8, rgba_f32, rgb_f32, alpha_f32 };
constexpr int n_channels(image_format f) {
    switch (f) {
        case image_format::rgb_u8: case image_format::rgb_f32: return 3;
        case image_format::alpha_u8: case image_format::alpha_f32: return 1;
        default: return 4;
    }
}
constexpr bool is_float(image_format f) { return int(f) >= int(image_format::rgba_f32); }
constexpr int n_bytes(image_format f) { return n_channels(f) * (is_float(f) ? 4 : 1); }

struct image_data;
struct image_view { // include/visp/image.h:37-41: non-owning
    i32x2 extent;
    int32_t stride = 0;
    image_format format = image_format::rgba_u8;
    void const* data = nullptr;

    image_view() = default;
    image_view(i32x2 e, image_format f, void const* d) : extent(e), stride(e[0] * n_bytes(f)), format(f), data(d) {}
    image_view(i32x2 e, int32_t s, image_format f, void const* d) : extent(e), stride(s), format(f), data(d) {}
    image_view(image_data const& img);
    image_view(i32x2 e, std::span<float const> d) : image_view(e, image_format::alpha_f32, d.data()) {} // one float per pixel
    std::span<uint8_t const> as_bytes() const { return {static_cast<uint8_t const*>(data), size_t(stride) * size_t(extent[1])}; }
    std::span<float const> as_floats() const { return {static_cast<float const*>(data), size_t(extent[0]) * size_t(extent[1]) * size_t(n_channels(format))}; }
};
struct image_data { // owning; include/visp/image.h:60-64
    i32x2 extent;
    image_format format = image_format::rgba_u8;
    std::unique_ptr<uint8_t[]> data;
};
inline image_view::image_view(image_data const& img) : image_view(img.extent, img.format, img.data.get()) {}

inline image_data image_alloc(i32x2 extent, image_format format) {
    size_t n = size_t(extent[0]) * size_t(extent[1]) * size_t(n_bytes(format));
    return image_data{extent, format, std::unique_ptr<uint8_t[]>(new uint8_t[n ? n : 1])};
}
inline void image_clear(image_data& img) { std::memset(img.data.get(), 0, size_t(img.extent[0]) * size_t(img.extent[1]) * size_t(n_bytes(img.format))); }

namespace detail {
inline visp_image_view c_view(image_view const& v) { return {v.extent[0], v.extent[1], v.stride, int32_t(v.format), const_cast<void*>(v.data)}; }
inline image_data take(visp_image_view const& v, visp_image_data* owner) { // copies the library-owned result into an image_data
    image_data out = image_alloc({v.width, v.height}, image_format(v.format));
    const size_t row = size_t(v.width) * size_t(n_bytes(out.format));
    for (int y = 0; y < v.height; ++y) std::memcpy(out.data.get() + y * row, static_cast<uint8_t const*>(v.data) + size_t(y) * size_t(v.stride), row);
    visp_image_destroy(owner);
    return out;
}
} // namespace detail

inline image_data image_scale(image_view const& img, i32x2 target) { // src/visp/image.cpp:352-356 (stb_image_resize semantics)
    visp_image_view in = detail::c_view(img), out{};
    visp_image_data* owner = nullptr;
    detail::check(visp_image_scale(&in, target[0], target[1], &out, &owner));
    return detail::take(out, owner);
}

// image.cpp:215-255: dst = (src / 255 + offset) * scale per channel, any u8 format -> the float format `format`
inline image_data image_u8_to_f32(image_view const& img, image_format format, std::array<float, 4> offset = {0, 0, 0, 0}, std::array<float, 4> scale = {1, 1, 1, 1}) {
    visp_image_view in = detail::c_view(img), out{};
    visp_image_data* owner = nullptr;
    detail::check(visp_image_u8_to_f32(&in, int32_t(format), offset.data(), scale.data(), &out, &owner));
    return detail::take(out, owner);
}
// image.cpp:537-582: min-max of an alpha_f32 image mapped to [min, max]
inline image_data image_normalize(image_view const& img, float min = 0, float max = 1) {
    visp_image_view in = detail::c_view(img), out{};
    visp_image_data* owner = nullptr;
    detail::check(visp_image_normalize(&in, min, max, &out, &owner));
    return detail::take(out, owner);
}

// include/visp/image.h:68-88: mutable, non-owning; converts to an image_view
struct image_span {
    i32x2 extent;
    int32_t stride = 0;
    image_format format = image_format::rgba_u8;
    void* data = nullptr;

    image_span() = default;
    image_span(image_data& img) : extent(img.extent), stride(img.extent[0] * n_bytes(img.format)), format(img.format), data(img.data.get()) {}
    image_span(i32x2 e, image_format f, void* d) : extent(e), stride(e[0] * n_bytes(f)), format(f), data(d) {}
    image_span(i32x2 e, std::span<float> d) : image_span(e, image_format::alpha_f32, d.data()) {} // one float per pixel
    operator image_view() const { return image_view(extent, stride, format, data); }
};
namespace detail {
inline void take_into(visp_image_view const& v, visp_image_data* owner, image_span const& dst, char const* who) { // the library-owned result into the caller's span
    const bool fits = dst.extent == i32x2{v.width, v.height} && int32_t(dst.format) == v.format && dst.data;
    const size_t row = size_t(v.width) * size_t(n_bytes(image_format(v.format)));
    for (int y = 0; fits && y < v.height; ++y)
        std::memcpy(static_cast<uint8_t*>(dst.data) + size_t(y) * size_t(dst.stride), static_cast<uint8_t const*>(v.data) + size_t(y) * size_t(v.stride), row);
    visp_image_destroy(owner);
    if (!fits) throw exception(std::string(who) + ": the destination's extent or format differs from the source's");
}
} // namespace detail

// The matting ops (include/visp/image.h:141-170). They compute on the calling thread's current HIP device (the reference's run on the host and take no
// device either); image_to_mask and image_set_alpha are host code.
// image.cpp:304-308: the first channel of a u8 image as alpha_u8
inline image_data image_to_mask(image_view const& src) {
    visp_image_view in = detail::c_view(src), out{};
    visp_image_data* owner = nullptr;
    detail::check(visp_image_to_mask(&in, &out, &owner));
    return detail::take(out, owner);
}
inline void image_to_mask(image_view const& src, image_span const& dst) {
    visp_image_view in = detail::c_view(src), out{};
    visp_image_data* owner = nullptr;
    detail::check(visp_image_to_mask(&in, &out, &owner));
    detail::take_into(out, owner, dst, "image_to_mask");
}
// image.cpp:310-323: writes `alpha` (alpha_u8) to the alpha channel of `img` (rgba_u8 / bgra_u8 / argb_u8), in place
inline void image_set_alpha(image_span const& img, image_view const& alpha) {
    visp_image_view in = detail::c_view(img), a = detail::c_view(alpha), out{};
    visp_image_data* owner = nullptr;
    detail::check(visp_image_set_alpha(&in, &a, &out, &owner));
    detail::take_into(out, owner, img, "image_set_alpha");
}
// image.cpp:410-419: box filter of size 2 radius + 1, alpha_f32 / rgba_f32
inline void image_blur(image_view const& src, image_span const& dst, int radius) {
    visp_image_view in = detail::c_view(src), out{};
    visp_image_data* owner = nullptr;
    detail::check(visp_image_blur(nullptr, &in, radius, &out, &owner));
    detail::take_into(out, owner, dst, "image_blur");
}
// image.cpp:527-535: minimum in the square neighbourhood, alpha_u8 / alpha_f32
inline void image_erosion(image_view const& src, image_span const& dst, int radius) {
    visp_image_view in = detail::c_view(src), out{};
    visp_image_data* owner = nullptr;
    detail::check(visp_image_erosion(nullptr, &in, radius, &out, &owner));
    detail::take_into(out, owner, dst, "image_erosion");
}
// not in the reference's header: SAM's remove_small_regions on an alpha_u8 mask, in place on the device (non-zero = foreground, 8-connectivity). Components of
// fewer than min_area pixels go: holes (background) become 255, islands (foreground) 0 -- but where every island is small the largest stays --, `both` the
// holes first. Returns whether a pixel changed.
enum class region_mode { holes = VISP_REGIONS_HOLES, islands = VISP_REGIONS_ISLANDS, both = VISP_REGIONS_BOTH };
inline bool image_remove_small_regions(image_span const& mask, int min_area, region_mode mode = region_mode::both) {
    if (mask.format != image_format::alpha_u8) throw exception("image_remove_small_regions: expected an alpha_u8 mask");
    const size_t w = size_t(mask.extent[0]), h = size_t(mask.extent[1]);
    std::vector<uint8_t> packed(w * h);
    for (size_t y = 0; y < h; ++y) std::memcpy(packed.data() + y * w, static_cast<uint8_t const*>(mask.data) + y * size_t(mask.stride), w);
    int32_t changed = 0;
    detail::check(visp_image_remove_small_regions_host(packed.data(), 1, mask.extent[0], mask.extent[1], min_area, int32_t(mode), &changed, nullptr));
    for (size_t y = 0; y < h; ++y) std::memcpy(static_cast<uint8_t*>(mask.data) + y * size_t(mask.stride), packed.data() + y * w, w);
    return changed != 0;
}
// image.cpp:471-476: img rgba_f32 (its alpha is not used), mask alpha_f32 -> rgba_f32 foreground colours, alpha = mask
inline image_data image_estimate_foreground(image_view const& img, image_view const& mask, int radius = 30) {
    visp_image_view in = detail::c_view(img), mk = detail::c_view(mask), out{};
    visp_image_data* owner = nullptr;
    detail::check(visp_image_estimate_foreground(nullptr, &in, &mk, radius, &out, &owner));
    return detail::take(out, owner);
}
// image.cpp:491-507: dst = fg * alpha + bg * (1 - alpha) as rgba_u8
inline image_data image_alpha_composite(image_view const& fg, image_view const& bg, image_view const& mask) {
    visp_image_view f = detail::c_view(fg), b = detail::c_view(bg), mk = detail::c_view(mask), out{};
    visp_image_data* owner = nullptr;
    detail::check(visp_image_alpha_composite(nullptr, &f, &b, &mk, &out, &owner));
    return detail::take(out, owner);
}
inline void image_alpha_composite(image_view const& fg, image_view const& bg, image_view const& mask, image_span const& dst) {
    visp_image_view f = detail::c_view(fg), b = detail::c_view(bg), mk = detail::c_view(mask), out{};
    visp_image_data* owner = nullptr;
    detail::check(visp_image_alpha_composite(nullptr, &f, &b, &mk, &out, &owner));
    detail::take_into(out, owner, dst, "image_alpha_composite");
}

//
// backend (include/visp/ml.h:32-64)

enum class backend_type : int32_t { cpu = 1, gpu = 2, vulkan = gpu | 1 << 8 };

struct backend_device {
    visp_device* handle = nullptr;
    backend_device() = default;
    explicit backend_device(visp_device* h) : handle(h) {}
    backend_device(backend_device&& o) noexcept : handle(std::exchange(o.handle, nullptr)) {}
    backend_device& operator=(backend_device&& o) noexcept { std::swap(handle, o.handle); return *this; }
    ~backend_device() { if (handle) visp_device_destroy(handle); }
    backend_type type() const { return backend_type(visp_device_type(handle)); }
    char const* name() const { return visp_device_name(handle); }
    char const* description() const { return visp_device_description(handle); }
};
inline backend_device backend_init() { // first available device (here: the first gfx950 GPU)
    visp_device* d = nullptr;
    detail::check(visp_device_init(VISP_BACKEND_AUTO, &d));
    return backend_device(d);
}
inline backend_device backend_init(backend_type t) { // backend_type::cpu throws: this build has no CPU backend
    visp_device* d = nullptr;
    detail::check(visp_device_init(int32_t(t), &d));
    return backend_device(d);
}
inline bool backend_is_available(backend_type t) { return t == backend_type::gpu; }

//
// models (include/visp/vision.h)

namespace detail {
template <int Family>
struct model_handle {
    visp_model* handle = nullptr;
    model_handle() = default;
    explicit model_handle(visp_model* h) : handle(h) {}
    model_handle(model_handle&& o) noexcept : handle(std::exchange(o.handle, nullptr)) {}
    model_handle& operator=(model_handle&& o) noexcept { std::swap(handle, o.handle); return *this; }
    ~model_handle() { if (handle) visp_model_destroy(handle, Family); }
};
template <int Family>
inline visp_model* load(char const* filepath, backend_device const& dev) {
    visp_model* m = nullptr;
    check(visp_model_load(filepath, dev.handle, Family, &m));
    return m;
}
template <int Family>
inline image_data compute(visp_model* m, image_view const& image, int32_t* args = nullptr, int32_t n_args = 0) {
    visp_image_view in = c_view(image), out{};
    visp_image_data* owner = nullptr;
    check(visp_model_compute(m, Family, &in, 1, args, n_args, &out, &owner));
    return take(out, owner);
}
} // namespace detail

// Depth-Anything (vision.h:224-252, 339-347). The device must outlive the model.
using depthany_model = detail::model_handle<VISP_DEPTH_ANYTHING>;
inline depthany_model depthany_load_model(char const* filepath, backend_device const& dev) { return depthany_model(detail::load<VISP_DEPTH_ANYTHING>(filepath, dev)); }
inline image_data depthany_compute(depthany_model& model, image_view image) { // -> alpha_f32 in [0, 1] at the input extent (vision.cpp:147-167)
    visp_image_view in = detail::c_view(image), out{};
    visp_image_data* owner = nullptr;
    detail::check(visp_depthany_compute_f32(model.handle, &in, &out, &owner));
    return detail::take(out, owner);
}

// --- Depth Anything pipeline (vision.h:236-252, arch/depth-anything.cpp:112-149). The reference reads the parameters from a
// model_file; this backend has no GGUF surface in its public header, so they come from the loaded model.
struct dino_params { int patch_size = 14, embed_dim = 384, n_layers = 12, n_heads = 6; }; // vision.h dino_params
struct depthany_params {
    int image_size = 518;
    int image_multiple = 14;
    i32x2 image_extent = {518, 518};
    float max_depth = 1;
    std::array<int, 4> feature_layers = {2, 5, 8, 11};
    dino_params dino;
};
// --- ESRGAN pipeline (vision.h:294-304): scale factor and number of RRDB blocks, from the GGUF keys esrgan.scale / esrgan.block_count
struct esrgan_params {
    int scale = 4;
    int n_blocks = 23;
};
#ifdef VISP_ARCH_FROM_SOURCE
// the reference's own definitions (src/visp/arch/depth-anything.cpp:112-149) are part of the build
i32x2 depthany_image_extent(i32x2 input_extent, depthany_params const&);
image_data depthany_process_input(image_view image, depthany_params const&);
image_data depthany_process_output(std::span<float const> output_data, i32x2 target_extent, depthany_params const&);
#else
// round the short side up to a multiple of image_multiple (at least image_size), keep the aspect ratio, round both up (:112-117)
inline i32x2 depthany_image_extent(i32x2 extent, depthany_params const& p) {
    auto next_multiple = [](int x, int m) { return (x + m - 1) / m * m; };
    const int min_side = extent[0] < extent[1] ? extent[0] : extent[1];
    const int tgt = next_multiple(min_side, p.image_multiple) > p.image_size ? next_multiple(min_side, p.image_multiple) : p.image_size;
    return i32x2(next_multiple(extent[0] * tgt / min_side, p.image_multiple), next_multiple(extent[1] * tgt / min_side, p.image_multiple));
}
#endif
inline depthany_params depthany_detect_params(depthany_model const& model, i32x2 input_extent = {}) { // (:119-128)
    visp_depthany_info info{};
    detail::check(visp_depthany_get_info(model.handle, &info));
    depthany_params p;
    p.image_size = info.image_size;
    p.image_multiple = info.image_multiple;
    p.max_depth = info.max_depth;
    for (int i = 0; i < 4; ++i) p.feature_layers[size_t(i)] = info.feature_layers[i];
    p.dino = dino_params{info.patch_size, info.embed_dim, info.n_layers, info.n_heads};
    if (input_extent[0] > 0 && input_extent[1] > 0) p.image_extent = depthany_image_extent(input_extent, p);
    return p;
}
#ifndef VISP_ARCH_FROM_SOURCE
// image_scale to the model extent where it differs, then (u8 / 255 - mean) / std -> rgb_f32 (:130-140)
inline image_data depthany_process_input(image_view image, depthany_params const& p) {
    image_data resized;
    if (image.extent[0] != p.image_extent[0] || image.extent[1] != p.image_extent[1]) {
        resized = image_scale(image, p.image_extent);
        image = image_view(resized);
    }
    return image_u8_to_f32(image, image_format::rgb_f32, {-0.485f, -0.456f, -0.406f, 0.f}, {1.f / 0.229f, 1.f / 0.224f, 1.f / 0.225f, 1.f});
}
// min-max normalise the raw depth at the model extent, scale to the caller's extent where it differs (:142-149)
inline image_data depthany_process_output(std::span<float const> output_data, i32x2 target_extent, depthany_params const& p) {
    image_data normalized = image_normalize(image_view(p.image_extent, image_format::alpha_f32, output_data.data()));
    if (normalized.extent[0] != target_extent[0] || normalized.extent[1] != target_extent[1]) return image_scale(normalized, target_extent);
    return normalized;
}
#endif

// MI-GAN (vision.h:257-279): image rgb/rgba u8 + alpha_u8 mask of any extent -> rgba_u8 at that extent, alpha = mask (vision.cpp:172-203)
using migan_model = detail::model_handle<VISP_MIGAN>;
inline migan_model migan_load_model(char const* filepath, backend_device const& dev) {
    visp_model* m = nullptr;
    detail::check(visp_migan_load(filepath, dev.handle, &m));
    return migan_model(m);
}
inline image_data migan_compute(migan_model& model, image_view image, image_view mask) {
    visp_image_view in = detail::c_view(image), mk = detail::c_view(mask), out{};
    visp_image_data* owner = nullptr;
    detail::check(visp_migan_compute(model.handle, &in, &mk, &out, &owner));
    return detail::take(out, owner);
}
struct migan_params { int resolution = 256; bool invert_mask = true; }; // vision.h:263-266
inline migan_params migan_detect_params(migan_model const& model) { // the GGUF key migan.image_size, read from the loaded model
    visp_migan_info info{};
    detail::check(visp_migan_get_info(model.handle, &info));
    return migan_params{info.resolution, true};
}
// migan.cpp:142-159, 181-196: both inputs scaled to resolution^2, then {a - 0.5, a (2 rgb - 1)} with a = 1 - mask (inverted) -> rgba_f32
inline image_data migan_process_input(image_view image, image_view mask, migan_params const& p) {
    const i32x2 res{p.resolution, p.resolution};
    image_data si, sm;
    if (image.extent != res) { si = image_scale(image, res); image = image_view(si); }
    if (mask.extent != res) { sm = image_scale(mask, res); mask = image_view(sm); }
    const int ch = n_channels(image.format);
    if (ch != 3 && ch != 4) throw exception("Unsupported image format for migan image input");
    image_data out = image_alloc(res, image_format::rgba_f32);
    float* o = reinterpret_cast<float*>(out.data.get());
    for (int y = 0; y < res[1]; ++y)
        for (int x = 0; x < res[0]; ++x) {
            const uint8_t* px = static_cast<const uint8_t*>(image.data) + size_t(y) * image.stride + size_t(x) * ch;
            float a = static_cast<const uint8_t*>(mask.data)[size_t(y) * mask.stride + x] / 255.0f;
            if (p.invert_mask) a = 1.0f - a;
            float* d = o + (size_t(y) * res[0] + x) * 4;
            d[0] = a - 0.5f;
            for (int c = 0; c < 3; ++c) d[1 + c] = a * (px[c] / 255.0f * 2.0f - 1.0f);
        }
    return out;
}
// migan.cpp:198-206: rgb f32 at resolution^2 -> scaled to extent -> rgba_u8 with x * 0.5 + 0.5 (alpha 255; vision.cpp then sets the mask)
inline image_data migan_process_output(std::span<float const> data, i32x2 extent, migan_params const& p) {
    const i32x2 res{p.resolution, p.resolution};
    image_view img(res, image_format::rgb_f32, data.data());
    image_data scaled;
    if (extent != res) { scaled = image_scale(img, extent); img = image_view(scaled); }
    image_data out = image_alloc(extent, image_format::rgba_u8);
    for (int y = 0; y < extent[1]; ++y)
        for (int x = 0; x < extent[0]; ++x) {
            const float* s = reinterpret_cast<const float*>(static_cast<const uint8_t*>(img.data) + size_t(y) * img.stride) + size_t(x) * 3;
            uint8_t* d = out.data.get() + (size_t(y) * extent[0] + x) * 4;
            for (int c = 0; c < 3; ++c) d[c] = uint8_t(std::clamp(s[c] * 0.5f + 0.5f, 0.0f, 1.0f) * 255.0f);
            d[3] = 255;
        }
    return out;
}

// YOLOv9t (reference src/visp/arch/yolov9t.h, namespace visp::yolov9t): loaded through visp_yolov9t_load, since the reference has no
// model_family for it. detect = letterbox + network + non_max_suppression + scale_boxes
// (inference_yolov9t.cpp:300-405); inputs rgb_u8 / rgba_u8 (alpha ignored).
namespace yolov9t {
using detected_obj = visp_detection; // {x1, y1, x2, y2, confidence, class_id, class_confidence} (yolov9t.h:30-35)
struct NMSParams { // yolov9t.h:68-74 field names; the defaults are the values inference_yolov9t.cpp:383 passes (max_det 300, max_wh 640)
    float conf_thres = 0.25f;
    float iou_thres = 0.45f;
    int max_det = 300;
    int max_nms = 30000;
    int max_wh = 640;
};
struct LetterboxResult { image_data img; float gain = 1, pad_w = 0, pad_h = 0; }; // yolov9t.h:13-18
using yolov9t_model = detail::model_handle<VISP_FAMILY_COUNT>; // outside visp_model_family; visp_model_destroy ignores the family
struct yolov9t_params { int num_classes = 80, input_size = 640, reg_max = 16; };

inline yolov9t_model yolov9t_load_model(char const* filepath, backend_device const& dev) {
    visp_model* m = nullptr;
    detail::check(visp_yolov9t_load(filepath, dev.handle, &m));
    return yolov9t_model(m);
}
inline yolov9t_params yolov9t_detect_params(yolov9t_model const& model) {
    visp_yolov9t_info info{};
    detail::check(visp_yolov9t_get_info(model.handle, &info));
    return yolov9t_params{info.num_classes, info.input_size, info.reg_max};
}
// letterbox (yolov9t.cpp:1028-1083) to size x size rgb_u8 with the colour-114 border
inline LetterboxResult letterbox(image_view image, int size = 640) {
    LetterboxResult r;
    r.img = image_alloc(i32x2{size, size}, image_format::rgb_u8);
    visp_image_view in = detail::c_view(image);
    detail::check(visp_yolov9t_letterbox(&in, size, r.img.data.get(), &r.gain, &r.pad_w, &r.pad_h));
    return r;
}
inline std::vector<detected_obj> yolov9t_detect(yolov9t_model& model, image_view image, NMSParams const& p = {}) {
    const visp_yolov9t_nms_params c{p.conf_thres, p.iou_thres, p.max_det, p.max_nms, p.max_wh};
    std::vector<detected_obj> out(size_t(std::max(p.max_det, 0)));
    visp_image_view in = detail::c_view(image);
    int32_t n = 0;
    detail::check(visp_yolov9t_detect(model.handle, &in, &c, out.data(), int32_t(out.size()), &n));
    out.resize(size_t(std::min<int32_t>(n, int32_t(out.size()))));
    return out;
}
} // namespace yolov9t

// ESRGAN (vision.h:284-304): any size, tiled, -> rgba_u8 at scale x the input extent (vision.cpp:220-253)
using esrgan_model = detail::model_handle<VISP_ESRGAN>;
inline esrgan_model esrgan_load_model(char const* filepath, backend_device const& dev) { return esrgan_model(detail::load<VISP_ESRGAN>(filepath, dev)); }
inline image_data esrgan_compute(esrgan_model& model, image_view image) { return detail::compute<VISP_ESRGAN>(model.handle, image); }

// BiRefNet (vision.h birefnet_*; vision.cpp:98-132): any 8-bit colour image -> alpha_u8 foreground mask at the input extent
using birefnet_model = detail::model_handle<VISP_BIREFNET>;
inline birefnet_model birefnet_load_model(char const* filepath, backend_device const& dev) { return birefnet_model(detail::load<VISP_BIREFNET>(filepath, dev)); }
inline image_data birefnet_compute(birefnet_model& model, image_view image) { return detail::compute<VISP_BIREFNET>(model.handle, image); }
// not in the reference's header: what its `vision-cli birefnet --composite` makes (src/cli/cli.cpp:327-347) -- the image as an rgba_u8 cutout at its own
// extent, colours from image_estimate_foreground on the network's mask, alpha = the mask -- without the mask leaving the device
inline image_data birefnet_cutout(birefnet_model& model, image_view image, int radius = 30) {
    visp_image_view in = detail::c_view(image), out{};
    visp_image_data* owner = nullptr;
    detail::check(visp_birefnet_cutout(model.handle, &in, radius, &out, &owner));
    return detail::take(out, owner);
}

// MobileSAM (vision.h:139-160): sam_encode once per image, then any number of prompts (vision.cpp:26-92) -> alpha_u8 mask
using sam_model = detail::model_handle<VISP_SAM>;
inline sam_model sam_load_model(char const* filepath, backend_device const& dev) { return sam_model(detail::load<VISP_SAM>(filepath, dev)); }
inline void sam_encode(sam_model& model, image_view image) {
    visp_image_view in = detail::c_view(image);
    detail::check(visp_sam_encode(model.handle, &in));
}
namespace detail {
inline image_data sam_prompt(sam_model& model, int32_t const* prompt, int32_t n) {
    visp_image_view out{};
    visp_image_data* owner = nullptr;
    check(visp_sam_compute(model.handle, prompt, n, &out, &owner));
    return take(out, owner);
}
} // namespace detail
inline image_data sam_compute(sam_model& model, i32x2 point) {
    int32_t p[2] = {point[0], point[1]};
    return detail::sam_prompt(model, p, 2);
}
inline image_data sam_compute(sam_model& model, box_2d box) {
    int32_t p[4] = {box.top_left[0], box.top_left[1], box.bottom_right[0], box.bottom_right[1]};
    return detail::sam_prompt(model, p, 4);
}
// not in the reference's header: many prompts on one sam_encode in one batched pass -> one alpha_u8 mask per prompt, in order
namespace detail {
inline std::vector<image_data> sam_prompts(sam_model& model, std::vector<int32_t> const& prompts, int32_t n_args) {
    const int32_t n = int32_t(prompts.size() / 4);
    int32_t w = 0, h = 0;
    check(visp_sam_image_extent(model.handle, &w, &h));
    std::vector<int32_t> counts(size_t(n), n_args);
    std::vector<uint8_t> masks(size_t(n) * size_t(w) * size_t(h));
    check(visp_sam_compute_batch_host(model.handle, prompts.data(), counts.data(), n, masks.data(), nullptr, nullptr));
    std::vector<image_data> out;
    for (int32_t i = 0; i < n; ++i) {
        out.push_back(image_alloc({w, h}, image_format::alpha_u8));
        std::memcpy(out.back().data.get(), masks.data() + size_t(i) * size_t(w) * size_t(h), size_t(w) * size_t(h));
    }
    return out;
}
} // namespace detail
inline std::vector<image_data> sam_compute_batch(sam_model& model, span<i32x2 const> points) {
    std::vector<int32_t> p;
    for (i32x2 const& pt : points) p.insert(p.end(), {pt[0], pt[1], 0, 0});
    return detail::sam_prompts(model, p, 2);
}
inline std::vector<image_data> sam_compute_batch(sam_model& model, span<box_2d const> boxes) {
    std::vector<int32_t> p;
    for (box_2d const& b : boxes) p.insert(p.end(), {b.top_left[0], b.top_left[1], b.bottom_right[0], b.bottom_right[1]});
    return detail::sam_prompts(model, p, 4);
}

// not in the reference's header: automatic mask generation, SAM's automatic mask generator on one sam_encode (one crop layer, no crop-edge filter).
// The pixel centres of an n x n grid over an image of `extent`, row by row: the point prompts of a "segment everything" pass
inline std::vector<i32x2> sam_point_grid(int n_per_side, i32x2 extent) {
    std::vector<i32x2> out;
    for (int y = 0; y < n_per_side; ++y)
        for (int x = 0; x < n_per_side; ++x) out.push_back(i32x2{int((x + 0.5) * extent[0] / n_per_side), int((y + 0.5) * extent[1] / n_per_side)});
    return out;
}
struct sam_generate_params { // SAM's defaults
    float pred_iou_thresh = 0.88f;
    float stability_thresh = 0.95f;
    float stability_offset = 1.0f;
    float nms_iou_thresh = 0.7f;
    int max_masks = 256;
    // SAM's min_mask_region_area: above 0, holes and islands of fewer pixels are removed from the masks on the device and a second NMS runs
    // (postprocess_small_regions); unchanged masks then come first and changed ones behind them, each by predicted iou -- not the order without cleaning
    int min_mask_region_area = 0;
};
struct sam_mask {
    image_data segmentation;   // alpha_u8 at the encoded image's extent, 0 / 255
    int area = 0;              // pixels that are 255
    i32x2 bbox_top_left{0, 0}, bbox_extent{0, 0}; // of those pixels; 0, 0, 0, 0 for an empty mask
    float predicted_iou = 0, stability_score = 0;
    int prompt = 0, plane = 0; // which prompt of the call and which of its three logit planes
    bool cleaned = false;      // min_mask_region_area changed a pixel of it
};
namespace detail {
inline std::vector<sam_mask> sam_generate(sam_model& model, std::vector<int32_t> const& prompts, int32_t n_args, sam_generate_params const& p) {
    const int32_t n = int32_t(prompts.size() / 4), cap = int32_t(p.max_masks);
    int32_t w = 0, h = 0, counts[4] = {0, 0, 0, 0};
    check(visp_sam_image_extent(model.handle, &w, &h));
    const size_t px = size_t(w) * size_t(h), rows = size_t(cap > 0 ? cap : 0);
    std::vector<int32_t> n_arg(size_t(n), n_args), info_i(rows * 8);
    std::vector<uint8_t> masks(rows * px);
    std::vector<float> info_f(rows * 2);
    if (p.min_mask_region_area != 0)
        check(visp_sam_generate_masks_clean_host(model.handle, prompts.data(), n_arg.data(), n, p.pred_iou_thresh, p.stability_thresh, p.stability_offset, p.nms_iou_thresh,
                                                 cap, p.min_mask_region_area, masks.data(), info_i.data(), info_f.data(), counts));
    else
        check(visp_sam_generate_masks_host(model.handle, prompts.data(), n_arg.data(), n, p.pred_iou_thresh, p.stability_thresh, p.stability_offset, p.nms_iou_thresh, cap,
                                           masks.data(), info_i.data(), info_f.data(), counts));
    std::vector<sam_mask> out;
    for (int32_t k = 0; k < counts[0]; ++k) {
        sam_mask s;
        s.segmentation = image_alloc({w, h}, image_format::alpha_u8);
        std::memcpy(s.segmentation.data.get(), masks.data() + size_t(k) * px, px);
        int32_t const* r = info_i.data() + size_t(k) * 8;
        s.prompt = r[0]; s.plane = r[1];
        s.bbox_top_left = i32x2{r[2], r[3]};
        s.bbox_extent = i32x2{r[4], r[5]};
        s.area = r[6];
        s.cleaned = r[7] != 0;
        s.predicted_iou = info_f[size_t(k) * 2];
        s.stability_score = info_f[size_t(k) * 2 + 1];
        out.push_back(std::move(s));
    }
    return out;
}
} // namespace detail
inline std::vector<sam_mask> sam_generate_masks(sam_model& model, span<i32x2 const> points, sam_generate_params const& params = {}) {
    std::vector<int32_t> p;
    for (i32x2 const& pt : points) p.insert(p.end(), {pt[0], pt[1], 0, 0});
    return detail::sam_generate(model, p, 2, params);
}
inline std::vector<sam_mask> sam_generate_masks(sam_model& model, span<box_2d const> boxes, sam_generate_params const& params = {}) {
    std::vector<int32_t> p;
    for (box_2d const& b : boxes) p.insert(p.end(), {b.top_left[0], b.top_left[1], b.bottom_right[0], b.bottom_right[1]});
    return detail::sam_generate(model, p, 4, params);
}
inline std::vector<sam_mask> sam_generate_masks(sam_model& model, int points_per_side = 32, sam_generate_params const& params = {}) {
    int32_t w = 0, h = 0;
    detail::check(visp_sam_image_extent(model.handle, &w, &h));
    std::vector<i32x2> grid = sam_point_grid(points_per_side, i32x2{w, h});
    return sam_generate_masks(model, span<i32x2 const>(grid), params);
}

} // namespace visp
