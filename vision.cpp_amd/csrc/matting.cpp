#include "matting.h"

#include <algorithm>
#include <optional>

#include "visp_util.h"

namespace visp {

namespace {

// the device a host-view op runs on: the given one (its turn held, its stream), or whatever is current for the thread (default stream)
struct device_scope {
    std::optional<device_turn> turn;
    void* stream = nullptr;
    explicit device_scope(backend_device const* dev) {
        if (dev) {
            turn.emplace(*dev);
            stream = dev->stream;
        }
    }
};

void require_view(char const* who, image_view const& v) {
    if (!v.data) throw except("%s: null image data", who);
    if (v.extent[0] < 1 || v.extent[1] < 1) throw except("%s: empty image (%dx%d)", who, v.extent[0], v.extent[1]);
    if (int(v.format) < 0 || int(v.format) > int(image_format::alpha_f32)) throw except("Unsupported image format [%d]", int(v.format));
    if ((int64_t)v.stride < (int64_t)v.extent[0] * n_bytes(v.format)) throw except("%s: row stride %d is shorter than a row", who, v.stride);
}
void require_radius(char const* who, int radius, i32x2 extent) { // blur()'s assertions (image.cpp:361-363)
    if (radius < 1) throw except("%s: radius %d must be at least 1", who, radius);
    if (radius > extent[0] / 2 || radius > extent[1] / 2) throw except("%s: radius %d exceeds half the extent %dx%d", who, radius, extent[0], extent[1]);
}
void require_same_extent(char const* who, image_view const& a, image_view const& b) {
    if (a.extent != b.extent) throw except("%s: extents differ (%dx%d and %dx%d)", who, a.extent[0], a.extent[1], b.extent[0], b.extent[1]);
}

device_buffer upload(image_data const& img, void* stream) {
    const size_t n = n_bytes(view_of(img));
    device_buffer b(n);
    VX(vx_memcpy_h2d(b.ptr, img.data.get(), n, stream));
    return b;
}
image_data download(device_buffer const& b, i32x2 extent, image_format format, void* stream) {
    image_data out = image_alloc(extent, format);
    VX(vx_memcpy_d2h(out.data.get(), b.ptr, n_bytes(view_of(out)), stream)); // synchronises the stream
    return out;
}

} // namespace

image_data image_blur(backend_device const* dev, image_view const& src, int radius) {
    require_view("image_blur", src);
    if (src.format != image_format::alpha_f32 && src.format != image_format::rgba_f32)
        throw except("image_blur: unsupported image format [%d], expected alpha_f32 or rgba_f32", int(src.format));
    require_radius("image_blur", radius, src.extent);
    const int C = n_channels(src.format), w = src.extent[0], h = src.extent[1];
    device_scope on(dev);
    image_data packed = image_packed(src);
    device_buffer x = upload(packed, on.stream), tmp(n_bytes(src)), y(n_bytes(src));
    VX(vx_box_blur_f32(static_cast<float*>(x.ptr), (int64_t)w * C, static_cast<float*>(tmp.ptr), static_cast<float*>(y.ptr), (int64_t)w * C, 1, h, w, C, radius, on.stream));
    return download(y, src.extent, src.format, on.stream);
}

image_data image_erosion(backend_device const* dev, image_view const& src, int radius) {
    require_view("image_erosion", src);
    if (src.format != image_format::alpha_u8 && src.format != image_format::alpha_f32)
        throw except("image_erosion: unsupported image format [%d], expected alpha_u8 or alpha_f32", int(src.format));
    if (radius < 1 || radius > 64) throw except("image_erosion: radius %d (1 .. 64)", radius);
    const int w = src.extent[0], h = src.extent[1];
    device_scope on(dev);
    image_data packed = image_packed(src);
    device_buffer x = upload(packed, on.stream), y(n_bytes(src));
    if (src.format == image_format::alpha_u8) VX(vx_erode_u8(static_cast<uint8_t*>(x.ptr), w, static_cast<uint8_t*>(y.ptr), w, 1, h, w, radius, on.stream));
    else VX(vx_erode_f32(static_cast<float*>(x.ptr), w, static_cast<float*>(y.ptr), w, 1, h, w, radius, on.stream));
    return download(y, src.extent, src.format, on.stream);
}

image_data image_alpha_composite(backend_device const* dev, image_view const& fg, image_view const& bg, image_view const& mask) {
    require_view("image_alpha_composite", fg);
    require_view("image_alpha_composite", bg);
    require_view("image_alpha_composite", mask);
    if (fg.format != image_format::rgba_u8) throw except("image_alpha_composite: foreground format [%d], expected rgba_u8", int(fg.format));
    if (bg.format != image_format::rgb_u8 && bg.format != image_format::rgba_u8) throw except("image_alpha_composite: background format [%d], expected rgb_u8 or rgba_u8", int(bg.format));
    if (mask.format != image_format::alpha_u8) throw except("image_alpha_composite: mask format [%d], expected alpha_u8", int(mask.format));
    require_same_extent("image_alpha_composite", fg, bg);
    require_same_extent("image_alpha_composite", fg, mask);
    device_scope on(dev);
    image_data pf = image_packed(fg), pb = image_packed(bg), pm = image_packed(mask);
    device_buffer f = upload(pf, on.stream), b = upload(pb, on.stream), m = upload(pm, on.stream), out(n_bytes(fg));
    VX(vx_alpha_composite_u8(static_cast<uint8_t*>(f.ptr), static_cast<uint8_t*>(b.ptr), n_channels(bg.format), static_cast<uint8_t*>(m.ptr), static_cast<uint8_t*>(out.ptr),
                             (int64_t)fg.extent[0] * fg.extent[1], on.stream));
    return download(out, fg.extent, image_format::rgba_u8, on.stream);
}

void check_foreground_batch(image_format img_format, int B, int w, int h, int radius, image_format out_format) {
    if (img_format != image_format::rgba_f32 && img_format != image_format::rgb_u8 && img_format != image_format::rgba_u8)
        throw except("estimate_foreground: image format [%d], expected rgba_f32, rgb_u8 or rgba_u8", int(img_format));
    if (out_format != image_format::rgba_f32 && out_format != image_format::rgba_u8)
        throw except("estimate_foreground: output format [%d], expected rgba_f32 or rgba_u8", int(out_format));
    if (B < 1 || w < 1 || h < 1) throw except("estimate_foreground: batch %d of %dx%d images", B, w, h);
    if ((int64_t)B * w * h * 8 >= (int64_t(1) << 31)) throw except("estimate_foreground: %d images of %dx%d pass 32-bit indexing", B, w, h);
    require_radius("estimate_foreground", radius, i32x2{{w, h}});
    if (w < 6 || h < 6) throw except("estimate_foreground: extent %dx%d is below the second stage's radius 3", w, h); // blur()'s assertion in stage two
}

size_t foreground_workspace_bytes(int B, int w, int h) { return (size_t)B * w * h * 16 * sizeof(float); }

void estimate_foreground_batch(void const* img, image_format img_format, float const* mask, int B, int w, int h, int radius, void* out, image_format out_format,
                               void* workspace, void* stream) {
    const size_t n = (size_t)B * w * h;
    float* planes = static_cast<float*>(workspace);
    float *fg1 = planes + n * 8, *bg1 = fg1 + n * 4;
    VX(vx_foreground_stage(img, int(img_format), nullptr, nullptr, mask, planes, fg1, int(image_format::rgba_f32), bg1, B, h, w, radius, 3, stream));
    VX(vx_foreground_stage(img, int(img_format), fg1, bg1, mask, planes, out, int(out_format), nullptr, B, h, w, 3, 3, stream));
}

void estimate_foreground_batch_device(backend_device const* dev, void const* img, image_format img_format, float const* mask, int B, int w, int h, int radius, void* out,
                                      image_format out_format, void* stream) {
    if (!img || !mask || !out) throw except("estimate_foreground: null pointer");
    check_foreground_batch(img_format, B, w, h, radius, out_format);
    device_scope on(dev);
    void* s = stream ? stream : on.stream;
    device_buffer ws(foreground_workspace_bytes(B, w, h));
    estimate_foreground_batch(img, img_format, mask, B, w, h, radius, out, out_format, ws.ptr, s);
    VX(vx_stream_sync(s));
}

image_data image_estimate_foreground(backend_device const* dev, image_view const& img, image_view const& mask, int radius) {
    require_view("image_estimate_foreground", img);
    require_view("image_estimate_foreground", mask);
    if (img.format != image_format::rgba_f32) throw except("image_estimate_foreground: image format [%d], expected rgba_f32", int(img.format));
    if (mask.format != image_format::alpha_f32) throw except("image_estimate_foreground: mask format [%d], expected alpha_f32", int(mask.format));
    require_same_extent("image_estimate_foreground", img, mask);
    const int w = img.extent[0], h = img.extent[1];
    check_foreground_batch(img.format, 1, w, h, radius, image_format::rgba_f32);
    device_scope on(dev);
    image_data pi = image_packed(img), pm = image_packed(mask);
    device_buffer i = upload(pi, on.stream), m = upload(pm, on.stream), out(n_bytes(img)), ws(foreground_workspace_bytes(1, w, h));
    estimate_foreground_batch(i.ptr, img.format, static_cast<float*>(m.ptr), 1, w, h, radius, out.ptr, image_format::rgba_f32, ws.ptr, on.stream);
    return download(out, img.extent, image_format::rgba_f32, on.stream);
}

void check_remove_small_regions(int n, int w, int h, int min_area, int mode) {
    if (n < 1) throw except("remove_small_regions: empty batch of masks (n = %d)", n);
    if (w < 1 || h < 1 || (int64_t)w * h > (int64_t(1) << 31) - 256) throw except("remove_small_regions: extent %dx%d", w, h);
    if (min_area < 0) throw except("remove_small_regions: min_area %d is below 0", min_area);
    if (mode < VX_REGIONS_HOLES || mode > VX_REGIONS_BOTH) throw except("remove_small_regions: unknown mode %d (1 holes, 2 islands, 3 both)", mode);
}

void remove_small_regions_device(backend_device const* dev, void* masks_dev, int n, int w, int h, int min_area, int mode, void* changed_dev, void* stream) {
    if (!masks_dev) throw except("remove_small_regions: null pointer");
    check_remove_small_regions(n, w, h, min_area, mode);
    device_scope on(dev);
    void* s = stream ? stream : on.stream;
    const int64_t per_mask = (int64_t)w * h * 8; // labels and areas
    const int group = (int)std::max<int64_t>(1, std::min<int64_t>(n, (int64_t(256) << 20) / per_mask));
    const size_t bytes = vx_mask_regions_workspace_bytes(w, h, group);
    device_buffer ws(bytes);
    VX(vx_mask_remove_small_regions_u8(static_cast<uint8_t*>(masks_dev), w, h, n, nullptr, min_area, mode, static_cast<int32_t*>(changed_dev), ws.ptr, bytes, group, s));
    VX(vx_stream_sync(s));
}

void remove_small_regions_host(backend_device const* dev, uint8_t* masks, int n, int w, int h, int min_area, int mode, int32_t* changed) {
    if (!masks) throw except("remove_small_regions: null pointer");
    check_remove_small_regions(n, w, h, min_area, mode);
    device_scope on(dev);
    const size_t bytes = (size_t)n * w * h;
    device_buffer m(bytes), c((size_t)n * 4);
    VX(vx_memcpy_h2d(m.ptr, masks, bytes, on.stream));
    remove_small_regions_device(dev, m.ptr, n, w, h, min_area, mode, c.ptr, on.stream);
    VX(vx_memcpy_d2h(masks, m.ptr, bytes, on.stream));
    if (changed) VX(vx_memcpy_d2h(changed, c.ptr, (size_t)n * 4, on.stream));
}

void birefnet_cutout_batch_device(birefnet_model& m, void const* rgb_dev, int B, int w, int h, int radius, void* rgba_dev, void* stream) {
    if (!rgb_dev || !rgba_dev) throw except("birefnet cutout: null pointer");
    check_foreground_batch(image_format::rgb_u8, B, w, h, radius, image_format::rgba_u8);
    device_turn turn(*m.backend);
    void* s = stream ? stream : m.backend->stream;
    const size_t mask_bytes = round_up<size_t>((size_t)B * w * h * sizeof(float), 256);
    grow(m.cutout_ws, mask_bytes + foreground_workspace_bytes(B, w, h), {m.backend->stream, s});
    float* mask = static_cast<float*>(m.cutout_ws.ptr);
    birefnet_compute_batch_device(m, rgb_dev, B, w, h, mask, s);
    estimate_foreground_batch(rgb_dev, image_format::rgb_u8, mask, B, w, h, radius, rgba_dev, image_format::rgba_u8, static_cast<uint8_t*>(m.cutout_ws.ptr) + mask_bytes, s);
    if (!stream) VX(vx_stream_sync(s));
}

void birefnet_cutout_batch_host(birefnet_model& m, uint8_t const* rgb, int B, int w, int h, int radius, uint8_t* rgba) {
    if (!rgb || !rgba) throw except("birefnet cutout: null pointer");
    check_foreground_batch(image_format::rgb_u8, B, w, h, radius, image_format::rgba_u8);
    device_turn turn(*m.backend);
    void* s = m.backend->stream;
    const size_t n = (size_t)B * w * h;
    device_buffer in(n * 3), out(n * 4);
    VX(vx_memcpy_h2d(in.ptr, rgb, n * 3, s));
    birefnet_cutout_batch_device(m, in.ptr, B, w, h, radius, out.ptr, s);
    VX(vx_memcpy_d2h(rgba, out.ptr, n * 4, s));
}

image_data birefnet_cutout(birefnet_model& m, image_view image, int radius) {
    if (is_float(image.format) || n_channels(image.format) < 3)
        throw except("birefnet: unsupported input image format [%d], expected an 8-bit colour image", int(image.format));
    require_view("birefnet_cutout", image);
    check_foreground_batch(image_format::rgb_u8, 1, image.extent[0], image.extent[1], radius, image_format::rgba_u8);
    const i32x2 res = birefnet_image_extent(image.extent, m.bparams), extent = image.extent;
    image_data rgb = image_to_rgb_u8(image);
    image_data out = image_alloc(extent, image_format::rgba_u8);
    if (res == extent) { // the image is the network's input: everything stays on the device
        m.bparams.image_extent = res;
        birefnet_cutout_batch_host(m, rgb.data.get(), 1, extent[0], extent[1], radius, out.data.get());
        return out;
    }
    // the mask as birefnet_compute makes it (network at the model's extent, image_scale back: vision.cpp:108-132, birefnet.cpp:272-281), kept in f32; then the
    // estimator on the caller's own pixels at the caller's extent, as the reference's composite_image_with_mask does
    m.bparams.image_extent = res;
    image_data resized = image_scale(image, res);
    image_data rgb_res = image_to_rgb_u8(view_of(resized));
    image_data mask_res = image_alloc(res, image_format::alpha_f32);
    birefnet_compute_batch_host(m, rgb_res.data.get(), 1, res[0], res[1], reinterpret_cast<float*>(mask_res.data.get()));
    image_data mask = image_scale(view_of(mask_res), extent);
    float* mv = reinterpret_cast<float*>(mask.data.get()); // the resize filter overshoots; image_f32_to_u8 clamps at this point in the reference
    for (size_t k = 0, n = (size_t)extent[0] * extent[1]; k < n; ++k) mv[k] = mv[k] < 0.0f ? 0.0f : (mv[k] > 1.0f ? 1.0f : mv[k]);
    device_turn turn(*m.backend);
    void* s = m.backend->stream;
    device_buffer i = upload(rgb, s), mk = upload(mask, s), o(n_bytes(view_of(out))), ws(foreground_workspace_bytes(1, extent[0], extent[1]));
    estimate_foreground_batch(i.ptr, image_format::rgb_u8, static_cast<float*>(mk.ptr), 1, extent[0], extent[1], radius, o.ptr, image_format::rgba_u8, ws.ptr, s);
    return download(o, extent, image_format::rgba_u8, s);
}

} // namespace visp
