#include "image_scale_device.h"

#include <algorithm>
#include <climits>
#include <cstring>

#include "image_scale_tables.h"
#include "visp_util.h"

namespace visp {

namespace {

using visp_scale::MAX_TAPS;
using visp_scale::TH;

uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

int most_taps(std::vector<taps> const& t) {
    size_t n = 1;
    for (taps const& s : t) n = std::max(n, s.w.size());
    return (int)n;
}

[[noreturn]] void refuse_taps(int in, int out, long n) {
    throw except("image_scale: reducing %d to %d takes %ld taps per output sample, the device kernel holds at most %d (a reduction of about 190:1)", in, out, n, MAX_TAPS);
}

// the unclamped source range [lo, lo + n) the taps of outputs [begin, end) reach
void reach(std::vector<taps> const& t, int begin, int end, int& lo, int& n) {
    int first = INT_MAX, last = INT_MIN;
    for (int i = begin; i < end; ++i) {
        first = std::min(first, t[(size_t)i].first);
        last = std::max(last, t[(size_t)i].first + (int)t[(size_t)i].w.size());
    }
    lo = first;
    n = last - first;
}

int widest_span(std::vector<taps> const& t, int tile) {
    int widest = 1;
    for (int x0 = 0; x0 < (int)t.size(); x0 += tile) {
        int lo, n;
        reach(t, x0, std::min(x0 + tile, (int)t.size()), lo, n);
        widest = std::max(widest, n);
    }
    return widest;
}

} // namespace

void check_image_scale_batch(image_format format, int B, int w, int h, int ow, int oh) {
    if (int(format) < 0 || int(format) > int(image_format::alpha_f32)) throw except("Unsupported image format [%d]", int(format));
    if (B < 1) throw except("image_scale: batch %d must be at least 1", B);
    if (w < 1 || h < 1 || ow < 1 || oh < 1) throw except("Failed to resize image %dx%d to %dx%d", w, h, ow, oh);
    const int64_t ch = n_channels(format);
    if ((int64_t)w * h * ch >= (int64_t(1) << 31) || (int64_t)ow * oh * ch >= (int64_t(1) << 31))
        throw except("image_scale: an image of %dx%d or %dx%d passes 32-bit indexing", w, h, ow, oh);
    // a reducing axis takes about 4 in / out taps; the exact count is checked once the taps exist, this keeps an absurd ratio from building them
    if (((int64_t)4 * w + ow - 1) / ow > MAX_TAPS) refuse_taps(w, ow, (long)(((int64_t)4 * w + ow - 1) / ow));
    if (((int64_t)4 * h + oh - 1) / oh > MAX_TAPS) refuse_taps(h, oh, (long)(((int64_t)4 * h + oh - 1) / oh));
}

image_scale_plan image_scale_make_plan(image_format format, int w, int h, int ow, int oh) {
    check_image_scale_batch(format, 1, w, h, ow, oh);
    const std::vector<taps> tx = axis_taps(w, ow), ty = axis_taps(h, oh);
    image_scale_plan p;
    p.format = format; p.w = w; p.h = h; p.ow = ow; p.oh = oh;
    p.taps_x = most_taps(tx);
    p.taps_y = most_taps(ty);
    if (p.taps_x > MAX_TAPS) refuse_taps(w, ow, p.taps_x);
    if (p.taps_y > MAX_TAPS) refuse_taps(h, oh, p.taps_y);
    // the widest tile whose tables and two row buffers fit: a large reduction narrows it (one column always fits: image_scale_tables.h)
    const int ch = n_channels(format);
    for (p.tile_w = visp_scale::TW; p.tile_w >= 1; p.tile_w /= 2) {
        p.span = widest_span(tx, p.tile_w);
        if (visp_scale::lds_words(ch, is_float(format), p.tile_w, p.taps_x, p.taps_y, p.span) * 4 <= (size_t)visp_scale::LDS_BUDGET) break;
    }
    VISP_ASSERT(p.tile_w >= 1);

    const visp_scale::table_layout l = visp_scale::layout(ow, oh, p.tile_w, p.taps_x, p.taps_y);
    p.words.assign(l.total, 0u);
    uint32_t* T = p.words.data();
    const float* srgb = srgb_to_linear_table();
    for (int i = 0; i < 256; ++i) {
        T[i] = bits(srgb[i]);
        T[256 + i] = bits((float)i / 255.0f);
    }
    memcpy(T + 512, linear_to_srgb_table(), 104 * sizeof(uint32_t));
    for (int x = 0; x < ow; ++x) {
        taps const& t = tx[(size_t)x];
        T[l.xfirst + x] = (uint32_t)t.first;
        T[l.xcount + x] = (uint32_t)t.w.size();
        uint32_t* tile = T + l.xw + (size_t)(x / p.tile_w) * p.taps_x * p.tile_w + x % p.tile_w;
        for (size_t i = 0; i < t.w.size(); ++i) tile[i * p.tile_w] = bits(t.w[i]);
    }
    for (int k = 0; k < l.tiles_x; ++k) {
        int lo, n;
        reach(tx, k * p.tile_w, std::min((k + 1) * p.tile_w, ow), lo, n);
        T[l.tile_xlo + k] = (uint32_t)lo;
        T[l.tile_span + k] = (uint32_t)n;
    }
    for (int y = 0; y < oh; ++y) {
        taps const& t = ty[(size_t)y];
        T[l.yfirst + y] = (uint32_t)t.first;
        T[l.ycount + y] = (uint32_t)t.w.size();
        for (size_t i = 0; i < t.w.size(); ++i) T[l.yw + (size_t)y * p.taps_y + i] = bits(t.w[i]);
    }
    for (int k = 0; k < l.tiles_y; ++k) {
        int lo, n;
        reach(ty, k * TH, std::min((k + 1) * TH, oh), lo, n);
        T[l.band_lo + k] = (uint32_t)lo;
        T[l.band_n + k] = (uint32_t)n;
    }
    return p;
}

void image_scale_upload(image_scale_plan& p, void* stream) {
    p.tables = device_buffer(p.words.size() * 4);
    VX(vx_memcpy_h2d(p.tables.ptr, p.words.data(), p.words.size() * 4, stream));
}

void image_scale_run(image_scale_plan const& p, void const* src, int B, void* dst, void* stream) {
    VX(vx_image_scale(src, int(p.format), B, p.h, p.w, dst, p.oh, p.ow, p.tables.ptr, p.words.size() * 4, p.tile_w, p.taps_x, p.taps_y, p.span, stream));
}

void image_scale_batch_device(backend_device const* dev, void const* src, image_format format, int B, int w, int h, void* dst, int ow, int oh, void* stream) {
    if (!src || !dst) throw except("image_scale: null pointer");
    check_image_scale_batch(format, B, w, h, ow, oh);
    image_scale_plan plan = image_scale_make_plan(format, w, h, ow, oh);
    device_scope on(dev);
    void* s = stream ? stream : on.stream;
    image_scale_upload(plan, s);
    image_scale_run(plan, src, B, dst, s);
    VX(vx_stream_sync(s)); // the tables are freed behind this
}

void image_scale_batch_host(backend_device const* dev, void const* src, image_format format, int B, int w, int h, void* dst, int ow, int oh) {
    if (!src || !dst) throw except("image_scale: null pointer");
    check_image_scale_batch(format, B, w, h, ow, oh);
    image_scale_plan plan = image_scale_make_plan(format, w, h, ow, oh);
    device_scope on(dev);
    const size_t px = (size_t)n_bytes(format), in_bytes = (size_t)B * h * w * px, out_bytes = (size_t)B * oh * ow * px;
    device_buffer in(in_bytes), out(out_bytes);
    VX(vx_memcpy_h2d(in.ptr, src, in_bytes, on.stream));
    image_scale_upload(plan, on.stream);
    image_scale_run(plan, in.ptr, B, out.ptr, on.stream);
    VX(vx_memcpy_d2h(dst, out.ptr, out_bytes, on.stream)); // synchronises the stream
}

} // namespace visp
