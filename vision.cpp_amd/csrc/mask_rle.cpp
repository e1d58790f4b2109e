#include "mask_rle.h"

#include <algorithm>
#include <cmath>

#include "visp_util.h"

namespace visp {

namespace {

constexpr int kRleGroup = 256;                      // masks in flight through the boundary words (32 MB at 1024^2)
constexpr int64_t kRlePassBytes = int64_t(256) << 20; // runs on the device in one encode pass of the host entries

// Device masks [n, h, w] -> CSR on the host. A count-only pass and one readback of the counts; their running sum, uploaded, lets the encode write every mask's runs
// right behind the previous mask's (vx_mask_rle_packed_u8), so exactly the runs cross to the host, in one copy per pass straight into the result. A pass holds at
// most kRlePassBytes of runs on the device (a single mask with more has a pass of its own). counts_dev (nullable) cuts the masks to its first entry, which the count
// pass's readback brings along into counts_host [n_counts].
// `sink(b0, b1, rows_dev, offsets_dev, rel)` takes each pass's rows off the device: masks b0 .. b1, rel their offsets from 0.
template <class Sink>
void encode_passes(uint8_t const* masks_dev, int n, int w, int h, int32_t const* counts_dev, int32_t* counts_host, int n_counts, int64_t* offsets, void* s, Sink&& sink) {
    const int group = std::min(n, kRleGroup);
    const size_t ws_bytes = vx_mask_rle_workspace_bytes(w, h, group);
    device_buffer ws(ws_bytes), nr((size_t)n * 4);
    int32_t* nr_dev = static_cast<int32_t*>(nr.ptr);
    VX(vx_mask_rle_u8(masks_dev, w, h, n, counts_dev, nullptr, 0, nr_dev, ws.ptr, ws_bytes, group, s));
    if (counts_dev) VX(vx_memcpy_d2h(counts_host, counts_dev, (size_t)n_counts * 4, s));
    std::vector<int32_t> n_runs((size_t)n);
    VX(vx_memcpy_d2h(n_runs.data(), nr_dev, (size_t)n * 4, s));
    VX(vx_stream_sync(s));
    const int k = counts_dev ? std::min(std::max(counts_host[0], 0), n) : n;
    offsets[0] = 0;
    for (int b = 0; b < n; ++b) offsets[b + 1] = offsets[b] + (b < k ? n_runs[(size_t)b] : 0);
    device_buffer rows, off_dev;
    std::vector<int64_t> rel;
    for (int b0 = 0, b1; b0 < k; b0 = b1) {
        for (b1 = b0 + 1; b1 < k && (offsets[b1 + 1] - offsets[b0]) * 4 <= kRlePassBytes; ++b1) {}
        rel.assign(offsets + b0, offsets + b1 + 1);
        for (int64_t& v : rel) v -= offsets[b0];
        grow(rows, (size_t)rel.back() * 4, {s});
        grow(off_dev, rel.size() * 8, {s});
        VX(vx_memcpy_h2d(off_dev.ptr, rel.data(), rel.size() * 8, s));
        VX(vx_mask_rle_packed_u8(masks_dev + (size_t)b0 * w * h, w, h, b1 - b0, static_cast<int64_t const*>(off_dev.ptr), static_cast<uint32_t*>(rows.ptr), nr_dev + b0, ws.ptr,
                                 ws_bytes, group, s));
        sink(b0, b1, static_cast<uint32_t const*>(rows.ptr), static_cast<int64_t const*>(off_dev.ptr), rel);
    }
}

std::vector<uint32_t> encode_to_host(uint8_t const* masks_dev, int n, int w, int h, int32_t const* counts_dev, int32_t* counts_host, int n_counts, int64_t* offsets, void* s) {
    std::vector<uint32_t> out;
    encode_passes(masks_dev, n, w, h, counts_dev, counts_host, n_counts, offsets, s, [&](int b0, int, uint32_t const* rows_dev, int64_t const*, std::vector<int64_t> const& rel) {
        out.resize((size_t)offsets[n]);
        VX(vx_memcpy_d2h(out.data() + offsets[b0], rows_dev, (size_t)rel.back() * 4, s));
        VX(vx_stream_sync(s));
    });
    return out;
}

constexpr int kCodecGroup = 65535; // records of one launch of the codec

// Device CSR rows (off_dev [n + 1], `off` the same values on the host) -> their strings appended to `out`, byte_offsets[1 .. n] continued from byte_offsets[0].
// The compressor's count pass, one readback of the sizes, their running sum uploaded, the write pass, one copy of the bytes: per group of kCodecGroup records.
void compress_rows(uint32_t const* runs_dev, int64_t const* off_dev, int64_t const* off, int n, std::vector<uint8_t>& out, int64_t* byte_offsets, void* s) {
    device_buffer ws, sizes_dev, boff_dev, bytes_dev;
    std::vector<int32_t> sizes;
    std::vector<int64_t> brel;
    for (int g0 = 0; g0 < n; g0 += kCodecGroup) {
        const int g = std::min(kCodecGroup, n - g0);
        const int64_t total = off[g0 + g] - off[g0];
        int64_t longest = 0;
        for (int b = g0; b < g0 + g; ++b) longest = std::max(longest, off[b + 1] - off[b]);
        const size_t ws_bytes = vx_rle_compress_workspace_bytes(total, g);
        if (!ws_bytes) throw except("rle_compress: %lld runs in the %d records from %d: too many for one pass", (long long)total, g, g0);
        grow(ws, ws_bytes, {s});
        grow(sizes_dev, (size_t)g * 4, {s});
        VX(vx_rle_compress(runs_dev, off_dev + g0, total, longest, g, nullptr, 0, nullptr, nullptr, static_cast<int32_t*>(sizes_dev.ptr), ws.ptr, ws_bytes, s));
        sizes.resize((size_t)g);
        VX(vx_memcpy_d2h(sizes.data(), sizes_dev.ptr, (size_t)g * 4, s));
        VX(vx_stream_sync(s));
        brel.assign((size_t)g + 1, 0);
        for (int b = 0; b < g; ++b) brel[(size_t)b + 1] = brel[(size_t)b] + sizes[(size_t)b];
        grow(boff_dev, brel.size() * 8, {s});
        grow(bytes_dev, std::max<size_t>((size_t)brel.back(), 16), {s});
        VX(vx_memcpy_h2d(boff_dev.ptr, brel.data(), brel.size() * 8, s));
        VX(vx_rle_compress(runs_dev, off_dev + g0, total, longest, g, nullptr, 0, static_cast<uint8_t*>(bytes_dev.ptr), static_cast<int64_t const*>(boff_dev.ptr), nullptr, ws.ptr,
                           ws_bytes, s));
        const size_t at = out.size();
        out.resize(at + (size_t)brel.back());
        if (brel.back()) VX(vx_memcpy_d2h(out.data() + at, bytes_dev.ptr, (size_t)brel.back(), s));
        VX(vx_stream_sync(s));
        for (int b = 0; b < g; ++b) byte_offsets[g0 + b + 1] = byte_offsets[g0] + brel[(size_t)b + 1];
    }
}

// masks on the device -> strings on the host: each encode pass's rows go through the compressor while they are on the device
std::vector<uint8_t> encode_compressed_to_host(uint8_t const* masks_dev, int n, int w, int h, int32_t const* counts_dev, int32_t* counts_host, int n_counts, int64_t* byte_offsets,
                                               void* s) {
    std::vector<int64_t> offsets((size_t)n + 1);
    std::vector<uint8_t> out;
    byte_offsets[0] = 0;
    encode_passes(masks_dev, n, w, h, counts_dev, counts_host, n_counts, offsets.data(), s,
                  [&](int b0, int b1, uint32_t const* rows_dev, int64_t const* off_dev, std::vector<int64_t> const& rel) {
                      compress_rows(rows_dev, off_dev, rel.data(), b1 - b0, out, byte_offsets + b0, s);
                  });
    const int k = counts_dev ? std::min(std::max(counts_host[0], 0), n) : n;
    for (int b = k; b < n; ++b) byte_offsets[b + 1] = byte_offsets[b]; // no pass reaches the masks behind the count
    return out;
}

} // namespace

void check_rle_encode(int n, int w, int h, int64_t run_stride) {
    if (n < 1) throw except("rle_encode: empty batch of masks (n = %d)", n);
    if (w < 1 || h < 1 || (int64_t)w * h >= (int64_t(1) << 31) - 1) throw except("rle_encode: extent %dx%d", w, h);
    if (run_stride < 0) throw except("rle_encode: run_stride %lld is below 0", (long long)run_stride);
}

void rle_encode_device(backend_device const* dev, void const* masks_dev, int n, int w, int h, void const* counts_dev, void* runs_dev, int64_t run_stride, void* n_runs_dev,
                       void* stream) {
    if (!masks_dev || !n_runs_dev) throw except("rle_encode: null pointer");
    check_rle_encode(n, w, h, run_stride);
    device_scope on(dev);
    void* s = stream ? stream : on.stream;
    const int group = std::min(n, kRleGroup);
    const size_t bytes = vx_mask_rle_workspace_bytes(w, h, group);
    device_buffer ws(bytes);
    VX(vx_mask_rle_u8(static_cast<uint8_t const*>(masks_dev), w, h, n, static_cast<int32_t const*>(counts_dev), static_cast<uint32_t*>(runs_dev), run_stride,
                      static_cast<int32_t*>(n_runs_dev), ws.ptr, bytes, group, s));
    VX(vx_stream_sync(s));
}

std::vector<uint32_t> rle_encode_host(backend_device const* dev, uint8_t const* masks, int n, int w, int h, int64_t* offsets) {
    if (!masks || !offsets) throw except("rle_encode: null pointer");
    check_rle_encode(n, w, h, 0);
    device_scope on(dev);
    const size_t bytes = (size_t)n * w * h;
    device_buffer m(bytes);
    VX(vx_memcpy_h2d(m.ptr, masks, bytes, on.stream));
    return encode_to_host(static_cast<uint8_t const*>(m.ptr), n, w, h, nullptr, nullptr, 0, offsets, on.stream);
}

namespace {

// the generate call into the model's staging buffer, `encode` of its masks behind it on the same stream, then the info rows of the masks returned
template <class Out, class Encode>
std::vector<Out> generate_encoded(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, sam_select_params const& p, int32_t* info_i32, float* info_f32,
                                  int32_t* counts, int64_t* offsets, Encode&& encode) {
    if (!info_i32 || !info_f32 || !counts || !offsets) throw except("sam: null argument");
    device_turn turn(*m.backend);
    void* s = m.backend->stream;
    const int w = m.image_extent[0], h = m.image_extent[1];
    workspace_layout lay;
    const size_t o_m = lay.take((size_t)p.capacity * w * h), o_i = lay.take((size_t)p.capacity * 32), o_f = lay.take((size_t)p.capacity * 8), o_c = lay.take(16);
    grow(m.generate_rle_stage, lay.top, {s});
    uint8_t* base = static_cast<uint8_t*>(m.generate_rle_stage.ptr);
    sam_generate_masks_device(m, prompts, n_args, n, p, {base + o_m, base + o_i, base + o_f, base + o_c}, s); // checks the model: decoder, encoded image
    const int n_counts = p.min_region_area > 0 ? 4 : 2;
    std::vector<Out> runs = encode(base + o_m, p.capacity, w, h, reinterpret_cast<int32_t const*>(base + o_c), counts, n_counts, offsets, s);
    const size_t k = (size_t)std::min(std::max(counts[0], 0), p.capacity); // rows behind the returned ones stay as the caller left them
    if (k) {
        VX(vx_memcpy_d2h(info_i32, base + o_i, k * 32, s));
        VX(vx_memcpy_d2h(info_f32, base + o_f, k * 8, s));
        VX(vx_stream_sync(s));
    }
    return runs;
}

} // namespace

std::vector<uint32_t> sam_generate_masks_rle_host(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, sam_select_params const& p, int32_t* info_i32,
                                                  float* info_f32, int32_t* counts, int64_t* offsets) {
    return generate_encoded<uint32_t>(m, prompts, n_args, n, p, info_i32, info_f32, counts, offsets, encode_to_host);
}

std::vector<uint8_t> sam_generate_masks_coco_rle_host(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, sam_select_params const& p, int32_t* info_i32,
                                                      float* info_f32, int32_t* counts, int64_t* byte_offsets) {
    return generate_encoded<uint8_t>(m, prompts, n_args, n, p, info_i32, info_f32, counts, byte_offsets, encode_compressed_to_host);
}

// ---- the way back: decode, area, IoU ----

namespace {

// the offsets of n device rows on the host, held to be non-decreasing before anything is launched on them
std::vector<int64_t> read_offsets(char const* who, void const* offsets_dev, int n, void* s) {
    std::vector<int64_t> off((size_t)n + 1);
    VX(vx_memcpy_d2h(off.data(), offsets_dev, off.size() * 8, s));
    VX(vx_stream_sync(s));
    for (int b = 0; b < n; ++b)
        if (off[(size_t)b + 1] < off[(size_t)b]) throw except("%s: offsets decrease at row %d (%lld then %lld)", who, b, (long long)off[(size_t)b], (long long)off[(size_t)b + 1]);
    return off;
}

void decode_on(uint32_t const* runs_dev, int64_t const* offsets_dev, std::vector<int64_t> const& off, int n, int w, int h, int32_t const* counts_dev, int value,
               uint8_t* masks_dev, int32_t* status_dev, int64_t* area_dev, void* s) {
    const int group = std::min(n, kRleGroup);
    int64_t most = 0; // runs of the largest group
    for (int b0 = 0; b0 < n; b0 += group) most = std::max(most, off[(size_t)std::min(n, b0 + group)] - off[(size_t)b0]);
    const size_t pos_bytes = vx_rle_to_bits_workspace_bytes(most, group);
    device_buffer words((size_t)group * vx_mask_rle_workspace_bytes(w, h, 1)), pos(pos_bytes);
    for (int b0 = 0; b0 < n; b0 += group) {
        const int g = std::min(group, n - b0);
        VX(vx_rle_to_bits(runs_dev, offsets_dev + b0, off[(size_t)b0 + g] - off[(size_t)b0], g, w, h, counts_dev, b0, words.ptr, area_dev ? area_dev + b0 : nullptr,
                          status_dev ? status_dev + b0 : nullptr, pos.ptr, pos_bytes, s));
        VX(vx_bits_to_mask_u8(words.ptr, g, w, h, counts_dev, b0, value, masks_dev + (size_t)b0 * w * h, s));
    }
    VX(vx_stream_sync(s));
}

// a host array on the device (at least 16 bytes, so that an empty one still has an address)
device_buffer uploaded(void const* host, size_t bytes, void* s) {
    device_buffer d(std::max<size_t>(bytes, 16));
    if (bytes) VX(vx_memcpy_h2d(d.ptr, host, bytes, s));
    return d;
}

// one side of an IoU call, on the device, as bit words
device_buffer words_of(char const* who, mask_set const& d, void* s) {
    device_buffer words((size_t)d.n * vx_mask_rle_workspace_bytes(d.w, d.h, 1));
    if (d.masks) {
        VX(vx_mask_to_bits_u8(static_cast<uint8_t const*>(d.masks), d.n, d.w, d.h, nullptr, 0, words.ptr, s));
        return words;
    }
    const std::vector<int64_t> off = read_offsets(who, d.offsets, d.n, s);
    const int64_t total = off.back() - off.front();
    const size_t pos_bytes = vx_rle_to_bits_workspace_bytes(total, d.n);
    device_buffer pos(pos_bytes);
    VX(vx_rle_to_bits(static_cast<uint32_t const*>(d.runs), static_cast<int64_t const*>(d.offsets), total, d.n, d.w, d.h, nullptr, 0, words.ptr, nullptr, nullptr, pos.ptr,
                      pos_bytes, s));
    VX(vx_stream_sync(s)); // the positions are freed behind this
    return words;
}

void iou_on(mask_set const& a, mask_set const& b, void const* iscrowd_dev, void* iou_dev, void* inter_dev, void* s) {
    device_buffer wa = words_of("mask_iou", a, s), wb = words_of("mask_iou", b, s);
    const size_t bytes = vx_bitmask_iou_workspace_bytes(a.n, b.n);
    device_buffer areas(bytes);
    VX(vx_bitmask_iou(wa.ptr, a.n, wb.ptr, b.n, a.w, a.h, nullptr, nullptr, static_cast<uint8_t const*>(iscrowd_dev), static_cast<int32_t*>(inter_dev),
                      static_cast<float*>(iou_dev), areas.ptr, bytes, s));
    VX(vx_stream_sync(s));
}

// a host side of an IoU call moved to the device; `keep` owns what was uploaded
mask_set side_uploaded(mask_set const& d, std::vector<device_buffer>& keep, void* s) {
    mask_set out = d;
    if (d.masks) {
        keep.push_back(uploaded(d.masks, (size_t)d.n * d.w * d.h, s));
        out.masks = keep.back().ptr;
        return out;
    }
    int64_t const* off = static_cast<int64_t const*>(d.offsets);
    keep.push_back(uploaded(static_cast<uint32_t const*>(d.runs) + off[0], (size_t)(off[d.n] - off[0]) * 4, s));
    out.runs = keep.back().ptr;
    std::vector<int64_t> rel(off, off + d.n + 1);
    for (int64_t& v : rel) v -= off[0];
    keep.push_back(uploaded(rel.data(), rel.size() * 8, s));
    VX(vx_stream_sync(s)); // rel leaves scope
    out.offsets = keep.back().ptr;
    return out;
}

} // namespace

void check_rle_extent(char const* who, int n, int w, int h) {
    if (n < 1 || n > 65535) throw except("%s: %d masks (1 .. 65535)", who, n);
    if (w < 1 || h < 1 || (int64_t)w * h >= (int64_t(1) << 31) - 1) throw except("%s: extent %dx%d", who, w, h);
}

void check_rle_rows(char const* who, int64_t const* offsets, uint32_t const* runs, int n, int64_t hw) {
    for (int b = 0; b < n; ++b) {
        if (offsets[b + 1] < offsets[b] || offsets[b] < 0) throw except("%s: offsets decrease at row %d", who, b);
        int64_t sum = 0;
        for (int64_t i = offsets[b]; i < offsets[b + 1]; ++i) sum += runs[i];
        if (hw >= 0 && sum != hw) throw except("%s: the runs of row %d sum to %lld, the extent has %lld pixels", who, b, (long long)sum, (long long)hw);
    }
}

void rle_decode_device(backend_device const* dev, void const* runs_dev, void const* offsets_dev, int n, int w, int h, void const* counts_dev, int value, void* masks_dev,
                       void* status_dev, void* area_dev, void* stream) {
    if (!runs_dev || !offsets_dev || !masks_dev) throw except("rle_decode: null pointer");
    check_rle_extent("rle_decode", n, w, h);
    if (value < 1 || value > 255) throw except("rle_decode: foreground value %d (1 .. 255)", value);
    device_scope on(dev);
    void* s = stream ? stream : on.stream;
    decode_on(static_cast<uint32_t const*>(runs_dev), static_cast<int64_t const*>(offsets_dev), read_offsets("rle_decode", offsets_dev, n, s), n, w, h,
              static_cast<int32_t const*>(counts_dev), value, static_cast<uint8_t*>(masks_dev), static_cast<int32_t*>(status_dev), static_cast<int64_t*>(area_dev), s);
}

void rle_decode_host(backend_device const* dev, int64_t const* offsets, uint32_t const* runs, int n, int w, int h, int value, uint8_t* masks) {
    if (!offsets || !runs || !masks) throw except("rle_decode: null pointer");
    check_rle_extent("rle_decode", n, w, h);
    if (value < 1 || value > 255) throw except("rle_decode: foreground value %d (1 .. 255)", value);
    check_rle_rows("rle_decode", offsets, runs, n, (int64_t)w * h);
    device_scope on(dev);
    void* s = on.stream;
    std::vector<int64_t> rel(offsets, offsets + n + 1);
    for (int64_t& v : rel) v -= offsets[0];
    device_buffer r = uploaded(runs + offsets[0], (size_t)rel.back() * 4, s), o = uploaded(rel.data(), rel.size() * 8, s);
    const size_t bytes = (size_t)n * w * h;
    device_buffer m(bytes);
    decode_on(static_cast<uint32_t const*>(r.ptr), static_cast<int64_t const*>(o.ptr), rel, n, w, h, nullptr, value, static_cast<uint8_t*>(m.ptr), nullptr, nullptr, s);
    VX(vx_memcpy_d2h(masks, m.ptr, bytes, s));
    VX(vx_stream_sync(s));
}

void rle_area_host(int64_t const* offsets, uint32_t const* runs, int n, int64_t* area) {
    if (!offsets || !runs || !area) throw except("rle_area: null pointer");
    if (n < 1) throw except("rle_area: empty batch of rows (n = %d)", n);
    check_rle_rows("rle_area", offsets, runs, n, -1);
    for (int b = 0; b < n; ++b) {
        area[b] = 0;
        for (int64_t i = offsets[b] + 1; i < offsets[b + 1]; i += 2) area[b] += runs[i];
    }
}

void check_mask_iou(char const* who, mask_set const& a, mask_set const& b) {
    for (mask_set const* d : {&a, &b}) {
        if (d->masks ? (d->runs || d->offsets) : (!d->runs || !d->offsets)) throw except("%s: each side is u8 masks, or runs with offsets: null pointer, or both forms", who);
        check_rle_extent(who, d->n, d->w, d->h);
    }
    if (a.w != b.w || a.h != b.h) throw except("%s: the extents differ, %dx%d and %dx%d", who, a.w, a.h, b.w, b.h);
}

void mask_iou_device(backend_device const* dev, mask_set const& a, mask_set const& b, void const* iscrowd_dev, void* iou_dev, void* inter_dev, void* stream) {
    check_mask_iou("mask_iou", a, b);
    if (!iou_dev) throw except("mask_iou: null pointer");
    device_scope on(dev);
    iou_on(a, b, iscrowd_dev, iou_dev, inter_dev, stream ? stream : on.stream);
}

void mask_iou_host(backend_device const* dev, mask_set const& a, mask_set const& b, uint8_t const* iscrowd, float* iou, int32_t* inter) {
    check_mask_iou("mask_iou", a, b);
    if (!iou) throw except("mask_iou: null pointer");
    for (mask_set const* d : {&a, &b})
        if (!d->masks) check_rle_rows("mask_iou", static_cast<int64_t const*>(d->offsets), static_cast<uint32_t const*>(d->runs), d->n, (int64_t)d->w * d->h);
    device_scope on(dev);
    void* s = on.stream;
    std::vector<device_buffer> keep;
    const mask_set da = side_uploaded(a, keep, s), db = side_uploaded(b, keep, s);
    const size_t pairs = (size_t)a.n * b.n;
    device_buffer crowd, out(pairs * 4), out_inter(pairs * 4);
    if (iscrowd) crowd = uploaded(iscrowd, (size_t)b.n, s);
    iou_on(da, db, crowd.ptr, out.ptr, out_inter.ptr, s);
    VX(vx_memcpy_d2h(iou, out.ptr, pairs * 4, s));
    if (inter) VX(vx_memcpy_d2h(inter, out_inter.ptr, pairs * 4, s));
    VX(vx_stream_sync(s));
}

// ---- COCO's compressed counts strings (kernels_rle_codec.hip) ----

void check_rle_codec(char const* who, int n) {
    if (n < 1 || n > 65535) throw except("%s: %d records (1 .. 65535)", who, n);
}

rle_string_fault check_rle_strings(int64_t const* byte_offsets, uint8_t const* bytes, int n) {
    for (int b = 0; b < n; ++b) {
        if (byte_offsets[b + 1] < byte_offsets[b] || byte_offsets[b] < 0) throw except("rle_decompress: byte offsets decrease at record %d", b);
        const int64_t begin = byte_offsets[b], end = byte_offsets[b + 1];
        int64_t chain[2] = {0, 0}, i = 0; // c[i - 2] by the parity of i
        for (int64_t p = begin; p < end; ++i) {
            int64_t x = 0;
            int k = 0;
            for (bool more = true; more; ++k, ++p) {
                if (p == end) return {b, end - 1 - begin, 2};
                const int g = bytes[p] - 48;
                if (g < 0 || g > 63) return {b, p - begin, 1};
                if (k == 7) return {b, p - begin, 3};
                x |= int64_t(g & 31) << (5 * k);
                more = g & 32;
                if (!more && (g & 16)) x -= int64_t(1) << (5 * (k + 1)); // the sign above the bits read
            }
            if (i > 2) x += chain[i & 1];
            if (x < 0 || x > 0x7fffffffLL) return {b, p - 1 - begin, 4};
            chain[i & 1] = x;
        }
    }
    return {-1, 0, 0};
}

void rle_compress_device(backend_device const* dev, void const* runs_dev, void const* offsets_dev, int n, void const* counts_dev, void* bytes_dev, void const* byte_offsets_dev,
                         void* sizes_dev, void* stream) {
    if (!runs_dev || !offsets_dev || (bytes_dev ? !byte_offsets_dev : !sizes_dev)) throw except("rle_compress: null pointer");
    check_rle_codec("rle_compress", n);
    device_scope on(dev);
    void* s = stream ? stream : on.stream;
    const std::vector<int64_t> off = read_offsets("rle_compress", offsets_dev, n, s);
    int64_t longest = 0;
    for (int b = 0; b < n; ++b) longest = std::max(longest, off[(size_t)b + 1] - off[(size_t)b]);
    const int64_t total = off.back() - off.front();
    const size_t ws_bytes = vx_rle_compress_workspace_bytes(total, n);
    if (!ws_bytes) throw except("rle_compress: %lld runs: too many for one call", (long long)total);
    device_buffer ws(ws_bytes);
    VX(vx_rle_compress(static_cast<uint32_t const*>(runs_dev), static_cast<int64_t const*>(offsets_dev), total, longest, n, static_cast<int32_t const*>(counts_dev), 0,
                       static_cast<uint8_t*>(bytes_dev), static_cast<int64_t const*>(byte_offsets_dev), static_cast<int32_t*>(sizes_dev), ws.ptr, ws_bytes, s));
    VX(vx_stream_sync(s)); // the workspace is freed behind this
}

std::vector<uint8_t> rle_compress_host(backend_device const* dev, int64_t const* offsets, uint32_t const* runs, int n, int64_t* byte_offsets) {
    if (!offsets || !runs || !byte_offsets) throw except("rle_compress: null pointer");
    check_rle_codec("rle_compress", n);
    check_rle_rows("rle_compress", offsets, runs, n, -1);
    for (int b = 0; b < n; ++b)
        for (int64_t i = offsets[b]; i < offsets[b + 1]; ++i)
            if (runs[i] >= 0x80000000u) throw except("rle_compress: run %lld of record %d is %u, at or above 2^31", (long long)(i - offsets[b]), b, runs[i]);
    device_scope on(dev);
    void* s = on.stream;
    std::vector<int64_t> rel(offsets, offsets + n + 1);
    for (int64_t& v : rel) v -= offsets[0];
    device_buffer r = uploaded(runs + offsets[0], (size_t)rel.back() * 4, s), o = uploaded(rel.data(), rel.size() * 8, s);
    std::vector<uint8_t> out;
    byte_offsets[0] = 0;
    compress_rows(static_cast<uint32_t const*>(r.ptr), static_cast<int64_t const*>(o.ptr), rel.data(), n, out, byte_offsets, s);
    return out;
}

void rle_decompress_device(backend_device const* dev, void const* bytes_dev, void const* byte_offsets_dev, int n, void const* counts_dev, void* runs_dev,
                           void const* offsets_dev, void* sizes_dev, void* status_dev, void* stream) {
    if (!bytes_dev || !byte_offsets_dev || (runs_dev ? !offsets_dev : !sizes_dev)) throw except("rle_decompress: null pointer");
    check_rle_codec("rle_decompress", n);
    device_scope on(dev);
    void* s = stream ? stream : on.stream;
    VX(vx_rle_decompress(static_cast<uint8_t const*>(bytes_dev), static_cast<int64_t const*>(byte_offsets_dev), n, static_cast<int32_t const*>(counts_dev), 0,
                         static_cast<uint32_t*>(runs_dev), static_cast<int64_t const*>(offsets_dev), static_cast<int32_t*>(sizes_dev), static_cast<int32_t*>(status_dev), s));
    VX(vx_stream_sync(s));
}

std::vector<uint32_t> rle_decompress_host(backend_device const* dev, int64_t const* byte_offsets, uint8_t const* bytes, int n, int64_t* offsets) {
    if (!byte_offsets || !bytes || !offsets) throw except("rle_decompress: null pointer");
    check_rle_codec("rle_decompress", n);
    const rle_string_fault bad = check_rle_strings(byte_offsets, bytes, n);
    if (bad.status) {
        static char const* const what[] = {"", "a byte outside 48 .. 111", "the last byte has bit 5 set (unterminated)", "a value of more than 7 bytes", "a count outside 0 .. 2^31 - 1"};
        throw except("rle_decompress: record %d, byte %lld: status %d, %s", bad.record, (long long)bad.byte, bad.status, what[bad.status]);
    }
    device_scope on(dev);
    void* s = on.stream;
    std::vector<int64_t> brel(byte_offsets, byte_offsets + n + 1);
    for (int64_t& v : brel) v -= byte_offsets[0];
    device_buffer src = uploaded(bytes + byte_offsets[0], (size_t)brel.back(), s), bo = uploaded(brel.data(), brel.size() * 8, s), sizes_dev((size_t)n * 4);
    uint8_t const* src_dev = static_cast<uint8_t const*>(src.ptr);
    int64_t const* bo_dev = static_cast<int64_t const*>(bo.ptr);
    VX(vx_rle_decompress(src_dev, bo_dev, n, nullptr, 0, nullptr, nullptr, static_cast<int32_t*>(sizes_dev.ptr), nullptr, s));
    std::vector<int32_t> sizes((size_t)n);
    VX(vx_memcpy_d2h(sizes.data(), sizes_dev.ptr, (size_t)n * 4, s));
    VX(vx_stream_sync(s));
    offsets[0] = 0;
    for (int b = 0; b < n; ++b) offsets[b + 1] = offsets[b] + sizes[(size_t)b];
    std::vector<uint32_t> out((size_t)offsets[n]);
    device_buffer o = uploaded(offsets, ((size_t)n + 1) * 8, s), rows(std::max<size_t>(out.size() * 4, 16)), st((size_t)n * 4);
    VX(vx_rle_decompress(src_dev, bo_dev, n, nullptr, 0, static_cast<uint32_t*>(rows.ptr), static_cast<int64_t const*>(o.ptr), nullptr, static_cast<int32_t*>(st.ptr), s));
    std::vector<int32_t> status((size_t)n);
    VX(vx_memcpy_d2h(status.data(), st.ptr, (size_t)n * 4, s));
    if (!out.empty()) VX(vx_memcpy_d2h(out.data(), rows.ptr, out.size() * 4, s));
    VX(vx_stream_sync(s));
    for (int b = 0; b < n; ++b)
        if (status[(size_t)b]) throw except("rle_decompress: record %d: the device reports status %d on a string the host check passed", b, status[(size_t)b]);
    return out;
}

std::vector<uint8_t> rle_encode_compressed_host(backend_device const* dev, uint8_t const* masks, int n, int w, int h, int64_t* byte_offsets) {
    if (!masks || !byte_offsets) throw except("rle_encode: null pointer");
    check_rle_encode(n, w, h, 0);
    device_scope on(dev);
    const size_t bytes = (size_t)n * w * h;
    device_buffer m(bytes);
    VX(vx_memcpy_h2d(m.ptr, masks, bytes, on.stream));
    return encode_compressed_to_host(static_cast<uint8_t const*>(m.ptr), n, w, h, nullptr, nullptr, 0, byte_offsets, on.stream);
}

// ---- polygons and boxes to records, merged records, boxes of records (kernels_rle_poly.hip) ----

std::vector<uint32_t> poly_rle_reference(double const* xy, int64_t k, int w, int h) {
    std::vector<int> x((size_t)k + 1), y((size_t)k + 1), u, v;
    for (int64_t j = 0; j < k; ++j) {
        x[(size_t)j] = (int)(5.0 * xy[2 * j] + 0.5);
        y[(size_t)j] = (int)(5.0 * xy[2 * j + 1] + 0.5);
    }
    x[(size_t)k] = x[0];
    y[(size_t)k] = y[0];
    for (int64_t j = 0; j < k; ++j) {
        int xs = x[(size_t)j], xe = x[(size_t)j + 1], ys = y[(size_t)j], ye = y[(size_t)j + 1];
        const int dx = std::abs(xe - xs), dy = std::abs(ys - ye);
        const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
        if (flip) {
            std::swap(xs, xe);
            std::swap(ys, ye);
        }
        if (dx == 0 && dy == 0) { // a single point; its v is never read below
            u.push_back(xs);
            v.push_back(ys);
            continue;
        }
        const double s = dx >= dy ? (double)(ye - ys) / dx : (double)(xe - xs) / dy;
        if (dx >= dy) {
            for (int d = 0; d <= dx; ++d) {
                const int t = flip ? dx - d : d;
                u.push_back(t + xs);
                v.push_back((int)(ys + s * t + 0.5));
            }
        } else {
            for (int d = 0; d <= dy; ++d) {
                const int t = flip ? dy - d : d;
                v.push_back(t + ys);
                u.push_back((int)(xs + s * t + 0.5));
            }
        }
    }
    std::vector<uint32_t> a;
    for (size_t j = 1; j < u.size(); ++j) {
        if (u[j] == u[j - 1]) continue;
        double xd = (double)(u[j] < u[j - 1] ? u[j] : u[j] - 1);
        xd = (xd + 0.5) / 5.0 - 0.5;
        if (std::floor(xd) != xd || xd < 0 || xd > w - 1) continue;
        double yd = (double)(v[j] < v[j - 1] ? v[j] : v[j - 1]);
        yd = (yd + 0.5) / 5.0 - 0.5;
        if (yd < 0) yd = 0;
        else if (yd > h) yd = h;
        yd = std::ceil(yd);
        a.push_back((uint32_t)((int)xd * h + (int)yd));
    }
    a.push_back((uint32_t)((int64_t)h * w));
    std::sort(a.begin(), a.end());
    uint32_t p = 0;
    for (uint32_t& t : a) {
        const uint32_t key = t;
        t -= p;
        p = key;
    }
    std::vector<uint32_t> b{a[0]};
    for (size_t i = 1; i < a.size();) {
        if (a[i] > 0) {
            b.push_back(a[i++]);
        } else {
            ++i;
            if (i < a.size()) b.back() += a[i++];
        }
    }
    return b;
}

int64_t check_polygons(char const* who, double const* xy, int64_t const* poly_offsets, int n, int w, int h) {
    check_rle_extent(who, n, w, h);
    int64_t longest = 0;
    for (int b = 0; b < n; ++b) {
        if (poly_offsets[b] < 0 || poly_offsets[b + 1] < poly_offsets[b]) throw except("%s: offsets decrease at polygon %d", who, b);
        if (poly_offsets[b + 1] == poly_offsets[b]) throw except("%s: polygon %d has no vertex", who, b);
        const int64_t k = poly_offsets[b + 1] - poly_offsets[b];
        double const* p = xy + 2 * poly_offsets[b];
        for (int64_t j = 0; j < 2 * k; ++j)
            if (!(std::fabs(p[j]) <= 1048576.0)) throw except("%s: polygon %d, vertex %lld: coordinate %g is not finite or beyond 2^20", who, b, (long long)(j / 2), p[j]);
        int64_t points = 0;
        for (int64_t j = 0; j < k; ++j) {
            const int64_t j1 = j + 1 < k ? j + 1 : 0;
            const int dx = std::abs((int)(5.0 * p[2 * j1] + 0.5) - (int)(5.0 * p[2 * j] + 0.5)), dy = std::abs((int)(5.0 * p[2 * j1 + 1] + 0.5) - (int)(5.0 * p[2 * j + 1] + 0.5));
            points += std::max(dx, dy) + 1;
        }
        if (points >= (int64_t(1) << 31)) throw except("%s: polygon %d walks %lld points, at or above 2^31", who, b, (long long)points);
        longest = std::max(longest, points);
    }
    return longest;
}

namespace {

// vx_poly_rle on device polygons: the sizing form and one readback of {M, K + 1} per polygon when made, then the forms with keys as often as asked
struct poly_pass {
    double const* xy;
    int64_t const* poff;
    int64_t total_vertices, max_points = 0, total_keys = 0;
    int n, w, h;
    int32_t const* counts;
    void* s;
    size_t ws_bytes = 0;
    device_buffer ws, keys;

    poly_pass(void const* xy_dev, void const* poff_dev, int64_t total_vertices, int n, int w, int h, void const* counts_dev, void* status_dev, void* s)
        : xy(static_cast<double const*>(xy_dev)), poff(static_cast<int64_t const*>(poff_dev)), total_vertices(total_vertices), n(n), w(w), h(h),
          counts(static_cast<int32_t const*>(counts_dev)), s(s) {
        size_t bytes = vx_poly_rle_workspace_bytes(total_vertices, n, 0);
        if (!bytes) throw except("rle_from_poly: %lld vertices in %d polygons: no workspace", (long long)total_vertices, n);
        std::vector<int64_t> mk((size_t)n * 2, 0);
        device_buffer first(bytes), mk_dev(mk.size() * 8);
        VX(vx_memcpy_h2d(mk_dev.ptr, mk.data(), mk.size() * 8, s)); // a polygon behind the device count stays {0, 0}
        VX(vx_poly_rle(xy, poff, total_vertices, 0, n, w, h, counts, 0, nullptr, 0, nullptr, nullptr, nullptr, static_cast<int64_t*>(mk_dev.ptr),
                       static_cast<int32_t*>(status_dev), first.ptr, bytes, s));
        VX(vx_memcpy_d2h(mk.data(), mk_dev.ptr, mk.size() * 8, s));
        VX(vx_stream_sync(s));
        for (int b = 0; b < n; ++b) {
            max_points = std::max(max_points, mk[(size_t)b * 2]);
            total_keys += vx_poly_rle_key_row(mk[(size_t)b * 2 + 1]);
        }
        ws_bytes = vx_poly_rle_workspace_bytes(total_vertices, n, max_points);
        grow(ws, ws_bytes, {s});
        grow(keys, std::max<size_t>((size_t)total_keys * 4, 16), {s});
    }
    void run(void* runs_dev, void const* offsets_dev, void* sizes_dev, void* status_dev) {
        VX(vx_poly_rle(xy, poff, total_vertices, max_points, n, w, h, counts, 0, static_cast<uint32_t*>(keys.ptr), total_keys, static_cast<uint32_t*>(runs_dev),
                       static_cast<int64_t const*>(offsets_dev), static_cast<int32_t*>(sizes_dev), nullptr, static_cast<int32_t*>(status_dev), ws.ptr, ws_bytes, s));
    }
};

// host rows held to their offsets, then on the device: the runs from offsets[0] on and the offsets from 0
struct uploaded_rows {
    std::vector<int64_t> rel;
    device_buffer runs, offsets;
    uploaded_rows(int64_t const* off, uint32_t const* r, int n, void* s) : rel(off, off + n + 1) {
        for (int64_t& v : rel) v -= off[0];
        runs = uploaded(r + off[0], (size_t)rel.back() * 4, s);
        offsets = uploaded(rel.data(), rel.size() * 8, s);
    }
};

void check_groups(char const* who, int64_t const* group_offsets, int groups, int n) {
    for (int g = 0; g < groups; ++g)
        if (group_offsets[g] < 0 || group_offsets[g + 1] < group_offsets[g] || group_offsets[g + 1] > n)
            throw except("%s: group %d is records %lld .. %lld of %d", who, g, (long long)group_offsets[g], (long long)group_offsets[g + 1], n);
}

// device records -> the groups' masks u8 [groups, h, w] on the device; `off` the records' offsets on the host
void merge_on(uint32_t const* runs_dev, int64_t const* offsets_dev, std::vector<int64_t> const& off, int n, int64_t const* group_offsets_dev, int groups, int w, int h,
              int intersect, int value, uint8_t* masks_dev, void* s) {
    const size_t per = vx_mask_rle_workspace_bytes(w, h, 1);
    const int64_t total = off.back() - off.front();
    const size_t pos_bytes = vx_rle_to_bits_workspace_bytes(total, n);
    device_buffer words((size_t)n * per), merged((size_t)groups * per), pos(pos_bytes);
    VX(vx_rle_to_bits(runs_dev, offsets_dev, total, n, w, h, nullptr, 0, words.ptr, nullptr, nullptr, pos.ptr, pos_bytes, s));
    VX(vx_bits_merge(words.ptr, n, group_offsets_dev, groups, w, h, intersect, merged.ptr, s));
    VX(vx_bits_to_mask_u8(merged.ptr, groups, w, h, nullptr, 0, value, masks_dev, s));
    VX(vx_stream_sync(s)); // the words are freed behind this
}

} // namespace

void rle_from_poly_device(backend_device const* dev, void const* xy_dev, void const* poly_offsets_dev, int n, int w, int h, void const* counts_dev, void* runs_dev,
                          void const* offsets_dev, void* sizes_dev, void* status_dev, void* stream) {
    if (!xy_dev || !poly_offsets_dev || (runs_dev ? !offsets_dev : !sizes_dev)) throw except("rle_from_poly: null pointer");
    check_rle_extent("rle_from_poly", n, w, h);
    device_scope on(dev);
    void* s = stream ? stream : on.stream;
    const std::vector<int64_t> poff = read_offsets("rle_from_poly", poly_offsets_dev, n, s);
    if (poff.back() == poff.front()) throw except("rle_from_poly: no vertex in %d polygons", n);
    poly_pass pass(xy_dev, poly_offsets_dev, poff.back() - poff.front(), n, w, h, counts_dev, status_dev, s);
    pass.run(runs_dev, offsets_dev, sizes_dev, status_dev);
    VX(vx_stream_sync(s)); // the workspaces are freed behind this
}

std::vector<uint32_t> rle_from_poly_host(backend_device const* dev, double const* xy, int64_t const* poly_offsets, int n, int w, int h, int64_t* offsets) {
    if (!xy || !poly_offsets || !offsets) throw except("rle_from_poly: null pointer");
    check_polygons("rle_from_poly", xy, poly_offsets, n, w, h);
    device_scope on(dev);
    void* s = on.stream;
    std::vector<int64_t> rel(poly_offsets, poly_offsets + n + 1);
    for (int64_t& v : rel) v -= poly_offsets[0];
    device_buffer xy_dev = uploaded(xy + 2 * poly_offsets[0], (size_t)rel.back() * 16, s), poff_dev = uploaded(rel.data(), rel.size() * 8, s), sizes_dev((size_t)n * 4),
                  st_dev((size_t)n * 4);
    poly_pass pass(xy_dev.ptr, poff_dev.ptr, rel.back(), n, w, h, nullptr, nullptr, s);
    pass.run(nullptr, nullptr, sizes_dev.ptr, st_dev.ptr);
    std::vector<int32_t> sizes((size_t)n), status((size_t)n);
    VX(vx_memcpy_d2h(sizes.data(), sizes_dev.ptr, (size_t)n * 4, s));
    VX(vx_memcpy_d2h(status.data(), st_dev.ptr, (size_t)n * 4, s));
    VX(vx_stream_sync(s));
    offsets[0] = 0;
    for (int b = 0; b < n; ++b) {
        if (status[(size_t)b]) throw except("rle_from_poly: polygon %d: the device reports status %d on input the host check passed", b, status[(size_t)b]);
        offsets[b + 1] = offsets[b] + sizes[(size_t)b];
    }
    std::vector<uint32_t> out((size_t)offsets[n]);
    device_buffer o = uploaded(offsets, ((size_t)n + 1) * 8, s), rows(std::max<size_t>(out.size() * 4, 16));
    pass.run(rows.ptr, o.ptr, nullptr, nullptr);
    if (!out.empty()) VX(vx_memcpy_d2h(out.data(), rows.ptr, out.size() * 4, s));
    VX(vx_stream_sync(s));
    return out;
}

std::vector<uint32_t> rle_from_bbox_host(backend_device const* dev, double const* boxes, int n, int w, int h, int64_t* offsets) {
    if (!boxes || !offsets) throw except("rle_from_bbox: null pointer");
    check_rle_extent("rle_from_bbox", n, w, h);
    std::vector<double> xy((size_t)n * 8);
    std::vector<int64_t> poff((size_t)n + 1);
    for (int b = 0; b < n; ++b) {
        const double x = boxes[4 * b], y = boxes[4 * b + 1], xe = x + boxes[4 * b + 2], ye = y + boxes[4 * b + 3];
        const double ring[8] = {x, y, x, ye, xe, ye, xe, y};
        std::copy(ring, ring + 8, xy.begin() + (size_t)b * 8);
        poff[(size_t)b + 1] = 4 * ((int64_t)b + 1);
    }
    check_polygons("rle_from_bbox", xy.data(), poff.data(), n, w, h);
    return rle_from_poly_host(dev, xy.data(), poff.data(), n, w, h, offsets);
}

void check_rle_merge(char const* who, int n, int groups, int w, int h) {
    check_rle_extent(who, n, w, h);
    if (groups < 1 || groups > 65535) throw except("%s: %d groups (1 .. 65535)", who, groups);
}

void rle_merge_device(backend_device const* dev, void const* runs_dev, void const* offsets_dev, int n, void const* group_offsets_dev, int groups, int w, int h, int intersect,
                      int value, void* masks_dev, void* stream) {
    if (!runs_dev || !offsets_dev || !group_offsets_dev || !masks_dev) throw except("rle_merge: null pointer");
    check_rle_merge("rle_merge", n, groups, w, h);
    if (value < 1 || value > 255) throw except("rle_merge: foreground value %d (1 .. 255)", value);
    device_scope on(dev);
    void* s = stream ? stream : on.stream;
    const std::vector<int64_t> off = read_offsets("rle_merge", offsets_dev, n, s), goff = read_offsets("rle_merge", group_offsets_dev, groups, s);
    check_groups("rle_merge", goff.data(), groups, n);
    merge_on(static_cast<uint32_t const*>(runs_dev), static_cast<int64_t const*>(offsets_dev), off, n, static_cast<int64_t const*>(group_offsets_dev), groups, w, h, intersect,
             value, static_cast<uint8_t*>(masks_dev), s);
}

std::vector<uint32_t> rle_merge_host(backend_device const* dev, int64_t const* offsets, uint32_t const* runs, int n, int64_t const* group_offsets, int groups, int w, int h,
                                     int intersect, int64_t* out_offsets) {
    if (!offsets || !runs || !group_offsets || !out_offsets) throw except("rle_merge: null pointer");
    check_rle_merge("rle_merge", n, groups, w, h);
    check_rle_rows("rle_merge", offsets, runs, n, (int64_t)w * h);
    check_groups("rle_merge", group_offsets, groups, n);
    device_scope on(dev);
    void* s = on.stream;
    uploaded_rows rows(offsets, runs, n, s);
    device_buffer g = uploaded(group_offsets, ((size_t)groups + 1) * 8, s), masks((size_t)groups * w * h);
    merge_on(static_cast<uint32_t const*>(rows.runs.ptr), static_cast<int64_t const*>(rows.offsets.ptr), rows.rel, n, static_cast<int64_t const*>(g.ptr), groups, w, h, intersect,
             1, static_cast<uint8_t*>(masks.ptr), s);
    return encode_to_host(static_cast<uint8_t const*>(masks.ptr), groups, w, h, nullptr, nullptr, 0, out_offsets, s);
}

void rle_to_bbox_device(backend_device const* dev, void const* runs_dev, void const* offsets_dev, int n, int w, int h, void const* counts_dev, void* boxes_dev, void* stream) {
    if (!runs_dev || !offsets_dev || !boxes_dev) throw except("rle_to_bbox: null pointer");
    check_rle_extent("rle_to_bbox", n, w, h);
    device_scope on(dev);
    void* s = stream ? stream : on.stream;
    const std::vector<int64_t> off = read_offsets("rle_to_bbox", offsets_dev, n, s);
    VX(vx_rle_bbox(static_cast<uint32_t const*>(runs_dev), static_cast<int64_t const*>(offsets_dev), off.back() - off.front(), n, w, h, static_cast<int32_t const*>(counts_dev), 0,
                   static_cast<int32_t*>(boxes_dev), s));
    VX(vx_stream_sync(s));
}

void rle_to_bbox_host(backend_device const* dev, int64_t const* offsets, uint32_t const* runs, int n, int w, int h, int32_t* boxes) {
    if (!offsets || !runs || !boxes) throw except("rle_to_bbox: null pointer");
    check_rle_extent("rle_to_bbox", n, w, h);
    check_rle_rows("rle_to_bbox", offsets, runs, n, -1);
    device_scope on(dev);
    void* s = on.stream;
    uploaded_rows rows(offsets, runs, n, s);
    device_buffer out((size_t)n * 16);
    VX(vx_rle_bbox(static_cast<uint32_t const*>(rows.runs.ptr), static_cast<int64_t const*>(rows.offsets.ptr), rows.rel.back(), n, w, h, nullptr, 0, static_cast<int32_t*>(out.ptr),
                   s));
    VX(vx_memcpy_d2h(boxes, out.ptr, (size_t)n * 16, s));
    VX(vx_stream_sync(s));
}

} // namespace visp
