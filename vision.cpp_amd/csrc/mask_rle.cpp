#include "mask_rle.h"

#include <algorithm>

#include "visp_util.h"

namespace visp {

namespace {

constexpr int kRleGroup = 256;                      // masks in flight through the boundary words (32 MB at 1024^2)
constexpr int64_t kRlePassBytes = int64_t(256) << 20; // runs on the device in one encode pass of the host entries

// Device masks [n, h, w] -> CSR on the host. A count-only pass and one readback of the counts; their running sum, uploaded, lets the encode write every mask's runs
// right behind the previous mask's (vx_mask_rle_packed_u8), so exactly the runs cross to the host, in one copy per pass straight into the result. A pass holds at
// most kRlePassBytes of runs on the device (a single mask with more has a pass of its own). counts_dev (nullable) cuts the masks to its first entry, which the count
// pass's readback brings along into counts_host [n_counts].
std::vector<uint32_t> encode_to_host(uint8_t const* masks_dev, int n, int w, int h, int32_t const* counts_dev, int32_t* counts_host, int n_counts, int64_t* offsets, void* s) {
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
    std::vector<uint32_t> out((size_t)offsets[n]);
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
        VX(vx_memcpy_d2h(out.data() + offsets[b0], rows.ptr, (size_t)rel.back() * 4, s));
        VX(vx_stream_sync(s));
    }
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

std::vector<uint32_t> sam_generate_masks_rle_host(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, sam_select_params const& p, int32_t* info_i32,
                                                  float* info_f32, int32_t* counts, int64_t* offsets) {
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
    std::vector<uint32_t> runs = encode_to_host(base + o_m, p.capacity, w, h, reinterpret_cast<int32_t const*>(base + o_c), counts, n_counts, offsets, s);
    const size_t k = (size_t)std::min(std::max(counts[0], 0), p.capacity); // rows behind the returned ones stay as the caller left them
    if (k) {
        VX(vx_memcpy_d2h(info_i32, base + o_i, k * 32, s));
        VX(vx_memcpy_d2h(info_f32, base + o_f, k * 8, s));
        VX(vx_stream_sync(s));
    }
    return runs;
}

} // namespace visp
