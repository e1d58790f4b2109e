// The host side of the device image_scale (kernels_imgscale.hip behind vx_image_scale): the tables of one (format, extent -> extent), how they
// are packed, and the launch. image.h declares the entries that own their tables for one call; a model that scales on its own stream keeps plans.
#pragma once
#include "image.h"
#include "model.h"

namespace visp {

struct image_scale_plan {
    image_format format = image_format::rgb_u8;
    int w = 0, h = 0, ow = 0, oh = 0;
    int tile_w = 0, taps_x = 0, taps_y = 0, span = 0; // the output columns of a block, the padded tap counts, the widest source span of a tile
    std::vector<uint32_t> words;                      // the tables as the kernel reads them (image_scale_tables.h); kept: the upload reads them
    device_buffer tables;                             // their device copy
    bool serves(image_format f, int w_, int h_, int ow_, int oh_) const { return tables.ptr && f == format && w_ == w && h_ == h && ow_ == ow && oh_ == oh; }
};

// throws what image_scale_batch_device refuses, touches no device: format, batch and extents below 1, images past 32-bit indexing, a reduction
// whose taps pass the kernel's limit (image_scale_tables.h MAX_TAPS per output sample and axis)
void check_image_scale_batch(image_format format, int B, int w, int h, int ow, int oh);
// host only: the checks above, axis_taps per axis, the widest tile whose tables and row buffers fit the LDS budget, the packed block
image_scale_plan image_scale_make_plan(image_format format, int w, int h, int ow, int oh);
void image_scale_upload(image_scale_plan& p, void* stream); // allocates the device copy and enqueues the transfer
// one launch on stream, no synchronisation: src [B, h, w, ch] -> dst [B, oh, ow, ch], device pointers
void image_scale_run(image_scale_plan const& p, void const* src, int B, void* dst, void* stream);

} // namespace visp
