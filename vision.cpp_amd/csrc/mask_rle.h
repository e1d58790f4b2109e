// COCO's uncompressed RLE of u8 masks on the device (vx_mask_rle_u8, kernels_rle.hip): the primitive on device and host arrays, and the generate call of
// MobileSAM with RLE records instead of mask bytes. Host C++ only. Every argument check runs before anything touches a device.
#pragma once
#include <vector>

#include "model.h"
#include "tinyvit.h"

namespace visp {

void check_rle_encode(int n, int w, int h, int64_t run_stride); // throws, touches no device
// masks u8 [n, h, w] -> runs u32 [n, run_stride] (nullable: count only) and n_runs i32 [n], all on the device; counts_dev (nullable): only the first counts[0]
// masks. The workspace (one bit per pixel, at most 256 masks in flight) is allocated for the CALL and freed behind a synchronisation of the stream.
void rle_encode_device(backend_device const* dev, void const* masks_dev, int n, int w, int h, void const* counts_dev, void* runs_dev, int64_t run_stride, void* n_runs_dev,
                       void* stream);
// host masks -> the runs of all masks one behind the other; offsets i64 [n + 1]: mask b's runs are [offsets[b], offsets[b + 1])
std::vector<uint32_t> rle_encode_host(backend_device const* dev, uint8_t const* masks, int n, int w, int h, int64_t* offsets);
// sam_generate_masks_device into a staging buffer of the model, the first counts[0] masks encoded behind it on the same stream; info_i32 [capacity][8],
// info_f32 [capacity][2], counts [2 or 4] as sam_generate_masks_host returns them, offsets i64 [capacity + 1] (entries behind counts[0] repeat the last one).
// No mask byte crosses to the host.
std::vector<uint32_t> sam_generate_masks_rle_host(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, sam_select_params const& p, int32_t* info_i32,
                                                  float* info_f32, int32_t* counts, int64_t* offsets);

} // namespace visp
