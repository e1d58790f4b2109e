// The matting image ops of the reference's image.h that compute on the device (image_blur, image_erosion, image_estimate_foreground,
// image_alpha_composite; src/visp/image.cpp:358-535) and the BiRefNet cutout built on the estimator. Host C++ only: the kernels are
// kernels_matting.hip behind the vx_* launchers. Every argument check of the host-view functions runs before anything touches a device.
#pragma once
#include "birefnet.h"
#include "image.h"
#include "model.h"

namespace visp {

// Host views in, host image out. dev == nullptr: the calling thread's current HIP device and its default stream.
image_data image_blur(backend_device const* dev, image_view const& src, int radius);       // alpha_f32 / rgba_f32
image_data image_erosion(backend_device const* dev, image_view const& src, int radius);    // alpha_u8 / alpha_f32
image_data image_estimate_foreground(backend_device const* dev, image_view const& img, image_view const& mask, int radius); // rgba_f32, alpha_f32 -> rgba_f32
image_data image_alpha_composite(backend_device const* dev, image_view const& fg, image_view const& bg, image_view const& mask); // -> rgba_u8

// The estimator's two stages (radius, then 3) on device-resident batches: img [B, h, w] rgba_f32 / rgb_u8 / rgba_u8, mask f32 [B, h, w]
// -> out rgba_f32 / rgba_u8. The u8 image is read where it lies: no f32 copy of it exists.
void check_foreground_batch(image_format img_format, int B, int w, int h, int radius, image_format out_format); // formats, extents, radius: throws, touches no device
size_t foreground_workspace_bytes(int B, int w, int h); // planes [.., 8] + stage one's foreground and background [.., 4] each, f32
void estimate_foreground_batch(void const* img, image_format img_format, float const* mask, int B, int w, int h, int radius, void* out, image_format out_format,
                               void* workspace, void* stream); // enqueues four launches, no synchronisation
// with a workspace of its own for the call: returns after the stream has been synchronised (the workspace is freed behind it)
void estimate_foreground_batch_device(backend_device const* dev, void const* img, image_format img_format, float const* mask, int B, int w, int h, int radius, void* out,
                                      image_format out_format, void* stream);

// SAM's remove_small_regions on n u8 masks [n, h, w] (non-zero = foreground; vx_mask_remove_small_regions_u8): mode 1 fills the holes, 2 removes the islands, 3 both in
// that order; changed i32 [n], nullable. The labelling workspace is allocated for the CALL (at most 256 MB: the masks pass through it in groups) and freed behind
// a synchronisation of the stream, so both entries return with the work done.
void check_remove_small_regions(int n, int w, int h, int min_area, int mode); // throws, touches no device
void remove_small_regions_device(backend_device const* dev, void* masks_dev, int n, int w, int h, int min_area, int mode, void* changed_dev, void* stream);
void remove_small_regions_host(backend_device const* dev, uint8_t* masks, int n, int w, int h, int min_area, int mode, int32_t* changed);

// birefnet_compute_batch_device as it stands, then the estimator on the mask where it lies: rgb_u8 [B, h, w, 3] -> rgba_u8 [B, h, w, 4] cutout
void birefnet_cutout_batch_device(birefnet_model& m, void const* rgb_dev, int B, int w, int h, int radius, void* rgba_dev, void* stream);
void birefnet_cutout_batch_host(birefnet_model& m, uint8_t const* rgb, int B, int w, int h, int radius, uint8_t* rgba);
// any 8-bit colour image of any extent -> rgba_u8 cutout at its extent (the network and the estimator run at the model's extent)
image_data birefnet_cutout(birefnet_model& m, image_view image, int radius);

} // namespace visp
