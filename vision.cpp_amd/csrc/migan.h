// MI-GAN inpainting on the MI355X backend: model load (GGUF -> one packed weight arena), the generator as a hand schedule of
// kernels_migan.hip launches and 1x1 GEMMs, replayed as a hipGraph per batch size. Host C++ only; all device work goes through
// the vx_* C ABI (include/visp_hip_kernels.h).
//
// Mirrors the reference's API for this family (include/visp/vision.h:257-279; src/visp/vision.cpp:172-203;
// src/visp/arch/migan.cpp).
#pragma once
#include <map>
#include <memory>
#include <vector>

#include "gguf.h"
#include "image.h"
#include "model.h"

namespace visp {

struct migan_params { // vision.h:263-266
    int resolution = 256;
    bool invert_mask = true;
};
migan_params migan_detect_params(model_file const&); // migan.cpp:161-169

// separable_conv_2d (migan.cpp:53-82) of one file: offsets into the weight arena
struct migan_sep {
    int res = 0, cin = 0, cout = 0; // extent of the depthwise conv's input; channels in / out
    size_t dw_w = SIZE_MAX, dw_b = SIZE_MAX; // f16 [9][cin], f32 [cin]
    size_t down = SIZE_MAX;                  // f32 [16][cin] or none
    packed_gemm pw;                          // f16 [cout][cin]: the 1x1 conv (no bias)
    size_t up = SIZE_MAX;                    // f32 [16][cout] or none
    size_t noise = SIZE_MAX;                 // f32 [out res]^2 = noise_const * noise_strength, or none
};
struct migan_level {
    int res = 0, ch = 0;
    migan_sep enc1, enc2, syn1, syn2;
    size_t torgb_w = SIZE_MAX, torgb_b = SIZE_MAX, img_up = SIZE_MAX; // f32 [3][ch], [3]; f32 [16][3] (levels above 4)
};

struct migan_model : model_base { // vision.h:371-375 counterpart
    migan_model() : model_base(family_migan) {}
    migan_params params;
    std::vector<migan_level> levels; // [0] = resolution ... [n-1] = 4
    size_t fromrgb_w = SIZE_MAX, fromrgb_b = SIZE_MAX; // f32 [ch0][4], [ch0]
    device_buffer weight_arena;
    device_buffer ws;
    int ws_batch = 0;
    std::map<int, captured_graph> graphs; // batch size -> captured launch list of the u8 -> rgba path (one stream, no branches)
};

migan_model* migan_load_model(char const* filepath, backend_device const& dev);

// B images (3 or 4 u8 channels) + B alpha_u8 masks at resolution^2 on the device -> rgba_u8 [B, res, res, 4] on the device
void migan_compute_batch_device(migan_model&, void const* img_dev, int img_channels, void const* mask_dev, int batch, void* out_rgba_dev,
                                void* stream);
void migan_compute_batch_host(migan_model&, uint8_t const* img, int img_channels, uint8_t const* mask, int batch, uint8_t* out_rgba);
// the generator on migan_process_input's f32 [n, res, res, 4] (host) -> rgb f32 [n, res, res, 3] (host): parity tests
void migan_generate_host(migan_model&, float const* in4, int n, float* out_rgb);
// reference API (vision.cpp:172-203): any extent, image rgb/rgba u8 + alpha_u8 mask -> rgba_u8 at the image's extent
image_data migan_compute(migan_model&, image_view image, image_view mask);

} // namespace visp
