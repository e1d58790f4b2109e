// Shaped like the reference's tests/test-models.cpp:89-100 (migan_load_model -> migan_compute) against the public C++ header:
// migan_check <model.gguf> <image rgb_u8 raw> <mask alpha_u8 raw> <width> <height> <out rgba_u8 raw>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "visp/vision.h"

using namespace visp;

static std::vector<uint8_t> read_file(char const* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), {});
}

int main(int argc, char** argv) {
    if (argc != 7) {
        fprintf(stderr, "usage: %s model.gguf image.raw mask.raw width height out.raw\n", argv[0]);
        return 2;
    }
    try {
        const int w = std::stoi(argv[4]), h = std::stoi(argv[5]);
        std::vector<uint8_t> img = read_file(argv[2]), mask = read_file(argv[3]);
        if (img.size() != size_t(w) * h * 3 || mask.size() != size_t(w) * h) throw exception("input sizes do not match the extent");
        backend_device b = backend_init();
        migan_model model = migan_load_model(argv[1], b);
        migan_params p = migan_detect_params(model);
        image_view input(i32x2{w, h}, image_format::rgb_u8, img.data());
        image_view mask_view(i32x2{w, h}, image_format::alpha_u8, mask.data());
        image_data output = migan_compute(model, input, mask_view);
        if (output.extent != input.extent || output.format != image_format::rgba_u8) throw exception("unexpected output image");
        for (size_t i = 0; i < mask.size(); ++i)
            if (output.data[i * 4 + 3] != mask[i]) throw exception("output alpha differs from the mask");
        image_data x = migan_process_input(input, mask_view, p); // the pipeline pieces compile and agree on the extent
        if (x.extent != i32x2{p.resolution, p.resolution}) throw exception("process_input extent");
        std::ofstream(argv[6], std::ios::binary).write(reinterpret_cast<char const*>(output.data.get()), std::streamsize(size_t(w) * h * 4));
        printf("migan-check ok (resolution %d)\n", p.resolution);
    } catch (std::exception const& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
