// The matting image ops of the public C++ header with the reference's signatures (include/visp/image.h:141-170), on the reference's own test vectors
// (tests/test-image.cpp:205-281), and birefnet_cutout on an image that is not at the model's extent:
// matting_check [<birefnet.gguf> <image rgb_u8 raw> <width> <height> <out rgba_u8 raw>]
#include <array>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "visp/vision.h"

using namespace visp;

static void check_rms(float const* got, float const* want, int n, char const* what) { // CHECK_IMAGES_EQUAL: rms <= 1e-5 (tests/testing.cpp:12)
    double s = 0;
    for (int i = 0; i < n; ++i) s += double(got[i] - want[i]) * double(got[i] - want[i]);
    if (std::sqrt(s / n) > 1e-5) throw exception(std::string(what) + ": rms above 1e-5");
}

int main(int argc, char** argv) {
    if (argc != 1 && argc != 6) {
        fprintf(stderr, "usage: %s [birefnet.gguf image.raw width height out.raw]\n", argv[0]);
        return 2;
    }
    try {
        backend_device b = backend_init(); // makes the device current for this thread: the image ops take none
        { // image_alpha_composite
            std::array<uint8_t, 16> fg_data = {255, 0, 0, 255, 0, 255, 0, 255, 0, 0, 255, 255, 255, 255, 0, 255};
            std::array<uint8_t, 12> bg_data = {0, 0, 0, 128, 128, 128, 255, 255, 255, 64, 64, 64};
            std::array<uint8_t, 4> mask_data = {255, 128, 64, 0};
            std::array<uint8_t, 16> expected = {255, 0, 0, 255, 63, 191, 63, 255, 191, 191, 255, 255, 64, 64, 64, 255};
            image_view fg(i32x2{2, 2}, image_format::rgba_u8, fg_data.data()), bg(i32x2{2, 2}, image_format::rgb_u8, bg_data.data());
            image_view mask(i32x2{2, 2}, image_format::alpha_u8, mask_data.data());
            image_data out = image_alpha_composite(fg, bg, mask);
            if (out.extent != i32x2{2, 2} || out.format != image_format::rgba_u8) throw exception("composite: unexpected output image");
            for (int i = 0; i < 16; ++i)
                if (out.data[i] != expected[i]) throw exception("composite: differs from the reference's vector");
            image_data dst = image_alloc({2, 2}, image_format::rgba_u8);
            image_alpha_composite(fg, bg, mask, image_span(dst));
            for (int i = 0; i < 16; ++i)
                if (dst.data[i] != expected[i]) throw exception("composite into a span: differs from the reference's vector");
            image_data m = image_to_mask(fg); // red channel
            if (m.format != image_format::alpha_u8 || m.data[0] != 255 || m.data[1] != 0 || m.data[3] != 255) throw exception("image_to_mask");
            image_set_alpha(image_span(dst), mask);
            for (int i = 0; i < 4; ++i)
                if (dst.data[4 * i + 3] != mask_data[i] || dst.data[4 * i] != expected[4 * i]) throw exception("image_set_alpha");
        }
        { // image_blur
            std::array<float, 36> input{}, output{};
            for (int i = 0; i < 36; ++i) input[i] = float(i + 1);
            std::array<float, 36> expected = {3.33334f,  4.0f,  5.0f,  6.0f,  7.0f,  7.66667f,  7.33334f,  8.0f,  9.0f,  10.0f, 11.0f, 11.66667f,
                                              13.33334f, 14.0f, 15.0f, 16.0f, 17.0f, 17.66667f, 19.33334f, 20.0f, 21.0f, 22.0f, 23.0f, 23.66667f,
                                              25.33334f, 26.0f, 27.0f, 28.0f, 29.0f, 29.66667f, 29.33334f, 30.0f, 31.0f, 32.0f, 33.0f, 33.66667f};
            image_blur(image_view(i32x2{6, 6}, input), image_span(i32x2{6, 6}, output), 1);
            check_rms(output.data(), expected.data(), 36, "image_blur");
        }
        { // image_erosion
            std::array<float, 36> input = {0.0f, 0.5f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.8f, 0.8f, 1.0f, 0.5f, 0.0f, 1.0f,
                                           0.8f, 0.8f, 1.0f, 0.5f, 0.5f, 0.0f, 0.8f, 1.0f, 1.0f, 0.5f, 0.5f, 0.0f, 0.0f, 1.0f, 1.0f, 0.2f, 0.5f, 0.0f};
            std::array<float, 36> expected = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f,
                                              0.8f, 0.8f, 0.5f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.2f, 0.2f, 0.0f, 0.0f, 0.0f, 0.0f, 0.2f, 0.2f, 0.0f, 0.0f};
            std::array<float, 36> output{};
            image_erosion(image_view(i32x2{6, 6}, input), image_span(i32x2{6, 6}, output), 1);
            for (int i = 0; i < 36; ++i)
                if (output[i] != expected[i]) throw exception("image_erosion: differs from the reference's vector");
        }
        { // image_estimate_foreground: the default radius is the reference's, an opaque mask gives the image back
            const int n = 64 * 64;
            std::vector<float> img(size_t(n) * 4), mask(n, 1.0f);
            for (int i = 0; i < n * 4; ++i) img[i] = float((i * 37) % 101) / 100.0f;
            image_data fg = image_estimate_foreground(image_view(i32x2{64, 64}, image_format::rgba_f32, img.data()), image_view(i32x2{64, 64}, mask));
            if (fg.extent != i32x2{64, 64} || fg.format != image_format::rgba_f32) throw exception("estimate_foreground: unexpected output image");
            float const* f = reinterpret_cast<float const*>(fg.data.get());
            for (int i = 0; i < n; ++i)
                for (int c = 0; c < 4; ++c)
                    if (std::fabs(f[4 * i + c] - (c == 3 ? 1.0f : img[4 * i + c])) > 1e-4f) throw exception("estimate_foreground: opaque mask");
        }
        if (argc == 6) {
            const int w = std::stoi(argv[3]), h = std::stoi(argv[4]);
            std::ifstream in(argv[2], std::ios::binary);
            std::vector<uint8_t> img((std::istreambuf_iterator<char>(in)), {});
            if (img.size() != size_t(w) * h * 3) throw exception("input size does not match the extent");
            birefnet_model model = birefnet_load_model(argv[1], b);
            image_view input(i32x2{w, h}, image_format::rgb_u8, img.data());
            image_data cut = birefnet_cutout(model, input);
            if (cut.extent != input.extent || cut.format != image_format::rgba_u8) throw exception("birefnet_cutout: unexpected output image");
            std::ofstream(argv[5], std::ios::binary).write(reinterpret_cast<char const*>(cut.data.get()), std::streamsize(size_t(w) * h * 4));
        }
        printf("matting-check ok\n");
    } catch (std::exception const& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
