// Shaped like the reference's src/cli/inference_yolov9t.cpp:300-405 (load -> letterbox -> detect) against the public C++ header:
// yolov9t_check <model.gguf> <image rgb_u8 raw> <width> <height> <out detections raw>
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
    if (argc != 6) {
        fprintf(stderr, "usage: %s model.gguf image.raw width height out.raw\n", argv[0]);
        return 2;
    }
    try {
        const int w = std::stoi(argv[3]), h = std::stoi(argv[4]);
        std::vector<uint8_t> img = read_file(argv[2]);
        if (img.size() != size_t(w) * h * 3) throw exception("input size does not match the extent");
        backend_device b = backend_init();
        yolov9t::yolov9t_model model = yolov9t::yolov9t_load_model(argv[1], b);
        yolov9t::yolov9t_params p = yolov9t::yolov9t_detect_params(model);
        image_view input(i32x2{w, h}, image_format::rgb_u8, img.data());
        yolov9t::LetterboxResult lb = yolov9t::letterbox(input, p.input_size);
        if (lb.img.extent != i32x2{p.input_size, p.input_size} || lb.gain <= 0) throw exception("letterbox extent");
        std::vector<yolov9t::detected_obj> dets = yolov9t::yolov9t_detect(model, input, yolov9t::NMSParams{});
        for (auto const& d : dets)
            if (d.x1 < 0 || d.x2 > w || d.y1 < 0 || d.y2 > h || d.class_id < 0 || d.class_id >= p.num_classes) throw exception("detection out of range");
        std::ofstream(argv[5], std::ios::binary).write(reinterpret_cast<char const*>(dets.data()), std::streamsize(dets.size() * sizeof(dets[0])));
        printf("yolov9t-check ok (%zu detections, %d classes)\n", dets.size(), p.num_classes);
    } catch (std::exception const& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
