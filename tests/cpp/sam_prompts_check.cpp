// The two batched prompt overloads of include/visp/vision.h, sam_compute_batch(points) and sam_compute_batch(boxes), compiled and linked against
// the library, and run on a MobileSAM file given on the command line:
//   sam_prompts_check <mobile_sam.gguf> <width> <height>
// A gradient image of that extent is encoded once; three points and two boxes go through the batched calls and, one by one, through sam_compute.
// Prints "<masks> masks <w>x<h> differing <pixels>": the pixels on which the batched masks and the single-prompt masks differ, over all five.
// Built by __graft_entry__.build(); tests/test_gpu_sam_prompts.py runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "visp/vision.h"

using namespace visp;

int main(int argc, char** argv) {
    try {
        if (argc != 4) throw exception("usage: sam_prompts_check <mobile_sam.gguf> <width> <height>");
        const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
        backend_device dev = backend_init();
        sam_model model = sam_load_model(argv[1], dev);
        image_data img = image_alloc({w, h}, image_format::rgb_u8);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                uint8_t* px = img.data.get() + (size_t(y) * w + x) * 3;
                px[0] = uint8_t(x * 255 / w), px[1] = uint8_t(y * 255 / h), px[2] = uint8_t((x ^ y) & 255);
            }
        sam_encode(model, image_view(img));
        std::vector<i32x2> points = {{w / 2, h / 2}, {w / 4, h / 3}, {3, h - 4}};
        std::vector<box_2d> boxes = {{{w / 8, h / 8}, {w / 2, h / 2}}, {{w / 3, h / 4}, {w - 5, h - 7}}};
        std::vector<image_data> by_point = sam_compute_batch(model, span<i32x2 const>(points));
        std::vector<image_data> by_box = sam_compute_batch(model, span<box_2d const>(boxes));
        if (by_point.size() != points.size() || by_box.size() != boxes.size()) throw exception("sam_prompts_check: wrong number of masks");
        long differing = 0;
        auto compare = [&](image_data const& a, image_data const& b) {
            if (a.extent[0] != w || a.extent[1] != h || a.format != image_format::alpha_u8 || b.extent[0] != w || b.extent[1] != h)
                throw exception("sam_prompts_check: a mask has the wrong extent or format");
            for (size_t i = 0; i < size_t(w) * h; ++i) differing += a.data.get()[i] != b.data.get()[i];
        };
        for (size_t i = 0; i < points.size(); ++i) compare(by_point[i], sam_compute(model, points[i]));
        for (size_t i = 0; i < boxes.size(); ++i) compare(by_box[i], sam_compute(model, boxes[i]));
        std::printf("%zu masks %dx%d differing %ld\n", by_point.size() + by_box.size(), w, h, differing);
        return 0;
    } catch (std::exception const& e) {
        std::fprintf(stderr, "sam_prompts_check: %s\n", e.what());
        return 1;
    }
}
