// The automatic mask generation of include/visp/vision.h -- sam_point_grid and the three sam_generate_masks overloads (points, boxes, points per side) --
// compiled and linked against the library, and run on a MobileSAM file given on the command line:
//   sam_autogen_check <mobile_sam.gguf> <width> <height>
// A gradient image of that extent is encoded once. With thresholds that let every candidate through (and NMS that suppresses nobody: an IoU never exceeds 1)
// each record is checked against its own mask: area = the pixels that are 255, the box is theirs, the records come by predicted iou descending, prompt and
// plane are in range; max_masks cuts the list. Prints "<by points> <by boxes> <by grid> <cut> masks <w>x<h> ok".
// Built by __graft_entry__.build(); tests/test_gpu_sam_autogen.py runs it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "visp/vision.h"

using namespace visp;

[[noreturn]] static void fail(std::string const& what, std::string const& why) { throw exception("sam_autogen_check: " + what + ": " + why); }

int main(int argc, char** argv) {
    try {
        if (argc != 4) throw exception("usage: sam_autogen_check <mobile_sam.gguf> <width> <height>");
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

        std::vector<i32x2> grid = sam_point_grid(3, i32x2{w, h});
        if (grid.size() != 9 || grid[0][0] != int(0.5 * w / 3) || grid[8][1] != int(2.5 * h / 3) || grid[1][1] != grid[0][1])
            throw exception("sam_autogen_check: sam_point_grid is not the row-by-row grid of pixel centres");

        sam_generate_params all;
        all.pred_iou_thresh = -1e30f;
        all.stability_thresh = -1.0f;
        all.nms_iou_thresh = 1.0f;
        all.max_masks = 64;
        auto verify = [&](std::vector<sam_mask> const& masks, int n_prompts, char const* what) {
            for (size_t k = 0; k < masks.size(); ++k) {
                sam_mask const& m = masks[k];
                if (m.segmentation.extent[0] != w || m.segmentation.extent[1] != h || m.segmentation.format != image_format::alpha_u8)
                    fail(what, "a mask has the wrong extent or format");
                int area = 0, x0 = w, y0 = h, x1 = -1, y1 = -1;
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x) {
                        const uint8_t v = m.segmentation.data.get()[size_t(y) * w + x];
                        if (v != 0 && v != 255) fail(what, "a mask value is neither 0 nor 255");
                        if (v == 255) { ++area; x0 = std::min(x0, x); y0 = std::min(y0, y); x1 = std::max(x1, x); y1 = std::max(y1, y); }
                    }
                const bool box_ok = area ? (m.bbox_top_left[0] == x0 && m.bbox_top_left[1] == y0 && m.bbox_extent[0] == x1 - x0 + 1 && m.bbox_extent[1] == y1 - y0 + 1)
                                         : (m.bbox_top_left[0] == 0 && m.bbox_top_left[1] == 0 && m.bbox_extent[0] == 0 && m.bbox_extent[1] == 0);
                if (m.area != area || !box_ok) fail(what, "record " + std::to_string(k) + " does not describe its mask");
                if (m.prompt < 0 || m.prompt >= n_prompts || m.plane < 0 || m.plane > 2) fail(what, "prompt or plane out of range");
                if (k && !(masks[k - 1].predicted_iou >= m.predicted_iou)) fail(what, "records are not in order of predicted iou");
                if (!(m.stability_score >= 0.0f && m.stability_score <= 1.0f)) fail(what, "stability score outside [0, 1]");
            }
        };
        std::vector<sam_mask> by_point = sam_generate_masks(model, span<i32x2 const>(grid), all);
        verify(by_point, 9, "points");
        std::vector<box_2d> boxes = {{{w / 8, h / 8}, {w / 2, h / 2}}, {{w / 3, h / 4}, {w - 5, h - 7}}};
        std::vector<sam_mask> by_box = sam_generate_masks(model, span<box_2d const>(boxes), all);
        verify(by_box, 2, "boxes");
        std::vector<sam_mask> by_grid = sam_generate_masks(model, 3, all);
        verify(by_grid, 9, "points per side");
        if (by_grid.size() != by_point.size()) throw exception("sam_autogen_check: the grid overload and the grid's points disagree");
        for (size_t k = 0; k < by_grid.size(); ++k)
            if (by_grid[k].prompt != by_point[k].prompt || by_grid[k].plane != by_point[k].plane || by_grid[k].area != by_point[k].area)
                fail("points per side", "differs from the grid's points at record " + std::to_string(k));
        sam_generate_params cut = all;
        cut.max_masks = 2;
        std::vector<sam_mask> two = sam_generate_masks(model, span<i32x2 const>(grid), cut);
        verify(two, 9, "cut");
        if (two.size() != std::min<size_t>(2, by_point.size())) throw exception("sam_autogen_check: max_masks does not cut the list");
        for (size_t k = 0; k < two.size(); ++k)
            if (two[k].prompt != by_point[k].prompt || two[k].plane != by_point[k].plane) throw exception("sam_autogen_check: the cut list is not the head of the full one");
        if (sam_generate_masks(model, 2).size() > 12) throw exception("sam_autogen_check: more masks than candidates"); // SAM's default thresholds
        std::printf("%zu %zu %zu %zu masks %dx%d ok\n", by_point.size(), by_box.size(), by_grid.size(), two.size(), w, h);
        return 0;
    } catch (std::exception const& e) {
        std::fprintf(stderr, "sam_autogen_check: %s\n", e.what());
        return 1;
    }
}
