// The region cleaning of include/visp/vision.h -- image_remove_small_regions, sam_generate_params::min_mask_region_area and sam_mask::cleaned -- compiled and
// linked against the library, and run on a MobileSAM file given on the command line:
//   sam_regions_check <mobile_sam.gguf> <width> <height>
// 1. image_remove_small_regions on a hand-made mask whose row stride is wider than its rows: a hole of 3 is filled and an island of 2 removed at min_area 4, a hole
//    and an island of 4 stay, the padding bytes are untouched; each mode alone; min_area 1 changes nothing.
// 2. a generate call that lets every candidate through, without and with min_mask_region_area: without, no record is `cleaned`; with, every returned mask is a
//    fixed point of image_remove_small_regions at that area unless it is the single-island exception, its record describes it, the unchanged masks come before
//    the changed ones and each group is in order of predicted iou.
// Prints "<plain> <cleaned list> <of them changed> masks <w>x<h> ok". Built by __graft_entry__.build(); tests/test_gpu_sam_regions.py runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "visp/vision.h"

using namespace visp;

[[noreturn]] static void fail(std::string const& what) { throw exception("sam_regions_check: " + what); }

int main(int argc, char** argv) {
    try {
        if (argc != 4) throw exception("usage: sam_regions_check <mobile_sam.gguf> <width> <height>");
        const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
        backend_device dev = backend_init();

        // ---- 1. the primitive on a strided span
        const int mw = 40, mh = 12, stride = 48;
        auto make = [&]() {
            std::vector<uint8_t> m(size_t(stride) * mh, 9); // 9 = padding
            for (int y = 0; y < mh; ++y)
                for (int x = 0; x < mw; ++x) m[size_t(y) * stride + x] = y >= 5 ? 255 : 0;
            for (int x = 1; x < 5; ++x) m[1 * stride + x] = 255;  // island of 4
            for (int x = 1; x < 3; ++x) m[3 * stride + x] = 255;  // island of 2
            for (int x = 2; x < 6; ++x) m[7 * stride + x] = 0;    // hole of 4
            for (int x = 2; x < 5; ++x) m[9 * stride + x] = 0;    // hole of 3
            return m;
        };
        auto span_of = [&](std::vector<uint8_t>& m) {
            image_span s({mw, mh}, image_format::alpha_u8, m.data());
            s.stride = stride;
            return s;
        };
        const std::vector<uint8_t> src = make();
        for (region_mode mode : {region_mode::holes, region_mode::islands, region_mode::both}) {
            std::vector<uint8_t> m = make(), want = make();
            if (mode != region_mode::islands) for (int x = 2; x < 5; ++x) want[9 * stride + x] = 255;
            if (mode != region_mode::holes) for (int x = 1; x < 3; ++x) want[3 * stride + x] = 0;
            if (!image_remove_small_regions(span_of(m), 4, mode)) fail("a mask with a small hole and a small island reported no change");
            if (m != want) fail("image_remove_small_regions at min_area 4, mode " + std::to_string(int(mode)));
        }
        {
            std::vector<uint8_t> m = make();
            if (image_remove_small_regions(span_of(m), 1) || m != src) fail("min_area 1 changed a mask");
        }

        // ---- 2. the generate call
        sam_model model = sam_load_model(argv[1], dev);
        image_data img = image_alloc({w, h}, image_format::rgb_u8);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                uint8_t* px = img.data.get() + (size_t(y) * w + x) * 3;
                px[0] = uint8_t(x * 255 / w), px[1] = uint8_t(y * 255 / h), px[2] = uint8_t((x ^ y) & 255);
            }
        sam_encode(model, image_view(img));
        sam_generate_params all;
        all.pred_iou_thresh = -1e30f;
        all.stability_thresh = -1.0f;
        all.nms_iou_thresh = 1.0f;
        all.max_masks = 64;
        std::vector<sam_mask> plain = sam_generate_masks(model, 3, all);
        for (sam_mask const& m : plain)
            if (m.cleaned) fail("a record is `cleaned` without min_mask_region_area");
        sam_generate_params clean = all;
        clean.min_mask_region_area = 40;
        std::vector<sam_mask> cleaned = sam_generate_masks(model, 3, clean);
        if (cleaned.size() != plain.size()) fail("an NMS threshold of 1 removed a mask"); // an IoU never exceeds 1
        size_t n_changed = 0;
        for (size_t k = 0; k < cleaned.size(); ++k) {
            sam_mask& m = cleaned[k];
            n_changed += m.cleaned;
            if (k && cleaned[k - 1].cleaned && !m.cleaned) fail("an unchanged mask behind a changed one");
            if (k && cleaned[k - 1].cleaned == m.cleaned && !(cleaned[k - 1].predicted_iou >= m.predicted_iou)) fail("a group is not in order of predicted iou");
            int area = 0, x0 = w, y0 = h, x1 = -1, y1 = -1;
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x)
                    if (m.segmentation.data.get()[size_t(y) * w + x] == 255) { ++area; x0 = std::min(x0, x); y0 = std::min(y0, y); x1 = std::max(x1, x); y1 = std::max(y1, y); }
            const bool box_ok = area ? (m.bbox_top_left[0] == x0 && m.bbox_top_left[1] == y0 && m.bbox_extent[0] == x1 - x0 + 1 && m.bbox_extent[1] == y1 - y0 + 1)
                                     : (m.bbox_extent[0] == 0 && m.bbox_extent[1] == 0);
            if (m.area != area || !box_ok) fail("record " + std::to_string(k) + " does not describe its cleaned mask");
            image_data again = image_alloc({w, h}, image_format::alpha_u8);
            std::memcpy(again.data.get(), m.segmentation.data.get(), size_t(w) * h);
            image_remove_small_regions(image_span(again), 40, region_mode::holes); // no small hole may be left; a single small island may stay by the exception
            if (std::memcmp(again.data.get(), m.segmentation.data.get(), size_t(w) * h) != 0) fail("a cleaned mask still has a small hole");
            // the same mask without cleaning, by prompt and plane: equal iff the record says unchanged
            for (sam_mask const& p : plain)
                if (p.prompt == m.prompt && p.plane == m.plane) {
                    const bool same = std::memcmp(p.segmentation.data.get(), m.segmentation.data.get(), size_t(w) * h) == 0;
                    if (same == m.cleaned) fail("`cleaned` of record " + std::to_string(k) + " contradicts its bytes");
                }
        }
        std::printf("%zu %zu %zu masks %dx%d ok\n", plain.size(), cleaned.size(), n_changed, w, h);
        return 0;
    } catch (std::exception const& e) {
        std::fprintf(stderr, "sam_regions_check: %s\n", e.what());
        return 1;
    }
}
