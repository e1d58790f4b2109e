// One decoder level of BiRefNet without its ASPP, written against include/visp/nn.h the way the reference's arch code is (src/visp/arch/birefnet.cpp:147-168,
// 198-209): the half-size image (downscale_by), image_to_patches of it, simple_conv, the channel concat with the carried map, the block's two 3x3 convs, gdt_conv
// and the gate -- over the weights of a BiRefNet GGUF given on the command line:
//   birefnet_graph_check <file.gguf> <image width> <image height> <batch> <fused models 0 | 1>
// The carried map is 1/16 of the image (level 3: 256 channels in, patches at grid 16 through ipt_blk4, 128 channels out). Host only: the graph is planned
// without a device and its launch list (compute_graph_describe) goes to stdout, where tests/test_graph_birefnet_cpu.py compares it with the Python face's for
// the same weights. Built by __graft_entry__.build().
#include <cstdio>
#include <cstdlib>

#define VISP_GGML_NAMES
#include "visp/nn.h"

using namespace visp;

namespace {

constexpr int32_t bilinear_align_corners = GGML_SCALE_MODE_BILINEAR | GGML_SCALE_FLAG_ALIGN_CORNERS;

tensor simple_conv(model_ref m, tensor x) {
    x = conv_2d(m["conv1"], x, 1, 1);
    x = conv_2d(m["conv_out"], x, 1, 1);
    return named(m, x);
}

tensor gdt_conv(model_ref m, tensor x) { return ggml_relu_inplace(m, conv_2d(m[0], x, 1, 1)); }

// ggml_mul(p, gate) with gate [1, W, H, N]: the broadcast is written out where the batch is larger than one (mul takes a plane [1, W, H, 1] only)
tensor gated(model_ref m, int level, tensor p) {
    char name[64];
    std::snprintf(name, sizeof name, "gdt_convs_%d", level);
    tensor p_gdt = gdt_conv(m[name], p);
    std::snprintf(name, sizeof name, "gdt_convs_attn_%d.0", level);
    tensor attn = ggml_sigmoid(m, conv_2d(m[name], p_gdt));
    if (p->ne[3] > 1) attn = ggml_repeat_4d(m, attn, p->ne[0], p->ne[1], p->ne[2], p->ne[3]);
    return ggml_mul(m, p, attn);
}

} // namespace

int main(int argc, char** argv) {
    try {
        if (argc != 6) throw exception("usage: birefnet_graph_check <file.gguf> <image width> <image height> <batch> <fused models 0 | 1>");
        const int64_t W = std::atoi(argv[2]), H = std::atoi(argv[3]), batch = std::atoi(argv[4]);
        model_file file = model_load(argv[1]);
        model_weights weights;
        model_transfer(file, weights);
        compute_graph graph = compute_graph_init(weights);
        model_ref m(graph);
        model_ref dec = m["decoder"];
        tensor image = compute_graph_input(m, GGML_TYPE_F32, {3, W, H, batch}, "image");
        tensor carried = compute_graph_input(m, GGML_TYPE_F16, {256, W / 16, H / 16, batch}, "p3_in");
        tensor half = interpolate(m, image, {W / 2, H / 2}, bilinear_align_corners);
        tensor patches = simple_conv(dec["ipt_blk4"], image_patches(m, image, carried->ne[1], carried->ne[2]));
        tensor half_patches = image_patches(m, half, carried->ne[1], carried->ne[2]); // grid 8: the half-size image is an image to every reader
        tensor x = ggml_concat(m, carried, patches, 0);
        x = ggml_relu_inplace(m, conv_2d(dec["block3"]["conv_in"], x, 1, 1));
        x = conv_2d(dec["block3"]["conv_out"], x, 1, 1);
        compute_graph_output(m, gated(dec, 3, x), "p3");
        compute_graph_output(m, half_patches, "half_patches");
        detail::check(visp_graph_set_fused_models(graph.handle, std::atoi(argv[5])));
        compute_graph_plan(graph);
        std::fputs(compute_graph_describe(graph).c_str(), stdout);
        return 0;
    } catch (std::exception const& e) {
        std::fprintf(stderr, "birefnet_graph_check: %s\n", e.what());
        return 1;
    }
}
