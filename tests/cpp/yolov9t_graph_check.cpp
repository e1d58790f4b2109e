// Two YOLOv9t blocks written against include/visp/nn.h with the ggml names (VISP_GGML_NAMES) -- the node sequences the reference's arch code emits
// for SPPELAN and RepNCSPELAN4 (src/visp/arch/yolov9t.cpp:78-130, 256-483) -- over the weights of a detector GGUF given on the command line:
//   yolov9t_graph_check <file.gguf> <sppelan | elan4> <prefix> <c_in> <c3> <c4> <width> <height> <batch> <fused models 0 | 1>
// Host only: the graph is planned without a device and its launch list (compute_graph_describe) goes to stdout, where
// tests/test_graph_yolo_cpu.py compares it with the Python face's for the same weights. Built by __graft_entry__.build().
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#define VISP_GGML_NAMES
#include "visp/nn.h"

using namespace visp;

namespace {

// conv at pad k / 2 with the folded batch norm's bias under "<name>.conv", then SiLU
tensor act_conv(model_ref root, tensor t, std::string const& name, int k, int stride = 1, bool act = true) {
    tensor y = conv_2d(root.with_prefix((name + ".conv").c_str()), t, stride, k / 2);
    return act ? ggml_silu_inplace(root, y) : y;
}

// 3x3 and 1x1 branches on one input, summed, then SiLU
tensor two_branch_conv(model_ref root, tensor t, std::string const& name) {
    tensor wide = act_conv(root, t, name + ".conv1", 3, 1, false);
    tensor point = act_conv(root, t, name + ".conv2", 1, 1, false);
    return ggml_silu(root, ggml_add(root, wide, point));
}

// two 1x1 branches; the first runs through `depth` shortcut bottlenecks (two-branch conv, 3x3 conv, + input); concat, 1x1
tensor csp_stage(model_ref root, tensor t, std::string const& name, int depth) {
    tensor deep = act_conv(root, t, name + ".cv1", 1);
    tensor side = act_conv(root, t, name + ".cv2", 1);
    for (int i = 0; i < depth; ++i) {
        const std::string b = name + ".m." + std::to_string(i);
        deep = ggml_add(root, deep, act_conv(root, two_branch_conv(root, deep, b + ".cv1"), b + ".cv2", 3));
    }
    return act_conv(root, ggml_cont(root, ggml_concat(root, deep, side, 0)), name + ".cv3", 1);
}

tensor elan4_block(model_ref root, tensor t, std::string const& name, int c3, int depth) {
    tensor stem = act_conv(root, t, name + ".cv1", 1);
    tensor low = slice(root, stem, {0, c3 / 2});
    tensor high = slice(root, stem, {c3 / 2, c3});
    tensor a = act_conv(root, csp_stage(root, high, name + ".cv2.0", depth), name + ".cv2.1", 3);
    tensor b = act_conv(root, csp_stage(root, a, name + ".cv3.0", depth), name + ".cv3.1", 3);
    return act_conv(root, concat(root, {low, high, a, b}, 0), name + ".cv4", 1);
}

tensor spp_block(model_ref root, tensor t, std::string const& name, int k) {
    tensor stem = act_conv(root, t, name + ".cv1", 1);
    tensor p1 = ggml_pool_2d(root, stem, GGML_OP_POOL_MAX, k, k, 1, 1, k / 2, k / 2);
    tensor p2 = ggml_pool_2d(root, p1, GGML_OP_POOL_MAX, k, k, 1, 1, k / 2, k / 2);
    tensor p3 = ggml_pool_2d(root, p2, GGML_OP_POOL_MAX, k, k, 1, 1, k / 2, k / 2);
    return act_conv(root, ggml_cont(root, concat(root, {stem, p1, p2, p3}, 0)), name + ".cv5", 1);
}

} // namespace

int main(int argc, char** argv) {
    try {
        if (argc != 11) throw exception("usage: yolov9t_graph_check <file.gguf> <sppelan | elan4> <prefix> <c_in> <c3> <c4> <width> <height> <batch> <fused models 0 | 1>");
        const int c_in = std::atoi(argv[4]), c3 = std::atoi(argv[5]), w = std::atoi(argv[7]), h = std::atoi(argv[8]), batch = std::atoi(argv[9]);
        model_file file = model_load(argv[1]);
        model_weights weights;
        model_transfer(file, weights);
        compute_graph graph = compute_graph_init(weights);
        model_ref m(graph);
        tensor x = compute_graph_input(m, GGML_TYPE_F16, {c_in, w, h, batch}, "x");
        tensor out = std::strcmp(argv[2], "sppelan") == 0 ? spp_block(m, x, argv[3], 5) : elan4_block(m, x, argv[3], c3, 3);
        compute_graph_output(m, out, "o0");
        detail::check(visp_graph_set_fused_models(graph.handle, std::atoi(argv[10])));
        compute_graph_plan(graph);
        std::fputs(compute_graph_describe(graph).c_str(), stdout);
        return 0;
    } catch (std::exception const& e) {
        std::fprintf(stderr, "yolov9t_graph_check: %s\n", e.what());
        return 1;
    }
}
