// One ASPP branch of a BiRefNet decoder block written against include/visp/nn.h with the ggml names (VISP_GGML_NAMES) -- the node sequence the
// reference's arch code emits (src/visp/arch/birefnet.cpp:83-92, 109-114) -- over the weights of a GGUF given on the command line:
//   deform_check <file.gguf> <module prefix> <Cin> <w> <h> <batch> <padding> <fused models 0 | 1>
// Host only: the graph is planned without a device and its launch list (compute_graph_describe) goes to stdout, where
// tests/test_graph_deform_cpu.py compares it with the Python face's for the same weights. Built by __graft_entry__.build().
#include <cstdio>
#include <cstdlib>

#define VISP_GGML_NAMES
#include "visp/nn.h"

using namespace visp;

namespace {

// offsets and modulation from two plain convolutions of the same input, then the sampled convolution (birefnet.cpp:83-92)
tensor sampled_conv(model_ref m, tensor x, int pad) {
    tensor where = conv_2d(m["offset"], x, 1, pad);
    tensor how_much = ggml_scale_inplace(m, ggml_sigmoid_inplace(m, conv_2d(m["modulator"], x, 1, pad)), 2.0f);
    return named(m, conv_2d_deform(m, x, m.weights("conv.weight"), where, how_much, 1, pad));
}

// ... its folded batch norm and the activation (birefnet.cpp:109-114)
tensor branch(model_ref m, tensor x, int pad) {
    tensor y = batch_norm_2d(m["bn"], sampled_conv(m["conv"], x, pad));
    return named(m, ggml_relu_inplace(m, y));
}

} // namespace

int main(int argc, char** argv) {
    try {
        if (argc != 9) throw exception("usage: deform_check <file.gguf> <module prefix> <Cin> <w> <h> <batch> <padding> <fused models 0 | 1>");
        const int cin = std::atoi(argv[3]), w = std::atoi(argv[4]), h = std::atoi(argv[5]), batch = std::atoi(argv[6]), pad = std::atoi(argv[7]);
        model_file file = model_load(argv[1]);
        model_weights weights;
        model_transfer(file, weights);
        compute_graph graph = compute_graph_init(weights);
        model_ref m(graph);
        tensor x = compute_graph_input(m, GGML_TYPE_F16, {cin, w, h, batch}, "x");
        compute_graph_output(m, branch(m.with_prefix(argv[2]), x, pad), "branch");
        detail::check(visp_graph_set_fused_models(graph.handle, std::atoi(argv[8])));
        compute_graph_plan(graph);
        std::fputs(compute_graph_describe(graph).c_str(), stdout);
        return 0;
    } catch (std::exception const& e) {
        std::fprintf(stderr, "deform_check: %s\n", e.what());
        return 1;
    }
}
