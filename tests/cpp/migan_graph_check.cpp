// MI-GAN's separable_conv_2d in any flag combination, and one synthesis_block, written against include/visp/nn.h with the ggml names (VISP_GGML_NAMES) --
// the node sequences of the CWHN branch of src/visp/arch/migan.cpp:17-127 -- over the weights of a generator GGUF given on the command line:
//   migan_graph_check <file.gguf> <sep | block> <prefix> <c_in> <width> <height> <batch> <flags> <fused models 0 | 1>
// flags: 1 activation, 2 downsample, 4 upsample, 8 noise (sep); 4 upsample + noise, 16 an incoming image (block). The image path is 8 channels wide, channels
// 3..7 zero, as vision.cpp_amd/graph.py builds it. Host only: the graph is planned without a device and its launch list (compute_graph_describe) goes to stdout,
// where tests/test_graph_migan_cpu.py compares it with the Python face's for the same weights. Built by __graft_entry__.build().
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define VISP_GGML_NAMES
#include "visp/nn.h"

using namespace visp;

namespace {

constexpr float sqrt2 = 1.4142135623f;
enum : int { f_activation = 1, f_downsample = 2, f_upsample = 4, f_noise = 8, f_image = 16 };

tensor lrelu_agc(model_ref m, tensor x, float alpha, float gain, float clamp) {
    x = ggml_leaky_relu(m, x, alpha, true);
    if (gain != 1) x = ggml_scale_inplace(m, x, gain);
    if (clamp != 0) x = ggml_clamp(m, x, -clamp, clamp);
    return named(m, x);
}

tensor upsample_2d(model_ref m, tensor x, tensor fir = {}) {
    tensor filter = m.weights("filter_const");
    filter = ggml_reshape_4d(m, filter, 1, filter->ne[0], filter->ne[1], 1);
    auto [w, h, c, n] = nelements_whcn(m, x);
    x = interpolate(m, x, {w * 2, h * 2}, GGML_SCALE_MODE_NEAREST);
    x = ggml_mul_inplace(m, x, filter);
    x = fir ? detail::op(m, VISP_OP_CONV_2D_DEPTHWISE, {x, fir}, {1, 2}) : conv_2d_depthwise(m["filter"], x, 1, 2);
    x = slice(m, x, {}, {0, -1}, {0, -1}, {});
    x = ggml_cont(m, x);
    return named(m, x);
}

tensor separable_conv_2d(model_ref m, tensor x, int flags) {
    const int pad = int(m["conv1"].weights("weight")->ne[2] / 2);
    x = conv_2d_depthwise(m["conv1"], x, 1, pad);
    if (flags & f_activation) x = lrelu_agc(m, x, 0.2f, sqrt2, 256);
    if (flags & f_downsample) x = conv_2d_depthwise(m["downsample"]["filter"], x, 2, 1);
    x = conv_2d(m["conv2"], x);
    if (flags & f_upsample) x = upsample_2d(m["upsample"], x);
    if (flags & f_noise) {
        tensor noise = m.weights("noise_const");
        noise = ggml_mul_inplace(m, noise, m.weights("noise_strength"));
        noise = ggml_reshape_4d(m, noise, 1, noise->ne[0], noise->ne[1], 1);
        x = ggml_add_inplace(m, x, noise);
    }
    if (flags & f_activation) x = lrelu_agc(m, x, 0.2f, sqrt2, 256);
    return named(m, x);
}

// the constant `name` under m, its 3 channels (the slowest dimension that is 3) zero-padded to 8, as the named host constant "<name>.pad8"
tensor pad8(model_ref m, char const* name) {
    const std::string full = std::string(m.prefix.c_str()) + "." + name + ".pad8";
    if (tensor t = get_tensor(m, full.c_str())) return t;
    tensor src = m.weights(name);
    int64_t ne[4] = {src->ne[0], src->ne[1], src->ne[2], src->ne[3]}, n = ne[0] * ne[1] * ne[2] * ne[3];
    int dim = 3;
    while (dim > 0 && ne[dim] != 3) --dim;
    std::vector<float> v((size_t)n), out((size_t)(n / 3 * 8), 0.0f);
    detail::check(visp_graph_read_constant(m.handle(), src.id, v.data(), n));
    std::copy(v.begin(), v.end(), out.begin()); // the padded dimension is the slowest one that is not 1: the values come first
    ne[dim] = 8;
    return compute_graph_constant(m, full.c_str(), GGML_TYPE_F16, {ne[0], ne[1], ne[2], ne[3]}, out.data());
}

tensor synthesis_block(model_ref m, tensor x, tensor feat, tensor img, int flags) {
    const int up = flags & f_upsample, noise = up ? f_noise : 0;
    x = separable_conv_2d(m["conv1"], x, f_activation | noise | up);
    x = ggml_add_inplace(m, x, feat);
    x = separable_conv_2d(m["conv2"], x, f_activation | noise);
    if (img) img = upsample_2d(m["upsample"], img, pad8(m["upsample"]["filter"], "weight"));
    tensor y = detail::op(m, VISP_OP_CONV_2D, {x, pad8(m["torgb"], "weight"), pad8(m["torgb"], "bias")}, {1, 0});
    img = img ? ggml_add_inplace(m, img, y) : y;
    compute_graph_output(m, img, "o1");
    return x;
}

} // namespace

int main(int argc, char** argv) {
    try {
        if (argc != 10) throw exception("usage: migan_graph_check <file.gguf> <sep | block> <prefix> <c_in> <width> <height> <batch> <flags> <fused models 0 | 1>");
        const int c_in = std::atoi(argv[4]), w = std::atoi(argv[5]), h = std::atoi(argv[6]), batch = std::atoi(argv[7]), flags = std::atoi(argv[8]);
        model_file file = model_load(argv[1]);
        model_weights weights;
        model_transfer(file, weights);
        compute_graph graph = compute_graph_init(weights);
        model_ref root(graph);
        model_ref m = root.with_prefix(argv[3]);
        tensor x = compute_graph_input(m, GGML_TYPE_F16, {c_in, w, h, batch}, "x");
        tensor out;
        if (std::strcmp(argv[2], "sep") == 0) out = separable_conv_2d(m, x, flags);
        else {
            const int s = flags & f_upsample ? 2 : 1;
            const int64_t c_out = m["conv2"]["conv2"].weights("weight")->ne[3];
            tensor feat = compute_graph_input(m, GGML_TYPE_F16, {c_out, w * s, h * s, batch}, "feat");
            tensor img = flags & f_image ? compute_graph_input(m, GGML_TYPE_F16, {8, w, h, batch}, "img") : tensor();
            out = synthesis_block(m, x, feat, img, flags);
        }
        compute_graph_output(root, out, "o0");
        detail::check(visp_graph_set_fused_models(graph.handle, std::atoi(argv[9])));
        compute_graph_plan(graph);
        std::fputs(compute_graph_describe(graph).c_str(), stdout);
        return 0;
    } catch (std::exception const& e) {
        std::fprintf(stderr, "migan_graph_check: %s\n", e.what());
        return 1;
    }
}
