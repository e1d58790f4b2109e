// The two kinds of TinyViT stage written against include/visp/nn.h with the ggml names (VISP_GGML_NAMES) -- the node sequences the reference's
// arch code emits for an inverted-bottleneck conv block and for a windowed transformer block (src/visp/arch/mobile-sam.cpp:25-65, 78-92, 115-161) --
// over the weights of an encoder GGUF given on the command line:
//   tinyvit_check <file.gguf> <mbconv | block> <prefix> <C> <resolution> <batch> <heads> <window> <fused models 0 | 1>
// Host only: the graph is planned without a device and its launch list (compute_graph_describe) goes to stdout, where
// tests/test_graph_tinyvit_cpu.py compares it with the Python face's for the same weights. Built by __graft_entry__.build().
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define VISP_GGML_NAMES
#include "visp/nn.h"

using namespace visp;

namespace {

// every conv of the encoder carries its folded batch norm under "<name>.c"
tensor pointwise(model_ref m, tensor t) { return conv_2d(m["c"], t); }
tensor per_channel_3x3(model_ref m, tensor t) { return conv_2d_depthwise(m["c"], t, 1, 1); }

// expand 1x1 -> depthwise 3x3 -> project 1x1, + input, GELU after each step (mobile-sam.cpp:78-92)
tensor inverted_bottleneck(model_ref m, tensor in) {
    tensor wide = ggml_gelu_inplace(m, pointwise(m["conv1"], in));
    wide = ggml_gelu_inplace(m, per_channel_3x3(m["conv2"], wide));
    tensor narrow = pointwise(m["conv3"], wide);
    return named(m, ggml_gelu_inplace(m, ggml_add_inplace(m, narrow, in)));
}

struct window_grid {
    int win;
    int64_t side, extra, per_side; // the map is side x side, padded by `extra` to per_side windows each way
    window_grid(int win_, int64_t side_) : win(win_), side(side_), extra((win_ - side_ % win_) % win_), per_side((side_ + extra) / win_) {}
};

// [C, side, side, B] -> [C, win * win, windows * B]: zero padding up to whole windows, then rows of `win` pixels move as units (mobile-sam.cpp:25-44)
tensor into_windows(model_ref m, tensor t, window_grid const& wg) {
    const int64_t ch = t->ne[0], bt = t->ne[3];
    if (wg.extra > 0) t = ggml_pad(m, t, 0, int(wg.extra), int(wg.extra), 0);
    tensor rows = ggml_reshape_4d(m, t, ch * wg.win, wg.per_side, wg.win, wg.per_side * bt);
    rows = ggml_cont(m, ggml_permute(m, rows, 0, 2, 1, 3));
    return ggml_reshape_3d(m, rows, ch, int64_t(wg.win) * wg.win, wg.per_side * wg.per_side * bt);
}
// ... and back, cropping the padding (mobile-sam.cpp:46-65)
tensor out_of_windows(model_ref m, tensor t, window_grid const& wg) {
    const int64_t ch = t->ne[0], bt = t->ne[2] / (wg.per_side * wg.per_side), padded = wg.side + wg.extra;
    tensor rows = ggml_reshape_4d(m, t, ch * wg.win, wg.win, wg.per_side, wg.per_side * bt);
    rows = ggml_cont(m, ggml_permute(m, rows, 0, 2, 1, 3));
    rows = ggml_reshape_4d(m, rows, ch, padded, padded, bt);
    return ggml_cont(m, slice(m, rows, {}, {0, wg.side}, {0, wg.side}, {}));
}

// LayerNorm, q | k | v per head, softmax(q k^T / sqrt(d) + the per-head bias image) v, projection (mobile-sam.cpp:124-132)
tensor biased_attention(model_ref m, tensor t, int heads) {
    const float inv_sqrt_d = 1.0f / std::sqrt(float(t->ne[0] / heads));
    tensor bias = m.weights("attention_biases_indexed");
    attention_qkv p = split_qkv(m["qkv"], layer_norm(m["norm"], t), heads, 1);
    return attention(m, p.q, p.k, p.v, bias, inv_sqrt_d, m["proj"]);
}

// windowed attention + input, depthwise 3x3 on the map, + MLP (mobile-sam.cpp:134-161)
tensor transformer_block(model_ref m, tensor tokens, int64_t side, int heads, int win) {
    const int64_t ch = tokens->ne[0], count = tokens->ne[1], bt = tokens->ne[2];
    if (count != side * side) throw exception("tinyvit_check: the tokens do not form a square map of that resolution");
    const window_grid wg(win, side);
    tensor t = into_windows(m, ggml_reshape_4d(m, tokens, ch, side, side, bt), wg);
    t = out_of_windows(m, biased_attention(m["attn"], t, heads), wg);
    t = ggml_add_inplace(m, ggml_reshape_3d(m, t, ch, count, bt), tokens);
    t = conv_2d_depthwise(m["local_conv"]["c"], ggml_reshape_4d(m, t, ch, side, side, bt), 1, 1);
    t = ggml_reshape_3d(m, t, ch, count, bt);
    model_ref ff = m["mlp"];
    tensor hidden = ggml_gelu_inplace(ff, linear(ff["fc1"], layer_norm(ff["norm"], t)));
    return named(m, ggml_add_inplace(m, t, named(ff, linear(ff["fc2"], hidden))));
}

} // namespace

int main(int argc, char** argv) {
    try {
        if (argc != 10) throw exception("usage: tinyvit_check <file.gguf> <mbconv | block> <prefix> <C> <resolution> <batch> <heads> <window> <fused models 0 | 1>");
        const int C = std::atoi(argv[4]), res = std::atoi(argv[5]), batch = std::atoi(argv[6]), heads = std::atoi(argv[7]), window = std::atoi(argv[8]);
        model_file file = model_load(argv[1]);
        model_weights weights;
        model_transfer(file, weights);
        compute_graph graph = compute_graph_init(weights);
        model_ref m(graph);
        tensor out;
        if (std::strcmp(argv[2], "mbconv") == 0) out = inverted_bottleneck(m.with_prefix(argv[3]), compute_graph_input(m, GGML_TYPE_F16, {C, res, res, batch}, "x"));
        else out = transformer_block(m.with_prefix(argv[3]), compute_graph_input(m, GGML_TYPE_F16, {C, int64_t(res) * res, batch, 1}, "x"), res, heads, window);
        compute_graph_output(m, out, "out");
        detail::check(visp_graph_set_fused_models(graph.handle, std::atoi(argv[9])));
        compute_graph_plan(graph);
        std::fputs(compute_graph_describe(graph).c_str(), stdout);
        return 0;
    } catch (std::exception const& e) {
        std::fprintf(stderr, "tinyvit_check: %s\n", e.what());
        return 1;
    }
}
