// One layer of the SAM3 vision transformer written against include/visp/nn.h with the ggml names (VISP_GGML_NAMES): the rotary embedding as two
// ggml_rope_ext calls on the two halves of every head of q and k, windows cut with pad / reshape / permute, over the weights of a 'sam3' GGUF:
//   sam3_check <file.gguf> <layer> <heads> <grid side> <window, 0 = global> <batch> <fused models 0 | 1>
// (a negative <layer> makes one ggml_rope_ext call that must be refused and prints the refusal to stderr.)
// Host only: the graph is planned without a device and its launch list (compute_graph_describe) goes to stdout, where
// tests/test_graph_sam3_cpu.py compares it line by line with the Python face's for the same weights. Built by __graft_entry__.build().
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define VISP_GGML_NAMES
#include "visp/nn.h"

using namespace visp;

namespace {

struct grid_positions { tensor col, row; float scale; };

// token i of a side x side grid sits in column i % side and row i / side: two i32 constants
grid_positions make_positions(model_ref m, int side, float scale, std::string const& name) {
    std::vector<int32_t> col(size_t(side) * side), row(col.size());
    for (int i = 0; i < side * side; ++i) { col[i] = i % side; row[i] = i / side; }
    tensor c = compute_graph_constant(m, (name + ".x").c_str(), GGML_TYPE_I32, {side * side, 1, 1, 1}, col.data());
    tensor r = compute_graph_constant(m, (name + ".y").c_str(), GGML_TYPE_I32, {side * side, 1, 1, 1}, row.data());
    return {c, r, scale};
}

// the lower half of every head turns with the column, the upper half with the row
tensor rotate_heads(model_ref m, tensor t, grid_positions const& p) {
    const int64_t hd = t->ne[0];
    tensor lo = ggml_rope_ext(m, slice(m, t, {0, hd / 2}), p.col, nullptr, int(hd / 2), GGML_ROPE_TYPE_NORMAL, 0, 10000.f, p.scale, 0.f, 1.f, 0.f, 0.f);
    tensor hi = ggml_rope_ext(m, slice(m, t, {hd / 2, hd}), p.row, nullptr, int(hd / 2), GGML_ROPE_TYPE_NORMAL, 0, 10000.f, p.scale, 0.f, 1.f, 0.f, 0.f);
    return ggml_concat(m, lo, hi, 0);
}

tensor rotary_attention(model_ref m, tensor t, int heads, grid_positions const& p) {
    const int64_t hd = t->ne[0] / heads;
    auto project = [&](char const* name) {
        tensor y = linear(m[name], t);
        return ggml_reshape_4d(m, y, hd, heads, y->ne[1], y->ne[2]);
    };
    tensor q = project("q_proj"), k = project("k_proj"), v = project("v_proj");
    return attention(m, rotate_heads(m, q, p), rotate_heads(m, k, p), v, nullptr, 1.0f / std::sqrt(float(hd)), m["o_proj"]);
}

// [C, W, H, B] -> [C, win * win, windows * B], zero-padded at the right and bottom to whole windows; and back
tensor to_windows(model_ref m, tensor t, int win, int64_t& pw, int64_t& ph) {
    auto [c, w, h, b] = nelements(t);
    pw = (win - w % win) % win;
    ph = (win - h % win) % win;
    if (pw || ph) t = ggml_pad(m, t, 0, int(pw), int(ph), 0);
    const int64_t nw = (w + pw) / win, nh = (h + ph) / win;
    t = ggml_cont(m, ggml_permute(m, ggml_reshape_4d(m, t, c * win, nw, win, nh * b), 0, 2, 1, 3));
    return ggml_reshape_3d(m, t, c, int64_t(win) * win, nw * nh * b);
}
tensor from_windows(model_ref m, tensor t, int win, int64_t w, int64_t h, int64_t b, int64_t pw, int64_t ph) {
    const int64_t c = t->ne[0], nw = (w + pw) / win, nh = (h + ph) / win;
    t = ggml_cont(m, ggml_permute(m, ggml_reshape_4d(m, t, c * win, win, nw, nh * b), 0, 2, 1, 3));
    t = ggml_reshape_4d(m, t, c, w + pw, h + ph, b);
    if (pw || ph) t = ggml_cont(m, slice(m, t, {}, {0, w}, {0, h}));
    return t;
}

tensor encoder_layer(model_ref m, tensor t, int win, int heads, grid_positions const& p) {
    auto [c, w, h, b] = nelements(t);
    tensor y = layer_norm(m["layer_norm1"], t);
    int64_t pw = 0, ph = 0;
    y = win > 0 ? to_windows(m, y, win, pw, ph) : ggml_reshape_3d(m, y, c, w * h, b);
    y = rotary_attention(m["attention"], y, heads, p);
    y = win > 0 ? from_windows(m, y, win, w, h, b, pw, ph) : ggml_reshape_4d(m, y, c, w, h, b);
    t = ggml_add(m, y, t);
    y = layer_norm(m["layer_norm2"], t);
    y = linear(m["mlp"]["fc2"], ggml_gelu(m, linear(m["mlp"]["fc1"], y)));
    return named(m, ggml_add(m, y, t));
}

} // namespace

int main(int argc, char** argv) {
    try {
        if (argc != 8) throw exception("usage: sam3_check <file.gguf> <layer> <heads> <grid side> <window, 0 = global> <batch> <fused models 0 | 1>");
        const int layer = std::atoi(argv[2]), heads = std::atoi(argv[3]), side = std::atoi(argv[4]), win = std::atoi(argv[5]), batch = std::atoi(argv[6]);
        model_file file = model_load(argv[1]);
        model_weights weights;
        model_transfer(file, weights);
        compute_graph graph = compute_graph_init(weights);
        model_ref m(graph);
        model_ref bb = m["det.ve.backbone"];
        const int64_t ch = bb["layer_norm"].weights("weight")->ne[0];
        tensor x = compute_graph_input(m, GGML_TYPE_F16, {ch, side, side, batch}, "x");
        if (layer < 0) { // the refusals of the ggml-named wrapper and of the op's mode: -1 ext_factor, -2 attn_factor, -3 beta_fast, -4 beta_slow, -5 frequency factors, -6 NEOX
            tensor t = compute_graph_input(m, GGML_TYPE_F16, {32, heads, int64_t(side) * side, batch}, "t");
            grid_positions g = make_positions(m, side, 1.0f, "p");
            ggml_rope_ext(m, t, g.col, layer == -5 ? t : tensor(nullptr), 32, layer == -6 ? GGML_ROPE_TYPE_NEOX : GGML_ROPE_TYPE_NORMAL, 0, 10000.f, 1.0f, layer == -1 ? 0.5f : 0.f,
                          layer == -2 ? 2.f : 1.f, layer == -3 ? 32.f : 0.f, layer == -4 ? 1.f : 0.f);
            throw exception("sam3_check: the call was not refused");
        }
        grid_positions p = win > 0 ? make_positions(m, win, 1.0f, "_vit_rope_pos_window") : make_positions(m, side, 0.5f, "_vit_rope_pos_global");
        compute_graph_output(m, encoder_layer(bb["layers"][layer], x, win, heads, p), "y");
        detail::check(visp_graph_set_fused_models(graph.handle, std::atoi(argv[7])));
        compute_graph_plan(graph);
        std::fputs(compute_graph_describe(graph).c_str(), stdout);
        return 0;
    } catch (std::exception const& e) {
        std::fprintf(stderr, "sam3_check: %s\n", e.what());
        return 1;
    }
}
