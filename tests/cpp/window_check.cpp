// One shifted SWIN block written against include/visp/nn.h with the ggml names (VISP_GGML_NAMES) -- the same node sequence the reference's
// arch code emits (src/visp/arch/swin.cpp:48-141) -- over the weights of a backbone GGUF given on the command line:
//   window_check <file.gguf> <block prefix> <C> <heads> <w> <h> <batch> <window>
// Host only: the graph is planned without a device and its launch list (compute_graph_describe) goes to stdout, where
// tests/test_graph_window_cpu.py compares it with the Python face's for the same weights. Built by __graft_entry__.build().
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define VISP_GGML_NAMES
#include "visp/nn.h"

using namespace visp;

namespace {

// geometry of one block: tokens of a wd x ht map, windows of `win` x `win`, cyclic shift `shift` (0 = unshifted)
struct geometry { int heads, win; int64_t wd, ht; int shift; };

// [C, wd, ht, B] -> [C, win * win, windows * B] and back: rows of `win` pixels are moved as units of C * win values (swin.cpp:48-67)
tensor to_windows(model_ref m, tensor t, int win) {
    const int64_t ch = t->ne[0], wd = t->ne[1], ht = t->ne[2], bt = t->ne[3];
    tensor rows = ggml_reshape_4d(m, t, ch * win, wd / win, win, (ht / win) * bt);
    tensor swapped = ggml_cont(m, ggml_permute(m, rows, 0, 2, 1, 3));
    return ggml_reshape_3d(m, swapped, ch, int64_t(win) * win, (wd / win) * (ht / win) * bt);
}
tensor from_windows(model_ref m, tensor t, int64_t wd, int64_t ht, int win) {
    const int64_t ch = t->ne[0], bt = t->ne[2] / ((wd / win) * (ht / win));
    tensor rows = ggml_reshape_4d(m, t, ch * win, win, wd / win, (ht / win) * bt);
    tensor swapped = ggml_cont(m, ggml_permute(m, rows, 0, 2, 1, 3));
    return ggml_reshape_4d(m, swapped, ch, wd, ht, bt);
}

// bias table rows picked by the precomputed index -> [keys, queries, heads], plus the layer's shift mask spread over heads and images;
// all of it constants, so the graph layer folds the chain into the one mask operand of the attention (swin.cpp:69-97)
tensor attend_in_windows(model_ref m, tensor t, tensor shift_mask, geometry const& g) {
    const int64_t ch = t->ne[0], tok = t->ne[1], wins = t->ne[2];
    const std::string index_name = "window_attention_" + std::to_string(g.win) + ".rel_pos_index";
    tensor bias = ggml_get_rows(m, m.weights("relative_position_bias_table"), ggml_get_tensor(m, index_name.c_str()));
    bias = ggml_cast(m, ggml_permute(m, ggml_reshape_4d(m, bias, g.heads, tok, tok, 1), 2, 0, 1, 3), GGML_TYPE_F16);
    tensor additive = bias;
    if (shift_mask) {
        const int64_t per_image = shift_mask->ne[2];
        tensor sm = shift_mask;
        if (wins > per_image) sm = ggml_repeat_4d(m, ggml_reshape_4d(m, sm, tok, tok, per_image, 1), tok, tok, per_image, wins / per_image);
        sm = ggml_repeat_4d(m, ggml_reshape_4d(m, sm, tok, tok, 1, wins), tok, tok, g.heads, wins);
        additive = ggml_add(m, sm, bias);
    }
    attention_qkv p = split_qkv(m["qkv"], t, g.heads, 2);
    return named(m, attention(m, p.q, p.k, p.v, additive, 1.0f / std::sqrt(float(ch / g.heads)), m["proj"]));
}

// norm1 -> pad to whole windows -> shift -> windows -> attention -> back -> unshift -> crop -> + x -> + mlp(norm2) (swin.cpp:99-141)
tensor swin_block(model_ref m, tensor x, tensor shift_mask, geometry const& g) {
    const int64_t ch = x->ne[0], tok = x->ne[1], bt = x->ne[2];
    const int extra_w = int((g.win - g.wd % g.win) % g.win), extra_h = int((g.win - g.ht % g.win) % g.win);
    const bool padded = extra_w > 0 || extra_h > 0;
    tensor t = ggml_reshape_4d(m, layer_norm(m["norm1"], x), ch, g.wd, g.ht, bt);
    if (padded) t = ggml_pad(m, t, 0, extra_w, extra_h, 0);
    if (g.shift > 0) t = ggml_roll(m, t, 0, -g.shift, -g.shift, 0);
    t = attend_in_windows(m["attn"], to_windows(m, t, g.win), shift_mask, g);
    t = from_windows(m, t, g.wd + extra_w, g.ht + extra_h, g.win);
    if (g.shift > 0) t = ggml_roll(m, t, 0, g.shift, g.shift, 0);
    if (padded) t = ggml_cont(m, slice(m, ggml_reshape_4d(m, t, ch, g.wd + extra_w, g.ht + extra_h, bt), {}, {0, g.wd}, {0, g.ht}, {}));
    tensor y = ggml_add_inplace(m, ggml_reshape_3d(m, t, ch, tok, bt), x);
    model_ref ff = m["mlp"];
    tensor hidden = ggml_gelu_inplace(ff, linear(ff["fc1"], layer_norm(m["norm2"], y)));
    return named(m, ggml_add_inplace(m, y, named(ff, linear(ff["fc2"], hidden))));
}

// what the caller precomputes (swin_precompute): index of the bias table per (query, key) pair of a window, and the shift mask of the
// windows in the last row / column: -inf between tokens on different sides of the seam the cyclic shift leaves inside them
std::vector<int32_t> relative_position_index(int n) {
    std::vector<int32_t> idx(size_t(n) * n * n * n);
    for (int y1 = 0; y1 < n; ++y1)
        for (int x1 = 0; x1 < n; ++x1)
            for (int y0 = 0; y0 < n; ++y0)
                for (int x0 = 0; x0 < n; ++x0) idx[size_t((y1 * n + x1) * n * n + y0 * n + x0)] = (y1 - y0 + n - 1) * (2 * n - 1) + (x1 - x0 + n - 1);
    return idx;
}
std::vector<float> attention_mask(int64_t w, int64_t h, int n) {
    const int64_t nwx = (w + n - 1) / n, nwy = (h + n - 1) / n, n2 = int64_t(n) * n;
    const int64_t seam_x = nwx * n - n / 2, seam_y = nwy * n - n / 2;
    std::vector<float> mask(size_t(nwx * nwy * n2 * n2), 0.0f);
    for (int64_t wy = 0; wy < nwy; ++wy)
        for (int64_t wx = 0; wx < nwx; ++wx) {
            if (wy < nwy - 1 && wx < nwx - 1) continue;
            for (int64_t a = 0; a < n2; ++a)
                for (int64_t b = 0; b < n2; ++b) {
                    const bool same_y = (wy * n + a / n < seam_y) == (wy * n + b / n < seam_y), same_x = (wx * n + a % n < seam_x) == (wx * n + b % n < seam_x);
                    if (!same_y || !same_x) mask[size_t(((wy * nwx + wx) * n2 + a) * n2 + b)] = -INFINITY;
                }
        }
    return mask;
}

} // namespace

int main(int argc, char** argv) {
    try {
        if (argc != 9) throw exception("usage: window_check <file.gguf> <block prefix> <C> <heads> <w> <h> <batch> <window>");
        const int C = std::atoi(argv[3]), heads = std::atoi(argv[4]), w = std::atoi(argv[5]), h = std::atoi(argv[6]), batch = std::atoi(argv[7]), window = std::atoi(argv[8]);
        model_file file = model_load(argv[1]);
        model_weights weights;
        model_transfer(file, weights);
        compute_graph graph = compute_graph_init(weights);
        model_ref m(graph);
        const int64_t n2 = int64_t(window) * window, nw = ((w + window - 1) / window) * ((h + window - 1) / window);
        std::vector<int32_t> idx = relative_position_index(window);
        std::vector<float> mask = attention_mask(w, h, window);
        std::string idx_name = "window_attention_" + std::to_string(window) + ".rel_pos_index";
        std::string mask_name = "swin_layer_" + std::to_string(w) + "x" + std::to_string(h) + ".attn_mask";
        compute_graph_constant(m, idx_name.c_str(), GGML_TYPE_I32, {n2 * n2, 1, 1, 1}, idx.data());
        compute_graph_constant(m, mask_name.c_str(), GGML_TYPE_F16, {n2, n2, nw, 1}, mask.data());

        tensor x = compute_graph_input(m, GGML_TYPE_F16, {C, int64_t(w) * h, batch, 1}, "tokens");
        tensor attn_mask = ggml_get_tensor(m, mask_name.c_str());
        tensor out = swin_block(m.with_prefix(argv[2]), x, attn_mask, {heads, window, w, h, window / 2});
        compute_graph_output(m, out, "block");
        compute_graph_plan(graph);
        std::fputs(compute_graph_describe(graph).c_str(), stdout);
        return 0;
    } catch (std::exception const& e) {
        std::fprintf(stderr, "window_check: %s\n", e.what());
        return 1;
    }
}
