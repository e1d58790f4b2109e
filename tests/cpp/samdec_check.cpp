// One two-way attention block and the whole mask prediction of the SAM mask decoder written against include/visp/nn.h with the ggml names
// (VISP_GGML_NAMES) -- the node sequences the reference's arch code emits (src/visp/arch/mobile-sam.cpp:294-478), with its writes into views
// (ggml_cpy / ggml_add_inplace on a slice) as concats, since this layer is functional -- over the weights of a decoder GGUF given on the command line:
//   samdec_check <file.gguf> <block | masks> <channels> <map side> <prompt tokens> <batch> <fused models 0 | 1>
// Host only: the graph is planned without a device and its launch list (compute_graph_describe) goes to stdout, where
// tests/test_graph_samdec_cpu.py compares it with the Python face's for the same weights. Built by __graft_entry__.build().
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <tuple>
#include <utility>

#define VISP_GGML_NAMES
#include "visp/nn.h"

using namespace visp;

namespace {

constexpr int kHeads = 8;

// three projections, heads split off the channel dimension (a view), softmax(q k^T / sqrt(d)) v for any token counts, output projection
tensor projected_attention(model_ref m, tensor q_in, tensor k_in, tensor v_in) {
    auto heads_of = [&](char const* name, tensor t) {
        tensor p = linear(m[name], t);
        return ggml_reshape_4d(m, p, p->ne[0] / kHeads, kHeads, p->ne[1], p->ne[2]);
    };
    tensor q = heads_of("q_proj", q_in), k = heads_of("k_proj", k_in), v = heads_of("v_proj", v_in);
    return attention_cross(m, q, k, v, 1.0f / std::sqrt(float(q->ne[0])), m["out_proj"]);
}

tensor two_layer_mlp(model_ref m, tensor t) { return linear(m["lin2"], ggml_relu_inplace(m, linear(m["lin1"], t))); }

// tokens attend to themselves, then to the map, an MLP, then the map attends to the tokens; a LayerNorm behind each of the four steps
std::pair<tensor, tensor> two_way_block(model_ref m, tensor tokens, tensor map, tensor token_pe, tensor map_pe, bool first) {
    if (first) tokens = projected_attention(m["self_attn"], tokens, tokens, tokens);
    else {
        tensor with_pe = ggml_add(m, tokens, token_pe);
        tokens = ggml_add(m, tokens, projected_attention(m["self_attn"], with_pe, with_pe, tokens));
    }
    tokens = layer_norm(m["norm1"], tokens);
    tensor tq = ggml_add(m, tokens, token_pe), mk = ggml_add(m, map, map_pe);
    tokens = layer_norm(m["norm2"], ggml_add_inplace(m, tokens, projected_attention(m["cross_attn_t2i"], tq, mk, map)));
    tokens = layer_norm(m["norm3"], ggml_add_inplace(m, tokens, two_layer_mlp(m["mlp"], tokens)));
    tokens = ggml_cont(m, tokens);
    tq = ggml_add(m, tokens, token_pe);
    map = layer_norm(m["norm4"], ggml_add_inplace(m, map, projected_attention(m["cross_attn_i2t"], mk, tq, tokens)));
    return {tokens, map};
}

tensor relu_mlp(model_ref m, tensor t, int layers) {
    for (int i = 0; i < layers; ++i) {
        t = linear(m["layers"][i], t);
        if (i + 1 < layers) t = ggml_relu_inplace(m, t);
    }
    return t;
}

// embed [C, side, side, 1], prompt [C, n, B], the no-mask embedding [C] -> masks [4 side, 4 side, 4, B], quality [4, B]
std::pair<tensor, tensor> mask_prediction(model_ref m, tensor embed, tensor prompt, tensor no_mask) {
    const int64_t batch = prompt->ne[2], ch = embed->ne[0], side_w = embed->ne[1], side_h = embed->ne[2];
    tensor out_tokens = ggml_concat(m, m.weights("iou_token.weight"), m.weights("mask_tokens.weight"), 1);
    out_tokens = ggml_repeat_4d(m, out_tokens, out_tokens->ne[0], out_tokens->ne[1], batch, 1);
    tensor tokens = ggml_concat(m, out_tokens, prompt, 1);
    tensor map = ggml_add_inplace(m, ggml_repeat_4d(m, embed, ch, side_w, side_h, batch), no_mask);
    tensor pe = m.weights("dense_positional_embedding");
    pe = ggml_repeat_4d(m, pe, pe->ne[0], pe->ne[1], pe->ne[2], batch);

    model_ref tr = m["transformer"];
    tensor map_rows = ggml_reshape_3d(m, map, ch, side_w * side_h, batch), pe_rows = ggml_reshape_3d(m, pe, ch, side_w * side_h, batch);
    tensor q = tokens;
    for (int i = 0; i < 2; ++i) std::tie(q, map_rows) = two_way_block(tr["layers"][i], q, map_rows, tokens, pe_rows, i == 0);
    tensor tq = ggml_add(m, q, tokens), mk = ggml_add(m, map_rows, pe_rows);
    q = layer_norm(tr["norm_final_attn"], ggml_add_inplace(m, q, projected_attention(tr["final_attn_t2i"], tq, mk, map_rows)));

    tensor quality_token = ggml_reshape_3d(m, slice(m, q, {}, 0), q->ne[0], batch, 1);
    tensor mask_tokens = slice(m, q, {}, {1, 5});
    model_ref up = m["output_upscaling"];
    tensor fine = conv_transpose_2d(up[0], ggml_reshape_4d(m, map_rows, ch, side_w, side_h, batch), 2);
    fine = ggml_gelu_inplace(m, layer_norm(up[1], fine));
    fine = ggml_gelu_inplace(m, conv_transpose_2d(up[3], fine, 2));
    const int64_t fw = fine->ne[1], fh = fine->ne[2];
    fine = ggml_reshape_3d(m, fine, fine->ne[0], fw * fh, batch);
    model_ref hyper = m["output_hypernetworks_mlps"];
    tensor rows[4];
    for (int i = 0; i < 4; ++i) rows[i] = relu_mlp(hyper[i], slice(m, mask_tokens, {}, i), 3);
    tensor masks = ggml_mul_mat(m, fine, concat(m, {rows[0], rows[1], rows[2], rows[3]}, 1));
    masks = ggml_reshape_4d(m, masks, fw, fh, masks->ne[1], batch);
    return {masks, relu_mlp(m["iou_prediction_head"], quality_token, 3)};
}

} // namespace

int main(int argc, char** argv) {
    try {
        if (argc != 8) throw exception("usage: samdec_check <file.gguf> <block | masks> <channels> <map side> <prompt tokens> <batch> <fused models 0 | 1>");
        const int64_t ch = std::atoi(argv[3]), side = std::atoi(argv[4]), n = std::atoi(argv[5]), batch = std::atoi(argv[6]);
        model_file file = model_load(argv[1]);
        model_weights weights;
        model_transfer(file, weights);
        compute_graph graph = compute_graph_init(weights);
        model_ref m(graph);
        model_ref dec = m["dec"];
        if (std::strcmp(argv[2], "block") == 0) {
            tensor tokens = compute_graph_input(m, GGML_TYPE_F16, {ch, n, batch, 1}, "tokens");
            tensor token_pe = compute_graph_input(m, GGML_TYPE_F16, {ch, n, batch, 1}, "token_pe");
            tensor map = compute_graph_input(m, GGML_TYPE_F16, {ch, side * side, batch, 1}, "map");
            tensor map_pe = compute_graph_input(m, GGML_TYPE_F16, {ch, side * side, batch, 1}, "map_pe");
            auto [t, k] = two_way_block(dec["transformer"]["layers"][1], tokens, map, token_pe, map_pe, false);
            compute_graph_output(m, t, "queries");
            compute_graph_output(m, k, "keys");
        } else {
            tensor embed = compute_graph_input(m, GGML_TYPE_F16, {ch, side, side, 1}, "embed");
            tensor prompt = compute_graph_input(m, GGML_TYPE_F16, {ch, n, batch, 1}, "prompt");
            auto [masks, quality] = mask_prediction(dec, embed, prompt, m["prompt_encoder"].weights("no_mask_embed.weight"));
            compute_graph_output(m, masks, "masks");
            compute_graph_output(m, quality, "iou");
        }
        detail::check(visp_graph_set_fused_models(graph.handle, std::atoi(argv[7])));
        compute_graph_plan(graph);
        std::fputs(compute_graph_describe(graph).c_str(), stdout);
        return 0;
    } catch (std::exception const& e) {
        std::fprintf(stderr, "samdec_check: %s\n", e.what());
        return 1;
    }
}
