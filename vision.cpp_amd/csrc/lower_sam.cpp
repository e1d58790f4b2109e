// Graph lowering: the nodes of the SAM prompt encoder and mask decoder (mobile-sam.cpp:210-478; see lowering.h) -- attention without a mask on q, k, v
// where the graph has them, ggml_mul_mat of two activations, sin / cos, and the Fourier-feature group of position_embedding_random.
#include "lowering.h"

#include <cmath>

namespace visp {

// ---- position_embedding_random (mobile-sam.cpp:238-248) --------------------------------------------------------------------------------
// mul_mat(constant [2, F], f32 input [2, n, ..]) -> scale(s) -> {sin, cos} -> concat(sin, cos, dim 0): ONE launch in both lowering modes, the way
// image_pad8 is. The arguments reach about +-20: as an f16 tensor between the product and the sine they would carry an absolute error near 1e-2,
// so the product, the scale and the argument reduction are done in f32 by the one kernel. The scale must be 2 pi (the kernel works in revolutions).
bool lowering::match_fourier_group(int cat, fourier_group& G) const {
    graph_node const& c = g.nodes[cat];
    if (c.op != gop_concat || c.constant || c.ip[0] != 0) return false;
    const int sn = c.src[0], cs = c.src[1];
    if (g.nodes[sn].op != gop_sin || g.nodes[cs].op != gop_cos || sole_consumer(sn) != cat || sole_consumer(cs) != cat) return false;
    const int sc = g.nodes[sn].src[0];
    if (g.nodes[cs].src[0] != sc) return false;
    graph_node const& s = g.nodes[sc];
    if (s.op != gop_scale || s.is_output || uses[sc] != 2 || fabsf(s.fp[0] - 6.28318530717958647692f) > 1e-5f) return false;
    const int mm = s.src[0];
    graph_node const& m = g.nodes[mm];
    if (m.op != gop_mul_mat || sole_consumer(mm) != sc) return false;
    graph_node const &a = g.nodes[m.src[0]], &b = g.nodes[m.src[1]];
    if (!a.constant || a.ne[0] != 2 || a.ne[2] != 1 || b.op != gop_input || b.dtype != gdt_f32) return false;
    for (int v : {sn, cs, sc, mm})
        if (!free_node(v)) return false;
    G.mm = mm; G.scale = sc; G.sin = sn; G.cos = cs;
    return true;
}
void lowering::find_sam_groups() {
    for (int t = 0; t < (int)g.nodes.size(); ++t) {
        fourier_group G;
        if (!needed[t] || !match_fourier_group(t, G)) continue;
        claim(t, {G.mm, G.scale, G.sin, G.cos});
        for (int v : {G.mm, G.scale, G.sin, G.cos}) skip[v] = 1;
        fourier_groups[t] = G;
    }
    // a K = 2 product on the f32 coordinates exists as the head of that group only
    for (int t = 0; t < (int)g.nodes.size(); ++t) {
        graph_node const& n = g.nodes[t];
        if (needed[t] && n.op == gop_mul_mat && !n.constant && g.nodes[n.src[0]].constant && !skip[t])
            throw except("mul_mat: a constant first operand with K = 2 on f32 coordinates is built as the head of mul_mat -> scale(2 pi) -> {sin, cos} -> concat(sin, cos, dim 0) only "
                         "(position_embedding_random); for any other product with a constant operand use LINEAR");
    }
}
void lowering::fourier_features(int t, fourier_group const& G) {
    graph_node& n = g.nodes[t];
    graph_node const& m = g.nodes[G.mm];
    const int at = m.src[0], xt = m.src[1];
    graph_node const& a = g.nodes[at];
    const int F = (int)a.ne[1];
    const int64_t points = g.nodes[xt].n_elements() / 2;
    // a's memory is [F][2] already (K = 2 contiguous): the values rounded to f16 -- what every weight of this layer is -- kept as f32 pairs
    const float* gauss = static_cast<const float*>(cached(at, role_fourier, [&](bool st) {
        std::vector<float> h((size_t)a.n_elements());
        for (size_t i = 0; i < h.size(); ++i) h[i] = f16_to_f32(f32_to_f16(a.values()[i]));
        return upload(h.data(), h.size() * 4, st);
    }));
    int named_src = at; // the weight behind the folded transpose, for the launch's line
    while (g.nodes[named_src].name.empty() && g.nodes[named_src].n_src > 0) named_src = g.nodes[named_src].src[0];
    const int xbuf = buf_of(xt);
    materialise(t);
    const int obuf = n.buffer;
    auto xp = ptr(xbuf), op = ptr(obuf);
    emit("fourier_features points=" + std::to_string(points) + " F=" + std::to_string(F) + " <- " + const_id(g, named_src), {xbuf}, {obuf},
         [=](void* st) { VX(vx_fourier_features_f32(reinterpret_cast<const float*>(xp()), gauss, op(), points, F, st)); });
    tag("glue", 0, (double)points * (8 + 4.0 * F));
}

// the buffer q / k / v of an attention_cross lives in: [hd * heads, T, B] rows as their producer wrote them
int lowering::token_rows(int t, const char* who) {
    if (row_stride.count(root_view(t))) throw except("%s: internal: operand %d was written with padded rows", who, t);
    return buf_of(t);
}

// softmax(scale q k^T) v on q, k, v where the graph has them (token-major rows of heads * head_dim: the reshape of a linear's output is a view): one
// launch, plus the combine launch when the keys are split (kernels_attn_cross.hip). No heads_major copies in either lowering mode.
void lowering::attention_cross(int t) {
    graph_node& n = g.nodes[t];
    graph_node const &q = g.nodes[n.src[0]], &k = g.nodes[n.src[1]];
    const int hd = (int)q.ne[0], H = (int)q.ne[1], Tq = (int)q.ne[2], Tk = (int)k.ne[2], B = (int)q.ne[3];
    const int qb = token_rows(n.src[0], "attention_cross"), kb = token_rows(n.src[1], "attention_cross"), vb = token_rows(n.src[2], "attention_cross");
    const size_t part_bytes = vx_attention_cross_partial_bytes(B, H, Tq, Tk, hd);
    const int parts = vx_attention_cross_parts(Tq, Tk);
    const int pbuf = part_bytes ? new_buffer(part_bytes) : -1;
    materialise(t);
    const int obuf = n.buffer;
    auto qp = ptr(qb), kp = ptr(kb), vp = ptr(vb), op = ptr(obuf), pp = ptr(std::max(pbuf, 0));
    const float scale = n.fp[0];
    char d[200];
    snprintf(d, sizeof d, "attention_cross B=%d heads=%d Tq=%d Tk=%d hd=%d", B, H, Tq, Tk, hd);
    if (parts == 1) {
        emit(d, {qb, kb, vb}, {obuf}, [=](void* st) { VX(vx_attention_cross_f16(qp(), kp(), vp(), op(), nullptr, 0, B, H, Tq, Tk, hd, scale, st)); });
        tag("attention", 4.0 * B * H * (double)Tq * Tk * hd, (double)B * H * ((double)Tq + Tk) * hd * 2 * 2);
        return;
    }
    emit(std::string(d) + " parts=" + std::to_string(parts), {qb, kb, vb}, {pbuf},
         [=](void* st) { VX(vx_attention_cross_step_f16(1, qp(), kp(), vp(), op(), pp(), part_bytes, B, H, Tq, Tk, hd, scale, st)); });
    tag("attention", 4.0 * B * H * (double)Tq * Tk * hd, (double)B * H * ((double)Tq + Tk) * hd * 2 * 2);
    snprintf(d, sizeof d, "attention_cross_combine B=%d heads=%d Tq=%d parts=%d hd=%d", B, H, Tq, parts, hd);
    emit(d, {pbuf}, {obuf}, [=](void* st) { VX(vx_attention_cross_step_f16(2, qp(), kp(), vp(), op(), pp(), part_bytes, B, H, Tq, Tk, hd, scale, st)); });
    tag("attention", 0, (double)part_bytes);
}

void lowering::mul_mat(int t) {
    graph_node& n = g.nodes[t];
    graph_node const &a = g.nodes[n.src[0]], &b = g.nodes[n.src[1]];
    if (a.constant || b.constant) throw except("mul_mat: internal: a product with a constant operand reached the launch"); // (find_sam_groups / graph_add refuse them)
    const int64_t M = a.ne[1];
    const int K = (int)a.ne[0], N = (int)b.ne[1], B = (int)b.ne[2], Ba = (int)a.ne[2];
    const int ab = token_rows(n.src[0], "mul_mat"), bb = token_rows(n.src[1], "mul_mat");
    materialise(t);
    const int obuf = n.buffer;
    auto ap = ptr(ab), bp = ptr(bb), op = ptr(obuf);
    char d[160];
    snprintf(d, sizeof d, "mul_mat M=%lld N=%d K=%d B=%d", (long long)M, N, K, B);
    emit(d, {ab, bb}, {obuf}, [=](void* st) { VX(vx_mul_mat_f16(ap(), bp(), op(), M, N, K, B, Ba, st)); });
    tag("glue", 2.0 * M * N * K * B, ((double)M * K * Ba + (double)N * K * B + (double)M * N * B) * 2);
}

void lowering::sincos(int t) {
    graph_node& n = g.nodes[t];
    if (g.nodes[n.src[0]].dtype != gdt_f16) throw except("%s: the operand is f32; sin / cos are built on f16 activations", graph_op_name(n.op));
    const int64_t cnt = n.n_elements();
    const int mode = n.op == gop_cos ? 1 : 0;
    map_launch(t, std::string(graph_op_name(n.op)) + " n=" + std::to_string(cnt), [=](char* x, char* o, char*, void* st) { VX(vx_sincos_f16(mode, x, o, cnt, st)); });
    tag("glue", 0, (double)cnt * 4);
}

} // namespace visp
