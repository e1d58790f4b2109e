// Graph lowering: the nodes of the SAM3 vision and text encoders (sam3.h:221-231, 413-455; see lowering.h) -- ROPE on its own, the rope_2d group of
// apply_rope_2d as one launch, that group inside the fused q|k|v chain as one in-place launch on the head-major q and k buffers, and get_rows with an
// index that is a graph input.
#include "lowering.h"

#include <cmath>

namespace visp {

// cos | sin of theta = pos[t] * scale * base^(-2 i / n) for pair i of token t: f32 [T][n], cos in [0, n / 2), sin in [n / 2, n). Computed in double from the
// constant positions and rounded once, so the device never evaluates a transcendental. One image per (positions, n, base, scale).
float* lowering::rope_table(int pos_t, int n, float base, float scale) {
    graph_node const& pos = g.nodes[pos_t];
    char with[96];
    snprintf(with, sizeof with, "rope:%d:%.9g:%.9g", n, (double)base, (double)scale);
    return static_cast<float*>(cached(pos_t, role_rope_table, [&](bool st) {
        const int64_t T = pos.ne[0];
        std::vector<float> h((size_t)(T * n));
        for (int i = 0; i < n / 2; ++i) {
            const double freq = (double)scale * std::pow((double)base, -2.0 * i / n);
            for (int64_t t = 0; t < T; ++t) {
                const double theta = (double)pos.values()[t] * freq;
                h[(size_t)(t * n + i)] = (float)std::cos(theta);
                h[(size_t)(t * n + n / 2 + i)] = (float)std::sin(theta);
            }
        }
        return upload(h.data(), h.size() * 4, st);
    }, with));
}

// ---- the rope_2d group (sam3.h:413-438) --------------------------------------------------------------------------------------------------
// concat(rope(slice(r, 0 : hd / 2), px), rope(slice(r, hd / 2 : hd), py), dim 0) on r [hd, heads, T, B], the inner nodes read by nothing else, the two
// ropes with equal base and scale: one vx_rope2d_f16 launch instead of two slice copies, two rotations and two concat copies.
bool lowering::match_rope2d_group(int cat, rope2d_group& G) const {
    graph_node const& c = g.nodes[cat];
    if (c.op != gop_concat || c.constant || c.ip[0] != 0 || !free_node(cat)) return false;
    int src = -1;
    for (int i = 0; i < 2; ++i) {
        const int rp = c.src[i];
        graph_node const& r = g.nodes[rp];
        if (r.op != gop_rope || sole_consumer(rp) != cat || !free_node(rp)) return false;
        const int sl = r.src[0];
        graph_node const& s = g.nodes[sl];
        if (s.op != gop_slice || sole_consumer(sl) != rp || !free_node(sl)) return false;
        graph_node const& x = g.nodes[s.src[0]];
        const int64_t half = x.ne[0] / 2;
        if (x.constant || x.dtype != gdt_f16 || x.ne[0] % 16 || s.ne[0] != half || s.ip[0] != i * half || s.ip[2] != 1) return false;
        for (int d = 1; d < 4; ++d)
            if (s.ip[3 * d] != 0 || s.ip[3 * d + 2] != 1 || s.ne[d] != x.ne[d]) return false;
        if (i == 0) src = s.src[0];
        else if (s.src[0] != src) return false;
        G.rope[i] = rp;
        G.slice[i] = sl;
    }
    graph_node const &r0 = g.nodes[G.rope[0]], &r1 = g.nodes[G.rope[1]];
    if (r0.fp[0] != r1.fp[0] || r0.fp[1] != r1.fp[1]) return false;
    graph_node const& x = g.nodes[src];
    const int64_t si[3] = {x.ne[0], x.ne[0] * x.ne[1], x.ne[0] * x.ne[1] * x.ne[2]};
    if (!vx_rope2d_supported((int)x.ne[0], (int)x.ne[1], (int)x.ne[2], (int)x.ne[3], si, si)) return false; // rows of the whole head, as the launcher checks them
    G.src = src;
    return true;
}
// before find_qkv_groups: the fused q|k|v chain walks through these groups
void lowering::find_sam3_groups() {
    if (!g.fused_models) return;
    for (int t = 0; t < (int)g.nodes.size(); ++t) {
        rope2d_group G;
        if (!needed[t] || !match_rope2d_group(t, G)) continue;
        claim(t, {G.rope[0], G.rope[1], G.slice[0], G.slice[1]});
        for (int v : {G.rope[0], G.rope[1], G.slice[0], G.slice[1]}) skip[v] = 1;
        rope2d_groups[t] = G;
    }
}
// the group on its own: r where the graph has it (token-major) in, a buffer of the concat's out
void lowering::rope2d(int t, rope2d_group const& G) {
    graph_node& n = g.nodes[t];
    graph_node const& x = g.nodes[G.src];
    graph_node const& r = g.nodes[G.rope[0]];
    const int hd = (int)x.ne[0], H = (int)x.ne[1], T = (int)x.ne[2], B = (int)x.ne[3];
    const float *tx = rope_table(r.src[1], hd / 2, r.fp[0], r.fp[1]), *ty = rope_table(g.nodes[G.rope[1]].src[1], hd / 2, r.fp[0], r.fp[1]);
    const int xbuf = token_rows(G.src, "rope_2d");
    materialise(t);
    const int obuf = n.buffer;
    auto xp = ptr(xbuf), op = ptr(obuf);
    const std::array<int64_t, 3> S{hd, (int64_t)hd * H, (int64_t)hd * H * T};
    char d[160];
    snprintf(d, sizeof d, "rope_2d hd=%d heads=%d T=%d B=%d", hd, H, T, B);
    emit(d, {xbuf}, {obuf}, [=](void* st) { VX(vx_rope2d_f16(xp(), op(), nullptr, nullptr, tx, ty, hd, H, T, B, S.data(), S.data(), 1.0f, st)); });
    tag("rope", 6.0 * n.n_elements() / 2, (double)n.n_elements() * 4);
}
// the group inside the fused q|k|v chain: one launch, in place on the head-major q and k buffers the product's epilogue wrote (q pre-scaled there: a
// rotation is linear, the factor commutes with it)
void lowering::rope2d_in_place(int att, std::array<int, 3> const& hb) {
    auto const& cats = qkv_rope.at(att);
    rope2d_group const& G = rope2d_groups.at(cats[0]);
    graph_node const& x = g.nodes[G.src];
    graph_node const& r = g.nodes[G.rope[0]];
    const int hd = (int)x.ne[0], H = (int)x.ne[1], T = (int)x.ne[2], B = (int)x.ne[3];
    const float *tx = rope_table(r.src[1], hd / 2, r.fp[0], r.fp[1]), *ty = rope_table(g.nodes[G.rope[1]].src[1], hd / 2, r.fp[0], r.fp[1]);
    for (int c : cats) skip[c] = 1; // the inner nodes are skipped since the group was found; the concats have no buffer: attention reads hb
    auto qp = ptr(hb[0]), kp = ptr(hb[1]);
    const std::array<int64_t, 3> S{(int64_t)hd * T, hd, (int64_t)hd * T * H}; // (head, token, batch) of [B][H][T][hd]
    char d[160];
    snprintf(d, sizeof d, "rope_2d[q k heads-major, in place] hd=%d heads=%d T=%d B=%d", hd, H, T, B);
    emit(d, {hb[0], hb[1]}, {hb[0], hb[1]}, [=](void* st) { VX(vx_rope2d_f16(qp(), qp(), kp(), kp(), tx, ty, hd, H, T, B, S.data(), S.data(), 1.0f, st)); });
    tag("rope", 6.0 * hd * H * T * B, (double)hd * H * T * B * 2 * 4);
}

// ---- the nodes on their own ---------------------------------------------------------------------------------------------------------------
void lowering::rope(int t) {
    graph_node& n = g.nodes[t];
    const int nd = (int)n.ne[0], H = (int)n.ne[1], T = (int)n.ne[2], B = (int)n.ne[3];
    const std::array<int64_t, 3> S{nd, (int64_t)nd * H, (int64_t)nd * H * T};
    if (!vx_rope_supported(nd, H, T, B, S.data(), S.data())) throw except("rope: %s is outside the kernel's range (32-bit indexing)", shape_str(n.ne).c_str());
    const float* tab = rope_table(n.src[1], nd, n.fp[0], n.fp[1]);
    const int xbuf = token_rows(n.src[0], "rope");
    materialise(t);
    const int obuf = n.buffer;
    auto xp = ptr(xbuf), op = ptr(obuf);
    char d[160];
    snprintf(d, sizeof d, "rope n=%d heads=%d T=%d B=%d", nd, H, T, B);
    emit(d, {xbuf}, {obuf}, [=](void* st) { VX(vx_rope_f16(xp(), op(), tab, nd, H, T, B, S.data(), S.data(), 1.0f, st)); });
    tag("rope", 3.0 * n.n_elements(), (double)n.n_elements() * 4);
}

// get_rows with an index that is an i32 graph input (the token ids of clip_text_embed, sam3.h:225) on a constant table: the table's f16 image is made once
// like any weight image, the gather is one launch and gives an f16 activation
void lowering::get_rows(int t) {
    graph_node& n = g.nodes[t];
    graph_node const &tab = g.nodes[n.src[0]], &idx = g.nodes[n.src[1]];
    if (!tab.constant)
        throw except("get_rows: a non-constant operand; get_rows is folded on the host from a constant table and a constant index (get_rows on activations is not built)");
    if (idx.op != gop_input || idx.dtype != gdt_i32) throw except("get_rows: internal: the index of a gather at run time is an i32 graph input");
    const int C = (int)tab.ne[0];
    const int64_t rows = tab.ne[1], cnt = idx.n_elements();
    void* image = const_f16(n.src[0]);
    const int ibuf = buf_of(n.src[1]);
    materialise(t);
    const int obuf = n.buffer;
    auto ip = ptr(ibuf), op = ptr(obuf);
    emit("get_rows rows=" + std::to_string(rows) + " C=" + std::to_string(C) + " n=" + std::to_string(cnt) + " <- " + const_id(g, n.src[0]), {ibuf}, {obuf},
         [=](void* st) { VX(vx_get_rows_f16(image, reinterpret_cast<const int32_t*>(ip()), op(), rows, C, cnt, st)); });
    tag("glue", 0, (double)cnt * C * 4);
}

} // namespace visp
