// Graph lowering: what BiRefNet written against this layer needs beyond a decoder block (birefnet.cpp:20-73, 147-260; see lowering.h).
//   (a) interpolate(bilinear | align_corners) of an f32 image and image_patches are one launch each of kernels_imgops.hip, in both lowering modes;
//   (b) conv_2d(1x1 to one channel) -> sigmoid -> [repeat to p's shape] -> mul(p, .), each link read by the next one only (the gdt gate, birefnet.cpp:189-192), is
//       one pixel_gate launch on the rows of p and of the conv's input;
//   (c) the sources of a channel concat that a bilinear | align_corners resize or a LayerNorm writes are written into their slice of the concat's buffer
//       (encode_concat, birefnet.cpp:43-65): lower_yolo.cpp's cat_slot / concat_in_place machinery with two more launches that can write through a pixel stride.
// (b) and (c) with fused models only; without them every node is one launch.
#include "lowering.h"

namespace visp {

// ---- (a) ------------------------------------------------------------------------------------------------------------------------------------------------------

void lowering::image_resize(int t) {
    graph_node const& n = g.nodes[t];
    graph_node const& x = g.nodes[n.src[0]];
    const int B = (int)x.ne[3], H = (int)x.ne[2], W = (int)x.ne[1], C = (int)x.ne[0], OH = (int)n.ne[2], OW = (int)n.ne[1];
    char d[160];
    snprintf(d, sizeof d, "image_bilinear_ac %dx%d -> %dx%d C=%d B=%d", W, H, OW, OH, C, B);
    map_launch(t, d, [=](char* xp, char* o, char*, void* st) { VX(vx_image_bilinear_ac_f32(reinterpret_cast<const float*>(xp), reinterpret_cast<float*>(o), B, H, W, C, OH, OW, st)); });
    tag("preprocess", (double)n.n_elements() * 6, (double)(x.n_elements() + n.n_elements()) * 4);
}

void lowering::image_patches(int t) {
    graph_node const& n = g.nodes[t];
    graph_node const& x = g.nodes[n.src[0]];
    const int B = (int)x.ne[3], IH = (int)x.ne[2], IW = (int)x.ne[1], C = (int)x.ne[0], h = (int)n.ne[2], w = (int)n.ne[1];
    char d[200];
    snprintf(d, sizeof d, "image_patches %dx%d -> %dx%d grid %dx%d C=%d -> %lld B=%d", IW, IH, w, h, IW / w, IH / h, C, (long long)n.ne[0], B);
    map_launch(t, d, [=](char* xp, char* o, char*, void* st) { VX(vx_image_patches_f16(reinterpret_cast<const float*>(xp), o, B, IH, IW, C, h, w, 0, st)); });
    tag("preprocess", 0, (double)x.n_elements() * 4 + (double)n.n_elements() * 2);
}

// ---- (b) ------------------------------------------------------------------------------------------------------------------------------------------------------

bool lowering::match_gate_group(int t, gate_group& G) const {
    graph_node const& m = g.nodes[t];
    if (m.op != gop_mul || m.constant || m.dtype != gdt_f16 || m.ne[0] % 8) return false;
    const int gate_at = g.nodes[m.src[0]].op == gop_repeat || g.nodes[m.src[0]].op == gop_sigmoid ? 0 : 1; // (graph_add puts the larger operand first; equal ones stay)
    G.p = m.src[1 - gate_at];
    int v = m.src[gate_at];
    graph_node const& p = g.nodes[G.p];
    if (p.constant || p.dtype != gdt_f16 || !same_shape(p, m)) return false;
    if (g.nodes[v].op == gop_repeat) { // ggml's broadcast of the one-channel gate written out: [1, W, H, N] -> [C, W, H, N]
        if (!free_node(v) || sole_consumer(v) != t || g.nodes[v].constant) return false;
        G.rep = v;
        v = g.nodes[v].src[0];
    }
    graph_node const& s = g.nodes[v];
    if (s.op != gop_sigmoid || s.constant || !free_node(v) || sole_consumer(v) != (G.rep >= 0 ? G.rep : t)) return false;
    if (s.ne[0] != 1 || s.ne[1] != m.ne[1] || s.ne[2] != m.ne[2] || s.ne[3] != m.ne[3]) return false;
    G.sig = v;
    G.conv = s.src[0];
    graph_node const& c = g.nodes[G.conv];
    if (c.op != gop_conv_2d || c.constant || c.dtype != gdt_f32 || !free_node(G.conv) || sole_consumer(G.conv) != G.sig) return false;
    graph_node const &w = g.nodes[c.src[1]], &a = g.nodes[c.src[0]];
    if (w.ne[1] != 1 || w.ne[2] != 1 || w.ne[3] != 1 || c.ip[0] != 1 || c.ip[1] != 0 || (c.n_src == 3 && !g.nodes[c.src[2]].constant)) return false;
    return !a.constant && a.dtype == gdt_f16 && a.ne[0] % 8 == 0 && c.src[0] != t;
}

void lowering::find_birefnet_groups() {
    if (!g.fused_models) return;
    const int N = (int)g.nodes.size();
    for (int t = 0; t < N; ++t) { // (b)
        gate_group G;
        if (!needed[t] || !free_node(t) || !match_gate_group(t, G)) continue;
        gate_groups[t] = G;
        for (int c : {G.conv, G.sig, G.rep})
            if (c >= 0) skip[c] = 1;
        claim(t, {G.conv, G.sig, G.rep});
    }
}

void lowering::pixel_gate(int t, gate_group const& G) {
    graph_node& n = g.nodes[t];
    graph_node const& c = g.nodes[G.conv];
    const int as = c.src[0];
    const int C = (int)n.ne[0], Cg = (int)g.nodes[as].ne[0];
    const int64_t rows = n.n_elements() / C;
    const float* w = const_f32(c.src[1]);
    const float bias = c.n_src == 3 ? g.nodes[c.src[2]].values()[0] : 0.0f;
    auto where = [&](int v) { // a map in a buffer of its own (its rows padded for a GEMM reader, perhaps), or inside a wider one
        located L = locate(v);
        if (auto it = row_stride.find(root_view(v)); it != row_stride.end()) L.pix = it->second;
        return L;
    };
    const located P = where(G.p), A = where(as);
    absorb(std::vector<int>{G.conv, G.sig, G.rep}, t);
    materialise(t);
    const int obuf = n.buffer;
    auto pp = ptr(P.buf), ap = ptr(A.buf), op = ptr(obuf);
    const int64_t p_off = P.off, p_pix = P.pix, a_off = A.off, a_pix = A.pix;
    char d[320];
    snprintf(d, sizeof d, "pixel_gate M=%lld C=%d Cg=%d <- %s", (long long)rows, C, Cg, weight_name(g, c).c_str());
    emit(d, {P.buf, A.buf}, {obuf}, [=](void* st) { VX(vx_pixel_gate_f16(pp() + p_off * 2, p_pix, ap() + a_off * 2, a_pix, w, bias, op(), C, rows, C, Cg, st)); });
    tag("glue", (double)rows * (2.0 * Cg + C), (double)rows * (2.0 * C + Cg) * 2);
}

// ---- (c) ------------------------------------------------------------------------------------------------------------------------------------------------------

// the LayerNorm behind the concat source v (a view of it that keeps the pixel width), when nothing else reads either: its launch can write the concat's slice
int lowering::norm_behind(int v) const {
    graph_node const& r = g.nodes[v];
    if (r.op != gop_reshape || r.constant || r.is_output || sole_consumer(v) < 0) return -1;
    const int ln = r.src[0];
    graph_node const& n = g.nodes[ln];
    if (n.op != gop_layer_norm || n.constant || n.is_output || n.dtype != gdt_f16 || n.ne[0] != r.ne[0] || n.ne[0] % 8 || n.ne[0] > 1024 || sole_consumer(ln) != v || !free_node(ln)) return -1;
    return ln;
}

// bilinear | align_corners that writes into its slice of a concat (its source may lie inside a wider map)
void lowering::bilinear_in_place(int t) {
    graph_node& n = g.nodes[t];
    graph_node const& x = g.nodes[n.src[0]];
    const int B = (int)x.ne[3], H = (int)x.ne[2], W = (int)x.ne[1], C = (int)x.ne[0], OH = (int)n.ne[2], OW = (int)n.ne[1];
    const located in = locate(n.src[0]);
    const located out = output_slot(t, t);
    char d[256];
    snprintf(d, sizeof d, "bilinear_ac[out ch %lld..%lld of %lld] %dx%d -> %dx%d C=%d", (long long)out.off, (long long)(out.off + C), (long long)out.pix, W, H, OW, OH, C);
    auto xp = ptr(in.buf), op = ptr(out.buf);
    const int64_t in_off = in.off, in_pix = in.pix, out_off = out.off, out_pix = out.pix;
    emit(d, {in.buf}, {out.buf}, [=](void* st) { VX(vx_bilinear_ac_pix_f16(xp() + in_off * 2, in_pix, op() + out_off * 2, out_pix, B, H, W, C, OH, OW, st)); });
    tag("bilinear", 0, (double)B * ((double)H * W + (double)OH * OW) * C * 2);
}

void lowering::layer_norm_in_place(int t) {
    graph_node& n = g.nodes[t];
    const int C = (int)n.ne[0];
    float *w = const_f32(n.src[1]), *b = const_f32(n.src[2]);
    const int64_t rows = n.n_elements() / C;
    const float eps = n.fp[0];
    const int xbuf = buf_of(n.src[0]);
    const located out = output_slot(t, t);
    auto xp = ptr(xbuf), op = ptr(out.buf);
    const int64_t out_off = out.off, out_pix = out.pix;
    char d[256];
    snprintf(d, sizeof d, "layer_norm[out ch %lld..%lld of %lld] rows=%lld C=%d%s%s", (long long)out.off, (long long)(out.off + C), (long long)out.pix, (long long)rows, C, n.name.empty() ? "" : " <- ",
             n.name.c_str());
    emit(d, {xbuf}, {out.buf}, [=](void* st) { VX(vx_layernorm_pix_f16(xp(), w, b, op() + out_off * 2, out_pix, rows, C, eps, st)); });
    tag("layernorm", 0, (double)rows * C * 4);
}

} // namespace visp
