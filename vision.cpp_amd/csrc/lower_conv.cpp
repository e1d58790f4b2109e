// Graph lowering: matrix products and convolutions, their fused epilogues and the patterns around them (see lowering.h).
#include "lowering.h"

namespace visp {

namespace {

// A/B switches of the conv lowerings, read once
struct switches {
    bool no_dconv = getenv("VISP_NO_DCONV") != nullptr;
    int dconv_min_w = getenv("VISP_DCONV_MIN_W") ? atoi(getenv("VISP_DCONV_MIN_W")) : 16; // narrower maps take the GEMM family's conv forms
    bool no_rcu_fuse = getenv("VISP_NO_RCU_FUSE") != nullptr;
    int halo_min_w = getenv("VISP_HALO_MIN_W") ? atoi(getenv("VISP_HALO_MIN_W")) : 96;
    bool no_bil_fuse = getenv("VISP_NO_BIL_FUSE") != nullptr;
};
switches const& env() {
    static const switches s;
    return s;
}

const char* act_name(int a) { return a == 1 ? "gelu" : (a == 2 ? "relu" : ""); }

} // namespace

bool is_conv3x3(graph_node const& c, graph_node const& w) {
    return c.op == gop_conv_2d && w.constant && w.ne[1] == 3 && w.ne[2] == 3 && c.ip[0] == 1 && c.ip[1] == 1;
}
bool same_shape(graph_node const& a, graph_node const& b) { return a.ne[0] == b.ne[0] && a.ne[1] == b.ne[1] && a.ne[2] == b.ne[2] && a.ne[3] == b.ne[3]; }

// ---- the one launch of the GEMM family ---------------------------------------------------------------------------------------------------------

// The plan as a launch: its reads and writes (A's buffer among the writes where its slack is zeroed first), the closure that puts the run-time
// addresses into a copy of the arguments, its timing group and work. Every behaviour comes from a field of the plan.
void lowering::emit_product(product const& P) {
    std::vector<int> reads = {P.in.buf}, writes;
    std::function<char*()> xp = ptr(P.in.buf), op, r1, r2, qp, kp, vp;
    if (P.out.buf >= 0) { writes.push_back(P.out.buf); op = ptr(P.out.buf); }
    if (P.qkv[0] >= 0) {
        writes.insert(writes.end(), P.qkv.begin(), P.qkv.end());
        qp = ptr(P.qkv[0]); kp = ptr(P.qkv[1]); vp = ptr(P.qkv[2]);
    }
    if (P.zero_at) writes.push_back(P.in.buf);
    if (P.res1.buf >= 0) { reads.push_back(P.res1.buf); r1 = ptr(P.res1.buf); }
    if (P.res2 >= 0) { reads.push_back(P.res2); r2 = ptr(P.res2); }
    emit(P.desc, reads, writes, [=](void* st) { // (the closure keeps its own copy of the plan)
        vx_gemm_args r = P.a;
        r.A = xp() + P.in.off * 2;
        if (op) r.out = op() + P.out.off * 2;
        if (r1) r.res1 = r1() + P.res1.off * 2;
        if (r2) r.res2 = r2();
        if (qp) { r.q = qp(); r.k = kp(); r.vt = vp(); }
        if (P.zero_at) VX(vx_memset(xp() + P.zero_at, 0, 128, st));
        if (P.halo && vx_conv3x3_supported(&r)) VX(vx_conv3x3_f16(&r, st));
        else VX(vx_gemm_f16(&r, st));
    });
    tag(P.group.c_str(), P.flops, P.bytes);
}
// the implicit conv's geometry: conv node n (conv_2d, or a conv_2d_deform whose offsets are computed with its kernel's extent) on x with kernel w
void lowering::conv_geometry(vx_gemm_args& a, graph_node const& n, graph_node const& x, graph_node const& w) const {
    a.conv_kh = (int)w.ne[2]; a.conv_kw = (int)w.ne[1]; a.conv_stride = (int)n.ip[0]; a.conv_pad = (int)n.ip[1];
    a.conv_H = (int)x.ne[2]; a.conv_W = (int)x.ne[1]; a.conv_Cin = image8_input(x) ? 8 : (int)x.ne[0];
    a.conv_OH = (int)n.ne[2]; a.conv_OW = (int)n.ne[1];
}
// the operand of conv / linear / patch_embed node n: its kernel's rows (LayerScale scale_t folded in), laid out for 8-channel image pixels, or folded
// with the 1x1 conv rep1 of a RepConv
void lowering::pack_conv_rows(product& P, graph_node const& n, bool image8_in, int rep1, int scale_t) {
    const int wt = n.src[1], bt = n.n_src == 3 ? n.src[2] : -1;
    if (rep1 >= 0) P.operand(pack_rep_conv(wt, bt, g.nodes[rep1].src[1], g.nodes[rep1].n_src == 3 ? g.nodes[rep1].src[2] : -1));
    else P.operand(image8_in ? pack_image8(wt, bt, (int)n.ne[0]) : pack_rows(wt, bt, (int)n.ne[0], scale_t));
}

// the epilogue behind a matrix product: [* LayerScale] [gelu | relu] then up to two [+ residual]; `res_after_relu` false: an add behind a
// relu stays a launch
lowering::epilogue lowering::match_epilogue(int t, bool allow_gelu, bool allow_scale, bool allow_two, bool res_after_relu) const {
    epilogue e;
    e.last = t;
    int c = sole_consumer(t);
    auto take = [&](int node) { e.absorbed.push_back(node); e.last = node; c = sole_consumer(node); };
    // where a tensor lives once the nodes matched so far are absorbed into t
    auto rt = [&](int v) { v = root(v); return std::find(e.absorbed.begin(), e.absorbed.end(), v) != e.absorbed.end() ? t : v; };
    if (allow_scale && c >= 0 && g.nodes[c].op == gop_mul) { // LayerScale behind a linear (dino.cpp:48-50): folded into the weights
        graph_node const& mu = g.nodes[c];
        const int v = rt(mu.src[0]) == t ? mu.src[1] : mu.src[0];
        if (g.nodes[v].constant && g.nodes[v].n_elements() == g.nodes[t].ne[0] && rt(mu.src[0]) == t) {
            e.scale = v;
            take(c);
        }
    }
    if (e.scale < 0 && c >= 0 && ((g.nodes[c].op == gop_gelu && allow_gelu) || g.nodes[c].op == gop_relu)) {
        e.act = g.nodes[c].op == gop_gelu ? 1 : 2;
        take(c);
    }
    // up to two residual adds (dpt::residual_conv's skip, then feature_fusion's x0 + ..., depth-anything.cpp:15-33)
    for (int round = 0; round < 2 && c >= 0 && g.nodes[c].op == gop_add && e.act != 1 && (e.act == 0 || res_after_relu); ++round) {
        graph_node const& a = g.nodes[c];
        const int other = rt(a.src[0]) == t ? a.src[1] : a.src[0];
        if (!residual_ready(other, t)) break;
        if (round == 1 && !allow_two) break;
        (round == 0 ? e.res : e.res2) = other;
        take(c);
    }
    return e;
}
// the matched nodes (entries < 0 are left out) are computed by `into`'s launch: they share its buffer, and an output among them keeps it
void lowering::absorb(std::vector<int> const& nodes, int into) {
    for (int c : nodes) {
        if (c < 0) continue;
        skip[c] = 1;
        g.nodes[c].alias_of = into;
        if (g.nodes[c].is_output) g.nodes[into].is_output = true;
    }
}
// `other` can be the residual operand of the epilogue of t's launch: an f16 map of t's shape, in an NHWC buffer before that launch runs
bool lowering::residual_ready(int other, int t) const {
    graph_node const& o = g.nodes[other];
    return !o.constant && o.dtype == gdt_f16 && root(other) != root(t) && root(other) < t /* already computed when this launch runs */ && same_shape(o, g.nodes[t]) &&
           g.nodes[root(other)].buffer >= 0;
}
// the residual operands of an epilogue: their buffers join `reads`, their addresses are taken when the launch runs
lowering::residual_ptrs lowering::read_residuals(epilogue const& e, std::vector<int>& reads) {
    residual_ptrs r;
    if (e.res >= 0) { reads.push_back(buf_of(e.res)); r.res1 = ptr(reads.back()); }
    if (e.res2 >= 0) { reads.push_back(buf_of(e.res2)); r.res2 = ptr(reads.back()); }
    return r;
}

// a plain-GEMM A operand whose row length is not a multiple of 64 is copied into zero-padded rows first (the kernel reads whole
// 64-wide k tiles; the weights' padding columns are zero, but 0 * garbage must not be NaN)
int lowering::padded_rows(int t, int K, int Kp, int64_t M, std::string const& who) {
    const int src = buf_of(t);
    if (K == Kp) return src;
    const int dst = new_buffer((size_t)M * Kp * 2);
    auto sp = ptr(src), dp = ptr(dst);
    emit("pad_rows K=" + std::to_string(K) + "->" + std::to_string(Kp) + " <- " + who, {src}, {dst}, [=](void* st) {
        VX(vx_memset(dp(), 0, (size_t)M * Kp * 2, st));
        const int64_t ne[4] = {K, M, 1, 1}, ss[4] = {1, K, 0, 0}, ds[4] = {1, Kp, 0, 0};
        VX(vx_copy_strided_f16(sp(), dp(), ne, ss, ds, 1.0f, st));
    });
    return dst;
}

// interpolate (bilinear, align_corners) -> conv 3x3 32 -> 32 + bias -> relu -> conv 1x1 -> 1 -> relu [-> scale], every link read by the
// next one only: the DPT head's tail (depth-anything.cpp:84-95) is ONE launch of the kernel made for it (kernels_headconv.hip)
bool lowering::head_tail(int t) {
    graph_node const& up = g.nodes[t];
    graph_node const& x = g.nodes[up.src[0]];
    const int cin = (int)x.ne[0];
    if ((up.ip[2] & 255) != 1 || !(up.ip[2] & 256) || (cin != 32 && cin != 64 && cin != 128)) return false;
    const int c2 = sole_consumer(t);
    if (c2 < 0 || g.nodes[c2].op != gop_conv_2d || g.nodes[c2].src[0] != t || g.nodes[c2].n_src != 3) return false;
    graph_node const& w2 = g.nodes[g.nodes[c2].src[1]];
    if (w2.ne[0] != cin || w2.ne[1] != 3 || w2.ne[2] != 3 || w2.ne[3] != 32 || g.nodes[c2].ip[0] != 1 || g.nodes[c2].ip[1] != 1) return false;
    const int r1 = sole_consumer(c2);
    if (r1 < 0 || g.nodes[r1].op != gop_relu) return false;
    const int c3 = sole_consumer(r1);
    if (c3 < 0 || g.nodes[c3].op != gop_conv_2d || g.nodes[c3].dtype != gdt_f32 || g.nodes[c3].src[0] != r1) return false;
    const int r2 = sole_consumer(c3);
    if (r2 < 0 || g.nodes[r2].op != gop_relu) return false; // the kernel's last ReLU is not optional
    const int H = (int)up.ne[2], W = (int)up.ne[1], hs = (int)x.ne[2], ws = (int)x.ne[1], B = (int)x.ne[3];
    if (cin == 32 ? !vx_headconv_supported(32, 32, H, W, hs, ws) || (size_t)B * hs * ws * 64 >= ((size_t)1 << 31)
                  : !vx_headconv_wide_supported(cin, 32, H, W, hs, ws) || (size_t)B * hs * ws * cin >= ((size_t)1 << 32))
        return false;
    std::vector<int> tail = {r2}; // what c3's launch computes behind c3
    float scale = 1.0f;
    const int sc = sole_consumer(r2);
    if (sc >= 0 && g.nodes[sc].op == gop_scale) { scale = g.nodes[sc].fp[0]; tail.push_back(sc); }
    const int wt = g.nodes[c2].src[1];
    void* frag = pack_head_fragments(wt, cin);
    const float* bias2 = const_f32(g.nodes[c2].src[2]);
    const float* w3 = const_f32(g.nodes[c3].src[1]);
    const float b3 = g.nodes[c3].n_src == 3 ? g.nodes[g.nodes[c3].src[2]].values()[0] : 0.0f;
    if (g.nodes[c3].n_src == 3) (void)const_f32(g.nodes[c3].src[2]); // (a kernel argument by value; its image makes the scalar part of the model's arena)
    const int xbuf = buf_of(up.src[0]);
    for (int f : {t, c2, r1, c3}) skip[f] = 1;
    absorb(tail, c3);
    materialise(c3);
    const int obuf = g.nodes[c3].buffer;
    auto xp = ptr(xbuf), op = ptr(obuf);
    char d[160];
    snprintf(d, sizeof d, "head_tail[resize %dx%d -> %dx%d, conv3x3 %d->32, relu, conv1x1 -> 1, relu%s] B=%d <- %s", ws, hs, W, H, cin, scale != 1.0f ? ", scale" : "", B,
             g.nodes[wt].name.c_str());
    if (cin == 32)
        emit(d, {xbuf}, {obuf}, [=](void* st) { VX(vx_headconv_bil_f16(xp(), frag, bias2, w3, b3, scale, reinterpret_cast<float*>(op()), B, H, W, hs, ws, st)); });
    else
        emit(d, {xbuf}, {obuf}, [=](void* st) { VX(vx_headconv_wide_bil_f16(xp(), cin, frag, bias2, w3, b3, scale, reinterpret_cast<float*>(op()), B, H, W, hs, ws, st)); });
    tag("head_conv2+3", 2.0 * B * H * W * 32.0 * (9.0 * cin + 1), (double)B * ((double)hs * ws * cin * 2 + (double)H * W * 4));
    return true;
}

// conv 1x1 -> one channel [-> relu] [-> scale]: one f32 launch
void lowering::one_channel_head(int t) {
    graph_node& n = g.nodes[t];
    graph_node const& x = g.nodes[n.src[0]];
    const int C = (int)x.ne[0];
    if (C % 8) throw except("conv_2d to one channel: Cin = %d must be a multiple of 8", C);
    std::vector<int> tail; // [relu] [scale] behind the conv
    float scale = 1.0f;
    int relu = 0, c = sole_consumer(t);
    if (c >= 0 && g.nodes[c].op == gop_relu) { relu = 1; tail.push_back(c); c = sole_consumer(c); }
    if (c >= 0 && g.nodes[c].op == gop_scale) { scale = g.nodes[c].fp[0]; tail.push_back(c); }
    absorb(tail, t); // (an output anywhere in the fused chain keeps the buffer)
    const float* w = const_f32(n.src[1]);
    const float bias = n.n_src == 3 ? g.nodes[n.src[2]].values()[0] : 0.0f;
    if (n.n_src == 3) (void)const_f32(n.src[2]);
    const int xbuf = buf_of(n.src[0]);
    materialise(t);
    const int obuf = n.buffer;
    auto xp = ptr(xbuf), op = ptr(obuf);
    const int64_t M = n.n_elements();
    std::string who = n.name.empty() ? g.nodes[n.src[1]].name : n.name; // (not weight_name: the node's own name comes first here)
    emit(std::string("conv1x1_to_1") + (relu ? "[relu]" : "") + (scale != 1.0f ? "[scale]" : "") + " M=" + std::to_string(M) + " C=" + std::to_string(C) + " <- " + who, {xbuf}, {obuf},
         [=](void* st) { VX(vx_conv1x1_to1_f32(xp(), w, bias, relu, scale, reinterpret_cast<float*>(op()), M, C, st)); });
    tag("head_out", 2.0 * M * C, (double)M * (C * 2 + 4));
}

// timing group of a matrix product from the weight's name (the groups the model entries and bench.py report)
static std::string group_of(std::string const& who, graph_node const& n, int stride) {
    auto has = [&](const char* k) { return who.find(k) != std::string::npos; };
    if (has("reassemble") && has("projection")) return "neck_proj";
    if (has("reassemble") && has("resize")) return n.op == gop_conv_transpose_2d ? "neck_convT" : (stride > 1 ? "neck_conv_s2" : "neck_resize");
    if (has("neck.convs")) return "neck_convs";
    if (has("residual_layer")) return "fusion_rcu";
    if (has("fusion_stage") && has("projection")) return "fusion_proj";
    if (has("head.conv1")) return "head_conv1";
    if (has("head.conv")) return "head_conv2+3";
    return n.op == gop_linear ? "gemm" : "conv";
}

int lowering::plain_gemm_reader(int t) const { // the sole reader of t (through single-reader views) if it reads t's rows as a plain GEMM A operand
    int c = sole_consumer(t);
    while (c >= 0 && (g.nodes[c].op == gop_reshape || g.nodes[c].op == gop_cont)) c = sole_consumer(c);
    if (c < 0 || root_view(g.nodes[c].src[0]) != t) return -1;
    graph_node const& n = g.nodes[c];
    if (n.op == gop_linear || n.op == gop_conv_transpose_2d) return c;
    if (n.op == gop_conv_2d && n.dtype == gdt_f16) {
        graph_node const& w = g.nodes[n.src[1]];
        if (w.ne[1] == 1 && w.ne[2] == 1 && n.ip[0] == 1 && n.ip[1] == 0) return c;
    }
    return -1;
}
bool lowering::dconv_shape(graph_node const& n, graph_node const& x, graph_node const& w) const {
    return g.fused_models && !env().no_dconv && n.op == gop_conv_2d && n.dtype == gdt_f16 && w.ne[1] == 3 && w.ne[2] == 3 && n.ip[0] == 1 && n.ip[1] == 1 && x.ne[0] % 16 == 0 && x.ne[0] >= 32 &&
           (w.ne[3] == 32 || w.ne[3] == 64) && n.ne[1] >= env().dconv_min_w;
}

void lowering::planar_to_nhwc(int r) {
    graph_node& n = g.nodes[r];
    const planar_map pm = planar.at(r);
    materialise(r);
    const int obuf = n.buffer;
    auto sp = ptr(pm.buf), op = ptr(obuf);
    const int64_t npix = pm.plane_elems / 32, C = n.ne[0], off = (int64_t)pm.plane0 * pm.plane_elems;
    std::array<int64_t, 4> A{32, npix, pm.n_planes, 1}, S{1, 32, pm.plane_elems, 0}, D{1, C, 32, 0};
    emit("planes_to_nhwc " + shape_str(n.ne), {pm.buf}, {obuf}, [=](void* st) { VX(vx_copy_strided_f16(sp() + off * 2, op(), A.data(), S.data(), D.data(), 1.0f, st)); });
}
// interpolate(NEAREST) to exactly twice the extent of a planar map, read by one 3x3 conv: the conv's loader does it (esrgan.cpp:13-19)
bool lowering::nearest_into_reader(int t) {
    graph_node const& n = g.nodes[t];
    const int xs = root(n.src[0]);
    graph_node const& x = g.nodes[xs];
    if (!g.fused_models || (n.ip[2] & 255) != 0 || n.is_output || !planar.count(xs) || n.ne[1] != 2 * x.ne[1] || n.ne[2] != 2 * x.ne[2]) return false;
    const int c = sole_consumer(t);
    if (c < 0 || g.nodes[c].src[0] != t || !is_conv3x3(g.nodes[c], g.nodes[g.nodes[c].src[1]])) return false;
    up2_of[t] = xs;
    return true;
}
// esrgan.cpp's epilogues behind a planar conv t: LeakyReLU 0.2 or ReLU, then up to two [* scale] + residual steps on planar maps of t's shape
// (res / res2 are ROOT nodes); the RGB conv has none
lowering::epilogue lowering::match_planar_epilogue(int t) const {
    graph_node const& n = g.nodes[t];
    epilogue e;
    e.last = t;
    int c = n.dtype == gdt_f32 ? -1 : sole_consumer(t);
    if (c >= 0 && (g.nodes[c].op == gop_relu || (g.nodes[c].op == gop_leaky_relu && g.nodes[c].fp[0] == 0.2f))) {
        e.act = g.nodes[c].op == gop_relu ? 2 : 1;
        e.absorbed.push_back(c);
        e.last = c;
        c = sole_consumer(c);
    }
    for (int round = 0; round < 2 && c >= 0; ++round) {
        float sc = 1.0f;
        int sn = -1, a = c;
        if (g.nodes[c].op == gop_scale) { sn = c; sc = g.nodes[c].fp[0]; a = sole_consumer(c); }
        if (a < 0 || g.nodes[a].op != gop_add) break;
        graph_node const& an = g.nodes[a];
        const int prev = sn >= 0 ? sn : e.last;
        const int other = an.src[0] == prev ? an.src[1] : (an.src[1] == prev ? an.src[0] : -1);
        if (other < 0 || !planar.count(root(other)) || g.nodes[other].n_elements() != n.n_elements() || g.nodes[other].ne[0] != n.ne[0]) break;
        (round == 0 ? e.s1 : e.s2) = sc;
        (round == 0 ? e.res : e.res2) = root(other);
        if (sn >= 0) e.absorbed.push_back(sn);
        e.absorbed.push_back(a);
        e.last = a;
        c = sole_consumer(a);
    }
    return e;
}
// A 3x3 / stride 1 / pad 1 conv on a planar map (or on the f32 image, or on the x2 nearest resize of a planar map) through the LDS-ring conv in
// its native layout, with esrgan.cpp's epilogues: LeakyReLU 0.2 or ReLU, then up to two [* scale] + residual steps (conv5 * 0.2 + x, and
// (.) * 0.2 + the rrdb's input, esrgan.cpp:38-40, 49-50), the skip x taken from the halo when it is the conv's own first 64 input channels;
// the RGB conv writes the f32 image. Returns false (nothing changed) when the conv is not of this kind.
bool lowering::planar_conv(int t, std::string const& who) {
    graph_node& n = g.nodes[t];
    if (!g.fused_models || !is_conv3x3(n, g.nodes[n.src[1]]) || (n.n_src == 3 && !g.nodes[n.src[2]].constant)) return false;
    if (relu_on_load[t]) return false; // relu -> conv: the NHWC form applies it in its loader
    const int xs = n.src[0], xr = root(xs);
    graph_node const& x = g.nodes[xr];
    const int cin = (int)g.nodes[xs].ne[0], cout = (int)n.ne[0], H = (int)n.ne[2], W = (int)n.ne[1], B = (int)n.ne[3];
    const bool rgb = cout == 3 && n.dtype == gdt_f32;
    if (!rgb && !((cout == 32 || cout == 64) && n.dtype == gdt_f16)) return false;
    const int64_t npix = (int64_t)B * H * W;
    // the input: planes as they are or resized x2 by the loader, or the f32 image (as a value | residue plane)
    const auto up = up2_of.find(xs);
    const int up2 = up != up2_of.end(), xp_node = up2 ? up->second : (planar.count(xr) ? xr : -1);
    const int dup = xp_node < 0 && x.op == gop_input && x.dtype == gdt_f32 && cin <= 16 ? cin : 0;
    if (xp_node >= 0 ? cin % 32 != 0 : !dup) return false;
    const epilogue e = match_planar_epilogue(t);
    const int act = e.act, last = e.last, res[2] = {e.res, e.res2};
    const float s1 = e.s1, s2 = e.s2;

    absorb(e, t);
    planar_map in;
    if (dup) {
        auto it = image_plane.find(xr);
        if (it == image_plane.end()) {
            const int ibuf = buf_of(xr), pbuf = new_buffer((size_t)npix * 32 * 2);
            auto ip = ptr(ibuf), pp = ptr(pbuf);
            emit("image_planes " + shape_str(x.ne), {ibuf}, {pbuf}, [=](void* st) { VX(vx_image_planes_f32(reinterpret_cast<const float*>(ip()), pp(), npix, cin, st)); });
            tag("image_in", 0, (double)npix * (cin * 4 + 64));
            it = image_plane.emplace(xr, pbuf).first;
        }
        in = {it->second, 0, 1, npix * 32};
    } else in = planar.at(xp_node);

    vx_dconv_args d;
    memset(&d, 0, sizeof d);
    int d_cin = 0;
    d.w = (dup || rgb) ? pack_dconv_ex(n.src[1], cin, dup, cout, rgb ? 32 : cout, &d_cin) : pack_dconv(n.src[1], cin, cout, &d_cin);
    d.bias = n.n_src == 3 ? (rgb ? bias_padded(n.src[2], 32) : const_f32(n.src[2])) : nullptr;
    d.cin = d_cin; d.cout = rgb ? 32 : cout;
    d.up2 = up2;
    d.B = B; d.H = H; d.W = W;
    d.epi = rgb ? VX_DC_RGB_F32 : VX_DC_F16;
    d.act = act;
    d.s1 = s1; d.s2 = s2;
    d.x_plane = in.plane_elems;
    const int64_t x_off = (int64_t)in.plane0 * in.plane_elems;
    std::vector<int> reads = {in.buf};
    std::function<char*()> rp[2];
    int64_t r_off[2] = {0, 0};
    for (int i = 0; i < 2; ++i) {
        if (res[i] < 0) continue;
        planar_map const& rm = planar.at(res[i]);
        if (i == 0 && !up2 && cout == 64 && rm.buf == in.buf && rm.plane0 == in.plane0 && in.n_planes >= 2 && vx_dconv_x_residual_supported(s1, act, 0)) { d.x_residual = 1; continue; } // x = the halo's first two planes (else: an ordinary res1)
        reads.push_back(rm.buf);
        rp[i] = ptr(rm.buf);
        r_off[i] = (int64_t)rm.plane0 * rm.plane_elems;
        (i == 0 ? d.res1_plane : d.res2_plane) = rm.plane_elems;
    }

    // ---- where the result goes
    int obuf;
    int64_t o_off = 0;
    if (rgb) {
        materialise(t);
        obuf = n.buffer;
    } else {
        planar_map om{-1, 0, cout / 32, npix * 32};
        if (auto it = placed.find(last); it != placed.end()) { om.buf = it->second.first; om.plane0 = it->second.second; placed.erase(it); }
        else {
            // the head of a concat chain along the channels: reserve the whole dense block and the slots of the maps that will join it
            std::vector<std::pair<int, int>> joins; // (concat node, second operand)
            int cur = last, width = cout;
            for (;;) {
                int cc = -1;
                for (int c : consumers[cur])
                    if (g.nodes[c].op == gop_concat && g.nodes[c].ip[0] == 0 && g.nodes[c].src[0] == cur && !g.nodes[c].is_output) { cc = c; break; }
                if (cc < 0) break;
                const int s2n = g.nodes[cc].src[1];
                graph_node const& sn = g.nodes[s2n];
                // the joining map must be one this function will write: a 3x3 conv of the chain so far to 32 or 64 channels (constant bias), alone or behind
                // an activation its epilogue absorbs
                auto joins_by_conv = [&](int cn) {
                    graph_node const& c = g.nodes[cn];
                    return !c.constant && c.op == gop_conv_2d && c.dtype == gdt_f16 && is_conv3x3(c, g.nodes[c.src[1]]) && (c.n_src == 2 || g.nodes[c.src[2]].constant) &&
                           (c.ne[0] == 32 || c.ne[0] == 64) && c.src[0] == cur;
                };
                const bool act_of_conv = (sn.op == gop_relu || (sn.op == gop_leaky_relu && sn.fp[0] == 0.2f)) && !sn.constant && joins_by_conv(sn.src[0]) && uses[sn.src[0]] == 1 &&
                                         !g.nodes[sn.src[0]].is_output;
                const bool conv_itself = joins_by_conv(s2n);
                if (!(act_of_conv || conv_itself) || uses[s2n] != 1 || sn.is_output || s2n < cur) break;
                joins.emplace_back(cc, s2n);
                width += (int)sn.ne[0];
                cur = cc;
            }
            om.buf = new_buffer((size_t)npix * width * 2, n.is_output);
            int at = cout / 32;
            for (auto const& j : joins) {
                placed[j.second] = {om.buf, at};
                at += (int)g.nodes[j.second].ne[0] / 32;
                planar[j.first] = {om.buf, 0, at, npix * 32};
                skip[j.first] = 1;
            }
        }
        planar[t] = om;
        obuf = om.buf;
        o_off = (int64_t)om.plane0 * om.plane_elems;
        d.out_plane = om.plane_elems;
    }
    char desc[320];
    snprintf(desc, sizeof desc, "dconv3x3(planes)%s%s%s%s%s%s M=%lld N=%d K=%d <- %s", dup ? "[f32 image]" : "", up2 ? "[nearest x2 in the loader]" : "",
             act == 1 ? "[leaky_relu]" : (act == 2 ? "[relu]" : ""), res[0] >= 0 ? (d.x_residual ? "[*s + x]" : "[*s + res]") : "", res[1] >= 0 ? "[*s + res]" : "", rgb ? "[rgb f32]" : "",
             (long long)npix, cout, 9 * cin, who.c_str());
    auto xp = ptr(in.buf), op = ptr(obuf);
    emit(desc, reads, {obuf}, [=](void* st) {
        vx_dconv_args r = d;
        r.x = xp() + x_off * 2;
        r.out = op() + o_off * 2;
        if (rp[0]) r.res1 = rp[0]() + r_off[0] * 2;
        if (rp[1]) r.res2 = rp[1]() + r_off[1] * 2;
        VX(vx_dconv3x3_f16(&r, st));
    });
    std::string grp = rgb ? "last" : (dup ? "first" : (up2 ? "upconv" : "conv"));
    if (auto k = who.find(".RDB"); k != std::string::npos && who.find(".conv", k) != std::string::npos) grp = "rdb_conv" + who.substr(who.find(".conv", k) + 5, 1);
    else if (!rgb && !dup && !up2 && who.find(".sub.") != std::string::npos) grp = "trunk";
    else if (!rgb && !dup && !up2 && act == 1) grp = "hrconv";
    tag(grp.c_str(), 2.0 * npix * (double)cout * 9 * cin, (double)npix * ((up2 ? 0.25 : 1.0) * d_cin * 2 + (rgb ? 12 : cout * 2)));
    if (!rgb && n.is_output) planar_to_nhwc(t); // a graph output is read back as NHWC
    return true;
}

// dpt::residual_conv on a small map (depth-anything.cpp:15-23): relu -> conv3x3 -> relu -> conv3x3 -> + x, every link read by the next one only,
// [+ feature_fusion's other addend (:28-31)] [-> the 1x1 out_conv that commutes with the resize behind the unit (:36-40)]: ONE launch of
// kernels_rcu.hip with the intermediate map in LDS. t = the first conv (its ReLU is on its loader already). Returns false (nothing changed)
// when the pattern or the kernel's limits do not hold.
bool lowering::residual_unit(int t, std::string const& who) {
    graph_node& n = g.nodes[t];
    const int xs = n.src[0];
    graph_node const& x = g.nodes[xs];
    const int H = (int)n.ne[2], W = (int)n.ne[1], B = (int)n.ne[3];
    auto conv64 = [&](graph_node const& c) {
        graph_node const& w = g.nodes[c.src[1]];
        return c.op == gop_conv_2d && c.dtype == gdt_f16 && w.constant && w.ne[0] == 64 && w.ne[1] == 3 && w.ne[2] == 3 && w.ne[3] == 64 && c.ip[0] == 1 && c.ip[1] == 1 &&
               (c.n_src == 2 || g.nodes[c.src[2]].constant);
    };
    if (env().no_rcu_fuse || !g.fused_models || !relu_on_load[t] || !conv64(n) || x.ne[0] != 64 || n.is_output || resized_in.count(xs) || !vx_rcu_supported(H, W)) return false;
    const int r1 = sole_consumer(t);
    if (r1 < 0 || g.nodes[r1].op != gop_relu) return false;
    const int c2 = sole_consumer(r1);
    if (c2 < 0 || !conv64(g.nodes[c2]) || g.nodes[c2].src[0] != r1) return false;
    // + x behind the second conv: the first addend must be the unit's own input, as a map the epilogue can take (not one that lives as planes only)
    const epilogue e = match_epilogue(c2, false, false, true);
    if (e.act != 0 || e.res < 0 || root(e.res) != root(xs)) return false;
    // the projection behind the unit's resize
    int up = g.nodes[e.last].is_output ? -1 : sole_consumer(e.last), pj = -1;
    if (up >= 0) {
        graph_node const& u = g.nodes[up];
        const bool bil = u.op == gop_interpolate && (u.ip[2] & 255) == 1 && (u.ip[2] & 256) && !u.is_output && u.src[0] == e.last;
        pj = bil ? sole_consumer(up) : -1;
        if (pj >= 0) {
            graph_node const& c = g.nodes[pj];
            graph_node const& w = g.nodes[c.src[1]];
            if (!(c.op == gop_conv_2d && c.dtype == gdt_f16 && c.src[0] == up && w.constant && w.ne[0] == 64 && w.ne[1] == 1 && w.ne[2] == 1 && w.ne[3] == 64 && c.ip[0] == 1 && c.ip[1] == 0 &&
                  (c.n_src == 2 || g.nodes[c.src[2]].constant)))
                pj = -1;
        }
    }

    skip[r1] = skip[c2] = 1; // both convs and the ReLU between them are this launch
    g.nodes[r1].alias_of = t;
    absorb(e, c2);
    vx_rcu_args a;
    memset(&a, 0, sizeof a);
    a.w1 = pack_rcu(n.src[1], 9);
    a.b1 = n.n_src == 3 ? const_f32(n.src[2]) : nullptr;
    a.w2 = pack_rcu(g.nodes[c2].src[1], 9);
    a.b2 = g.nodes[c2].n_src == 3 ? const_f32(g.nodes[c2].src[2]) : nullptr;
    a.B = B; a.H = H; a.W = W;
    const int xbuf = buf_of(xs);
    std::vector<int> reads = {xbuf};
    std::function<char*()> rp2;
    if (e.res2 >= 0) { reads.push_back(buf_of(e.res2)); rp2 = ptr(buf_of(e.res2)); }
    int obuf;
    if (pj >= 0) {
        a.wp = pack_rcu(g.nodes[pj].src[1], 1);
        a.bp = g.nodes[pj].n_src == 3 ? const_f32(g.nodes[pj].src[2]) : nullptr;
        obuf = new_buffer((size_t)B * H * W * 64 * 2);
        preprojected[up] = obuf;
    } else {
        materialise(c2);
        obuf = g.nodes[c2].buffer;
    }
    char d[320];
    snprintf(d, sizeof d, "residual_unit[relu, conv3x3, relu, conv3x3, + x%s%s] %dx%d B=%d <- %s", e.res2 >= 0 ? ", + x0" : "", pj >= 0 ? ", conv1x1 before its resize" : "", W, H, B,
             who.c_str());
    auto xp = ptr(xbuf), op = ptr(obuf);
    emit(d, reads, {obuf}, [=](void* st) {
        vx_rcu_args r = a;
        r.x = xp();
        r.out = op();
        if (rp2) r.res2 = rp2();
        VX(vx_rcu_fused_f16(&r, st));
    });
    const double px = (double)B * H * W;
    tag("fusion_rcu", 2.0 * px * 64 * (576 * 2 + (pj >= 0 ? 64 : 0)), px * 64 * 2 * (2 + (e.res2 >= 0 ? 1 : 0)));
    return true;
}

void lowering::gemm_like(int t) {
    graph_node& n = g.nodes[t];
    if (yolo_takes(t)) return yolo_product(t); // a SiLU group, a conv that reads or writes inside a wider map: never the LDS-ring kernels (lower_yolo.cpp)
    if (n.op == gop_conv_2d && planar_conv(t, weight_name(g, n))) return;
    if (n.op == gop_conv_2d && n.dtype == gdt_f32 && n.ne[0] != 1) throw except("conv_2d %s to an f32 image of %lld channels is lowered onto the LDS-ring conv only (3x3 / stride 1 / pad 1 behind planar maps)", n.name.c_str(), (long long)n.ne[0]);
    if (n.op == gop_conv_2d && n.dtype == gdt_f32) return one_channel_head(t);
    const int xs = n.src[0], wt = n.src[1], bt = n.n_src == 3 ? n.src[2] : -1;
    graph_node const& x = g.nodes[xs];
    // groups are keyed on the weight's name. (Not weight_name: a conv without a name on a kernel that is no named weight takes the kernel node's name)
    std::string who = n.name.empty() ? g.nodes[wt].name : n.name;
    if (g.nodes[wt].op == gop_weight && !g.nodes[wt].name.empty()) who = g.nodes[wt].name;
    product P;
    vx_gemm_args& a = P.a;
    std::string kind;
    epilogue e;
    e.last = t;
    int stride = 1;
    // the A rows of a plain product: in place from a sliced source, from a padded producer, or padded by a copy
    auto plain_rows = [&] {
        const int v = root_view(xs), K = P.p.k_real, Kp = P.p.K;
        if (auto it = sliced_in.find(v); it != sliced_in.end()) {
            a.a_group = (int)it->second.rows; a.a_group_stride = (int)it->second.stride; a.a_row_off = (int)it->second.begin;
            a.lda = K;
            kind += "[rows " + std::to_string(it->second.begin) + ".. of " + std::to_string(it->second.stride) + "]";
            return buf_of(it->second.src);
        }
        if (auto it = row_stride.find(v); it != row_stride.end() && it->second == Kp) { a.lda = Kp; return buf_of(xs); }
        a.lda = Kp;
        return padded_rows(xs, K, Kp, a.M, who);
    };
    if (n.op == gop_linear) {
        e = match_epilogue(t, true, true);
        pack_conv_rows(P, n, false, -1, e.scale);
        a.M = (int)(x.n_elements() / x.ne[0]);
        kind = "gemm";
        P.in.buf = plain_rows();
    } else if (n.op == gop_conv_2d) {
        graph_node const& w = g.nodes[wt];
        const int kw = (int)w.ne[1], kh = (int)w.ne[2], pad = (int)n.ip[1];
        stride = (int)n.ip[0];
        a.M = (int)(n.ne[1] * n.ne[2] * n.ne[3]);
        // a 3-channel f32 image (patch_embed of mobile-sam.cpp:71-76) or MI-GAN's mask | rgb (migan.cpp:84-86): read as 8-channel pixels by the conv loader
        const bool image8_in = image8_input(x);
        if (!image8_in && kw == 1 && kh == 1 && stride == 1 && pad == 0) { // 1x1: a plain product on the pixel rows (nn.cpp:76-81)
            pack_conv_rows(P, n, false);
            kind = "gemm(conv1x1)";
            P.in.buf = plain_rows();
        } else {
            if (!image8_in && x.ne[0] % 8) throw except("conv_2d %s: Cin = %lld must be a multiple of 8", who.c_str(), (long long)x.ne[0]);
            if (!image8_in && dconv_shape(n, x, w)) return dconv(t, who);
            pack_conv_rows(P, n, image8_in);
            P.in.buf = image8_in ? image_pad8(xs) : buf_of(xs);
            conv_geometry(a, n, x, w);
            a.a_relu = relu_on_load[t];
            P.halo = kh == 3 && kw == 3 && stride == 1 && pad == 1 && a.conv_W >= env().halo_min_w;
            kind = "conv" + std::to_string(kw) + "x" + std::to_string(kh) + (stride > 1 ? "s" + std::to_string(stride) : "") + (a.a_relu ? "[relu-in]" : "");
        }
    } else { // conv_transpose_2d with kernel == stride: a product + pixel shuffle
        const int s = (int)n.ip[0];
        P.operand(pack_conv_transpose(wt, bt, s));
        a.M = (int)(x.ne[1] * x.ne[2] * x.ne[3]);
        kind = "gemm+pixel_shuffle(s" + std::to_string(s) + ")";
        P.in.buf = plain_rows();
        a.ps_s = s; a.ps_Cout = (int)n.ne[0]; a.ps_H = (int)x.ne[2]; a.ps_W = (int)x.ne[1];
    }
    packed_operand const& p = P.p;
    // a channel count that is no multiple of 8 (the 2 k^2 offsets and k^2 modulator logits of a deformable conv on their own): the f16 epilogues store
    // 8 at a time, so the product writes rows padded to 8 and one strided copy compacts them
    const bool ragged = n.ne[0] % 8 != 0;
    if (ragged && n.op == gop_conv_transpose_2d) throw except("%s %s: %lld output channels; the f16 epilogues store 8 at a time", graph_op_name(n.op), who.c_str(), (long long)n.ne[0]);
    a.n_valid = n.op == gop_conv_transpose_2d ? p.n_real : (int)n.ne[0];
    a.ldo = n.ne[0];
    if (n.op == gop_conv_transpose_2d) a.epi = VX_EPI_PIXSHUF;
    else {
        if (n.op != gop_linear) e = match_epilogue(t, true, false, true);
        if (ragged && e.res >= 0) throw except("%s %s: %lld output channels with a residual; rows that are no multiple of 8 channels take no residual epilogue", graph_op_name(n.op), who.c_str(), (long long)n.ne[0]);
        absorb(e, t); // (no way back to another lowering from here)
        a.epi = e.res >= 0 ? VX_EPI_F16_ADD : (e.act == 1 ? VX_EPI_F16_GELU : (e.act == 2 ? VX_EPI_F16_RELU : VX_EPI_F16));
        a.relu = e.res >= 0 && e.act == 2;
    }
    // rows of a width that is no multiple of the GEMM's 64-wide k tile, read by one plain product only: written with the padded row
    // stride that reader wants (the pad columns are exact zeros: zero weights, zero bias), no pad_rows copy in between
    size_t out_bytes = n.n_bytes();
    if (g.fused_models && !ragged && a.epi == VX_EPI_F16 && n.op != gop_conv_transpose_2d && n.ne[0] % 64 != 0 && !n.is_output && p.N >= round_up((int)n.ne[0], 64) && plain_gemm_reader(t) >= 0) {
        const int Kp = round_up((int)n.ne[0], 64);
        row_stride[t] = Kp;
        a.ldo = Kp;
        a.n_valid = Kp;
        out_bytes = (size_t)(n.n_elements() / n.ne[0]) * Kp * 2;
    }
    n.buffer = new_buffer(out_bytes, n.is_output || n.op == gop_input);
    const int ld8 = round_up((int)n.ne[0], 8);
    const int64_t rows = n.n_elements() / n.ne[0];
    if (ragged) { a.ldo = ld8; a.n_valid = ld8; }
    P.out.buf = ragged ? new_buffer((size_t)rows * ld8 * 2) : n.buffer;
    if (e.res >= 0) P.res1.buf = buf_of(e.res);
    if (e.res2 >= 0) P.res2 = buf_of(e.res2);
    char d[320];
    snprintf(d, sizeof d, "%s%s%s%s%s%s%s M=%d N=%d K=%d <- %s", kind.c_str(), e.scale >= 0 ? "[*scale]" : "", e.act ? "[" : "", act_name(e.act), e.act ? "]" : "",
             e.res >= 0 ? "[+res]" : "", e.res2 >= 0 ? "[+res]" : "", a.M, (int)n.ne[0], p.k_real, who.c_str());
    P.desc = d;
    P.group = group_of(who, n, stride);
    P.work(p.k_real, (double)n.ne[0]); // (the residuals' rows are not counted here)
    emit_product(P);
    if (ragged) {
        const int obuf = P.out.buf, dst = n.buffer;
        auto sp = ptr(obuf), dp = ptr(dst);
        const int64_t c = n.ne[0];
        emit("unpad_rows N=" + std::to_string(ld8) + "->" + std::to_string(c) + " <- " + who, {obuf}, {dst}, [=](void* st) {
            const int64_t ne[4] = {c, rows, 1, 1}, ss[4] = {1, ld8, 0, 0}, ds[4] = {1, c, 0, 0};
            VX(vx_copy_strided_f16(sp(), dp(), ne, ss, ds, 1.0f, st));
        });
        tag("glue", 0, (double)rows * c * 4);
    }
}

// 3x3 / stride 1 / pad 1 with Cin % 16 == 0, Cin >= 32 (the kernel's pixel stride; a narrower map goes to the GEMM family's conv) and 32 or 64 output channels: the persistent LDS-ring conv (kernels_dconv.hip), with the
// ReLU of a relu -> conv chain applied to the fragments, ReLU or up to two residual maps in the epilogue, and -- where the input is the
// bilinear (align_corners) resize of a smaller map read by this conv only -- the resize done by the conv's halo loader
void lowering::dconv(int t, std::string const& who) {
    if (residual_unit(t, who)) return;
    graph_node& n = g.nodes[t];
    const int xs = n.src[0], wt = n.src[1], bt = n.n_src == 3 ? n.src[2] : -1;
    graph_node const& x = g.nodes[xs];
    const int cin = (int)x.ne[0], cout = (int)n.ne[0], H = (int)n.ne[2], W = (int)n.ne[1], B = (int)n.ne[3];
    const epilogue e = match_epilogue(t, false, false, true, false); // the LDS-ring conv applies the activation, then the residuals (tests/test_gpu_dconv_matrix.py), so it could take an add behind a relu; this lowering does not ask for one yet: it stays a launch
    absorb(e, t);
    vx_dconv_args d;
    memset(&d, 0, sizeof d);
    int d_cin = 0;
    d.w = pack_dconv(wt, cin, cout, &d_cin);
    d.bias = bt >= 0 ? const_f32(bt) : nullptr;
    d.cin = d_cin; d.cout = cout;
    d.x_pix = cin; d.x_plane = 32;
    d.B = B; d.H = H; d.W = W;
    d.epi = VX_DC_F16;
    d.act = e.act == 2 ? 2 : 0;
    d.a_relu = relu_on_load[t];
    d.s1 = d.s2 = 1.0f;
    d.res1_pix = d.res2_pix = d.out_pix = cout;
    d.res1_plane = d.res2_plane = d.out_plane = 32;
    int xbuf;
    std::string kind = "dconv3x3";
    if (auto it = resized_in.find(xs); it != resized_in.end()) {
        xbuf = it->second.buf;
        d.bil_hs = it->second.hs; d.bil_ws = it->second.ws;
        kind += "[resize " + std::to_string(it->second.ws) + "x" + std::to_string(it->second.hs) + " in the loader]";
    } else xbuf = buf_of(xs);
    if (d.a_relu) kind += "[relu-in]";
    materialise(t);
    const int obuf = n.buffer;
    std::vector<int> reads = {xbuf};
    const residual_ptrs rp = read_residuals(e, reads);
    char desc[320];
    snprintf(desc, sizeof desc, "%s%s%s%s M=%d N=%d K=%d <- %s", kind.c_str(), e.act == 2 ? "[relu]" : "", e.res >= 0 ? "[+res]" : "", e.res2 >= 0 ? "[+res]" : "", B * H * W, cout,
             9 * cin, who.c_str());
    auto xp = ptr(xbuf), op = ptr(obuf);
    emit(desc, reads, {obuf}, [=](void* st) {
        vx_dconv_args r = d;
        r.x = xp();
        r.out = op();
        if (rp.res1) r.res1 = rp.res1();
        if (rp.res2) r.res2 = rp.res2();
        VX(vx_dconv3x3_f16(&r, st));
    });
    tag(group_of(who, n, 1).c_str(), 2.0 * B * H * W * (double)cout * 9 * cin, (double)B * H * W * (cin + cout) * 2);
}

// interpolate (bilinear, align_corners) read by ONE consumer:
//   * conv 1x1 (+ bias): the two commute (the bilinear weights of a pixel sum to one), so the projection runs on the small map -- a
//     quarter of the products and no full-resolution intermediate (depth-anything.cpp:36-40) -- and the resize follows;
//   * conv 3x3 with 32 output channels that the LDS-ring kernel can feed from the small map: no resize launch at all.
// Returns true when the node needs no launch of its own.
bool lowering::resize_into_reader(int t) {
    if (!g.fused_models) return false;
    graph_node const& up = g.nodes[t];
    if ((up.ip[2] & 255) != 1 || !(up.ip[2] & 256) || up.is_output) return false;
    const int c = sole_consumer(t);
    if (c < 0 || g.nodes[c].op != gop_conv_2d || g.nodes[c].src[0] != t || g.nodes[c].dtype != gdt_f16) return false;
    graph_node const& x = g.nodes[up.src[0]];
    graph_node& cn = g.nodes[c];
    graph_node const& w = g.nodes[cn.src[1]];
    const int hs = (int)x.ne[2], ws = (int)x.ne[1], H = (int)up.ne[2], W = (int)up.ne[1], B = (int)x.ne[3];
    auto loader_can = [&](graph_node const& conv, graph_node const& cw, int cin) {
        return !env().no_bil_fuse && dconv_shape(conv, g.nodes[conv.src[0]], cw) && cw.ne[3] == 32 && cin % 32 == 0 && !relu_on_load[&conv - g.nodes.data()] &&
               vx_dconv_bilinear_supported(32, H, W, hs, ws);
    };
    if (w.ne[1] == 3 && w.ne[2] == 3) {
        if (!loader_can(cn, w, (int)x.ne[0])) return false;
        resized_in[t] = {buf_of(up.src[0]), hs, ws};
        return true;
    }
    if (!(w.ne[1] == 1 && w.ne[2] == 1 && cn.ip[0] == 1 && cn.ip[1] == 0) || cn.ne[0] % 8 || x.ne[0] % 64) return false;
    // the projection on the small map (where the residual unit in front of the resize has not applied it already)
    const int cout = (int)cn.ne[0];
    const int64_t M = (int64_t)B * hs * ws;
    int sbuf;
    if (auto it = preprojected.find(t); it != preprojected.end()) sbuf = it->second;
    else {
        product P;
        pack_conv_rows(P, cn, false);
        sbuf = new_buffer((size_t)M * cout * 2);
        P.in.buf = buf_of(up.src[0]);
        P.out.buf = sbuf;
        vx_gemm_args& a = P.a;
        a.lda = P.p.K; a.M = (int)M; a.n_valid = cout; a.ldo = cout; a.epi = VX_EPI_F16;
        std::string who = g.nodes[cn.src[1]].name;
        P.desc = "gemm(conv1x1 before its resize) M=" + std::to_string(M) + " N=" + std::to_string(cout) + " K=" + std::to_string(P.p.k_real) + " <- " + who;
        P.group = group_of(who, cn, 1);
        P.flops = 2.0 * M * (double)cout * P.p.k_real;
        P.bytes = (double)M * (P.p.k_real + cout) * 2; // (without the operand's image)
        emit_product(P);
    }
    auto sp = ptr(sbuf);
    skip[t] = 1;
    skip[c] = 1;
    // ... and its resize: by the next conv's loader where that is the only reader, else by the resize kernel into the conv node's buffer
    const int c2 = cn.is_output ? -1 : sole_consumer(c);
    if (c2 >= 0 && g.nodes[c2].op == gop_conv_2d && g.nodes[c2].src[0] == c) {
        graph_node const& w2 = g.nodes[g.nodes[c2].src[1]];
        if (w2.ne[1] == 3 && w2.ne[2] == 3 && loader_can(g.nodes[c2], w2, cout)) {
            resized_in[c] = {sbuf, hs, ws};
            return true;
        }
    }
    materialise(c);
    const int obuf = cn.buffer;
    auto op = ptr(obuf);
    char d[128];
    snprintf(d, sizeof d, "bilinear_ac %dx%d -> %dx%d C=%d", ws, hs, W, H, cout);
    emit(d, {sbuf}, {obuf}, [=](void* st) { VX(vx_bilinear_ac_f16(sp(), op(), B, hs, ws, cout, H, W, st)); });
    tag("bilinear", 0, (double)B * ((double)hs * ws + (double)H * W) * cout * 2);
    return true;
}


// ---- deformable convolution (nn.cpp:131-148) -----------------------------------------------------------------------------------------------

// deformable_conv_2d + the branch's batch norm and ReLU as the reference writes them (birefnet.cpp:83-92, 110-115): offset and modulator convs over
// the same x, stride and pad as the deformable conv, each link read by the next one only
bool lowering::match_deform_group(int t, deform_group& G) const {
    graph_node const& n = g.nodes[t];
    if (n.op != gop_conv_2d_deform || n.n_src != 4) return false;
    const int x = n.src[0];
    auto conv_on_x = [&](int c) {
        graph_node const& cn = g.nodes[c];
        return cn.op == gop_conv_2d && !cn.constant && cn.src[0] == x && cn.ip[0] == 1 && cn.ip[1] == n.ip[1] &&
               g.nodes[cn.src[1]].ne[1] == g.nodes[n.src[1]].ne[1] && g.nodes[cn.src[1]].ne[2] == g.nodes[n.src[1]].ne[2] && sole_consumer(c) >= 0;
    };
    G.off = n.src[2];
    G.scl = n.src[3];
    if (!conv_on_x(G.off) || sole_consumer(G.off) != t) return false;
    if (g.nodes[G.scl].op != gop_scale || g.nodes[G.scl].constant || sole_consumer(G.scl) != t) return false;
    G.s = g.nodes[G.scl].fp[0];
    G.sig = g.nodes[G.scl].src[0];
    if (g.nodes[G.sig].op != gop_sigmoid || g.nodes[G.sig].constant || sole_consumer(G.sig) != G.scl) return false;
    G.mod = g.nodes[G.sig].src[0];
    if (!conv_on_x(G.mod) || sole_consumer(G.mod) != G.sig || G.mod == G.off) return false;
    // [mul(c)] [add(c)] [relu] on per-channel constants behind it
    auto per_channel = [&](int c, int32_t op, int from) {
        graph_node const& cn = g.nodes[c];
        return cn.op == op && cn.src[0] == from && g.nodes[cn.src[1]].constant && g.nodes[cn.src[1]].n_elements() == n.ne[0];
    };
    int last = t, c = sole_consumer(t);
    if (c >= 0 && per_channel(c, gop_mul, last)) { G.mul = c; last = c; c = sole_consumer(c); }
    if (c >= 0 && per_channel(c, gop_add, last)) { G.add = c; last = c; c = sole_consumer(c); }
    if (c >= 0 && g.nodes[c].op == gop_relu && g.nodes[c].src[0] == last) G.relu = c;
    return true;
}
// before the node loop: the convs of a group come before their deformable conv in node order and must not be lowered on their own
void lowering::find_deform_groups() {
    if (!g.fused_models) return;
    for (int t = 0; t < (int)g.nodes.size(); ++t) {
        deform_group G;
        if (!needed[t] || !match_deform_group(t, G)) continue;
        deform_groups[t] = G;
        for (int c : {G.off, G.mod, G.sig, G.scl}) skip[c] = 1;
        claim(t, {G.off, G.mod, G.sig, G.scl, G.mul, G.add, G.relu}); // (the tail is absorbed when the launch is emitted)
    }
}

// any use of the op: offsets and mask are read where they are, the mask as it is
void lowering::deform_conv(int t) {
    if (auto it = deform_groups.find(t); it != deform_groups.end()) return deform_fused(t, it->second);
    graph_node& n = g.nodes[t];
    graph_node const &x = g.nodes[n.src[0]], &w = g.nodes[n.src[1]];
    vx_deform_conv_args a;
    memset(&a, 0, sizeof a);
    a.B = (int)x.ne[3]; a.H = (int)x.ne[2]; a.W = (int)x.ne[1]; a.Cin = (int)x.ne[0];
    a.Cout = (int)n.ne[0]; a.k = (int)w.ne[1]; a.pad = (int)n.ip[1];
    const int taps = a.k * a.k;
    a.ld_offset = 2 * taps; a.ld_mask = taps; a.mask_mode = n.n_src == 4 ? 1 : 0; a.mask_scale = 1.0f;
    a.ldo = a.Cout;
    int n_pad = 0;
    a.w = pack_deform(n.src[1], &n_pad);
    std::vector<int> reads = {buf_of(n.src[0])};
    auto xp = ptr(reads[0]);
    // offsets and mask: activations in their buffers, or constants uploaded as f16
    std::function<char*()> op_, mp_;
    void *oc = nullptr, *mc = nullptr;
    if (g.nodes[n.src[2]].constant) oc = const_f16(n.src[2]);
    else { reads.push_back(buf_of(n.src[2])); op_ = ptr(reads.back()); }
    if (n.n_src == 4) {
        if (g.nodes[n.src[3]].constant) mc = const_f16(n.src[3]);
        else { reads.push_back(buf_of(n.src[3])); mp_ = ptr(reads.back()); }
    }
    materialise(t);
    const int obuf = n.buffer;
    auto outp = ptr(obuf);
    const std::string who = weight_name(g, n);
    const int M = (int)(n.ne[1] * n.ne[2] * n.ne[3]);
    char d[320];
    snprintf(d, sizeof d, "deform_conv%s M=%d N=%d K=%d k=%d <- %s", n.n_src == 4 ? "[mask]" : "", M, a.Cout, taps * a.Cin, a.k, who.c_str());
    emit(d, reads, {obuf}, [=](void* st) {
        vx_deform_conv_args r = a;
        r.x = xp();
        r.offset = oc ? oc : op_();
        r.mask = r.mask_mode ? (mc ? mc : mp_()) : nullptr;
        r.out = outp();
        VX(vx_deform_conv_f16(&r, st));
    });
    tag("deform_conv", 2.0 * M * (double)a.Cout * taps * a.Cin, (double)M * (a.Cin + a.Cout + 3.0 * taps) * 2);
}

// the matched group: ONE conv / GEMM computes offsets and modulator logits side by side, ONE deform_conv launch reads them in logits mode and applies the
// per-channel scale, bias and ReLU
void lowering::deform_fused(int t, deform_group const& G) {
    graph_node& n = g.nodes[t];
    graph_node const &x = g.nodes[n.src[0]], &w = g.nodes[n.src[1]];
    graph_node const &on = g.nodes[G.off], &mn = g.nodes[G.mod];
    const int k = (int)w.ne[1], taps = k * k, pad = (int)n.ip[1], Cin = (int)x.ne[0];
    const int M = (int)(n.ne[1] * n.ne[2] * n.ne[3]);
    const std::string who = weight_name(g, n);
    const packed_operand p = pack_deform_offsets(on.src[1], on.n_src == 3 ? on.src[2] : -1, mn.src[1], mn.n_src == 3 ? mn.src[2] : -1);
    const int ldom = round_up(3 * taps, 8);
    const int xbuf = buf_of(n.src[0]);
    const int ombuf = new_buffer((size_t)M * ldom * 2);
    auto xp = ptr(xbuf), omp = ptr(ombuf);
    {
        product P;
        P.operand(p);
        P.in.buf = xbuf;
        P.out.buf = ombuf;
        vx_gemm_args& a = P.a;
        a.M = M; a.n_valid = ldom; a.ldo = ldom; a.epi = VX_EPI_F16;
        const bool plain = k == 1 && pad == 0 && Cin % 64 == 0; // a plain product on the pixel rows; every other shape through the conv loader
        if (plain) a.lda = Cin;
        else conv_geometry(a, n, x, w);
        char d[320];
        snprintf(d, sizeof d, "deform_offsets %s M=%d N=%d K=%d <- %s", plain ? "gemm" : ("conv" + std::to_string(k) + "x" + std::to_string(k)).c_str(), M, p.n_real, p.k_real,
                 weight_name(g, on).c_str());
        P.desc = d;
        P.group = "deform_offsets";
        P.work(Cin, p.n_real); // (one read of x, not of its k^2 taps)
        emit_product(P);
    }
    vx_deform_conv_args a;
    memset(&a, 0, sizeof a);
    a.B = (int)x.ne[3]; a.H = (int)x.ne[2]; a.W = (int)x.ne[1]; a.Cin = Cin;
    a.Cout = (int)n.ne[0]; a.k = k; a.pad = pad;
    a.ld_offset = ldom; a.ld_mask = ldom; a.mask_mode = 2; a.mask_scale = G.s;
    a.ldo = a.Cout;
    int n_pad = 0;
    a.w = pack_deform(n.src[1], &n_pad);
    if (G.mul >= 0) a.scale = const_f32(g.nodes[G.mul].src[1]);
    if (G.add >= 0) a.bias = const_f32(g.nodes[G.add].src[1]);
    a.relu = G.relu >= 0;
    absorb(std::vector<int>{G.mul, G.add, G.relu}, t);
    materialise(t);
    const int obuf = n.buffer;
    auto outp = ptr(obuf);
    char d[320];
    snprintf(d, sizeof d, "deform_conv[logits x%g]%s%s%s M=%d N=%d K=%d k=%d <- %s", G.s, G.mul >= 0 ? "[*scale]" : "", G.add >= 0 ? "[+bias]" : "", G.relu >= 0 ? "[relu]" : "", M,
             a.Cout, taps * Cin, k, who.c_str());
    emit(d, {xbuf, ombuf}, {obuf}, [=](void* st) {
        vx_deform_conv_args r = a;
        r.x = xp();
        r.offset = omp();
        r.mask = omp() + (size_t)2 * taps * 2;
        r.out = outp();
        VX(vx_deform_conv_f16(&r, st));
    });
    tag("deform_conv", 2.0 * M * (double)a.Cout * taps * Cin, (double)M * (Cin + a.Cout + ldom) * 2);
}

// ---- depthwise convolution (nn.cpp:102-115) and the 3-channel image in front of a model's first conv ---------------------------------------------

// the 8-channel f16 pixels of a 3- or 4-channel f32 image, made once per image whoever reads it
int lowering::image_pad8(int xs) {
    const int r = root(xs);
    if (auto it = image8.find(r); it != image8.end()) return it->second;
    graph_node const& x = g.nodes[r];
    const int64_t px = x.ne[1] * x.ne[2] * x.ne[3];
    const int src = buf_of(r), dst = new_buffer((size_t)px * 16);
    auto sp = ptr(src), dp = ptr(dst);
    if (x.ne[0] == 4) {
        emit("image4_pad8 " + shape_str(x.ne), {src}, {dst}, [=](void* st) { VX(vx_image4_pad8_f32(reinterpret_cast<const float*>(sp()), dp(), px, st)); });
        tag("preprocess", 0, (double)px * 32);
    } else {
        emit("image_pad8 " + shape_str(x.ne), {src}, {dst}, [=](void* st) { VX(vx_image_pad8_f32(reinterpret_cast<const float*>(sp()), dp(), px, st)); });
        tag("preprocess", 0, (double)px * 28);
    }
    image8[r] = dst;
    return dst;
}

// one launch of a depthwise kernel (kernels_dwconv.hip, or kernels_tinyvit.hip's for 3x3 / pad 1); with fused models a gelu / leaky_relu that is its only reader joins it
void lowering::depthwise_conv(int t) {
    graph_node& n = g.nodes[t];
    graph_node const &x = g.nodes[n.src[0]], &w = g.nodes[n.src[1]];
    const int C = (int)x.ne[0], k = (int)(w.ne[0] == C && w.ne[1] == 1 ? w.ne[2] : w.ne[1]);
    const int B = (int)x.ne[3], H = (int)x.ne[2], W = (int)x.ne[1], stride = (int)n.ip[0], pad = (int)n.ip[1];
    void* wp = pack_depthwise(n.src[1], C, k);
    const float* bp = n.n_src == 3 ? const_f32(n.src[2]) : nullptr;
    int act = 0;
    float act_param = 0.0f;
    if (const int c = sole_consumer(t); g.fused_models && c >= 0 && (g.nodes[c].op == gop_gelu || g.nodes[c].op == gop_leaky_relu)) {
        act = g.nodes[c].op == gop_gelu ? 1 : 2;
        act_param = g.nodes[c].fp[0];
        absorb(std::vector<int>{c}, t);
    }
    const std::string who = weight_name(g, n);
    const int xbuf = buf_of(n.src[0]);
    materialise(t);
    const int obuf = n.buffer;
    auto xp = ptr(xbuf), op = ptr(obuf);
    char d[320];
    snprintf(d, sizeof d, "dwconv%dx%d%s%s B=%d %dx%d -> %lldx%lld C=%d pad=%d <- %s", k, k, stride > 1 ? "s2" : "", act == 1 ? "[gelu]" : (act == 2 ? "[leaky_relu]" : ""), B, W, H,
             (long long)n.ne[1], (long long)n.ne[2], C, pad, who.c_str());
    // 3x3 / pad 1 with a bias and no activation but GELU is what the hand schedule's kernel computes, to the same bits and measurably faster at stride 1
    // (tools/bench_dwconv.py): those launches go to it, everything else to the generic kernel
    const bool hand3x3 = k == 3 && pad == 1 && bp && act != 2;
    emit(d, {xbuf}, {obuf}, [=](void* st) {
        if (hand3x3) VX(vx_dwconv3x3_f16(xp(), wp, bp, op(), B, H, W, C, stride, act == 1, st));
        else VX(vx_dwconv_f16(xp(), wp, bp, op(), B, H, W, C, k, stride, pad, act, act_param, st));
    });
    tag("dwconv", 2.0 * (double)n.n_elements() * k * k, (double)(x.n_elements() + n.n_elements()) * 2 + (double)k * k * C * 2);
}

} // namespace visp
