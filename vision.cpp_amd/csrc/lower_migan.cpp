// Graph lowering: the node groups of MI-GAN (migan.cpp), and the launches of clamp and of add / mul / sub with a plane operand (see lowering.h). What
// csrc/migan.cpp's hand schedule does by construction is matched here from nodes, for any width that is a multiple of 8:
//   (a) conv_2d_depthwise -> leaky_relu -> [scale] -> [clamp(-c, c)] (lrelu_agc, migan.cpp:17-26) is one vx_dwconv_agc_f16 launch;
//   (b) conv_2d 1x1 -> [add(plane constant)] -> lrelu_agc(0.2, sqrt2, 256) -> [add(map of the same shape)] is one launch of the plain product with the
//       VX_EPI_LRELU_AGC epilogue, on the rows where they lie whatever their width (migan_product says how), the 8-channel pixels of the f32 image included;
//       a bare 1x1 conv that reads the map such a group wrote (torgb) is the implicit conv with the plain f16 epilogue: no padded copy of its rows either;
//   (c) interpolate(x2, NEAREST) -> mul(plane constant equal to the tile [[1, 0], [0, 0]]) -> conv_2d_depthwise(4x4, stride 1, pad 2, no bias) ->
//       slice(W: 0..-1, H: 0..-1) -> [cont] (upsample_2d, migan.cpp:32-51) -> [add(plane constant)] -> [lrelu_agc] -> [add(map)] is one vx_upfirdn2x_f16 launch.
//       With any other constant the zero insertion does not hold and the group stays per node.
// Every link is read by the next one only. A group is emitted where its LAST node stands, when everything it reads (the residual map above all: torgb's
// output is made after the image upsample's nodes, migan.cpp:120-124) exists; the nodes before it are computed by nobody. Matchers are const and run before the
// node loop (find_migan_groups); with fused_models off none of this runs and every node is one launch.
#include <cmath>
#include <limits>

#include "lowering.h"

namespace visp {

namespace {

constexpr float AGC_SLOPE = 0.2f, AGC_GAIN = 1.41421356f, AGC_CLAMP = 256.0f; // what VX_EPI_LRELU_AGC computes (kernels_gemm.hip)

} // namespace

// [add(plane constant)] -> [leaky_relu -> [scale] -> [clamp(-c, c)]] -> [add(map of the same shape)] behind `from`, each read by the next only and none of them
// taken by another pattern or by a group found before (two chains that meet in one add: the first takes it with the second's last map as its residual, the
// second ends in front of it)
lowering::agc_tail lowering::match_agc_tail(int from, bool allow_plane, bool allow_add) const {
    agc_tail T;
    T.last = from;
    int c = sole_consumer(from);
    auto take = [&](int node) { T.absorbed.push_back(node); T.last = node; c = sole_consumer(node); if (!free_node(c)) c = -1; };
    if (!free_node(c)) c = -1;
    if (allow_plane && c >= 0 && g.nodes[c].op == gop_add && g.nodes[c].src[0] == T.last) {
        graph_node const& b = g.nodes[g.nodes[c].src[1]];
        if (b.constant && plane_broadcast(g.nodes[c].ne, b.ne)) { T.plane = g.nodes[c].src[1]; take(c); }
    }
    if (c >= 0 && g.nodes[c].op == gop_leaky_relu && g.nodes[c].dtype == gdt_f16) {
        T.act = true;
        T.slope = g.nodes[c].fp[0];
        take(c);
        if (c >= 0 && g.nodes[c].op == gop_scale && g.nodes[c].dtype == gdt_f16) { T.gain = g.nodes[c].fp[0]; take(c); }
        if (c >= 0 && g.nodes[c].op == gop_clamp && g.nodes[c].fp[0] == -g.nodes[c].fp[1] && g.nodes[c].fp[1] > 0.0f) { T.clamp = g.nodes[c].fp[1]; take(c); }
    }
    if (allow_add && c >= 0 && g.nodes[c].op == gop_add) {
        graph_node const& a = g.nodes[c];
        const int other = a.src[0] == T.last ? a.src[1] : a.src[0];
        graph_node const& o = g.nodes[other];
        if (other != T.last && !o.constant && o.dtype == gdt_f16 && same_shape(o, a) && (a.src[0] == T.last || a.src[1] == T.last)) { T.res = other; take(c); }
    }
    return T;
}

bool lowering::match_upfir_group(int t, upfir_group& G) const {
    graph_node const& up = g.nodes[t];
    if (up.op != gop_interpolate || up.constant || (up.ip[2] & 255) != 0) return false;
    graph_node const& x = g.nodes[up.src[0]];
    if (x.constant || x.dtype != gdt_f16 || x.ne[0] % 8 || up.ne[1] != 2 * x.ne[1] || up.ne[2] != 2 * x.ne[2]) return false;
    const int m = sole_consumer(t);
    if (!free_node(m) || g.nodes[m].op != gop_mul || g.nodes[m].src[0] != t) return false;
    graph_node const& f = g.nodes[g.nodes[m].src[1]];
    if (!f.constant || !plane_broadcast(up.ne, f.ne)) return false;
    // zero insertion holds only for the tile [[1, 0], [0, 0]] (csrc/migan.cpp compares the same way when it loads a file)
    const int64_t W2 = up.ne[1], H2 = up.ne[2];
    for (int64_t yy = 0; yy < H2; ++yy)
        for (int64_t xx = 0; xx < W2; ++xx)
            if (f.values()[yy * W2 + xx] != ((xx | yy) & 1 ? 0.0f : 1.0f)) return false;
    const int d = sole_consumer(m);
    if (!free_node(d) || g.nodes[d].op != gop_conv_2d_depthwise || g.nodes[d].src[0] != m || g.nodes[d].n_src != 2 || g.nodes[d].ip[0] != 1 || g.nodes[d].ip[1] != 2) return false;
    graph_node const& dn = g.nodes[d];
    if (dn.ne[1] != W2 + 1 || dn.ne[2] != H2 + 1) return false; // a 4x4 kernel
    const int s = sole_consumer(d);
    if (!free_node(s) || g.nodes[s].op != gop_slice) return false;
    graph_node const& sl = g.nodes[s];
    for (int dim = 0; dim < 4; ++dim)
        if (sl.ip[3 * dim] != 0 || sl.ip[3 * dim + 2] != 1 || sl.ne[dim] != up.ne[dim]) return false;
    G.src = up.src[0];
    G.fir = dn.src[1];
    G.members = {t, m, d, s};
    int last = s;
    if (const int c = sole_consumer(s); free_node(c) && g.nodes[c].op == gop_cont) { G.members.push_back(c); last = c; }
    G.tail = match_agc_tail(last, true, true);
    if (G.tail.act && G.tail.slope != AGC_SLOPE) { // (the kernel's slope is 0.2: the nodes behind the upsample stay launches)
        G.tail = agc_tail{};
        G.tail.last = last;
    }
    return true;
}

void lowering::find_migan_groups() {
    if (!g.fused_models) return;
    const int N = (int)g.nodes.size();
    // a group is keyed on its LAST node, where its launch is emitted; the nodes in front of it are computed by nobody
    std::vector<char> group_last(N, 0);
    auto accept = [&](std::vector<int> const& nodes, int last) {
        claim(last, nodes);
        group_last[last] = 1;
        for (int c : nodes)
            if (c != last) skip[c] = 1;
    };
    for (int t = 0; t < N; ++t) {
        if (!free_node(t) || g.nodes[t].constant) continue;
        graph_node const& n = g.nodes[t];
        if (n.op == gop_interpolate) { // (c)
            upfir_group G;
            if (!match_upfir_group(t, G)) continue;
            std::vector<int> all = G.members;
            all.insert(all.end(), G.tail.absorbed.begin(), G.tail.absorbed.end());
            accept(all, G.tail.last);
            upfir_at[G.tail.last] = G;
        } else if (n.op == gop_conv_2d_depthwise && n.dtype == gdt_f16) { // (a): only with a scale or a clamp; a bare leaky_relu is depthwise_conv's own epilogue
            agc_tail T = match_agc_tail(t, false, false);
            if (!T.act || (T.gain == 1.0f && T.clamp == 0.0f)) continue;
            std::vector<int> all = T.absorbed;
            all.push_back(t);
            accept(all, T.last);
            dw_agc_at[T.last] = {t, T};
        } else if (n.op == gop_conv_2d && n.dtype == gdt_f16 && n.ne[0] % 8 == 0) { // (b)
            graph_node const &w = g.nodes[n.src[1]], &x = g.nodes[n.src[0]];
            if (w.ne[1] != 1 || w.ne[2] != 1 || n.ip[0] != 1 || n.ip[1] != 0 || (n.n_src == 3 && !g.nodes[n.src[2]].constant) || x.constant) continue;
            const bool image = x.op == gop_input && image8_input(x);
            if (!image) {
                // an f16 map in a buffer of its own, as wide as its pixels: not one a product may have written with padded rows, nor a view another pattern reads in place
                const int32_t xop = g.nodes[root_view(n.src[0])].op;
                const bool plain_map = xop == gop_input || xop == gop_conv_2d_depthwise || xop == gop_add || xop == gop_mul || xop == gop_sub || xop == gop_clamp || xop == gop_scale ||
                                       xop == gop_leaky_relu;
                if (x.dtype != gdt_f16 || x.ne[0] % 8 || !plain_map) continue;
                // (the last node of a SiLU group is an add, too: where lower_yolo.cpp places it in a concat's buffer, or reads a slice in its source, the conv
                // stays that file's, which addresses it there)
                if (will_live_in_place(n.src[0])) continue;
            }
            agc_tail T = match_agc_tail(t, true, true);
            const bool agc = T.act && T.slope == AGC_SLOPE && T.gain == AGC_GAIN && T.clamp == AGC_CLAMP;
            // without the epilogue's exact constants: a bare conv, taken only behind a group's map (its rows then need no padded copy either)
            if (!agc) {
                if (!group_last[root_view(n.src[0])]) continue;
                // ... and only where no other lowering has plans for it: a SiLU group, a conv that writes into its slice of a concat (lower_yolo.cpp), or
                // one whose reader the generic product would take into its epilogue (gelu / relu / LayerScale / a residual add)
                if (silu_convs.count(t) || cat_slot.count(t)) continue;
                if (const int c = sole_consumer(t); c >= 0 && !(claimed_by[c] >= 0 && group_last[claimed_by[c]]) && // (a reader in a group of this file's takes t as it is)
                    (g.nodes[c].op == gop_gelu || g.nodes[c].op == gop_relu || g.nodes[c].op == gop_add || g.nodes[c].op == gop_mul))
                    continue;
                T = agc_tail{};
                T.last = t;
            }
            std::vector<int> all = T.absorbed;
            all.push_back(t);
            accept(all, T.last);
            conv_agc_at[T.last] = {t, T};
        }
    }
}

bool lowering::will_live_in_place(int v) const {
    for (;; v = g.nodes[v].src[0]) {
        if (chan_slice.count(v) || cat_slot.count(v)) return true;
        if (g.nodes[v].op != gop_cont && g.nodes[v].op != gop_reshape) return false;
    }
}

// What the graph alone proves about |values| of the f16 map v: a clamp's bounds, carried through views, sums of maps and depthwise convs with constant kernels
// (bound * the largest channel's sum of |taps| + the largest |bias|). Anything else, or a bound an f16 cannot hold, is infinity: the map may hold an inf.
double lowering::value_bound(int v) {
    if (auto it = bound_memo.find(v); it != bound_memo.end()) return it->second;
    graph_node const& n = g.nodes[v];
    const double inf = std::numeric_limits<double>::infinity();
    double b = inf;
    auto max_abs = [&](int c) {
        double m = 0.0;
        for (int64_t i = 0; i < g.nodes[c].n_elements(); ++i) m = std::max(m, (double)std::fabs(g.nodes[c].values()[i]));
        return m;
    };
    if (n.constant) b = max_abs(v);
    else if (n.op == gop_clamp) b = std::max(std::fabs((double)n.fp[0]), std::fabs((double)n.fp[1]));
    else if (n.op == gop_cont || n.op == gop_reshape || n.op == gop_slice) b = value_bound(n.src[0]);
    else if (n.op == gop_add || n.op == gop_sub) b = value_bound(n.src[0]) + value_bound(n.src[1]);
    else if (n.op == gop_conv_2d_depthwise) {
        graph_node const& w = g.nodes[n.src[1]];
        const int64_t C = n.ne[0], taps = w.n_elements() / C;
        const bool channel_first = w.ne[0] == C && w.ne[1] == 1;
        double worst = 0.0;
        for (int64_t c = 0; c < C; ++c) {
            double s = 0.0;
            for (int64_t t = 0; t < taps; ++t) s += std::fabs((double)w.values()[channel_first ? t * C + c : c * taps + t]);
            worst = std::max(worst, s);
        }
        b = value_bound(n.src[0]) * worst + (n.n_src == 3 ? max_abs(n.src[2]) : 0.0);
    }
    if (!(b < 65504.0)) b = inf;
    bound_memo[v] = b;
    return b;
}

bool lowering::migan_emits(int t) {
    if (auto it = upfir_at.find(t); it != upfir_at.end()) { migan_upfir(t, it->second); return true; }
    if (auto it = dw_agc_at.find(t); it != dw_agc_at.end()) { migan_depthwise(t, it->second.first, it->second.second); return true; }
    if (auto it = conv_agc_at.find(t); it != conv_agc_at.end()) { migan_product(t, it->second.first, it->second.second); return true; }
    return false;
}

// the f32 plane a fused epilogue adds per pixel: the [1, W, H, 1] constant's values as they are
float* lowering::plane_f32(int t) {
    return static_cast<float*>(cached(t, role_plane_f32, [&](bool st) { return upload(g.nodes[t].values(), (size_t)g.nodes[t].n_elements() * 4, st); }));
}

static std::string tail_tag(lowering::agc_tail const& T) {
    std::string s;
    if (T.plane >= 0) s += "[+plane]";
    if (T.act) {
        char b[96];
        snprintf(b, sizeof b, "[lrelu_agc %g %g %g]", (double)T.slope, (double)T.gain, (double)T.clamp);
        s += b;
    }
    if (T.res >= 0) s += "[+res]";
    return s;
}

void lowering::migan_upfir(int last, upfir_group const& G) {
    graph_node const& x = g.nodes[G.src];
    graph_node& out = g.nodes[last];
    const int B = (int)x.ne[3], h = (int)x.ne[2], w = (int)x.ne[1], C = (int)x.ne[0];
    void* fir = pack_depthwise(G.fir, C, 4);
    const float* plane = G.tail.plane >= 0 ? plane_f32(G.tail.plane) : nullptr;
    // the map upsampled and the residual are read where they lie (a channel slice, a map inside a concat's buffer: lower_yolo.cpp), through their pixel strides
    const located in = locate(G.src);
    std::vector<int> reads = {in.buf};
    located res{-1, 0, C};
    std::function<char*()> rp;
    if (G.tail.res >= 0) {
        res = locate(G.tail.res);
        reads.push_back(res.buf);
        rp = ptr(res.buf);
    }
    materialise(last);
    const int obuf = out.buffer;
    auto xp = ptr(in.buf), op = ptr(obuf);
    const int64_t in_off = in.off, in_pix = in.pix, res_off = res.off, res_pix = res.pix;
    const int agc = G.tail.act;
    const float gain = G.tail.gain, clamp = G.tail.clamp;
    char d[320];
    snprintf(d, sizeof d, "upfirdn2x%s B=%d %dx%d -> %dx%d C=%d <- %s", tail_tag(G.tail).c_str(), B, w, h, 2 * w, 2 * h, C, weight_name(g, g.nodes[G.members[2]]).c_str());
    emit(d, reads, {obuf}, [=](void* st) { VX(vx_upfirdn2x_f16(xp() + in_off * 2, in_pix, fir, op(), C, plane, rp ? rp() + res_off * 2 : nullptr, res_pix, agc, gain, clamp, B, h, w, C, st)); });
    const double px = (double)B * h * w * C;
    tag("fir", 2.0 * 4 * px * 4, px * 2 * (1 + 4 * (G.tail.res >= 0 ? 2 : 1)) + (plane ? 16.0 * h * w : 0.0) + 32.0 * C);
}

void lowering::migan_depthwise(int last, int t, agc_tail const& T) {
    graph_node const& n = g.nodes[t];
    graph_node const &x = g.nodes[n.src[0]], &w = g.nodes[n.src[1]];
    const int C = (int)x.ne[0], k = (int)(w.ne[0] == C && w.ne[1] == 1 ? w.ne[2] : w.ne[1]);
    const int B = (int)x.ne[3], H = (int)x.ne[2], W = (int)x.ne[1], stride = (int)n.ip[0], pad = (int)n.ip[1];
    void* wp = pack_depthwise(n.src[1], C, k);
    const float* bp = n.n_src == 3 ? const_f32(n.src[2]) : nullptr;
    const int xbuf = buf_of(n.src[0]);
    materialise(last);
    const int obuf = g.nodes[last].buffer;
    auto xp = ptr(xbuf), op = ptr(obuf);
    const float slope = T.slope, gain = T.gain, clamp = T.clamp;
    char d[320];
    snprintf(d, sizeof d, "dwconv%dx%d%s%s B=%d %dx%d -> %lldx%lld C=%d pad=%d <- %s", k, k, stride > 1 ? "s2" : "", tail_tag(T).c_str(), B, W, H, (long long)n.ne[1], (long long)n.ne[2], C, pad,
             weight_name(g, n).c_str());
    emit(d, {xbuf}, {obuf}, [=](void* st) { VX(vx_dwconv_agc_f16(xp(), wp, bp, op(), B, H, W, C, k, stride, pad, slope, gain, clamp, st)); });
    tag("fir", 2.0 * (double)n.n_elements() * k * k, (double)(x.n_elements() + n.n_elements()) * 2 + (double)k * k * C * 2);
}

void lowering::migan_product(int last, int t, agc_tail const& T) {
    graph_node const& n = g.nodes[t];
    const int xs = n.src[0];
    graph_node const& x = g.nodes[xs];
    const std::string who = weight_name(g, n);
    product P;
    auto& a = P.a;
    const bool image8_in = image8_input(x); // (the only f32 input find_migan_groups admits)
    std::string kind;
    a.M = (int)(n.ne[1] * n.ne[2] * n.ne[3]);
    if (T.act) {
        // VX_EPI_LRELU_AGC exists on the plain product only, whose loader reads whole 64-wide k tiles. Where the rows are narrower (Cin % 64 != 0, the 8-channel
        // image pixels) they are NOT copied into padded rows: the operand's columns behind Cin are zero, and what the loader reads there are the following
        // pixels of the same map -- finite f16 values, so 0 * them is 0 -- and, behind the last row, the buffer's own slack (new_buffer: 256 bytes), which this
        // launch zeroes first (the buffer is among the launch's writes for that). 0 * inf is a NaN, so this is done only where the graph proves the map finite
        // (value_bound: every map MI-GAN feeds here is clamped or a FIR of a clamped map); any other map is copied into padded rows, as per node, and so is a
        // graph input or output, which may be bound to a caller's buffer that has no slack. (The 8-channel pixels of the f32 image are as finite as the image.)
        pack_conv_rows(P, n, image8_in);
        const int cin = image8_in ? 8 : (int)x.ne[0], Kp = P.p.K;
        bool copy = !image8_in && cin != Kp && !(value_bound(xs) < 65504.0);
        for (int v = xs; !image8_in && cin != Kp && v >= 0; v = g.nodes[v].alias_of) copy = copy || g.nodes[v].op == gop_input || g.nodes[v].is_output; // xs and every view down to its root
        if (copy) {
            P.in.buf = padded_rows(xs, cin, Kp, a.M, who);
            a.lda = Kp;
        } else {
            P.in.buf = image8_in ? image_pad8(xs) : buf_of(xs);
            a.lda = cin;
            if (cin != Kp) P.zero_at = (size_t)a.M * cin * 2; // the slack behind the A rows
        }
        kind = "gemm(conv1x1)";
    } else { // the plain f16 epilogue: the implicit conv reads rows of any width % 8
        pack_conv_rows(P, n, false);
        P.in.buf = buf_of(xs);
        conv_geometry(a, n, x, g.nodes[n.src[1]]);
        kind = "conv1x1";
    }
    a.n_valid = (int)n.ne[0];
    a.ldo = n.ne[0];
    a.epi = T.act ? VX_EPI_LRELU_AGC : VX_EPI_F16;
    if (T.plane >= 0) { a.noise = plane_f32(T.plane); a.noise_hw = (int)(n.ne[1] * n.ne[2]); }
    if (T.res >= 0) P.res1.buf = buf_of(T.res);
    materialise(last);
    P.out.buf = g.nodes[last].buffer;
    char d[360];
    snprintf(d, sizeof d, "%s%s M=%d N=%d K=%d <- %s", kind.c_str(), tail_tag(T).c_str(), a.M, (int)n.ne[0], P.p.k_real, who.c_str());
    P.desc = d;
    P.group = "conv";
    P.work(P.p.k_real + (T.res >= 0 ? (double)n.ne[0] : 0.0), (double)n.ne[0]);
    emit_product(P);
}

// ggml_clamp on an f16 activation
void lowering::clamp_op(int t) {
    graph_node const& n = g.nodes[t];
    const int64_t cnt = n.n_elements();
    const float lo = n.fp[0], hi = n.fp[1];
    map_launch(t, "clamp n=" + std::to_string(cnt), [=](char* x, char* o, char*, void* st) { VX(vx_clamp_f16(x, o, cnt, lo, hi, st)); });
    tag("fir", 0, (double)cnt * 4);
}

// add / mul / sub of a map [C, W, H, N] and a plane [1, W, H, 1] (a constant, read as f32, or an f16 activation)
void lowering::plane_binary(int t) {
    graph_node& n = g.nodes[t];
    graph_node const& b = g.nodes[n.src[1]];
    if (g.nodes[n.src[0]].constant) throw except("%s: the larger operand is a constant; broadcast of an activation onto it is not built", graph_op_name(n.op));
    if (n.ne[0] % 8) throw except("%s: a plane operand on %lld channels (a multiple of 8)", graph_op_name(n.op), (long long)n.ne[0]);
    const int abuf = buf_of(n.src[0]);
    const int bop = n.op == gop_add ? 0 : (n.op == gop_mul ? 1 : 2), B = (int)n.ne[3], C = (int)n.ne[0];
    const int64_t HW = n.ne[1] * n.ne[2];
    std::vector<int> reads = {abuf};
    std::function<char*()> bp;
    float* bc = nullptr;
    if (b.constant) bc = const_f32(n.src[1]);
    else { reads.push_back(buf_of(n.src[1])); bp = ptr(reads.back()); }
    materialise(t);
    const int obuf = n.buffer;
    auto ap = ptr(abuf), op = ptr(obuf);
    char d[200];
    snprintf(d, sizeof d, "%s_plane B=%d HW=%lld C=%d%s", graph_op_name(n.op), B, (long long)HW, C, b.constant ? " (constant)" : "");
    emit(d, reads, {obuf}, [=](void* st) {
        if (bp) VX(vx_binary_plane_f16(bop, ap(), bp(), 0, op(), B, HW, C, st));
        else VX(vx_binary_plane_f16(bop, ap(), bc, 1, op(), B, HW, C, st));
    });
    tag("fir", (double)n.n_elements(), (double)n.n_elements() * 4);
}

} // namespace visp
