// Graph lowering: the patterns of a network built from SiLU convs, channel splits and channel concats (YOLO / ELAN / CSP; yolov9t.cpp), and the
// launches of pool_2d, soft_max and sum_rows (see lowering.h). What csrc/yolov9t.cpp's hand schedule does by construction is matched here from nodes:
//   (a) conv_2d / linear -> silu [-> add(map computed before)] is one GEMM-family launch with the SiLU epilogue, the residual added after the activation;
//   (b) silu(add(conv3x3(x), conv1x1(x))) (RepConv) is one 3x3 launch on weights folded on the host;
//   (c) a slice of channels [c0, c1) only, both multiples of 8, read by GEMM-family convs, pools, nearest resizes and channel concats, is no launch: its readers address
//       it in its source through a pixel stride;
//   (d) the sources of a channel concat that a GEMM-family launch (plain f16 or SiLU epilogue), the pool kernel or a nearest resize writes are written into their slice of
//       the concat's buffer; anything else is copied there;
//   (e) slice -> [cont] -> reshape [n, G, A, N] -> soft_max -> mul(constant [n]) -> sum_rows is one softmax-expectation launch on the sliced map's rows.
// Every matcher is const and runs before the node loop (find_yolo_groups); the node loop applies exactly what was matched. With fused_models off none
// of this runs and every node is one launch.
#include "lowering.h"

namespace visp {

bool lowering::channels_only(graph_node const& s) const {
    graph_node const& x = g.nodes[s.src[0]];
    if (s.op != gop_slice || s.constant || s.is_output || x.dtype != gdt_f16 || s.ip[2] != 1) return false;
    for (int d = 1; d < 4; ++d)
        if (s.ip[3 * d] != 0 || s.ne[d] != x.ne[d] || s.ip[3 * d + 2] != 1) return false;
    return s.ip[0] % 8 == 0 && s.ip[1] % 8 == 0;
}
// who reads t, looking through cont nodes (views here); an output among the conts counts as the reader -1
std::vector<int> lowering::readers_through_conts(int t) const {
    std::vector<int> out;
    for (int c : consumers[t]) {
        if (g.nodes[c].op != gop_cont) { out.push_back(c); continue; }
        if (g.nodes[c].is_output) out.push_back(-1);
        for (int r : readers_through_conts(c)) out.push_back(r);
    }
    return out;
}
// c reads `view` as the input of a conv that yolo_product will emit
bool lowering::gemm_family_reader(int c, int view) const {
    graph_node const& n = g.nodes[c];
    int v = n.src[0]; // through cont views only: a reshape in between may change the pixel width
    while (v != view && g.nodes[v].op == gop_cont) v = g.nodes[v].src[0];
    if (n.op != gop_conv_2d || n.constant || n.dtype != gdt_f16 || n.ne[0] % 8 || v != view) return false;
    if (silu_convs.count(c) || rep_member.count(c)) return true;
    return !is_conv3x3(n, g.nodes[n.src[1]]); // (those may go to the LDS-ring kernels)
}
// every reader of t (outside `chain`, the concat nodes it is placed by) can address it inside a wider map
bool lowering::in_place_readers_ok(int t, std::vector<int> const& chain) const {
    for (int c : readers_through_conts(t)) {
        if (c < 0) return false;
        if (std::find(chain.begin(), chain.end(), c) != chain.end()) continue;
        graph_node const& n = g.nodes[c];
        if (n.op == gop_pool_2d || chan_slice.count(c) || gemm_family_reader(c, t)) continue;
        if (n.op == gop_interpolate && (n.ip[2] & 255) == 0 && n.ne[0] % 8 == 0) continue; // nearest: vx_nearest_pix_f16
        if (n.op == gop_concat && n.ip[0] == 0 && !n.constant) continue; // (copied from where it lies, or placed)
        return false;
    }
    return true;
}

bool lowering::match_silu_group(int t, silu_group& G) const {
    graph_node const& n = g.nodes[t];
    if ((n.op != gop_conv_2d && n.op != gop_linear) || n.constant || n.dtype != gdt_f16 || n.ne[0] % 8 || (n.n_src == 3 && !g.nodes[n.src[2]].constant)) return false;
    // the input is an f16 activation, or (conv_2d) the 3-channel f32 image that image_pad8 turns into f16 pixels
    {
        graph_node const& x = g.nodes[n.src[0]];
        if (x.constant || !(x.dtype == gdt_f16 || (n.op == gop_conv_2d && x.dtype == gdt_f32 && x.ne[0] == 3))) return false;
    }
    // (a ReLU or a bilinear resize in front of a conv may be taken by that conv's loader, or take the conv over: resize_into_reader)
    if (g.nodes[n.src[0]].op == gop_relu || (g.nodes[n.src[0]].op == gop_interpolate && (g.nodes[n.src[0]].ip[2] & 255) != 0)) return false;
    int c = sole_consumer(t), last = t;
    if (c >= 0 && g.nodes[c].op == gop_add && n.op == gop_conv_2d) { // RepConv: this 3x3 + a 1x1 on the same map at the same stride, each read by the add only
        graph_node const &a = g.nodes[c], &w = g.nodes[n.src[1]];
        const int o = a.src[0] == t ? a.src[1] : a.src[0];
        graph_node const& on = g.nodes[o];
        if (o == t || w.ne[1] != 3 || w.ne[2] != 3 || n.ip[1] != 1 || on.op != gop_conv_2d || on.constant || sole_consumer(o) != c || on.src[0] != n.src[0] || on.ip[0] != n.ip[0] || on.ip[1] != 0)
            return false;
        graph_node const& ow = g.nodes[on.src[1]];
        if (ow.ne[1] != 1 || ow.ne[2] != 1 || ow.ne[3] != w.ne[3] || (on.n_src == 3 && !g.nodes[on.src[2]].constant) || g.nodes[n.src[0]].dtype != gdt_f16) return false;
        G.rep1 = o;
        G.rep_add = c;
        last = c;
        c = sole_consumer(c);
    }
    if (c < 0 || g.nodes[c].op != gop_silu || g.nodes[c].src[0] != last) return false;
    G.silu = c;
    const int a = sole_consumer(c);
    if (a >= 0 && g.nodes[a].op == gop_add) { // the shortcut of a RepBottleneck, added after the activation
        const int o = g.nodes[a].src[0] == c ? g.nodes[a].src[1] : g.nodes[a].src[0];
        graph_node const& on = g.nodes[o];
        if (o != c && !on.constant && on.dtype == gdt_f16 && o < std::min(t, G.rep1 >= 0 ? G.rep1 : t) && same_shape(on, n)) { G.add = a; G.res = o; }
    }
    return true;
}

bool lowering::match_dfl_group(int t, dfl_group& G) const {
    graph_node const& z = g.nodes[t];
    if (z.op != gop_sum_rows || z.constant) return false;
    const int mu = z.src[0];
    graph_node const& m = g.nodes[mu];
    if (m.op != gop_mul || m.constant || sole_consumer(mu) != t || !g.nodes[m.src[1]].constant) return false;
    const int sm = m.src[0];
    graph_node const& s = g.nodes[sm];
    if (s.op != gop_soft_max || sole_consumer(sm) != mu || g.nodes[m.src[1]].n_elements() != s.ne[0] || s.ne[0] > 64) return false;
    const int rs = s.src[0];
    if (g.nodes[rs].op != gop_reshape || sole_consumer(rs) != sm) return false;
    G.absorbed = {mu, sm, rs};
    int v = g.nodes[rs].src[0];
    while (g.nodes[v].op == gop_cont && sole_consumer(v) >= 0) { G.absorbed.push_back(v); v = g.nodes[v].src[0]; }
    graph_node const& sl = g.nodes[v];
    if (!channels_only(sl) || sole_consumer(v) < 0) return false;
    G.absorbed.push_back(v);
    graph_node const& r = g.nodes[rs];
    // [G n, pixels .., N] -> [n, G, A, N]: the rows of the sliced map in order
    if (sl.ne[0] != r.ne[0] * r.ne[1] || r.ne[2] * r.ne[3] != sl.ne[1] * sl.ne[2] * sl.ne[3]) return false;
    G.map = sl.src[0];
    G.c0 = (int)sl.ip[0];
    G.n = (int)r.ne[0];
    G.groups = (int)r.ne[1];
    G.proj = m.src[1];
    return true;
}

// s is the last node of a launch that can write with a pixel stride: the pool kernel, a nearest resize, a SiLU group on a conv, or a conv with the plain f16 epilogue
bool lowering::placeable_launch(int s) const {
    graph_node const& n = g.nodes[s];
    if (n.constant || n.is_output || n.dtype != gdt_f16 || n.ne[0] % 8) return false;
    if (n.op == gop_pool_2d) return true;
    if (n.op == gop_interpolate) {
        if ((n.ip[2] & 255) == 0) return true; // nearest (a planar source read by one 3x3 conv never feeds a concat: nearest_into_reader)
        // bilinear | align_corners of a map in a buffer of its own (vx_bilinear_ac_pix_f16; encode_concat, birefnet.cpp:50-57). A 1 x 1 source is a broadcast: it stays
        // the launch it is (aspp_deformable's x5, birefnet.cpp:127-132)
        graph_node const& x = g.nodes[n.src[0]];
        return (n.ip[2] & 255) == 1 && (n.ip[2] & 256) && !x.constant && x.dtype == gdt_f16 && x.ne[1] * x.ne[2] > 1;
    }
    if (auto it = launch_of_last.find(s); it != launch_of_last.end()) return g.nodes[it->second].op == gop_conv_2d;
    if (n.op != gop_conv_2d || silu_convs.count(s) || rep_member.count(s) || is_conv3x3(n, g.nodes[n.src[1]])) return false;
    graph_node const& x = g.nodes[n.src[0]];
    if (x.op == gop_interpolate || x.op == gop_relu || x.dtype != gdt_f16 || (n.n_src == 3 && !g.nodes[n.src[2]].constant)) return false;
    for (int c : consumers[s])
        if (g.nodes[c].op != gop_concat && g.nodes[c].op != gop_conv_2d && g.nodes[c].op != gop_pool_2d && g.nodes[c].op != gop_slice) return false; // no epilogue
    return true;
}

void lowering::find_yolo_groups() {
    if (!g.fused_models) return;
    const int N = (int)g.nodes.size();
    for (int t = 0; t < N; ++t) { // (a), (b)
        silu_group G;
        if (!needed[t] || rep_member.count(t) || !match_silu_group(t, G)) continue;
        silu_convs[t] = G;
        if (G.rep1 >= 0) { rep_member[G.rep1] = t; skip[G.rep1] = 1; } // (wherever it stands in node order, the 3x3 conv's launch computes it)
        launch_of_last[G.add >= 0 ? G.add : G.silu] = t;
        claim(t, {G.rep1, G.rep_add, G.silu, G.add}); // (absorbed when the launch is emitted)
    }
    for (int t = 0; t < N; ++t) { // (e)
        dfl_group G;
        if (!needed[t] || !match_dfl_group(t, G)) continue;
        dfl_groups[t] = G;
        for (int c : G.absorbed) skip[c] = 1;
        claim(t, G.absorbed);
    }
    // (c): in node order, so that a slice of a slice sees its source's decision; readers that are slices themselves are looked at once every
    // candidate is known (a candidate whose reader fails is dropped, which may drop others: repeat until nothing changes)
    for (int t = 0; t < N; ++t)
        if (needed[t] && !skip[t] && channels_only(g.nodes[t])) chan_slice[t] = {g.nodes[t].src[0], (int)g.nodes[t].ip[0]};
    for (bool changed = true; changed;) {
        changed = false;
        for (auto it = chan_slice.begin(); it != chan_slice.end();) {
            if (!in_place_readers_ok(it->first, {})) { it = chan_slice.erase(it); changed = true; }
            else ++it;
        }
    }
    // (d)
    for (int t = 0; t < N; ++t) {
        graph_node const& n = g.nodes[t];
        if (!needed[t] || skip[t] || n.op != gop_concat || n.constant || n.ip[0] != 0 || n.dtype != gdt_f16) continue;
        auto interior = [&](int c) { // a concat that is the first operand of the next one and nothing else
            const int r = sole_consumer(c);
            return r >= 0 && g.nodes[r].op == gop_concat && g.nodes[r].ip[0] == 0 && g.nodes[r].src[0] == c;
        };
        if (interior(t)) continue;
        std::vector<int> chain = {t}, srcs;
        int cur = t;
        for (;;) {
            srcs.push_back(g.nodes[cur].src[1]);
            const int a = g.nodes[cur].src[0];
            if (g.nodes[a].op == gop_concat && !g.nodes[a].constant && g.nodes[a].ip[0] == 0 && interior(a) && !skip[a]) { chain.push_back(a); cur = a; continue; }
            srcs.push_back(a);
            break;
        }
        std::reverse(srcs.begin(), srcs.end());
        std::vector<cat_source> list;
        std::vector<std::pair<int, int>> slots; // (launch's last node, first channel)
        int at = 0;
        bool aligned = true, any = false;
        for (int s : srcs) {
            int v = s;
            while (g.nodes[v].op == gop_cont && !g.nodes[v].constant && sole_consumer(v) >= 0) v = g.nodes[v].src[0];
            list.push_back({v, at, false});
            aligned = aligned && at % 8 == 0 && g.nodes[v].ne[0] % 8 == 0 && g.nodes[v].dtype == gdt_f16;
            at += (int)g.nodes[v].ne[0];
        }
        if (!aligned) continue;
        for (size_t i = 0; i < list.size(); ++i) {
            const int v = list[i].node;
            if (cat_slot.count(v)) continue; // (a source of two concats is written into the first and copied into the second)
            if (auto cs = chan_slice.find(v); cs != chan_slice.end()) {
                // consecutive slices that together are the whole of one map: the map itself is written here
                const int m = cs->second.first;
                if (cs->second.second != 0 || cat_slot.count(m) || chan_slice.count(m) || !placeable_launch(m)) continue;
                size_t j = i;
                int64_t end = 0;
                while (j < list.size()) {
                    auto cj = chan_slice.find(list[j].node);
                    if (cj == chan_slice.end() || cj->second.first != m || cj->second.second != end) break;
                    end += g.nodes[list[j].node].ne[0];
                    ++j;
                }
                if (end != g.nodes[m].ne[0] || !in_place_readers_ok(m, chain)) continue;
                slots.emplace_back(m, list[i].c0);
                for (size_t q = i; q < j; ++q) list[q].placed = true;
                any = true;
                i = j - 1;
                continue;
            }
            // a LayerNorm read through one view by this concat alone (swin_encode's outputs in encode_concat, swin.cpp:262-264): its launch writes the slice
            if (const int ln = v == srcs[i] ? norm_behind(v) : -1; ln >= 0 && !cat_slot.count(ln) && std::find(chain.begin(), chain.end(), sole_consumer(v)) != chain.end()) {
                slots.emplace_back(ln, list[i].c0);
                list[i].placed = true;
                any = true;
                continue;
            }
            if (!placeable_launch(v) || !in_place_readers_ok(v, chain)) continue;
            bool twice = false; // the same map twice in one concat: the second one is copied
            for (auto const& sl : slots) twice = twice || sl.first == v;
            if (twice) continue;
            slots.emplace_back(v, list[i].c0);
            list[i].placed = true;
            any = true;
        }
        if (!any) continue; // the copy_op it is today
        cat_sources[t] = list;
        for (auto const& sl : slots) cat_slot[sl.first] = {t, sl.second};
        for (size_t i = 1; i < chain.size(); ++i) skip[chain[i]] = 1;
    }
}

bool lowering::lives_in_place(int t) const {
    for (int v = t;;) {
        if (in_place.count(v) || chan_slice.count(v)) return true;
        if (g.nodes[v].alias_of < 0) return false;
        v = g.nodes[v].alias_of;
    }
}
// Where the map t lies. Views (reshape, cont, absorbed nodes) are aliases of their source, so the walk may pass a reshape that changes ne[0]: a map with a
// buffer of its own is contiguous, and its pixels are as wide as the node ASKED FOR, not as the root. Inside a wider map only a view of the same width can be
// addressed; the matchers admit no other (a reshape is not among the readers they allow), and a walk that finds one refuses.
lowering::located lowering::locate(int t) {
    const int64_t width = g.nodes[t].ne[0];
    for (int v = t;;) {
        const bool placed_here = in_place.count(v) != 0, slice_here = chan_slice.count(v) != 0;
        if ((placed_here || slice_here) && g.nodes[v].ne[0] != width)
            throw except("graph: internal: tensor %d (%lld channels) is a reshaped view of tensor %d (%lld channels), which lives inside a wider map", t, (long long)width, v,
                         (long long)g.nodes[v].ne[0]);
        if (placed_here) return in_place.at(v);
        if (slice_here) {
            auto const& cs = chan_slice.at(v);
            located L = locate(cs.first);
            L.off += cs.second;
            return L;
        }
        if (g.nodes[v].alias_of < 0) return {buf_of(v), 0, width};
        v = g.nodes[v].alias_of;
    }
}
// where the launch of node t, whose last absorbed node is `last`, writes: its slice of a concat's buffer, or a buffer of its own
lowering::located lowering::output_slot(int t, int last) {
    graph_node& n = g.nodes[t];
    if (auto it = cat_slot.find(last); it != cat_slot.end()) {
        graph_node& cat = g.nodes[it->second.first];
        if (cat.buffer < 0) materialise(it->second.first);
        located L{cat.buffer, it->second.second, cat.ne[0]};
        in_place[t] = L;
        return L;
    }
    n.buffer = new_buffer(n.n_bytes(), n.is_output);
    return {n.buffer, 0, n.ne[0]};
}

bool lowering::yolo_takes(int t) const {
    if (!g.fused_models) return false;
    if (silu_convs.count(t) || cat_slot.count(t)) return true;
    graph_node const& n = g.nodes[t];
    return n.op == gop_conv_2d && lives_in_place(n.src[0]);
}

static std::string place_tag(const char* what, lowering::located const& L, int64_t width) {
    if (L.off == 0 && L.pix == width) return {};
    return std::string("[") + what + " ch " + std::to_string(L.off) + ".." + std::to_string(L.off + width) + " of " + std::to_string(L.pix) + "]";
}

// one launch of the GEMM family (implicit conv for every conv_2d, as csrc/yolov9t.cpp runs them; the plain product for linear) with the plain f16 or
// the SiLU epilogue, reading and writing through pixel strides
void lowering::yolo_product(int t) {
    graph_node& n = g.nodes[t];
    silu_group G;
    if (auto it = silu_convs.find(t); it != silu_convs.end()) G = it->second;
    const int xs = n.src[0];
    graph_node const& x = g.nodes[xs];
    const std::string who = weight_name(g, n);
    product P;
    auto& a = P.a;
    std::string kind;
    if (n.op == gop_linear) {
        pack_conv_rows(P, n, false);
        a.M = (int)(x.n_elements() / x.ne[0]);
        a.lda = P.p.K;
        P.in = {padded_rows(xs, P.p.k_real, P.p.K, a.M, who), 0, P.p.K};
        kind = "gemm";
    } else {
        graph_node const& w = g.nodes[n.src[1]];
        const bool image8_in = image8_input(x); // (the SiLU matcher admits the 3-channel image only; nothing else of f32 gets here)
        if (!image8_in && x.ne[0] % 8) throw except("conv_2d %s: Cin = %lld must be a multiple of 8", who.c_str(), (long long)x.ne[0]);
        pack_conv_rows(P, n, image8_in, G.rep1);
        P.in = image8_in ? located{image_pad8(xs), 0, 8} : locate(xs);
        a.M = (int)(n.ne[1] * n.ne[2] * n.ne[3]);
        conv_geometry(a, n, x, w);
        a.conv_pix = P.in.pix;
        kind = "conv" + std::to_string(a.conv_kw) + "x" + std::to_string(a.conv_kh) + (a.conv_stride > 1 ? "s" + std::to_string(a.conv_stride) : "") + (G.rep1 >= 0 ? "[+conv1x1 folded]" : "") +
               place_tag("in", P.in, a.conv_Cin);
    }
    absorb(std::vector<int>{G.rep1, G.rep_add, G.silu, G.add}, t); // the nodes this launch computes besides its own
    const int last = G.add >= 0 ? G.add : (G.silu >= 0 ? G.silu : t);
    if (G.res >= 0) {
        P.res1 = locate(G.res);
        a.ld_res1 = P.res1.pix;
    }
    P.out = output_slot(t, last);
    a.n_valid = (int)n.ne[0];
    a.ldo = P.out.pix;
    a.epi = G.silu >= 0 ? VX_EPI_SILU : VX_EPI_F16;
    char d[360];
    snprintf(d, sizeof d, "%s%s%s%s M=%d N=%d K=%d <- %s", kind.c_str(), G.silu >= 0 ? "[silu]" : "", G.res >= 0 ? "[+res]" : "", place_tag("out", P.out, n.ne[0]).c_str(), a.M, (int)n.ne[0],
             P.p.k_real, who.c_str());
    P.desc = d;
    P.group = n.op == gop_linear ? "gemm" : "conv";
    P.work(P.p.k_real + (G.res >= 0 ? (double)n.ne[0] : 0.0), (double)n.ne[0]);
    emit_product(P);
}

// ggml_pool_2d: one launch of kernels_pool.hip; with fused models it reads a channel slice where it lies and writes into its slice of a concat
void lowering::pool_2d(int t) {
    graph_node& n = g.nodes[t];
    graph_node const& x = g.nodes[n.src[0]];
    const int kind = (int)n.ip[0], k = (int)n.ip[1], stride = (int)n.ip[3], pad = (int)n.ip[5];
    const int B = (int)x.ne[3], H = (int)x.ne[2], W = (int)x.ne[1], C = (int)x.ne[0];
    const located in = g.fused_models ? locate(n.src[0]) : located{buf_of(n.src[0]), 0, C};
    const located out = g.fused_models ? output_slot(t, t) : (materialise(t), located{n.buffer, 0, C});
    char d[320];
    snprintf(d, sizeof d, "pool_%s%dx%d%s%s%s B=%d %dx%d -> %lldx%lld C=%d pad=%d", kind == 0 ? "max" : "avg", k, k, stride > 1 ? "s2" : "", place_tag("in", in, C).c_str(),
             place_tag("out", out, C).c_str(), B, W, H, (long long)n.ne[1], (long long)n.ne[2], C, pad);
    auto xp = ptr(in.buf), op = ptr(out.buf);
    const int64_t in_off = in.off, in_pix = in.pix, out_off = out.off, out_pix = out.pix;
    // (the hand schedule's vx_yolo_spp_f16 and vx_yolo_avgpool2_f16 were measured against this kernel and are not used: DESIGN.md section 17)
    emit(d, {in.buf}, {out.buf}, [=](void* st) { VX(vx_pool2d_f16(xp() + in_off * 2, in_pix, op() + out_off * 2, out_pix, B, H, W, C, kind, k, stride, pad, st)); });
    tag("pool", (double)n.n_elements() * k * k, (double)(x.n_elements() + n.n_elements()) * 2);
}

// ggml_upscale(NEAREST) that reads a map where it lies inside a wider one, or writes into its slice of a concat (yolov9t.cpp:560-569)
void lowering::nearest_in_place(int t) {
    graph_node& n = g.nodes[t];
    graph_node const& x = g.nodes[n.src[0]];
    const int B = (int)x.ne[3], H = (int)x.ne[2], W = (int)x.ne[1], C = (int)x.ne[0], OH = (int)n.ne[2], OW = (int)n.ne[1];
    const located in = locate(n.src[0]);
    const located out = output_slot(t, t);
    char d[256];
    snprintf(d, sizeof d, "nearest%s%s %dx%d -> %dx%d C=%d", place_tag("in", in, C).c_str(), place_tag("out", out, C).c_str(), W, H, OW, OH, C);
    auto xp = ptr(in.buf), op = ptr(out.buf);
    const int64_t in_off = in.off, in_pix = in.pix, out_off = out.off, out_pix = out.pix;
    emit(d, {in.buf}, {out.buf}, [=](void* st) { VX(vx_nearest_pix_f16(xp() + in_off * 2, in_pix, op() + out_off * 2, out_pix, B, H, W, C, OH, OW, st)); });
    tag("glue", 0, (double)(x.n_elements() + n.n_elements()) * 2);
}

// the top concat of a chain with placed sources: the buffer exists (its first placed producer made it); what could not be placed is copied into its slice
void lowering::concat_in_place(int t) {
    graph_node& n = g.nodes[t];
    if (n.buffer < 0) materialise(t);
    else if (n.is_output) g.buffers[n.buffer].persistent = true;
    const int obuf = n.buffer;
    auto op = ptr(obuf);
    const int64_t pixels = n.ne[1] * n.ne[2] * n.ne[3], width = n.ne[0];
    int part = 0;
    for (cat_source const& s : cat_sources.at(t)) {
        const int i = part++;
        if (s.placed) continue;
        graph_node const& x = g.nodes[s.node];
        const int64_t C = x.ne[0], off = s.c0;
        std::string d = "concat part " + std::to_string(i) + " " + shape_str(x.ne) + " -> " + shape_str(n.ne);
        if (x.constant) {
            void* cp = const_f16(s.node);
            emit(d + " (constant)", {}, {obuf}, [=](void* st) {
                const int64_t ne[4] = {C, pixels, 1, 1}, ss[4] = {1, C, 0, 0}, ds[4] = {1, width, 0, 0};
                VX(vx_copy_strided_f16(cp, op() + off * 2, ne, ss, ds, 1.0f, st));
            });
        } else {
            const located L = locate(s.node);
            auto xp = ptr(L.buf);
            const int64_t x_off = L.off, x_pix = L.pix;
            emit(d, {L.buf}, {obuf}, [=](void* st) {
                const int64_t ne[4] = {C, pixels, 1, 1}, ss[4] = {1, x_pix, 0, 0}, ds[4] = {1, width, 0, 0};
                VX(vx_copy_strided_f16(xp() + x_off * 2, op() + off * 2, ne, ss, ds, 1.0f, st));
            });
        }
        tag("glue", 0, (double)C * pixels * 4);
    }
}

// ggml_soft_max over dimension 0; as the tail of a DFL chain (with fused models) it never gets here
void lowering::soft_max(int t) {
    graph_node const& n = g.nodes[t];
    const int cols = (int)n.ne[0];
    const int64_t rows = n.n_elements() / cols;
    map_launch(t, "soft_max rows=" + std::to_string(rows) + " n=" + std::to_string(cols), [=](char* x, char* o, char*, void* st) { VX(vx_softmax_rows_f16(x, cols, o, cols, rows, cols, st)); });
    tag("softmax", (double)n.n_elements() * 4, (double)n.n_elements() * 4);
}

// ggml_sum_rows, or -- behind a matched DFL chain -- the softmax expectation of the box logits where they lie
void lowering::sum_rows(int t) {
    graph_node& n = g.nodes[t];
    auto it = dfl_groups.find(t);
    if (it == dfl_groups.end()) {
        graph_node const& x = g.nodes[n.src[0]];
        const int cols = (int)x.ne[0];
        const int64_t rows = n.n_elements();
        map_launch(t, "sum_rows rows=" + std::to_string(rows) + " n=" + std::to_string(cols), [=](char* xp, char* o, char*, void* st) { VX(vx_sum_rows_f16(xp, o, rows, cols, st)); });
        tag("softmax", (double)x.n_elements(), (double)x.n_elements() * 2);
        return;
    }
    dfl_group const& G = it->second;
    located in = locate(G.map);
    in.off += G.c0;
    const float* proj = const_f32(G.proj);
    const int64_t rows = n.n_elements() / G.groups;
    const int groups = G.groups, cols = G.n;
    materialise(t);
    const int obuf = n.buffer;
    auto xp = ptr(in.buf), op = ptr(obuf);
    const int64_t in_off = in.off, in_pix = in.pix;
    char d[200];
    snprintf(d, sizeof d, "softmax_expect rows=%lld groups=%d n=%d [in ch %lld..%lld of %lld]", (long long)rows, groups, cols, (long long)in_off, (long long)(in_off + groups * cols), (long long)in_pix);
    emit(d, {in.buf}, {obuf}, [=](void* st) { VX(vx_softmax_expect_f16(xp() + in_off * 2, in_pix, groups, proj, op(), rows, cols, st)); });
    tag("softmax", (double)rows * groups * cols * 4, (double)rows * groups * (cols + 1) * 2);
}

} // namespace visp
