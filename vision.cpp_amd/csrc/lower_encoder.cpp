// Graph lowering: attention, patch embedding and the DINOv2 encoder chain (see lowering.h).
#include "lowering.h"

#include <cmath>

namespace visp {

void lowering::patch_embed(int t) {
    graph_node& n = g.nodes[t];
    graph_node const& x = g.nodes[n.src[0]];
    const int ps = (int)n.ip[0], C = (int)x.ne[0], W = (int)x.ne[1], H = (int)x.ne[2], B = (int)x.ne[3];
    product P;
    pack_conv_rows(P, n, false);
    packed_operand const& p = P.p;
    const int64_t M = (int64_t)B * (H / ps) * (W / ps);
    const int xbuf = buf_of(n.src[0]), pbuf = new_buffer((size_t)M * p.K * 2);
    std::string who = n.name.empty() ? g.nodes[n.src[1]].name : n.name; // (not weight_name: the node's own name comes first here)
    auto xp = ptr(xbuf), pp = ptr(pbuf);
    const int Kp = p.K;
    emit("im2col_patches " + std::to_string(ps) + "x" + std::to_string(ps) + " M=" + std::to_string(M) + " <- " + who, {xbuf}, {pbuf},
         [=](void* st) { VX(vx_im2col_patches_f32(reinterpret_cast<const float*>(xp()), pp(), B, H, W, C, ps, Kp, st)); });
    if (n.ne[0] % 8) throw except("patch_embed %s: %lld output channels", who.c_str(), (long long)n.ne[0]);
    materialise(t);
    P.in.buf = pbuf;
    P.out.buf = n.buffer;
    P.a.lda = p.K; P.a.M = (int)M; P.a.n_valid = (int)n.ne[0]; P.a.ldo = n.ne[0]; P.a.epi = VX_EPI_F16;
    P.desc = "gemm M=" + std::to_string(M) + " N=" + std::to_string(n.ne[0]) + " K=" + std::to_string(p.k_real) + " <- " + who;
    emit_product(P); // (no timing group of its own)
}

// q, k, v of an attention that are views of three linears over ONE input, read by nothing else: the three products become one GEMM
// whose epilogue writes head-major q (scaled), k, v (dino.cpp:59-70 as one launch instead of three products + three permutes)
void lowering::find_qkv_groups() {
    for (int t = 0; t < (int)g.nodes.size(); ++t) {
        graph_node const& n = g.nodes[t];
        if (!needed[t] || n.op != gop_attention) continue;
        std::array<int, 3> lin{-1, -1, -1}, top{n.src[0], n.src[1], n.src[2]}; // top: where the walk down to the linear starts
        std::array<int, 2> ropes{-1, -1};
        bool ok = g.nodes[n.src[0]].ne[0] == 64 && g.nodes[n.src[0]].ne[2] == g.nodes[n.src[1]].ne[2];
        for (int i = 0; i < 3 && ok; ++i) {
            int v = n.src[i];
            // q or k through a rope_2d group (sam3.h:452-453): the group is read by this attention alone, and the view r it rotates by its two slices alone
            if (auto rg = rope2d_groups.find(v); i < 2 && rg != rope2d_groups.end()) {
                const int r = rg->second.src;
                ok = sole_consumer(v) == t && uses[r] == 2 && !g.nodes[r].is_output && g.nodes[r].op == gop_reshape;
                ropes[i] = v;
                top[i] = r;
                if (ok) v = g.nodes[r].src[0];
            }
            while (ok && (g.nodes[v].op == gop_reshape || g.nodes[v].op == gop_cont)) { // single-reader views only
                ok = uses[v] == 1 && !g.nodes[v].is_output;
                v = g.nodes[v].src[0];
            }
            ok = ok && g.nodes[v].op == gop_linear && uses[v] == 1 && !g.nodes[v].is_output;
            lin[i] = v;
        }
        ok = ok && lin[0] != lin[1] && lin[1] != lin[2] && lin[0] != lin[2];
        if (ok && (ropes[0] >= 0 || ropes[1] >= 0)) { // q and k rotated alike (one launch takes both), or the chain is left to its nodes
            ok = ropes[0] >= 0 && ropes[1] >= 0;
            if (ok) {
                auto const &A = rope2d_groups[ropes[0]], &K = rope2d_groups[ropes[1]];
                for (int h = 0; h < 2 && ok; ++h) {
                    graph_node const &a = g.nodes[A.rope[h]], &b = g.nodes[K.rope[h]];
                    ok = a.src[1] == b.src[1] && a.fp[0] == b.fp[0] && a.fp[1] == b.fp[1];
                }
            }
        }
        for (int i = 1; i < 3 && ok; ++i)
            ok = g.nodes[lin[i]].src[0] == g.nodes[lin[0]].src[0] && g.nodes[g.nodes[lin[i]].src[1]].ne[0] == g.nodes[g.nodes[lin[0]].src[1]].ne[0] &&
                 g.nodes[g.nodes[lin[i]].src[1]].ne[1] == g.nodes[g.nodes[lin[0]].src[1]].ne[1];
        ok = ok && g.nodes[g.nodes[lin[0]].src[1]].ne[0] % 64 == 0 && g.nodes[g.nodes[lin[0]].src[1]].ne[1] == g.nodes[n.src[0]].ne[0] * g.nodes[n.src[0]].ne[1];
        if (!ok) continue;
        qkv_lin[t] = lin;
        qkv_first[std::min({lin[0], lin[1], lin[2]})] = t;
        for (int i = 0; i < 3; ++i) { // the linears and their views are computed by the attention's q|k|v launch (fused_qkv, or the encoder chain's block launch)
            claim(t, {lin[i]});
            for (int v = top[i]; v != lin[i]; v = g.nodes[v].src[0]) claim(t, {v});
        }
        if (ropes[0] >= 0) qkv_rope[t] = ropes; // (their nodes stay claimed by the groups themselves)
    }
}
void lowering::fused_qkv(int att) {
    graph_node const& n = g.nodes[att];
    graph_node const& q = g.nodes[n.src[0]];
    const int64_t H = q.ne[1], T = q.ne[2], B = q.ne[3];
    auto const& lin = qkv_lin[att];
    product P;
    P.operand(pack_qkv(lin.data()));
    packed_operand const& p = P.p;
    const int xs = g.nodes[lin[0]].src[0];
    P.in.buf = buf_of(xs);
    std::array<int, 3>& hb = P.qkv;
    for (int i = 0; i < 3; ++i) hb[i] = new_buffer((size_t)(64 * H * T * B) * 2);
    for (size_t c = 0; c < claimed_by.size(); ++c) // the linears and their views, as find_qkv_groups claimed them, are computed by this launch
        if (claimed_by[c] == att) skip[c] = 1;
    auto& a = P.a;
    a.lda = p.K; a.M = (int)(B * T); a.n_valid = p.N;
    a.epi = VX_EPI_QKV;
    a.qkv_T = (int)T; a.qkv_H = (int)H;
    a.q_scale = n.fp[0] * 1.4426950408889634f; // the attention kernel works in the exp2 domain (VX_ATTN_Q_SCALE)
    char d[200];
    snprintf(d, sizeof d, "gemm[qkv heads-major] M=%d N=%d K=%d <- %s", a.M, p.N, p.k_real, g.nodes[g.nodes[lin[0]].src[1]].name.c_str());
    P.desc = d;
    P.group = "gemm_qkv";
    P.flops = 2.0 * a.M * (double)p.N * p.k_real;
    P.bytes = (double)a.M * (p.k_real + p.N) * 2; // (without the operand's image)
    emit_product(P);
    qkv_bufs[att] = hb;
    if (qkv_rope.count(att)) rope2d_in_place(att, hb);
}

// q, k, v of an attention node, [hd, H, T, B] -> head-major [hd, T, H, B] copies, q multiplied by q_scale on the way
std::array<int, 3> lowering::heads_major(graph_node const& n, float q_scale) {
    graph_node const& q = g.nodes[n.src[0]];
    const int64_t hd = q.ne[0], H = q.ne[1], T = q.ne[2], B = q.ne[3];
    std::array<int, 3> hb;
    for (int i = 0; i < 3; ++i) {
        const int sb = buf_of(n.src[i]);
        hb[i] = new_buffer((size_t)(hd * H * T * B) * 2);
        auto sp = ptr(sb), dp = ptr(hb[i]);
        const float s = i == 0 ? q_scale : 1.0f;
        emit(std::string("heads_major ") + "qkv"[i] + (i == 0 ? " (scaled)" : ""), {sb}, {hb[i]}, [=](void* st) {
            const int64_t ne[4] = {hd, T, H, B}, ss[4] = {1, H * hd, hd, T * H * hd}, ds[4] = {1, hd, T * hd, H * T * hd};
            VX(vx_copy_strided_f16(sp(), dp(), ne, ss, ds, s, st));
        });
    }
    return hb;
}

void lowering::attention(int t) {
    graph_node& n = g.nodes[t];
    graph_node const &q = g.nodes[n.src[0]], &k = g.nodes[n.src[1]];
    const int64_t hd = q.ne[0], H = q.ne[1], Tq = q.ne[2], Tk = k.ne[2], B = q.ne[3];
    if (hd != 64 || Tq != Tk) throw except("attention: head_dim %lld, %lld queries on %lld keys; the fused kernel is built for head_dim 64 self-attention", (long long)hd, (long long)Tq, (long long)Tk);
    const float q_scale = n.fp[0] * 1.4426950408889634f; // the kernel works in the exp2 domain (VX_ATTN_Q_SCALE)
    std::array<int, 3> hb;
    if (auto it = qkv_bufs.find(t); it != qkv_bufs.end()) hb = it->second;
    else hb = heads_major(n, q_scale);
    materialise(t);
    const int obuf = n.buffer;
    auto qp = ptr(hb[0]), kp = ptr(hb[1]), vp = ptr(hb[2]), op = ptr(obuf);
    char d[128];
    snprintf(d, sizeof d, "attention B=%lld heads=%lld T=%lld", (long long)B, (long long)H, (long long)Tq);
    emit(d, {hb[0], hb[1], hb[2]}, {obuf}, [=](void* st) { VX(vx_attention_f16(qp(), kp(), vp(), op(), (int)B, (int)H, (int)Tq, st)); });
    tag("attention", 4.0 * B * H * (double)Tq * Tq * 64, (double)B * H * Tq * 64 * 2 * 4);
}

// softmax(scale q k^T + mask) v at head_dim 32 / 64 (the window-attention families: swin.cpp:69-97). q, k, v head-major as above, the scale
// folded into q; a constant mask (bias table [+ shift mask], folded on the host) becomes one f16 device image [Bm][Hm][T_q][T_k] -- ggml's
// [T_k, T_q, Hm, Bm] is that layout already --, cut to its shortest period over the batch; an activation mask is read where it is, f16 or f32.
void lowering::attention_masked(int t) {
    if (auto it = window_groups.find(t); it != window_groups.end()) return window_attention(t, it->second);
    graph_node& n = g.nodes[t];
    graph_node const &q = g.nodes[n.src[0]], &mk = g.nodes[n.src[3]];
    const int64_t hd = q.ne[0], H = q.ne[1], T = q.ne[2], B = q.ne[3], Hm = mk.ne[2];
    int64_t Bm = mk.ne[3];
    const float q_scale = n.fp[0] * 1.4426950408889634f; // the kernel works in the exp2 domain
    // a constant mask that repeats over its batch (swin.cpp:83-88 repeats the layer's windows once per image) is kept once, the kernel's b % Bm does the
    // rest: at SWIN-T stage 0, 1024^2, batch 8 that is 20 MB per block on the device instead of 158 MB
    const int64_t image = mk.ne[0] * mk.ne[1] * mk.ne[2];
    if (mk.constant)
        for (int64_t p = 1; p < Bm; ++p)
            if (Bm % p == 0 && memcmp(mk.values(), mk.values() + p * image, (size_t)((Bm - p) * image) * 4) == 0) { Bm = p; break; }
    const std::array<int, 3> hb = heads_major(n, q_scale);
    std::vector<int> reads = {hb[0], hb[1], hb[2]};
    void* mconst = nullptr;
    std::function<char*()> mp;
    const int mask_f32 = !mk.constant && mk.dtype == gdt_f32;
    if (mk.constant)
        mconst = cached(n.src[3], role_f16, [&](bool st) {
            std::vector<uint16_t> h((size_t)(Bm * image));
            for (size_t i = 0; i < h.size(); ++i) h[i] = f32_to_f16(mk.values()[i]);
            return upload(h.data(), h.size() * 2, st);
        }, "images:" + std::to_string(Bm));
    else { reads.push_back(buf_of(n.src[3])); mp = ptr(buf_of(n.src[3])); }
    materialise(t);
    const int obuf = n.buffer;
    auto qp = ptr(hb[0]), kp = ptr(hb[1]), vp = ptr(hb[2]), op = ptr(obuf);
    char d[160];
    snprintf(d, sizeof d, "attention_masked B=%lld heads=%lld T=%lld hd=%lld mask=[%lld, %lld] %s", (long long)B, (long long)H, (long long)T, (long long)hd, (long long)Hm, (long long)Bm,
             mk.constant ? "(constant)" : (mask_f32 ? "f32" : "f16"));
    emit(d, reads, {obuf}, [=](void* st) {
        VX(vx_attention_masked_f16(qp(), kp(), vp(), mp ? static_cast<const void*>(mp()) : mconst, op(), (int)B, (int)H, (int)T, (int)hd, (int)Hm, (int)Bm, mask_f32, st));
    });
    tag("attention", 4.0 * B * H * (double)T * T * hd, (double)B * H * T * hd * 2 * 4 + (double)B * H * T * T * (mask_f32 ? 4 : 2));
}

// ---- the packed-bias window attention (mobile-sam.cpp:124-132) ---------------------------------------------------------------------------
// split_qkv(.., 1) leaves every token row of the q|k|v product as heads x (q | k | v) of 32 channels each -- the operand layout of
// vx_window_attention_f16 (kernels_winattn.hip). When the views between the product and the attention are read by nothing else, the attention runs on
// the product's rows where they are: two launches instead of permute, three slices, three heads_major copies and the masked attention. SWIN splits with
// split_dim 2 (its rows are q | k | v of ALL heads): its permute has other axes and does not match.
bool lowering::match_window_group(int att, window_group& G) const {
    graph_node const& n = g.nodes[att];
    if (n.op != gop_attention_masked) return false;
    graph_node const &q = g.nodes[n.src[0]], &mk = g.nodes[n.src[3]];
    const int64_t hd = q.ne[0], H = q.ne[1], T = q.ne[2], B = q.ne[3];
    if (hd != 32 || T > 256 || fabsf(n.fp[0] - 1.0f / sqrtf(32.0f)) > 1e-6f) return false; // (the kernel's own scale is 1 / sqrt(32))
    if (!mk.constant || mk.ne[0] != T || mk.ne[1] != T || mk.ne[2] != H || mk.ne[3] != 1) return false;
    int cn = -1;
    for (int i = 0; i < 3; ++i) {
        const int r = n.src[i];
        graph_node const& rn = g.nodes[r];
        if (rn.op != gop_reshape || rn.constant || sole_consumer(r) != att || rn.ne[0] != 32 || rn.ne[1] != H || rn.ne[2] != T || rn.ne[3] != B) return false;
        const int sl = rn.src[0];
        graph_node const& sn = g.nodes[sl];
        if (sn.op != gop_slice || sole_consumer(sl) != r) return false;
        graph_node const& c = g.nodes[sn.src[0]];
        // part i of the last dimension, everything of the others
        if (sn.ip[9] != i || sn.ne[3] != 1 || sn.ip[11] != 1 || sn.ip[0] != 0 || sn.ip[3] != 0 || sn.ip[6] != 0 || sn.ip[2] != 1 || sn.ip[5] != 1 || sn.ip[8] != 1 ||
            sn.ne[0] != c.ne[0] || sn.ne[1] != c.ne[1] || sn.ne[2] != c.ne[2])
            return false;
        if (i == 0) cn = sn.src[0];
        else if (sn.src[0] != cn) return false;
        G.views.push_back(r);
        G.views.push_back(sl);
    }
    graph_node const& c = g.nodes[cn];
    if (c.op != gop_cont || c.is_output || uses[cn] != 3 || c.ne[0] != 32 || c.ne[1] != H * T || c.ne[2] != B || c.ne[3] != 3) return false;
    const int pm = c.src[0];
    graph_node const& p = g.nodes[pm];
    if (p.op != gop_permute || sole_consumer(pm) != cn || p.ip[0] != 0 || p.ip[1] != 3 || p.ip[2] != 1 || p.ip[3] != 2) return false;
    const int r0 = p.src[0];
    graph_node const& r = g.nodes[r0];
    if (r.op != gop_reshape || sole_consumer(r0) != pm || r.ne[0] != 32 || r.ne[1] != 3 || r.ne[2] != H * T || r.ne[3] != B) return false;
    const int lin = r.src[0];
    graph_node const& l = g.nodes[lin];
    if (l.op != gop_linear || l.constant || sole_consumer(lin) != r0 || l.ne[0] != 96 * H || l.ne[1] != T || l.ne[2] != B || l.ne[3] != 1) return false;
    G.lin = lin;
    for (int v : {cn, pm, r0}) G.views.push_back(v);
    return true;
}
// before the node loop: the views come before their attention in node order and must not be lowered on their own
void lowering::find_window_groups() {
    if (!g.fused_models) return;
    for (int t = 0; t < (int)g.nodes.size(); ++t) {
        window_group G;
        if (!needed[t] || !match_window_group(t, G)) continue;
        for (int v : G.views) skip[v] = 1;
        claim(t, G.views);
        window_groups[t] = std::move(G);
    }
}
void lowering::window_attention(int t, window_group const& G) {
    graph_node& n = g.nodes[t];
    graph_node const &q = g.nodes[n.src[0]], &mk = g.nodes[n.src[3]];
    const int H = (int)q.ne[1], T = (int)q.ne[2], B = (int)q.ne[3];
    void* bias = cached(n.src[3], role_winattn_bias, [&](bool st) {
        std::vector<char> h(vx_window_attention_bias_bytes(T, H));
        VX(vx_window_attention_pack_bias(mk.values(), T, H, h.data())); // ggml's [T_k, T_q, heads, 1] is [heads][T_q][T_k] in memory
        return upload(h.data(), h.size(), st);
    });
    const int qbuf = buf_of(G.lin);
    materialise(t);
    const int obuf = n.buffer;
    auto qp = ptr(qbuf), op = ptr(obuf);
    graph_node const& w = g.nodes[g.nodes[G.lin].src[1]];
    char d[240];
    snprintf(d, sizeof d, "window_attention windows=%d heads=%d T=%d hd=32 <- %s", B, H, T, w.name.c_str());
    emit(d, {qbuf}, {obuf}, [=](void* st) { VX(vx_window_attention_f16(qp(), bias, op(), B, T, H, st)); });
    tag("attention", 4.0 * B * H * (double)T * T * 32, (double)B * H * T * 32 * 2 * 4 + (double)H * T * T * 2);
}

// ---- fused model group 1: the DINOv2 encoder (dino.cpp:10-110) -----------------------------------------------------------------------
// prepare_tokens (patch_embed -> reshape -> concat with the cls constant -> + position constant) followed by a chain of dino::layer
// groups  x -> LN1 -> q|k|v -> attention -> out-proj * lambda1 + x -> LN2 -> fc1 -> gelu -> fc2 * lambda2 + x1 [-> final LN taps]
// at the block kernel's widths (384 / 1536 / heads of 64) lowers to what csrc/kernels_block16.hip was written for: the residual stream
// as ONE f32 buffer, per layer one attention launch and one token-stationary block launch (out-proj .. fc2 of layer i, the taps' final
// LayerNorm, LN1 + QKV of layer i + 1), the first layer's LN1 + QKV as the kernel's QKV-only instance. Every interior node must be
// read inside the group only; the token tensor and the layer outputs may be graph outputs (they are copied out of the stream as f32).
bool lowering::match_layer(int att, enc_layer& L) const {
    auto it = qkv_lin.find(att);
    if (it == qkv_lin.end() || qkv_rope.count(att)) return false; // (the block kernel has no rotation in front of its attention)
    for (int i = 0; i < 3; ++i) L.lin[i] = it->second[i];
    L.att = att;
    L.ln1 = g.nodes[L.lin[0]].src[0];
    graph_node const& ln1 = g.nodes[L.ln1];
    if (ln1.op != gop_layer_norm || uses[L.ln1] != 3 || ln1.is_output || ln1.ne[0] != 384) return false;
    if (g.nodes[att].ne[0] != 384 || g.nodes[att].is_output) return false;
    auto sole = [&](int t, int op) { const int c = sole_consumer(t); return c >= 0 && g.nodes[c].op == op ? c : -1; };
    auto scaled = [&](int t, int& lam) { // mul by a 384-element constant behind t
        const int c = sole(t, gop_mul);
        if (c < 0 || root(g.nodes[c].src[0]) != t || !g.nodes[g.nodes[c].src[1]].constant || g.nodes[g.nodes[c].src[1]].n_elements() != 384) return -1;
        lam = g.nodes[c].src[1];
        return c;
    };
    auto residual = [&](int t, int x) { // add(x, t), either order
        const int c = sole(t, gop_add);
        if (c < 0) return -1;
        const int a = g.nodes[c].src[0], b = g.nodes[c].src[1];
        return ((a == x && b == t) || (a == t && b == x)) ? c : -1;
    };
    const int x = ln1.src[0];
    if ((L.o = sole(att, gop_linear)) < 0 || g.nodes[L.o].src[0] != att || g.nodes[L.o].ne[0] != 384) return false;
    if ((L.s1 = scaled(L.o, L.lam1)) < 0 || (L.x1 = residual(L.s1, x)) < 0) return false;
    if (uses[L.x1] != 2 || g.nodes[L.x1].is_output) return false;
    for (int c : consumers[L.x1])
        if (g.nodes[c].op == gop_layer_norm && g.nodes[c].src[0] == L.x1) L.ln2 = c;
    if (L.ln2 < 0 || g.nodes[L.ln2].is_output || g.nodes[L.ln2].fp[0] != ln1.fp[0]) return false;
    if ((L.f1 = sole(L.ln2, gop_linear)) < 0 || g.nodes[L.f1].ne[0] != 1536 || (L.ge = sole(L.f1, gop_gelu)) < 0) return false;
    if ((L.f2 = sole(L.ge, gop_linear)) < 0 || g.nodes[L.f2].ne[0] != 384) return false;
    if ((L.s2 = scaled(L.f2, L.lam2)) < 0 || (L.x2 = residual(L.s2, L.x1)) < 0) return false;
    for (int t : {L.o, L.s1, L.f1, L.ge, L.f2, L.s2})
        if (g.nodes[t].is_output) return false;
    return true;
}
void lowering::find_encoder_chain() {
    auto through_views = [&](int v, std::vector<int>* seen) { // the producer behind single-reader reshape / cont views
        while (g.nodes[v].op == gop_reshape || g.nodes[v].op == gop_cont) {
            if (uses[v] != 1 || g.nodes[v].is_output) return -1;
            seen->push_back(v);
            v = g.nodes[v].src[0];
        }
        return v;
    };
    if (!g.fused_models || !vx_dino_block_supported(384, 1536, 64)) return;
    std::vector<enc_layer> found;
    for (auto const& kv : qkv_lin) { // std::map: attention nodes in node order = layer order
        enc_layer L;
        if (match_layer(kv.first, L)) found.push_back(L);
    }
    if (found.empty()) return;
    // a chain: layer l + 1 normalises what layer l produced; x2's other readers are the final-LayerNorm taps
    std::vector<enc_layer> chain;
    for (auto& L : found) {
        const int x = g.nodes[L.ln1].src[0];
        if (!chain.empty() && x != chain.back().x2) return; // two encoders / a branch: not this pattern
        chain.push_back(L);
    }
    for (size_t l = 0; l < chain.size(); ++l) {
        enc_layer& L = chain[l];
        int known = 0;
        for (int c : consumers[L.x2]) {
            if (l + 1 < chain.size() && (c == chain[l + 1].ln1 || c == chain[l + 1].x1)) { ++known; continue; }
            if (g.nodes[c].op == gop_layer_norm && g.nodes[c].src[0] == L.x2) { L.taps.push_back(c); ++known; continue; }
            return;
        }
        if (known != uses[L.x2]) return;
    }
    int tap_w = -1, tap_b = -1;
    float eps = g.nodes[chain[0].ln1].fp[0];
    for (auto& L : chain) {
        if (g.nodes[L.ln1].fp[0] != eps) return;
        if (g.nodes[L.att].fp[0] != g.nodes[chain[0].att].fp[0]) return; // the block launches take one q scale for the whole chain
        for (int t : L.taps) {
            if (tap_w < 0) { tap_w = g.nodes[t].src[1]; tap_b = g.nodes[t].src[2]; }
            if (g.nodes[t].src[1] != tap_w || g.nodes[t].src[2] != tap_b || g.nodes[t].fp[0] != eps) return; // one shared final LayerNorm
        }
    }
    // prepare_tokens in front of the first layer
    enc_chain e;
    e.tok = g.nodes[chain[0].ln1].src[0];
    graph_node const& tok = g.nodes[e.tok];
    if (tok.op != gop_add || uses[e.tok] != 2 || !g.nodes[tok.src[1]].constant) return;
    e.pos = tok.src[1];
    e.cat = tok.src[0];
    graph_node const& cat = g.nodes[e.cat];
    const int64_t D = tok.ne[0], T = tok.ne[1], B = tok.ne[2];
    if (cat.op != gop_concat || cat.ip[0] != 1 || sole_consumer(e.cat) != e.tok || g.nodes[e.pos].n_elements() != D * T || tok.ne[3] != 1) return;
    if (!g.nodes[cat.src[0]].constant || g.nodes[cat.src[0]].ne[1] != 1) return;
    e.cls = cat.src[0];
    if (sole_consumer(cat.src[1]) != e.cat) return;
    e.pe = through_views(cat.src[1], &e.views);
    if (e.pe < 0 || g.nodes[e.pe].op != gop_patch_embed || uses[e.pe] != 1 || g.nodes[e.pe].is_output) return;
    graph_node const& pe = g.nodes[e.pe];
    if (pe.ne[0] != D || pe.ne[1] * pe.ne[2] + 1 != T || pe.ne[3] != B) return;
    e.img = pe.src[0];
    if (g.nodes[e.img].op == gop_image_u8_to_f32 && sole_consumer(e.img) == e.pe) { e.u8 = g.nodes[e.img].src[0]; }
    e.layers = std::move(chain);
    e.first = e.u8 >= 0 ? e.img : e.pe;
    e.ok = true;
    enc = std::move(e);
    for (auto const& L : enc.layers) qkv_first.erase(std::min({L.lin[0], L.lin[1], L.lin[2]})); // these attentions are not lowered one by one
}

static void put(std::vector<float>& v, const float* src, size_t n) { // n floats (zeros if the tensor is absent)
    if (src) v.insert(v.end(), src, src + n); else v.insert(v.end(), n, 0.0f);
}

void lowering::emit_encoder() {
    auto values_or_null = [&](int t) -> const float* { return t >= 0 ? g.nodes[t].values() : nullptr; };
    auto wname = [&](int t) { return const_id(g, t); };
    enc_chain const& e = enc;
    graph_node const& tok = g.nodes[e.tok];
    graph_node const& pe = g.nodes[e.pe];
    const int D = 384, HID = 1536, NH = 6;
    const int T = (int)tok.ne[1], B = (int)tok.ne[2], Pn = T - 1;
    const long M = (long)B * T, MP = (long)B * Pn;
    const int ps = (int)pe.ip[0], Wimg = (int)g.nodes[e.img].ne[1], Himg = (int)g.nodes[e.img].ne[2];
    const float eps = g.nodes[enc.layers[0].ln1].fp[0];
    auto bias_of = [&](int lin) { return g.nodes[lin].n_src == 3 ? g.nodes[lin].src[2] : -1; };
    std::vector<int> all = {e.pe, e.cat, e.tok};
    if (e.u8 >= 0) all.push_back(e.img);
    all.insert(all.end(), e.views.begin(), e.views.end());

    // ---- tokens: patches (u8 -> f16 with the normalisation folded in, or from the f32 image), cls rows, patch GEMM whose epilogue adds
    // bias + position embedding and writes f32 token rows
    product tokens;
    pack_conv_rows(tokens, pe, false); // (pe.ne[0] == D: find_encoder_chain)
    packed_operand const& p = tokens.p;
    const int Kp = p.K;
    const int pbuf = new_buffer((size_t)MP * Kp * 2), xbuf = new_buffer((size_t)M * D * 4);
    auto pp = ptr(pbuf), xp = ptr(xbuf);
    if (e.u8 >= 0) {
        const int ibuf = buf_of(e.u8);
        auto ip = ptr(ibuf);
        graph_node const& im = g.nodes[e.img];
        std::array<float, 3> mean{im.fp[0], im.fp[1], im.fp[2]}, istd{im.fp[3], im.fp[4], im.fp[5]};
        emit("preprocess_patches " + std::to_string(ps) + "x" + std::to_string(ps) + " M=" + std::to_string(MP), {ibuf}, {pbuf}, [=](void* st) {
            VX(vx_preprocess_patches(reinterpret_cast<const uint8_t*>(ip()), pp(), B, Himg, Wimg, ps, Kp, mean.data(), istd.data(), st));
        });
        tag("preprocess", 0, (double)B * Himg * Wimg * 3 + (double)MP * Kp * 2);
    } else {
        const int ibuf = buf_of(e.img);
        auto ip = ptr(ibuf);
        const int C = (int)g.nodes[e.img].ne[0];
        emit("im2col_patches " + std::to_string(ps) + "x" + std::to_string(ps) + " M=" + std::to_string(MP), {ibuf}, {pbuf},
             [=](void* st) { VX(vx_im2col_patches_f32(reinterpret_cast<const float*>(ip()), pp(), B, Himg, Wimg, C, ps, Kp, st)); });
        tag("preprocess", 0, (double)B * Himg * Wimg * C * 4 + (double)MP * Kp * 2);
    }
    const float* cls = const_f32(e.cls);
    const float* pos = const_f32(e.pos);
    emit("cls_rows B=" + std::to_string(B), {}, {xbuf}, [=](void* st) { VX(vx_write_cls_rows(reinterpret_cast<float*>(xp()), cls, pos, B, T, D, st)); });
    tag("preprocess");
    {
        auto& a = tokens.a;
        a.lda = Kp; a.M = (int)MP; a.n_valid = D;
        a.epi = VX_EPI_TOKENS; a.ldo = D; a.pos = pos; a.tokens_P = Pn;
        tokens.in.buf = pbuf;
        tokens.out.buf = xbuf;
        tokens.desc = "gemm[tokens f32: + bias + pos] M=" + std::to_string(MP) + " N=384 K=" + std::to_string(p.k_real) + " <- " + g.nodes[pe.src[1]].name;
        tokens.group = "patch_embed";
        tokens.flops = 2.0 * MP * D * p.k_real;
        tokens.bytes = (double)MP * Kp * 2 + (double)M * D * 4;
        emit_product(tokens);
    }
    auto copy_out = [&](int node, const char* what) { // a graph output inside the group: the residual stream as it stands, f32
        graph_node& n = g.nodes[node];
        n.dtype = gdt_f32;
        materialise(node);
        const int ob = n.buffer;
        auto op = ptr(ob);
        const size_t bytes = (size_t)M * D * 4;
        emit(std::string("copy_f32 ") + what, {xbuf}, {ob}, [=](void* st) { VX(vx_memcpy_d2d(op(), xp(), bytes, st)); });
        tag("capture");
    };
    if (tok.is_output) copy_out(e.tok, "tokens");

    // ---- per layer: attention + one block launch
    const int qb = new_buffer((size_t)M * D * 2), kb = new_buffer((size_t)M * D * 2), vb = new_buffer((size_t)M * D * 2), ab = new_buffer((size_t)M * D * 2);
    auto qp = ptr(qb), kp = ptr(kb), vp = ptr(vb), ap = ptr(ab);
    const float q_scale = g.nodes[enc.layers[0].att].fp[0] * 1.4426950408889634f; // the attention kernel works in the exp2 domain
    auto pack_mlp = [&](enc_layer const& L) -> void* {
        const int wo = g.nodes[L.o].src[1], w1 = g.nodes[L.f1].src[1], w2 = g.nodes[L.f2].src[1];
        return cached(wo, role_block_mlp, [&](bool st) {
            // LayerScale folded into the two residual products (W' = f16(lambda[n] * W[n, :])): the residual stream stays in the accumulators
            std::vector<uint16_t> a((size_t)D * D), b((size_t)HID * D), c((size_t)D * HID), out(vx_dino_block_mlp_bytes() / 2);
            const float *ho = g.nodes[wo].values(), *h1 = g.nodes[w1].values(), *h2 = g.nodes[w2].values(), *l1 = g.nodes[L.lam1].values(), *l2 = g.nodes[L.lam2].values();
            for (int n = 0; n < D; ++n) {
                for (int k = 0; k < D; ++k) a[(size_t)n * D + k] = f32_to_f16(f16_to_f32(f32_to_f16(ho[(size_t)n * D + k])) * l1[n]);
                for (int k = 0; k < HID; ++k) c[(size_t)n * HID + k] = f32_to_f16(f16_to_f32(f32_to_f16(h2[(size_t)n * HID + k])) * l2[n]);
            }
            for (size_t i = 0; i < b.size(); ++i) b[i] = f32_to_f16(h1[i]);
            VX(vx_dino_block16_pack_mlp(a.data(), b.data(), c.data(), out.data()));
            return upload(out.data(), out.size() * 2, st);
        }, wname(w1) + "|" + wname(w2) + "|*" + wname(L.lam1) + "|*" + wname(L.lam2));
    };
    auto pack_qkv_block = [&](enc_layer const& L) -> void* {
        return cached(g.nodes[L.lin[0]].src[1], role_block_qkv, [&](bool st) {
            std::vector<uint16_t> rows((size_t)3 * D * D), out(vx_dino_block_qkv_bytes() / 2);
            for (int i = 0; i < 3; ++i) {
                const float* h = g.nodes[g.nodes[L.lin[i]].src[1]].values();
                for (size_t j = 0; j < (size_t)D * D; ++j) rows[(size_t)i * D * D + j] = f32_to_f16(h[j]);
            }
            VX(vx_dino_block16_pack_qkv(rows.data(), out.data()));
            return upload(out.data(), out.size() * 2, st);
        }, wname(g.nodes[L.lin[1]].src[1]) + "|" + wname(g.nodes[L.lin[2]].src[1]));
    };
    auto vec_mlp = [&](enc_layer const& L) {
        const int bo = bias_of(L.o), b1 = bias_of(L.f1), b2 = bias_of(L.f2);
        return vec_cached(g.nodes[L.o].src[1], role_block_mlp_vec, wname(bo) + "|" + wname(b1) + "|" + wname(b2) + "|" + wname(g.nodes[L.ln2].src[1]) + "|*" + wname(L.lam1) + "|*" + wname(L.lam2), [&]() {
            std::vector<float> v;
            const float *l1 = g.nodes[L.lam1].values(), *l2 = g.nodes[L.lam2].values();
            put(v, values_or_null(bo), D);
            for (int n = 0; n < D; ++n) v[n] *= l1[n];
            put(v, l1, D);
            put(v, g.nodes[g.nodes[L.ln2].src[1]].values(), D);
            put(v, g.nodes[g.nodes[L.ln2].src[2]].values(), D);
            put(v, values_or_null(b1), HID);
            const size_t at = v.size();
            put(v, values_or_null(b2), D);
            for (int n = 0; n < D; ++n) v[at + n] *= l2[n];
            put(v, l2, D);
            return v;
        });
    };
    auto vec_qkv = [&](enc_layer const& L) {
        return vec_cached(g.nodes[L.ln1].src[1], role_block_qkv_vec, wname(g.nodes[L.ln1].src[2]) + "|" + wname(bias_of(L.lin[0])) + "|" + wname(bias_of(L.lin[1])) + "|" + wname(bias_of(L.lin[2])), [&]() {
            std::vector<float> v;
            put(v, g.nodes[g.nodes[L.ln1].src[1]].values(), D);
            put(v, g.nodes[g.nodes[L.ln1].src[2]].values(), D);
            for (int i = 0; i < 3; ++i) put(v, values_or_null(bias_of(L.lin[i])), D);
            return v;
        });
    };
    float* vec_tap = nullptr;
    for (auto const& L : enc.layers)
        if (!L.taps.empty() && !vec_tap) {
            const int t = L.taps[0];
            vec_tap = vec_cached(g.nodes[t].src[1], role_tap_vec, wname(g.nodes[t].src[2]), [&]() {
                std::vector<float> v;
                put(v, g.nodes[g.nodes[t].src[1]].values(), D);
                put(v, g.nodes[g.nodes[t].src[2]].values(), D);
                return v;
            });
        }
    auto block = [&](const enc_layer* mlp, const enc_layer* qkv, int feat_buf, const char* group, std::string const& who) {
        vx_dino_block_args a;
        memset(&a, 0, sizeof a);
        a.M = (int)M; a.T = T; a.H = NH; a.q_scale = q_scale; a.eps = eps;
        double flops = 0, bytes = (double)M * D * 4;
        std::vector<int> reads = {xbuf}, writes = {xbuf};
        if (mlp) {
            a.w_mlp = pack_mlp(*mlp); a.vec_mlp = vec_mlp(*mlp);
            flops += 2.0 * M * D * (D + 2.0 * HID);
            bytes += (double)M * D * (2 + 4);
            reads.push_back(ab);
        }
        if (qkv) {
            a.w_qkv = pack_qkv_block(*qkv); a.vec_qkv = vec_qkv(*qkv);
            flops += 2.0 * M * D * 3.0 * D;
            bytes += (double)M * D * 2 * 3;
            writes.insert(writes.end(), {qb, kb, vb});
        }
        std::function<char*()> fp;
        if (feat_buf >= 0) { a.vec_tap = vec_tap; fp = ptr(feat_buf); bytes += (double)M * D * 2; writes.push_back(feat_buf); }
        const bool has_mlp = mlp != nullptr, has_qkv = qkv != nullptr;
        emit(std::string("dino_block[") + (has_mlp ? "out-proj + mlp" : "") + (feat_buf >= 0 ? " + tap" : "") + (has_qkv ? (has_mlp ? " + next ln1 + qkv" : "ln1 + qkv") : "") + "] M=" + std::to_string(M) + " <- " + who,
             reads, writes, [=](void* st) {
                 vx_dino_block_args r = a;
                 r.x = reinterpret_cast<float*>(xp());
                 if (has_mlp) r.att = ap();
                 if (has_qkv) { r.q = qp(); r.k = kp(); r.v = vp(); }
                 if (fp) r.feat = fp();
                 VX(vx_dino_block16_f16(&r, st));
             });
        tag(group, flops, bytes);
    };
    block(nullptr, &enc.layers[0], -1, "block_qkv0", g.nodes[g.nodes[enc.layers[0].lin[0]].src[1]].name);
    for (size_t l = 0; l < enc.layers.size(); ++l) {
        enc_layer const& L = enc.layers[l];
        emit("attention B=" + std::to_string(B) + " heads=" + std::to_string(NH) + " T=" + std::to_string(T), {qb, kb, vb}, {ab},
             [=](void* st) { VX(vx_attention_f16(qp(), kp(), vp(), ap(), B, NH, T, st)); });
        tag("attention", 4.0 * B * NH * (double)T * T * 64, (double)M * D * 2 * 4);
        int feat = -1;
        for (int t : L.taps) {
            materialise(t);
            if (feat < 0) feat = g.nodes[t].buffer;
        }
        block(&L, l + 1 < enc.layers.size() ? &enc.layers[l + 1] : nullptr, feat, "block", g.nodes[g.nodes[L.o].src[1]].name);
        for (size_t i = 1; i < L.taps.size(); ++i) { // further taps that name this layer: the same rows
            const int ob = g.nodes[L.taps[i]].buffer;
            auto fp = ptr(feat), op = ptr(ob);
            const size_t bytes = (size_t)M * D * 2;
            emit("copy tap", {feat}, {ob}, [=](void* st) { VX(vx_memcpy_d2d(op(), fp(), bytes, st)); });
            tag("block");
        }
        if (g.nodes[L.x2].is_output) copy_out(L.x2, "layer output");
        for (int t : {L.ln1, L.lin[0], L.lin[1], L.lin[2], L.att, L.o, L.s1, L.x1, L.ln2, L.f1, L.ge, L.f2, L.s2, L.x2}) all.push_back(t);
        for (int i = 0; i < 3; ++i)
            for (int v = g.nodes[L.att].src[i]; v != L.lin[i]; v = g.nodes[v].src[0]) all.push_back(v);
        for (int t : L.taps) all.push_back(t);
    }
    for (int t : all) skip[t] = 1;
}

} // namespace visp
