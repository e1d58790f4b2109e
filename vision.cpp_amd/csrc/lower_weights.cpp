// Graph lowering: device images of weights and constants (see lowering.h).
#include "lowering.h"

namespace visp {

std::string weight_name(graph const& g, graph_node const& n) {
    graph_node const& w = g.nodes[n.src[1]];
    return w.op == gop_weight && !w.name.empty() ? w.name : n.name;
}
std::string const_id(graph const& g, int t) {
    if (t < 0) return "-";
    return g.nodes[t].op == gop_weight && !g.nodes[t].name.empty() ? g.nodes[t].name : "#" + std::to_string(t);
}

// device image of constant t in `role`: model weights are cached in the weight store (shared by every graph over the model),
// constants folded inside this graph belong to the graph
// `with`: names of the other weights a derived image was made from (a folded LayerScale vector, the k and v parts of a fused
// q|k|v operand) -- part of its identity
void* lowering::cached(int t, pack_role role, std::function<void*(bool)> make, std::string const& with) {
    auto key = std::make_pair(std::make_pair(t, (int)role), with);
    auto it = const_cache.find(key);
    if (it != const_cache.end()) return it->second;
    graph_node const& n = g.nodes[t];
    void* d = nullptr;
    // only images made from NAMED model weights alone are shared: a derived image whose other operand is a constant folded inside this
    // graph ("#<node>": a node index means nothing to another graph) stays with the graph
    const bool shareable = n.op == gop_weight && with.find('#') == std::string::npos;
    if (shareable && !g.dev) d = make(true); // planning: upload() only counts what the store would take
    else if (shareable) {
        auto skey = std::make_pair(with.empty() ? n.name : n.name + "|" + with, (int)role);
        std::lock_guard<std::mutex> lock(g.store->mutex); // graphs over one store may be allocated from several threads
        auto sit = g.store->packs.find(skey);
        if (sit != g.store->packs.end()) d = sit->second; // uploaded by an earlier graph over the same weights
        else { d = make(true); g.store->packs[skey] = d; }
    } else d = make(false);
    const_cache[key] = d;
    return d;
}
void* lowering::upload(const void* host, size_t bytes, bool to_store) {
    g.const_bytes += bytes;
    if (!g.dev) {
        if (to_store) g.plan_store_bytes += round_up<size_t>(bytes + 256, 256);
        return nullptr;
    }
    void* d = nullptr;
    weight_store& ws = *g.store;
    if (to_store && ws.arena.ptr && ws.arena_used + round_up<size_t>(bytes + 256, 256) <= ws.arena.bytes) { // the model's one arena, in lowering order
        d = static_cast<char*>(ws.arena.ptr) + ws.arena_used;
        ws.arena_used += round_up<size_t>(bytes + 256, 256);
        ws.device_bytes += bytes;
    } else {
        if (to_store && ws.no_data) throw except("graph: this rank holds no weight data (the arena came by broadcast) and the image it needs is not part of the arena");
        device_buffer b(bytes + 256);
        d = b.ptr;
        if (to_store) { ws.allocs.push_back(std::move(b)); ws.device_bytes += bytes; }
        else g.const_allocs.push_back(std::move(b));
    }
    if (to_store && ws.no_data) return d; // laid out, filled by the broadcast
    VX(vx_memcpy_h2d(d, host, bytes, g.dev->stream));
    VX(vx_stream_sync(g.dev->stream)); // the host image is a temporary
    return d;
}
float* lowering::const_f32(int t) {
    return static_cast<float*>(cached(t, role_f32, [&](bool st) { return upload(g.nodes[t].values(), (size_t)g.nodes[t].n_elements() * 4, st); }));
}
void* lowering::const_f16(int t) {
    return cached(t, role_f16, [&](bool st) {
        std::vector<uint16_t> h((size_t)g.nodes[t].n_elements());
        for (size_t i = 0; i < h.size(); ++i) h[i] = f32_to_f16(g.nodes[t].values()[i]);
        return upload(h.data(), h.size() * 2, st);
    });
}
// rows [n][k] -> f16 [N pad][K pad 64] + f32 bias [N pad] (bias of `period` elements repeated)
packed_operand lowering::pack_matrix(int wt, pack_role role, int n, int k, std::function<float(int, int)> at, int bias_t, int bias_period, int scale_t) {
    packed_operand p;
    // LayerScale folded into the operand: W' = f16(lambda[n] * W[n, :]), b' = lambda[n] * b[n] (what csrc/depthany.cpp does for the
    // block kernel: the product's epilogue can then take the residual)
    const float* lam = scale_t >= 0 ? g.nodes[scale_t].values() : nullptr;
    const std::string with = scale_t >= 0 ? "*" + const_id(g, scale_t) : std::string();
    p.n_real = n; p.k_real = k;
    p.N = round_up(n, n > 64 ? 64 : 32);
    p.K = round_up(k, 64);
    p.w = cached(wt, role, [&](bool st) {
        std::vector<uint16_t> h((size_t)p.N * p.K, 0);
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < k; ++c) h[(size_t)r * p.K + c] = f32_to_f16(lam ? lam[r] * at(r, c) : at(r, c));
        return upload(h.data(), h.size() * 2, st);
    }, with);
    if (bias_t >= 0)
        p.bias = static_cast<float*>(cached(bias_t, bias_of_role(role), [&](bool st) {
            std::vector<float> b((size_t)p.N, 0.0f);
            for (int r = 0; r < n; ++r) b[r] = g.nodes[bias_t].values()[r % bias_period] * (lam ? lam[r] : 1.0f);
            return upload(b.data(), b.size() * 4, st);
        }, with));
    return p;
}
packed_operand lowering::pack_rows(int wt, int bias_t, int n, int scale_t) { // linear [K, N] and conv [Cin, kw, kh, Cout]: the n rows of the host image as they are
    graph_node const& w = g.nodes[wt];
    const int k = (int)(w.n_elements() / n);
    const float* h = w.values();
    return pack_matrix(wt, role_rows, n, k, [h, k](int r, int c) { return h[(size_t)r * k + c]; }, bias_t, n, scale_t);
}
// q | k | v rows of three linears over the same input as one operand (N = 3 * heads * 64), for the head-major epilogue
packed_operand lowering::pack_qkv(const int lin[3]) {
    graph_node const* w[3];
    int bias[3];
    std::string with;
    for (int i = 0; i < 3; ++i) {
        w[i] = &g.nodes[g.nodes[lin[i]].src[1]];
        bias[i] = g.nodes[lin[i]].n_src == 3 ? g.nodes[lin[i]].src[2] : -1;
        if (i) with += (i > 1 ? "|" : "") + w[i]->name;
    }
    const int k = (int)w[0]->ne[0], n1 = (int)w[0]->ne[1];
    packed_operand p;
    p.n_real = 3 * n1; p.k_real = k; p.N = 3 * n1; p.K = round_up(k, 64);
    p.w = cached(g.nodes[lin[0]].src[1], role_qkv, [&](bool st) {
        std::vector<uint16_t> h((size_t)p.N * p.K, 0);
        for (int i = 0; i < 3; ++i)
            for (int r = 0; r < n1; ++r)
                for (int c = 0; c < k; ++c) h[((size_t)i * n1 + r) * p.K + c] = f32_to_f16(w[i]->values()[(size_t)r * k + c]);
        return upload(h.data(), h.size() * 2, st);
    }, with);
    if (bias[0] >= 0 || bias[1] >= 0 || bias[2] >= 0)
        p.bias = static_cast<float*>(cached(g.nodes[lin[0]].src[1], bias_of_role(role_qkv), [&](bool st) {
            std::vector<float> b((size_t)p.N, 0.0f);
            for (int i = 0; i < 3; ++i)
                if (bias[i] >= 0)
                    for (int r = 0; r < n1; ++r) b[(size_t)i * n1 + r] = g.nodes[bias[i]].values()[r];
            return upload(b.data(), b.size() * 4, st);
        }, with));
    return p;
}
packed_operand lowering::pack_conv_transpose(int wt, int bias_t, int s) { // ne [kw, kh, Cout, Cin]: row (dy * s + dx) * Cout + co, column ci
    graph_node const& w = g.nodes[wt];
    const int kw = (int)w.ne[0], kh = (int)w.ne[1], cout = (int)w.ne[2], cin = (int)w.ne[3];
    const float* h = w.values();
    return pack_matrix(wt, role_conv_transpose, s * s * cout, cin,
                       [=](int r, int c) {
                           const int tap = r / cout, co = r % cout, dy = tap / s, dx = tap % s;
                           return h[(((size_t)c * cout + co) * kh + dy) * kw + dx];
                       },
                       bias_t, cout);
}

// the DPT head's 3x3 kernel (Cin -> 32) as the head kernel's MFMA fragments (Cin 64 / 128: one 32-channel slice after the other)
void* lowering::pack_head_fragments(int wt, int cin) {
    return cached(wt, role_head_frag, [&](bool st) {
        const int K = 9 * cin, Kp = cin == 32 ? 320 : K;
        std::vector<uint16_t> rows((size_t)32 * Kp, 0), out((cin == 32 ? vx_headconv_frag_bytes() : vx_headconv_wide_frag_bytes(cin)) / 2);
        for (int r = 0; r < 32; ++r)
            for (int k = 0; k < K; ++k) rows[(size_t)r * Kp + k] = f32_to_f16(g.nodes[wt].values()[(size_t)r * K + k]);
        if (cin == 32) VX(vx_headconv_pack(rows.data(), Kp, out.data()));
        else VX(vx_headconv_wide_pack(rows.data(), cin, Kp, out.data()));
        return upload(out.data(), out.size() * 2, st);
    });
}

// the LDS-ring conv's operand: slabs [cin pad 32 / 32][9 taps][cout][32] f16, 16-byte groups swizzled (kernels_dconv.hip)
void* lowering::pack_dconv(int wt, int cin, int cout, int* d_cin) {
    const int dc = round_up(cin, 32);
    *d_cin = dc;
    return cached(wt, role_dconv, [&](bool st) {
        std::vector<uint16_t> h((size_t)dc * 9 * cout, 0);
        const float* w = g.nodes[wt].values(); // [cout][ky][kx][cin]
        for (int n = 0; n < cout; ++n)
            for (int tap = 0; tap < 9; ++tap)
                for (int c = 0; c < cin; ++c) {
                    const size_t row = ((size_t)(c / 32) * 9 + tap) * cout + n;
                    h[row * 32 + (size_t)(((c % 32) / 8) ^ ((n >> 2) & 3)) * 8 + c % 8] = f32_to_f16(w[((size_t)n * 9 + tap) * cin + c]);
                }
        return upload(h.data(), h.size() * 2, st);
    });
}
// the LDS-ring conv's operand with the input columns repeated (`dup`: an image plane carries value | residue) and the outputs padded to `cout_pad`
void* lowering::pack_dconv_ex(int wt, int cin, int dup, int cout, int cout_pad, int* d_cin) {
    const int n_in = dup ? 2 * cin : cin, dc = round_up(n_in, 32);
    *d_cin = dc;
    return cached(wt, role_dconv_ex, [&](bool st) {
        std::vector<uint16_t> h((size_t)dc * 9 * cout_pad, 0);
        const float* w = g.nodes[wt].values(); // [cout][ky][kx][cin]
        for (int n = 0; n < cout; ++n)
            for (int tap = 0; tap < 9; ++tap)
                for (int c = 0; c < n_in; ++c) {
                    const size_t row = ((size_t)(c / 32) * 9 + tap) * cout_pad + n;
                    h[row * 32 + (size_t)(((c % 32) / 8) ^ ((n >> 2) & 3)) * 8 + c % 8] = f32_to_f16(w[((size_t)n * 9 + tap) * cin + c % cin]);
                }
        return upload(h.data(), h.size() * 2, st);
    }, "dup" + std::to_string(dup) + "pad" + std::to_string(cout_pad));
}
float* lowering::bias_padded(int bt, int n_pad) {
    return static_cast<float*>(cached(bt, role_bias_padded, [&](bool st) {
        std::vector<float> b((size_t)n_pad, 0.0f);
        for (int64_t i = 0; i < g.nodes[bt].n_elements() && i < n_pad; ++i) b[(size_t)i] = g.nodes[bt].values()[i];
        return upload(b.data(), b.size() * 4, st);
    }, "pad" + std::to_string(n_pad)));
}

// the residual-unit kernel's operand: [taps][64 n][64 c] f16, the 16-byte groups of row n at position g ^ ((n >> 1) & 7) (kernels_rcu.hip)
void* lowering::pack_rcu(int wt, int taps) {
    return cached(wt, role_rcu, [&](bool st) {
        std::vector<uint16_t> h((size_t)taps * 64 * 64);
        const float* w = g.nodes[wt].values(); // [n][ky][kx][c]
        for (int n = 0; n < 64; ++n)
            for (int tap = 0; tap < taps; ++tap)
                for (int c = 0; c < 64; ++c)
                    h[((size_t)tap * 64 + n) * 64 + (size_t)((c >> 3) ^ ((n >> 1) & 7)) * 8 + (c & 7)] = f32_to_f16(w[((size_t)n * taps + tap) * 64 + c]);
        return upload(h.data(), h.size() * 2, st);
    });
}

// the deformable conv's operand: the kernel's rows [cout][ky][kx][cin] as they are, f16, zero rows up to a multiple of 32 (kernels_deform.hip)
void* lowering::pack_deform(int wt, int* n_pad) {
    graph_node const& w = g.nodes[wt];
    const int cout = (int)w.ne[3], np = round_up(cout, 32);
    const size_t k = (size_t)(w.n_elements() / cout);
    *n_pad = np;
    return cached(wt, role_deform, [&](bool st) {
        std::vector<uint16_t> h((size_t)np * k, 0);
        for (size_t i = 0; i < (size_t)cout * k; ++i) h[i] = f32_to_f16(w.values()[i]);
        return upload(h.data(), h.size() * 2, st);
    });
}
// offset and modulator kernels over the same input as ONE operand: rows 0 .. 2 k^2 - 1 the offsets, then k^2 modulator logits, biases alike
// (what pack_deform of csrc/birefnet.cpp does for the hand schedule)
packed_operand lowering::pack_deform_offsets(int w_off, int b_off, int w_mod, int b_mod) {
    graph_node const &wo = g.nodes[w_off], &wm = g.nodes[w_mod];
    const int n_off = (int)wo.ne[3], n_mod = (int)wm.ne[3], k = (int)(wo.n_elements() / n_off);
    const std::string with = const_id(g, w_mod) + "|" + const_id(g, b_off) + "|" + const_id(g, b_mod);
    packed_operand p;
    p.n_real = n_off + n_mod; p.k_real = k;
    p.N = round_up(p.n_real, p.n_real > 64 ? 64 : 32);
    p.K = round_up(k, 64);
    p.w = cached(w_off, role_deform_offsets, [&](bool st) {
        std::vector<uint16_t> h((size_t)p.N * p.K, 0);
        for (int r = 0; r < p.n_real; ++r) {
            const float* row = r < n_off ? wo.values() + (size_t)r * k : wm.values() + (size_t)(r - n_off) * k;
            for (int c = 0; c < k; ++c) h[(size_t)r * p.K + c] = f32_to_f16(row[c]);
        }
        return upload(h.data(), h.size() * 2, st);
    }, with);
    p.bias = vec_cached(w_off, role_deform_offsets_bias, with, [&] {
        std::vector<float> b((size_t)p.N, 0.0f);
        for (int r = 0; r < n_off && b_off >= 0; ++r) b[(size_t)r] = g.nodes[b_off].values()[r];
        for (int r = 0; r < n_mod && b_mod >= 0; ++r) b[(size_t)n_off + r] = g.nodes[b_mod].values()[r];
        return b;
    });
    return p;
}

// the depthwise conv's operand: f16 [k * k][C], tap = ky * k + kx, from either stored form -- [C, 1, kw, kh] (channel fastest: the rows as they
// are) or [1, kw, kh, C] (a depthwise OIHW kernel listed in conv2d_weights: channel slowest)
void* lowering::pack_depthwise(int wt, int C, int k) {
    graph_node const& w = g.nodes[wt];
    const bool channel_first = w.ne[0] == C && w.ne[1] == 1;
    return cached(wt, role_depthwise, [&](bool st) {
        std::vector<uint16_t> h((size_t)k * k * C);
        for (int tap = 0; tap < k * k; ++tap)
            for (int c = 0; c < C; ++c) h[(size_t)tap * C + c] = f32_to_f16(w.values()[channel_first ? (size_t)tap * C + c : (size_t)c * k * k + tap]);
        return upload(h.data(), h.size() * 2, st);
    });
}
// conv [C, kw, kh, Cout], C = 3 or 4, on 8-channel value | residue pixels (image_pad8): every tap's C columns repeated on channels C..2C-1, zeros behind them, so the f32
// accumulator adds w * hi + w * lo = w * (the f32 pixel up to the residue's own rounding)
packed_operand lowering::pack_image8(int wt, int bias_t, int n) {
    graph_node const& w = g.nodes[wt];
    const int C = (int)w.ne[0], kc = (int)(w.n_elements() / n), taps = kc / C;
    const float* h = w.values();
    return pack_matrix(wt, role_image8, n, taps * 8, [h, kc, C](int r, int c) { return c % 8 < 2 * C ? h[(size_t)r * kc + (c / 8) * C + (c % 8) % C] : 0.0f; }, bias_t, n);
}

// RepConv (yolov9t.cpp:256-300): conv3x3(x) + conv1x1(x) at the same stride is one 3x3 conv whose centre tap holds the 1x1 kernel as well. Rows [Cout][9 Cin],
// k = (ky, kx, c); the sums are made in f32 before the one f16 rounding, the biases summed in f32
packed_operand lowering::pack_rep_conv(int w3, int b3, int w1, int b1) {
    graph_node const &a = g.nodes[w3], &b = g.nodes[w1];
    const int n = (int)a.ne[3], cin = (int)a.ne[0], k = 9 * cin;
    const std::string with = "+" + const_id(g, w1);
    packed_operand p;
    p.n_real = n; p.k_real = k;
    p.N = round_up(n, n > 64 ? 64 : 32);
    p.K = round_up(k, 64);
    p.w = cached(w3, role_rep_conv, [&](bool st) {
        std::vector<uint16_t> h((size_t)p.N * p.K, 0);
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < k; ++c) {
                float v = a.values()[(size_t)r * k + c];
                if (c / cin == 4) v += b.values()[(size_t)r * cin + c % cin];
                h[(size_t)r * p.K + c] = f32_to_f16(v);
            }
        return upload(h.data(), h.size() * 2, st);
    }, with);
    if (b3 >= 0 || b1 >= 0)
        p.bias = static_cast<float*>(cached(w3, role_rep_conv_bias, [&](bool st) {
            std::vector<float> v((size_t)p.N, 0.0f);
            for (int r = 0; r < n; ++r) v[r] = (b3 >= 0 ? g.nodes[b3].values()[r] : 0.0f) + (b1 >= 0 ? g.nodes[b1].values()[r] : 0.0f);
            return upload(v.data(), v.size() * 4, st);
        }, with));
    return p;
}

float* lowering::vec_cached(int key_node, pack_role role, std::string const& with, std::function<std::vector<float>()> make_host) {
    return static_cast<float*>(cached(key_node, role, [&](bool st) { std::vector<float> v = make_host(); return upload(v.data(), v.size() * 4, st); }, with));
}

} // namespace visp
