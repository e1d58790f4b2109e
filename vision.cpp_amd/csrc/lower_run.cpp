// Graph lowering: liveness, the per-node dispatch, the glue ops and the buffer plan (see lowering.h).
#include "lowering.h"

namespace visp {

void lowering::map_launch(int t, std::string desc, std::function<void(char* x, char* out, char* scratch, void* stream)> run, size_t scratch_bytes) {
    const int xbuf = buf_of(g.nodes[t].src[0]);
    materialise(t);
    const int obuf = g.nodes[t].buffer, sbuf = scratch_bytes ? new_buffer(scratch_bytes) : -1;
    auto xp = ptr(xbuf), op = ptr(obuf), sp = ptr(std::max(sbuf, 0));
    emit(std::move(desc), {xbuf}, sbuf < 0 ? std::vector<int>{obuf} : std::vector<int>{obuf, sbuf}, [=](void* st) { run(xp(), op(), sbuf < 0 ? nullptr : sp(), st); });
}

void lowering::copy_op(int t) {
    graph_node& n = g.nodes[t];
    materialise(t);
    const int obuf = n.buffer;
    auto op = ptr(obuf);
    auto strides = [](const int64_t ne[4], int64_t s[4]) { s[0] = 1; s[1] = ne[0]; s[2] = ne[0] * ne[1]; s[3] = ne[0] * ne[1] * ne[2]; };
    if (n.op == gop_slice || n.op == gop_repeat) {
        graph_node const& x = g.nodes[n.src[0]];
        const int xbuf = buf_of(n.src[0]);
        auto xp = ptr(xbuf);
        int64_t xs[4], ds[4], ne[4], ss[4], off = 0;
        strides(x.ne, xs);
        strides(n.ne, ds);
        for (int d = 0; d < 4; ++d) {
            ne[d] = n.ne[d];
            if (n.op == gop_slice) { off += n.ip[3 * d] * xs[d]; ss[d] = xs[d] * n.ip[3 * d + 2]; }
            else ss[d] = x.ne[d] == 1 && n.ne[d] > 1 ? 0 : xs[d];
        }
        std::array<int64_t, 4> A{ne[0], ne[1], ne[2], ne[3]}, S{ss[0], ss[1], ss[2], ss[3]}, D{ds[0], ds[1], ds[2], ds[3]};
        emit(std::string(graph_op_name(n.op)) + " " + shape_str(x.ne) + " -> " + shape_str(n.ne), {xbuf}, {obuf},
             [=](void* st) { VX(vx_copy_strided_f16(xp() + off * 2, op(), A.data(), S.data(), D.data(), 1.0f, st)); });
        return;
    }
    // concat: each source into its block of the destination
    const int dim = (int)n.ip[0];
    int64_t ds[4];
    strides(n.ne, ds);
    int64_t at = 0;
    for (int i = 0; i < 2; ++i) {
        graph_node const& x = g.nodes[n.src[i]];
        int64_t xs[4];
        strides(x.ne, xs);
        std::array<int64_t, 4> A{x.ne[0], x.ne[1], x.ne[2], x.ne[3]}, S{xs[0], xs[1], xs[2], xs[3]}, D{ds[0], ds[1], ds[2], ds[3]};
        const int64_t off = at * ds[dim];
        at += x.ne[dim];
        std::string d = "concat part " + std::to_string(i) + " " + shape_str(x.ne) + " -> " + shape_str(n.ne);
        if (x.constant) {
            void* cp = const_f16(n.src[i]);
            emit(d + " (constant)", {}, {obuf}, [=](void* st) { VX(vx_copy_strided_f16(cp, op() + off * 2, A.data(), S.data(), D.data(), 1.0f, st)); });
        } else if (lives_in_place(n.src[i])) { // a channel slice read in its source, or a map that lives in another concat's buffer
            const located L = locate(n.src[i]);
            auto xp = ptr(L.buf);
            const int64_t x_off = L.off;
            std::array<int64_t, 4> SP{1, L.pix, L.pix * x.ne[1], L.pix * x.ne[1] * x.ne[2]};
            emit(d, {L.buf}, {obuf}, [=](void* st) { VX(vx_copy_strided_f16(xp() + x_off * 2, op() + off * 2, A.data(), SP.data(), D.data(), 1.0f, st)); });
        } else {
            const int xbuf = buf_of(n.src[i]);
            auto xp = ptr(xbuf);
            emit(d, {xbuf}, {obuf}, [=](void* st) { VX(vx_copy_strided_f16(xp(), op() + off * 2, A.data(), S.data(), D.data(), 1.0f, st)); });
        }
    }
}

void lowering::run() {
    const int N = (int)g.nodes.size();
    needed.assign(N, 0);
    skip.assign(N, 0);
    uses.assign(N, 0);
    relu_on_load.assign(N, 0);
    claimed_by.assign(N, -1);
    consumers.assign(N, {});
    bool any_out = false;
    for (int t = N - 1; t >= 0; --t) {
        graph_node const& n = g.nodes[t];
        if (n.is_output) { needed[t] = 1; any_out = true; }
        if (!needed[t]) continue;
        for (int i = 0; i < n.n_src; ++i) needed[n.src[i]] = 1;
    }
    if (!any_out) throw except("graph_allocate: the graph has no output (compute_graph_output)");
    for (int t = 0; t < N; ++t) {
        graph_node const& n = g.nodes[t];
        if (!needed[t] || n.constant) continue;
        for (int i = 0; i < n.n_src; ++i) {
            uses[n.src[i]]++;
            consumers[n.src[i]].push_back(t);
        }
    }
    find_deform_groups();
    find_sam3_groups(); // (before find_qkv_groups: the q|k|v chain walks through a rope_2d group)
    find_qkv_groups();
    find_window_groups();
    find_encoder_chain();
    find_yolo_groups();
    find_migan_groups();
    find_sam_groups();
    find_birefnet_groups();
    for (int t = 0; t < N; ++t) {
        graph_node& n = g.nodes[t];
        if (enc.ok && t == enc.first) emit_encoder();
        if (auto it = qkv_first.find(t); it != qkv_first.end() && !skip[t]) fused_qkv(it->second);
        if (!needed[t] || skip[t]) continue;
        if (n.constant) {
            if (n.is_output) throw except("graph_allocate: output '%s' is a constant", n.name.c_str());
            continue;
        }
        if (migan_emits(t)) continue; // the last node of an lrelu_agc / FIR upsample group: the group's one launch
        std::string who = n.name;
        switch (n.op) {
            case gop_input: materialise(t); break;
            case gop_reshape:
            case gop_cont:
                n.alias_of = n.src[0];
                if (n.is_output) { // an output view keeps its source alive
                    graph_node& r = g.nodes[root(t)];
                    r.is_output = true;
                    if (r.buffer >= 0) g.buffers[r.buffer].persistent = true;
                }
                break;
            case gop_linear:
            case gop_conv_2d:
            case gop_conv_transpose_2d: gemm_like(t); break;
            case gop_patch_embed: patch_embed(t); break;
            case gop_attention: attention(t); break;
            case gop_attention_masked: attention_masked(t); break;
            case gop_attention_cross: attention_cross(t); break;
            case gop_mul_mat: mul_mat(t); break;
            case gop_sin:
            case gop_cos: sincos(t); break;
            case gop_conv_2d_deform: deform_conv(t); break;
            case gop_conv_2d_depthwise: depthwise_conv(t); break;
            case gop_pool_2d: pool_2d(t); break;
            case gop_soft_max: soft_max(t); break;
            case gop_sum_rows: sum_rows(t); break;
            case gop_sigmoid: {
                const int64_t cnt = n.n_elements();
                const int x_f32 = g.nodes[n.src[0]].dtype == gdt_f32;
                map_launch(t, "sigmoid n=" + std::to_string(cnt), [=](char* x, char* o, char*, void* st) { VX(vx_sigmoid_f16(x, x_f32, o, cnt, st)); });
                tag("glue", 0, (double)cnt * 4);
            } break;
            case gop_mean_2d: {
                graph_node const& x = g.nodes[n.src[0]];
                const int B = (int)x.ne[3], C = (int)x.ne[0];
                const int64_t px = x.ne[1] * x.ne[2];
                map_launch(t, "mean_2d " + shape_str(x.ne), [=](char* xp, char* o, char*, void* st) { VX(vx_mean_2d_f16(xp, o, B, px, C, st)); });
                tag("mean", 0, (double)x.n_elements() * 2);
            } break;
            case gop_cast: n.alias_of = n.src[0]; break; // an activation already has the type (graph_add refuses the rest): a view
            case gop_get_rows: get_rows(t); break; // an i32 graph input on a constant table; a non-constant table is refused there
            case gop_rope: rope(t); break;
            case gop_permute: { // one strided copy: destination dimension ip[d] walks source dimension d
                graph_node const& x = g.nodes[n.src[0]];
                const int xbuf = buf_of(n.src[0]);
                materialise(t);
                const int obuf = n.buffer;
                auto xp = ptr(xbuf), op = ptr(obuf);
                std::array<int64_t, 4> A{n.ne[0], n.ne[1], n.ne[2], n.ne[3]}, D{1, n.ne[0], n.ne[0] * n.ne[1], n.ne[0] * n.ne[1] * n.ne[2]}, S{};
                const int64_t xs[4] = {1, x.ne[0], x.ne[0] * x.ne[1], x.ne[0] * x.ne[1] * x.ne[2]};
                for (int d = 0; d < 4; ++d) S[n.ip[d]] = xs[d];
                emit("permute " + shape_str(x.ne) + " -> " + shape_str(n.ne), {xbuf}, {obuf}, [=](void* st) { VX(vx_copy_strided_f16(xp(), op(), A.data(), S.data(), D.data(), 1.0f, st)); });
                tag("glue", 0, (double)n.n_elements() * 4);
            } break;
            case gop_roll: {
                graph_node const& x = g.nodes[n.src[0]];
                std::array<int64_t, 4> A{x.ne[0], x.ne[1], x.ne[2], x.ne[3]}, Sh{n.ip[0], n.ip[1], n.ip[2], n.ip[3]};
                char d[160];
                snprintf(d, sizeof d, "roll %s by [%lld, %lld, %lld, %lld]", shape_str(x.ne).c_str(), (long long)Sh[0], (long long)Sh[1], (long long)Sh[2], (long long)Sh[3]);
                map_launch(t, d, [=](char* xp, char* o, char*, void* st) { VX(vx_roll_f16(xp, o, A.data(), Sh.data(), st)); });
                tag("glue", 0, (double)n.n_elements() * 4);
            } break;
            case gop_pad: {
                graph_node const& x = g.nodes[n.src[0]];
                std::array<int64_t, 4> A{x.ne[0], x.ne[1], x.ne[2], x.ne[3]}, D{n.ne[0], n.ne[1], n.ne[2], n.ne[3]};
                map_launch(t, "pad " + shape_str(x.ne) + " -> " + shape_str(n.ne), [=](char* xp, char* o, char*, void* st) { VX(vx_pad_f16(xp, o, A.data(), D.data(), st)); });
                tag("glue", 0, (double)(x.n_elements() + n.n_elements()) * 2);
            } break;
            case gop_relu: {
                const int c = sole_consumer(t);
                if (c >= 0 && g.nodes[c].op == gop_conv_2d && g.nodes[c].src[0] == t && !(g.nodes[g.nodes[c].src[1]].ne[1] == 1 && g.nodes[g.nodes[c].src[1]].ne[2] == 1)) {
                    relu_on_load[c] = 1; // the conv's loader applies it (depth-anything.cpp:17-20)
                    n.alias_of = n.src[0];
                    break;
                }
            }
                [[fallthrough]];
            case gop_gelu:
            case gop_leaky_relu:
            case gop_silu:
            case gop_scale: {
                if (n.dtype != gdt_f16) throw except("%s on the f32 map of a one-channel head that has other readers is not built", graph_op_name(n.op));
                const int64_t cnt = n.n_elements();
                const int uop = n.op == gop_gelu ? 0 : (n.op == gop_relu ? 1 : (n.op == gop_leaky_relu ? 3 : (n.op == gop_silu ? 4 : 2)));
                const float s = n.fp[0];
                map_launch(t, std::string(graph_op_name(n.op)) + " n=" + std::to_string(cnt), [=](char* x, char* o, char*, void* st) { VX(vx_unary_f16(uop, x, o, cnt, s, st)); });
            } break;
            case gop_clamp: clamp_op(t); break;
            case gop_add:
            case gop_mul:
            case gop_sub: {
                if (auto it = gate_groups.find(t); it != gate_groups.end()) { pixel_gate(t, it->second); break; }
                graph_node const& b = g.nodes[n.src[1]];
                if (plane_broadcast(n.ne, b.ne)) { plane_binary(t); break; }
                if (g.nodes[n.src[0]].constant) throw except("%s: the larger operand is a constant; broadcast of an activation onto it is not built", graph_op_name(n.op));
                const int abuf = buf_of(n.src[0]);
                const int64_t period = b.n_elements(), cnt = n.n_elements();
                const int bop = n.op == gop_add ? 0 : (n.op == gop_mul ? 1 : 2);
                std::vector<int> reads = {abuf};
                std::function<char*()> bp;
                float* bc = nullptr;
                if (b.constant) bc = const_f32(n.src[1]);
                else { reads.push_back(buf_of(n.src[1])); bp = ptr(buf_of(n.src[1])); }
                materialise(t);
                const int obuf = n.buffer;
                auto ap = ptr(abuf), op = ptr(obuf);
                emit(std::string(graph_op_name(n.op)) + " n=" + std::to_string(cnt) + " period=" + std::to_string(period) + (bc || !bp ? " (constant)" : ""), reads, {obuf}, [=](void* st) {
                    if (bp) VX(vx_binary_rows(bop, ap(), 0, bp(), 0, period, op(), 0, cnt, st));
                    else VX(vx_binary_rows(bop, ap(), 0, bc, 1, period, op(), 0, cnt, st));
                });
            } break;
            case gop_layer_norm: {
                if (g.fused_models && cat_slot.count(t)) { layer_norm_in_place(t); break; } // into its slice of a concat (lower_birefnet.cpp)
                const int C = (int)n.ne[0];
                if (C % 8 || C > 1024) throw except("layer_norm: %d channels (a multiple of 8, at most 1024)", C);
                float *w = const_f32(n.src[1]), *b = const_f32(n.src[2]);
                const int64_t rows = n.n_elements() / C;
                const float eps = n.fp[0];
                map_launch(t, "layer_norm rows=" + std::to_string(rows) + " C=" + std::to_string(C) + (who.empty() ? "" : " <- " + who),
                           [=](char* x, char* o, char*, void* st) { VX(vx_layernorm_f16(x, w, b, o, rows, C, eps, 0, 0, 0, st)); });
                tag("layernorm", 0, (double)rows * C * 4);
            } break;
            case gop_image_patches: image_patches(t); break;
            case gop_interpolate: {
                if (n.dtype == gdt_f32) { image_resize(t); break; } // an f32 image (graph_add admits bilinear | align_corners only)
                if (g.fused_models && (n.ip[2] & 255) == 1 && cat_slot.count(t)) { bilinear_in_place(t); break; }
                if (nearest_into_reader(t)) break;
                const bool nearest = (n.ip[2] & 255) == 0; // NEAREST on its own, or bilinear | align_corners
                if (!nearest && ((!n.is_output && head_tail(t)) || resize_into_reader(t))) break;
                graph_node const& x = g.nodes[n.src[0]];
                if (!nearest && ((n.ip[2] & 255) != 1 || !(n.ip[2] & 256))) throw except("interpolate: mode %lld on activations is not built (bilinear | align_corners is; bicubic on constants)", (long long)n.ip[2]);
                if (x.ne[0] % 8) throw except("interpolate: %lld channels (a multiple of 8)", (long long)x.ne[0]);
                const int B = (int)x.ne[3], H = (int)x.ne[2], W = (int)x.ne[1], C = (int)x.ne[0], OH = (int)n.ne[2], OW = (int)n.ne[1];
                if (nearest && g.fused_models && (lives_in_place(n.src[0]) || cat_slot.count(t))) { nearest_in_place(t); break; }
                char d[128];
                snprintf(d, sizeof d, "%s %dx%d -> %dx%d C=%d", nearest ? "nearest" : "bilinear_ac", W, H, OW, OH, C);
                map_launch(t, d, [=](char* xp, char* o, char*, void* st) {
                    if (nearest) VX(vx_nearest_f16(xp, o, B, H, W, C, OH, OW, st));
                    else VX(vx_bilinear_ac_f16(xp, o, B, H, W, C, OH, OW, st));
                });
                if (!nearest) tag("bilinear", 0, (double)B * ((double)H * W + (double)OH * OW) * C * 2);
            } break;
            case gop_image_u8_to_f32: { // not read by a fused patch embedding: the f32 image itself
                graph_node const& x = g.nodes[n.src[0]];
                const int B = (int)x.ne[3], H = (int)x.ne[2], W = (int)x.ne[1];
                std::array<float, 3> mean{n.fp[0], n.fp[1], n.fp[2]}, istd{n.fp[3], n.fp[4], n.fp[5]};
                map_launch(t, "image_u8_to_f32 " + shape_str(x.ne), [=](char* xp, char* o, char*, void* st) {
                    VX(vx_preprocess_f32(reinterpret_cast<const uint8_t*>(xp), reinterpret_cast<float*>(o), B, H, W, mean.data(), istd.data(), st));
                });
                tag("preprocess", 0, (double)B * H * W * 15);
            } break;
            case gop_image_normalize: {
                graph_node const& x = g.nodes[n.src[0]];
                const int B = (int)x.ne[3];
                const int64_t px = x.ne[1] * x.ne[2];
                map_launch(t, "image_normalize B=" + std::to_string(B), [=](char* xp, char* o, char* minmax, void* st) {
                    VX(vx_minmax_normalize(reinterpret_cast<const float*>(xp), reinterpret_cast<float*>(o), reinterpret_cast<float*>(minmax), B, px, st));
                }, (size_t)x.ne[3] * 8);
                tag("normalize", 0, (double)B * px * 12);
            } break;
            case gop_slice:
                if (chan_slice.count(t)) break; // channels [c0, c1) only: its readers address it in its source (lower_yolo.cpp)
                // rows [b, e) of every image's token block, read by one plain product only (dpt::neck drops the cls token, depth-anything.cpp:50):
                // the GEMM's A rows are addressed in the source, no copy
                if (g.fused_models && !n.is_output && plain_gemm_reader(t) >= 0 && n.ip[0] == 0 && n.ne[0] == g.nodes[n.src[0]].ne[0] && n.ne[0] % 64 == 0 && n.ip[5] == 1 &&
                    n.ne[2] == g.nodes[n.src[0]].ne[2] && n.ip[6] == 0 && n.ne[3] == g.nodes[n.src[0]].ne[3] && n.ip[9] == 0 && g.nodes[n.src[0]].ne[3] == 1 &&
                    row_stride.find(root_view(n.src[0])) == row_stride.end()) {
                    sliced_in[t] = {n.src[0], n.ip[3], n.ne[1], g.nodes[n.src[0]].ne[1]};
                    n.alias_of = n.src[0];
                    break;
                }
                copy_op(t);
                break;
            case gop_concat:
                if (auto it = fourier_groups.find(t); it != fourier_groups.end()) { fourier_features(t, it->second); break; }
                if (auto it = rope2d_groups.find(t); it != rope2d_groups.end()) { rope2d(t, it->second); break; }
                if (cat_sources.count(t)) { concat_in_place(t); break; }
                copy_op(t);
                break;
            case gop_repeat:
                if (same_shape(n, g.nodes[n.src[0]])) { // to its own shape (mobile-sam.cpp:439 at batch 1): a view
                    n.alias_of = n.src[0];
                    if (n.is_output) {
                        graph_node& r = g.nodes[root(t)];
                        r.is_output = true;
                        if (r.buffer >= 0) g.buffers[r.buffer].persistent = true;
                    }
                    break;
                }
                copy_op(t);
                break;
            default: throw except("graph_allocate: %s is not lowered", graph_op_name(n.op));
        }
    }
    for (auto const& sl : cat_slot)
        if (!lives_in_place(sl.first)) throw except("graph: internal: the slice of concat %d reserved for tensor %d was never written", sl.second.first, sl.first);
    if (!placed.empty()) throw except("graph: internal: a plane reserved for tensor %d of a dense block was never written", placed.begin()->first);
    plan_arena();
}

// buffer lifetimes from the launch list, then offsets: persistent buffers first, the others first-fit into the holes their
// predecessors left (ggml_gallocr's job in the reference, ml.cpp:545-552)
void lowering::plan_arena() {
    const int L = (int)g.launches.size();
    for (auto& b : g.buffers) { b.first = L; b.last = -1; }
    for (int i = 0; i < L; ++i) {
        for (int b : io[i].second) { g.buffers[b].first = std::min(g.buffers[b].first, i); g.buffers[b].last = std::max(g.buffers[b].last, i); }
        for (int b : io[i].first) { g.buffers[b].first = std::min(g.buffers[b].first, i); g.buffers[b].last = std::max(g.buffers[b].last, i); }
    }
    for (auto& n : g.nodes)
        if (n.buffer >= 0 && (n.is_output || n.op == gop_input)) g.buffers[n.buffer].persistent = true;
    size_t top = 0;
    g.sum_bytes = 0;
    for (auto& b : g.buffers) {
        g.sum_bytes += b.bytes;
        if (b.persistent) { b.offset = top; top += b.bytes; }
    }
    const size_t base = top;
    struct block { size_t off, bytes; };
    std::vector<block> free_list;
    std::vector<std::vector<int>> starts(L + 1), ends(L + 1);
    for (int i = 0; i < (int)g.buffers.size(); ++i) {
        graph_buffer const& b = g.buffers[i];
        if (b.persistent || b.last < 0) continue;
        starts[b.first].push_back(i);
        ends[b.last].push_back(i);
    }
    size_t high = base;
    for (int i = 0; i < L; ++i) {
        for (int bi : starts[i]) {
            graph_buffer& b = g.buffers[bi];
            int best = -1;
            for (int f = 0; f < (int)free_list.size(); ++f)
                if (free_list[f].bytes >= b.bytes && (best < 0 || free_list[f].bytes < free_list[best].bytes)) best = f;
            if (best >= 0) {
                b.offset = free_list[best].off;
                free_list[best].off += b.bytes;
                free_list[best].bytes -= b.bytes;
                if (free_list[best].bytes == 0) free_list.erase(free_list.begin() + best);
            } else if (!free_list.empty() && free_list.back().off + free_list.back().bytes == high) { // grow the block at the top
                b.offset = free_list.back().off;
                high = b.offset + b.bytes;
                free_list.pop_back();
            } else {
                b.offset = high;
                high += b.bytes;
            }
        }
        for (int bi : ends[i]) {
            graph_buffer const& b = g.buffers[bi];
            free_list.push_back({b.offset, b.bytes});
            std::sort(free_list.begin(), free_list.end(), [](block const& x, block const& y) { return x.off < y.off; });
            for (size_t f = 0; f + 1 < free_list.size();) {
                if (free_list[f].off + free_list[f].bytes == free_list[f + 1].off) {
                    free_list[f].bytes += free_list[f + 1].bytes;
                    free_list.erase(free_list.begin() + f + 1);
                } else ++f;
            }
        }
    }
    g.arena_bytes = high + 65536; // slack behind the last buffer: tile-granular loaders may read past a tail row
}

} // namespace visp
