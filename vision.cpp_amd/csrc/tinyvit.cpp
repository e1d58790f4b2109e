#include <algorithm>
#include <cstdlib>

#include "packer.h"
#include "sam_pass.h"

namespace visp {

sam_model* sam_load_model(char const* filepath, backend_device const& dev, int flags) {
    const bool with_data = !(flags & load_no_upload);
    model_file file = model_load(filepath, /*header_only=*/!with_data);
    if (file.arch() != "mobile-sam")
        throw except("Model %s has architecture '%.*s', expected 'mobile-sam'", filepath, (int)file.arch().size(), file.arch().data());
    auto model = std::make_unique<sam_model>();
    model->backend = &dev;
    tiny_vit_params const& P = model->params;
    arena_builder ab;
    packer pk{file, ab, with_data, file.tensor_layout() != layout_cwhn, file.conv2d_weights()};
    tinyvit_weights& Wt = model->weights;
    const std::string e = "enc.";
    int k, cin;
    Wt.pe0 = pk.conv(e + "patch_embed.seq.0.c", &k, &cin, /*dup_in=*/true);
    if (k != 3) throw except("mobile-sam: patch embedding kernel is %dx%d, expected 3x3", k, k);
    Wt.pe2 = pk.conv(e + "patch_embed.seq.2.c", &k, &cin);
    if (Wt.pe2.n_real != P.layers[0].embed_dim) throw except("mobile-sam: patch embedding width %d, expected %d", Wt.pe2.n_real, P.layers[0].embed_dim);
    auto merge = [&](std::string const& p) {
        tv_merge_weights m;
        m.conv1 = pk.conv(p + ".conv1.c");
        m.conv2 = pk.depthwise(p + ".conv2.c");
        m.conv3 = pk.conv(p + ".conv3.c");
        const int co = m.conv1.n_real;
        m.stride = (co == 320 || co == 448 || co == 576) ? 1 : 2; // mobile-sam.cpp:98-100
        return m;
    };
    for (int i = 0; i < P.layers[0].depth; ++i) {
        std::string p = e + "layers.0.blocks." + std::to_string(i);
        tv_mbconv_weights mb;
        mb.conv1 = pk.conv(p + ".conv1.c");
        mb.conv2 = pk.depthwise(p + ".conv2.c");
        mb.conv3 = pk.conv(p + ".conv3.c");
        if (vx_mbconv_dw_pw_supported(mb.conv2.C, mb.conv3.n_real, P.layers[0].resolution) && mb.conv3.N == mb.conv3.n_real && mb.conv3.K == mb.conv2.C) {
            mb.conv3_frag = ab.alloc((size_t)mb.conv3.N * mb.conv3.K * 2); // the fused kernel reads W3 in MFMA fragment order
            if (with_data) {
                std::vector<uint16_t> rows((size_t)mb.conv3.N * mb.conv3.K); // copy: alloc() may have moved the arena
                memcpy(rows.data(), ab.data.data() + mb.conv3.w, rows.size() * 2);
                VX(vx_mbconv_pack_w3(rows.data(), ab.data.data() + mb.conv3_frag));
            }
        }
        Wt.mbconv.push_back(mb);
    }
    Wt.merge[0] = merge(e + "layers.0.downsample");
    for (int l = 1; l < 4; ++l) {
        tiny_vit_layer const& L = P.layers[l];
        for (int i = 0; i < L.depth; ++i) {
            std::string p = e + "layers." + std::to_string(l) + ".blocks." + std::to_string(i);
            tv_block_weights b;
            b.attn_ln_w = pk.vec(p + ".attn.norm.weight");
            b.attn_ln_b = pk.vec(p + ".attn.norm.bias");
            b.qkv = pk.linear(p + ".attn.qkv");
            b.proj = pk.linear(p + ".attn.proj");
            b.bias = pk.attention_bias(p + ".attn.attention_biases_indexed", L.window_size * L.window_size, L.num_heads);
            if (b.qkv.n_real != 3 * L.embed_dim || b.qkv.k_real != L.embed_dim || L.embed_dim != 32 * L.num_heads)
                throw except("mobile-sam: %s.attn.qkv is %d x %d (this backend implements head_dim 32)", p.c_str(), b.qkv.n_real, b.qkv.k_real);
            b.local_conv = pk.depthwise(p + ".local_conv.c");
            b.mlp_ln_w = pk.vec(p + ".mlp.norm.weight");
            b.mlp_ln_b = pk.vec(p + ".mlp.norm.bias");
            b.fc1 = pk.linear(p + ".mlp.fc1");
            b.fc2 = pk.linear(p + ".mlp.fc2");
            Wt.blocks[l].push_back(b);
        }
        if (L.downsample) Wt.merge[l] = merge(e + "layers." + std::to_string(l) + ".downsample");
    }
    Wt.neck0 = pk.conv(e + "neck.0");
    Wt.neck1_w = pk.vec(e + "neck.1.weight");
    Wt.neck1_b = pk.vec(e + "neck.1.bias");
    Wt.neck2 = pk.conv(e + "neck.2");
    Wt.neck3_w = pk.vec(e + "neck.3.weight");
    Wt.neck3_b = pk.vec(e + "neck.3.bias");

    if (file.find("dec.iou_token.weight")) { // prompt encoder + mask decoder (mobile-sam.cpp:207-483)
        samdec_weights& D = model->dec;
        D.present = true;
        const int dim = D.dim;
        D.res = P.layers[3].resolution;
        D.gaussian = pk.host_vec("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", dim);
        for (int i = 0; i < 4; ++i) D.point_embed[i] = pk.host_vec("prompt_encoder.point_embeddings." + std::to_string(i) + ".weight", dim);
        D.not_a_point = pk.host_vec("prompt_encoder.not_a_point_embed.weight", dim);
        D.output_tokens = pk.host_vec("dec.iou_token.weight", dim);
        std::vector<float> mt = pk.host_vec("dec.mask_tokens.weight", 4 * dim);
        D.output_tokens.insert(D.output_tokens.end(), mt.begin(), mt.end());
        D.no_mask = pk.f16_vec("prompt_encoder.no_mask_embed.weight", dim);
        D.dense_pe = pk.f16_vec("dec.dense_positional_embedding", (int64_t)D.res * D.res * dim);
        auto attn = [&](std::string const& p) {
            sam_attn_weights a;
            a.q = pk.linear(p + ".q_proj");
            a.k = pk.linear(p + ".k_proj");
            a.v = pk.linear(p + ".v_proj");
            a.o = pk.linear(p + ".out_proj");
            if (a.q.k_real != dim || a.o.n_real != dim || a.q.n_real % D.heads || a.q.n_real / D.heads > 32)
                throw except("mobile-sam: %s has an unsupported shape (%d -> %d)", p.c_str(), a.q.k_real, a.q.n_real);
            return a;
        };
        for (int i = 0; i < 2; ++i) {
            std::string p = "dec.transformer.layers." + std::to_string(i);
            sam_twoway_weights L;
            L.self_attn = attn(p + ".self_attn");
            L.t2i = attn(p + ".cross_attn_t2i");
            L.i2t = attn(p + ".cross_attn_i2t");
            L.lin1 = pk.linear(p + ".mlp.lin1");
            L.lin2 = pk.linear(p + ".mlp.lin2");
            for (int n = 0; n < 4; ++n) {
                L.norm_w[n] = pk.vec(p + ".norm" + std::to_string(n + 1) + ".weight");
                L.norm_b[n] = pk.vec(p + ".norm" + std::to_string(n + 1) + ".bias");
            }
            D.layers.push_back(L);
        }
        D.final_attn = attn("dec.transformer.final_attn_t2i");
        D.final_norm_w = pk.vec("dec.transformer.norm_final_attn.weight");
        D.final_norm_b = pk.vec("dec.transformer.norm_final_attn.bias");
        D.up0 = pk.conv_transpose("dec.output_upscaling.0", 2, &D.up_c1);
        D.up_norm_w = pk.vec("dec.output_upscaling.1.weight");
        D.up_norm_b = pk.vec("dec.output_upscaling.1.bias");
        D.up3 = pk.conv_transpose("dec.output_upscaling.3", 2, &D.up_c2);
        if (D.up_c1 % 8 || D.up_c2 % 8 || D.up_c2 > 64) throw except("mobile-sam: upscaling widths %d / %d are not supported", D.up_c1, D.up_c2);
        for (int i = 0; i < 4; ++i)
            for (int l = 0; l < 3; ++l) D.hyper[i][l] = pk.linear("dec.output_hypernetworks_mlps." + std::to_string(i) + ".layers." + std::to_string(l));
        for (int l = 0; l < 3; ++l) D.iou_head[l] = pk.linear("dec.iou_prediction_head.layers." + std::to_string(l));
        if (D.hyper[0][2].n_real != D.up_c2 || D.iou_head[2].n_real != 4) throw except("mobile-sam: hypernetwork / iou head output widths do not match");
        D.tables_off = ab.alloc((size_t)11 * dim * 4);
        if (with_data) {
            float* tb = reinterpret_cast<float*>(ab.data.data() + D.tables_off);
            memcpy(tb, D.gaussian.data(), (size_t)dim * 4);
            for (int i = 0; i < 4; ++i) memcpy(tb + (size_t)(1 + i) * dim, D.point_embed[i].data(), (size_t)dim * 4);
            memcpy(tb + (size_t)5 * dim, D.not_a_point.data(), (size_t)dim * 4);
            memcpy(tb + (size_t)6 * dim, D.output_tokens.data(), (size_t)5 * dim * 4);
        }
    }

    device_turn turn(dev);
    model->weight_arena = upload_arena(ab.data, dev.stream, with_data);
    if (with_data) sam_weights_ready(*model);
    return model.release();
}

// The arena is complete (uploaded here, or received from the rank that read the file): rebuild everything the host computes
// with from it -- the prompt encoder's tables -- and the device's f32 copy of the iou head (vision.cpp:80-82 picks a mask by its output).
void sam_weights_ready(sam_model& m) {
    samdec_weights& D = m.dec;
    if (D.present) {
        device_turn turn(*m.backend);
        void* s = m.backend->stream;
        const uint8_t* wa = static_cast<const uint8_t*>(m.weight_arena.ptr);
        const int dim = D.dim;
        std::vector<float> tb((size_t)11 * dim);
        VX(vx_memcpy_d2h(tb.data(), wa + D.tables_off, tb.size() * 4, s));
        D.gaussian.assign(tb.begin(), tb.begin() + dim);
        for (int i = 0; i < 4; ++i) D.point_embed[i].assign(tb.begin() + (size_t)(1 + i) * dim, tb.begin() + (size_t)(2 + i) * dim);
        D.not_a_point.assign(tb.begin() + (size_t)5 * dim, tb.begin() + (size_t)6 * dim);
        D.output_tokens.assign(tb.begin() + (size_t)6 * dim, tb.end());
        std::vector<float> iou_w[3], iou_b[3]; // f32 copies [n][k] of the f16-rounded iou head weights, biases
        for (int l = 0; l < 3; ++l) {
            packed_gemm const& g = D.iou_head[l];
            std::vector<uint16_t> w16((size_t)g.N * g.K);
            VX(vx_memcpy_d2h(w16.data(), wa + g.w, w16.size() * 2, s));
            iou_w[l].resize((size_t)g.n_real * g.k_real);
            for (int n = 0; n < g.n_real; ++n)
                for (int k = 0; k < g.k_real; ++k) iou_w[l][(size_t)n * g.k_real + k] = f16_to_f32(w16[(size_t)n * g.K + k]);
            iou_b[l].assign((size_t)g.n_real, 0.0f);
            if (g.b != SIZE_MAX) VX(vx_memcpy_d2h(iou_b[l].data(), wa + g.b, (size_t)g.n_real * 4, s));
        }
        VX(vx_stream_sync(s));
        // those f32 values on the device for vx_sam_iou_head_f32 (the decoder ranks the masks there): [w0 | b0 | w1 | b1 | w2 | b2]
        workspace_layout lay;
        for (int l = 0; l < 3; ++l) {
            m.iou_head_off[2 * l] = lay.take(iou_w[l].size() * 4);
            m.iou_head_off[2 * l + 1] = lay.take(iou_b[l].size() * 4);
        }
        m.iou_head_dev = device_buffer(lay.top);
        uint8_t* base = static_cast<uint8_t*>(m.iou_head_dev.ptr);
        for (int l = 0; l < 3; ++l) {
            VX(vx_memcpy_h2d(base + m.iou_head_off[2 * l], iou_w[l].data(), iou_w[l].size() * 4, s));
            VX(vx_memcpy_h2d(base + m.iou_head_off[2 * l + 1], iou_b[l].data(), iou_b[l].size() * 4, s));
        }
        VX(vx_stream_sync(s));
    }
    m.weights_uploaded = true;
}

sam_model::~sam_model() {
    if (!prompt_tokens_host && !prompt_tokens_event) return;
    try {
        device_turn turn(*backend);
        if (prompt_tokens_event) {
            vx_event_sync(prompt_tokens_event);
            vx_event_destroy(prompt_tokens_event);
        }
        if (prompt_tokens_host) vx_free_host(prompt_tokens_host);
    } catch (...) {
    }
}

// e4m3 images of the stage MLPs' weights: read back from the packed f16 arena (what is on every rank), quantised on the host per output channel
void sam_set_fp8_mlp(sam_model& m, bool enable) {
    if (!enable || m.fp8_arena.ptr) { m.fp8_mlp = enable; return; }
    if (!m.weights_uploaded) throw except("sam: weights have not been uploaded");
    device_turn turn(*m.backend);
    std::vector<uint8_t> host;
    auto put = [&](size_t bytes) { const size_t off = (host.size() + 255) / 256 * 256; host.resize(off + bytes, 0); return off; };
    const uint8_t* wa = static_cast<const uint8_t*>(m.weight_arena.ptr);
    auto quantise = [&](packed_gemm const& g) {
        std::vector<uint16_t> h16((size_t)g.N * g.K);
        VX(vx_memcpy_d2h(h16.data(), wa + g.w, h16.size() * 2, m.backend->stream));
        std::vector<float> rows((size_t)g.n_real * g.k_real);
        for (int n = 0; n < g.n_real; ++n)
            for (int k = 0; k < g.k_real; ++k) rows[(size_t)n * g.k_real + k] = f16_to_f32(h16[(size_t)n * g.K + k]);
        fp8_linear f;
        f.N = (g.n_real + 127) / 128 * 128;
        f.Kp = (g.k_real + 127) / 128 * 128;
        f.w = put((size_t)f.N * f.Kp);
        f.s = put((size_t)f.N * 4);
        VX(vx_quantize_rows_e4m3_host(rows.data(), g.n_real, g.k_real, f.Kp, host.data() + f.w, reinterpret_cast<float*>(host.data() + f.s)));
        for (int n = g.n_real; n < f.N; ++n) reinterpret_cast<float*>(host.data() + f.s)[n] = 1.0f; // pad rows: zero bytes, any finite scale
        return f;
    };
    for (int l = 1; l < 4; ++l)
        for (tv_block_weights& b : m.weights.blocks[l]) {
            b.fc1_e4m3 = quantise(b.fc1);
            b.fc2_e4m3 = quantise(b.fc2);
        }
    m.fp8_arena = device_buffer(host.size());
    VX(vx_memcpy_h2d(m.fp8_arena.ptr, host.data(), host.size(), m.backend->stream));
    VX(vx_stream_sync(m.backend->stream));
    m.fp8_mlp = true;
}

void sam_encode_batch_device(sam_model& m, void const* rgb_dev, int B, void* out_dev, void* stream) {
    if (!m.weights_uploaded) throw except("sam: weights have not been uploaded (load_no_upload without weights_ready)");
    if (B < 1 || !rgb_dev || !out_dev) throw except("sam: empty batch or null pointer");
    device_turn turn(*m.backend);
    void* s = stream ? stream : m.backend->stream;
    tiny_vit_params const& P = m.params;
    tinyvit_weights const& Wt = m.weights;
    const int S = P.img_size;
    // scratch: three rotating activation buffers (largest map: 256 x 256 x 256 f16 of an MBConv) + input / patch-embed buffers
    const size_t big = (size_t)B * 256 * 256 * 256 * 2 + 4096;
    const size_t in_bytes = (size_t)B * S * S * 8 * 2 + 4096, pe_bytes = (size_t)B * (S / 2) * (S / 2) * 32 * 2 + 4096;
    const size_t need = 4 * big + in_bytes + pe_bytes;
    grow(m.ws, need, {m.backend->stream, s}, s); // zero-filled: GEMM rows are read up to K padded to 64, stale bytes must be finite (pads of W are 0)
    uint8_t* base = static_cast<uint8_t*>(m.ws.ptr);
    void* buf[4] = {base, base + big, base + 2 * big, base + 3 * big};
    void* in8 = base + 4 * big;
    void* pe = base + 4 * big + in_bytes;

    tv_exec ex(m, s, m.weight_arena.ptr);
    if (const char* e = getenv("VISP_TV_GEMM_VARIANT")) ex.gemm_variant = atoi(e);
    const bool fuse_mbconv = !getenv("VISP_TV_NO_FUSED_MBCONV");
    ex.mark("preprocess", 0, (double)B * S * S * 19);
    VX(vx_tv_preprocess(static_cast<const uint8_t*>(rgb_dev), in8, (int64_t)B * S * S, s));
    // patch_embed (mobile-sam.cpp:70-75)
    ex.conv(Wt.pe0, in8, B, S, S, 8, 3, 2, 1, pe, VX_EPI_F16_GELU, "patch_embed");
    void *x = buf[0], *t1 = buf[1], *t2 = buf[2], *t3 = buf[3];
    ex.conv(Wt.pe2, pe, B, S / 2, S / 2, Wt.pe0.n_real, 3, 2, 1, x, VX_EPI_F16, "patch_embed");
    int res = P.layers[0].resolution, C = P.layers[0].embed_dim;
    ex.capture("patch_embed", x, B, res, C);
    // conv_layer (mobile-sam.cpp:162-170): mb_conv x depth
    for (tv_mbconv_weights const& mb : Wt.mbconv) {
        const long M = (long)B * res * res;
        ex.gemm(mb.conv1, x, M, C, t1, VX_EPI_F16_GELU, nullptr, "mbconv_1x1");
        if (fuse_mbconv && mb.conv3_frag != SIZE_MAX && mb.conv3.b != SIZE_MAX && vx_mbconv_dw_pw_supported(mb.conv2.C, mb.conv3.n_real, res)) {
            // depthwise + GELU + conv3 + residual + GELU in one launch: the depthwise output stays in LDS (kernels_mbconv.hip)
            ex.mark("mbconv_dw_pw", 2.0 * M * (9.0 * mb.conv2.C + (double)mb.conv2.C * C), (double)M * (mb.conv2.C + 2.0 * C) * 2);
            VX(vx_mbconv_dw_pw_f16(t1, ex.wa + mb.conv2.w, reinterpret_cast<const float*>(ex.wa + mb.conv2.b), ex.wa + mb.conv3_frag,
                                   reinterpret_cast<const float*>(ex.wa + mb.conv3.b), x, t3, B, res, res, mb.conv2.C, C, s));
        } else {
            ex.dw(mb.conv2, t1, t2, B, res, res, 1, true, "depthwise_mbconv"); // the step's largest kernel: [B, 256, 256, 256] in and out
            ex.gemm(mb.conv3, t2, M, mb.conv1.n_real, t3, VX_EPI_F16_ADD, x, "mbconv_1x1", /*post_gelu=*/true); // gelu(x + conv3) in the epilogue
        }
        std::swap(x, t3);
    }
    auto patch_merging = [&](tv_merge_weights const& mg) { // mobile-sam.cpp:94-110
        const long M = (long)B * res * res;
        ex.gemm(mg.conv1, x, M, C, t1, VX_EPI_F16_GELU, nullptr, "merge_1x1");
        const int co = mg.conv1.n_real;
        ex.dw(mg.conv2, t1, t2, B, res, res, mg.stride, true, "depthwise");
        res = (res + 2 - 3) / mg.stride + 1;
        ex.gemm(mg.conv3, t2, (long)B * res * res, co, t1, VX_EPI_F16, nullptr, "merge_1x1");
        std::swap(x, t1);
        C = mg.conv3.n_real;
    };
    patch_merging(Wt.merge[0]);
    ex.capture("layer_0", x, B, res, C);
    for (int l = 1; l < 4; ++l) { // basic_layer (mobile-sam.cpp:172-186)
        tiny_vit_layer const& L = P.layers[l];
        if (res != L.resolution || C != L.embed_dim) throw except("sam: layer %d gets %dx%dx%d, expects %dx%d", l, res, res, C, L.resolution, L.embed_dim);
        const int ws = L.window_size, nw = (res + ws - 1) / ws, N = ws * ws;
        const long T = (long)B * res * res, rows = (long)B * nw * nw * N;
        for (tv_block_weights const& b : Wt.blocks[l]) { // tiny_vit_block (mobile-sam.cpp:133-160)
            ex.mark("layernorm", 0, (double)(T + rows) * C * 2);
            VX(vx_layernorm_f16(x, ex.vec(b.attn_ln_w), ex.vec(b.attn_ln_b), t1, rows, C, 1e-5f, res, ws, 0, s));
            ex.gemm(b.qkv, t1, rows, C, t2, VX_EPI_F16, nullptr, "gemm_qkv");
            ex.mark("window_attention", 4.0 * rows * N * C, (double)rows * C * 8);
            VX(vx_window_attention_f16(t2, ex.wa + b.bias.off, t1, (int)(rows / N), N, L.num_heads, s));
            // proj + window_reverse + residual: window rows are scattered to their pixels by the epilogue
            ex.gemm(b.proj, t1, rows, C, t2, VX_EPI_F16_ADD, x, "gemm_proj", false, ws, res);
            ex.dw(b.local_conv, t2, t3, B, res, res, 1, false, "depthwise");
            ex.mark("layernorm", 0, (double)T * C * 4);
            VX(vx_layernorm_f16(t3, ex.vec(b.mlp_ln_w), ex.vec(b.mlp_ln_b), t1, T, C, 1e-5f, 0, 0, 0, s));
            if (m.fp8_mlp) { // opt-in: both products on the e4m3 matrix instruction, activations quantised per token in between
                const int hid = b.fc1.n_real;
                ex.fp8_linear_launch(b.fc1_e4m3, b.fc1, t1, T, C, t2, hid, 1, nullptr, "gemm_fc1_e4m3");
                ex.fp8_linear_launch(b.fc2_e4m3, b.fc2, t2, T, hid, x, C, 0, t3, "gemm_fc2_e4m3");
            } else {
            ex.gemm(b.fc1, t1, T, C, t2, VX_EPI_F16_GELU, nullptr, "gemm_fc1");
            ex.gemm(b.fc2, t2, T, b.fc1.n_real, x, VX_EPI_F16_ADD, t3, "gemm_fc2");
            }
        }
        if (L.downsample) patch_merging(Wt.merge[l]);
        ex.capture(("layer_" + std::to_string(l)).c_str(), x, B, res, C);
    }
    // neck (mobile-sam.cpp:197-205): conv 1x1, LayerNorm over channels, conv 3x3, LayerNorm -> f32 [B, res, res, 256]
    const long T = (long)B * res * res;
    ex.gemm(Wt.neck0, x, T, C, t1, VX_EPI_F16, nullptr, "neck");
    const int NC = Wt.neck0.n_real;
    ex.mark("layernorm", 0, (double)T * NC * 4);
    VX(vx_layernorm_f16(t1, ex.vec(Wt.neck1_w), ex.vec(Wt.neck1_b), t2, T, NC, 1e-5f, 0, 0, 0, s));
    ex.conv(Wt.neck2, t2, B, res, res, NC, 3, 1, 1, t1, VX_EPI_F16, "neck");
    ex.mark("layernorm", 0, (double)T * NC * 6);
    VX(vx_layernorm_f16(t1, ex.vec(Wt.neck3_w), ex.vec(Wt.neck3_b), out_dev, T, Wt.neck2.n_real, 1e-5f, 0, 0, 1, s));
    ex.finish_timing();
    if (!stream) VX(vx_stream_sync(s));
}

void sam_encode_batch_host(sam_model& m, uint8_t const* rgb, int B, float* out) {
    if (B < 1 || !rgb || !out) throw except("sam: empty batch or null pointer");
    device_turn turn(*m.backend);
    const int S = m.params.img_size, R = m.params.layers[3].resolution;
    const size_t in_bytes = (size_t)B * S * S * 3, out_bytes = (size_t)B * R * R * 256 * 4;
    device_buffer din(in_bytes), dout(out_bytes);
    void* s = m.backend->stream;
    VX(vx_memcpy_h2d(din.ptr, rgb, in_bytes, s));
    sam_encode_batch_device(m, din.ptr, B, dout.ptr, s);
    VX(vx_memcpy_d2h(out, dout.ptr, out_bytes, s));
    VX(vx_stream_sync(s));
}

void sam_encode(sam_model& m, image_view image) {
    if (is_float(image.format) || n_channels(image.format) < 3)
        throw except("sam: unsupported input image format [%d], expected an 8-bit colour image", int(image.format));
    if (image.extent[0] < 1 || image.extent[1] < 1) throw except("sam: empty image");
    const int S = m.params.img_size;
    image_data rgb = image_to_rgb_u8(image);
    image_view v = view_of(rgb);
    image_data resized;
    // sam_process_input (mobile-sam.cpp:533-547): resize_longest_side, then u8 -> f32 with source coordinates clamped
    const float scale = float(S) / float(std::max(image.extent[0], image.extent[1]));
    if (scale != 1) {
        resized = image_scale(v, i32x2{{int(image.extent[0] * scale + 0.5f), int(image.extent[1] * scale + 0.5f)}});
        v = view_of(resized);
    }
    std::vector<uint8_t> square((size_t)S * S * 3);
    const uint8_t* src = static_cast<const uint8_t*>(v.data);
    const int vw = std::min(v.extent[0], S), vh = std::min(v.extent[1], S);
    for (int y = 0; y < S; ++y) { // clamped source coordinates = edge replication (image.cpp convert<>, :216-226)
        uint8_t* dst = &square[(size_t)y * S * 3];
        if (y < vh) {
            memcpy(dst, src + (size_t)y * v.stride, (size_t)vw * 3);
            for (int x = vw; x < S; ++x) memcpy(dst + (size_t)x * 3, dst + (size_t)(vw - 1) * 3, 3);
        } else {
            memcpy(dst, dst - (size_t)S * 3, (size_t)S * 3);
        }
    }
    device_turn turn(*m.backend);
    const int R = m.params.layers[3].resolution;
    const size_t out_bytes = (size_t)R * R * 256 * 4;
    if (!m.embed.ptr) m.embed = device_buffer(out_bytes + square.size()); // embedding + the staging copy of the input stay with the model
    void* din = static_cast<uint8_t*>(m.embed.ptr) + out_bytes;
    void* s = m.backend->stream;
    VX(vx_memcpy_h2d(din, square.data(), square.size(), s));
    sam_encode_batch_device(m, din, 1, m.embed.ptr, s);
    VX(vx_stream_sync(s));
    m.image_extent = image.extent;
}

} // namespace visp
