#include "tinyvit.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "../../include/visp_hip_kernels.h"
#include "packer.h"
#include "visp_util.h"

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

namespace {

struct tv_exec : model_pass<sam_model> {
    using model_pass::model_pass;
    int gemm_variant = 0; // vx_gemm_args.stages: tile-shape selector of the plain GEMM (0 = its default)

    // C[M, N] = A[M, lda] * W^T (+bias) with the epilogues of the GEMM family
    void gemm(packed_gemm const& g, const void* A, long M, int lda, void* out, int epi, const void* res1, const char* group,
              bool post_gelu = false, int win_ws = 0, int win_res = 0) {
        vx_gemm_args a = gemm_args(g, wa);
        a.A = A; a.lda = lda;
        a.M = (int)M;
        a.epi = epi; a.out = out; a.ldo = g.n_real; a.res1 = res1;
        a.stages = gemm_variant;
        a.post_gelu = post_gelu; a.win_ws = win_ws; a.win_res = win_res;
        mark(group, 2.0 * M * g.n_real * g.k_real, (double)M * (g.k_real + g.n_real) * 2);
        VX(vx_gemm_f16(&a, stream));
    }
    // k x k conv as implicit GEMM on NHWC f16
    void conv(packed_gemm const& g, const void* x, int B, int H, int W, int Cpix, int k, int stride, int pad, void* out, int epi, const char* group) {
        const int OH = (H + 2 * pad - k) / stride + 1, OW = (W + 2 * pad - k) / stride + 1;
        vx_gemm_args a = gemm_args(g, wa);
        a.A = x;
        a.conv_kh = a.conv_kw = k; a.conv_stride = stride; a.conv_pad = pad;
        a.conv_H = H; a.conv_W = W; a.conv_Cin = Cpix; a.conv_OH = OH; a.conv_OW = OW;
        a.M = B * OH * OW;
        a.epi = epi; a.out = out; a.ldo = g.n_real;
        mark(group, 2.0 * a.M * g.n_real * g.k_real, (double)B * H * W * Cpix * 2 + (double)a.M * g.n_real * 2);
        VX(vx_gemm_f16(&a, stream));
    }
    // out f16 [M, n_out] = act(A W^T + b) [+ res] with A f16 [M, k_in] quantised to e4m3 rows first (scratch: m.fp8_ws)
    void fp8_linear_launch(fp8_linear const& f, packed_gemm const& g, const void* A, long M, int k_in, void* out, int n_out, int act, const void* res, const char* group) {
        const size_t need = (size_t)M * f.Kp + (size_t)M * 4 + 512;
        grow(m.fp8_ws, need, {stream});
        uint8_t* q = static_cast<uint8_t*>(m.fp8_ws.ptr);
        float* qs = reinterpret_cast<float*>(q + ((size_t)M * f.Kp + 255) / 256 * 256);
        const uint8_t* fa = static_cast<const uint8_t*>(m.fp8_arena.ptr);
        mark("quantise_e4m3", 0, (double)M * k_in * 3);
        VX(vx_quantize_rows_e4m3(A, k_in, q, qs, (int)M, k_in, f.Kp, stream));
        vx_gemm_fp8_args a;
        memset(&a, 0, sizeof a);
        a.A = q; a.a_scale = qs; a.W = fa + f.w; a.w_scale = reinterpret_cast<const float*>(fa + f.s);
        a.bias = gemm_args(g, wa).bias;
        a.M = (int)M; a.N = f.N; a.Kp = f.Kp; a.n_valid = n_out; a.out = out; a.ldo = n_out; a.act = act; a.res = res;
        mark(group, 2.0 * M * g.n_real * g.k_real, (double)M * (g.k_real + 2.0 * g.n_real));
        VX(vx_gemm_fp8(&a, stream));
    }
    void capture(const char* name, const void* src, int B, int res, int C) { keep(name, src, {B, res, res, C}); }
    void dw(packed_dw const& d, const void* x, void* y, int B, int H, int W, int stride, bool gelu, const char* group) {
        mark(group, 2.0 * B * (H / stride) * (W / stride) * 9 * d.C, (double)B * H * W * d.C * 2 * (1.0 + 1.0 / (stride * stride)));
        VX(vx_dwconv3x3_f16(x, wa + d.w, reinterpret_cast<const float*>(wa + d.b), y, B, H, W, d.C, stride, gelu, stream));
    }
};

} // namespace

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

// ---- prompt encoder + mask decoder + mask post-processing: one schedule, the prompt index folded into the rows of its launches ---------
// (sam_compute is a batch of one prompt)

void sam_set_prompt_chunk(sam_model& m, int n) {
    if (n < 1 || n > 256) throw except("sam: prompt chunk %d is outside 1 .. 256", n);
    m.prompt_chunk = n;
}

namespace {

float sam_transform_coord(int p, float scale, int image_size) { // mobile-sam.cpp:213-217
    const float center_normalized = (float(p) * scale + 0.5f) / float(image_size);
    return 2.f * center_normalized - 1.f;
}

constexpr int kSamTokens = 7; // [iou | 4 mask tokens | 2 prompt points]

// prompt encoder on the host (two points of 256 sin/cos values; mobile-sam.cpp:219-286): the decoder's token rows of one prompt, f16 [7][dim]
void sam_prompt_tokens(sam_model const& m, int const* prompt, int n_prompt, uint16_t* out) {
    samdec_weights const& D = m.dec;
    const int dim = D.dim, F = dim / 2, image_size = m.params.img_size;
    const bool is_box = n_prompt == 4;
    const float scale = float(image_size) / float(std::max(m.image_extent[0], m.image_extent[1]));
    float coords[4] = {sam_transform_coord(prompt[0], scale, image_size), sam_transform_coord(prompt[1], scale, image_size), 0.f, 0.f};
    if (is_box) { coords[2] = sam_transform_coord(prompt[2], scale, image_size); coords[3] = sam_transform_coord(prompt[3], scale, image_size); }
    std::vector<float> tokens(D.output_tokens); // [iou | 4 mask tokens]
    tokens.resize((size_t)kSamTokens * dim);
    for (int i = 0; i < 2; ++i) {
        float* t = tokens.data() + (size_t)(5 + i) * dim;
        for (int f = 0; f < F; ++f) {
            float v = coords[2 * i] * D.gaussian[f] + coords[2 * i + 1] * D.gaussian[F + f];
            v *= 2.f * 3.14159265358979323846f;
            t[f] = std::sin(v);
            t[F + f] = std::cos(v);
        }
        if (is_box) for (int c = 0; c < dim; ++c) t[c] += D.point_embed[2 + i][c];
        else if (i == 0) for (int c = 0; c < dim; ++c) t[c] += D.point_embed[1][c];
        else for (int c = 0; c < dim; ++c) t[c] = D.not_a_point[c];
    }
    for (size_t i = 0; i < tokens.size(); ++i) out[i] = f32_to_f16(tokens[i]);
}

void sam_require_decoder(sam_model const& m) {
    samdec_weights const& D = m.dec;
    if (!D.present) throw except("sam: this model file holds no prompt encoder / mask decoder (dec.* tensors)");
    if (D.gaussian.empty()) throw except("sam: the decoder's host tables were not read (model loaded without data)");
    if (!m.embed.ptr || m.image_extent[0] <= 0) throw except("Missing image embeds, call sam_encode() first");
}

// what the launches behind a chunk's mask product need of the decode: the stream, the maps the masks pass through and the extents
struct sam_decode_ctx {
    void* s = nullptr;
    float* scaled = nullptr; // f32 [Bmax][image_size^2]
    int Bmax = 0, image_size = 0, mask_size = 0, sw = 0, sh = 0;
    int64_t n_px = 0;
    i32x2 target = {{0, 0}};
};

// The decoder, which sam_compute, sam_compute_batch_* and sam_generate_masks_* all run: the prompt tokens of the call, layer 0's shared image side, then per
// chunk the decoder, the mask product and the iou head. The logits of a chunk go to the chunk buffer of the workspace, or, with logits_all, to
// [p0 ..] of a buffer that keeps the planes of every prompt; after_chunk(ctx, p0, B, logits, iou, chosen) launches what follows them. With captures on,
// `kept` receives the logits and iou predictions of every prompt (a synchronisation per chunk); with captures off it is emptied.
template <class F>
sam_decode_ctx sam_decode_prompts(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, void* logits_all, void* iou_dev, void* chosen_dev, void* stream,
                                  sam_kept_logits& kept, F&& after_chunk) {
    samdec_weights const& D = m.dec;
    if (n < 1) throw except("sam: empty batch of prompts (n = %d)", n);
    for (int i = 0; i < n; ++i)
        if (n_args[i] != 2 && n_args[i] != 4) throw except("sam: bad number of arguments (%d) for prompt %d, must be 2 or 4", n_args[i], i);
    sam_require_decoder(m);
    if (!m.iou_head_dev.ptr) throw except("sam: weights have not been uploaded (load_no_upload without weights_ready)");
    device_turn turn(*m.backend);
    void* s = stream ? stream : m.backend->stream;
    const int dim = D.dim, H = D.heads, res = D.res, Nk = res * res, Nt = kSamTokens;
    const int image_size = m.params.img_size, mask_size = 4 * res;
    const int64_t n_px = (int64_t)mask_size * mask_size;
    const int Bmax = std::min(n, m.prompt_chunk);
    sam_twoway_weights const& L0 = D.layers.at(0);
    const int ci = L0.t2i.q.n_real, cs = L0.self_attn.q.n_real; // widths inside the cross and the self attention
    const int hd_c = ci / H, hd_s = cs / H;
    auto built = [](int hd) { return hd == 16 || hd == 32 || hd == 64; };
    if (!built(hd_c) || !built(hd_s)) throw except("sam: the batched decoder is built for attention head widths 16, 32 and 64 (got %d and %d)", hd_s, hd_c);
    for (sam_twoway_weights const& L : D.layers)
        if (L.t2i.q.n_real != ci || L.i2t.q.n_real != ci || L.self_attn.q.n_real != cs) throw except("sam: the decoder layers differ in their attention widths");
    if (D.final_attn.q.n_real != ci) throw except("sam: the final attention's width differs from the layers'");
    int tok_w = std::max({dim, cs, ci}), hyp_w = 0, mlp_w = 0;
    for (sam_twoway_weights const& L : D.layers) mlp_w = std::max(mlp_w, L.lin1.n_real);
    for (int i = 0; i < 4; ++i) hyp_w = std::max({hyp_w, D.hyper[i][0].n_real, D.hyper[i][1].n_real});

    // ---- the prompt tokens of the whole call, encoded on the host into pinned memory and uploaded once
    const size_t tok_bytes = (size_t)n * Nt * dim * 2;
    if (m.prompt_tokens_event) VX(vx_event_sync(m.prompt_tokens_event)); // the previous call's upload has read them (long done in practice)
    else VX(vx_event_create(&m.prompt_tokens_event));
    if (m.prompt_tokens_bytes < tok_bytes) {
        if (m.prompt_tokens_host) VX(vx_free_host(m.prompt_tokens_host));
        m.prompt_tokens_host = nullptr;
        m.prompt_tokens_bytes = 0;
        VX(vx_malloc_host(&m.prompt_tokens_host, tok_bytes));
        m.prompt_tokens_bytes = tok_bytes;
    }
    uint16_t* tok_host = static_cast<uint16_t*>(m.prompt_tokens_host);
    for (int i = 0; i < n; ++i) sam_prompt_tokens(m, prompts + (size_t)i * 4, n_args[i], tok_host + (size_t)i * Nt * dim);

    // ---- workspace: what every prompt shares, then the buffers of one chunk of Bmax prompts (f16 unless said otherwise)
    const size_t R = (size_t)Bmax * Nt, big = (size_t)Bmax * Nk;
    workspace_layout layout;
    auto take = [&](size_t elems) { return layout.take(elems * 2, 256); };
    const size_t o_tok = take((size_t)n * Nt * dim);
    const size_t o_K0 = take((size_t)Nk * dim), o_k10 = take((size_t)Nk * dim), o_pk0 = take((size_t)Nk * ci), o_pv0 = take((size_t)Nk * ci), o_pq0 = take((size_t)Nk * ci);
    const size_t o_Q = take(R * dim), o_t1 = take(R * dim), o_t2 = take(R * dim), o_h = take(R * mlp_w + 64);
    const size_t o_tq = take(R * tok_w), o_tk = take(R * tok_w), o_tv = take(R * tok_w), o_ta = take(R * tok_w);
    const size_t o_K = take(big * dim), o_k1 = take(big * dim), o_k2 = take(big * dim);
    const size_t o_pq = take(big * ci), o_pk = take(big * ci), o_pv = take(big * ci), o_ao = take(big * ci);
    const size_t o_u1 = take(4 * big * D.up_c1), o_u1n = take(4 * big * D.up_c1), o_u2p = take(16 * big * D.up_c2), o_u2 = take(16 * big * D.up_c2 + 64);
    const size_t o_ha = take((size_t)Bmax * hyp_w + 64), o_hb = take((size_t)Bmax * hyp_w + 64), o_hy = take((size_t)Bmax * 4 * D.up_c2 + 64);
    const size_t o_mask = take((size_t)Bmax * 4 * n_px);
    const size_t o_iou = layout.take((size_t)Bmax * 4 * 4, 256), o_chosen = layout.take((size_t)Bmax * 4, 256);
    const size_t o_scaled = layout.take((size_t)Bmax * image_size * image_size * 4, 256);
    const size_t part_bytes = std::max(vx_attention_cross_partial_bytes(Bmax, H, Nt, Nk, hd_c), vx_attention_cross_partial_bytes(1, H, (int)R, Nk, hd_c));
    const size_t o_part = layout.take(part_bytes, 256);
    grow(m.batch_ws, layout.top, {m.backend->stream, s}, s); // zero-filled: GEMM rows are read up to K padded to 64, stale bytes must be finite
    uint8_t* base = static_cast<uint8_t*>(m.batch_ws.ptr);
    auto P = [&](size_t off) { return static_cast<void*>(base + off); };
    void *tok_all = P(o_tok), *K0 = P(o_K0), *k10 = P(o_k10), *pk0 = P(o_pk0), *pv0 = P(o_pv0), *pq0 = P(o_pq0);
    void *Q = P(o_Q), *t1 = P(o_t1), *t2 = P(o_t2), *hbuf = P(o_h), *tq = P(o_tq), *tk = P(o_tk), *tv = P(o_tv), *ta = P(o_ta);
    void *K = P(o_K), *k1 = P(o_k1), *k2 = P(o_k2), *pq = P(o_pq), *pk = P(o_pk), *pv = P(o_pv), *ao = P(o_ao);
    void *u1 = P(o_u1), *u1n = P(o_u1n), *u2p = P(o_u2p), *u2 = P(o_u2), *ha = P(o_ha), *hb = P(o_hb), *hy = P(o_hy), *masks_d = P(o_mask);
    void *iou_ws = P(o_iou), *chosen_ws = P(o_chosen), *scaled = P(o_scaled), *part = part_bytes ? P(o_part) : nullptr;

    tv_exec ex(m, s, m.weight_arena.ptr);
    const bool timing = m.timing;
    m.timing = false; // the per-group table belongs to the encoder
    struct restore_timing { sam_model& m; bool v; ~restore_timing() { m.timing = v; } } restore{m, timing};
    const uint8_t* wa = ex.wa;
    VX(vx_memcpy_h2d_async(tok_all, tok_host, tok_bytes, s));
    VX(vx_event_record(m.prompt_tokens_event, s));

    auto linear = [&](packed_gemm const& g, const void* A, long M, void* out, int epi = VX_EPI_F16, const void* res1 = nullptr) {
        ex.gemm(g, A, M, g.k_real, out, epi, res1, "decoder");
    };
    auto norm = [&](packed_vec const& w, packed_vec const& b, const void* x, void* y, long rows, int C) {
        VX(vx_layernorm_f16(x, ex.vec(w), ex.vec(b), y, rows, C, 1e-5f, 0, 0, 0, s));
    };
    auto add = [&](const void* a, const void* b, void* y, long n_el) { VX(vx_add_rows_f16(a, 0, b, n_el, y, n_el, s)); };
    auto cross = [&](const void* q, const void* k, const void* v, void* out, int Bt, int Tq, int Tk, int hd) {
        VX(vx_attention_cross_f16(q, k, v, out, part, part_bytes, Bt, H, Tq, Tk, hd, 1.0f / std::sqrt((float)hd), s));
    };
    const void* KPE = wa + D.dense_pe.off;

    // ---- layer 0's image side is the same for every prompt (the dense prompt is no_mask_embed for all): once per call
    // src = image_embeddings + dense prompt (mobile-sam.cpp:437-440), keys + key_pe, t2i's k_proj / v_proj and i2t's q_proj of them
    VX(vx_add_rows_f16(m.embed.ptr, 1, wa + D.no_mask.off, dim, K0, (int64_t)Nk * dim, s));
    add(K0, KPE, k10, (long)Nk * dim);
    linear(L0.t2i.k, k10, Nk, pk0);
    linear(L0.t2i.v, K0, Nk, pv0);
    linear(L0.i2t.q, k10, Nk, pq0);

    const i32x2 target = m.image_extent;
    const float up = float(image_size) / float(std::max(target[0], target[1]));
    const int sw = int(target[0] * up + 0.5f), sh = int(target[1] * up + 0.5f);
    kept.masks.assign(m.captures ? (size_t)n * 4 * n_px : 0, 0.0f);
    kept.iou.assign(m.captures ? (size_t)n * 4 : 0, 0.0f);

    sam_decode_ctx ctx;
    ctx.s = s; ctx.scaled = static_cast<float*>(scaled); ctx.Bmax = Bmax; ctx.image_size = image_size; ctx.mask_size = mask_size; ctx.sw = sw; ctx.sh = sh;
    ctx.n_px = n_px; ctx.target = target;
    for (int p0 = 0; p0 < n; p0 += Bmax) {
        const int B = std::min(Bmax, n - p0); // every launch below covers rows of these B prompts only: a short last chunk reads no rows behind them
        const long Rt = (long)B * Nt, Mi = (long)B * Nk;
        const void* T = static_cast<const uint8_t*>(tok_all) + (size_t)p0 * Nt * dim * 2;
        VX(vx_memcpy_d2d(Q, T, (size_t)Rt * dim * 2, s));
        // token-side attention: B prompts x 7 queries; the image side is [B][Nk] rows, or the shared layer-0 operands with all 7 B queries in one batch
        auto token_attention = [&](sam_attn_weights const& w, const void* q, const void* k_img, const void* v_img, bool shared, const void* res1) {
            linear(w.q, q, Rt, tq);
            if (shared) cross(tq, pk0, pv0, ta, 1, (int)Rt, Nk, hd_c); // queries are independent in a softmax
            else {
                linear(w.k, k_img, Mi, pk);
                linear(w.v, v_img, Mi, pv);
                cross(tq, pk, pv, ta, B, Nt, Nk, hd_c);
            }
            linear(w.o, ta, Rt, t2, VX_EPI_F16_ADD, res1);
        };
        for (size_t li = 0; li < D.layers.size(); ++li) { // two_way_attention_block (mobile-sam.cpp:322-364)
            sam_twoway_weights const& L = D.layers[li];
            const void* sq = Q; // skip_first_layer_pe: queries = self_attn(queries)
            if (li > 0) { add(Q, T, t1, Rt * dim); sq = t1; }
            linear(L.self_attn.q, sq, Rt, tq);
            linear(L.self_attn.k, sq, Rt, tk);
            linear(L.self_attn.v, Q, Rt, tv);
            cross(tq, tk, tv, ta, B, Nt, Nt, hd_s);
            linear(L.self_attn.o, ta, Rt, t2, li > 0 ? VX_EPI_F16_ADD : VX_EPI_F16, li > 0 ? Q : nullptr);
            norm(L.norm_w[0], L.norm_b[0], t2, Q, Rt, dim);
            add(Q, T, t1, Rt * dim); // tokens attending to the image embedding
            if (li > 0) VX(vx_add_rows_f16(K, 0, KPE, (int64_t)Nk * dim, k1, (int64_t)Mi * dim, s));
            token_attention(L.t2i, t1, k1, K, li == 0, Q);
            norm(L.norm_w[1], L.norm_b[1], t2, Q, Rt, dim);
            linear(L.lin1, Q, Rt, hbuf, VX_EPI_F16_RELU); // mlp_block
            linear(L.lin2, hbuf, Rt, t2, VX_EPI_F16_ADD, Q);
            norm(L.norm_w[2], L.norm_b[2], t2, Q, Rt, dim);
            add(Q, T, t1, Rt * dim); // image embedding attending to the tokens (k1 = keys + key_pe from above)
            if (li == 0) { // the shared rows laid out per prompt: from here on the keys differ
                VX(vx_sam_tile_rows_f16(pq0, (int64_t)Nk * ci, pq, B, s));
                VX(vx_sam_tile_rows_f16(K0, (int64_t)Nk * dim, K, B, s));
            } else {
                linear(L.i2t.q, k1, Mi, pq);
            }
            linear(L.i2t.k, t1, Rt, tk);
            linear(L.i2t.v, Q, Rt, tv);
            cross(pq, tk, tv, ao, B, Nk, Nt, hd_c);
            linear(L.i2t.o, ao, Mi, k2, VX_EPI_F16_ADD, K);
            norm(L.norm_w[3], L.norm_b[3], k2, K, Mi, dim);
        }
        add(Q, T, t1, Rt * dim); // final attention from the points to the image (mobile-sam.cpp:386-392)
        VX(vx_add_rows_f16(K, 0, KPE, (int64_t)Nk * dim, k1, (int64_t)Mi * dim, s));
        token_attention(D.final_attn, t1, k1, K, false, Q);
        norm(D.final_norm_w, D.final_norm_b, t2, Q, Rt, dim);

        // upscale_outputs (mobile-sam.cpp:396-404): convT k2 s2 -> LayerNorm -> GELU -> convT k2 s2 -> GELU, the prompt as the maps' batch
        auto conv_transpose = [&](packed_gemm const& g, const void* x, int hw, int cin, int cout, void* out) {
            vx_gemm_args a = gemm_args(g, wa);
            a.A = x; a.lda = cin;
            a.M = B * hw * hw;
            a.epi = VX_EPI_PIXSHUF; a.out = out; a.ldo = cout;
            a.ps_s = 2; a.ps_Cout = cout; a.ps_H = hw; a.ps_W = hw;
            VX(vx_gemm_f16(&a, s));
        };
        conv_transpose(D.up0, K, res, dim, D.up_c1, u1);
        norm(D.up_norm_w, D.up_norm_b, u1, u1n, 4 * Mi, D.up_c1);
        VX(vx_add_gelu_f16(u1n, nullptr, u1, (int64_t)4 * Mi * D.up_c1, s));
        conv_transpose(D.up3, u1, 2 * res, D.up_c1, D.up_c2, u2p);
        VX(vx_add_gelu_f16(u2p, nullptr, u2, (int64_t)16 * Mi * D.up_c2, s));

        // hypernetwork MLPs: mask token i of every prompt is one row of an M = B product -> hyper_in [B][4][up_c2]
        for (int i = 0; i < 4; ++i) {
            const uint8_t* tok_i = static_cast<const uint8_t*>(Q) + (size_t)(1 + i) * dim * 2;
            ex.gemm(D.hyper[i][0], tok_i, B, Nt * dim, ha, VX_EPI_F16_RELU, nullptr, "decoder");
            linear(D.hyper[i][1], ha, B, hb, VX_EPI_F16_RELU);
            vx_gemm_args a = gemm_args(D.hyper[i][2], wa);
            a.A = hb; a.lda = D.hyper[i][2].k_real; a.M = B;
            a.epi = VX_EPI_F16; a.out = static_cast<uint8_t*>(hy) + (size_t)i * D.up_c2 * 2; a.ldo = 4 * D.up_c2;
            VX(vx_gemm_f16(&a, s));
        }
        // masks[b][i][pixel] = <upscaled[b][pixel], hyper_in[b][i]> (mobile-sam.cpp:472-473): four planes of 16 Nk logits per prompt
        void* logits = logits_all ? static_cast<uint8_t*>(logits_all) + (size_t)p0 * 4 * n_px * 2 : masks_d;
        VX(vx_mul_mat_f16(u2, hy, logits, 16 * (int64_t)Nk, 4, D.up_c2, B, B, s));
        // iou prediction head on the iou token (row 0 of each prompt's seven; mobile-sam.cpp:476-481), and the choice among the first three (vision.cpp:80-82).
        // Three small linears on ONE token whose output decides which mask is returned, so they run in f32 from the token's values: an f16 pipeline
        // (ulp 5e-4 near 1) can flip the choice between near-tied predictions and return an entirely different mask
        float* iou_out = iou_dev ? static_cast<float*>(iou_dev) + (size_t)p0 * 4 : static_cast<float*>(iou_ws);
        int32_t* chosen_out = chosen_dev ? static_cast<int32_t*>(chosen_dev) + p0 : static_cast<int32_t*>(chosen_ws);
        const uint8_t* ih = static_cast<const uint8_t*>(m.iou_head_dev.ptr);
        auto ihp = [&](int i) { return reinterpret_cast<const float*>(ih + m.iou_head_off[i]); };
        VX(vx_sam_iou_head_f32(Q, (int64_t)Nt * dim, B, ihp(0), ihp(1), ihp(2), ihp(3), ihp(4), ihp(5), D.iou_head[0].k_real, D.iou_head[0].n_real, D.iou_head[1].n_real,
                               D.iou_head[2].n_real, iou_out, chosen_out, s));
        after_chunk(ctx, p0, B, logits, iou_out, chosen_out);
        if (m.captures) { // test hook: the four logit planes (f16-rounded) and the iou predictions of every prompt
            std::vector<uint16_t> mh((size_t)B * 4 * n_px);
            VX(vx_memcpy_d2h(mh.data(), logits, mh.size() * 2, s));
            VX(vx_memcpy_d2h(kept.iou.data() + (size_t)p0 * 4, iou_out, (size_t)B * 16, s));
            VX(vx_stream_sync(s));
            float* dst = kept.masks.data() + (size_t)p0 * 4 * n_px;
            for (size_t i = 0; i < mh.size(); ++i) dst[i] = f16_to_f32(mh[i]);
        }
    }
    return ctx;
}

// the decode with sam_process_mask (mobile-sam.cpp:556-583) on each prompt's chosen plane: masks u8 [n][h][w], iou, chosen on the device
void sam_decode_masks(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, void* masks_u8_dev, void* iou_dev, void* chosen_dev, void* stream,
                      sam_kept_logits& kept) {
    device_turn turn(*m.backend);
    const size_t out_px = (size_t)m.image_extent[0] * m.image_extent[1];
    sam_decode_ctx ctx = sam_decode_prompts(m, prompts, n_args, n, nullptr, iou_dev, chosen_dev, stream, kept,
                                            [&](sam_decode_ctx const& c, int p0, int B, void* logits, float*, int32_t* chosen) {
        VX(vx_sam_process_masks(logits, 4 * c.n_px, c.n_px, 1, c.mask_size, 4, chosen, c.scaled, c.image_size, c.sw, c.sh,
                                static_cast<uint8_t*>(masks_u8_dev) + (size_t)p0 * out_px, c.target[0], c.target[1], B, c.s));
    });
    if (!stream) VX(vx_stream_sync(ctx.s));
}

// The host entries (their callers have checked the decoder and n): masks, iou and chosen into `stage` on the device's stream, then what the caller asked for
// to the host. `stage` grows to what the call needs; every use of it ends synchronised, so nothing in flight holds it.
void sam_decode_masks_to_host(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, uint8_t* masks_u8, float* iou, int32_t* chosen, device_buffer& stage,
                              sam_kept_logits& kept) {
    device_turn turn(*m.backend);
    void* s = m.backend->stream;
    const size_t mask_bytes = (size_t)n * m.image_extent[0] * m.image_extent[1];
    workspace_layout lay;
    const size_t o_m = lay.take(mask_bytes), o_i = lay.take((size_t)n * 16), o_c = lay.take((size_t)n * 4);
    grow(stage, lay.top, {});
    uint8_t* base = static_cast<uint8_t*>(stage.ptr);
    sam_decode_masks(m, prompts, n_args, n, base + o_m, base + o_i, base + o_c, s, kept);
    VX(vx_memcpy_d2h(masks_u8, base + o_m, mask_bytes, s)); // waits for the stream
    if (iou) VX(vx_memcpy_d2h(iou, base + o_i, (size_t)n * 16, s));
    if (chosen) VX(vx_memcpy_d2h(chosen, base + o_c, (size_t)n * 4, s));
}

} // namespace

image_data sam_compute(sam_model& m, int const* prompt, int n_prompt) {
    if (n_prompt != 2 && n_prompt != 4) throw except("sam: bad number of arguments (%d), must be 2 or 4", n_prompt);
    sam_require_decoder(m);
    const int32_t args[4] = {prompt[0], prompt[1], n_prompt == 4 ? prompt[2] : 0, n_prompt == 4 ? prompt[3] : 0}, n_args = n_prompt;
    image_data out = image_alloc(m.image_extent, image_format::alpha_u8);
    sam_decode_masks_to_host(m, args, &n_args, 1, out.data.get(), nullptr, nullptr, m.single_out, m.last_single); // the device side of the mask stays with the model
    return out;
}

void sam_compute_batch_device(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, void* masks_u8_dev, void* iou_dev, void* chosen_dev, void* stream) {
    if (!prompts || !n_args || !masks_u8_dev) throw except("sam: null argument");
    sam_decode_masks(m, prompts, n_args, n, masks_u8_dev, iou_dev, chosen_dev, stream, m.last_batch);
}

void sam_compute_batch_host(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, uint8_t* masks_u8, float* iou, int32_t* chosen) {
    if (!prompts || !n_args || !masks_u8) throw except("sam: null argument");
    if (n < 1) throw except("sam: empty batch of prompts (n = %d)", n);
    sam_require_decoder(m);
    device_buffer stage; // of this call
    sam_decode_masks_to_host(m, prompts, n_args, n, masks_u8, iou, chosen, stage, m.last_batch);
}

// ---- automatic mask generation: the batched decode with every prompt's planes kept, scored per chunk, then rank + NMS and the masks that survive ------

void sam_generate_check_args(int32_t const* prompts, int32_t const* n_args, int n, float pred_iou_thresh, float stability_thresh, float stability_offset,
                             float nms_iou_thresh, int capacity) {
    if (!prompts || !n_args) throw except("sam: null argument");
    if (n < 1) throw except("sam: empty batch of prompts (n = %d)", n);
    if (n > kSamGenerateMaxPrompts)
        throw except("sam: %d prompts in one generate call, at most %d (three candidates each, 16384 candidates per call)", n, kSamGenerateMaxPrompts);
    if (std::isnan(pred_iou_thresh) || std::isnan(stability_thresh) || std::isnan(stability_offset) || std::isnan(nms_iou_thresh)) throw except("sam: a threshold is NaN");
    if (nms_iou_thresh < 0.0f || nms_iou_thresh > 1.0f) throw except("sam: nms_iou_thresh %g is outside [0, 1]", (double)nms_iou_thresh);
    if (stability_offset < 0.0f) throw except("sam: stability_offset %g is below 0", (double)stability_offset);
    if (capacity < 1) throw except("sam: capacity %d is below 1", capacity);
}

void sam_generate_check_region_area(int min_region_area) {
    if (min_region_area < 0) throw except("sam: min_region_area %d is below 0", min_region_area);
}

// masks in flight through the labelling workspace of the cleaning stage: labels and areas, 8 bytes per pixel each (512 MB at 1024^2)
constexpr int kSamCleanGroup = 64;

void sam_generate_masks_clean_device(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, float pred_iou_thresh, float stability_thresh,
                                     float stability_offset, float nms_iou_thresh, int capacity, int min_region_area, void* masks_u8_dev, void* info_i32_dev,
                                     void* info_f32_dev, void* counts_dev, void* stream) {
    sam_generate_check_args(prompts, n_args, n, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh, capacity);
    sam_generate_check_region_area(min_region_area);
    if (!masks_u8_dev || !info_i32_dev || !info_f32_dev || !counts_dev) throw except("sam: null argument");
    sam_require_decoder(m);
    device_turn turn(*m.backend);
    void* s = stream ? stream : m.backend->stream;
    const int N = 3 * n; // the planes the reference chooses among (vision.cpp:80-82) are the candidates of a prompt
    const int64_t n_px = (int64_t)16 * m.dec.res * m.dec.res;
    const size_t nms_bytes = vx_sam_rank_nms_workspace_bytes(N);
    workspace_layout layout;
    const size_t o_logits = layout.take((size_t)n * 4 * n_px * 2, 256), o_iou = layout.take((size_t)n * 16, 256), o_table = layout.take((size_t)N * 24, 256);
    const size_t o_stab = layout.take((size_t)N * 4, 256), o_flags = layout.take((size_t)N * 4, 256), o_rank = layout.take((size_t)N * 4, 256);
    const size_t o_keep = layout.take((size_t)capacity * 4, 256), o_nms = layout.take(nms_bytes, 256);
    // the cleaning stage (min_region_area > 0) needs the masks somewhere other than their final place, since its second NMS reorders them: the first stage's
    // masks and records are staged here, capacity * h * w bytes (256 MB at 256 masks of 1024^2), next to the labelling workspace and the second NMS's tables
    const bool clean = min_region_area > 0;
    const size_t out_px = (size_t)m.image_extent[0] * m.image_extent[1];
    const int N2 = std::min(capacity, N), clean_group = std::min(N2, kSamCleanGroup);
    const size_t nms2_bytes = clean ? vx_sam_rank_nms_workspace_bytes(N2) : 0;
    const size_t regions_bytes = clean ? vx_mask_regions_workspace_bytes(m.image_extent[0], m.image_extent[1], clean_group) : 0;
    size_t o_smasks = 0, o_sinfo = 0, o_sinfof = 0, o_scounts = 0, o_changed = 0, o_table2 = 0, o_key2 = 0, o_flags2 = 0, o_rank2 = 0, o_keep2 = 0, o_counts2 = 0, o_nms2 = 0,
           o_regions = 0;
    if (clean) {
        if (m.image_extent[0] <= 0) throw except("Missing image embeds, call sam_encode() first");
        o_smasks = layout.take((size_t)N2 * out_px, 256), o_sinfo = layout.take((size_t)N2 * 32, 256), o_sinfof = layout.take((size_t)N2 * 8, 256);
        o_scounts = layout.take(8, 256), o_changed = layout.take((size_t)N2 * 4, 256), o_table2 = layout.take((size_t)N2 * 24, 256), o_key2 = layout.take((size_t)N2 * 4, 256);
        o_flags2 = layout.take((size_t)N2 * 4, 256), o_rank2 = layout.take((size_t)N2 * 4, 256), o_keep2 = layout.take((size_t)N2 * 4, 256), o_counts2 = layout.take(8, 256);
        o_nms2 = layout.take(nms2_bytes, 256), o_regions = layout.take(regions_bytes, 256);
    }
    grow(m.generate_ws, layout.top, {m.backend->stream, s});
    uint8_t* base = static_cast<uint8_t*>(m.generate_ws.ptr);
    void* logits_all = base + o_logits;
    float *iou = reinterpret_cast<float*>(base + o_iou), *stab = reinterpret_cast<float*>(base + o_stab);
    int32_t *table = reinterpret_cast<int32_t*>(base + o_table), *flags = reinterpret_cast<int32_t*>(base + o_flags), *rank = reinterpret_cast<int32_t*>(base + o_rank);
    int32_t *keep = reinterpret_cast<int32_t*>(base + o_keep), *counts = static_cast<int32_t*>(counts_dev);

    // diagnostics (sam_enable_timing; tools/bench_sam_autogen.py): events around the stages, read after the call, which then waits for the device
    struct event_list {
        std::vector<void*> ev;
        void* s;
        bool on;
        void mark() {
            if (!on) return;
            void* e = nullptr;
            VX(vx_event_create(&e));
            ev.push_back(e);
            VX(vx_event_record(e, s));
        }
        ~event_list() { for (void* e : ev) vx_event_destroy(e); }
    } marks{{}, s, m.timing};
    marks.mark();
    sam_decode_ctx ctx = sam_decode_prompts(m, prompts, n_args, n, logits_all, iou, nullptr, stream, m.last_batch,
                                            [&](sam_decode_ctx const& c, int p0, int B, void* logits, float*, int32_t*) {
        // the part of the plane the image occupies: SAM scores at image resolution, this scores the decoder's own logits
        const int cw = (c.sw * c.mask_size + c.image_size - 1) / c.image_size, ch = (c.sh * c.mask_size + c.image_size - 1) / c.image_size;
        marks.mark();
        VX(vx_sam_score_planes_f16(logits, 4 * c.n_px, c.n_px, c.mask_size, 3, cw, ch, stability_offset, table + (size_t)p0 * 18, stab + (size_t)p0 * 3, B, c.s));
        marks.mark();
    });
    // the first stage's outputs: the caller's buffers, or with cleaning the staging buffers (of min(capacity, N) masks: no more can come out)
    uint8_t* masks1 = clean ? base + o_smasks : static_cast<uint8_t*>(masks_u8_dev);
    int32_t *info1 = clean ? reinterpret_cast<int32_t*>(base + o_sinfo) : static_cast<int32_t*>(info_i32_dev), *counts1 = clean ? reinterpret_cast<int32_t*>(base + o_scounts) : counts;
    float* infof1 = clean ? reinterpret_cast<float*>(base + o_sinfof) : static_cast<float*>(info_f32_dev);
    const int cap1 = clean ? N2 : capacity;
    VX(vx_sam_rank_nms(table, iou, 3, 4, N, pred_iou_thresh, stability_thresh, nms_iou_thresh, cap1, base + o_nms, nms_bytes, flags, rank, keep, counts1, s));
    marks.mark();
    VX(vx_sam_process_masks_indexed(logits_all, 4 * ctx.n_px, ctx.n_px, 1, ctx.mask_size, 3, n, keep, counts1, cap1, ctx.Bmax, ctx.scaled, ctx.image_size, ctx.sw, ctx.sh,
                                    masks1, ctx.target[0], ctx.target[1], s));
    VX(vx_sam_mask_stats_u8(masks1, ctx.target[0], ctx.target[1], keep, counts1, cap1, 3, n, iou, 4, stab, info1, infof1, s));
    if (clean) { // SAM's postprocess_small_regions: clean, measure again, a second NMS with the scores 1 (unchanged) / 0 (changed), the survivors in its order
        int32_t *changed = reinterpret_cast<int32_t*>(base + o_changed), *table2 = reinterpret_cast<int32_t*>(base + o_table2), *keep2 = reinterpret_cast<int32_t*>(base + o_keep2);
        int32_t* counts2 = reinterpret_cast<int32_t*>(base + o_counts2);
        float* key2 = reinterpret_cast<float*>(base + o_key2);
        marks.mark();
        VX(vx_mask_remove_small_regions_u8(masks1, ctx.target[0], ctx.target[1], N2, counts1, min_region_area, VX_REGIONS_BOTH, changed, base + o_regions, regions_bytes,
                                           clean_group, s));
        marks.mark();
        VX(vx_sam_mask_stats_u8(masks1, ctx.target[0], ctx.target[1], keep, counts1, N2, 3, n, iou, 4, stab, info1, infof1, s));
        VX(vx_sam_clean_nms_inputs(info1, changed, counts1, N2, table2, key2, s));
        VX(vx_sam_rank_nms(table2, key2, 1, 1, N2, -1.0f, 0.0f, nms_iou_thresh, N2, base + o_nms2, nms2_bytes, reinterpret_cast<int32_t*>(base + o_flags2),
                           reinterpret_cast<int32_t*>(base + o_rank2), keep2, counts2, s));
        marks.mark();
        VX(vx_sam_gather_clean_masks(masks1, ctx.target[0], ctx.target[1], info1, infof1, changed, keep2, counts1, counts2, N2, static_cast<uint8_t*>(masks_u8_dev),
                                     static_cast<int32_t*>(info_i32_dev), static_cast<float*>(info_f32_dev), counts, s));
    }
    if (marks.on) { // {decode, scoring, rank + NMS, output masks and their records | clean, records + second NMS, gather} in ms: events 0 | (before, behind a chunk's
                    // scoring) .. | behind NMS | behind the records [| behind the cleaning | behind the second NMS] | end
        marks.mark();
        float* out = m.generate_split_ms;
        for (int i = 0; i < 7; ++i) out[i] = 0.0f;
        const size_t last = marks.ev.size() - 1, tail = clean ? 5 : 2; // intervals behind the chunks
        for (size_t i = 1; i <= last; ++i) {
            float ms = 0.0f;
            VX(vx_event_elapsed_ms(marks.ev[i - 1], marks.ev[i], &ms));
            out[i + tail > last ? 2 + (i + tail - last - 1) : (i & 1) ? 0 : 1] += ms;
        }
    }
    if (!stream) VX(vx_stream_sync(s));
}

void sam_generate_masks_device(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, float pred_iou_thresh, float stability_thresh, float stability_offset,
                               float nms_iou_thresh, int capacity, void* masks_u8_dev, void* info_i32_dev, void* info_f32_dev, void* counts_dev, void* stream) {
    sam_generate_masks_clean_device(m, prompts, n_args, n, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh, capacity, 0, masks_u8_dev, info_i32_dev,
                                    info_f32_dev, counts_dev, stream);
}

void sam_generate_masks_clean_host(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, float pred_iou_thresh, float stability_thresh,
                                   float stability_offset, float nms_iou_thresh, int capacity, int min_region_area, uint8_t* masks_u8, int32_t* info_i32, float* info_f32,
                                   int32_t* counts) {
    sam_generate_check_args(prompts, n_args, n, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh, capacity);
    sam_generate_check_region_area(min_region_area);
    if (!masks_u8 || !info_i32 || !info_f32 || !counts) throw except("sam: null argument");
    sam_require_decoder(m);
    device_turn turn(*m.backend);
    void* s = m.backend->stream;
    const size_t px = (size_t)m.image_extent[0] * m.image_extent[1];
    workspace_layout lay;
    const size_t o_m = lay.take((size_t)capacity * px), o_i = lay.take((size_t)capacity * 32), o_f = lay.take((size_t)capacity * 8), o_c = lay.take(16);
    device_buffer out(lay.top);
    uint8_t* base = static_cast<uint8_t*>(out.ptr);
    sam_generate_masks_clean_device(m, prompts, n_args, n, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh, capacity, min_region_area, base + o_m,
                                    base + o_i, base + o_f, base + o_c, s);
    VX(vx_memcpy_d2h(counts, base + o_c, min_region_area > 0 ? 16 : 8, s));
    VX(vx_stream_sync(s));
    const size_t k = (size_t)std::min(std::max(counts[0], 0), capacity); // rows and masks behind the returned ones stay as the caller left them
    if (k) {
        VX(vx_memcpy_d2h(masks_u8, base + o_m, k * px, s));
        VX(vx_memcpy_d2h(info_i32, base + o_i, k * 32, s));
        VX(vx_memcpy_d2h(info_f32, base + o_f, k * 8, s));
        VX(vx_stream_sync(s));
    }
}

void sam_generate_masks_host(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, float pred_iou_thresh, float stability_thresh, float stability_offset,
                             float nms_iou_thresh, int capacity, uint8_t* masks_u8, int32_t* info_i32, float* info_f32, int32_t* counts) {
    sam_generate_masks_clean_host(m, prompts, n_args, n, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh, capacity, 0, masks_u8, info_i32, info_f32,
                                  counts);
}

} // namespace visp
