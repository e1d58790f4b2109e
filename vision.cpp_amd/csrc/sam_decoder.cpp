#include "sam_pass.h"

#include <algorithm>
#include <cmath>

namespace visp {

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

} // namespace

void sam_require_decoder(sam_model const& m) {
    samdec_weights const& D = m.dec;
    if (!D.present) throw except("sam: this model file holds no prompt encoder / mask decoder (dec.* tensors)");
    if (D.gaussian.empty()) throw except("sam: the decoder's host tables were not read (model loaded without data)");
    if (!m.embed.ptr || m.image_extent[0] <= 0) throw except("Missing image embeds, call sam_encode() first");
}

sam_decode_ctx sam_decode_prompts(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, void* logits_all, void* iou_dev, void* chosen_dev, void* stream,
                                  sam_kept_logits& kept, sam_chunk_hook const& after_chunk) {
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
    workspace_table ws; // each slot reads as its address once the workspace has grown
    auto take = [&](size_t elems) { return ws.add<uint8_t>(elems * 2, 256); };
    const auto tok_all = take((size_t)n * Nt * dim);
    const auto K0 = take((size_t)Nk * dim), k10 = take((size_t)Nk * dim), pk0 = take((size_t)Nk * ci), pv0 = take((size_t)Nk * ci), pq0 = take((size_t)Nk * ci);
    const auto Q = take(R * dim), t1 = take(R * dim), t2 = take(R * dim), hbuf = take(R * mlp_w + 64);
    const auto tq = take(R * tok_w), tk = take(R * tok_w), tv = take(R * tok_w), ta = take(R * tok_w);
    const auto K = take(big * dim), k1 = take(big * dim), k2 = take(big * dim);
    const auto pq = take(big * ci), pk = take(big * ci), pv = take(big * ci), ao = take(big * ci);
    const auto u1 = take(4 * big * D.up_c1), u1n = take(4 * big * D.up_c1), u2p = take(16 * big * D.up_c2), u2 = take(16 * big * D.up_c2 + 64);
    const auto ha = take((size_t)Bmax * hyp_w + 64), hb = take((size_t)Bmax * hyp_w + 64), hy = take((size_t)Bmax * 4 * D.up_c2 + 64);
    const auto masks_d = take((size_t)Bmax * 4 * n_px);
    const auto iou_ws = ws.add<float>((size_t)Bmax * 4 * 4, 256);
    const auto chosen_ws = ws.add<int32_t>((size_t)Bmax * 4, 256);
    const auto scaled = ws.add<float>((size_t)Bmax * image_size * image_size * 4, 256);
    const size_t part_bytes = std::max(vx_attention_cross_partial_bytes(Bmax, H, Nt, Nk, hd_c), vx_attention_cross_partial_bytes(1, H, (int)R, Nk, hd_c));
    const auto part = ws.add(part_bytes, 256);
    grow(m.batch_ws, ws.layout.top, {m.backend->stream, s}, s); // zero-filled: GEMM rows are read up to K padded to 64, stale bytes must be finite
    ws.base = static_cast<uint8_t*>(m.batch_ws.ptr);

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
        VX(vx_attention_cross_f16(q, k, v, out, part_bytes ? static_cast<void*>(part) : nullptr, part_bytes, Bt, H, Tq, Tk, hd, 1.0f / std::sqrt((float)hd), s));
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

    const sam_decode_ctx ctx{s, scaled, Bmax, image_size, mask_size, sw, sh, n_px, target};
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
            linear(L.self_attn.o, ta, Rt, t2, li > 0 ? VX_EPI_F16_ADD : VX_EPI_F16, li > 0 ? static_cast<const void*>(Q) : nullptr);
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
        float* iou_out = iou_dev ? static_cast<float*>(iou_dev) + (size_t)p0 * 4 : iou_ws;
        int32_t* chosen_out = chosen_dev ? static_cast<int32_t*>(chosen_dev) + p0 : chosen_ws;
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

namespace {

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

} // namespace visp
