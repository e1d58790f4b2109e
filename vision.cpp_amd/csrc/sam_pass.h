// What MobileSAM's three translation units share (tinyvit.cpp: loader + encoder, sam_decoder.cpp: prompt encoder + mask decoder, sam_generate.cpp:
// automatic mask generation): the launch pass of the family and the decoder's chunk loop. Internal: included by those three files only.
#pragma once
#include <cstring>
#include <functional>

#include "tinyvit.h"
#include "visp_util.h"

namespace visp {

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

void sam_require_decoder(sam_model const&); // throws without decoder weights, host tables or an encoded image

// what the launches behind a chunk's mask product need of the decode: the stream, the maps the masks pass through and the extents
struct sam_decode_ctx {
    void* s = nullptr;
    float* scaled = nullptr; // f32 [Bmax][image_size^2]
    int Bmax = 0, image_size = 0, mask_size = 0, sw = 0, sh = 0;
    int64_t n_px = 0;
    i32x2 target = {{0, 0}};
};
// launches what follows the logits of prompts [p0, p0 + B) on ctx.s
using sam_chunk_hook = std::function<void(sam_decode_ctx const& ctx, int p0, int B, void* logits, float* iou, int32_t* chosen)>;

// The decoder, which sam_compute, sam_compute_batch_* and sam_generate_masks_* all run: the prompt tokens of the call, layer 0's shared image side, then per
// chunk the decoder, the mask product and the iou head. The logits of a chunk go to the chunk buffer of the workspace, or, with logits_all, to
// [p0 ..] of a buffer that keeps the planes of every prompt; after_chunk launches what follows them. With captures on, `kept` receives the logits and iou
// predictions of every prompt (a synchronisation per chunk); with captures off it is emptied.
sam_decode_ctx sam_decode_prompts(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, void* logits_all, void* iou_dev, void* chosen_dev, void* stream,
                                  sam_kept_logits& kept, sam_chunk_hook const& after_chunk);

} // namespace visp
