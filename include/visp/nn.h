// visp/nn.h -- the neural-network building blocks of the reference's src/visp/nn.h with the same names and argument meaning,
// over this backend's graph layer (visp/ml.h). A module's parameters are looked up under the model_ref's prefix ("weight",
// "bias"), as in the reference. 2D maps are CWHN throughout, so the permute / contiguous helpers are identities.
// Below them: the element-wise and shape ops the reference's arch code calls on ggml directly, under plain names (add, mul, gelu,
// relu, scale, reshape_3d / _4d, repeat_4d, cont), and -- opt-in, #define VISP_GGML_NAMES before including -- under the ggml_* names
// with a model_ref where ggml takes its context, which is how that code passes it.
#pragma once

#include <cstdarg>
#include <cstdio>

#include "ml.h"

namespace visp {

inline tensor linear(model_ref m, tensor x) { // nn.cpp:6-12
    tensor b = m.find("bias");
    return b ? detail::op(m, VISP_OP_LINEAR, {x, m.weights("weight"), b}) : detail::op(m, VISP_OP_LINEAR, {x, m.weights("weight")});
}
inline tensor layer_norm(model_ref m, tensor x, float eps = 1e-5f) { // nn.cpp:14-19
    return detail::op(m, VISP_OP_LAYER_NORM, {x, m.weights("weight"), m.weights("bias")}, {}, {eps});
}

inline bool is_whcn(model_ref m) { return !(m.flags & model_build_flag::cwhn); }
inline bool is_cwhn(model_ref m) { return !!(m.flags & model_build_flag::cwhn); }
inline tensor permute_cwhn_to_whcn(model_ref, tensor x) { return x; }
inline tensor permute_whcn_to_cwhn(model_ref, tensor x) { return x; }
inline tensor cwhn_to_contiguous_2d(model_ref, tensor x) { return x; }
inline tensor whcn_to_contiguous_2d(model_ref, tensor x) { return x; }
inline tensor contiguous_2d_to_cwhn(model_ref, tensor x) { return x; }
inline tensor contiguous_2d_to_whcn(model_ref, tensor x) { return x; }
inline std::array<int64_t, 4> nelements_whcn(model_ref const&, tensor t) { return {t->ne[1], t->ne[2], t->ne[0], t->ne[3]}; }

inline tensor conv_2d(model_ref m, tensor x, int stride = 1, int pad = 0) { // nn.cpp:72-100; weight [Cin, kw, kh, Cout]
    tensor b = m.find("bias");
    return b ? detail::op(m, VISP_OP_CONV_2D, {x, m.weights("weight"), b}, {stride, pad}) : detail::op(m, VISP_OP_CONV_2D, {x, m.weights("weight")}, {stride, pad});
}
// depthwise: weight [C, 1, kw, kh] (written NHWC: local_conv of mobile-sam.cpp:152-155) or [1, kw, kh, C] (OIHW, listed in conv2d_weights); nn.cpp:102-115
inline tensor conv_2d_depthwise(model_ref m, tensor x, int stride = 1, int pad = 0) {
    tensor b = m.find("bias");
    return b ? detail::op(m, VISP_OP_CONV_2D_DEPTHWISE, {x, m.weights("weight"), b}, {stride, pad}) : detail::op(m, VISP_OP_CONV_2D_DEPTHWISE, {x, m.weights("weight")}, {stride, pad});
}
inline tensor conv_transpose_2d(model_ref m, tensor x, int stride) { // nn.cpp:117-129; weight [kw, kh, Cout, Cin], kernel == stride
    tensor b = m.find("bias");
    return b ? detail::op(m, VISP_OP_CONV_TRANSPOSE_2D, {x, m.weights("weight"), b}, {stride}) : detail::op(m, VISP_OP_CONV_TRANSPOSE_2D, {x, m.weights("weight")}, {stride});
}
// image [C, W, H, N] f32 -> [D, W / p, H / p, N]: the projection conv with kernel == stride (nn.cpp:166-180; DINOv2 has no norm)
inline tensor patch_embed(model_ref m, tensor x, int patch_size) {
    model_ref p = m[m.find("proj.weight") ? "proj" : "projection"]; // nn.cpp:168
    tensor b = p.find("bias");
    tensor out = b ? detail::op(m, VISP_OP_PATCH_EMBED, {x, p.weights("weight"), b}, {patch_size}) : detail::op(m, VISP_OP_PATCH_EMBED, {x, p.weights("weight")}, {patch_size});
    if (m.find("norm.weight")) out = layer_norm(m["norm"], out);
    return out;
}

// deformable convolution (nn.cpp:131-148): weight [Cin, k, k, Cout], offset [2 k k, OW, OH, N] (dy, dx per tap), mask [k k, OW, OH, N] or null; stride 1
inline tensor conv_2d_deform(model_ref m, tensor x, tensor weight, tensor offset, tensor mask, int stride, int pad) {
    return mask ? detail::op(m, VISP_OP_CONV_2D_DEFORM, {x, weight, offset, mask}, {stride, pad}) : detail::op(m, VISP_OP_CONV_2D_DEFORM, {x, weight, offset}, {stride, pad});
}
// x * weight + bias per channel: the form a batch norm has once model conversion folded its statistics (nn.cpp:150-164)
inline tensor batch_norm_2d(model_ref m, tensor x) {
    if (m.find("running_mean") || m.find("running_var")) throw exception("Batch norm was not fused");
    x = detail::op(m, VISP_OP_MUL, {x, m.weights("weight")});
    return named(m, detail::op(m, VISP_OP_ADD, {x, m.weights("bias")}));
}

// element-wise and shape ops
inline tensor add(model_ref const& m, tensor a, tensor b) { return detail::op(m, VISP_OP_ADD, {a, b}); }
inline tensor mul(model_ref const& m, tensor a, tensor b) { return detail::op(m, VISP_OP_MUL, {a, b}); }
inline tensor gelu(model_ref const& m, tensor x) { return detail::op(m, VISP_OP_GELU, {x}); }
inline tensor relu(model_ref const& m, tensor x) { return detail::op(m, VISP_OP_RELU, {x}); }
inline tensor scale(model_ref const& m, tensor x, float s) { return detail::op(m, VISP_OP_SCALE, {x}, {}, {s}); }
inline tensor leaky_relu(model_ref const& m, tensor x, float negative_slope) { return detail::op(m, VISP_OP_LEAKY_RELU, {x}, {}, {negative_slope}); }
inline tensor sigmoid(model_ref const& m, tensor x) { return detail::op(m, VISP_OP_SIGMOID, {x}); }
// [C, W, H, N] -> [C, 1, 1, N] (mean_2d, birefnet.cpp:93-100; not ggml_mean, which reduces ne[0])
inline tensor mean_2d(model_ref const& m, tensor x) { return detail::op(m, VISP_OP_MEAN_2D, {x}); }
// the ggml calls of yolov9t.cpp beyond the above
inline tensor silu(model_ref const& m, tensor x) { return detail::op(m, VISP_OP_SILU, {x}); }
inline tensor sub(model_ref const& m, tensor a, tensor b) { return detail::op(m, VISP_OP_SUB, {a, b}); } // a - b, b broadcast as for add
// x [C, W, H, N]; kind 0 max, 1 average (ggml's values); kernel, stride and pad per dimension as ggml_pool_2d takes them
inline tensor pool_2d(model_ref const& m, tensor x, int kind, int k0, int k1, int s0, int s1, int p0, int p1) { return detail::op(m, VISP_OP_POOL_2D, {x}, {kind, k0, k1, s0, s1, p0, p1}); }
inline tensor soft_max(model_ref const& m, tensor x) { return detail::op(m, VISP_OP_SOFT_MAX, {x}); } // over dimension 0
inline tensor sum_rows(model_ref const& m, tensor x) { return detail::op(m, VISP_OP_SUM_ROWS, {x}); } // [n, a, b, c] -> [1, a, b, c]
// the ggml call of migan.cpp beyond the above: min(max(x, lo), hi) (migan.cpp:23); add / mul / sub also take a plane [1, W, H, 1] on [C, W, H, N] (migan.cpp:40, 76)
inline tensor clamp(model_ref const& m, tensor x, float lo, float hi) { return detail::op(m, VISP_OP_CLAMP, {x}, {}, {lo, hi}); }
// ggml_upscale: both extents times `factor` (NEAREST: the existing interpolate at mode 0)
inline tensor upscale(model_ref const& m, tensor x, int factor, int32_t mode) { return interpolate(m, x, {x->ne[1] * factor, x->ne[2] * factor}, mode); }
inline tensor cont(model_ref const& m, tensor x) { return detail::op(m, VISP_OP_CONT, {x}); }
inline tensor reshape_4d(model_ref const& m, tensor x, int64_t n0, int64_t n1, int64_t n2, int64_t n3) { return detail::op(m, VISP_OP_RESHAPE, {x}, {n0, n1, n2, n3}); }
inline tensor reshape_3d(model_ref const& m, tensor x, int64_t n0, int64_t n1, int64_t n2) { return reshape_4d(m, x, n0, n1, n2, 1); }
inline tensor repeat_4d(model_ref const& m, tensor x, int64_t n0, int64_t n1, int64_t n2, int64_t n3) { return detail::op(m, VISP_OP_REPEAT, {x}, {n0, n1, n2, n3}); }

inline tensor permute(model_ref const& m, tensor x, int a0, int a1, int a2, int a3) { return detail::op(m, VISP_OP_PERMUTE, {x}, {a0, a1, a2, a3}); } // ggml_permute's axes
inline tensor roll(model_ref const& m, tensor x, int s0, int s1, int s2, int s3) { return detail::op(m, VISP_OP_ROLL, {x}, {s0, s1, s2, s3}); }
inline tensor pad(model_ref const& m, tensor x, int p0, int p1, int p2, int p3) { return detail::op(m, VISP_OP_PAD, {x}, {p0, p1, p2, p3}); }
inline tensor get_rows(model_ref const& m, tensor table, tensor index) { return detail::op(m, VISP_OP_GET_ROWS, {table, index}); }
inline tensor cast(model_ref const& m, tensor x, int32_t type) { return detail::op(m, VISP_OP_CAST, {x}, {type}); }

struct attention_qkv { tensor q, k, v; };
// one linear to 3 C channels, split into q, k, v [head_dim, n_heads, n_tokens, batch] (nn.cpp:182-208). split_dim says how the 3 C outputs are
// ordered: 1 = (head, q|k|v, head_dim), 2 = (q|k|v, head, head_dim)
inline attention_qkv split_qkv(model_ref m, tensor x, int n_heads, int split_dim) {
    auto [c, n, b, _] = nelements(x);
    tensor qkv = linear(m, x);
    switch (split_dim) {
        case 1:
            qkv = reshape_4d(m, qkv, c / n_heads, 3, n_heads * n, b);
            qkv = cont(m, permute(m, qkv, 0, 3, 1, 2));
            break;
        case 2:
            qkv = reshape_4d(m, qkv, c / n_heads, n_heads, 3, n * b);
            qkv = cont(m, permute(m, qkv, 0, 1, 3, 2));
            break;
        default: throw exception("split_qkv: split_dim is 1 or 2");
    }
    auto split = [&](tensor t, int64_t index) {
        t = slice(m, t, {}, {}, {}, index);
        return reshape_4d(m, t, c / n_heads, n_heads, n, b);
    };
    return {split(qkv, 0), split(qkv, 1), split(qkv, 2)};
}
// attention with an optional mask [n_keys, n_queries, 1 | n_heads, a divisor of batch] and an output linear layer; q, k, v
// [head_dim, n_heads, n_tokens, batch] (nn.cpp:210-244). Without a mask: the head_dim-64 kernel; with one: head_dim 32 and 64.
inline tensor attention(model_ref m, tensor q, tensor k, tensor v, tensor mask, float scale_, model_ref m_out) {
    tensor x = mask ? detail::op(m, VISP_OP_ATTENTION_MASKED, {q, k, v, mask}, {}, {scale_}) : detail::op(m, VISP_OP_ATTENTION, {q, k, v}, {}, {scale_});
    return linear(m_out, x);
}

// attention WITHOUT a mask for any number of queries and keys at head_dim 16, 32 and 64, with an output linear layer: q [head_dim, n_heads, n_queries, batch],
// k, v [head_dim, n_heads, n_keys, batch] (nn.cpp:210-244 with mask == nullptr, as the SAM mask decoder calls it: mobile-sam.cpp:307-319). A builder of its
// own next to attention(), whose mask-less form keeps the head_dim-64 self-attention kernel and its refusals.
inline tensor attention_cross(model_ref m, tensor q, tensor k, tensor v, float scale_, model_ref m_out) {
    return linear(m_out, detail::op(m, VISP_OP_ATTENTION_CROSS, {q, k, v}, {}, {scale_}));
}
// the ggml calls of the SAM prompt encoder and mask decoder beyond the above (mobile-sam.cpp:243-246, 471)
inline tensor mul_mat(model_ref const& m, tensor a, tensor b) { return detail::op(m, VISP_OP_MUL_MAT, {a, b}); } // a [K, M, Ba], b [K, N, B] -> [M, N, B]
inline tensor sin(model_ref const& m, tensor x) { return detail::op(m, VISP_OP_SIN, {x}); }
inline tensor cos(model_ref const& m, tensor x) { return detail::op(m, VISP_OP_COS, {x}); }
// the ggml call of the SAM3 vision encoder beyond the above (sam3.h:413-438): ggml_rope_ext in GGML_ROPE_TYPE_NORMAL. x [n, heads, T, B] f16, pos an i32 constant
// [T]; n_dims == n. Pair i of token t is rotated by pos[t] * freq_scale * freq_base^(-2 i / n).
inline tensor rope(model_ref const& m, tensor x, tensor pos, int n_dims, float freq_base, float freq_scale) {
    return detail::op(m, VISP_OP_ROPE, {x, pos}, {n_dims, 0}, {freq_base, freq_scale});
}
// image_to_patches (birefnet.cpp:153-162) as one op: the f32 image [C <= 4, W, H, N] (the graph input, or interpolate of it in bilinear | align_corners) ->
// f16 [gw gh C, out_w, out_h, N] with gw = W / out_w, gh = H / out_h; channel gx + gw (gy + gh c) of pixel (py, px) is image (gy out_h + py, gx out_w + px, c)
inline tensor image_patches(model_ref const& m, tensor image, int64_t out_w, int64_t out_h) { return detail::op(m, VISP_OP_IMAGE_PATCHES, {image}, {out_w, out_h}); }

#ifdef VISP_GGML_NAMES
// the two calls the reference's arch code makes without a context (dino.cpp:104-105): the tensor knows its graph
inline tensor ggml_format_name(tensor t, char const* fmt, ...) __attribute__((format(printf, 2, 3)));
inline tensor ggml_format_name(tensor t, char const* fmt, ...) {
    char buf[128];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    detail::check(visp_graph_set_name(t.graph, t.id, buf));
    return t;
}
// ggml adds the tensor to the forward graph so that it is computed and kept; here: it becomes an output under its current name
inline void ggml_build_forward_expand(compute_graph& g, tensor t) { detail::check(visp_graph_output(g.handle, t.id, nullptr)); }
inline tensor ggml_add(model_ref const& m, tensor a, tensor b) { return add(m, a, b); }
inline tensor ggml_add_inplace(model_ref const& m, tensor a, tensor b) { return add(m, a, b); }
inline tensor ggml_mul(model_ref const& m, tensor a, tensor b) { return mul(m, a, b); }
inline tensor ggml_gelu(model_ref const& m, tensor x) { return gelu(m, x); }
inline tensor ggml_relu(model_ref const& m, tensor x) { return relu(m, x); }
inline tensor ggml_relu_inplace(model_ref const& m, tensor x) { return relu(m, x); }
inline tensor ggml_scale(model_ref const& m, tensor x, float s) { return scale(m, x, s); }
inline tensor ggml_scale_inplace(model_ref const& m, tensor x, float s) { return scale(m, x, s); }
inline tensor ggml_sigmoid(model_ref const& m, tensor x) { return sigmoid(m, x); }
inline tensor ggml_sigmoid_inplace(model_ref const& m, tensor x) { return sigmoid(m, x); }
inline tensor ggml_leaky_relu(model_ref const& m, tensor x, float negative_slope, bool /*inplace*/) { return leaky_relu(m, x, negative_slope); }
inline tensor ggml_cont(model_ref const& m, tensor x) { return cont(m, x); }
inline tensor ggml_reshape_3d(model_ref const& m, tensor x, int64_t n0, int64_t n1, int64_t n2) { return reshape_3d(m, x, n0, n1, n2); }
inline tensor ggml_reshape_4d(model_ref const& m, tensor x, int64_t n0, int64_t n1, int64_t n2, int64_t n3) { return reshape_4d(m, x, n0, n1, n2, n3); }
inline tensor ggml_repeat_4d(model_ref const& m, tensor x, int64_t n0, int64_t n1, int64_t n2, int64_t n3) { return repeat_4d(m, x, n0, n1, n2, n3); }
inline tensor ggml_permute(model_ref const& m, tensor x, int a0, int a1, int a2, int a3) { return permute(m, x, a0, a1, a2, a3); }
inline tensor ggml_roll(model_ref const& m, tensor x, int s0, int s1, int s2, int s3) { return roll(m, x, s0, s1, s2, s3); }
inline tensor ggml_pad(model_ref const& m, tensor x, int p0, int p1, int p2, int p3) { return pad(m, x, p0, p1, p2, p3); }
inline tensor ggml_get_rows(model_ref const& m, tensor table, tensor index) { return get_rows(m, table, index); }
inline tensor ggml_cast(model_ref const& m, tensor x, int32_t type) { return cast(m, x, type); }
inline tensor ggml_gelu_inplace(model_ref const& m, tensor x) { return gelu(m, x); }
inline tensor ggml_get_tensor(model_ref const& m, char const* name) { return get_tensor(m, name); }
constexpr int GGML_OP_POOL_MAX = 0, GGML_OP_POOL_AVG = 1;
inline tensor ggml_silu(model_ref const& m, tensor x) { return silu(m, x); }
inline tensor ggml_silu_inplace(model_ref const& m, tensor x) { return silu(m, x); }
inline tensor ggml_pool_2d(model_ref const& m, tensor x, int kind, int k0, int k1, int s0, int s1, int p0, int p1) { return pool_2d(m, x, kind, k0, k1, s0, s1, p0, p1); }
inline tensor ggml_soft_max(model_ref const& m, tensor x) { return soft_max(m, x); }
inline tensor ggml_sum_rows(model_ref const& m, tensor x) { return sum_rows(m, x); }
inline tensor ggml_sub(model_ref const& m, tensor a, tensor b) { return sub(m, a, b); }
inline tensor ggml_upscale(model_ref const& m, tensor x, int factor, int32_t mode) { return upscale(m, x, factor, mode); }
inline tensor ggml_concat(model_ref const& m, tensor a, tensor b, int dim) { return concat(m, {a, b}, dim); }
inline tensor ggml_clamp(model_ref const& m, tensor x, float lo, float hi) { return clamp(m, x, lo, hi); }
inline tensor ggml_mul_inplace(model_ref const& m, tensor a, tensor b) { return mul(m, a, b); }
inline tensor ggml_mul_mat(model_ref const& m, tensor a, tensor b) { return mul_mat(m, a, b); }
inline tensor ggml_sin(model_ref const& m, tensor x) { return sin(m, x); }
inline tensor ggml_cos(model_ref const& m, tensor x) { return cos(m, x); }
constexpr int GGML_ROPE_TYPE_NORMAL = 0, GGML_ROPE_TYPE_NEOX = 2;
// ggml's full argument list. Built: no frequency factors, GGML_ROPE_TYPE_NORMAL (any other mode is refused by the op), and the defaults of the YaRN
// arguments (ext_factor 0, attn_factor 1, beta_fast / beta_slow 0, as sam3.h:423-427 passes them); n_ctx_orig is not read without YaRN.
inline tensor ggml_rope_ext(model_ref const& m, tensor a, tensor b, tensor c, int n_dims, int mode, int /*n_ctx_orig*/, float freq_base, float freq_scale, float ext_factor,
                            float attn_factor, float beta_fast, float beta_slow) {
    if (c) throw exception("rope: frequency factors are not built (pass a null tensor)");
    if (ext_factor != 0.0f || attn_factor != 1.0f || beta_fast != 0.0f || beta_slow != 0.0f)
        throw exception("rope: ext_factor / attn_factor / beta_fast / beta_slow other than 0, 1, 0, 0 (YaRN) are not built");
    return detail::op(m, VISP_OP_ROPE, {a, b}, {n_dims, mode}, {freq_base, freq_scale});
}
#endif

} // namespace visp
