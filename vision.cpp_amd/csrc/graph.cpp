// Tensor graph + executor (see graph.h). Host C++ only: device work goes through the vx_* C ABI.
#include "graph.h"

#include <cmath>
#include <optional>

#include "lowering.h"

namespace visp {

std::string shape_str(const int64_t ne[4]) {
    char b[96];
    snprintf(b, sizeof b, "[%lld, %lld, %lld, %lld]", (long long)ne[0], (long long)ne[1], (long long)ne[2], (long long)ne[3]);
    return b;
}

namespace {

const char* const op_names[gop_count] = {"input", "weight", "linear", "layer_norm", "gelu", "relu", "scale", "add", "mul", "conv_2d",
                                         "conv_transpose_2d", "interpolate", "attention", "concat", "slice", "reshape", "repeat",
                                         "patch_embed", "cont", "image_u8_to_f32", "image_normalize", "leaky_relu", "permute", "roll", "pad", "get_rows",
                                         "cast", "attention_masked", "conv_2d_deform", "sigmoid", "mean_2d", "conv_2d_depthwise", "silu", "pool_2d", "soft_max",
                                         "sum_rows", "sub", "clamp", "attention_cross", "mul_mat", "sin", "cos", "rope", "image_patches"};

// ---- host evaluation of constants (f32, ggml index order: i0 fastest) ------------------------------------------------------

struct host_view {
    const float* p;
    const int64_t* ne;
    float at(int64_t i0, int64_t i1, int64_t i2, int64_t i3) const { return p[((i3 * ne[2] + i2) * ne[1] + i1) * ne[0] + i0]; }
};

// ggml's bicubic (a = -0.75, half-pixel centres, taps clamped to the map) on CWHN: dino.cpp:22-27 runs it on the stored position
// embeddings; the same arithmetic as depthany.cpp's interpolate_pos, for any [C, W, H, N]
void host_bicubic(const float* src, const int64_t sne[4], float* dst, int64_t tw, int64_t th) {
    const int64_t C = sne[0], W = sne[1], H = sne[2], N = sne[3];
    auto coeffs = [](float t, float c[4]) {
        const float a = -0.75f;
        float x;
        x = t + 1.0f; c[0] = ((a * x - 5.0f * a) * x + 8.0f * a) * x - 4.0f * a;
        x = t;        c[1] = ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
        x = 1.0f - t; c[2] = ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
        x = 2.0f - t; c[3] = ((a * x - 5.0f * a) * x + 8.0f * a) * x - 4.0f * a;
    };
    const float sfy = (float)th / (float)H, sfx = (float)tw / (float)W;
    for (int64_t n = 0; n < N; ++n)
        for (int64_t oy = 0; oy < th; ++oy) {
            const float sy = ((float)oy + 0.5f) / sfy - 0.5f;
            const int64_t iy = (int64_t)std::floor(sy);
            float cy[4];
            coeffs(sy - (float)iy, cy);
            for (int64_t ox = 0; ox < tw; ++ox) {
                const float sx = ((float)ox + 0.5f) / sfx - 0.5f;
                const int64_t ix = (int64_t)std::floor(sx);
                float cx[4];
                coeffs(sx - (float)ix, cx);
                float* o = dst + ((n * th + oy) * tw + ox) * C;
                for (int64_t c = 0; c < C; ++c) o[c] = 0.0f;
                for (int j = 0; j < 4; ++j) {
                    const int64_t yy = std::clamp<int64_t>(iy - 1 + j, 0, H - 1);
                    for (int i = 0; i < 4; ++i) {
                        const int64_t xx = std::clamp<int64_t>(ix - 1 + i, 0, W - 1);
                        const float wgt = cy[j] * cx[i];
                        const float* s = src + ((n * H + yy) * W + xx) * C;
                        for (int64_t c = 0; c < C; ++c) o[c] += wgt * s[c];
                    }
                }
            }
        }
}

// bilinear with align_corners as vx_bilinear_ac_f16 / ggml do it: sf = (out - 1) / (in - 1), src = i / sf
void host_bilinear_ac(const float* src, const int64_t sne[4], float* dst, int64_t tw, int64_t th) {
    const int64_t C = sne[0], W = sne[1], H = sne[2], N = sne[3];
    const float sfx = tw > 1 && W > 1 ? (float)(tw - 1) / (float)(W - 1) : (float)tw / (float)W;
    const float sfy = th > 1 && H > 1 ? (float)(th - 1) / (float)(H - 1) : (float)th / (float)H;
    for (int64_t n = 0; n < N; ++n)
        for (int64_t oy = 0; oy < th; ++oy) {
            const float sy = (float)oy / sfy;
            const int64_t y0 = std::min<int64_t>((int64_t)sy, H - 1), y1 = std::min<int64_t>(y0 + 1, H - 1);
            const float fy = sy - (float)y0;
            for (int64_t ox = 0; ox < tw; ++ox) {
                const float sx = (float)ox / sfx;
                const int64_t x0 = std::min<int64_t>((int64_t)sx, W - 1), x1 = std::min<int64_t>(x0 + 1, W - 1);
                const float fx = sx - (float)x0;
                float* o = dst + ((n * th + oy) * tw + ox) * C;
                const float* a = src + ((n * H + y0) * W + x0) * C;
                const float* b = src + ((n * H + y0) * W + x1) * C;
                const float* c = src + ((n * H + y1) * W + x0) * C;
                const float* d = src + ((n * H + y1) * W + x1) * C;
                for (int64_t k = 0; k < C; ++k) {
                    const float top = a[k] + (b[k] - a[k]) * fx, bot = c[k] + (d[k] - c[k]) * fx;
                    o[k] = top + (bot - top) * fy;
                }
            }
        }
}

// b broadcast over the trailing dimensions of a: b.ne[i] == a.ne[i] up to some dimension, 1 from there on. Returns b's period. The one other form
// admitted is a plane (plane_broadcast, graph.h): b [1, W, H, 1] on a [C, W, H, N], one value per pixel; its period is W * H pixels, not elements.
int64_t broadcast_period(const int64_t a[4], const int64_t b[4], const char* what) {
    if (plane_broadcast(a, b)) return b[1] * b[2];
    bool ones = false;
    int64_t period = 1;
    for (int i = 0; i < 4; ++i) {
        if (!ones && b[i] == a[i]) { period *= b[i]; continue; }
        if (b[i] == 1) { ones = ones || a[i] != 1; continue; }
        throw except("%s: cannot broadcast %s onto %s (the second operand must equal the first in its leading dimensions and be 1 in the rest, or be a plane [1, W, H, 1] on [C, W, H, N])", what,
                     shape_str(b).c_str(), shape_str(a).c_str());
    }
    return period;
}

void fold_constant(graph& g, graph_node& n) {
    auto src = [&](int i) -> graph_node const& { return g.nodes[n.src[i]]; };
    const int64_t total = n.n_elements();
    n.host.resize((size_t)total);
    float* out = n.host.data();
    switch (n.op) {
        case gop_reshape:
        case gop_cont: n.host.assign(src(0).values(), src(0).values() + total); break;
        case gop_scale:
            for (int64_t i = 0; i < total; ++i) out[i] = src(0).values()[i] * n.fp[0];
            break;
        case gop_add:
        case gop_mul:
        case gop_sub: {
            const bool plane = plane_broadcast(src(0).ne, src(1).ne); // b's index is then the pixel's, not the element's
            const int64_t period = src(1).n_elements(), C = plane ? n.ne[0] : 1;
            const float *a = src(0).values(), *bv = src(1).values();
            std::vector<float> spread;
            if (plane) {
                spread.resize((size_t)(period * C));
                for (int64_t i = 0; i < period * C; ++i) spread[(size_t)i] = bv[i / C];
            }
            const float* b = plane ? spread.data() : bv;
            for (int64_t i = 0; i < total; ++i) out[i] = n.op == gop_add ? a[i] + b[i % (period * C)] : (n.op == gop_mul ? a[i] * b[i % (period * C)] : a[i] - b[i % (period * C)]);
        } break;
        case gop_silu:
            for (int64_t i = 0; i < total; ++i) out[i] = (float)((double)src(0).values()[i] / (1.0 + std::exp(-(double)src(0).values()[i])));
            break;
        case gop_clamp: // ggml_clamp's comparisons: a NaN stays one, -0.0 stays -0.0
            for (int64_t i = 0; i < total; ++i) {
                const float v = src(0).values()[i];
                out[i] = v < n.fp[0] ? n.fp[0] : (v > n.fp[1] ? n.fp[1] : v);
            }
            break;
        case gop_slice: {
            host_view v{src(0).values(), src(0).ne};
            int64_t o = 0;
            for (int64_t i3 = 0; i3 < n.ne[3]; ++i3)
                for (int64_t i2 = 0; i2 < n.ne[2]; ++i2)
                    for (int64_t i1 = 0; i1 < n.ne[1]; ++i1)
                        for (int64_t i0 = 0; i0 < n.ne[0]; ++i0)
                            out[o++] = v.at(n.ip[0] + i0 * n.ip[2], n.ip[3] + i1 * n.ip[5], n.ip[6] + i2 * n.ip[8], n.ip[9] + i3 * n.ip[11]);
        } break;
        case gop_repeat: {
            host_view v{src(0).values(), src(0).ne};
            int64_t o = 0;
            for (int64_t i3 = 0; i3 < n.ne[3]; ++i3)
                for (int64_t i2 = 0; i2 < n.ne[2]; ++i2)
                    for (int64_t i1 = 0; i1 < n.ne[1]; ++i1)
                        for (int64_t i0 = 0; i0 < n.ne[0]; ++i0) out[o++] = v.at(i0 % v.ne[0], i1 % v.ne[1], i2 % v.ne[2], i3 % v.ne[3]);
        } break;
        case gop_concat: {
            const int dim = (int)n.ip[0];
            host_view a{src(0).values(), src(0).ne}, b{src(1).values(), src(1).ne};
            int64_t o = 0;
            for (int64_t i3 = 0; i3 < n.ne[3]; ++i3)
                for (int64_t i2 = 0; i2 < n.ne[2]; ++i2)
                    for (int64_t i1 = 0; i1 < n.ne[1]; ++i1)
                        for (int64_t i0 = 0; i0 < n.ne[0]; ++i0) {
                            int64_t idx[4] = {i0, i1, i2, i3};
                            if (idx[dim] < a.ne[dim]) out[o++] = a.at(idx[0], idx[1], idx[2], idx[3]);
                            else { idx[dim] -= a.ne[dim]; out[o++] = b.at(idx[0], idx[1], idx[2], idx[3]); }
                        }
        } break;
        case gop_interpolate: {
            const int mode = (int)n.ip[2];
            if ((mode & 255) == 2 && !(mode & 256)) host_bicubic(src(0).values(), src(0).ne, out, n.ip[0], n.ip[1]);
            else if ((mode & 255) == 1 && (mode & 256)) host_bilinear_ac(src(0).values(), src(0).ne, out, n.ip[0], n.ip[1]);
            else throw except("interpolate: mode %d is not built (bicubic, and bilinear | align_corners, are)", mode);
        } break;
        case gop_permute: { // source dimension d is destination dimension ip[d]
            host_view v{src(0).values(), src(0).ne};
            int64_t o = 0, idx[4];
            for (idx[3] = 0; idx[3] < n.ne[3]; ++idx[3])
                for (idx[2] = 0; idx[2] < n.ne[2]; ++idx[2])
                    for (idx[1] = 0; idx[1] < n.ne[1]; ++idx[1])
                        for (idx[0] = 0; idx[0] < n.ne[0]; ++idx[0]) out[o++] = v.at(idx[n.ip[0]], idx[n.ip[1]], idx[n.ip[2]], idx[n.ip[3]]);
        } break;
        case gop_roll: {
            host_view v{src(0).values(), src(0).ne};
            auto from = [&](int64_t i, int d) { return ((i - n.ip[d]) % n.ne[d] + n.ne[d]) % n.ne[d]; };
            int64_t o = 0;
            for (int64_t i3 = 0; i3 < n.ne[3]; ++i3)
                for (int64_t i2 = 0; i2 < n.ne[2]; ++i2)
                    for (int64_t i1 = 0; i1 < n.ne[1]; ++i1)
                        for (int64_t i0 = 0; i0 < n.ne[0]; ++i0) out[o++] = v.at(from(i0, 0), from(i1, 1), from(i2, 2), from(i3, 3));
        } break;
        case gop_pad: {
            host_view v{src(0).values(), src(0).ne};
            int64_t o = 0;
            for (int64_t i3 = 0; i3 < n.ne[3]; ++i3)
                for (int64_t i2 = 0; i2 < n.ne[2]; ++i2)
                    for (int64_t i1 = 0; i1 < n.ne[1]; ++i1)
                        for (int64_t i0 = 0; i0 < n.ne[0]; ++i0)
                            out[o++] = i0 < v.ne[0] && i1 < v.ne[1] && i2 < v.ne[2] && i3 < v.ne[3] ? v.at(i0, i1, i2, i3) : 0.0f;
        } break;
        case gop_get_rows: {
            const int64_t C = src(0).ne[0], rows = src(0).ne[1], cnt = src(1).n_elements();
            for (int64_t i = 0; i < cnt; ++i) {
                const int64_t row = (int64_t)src(1).values()[i];
                if (row < 0 || row >= rows) throw except("get_rows: index %lld at position %lld is outside the table's %lld rows", (long long)row, (long long)i, (long long)rows);
                std::copy(src(0).values() + row * C, src(0).values() + (row + 1) * C, out + i * C);
            }
        } break;
        case gop_sigmoid:
            for (int64_t i = 0; i < total; ++i) out[i] = (float)(1.0 / (1.0 + std::exp(-(double)src(0).values()[i])));
            break;
        case gop_sin:
            for (int64_t i = 0; i < total; ++i) out[i] = (float)std::sin((double)src(0).values()[i]);
            break;
        case gop_cos:
            for (int64_t i = 0; i < total; ++i) out[i] = (float)std::cos((double)src(0).values()[i]);
            break;
        case gop_mul_mat: { // out[m, n, b] = sum_k a[k, m, b or 0] b[k, n, b], in double
            const int64_t K = src(0).ne[0], M = n.ne[0], N = n.ne[1], Ba = src(0).ne[2];
            const float *a = src(0).values(), *bv = src(1).values();
            for (int64_t b = 0; b < n.ne[2]; ++b)
                for (int64_t j = 0; j < N; ++j)
                    for (int64_t m = 0; m < M; ++m) {
                        double acc = 0.0;
                        for (int64_t k = 0; k < K; ++k) acc += (double)a[((Ba == 1 ? 0 : b) * M + m) * K + k] * (double)bv[(b * N + j) * K + k];
                        out[(b * N + j) * M + m] = (float)acc;
                    }
        } break;
        case gop_cast:
            for (int64_t i = 0; i < total; ++i) out[i] = n.dtype == gdt_f16 ? f16_to_f32(f32_to_f16(src(0).values()[i])) : src(0).values()[i];
            break;
        default: throw except("graph: %s on constants is not folded", graph_op_name(n.op));
    }
}

bool foldable(int32_t op) {
    return op == gop_reshape || op == gop_cont || op == gop_scale || op == gop_add || op == gop_mul || op == gop_slice || op == gop_repeat ||
           op == gop_concat || op == gop_interpolate || op == gop_permute || op == gop_roll || op == gop_pad || op == gop_get_rows || op == gop_cast || op == gop_sigmoid ||
           op == gop_silu || op == gop_sub || op == gop_clamp || op == gop_mul_mat || op == gop_sin || op == gop_cos;
}

// the f32 image the reference uploads, [C <= 4, W, H, N], or a resize of one: what interpolate and image_patches take besides f16 activations
bool is_f32_image(graph_node const& x) { return !x.constant && x.dtype == gdt_f32 && x.ne[0] <= 4 && (x.op == gop_input || x.op == gop_interpolate); }

void check_tensor(graph const& g, int t, const char* what) {
    if (t < 0 || t >= (int)g.nodes.size()) throw except("%s: tensor handle %d is not part of this graph", what, t);
}

} // namespace

const char* graph_op_name(int32_t op) { return op >= 0 && op < gop_count ? op_names[op] : "?"; }

graph::~graph() {
    if (dev) vx_set_device(dev->index); // frees go to the device the graph lives on, whatever the calling thread's current device is
}
weight_store::~weight_store() {
    if (dev) vx_set_device(dev->index);
}

std::shared_ptr<weight_store> weights_create() { return std::make_shared<weight_store>(); }

void weights_add(weight_store& ws, char const* name, int32_t dtype, const int64_t ne[4], const float* data) {
    if (!name || !*name) throw except("weights: a tensor needs a name");
    if (ws.tensors.count(name)) throw except("weights: '%s' exists already", name);
    if (ws.dev) throw except("weights: '%s' added after a graph over these weights was allocated", name);
    weight_store::entry e;
    e.dtype = dtype == gdt_f32 ? gdt_f32 : (dtype == gdt_i32 ? gdt_i32 : gdt_f16);
    int64_t n = 1;
    for (int i = 0; i < 4; ++i) {
        if (ne[i] <= 0) throw except("weights: '%s' has a non-positive extent", name);
        e.ne[i] = ne[i];
        n *= ne[i];
    }
    if (data && dtype == gdt_i32) { // `data` points at int32 values: index constants (ggml_get_rows), kept as floats -- exact below 2^24
        const int32_t* idx = reinterpret_cast<const int32_t*>(data);
        e.data.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            if (idx[i] < -(1 << 24) || idx[i] > (1 << 24)) throw except("weights: i32 tensor '%s' holds %d (magnitudes up to 2^24)", name, idx[i]);
            e.data[(size_t)i] = (float)idx[i];
        }
    } else if (data) e.data.assign(data, data + n);
    else e.data.assign((size_t)n, 0.0f);
    ws.tensors.emplace(name, std::move(e));
}

std::shared_ptr<weight_store> weights_load(char const* path) { return weights_from_file(model_load(path)); }

std::shared_ptr<weight_store> weights_from_file(model_file const& f) {
    auto ws = weights_create();
    const bool file_whcn = f.tensor_layout() == layout_whcn;
    std::vector<int32_t> conv2d = f.conv2d_weights();
    std::vector<float> tmp, perm;
    for (int idx = 0; idx < (int)f.tensors.size(); ++idx) {
        gguf_tensor const& t = f.tensors[idx];
        if (t.type != GGML_F32 && t.type != GGML_F16) continue; // index tables etc. are not weights of this executor
        const int64_t n = t.n_elements();
        tmp.assign((size_t)n, 0.0f);
        if (!t.data) ws->no_data = true; // header-only read (a rank that receives the packed arena by broadcast): shapes only
        else if (t.type == GGML_F32) memcpy(tmp.data(), t.data, (size_t)n * 4);
        else
            for (int64_t i = 0; i < n; ++i) tmp[i] = f16_to_f32(reinterpret_cast<const uint16_t*>(t.data)[i]);
        int64_t ne[4] = {t.ne[0], t.ne[1], t.ne[2], t.ne[3]};
        const float* data = tmp.data();
        if (file_whcn && std::binary_search(conv2d.begin(), conv2d.end(), idx)) {
            // torch OIHW (ne [kw, kh, Cin, Cout]) -> OHWI (ne [Cin, kw, kh, Cout]): what model_transfer does for a cwhn backend (ml.cpp:449-498)
            const int64_t kw = ne[0], kh = ne[1], ci = ne[2], co = ne[3];
            perm.resize((size_t)n);
            for (int64_t o = 0; o < co; ++o)
                for (int64_t c = 0; c < ci; ++c)
                    for (int64_t y = 0; y < kh; ++y)
                        for (int64_t x = 0; x < kw; ++x) perm[((o * kh + y) * kw + x) * ci + c] = tmp[((o * ci + c) * kh + y) * kw + x];
            ne[0] = ci; ne[1] = kw; ne[2] = kh; ne[3] = co;
            data = perm.data();
        }
        weights_add(*ws, t.name.c_str(), t.type, ne, data);
    }
    return ws;
}

graph* graph_create(std::shared_ptr<weight_store> weights) {
    graph* g = new graph;
    g->store = weights ? std::move(weights) : weights_create();
    return g;
}

static void require_building(graph const& g, const char* what) {
    if (g.allocated) throw except("%s: the graph is already allocated (build a new one)", what);
}

int graph_find_weight(graph& g, char const* name) {
    std::string_view key(name ? name : "");
    auto it = g.weights.find(key);
    if (it != g.weights.end()) return it->second;
    auto st = g.store->tensors.find(key);
    if (st == g.store->tensors.end()) return -1;
    require_building(g, "model_ref::find");
    graph_node n;
    n.op = gop_weight;
    n.dtype = st->second.dtype;
    for (int i = 0; i < 4; ++i) n.ne[i] = st->second.ne[i];
    n.name = st->first;
    n.constant = true;
    n.cdata = st->second.data.data(); // std::map nodes do not move
    g.nodes.push_back(std::move(n));
    const int id = (int)g.nodes.size() - 1;
    g.weights.emplace(st->first, id);
    return id;
}

int graph_add_weight(graph& g, char const* name, int32_t dtype, const int64_t ne[4], const float* data) {
    require_building(g, "graph_add_weight");
    weights_add(*g.store, name, dtype, ne, data);
    return graph_find_weight(g, name);
}

int graph_input(graph& g, int32_t dtype, const int64_t ne[4], char const* name) {
    require_building(g, "graph_input");
    if (dtype != gdt_f32 && dtype != gdt_f16 && dtype != gdt_u8 && dtype != gdt_i32) throw except("graph_input: dtype %d (0 = f32, 1 = f16, 24 = u8 image bytes, 26 = i32 indices)", dtype);
    graph_node n;
    n.op = gop_input;
    n.dtype = dtype;
    for (int i = 0; i < 4; ++i) {
        if (ne[i] <= 0) throw except("graph_input: non-positive extent");
        n.ne[i] = ne[i];
    }
    n.name = name && *name ? name : "input";
    g.nodes.push_back(n);
    const int id = (int)g.nodes.size() - 1;
    g.named[g.nodes[id].name] = id;
    return id;
}

void graph_set_name(graph& g, int t, char const* name) {
    check_tensor(g, t, "graph_set_name");
    g.nodes[t].name = name ? name : "";
    if (name && *name) g.named[name] = t;
}

int graph_get_tensor(graph& g, char const* name) {
    auto it = g.named.find(std::string_view(name ? name : ""));
    if (it != g.named.end()) return it->second;
    return graph_find_weight(g, name);
}

void graph_output(graph& g, int t, char const* name) {
    require_building(g, "graph_output");
    check_tensor(g, t, "graph_output");
    g.nodes[t].is_output = true;
    if (name && *name) graph_set_name(g, t, name);
}

int graph_add(graph& g, int32_t op, const int* src, int n_src, const int64_t* ip, int n_ip, const float* fp, int n_fp) {
    require_building(g, "graph_add");
    if (op <= gop_weight || op >= gop_count) throw except("graph_add: op %d is not a node op", op);
    if (n_src < 1 || n_src > 4 || n_ip < 0 || n_ip > 12 || n_fp < 0 || n_fp > 8) throw except("graph_add(%s): bad argument counts", graph_op_name(op));
    graph_node n;
    n.op = op;
    n.n_src = n_src;
    for (int i = 0; i < n_src; ++i) {
        check_tensor(g, src[i], graph_op_name(op));
        n.src[i] = src[i];
    }
    for (int i = 0; i < n_ip; ++i) n.ip[i] = ip[i];
    for (int i = 0; i < n_fp; ++i) n.fp[i] = fp[i];
    auto S = [&](int i) -> graph_node const& { return g.nodes[n.src[i]]; };
    const char* nm = graph_op_name(op);
    auto need_src = [&](int lo, int hi) {
        if (n_src < lo || n_src > hi) throw except("%s: takes %d..%d tensors, got %d", nm, lo, hi, n_src);
    };
    auto same_shape = [&]() { for (int i = 0; i < 4; ++i) n.ne[i] = S(0).ne[i]; };
    n.dtype = gdt_f16;

    switch (op) {
        case gop_linear: {
            need_src(2, 3);
            graph_node const &x = S(0), &w = S(1);
            if (!w.constant) throw except("linear: the weight must be a model weight");
            if (w.ne[2] != 1 || w.ne[3] != 1 || w.ne[0] != x.ne[0])
                throw except("linear: weight %s does not match input %s", shape_str(w.ne).c_str(), shape_str(x.ne).c_str());
            if (n_src == 3 && S(2).n_elements() != w.ne[1]) throw except("linear: bias has %lld elements, expected %lld", (long long)S(2).n_elements(), (long long)w.ne[1]);
            same_shape();
            n.ne[0] = w.ne[1];
        } break;
        case gop_layer_norm:
            need_src(3, 3);
            if (S(1).n_elements() != S(0).ne[0] || S(2).n_elements() != S(0).ne[0]) throw except("layer_norm: weight / bias must have %lld elements", (long long)S(0).ne[0]);
            same_shape();
            break;
        case gop_gelu:
        case gop_relu:
        case gop_leaky_relu:
        case gop_scale:
        case gop_cont:
            need_src(1, 1);
            same_shape();
            if ((op == gop_relu || op == gop_scale) && !S(0).constant) n.dtype = S(0).dtype; // the f32 tail of a one-channel head
            break;
        case gop_add:
        case gop_mul: {
            need_src(2, 2);
            if (S(0).n_elements() < S(1).n_elements()) { std::swap(n.src[0], n.src[1]); } // commutative: the larger operand first
            broadcast_period(S(0).ne, S(1).ne, nm);
            same_shape();
        } break;
        case gop_conv_2d: {
            need_src(2, 3);
            graph_node const &x = S(0), &w = S(1);
            const int64_t stride = n.ip[0] > 0 ? n.ip[0] : 1, pad = n.ip[1];
            n.ip[0] = stride;
            if (!w.constant) throw except("conv_2d: the kernel must be a model weight");
            if (w.ne[0] != x.ne[0]) throw except("conv_2d: kernel %s (ne = [Cin, kw, kh, Cout]) does not match input %s (CWHN)", shape_str(w.ne).c_str(), shape_str(x.ne).c_str());
            if (n_src == 3 && S(2).n_elements() != w.ne[3]) throw except("conv_2d: bias has %lld elements, expected %lld", (long long)S(2).n_elements(), (long long)w.ne[3]);
            n.ne[0] = w.ne[3];
            n.ne[1] = (x.ne[1] + 2 * pad - w.ne[1]) / stride + 1;
            n.ne[2] = (x.ne[2] + 2 * pad - w.ne[2]) / stride + 1;
            n.ne[3] = x.ne[3];
            if (n.ne[1] <= 0 || n.ne[2] <= 0) throw except("conv_2d: the kernel does not fit the input");
            // a 1x1 convolution to ONE channel is a model's final map (depth-anything.cpp:91-94): kept in f32, like the static schedule's output
            if (w.ne[3] == 1 && w.ne[1] == 1 && w.ne[2] == 1 && stride == 1 && pad == 0) n.dtype = gdt_f32;
            // ... and so is a 3x3 convolution to an RGB image (esrgan.cpp:75)
            if (w.ne[3] == 3 && w.ne[1] == 3 && w.ne[2] == 3 && stride == 1 && pad == 1) n.dtype = gdt_f32;
        } break;
        case gop_conv_transpose_2d: {
            need_src(2, 3);
            graph_node const &x = S(0), &w = S(1);
            const int64_t stride = n.ip[0];
            if (!w.constant) throw except("conv_transpose_2d: the kernel must be a model weight");
            if (w.ne[3] != x.ne[0]) throw except("conv_transpose_2d: kernel %s (ne = [kw, kh, Cout, Cin]) does not match input %s", shape_str(w.ne).c_str(), shape_str(x.ne).c_str());
            if (w.ne[0] != stride || w.ne[1] != stride) throw except("conv_transpose_2d: kernel %lldx%lld with stride %lld is not built (kernel == stride is)", (long long)w.ne[0], (long long)w.ne[1], (long long)stride);
            if (n_src == 3 && S(2).n_elements() != w.ne[2]) throw except("conv_transpose_2d: bias has %lld elements, expected %lld", (long long)S(2).n_elements(), (long long)w.ne[2]);
            n.ne[0] = w.ne[2];
            n.ne[1] = x.ne[1] * stride;
            n.ne[2] = x.ne[2] * stride;
            n.ne[3] = x.ne[3];
        } break;
        case gop_interpolate:
            need_src(1, 1);
            if (n.ip[0] <= 0 || n.ip[1] <= 0) throw except("interpolate: non-positive target extent");
            same_shape();
            n.ne[1] = n.ip[0];
            n.ne[2] = n.ip[1];
            if (is_f32_image(S(0))) { // downscale_by(image, 2) (birefnet.cpp:36-41): an f32 image again, for every reader of the input image
                if ((n.ip[2] & 255) != 1 || !(n.ip[2] & 256))
                    throw except("interpolate: mode %lld (%s%s) on an f32 image is not built (bilinear | align_corners is)", (long long)n.ip[2],
                                 (n.ip[2] & 255) == 0 ? "nearest" : ((n.ip[2] & 255) == 1 ? "bilinear" : ((n.ip[2] & 255) == 2 ? "bicubic" : "unknown")), n.ip[2] & 256 ? " | align_corners" : "");
                n.dtype = gdt_f32;
            }
            break;
        case gop_image_patches: {
            need_src(1, 1);
            graph_node const& x = S(0);
            const int64_t w = n.ip[0], h = n.ip[1];
            if (!is_f32_image(x)) throw except("image_patches: the operand is an f32 image [C <= 4, W, H, N] (the graph input, or interpolate of it), not %s %s", x.constant ? "the constant" : (x.dtype == gdt_f32 ? "the f32 tensor" : "the f16 / integer tensor"), shape_str(x.ne).c_str());
            if (n_ip != 2 || w <= 0 || h <= 0) throw except("image_patches: two positive integer parameters (w, h of the patch map)");
            if (x.ne[1] % w || x.ne[2] % h) throw except("image_patches: Grid must divide image size (image %lldx%lld, patches %lldx%lld)", (long long)x.ne[1], (long long)x.ne[2], (long long)w, (long long)h);
            const int64_t gw = x.ne[1] / w, gh = x.ne[2] / h;
            if (gw * gh * x.ne[0] % 8) throw except("image_patches: grid %lldx%lld of a %lld-channel image gives %lld channels (a multiple of 8; at grid 1 a conv reads the image itself)", (long long)gw, (long long)gh, (long long)x.ne[0], (long long)(gw * gh * x.ne[0]));
            n.ne[0] = gw * gh * x.ne[0]; n.ne[1] = w; n.ne[2] = h; n.ne[3] = x.ne[3];
        } break;
        case gop_attention: {
            need_src(3, 3);
            graph_node const &q = S(0), &k = S(1), &v = S(2);
            for (int i = 0; i < 4; ++i)
                if (k.ne[i] != v.ne[i] || (i != 2 && q.ne[i] != k.ne[i])) throw except("attention: q %s, k %s, v %s do not match ([head_dim, heads, tokens, batch])", shape_str(q.ne).c_str(), shape_str(k.ne).c_str(), shape_str(v.ne).c_str());
            n.ne[0] = q.ne[0] * q.ne[1];
            n.ne[1] = q.ne[2];
            n.ne[2] = q.ne[3];
            n.ne[3] = 1;
        } break;
        case gop_concat: {
            need_src(2, 2);
            const int64_t dim = n.ip[0];
            if (dim < 0 || dim > 3) throw except("concat: dimension %lld", (long long)dim);
            same_shape();
            for (int i = 0; i < 4; ++i)
                if (i != dim && S(0).ne[i] != S(1).ne[i]) throw except("concat: %s and %s differ outside dimension %lld", shape_str(S(0).ne).c_str(), shape_str(S(1).ne).c_str(), (long long)dim);
            n.ne[dim] = S(0).ne[dim] + S(1).ne[dim];
        } break;
        case gop_slice:
            need_src(1, 1);
            for (int d = 0; d < 4; ++d) {
                int64_t &b = n.ip[3 * d], &e = n.ip[3 * d + 1], &s = n.ip[3 * d + 2];
                const int64_t ext = S(0).ne[d];
                if (s <= 0) s = 1;
                if (b < 0) b += ext; // python-style negative indices (ml.cpp:752-756)
                if (e < 0) e += ext;
                e = std::min(e, ext);
                if (b < 0 || b >= e) throw except("slice: empty or out-of-range selection in dimension %d of %s", d, shape_str(S(0).ne).c_str());
                n.ne[d] = (e - b + s - 1) / s;
            }
            break;
        case gop_reshape: {
            need_src(1, 1);
            int64_t total = 1;
            for (int i = 0; i < 4; ++i) {
                if (n.ip[i] <= 0) throw except("reshape: non-positive extent");
                n.ne[i] = n.ip[i];
                total *= n.ip[i];
            }
            if (total != S(0).n_elements()) throw except("reshape: %s has %lld elements, the target %s has %lld", shape_str(S(0).ne).c_str(), (long long)S(0).n_elements(), shape_str(n.ne).c_str(), (long long)total);
        } break;
        case gop_repeat:
            need_src(1, 1);
            for (int i = 0; i < 4; ++i) {
                n.ne[i] = n.ip[i];
                const bool tiles = S(0).constant && n.ip[i] > 0 && n.ip[i] % S(0).ne[i] == 0; // a constant is tiled on the host (ggml_repeat: out[i] = src[i mod ne_src])
                if (n.ip[i] <= 0 || (S(0).ne[i] != 1 && S(0).ne[i] != n.ip[i] && !tiles)) throw except("repeat: %s to %s (source dimensions must be 1 or already equal)", shape_str(S(0).ne).c_str(), shape_str(n.ip).c_str());
            }
            break;
        case gop_patch_embed: {
            need_src(2, 3);
            graph_node const &x = S(0), &w = S(1);
            const int64_t ps = n.ip[0];
            if (!w.constant) throw except("patch_embed: the kernel must be a model weight");
            if (x.dtype != gdt_f32) throw except("patch_embed: the input image tensor is f32 (the tensor the reference uploads, or image_u8_to_f32 of a u8 input)");
            if (ps <= 0 || w.ne[1] != ps || w.ne[2] != ps || w.ne[0] != x.ne[0]) throw except("patch_embed: kernel %s does not match patch size %lld and input %s", shape_str(w.ne).c_str(), (long long)ps, shape_str(x.ne).c_str());
            if (x.ne[1] % ps || x.ne[2] % ps) throw except("patch_embed: extent %lldx%lld is not a multiple of the patch size %lld", (long long)x.ne[1], (long long)x.ne[2], (long long)ps);
            n.ne[0] = w.ne[3];
            n.ne[1] = x.ne[1] / ps;
            n.ne[2] = x.ne[2] / ps;
            n.ne[3] = x.ne[3];
        } break;
        case gop_image_u8_to_f32: {
            need_src(1, 1);
            graph_node const& x = S(0);
            if (x.op != gop_input || x.dtype != gdt_u8 || x.ne[0] != 3) throw except("image_u8_to_f32: the operand is a u8 input tensor [3, W, H, N]");
            if (n_fp != 6) throw except("image_u8_to_f32: six float parameters (mean r g b, 1 / std r g b)");
            same_shape();
            n.dtype = gdt_f32;
        } break;
        case gop_image_normalize: {
            need_src(1, 1);
            if (S(0).constant || S(0).dtype != gdt_f32 || S(0).ne[0] != 1) throw except("image_normalize: the operand is a one-channel f32 map [1, W, H, N]");
            same_shape();
            n.dtype = gdt_f32;
        } break;
        case gop_permute: {
            need_src(1, 1);
            bool seen[4] = {false, false, false, false};
            for (int d = 0; d < 4; ++d) {
                if (n_ip != 4 || n.ip[d] < 0 || n.ip[d] > 3 || seen[n.ip[d]]) throw except("permute: the axes must be a permutation of 0..3 (ggml_permute: source dimension d becomes dimension axes[d])");
                seen[n.ip[d]] = true;
                n.ne[n.ip[d]] = S(0).ne[d];
            }
            n.dtype = S(0).dtype;
        } break;
        case gop_roll:
            need_src(1, 1);
            if (n_ip != 4) throw except("roll: four shifts");
            same_shape();
            n.dtype = S(0).dtype;
            break;
        case gop_pad:
            need_src(1, 1);
            for (int d = 0; d < 4; ++d) {
                if (n_ip != 4 || n.ip[d] < 0) throw except("pad: four non-negative paddings (zeros are appended at the end of a dimension)");
                n.ne[d] = S(0).ne[d] + n.ip[d];
            }
            n.dtype = S(0).dtype;
            break;
        case gop_get_rows: {
            need_src(2, 2);
            graph_node const &tab = S(0), &idx = S(1);
            const bool runtime_idx = idx.dtype == gdt_i32 && idx.op == gop_input; // the token ids of clip_text_embed (sam3.h:225): gathered on the device
            if (idx.dtype != gdt_i32 || (!idx.constant && !runtime_idx)) throw except("get_rows: the index is an i32 constant (visp_graph_add_weight with dtype 26)");
            if (tab.ne[2] != 1 || tab.ne[3] != 1 || idx.ne[3] != 1) throw except("get_rows: table %s must be a matrix, index %s at most 3-dimensional", shape_str(tab.ne).c_str(), shape_str(idx.ne).c_str());
            if (tab.dtype == gdt_i32) throw except("get_rows: the table is an f16 / f32 tensor");
            n.ne[0] = tab.ne[0]; n.ne[1] = idx.ne[0]; n.ne[2] = idx.ne[1]; n.ne[3] = idx.ne[2];
            n.dtype = gdt_f32; // ggml: the result of get_rows is always f32
            if (runtime_idx && tab.constant) { // ... but activations of this layer are f16: a gather at run time gives an f16 activation
                if (tab.ne[0] % 8) throw except("get_rows: a table of %lld channels with a run-time index (a multiple of 8)", (long long)tab.ne[0]);
                n.dtype = gdt_f16;
            }
        } break;
        case gop_cast:
            need_src(1, 1);
            if (n_ip != 1 || (n.ip[0] != gdt_f32 && n.ip[0] != gdt_f16)) throw except("cast: the target type is 0 (f32) or 1 (f16)");
            if (S(0).dtype == gdt_i32) throw except("cast: an i32 tensor is an index, not a value");
            if (!S(0).constant && S(0).dtype != n.ip[0]) throw except("cast: an %s activation to %s is not built (activations of this layer are f16; a cast to the type they have is a view)", S(0).dtype == gdt_f16 ? "f16" : "f32", n.ip[0] == gdt_f16 ? "f16" : "f32");
            same_shape();
            n.dtype = (int32_t)n.ip[0];
            break;
        case gop_attention_masked: {
            need_src(4, 4);
            graph_node const &q = S(0), &k = S(1), &v = S(2), &mk = S(3);
            for (int i = 0; i < 4; ++i)
                if (k.ne[i] != v.ne[i] || (i != 2 && q.ne[i] != k.ne[i])) throw except("attention_masked: q %s, k %s, v %s do not match ([head_dim, heads, tokens, batch])", shape_str(q.ne).c_str(), shape_str(k.ne).c_str(), shape_str(v.ne).c_str());
            if (q.ne[2] != k.ne[2]) throw except("attention_masked: %lld queries on %lld keys; cross-attention (T_q != T_k) is not built", (long long)q.ne[2], (long long)k.ne[2]);
            if (q.ne[0] != 32 && q.ne[0] != 64) throw except("attention_masked: head_dim %lld; the masked kernel is built for head_dim 32 and 64", (long long)q.ne[0]);
            if (mk.dtype != gdt_f16 && mk.dtype != gdt_f32) throw except("attention_masked: the mask is an f16 or f32 tensor");
            if (mk.ne[0] != k.ne[2] || mk.ne[1] != q.ne[2]) throw except("attention_masked: mask %s does not match %lld keys x %lld queries ([T_k, T_q, Hm, Bm])", shape_str(mk.ne).c_str(), (long long)k.ne[2], (long long)q.ne[2]);
            if (mk.ne[2] != 1 && mk.ne[2] != q.ne[1]) throw except("attention_masked: the mask has %lld heads; 1 (broadcast) or %lld", (long long)mk.ne[2], (long long)q.ne[1]);
            if (q.ne[3] % mk.ne[3]) throw except("attention_masked: the mask's batch %lld does not divide the batch %lld (batch b reads mask b %% Bm)", (long long)mk.ne[3], (long long)q.ne[3]);
            n.ne[0] = q.ne[0] * q.ne[1];
            n.ne[1] = q.ne[2];
            n.ne[2] = q.ne[3];
            n.ne[3] = 1;
        } break;
        case gop_sigmoid:
        case gop_silu:
        case gop_sin:
        case gop_cos:
            need_src(1, 1);
            same_shape();
            break;
        case gop_attention_cross: {
            need_src(3, 3);
            graph_node const &q = S(0), &k = S(1), &v = S(2);
            for (int i = 0; i < 4; ++i)
                if (k.ne[i] != v.ne[i] || (i != 2 && q.ne[i] != k.ne[i]))
                    throw except("attention_cross: q %s, k %s, v %s do not match (q [head_dim, heads, T_q, batch]; k, v [head_dim, heads, T_k, batch])", shape_str(q.ne).c_str(), shape_str(k.ne).c_str(), shape_str(v.ne).c_str());
            if (q.ne[0] != 16 && q.ne[0] != 32 && q.ne[0] != 64) throw except("attention_cross: head_dim %lld; the kernel is built for head_dim 16, 32 and 64", (long long)q.ne[0]);
            for (int i = 0; i < 3; ++i)
                if (S(i).constant || S(i).dtype != gdt_f16) throw except("attention_cross: operand %d (%s) is %s; q, k and v are f16 activations", i, i == 0 ? "q" : (i == 1 ? "k" : "v"), S(i).constant ? "a constant" : "f32");
            n.ne[0] = q.ne[0] * q.ne[1];
            n.ne[1] = q.ne[2];
            n.ne[2] = q.ne[3];
            n.ne[3] = 1;
        } break;
        case gop_mul_mat: {
            need_src(2, 2);
            graph_node const &a = S(0), &b = S(1);
            const int64_t K = a.ne[0], M = a.ne[1], Ba = a.ne[2], N = b.ne[1], B = b.ne[2];
            if (b.ne[0] != K || a.ne[3] != 1 || b.ne[3] != 1) throw except("mul_mat: a %s and b %s do not match (a [K, M, Ba], b [K, N, B] -> [M, N, B])", shape_str(a.ne).c_str(), shape_str(b.ne).c_str());
            if (Ba != 1 && Ba != B) throw except("mul_mat: the first operand's batch %lld is neither 1 nor the second's %lld", (long long)Ba, (long long)B);
            if (a.dtype == gdt_i32 || b.dtype == gdt_i32) throw except("mul_mat: an i32 tensor is an index, not a value");
            n.ne[0] = M; n.ne[1] = N; n.ne[2] = B; n.ne[3] = 1;
            if (a.constant && b.constant) break; // folded on the host
            if (!a.constant && b.constant) throw except("mul_mat: the second operand is a constant and the first an activation; this product is not built (swap the roles: LINEAR takes the constant as its weight)");
            if (a.constant) {
                // a constant [2, F] on the f32 coordinates: the head of position_embedding_random's chain (mobile-sam.cpp:243), lowered with it as one launch
                if (K == 2 && b.op == gop_input && b.dtype == gdt_f32) break;
                if (K == 2) throw except("mul_mat: a constant first operand with K = 2 is built on an f32 graph input only (the coordinates of position_embedding_random), not on an f16 activation");
                throw except("mul_mat: the first operand is a constant; use LINEAR (linear(x, w) is mul_mat(w, x) with w as the layer's weight) -- mul_mat is built for two activations, and for a constant [2, F] on f32 coordinates");
            }
            if (a.dtype != gdt_f16 || b.dtype != gdt_f16) throw except("mul_mat: operands of two activations are f16 (a is %s, b is %s)", a.dtype == gdt_f16 ? "f16" : "f32", b.dtype == gdt_f16 ? "f16" : "f32");
            if (K % 8 || K > 256) throw except("mul_mat: K = %lld; two activations are multiplied for K a multiple of 8, at most 256", (long long)K);
            if (N > 16) throw except("mul_mat: N = %lld columns in the second operand; at most 16 (one thread per row of the first keeps them in registers)", (long long)N);
        } break;
        case gop_rope: {
            need_src(2, 2);
            graph_node const &x = S(0), &pos = S(1);
            if (n_ip < 1 || n_fp != 2) throw except("rope: one or two integer parameters (n_dims, mode) and two float parameters (freq_base, freq_scale)");
            if (n_ip > 1 && n.ip[1] != 0) throw except("rope: mode %lld is not built (0, GGML_ROPE_TYPE_NORMAL: adjacent pairs, is)", (long long)n.ip[1]);
            if (x.constant || x.dtype != gdt_f16) throw except("rope: x is %s; the operand is an f16 activation [n, heads, T, B]", x.constant ? "a constant" : "f32");
            if (!pos.constant || pos.dtype != gdt_i32) throw except("rope: the positions are an i32 constant [T] (visp_graph_add_weight with dtype 26), not %s", pos.constant ? "an f16 / f32 constant" : "an activation");
            if (pos.ne[0] != x.ne[2] || pos.n_elements() != pos.ne[0]) throw except("rope: positions %s do not match the %lld tokens of x %s", shape_str(pos.ne).c_str(), (long long)x.ne[2], shape_str(x.ne).c_str());
            if (n.ip[0] != x.ne[0]) throw except("rope: n_dims %lld on rows of %lld channels; the op is built for n_dims == ne[0] (slice the part to rotate)", (long long)n.ip[0], (long long)x.ne[0]);
            if (x.ne[0] % 8) throw except("rope: rows of %lld channels (a multiple of 8)", (long long)x.ne[0]);
            if (!(n.fp[0] > 0.0f) || !std::isfinite(n.fp[0]) || !std::isfinite(n.fp[1])) throw except("rope: freq_base %g, freq_scale %g (a positive base, finite)", (double)n.fp[0], (double)n.fp[1]);
            same_shape();
        } break;
        case gop_clamp:
            need_src(1, 1);
            if (n_fp != 2) throw except("clamp: two float parameters (lower bound, upper bound)");
            if (!std::isfinite(n.fp[0]) || !std::isfinite(n.fp[1])) throw except("clamp: bounds %g .. %g; both must be finite", (double)n.fp[0], (double)n.fp[1]);
            if (n.fp[0] > n.fp[1]) throw except("clamp: lower bound %g above upper bound %g", (double)n.fp[0], (double)n.fp[1]);
            same_shape();
            break;
        case gop_sub: // not commutative: the operands stay where they are, so the first one is the larger
            need_src(2, 2);
            broadcast_period(S(0).ne, S(1).ne, nm);
            same_shape();
            break;
        case gop_soft_max:
            need_src(1, 1);
            if (S(0).ne[0] % 8 || S(0).ne[0] > 1024) throw except("soft_max: rows of %lld elements (a multiple of 8, at most 1024)", (long long)S(0).ne[0]);
            same_shape();
            break;
        case gop_sum_rows:
            need_src(1, 1);
            same_shape();
            n.ne[0] = 1;
            break;
        case gop_pool_2d: {
            need_src(1, 1);
            graph_node const& x = S(0);
            const int64_t kind = n.ip[0], kw = n.ip[1], kh = n.ip[2], sw = n.ip[3], sh = n.ip[4], pw = n.ip[5], ph = n.ip[6], C = x.ne[0];
            if (n_ip != 7) throw except("pool_2d: seven integer parameters (kind, kernel w h, stride w h, pad w h)");
            if (kind != 0 && kind != 1) throw except("pool_2d: kind %lld (0 max, 1 average)", (long long)kind);
            if (kw != kh) throw except("pool_2d: kernel %lldx%lld; square kernels only", (long long)kw, (long long)kh);
            if (sw != sh) throw except("pool_2d: strides %lld and %lld; equal strides only", (long long)sw, (long long)sh);
            if (sw != 1 && sw != 2) throw except("pool_2d: stride %lld is not built (1 and 2 are)", (long long)sw);
            if (kw < 1 || kw > 13) throw except("pool_2d: kernel %lldx%lld; kernels 1x1 up to 13x13", (long long)kw, (long long)kh);
            if (pw != ph || pw < 0 || pw > kw / 2) throw except("pool_2d: pad %lld, %lld with a %lldx%lld kernel (equal, 0 .. k / 2)", (long long)pw, (long long)ph, (long long)kw, (long long)kh);
            if (kind == 1 && pw > 0) throw except("pool_2d: average pooling with pad %lld is not built (pad 0 is; the divisor at the border would be a convention)", (long long)pw);
            if (C % 8) throw except("pool_2d: C = %lld must be a multiple of 8", (long long)C);
            n.ne[0] = C;
            n.ne[1] = x.ne[1] + 2 * pw - kw < 0 ? 0 : (x.ne[1] + 2 * pw - kw) / sw + 1;
            n.ne[2] = x.ne[2] + 2 * pw - kh < 0 ? 0 : (x.ne[2] + 2 * pw - kh) / sw + 1;
            n.ne[3] = x.ne[3];
            if (n.ne[1] < 1 || n.ne[2] < 1) throw except("pool_2d: a %lldx%lld kernel at pad %lld does not fit the %lldx%lld input", (long long)kw, (long long)kh, (long long)pw, (long long)x.ne[1], (long long)x.ne[2]);
        } break;
        case gop_mean_2d:
            need_src(1, 1);
            n.ne[0] = S(0).ne[0]; n.ne[1] = 1; n.ne[2] = 1; n.ne[3] = S(0).ne[3];
            break;
        case gop_conv_2d_deform: {
            need_src(3, 4);
            graph_node const &x = S(0), &w = S(1), &off = S(2);
            const int64_t stride = n.ip[0] > 0 ? n.ip[0] : 1, pad = n.ip[1];
            n.ip[0] = stride;
            if (!w.constant) throw except("conv_2d_deform: the kernel must be a model weight");
            if (stride != 1) throw except("conv_2d_deform: stride %lld is not built (stride 1 is)", (long long)stride);
            if (w.ne[1] != w.ne[2]) throw except("conv_2d_deform: kernel %lldx%lld; square kernels only", (long long)w.ne[1], (long long)w.ne[2]);
            if (w.ne[1] > 7 || pad < 0) throw except("conv_2d_deform: kernel %lld, pad %lld (kernels up to 7x7, pad >= 0)", (long long)w.ne[1], (long long)pad);
            if (w.ne[0] != x.ne[0]) throw except("conv_2d_deform: kernel %s (ne = [Cin, kw, kh, Cout]) does not match input %s (CWHN)", shape_str(w.ne).c_str(), shape_str(x.ne).c_str());
            if (x.ne[0] % 16) throw except("conv_2d_deform: Cin = %lld must be a multiple of 16", (long long)x.ne[0]);
            if (w.ne[3] > 256) throw except("conv_2d_deform: Cout = %lld; one block computes every output channel of its pixels, at most 256", (long long)w.ne[3]);
            if (w.ne[3] % 8) throw except("conv_2d_deform: Cout = %lld must be a multiple of 8", (long long)w.ne[3]);
            const int64_t taps = w.ne[1] * w.ne[2];
            n.ne[0] = w.ne[3];
            n.ne[1] = x.ne[1] + 2 * pad - w.ne[1] + 1;
            n.ne[2] = x.ne[2] + 2 * pad - w.ne[2] + 1;
            n.ne[3] = x.ne[3];
            if (n.ne[1] <= 0 || n.ne[2] <= 0) throw except("conv_2d_deform: the kernel does not fit the input");
            auto matches = [&](graph_node const& t, int64_t ch) { return t.ne[0] == ch && t.ne[1] == n.ne[1] && t.ne[2] == n.ne[2] && t.ne[3] == n.ne[3] && t.dtype != gdt_i32; };
            if (!matches(off, 2 * taps))
                throw except("conv_2d_deform: offset %s does not match a %lldx%lld kernel on a %lldx%lld output ([2 kh kw, OW, OH, N] = [%lld, %lld, %lld, %lld])", shape_str(off.ne).c_str(),
                             (long long)w.ne[1], (long long)w.ne[2], (long long)n.ne[1], (long long)n.ne[2], (long long)(2 * taps), (long long)n.ne[1], (long long)n.ne[2], (long long)n.ne[3]);
            if (n_src == 4 && !matches(S(3), taps))
                throw except("conv_2d_deform: mask %s does not match a %lldx%lld kernel on a %lldx%lld output ([kh kw, OW, OH, N] = [%lld, %lld, %lld, %lld])", shape_str(S(3).ne).c_str(),
                             (long long)w.ne[1], (long long)w.ne[2], (long long)n.ne[1], (long long)n.ne[2], (long long)taps, (long long)n.ne[1], (long long)n.ne[2], (long long)n.ne[3]);
        } break;
        case gop_conv_2d_depthwise: {
            need_src(2, 3);
            graph_node const &x = S(0), &w = S(1);
            const int64_t stride = n.ip[0] > 0 ? n.ip[0] : 1, pad = n.ip[1], C = x.ne[0];
            n.ip[0] = stride;
            if (!w.constant) throw except("conv_2d_depthwise: the kernel must be a model weight (a constant)");
            // the two forms the weight store hands over: [C, 1, kw, kh] (written NHWC, nn.cpp:106 permutes it) and [1, kw, kh, C] (a depthwise OIHW kernel
            // listed in conv2d_weights)
            int64_t kw, kh;
            if (w.ne[0] == C && w.ne[1] == 1) { kw = w.ne[2]; kh = w.ne[3]; }
            else if (w.ne[0] == 1 && w.ne[3] == C) { kw = w.ne[1]; kh = w.ne[2]; }
            else throw except("conv_2d_depthwise: kernel %s is neither [C, 1, kw, kh] nor [1, kw, kh, C] for input %s (CWHN)", shape_str(w.ne).c_str(), shape_str(x.ne).c_str());
            if (stride != 1 && stride != 2) throw except("conv_2d_depthwise: stride %lld is not built (1 and 2 are)", (long long)stride);
            if (kw != kh) throw except("conv_2d_depthwise: kernel %lldx%lld; square kernels only", (long long)kw, (long long)kh);
            if (kw > 7) throw except("conv_2d_depthwise: kernel %lldx%lld; kernels up to 7x7", (long long)kw, (long long)kh);
            if (pad < 0 || pad > kw - 1) throw except("conv_2d_depthwise: pad %lld with a %lldx%lld kernel (0 .. k - 1)", (long long)pad, (long long)kw, (long long)kh);
            if (C % 8) throw except("conv_2d_depthwise: C = %lld must be a multiple of 8", (long long)C);
            if (n_src == 3 && (!S(2).constant || S(2).n_elements() != C)) throw except("conv_2d_depthwise: bias has %lld elements, expected %lld (a constant)", (long long)S(2).n_elements(), (long long)C);
            n.ne[0] = C;
            n.ne[1] = x.ne[1] + 2 * pad - kw < 0 ? 0 : (x.ne[1] + 2 * pad - kw) / stride + 1;
            n.ne[2] = x.ne[2] + 2 * pad - kh < 0 ? 0 : (x.ne[2] + 2 * pad - kh) / stride + 1;
            n.ne[3] = x.ne[3];
            if (n.ne[1] < 1 || n.ne[2] < 1) throw except("conv_2d_depthwise: a %lldx%lld kernel at pad %lld does not fit the %lldx%lld input", (long long)kw, (long long)kh, (long long)pad, (long long)x.ne[1], (long long)x.ne[2]);
        } break;
        default: throw except("graph_add: op %d", op);
    }
    // f32 tensors exist as inputs only; an f32 operand anywhere else would need kernels this executor does not have
    if (op != gop_patch_embed && op != gop_image_u8_to_f32 && op != gop_image_normalize && op != gop_image_patches && !(op == gop_interpolate && is_f32_image(S(0))))
        for (int i = 0; i < n_src; ++i) {
            const bool head_tail = (op == gop_relu || op == gop_scale || op == gop_sigmoid) && S(i).op != gop_input; // (sigmoid: f32 in, f16 out)
            // (a 3x3 conv on the f32 image of <= 16 channels: the first conv of an image-to-image network, esrgan.cpp:58)
            const bool image_conv = op == gop_conv_2d && i == 0 && S(0).op == gop_input && S(0).ne[0] <= 16 && S(1).ne[1] == 3 && S(1).ne[2] == 3 && n.ip[0] == 1 && n.ip[1] == 1;
            const bool f32_mask = op == gop_attention_masked && i == 3; // the masked attention reads an f32 mask in place
            // (any conv on a 3- or 4-channel f32 image: image_pad8 in front of the GEMM family's conv, mobile-sam.cpp:71-73, migan.cpp:84-86)
            const bool image8_conv = op == gop_conv_2d && i == 0 && S(0).dtype == gdt_f32 && (S(0).ne[0] == 3 || S(0).ne[0] == 4);
            const bool fourier_head = op == gop_mul_mat && i == 1 && S(0).constant && S(0).ne[0] == 2 && S(1).op == gop_input; // (checked above)
            const bool row_index = op == gop_get_rows && i == 1; // (an i32 graph input, checked above)
            if (!S(i).constant && S(i).dtype == gdt_i32 && !row_index) throw except("%s: operand %d is an i32 graph input; an i32 tensor is an index, not a value (get_rows reads one)", nm, i);
            if (!S(i).constant && S(i).dtype != gdt_f16 && !head_tail && !image_conv && !image8_conv && !f32_mask && !fourier_head && !row_index)
                throw except("%s: operand %d is f32; only patch_embed and an image's first 3x3 conv read the f32 input tensor", nm, i);
        }

    bool all_const = true;
    for (int i = 0; i < n_src; ++i) all_const = all_const && S(i).constant;
    if (all_const && foldable(op)) {
        n.constant = true;
        fold_constant(g, n);
    } else if (all_const) {
        throw except("%s: every operand is a constant; the executor computes this op on activations only", nm);
    }
    g.nodes.push_back(std::move(n));
    return (int)g.nodes.size() - 1;
}

device_span build_weight_arena(weight_store& ws, backend_device const& dev, std::function<std::unique_ptr<graph>()> const& make_graph) {
    size_t need = 0;
    {
        std::unique_ptr<graph> plan = make_graph();
        graph_allocate(*plan, nullptr);
        need = plan->plan_store_bytes;
    }
    ws.arena = device_buffer(need + (1u << 20));
    graph_allocate(*make_graph(), &dev);
    return {ws.arena.ptr, round_up<size_t>(ws.arena_used, 256)};
}

void graph_allocate(graph& g, backend_device const* dev) {
    if (g.allocated) return;
    g.dev = dev;
    std::optional<device_turn> turn; // the arena, the packed weights and the kernel attributes belong to THIS device; uploads use its stream
    if (dev) {
        turn.emplace(*dev);
        std::lock_guard<std::mutex> lock(g.store->mutex);
        if (g.store->dev && g.store->dev != dev) throw except("compute_graph_allocate: the weights of this graph live on another device");
        g.store->dev = dev;
    }
    lowering low(g);
    low.run();
    if (g.dev) {
        g.arena = device_buffer(g.arena_bytes);
        VX(vx_memset(g.arena.ptr, 0, g.arena_bytes, g.dev->stream));
        VX(vx_stream_sync(g.dev->stream));
    }
    g.allocated = true;
}

static void require_device(graph const& g, const char* what) {
    if (!g.allocated) throw except("%s: call compute_graph_allocate first", what);
    if (!g.dev) throw except("%s: this graph was made without a device (planning only)", what);
}

void graph_compute(graph& g) {
    require_device(g, "compute");
    device_turn turn(*g.dev);
    void* st = g.dev->stream;
    if (g.use_hip_graph && g.graph_exec) {
        g.graph_exec.launch(st);
        VX(vx_stream_sync(st));
        return;
    }
    for (auto& l : g.launches) l.run(st);
    VX(vx_stream_sync(st));
    if (g.use_hip_graph) // the eager pass above set every kernel attribute; now record the same launches once
        g.graph_exec = capture(st, [&] {
            for (auto& l : g.launches) l.run(st);
        });
}

static char* tensor_ptr(graph& g, int t, const char* what) {
    check_tensor(g, t, what);
    int r = t;
    while (g.nodes[r].alias_of >= 0) r = g.nodes[r].alias_of;
    graph_node const& n = g.nodes[r];
    if (n.buffer < 0) throw except("%s: tensor %d (%s) has no storage (a constant, fused away, or not needed by any output)", what, t, graph_op_name(g.nodes[t].op));
    if (!g.buffers[n.buffer].persistent) throw except("%s: tensor %d (%s) is an intermediate whose buffer is recycled; mark it with compute_graph_output", what, t, graph_op_name(g.nodes[t].op));
    return static_cast<char*>(g.arena.ptr) + g.buffers[n.buffer].offset;
}

void graph_tensor_set(graph& g, int t, const void* data, size_t bytes) {
    require_device(g, "transfer_to_backend");
    device_turn turn(*g.dev);
    char* p = tensor_ptr(g, t, "transfer_to_backend");
    if (bytes != g.nodes[t].n_bytes()) throw except("transfer_to_backend: %zu bytes for a tensor of %zu", bytes, g.nodes[t].n_bytes());
    VX(vx_memcpy_h2d(p, data, bytes, g.dev->stream));
    VX(vx_stream_sync(g.dev->stream));
}

void graph_tensor_get(graph& g, int t, void* data, size_t bytes, bool as_f32) {
    require_device(g, "transfer_from_backend");
    device_turn turn(*g.dev);
    char* p = tensor_ptr(g, t, "transfer_from_backend");
    graph_node const& n = g.nodes[t];
    const bool convert = as_f32 && n.dtype == gdt_f16;
    const size_t want = convert ? (size_t)n.n_elements() * 4 : n.n_bytes();
    if (bytes != want) throw except("transfer_from_backend: %zu bytes for a tensor of %zu", bytes, want);
    if (!convert) {
        VX(vx_memcpy_d2h(data, p, bytes, g.dev->stream));
        VX(vx_stream_sync(g.dev->stream));
        return;
    }
    std::vector<uint16_t> h((size_t)n.n_elements());
    VX(vx_memcpy_d2h(h.data(), p, h.size() * 2, g.dev->stream));
    VX(vx_stream_sync(g.dev->stream));
    float* out = static_cast<float*>(data);
    for (size_t i = 0; i < h.size(); ++i) out[i] = f16_to_f32(h[i]);
}

void graph_bind_external(graph& g, int t, void* ptr) {
    if (!g.allocated) throw except("graph_bind_external: call compute_graph_allocate first");
    check_tensor(g, t, "graph_bind_external");
    int r = t;
    while (g.nodes[r].alias_of >= 0) r = g.nodes[r].alias_of;
    graph_node const& n = g.nodes[r];
    if (n.buffer < 0 || !g.buffers[n.buffer].persistent) throw except("graph_bind_external: tensor %d is not an input or output of the graph", t);
    g.buffers[n.buffer].external = ptr;
}
void* graph_tensor_device_ptr(graph& g, int t) {
    require_device(g, "graph_tensor_device_ptr");
    char* p = tensor_ptr(g, t, "graph_tensor_device_ptr");
    int r = t;
    while (g.nodes[r].alias_of >= 0) r = g.nodes[r].alias_of;
    graph_buffer const& b = g.buffers[g.nodes[r].buffer];
    return b.external ? b.external : p;
}

std::string graph_describe(graph const& g) {
    std::string s;
    for (auto const& l : g.launches) { s += l.desc; s += '\n'; }
    char b[256];
    snprintf(b, sizeof b, "launches=%zu nodes=%zu buffers=%zu arena_bytes=%zu unshared_bytes=%zu constant_bytes=%zu\n", g.launches.size(), g.nodes.size(), g.buffers.size(),
             g.arena_bytes, g.sum_bytes, g.const_bytes);
    s += b;
    return s;
}

} // namespace visp
