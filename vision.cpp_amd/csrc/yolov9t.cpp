// YOLOv9t: load + hand schedule + host post-processing (see yolov9t.h). Reference: src/visp/arch/yolov9t.cpp,
// src/cli/inference_yolov9t.cpp:300-405.
#include "yolov9t.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <chrono>
#include <numeric>
#include <string>

#include "packer.h"
#include "visp_util.h"

namespace visp {

int yolov9t_anchors(int S) { return (S / 8) * (S / 8) + (S / 16) * (S / 16) + (S / 32) * (S / 32); }

namespace {

// ---- loader ----------------------------------------------------------------------------------------------------------------

struct yolo_loader {
    model_file const& file;
    packer& pk;
    arena_builder& ab;
    yolov9t_model& m;

    // conv kernel "<name>" -> f32 [cout][k*k*cin] rows k = (ky, kx, c); OIHW when listed in conv2d_weights of a whcn file, else OHWI
    std::vector<float> kernel(std::string const& name, int cin, int cout, int k) {
        gguf_tensor const& t = pk.get(name);
        const bool oihw = pk.file_whcn && pk.listed(name);
        const int64_t want[4] = {oihw ? k : cin, k, oihw ? cin : k, cout};
        for (int i = 0; i < 4; ++i)
            if (t.ne[i] != want[i])
                throw except("yolov9t: %s has ne [%lld, %lld, %lld, %lld], expected a %dx%d conv %d -> %d", name.c_str(), (long long)t.ne[0], (long long)t.ne[1],
                             (long long)t.ne[2], (long long)t.ne[3], k, k, cin, cout);
        std::vector<float> w((size_t)cout * k * k * cin);
        for (int n = 0; n < cout; ++n)
            for (int ky = 0; ky < k; ++ky)
                for (int kx = 0; kx < k; ++kx)
                    for (int c = 0; c < cin; ++c) {
                        const size_t src = oihw ? (((size_t)n * cin + c) * k + ky) * k + kx : (((size_t)n * k + ky) * k + kx) * cin + c;
                        w[(((size_t)n * k + ky) * k + kx) * cin + c] = tensor_at(t, src);
                    }
        return w;
    }
    std::vector<float> bias(std::string const& name, int cout) {
        gguf_tensor const& t = pk.get(name);
        if (t.n_elements() != cout) throw except("yolov9t: %s has %lld elements, expected %d", name.c_str(), (long long)t.n_elements(), cout);
        std::vector<float> b((size_t)cout);
        for (int i = 0; i < cout; ++i) b[(size_t)i] = tensor_at(t, (size_t)i);
        return b;
    }
    // f32 kernel + bias -> the arena (input channels padded to cin_pad with zero weights)
    void pack(std::string const& key, std::vector<float> const& w, std::vector<float> const& b, int cin, int cin_pad, int cout, int k) {
        yolo_conv c;
        c.k = k; c.cin = cin_pad; c.cin_real = cin; c.cout = cout;
        auto at = [&](int n, int kk) -> float {
            const int tap = kk / cin_pad, ch = kk % cin_pad;
            return ch < cin ? w[((size_t)n * k * k + tap) * cin + ch] : 0.0f;
        };
        c.g = pk.matrix(cout, k * k * cin_pad, at, nullptr);
        c.g.b = ab.alloc((size_t)c.g.N * 4);
        memcpy(ab.data.data() + c.g.b, b.data(), b.size() * 4);
        m.convs[key] = c;
    }
    // Conv (yolov9t.cpp:78-120): "<key>.conv.{weight,bias}", BatchNorm already folded
    void conv(std::string const& key, int cin, int cout, int k, int cin_pad = 0) {
        pack(key, kernel(key + ".conv.weight", cin, cout, k), bias(key + ".conv.bias", cout), cin, cin_pad ? cin_pad : cin, cout, k);
    }
    // the detect head's plain 1x1 conv_2d "<key>.{weight,bias}" (yolov9t.cpp:783-795)
    void plain(std::string const& key, int cin, int cout) { pack(key, kernel(key + ".weight", cin, cout, 1), bias(key + ".bias", cout), cin, cin, cout, 1); }
    // RepConv (yolov9t.cpp:256-302): conv1 3x3 + conv2 1x1, added, then SiLU. The 1x1 kernel and its bias are folded into the centre
    // tap of the 3x3 in f32 and rounded to f16 once (the reference evaluates two convs and adds them)
    void repconv(std::string const& key, int c) {
        std::vector<float> w3 = kernel(key + ".conv1.conv.weight", c, c, 3), b3 = bias(key + ".conv1.conv.bias", c);
        std::vector<float> w1 = kernel(key + ".conv2.conv.weight", c, c, 1), b1 = bias(key + ".conv2.conv.bias", c);
        for (int n = 0; n < c; ++n) {
            for (int ch = 0; ch < c; ++ch) w3[((size_t)n * 9 + 4) * c + ch] += w1[(size_t)n * c + ch];
            b3[(size_t)n] += b1[(size_t)n];
        }
        pack(key, w3, b3, c, c, c, 3);
    }
    void elan1(std::string const& p, int c1, int c2, int c3, int c4) { // yolov9t.cpp:187-240
        conv(p + ".cv1", c1, c3, 1);
        conv(p + ".cv2", c3 / 2, c4, 3);
        conv(p + ".cv3", c4, c4, 3);
        conv(p + ".cv4", c3 + 2 * c4, c2, 1);
    }
    void repcsp(std::string const& p, int c1, int c2, int n) { // yolov9t.cpp:370-404, RepBottleneck :304-330
        const int c_ = c2 / 2;
        conv(p + ".cv1", c1, c_, 1);
        conv(p + ".cv2", c1, c_, 1);
        for (int j = 0; j < n; ++j) {
            const std::string q = p + ".m." + std::to_string(j);
            repconv(q + ".cv1", c_);
            conv(q + ".cv2", c_, c_, 3);
        }
        conv(p + ".cv3", 2 * c_, c2, 1);
    }
    void repncspelan4(std::string const& p, int c1, int c2, int c3, int c4, int n) { // yolov9t.cpp:406-447
        conv(p + ".cv1", c1, c3, 1);
        repcsp(p + ".cv2.0", c3 / 2, c4, n);
        conv(p + ".cv2.1", c4, c4, 3);
        repcsp(p + ".cv3.0", c4, c4, n);
        conv(p + ".cv3.1", c4, c4, 3);
        conv(p + ".cv4", c3 + 2 * c4, c2, 1);
    }
};

constexpr int kRepN = 3;                       // RepCSP depth of every RepNCSPELAN4 (the yolov9t_backbone table, yolov9t.cpp:507-630)
constexpr int kHeadCh[3] = {64, 96, 128};      // detect inputs: model.15, model.18, model.21

int cout_of(model_file const& f, std::string const& name) { return (int)f.tensor(name).ne[3]; } // conv kernels: ne[3] = Cout in both layouts

} // namespace

yolov9t_model* yolov9t_load_model(char const* filepath, backend_device const& dev) {
    model_file file = model_load(filepath, /*header_only=*/false);
    std::string_view arch = file.arch();
    if (arch != "yolov9t")
        throw except("Architecture expected to be 'yolov9t', but was '%.*s' (%s)", (int)arch.size(), arch.data(), file.path.c_str());
    auto model = std::make_unique<yolov9t_model>();
    model->backend = &dev;
    arena_builder ab;
    packer pk{file, ab, true, file.tensor_layout() != layout_cwhn, file.conv2d_weights()};
    yolo_loader ld{file, pk, ab, *model};

    const int box_ch = cout_of(file, "detect.cv2.0.2.weight");
    if (box_ch % 4 != 0 || box_ch / 4 != 16) throw except("yolov9t: reg_max %d is not supported (the DFL decode is built for reg_max 16)", box_ch / 4);
    model->reg_max = 16;
    const int nc = cout_of(file, "detect.cv3.0.2.weight");
    if (nc <= 0 || nc % 8 != 0 || nc > 1024) throw except("yolov9t: %d classes (a multiple of 8 up to 1024 is built)", nc);
    model->num_classes = nc;
    model->head_c3 = std::max(kHeadCh[0], std::min(nc, 100)); // detect_forward (yolov9t.cpp:770-776)
    if (model->head_c3 % 8 != 0)
        throw except("yolov9t: %d classes give a class branch of %d channels, which is not a multiple of 8 (the conv loader needs that); "
                     "up to 96 classes are built", nc, model->head_c3);

    ld.conv("model.0", 3, 16, 3, /*cin_pad=*/8); // the preprocess writes 8 channels per pixel (rgb + 5 zeros)
    ld.conv("model.1", 16, 32, 3);
    ld.elan1("model.2", 32, 32, 32, 16);
    ld.conv("model.3.cv1", 32, 64, 3);
    ld.repncspelan4("model.4", 64, 64, 64, 32, kRepN);
    ld.conv("model.5.cv1", 64, 96, 3);
    ld.repncspelan4("model.6", 96, 96, 96, 48, kRepN);
    ld.conv("model.7.cv1", 96, 128, 3);
    ld.repncspelan4("model.8", 128, 128, 128, 64, kRepN);
    ld.conv("model.9.cv1", 128, 64, 1);
    ld.conv("model.9.cv5", 256, 128, 1);
    ld.repncspelan4("model.12", 224, 96, 96, 48, kRepN);
    ld.repncspelan4("model.15", 160, 64, 64, 32, kRepN);
    ld.conv("model.16.cv1", 64, 48, 3);
    ld.repncspelan4("model.18", 144, 96, 96, 48, kRepN);
    ld.conv("model.19.cv1", 96, 64, 3);
    ld.repncspelan4("model.21", 192, 128, 128, 64, kRepN);
    for (int l = 0; l < 3; ++l) {
        const std::string r = "detect.cv2." + std::to_string(l), c = "detect.cv3." + std::to_string(l);
        ld.conv(r + ".0", kHeadCh[l], 64, 3);
        ld.conv(r + ".1", 64, 64, 3);
        ld.plain(r + ".2", 64, 64);
        ld.conv(c + ".0", kHeadCh[l], model->head_c3, 3);
        ld.conv(c + ".1", model->head_c3, model->head_c3, 3);
        ld.plain(c + ".2", model->head_c3, nc);
    }

    device_turn turn(dev);
    model->weight_arena = upload_arena(ab.data, dev.stream);
    return model.release();
}

namespace {

// ---- schedule --------------------------------------------------------------------------------------------------------------

struct fmap { // an NHWC f16 map, possibly a channel slice of a wider buffer
    uint8_t* p = nullptr; // first channel of pixel 0
    int64_t pix = 0;      // elements between pixels
    int H = 0, W = 0, C = 0;
    fmap slice(int c0, int c) const { return fmap{p + (size_t)c0 * 2, pix, H, W, c}; }
};

// One pass over the launch list for a (batch, S). The same code lays out the workspace (dry: bump offsets only, nothing launched)
// and enqueues the launches, so the layout cannot drift from the schedule.
struct yolo_exec : model_pass<yolov9t_model> {
    uint8_t* ws;
    int B, S, A, nc;
    workspace_layout layout;
    // fixed buffers (laid out first, in this order)
    uint8_t *in_u8 = nullptr, *in_f32 = nullptr, *boxes = nullptr, *scores = nullptr, *cand_count = nullptr, *cand_idx = nullptr, *cand_score = nullptr,
            *cap_tmp = nullptr;
    fmap in8, raw[3];

    yolo_exec(yolov9t_model& mm, void* s, int b, int size, bool d)
        : model_pass(mm, s, mm.weight_arena.ptr, d), ws(static_cast<uint8_t*>(mm.ws.ptr)), B(b), S(size), A(yolov9t_anchors(size)), nc(mm.num_classes) {
        in_u8 = alloc((size_t)B * S * S * 4);
        in_f32 = alloc((size_t)B * S * S * 12);
        boxes = alloc((size_t)B * A * 16);
        scores = alloc((size_t)B * A * nc * 4);
        cand_count = alloc((size_t)B * 4);
        cand_idx = alloc((size_t)B * A * nc * 4);
        cand_score = alloc((size_t)B * A * nc * 4);
        cap_tmp = alloc((size_t)B * (S / 8) * (S / 8) * 128 * 2); // the largest slice that is captured (model.13: S/8, 96 channels)
        in8 = map(S, S, 8);
    }

    uint8_t* alloc(size_t bytes) { return reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(ws) + layout.take(bytes)); }
    fmap map(int H, int W, int C) { return fmap{alloc((size_t)B * H * W * C * 2), C, H, W, C}; }

    void capture(std::string const& name, fmap const& v) {
        if (dry || !m.captures) return;
        const void* src = v.p;
        if (v.pix != v.C) { // a slice: gather it into a contiguous map first
            const int64_t ne[4] = {v.C, (int64_t)v.H * v.W, B, 1};
            const int64_t ss[4] = {1, v.pix, (int64_t)v.H * v.W * v.pix, 0}, ds[4] = {1, v.C, (int64_t)v.H * v.W * v.C, 0};
            VX(vx_copy_strided_f16(v.p, cap_tmp, ne, ss, ds, 1.0f, stream));
            src = cap_tmp;
        }
        keep(name, src, {B, v.H, v.W, v.C});
    }
    void capture_f32(std::string const& name, const void* src, int64_t d1, int64_t d2) { keep(name, src, {B, d1, d2, 1}, false); }

    // one conv on the GEMM family: out = act(conv(in) + bias) [+ res]; act = SiLU (Conv) or none (the head's plain 1x1)
    void conv(std::string const& key, fmap const& in, fmap const& out, int stride, const fmap* res, bool act, const char* group) {
        auto it = m.convs.find(key);
        if (it == m.convs.end()) throw except("yolov9t: no conv '%s' in the loaded model", key.c_str());
        yolo_conv const& c = it->second;
        const int pad = c.k / 2, OH = (in.H + 2 * pad - c.k) / stride + 1, OW = (in.W + 2 * pad - c.k) / stride + 1;
        if (in.C != c.cin || out.C != c.cout || out.H != OH || out.W != OW)
            throw except("yolov9t: %s: %dx%dx%d -> %dx%dx%d does not fit the conv (%d -> %d, k %d, s %d)", key.c_str(), in.H, in.W, in.C, out.H, out.W, out.C, c.cin,
                         c.cout, c.k, stride);
        const double M = (double)B * OH * OW;
        mark(group, 2.0 * M * c.cout * c.k * c.k * c.cin_real,
             ((double)B * in.H * in.W * c.cin + M * c.cout * (res ? 2 : 1)) * 2 + (double)c.cout * c.k * c.k * c.cin * 2);
        if (dry) return;
        vx_gemm_args a = gemm_args(c.g, wa);
        a.A = in.p;
        a.conv_kh = a.conv_kw = c.k;
        a.conv_stride = stride;
        a.conv_pad = pad;
        a.conv_H = in.H; a.conv_W = in.W; a.conv_Cin = c.cin; a.conv_OH = OH; a.conv_OW = OW;
        a.conv_pix = in.pix;
        a.M = (int)M;
        a.epi = act ? VX_EPI_SILU : VX_EPI_F16;
        a.out = out.p; a.ldo = out.pix;
        if (res) { a.res1 = res->p; a.ld_res1 = res->pix; }
        VX(vx_gemm_f16(&a, stream));
    }
    const char* group(std::string const& key) const { return m.convs.at(key).k == 3 ? "conv3x3" : "conv1x1"; }
    void C(std::string const& key, fmap const& in, fmap const& out, const fmap* res = nullptr) { conv(key, in, out, 1, res, true, group(key)); }

    // ---- blocks (yolov9t.cpp:165-484); every concat is a buffer its producers write into
    void aconv(std::string const& p, fmap const& in, fmap const& out) {
        fmap pooled = map(in.H - 1, in.W - 1, in.C);
        mark("aconv", (double)B * pooled.H * pooled.W * in.C * 4, (double)B * (in.H * in.W + pooled.H * pooled.W) * in.C * 2);
        if (!dry) VX(vx_yolo_avgpool2_f16(in.p, in.pix, pooled.p, B, in.H, in.W, in.C, stream));
        conv(p + ".cv1", pooled, out, 2, nullptr, true, "aconv");
    }
    void elan1(std::string const& p, fmap const& in, fmap const& out) {
        const int c3 = m.convs.at(p + ".cv1").cout, c4 = m.convs.at(p + ".cv2").cout;
        fmap cat = map(in.H, in.W, c3 + 2 * c4);
        C(p + ".cv1", in, cat.slice(0, c3));
        C(p + ".cv2", cat.slice(c3 / 2, c3 / 2), cat.slice(c3, c4));
        C(p + ".cv3", cat.slice(c3, c4), cat.slice(c3 + c4, c4));
        C(p + ".cv4", cat, out);
    }
    void repcsp(std::string const& p, fmap const& in, fmap const& out) {
        const int c_ = m.convs.at(p + ".cv1").cout;
        fmap cat = map(in.H, in.W, 2 * c_), t[2] = {map(in.H, in.W, c_), map(in.H, in.W, c_)}, y = map(in.H, in.W, c_);
        C(p + ".cv1", in, t[0]);
        C(p + ".cv2", in, cat.slice(c_, c_));
        for (int j = 0; j < kRepN; ++j) { // RepBottleneck: x + Conv(RepConv(x))
            const std::string q = p + ".m." + std::to_string(j);
            const fmap& x = t[j & 1];
            C(q + ".cv1", x, y);
            C(q + ".cv2", y, j + 1 == kRepN ? cat.slice(0, c_) : t[(j + 1) & 1], &x);
        }
        C(p + ".cv3", cat, out);
    }
    void repncspelan4(std::string const& p, fmap const& in, fmap const& out) {
        const int c3 = m.convs.at(p + ".cv1").cout, c4 = m.convs.at(p + ".cv2.1").cout;
        fmap cat = map(in.H, in.W, c3 + 2 * c4), t2 = map(in.H, in.W, c4), t3 = map(in.H, in.W, c4);
        C(p + ".cv1", in, cat.slice(0, c3));
        repcsp(p + ".cv2.0", cat.slice(c3 / 2, c3 / 2), t2);
        C(p + ".cv2.1", t2, cat.slice(c3, c4));
        repcsp(p + ".cv3.0", cat.slice(c3, c4), t3);
        C(p + ".cv3.1", t3, cat.slice(c3 + c4, c4));
        C(p + ".cv4", cat, out);
    }
    void sppelan(std::string const& p, fmap const& in, fmap const& out) {
        const int c3 = m.convs.at(p + ".cv1").cout;
        fmap cat = map(in.H, in.W, 4 * c3);
        C(p + ".cv1", in, cat.slice(0, c3));
        mark("spp", (double)B * in.H * in.W * c3 * 169, (double)B * in.H * in.W * c3 * 2 * 4);
        if (!dry) VX(vx_yolo_spp_f16(cat.p, cat.pix, B, in.H, in.W, c3, stream));
        C(p + ".cv5", cat, out);
    }
    void upsample(fmap const& in, fmap const& out) {
        mark("upsample", 0, (double)B * in.H * in.W * in.C * 2 * 5);
        if (!dry) VX(vx_yolo_upsample2_f16(in.p, in.pix, out.p, out.pix, B, in.H, in.W, in.C, stream));
    }

    // yolov9t_backbone (yolov9t.cpp:507-630) + detect_forward's convs (:770-800) from in8; raw[l] = the level's 64 + nc head outputs
    void network() {
        const int s2 = S / 2, s4 = S / 4, s8 = S / 8, s16 = S / 16, s32 = S / 32;
        fmap x0 = map(s2, s2, 16), x1 = map(s4, s4, 32), x2 = map(s4, s4, 32), x3 = map(s8, s8, 64);
        fmap x14 = map(s8, s8, 160), x5 = map(s16, s16, 96), x11 = map(s16, s16, 224), x7 = map(s32, s32, 128), x8 = map(s32, s32, 128);
        fmap x20 = map(s32, s32, 192), x17 = map(s16, s16, 144), x15 = map(s8, s8, 64), x18 = map(s16, s16, 96), x21 = map(s32, s32, 128);
        fmap x4 = x14.slice(96, 64), x6 = x11.slice(128, 96), x9 = x20.slice(64, 128), x10 = x11.slice(0, 128), x12 = x17.slice(48, 96);
        fmap x13 = x14.slice(0, 96), x16 = x17.slice(0, 48), x19 = x20.slice(0, 64);
        conv("model.0", in8, x0, 2, nullptr, true, "conv3x3");
        capture("model.0", x0);
        conv("model.1", x0, x1, 2, nullptr, true, "conv3x3");
        capture("model.1", x1);
        elan1("model.2", x1, x2);
        capture("model.2", x2);
        aconv("model.3", x2, x3);
        capture("model.3", x3);
        repncspelan4("model.4", x3, x4);
        capture("model.4", x4);
        aconv("model.5", x4, x5);
        capture("model.5", x5);
        repncspelan4("model.6", x5, x6);
        capture("model.6", x6);
        aconv("model.7", x6, x7);
        capture("model.7", x7);
        repncspelan4("model.8", x7, x8);
        capture("model.8", x8);
        sppelan("model.9", x8, x9);
        capture("model.9", x9);
        upsample(x9, x10);
        capture("model.10", x10);
        capture("model.11", x11);
        repncspelan4("model.12", x11, x12);
        capture("model.12", x12);
        upsample(x12, x13);
        capture("model.13", x13);
        capture("model.14", x14);
        repncspelan4("model.15", x14, x15);
        capture("model.15", x15);
        aconv("model.16", x15, x16);
        capture("model.16", x16);
        capture("model.17", x17);
        repncspelan4("model.18", x17, x18);
        capture("model.18", x18);
        aconv("model.19", x18, x19);
        capture("model.19", x19);
        capture("model.20", x20);
        repncspelan4("model.21", x20, x21);
        capture("model.21", x21);
        const fmap feats[3] = {x15, x18, x21};
        for (int l = 0; l < 3; ++l) {
            const fmap& f = feats[l];
            const std::string r = "detect.cv2." + std::to_string(l), c = "detect.cv3." + std::to_string(l);
            const int c3 = m.head_c3;
            raw[l] = map(f.H, f.W, 64 + nc);
            fmap r0 = map(f.H, f.W, 64), r1 = map(f.H, f.W, 64), k0 = map(f.H, f.W, c3), k1 = map(f.H, f.W, c3);
            conv(r + ".0", f, r0, 1, nullptr, true, "head");
            conv(r + ".1", r0, r1, 1, nullptr, true, "head");
            conv(r + ".2", r1, raw[l].slice(0, 64), 1, nullptr, false, "head");
            conv(c + ".0", f, k0, 1, nullptr, true, "head");
            conv(c + ".1", k0, k1, 1, nullptr, true, "head");
            conv(c + ".2", k1, raw[l].slice(64, nc), 1, nullptr, false, "head");
            capture("detect.raw" + std::to_string(l), raw[l]);
        }
    }
    // inference (yolov9t.cpp:693-768); candidates: also the per-image list of (anchor, class) with score >= conf
    void decode(float conf, bool candidates) {
        mark("decode", (double)B * A * (16 * 6 + nc * 4), (double)B * A * ((64 + nc) * 2 + 16 + nc * 4));
        if (dry) return;
        if (candidates) VX(vx_memset(cand_count, 0, (size_t)B * 4, stream));
        VX(vx_yolo_decode(raw[0].p, raw[1].p, raw[2].p, B, S, nc, reinterpret_cast<float*>(boxes), reinterpret_cast<float*>(scores), conf,
                          candidates ? reinterpret_cast<int*>(cand_count) : nullptr, candidates ? reinterpret_cast<int*>(cand_idx) : nullptr,
                          candidates ? reinterpret_cast<float*>(cand_score) : nullptr, stream));
        capture_f32("boxes", boxes, A, 4);
        capture_f32("scores", scores, A, nc);
    }
    // the u8 launch list on the workspace's own input buffer
    void run_u8(int channels, float conf) {
        mark("preprocess", (double)B * S * S * 3, (double)B * S * S * (channels + 16));
        if (!dry) VX(vx_yolo_preprocess(in_u8, channels, nullptr, in8.p, (int64_t)B * S * S, stream));
        network();
        decode(conf, true);
    }
};

void check_extent(int B, int S) {
    if (B < 1) throw except("yolov9t: empty batch");
    if (S < 64 || S % 32 != 0 || S > 4096) throw except("yolov9t: input size %d is not a multiple of 32 in [64, 4096]", S);
}

// a workspace that holds the layout of (B, S); graphs of other extents stay valid unless the buffer moves
yolo_exec make_exec(yolov9t_model& m, int B, int S, void* stream) {
    check_extent(B, S);
    size_t total;
    {
        yolo_exec dry(m, stream, B, S, true);
        dry.run_u8(3, 0.0f);
        total = dry.layout.top;
    }
    if (grow(m.ws, total, {m.backend->stream, stream})) m.graphs.clear();
    return yolo_exec(m, stream, B, S, false);
}

void check_params(yolo_nms_params const& p) {
    if (!(0.0f <= p.conf && p.conf <= 1.0f)) throw except("Invalid Confidence threshold");
    if (!(0.0f <= p.iou && p.iou <= 1.0f)) throw except("Invalid IoU threshold");
    if (p.max_det < 1 || p.max_nms < 1) throw except("yolov9t: max_det (%d) and max_nms (%d) must be positive", p.max_det, p.max_nms);
}

struct cand {
    int idx; // anchor * nc + class
    float score;
};

// non_max_suppression (yolov9t.cpp:1145-1253) + nms (:1117-1143) on the candidates with score >= conf, in any order. Ties of the score
// are ordered by (anchor, class), where the reference's std::sort leaves the order unspecified.
std::vector<yolo_detection> nms_candidates(std::vector<cand>& c, float const* boxes, int nc, yolo_nms_params const& p) {
    std::sort(c.begin(), c.end(), [](cand const& a, cand const& b) { return a.score > b.score || (a.score == b.score && a.idx < b.idx); });
    if ((int)c.size() > p.max_nms) c.resize((size_t)p.max_nms);
    const size_t n = c.size();
    std::vector<char> removed(n, 0);
    std::vector<yolo_detection> out;
    // intersection over union of two xyxy boxes; 0 when the union is not positive. For bit parity with the reference the float
    // operations keep its order: overlap width times height, then (area of a + area of b) - overlap
    auto overlap_ratio = [](const float* a, const float* b) {
        const float ow = std::max(0.0f, std::min(a[2], b[2]) - std::max(a[0], b[0]));
        const float oh = std::max(0.0f, std::min(a[3], b[3]) - std::max(a[1], b[1]));
        const float common = ow * oh;
        const float both = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - common;
        if (!(both > 0.0f)) return 0.0f;
        return common / both;
    };
    for (size_t i = 0; i < n && (int)out.size() < p.max_det; ++i) { // the greedy pass stops once max_det boxes are kept: same first max_det
        if (removed[i]) continue;
        const int ai = c[i].idx / nc, ci = c[i].idx % nc;
        const float* bi = boxes + (size_t)ai * 4;
        const int oi = ci * p.max_wh; // the class offset moves x only, as the reference's nms does
        const float b1[4] = {bi[0] + oi, bi[1], bi[2] + oi, bi[3]};
        out.push_back(yolo_detection{bi[0], bi[1], bi[2], bi[3], c[i].score, ci, c[i].score});
        for (size_t j = i + 1; j < n; ++j) {
            if (removed[j]) continue;
            const int aj = c[j].idx / nc, oj = (c[j].idx % nc) * p.max_wh;
            const float* bj = boxes + (size_t)aj * 4;
            const float b2[4] = {bj[0] + oj, bj[1], bj[2] + oj, bj[3]};
            if (overlap_ratio(b1, b2) > p.iou) removed[j] = 1;
        }
    }
    return out;
}

} // namespace

yolov9t_model::~yolov9t_model() {
    for (void* e : events) vx_event_destroy(e);
}

std::vector<yolo_detection> yolov9t_nms(float const* boxes, float const* scores, int A, int nc, yolo_nms_params const& p) {
    if (!boxes || !scores) throw except("yolov9t: null boxes / scores");
    if (A < 1 || nc < 1) throw except("yolov9t: %d anchors x %d classes", A, nc);
    check_params(p);
    std::vector<cand> c;
    for (int a = 0; a < A; ++a)
        for (int k = 0; k < nc; ++k) {
            const float s = scores[(size_t)a * nc + k];
            if (s >= p.conf) c.push_back(cand{a * nc + k, s});
        }
    return nms_candidates(c, boxes, nc, p);
}

void yolov9t_scale_boxes(std::vector<yolo_detection>& d, i32x2 extent, float gain, float pad_w, float pad_h) {
    const float w = (float)extent[0], h = (float)extent[1];
    for (yolo_detection& o : d) {
        o.x1 = std::clamp((o.x1 - pad_w) / gain, 0.0f, w);
        o.x2 = std::clamp((o.x2 - pad_w) / gain, 0.0f, w);
        o.y1 = std::clamp((o.y1 - pad_h) / gain, 0.0f, h);
        o.y2 = std::clamp((o.y2 - pad_h) / gain, 0.0f, h);
    }
}

yolo_letterbox yolov9t_letterbox(image_view const& image, int S) {
    if (!image.data) throw except("yolov9t: null image");
    if (image.format != image_format::rgb_u8 && image.format != image_format::rgba_u8)
        throw except("yolov9t: image must be rgb_u8 or rgba_u8 (format %d)", (int)image.format);
    if (image.extent[0] < 1 || image.extent[1] < 1) throw except("yolov9t: empty image");
    if (S < 32 || S > 4096) throw except("yolov9t: letterbox size %d", S);
    const int w = image.extent[0], h = image.extent[1];
    const float r = std::min((float)S / (float)h, (float)S / (float)w);
    const int nw = (int)std::round(w * r), nh = (int)std::round(h * r);
    const float dw = (float)(S - nw) / 2.0f, dh = (float)(S - nh) / 2.0f;
    image_data rgb = image_to_rgb_u8(image); // alpha is ignored (the reference's border code handles 3 channels only)
    image_data scaled = image_scale(view_of(rgb), i32x2{{nw, nh}});
    const int left = (int)std::round(dw - 0.1f), top = (int)std::round(dh - 0.1f);
    yolo_letterbox out;
    out.img = image_alloc(i32x2{{S, S}}, image_format::rgb_u8);
    memset(out.img.data.get(), 114, (size_t)S * S * 3);
    for (int y = 0; y < nh; ++y) memcpy(out.img.data.get() + ((size_t)(y + top) * S + left) * 3, scaled.data.get() + (size_t)y * nw * 3, (size_t)nw * 3);
    out.gain = r;
    out.pad_w = dw;
    out.pad_h = dh;
    return out;
}

namespace {

using clock_type = std::chrono::steady_clock;
float ms_since(clock_type::time_point t0) { return std::chrono::duration<float, std::milli>(clock_type::now() - t0).count(); }

// the batch entry once the images are in the workspace's in_u8: the launch list (hipGraph replay after the first call of a key), then the
// candidate lists back to the host and NMS per image; m.last_split_ms = {launch list on the device, readback, host NMS}
std::vector<std::vector<yolo_detection>> run_batch(yolov9t_model& m, yolo_exec& ex, int channels, yolo_nms_params const& p) {
    void* s = ex.stream;
    const int batch = ex.B, S = ex.S;
    for (void*& e : m.events)
        if (!e) VX(vx_event_create(&e));
    VX(vx_event_record(m.events[0], s));
    uint32_t conf_bits;
    memcpy(&conf_bits, &p.conf, 4);
    const auto gkey = std::make_tuple(batch * 8 + channels, S, (int)conf_bits); // the decode's threshold is part of the launch list
    replay_or_run(m, m.graphs, gkey, s, [&] {
        yolo_exec pass(m, s, batch, S, false); // a fresh pass: the same workspace offsets as ex
        pass.run_u8(channels, p.conf);
        pass.finish_timing();
    });
    VX(vx_event_record(m.events[1], s));
    VX(vx_event_elapsed_ms(m.events[0], m.events[1], &m.last_split_ms[0])); // waits for the launch list
    const clock_type::time_point t_read = clock_type::now();
    const int A = ex.A, nc = ex.nc;
    std::vector<int> counts((size_t)batch);
    std::vector<float> boxes((size_t)batch * A * 4);
    VX(vx_memcpy_d2h(counts.data(), ex.cand_count, counts.size() * 4, s));
    VX(vx_memcpy_d2h(boxes.data(), ex.boxes, boxes.size() * 4, s));
    VX(vx_stream_sync(s));
    std::vector<std::vector<int>> idx((size_t)batch);
    std::vector<std::vector<float>> sc((size_t)batch);
    for (int b = 0; b < batch; ++b) { // every list is enqueued before the one synchronisation
        const int n = counts[(size_t)b];
        if (n < 0 || n > A * nc) throw except("yolov9t: candidate count %d out of range", n);
        idx[(size_t)b].resize((size_t)n);
        sc[(size_t)b].resize((size_t)n);
        const size_t base = (size_t)b * A * nc;
        if (n > 0) {
            VX(vx_memcpy_d2h(idx[(size_t)b].data(), ex.cand_idx + base * 4, (size_t)n * 4, s));
            VX(vx_memcpy_d2h(sc[(size_t)b].data(), ex.cand_score + base * 4, (size_t)n * 4, s));
        }
    }
    VX(vx_stream_sync(s));
    m.last_split_ms[1] = ms_since(t_read);
    const clock_type::time_point t_nms = clock_type::now();
    std::vector<std::vector<yolo_detection>> out((size_t)batch);
    for (int b = 0; b < batch; ++b) {
        const size_t n = idx[(size_t)b].size();
        std::vector<cand> c(n);
        for (size_t i = 0; i < n; ++i) c[i] = cand{idx[(size_t)b][i], sc[(size_t)b][i]};
        out[(size_t)b] = nms_candidates(c, boxes.data() + (size_t)b * A * 4, nc, p);
    }
    m.last_split_ms[2] = ms_since(t_nms);
    return out;
}

void check_batch_args(void const* img, int channels, yolo_nms_params const& p) {
    if (!img) throw except("yolov9t: null input pointer");
    if (channels != 3 && channels != 4) throw except("yolov9t: image must have 3 or 4 channels, got %d", channels);
    check_params(p);
}

} // namespace

std::vector<std::vector<yolo_detection>> yolov9t_detect_batch_device(yolov9t_model& m, void const* img_dev, int channels, int batch, int S,
                                                                     yolo_nms_params const& p, void* stream) {
    check_batch_args(img_dev, channels, p);
    device_turn turn(*m.backend);
    void* s = stream ? stream : m.backend->stream;
    yolo_exec ex = make_exec(m, batch, S, s);
    VX(vx_memcpy_d2d(ex.in_u8, img_dev, (size_t)batch * S * S * channels, s));
    return run_batch(m, ex, channels, p);
}

std::vector<std::vector<yolo_detection>> yolov9t_detect_batch_host(yolov9t_model& m, uint8_t const* img, int channels, int batch, int S,
                                                                   yolo_nms_params const& p) {
    check_batch_args(img, channels, p);
    device_turn turn(*m.backend);
    void* s = m.backend->stream;
    yolo_exec ex = make_exec(m, batch, S, s);
    VX(vx_memcpy_h2d(ex.in_u8, img, (size_t)batch * S * S * channels, s)); // straight into the workspace's input
    return run_batch(m, ex, channels, p);
}

void yolov9t_forward_host(yolov9t_model& m, float const* rgb, int n, int S, float* boxes, float* scores) {
    if (!rgb || !boxes || !scores) throw except("yolov9t: null input/output pointer");
    device_turn turn(*m.backend);
    void* s = m.backend->stream;
    yolo_exec ex = make_exec(m, n, S, s);
    const size_t px = (size_t)n * S * S;
    VX(vx_memcpy_h2d(ex.in_f32, rgb, px * 12, s));
    ex.mark("preprocess", (double)px * 3, (double)px * 28);
    VX(vx_yolo_preprocess(nullptr, 3, reinterpret_cast<const float*>(ex.in_f32), ex.in8.p, (int64_t)px, s));
    ex.network();
    ex.decode(0.0f, false);
    ex.finish_timing();
    VX(vx_memcpy_d2h(boxes, ex.boxes, (size_t)n * ex.A * 16, s));
    VX(vx_memcpy_d2h(scores, ex.scores, (size_t)n * ex.A * ex.nc * 4, s));
    VX(vx_stream_sync(s));
}

std::vector<yolo_detection> yolov9t_detect(yolov9t_model& m, image_view const& image, yolo_nms_params const& p) {
    check_params(p);
    yolo_letterbox lb = yolov9t_letterbox(image, m.input_size);
    std::vector<yolo_detection> d = yolov9t_detect_batch_host(m, lb.img.data.get(), 3, 1, m.input_size, p)[0];
    yolov9t_scale_boxes(d, image.extent, lb.gain, lb.pad_w, lb.pad_h);
    return d;
}

} // namespace visp
