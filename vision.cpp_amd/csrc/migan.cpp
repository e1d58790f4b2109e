// MI-GAN inpainting: load + hand schedule (see migan.h). Reference: src/visp/arch/migan.cpp, src/visp/vision.cpp:172-203.
#include "migan.h"

#include <cmath>
#include <cstring>
#include <string>

#include "packer.h"
#include "visp_util.h"

namespace visp {

migan_params migan_detect_params(model_file const& f) {
    std::string_view arch = f.arch();
    if (arch != "migan")
        throw except("Architecture expected to be 'migan', but was '%.*s' (%s)", (int)arch.size(), arch.data(), f.path.c_str());
    migan_params p;
    p.resolution = f.get_int("migan.image_size");
    return p;
}

namespace {

struct migan_loader {
    model_file const& file;
    packer& pk;
    arena_builder& ab;

    // the depthwise / FIR kernels of one conv: OIHW-listed ne = [k, k, 1, C] (index c*k*k + tap), otherwise [C, 1, k, k] (tap*C + c)
    size_t fir(std::string const& name, int C) {
        gguf_tensor const& t = pk.get(name);
        const bool oihw = pk.file_whcn && pk.listed(name);
        const int64_t want[4] = {oihw ? 4 : C, oihw ? 4 : 1, oihw ? 1 : 4, oihw ? C : 4};
        for (int i = 0; i < 4; ++i)
            if (t.ne[i] != want[i]) throw except("migan: %s is not a 4x4 depthwise filter over %d channels", name.c_str(), C);
        const size_t off = ab.alloc((size_t)16 * C * 4);
        float* d = reinterpret_cast<float*>(ab.data.data() + off);
        for (int c = 0; c < C; ++c)
            for (int tap = 0; tap < 16; ++tap) d[(size_t)tap * C + c] = tensor_at(t, oihw ? (size_t)c * 16 + tap : (size_t)tap * C + c);
        return off;
    }
    // the upsample assumes nearest x2 times the [[1,0],[0,0]] tile (migan.cpp:34-51): refuse anything else
    void check_filter_const(std::string const& name, int res) {
        gguf_tensor const& t = pk.get(name);
        if (t.n_elements() != (int64_t)res * res) throw except("migan: %s has %lld elements, expected %d x %d", name.c_str(), (long long)t.n_elements(), res, res);
        for (int y = 0; y < res; ++y)
            for (int x = 0; x < res; ++x) {
                const float want = (y % 2 == 0 && x % 2 == 0) ? 1.0f : 0.0f;
                if (tensor_at(t, (size_t)y * res + x) != want)
                    throw except("migan: %s is not the zero-insertion tile [[1,0],[0,0]] (value %g at %d,%d)", name.c_str(), tensor_at(t, (size_t)y * res + x), y, x);
            }
    }
    size_t f32_copy(std::vector<float> const& v) {
        const size_t off = ab.alloc(v.size() * 4);
        memcpy(ab.data.data() + off, v.data(), v.size() * 4);
        return off;
    }
    // separable_conv_2d "<p>.conv1" (depthwise 3x3 + bias) / "<p>.conv2" (1x1, no bias) with optional down / up / noise
    migan_sep sep(std::string const& p, int res, int cin, int cout, bool down, bool up, bool noise) {
        migan_sep s;
        s.res = res; s.cin = cin; s.cout = cout;
        packed_dw d = pk.depthwise(p + ".conv1");
        if (d.C != cin) throw except("migan: %s.conv1 has %d channels, expected %d", p.c_str(), d.C, cin);
        s.dw_w = d.w; s.dw_b = d.b;
        int k = 0, ci = 0;
        packed_gemm g = pk.conv(p + ".conv2", &k, &ci);
        if (k != 1 || ci != cin || g.n_real != cout || g.K != cin || g.b != SIZE_MAX)
            throw except("migan: %s.conv2 is %dx%d %d -> %d%s, expected 1x1 %d -> %d without bias", p.c_str(), k, k, ci, g.n_real,
                         g.b != SIZE_MAX ? " with bias" : "", cin, cout);
        s.pw = g;
        if (down) s.down = fir(p + ".downsample.filter.weight", cin);
        const int ores = up ? 2 * res : (down ? res / 2 : res);
        if (up) {
            s.up = fir(p + ".upsample.filter.weight", cout);
            check_filter_const(p + ".upsample.filter_const", ores);
        }
        if (noise) {
            std::vector<float> nc = pk.host_vec(p + ".noise_const", (int64_t)ores * ores);
            std::vector<float> ns = pk.host_vec(p + ".noise_strength", 1);
            for (float& v : nc) v *= ns[0];
            s.noise = f32_copy(nc);
        }
        return s;
    }
};

int level_channels(model_file const& file, std::string const& name, bool oihw_listed) { // depthwise kernel of the level -> its width
    gguf_tensor const& t = file.tensor(name);
    return (int)(oihw_listed ? t.ne[3] : t.ne[0]);
}

} // namespace

migan_model* migan_load_model(char const* filepath, backend_device const& dev) {
    model_file file = model_load(filepath, /*header_only=*/false);
    auto model = std::make_unique<migan_model>();
    model->backend = &dev;
    model->params = migan_detect_params(file);
    const int R = model->params.resolution;
    if (R < 8 || R > 1024 || (R & (R - 1))) throw except("migan: image size %d is not a power of two in [8, 1024]", R);
    arena_builder ab;
    packer pk{file, ab, true, file.tensor_layout() != layout_cwhn, file.conv2d_weights()};
    migan_loader ld{file, pk, ab};

    for (int r = R; r >= 4; r >>= 1) {
        migan_level lv;
        lv.res = r;
        const std::string dwn = "encoder.b" + std::to_string(r) + ".conv1.conv1.weight";
        lv.ch = level_channels(file, dwn, pk.file_whcn && pk.listed(dwn));
        if (lv.ch <= 0 || lv.ch % 64 != 0 || lv.ch > 512) throw except("migan: level %d has %d channels (a multiple of 64 up to 512 is built)", r, lv.ch);
        model->levels.push_back(lv);
    }
    const int n = (int)model->levels.size();
    { // from_rgb (migan.cpp:84-89): 1x1, 4 -> ch(R), bias
        const std::string p = "encoder.b" + std::to_string(R) + ".fromrgb";
        int k = 0, ci = 0;
        packed_gemm g = pk.conv(p, &k, &ci);
        if (k != 1 || ci != 4 || g.n_real != model->levels[0].ch || g.b == SIZE_MAX)
            throw except("migan: %s is %dx%d %d -> %d, expected 1x1 4 -> %d with bias", p.c_str(), k, k, ci, g.n_real, model->levels[0].ch);
        std::vector<float> w((size_t)g.n_real * 4);
        const uint16_t* wp = reinterpret_cast<const uint16_t*>(ab.data.data() + g.w);
        for (int co = 0; co < g.n_real; ++co)
            for (int c = 0; c < 4; ++c) w[(size_t)co * 4 + c] = f16_to_f32(wp[(size_t)co * g.K + c]);
        std::vector<float> b = pk.host_vec(p + ".bias", g.n_real);
        model->fromrgb_w = ld.f32_copy(w);
        model->fromrgb_b = ld.f32_copy(b);
    }
    for (int i = 0; i < n; ++i) { // encoder blocks (migan.cpp:91-114)
        migan_level& lv = model->levels[(size_t)i];
        const std::string p = "encoder.b" + std::to_string(lv.res);
        const bool last = i == n - 1;
        lv.enc1 = ld.sep(p + ".conv1", lv.res, lv.ch, lv.ch, false, false, false);
        lv.enc2 = ld.sep(p + ".conv2", lv.res, lv.ch, last ? lv.ch : model->levels[(size_t)i + 1].ch, !last, false, false);
    }
    for (int i = n - 1; i >= 0; --i) { // synthesis blocks (migan.cpp:116-140)
        migan_level& lv = model->levels[(size_t)i];
        const std::string p = "synthesis.b" + std::to_string(lv.res);
        const bool first = i == n - 1;
        const int cin = first ? lv.ch : model->levels[(size_t)i + 1].ch;
        lv.syn1 = ld.sep(p + ".conv1", first ? lv.res : lv.res / 2, cin, lv.ch, false, !first, !first);
        lv.syn2 = ld.sep(p + ".conv2", lv.res, lv.ch, lv.ch, false, false, !first);
        int k = 0, ci = 0;
        packed_gemm g = pk.conv(p + ".torgb", &k, &ci);
        if (k != 1 || ci != lv.ch || g.n_real != 3 || g.b == SIZE_MAX)
            throw except("migan: %s.torgb is %dx%d %d -> %d, expected 1x1 %d -> 3 with bias", p.c_str(), k, k, ci, g.n_real, lv.ch);
        std::vector<float> w((size_t)3 * lv.ch);
        const uint16_t* wp = reinterpret_cast<const uint16_t*>(ab.data.data() + g.w);
        for (int co = 0; co < 3; ++co)
            for (int c = 0; c < lv.ch; ++c) w[(size_t)co * lv.ch + c] = f16_to_f32(wp[(size_t)co * g.K + c]);
        lv.torgb_w = ld.f32_copy(w);
        lv.torgb_b = ld.f32_copy(pk.host_vec(p + ".torgb.bias", 3));
        if (!first) {
            lv.img_up = ld.fir(p + ".upsample.filter.weight", 3);
            ld.check_filter_const(p + ".upsample.filter_const", lv.res);
        }
    }

    device_turn turn(dev);
    model->weight_arena = upload_arena(ab.data, dev.stream);
    return model.release();
}

namespace {

// workspace layout for a batch: the skip features of every level, three activation buffers of the largest map, two f32 image
// planes, the u8 inputs / output and the f32 input of the parity path
struct migan_layout {
    std::vector<size_t> feat;
    size_t act[3] = {0, 0, 0}, img[2] = {0, 0}, in_img = 0, in_mask = 0, out_rgba = 0, in4 = 0, total = 0;
};

migan_layout plan(migan_model const& m, int B) {
    migan_layout L;
    workspace_layout ws;
    size_t big = 0;
    for (migan_level const& lv : m.levels) {
        const size_t px = (size_t)B * lv.res * lv.res;
        L.feat.push_back(ws.take(px * lv.ch * 2));
        big = std::max(big, px * lv.ch * 2);
    }
    for (auto& a : L.act) a = ws.take(big);
    const size_t px = (size_t)B * m.params.resolution * m.params.resolution;
    for (auto& i : L.img) i = ws.take(px * 3 * 4);
    L.in_img = ws.take(px * 4);
    L.in_mask = ws.take(px);
    L.out_rgba = ws.take(px * 4);
    L.in4 = ws.take(px * 4 * 4);
    L.total = ws.top;
    return L;
}

struct migan_exec : model_pass<migan_model> {
    uint8_t* ws;
    migan_layout L;
    int B;

    template <typename T = float>
    const T* w(size_t off) const { return off == SIZE_MAX ? nullptr : reinterpret_cast<const T*>(wa + off); }
    void* at(size_t off) const { return ws + off; }

    void capture(std::string const& name, const void* src, int res, int C, bool f16) { keep(name, src, {B, res, res, C}, f16); }

    void dw(migan_sep const& s, const void* x, void* y) {
        const double px = (double)B * s.res * s.res;
        const bool down = s.down != SIZE_MAX;
        mark(down ? "dwconv_down" : "dwconv", px * s.cin * (18.0 + (down ? 8.0 : 0.0)), px * s.cin * 2 * (1.0 + (down ? 0.25 : 1.0)));
        VX(vx_migan_dwconv_f16(x, w<uint16_t>(s.dw_w), w(s.dw_b), w(s.down), y, B, s.res, s.res, s.cin, stream));
    }
    // 1x1 conv at extent res: out = act(x W^T (+ noise)) (+ res1); act = false: the raw product (before an upsample)
    void pw(migan_sep const& s, int res, const void* x, void* out, bool act, const void* res1) {
        vx_gemm_args a = gemm_args(s.pw, wa);
        const long M = (long)B * res * res;
        a.A = x; a.lda = s.cin;
        a.M = (int)M;
        a.epi = act ? VX_EPI_LRELU_AGC : VX_EPI_F16;
        a.out = out; a.ldo = s.cout;
        if (act && s.noise != SIZE_MAX) { a.noise = w(s.noise); a.noise_hw = res * res; }
        a.res1 = res1;
        mark("conv1x1", 2.0 * M * s.cin * s.cout, (double)M * (s.cin + s.cout + (res1 ? s.cout : 0)) * 2);
        VX(vx_gemm_f16(&a, stream));
    }

    // the generator from the fromrgb-activated map in act[0] to the rgb f32 image in img[final]; returns that image
    float* generate() {
        const int n = (int)m.levels.size();
        void* A = at(L.act[0]);
        void* Bf = at(L.act[1]);
        void* Cf = at(L.act[2]);
        for (int i = 0; i < n; ++i) { // encoder (migan.cpp:91-114): x in A
            migan_level const& lv = m.levels[(size_t)i];
            void* feat = at(L.feat[(size_t)i]);
            dw(lv.enc1, A, Bf);
            pw(lv.enc1, lv.res, Bf, feat, true, nullptr);
            capture("enc.feat" + std::to_string(lv.res), feat, lv.res, lv.ch, true);
            dw(lv.enc2, feat, Bf);
            pw(lv.enc2, lv.enc2.down != SIZE_MAX ? lv.res / 2 : lv.res, Bf, A, true, nullptr);
        }
        capture("enc.out", A, 4, m.levels.back().ch, true);
        float* img = nullptr;
        int cur = 0;
        for (int i = n - 1; i >= 0; --i) { // synthesis (migan.cpp:116-140): x in A
            migan_level const& lv = m.levels[(size_t)i];
            const void* feat = at(L.feat[(size_t)i]);
            if (i == n - 1) {
                dw(lv.syn1, A, Bf);
                pw(lv.syn1, lv.res, Bf, Cf, true, feat); // conv1, then + feat
                dw(lv.syn2, Cf, Bf);
                pw(lv.syn2, lv.res, Bf, A, true, nullptr);
            } else {
                const int h = lv.res / 2;
                dw(lv.syn1, A, Bf);
                pw(lv.syn1, h, Bf, Cf, false, nullptr);
                mark("upsample", (double)B * lv.res * lv.res * lv.ch * 12, (double)B * lv.res * lv.res * lv.ch * 2 * 2.25);
                VX(vx_migan_upsample_f16(Cf, w(lv.syn1.up), w(lv.syn1.noise), feat, Bf, B, h, h, lv.ch, stream));
                dw(lv.syn2, Bf, Cf);
                pw(lv.syn2, lv.res, Cf, A, true, nullptr);
            }
            float* next = static_cast<float*>(at(L.img[cur]));
            mark("torgb", (double)B * lv.res * lv.res * (6.0 * lv.ch + 24), (double)B * lv.res * lv.res * (2.0 * lv.ch + 12 + 3));
            VX(vx_migan_torgb(A, w(lv.torgb_w), w(lv.torgb_b), img, w(lv.img_up), next, B, lv.res, lv.res, lv.ch, stream));
            img = next;
            cur ^= 1;
            capture("syn.b" + std::to_string(lv.res) + ".x", A, lv.res, lv.ch, true);
            capture("syn.b" + std::to_string(lv.res) + ".img", img, lv.res, 3, false);
        }
        return img;
    }
};

migan_exec make_exec(migan_model& m, int B, void* stream) {
    if (B < 1) throw except("migan: empty batch");
    if (B > m.ws_batch) {
        if (grow(m.ws, plan(m, B).total, {m.backend->stream, stream})) m.graphs.clear();
        m.ws_batch = B;
    }
    return migan_exec{{m, stream, m.weight_arena.ptr}, static_cast<uint8_t*>(m.ws.ptr), plan(m, B), B};
}

// the u8 -> rgba launch list on the workspace's own input / output buffers
void run_u8(migan_exec& ex, int img_channels) {
    migan_model& m = ex.m;
    const int R = m.params.resolution;
    const int64_t px = (int64_t)ex.B * R * R;
    ex.mark("preprocess", (double)px * m.levels[0].ch * 10, (double)px * (img_channels + 1 + m.levels[0].ch * 2));
    VX(vx_migan_preprocess(static_cast<const uint8_t*>(ex.at(ex.L.in_img)), img_channels, static_cast<const uint8_t*>(ex.at(ex.L.in_mask)), nullptr,
                           ex.w(m.fromrgb_w), ex.w(m.fromrgb_b), ex.at(ex.L.act[0]), px, m.levels[0].ch, ex.stream));
    float* img = ex.generate();
    ex.mark("postprocess", 0, (double)px * 17);
    VX(vx_migan_postprocess(img, static_cast<const uint8_t*>(ex.at(ex.L.in_mask)), static_cast<uint8_t*>(ex.at(ex.L.out_rgba)), px, ex.stream));
}

} // namespace

void migan_compute_batch_device(migan_model& m, void const* img_dev, int img_channels, void const* mask_dev, int batch, void* out_rgba_dev, void* stream) {
    if (!img_dev || !mask_dev || !out_rgba_dev) throw except("migan: null input/output pointer");
    if (img_channels != 3 && img_channels != 4) throw except("migan: image must have 3 or 4 channels, got %d", img_channels);
    device_turn turn(*m.backend);
    void* s = stream ? stream : m.backend->stream;
    migan_exec ex = make_exec(m, batch, s);
    const int R = m.params.resolution;
    const size_t px = (size_t)batch * R * R;
    VX(vx_memcpy_d2d(ex.at(ex.L.in_img), img_dev, px * img_channels, s));
    VX(vx_memcpy_d2d(ex.at(ex.L.in_mask), mask_dev, px, s));
    replay_or_run(m, m.graphs, batch * 8 + img_channels, s, [&] {
        run_u8(ex, img_channels);
        ex.finish_timing();
    });
    VX(vx_memcpy_d2d(out_rgba_dev, ex.at(ex.L.out_rgba), px * 4, s));
    if (!stream) VX(vx_stream_sync(s));
}

void migan_compute_batch_host(migan_model& m, uint8_t const* img, int img_channels, uint8_t const* mask, int batch, uint8_t* out_rgba) {
    if (!img || !mask || !out_rgba) throw except("migan: null input/output pointer");
    if (batch < 1) throw except("migan: empty batch");
    if (img_channels != 3 && img_channels != 4) throw except("migan: image must have 3 or 4 channels, got %d", img_channels);
    device_turn turn(*m.backend);
    void* s = m.backend->stream;
    const int R = m.params.resolution;
    const size_t px = (size_t)batch * R * R;
    device_buffer din(px * img_channels), dmask(px), dout(px * 4);
    VX(vx_memcpy_h2d(din.ptr, img, px * img_channels, s));
    VX(vx_memcpy_h2d(dmask.ptr, mask, px, s));
    migan_compute_batch_device(m, din.ptr, img_channels, dmask.ptr, batch, dout.ptr, s);
    VX(vx_memcpy_d2h(out_rgba, dout.ptr, px * 4, s));
    VX(vx_stream_sync(s));
}

void migan_generate_host(migan_model& m, float const* in4, int n, float* out_rgb) {
    if (!in4 || !out_rgb) throw except("migan: null input/output pointer");
    device_turn turn(*m.backend);
    void* s = m.backend->stream;
    migan_exec ex = make_exec(m, n, s);
    const int R = m.params.resolution;
    const int64_t px = (int64_t)n * R * R;
    VX(vx_memcpy_h2d(ex.at(ex.L.in4), in4, (size_t)px * 16, s));
    ex.mark("preprocess", 0, 0);
    VX(vx_migan_preprocess(nullptr, 0, nullptr, static_cast<const float*>(ex.at(ex.L.in4)), ex.w(m.fromrgb_w), ex.w(m.fromrgb_b), ex.at(ex.L.act[0]), px,
                           m.levels[0].ch, s));
    float* img = ex.generate();
    ex.finish_timing();
    VX(vx_memcpy_d2h(out_rgb, img, (size_t)px * 12, s));
    VX(vx_stream_sync(s));
}

// vision.cpp:172-203 + migan_process_input / migan_process_output (migan.cpp:181-206) + image_set_alpha with the original mask
image_data migan_compute(migan_model& m, image_view image, image_view mask) {
    if (mask.format != image_format::alpha_u8) throw except("migan: second input image (mask) must be alpha_u8 format");
    const int ch = n_channels(image.format);
    if (is_float(image.format) || (ch != 3 && ch != 4)) throw except("Unsupported image format for migan image input");
    if (mask.extent[0] != image.extent[0] || mask.extent[1] != image.extent[1])
        throw except("migan: mask extent %dx%d differs from the image's %dx%d", mask.extent[0], mask.extent[1], image.extent[0], image.extent[1]);
    const int R = m.params.resolution;
    const i32x2 res{{R, R}};
    auto tight = [](image_view v) { // rows packed (stride may be larger than width * pixel bytes)
        std::vector<uint8_t> out((size_t)v.extent[0] * v.extent[1] * n_bytes(v.format));
        const size_t row = (size_t)v.extent[0] * n_bytes(v.format);
        for (int y = 0; y < v.extent[1]; ++y) memcpy(out.data() + y * row, static_cast<const uint8_t*>(v.data) + (size_t)y * v.stride, row);
        return out;
    };
    auto at_res = [&](image_view v) {
        if (v.extent[0] == R && v.extent[1] == R) return tight(v);
        image_data d = image_scale(v, res);
        return tight(view_of(d));
    };
    std::vector<uint8_t> img_r = at_res(image), mask_r = at_res(mask);
    std::vector<uint8_t> rgba((size_t)R * R * 4);
    std::vector<float> rgb;
    { // the generator's rgb f32 (the u8 path's rgba is not used here: the output is scaled as f32 first)
        device_turn turn(*m.backend);
        void* s = m.backend->stream;
        migan_exec ex = make_exec(m, 1, s);
        const int64_t px = (int64_t)R * R;
        VX(vx_memcpy_h2d(ex.at(ex.L.in_img), img_r.data(), img_r.size(), s));
        VX(vx_memcpy_h2d(ex.at(ex.L.in_mask), mask_r.data(), mask_r.size(), s));
        ex.mark("preprocess", 0, 0);
        VX(vx_migan_preprocess(static_cast<const uint8_t*>(ex.at(ex.L.in_img)), ch, static_cast<const uint8_t*>(ex.at(ex.L.in_mask)), nullptr,
                               ex.w(m.fromrgb_w), ex.w(m.fromrgb_b), ex.at(ex.L.act[0]), px, m.levels[0].ch, s));
        float* img = ex.generate();
        ex.finish_timing();
        rgb.resize((size_t)px * 3);
        VX(vx_memcpy_d2h(rgb.data(), img, rgb.size() * 4, s));
        VX(vx_stream_sync(s));
    }
    image_view out_f32{res, R * 12, image_format::rgb_f32, rgb.data()};
    image_data scaled;
    if (image.extent[0] != R || image.extent[1] != R) {
        scaled = image_scale(out_f32, image.extent);
        out_f32 = view_of(scaled);
    }
    image_data out = image_f32_to_u8(out_f32, image_format::rgba_u8, 0.5f, 0.5f);
    std::vector<uint8_t> alpha = tight(mask); // image_set_alpha(output, mask): the original, un-inverted mask
    for (size_t i = 0; i < alpha.size(); ++i) out.data[i * 4 + 3] = alpha[i];
    return out;
}

} // namespace visp
