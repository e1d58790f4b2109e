// The drop-in C ABI (include/visp_c_api.h). Part 1 restates the reference's
// src/visp/c-api.cpp:145-253 symbol for symbol on top of this backend; part 2 is the batched
// extension. Error convention: return 1 on success, 0 on error + thread-local message
// (reference c-api.cpp:6-21).
#include "../../include/visp_c_api.h"

#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <string>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/visp_hip_kernels.h"
#include "depthany.h"
#include "esrgan.h"
#include "migan.h"
#include "yolov9t.h"
#include "tinyvit.h"
#include "swin.h"
#include "birefnet.h"
#include "matting.h"
#include "graph.h"
#include "visp_util.h"

using namespace visp;

struct visp_image_data : image_data {};
struct visp_device : backend_device {};
struct visp_graph : graph {};
struct visp_weights { std::shared_ptr<weight_store> store; };
struct visp_file { model_file file; };
// visp_model stays opaque: handles are depthany_model* (any_model in the reference, c-api.cpp:193)

namespace {

thread_local char g_error[512] = {0};

void set_error(const char* msg) { snprintf(g_error, sizeof g_error, "%s", msg); }

template <typename F>
int32_t handle_errors(F&& f) {
    try {
        f();
    } catch (std::exception const& e) {
        set_error(e.what());
        return 0;
    } catch (...) {
        set_error("unknown error");
        return 0;
    }
    return 1;
}

int32_t family_of(visp_model const* m) {
    if (!m) throw except("model handle is null");
    return reinterpret_cast<model_base const*>(m)->family;
}
// the handle as family T's model, or the family's refusal
template <typename T>
T& as(visp_model const* m, int32_t family, char const* what) {
    if (family_of(m) != family) throw except("model handle is not %s (family %d)", what, family_of(m));
    return *static_cast<T*>(reinterpret_cast<model_base*>(const_cast<visp_model*>(m)));
}
depthany_model& as_depthany(visp_model const* m) { return as<depthany_model>(m, VISP_DEPTH_ANYTHING, "a depth_anything model"); }
esrgan_model& as_esrgan(visp_model const* m) { return as<esrgan_model>(m, VISP_ESRGAN, "an esrgan model"); }
migan_model& as_migan(visp_model const* m) { return as<migan_model>(m, VISP_MIGAN, "a migan model"); }
yolov9t_model& as_yolov9t(visp_model const* m) { return as<yolov9t_model>(m, family_yolov9t, "a yolov9t model"); }
sam_model& as_sam(visp_model const* m) { return as<sam_model>(m, VISP_SAM, "a sam model"); }
swin_model& as_swin(visp_model const* m) { return as<swin_model>(m, VISP_BIREFNET, "a swin encoder"); } // the encoder half of the birefnet family (visp_swin_load)
birefnet_model& as_birefnet(visp_model* m) {
    swin_model& s = as_swin(m);
    if (!s.full) throw except("model handle is a swin encoder (visp_swin_load), not a birefnet model");
    return static_cast<birefnet_model&>(s);
}
visp_model* handle_of(model_base* m) { return reinterpret_cast<visp_model*>(m); }

int32_t detect_family(model_file const& file) { // reference vision.cpp:7-21
    std::string_view arch = file.arch();
    if (arch == "mobile-sam") return VISP_SAM;
    if (arch == "birefnet") return VISP_BIREFNET;
    if (arch == "depthanything") return VISP_DEPTH_ANYTHING;
    if (arch == "migan") return VISP_MIGAN;
    if (arch == "esrgan") return VISP_ESRGAN;
    return VISP_FAMILY_COUNT;
}

void require_built(int32_t family) {
    if (family < 0 || family >= VISP_FAMILY_COUNT) throw except("Unsupported model family");
    if (family != VISP_DEPTH_ANYTHING && family != VISP_ESRGAN && family != VISP_SAM && family != VISP_BIREFNET)
        throw except("Model family %d is not built in this backend (MI355X backend implements depth_anything, esrgan, sam and birefnet)", family);
}

// the accessors every family with captures / timing shares (`who` names the family in the null-argument message)
void read_capture(model_base& m, char const* who, char const* name, float* host_out, int64_t capacity, int64_t* n_written, int64_t shape[4]) {
    if (!name || !n_written) throw except("%s: null argument", who);
    device_turn turn(*m.backend);
    auto it = m.capture_bufs.find(name);
    if (it == m.capture_bufs.end()) throw except("capture '%s' not available (enable captures before compute)", name);
    capture_entry const& c = it->second;
    int64_t n = c.shape[0] * c.shape[1] * c.shape[2] * c.shape[3];
    *n_written = n;
    if (shape) memcpy(shape, c.shape, sizeof(int64_t) * 4);
    if (n > capacity) return; // caller learns the size and retries
    if (c.f16) {
        std::unique_ptr<uint16_t[]> tmp(new uint16_t[(size_t)n]);
        if (!vx_memcpy_d2h(tmp.get(), c.dev.ptr, (size_t)n * 2, m.backend->stream)) throw except("%s", vx_last_error());
        for (int64_t i = 0; i < n; ++i) host_out[i] = f16_to_f32(tmp[(size_t)i]);
    } else {
        if (!vx_memcpy_d2h(host_out, c.dev.ptr, (size_t)n * 4, m.backend->stream)) throw except("%s", vx_last_error());
    }
}

void read_timing(model_base const& m, visp_timing* out, int32_t cap, int32_t* n) {
    int32_t count = 0;
    for (timing_entry const& t : m.last_timing) {
        if (count >= cap) break;
        snprintf(out[count].name, sizeof out[count].name, "%s", t.name.c_str());
        out[count].ms = t.ms;
        out[count].launches = t.launches;
        out[count].flops = t.flops;
        out[count].bytes = t.bytes;
        ++count;
    }
    *n = count;
}

void return_image(image_data&& img, visp_image_view* out_image, visp_image_data** out_data) {
    auto* owned = new visp_image_data;
    static_cast<image_data&>(*owned) = std::move(img);
    *out_data = owned;
    out_image->width = owned->extent[0];
    out_image->height = owned->extent[1];
    out_image->stride = owned->extent[0] * n_bytes(owned->format);
    out_image->format = int32_t(owned->format);
    out_image->data = owned->data.get();
}

// a caller's view as visp::image_view: present, with data, a format of the enum, a positive extent and rows no shorter than their pixels
image_view host_view(char const* who, visp_image_view const* v) {
    if (!v || !v->data) throw except("%s: null argument", who);
    if (v->format < 0 || v->format > int32_t(image_format::alpha_f32)) throw except("Unsupported image format [%d]", v->format);
    if (v->width < 1 || v->height < 1) throw except("%s: empty image (%dx%d)", who, v->width, v->height);
    if ((int64_t)v->stride < (int64_t)v->width * n_bytes(image_format(v->format))) throw except("%s: row stride %d is shorter than a row", who, v->stride);
    return image_view{i32x2{{v->width, v->height}}, v->stride, image_format(v->format), v->data};
}

} // namespace

extern "C" {

char const* visp_get_last_error(void) { return g_error; }

void visp_image_destroy(visp_image_data* img) { delete img; }

// host-only: the reference's image_scale (src/visp/image.cpp:328-356, what depthany_compute / sam_encode apply to inputs whose
// extent is not the model's); no device involved
int32_t visp_image_scale(visp_image_view const* src, int32_t width, int32_t height, visp_image_view* out_image, visp_image_data** out_data) {
    return handle_errors([&]() {
        if (!src || !src->data || !out_image || !out_data) throw except("visp_image_scale: null argument");
        if (src->format < 0 || src->format > int32_t(image_format::alpha_f32)) throw except("Unsupported image format [%d]", src->format);
        image_view v{i32x2{{src->width, src->height}}, src->stride, image_format(src->format), src->data};
        return_image(image_scale(v, i32x2{{width, height}}), out_image, out_data);
    });
}

int32_t visp_image_u8_to_f32(visp_image_view const* src, int32_t format, float const offset[4], float const scale[4], visp_image_view* out_image,
                             visp_image_data** out_data) {
    return handle_errors([&]() {
        if (!src || !src->data || !offset || !scale || !out_image || !out_data) throw except("visp_image_u8_to_f32: null argument");
        if (src->format < 0 || src->format > int32_t(image_format::alpha_f32) || format < 0 || format > int32_t(image_format::alpha_f32))
            throw except("Unsupported image format [%d]", src->format);
        image_view v{i32x2{{src->width, src->height}}, src->stride, image_format(src->format), src->data};
        return_image(image_u8_to_f32(v, image_format(format), offset, scale), out_image, out_data);
    });
}

int32_t visp_image_normalize(visp_image_view const* src, float min, float max, visp_image_view* out_image, visp_image_data** out_data) {
    return handle_errors([&]() {
        if (!src || !src->data || !out_image || !out_data) throw except("visp_image_normalize: null argument");
        if (src->format != int32_t(image_format::alpha_f32)) throw except("visp_image_normalize: expected an alpha_f32 image, got format %d", src->format);
        image_view v{i32x2{{src->width, src->height}}, src->stride, image_format(src->format), src->data};
        return_image(image_normalize(v, min, max), out_image, out_data);
    });
}

int32_t visp_backend_load_all(char const*) { return 1; } // single built-in backend, nothing to load

int32_t visp_device_init(int32_t type, visp_device** out_device) {
    return handle_errors([&]() {
        if (type == VISP_BACKEND_CPU)
            throw except("Failed to initialize backend, no suitable device available (this build has no CPU backend)");
        if (type != VISP_BACKEND_AUTO && type != VISP_BACKEND_GPU)
            throw except("Failed to initialize backend, backend type %d is not available in this build", type);
        *out_device = static_cast<visp_device*>(backend_init(0));
    });
}

int32_t visp_hip_device_init(int32_t device_index, visp_device** out_device) {
    return handle_errors([&]() { *out_device = static_cast<visp_device*>(backend_init(device_index)); });
}

void visp_device_destroy(visp_device* d) { delete static_cast<backend_device*>(d); }

int32_t visp_device_type(visp_device const* d) { return int32_t(d->type()); }
char const* visp_device_name(visp_device const* d) { return d->name.c_str(); }
char const* visp_device_description(visp_device const* d) { return d->description.c_str(); }

int32_t visp_model_detect_family(char const* filepath, int32_t* out_family) {
    return handle_errors([&]() {
        model_file file = model_load(filepath, /*header_only=*/true);
        *out_family = detect_family(file);
    });
}

// host-only: parses the whole file (header AND tensor data ranges) without touching a device; what visp_model_load checks first
int32_t visp_gguf_validate(char const* filepath, int32_t* out_n_tensors) {
    return handle_errors([&]() {
        model_file file = model_load(filepath, /*header_only=*/false);
        if (out_n_tensors) *out_n_tensors = (int32_t)file.tensors.size();
    });
}

int32_t visp_model_load_ex(char const* filepath, visp_device const* dev, int32_t arch, int32_t flags, visp_model** out) {
    return handle_errors([&]() {
        if (!dev) throw except("device handle is null");
        int32_t family = arch;
        if (family == VISP_FAMILY_COUNT) {
            model_file file = model_load(filepath, true);
            family = detect_family(file);
        }
        require_built(family);
        if (family == VISP_ESRGAN) *out = handle_of(esrgan_load_model(filepath, *dev, flags));
        else if (family == VISP_SAM) *out = handle_of(sam_load_model(filepath, *dev, flags));
        else if (family == VISP_BIREFNET) {
            if (flags & VISP_LOAD_NO_UPLOAD) throw except("birefnet: load without upload is not supported (every rank reads the file)");
            *out = handle_of(birefnet_load_model(filepath, *dev));
        }
        else *out = handle_of(depthany_load_model(filepath, *dev, flags));
    });
}

int32_t visp_model_load(char const* filepath, visp_device const* dev, int32_t arch, visp_model** out) {
    return visp_model_load_ex(filepath, dev, arch, VISP_LOAD_DEFAULT, out);
}

void visp_model_destroy(visp_model* model, int32_t arch) {
    if (!model) return;
    // the handle carries its own family; `arch` is what the reference's destroy switch uses (c-api.cpp:224-229)
    (void)arch;
    delete reinterpret_cast<model_base*>(model); // (virtual destructor)
}

int32_t visp_model_compute(visp_model* model, int32_t family, visp_image_view* inputs, int32_t n_inputs, int32_t* args, int32_t n_args,
                           visp_image_view* out_image, visp_image_data** out_data) {
    return handle_errors([&]() {
        if (family == VISP_MIGAN && model && family_of(model) == VISP_MIGAN) { // model_funcs<migan>::compute (reference c-api.cpp:87-92)
            if (n_inputs != 2) throw except("Expected %d input images, but got %d.", 2, n_inputs);
            image_view in[2];
            for (int i = 0; i < 2; ++i) in[i] = image_view{i32x2{{inputs[i].width, inputs[i].height}}, inputs[i].stride, image_format(inputs[i].format), inputs[i].data};
            return_image(migan_compute(as_migan(model), in[0], in[1]), out_image, out_data);
            return;
        }
        require_built(family);
        if (family_of(model) != family) throw except("model handle belongs to family %d, not %d", family_of(model), family);
        if (n_inputs != 1) throw except("Expected %d input images, but got %d.", 1, n_inputs);
        image_view in;
        in.extent = {{inputs[0].width, inputs[0].height}};
        in.stride = inputs[0].stride;
        in.format = image_format(inputs[0].format);
        in.data = inputs[0].data;
        if (family == VISP_SAM) { // model_funcs<sam>::compute = sam_encode + sam_compute (reference c-api.cpp:34-52)
            if (n_args != 2 && n_args != 4) throw except("sam: bad number of arguments (%d), must be 2 or 4", n_args);
            sam_model& sm = as_sam(model);
            sam_encode(sm, in);
            return_image(sam_compute(sm, args, n_args), out_image, out_data);
            return;
        }
        if (family == VISP_BIREFNET) { // model_funcs<birefnet>::compute (reference c-api.cpp:59-62)
            return_image(birefnet_compute(as_birefnet(model), in), out_image, out_data);
            return;
        }
        if (family == VISP_ESRGAN) { // model_funcs<esrgan>::compute (reference c-api.cpp:103-106)
            return_image(esrgan_compute(as_esrgan(model), in), out_image, out_data);
            return;
        }
        // model_funcs<depth_anything>::compute (reference c-api.cpp:72-77)
        image_data result_f32 = depthany_compute(as_depthany(model), in);
        image_data normalized = image_normalize(view_of(result_f32));
        return_image(image_f32_to_u8(view_of(normalized), image_format::alpha_u8), out_image, out_data);
    });
}

// ---- extension ---------------------------------------------------------------------------

int32_t visp_depthany_weights_arena(visp_model* m, void** device_ptr, size_t* n_bytes) {
    return handle_errors([&]() {
        depthany_model& dm = as_depthany(m);
        *device_ptr = dm.weight_arena.ptr;
        *n_bytes = dm.weight_arena.bytes;
    });
}

int32_t visp_depthany_weights_ready(visp_model* m) {
    return handle_errors([&]() { depthany_weights_ready(as_depthany(m)); });
}

int32_t visp_depthany_get_info(visp_model const* m, visp_depthany_info* out) {
    return handle_errors([&]() {
        depthany_params const& p = as_depthany(m).params;
        out->patch_size = p.dino.patch_size;
        out->embed_dim = p.dino.embed_dim;
        out->n_layers = p.dino.n_layers;
        out->n_heads = p.dino.n_heads;
        out->image_size = p.image_size;
        out->image_multiple = p.image_multiple;
        for (int i = 0; i < 4; ++i) out->feature_layers[i] = p.feature_layers[i];
        out->max_depth = p.max_depth;
    });
}

int32_t visp_depthany_image_extent(visp_model const* m, int32_t w, int32_t h, int32_t* out_w, int32_t* out_h) {
    return handle_errors([&]() {
        if (w <= 0 || h <= 0) throw except("invalid extent %dx%d", w, h);
        i32x2 e = depthany_image_extent(i32x2{{w, h}}, as_depthany(m).params);
        *out_w = e[0];
        *out_h = e[1];
    });
}

int32_t visp_depthany_reserve(visp_model* m, int32_t batch, int32_t w, int32_t h) {
    return handle_errors([&]() { depthany_reserve(as_depthany(m), batch, w, h); });
}

int32_t visp_depthany_compute_batch_device(visp_model* m, void const* rgb, int32_t batch, int32_t w, int32_t h, void* out,
                                           void* raw_out, void* stream) {
    return handle_errors([&]() {
        if (!rgb || !out) throw except("depthany: null input/output pointer");
        depthany_compute_batch_device(as_depthany(m), rgb, batch, w, h, out, raw_out, stream);
    });
}

int32_t visp_depthany_compute_f32(visp_model* m, visp_image_view const* image, visp_image_view* out_image, visp_image_data** out_data) {
    return handle_errors([&]() {
        if (!image || !image->data || !out_image || !out_data) throw except("depthany: null argument");
        image_view in{i32x2{{image->width, image->height}}, image->stride, image_format(image->format), image->data};
        return_image(depthany_compute(as_depthany(m), in), out_image, out_data);
    });
}

int32_t visp_depthany_compute_batch_host(visp_model* m, uint8_t const* rgb, int32_t batch, int32_t w, int32_t h, float* out,
                                         float* raw_out) {
    return handle_errors([&]() {
        if (!rgb || !out) throw except("depthany: null input/output pointer");
        depthany_compute_batch_host(as_depthany(m), rgb, batch, w, h, out, raw_out);
    });
}

// Multi-GPU without Python: one model per device (each loaded on its own visp_hip_device_init(i) device), one host thread per
// model, contiguous image shards whose sizes differ by at most one (the partitioning of vision.cpp_amd/dist.py::shard_range),
// no data-path collective -- images are independent units (image_normalize is per image, reference image.cpp:537-576). Each shard
// goes through its model's overlapped host pipeline in chunks of 32 (pinned staging, H2D / forward / D2H on three streams).
int32_t visp_depthany_compute_sharded(visp_model* const* models, int32_t n_models, uint8_t const* rgb, int32_t batch, int32_t w, int32_t h,
                                      float* out) {
    return handle_errors([&]() {
        if (!models || n_models <= 0 || !rgb || !out) throw except("depthany sharded: null / empty argument");
        if (batch <= 0 || w <= 0 || h <= 0) throw except("depthany sharded: invalid batch/extent %d x %dx%d", batch, w, h);
        std::vector<depthany_model*> ms;
        for (int i = 0; i < n_models; ++i) {
            ms.push_back(&as_depthany(models[i]));
            for (int j = 0; j < i; ++j)
                if (ms[(size_t)j] == ms[(size_t)i]) throw except("depthany sharded: model %d is passed twice (one model = one thread at a time)", i);
        }
        std::vector<std::string> errors((size_t)n_models);
        std::vector<std::thread> threads;
        // models that sit on the same backend_device share its compute stream (a one-GPU rehearsal of the multi-device call): every call
        // that touches that stream holds the device's turn (device_turn, csrc/model.h), so the shards interleave chunk by chunk and a
        // hipGraph capture by one thread is never crossed by another thread's launches
        const int base = batch / n_models, rem = batch % n_models;
        for (int i = 0; i < n_models; ++i) {
            const int begin = i * base + std::min(i, rem), count = base + (i < rem ? 1 : 0);
            if (count == 0) continue;
            threads.emplace_back([&, i, begin, count]() {
                try {
                    depthany_compute_shard_host(*ms[(size_t)i], rgb + (size_t)begin * h * w * 3, count, w, h, out + (size_t)begin * h * w);
                } catch (std::exception const& e) {
                    errors[(size_t)i] = e.what();
                } catch (...) {
                    errors[(size_t)i] = "unknown error";
                }
            });
        }
        for (auto& t : threads) t.join();
        for (int i = 0; i < n_models; ++i)
            if (!errors[(size_t)i].empty()) throw except("depthany sharded: shard %d failed: %s", i, errors[(size_t)i].c_str());
    });
}

int32_t visp_depthany_pipeline_create(visp_model* m, int32_t batch, int32_t w, int32_t h, int32_t n_slots, visp_depthany_pipeline** out) {
    return handle_errors([&]() { *out = reinterpret_cast<visp_depthany_pipeline*>(depthany_pipeline_create(as_depthany(m), batch, w, h, n_slots)); });
}
void visp_depthany_pipeline_destroy(visp_depthany_pipeline* p) { delete reinterpret_cast<depthany_pipeline*>(p); }
int32_t visp_depthany_pipeline_input(visp_depthany_pipeline* p, uint8_t** out_pinned) {
    return handle_errors([&]() {
        if (!p || !out_pinned) throw except("depthany pipeline: null argument");
        *out_pinned = depthany_pipeline_input(*reinterpret_cast<depthany_pipeline*>(p));
    });
}
int32_t visp_depthany_pipeline_submit(visp_depthany_pipeline* p, uint8_t const* rgb_u8, int32_t* out_ticket) {
    return handle_errors([&]() {
        if (!p || !out_ticket) throw except("depthany pipeline: null argument");
        *out_ticket = depthany_pipeline_submit(*reinterpret_cast<depthany_pipeline*>(p), rgb_u8);
    });
}
int32_t visp_depthany_pipeline_wait(visp_depthany_pipeline* p, int32_t ticket, float const** out_pinned) {
    return handle_errors([&]() {
        if (!p || !out_pinned) throw except("depthany pipeline: null argument");
        *out_pinned = depthany_pipeline_wait(*reinterpret_cast<depthany_pipeline*>(p), ticket);
    });
}

int32_t visp_depthany_use_graph(visp_model* m, int32_t enable) {
    return handle_errors([&]() {
        depthany_model& dm = as_depthany(m);
        dm.use_graph = enable != 0;
        if (!enable) depthany_drop_captured_steps(dm);
    });
}

int32_t visp_depthany_set_schedule(visp_model* m, int32_t schedule) {
    return handle_errors([&]() {
        depthany_model& dm = as_depthany(m);
        if (schedule < -1 || schedule > 1) throw except("visp_depthany_set_schedule: unknown schedule %d (-1 = auto, 0 = GEMM launches, 1 = token-stationary block kernel)", schedule);
        if (schedule == 1 && !dm.block_shape) throw except("visp_depthany_set_schedule: the block kernel is built for embed dim 384 / mlp 1536 / head dim 64 only");
        dm.schedule = schedule;
        depthany_drop_captured_steps(dm); // (steps are keyed by the schedule: the other one is lowered on first use)
    });
}

int32_t visp_depthany_set_split(visp_model* m, int32_t n) {
    return handle_errors([&]() {
        depthany_model& dm = as_depthany(m);
        if (n < 0 || n > 4) throw except("visp_depthany_set_split: %d sub-batches (0 = automatic, 1 = none, at most 4)", n);
        dm.split = n;
    });
}

int32_t visp_depthany_enable_captures(visp_model* m, int32_t enable) {
    return handle_errors([&]() { as_depthany(m).captures = enable != 0; });
}

int32_t visp_depthany_read_capture(visp_model* m, char const* name, float* host_out, int64_t capacity, int64_t* n_written,
                                   int64_t shape[4]) {
    return handle_errors([&]() { read_capture(as_depthany(m), "depthany", name, host_out, capacity, n_written, shape); });
}

int32_t visp_depthany_enable_timing(visp_model* m, int32_t enable) {
    // 1 = the whole batch on one stream; 2 = the step's own launch shapes (sub-batches on parallel streams, every launch timed on its stream)
    return handle_errors([&]() { as_depthany(m).timing = enable != 0; as_depthany(m).timing_split = enable == 2; });
}

int32_t visp_depthany_read_timing(visp_model* m, visp_timing* out, int32_t cap, int32_t* n) {
    return handle_errors([&]() { read_timing(as_depthany(m), out, cap, n); });
}

// ---- ESRGAN extension ----------------------------------------------------------------------

int32_t visp_esrgan_get_info(visp_model const* m, visp_esrgan_info* out) {
    return handle_errors([&]() {
        esrgan_model const& em = as_esrgan(m);
        out->scale = em.params.scale;
        out->n_blocks = em.params.n_blocks;
        out->n_filters = em.nf;
        out->growth = em.gc;
        out->tile_group = em.tile_group;
    });
}

int32_t visp_esrgan_set_tile_group(visp_model* m, int32_t tiles) {
    return handle_errors([&]() {
        if (tiles < 1) throw except("esrgan: tile group must be >= 1");
        as_esrgan(m).tile_group = tiles;
    });
}

int32_t visp_esrgan_weights_arena(visp_model* m, void** device_ptr, size_t* n_bytes) {
    return handle_errors([&]() {
        esrgan_model& em = as_esrgan(m);
        *device_ptr = em.weight_arena.ptr;
        *n_bytes = em.weight_arena.bytes;
    });
}

int32_t visp_esrgan_weights_ready(visp_model* m) {
    return handle_errors([&]() { esrgan_weights_ready(as_esrgan(m)); });
}

int32_t visp_esrgan_tile_layout(int32_t w, int32_t h, int32_t scale, int32_t out8[8]) {
    return handle_errors([&]() {
        tile_layout t = tile_scale(tile_layout({{w, h}}, 224, 16), scale);
        int32_t v[8] = {t.image_extent[0], t.image_extent[1], t.overlap[0], t.overlap[1], t.n_tiles[0], t.n_tiles[1], t.tile_size[0], t.tile_size[1]};
        memcpy(out8, v, sizeof v);
    });
}

int32_t visp_esrgan_compute_batch_device(visp_model* m, void const* img, int32_t batch, int32_t w, int32_t h, int32_t format, void* out_rgba,
                                         void* stream) {
    return handle_errors([&]() {
        if (!img || !out_rgba) throw except("esrgan: null input/output pointer");
        esrgan_compute_batch_device(as_esrgan(m), img, batch, w, h, image_format(format), out_rgba, stream);
    });
}

int32_t visp_esrgan_compute_batch_host(visp_model* m, uint8_t const* img, int32_t batch, int32_t w, int32_t h, int32_t format, uint8_t* out_rgba) {
    return handle_errors([&]() {
        if (!img || !out_rgba) throw except("esrgan: null input/output pointer");
        esrgan_compute_batch_host(as_esrgan(m), img, batch, w, h, image_format(format), out_rgba);
    });
}

int32_t visp_esrgan_generate_host(visp_model* m, float const* rgb, int32_t n, int32_t w, int32_t h, float* out) {
    return handle_errors([&]() {
        if (!rgb || !out) throw except("esrgan: null input/output pointer");
        esrgan_generate_host(as_esrgan(m), rgb, n, w, h, out);
    });
}

int32_t visp_esrgan_enable_timing(visp_model* m, int32_t enable) {
    return handle_errors([&]() { as_esrgan(m).timing = enable != 0; });
}

int32_t visp_esrgan_read_timing(visp_model* m, visp_timing* out, int32_t cap, int32_t* n) {
    return handle_errors([&]() { read_timing(as_esrgan(m), out, cap, n); });
}

// ---- MI-GAN (loaded only through visp_migan_load) ----

int32_t visp_migan_load(char const* filepath, visp_device const* dev, visp_model** out) {
    return handle_errors([&]() {
        if (!dev || !out) throw except("migan: null argument");
        *out = handle_of(migan_load_model(filepath, *dev));
    });
}

int32_t visp_migan_get_info(visp_model const* m, visp_migan_info* out) {
    return handle_errors([&]() {
        migan_model const& mm = as_migan(m);
        memset(out, 0, sizeof *out);
        out->resolution = mm.params.resolution;
        out->n_levels = (int32_t)mm.levels.size();
        for (size_t i = 0; i < mm.levels.size() && i < 9; ++i) out->channels[i] = mm.levels[i].ch;
    });
}

int32_t visp_migan_compute(visp_model* m, visp_image_view const* image, visp_image_view const* mask, visp_image_view* out_image, visp_image_data** out_data) {
    return handle_errors([&]() {
        if (!image || !image->data || !mask || !mask->data || !out_image || !out_data) throw except("migan: null argument");
        image_view im{i32x2{{image->width, image->height}}, image->stride, image_format(image->format), image->data};
        image_view mk{i32x2{{mask->width, mask->height}}, mask->stride, image_format(mask->format), mask->data};
        return_image(migan_compute(as_migan(m), im, mk), out_image, out_data);
    });
}

int32_t visp_migan_compute_batch_device(visp_model* m, void const* img, int32_t channels, void const* mask, int32_t batch, void* out_rgba, void* stream) {
    return handle_errors([&]() { migan_compute_batch_device(as_migan(m), img, channels, mask, batch, out_rgba, stream); });
}

int32_t visp_migan_compute_batch_host(visp_model* m, uint8_t const* img, int32_t channels, uint8_t const* mask, int32_t batch, uint8_t* out_rgba) {
    return handle_errors([&]() { migan_compute_batch_host(as_migan(m), img, channels, mask, batch, out_rgba); });
}

int32_t visp_migan_generate_host(visp_model* m, float const* in4, int32_t n, float* out_rgb) {
    return handle_errors([&]() { migan_generate_host(as_migan(m), in4, n, out_rgb); });
}

int32_t visp_migan_enable_captures(visp_model* m, int32_t enable) {
    return handle_errors([&]() { as_migan(m).captures = enable != 0; });
}

int32_t visp_migan_read_capture(visp_model* m, char const* name, float* host_out, int64_t capacity, int64_t* n_written, int64_t shape[4]) {
    return handle_errors([&]() { read_capture(as_migan(m), "migan", name, host_out, capacity, n_written, shape); });
}

int32_t visp_migan_enable_timing(visp_model* m, int32_t enable) {
    return handle_errors([&]() { as_migan(m).timing = enable != 0; });
}

int32_t visp_migan_read_timing(visp_model* m, visp_timing* out, int32_t cap, int32_t* n) {
    return handle_errors([&]() { read_timing(as_migan(m), out, cap, n); });
}

// ---- YOLOv9t (loaded only through visp_yolov9t_load) ----

void visp_yolov9t_nms_defaults(visp_yolov9t_nms_params* out) {
    if (!out) return;
    yolo_nms_params d;
    *out = visp_yolov9t_nms_params{d.conf, d.iou, d.max_det, d.max_nms, d.max_wh};
}

static yolo_nms_params nms_params(visp_yolov9t_nms_params const* p) {
    yolo_nms_params d;
    if (p) d = yolo_nms_params{p->conf, p->iou, p->max_det, p->max_nms, p->max_wh};
    return d;
}

static visp_detection to_c(yolo_detection const& d) { return visp_detection{d.x1, d.y1, d.x2, d.y2, d.confidence, d.class_id, d.class_confidence}; }

static void write_detections(std::vector<yolo_detection> const& d, visp_detection* out, int32_t capacity, int32_t* n) {
    for (size_t i = 0; i < d.size() && (int64_t)i < capacity; ++i) out[i] = to_c(d[i]);
    *n = (int32_t)d.size();
}

static void write_batch(std::vector<std::vector<yolo_detection>> const& r, int max_det, visp_detection* out, int32_t* counts) {
    for (size_t b = 0; b < r.size(); ++b) {
        for (size_t i = 0; i < r[b].size(); ++i) out[b * (size_t)max_det + i] = to_c(r[b][i]);
        counts[b] = (int32_t)r[b].size();
    }
}

int32_t visp_yolov9t_load(char const* filepath, visp_device const* dev, visp_model** out) {
    return handle_errors([&]() {
        if (!filepath || !dev || !out) throw except("yolov9t: null argument");
        *out = handle_of(yolov9t_load_model(filepath, *dev));
    });
}

int32_t visp_yolov9t_get_info(visp_model const* m, visp_yolov9t_info* out) {
    return handle_errors([&]() {
        if (!out) throw except("yolov9t: null argument");
        yolov9t_model const& ym = as_yolov9t(m);
        *out = visp_yolov9t_info{ym.input_size, ym.num_classes, ym.reg_max, yolov9t_anchors(ym.input_size)};
    });
}

int32_t visp_yolov9t_detect(visp_model* m, visp_image_view const* image, visp_yolov9t_nms_params const* params, visp_detection* out, int32_t capacity,
                            int32_t* n) {
    return handle_errors([&]() {
        if (!image || !image->data || (!out && capacity > 0) || !n) throw except("yolov9t: null argument");
        image_view im{i32x2{{image->width, image->height}}, image->stride, image_format(image->format), image->data};
        write_detections(yolov9t_detect(as_yolov9t(m), im, nms_params(params)), out, capacity, n);
    });
}

int32_t visp_yolov9t_detect_batch_host(visp_model* m, uint8_t const* img, int32_t channels, int32_t batch, int32_t size,
                                       visp_yolov9t_nms_params const* params, visp_detection* out, int32_t* counts) {
    return handle_errors([&]() {
        if (!img || !out || !counts) throw except("yolov9t: null input/output pointer");
        yolo_nms_params p = nms_params(params);
        write_batch(yolov9t_detect_batch_host(as_yolov9t(m), img, channels, batch, size, p), p.max_det, out, counts);
    });
}

int32_t visp_yolov9t_detect_batch_device(visp_model* m, void const* img, int32_t channels, int32_t batch, int32_t size,
                                         visp_yolov9t_nms_params const* params, visp_detection* out, int32_t* counts, void* stream) {
    return handle_errors([&]() {
        if (!img || !out || !counts) throw except("yolov9t: null input/output pointer");
        yolo_nms_params p = nms_params(params);
        write_batch(yolov9t_detect_batch_device(as_yolov9t(m), img, channels, batch, size, p, stream), p.max_det, out, counts);
    });
}

int32_t visp_yolov9t_forward_host(visp_model* m, float const* rgb, int32_t n, int32_t size, float* boxes, float* scores) {
    return handle_errors([&]() { yolov9t_forward_host(as_yolov9t(m), rgb, n, size, boxes, scores); });
}

int32_t visp_yolov9t_letterbox(visp_image_view const* image, int32_t size, uint8_t* out_rgb, float* gain, float* pad_w, float* pad_h) {
    return handle_errors([&]() {
        if (!image || !image->data || !out_rgb || !gain || !pad_w || !pad_h) throw except("yolov9t: null argument");
        image_view im{i32x2{{image->width, image->height}}, image->stride, image_format(image->format), image->data};
        yolo_letterbox lb = yolov9t_letterbox(im, size);
        memcpy(out_rgb, lb.img.data.get(), (size_t)size * size * 3);
        *gain = lb.gain;
        *pad_w = lb.pad_w;
        *pad_h = lb.pad_h;
    });
}

int32_t visp_yolov9t_nms(float const* boxes, float const* scores, int32_t n_anchors, int32_t nc, visp_yolov9t_nms_params const* params, visp_detection* out,
                         int32_t capacity, int32_t* n) {
    return handle_errors([&]() {
        if ((!out && capacity > 0) || !n) throw except("yolov9t: null argument");
        write_detections(yolov9t_nms(boxes, scores, n_anchors, nc, nms_params(params)), out, capacity, n);
    });
}

int32_t visp_yolov9t_scale_boxes(visp_detection* dets, int32_t n, int32_t width, int32_t height, float gain, float pad_w, float pad_h) {
    return handle_errors([&]() {
        if ((!dets && n > 0) || n < 0) throw except("yolov9t: null argument");
        if (!(gain > 0.0f)) throw except("yolov9t: gain %g must be positive", gain);
        std::vector<yolo_detection> d((size_t)n);
        for (int32_t i = 0; i < n; ++i) d[(size_t)i] = yolo_detection{dets[i].x1, dets[i].y1, dets[i].x2, dets[i].y2, dets[i].confidence, dets[i].class_id, dets[i].class_confidence};
        yolov9t_scale_boxes(d, i32x2{{width, height}}, gain, pad_w, pad_h);
        for (int32_t i = 0; i < n; ++i) dets[i] = to_c(d[(size_t)i]);
    });
}

int32_t visp_yolov9t_last_split(visp_model const* m, float out_ms[3]) {
    return handle_errors([&]() {
        if (!out_ms) throw except("yolov9t: null argument");
        yolov9t_model const& ym = as_yolov9t(m);
        for (int i = 0; i < 3; ++i) out_ms[i] = ym.last_split_ms[i];
    });
}

int32_t visp_yolov9t_enable_captures(visp_model* m, int32_t enable) {
    return handle_errors([&]() { as_yolov9t(m).captures = enable != 0; });
}

int32_t visp_yolov9t_read_capture(visp_model* m, char const* name, float* host_out, int64_t capacity, int64_t* n_written, int64_t shape[4]) {
    return handle_errors([&]() { read_capture(as_yolov9t(m), "yolov9t", name, host_out, capacity, n_written, shape); });
}

int32_t visp_yolov9t_enable_timing(visp_model* m, int32_t enable) {
    return handle_errors([&]() { as_yolov9t(m).timing = enable != 0; });
}

int32_t visp_yolov9t_read_timing(visp_model* m, visp_timing* out, int32_t cap, int32_t* n) {
    return handle_errors([&]() { read_timing(as_yolov9t(m), out, cap, n); });
}

// ---- MobileSAM image encoder (TinyViT) ----

int32_t visp_sam_weights_arena(visp_model* m, void** device_ptr, size_t* n_bytes) {
    return handle_errors([&]() {
        sam_model& sm = as_sam(m);
        *device_ptr = sm.weight_arena.ptr;
        *n_bytes = sm.weight_arena.bytes;
    });
}

int32_t visp_sam_weights_ready(visp_model* m) {
    return handle_errors([&]() { sam_weights_ready(as_sam(m)); });
}

int32_t visp_sam_encode(visp_model* m, visp_image_view const* image) {
    return handle_errors([&]() {
        if (!image) throw except("sam: null image");
        image_view in{i32x2{{image->width, image->height}}, image->stride, image_format(image->format), image->data};
        sam_encode(as_sam(m), in);
    });
}

int32_t visp_sam_read_embedding(visp_model* m, float* host_out, int64_t capacity, int64_t shape[3]) {
    return handle_errors([&]() {
        sam_model& sm = as_sam(m);
        if (!sm.embed.ptr || sm.image_extent[0] <= 0) throw except("Missing image embeds, call sam_encode() first");
        const int R = sm.params.layers[3].resolution;
        shape[0] = R; shape[1] = R; shape[2] = 256;
        if (capacity < (int64_t)R * R * 256) throw except("sam: embedding buffer too small (%lld < %d)", (long long)capacity, R * R * 256);
        if (!vx_memcpy_d2h(host_out, sm.embed.ptr, (size_t)R * R * 256 * 4, sm.backend->stream) || !vx_stream_sync(sm.backend->stream))
            throw except("%s", vx_last_error());
    });
}

int32_t visp_sam_compute(visp_model* m, int32_t const* prompt, int32_t n_prompt, visp_image_view* out_image, visp_image_data** out_data) {
    return handle_errors([&]() {
        if (!prompt || !out_image || !out_data) throw except("sam: null argument");
        return_image(sam_compute(as_sam(m), prompt, n_prompt), out_image, out_data);
    });
}

int32_t visp_sam_read_masks(visp_model* m, float* masks, int64_t capacity, float iou[4]) {
    return handle_errors([&]() {
        sam_kept_logits const& kept = as_sam(m).last_single;
        if (kept.masks.empty()) throw except("sam: no mask logits kept: enable captures, then call sam_compute()");
        if (capacity < (int64_t)kept.masks.size()) throw except("sam: mask buffer too small (%lld < %zu)", (long long)capacity, kept.masks.size());
        memcpy(masks, kept.masks.data(), kept.masks.size() * sizeof(float));
        memcpy(iou, kept.iou.data(), kept.iou.size() * sizeof(float));
    });
}

int32_t visp_sam_compute_batch_device(visp_model* m, int32_t const* prompts, int32_t const* n_args, int32_t n, void* masks_u8_dev, void* iou_dev, void* chosen_dev,
                                      void* stream) {
    return handle_errors([&]() { sam_compute_batch_device(as_sam(m), prompts, n_args, n, masks_u8_dev, iou_dev, chosen_dev, stream); });
}

int32_t visp_sam_compute_batch_host(visp_model* m, int32_t const* prompts, int32_t const* n_args, int32_t n, uint8_t* masks_u8, float* iou, int32_t* chosen) {
    return handle_errors([&]() { sam_compute_batch_host(as_sam(m), prompts, n_args, n, masks_u8, iou, chosen); });
}

int32_t visp_sam_generate_masks_device(visp_model* m, int32_t const* prompts, int32_t const* n_args, int32_t n, float pred_iou_thresh, float stability_thresh,
                                       float stability_offset, float nms_iou_thresh, int32_t capacity, void* masks_u8_dev, void* info_i32_dev, void* info_f32_dev,
                                       void* counts_dev, void* stream) {
    return handle_errors([&]() {
        const sam_select_params p{pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh, capacity, 0};
        sam_generate_check(prompts, n_args, n, p); // before the handle: needs no model
        sam_generate_masks_device(as_sam(m), prompts, n_args, n, p, {masks_u8_dev, info_i32_dev, info_f32_dev, counts_dev}, stream);
    });
}

int32_t visp_sam_generate_masks_host(visp_model* m, int32_t const* prompts, int32_t const* n_args, int32_t n, float pred_iou_thresh, float stability_thresh,
                                     float stability_offset, float nms_iou_thresh, int32_t capacity, uint8_t* masks_u8, int32_t* info_i32, float* info_f32,
                                     int32_t* counts) {
    return handle_errors([&]() {
        const sam_select_params p{pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh, capacity, 0};
        sam_generate_check(prompts, n_args, n, p);
        sam_generate_masks_host(as_sam(m), prompts, n_args, n, p, {masks_u8, info_i32, info_f32, counts});
    });
}

int32_t visp_sam_generate_masks_clean_device(visp_model* m, int32_t const* prompts, int32_t const* n_args, int32_t n, float pred_iou_thresh, float stability_thresh,
                                             float stability_offset, float nms_iou_thresh, int32_t capacity, int32_t min_region_area, void* masks_u8_dev,
                                             void* info_i32_dev, void* info_f32_dev, void* counts_dev, void* stream) {
    return handle_errors([&]() {
        const sam_select_params p{pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh, capacity, min_region_area};
        sam_generate_check(prompts, n_args, n, p); // before the handle: needs no model
        sam_generate_masks_device(as_sam(m), prompts, n_args, n, p, {masks_u8_dev, info_i32_dev, info_f32_dev, counts_dev}, stream);
    });
}

int32_t visp_sam_generate_masks_clean_host(visp_model* m, int32_t const* prompts, int32_t const* n_args, int32_t n, float pred_iou_thresh, float stability_thresh,
                                           float stability_offset, float nms_iou_thresh, int32_t capacity, int32_t min_region_area, uint8_t* masks_u8, int32_t* info_i32,
                                           float* info_f32, int32_t* counts) {
    return handle_errors([&]() {
        const sam_select_params p{pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh, capacity, min_region_area};
        sam_generate_check(prompts, n_args, n, p);
        sam_generate_masks_host(as_sam(m), prompts, n_args, n, p, {masks_u8, info_i32, info_f32, counts});
    });
}

// the last generate call's ms of the stages named, in that order (0 for a stage the call did not run)
static void sam_stage_ms(visp_model const* m, float* out_ms, std::initializer_list<sam_generate_stage> stages) {
    if (!out_ms) throw except("sam: null argument");
    for (sam_generate_stage st : stages) *out_ms++ = as_sam(m).generate_split_ms[st];
}

int32_t visp_sam_generate_last_split5(visp_model const* m, float out_ms[5]) {
    return handle_errors([&]() {
        float parts[3];
        sam_stage_ms(m, out_ms, {sam_stage_decode, sam_stage_scoring, sam_stage_rank_nms, sam_stage_output});
        sam_stage_ms(m, parts, {sam_stage_clean, sam_stage_records_nms2, sam_stage_gather});
        out_ms[4] = parts[0] + parts[1] + parts[2];
    });
}

int32_t visp_sam_generate_last_clean_split(visp_model const* m, float out_ms[3]) {
    return handle_errors([&]() { sam_stage_ms(m, out_ms, {sam_stage_clean, sam_stage_records_nms2, sam_stage_gather}); });
}

int32_t visp_sam_generate_last_split(visp_model const* m, float out_ms[4]) {
    return handle_errors([&]() { sam_stage_ms(m, out_ms, {sam_stage_decode, sam_stage_scoring, sam_stage_rank_nms, sam_stage_output}); });
}

int32_t visp_sam_generate_defaults(float out[4]) {
    return handle_errors([&]() {
        if (!out) throw except("sam: null argument");
        out[0] = 0.88f; // SAM's automatic mask generator: pred_iou_thresh, stability_score_thresh, stability_score_offset, box_nms_thresh
        out[1] = 0.95f;
        out[2] = 1.0f;
        out[3] = 0.7f;
    });
}

int32_t visp_sam_image_extent(visp_model* m, int32_t* width, int32_t* height) {
    return handle_errors([&]() {
        sam_model& sm = as_sam(m);
        if (!width || !height) throw except("sam: null argument");
        if (!sm.embed.ptr || sm.image_extent[0] <= 0) throw except("Missing image embeds, call sam_encode() first");
        *width = sm.image_extent[0];
        *height = sm.image_extent[1];
    });
}

int32_t visp_sam_set_prompt_chunk(visp_model* m, int32_t n) {
    return handle_errors([&]() { sam_set_prompt_chunk(as_sam(m), n); });
}

int32_t visp_sam_read_masks_batch(visp_model* m, float* logits, int64_t capacity, float* iou) {
    return handle_errors([&]() {
        sam_kept_logits const& kept = as_sam(m).last_batch;
        if (!logits) throw except("sam: null argument");
        if (kept.masks.empty()) throw except("sam: no mask logits kept: enable captures, then call sam_compute_batch()");
        if (capacity < (int64_t)kept.masks.size()) throw except("sam: mask buffer too small (%lld < %zu)", (long long)capacity, kept.masks.size());
        memcpy(logits, kept.masks.data(), kept.masks.size() * sizeof(float));
        if (iou) memcpy(iou, kept.iou.data(), kept.iou.size() * sizeof(float));
    });
}

int32_t visp_sam_encode_batch_device(visp_model* m, void const* rgb, int32_t batch, void* out, void* stream) {
    return handle_errors([&]() { sam_encode_batch_device(as_sam(m), rgb, batch, out, stream); });
}

int32_t visp_sam_encode_batch_host(visp_model* m, uint8_t const* rgb, int32_t batch, float* out) {
    return handle_errors([&]() { sam_encode_batch_host(as_sam(m), rgb, batch, out); });
}

int32_t visp_sam_set_fp8_mlp(visp_model* m, int32_t enable) {
    return handle_errors([&]() { sam_set_fp8_mlp(as_sam(m), enable != 0); });
}

int32_t visp_sam_enable_captures(visp_model* m, int32_t enable) {
    return handle_errors([&]() { as_sam(m).captures = enable != 0; });
}

int32_t visp_sam_read_capture(visp_model* m, char const* name, float* host_out, int64_t capacity, int64_t* n_written, int64_t shape[4]) {
    return handle_errors([&]() { read_capture(as_sam(m), "sam", name, host_out, capacity, n_written, shape); });
}

int32_t visp_sam_enable_timing(visp_model* m, int32_t enable) {
    return handle_errors([&]() { as_sam(m).timing = enable != 0; });
}

int32_t visp_sam_read_timing(visp_model* m, visp_timing* out, int32_t cap, int32_t* n) {
    return handle_errors([&]() { read_timing(as_sam(m), out, cap, n); });
}

// ---- SWIN encoder (BiRefNet backbone) ----------------------------------------------------------------------------------

int32_t visp_swin_load(char const* filepath, visp_device const* dev, visp_model** out) {
    return handle_errors([&]() {
        if (!filepath || !dev || !out) throw except("visp_swin_load: null argument");
        *out = handle_of(swin_load_model(filepath, *reinterpret_cast<backend_device const*>(dev)));
    });
}

int32_t visp_birefnet_compute_batch_device(visp_model* m, void const* rgb_u8, int32_t batch, int32_t w, int32_t h, void* mask_f32, void* stream) {
    return handle_errors([&]() { birefnet_compute_batch_device(as_birefnet(m), rgb_u8, batch, w, h, mask_f32, stream); });
}

int32_t visp_birefnet_compute_batch_host(visp_model* m, uint8_t const* rgb_u8, int32_t batch, int32_t w, int32_t h, float* mask) {
    return handle_errors([&]() { birefnet_compute_batch_host(as_birefnet(m), rgb_u8, batch, w, h, mask); });
}

int32_t visp_birefnet_cutout_batch_device(visp_model* m, void const* rgb_u8, int32_t batch, int32_t w, int32_t h, int32_t radius, void* rgba_u8_out, void* stream) {
    return handle_errors([&]() { birefnet_cutout_batch_device(as_birefnet(m), rgb_u8, batch, w, h, radius, rgba_u8_out, stream); });
}

int32_t visp_birefnet_cutout_batch_host(visp_model* m, uint8_t const* rgb_u8, int32_t batch, int32_t w, int32_t h, int32_t radius, uint8_t* rgba_u8_out) {
    return handle_errors([&]() { birefnet_cutout_batch_host(as_birefnet(m), rgb_u8, batch, w, h, radius, rgba_u8_out); });
}

int32_t visp_birefnet_cutout(visp_model* m, visp_image_view const* image, int32_t radius, visp_image_view* out_image, visp_image_data** out_data) {
    return handle_errors([&]() {
        if (!image || !out_image || !out_data) throw except("visp_birefnet_cutout: null argument");
        return_image(birefnet_cutout(as_birefnet(m), host_view("visp_birefnet_cutout", image), radius), out_image, out_data);
    });
}

// ---- matting image ops (matting.h): the argument checks run inside the visp:: functions, before their first device call ----

int32_t visp_image_blur(visp_device const* dev, visp_image_view const* src, int32_t radius, visp_image_view* out_image, visp_image_data** out_data) {
    return handle_errors([&]() {
        if (!out_image || !out_data) throw except("visp_image_blur: null argument");
        return_image(image_blur(dev, host_view("visp_image_blur", src), radius), out_image, out_data);
    });
}

int32_t visp_image_remove_small_regions_device(void* masks_u8_dev, int32_t n, int32_t w, int32_t h, int32_t min_area, int32_t mode, void* changed_i32_dev, void* stream,
                                               visp_device const* dev) {
    return handle_errors([&]() {
        if (!masks_u8_dev) throw except("visp_image_remove_small_regions_device: null argument");
        check_remove_small_regions(n, w, h, min_area, mode);
        remove_small_regions_device(dev, masks_u8_dev, n, w, h, min_area, mode, changed_i32_dev, stream);
    });
}

int32_t visp_image_remove_small_regions_host(uint8_t* masks_u8, int32_t n, int32_t w, int32_t h, int32_t min_area, int32_t mode, int32_t* changed_i32, visp_device const* dev) {
    return handle_errors([&]() {
        if (!masks_u8) throw except("visp_image_remove_small_regions_host: null argument");
        check_remove_small_regions(n, w, h, min_area, mode);
        remove_small_regions_host(dev, masks_u8, n, w, h, min_area, mode, changed_i32);
    });
}

int32_t visp_image_erosion(visp_device const* dev, visp_image_view const* src, int32_t radius, visp_image_view* out_image, visp_image_data** out_data) {
    return handle_errors([&]() {
        if (!out_image || !out_data) throw except("visp_image_erosion: null argument");
        return_image(image_erosion(dev, host_view("visp_image_erosion", src), radius), out_image, out_data);
    });
}

int32_t visp_image_estimate_foreground(visp_device const* dev, visp_image_view const* image, visp_image_view const* mask, int32_t radius, visp_image_view* out_image,
                                       visp_image_data** out_data) {
    return handle_errors([&]() {
        if (!out_image || !out_data) throw except("visp_image_estimate_foreground: null argument");
        return_image(image_estimate_foreground(dev, host_view("visp_image_estimate_foreground", image), host_view("visp_image_estimate_foreground", mask), radius), out_image,
                     out_data);
    });
}

int32_t visp_image_alpha_composite(visp_device const* dev, visp_image_view const* fg, visp_image_view const* bg, visp_image_view const* mask, visp_image_view* out_image,
                                   visp_image_data** out_data) {
    return handle_errors([&]() {
        if (!out_image || !out_data) throw except("visp_image_alpha_composite: null argument");
        char const* who = "visp_image_alpha_composite";
        return_image(image_alpha_composite(dev, host_view(who, fg), host_view(who, bg), host_view(who, mask)), out_image, out_data);
    });
}

int32_t visp_image_set_alpha(visp_image_view const* img, visp_image_view const* alpha, visp_image_view* out_image, visp_image_data** out_data) {
    return handle_errors([&]() {
        if (!out_image || !out_data) throw except("visp_image_set_alpha: null argument");
        return_image(image_set_alpha(host_view("visp_image_set_alpha", img), host_view("visp_image_set_alpha", alpha)), out_image, out_data);
    });
}

int32_t visp_image_to_mask(visp_image_view const* src, visp_image_view* out_image, visp_image_data** out_data) {
    return handle_errors([&]() {
        if (!out_image || !out_data) throw except("visp_image_to_mask: null argument");
        return_image(image_to_mask(host_view("visp_image_to_mask", src)), out_image, out_data);
    });
}

int32_t visp_image_estimate_foreground_batch_device(visp_device const* dev, void const* img, int32_t img_format, void const* mask_f32, int32_t batch, int32_t w, int32_t h,
                                                    int32_t radius, void* out, int32_t out_format, void* stream) {
    return handle_errors([&]() {
        if (img_format < 0 || img_format > int32_t(image_format::alpha_f32) || out_format < 0 || out_format > int32_t(image_format::alpha_f32))
            throw except("Unsupported image format [%d]", img_format);
        estimate_foreground_batch_device(dev, img, image_format(img_format), static_cast<float const*>(mask_f32), batch, w, h, radius, out, image_format(out_format), stream);
    });
}

int32_t visp_birefnet_image_extent(visp_model* m, int32_t w, int32_t h, int32_t* out_w, int32_t* out_h) {
    return handle_errors([&]() {
        i32x2 e = birefnet_image_extent({{w, h}}, as_birefnet(m).bparams);
        *out_w = e[0];
        *out_h = e[1];
    });
}

int32_t visp_swin_output_dims(visp_model* m, int32_t w, int32_t h, int32_t dims[12]) {
    return handle_errors([&]() {
        int d[4][3];
        swin_output_dims(as_swin(m), w, h, d);
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 3; ++j) dims[i * 3 + j] = d[i][j];
    });
}

int32_t visp_swin_encode_batch_device(visp_model* m, void const* rgb_u8, int32_t batch, int32_t w, int32_t h, void* const outs[4], void* stream) {
    return handle_errors([&]() { swin_encode_batch_device(as_swin(m), rgb_u8, batch, w, h, outs, stream); });
}

int32_t visp_swin_encode_batch_host(visp_model* m, uint8_t const* rgb_u8, int32_t batch, int32_t w, int32_t h, float* const outs[4]) {
    return handle_errors([&]() { swin_encode_batch_host(as_swin(m), rgb_u8, batch, w, h, outs); });
}

int32_t visp_swin_enable_captures(visp_model* m, int32_t enable) {
    return handle_errors([&]() { as_swin(m).captures = enable != 0; });
}

int32_t visp_swin_read_capture(visp_model* m, char const* name, float* host_out, int64_t capacity, int64_t* n_written, int64_t shape[4]) {
    return handle_errors([&]() { read_capture(as_swin(m), "swin", name, host_out, capacity, n_written, shape); });
}

int32_t visp_swin_set_mask_mode(visp_model* m, int32_t shifted_only) {
    return handle_errors([&]() { as_swin(m).mask_shifted_only = shifted_only != 0; });
}

int32_t visp_swin_enable_timing(visp_model* m, int32_t enable) {
    return handle_errors([&]() { as_swin(m).timing = enable != 0; });
}

int32_t visp_swin_read_timing(visp_model* m, visp_timing* out, int32_t cap, int32_t* n) {
    return handle_errors([&]() { read_timing(as_swin(m), out, cap, n); });
}

// ---- model file: the GGUF key/value surface of the reference's model_file (ml.h:85-103, ml.cpp:206-281) ----

static model_file const& as_file(visp_file const* f) {
    if (!f) throw except("model file handle is null");
    return f->file;
}
int32_t visp_file_load(char const* gguf_path, visp_file** out) {
    return handle_errors([&]() {
        if (!out) throw except("visp_file_load: null out pointer");
        if (!gguf_path) throw except("visp_file_load: null path");
        *out = new visp_file{model_load(gguf_path)};
    });
}
void visp_file_destroy(visp_file* f) { delete f; }
int32_t visp_file_n_tensors(visp_file const* f, int64_t* out) {
    return handle_errors([&]() {
        if (!out) throw except("visp_file_n_tensors: null out pointer");
        *out = as_file(f).n_tensors();
    });
}
int32_t visp_file_get_int(visp_file const* f, char const* key, int32_t* out) {
    return handle_errors([&]() {
        if (!key || !out) throw except("visp_file_get_int: null argument");
        *out = as_file(f).get_int(key);
    });
}
int32_t visp_file_get_int_array(visp_file const* f, char const* key, int32_t* out, int64_t n) {
    return handle_errors([&]() {
        if (!key || !out || n < 0) throw except("visp_file_get_int_array: bad argument");
        as_file(f).get_array(key, out, (size_t)n);
    });
}
int32_t visp_file_get_string(visp_file const* f, char const* key, char* out, int64_t capacity, int64_t* needed) {
    return handle_errors([&]() {
        if (!key) throw except("visp_file_get_string: null key");
        std::string_view v = as_file(f).get_string(key);
        if (needed) *needed = (int64_t)v.size() + 1;
        if (out && capacity > 0) snprintf(out, (size_t)capacity, "%.*s", (int)v.size(), v.data());
    });
}
int32_t visp_weights_from_file(visp_file const* f, visp_weights** out) {
    return handle_errors([&]() {
        if (!out) throw except("visp_weights_from_file: null out pointer");
        *out = new visp_weights{weights_from_file(as_file(f))};
    });
}

// ---- graph layer (graph.h) ----

int32_t visp_weights_load(char const* gguf_path, visp_weights** out) {
    return handle_errors([&]() {
        if (!out) throw except("visp_weights_load: null out pointer");
        *out = new visp_weights{weights_load(gguf_path)};
    });
}
int32_t visp_weights_create(visp_weights** out) {
    return handle_errors([&]() {
        if (!out) throw except("visp_weights_create: null out pointer");
        *out = new visp_weights{weights_create()};
    });
}
int32_t visp_weights_add(visp_weights* w, char const* name, int32_t dtype, int64_t const ne[4], float const* data) {
    return handle_errors([&]() {
        if (!w) throw except("weights handle is null");
        weights_add(*w->store, name, dtype, ne, data);
    });
}
void visp_weights_destroy(visp_weights* w) { delete w; }

int32_t visp_graph_create(visp_weights* weights, visp_graph** out) {
    return handle_errors([&]() {
        if (!out) throw except("visp_graph_create: null out pointer");
        *out = static_cast<visp_graph*>(graph_create(weights ? weights->store : nullptr));
    });
}
void visp_graph_destroy(visp_graph* g) { delete static_cast<graph*>(g); }

static graph& as_graph(visp_graph* g) {
    if (!g) throw except("graph handle is null");
    return *g;
}
static graph const& as_cgraph(visp_graph const* g) {
    if (!g) throw except("graph handle is null");
    return *g;
}

int32_t visp_graph_add_weight(visp_graph* g, char const* name, int32_t dtype, int64_t const ne[4], float const* data, int32_t* out) {
    return handle_errors([&]() {
        const int t = graph_add_weight(as_graph(g), name, dtype, ne, data);
        if (out) *out = t;
    });
}
int32_t visp_graph_find_weight(visp_graph* g, char const* name, int32_t* out) {
    return handle_errors([&]() {
        if (!out) throw except("visp_graph_find_weight: null out pointer");
        *out = graph_find_weight(as_graph(g), name);
    });
}
int32_t visp_graph_input(visp_graph* g, int32_t dtype, int64_t const ne[4], char const* name, int32_t* out) {
    return handle_errors([&]() {
        if (!out || !ne) throw except("visp_graph_input: null pointer");
        *out = graph_input(as_graph(g), dtype, ne, name);
    });
}
int32_t visp_graph_op(visp_graph* g, int32_t op, int32_t const* src, int32_t n_src, int64_t const* iparams, int32_t n_iparams, float const* fparams,
                      int32_t n_fparams, int32_t* out) {
    return handle_errors([&]() {
        if (!out || !src) throw except("visp_graph_op: null pointer");
        *out = graph_add(as_graph(g), op, src, n_src, iparams, n_iparams, fparams, n_fparams);
    });
}
int32_t visp_graph_set_name(visp_graph* g, int32_t tensor, char const* name) {
    return handle_errors([&]() { graph_set_name(as_graph(g), tensor, name); });
}
int32_t visp_graph_get_tensor(visp_graph* g, char const* name, int32_t* out) {
    return handle_errors([&]() {
        if (!out) throw except("visp_graph_get_tensor: null out pointer");
        *out = graph_get_tensor(as_graph(g), name);
    });
}
int32_t visp_graph_output(visp_graph* g, int32_t tensor, char const* name) {
    return handle_errors([&]() { graph_output(as_graph(g), tensor, name); });
}
int32_t visp_graph_tensor_info(visp_graph const* g, int32_t tensor, int32_t* dtype, int64_t ne[4], int32_t* is_constant) {
    return handle_errors([&]() {
        graph const& gr = as_cgraph(g);
        if (tensor < 0 || tensor >= (int)gr.nodes.size()) throw except("visp_graph_tensor_info: tensor handle %d is not part of this graph", tensor);
        graph_node const& n = gr.nodes[tensor];
        if (dtype) *dtype = n.dtype;
        if (ne) for (int i = 0; i < 4; ++i) ne[i] = n.ne[i];
        if (is_constant) *is_constant = n.constant;
    });
}
int32_t visp_graph_read_constant(visp_graph const* g, int32_t tensor, float* out, int64_t capacity) {
    return handle_errors([&]() {
        graph const& gr = as_cgraph(g);
        if (tensor < 0 || tensor >= (int)gr.nodes.size()) throw except("visp_graph_read_constant: tensor handle %d is not part of this graph", tensor);
        graph_node const& n = gr.nodes[tensor];
        if (!out) throw except("visp_graph_read_constant: null out pointer");
        if (!n.constant) throw except("visp_graph_read_constant: tensor %d is not a constant", tensor);
        if (capacity < n.n_elements()) throw except("visp_graph_read_constant: capacity %lld < %lld elements", (long long)capacity, (long long)n.n_elements());
        memcpy(out, n.values(), (size_t)n.n_elements() * 4);
    });
}
int32_t visp_graph_allocate(visp_graph* g, visp_device const* dev) {
    return handle_errors([&]() { graph_allocate(as_graph(g), dev); });
}
int32_t visp_graph_use_hip_graph(visp_graph* g, int32_t enable) {
    return handle_errors([&]() { as_graph(g).use_hip_graph = enable != 0; });
}
int32_t visp_graph_set_fused_models(visp_graph* g, int32_t enable) {
    return handle_errors([&]() {
        graph& gr = as_graph(g);
        if (gr.allocated) throw except("visp_graph_set_fused_models: the graph is already allocated");
        gr.fused_models = enable != 0;
    });
}
int32_t visp_graph_compute(visp_graph* g) {
    return handle_errors([&]() { graph_compute(as_graph(g)); });
}
int32_t visp_graph_tensor_set(visp_graph* g, int32_t tensor, void const* data, size_t n_bytes) {
    return handle_errors([&]() { graph_tensor_set(as_graph(g), tensor, data, n_bytes); });
}
int32_t visp_graph_tensor_get(visp_graph* g, int32_t tensor, void* data, size_t n_bytes, int32_t as_f32) {
    return handle_errors([&]() { graph_tensor_get(as_graph(g), tensor, data, n_bytes, as_f32 != 0); });
}
int32_t visp_graph_describe(visp_graph const* g, char* out, int64_t capacity, int64_t* needed) {
    return handle_errors([&]() {
        std::string s = graph_describe(as_cgraph(g));
        if (needed) *needed = (int64_t)s.size() + 1;
        if (out && capacity > 0) snprintf(out, (size_t)capacity, "%s", s.c_str());
    });
}

} // extern "C"
