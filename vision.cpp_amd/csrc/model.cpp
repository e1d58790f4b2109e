#include "model.h"

#include <cstring>

#include "../../include/visp_hip_kernels.h"
#include "visp_util.h"

namespace visp {

#define VX(call)                                        \
    do {                                                \
        if (!(call)) throw except("%s", vx_last_error()); \
    } while (0)

//
// backend (reference src/visp/ml.cpp:59-95)

device_turn::device_turn(backend_device const& dev) : lock(dev.turn) { VX(vx_set_device(dev.index)); }

backend_device* backend_init(int device_index) {
    int n = vx_device_count();
    if (n <= 0) throw except("Failed to initialize backend, no suitable device available");
    if (device_index < 0 || device_index >= n) throw except("Failed to initialize backend, device index %d out of range (%d devices)", device_index, n);
    VX(vx_set_device(device_index));
    char name[256] = {0}, arch[128] = {0};
    size_t total = 0;
    int n_cu = 0;
    VX(vx_device_info(device_index, name, sizeof name, arch, sizeof arch, &total, nullptr, &n_cu));
    if (strncmp(arch, "gfx950", 6) != 0)
        throw except("Failed to initialize backend: device %d is %s, this backend is built for gfx950 (MI355X) only", device_index, arch);
    auto* d = new backend_device;
    d->index = device_index;
    d->name = std::string("HIP") + std::to_string(device_index);
    d->description = std::string(name) + " (" + arch + ")";
    d->total_mem = total;
    d->n_cu = n_cu;
    VX(vx_stream_create(&d->stream));
    return d;
}
backend_device::~backend_device() {
    if (stream) vx_stream_destroy(stream);
}

//
// instrumentation

model_base::~model_base() {
    if (backend) vx_set_device(backend->index);
    for (auto& c : capture_bufs) vx_free(c.second.dev);
}

void model_base::keep_capture(std::string const& name, void const* src, int64_t const (&shape)[4], bool f16, void* stream) {
    capture_entry& c = capture_bufs[name];
    vx_free(c.dev);
    c.dev = nullptr;
    const size_t bytes = (size_t)(shape[0] * shape[1] * shape[2] * shape[3]) * (f16 ? 2 : 4);
    VX(vx_malloc(&c.dev, bytes));
    memcpy(c.shape, shape, sizeof c.shape);
    c.f16 = f16;
    VX(vx_memcpy_d2d(c.dev, src, bytes, stream));
}

void timing_add(std::vector<timing_entry>& rows, timing_entry const& t) {
    for (timing_entry& r : rows)
        if (r.name == t.name) {
            r.ms += t.ms;
            r.launches += t.launches;
            r.flops += t.flops;
            r.bytes += t.bytes;
            return;
        }
    rows.push_back(t);
}

void timing_marks::mark(const char* name, double flops, double bytes, void* stream) {
    void* ev = nullptr;
    VX(vx_event_create(&ev));
    events.push_back(ev);
    VX(vx_event_record(ev, stream));
    launches.push_back({name, 0, 1, flops, bytes});
}

void timing_marks::finish(void* stream, std::vector<timing_entry>& out, bool append) {
    mark("end", 0, 0, stream); // closes the last launch: never a row
    if (!append) out.clear();
    for (size_t i = 0; i + 1 < events.size(); ++i) {
        timing_entry t = launches[i];
        VX(vx_event_elapsed_ms(events[i], events[i + 1], &t.ms));
        timing_add(out, t);
    }
    release();
}

void timing_marks::release() {
    for (void* ev : events) vx_event_destroy(ev);
    events.clear();
    launches.clear();
}

} // namespace visp
