#include "model.h"

#include <cstring>

#include "visp_util.h"

namespace visp {

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
// device memory and captured graphs

device_buffer::device_buffer(size_t n) : bytes(n) { VX(vx_malloc(&ptr, n)); }
device_buffer& device_buffer::operator=(device_buffer&& o) noexcept {
    if (this != &o) {
        vx_free(ptr);
        ptr = o.ptr;
        bytes = o.bytes;
        o.ptr = nullptr;
        o.bytes = 0;
    }
    return *this;
}
device_buffer::~device_buffer() { vx_free(ptr); }

bool grow(device_buffer& b, size_t need, std::initializer_list<void*> syncs, void* zero_on) {
    if (b.bytes >= need) return false;
    for (void* s : syncs)
        if (s) VX(vx_stream_sync(s));
    b = {};
    b = device_buffer(need);
    if (zero_on) VX(vx_memset(b.ptr, 0, need, zero_on));
    return true;
}

device_buffer upload_arena(std::vector<uint8_t> const& image, void* stream, bool copy) {
    device_buffer b(round_up<size_t>(image.size(), 256) + 4096);
    if (copy) {
        VX(vx_memcpy_h2d(b.ptr, image.data(), image.size(), stream));
        VX(vx_stream_sync(stream));
    }
    return b;
}

captured_graph& captured_graph::operator=(captured_graph&& o) noexcept {
    if (this != &o) {
        vx_graph_destroy(exec);
        exec = o.exec;
        o.exec = nullptr;
    }
    return *this;
}
captured_graph::~captured_graph() { vx_graph_destroy(exec); }
void captured_graph::launch(void* stream) const { VX(vx_graph_launch(exec, stream)); }

captured_graph capture(void* stream, std::function<void()> const& record) {
    captured_graph g;
    VX(vx_graph_begin_capture(stream));
    try {
        record();
    } catch (...) {
        vx_graph_end_capture(stream, &g.exec); // (g drops what a partial capture instantiated)
        throw;
    }
    VX(vx_graph_end_capture(stream, &g.exec));
    return g;
}

vx_gemm_args gemm_args(packed_gemm const& g, const uint8_t* arena) {
    vx_gemm_args a;
    memset(&a, 0, sizeof a);
    a.W = arena + g.w;
    a.bias = g.b == SIZE_MAX ? nullptr : reinterpret_cast<const float*>(arena + g.b);
    a.N = g.N;
    a.K = g.K;
    a.n_valid = g.n_real;
    return a;
}

size_t workspace_layout::take(size_t bytes, size_t slack) {
    const size_t o = top;
    top = round_up<size_t>(top + bytes + slack, 256);
    return o;
}

//
// instrumentation

model_base::~model_base() {
    if (backend) vx_set_device(backend->index);
}

void model_base::keep_capture(std::string const& name, void const* src, int64_t const (&shape)[4], bool f16, void* stream) {
    capture_entry& c = capture_bufs[name];
    c.dev = {};
    const size_t bytes = (size_t)(shape[0] * shape[1] * shape[2] * shape[3]) * (f16 ? 2 : 4);
    c.dev = device_buffer(bytes);
    memcpy(c.shape, shape, sizeof c.shape);
    c.f16 = f16;
    VX(vx_memcpy_d2d(c.dev.ptr, src, bytes, stream));
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
