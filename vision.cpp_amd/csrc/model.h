// What every model family of the MI355X backend shares: the device and its turn, the handle base with the per-group timing and
// the captured intermediate maps of the last pass, and the small weight / buffer records the loaders pack. Host C++ only; all
// device work goes through the vx_* C ABI (include/visp_hip_kernels.h).
#pragma once
#include <cstdint>
#include <functional>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/visp_hip_kernels.h"

namespace visp {

enum class backend_type : int32_t { cpu = 1, gpu = 2, vulkan = 2 | 1 << 8 }; // include/visp/ml.h:32-36

struct backend_device { // include/visp/ml.h:44-55, here: one HIP device + its compute stream
    int index = 0;
    std::string name, description;
    void* stream = nullptr;
    size_t total_mem = 0;
    int n_cu = 0;
    backend_type type() const { return backend_type::gpu; }
    // Every model and graph made on this device shares `stream`. Whatever enqueues on it, captures a hipGraph on it or synchronises it
    // holds the device's turn (device_turn below), so that host threads driving different models of one device cannot interleave a
    // capture with another thread's launches ("capturing stream has unjoined work"). Recursive: entry points nest.
    mutable std::recursive_mutex turn;
    ~backend_device();
};
// makes the device current for the calling thread and holds its turn for the scope
struct device_turn {
    std::unique_lock<std::recursive_mutex> lock;
    explicit device_turn(backend_device const& dev);
};
backend_device* backend_init(int device_index); // throws visp::exception if no gfx950 device

// One GEMM-shaped weight in a packed arena: f16 [N][K] (both padded for the kernel's tiles, pads are zero) + optional f32 bias [N]
// (the model loaders that pack for hand schedules: tinyvit.cpp, swin.cpp, birefnet.cpp)
struct packed_gemm {
    size_t w = 0, b = SIZE_MAX; // byte offsets into the arena
    int N = 0, K = 0;           // padded
    int n_real = 0, k_real = 0; // for FLOP accounting and n_valid
};
struct packed_vec { size_t off = SIZE_MAX; int n = 0; }; // f32 vector
// a zeroed GEMM argument block with what the pack decides: W, bias (null without one), the padded N and K, n_valid = n_real
vx_gemm_args gemm_args(packed_gemm const& g, const uint8_t* arena);

// offsets of one workspace, bumped: every offset starts 256-aligned; slack: bytes left free behind the block
struct workspace_layout {
    size_t top = 0;
    size_t take(size_t bytes, size_t slack = 0);
};
// The slots of one workspace, each written once: add() lays a slot out as take() does and returns it, and the slot reads as its address from when `base`
// is set (after the grow to layout.top). A slot that is not added (when = false) takes no room and reads as null. Slots point back at their table: do not copy or move it.
struct workspace_table {
    workspace_layout layout;
    uint8_t* base = nullptr;
    template <class T> struct slot {
        workspace_table const* table; size_t off;
        operator T*() const { return table ? static_cast<T*>(static_cast<void*>(table->base + off)) : nullptr; }
    };
    template <class T = void> slot<T> add(size_t bytes, size_t slack = 0, bool when = true) {
        return when ? slot<T>{this, layout.take(bytes, slack)} : slot<T>{nullptr, 0};
    }
};

// Device memory with one owner: freed by the destructor, moved but never copied. Kernel arguments and the weight store's packs
// keep raw pointers into it.
struct device_buffer {
    void* ptr = nullptr;
    size_t bytes = 0;
    device_buffer() = default;
    explicit device_buffer(size_t n); // throws visp::exception
    device_buffer(device_buffer&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
    device_buffer& operator=(device_buffer&& o) noexcept; // frees what this one held first
    ~device_buffer();
};
// a view of device memory another object owns (the weight store's arena)
struct device_span { void* ptr = nullptr; size_t bytes = 0; };

// Makes b hold at least `need` bytes. When it is smaller: synchronises the non-null streams of `syncs` (the work that may still
// use it), frees it, allocates `need` bytes and zero-fills them on `zero_on` if that is not null. Returns whether b moved: a
// hipGraph captured over it is stale then.
bool grow(device_buffer& b, size_t need, std::initializer_list<void*> syncs, void* zero_on = nullptr);
// the device copy of a packed host arena: round_up(size, 256) + 4096 bytes, uploaded on stream, which is then synchronised;
// copy = false only allocates (the data comes later: a broadcast from the rank that read the file)
device_buffer upload_arena(std::vector<uint8_t> const& image, void* stream, bool copy = true);

// A captured hipGraph exec with one owner: destroyed by the destructor, moved but never copied.
struct captured_graph {
    void* exec = nullptr;
    captured_graph() = default;
    captured_graph(captured_graph&& o) noexcept : exec(o.exec) { o.exec = nullptr; }
    captured_graph& operator=(captured_graph&& o) noexcept; // destroys what this one held first
    ~captured_graph();
    explicit operator bool() const { return exec != nullptr; }
    void launch(void* stream) const;
};
// the launches `record` enqueues on stream, captured and instantiated; if it throws, the partial capture is ended and dropped
captured_graph capture(void* stream, std::function<void()> const& record);

struct capture_entry { device_buffer dev; int64_t shape[4] = {1, 1, 1, 1}; bool f16 = true; };

struct timing_entry { std::string name; float ms = 0; int launches = 0; double flops = 0, bytes = 0; };
// adds t to the row of its name, or appends it as a new row: a table keeps its rows in first-seen order
void timing_add(std::vector<timing_entry>& rows, timing_entry const& t);

// every model handle starts with its family (the C ABI's handles are untyped: c-api.cpp:193 any_model)
enum model_family_id : int32_t { family_sam = 0, family_birefnet, family_depth_anything, family_migan, family_esrgan, family_count };
// families outside the public visp_model_family range: the generic entry points (visp_model_compute, ..) refuse their handles
constexpr int32_t family_yolov9t = 64;
struct model_base {
    int32_t family;
    backend_device const* backend = nullptr;
    bool captures = false, timing = false;
    bool use_graph = true; // replay captured launch lists (MI-GAN, YOLOv9t, Depth-Anything's device entry)
    std::map<std::string, capture_entry> capture_bufs; // named intermediate maps of the last pass with captures on (the parity tests)
    std::vector<timing_entry> last_timing;             // per kernel group, of the last pass with timing on
    explicit model_base(int32_t f) : family(f) {}
    model_base(model_base const&) = delete;
    model_base& operator=(model_base const&) = delete;
    virtual ~model_base(); // the capture buffers are freed on the model's device
    // a device copy of the contiguous map at src (shape[0] * .. * shape[3] f16 or f32 elements), enqueued on stream, as capture `name`
    void keep_capture(std::string const& name, void const* src, int64_t const (&shape)[4], bool f16, void* stream);
    bool replays() const { return use_graph && !timing && !captures; } // timing and captures need the eager launches
};

// per-kernel-group timing of one pass on one stream: an event in front of every launch, summed per group name by finish()
struct timing_marks {
    std::vector<void*> events;           // events[i] is recorded in front of launches[i]
    std::vector<timing_entry> launches;
    timing_marks() = default;
    timing_marks(timing_marks const&) = delete; // owns its events
    timing_marks& operator=(timing_marks const&) = delete;
    void mark(const char* name, double flops, double bytes, void* stream);
    // out = the marked groups (append: added to the rows out already holds); the events are released
    void finish(void* stream, std::vector<timing_entry>& out, bool append = false);
    void release();
    ~timing_marks() { release(); }
};

// the launch list `run` enqueues on stream, replayed from graphs[key] when the model replays and holds a capture of key; otherwise run
// eagerly (the first call of a key also warms every kernel up) and, when the model replays, captured into graphs[key] by a second run
template <typename Key>
void replay_or_run(model_base const& m, std::map<Key, captured_graph>& graphs, Key const& key, void* stream, std::function<void()> const& run) {
    auto it = graphs.find(key);
    if (m.replays() && it != graphs.end()) return it->second.launch(stream);
    run();
    if (m.replays()) graphs[key] = capture(stream, run);
}

// One pass of a family's launch list on one stream (Model: the family's model). Its timing marks and captures record only when the model
// asks for them and the pass is not a dry one (a sizing pass: the family launches nothing either).
template <typename Model>
struct model_pass {
    Model& m;
    void* stream;
    const uint8_t* wa; // the model's weight arena
    bool dry = false;
    timing_marks tm;

    model_pass(Model& model, void* s, const void* arena, bool d = false) : m(model), stream(s), wa(static_cast<const uint8_t*>(arena)), dry(d) {}
    void mark(const char* group, double flops, double bytes) { if (m.timing && !dry) tm.mark(group, flops, bytes, stream); }
    void keep(std::string const& name, const void* src, int64_t const (&shape)[4], bool f16 = true) {
        if (m.captures && !dry) m.keep_capture(name, src, shape, f16, stream);
    }
    // the marked groups into out (append: added to its rows); false when the pass does not time
    bool finish_timing(std::vector<timing_entry>& out, bool append = false) {
        if (!m.timing || dry) return false;
        tm.finish(stream, out, append);
        return true;
    }
    void finish_timing() { finish_timing(m.last_timing); }
    const float* vec(packed_vec const& v) const { return reinterpret_cast<const float*>(wa + v.off); }
};

enum load_flags { load_default = 0, load_no_upload = 1 };

} // namespace visp
