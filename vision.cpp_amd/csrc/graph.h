// Tensor graph + executor: the layer the reference's arch code is written against (include/visp/ml.h:154-256 compute_graph,
// model_ref, compute_graph_input/output, transfer_*; src/visp/ml.cpp:531-741, 746-788; src/visp/nn.h), rebuilt for the MI355X
// backend. The reference delegates this layer to ggml (graph container, ggml_gallocr liveness allocator, one backend kernel per
// node). Here a graph is a list of nn-level nodes (linear, layer_norm, conv_2d, conv_transpose_2d, attention, interpolate, the
// element-wise glue, slice / concat / repeat / reshape) that `graph_allocate` lowers ONCE into a launch list on the fused kernel
// families of this library:
//   * activation / residual / ReLU-on-load fusion by use count (linear -> gelu, conv -> relu, relu -> conv, conv -> add become
//     GEMM epilogues and loader flags: what ggml runs as 2-4 nodes and HBM round trips is one launch),
//   * constant folding on the host of everything computed from weights alone (the bicubic position-embedding resize, the
//     repeated cls token: dino.cpp:10-44),
//   * weights packed per consumer role (f16 [N][K pad 64] GEMM operand, pixel-shuffle row order for conv_transpose, f32 vectors),
//   * a liveness-based arena in HBM (a buffer is recycled after its last reader), the whole launch list optionally captured
//     into one hipGraph.
// Tensors follow ggml's conventions at the API: ne[0] is the contiguous dimension, activations of 2D ops are CWHN
// ([C, W, H, N] = NHWC in memory, model_build_flag::cwhn), linear weights are [in, out], conv weights [Cin, kw, kh, Cout],
// conv_transpose weights [kw, kh, Cout, Cin]. Activations are f16 in HBM (f32 accumulation inside the kernels), vectors f32.
#pragma once
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "model.h"
#include "gguf.h"

namespace visp {

enum graph_op : int32_t {
    gop_input = 0,
    gop_weight,
    gop_linear,           // x, w [K, N], (b)                         nn.cpp:6-12
    gop_layer_norm,       // x, w, b; f0 = eps                         nn.cpp:14-19
    gop_gelu,             // ggml_gelu                                 dino.cpp:54
    gop_relu,             // ggml_relu
    gop_scale,            // f0 = factor                               depth-anything.cpp:93-95
    gop_add,              // a + b, b broadcast over trailing dims     ggml_add
    gop_mul,              // a * b, same broadcast                     dino.cpp:48-50
    gop_conv_2d,          // x CWHN, w [Cin, kw, kh, Cout], (b); i0 = stride, i1 = pad       nn.cpp:72-100
    gop_conv_transpose_2d,// x CWHN, w [kw, kh, Cout, Cin], (b); i0 = stride (== kernel)      nn.cpp:117-129
    gop_interpolate,      // x CWHN; i0 = w, i1 = h, i2 = mode (ggml: 1 bilinear, 2 bicubic, | 256 align_corners)  ml.cpp:782-788
    gop_attention,        // q, k, v [hd, heads, T, B]; f0 = scale -> [hd * heads, T, B]         nn.cpp:210-244 (without the output linear)
    gop_concat,           // a, b; i0 = dim                            ml.cpp:770-780
    gop_slice,            // x; i[3d..3d+2] = begin, end, step         ml.cpp:746-768
    gop_reshape,          // x; i0..i3 = ne (a view)
    gop_repeat,           // x; i0..i3 = ne (source dims 1 or equal; a constant source may be tiled: folded)   dino.cpp:38-40, sam3.h:331-334
    gop_patch_embed,      // x f32 [C, W, H, N], w conv weight, (b); i0 = patch size            nn.cpp:166-180
    gop_cont,             // a view: every tensor of this executor is contiguous
    // extensions for callers that keep images in HBM (the batched entries of this library); the reference does both steps on the host
    gop_image_u8_to_f32,  // x u8 [3, W, H, N] -> f32: (x / 255 - f0..f2) * f3..f5     image.cpp:215-255 as depthany_process_input calls it
    gop_image_normalize,  // x f32 [1, W, H, N] -> f32: per-image min-max to [0, 1]     image.cpp:537-582 (depthany_process_output)
    gop_leaky_relu,       // f0 = negative slope                         ggml_leaky_relu (esrgan.cpp:17, 24)
    // the window ops of a SWIN block (swin.cpp:48-141) and the masked attention behind them
    gop_permute,          // x; i0..i3 = ggml_permute's axes: source dimension d becomes dimension i_d; the result is contiguous (cont behind it: a view)
    gop_roll,             // x; i0..i3 = cyclic shifts (negative allowed)  ggml_roll (swin.cpp:116, 124)
    gop_pad,              // x; i0..i3 = zeros appended per dimension       ggml_pad (swin.cpp:111)
    gop_get_rows,         // table [C, rows] constant, idx i32: a constant -> f32 (folded); a graph input -> f16 activation [C, idx.ne0, idx.ne1, idx.ne2]   swin.cpp:75, sam3.h:225
    gop_cast,             // x; i0 = type (0 f32, 1 f16): a view on activations of that type, a rounding on constants           swin.cpp:78
    gop_attention_masked, // q, k, v [hd, heads, T, B], mask [T_k, T_q, Hm, Bm]; f0 = scale; hd 32 / 64 -> [hd * heads, T, B]   nn.cpp:210-244 with a mask
    // the nodes of a BiRefNet decoder block (birefnet.cpp:79-145)
    gop_conv_2d_deform,   // x CWHN, w [Cin, k, k, Cout], offset [2 k k, OW, OH, N], (mask [k k, OW, OH, N]); i0 = stride (1), i1 = pad   nn.cpp:131-148
    gop_sigmoid,          // ggml_sigmoid                              birefnet.cpp:86
    gop_mean_2d,          // x [C, W, H, N] -> [C, 1, 1, N]: the pixel mean, f32 sums in a fixed order   birefnet.cpp:93-100
    // the one nn.h function TinyViT (mobile-sam.cpp:15-208) and MI-GAN (migan.cpp:28-57) need beyond the above
    gop_conv_2d_depthwise,// x CWHN, w [C, 1, kw, kh] or [1, kw, kh, C], (b [C]); i0 = stride (1 | 2), i1 = pad   nn.cpp:102-115
    // the ggml calls of YOLOv9t beyond nn.h (yolov9t.cpp:124, 171-177, 461, 644, 681, 687)
    gop_silu,             // ggml_silu
    gop_pool_2d,          // x CWHN; i0 = kind (0 max, 1 avg), i1 i2 = kernel, i3 i4 = stride, i5 i6 = pad   ggml_pool_2d
    gop_soft_max,         // over ne[0], the row maximum subtracted           ggml_soft_max
    gop_sum_rows,         // [n, a, b, c] -> [1, a, b, c]                      ggml_sum_rows
    gop_sub,              // a - b, b broadcast as for add                     ggml_sub
    // MI-GAN's node beyond the above (migan.cpp:23); add / mul / sub also take a plane [1, W, H, 1] on [C, W, H, N] (migan.cpp:40, 76)
    gop_clamp,            // f0 = lower, f1 = upper bound: min(max(x, f0), f1)   ggml_clamp
    // the nodes of the SAM prompt encoder and mask decoder beyond the above (mobile-sam.cpp:238-248, 307-319, 471)
    gop_attention_cross,  // q [hd, heads, T_q, B], k, v [hd, heads, T_k, B]; f0 = scale; hd 16 / 32 / 64, any T_q, T_k -> [hd * heads, T_q, B]   nn.cpp:210-244 without a mask
    gop_mul_mat,          // a [K, M, Ba], b [K, N, B] -> [M, N, B], Ba 1 or B     ggml_mul_mat
    gop_sin,              // ggml_sin
    gop_cos,              // ggml_cos
    // the node of the SAM3 vision encoder beyond the above (sam3.h:413-438)
    gop_rope,             // x [n, heads, T, B] f16, pos i32 constant [T]; i0 = n_dims (== n), i1 = mode (0: NORMAL); f0 = freq_base, f1 = freq_scale   ggml_rope_ext
    // the node of BiRefNet's decoder beyond the above (birefnet.cpp:153-162); interpolate also takes an f32 image [C <= 4, W, H, N] (birefnet.cpp:36-41)
    gop_image_patches,    // f32 image [C <= 4, W, H, N]; i0 = w, i1 = h -> f16 [gw gh C, w, h, N], channel gx + gw (gy + gh c)   image_to_patches
    gop_count
};
const char* graph_op_name(int32_t op);

constexpr int32_t gdt_f32 = 0, gdt_f16 = 1, gdt_u8 = 24, gdt_i32 = 26; // ggml type ids (24 = I8: one byte per element; image inputs. 26 = I32: index constants, held as exact floats on the host)

struct graph_node {
    int32_t op = gop_input;
    int32_t dtype = gdt_f16;
    int64_t ne[4] = {1, 1, 1, 1};
    int src[4] = {-1, -1, -1, -1};
    int n_src = 0;
    int64_t ip[12] = {0};
    float fp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::string name;
    bool is_output = false;
    bool constant = false;        // a weight, or computed from weights alone: evaluated on the host when the node is made
    std::vector<float> host;      // folded constants: the values
    const float* cdata = nullptr; // weights: the values live in the weight store
    const float* values() const { return cdata ? cdata : host.data(); }
    // filled by graph_allocate
    int alias_of = -1;            // shares the buffer of that node (views, fused activations)
    int buffer = -1;              // index into graph::buffers (materialised nodes)
    int64_t n_elements() const { return ne[0] * ne[1] * ne[2] * ne[3]; }
    size_t n_bytes() const { return (size_t)n_elements() * (dtype == gdt_f16 ? 2 : (dtype == gdt_u8 ? 1 : 4)); }
};

struct graph_buffer {
    size_t bytes = 0, offset = 0;
    int first = 0, last = 0; // launch indices of the first writer and the last reader
    bool persistent = false; // inputs and outputs
    void* external = nullptr; // graph_bind_external: an input / output that lives in the caller's memory instead of the arena
};

struct graph_launch {
    std::string desc; // e.g. "gemm[gelu] M=43840 N=1536 K=384 <- layer0.mlp.fc1": what tests and `describe` show
    std::function<void(void* stream)> run;
    std::string group; // timing group (per-group HIP-event times of the model entries: "block", "attention", "fusion_rcu", ...)
    double flops = 0, bytes = 0; // algorithmic work of the launch (2 x MACs; operand bytes), for the roofline lines
};

// Which device image of a weight a (name, role) key of weight_store::packs holds. The numbers are part of the store's keys: two
// kinds that shared one would silently alias two different images of a weight, so a new kind gets a new number.
enum pack_role : int {
    role_f32 = 0,            // the values as they are, f32 (vectors, position embeddings, the one-channel head's kernel)
    role_f16 = 1,            // the values as f16 (constants a copy launch concatenates into activations)
    role_rows = 2,           // GEMM operand: f16 rows [N pad][K pad 64] of a linear / conv weight
    role_conv_transpose = 3, // GEMM operand of conv_transpose: rows in pixel-shuffle order
    role_qkv = 4,            // q | k | v rows of three linears as one operand (keyed on q's weight)
    role_head_frag = 5,      // the DPT head's 3x3 kernel as the head kernel's MFMA fragments
    role_dconv = 6,          // LDS-ring conv slabs [cin / 32][9][cout][32]
    role_rcu = 7,            // residual-unit kernel operand [taps][64][64], swizzled
    role_dconv_ex = 8,       // LDS-ring conv slabs with repeated input columns / padded outputs
    role_bias_padded = 9,    // f32 bias zero-padded to a kernel's channel count
    role_deform = 10,        // deformable conv operand: f16 rows [Cout pad 32][taps * Cin]
    role_deform_offsets = 11,// offset | modulator kernels of a deformable conv as one GEMM operand (keyed on the offset kernel)
    role_deform_offsets_bias = 12, // ... and their biases, f32 [N pad]
    role_depthwise = 13,     // depthwise conv operand: f16 [k * k][C], tap-major, from either stored form
    role_image8 = 14,        // GEMM operand of a conv on a 3-channel f32 image read as 8-channel value | residue pixels: taps 0..2 repeated on 3..5
    role_winattn_bias = 15,  // attention bias [T, T, heads, 1] in the window-attention kernel's accumulator order (vx_window_attention_pack_bias)
    role_bias_base = 16,     // 16..24: bias_of_role(r), the f32 bias [N pad] that goes with the operand of role r (0..8); 30: that of role_image8
    role_block_mlp = 40,     // block kernel: out-proj | fc1 | fc2 fragments, LayerScale folded (keyed on the out-proj weight)
    role_block_qkv = 41,     // block kernel: q | k | v fragments
    role_block_mlp_vec = 42, // block kernel: biases, lambdas and LN2 of the MLP half as one f32 vector
    role_block_qkv_vec = 43, // block kernel: LN1 and the q | k | v biases as one f32 vector
    role_tap_vec = 44,       // block kernel: the taps' final LayerNorm weight | bias
    role_rep_conv = 45,      // GEMM operand of a RepConv: the 3x3 kernel with the 1x1 kernel added into its centre tap (keyed on the 3x3 kernel)
    role_rep_conv_bias = 46, // ... and the two biases summed in f32, [N pad]
    role_plane_f32 = 47,     // a [1, W, H, 1] constant as the f32 plane a fused epilogue adds per pixel (MI-GAN's folded noise)
    role_fourier = 48,       // the [2, F] gaussian matrix of position_embedding_random, rounded to f16, as f32 pairs [F][2]
    role_rope_table = 49,    // i32 positions [T] -> f32 [T][n]: cos | sin of pos * scale * base^(-2 i / n), computed in double (keyed with n, base, scale)
};
// the second form of broadcast add / mul / sub admit next to the trailing-dimension one: b [1, W, H, 1] on a [C, W, H, N], one value per pixel for every
// channel and image (ggml_mul_inplace(x, filter), ggml_add_inplace(x, noise): migan.cpp:40, 76). Where C == 1 or W H == 1 the trailing rule holds already.
inline bool plane_broadcast(const int64_t a[4], const int64_t b[4]) {
    return b[0] == 1 && b[3] == 1 && b[1] == a[1] && b[2] == a[2] && a[0] > 1 && b[1] * b[2] > 1;
}

constexpr pack_role bias_of_role(pack_role r) { return static_cast<pack_role>(role_bias_base + r); }
static_assert(bias_of_role(role_rows) == 18 && bias_of_role(role_qkv) == 20 && bias_of_role(role_dconv_ex) == 24 && role_bias_padded < role_bias_base,
              "16..24 are reserved for the biases of roles 0..8");

// model_weights (ml.h:126-149): the tensors of a model by name, f32 on the host, and -- once a graph over them has been allocated on a
// device -- their packed device images per consumer role (GEMM operand, pixel-shuffle rows, f32 vector, ...). Shared by every graph built
// over the model: rebuilding the graph for another input extent (the reference's lazy graph build, vision.cpp:150-158) uploads nothing.
struct weight_store {
    struct entry {
        int32_t dtype = gdt_f16;
        int64_t ne[4] = {1, 1, 1, 1};
        std::vector<float> data;
    };
    std::map<std::string, entry, std::less<>> tensors;
    backend_device const* dev = nullptr;                    // bound by the first graph_allocate with a device
    std::map<std::pair<std::string, int>, void*> packs;     // (name, role) -> device image
    std::vector<device_buffer> allocs;
    size_t device_bytes = 0;
    // One device arena for every image (optional; depthany's loader sizes it from a planning pass): images are then bump-allocated in
    // lowering order, which is the same on every rank -- the arena IS the model on the device, one RCCL broadcast moves it. no_data: the
    // tensors came from a header-only read (zeros on the host): images are laid out but not uploaded (the broadcast fills them).
    device_buffer arena;
    size_t arena_used = 0;
    bool no_data = false;
    std::mutex mutex;                                       // guards dev / packs / allocs / device_bytes
    ~weight_store();
};
std::shared_ptr<weight_store> weights_create();
// all f16 / f32 tensors of a GGUF file (conv kernels listed in <arch>.conv2d_weights of a whcn file are presented as CWHN)
std::shared_ptr<weight_store> weights_load(char const* gguf_path);
std::shared_ptr<weight_store> weights_from_file(model_file const& file); // model_transfer (ml.cpp:449-516) from a file already read
void weights_add(weight_store&, char const* name, int32_t dtype, const int64_t ne[4], const float* data);

struct graph {
    backend_device const* dev = nullptr; // null: build / fold / plan only (no device work; the CPU tests)
    std::shared_ptr<weight_store> store;
    std::vector<graph_node> nodes;
    std::map<std::string, int, std::less<>> weights; // name -> node (made when first looked up)
    std::map<std::string, int, std::less<>> named;   // graph_set_name, inputs, outputs

    bool allocated = false;
    std::vector<graph_buffer> buffers;
    std::vector<graph_launch> launches;
    size_t arena_bytes = 0, sum_bytes = 0; // with recycling / if every buffer had its own storage
    size_t plan_store_bytes = 0;           // planning only (no device): bytes of weight images this graph would add to the shared store
    device_buffer arena;
    std::vector<device_buffer> const_allocs; // packed weights and constants (device)
    size_t const_bytes = 0;
    bool use_hip_graph = false;
    captured_graph graph_exec; // (after the buffers: destroyed before them)
    // fused_models: the lowering may replace whole node groups by the kernels written for them (the dino::layer group -> attention + one
    // token-stationary block launch with an f32 residual stream, interpolate -> conv 3x3 -> the resizing halo loader, ...). false: one
    // launch per (epilogue-fused) node on f16 activations -- what visp_depthany_set_schedule(model, 0) selects.
    bool fused_models = true;
    ~graph();
};

graph* graph_create(std::shared_ptr<weight_store> weights); // null: the graph gets a store of its own (graph_add_weight)
int graph_add_weight(graph&, char const* name, int32_t dtype, const int64_t ne[4], const float* data);
int graph_find_weight(graph&, char const* name); // -1 if absent
int graph_input(graph&, int32_t dtype, const int64_t ne[4], char const* name);
int graph_add(graph&, int32_t op, const int* src, int n_src, const int64_t* ip, int n_ip, const float* fp, int n_fp);
void graph_set_name(graph&, int t, char const* name);
int graph_get_tensor(graph&, char const* name); // -1 if absent
void graph_output(graph&, int t, char const* name);
void graph_allocate(graph&, backend_device const* dev); // dev == null: lower and plan only
void graph_compute(graph&);
void graph_tensor_set(graph&, int t, const void* data, size_t bytes);            // the tensor's own dtype
void graph_tensor_get(graph&, int t, void* data, size_t bytes, bool as_f32);     // as_f32: converted on the host
// an input or output tensor lives at `ptr` (device memory of the caller, at least the tensor's size) instead of in the graph's arena;
// may be called again with another pointer between computes (not while a captured hipGraph of this graph is in use)
void graph_bind_external(graph&, int t, void* ptr);
void* graph_tensor_device_ptr(graph&, int t);                                    // where an input / output tensor lives
std::string graph_describe(graph const&); // one line per launch, then the arena summary

// The one weight arena of a graph-driven model: a planning pass of make_graph() says how many bytes of images the lowering makes of the
// weights, the arena gets that plus 1 MiB, and a second graph allocated on dev packs them into it in lowering order (the same order on every
// rank: what the broadcast at load time moves). Returns the part that holds images.
device_span build_weight_arena(weight_store&, backend_device const& dev, std::function<std::unique_ptr<graph>()> const& make_graph);

} // namespace visp
