// The lowering of a graph into its launch list (graph_allocate, graph.h): internal to the graph layer. One struct, its state gathered
// here, its member functions defined by concern in
//   lower_weights.cpp  device images of weights and constants (cached / upload / pack_*)
//   lower_conv.cpp     the one emitter of a GEMM-family launch (product, emit_product), matrix products and convolutions with their fused epilogues,
//                      the planar maps, the DPT neck / head patterns
//   lower_encoder.cpp  attention, the fused q|k|v product, patch embedding, the DINOv2 encoder chain on the block kernel
//   lower_yolo.cpp     SiLU epilogues, the folded RepConv, channel slices and concats in place, pooling, softmax and the DFL decode
//   lower_migan.cpp    lrelu_agc epilogues, the x2 FIR upsample group, clamp and plane-broadcast launches
//   lower_sam.cpp      attention without a mask on token-major q / k / v, mul_mat of activations, sin / cos, the Fourier-feature group
//   lower_sam3.cpp     ROPE, the rope_2d group (alone, and in place behind the fused q|k|v product), get_rows with a run-time index
//   lower_birefnet.cpp resize and patches of an f32 image, the pixel gate group, bilinear resizes and LayerNorms that write into a concat's buffer
//   lower_run.cpp      liveness, the per-node dispatch, element-wise / copy / interpolate / image ops, the buffer plan
// Pattern functions MATCH first (const, nothing changes), and only when everything they need holds do they absorb nodes, pack and emit:
// a `return false` leaves the lowering's state as it was. A finder that accepts a group says so in ONE table (claim): a matcher asks free_node()
// whether a node may still join a group of its own and needs to know nothing about the other families.
#pragma once
#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>

#include "../../include/visp_hip_kernels.h"
#include "graph.h"
#include "visp_util.h"

namespace visp {

std::string shape_str(const int64_t ne[4]); // graph.cpp

struct packed_operand {
    void* w = nullptr;
    float* bias = nullptr;
    int N = 0, K = 0, n_real = 0, k_real = 0;
};

std::string weight_name(graph const& g, graph_node const& n); // of the node's second operand if that is a named weight, else the node's own name
std::string const_id(graph const& g, int t);                   // a key for the constant t: its name, "#index" if it has none, "-" for t < 0
bool is_conv3x3(graph_node const& c, graph_node const& w);     // conv_2d on a constant 3x3 kernel, stride 1, pad 1
bool same_shape(graph_node const& a, graph_node const& b);

struct lowering {
    graph& g;

    // ---- liveness and fusion marks (run): which nodes any output needs, who reads them; skip: computed by another node's launch
    std::vector<char> needed, skip;
    std::vector<int> uses;
    std::vector<std::vector<int>> consumers;
    std::vector<char> relu_on_load; // conv node -> the ReLU in front of it is applied by its loader
    // node -> the anchor node of the group whose launch will compute it, or -1: written by claim() when a finder accepts a group. skip[] keeps its own
    // meaning and timing (some groups set it when they match, others when their launch is emitted); this table is what matchers ask besides
    std::vector<int> claimed_by;

    // ---- the launch list's buffer traffic (emit; read by plan_arena)
    std::vector<std::pair<std::vector<int>, std::vector<int>>> io; // per launch: buffers read, buffers written

    // ---- weight images (lower_weights.cpp)
    std::map<std::pair<std::pair<int, int>, std::string>, void*> const_cache; // (node, role, derived-from) -> device copy made for this graph

    // ---- inputs that a consumer reads in place instead of through a copy / a resize launch (g.fused_models)
    struct sliced_rows { int src; int64_t begin, rows, stride; };  // rows [begin, begin + rows) of every group of `stride` rows of src
    std::map<int, sliced_rows> sliced_in;                           // slice node -> what its (sole, plain-GEMM) reader addresses directly
    struct resized_map { int buf; int hs, ws; };                    // the bilinear (align_corners) resize of [.., ws, hs, B] in `buf`
    std::map<int, resized_map> resized_in;                          // interpolate / projected node -> what its (sole) conv reader interpolates itself
    std::map<int, int> row_stride;                                  // node -> elements between rows when its buffer is padded for a GEMM reader
    std::map<int, int> preprojected; // interpolate node -> buffer that already holds the 1x1 projection of its SOURCE (written by the residual-unit launch)

    // ---- maps kept as 32-channel PLANES ([plane][B * H * W][32] f16) -- the layout the LDS-ring conv was built on for the ESRGAN dense blocks
    // (kernels_dconv.hip; profiles/r04_esrgan_layout_experiment.txt: 5 % faster than NHWC). Layout is this lowering's choice: a map is planar when
    // the conv that writes it read a planar map (or the f32 image), every reader that is such a conv takes it as it is, and any other reader gets
    // an NHWC copy made on first use. A channel concat of planar maps is then no launch at all: the dense block [x | x1 | x2 | x3 | x4] of
    // esrgan.cpp:27-41 is six planes of ONE buffer, x written by its producer into planes 0-1, every conv_block into the plane behind its input.
    struct planar_map { int buf; int plane0; int n_planes; int64_t plane_elems; };
    std::map<int, planar_map> planar;                 // ROOT node -> where it lives
    std::map<int, std::pair<int, int>> placed;        // node a concat chain will read -> (buffer, first plane) reserved for it
    std::map<int, int> up2_of;                        // interpolate(NEAREST, x2) node -> its (planar) source, resized by the reading conv's loader
    std::map<int, int> image_plane;                   // f32 image input -> buffer of its value | residue plane
    std::map<int, int> image8;                        // 3- or 4-channel f32 image -> buffer of its 8-channel value | residue pixels (image_pad8)

    // ---- attention and the encoder chain (lower_encoder.cpp)
    std::map<int, int> qkv_first;                 // first of the three linears (node order) -> attention node
    std::map<int, std::array<int, 3>> qkv_lin;    // attention node -> its three linears
    std::map<int, std::array<int, 3>> qkv_bufs;   // attention node -> head-major buffers, once the fused launch is emitted
    struct enc_layer {
        int ln1 = -1, lin[3] = {-1, -1, -1}, att = -1, o = -1, s1 = -1, x1 = -1, ln2 = -1, f1 = -1, ge = -1, f2 = -1, s2 = -1, x2 = -1;
        int lam1 = -1, lam2 = -1;
        std::vector<int> taps;
    };
    struct enc_chain {
        bool ok = false;
        int img = -1, u8 = -1, pe = -1, resh = -1, cat = -1, tok = -1, cls = -1, pos = -1, first = -1;
        std::vector<int> views;
        std::vector<enc_layer> layers;
    } enc;

    // ---- deformable-conv groups (lower_conv.cpp)
    // conv_2d(offset, x), scale(sigmoid(conv_2d(modulator, x)), s), conv_2d_deform(x, W, ., .) [-> mul(c) -> add(c) -> relu] (birefnet.cpp:83-92, 110-115)
    struct deform_group {
        int off = -1, mod = -1, sig = -1, scl = -1; // the offset conv, the modulator conv, its sigmoid and scale nodes
        int mul = -1, add = -1, relu = -1;          // the per-channel epilogue behind the deformable conv
        float s = 1.0f;
    };
    std::map<int, deform_group> deform_groups;      // conv_2d_deform node -> its group (g.fused_models)

    // ---- the packed-bias window attention (lower_encoder.cpp)
    // split_qkv(.., 1) of nn.cpp:182-208 feeding a masked attention at head_dim 32 with a constant per-head bias (mobile-sam.cpp:124-132):
    // linear -> reshape -> permute(0, 3, 1, 2) -> cont -> 3 x (slice -> reshape) -> attention_masked
    struct window_group { int lin = -1; std::vector<int> views; }; // the q|k|v linear; the nodes between it and the attention, computed by nobody
    std::map<int, window_group> window_groups;      // attention_masked node -> its group (g.fused_models)

    // ---- SiLU-conv / channel-split / channel-concat networks (lower_yolo.cpp; all of it g.fused_models only)
    struct located { int buf; int64_t off, pix; };  // a map inside a wider one: buffer, first channel, elements between pixels; a buffer of its own is {buf, 0, width}
    // conv_2d / linear -> silu [-> add(map computed before)], or silu(add(conv3x3(x), conv1x1(x))) keyed on the 3x3 conv: one GEMM-family launch
    struct silu_group { int silu = -1, add = -1, res = -1, rep1 = -1, rep_add = -1; };
    std::map<int, silu_group> silu_convs;              // product node -> what its launch computes besides
    std::map<int, int> rep_member;                     // the 1x1 conv of a folded RepConv -> its 3x3 conv
    std::map<int, int> launch_of_last;                 // last node of a silu group -> its product node
    std::map<int, std::pair<int, int>> chan_slice;     // slice of channels [c0, c1) only -> (source, c0): no launch, its readers address the source
    struct cat_source { int node; int c0; bool placed; };
    std::map<int, std::vector<cat_source>> cat_sources; // top concat of a dimension-0 chain with a placeable source -> its flattened sources
    std::map<int, std::pair<int, int>> cat_slot;       // last node of a launch -> (top concat, first channel) it writes into
    std::map<int, located> in_place;                   // node without a buffer of its own -> where it lives (set when its launch is emitted)
    struct dfl_group { int map = -1, c0 = 0, n = 0, groups = 0, proj = -1; std::vector<int> absorbed; };
    std::map<int, dfl_group> dfl_groups;               // sum_rows node -> slice -> [cont] -> reshape -> soft_max -> mul(constant) in front of it

    // ---- the node groups of MI-GAN (lower_migan.cpp; g.fused_models only)
    // what a launch takes over from the nodes behind it: [+ plane constant] [leaky_relu [scale] [clamp(-c, c)]] [+ map]
    struct agc_tail {
        int plane = -1, res = -1, last = -1;
        bool act = false;
        float slope = 0.0f, gain = 1.0f, clamp = 0.0f;
        std::vector<int> absorbed;
    };
    struct upfir_group { int src = -1, fir = -1; std::vector<int> members; agc_tail tail; }; // the map upsampled, the 4x4 kernel, interpolate .. [cont]
    std::map<int, upfir_group> upfir_at;                      // LAST node of a group -> the group its launch computes
    std::map<int, std::pair<int, agc_tail>> dw_agc_at;        // last node -> (conv_2d_depthwise node, its tail)
    std::map<int, std::pair<int, agc_tail>> conv_agc_at;      // last node -> (1x1 conv_2d node, its tail)
    std::map<int, double> bound_memo;                         // value_bound's results

    // ---- the nodes of the SAM prompt encoder and mask decoder (lower_sam.cpp; the Fourier group in BOTH lowering modes)
    struct fourier_group { int mm = -1, scale = -1, sin = -1, cos = -1; };  // mul_mat(constant [2, F], f32 input) -> scale(2 pi) -> {sin, cos}
    std::map<int, fourier_group> fourier_groups;              // concat(sin, cos, dim 0) node -> the group its one launch computes

    // ---- the nodes of the SAM3 encoders (lower_sam3.cpp; the groups with g.fused_models only)
    struct rope2d_group { int src = -1, slice[2] = {-1, -1}, rope[2] = {-1, -1}; }; // r [hd, heads, T, B]; the slices of its two halves and their ropes
    std::map<int, rope2d_group> rope2d_groups;               // concat(rope(slice(r, first half), px), rope(slice(r, second half), py), dim 0) node -> its group
    std::map<int, std::array<int, 2>> qkv_rope;              // attention node of a fused q|k|v chain -> the rope_2d groups (concat nodes) q and k come through

    // ---- the nodes of BiRefNet beyond a decoder block (lower_birefnet.cpp; the group with g.fused_models only)
    struct gate_group { int p = -1, conv = -1, sig = -1, rep = -1; }; // the map gated; conv_2d(1x1 to one channel) -> sigmoid -> [repeat to p's shape]
    std::map<int, gate_group> gate_groups;                   // mul(p, .) node -> the group its one launch computes

    explicit lowering(graph& gr) : g(gr) {}
    void run(); // the whole lowering: fills g.launches / g.buffers / the arena plan

    // ---- nodes, buffers, launches
    int root(int t) const {
        while (g.nodes[t].alias_of >= 0) t = g.nodes[t].alias_of;
        return t;
    }
    int root_view(int v) const { // the node behind reshape / cont views (before aliases are assigned)
        while (g.nodes[v].op == gop_reshape || g.nodes[v].op == gop_cont) v = g.nodes[v].src[0];
        return v;
    }
    // the sole reader of t, if it is not an output
    int sole_consumer(int t) const { return uses[t] == 1 && !g.nodes[t].is_output && consumers[t].size() == 1 ? consumers[t][0] : -1; }
    int buf_of(int t) {
        const int r = root(t);
        if (g.nodes[r].buffer < 0 && planar.count(r)) planar_to_nhwc(r); // a reader outside the LDS-ring conv: the map as NHWC, once
        const int b = g.nodes[r].buffer;
        if (b < 0) throw except("graph: tensor %d (%s) is read before it is computed", t, graph_op_name(g.nodes[t].op));
        return b;
    }
    int new_buffer(size_t bytes, bool persistent = false) {
        graph_buffer b;
        b.bytes = round_up<size_t>(bytes, 256) + 256;
        b.persistent = persistent;
        b.first = b.last = (int)g.launches.size();
        g.buffers.push_back(b);
        return (int)g.buffers.size() - 1;
    }
    void materialise(int t) {
        graph_node& n = g.nodes[t];
        n.buffer = new_buffer(n.n_bytes(), n.is_output || n.op == gop_input);
    }
    void emit(std::string desc, std::vector<int> reads, std::vector<int> writes, std::function<void(void*)> run) {
        graph_launch l;
        l.desc = std::move(desc);
        l.run = std::move(run);
        g.launches.push_back(std::move(l));
        io.emplace_back(std::move(reads), std::move(writes));
    }
    void tag(const char* group, double flops = 0, double bytes = 0) { // timing group and algorithmic work of the launch emitted last
        graph_launch& l = g.launches.back();
        l.group = group;
        l.flops = flops;
        l.bytes = bytes;
    }
    // device pointer of a buffer at run time (offsets are assigned after the launch list is complete)
    std::function<char*()> ptr(int buf) {
        graph* gp = &g;
        return [gp, buf]() {
            graph_buffer const& b = gp->buffers[buf];
            return b.external ? static_cast<char*>(b.external) : static_cast<char*>(gp->arena.ptr) + b.offset;
        };
    }
    // a finder accepted a group: `anchor`'s launch will compute `nodes` (entries < 0 are left out). Two groups never share a node
    void claim(int anchor, std::vector<int> const& nodes) {
        for (int c : nodes) {
            if (c < 0) continue;
            if (claimed_by[c] >= 0 && claimed_by[c] != anchor)
                throw except("graph: internal: node %d (%s) is claimed by the group of node %d and by the group of node %d", c, graph_op_name(g.nodes[c].op), claimed_by[c], anchor);
            claimed_by[c] = anchor;
        }
    }
    bool free_node(int c) const { return c >= 0 && needed[c] && !skip[c] && claimed_by[c] < 0; } // c may still join a group: no launch computes it yet
    // src[0]'s buffer in, a freshly materialised buffer of t out (and `scratch_bytes` of a further buffer the launch writes): one launch
    void map_launch(int t, std::string desc, std::function<void(char* x, char* out, char* scratch, void* stream)> run, size_t scratch_bytes = 0);

    // ---- lower_weights.cpp
    void* cached(int t, pack_role role, std::function<void*(bool)> make, std::string const& with = {});
    void* upload(const void* host, size_t bytes, bool to_store);
    float* const_f32(int t);
    void* const_f16(int t);
    float* vec_cached(int key_node, pack_role role, std::string const& with, std::function<std::vector<float>()> make_host);
    float* bias_padded(int bt, int n_pad);
    packed_operand pack_matrix(int wt, pack_role role, int n, int k, std::function<float(int, int)> at, int bias_t, int bias_period, int scale_t = -1);
    packed_operand pack_rows(int wt, int bias_t, int n, int scale_t = -1);
    packed_operand pack_qkv(const int lin[3]);
    packed_operand pack_conv_transpose(int wt, int bias_t, int s);
    void* pack_head_fragments(int wt, int cin);
    void* pack_dconv(int wt, int cin, int cout, int* d_cin);
    void* pack_dconv_ex(int wt, int cin, int dup, int cout, int cout_pad, int* d_cin);
    void* pack_rcu(int wt, int taps);
    void* pack_deform(int wt, int* n_pad);
    packed_operand pack_deform_offsets(int w_off, int b_off, int w_mod, int b_mod);
    void* pack_depthwise(int wt, int C, int k);
    packed_operand pack_image8(int wt, int bias_t, int n);

    // ---- lower_conv.cpp
    // One launch of the GEMM family (vx_gemm_f16, or vx_conv3x3_f16 where `halo` allows and the arguments fit), planned as data: everything but the
    // run-time addresses. The planners (gemm_like, yolo_product, migan_product, ..) decide and fill it; emit_product turns it into the launch.
    struct product {
        vx_gemm_args a;                                   // zeroed; A / out / res1 / res2 / q / k / vt are set when the launch runs
        packed_operand p;
        located in{-1, 0, 0}, out{-1, 0, 0}, res1{-1, 0, 0}; // where A, the output and the first residual lie (buf < 0: none; pix is the planner's to put into `a`)
        int res2 = -1;                                    // the second residual's buffer
        std::array<int, 3> qkv{-1, -1, -1};               // VX_EPI_QKV: the head-major q, k, v buffers it writes
        size_t zero_at = 0;                               // byte offset into A's buffer of 128 bytes of slack to zero first (0: none)
        bool halo = false;                                // vx_conv3x3_f16 may take the launch
        std::string desc, group;
        double flops = 0, bytes = 0;
        product() { memset(&a, 0, sizeof a); }
        void operand(packed_operand const& q) { p = q; a.W = q.w; a.bias = q.bias; a.N = q.N; a.K = q.K; }
        void work(double reads_per_row, double writes_per_row) { // 2 M N K, and the rows read and written plus the operand's image
            flops = 2.0 * a.M * (double)p.n_real * p.k_real;
            bytes = (double)a.M * (reads_per_row + writes_per_row) * 2 + (double)p.N * p.K * 2;
        }
    };
    void emit_product(product const& P);
    static bool image8_input(graph_node const& x) { return x.dtype == gdt_f32 && (x.ne[0] == 3 || x.ne[0] == 4); } // read as 8-channel value | residue pixels (image_pad8)
    void conv_geometry(vx_gemm_args& a, graph_node const& n, graph_node const& x, graph_node const& w) const;
    void pack_conv_rows(product& P, graph_node const& n, bool image8_in, int rep1 = -1, int scale_t = -1);
    // What a product's launch takes over from the nodes behind it: [* LayerScale] [gelu | relu | leaky_relu] [(* s1) + res] [(* s2) + res2].
    // A matcher fills it and changes nothing; absorb() applies exactly what was matched.
    struct epilogue {
        int act = 0; // 1 gelu (the planar conv: leaky_relu 0.2), 2 relu
        int res = -1, res2 = -1, last = -1, scale = -1;
        float s1 = 1.0f, s2 = 1.0f; // the planar conv's factors in front of its residual steps
        std::vector<int> absorbed;  // the nodes this launch computes besides its own
    };
    epilogue match_epilogue(int t, bool allow_gelu, bool allow_scale = false, bool allow_two = false, bool res_after_relu = true) const;
    epilogue match_planar_epilogue(int t) const;
    void absorb(std::vector<int> const& nodes, int into);
    void absorb(epilogue const& e, int into) { absorb(e.absorbed, into); }
    bool residual_ready(int other, int t) const;
    struct residual_ptrs { std::function<char*()> res1, res2; };
    residual_ptrs read_residuals(epilogue const& e, std::vector<int>& reads);
    int padded_rows(int t, int K, int Kp, int64_t M, std::string const& who);
    int plain_gemm_reader(int t) const;
    bool dconv_shape(graph_node const& n, graph_node const& x, graph_node const& w) const;
    void gemm_like(int t);
    void dconv(int t, std::string const& who);
    bool residual_unit(int t, std::string const& who);
    bool planar_conv(int t, std::string const& who);
    void planar_to_nhwc(int r);
    bool nearest_into_reader(int t);
    bool resize_into_reader(int t);
    bool head_tail(int t);
    void one_channel_head(int t);
    bool match_deform_group(int t, deform_group& G) const;
    void find_deform_groups();
    void deform_conv(int t);
    void deform_fused(int t, deform_group const& G);
    int image_pad8(int xs);
    void depthwise_conv(int t);

    // ---- lower_encoder.cpp
    void find_qkv_groups();
    void fused_qkv(int att);
    std::array<int, 3> heads_major(graph_node const& n, float q_scale);
    void attention(int t);
    void attention_masked(int t);
    bool match_window_group(int att, window_group& G) const;
    void find_window_groups();
    void window_attention(int t, window_group const& G);
    void patch_embed(int t);
    bool match_layer(int att, enc_layer& L) const;
    void find_encoder_chain();
    void emit_encoder();

    // ---- lower_yolo.cpp: the patterns of SiLU-conv / channel-split / channel-concat networks (yolov9t.cpp; all of it g.fused_models only)
    bool channels_only(graph_node const& s) const;
    std::vector<int> readers_through_conts(int t) const;
    bool gemm_family_reader(int c, int view) const;
    bool in_place_readers_ok(int t, std::vector<int> const& chain) const;
    bool match_silu_group(int t, silu_group& G) const;
    bool match_dfl_group(int t, dfl_group& G) const;
    bool placeable_launch(int s) const;
    void find_yolo_groups();
    bool lives_in_place(int t) const;
    located locate(int t);
    located output_slot(int t, int last);
    bool yolo_takes(int t) const;
    void yolo_product(int t);
    void pool_2d(int t);
    void nearest_in_place(int t);
    void concat_in_place(int t);
    void soft_max(int t);
    void sum_rows(int t);
    packed_operand pack_rep_conv(int w3, int b3, int w1, int b1);

    // ---- lower_migan.cpp: the node groups of MI-GAN (migan.cpp; the groups with g.fused_models only), clamp and plane-broadcast launches
    double value_bound(int v);                                // a proven bound of |values| of map v from the graph alone, or infinity
    bool will_live_in_place(int v) const;                     // v (through cont / reshape views) is a channel slice read in its source or a map placed in a concat
    agc_tail match_agc_tail(int from, bool allow_plane, bool allow_add) const;
    bool match_upfir_group(int t, upfir_group& G) const;
    void find_migan_groups();
    bool migan_emits(int t);
    float* plane_f32(int t);
    void migan_upfir(int last, upfir_group const& G);
    void migan_depthwise(int last, int t, agc_tail const& T);
    void migan_product(int last, int t, agc_tail const& T);
    void clamp_op(int t);
    void plane_binary(int t);

    // ---- lower_sam.cpp
    bool match_fourier_group(int cat, fourier_group& G) const;
    void find_sam_groups();
    void fourier_features(int t, fourier_group const& G);
    int token_rows(int t, const char* who);
    void attention_cross(int t);
    void mul_mat(int t);
    void sincos(int t);

    // ---- lower_sam3.cpp
    float* rope_table(int pos_t, int n, float base, float scale);
    bool match_rope2d_group(int cat, rope2d_group& G) const;
    void find_sam3_groups();
    void rope2d(int t, rope2d_group const& G);
    void rope2d_in_place(int att, std::array<int, 3> const& hb);
    void rope(int t);
    void get_rows(int t);

    // ---- lower_birefnet.cpp
    void image_resize(int t);
    void image_patches(int t);
    bool match_gate_group(int t, gate_group& G) const;
    void find_birefnet_groups();
    void pixel_gate(int t, gate_group const& G);
    int norm_behind(int v) const;
    void bilinear_in_place(int t);
    void layer_norm_in_place(int t);

    // ---- lower_run.cpp
    void copy_op(int t);
    void plan_arena();
};

} // namespace visp
