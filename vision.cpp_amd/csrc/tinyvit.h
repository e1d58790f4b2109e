// TinyViT image encoder of MobileSAM on the MI355X backend (BASELINE.json configs[4]): model
// load (mobile-sam GGUF -> packed f16 weights), static schedule, batched executor. Mirrors sam_load_model / sam_encode
// (reference src/visp/vision.cpp:26-52; graph src/visp/arch/mobile-sam.cpp:20-215, sam_process_input :533-547), and the
// prompt encoder + mask decoder + mask post-processing (vision.cpp:54-92, mobile-sam.cpp:207-583): ONE decoder schedule with the
// prompt index folded into its rows, behind sam_compute (one prompt), sam_compute_batch_* and sam_generate_masks_*.
#pragma once
#include <vector>

#include "gguf.h"
#include "image.h"
#include "model.h"

namespace visp {

struct tiny_vit_layer { int resolution, embed_dim, depth, num_heads, window_size; bool downsample; };
struct tiny_vit_params { // mobile-sam.h:16-37
    int img_size = 1024;
    tiny_vit_layer layers[4] = {{256, 64, 2, 2, 7, true}, {128, 128, 2, 4, 7, true}, {64, 160, 6, 5, 14, true}, {64, 320, 2, 10, 7, false}};
};

struct packed_dw { size_t w = 0, b = 0; int C = 0; };   // depthwise 3x3: f16 [9][C] + f32 bias [C]
struct tv_mbconv_weights { packed_gemm conv1, conv3; packed_dw conv2; size_t conv3_frag = SIZE_MAX; }; // conv3_frag: vx_mbconv_pack_w3 image
struct tv_merge_weights { packed_gemm conv1, conv3; packed_dw conv2; int stride = 2; };
// opt-in e4m3 image of a linear weight (kernels_gemm_fp8.hip): rows [N pad 128][K pad 128] + one f32 scale per row, offsets into sam_model::fp8_arena
struct fp8_linear { size_t w = SIZE_MAX, s = SIZE_MAX; int N = 0, Kp = 0; };
struct tv_block_weights {
    packed_vec attn_ln_w, attn_ln_b, bias; // bias: attention_biases_indexed packed f16 (vx_window_attention_pack_bias), n = f16 count
    packed_gemm qkv, proj, fc1, fc2;
    fp8_linear fc1_e4m3, fc2_e4m3;
    packed_dw local_conv;
    packed_vec mlp_ln_w, mlp_ln_b;
};
struct tinyvit_weights {
    packed_gemm pe0, pe2; // patch_embed.seq.0 (3 -> 32, input channels 3..5 repeat 0..2), seq.2
    std::vector<tv_mbconv_weights> mbconv;
    tv_merge_weights merge[3];
    std::vector<tv_block_weights> blocks[4];
    packed_gemm neck0, neck2;
    packed_vec neck1_w, neck1_b, neck3_w, neck3_b;
};

// prompt encoder + mask decoder (mobile-sam.cpp:207-483); present when the file holds the dec.* / prompt_encoder.* tensors
struct sam_attn_weights { packed_gemm q, k, v, o; };
struct sam_twoway_weights {
    sam_attn_weights self_attn, t2i, i2t;
    packed_gemm lin1, lin2;
    packed_vec norm_w[4], norm_b[4];
};
struct samdec_weights {
    bool present = false;
    int dim = 256, heads = 8, res = 64;
    std::vector<float> gaussian;                       // host: positional_encoding_gaussian_matrix [2][dim/2]
    std::vector<float> point_embed[4], not_a_point;    // host: label embeddings [dim]
    std::vector<float> output_tokens;                  // host: [iou_token | mask_tokens] = [5][dim]
    packed_vec no_mask, dense_pe;                      // arena f16: [dim], [res*res][dim] (n = f16 count)
    std::vector<sam_twoway_weights> layers;
    sam_attn_weights final_attn;
    packed_vec final_norm_w, final_norm_b;
    packed_gemm up0, up3;                              // conv_transpose k2 s2 as GEMM + pixel shuffle
    packed_vec up_norm_w, up_norm_b;
    int up_c1 = 0, up_c2 = 0;
    packed_gemm hyper[4][3], iou_head[3];
    // The prompt encoder's tables above are host arithmetic: their f32 values ALSO live in the weight arena (tables_off: gaussian |
    // point_embed[4] | not_a_point | output_tokens = 11 dim floats), so that a rank whose arena arrived by RCCL broadcast
    // (load_no_upload) rebuilds them in sam_weights_ready; the f32 iou head of the device (sam_model::iou_head_dev) is made there too.
    size_t tables_off = SIZE_MAX;
};
// the stages sam_model::generate_split_ms tells apart; the last three run with min_region_area > 0 only
enum sam_generate_stage { sam_stage_decode, sam_stage_scoring, sam_stage_rank_nms, sam_stage_output, sam_stage_clean, sam_stage_records_nms2, sam_stage_gather, sam_stage_count };
// test hook (captures on): the logit planes [n][4][mask_size^2] (f16-rounded) and the iou predictions [n][4] a decode left; empty with captures off
struct sam_kept_logits { std::vector<float> masks, iou; };

struct sam_model : model_base { // vision.h sam_model counterpart (encoder part)
    sam_model() : model_base(family_sam) {}
    tiny_vit_params params;
    tinyvit_weights weights;
    device_buffer weight_arena;
    bool weights_uploaded = false;
    device_buffer ws;
    samdec_weights dec;
    sam_kept_logits last_single;  // of the last sam_compute (n = 1), for visp_sam_read_masks
    device_buffer single_out;     // sam_compute's mask on the device, on its way to the host
    device_buffer embed;          // image embedding of the last sam_encode: f32 [64, 64, 256] (NHWC)
    i32x2 image_extent = {{0, 0}}; // extent of the image passed to sam_encode (vision.h sam_model::image_extent)
    // BASELINE.json configs[4] ("fp8 GGUF weights on CDNA4 fp8 MFMA"), opt-in and never the default: the MLPs of the transformer stages
    // (mobile-sam.cpp:150-160: fc1 + gelu, fc2 + residual -- 39 % of the encoder's time) on the block-scaled e4m3 matrix instruction, activations
    // quantised per token on the way in. The decision on accuracy stands (tests/test_fp8_decision.py: mask IoU below the bar); this is the measured form of it.
    bool fp8_mlp = false;
    device_buffer fp8_arena, fp8_ws;
    // the decoder (sam_compute is a batch of one, sam_compute_batch_*, sam_generate_masks_*): prompts run in chunks of prompt_chunk, the workspace is
    // sized for one chunk of the largest call so far
    int prompt_chunk = 64;
    device_buffer batch_ws;
    device_buffer iou_head_dev;            // f32 [w0 | b0 | w1 | b1 | w2 | b2]: the f16-rounded iou head, uploaded by sam_weights_ready
    size_t iou_head_off[6] = {0, 0, 0, 0, 0, 0}; // byte offsets into it
    void* prompt_tokens_host = nullptr;    // pinned: the prompt tokens of one call, f16 [n][7][dim]
    size_t prompt_tokens_bytes = 0;
    void* prompt_tokens_event = nullptr;   // recorded behind their upload: the next call waits for it before it overwrites them
    sam_kept_logits last_batch;            // of the last batch or generate call, for visp_sam_read_masks_batch; a sam_compute in between leaves it alone
    // automatic mask generation (sam_generate_masks_device): the logit planes and iou predictions of every prompt of the call, the selection stage's tables
    // and the NMS workspace, next to the decoder's batch_ws
    device_buffer generate_ws;
    // with timing enabled: the last generate call's ms per sam_generate_stage, by events
    float generate_split_ms[sam_stage_count] = {};
    ~sam_model() override;
};
void sam_set_fp8_mlp(sam_model&, bool enable); // builds the e4m3 weight images on first use (from the f16 weights on the device)

sam_model* sam_load_model(char const* filepath, backend_device const& dev, int flags = load_default);
void sam_weights_ready(sam_model&);
// B images rgb_u8 [B, 1024, 1024, 3] already at the model extent, on the device -> image embeddings f32 [B, 64, 64, 256] (NHWC)
void sam_encode_batch_device(sam_model&, void const* rgb_dev, int batch, void* out_dev, void* stream);
void sam_encode_batch_host(sam_model&, uint8_t const* rgb, int batch, float* out);
// reference API (vision.cpp:36-52): any extent, any u8 colour format; longest side scaled to 1024, edge-replicated to the
// square (sam_process_input); the embedding stays on the device in model.embed
void sam_encode(sam_model&, image_view image);
// reference API (vision.cpp:54-92): point (n = 2) or box (n = 4) in pixels of the image given to sam_encode -> alpha_u8 mask
// at that image's extent (best of the first three masks by predicted iou). A batch of one prompt through the decoder of
// sam_compute_batch_*: the same bytes as that call with this prompt alone; one synchronisation, at the end.
image_data sam_compute(sam_model&, int const* prompt, int n);
// n prompts on the embedding of the last sam_encode in one batched pass. prompts host [n][4], n_args host [n] (2 = point, 4 = box); device outputs
// masks u8 [n][h][w] at the encoded image's extent, iou f32 [n][4], chosen i32 [n] (the last two nullable). Runs in chunks of m.prompt_chunk prompts;
// no host synchronisation (stream == nullptr: the device's stream, synchronised at the end; captures: synchronised per chunk).
void sam_compute_batch_device(sam_model&, int32_t const* prompts, int32_t const* n_args, int n, void* masks_u8_dev, void* iou_dev, void* chosen_dev, void* stream);
void sam_compute_batch_host(sam_model&, int32_t const* prompts, int32_t const* n_args, int n, uint8_t* masks_u8, float* iou, int32_t* chosen);
void sam_set_prompt_chunk(sam_model&, int n); // 1 .. 256
// SAM's automatic mask generator on the prompts of a batch call (one crop layer, no crop-edge filter): every prompt gives three candidates (planes 0 .. 2),
// filtered by predicted iou and stability score, ranked by predicted iou, de-duplicated by greedy box NMS; the first min(kept, capacity) come out as u8 masks
// [capacity][h][w] with info_i32 [capacity][8] = {prompt, plane, x, y, w, h, area, 0}, info_f32 [capacity][2] = {predicted_iou, stability_score} and
// counts i32 [2] = {returned, kept}. Device outputs; rows and masks at and behind counts[0] untouched. No host synchronisation beyond sam_compute_batch_device's.
constexpr int kSamGenerateMaxPrompts = 5461; // 16384 candidates
// With min_region_area > 0, SAM's min_mask_region_area (postprocess_small_regions) runs behind that first stage: its first k = min(kept, capacity) masks, produced
// exactly as above into a staging buffer in generate_ws (capacity * h * w bytes: the second NMS reorders them, so they cannot be cleaned in their final place), are cleaned
// (vx_mask_remove_small_regions_u8: holes, then islands, below min_region_area pixels; 64 masks in flight, 8 bytes per pixel each), measured again, and passed
// through a second greedy NMS on their inclusive image-pixel boxes with the scores 1 (unchanged) / 0 (changed), equal scores in first-stage order. The survivors
// come out in that order -- unchanged masks first, then changed ones, each by predicted iou: NOT the order without cleaning --, info_i32 column 7 = 1 for a changed
// mask, counts i32 [4] = {returned, kept by the first NMS, returned masks that cleaning changed, masks the second NMS removed}. min_region_area 0: the first
// stage alone (counts [2]). Nothing waits for the host beyond where that does.
struct sam_select_params { float pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh; int capacity, min_region_area; };
struct sam_generate_outputs { void *masks, *info_i32, *info_f32, *counts; }; // all on the device, or all on the host
// throws on what needs neither model nor device to refuse: the C entries call it before they look the handle up, the two functions below do not repeat it
void sam_generate_check(int32_t const* prompts, int32_t const* n_args, int n, sam_select_params const&);
void sam_generate_masks_device(sam_model&, int32_t const* prompts, int32_t const* n_args, int n, sam_select_params const&, sam_generate_outputs const& dev, void* stream);
void sam_generate_masks_host(sam_model&, int32_t const* prompts, int32_t const* n_args, int n, sam_select_params const&, sam_generate_outputs const& host);

} // namespace visp
