// MobileSAM's automatic mask generation: the batched decode with every prompt's planes kept, scored per chunk, then rank + NMS and the masks that survive
#include <algorithm>
#include <cmath>

#include "sam_pass.h"

namespace visp {

void sam_generate_check(int32_t const* prompts, int32_t const* n_args, int n, sam_select_params const& p) {
    if (!prompts || !n_args) throw except("sam: null argument");
    if (n < 1) throw except("sam: empty batch of prompts (n = %d)", n);
    if (n > kSamGenerateMaxPrompts)
        throw except("sam: %d prompts in one generate call, at most %d (three candidates each, 16384 candidates per call)", n, kSamGenerateMaxPrompts);
    if (std::isnan(p.pred_iou_thresh) || std::isnan(p.stability_thresh) || std::isnan(p.stability_offset) || std::isnan(p.nms_iou_thresh)) throw except("sam: a threshold is NaN");
    if (p.nms_iou_thresh < 0.0f || p.nms_iou_thresh > 1.0f) throw except("sam: nms_iou_thresh %g is outside [0, 1]", (double)p.nms_iou_thresh);
    if (p.stability_offset < 0.0f) throw except("sam: stability_offset %g is below 0", (double)p.stability_offset);
    if (p.capacity < 1) throw except("sam: capacity %d is below 1", p.capacity);
    if (p.min_region_area < 0) throw except("sam: min_region_area %d is below 0", p.min_region_area);
}

namespace {

// masks in flight through the labelling workspace of the cleaning stage: labels and areas, 8 bytes per pixel each (512 MB at 1024^2)
constexpr int kSamCleanGroup = 64;

// diagnostics (sam_enable_timing; tools/bench_sam_autogen.py): events around the stages, read after the call, which then waits for the device.
// open() records the first event; every mark(stage) after it ends an interval of that stage.
struct stage_marks {
    std::vector<void*> ev;
    std::vector<sam_generate_stage> stage;
    void* s;
    bool on;
    void open() { mark(sam_stage_count); } // stage[0] is never read
    void mark(sam_generate_stage closes) {
        if (!on) return;
        void* e = nullptr;
        VX(vx_event_create(&e));
        ev.push_back(e);
        stage.push_back(closes);
        VX(vx_event_record(e, s));
    }
    void sum_into(float (&out)[sam_stage_count]) {
        for (float& v : out) v = 0.0f;
        for (size_t i = 1; i < ev.size(); ++i) {
            float ms = 0.0f;
            VX(vx_event_elapsed_ms(ev[i - 1], ev[i], &ms));
            out[stage[i]] += ms;
        }
    }
    ~stage_marks() { for (void* e : ev) vx_event_destroy(e); }
};

} // namespace

void sam_generate_masks_device(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, sam_select_params const& p, sam_generate_outputs const& out, void* stream) {
    if (!out.masks || !out.info_i32 || !out.info_f32 || !out.counts) throw except("sam: null argument");
    sam_require_decoder(m);
    device_turn turn(*m.backend);
    void* s = stream ? stream : m.backend->stream;
    const int N = 3 * n; // the planes the reference chooses among (vision.cpp:80-82) are the candidates of a prompt
    const int64_t n_px = (int64_t)16 * m.dec.res * m.dec.res;
    const size_t nms_bytes = vx_sam_rank_nms_workspace_bytes(N);
    // the cleaning stage (min_region_area > 0) needs the masks somewhere other than their final place, since its second NMS reorders them: the first stage's masks
    // and records are staged in the workspace, capacity * h * w bytes (256 MB at 256 masks of 1024^2), next to the labelling workspace and the second NMS's tables
    const bool clean = p.min_region_area > 0;
    const size_t out_px = (size_t)m.image_extent[0] * m.image_extent[1];
    const int N2 = std::min(p.capacity, N), clean_group = std::min(N2, kSamCleanGroup);
    const size_t nms2_bytes = clean ? vx_sam_rank_nms_workspace_bytes(N2) : 0;
    const size_t regions_bytes = clean ? vx_mask_regions_workspace_bytes(m.image_extent[0], m.image_extent[1], clean_group) : 0;
    workspace_table ws;
    const auto logits_all = ws.add((size_t)n * 4 * n_px * 2, 256);
    const auto iou = ws.add<float>((size_t)n * 16, 256);
    const auto table = ws.add<int32_t>((size_t)N * 24, 256);
    const auto stab = ws.add<float>((size_t)N * 4, 256);
    const auto flags = ws.add<int32_t>((size_t)N * 4, 256), rank = ws.add<int32_t>((size_t)N * 4, 256), keep = ws.add<int32_t>((size_t)p.capacity * 4, 256);
    const auto nms = ws.add(nms_bytes, 256);
    const auto smasks = ws.add<uint8_t>((size_t)N2 * out_px, 256, clean);
    const auto sinfo = ws.add<int32_t>((size_t)N2 * 32, 256, clean);
    const auto sinfof = ws.add<float>((size_t)N2 * 8, 256, clean);
    const auto scounts = ws.add<int32_t>(8, 256, clean), changed = ws.add<int32_t>((size_t)N2 * 4, 256, clean), table2 = ws.add<int32_t>((size_t)N2 * 24, 256, clean);
    const auto key2 = ws.add<float>((size_t)N2 * 4, 256, clean);
    const auto flags2 = ws.add<int32_t>((size_t)N2 * 4, 256, clean), rank2 = ws.add<int32_t>((size_t)N2 * 4, 256, clean), keep2 = ws.add<int32_t>((size_t)N2 * 4, 256, clean);
    const auto counts2 = ws.add<int32_t>(8, 256, clean);
    const auto nms2 = ws.add(nms2_bytes, 256, clean), regions = ws.add(regions_bytes, 256, clean);
    grow(m.generate_ws, ws.layout.top, {m.backend->stream, s});
    ws.base = static_cast<uint8_t*>(m.generate_ws.ptr);
    int32_t* counts = static_cast<int32_t*>(out.counts);

    stage_marks marks{{}, {}, s, m.timing};
    marks.open();
    sam_decode_ctx ctx = sam_decode_prompts(m, prompts, n_args, n, logits_all, iou, nullptr, stream, m.last_batch,
                                            [&](sam_decode_ctx const& c, int p0, int B, void* logits, float*, int32_t*) {
        // the part of the plane the image occupies: SAM scores at image resolution, this scores the decoder's own logits
        const int cw = (c.sw * c.mask_size + c.image_size - 1) / c.image_size, ch = (c.sh * c.mask_size + c.image_size - 1) / c.image_size;
        marks.mark(sam_stage_decode);
        VX(vx_sam_score_planes_f16(logits, 4 * c.n_px, c.n_px, c.mask_size, 3, cw, ch, p.stability_offset, table + (size_t)p0 * 18, stab + (size_t)p0 * 3, B, c.s));
        marks.mark(sam_stage_scoring);
    });
    // the first stage's outputs: the caller's buffers, or with cleaning the staging buffers (of min(capacity, N) masks: no more can come out)
    uint8_t* masks1 = clean ? smasks : static_cast<uint8_t*>(out.masks);
    int32_t *info1 = clean ? sinfo : static_cast<int32_t*>(out.info_i32), *counts1 = clean ? scounts : counts;
    float* infof1 = clean ? sinfof : static_cast<float*>(out.info_f32);
    const int cap1 = clean ? N2 : p.capacity;
    VX(vx_sam_rank_nms(table, iou, 3, 4, N, p.pred_iou_thresh, p.stability_thresh, p.nms_iou_thresh, cap1, nms, nms_bytes, flags, rank, keep, counts1, s));
    marks.mark(sam_stage_rank_nms);
    VX(vx_sam_process_masks_indexed(logits_all, 4 * ctx.n_px, ctx.n_px, 1, ctx.mask_size, 3, n, keep, counts1, cap1, ctx.Bmax, ctx.scaled, ctx.image_size, ctx.sw, ctx.sh,
                                    masks1, ctx.target[0], ctx.target[1], s));
    VX(vx_sam_mask_stats_u8(masks1, ctx.target[0], ctx.target[1], keep, counts1, cap1, 3, n, iou, 4, stab, info1, infof1, s));
    if (clean) { // SAM's postprocess_small_regions: clean, measure again, a second NMS with the scores 1 (unchanged) / 0 (changed), the survivors in its order
        marks.mark(sam_stage_output);
        VX(vx_mask_remove_small_regions_u8(masks1, ctx.target[0], ctx.target[1], N2, counts1, p.min_region_area, VX_REGIONS_BOTH, changed, regions, regions_bytes,
                                           clean_group, s));
        marks.mark(sam_stage_clean);
        VX(vx_sam_mask_stats_u8(masks1, ctx.target[0], ctx.target[1], keep, counts1, N2, 3, n, iou, 4, stab, info1, infof1, s));
        VX(vx_sam_clean_nms_inputs(info1, changed, counts1, N2, table2, key2, s));
        VX(vx_sam_rank_nms(table2, key2, 1, 1, N2, -1.0f, 0.0f, p.nms_iou_thresh, N2, nms2, nms2_bytes, flags2, rank2, keep2, counts2, s));
        marks.mark(sam_stage_records_nms2);
        VX(vx_sam_gather_clean_masks(masks1, ctx.target[0], ctx.target[1], info1, infof1, changed, keep2, counts1, counts2, N2, static_cast<uint8_t*>(out.masks),
                                     static_cast<int32_t*>(out.info_i32), static_cast<float*>(out.info_f32), counts, s));
    }
    if (marks.on) {
        marks.mark(clean ? sam_stage_gather : sam_stage_output);
        marks.sum_into(m.generate_split_ms);
    }
    if (!stream) VX(vx_stream_sync(s));
}

void sam_generate_masks_host(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, sam_select_params const& p, sam_generate_outputs const& out) {
    if (!out.masks || !out.info_i32 || !out.info_f32 || !out.counts) throw except("sam: null argument");
    sam_require_decoder(m);
    device_turn turn(*m.backend);
    void* s = m.backend->stream;
    const size_t px = (size_t)m.image_extent[0] * m.image_extent[1];
    workspace_layout lay;
    const size_t o_m = lay.take((size_t)p.capacity * px), o_i = lay.take((size_t)p.capacity * 32), o_f = lay.take((size_t)p.capacity * 8), o_c = lay.take(16);
    device_buffer dev(lay.top);
    uint8_t* base = static_cast<uint8_t*>(dev.ptr);
    sam_generate_masks_device(m, prompts, n_args, n, p, {base + o_m, base + o_i, base + o_f, base + o_c}, s);
    int32_t* counts = static_cast<int32_t*>(out.counts);
    VX(vx_memcpy_d2h(counts, base + o_c, p.min_region_area > 0 ? 16 : 8, s));
    VX(vx_stream_sync(s));
    const size_t k = (size_t)std::min(std::max(counts[0], 0), p.capacity); // rows and masks behind the returned ones stay as the caller left them
    if (k) {
        VX(vx_memcpy_d2h(out.masks, base + o_m, k * px, s));
        VX(vx_memcpy_d2h(out.info_i32, base + o_i, k * 32, s));
        VX(vx_memcpy_d2h(out.info_f32, base + o_f, k * 8, s));
        VX(vx_stream_sync(s));
    }
}

} // namespace visp
