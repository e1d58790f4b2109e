// COCO's uncompressed RLE of u8 masks on the device (vx_mask_rle_u8, kernels_rle.hip): the primitive on device and host arrays, and the generate call of
// MobileSAM with RLE records instead of mask bytes. Host C++ only. Every argument check runs before anything touches a device.
#pragma once
#include <vector>

#include "model.h"
#include "tinyvit.h"

namespace visp {

void check_rle_encode(int n, int w, int h, int64_t run_stride); // throws, touches no device
// masks u8 [n, h, w] -> runs u32 [n, run_stride] (nullable: count only) and n_runs i32 [n], all on the device; counts_dev (nullable): only the first counts[0]
// masks. The workspace (one bit per pixel, at most 256 masks in flight) is allocated for the CALL and freed behind a synchronisation of the stream.
void rle_encode_device(backend_device const* dev, void const* masks_dev, int n, int w, int h, void const* counts_dev, void* runs_dev, int64_t run_stride, void* n_runs_dev,
                       void* stream);
// host masks -> the runs of all masks one behind the other; offsets i64 [n + 1]: mask b's runs are [offsets[b], offsets[b + 1])
std::vector<uint32_t> rle_encode_host(backend_device const* dev, uint8_t const* masks, int n, int w, int h, int64_t* offsets);
// sam_generate_masks_device into a staging buffer of the model, the first counts[0] masks encoded behind it on the same stream; info_i32 [capacity][8],
// info_f32 [capacity][2], counts [2 or 4] as sam_generate_masks_host returns them, offsets i64 [capacity + 1] (entries behind counts[0] repeat the last one).
// No mask byte crosses to the host.
std::vector<uint32_t> sam_generate_masks_rle_host(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, sam_select_params const& p, int32_t* info_i32,
                                                  float* info_f32, int32_t* counts, int64_t* offsets);


// ---- the way back (kernels_rle_decode.hip): decode, area and pairwise IoU of CSR rows of runs ----
void check_rle_extent(char const* who, int n, int w, int h); // throws, touches no device
// host CSR rows: offsets non-decreasing from 0 .. ; with hw >= 0 every row sums to exactly hw. Throws naming the row and its sum.
void check_rle_rows(char const* who, int64_t const* offsets, uint32_t const* runs, int n, int64_t hw);
// device runs u32 and offsets i64 [n + 1] -> device masks u8 [n, h, w] with foreground `value`; status i32 [n] and area i64 [n] nullable (vx_rle_to_bits);
// counts_dev (nullable): only the first counts[0] masks. The offsets are read back and checked before the first launch; workspaces are allocated for the CALL,
// at most 256 masks in flight through the bit words; returns with the work done.
void rle_decode_device(backend_device const* dev, void const* runs_dev, void const* offsets_dev, int n, int w, int h, void const* counts_dev, int value, void* masks_dev,
                       void* status_dev, void* area_dev, void* stream);
// host rows -> host masks; a row whose runs do not sum to h w is refused before any launch
void rle_decode_host(backend_device const* dev, int64_t const* offsets, uint32_t const* runs, int n, int w, int h, int value, uint8_t* masks);
// area[b] = the sum of row b's odd runs. Host code: the runs are on the host and the sum is one pass over them.
void rle_area_host(int64_t const* offsets, uint32_t const* runs, int n, int64_t* area);
// One side of an IoU call: u8 masks [n, h, w], or CSR rows (runs, offsets [n + 1]) -- exactly one of the two.
struct mask_set {
    void const* masks = nullptr;
    void const* runs = nullptr;
    void const* offsets = nullptr;
    int n = 0, w = 0, h = 0;
};
void check_mask_iou(char const* who, mask_set const& a, mask_set const& b); // throws, touches no device
// iou f32 [na, nb], inter i32 [na, nb] (nullable), iscrowd u8 [nb] (nullable): vx_bitmask_iou on both sides' bit words. All pointers on the device.
void mask_iou_device(backend_device const* dev, mask_set const& a, mask_set const& b, void const* iscrowd_dev, void* iou_dev, void* inter_dev, void* stream);
// the same on host arrays: up, the matrix, down; rows of runs are held to their sum h w before any launch
void mask_iou_host(backend_device const* dev, mask_set const& a, mask_set const& b, uint8_t const* iscrowd, float* iou, int32_t* inter);

// ---- COCO's compressed counts strings (kernels_rle_codec.hip): CSR rows of runs <-> CSR rows of bytes (bytes u8, byte_offsets i64 [n + 1]) ----
void check_rle_codec(char const* who, int n); // throws, touches no device
// the first malformed record of host strings by pycocotools' rleFrString, the loop as it reads: status as vx_rle_decompress gives it, 0 (record -1) = all good
struct rle_string_fault { int record; int64_t byte; int status; };
rle_string_fault check_rle_strings(int64_t const* byte_offsets, uint8_t const* bytes, int n);
// count, then write, as the launcher: bytes_dev null -> sizes i32 [n] alone; else the strings at byte_offsets_dev. The run offsets are read back and checked before
// the first launch; the workspace is allocated for the CALL; returns with the work done.
void rle_compress_device(backend_device const* dev, void const* runs_dev, void const* offsets_dev, int n, void const* counts_dev, void* bytes_dev, void const* byte_offsets_dev,
                         void* sizes_dev, void* stream);
// host rows -> the strings one behind the other, byte_offsets i64 [n + 1]; a run at or above 2^31 is refused before any launch. Only sizes and strings come back.
std::vector<uint8_t> rle_compress_host(backend_device const* dev, int64_t const* offsets, uint32_t const* runs, int n, int64_t* byte_offsets);
// runs_dev null -> sizes i32 [n] alone; else the runs at offsets_dev; status i32 [n] nullable
void rle_decompress_device(backend_device const* dev, void const* bytes_dev, void const* byte_offsets_dev, int n, void const* counts_dev, void* runs_dev,
                           void const* offsets_dev, void* sizes_dev, void* status_dev, void* stream);
// host strings -> the runs one behind the other, offsets i64 [n + 1]; a malformed record is refused before any launch, naming the record, the byte and the status
std::vector<uint32_t> rle_decompress_host(backend_device const* dev, int64_t const* byte_offsets, uint8_t const* bytes, int n, int64_t* offsets);
// host masks -> strings: the encoder's two passes and the compressor's on one stream; only sizes and string bytes cross to the host
std::vector<uint8_t> rle_encode_compressed_host(backend_device const* dev, uint8_t const* masks, int n, int w, int h, int64_t* byte_offsets);
// sam_generate_masks_rle_host with strings out: byte_offsets i64 [capacity + 1]
std::vector<uint8_t> sam_generate_masks_coco_rle_host(sam_model& m, int32_t const* prompts, int32_t const* n_args, int n, sam_select_params const& p, int32_t* info_i32,
                                                      float* info_f32, int32_t* counts, int64_t* byte_offsets);

// ---- polygons and boxes to records, merged records, boxes of records (kernels_rle_poly.hip) ----
// Polygons are a CSR: xy f64 [total_vertices][2], poly_offsets i64 [n + 1], one extent w x h for all.
// pycocotools' rleFrPoly on one polygon of k >= 1 vertices, the loop as it reads, on the host: what the host entries hold their input against and what
// tools/bench_mask_rle_poly.py measures against. No entry falls back to it.
std::vector<uint32_t> poly_rle_reference(double const* xy, int64_t k, int w, int h);
// host polygons: offsets non-decreasing with k >= 1 everywhere, coordinates finite and at most 2^20 in size, fewer than 2^31 walked points, 1 .. 65535 polygons,
// w h below 2^31 - 1. Throws naming the polygon, touches no device. Returns the largest number of walked points.
int64_t check_polygons(char const* who, double const* xy, int64_t const* poly_offsets, int n, int w, int h);
// count, then write, as vx_poly_rle: runs_dev null -> sizes i32 [n] alone; else the runs at offsets_dev; status i32 [n] nullable. The polygon offsets are read
// back and checked, then each polygon's points and keys (2 n values) before the key rows are sized; workspaces are allocated for the CALL; returns with the work done.
void rle_from_poly_device(backend_device const* dev, void const* xy_dev, void const* poly_offsets_dev, int n, int w, int h, void const* counts_dev, void* runs_dev,
                          void const* offsets_dev, void* sizes_dev, void* status_dev, void* stream);
// host polygons -> the runs one behind the other, offsets i64 [n + 1]; bad input is refused before any launch
std::vector<uint32_t> rle_from_poly_host(backend_device const* dev, double const* xy, int64_t const* poly_offsets, int n, int w, int h, int64_t* offsets);
// boxes f64 [n][4] = {x, y, bw, bh} -> the polygons (x, y) (x, y + bh) (x + bw, y + bh) (x + bw, y), through rle_from_poly_host
std::vector<uint32_t> rle_from_bbox_host(backend_device const* dev, double const* boxes, int n, int w, int h, int64_t* offsets);
void check_rle_merge(char const* who, int n, int groups, int w, int h); // throws, touches no device
// device records and group_offsets i64 [groups + 1] over them -> device masks u8 [groups, h, w] (0 / value): the OR of each group's masks, the AND with intersect.
// Both offset arrays are read back and checked before the first launch.
void rle_merge_device(backend_device const* dev, void const* runs_dev, void const* offsets_dev, int n, void const* group_offsets_dev, int groups, int w, int h, int intersect,
                      int value, void* masks_dev, void* stream);
// host records -> the merged records: vx_rle_to_bits, vx_bits_merge, vx_bits_to_mask_u8 and the encoder's two passes on one stream; only runs come back
std::vector<uint32_t> rle_merge_host(backend_device const* dev, int64_t const* offsets, uint32_t const* runs, int n, int64_t const* group_offsets, int groups, int w, int h,
                                     int intersect, int64_t* out_offsets);
// boxes i32 [n][4] = {x, y, bw, bh} of device / host records
void rle_to_bbox_device(backend_device const* dev, void const* runs_dev, void const* offsets_dev, int n, int w, int h, void const* counts_dev, void* boxes_dev, void* stream);
void rle_to_bbox_host(backend_device const* dev, int64_t const* offsets, uint32_t const* runs, int n, int w, int h, int32_t* boxes);

} // namespace visp
