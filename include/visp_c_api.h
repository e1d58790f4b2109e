/*
 * visp_c_api.h -- the drop-in C ABI of the MI355X backend (lib/libvisioncpp.so).
 *
 * Part 1 re-exports, with identical names, signatures and semantics, the 11 symbols of the
 * reference's C API (reference src/visp/c-api.cpp:145-253), i.e. exactly what the reference's
 * ctypes binding (bindings/python/visioncpp/_lib.py:118-171) binds. Return value 1 = ok,
 * 0 = error with the message available from visp_get_last_error() (thread-local,
 * c-api.cpp:6-21). Built behind it: depth_anything, esrgan, sam (MobileSAM: image encoder + prompt encoder / mask decoder) and
 * birefnet (swin-T / BiRefNet-lite); migan through visp_migan_load (visp_model_load returns "not built in this backend"); yolov9t
 * through visp_yolov9t_load (the reference has no model_family for it).
 *
 * Part 2 is the batched, device-resident extension the reference does not have (its
 * depthany_compute is batch 1, src/visp/vision.cpp:155): it is what bench.py and a
 * data-parallel caller use.
 */
#ifndef VISP_C_API_H
#define VISP_C_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VISP_API __attribute__((visibility("default")))

/* visp::image_format, include/visp/image.h:17-29 */
enum visp_image_format {
    VISP_RGBA_U8 = 0, VISP_BGRA_U8, VISP_ARGB_U8, VISP_RGB_U8, VISP_ALPHA_U8,
    VISP_RGBA_F32, VISP_RGB_F32, VISP_ALPHA_F32
};
/* visp::backend_type, include/visp/ml.h:32-36 */
enum visp_backend_type { VISP_BACKEND_AUTO = 0, VISP_BACKEND_CPU = 1, VISP_BACKEND_GPU = 2, VISP_BACKEND_VULKAN = 258 };
/* visp::model_family, include/visp/vision.h:86-94 */
enum visp_model_family { VISP_SAM = 0, VISP_BIREFNET, VISP_DEPTH_ANYTHING, VISP_MIGAN, VISP_ESRGAN, VISP_FAMILY_COUNT };

/* == visp::image_view {i32x2 extent; int stride; image_format format; void const* data}
 * (include/visp/image.h:37-41) == c-api.cpp:121-127 visp_image_view == _lib.py:36-43 ImageView */
typedef struct visp_image_view {
    int32_t width;
    int32_t height;
    int32_t stride; /* bytes per row */
    int32_t format;
    void* data;
} visp_image_view;

typedef struct visp_image_data visp_image_data; /* visp::image_data, owned by the library */
typedef struct visp_device visp_device;         /* visp::backend_device */
typedef struct visp_model visp_model;           /* any_model (c-api.cpp:193) */

/* ---- Part 1: the reference's symbols ------------------------------------------------- */
VISP_API char const* visp_get_last_error(void);                                   /* c-api.cpp:147 */
VISP_API void visp_image_destroy(visp_image_data* img);                           /* :153 */
VISP_API int32_t visp_backend_load_all(char const* dir);                          /* :159 (no-op here: returns 1 backend) */
VISP_API int32_t visp_device_init(int32_t type, visp_device** out_device);        /* :164 */
VISP_API void visp_device_destroy(visp_device* d);                                /* :174 */
VISP_API int32_t visp_device_type(visp_device const* d);                          /* :178 */
VISP_API char const* visp_device_name(visp_device const* d);                      /* :182 */
VISP_API char const* visp_device_description(visp_device const* d);               /* :188 */
VISP_API int32_t visp_model_detect_family(char const* filepath, int32_t* out_family); /* :198 */
VISP_API int32_t visp_model_load(char const* filepath, visp_device const* dev, int32_t arch, visp_model** out); /* :206 */
VISP_API void visp_model_destroy(visp_model* model, int32_t arch);                /* :222 */
/* Depth-Anything: inputs[0] any u8 format; returns alpha_u8 after image_normalize (c-api.cpp:72-77) */
VISP_API int32_t visp_model_compute(visp_model* model, int32_t family, visp_image_view* inputs, int32_t n_inputs,
                                    int32_t* args, int32_t n_args, visp_image_view* out_image,
                                    visp_image_data** out_data);                  /* :230 */

/* ---- Part 2: MI355X extension ---------------------------------------------------------- */
/* like visp_device_init(GPU) but on an explicit HIP device index (one process per GPU) */
VISP_API int32_t visp_hip_device_init(int32_t device_index, visp_device** out_device);

enum { VISP_LOAD_DEFAULT = 0, VISP_LOAD_NO_UPLOAD = 1 /* parse + allocate only; weights arrive by broadcast */ };
VISP_API int32_t visp_model_load_ex(char const* filepath, visp_device const* dev, int32_t arch, int32_t flags,
                                    visp_model** out);
/* packed device weight arena (one allocation) -- the unit RCCL broadcasts at load */
VISP_API int32_t visp_depthany_weights_arena(visp_model* m, void** device_ptr, size_t* n_bytes);
/* call after a VISP_LOAD_NO_UPLOAD model's arena has been filled by the broadcast */
VISP_API int32_t visp_depthany_weights_ready(visp_model* m);

typedef struct visp_depthany_info {
    int32_t patch_size, embed_dim, n_layers, n_heads;
    int32_t image_size, image_multiple;
    int32_t feature_layers[4];
    float max_depth;
} visp_depthany_info;
VISP_API int32_t visp_depthany_get_info(visp_model const* m, visp_depthany_info* out);
/* depthany_image_extent (depth-anything.cpp:112-117) */
VISP_API int32_t visp_depthany_image_extent(visp_model const* m, int32_t w, int32_t h, int32_t* out_w, int32_t* out_h);

/* Pre-allocates the activation workspace for `batch` images of w x h (w,h multiples of the
 * patch size). Also called implicitly on the first compute of a new shape. */
VISP_API int32_t visp_depthany_reserve(visp_model* m, int32_t batch, int32_t w, int32_t h);

/* Batched hot path, everything on the device: rgb_u8 [batch,h,w,3] -> out [batch,h,w] f32 in [0,1]
 * (depthany_compute semantics per image: process_input, predict, image_normalize).
 * raw_out (nullable) receives the un-normalised depth. Asynchronous on `stream` (hipStream_t,
 * NULL = the model's own stream, in which case the call returns after synchronising). */
VISP_API int32_t visp_depthany_compute_batch_device(visp_model* m, void const* rgb_u8_dev, int32_t batch, int32_t w,
                                                    int32_t h, void* out_dev, void* raw_out_dev, void* stream);
/* the reference's C++ depthany_compute (vision.cpp:147-167): one image of any extent / u8 colour format -> alpha_f32 in [0, 1] at
 * the caller's extent (visp_model_compute returns the same map as alpha_u8, c-api.cpp:72-77); result owned by *out_data */
VISP_API int32_t visp_depthany_compute_f32(visp_model* m, visp_image_view const* image, visp_image_view* out_image, visp_image_data** out_data);
/* same with host buffers (H2D + compute + D2H on the model's stream, blocking) */
VISP_API int32_t visp_depthany_compute_batch_host(visp_model* m, uint8_t const* rgb_u8, int32_t batch, int32_t w,
                                                  int32_t h, float* out, float* raw_out);
/* Multi-GPU from C: models[i] is a depth_anything model loaded on its own device (visp_hip_device_init(i) + visp_model_load);
 * the batch is cut into n_models contiguous shards (sizes differ by at most one), each shard runs on its model's device from
 * its own host thread, outputs land at the matching offsets of `out` [batch, h, w] f32. No collective is involved: images are
 * independent. (Per-device kernel attributes are set per (kernel, device), so several devices in one process are fine. Models that share
 * one visp_device share its compute stream: their shards take turns instead of running concurrently.) */
VISP_API int32_t visp_depthany_compute_sharded(visp_model* const* models, int32_t n_models, uint8_t const* rgb_u8, int32_t batch,
                                               int32_t w, int32_t h, float* out);
/* Overlapped host pipeline (the reference's benchmark loop -- upload, compute, download per call, tests/benchmark.cpp:55-91 --
 * with the transfers hidden): n_slots (2..8) slots of pinned staging + device buffers; submit() chains H2D (copy stream) ->
 * forward (the model's stream) -> D2H (second copy stream) by events and returns at once with a ticket; wait() blocks until
 * that batch's normalised depth maps [batch, h, w] f32 are in pinned host memory and returns them (valid until the slot is
 * reused, i.e. for n_slots - 1 further submits). input() = the next slot's pinned rgb buffer [batch, h, w, 3] to fill in
 * place (then submit(NULL)); submit(ptr) copies from pageable memory. One thread per pipeline. */
typedef struct visp_depthany_pipeline visp_depthany_pipeline;
VISP_API int32_t visp_depthany_pipeline_create(visp_model* m, int32_t batch, int32_t w, int32_t h, int32_t n_slots, visp_depthany_pipeline** out);
VISP_API void visp_depthany_pipeline_destroy(visp_depthany_pipeline* p);
VISP_API int32_t visp_depthany_pipeline_input(visp_depthany_pipeline* p, uint8_t** out_pinned);
VISP_API int32_t visp_depthany_pipeline_submit(visp_depthany_pipeline* p, uint8_t const* rgb_u8_or_null, int32_t* out_ticket);
VISP_API int32_t visp_depthany_pipeline_wait(visp_depthany_pipeline* p, int32_t ticket, float const** out_pinned);
/* capture the launch sequence of the current reserved shape into a hipGraph and replay it on
 * every later compute of that shape (enable = 0 turns it off) */
VISP_API int32_t visp_depthany_use_graph(visp_model* m, int32_t enable);
/* encoder schedule: -1 = auto (default: 1 where the model has the kernel's shape), 0 = one launch per op group, 1 = one attention
 * + one token-stationary block launch per layer (csrc/kernels_block16.hip; embed dim 384 / mlp 1536 / head dim 64 only).
 * Results agree to f16 rounding. */
VISP_API int32_t visp_depthany_set_schedule(visp_model* m, int32_t schedule);
/* sub-batches of one step on parallel HIP streams (parallel branches of the step's hipGraph): 0 = automatic (3 from batch 24, 2
 * from batch 8), 1 = none, up to 4. Results are bit-identical for every value (images are independent). */
VISP_API int32_t visp_depthany_set_split(visp_model* m, int32_t n);

/* Named intermediate tensors of the last compute, converted to f32 on the host (parity tests;
 * the reference's counterpart is the workbench capture, tests/workbench.cpp:754-760).
 * Names: tokens, layer_<i>, dino_layer_<i>, reassemble_<i>, neck_conv_<i>, fusion_<i>, head_conv1, depth.
 * Only available when captures were enabled before the compute. */
VISP_API int32_t visp_depthany_enable_captures(visp_model* m, int32_t enable);
VISP_API int32_t visp_depthany_read_capture(visp_model* m, char const* name, float* host_out, int64_t capacity,
                                            int64_t* n_written, int64_t shape[4]);

/* per-kernel-group timing of the last compute (HIP events on the compute stream); writes up to
 * cap entries, returns count via n. Only when enabled. */
typedef struct visp_timing { char name[32]; float ms; int32_t launches; double flops; double bytes; } visp_timing;
VISP_API int32_t visp_depthany_enable_timing(visp_model* m, int32_t enable);
VISP_API int32_t visp_depthany_read_timing(visp_model* m, visp_timing* out, int32_t cap, int32_t* n);

/* ---- ESRGAN extension (family 4; reference vision.h:284-304, vision.cpp:208-253) ---------------------------
 * visp_model_load / visp_model_compute work as in the reference (one image in, rgba_u8 at extent*scale out).
 * The batched entry points take B images of one extent and push all their tiles through the network together. */
typedef struct visp_esrgan_info { int32_t scale, n_blocks, n_filters, growth, tile_group; } visp_esrgan_info;
VISP_API int32_t visp_esrgan_get_info(visp_model const* m, visp_esrgan_info* out);
/* tiles per network pass (workspace bound / cache-locality knob); default 64 or $VISP_ESRGAN_TILE_GROUP */
VISP_API int32_t visp_esrgan_set_tile_group(visp_model* m, int32_t tiles);
VISP_API int32_t visp_esrgan_weights_arena(visp_model* m, void** device_ptr, size_t* n_bytes);
VISP_API int32_t visp_esrgan_weights_ready(visp_model* m);
/* tile_scale(tile_layout(extent, 224, 16), scale): out8 = image w,h, overlap x,y, n_tiles x,y, tile w,h (image.cpp:612-629) */
/* host-only: read a GGUF file completely (header, key/values, tensor infos, bounds of every tensor's data) as visp_model_load
 * does before it packs weights; 0 + error message if the file is malformed */
VISP_API int32_t visp_gguf_validate(char const* filepath, int32_t* out_n_tensors);
/* host-only image_scale of the reference (src/visp/image.cpp:328-356: stb_image_resize semantics, csrc/image_resize.cpp):
 * any supported format; the result is owned by *out_data (visp_image_destroy) */
VISP_API int32_t visp_image_scale(visp_image_view const* src, int32_t width, int32_t height, visp_image_view* out_image,
                                  visp_image_data** out_data);
/* host-only image_u8_to_f32 of the reference (src/visp/image.cpp:215-255, image-impl.h:17-34): dst = (src / 255 + offset) * scale per
 * channel, any u8 format -> the float format `format` (what *_process_input applies); result owned by *out_data */
VISP_API int32_t visp_image_u8_to_f32(visp_image_view const* src, int32_t format, float const offset[4], float const scale[4],
                                      visp_image_view* out_image, visp_image_data** out_data);
/* host-only image_normalize of the reference (src/visp/image.cpp:537-582): min-max of an alpha_f32 image mapped to [min, max]
 * (depthany_process_output); result owned by *out_data */
VISP_API int32_t visp_image_normalize(visp_image_view const* src, float min, float max, visp_image_view* out_image, visp_image_data** out_data);
VISP_API int32_t visp_esrgan_tile_layout(int32_t w, int32_t h, int32_t scale, int32_t out8[8]);
/* img: u8 [B,h,w,channels(format)] (rgba/bgra/argb/rgb), out: rgba_u8 [B, h*scale, w*scale, 4]; device pointers;
 * stream = hipStream_t or NULL (NULL: the device's stream, synchronised before returning) */
VISP_API int32_t visp_esrgan_compute_batch_device(visp_model* m, void const* img, int32_t batch, int32_t w, int32_t h, int32_t format,
                                                  void* out_rgba, void* stream);
VISP_API int32_t visp_esrgan_compute_batch_host(visp_model* m, uint8_t const* img, int32_t batch, int32_t w, int32_t h, int32_t format,
                                                uint8_t* out_rgba);
/* esrgan_generate (esrgan.cpp:55-79) on n rgb_f32 tiles [n,h,w,3] -> [n,h*scale,w*scale,3] (host buffers; for tests) */
VISP_API int32_t visp_esrgan_generate_host(visp_model* m, float const* rgb, int32_t n, int32_t w, int32_t h, float* out);
VISP_API int32_t visp_esrgan_enable_timing(visp_model* m, int32_t enable);
VISP_API int32_t visp_esrgan_read_timing(visp_model* m, visp_timing* out, int32_t cap, int32_t* n);

/* ---- MI-GAN extension (family 3; reference vision.h:257-279, vision.cpp:172-203, migan.cpp) ---------------------------
 * Loaded through visp_migan_load only: visp_model_load(.., VISP_MIGAN) and auto-detect keep refusing the family. A loaded handle
 * works with visp_model_compute(h, VISP_MIGAN, {image, mask}, 2, ..) (reference c-api.cpp:87-92) and is destroyed with
 * visp_model_destroy(h, VISP_MIGAN). */
typedef struct visp_migan_info { int32_t resolution, n_levels, channels[9]; } visp_migan_info; /* channels[i] at resolution >> i */
VISP_API int32_t visp_migan_load(char const* filepath, visp_device const* dev, visp_model** out);
VISP_API int32_t visp_migan_get_info(visp_model const* m, visp_migan_info* out);
/* migan_compute: image rgb/rgba u8 of any extent + alpha_u8 mask of the same extent -> rgba_u8 at that extent, alpha = mask */
VISP_API int32_t visp_migan_compute(visp_model* m, visp_image_view const* image, visp_image_view const* mask, visp_image_view* out_image,
                                    visp_image_data** out_data);
/* img u8 [B,res,res,channels] (3 or 4), mask u8 [B,res,res] -> rgba_u8 [B,res,res,4]; device pointers; stream = hipStream_t or NULL
 * (NULL: the device's stream, synchronised before returning). Replayed as a hipGraph per (batch, channels) after the first call. */
VISP_API int32_t visp_migan_compute_batch_device(visp_model* m, void const* img, int32_t channels, void const* mask, int32_t batch,
                                                 void* out_rgba, void* stream);
VISP_API int32_t visp_migan_compute_batch_host(visp_model* m, uint8_t const* img, int32_t channels, uint8_t const* mask, int32_t batch,
                                               uint8_t* out_rgba);
/* the generator on migan_process_input's f32 [n,res,res,4] -> rgb f32 [n,res,res,3] (host buffers; for tests) */
VISP_API int32_t visp_migan_generate_host(visp_model* m, float const* in4, int32_t n, float* out_rgb);
/* captures of the next computes: "enc.feat<r>", "enc.out", "syn.b<r>.x", "syn.b<r>.img" (computes run without the hipGraph) */
VISP_API int32_t visp_migan_enable_captures(visp_model* m, int32_t enable);
VISP_API int32_t visp_migan_read_capture(visp_model* m, char const* name, float* host_out, int64_t capacity, int64_t* n_written,
                                         int64_t shape[4]);
VISP_API int32_t visp_migan_enable_timing(visp_model* m, int32_t enable);
VISP_API int32_t visp_migan_read_timing(visp_model* m, visp_timing* out, int32_t cap, int32_t* n);

/* ---- YOLOv9t extension (reference src/visp/arch/yolov9t.cpp, src/cli/inference_yolov9t.cpp:300-405) ------------------------------
 * The reference never adds the family to model_family: visp_model_load and visp_model_detect_family keep refusing / ignoring a
 * "yolov9t" file; it loads through visp_yolov9t_load and is destroyed with visp_model_destroy. Inputs are rgb_u8 / rgba_u8 (alpha
 * ignored). Detections are in the pixel coordinates of the image given (detect) or of the S x S input (batch entries). */
typedef struct visp_detection { float x1, y1, x2, y2, confidence; int32_t class_id; float class_confidence; } visp_detection; /* detected_obj */
/* non_max_suppression's arguments; visp_yolov9t_nms_defaults gives the CLI's: conf 0.25, iou 0.45, max_det 300, max_nms 30000, max_wh 640.
 * Every (anchor, class) with score >= conf is a candidate (multi-label); ties of the score are ordered by (anchor, class). */
typedef struct visp_yolov9t_nms_params { float conf, iou; int32_t max_det, max_nms, max_wh; } visp_yolov9t_nms_params;
typedef struct visp_yolov9t_info { int32_t input_size, num_classes, reg_max, n_anchors; } visp_yolov9t_info; /* n_anchors at input_size */
VISP_API void visp_yolov9t_nms_defaults(visp_yolov9t_nms_params* out);
VISP_API int32_t visp_yolov9t_load(char const* filepath, visp_device const* dev, visp_model** out);
VISP_API int32_t visp_yolov9t_get_info(visp_model const* m, visp_yolov9t_info* out);
/* one image of any extent: letterbox to input_size, network, NMS, boxes scaled back to the image. params NULL = defaults.
 * Writes min(found, capacity) detections in score order and the number found to *n. */
VISP_API int32_t visp_yolov9t_detect(visp_model* m, visp_image_view const* image, visp_yolov9t_nms_params const* params, visp_detection* out,
                                     int32_t capacity, int32_t* n);
/* B images already letterboxed, u8 [B, size, size, channels] (3 or 4) -> out [B][max_det] detections in input pixels + counts [B].
 * size: a multiple of 32 from 64 up. The device form reads a device pointer (stream = hipStream_t or NULL) and returns host results;
 * the launch list is replayed as a hipGraph per (batch, size, channels, conf) after the first call. */
VISP_API int32_t visp_yolov9t_detect_batch_host(visp_model* m, uint8_t const* img, int32_t channels, int32_t batch, int32_t size,
                                                visp_yolov9t_nms_params const* params, visp_detection* out, int32_t* counts);
VISP_API int32_t visp_yolov9t_detect_batch_device(visp_model* m, void const* img, int32_t channels, int32_t batch, int32_t size,
                                                  visp_yolov9t_nms_params const* params, visp_detection* out, int32_t* counts, void* stream);
/* the network on f32 rgb [n, size, size, 3] in [0, 1] -> boxes f32 [n, A, 4] (xyxy, input pixels), scores f32 [n, A, nc] (host buffers) */
VISP_API int32_t visp_yolov9t_forward_host(visp_model* m, float const* rgb, int32_t n, int32_t size, float* boxes, float* scores);
/* host only: letterbox (rgb_u8 / rgba_u8 of any extent -> rgb_u8 [size, size, 3]) and NMS over dense boxes [A, 4] / scores [A, nc] */
VISP_API int32_t visp_yolov9t_letterbox(visp_image_view const* image, int32_t size, uint8_t* out_rgb, float* gain, float* pad_w, float* pad_h);
/* host only: scale_boxes (yolov9t.cpp:1255-1281) in place: (v - pad) / gain with the unrounded pads, clamped to [0, width] / [0, height] */
VISP_API int32_t visp_yolov9t_scale_boxes(visp_detection* dets, int32_t n, int32_t width, int32_t height, float gain, float pad_w, float pad_h);
/* the last batch call (detect, detect_batch_*) split in ms: {launch list on the device (HIP events), candidate readback, host NMS} */
VISP_API int32_t visp_yolov9t_last_split(visp_model const* m, float out_ms[3]);
VISP_API int32_t visp_yolov9t_nms(float const* boxes, float const* scores, int32_t n_anchors, int32_t nc, visp_yolov9t_nms_params const* params,
                                  visp_detection* out, int32_t capacity, int32_t* n);
/* captures of the next computes: "model.<i>" (i = 0..21), "detect.raw<l>", "boxes", "scores" (computes run without the hipGraph) */
VISP_API int32_t visp_yolov9t_enable_captures(visp_model* m, int32_t enable);
VISP_API int32_t visp_yolov9t_read_capture(visp_model* m, char const* name, float* host_out, int64_t capacity, int64_t* n_written,
                                           int64_t shape[4]);
VISP_API int32_t visp_yolov9t_enable_timing(visp_model* m, int32_t enable);
VISP_API int32_t visp_yolov9t_read_timing(visp_model* m, visp_timing* out, int32_t cap, int32_t* n);

/* ---- MobileSAM extension (family 0; reference vision.h:186-222, vision.cpp:26-92, mobile-sam.cpp) ----
 * visp_model_load / visp_model_compute work as in the reference: one image + 2 (point) or 4 (box) integer arguments in
 * pixels of that image -> alpha_u8 mask at the image's extent (sam_encode + sam_compute, c-api.cpp:34-52). A file
 * with only the enc.* tensors loads too; sam_compute then fails. */
/* sam_encode: any extent / u8 colour format; the embedding is kept on the device with the model */
VISP_API int32_t visp_sam_encode(visp_model* m, visp_image_view const* image);
/* embedding of the last visp_sam_encode: f32 [64, 64, 256] (rows, columns, channels), shape returned via shape[3] */
VISP_API int32_t visp_sam_read_embedding(visp_model* m, float* host_out, int64_t capacity, int64_t shape[3]);
/* sam_compute on the embedding of the last visp_sam_encode (several prompts per image, vision.cpp:54-92) */
VISP_API int32_t visp_sam_compute(visp_model* m, int32_t const* prompt, int32_t n_prompt, visp_image_view* out_image, visp_image_data** out_data);
/* test hook: mask logits [4][256][256] (f16-rounded; kept only while captures are enabled) and iou predictions [4] of the last sam_compute */
VISP_API int32_t visp_sam_read_masks(visp_model* m, float* masks, int64_t capacity, float iou[4]);
/* Many prompts on the embedding of the last visp_sam_encode in one batched pass (the prompt index folded into the rows of the decoder's launches).
 * prompts: host i32 [n][4] in pixels of the encoded image, a point uses entries 0 and 1, a box all four; n_args: host i32 [n], each 2 or 4 (points and
 * boxes may be mixed). Outputs are DEVICE pointers: masks_u8 [n][h][w] (0 / 255, h x w = the encoded image's extent), iou f32 [n][4] and chosen i32 [n]
 * (best of the first three masks by predicted iou, vision.cpp:80-82); iou and chosen may be NULL. The prompts run in chunks (visp_sam_set_prompt_chunk);
 * nothing in the call waits for the device, except that the first call (and one with a larger chunk or more prompts) allocates the workspace, and
 * that stream = NULL means the device's stream, synchronised before returning. With captures enabled the call synchronises per chunk.
 * All batch calls on one model share its workspace and its pinned token buffer: they must be ordered on ONE stream. A call on another stream while an
 * earlier one may still run is the caller's to order (an event between the streams); the library does not. */
VISP_API int32_t visp_sam_compute_batch_device(visp_model* m, int32_t const* prompts, int32_t const* n_args, int32_t n, void* masks_u8_dev, void* iou_dev,
                                               void* chosen_dev, void* stream);
/* the same with host outputs (masks u8 [n][h][w], iou f32 [n][4], chosen i32 [n]; iou and chosen may be NULL); blocks */
VISP_API int32_t visp_sam_compute_batch_host(visp_model* m, int32_t const* prompts, int32_t const* n_args, int32_t n, uint8_t* masks_u8, float* iou,
                                             int32_t* chosen);
/* extent in pixels of the image given to the last visp_sam_encode: what sizes the masks of the calls above */
VISP_API int32_t visp_sam_image_extent(visp_model* m, int32_t* width, int32_t* height);
/* prompts per internal chunk of the batch calls: 1 .. 256, default 64. It sizes the workspace: about 27 MB per prompt in flight. */
VISP_API int32_t visp_sam_set_prompt_chunk(visp_model* m, int32_t n);
/* Automatic mask generation: SAM's automatic mask generator (one crop layer, no crop-edge filter, no hole / island removal, no RLE) on n prompts in the
 * format of the batch calls above (at most 5461: three candidates per prompt, logit planes 0 .. 2, candidate = 3 * prompt + plane). A candidate is kept iff its
 * predicted iou > pred_iou_thresh and its stability score (logits > +offset over logits > -offset, counted on the decoder's 256^2 logits over the part of
 * the plane the image occupies) >= stability_thresh; the kept are ranked by predicted iou and de-duplicated by greedy NMS on the boxes of their positive
 * logits at nms_iou_thresh. The first min(kept, capacity) come out in rank order. Outputs are DEVICE pointers: masks_u8 [capacity][h][w] (0 / 255, the
 * arithmetic of the batch calls' masks), info_i32 [capacity][8] = {prompt, plane, x, y, w, h, area, 0} (box and area of the mask that came out, image
 * pixels), info_f32 [capacity][2] = {predicted_iou, stability_score}, counts i32 [2] = {returned, kept before the capacity cut}. Rows and masks at and
 * behind counts[0] are left untouched. The logits of all n prompts stay on the device for the call (0.5 MB per prompt). Waits for the host exactly where
 * visp_sam_compute_batch_device does (workspace growth, stream = NULL, captures), and shares its ordering rule: one stream per model. */
VISP_API int32_t visp_sam_generate_masks_device(visp_model* m, int32_t const* prompts, int32_t const* n_args, int32_t n, float pred_iou_thresh, float stability_thresh,
                                                float stability_offset, float nms_iou_thresh, int32_t capacity, void* masks_u8_dev, void* info_i32_dev,
                                                void* info_f32_dev, void* counts_dev, void* stream);
/* the same with host outputs; blocks */
VISP_API int32_t visp_sam_generate_masks_host(visp_model* m, int32_t const* prompts, int32_t const* n_args, int32_t n, float pred_iou_thresh, float stability_thresh,
                                              float stability_offset, float nms_iou_thresh, int32_t capacity, uint8_t* masks_u8, int32_t* info_i32, float* info_f32,
                                              int32_t* counts);
/* The generate calls with SAM's min_mask_region_area (postprocess_small_regions), all on the device. min_region_area = 0: exactly the launches and the bytes of
 * the entries above (counts [2] written). min_region_area > 0: the first k = min(kept, capacity) masks are produced exactly as above, then
 *  1. cleaned as visp_image_remove_small_regions_device cleans them (mode 3: holes, then islands, components below min_region_area pixels, 8-connectivity);
 *  2. area and box are taken again from the cleaned masks;
 *  3. a second greedy NMS runs over the k with SAM's scores, 1 for an unchanged mask and 0 for a changed one, equal scores in first-stage rank order (torchvision
 *     leaves that tie open), on the inclusive boxes of the cleaned masks in image pixels [x, y, x + w - 1, y + h - 1] ([0, 0, 0, 0] for an empty mask), with the
 *     arithmetic and the nms_iou_thresh of the first NMS;
 *  4. the survivors come out in SAM's order: unchanged masks first, then changed ones, each group by predicted iou. THIS IS NOT THE ORDER WITHOUT CLEANING.
 * info_i32 column 7 is 1 for a changed mask; counts i32 [4] = {returned, kept by the first NMS before the capacity cut, returned masks that cleaning changed,
 * masks the second NMS removed}. The first NMS still runs on the boxes of the logit grid (the difference from SAM stated above). Memory: the k masks are staged
 * on the device next to the logits (capacity * h * w bytes, 256 MB for 256 masks of 1024^2: the reordering needs them somewhere other than their final place)
 * and pass through a labelling workspace 64 masks at a time (8 bytes per pixel each, 512 MB at 1024^2). Waits for the host where the entries above do. */
VISP_API int32_t visp_sam_generate_masks_clean_device(visp_model* m, int32_t const* prompts, int32_t const* n_args, int32_t n, float pred_iou_thresh,
                                                      float stability_thresh, float stability_offset, float nms_iou_thresh, int32_t capacity, int32_t min_region_area,
                                                      void* masks_u8_dev, void* info_i32_dev, void* info_f32_dev, void* counts_dev, void* stream);
/* the same with host outputs (counts i32 [4]; with min_region_area = 0 only its first two are written); blocks */
VISP_API int32_t visp_sam_generate_masks_clean_host(visp_model* m, int32_t const* prompts, int32_t const* n_args, int32_t n, float pred_iou_thresh, float stability_thresh,
                                                    float stability_offset, float nms_iou_thresh, int32_t capacity, int32_t min_region_area, uint8_t* masks_u8,
                                                    int32_t* info_i32, float* info_f32, int32_t* counts);
/* diagnostics, as visp_sam_generate_last_split: its four figures and a fifth, the cleaning stage of the last call (0 without one); and that stage alone as
 * {clean, records + second NMS, gather} */
VISP_API int32_t visp_sam_generate_last_split5(visp_model const* m, float out_ms[5]);
VISP_API int32_t visp_sam_generate_last_clean_split(visp_model const* m, float out_ms[3]);
/* diagnostics: with visp_sam_enable_timing on, a generate call records events around its stages and waits for them; this reads the last call's
 * {decode, scoring, rank + NMS, output masks and their records} in ms */
VISP_API int32_t visp_sam_generate_last_split(visp_model const* m, float out_ms[4]);
/* SAM's defaults: {pred_iou_thresh 0.88, stability_thresh 0.95, stability_offset 1.0, nms_iou_thresh 0.7} */
VISP_API int32_t visp_sam_generate_defaults(float out[4]);
/* test hook, the batch twin of visp_sam_read_masks: with captures enabled, the f16-rounded logit planes [n][4][256][256] and (iou nullable) the iou
 * predictions [n][4] of the last batch or generate call; capacity in floats of `logits` */
VISP_API int32_t visp_sam_read_masks_batch(visp_model* m, float* logits, int64_t capacity, float* iou);
/* rgb: u8 [B, 1024, 1024, 3] already at the model extent -> out f32 [B, 64, 64, 256]; device pointers;
 * stream = hipStream_t or NULL (NULL: the device's stream, synchronised before returning) */
VISP_API int32_t visp_sam_encode_batch_device(visp_model* m, void const* rgb, int32_t batch, void* out, void* stream);
VISP_API int32_t visp_sam_encode_batch_host(visp_model* m, uint8_t const* rgb, int32_t batch, float* out);
/* opt-in, never the default (BASELINE.json configs[4]: "fp8 GGUF weights on CDNA4 fp8 MFMA"; the reference has no fp8 type): the MLPs of the transformer
 * stages run on the block-scaled e4m3 matrix instruction -- weights quantised per output channel (on first use, from the f16 weights), activations per
 * token. Changes the embedding by several percent of its scale (tests/test_fp8_decision.py, tests/test_gpu_tinyvit.py): a measurement, not a recommendation. */
VISP_API int32_t visp_sam_set_fp8_mlp(visp_model* m, int32_t enable);
VISP_API int32_t visp_sam_weights_arena(visp_model* m, void** device_ptr, size_t* n_bytes);
VISP_API int32_t visp_sam_weights_ready(visp_model* m);
/* test hook as for depth_anything: "patch_embed", "layer_0" .. "layer_3" = the stage outputs of the last batch, f16 -> f32 */
VISP_API int32_t visp_sam_enable_captures(visp_model* m, int32_t enable);
VISP_API int32_t visp_sam_read_capture(visp_model* m, char const* name, float* host_out, int64_t capacity, int64_t* n_written, int64_t shape[4]);
VISP_API int32_t visp_sam_enable_timing(visp_model* m, int32_t enable);
VISP_API int32_t visp_sam_read_timing(visp_model* m, visp_timing* out, int32_t cap, int32_t* n);

/* ---- BiRefNet (family 1; reference src/visp/arch/birefnet.cpp, vision.cpp:98-132): visp_model_load + visp_model_compute run
 * birefnet_compute (any 8-bit colour image -> alpha_u8 mask at its extent). Batched extension: rgb_u8 [batch, h, w, 3] at the
 * model extent (visp_birefnet_image_extent; multiples of 64) -> sigmoid mask f32 [batch, h, w]. */
VISP_API int32_t visp_birefnet_image_extent(visp_model* m, int32_t w, int32_t h, int32_t* out_w, int32_t* out_h);
VISP_API int32_t visp_birefnet_compute_batch_device(visp_model* m, void const* rgb_u8, int32_t batch, int32_t w, int32_t h, void* mask_f32, void* stream);
VISP_API int32_t visp_birefnet_compute_batch_host(visp_model* m, uint8_t const* rgb_u8, int32_t batch, int32_t w, int32_t h, float* mask);
/* The cutout: visp_birefnet_compute_batch_* as it stands, then the foreground estimator (visp_image_estimate_foreground_batch_device, below) on the mask
 * where it lies on the device -- what the reference's `vision-cli birefnet --composite` makes on the host (src/cli/cli.cpp:327-347). rgb_u8 [batch, h, w, 3]
 * at the model extent -> rgba_u8 [batch, h, w, 4], alpha = the mask; radius as for the estimator (the reference's default is 30). stream as above.
 * visp_model_compute for the family keeps returning the mask. */
VISP_API int32_t visp_birefnet_cutout_batch_device(visp_model* m, void const* rgb_u8, int32_t batch, int32_t w, int32_t h, int32_t radius, void* rgba_u8_out, void* stream);
VISP_API int32_t visp_birefnet_cutout_batch_host(visp_model* m, uint8_t const* rgb_u8, int32_t batch, int32_t w, int32_t h, int32_t radius, uint8_t* rgba_u8_out);
/* one 8-bit colour image of any extent -> rgba_u8 cutout at that extent: the mask as visp_model_compute makes it (kept in f32), then the estimator on the
 * caller's own pixels; result owned by *out_data */
VISP_API int32_t visp_birefnet_cutout(visp_model* m, visp_image_view const* image, int32_t radius, visp_image_view* out_image, visp_image_data** out_data);

/* ---- matting image ops (reference include/visp/image.h:141-170, src/visp/image.cpp:290-323, 358-535) ------------------------------------------------
 * Host views in (the row stride is honoured), a library-owned image out (visp_image_destroy). The four that compute run on `dev`; dev == NULL means the
 * calling thread's current HIP device. Every argument check -- null, format, extent mismatch, radius -- happens before anything touches a device. */
/* image_blur: box filter of size 2 radius + 1, edges replicated; alpha_f32 or rgba_f32; 1 <= radius <= min(w, h) / 2. Every output sums its own window:
 * the reference's running sum along the whole row is not reproduced (its error grows with the row) */
VISP_API int32_t visp_image_blur(visp_device const* dev, visp_image_view const* src, int32_t radius, visp_image_view* out_image, visp_image_data** out_data);
/* image_erosion: minimum over the clamped (2 radius + 1)^2 neighbourhood; alpha_u8 or alpha_f32; bit-exact; 1 <= radius <= 64 */
VISP_API int32_t visp_image_erosion(visp_device const* dev, visp_image_view const* src, int32_t radius, visp_image_view* out_image, visp_image_data** out_data);
/* SAM's remove_small_regions on n u8 masks [n][h][w] in place, for masks from visp_sam_compute_batch_device, BiRefNet or anywhere else. A pixel is foreground iff
 * its byte is non-zero; 8-connectivity; a component is small iff it has fewer than min_area (>= 0) pixels. mode VISP_REGIONS_HOLES (1): every small component of
 * the background becomes 255, none exempt for touching the border; VISP_REGIONS_ISLANDS (2): every small component of the foreground becomes 0, but where every
 * one is small the largest stays (of equal ones the one whose first pixel in row-major order comes first); VISP_REGIONS_BOTH (3): the holes, then the islands of
 * the result (SAM's order: a filled hole can join two small islands into one that stays). Only flipped pixels are written. changed i32 [n] (nullable): 1 where a
 * pixel of the mask flipped. masks and changed are DEVICE pointers; stream NULL = the stream of `dev`; dev NULL = the calling thread's current device. The
 * labelling workspace (8 bytes per pixel and mask in flight, at most 256 MB) is allocated per CALL and freed behind a synchronisation: the call returns with
 * the work done. Every argument check happens before anything touches a device. */
#define VISP_REGIONS_HOLES 1
#define VISP_REGIONS_ISLANDS 2
#define VISP_REGIONS_BOTH 3
VISP_API int32_t visp_image_remove_small_regions_device(void* masks_u8_dev, int32_t n, int32_t w, int32_t h, int32_t min_area, int32_t mode, void* changed_i32_dev,
                                                        void* stream, visp_device const* dev);
/* the same on host arrays: up, clean, down; blocks */
VISP_API int32_t visp_image_remove_small_regions_host(uint8_t* masks_u8, int32_t n, int32_t w, int32_t h, int32_t min_area, int32_t mode, int32_t* changed_i32,
                                                      visp_device const* dev);
/* image_estimate_foreground: image rgba_f32, mask alpha_f32 of the same extent -> rgba_f32 foreground colours, alpha = mask. Two blur-fusion stages, radius
 * (the reference's default: 30) then 3; radius <= min(w, h) / 2, extent at least 6x6 */
VISP_API int32_t visp_image_estimate_foreground(visp_device const* dev, visp_image_view const* image, visp_image_view const* mask, int32_t radius,
                                                visp_image_view* out_image, visp_image_data** out_data);
/* image_alpha_composite: fg rgba_u8, bg rgb_u8 or rgba_u8, mask alpha_u8 -> rgba_u8 = trunc((w fg + (1 - w) bg) * 255), w = mask / 255, alpha 255 */
VISP_API int32_t visp_image_alpha_composite(visp_device const* dev, visp_image_view const* fg, visp_image_view const* bg, visp_image_view const* mask,
                                            visp_image_view* out_image, visp_image_data** out_data);
/* host only. image_set_alpha: a copy of img (rgba_u8 / bgra_u8 / argb_u8) with its alpha channel, by the format's channel map, taken from alpha (alpha_u8) */
VISP_API int32_t visp_image_set_alpha(visp_image_view const* img, visp_image_view const* alpha, visp_image_view* out_image, visp_image_data** out_data);
/* host only. image_to_mask: the first channel of every pixel of a u8 image as alpha_u8 */
VISP_API int32_t visp_image_to_mask(visp_image_view const* src, visp_image_view* out_image, visp_image_data** out_data);
/* the estimator on device-resident batches: img [batch, h, w] pixels of img_format (VISP_RGBA_F32, or VISP_RGB_U8 / VISP_RGBA_U8 read directly: no f32 copy
 * of the image is made), mask f32 [batch, h, w] -> out [batch, h, w, 4] of out_format (VISP_RGBA_F32 or VISP_RGBA_U8). stream = hipStream_t or NULL (the
 * device's stream). The workspace (64 bytes per pixel) lives for the call: the stream is synchronised before it returns. */
VISP_API int32_t visp_image_estimate_foreground_batch_device(visp_device const* dev, void const* img, int32_t img_format, void const* mask_f32, int32_t batch,
                                                             int32_t w, int32_t h, int32_t radius, void* out, int32_t out_format, void* stream);

/* ---- SWIN encoder, the backbone of BiRefNet (reference src/visp/arch/swin.cpp, swin_encode) ---------
 * The encoder of a birefnet GGUF (tensors bb.*, KV swin.embed_dim) on its own: visp_swin_load reads only the backbone; the
 * visp_swin_* calls also accept a full birefnet model handle. Destroyed with visp_model_destroy(m, VISP_BIREFNET). */
VISP_API int32_t visp_swin_load(char const* filepath, visp_device const* dev, visp_model** out);
/* dims[3 i .. 3 i + 2] = {w_i, h_i, C_i} of output i for an image of extent (w, h) (swin.cpp:229-262) */
VISP_API int32_t visp_swin_output_dims(visp_model* m, int32_t w, int32_t h, int32_t dims[12]);
/* rgb_u8 [batch, h, w, 3] (device) -> outs[i] f32 [batch, h_i, w_i, C_i] (device; NHWC = the reference's CWHN result tensors):
 * birefnet_process_input's normalisation (birefnet.cpp:259-270) + swin_encode. w, h multiples of 32. stream = hipStream_t or
 * NULL (NULL: the device's stream, synchronised before returning). */
VISP_API int32_t visp_swin_encode_batch_device(visp_model* m, void const* rgb_u8, int32_t batch, int32_t w, int32_t h, void* const outs[4],
                                               void* stream);
VISP_API int32_t visp_swin_encode_batch_host(visp_model* m, uint8_t const* rgb_u8, int32_t batch, int32_t w, int32_t h, float* const outs[4]);
/* test hooks as for the other families: "patch_embed", "block_<layer>_<i>" (f16 -> f32), per-kernel-group timing */
/* Shift-mask semantics of the window attention. 0 (default) = the reference as written: swin::layer passes the layer's attn_mask to
 * every block and swin::block forwards it unconditionally (swin.cpp:128-139, 226-237), so the edge windows of UNSHIFTED blocks are
 * masked too. 1 = shifted blocks only, as the reference's torch twin / the original Swin (tests/test_birefnet.py:249-255). */
VISP_API int32_t visp_swin_set_mask_mode(visp_model* m, int32_t shifted_only);
VISP_API int32_t visp_swin_enable_captures(visp_model* m, int32_t enable);
VISP_API int32_t visp_swin_read_capture(visp_model* m, char const* name, float* host_out, int64_t capacity, int64_t* n_written, int64_t shape[4]);
VISP_API int32_t visp_swin_enable_timing(visp_model* m, int32_t enable);
VISP_API int32_t visp_swin_read_timing(visp_model* m, visp_timing* out, int32_t cap, int32_t* n);

/* ---- graph layer: the executor boundary the reference's arch code is written against -----------------------------------------------------------
 * replaces include/visp/ml.h:154-256 (compute_graph, compute_graph_init / _allocate, compute, model_ref::weights / find, compute_graph_input /
 * _output, transfer_to_backend / transfer_from_backend) and the builders of src/visp/nn.h + ml.cpp:746-788, which the reference implements on
 * ggml (ggml_new_tensor / ggml_mul_mat / ggml_add / ... / ggml_gallocr / ggml_backend_graph_compute). A tensor handle is an index into its
 * graph (>= 0); shapes are ggml's ne order (ne[0] contiguous). include/visp/ml.h is the C++ face of these entries (model_ref, tensor, the
 * nn.h builder names). One generic entry adds a node: `op` is a visp_graph_op, `src` the operand handles, `iparams` / `fparams` its integer
 * and float arguments (listed per op below). */
typedef struct visp_graph visp_graph;
typedef struct visp_weights visp_weights; /* model_weights (ml.h:126-149): tensors by name + their packed device images, shared by the graphs over them */
enum visp_graph_op {
    VISP_OP_LINEAR = 2,            /* src x, w [K,N], (b)                                  nn.cpp:6-12 */
    VISP_OP_LAYER_NORM = 3,        /* src x, w, b; f0 eps                                  nn.cpp:14-19 */
    VISP_OP_GELU = 4, VISP_OP_RELU = 5,
    VISP_OP_SCALE = 6,             /* f0 factor */
    VISP_OP_ADD = 7, VISP_OP_MUL = 8, /* second operand broadcast over trailing dimensions, or a plane [1, W, H, 1] on [C, W, H, N] */
    VISP_OP_CONV_2D = 9,           /* src x [C,W,H,N], w [Cin,kw,kh,Cout], (b); i0 stride, i1 pad        nn.cpp:72-100 */
    VISP_OP_CONV_TRANSPOSE_2D = 10,/* src x, w [kw,kh,Cout,Cin], (b); i0 stride (== kernel)               nn.cpp:117-129 */
    VISP_OP_INTERPOLATE = 11,      /* i0 w, i1 h, i2 mode: 1 bilinear, 2 bicubic, | 256 align_corners     ml.cpp:782-788 */
    VISP_OP_ATTENTION = 12,        /* src q, k, v [head_dim, heads, tokens, batch]; f0 scale               nn.cpp:210-244 */
    VISP_OP_CONCAT = 13,           /* src a, b; i0 dim                                                      ml.cpp:770-780 */
    VISP_OP_SLICE = 14,            /* i[3d], i[3d+1], i[3d+2] = begin, end, step of dimension d            ml.cpp:746-768 */
    VISP_OP_RESHAPE = 15,          /* i0..i3 ne */
    VISP_OP_REPEAT = 16,           /* i0..i3 ne: a source dimension is 1 or equal; a CONSTANT source may be tiled (every target extent a multiple of the
                                    * source's, out[i] = src[i mod ne_src] as ggml_repeat defines it), folded on the host          dino.cpp:38-40, sam3.h:331-334 */
    VISP_OP_PATCH_EMBED = 17,      /* src x f32 [C,W,H,N], w, (b); i0 patch size                           nn.cpp:166-180 */
    VISP_OP_CONT = 18,
    /* extensions for callers that keep images in HBM (the reference does both steps on the host): */
    VISP_OP_IMAGE_U8_TO_F32 = 19,  /* src x u8 input [3,W,H,N]; f0..f2 mean, f3..f5 1/std: (x / 255 - mean) / std        image.cpp:215-255 */
    VISP_OP_IMAGE_NORMALIZE = 20,  /* src x f32 [1,W,H,N]: per-image min-max to [0, 1]                                   image.cpp:537-582 */
    VISP_OP_LEAKY_RELU = 21,       /* f0 negative slope                                                                    ggml_leaky_relu, esrgan.cpp:17, 24 */
    /* the window ops of a SWIN block (swin.cpp:48-141); all of them are folded on the host when every operand is a constant */
    VISP_OP_PERMUTE = 22,          /* i0..i3 ggml_permute's axes (source dimension d becomes dimension i_d); the result is contiguous, cont behind it a view */
    VISP_OP_ROLL = 23,             /* i0..i3 cyclic shifts, negative allowed                                               ggml_roll, swin.cpp:116, 124 */
    VISP_OP_PAD = 24,              /* i0..i3 zeros appended at the end of each dimension                                   ggml_pad, swin.cpp:111 */
    /* src table [C, rows] (a constant, f16 / f32), index i32 -> [C, idx ne0, ne1, ne2]. A constant index is folded on the host and gives f32, as ggml says. An
     * index that is an i32 GRAPH INPUT (the token ids of clip_text_embed) is gathered on the device and gives an f16 ACTIVATION -- ggml says f32 there too, but
     * activations of this layer are f16; C a multiple of 8. An index outside the table reads nothing and gives a row of zeros.   ggml_get_rows, swin.cpp:75, sam3.h:225 */
    VISP_OP_GET_ROWS = 25,
    VISP_OP_CAST = 26,             /* i0 type (0 f32, 1 f16): rounds constants, a view on activations that have the type   ggml_cast, swin.cpp:78 */
    /* src q, k, v [head_dim, heads, T, B], mask [T_k, T_q, Hm, Bm] f16 / f32, constant or activation; f0 scale. Hm is 1 or heads, Bm divides B (batch b
     * reads mask b % Bm). softmax(scale q k^T + mask) v as the 3-source op. head_dim 32 and 64, T_q == T_k. head_dim 32 exists through THIS op only:
     * VISP_OP_ATTENTION keeps its head_dim-64 kernel and its refusal of everything else.                         nn.cpp:210-244, swin.cpp:69-97 */
    VISP_OP_ATTENTION_MASKED = 27,
    /* the nodes of a BiRefNet decoder block (birefnet.cpp:79-145) */
    /* src x [Cin, W, H, N] f16, w [Cin, kw, kh, Cout] (a constant, stored as conv_2d stores it), offset [2 kh kw, OW, OH, N], (mask [kh kw, OW, OH, N]); i0 stride,
     * i1 pad. Offset channel 2t is dy, 2t + 1 is dx of tap t = ky kw + kx. A sample at (py, px) counts only inside (-1, H) x (-1, W), corners outside the map are
     * zero: the convention of the oracle's vo_deform_conv2d_nhwc, pinned on grid_sample and NOT on torchvision (the parity caveat of
     * tests/test_oracle_birefnet.py:1-10 carries over). Built for stride 1, kw == kh <= 7, Cin % 16 == 0, Cout % 8 == 0 and <= 256; anything else is refused
     * when the node is made. With the default fused models the group conv_2d(offset, x), scale(sigmoid(conv_2d(modulator, x)), s), conv_2d_deform [, mul(c),
     * add(c), relu] is two launches (kernels_deform.hip).                                                                  nn.cpp:131-148, birefnet.cpp:83-92 */
    VISP_OP_CONV_2D_DEFORM = 28,
    VISP_OP_SIGMOID = 29,          /* element-wise on f16 activations; folded on the host on constants                     ggml_sigmoid, birefnet.cpp:86 */
    VISP_OP_MEAN_2D = 30,          /* x [C, W, H, N] -> [C, 1, 1, N]: f32 sums in a fixed order, no atomics (the same bits every launch). NOT ggml_mean, which
                                      reduces ne[0] -- here the channel                                                    mean_2d, birefnet.cpp:93-100 */
    /* src x [C, W, H, N] f16, kernel (a constant) as [C, 1, kw, kh] (the NHWC form of TinyViT's local_conv) or [1, kw, kh, C] (a depthwise OIHW kernel listed in
     * conv2d_weights), (bias [C], a constant); i0 stride (1 or 2), i1 pad. -> [C, (W + 2 pad - kw) / stride + 1, (H + 2 pad - kh) / stride + 1, N], floor division,
     * even kernels like odd ones (4x4 at pad 2 gives W + 1 columns). Built for kw == kh <= 7, pad <= k - 1, C % 8 == 0; anything else is refused when the node is
     * made. One launch (kernels_dwconv.hip); with the default fused models a gelu / leaky_relu that is its only reader joins it.
     *                                                                                                        nn.cpp:102-115, mobile-sam.cpp:20-23, migan.cpp:28-57 */
    VISP_OP_CONV_2D_DEPTHWISE = 31,
    /* the ggml calls of YOLOv9t (yolov9t.cpp) beyond nn.h. With the default fused models a silu that is the only reader of a conv_2d / linear is that launch's
     * epilogue, silu(add(conv3x3(x), conv1x1(x))) is one 3x3 launch on folded weights, channel slices and channel concats of such maps are read and written
     * in place, and slice -> reshape [n, 4, A, N] -> soft_max -> mul(c [n]) -> sum_rows is one launch. */
    VISP_OP_SILU = 32,             /* x / (1 + exp(-x)), element-wise on f16 activations; folded on the host on constants          ggml_silu, yolov9t.cpp:124 */
    /* x [C, W, H, N] f16; i0 kind (ggml's values: 0 max, 1 avg), i1, i2 kernel w, h, i3, i4 stride w, h, i5, i6 pad w, h -> [C, (W + 2 pad - k) / stride + 1, .., N],
     * floor division. Max: positions outside the map never win. Built: square kernels 1..13, equal strides 1 or 2, pad <= k / 2, C % 8 == 0; average with
     * pad > 0 is refused (the reference never builds it, and ggml's divisor there is a convention of its own).      ggml_pool_2d, yolov9t.cpp:171-177, 461 */
    VISP_OP_POOL_2D = 33,
    VISP_OP_SOFT_MAX = 34,         /* over dimension 0, the row maximum subtracted; ne[0] a multiple of 8, at most 1024             ggml_soft_max, yolov9t.cpp:681 */
    VISP_OP_SUM_ROWS = 35,         /* [n, a, b, c] -> [1, a, b, c]: f32 sum in a fixed order                                        ggml_sum_rows, yolov9t.cpp:687 */
    VISP_OP_SUB = 36,              /* a - b, b broadcast as for ADD (the operands are not swapped)                                  ggml_sub, yolov9t.cpp:644 */
    /* the nodes of MI-GAN (migan.cpp) beyond the above. f0 lower bound, f1 upper bound: min(max(x, f0), f1) on f16 activations, folded on the host on
     * constants; refused when f0 > f1 or a bound is not finite. ADD / MUL / SUB also take a second operand [1, W, H, 1] on a first operand [C, W, H, N] (one value
     * per pixel, for every channel and image: migan.cpp:40, 76), and CONV_2D reads an f32 image of 4 channels as it reads one of 3. With the default fused
     * models leaky_relu -> scale -> clamp joins the convolution in front of it, and interpolate(x2 NEAREST) -> mul(zero-insertion tile) -> depthwise 4x4 pad 2 ->
     * slice -> cont is one polyphase FIR launch.                                          ggml_clamp, migan.cpp:23 */
    VISP_OP_CLAMP = 37,
    /* the nodes of the SAM prompt encoder and mask decoder (mobile-sam.cpp:210-478) beyond the above.
     * src q [head_dim, heads, T_q, B], k, v [head_dim, heads, T_k, B], f16 activations; f0 scale -> [head_dim * heads, T_q, B] = softmax(scale q k^T) v, what
     * nn.cpp:210-244 computes without a mask. head_dim 16, 32 and 64, any T_q, T_k >= 1; other head_dims, shapes that do not match and non-f16 operands are
     * refused when the node is made. One launch on q, k, v where they are (no head-major copies); with T_q <= 32 and T_k >= 256 the keys are split over blocks
     * and a second launch folds the parts in a fixed order. VISP_OP_ATTENTION and VISP_OP_ATTENTION_MASKED keep their kernels and
     * their refusals. */
    VISP_OP_ATTENTION_CROSS = 38,
    /* ggml_mul_mat: a [K, M, Ba], b [K, N, B] -> [M, N, B], Ba 1 or B. Folded on the host when both are constants. On the device: two f16 activations with
     * K % 8 == 0, K <= 256, N <= 16 (one launch), and a constant a with K == 2 on an f32 graph input b as the head of mul_mat -> scale -> {sin, cos} ->
     * concat(dim 0), which is one launch (position_embedding_random, mobile-sam.cpp:238-248). Everything else is refused; with a constant a, LINEAR is the
     * op to use.                                                                                                            mobile-sam.cpp:243, 471 */
    VISP_OP_MUL_MAT = 39,
    VISP_OP_SIN = 40,              /* element-wise on f16 activations, f32 inside; folded on the host on constants             ggml_sin, mobile-sam.cpp:245 */
    VISP_OP_COS = 41,              /* likewise                                                                                 ggml_cos, mobile-sam.cpp:246 */
    /* the node of the SAM3 vision encoder beyond the above: ggml_rope_ext in GGML_ROPE_TYPE_NORMAL (sam3.h:413-438). src x [n, heads, T, B] (an f16 activation),
     * pos i32 CONSTANT [T] (visp_graph_add_weight with dtype 26, like a get_rows index); i0 n_dims (== n, a multiple of 8), i1 mode (0, NORMAL, only); f0
     * freq_base, f1 freq_scale. For pair i in [0, n / 2): theta = pos[t] * freq_scale * freq_base^(-2 i / n); out[2i] = x[2i] cos - x[2i+1] sin, out[2i+1] =
     * x[2i] sin + x[2i+1] cos. The result has x's shape, f16. The angles never go through device transcendentals: the lowering makes a cos | sin table in double
     * from the constant positions, once per (positions, n_dims, base, scale). apply_rope_2d is two ROPE nodes on the two halves of a head. */
    VISP_OP_ROPE = 42,
    /* the node of BiRefNet's decoder beyond the above: image_to_patches (birefnet.cpp:153-162) as ONE op, since the reference's reshape / permute chain lives in
     * WHCN, which this layer keeps only as views. src an f32 image [C, W, H, N] with C <= 4 (the graph input, or INTERPOLATE of it: INTERPOLATE takes such an image
     * in mode bilinear | align_corners and gives an f32 image every reader of the input takes); i0 = w, i1 = h. The result is f16 [gw gh C, w, h, N] with gw = W / w,
     * gh = H / h: channel gx + gw (gy + gh c) of pixel (py, px) is image (gy h + py, gx w + px, c). w and h divide the image; gw gh C is a multiple of 8. */
    VISP_OP_IMAGE_PATCHES = 43
};
/* every f16 / f32 tensor of the file becomes a weight (model_load + model_transfer, ml.cpp:206-217, 449-516); conv kernels listed in
 * <arch>.conv2d_weights of a whcn file are presented as [Cin,kw,kh,Cout]. Device images are made when a graph that uses a tensor is
 * allocated, once per (tensor, role), and are reused by later graphs over the same weights. */
VISP_API int32_t visp_weights_load(char const* gguf_path, visp_weights** out);
/* model_file (ml.h:85-103; ml.cpp:206-281): a GGUF file read into memory, its key/values by name. get_int needs an i32 value, the array
 * getter an i32 array of exactly n entries (the reference's rules); a missing key is an error naming it. */
typedef struct visp_file visp_file;
VISP_API int32_t visp_file_load(char const* gguf_path, visp_file** out);
VISP_API void visp_file_destroy(visp_file* f);
VISP_API int32_t visp_file_n_tensors(visp_file const* f, int64_t* out);
VISP_API int32_t visp_file_get_int(visp_file const* f, char const* key, int32_t* out);
VISP_API int32_t visp_file_get_int_array(visp_file const* f, char const* key, int32_t* out, int64_t n);
VISP_API int32_t visp_file_get_string(visp_file const* f, char const* key, char* out, int64_t capacity, int64_t* needed);
VISP_API int32_t visp_weights_from_file(visp_file const* f, visp_weights** out); /* model_transfer: the file's tensors as model weights */
VISP_API int32_t visp_weights_create(visp_weights** out);
VISP_API int32_t visp_weights_add(visp_weights* w, char const* name, int32_t dtype, int64_t const ne[4], float const* data);
VISP_API void visp_weights_destroy(visp_weights* w); /* graphs over the weights keep them alive */
/* compute_graph_init (ml.cpp:531-543). weights == NULL: the graph starts with an empty store of its own (visp_graph_add_weight) */
VISP_API int32_t visp_graph_create(visp_weights* weights, visp_graph** out);
VISP_API void visp_graph_destroy(visp_graph* g);
/* dtype 0 f32 / 1 f16: `data` f32 values. dtype 26 (i32): `data` points at int32 values -- an index constant for VISP_OP_GET_ROWS. Also how a caller adds
 * a constant that is not a file weight (the shift mask of swin.cpp:165-221, -inf entries included); visp_graph_get_tensor finds it by name. */
VISP_API int32_t visp_graph_add_weight(visp_graph* g, char const* name, int32_t dtype, int64_t const ne[4], float const* data, int32_t* out);
VISP_API int32_t visp_graph_find_weight(visp_graph* g, char const* name, int32_t* out); /* *out = -1 when absent (model_ref::find) */
VISP_API int32_t visp_graph_input(visp_graph* g, int32_t dtype /* 0 f32, 1 f16, 24 u8 image bytes, 26 i32 indices */, int64_t const ne[4], char const* name, int32_t* out);
VISP_API int32_t visp_graph_op(visp_graph* g, int32_t op, int32_t const* src, int32_t n_src, int64_t const* iparams, int32_t n_iparams,
                               float const* fparams, int32_t n_fparams, int32_t* out);
VISP_API int32_t visp_graph_set_name(visp_graph* g, int32_t tensor, char const* name);
VISP_API int32_t visp_graph_get_tensor(visp_graph* g, char const* name, int32_t* out); /* ggml_get_tensor; -1 when absent */
VISP_API int32_t visp_graph_output(visp_graph* g, int32_t tensor, char const* name);
VISP_API int32_t visp_graph_tensor_info(visp_graph const* g, int32_t tensor, int32_t* dtype, int64_t ne[4], int32_t* is_constant);
/* constants (weights and everything folded from them): their f32 values */
VISP_API int32_t visp_graph_read_constant(visp_graph const* g, int32_t tensor, float* out, int64_t capacity);
/* compute_graph_allocate (ml.cpp:545-552): lower to launches, pack the weights the graph uses, plan + allocate the arena on `dev`.
 * dev == NULL: lower and plan only -- no device work (visp_graph_describe shows the launch list and the arena size) */
VISP_API int32_t visp_graph_allocate(visp_graph* g, visp_device const* dev);
/* before visp_graph_allocate. 1 (default): the lowering may replace whole node groups by the kernels written for them -- the dino::layer group
 * (embed 384 / mlp 1536 / heads of 64) by attention + one token-stationary block launch on an f32 residual stream, 3x3 convs by the LDS-ring conv,
 * interpolate -> conv by the resizing halo loader, interpolate -> conv 1x1 by projection-then-resize, a sliced GEMM operand by row addressing.
 * 0: one launch per epilogue-fused node on f16 activations. */
VISP_API int32_t visp_graph_set_fused_models(visp_graph* g, int32_t enable);
VISP_API int32_t visp_graph_use_hip_graph(visp_graph* g, int32_t enable); /* replay the launch list as one hipGraph from the second compute on */
VISP_API int32_t visp_graph_compute(visp_graph* g);   /* blocking (ml.cpp:559-562) */
VISP_API int32_t visp_graph_tensor_set(visp_graph* g, int32_t tensor, void const* data, size_t n_bytes);
VISP_API int32_t visp_graph_tensor_get(visp_graph* g, int32_t tensor, void* data, size_t n_bytes, int32_t as_f32);
/* one line per launch, then "launches=.. arena_bytes=.. unshared_bytes=.. constant_bytes=.."; returns the length needed */
VISP_API int32_t visp_graph_describe(visp_graph const* g, char* out, int64_t capacity, int64_t* needed);

#ifdef __cplusplus
}
#endif
#endif
