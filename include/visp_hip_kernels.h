/*
 * visp_hip_kernels.h -- thin C ABI between the host C++ of the backend and its HIP
 * translation units (gfx950 / MI355X only). Host code never includes HIP headers; every
 * pointer below is a device pointer unless it says "host", `stream` is a hipStream_t.
 *
 * Each launcher replaces the ggml ops the reference's graph emits for the Depth-Anything
 * path; the reference call sites are cited per entry.
 * All functions return 1 on success and 0 on error (message via vx_last_error()), the
 * convention of the reference's C API (src/visp/c-api.cpp:6-21).
 */
#ifndef VISP_HIP_KERNELS_H
#define VISP_HIP_KERNELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VX_API __attribute__((visibility("default")))

/* ---- runtime ------------------------------------------------------------------------- */
VX_API const char* vx_last_error(void);
VX_API int vx_device_count(void);
VX_API int vx_set_device(int index);
/* name/arch strings are copied into caller buffers; total/free memory in bytes */
VX_API int vx_device_info(int index, char* name, int name_cap, char* arch, int arch_cap,
                          size_t* total_mem, size_t* free_mem, int* n_cu);
VX_API int vx_malloc(void** ptr, size_t bytes);
VX_API int vx_free(void* ptr);
VX_API int vx_memset(void* ptr, int value, size_t bytes, void* stream);
VX_API int vx_memcpy_h2d(void* dst, const void* host_src, size_t bytes, void* stream);
VX_API int vx_memcpy_d2h(void* host_dst, const void* src, size_t bytes, void* stream);
VX_API int vx_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
/* pinned host memory + copies that do NOT synchronise (the overlapped host pipeline: H2D / compute / D2H on three streams) */
VX_API int vx_malloc_host(void** ptr, size_t bytes);
VX_API int vx_free_host(void* ptr);
VX_API int vx_memcpy_h2d_async(void* dst, const void* pinned_src, size_t bytes, void* stream);
VX_API int vx_memcpy_d2h_async(void* pinned_dst, const void* src, size_t bytes, void* stream);
VX_API int vx_event_sync(void* ev);
VX_API int vx_stream_create(void** stream);
VX_API int vx_stream_destroy(void* stream);
VX_API int vx_stream_sync(void* stream);
VX_API int vx_event_create(void** ev);
VX_API int vx_event_destroy(void* ev);
VX_API int vx_event_record(void* ev, void* stream);
VX_API int vx_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on stop */
VX_API int vx_stream_wait_event(void* stream, void* ev);            /* fork/join between streams (also under capture) */
/* hipGraph capture of a launch sequence */
VX_API int vx_graph_begin_capture(void* stream);
VX_API int vx_graph_end_capture(void* stream, void** graph_exec);
VX_API int vx_graph_launch(void* graph_exec, void* stream);
VX_API int vx_graph_destroy(void* graph_exec);

/* ---- GEMM family: C[M,N] = A[M,K] * W[N,K]^T (f16 in, f32 accumulate on MFMA) ----------
 * replaces ggml_mul_mat (+ggml_add bias, +ggml_gelu, +ggml_mul lambda, +ggml_add residual)
 * emitted by linear() src/visp/nn.cpp:6-12, conv_2d 1x1 nn.cpp:76-81, dino.cpp:48-90,
 * conv_transpose_2d nn.cpp:117-129 (k == stride => a GEMM + pixel shuffle),
 * and ggml_conv_2d 3x3 (nn.cpp:83-97) as an implicit GEMM over NHWC input. */
enum vx_epilogue {
    VX_EPI_F16 = 0,       /* out f16 [M, ldo] = acc + bias                                      */
    VX_EPI_F16_GELU = 1,  /* ... then tanh-GELU (ggml_gelu, dino.cpp:54)                        */
    VX_EPI_F16_RELU = 2,  /* ... then ReLU                                                      */
    VX_EPI_RESID_F32 = 3, /* x f32 [M, ldo] += lambda[n] * (acc + bias)   (dino.cpp:48-50,80-87) */
    VX_EPI_TOKENS = 4,    /* patch embed: x f32 [(m/P)*(P+1) + 1 + m%P, n] = acc + bias + pos[1 + m%P, n]
                             (dino.cpp:32-46, pos-embed add fused)                              */
    VX_EPI_QKV = 5,       /* scatter into head-major q, k, v f16 [B,H,T,64]; q scaled             */
    VX_EPI_PIXSHUF = 6,   /* conv-transpose k==s: n = (dy*s+dx)*Cout + co ->
                             out f16 [b, y*s+dy, x*s+dx, co]  (nn.cpp:117-129)                  */
    VX_EPI_F16_ADD = 7,   /* out f16 = [relu](acc + bias) + res1 + res2 (nullable), conv residual units
                             (depth-anything.cpp:15-30)                                          */
    VX_EPI_HEAD_OUT = 8,  /* N == 32: out f32 [M] = head_scale * relu(sum_n relu(acc+bias)[n] * lambda[n] + head_bias):
                             head.conv2 + ReLU + head.conv3 (1x1 -> 1) + ReLU fused (depth-anything.cpp:87-94) */
    VX_EPI_LRELU_AGC = 9, /* MI-GAN: out f16 = clamp(lrelu_0.2(acc + bias + noise[m % noise_hw]) * sqrt2, +-256); noise f32 plane
                             or NULL; then + res1 f16 [M, ldo] if given (plain GEMM only; migan.cpp:17-26, 53-82) */
    VX_EPI_SILU = 10,     /* YOLOv9t Conv: out f16 = silu(acc + bias), then + res1 f16 [M, ld_res1] if given (the RepBottleneck
                             shortcut, added after the activation; yolov9t.cpp:78-120, 304-330). Plain GEMM and implicit conv */
};

typedef struct {
    /* A operand: plain rows, or implicit im2col over an NHWC image when conv_kh > 0 */
    const void* A;      /* f16 */
    int64_t lda;        /* elements between consecutive A rows (plain mode)                      */
    int a_group;        /* plain mode row remap: arow = (m / a_group) * a_group_stride + a_row_off + m % a_group */
    int a_group_stride; /* (a_group == 0: identity). Used to skip the cls token (depth-anything.cpp:50) */
    int a_row_off;
    /* implicit-GEMM conv (conv_kh > 0): A is [B, H, W, Cin] f16, m = (b, oy, ox), k = (ky, kx, c) */
    int conv_kh, conv_kw, conv_stride, conv_pad;
    int conv_H, conv_W, conv_Cin, conv_OH, conv_OW;
    int a_relu;         /* implicit conv only: apply ReLU to A elements while loading (depth-anything.cpp:17,19);
                           refused in plain mode, whose loader has no ReLU                       */

    const void* W;      /* f16 [N, K], K padded to a multiple of 64 with zeros                   */
    const float* bias;  /* f32 [N] or NULL                                                      */
    int M, N, K;

    int epi;            /* enum vx_epilogue */
    void* out;
    int64_t ldo;
    int relu;           /* VX_EPI_F16_ADD: apply ReLU before adding residuals                   */
    const float* lambda; /* VX_EPI_RESID_F32: f32 [N]                                           */
    const float* pos;   /* VX_EPI_TOKENS: f32 [(P+1), N]                                        */
    int tokens_P;       /* VX_EPI_TOKENS: patches per image                                     */
    /* VX_EPI_QKV */
    void* q; void* k; void* vt;
    int qkv_T, qkv_Tp, qkv_H; /* tokens per image, (unused), heads; vt receives v as [B,H,T,64]    */
    float q_scale;
    /* VX_EPI_PIXSHUF */
    int ps_s, ps_Cout, ps_H, ps_W; /* stride, real Cout, input H, W; ldo = output channel stride */
    /* VX_EPI_F16_ADD */
    const void* res1; const void* res2; /* f16 [M, ldo] or NULL */
    int n_valid;        /* f16 outputs: columns >= n_valid are not stored (N padded for tiling); 0 = N. The f32 epilogues
                           (RESID_F32, TOKENS) store all N columns and refuse 0 < n_valid < N    */
    int stages;         /* LDS ring depth of the k-loop: 0 = kernel default (tuning knob for benches) */
    float head_bias, head_scale; /* VX_EPI_HEAD_OUT: conv3 bias, max_depth; lambda = conv3 weights f32 [N] */
    /* VX_EPI_F16_ADD extras (TinyViT): post_gelu: out = gelu(acc + bias + res1 [+ res2]) (mb_conv tail, mobile-sam.cpp:88-90).
     * win_ws > 0: the M rows are in window order of a win_res x win_res map (window_partition with zero padding,
     * mobile-sam.cpp:25-46); out and res1/res2 are addressed at the PIXEL row of each window row, padded rows are dropped:
     * window_reverse + residual add fused (mobile-sam.cpp:48-64, 146-149) */
    int post_gelu, win_ws, win_res;
    /* SWIN (swin.cpp:141-156): win_res_h > 0 makes the map win_res (width) x win_res_h (height); win_shift > 0 undoes the cyclic
     * shift as well (window row -> padded position -> + shift modulo the padded extent -> pixel, dropped if outside the map) */
    int win_res_h, win_shift;
    /* split-K for deep reductions on few output tiles (3x3 convs with thousands of input channels on small maps): k_splits > 1
     * cuts the k-loop into that many ranges, one workgroup each, partial sums f32 in k_partial [k_splits][M][N] (caller's scratch),
     * summed in a fixed order by a second launch that applies bias / ReLU / res1 -- deterministic. Epilogues F16, F16_RELU, and F16_ADD
     * with `relu` and res1 only (no res2, post_gelu or window order). */
    int k_splits; float* k_partial;
    void* debug_stamps; /* diagnostics only: u64 [blocks][8] s_memtime stamps per phase, NULL in product */
    const float* noise; /* VX_EPI_LRELU_AGC: f32 [noise_hw] (noise_const * noise_strength) added at row m % noise_hw, or NULL */
    int noise_hw;
    /* implicit conv: elements between consecutive input pixels (0 = conv_Cin), so that a conv reads a channel slice of a wider
     * NHWC map (A points at the slice's first channel; a multiple of 8, >= conv_Cin) */
    int64_t conv_pix;
    int64_t ld_res1;    /* row stride of res1 in elements (0 = ldo); VX_EPI_SILU only */
} vx_gemm_args;

VX_API int vx_gemm_f16(const vx_gemm_args* args, void* stream);
/* heuristic for vx_gemm_args.k_splits: > 1 only when the tile grid fills less than half the chip and the k-loop has >= 16 tiles */
VX_API int vx_gemm_pick_k_splits(int M, int N, int K);

/* 3x3 / stride 1 / pad 1 NHWC convolution with the input halo staged once in LDS (Cin, Cout in {32, 64};
 * epilogues F16, F16_RELU, F16_ADD, HEAD_OUT). Same argument block as the implicit-GEMM form (conv_* fields,
 * W = [Cout][Kp] with k = (ky,kx,c)); used for the DPT fusion / head convs at >= 96 px (depth-anything.cpp:15-23, 81-94).
 * It reads whole pixels of conv_Cin channels and addresses out, res1 and res2 at pixel * ldo (ldo % 8 == 0, >= N), in pixel order, over
 * the whole k range. What it does not implement it refuses: vx_conv3x3_supported answers 0 and vx_conv3x3_f16 returns 0 with a message for
 * conv_pix other than 0 or conv_Cin, non-zero post_gelu, win_ws, win_res_h, ld_res1 or a_group, k_splits above 1, and res2 without res1
 * -- vx_gemm_f16 implements those. */
VX_API int vx_conv3x3_supported(const vx_gemm_args* args);
VX_API int vx_conv3x3_f16(const vx_gemm_args* args, void* stream);

/* ---- ESRGAN dense-block 3x3 convolution (esrgan.cpp:13-79) ---------------------------------
 * Activations are f16, PLANAR in groups of 32 channels: a C-channel map is C/32 planes of [B, H, W, 32], consecutive
 * planes `*_plane` elements apart. A residual dense block keeps [x|x1|x2|x3|x4] as six planes of one buffer: a conv
 * reads the first cin/32 planes and writes its 32 (or 64) outputs as the next plane(s), so concat
 * (esrgan.cpp:29-36) is never materialised.
 *   v = conv(x) + bias;  act: v = max(v, 0.2 v);  res1: v = v*s1 + res1;  res2: v = v*s2 + res2.
 *   The order is fixed: activation first, then res1, then res2. s1 / s2 apply only together with their residual.
 *   x_residual (cout = 64): v = v*s1 + x[planes 0,1] with x taken from the halo already in LDS (no second read);
 *   mutually exclusive with res1, res2 still applies afterwards. The fold adds x * f16(1/s1) to the accumulators, so it is
 *   refused with act != 0, with a_relu and for an s1 whose f16 reciprocal times s1 is not 1 (vx_dconv_x_residual_supported);
 *   pass x as res1 there.
 * up2: the source is [B, H/2, W/2, 32] per plane and is nearest-upsampled on the fly (esrgan.cpp:13-19).
 * w: packed by the host as [cin/32][9 taps][cout][32] f16 with the four 16-byte groups of every (tap, n) row
 *    stored at position g ^ ((n >> 2) & 3)  (see pack_dconv in csrc/graph.cpp).
 * VX_DC_RGB_F32: cout = 32 (3 real), out = f32 [B, H, W, 3], no activation / residuals.
 * VX_DC_HEAD_F32: cout = 32, out = f32 [B, H, W] = head_scale * relu(sum_n relu(v)[n] * head_w[n] + head_bias)
 *   (head.conv2 + ReLU + head.conv3 1x1 + ReLU of the DPT head, depth-anything.cpp:87-94).
 *   Both f32 epilogues refuse act != 0, res1, res2 and x_residual (they have no place to apply them).
 * The same kernel serves NHWC maps: *_pix = elements between pixels (0 = 32 = planar), *_plane = elements between
 *   consecutive 32-channel groups (32 for NHWC). act: 0 none, 1 LeakyReLU 0.2, 2 ReLU. a_relu: convolve relu(x). */
enum { VX_DC_F16 = 0, VX_DC_RGB_F32 = 1, VX_DC_HEAD_F32 = 2 };
typedef struct {
    const void* x; int64_t x_plane; int cin; int up2;
    int B, H, W;                 /* output (= conv-space) extent */
    const void* w; const float* bias; int cout;
    int epi, act;
    float s1; const void* res1; int64_t res1_plane;
    float s2; const void* res2; int64_t res2_plane;
    void* out; int64_t out_plane;
    int x_residual;
    int64_t x_pix, out_pix, res1_pix, res2_pix;
    int a_relu;
    const float* head_w; float head_bias, head_scale;
    void* stamps; /* diagnostics only: u64 [blocks][8] = cycles in {dma wait, barrier, dma issue + halo cursor, mfma loop, epilogue, tile setup}, steps, end clock; NULL in product */
    /* round 3 -- ggml_interpolate(BILINEAR | ALIGN_CORNERS) fused into the consumer (depth-anything.cpp:36-38, 84-85; ml.cpp:782-788):
     * bil_hs > 0: x is the LOW-resolution map [B, bil_hs, bil_ws, .] and the conv runs on its bilinear resize to H x W, interpolated by
     *   the halo loader (source patch by LDS-DMA, packed-f16 weights); cout = 32, no up2 / a_relu / x_residual, H + W <= 2048 and a
     *   scale that keeps an 18 x 34 halo inside a 12 x 21 source patch (about <= 0.575; vx_dconv_bilinear_supported).
     * res2_hs > 0: res2 is [B, res2_hs, res2_ws, .] and is resized to H x W where the epilogue adds it (same arithmetic). */
    int bil_hs, bil_ws;
    int res2_hs, res2_ws;
} vx_dconv_args;
VX_API int vx_dconv_bilinear_supported(int cout, int H, int W, int hs, int ws);
VX_API int vx_dconv3x3_f16(const vx_dconv_args* args, void* stream);
/* sets the kernels' dynamic-LDS attribute (call once per process before capturing launches into a hipGraph) */
VX_API int vx_dconv_prepare(void);
/* may the "+ x" of x_residual be folded into the accumulators for this s1 / act / a_relu (see above) */
VX_API int vx_dconv_x_residual_supported(float s1, int act, int a_relu);
/* test hooks (process-global, host side only; the device code is the product's):
 * vx_dconv_set_block_cap(n): the launcher sizes its persistent grid as on a device with n CUs (n a multiple of 8, >= 8), so that a small
 *   problem walks several tiles per block; n <= 0 restores the device's CU count. Returns 0 for any other n.
 * vx_dconv_set_resident_mode(mode): overrides VISP_DCONV_RES (0 never resident, 1 cin 64, 2 cin <= 128); mode < 0 = the environment
 *   variable or, without one, the default. */
VX_API int vx_dconv_set_block_cap(int n);
VX_API void vx_dconv_set_resident_mode(int mode);

/* ---- one launch per DPT residual unit on small maps (depth-anything.cpp:15-33; kernels_rcu.hip) -------------
 *   out = P( conv2( relu( conv1( relu(x) ) + b1 ) ) + b2 + x [+ res2] ),  P = identity or the 1x1 projection wp (+ bp)
 * x, res2, out: f16 NHWC [B, H, W, 64]; biases f32 [64] or NULL. w1, w2: f16 [9 taps][64 n][64 c], wp: f16 [64 n][64 c], every (tap, n) row of
 * 128 bytes with its eight 16-byte groups stored at position g ^ ((n >> 1) & 7) (the linear LDS image of a tap's slab).
 * The intermediate map stays in LDS. Supported (vx_rcu_supported): H, W in 1..96 whose tile (chosen from H and W) has an input region of at
 * most 512 pixels and fits 160 KB of LDS -- 148 of the 9216 extents are refused for that, most of them narrow and tall (29 x 11, 29 x 21,
 * 57 x 21, 96 x 2 as H x W). Everything else, larger maps included, is the LDS-ring conv's. */
typedef struct {
    const void* x; const void* w1; const float* b1; const void* w2; const float* b2;
    const void* res2; const void* wp; const float* bp;
    void* out;
    int B, H, W;
} vx_rcu_args;
VX_API int vx_rcu_supported(int H, int W);
VX_API int vx_rcu_fused_f16(const vx_rcu_args* args, void* stream);

/* tile_layout (include/visp/image.h:163-181, src/visp/image.cpp:612-651) */
typedef struct { int image_w, image_h, overlap_x, overlap_y, n_x, n_y, tile_w, tile_h; } vx_tile_layout;
/* image_u8_to_f32 with tile offset for every tile (vision.cpp:236-241) -> one plane f16 [B*n_tiles, tile_h, tile_w, 32]
 * (channels 0..2 = value, 3..5 = f16 rounding residue, rest 0). format = visp::image_format (u8 colour). */
VX_API int vx_esrgan_tiles_in(const uint8_t* img, int B, int w, int h, int format, const vx_tile_layout* t, void* out, void* stream);
/* the same tiles as f32 rgb [B*n_tiles, tile_h, tile_w, 3]: the input tensor of the generator's graph (which splits it into value | residue itself) */
VX_API int vx_esrgan_tiles_in_f32(const uint8_t* img, int B, int w, int h, int format, const vx_tile_layout* t, float* out, void* stream);
/* tile_merge of all tiles in the reference's order + image_f32_to_u8 rgba (image.cpp:653-693, vision.cpp:246-252).
 * tiles: f32 [B, n_y, n_x, tile_h, tile_w, 3] (t = the SCALED layout); out_f32 [B,h,w,3] and/or out_rgba [B,h,w,4]. */
VX_API int vx_esrgan_tiles_out(const float* tiles, int B, const vx_tile_layout* t, float* out_f32, uint8_t* out_rgba, void* stream);

/* ---- TinyViT (MobileSAM image encoder) helpers, kernels_tinyvit.hip -------------------------------------------------
 * u8 rgb -> f16 [pixels][8]: (v/255 - mean)/std (sam_process_input, mobile-sam.cpp:533-547) as value + f16 residue */
VX_API int vx_tv_preprocess(const uint8_t* rgb, void* out, int64_t n_pixels, void* stream);
/* depthwise 3x3 pad 1 (+ bias, optional GELU) on NHWC f16: conv_2d_depthwise, nn.cpp:102-115; w f16 [9][C], bias f32 [C] */
VX_API int vx_dwconv3x3_f16(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int stride, int gelu, void* stream);
/* second half of mb_conv in one launch (mobile-sam.cpp:82-90; kernels_mbconv.hip): y = gelu(x + conv3(gelu(dw3x3(h) + b2)) + b3)
 * h f16 [B,H,W,C] (= gelu(conv1(x))), w2 f16 [9][C], w3 f16 = vx_mbconv_pack_w3 (host code) of the row-major [Cout][C] weight
 * (MFMA fragment order, same byte count), x / y f16 [B,H,W,Cout]. Built for C = 256, Cout = 64, W % 64 == 0
 * (vx_mbconv_dw_pw_supported); the depthwise output only exists as an LDS tile. */
VX_API int vx_mbconv_dw_pw_supported(int C, int Cout, int W);
VX_API int vx_mbconv_pack_w3(const void* w3_rows_host, void* packed_host);
VX_API int vx_mbconv_dw_pw_f16(const void* h, const void* w2, const float* b2, const void* w3, const float* b3, const void* x, void* y, int B, int H,
                               int W, int C, int Cout, void* stream);
/* LayerNorm of f16 rows (nn.cpp:14-19). ws > 0: output rows in window order of a res x res map (window_partition,
 * mobile-sam.cpp:25-46; padded positions = norm of zero = bias). out_f32: f32 output. C <= 1024 (above 512: one wave per row). */
VX_API int vx_layernorm_f16(const void* x, const float* w, const float* b, void* y, int64_t rows_out, int C, float eps, int res, int ws,
                            int out_f32, void* stream);
/* window attention with relative position bias, head_dim 32, on MFMA (mobile-sam.cpp:112-131; kernels_winattn.hip): qkv f16
 * [n_windows*N][heads*96] (per head q|k|v), out f16 [n_windows*N][heads*32]; N <= 256. bias_packed: the f16 image that
 * vx_window_attention_pack_bias (host code) makes of attention_biases_indexed f32 [heads][N][N] -- accumulator order,
 * padded keys = -inf -- vx_window_attention_bias_bytes(N, heads) bytes, uploaded by the caller. */
VX_API size_t vx_window_attention_bias_bytes(int N, int heads);
VX_API int vx_window_attention_pack_bias(const float* bias_host, int N, int heads, void* packed_host);
VX_API int vx_window_attention_f16(const void* qkv, const void* bias_packed, void* out, int n_windows, int N, int heads, void* stream);
/* ---- SWIN encoder (BiRefNet backbone, swin.cpp), kernels_swin.hip + the masked form of the window attention --------------
 * shifted windows (swin.cpp:165-213): bias_packed holds FOUR images (vx_swin_attention_pack_bias: bias, + last-column mask,
 * + last-row mask, + corner mask); window (wy, wx) of an nwy x nwx image picks its class. nwx = nwy = 0: one image. */
VX_API int vx_swin_attention_pack_bias(const float* table /*[(2ws-1)^2][heads]*/, int ws, int heads, void* packed_host /*4 x bias_bytes(ws*ws, heads)*/);
VX_API int vx_window_attention_masked_f16(const void* qkv, const void* bias_packed, void* out, int n_windows, int N, int heads, int nwx, int nwy,
                                          void* stream);
/* LayerNorm of f16 rows [.., C] (C % 8 == 0, <= 2048). ws > 0: norm1 + pad + roll(-shift) + window_partition of swin::block
 * (swin.cpp:124-139): x is [B, H, W, C], output rows are window tokens (zeros where the padded map has no pixel). ws = 0: rows in
 * place; out_f32 writes f32 (the per-stage output norms, swin.cpp:255-258). */
VX_API int vx_swin_layernorm_f16(const void* x, const float* w, const float* b, void* y, int64_t rows_out, int C, float eps, int H, int W, int ws,
                                 int shift, int out_f32, void* stream);
VX_API int vx_swin_layernorm_strided_f16(const void* x, const float* w, const float* b, void* y, int64_t rows, int C, float eps, int ldy, int out_f32,
                                         void* stream); /* plain rows, output row stride ldy elements (0 = C) */
/* patch_merging up to the reduction linear (swin.cpp:140-158): 2x2 gather in the reference's concat order + LayerNorm(4C);
 * x [B, H, W, C] -> y [B * H/2 * W/2, 4C] */
VX_API int vx_swin_merge_layernorm_f16(const void* x, const float* w, const float* b, void* y, int B, int H, int W, int C, float eps, void* stream);
/* window_reverse + roll(+shift) + crop + shortcut (swin.cpp:141-156): y [B,H,W,C] = x + a[window row] */
VX_API int vx_swin_window_reverse_add_f16(const void* a, const void* x, void* y, int B, int H, int W, int C, int ws, int shift, void* stream);
/* window_reverse + residual: y[b,py,px,:] = x[b,py,px,:] + a[window row of (py,px),:] (mobile-sam.cpp:48-64, 146-149) */
VX_API int vx_window_reverse_add_f16(const void* a, const void* x, void* y, int B, int res, int ws, int C, void* stream);
/* ---- BiRefNet glue (two-scale encode + decoder, birefnet.cpp), kernels_birefnet.hip ---------------------------------------
 * normalised (birefnet_process_input) and downscaled by 2 (bilinear, align_corners): rgb u8 [B,H,W,3] -> f16 [B,H/2,W/2][8] value + residue */
VX_API int vx_bf_preprocess_half(const uint8_t* rgb, void* out8, int B, int H, int W, void* stream);
/* image_to_patches of the normalised image (birefnet.cpp:158-167): -> f16 [B, h, w, (IW/w)*(IH/h)*3], channel = gx + gw (gy + gh c) */
VX_API int vx_bf_patches(const uint8_t* rgb, void* out, int B, int IH, int IW, int h, int w, void* stream);
/* bilinear align-corners resize of f16 NHWC maps; lds / ldd = row strides in elements (channel slices of wider buffers); C % 8 == 0 */
VX_API int vx_bf_resize_f16(const void* src, int lds, void* dst, int ldd, int B, int h, int w, int C, int oh, int ow, void* stream);
/* sampling half of deformable_conv_2d (birefnet.cpp:83-92 = torchvision deform_conv2d, stride 1, pad k/2): x f16 [B,h,w,C]; offmod
 * [B*h*w, ldom] = per pixel 2 k^2 offsets (dy, dx per tap) then k^2 modulator logits; cols [B*h*w, k*k*C] = 2 sigmoid(mod) * sample */
VX_API int vx_bf_deform_cols_f16(const void* x, const void* offmod, int ldom, void* cols, int B, int h, int w, int C, int k, void* stream);
/* ---- deformable convolution as one implicit GEMM whose A loader samples (kernels_deform.hip; nn.cpp:131-148, stride 1) ----
 * x f16 [B,H,W,Cin], Cin % 16 == 0; w f16 [Cout pad 32][k*k*Cin] (row n = the kernel of output n, taps (ky, kx) then channels; pad rows
 * zero); Cout % 8 == 0, <= 256; k 1..7. Output extent OH = H + 2 pad - k + 1 (OW alike). offset f16 [B*OH*OW][ld_offset]: element 2t = dy,
 * 2t+1 = dx of tap t = ky*k + kx. mask f16 [B*OH*OW][ld_mask], element t: mask_mode 0 none, 1 the factor as it is, 2 a logit (factor =
 * mask_scale * sigmoid(logit)). A sample at (py, px) counts only inside (-1, H) x (-1, W); corners outside the map are zero. out f16
 * [B*OH*OW][ldo] = relu?(scale[n] * conv + bias[n]) (scale, bias f32 [Cout], NULL = none). */
typedef struct {
    const void* x; int B, H, W, Cin;
    const void* w; int Cout, k, pad;
    const void* offset; int ld_offset;
    const void* mask; int ld_mask; int mask_mode; float mask_scale;
    const float* scale; const float* bias; int relu;
    void* out; int ldo;
} vx_deform_conv_args;
VX_API int vx_deform_conv_f16(const vx_deform_conv_args* args, void* stream);
/* per-image pixel mean [B, n, C] (row stride ld) -> [B, C]; broadcast of [B, C] rows to every pixel of a slice; y *= sigmoid(a); final mask */
VX_API int vx_bf_mean_f16(const void* x, int ld, void* y, float* acc_scratch /*f32 [B*C]*/, int B, int64_t n, int C, void* stream);
VX_API int vx_bf_broadcast_f16(const void* g, int ldg, void* dst, int ldd, int B, int64_t n, int C, void* stream);
VX_API int vx_bf_mul_sigmoid_f16(void* y, int ldy, const void* a, int lda, int64_t rows, int C, void* stream);
VX_API int vx_bf_sigmoid_out_f32(const void* a, int lda, float* out, int64_t n, void* stream);
/* y f16 = a + b[i mod b_period]; a f16 or f32 (SAM decoder: queries + query_pe, keys + key_pe, embedding + no_mask_embed) */
VX_API int vx_add_rows_f16(const void* a, int a_is_f32, const void* b, int64_t b_period, void* y, int64_t n, void* stream);
/* attention with few queries or few keys (SAM mask decoder, mobile-sam.cpp:306-320): q [Nq][heads*hd], k, v [Nk][heads*hd]
 * -> out [Nq][heads*hd]; hd a power of two <= 32 (1, 2, 4, 8, 16, 32), Nk <= 4096; scale = 1/sqrt(hd) */
VX_API int vx_small_attention_f16(const void* q, const void* k, const void* v, void* out, int Nq, int Nk, int heads, int hd, void* stream);
/* sam::interpolate_bilinear (mobile-sam.cpp:485-516) for sam_process_mask (:556-583): source element (x, y) at
 * src[(y * sstride + x) * step], f16 or f32; dst f32 [dh][dw], or u8 thresholded at 0 (0 / 255) when out_u8 */
VX_API int vx_sam_interpolate(const void* src, int src_f16, int sw, int sh, int sstride, int step, void* dst, int dw, int dh, int out_u8, void* stream);
/* y = gelu(a + b), b nullable (mb_conv tail, mobile-sam.cpp:88-90) */
VX_API int vx_add_gelu_f16(const void* a, const void* b, void* y, int64_t n, void* stream);

/* ---- fused multi-head attention, head_dim 64 (nn.cpp:210-244, dino.cpp:59-74) ------------
 * q,k,v: f16 [B,H,T,64], q pre-scaled by VX_ATTN_Q_SCALE = log2(e) / sqrt(64): the kernel works in the exp2 domain and the
 * producer of q (QKV epilogue / block kernel, their q_scale argument) folds the factor in; out: f16 [B*T, H*64].
 * softmax in f32, S never leaves registers; V is transposed on the fly by ds_read_b64_tr_b16. */
#define VX_ATTN_Q_SCALE 0.18033688011112042f
VX_API int vx_attention_f16(const void* q, const void* k, const void* v, void* out, int B, int H, int T,
                            void* stream);
/* attention with an additive mask, head_dim 32 or 64, any T (kernels_attn_mask.hip; nn.cpp:210-244 with a mask, swin.cpp:69-97):
 * q, k, v f16 head-major [B,H,T,head_dim], q pre-scaled by scale * log2(e) (for 1 / sqrt(head_dim): VX_ATTN_Q_SCALE at 64);
 * mask f16 (or f32: mask_is_f32) [Bm][Hm][T queries][T keys], Hm = 1 or H, Bm divides B, batch b reads image b % Bm; -inf entries
 * allowed, a row that is -inf on every key is unspecified; out f16 [B*T, H*head_dim] = softmax(scale q k^T + mask) v */
VX_API int vx_attention_masked_f16(const void* q, const void* k, const void* v, const void* mask, void* out, int B, int H, int T, int head_dim,
                                   int Hm, int Bm, int mask_is_f32, void* stream);
/* attention without a mask for any T_q, T_k >= 1, head_dim 16, 32 or 64 (kernels_attn_cross.hip; nn.cpp:210-244 with mask == nullptr as
 * mobile-sam.cpp:307-319 calls it): q f16 [B][T_q][H][head_dim], k, v f16 [B][T_k][H][head_dim] -- token-major rows of H * head_dim, NOT head-major and
 * NOT pre-scaled: the kernel multiplies the f32 scores by scale * log2(e). out f16 [B][T_q][H * head_dim] = softmax(scale q k^T) v.
 * With T_q <= 32 and T_k >= 256 the keys are split into parts of 128 over blocks; the parts' (m, l, O) triples go through `partial`
 * (vx_attention_cross_partial_bytes, 0 when there is one part; NULL is then fine) and a second launch folds them in part order: no atomics, the same
 * bits on every run. vx_attention_cross_parts: the number of parts (1: a single launch). */
VX_API int vx_attention_cross_parts(int Tq, int Tk);
VX_API size_t vx_attention_cross_partial_bytes(int B, int H, int Tq, int Tk, int head_dim);
VX_API int vx_attention_cross_f16(const void* q, const void* k, const void* v, void* out, void* partial, size_t partial_bytes, int B, int H, int Tq, int Tk,
                                  int head_dim, float scale, void* stream);
/* the two launches of a split one by one (the graph layer lists them as two): step 1 the attention launch, step 2 the combine launch (nothing when parts == 1) */
VX_API int vx_attention_cross_step_f16(int step, const void* q, const void* k, const void* v, void* out, void* partial, size_t partial_bytes, int B, int H, int Tq,
                                       int Tk, int head_dim, float scale, void* stream);
/* ggml_mul_mat of two f16 activations (kernels_samdec.hip; mobile-sam.cpp:471): a [Ba][M][K], b [B][N][K] -> out [B][N][M], out[b][n][m] = sum_k a[b or 0][m][k]
 * b[b][n][k], f32 sums with k ascending, one f16 rounding. K a multiple of 8 and <= 256, N <= 16, Ba 1 or B; a 16-byte aligned. One thread per row m. */
VX_API int vx_mul_mat_f16(const void* a, const void* b, void* out, int64_t M, int N, int K, int B, int Ba, void* stream);
/* ggml_sin (mode 0) / ggml_cos (mode 1): y f16 = sin(x) / cos(x), x f16 in radians, f32 inside (x / 2 pi reduced to [-0.5, 0.5] revolutions); 16-byte aligned */
VX_API int vx_sincos_f16(int mode, const void* x, void* y, int64_t n, void* stream);
/* position_embedding_random (mobile-sam.cpp:238-248): coords f32 [n_points][2] (x, y), gauss f32 [F][2] (g0[f], g1[f]) -> out f16 [n_points][2 F] =
 * sin | cos of 2 pi (x g0 + y g1); product, scale and argument reduction in f32 */
VX_API int vx_fourier_features_f32(const float* coords, const float* gauss, void* out, int64_t n_points, int F, void* stream);
/* ---- batched MobileSAM decode, many prompts per encoded image (kernels_samprompts.hip) ----
 * iou_prediction_head (mobile-sam.cpp:476-481) on one f16 token per prompt (prompt p at tokens + p * row_stride elements): three linears K0 -> N0 -> N1 -> N2 with
 * ReLU behind the first two, f32 weights [n][k] and biases on the device, f32 sums. iou f32 [P][N2]; chosen i32 [P] (nullable) = argmax of the first three
 * predictions, the first index on ties (std::max_element, vision.cpp:80-82). Widths <= 1024, 3 <= N2 <= 64. */
VX_API int vx_sam_iou_head_f32(const void* tokens, int64_t row_stride, int P, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                               const float* b2, int K0, int N0, int N1, int N2, float* iou, int32_t* chosen, void* stream);
/* sam_process_mask (mobile-sam.cpp:556-583) for P prompts in two launches with the arithmetic of vx_sam_interpolate, bit for bit. Prompt p reads the f16 logit
 * plane chosen[p] (clamped to 0 .. n_planes - 1): element (x, y) of plane c at planes[p * prompt_stride + c * plane_stride + (y * mask_size + x) * step].
 * Step 1: mask_size^2 -> scaled f32 [P][image_size^2]; step 2: the top-left sw x sh of that -> out u8 [P][dh][dw], 0 / 255 by the sign. */
VX_API int vx_sam_process_masks(const void* planes, int64_t prompt_stride, int64_t plane_stride, int step, int mask_size, int n_planes, const int32_t* chosen,
                                float* scaled, int image_size, int sw, int sh, uint8_t* out, int dw, int dh, int P, void* stream);
/* dst f16 [B][n] = B copies of src f16 [n]; n a multiple of 8, both 16-byte aligned */
VX_API int vx_sam_tile_rows_f16(const void* src, int64_t n, void* dst, int B, void* stream);
/* ---- MobileSAM automatic mask generation: the selection stage behind a batched decode (kernels_samselect.hip) ----
 * Candidate c = prompt * n_planes + plane, the first n_planes f16 logit planes of each prompt: plane at planes + prompt * prompt_stride + plane * plane_stride
 * elements, mask_size^2 logits row by row. Over the region x < cw, y < ch: table i32 [c][6] = {logits > +offset, logits > -offset, then the inclusive box
 * x0, y0, x1, y1 of the logits > 0, all 0 without one}; stability f32 [c] = table[0] / table[1], 0 when table[1] is 0. One block per candidate; 16-byte loads
 * when the planes are 16-byte aligned and mask_size and both strides are multiples of 8. */
VX_API int vx_sam_score_planes_f16(const void* planes, int64_t prompt_stride, int64_t plane_stride, int mask_size, int n_planes, int cw, int ch, float offset,
                                   int32_t* table, float* stability, int P, void* stream);
/* Filters, rank and greedy box NMS over N candidates (1 .. 16384) in four launches. Candidate c has the predicted iou iou[(c / n_planes) * iou_stride + c % n_planes]
 * and the table row above. flags i32 [N]: iou > pred_iou_thresh (a NaN fails), table[1] > 0 and (float)table[0] >= stability_thresh * (float)table[1].
 * rank i32 [N]: position among the survivors by iou descending, ties to the smaller index; -1 for the others. NMS on the inclusive integer boxes with
 * torchvision's arithmetic (area (x1 - x0)(y1 - y0)): a KEPT survivor suppresses a later one iff (float)inter > nms_iou_thresh * (float)union.
 * keep_idx i32 [capacity]: the first min(kept, capacity) kept candidates in rank order, the rest untouched; counts i32 [2] = {returned, kept}.
 * workspace: vx_sam_rank_nms_workspace_bytes(N) bytes, 16-byte aligned (keys, order, ranked boxes, the suppression bit matrix of N rows of ceil(N / 64) words). */
VX_API size_t vx_sam_rank_nms_workspace_bytes(int N);
VX_API int vx_sam_rank_nms(const int32_t* table, const float* iou, int n_planes, int iou_stride, int N, float pred_iou_thresh, float stability_thresh,
                           float nms_iou_thresh, int capacity, void* workspace, size_t workspace_bytes, int32_t* flags, int32_t* rank, int32_t* keep_idx,
                           int32_t* counts, void* stream);
/* vx_sam_process_masks with the plane of output mask k named by keep_idx[k] = prompt * n_scored + plane (clamped to the n_prompts * n_scored candidates), for
 * k < counts[0] (a device value); masks at and behind counts[0] are neither read nor written. out u8 [capacity][dh][dw]. The masks pass through
 * scaled f32 [group][image_size^2] a group at a time: two launches per group. */
VX_API int vx_sam_process_masks_indexed(const void* planes, int64_t prompt_stride, int64_t plane_stride, int step, int mask_size, int n_scored, int n_prompts,
                                        const int32_t* keep_idx, const int32_t* counts, int capacity, int group, float* scaled, int image_size, int sw, int sh,
                                        uint8_t* out, int dw, int dh, void* stream);
/* masks u8 [capacity][h][w] -> info_i32 [k][8] = {prompt, plane (of keep_idx[k], clamped to the n_prompts * n_scored candidates), x, y, w, h of the pixels that are 255 (0, 0, 0, 0 without one), their number, 0} and,
 * when info_f32 is given, info_f32 [k][2] = {iou of the candidate, stability[candidate]}; rows at and behind counts[0] untouched. One block per mask. */
VX_API int vx_sam_mask_stats_u8(const uint8_t* masks, int w, int h, const int32_t* keep_idx, const int32_t* counts, int capacity, int n_scored, int n_prompts,
                                const float* iou, int iou_stride, const float* stability, int32_t* info_i32, float* info_f32, void* stream);
/* ---- connected components of u8 masks: SAM's remove_small_regions on the device (kernels_regions.hip) ----
 * masks u8 [n][h][w], any w, h >= 1, no alignment. A pixel is foreground iff its byte is non-zero; 8-connectivity; a component is small iff it has fewer than
 * min_area (>= 0) pixels. VX_REGIONS_HOLES: every small component of the background becomes 255 (none is exempt for touching the border).
 * VX_REGIONS_ISLANDS: every small component of the foreground becomes 0, except that where EVERY one is small the largest stays (of equal ones the one whose
 * first pixel in row-major order comes first). VX_REGIONS_BOTH: the holes, then the islands of the result. Only flipped pixels are written; with min_area 0 or 1
 * no mask byte is read or written. changed i32 [n] (nullable): 1 where a pixel of the mask flipped, else 0. counts (nullable): a device i32; masks at and behind
 * counts[0] are neither read nor written, nor are their `changed`. The masks pass through the workspace `group` at a time: labels and areas i32 per pixel,
 * vx_mask_regions_workspace_bytes(w, h, group) bytes (8 MB per mask in flight at 1024^2; 0 for arguments the launcher refuses), 16-byte aligned. Per group
 * and step five or six launches; union-find, parents only decrease; integer min / add / max atomics only: the same bytes on every run. */
#define VX_REGIONS_HOLES 1
#define VX_REGIONS_ISLANDS 2
#define VX_REGIONS_BOTH 3
VX_API size_t vx_mask_regions_workspace_bytes(int w, int h, int group);
VX_API int vx_mask_remove_small_regions_u8(uint8_t* masks, int w, int h, int n, const int32_t* counts, int min_area, int mode, int32_t* changed, void* workspace,
                                           size_t workspace_bytes, int group, void* stream);
/* The second NMS of SAM's postprocess_small_regions as an input of vx_sam_rank_nms (n_planes 1, iou_stride 1, pred_iou_thresh below 0, any stability threshold
 * up to 1). info_i32 [N][8] as vx_sam_mask_stats_u8 writes it for the cleaned masks, changed i32 [N] -> table i32 [N][6] = {1, 1, the mask's inclusive box
 * x, y, x + w - 1, y + h - 1 in image pixels, 0 0 0 0 for an empty mask}, key f32 [N] = 1 for an unchanged mask, 0 for a changed one, NaN (refused by the
 * filter) for rows at and behind counts[0]. Equal keys rank by row, which is the first stage's rank. */
VX_API int vx_sam_clean_nms_inputs(const int32_t* info_i32, const int32_t* changed, const int32_t* counts, int N, int32_t* table, float* key, void* stream);
/* Output mask i < second_counts[0] = staged mask keep_idx[i] (clamped to 0 .. N - 1) with its rows, column 7 of info_i32 = 1 for a changed mask; masks u8
 * [N][h][w], any alignment (16 bytes per thread where both buffers and h * w allow it). out_counts i32 [4] = {second_counts[0], first_counts[1], the returned
 * masks with `changed` set, min(first_counts[0], N) - second_counts[1]}. Masks and rows at and behind the count are untouched. One launch. */
VX_API int vx_sam_gather_clean_masks(const uint8_t* masks, int w, int h, const int32_t* info_i32, const float* info_f32, const int32_t* changed, const int32_t* keep_idx,
                                     const int32_t* first_counts, const int32_t* second_counts, int N, uint8_t* out_masks, int32_t* out_info_i32, float* out_info_f32,
                                     int32_t* out_counts, void* stream);
/* test hook: a lane's partial row sum above `limit` sends a key tile from the lagging-reference fast path to the full path
 * (0 = always the full path; negative = restore the default 1024) */
VX_API void vx_attention_set_fast_limit(float limit);
/* test hook (host side only): 4 or 8 forces vx_attention_f16's waves per block (128 / 256 queries), whatever T and VISP_ATTN_WAVES say;
 * anything else restores the default rule (VISP_ATTN_WAVES, else 8 above T = 512 and 4 up to it) */
VX_API void vx_attention_set_waves(int waves);
/* diagnostics (tools/attn_stamps.py): u64 [blocks][waves][4] = cycles in {wait + barrier, scores + softmax, PV, lifetime}; NULL = off */
VX_API void vx_attention_set_stamps(void* stamps);

/* ---- token-stationary DINOv2 block (kernels_block16.hip; embed dim 384, mlp 1536, head dim 64) ----------------------------
 * One launch per layer replaces everything between two attentions of dino::layer (src/visp/arch/dino.cpp:48-90):
 *   att != NULL:  x += lambda1 * (att Wo^T + bo);  x += lambda2 * (gelu(LN2(x) W1^T + b1) W2^T + b2)
 *   feat != NULL: feat = LN_final(x) as f16 rows (get_intermediate_layers, dino.cpp:100-107)
 *   q != NULL:    q, k, v = LN1(x) Wqkv^T + b of the NEXT layer, head-major f16 [B, H, T, 64], q scaled by q_scale
 * (att == NULL, q != NULL: the first layer's LN1 + QKV on x as it is.)
 * att f16 [M, 384]; x f32 [M, 384] in place; weights as the slab streams of vx_dino_block16_pack_mlp / _qkv. LayerScale arrives FOLDED
 * in by the caller: wo / w2 rows and bo / b2 scaled by lambda1 / lambda2 -- the residual stream then stays in the MFMA accumulators from
 * the attention output to the next layer's q, k, v (x read once, written once per launch).
 * vec_mlp f32 = bo' | (unused) | ln2.w | ln2.b | b1[1536] | b2' | (unused) (3840 floats), vec_qkv f32 = ln1.w | ln1.b | bqkv[1152]
 * (1920 floats), vec_tap f32 = lnf.w | lnf.b (768 floats). When q != NULL: M % T == 0 and H == 6 -- the kernel writes embed_dim / 64 heads
 * per token and uses H only as the image stride, so any other H is refused. 16 tokens per wave on v_mfma_f32_16x16x32_f16, two waves per SIMD. */
typedef struct {
    const void* att; float* x;
    const void* w_mlp; const float* vec_mlp;
    const void* w_qkv; const float* vec_qkv;
    const float* vec_tap; void* feat;
    void *q, *k, *v;
    int M, T, H;
    float q_scale, eps;
    float* cap_x1; /* tests only: f32 [M, 384] copy of x after the attention half; NULL in the product path */
    void* stamps;  /* diagnostics only: u64 [workgroups][16] s_memtime at the phase boundaries; NULL in the product path */
} vx_dino_block_args;
VX_API int vx_dino_block_supported(int embed_dim, int hidden, int head_dim);
VX_API size_t vx_dino_block_mlp_bytes(void);
VX_API size_t vx_dino_block_qkv_bytes(void);
/* host code: f16 row-major wo' [384][384], w1 [1536][384], w2' [384][1536] -> out (vx_dino_block_mlp_bytes());
 * wqkv [1152][384] (q rows, then k, then v) -> out (vx_dino_block_qkv_bytes()) */
VX_API int vx_dino_block16_pack_mlp(const void* wo, const void* w1, const void* w2, void* out);
VX_API int vx_dino_block16_pack_qkv(const void* wqkv, void* out);
VX_API int vx_dino_block16_f16(const vx_dino_block_args* args, void* stream);

/* ---- e4m3 GEMM on the block-scaled matrix instruction (kernels_gemm_fp8.hip), opt-in: BASELINE.json configs[4] "fp8 GGUF weights on CDNA4 fp8 MFMA".
 * The reference has no fp8 tensor type; the format is this backend's own: OCP e4m3 values + ONE f32 scale per row (per output channel of a weight,
 * per token of an activation), K padded to a multiple of 128 with zeros:
 *   out f16 [M, ldo] = act( a_scale[m] * w_scale[n] * sum_k A8[m, k] * W8[n, k] + bias[n] ) [+ res]   (linear + bias [+ GELU] [+ residual], nn.cpp:6-12, mobile-sam.cpp MLP);
 * n_valid and ldo multiples of 8 */
typedef struct {
    const void* A; const float* a_scale; /* e4m3 [M][Kp], f32 [M] (vx_quantize_rows_e4m3) */
    const void* W; const float* w_scale; /* e4m3 [N][Kp], f32 [N] (vx_quantize_rows_e4m3_host), N % 128 == 0 */
    const float* bias;                   /* f32 [N] or NULL */
    int M, N, Kp, n_valid;               /* columns >= n_valid are not stored */
    void* out; int64_t ldo;
    int act;                             /* 0 none, 1 tanh-GELU */
    const void* res;                     /* f16 [M, ldo] added to the result, or NULL (the MLP's residual, mobile-sam.cpp:150-160) */
} vx_gemm_fp8_args;
VX_API int vx_gemm_fp8_supported(int N, int K);
VX_API int vx_gemm_fp8(const vx_gemm_fp8_args* args, void* stream);
/* f16 rows [M][ldx] (first K columns) -> e4m3 rows [M][Kp] + scale[m] = absmax / 448 (device) */
VX_API int vx_quantize_rows_e4m3(const void* x_f16, int64_t ldx, void* q, float* scale, int M, int K, int Kp, void* stream);
/* host code: f32 rows [N][K] -> e4m3 [N][Kp] (round to nearest even, saturating at 448) + scale[n] */
VX_API int vx_quantize_rows_e4m3_host(const float* w, int N, int K, int Kp, void* q_out, float* scale_out);

/* ---- LayerNorm (nn.cpp:14-19): x f32 [M,C] -> y f16 [M,C]; biased variance, eps in sqrt --- */
VX_API int vx_layernorm_f32_f16(const float* x, const float* w, const float* b, void* y, int M, int C,
                                float eps, void* stream);

/* ---- pre-processing (depth-anything.cpp:130-140, image.cpp:215-255) + im2col of the 14x14
 * stride-14 patch embedding (nn.cpp:166-180): rgb_u8 [B,H,W,3] -> f16 [B*P, Kp],
 * k = (ky*ps + kx)*3 + c, zero padded to Kp; value = (u8/255 - mean[c]) / std[c] ----------- */
VX_API int vx_preprocess_patches(const uint8_t* rgb, void* patches, int B, int H, int W, int ps, int Kp,
                                 const float mean[3], const float inv_std[3], void* stream);
/* same normalisation to plain NHWC f32 [B,H,W,3] (the tensor the reference uploads) */
VX_API int vx_preprocess_f32(const uint8_t* rgb, float* out, int B, int H, int W, const float mean[3],
                             const float inv_std[3], void* stream);
/* cls token rows: x[b*(P+1), :] = cls + pos[0, :]  (dino.cpp:37-44) */
VX_API int vx_write_cls_rows(float* x, const float* cls, const float* pos, int B, int T, int C, void* stream);

/* ---- bilinear resize, align_corners (ml.cpp:782-788, depth-anything.cpp:36-38,83-85),
 * NHWC f16 [B,H,W,C] -> [B,OH,OW,C], C % 8 == 0 ------------------------------------------- */
VX_API int vx_bilinear_ac_f16(const void* x, void* y, int B, int H, int W, int C, int OH, int OW, void* stream);

/* ---- head tail: depth[b,y,x] = max_depth * relu(sum_c x[b,y,x,c]*w[c] + bias), x f16 NHWC
 * (already ReLU-ed conv2 output), C = 8, 16, 32 or 64 (depth-anything.cpp:89-94) ----------- */
VX_API int vx_head_out_f32(const void* x, const float* w, float bias, float max_depth, float* depth,
                           int64_t n_pixels, int C, void* stream);

/* ---- the DPT head's tail as one kernel (depth-anything.cpp:84-94; kernels_headconv.hip): x f16 [B, hs, ws, 32] --bilinear, align_corners-->
 * [B, H, W, 32] -> conv 3x3 (32 -> 32, pad 1) + bias + ReLU -> conv 1x1 (32 -> 1) + b3 + ReLU -> * scale -> out f32 [B, H, W]. The 3x3 kernel
 * is held in registers: `wfrag` = vx_headconv_pack (host code) of the GEMM-family rows [32][Kp], k = (ky, kx, c); vx_headconv_frag_bytes()
 * bytes. Supported: cin = cout = 32 and a resize whose 18 x 34 halo fits a 12 x 21 source patch (scale up to about 0.58). */
VX_API size_t vx_headconv_frag_bytes(void);
/* test hook (process-global, host side only; the device code is the product's): the 32-channel launcher starts at most n persistent blocks
 * (n a multiple of 8: one block per XCD at least), so that a small problem walks several tiles per block; n <= 0 restores the default of
 * two blocks per CU. Returns 0 for any other n. */
VX_API int vx_headconv_set_block_cap(int n);
VX_API int vx_headconv_pack(const void* w_rows, int Kp, void* out_frag);
VX_API int vx_headconv_supported(int cin, int cout, int H, int W, int hs, int ws);
/* diagnostics (tools/headconv_stamps.py): u64 [blocks][4][8] per-phase cycles of the next launches; NULL = off */
VX_API void vx_headconv_set_stamps(void* stamps);
VX_API int vx_headconv_bil_f16(const void* x, const void* wfrag, const float* bias, const float* w3, float b3, float scale, float* out, int B, int H, int W,
                               int hs, int ws, void* stream);
/* the same tail for x f16 [B, hs, ws, cin], cin = 64 or 128 (the Base / Large heads), in 32-channel K slices: `wfrag` =
 * vx_headconv_wide_pack (host code) of the rows [32][Kp], k = (ky, kx, c); vx_headconv_wide_frag_bytes(cin) bytes */
VX_API int vx_headconv_wide_supported(int cin, int cout, int H, int W, int hs, int ws); /* cin 64 / 128, cout 32, the same resize bound */
VX_API size_t vx_headconv_wide_frag_bytes(int cin);
VX_API int vx_headconv_wide_pack(const void* w_rows, int cin, int Kp, void* out_frag);
VX_API int vx_headconv_wide_bil_f16(const void* x, int cin, const void* wfrag, const float* bias, const float* w3, float b3, float scale, float* out, int B,
                                    int H, int W, int hs, int ws, void* stream);

/* ---- post-processing: per-image min/max then (v-min)/(max-min) (image.cpp:537-576), each image by its own extremes; max - min below
 * 1e-5 divides by 1. The input is finite (no NaN, no infinity). The product and the sum round separately, so an image's minimum maps to
 * +0.0 exactly. minmax: scratch of 2 B 32-bit words, nothing behind them is written; what the call leaves there is unspecified. B <= 65535 */
VX_API int vx_minmax_normalize(const float* depth, float* out, float* minmax, int B, int64_t pixels_per_image,
                               void* stream);
/* alpha_f32 -> alpha_u8: uint8(clamp(v,0,1)*255) (image-impl.h:36-38) */
VX_API int vx_f32_to_u8(const float* src, uint8_t* dst, int64_t n, void* stream);

/* ---- graph executor glue (csrc/graph.cpp, kernels_graph.hip): the stand-alone forms of the ops the reference's arch code emits between
 * its matrix products (ml.cpp:746-788 slice / concat, ggml_add / ggml_mul broadcasts, ggml_gelu / relu / scale, ggml_cont of a permute) */
/* dst[i . dst_stride] = scale * src[i . src_stride], i over ne (element strides, 0 = broadcast a source dimension) */
VX_API int vx_copy_strided_f16(const void* src, void* dst, const int64_t ne[4], const int64_t src_stride[4], const int64_t dst_stride[4], float scale,
                               void* stream);
/* ---- rotary position embedding and the token gather of the SAM3 encoders (kernels_rope.hip; sam3.h:221-231, 413-438). Memory-bound passes next to
 * vx_copy_strided_f16: 16 bytes per lane and access, no LDS, no scratch.
 * vx_rope_f16: ggml_rope_ext in GGML_ROPE_TYPE_NORMAL on rows of n f16 channels. Row (h, t, b) of x lies at x + h si[0] + t si[1] + b si[2] elements (so: out),
 * which serves token-major [B][T][heads][n] and head-major [B][heads][T][n] alike. table f32 [T][n]: cos of pair i at [t][i], sin at [t][n / 2 + i], computed
 * on the host (the kernel only multiplies): out[2i] = (x[2i] cos - x[2i+1] sin) q_scale, out[2i+1] = (x[2i] sin + x[2i+1] cos) q_scale, f32 arithmetic, one
 * f16 rounding. out == x (in place) is legal with equal strides: a lane reads and writes the same four pairs. Refused (0, vx_last_error, no launch): null or
 * misaligned (16 bytes) pointers, n % 8 != 0, strides that are no multiples of 8, an empty problem, extents past the kernel's 32-bit indexing, and an output
 * whose extent overlaps an input's (or the other output's) in any way but being that input's own in-place buffer.
 * vx_rope_supported / vx_rope2d_supported answer the shape part of that (rows of n, rows of head_dim) without launching. */
VX_API int vx_rope2d_supported(int head_dim, int heads, int T, int B, const int64_t strides_in[3], const int64_t strides_out[3]);
VX_API int vx_rope_supported(int n, int heads, int T, int B, const int64_t strides_in[3], const int64_t strides_out[3]);
VX_API int vx_rope_f16(const void* x, void* out, const float* table, int n, int heads, int T, int B, const int64_t strides_in[3], const int64_t strides_out[3],
                       float q_scale, void* stream);
/* apply_rope_2d (sam3.h:413-438) on whole heads of head_dim channels (a multiple of 16): channels [0, hd / 2) are rotated by table_x, [hd / 2, hd) by table_y
 * (each f32 [T][hd / 2] as above). q and k in ONE launch (blockIdx.y selects; k and k_out NULL: q alone), both with the same strides; q_scale is multiplied
 * into q only. The launch that replaces 2 x (2 slices + 2 ropes + 1 concat). */
VX_API int vx_rope2d_f16(const void* q, void* q_out, const void* k, void* k_out, const float* table_x, const float* table_y, int head_dim, int heads, int T, int B,
                         const int64_t strides_in[3], const int64_t strides_out[3], float q_scale, void* stream);
/* ggml_get_rows with an index known at run time only: out f16 [n_idx][C] = table f16 [rows][C] at idx i32 [n_idx] (device memory), C % 8 == 0. The guard is
 * part of the kernel: an index outside [0, rows) gives a row of zeros and reads nothing. */
VX_API int vx_get_rows_f16(const void* table, const int32_t* idx, void* out, int64_t rows, int C, int64_t n_idx, void* stream);
/* ggml_roll: dst[i] = src[(i - shift) mod ne] in every dimension (negative shifts wrap); f16, contiguous, dst != src */
VX_API int vx_roll_f16(const void* src, void* dst, const int64_t ne[4], const int64_t shift[4], void* stream);
/* ggml_pad: src [src_ne] in the low corner of dst [dst_ne >= src_ne], zeros behind it; f16, contiguous */
VX_API int vx_pad_f16(const void* src, void* dst, const int64_t src_ne[4], const int64_t dst_ne[4], void* stream);
/* y[i] = a[i] (op) b[i mod b_period]; op 0 add, 1 mul, 2 sub (a - b); each operand f16 or f32 */
VX_API int vx_binary_rows(int op, const void* a, int a_f32, const void* b, int b_f32, int64_t b_period, void* y, int y_f32, int64_t n, void* stream);
/* op 0 tanh-GELU (ggml_gelu), 1 ReLU, 2 x * s, 3 leaky ReLU x > 0 ? x : s x (ggml_leaky_relu, any slope), 4 SiLU x / (1 + exp(-x)) (ggml_silu);
 * f16, 16-byte aligned */
VX_API int vx_unary_f16(int op, const void* x, void* y, int64_t n, float s, void* stream);
/* ggml_sigmoid: y f16 = 1 / (1 + exp(-x)); x f16, or f32 (x_f32: the map of a 1x1 convolution to one channel); 16-byte aligned */
VX_API int vx_sigmoid_f16(const void* x, int x_f32, void* y, int64_t n, void* stream);
/* mean_2d (birefnet.cpp:93-100) on an NHWC map: x f16 [B, n pixels, C] -> y f16 [B, C]. f32 sums in a fixed order (four pixel slices of four chains
 * each, combined pairwise), no atomics: the same bits on every launch (kernels_birefnet.hip:137-142) */
VX_API int vx_mean_2d_f16(const void* x, void* y, int B, int64_t n, int C, void* stream);
/* y = x, f32 -> f16 (round to nearest even) or f16 -> f32 */
VX_API int vx_convert(const void* x, int x_f32, void* y, int y_f32, int64_t n, void* stream);
/* ggml_interpolate(NEAREST) of an NHWC f16 map (ml.cpp:782-788; esrgan.cpp:15) */
VX_API int vx_nearest_f16(const void* x, void* y, int B, int H, int W, int C, int OH, int OW, void* stream);
/* ... x and y pixels x_pix / y_pix elements apart (multiples of 8, >= C): an upsample that reads a channel slice and writes into a slice of a concat's buffer */
VX_API int vx_nearest_pix_f16(const void* x, int64_t x_pix, void* y, int64_t y_pix, int B, int H, int W, int C, int OH, int OW, void* stream);
/* f32 image [pixels][C <= 16] -> one 32-channel f16 plane: values, then what the f16 rounding dropped, then zeros (input of an image's first conv) */
VX_API int vx_image_planes_f32(const float* x, void* y, int64_t n_pix, int C, void* stream);
/* f32 image [pixels][3] -> f16 [pixels][8]: the values in channels 0..2, what the f16 rounding dropped in 3..5, zeros in 6..7 (the arithmetic of
 * vx_tv_preprocess without the normalisation): the input of a 3-channel conv whose GEMM operand repeats taps 0..2 on 3..5 */
VX_API int vx_image_pad8_f32(const float* x, void* y, int64_t n_pix, void* stream);
/* ---- depthwise convolution, any square kernel (kernels_dwconv.hip; conv_2d_depthwise + add_bias_2d, nn.cpp:102-115) ----
 * x f16 [B,H,W,C], C % 8 == 0; w f16 [k*k][C] (tap-major, tap = ky*k + kx); bias f32 [C] or NULL; y f16 [B,OH,OW,C] with OH = (H + 2 pad - k) / stride + 1
 * (OW alike; even kernels like odd ones). k 1..7, stride 1 or 2, pad 0..k-1. Taps outside the map are zeros. act 0 none, 1 tanh GELU (ggml_gelu),
 * 2 leaky ReLU with slope act_param. 16-byte aligned operands. */
VX_API int vx_dwconv_f16(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int k, int stride, int pad, int act, float act_param,
                         void* stream);
/* ggml_clamp: y = x < lo ? lo : (x > hi ? hi : x) on f16 (a NaN stays one); lo <= hi, both finite; 16-byte aligned */
VX_API int vx_clamp_f16(const void* x, void* y, int64_t n, float lo, float hi, void* stream);
/* y[b, p, c] = a[b, p, c] (op) plane[p] for a f16 [B, HW, C], C % 8 == 0: one value per pixel for every channel and image (migan.cpp:40, 76).
 * op 0 add, 1 mul, 2 sub; plane f16 or f32 (b_f32) [HW]; f32 arithmetic, one rounding; a and y 16-byte aligned */
VX_API int vx_binary_plane_f16(int op, const void* a, const void* b, int b_f32, void* y, int B, int64_t HW, int C, void* stream);
/* f32 image [pixels][4] -> f16 [pixels][8]: the values in channels 0..3, what the f16 rounding dropped in 4..7 (vx_image_pad8_f32 for 4 channels) */
VX_API int vx_image4_pad8_f32(const float* x, void* y, int64_t n_pix, void* stream);
/* ---- x2 FIR upsample and the depthwise conv with MI-GAN's activation (kernels_fir.hip; migan.cpp:17-26, 32-51) ----
 * out[Y, X, c] = sum_{i,j} fir[i * 4 + j][c] z[Y + i - 2, X + j - 2, c] with z[2a, 2b] = x[a, b] and zero elsewhere and outside 2h x 2w: zero insertion, a 4x4
 * depthwise FIR at pad 2, last row and column dropped, computed polyphase (each output parity reads 2 x 2 input pixels and 4 taps; no x2 intermediate).
 * x f16 [B,h,w] pixels of x_pix elements, fir f16 [16][C], y f16 [B,2h,2w] pixels of y_pix elements; channels of a y pixel beyond C are not touched.
 * Epilogue in f32 before the one f16 rounding: + plane[Y * 2w + X] (f32 [2h * 2w] or NULL); if agc: leaky ReLU 0.2, * gain, clamp to +-clamp (clamp 0: none);
 * + res (f16 [B,2h,2w] pixels of res_pix elements, or NULL). C % 8 == 0, pixel strides multiples of 8 and >= C, 16-byte aligned operands. */
VX_API int vx_upfirdn2x_f16(const void* x, int64_t x_pix, const void* fir, void* y, int64_t y_pix, const float* plane, const void* res, int64_t res_pix, int agc,
                            float gain, float clamp, int B, int h, int w, int C, void* stream);
/* vx_dwconv_f16 with lrelu_agc behind it: y = clamp((v > 0 ? v : slope v) * gain, +-clamp) of v = conv + bias, in f32 before the rounding (clamp 0: none) */
VX_API int vx_dwconv_agc_f16(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int k, int stride, int pad, float slope, float gain,
                             float clamp, void* stream);
/* ---- pooling, row softmax and row sums (kernels_pool.hip; ggml_pool_2d, ggml_soft_max, ggml_sum_rows as yolov9t.cpp:165-185, 449-483, 657-691 use them) ----
 * x f16 [B,H,W] pixels of x_pix elements, the C pooled channels first (x points at the slice's first channel); y f16 [B,OH,OW] pixels of y_pix elements,
 * OH = (H + 2 pad - k) / stride + 1 (OW alike). kind 0 max (taken in f16: exact; positions outside the map never win), 1 average (f32 sum, one rounding;
 * pad 0 only). k 1..13, stride 1 or 2, pad 0..k/2, C % 8 == 0, pixel strides multiples of 8 and >= C, 16-byte aligned operands. Channels of a y pixel
 * beyond C are not touched. */
VX_API int vx_pool2d_f16(const void* x, int64_t x_pix, void* y, int64_t y_pix, int B, int H, int W, int C, int kind, int k, int stride, int pad, void* stream);
/* y[r, :n] = softmax(x[r, :n]) for rows of n f16 (n % 8 == 0, n <= 1024) x_ld / y_ld elements apart: f32 arithmetic, the row maximum subtracted */
VX_API int vx_softmax_rows_f16(const void* x, int64_t x_ld, void* y, int64_t y_ld, int64_t rows, int n, void* stream);
/* y f16 [rows][group]: y[r, g] = sum_i softmax(x[r, g n .. g n + n))_i * proj[i], proj f32 [n]; n % 8 == 0, n <= 64, x_ld >= group * n: the DFL decode
 * (dfl_forward, yolov9t.cpp:657-691) on the box logits where they lie, inside rows of 64 + nc channels */
VX_API int vx_softmax_expect_f16(const void* x, int64_t x_ld, int group, const float* proj, void* y, int64_t rows, int n, void* stream);
/* y f16 [rows] = the sum of each row of n f16, f32, left to right (ggml_sum_rows). One thread per row with scalar loads: not a hot-path kernel (long rows are
 * read uncoalesced); with fused models the one chain that uses it, the DFL decode, is vx_softmax_expect_f16 instead */
VX_API int vx_sum_rows_f16(const void* x, void* y, int64_t rows, int n, void* stream);
/* patch_embed's im2col (nn.cpp:166-180) on the f32 image tensor [B,H,W,C]: rows (b,py,px), k = (ky,kx,c), zero padded to Kp, f16 */
/* 1x1 convolution to one channel: out f32 [M] = scale * act(sum_c x[m,c] w[c] + bias), x f16 [M][C] (depth-anything.cpp:91-95) */
VX_API int vx_conv1x1_to1_f32(const void* x, const float* w, float bias, int relu, float scale, float* out, int64_t M, int C, void* stream);
VX_API int vx_im2col_patches_f32(const float* x, void* patches, int B, int H, int W, int C, int ps, int Kp, void* stream);


/* ---- MI-GAN inpainting (migan.cpp, kernels_migan.hip): NHWC f16, f32 arithmetic, lrelu_agc = clamp(lrelu_0.2(v) * sqrt2, +-256).
 * Depthwise weights f16 [9][C] tap-major + f32 bias [C]; 4x4 FIR filters f32 [16][C]: per channel, any 16 taps (nothing assumes the symmetric
 * filter of the trained file). The f16 operands (x, w, y, feat, out) are read and written 16 bytes at a time and must be 16-byte aligned. */
/* y = lrelu_agc(dw3x3(x) + bias) [B,H,W,C]; with down_fir: then the 4x4 / stride 2 / pad 1 FIR, y [B,H/2,W/2,C] (C % 64 == 0) */
VX_API int vx_migan_dwconv_f16(const void* x, const void* w, const float* bias, const float* down_fir, void* y, int B, int H, int W, int C,
                               void* stream);
/* out [B,2h,2w,C] = lrelu_agc(upFIR(y) + noise[2h*2w] (nullable)) + feat (nullable); upFIR = zero insertion x2, 4x4 FIR pad 2, crop */
VX_API int vx_migan_upsample_f16(const void* y, const float* fir, const float* noise, const void* feat, void* out, int B, int h, int w, int C,
                                 void* stream);
/* img f32 [B,H,W,3] = x [B,H,W,C] . w[3][C] + bias[3] (+ upFIR(img_prev [B,H/2,W/2,3]) with fir f32 [16][3]); C <= 512 */
VX_API int vx_migan_torgb(const void* x, const float* w, const float* bias, const float* img_prev, const float* fir, float* img, int B, int H, int W,
                          int C, void* stream);
/* out f16 [n_pixels, C] = lrelu_agc(fromrgb(p)) with p = {a - 0.5, a (2 rgb/255 - 1)}, a = 1 - mask/255 from a u8 image (3 or 4
 * channels) + u8 mask, or p = in4 f32 [n_pixels, 4] when in4 != NULL; fromrgb w f32 [C][4], bias f32 [C] */
VX_API int vx_migan_preprocess(const uint8_t* img, int img_channels, const uint8_t* mask, const float* in4, const float* w, const float* bias,
                               void* out, int64_t n_pixels, int C, void* stream);
/* rgba u8 [n_pixels, 4] = trunc(clamp(img * 0.5 + 0.5, 0, 1) * 255) of rgb f32, alpha = mask */
VX_API int vx_migan_postprocess(const float* img, const uint8_t* mask, uint8_t* rgba, int64_t n_pixels, void* stream);

/* ---- YOLOv9t detector (yolov9t.cpp, kernels_yolov9t.hip): NHWC f16 maps, f32 arithmetic. *_pix = elements between consecutive
 * pixels of a map, so that a producer writes (or a consumer reads) a channel slice of a wider concat buffer; C % 8 == 0, pointers
 * and pixel strides 16-byte aligned.
 * preprocess: rgb / rgba u8 [n][channels] (alpha ignored) or f32 rgb [n][3] -> f16 [n][8] = v / 255 (u8) or v (f32), channels 3..7 zero */
VX_API int vx_yolo_preprocess(const uint8_t* img_u8, int channels, const float* img_f32, void* out8, int64_t n_pixels, void* stream);
/* AConv's avg_pool 2x2 / stride 1 / no pad (yolov9t.cpp:165-185): x [B, H, W, C] -> y [B, H-1, W-1, C] (contiguous) */
VX_API int vx_yolo_avgpool2_f16(const void* x, int64_t x_pix, void* y, int B, int H, int W, int C, void* stream);
/* SPPELAN's three chained 5x5 / stride 1 / pad 2 max pools (yolov9t.cpp:449-484) in one pass: buf [B, H, W, pix] holds cv1's
 * output in channels [0, C); channels [C, 2C), [2C, 3C), [3C, 4C) receive the 5-, 9- and 13-wide window maxima (clipped at the
 * border, which equals the chained pools with -inf padding). pix >= 4C */
VX_API int vx_yolo_spp_f16(void* buf, int64_t pix, int B, int H, int W, int C, void* stream);
/* nearest x2 upsample (yolov9t.cpp:486-493): x [B, h, w, C] -> y [B, 2h, 2w, C] */
VX_API int vx_yolo_upsample2_f16(const void* x, int64_t x_pix, void* y, int64_t y_pix, int B, int h, int w, int C, void* stream);
/* Detect inference (yolov9t.cpp:631-770, 875-925): raw[l] f16 [B, S/s_l, S/s_l, 64 + nc] with s_l = 8, 16, 32 (channels: 4 sides x 16
 * DFL bins side-major, then nc class logits). Per anchor (levels in order, y-major): softmax over the bins and the expectation with
 * arange(16), dist2bbox xyxy around cell + 0.5, times the stride -> boxes f32 [B, A, 4]; sigmoid -> scores f32 [B, A, nc]. Every
 * (anchor, class) with score >= conf is appended to image b's list: cand_idx[b * A * nc + i] = anchor * nc + class, cand_score the
 * same f32 score; cand_count i32 [B] must be zero on entry (the list holds A * nc entries and cannot overflow; its order is not
 * deterministic). cand_* may be NULL (dense outputs only). nc % 8 == 0 */
VX_API int vx_yolo_decode(const void* raw0, const void* raw1, const void* raw2, int B, int S, int nc, float* boxes, float* scores, float conf,
                          int* cand_count, int* cand_idx, float* cand_score, void* stream);

/* ---- matting image ops (kernels_matting.hip; image_blur, image_erosion, image_estimate_foreground, image_alpha_composite of the reference's
 * src/visp/image.cpp:358-535). Images are [B, h, w] pixels, rows *_row ELEMENTS apart (image b starts h rows behind image b - 1), or
 * contiguous where no row stride is given. Every launcher refuses null and misaligned pointers, an illegal radius, outputs that overlap
 * inputs and batches whose element count passes 32-bit indexing. No atomics: the same bits every run, for every batch size. */
/* box filter of size 2 radius + 1, edges replicated, horizontal pass into tmp (f32 [B, h, w, C] contiguous) then vertical pass into y.
 * C = 1 (alpha_f32) or 4 (rgba_f32; 16-byte aligned pointers, row strides multiples of 4). 1 <= radius <= min(w, h) / 2. Every output
 * is the sum of its own window, left to right / top to bottom, times fl(1 / (2 radius + 1)) per pass: the reference's running sum over
 * the whole row is NOT reproduced. */
VX_API int vx_box_blur_f32(const float* x, int64_t x_row, float* tmp, float* y, int64_t y_row, int B, int h, int w, int C, int radius, void* stream);
/* minimum over the clamped (2 radius + 1)^2 neighbourhood and the format's one (1.0f / 255), bit-exact; 1 <= radius <= 64 */
VX_API int vx_erode_f32(const float* x, int64_t x_row, float* y, int64_t y_row, int B, int h, int w, int radius, void* stream);
VX_API int vx_erode_u8(const uint8_t* x, int64_t x_row, uint8_t* y, int64_t y_row, int B, int h, int w, int radius, void* stream);
/* One stage of the blur-fusion foreground estimator (image.cpp:423-469) as two launches, all maps contiguous. img: the image, img_format one of
 * enum visp_image_format: rgba_u8 or rgb_u8 (read directly, / 255 in the loader), or rgba_f32. fg, bg: rgba_f32 maps, or both NULL = the image
 * itself (stage one). mask f32. planes: f32 workspace [B, h, w, 8], the horizontal window means of m, fg m, bg (1 - m). out: the
 * foreground, alpha = clamp(mask, 0, 1), as out_format rgba_f32 or rgba_u8 (truncating, as image_store does). bg_out (nullable): the
 * blurred background as rgba_f32 (its alpha is 0, nothing reads it). passes: 3 = both launches; 1 = the horizontal launch alone, 2 = the vertical launch alone
 * on the planes an earlier horizontal launch left (per-launch timing, tools/bench_matting.py); 1 then 2 gives the bits of 3. */
VX_API int vx_foreground_stage(const void* img, int img_format, const float* fg, const float* bg, const float* mask, float* planes, void* out, int out_format,
                               float* bg_out, int B, int h, int w, int radius, int passes, void* stream);
/* out rgba_u8 = trunc(clamp(w fg + (1 - w) bg, 0, 1) * 255), w = mask / 255, alpha 255; fg rgba_u8, bg rgb_u8 / rgba_u8 (bg_channels 3 / 4),
 * mask u8. f32 arithmetic without fused multiply-adds: the bits of the reference's host code. */
VX_API int vx_alpha_composite_u8(const uint8_t* fg_rgba, const uint8_t* bg, int bg_channels, const uint8_t* mask, uint8_t* out_rgba, int64_t n_pixels, void* stream);

/* ---- image ops and pixel gates of BiRefNet on the graph layer (kernels_imgops.hip; birefnet.cpp:20-73, 147-260). Memory-bound passes, no atomics: the
 * same bits on every launch. */
/* bilinear | align_corners resize of an f32 image: x [B, H, W, C] -> y [B, OH, OW, C], C 1..4. Source coordinate o * fl((in - 1) / (out - 1)) in f32 (0 where
 * out is 1), both taps clamped to the image, horizontal lerp v0 + (v1 - v0) t, then vertical: the arithmetic of vx_bf_preprocess_half */
VX_API int vx_image_bilinear_ac_f32(const float* x, float* y, int B, int H, int W, int C, int OH, int OW, void* stream);
/* image_to_patches (birefnet.cpp:153-162) of an f32 image x [B, IH, IW, C], C 1..4, as an f16 map y [B, h, w, gw gh C] with gw = IW / w, gh = IH / h:
 * channel gx + gw (gy + gh c) of pixel (py, px) is x[gy h + py, gx w + px, c], rounded to nearest even. w and h divide the image; gw gh C % 8 == 0. form 1: one
 * thread gathers 8 channels (8 loads w pixels apart); form 2: a block stages vx_image_patches_tile(gw gh C) output pixels in LDS from contiguous image-row
 * segments and writes them as one contiguous run; form 0 takes form 2 where it was measured faster (tiles below 32 pixels: more than 888 channels) and form 1 otherwise.
 * Both give the same bits. */
VX_API int vx_image_patches_f16(const float* x, void* y, int B, int IH, int IW, int C, int h, int w, int form, void* stream);
/* output pixels per block of form 2 for that many channels: the largest power of two <= 64 whose tile (channels + 8 halves per pixel) fits 56 KiB; 0 if none */
VX_API int vx_image_patches_tile(int channels);
/* the gdt gate (birefnet.cpp:189-192) per pixel: g = sigmoid(bias + sum_k a[r, k] w[k]) over the Cg channels of a (f32 sum, k ascending), rounded to f16 as
 * vx_bf_mul_sigmoid_f16's operand is; y[r, c] = f16(p[r, c] * g) for the C channels of p. p, a, y f16 with rows ldp / lda / ldy elements apart (multiples of 8);
 * w f32 [Cg]; C and Cg multiples of 8; 16-byte aligned; y overlaps neither p nor a. */
VX_API int vx_pixel_gate_f16(const void* p, int64_t ldp, const void* a, int64_t lda, const float* w, float bias, void* y, int64_t ldy, int64_t rows, int C, int Cg, void* stream);
/* vx_bilinear_ac_f16 with x and y pixels x_pix / y_pix elements apart (multiples of 8, >= C): a resize that reads a channel slice and writes its slice of a
 * concat's buffer. The same bits as vx_bilinear_ac_f16 where both strides are C. */
VX_API int vx_bilinear_ac_pix_f16(const void* x, int64_t x_pix, void* y, int64_t y_pix, int B, int H, int W, int C, int OH, int OW, void* stream);
/* LayerNorm (nn.cpp:14-19) of contiguous f16 rows x [rows][C] with output rows y_pix elements apart (a multiple of 8, >= C): a norm that writes its slice of a
 * concat's buffer. w, b f32 [C]; C % 8 == 0, C <= 1024. f32: mean, then the mean of squared deviations, 1 / sqrt(var + eps); one rounding to f16.
 * 8, 16, 32 or 64 lanes per row by C. */
VX_API int vx_layernorm_pix_f16(const void* x, const float* w, const float* b, void* y, int64_t y_pix, int64_t rows, int C, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif
