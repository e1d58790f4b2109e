// YOLOv9t object detection on the MI355X backend: model load (GGUF -> one packed weight arena), the network as a hand schedule of
// GEMM-family convolutions and kernels_yolov9t.hip launches, replayed as a hipGraph per (batch, input size), and the host
// post-processing (letterbox, NMS, scale_boxes). Host C++ only; all device work goes through the vx_* C ABI
// (include/visp_hip_kernels.h).
//
// Mirrors the reference's arch file src/visp/arch/yolov9t.cpp and its one caller src/cli/inference_yolov9t.cpp:300-405. The
// reference never wires the family into model_family / vision.h; neither does this backend (visp_model_load refuses it, the family
// loads through visp_yolov9t_load).
#pragma once
#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "gguf.h"
#include "image.h"
#include "model.h"

namespace visp {

struct yolo_detection { // detected_obj (yolov9t.h:30-35)
    float x1, y1, x2, y2;
    float confidence;
    int32_t class_id;
    float class_confidence;
};

struct yolo_nms_params { // non_max_suppression's arguments as inference_yolov9t.cpp:383 passes them
    float conf = 0.25f, iou = 0.45f;
    int max_det = 300, max_nms = 30000, max_wh = 640;
};

struct yolo_letterbox { // LetterboxResult (yolov9t.cpp:1028-1083): the S x S rgb_u8 image and the mapping back
    image_data img;
    float gain = 1, pad_w = 0, pad_h = 0;
};

// one convolution of the network: f16 [N pad][K pad] rows k = (ky, kx, c), f32 bias (BatchNorm folded by the converter; a RepConv's
// 1x1 branch folded into the centre tap of its 3x3 by the loader)
struct yolo_conv {
    packed_gemm g;
    int k = 0, cin = 0, cin_real = 0, cout = 0; // cin: channels per input pixel (model.0 reads rgb padded to 8)
};

struct yolov9t_model : model_base {
    yolov9t_model() : model_base(family_yolov9t) {}
    int input_size = 640, num_classes = 80, reg_max = 16, head_c3 = 80;
    std::map<std::string, yolo_conv> convs; // by tensor prefix, e.g. "model.4.cv2.0.m.1.cv1" (the folded RepConv), "detect.cv3.2.2"
    device_buffer weight_arena;
    device_buffer ws;
    // (batch * 8 + channels, S, bits of conf) -> captured u8 launch list (one stream, no branches; the threshold is baked into the decode)
    std::map<std::tuple<int, int, int>, captured_graph> graphs;
    void* events[2] = {nullptr, nullptr};     // around the launch list of a batch call
    float last_split_ms[3] = {0, 0, 0};       // last batch call: launch list on the device (events), candidate readback, host NMS
    ~yolov9t_model() override;
};

yolov9t_model* yolov9t_load_model(char const* filepath, backend_device const& dev);

int yolov9t_anchors(int S); // (S/8)^2 + (S/16)^2 + (S/32)^2

// letterbox (yolov9t.cpp:1028-1083) of an rgb / rgba u8 image to S x S rgb_u8: image_scale, then the colour-114 border
yolo_letterbox yolov9t_letterbox(image_view const& image, int S);
// non_max_suppression (yolov9t.cpp:1145-1253) over dense outputs boxes f32 [A][4], scores f32 [A][nc]
std::vector<yolo_detection> yolov9t_nms(float const* boxes, float const* scores, int A, int nc, yolo_nms_params const& p);
// scale_boxes (yolov9t.cpp:1255-1281)
void yolov9t_scale_boxes(std::vector<yolo_detection>& d, i32x2 image_extent, float gain, float pad_w, float pad_h);

// B letterboxed u8 images [B, S, S, channels] (3 or 4, alpha ignored) on the device -> detections per image (host)
std::vector<std::vector<yolo_detection>> yolov9t_detect_batch_device(yolov9t_model&, void const* img_dev, int channels, int batch, int S,
                                                                     yolo_nms_params const& p, void* stream);
std::vector<std::vector<yolo_detection>> yolov9t_detect_batch_host(yolov9t_model&, uint8_t const* img, int channels, int batch, int S,
                                                                   yolo_nms_params const& p);
// the network on f32 rgb [n, S, S, 3] in [0, 1] (host) -> boxes f32 [n, A, 4], scores f32 [n, A, nc] (host): parity tests
void yolov9t_forward_host(yolov9t_model&, float const* rgb, int n, int S, float* boxes, float* scores);
// one image of any extent -> detections in its own pixel coordinates (inference_yolov9t.cpp:300-405)
std::vector<yolo_detection> yolov9t_detect(yolov9t_model&, image_view const& image, yolo_nms_params const& p);

} // namespace visp
