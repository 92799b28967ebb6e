// tfl_detect.h — the detection tail on a TFLite model's own output tensors (DESIGN.md section 11 "TFLite detections"): what
// tfl_detect.hip (the kernels) and tflite_exec.hip (the yh_tfl_* C ABI) share. Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/yolact_hip_debug.h"   // (yh_detection; the debug header first, as yh_internal.h has it)

namespace yh __attribute__((visibility("hidden"))) {

enum { TQ_U8 = 0, TQ_I8 = 1, TQ_F32 = 2 };
// One head tensor as it lies in device memory: image-major, `stride` ELEMENTS per image. A quantised element's value is
// (float)(q - zp) * scale (one f32 multiply); an f32 element is itself.
struct TflHead { const void* p; int kind; float scale; int zp; long long stride; };

// Limits of the tail (the engine's: detect.hip)
constexpr int kTdTopkMax = 256, kTdDetsMax = 128, kTdSlotsMax = 16384, kTdClassesMax = 81;

struct TflDetectParams {
    TflHead loc, conf, mask, proto;   // [n][P][4], [n][P][C], [n][P][32], [n][hp][wp][32]
    const float* priors;              // [P][4] cx, cy, w, h: indexed by the prior, no anchors-per-cell structure
    int n, P, C, hp, wp, top_k, max_dets;
    int int_mask;                     // mask and proto are both quantised: the mask bit is the sign of the exact integer sum (rule 3)
    float conf_thresh, nms_thresh;
    // workspaces, as DetectParams
    int* cls_count;       // [n][C-1]
    uint2* cand;          // [n][C-1][P]  {score bits, prior}
    float* surv_score;    // [n][(C-1)*top_k]  (-1: empty)
    int* surv_prior;
    float* surv_box;      // [..][4]
    int* det_count;       // [n]
    yh_detection* dets;   // [n][max_dets]
    float* det_crop;      // [n][max_dets][4]  xa, xb, ya, yb
    // a detection's 32 mask coefficients: int_mask ? 8 dwords of bytes in the uint8 domain (int8 bytes with the top bit flipped)
    // at [..][8] : 32 dequantised f32 at [..][32]
    void* det_coef;
    int* det_csum;        // [n][max_dets]: int_mask: the sum of those 32 bytes
    uint8_t* masks;       // [n][max_dets][hp*wp]
};

int tfl_detect_launch_count();
const char* tfl_detect_stage_name(int stage);
hipError_t launch_tfl_detect_stage(const TflDetectParams& p, int stage, hipStream_t s);
hipError_t launch_tfl_detect(const TflDetectParams& p, hipStream_t s);

}  // namespace yh
