// tfl_instance.h - the instance frames of a yh_tfl handle (DESIGN.md section 11 "TFLite instance frames"): what tfl_instance.hip
// (the kernels and the one call that runs them) and tflite_exec.hip (the yh_tfl_* C ABI) share. Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/yolact_hip_debug.h"

namespace yh __attribute__((visibility("hidden"))) {

constexpr size_t kTflInstBand = 4096;   // bytes in front of and behind the frames: yh_tfl_op_instance_frames' guard bands
constexpr int kTflOpClasses = 80;       // foreground classes (and class_map entries) of yh_tfl_op_instance_frames: the tail's limit - 1

// The handle's one instance batch: device buffers of its own, allocated at the first call, grow only, freed by tfl_instance_free.
struct TflInstance {
    void *bits = nullptr, *frames = nullptr, *cmap = nullptr;   // sets [images][px][4 words]; band | frames [n][H][W] | band; class map
    uint32_t* meta = nullptr;   // [images][2][128] (inst_pack_body's values and counts), then [n_frames][4][256] (val, src, qof, pixel counts by frame rank)
    size_t bits_cap = 0, frames_cap = 0, cmap_cap = 0, meta_cap = 0;
    // yh_tfl_op_instance_frames' uploads
    void *op_masks = nullptr, *op_dets = nullptr, *op_counts = nullptr;
    size_t op_masks_cap = 0, op_dets_cap = 0, op_counts_cap = 0;
    std::vector<uint8_t> cmap_host;
    std::vector<uint32_t> meta_host;
    std::vector<std::vector<int32_t>> tables;
    int n = -1;          // frames of the last batch; -1: no batch
    int row_width = 4;   // 4: per image (yh_tfl_instance_batch), 5: per camera frame (yh_tfl_instance_frames)
};

// The detections a batch is painted from, as the tail left them: image i reads masks + i max_n hp wp, dets + i max_n, count + i.
struct TflInstSource { const uint8_t* masks; const yh_detection* dets; const int* count; int max_n, hp, wp, ncls; };

// n images (per_frame = false: inst_pack_body / inst_paint_body per image, rows of 4) or n camera frames of two tiles each
// (per_frame: pack, order, stitched paint, rows of 5) in one set of launches on `s`: one class-map upload, one read-back, one wait.
// Everything has been checked by the caller. guard: the frames' bands are painted 0xFF before and read back and checked behind the
// launches (YH_EOVERFLOW names the band). A failure leaves no batch and its text in *err.
int tfl_instance_run(TflInstance& st, hipStream_t s, std::string* err, const TflInstSource& src, int n, bool per_frame, int width, int height,
                     const uint8_t* class_map, float min_score, uint32_t* out_host, bool guard);
inline const uint32_t* tfl_instance_frames(const TflInstance& st) {
    return st.n >= 1 ? (const uint32_t*)((const char*)st.frames + kTflInstBand) : nullptr;
}
void tfl_instance_free(TflInstance& st);

}  // namespace yh
