// classify_geo.h - the frame-major front and back end of a classify batch, for whichever handle runs the network in the middle
// (classify_batch.hip holds the kernels: resize_tables, classify_pre_batch, classify_post_batch). yh_engine's batch
// (yh_classify_batch_u32) and yh_tfl's (yh_tfl_classify_batch_u32) each own one ClassifyGeo record and call these with their own
// stream: the same tables, the same LDS-or-fallback choice and the same launches for one geometry (W, H, S). Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// (hidden: nothing declared here is exported from the shared library)
namespace yh __attribute__((visibility("hidden"))) {

// One Triangle resize table of the classify batch (resize_tables): for output index o the source window win[o] = (left, n) and its
// n weights w[o * pitch ..], each the quotient tri_w / sum the single-frame kernels form per lane.
struct ResizeTab { int2* win; float* w; int pitch, in_size, out_size; };

// The tables of one geometry and the plan of the pre kernel at it. The allocation grows only; classify_geo_free releases it.
struct ClassifyGeo {
    void* tab = nullptr;        // the four tables' one allocation
    size_t tab_cap = 0;
    ResizeTab tabs[4] = {};     // vertical H -> S, horizontal W -> 2S, vertical S -> H, horizontal 2S -> W
    int w = 0, h = 0, S = 0;    // the geometry the tables were built for (0: none)
    int pre_cols = 0;           // LDS columns of a classify_pre_batch block at this geometry; 0: the fallback form
};

// The tables of (w, h, S) exist on the device (enqueued on `s` if they had to be built). hipErrorOutOfMemory: the allocation failed.
hipError_t classify_geo_ensure(ClassifyGeo* g, int w, int h, int S, hipStream_t s);
// frames [n][h][w] packed -> RGB8 tiles [2n][S][S][3] (frame b: tiles 2b, 2b + 1)
hipError_t classify_geo_pre(const ClassifyGeo& g, const uint32_t* frames, int n, uint8_t* tiles, hipStream_t s);
// codes [2n][(S / 8)^2] -> packed frames [n][h][w]
hipError_t classify_geo_post(const ClassifyGeo& g, const uint32_t* codes, int n, uint32_t* out, hipStream_t s);
void classify_geo_free(ClassifyGeo* g);

}  // namespace yh
