// instance_batch.hip - yh_instance_batch: the instance frames of n frames of the last yh_evaluate in one pair of launches (DESIGN.md
// section 11 "Instance batch"). Frame b of a batch has exactly the packed frame and the instance table yh_instance_frame gives for
// frame first + b: both kernels here take their frame from blockIdx.z, advance their pointers by that frame and run the body the
// single call's kernel runs (instance_dev.h) - there is no second definition of anything. One upload of the class map, one read-back
// of n x 1 KB of values and counts (and of the frames, if the caller wants them on the host), one wait. The buffers are the
// batch's own: a batch neither reads nor writes what yh_instance_frame, yh_instance_track and their readers use, and those calls
// leave the batch alone. A tracked batch (yh_instance_track_batch, instance_track_batch.hip) is this call with the trackers' rounds
// between the two launches: each frame is matched against the tracker of its camera stream, frames of one stream in batch order.
#include <string.h>

#include "engine.h"
#include "instance_dev.h"

using namespace yh;

namespace {

// grid (ceil(px / 4 / kInstPackLanes), 4, n). Frame b reads masks + b max_n px: whether its four mask bytes may be read as one dword
// is decided per frame, on the advanced pointer, by the body's own test ((px & 3) == 0 && the pointer is aligned) - with px no
// multiple of four the bases of frames 1, 2, ... are misaligned even where frame 0's is not.
__global__ void __launch_bounds__(kInstPackLanes) inst_batch_pack(const uint8_t* __restrict__ masks, const yh_detection* __restrict__ dets,
                                                                  const int* __restrict__ count, int max_n, int px,
                                                                  const uint8_t* __restrict__ cmap, int ncls, float min_score,
                                                                  uint32_t* __restrict__ bits, uint32_t* __restrict__ meta) {
    const size_t b = blockIdx.z;
    inst_pack_body(masks + b * max_n * px, dets + b * max_n, count + b, max_n, px, cmap, ncls, min_score, bits + b * px * 4,
                   meta + b * 2 * kInstRanks);
}

// grid (ceil(W / kInstPaintX), ceil(H / kInstPaintY), n): bits [n][hp wp], meta [n][2][128], out [n][H][W]
__global__ void __launch_bounds__(kInstPaintX * kInstPaintY) inst_batch_paint(const uint4* __restrict__ bits, int hp, int wp, int W, int H,
                                                                              uint32_t* __restrict__ meta, uint32_t* __restrict__ out) {
    const size_t b = blockIdx.z;
    inst_paint_body(bits + b * hp * wp, hp, wp, W, H, meta + b * 2 * kInstRanks, out + b * W * H);
}

}  // namespace

namespace yh {

// One call: inst_batch_pack, for a tracked batch the trackers' rounds (instance_track_batch.hip: inst_track_match rewrites the values
// inst_batch_paint reads), inst_batch_paint, then the one wait behind the read-back of the tables (and of the slots).
static int run(yh_engine* h, const uint8_t* masks, const yh_detection* dets, const int* count, int max_n, int n, int hp, int wp,
               int width, int height, const uint8_t* class_map, float min_score, uint32_t* out_host, const InstTrackBatch* trk) {
    const int ncls = h->C - 1, px = hp * wp;
    const size_t npx = (size_t)width * height, meta_words = (size_t)n * 2 * kInstRanks;
    int rc;
    h->instb_n = -1;   // (until this batch is complete there is none: the buffers below may move)
    h->trkb_n = -1;
    if ((rc = instance_grow(h, (void**)&h->instb_bits, &h->instb_bits_cap, (size_t)n * px * 16))) return rc;
    if ((rc = instance_grow(h, (void**)&h->instb_frames, &h->instb_frames_cap, (size_t)n * npx * 4))) return rc;
    if ((rc = instance_grow(h, (void**)&h->instb_meta, &h->instb_meta_cap, meta_words * 4))) return rc;
    if ((rc = instance_grow(h, (void**)&h->instb_cmap, &h->instb_cmap_cap, (size_t)ncls))) return rc;
    instance_class_map(class_map, ncls, h->instb_cmap_host);
    h->instb_meta_host.resize(meta_words);
    HIPCHK(h, hipMemcpyAsync(h->instb_cmap, h->instb_cmap_host.data(), (size_t)ncls, hipMemcpyHostToDevice, h->stream));
    const dim3 gp((unsigned)((px + 4 * kInstPackLanes - 1) / (4 * kInstPackLanes)), kInstRanks / 32, (unsigned)n);
    hipLaunchKernelGGL(inst_batch_pack, gp, dim3(kInstPackLanes), 0, h->stream, masks, dets, count, max_n, px, (const uint8_t*)h->instb_cmap,
                       ncls, min_score, (uint32_t*)h->instb_bits, h->instb_meta);
    if (trk && (rc = track_batch_enqueue(h, n, hp, wp, *trk))) return rc;
    const dim3 gq((unsigned)((width + kInstPaintX - 1) / kInstPaintX), (unsigned)((height + kInstPaintY - 1) / kInstPaintY), (unsigned)n);
    hipLaunchKernelGGL(inst_batch_paint, gq, dim3(kInstPaintX, kInstPaintY), 0, h->stream, (const uint4*)h->instb_bits, hp, wp, width, height,
                       h->instb_meta, h->instb_frames);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(h->instb_meta_host.data(), h->instb_meta, meta_words * 4, hipMemcpyDeviceToHost, h->stream));
    if (trk && (rc = track_batch_readback(h, n))) return rc;
    if (out_host) HIPCHK(h, hipMemcpyAsync(out_host, h->instb_frames, (size_t)n * npx * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->instb_tables.resize((size_t)n);
    for (int b = 0; b < n; ++b) instance_table(h->instb_meta_host.data() + (size_t)b * 2 * kInstRanks, h->instb_tables[b]);
    if (trk) track_batch_finish(h, n, *trk);
    h->instb_n = n;
    return YH_OK;
}

int instance_batch_run(yh_engine* h, const uint8_t* masks, const yh_detection* dets, const int* count, int max_n, int n, int hp, int wp,
                       int width, int height, const uint8_t* class_map, float min_score, uint32_t* out_host, const InstTrackBatch* trk) {
    const int rc = run(h, masks, dets, count, max_n, n, hp, wp, width, height, class_map, min_score, out_host, trk);
    if (rc != YH_OK && trk) track_batch_drop(h, n, *trk);   // a tracked batch that failed leaves no batch and empties every tracker it named
    return rc;
}

void instance_batch_free(yh_engine* h) {
    void* bufs[] = { h->instb_bits, h->instb_frames, h->instb_meta, h->instb_cmap };
    for (void* b : bufs) if (b) hipFree(b);
}

}  // namespace yh

extern "C" {

int yh_instance_batch(yh_engine* h, int32_t first_frame, int32_t n_frames, int32_t width, int32_t height, const uint8_t* class_map,
                      float min_score, uint32_t* out_host) {
    if (!h) return YH_EINVAL;
    if (!h->dets_valid) return h->fail(YH_ESTATE, "instance batch: the handle's last step was not a yh_evaluate");
    if (n_frames < 1) return h->fail(YH_EINVAL, "instance batch: n_frames must be at least 1");
    if (first_frame < 0 || first_frame >= h->cur_n || n_frames > h->cur_n - first_frame)
        return h->fail(YH_EINVAL, "instance batch: frames outside the last step's batch");
    if (const char* why = instance_check(width, height, class_map, h->C - 1, min_score)) return h->fail(YH_EINVAL, why);
    HIPCHK(h, hipSetDevice(h->dev));
    TraceRange tr("yh_instance_batch");
    const size_t px = (size_t)h->hp * h->wp, md = (size_t)h->cfg.max_dets;
    return instance_batch_run(h, h->det.masks + (size_t)first_frame * md * px, h->det.dets + (size_t)first_frame * md,
                              h->det.det_count + first_frame, (int)md, n_frames, h->hp, h->wp, width, height, class_map, min_score, out_host);
}

const uint32_t* yh_instance_batch_device_frames(const yh_engine* h) { return h && h->instb_n >= 1 ? h->instb_frames : nullptr; }

int yh_instance_batch_read(yh_engine* h, int32_t frame, int32_t* n_instances, int32_t* table, int32_t capacity) {
    if (!h || !n_instances) return YH_EINVAL;
    if (h->instb_n < 1) return h->fail(YH_ESTATE, "instance batch table: no instance batch yet");
    if (frame < 0 || frame >= h->instb_n) return h->fail(YH_EINVAL, "instance batch table: frame outside the last batch");
    const std::vector<int32_t>& t = h->instb_tables[(size_t)frame];
    *n_instances = (int32_t)(t.size() / 4);
    if (!table) return YH_OK;
    if (capacity < *n_instances) return h->fail(YH_EOVERFLOW, "instance batch table: capacity too small");
    memcpy(table, t.data(), t.size() * sizeof(int32_t));
    return YH_OK;
}

}  // extern "C"
