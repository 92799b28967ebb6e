// instance.hip - the instance frame (DESIGN.md section 11 "Instance frame"): one frame's detections of the last yh_evaluate - rank
// order, class, score, binary masks at prototype resolution - rasterised into the packed (class << 24 | id << 16) W x H frame the
// scene back-end reads, plus the instance table. Two kernels on the handle's stream behind the tail, outside the captured step:
//   inst_pack   per prototype pixel a 128-bit set: bit d = mask d is on there AND detection d is eligible;
//   inst_paint  a lane per output pixel: the four taps' sets, the lowest bit whose exact-integer bilinear sum passes the threshold.
// All arithmetic is integer: tests/instance_ref.py restates it and every result is compared with array_equal.
#include <math.h>
#include <string.h>

#include "engine.h"
#include "instance_dev.h"

using namespace yh;

namespace {

constexpr int kRanks = kInstRanks, kPackLanes = kInstPackLanes, kPaintX = kInstPaintX, kPaintY = kInstPaintY;

// The bodies of both kernels are instance_dev.h's (instance_batch.hip runs the same ones per frame of a batch).
// grid (ceil(px / 4 / kPackLanes), 4)
__global__ void __launch_bounds__(kPackLanes) inst_pack(const uint8_t* __restrict__ masks, const yh_detection* __restrict__ dets,
                                                        const int* __restrict__ count, int max_n, int px, const uint8_t* __restrict__ cmap,
                                                        int ncls, float min_score, uint32_t* __restrict__ bits, uint32_t* __restrict__ meta) {
    inst_pack_body(masks, dets, count, max_n, px, cmap, ncls, min_score, bits, meta);
}

// grid (ceil(W / kPaintX), ceil(H / kPaintY))
__global__ void __launch_bounds__(kPaintX * kPaintY) inst_paint(const uint4* __restrict__ bits, int hp, int wp, int W, int H,
                                                                uint32_t* __restrict__ meta, uint32_t* __restrict__ out) {
    inst_paint_body(bits, hp, wp, W, H, meta, out);
}

}  // namespace

namespace yh {

bool instance_grow_bytes(void** p, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return true;
    if (*p) hipFree(*p);
    *p = nullptr; *cap = 0;
    if (hipMalloc(p, bytes) != hipSuccess) { *p = nullptr; return false; }
    *cap = bytes;
    return true;
}

int instance_grow(yh_engine* h, void** p, size_t* cap, size_t bytes) {
    return instance_grow_bytes(p, cap, bytes) ? YH_OK : h->fail(YH_ENOMEM, "hipMalloc instance frame");
}

void instance_table(const uint32_t* meta, std::vector<int32_t>& table) {
    table.clear();
    for (int d = 0; d < kRanks; ++d)
        if (meta[d] != 0) {
            const int32_t row[4] = { d, (int32_t)(meta[d] >> 24), (int32_t)((meta[d] >> 16) & 0xFFu), (int32_t)meta[kRanks + d] };
            table.insert(table.end(), row, row + 4);
        }
}

const char* instance_check(int width, int height, const uint8_t* class_map, int ncls, float min_score) {
    if (width < 1 || width > 4096 || height < 1 || height > 4096) return "instance frame: width and height must be in 1 .. 4096";
    if (class_map)
        for (int i = 0; i < ncls; ++i)
            if (class_map[i] > 3) return "instance frame: a class_map value is above 3";
    if (min_score != min_score) return "instance frame: min_score is NaN";
    return nullptr;
}

// NULL: the reference's model (yolact.rs:99-101, :113-115): foreground class 0 a red robot, 1 a blue robot, 2 a ball
void instance_class_map(const uint8_t* class_map, int ncls, std::vector<uint8_t>& out) {
    out.assign((size_t)ncls, 0);
    for (int i = 0; i < ncls; ++i) out[i] = class_map ? class_map[i] : (i < 3 ? (uint8_t)(i + 1) : (uint8_t)0);
}

// One call: inst_pack, for a tracked call the tracker's kernels (instance_track.hip: inst_match rewrites the values inst_paint
// reads), inst_paint, then the one wait behind the read-back of the table (and of the slots).
static int run(yh_engine* h, const uint8_t* masks, const yh_detection* dets, const int* count, int max_n, int hp, int wp, int width,
               int height, const uint8_t* class_map, float min_score, uint32_t* out_host, const InstTrack* trk) {
    const int ncls = h->C - 1, px = hp * wp;
    const size_t npx = (size_t)width * height;
    int rc;
    h->inst_rows = -1;   // (until this frame is complete there is none: the buffers below may move)
    if ((rc = instance_grow(h, (void**)&h->inst_bits, &h->inst_bits_cap, (size_t)px * 16))) return rc;
    if ((rc = instance_grow(h, (void**)&h->inst_frame, &h->inst_frame_cap, npx * 4))) return rc;
    if (!h->inst_meta) {
        size_t cap = 0;
        if ((rc = instance_grow(h, (void**)&h->inst_meta, &cap, 2 * kRanks * 4))) return rc;
        cap = 0;
        if ((rc = instance_grow(h, (void**)&h->inst_cmap, &cap, (size_t)ncls))) return rc;
    }
    instance_class_map(class_map, ncls, h->inst_cmap_host);
    HIPCHK(h, hipMemcpyAsync(h->inst_cmap, h->inst_cmap_host.data(), (size_t)ncls, hipMemcpyHostToDevice, h->stream));
    const dim3 gp((unsigned)((px + 4 * kPackLanes - 1) / (4 * kPackLanes)), kRanks / 32);
    hipLaunchKernelGGL(inst_pack, gp, dim3(kPackLanes), 0, h->stream, masks, dets, count, max_n, px, (const uint8_t*)h->inst_cmap, ncls,
                       min_score, (uint32_t*)h->inst_bits, h->inst_meta);
    if (trk && (rc = track_enqueue(h, hp, wp, *trk))) return rc;
    const dim3 gq((unsigned)((width + kPaintX - 1) / kPaintX), (unsigned)((height + kPaintY - 1) / kPaintY));
    hipLaunchKernelGGL(inst_paint, gq, dim3(kPaintX, kPaintY), 0, h->stream, (const uint4*)h->inst_bits, hp, wp, width, height, h->inst_meta,
                       h->inst_frame);
    HIPCHK(h, hipGetLastError());
    uint32_t* meta = h->inst_meta_host;
    static_assert(sizeof h->inst_meta_host == 2 * kRanks * 4, "inst_meta_host holds the values and the counts of every rank");
    HIPCHK(h, hipMemcpyAsync(meta, h->inst_meta, sizeof h->inst_meta_host, hipMemcpyDeviceToHost, h->stream));
    if (trk && (rc = track_readback(h))) return rc;
    if (out_host) HIPCHK(h, hipMemcpyAsync(out_host, h->inst_frame, npx * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (trk) track_finish(h);
    instance_table(meta, h->inst_table);
    h->inst_rows = (int)(h->inst_table.size() / 4);
    return YH_OK;
}

int instance_run(yh_engine* h, const uint8_t* masks, const yh_detection* dets, const int* count, int max_n, int hp, int wp,
                 int width, int height, const uint8_t* class_map, float min_score, uint32_t* out_host, const InstTrack* trk) {
    const int rc = run(h, masks, dets, count, max_n, hp, wp, width, height, class_map, min_score, out_host, trk);
    if (rc != YH_OK && trk) track_drop(h);   // a tracked call that failed leaves an empty tracker (and, as any failed call, no frame)
    return rc;
}

void instance_free(yh_engine* h) {
    if (h->inst_bits) hipFree(h->inst_bits);
    if (h->inst_frame) hipFree(h->inst_frame);
    if (h->inst_meta) hipFree(h->inst_meta);
    if (h->inst_cmap) hipFree(h->inst_cmap);
    instance_batch_free(h);
    track_free(h);
}

}  // namespace yh

extern "C" {

int yh_instance_frame(yh_engine* h, int32_t frame, int32_t width, int32_t height, const uint8_t* class_map, float min_score,
                      uint32_t* out_host) {
    if (!h) return YH_EINVAL;
    if (!h->dets_valid) return h->fail(YH_ESTATE, "instance frame: the handle's last step was not a yh_evaluate");
    if (frame < 0 || frame >= h->cur_n) return h->fail(YH_EINVAL, "instance frame: frame out of range");
    if (const char* why = instance_check(width, height, class_map, h->C - 1, min_score)) return h->fail(YH_EINVAL, why);
    HIPCHK(h, hipSetDevice(h->dev));
    TraceRange tr("yh_instance_frame");
    const size_t px = (size_t)h->hp * h->wp, md = (size_t)h->cfg.max_dets;
    return instance_run(h, h->det.masks + (size_t)frame * md * px, h->det.dets + (size_t)frame * md, h->det.det_count + frame, (int)md,
                        h->hp, h->wp, width, height, class_map, min_score, out_host);
}

const uint32_t* yh_instance_device_frame(const yh_engine* h) { return h && h->inst_rows >= 0 ? h->inst_frame : nullptr; }

int yh_instance_read(yh_engine* h, int32_t* n_instances, int32_t* table, int32_t capacity) {
    if (!h || !n_instances) return YH_EINVAL;
    if (h->inst_rows < 0) return h->fail(YH_ESTATE, "instance table: no instance frame yet");
    *n_instances = h->inst_rows;
    if (!table) return YH_OK;
    if (capacity < h->inst_rows) return h->fail(YH_EOVERFLOW, "instance table: capacity too small");
    memcpy(table, h->inst_table.data(), h->inst_table.size() * sizeof(int32_t));
    return YH_OK;
}

}  // extern "C"
