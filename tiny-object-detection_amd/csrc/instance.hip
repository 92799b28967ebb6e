// instance.hip - the instance frame (DESIGN.md section 11 "Instance frame"): one frame's detections of the last yh_evaluate - rank
// order, class, score, binary masks at prototype resolution - rasterised into the packed (class << 24 | id << 16) W x H frame the
// scene back-end reads, plus the instance table. Two kernels on the handle's stream behind the tail, outside the captured step:
//   inst_pack   per prototype pixel a 128-bit set: bit d = mask d is on there AND detection d is eligible;
//   inst_paint  a lane per output pixel: the four taps' sets, the lowest bit whose exact-integer bilinear sum passes the threshold.
// All arithmetic is integer: tests/instance_ref.py restates it and every result is compared with array_equal.
#include <math.h>
#include <string.h>

#include "engine.h"

using namespace yh;

namespace {

constexpr int kRanks = 128;        // bits of a set = yh_config.max_dets' upper bound (yh_create)
constexpr int kPackLanes = 256;    // inst_pack: lanes per workgroup, four prototype pixels each
constexpr int kPaintX = 64, kPaintY = 4;

// Eligibility, output class and id per rank, from the detections: one lane per rank, `cls` is LDS [kRanks]. Returns the lane's packed
// value class << 24 | id << 16 (0: not eligible, or no such rank); lanes >= kRanks only take part in the barrier.
__device__ __forceinline__ uint32_t rank_value(const yh_detection* __restrict__ dets, int n, const uint8_t* __restrict__ cmap, int ncls,
                                               float min_score, uint32_t* cls) {
    const int t = threadIdx.x;
    uint32_t c = 0;
    if (t < kRanks) {
        if (t < n) {
            const int k = dets[t].class_id;
            if (k >= 0 && k < ncls && dets[t].score >= min_score) c = cmap[k];
        }
        cls[t] = c;
    }
    __syncthreads();
    if (t >= kRanks || c == 0) return 0;
    uint32_t id = 0;
    for (int j = 0; j < t; ++j) id += cls[j] == c ? 1u : 0u;   // (the eligible detections of the same output class with smaller rank)
    return (c << 24) | (id << 16);
}

// grid (ceil(px / 4 / kPackLanes), 4): blockIdx.y = the set's word (ranks 32 w .. 32 w + 31), a lane = four consecutive prototype
// pixels, whose four mask bytes of one detection are one dword when the masks allow it. Only ranks below the frame's count are read:
// the slots past it are stale. Block (0, 0) also writes the packed value per rank and clears the pixel counts: meta [2][kRanks].
__global__ void __launch_bounds__(kPackLanes) inst_pack(const uint8_t* __restrict__ masks, const yh_detection* __restrict__ dets,
                                                        const int* __restrict__ count, int max_n, int px, const uint8_t* __restrict__ cmap,
                                                        int ncls, float min_score, uint32_t* __restrict__ bits, uint32_t* __restrict__ meta) {
    __shared__ uint32_t s_cls[kRanks];
    __shared__ uint32_t s_elig[kRanks / 32];
    const int t = threadIdx.x, w = blockIdx.y;
    int n = *count;
    n = n < 0 ? 0 : (n > max_n ? max_n : n);
    if (t < kRanks / 32) s_elig[t] = 0;
    const uint32_t val = rank_value(dets, n, cmap, ncls, min_score, s_cls);   // (its barrier also publishes the cleared words)
    if (t < kRanks && val != 0) atomicOr(&s_elig[t >> 5], 1u << (t & 31));
    if (blockIdx.x == 0 && w == 0 && t < kRanks) { meta[t] = val; meta[kRanks + t] = 0; }
    __syncthreads();
    const int q = (blockIdx.x * kPackLanes + t) * 4;
    if (q >= px) return;
    uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0;
    const bool dwords = (px & 3) == 0 && ((uintptr_t)masks & 3) == 0;
    for (uint32_t e = s_elig[w]; e != 0; e &= e - 1) {                         // at most 32 set bits
        const int b = __builtin_ctz(e);
        const uint8_t* m = masks + (size_t)(32 * w + b) * px + q;
        uint32_t v;
        if (dwords) v = *(const uint32_t*)m;
        else {
            v = m[0];
            if (q + 1 < px) v |= (uint32_t)m[1] << 8;
            if (q + 2 < px) v |= (uint32_t)m[2] << 16;
            if (q + 3 < px) v |= (uint32_t)m[3] << 24;
        }
        o0 |= (v & 0xFFu) ? 1u << b : 0u;
        o1 |= (v & 0xFF00u) ? 1u << b : 0u;
        o2 |= (v & 0xFF0000u) ? 1u << b : 0u;
        o3 |= (v & 0xFF000000u) ? 1u << b : 0u;
    }
    bits[(size_t)q * 4 + w] = o0;
    if (q + 1 < px) bits[(size_t)(q + 1) * 4 + w] = o1;
    if (q + 2 < px) bits[(size_t)(q + 2) * 4 + w] = o2;
    if (q + 3 < px) bits[(size_t)(q + 3) * 4 + w] = o3;
}

// One axis of the half-pixel-centre bilinear resize in integers: the two taps and the weight of the second in units of 1 / (2 out).
__device__ __forceinline__ void axis_taps(int o, int out, int in, int* t0, int* t1, int* f) {
    int nx = (2 * o + 1) * in - out;
    nx = nx < 0 ? 0 : nx;
    *t0 = nx / (2 * out);
    *f = nx - *t0 * (2 * out);
    *t1 = *t0 + 1 < in ? *t0 + 1 : in - 1;
}

// grid (ceil(W / kPaintX), ceil(H / kPaintY)), a lane per output pixel. The sets of the four taps; a bit in all four is on without
// arithmetic, a bit in none is off, a mixed bit is on iff its weighted sum S > 2 W H. The winner is the lowest bit that is on.
__global__ void __launch_bounds__(kPaintX * kPaintY) inst_paint(const uint4* __restrict__ bits, int hp, int wp, int W, int H,
                                                                uint32_t* __restrict__ meta, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_val[kRanks];
    __shared__ uint32_t s_hist[kRanks];
    const int t = threadIdx.y * kPaintX + threadIdx.x;
    if (t < kRanks) { s_val[t] = meta[t]; s_hist[t] = 0; }
    __syncthreads();
    const int x = blockIdx.x * kPaintX + threadIdx.x, y = blockIdx.y * kPaintY + threadIdx.y;
    if (x < W && y < H) {
        int u0, u1, fx, v0, v1, fy;
        axis_taps(x, W, wp, &u0, &u1, &fx);
        axis_taps(y, H, hp, &v0, &v1, &fy);
        const uint4 ta = bits[v0 * wp + u0], tb = bits[v0 * wp + u1], tc = bits[v1 * wp + u0], td = bits[v1 * wp + u1];
        const uint32_t a[4] = { ta.x, ta.y, ta.z, ta.w }, b[4] = { tb.x, tb.y, tb.z, tb.w };
        const uint32_t c[4] = { tc.x, tc.y, tc.z, tc.w }, d[4] = { td.x, td.y, td.z, td.w };
        const int wa = (2 * W - fx) * (2 * H - fy), wb = fx * (2 * H - fy), wc = (2 * W - fx) * fy, wd = fx * fy, thr = 2 * W * H;
        int win = -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (win >= 0) break;
            const uint32_t all = a[k] & b[k] & c[k] & d[k];
            uint32_t any = a[k] | b[k] | c[k] | d[k];
            if (all) any &= ((all & (0u - all)) << 1) - 1u;                  // nothing above the lowest certain bit can win
            for (; any != 0; any &= any - 1) {                                // at most 32 set bits
                const int i = __builtin_ctz(any);
                const uint32_t m = 1u << i;
                bool on = (all & m) != 0;
                if (!on) {
                    const int S = ((a[k] & m) ? wa : 0) + ((b[k] & m) ? wb : 0) + ((c[k] & m) ? wc : 0) + ((d[k] & m) ? wd : 0);
                    on = S > thr;
                }
                if (on) { win = 32 * k + i; break; }
            }
        }
        out[(size_t)y * W + x] = win >= 0 ? s_val[win] : 0u;
        if (win >= 0) atomicAdd(&s_hist[win], 1u);
    }
    __syncthreads();
    if (t < kRanks && s_hist[t] != 0) atomicAdd(&meta[kRanks + t], s_hist[t]);
}

int grow(yh_engine* h, void** p, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return YH_OK;
    if (*p) hipFree(*p);
    *p = nullptr; *cap = 0;
    if (hipMalloc(p, bytes) != hipSuccess) return h->fail(YH_ENOMEM, "hipMalloc instance frame");
    *cap = bytes;
    return YH_OK;
}

}  // namespace

namespace yh {

const char* instance_check(int width, int height, const uint8_t* class_map, int ncls, float min_score) {
    if (width < 1 || width > 4096 || height < 1 || height > 4096) return "instance frame: width and height must be in 1 .. 4096";
    if (class_map)
        for (int i = 0; i < ncls; ++i)
            if (class_map[i] > 3) return "instance frame: a class_map value is above 3";
    if (min_score != min_score) return "instance frame: min_score is NaN";
    return nullptr;
}

// One call: inst_pack, for a tracked call the tracker's kernels (instance_track.hip: inst_match rewrites the values inst_paint
// reads), inst_paint, then the one wait behind the read-back of the table (and of the slots).
static int run(yh_engine* h, const uint8_t* masks, const yh_detection* dets, const int* count, int max_n, int hp, int wp, int width,
               int height, const uint8_t* class_map, float min_score, uint32_t* out_host, const InstTrack* trk) {
    const int ncls = h->C - 1, px = hp * wp;
    const size_t npx = (size_t)width * height;
    int rc;
    h->inst_rows = -1;   // (until this frame is complete there is none: the buffers below may move)
    if ((rc = grow(h, (void**)&h->inst_bits, &h->inst_bits_cap, (size_t)px * 16))) return rc;
    if ((rc = grow(h, (void**)&h->inst_frame, &h->inst_frame_cap, npx * 4))) return rc;
    if (!h->inst_meta) {
        size_t cap = 0;
        if ((rc = grow(h, (void**)&h->inst_meta, &cap, 2 * kRanks * 4))) return rc;
        cap = 0;
        if ((rc = grow(h, (void**)&h->inst_cmap, &cap, (size_t)ncls))) return rc;
    }
    // the reference's model (yolact.rs:99-101, :113-115): foreground class 0 a red robot, 1 a blue robot, 2 a ball
    h->inst_cmap_host.assign((size_t)ncls, 0);
    for (int i = 0; i < ncls; ++i) h->inst_cmap_host[i] = class_map ? class_map[i] : (i < 3 ? (uint8_t)(i + 1) : (uint8_t)0);
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
    h->inst_table.clear();
    for (int d = 0; d < kRanks; ++d)
        if (meta[d] != 0) {
            const int32_t row[4] = { d, (int32_t)(meta[d] >> 24), (int32_t)((meta[d] >> 16) & 0xFFu), (int32_t)meta[kRanks + d] };
            h->inst_table.insert(h->inst_table.end(), row, row + 4);
        }
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
