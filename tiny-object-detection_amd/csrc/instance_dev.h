// instance_dev.h - the instance frame's device code, shared by instance.hip (one frame per launch: yh_instance_frame, yh_instance_track)
// and instance_batch.hip (n frames per launch, yh_instance_batch: the frame is blockIdx.z, the kernel advances its pointers by that
// frame and runs the same body). What is computed and why is said at the head of instance.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/yolact_hip.h"

namespace yh {

constexpr int kInstRanks = 128;        // bits of a set = yh_config.max_dets' upper bound (yh_create)
constexpr int kInstPackLanes = 256;    // inst_pack: lanes per workgroup, four prototype pixels each
constexpr int kInstPaintX = 64, kInstPaintY = 4;

// Eligibility, output class and id per rank, from the detections: one lane per rank, `cls` is LDS [kInstRanks]. Returns the lane's
// packed value class << 24 | id << 16 (0: not eligible, or no such rank); lanes >= kInstRanks only take part in the barrier.
__device__ __forceinline__ uint32_t inst_rank_value(const yh_detection* __restrict__ dets, int n, const uint8_t* __restrict__ cmap, int ncls,
                                                    float min_score, uint32_t* cls) {
    const int t = threadIdx.x;
    uint32_t c = 0;
    if (t < kInstRanks) {
        if (t < n) {
            const int k = dets[t].class_id;
            if (k >= 0 && k < ncls && dets[t].score >= min_score) c = cmap[k];
        }
        cls[t] = c;
    }
    __syncthreads();
    if (t >= kInstRanks || c == 0) return 0;
    uint32_t id = 0;
    for (int j = 0; j < t; ++j) id += cls[j] == c ? 1u : 0u;   // (the eligible detections of the same output class with smaller rank)
    return (c << 24) | (id << 16);
}

// inst_pack's body, for one frame: blockIdx.y = the set's word (ranks 32 w .. 32 w + 31), a lane = four consecutive prototype
// pixels, whose four mask bytes of one detection are one dword when the masks allow it. Only ranks below the frame's count are read:
// the slots past it are stale. Block (0, 0) also writes the packed value per rank and clears the pixel counts: meta [2][kInstRanks].
// Every pointer is the frame's own: whether the dword path may be taken is decided on `masks` as it arrives here, so a frame of a
// batch whose base is misaligned (px no multiple of four) takes the byte path whatever frame 0 does.
__device__ __forceinline__ void inst_pack_body(const uint8_t* __restrict__ masks, const yh_detection* __restrict__ dets,
                                               const int* __restrict__ count, int max_n, int px, const uint8_t* __restrict__ cmap, int ncls,
                                               float min_score, uint32_t* __restrict__ bits, uint32_t* __restrict__ meta) {
    __shared__ uint32_t s_cls[kInstRanks];
    __shared__ uint32_t s_elig[kInstRanks / 32];
    const int t = threadIdx.x, w = blockIdx.y;
    int n = *count;
    n = n < 0 ? 0 : (n > max_n ? max_n : n);
    if (t < kInstRanks / 32) s_elig[t] = 0;
    const uint32_t val = inst_rank_value(dets, n, cmap, ncls, min_score, s_cls);   // (its barrier also publishes the cleared words)
    if (t < kInstRanks && val != 0) atomicOr(&s_elig[t >> 5], 1u << (t & 31));
    if (blockIdx.x == 0 && w == 0 && t < kInstRanks) { meta[t] = val; meta[kInstRanks + t] = 0; }
    __syncthreads();
    const int q = (blockIdx.x * kInstPackLanes + t) * 4;
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
__device__ __forceinline__ void inst_axis_taps(int o, int out, int in, int* t0, int* t1, int* f) {
    int nx = (2 * o + 1) * in - out;
    nx = nx < 0 ? 0 : nx;
    *t0 = nx / (2 * out);
    *f = nx - *t0 * (2 * out);
    *t1 = *t0 + 1 < in ? *t0 + 1 : in - 1;
}

// inst_paint's body, for one frame: a lane per output pixel (blockIdx.x, blockIdx.y). The sets of the four taps; a bit in all four
// is on without arithmetic, a bit in none is off, a mixed bit is on iff its weighted sum S > 2 W H. The winner is the lowest bit
// that is on. Values and histogram are LDS arrays of the workgroup; one atomicAdd per non-zero entry goes into the frame's counts.
__device__ __forceinline__ void inst_paint_body(const uint4* __restrict__ bits, int hp, int wp, int W, int H, uint32_t* __restrict__ meta,
                                                uint32_t* __restrict__ out) {
    __shared__ uint32_t s_val[kInstRanks];
    __shared__ uint32_t s_hist[kInstRanks];
    const int t = threadIdx.y * kInstPaintX + threadIdx.x;
    if (t < kInstRanks) { s_val[t] = meta[t]; s_hist[t] = 0; }
    __syncthreads();
    const int x = blockIdx.x * kInstPaintX + threadIdx.x, y = blockIdx.y * kInstPaintY + threadIdx.y;
    if (x < W && y < H) {
        int u0, u1, fx, v0, v1, fy;
        inst_axis_taps(x, W, wp, &u0, &u1, &fx);
        inst_axis_taps(y, H, hp, &v0, &v1, &fy);
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
    if (t < kInstRanks && s_hist[t] != 0) atomicAdd(&meta[kInstRanks + t], s_hist[t]);
}

}  // namespace yh
