// tfl_instance.hip - the instance frames of a yh_tfl handle (DESIGN.md section 11 "TFLite instance frames"): the detections the
// TFLite tail left on the device (tfl_detect.hip) painted into packed class << 24 | id << 16 frames for the scene back-end.
//   per image         (yh_tfl_instance_batch)   inst_pack_body and inst_paint_body of instance_dev.h with the image taken from
//                     blockIdx.z, as instance_batch.hip runs them: image i is yh_instance_batch's frame i, rows of 4.
//   per camera frame  (yh_tfl_instance_frames)  classify cuts a camera frame into two S x S tiles, so after a classify batch the
//                     tail's images are tiles: frame b is painted from images 2b (the left half) and 2b + 1. Three launches:
//       tfl_inst_pack    both tiles' masks into 128-bit sets per prototype pixel: inst_pack_body unchanged, grid z = 2n images;
//       tfl_inst_order   a workgroup per frame, a lane per (tile, rank): eligibility, the frame rank q under the key (score descending
//                        in float32, tile 0 before tile 1, the smaller rank), the id counted ACROSS the tiles in frame order;
//       tfl_inst_paint   a lane per output pixel: the taps of the stitched hp x 2wp mask, each tap's tile and set, per tile the lowest
//                        bit that is on with the other tile's taps contributing nothing, both mapped to q: the smaller q wins.
// All arithmetic is integer but the two float32 comparisons named (score >= min_score, score against score); tests/tfl_instance_ref.py
// restates the definition and every result is compared with array_equal.
#include <stdio.h>
#include <string.h>

#include "tfl_instance.h"   // (first: the debug header before the public one, as yh_internal.h has it)
#include "instance_dev.h"
#include "instance_host.h"

using namespace yh;

namespace {

constexpr int kFrameRanks = 2 * kInstRanks;   // frame ranks of a camera frame: both tiles' detections
constexpr int kFrameMeta = 4 * kFrameRanks;   // words per frame: val [q], src [q], qof [tile][rank], pixel counts [q]

// grid (ceil(px / 4 / kInstPackLanes), 4, images): instance_batch.hip's kernel on the TFLite tail's buffers
__global__ void __launch_bounds__(kInstPackLanes) tfl_inst_pack(const uint8_t* __restrict__ masks, const yh_detection* __restrict__ dets,
                                                                const int* __restrict__ count, int max_n, int px,
                                                                const uint8_t* __restrict__ cmap, int ncls, float min_score,
                                                                uint32_t* __restrict__ bits, uint32_t* __restrict__ meta) {
    const size_t b = blockIdx.z;
    inst_pack_body(masks + b * max_n * px, dets + b * max_n, count + b, max_n, px, cmap, ncls, min_score, bits + b * px * 4,
                   meta + b * 2 * kInstRanks);
}

// grid (ceil(W / kInstPaintX), ceil(H / kInstPaintY), images)
__global__ void __launch_bounds__(kInstPaintX * kInstPaintY) tfl_inst_paint_image(const uint4* __restrict__ bits, int hp, int wp, int W, int H,
                                                                                  uint32_t* __restrict__ meta, uint32_t* __restrict__ out) {
    const size_t b = blockIdx.z;
    inst_paint_body(bits + b * hp * wp, hp, wp, W, H, meta + b * 2 * kInstRanks, out + b * W * H);
}

// grid (n_frames), kFrameRanks lanes: lane t = tile << 7 | rank. Eligibility is inst_rank_value's rule (the sets of tfl_inst_pack
// hold exactly the bits of the lanes that are eligible here). The frame rank of an eligible lane is the number of eligible lanes
// in front of it under the key - a larger score, or the same score and a smaller t, which is tile 0 before tile 1 and then the
// smaller rank; the id the number of eligible lanes of the same output class with a smaller frame rank. 2 x 256 compares per lane,
// all from LDS, every lane reading the same word (a broadcast). No atomics.
__global__ void __launch_bounds__(kFrameRanks) tfl_inst_order(const yh_detection* __restrict__ dets, const int* __restrict__ count, int max_n,
                                                              const uint8_t* __restrict__ cmap, int ncls, float min_score,
                                                              uint32_t* __restrict__ fmeta) {
    __shared__ uint32_t s_cls[kFrameRanks];
    __shared__ float s_score[kFrameRanks];
    __shared__ int s_q[kFrameRanks];
    __shared__ uint32_t s_val[kFrameRanks], s_src[kFrameRanks];
    const int t = threadIdx.x, tile = t / kInstRanks, r = t % kInstRanks;
    const size_t img = (size_t)blockIdx.x * 2 + tile;
    int n = count[img];
    n = n < 0 ? 0 : (n > max_n ? max_n : n);
    uint32_t c = 0;
    float sc = 0.0f;
    if (r < n) {
        const yh_detection* d = dets + img * max_n + r;
        const int k = d->class_id;
        sc = d->score;
        if (k >= 0 && k < ncls && sc >= min_score) c = cmap[k];
    }
    s_cls[t] = c; s_score[t] = sc; s_val[t] = 0; s_src[t] = 0;
    __syncthreads();
    int q = -1;
    if (c != 0) {
        q = 0;
        for (int j = 0; j < kFrameRanks; ++j) q += (s_cls[j] != 0 && (s_score[j] > sc || (s_score[j] == sc && j < t))) ? 1 : 0;
    }
    s_q[t] = q;
    __syncthreads();
    if (c != 0) {
        uint32_t id = 0;
        for (int j = 0; j < kFrameRanks; ++j) id += (s_cls[j] == c && s_q[j] < q) ? 1u : 0u;
        s_val[q] = (c << 24) | (id << 16);   // (q is a permutation of the eligible lanes onto 0 .. m - 1: no two lanes write one word)
        s_src[q] = (uint32_t)(tile << 8 | r);
    }
    __syncthreads();
    uint32_t* fm = fmeta + (size_t)blockIdx.x * kFrameMeta;
    fm[t] = s_val[t];
    fm[kFrameRanks + t] = s_src[t];
    fm[2 * kFrameRanks + t] = (uint32_t)q;
    fm[3 * kFrameRanks + t] = 0;
}

// The lowest bit that is on under the four taps' sets and weights, or -1: a bit in all four is on without arithmetic, a bit in none
// is off, a mixed bit is on iff its weighted sum S > thr (a tie is off). A tap of the other tile comes in as an empty set.
__device__ __forceinline__ int lowest_on(const uint4 ta, const uint4 tb, const uint4 tc, const uint4 td, int wa, int wb, int wc, int wd, int thr) {
    const uint32_t a[4] = { ta.x, ta.y, ta.z, ta.w }, b[4] = { tb.x, tb.y, tb.z, tb.w };
    const uint32_t c[4] = { tc.x, tc.y, tc.z, tc.w }, d[4] = { td.x, td.y, td.z, td.w };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t all = a[k] & b[k] & c[k] & d[k];
        uint32_t any = a[k] | b[k] | c[k] | d[k];
        if (all) any &= ((all & (0u - all)) << 1) - 1u;                       // nothing above the lowest certain bit can win
        for (; any != 0; any &= any - 1) {                                     // at most 32 set bits
            const uint32_t m = any & (0u - any);
            if ((all & m) != 0) return 32 * k + __builtin_ctz(m);
            const int S = ((a[k] & m) ? wa : 0) + ((b[k] & m) ? wb : 0) + ((c[k] & m) ? wc : 0) + ((d[k] & m) ? wd : 0);
            if (S > thr) return 32 * k + __builtin_ctz(m);
        }
    }
    return -1;
}

// grid (ceil(W / kInstPaintX), ceil(H / kInstPaintY), n_frames): bits [2n][hp wp] sets, fmeta [n][4][256], out [n][H][W].
// The stitched mask of a detection of tile t is its own mask on columns t wp .. (t + 1) wp - 1 of an hp x 2wp map and 0 elsewhere, so
// a tap at stitched column U reads tile U / wp's set at column U mod wp and is an empty set for the other tile. Both column taps in
// one tile (every pixel but the seam's): one search. At the seam tile 0 owns the left taps and tile 1 the right ones: two searches.
__global__ void __launch_bounds__(kInstPaintX * kInstPaintY) tfl_inst_paint_frame(const uint4* __restrict__ bits, int hp, int wp, int W, int H,
                                                                                  uint32_t* __restrict__ fmeta, uint32_t* __restrict__ out) {
    static_assert(kInstPaintX * kInstPaintY == kFrameRanks, "a lane per frame rank loads and flushes the tables");
    __shared__ uint32_t s_val[kFrameRanks];
    __shared__ int s_qof[kFrameRanks];
    __shared__ uint32_t s_hist[kFrameRanks];
    const size_t f = blockIdx.z;
    uint32_t* fm = fmeta + f * kFrameMeta;
    const int t = threadIdx.y * kInstPaintX + threadIdx.x;
    s_val[t] = fm[t]; s_qof[t] = (int)fm[2 * kFrameRanks + t]; s_hist[t] = 0;
    __syncthreads();
    const int x = blockIdx.x * kInstPaintX + threadIdx.x, y = blockIdx.y * kInstPaintY + threadIdx.y;
    if (x < W && y < H) {
        int u0, u1, fx, v0, v1, fy;
        inst_axis_taps(x, W, 2 * wp, &u0, &u1, &fx);
        inst_axis_taps(y, H, hp, &v0, &v1, &fy);
        const int t0 = u0 >= wp ? 1 : 0, t1 = u1 >= wp ? 1 : 0;
        const size_t px = (size_t)hp * wp;
        const uint4* b0 = bits + (2 * f + t0) * px + (u0 - t0 * wp);
        const uint4* b1 = bits + (2 * f + t1) * px + (u1 - t1 * wp);
        const uint4 ta = b0[v0 * wp], tb = b1[v0 * wp], tc = b0[v1 * wp], td = b1[v1 * wp];
        const int wa = (2 * W - fx) * (2 * H - fy), wb = fx * (2 * H - fy), wc = (2 * W - fx) * fy, wd = fx * fy, thr = 2 * W * H;
        int q = -1;
        if (t0 == t1) {
            const int win = lowest_on(ta, tb, tc, td, wa, wb, wc, wd, thr);
            if (win >= 0) q = s_qof[t0 * kInstRanks + win];
        } else {
            const uint4 none = make_uint4(0u, 0u, 0u, 0u);
            const int w0 = lowest_on(ta, none, tc, none, wa, wb, wc, wd, thr), w1 = lowest_on(none, tb, none, td, wa, wb, wc, wd, thr);
            const int q0 = w0 >= 0 ? s_qof[w0] : -1, q1 = w1 >= 0 ? s_qof[kInstRanks + w1] : -1;
            q = q0 < 0 ? q1 : (q1 < 0 ? q0 : (q0 < q1 ? q0 : q1));
        }
        out[(f * H + y) * W + x] = q >= 0 ? s_val[q] : 0u;
        if (q >= 0) atomicAdd(&s_hist[q], 1u);
    }
    __syncthreads();
    if (s_hist[t] != 0) atomicAdd(&fm[3 * kFrameRanks + t], s_hist[t]);
}

int fail(std::string* err, int code, const std::string& msg) { *err = msg; return code; }

#define ICHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(err, YH_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

// fmeta [4][256] as read back -> rows (tile, rank within the tile, class, id, pixels won), in frame order
void frame_table(const uint32_t* fm, std::vector<int32_t>& table) {
    table.clear();
    for (int q = 0; q < kFrameRanks && fm[q] != 0; ++q) {
        const int32_t row[5] = { (int32_t)(fm[kFrameRanks + q] >> 8), (int32_t)(fm[kFrameRanks + q] & 0xFFu), (int32_t)(fm[q] >> 24),
                                 (int32_t)((fm[q] >> 16) & 0xFFu), (int32_t)fm[3 * kFrameRanks + q] };
        table.insert(table.end(), row, row + 5);
    }
}

}  // namespace

namespace yh {

int tfl_instance_run(TflInstance& st, hipStream_t s, std::string* err, const TflInstSource& src, int n, bool per_frame, int width, int height,
                     const uint8_t* class_map, float min_score, uint32_t* out_host, bool guard) {
    const int images = per_frame ? 2 * n : n, px = src.hp * src.wp;
    const size_t npx = (size_t)width * height, frame_bytes = (size_t)n * npx * 4;
    const size_t pack_words = (size_t)images * 2 * kInstRanks, frame_words = per_frame ? (size_t)n * kFrameMeta : 0;
    st.n = -1;   // (until this batch is complete there is none: the buffers below may move)
    if (!instance_grow_bytes(&st.bits, &st.bits_cap, (size_t)images * px * 16) ||
        !instance_grow_bytes(&st.frames, &st.frames_cap, frame_bytes + 2 * kTflInstBand) ||
        !instance_grow_bytes((void**)&st.meta, &st.meta_cap, (pack_words + frame_words) * 4) ||
        !instance_grow_bytes(&st.cmap, &st.cmap_cap, (size_t)src.ncls))
        return fail(err, YH_ENOMEM, "hipMalloc instance frames");
    uint8_t* front = (uint8_t*)st.frames;
    uint32_t* frames = (uint32_t*)(front + kTflInstBand);
    uint8_t* back = front + kTflInstBand + frame_bytes;
    uint32_t* fmeta = st.meta + pack_words;
    instance_class_map(class_map, src.ncls, st.cmap_host);
    // what is read back: per image the pack's values and counts, per camera frame the order's tables and the painter's counts
    const uint32_t* meta_src = per_frame ? fmeta : st.meta;
    st.meta_host.resize(per_frame ? frame_words : pack_words);
    std::vector<uint8_t> bands;
    ICHK(hipMemcpyAsync(st.cmap, st.cmap_host.data(), (size_t)src.ncls, hipMemcpyHostToDevice, s));
    if (guard) {
        ICHK(hipMemsetAsync(front, 0xFF, kTflInstBand, s));
        ICHK(hipMemsetAsync(back, 0xFF, kTflInstBand, s));
        bands.resize(2 * kTflInstBand);
    }
    const dim3 gp((unsigned)((px + 4 * kInstPackLanes - 1) / (4 * kInstPackLanes)), kInstRanks / 32, (unsigned)images);
    hipLaunchKernelGGL(tfl_inst_pack, gp, dim3(kInstPackLanes), 0, s, src.masks, src.dets, src.count, src.max_n, px, (const uint8_t*)st.cmap,
                       src.ncls, min_score, (uint32_t*)st.bits, st.meta);
    const dim3 gq((unsigned)((width + kInstPaintX - 1) / kInstPaintX), (unsigned)((height + kInstPaintY - 1) / kInstPaintY), (unsigned)n);
    if (per_frame) {
        hipLaunchKernelGGL(tfl_inst_order, dim3((unsigned)n), dim3(kFrameRanks), 0, s, src.dets, src.count, src.max_n, (const uint8_t*)st.cmap,
                           src.ncls, min_score, fmeta);
        hipLaunchKernelGGL(tfl_inst_paint_frame, gq, dim3(kInstPaintX, kInstPaintY), 0, s, (const uint4*)st.bits, src.hp, src.wp, width, height,
                           fmeta, frames);
    } else {
        hipLaunchKernelGGL(tfl_inst_paint_image, gq, dim3(kInstPaintX, kInstPaintY), 0, s, (const uint4*)st.bits, src.hp, src.wp, width, height,
                           st.meta, frames);
    }
    ICHK(hipGetLastError());
    ICHK(hipMemcpyAsync(st.meta_host.data(), meta_src, st.meta_host.size() * 4, hipMemcpyDeviceToHost, s));
    if (guard) {
        ICHK(hipMemcpyAsync(bands.data(), front, kTflInstBand, hipMemcpyDeviceToHost, s));
        ICHK(hipMemcpyAsync(bands.data() + kTflInstBand, back, kTflInstBand, hipMemcpyDeviceToHost, s));
    }
    if (out_host) ICHK(hipMemcpyAsync(out_host, frames, frame_bytes, hipMemcpyDeviceToHost, s));
    ICHK(hipStreamSynchronize(s));
    for (size_t i = 0; i < bands.size(); ++i)
        if (bands[i] != 0xFF) {
            char at[160];
            snprintf(at, sizeof at, "instance frames op: frames %s guard, byte %zu is 0x%02X", i < kTflInstBand ? "front" : "back",
                     i < kTflInstBand ? i : i - kTflInstBand, bands[i]);
            return fail(err, YH_EOVERFLOW, at);
        }
    st.tables.resize((size_t)n);
    for (int b = 0; b < n; ++b) {
        if (per_frame) frame_table(st.meta_host.data() + (size_t)b * kFrameMeta, st.tables[b]);
        else instance_table(st.meta_host.data() + (size_t)b * 2 * kInstRanks, st.tables[b]);
    }
    st.row_width = per_frame ? 5 : 4;
    st.n = n;
    return YH_OK;
}

void tfl_instance_free(TflInstance& st) {
    void* bufs[] = { st.bits, st.frames, st.meta, st.cmap, st.op_masks, st.op_dets, st.op_counts };
    for (void* b : bufs) if (b) hipFree(b);
    st = TflInstance();
}

}  // namespace yh
