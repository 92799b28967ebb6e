// instance_track.hip - instance tracks (DESIGN.md section 11 "Instance tracks"): the eligible detections of a frame associated with
// the tracker's live slots by mask overlap at prototype resolution, so that the instance frame carries ids that persist. A tracked
// call is inst_pack (instance.hip, as it is), the three kernels below, then inst_paint (as it is), all on the handle's stream:
//   inst_overlap  I[s][c] = |T_s AND C_c| and A_c = |C_c| from the two 128-bit set images: a wave transposes 64 pixels' sets into 64-bit
//                 pixel masks per slot and per rank with ballots, the workgroup sums popcounts in registers, one atomicAdd per entry;
//   inst_match    one workgroup: candidates, the greedy match (as rounds of mutually best pairs), ageing, room, births; it overwrites
//                 meta[rank] with the tracked class << 24 | id << 16 and writes the rank -> slot map and the slot table;
//   inst_retrack  per prototype pixel T' = (T & keep) | permute(C).
// All arithmetic is integer: tests/track_ref.py restates it and every result is compared with array_equal.
#include <string.h>

#include "engine.h"

using namespace yh;

namespace {

constexpr int kRanks = 128;          // slots of the tracker = bits of a set (instance.hip)
constexpr int kOvLanes = 256;        // inst_overlap: four waves of 64 prototype pixels
constexpr int kOvWaves = kOvLanes / 64;
constexpr int kOvGridMax = 1024;     // workgroups (each merges at most 128 x 128 sums once)
constexpr int kMatchLanes = 1024;    // inst_match: eight lanes per slot (row pass) or per rank (column pass)
constexpr int kRetrackLanes = 256;
// the tracker's device state, i32: slots [128][4] = (class or 0: free, id, age, area), rank of slot [128] (-1: not seen by the last
// call), slot of rank [128] (-1: not eligible), keep [4] (the bits of the slots that are lost but alive)
constexpr int kStSlots = 0, kStRankOf = 4 * kRanks, kStSlotOf = 5 * kRanks, kStKeep = 6 * kRanks, kStInts = 6 * kRanks + 4;
constexpr int kStRead = kStSlotOf;   // what the host reads back: the slots and their ranks
constexpr int kOvInts = kRanks * kRanks + kRanks;   // I [128][128], then A [128]

// grid min(ceil(px / 256), kOvGridMax), a lane = a prototype pixel per round. Per round a wave turns its 64 pixels' two sets into
// 64-bit pixel masks, one per slot and one per rank (lane l keeps rows l and 64 + l), through LDS; then lane t of the workgroup
// owns slot t / 2 and the 64 ranks of half t % 2 and adds popcount(T_s & C_c) of the four waves' masks to its 64 sums.
__global__ void __launch_bounds__(kOvLanes) inst_overlap(const uint4* __restrict__ trk, const uint4* __restrict__ bits, int px,
                                                         uint32_t* __restrict__ ov) {
    __shared__ unsigned long long s_t[kOvWaves][kRanks], s_c[kOvWaves][kRanks];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, s = t >> 1, c0 = (t & 1) * 64;
    uint32_t acc[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) acc[j] = 0;
    uint32_t area = 0;
    const int groups = (px + kOvLanes - 1) / kOvLanes;
    for (int g = blockIdx.x; g < groups; g += gridDim.x) {
        const int q = g * kOvLanes + t;
        uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
        if (q < px) { a = trk[q]; b = bits[q]; }
        const uint32_t aw[4] = { a.x, a.y, a.z, a.w }, bw[4] = { b.x, b.y, b.z, b.w };
        unsigned long long ta[2] = { 0, 0 }, tc[2] = { 0, 0 };
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (__any(aw[w] != 0)) {
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const unsigned long long m = __ballot((aw[w] >> i) & 1u);
                    if (lane == ((32 * w + i) & 63)) ta[w >> 1] = m;
                }
            }
            if (__any(bw[w] != 0)) {
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const unsigned long long m = __ballot((bw[w] >> i) & 1u);
                    if (lane == ((32 * w + i) & 63)) tc[w >> 1] = m;
                }
            }
        }
        s_t[wv][lane] = ta[0]; s_t[wv][64 + lane] = ta[1];
        s_c[wv][lane] = tc[0]; s_c[wv][64 + lane] = tc[1];
        __syncthreads();
        if (t < kRanks)
            for (int k = 0; k < kOvWaves; ++k) area += (uint32_t)__popcll(s_c[k][t]);
        for (int k = 0; k < kOvWaves; ++k) {
            const unsigned long long x = s_t[k][s];
            if (x == 0) continue;
#pragma unroll
            for (int j = 0; j < 64; ++j) acc[j] += (uint32_t)__popcll(x & s_c[k][c0 + j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 64; ++j)
        if (acc[j] != 0) atomicAdd(&ov[s * kRanks + c0 + j], acc[j]);
    if (t < kRanks && area != 0) atomicAdd(&ov[kRanks * kRanks + t], area);
}

// A candidate pair; i == 0: none.
struct Cand { uint32_t i, u; int age, c, s; };

// a precedes b: the larger I / U by cross-multiplication (below 2^49), then the smaller age, the smaller rank, the smaller slot
__device__ __forceinline__ bool precedes(const Cand& a, const Cand& b) {
    if (a.i == 0) return false;
    if (b.i == 0) return true;
    const unsigned long long l = (unsigned long long)a.i * b.u, r = (unsigned long long)b.i * a.u;
    if (l != r) return l > r;
    if (a.age != b.age) return a.age < b.age;
    if (a.c != b.c) return a.c < b.c;
    return a.s < b.s;
}

// the best of the eight lanes that share a row (or a column), in every one of them
__device__ __forceinline__ Cand best_of_eight(Cand best) {
#pragma unroll
    for (int off = 4; off != 0; off >>= 1) {
        Cand o;
        o.i = __shfl_xor(best.i, off); o.u = __shfl_xor(best.u, off);
        o.age = __shfl_xor(best.age, off); o.c = __shfl_xor(best.c, off); o.s = __shfl_xor(best.s, off);
        if (precedes(o, best)) best = o;
    }
    return best;
}

// One workgroup. The greedy match is computed as rounds: the order on the candidates is total, so a pair that is the best candidate
// of its slot AND of its rank among the pairs still free is one the sequential greedy takes (nothing that could remove it precedes
// it), and taking all such pairs at once leaves the greedy's remaining problem. Every round with a candidate left matches at least
// the best one, so there are at most 128 rounds.
__global__ void __launch_bounds__(kMatchLanes) inst_match(const uint32_t* __restrict__ ov, uint32_t* __restrict__ meta,
                                                          int32_t* __restrict__ st, int iou_permille, int max_age) {
    __shared__ int s_cls[kRanks], s_id[kRanks], s_age[kRanks], s_area[kRanks];   // slots
    __shared__ int s_ccls[kRanks], s_carea[kRanks];                              // ranks: output class (0: not eligible), A_c
    __shared__ int s_slot_of[kRanks], s_rank_of[kRanks];
    __shared__ int s_rowbest[kRanks], s_colbest[kRanks], s_kill[kRanks];
    __shared__ uint32_t s_live[4], s_used[4][4], s_keep[4];
    __shared__ int s_found, s_nfree, s_unmatched;
    const int t = threadIdx.x, grp = t >> 3, part = t & 7;
    if (t < kRanks) {
        s_cls[t] = st[kStSlots + 4 * t]; s_id[t] = st[kStSlots + 4 * t + 1];
        s_age[t] = st[kStSlots + 4 * t + 2]; s_area[t] = st[kStSlots + 4 * t + 3];
        s_ccls[t] = (int)(meta[t] >> 24);
        s_carea[t] = (int)ov[kRanks * kRanks + t];
        s_slot_of[t] = -1; s_rank_of[t] = -1; s_kill[t] = 0;
    }
    if (t < 4) { s_live[t] = 0; s_keep[t] = 0; }
    if (t < 16) s_used[t >> 2][t & 3] = 0;
    if (t == 0) { s_nfree = 0; s_unmatched = 0; }
    __syncthreads();
    // steps 2 and 3
    for (int round = 0; round < kRanks; ++round) {
        if (t == 0) s_found = 0;
        Cand best = { 0, 0, 0, 0, 0 };
        if (s_cls[grp] != 0 && s_rank_of[grp] < 0) {                         // row pass: grp is a slot
            const int s = grp;
            for (int k = 0; k < kRanks / 8; ++k) {
                const int c = part + 8 * k;
                if (s_ccls[c] != s_cls[s] || s_slot_of[c] >= 0) continue;
                const uint32_t i = ov[s * kRanks + c];
                if (i == 0) continue;
                const uint32_t u = (uint32_t)s_area[s] + (uint32_t)s_carea[c] - i;
                if (1000ull * i < (unsigned long long)iou_permille * u) continue;
                const Cand k2 = { i, u, s_age[s], c, s };
                if (precedes(k2, best)) best = k2;
            }
        }
        best = best_of_eight(best);
        if (part == 0) s_rowbest[grp] = best.i != 0 ? best.c : -1;
        best = Cand{ 0, 0, 0, 0, 0 };
        if (s_ccls[grp] != 0 && s_slot_of[grp] < 0) {                        // column pass: grp is a rank
            const int c = grp;
            for (int k = 0; k < kRanks / 8; ++k) {
                const int s = part + 8 * k;
                if (s_cls[s] != s_ccls[c] || s_rank_of[s] >= 0) continue;
                const uint32_t i = ov[s * kRanks + c];
                if (i == 0) continue;
                const uint32_t u = (uint32_t)s_area[s] + (uint32_t)s_carea[c] - i;
                if (1000ull * i < (unsigned long long)iou_permille * u) continue;
                const Cand k2 = { i, u, s_age[s], c, s };
                if (precedes(k2, best)) best = k2;
            }
        }
        best = best_of_eight(best);
        if (part == 0) s_colbest[grp] = best.i != 0 ? best.s : -1;
        __syncthreads();
        if (t < kRanks) {
            const int s = s_colbest[t];
            if (s >= 0 && s_rowbest[s] == t) { s_slot_of[t] = s; s_rank_of[s] = t; s_found = 1; }
        }
        __syncthreads();
        const int found = s_found;
        __syncthreads();                                                         // (lane 0 clears s_found at the top)
        if (!found) break;
    }
    // step 4: ageing
    if (t < kRanks && s_cls[t] != 0 && s_rank_of[t] < 0) {
        if (++s_age[t] > max_age) { s_cls[t] = 0; s_id[t] = 0; s_age[t] = 0; s_area[t] = 0; }
    }
    __syncthreads();
    // step 5: room. The lost slots in the order (largest age, largest slot); the first u - free of them die.
    if (t < kRanks) {
        if (s_cls[t] == 0) atomicAdd(&s_nfree, 1);
        if (s_ccls[t] != 0 && s_slot_of[t] < 0) atomicAdd(&s_unmatched, 1);
    }
    __syncthreads();
    if (t < kRanks && s_cls[t] != 0 && s_rank_of[t] < 0) {
        int pos = 0;
        for (int o = 0; o < kRanks; ++o)
            if (s_cls[o] != 0 && s_rank_of[o] < 0 && (s_age[o] > s_age[t] || (s_age[o] == s_age[t] && o > t))) ++pos;
        s_kill[t] = pos < s_unmatched - s_nfree ? 1 : 0;
    }
    __syncthreads();
    if (t < kRanks) {
        if (s_kill[t]) { s_cls[t] = 0; s_id[t] = 0; s_age[t] = 0; s_area[t] = 0; }
        if (s_cls[t] != 0) {
            atomicOr(&s_live[t >> 5], 1u << (t & 31));
            atomicOr(&s_used[s_cls[t] & 3][(s_id[t] >> 5) & 3], 1u << (s_id[t] & 31));
            if (s_rank_of[t] < 0) atomicOr(&s_keep[t >> 5], 1u << (t & 31));
        }
    }
    __syncthreads();
    // step 6: births, in rank order
    if (t == 0) {
        for (int c = 0; c < kRanks; ++c) {
            if (s_ccls[c] == 0 || s_slot_of[c] >= 0) continue;
            int s = -1, id = -1;
            for (int w = 0; w < 4 && s < 0; ++w)
                if (~s_live[w] != 0) s = 32 * w + __builtin_ctz(~s_live[w]);
            for (int w = 0; w < 4 && id < 0; ++w)
                if (~s_used[s_ccls[c] & 3][w] != 0) id = 32 * w + __builtin_ctz(~s_used[s_ccls[c] & 3][w]);
            if (s < 0 || id < 0) continue;                                        // (cannot happen: matched + unmatched ranks <= 128)
            s_live[s >> 5] |= 1u << (s & 31);
            s_used[s_ccls[c] & 3][id >> 5] |= 1u << (id & 31);
            s_cls[s] = s_ccls[c]; s_id[s] = id;
            s_slot_of[c] = s; s_rank_of[s] = c;
        }
    }
    __syncthreads();
    // step 7 for the slot table, the maps, and the value inst_paint gives rank t
    if (t < kRanks) {
        const int r = s_rank_of[t];
        if (r >= 0) { s_age[t] = 0; s_area[t] = s_carea[r]; }
        st[kStSlots + 4 * t] = s_cls[t]; st[kStSlots + 4 * t + 1] = s_id[t];
        st[kStSlots + 4 * t + 2] = s_age[t]; st[kStSlots + 4 * t + 3] = s_area[t];
        st[kStRankOf + t] = r;
        const int s = s_slot_of[t];
        st[kStSlotOf + t] = s;
        meta[t] = s >= 0 ? ((uint32_t)s_cls[s] << 24) | ((uint32_t)s_id[s] << 16) : 0u;
    }
    if (t < 4) st[kStKeep + t] = (int32_t)s_keep[t];
}

// A lane per prototype pixel: the bits of the lost-but-alive slots stay, every bit of C moves to its rank's slot.
__global__ void __launch_bounds__(kRetrackLanes) inst_retrack(uint4* __restrict__ trk, const uint4* __restrict__ bits, int px,
                                                              const int32_t* __restrict__ st) {
    __shared__ int s_map[kRanks];
    __shared__ uint32_t s_keep[4];
    const int t = threadIdx.x;
    if (t < kRanks) s_map[t] = st[kStSlotOf + t];
    if (t < 4) s_keep[t] = (uint32_t)st[kStKeep + t];
    __syncthreads();
    const int q = blockIdx.x * kRetrackLanes + t;
    if (q >= px) return;
    const uint4 a = trk[q], b = bits[q];
    uint32_t o0 = a.x & s_keep[0], o1 = a.y & s_keep[1], o2 = a.z & s_keep[2], o3 = a.w & s_keep[3];
    const uint32_t bw[4] = { b.x, b.y, b.z, b.w };
#pragma unroll
    for (int w = 0; w < 4; ++w)
        for (uint32_t e = bw[w]; e != 0; e &= e - 1) {                          // at most 32 set bits
            const int s = s_map[32 * w + __builtin_ctz(e)];
            if (s < 0) continue;
            const uint32_t m = 1u << (s & 31);
            const int k = s >> 5;
            o0 |= k == 0 ? m : 0u; o1 |= k == 1 ? m : 0u; o2 |= k == 2 ? m : 0u; o3 |= k == 3 ? m : 0u;
        }
    trk[q] = make_uint4(o0, o1, o2, o3);
}

void drop(yh_engine* h) {
    h->trk_live = false;
    if (h->trk_rows >= 0) { h->trk_rows = 0; h->trk_table.clear(); }
}

}  // namespace

namespace yh {

const char* track_check(int iou_permille, int max_age) {
    if (iou_permille < 1 || iou_permille > 1000) return "instance track: iou_permille must be in 1 .. 1000";
    if (max_age < 0 || max_age > 255) return "instance track: max_age must be in 0 .. 255";
    return nullptr;
}

int track_enqueue(yh_engine* h, int hp, int wp, const InstTrack& trk) {
    const int px = hp * wp;
    static_assert(sizeof h->trk_host == kStRead * 4, "trk_host holds the slots and their ranks");
    if (!h->trk_ov) {
        if (hipMalloc((void**)&h->trk_ov, kOvInts * 4) != hipSuccess) return h->fail(YH_ENOMEM, "hipMalloc instance tracks");
        if (hipMalloc((void**)&h->trk_state, kStInts * 4) != hipSuccess) return h->fail(YH_ENOMEM, "hipMalloc instance tracks");
    }
    if (!h->trk_live || h->trk_hp != hp || h->trk_wp != wp) {                  // an empty tracker at this prototype size
        drop(h);
        if ((size_t)px * 16 > h->trk_img_cap) {
            if (h->trk_img) hipFree(h->trk_img);
            h->trk_img = nullptr; h->trk_img_cap = 0;
            if (hipMalloc((void**)&h->trk_img, (size_t)px * 16) != hipSuccess) return h->fail(YH_ENOMEM, "hipMalloc instance tracks");
            h->trk_img_cap = (size_t)px * 16;
        }
        HIPCHK(h, hipMemsetAsync(h->trk_img, 0, (size_t)px * 16, h->stream));
        HIPCHK(h, hipMemsetAsync(h->trk_state, 0, kStInts * 4, h->stream));
        h->trk_hp = hp; h->trk_wp = wp;
    }
    HIPCHK(h, hipMemsetAsync(h->trk_ov, 0, kOvInts * 4, h->stream));
    const int groups = (px + kOvLanes - 1) / kOvLanes;
    hipLaunchKernelGGL(inst_overlap, dim3((unsigned)(groups < kOvGridMax ? groups : kOvGridMax)), dim3(kOvLanes), 0, h->stream,
                       (const uint4*)h->trk_img, (const uint4*)h->inst_bits, px, h->trk_ov);
    hipLaunchKernelGGL(inst_match, dim3(1), dim3(kMatchLanes), 0, h->stream, (const uint32_t*)h->trk_ov, h->inst_meta, h->trk_state,
                       trk.iou_permille, trk.max_age);
    hipLaunchKernelGGL(inst_retrack, dim3((unsigned)((px + kRetrackLanes - 1) / kRetrackLanes)), dim3(kRetrackLanes), 0, h->stream,
                       h->trk_img, (const uint4*)h->inst_bits, px, (const int32_t*)h->trk_state);
    HIPCHK(h, hipGetLastError());
    h->trk_live = true;
    return YH_OK;
}

int track_readback(yh_engine* h) {
    HIPCHK(h, hipMemcpyAsync(h->trk_host, h->trk_state, sizeof h->trk_host, hipMemcpyDeviceToHost, h->stream));
    return YH_OK;
}

void track_finish(yh_engine* h) {
    const int32_t* st = h->trk_host;
    h->trk_table.clear();
    for (int s = 0; s < kRanks; ++s)
        if (st[kStSlots + 4 * s] != 0) {
            const int32_t row[6] = { s, st[4 * s], st[4 * s + 1], st[4 * s + 2], st[4 * s + 3], st[kStRankOf + s] };
            h->trk_table.insert(h->trk_table.end(), row, row + 6);
        }
    h->trk_rows = (int)(h->trk_table.size() / 6);
}

void track_drop(yh_engine* h) { drop(h); }

void track_free(yh_engine* h) {
    if (h->trk_img) hipFree(h->trk_img);
    if (h->trk_ov) hipFree(h->trk_ov);
    if (h->trk_state) hipFree(h->trk_state);
}

}  // namespace yh

extern "C" {

int yh_instance_track(yh_engine* h, int32_t frame, int32_t width, int32_t height, const uint8_t* class_map, float min_score,
                      int32_t iou_permille, int32_t max_age, uint32_t* out_host) {
    if (!h) return YH_EINVAL;
    if (!h->dets_valid) return h->fail(YH_ESTATE, "instance track: the handle's last step was not a yh_evaluate");
    if (frame < 0 || frame >= h->cur_n) return h->fail(YH_EINVAL, "instance track: frame out of range");
    if (const char* why = instance_check(width, height, class_map, h->C - 1, min_score)) return h->fail(YH_EINVAL, why);
    if (const char* why = track_check(iou_permille, max_age)) return h->fail(YH_EINVAL, why);
    HIPCHK(h, hipSetDevice(h->dev));
    TraceRange tr("yh_instance_track");
    const size_t px = (size_t)h->hp * h->wp, md = (size_t)h->cfg.max_dets;
    const InstTrack trk = { iou_permille, max_age };
    return instance_run(h, h->det.masks + (size_t)frame * md * px, h->det.dets + (size_t)frame * md, h->det.det_count + frame, (int)md,
                        h->hp, h->wp, width, height, class_map, min_score, out_host, &trk);
}

int yh_instance_tracks_read(yh_engine* h, int32_t* n_tracks, int32_t* table, int32_t capacity) {
    if (!h || !n_tracks) return YH_EINVAL;
    if (h->trk_rows < 0) return h->fail(YH_ESTATE, "track table: no tracked call yet");
    *n_tracks = h->trk_rows;
    if (!table) return YH_OK;
    if (capacity < h->trk_rows) return h->fail(YH_EOVERFLOW, "track table: capacity too small");
    memcpy(table, h->trk_table.data(), h->trk_table.size() * sizeof(int32_t));
    return YH_OK;
}

int yh_instance_track_reset(yh_engine* h) {
    if (!h) return YH_EINVAL;
    drop(h);
    return YH_OK;
}

}  // extern "C"
