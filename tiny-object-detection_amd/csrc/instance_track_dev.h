// instance_track_dev.h - the tracker's device code, shared by instance_track.hip (one frame per call, yh_instance_track: inst_overlap,
// inst_match, inst_retrack) and instance_track_batch.hip (n frames of a step in rounds, yh_instance_track_batch: inst_track_sweep,
// inst_track_match, which take their stream and frame from a descriptor, advance their pointers and run the same bodies). What is
// computed and why is said at the head of instance_track.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace yh {

constexpr int kTrkRanks = 128;          // slots of the tracker = bits of a set (instance.hip)
constexpr int kTrkOvLanes = 256;        // inst_overlap: four waves of 64 prototype pixels
constexpr int kTrkOvWaves = kTrkOvLanes / 64;
constexpr int kTrkOvGridMax = 1024;     // workgroups (each merges at most 128 x 128 sums once)
constexpr int kTrkMatchLanes = 1024;    // inst_match: eight lanes per slot (row pass) or per rank (column pass)
constexpr int kTrkRetrackLanes = 256;
// the tracker's device state, i32: slots [128][4] = (class or 0: free, id, age, area), rank of slot [128] (-1: not seen by the last
// call), slot of rank [128] (-1: not eligible), keep [4] (the bits of the slots that are lost but alive)
constexpr int kTrkStSlots = 0, kTrkStRankOf = 4 * kTrkRanks, kTrkStSlotOf = 5 * kTrkRanks, kTrkStKeep = 6 * kTrkRanks,
              kTrkStInts = 6 * kTrkRanks + 4;
constexpr int kTrkStRead = kTrkStSlotOf;   // what the host reads back: the slots and their ranks
constexpr int kTrkOvInts = kTrkRanks * kTrkRanks + kTrkRanks;   // I [128][128], then A [128]

// One round of inst_overlap, by the whole workgroup of kTrkOvLanes lanes: lane t brings the two sets a (tracks) and b (ranks) of its
// prototype pixel (zero: no pixel). A wave turns its 64 pixels' sets into 64-bit pixel masks, one per slot and one per rank (lane l
// keeps rows l and 64 + l), through LDS; then lane t owns slot t / 2 and the 64 ranks of half t % 2 and adds popcount(T_s & C_c) of
// the four waves' masks to its 64 sums; lanes 0 .. 127 add the rank's pixels to `area`.
__device__ __forceinline__ void inst_overlap_group(const uint4 a, const uint4 b, uint32_t (&acc)[64], uint32_t& area) {
    __shared__ unsigned long long s_t[kTrkOvWaves][kTrkRanks], s_c[kTrkOvWaves][kTrkRanks];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, s = t >> 1, c0 = (t & 1) * 64;
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
    if (t < kTrkRanks)
        for (int k = 0; k < kTrkOvWaves; ++k) area += (uint32_t)__popcll(s_c[k][t]);
    for (int k = 0; k < kTrkOvWaves; ++k) {
        const unsigned long long x = s_t[k][s];
        if (x == 0) continue;
#pragma unroll
        for (int j = 0; j < 64; ++j) acc[j] += (uint32_t)__popcll(x & s_c[k][c0 + j]);
    }
    __syncthreads();
}

// The workgroup's sums into the matrix: ov = I [128][128] then A [128], one atomicAdd per non-zero entry.
__device__ __forceinline__ void inst_overlap_merge(const uint32_t (&acc)[64], uint32_t area, uint32_t* __restrict__ ov) {
    const int t = threadIdx.x, s = t >> 1, c0 = (t & 1) * 64;
#pragma unroll
    for (int j = 0; j < 64; ++j)
        if (acc[j] != 0) atomicAdd(&ov[s * kTrkRanks + c0 + j], acc[j]);
    if (t < kTrkRanks && area != 0) atomicAdd(&ov[kTrkRanks * kTrkRanks + t], area);
}

// inst_overlap's body: I[s][c] = |T_s AND C_c| and A_c = |C_c| of one frame against one track image. The workgroups of the grid
// share the 256-pixel groups of the image.
__device__ __forceinline__ void inst_overlap_body(const uint4* __restrict__ trk, const uint4* __restrict__ bits, int px,
                                                  uint32_t* __restrict__ ov) {
    const int t = threadIdx.x;
    uint32_t acc[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) acc[j] = 0;
    uint32_t area = 0;
    const int groups = (px + kTrkOvLanes - 1) / kTrkOvLanes;
    for (int g = blockIdx.x; g < groups; g += gridDim.x) {
        const int q = g * kTrkOvLanes + t;
        uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
        if (q < px) { a = trk[q]; b = bits[q]; }
        inst_overlap_group(a, b, acc, area);
    }
    inst_overlap_merge(acc, area, ov);
}

// A candidate pair; i == 0: none.
struct TrkCand { uint32_t i, u; int age, c, s; };

// a precedes b: the larger I / U by cross-multiplication (below 2^49), then the smaller age, the smaller rank, the smaller slot
__device__ __forceinline__ bool trk_precedes(const TrkCand& a, const TrkCand& b) {
    if (a.i == 0) return false;
    if (b.i == 0) return true;
    const unsigned long long l = (unsigned long long)a.i * b.u, r = (unsigned long long)b.i * a.u;
    if (l != r) return l > r;
    if (a.age != b.age) return a.age < b.age;
    if (a.c != b.c) return a.c < b.c;
    return a.s < b.s;
}

// the best of the eight lanes that share a row (or a column), in every one of them
__device__ __forceinline__ TrkCand trk_best_of_eight(TrkCand best) {
#pragma unroll
    for (int off = 4; off != 0; off >>= 1) {
        TrkCand o;
        o.i = __shfl_xor(best.i, off); o.u = __shfl_xor(best.u, off);
        o.age = __shfl_xor(best.age, off); o.c = __shfl_xor(best.c, off); o.s = __shfl_xor(best.s, off);
        if (trk_precedes(o, best)) best = o;
    }
    return best;
}

// inst_match's body: one workgroup of kTrkMatchLanes lanes, steps 2 - 6 of one frame (its matrix ov, its values meta) against one
// tracker's state st. The greedy match is computed as rounds: the order on the candidates is total, so a pair that is the best
// candidate of its slot AND of its rank among the pairs still free is one the sequential greedy takes (nothing that could remove it
// precedes it), and taking all such pairs at once leaves the greedy's remaining problem. Every round with a candidate left matches
// at least the best one, so there are at most 128 rounds. Lane t < 128 ends by storing slot t's row and rank and rank t's slot.
__device__ __forceinline__ void inst_match_body(const uint32_t* __restrict__ ov, uint32_t* __restrict__ meta, int32_t* __restrict__ st,
                                                int iou_permille, int max_age) {
    __shared__ int s_cls[kTrkRanks], s_id[kTrkRanks], s_age[kTrkRanks], s_area[kTrkRanks];   // slots
    __shared__ int s_ccls[kTrkRanks], s_carea[kTrkRanks];                                    // ranks: output class (0: not eligible), A_c
    __shared__ int s_slot_of[kTrkRanks], s_rank_of[kTrkRanks];
    __shared__ int s_rowbest[kTrkRanks], s_colbest[kTrkRanks], s_kill[kTrkRanks];
    __shared__ uint32_t s_live[4], s_used[4][4], s_keep[4];
    __shared__ int s_found, s_nfree, s_unmatched;
    const int t = threadIdx.x, grp = t >> 3, part = t & 7;
    if (t < kTrkRanks) {
        s_cls[t] = st[kTrkStSlots + 4 * t]; s_id[t] = st[kTrkStSlots + 4 * t + 1];
        s_age[t] = st[kTrkStSlots + 4 * t + 2]; s_area[t] = st[kTrkStSlots + 4 * t + 3];
        s_ccls[t] = (int)(meta[t] >> 24);
        s_carea[t] = (int)ov[kTrkRanks * kTrkRanks + t];
        s_slot_of[t] = -1; s_rank_of[t] = -1; s_kill[t] = 0;
    }
    if (t < 4) { s_live[t] = 0; s_keep[t] = 0; }
    if (t < 16) s_used[t >> 2][t & 3] = 0;
    if (t == 0) { s_nfree = 0; s_unmatched = 0; }
    __syncthreads();
    // steps 2 and 3
    for (int round = 0; round < kTrkRanks; ++round) {
        if (t == 0) s_found = 0;
        TrkCand best = { 0, 0, 0, 0, 0 };
        if (s_cls[grp] != 0 && s_rank_of[grp] < 0) {                         // row pass: grp is a slot
            const int s = grp;
            for (int k = 0; k < kTrkRanks / 8; ++k) {
                const int c = part + 8 * k;
                if (s_ccls[c] != s_cls[s] || s_slot_of[c] >= 0) continue;
                const uint32_t i = ov[s * kTrkRanks + c];
                if (i == 0) continue;
                const uint32_t u = (uint32_t)s_area[s] + (uint32_t)s_carea[c] - i;
                if (1000ull * i < (unsigned long long)iou_permille * u) continue;
                const TrkCand k2 = { i, u, s_age[s], c, s };
                if (trk_precedes(k2, best)) best = k2;
            }
        }
        best = trk_best_of_eight(best);
        if (part == 0) s_rowbest[grp] = best.i != 0 ? best.c : -1;
        best = TrkCand{ 0, 0, 0, 0, 0 };
        if (s_ccls[grp] != 0 && s_slot_of[grp] < 0) {                        // column pass: grp is a rank
            const int c = grp;
            for (int k = 0; k < kTrkRanks / 8; ++k) {
                const int s = part + 8 * k;
                if (s_cls[s] != s_ccls[c] || s_rank_of[s] >= 0) continue;
                const uint32_t i = ov[s * kTrkRanks + c];
                if (i == 0) continue;
                const uint32_t u = (uint32_t)s_area[s] + (uint32_t)s_carea[c] - i;
                if (1000ull * i < (unsigned long long)iou_permille * u) continue;
                const TrkCand k2 = { i, u, s_age[s], c, s };
                if (trk_precedes(k2, best)) best = k2;
            }
        }
        best = trk_best_of_eight(best);
        if (part == 0) s_colbest[grp] = best.i != 0 ? best.s : -1;
        __syncthreads();
        if (t < kTrkRanks) {
            const int s = s_colbest[t];
            if (s >= 0 && s_rowbest[s] == t) { s_slot_of[t] = s; s_rank_of[s] = t; s_found = 1; }
        }
        __syncthreads();
        const int found = s_found;
        __syncthreads();                                                         // (lane 0 clears s_found at the top)
        if (!found) break;
    }
    // step 4: ageing
    if (t < kTrkRanks && s_cls[t] != 0 && s_rank_of[t] < 0) {
        if (++s_age[t] > max_age) { s_cls[t] = 0; s_id[t] = 0; s_age[t] = 0; s_area[t] = 0; }
    }
    __syncthreads();
    // step 5: room. The lost slots in the order (largest age, largest slot); the first u - free of them die.
    if (t < kTrkRanks) {
        if (s_cls[t] == 0) atomicAdd(&s_nfree, 1);
        if (s_ccls[t] != 0 && s_slot_of[t] < 0) atomicAdd(&s_unmatched, 1);
    }
    __syncthreads();
    if (t < kTrkRanks && s_cls[t] != 0 && s_rank_of[t] < 0) {
        int pos = 0;
        for (int o = 0; o < kTrkRanks; ++o)
            if (s_cls[o] != 0 && s_rank_of[o] < 0 && (s_age[o] > s_age[t] || (s_age[o] == s_age[t] && o > t))) ++pos;
        s_kill[t] = pos < s_unmatched - s_nfree ? 1 : 0;
    }
    __syncthreads();
    if (t < kTrkRanks) {
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
        for (int c = 0; c < kTrkRanks; ++c) {
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
    if (t < kTrkRanks) {
        const int r = s_rank_of[t];
        if (r >= 0) { s_age[t] = 0; s_area[t] = s_carea[r]; }
        st[kTrkStSlots + 4 * t] = s_cls[t]; st[kTrkStSlots + 4 * t + 1] = s_id[t];
        st[kTrkStSlots + 4 * t + 2] = s_age[t]; st[kTrkStSlots + 4 * t + 3] = s_area[t];
        st[kTrkStRankOf + t] = r;
        const int s = s_slot_of[t];
        st[kTrkStSlotOf + t] = s;
        meta[t] = s >= 0 ? ((uint32_t)s_cls[s] << 24) | ((uint32_t)s_id[s] << 16) : 0u;
    }
    if (t < 4) st[kTrkStKeep + t] = (int32_t)s_keep[t];
}

// The rank -> slot map and the keep words of a tracker's state into LDS (s_map [128], s_keep [4]), by the whole workgroup.
__device__ __forceinline__ void inst_retrack_maps(const int32_t* __restrict__ st, int* s_map, uint32_t* s_keep) {
    const int t = threadIdx.x;
    if (t < kTrkRanks) s_map[t] = st[kTrkStSlotOf + t];
    if (t < 4) s_keep[t] = (uint32_t)st[kTrkStKeep + t];
    __syncthreads();
}

// Step 7 for one prototype pixel: the bits of the lost-but-alive slots of a stay, every bit of b moves to its rank's slot.
__device__ __forceinline__ uint4 inst_retrack_pixel(const uint4 a, const uint4 b, const int* s_map, const uint32_t* s_keep) {
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
    return make_uint4(o0, o1, o2, o3);
}

// inst_retrack's body: a lane per prototype pixel, T' = (T & keep) | permute(C).
__device__ __forceinline__ void inst_retrack_body(uint4* __restrict__ trk, const uint4* __restrict__ bits, int px,
                                                  const int32_t* __restrict__ st) {
    __shared__ int s_map[kTrkRanks];
    __shared__ uint32_t s_keep[4];
    inst_retrack_maps(st, s_map, s_keep);
    const int q = blockIdx.x * kTrkRetrackLanes + threadIdx.x;
    if (q >= px) return;
    trk[q] = inst_retrack_pixel(trk[q], bits[q], s_map, s_keep);
}

}  // namespace yh
