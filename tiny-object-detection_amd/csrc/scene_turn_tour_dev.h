// scene_turn_tour_dev.h — the turn-aware tour's device code and its order search (DESIGN.md §11 "Turn tour"), for
// scene_turn_tour.hip (yh_scene_plan_turn_tour and yh_scene_batch_plan_turn_tour: n frames per launch, the frame from blockIdx.z;
// a scene is the batch of one): the action-and-label rule, an entry of the leg
// table, a leg's walk, the join of the legs, and the choice of the order on the host. What they compute is said at the head of
// scene_turn_tour.hip. A body reads the frame it works on through p (cost [K][8][H][W], edge, edge2, W, H) and through the pointers
// it is given, all of them that frame's own; it knows nothing of a batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "scene_path_dev.h"
#include "scene_turn_dev.h"
#include "yh_internal.h"

#define TT_JOIN_BLOCKS 120   // the join kernel's grid x (its lanes stride over the route)

namespace yh {

constexpr int kRowsMax = 1 + 8 * YH_TOUR_MAX, kEntriesMax = kRowsMax * YH_TOUR_MAX;   // the leg table at K = YH_TOUR_MAX

struct TurnTourPoints { int32_t K, start, heading, t[YH_TOUR_MAX]; };                             // the start state and the targets, linear indices
struct TurnTourLegs { int32_t K, field[YH_TOUR_MAX], from[YH_TOUR_MAX], heading[YH_TOUR_MAX]; };   // leg j walks act_{field[j]} from (from[j], heading[j])

// field b of the turn tour: its eight layers; map and the edge terms are the frame's, whatever the field
__device__ __forceinline__ PathParams turn_field_of(const PathParams& p, int b) {
    PathParams q = p;
    q.cost += (size_t)b * 8 * p.W * p.H;
    return q;
}

// act_b of pixel i = blockIdx.x * 256 + threadIdx.x for every field (turn_act_pixel: the bits of turn_act_body), 255 at t_b, and
// the label of its eight states
__device__ __forceinline__ void turn_tour_act_body(const PathParams& p, const TurnTourPoints& pts, float tau, uint8_t* act, uint8_t* label) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.W * p.H) return;
    const size_t npx = (size_t)p.W * p.H;
    const Around<8> e = around<8>(p, i);
    float best[8];
    int lab[8];
#pragma unroll
    for (int h = 0; h < 8; ++h) { best[h] = SP_INF; lab[h] = 0; }
    for (int b = 0; b < pts.K; ++b) {
        float d[8];
        uint8_t* ab = act + (size_t)b * 8 * npx;
        turn_act_pixel(e, p.cost + (size_t)b * 8 * npx, npx, i, tau, ab, d);
        if (i == pts.t[b]) {
#pragma unroll
            for (int h = 0; h < 8; ++h) ab[h * npx + i] = (uint8_t)ACT_TARGET;
        }
#pragma unroll
        for (int h = 0; h < 8; ++h) if (d[h] < best[h]) { best[h] = d[h]; lab[h] = b; }   // (strictly: the smallest b among equals)
    }
#pragma unroll
    for (int h = 0; h < 8; ++h) label[h * npx + i] = (uint8_t)lab[h];
}

// entry blockIdx.x = r * K + b of the leg table [3][kEntriesMax]: d_b at row r's state, the heading with which act_b takes it to
// t_b, whether that chase was lost. One wave.
__device__ __forceinline__ void turn_tour_arrive_body(const PathParams& p, const TurnTourPoints& pts, const uint8_t* act, int32_t* table) {
    const int e = blockIdx.x, r = e / pts.K, b = e - r * pts.K;
    const size_t npx = (size_t)p.W * p.H;
    const int at = r == 0 ? pts.start : pts.t[(r - 1) >> 3];
    int hd = r == 0 ? pts.heading : (r - 1) & 7;
    const float d = p.cost[((size_t)b * 8 + hd) * npx + at];
    bool lost = false;
    if (at != pts.t[b]) {   // (workgroup-uniform; on its own target the row's heading is the arrival heading)
        (void)turn_chase<false>(act + (size_t)b * 8 * npx, p.W, p.H, at, hd, nullptr, nullptr, lost);
    }
    if (threadIdx.x == 0) { table[e] = (int32_t)__float_as_uint(d); table[kEntriesMax + e] = hd; table[2 * kEntriesMax + e] = lost ? 1 : 0; }
}

// leg j = blockIdx.x, one wave: out[2 j] = its nodes (its start and its target included), out[2 j + 1] = 1 if it was lost (turn_walk_body)
__device__ __forceinline__ void turn_tour_walk_body(const PathParams& p, const TurnTourLegs& legs, const uint8_t* act, int2* seg_nodes, int32_t* seg_turns,
                                                    float2* seg_dirs, int32_t* out) {
    const int j = blockIdx.x, f = legs.field[j];
    const size_t npx = (size_t)p.W * p.H;
    turn_walk_body(turn_field_of(p, f), act + (size_t)f * 8 * npx, legs.from[j], legs.heading[j], seg_nodes + j * npx, seg_turns + j * npx, seg_dirs + j * npx, out + 2 * j);
}

// Leg j holds the route's nodes off[j] .. off[j + 1] (both ends: a junction is the last node of one leg and the first of the next;
// a leg of one node adds nothing), off[0] = 0, off[j + 1] = off[j] + len[j] - 1; the route has off[K] + 1 nodes. Step g (node g ->
// node g + 1) lies in the leg with off[j] <= g < off[j + 1] and is that leg's step g - off[j]: its turns were counted from the
// heading the leg started with - at a junction the one the leg before arrived with - in that leg's action field, its magnitude is
// the difference of that leg's cost field. out: walk_out; leg_ends at out[2 YH_TOUR_MAX ..], the route's nodes at out[3 YH_TOUR_MAX].
// The lanes of gridDim.x blocks of 256 stride over the route.
__device__ __forceinline__ void turn_tour_join_body(const PathParams& p, int K, const int2* seg_nodes, const int32_t* seg_turns, const float2* seg_dirs, int32_t* out,
                                                    int2* nodes, int32_t* turns, float2* dirs) {
    const size_t npx = (size_t)p.W * p.H;
    int off[YH_TOUR_MAX + 1];
    off[0] = 0;
#pragma unroll
    for (int j = 0; j < YH_TOUR_MAX; ++j) off[j + 1] = off[j] + (j < K ? max(out[2 * j], 1) - 1 : 0);
    const int L = off[YH_TOUR_MAX] + 1;
    // (unrolled with constant indices: off[] stays in registers)
    for (int g = blockIdx.x * 256 + threadIdx.x; g < L; g += gridDim.x * 256) {
        int j = 0, base = 0;   // the leg that holds node g: the last one whose first node lies before g
#pragma unroll
        for (int k = 1; k < YH_TOUR_MAX; ++k) if (k < K && g > off[k]) { j = k; base = off[k]; }
        nodes[g] = seg_nodes[j * npx + (g - base)];
        if (g + 1 >= L) continue;
        j = 0; base = 0;       // the leg that holds step g: the last one that starts at or before node g
#pragma unroll
        for (int k = 1; k < YH_TOUR_MAX; ++k) if (k < K && g >= off[k]) { j = k; base = off[k]; }
        turns[g] = seg_turns[j * npx + (g - base)];
        dirs[g] = seg_dirs[j * npx + (g - base)];
    }
    if (blockIdx.x == 0 && threadIdx.x <= YH_TOUR_MAX) {
        const int j = threadIdx.x;
        int v = L;
#pragma unroll
        for (int k = 0; k < YH_TOUR_MAX; ++k) if (j == k) v = off[k + 1];
        out[2 * YH_TOUR_MAX + j] = v;
    }
}

// legs, arrive [1 + 8 K][K] -> the order of least total (f32, summed left to right from the carried state), the lexicographically
// first among equals; row[j]: the table row of the state leg j starts in
inline float best_order(const float* legs, const uint8_t* arrive, int K, int32_t* order, int32_t* row) {
    int perm[YH_TOUR_MAX], rows[YH_TOUR_MAX];
    for (int k = 0; k < K; ++k) perm[k] = k;
    float best = 0.0f;
    bool have = false;
    do {
        float total = 0.0f;
        int r = 0;
        for (int j = 0; j < K; ++j) {
            rows[j] = r;
            total = total + legs[r * K + perm[j]];
            r = 1 + 8 * perm[j] + arrive[r * K + perm[j]];
        }
        if (!have || total < best) { best = total; have = true; std::copy(perm, perm + K, order); std::copy(rows, rows + K, row); }
    } while (std::next_permutation(perm, perm + K));
    return best;
}

}  // namespace yh
