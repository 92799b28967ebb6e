// scene_turn_dev.h — the turn-aware planner's device code (DESIGN.md §11 "Turns"), shared by scene_turn.hip (yh_scene_plan_turn and
// yh_scene_batch_plan_turn: n frames per launch, the frame from blockIdx.z) and scene_turn_tour.hip (yh_scene_plan_turn_tour and
// yh_scene_batch_plan_turn_tour: one field per frame and target, the field from blockIdx.z): the compass, the round over a tile of all eight layers,
// the action rule, the chase along the action field and the walk. What they compute and why it is unique is said at the head of
// scene_turn.hip. A body reads the frame it works on through p (cost [8][H][W], edge, edge2, W, H, tx) and through the pointers it is
// given; it knows nothing of a batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scene_path_dev.h"

struct yh_scene;

namespace yh {

// scene_turn.hip: the turn planners' one round kernel as solve_rounds takes it - field z of F = n kmax fields, kmax per frame
SolveRound scene_turn_round(yh_scene* h, const PathParams& p, float tau, int kmax, int F);

constexpr int TL = (SP_TH + 2) * SP_P;   // one layer of the tile with its halo
constexpr int ACT_DRIVE = 0, ACT_CCW = 1, ACT_CW = 2, ACT_NONE = 3, ACT_TARGET = 255;

// heading h: its step (dx, dy) and the index of that step in around<8>'s order (left, right, up, down, up-left, up-right,
// down-left, down-right); four bits per heading
__host__ __device__ constexpr int head_dx(int h) { return (int)((0x21000122u >> (4 * h)) & 3u) - 1; }
__host__ __device__ constexpr int head_dy(int h) { return (int)((0x00012221u >> (4 * h)) & 3u) - 1; }
__host__ __device__ constexpr int head_edge(int h) { return (int)((0x52406371u >> (4 * h)) & 7u); }
static_assert(head_dx(0) == 1 && head_dy(0) == 0 && head_dx(3) == -1 && head_dy(3) == 1 && head_dx(6) == 0 && head_dy(6) == -1 && head_dx(7) == 1 && head_dy(7) == -1, "compass");
static_assert(head_edge(0) == 1 && head_edge(1) == 7 && head_edge(2) == 3 && head_edge(3) == 6 && head_edge(4) == 0 && head_edge(5) == 4 && head_edge(6) == 2 && head_edge(7) == 5, "compass");

// One round of the turn field at p.cost: tile (blockIdx.x, blockIdx.y), flagged in `mine`; neighbours are flagged in `theirs`. As
// relax_tile<8> with eight layers: the lane's block is a b / c d = q 0 1 / 2 3, V[h][q] its 32 values, L / D[q][h] the (length, |dh|)
// of pixel q's edge along heading h (length +inf where the frame ends or the pixel is off it: such a candidate is never smaller and
// the cell keeps its +inf).
__device__ __forceinline__ void turn_round_body(const PathParams& p, float tau, uint32_t* mine, uint32_t* theirs, uint32_t* cnt_next) {
    __shared__ float dl[8 * TL];
    __shared__ uint32_t active, border;
    const int tid = threadIdx.x;
    const int tile = blockIdx.y * p.tx + blockIdx.x;
    if (tid == 0) { active = mine[tile]; border = 0u; }
    __syncthreads();
    if (!active) return;   // (workgroup-uniform)
    if (tid == 0) mine[tile] = 0u;   // this array is next read two rounds on; nobody sets it during this round
    const int x0 = blockIdx.x * SP_TW, y0 = blockIdx.y * SP_TH;
    const size_t npx = (size_t)p.W * p.H;
    for (int i = tid; i < 8 * TL; i += SP_NT) {
        const int h = i / TL, r = i - h * TL;
        const int ly = r / SP_P, lx = r - ly * SP_P;
        const int gx = x0 + lx - 1, gy = y0 + ly - 1;
        dl[i] = gx >= 0 && gx < p.W && gy >= 0 && gy < p.H ? p.cost[h * npx + (size_t)gy * p.W + gx] : SP_INF;
    }
    const int cx = 2 * (tid % (SP_TW / 2)), cy = 2 * (tid / (SP_TW / 2));
    const int gx = x0 + cx, gy = y0 + cy;
    float L[4][8], D[4][8];
    bool in[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int px = gx + (q & 1), py = gy + (q >> 1);
        in[q] = px < p.W && py < p.H;
        if (in[q]) {
            const Around<8> e = around<8>(p, py * p.W + px);
#pragma unroll
            for (int h = 0; h < 8; ++h) { L[q][h] = e.at[head_edge(h)] >= 0 ? e.len[head_edge(h)] : SP_INF; D[q][h] = e.dh[head_edge(h)]; }
        } else {
#pragma unroll
            for (int h = 0; h < 8; ++h) { L[q][h] = SP_INF; D[q][h] = 0.0f; }
        }
    }
    const int ia = (cy + 1) * SP_P + cx + 1;
    __syncthreads();
    // other lanes store between two of this lane's reads: relaxed workgroup-scope atomics, so that every read is a read
#define ST_LD(i) __hip_atomic_load(&dl[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define ST_ST(i, v) __hip_atomic_store(&dl[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
    float V[8][4];
#pragma unroll
    for (int h = 0; h < 8; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) V[h][q] = ST_LD(h * TL + ia + (q >> 1) * SP_P + (q & 1));
    uint32_t changed = 0u;   // bit 4 h + q: V[h][q] is below what was loaded
    int any;
    do {
        uint32_t ch = 0u;
#pragma unroll
        for (int k = 0; k < SP_INNER; ++k) {
            uint32_t dirty = 0u;   // bit 4 h + q: V[h][q] got smaller in this sweep
            // drive: per layer first the pixels whose neighbour is another lane's (or the halo), then those whose neighbour is in
            // the block - which is always one of the former
#pragma unroll
            for (int h = 0; h < 8; ++h) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int nx = (q & 1) + head_dx(h), ny = (q >> 1) + head_dy(h);
                    if (nx < 0 || nx > 1 || ny < 0 || ny > 1) {
                        const float c = cand(ST_LD(h * TL + ia + ny * SP_P + nx), L[q][h], D[q][h]);
                        if (c < V[h][q]) { V[h][q] = c; dirty |= 1u << (4 * h + q); }
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int nx = (q & 1) + head_dx(h), ny = (q >> 1) + head_dy(h);
                    if (nx >= 0 && nx <= 1 && ny >= 0 && ny <= 1) {
                        const float c = cand(V[h][2 * ny + nx], L[q][h], D[q][h]);
                        if (c < V[h][q]) { V[h][q] = c; dirty |= 1u << (4 * h + q); }
                    }
                }
            }
            // turn: once round the ring clockwise, once counter-clockwise; every turn candidate is looked at in every sweep
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int h = 0; h < 8; ++h) {
                    const float c = __fadd_rn(V[(h + 7) & 7][q], tau);
                    if (c < V[h][q]) { V[h][q] = c; dirty |= 1u << (4 * h + q); }
                }
#pragma unroll
                for (int h = 7; h >= 0; --h) {
                    const float c = __fadd_rn(V[(h + 1) & 7][q], tau);
                    if (c < V[h][q]) { V[h][q] = c; dirty |= 1u << (4 * h + q); }
                }
            }
#pragma unroll
            for (int h = 0; h < 8; ++h)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (dirty & (1u << (4 * h + q))) ST_ST(h * TL + ia + (q >> 1) * SP_P + (q & 1), V[h][q]);
            ch |= dirty;
        }
        changed |= ch;
        any = __syncthreads_or(ch != 0u);
    } while (any);
    // (no store by any lane between two votes: the tile in LDS stood still while every lane looked at every candidate of its states)
#undef ST_LD
#undef ST_ST
    uint32_t* cu = reinterpret_cast<uint32_t*>(p.cost);
#pragma unroll
    for (int h = 0; h < 8; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if ((changed & (1u << (4 * h + q))) && in[q]) atomicMin(cu + h * npx + (size_t)(gy + (q >> 1)) * p.W + gx + (q & 1), __float_as_uint(V[h][q]));
    const bool ca = changed & 0x11111111u, cb = changed & 0x22222222u, cc = changed & 0x44444444u, cd = changed & 0x88888888u;
    uint32_t m = 0u;
    if (cx == 0 && (ca || cc)) m |= 1u;
    if (cx == SP_TW - 2 && (cb || cd)) m |= 2u;
    if (cy == 0 && (ca || cb)) m |= 4u;
    if (cy == SP_TH - 2 && (cc || cd)) m |= 8u;
    if (cx == 0 && cy == 0 && ca) m |= 16u;   // the four corner cells: up-left, up-right, down-left, down-right
    if (cx == SP_TW - 2 && cy == 0 && cb) m |= 32u;
    if (cx == 0 && cy == SP_TH - 2 && cc) m |= 64u;
    if (cx == SP_TW - 2 && cy == SP_TH - 2 && cd) m |= 128u;
    if (m) atomicOr(&border, m);
    __syncthreads();
    if (tid < 8 && ((border >> tid) & 1u)) {
        const int sx = tid == 0 ? -1 : tid == 1 ? 1 : tid < 4 ? 0 : (tid & 1) ? 1 : -1, sy = tid < 2 ? 0 : tid == 2 ? -1 : tid == 3 ? 1 : tid < 6 ? -1 : 1;
        const int bx = (int)blockIdx.x + sx, by = (int)blockIdx.y + sy;
        if (bx >= 0 && bx < p.tx && by >= 0 && by < (int)gridDim.y && atomicExch(theirs + by * p.tx + bx, 1u) == 0u) atomicAdd(cnt_next, 1u);
    }
}

// act[h][i] of pixel i for the eight headings of the field `cost`, e the pixel's edge terms: the first of (drive, turn to h - 1, turn
// to h + 1) whose candidate equals d[h][i] bitwise. d: the pixel's eight costs, for a caller that goes on with them.
__device__ __forceinline__ void turn_act_pixel(const Around<8>& e, const float* cost, size_t npx, int i, float tau, uint8_t* act, float (&d)[8]) {
#pragma unroll
    for (int h = 0; h < 8; ++h) d[h] = cost[h * npx + i];
#pragma unroll
    for (int h = 0; h < 8; ++h) {
        const uint32_t dv = __float_as_uint(d[h]);
        const int k = head_edge(h);
        int a = ACT_NONE;   // (in reverse, so that the first of the order wins)
        if (__float_as_uint(__fadd_rn(d[(h + 1) & 7], tau)) == dv) a = ACT_CW;
        if (__float_as_uint(__fadd_rn(d[(h + 7) & 7], tau)) == dv) a = ACT_CCW;
        if (e.at[k] >= 0 && __float_as_uint(cand(cost[h * npx + e.at[k]], e.len[k], e.dh[k])) == dv) a = ACT_DRIVE;
        act[h * npx + i] = (uint8_t)a;
    }
}

// act[h][i] of pixel i = blockIdx.x * 256 + threadIdx.x, its edge terms read once for the eight headings
__device__ __forceinline__ void turn_act_body(const PathParams& p, float tau, uint8_t* act) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.W * p.H) return;
    float d[8];
    turn_act_pixel(around<8>(p, i), p.cost, (size_t)p.W * p.H, i, tau, act, d);
}

__device__ __forceinline__ float turn_rot(int k) {   // float32((4 - k) * pi / 4)
    constexpr double pi = 3.14159265358979323846;
    return k == 0 ? (float)pi : k == 1 ? (float)(3.0 * pi / 4.0) : k == 2 ? (float)(pi / 2.0) : k == 3 ? (float)(pi / 4.0) : 0.0f;
}

// One wave follows act from (start, heading) through a 32 x 32 x 8 window of it in LDS. STORE: it writes a node per drive and the
// turns made before it (else nodes and turns are not touched: the chase of an entry of the turn tour's leg table). Returns the nodes
// on the route (start and target included); heading is the one it arrived with; lost: no target within 8 W H actions, an action that
// is none, or a drive off the frame (costs strictly decrease along act, so none of this happens at a solution; the bounds are what
// keeps the loop finite and the stores inside their arrays on any input). What it stored is visible to the whole wave on return.
template <bool STORE>
__device__ __forceinline__ int turn_chase(const uint8_t* act, int W, int H, int start, int& heading, int2* nodes, int32_t* turns, bool& lost) {
    __shared__ uint8_t win[8 * SP_WS * SP_WS];
    const int lane = threadIdx.x;
    const size_t npx = (size_t)W * H;
    const long long cap = 8ll * W * H;
    int cx = start % W, cy = start / W, hd = heading & 7, t = 0, n = 1;
    long long actions = 0;
    bool done = false;
    lost = false;
    if (STORE && lane == 0) nodes[0] = make_int2(cx, cy);
    while (!done && !lost) {   // (wave-uniform)
        const int wx0 = max(0, min(cx - SP_WS / 2, W - SP_WS)), wy0 = max(0, min(cy - SP_WS / 2, H - SP_WS));
        for (int i = lane; i < 8 * SP_WS * SP_WS; i += 64) {
            const int h = i / (SP_WS * SP_WS), r = i % (SP_WS * SP_WS);
            const int gx = wx0 + r % SP_WS, gy = wy0 + r / SP_WS;
            win[i] = gx < W && gy < H ? act[h * npx + (size_t)gy * W + gx] : (uint8_t)ACT_NONE;
        }
        __syncthreads();
        while (true) {
            if (actions >= cap) { lost = true; break; }
            ++actions;
            const int a = win[hd * SP_WS * SP_WS + (cy - wy0) * SP_WS + (cx - wx0)];
            if (a == ACT_TARGET) { done = true; break; }
            if (a == ACT_CCW) { hd = (hd + 7) & 7; --t; continue; }
            if (a == ACT_CW) { hd = (hd + 1) & 7; ++t; continue; }
            const int nx = cx + head_dx(hd), ny = cy + head_dy(hd);
            if (a != ACT_DRIVE || nx < 0 || nx >= W || ny < 0 || ny >= H || (size_t)n >= npx) { lost = true; break; }
            if (STORE && lane == 0) { turns[n - 1] = t; nodes[n] = make_int2(nx, ny); }
            ++n; t = 0; cx = nx; cy = ny;
            if (cx < wx0 || cx >= wx0 + SP_WS || cy < wy0 || cy >= wy0 + SP_WS) break;
        }
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    heading = hd;
    return n;
}

// One wave: the route along act from (start, heading), then its lanes write the directions.
// out[0] = nodes on the route (start and target included), out[1] = 0, or 1 if the walk was lost (turn_chase)
__device__ __forceinline__ void turn_walk_body(const PathParams& p, const uint8_t* act, int start, int heading, int2* nodes, int32_t* turns, float2* dirs, int32_t* out) {
    const int lane = threadIdx.x, W = p.W;
    const size_t npx = (size_t)W * p.H;
    bool lost;
    const int n = turn_chase<true>(act, W, p.H, start, heading, nodes, turns, lost);
    // directions[i] = (d[h_i][n_i] - d[h_i][n_i+1], rot of |turns[i]|): the drive edge alone, h_i the heading driven
    if (!lost)
        for (int i = lane; i + 1 < n; i += 64) {
            const int2 a = nodes[i], b = nodes[i + 1];
            int h = 0;
#pragma unroll
            for (int k = 1; k < 8; ++k) if (b.x - a.x == head_dx(k) && b.y - a.y == head_dy(k)) h = k;
            const float mag = __fsub_rn(p.cost[h * npx + (size_t)a.y * W + a.x], p.cost[h * npx + (size_t)b.y * W + b.x]);
            dirs[i] = make_float2(mag, turn_rot(abs(turns[i])));
        }
    if (lane == 0) { out[0] = n; out[1] = lost ? 1 : 0; }
}

}  // namespace yh
