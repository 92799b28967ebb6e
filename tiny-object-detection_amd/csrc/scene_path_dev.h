// scene_path_dev.h — the planner's device code shared by scene_path.hip (one multi-source field, yh_scene_plan) and
// scene_tour.hip (K single-target fields relaxed in the same launches, yh_scene_plan_tour): the tile relaxation, the successor
// rule and the windowed chase. What they compute and why it is unique is said at the head of scene_path.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef SP_TW
#define SP_TW 32   // tile width and height (even). Measured alternatives: DESIGN.md §11
#endif
#ifndef SP_TH
#define SP_TH 32
#endif
#ifndef SP_INNER
#define SP_INNER 4   // sweeps between two workgroup votes
#endif
#ifndef SP_BATCH
#define SP_BATCH 16   // rounds enqueued per host read of the counters
#endif
#define SP_NT ((SP_TW / 2) * (SP_TH / 2))
#define SP_P (SP_TW + 2)
#define SP_WS 32   // the chase's window
#define SP_INF __uint_as_float(0x7f800000u)

static_assert(SP_TW % 2 == 0 && SP_TH % 2 == 0 && SP_NT % 64 == 0 && SP_NT <= 1024, "tile: whole waves of 2 x 2 blocks");

namespace yh {

struct PathParams {
    int W, H, tx, ntiles;
    const uint32_t* map;
    const float4 *conn0, *conn1;
    float4* edge;
    float* cost;
    int32_t* next;
    uint32_t* flags;
};

// path_weights (scene_path.hip) on stream s: p.map, p.conn0, p.conn1 -> p.edge. The edge terms do not depend on the targets: a tour
// computes them once for all its fields.
void path_weights_launch(const PathParams& p, hipStream_t s);

__device__ __forceinline__ float cand(float dn, float len, float dh) { return __fadd_rn(__fadd_rn(dn, len), dh); }

// One workgroup of SP_NT lanes, tile (blockIdx.x, blockIdx.y) of the field `cost`: if `mine` flags the tile, relax it to its local
// fixed point for the halo it loads, write back what got smaller, flag in `theirs` the tiles across every border that moved and
// count each newly flagged one in *cnt_next.
__device__ __forceinline__ void relax_tile(const PathParams& p, float* cost, uint32_t* mine, uint32_t* theirs, uint32_t* cnt_next) {
    __shared__ float dl[(SP_TH + 2) * SP_P];
    __shared__ uint32_t active, border;
    const int tid = threadIdx.x;
    const int tile = blockIdx.y * p.tx + blockIdx.x;
    if (tid == 0) { active = mine[tile]; border = 0u; }
    __syncthreads();
    if (!active) return;   // (workgroup-uniform)
    if (tid == 0) mine[tile] = 0u;   // this array is next read two rounds on; nobody sets it during this round
    const int x0 = blockIdx.x * SP_TW, y0 = blockIdx.y * SP_TH;
    for (int i = tid; i < (SP_TH + 2) * SP_P; i += SP_NT) {
        const int ly = i / SP_P, lx = i - ly * SP_P;
        const int gx = x0 + lx - 1, gy = y0 + ly - 1;
        dl[i] = gx >= 0 && gx < p.W && gy >= 0 && gy < p.H ? cost[(size_t)gy * p.W + gx] : SP_INF;
    }
    // this lane's 2 x 2 block: a b / c d. Edge terms: (length, |dh|); an edge with an end off the frame (by the frame's geometry,
    // whatever the fields say) has length +inf: such a candidate is never smaller, a cell off the frame (ragged tiles) keeps its
    // +inf and is never stored
    const int cx = 2 * (tid % (SP_TW / 2)), cy = 2 * (tid / (SP_TW / 2));
    const int gx = x0 + cx, gy = y0 + cy;
    const bool in_a = gx < p.W && gy < p.H, in_b = gx + 1 < p.W && gy < p.H, in_c = gx < p.W && gy + 1 < p.H, in_d = gx + 1 < p.W && gy + 1 < p.H;
    const bool has_l = gx > 0, has_r = gx + 2 < p.W, has_u = gy > 0, has_d = gy + 2 < p.H;
    const float4 none = make_float4(-1.0f, 0.0f, -1.0f, 0.0f);
    const size_t ga = (size_t)gy * p.W + gx;
    const float4 ea = in_a ? p.edge[ga] : none, eb = in_b ? p.edge[ga + 1] : none;
    const float4 ec = in_c ? p.edge[ga + p.W] : none, ed = in_d ? p.edge[ga + p.W + 1] : none;
    const float4 ela = has_l && in_a ? p.edge[ga - 1] : none, elc = has_l && in_c ? p.edge[ga + p.W - 1] : none;
    const float4 eua = has_u && in_a ? p.edge[ga - p.W] : none, eub = has_u && in_b ? p.edge[ga - p.W + 1] : none;
#define SP_LEN(ok, v) ((ok) && (v) >= 0.0f ? (v) : SP_INF)
    const float l_ab = SP_LEN(in_a && in_b, ea.x), h_ab = ea.y, l_cd = SP_LEN(in_c && in_d, ec.x), h_cd = ec.y;   // inside the block
    const float l_ac = SP_LEN(in_a && in_c, ea.z), h_ac = ea.w, l_bd = SP_LEN(in_b && in_d, eb.z), h_bd = eb.w;
    const float l_la = SP_LEN(has_l && in_a, ela.x), h_la = ela.y, l_lc = SP_LEN(has_l && in_c, elc.x), h_lc = elc.y;   // to the left of a, c
    const float l_rb = SP_LEN(has_r && in_b, eb.x), h_rb = eb.y, l_rd = SP_LEN(has_r && in_d, ed.x), h_rd = ed.y;       // to the right of b, d
    const float l_ua = SP_LEN(has_u && in_a, eua.z), h_ua = eua.w, l_ub = SP_LEN(has_u && in_b, eub.z), h_ub = eub.w;   // above a, b
    const float l_dc = SP_LEN(has_d && in_c, ec.z), h_dc = ec.w, l_dd = SP_LEN(has_d && in_d, ed.z), h_dd = ed.w;       // below c, d
#undef SP_LEN
    const int ia = (cy + 1) * SP_P + cx + 1, ib = ia + 1, ic = ia + SP_P, id = ic + 1;
    __syncthreads();
    // other lanes store between two of this lane's reads: relaxed workgroup-scope atomics, so that every read is a read (and stays a
    // ds_read: a volatile access would go through the flat path)
#define SP_LD(i) __hip_atomic_load(&dl[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define SP_ST(i, v) __hip_atomic_store(&dl[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
    float va = SP_LD(ia), vb = SP_LD(ib), vc = SP_LD(ic), vd = SP_LD(id);
    const float oa = va, ob = vb, oc = vc, od = vd;
    int any;
    do {
        int ch = 0;
#pragma unroll
        for (int k = 0; k < SP_INNER; ++k) {
            const float na_l = SP_LD(ia - 1), nc_l = SP_LD(ic - 1), nb_r = SP_LD(ib + 1), nd_r = SP_LD(id + 1);
            const float na_u = SP_LD(ia - SP_P), nb_u = SP_LD(ib - SP_P), nc_d = SP_LD(ic + SP_P), nd_d = SP_LD(id + SP_P);
            float a = fminf(va, fminf(cand(na_l, l_la, h_la), cand(na_u, l_ua, h_ua)));
            float b = fminf(vb, fminf(cand(nb_r, l_rb, h_rb), cand(nb_u, l_ub, h_ub)));
            float c = fminf(vc, fminf(cand(nc_l, l_lc, h_lc), cand(nc_d, l_dc, h_dc)));
            float d = fminf(vd, fminf(cand(nd_r, l_rd, h_rd), cand(nd_d, l_dd, h_dd)));
            a = fminf(a, fminf(cand(b, l_ab, h_ab), cand(c, l_ac, h_ac)));       // forwards a, b, c, d
            b = fminf(b, fminf(cand(a, l_ab, h_ab), cand(d, l_bd, h_bd)));
            c = fminf(c, fminf(cand(a, l_ac, h_ac), cand(d, l_cd, h_cd)));
            d = fminf(d, fminf(cand(b, l_bd, h_bd), cand(c, l_cd, h_cd)));
            c = fminf(c, cand(d, l_cd, h_cd));                                   // and back
            b = fminf(b, cand(d, l_bd, h_bd));
            a = fminf(a, fminf(cand(b, l_ab, h_ab), cand(c, l_ac, h_ac)));
            if (a < va) { SP_ST(ia, a); va = a; ch = 1; }
            if (b < vb) { SP_ST(ib, b); vb = b; ch = 1; }
            if (c < vc) { SP_ST(ic, c); vc = c; ch = 1; }
            if (d < vd) { SP_ST(id, d); vd = d; ch = 1; }
        }
        any = __syncthreads_or(ch);
    } while (any);
#undef SP_LD
#undef SP_ST
    // back to the field, and which borders moved
    uint32_t* cu = reinterpret_cast<uint32_t*>(cost);
    const bool ca = va < oa, cb = vb < ob, cc = vc < oc, cd = vd < od;
    if (ca && in_a) atomicMin(cu + ga, __float_as_uint(va));
    if (cb && in_b) atomicMin(cu + ga + 1, __float_as_uint(vb));
    if (cc && in_c) atomicMin(cu + ga + p.W, __float_as_uint(vc));
    if (cd && in_d) atomicMin(cu + ga + p.W + 1, __float_as_uint(vd));
    uint32_t m = 0u;
    if (cx == 0 && (ca || cc)) m |= 1u;
    if (cx == SP_TW - 2 && (cb || cd)) m |= 2u;
    if (cy == 0 && (ca || cb)) m |= 4u;
    if (cy == SP_TH - 2 && (cc || cd)) m |= 8u;
    if (m) atomicOr(&border, m);
    __syncthreads();
    if (tid < 4 && ((border >> tid) & 1u)) {
        const int bx = (int)blockIdx.x + (tid == 0 ? -1 : tid == 1 ? 1 : 0), by = (int)blockIdx.y + (tid == 2 ? -1 : tid == 3 ? 1 : 0);
        if (bx >= 0 && bx < p.tx && by >= 0 && by < (int)gridDim.y && atomicExch(theirs + by * p.tx + bx, 1u) == 0u) atomicAdd(cnt_next, 1u);
    }
}

// next[i] of the field `cost`: the first neighbour in the order (left, right, up, down) whose candidate equals d[i] bitwise, -1 if none
__device__ __forceinline__ int successor(const PathParams& p, const float* cost, int i) {
    const int x = i % p.W, y = i / p.W;
    const uint32_t dv = __float_as_uint(cost[i]);
    const float4 e = p.edge[i];
    int nx = -1;
    // (in reverse, so that the first of the order left, right, up, down wins)
    if (y + 1 < p.H && __float_as_uint(cand(cost[i + p.W], e.z, e.w)) == dv) nx = i + p.W;
    if (y > 0) { const float4 u = p.edge[i - p.W]; if (__float_as_uint(cand(cost[i - p.W], u.z, u.w)) == dv) nx = i - p.W; }
    if (x + 1 < p.W && __float_as_uint(cand(cost[i + 1], e.x, e.y)) == dv) nx = i + 1;
    if (x > 0) { const float4 l = p.edge[i - 1]; if (__float_as_uint(cand(cost[i - 1], l.x, l.y)) == dv) nx = i - 1; }
    return nx;
}

// One wave chases `next` from `start` through a SP_WS x SP_WS window of it held in LDS (reloaded when the route leaves it) and
// writes the nodes it visits, start and target included. Returns their number; lost = no -1 met within W * H nodes (costs
// strictly decrease along `next`, so this cannot happen on SANE fields; the bound is what keeps the loop finite on any input).
// The nodes are visible to the whole wave on return.
__device__ __forceinline__ int chase(const int32_t* next, int W, int H, int start, int2* nodes, bool& lost) {
    __shared__ int win[SP_WS * SP_WS];
    const int lane = threadIdx.x, npx = W * H;
    int cx = start % W, cy = start / W, n = 0;
    bool done = false;
    lost = false;
    while (!done && !lost) {   // (wave-uniform)
        const int wx0 = max(0, min(cx - SP_WS / 2, W - SP_WS)), wy0 = max(0, min(cy - SP_WS / 2, H - SP_WS));
        for (int i = lane; i < SP_WS * SP_WS; i += 64) {
            const int gx = wx0 + i % SP_WS, gy = wy0 + i / SP_WS;
            win[i] = gx < W && gy < H ? next[(size_t)gy * W + gx] : -1;
        }
        __syncthreads();
        while (true) {
            if (n >= npx) { lost = true; break; }
            if (lane == 0) nodes[n] = make_int2(cx, cy);
            ++n;
            const int nx = win[(cy - wy0) * SP_WS + (cx - wx0)];
            if (nx < 0) { done = true; break; }
            cx = nx % W; cy = nx / W;
            if (cx < wx0 || cx >= wx0 + SP_WS || cy < wy0 || cy >= wy0 + SP_WS) break;
        }
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    return n;
}

}  // namespace yh
