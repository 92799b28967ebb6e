// scene_tour.hip — the tour (yh_scene_plan_tour): which ball first, then which, and the whole route. The reference stops at "the
// cheapest way to the nearest of the balls" and says so (path.rs:38 "Dijkstra's algorithm with 3 targets (yet to choose heuristic)",
// :35,:66 a ball[node] label "Use in optimizations and UI"). What is computed is the definition frozen in DESIGN.md §11 "Tour" and
// restated in tests/tour_ref.py: K <= YH_TOUR_MAX distinct targets; per target t_b the single-target cost field d_b and successor
// field next_b of scene_path.hip's planner (same graph, same edge terms, same association: the device functions of
// scene_path_dev.h); label[v] = the smallest b with d_b[v] == min_b d_b[v]; the leg matrix legs[0][b] = d_b[start],
// legs[1 + a][b] = d_b[t_a] (FROM t_a TO t_b: costs accumulate from the target outward, d_b[t_a] and d_a[t_b] differ in their last
// bits); the order minimising the f32 left-to-right sum of its legs, ties to the lexicographically smallest; the legs' walks joined.
// A plan is bound by serial depth (a round is as long as its slowest tile, ~42 of 300 workgroups have work), so the fields relax in
// the SAME launches, the field as grid z: a call's rounds are those of its slowest field, not their sum.
// There is one driver (run_tour) and one set of kernels for yh_scene_plan_tour_conn (the batch of one) and yh_scene_batch_plan_tour
// (the first n of the handle's max_frames; DESIGN.md §11 "Scene batch: tours"): each kernel takes its frame from blockIdx.z. A field is
// unique (every weight >= 1) and has its own cost field and tile flags, so fields that share rounds cannot change each other's bits.
//
// K is ragged: Kmax is one number per call (a batch's n_targets; a scene's number of distinct targets), frame b has K_b <= Kmax
// targets (fewer balls, or balls on one pixel). Field f of frame b is solver field z = b Kmax + f - NOT b K_b + f. What advances by what:
//   edge, edge2 (and map, conn0, conn1 under path_weights)    b W H          one set of edge terms per frame, shared by its fields
//   cost f32, next i32 [n][Kmax][H][W]                        z W H
//   label u8 [n][H][W]                                        b W H
//   segs int2 [n][Kmax][W H]                                  z W H          leg j of frame b: z = b Kmax + j
//   nodes int2, dirs float2 [n][Kmax W H]                     b Kmax W H     a joined route is at most K W H long
//   leg matrices f32 [n][kLegsMax] (the solver's tail), walk_out i32 [n][2 YH_TOUR_MAX], points, legs [n]
//   flags [2][n Kmax][ntiles]                                 as field_round indexes them, F = n Kmax
// Bytes per pixel: 32 per (frame, target) - cost 4, next 4, the legs' walks 8, the joined route 16 - plus 1 per frame for the label;
// allocated at the first call for max_frames x the largest Kmax so far, growing only (growing drops the last tour). 640 x 480 with
// max_frames = 64 and Kmax = 6 is 3.8 GB: a caller sizes max_frames and n_targets accordingly.
// A field f >= K_b has no seed: it flags nothing and its tiles exit at once (the solver's ragged field_of form); the legs, next, walk
// and join kernels skip it.
//
// Launches of one call, their number independent of n (the solver and its buffers are scene_solve.hip's, shared with the other kinds):
//   the inputs     ONE copy from the state's pinned block: the seeds as (pixel, field z) pairs, then the points [n].
//   path_weights   (scene_solve.hip) over the n frames: the edge terms are shared by all fields of a frame.
//   one fill of n Kmax W H values with +inf, tour_seeds (0 at t_b in its field).
//   field_round    x rounds, grid (tiles x, tiles y, n Kmax) (scene_solve.hip, through solve_field_round): relax_tile on field z with
//                  the edge terms of frame z / Kmax.
//   tour_legs      after every batch of rounds (the solver's after-batch hook), one wave per frame: the K_b (K_b + 1) entries of frame
//                  b's leg matrix into its kLegsMax words of the tail of the block the host reads the batch's counters from: the n
//                  matrices arrive with the last counters (earlier copies are ignored) - no copy and no wait of their own.
//   tour_next      one lane per pixel (pixels x 1 x n): next_b for the frame's K_b fields and the label (the pixel's edge terms read
//                  once for all of them).
//   (host)         the order of every frame: all K! <= 720 permutations from its leg matrix (best_order). ONE upload of the legs [n].
//   tour_walk      Kmax x 1 x n waves, one per leg: leg j chases next_{o_j} from the start (j = 0) or from t_{o_{j-1}} into its own segment.
//   tour_join      (blocks x 1 x n) the segments into one node list (a junction node once) and the directions over it.
//   ONE copy of n x 2 YH_TOUR_MAX words and ONE wait.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "scene.h"
#include "scene_batch.h"
#include "scene_path_dev.h"
#include "yh_internal.h"

using namespace yh;

#define ST_JOIN_BLOCKS 120   // tour_join's grid per frame (its lanes stride over the route)

namespace {
constexpr int kLegsMax = (YH_TOUR_MAX + 1) * YH_TOUR_MAX;
static_assert(kLegsMax <= kSolveTail, "a frame's leg matrix rides in its part of the solver's read-back block");

struct TourPoints { int32_t K, start, t[YH_TOUR_MAX]; };             // the start and the targets, linear indices
struct TourLegs { int32_t K, field[YH_TOUR_MAX], from[YH_TOUR_MAX]; };   // leg j walks next_{field[j]} from pixel from[j]
constexpr size_t kPointsWords = sizeof(TourPoints) / 4, kLegsWords = sizeof(TourLegs) / 4;

struct FrameTour {   // what the host keeps of frame b's tour
    std::vector<int32_t> targets;   // linear indices, t_0 .. t_{K-1}; empty: no tour for this frame
    int32_t order[YH_TOUR_MAX], leg_ends[YH_TOUR_MAX];
    float legs[kLegsMax], total = 0.0f;
};
}  // namespace

struct yh_scene_tour : PlanFrames {   // nodes, dirs [max][K*W*H] the joined routes; walk_out [max][2 * YH_TOUR_MAX]: nodes of leg j, then status of leg j
    int cap_k = 0;                 // the field buffers are sized for max_frames x this many fields; they only grow
    float* cost = nullptr;         // [max][K][H][W]
    int32_t* next = nullptr;       // [max][K][H][W]
    uint8_t* label = nullptr;      // [max][H][W]
    int2* segs = nullptr;          // [max][K][W*H] the legs' walks
    int32_t* host_walk = nullptr;  // pinned: walk_out as read back
    // the last call (the replay runs exactly this); in: the seeds, then points [n], then legs [n]
    int kmax = 0;
    std::vector<TourPoints> last_points;   // K = 0: no tour for that frame
    std::vector<FrameTour> frames;
};

namespace {

// seeds [ns][2] (pixel, field z): cost = 0 there
__global__ __launch_bounds__(256) void tour_seeds(const PathParams p, const int32_t* seeds, int ns) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < ns) p.cost[(size_t)seeds[2 * k + 1] * p.W * p.H + seeds[2 * k]] = 0.0f;
}

__global__ __launch_bounds__(64) void tour_legs(const PathParams p, const TourPoints* __restrict__ points, int kmax, float* legs) {
    const int b = blockIdx.z, e = threadIdx.x;
    const TourPoints& pts = points[b];   // (read where it lies: a copy indexed by a variable would live in scratch)
    if (e >= (pts.K + 1) * pts.K) return;
    const int a = e / pts.K, f = e - a * pts.K;
    legs[b * kLegsMax + e] = p.cost[((size_t)b * kmax + f) * p.W * p.H + (a == 0 ? pts.start : pts.t[a - 1])];
}

template <int CONN>
__global__ __launch_bounds__(256) void tour_next(const PathParams p, const TourPoints* __restrict__ points, int kmax, uint8_t* label) {
    const int b = blockIdx.z;
    const TourPoints& pts = points[b];
    if (pts.K < 1) return;   // (workgroup-uniform: no tour for this frame)
    const int i = blockIdx.x * 256 + threadIdx.x, npx = p.W * p.H;
    if (i >= npx) return;
    const size_t fo = (size_t)b * kmax * npx;
    const PathParams q = frame_of(p, b, (size_t)kmax * npx);
    const Around<CONN> e = around<CONN>(q, i);
    float best = SP_INF;
    int lab = 0;
    for (int f = 0; f < pts.K; ++f) {
        const float* cost = q.cost + (size_t)f * npx;
        p.next[fo + (size_t)f * npx + i] = i == pts.t[f] ? -1 : successor(e, cost, i);
        const float d = cost[i];
        if (d < best) { best = d; lab = f; }   // (strictly: the smallest f among equals)
    }
    label[(size_t)b * npx + i] = (uint8_t)lab;
}

// out[j] = nodes of leg j (its start and its target included), out[YH_TOUR_MAX + j] = 1 if it did not arrive within W * H nodes
__global__ __launch_bounds__(64) void tour_walk(const PathParams p, const TourLegs* __restrict__ legs, int kmax, int2* segs, int32_t* out) {
    const int b = blockIdx.z, j = blockIdx.x;
    const TourLegs& lg = legs[b];
    if (j >= lg.K) return;   // (workgroup-uniform)
    const size_t npx = (size_t)p.W * p.H, fo = (size_t)b * kmax * npx;
    // (no SP_BODY_ON_CACHE_LINE() here: with it this kernel ran 6 % slower than the parent's one-frame form, without it as the parent's)
    bool lost;
    const int n = chase(p.next + fo + (size_t)lg.field[j] * npx, p.W, p.H, lg.from[j], segs + fo + (size_t)j * npx, lost);
    if (threadIdx.x == 0) { out[b * 2 * YH_TOUR_MAX + j] = n; out[b * 2 * YH_TOUR_MAX + YH_TOUR_MAX + j] = lost ? 1 : 0; }
}

// Leg j holds the route's nodes off[j] .. off[j + 1] (both ends: a junction is the last node of one leg and the first of the next;
// a leg of one node adds nothing), off[0] = 0, off[j + 1] = off[j] + len[j] - 1; the route has off[K] + 1 nodes. Step g (node g ->
// node g + 1) lies in the leg with off[j] <= g < off[j + 1]: its magnitude is the difference of THAT leg's field.
__global__ __launch_bounds__(256) void tour_join(const PathParams p, const TourLegs* __restrict__ legs, int kmax, const int2* segs, const int32_t* len, int2* nodes, float2* dirs) {
    const int b = blockIdx.z;
    const TourLegs& lg = legs[b];
    const int K = lg.K;
    if (K < 1) return;   // (workgroup-uniform)
    const size_t npx = (size_t)p.W * p.H, fo = (size_t)b * kmax * npx;
    segs += fo; nodes += fo; dirs += fo; len += b * 2 * YH_TOUR_MAX;
    int off[YH_TOUR_MAX + 1];
    off[0] = 0;
#pragma unroll
    for (int j = 0; j < YH_TOUR_MAX; ++j) off[j + 1] = off[j] + (j < K ? len[j] - 1 : 0);
    const int L = off[YH_TOUR_MAX] + 1;
    // (unrolled with constant indices: off[] stays in registers)
    auto node = [&](int g) {   // the leg that holds node g: the last one whose first node lies before g
        int j = 0, base = 0;
#pragma unroll
        for (int k = 1; k < YH_TOUR_MAX; ++k) if (k < K && g > off[k]) { j = k; base = off[k]; }
        return segs[(size_t)j * npx + (g - base)];
    };
    for (int g = blockIdx.x * 256 + threadIdx.x; g < L; g += gridDim.x * 256) {
        const int2 a = node(g);
        nodes[g] = a;
        if (g + 1 >= L) continue;
        int field = lg.field[0];   // the leg that holds step g: the last one that starts at or before node g
#pragma unroll
        for (int k = 1; k < YH_TOUR_MAX; ++k) if (k < K && g >= off[k]) field = lg.field[k];
        const float* cost = p.cost + fo + (size_t)field * npx;
        const int2 c = node(g + 1);
        const float mag = __fsub_rn(cost[(size_t)a.y * p.W + a.x], cost[(size_t)c.y * p.W + c.x]);
        // (0 at step 0, and at a reversal, n_{g-1} == n_{g+1}: at a junction only)
        dirs[g] = make_float2(mag, g > 0 ? rotation(node(g - 1), a, c) : 0.0f);
    }
}

void free_fields(yh_scene_tour* q) {
    void* bufs[] = { q->cost, q->next, q->segs, q->nodes, q->dirs };
    for (void* b : bufs) if (b) (void)hipFree(b);
    q->cost = nullptr; q->next = nullptr; q->segs = nullptr; q->nodes = nullptr; q->dirs = nullptr;
    q->cap_k = 0;
}

// the state at the first tour (a handle that never tours pays nothing), with the buffers that do not depend on Kmax; those that do
// whenever Kmax exceeds what they were sized for
int ensure_tour(yh_scene* h, int kmax) {
    if (!h->tour) h->tour = new yh_scene_tour();
    yh_scene_tour* q = h->tour;
    const size_t mf = (size_t)h->max_frames, npx = (size_t)h->W * h->H;
    if (!q->label) SCHK(h, hipMalloc((void**)&q->label, mf * npx));
    if (!q->walk_out) SCHK(h, hipMalloc((void**)&q->walk_out, mf * 2 * YH_TOUR_MAX * 4));
    if (!q->host_walk) SCHK(h, hipHostMalloc((void**)&q->host_walk, mf * 2 * YH_TOUR_MAX * 4, hipHostMallocDefault));
    const int rc = plan_inputs_reserve(h, q->in, mf * (2 * YH_TOUR_MAX + kPointsWords + kLegsWords));
    if (rc) return rc;
    if (kmax <= q->cap_k) return YH_OK;
    SCHK(h, hipStreamSynchronize(h->stream));
    free_fields(q);
    q->last.planned = false;   // (the last tour lived in them)
    const size_t all = mf * kmax * npx;
    SCHK(h, hipMalloc((void**)&q->cost, all * 4));
    SCHK(h, hipMalloc((void**)&q->next, all * 4));
    SCHK(h, hipMalloc((void**)&q->segs, all * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&q->nodes, all * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&q->dirs, all * sizeof(float2)));
    q->cap_k = kmax;
    return YH_OK;
}

// legs [K + 1][K] -> the order of least total (f32, summed left to right), the lexicographically first among equals
float best_order(const float* legs, int K, int32_t* order) {
    int perm[YH_TOUR_MAX];
    for (int k = 0; k < K; ++k) perm[k] = k;
    float best = 0.0f;
    bool have = false;
    do {
        float total = legs[perm[0]];
        for (int j = 1; j < K; ++j) total = total + legs[(1 + perm[j - 1]) * K + perm[j]];
        if (!have || total < best) { best = total; have = true; std::copy(perm, perm + K, order); }
    } while (std::next_permutation(perm, perm + K));
    return best;
}

// the whole tour of q->n frames on the handle's stream: last_seeds / last_field (pixel and field z of every target), last_points,
// kmax, the connectivity. Returns when every route's length is known.
int run_tour(yh_scene* h, int conn) {
    yh_scene_tour* q = h->tour;
    const int n = q->n, kmax = q->kmax, ns = (int)q->last_seeds.size(), F = n * kmax;
    const size_t npx = (size_t)h->W * h->H;
    const size_t ws = plan_inputs_seeds(*q), wl = ws + n * kPointsWords;   // where the points and the legs lie
    memcpy(q->in.host + ws, q->last_points.data(), (size_t)n * sizeof(TourPoints));
    SCHK(h, hipMemcpyAsync(q->in.dev, q->in.host, wl * 4, hipMemcpyHostToDevice, h->stream));
    const int32_t* seeds = q->in.dev;
    const TourPoints* points = reinterpret_cast<const TourPoints*>(q->in.dev + ws);
    const TourLegs* legs = reinterpret_cast<const TourLegs*>(q->in.dev + wl);
    PathParams p;
    int rc = solve_begin(h, conn, h->max_frames * q->cap_k, n, p);
    if (rc) return rc;
    p.cost = q->cost; p.next = q->next;
    SCHK(h, hipMemsetD32Async((hipDeviceptr_t)q->cost, 0x7f800000, (size_t)F * npx, h->stream));   // +inf
    hipLaunchKernelGGL(tour_seeds, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, h->stream, p, seeds, ns);
    const SolveRound round = solve_field_round(h, p, conn, kmax, F);
    auto matrices = [&](uint32_t* tail) { hipLaunchKernelGGL(tour_legs, dim3(1, 1, (unsigned)n), dim3(64), 0, h->stream, p, points, kmax, reinterpret_cast<float*>(tail)); };
    if ((rc = solve_rounds(h, p, conn, F, q->last_seeds, h->batch ? "batch tour" : "tour", n * kLegsMax, matrices, &round, &q->last_field))) return rc;
    hipLaunchKernelGGL(conn == 8 ? tour_next<8> : tour_next<4>, dim3((unsigned)((npx + 255) / 256), 1, (unsigned)n), dim3(256), 0, h->stream, p, points, kmax, q->label);
    // per frame: the order, from the matrix the last batch's read brought; with it every leg's field and start: the walks are independent
    TourLegs* host_legs = reinterpret_cast<TourLegs*>(q->in.host + wl);
    for (int b = 0; b < n; ++b) {
        FrameTour& ft = q->frames[b];
        const TourPoints& pts = q->last_points[b];
        const int K = pts.K;
        TourLegs& lg = host_legs[b];
        lg = TourLegs();
        if (K < 1) continue;
        memcpy(ft.legs, h->solve->host + kSolveCnt + (size_t)b * kLegsMax, (size_t)(K + 1) * K * 4);
        ft.total = best_order(ft.legs, K, ft.order);
        lg.K = K;
        for (int j = 0; j < K; ++j) {
            lg.field[j] = ft.order[j];
            lg.from[j] = j == 0 ? pts.start : pts.t[ft.order[j - 1]];
        }
    }
    SCHK(h, hipMemcpyAsync(q->in.dev + wl, host_legs, (size_t)n * sizeof(TourLegs), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(tour_walk, dim3((unsigned)kmax, 1, (unsigned)n), dim3(64), 0, h->stream, p, legs, kmax, q->segs, q->walk_out);
    hipLaunchKernelGGL(tour_join, dim3(ST_JOIN_BLOCKS, 1, (unsigned)n), dim3(256), 0, h->stream, p, legs, kmax, q->segs, q->walk_out, q->nodes, q->dirs);
    SCHK(h, hipGetLastError());
    SCHK(h, hipMemcpyAsync(q->host_walk, q->walk_out, (size_t)n * 2 * YH_TOUR_MAX * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    q->path_len.assign(n, 0);
    for (int b = 0; b < n; ++b) {
        FrameTour& ft = q->frames[b];
        const int K = q->last_points[b].K;
        const int32_t* w = q->host_walk + (size_t)b * 2 * YH_TOUR_MAX;
        int32_t at = 0;
        for (int j = 0; j < K; ++j) {
            if (w[YH_TOUR_MAX + j]) return h->fail(YH_EHIP, h->frame_tag(b) + "tour walk: leg " + std::to_string(j) + " met no target within W*H steps (fields not those of a SANE frame?)");
            at += w[j] - 1;
            ft.leg_ends[j] = at;
        }
        if (K > 0) q->path_len[b] = at + 1;
    }
    return YH_OK;
}

// a frame's distinct targets from those chosen for it: a ball on an earlier ball's pixel is dropped, an explicit duplicate refused
int distinct_targets(yh_scene* h, const std::vector<int32_t>& chosen, bool given, std::vector<int32_t>& targets) {
    targets.clear();
    for (int32_t t : chosen) {
        if (std::find(targets.begin(), targets.end(), t) == targets.end()) { targets.push_back(t); continue; }
        if (given) return h->fail(YH_EINVAL, "duplicate target (" + std::to_string(t % h->W) + ", " + std::to_string(t / h->W) + "): a tour's targets are distinct pixels");
    }
    return YH_OK;
}

// ensures the state for n frames of kmax fields and clears the inputs of the last call (which is gone from here on)
int begin_inputs(yh_scene* h, int n, int kmax) {
    const int rc = ensure_tour(h, kmax);
    if (rc) { scene_tour_free(h); return rc; }
    yh_scene_tour* q = h->tour;
    q->last.planned = false;
    q->n = n; q->kmax = kmax;
    q->last_seeds.clear(); q->last_field.clear();
    q->last_points.assign(n, TourPoints()); q->frames.assign(n, FrameTour());
    return YH_OK;
}

// frame b of a call's inputs: its points, its seeds (field z = b kmax + f) and what the host keeps of its targets
void frame_inputs(yh_scene_tour* q, int b, const std::vector<int32_t>& targets, int32_t start) {
    TourPoints& pts = q->last_points[b];
    pts.K = (int32_t)targets.size(); pts.start = start;
    for (int f = 0; f < YH_TOUR_MAX; ++f) pts.t[f] = f < pts.K ? targets[f] : -1;
    for (int f = 0; f < pts.K; ++f) { q->last_seeds.push_back(targets[f]); q->last_field.push_back(b * q->kmax + f); }
    q->frames[b].targets = targets;
}

// the inputs of a call are in h->tour: run it, and it is the handle's last tour
int tour_now(yh_scene* h, int conn) {
    yh_scene_tour* q = h->tour;
    const int rc = run_tour(h, conn);
    if (rc) return rc;
    q->last.conn = conn; q->last.planned = true; q->last.frame = h->frames;
    return YH_OK;
}

int tour_read(yh_scene* h, int frame, int32_t* n_targets, int32_t* targets_xy, int32_t* order, float* legs, float* total, float* cost, int32_t* next, uint8_t* label,
              int32_t* path_xy, float* directions, int32_t* leg_ends, int32_t path_capacity, int32_t* path_len) {
    const yh_scene_tour* q = h->tour;
    const size_t npx = (size_t)h->W * h->H;
    const size_t fo = q ? (size_t)frame * q->kmax * npx : 0;   // the frame's first field, in pixels
    SolveLast one;
    int rc = solve_frame(h, q, frame, q ? q->kmax * npx : 0, "tour", one);
    if (rc) return rc;
    const FrameTour* ft = one.planned && one.frame == h->frames ? &q->frames[frame] : nullptr;
    const int K = ft ? (int)ft->targets.size() : 0;
    rc = solve_read(h, "tour", "plan the tour again", &one,
                    { { cost, q ? q->cost + fo : nullptr, K * npx * 4 }, { next, q ? q->next + fo : nullptr, K * npx * 4 }, { label, q ? q->label + frame * npx : nullptr, npx } },
                    path_xy, directions, path_capacity, path_len);
    if (rc) return rc;
    if (n_targets) *n_targets = K;
    for (int b = 0; b < K; ++b) {
        if (targets_xy) { targets_xy[2 * b] = ft->targets[b] % h->W; targets_xy[2 * b + 1] = ft->targets[b] / h->W; }
        if (order) order[b] = ft->order[b];
        if (leg_ends) leg_ends[b] = ft->leg_ends[b];
    }
    if (legs) memcpy(legs, ft->legs, (size_t)(K + 1) * K * 4);
    if (total) *total = ft->total;
    return YH_OK;
}

int tour_time(yh_scene* h, int32_t reps, float* ms, int32_t* rounds, int32_t* tile_runs) {
    yh_scene_tour* q = h->tour;
    // (a failed replay has overwritten part of the last tour: it is gone; the host's choice of the orders is inside the time)
    auto run = [&] { const int rc = run_tour(h, q->last.conn); if (rc) q->last.planned = false; return rc; };
    return solve_time(h, "tour", "plan the tour again", q ? &q->last : nullptr, reps, run, ms, rounds, tile_runs);
}

}  // namespace

namespace yh {
void scene_tour_free(yh_scene* h) {
    yh_scene_tour* q = h->tour;
    if (!q) return;
    free_fields(q);
    if (q->label) (void)hipFree(q->label);
    if (q->walk_out) (void)hipFree(q->walk_out);
    if (q->host_walk) (void)hipHostFree(q->host_walk);
    plan_inputs_free(q->in);
    delete q;
    h->tour = nullptr;
}
}  // namespace yh

extern "C" {

int yh_scene_plan_tour(yh_scene* h, const int32_t* targets_xy, int32_t n_targets, int32_t start_x, int32_t start_y) {
    return yh_scene_plan_tour_conn(h, targets_xy, n_targets, start_x, start_y, 4);
}

int yh_scene_plan_tour_conn(yh_scene* h, const int32_t* targets_xy, int32_t n_targets, int32_t start_x, int32_t start_y, int32_t connectivity) {
    if (!h) return YH_EINVAL;
    if (connectivity != 4 && connectivity != 8) return h->fail(YH_EINVAL, "connectivity " + std::to_string(connectivity) + ": 4 or 8");
    if (n_targets > YH_TOUR_MAX) return h->fail(YH_EINVAL, "n_targets " + std::to_string(n_targets) + " > YH_TOUR_MAX = " + std::to_string(YH_TOUR_MAX));
    std::vector<int32_t> chosen, targets;
    int rc = scene_plan_targets(h, targets_xy, n_targets, start_x, start_y, chosen);
    if (rc) return rc;
    if ((rc = distinct_targets(h, chosen, targets_xy != nullptr, targets))) return rc;
    if (connectivity == 8 && (rc = scene_plan_diagonals(h, h->diag_ok, h->diag_why))) return rc;
    // the batch of one: Kmax is the number of distinct targets
    if ((rc = begin_inputs(h, 1, (int)targets.size()))) return rc;
    frame_inputs(h->tour, 0, targets, (int32_t)((long long)start_y * h->W + start_x));
    h->tour->status.assign(1, YH_OK);
    return tour_now(h, connectivity);
}

int yh_scene_batch_plan_tour(yh_scene_batch* hb, const int32_t* targets_xy, int32_t n_targets, const int32_t* starts_xy, int32_t connectivity, int32_t* status) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (connectivity != 4 && connectivity != 8) return h->fail(YH_EINVAL, "connectivity " + std::to_string(connectivity) + ": 4 or 8");
    if (!starts_xy) return h->fail(YH_EINVAL, "starts_xy is null");
    if (n_targets > YH_TOUR_MAX) return h->fail(YH_EINVAL, "n_targets " + std::to_string(n_targets) + " > YH_TOUR_MAX = " + std::to_string(YH_TOUR_MAX));
    std::vector<int32_t> st;
    std::vector<std::vector<int32_t>> targets(hb->n);
    bool any = false;
    int rc = scene_batch_frames(hb, targets_xy, n_targets, starts_xy, nullptr, connectivity, st, [&](int b, const std::vector<int32_t>& chosen) {
        any = true;
        return distinct_targets(h, chosen, targets_xy != nullptr, targets[b]);
    });
    if (rc) return rc;
    if (!any) return h->fail(YH_ESTATE, "no target given and no frame of the batch has a ball inside it");
    if (status) std::copy(st.begin(), st.end(), status);
    h->err.clear();
    if ((rc = begin_inputs(h, hb->n, n_targets))) return rc;
    for (int b = 0; b < hb->n; ++b) frame_inputs(h->tour, b, targets[b], starts_xy[2 * b + 1] * h->W + starts_xy[2 * b]);
    h->tour->status = st;
    return tour_now(h, connectivity);
}

int yh_scene_tour_read(yh_scene* h, int32_t* n_targets, int32_t* targets_xy, int32_t* order, float* legs, float* total, float* cost, int32_t* next,
                       uint8_t* label, int32_t* path_xy, float* directions, int32_t* leg_ends, int32_t path_capacity, int32_t* path_len) {
    if (!h) return YH_EINVAL;
    return tour_read(h, 0, n_targets, targets_xy, order, legs, total, cost, next, label, path_xy, directions, leg_ends, path_capacity, path_len);
}

int yh_scene_batch_tour_read(yh_scene_batch* hb, int32_t frame, int32_t* n_targets, int32_t* targets_xy, int32_t* order, float* legs, float* total, float* cost,
                             int32_t* next, uint8_t* label, int32_t* path_xy, float* directions, int32_t* leg_ends, int32_t path_capacity, int32_t* path_len) {
    if (!hb) return YH_EINVAL;
    const int rc = hb->frame_ok(frame);
    if (rc) return rc;
    return tour_read(&hb->core, frame, n_targets, targets_xy, order, legs, total, cost, next, label, path_xy, directions, leg_ends, path_capacity, path_len);
}

int yh_scene_tour_time(yh_scene* h, int32_t reps, float* ms_per_tour, int32_t* rounds, int32_t* tile_runs) {
    if (!h || reps < 1 || !ms_per_tour) return YH_EINVAL;
    return tour_time(h, reps, ms_per_tour, rounds, tile_runs);
}

int yh_scene_batch_tour_time(yh_scene_batch* hb, int32_t reps, float* ms_per_batch, int32_t* rounds, int32_t* tile_runs) {
    if (!hb || reps < 1 || !ms_per_batch) return YH_EINVAL;
    return tour_time(&hb->core, reps, ms_per_batch, rounds, tile_runs);
}

}  // extern "C"
