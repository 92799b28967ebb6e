// scene_tour.hip — the tour (yh_scene_plan_tour): which ball first, then which, and the whole route. The reference stops at "the
// cheapest way to the nearest of the balls" and says so (path.rs:38 "Dijkstra's algorithm with 3 targets (yet to choose heuristic)",
// :35,:66 a ball[node] label "Use in optimizations and UI"). What is computed is the definition frozen in DESIGN.md §11 "Tour" and
// restated in tests/tour_ref.py: K <= YH_TOUR_MAX distinct targets; per target t_b the single-target cost field d_b and successor
// field next_b of scene_path.hip's planner (same graph, same edge terms, same association: the device functions of
// scene_path_dev.h); label[v] = the smallest b with d_b[v] == min_b d_b[v]; the leg matrix legs[0][b] = d_b[start],
// legs[1 + a][b] = d_b[t_a] (FROM t_a TO t_b: costs accumulate from the target outward, d_b[t_a] and d_a[t_b] differ in their last
// bits); the order minimising the f32 left-to-right sum of its legs, ties to the lexicographically smallest; the legs' walks joined.
// A plan is bound by serial depth (a round is as long as its slowest tile, ~42 of 300 workgroups have work), so the K fields relax in
// the SAME launches, the field as grid z: a tour's rounds are those of its slowest field, not their sum.
//
// Launches of one tour (the solver and its buffers are scene_solve.hip's, shared with scene_path.hip):
//   path_weights   (scene_solve.hip) once: the edge terms are shared by all fields.
//   tour_fill      cost[b] = +inf, 0 at t_b.
//   field_round    x rounds, grid (tiles x, tiles y, K) (scene_solve.hip): field b's one seed is t_b.
//   tour_legs      after every batch of rounds (the solver's after-batch hook): the K (K + 1) entries of the leg matrix into the tail of
//                  the block the host reads the batch's counters from: it arrives with the last counters (earlier copies are ignored).
//   tour_next      one lane per pixel: next_b for the K fields and the label (the pixel's edge terms read once for all of them).
//   (host)         the order: all K! <= 720 permutations from the leg matrix.
//   tour_walk      K waves, one per leg: leg j chases next_{o_j} from the start (j = 0) or from t_{o_{j-1}} into its own segment.
//   tour_join      the segments into one node list (a junction node once) and the directions over it.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "scene.h"
#include "scene_path_dev.h"
#include "yh_internal.h"

using namespace yh;

#define ST_JOIN_BLOCKS 120   // tour_join's grid (its lanes stride over the route)

struct yh_scene_tour : SolveLast {   // (the joined route [K * W * H], the start, the connectivity and whether a tour exists: SolveLast)
    int cap_k = 0;               // the buffers below are sized for this many fields; they only grow
    float* cost = nullptr;       // [K][H][W]
    int32_t* next = nullptr;     // [K][H][W]
    uint8_t* label = nullptr;    // [H][W]
    int2* segs = nullptr;        // [K][W * H] the legs' walks
    int32_t* walk_out = nullptr; // [2 * YH_TOUR_MAX]: nodes of leg j, then status of leg j
    std::vector<int32_t> targets;   // of the last tour: linear indices, t_0 .. t_{K-1}
    int32_t order[YH_TOUR_MAX], leg_ends[YH_TOUR_MAX];
    float legs[(YH_TOUR_MAX + 1) * YH_TOUR_MAX], total = 0.0f;
};

namespace {

constexpr int kLegsMax = (YH_TOUR_MAX + 1) * YH_TOUR_MAX;
static_assert(kLegsMax <= kSolveTail && 2 * YH_TOUR_MAX <= kSolveWalk, "the leg matrix and walk_out ride in the solver's read-back block");

struct TourPoints { int32_t K, start, t[YH_TOUR_MAX]; };             // the start and the targets, linear indices
struct TourLegs { int32_t K, field[YH_TOUR_MAX], from[YH_TOUR_MAX]; };   // leg j walks next_{field[j]} from pixel from[j]

__global__ __launch_bounds__(256) void tour_fill(const PathParams p, const TourPoints pts) {
    const int i = blockIdx.x * 256 + threadIdx.x, npx = p.W * p.H;
    if (i < npx)
        for (int b = 0; b < pts.K; ++b) p.cost[(size_t)b * npx + i] = i == pts.t[b] ? 0.0f : SP_INF;
}

__global__ __launch_bounds__(64) void tour_legs(const PathParams p, const TourPoints pts, float* legs) {
    const int e = threadIdx.x;
    if (e >= (pts.K + 1) * pts.K) return;
    const int a = e / pts.K, b = e - a * pts.K;
    legs[e] = p.cost[(size_t)b * p.W * p.H + (a == 0 ? pts.start : pts.t[a - 1])];
}

template <int CONN>
__global__ __launch_bounds__(256) void tour_next(const PathParams p, const TourPoints pts, uint8_t* label) {
    const int i = blockIdx.x * 256 + threadIdx.x, npx = p.W * p.H;
    if (i >= npx) return;
    const Around<CONN> e = around<CONN>(p, i);
    float best = SP_INF;
    int lab = 0;
    for (int b = 0; b < pts.K; ++b) {
        const float* cost = p.cost + (size_t)b * npx;
        p.next[(size_t)b * npx + i] = i == pts.t[b] ? -1 : successor(e, cost, i);
        const float d = cost[i];
        if (d < best) { best = d; lab = b; }   // (strictly: the smallest b among equals)
    }
    label[i] = (uint8_t)lab;
}

// out[j] = nodes of leg j (its start and its target included), out[YH_TOUR_MAX + j] = 1 if it did not arrive within W * H nodes
__global__ __launch_bounds__(64) void tour_walk(const PathParams p, const TourLegs legs, int2* segs, int32_t* out) {
    const int j = blockIdx.x, npx = p.W * p.H;
    bool lost;
    const int n = chase(p.next + (size_t)legs.field[j] * npx, p.W, p.H, legs.from[j], segs + (size_t)j * npx, lost);
    if (threadIdx.x == 0) { out[j] = n; out[YH_TOUR_MAX + j] = lost ? 1 : 0; }
}

// Leg j holds the route's nodes off[j] .. off[j + 1] (both ends: a junction is the last node of one leg and the first of the next;
// a leg of one node adds nothing), off[0] = 0, off[j + 1] = off[j] + len[j] - 1; the route has off[K] + 1 nodes. Step g (node g ->
// node g + 1) lies in the leg with off[j] <= g < off[j + 1]: its magnitude is the difference of THAT leg's field.
__global__ __launch_bounds__(256) void tour_join(const PathParams p, const TourLegs legs, const int2* segs, const int32_t* len, int2* nodes, float2* dirs) {
    const int npx = p.W * p.H;
    int off[YH_TOUR_MAX + 1];
    off[0] = 0;
#pragma unroll
    for (int j = 0; j < YH_TOUR_MAX; ++j) off[j + 1] = off[j] + (j < legs.K ? len[j] - 1 : 0);
    const int L = off[YH_TOUR_MAX] + 1;
    // (unrolled with constant indices: off[] stays in registers)
    auto node = [&](int g) {   // the leg that holds node g: the last one whose first node lies before g
        int j = 0, base = 0;
#pragma unroll
        for (int k = 1; k < YH_TOUR_MAX; ++k) if (k < legs.K && g > off[k]) { j = k; base = off[k]; }
        return segs[(size_t)j * npx + (g - base)];
    };
    for (int g = blockIdx.x * 256 + threadIdx.x; g < L; g += gridDim.x * 256) {
        const int2 a = node(g);
        nodes[g] = a;
        if (g + 1 >= L) continue;
        int field = legs.field[0];   // the leg that holds step g: the last one that starts at or before node g
#pragma unroll
        for (int k = 1; k < YH_TOUR_MAX; ++k) if (k < legs.K && g >= off[k]) field = legs.field[k];
        const float* cost = p.cost + (size_t)field * npx;
        const int2 b = node(g + 1);
        const float mag = __fsub_rn(cost[(size_t)a.y * p.W + a.x], cost[(size_t)b.y * p.W + b.x]);
        // (0 at step 0, and at a reversal, n_{g-1} == n_{g+1}: at a junction only)
        dirs[g] = make_float2(mag, g > 0 ? rotation(node(g - 1), a, b) : 0.0f);
    }
}

void free_fields(yh_scene_tour* q) {
    void* bufs[] = { q->cost, q->next, q->segs, q->nodes, q->dirs };
    for (void* b : bufs) if (b) (void)hipFree(b);
    q->cost = nullptr; q->next = nullptr; q->segs = nullptr; q->nodes = nullptr; q->dirs = nullptr;
    q->cap_k = 0;
}

// the buffers that do not depend on K at the first tour; those that do whenever K exceeds what they were sized for
int ensure_buffers(yh_scene* h, int K) {
    yh_scene_tour* q = h->tour;
    const size_t npx = (size_t)h->W * h->H;
    if (!q->label) SCHK(h, hipMalloc((void**)&q->label, npx));
    if (!q->walk_out) SCHK(h, hipMalloc((void**)&q->walk_out, 2 * YH_TOUR_MAX * 4));
    if (K <= q->cap_k) return YH_OK;
    SCHK(h, hipStreamSynchronize(h->stream));
    free_fields(q);
    q->planned = false;   // (the last tour lived in them)
    SCHK(h, hipMalloc((void**)&q->cost, K * npx * 4));
    SCHK(h, hipMalloc((void**)&q->next, K * npx * 4));
    SCHK(h, hipMalloc((void**)&q->segs, K * npx * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&q->nodes, K * npx * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&q->dirs, K * npx * sizeof(float2)));
    q->cap_k = K;
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

// the whole tour on the handle's stream; returns when the route's length is known
int run_tour(yh_scene* h, const std::vector<int32_t>& targets, int32_t start, int conn) {
    yh_scene_tour* q = h->tour;
    const int K = (int)targets.size(), npx = h->W * h->H;
    TourPoints pts;
    pts.K = K; pts.start = start;
    for (int b = 0; b < YH_TOUR_MAX; ++b) pts.t[b] = b < K ? targets[b] : -1;
    PathParams p;
    int rc = solve_begin(h, conn, K, 1, p);
    if (rc) return rc;
    p.cost = q->cost; p.next = q->next;
    hipLaunchKernelGGL(tour_fill, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, h->stream, p, pts);
    auto legs = [&](uint32_t* tail) { hipLaunchKernelGGL(tour_legs, dim3(1), dim3(64), 0, h->stream, p, pts, reinterpret_cast<float*>(tail)); };
    if ((rc = solve_rounds(h, p, conn, K, targets, "tour", kLegsMax, legs))) return rc;
    hipLaunchKernelGGL(conn == 8 ? tour_next<8> : tour_next<4>, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, h->stream, p, pts, q->label);
    // the order, from the matrix the last batch's read brought; then the legs are independent: leg j's field and start are fixed
    memcpy(q->legs, h->solve->host + kSolveCnt, (size_t)(K + 1) * K * 4);
    q->total = best_order(q->legs, K, q->order);
    TourLegs lg;
    lg.K = K;
    for (int j = 0; j < YH_TOUR_MAX; ++j) {
        lg.field[j] = j < K ? q->order[j] : 0;
        lg.from[j] = j == 0 ? start : j < K ? targets[q->order[j - 1]] : 0;
    }
    hipLaunchKernelGGL(tour_walk, dim3((unsigned)K), dim3(64), 0, h->stream, p, lg, q->segs, q->walk_out);
    hipLaunchKernelGGL(tour_join, dim3(ST_JOIN_BLOCKS), dim3(256), 0, h->stream, p, lg, q->segs, q->walk_out, q->nodes, q->dirs);
    SCHK(h, hipGetLastError());
    int32_t* wo = reinterpret_cast<int32_t*>(h->solve->host + kSolveCnt + kSolveTail);
    SCHK(h, hipMemcpyAsync(wo, q->walk_out, 2 * YH_TOUR_MAX * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    int32_t at = 0;
    for (int j = 0; j < K; ++j) {
        if (wo[YH_TOUR_MAX + j]) return h->fail(YH_EHIP, "tour walk: leg " + std::to_string(j) + " met no target within W*H steps (fields not those of a SANE frame?)");
        at += wo[j] - 1;
        q->leg_ends[j] = at;
    }
    q->path_len = at + 1;
    return YH_OK;
}

}  // namespace

namespace yh {
void scene_tour_free(yh_scene* h) {
    yh_scene_tour* q = h->tour;
    if (!q) return;
    free_fields(q);
    if (q->label) (void)hipFree(q->label);
    if (q->walk_out) (void)hipFree(q->walk_out);
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
    for (int32_t t : chosen) {
        if (std::find(targets.begin(), targets.end(), t) == targets.end()) { targets.push_back(t); continue; }
        // (a ball on an earlier ball's pixel is dropped)
        if (targets_xy) return h->fail(YH_EINVAL, "duplicate target (" + std::to_string(t % h->W) + ", " + std::to_string(t / h->W) + "): a tour's targets are distinct pixels");
    }
    if (connectivity == 8 && (rc = scene_plan_diagonals(h, h->diag_ok, h->diag_why))) return rc;
    if (!h->tour) h->tour = new yh_scene_tour();   // the tour's buffers are allocated at the first tour: a handle that never tours pays nothing
    rc = ensure_buffers(h, (int)targets.size());
    if (rc) { scene_tour_free(h); return rc; }
    yh_scene_tour* q = h->tour;
    q->planned = false;
    const int32_t start = (int32_t)((long long)start_y * h->W + start_x);
    rc = run_tour(h, targets, start, connectivity);
    if (rc) return rc;
    q->conn = connectivity;
    q->planned = true; q->frame = h->frames; q->targets = targets; q->start = start;
    return YH_OK;
}

int yh_scene_tour_read(yh_scene* h, int32_t* n_targets, int32_t* targets_xy, int32_t* order, float* legs, float* total, float* cost, int32_t* next,
                       uint8_t* label, int32_t* path_xy, float* directions, int32_t* leg_ends, int32_t path_capacity, int32_t* path_len) {
    if (!h) return YH_EINVAL;
    const yh_scene_tour* q = h->tour;
    const int K = q ? (int)q->targets.size() : 0;
    const size_t npx = (size_t)h->W * h->H;
    const int rc = solve_read(h, "tour", "plan the tour again", q, { { cost, q ? q->cost : nullptr, K * npx * 4 }, { next, q ? q->next : nullptr, K * npx * 4 }, { label, q ? q->label : nullptr, npx } },
                              path_xy, directions, path_capacity, path_len);
    if (rc) return rc;
    if (n_targets) *n_targets = K;
    for (int b = 0; b < K; ++b) {
        if (targets_xy) { targets_xy[2 * b] = q->targets[b] % h->W; targets_xy[2 * b + 1] = q->targets[b] / h->W; }
        if (order) order[b] = q->order[b];
        if (leg_ends) leg_ends[b] = q->leg_ends[b];
    }
    if (legs) memcpy(legs, q->legs, (size_t)(K + 1) * K * 4);
    if (total) *total = q->total;
    return YH_OK;
}

int yh_scene_tour_time(yh_scene* h, int32_t reps, float* ms_per_tour, int32_t* rounds, int32_t* tile_runs) {
    if (!h || reps < 1 || !ms_per_tour) return YH_EINVAL;
    yh_scene_tour* q = h->tour;
    // (a failed replay has overwritten part of the last tour: it is gone; the host's choice of the order is inside the time)
    auto run = [&] { const int rc = run_tour(h, q->targets, q->start, q->conn); if (rc) q->planned = false; return rc; };
    return solve_time(h, "tour", "plan the tour again", q, reps, run, ms_per_tour, rounds, tile_runs);
}

}  // extern "C"
