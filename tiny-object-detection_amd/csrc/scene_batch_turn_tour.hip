// scene_batch_turn_tour.hip — yh_scene_batch_plan_turn_tour: the turn-aware tour (scene_turn_tour.hip; DESIGN.md §11 "Turn tour") for
// every frame of a scene batch in shared solver rounds (DESIGN.md §11 "Scene batch: turn tours"). Frame b has exactly the results of
// yh_scene_plan_turn_tour on a yh_scene of the same size fed that frame alone: every kernel here takes its frame from blockIdx.z,
// advances its own copy of the parameter block and of its pointers to that frame and runs the body the single handle's kernel runs
// (scene_turn_dev.h, scene_turn_tour_dev.h). A field is unique (every weight >= 1) and has its own eight layers and tile flags, so
// fields that share rounds cannot change each other's bits; the batch takes the rounds of its slowest field, not their sum.
//
// K is ragged: n_targets = Kmax is one number per call, frame b has K_b <= Kmax targets (fewer balls, or balls on one pixel). Field f
// of frame b is solver field z = b Kmax + f - NOT b K_b + f. What advances by what:
//   edge, edge2 (and map, conn0, conn1 under batch_weights)   b W H          one set of edge terms per frame, shared by its fields
//   cost f32, act u8 [n][Kmax][8][H][W]                        z 8 W H
//   label u8 [n][8][H][W]                                      b 8 W H
//   seg_nodes, seg_turns, seg_dirs [n][Kmax][W H]              z W H          leg j of frame b: z = b Kmax + j
//   nodes, dirs, turns [n][Kmax W H]                           b Kmax W H     a joined route is at most K W H long
//   table i32 [n][3][kEntriesMax], walk_out i32 [n][4 YH_TOUR_MAX], points, legs [n]
//   flags [2][n Kmax][ntiles]                                  as tt_round indexes them, F = n Kmax
// Bytes per pixel: 80 per (frame, target) - cost 32, act 8, the legs' segments 20, the joined route 20 - plus 8 per frame for the
// label; allocated at the first call for max_frames x the largest Kmax so far, growing only (growing drops the last batched turn
// tour). 640 x 480 with max_frames = 64 and Kmax = 6 is 9.6 GB: a caller sizes max_frames and n_targets accordingly.
// A field f >= K_b has no seed: it flags nothing and its tiles exit at once (the solver's ragged field_of form); the act, arrive,
// walk and join kernels skip it.
//
// Launches of one call, their number independent of n: the uploads (seeds with their fields, points [n]), batch_weights<8>
// (scene_batch.hip), one fill of 8 n Kmax W H values with +inf, btt_seeds (0 in the eight layers of the seed's field), btt_round x
// rounds through scene_solve.hip's host loop (SolveRound{.., 8}, ragged seeds, tiles x n Kmax), btt_act (pixels x 1 x n), btt_arrive
// (one wave per (entry, frame)), ONE copy of the tables and ONE wait; the order of every frame on the host (best_order); one upload
// of the legs [n], btt_walk (Kmax x 1 x n waves), btt_join (blocks x 1 x n), ONE copy of n x 4 YH_TOUR_MAX words and ONE wait.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "scene.h"
#include "scene_batch.h"
#include "scene_path_dev.h"
#include "scene_turn_dev.h"
#include "scene_turn_tour_dev.h"
#include "yh_internal.h"

using namespace yh;

namespace {
struct FrameTour {   // what the host keeps of frame b's turn tour (yh_scene_turn_tour's members of the same names)
    std::vector<int32_t> targets;   // linear indices, t_0 .. t_{K-1}; empty: no tour for this frame
    int32_t order[YH_TOUR_MAX], leg_ends[YH_TOUR_MAX], leg_headings[YH_TOUR_MAX], path_len = 0;
    float legs[kEntriesMax], total = 0.0f;
    uint8_t arrive[kEntriesMax];
};
}  // namespace

struct yh_scene_batch_turn_tour {
    int cap_k = 0;                   // the field buffers are sized for max_frames x this many fields; they only grow
    float* cost = nullptr;           // [max][K][8][H][W]
    uint8_t* act = nullptr;          // [max][K][8][H][W]
    uint8_t* label = nullptr;        // [max][8][H][W]
    int2* seg_nodes = nullptr;       // [max][K][W*H] the legs' walks
    int32_t* seg_turns = nullptr;
    float2* seg_dirs = nullptr;
    int2* nodes = nullptr;           // [max][K*W*H] the joined routes
    float2* dirs = nullptr;
    int32_t* turns = nullptr;
    int32_t* table = nullptr;        // [max][3][kEntriesMax]
    int32_t* walk_out = nullptr;     // [max][4 * YH_TOUR_MAX]
    TurnTourPoints* points = nullptr;   // [max]
    TurnTourLegs* legs = nullptr;       // [max]
    int32_t* seeds = nullptr;        // [max * YH_TOUR_MAX][2]: linear index, field z
    int32_t* host = nullptr;         // pinned: the tables [max][3][kEntriesMax], then walk_out [max][4 * YH_TOUR_MAX], as read back
    SolveLast last;                  // planned, frame generation
    // the last call (the replay runs exactly this)
    int n = 0, kmax = 0;
    float tau = 1.0f;
    std::vector<int32_t> status, last_seeds, last_field, pairs;
    std::vector<TurnTourPoints> last_points;
    std::vector<TurnTourLegs> last_legs;
    std::vector<FrameTour> frames;
};

namespace {

// frame b of a turn tour batch of Kmax fields per frame: the edge terms advance by W H as everywhere, cost to the frame's field 0
__device__ __forceinline__ PathParams tour_frame_of(const PathParams& p, int b, int kmax) {
    PathParams q = p;
    const size_t npx = (size_t)p.W * p.H;
    q.edge += b * npx; q.edge2 += b * npx; q.cost += (size_t)b * kmax * 8 * npx;
    return q;
}

// seeds [ns][2] (pixel, field z): cost = 0 in all eight layers of that field there
__global__ __launch_bounds__(256) void btt_seeds(const PathParams p, const int32_t* seeds, int ns) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= 8 * ns) return;
    p.cost[((size_t)seeds[2 * (k >> 3) + 1] * 8 + (k & 7)) * p.W * p.H + seeds[2 * (k >> 3)]] = 0.0f;
}

__global__ __launch_bounds__(SP_NT) void btt_round(const PathParams p, float tau, int kmax, int F, int parity, uint32_t* cnt_next) {
    const int z = blockIdx.z, b = z / kmax;
    turn_round_body(turn_field_of(tour_frame_of(p, b, kmax), z - b * kmax), tau, p.flags + (size_t)(parity * F + z) * p.ntiles,
                    p.flags + (size_t)((parity ^ 1) * F + z) * p.ntiles, cnt_next);
}

__global__ __launch_bounds__(256) void btt_act(const PathParams p, const TurnTourPoints* __restrict__ points, int kmax, float tau, uint8_t* act, uint8_t* label) {
    const int b = blockIdx.z;
    const TurnTourPoints& pts = points[b];   // (read where it lies: a copy indexed by a variable would live in scratch)
    if (pts.K < 1) return;   // (workgroup-uniform: no tour for this frame)
    const size_t npx = (size_t)p.W * p.H;
    turn_tour_act_body(tour_frame_of(p, b, kmax), pts, tau, act + (size_t)b * kmax * 8 * npx, label + (size_t)b * 8 * npx);
}

__global__ __launch_bounds__(64) void btt_arrive(const PathParams p, const TurnTourPoints* __restrict__ points, int kmax, const uint8_t* act, int32_t* table) {
    const int b = blockIdx.z;
    const TurnTourPoints& pts = points[b];   // (read where it lies: a copy indexed by a variable would live in scratch)
    if ((int)blockIdx.x >= (1 + 8 * pts.K) * pts.K) return;   // (workgroup-uniform: this frame's table ends before this entry)
    turn_tour_arrive_body(tour_frame_of(p, b, kmax), pts, act + (size_t)b * kmax * 8 * p.W * p.H, table + (size_t)b * 3 * kEntriesMax);
}

__global__ __launch_bounds__(64) void btt_walk(const PathParams p, const TurnTourLegs* __restrict__ legs, int kmax, const uint8_t* act, int2* seg_nodes, int32_t* seg_turns, float2* seg_dirs,
                                               int32_t* out) {
    const int b = blockIdx.z;
    const TurnTourLegs& lg = legs[b];
    if ((int)blockIdx.x >= lg.K) return;   // (workgroup-uniform)
    const size_t npx = (size_t)p.W * p.H, fo = (size_t)b * kmax * npx;
    turn_tour_walk_body(tour_frame_of(p, b, kmax), lg, act + fo * 8, seg_nodes + fo, seg_turns + fo, seg_dirs + fo, out + b * 4 * YH_TOUR_MAX);
}

__global__ __launch_bounds__(256) void btt_join(const PathParams p, const TurnTourLegs* __restrict__ legs, int kmax, const int2* seg_nodes, const int32_t* seg_turns, const float2* seg_dirs,
                                                int32_t* out, int2* nodes, int32_t* turns, float2* dirs) {
    const int b = blockIdx.z, K = legs[b].K;
    if (K < 1) return;   // (workgroup-uniform)
    const size_t fo = (size_t)b * kmax * p.W * p.H;
    turn_tour_join_body(p, K, seg_nodes + fo, seg_turns + fo, seg_dirs + fo, out + b * 4 * YH_TOUR_MAX, nodes + fo, turns + fo, dirs + fo);
}

void free_fields(yh_scene_batch_turn_tour* q) {
    void* bufs[] = { q->cost, q->act, q->seg_nodes, q->seg_turns, q->seg_dirs, q->nodes, q->dirs, q->turns };
    for (void* b : bufs) if (b) (void)hipFree(b);
    q->cost = nullptr; q->act = nullptr; q->seg_nodes = nullptr; q->seg_turns = nullptr; q->seg_dirs = nullptr; q->nodes = nullptr; q->dirs = nullptr; q->turns = nullptr;
    q->cap_k = 0;
}

// the buffers that do not depend on Kmax at the first call; those that do whenever Kmax exceeds what they were sized for
int ensure_buffers(yh_scene_batch* hb, int kmax) {
    yh_scene* h = &hb->core;
    yh_scene_batch_turn_tour* q = hb->turn_tour;
    const size_t mf = (size_t)hb->max_frames, npx = (size_t)h->W * h->H;
    if (!q->label) SCHK(h, hipMalloc((void**)&q->label, mf * 8 * npx));
    if (!q->table) SCHK(h, hipMalloc((void**)&q->table, mf * 3 * kEntriesMax * 4));
    if (!q->walk_out) SCHK(h, hipMalloc((void**)&q->walk_out, mf * 4 * YH_TOUR_MAX * 4));
    if (!q->points) SCHK(h, hipMalloc((void**)&q->points, mf * sizeof(TurnTourPoints)));
    if (!q->legs) SCHK(h, hipMalloc((void**)&q->legs, mf * sizeof(TurnTourLegs)));
    if (!q->seeds) SCHK(h, hipMalloc((void**)&q->seeds, mf * YH_TOUR_MAX * 2 * 4));
    if (!q->host) SCHK(h, hipHostMalloc((void**)&q->host, mf * (3 * kEntriesMax + 4 * YH_TOUR_MAX) * 4, hipHostMallocDefault));
    if (kmax <= q->cap_k) return YH_OK;
    SCHK(h, hipStreamSynchronize(h->stream));
    free_fields(q);
    q->last.planned = false;   // (the last batched turn tour lived in them)
    const size_t all = mf * kmax * npx;
    SCHK(h, hipMalloc((void**)&q->cost, all * 8 * 4));
    SCHK(h, hipMalloc((void**)&q->act, all * 8));
    SCHK(h, hipMalloc((void**)&q->seg_nodes, all * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&q->seg_turns, all * 4));
    SCHK(h, hipMalloc((void**)&q->seg_dirs, all * sizeof(float2)));
    SCHK(h, hipMalloc((void**)&q->nodes, all * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&q->dirs, all * sizeof(float2)));
    SCHK(h, hipMalloc((void**)&q->turns, all * 4));
    q->cap_k = kmax;
    return YH_OK;
}

// the whole turn tour of q->n frames on the handle's stream: last_seeds / last_field (pixel and field z of every target), last_points
// (K = 0: no tour for that frame), kmax, tau. Returns when every route's length is known.
int run_turn_tour(yh_scene_batch* hb) {
    yh_scene* h = &hb->core;
    yh_scene_batch_turn_tour* q = hb->turn_tour;
    const int n = q->n, kmax = q->kmax, ns = (int)q->last_seeds.size(), F = n * kmax;
    const size_t npx = (size_t)h->W * h->H;
    const float tau = q->tau;
    q->pairs.resize((size_t)ns * 2);
    for (int k = 0; k < ns; ++k) { q->pairs[2 * k] = q->last_seeds[k]; q->pairs[2 * k + 1] = q->last_field[k]; }
    SCHK(h, hipMemcpyAsync(q->seeds, q->pairs.data(), q->pairs.size() * 4, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipMemcpyAsync(q->points, q->last_points.data(), (size_t)n * sizeof(TurnTourPoints), hipMemcpyHostToDevice, h->stream));
    PathParams p;
    int rc = solve_alloc(h, 8, hb->max_frames * q->cap_k, hb->max_frames, p);
    if (rc) return rc;
    p.cost = q->cost; p.next = nullptr;
    scene_batch_weights(h, p, 8, n);
    SCHK(h, hipMemsetD32Async((hipDeviceptr_t)q->cost, 0x7f800000, (size_t)F * 8 * npx, h->stream));   // +inf
    hipLaunchKernelGGL(btt_seeds, dim3((unsigned)((8 * (size_t)ns + 255) / 256)), dim3(256), 0, h->stream, p, q->seeds, ns);
    const SolveRound round{ [&](const dim3& tiles, int parity, uint32_t* cnt_next) {
        hipLaunchKernelGGL(btt_round, tiles, dim3(SP_NT), 0, h->stream, p, tau, kmax, F, parity, cnt_next);
    }, 8 };
    if ((rc = solve_rounds(h, p, 8, F, q->last_seeds, "batch turn tour", 0, nullptr, &round, &q->last_field))) return rc;
    hipLaunchKernelGGL(btt_act, dim3((unsigned)((npx + 255) / 256), 1, (unsigned)n), dim3(256), 0, h->stream, p, q->points, kmax, tau, q->act, q->label);
    hipLaunchKernelGGL(btt_arrive, dim3((unsigned)((1 + 8 * kmax) * kmax), 1, (unsigned)n), dim3(64), 0, h->stream, p, q->points, kmax, q->act, q->table);
    SCHK(h, hipGetLastError());
    SCHK(h, hipMemcpyAsync(q->host, q->table, (size_t)n * 3 * kEntriesMax * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    // per frame: the tables, the order, and with it every leg's field and start state
    q->last_legs.assign(n, TurnTourLegs());
    for (int b = 0; b < n; ++b) {
        FrameTour& ft = q->frames[b];
        const TurnTourPoints& pts = q->last_points[b];
        const int K = pts.K;
        if (K < 1) continue;
        const int32_t* tab = q->host + (size_t)b * 3 * kEntriesMax;
        for (int e = 0; e < (1 + 8 * K) * K; ++e) {
            if (tab[2 * kEntriesMax + e])
                return h->fail(YH_EHIP, "frame " + std::to_string(b) + ": turn tour: the walk of leg table entry (" + std::to_string(e / K) + ", " + std::to_string(e % K) +
                                            ") met no target within 8*W*H actions (fields not those of a SANE frame?)");
            memcpy(&ft.legs[e], &tab[e], 4);
            ft.arrive[e] = (uint8_t)tab[kEntriesMax + e];
        }
        int32_t row[YH_TOUR_MAX];
        ft.total = best_order(ft.legs, ft.arrive, K, ft.order, row);
        TurnTourLegs& lg = q->last_legs[b];
        lg.K = K;
        for (int j = 0; j < YH_TOUR_MAX; ++j) {
            lg.field[j] = j < K ? ft.order[j] : 0;
            lg.from[j] = j == 0 ? pts.start : j < K ? pts.t[ft.order[j - 1]] : 0;
            lg.heading[j] = j == 0 ? pts.heading : j < K ? ft.leg_headings[j - 1] : 0;
            if (j < K) ft.leg_headings[j] = ft.arrive[row[j] * K + ft.order[j]];
        }
    }
    SCHK(h, hipMemcpyAsync(q->legs, q->last_legs.data(), (size_t)n * sizeof(TurnTourLegs), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(btt_walk, dim3((unsigned)kmax, 1, (unsigned)n), dim3(64), 0, h->stream, p, q->legs, kmax, q->act, q->seg_nodes, q->seg_turns, q->seg_dirs, q->walk_out);
    hipLaunchKernelGGL(btt_join, dim3(TT_JOIN_BLOCKS, 1, (unsigned)n), dim3(256), 0, h->stream, p, q->legs, kmax, q->seg_nodes, q->seg_turns, q->seg_dirs, q->walk_out, q->nodes,
                       q->turns, q->dirs);
    SCHK(h, hipGetLastError());
    int32_t* wo = q->host + (size_t)hb->max_frames * 3 * kEntriesMax;
    SCHK(h, hipMemcpyAsync(wo, q->walk_out, (size_t)n * 4 * YH_TOUR_MAX * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    for (int b = 0; b < n; ++b) {
        FrameTour& ft = q->frames[b];
        const int K = q->last_points[b].K;
        const int32_t* w = wo + (size_t)b * 4 * YH_TOUR_MAX;
        for (int j = 0; j < K; ++j) {
            if (w[2 * j + 1])
                return h->fail(YH_EHIP, "frame " + std::to_string(b) + ": turn tour walk: leg " + std::to_string(j) + " met no target within 8*W*H actions (fields not those of a SANE frame?)");
            ft.leg_ends[j] = w[2 * YH_TOUR_MAX + j];
        }
        ft.path_len = K < 1 ? 0 : w[3 * YH_TOUR_MAX];
    }
    return YH_OK;
}

}  // namespace

namespace yh {
void scene_batch_turn_tour_free(yh_scene_batch* hb) {
    yh_scene_batch_turn_tour* q = hb->turn_tour;
    if (!q) return;
    free_fields(q);
    void* bufs[] = { q->label, q->table, q->walk_out, q->points, q->legs, q->seeds };
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (q->host) (void)hipHostFree(q->host);
    delete q;
    hb->turn_tour = nullptr;
}
}  // namespace yh

extern "C" {

int yh_scene_batch_plan_turn_tour(yh_scene_batch* hb, const int32_t* targets_xy, int32_t n_targets, const int32_t* starts_xy, const int32_t* start_headings,
                                  float turn_price, int32_t* status) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (!starts_xy) return h->fail(YH_EINVAL, "starts_xy is null");
    if (!start_headings) return h->fail(YH_EINVAL, "start_headings is null");
    if (!std::isfinite(turn_price) || turn_price < 1.0f || turn_price > 1024.0f)
        return h->fail(YH_EINVAL, "turn price must be a finite number in [1, 1024] (every weight >= 1 is what makes the field unique)");
    if (n_targets > YH_TOUR_MAX) return h->fail(YH_EINVAL, "n_targets " + std::to_string(n_targets) + " > YH_TOUR_MAX = " + std::to_string(YH_TOUR_MAX));
    if (!h->ran || hb->n < 1) return h->fail(YH_ESTATE, "no frame has been appended");
    const int n = hb->n;
    const auto framed = [&](int b, int rc) { h->err = "frame " + std::to_string(b) + ": " + h->err; return rc; };
    // every check of every frame before anything is touched: a refused call leaves an earlier turn tour of this append readable
    int rc;
    for (int b = 0; b < n; ++b) {
        if (start_headings[b] < 0 || start_headings[b] > 7)
            return h->fail(YH_EINVAL, "frame " + std::to_string(b) + ": start heading " + std::to_string(start_headings[b]) + ": 0 .. 7 (0 right, clockwise on the image, 6 up)");
        if ((rc = scene_plan_checks(h, n_targets, starts_xy[2 * b], starts_xy[2 * b + 1]))) return framed(b, rc);
        if (hb->from_fields && !hb->fields_set[b]) return h->fail(YH_ESTATE, "frame " + std::to_string(b) + " has been given no fields since the last append");
    }
    const long long W = h->W, H = h->H;
    if ((W + H) * (2 * std::max(H, 101LL) + 1) + 8 * 1024 >= (1LL << 24))
        return h->fail(YH_EINVAL, "frame too large for the turn planner: (W + H) * (2 * max(H, 101) + 1) + 8 * 1024 must stay below 2^24");
    for (int b = 0; b < n; ++b)
        if (!hb->diag_ok[b]) return h->fail(YH_ESTATE, "frame " + std::to_string(b) + ": the uploaded fields allow 4-connected plans only: " + hb->diag_why[b]);
    SCHK(h, hipSetDevice(h->dev));
    std::vector<float> balls;
    if (!targets_xy) {   // one read-back for all frames
        balls.resize((size_t)n * 400);
        SCHK(h, hipMemcpyAsync(balls.data(), h->balls, balls.size() * 4, hipMemcpyDeviceToHost, h->stream));
        SCHK(h, hipStreamSynchronize(h->stream));
    }
    std::vector<int32_t> seeds, field, st(n, YH_OK), chosen;
    std::vector<TurnTourPoints> points(n);
    std::vector<std::vector<int32_t>> targets(n);
    for (int b = 0; b < n; ++b) {
        TurnTourPoints& pts = points[b];
        pts.K = 0; pts.start = (int32_t)(starts_xy[2 * b + 1] * W + starts_xy[2 * b]); pts.heading = start_headings[b];
        std::fill(pts.t, pts.t + YH_TOUR_MAX, -1);
        rc = scene_plan_choose(h, targets_xy ? targets_xy + (size_t)b * n_targets * 2 : nullptr, n_targets,
                               targets_xy ? nullptr : reinterpret_cast<const float(*)[4]>(balls.data() + (size_t)b * 400), chosen);
        if (rc == YH_ESTATE && !targets_xy) { st[b] = YH_ESTATE; continue; }   // no usable ball: this frame gets no tour
        if (rc) return framed(b, rc);
        std::vector<int32_t>& t = targets[b];
        for (int32_t v : chosen) {
            if (std::find(t.begin(), t.end(), v) == t.end()) { t.push_back(v); continue; }
            // (a ball on an earlier ball's pixel is dropped)
            if (targets_xy)
                return h->fail(YH_EINVAL, "frame " + std::to_string(b) + ": duplicate target (" + std::to_string(v % h->W) + ", " + std::to_string(v / h->W) + "): a tour's targets are distinct pixels");
        }
        pts.K = (int32_t)t.size();
        for (int f = 0; f < pts.K; ++f) { pts.t[f] = t[f]; seeds.push_back(t[f]); field.push_back(b * n_targets + f); }
    }
    if (seeds.empty()) return h->fail(YH_ESTATE, "no target given and no frame of the batch has a ball inside it");
    if (status) std::copy(st.begin(), st.end(), status);
    h->err.clear();
    if (!hb->turn_tour) hb->turn_tour = new yh_scene_batch_turn_tour();   // allocated at the first batched turn tour: a handle that never makes one pays nothing
    if ((rc = ensure_buffers(hb, n_targets))) { scene_batch_turn_tour_free(hb); return rc; }
    yh_scene_batch_turn_tour* q = hb->turn_tour;
    q->last.planned = false;
    q->n = n; q->kmax = n_targets; q->tau = turn_price;
    q->last_seeds = seeds; q->last_field = field; q->last_points = points; q->status = st;
    q->frames.assign(n, FrameTour());
    for (int b = 0; b < n; ++b) q->frames[b].targets = targets[b];
    if ((rc = run_turn_tour(hb))) return rc;
    q->last.conn = 8; q->last.planned = true; q->last.frame = h->frames;
    return YH_OK;
}

int yh_scene_batch_turn_tour_read(yh_scene_batch* hb, int32_t frame, int32_t* n_targets, int32_t* targets_xy, int32_t* order, float* legs, uint8_t* arrive, float* total,
                                  int32_t* leg_headings, float* cost, uint8_t* act, uint8_t* label, int32_t* path_xy, float* directions, int32_t* turns, int32_t* leg_ends,
                                  int32_t path_capacity, int32_t* path_len) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (frame < 0 || frame >= hb->max_frames || (h->ran && frame >= hb->n)) return h->fail(YH_EINVAL, "frame " + std::to_string(frame) + " outside the last append's " + std::to_string(hb->n));
    const yh_scene_batch_turn_tour* q = hb->turn_tour;
    SolveLast one = q ? q->last : SolveLast();   // this frame's part of the batch's turn tour
    const size_t npx = (size_t)h->W * h->H, states = 8 * npx;
    const FrameTour* ft = nullptr;
    size_t fo = 0;   // the frame's first field, in pixels
    if (one.planned && one.frame == h->frames) {
        if (q->status[frame] != YH_OK) return h->fail(YH_ESTATE, "frame " + std::to_string(frame) + " had no ball inside it: it has no turn tour");
        ft = &q->frames[frame];
        fo = (size_t)frame * q->kmax * npx;
        one.path_len = ft->path_len; one.nodes = q->nodes + fo; one.dirs = q->dirs + fo;
    }
    // the checks first (a turn tour of this frame exists; turns takes the route's capacity as path_xy and directions do), then the copies
    int rc = solve_read(h, "turn tour", "plan the turn tour again", &one, {}, nullptr, nullptr, 0, path_len);
    if (rc) return rc;
    if ((path_xy || directions || turns) && path_capacity < one.path_len)
        return h->fail(YH_EOVERFLOW, "path_capacity " + std::to_string(path_capacity) + " < the route's " + std::to_string(one.path_len) + " nodes");
    const int K = (int)ft->targets.size();
    const size_t nturns = one.path_len > 1 ? (size_t)(one.path_len - 1) * 4 : 0;
    rc = solve_read(h, "turn tour", "plan the turn tour again", &one,
                    { { cost, q->cost + fo * 8, K * states * 4 }, { act, q->act + fo * 8, K * states }, { label, q->label + frame * states, states },
                      { nturns ? turns : nullptr, q->turns + fo, nturns } },
                    path_xy, directions, path_capacity, path_len);
    if (rc) return rc;
    if (n_targets) *n_targets = K;
    for (int b = 0; b < K; ++b) {
        if (targets_xy) { targets_xy[2 * b] = ft->targets[b] % h->W; targets_xy[2 * b + 1] = ft->targets[b] / h->W; }
        if (order) order[b] = ft->order[b];
        if (leg_ends) leg_ends[b] = ft->leg_ends[b];
        if (leg_headings) leg_headings[b] = ft->leg_headings[b];
    }
    if (legs) memcpy(legs, ft->legs, (size_t)(1 + 8 * K) * K * 4);
    if (arrive) memcpy(arrive, ft->arrive, (size_t)(1 + 8 * K) * K);
    if (total) *total = ft->total;
    return YH_OK;
}

int yh_scene_batch_turn_tour_time(yh_scene_batch* hb, int32_t reps, float* ms_per_batch, int32_t* rounds, int32_t* tile_runs) {
    if (!hb || reps < 1 || !ms_per_batch) return YH_EINVAL;
    yh_scene_batch_turn_tour* q = hb->turn_tour;
    // (a failed replay has overwritten part of the last turn tour: it is gone; the host's choice of the orders is inside the time)
    auto run = [&] { const int rc = run_turn_tour(hb); if (rc) q->last.planned = false; return rc; };
    return solve_time(&hb->core, "turn tour", "plan the turn tour again", q ? &q->last : nullptr, reps, run, ms_per_batch, rounds, tile_runs);
}

}  // extern "C"
