// scene_turn_tour.hip — the turn-aware tour (yh_scene_plan_turn_tour; DESIGN.md §11 "Turn tour", restated in tests/turn_tour_ref.py):
// which ball first, then which, on a route a drive base can follow. Everything not said here is "Turns" (scene_turn.hip: the graph
// over (pixel, heading) states, the price tau per 45 degrees, the action rule, the walk) and "Tour" (scene_tour.hip: K <= YH_TOUR_MAX
// distinct targets, a field per target, the label, all K! orders on the host, the legs joined).
//   d_b f32 [8][H][W], act_b u8 [8][H][W]: the turn plan's cost and action field with the single target t_b.
//   label u8 [8][H][W]: the smallest b with d_b[h][v] == min_b d_b[h][v].
//   The leg table, rows r = 0 .. 8K: row 0 is the state (start, h0), row 1 + 8 a + h the state (t_a, h). legs[r][b] = d_b there,
//   arrive[r][b] = the heading with which the walk along act_b from there reaches t_b (the row's own where its pixel is t_b).
//   An order's total: from (start, h0), leg by leg tot = fl(tot + legs[row][o_j]), the next row that of (t_{o_j}, arrive[row][o_j]):
//   a leg is the turn plan's route from the state in which the leg before ended - the arrival heading is taken as it comes.
// There is one driver (run_turn_tour) and one set of kernels for yh_scene_plan_turn_tour (the batch of one) and
// yh_scene_batch_plan_turn_tour (the first n of the handle's max_frames; DESIGN.md §11 "Scene batch: turn tours"): each kernel takes its
// frame from blockIdx.z, advances its own copy of the parameter block and of its pointers to that frame and runs the body
// (scene_turn_dev.h, scene_turn_tour_dev.h). A field is unique (every weight >= 1) and has its own eight layers and tile flags, so fields
// that share rounds cannot change each other's bits; a call takes the rounds of its slowest field, not their sum.
//
// K is ragged: Kmax is one number per call (a batch's n_targets; a scene's number of distinct targets), frame b has K_b <= Kmax
// targets (fewer balls, or balls on one pixel). Field f of frame b is solver field z = b Kmax + f - NOT b K_b + f. What advances by what:
//   edge, edge2 (and map, conn0, conn1 under path_weights)    b W H          one set of edge terms per frame, shared by its fields
//   cost f32, act u8 [n][Kmax][8][H][W]                        z 8 W H
//   label u8 [n][8][H][W]                                      b 8 W H
//   seg_nodes, seg_turns, seg_dirs [n][Kmax][W H]              z W H          leg j of frame b: z = b Kmax + j
//   nodes, dirs, turns [n][Kmax W H]                           b Kmax W H     a joined route is at most K W H long
//   table i32 [n][3][kEntriesMax], walk_out i32 [n][4 YH_TOUR_MAX], points, legs [n]
//   flags [2][n Kmax][ntiles]                                  as turn_round indexes them, F = n Kmax
// Bytes per pixel: 80 per (frame, target) - cost 32, act 8, the legs' segments 20, the joined route 20 - plus 8 per frame for the
// label; allocated at the first call for max_frames x the largest Kmax so far, growing only (growing drops the last turn tour).
// 640 x 480 with max_frames = 64 and Kmax = 6 is 9.6 GB: a caller sizes max_frames and n_targets accordingly.
// A field f >= K_b has no seed: it flags nothing and its tiles exit at once (the solver's ragged field_of form); the act, arrive,
// walk and join kernels skip it.
//
// Launches of one call, their number independent of n: ONE copy of the inputs from the state's pinned block (the seeds as (pixel,
// field z) pairs, then the points [n]), path_weights<8> (scene_solve.hip) over the n frames, one fill of 8 n Kmax W H values with +inf,
// tt_seeds (0 in the eight layers of the seed's field), then
//   turn_round (scene_turn.hip's, through scene_turn_round) x rounds, grid (tiles x, tiles y, n Kmax), through scene_solve.hip's host
//              loop (SolveRound{.., 8}, ragged seeds): turn_round_body on field z with field z's flags.
//   tt_act     one lane per pixel (pixels x 1 x n), its edge terms read once for all 8 K states: act_b (255 at t_b) and the label.
//   tt_arrive  one wave per (entry of the leg table, frame): the cost there and, where the row's pixel is not t_b - the K + 8 K (K - 1)
//              entries an order can reach -, a chase along act_b (turn_chase<false>: no node is stored) for the arrival heading.
//   (host)     ONE copy of the tables (3 words per entry) and ONE wait; the order of every frame: all K! <= 720 permutations
//              (best_order). It fixes every leg's start state. One upload of the legs [n], from the same pinned block.
//   tt_walk    Kmax x 1 x n waves, one per leg: turn_walk_body on field o_j from (t_{o_{j-1}}, the heading leg j - 1 arrived with) into
//              the leg's own segment: its nodes, the turns before each drive (the first one counted from the carried heading) and directions.
//   tt_join    (blocks x 1 x n) the segments into one route (a junction node once), turns and directions per step, and leg_ends.
//   ONE copy of n x 4 YH_TOUR_MAX words and ONE wait.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
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
struct FrameTour {   // what the host keeps of frame b's turn tour
    std::vector<int32_t> targets;   // linear indices, t_0 .. t_{K-1}; empty: no tour for this frame
    int32_t order[YH_TOUR_MAX], leg_ends[YH_TOUR_MAX], leg_headings[YH_TOUR_MAX];
    float legs[kEntriesMax], total = 0.0f;
    uint8_t arrive[kEntriesMax];
};
constexpr size_t kPointsWords = sizeof(TurnTourPoints) / 4, kLegsWords = sizeof(TurnTourLegs) / 4;
}  // namespace

struct yh_scene_turn_tour : PlanFrames {   // nodes, dirs [max][K*W*H] the joined routes; walk_out [max][4 * YH_TOUR_MAX]
    int cap_k = 0;                   // the field buffers are sized for max_frames x this many fields; they only grow
    float* cost = nullptr;           // [max][K][8][H][W]
    uint8_t* act = nullptr;          // [max][K][8][H][W]
    uint8_t* label = nullptr;        // [max][8][H][W]
    int2* seg_nodes = nullptr;       // [max][K][W*H] the legs' walks
    int32_t* seg_turns = nullptr;
    float2* seg_dirs = nullptr;
    int32_t* turns = nullptr;        // [max][K*W*H]: before the drive from node i of the joined route
    int32_t* table = nullptr;        // [max][3][kEntriesMax]: cost bits, arrival heading, lost flag of entry r * K + b
    int32_t* host = nullptr;         // pinned: the tables [max][3][kEntriesMax], then walk_out [max][4 * YH_TOUR_MAX], as read back
    // the last call (the replay runs exactly this); in: the seeds, then points [n], then legs [n]
    int kmax = 0;
    float tau = 1.0f;
    std::vector<TurnTourPoints> last_points;   // K = 0: no tour for that frame
    std::vector<FrameTour> frames;
};

namespace {

// seeds [ns][2] (pixel, field z): cost = 0 in all eight layers of that field there
__global__ __launch_bounds__(256) void tt_seeds(const PathParams p, const int32_t* seeds, int ns) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= 8 * ns) return;
    p.cost[((size_t)seeds[2 * (k >> 3) + 1] * 8 + (k & 7)) * p.W * p.H + seeds[2 * (k >> 3)]] = 0.0f;
}

__global__ __launch_bounds__(256) void tt_act(const PathParams p, const TurnTourPoints* __restrict__ points, int kmax, float tau, uint8_t* act, uint8_t* label) {
    const int b = blockIdx.z;
    const TurnTourPoints& pts = points[b];   // (read where it lies: a copy indexed by a variable would live in scratch)
    if (pts.K < 1) return;   // (workgroup-uniform: no tour for this frame)
    const size_t npx = (size_t)p.W * p.H;
    turn_tour_act_body(frame_of(p, b, kmax * 8 * npx), pts, tau, act + (size_t)b * kmax * 8 * npx, label + (size_t)b * 8 * npx);
}

__global__ __launch_bounds__(64) void tt_arrive(const PathParams p, const TurnTourPoints* __restrict__ points, int kmax, const uint8_t* act, int32_t* table) {
    const int b = blockIdx.z;
    const TurnTourPoints& pts = points[b];   // (read where it lies: a copy indexed by a variable would live in scratch)
    if ((int)blockIdx.x >= (1 + 8 * pts.K) * pts.K) return;   // (workgroup-uniform: this frame's table ends before this entry)
    const size_t fields = (size_t)kmax * 8 * p.W * p.H;
    turn_tour_arrive_body(frame_of(p, b, fields), pts, act + b * fields, table + (size_t)b * 3 * kEntriesMax);
}

__global__ __launch_bounds__(64) void tt_walk(const PathParams p, const TurnTourLegs* __restrict__ legs, int kmax, const uint8_t* act, int2* seg_nodes, int32_t* seg_turns, float2* seg_dirs,
                                              int32_t* out) {
    const int b = blockIdx.z;
    const TurnTourLegs& lg = legs[b];
    if ((int)blockIdx.x >= lg.K) return;   // (workgroup-uniform)
    const size_t npx = (size_t)p.W * p.H, fo = (size_t)b * kmax * npx;
    SP_BODY_ON_CACHE_LINE();
    turn_tour_walk_body(frame_of(p, b, kmax * 8 * npx), lg, act + fo * 8, seg_nodes + fo, seg_turns + fo, seg_dirs + fo, out + b * 4 * YH_TOUR_MAX);
}

__global__ __launch_bounds__(256) void tt_join(const PathParams p, const TurnTourLegs* __restrict__ legs, int kmax, const int2* seg_nodes, const int32_t* seg_turns, const float2* seg_dirs,
                                               int32_t* out, int2* nodes, int32_t* turns, float2* dirs) {
    const int b = blockIdx.z, K = legs[b].K;
    if (K < 1) return;   // (workgroup-uniform)
    const size_t fo = (size_t)b * kmax * p.W * p.H;
    turn_tour_join_body(p, K, seg_nodes + fo, seg_turns + fo, seg_dirs + fo, out + b * 4 * YH_TOUR_MAX, nodes + fo, turns + fo, dirs + fo);
}

void free_fields(yh_scene_turn_tour* q) {
    void* bufs[] = { q->cost, q->act, q->seg_nodes, q->seg_turns, q->seg_dirs, q->nodes, q->dirs, q->turns };
    for (void* b : bufs) if (b) (void)hipFree(b);
    q->cost = nullptr; q->act = nullptr; q->seg_nodes = nullptr; q->seg_turns = nullptr; q->seg_dirs = nullptr; q->nodes = nullptr; q->dirs = nullptr; q->turns = nullptr;
    q->cap_k = 0;
}

// the state at the first turn tour (a handle that never makes one pays nothing), with the buffers that do not depend on Kmax; those
// that do whenever Kmax exceeds what they were sized for
int ensure_turn_tour(yh_scene* h, int kmax) {
    if (!h->turn_tour) h->turn_tour = new yh_scene_turn_tour();
    yh_scene_turn_tour* q = h->turn_tour;
    const size_t mf = (size_t)h->max_frames, npx = (size_t)h->W * h->H;
    if (!q->label) SCHK(h, hipMalloc((void**)&q->label, mf * 8 * npx));
    if (!q->table) SCHK(h, hipMalloc((void**)&q->table, mf * 3 * kEntriesMax * 4));
    if (!q->walk_out) SCHK(h, hipMalloc((void**)&q->walk_out, mf * 4 * YH_TOUR_MAX * 4));
    if (!q->host) SCHK(h, hipHostMalloc((void**)&q->host, mf * (3 * kEntriesMax + 4 * YH_TOUR_MAX) * 4, hipHostMallocDefault));
    const int rc = plan_inputs_reserve(h, q->in, mf * (2 * YH_TOUR_MAX + kPointsWords + kLegsWords));
    if (rc) return rc;
    if (kmax <= q->cap_k) return YH_OK;
    SCHK(h, hipStreamSynchronize(h->stream));
    free_fields(q);
    q->last.planned = false;   // (the last turn tour lived in them)
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

// the whole turn tour of q->n frames on the handle's stream: last_seeds / last_field (pixel and field z of every target), last_points,
// kmax, tau. Returns when every route's length is known.
int run_turn_tour(yh_scene* h) {
    yh_scene_turn_tour* q = h->turn_tour;
    const int n = q->n, kmax = q->kmax, ns = (int)q->last_seeds.size(), F = n * kmax;
    const size_t npx = (size_t)h->W * h->H;
    const float tau = q->tau;
    const size_t ws = plan_inputs_seeds(*q), wl = ws + n * kPointsWords;   // where the points and the legs lie
    memcpy(q->in.host + ws, q->last_points.data(), (size_t)n * sizeof(TurnTourPoints));
    SCHK(h, hipMemcpyAsync(q->in.dev, q->in.host, wl * 4, hipMemcpyHostToDevice, h->stream));
    const int32_t* seeds = q->in.dev;
    const TurnTourPoints* points = reinterpret_cast<const TurnTourPoints*>(q->in.dev + ws);
    const TurnTourLegs* legs = reinterpret_cast<const TurnTourLegs*>(q->in.dev + wl);
    PathParams p;
    int rc = solve_begin(h, 8, h->max_frames * q->cap_k, n, p);
    if (rc) return rc;
    p.cost = q->cost;
    SCHK(h, hipMemsetD32Async((hipDeviceptr_t)q->cost, 0x7f800000, (size_t)F * 8 * npx, h->stream));   // +inf
    hipLaunchKernelGGL(tt_seeds, dim3((unsigned)((8 * (size_t)ns + 255) / 256)), dim3(256), 0, h->stream, p, seeds, ns);
    const SolveRound round = scene_turn_round(h, p, tau, kmax, F);
    if ((rc = solve_rounds(h, p, 8, F, q->last_seeds, h->batch ? "batch turn tour" : "turn tour", 0, nullptr, &round, &q->last_field))) return rc;
    hipLaunchKernelGGL(tt_act, dim3((unsigned)((npx + 255) / 256), 1, (unsigned)n), dim3(256), 0, h->stream, p, points, kmax, tau, q->act, q->label);
    hipLaunchKernelGGL(tt_arrive, dim3((unsigned)((1 + 8 * kmax) * kmax), 1, (unsigned)n), dim3(64), 0, h->stream, p, points, kmax, q->act, q->table);
    SCHK(h, hipGetLastError());
    SCHK(h, hipMemcpyAsync(q->host, q->table, (size_t)n * 3 * kEntriesMax * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    // per frame: the tables, the order, and with it every leg's field and start state: the walks are independent
    TurnTourLegs* host_legs = reinterpret_cast<TurnTourLegs*>(q->in.host + wl);
    for (int b = 0; b < n; ++b) {
        FrameTour& ft = q->frames[b];
        const TurnTourPoints& pts = q->last_points[b];
        const int K = pts.K;
        TurnTourLegs& lg = host_legs[b];
        lg = TurnTourLegs();
        if (K < 1) continue;
        const int32_t* tab = q->host + (size_t)b * 3 * kEntriesMax;
        for (int e = 0; e < (1 + 8 * K) * K; ++e) {
            if (tab[2 * kEntriesMax + e])
                return h->fail(YH_EHIP, h->frame_tag(b) + "turn tour: the walk of leg table entry (" + std::to_string(e / K) + ", " + std::to_string(e % K) +
                                            ") met no target within 8*W*H actions (fields not those of a SANE frame?)");
            memcpy(&ft.legs[e], &tab[e], 4);
            ft.arrive[e] = (uint8_t)tab[kEntriesMax + e];
        }
        int32_t row[YH_TOUR_MAX];
        ft.total = best_order(ft.legs, ft.arrive, K, ft.order, row);
        lg.K = K;
        for (int j = 0; j < YH_TOUR_MAX; ++j) {
            lg.field[j] = j < K ? ft.order[j] : 0;
            lg.from[j] = j == 0 ? pts.start : j < K ? pts.t[ft.order[j - 1]] : 0;
            lg.heading[j] = j == 0 ? pts.heading : j < K ? ft.leg_headings[j - 1] : 0;
            if (j < K) ft.leg_headings[j] = ft.arrive[row[j] * K + ft.order[j]];
        }
    }
    SCHK(h, hipMemcpyAsync(q->in.dev + wl, host_legs, (size_t)n * sizeof(TurnTourLegs), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(tt_walk, dim3((unsigned)kmax, 1, (unsigned)n), dim3(64), 0, h->stream, p, legs, kmax, q->act, q->seg_nodes, q->seg_turns, q->seg_dirs, q->walk_out);
    hipLaunchKernelGGL(tt_join, dim3(TT_JOIN_BLOCKS, 1, (unsigned)n), dim3(256), 0, h->stream, p, legs, kmax, q->seg_nodes, q->seg_turns, q->seg_dirs, q->walk_out, q->nodes,
                       q->turns, q->dirs);
    SCHK(h, hipGetLastError());
    int32_t* wo = q->host + (size_t)h->max_frames * 3 * kEntriesMax;
    SCHK(h, hipMemcpyAsync(wo, q->walk_out, (size_t)n * 4 * YH_TOUR_MAX * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    q->path_len.assign(n, 0);
    for (int b = 0; b < n; ++b) {
        FrameTour& ft = q->frames[b];
        const int K = q->last_points[b].K;
        const int32_t* w = wo + (size_t)b * 4 * YH_TOUR_MAX;
        for (int j = 0; j < K; ++j) {
            if (w[2 * j + 1])
                return h->fail(YH_EHIP, h->frame_tag(b) + "turn tour walk: leg " + std::to_string(j) + " met no target within 8*W*H actions (fields not those of a SANE frame?)");
            ft.leg_ends[j] = w[2 * YH_TOUR_MAX + j];
        }
        if (K > 0) q->path_len[b] = w[3 * YH_TOUR_MAX];
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

// frame b of a call's inputs: its points, its seeds (field z = b kmax + f) and what the host keeps of its targets
void frame_inputs(yh_scene_turn_tour* q, int b, int kmax, const std::vector<int32_t>& targets, int32_t start, int32_t heading) {
    TurnTourPoints& pts = q->last_points[b];
    pts.K = (int32_t)targets.size(); pts.start = start; pts.heading = heading;
    for (int f = 0; f < YH_TOUR_MAX; ++f) pts.t[f] = f < pts.K ? targets[f] : -1;
    for (int f = 0; f < pts.K; ++f) { q->last_seeds.push_back(targets[f]); q->last_field.push_back(b * kmax + f); }
    q->frames[b].targets = targets;
}

// ensures the state for n frames of kmax fields and clears the inputs of the last call (which is gone from here on)
int begin_inputs(yh_scene* h, int n, int kmax, float tau) {
    const int rc = ensure_turn_tour(h, kmax);
    if (rc) { scene_turn_tour_free(h); return rc; }
    yh_scene_turn_tour* q = h->turn_tour;
    q->last.planned = false;
    q->n = n; q->kmax = kmax; q->tau = tau;
    q->last_seeds.clear(); q->last_field.clear();
    q->last_points.assign(n, TurnTourPoints()); q->frames.assign(n, FrameTour());
    return YH_OK;
}

// the inputs of a call are in h->turn_tour: run it, and it is the handle's last turn tour
int turn_tour_now(yh_scene* h) {
    yh_scene_turn_tour* q = h->turn_tour;
    const int rc = run_turn_tour(h);
    if (rc) return rc;
    q->last.conn = 8; q->last.planned = true; q->last.frame = h->frames;
    return YH_OK;
}

int turn_tour_read(yh_scene* h, int frame, int32_t* n_targets, int32_t* targets_xy, int32_t* order, float* legs, uint8_t* arrive, float* total, int32_t* leg_headings,
                   float* cost, uint8_t* act, uint8_t* label, int32_t* path_xy, float* directions, int32_t* turns, int32_t* leg_ends, int32_t path_capacity,
                   int32_t* path_len) {
    const yh_scene_turn_tour* q = h->turn_tour;
    const size_t npx = (size_t)h->W * h->H, states = 8 * npx;
    const size_t fo = q ? (size_t)frame * q->kmax * npx : 0;   // the frame's first field, in pixels
    SolveLast one;
    int rc = solve_frame(h, q, frame, q ? q->kmax * npx : 0, "turn tour", one);
    if (rc) return rc;
    const FrameTour* ft = one.planned && one.frame == h->frames ? &q->frames[frame] : nullptr;
    const int K = ft ? (int)ft->targets.size() : 0;
    // (turns takes the route's capacity as path_xy and directions do)
    const size_t nturns = one.path_len > 1 ? (size_t)(one.path_len - 1) * 4 : 0;
    rc = solve_read(h, "turn tour", "plan the turn tour again", &one,
                    { { cost, q ? q->cost + fo * 8 : nullptr, K * states * 4 }, { act, q ? q->act + fo * 8 : nullptr, K * states },
                      { label, q ? q->label + frame * states : nullptr, states }, { nturns ? turns : nullptr, q ? q->turns + fo : nullptr, nturns } },
                    path_xy, directions, path_capacity, path_len, turns != nullptr);
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

int turn_tour_time(yh_scene* h, int32_t reps, float* ms, int32_t* rounds, int32_t* tile_runs) {
    yh_scene_turn_tour* q = h->turn_tour;
    // (a failed replay has overwritten part of the last turn tour: it is gone; the host's choice of the orders is inside the time)
    auto run = [&] { const int rc = run_turn_tour(h); if (rc) q->last.planned = false; return rc; };
    return solve_time(h, "turn tour", "plan the turn tour again", q ? &q->last : nullptr, reps, run, ms, rounds, tile_runs);
}

}  // namespace

namespace yh {
void scene_turn_tour_free(yh_scene* h) {
    yh_scene_turn_tour* q = h->turn_tour;
    if (!q) return;
    free_fields(q);
    void* bufs[] = { q->label, q->table, q->walk_out };
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (q->host) (void)hipHostFree(q->host);
    plan_inputs_free(q->in);
    delete q;
    h->turn_tour = nullptr;
}
}  // namespace yh

extern "C" {

int yh_scene_plan_turn_tour(yh_scene* h, const int32_t* targets_xy, int32_t n_targets, int32_t start_x, int32_t start_y, int32_t start_heading, float turn_price) {
    if (!h) return YH_EINVAL;
    int rc;
    if ((rc = scene_turn_heading(h, start_heading)) || (rc = scene_turn_price(h, turn_price))) return rc;
    if (n_targets > YH_TOUR_MAX) return h->fail(YH_EINVAL, "n_targets " + std::to_string(n_targets) + " > YH_TOUR_MAX = " + std::to_string(YH_TOUR_MAX));
    std::vector<int32_t> chosen, targets;
    if ((rc = scene_plan_targets(h, targets_xy, n_targets, start_x, start_y, chosen))) return rc;
    if ((rc = distinct_targets(h, chosen, targets_xy != nullptr, targets))) return rc;
    if ((rc = scene_turn_size(h)) || (rc = scene_plan_diagonals(h, h->diag_ok, h->diag_why))) return rc;
    // the batch of one: Kmax is the number of distinct targets
    const int K = (int)targets.size();
    if ((rc = begin_inputs(h, 1, K, turn_price))) return rc;
    frame_inputs(h->turn_tour, 0, K, targets, start_y * h->W + start_x, start_heading);
    h->turn_tour->status.assign(1, YH_OK);
    return turn_tour_now(h);
}

int yh_scene_batch_plan_turn_tour(yh_scene_batch* hb, const int32_t* targets_xy, int32_t n_targets, const int32_t* starts_xy, const int32_t* start_headings,
                                  float turn_price, int32_t* status) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (!starts_xy) return h->fail(YH_EINVAL, "starts_xy is null");
    if (!start_headings) return h->fail(YH_EINVAL, "start_headings is null");
    int rc = scene_turn_price(h, turn_price);
    if (rc) return rc;
    if (n_targets > YH_TOUR_MAX) return h->fail(YH_EINVAL, "n_targets " + std::to_string(n_targets) + " > YH_TOUR_MAX = " + std::to_string(YH_TOUR_MAX));
    std::vector<int32_t> st;
    std::vector<std::vector<int32_t>> targets(hb->n);
    bool any = false;
    rc = scene_batch_frames(hb, targets_xy, n_targets, starts_xy, start_headings, 8, st, [&](int b, const std::vector<int32_t>& chosen) {
        any = true;
        return distinct_targets(h, chosen, targets_xy != nullptr, targets[b]);
    });
    if (rc) return rc;
    if (!any) return h->fail(YH_ESTATE, "no target given and no frame of the batch has a ball inside it");
    if (status) std::copy(st.begin(), st.end(), status);
    h->err.clear();
    if ((rc = begin_inputs(h, hb->n, n_targets, turn_price))) return rc;
    for (int b = 0; b < hb->n; ++b) frame_inputs(h->turn_tour, b, n_targets, targets[b], starts_xy[2 * b + 1] * h->W + starts_xy[2 * b], start_headings[b]);
    h->turn_tour->status = st;
    return turn_tour_now(h);
}

int yh_scene_turn_tour_read(yh_scene* h, int32_t* n_targets, int32_t* targets_xy, int32_t* order, float* legs, uint8_t* arrive, float* total, int32_t* leg_headings,
                            float* cost, uint8_t* act, uint8_t* label, int32_t* path_xy, float* directions, int32_t* turns, int32_t* leg_ends,
                            int32_t path_capacity, int32_t* path_len) {
    if (!h) return YH_EINVAL;
    return turn_tour_read(h, 0, n_targets, targets_xy, order, legs, arrive, total, leg_headings, cost, act, label, path_xy, directions, turns, leg_ends, path_capacity, path_len);
}

int yh_scene_batch_turn_tour_read(yh_scene_batch* hb, int32_t frame, int32_t* n_targets, int32_t* targets_xy, int32_t* order, float* legs, uint8_t* arrive, float* total,
                                  int32_t* leg_headings, float* cost, uint8_t* act, uint8_t* label, int32_t* path_xy, float* directions, int32_t* turns, int32_t* leg_ends,
                                  int32_t path_capacity, int32_t* path_len) {
    if (!hb) return YH_EINVAL;
    const int rc = hb->frame_ok(frame);
    if (rc) return rc;
    return turn_tour_read(&hb->core, frame, n_targets, targets_xy, order, legs, arrive, total, leg_headings, cost, act, label, path_xy, directions, turns, leg_ends, path_capacity,
                          path_len);
}

int yh_scene_turn_tour_time(yh_scene* h, int32_t reps, float* ms_per_tour, int32_t* rounds, int32_t* tile_runs) {
    if (!h || reps < 1 || !ms_per_tour) return YH_EINVAL;
    return turn_tour_time(h, reps, ms_per_tour, rounds, tile_runs);
}

int yh_scene_batch_turn_tour_time(yh_scene_batch* hb, int32_t reps, float* ms_per_batch, int32_t* rounds, int32_t* tile_runs) {
    if (!hb || reps < 1 || !ms_per_batch) return YH_EINVAL;
    return turn_tour_time(&hb->core, reps, ms_per_batch, rounds, tile_runs);
}

}  // extern "C"
