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
// The K fields relax in the SAME launches, the field as grid z (a tour's rounds are those of its slowest field); map and edge terms
// are shared by all of them, so only cost advances with the field - not, as in scene_batch_turn.hip's turn_frame_of, the edges too.
//
// Launches of one turn tour (the solver and its buffers are scene_solve.hip's, the bodies scene_turn_dev.h's and - shared with the
// scene batch, scene_batch_turn_tour.hip - scene_turn_tour_dev.h's):
//   path_weights<8> (scene_solve.hip) once, tt_fill (+inf over [K][8][H][W]), tt_targets (0 at t_b in field b's eight layers), then
//   tt_round   x rounds, grid (tiles x, tiles y, K), through scene_solve.hip's host loop: turn_round_body on field z with field z's flags.
//   tt_act     one lane per pixel, its edge terms read once for all 8 K states: act_b (255 at t_b) and the label.
//   tt_arrive  one wave per entry of the leg table: the cost there and, where the row's pixel is not t_b - the K + 8 K (K - 1) entries
//              an order can reach -, a chase along act_b (turn_chase<false>: no node is stored) for the arrival heading.
//   (host)     one copy of the table (3 words per entry); the order: all K! <= 720 permutations. It fixes every leg's start state.
//   tt_walk    K waves, one per leg: turn_walk_body on field o_j from (t_{o_{j-1}}, the heading leg j - 1 arrived with) into the leg's
//              own segment: its nodes, the turns before each drive (the first one counted from the carried heading) and directions.
//   tt_join    the segments into one route (a junction node once), turns and directions per step, and leg_ends.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "scene.h"
#include "scene_path_dev.h"
#include "scene_turn_dev.h"
#include "scene_turn_tour_dev.h"
#include "yh_internal.h"

using namespace yh;

struct yh_scene_turn_tour : SolveLast {   // (the joined route [K * W * H], the start and whether a turn tour exists: SolveLast)
    int cap_k = 0;               // the buffers below are sized for this many fields; they only grow
    float* cost = nullptr;       // [K][8][H][W]
    uint8_t* act = nullptr;      // [K][8][H][W]
    uint8_t* label = nullptr;    // [8][H][W]
    int32_t* turns = nullptr;    // [K * W * H]: before the drive from node i of the joined route
    int2* seg_nodes = nullptr;   // [K][W * H] the legs' walks
    int32_t* seg_turns = nullptr;
    float2* seg_dirs = nullptr;
    int32_t* table = nullptr;    // [3][kEntriesMax]: cost bits, arrival heading, lost flag of entry r * K + b
    int32_t* walk_out = nullptr; // [4 * YH_TOUR_MAX]: (nodes, status) of leg j, then leg_ends, then the route's nodes
    int32_t* host = nullptr;     // pinned: the table, then walk_out, as read back
    std::vector<int32_t> targets;   // of the last turn tour: linear indices, t_0 .. t_{K-1}
    int32_t heading = 6;
    float tau = 1.0f;
    int32_t order[YH_TOUR_MAX], leg_ends[YH_TOUR_MAX], leg_headings[YH_TOUR_MAX];
    float legs[kEntriesMax], total = 0.0f;
    uint8_t arrive[kEntriesMax];
};

namespace {

__global__ __launch_bounds__(256) void tt_fill(const PathParams p) { turn_fill_body(turn_field_of(p, blockIdx.z)); }

__global__ __launch_bounds__(64) void tt_targets(const PathParams p, const TurnTourPoints pts) {
    const int k = threadIdx.x;
    if (k >= 8 * pts.K) return;
    p.cost[(size_t)k * p.W * p.H + pts.t[k >> 3]] = 0.0f;   // (layer k & 7 of field k >> 3)
}

__global__ __launch_bounds__(SP_NT) void tt_round(const PathParams p, float tau, int F, int parity, uint32_t* cnt_next) {
    const int b = blockIdx.z;
    turn_round_body(turn_field_of(p, b), tau, p.flags + (size_t)(parity * F + b) * p.ntiles, p.flags + (size_t)((parity ^ 1) * F + b) * p.ntiles, cnt_next);
}

// the bodies of the four kernels below: scene_turn_tour_dev.h (the scene batch runs them on the frame of blockIdx.z)
__global__ __launch_bounds__(256) void tt_act(const PathParams p, const TurnTourPoints pts, float tau, uint8_t* act, uint8_t* label) {
    turn_tour_act_body(p, pts, tau, act, label);
}

__global__ __launch_bounds__(64) void tt_arrive(const PathParams p, const TurnTourPoints pts, const uint8_t* act, int32_t* table) {
    turn_tour_arrive_body(p, pts, act, table);
}

__global__ __launch_bounds__(64) void tt_walk(const PathParams p, const TurnTourLegs legs, const uint8_t* act, int2* seg_nodes, int32_t* seg_turns, float2* seg_dirs, int32_t* out) {
    turn_tour_walk_body(p, legs, act, seg_nodes, seg_turns, seg_dirs, out);
}

__global__ __launch_bounds__(256) void tt_join(const PathParams p, int K, const int2* seg_nodes, const int32_t* seg_turns, const float2* seg_dirs, int32_t* out,
                                               int2* nodes, int32_t* turns, float2* dirs) {
    turn_tour_join_body(p, K, seg_nodes, seg_turns, seg_dirs, out, nodes, turns, dirs);
}

void free_fields(yh_scene_turn_tour* q) {
    void* bufs[] = { q->cost, q->act, q->turns, q->seg_nodes, q->seg_turns, q->seg_dirs, q->nodes, q->dirs };
    for (void* b : bufs) if (b) (void)hipFree(b);
    q->cost = nullptr; q->act = nullptr; q->turns = nullptr; q->seg_nodes = nullptr; q->seg_turns = nullptr; q->seg_dirs = nullptr; q->nodes = nullptr; q->dirs = nullptr;
    q->cap_k = 0;
}

// the buffers that do not depend on K at the first turn tour; those that do whenever K exceeds what they were sized for
int ensure_buffers(yh_scene* h, int K) {
    yh_scene_turn_tour* q = h->turn_tour;
    const size_t npx = (size_t)h->W * h->H;
    if (!q->label) SCHK(h, hipMalloc((void**)&q->label, 8 * npx));
    if (!q->table) SCHK(h, hipMalloc((void**)&q->table, 3 * kEntriesMax * 4));
    if (!q->walk_out) SCHK(h, hipMalloc((void**)&q->walk_out, 4 * YH_TOUR_MAX * 4));
    if (!q->host) SCHK(h, hipHostMalloc((void**)&q->host, (3 * kEntriesMax + 4 * YH_TOUR_MAX) * 4, hipHostMallocDefault));
    if (K <= q->cap_k) return YH_OK;
    SCHK(h, hipStreamSynchronize(h->stream));
    free_fields(q);
    q->planned = false;   // (the last turn tour lived in them)
    SCHK(h, hipMalloc((void**)&q->cost, K * 8 * npx * 4));
    SCHK(h, hipMalloc((void**)&q->act, K * 8 * npx));
    SCHK(h, hipMalloc((void**)&q->turns, K * npx * 4));
    SCHK(h, hipMalloc((void**)&q->seg_nodes, K * npx * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&q->seg_turns, K * npx * 4));
    SCHK(h, hipMalloc((void**)&q->seg_dirs, K * npx * sizeof(float2)));
    SCHK(h, hipMalloc((void**)&q->nodes, K * npx * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&q->dirs, K * npx * sizeof(float2)));
    q->cap_k = K;
    return YH_OK;
}

// the whole turn tour on the handle's stream; returns when the route's length is known
int run_turn_tour(yh_scene* h, const std::vector<int32_t>& targets, int32_t start, int32_t heading, float tau) {
    yh_scene_turn_tour* q = h->turn_tour;
    const int K = (int)targets.size(), rows = 1 + 8 * K;
    const size_t npx = (size_t)h->W * h->H;
    TurnTourPoints pts;
    pts.K = K; pts.start = start; pts.heading = heading;
    for (int b = 0; b < YH_TOUR_MAX; ++b) pts.t[b] = b < K ? targets[b] : -1;
    PathParams p;
    int rc = solve_begin(h, 8, K, p);
    if (rc) return rc;
    p.cost = q->cost; p.next = nullptr;
    const dim3 px((unsigned)((npx + 255) / 256)), st((unsigned)((8 * npx + 255) / 256), 1, (unsigned)K);
    hipLaunchKernelGGL(tt_fill, st, dim3(256), 0, h->stream, p);
    hipLaunchKernelGGL(tt_targets, dim3(1), dim3(64), 0, h->stream, p, pts);
    const SolveRound round = { [&](const dim3& tiles, int parity, uint32_t* cnt_next) {
        hipLaunchKernelGGL(tt_round, tiles, dim3(SP_NT), 0, h->stream, p, tau, K, parity, cnt_next);
    }, 8 };
    std::vector<int32_t> field_of(K);
    for (int b = 0; b < K; ++b) field_of[b] = b;   // one seed per field
    if ((rc = solve_rounds(h, p, 8, K, targets, "turn tour", 0, nullptr, &round, &field_of))) return rc;
    hipLaunchKernelGGL(tt_act, px, dim3(256), 0, h->stream, p, pts, tau, q->act, q->label);
    hipLaunchKernelGGL(tt_arrive, dim3((unsigned)(rows * K)), dim3(64), 0, h->stream, p, pts, q->act, q->table);
    SCHK(h, hipGetLastError());
    SCHK(h, hipMemcpyAsync(q->host, q->table, 3 * kEntriesMax * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    for (int e = 0; e < rows * K; ++e) {
        if (q->host[2 * kEntriesMax + e])
            return h->fail(YH_EHIP, "turn tour: the walk of leg table entry (" + std::to_string(e / K) + ", " + std::to_string(e % K) + ") met no target within 8*W*H actions (fields not those of a SANE frame?)");
        memcpy(&q->legs[e], &q->host[e], 4);
        q->arrive[e] = (uint8_t)q->host[kEntriesMax + e];
    }
    // the order, and with it every leg's field and start state: the K walks are independent
    int32_t row[YH_TOUR_MAX];
    q->total = best_order(q->legs, q->arrive, K, q->order, row);
    TurnTourLegs lg;
    lg.K = K;
    for (int j = 0; j < YH_TOUR_MAX; ++j) {
        lg.field[j] = j < K ? q->order[j] : 0;
        lg.from[j] = j == 0 ? start : j < K ? targets[q->order[j - 1]] : 0;
        lg.heading[j] = j == 0 ? heading : j < K ? q->leg_headings[j - 1] : 0;
        if (j < K) q->leg_headings[j] = q->arrive[row[j] * K + q->order[j]];
    }
    hipLaunchKernelGGL(tt_walk, dim3((unsigned)K), dim3(64), 0, h->stream, p, lg, q->act, q->seg_nodes, q->seg_turns, q->seg_dirs, q->walk_out);
    hipLaunchKernelGGL(tt_join, dim3(TT_JOIN_BLOCKS), dim3(256), 0, h->stream, p, K, q->seg_nodes, q->seg_turns, q->seg_dirs, q->walk_out, q->nodes, q->turns, q->dirs);
    SCHK(h, hipGetLastError());
    int32_t* wo = q->host + 3 * kEntriesMax;
    SCHK(h, hipMemcpyAsync(wo, q->walk_out, 4 * YH_TOUR_MAX * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    for (int j = 0; j < K; ++j) {
        if (wo[2 * j + 1]) return h->fail(YH_EHIP, "turn tour walk: leg " + std::to_string(j) + " met no target within 8*W*H actions (fields not those of a SANE frame?)");
        q->leg_ends[j] = wo[2 * YH_TOUR_MAX + j];
    }
    q->path_len = wo[3 * YH_TOUR_MAX];
    return YH_OK;
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
    delete q;
    h->turn_tour = nullptr;
}
}  // namespace yh

extern "C" {

int yh_scene_plan_turn_tour(yh_scene* h, const int32_t* targets_xy, int32_t n_targets, int32_t start_x, int32_t start_y, int32_t start_heading, float turn_price) {
    if (!h) return YH_EINVAL;
    if (start_heading < 0 || start_heading > 7) return h->fail(YH_EINVAL, "start heading " + std::to_string(start_heading) + ": 0 .. 7 (0 right, clockwise on the image, 6 up)");
    if (!std::isfinite(turn_price) || turn_price < 1.0f || turn_price > 1024.0f)
        return h->fail(YH_EINVAL, "turn price must be a finite number in [1, 1024] (every weight >= 1 is what makes the field unique)");
    if (n_targets > YH_TOUR_MAX) return h->fail(YH_EINVAL, "n_targets " + std::to_string(n_targets) + " > YH_TOUR_MAX = " + std::to_string(YH_TOUR_MAX));
    std::vector<int32_t> chosen, targets;
    int rc = scene_plan_targets(h, targets_xy, n_targets, start_x, start_y, chosen);
    if (rc) return rc;
    for (int32_t t : chosen) {
        if (std::find(targets.begin(), targets.end(), t) == targets.end()) { targets.push_back(t); continue; }
        // (a ball on an earlier ball's pixel is dropped)
        if (targets_xy) return h->fail(YH_EINVAL, "duplicate target (" + std::to_string(t % h->W) + ", " + std::to_string(t / h->W) + "): a tour's targets are distinct pixels");
    }
    const long long W = h->W, H = h->H;
    if ((W + H) * (2 * std::max(H, 101LL) + 1) + 8 * 1024 >= (1LL << 24))
        return h->fail(YH_EINVAL, "frame too large for the turn planner: (W + H) * (2 * max(H, 101) + 1) + 8 * 1024 must stay below 2^24");
    if ((rc = scene_plan_diagonals(h))) return rc;
    if (!h->turn_tour) h->turn_tour = new yh_scene_turn_tour();   // allocated at the first turn tour: a handle that never makes one pays nothing
    rc = ensure_buffers(h, (int)targets.size());
    if (rc) { scene_turn_tour_free(h); return rc; }
    yh_scene_turn_tour* q = h->turn_tour;
    q->planned = false;
    const int32_t start = (int32_t)(start_y * W + start_x);
    rc = run_turn_tour(h, targets, start, start_heading, turn_price);
    if (rc) return rc;
    q->conn = 8;
    q->planned = true; q->frame = h->frames; q->targets = targets; q->start = start; q->heading = start_heading; q->tau = turn_price;
    return YH_OK;
}

int yh_scene_turn_tour_read(yh_scene* h, int32_t* n_targets, int32_t* targets_xy, int32_t* order, float* legs, uint8_t* arrive, float* total, int32_t* leg_headings,
                            float* cost, uint8_t* act, uint8_t* label, int32_t* path_xy, float* directions, int32_t* turns, int32_t* leg_ends,
                            int32_t path_capacity, int32_t* path_len) {
    if (!h) return YH_EINVAL;
    const yh_scene_turn_tour* q = h->turn_tour;
    // the checks first (a turn tour of this frame exists; turns takes the route's capacity as path_xy and directions do), then the copies
    int rc = solve_read(h, "turn tour", "plan the turn tour again", q, {}, nullptr, nullptr, 0, path_len);
    if (rc) return rc;
    if ((path_xy || directions || turns) && path_capacity < q->path_len)
        return h->fail(YH_EOVERFLOW, "path_capacity " + std::to_string(path_capacity) + " < the route's " + std::to_string(q->path_len) + " nodes");
    const int K = (int)q->targets.size();
    const size_t states = (size_t)8 * h->W * h->H, nturns = q->path_len > 1 ? (size_t)(q->path_len - 1) * 4 : 0;
    rc = solve_read(h, "turn tour", "plan the turn tour again", q,
                    { { cost, q->cost, K * states * 4 }, { act, q->act, K * states }, { label, q->label, states }, { nturns ? turns : nullptr, q->turns, nturns } },
                    path_xy, directions, path_capacity, path_len);
    if (rc) return rc;
    if (n_targets) *n_targets = K;
    for (int b = 0; b < K; ++b) {
        if (targets_xy) { targets_xy[2 * b] = q->targets[b] % h->W; targets_xy[2 * b + 1] = q->targets[b] / h->W; }
        if (order) order[b] = q->order[b];
        if (leg_ends) leg_ends[b] = q->leg_ends[b];
        if (leg_headings) leg_headings[b] = q->leg_headings[b];
    }
    if (legs) memcpy(legs, q->legs, (size_t)(1 + 8 * K) * K * 4);
    if (arrive) memcpy(arrive, q->arrive, (size_t)(1 + 8 * K) * K);
    if (total) *total = q->total;
    return YH_OK;
}

int yh_scene_turn_tour_time(yh_scene* h, int32_t reps, float* ms_per_tour, int32_t* rounds, int32_t* tile_runs) {
    if (!h || reps < 1 || !ms_per_tour) return YH_EINVAL;
    yh_scene_turn_tour* q = h->turn_tour;
    // (a failed replay has overwritten part of the last turn tour: it is gone; the host's choice of the order is inside the time)
    auto run = [&] { const int rc = run_turn_tour(h, q->targets, q->start, q->heading, q->tau); if (rc) q->planned = false; return rc; };
    return solve_time(h, "turn tour", "plan the turn tour again", q, reps, run, ms_per_tour, rounds, tile_runs);
}

}  // extern "C"
