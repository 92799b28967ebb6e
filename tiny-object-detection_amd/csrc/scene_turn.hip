// scene_turn.hip — the turn-aware planner (yh_scene_plan_turn; DESIGN.md §11 "Turns", restated in tests/turn_ref.py): the cost
// field over states (pixel, heading) with a price tau per 45 degrees turned in place, the action field and the route from
// (start, start heading) as the (magnitude, rotation) pairs GetPath serialises, with the signed turn count before every drive.
//   d[h][t] = 0 at targets in all eight layers; elsewhere d[h][v] = min( fl(fl(d[h][v + s_h] + c(v, v + s_h)) + |h[v] - h[v + s_h]|),
//   fl(d[h - 1][v] + tau), fl(d[h + 1][v] + tau) ), all f32: the 8-connected planner's edge term for the one direction the state
//   faces, and two turns. Every weight is >= 1 (a SANE length, tau), so the uniqueness argument of scene_path.hip carries over and
//   any relaxation order reaches the same bits.
// Headings are the compass index of scene_path_dev.h's rotation(): 0 right, 1 down-right, 2 down, .. 6 up, 7 up-right; h + 1 is
// clockwise on the image.
//
// The device code (the compass, the round, the action rule, the walk) is scene_turn_dev.h's. There is one driver (run_turn) and one
// set of kernels for yh_scene_plan_turn (the batch of one) and yh_scene_batch_plan_turn (the first n of the handle's max_frames): each
// kernel takes its frame from blockIdx.z, advances its own copy of the parameter block to that frame (frame_of with the cost stride
// 8 W H) and runs the body. A frame has its own eight layers, edge terms and tile flags, so frames that share rounds cannot change each
// other's bits (DESIGN.md §11 "Scene batch: turns"); a batch takes the rounds of its slowest frame, not their sum. All arrays are
// frame-major: cost [n][8][H][W] f32, act [n][8][H][W] u8, nodes, dirs, turns [n][W*H], walk_out [n][2].
//
// Launches of one turn plan of n frames:
//   the inputs     ONE copy from the state's pinned block: the seeds as (pixel, frame) pairs, the starts (-1: no plan for that frame),
//                  the headings.
//   path_weights<8> (scene_solve.hip) over the n frames, one fill of 8 n W H values with +inf and turn_seeds (0 in all eight layers of
//                  the seed's frame), then
//   turn_round     (also the turn tour's round kernel: scene_turn_round) x rounds (tiles x n), through scene_solve.hip's host loop (its flags, counters, batches and round cap; ragged seeds):
//                  a flagged workgroup holds its 32 x 32 tile of all eight layers with a one-cell halo each in LDS (36 992 B), a lane
//                  owns a 2 x 2 block x 8 headings in registers with the block's edge terms, sweeps drive moves inside each layer and
//                  turn moves between the layers (7 <-> 0 wraps) in place until a vote finds no change, writes back with atomicMin on
//                  the u32 view and flags neighbours by the 8-connected rule: state (v, h) is read by v and by v - s_h only, so by v's
//                  tile or the tile across a border or corner v lies on. No workgroup waits for another one.
//   turn_act       one lane per pixel (pixels x 1 x n), its edge terms read once for the eight headings: the first of (drive 0, turn to
//                  h - 1 = 1, turn to h + 1 = 2) whose candidate equals d[h][v] bitwise; turn_seeds again writes 255 at the targets.
//   turn_walk      one wave per frame follows act from (start, h0) through a 32 x 32 x 8 window of it in LDS (8 KiB), writes a node per
//                  drive and the turns made before it; then its lanes write the directions.
//   One read-back of n x 2 words and one wait. A frame without a target seeds nothing and flags nothing; its action kernel and walk
//   are skipped.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "scene.h"
#include "scene_batch.h"
#include "scene_path_dev.h"
#include "scene_turn_dev.h"
#include "yh_internal.h"

using namespace yh;

struct yh_scene_turn : PlanFrames {   // all [max_frames][...]; nodes and dirs [max][W*H], walk_out [max][2]
    float* cost = nullptr;        // [max][8][H][W]
    uint8_t* act = nullptr;       // [max][8][H][W]
    int32_t* turns = nullptr;     // [max][W*H]: before the drive from node i
    int32_t* host_walk = nullptr; // pinned [max][2]
    std::vector<int32_t> last_starts, last_headings;   // per frame; start -1: no plan for this frame
    float tau = 1.0f;
};

namespace {

// seeds [n][2] (pixel, frame): cost = 0 in all eight layers of that frame there, or (act given) act = 255 there
__global__ __launch_bounds__(256) void turn_seeds(const PathParams p, const int32_t* seeds, int n, uint8_t* act) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= 8 * n) return;
    const size_t i = ((size_t)seeds[2 * (k >> 3) + 1] * 8 + (k & 7)) * p.W * p.H + seeds[2 * (k >> 3)];
    if (act) act[i] = (uint8_t)ACT_TARGET;
    else p.cost[i] = 0.0f;
}

// The one round kernel of the turn plan and the turn tour: field z = blockIdx.z of F = n kmax fields, kmax per frame (the turn plan:
// one, the field is the frame). The edge terms are the frame's, the eight layers at cost the field's.
__global__ __launch_bounds__(SP_NT) void turn_round(const PathParams p, float tau, int kmax, int F, int parity, uint32_t* cnt_next) {
    const int z = blockIdx.z;
    PathParams q = frame_of(p, z / kmax, 0);
    q.cost += (size_t)z * 8 * p.W * p.H;
    turn_round_body(q, tau, p.flags + (size_t)(parity * F + z) * p.ntiles, p.flags + (size_t)((parity ^ 1) * F + z) * p.ntiles, cnt_next);
}

__global__ __launch_bounds__(256) void turn_act(const PathParams p, float tau, const int32_t* starts, uint8_t* act) {
    const int b = blockIdx.z;
    if (starts[b] < 0) return;
    const size_t states = (size_t)8 * p.W * p.H;
    turn_act_body(frame_of(p, b, states), tau, act + b * states);
}

__global__ __launch_bounds__(64) void turn_walk(const PathParams p, const uint8_t* act, const int32_t* starts, const int32_t* headings, int2* nodes, int32_t* turns,
                                                float2* dirs, int32_t* out) {
    const int b = blockIdx.z, start = starts[b];
    if (start < 0) return;   // (workgroup-uniform)
    const size_t npx = (size_t)p.W * p.H;
    SP_BODY_ON_CACHE_LINE();
    turn_walk_body(frame_of(p, b, 8 * npx), act + b * 8 * npx, start, headings[b], nodes + b * npx, turns + b * npx, dirs + b * npx, out + 2 * b);
}

// the turn planner's buffers, for the handle's max_frames frames, at the first turn plan: a handle that never makes one pays nothing
int ensure_turn(yh_scene* h) {
    if (h->turn) return YH_OK;
    yh_scene_turn* q = h->turn = new yh_scene_turn();
    const size_t mf = (size_t)h->max_frames, all = mf * h->W * h->H;
    SCHK(h, hipMalloc((void**)&q->cost, 8 * all * 4));
    SCHK(h, hipMalloc((void**)&q->act, 8 * all));
    SCHK(h, hipMalloc((void**)&q->nodes, all * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&q->dirs, all * sizeof(float2)));
    SCHK(h, hipMalloc((void**)&q->turns, all * 4));
    SCHK(h, hipMalloc((void**)&q->walk_out, mf * 2 * 4));
    SCHK(h, hipHostMalloc((void**)&q->host_walk, mf * 2 * 4, hipHostMallocDefault));
    return YH_OK;
}

// the whole turn plan of q->n frames on the handle's stream: last_seeds / last_field (pixel and frame of every target), last_starts,
// last_headings, tau. Returns when every route's length is known.
int run_turn(yh_scene* h) {
    yh_scene_turn* q = h->turn;
    const int n = q->n, ns = (int)q->last_seeds.size();
    int rc = plan_inputs_reserve(h, q->in, 2 * (size_t)ns + 2 * h->max_frames);
    if (rc) return rc;
    const size_t ws = plan_inputs_seeds(*q);
    std::copy(q->last_starts.begin(), q->last_starts.end(), q->in.host + ws);
    std::copy(q->last_headings.begin(), q->last_headings.end(), q->in.host + ws + n);
    SCHK(h, hipMemcpyAsync(q->in.dev, q->in.host, (ws + 2 * n) * 4, hipMemcpyHostToDevice, h->stream));
    const int32_t *seeds = q->in.dev, *starts = seeds + ws, *headings = starts + n;
    PathParams p;
    if ((rc = solve_begin(h, 8, h->max_frames, n, p))) return rc;
    p.cost = q->cost;
    const size_t npx = (size_t)h->W * h->H;
    const float tau = q->tau;
    const dim3 px((unsigned)((npx + 255) / 256), 1, (unsigned)n), sd((unsigned)((8 * (size_t)ns + 255) / 256));
    SCHK(h, hipMemsetD32Async((hipDeviceptr_t)q->cost, 0x7f800000, 8 * n * npx, h->stream));   // +inf
    hipLaunchKernelGGL(turn_seeds, sd, dim3(256), 0, h->stream, p, seeds, ns, (uint8_t*)nullptr);
    const SolveRound round = scene_turn_round(h, p, tau, 1, n);
    if ((rc = solve_rounds(h, p, 8, n, q->last_seeds, h->batch ? "batch turn" : "turn", 0, nullptr, &round, &q->last_field))) return rc;
    hipLaunchKernelGGL(turn_act, px, dim3(256), 0, h->stream, p, tau, starts, q->act);
    hipLaunchKernelGGL(turn_seeds, sd, dim3(256), 0, h->stream, p, seeds, ns, q->act);
    hipLaunchKernelGGL(turn_walk, dim3(1, 1, (unsigned)n), dim3(64), 0, h->stream, p, q->act, starts, headings, q->nodes, q->turns, q->dirs, q->walk_out);
    SCHK(h, hipGetLastError());
    SCHK(h, hipMemcpyAsync(q->host_walk, q->walk_out, (size_t)n * 2 * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    q->path_len.assign(n, 0);
    for (int b = 0; b < n; ++b) {
        if (q->last_starts[b] < 0) continue;
        if (q->host_walk[2 * b + 1]) return h->fail(YH_EHIP, h->frame_tag(b) + "turn walk: no target within 8*W*H actions (fields not those of a SANE frame?)");
        q->path_len[b] = q->host_walk[2 * b];
    }
    return YH_OK;
}

// the inputs of a call are in h->turn: run it, and it is the handle's last turn plan
int turn_now(yh_scene* h) {
    yh_scene_turn* q = h->turn;
    q->last.planned = false;
    const int rc = run_turn(h);
    if (rc) return rc;
    q->last.conn = 8; q->last.planned = true; q->last.frame = h->frames;
    return YH_OK;
}

int turn_read(yh_scene* h, int frame, float* cost, uint8_t* act, int32_t* path_xy, float* directions, int32_t* turns, int32_t path_capacity, int32_t* path_len) {
    const yh_scene_turn* q = h->turn;
    const size_t npx = (size_t)h->W * h->H, states = 8 * npx;
    SolveLast one;
    const int rc = solve_frame(h, q, frame, npx, "turn plan", one);
    if (rc) return rc;
    // (turns takes the route's capacity as path_xy and directions do)
    const size_t nturns = one.path_len > 1 ? (size_t)(one.path_len - 1) * 4 : 0;
    return solve_read(h, "turn plan", "plan again", &one,
                      { { cost, q ? q->cost + frame * states : nullptr, states * 4 }, { act, q ? q->act + frame * states : nullptr, states },
                        { nturns ? turns : nullptr, q ? q->turns + frame * npx : nullptr, nturns } },
                      path_xy, directions, path_capacity, path_len, turns != nullptr);
}

int turn_time(yh_scene* h, int32_t reps, float* ms, int32_t* rounds, int32_t* tile_runs) {
    yh_scene_turn* q = h->turn;
    // (a failed replay has overwritten part of the last turn plan: it is gone)
    auto run = [&] { const int rc = run_turn(h); if (rc) q->last.planned = false; return rc; };
    return solve_time(h, "turn plan", "plan again", q ? &q->last : nullptr, reps, run, ms, rounds, tile_runs);
}

}  // namespace

namespace yh {
SolveRound scene_turn_round(yh_scene* h, const PathParams& p, float tau, int kmax, int F) {
    return SolveRound{ [=](const dim3& tiles, int parity, uint32_t* cnt_next) {
        hipLaunchKernelGGL(turn_round, tiles, dim3(SP_NT), 0, h->stream, p, tau, kmax, F, parity, cnt_next);
    }, 8 };
}

void scene_turn_free(yh_scene* h) {
    yh_scene_turn* q = h->turn;
    if (!q) return;
    void* bufs[] = { q->cost, q->act, q->turns, q->nodes, q->dirs, q->walk_out };
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (q->host_walk) (void)hipHostFree(q->host_walk);
    plan_inputs_free(q->in);
    delete q;
    h->turn = nullptr;
}
}  // namespace yh

extern "C" {

int yh_scene_plan_turn(yh_scene* h, const int32_t* targets_xy, int32_t n_targets, int32_t start_x, int32_t start_y, int32_t start_heading, float turn_price) {
    if (!h) return YH_EINVAL;
    int rc;
    if ((rc = scene_turn_heading(h, start_heading)) || (rc = scene_turn_price(h, turn_price))) return rc;
    std::vector<int32_t> targets;
    if ((rc = scene_plan_targets(h, targets_xy, n_targets, start_x, start_y, targets))) return rc;
    if ((rc = scene_turn_size(h)) || (rc = scene_plan_diagonals(h, h->diag_ok, h->diag_why))) return rc;
    if ((rc = ensure_turn(h))) { scene_turn_free(h); return rc; }
    yh_scene_turn* q = h->turn;   // the batch of one: every seed in frame 0, one start, one heading
    q->n = 1; q->tau = turn_price; q->status.assign(1, YH_OK);
    q->last_starts.assign(1, start_y * h->W + start_x); q->last_headings.assign(1, start_heading);
    q->last_field.assign(targets.size(), 0); q->last_seeds = std::move(targets);
    return turn_now(h);
}

int yh_scene_batch_plan_turn(yh_scene_batch* hb, const int32_t* targets_xy, int32_t n_targets, const int32_t* starts_xy, const int32_t* start_headings,
                             float turn_price, int32_t* status) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (!starts_xy) return h->fail(YH_EINVAL, "starts_xy is null");
    if (!start_headings) return h->fail(YH_EINVAL, "start_headings is null");
    int rc = scene_turn_price(h, turn_price);
    if (rc) return rc;
    std::vector<int32_t> seeds, field, starts(hb->n, -1), st;
    rc = scene_batch_frames(hb, targets_xy, n_targets, starts_xy, start_headings, 8, st, [&](int b, const std::vector<int32_t>& t) {
        starts[b] = starts_xy[2 * b + 1] * h->W + starts_xy[2 * b];
        for (int32_t v : t) { seeds.push_back(v); field.push_back(b); }
        return YH_OK;
    });
    if (rc) return rc;
    if (status) std::copy(st.begin(), st.end(), status);
    if (seeds.empty()) return h->fail(YH_ESTATE, "no target given and no frame of the batch has a ball inside it");
    h->err.clear();
    if ((rc = ensure_turn(h))) { scene_turn_free(h); return rc; }
    yh_scene_turn* q = h->turn;
    q->n = hb->n; q->tau = turn_price; q->status = st;
    q->last_starts = starts; q->last_headings.assign(start_headings, start_headings + hb->n);
    q->last_seeds = seeds; q->last_field = field;
    return turn_now(h);
}

int yh_scene_turn_read(yh_scene* h, float* cost, uint8_t* act, int32_t* path_xy, float* directions, int32_t* turns, int32_t path_capacity, int32_t* path_len) {
    if (!h) return YH_EINVAL;
    return turn_read(h, 0, cost, act, path_xy, directions, turns, path_capacity, path_len);
}

int yh_scene_batch_turn_read(yh_scene_batch* hb, int32_t frame, float* cost, uint8_t* act, int32_t* path_xy, float* directions, int32_t* turns, int32_t path_capacity,
                             int32_t* path_len) {
    if (!hb) return YH_EINVAL;
    const int rc = hb->frame_ok(frame);
    if (rc) return rc;
    return turn_read(&hb->core, frame, cost, act, path_xy, directions, turns, path_capacity, path_len);
}

int yh_scene_turn_time(yh_scene* h, int32_t reps, float* ms_per_plan, int32_t* rounds, int32_t* tile_runs) {
    if (!h || reps < 1 || !ms_per_plan) return YH_EINVAL;
    return turn_time(h, reps, ms_per_plan, rounds, tile_runs);
}

int yh_scene_batch_turn_time(yh_scene_batch* hb, int32_t reps, float* ms_per_batch, int32_t* rounds, int32_t* tile_runs) {
    if (!hb || reps < 1 || !ms_per_batch) return YH_EINVAL;
    return turn_time(&hb->core, reps, ms_per_batch, rounds, tile_runs);
}

}  // extern "C"
