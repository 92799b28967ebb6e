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
// The device code (the compass, the round, the action rule, the walk) is scene_turn_dev.h's: the kernels here call its bodies with
// their own arguments, the scene batch's (scene_batch_turn.hip) with the frame taken from blockIdx.z.
//
// Launches of one turn plan:
//   path_weights<8> (scene_solve.hip), turn_fill (+inf in the eight layers) and turn_targets (0 at the targets, all layers), then
//   turn_round     x rounds, through scene_solve.hip's host loop (its flags, counters, batches and round cap): a flagged workgroup
//                  holds its 32 x 32 tile of all eight layers with a one-cell halo each in LDS (36 992 B), a lane owns a 2 x 2 block
//                  x 8 headings in registers with the block's edge terms, sweeps drive moves inside each layer and turn moves between
//                  the layers (7 <-> 0 wraps) in place until a vote finds no change, writes back with atomicMin on the u32 view and
//                  flags neighbours by the 8-connected rule: state (v, h) is read by v and by v - s_h only, so by v's tile or the tile
//                  across a border or corner v lies on. No workgroup waits for another one.
//   turn_act       one lane per pixel, its edge terms read once for the eight headings: the first of (drive 0, turn to h - 1 = 1,
//                  turn to h + 1 = 2) whose candidate equals d[h][v] bitwise; turn_mark_targets then writes 255 at the targets.
//   turn_walk      one wave follows act from (start, h0) through a 32 x 32 x 8 window of it in LDS (8 KiB), writes a node per drive
//                  and the turns made before it; then its lanes write the directions.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "scene.h"
#include "scene_path_dev.h"
#include "scene_turn_dev.h"
#include "yh_internal.h"

using namespace yh;

struct yh_scene_turn : SolveLast {   // (the route, the start and whether a turn plan exists: SolveLast)
    float* cost = nullptr;        // [8][H][W]
    uint8_t* act = nullptr;       // [8][H][W]
    int32_t* turns = nullptr;     // [H * W]: before the drive from node i
    int32_t* targets = nullptr;   // [targets_cap] linear indices
    int32_t targets_cap = 0;
    int32_t* walk_out = nullptr;  // [2]: length, status
    std::vector<int32_t> last_targets;
    int32_t heading = 6;
    float tau = 1.0f;
};

namespace {

__global__ __launch_bounds__(256) void turn_fill(const PathParams p) { turn_fill_body(p); }

__global__ __launch_bounds__(256) void turn_targets(const PathParams p, const int32_t* targets, int n) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= 8 * n) return;
    p.cost[(size_t)(k & 7) * p.W * p.H + targets[k >> 3]] = 0.0f;
}

__global__ __launch_bounds__(256) void turn_mark_targets(const PathParams p, uint8_t* act, const int32_t* targets, int n) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= 8 * n) return;
    act[(size_t)(k & 7) * p.W * p.H + targets[k >> 3]] = (uint8_t)ACT_TARGET;
}

// The bodies are scene_turn_dev.h's; the batch (scene_batch_turn.hip) runs the same ones on the frame of blockIdx.z.
__global__ __launch_bounds__(SP_NT) void turn_round(const PathParams p, float tau, int parity, uint32_t* cnt_next) {
    turn_round_body(p, tau, p.flags + (size_t)parity * p.ntiles, p.flags + (size_t)(parity ^ 1) * p.ntiles, cnt_next);
}

__global__ __launch_bounds__(256) void turn_act(const PathParams p, float tau, uint8_t* act) { turn_act_body(p, tau, act); }

__global__ __launch_bounds__(64) void turn_walk(const PathParams p, const uint8_t* act, int start, int heading, int2* nodes, int32_t* turns, float2* dirs, int32_t* out) {
    turn_walk_body(p, act, start, heading, nodes, turns, dirs, out);
}

int ensure_buffers(yh_scene* h) {
    yh_scene_turn* q = h->turn;
    const size_t npx = (size_t)h->W * h->H;
    SCHK(h, hipMalloc((void**)&q->cost, 8 * npx * 4));
    SCHK(h, hipMalloc((void**)&q->act, 8 * npx));
    SCHK(h, hipMalloc((void**)&q->nodes, npx * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&q->dirs, npx * sizeof(float2)));
    SCHK(h, hipMalloc((void**)&q->turns, npx * 4));
    SCHK(h, hipMalloc((void**)&q->walk_out, 2 * 4));
    return YH_OK;
}

// the whole turn plan on the handle's stream; returns when the route's length is known
int run_turn(yh_scene* h, const std::vector<int32_t>& targets, int32_t start, int32_t heading, float tau) {
    yh_scene_turn* q = h->turn;
    const int n = (int)targets.size();
    if (n > q->targets_cap) {
        if (q->targets) { SCHK(h, hipStreamSynchronize(h->stream)); SCHK(h, hipFree(q->targets)); q->targets = nullptr; q->targets_cap = 0; }
        SCHK(h, hipMalloc((void**)&q->targets, (size_t)n * 4));
        q->targets_cap = n;
    }
    const size_t npx = (size_t)h->W * h->H;
    const dim3 px((unsigned)((npx + 255) / 256)), st((unsigned)((8 * npx + 255) / 256)), tg((unsigned)((8 * (size_t)n + 255) / 256));
    SCHK(h, hipMemcpyAsync(q->targets, targets.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    PathParams p;
    int rc = solve_begin(h, 8, 1, p);
    if (rc) return rc;
    p.cost = q->cost; p.next = nullptr;
    hipLaunchKernelGGL(turn_fill, st, dim3(256), 0, h->stream, p);
    hipLaunchKernelGGL(turn_targets, tg, dim3(256), 0, h->stream, p, q->targets, n);
    const SolveRound round = { [&](const dim3& tiles, int parity, uint32_t* cnt_next) {
        hipLaunchKernelGGL(turn_round, dim3(tiles.x, tiles.y), dim3(SP_NT), 0, h->stream, p, tau, parity, cnt_next);
    }, 8 };
    if ((rc = solve_rounds(h, p, 8, 1, targets, "turn", 0, nullptr, &round))) return rc;
    hipLaunchKernelGGL(turn_act, px, dim3(256), 0, h->stream, p, tau, q->act);
    hipLaunchKernelGGL(turn_mark_targets, tg, dim3(256), 0, h->stream, p, q->act, q->targets, n);
    hipLaunchKernelGGL(turn_walk, dim3(1), dim3(64), 0, h->stream, p, q->act, (int)start, (int)heading, q->nodes, q->turns, q->dirs, q->walk_out);
    SCHK(h, hipGetLastError());
    int32_t* wo = reinterpret_cast<int32_t*>(h->solve->host + kSolveCnt + kSolveTail);
    SCHK(h, hipMemcpyAsync(wo, q->walk_out, 2 * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    if (wo[1]) return h->fail(YH_EHIP, "turn walk: no target within 8*W*H actions (fields not those of a SANE frame?)");
    q->path_len = wo[0];
    return YH_OK;
}

}  // namespace

namespace yh {
void scene_turn_free(yh_scene* h) {
    yh_scene_turn* q = h->turn;
    if (!q) return;
    void* bufs[] = { q->cost, q->act, q->turns, q->targets, q->nodes, q->dirs, q->walk_out };
    for (void* b : bufs) if (b) (void)hipFree(b);
    delete q;
    h->turn = nullptr;
}
}  // namespace yh

extern "C" {

int yh_scene_plan_turn(yh_scene* h, const int32_t* targets_xy, int32_t n_targets, int32_t start_x, int32_t start_y, int32_t start_heading, float turn_price) {
    if (!h) return YH_EINVAL;
    if (start_heading < 0 || start_heading > 7) return h->fail(YH_EINVAL, "start heading " + std::to_string(start_heading) + ": 0 .. 7 (0 right, clockwise on the image, 6 up)");
    if (!std::isfinite(turn_price) || turn_price < 1.0f || turn_price > 1024.0f)
        return h->fail(YH_EINVAL, "turn price must be a finite number in [1, 1024] (every weight >= 1 is what makes the field unique)");
    std::vector<int32_t> targets;
    int rc = scene_plan_targets(h, targets_xy, n_targets, start_x, start_y, targets);
    if (rc) return rc;
    const long long W = h->W, H = h->H;
    if ((W + H) * (2 * std::max(H, 101LL) + 1) + 8 * 1024 >= (1LL << 24))
        return h->fail(YH_EINVAL, "frame too large for the turn planner: (W + H) * (2 * max(H, 101) + 1) + 8 * 1024 must stay below 2^24");
    if ((rc = scene_plan_diagonals(h))) return rc;
    if (!h->turn) {   // allocated at the first turn plan: a handle that never makes one pays nothing
        h->turn = new yh_scene_turn();
        rc = ensure_buffers(h);
        if (rc) { scene_turn_free(h); return rc; }
    }
    yh_scene_turn* q = h->turn;
    q->planned = false;
    const int32_t start = (int32_t)(start_y * W + start_x);
    rc = run_turn(h, targets, start, start_heading, turn_price);
    if (rc) return rc;
    q->conn = 8;
    q->planned = true; q->frame = h->frames; q->last_targets = targets; q->start = start; q->heading = start_heading; q->tau = turn_price;
    return YH_OK;
}

int yh_scene_turn_read(yh_scene* h, float* cost, uint8_t* act, int32_t* path_xy, float* directions, int32_t* turns, int32_t path_capacity, int32_t* path_len) {
    if (!h) return YH_EINVAL;
    const yh_scene_turn* q = h->turn;
    const size_t states = (size_t)8 * h->W * h->H;
    // the checks first (a turn plan of this frame exists; turns takes the route's capacity as path_xy and directions do), then the copies
    int rc = solve_read(h, "turn plan", "plan again", q, {}, nullptr, nullptr, 0, path_len);
    if (rc) return rc;
    if ((path_xy || directions || turns) && path_capacity < q->path_len)
        return h->fail(YH_EOVERFLOW, "path_capacity " + std::to_string(path_capacity) + " < the route's " + std::to_string(q->path_len) + " nodes");
    const size_t nturns = q->path_len > 1 ? (size_t)(q->path_len - 1) * 4 : 0;
    return solve_read(h, "turn plan", "plan again", q, { { cost, q->cost, states * 4 }, { act, q->act, states }, { nturns ? turns : nullptr, q->turns, nturns } },
                      path_xy, directions, path_capacity, path_len);
}

int yh_scene_turn_time(yh_scene* h, int32_t reps, float* ms_per_plan, int32_t* rounds, int32_t* tile_runs) {
    if (!h || reps < 1 || !ms_per_plan) return YH_EINVAL;
    yh_scene_turn* q = h->turn;
    // (a failed replay has overwritten part of the last turn plan: it is gone)
    auto run = [&] { const int rc = run_turn(h, q->last_targets, q->start, q->heading, q->tau); if (rc) q->planned = false; return rc; };
    return solve_time(h, "turn plan", "plan again", q, reps, run, ms_per_plan, rounds, tile_runs);
}

}  // extern "C"
