// scene_batch_turn.hip — yh_scene_batch_plan_turn: the turn-aware plan (scene_turn.hip; DESIGN.md §11 "Turns") for every frame of a
// scene batch in shared solver rounds (DESIGN.md §11 "Scene batch: turns"). Frame b has exactly the results of yh_scene_plan_turn on a
// yh_scene of the same size fed that frame alone: every kernel here takes its frame from blockIdx.z, advances its own copy of the
// parameter block to that frame and runs the body the single handle's kernel runs (scene_turn_dev.h). The field is unique (every
// weight >= 1), and a frame has its own eight layers, edge terms and tile flags, so frames that share rounds cannot change each
// other's bits; the batch takes the rounds of its slowest frame, not their sum.
//
// Layout, all frame-major for max_frames frames, allocated at the first batched turn plan: cost [n][8][H][W] f32, act [n][8][H][W] u8,
// nodes, dirs, turns [n][W*H], walk_out [n][2], starts and headings [n] (start -1: no plan for that frame). The frame stride of cost
// and act is 8 W H - NOT the W H of the plain plan's cost (scene_batch.hip's frame_of); turn_frame_of below is this unit's own advance.
//
// Launches of one call: the uploads (seeds with their frames, starts, headings), batch_weights<8> (scene_batch.hip), one fill of
// 8 n W H values with +inf, batch_turn_seeds (0 in all eight layers of the seed's frame), batch_turn_round x rounds through
// scene_solve.hip's host loop (SolveRound{.., 8}, ragged seeds, tiles x n; flags [2][n][ntiles] as batch_round indexes them),
// batch_turn_act (pixels x 1 x n), batch_turn_seeds again (255 in act), batch_turn_walk (one wave per frame), one read-back of n x 2
// words, one wait. A frame without a target seeds nothing and flags nothing; its action kernel and walk are skipped.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "scene.h"
#include "scene_batch.h"
#include "scene_path_dev.h"
#include "scene_turn_dev.h"
#include "yh_internal.h"

using namespace yh;

struct yh_scene_batch_turn {
    float* cost = nullptr;        // [max][8][H][W]
    uint8_t* act = nullptr;       // [max][8][H][W]
    int2* nodes = nullptr;        // [max][W*H]
    float2* dirs = nullptr;       // [max][W*H]
    int32_t* turns = nullptr;     // [max][W*H]: before the drive from node i
    int32_t* walk_out = nullptr;  // [max][2]: length, status
    int32_t* starts = nullptr;    // [max] linear index, -1: no plan for this frame
    int32_t* headings = nullptr;  // [max]
    int32_t* seeds = nullptr;     // [seeds_cap][2]: linear index, frame
    int32_t seeds_cap = 0;
    int32_t* host_walk = nullptr; // pinned [max][2]
    SolveLast last;               // planned, frame generation
    std::vector<int32_t> status, path_len, last_seeds, last_field, last_starts, last_headings;
    std::vector<int32_t> pairs;   // last_seeds and last_field interleaved, as uploaded
    float tau = 1.0f;
};

namespace {

// frame b of the turn batch: the scene fields and edge terms advance by W H as everywhere, the eight layers at cost by 8 W H
__device__ __forceinline__ PathParams turn_frame_of(const PathParams& p, int b) {
    PathParams q = p;
    const size_t npx = (size_t)p.W * p.H;
    q.edge += b * npx; q.edge2 += b * npx; q.cost += b * 8 * npx;
    return q;
}

// seeds [n][2] (pixel, frame): cost = 0 in all eight layers of that frame there, or (act given) act = 255 there
__global__ __launch_bounds__(256) void batch_turn_seeds(const PathParams p, const int32_t* seeds, int n, uint8_t* act) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= 8 * n) return;
    const size_t i = ((size_t)seeds[2 * (k >> 3) + 1] * 8 + (k & 7)) * p.W * p.H + seeds[2 * (k >> 3)];
    if (act) act[i] = (uint8_t)ACT_TARGET;
    else p.cost[i] = 0.0f;
}

__global__ __launch_bounds__(SP_NT) void batch_turn_round(const PathParams p, float tau, int F, int parity, uint32_t* cnt_next) {
    const int b = blockIdx.z;
    turn_round_body(turn_frame_of(p, b), tau, p.flags + (size_t)(parity * F + b) * p.ntiles, p.flags + (size_t)((parity ^ 1) * F + b) * p.ntiles, cnt_next);
}

__global__ __launch_bounds__(256) void batch_turn_act(const PathParams p, float tau, const int32_t* starts, uint8_t* act) {
    const int b = blockIdx.z;
    if (starts[b] < 0) return;
    turn_act_body(turn_frame_of(p, b), tau, act + (size_t)b * 8 * p.W * p.H);
}

__global__ __launch_bounds__(64) void batch_turn_walk(const PathParams p, const uint8_t* act, const int32_t* starts, const int32_t* headings, int2* nodes, int32_t* turns,
                                                      float2* dirs, int32_t* out) {
    const int b = blockIdx.z, start = starts[b];
    if (start < 0) return;   // (workgroup-uniform)
    const size_t npx = (size_t)p.W * p.H;
    turn_walk_body(turn_frame_of(p, b), act + b * 8 * npx, start, headings[b], nodes + b * npx, turns + b * npx, dirs + b * npx, out + 2 * b);
}

int ensure_buffers(yh_scene_batch* hb) {
    yh_scene* h = &hb->core;
    yh_scene_batch_turn* q = hb->turn;
    const size_t all = (size_t)hb->max_frames * h->W * h->H;
    SCHK(h, hipMalloc((void**)&q->cost, 8 * all * 4));
    SCHK(h, hipMalloc((void**)&q->act, 8 * all));
    SCHK(h, hipMalloc((void**)&q->nodes, all * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&q->dirs, all * sizeof(float2)));
    SCHK(h, hipMalloc((void**)&q->turns, all * 4));
    SCHK(h, hipMalloc((void**)&q->walk_out, (size_t)hb->max_frames * 2 * 4));
    SCHK(h, hipMalloc((void**)&q->starts, (size_t)hb->max_frames * 4));
    SCHK(h, hipMalloc((void**)&q->headings, (size_t)hb->max_frames * 4));
    SCHK(h, hipHostMalloc((void**)&q->host_walk, (size_t)hb->max_frames * 2 * 4, hipHostMallocDefault));
    return YH_OK;
}

// the whole turn plan of hb->n frames on the handle's stream: last_seeds / last_field (pixel and frame of every target), last_starts
// (-1: no plan for that frame), last_headings, tau. Returns when every route's length is known.
int run_turn(yh_scene_batch* hb) {
    yh_scene* h = &hb->core;
    yh_scene_batch_turn* q = hb->turn;
    const int n = hb->n, ns = (int)q->last_seeds.size();
    if (ns > q->seeds_cap) {
        if (q->seeds) { SCHK(h, hipStreamSynchronize(h->stream)); SCHK(h, hipFree(q->seeds)); q->seeds = nullptr; q->seeds_cap = 0; }
        SCHK(h, hipMalloc((void**)&q->seeds, (size_t)ns * 2 * 4));
        q->seeds_cap = ns;
    }
    q->pairs.resize((size_t)ns * 2);
    for (int k = 0; k < ns; ++k) { q->pairs[2 * k] = q->last_seeds[k]; q->pairs[2 * k + 1] = q->last_field[k]; }
    SCHK(h, hipMemcpyAsync(q->seeds, q->pairs.data(), q->pairs.size() * 4, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipMemcpyAsync(q->starts, q->last_starts.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipMemcpyAsync(q->headings, q->last_headings.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    PathParams p;
    int rc = solve_alloc(h, 8, hb->max_frames, hb->max_frames, p);
    if (rc) return rc;
    p.cost = q->cost; p.next = nullptr;
    const size_t npx = (size_t)h->W * h->H;
    const float tau = q->tau;
    const dim3 px((unsigned)((npx + 255) / 256), 1, (unsigned)n), sd((unsigned)((8 * (size_t)ns + 255) / 256));
    scene_batch_weights(h, p, 8, n);
    SCHK(h, hipMemsetD32Async((hipDeviceptr_t)q->cost, 0x7f800000, 8 * n * npx, h->stream));   // +inf
    hipLaunchKernelGGL(batch_turn_seeds, sd, dim3(256), 0, h->stream, p, q->seeds, ns, (uint8_t*)nullptr);
    const SolveRound round{ [&](const dim3& tiles, int parity, uint32_t* cnt_next) {
        hipLaunchKernelGGL(batch_turn_round, tiles, dim3(SP_NT), 0, h->stream, p, tau, n, parity, cnt_next);
    }, 8 };
    if ((rc = solve_rounds(h, p, 8, n, q->last_seeds, "batch turn", 0, nullptr, &round, &q->last_field))) return rc;
    hipLaunchKernelGGL(batch_turn_act, px, dim3(256), 0, h->stream, p, tau, q->starts, q->act);
    hipLaunchKernelGGL(batch_turn_seeds, sd, dim3(256), 0, h->stream, p, q->seeds, ns, q->act);
    hipLaunchKernelGGL(batch_turn_walk, dim3(1, 1, (unsigned)n), dim3(64), 0, h->stream, p, q->act, q->starts, q->headings, q->nodes, q->turns, q->dirs, q->walk_out);
    SCHK(h, hipGetLastError());
    SCHK(h, hipMemcpyAsync(q->host_walk, q->walk_out, (size_t)n * 2 * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    q->path_len.assign(n, 0);
    for (int b = 0; b < n; ++b) {
        if (q->last_starts[b] < 0) continue;
        if (q->host_walk[2 * b + 1]) return h->fail(YH_EHIP, "frame " + std::to_string(b) + ": turn walk: no target within 8*W*H actions (fields not those of a SANE frame?)");
        q->path_len[b] = q->host_walk[2 * b];
    }
    return YH_OK;
}

}  // namespace

namespace yh {
void scene_batch_turn_free(yh_scene_batch* hb) {
    yh_scene_batch_turn* q = hb->turn;
    if (!q) return;
    void* bufs[] = { q->cost, q->act, q->nodes, q->dirs, q->turns, q->walk_out, q->starts, q->headings, q->seeds };
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (q->host_walk) (void)hipHostFree(q->host_walk);
    delete q;
    hb->turn = nullptr;
}
}  // namespace yh

extern "C" {

int yh_scene_batch_plan_turn(yh_scene_batch* hb, const int32_t* targets_xy, int32_t n_targets, const int32_t* starts_xy, const int32_t* start_headings,
                             float turn_price, int32_t* status) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (!starts_xy) return h->fail(YH_EINVAL, "starts_xy is null");
    if (!start_headings) return h->fail(YH_EINVAL, "start_headings is null");
    if (!std::isfinite(turn_price) || turn_price < 1.0f || turn_price > 1024.0f)
        return h->fail(YH_EINVAL, "turn price must be a finite number in [1, 1024] (every weight >= 1 is what makes the field unique)");
    if (!h->ran || hb->n < 1) return h->fail(YH_ESTATE, "no frame has been appended");
    const int n = hb->n;
    const auto framed = [&](int b, int rc) { h->err = "frame " + std::to_string(b) + ": " + h->err; return rc; };
    // every check of every frame before anything is touched: a refused call leaves an earlier turn plan of this append readable
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
    std::vector<int32_t> seeds, field, starts(n, -1), st(n, YH_OK), t;
    for (int b = 0; b < n; ++b) {
        rc = scene_plan_choose(h, targets_xy ? targets_xy + (size_t)b * n_targets * 2 : nullptr, n_targets,
                               targets_xy ? nullptr : reinterpret_cast<const float(*)[4]>(balls.data() + (size_t)b * 400), t);
        if (rc == YH_ESTATE && !targets_xy) { st[b] = YH_ESTATE; continue; }   // no usable ball: this frame gets no plan
        if (rc) return framed(b, rc);
        starts[b] = (int32_t)(starts_xy[2 * b + 1] * W + starts_xy[2 * b]);
        for (int32_t v : t) { seeds.push_back(v); field.push_back(b); }
    }
    if (status) std::copy(st.begin(), st.end(), status);
    if (seeds.empty()) return h->fail(YH_ESTATE, "no target given and no frame of the batch has a ball inside it");
    h->err.clear();
    if (!hb->turn) {   // allocated at the first batched turn plan: a handle that never makes one pays nothing
        hb->turn = new yh_scene_batch_turn();
        if ((rc = ensure_buffers(hb))) { scene_batch_turn_free(hb); return rc; }
    }
    yh_scene_batch_turn* q = hb->turn;
    q->last.planned = false;
    q->last_seeds = seeds; q->last_field = field; q->last_starts = starts; q->status = st;
    q->last_headings.assign(start_headings, start_headings + n);
    q->tau = turn_price;
    if ((rc = run_turn(hb))) return rc;
    q->last.conn = 8; q->last.planned = true; q->last.frame = h->frames;
    return YH_OK;
}

int yh_scene_batch_turn_read(yh_scene_batch* hb, int32_t frame, float* cost, uint8_t* act, int32_t* path_xy, float* directions, int32_t* turns, int32_t path_capacity,
                             int32_t* path_len) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (frame < 0 || frame >= hb->max_frames || (h->ran && frame >= hb->n)) return h->fail(YH_EINVAL, "frame " + std::to_string(frame) + " outside the last append's " + std::to_string(hb->n));
    const yh_scene_batch_turn* q = hb->turn;
    SolveLast one = q ? q->last : SolveLast();   // this frame's part of the batch's turn plan
    const size_t npx = (size_t)h->W * h->H, states = 8 * npx;
    if (one.planned && one.frame == h->frames) {
        if (q->status[frame] != YH_OK) return h->fail(YH_ESTATE, "frame " + std::to_string(frame) + " had no ball inside it: it has no turn plan");
        one.path_len = q->path_len[frame]; one.nodes = q->nodes + frame * npx; one.dirs = q->dirs + frame * npx;
    }
    // the checks first (a turn plan of this frame exists; turns takes the route's capacity as path_xy and directions do), then the copies
    int rc = solve_read(h, "turn plan", "plan again", &one, {}, nullptr, nullptr, 0, path_len);
    if (rc) return rc;
    if ((path_xy || directions || turns) && path_capacity < one.path_len)
        return h->fail(YH_EOVERFLOW, "path_capacity " + std::to_string(path_capacity) + " < the route's " + std::to_string(one.path_len) + " nodes");
    const size_t nturns = one.path_len > 1 ? (size_t)(one.path_len - 1) * 4 : 0;
    return solve_read(h, "turn plan", "plan again", &one,
                      { { cost, q->cost + frame * states, states * 4 }, { act, q->act + frame * states, states }, { nturns ? turns : nullptr, q->turns + frame * npx, nturns } },
                      path_xy, directions, path_capacity, path_len);
}

int yh_scene_batch_turn_time(yh_scene_batch* hb, int32_t reps, float* ms_per_batch, int32_t* rounds, int32_t* tile_runs) {
    if (!hb || reps < 1 || !ms_per_batch) return YH_EINVAL;
    yh_scene_batch_turn* q = hb->turn;
    // (a failed replay has overwritten part of the last turn plan: it is gone)
    auto run = [&] { const int rc = run_turn(hb); if (rc) q->last.planned = false; return rc; };
    return solve_time(&hb->core, "turn plan", "plan again", q ? &q->last : nullptr, reps, run, ms_per_batch, rounds, tile_runs);
}

}  // extern "C"
