// scene_path.hip — modify_path (src/path.rs:25-120 of the reference) on the scene's device-resident fields: the multi-source cost
// field from the balls over the 4-connected pixel grid, the successor field, and the route from the robot's pixel as the
// (magnitude, rotation) pairs GetPath serialises (path.rs:17-21). What is computed is the definition frozen in DESIGN.md §11
// "Path planner" and restated in tests/path_ref.py (the reference's function indexes 224 x 224 arrays by x + y * 480 and panics):
//   d[t] = 0 at targets, elsewhere d[v] = min over neighbours u of fl(fl(d[u] + c(v,u)) + |h[v] - h[u]|), all f32, this association
//   (path.rs:59's left-to-right sum; the unit builds with -ffp-contract=off and the sum has no product to contract anyway).
// Every c >= 1 in SANE, so fl(d + w) > d while d < 2^24: the equations have ONE solution and any relaxation order reaches it bit
// for bit - every value a relaxation ever writes is the cost of a real path evaluated in that association, values only decrease,
// and the set of f32 values is finite. That is what lets the solver below be asynchronous and still be tested with array_equal.
//
// Launches of one plan of n frames (yh_scene_plan: the batch of one; yh_scene_batch_plan: the first n of the handle's max_frames). There
// is one driver (run_plan) and one set of kernels: each takes its frame from blockIdx.z, advances its own copy of the by-value parameter
// block by that many frames (frame_of, scene_path_dev.h) and runs the body. The field is unique, so frames that share the solver's
// rounds cannot change each other's bits: a frame has its own cost field, edge terms and tile flags, the counters sum over the frames
// as they do over a tour's fields, and a batch takes the rounds of its slowest frame. A frame without a target (no usable ball) seeds
// nothing, flags nothing, and its successor kernel and walk are skipped (start -1).
//   the inputs     ONE copy from the state's pinned block: the seeds as (pixel, frame) pairs, then the starts.
//   path_weights   (scene_solve.hip) over the n frames, then one fill of the n cost fields with +inf and plan_seeds (cost = 0), then
//   plan_round     x rounds (tiles x n; scene_solve.hip's host loop, ragged seeds): relaxes every frame's field tile by tile to its
//                  fixed point, the targets its seeds.
//   plan_next      one lane per pixel: the first neighbour in the order (left, right, up, down) whose candidate equals d[v] bitwise;
//                  plan_seeds again writes next = -1 at the targets.
//   plan_walk      one wave per frame: chases `next` from the start through a 32 x 32 window of it held in LDS (reloaded when the route
//                  leaves it: ~1 global round trip per >= 16 steps instead of one per step), then its 64 lanes write the directions.
//   One read-back of n x 2 words (length, status) and one wait.
// scene_tour.hip (yh_scene_plan_tour) runs the same solver and the same device functions (scene_path_dev.h) over K single-target fields.
// Connectivity 8 searches the 8-connected grid (DESIGN.md §11 "Diagonals"): the solver relaxes over the diagonal terms too
// and wakes the diagonally adjacent tile when a corner cell drops, plan_next<8> orders (left, right, up, down, up-left, up-right,
// down-left, down-right), and the walk's rotations are pi, 3 pi / 4, pi / 2, pi / 4. The <4> forms are the code described above.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "scene.h"
#include "scene_batch.h"
#include "scene_path_dev.h"
#include "yh_internal.h"

using namespace yh;

struct yh_scene_path : PlanFrames {   // all [max_frames][...]; nodes and dirs [max][W*H], walk_out [max][2]
    float* cost = nullptr;        // [max][H][W]
    int32_t* next = nullptr;      // [max][H][W]
    int32_t* host_walk = nullptr; // pinned [max][2]
    std::vector<int32_t> last_starts;   // per frame: linear index, -1: no plan for this frame
};

namespace {

// seeds [n][2] (pixel, frame): cost = 0 there, or (mark) next = -1 there
__global__ __launch_bounds__(256) void plan_seeds(const PathParams p, const int32_t* seeds, int n, int mark) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const size_t i = (size_t)seeds[2 * k + 1] * p.W * p.H + seeds[2 * k];
    if (mark) p.next[i] = -1;
    else p.cost[i] = 0.0f;
}

// frame b of the plan: cost advances by W H, and so does next
__device__ __forceinline__ PathParams plan_frame_of(const PathParams& p, int b) {
    PathParams q = frame_of(p, b, (size_t)p.W * p.H);
    q.next += (size_t)b * p.W * p.H;
    return q;
}

template <int CONN>
__global__ __launch_bounds__(SP_NT) void plan_round(const PathParams p, int F, int parity, uint32_t* cnt_next) {
    const int b = blockIdx.z;
    const PathParams q = plan_frame_of(p, b);
    relax_tile<CONN>(q, q.cost, p.flags + (size_t)(parity * F + b) * p.ntiles, p.flags + (size_t)((parity ^ 1) * F + b) * p.ntiles, cnt_next);
}

template <int CONN>
__global__ __launch_bounds__(256) void plan_next(const PathParams p, const int32_t* starts) {
    if (starts[blockIdx.z] < 0) return;
    next_body<CONN>(plan_frame_of(p, blockIdx.z));
}

__global__ __launch_bounds__(64) void plan_walk(const PathParams p, const int32_t* starts, int2* nodes, float2* dirs, int32_t* out) {
    const int b = blockIdx.z, start = starts[b];
    if (start < 0) return;   // (workgroup-uniform)
    const size_t npx = (size_t)p.W * p.H;
    walk_body(plan_frame_of(p, b), start, nodes + b * npx, dirs + b * npx, out + 2 * b);
}

// the planner's buffers, for the handle's max_frames frames, at the first plan: a handle that never plans pays nothing
int ensure_planner(yh_scene* h) {
    if (h->path) return YH_OK;
    yh_scene_path* q = h->path = new yh_scene_path();
    const size_t mf = (size_t)h->max_frames, all = mf * h->W * h->H;
    SCHK(h, hipMalloc((void**)&q->cost, all * 4));
    SCHK(h, hipMalloc((void**)&q->next, all * 4));
    SCHK(h, hipMalloc((void**)&q->nodes, all * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&q->dirs, all * sizeof(float2)));
    SCHK(h, hipMalloc((void**)&q->walk_out, mf * 2 * 4));
    SCHK(h, hipHostMalloc((void**)&q->host_walk, mf * 2 * 4, hipHostMallocDefault));
    return YH_OK;
}

// the whole plan of q->n frames on the handle's stream: last_seeds / last_field (pixel and frame of every target), last_starts. Returns
// when every route's length is known (the batches' counter reads are host waits anyway).
int run_plan(yh_scene* h, int conn) {
    yh_scene_path* q = h->path;
    const int n = q->n, ns = (int)q->last_seeds.size();
    int rc = plan_inputs_reserve(h, q->in, 2 * (size_t)ns + h->max_frames);
    if (rc) return rc;
    const size_t ws = plan_inputs_seeds(*q);
    std::copy(q->last_starts.begin(), q->last_starts.end(), q->in.host + ws);
    SCHK(h, hipMemcpyAsync(q->in.dev, q->in.host, (ws + n) * 4, hipMemcpyHostToDevice, h->stream));
    const int32_t *seeds = q->in.dev, *starts = q->in.dev + ws;
    PathParams p;
    if ((rc = solve_begin(h, conn, h->max_frames, n, p))) return rc;
    p.cost = q->cost; p.next = q->next;
    const size_t npx = (size_t)h->W * h->H;
    const dim3 px((unsigned)((npx + 255) / 256), 1, (unsigned)n), sd((unsigned)((ns + 255) / 256));
    SCHK(h, hipMemsetD32Async((hipDeviceptr_t)q->cost, 0x7f800000, n * npx, h->stream));   // +inf
    hipLaunchKernelGGL(plan_seeds, sd, dim3(256), 0, h->stream, p, seeds, ns, 0);
    const SolveRound round{ [&](const dim3& tiles, int parity, uint32_t* cnt_next) {
        hipLaunchKernelGGL(conn == 8 ? plan_round<8> : plan_round<4>, tiles, dim3(SP_NT), 0, h->stream, p, n, parity, cnt_next);
    }, 1 };
    if ((rc = solve_rounds(h, p, conn, n, q->last_seeds, h->batch ? "batch" : "path", 0, nullptr, &round, &q->last_field))) return rc;
    hipLaunchKernelGGL(conn == 8 ? plan_next<8> : plan_next<4>, px, dim3(256), 0, h->stream, p, starts);
    hipLaunchKernelGGL(plan_seeds, sd, dim3(256), 0, h->stream, p, seeds, ns, 1);
    hipLaunchKernelGGL(plan_walk, dim3(1, 1, (unsigned)n), dim3(64), 0, h->stream, p, starts, q->nodes, q->dirs, q->walk_out);
    SCHK(h, hipGetLastError());
    SCHK(h, hipMemcpyAsync(q->host_walk, q->walk_out, (size_t)n * 2 * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    q->path_len.assign(n, 0);
    for (int b = 0; b < n; ++b) {
        if (q->last_starts[b] < 0) continue;
        if (q->host_walk[2 * b + 1]) return h->fail(YH_EHIP, h->frame_tag(b) + "path walk: no target within W*H steps (fields not those of a SANE frame?)");
        q->path_len[b] = q->host_walk[2 * b];
    }
    return YH_OK;
}

// the inputs of a call are in h->path: run it, and it is the handle's last plan
int plan_now(yh_scene* h, int conn) {
    yh_scene_path* q = h->path;
    q->last.planned = false;
    const int rc = run_plan(h, conn);
    if (rc) return rc;
    q->last.conn = conn; q->last.planned = true; q->last.frame = h->frames;
    return YH_OK;
}

int plan_read(yh_scene* h, int frame, float* cost, int32_t* next, int32_t* path_xy, float* directions, int32_t path_capacity, int32_t* path_len) {
    const yh_scene_path* q = h->path;
    const size_t npx = (size_t)h->W * h->H, o = frame * npx;
    SolveLast one;
    const int rc = solve_frame(h, q, frame, npx, "plan", one);
    if (rc) return rc;
    return solve_read(h, "plan", "plan again", &one, { { cost, q ? q->cost + o : nullptr, npx * 4 }, { next, q ? q->next + o : nullptr, npx * 4 } },
                      path_xy, directions, path_capacity, path_len);
}

int plan_time(yh_scene* h, int32_t reps, float* ms, int32_t* rounds, int32_t* tile_runs) {
    yh_scene_path* q = h->path;
    // (a failed replay has overwritten part of the last plan: it is gone)
    auto run = [&] { const int rc = run_plan(h, q->last.conn); if (rc) q->last.planned = false; return rc; };
    return solve_time(h, "plan", "plan again", q ? &q->last : nullptr, reps, run, ms, rounds, tile_runs);
}

}  // namespace

namespace yh {
// What every plan checks of the frame and the start before it touches anything (yh_scene_plan, yh_scene_plan_tour, yh_scene_batch_plan)
int scene_plan_checks(yh_scene* h, int32_t n_targets, int32_t start_x, int32_t start_y) {
    if (n_targets < 1) return h->fail(YH_EINVAL, "n_targets < 1");
    if (!h->ran) return h->fail(YH_ESTATE, "no frame has been appended");
    if (h->last_mode != YH_COMPAT_SANE)
        return h->fail(YH_ESTATE, "the last frame was appended in YH_COMPAT_STRICT: its connections are all distances to world(0,0) "
                                  "(pt_cloud_weights.comp:32), no planner is defined on them; append in YH_COMPAT_SANE");
    const long long W = h->W, H = h->H;
    if ((W + H) * (2 * std::max(H, 101LL) + 1) >= (1LL << 24))
        return h->fail(YH_EINVAL, "frame too large for the planner: (W + H) * (2 * max(H, 101) + 1) must stay below 2^24 (f32 costs stay exact steps apart)");
    if (start_x < 0 || start_x >= W || start_y < 0 || start_y >= H) return h->fail(YH_EINVAL, "start outside the frame");
    return YH_OK;
}

// The targets a plan runs on, as linear indices: the given pixels, or (targets_xy null) the first n_targets balls of `balls` that have pixels
int scene_plan_choose(yh_scene* h, const int32_t* targets_xy, int32_t n_targets, const float (*balls)[4], std::vector<int32_t>& targets) {
    const long long W = h->W, H = h->H;
    targets.clear();
    if (targets_xy) {
        for (int k = 0; k < n_targets; ++k) {
            const int x = targets_xy[2 * k], y = targets_xy[2 * k + 1];
            if (x < 0 || x >= W || y < 0 || y >= H) return h->fail(YH_EINVAL, "target " + std::to_string(k) + " outside the frame");
            targets.push_back((int32_t)(y * W + x));
        }
    } else {
        // balls[..3] (path.rs:37), means truncated as `as i32` does (scene.rs:321); here: the first n_targets balls that have pixels
        int taken = 0;
        for (int k = 0; k < 100 && taken < n_targets; ++k) {
            if (!(balls[k][2] > 0.0f)) continue;
            ++taken;
            const int x = (int)balls[k][0], y = (int)balls[k][1];
            if (x >= 0 && x < W && y >= 0 && y < H) targets.push_back((int32_t)(y * W + x));
        }
        if (targets.empty()) return h->fail(YH_ESTATE, "no target given and the frame has no ball inside it");
    }
    return YH_OK;
}

// What yh_scene_plan and yh_scene_plan_tour check before they touch anything, and the targets they run on (linear indices)
int scene_plan_targets(yh_scene* h, const int32_t* targets_xy, int32_t n_targets, int32_t start_x, int32_t start_y, std::vector<int32_t>& targets) {
    const int rc = scene_plan_checks(h, n_targets, start_x, start_y);
    if (rc) return rc;
    SCHK(h, hipSetDevice(h->dev));
    float balls[100][4];
    if (!targets_xy) {
        SCHK(h, hipMemcpyAsync(balls, h->balls, sizeof(balls), hipMemcpyDeviceToHost, h->stream));
        SCHK(h, hipStreamSynchronize(h->stream));
    }
    return scene_plan_choose(h, targets_xy, n_targets, balls, targets);
}

// yh_scene_set_fields' host-side check of uploaded fields (also yh_scene_batch_set_fields'): YH_EINVAL unless the straight lengths are
// those of a SANE frame; diag_ok / diag_why: whether an 8-connected plan may read the diagonals
int scene_check_fields(yh_scene* h, const float* conn0, const float* conn1, bool& diag_ok, std::string& diag_why) {
    // what the planner assumes of SANE fields and the frozen definition reads from the other end: every in-frame length >= 1
    // (a finite number), left == the left neighbour's right, up == the upper neighbour's down
    for (int y = 0; y < h->H; ++y)
        for (int x = 0; x < h->W; ++x) {
            const size_t i = (size_t)y * h->W + x;
            const bool okr = x + 1 >= h->W || (conn0[4 * i + 2] >= 1.0f && conn0[4 * i + 2] < 3.0e38f && conn0[4 * i + 2] == conn1[4 * (i + 1) + 2]);
            const bool okd = y + 1 >= h->H || (conn1[4 * i] >= 1.0f && conn1[4 * i] < 3.0e38f && conn1[4 * i] == conn0[4 * (i + h->W)]);
            if (!okr || !okd)
                return h->fail(YH_EINVAL, "fields are not those of a SANE frame at pixel (" + std::to_string(x) + ", " + std::to_string(y) + "): the " +
                                              (okr ? "down" : "right") + " length must be a finite number >= 1 and equal the neighbour's entry for the same edge");
        }
    // the diagonals are no reason to refuse: what is recorded is whether an 8-connected plan may read them the same way (the
    // down-right and down-left entry of the upper pixel for both directions)
    diag_ok = true;
    diag_why.clear();
    for (int y = 0; y + 1 < h->H && diag_ok; ++y)
        for (int x = 0; x < h->W && diag_ok; ++x) {
            const size_t i = (size_t)y * h->W + x;
            const bool okr = x + 1 >= h->W || (conn0[4 * i + 3] >= 1.0f && conn0[4 * i + 3] < 3.0e38f && conn0[4 * i + 3] == conn1[4 * (i + h->W + 1) + 3]);
            const bool okl = x < 1 || (conn1[4 * i + 1] >= 1.0f && conn1[4 * i + 1] < 3.0e38f && conn1[4 * i + 1] == conn0[4 * (i + h->W - 1) + 1]);
            if (!okr || !okl) {
                diag_ok = false;
                diag_why = std::string("the down-") + (okr ? "left" : "right") + " length of pixel (" + std::to_string(x) + ", " + std::to_string(y) +
                           ") is not a finite number >= 1 equal to the other end's entry for the same edge";
            }
        }
    return YH_OK;
}

int scene_plan_diagonals(yh_scene* h, bool ok, const std::string& why) {
    if (ok) return YH_OK;
    return h->fail(YH_ESTATE, "the uploaded fields allow 4-connected plans only: " + why);
}

int scene_turn_heading(yh_scene* h, int32_t heading) {
    if (heading >= 0 && heading <= 7) return YH_OK;
    return h->fail(YH_EINVAL, "start heading " + std::to_string(heading) + ": 0 .. 7 (0 right, clockwise on the image, 6 up)");
}

int scene_turn_price(yh_scene* h, float turn_price) {
    if (std::isfinite(turn_price) && turn_price >= 1.0f && turn_price <= 1024.0f) return YH_OK;
    return h->fail(YH_EINVAL, "turn price must be a finite number in [1, 1024] (every weight >= 1 is what makes the field unique)");
}

int scene_turn_size(yh_scene* h) {
    const long long W = h->W, H = h->H;
    if ((W + H) * (2 * std::max(H, 101LL) + 1) + 8 * 1024 < (1LL << 24)) return YH_OK;
    return h->fail(YH_EINVAL, "frame too large for the turn planner: (W + H) * (2 * max(H, 101) + 1) + 8 * 1024 must stay below 2^24");
}

void scene_path_free(yh_scene* h) {
    yh_scene_path* q = h->path;
    if (!q) return;
    void* bufs[] = { q->cost, q->next, q->nodes, q->dirs, q->walk_out };
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (q->host_walk) (void)hipHostFree(q->host_walk);
    plan_inputs_free(q->in);
    delete q;
    h->path = nullptr;
}
}  // namespace yh

extern "C" {

int yh_scene_plan(yh_scene* h, const int32_t* targets_xy, int32_t n_targets, int32_t start_x, int32_t start_y) {
    return yh_scene_plan_conn(h, targets_xy, n_targets, start_x, start_y, 4);
}

int yh_scene_plan_conn(yh_scene* h, const int32_t* targets_xy, int32_t n_targets, int32_t start_x, int32_t start_y, int32_t connectivity) {
    if (!h) return YH_EINVAL;
    if (connectivity != 4 && connectivity != 8) return h->fail(YH_EINVAL, "connectivity " + std::to_string(connectivity) + ": 4 or 8");
    std::vector<int32_t> targets;
    int rc = scene_plan_targets(h, targets_xy, n_targets, start_x, start_y, targets);
    if (rc) return rc;
    if (connectivity == 8 && (rc = scene_plan_diagonals(h, h->diag_ok, h->diag_why))) return rc;
    if ((rc = ensure_planner(h))) { scene_path_free(h); return rc; }
    yh_scene_path* q = h->path;   // the batch of one: every seed in frame 0, one start
    q->n = 1; q->status.assign(1, YH_OK); q->last_starts.assign(1, start_y * h->W + start_x);
    q->last_field.assign(targets.size(), 0); q->last_seeds = std::move(targets);
    return plan_now(h, connectivity);
}

int yh_scene_batch_plan(yh_scene_batch* hb, const int32_t* targets_xy, int32_t n_targets, const int32_t* starts_xy, int32_t connectivity, int32_t* status) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (connectivity != 4 && connectivity != 8) return h->fail(YH_EINVAL, "connectivity " + std::to_string(connectivity) + ": 4 or 8");
    if (!starts_xy) return h->fail(YH_EINVAL, "starts_xy is null");
    std::vector<int32_t> seeds, field, starts(hb->n, -1), st;
    int rc = scene_batch_frames(hb, targets_xy, n_targets, starts_xy, nullptr, connectivity, st, [&](int b, const std::vector<int32_t>& t) {
        starts[b] = starts_xy[2 * b + 1] * h->W + starts_xy[2 * b];
        for (int32_t v : t) { seeds.push_back(v); field.push_back(b); }
        return YH_OK;
    });
    if (rc) return rc;
    if (status) std::copy(st.begin(), st.end(), status);
    if (seeds.empty()) return h->fail(YH_ESTATE, "no target given and no frame of the batch has a ball inside it");
    h->err.clear();
    if ((rc = ensure_planner(h))) { scene_path_free(h); return rc; }
    yh_scene_path* q = h->path;
    q->n = hb->n; q->status = st; q->last_starts = starts; q->last_seeds = seeds; q->last_field = field;
    return plan_now(h, connectivity);
}

int yh_scene_plan_read(yh_scene* h, float* cost, int32_t* next, int32_t* path_xy, float* directions, int32_t path_capacity, int32_t* path_len) {
    if (!h) return YH_EINVAL;
    return plan_read(h, 0, cost, next, path_xy, directions, path_capacity, path_len);
}

int yh_scene_batch_plan_read(yh_scene_batch* hb, int32_t frame, float* cost, int32_t* next, int32_t* path_xy, float* directions, int32_t path_capacity, int32_t* path_len) {
    if (!hb) return YH_EINVAL;
    const int rc = hb->frame_ok(frame);
    if (rc) return rc;
    return plan_read(&hb->core, frame, cost, next, path_xy, directions, path_capacity, path_len);
}

int yh_scene_plan_time(yh_scene* h, int32_t reps, float* ms_per_plan, int32_t* rounds, int32_t* tile_runs) {
    if (!h || reps < 1 || !ms_per_plan) return YH_EINVAL;
    return plan_time(h, reps, ms_per_plan, rounds, tile_runs);
}

int yh_scene_batch_plan_time(yh_scene_batch* hb, int32_t reps, float* ms_per_batch, int32_t* rounds, int32_t* tile_runs) {
    if (!hb || reps < 1 || !ms_per_batch) return YH_EINVAL;
    return plan_time(&hb->core, reps, ms_per_batch, rounds, tile_runs);
}

int yh_scene_set_fields(yh_scene* h, const uint32_t* map, const float* conn0, const float* conn1) {
    if (!h || !map || !conn0 || !conn1) return YH_EINVAL;
    bool diag_ok = true;
    std::string diag_why;
    const int rc = scene_check_fields(h, conn0, conn1, diag_ok, diag_why);
    if (rc) return rc;
    SCHK(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)h->W * h->H;
    SCHK(h, hipMemcpyAsync(h->map, map, npx * 4, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipMemcpyAsync(h->conn0, conn0, npx * 16, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipMemcpyAsync(h->conn1, conn1, npx * 16, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipMemsetAsync(h->world, 0, npx * 16, h->stream));
    SCHK(h, hipMemsetAsync(h->balls, 0, 100 * 16, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    h->ran = true; h->last_mode = YH_COMPAT_SANE; h->last_cls = h->cls_id; h->last_frame = nullptr; h->last_frame_mode = 0;
    h->diag_ok = diag_ok; h->diag_why = diag_why;
    ++h->frames;
    return YH_OK;
}

}  // extern "C"
