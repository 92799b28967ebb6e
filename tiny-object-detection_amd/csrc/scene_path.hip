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
// Launches of one plan (yh_scene_plan):
//   path_weights, then after path_fill (cost = +inf) and path_targets (cost = 0) field_round x rounds: scene_solve.hip's, which
//                  relaxes the one field tile by tile to its fixed point, the targets its seeds.
//   path_next      one lane per pixel: the first neighbour in the order (left, right, up, down) whose candidate equals d[v] bitwise.
//   path_walk      one wave: chases `next` from the start through a 32 x 32 window of it held in LDS (reloaded when the route leaves
//                  it: ~1 global round trip per >= 16 steps instead of one per step), then its 64 lanes write the directions.
// scene_tour.hip (yh_scene_plan_tour) runs the same solver and the same device functions (scene_path_dev.h) over K single-target fields.
// yh_scene_plan_conn(.., 8) searches the 8-connected grid (DESIGN.md §11 "Diagonals"): the solver relaxes over the diagonal terms too
// and wakes the diagonally adjacent tile when a corner cell drops, path_next<8> orders (left, right, up, down, up-left, up-right,
// down-left, down-right), and the walk's rotations are pi, 3 pi / 4, pi / 2, pi / 4. The <4> forms are the code described above.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "scene.h"
#include "scene_path_dev.h"
#include "yh_internal.h"

using namespace yh;

struct yh_scene_path : SolveLast {   // (the route, the start, the connectivity and whether a plan exists: SolveLast)
    float* cost = nullptr;       // [H][W]
    int32_t* next = nullptr;     // [H][W]
    int32_t* targets = nullptr;  // [targets_cap] linear indices
    int32_t targets_cap = 0;
    int32_t* walk_out = nullptr; // [2]: length, status
    std::vector<int32_t> last_targets;
};

namespace {

__global__ __launch_bounds__(256) void path_fill(const PathParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < p.W * p.H) p.cost[i] = SP_INF;
}

__global__ __launch_bounds__(256) void path_targets(const PathParams p, const int32_t* targets, int n) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    p.cost[targets[k]] = 0.0f;
}

__global__ __launch_bounds__(256) void path_mark_targets(const PathParams p, const int32_t* targets, int n) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) p.next[targets[k]] = -1;
}

template <int CONN>
__global__ __launch_bounds__(256) void path_next(const PathParams p) { next_body<CONN>(p); }

__global__ __launch_bounds__(64) void path_walk(const PathParams p, int start, int2* nodes, float2* dirs, int32_t* out) { walk_body(p, start, nodes, dirs, out); }

int ensure_buffers(yh_scene* h) {
    yh_scene_path* q = h->path;
    const size_t npx = (size_t)h->W * h->H;
    SCHK(h, hipMalloc((void**)&q->cost, npx * 4));
    SCHK(h, hipMalloc((void**)&q->next, npx * 4));
    SCHK(h, hipMalloc((void**)&q->nodes, npx * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&q->dirs, npx * sizeof(float2)));
    SCHK(h, hipMalloc((void**)&q->walk_out, 2 * 4));
    return YH_OK;
}

// the whole plan on the handle's stream; returns when the route's length is known (the batches' counter reads are host waits anyway)
int run_plan(yh_scene* h, const std::vector<int32_t>& targets, int32_t start, int conn) {
    yh_scene_path* q = h->path;
    const int n = (int)targets.size();
    if (n > q->targets_cap) {
        if (q->targets) { SCHK(h, hipStreamSynchronize(h->stream)); SCHK(h, hipFree(q->targets)); q->targets = nullptr; q->targets_cap = 0; }
        SCHK(h, hipMalloc((void**)&q->targets, (size_t)n * 4));
        q->targets_cap = n;
    }
    const int npx = h->W * h->H;
    const dim3 px((unsigned)((npx + 255) / 256)), tg((unsigned)((n + 255) / 256));
    SCHK(h, hipMemcpyAsync(q->targets, targets.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    PathParams p;
    int rc = solve_begin(h, conn, 1, p);
    if (rc) return rc;
    p.cost = q->cost; p.next = q->next;
    hipLaunchKernelGGL(path_fill, px, dim3(256), 0, h->stream, p);
    hipLaunchKernelGGL(path_targets, tg, dim3(256), 0, h->stream, p, q->targets, n);
    if ((rc = solve_rounds(h, p, conn, 1, targets, "path"))) return rc;
    hipLaunchKernelGGL(conn == 8 ? path_next<8> : path_next<4>, px, dim3(256), 0, h->stream, p);
    hipLaunchKernelGGL(path_mark_targets, tg, dim3(256), 0, h->stream, p, q->targets, n);
    hipLaunchKernelGGL(path_walk, dim3(1), dim3(64), 0, h->stream, p, (int)start, q->nodes, q->dirs, q->walk_out);
    SCHK(h, hipGetLastError());
    int32_t* wo = reinterpret_cast<int32_t*>(h->solve->host + kSolveCnt + kSolveTail);
    SCHK(h, hipMemcpyAsync(wo, q->walk_out, 2 * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    if (wo[1]) return h->fail(YH_EHIP, "path walk: no target within W*H steps (fields not those of a SANE frame?)");
    q->path_len = wo[0];
    return YH_OK;
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

int scene_plan_diagonals(yh_scene* h) {
    if (h->diag_ok) return YH_OK;
    return h->fail(YH_ESTATE, "the uploaded fields allow 4-connected plans only: " + h->diag_why);
}

void scene_path_free(yh_scene* h) {
    yh_scene_path* q = h->path;
    if (!q) return;
    void* bufs[] = { q->cost, q->next, q->targets, q->nodes, q->dirs, q->walk_out };
    for (void* b : bufs) if (b) hipFree(b);
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
    if (connectivity == 8 && (rc = scene_plan_diagonals(h))) return rc;
    const long long W = h->W;
    if (!h->path) {   // the planner's buffers are allocated at the first plan: a handle that never plans pays nothing
        h->path = new yh_scene_path();
        rc = ensure_buffers(h);
        if (rc) { scene_path_free(h); return rc; }
    }
    h->path->planned = false;
    rc = run_plan(h, targets, (int32_t)(start_y * W + start_x), connectivity);
    if (rc) return rc;
    h->path->conn = connectivity;
    h->path->planned = true; h->path->frame = h->frames; h->path->last_targets = targets; h->path->start = (int32_t)(start_y * W + start_x);
    return YH_OK;
}

int yh_scene_plan_read(yh_scene* h, float* cost, int32_t* next, int32_t* path_xy, float* directions, int32_t path_capacity, int32_t* path_len) {
    if (!h) return YH_EINVAL;
    const yh_scene_path* q = h->path;
    const size_t bytes = (size_t)h->W * h->H * 4;
    return solve_read(h, "plan", "plan again", q, { { cost, q ? q->cost : nullptr, bytes }, { next, q ? q->next : nullptr, bytes } }, path_xy, directions, path_capacity, path_len);
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

int yh_scene_plan_time(yh_scene* h, int32_t reps, float* ms_per_plan, int32_t* rounds, int32_t* tile_runs) {
    if (!h || reps < 1 || !ms_per_plan) return YH_EINVAL;
    yh_scene_path* q = h->path;
    // (a failed replay has overwritten part of the last plan: it is gone)
    auto run = [&] { const int rc = run_plan(h, q->last_targets, q->start, q->conn); if (rc) q->planned = false; return rc; };
    return solve_time(h, "plan", "plan again", q, reps, run, ms_per_plan, rounds, tile_runs);
}

}  // extern "C"
