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
//   path_weights   one lane per pixel: conn0 / conn1 / map -> one float4 per pixel (right length, right height step, down length,
//                  down height step): the solver reads 16 B per pixel instead of 32 B of connections + the map, length and step
//                  stay apart for the two roundings.
//   path_fill      cost = +inf, path_targets: cost = 0. The host flags round 0's tiles: each target's own tile, and the tile across
//                  every tile border the target lies on - a target's drop from +inf to 0 is a lowered border cell like any other,
//                  and a neighbour whose border sees nothing but targets (a wall of targets along a tile border) would otherwise
//                  never be flagged.
//   path_round     x rounds. A workgroup owns a SP_TW x SP_TH tile of the cost field with a one-cell halo in LDS; a lane owns a
//                  2 x 2 block of cells whose twelve edge terms sit in registers. It relaxes in place (chaotic relaxation: a lane
//                  reads its eight outer neighbours from LDS, sweeps its four cells forwards and backwards in registers, stores
//                  what got smaller) SP_INNER times between workgroup votes, until a vote finds nothing changed: the tile's local
//                  fixed point for the halo it loaded. Cells that changed go back with atomicMin on the u32 view (non-negative f32
//                  order as their bits). Only a tile whose halo may have changed runs: a tile that lowered a cell of its border
//                  flags that neighbour for the NEXT round (two flag arrays, by round parity) and counts it once. No workgroup
//                  ever waits for another one: a round is a launch, the host enqueues SP_BATCH of them and reads the batch's
//                  counters back once (rounds past convergence find no flag and exit at once).
//   path_next      one lane per pixel: the first neighbour in the order (left, right, up, down) whose candidate equals d[v] bitwise.
//   path_walk      one wave: chases `next` from the start through a 32 x 32 window of it held in LDS (reloaded when the route leaves
//                  it: ~1 global round trip per >= 16 steps instead of one per step), then its 64 lanes write the directions.
// The tile relaxation, the successor rule and the chase are device functions of scene_path_dev.h: scene_tour.hip (yh_scene_plan_tour)
// runs the same ones over K single-target fields.
// yh_scene_plan_conn(.., 8) searches the 8-connected grid (DESIGN.md §11 "Diagonals"): path_weights<8> also writes the down-right and
// down-left terms (a second float4 per pixel, allocated at the first such plan), path_round<8> relaxes over them and wakes the
// diagonally adjacent tile when a corner cell drops, path_next<8> orders (left, right, up, down, up-left, up-right, down-left,
// down-right), and the walk's rotations are pi, 3 pi / 4, pi / 2, pi / 4. The <4> forms are the code described above.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "scene.h"
#include "scene_path_dev.h"
#include "yh_internal.h"

using namespace yh;

struct yh_scene_path {
    float* cost = nullptr;       // [H][W]
    int32_t* next = nullptr;     // [H][W]
    float4* edge = nullptr;      // [H][W]: right length, right |dh|, down length, down |dh| (length -1 off the frame)
    float4* edge2 = nullptr;     // [H][W]: down-right length, |dh|, down-left length, |dh|; allocated at the first 8-connected plan
    uint32_t* flags = nullptr;   // [2][ntiles]
    uint32_t* cnt = nullptr;     // [SP_BATCH + 1]: cnt[j + 1] = tiles flagged by round j of the batch
    int32_t* targets = nullptr;  // [targets_cap] linear indices
    int32_t targets_cap = 0;
    int2* nodes = nullptr;       // [W * H] the route
    float2* dirs = nullptr;      // [W * H]
    int32_t* walk_out = nullptr; // [2]: length, status
    uint32_t* host = nullptr;    // pinned: SP_BATCH + 1 counters, then walk_out
    int tx = 0, ty = 0;
    // the last plan
    bool planned = false;
    uint64_t frame = 0;
    std::vector<int32_t> last_targets;
    std::vector<uint32_t> flags0;   // round 0's tile flags, built on the host
    int32_t start = 0, path_len = 0, conn = 4;
    long long rounds = 0, tile_runs = 0;
};

namespace {

template <int CONN>
__global__ __launch_bounds__(256) void path_weights(const PathParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.W * p.H) return;
    const int x = i % p.W, y = i / p.W;
    const float h = (float)p.map[i];
    const float hr = x + 1 < p.W ? fabsf(__fsub_rn(h, (float)p.map[i + 1])) : 0.0f;
    const float hd = y + 1 < p.H ? fabsf(__fsub_rn(h, (float)p.map[i + p.W])) : 0.0f;
    const float4 c0 = p.conn0[i], c1 = p.conn1[i];
    p.edge[i] = make_float4(x + 1 < p.W ? c0.z : -1.0f, hr, y + 1 < p.H ? c1.x : -1.0f, hd);
    if constexpr (CONN == 8) {
        const bool dr = x + 1 < p.W && y + 1 < p.H, dl = x > 0 && y + 1 < p.H;
        const float hdr = dr ? fabsf(__fsub_rn(h, (float)p.map[i + p.W + 1])) : 0.0f;
        const float hdl = dl ? fabsf(__fsub_rn(h, (float)p.map[i + p.W - 1])) : 0.0f;
        p.edge2[i] = make_float4(dr ? c0.w : -1.0f, hdr, dl ? c1.y : -1.0f, hdl);
    }
}

__global__ __launch_bounds__(256) void path_fill(const PathParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < p.W * p.H) p.cost[i] = SP_INF;
    if (i < 2 * p.ntiles) p.flags[i] = 0u;
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
__global__ __launch_bounds__(SP_NT) void path_round(const PathParams p, int parity, uint32_t* cnt_next) {
    relax_tile<CONN>(p, p.cost, p.flags + parity * p.ntiles, p.flags + (parity ^ 1) * p.ntiles, cnt_next);
}

template <int CONN>
__global__ __launch_bounds__(256) void path_next(const PathParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < p.W * p.H) p.next[i] = successor(around<CONN>(p, i), p.cost, i);
}

// out[0] = nodes on the route (start and target included), out[1] = 0, or 1 if the walk did not end within W * H nodes (costs
// strictly decrease along `next`, so this cannot happen on SANE fields; the bound is what keeps the loop finite on any input)
__global__ __launch_bounds__(64) void path_walk(const PathParams p, int start, int2* nodes, float2* dirs, int32_t* out) {
    const int lane = threadIdx.x;
    bool lost;
    const int n = chase(p.next, p.W, p.H, start, nodes, lost);
    // directions[i] = (d[n_i] - d[n_i+1], rot_i): rot_0 = 0, else the angle at n_i between n_i-1 and n_i+1 - on a 4-grid without
    // backtracking pi when straight, pi / 2 for a turn; with diagonals 3 pi / 4 and pi / 4 too (constants, not a device acosf)
    for (int i = lane; i + 1 < n; i += 64) {
        const int2 a = nodes[i], b = nodes[i + 1];
        const float mag = __fsub_rn(p.cost[(size_t)a.y * p.W + a.x], p.cost[(size_t)b.y * p.W + b.x]);
        dirs[i] = make_float2(mag, i > 0 ? rotation(nodes[i - 1], a, b) : 0.0f);
    }
    if (lane == 0) { out[0] = n; out[1] = lost ? 1 : 0; }
}

int ensure_buffers(yh_scene* h) {
    yh_scene_path* q = h->path;
    const size_t npx = (size_t)h->W * h->H;
    q->tx = (h->W + SP_TW - 1) / SP_TW; q->ty = (h->H + SP_TH - 1) / SP_TH;
    SCHK(h, hipMalloc((void**)&q->cost, npx * 4));
    SCHK(h, hipMalloc((void**)&q->next, npx * 4));
    SCHK(h, hipMalloc((void**)&q->edge, npx * 16));
    SCHK(h, hipMalloc((void**)&q->flags, (size_t)2 * q->tx * q->ty * 4));
    SCHK(h, hipMalloc((void**)&q->cnt, (SP_BATCH + 1) * 4));
    SCHK(h, hipMalloc((void**)&q->nodes, npx * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&q->dirs, npx * sizeof(float2)));
    SCHK(h, hipMalloc((void**)&q->walk_out, 2 * 4));
    SCHK(h, hipHostMalloc((void**)&q->host, (SP_BATCH + 3) * 4, hipHostMallocDefault));
    return YH_OK;
}

// the whole plan on the handle's stream; returns when the route's length is known (the batches' counter reads are host waits anyway)
int run_plan(yh_scene* h, const std::vector<int32_t>& targets, int32_t start, int conn) {
    yh_scene_path* q = h->path;
    const int n = (int)targets.size();
    if (conn == 8 && !q->edge2) SCHK(h, hipMalloc((void**)&q->edge2, (size_t)h->W * h->H * 16));
    if (n > q->targets_cap) {
        if (q->targets) { SCHK(h, hipStreamSynchronize(h->stream)); SCHK(h, hipFree(q->targets)); q->targets = nullptr; q->targets_cap = 0; }
        SCHK(h, hipMalloc((void**)&q->targets, (size_t)n * 4));
        q->targets_cap = n;
    }
    PathParams p;
    p.W = h->W; p.H = h->H; p.tx = q->tx; p.ntiles = q->tx * q->ty;
    p.map = h->map; p.conn0 = h->conn0; p.conn1 = h->conn1; p.edge = q->edge; p.edge2 = conn == 8 ? q->edge2 : nullptr; p.cost = q->cost; p.next = q->next; p.flags = q->flags;
    const int npx = h->W * h->H;
    const dim3 px((unsigned)((std::max(npx, 2 * p.ntiles) + 255) / 256)), tg((unsigned)((n + 255) / 256)), tiles((unsigned)q->tx, (unsigned)q->ty);
    SCHK(h, hipMemcpyAsync(q->targets, targets.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    path_weights_launch(p, conn, h->stream);
    hipLaunchKernelGGL(path_fill, px, dim3(256), 0, h->stream, p);
    hipLaunchKernelGGL(path_targets, tg, dim3(256), 0, h->stream, p, q->targets, n);
    // round 0's work list (flag array 0): the rule path_round applies to every later decrease - a lowered cell on a tile's border
    // flags the tile across that border, and with diagonals a lowered corner cell the tile diagonally across - applied to the
    // targets' drop from +inf to 0, plus the targets' own tiles
    q->flags0.assign((size_t)p.ntiles, 0u);
    long long active = 0;
    auto flag = [&](int bx, int by) {
        if (bx < 0 || bx >= q->tx || by < 0 || by >= q->ty) return;
        uint32_t& f = q->flags0[(size_t)by * q->tx + bx];
        if (!f) { f = 1u; ++active; }
    };
    for (int t : targets) round0_flags(t % h->W, t / h->W, conn, flag);
    SCHK(h, hipMemcpyAsync(q->flags, q->flags0.data(), (size_t)p.ntiles * 4, hipMemcpyHostToDevice, h->stream));
    q->rounds = 0; q->tile_runs = 0;
    const long long cap = (long long)npx;   // costs only decrease over a finite set: this never fires
    long long round = 0;
    while (active) {
        if (round >= cap) return h->fail(YH_EHIP, "path solver: round cap W*H reached without convergence (fields not those of a SANE frame?)");
        SCHK(h, hipMemsetAsync(q->cnt, 0, (SP_BATCH + 1) * 4, h->stream));
        for (int j = 0; j < SP_BATCH; ++j, ++round)
            hipLaunchKernelGGL(conn == 8 ? path_round<8> : path_round<4>, tiles, dim3(SP_NT), 0, h->stream, p, (int)(round & 1), q->cnt + j + 1);
        SCHK(h, hipGetLastError());
        SCHK(h, hipMemcpyAsync(q->host, q->cnt, (SP_BATCH + 1) * 4, hipMemcpyDeviceToHost, h->stream));
        SCHK(h, hipStreamSynchronize(h->stream));
        q->host[0] = (uint32_t)active;   // tiles that ran in round j of the batch: host[j]
        for (int j = 0; j < SP_BATCH; ++j) if (q->host[j]) { ++q->rounds; q->tile_runs += q->host[j]; }
        active = q->host[SP_BATCH];
    }
    hipLaunchKernelGGL(conn == 8 ? path_next<8> : path_next<4>, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, h->stream, p);
    hipLaunchKernelGGL(path_mark_targets, tg, dim3(256), 0, h->stream, p, q->targets, n);
    hipLaunchKernelGGL(path_walk, dim3(1), dim3(64), 0, h->stream, p, (int)start, q->nodes, q->dirs, q->walk_out);
    SCHK(h, hipGetLastError());
    int32_t* wo = reinterpret_cast<int32_t*>(q->host + SP_BATCH + 1);
    SCHK(h, hipMemcpyAsync(wo, q->walk_out, 2 * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    if (wo[1]) return h->fail(YH_EHIP, "path walk: no target within W*H steps (fields not those of a SANE frame?)");
    q->path_len = wo[0];
    return YH_OK;
}

}  // namespace

namespace yh {
void path_weights_launch(const PathParams& p, int conn, hipStream_t s) {
    hipLaunchKernelGGL(conn == 8 ? path_weights<8> : path_weights<4>, dim3((unsigned)((p.W * p.H + 255) / 256)), dim3(256), 0, s, p);
}

// What yh_scene_plan and yh_scene_plan_tour check before they touch anything, and the targets they run on (linear indices)
int scene_plan_targets(yh_scene* h, const int32_t* targets_xy, int32_t n_targets, int32_t start_x, int32_t start_y, std::vector<int32_t>& targets) {
    if (n_targets < 1) return h->fail(YH_EINVAL, "n_targets < 1");
    if (!h->ran) return h->fail(YH_ESTATE, "no frame has been appended");
    if (h->last_mode != YH_COMPAT_SANE)
        return h->fail(YH_ESTATE, "the last frame was appended in YH_COMPAT_STRICT: its connections are all distances to world(0,0) "
                                  "(pt_cloud_weights.comp:32), no planner is defined on them; append in YH_COMPAT_SANE");
    const long long W = h->W, H = h->H;
    if ((W + H) * (2 * std::max(H, 101LL) + 1) >= (1LL << 24))
        return h->fail(YH_EINVAL, "frame too large for the planner: (W + H) * (2 * max(H, 101) + 1) must stay below 2^24 (f32 costs stay exact steps apart)");
    if (start_x < 0 || start_x >= W || start_y < 0 || start_y >= H) return h->fail(YH_EINVAL, "start outside the frame");
    SCHK(h, hipSetDevice(h->dev));
    targets.clear();
    if (targets_xy) {
        for (int k = 0; k < n_targets; ++k) {
            const int x = targets_xy[2 * k], y = targets_xy[2 * k + 1];
            if (x < 0 || x >= W || y < 0 || y >= H) return h->fail(YH_EINVAL, "target " + std::to_string(k) + " outside the frame");
            targets.push_back((int32_t)(y * W + x));
        }
    } else {
        // balls[..3] (path.rs:37), means truncated as `as i32` does (scene.rs:321); here: the first n_targets balls that have pixels
        float balls[100][4];
        SCHK(h, hipMemcpyAsync(balls, h->balls, sizeof(balls), hipMemcpyDeviceToHost, h->stream));
        SCHK(h, hipStreamSynchronize(h->stream));
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

int scene_plan_diagonals(yh_scene* h) {
    if (h->diag_ok) return YH_OK;
    return h->fail(YH_ESTATE, "the uploaded fields allow 4-connected plans only: " + h->diag_why);
}

void scene_path_free(yh_scene* h) {
    yh_scene_path* q = h->path;
    if (!q) return;
    void* bufs[] = { q->cost, q->next, q->edge, q->edge2, q->flags, q->cnt, q->targets, q->nodes, q->dirs, q->walk_out };
    for (void* b : bufs) if (b) hipFree(b);
    if (q->host) hipHostFree(q->host);
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
    yh_scene_path* q = h->path;
    if (!q || !q->planned) return h->fail(YH_ESTATE, "no plan has been made");
    if (q->frame != h->frames) return h->fail(YH_ESTATE, "a newer frame has been appended since the plan: plan again");
    if (path_len) *path_len = q->path_len;
    if ((path_xy || directions) && path_capacity < q->path_len)
        return h->fail(YH_EOVERFLOW, "path_capacity " + std::to_string(path_capacity) + " < the route's " + std::to_string(q->path_len) + " nodes");
    SCHK(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)h->W * h->H;
    if (cost) SCHK(h, hipMemcpyAsync(cost, q->cost, npx * 4, hipMemcpyDeviceToHost, h->stream));
    if (next) SCHK(h, hipMemcpyAsync(next, q->next, npx * 4, hipMemcpyDeviceToHost, h->stream));
    if (path_xy) SCHK(h, hipMemcpyAsync(path_xy, q->nodes, (size_t)q->path_len * sizeof(int2), hipMemcpyDeviceToHost, h->stream));
    if (directions && q->path_len > 1) SCHK(h, hipMemcpyAsync(directions, q->dirs, (size_t)(q->path_len - 1) * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    return YH_OK;
}

int yh_scene_set_fields(yh_scene* h, const uint32_t* map, const float* conn0, const float* conn1) {
    if (!h || !map || !conn0 || !conn1) return YH_EINVAL;
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
    bool diag_ok = true;
    std::string diag_why;
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
    if (!q || !q->planned) return h->fail(YH_ESTATE, "no plan has been made");
    if (q->frame != h->frames) return h->fail(YH_ESTATE, "a newer frame has been appended since the plan: plan again");
    SCHK(h, hipSetDevice(h->dev));
    hipEvent_t a, b;
    SCHK(h, hipEventCreate(&a)); SCHK(h, hipEventCreate(&b));
    SCHK(h, hipEventRecord(a, h->stream));
    for (int r = 0; r < reps; ++r) { const int rc = run_plan(h, q->last_targets, q->start, q->conn); if (rc) { hipEventDestroy(a); hipEventDestroy(b); return rc; } }
    SCHK(h, hipEventRecord(b, h->stream));
    SCHK(h, hipEventSynchronize(b));
    float ms = 0;
    hipEventElapsedTime(&ms, a, b);
    hipEventDestroy(a); hipEventDestroy(b);
    *ms_per_plan = ms / reps;   // (the host's waits for the batches' counters are inside: what a caller of yh_scene_plan waits for)
    if (rounds) *rounds = (int32_t)q->rounds;
    if (tile_runs) *tile_runs = (int32_t)q->tile_runs;
    return YH_OK;
}

}  // extern "C"
