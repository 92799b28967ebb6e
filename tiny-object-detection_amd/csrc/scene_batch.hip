// scene_batch.hip — yh_scene_batch: the scene back-end and its planner over N frames in one set of launches (DESIGN.md §11 "Scene
// batch"). Frame b of a batch has exactly the results a yh_scene handle of the same size gives when it is fed that frame alone: every
// kernel here takes its frame from blockIdx.z, advances its own copy of the by-value parameter block by b frames and runs the body
// the single handle's kernel runs (scene_dev.h, scene_path_dev.h) - there is no second definition of anything. The planner's field is
// unique (scene_path.hip), so frames that share the solver's rounds cannot change each other's bits: a frame has its own cost field,
// edge terms and tile flags, the counters sum over the frames as they do over a tour's fields, and the batch takes the rounds of its
// slowest frame. A frame without a target (no usable ball) seeds nothing, flags nothing, and its walk is skipped (start -1).
//
// Launches of one append of n frames: two memsets (maps, ball sums), batch_cloud_strips (strips x bands x n), batch_balls (n blocks),
// batch_world, batch_conn1, batch_conn0 (8 x 8 pixels x n). Of one plan: batch_weights, a fill of the n cost fields, batch_seeds,
// batch_round x rounds (tiles x n; scene_solve.hip's host loop, ragged seeds), batch_next, batch_seeds again (next = -1 at the
// targets), batch_walk (one wave per frame).
//
// The handle holds a yh_scene as its core: device, size, stream, error text, bump tables, the frame generation and mode - and array
// pointers that are frame 0 of the batch's [max_frames][...] arrays. That is what lets the single handle's host code (the plan's checks
// and choice of targets, the fields check, the solver's loop, its read and time) run on a batch unchanged. The handle itself is
// scene_batch.h's; the turn-aware plan over the batch (yh_scene_batch_plan_turn) is scene_batch_turn.hip, the turn-aware tour
// (yh_scene_batch_plan_turn_tour) scene_batch_turn_tour.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "scene.h"
#include "scene_batch.h"
#include "scene_dev.h"
#include "scene_path_dev.h"
#include "yh_internal.h"

using namespace yh;

namespace {

__device__ __forceinline__ SceneParams frame_of(const SceneParams& p, int b) {
    SceneParams q = p;
    const size_t npx = (size_t)p.W * p.H;
    q.depth += b * npx; q.frame += b * npx; q.map += b * npx; q.world += b * npx; q.conn0 += b * npx; q.conn1 += b * npx;
    q.ball_acc += b * 300; q.balls += b * 100;
    return q;
}

__device__ __forceinline__ PathParams frame_of(const PathParams& p, int b) {
    PathParams q = p;
    const size_t npx = (size_t)p.W * p.H;
    q.map += b * npx; q.conn0 += b * npx; q.conn1 += b * npx; q.edge += b * npx; q.cost += b * npx; q.next += b * npx;
    if (q.edge2) q.edge2 += b * npx;
    return q;
}

__global__ __launch_bounds__(512) void batch_cloud_strips(const SceneParams p) { cloud_strips_body(frame_of(p, blockIdx.z)); }
__global__ void batch_balls(const SceneParams p) { balls_body(frame_of(p, blockIdx.z)); }
__global__ __launch_bounds__(64) void batch_world(const SceneParams p) { world_body(frame_of(p, blockIdx.z)); }
__global__ __launch_bounds__(64) void batch_conn1(const SceneParams p) { conn1_body(frame_of(p, blockIdx.z)); }
__global__ __launch_bounds__(64) void batch_conn0(const SceneParams p) { conn0_body(frame_of(p, blockIdx.z)); }

template <int CONN>
__global__ __launch_bounds__(256) void batch_weights(const PathParams p) { weights_body<CONN>(frame_of(p, blockIdx.z)); }

// seeds [n][2] (pixel, frame): cost = 0 there, or (mark) next = -1 there
__global__ __launch_bounds__(256) void batch_seeds(const PathParams p, const int32_t* seeds, int n, int mark) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const size_t i = (size_t)seeds[2 * k + 1] * p.W * p.H + seeds[2 * k];
    if (mark) p.next[i] = -1;
    else p.cost[i] = 0.0f;
}

template <int CONN>
__global__ __launch_bounds__(SP_NT) void batch_round(const PathParams p, int F, int parity, uint32_t* cnt_next) {
    const int b = blockIdx.z;
    const PathParams q = frame_of(p, b);
    relax_tile<CONN>(q, q.cost, p.flags + (size_t)(parity * F + b) * p.ntiles, p.flags + (size_t)((parity ^ 1) * F + b) * p.ntiles, cnt_next);
}

template <int CONN>
__global__ __launch_bounds__(256) void batch_next(const PathParams p, const int32_t* starts) {
    if (starts[blockIdx.z] < 0) return;
    next_body<CONN>(frame_of(p, blockIdx.z));
}

__global__ __launch_bounds__(64) void batch_walk(const PathParams p, const int32_t* starts, int2* nodes, float2* dirs, int32_t* out) {
    const int b = blockIdx.z, start = starts[b];
    if (start < 0) return;   // (workgroup-uniform)
    const size_t npx = (size_t)p.W * p.H;
    walk_body(frame_of(p, b), start, nodes + b * npx, dirs + b * npx, out + 2 * b);
}

thread_local std::string g_batch_create_error;

int run_append(yh_scene_batch* hb, int n, int mode) {
    yh_scene* h = &hb->core;
    SceneParams p;
    p.depth = h->depth; p.cls_id = nullptr; p.frame = h->frame; p.frame_mode = mode == YH_COMPAT_STRICT ? 0 : 1;
    p.W = h->W; p.H = h->H; p.mode = mode; p.band_h = h->band_h;
    p.terrain_tab = h->terrain_tab; p.robot_tab = h->robot_tab;
    p.map = h->map; p.world = h->world; p.conn0 = h->conn0; p.conn1 = h->conn1; p.ball_acc = h->ball_acc; p.balls = h->balls;
    const size_t npx = (size_t)h->W * h->H;
    SCHK(h, hipMemsetAsync(h->map, 0, n * npx * 4, h->stream));
    SCHK(h, hipMemsetAsync(h->ball_acc, 0, (size_t)n * 300 * sizeof(long long), h->stream));
    const dim3 grid((unsigned)((h->W + 7) / 8), (unsigned)((h->H + 7) / 8), (unsigned)n), block(8, 8);
    hipLaunchKernelGGL(batch_cloud_strips, dim3((unsigned)((h->W + SC_CW - 1) / SC_CW), (unsigned)((h->H + h->band_h - 1) / h->band_h), (unsigned)n), dim3(512), 0, h->stream, p);
    hipLaunchKernelGGL(batch_balls, dim3(1, 1, (unsigned)n), dim3(128), 0, h->stream, p);
    hipLaunchKernelGGL(batch_world, grid, block, 0, h->stream, p);
    hipLaunchKernelGGL(batch_conn1, grid, block, 0, h->stream, p);
    hipLaunchKernelGGL(batch_conn0, grid, block, 0, h->stream, p);
    SCHK(h, hipGetLastError());
    h->ran = true; h->last_mode = mode;
    hb->n = n; hb->append_n = n; hb->append_mode = mode; hb->from_fields = false;
    std::fill(hb->diag_ok.begin(), hb->diag_ok.end(), (uint8_t)1);   // (a frame's own diagonals: both ends hold the same length)
    return YH_OK;
}

int ensure_planner(yh_scene_batch* hb) {
    if (hb->cost) return YH_OK;
    yh_scene* h = &hb->core;
    const size_t all = (size_t)hb->max_frames * h->W * h->H;
    SCHK(h, hipMalloc((void**)&hb->cost, all * 4));
    SCHK(h, hipMalloc((void**)&hb->next, all * 4));
    SCHK(h, hipMalloc((void**)&hb->nodes, all * sizeof(int2)));
    SCHK(h, hipMalloc((void**)&hb->dirs, all * sizeof(float2)));
    SCHK(h, hipMalloc((void**)&hb->walk_out, (size_t)hb->max_frames * 2 * 4));
    SCHK(h, hipMalloc((void**)&hb->starts, (size_t)hb->max_frames * 4));
    SCHK(h, hipHostMalloc((void**)&hb->host_walk, (size_t)hb->max_frames * 2 * 4, hipHostMallocDefault));
    return YH_OK;
}

void free_planner(yh_scene_batch* hb) {
    void* bufs[] = { hb->cost, hb->next, hb->nodes, hb->dirs, hb->walk_out, hb->starts, hb->seeds };
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (hb->host_walk) (void)hipHostFree(hb->host_walk);
    hb->cost = nullptr; hb->next = nullptr; hb->nodes = nullptr; hb->dirs = nullptr; hb->walk_out = nullptr; hb->starts = nullptr; hb->seeds = nullptr;
    hb->host_walk = nullptr; hb->seeds_cap = 0;
}

// the whole plan of hb->n frames on the handle's stream: last_seeds / last_field (pixel and frame of every target), last_starts (-1: no
// plan for that frame). Returns when every route's length is known.
int run_plan(yh_scene_batch* hb, int conn) {
    yh_scene* h = &hb->core;
    const int n = hb->n, ns = (int)hb->last_seeds.size();
    if (ns > hb->seeds_cap) {
        if (hb->seeds) { SCHK(h, hipStreamSynchronize(h->stream)); SCHK(h, hipFree(hb->seeds)); hb->seeds = nullptr; hb->seeds_cap = 0; }
        SCHK(h, hipMalloc((void**)&hb->seeds, (size_t)ns * 2 * 4));
        hb->seeds_cap = ns;
    }
    hb->pairs.resize((size_t)ns * 2);
    for (int k = 0; k < ns; ++k) { hb->pairs[2 * k] = hb->last_seeds[k]; hb->pairs[2 * k + 1] = hb->last_field[k]; }
    SCHK(h, hipMemcpyAsync(hb->seeds, hb->pairs.data(), hb->pairs.size() * 4, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipMemcpyAsync(hb->starts, hb->last_starts.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    PathParams p;
    int rc = solve_alloc(h, conn, hb->max_frames, hb->max_frames, p);
    if (rc) return rc;
    p.cost = hb->cost; p.next = hb->next;
    const size_t npx = (size_t)h->W * h->H;
    const dim3 px((unsigned)((npx + 255) / 256), 1, (unsigned)n), sd((unsigned)((ns + 255) / 256));
    scene_batch_weights(h, p, conn, n);
    SCHK(h, hipMemsetD32Async((hipDeviceptr_t)hb->cost, 0x7f800000, n * npx, h->stream));   // +inf
    hipLaunchKernelGGL(batch_seeds, sd, dim3(256), 0, h->stream, p, hb->seeds, ns, 0);
    const SolveRound round{ [&](const dim3& tiles, int parity, uint32_t* cnt_next) {
        hipLaunchKernelGGL(conn == 8 ? batch_round<8> : batch_round<4>, tiles, dim3(SP_NT), 0, h->stream, p, n, parity, cnt_next);
    }, 1 };
    if ((rc = solve_rounds(h, p, conn, n, hb->last_seeds, "batch", 0, nullptr, &round, &hb->last_field))) return rc;
    hipLaunchKernelGGL(conn == 8 ? batch_next<8> : batch_next<4>, px, dim3(256), 0, h->stream, p, hb->starts);
    hipLaunchKernelGGL(batch_seeds, sd, dim3(256), 0, h->stream, p, hb->seeds, ns, 1);
    hipLaunchKernelGGL(batch_walk, dim3(1, 1, (unsigned)n), dim3(64), 0, h->stream, p, hb->starts, hb->nodes, hb->dirs, hb->walk_out);
    SCHK(h, hipGetLastError());
    SCHK(h, hipMemcpyAsync(hb->host_walk, hb->walk_out, (size_t)n * 2 * 4, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    hb->path_len.assign(n, 0);
    for (int b = 0; b < n; ++b) {
        if (hb->last_starts[b] < 0) continue;
        if (hb->host_walk[2 * b + 1]) return h->fail(YH_EHIP, "frame " + std::to_string(b) + ": path walk: no target within W*H steps (fields not those of a SANE frame?)");
        hb->path_len[b] = hb->host_walk[2 * b];
    }
    return YH_OK;
}

}  // namespace

namespace yh {
void scene_batch_weights(yh_scene* h, const PathParams& p, int conn, int n) {
    const dim3 px((unsigned)(((size_t)h->W * h->H + 255) / 256), 1, (unsigned)n);
    hipLaunchKernelGGL(conn == 8 ? batch_weights<8> : batch_weights<4>, px, dim3(256), 0, h->stream, p);
}
}  // namespace yh

extern "C" {

const char* yh_scene_batch_last_error(const yh_scene_batch* h) { return h ? h->core.err.c_str() : g_batch_create_error.c_str(); }

int yh_scene_batch_create(int32_t device, int32_t width, int32_t height, int32_t max_frames, yh_scene_batch** out) {
    if (!out) { g_batch_create_error = "null argument"; return YH_EINVAL; }
    *out = nullptr;
    if (width < 3 || height < 3 || width > 8192 || height > 8192) { g_batch_create_error = "frame size out of range"; return YH_EINVAL; }
    if (max_frames < 1 || max_frames > 256) { g_batch_create_error = "max_frames out of range (1 .. 256)"; return YH_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { g_batch_create_error = "no such HIP device (no CPU fallback)"; return YH_EHIP; }
    yh_scene_batch* hb = new yh_scene_batch();
    yh_scene* h = &hb->core;
    h->dev = device; h->W = width; h->H = height; h->band_h = 64;
    hb->max_frames = max_frames;
    hb->staged.assign(max_frames, 0); hb->fields_set.assign(max_frames, 0); hb->diag_ok.assign(max_frames, 1); hb->diag_why.resize(max_frames);
    const size_t all = (size_t)max_frames * width * height;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->copied, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void**)&h->depth, all * 2);
    if (e == hipSuccess) e = hipMalloc((void**)&h->frame, all * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->map, all * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->world, all * 16);
    if (e == hipSuccess) e = hipMalloc((void**)&h->conn0, all * 16);
    if (e == hipSuccess) e = hipMalloc((void**)&h->conn1, all * 16);
    if (e == hipSuccess) e = hipMalloc((void**)&h->balls, (size_t)max_frames * 100 * 16);
    if (e == hipSuccess) e = hipMalloc((void**)&h->ball_acc, (size_t)max_frames * 300 * sizeof(long long));
    if (e == hipSuccess) e = scene_tables_build(h);
    if (e != hipSuccess) { g_batch_create_error = std::string("scene batch setup: ") + hipGetErrorString(e); yh_scene_batch_destroy(hb); return YH_EHIP; }
    *out = hb;
    return YH_OK;
}

void yh_scene_batch_destroy(yh_scene_batch* hb) {
    if (!hb) return;
    yh_scene* h = &hb->core;
    hipSetDevice(h->dev);
    if (h->stream) hipStreamSynchronize(h->stream);
    free_planner(hb);
    scene_batch_turn_free(hb);
    scene_batch_turn_tour_free(hb);
    scene_solve_free(h);
    void* bufs[] = { h->depth, h->frame, h->map, h->world, h->conn0, h->conn1, h->balls, h->ball_acc, h->terrain_tab, h->robot_tab };
    for (void* b : bufs) if (b) hipFree(b);
    if (h->copied) hipEventDestroy(h->copied);
    if (h->stream) hipStreamDestroy(h->stream);
    delete hb;
}

int yh_scene_batch_stage(yh_scene_batch* hb, int32_t slot, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device) {
    if (!hb || !depth_host || !frame) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (slot < 0 || slot >= hb->max_frames) return h->fail(YH_EINVAL, "slot " + std::to_string(slot) + " outside 0 .. " + std::to_string(hb->max_frames - 1));
    SCHK(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)h->W * h->H;
    SCHK(h, hipMemcpyAsync(h->depth + slot * npx, depth_host, npx * 2, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipMemcpyAsync(h->frame + slot * npx, frame, npx * 4, frame_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    const int rc = host_sources_done(h, depth_host, frame_on_device ? nullptr : frame);
    if (rc) return rc;
    if (frame_on_device) SCHK(h, hipStreamSynchronize(h->stream));   // the caller's device frame is free again (the next classify overwrites it)
    hb->staged[slot] = 1;
    return YH_OK;
}

// The slot buffers are contiguous ([max_frames][H][W]): n slots are one depth copy and one frame copy, then yh_scene_batch_stage's waits.
int yh_scene_batch_stage_frames(yh_scene_batch* hb, int32_t first_slot, int32_t n_frames, const uint16_t* depth_host, const uint32_t* frames,
                                int32_t frames_on_device) {
    if (!hb || !depth_host || !frames) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (n_frames < 1) return h->fail(YH_EINVAL, "n_frames " + std::to_string(n_frames) + " is below 1");
    if (first_slot < 0 || first_slot >= hb->max_frames || n_frames > hb->max_frames - first_slot)
        return h->fail(YH_EINVAL, "slots " + std::to_string(first_slot) + " .. " + std::to_string((long long)first_slot + n_frames - 1) + " outside 0 .. " + std::to_string(hb->max_frames - 1));
    SCHK(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)h->W * h->H;
    SCHK(h, hipMemcpyAsync(h->depth + first_slot * npx, depth_host, n_frames * npx * 2, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipMemcpyAsync(h->frame + first_slot * npx, frames, n_frames * npx * 4, frames_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    const int rc = host_sources_done(h, depth_host, frames_on_device ? nullptr : frames);
    if (rc) return rc;
    if (frames_on_device) SCHK(h, hipStreamSynchronize(h->stream));   // the caller's device frames are free again (the next yh_instance_batch overwrites them)
    std::fill(hb->staged.begin() + first_slot, hb->staged.begin() + first_slot + n_frames, (uint8_t)1);
    return YH_OK;
}

int yh_scene_batch_append(yh_scene_batch* hb, int32_t n_frames, int32_t mode) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (n_frames < 1 || n_frames > hb->max_frames) return h->fail(YH_EINVAL, "n_frames " + std::to_string(n_frames) + " outside 1 .. " + std::to_string(hb->max_frames));
    if (mode != YH_COMPAT_STRICT && mode != YH_COMPAT_SANE) return h->fail(YH_EINVAL, "bad compat mode");
    for (int b = 0; b < n_frames; ++b)
        if (!hb->staged[b]) return h->fail(YH_ESTATE, "slot " + std::to_string(b) + " has never been staged");
    SCHK(h, hipSetDevice(h->dev));
    ++h->frames;
    return run_append(hb, n_frames, mode);
}

int yh_scene_batch_read(yh_scene_batch* hb, int32_t frame, uint32_t* map, float* world, float* conn0, float* conn1, float* balls) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (!h->ran) return h->fail(YH_ESTATE, "no frame has been appended");
    if (frame < 0 || frame >= hb->n) return h->fail(YH_EINVAL, "frame " + std::to_string(frame) + " outside the last append's " + std::to_string(hb->n));
    SCHK(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)h->W * h->H, o = frame * npx;
    if (map) SCHK(h, hipMemcpyAsync(map, h->map + o, npx * 4, hipMemcpyDeviceToHost, h->stream));
    if (world) SCHK(h, hipMemcpyAsync(world, h->world + o, npx * 16, hipMemcpyDeviceToHost, h->stream));
    if (conn0) SCHK(h, hipMemcpyAsync(conn0, h->conn0 + o, npx * 16, hipMemcpyDeviceToHost, h->stream));
    if (conn1) SCHK(h, hipMemcpyAsync(conn1, h->conn1 + o, npx * 16, hipMemcpyDeviceToHost, h->stream));
    if (balls) SCHK(h, hipMemcpyAsync(balls, h->balls + (size_t)frame * 100, 100 * 16, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    return YH_OK;
}

int yh_scene_batch_plan(yh_scene_batch* hb, const int32_t* targets_xy, int32_t n_targets, const int32_t* starts_xy, int32_t connectivity, int32_t* status) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (connectivity != 4 && connectivity != 8) return h->fail(YH_EINVAL, "connectivity " + std::to_string(connectivity) + ": 4 or 8");
    if (!starts_xy) return h->fail(YH_EINVAL, "starts_xy is null");
    if (!h->ran || hb->n < 1) return h->fail(YH_ESTATE, "no frame has been appended");
    const int n = hb->n;
    const auto framed = [&](int b, int rc) { h->err = "frame " + std::to_string(b) + ": " + h->err; return rc; };
    // every check of every frame before anything is touched: a refused call leaves an earlier plan of this append readable
    int rc;
    for (int b = 0; b < n; ++b) {
        if ((rc = scene_plan_checks(h, n_targets, starts_xy[2 * b], starts_xy[2 * b + 1]))) return framed(b, rc);
        if (hb->from_fields && !hb->fields_set[b]) return h->fail(YH_ESTATE, "frame " + std::to_string(b) + " has been given no fields since the last append");
        if (connectivity == 8 && !hb->diag_ok[b]) return h->fail(YH_ESTATE, "frame " + std::to_string(b) + ": the uploaded fields allow 4-connected plans only: " + hb->diag_why[b]);
    }
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
        starts[b] = starts_xy[2 * b + 1] * h->W + starts_xy[2 * b];
        for (int32_t v : t) { seeds.push_back(v); field.push_back(b); }
    }
    if (status) std::copy(st.begin(), st.end(), status);
    if (seeds.empty()) return h->fail(YH_ESTATE, "no target given and no frame of the batch has a ball inside it");
    h->err.clear();
    if ((rc = ensure_planner(hb))) { free_planner(hb); return rc; }
    hb->last.planned = false;
    hb->last_seeds = seeds; hb->last_field = field; hb->last_starts = starts; hb->status = st;
    if ((rc = run_plan(hb, connectivity))) return rc;
    hb->last.conn = connectivity; hb->last.planned = true; hb->last.frame = h->frames;
    return YH_OK;
}

int yh_scene_batch_plan_read(yh_scene_batch* hb, int32_t frame, float* cost, int32_t* next, int32_t* path_xy, float* directions, int32_t path_capacity, int32_t* path_len) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (frame < 0 || frame >= hb->max_frames || (h->ran && frame >= hb->n)) return h->fail(YH_EINVAL, "frame " + std::to_string(frame) + " outside the last append's " + std::to_string(hb->n));
    SolveLast one = hb->last;   // this frame's part of the batch's plan
    if (one.planned && one.frame == h->frames) {
        if (hb->status[frame] != YH_OK) return h->fail(YH_ESTATE, "frame " + std::to_string(frame) + " had no ball inside it: it has no plan");
        const size_t npx = (size_t)h->W * h->H;
        one.path_len = hb->path_len[frame]; one.nodes = hb->nodes + frame * npx; one.dirs = hb->dirs + frame * npx;
    }
    const size_t o = (size_t)frame * h->W * h->H, bytes = (size_t)h->W * h->H * 4;
    return solve_read(h, "plan", "plan again", &one, { { cost, hb->cost ? hb->cost + o : nullptr, bytes }, { next, hb->next ? hb->next + o : nullptr, bytes } },
                      path_xy, directions, path_capacity, path_len);
}

int yh_scene_batch_time(yh_scene_batch* hb, int32_t reps, float* ms_per_batch) {
    if (!hb || reps < 1 || !ms_per_batch) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (hb->append_n < 1) return h->fail(YH_ESTATE, "no batch has been appended");
    SCHK(h, hipSetDevice(h->dev));
    struct Events { hipEvent_t a = nullptr, b = nullptr; ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev;
    SCHK(h, hipEventCreate(&ev.a)); SCHK(h, hipEventCreate(&ev.b));
    SCHK(h, hipEventRecord(ev.a, h->stream));
    ++h->frames;   // the replays read the slots as they are staged NOW: a new frame generation, as an append is
    for (int r = 0; r < reps; ++r) { const int rc = run_append(hb, hb->append_n, hb->append_mode); if (rc) return rc; }
    SCHK(h, hipEventRecord(ev.b, h->stream));
    SCHK(h, hipEventSynchronize(ev.b));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ev.a, ev.b);
    *ms_per_batch = ms / reps;
    return YH_OK;
}

int yh_scene_batch_plan_time(yh_scene_batch* hb, int32_t reps, float* ms_per_batch, int32_t* rounds, int32_t* tile_runs) {
    if (!hb || reps < 1 || !ms_per_batch) return YH_EINVAL;
    // (a failed replay has overwritten part of the last plan: it is gone)
    auto run = [&] { const int rc = run_plan(hb, hb->last.conn); if (rc) hb->last.planned = false; return rc; };
    return solve_time(&hb->core, "plan", "plan again", &hb->last, reps, run, ms_per_batch, rounds, tile_runs);
}

int yh_scene_batch_set_fields(yh_scene_batch* hb, int32_t frame, const uint32_t* map, const float* conn0, const float* conn1) {
    if (!hb || !map || !conn0 || !conn1) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (frame < 0 || frame >= hb->max_frames) return h->fail(YH_EINVAL, "frame " + std::to_string(frame) + " outside 0 .. " + std::to_string(hb->max_frames - 1));
    bool diag_ok = true;
    std::string diag_why;
    const int rc = scene_check_fields(h, conn0, conn1, diag_ok, diag_why);
    if (rc) return rc;
    SCHK(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)h->W * h->H, o = frame * npx;
    SCHK(h, hipMemcpyAsync(h->map + o, map, npx * 4, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipMemcpyAsync(h->conn0 + o, conn0, npx * 16, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipMemcpyAsync(h->conn1 + o, conn1, npx * 16, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipMemsetAsync(h->world + o, 0, npx * 16, h->stream));
    SCHK(h, hipMemsetAsync(h->balls + (size_t)frame * 100, 0, 100 * 16, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    if (!hb->from_fields) {   // the first use after create or append: the batch is now the frames given here
        hb->from_fields = true; hb->n = 0;
        std::fill(hb->fields_set.begin(), hb->fields_set.end(), (uint8_t)0);
    }
    hb->n = std::max(hb->n, frame + 1);
    hb->fields_set[frame] = 1; hb->diag_ok[frame] = diag_ok; hb->diag_why[frame] = diag_why;
    h->ran = true; h->last_mode = YH_COMPAT_SANE;
    ++h->frames;
    return YH_OK;
}

}  // extern "C"
