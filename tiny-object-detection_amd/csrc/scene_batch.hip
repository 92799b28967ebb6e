// scene_batch.hip — yh_scene_batch: the scene back-end over N frames in one set of launches (DESIGN.md §11 "Scene batch"), and what
// its planners' entry points share. Frame b of a batch has exactly the results a yh_scene handle of the same size gives when it is fed
// that frame alone: every append kernel here takes its frame from blockIdx.z, advances its own copy of the by-value parameter block by
// b frames and runs the body the single handle's kernel runs (scene_dev.h) - there is no second definition of anything.
//
// Launches of one append of n frames: two memsets (maps, ball sums), batch_cloud_strips (strips x bands x n), batch_balls (n blocks),
// batch_world, batch_conn1, batch_conn0 (8 x 8 pixels x n). The first four are scene_batch_stamp, which the memory append
// (scene_batch_memory.hip: a bank of memories, one per camera stream) runs as well, into its own array.
//
// The handle holds a yh_scene as its core: device, size, stream, error text, bump tables, the frame generation and mode - and array
// pointers that are frame 0 of the batch's [max_frames][...] arrays. The planners hang off that core and are the single handle's:
// yh_scene_batch_plan, _plan_tour, _plan_turn and _plan_turn_tour (scene_path.hip, scene_tour.hip, scene_turn.hip, scene_turn_tour.hip) run the one driver of
// their kind over the core's frames, after scene_batch_frames below has checked every frame and chosen its targets.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "scene.h"
#include "scene_batch.h"
#include "scene_dev.h"
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

__global__ __launch_bounds__(512) void batch_cloud_strips(const SceneParams p) { cloud_strips_body(frame_of(p, blockIdx.z)); }
__global__ void batch_balls(const SceneParams p) { balls_body(frame_of(p, blockIdx.z)); }
__global__ __launch_bounds__(64) void batch_world(const SceneParams p) { world_body(frame_of(p, blockIdx.z)); }
__global__ __launch_bounds__(64) void batch_conn1(const SceneParams p) { conn1_body(frame_of(p, blockIdx.z)); }
__global__ __launch_bounds__(64) void batch_conn0(const SceneParams p) { conn0_body(frame_of(p, blockIdx.z)); }

thread_local std::string g_batch_create_error;

}  // namespace

namespace yh {
int scene_batch_stamp(yh_scene_batch* hb, const SceneParams& p, int n) {
    yh_scene* h = &hb->core;
    SCHK(h, hipMemsetAsync(p.map, 0, (size_t)n * p.W * p.H * 4, h->stream));
    SCHK(h, hipMemsetAsync(p.ball_acc, 0, (size_t)n * 300 * sizeof(long long), h->stream));
    hipLaunchKernelGGL(batch_cloud_strips, dim3((unsigned)((p.W + SC_CW - 1) / SC_CW), (unsigned)((p.H + p.band_h - 1) / p.band_h), (unsigned)n), dim3(512), 0, h->stream, p);
    hipLaunchKernelGGL(batch_balls, dim3(1, 1, (unsigned)n), dim3(128), 0, h->stream, p);
    return YH_OK;
}
}  // namespace yh

namespace {

int run_append(yh_scene_batch* hb, int n, int mode) {
    yh_scene* h = &hb->core;
    SceneParams p;
    p.depth = h->depth; p.cls_id = nullptr; p.frame = h->frame; p.frame_mode = mode == YH_COMPAT_STRICT ? 0 : 1;
    p.W = h->W; p.H = h->H; p.mode = mode; p.band_h = h->band_h;
    p.terrain_tab = h->terrain_tab; p.robot_tab = h->robot_tab;
    p.map = h->map; p.world = h->world; p.conn0 = h->conn0; p.conn1 = h->conn1; p.ball_acc = h->ball_acc; p.balls = h->balls;
    const int rc = scene_batch_stamp(hb, p, n);
    if (rc) return rc;
    const dim3 grid((unsigned)((h->W + 7) / 8), (unsigned)((h->H + 7) / 8), (unsigned)n), block(8, 8);
    hipLaunchKernelGGL(batch_world, grid, block, 0, h->stream, p);
    hipLaunchKernelGGL(batch_conn1, grid, block, 0, h->stream, p);
    hipLaunchKernelGGL(batch_conn0, grid, block, 0, h->stream, p);
    SCHK(h, hipGetLastError());
    h->ran = true; h->last_mode = mode;
    hb->n = n; hb->append_n = n; hb->append_mode = mode; hb->from_fields = false;
    std::fill(hb->diag_ok.begin(), hb->diag_ok.end(), (uint8_t)1);   // (a frame's own diagonals: both ends hold the same length)
    return YH_OK;
}

}  // namespace

namespace yh {
int scene_batch_frames(yh_scene_batch* hb, const int32_t* targets_xy, int32_t n_targets, const int32_t* starts_xy, const int32_t* headings, int connectivity,
                       std::vector<int32_t>& st, const std::function<int(int, const std::vector<int32_t>&)>& each) {
    yh_scene* h = &hb->core;
    if (!h->ran || hb->n < 1) return h->fail(YH_ESTATE, "no frame has been appended");
    const int n = hb->n;
    // every check of every frame before anything is touched: a refused call leaves an earlier plan of this append readable
    int rc;
    for (int b = 0; b < n; ++b) {
        if (headings && (rc = scene_turn_heading(h, headings[b]))) return hb->framed(b, rc);
        if ((rc = scene_plan_checks(h, n_targets, starts_xy[2 * b], starts_xy[2 * b + 1]))) return hb->framed(b, rc);
        if (hb->from_fields && !hb->fields_set[b]) return h->fail(YH_ESTATE, "frame " + std::to_string(b) + " has been given no fields since the last append");
        if (!headings && connectivity == 8 && (rc = scene_plan_diagonals(h, hb->diag_ok[b], hb->diag_why[b]))) return hb->framed(b, rc);
    }
    if (headings) {
        if ((rc = scene_turn_size(h))) return rc;
        for (int b = 0; b < n; ++b)
            if ((rc = scene_plan_diagonals(h, hb->diag_ok[b], hb->diag_why[b]))) return hb->framed(b, rc);
    }
    SCHK(h, hipSetDevice(h->dev));
    std::vector<float> balls;
    if (!targets_xy) {   // one read-back for all frames
        balls.resize((size_t)n * 400);
        SCHK(h, hipMemcpyAsync(balls.data(), h->balls, balls.size() * 4, hipMemcpyDeviceToHost, h->stream));
        SCHK(h, hipStreamSynchronize(h->stream));
    }
    st.assign(n, YH_OK);
    std::vector<int32_t> t;
    for (int b = 0; b < n; ++b) {
        rc = scene_plan_choose(h, targets_xy ? targets_xy + (size_t)b * n_targets * 2 : nullptr, n_targets,
                               targets_xy ? nullptr : reinterpret_cast<const float(*)[4]>(balls.data() + (size_t)b * 400), t);
        if (rc == YH_ESTATE && !targets_xy) { st[b] = YH_ESTATE; continue; }   // no usable ball: this frame gets no plan
        if (rc || (rc = each(b, t))) return hb->framed(b, rc);
    }
    return YH_OK;
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
    h->max_frames = max_frames; h->batch = true;
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
    scene_path_free(h);
    scene_tour_free(h);
    scene_turn_free(h);
    scene_turn_tour_free(h);
    scene_solve_free(h);
    scene_batch_memory_free(hb);
    void* bufs[] = { h->depth, h->frame, h->map, h->world, h->conn0, h->conn1, h->balls, h->ball_acc, h->terrain_tab, h->robot_tab };
    for (void* b : bufs) if (b) hipFree(b);
    if (h->copied) hipEventDestroy(h->copied);
    if (h->stream) hipStreamDestroy(h->stream);
    delete hb;
}

int yh_scene_batch_stage(yh_scene_batch* hb, int32_t slot, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device) {
    if (!hb || !depth_host || !frame) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (slot < 0 || slot >= h->max_frames) return h->fail(YH_EINVAL, "slot " + std::to_string(slot) + " outside 0 .. " + std::to_string(h->max_frames - 1));
    SCHK(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)h->W * h->H;
    ++hb->stagings;
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
    if (first_slot < 0 || first_slot >= h->max_frames || n_frames > h->max_frames - first_slot)
        return h->fail(YH_EINVAL, "slots " + std::to_string(first_slot) + " .. " + std::to_string((long long)first_slot + n_frames - 1) + " outside 0 .. " + std::to_string(h->max_frames - 1));
    SCHK(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)h->W * h->H;
    ++hb->stagings;
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
    if (n_frames < 1 || n_frames > h->max_frames) return h->fail(YH_EINVAL, "n_frames " + std::to_string(n_frames) + " outside 1 .. " + std::to_string(h->max_frames));
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

int yh_scene_batch_time(yh_scene_batch* hb, int32_t reps, float* ms_per_batch) {
    if (!hb || reps < 1 || !ms_per_batch) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (scene_batch_memory_is_pyramid_norm(hb))
        return h->fail(YH_ESTATE, "the last frames came from yh_scene_batch_append_memory_pyramid_norm: yh_scene_batch_memory_pyramid_norm_time replays them");
    if (scene_batch_memory_is_norm(hb))
        return h->fail(YH_ESTATE, "the last frames came from yh_scene_batch_append_memory_search_norm: yh_scene_batch_memory_search_norm_time replays them");
    if (scene_batch_memory_is_pyramid(hb))
        return h->fail(YH_ESTATE, "the last frames came from yh_scene_batch_append_memory_pyramid: yh_scene_batch_memory_pyramid_time replays them");
    if (scene_batch_memory_is_search(hb))
        return h->fail(YH_ESTATE, "the last frames came from yh_scene_batch_append_memory_search: yh_scene_batch_memory_search_time replays them");
    if (scene_batch_memory_is_last(hb))
        return h->fail(YH_ESTATE, "the last frames came from yh_scene_batch_append_memory: yh_scene_batch_memory_time replays them");
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

int yh_scene_batch_set_fields(yh_scene_batch* hb, int32_t frame, const uint32_t* map, const float* conn0, const float* conn1) {
    if (!hb || !map || !conn0 || !conn1) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (frame < 0 || frame >= h->max_frames) return h->fail(YH_EINVAL, "frame " + std::to_string(frame) + " outside 0 .. " + std::to_string(h->max_frames - 1));
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
