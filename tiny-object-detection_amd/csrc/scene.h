// scene.h — the scene handle, shared by scene.hip (the two shaders as HIP kernels), scene_path.hip (the planner on its fields),
// scene_tour.hip (the tour over several targets), scene_turn.hip (the turn-aware plan), scene_turn_tour.hip (the turn-aware tour),
// scene_solve.hip (the field solver they run on)
// and scene_batch.hip / scene_batch_turn.hip / scene_batch_turn_tour.hip (yh_scene_batch, scene_batch.h: N frames per launch; its handle holds one of these as its
// core, the arrays those of N frames).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "yh_internal.h"

struct yh_scene_path;   // the planner's fields, route and last plan (scene_path.hip); allocated at the first yh_scene_plan
struct yh_scene_tour;   // the tour's fields, route and last tour (scene_tour.hip); allocated at the first yh_scene_plan_tour
struct yh_scene_turn;   // the turn-aware planner's fields, route and last turn plan (scene_turn.hip); allocated at the first yh_scene_plan_turn
struct yh_scene_turn_tour;   // the turn-aware tour's fields, leg table and route (scene_turn_tour.hip); allocated at the first yh_scene_plan_turn_tour
struct yh_scene_solve;  // the solver's buffers, one set for both (scene_path_dev.h, scene_solve.hip); allocated at the first of either

struct yh_scene {
    int dev = 0, W = 0, H = 0, band_h = 64;
    hipStream_t stream = nullptr;
    hipEvent_t copied = nullptr;
    std::string err;
    uint16_t* depth = nullptr;
    uint8_t* cls_id = nullptr;
    uint32_t* frame = nullptr;
    uint32_t* map = nullptr;
    float4 *world = nullptr, *conn0 = nullptr, *conn1 = nullptr, *balls = nullptr;
    long long* ball_acc = nullptr;
    uint32_t *terrain_tab = nullptr, *robot_tab = nullptr;
    bool ran = false;
    // what the last append ran on (yh_scene_time replays exactly this)
    const uint8_t* last_cls = nullptr;
    const uint32_t* last_frame = nullptr;
    int last_frame_mode = 0, last_mode = 0;
    uint64_t frames = 0;   // appends (and yh_scene_set_fields) so far: a plan belongs to the frame it was made on
    // whether every in-frame diagonal length of the last frame is finite, >= 1 and equal to the other end's entry (what an
    // 8-connected plan assumes): a SANE append makes them so, yh_scene_set_fields records what it was given
    bool diag_ok = true;
    std::string diag_why;
    yh_scene_path* path = nullptr;
    yh_scene_tour* tour = nullptr;
    yh_scene_turn* turn = nullptr;
    yh_scene_turn_tour* turn_tour = nullptr;
    yh_scene_solve* solve = nullptr;
    int fail(int code, const std::string& m) { err = m; return code; }
};

#define SCHK(h, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return (h)->fail(YH_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

namespace yh {
void scene_path_free(yh_scene* h);   // yh_scene_destroy: the planner's buffers (the handle's device is current, its stream idle)
void scene_tour_free(yh_scene* h);
void scene_turn_free(yh_scene* h);
void scene_turn_tour_free(yh_scene* h);
void scene_solve_free(yh_scene* h);
// yh_scene_plan's checks (frame, mode, size guard, start, targets) and its choice of targets, as linear indices; touches nothing
int scene_plan_targets(yh_scene* h, const int32_t* targets_xy, int32_t n_targets, int32_t start_x, int32_t start_y, std::vector<int32_t>& targets);
// its two halves, for a caller that checks several frames and reads their balls back once (scene_batch.hip)
int scene_plan_checks(yh_scene* h, int32_t n_targets, int32_t start_x, int32_t start_y);
int scene_plan_choose(yh_scene* h, const int32_t* targets_xy, int32_t n_targets, const float (*balls)[4], std::vector<int32_t>& targets);
// yh_scene_set_fields' host-side check (YH_EINVAL and why), and whether the diagonals allow 8-connected plans; touches nothing
int scene_check_fields(yh_scene* h, const float* conn0, const float* conn1, bool& diag_ok, std::string& diag_why);
// scene.hip: waits until host sources a, b (either may be null) of copies enqueued on the stream may be reused; the bump tables of a handle
int host_sources_done(yh_scene* h, const void* a, const void* b);
hipError_t scene_tables_build(yh_scene* h);
// what an 8-connected plan or tour asks of the last frame's diagonal lengths (YH_ESTATE and why if they fail it); touches nothing
int scene_plan_diagonals(yh_scene* h);
}
