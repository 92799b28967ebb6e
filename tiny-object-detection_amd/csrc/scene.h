// scene.h — the scene handle, shared by scene.hip (the two shaders as HIP kernels), scene_path.hip (the planner on its fields),
// scene_tour.hip (the tour over several targets), scene_turn.hip (the turn-aware plan), scene_turn_tour.hip (the turn-aware tour),
// scene_solve.hip (the field solver they run on) and scene_batch.hip (yh_scene_batch, scene_batch.h: N frames per launch; its handle
// holds one of these as its core, the arrays those of N frames). The four planners (plan, tour, turn plan, turn tour) exist for
// both handles and have ONE driver each, over max_frames frames: a yh_scene is the batch of one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "yh_internal.h"

struct yh_scene_path;   // the planner's fields, routes and last plan, frame-major (scene_path.hip); allocated at the first plan
struct yh_scene_tour;   // the tour's fields, routes and last tour, frame-major (scene_tour.hip); allocated at the first tour
struct yh_scene_turn;   // the turn-aware planner's fields, routes and last turn plan, frame-major (scene_turn.hip); allocated at the first turn plan
struct yh_scene_turn_tour;   // the turn-aware tour's fields, leg tables and routes, frame-major (scene_turn_tour.hip); allocated at the first turn tour
struct yh_scene_batch;  // scene_batch.h
struct yh_scene_solve;  // the solver's buffers, one set for both (scene_path_dev.h, scene_solve.hip); allocated at the first of either
struct yh_scene_memory; // the scene memory: map and ball table carried across frames (scene_memory.hip); allocated at the first memory append
namespace yh { struct SceneParams; }   // scene_dev.h

struct yh_scene {
    int dev = 0, W = 0, H = 0, band_h = 64;
    int max_frames = 1;    // frames the arrays below (and the planners') hold one after the other: 1, or what yh_scene_batch_create was given
    bool batch = false;    // the core of a yh_scene_batch: the planners' error texts name the frame
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
    yh_scene_memory* memory = nullptr;
    int fail(int code, const std::string& m) { err = m; return code; }
    std::string frame_tag(int b) const { return batch ? "frame " + std::to_string(b) + ": " : std::string(); }
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
// scene.hip: the first two stages of a frame on the handle's stream - p.map and p.ball_acc cleared, the bumps stamped into p.map, the
// ball means into p.balls (run_scene's own first half; the memory append stamps into a buffer of its own)
int scene_stamp(yh_scene* h, const SceneParams& p);
// scene_memory.hip: the memory's buffers (yh_scene_destroy); whether the handle's last frame came from yh_scene_append_memory
void scene_memory_free(yh_scene* h);
bool scene_memory_is_last(const yh_scene* h);
bool scene_memory_is_search(const yh_scene* h);   // .. from yh_scene_append_memory_search
bool scene_memory_is_norm(const yh_scene* h);     // .. from yh_scene_append_memory_search_norm (is_search holds as well)
bool scene_memory_is_pyramid(const yh_scene* h);  // .. from yh_scene_append_memory_pyramid
bool scene_memory_is_pyramid_norm(const yh_scene* h);   // .. from yh_scene_append_memory_pyramid_norm (is_pyramid does not hold)
// what an 8-connected plan or tour asks of a frame's diagonal lengths (YH_ESTATE and why if they fail it: ok and why are the
// scene's diag_ok / diag_why, or those of a batch's frame); touches nothing
int scene_plan_diagonals(yh_scene* h, bool ok, const std::string& why);
// the turn planners' checks of their own arguments, one text each for all four turn entry points; touch nothing
int scene_turn_heading(yh_scene* h, int32_t heading);
int scene_turn_price(yh_scene* h, float turn_price);
int scene_turn_size(yh_scene* h);
// What the four batched plans do before they touch anything (scene_batch.hip): every check of every frame (headings, if given,
// are the turn planners': their size guard and every frame's diagonals are checked too; otherwise the diagonals only for
// connectivity 8), one read-back of the balls, the choice of targets per frame - each(b, targets) takes frame b's and may refuse them -
// and st[b] = YH_ESTATE for a frame without a usable ball (each is not called for it). A refusal names its frame.
int scene_batch_frames(yh_scene_batch* hb, const int32_t* targets_xy, int32_t n_targets, const int32_t* starts_xy, const int32_t* headings, int connectivity,
                       std::vector<int32_t>& st, const std::function<int(int, const std::vector<int32_t>&)>& each);
}
