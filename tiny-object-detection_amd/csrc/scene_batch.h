// scene_batch.h — the scene batch handle (yh_scene_batch), shared by scene_batch.hip (stage, append, the plain plan),
// scene_batch_turn.hip (the turn-aware plan over the batch) and scene_batch_turn_tour.hip (the turn-aware tour over the batch).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "scene.h"
#include "scene_path_dev.h"

struct yh_scene_batch_turn;   // the turn plan's fields, routes and last call (scene_batch_turn.hip); allocated at the first yh_scene_batch_plan_turn
struct yh_scene_batch_turn_tour;   // the turn tour's fields, tables, routes and last call (scene_batch_turn_tour.hip); allocated at the first yh_scene_batch_plan_turn_tour

struct yh_scene_batch {
    yh_scene core;
    int max_frames = 0;
    int n = 0;                          // frames of the last append (or the highest frame given to yh_scene_batch_set_fields + 1)
    int append_n = 0, append_mode = 0;  // the last append proper (yh_scene_batch_time replays it)
    bool from_fields = false;           // the current frames came through yh_scene_batch_set_fields
    std::vector<uint8_t> staged, fields_set, diag_ok;   // per slot / frame
    std::vector<std::string> diag_why;
    // the planner (allocated at the first plan, for max_frames frames)
    float* cost = nullptr;        // [max][H][W]
    int32_t* next = nullptr;      // [max][H][W]
    int2* nodes = nullptr;        // [max][W*H]
    float2* dirs = nullptr;       // [max][W*H]
    int32_t* walk_out = nullptr;  // [max][2]: length, status
    int32_t* starts = nullptr;    // [max] linear index, -1: no plan for this frame
    int32_t* seeds = nullptr;     // [seeds_cap][2]: linear index, frame
    int32_t seeds_cap = 0;
    int32_t* host_walk = nullptr; // pinned [max][2]
    yh::SolveLast last;           // planned, frame generation, connectivity of the last plan
    std::vector<int32_t> status, path_len, last_seeds, last_field, last_starts;
    std::vector<int32_t> pairs;   // last_seeds and last_field interleaved, as uploaded
    yh_scene_batch_turn* turn = nullptr;   // the turn-aware plan (scene_batch_turn.hip)
    yh_scene_batch_turn_tour* turn_tour = nullptr;   // the turn-aware tour (scene_batch_turn_tour.hip)
    int fail(int code, const std::string& m) { return core.fail(code, m); }
};

namespace yh {
// scene_batch.hip: enqueues the edge terms of the first n frames (batch_weights<conn>: weights_body on the frame of blockIdx.z)
void scene_batch_weights(yh_scene* h, const PathParams& p, int conn, int n);
// yh_scene_batch_destroy: the turn plan's buffers (the handle's device is current, its stream idle)
void scene_batch_turn_free(yh_scene_batch* hb);
void scene_batch_turn_tour_free(yh_scene_batch* hb);   // the same for the turn tour's
}
