// scene_batch.h — the scene batch handle (yh_scene_batch): what is about frames as such. Its planners are its core's (scene.h): the
// plan, tour, turn plan and turn tour of a batch are the drivers of scene_path.hip, scene_tour.hip, scene_turn.hip and scene_turn_tour.hip run over the
// core's max_frames frames, and their yh_scene_batch_* entry points stand next to the yh_scene_* ones in those units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "scene.h"

struct yh_scene_batch_memory;   // the bank of memories, one per camera stream (scene_batch_memory.hip); allocated at the first memory append

struct yh_scene_batch {
    yh_scene core;                      // core.max_frames: the slots; core.batch is set
    yh_scene_batch_memory* memory = nullptr;
    int n = 0;                          // frames of the last append (or the highest frame given to yh_scene_batch_set_fields + 1)
    int append_n = 0, append_mode = 0;  // the last append proper (yh_scene_batch_time replays it)
    bool from_fields = false;           // the current frames came through yh_scene_batch_set_fields
    std::vector<uint8_t> staged, fields_set, diag_ok;   // per slot / frame
    uint64_t stagings = 0;              // stage calls so far: a replay of the staged slots knows whether they are still what it ran on
    std::vector<std::string> diag_why;
    int fail(int code, const std::string& m) { return core.fail(code, m); }
    // rc of a check of frame b, its text now naming the frame
    int framed(int b, int rc) { core.err = "frame " + std::to_string(b) + ": " + core.err; return rc; }
    // the frame argument of the planners' read entry points
    int frame_ok(int32_t frame) {
        if (frame < 0 || frame >= core.max_frames || (core.ran && frame >= n)) return fail(YH_EINVAL, "frame " + std::to_string(frame) + " outside the last append's " + std::to_string(n));
        return YH_OK;
    }
};

namespace yh {
// scene_batch.hip: the first two stages of n frames on the handle's stream - n frames of p.map and p.ball_acc cleared, every frame's
// bumps stamped into its p.map, its ball means into its p.balls (the append's own first half; the memory append stamps into the
// bank's array)
int scene_batch_stamp(yh_scene_batch* hb, const SceneParams& p, int n);
// scene_batch_memory.hip: the bank's buffers (yh_scene_batch_destroy); whether the current frames came from yh_scene_batch_append_memory
void scene_batch_memory_free(yh_scene_batch* hb);
bool scene_batch_memory_is_last(const yh_scene_batch* hb);
bool scene_batch_memory_is_search(const yh_scene_batch* hb);   // .. from yh_scene_batch_append_memory_search
bool scene_batch_memory_is_pyramid(const yh_scene_batch* hb);  // .. from yh_scene_batch_append_memory_pyramid
bool scene_batch_memory_is_norm(const yh_scene_batch* hb);          // .. from yh_scene_batch_append_memory_search_norm (is_search holds too)
bool scene_batch_memory_is_pyramid_norm(const yh_scene_batch* hb);  // .. from yh_scene_batch_append_memory_pyramid_norm (is_pyramid does not hold)
}
