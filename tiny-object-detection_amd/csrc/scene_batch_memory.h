// scene_batch_memory.h — the state of the scene batch's bank of memories (scene_batch_memory.hip), for the units that run on it:
// the memory append itself, its registration (scene_batch_register.hip), its pyramid registration (scene_batch_pyramid.hip) and the
// normalised forms of both (scene_batch_register_norm.hip, scene_batch_pyramid_norm.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "scene_batch.h"
#include "scene_memory_dev.h"
#include "scene_pyramid_dev.h"
#include "scene_pyramid_norm_dev.h"
#include "scene_register_dev.h"
#include "scene_register_norm_dev.h"

namespace yh {

struct BankStream {
    uint32_t* map[2] = { nullptr, nullptr };   // M [H][W]: map[cur] is the memory, map[cur ^ 1] what it was before the last call that named the stream
    int4* tab[2] = { nullptr, nullptr };       // B [100], likewise
    int cur = 0;
    bool stale = true;                         // cleared before the next use: fresh buffers, a reset, or a call that failed half-way
};

}  // namespace yh

struct yh_scene_batch_memory {
    uint32_t* stamp = nullptr;    // N [max_frames][H][W]
    int4* tabs = nullptr;         // [max_frames][100]: every frame's table right after it
    // device: SceneFuseSlot [max_frames], SceneBallsStep [max_frames], SceneBallsChain [YH_SCENE_STREAMS_MAX] and, from the first
    // search on, SceneRegisterBases [max_frames]
    unsigned char* table = nullptr;
    size_t table_bytes = 0;
    std::vector<unsigned char> table_host;
    yh::BankStream bank[YH_SCENE_STREAMS_MAX];
    // the last memory append, for yh_scene_batch_memory_time: the handle's frames are that append's while core.frames == frame
    // (every append and yh_scene_batch_set_fields counts core.frames up); a reset or a staged slot since leaves nothing to replay
    uint64_t frame = 0, stagings = 0;
    bool replayable = false;
    int n = 0, keep = 0, max_age = 0, chains = 0;
    std::vector<int> round_off;   // slots of round r: round_off[r] .. round_off[r + 1]
    // registration, allocated at the first search: frame b's sum_n and score table at reg_acc + b * acc_stride (the stride is the
    // call's: 1 + n_rot (2 radius + 1)^2 words), its record at reg_rec + b. searched: the last memory append was a search.
    unsigned long long* reg_acc = nullptr;    // [max_frames][1 + SR_MAX_ROT * SR_MAX_NU^2]
    yh::SceneRegisterRecord* reg_rec = nullptr;   // [max_frames]
    bool searched = false;
    int n_rot = 0, radius = 0;
    size_t acc_stride() const { return 1 + (norm_min_inside ? 3 : 1) * yh::register_norm_table_words(n_rot, radius); }
    // pyramid registration, allocated at the first pyramid append (it shares reg_rec): frame b's pooled levels of N, then of M, at
    // pyr_maps + b * 2 * scene_pyramid_map_words, its level tables at pyr_acc + b * pyr.acc_offset(levels + 1) (the stride is the
    // call's), its table of level bases at pyr_table + b. pyramid: the last memory append was a pyramid append; pyr: its n_rot,
    // levels, radius and refine (the plan's own table is not used: every frame has one in pyr_host).
    uint32_t* pyr_maps = nullptr;             // [max_frames][2][scene_pyramid_map_words]
    unsigned long long* pyr_acc = nullptr;    // [max_frames][scene_pyramid_acc_bytes / 8]
    yh::ScenePyramidTable* pyr_table = nullptr;   // [max_frames]
    std::vector<yh::ScenePyramidTable> pyr_host;
    bool pyramid = false;
    yh::ScenePyramidPlan pyr;
    // normalised registration, allocated at the first such append. norm_min_inside != 0: the last memory append was a normalised
    // search (searched is true as well, n_rot and radius are its own): frame b's sum_n, then its S, T and C tables, at
    // norm_acc + b * acc_stride (the call's: 1 + 3 n_rot (2 radius + 1)^2 words), its record at reg_rec + b, the extension at
    // norm_rec + b.
    unsigned long long* norm_acc = nullptr;          // [max_frames][scene_register_norm_acc_bytes / 8]
    yh::SceneRegisterNormRecord* norm_rec = nullptr; // [max_frames]
    int norm_min_inside = 0;
    // normalised pyramid registration, allocated at the first such append (it shares pyr_maps, pyr_table, pyr_host, reg_rec and
    // norm_rec; pyramid stays false). pyr_norm_min_inside != 0: the last memory append was one, pyr its parameters: frame b's level
    // tables at pyrn_acc + b * pyramid_norm_acc_offset(pyr, levels + 1) (the stride is the call's), its flags at pyrn_ext + b.
    unsigned long long* pyrn_acc = nullptr;          // [max_frames][scene_pyramid_norm_acc_bytes / 8]
    yh::ScenePyramidNormExt* pyrn_ext = nullptr;     // [max_frames]
    int pyr_norm_min_inside = 0;
};

namespace yh {
// the layout of the device table
inline size_t scene_batch_slots_bytes(const yh_scene* h) { return (size_t)h->max_frames * sizeof(SceneFuseSlot); }
inline size_t scene_batch_steps_bytes(const yh_scene* h) { return (size_t)h->max_frames * sizeof(SceneBallsStep); }
inline size_t scene_batch_bases_offset(const yh_scene* h) { return scene_batch_slots_bytes(h) + scene_batch_steps_bytes(h) + YH_SCENE_STREAMS_MAX * sizeof(SceneBallsChain); }

// scene_batch_register.hip, on the handle's stream (its device current), from the device table and the schedule of the last
// scheduled search append. reserve: the score tables and the records. search: the clear, then per round the scores and the choice
// and, with `f` given, the fuse of that round with each frame's motion read from its record (without: the registration launches
// alone, on the map slots an earlier run left). balls: the ball chains with each step's carry read from its frame's record.
int scene_batch_register_reserve(yh_scene_batch* hb);
int scene_batch_register_search(yh_scene_batch* hb, const SceneFuseParams* f);
int scene_batch_register_balls(yh_scene_batch* hb, const SceneBallsMemParams& b);
// the fuse of one round alone: `count` slots from `round`, each frame's motion read from its record
void scene_batch_register_fuse_round(yh_scene_batch* hb, const SceneFuseParams& f, const SceneFuseSlot* round, unsigned count);

// scene_batch_pyramid.hip, likewise, for the last scheduled pyramid append. reserve: the pooled levels, the level tables, the tables
// of level bases and the records. search: the clear, then per round the levels of every frame's N and M, scores and choice level by
// level and, with `f` given, the fuse of that round (without: the registration launches alone). The ball chains are
// scene_batch_register_balls.
int scene_batch_pyramid_reserve(yh_scene_batch* hb);
int scene_batch_pyramid_search(yh_scene_batch* hb, const SceneFuseParams* f);
// the pooling of one round alone: levels 1 .. levels of N and M of `count` slots from `round` into the frames' parts of pyr_maps;
// pp is filled for frame 0 (level l of its N at pp.dst[0][l - 1], of its M at pp.dst[1][l - 1]; a frame 2 x map_words further on)
void scene_batch_pyramid_levels_round(yh_scene_batch* hb, int levels, const SceneFuseSlot* round, unsigned count, ScenePyramidParams& pp);

// scene_batch_register_norm.hip: scene_batch_register_reserve / _search for the last scheduled normalised search append (the S, T
// and C tables, the records and their extensions; min_inside is the call's). The fuse and the ball chains are the plain search's.
int scene_batch_register_norm_reserve(yh_scene_batch* hb);
int scene_batch_register_norm_search(yh_scene_batch* hb, const SceneFuseParams* f);

// scene_batch_pyramid_norm.hip: scene_batch_pyramid_reserve / _search for the last scheduled normalised pyramid append. The pooling
// is scene_batch_pyramid_levels_round, the fuse and the ball chains are the plain search's.
int scene_batch_pyramid_norm_reserve(yh_scene_batch* hb);
int scene_batch_pyramid_norm_search(yh_scene_batch* hb, const SceneFuseParams* f);
}
