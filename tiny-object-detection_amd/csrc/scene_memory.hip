// scene_memory.hip — the scene memory (DESIGN.md section 11 "Scene memory"): a yh_scene handle carries its height map and its balls
// from frame to frame by the robot's motion, so that the planners see what the camera saw, not only what it sees now.
// yh_scene_append_memory is yh_scene_append_classified(.., YH_COMPAT_SANE) with two stages replaced:
//   stamps        scene_cloud_strips + scene_balls, unchanged (scene.hip: scene_stamp), but into the memory's own stamp buffer N;
//   scene_balls_memory   one small workgroup: the ball table B carried by carry_q16, aged, merged with the frame's balls;
//   scene_fuse    ONE launch in place of scene_world + scene_conn1 + scene_conn0: F = max(N, fade(M gathered by gather_q16)) per tile
//                 with a one-pixel halo in LDS; F (to the map and to the next memory), world, conn0, conn1 written from there.
// N, the old M and the new M are three buffers: a workgroup's halo reads N and the old M of pixels whose F a neighbour is writing.
// The two memory buffers (and the two ball tables) swap at every memory append, so the previous state survives the append:
// yh_scene_memory_time replays the same launches on it and rewrites the same bits.
// yh_scene_append_memory_search (DESIGN.md section 11 "Scene memory: registration") is the same append with the motion found on the
// device: between the stamps and the fuse, scene_register.hip scores N against M over the caller's candidates and leaves the
// chosen one in a device record, which the fuse and the ball carry read (scene_fuse_dev, scene_balls_memory_dev).
// yh_scene_append_memory_pyramid (DESIGN.md section 11 "Scene memory: pyramid registration") is that append with the candidates
// searched coarse to fine (scene_pyramid.hip), into the same record.
// yh_scene_append_memory_search_norm (DESIGN.md section 11 "Scene memory: normalised registration") is the search append with the
// candidates ranked by the normalised score (scene_register_norm.hip), into the same record and an extension of it.
// yh_scene_append_memory_pyramid_norm (DESIGN.md section 11 "Scene memory: normalised pyramid registration") is the pyramid append
// with every level decided by that score (scene_pyramid_norm.hip), into the same two records.
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>

#include "scene.h"
#include "scene_dev.h"
#include "scene_memory_dev.h"
#include "scene_pyramid_dev.h"
#include "scene_pyramid_norm_dev.h"
#include "scene_register_dev.h"
#include "scene_register_norm_dev.h"
#include "yh_internal.h"

using namespace yh;

struct MemoryCall {   // what one memory append runs on, besides the depth image in the handle's buffer
    const uint32_t* frame = nullptr;   // device
    int g[6] = {}, c[6] = {}, keep = 0, max_age = 0;
};

struct yh_scene_memory {
    uint32_t* stamp = nullptr;             // N [H][W]
    uint32_t* map[2] = { nullptr, nullptr };   // M [H][W]: map[cur] is the memory, map[cur ^ 1] what it was before the last memory append
    int4* tab[2] = { nullptr, nullptr };   // B [100], likewise
    int cur = 0;
    bool stale = true;                     // the buffers are cleared before their next use: fresh ones, or a memory append failed half-way (YH_EHIP)
    // the last memory append, for yh_scene_memory_time (frame == 0: none to replay); the handle's last frame is that append
    // while h->frames == frame (every append and yh_scene_set_fields counts h->frames up)
    uint64_t frame = 0;
    MemoryCall last;
    // registration: allocated at the first search. searched: the last memory append was a search - last_bases are its candidates,
    // reg_rec its choice, reg_acc its sum_n and score table
    unsigned long long* reg_acc = nullptr;
    SceneRegisterRecord* reg_rec = nullptr;
    bool searched = false;
    SceneRegisterBases last_bases = {};
    // normalised registration: norm_min_inside != 0: the last memory append was a normalised search (searched is true as well: the
    // record, sum_n and the S table are where a plain search leaves them) - reg_acc holds T and C behind S, norm_rec the extension
    SceneRegisterNormRecord* norm_rec = nullptr;
    int norm_min_inside = 0;
    // pyramid registration: allocated at the first pyramid append. pyramid: the last memory append was one - last_pyr is its plan,
    // reg_rec its choice, pyr.acc its level tables, pyr.table the centres (searched is false then)
    ScenePyramidBufs pyr;
    bool pyramid = false;
    ScenePyramidPlan last_pyr;
    // normalised pyramid registration: pyrn allocated at the first such append. pyr_norm_min_inside != 0: the last memory append was
    // one (pyramid and searched are false then) - last_pyr is its plan, pyr.table the centres, pyr.maps the levels, reg_rec and
    // norm_rec its choice, pyrn.acc its level tables, pyrn.ext its flags
    ScenePyramidNormBufs pyrn;
    int pyr_norm_min_inside = 0;
};

namespace {

__global__ __launch_bounds__(256) void scene_fuse(const SceneFuseParams p) { fuse_body(p); }
__global__ __launch_bounds__(128) void scene_balls_memory(const SceneBallsMemParams p) { balls_memory_body(p); }

int memory_clear(yh_scene* h, yh_scene_memory* m) {
    const size_t npx = (size_t)h->W * h->H;
    for (int i = 0; i < 2; ++i) {
        SCHK(h, hipMemsetAsync(m->map[i], 0, npx * 4, h->stream));
        SCHK(h, hipMemsetAsync(m->tab[i], 0, 100 * sizeof(int4), h->stream));
    }
    m->stale = false;
    m->frame = 0;
    return YH_OK;
}

// the memory's buffers, at the first memory append: a handle that never remembers pays nothing
int memory_reserve(yh_scene* h) {
    if (!h->memory) h->memory = new yh_scene_memory();
    yh_scene_memory* m = h->memory;
    const size_t npx = (size_t)h->W * h->H;
    if (!m->stamp) SCHK(h, hipMalloc((void**)&m->stamp, npx * 4));
    for (int i = 0; i < 2; ++i) {
        if (!m->map[i]) SCHK(h, hipMalloc((void**)&m->map[i], npx * 4));
        if (!m->tab[i]) SCHK(h, hipMalloc((void**)&m->tab[i], 100 * sizeof(int4)));
    }
    return m->stale ? memory_clear(h, m) : YH_OK;
}

int register_reserve(yh_scene* h) {
    yh_scene_memory* m = h->memory;
    if (!m->reg_acc) SCHK(h, hipMalloc((void**)&m->reg_acc, scene_register_norm_acc_bytes()));   // (the plain search's table is its first third)
    if (!m->norm_rec) SCHK(h, hipMalloc((void**)&m->norm_rec, sizeof(SceneRegisterNormRecord)));
    if (!m->reg_rec) SCHK(h, hipMalloc((void**)&m->reg_rec, sizeof(SceneRegisterRecord)));
    return YH_OK;
}

// the launches of one memory append: reads map[from] / tab[from], writes map[from ^ 1] / tab[from ^ 1] and the handle's fields
// (bases or pyr given: the motion is searched for around them and read from the device record, q.g and q.c are not used; upload:
// the pyramid's table goes to the device first - a replay finds it there; min_inside != 0: the normalised search, or with pyr the
// normalised pyramid)
int run_memory(yh_scene* h, const MemoryCall& q, int from, const SceneRegisterBases* bases = nullptr, const ScenePyramidPlan* pyr = nullptr, bool upload = false,
               int min_inside = 0) {
    yh_scene_memory* m = h->memory;
    SceneParams p;
    p.depth = h->depth; p.cls_id = nullptr; p.frame = q.frame; p.frame_mode = 1;
    p.W = h->W; p.H = h->H; p.mode = YH_COMPAT_SANE; p.band_h = h->band_h;
    p.terrain_tab = h->terrain_tab; p.robot_tab = h->robot_tab;
    p.map = m->stamp; p.world = h->world; p.conn0 = h->conn0; p.conn1 = h->conn1; p.ball_acc = h->ball_acc; p.balls = h->balls;
    const int rc = scene_stamp(h, p);
    if (rc) return rc;
    SceneBallsMemParams b;
    b.ball_acc = h->ball_acc; b.balls = h->balls; b.tab_prev = m->tab[from]; b.tab_next = m->tab[from ^ 1];
    b.W = h->W; b.H = h->H; b.max_age = q.max_age;
    SceneFuseParams f;
    f.stamp = m->stamp; f.mem_prev = m->map[from]; f.mem_next = m->map[from ^ 1];
    f.map = h->map; f.world = h->world; f.conn0 = h->conn0; f.conn1 = h->conn1;
    f.W = h->W; f.H = h->H; f.keep = q.keep;
    for (int i = 0; i < 6; ++i) { b.c[i] = q.c[i]; f.g[i] = q.g[i]; }
    if (pyr) {
        const int rs = min_inside ? scene_pyramid_norm_search(h, m->stamp, m->map[from], *pyr, min_inside, m->pyr, m->pyrn, m->reg_rec, m->norm_rec, upload)
                                  : scene_pyramid_search(h, m->stamp, m->map[from], *pyr, m->pyr, m->reg_rec, upload);
        return rs ? rs : scene_register_fuse(h, f, b, m->reg_rec);
    }
    if (bases) {
        const int rs = min_inside ? scene_register_norm_search(h, m->stamp, m->map[from], *bases, min_inside, m->reg_acc, m->reg_rec, m->norm_rec)
                                  : scene_register_search(h, m->stamp, m->map[from], *bases, m->reg_acc, m->reg_rec);
        return rs ? rs : scene_register_fuse(h, f, b, m->reg_rec);
    }
    hipLaunchKernelGGL(scene_balls_memory, dim3(1), dim3(128), 0, h->stream, b);
    hipLaunchKernelGGL(scene_fuse, dim3((unsigned)((h->W + SF_TW - 1) / SF_TW), (unsigned)((h->H + SF_TH - 1) / SF_TH)), dim3(256), 0, h->stream, f);
    SCHK(h, hipGetLastError());
    return YH_OK;
}

int append_memory(yh_scene* h, const uint16_t* depth_host, const uint32_t* frame, int frame_on_device, MemoryCall q, const SceneRegisterBases* bases, const ScenePyramidPlan* pyr,
                  int min_inside) {
    SCHK(h, hipSetDevice(h->dev));
    int rc = memory_reserve(h);
    if (rc) return rc;
    if ((bases || pyr) && (rc = register_reserve(h))) return rc;
    if (pyr && (rc = scene_pyramid_reserve(h, h->memory->pyr))) return rc;
    if (pyr && min_inside && (rc = scene_pyramid_norm_reserve(h, h->memory->pyrn))) return rc;
    const size_t npx = (size_t)h->W * h->H;
    SCHK(h, hipMemcpyAsync(h->depth, depth_host, npx * 2, hipMemcpyHostToDevice, h->stream));
    q.frame = frame;
    if (!frame_on_device) { SCHK(h, hipMemcpyAsync(h->frame, frame, npx * 4, hipMemcpyHostToDevice, h->stream)); q.frame = h->frame; }
    if ((rc = host_sources_done(h, depth_host, frame_on_device ? nullptr : frame))) return rc;
    yh_scene_memory* m = h->memory;
    if (pyr) m->last_pyr = *pyr;   // (the upload reads the handle's copy: the caller's is free when the call returns)
    if ((rc = run_memory(h, q, m->cur, bases, pyr ? &m->last_pyr : nullptr, true, min_inside))) return rc;
    m->cur ^= 1;
    m->last = q;
    m->searched = bases != nullptr;
    m->pyramid = pyr != nullptr && !min_inside;
    m->norm_min_inside = bases ? min_inside : 0;
    m->pyr_norm_min_inside = pyr ? min_inside : 0;
    if (bases) m->last_bases = *bases;
    return YH_OK;
}

// what every memory append does around append_memory: the frame count, and what a failure or a success leaves
int append_memory_call(yh_scene* h, const uint16_t* depth_host, const uint32_t* frame, int frame_on_device, const MemoryCall& q, const SceneRegisterBases* bases,
                       const ScenePyramidPlan* pyr = nullptr, int min_inside = 0) {
    ++h->frames;   // (earlier plans are of another frame, whatever becomes of this one)
    const int rc = append_memory(h, depth_host, frame, frame_on_device, q, bases, pyr, min_inside);
    yh_scene_memory* m = h->memory;
    if (rc) {
        // a call that fails after its checks leaves no frame and an empty memory
        h->ran = false;
        if (m) { m->stale = true; m->frame = 0; m->searched = false; m->pyramid = false; m->norm_min_inside = 0; m->pyr_norm_min_inside = 0; }
        return rc;
    }
    m->frame = h->frames;
    h->ran = true;
    h->last_cls = nullptr; h->last_frame = m->last.frame; h->last_frame_mode = 1; h->last_mode = YH_COMPAT_SANE;
    h->diag_ok = true; h->diag_why.clear();   // (F is a height map like any other: both ends of a diagonal hold the same length)
    return YH_OK;
}

// `reps` replays of the last memory append from the state it started from, between two events; with search_only, of its
// registration launches alone (the stamps the last replay left are the frame's)
int replay_time(yh_scene* h, int reps, bool search_only, float* ms_out) {
    yh_scene_memory* m = h->memory;
    hipEvent_t a, b;
    SCHK(h, hipEventCreate(&a)); SCHK(h, hipEventCreate(&b));
    SCHK(h, hipEventRecord(a, h->stream));
    // the last append's own inputs and motion, from the state it started from (the other pair of buffers) into the state it left:
    // the same bits again, so nothing is committed (a device frame given to the append must still be valid)
    for (int r = 0; r < reps; ++r) {
        const bool pyr = m->pyramid || m->pyr_norm_min_inside;
        const int rc = !search_only ? run_memory(h, m->last, m->cur ^ 1, m->searched ? &m->last_bases : nullptr, pyr ? &m->last_pyr : nullptr, false,
                                                 m->norm_min_inside | m->pyr_norm_min_inside)
                       : m->pyr_norm_min_inside
                           ? scene_pyramid_norm_search(h, m->stamp, m->map[m->cur ^ 1], m->last_pyr, m->pyr_norm_min_inside, m->pyr, m->pyrn, m->reg_rec, m->norm_rec, false)
                       : m->pyramid ? scene_pyramid_search(h, m->stamp, m->map[m->cur ^ 1], m->last_pyr, m->pyr, m->reg_rec, false)
                       : m->norm_min_inside
                           ? scene_register_norm_search(h, m->stamp, m->map[m->cur ^ 1], m->last_bases, m->norm_min_inside, m->reg_acc, m->reg_rec, m->norm_rec)
                           : scene_register_search(h, m->stamp, m->map[m->cur ^ 1], m->last_bases, m->reg_acc, m->reg_rec);
        if (rc) {
            hipEventDestroy(a); hipEventDestroy(b);
            h->ran = false; m->stale = true; m->frame = 0; m->searched = false; m->pyramid = false; m->norm_min_inside = 0; m->pyr_norm_min_inside = 0;
            return rc;
        }
    }
    SCHK(h, hipEventRecord(b, h->stream));
    SCHK(h, hipEventSynchronize(b));
    float ms = 0;
    hipEventElapsedTime(&ms, a, b);
    hipEventDestroy(a); hipEventDestroy(b);
    *ms_out = ms / reps;
    return YH_OK;
}

}  // namespace

namespace yh {
void scene_memory_free(yh_scene* h) {
    yh_scene_memory* m = h->memory;
    if (!m) return;
    void* bufs[] = { m->stamp, m->map[0], m->map[1], m->tab[0], m->tab[1], m->reg_acc, m->reg_rec, m->norm_rec };
    for (void* b : bufs) if (b) hipFree(b);
    scene_pyramid_release(m->pyr);
    scene_pyramid_norm_release(m->pyrn);
    delete m;
    h->memory = nullptr;
}

bool scene_memory_is_last(const yh_scene* h) { return h->memory && h->memory->frame != 0 && h->memory->frame == h->frames; }
bool scene_memory_is_search(const yh_scene* h) { return scene_memory_is_last(h) && h->memory->searched; }
bool scene_memory_is_norm(const yh_scene* h) { return scene_memory_is_search(h) && h->memory->norm_min_inside != 0; }
bool scene_memory_is_pyramid(const yh_scene* h) { return scene_memory_is_last(h) && h->memory->pyramid; }
bool scene_memory_is_pyramid_norm(const yh_scene* h) { return scene_memory_is_last(h) && h->memory->pyr_norm_min_inside != 0; }
}  // namespace yh

extern "C" {

int yh_scene_append_memory(yh_scene* h, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device,
                           const int32_t* gather_q16, const int32_t* carry_q16, int32_t keep, int32_t ball_max_age) {
    if (!h || !depth_host || !frame || !gather_q16 || !carry_q16) return YH_EINVAL;
    if (keep < 0 || keep > 256) return h->fail(YH_EINVAL, "keep outside 0 .. 256");
    if (ball_max_age < 0 || ball_max_age > 255) return h->fail(YH_EINVAL, "ball_max_age outside 0 .. 255");
    MemoryCall q;
    for (int i = 0; i < 6; ++i) { q.g[i] = gather_q16[i]; q.c[i] = carry_q16[i]; }
    q.keep = keep; q.max_age = ball_max_age;
    return append_memory_call(h, depth_host, frame, frame_on_device, q, nullptr);
}

int yh_scene_append_memory_search(yh_scene* h, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device, int32_t n_rot,
                                  const int32_t* gather_q16, const int32_t* carry_q16, int32_t radius, int32_t keep, int32_t ball_max_age) {
    if (!h || !depth_host || !frame || !gather_q16 || !carry_q16) return YH_EINVAL;
    const int rc = scene_register_bases_check(h, n_rot, gather_q16, carry_q16, radius);
    if (rc) return rc;
    if (keep < 0 || keep > 256) return h->fail(YH_EINVAL, "keep outside 0 .. 256");
    if (ball_max_age < 0 || ball_max_age > 255) return h->fail(YH_EINVAL, "ball_max_age outside 0 .. 255");
    SceneRegisterBases bases = {};
    bases.n_rot = n_rot; bases.radius = radius;
    for (int k = 0; k < n_rot; ++k)
        for (int i = 0; i < 6; ++i) { bases.g[k][i] = gather_q16[6 * k + i]; bases.c[k][i] = carry_q16[6 * k + i]; }
    MemoryCall q;   // (its motion stays zero: the kernels read the chosen one from the device record)
    q.keep = keep; q.max_age = ball_max_age;
    return append_memory_call(h, depth_host, frame, frame_on_device, q, &bases);
}

int yh_scene_append_memory_search_norm(yh_scene* h, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device, int32_t n_rot,
                                       const int32_t* gather_q16, const int32_t* carry_q16, int32_t radius, int32_t min_inside, int32_t keep, int32_t ball_max_age) {
    if (!h || !depth_host || !frame || !gather_q16 || !carry_q16) return YH_EINVAL;
    const int rc = scene_register_bases_check(h, n_rot, gather_q16, carry_q16, radius);
    if (rc) return rc;
    if (min_inside < 1 || (long long)min_inside > (long long)h->W * h->H) return h->fail(YH_EINVAL, "min_inside outside 1 .. width x height");
    if (keep < 0 || keep > 256) return h->fail(YH_EINVAL, "keep outside 0 .. 256");
    if (ball_max_age < 0 || ball_max_age > 255) return h->fail(YH_EINVAL, "ball_max_age outside 0 .. 255");
    SceneRegisterBases bases = {};
    bases.n_rot = n_rot; bases.radius = radius;
    for (int k = 0; k < n_rot; ++k)
        for (int i = 0; i < 6; ++i) { bases.g[k][i] = gather_q16[6 * k + i]; bases.c[k][i] = carry_q16[6 * k + i]; }
    MemoryCall q;   // (its motion stays zero: the kernels read the chosen one from the device record)
    q.keep = keep; q.max_age = ball_max_age;
    return append_memory_call(h, depth_host, frame, frame_on_device, q, &bases, nullptr, min_inside);
}

int yh_scene_motion_norm_read(yh_scene* h, uint64_t* totals, uint64_t* inside, uint64_t* chosen_stc, uint64_t* prior_stc, int32_t* qualified) {
    if (!h) return YH_EINVAL;
    yh_scene_memory* m = h->memory;
    const bool pyr_norm = m && !m->stale && m->pyr_norm_min_inside;
    if (!pyr_norm && (!m || m->stale || !m->searched || !m->norm_min_inside))
        return h->fail(YH_ESTATE, "the last memory append was not yh_scene_append_memory_search_norm (or the memory was reset since)");
    if (pyr_norm && (totals || inside))
        return h->fail(YH_EINVAL, "the last memory append was yh_scene_append_memory_pyramid_norm: yh_scene_pyramid_norm_read returns its level tables");
    SCHK(h, hipSetDevice(h->dev));
    SceneRegisterNormRecord ext;
    const size_t words = register_norm_table_words(m->last_bases.n_rot, m->last_bases.radius);
    SCHK(h, hipMemcpyAsync(&ext, m->norm_rec, sizeof(ext), hipMemcpyDeviceToHost, h->stream));
    if (totals) SCHK(h, hipMemcpyAsync(totals, m->reg_acc + 1 + words, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    if (inside) SCHK(h, hipMemcpyAsync(inside, m->reg_acc + 1 + 2 * words, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 3; ++i) { if (chosen_stc) chosen_stc[i] = ext.chosen[i]; if (prior_stc) prior_stc[i] = ext.prior[i]; }
    if (qualified) *qualified = ext.qualified;
    return YH_OK;
}

int yh_scene_append_memory_pyramid(yh_scene* h, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device, int32_t n_rot,
                                   const int32_t* gather_q16, const int32_t* carry_q16, int32_t levels, int32_t radius, int32_t refine, int32_t keep,
                                   int32_t ball_max_age) {
    if (!h || !depth_host || !frame || !gather_q16 || !carry_q16) return YH_EINVAL;
    ScenePyramidPlan plan;
    const int rc = scene_pyramid_plan_make(h, n_rot, gather_q16, carry_q16, levels, radius, refine, plan);
    if (rc) return rc;
    if (keep < 0 || keep > 256) return h->fail(YH_EINVAL, "keep outside 0 .. 256");
    if (ball_max_age < 0 || ball_max_age > 255) return h->fail(YH_EINVAL, "ball_max_age outside 0 .. 255");
    MemoryCall q;   // (its motion stays zero: the kernels read the chosen one from the device record)
    q.keep = keep; q.max_age = ball_max_age;
    return append_memory_call(h, depth_host, frame, frame_on_device, q, nullptr, &plan);
}

int yh_scene_append_memory_pyramid_norm(yh_scene* h, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device, int32_t n_rot,
                                        const int32_t* gather_q16, const int32_t* carry_q16, int32_t levels, int32_t radius, int32_t refine, int32_t min_inside,
                                        int32_t keep, int32_t ball_max_age) {
    if (!h || !depth_host || !frame || !gather_q16 || !carry_q16) return YH_EINVAL;
    ScenePyramidPlan plan;
    const int rc = scene_pyramid_plan_make(h, n_rot, gather_q16, carry_q16, levels, radius, refine, plan);
    if (rc) return rc;
    if (min_inside < 1 || (long long)min_inside > (long long)h->W * h->H) return h->fail(YH_EINVAL, "min_inside outside 1 .. width x height");
    if (keep < 0 || keep > 256) return h->fail(YH_EINVAL, "keep outside 0 .. 256");
    if (ball_max_age < 0 || ball_max_age > 255) return h->fail(YH_EINVAL, "ball_max_age outside 0 .. 255");
    MemoryCall q;   // (its motion stays zero: the kernels read the chosen one from the device record)
    q.keep = keep; q.max_age = ball_max_age;
    return append_memory_call(h, depth_host, frame, frame_on_device, q, nullptr, &plan, min_inside);
}

int yh_scene_pyramid_norm_read(yh_scene* h, int32_t level, int32_t* centres, uint64_t* scores, uint64_t* totals, uint64_t* inside, uint64_t* sum_n,
                               int32_t* level_min_inside, int32_t* qualified) {
    if (!h) return YH_EINVAL;
    yh_scene_memory* m = h->memory;
    if (!m || m->stale || !m->pyr_norm_min_inside)
        return h->fail(YH_ESTATE, "the last memory append was not yh_scene_append_memory_pyramid_norm (or the memory was reset since)");
    const ScenePyramidPlan& plan = m->last_pyr;
    if (level < 0 || level > plan.levels) return h->fail(YH_EINVAL, "level outside 0 .. " + std::to_string(plan.levels));
    SCHK(h, hipSetDevice(h->dev));
    const int hyp = plan.hyp(level);
    const size_t words = register_norm_table_words(hyp, plan.rho(level));
    const unsigned long long* acc = m->pyrn.acc + pyramid_norm_acc_offset(plan, level);
    int cen[SR_MAX_ROT][2], flags[SR_MAX_ROT];
    unsigned long long sum = 0;
    if (centres) SCHK(h, hipMemcpyAsync(cen, m->pyr.table->centre[level], sizeof(cen), hipMemcpyDeviceToHost, h->stream));
    if (qualified) SCHK(h, hipMemcpyAsync(flags, m->pyrn.ext->qualified[level], sizeof(flags), hipMemcpyDeviceToHost, h->stream));
    if (sum_n) SCHK(h, hipMemcpyAsync(&sum, acc, sizeof(sum), hipMemcpyDeviceToHost, h->stream));
    uint64_t* const tabs[3] = { scores, totals, inside };
    for (int t = 0; t < 3; ++t)
        if (tabs[t]) SCHK(h, hipMemcpyAsync(tabs[t], acc + 1 + t * words, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < hyp; ++k) {
        if (centres) { centres[2 * k] = cen[k][0]; centres[2 * k + 1] = cen[k][1]; }
        if (qualified) qualified[k] = flags[k];
    }
    if (sum_n) *sum_n = sum;
    if (level_min_inside) *level_min_inside = (int32_t)pyramid_norm_min_inside(m->pyr_norm_min_inside, level);
    return YH_OK;
}

int yh_scene_pyramid_read(yh_scene* h, int32_t level, int32_t* centres, uint64_t* scores, uint64_t* sum_n) {
    if (!h) return YH_EINVAL;
    yh_scene_memory* m = h->memory;
    if (!m || m->stale || !(m->pyramid || m->pyr_norm_min_inside))
        return h->fail(YH_ESTATE, "the last memory append was not yh_scene_append_memory_pyramid (or the memory was reset since)");
    const ScenePyramidPlan& plan = m->last_pyr;
    if (level < 0 || level > plan.levels) return h->fail(YH_EINVAL, "level outside 0 .. " + std::to_string(plan.levels));
    SCHK(h, hipSetDevice(h->dev));
    const int hyp = plan.hyp(level), nu = 2 * plan.rho(level) + 1;
    // (after a normalised pyramid append: its S tables, which lie first in each level of its own tables)
    const unsigned long long* acc = m->pyr_norm_min_inside ? m->pyrn.acc + pyramid_norm_acc_offset(plan, level) : m->pyr.acc + plan.acc_offset(level);
    int cen[SR_MAX_ROT][2];
    unsigned long long sum = 0;
    if (centres) SCHK(h, hipMemcpyAsync(cen, m->pyr.table->centre[level], sizeof(cen), hipMemcpyDeviceToHost, h->stream));
    if (sum_n) SCHK(h, hipMemcpyAsync(&sum, acc, sizeof(sum), hipMemcpyDeviceToHost, h->stream));
    if (scores) SCHK(h, hipMemcpyAsync(scores, acc + 1, (size_t)hyp * nu * nu * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < hyp && centres; ++k) { centres[2 * k] = cen[k][0]; centres[2 * k + 1] = cen[k][1]; }
    if (sum_n) *sum_n = sum;
    return YH_OK;
}

int yh_scene_motion_read(yh_scene* h, int32_t* gather_q16, int32_t* carry_q16, int32_t* chosen, uint64_t* score, uint64_t* scores) {
    if (!h) return YH_EINVAL;
    yh_scene_memory* m = h->memory;
    if (!m || m->stale || !(m->searched || m->pyramid || m->pyr_norm_min_inside))
        return h->fail(YH_ESTATE, "the last memory append was not yh_scene_append_memory_search (or the memory was reset since)");
    if (m->pyr_norm_min_inside && scores)
        return h->fail(YH_EINVAL, "the last memory append was yh_scene_append_memory_pyramid_norm: yh_scene_pyramid_read returns its level tables");
    if (m->pyramid && scores) return h->fail(YH_EINVAL, "the last memory append was yh_scene_append_memory_pyramid: yh_scene_pyramid_read returns its level tables");
    SCHK(h, hipSetDevice(h->dev));
    SceneRegisterRecord rec;
    const int nu = 2 * m->last_bases.radius + 1;
    SCHK(h, hipMemcpyAsync(&rec, m->reg_rec, sizeof(rec), hipMemcpyDeviceToHost, h->stream));
    if (scores) SCHK(h, hipMemcpyAsync(scores, m->reg_acc + 1, (size_t)m->last_bases.n_rot * nu * nu * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 6; ++i) { if (gather_q16) gather_q16[i] = rec.g[i]; if (carry_q16) carry_q16[i] = rec.c[i]; }
    for (int i = 0; i < 3; ++i) { if (chosen) chosen[i] = rec.chosen[i]; if (score) score[i] = rec.score[i]; }
    return YH_OK;
}

int yh_scene_memory_read(yh_scene* h, uint32_t* map_mem, int32_t* balls_mem) {
    if (!h) return YH_EINVAL;
    SCHK(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)h->W * h->H;
    yh_scene_memory* m = h->memory;
    if (!m) {   // no memory append yet: empty
        if (map_mem) memset(map_mem, 0, npx * 4);
        if (balls_mem) memset(balls_mem, 0, 100 * 4 * sizeof(int32_t));
        SCHK(h, hipStreamSynchronize(h->stream));
        return YH_OK;
    }
    if (m->stale) { const int rc = memory_reserve(h); if (rc) return rc; }
    if (map_mem) SCHK(h, hipMemcpyAsync(map_mem, m->map[m->cur], npx * 4, hipMemcpyDeviceToHost, h->stream));
    if (balls_mem) SCHK(h, hipMemcpyAsync(balls_mem, m->tab[m->cur], 100 * sizeof(int4), hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    return YH_OK;
}

int yh_scene_memory_reset(yh_scene* h) {
    if (!h) return YH_EINVAL;
    yh_scene_memory* m = h->memory;
    if (!m) return YH_OK;
    SCHK(h, hipSetDevice(h->dev));
    m->stale = true;   // (should the clearing fail, it is made again before the next use)
    m->frame = 0;      // (nothing to replay: the state the last memory append started from is gone)
    m->searched = false;
    m->pyramid = false;
    m->norm_min_inside = 0;
    m->pyr_norm_min_inside = 0;
    return memory_reserve(h);
}

int yh_scene_memory_time(yh_scene* h, int32_t reps, float* ms_per_frame) {
    if (!h || reps < 1 || !ms_per_frame) return YH_EINVAL;
    if (!scene_memory_is_last(h)) return h->fail(YH_ESTATE, "the last frame did not come from yh_scene_append_memory (or the memory was reset since)");
    if (h->memory->pyr_norm_min_inside) return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory_pyramid_norm: yh_scene_memory_pyramid_norm_time replays it");
    if (h->memory->norm_min_inside) return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory_search_norm: yh_scene_memory_search_norm_time replays it");
    if (h->memory->searched) return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory_search: yh_scene_memory_search_time replays it");
    if (h->memory->pyramid) return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory_pyramid: yh_scene_memory_pyramid_time replays it");
    SCHK(h, hipSetDevice(h->dev));
    return replay_time(h, reps, false, ms_per_frame);
}

int yh_scene_memory_search_time(yh_scene* h, int32_t reps, float* ms_per_frame, float* ms_search) {
    if (!h || reps < 1 || !ms_per_frame || !ms_search) return YH_EINVAL;
    if (scene_memory_is_pyramid_norm(h)) return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory_pyramid_norm: yh_scene_memory_pyramid_norm_time replays it");
    if (scene_memory_is_pyramid(h)) return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory_pyramid: yh_scene_memory_pyramid_time replays it");
    if (scene_memory_is_norm(h)) return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory_search_norm: yh_scene_memory_search_norm_time replays it");
    if (!scene_memory_is_search(h)) return h->fail(YH_ESTATE, "the last frame did not come from yh_scene_append_memory_search (or the memory was reset since)");
    SCHK(h, hipSetDevice(h->dev));
    // the whole append first, then its registration launches alone on what that left: the same record and scores again
    const int rc = replay_time(h, reps, false, ms_per_frame);
    return rc ? rc : replay_time(h, reps, true, ms_search);
}

int yh_scene_memory_search_norm_time(yh_scene* h, int32_t reps, float* ms_per_frame, float* ms_search) {
    if (!h || reps < 1 || !ms_per_frame || !ms_search) return YH_EINVAL;
    if (scene_memory_is_pyramid_norm(h)) return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory_pyramid_norm: yh_scene_memory_pyramid_norm_time replays it");
    if (!scene_memory_is_norm(h)) return h->fail(YH_ESTATE, "the last frame did not come from yh_scene_append_memory_search_norm (or the memory was reset since)");
    SCHK(h, hipSetDevice(h->dev));
    // as yh_scene_memory_search_time: the whole append, then its registration launches alone (the clear, the three tables, the choice)
    const int rc = replay_time(h, reps, false, ms_per_frame);
    return rc ? rc : replay_time(h, reps, true, ms_search);
}

int yh_scene_memory_pyramid_time(yh_scene* h, int32_t reps, float* ms_per_frame, float* ms_search) {
    if (!h || reps < 1 || !ms_per_frame || !ms_search) return YH_EINVAL;
    if (scene_memory_is_pyramid_norm(h)) return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory_pyramid_norm: yh_scene_memory_pyramid_norm_time replays it");
    if (scene_memory_is_norm(h)) return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory_search_norm: yh_scene_memory_search_norm_time replays it");
    if (!scene_memory_is_pyramid(h)) return h->fail(YH_ESTATE, "the last frame did not come from yh_scene_append_memory_pyramid (or the memory was reset since)");
    SCHK(h, hipSetDevice(h->dev));
    // as yh_scene_memory_search_time: the whole append, then its registration launches alone (the levels, the clear, scores and select)
    const int rc = replay_time(h, reps, false, ms_per_frame);
    return rc ? rc : replay_time(h, reps, true, ms_search);
}

int yh_scene_memory_pyramid_norm_time(yh_scene* h, int32_t reps, float* ms_per_frame, float* ms_search) {
    if (!h || reps < 1 || !ms_per_frame || !ms_search) return YH_EINVAL;
    if (!scene_memory_is_pyramid_norm(h)) return h->fail(YH_ESTATE, "the last frame did not come from yh_scene_append_memory_pyramid_norm (or the memory was reset since)");
    SCHK(h, hipSetDevice(h->dev));
    // as yh_scene_memory_pyramid_time: the whole append, then its registration launches alone (the levels, the clear, tables and select)
    const int rc = replay_time(h, reps, false, ms_per_frame);
    return rc ? rc : replay_time(h, reps, true, ms_search);
}

}  // extern "C"
