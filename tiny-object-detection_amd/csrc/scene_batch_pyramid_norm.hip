// scene_batch_pyramid_norm.hip — the scene batch's normalised pyramid registration (DESIGN.md section 11 "Scene batch: normalised
// pyramid registration"): yh_scene_batch_append_memory_pyramid_norm is yh_scene_batch_append_memory_pyramid
// (scene_batch_pyramid.hip) with the single handle's normalised bodies (scene_pyramid_norm_dev.h) in place of the plain ones, exactly
// as n yh_scene_append_memory_pyramid_norm calls in batch order. The schedule, the frames' tables of level bases, the pooled levels,
// the fuse and the ball chains are the plain batched pyramid's. With R the most frames one stream has in the call and L levels,
// after the stamps and on the handle's stream:
//   (upload)                     the n frames' tables of level bases, one copy (scene_batch_memory.hip; not when a call is replayed)
//   (clear)                      the level tables of all n frames, one memset (a frame's: pyramid_norm_acc_offset(L + 1) words)
//   per round r:
//     batch_pyramid              (scene_batch_pyramid.hip, unchanged) levels 1 .. L of every frame's N and M
//     per level L .. 0:
//       batch_pyramid_norm_scores       grid (tiles of the level, its hypotheses, frames of the round): register_norm_scores_body;
//                                       at level L instead
//       batch_pyramid_norm_scores_rows  grid (tiles, hypotheses, frames x (2 R + 1)): a row of shifts a workgroup
//       batch_pyramid_norm_select       grid (level > 0: n_rot, else 1; frames of the round): pyramid_norm_select_body; at level 0
//                                       into the frame's two records
//     batch_fuse_dev             (scene_batch_register.hip, unchanged) with g read from the frame's record
//   batch_balls_memory_dev       (scene_batch_register.hip, unchanged) ONE launch after the last round
// R (2 L + 4) + 1 launches and the stamps' four, as the plain batched pyramid; no host wait. The entry points live with the bank's
// state in scene_batch_memory.hip.
#include <hip/hip_runtime.h>

#include "scene.h"
#include "scene_batch.h"
#include "scene_batch_memory.h"
#include "scene_memory_dev.h"
#include "scene_pyramid_norm_dev.h"
#include "yh_internal.h"

using namespace yh;

namespace {

// p: W, H of the level; stamp = level `level` of frame 0's N (level 0: the bank's stamps), a frame frame_words further on; acc = the
// level's tables of frame 0. POOLED (level > 0): a frame's M lies mem_off words behind its N; level 0: it is the slot's mem_prev (two
// instantiations for the reason written above batch_pyramid_scores). The frame is uniform over the workgroup and only the three
// pointers change; the bases stay where they are, so the body's reads of the coefficients are scalar loads.
template <bool POOLED>
__global__ __launch_bounds__(256, 4) void batch_pyramid_norm_scores(const SceneRegisterParams p, const SceneFuseSlot* __restrict__ slots,
                                                                    const ScenePyramidTable* __restrict__ tables, const int level, const size_t frame_words,
                                                                    const size_t mem_off, const size_t acc_stride) {
    const SceneFuseSlot* e = slots + blockIdx.z;
    const int frame = e->frame;
    SceneRegisterParams q = p;
    q.stamp += (size_t)frame * frame_words;
    if (POOLED) q.mem = q.stamp + mem_off; else q.mem = e->mem_prev;
    q.acc += (size_t)frame * acc_stride;
    register_norm_scores_body(q, tables[frame].lv[level]);
}

// the coarsest level (always pooled: levels >= 1): blockIdx.z = slot x rows + row, rows = 2 radius + 1 of that level
__global__ __launch_bounds__(256, 4) void batch_pyramid_norm_scores_rows(const SceneRegisterParams p, const SceneFuseSlot* __restrict__ slots,
                                                                         const ScenePyramidTable* __restrict__ tables, const int level, const int rows,
                                                                         const size_t frame_words, const size_t mem_off, const size_t acc_stride) {
    const int slot = (int)blockIdx.z / rows, row = (int)blockIdx.z - slot * rows;
    const int frame = slots[slot].frame;
    SceneRegisterParams q = p;
    q.stamp += (size_t)frame * frame_words;
    q.mem = q.stamp + mem_off;
    q.acc += (size_t)frame * acc_stride;
    pyramid_norm_scores_rows_body(q, tables[frame].lv[level], row, row + 1);
}

__global__ __launch_bounds__(256) void batch_pyramid_norm_select(const unsigned long long* acc, const SceneFuseSlot* __restrict__ slots, ScenePyramidTable* tables,
                                                                 const int level, const int min_inside, SceneRegisterRecord* recs, SceneRegisterNormRecord* nrecs,
                                                                 ScenePyramidNormExt* exts, const size_t acc_stride) {
    const int frame = slots[blockIdx.y].frame;
    pyramid_norm_select_body(acc + (size_t)frame * acc_stride, tables + frame, level, min_inside, recs + frame, nrecs + frame, exts + frame);
}

}  // namespace

namespace yh {

int scene_batch_pyramid_norm_reserve(yh_scene_batch* hb) {
    yh_scene* h = &hb->core;
    yh_scene_batch_memory* m = hb->memory;
    const size_t frames = (size_t)h->max_frames;
    // (the pooled levels, the tables of level bases and the records are the plain batched pyramid's; its level tables are not used)
    if (!m->pyr_maps) SCHK(h, hipMalloc((void**)&m->pyr_maps, frames * 2 * scene_pyramid_map_words(h->W, h->H) * 4));
    if (!m->pyr_table) SCHK(h, hipMalloc((void**)&m->pyr_table, frames * sizeof(ScenePyramidTable)));
    if (!m->reg_rec) SCHK(h, hipMalloc((void**)&m->reg_rec, frames * sizeof(SceneRegisterRecord)));
    if (!m->norm_rec) SCHK(h, hipMalloc((void**)&m->norm_rec, frames * sizeof(SceneRegisterNormRecord)));
    if (!m->pyrn_acc) SCHK(h, hipMalloc((void**)&m->pyrn_acc, frames * scene_pyramid_norm_acc_bytes()));
    if (!m->pyrn_ext) SCHK(h, hipMalloc((void**)&m->pyrn_ext, frames * sizeof(ScenePyramidNormExt)));
    return YH_OK;
}

int scene_batch_pyramid_norm_search(yh_scene_batch* hb, const SceneFuseParams* f) {
    yh_scene* h = &hb->core;
    yh_scene_batch_memory* m = hb->memory;
    const ScenePyramidPlan& plan = m->pyr;
    const int W = h->W, H = h->H, L = plan.levels;
    const size_t stride = pyramid_norm_acc_offset(plan, L + 1);   // <= scene_pyramid_norm_acc_bytes() / 8: the call's parameters have been checked
    SCHK(h, hipMemsetAsync(m->pyrn_acc, 0, (size_t)m->n * stride * sizeof(unsigned long long), h->stream));
    const SceneFuseSlot* slots = (const SceneFuseSlot*)m->table;
    const size_t words = scene_pyramid_map_words(W, H), npx = (size_t)W * H;
    const ScenePyramidTable* tables = m->pyr_table;
    ScenePyramidParams pp = {};
    for (size_t r = 0; r + 1 < m->round_off.size(); ++r) {
        const SceneFuseSlot* round = slots + m->round_off[r];
        const unsigned count = (unsigned)(m->round_off[r + 1] - m->round_off[r]);   // <= max_frames <= 256
        scene_batch_pyramid_levels_round(hb, L, round, count, pp);
        for (int l = L; l >= 0; --l) {
            SceneRegisterParams p;
            p.stamp = l ? pp.dst[0][l - 1] : m->stamp; p.mem = nullptr;
            p.acc = m->pyrn_acc + pyramid_norm_acc_offset(plan, l); p.W = pyramid_dim(W, l); p.H = pyramid_dim(H, l);
            const unsigned tiles = (unsigned)(((p.W + SR_TW - 1) / SR_TW) * ((p.H + SR_TH - 1) / SR_TH));
            const unsigned hyp = (unsigned)plan.hyp(l), rows = (unsigned)(2 * plan.rho(l) + 1);   // rows <= 17: count x rows <= 4352
            // The coarsest level's rows are spread over the grid whatever the round's size, as the single handle spreads them: split
            // or not gives the same bits (integer sums), and measured at 1, 8 and 64 frames a round the split is 0.14 ms a frame
            // ahead in a round of one frame and 0.001 behind in a round of 64 (profiles/scene_batch_pyramid_norm_timings.txt).
            if (l == L)
                hipLaunchKernelGGL(batch_pyramid_norm_scores_rows, dim3(tiles, hyp, count * rows), dim3(256), 0, h->stream, p, round, tables, l, (int)rows, 2 * words, words, stride);
            else if (l)
                hipLaunchKernelGGL(batch_pyramid_norm_scores<true>, dim3(tiles, hyp, count), dim3(256), 0, h->stream, p, round, tables, l, 2 * words, words, stride);
            else
                hipLaunchKernelGGL(batch_pyramid_norm_scores<false>, dim3(tiles, hyp, count), dim3(256), 0, h->stream, p, round, tables, 0, npx, (size_t)0, stride);
            hipLaunchKernelGGL(batch_pyramid_norm_select, dim3(l ? (unsigned)plan.n_rot : 1u, count), dim3(256), 0, h->stream, (const unsigned long long*)p.acc, round,
                               m->pyr_table, l, m->pyr_norm_min_inside, m->reg_rec, m->norm_rec, m->pyrn_ext, stride);
        }
        if (f) scene_batch_register_fuse_round(hb, *f, round, count);
    }
    SCHK(h, hipGetLastError());
    return YH_OK;
}

}  // namespace yh
