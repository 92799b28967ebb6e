// scene_batch_pyramid.hip — the scene batch's pyramid registration (DESIGN.md section 11 "Scene batch: pyramid registration"):
// yh_scene_batch_append_memory_pyramid is yh_scene_batch_append_memory with every frame's motion found coarse to fine on the device,
// exactly as n yh_scene_append_memory_pyramid calls in batch order find it. Frames of one stream form a chain: frame r of a stream
// is registered against the map frame r - 1 of that stream has just fused, so M is pooled round by round, not once per call. With R
// the most frames one stream has in the call and L levels, after the stamps and on the handle's stream:
//   (upload)                the n frames' tables of level bases, one copy (scene_batch_memory.hip; not when a call is replayed)
//   (clear)                 the level tables of all n frames, one memset (a frame's tables: acc_offset(L + 1) words from the last)
//   per round r:
//     batch_pyramid         grid (tiles of 64 x 16, 2 maps, frames of the round): pyramid_body, levels 1 .. L of the frame's N and
//                           of its M - the slot's mem_prev: the bank map or the predecessor's map slot
//     per level L .. 0:
//       batch_pyramid_scores  grid (tiles of the level, its hypotheses, frames of the round): register_scores_body, the bases read in
//                             place from the frame's table
//       batch_pyramid_select  grid (level > 0: n_rot, else 1; frames of the round): pyramid_select_body; at level 0 into the frame's record
//     batch_fuse_dev        (scene_batch_register.hip, unchanged) with g read from the frame's record
//   batch_balls_memory_dev  (scene_batch_register.hip, unchanged) ONE launch after the last round
// R (2 L + 4) + 1 launches and the stamps' four, against n (2 L + 10) frame by frame; no host wait. The entry points live with the
// bank's state in scene_batch_memory.hip.
#include <hip/hip_runtime.h>

#include "scene.h"
#include "scene_batch.h"
#include "scene_batch_memory.h"
#include "scene_memory_dev.h"
#include "scene_pyramid_dev.h"
#include "scene_register_dev.h"
#include "yh_internal.h"

using namespace yh;

namespace {

// p: src[0] the bank's stamps, dst the levels of frame 0 (those above p.levels are not touched). The frame comes from the grid and is
// uniform over the workgroup: the body's waves stay whole and its early returns uniform.
__global__ __launch_bounds__(256) void batch_pyramid(const ScenePyramidParams p, const SceneFuseSlot* __restrict__ slots, const size_t frame_words) {
    const SceneFuseSlot* e = slots + blockIdx.z;
    const int frame = e->frame;
    ScenePyramidParams q = p;
    q.src[0] += (size_t)frame * p.W * p.H;
    q.src[1] = e->mem_prev;
#pragma unroll
    for (int l = 0; l < SP_MAX_LEVELS; ++l) {
        if (l >= p.levels) break;
        q.dst[0][l] += (size_t)frame * frame_words; q.dst[1][l] += (size_t)frame * frame_words;
    }
    pyramid_body(q);
}

// p: W, H of the level; stamp = level `level` of frame 0's N (level 0: the bank's stamps), a frame frame_words further on; acc = the
// level's table of frame 0. POOLED (level > 0): a frame's M lies mem_off words behind its N; level 0: it is the slot's mem_prev. (Two
// instantiations, not a select of the two pointers: with the select the body's loops take 175 registers, without it the single
// handle's 119.) The bases stay where they are: the address is uniform over the workgroup, so the body's reads of the coefficients
// are scalar loads.
template <bool POOLED>
__global__ __launch_bounds__(256) void batch_pyramid_scores(const SceneRegisterParams p, const SceneFuseSlot* __restrict__ slots,
                                                            const ScenePyramidTable* __restrict__ tables, const int level, const size_t frame_words,
                                                            const size_t mem_off, const size_t acc_stride) {
    const SceneFuseSlot* e = slots + blockIdx.z;
    const int frame = e->frame;
    SceneRegisterParams q = p;
    q.stamp += (size_t)frame * frame_words;
    if (POOLED) q.mem = q.stamp + mem_off; else q.mem = e->mem_prev;
    q.acc += (size_t)frame * acc_stride;
    register_scores_body(q, tables[frame].lv[level]);
}

__global__ __launch_bounds__(256) void batch_pyramid_select(const unsigned long long* acc, const SceneFuseSlot* __restrict__ slots, ScenePyramidTable* tables,
                                                            const int level, SceneRegisterRecord* recs, const size_t acc_stride) {
    const int frame = slots[blockIdx.y].frame;
    pyramid_select_body(acc + (size_t)frame * acc_stride, tables + frame, level, recs + frame);
}

}  // namespace

namespace yh {

int scene_batch_pyramid_reserve(yh_scene_batch* hb) {
    yh_scene* h = &hb->core;
    yh_scene_batch_memory* m = hb->memory;
    const size_t frames = (size_t)h->max_frames;
    if (!m->pyr_maps) SCHK(h, hipMalloc((void**)&m->pyr_maps, frames * 2 * scene_pyramid_map_words(h->W, h->H) * 4));
    if (!m->pyr_acc) SCHK(h, hipMalloc((void**)&m->pyr_acc, frames * scene_pyramid_acc_bytes()));
    if (!m->pyr_table) SCHK(h, hipMalloc((void**)&m->pyr_table, frames * sizeof(ScenePyramidTable)));
    if (!m->reg_rec) SCHK(h, hipMalloc((void**)&m->reg_rec, frames * sizeof(SceneRegisterRecord)));
    return YH_OK;
}

void scene_batch_pyramid_levels_round(yh_scene_batch* hb, int levels, const SceneFuseSlot* round, unsigned count, ScenePyramidParams& pp) {
    yh_scene* h = &hb->core;
    yh_scene_batch_memory* m = hb->memory;
    const int W = h->W, H = h->H;
    const size_t words = scene_pyramid_map_words(W, H);
    pp = ScenePyramidParams{};
    pp.src[0] = m->stamp; pp.src[1] = nullptr; pp.W = W; pp.H = H; pp.levels = levels;
    for (int l = 1; l <= levels; ++l) {
        pp.dst[0][l - 1] = m->pyr_maps + scene_pyramid_map_offset(W, H, l);
        pp.dst[1][l - 1] = m->pyr_maps + words + scene_pyramid_map_offset(W, H, l);
    }
    const unsigned tiles0 = (unsigned)(((W + SP_TW - 1) / SP_TW) * ((H + SP_TH - 1) / SP_TH));   // <= 128 * 512
    hipLaunchKernelGGL(batch_pyramid, dim3(tiles0, 2, count), dim3(256), 0, h->stream, pp, round, 2 * words);
}

int scene_batch_pyramid_search(yh_scene_batch* hb, const SceneFuseParams* f) {
    yh_scene* h = &hb->core;
    yh_scene_batch_memory* m = hb->memory;
    const ScenePyramidPlan& plan = m->pyr;
    const int W = h->W, H = h->H, L = plan.levels;
    const size_t stride = plan.acc_offset(L + 1);   // <= scene_pyramid_acc_bytes() / 8: the call's parameters have been checked
    SCHK(h, hipMemsetAsync(m->pyr_acc, 0, (size_t)m->n * stride * sizeof(unsigned long long), h->stream));
    const SceneFuseSlot* slots = (const SceneFuseSlot*)m->table;
    const size_t words = scene_pyramid_map_words(W, H), npx = (size_t)W * H;
    ScenePyramidParams pp = {};
    for (size_t r = 0; r + 1 < m->round_off.size(); ++r) {
        const SceneFuseSlot* round = slots + m->round_off[r];
        const unsigned count = (unsigned)(m->round_off[r + 1] - m->round_off[r]);   // <= max_frames <= 256
        scene_batch_pyramid_levels_round(hb, L, round, count, pp);
        for (int l = L; l >= 0; --l) {
            SceneRegisterParams p;
            p.stamp = l ? pp.dst[0][l - 1] : m->stamp; p.mem = nullptr;
            p.acc = m->pyr_acc + plan.acc_offset(l); p.W = pyramid_dim(W, l); p.H = pyramid_dim(H, l);
            const unsigned tiles = (unsigned)(((p.W + SR_TW - 1) / SR_TW) * ((p.H + SR_TH - 1) / SR_TH));
            const dim3 grid(tiles, (unsigned)plan.hyp(l), count);
            if (l) hipLaunchKernelGGL(batch_pyramid_scores<true>, grid, dim3(256), 0, h->stream, p, round, (const ScenePyramidTable*)m->pyr_table, l, 2 * words, words, stride);
            else hipLaunchKernelGGL(batch_pyramid_scores<false>, grid, dim3(256), 0, h->stream, p, round, (const ScenePyramidTable*)m->pyr_table, 0, npx, (size_t)0, stride);
            hipLaunchKernelGGL(batch_pyramid_select, dim3(l ? (unsigned)plan.n_rot : 1u, count), dim3(256), 0, h->stream,
                               (const unsigned long long*)p.acc, round, m->pyr_table, l, m->reg_rec, stride);
        }
        if (f) scene_batch_register_fuse_round(hb, *f, round, count);
    }
    SCHK(h, hipGetLastError());
    return YH_OK;
}

}  // namespace yh
