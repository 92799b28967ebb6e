// scene_batch_register_norm.hip — the scene batch's normalised registration (DESIGN.md section 11 "Scene batch: normalised
// registration"): yh_scene_batch_append_memory_search_norm is yh_scene_batch_append_memory_search (scene_batch_register.hip) with
// the single handle's normalised bodies (scene_register_norm_dev.h) in place of the plain ones, exactly as n
// yh_scene_append_memory_search_norm calls in batch order. The schedule, the device table, the fuse and the ball chains are the plain
// batched search's. With R the most frames one stream has in the call, after the stamps and on the handle's stream:
//   (clear)                       sum_n and the S, T and C tables of all n frames, one memset (a frame's: stride words from the last)
//   per round r:
//     batch_register_norm_scores  grid (tiles of 64 x 16, n_rot, frames of the round): register_norm_scores_body, frame z's N, M and
//                                 tables taken from the round's device slots, its bases read in place from the device table
//     batch_register_norm_select  a workgroup per frame of the round: register_norm_select_body into the frame's two records
//     batch_fuse_dev              (scene_batch_register.hip, unchanged) with g read from the frame's record
//   batch_balls_memory_dev        (scene_batch_register.hip, unchanged) ONE launch after the last round
// 3 R + 6 launches with the four of the stamps, as the plain batched search; no host wait. The entry points live with the bank's
// state in scene_batch_memory.hip.
#include <hip/hip_runtime.h>

#include "scene.h"
#include "scene_batch.h"
#include "scene_batch_memory.h"
#include "scene_memory_dev.h"
#include "scene_register_norm_dev.h"
#include "yh_internal.h"

using namespace yh;

namespace {

// The frame comes from the grid and is uniform over the workgroup; only the three pointers of the parameters change. The bases
// stay where they are: the address is uniform, so the body's reads of the coefficients are scalar loads.
__global__ __launch_bounds__(256, 4) void batch_register_norm_scores(const SceneRegisterParams p, const SceneFuseSlot* __restrict__ slots,
                                                                     const SceneRegisterBases* __restrict__ bases, const size_t acc_stride) {
    const SceneFuseSlot* e = slots + blockIdx.z;
    const int frame = e->frame;
    SceneRegisterParams q = p;
    q.stamp += (size_t)frame * p.W * p.H;
    q.mem = e->mem_prev;
    q.acc += (size_t)frame * acc_stride;
    register_norm_scores_body(q, bases[frame]);
}

__global__ __launch_bounds__(256) void batch_register_norm_select(const unsigned long long* acc, const SceneFuseSlot* __restrict__ slots,
                                                                  const SceneRegisterBases* __restrict__ bases, const int min_inside, SceneRegisterRecord* recs,
                                                                  SceneRegisterNormRecord* exts, const size_t acc_stride) {
    const int frame = slots[blockIdx.x].frame;
    register_norm_select_body(acc + (size_t)frame * acc_stride, bases[frame], min_inside, recs + frame, exts + frame);
}

}  // namespace

namespace yh {

int scene_batch_register_norm_reserve(yh_scene_batch* hb) {
    yh_scene* h = &hb->core;
    yh_scene_batch_memory* m = hb->memory;
    const size_t frames = (size_t)h->max_frames;
    if (!m->norm_acc) SCHK(h, hipMalloc((void**)&m->norm_acc, frames * scene_register_norm_acc_bytes()));
    if (!m->norm_rec) SCHK(h, hipMalloc((void**)&m->norm_rec, frames * sizeof(SceneRegisterNormRecord)));
    if (!m->reg_rec) SCHK(h, hipMalloc((void**)&m->reg_rec, frames * sizeof(SceneRegisterRecord)));
    return YH_OK;
}

int scene_batch_register_norm_search(yh_scene_batch* hb, const SceneFuseParams* f) {
    yh_scene* h = &hb->core;
    yh_scene_batch_memory* m = hb->memory;
    const size_t stride = m->acc_stride();   // <= scene_register_norm_acc_bytes() / 8: n_rot and radius have been checked
    SCHK(h, hipMemsetAsync(m->norm_acc, 0, (size_t)m->n * stride * sizeof(unsigned long long), h->stream));
    const SceneFuseSlot* slots = (const SceneFuseSlot*)m->table;
    const SceneRegisterBases* bases = (const SceneRegisterBases*)(m->table + scene_batch_bases_offset(h));
    SceneRegisterParams p;
    p.stamp = m->stamp; p.mem = nullptr; p.acc = m->norm_acc; p.W = h->W; p.H = h->H;
    const unsigned tiles = (unsigned)(((h->W + SR_TW - 1) / SR_TW) * ((h->H + SR_TH - 1) / SR_TH));   // <= 128 * 512
    for (size_t r = 0; r + 1 < m->round_off.size(); ++r) {
        const SceneFuseSlot* round = slots + m->round_off[r];
        const unsigned count = (unsigned)(m->round_off[r + 1] - m->round_off[r]);   // <= max_frames <= 256
        hipLaunchKernelGGL(batch_register_norm_scores, dim3(tiles, (unsigned)m->n_rot, count), dim3(256), 0, h->stream, p, round, bases, stride);
        hipLaunchKernelGGL(batch_register_norm_select, dim3(count), dim3(256), 0, h->stream, (const unsigned long long*)m->norm_acc, round, bases, m->norm_min_inside,
                           m->reg_rec, m->norm_rec, stride);
        if (f) scene_batch_register_fuse_round(hb, *f, round, count);
    }
    SCHK(h, hipGetLastError());
    return YH_OK;
}

}  // namespace yh
