// scene_batch_register.hip — the scene batch's registration (DESIGN.md section 11 "Scene batch: registration"):
// yh_scene_batch_append_memory_search is yh_scene_batch_append_memory with every frame's motion found on the device, exactly as n
// yh_scene_append_memory_search calls in batch order find it. Frames of one stream form a chain: frame r of a stream is scored
// against the map frame r - 1 of that stream has just fused, so the rounds of the memory append (scene_batch_memory.hip) each gain
// two launches in front of their fuse. With R the most frames one stream has in the call, after the stamps and on the handle's stream:
//   (clear)                  sum_n and the score tables of all n frames, one memset (a frame's table: stride words from the last)
//   per round r:
//     batch_register_scores  grid (tiles of 64 x 16, n_rot, frames of the round): register_scores_body, frame z's N, M and table
//                            taken from the round's device slots, its bases read in place from the device table
//     batch_register_select  a workgroup per frame of the round: register_select_body into the frame's record
//     batch_fuse_dev         batch_fuse with g read from the frame's record
//   batch_balls_memory_dev   ONE launch after the last round: batch_balls_memory with each step's c read from its frame's record
// 3 R + 6 launches with the four of the stamps, against 9 n frame by frame; no host wait. The entry points live with the bank's
// state in scene_batch_memory.hip.
#include <hip/hip_runtime.h>

#include "scene.h"
#include "scene_batch.h"
#include "scene_batch_memory.h"
#include "scene_memory_dev.h"
#include "scene_register_dev.h"
#include "yh_internal.h"

using namespace yh;

namespace {

// M of a slot: the stream's bank map for its first frame in the call, the predecessor's map slot (complete since the previous
// round's fuse, unfaded) for a later one - what the round's fuse gathers from. The bases stay where they are: the address is
// uniform over the workgroup, so the body's reads of the coefficients are scalar loads.
__global__ __launch_bounds__(256) void batch_register_scores(const SceneRegisterParams p, const SceneFuseSlot* __restrict__ slots,
                                                             const SceneRegisterBases* __restrict__ bases, const size_t acc_stride) {
    const SceneFuseSlot* e = slots + blockIdx.z;
    const int frame = e->frame;
    SceneRegisterParams q = p;
    q.stamp += (size_t)frame * p.W * p.H;
    q.mem = e->mem_prev;
    q.acc += (size_t)frame * acc_stride;
    register_scores_body(q, bases[frame]);
}

__global__ __launch_bounds__(256) void batch_register_select(const unsigned long long* acc, const SceneFuseSlot* __restrict__ slots,
                                                             const SceneRegisterBases* __restrict__ bases, SceneRegisterRecord* recs, const size_t acc_stride) {
    const int frame = slots[blockIdx.x].frame;
    register_select_body(acc + (size_t)frame * acc_stride, bases[frame], recs + frame);
}

__global__ __launch_bounds__(256) void batch_fuse_dev(const SceneFuseParams p, const SceneFuseSlot* __restrict__ slots, const SceneRegisterRecord* __restrict__ recs) {
    const SceneFuseSlot e = slots[blockIdx.z];
    const size_t o = (size_t)e.frame * p.W * p.H;
    SceneFuseParams q = p;
    q.stamp += o; q.map += o; q.world += o; q.conn0 += o; q.conn1 += o;
    q.mem_prev = e.mem_prev; q.mem_next = e.mem_next;
    const SceneRegisterRecord* rec = recs + e.frame;
#pragma unroll
    for (int i = 0; i < 6; ++i) q.g[i] = rec->g[i];
    fuse_body(q);
}

__global__ __launch_bounds__(128) void batch_balls_memory_dev(const SceneBallsMemParams p, const SceneBallsChain* __restrict__ chains,
                                                              const SceneBallsStep* __restrict__ steps, const SceneRegisterRecord* __restrict__ recs, int4* tabs) {
    const SceneBallsChain ch = chains[blockIdx.x];
    const int4* prev = ch.tab_prev;
    for (int j = 0; j < ch.count; ++j) {   // (lane k reads what lane k wrote: the chain needs no barrier)
        const int frame = steps[ch.first + j].frame;
        SceneBallsMemParams q = p;
        q.ball_acc += (size_t)frame * 300; q.balls += (size_t)frame * 100;
        q.tab_prev = prev; q.tab_next = tabs + (size_t)frame * 100;
        const SceneRegisterRecord* rec = recs + frame;
#pragma unroll
        for (int i = 0; i < 6; ++i) q.c[i] = rec->c[i];
        balls_memory_body(q);
        prev = q.tab_next;
    }
    if (threadIdx.x < 100) ch.tab_next[threadIdx.x] = prev[threadIdx.x];
}

}  // namespace

namespace yh {

int scene_batch_register_reserve(yh_scene_batch* hb) {
    yh_scene* h = &hb->core;
    yh_scene_batch_memory* m = hb->memory;
    if (!m->reg_acc) SCHK(h, hipMalloc((void**)&m->reg_acc, (size_t)h->max_frames * scene_register_acc_bytes()));
    if (!m->reg_rec) SCHK(h, hipMalloc((void**)&m->reg_rec, (size_t)h->max_frames * sizeof(SceneRegisterRecord)));
    return YH_OK;
}

void scene_batch_register_fuse_round(yh_scene_batch* hb, const SceneFuseParams& f, const SceneFuseSlot* round, unsigned count) {
    yh_scene* h = &hb->core;
    const unsigned gx = (unsigned)((h->W + SF_TW - 1) / SF_TW), gy = (unsigned)((h->H + SF_TH - 1) / SF_TH);
    hipLaunchKernelGGL(batch_fuse_dev, dim3(gx, gy, count), dim3(256), 0, h->stream, f, round, (const SceneRegisterRecord*)hb->memory->reg_rec);
}

int scene_batch_register_search(yh_scene_batch* hb, const SceneFuseParams* f) {
    yh_scene* h = &hb->core;
    yh_scene_batch_memory* m = hb->memory;
    const size_t stride = m->acc_stride();   // <= scene_register_acc_bytes() / 8: n_rot and radius have been checked
    SCHK(h, hipMemsetAsync(m->reg_acc, 0, (size_t)m->n * stride * sizeof(unsigned long long), h->stream));
    const SceneFuseSlot* slots = (const SceneFuseSlot*)m->table;
    const SceneRegisterBases* bases = (const SceneRegisterBases*)(m->table + scene_batch_bases_offset(h));
    SceneRegisterParams p;
    p.stamp = m->stamp; p.mem = nullptr; p.acc = m->reg_acc; p.W = h->W; p.H = h->H;
    const unsigned tiles = (unsigned)(((h->W + SR_TW - 1) / SR_TW) * ((h->H + SR_TH - 1) / SR_TH));   // <= 128 * 512
    for (size_t r = 0; r + 1 < m->round_off.size(); ++r) {
        const SceneFuseSlot* round = slots + m->round_off[r];
        const unsigned count = (unsigned)(m->round_off[r + 1] - m->round_off[r]);   // <= max_frames <= 256
        hipLaunchKernelGGL(batch_register_scores, dim3(tiles, (unsigned)m->n_rot, count), dim3(256), 0, h->stream, p, round, bases, stride);
        hipLaunchKernelGGL(batch_register_select, dim3(count), dim3(256), 0, h->stream, (const unsigned long long*)m->reg_acc, round, bases, m->reg_rec, stride);
        if (f) scene_batch_register_fuse_round(hb, *f, round, count);
    }
    SCHK(h, hipGetLastError());
    return YH_OK;
}

int scene_batch_register_balls(yh_scene_batch* hb, const SceneBallsMemParams& b) {
    yh_scene* h = &hb->core;
    yh_scene_batch_memory* m = hb->memory;
    const SceneBallsStep* steps = (const SceneBallsStep*)(m->table + scene_batch_slots_bytes(h));
    const SceneBallsChain* chains = (const SceneBallsChain*)(m->table + scene_batch_slots_bytes(h) + scene_batch_steps_bytes(h));
    hipLaunchKernelGGL(batch_balls_memory_dev, dim3((unsigned)m->chains), dim3(128), 0, h->stream, b, chains, steps, (const SceneRegisterRecord*)m->reg_rec, m->tabs);
    SCHK(h, hipGetLastError());
    return YH_OK;
}

}  // namespace yh
