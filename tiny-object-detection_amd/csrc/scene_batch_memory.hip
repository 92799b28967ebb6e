// scene_batch_memory.hip — the scene batch's memory (DESIGN.md section 11 "Scene batch: memory"): a yh_scene_batch holds a bank of
// YH_SCENE_STREAMS_MAX memories, one per camera stream, each what a yh_scene holds (scene_memory.hip). yh_scene_batch_append_memory on
// n staged frames is exactly n yh_scene_append_memory calls in batch order, frame b on the memory of streams[b]: frames of different
// streams share launches, frames of one stream form a chain on the device. With R the most frames one stream has in the call:
//   stamps                two memsets, batch_cloud_strips, batch_balls for all n frames (scene_batch.hip: scene_batch_stamp), into the
//                         bank's own array N [max_frames][H][W] (a tile's halo reads N of pixels whose F a neighbour is writing);
//   batch_balls_memory    ONE launch: a workgroup per stream of the call walks the stream's frames in batch order, a lane per ball id
//                         (balls_memory_body per frame; frame k reads the table frame k - 1 wrote, the first the bank's); tables are
//                         kept per frame, the last one is the bank's new table. It depends on the stamps' balls only;
//   batch_fuse            R launches, one per round r: grid z runs over the frames whose rank within their stream is r, a device
//                         table gives each z its frame, its motion and its source (fuse_body, the single handle's body). A rank-0
//                         frame gathers from the stream's bank map, a later one from its predecessor's map slot, complete since the
//                         previous launch; only a stream's last frame writes the bank.
// R + 5 launches against 6 n frame by frame. The bank keeps two maps and two tables per stream (allocated at the stream's first use)
// which swap at every call that names the stream: the state a call started from survives it, and yh_scene_batch_memory_time replays
// the same launches from it and rewrites the same bits.
// yh_scene_batch_append_memory_search (DESIGN.md section 11 "Scene batch: registration") is the same append with every frame's
// motion found on the device: the same schedule, its slots and steps without motions and the frames' bases behind the chains in the
// one upload; each round's fuse is preceded by the round's scores and choice, and the ball chains run last, on the records
// (scene_batch_register.hip). yh_scene_batch_append_memory_pyramid (DESIGN.md section 11 "Scene batch: pyramid registration") is that
// again with each round's motions found coarse to fine (scene_batch_pyramid.hip): the frames' tables of level bases go up in a copy
// of their own. yh_scene_batch_append_memory_search_norm and _pyramid_norm (DESIGN.md section 11 "Scene batch: normalised
// registration", "Scene batch: normalised pyramid registration") are those two with every choice made by the single handle's
// normalised score among the candidates that keep min_inside pixels inside (scene_batch_register_norm.hip,
// scene_batch_pyramid_norm.hip): the same schedule, uploads and launches. The bank's state is in scene_batch_memory.h for the units.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "scene.h"
#include "scene_batch.h"
#include "scene_batch_memory.h"
#include "scene_dev.h"
#include "scene_memory_dev.h"
#include "scene_pyramid_dev.h"
#include "yh_internal.h"

using namespace yh;

namespace {

__global__ __launch_bounds__(256) void batch_fuse(const SceneFuseParams p, const SceneFuseSlot* __restrict__ slots) {
    const SceneFuseSlot e = slots[blockIdx.z];
    const size_t o = (size_t)e.frame * p.W * p.H;
    SceneFuseParams q = p;
    q.stamp += o; q.map += o; q.world += o; q.conn0 += o; q.conn1 += o;
    q.mem_prev = e.mem_prev; q.mem_next = e.mem_next;
#pragma unroll
    for (int i = 0; i < 6; ++i) q.g[i] = e.g[i];
    fuse_body(q);
}

__global__ __launch_bounds__(128) void batch_balls_memory(const SceneBallsMemParams p, const SceneBallsChain* __restrict__ chains,
                                                          const SceneBallsStep* __restrict__ steps, int4* tabs) {
    const SceneBallsChain ch = chains[blockIdx.x];
    const int4* prev = ch.tab_prev;
    for (int j = 0; j < ch.count; ++j) {   // (lane k reads what lane k wrote: the chain needs no barrier)
        const SceneBallsStep s = steps[ch.first + j];
        SceneBallsMemParams q = p;
        q.ball_acc += (size_t)s.frame * 300; q.balls += (size_t)s.frame * 100;
        q.tab_prev = prev; q.tab_next = tabs + (size_t)s.frame * 100;
#pragma unroll
        for (int i = 0; i < 6; ++i) q.c[i] = s.c[i];
        balls_memory_body(q);
        prev = q.tab_next;
    }
    if (threadIdx.x < 100) ch.tab_next[threadIdx.x] = prev[threadIdx.x];
}

size_t slots_bytes(const yh_scene* h) { return scene_batch_slots_bytes(h); }
size_t steps_bytes(const yh_scene* h) { return scene_batch_steps_bytes(h); }

// the buffers every memory append uses, at the first one: a batch that never remembers pays nothing
// (a search: the score tables and records too, and the device table grows by the frames' bases - the stream is drained before
// the smaller one goes, and whoever fails after this leaves nothing to replay; a pyramid append: its own buffers instead)
int memory_reserve(yh_scene_batch* hb, bool search, bool pyramid, bool norm) {
    yh_scene* h = &hb->core;
    if (!hb->memory) hb->memory = new yh_scene_batch_memory();
    yh_scene_batch_memory* m = hb->memory;
    const size_t all = (size_t)h->max_frames * h->W * h->H;
    if (!m->stamp) SCHK(h, hipMalloc((void**)&m->stamp, all * 4));
    if (!m->tabs) SCHK(h, hipMalloc((void**)&m->tabs, (size_t)h->max_frames * 100 * sizeof(int4)));
    const size_t need = scene_batch_bases_offset(h) + (search ? (size_t)h->max_frames * sizeof(SceneRegisterBases) : 0);
    if (m->table_bytes < need) {
        if (m->table) {
            SCHK(h, hipStreamSynchronize(h->stream));
            unsigned char* old = m->table;
            m->table = nullptr; m->table_bytes = 0;
            SCHK(h, hipFree(old));
        }
        SCHK(h, hipMalloc((void**)&m->table, need));
        m->table_bytes = need;
    }
    if (pyramid) return norm ? scene_batch_pyramid_norm_reserve(hb) : scene_batch_pyramid_reserve(hb);
    if (search) return norm ? scene_batch_register_norm_reserve(hb) : scene_batch_register_reserve(hb);
    return YH_OK;
}

// one stream's two maps and two tables, at its first use; cleared if they are fresh or stale
int stream_reserve(yh_scene_batch* hb, int s) {
    yh_scene* h = &hb->core;
    BankStream& k = hb->memory->bank[s];
    const size_t npx = (size_t)h->W * h->H;
    for (int i = 0; i < 2; ++i) {
        if (!k.map[i]) SCHK(h, hipMalloc((void**)&k.map[i], npx * 4));
        if (!k.tab[i]) SCHK(h, hipMalloc((void**)&k.tab[i], 100 * sizeof(int4)));
    }
    if (!k.stale) return YH_OK;
    for (int i = 0; i < 2; ++i) {
        SCHK(h, hipMemsetAsync(k.map[i], 0, npx * 4, h->stream));
        SCHK(h, hipMemsetAsync(k.tab[i], 0, 100 * sizeof(int4), h->stream));
    }
    k.stale = false;
    return YH_OK;
}

// the registration launches of the last scheduled searching append (with f: each round's fuse behind them)
int registration(yh_scene_batch* hb, const SceneFuseParams* f) {
    const yh_scene_batch_memory* m = hb->memory;
    if (m->pyr_norm_min_inside) return scene_batch_pyramid_norm_search(hb, f);
    if (m->pyramid) return scene_batch_pyramid_search(hb, f);
    return m->norm_min_inside ? scene_batch_register_norm_search(hb, f) : scene_batch_register_search(hb, f);
}

// the launches of the last scheduled memory append, from the device tables as they stand
int run_memory(yh_scene_batch* hb) {
    yh_scene* h = &hb->core;
    yh_scene_batch_memory* m = hb->memory;
    SceneParams p;
    p.depth = h->depth; p.cls_id = nullptr; p.frame = h->frame; p.frame_mode = 1;
    p.W = h->W; p.H = h->H; p.mode = YH_COMPAT_SANE; p.band_h = h->band_h;
    p.terrain_tab = h->terrain_tab; p.robot_tab = h->robot_tab;
    p.map = m->stamp; p.world = h->world; p.conn0 = h->conn0; p.conn1 = h->conn1; p.ball_acc = h->ball_acc; p.balls = h->balls;
    const int rc = scene_batch_stamp(hb, p, m->n);
    if (rc) return rc;
    const SceneFuseSlot* slots = (const SceneFuseSlot*)m->table;
    const SceneBallsStep* steps = (const SceneBallsStep*)(m->table + slots_bytes(h));
    const SceneBallsChain* chains = (const SceneBallsChain*)(m->table + slots_bytes(h) + steps_bytes(h));
    SceneBallsMemParams b;
    b.ball_acc = h->ball_acc; b.balls = h->balls; b.tab_prev = nullptr; b.tab_next = nullptr;
    b.W = h->W; b.H = h->H; b.max_age = m->max_age;
    SceneFuseParams f;
    f.stamp = m->stamp; f.mem_prev = nullptr; f.mem_next = nullptr;
    f.map = h->map; f.world = h->world; f.conn0 = h->conn0; f.conn1 = h->conn1;
    f.W = h->W; f.H = h->H; f.keep = m->keep;
    for (int i = 0; i < 6; ++i) { b.c[i] = 0; f.g[i] = 0; }
    if (m->searched || m->pyramid || m->pyr_norm_min_inside) {   // the motions are found round by round; the ball chains need every frame's record
        const int rs = registration(hb, &f);
        return rs ? rs : scene_batch_register_balls(hb, b);
    }
    hipLaunchKernelGGL(batch_balls_memory, dim3((unsigned)m->chains), dim3(128), 0, h->stream, b, chains, steps, m->tabs);
    const unsigned gx = (unsigned)((h->W + SF_TW - 1) / SF_TW), gy = (unsigned)((h->H + SF_TH - 1) / SF_TH);
    for (size_t r = 0; r + 1 < m->round_off.size(); ++r)
        hipLaunchKernelGGL(batch_fuse, dim3(gx, gy, (unsigned)(m->round_off[r + 1] - m->round_off[r])), dim3(256), 0, h->stream, f, slots + m->round_off[r]);
    SCHK(h, hipGetLastError());
    return YH_OK;
}

int stream_of(const int32_t* streams, int b) { return streams ? streams[b] : 0; }

// n_rot 0: gather and carry are one motion per frame. Otherwise n_rot bases per frame, searched around with `radius`: the slots and
// steps carry no motion (the kernels read each frame's from its record) and the frames' bases follow the chains in the one upload.
// plans given: a pyramid append, frame b's table of level bases in plans[b]; the slots and steps carry no motion either, there are no
// plain bases, and the tables go up in a second copy. min_inside != 0: the normalised form of the search or of the pyramid append.
int append_memory(yh_scene_batch* hb, int n, const int32_t* streams, const int32_t* gather, const int32_t* carry, int keep, int max_age, int n_rot = 0, int radius = 0,
                  const std::vector<ScenePyramidPlan>* plans = nullptr, int min_inside = 0) {
    yh_scene* h = &hb->core;
    SCHK(h, hipSetDevice(h->dev));
    const bool search = n_rot > 0 && !plans, given = n_rot == 0;
    int rc = memory_reserve(hb, search, plans != nullptr, min_inside != 0);
    if (rc) return rc;
    yh_scene_batch_memory* m = hb->memory;
    // the schedule: the frames of every stream in batch order; R rounds
    std::vector<int> frames_of[YH_SCENE_STREAMS_MAX];
    std::vector<int> named;   // the streams in the order of their first frame
    size_t R = 0;
    for (int b = 0; b < n; ++b) {
        std::vector<int>& f = frames_of[stream_of(streams, b)];
        if (f.empty()) named.push_back(stream_of(streams, b));
        f.push_back(b);
        R = f.size() > R ? f.size() : R;
    }
    for (int s : named)
        if ((rc = stream_reserve(hb, s))) return rc;
    const size_t npx = (size_t)h->W * h->H;
    m->table_host.assign(scene_batch_bases_offset(h) + (search ? (size_t)n * sizeof(SceneRegisterBases) : 0), 0);
    SceneFuseSlot* slots = (SceneFuseSlot*)m->table_host.data();
    SceneBallsStep* steps = (SceneBallsStep*)(m->table_host.data() + slots_bytes(h));
    SceneBallsChain* chains = (SceneBallsChain*)(m->table_host.data() + slots_bytes(h) + steps_bytes(h));
    m->round_off.assign(1, 0);
    int total = 0;
    for (size_t r = 0; r < R; ++r) {
        for (int s : named) {
            const std::vector<int>& f = frames_of[s];
            if (r >= f.size()) continue;
            const BankStream& k = m->bank[s];
            SceneFuseSlot& e = slots[total++];
            e.mem_prev = r == 0 ? k.map[k.cur] : h->map + (size_t)f[r - 1] * npx;
            e.mem_next = r + 1 == f.size() ? k.map[k.cur ^ 1] : nullptr;
            e.frame = f[r];
            for (int i = 0; i < 6 && given; ++i) e.g[i] = gather[6 * f[r] + i];
        }
        m->round_off.push_back(total);
    }
    total = 0;
    m->chains = 0;
    for (int s : named) {
        const BankStream& k = m->bank[s];
        chains[m->chains++] = SceneBallsChain{ k.tab[k.cur], k.tab[k.cur ^ 1], total, (int)frames_of[s].size() };
        for (int b : frames_of[s]) {
            SceneBallsStep& e = steps[total++];
            e.frame = b;
            for (int i = 0; i < 6 && given; ++i) e.c[i] = carry[6 * b + i];
        }
    }
    if (search) {
        SceneRegisterBases* bases = (SceneRegisterBases*)(m->table_host.data() + scene_batch_bases_offset(h));
        for (int b = 0; b < n; ++b) {
            bases[b].n_rot = n_rot; bases[b].radius = radius;
            for (int k = 0; k < n_rot; ++k)
                for (int i = 0; i < 6; ++i) {
                    bases[b].g[k][i] = gather[((size_t)b * n_rot + k) * 6 + i];
                    bases[b].c[k][i] = carry[((size_t)b * n_rot + k) * 6 + i];
                }
        }
    }
    m->n = n; m->keep = keep; m->max_age = max_age;
    m->searched = search; m->n_rot = n_rot; m->radius = radius;
    m->pyramid = plans != nullptr && !min_inside;
    m->norm_min_inside = search ? min_inside : 0;
    m->pyr_norm_min_inside = plans ? min_inside : 0;
    // (from pageable memory: staged by the runtime before the call returns, as the caller's own arrays have been read by now)
    SCHK(h, hipMemcpyAsync(m->table, m->table_host.data(), m->table_host.size(), hipMemcpyHostToDevice, h->stream));
    if (plans) {
        m->pyr = (*plans)[0];   // (n_rot, levels, radius and refine are the call's)
        m->pyr_host.resize((size_t)n);
        for (int b = 0; b < n; ++b) m->pyr_host[b] = (*plans)[b].table;
        SCHK(h, hipMemcpyAsync(m->pyr_table, m->pyr_host.data(), (size_t)n * sizeof(ScenePyramidTable), hipMemcpyHostToDevice, h->stream));
    }
    if ((rc = run_memory(hb))) return rc;
    for (int s : named) m->bank[s].cur ^= 1;
    return YH_OK;
}

int stream_ok(yh_scene_batch* hb, int32_t stream, int lowest) {
    if (stream < lowest || stream >= YH_SCENE_STREAMS_MAX)
        return hb->fail(YH_EINVAL, "stream " + std::to_string(stream) + " outside 0 .. " + std::to_string(YH_SCENE_STREAMS_MAX - 1));
    return YH_OK;
}

}  // namespace

namespace yh {
void scene_batch_memory_free(yh_scene_batch* hb) {
    yh_scene_batch_memory* m = hb->memory;
    if (!m) return;
    for (BankStream& k : m->bank) {
        void* bufs[] = { k.map[0], k.map[1], k.tab[0], k.tab[1] };
        for (void* b : bufs) if (b) hipFree(b);
    }
    void* bufs[] = { m->stamp, m->tabs, m->table, m->reg_acc, m->reg_rec, m->pyr_maps, m->pyr_acc, m->pyr_table, m->norm_acc, m->norm_rec, m->pyrn_acc, m->pyrn_ext };
    for (void* b : bufs) if (b) hipFree(b);
    delete m;
    hb->memory = nullptr;
}

bool scene_batch_memory_is_last(const yh_scene_batch* hb) { return hb->memory && hb->memory->frame != 0 && hb->memory->frame == hb->core.frames; }
bool scene_batch_memory_is_search(const yh_scene_batch* hb) { return scene_batch_memory_is_last(hb) && hb->memory->searched; }
bool scene_batch_memory_is_pyramid(const yh_scene_batch* hb) { return scene_batch_memory_is_last(hb) && hb->memory->pyramid; }
bool scene_batch_memory_is_norm(const yh_scene_batch* hb) { return scene_batch_memory_is_search(hb) && hb->memory->norm_min_inside != 0; }
bool scene_batch_memory_is_pyramid_norm(const yh_scene_batch* hb) { return scene_batch_memory_is_last(hb) && hb->memory->pyr_norm_min_inside != 0; }
}  // namespace yh

namespace {

// the checks both memory appends share, for every frame before anything is touched
int append_memory_checks(yh_scene_batch* hb, int32_t n_frames, const int32_t* streams, const int32_t* gather_q16, const int32_t* carry_q16, int32_t keep, int32_t ball_max_age) {
    yh_scene* h = &hb->core;
    if (!gather_q16 || !carry_q16) return h->fail(YH_EINVAL, "null motion array");
    if (n_frames < 1 || n_frames > h->max_frames) return h->fail(YH_EINVAL, "n_frames " + std::to_string(n_frames) + " outside 1 .. " + std::to_string(h->max_frames));
    if (keep < 0 || keep > 256) return h->fail(YH_EINVAL, "keep outside 0 .. 256");
    if (ball_max_age < 0 || ball_max_age > 255) return h->fail(YH_EINVAL, "ball_max_age outside 0 .. 255");
    for (int b = 0; b < n_frames; ++b) {
        if (streams && (streams[b] < 0 || streams[b] >= YH_SCENE_STREAMS_MAX))
            return h->fail(YH_EINVAL, "frame " + std::to_string(b) + ": stream " + std::to_string(streams[b]) + " outside 0 .. " + std::to_string(YH_SCENE_STREAMS_MAX - 1));
        if (!hb->staged[b]) return h->fail(YH_ESTATE, "slot " + std::to_string(b) + " has never been staged");
    }
    return YH_OK;
}

// what all five do around append_memory once the checks have passed (n_rot 0: the motions are given; plans: a pyramid append;
// min_inside != 0: a normalised one)
int append_memory_call(yh_scene_batch* hb, int32_t n_frames, const int32_t* streams, const int32_t* gather_q16, const int32_t* carry_q16,
                       int32_t keep, int32_t ball_max_age, int32_t n_rot, int32_t radius, const std::vector<ScenePyramidPlan>* plans = nullptr,
                       int32_t min_inside = 0) {
    yh_scene* h = &hb->core;
    ++h->frames;   // (earlier plans are of other frames, whatever becomes of these)
    const int rc = append_memory(hb, n_frames, streams, gather_q16, carry_q16, keep, ball_max_age, n_rot, radius, plans, min_inside);
    yh_scene_batch_memory* m = hb->memory;
    if (rc) {
        // a call that fails after its checks leaves no frame and empties the memories of the streams it named
        h->ran = false; hb->n = 0;
        if (m) {
            m->frame = 0; m->replayable = false; m->searched = false; m->pyramid = false; m->norm_min_inside = 0; m->pyr_norm_min_inside = 0;
            for (int b = 0; b < n_frames; ++b) m->bank[stream_of(streams, b)].stale = true;
        }
        return rc;
    }
    m->frame = h->frames; m->stagings = hb->stagings; m->replayable = true;
    h->ran = true; h->last_mode = YH_COMPAT_SANE;
    hb->n = n_frames; hb->from_fields = false;
    std::fill(hb->diag_ok.begin(), hb->diag_ok.end(), (uint8_t)1);   // (F is a height map like any other: both ends of a diagonal hold the same length)
    return YH_OK;
}

// `reps` runs of `run` between two events on the handle's stream; a failure leaves no frame and nothing to replay
template <class Run>
int replay_time(yh_scene_batch* hb, int reps, Run run, float* ms_out) {
    yh_scene* h = &hb->core;
    yh_scene_batch_memory* m = hb->memory;
    struct Events { hipEvent_t a = nullptr, b = nullptr; ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev;
    SCHK(h, hipEventCreate(&ev.a)); SCHK(h, hipEventCreate(&ev.b));
    SCHK(h, hipEventRecord(ev.a, h->stream));
    for (int r = 0; r < reps; ++r) {
        const int rc = run();
        if (rc) {
            h->ran = false; hb->n = 0; m->frame = 0; m->replayable = false; m->searched = false; m->pyramid = false; m->norm_min_inside = 0; m->pyr_norm_min_inside = 0;
            for (BankStream& k : m->bank) k.stale = true;
            return rc;
        }
    }
    SCHK(h, hipEventRecord(ev.b, h->stream));
    SCHK(h, hipEventSynchronize(ev.b));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ev.a, ev.b);
    *ms_out = ms / reps;
    return YH_OK;
}

}  // namespace

extern "C" {

int yh_scene_batch_append_memory(yh_scene_batch* hb, int32_t n_frames, const int32_t* streams, const int32_t* gather_q16, const int32_t* carry_q16,
                                 int32_t keep, int32_t ball_max_age) {
    if (!hb) return YH_EINVAL;
    const int rc = append_memory_checks(hb, n_frames, streams, gather_q16, carry_q16, keep, ball_max_age);
    return rc ? rc : append_memory_call(hb, n_frames, streams, gather_q16, carry_q16, keep, ball_max_age, 0, 0);
}

int yh_scene_batch_append_memory_search(yh_scene_batch* hb, int32_t n_frames, const int32_t* streams, int32_t n_rot, const int32_t* gather_q16,
                                        const int32_t* carry_q16, int32_t radius, int32_t keep, int32_t ball_max_age) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    int rc = append_memory_checks(hb, n_frames, streams, gather_q16, carry_q16, keep, ball_max_age);
    if (rc) return rc;
    // (the two ranges here: they are about the call, not about frame 0)
    if (n_rot < 1 || n_rot > SR_MAX_ROT) return h->fail(YH_EINVAL, "n_rot outside 1 .. 16");
    if (radius < 0 || radius > SR_MAX_R) return h->fail(YH_EINVAL, "radius outside 0 .. 8");
    for (int b = 0; b < n_frames; ++b)
        if ((rc = scene_register_bases_check(h, n_rot, gather_q16 + (size_t)b * n_rot * 6, carry_q16 + (size_t)b * n_rot * 6, radius))) return hb->framed(b, rc);
    return append_memory_call(hb, n_frames, streams, gather_q16, carry_q16, keep, ball_max_age, n_rot, radius);
}

int yh_scene_batch_append_memory_pyramid(yh_scene_batch* hb, int32_t n_frames, const int32_t* streams, int32_t n_rot, const int32_t* gather_q16,
                                         const int32_t* carry_q16, int32_t levels, int32_t radius, int32_t refine, int32_t keep, int32_t ball_max_age) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    int rc = append_memory_checks(hb, n_frames, streams, gather_q16, carry_q16, keep, ball_max_age);
    if (rc) return rc;
    // (the four ranges here: they are about the call, not about frame 0)
    if (n_rot < 1 || n_rot > SP_MAX_ROT) return h->fail(YH_EINVAL, "n_rot outside 1 .. 15");
    if (levels < 1 || levels > SP_MAX_LEVELS) return h->fail(YH_EINVAL, "levels outside 1 .. 3");
    if (radius < 0 || radius > SR_MAX_R) return h->fail(YH_EINVAL, "radius outside 0 .. 8");
    if (refine < 0 || refine > SR_MAX_R) return h->fail(YH_EINVAL, "refine outside 0 .. 8");
    std::vector<ScenePyramidPlan> plans((size_t)n_frames);
    for (int b = 0; b < n_frames; ++b)
        if ((rc = scene_pyramid_plan_make(h, n_rot, gather_q16 + (size_t)b * n_rot * 6, carry_q16 + (size_t)b * n_rot * 6, levels, radius, refine, plans[b]))) return hb->framed(b, rc);
    return append_memory_call(hb, n_frames, streams, gather_q16, carry_q16, keep, ball_max_age, n_rot, radius, &plans);
}

int yh_scene_batch_append_memory_search_norm(yh_scene_batch* hb, int32_t n_frames, const int32_t* streams, int32_t n_rot, const int32_t* gather_q16,
                                             const int32_t* carry_q16, int32_t radius, int32_t min_inside, int32_t keep, int32_t ball_max_age) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    int rc = append_memory_checks(hb, n_frames, streams, gather_q16, carry_q16, keep, ball_max_age);
    if (rc) return rc;
    if (n_rot < 1 || n_rot > SR_MAX_ROT) return h->fail(YH_EINVAL, "n_rot outside 1 .. 16");
    if (radius < 0 || radius > SR_MAX_R) return h->fail(YH_EINVAL, "radius outside 0 .. 8");
    if (min_inside < 1 || (long long)min_inside > (long long)h->W * h->H) return h->fail(YH_EINVAL, "min_inside outside 1 .. width x height");
    for (int b = 0; b < n_frames; ++b)
        if ((rc = scene_register_bases_check(h, n_rot, gather_q16 + (size_t)b * n_rot * 6, carry_q16 + (size_t)b * n_rot * 6, radius))) return hb->framed(b, rc);
    return append_memory_call(hb, n_frames, streams, gather_q16, carry_q16, keep, ball_max_age, n_rot, radius, nullptr, min_inside);
}

int yh_scene_batch_append_memory_pyramid_norm(yh_scene_batch* hb, int32_t n_frames, const int32_t* streams, int32_t n_rot, const int32_t* gather_q16,
                                              const int32_t* carry_q16, int32_t levels, int32_t radius, int32_t refine, int32_t min_inside, int32_t keep,
                                              int32_t ball_max_age) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    int rc = append_memory_checks(hb, n_frames, streams, gather_q16, carry_q16, keep, ball_max_age);
    if (rc) return rc;
    if (n_rot < 1 || n_rot > SP_MAX_ROT) return h->fail(YH_EINVAL, "n_rot outside 1 .. 15");
    if (levels < 1 || levels > SP_MAX_LEVELS) return h->fail(YH_EINVAL, "levels outside 1 .. 3");
    if (radius < 0 || radius > SR_MAX_R) return h->fail(YH_EINVAL, "radius outside 0 .. 8");
    if (refine < 0 || refine > SR_MAX_R) return h->fail(YH_EINVAL, "refine outside 0 .. 8");
    if (min_inside < 1 || (long long)min_inside > (long long)h->W * h->H) return h->fail(YH_EINVAL, "min_inside outside 1 .. width x height");
    std::vector<ScenePyramidPlan> plans((size_t)n_frames);
    for (int b = 0; b < n_frames; ++b)
        if ((rc = scene_pyramid_plan_make(h, n_rot, gather_q16 + (size_t)b * n_rot * 6, carry_q16 + (size_t)b * n_rot * 6, levels, radius, refine, plans[b]))) return hb->framed(b, rc);
    return append_memory_call(hb, n_frames, streams, gather_q16, carry_q16, keep, ball_max_age, n_rot, radius, &plans, min_inside);
}

int yh_scene_batch_motion_norm_read(yh_scene_batch* hb, int32_t frame, uint64_t* totals, uint64_t* inside, uint64_t* chosen_stc, uint64_t* prior_stc, int32_t* qualified) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    const bool pyr_norm = h->ran && scene_batch_memory_is_pyramid_norm(hb);
    if (!pyr_norm && (!h->ran || !scene_batch_memory_is_norm(hb))) return h->fail(YH_ESTATE, "the current frames did not come from yh_scene_batch_append_memory_search_norm");
    if (pyr_norm && (totals || inside))
        return h->fail(YH_EINVAL, "the current frames came from yh_scene_batch_append_memory_pyramid_norm: yh_scene_batch_pyramid_norm_read returns their level tables");
    if (frame < 0 || frame >= hb->n) return h->fail(YH_EINVAL, "frame " + std::to_string(frame) + " outside the last append's " + std::to_string(hb->n));
    SCHK(h, hipSetDevice(h->dev));
    yh_scene_batch_memory* m = hb->memory;
    SceneRegisterNormRecord ext;
    const size_t words = register_norm_table_words(m->n_rot, m->radius);
    const unsigned long long* acc = pyr_norm ? nullptr : m->norm_acc + (size_t)frame * m->acc_stride();
    SCHK(h, hipMemcpyAsync(&ext, m->norm_rec + frame, sizeof(ext), hipMemcpyDeviceToHost, h->stream));
    if (totals) SCHK(h, hipMemcpyAsync(totals, acc + 1 + words, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    if (inside) SCHK(h, hipMemcpyAsync(inside, acc + 1 + 2 * words, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 3; ++i) { if (chosen_stc) chosen_stc[i] = ext.chosen[i]; if (prior_stc) prior_stc[i] = ext.prior[i]; }
    if (qualified) *qualified = ext.qualified;
    return YH_OK;
}

int yh_scene_batch_pyramid_norm_read(yh_scene_batch* hb, int32_t frame, int32_t level, int32_t* centres, uint64_t* scores, uint64_t* totals, uint64_t* inside,
                                     uint64_t* sum_n, int32_t* level_min_inside, int32_t* qualified) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    // (replayable: no memory has been reset since, as yh_scene_batch_pyramid_read asks)
    if (!h->ran || !scene_batch_memory_is_pyramid_norm(hb) || !hb->memory->replayable)
        return h->fail(YH_ESTATE, "the last memory append of the batch was not yh_scene_batch_append_memory_pyramid_norm (or a memory was reset since)");
    if (frame < 0 || frame >= hb->n) return h->fail(YH_EINVAL, "frame " + std::to_string(frame) + " outside the last append's " + std::to_string(hb->n));
    yh_scene_batch_memory* m = hb->memory;
    const ScenePyramidPlan& plan = m->pyr;
    if (level < 0 || level > plan.levels) return h->fail(YH_EINVAL, "level outside 0 .. " + std::to_string(plan.levels));
    SCHK(h, hipSetDevice(h->dev));
    const int hyp = plan.hyp(level);
    const size_t words = register_norm_table_words(hyp, plan.rho(level));
    const unsigned long long* acc = m->pyrn_acc + (size_t)frame * pyramid_norm_acc_offset(plan, plan.levels + 1) + pyramid_norm_acc_offset(plan, level);
    int cen[SR_MAX_ROT][2], flags[SR_MAX_ROT];
    unsigned long long sum = 0;
    if (centres) SCHK(h, hipMemcpyAsync(cen, m->pyr_table[frame].centre[level], sizeof(cen), hipMemcpyDeviceToHost, h->stream));
    if (qualified) SCHK(h, hipMemcpyAsync(flags, m->pyrn_ext[frame].qualified[level], sizeof(flags), hipMemcpyDeviceToHost, h->stream));
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

int yh_scene_batch_pyramid_read(yh_scene_batch* hb, int32_t frame, int32_t level, int32_t* centres, uint64_t* scores, uint64_t* sum_n) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    // (replayable: no memory has been reset since, as yh_scene_pyramid_read asks of the single handle)
    const bool norm = scene_batch_memory_is_pyramid_norm(hb);
    if (!h->ran || !(scene_batch_memory_is_pyramid(hb) || norm) || !hb->memory->replayable)
        return h->fail(YH_ESTATE, "the last memory append of the batch was not yh_scene_batch_append_memory_pyramid (or a memory was reset since)");
    if (frame < 0 || frame >= hb->n) return h->fail(YH_EINVAL, "frame " + std::to_string(frame) + " outside the last append's " + std::to_string(hb->n));
    yh_scene_batch_memory* m = hb->memory;
    const ScenePyramidPlan& plan = m->pyr;
    if (level < 0 || level > plan.levels) return h->fail(YH_EINVAL, "level outside 0 .. " + std::to_string(plan.levels));
    SCHK(h, hipSetDevice(h->dev));
    const int hyp = plan.hyp(level), nu = 2 * plan.rho(level) + 1;
    // (after a normalised pyramid append: its S tables, which lie first in each level of its own tables)
    const unsigned long long* acc = norm ? m->pyrn_acc + (size_t)frame * pyramid_norm_acc_offset(plan, plan.levels + 1) + pyramid_norm_acc_offset(plan, level)
                                         : m->pyr_acc + (size_t)frame * plan.acc_offset(plan.levels + 1) + plan.acc_offset(level);
    int cen[SR_MAX_ROT][2];
    unsigned long long sum = 0;
    if (centres) SCHK(h, hipMemcpyAsync(cen, m->pyr_table[frame].centre[level], sizeof(cen), hipMemcpyDeviceToHost, h->stream));
    if (sum_n) SCHK(h, hipMemcpyAsync(&sum, acc, sizeof(sum), hipMemcpyDeviceToHost, h->stream));
    if (scores) SCHK(h, hipMemcpyAsync(scores, acc + 1, (size_t)hyp * nu * nu * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < hyp && centres; ++k) { centres[2 * k] = cen[k][0]; centres[2 * k + 1] = cen[k][1]; }
    if (sum_n) *sum_n = sum;
    return YH_OK;
}

int yh_scene_batch_motion_read(yh_scene_batch* hb, int32_t frame, int32_t* gather_q16, int32_t* carry_q16, int32_t* chosen, uint64_t* score, uint64_t* scores) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    const bool pyr_norm = h->ran && scene_batch_memory_is_pyramid_norm(hb);
    const bool pyramid = pyr_norm || (h->ran && scene_batch_memory_is_pyramid(hb));
    if (!pyramid && (!h->ran || !scene_batch_memory_is_search(hb))) return h->fail(YH_ESTATE, "the current frames did not come from yh_scene_batch_append_memory_search");
    if (pyr_norm && scores)
        return h->fail(YH_EINVAL, "the current frames came from yh_scene_batch_append_memory_pyramid_norm: yh_scene_batch_pyramid_read returns their level tables");
    if (pyramid && scores) return h->fail(YH_EINVAL, "the current frames came from yh_scene_batch_append_memory_pyramid: yh_scene_batch_pyramid_read returns their level tables");
    if (frame < 0 || frame >= hb->n) return h->fail(YH_EINVAL, "frame " + std::to_string(frame) + " outside the last append's " + std::to_string(hb->n));
    SCHK(h, hipSetDevice(h->dev));
    yh_scene_batch_memory* m = hb->memory;
    SceneRegisterRecord rec;
    const size_t stride = m->acc_stride();
    SCHK(h, hipMemcpyAsync(&rec, m->reg_rec + frame, sizeof(rec), hipMemcpyDeviceToHost, h->stream));
    // (after a normalised search: its S table, which lies first in the frame's tables)
    const unsigned long long* acc = m->norm_min_inside ? m->norm_acc : m->reg_acc;
    if (scores) SCHK(h, hipMemcpyAsync(scores, acc + (size_t)frame * stride + 1, register_norm_table_words(m->n_rot, m->radius) * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 6; ++i) { if (gather_q16) gather_q16[i] = rec.g[i]; if (carry_q16) carry_q16[i] = rec.c[i]; }
    for (int i = 0; i < 3; ++i) { if (chosen) chosen[i] = rec.chosen[i]; if (score) score[i] = rec.score[i]; }
    return YH_OK;
}

int yh_scene_batch_memory_read(yh_scene_batch* hb, int32_t stream, uint32_t* map_mem, int32_t* balls_mem) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    int rc = stream_ok(hb, stream, 0);
    if (rc) return rc;
    SCHK(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)h->W * h->H;
    yh_scene_batch_memory* m = hb->memory;
    if (!m || !m->bank[stream].map[0]) {   // never used: empty
        if (map_mem) memset(map_mem, 0, npx * 4);
        if (balls_mem) memset(balls_mem, 0, 100 * 4 * sizeof(int32_t));
        SCHK(h, hipStreamSynchronize(h->stream));
        return YH_OK;
    }
    if ((rc = stream_reserve(hb, stream))) return rc;   // (a stale stream is cleared first)
    const BankStream& k = m->bank[stream];
    if (map_mem) SCHK(h, hipMemcpyAsync(map_mem, k.map[k.cur], npx * 4, hipMemcpyDeviceToHost, h->stream));
    if (balls_mem) SCHK(h, hipMemcpyAsync(balls_mem, k.tab[k.cur], 100 * sizeof(int4), hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    return YH_OK;
}

int yh_scene_batch_memory_frame_balls(yh_scene_batch* hb, int32_t frame, int32_t* balls_mem) {
    if (!hb || !balls_mem) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (!h->ran || !scene_batch_memory_is_last(hb)) return h->fail(YH_ESTATE, "the current frames did not come from yh_scene_batch_append_memory");
    if (frame < 0 || frame >= hb->n) return h->fail(YH_EINVAL, "frame " + std::to_string(frame) + " outside the last append's " + std::to_string(hb->n));
    SCHK(h, hipSetDevice(h->dev));
    SCHK(h, hipMemcpyAsync(balls_mem, hb->memory->tabs + (size_t)frame * 100, 100 * sizeof(int4), hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    return YH_OK;
}

int yh_scene_batch_memory_reset(yh_scene_batch* hb, int32_t stream) {
    if (!hb) return YH_EINVAL;
    yh_scene* h = &hb->core;
    int rc = stream_ok(hb, stream, -1);
    if (rc) return rc;
    yh_scene_batch_memory* m = hb->memory;
    if (!m) return YH_OK;
    SCHK(h, hipSetDevice(h->dev));
    m->replayable = false;   // (the state the last memory append started from may be gone)
    for (int s = stream < 0 ? 0 : stream; s < (stream < 0 ? YH_SCENE_STREAMS_MAX : stream + 1); ++s) {
        if (!m->bank[s].map[0]) continue;
        m->bank[s].stale = true;   // (should the clearing fail, it is made again before the next use)
        if ((rc = stream_reserve(hb, s))) return rc;
    }
    return YH_OK;
}

int yh_scene_batch_memory_time(yh_scene_batch* hb, int32_t reps, float* ms_per_batch) {
    if (!hb || reps < 1 || !ms_per_batch) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (h->ran && scene_batch_memory_is_pyramid_norm(hb))
        return h->fail(YH_ESTATE, "the last frames came from yh_scene_batch_append_memory_pyramid_norm: yh_scene_batch_memory_pyramid_norm_time replays them");
    if (h->ran && scene_batch_memory_is_norm(hb))
        return h->fail(YH_ESTATE, "the last frames came from yh_scene_batch_append_memory_search_norm: yh_scene_batch_memory_search_norm_time replays them");
    if (h->ran && scene_batch_memory_is_pyramid(hb))
        return h->fail(YH_ESTATE, "the last frames came from yh_scene_batch_append_memory_pyramid: yh_scene_batch_memory_pyramid_time replays them");
    if (h->ran && scene_batch_memory_is_search(hb))
        return h->fail(YH_ESTATE, "the last frames came from yh_scene_batch_append_memory_search: yh_scene_batch_memory_search_time replays them");
    if (!h->ran || !scene_batch_memory_is_last(hb) || !hb->memory->replayable || hb->memory->stagings != hb->stagings)
        return h->fail(YH_ESTATE, "the last frames did not come from yh_scene_batch_append_memory (or a memory was reset or a slot staged since)");
    SCHK(h, hipSetDevice(h->dev));
    // the last append's own slots, motions and streams (its device tables), from the state it started from - the other buffers of
    // every stream it named - into the state it left: the same bits again, so nothing is committed
    return replay_time(hb, reps, [hb] { return run_memory(hb); }, ms_per_batch);
}

int yh_scene_batch_memory_search_time(yh_scene_batch* hb, int32_t reps, float* ms_per_batch, float* ms_search) {
    if (!hb || reps < 1 || !ms_per_batch || !ms_search) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (h->ran && scene_batch_memory_is_pyramid_norm(hb))
        return h->fail(YH_ESTATE, "the last frames came from yh_scene_batch_append_memory_pyramid_norm: yh_scene_batch_memory_pyramid_norm_time replays them");
    if (h->ran && scene_batch_memory_is_norm(hb))
        return h->fail(YH_ESTATE, "the last frames came from yh_scene_batch_append_memory_search_norm: yh_scene_batch_memory_search_norm_time replays them");
    if (h->ran && scene_batch_memory_is_pyramid(hb))
        return h->fail(YH_ESTATE, "the last frames came from yh_scene_batch_append_memory_pyramid: yh_scene_batch_memory_pyramid_time replays them");
    if (!h->ran || !scene_batch_memory_is_search(hb) || !hb->memory->replayable || hb->memory->stagings != hb->stagings)
        return h->fail(YH_ESTATE, "the last frames did not come from yh_scene_batch_append_memory_search (or a memory was reset or a slot staged since)");
    SCHK(h, hipSetDevice(h->dev));
    // the whole append first, as yh_scene_batch_memory_time replays a plain one; then its registration launches alone, on the map
    // slots that left - each predecessor's fused map - so the same tables and records again
    const int rc = replay_time(hb, reps, [hb] { return run_memory(hb); }, ms_per_batch);
    return rc ? rc : replay_time(hb, reps, [hb] { return scene_batch_register_search(hb, nullptr); }, ms_search);
}

int yh_scene_batch_memory_pyramid_time(yh_scene_batch* hb, int32_t reps, float* ms_per_batch, float* ms_search) {
    if (!hb || reps < 1 || !ms_per_batch || !ms_search) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (h->ran && scene_batch_memory_is_pyramid_norm(hb))
        return h->fail(YH_ESTATE, "the last frames came from yh_scene_batch_append_memory_pyramid_norm: yh_scene_batch_memory_pyramid_norm_time replays them");
    if (h->ran && scene_batch_memory_is_norm(hb))
        return h->fail(YH_ESTATE, "the last frames came from yh_scene_batch_append_memory_search_norm: yh_scene_batch_memory_search_norm_time replays them");
    if (!h->ran || !scene_batch_memory_is_pyramid(hb) || !hb->memory->replayable || hb->memory->stagings != hb->stagings)
        return h->fail(YH_ESTATE, "the last frames did not come from yh_scene_batch_append_memory_pyramid (or a memory was reset or a slot staged since)");
    SCHK(h, hipSetDevice(h->dev));
    // as yh_scene_batch_memory_search_time: the whole append from the tables on the device (select rewrites the same centres into
    // them), then the clear and every round's levels, scores and choices alone, on each predecessor's fused map
    const int rc = replay_time(hb, reps, [hb] { return run_memory(hb); }, ms_per_batch);
    return rc ? rc : replay_time(hb, reps, [hb] { return scene_batch_pyramid_search(hb, nullptr); }, ms_search);
}

int yh_scene_batch_memory_search_norm_time(yh_scene_batch* hb, int32_t reps, float* ms_per_batch, float* ms_search) {
    if (!hb || reps < 1 || !ms_per_batch || !ms_search) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (!h->ran || !scene_batch_memory_is_norm(hb) || !hb->memory->replayable || hb->memory->stagings != hb->stagings)
        return h->fail(YH_ESTATE, "the last frames did not come from yh_scene_batch_append_memory_search_norm (or a memory was reset or a slot staged since)");
    SCHK(h, hipSetDevice(h->dev));
    // as yh_scene_batch_memory_search_time: the whole append, then its registration launches alone on the map slots that left
    const int rc = replay_time(hb, reps, [hb] { return run_memory(hb); }, ms_per_batch);
    return rc ? rc : replay_time(hb, reps, [hb] { return scene_batch_register_norm_search(hb, nullptr); }, ms_search);
}

int yh_scene_batch_memory_pyramid_norm_time(yh_scene_batch* hb, int32_t reps, float* ms_per_batch, float* ms_search) {
    if (!hb || reps < 1 || !ms_per_batch || !ms_search) return YH_EINVAL;
    yh_scene* h = &hb->core;
    if (!h->ran || !scene_batch_memory_is_pyramid_norm(hb) || !hb->memory->replayable || hb->memory->stagings != hb->stagings)
        return h->fail(YH_ESTATE, "the last frames did not come from yh_scene_batch_append_memory_pyramid_norm (or a memory was reset or a slot staged since)");
    SCHK(h, hipSetDevice(h->dev));
    // as yh_scene_batch_memory_pyramid_time: the whole append from the tables on the device, then the clear and every round's
    // levels, tables and choices alone, on each predecessor's fused map
    const int rc = replay_time(hb, reps, [hb] { return run_memory(hb); }, ms_per_batch);
    return rc ? rc : replay_time(hb, reps, [hb] { return scene_batch_pyramid_norm_search(hb, nullptr); }, ms_search);
}

}  // extern "C"
