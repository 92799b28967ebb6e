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
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "scene.h"
#include "scene_batch.h"
#include "scene_dev.h"
#include "scene_memory_dev.h"
#include "yh_internal.h"

using namespace yh;

namespace {

struct BankStream {
    uint32_t* map[2] = { nullptr, nullptr };   // M [H][W]: map[cur] is the memory, map[cur ^ 1] what it was before the last call that named the stream
    int4* tab[2] = { nullptr, nullptr };       // B [100], likewise
    int cur = 0;
    bool stale = true;                         // cleared before the next use: fresh buffers, a reset, or a call that failed half-way
};

}  // namespace

struct yh_scene_batch_memory {
    uint32_t* stamp = nullptr;    // N [max_frames][H][W]
    int4* tabs = nullptr;         // [max_frames][100]: every frame's table right after it
    unsigned char* table = nullptr;   // device: SceneFuseSlot [max_frames], SceneBallsStep [max_frames], SceneBallsChain [YH_SCENE_STREAMS_MAX]
    std::vector<unsigned char> table_host;
    BankStream bank[YH_SCENE_STREAMS_MAX];
    // the last memory append, for yh_scene_batch_memory_time: the handle's frames are that append's while core.frames == frame
    // (every append and yh_scene_batch_set_fields counts core.frames up); a reset or a staged slot since leaves nothing to replay
    uint64_t frame = 0, stagings = 0;
    bool replayable = false;
    int n = 0, keep = 0, max_age = 0, chains = 0;
    std::vector<int> round_off;   // slots of round r: round_off[r] .. round_off[r + 1]
};

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

size_t slots_bytes(const yh_scene* h) { return (size_t)h->max_frames * sizeof(SceneFuseSlot); }
size_t steps_bytes(const yh_scene* h) { return (size_t)h->max_frames * sizeof(SceneBallsStep); }

// the buffers every memory append uses, at the first one: a batch that never remembers pays nothing
int memory_reserve(yh_scene_batch* hb) {
    yh_scene* h = &hb->core;
    if (!hb->memory) hb->memory = new yh_scene_batch_memory();
    yh_scene_batch_memory* m = hb->memory;
    const size_t all = (size_t)h->max_frames * h->W * h->H;
    if (!m->stamp) SCHK(h, hipMalloc((void**)&m->stamp, all * 4));
    if (!m->tabs) SCHK(h, hipMalloc((void**)&m->tabs, (size_t)h->max_frames * 100 * sizeof(int4)));
    if (!m->table) SCHK(h, hipMalloc((void**)&m->table, slots_bytes(h) + steps_bytes(h) + YH_SCENE_STREAMS_MAX * sizeof(SceneBallsChain)));
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
    hipLaunchKernelGGL(batch_balls_memory, dim3((unsigned)m->chains), dim3(128), 0, h->stream, b, chains, steps, m->tabs);
    const unsigned gx = (unsigned)((h->W + SF_TW - 1) / SF_TW), gy = (unsigned)((h->H + SF_TH - 1) / SF_TH);
    for (size_t r = 0; r + 1 < m->round_off.size(); ++r)
        hipLaunchKernelGGL(batch_fuse, dim3(gx, gy, (unsigned)(m->round_off[r + 1] - m->round_off[r])), dim3(256), 0, h->stream, f, slots + m->round_off[r]);
    SCHK(h, hipGetLastError());
    return YH_OK;
}

int stream_of(const int32_t* streams, int b) { return streams ? streams[b] : 0; }

int append_memory(yh_scene_batch* hb, int n, const int32_t* streams, const int32_t* gather, const int32_t* carry, int keep, int max_age) {
    yh_scene* h = &hb->core;
    SCHK(h, hipSetDevice(h->dev));
    int rc = memory_reserve(hb);
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
    m->table_host.assign(slots_bytes(h) + steps_bytes(h) + YH_SCENE_STREAMS_MAX * sizeof(SceneBallsChain), 0);
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
            for (int i = 0; i < 6; ++i) e.g[i] = gather[6 * f[r] + i];
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
            for (int i = 0; i < 6; ++i) e.c[i] = carry[6 * b + i];
        }
    }
    m->n = n; m->keep = keep; m->max_age = max_age;
    // (from pageable memory: staged by the runtime before the call returns, as the caller's own arrays have been read by now)
    SCHK(h, hipMemcpyAsync(m->table, m->table_host.data(), m->table_host.size(), hipMemcpyHostToDevice, h->stream));
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
    void* bufs[] = { m->stamp, m->tabs, m->table };
    for (void* b : bufs) if (b) hipFree(b);
    delete m;
    hb->memory = nullptr;
}

bool scene_batch_memory_is_last(const yh_scene_batch* hb) { return hb->memory && hb->memory->frame != 0 && hb->memory->frame == hb->core.frames; }
}  // namespace yh

extern "C" {

int yh_scene_batch_append_memory(yh_scene_batch* hb, int32_t n_frames, const int32_t* streams, const int32_t* gather_q16, const int32_t* carry_q16,
                                 int32_t keep, int32_t ball_max_age) {
    if (!hb) return YH_EINVAL;
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
    ++h->frames;   // (earlier plans are of other frames, whatever becomes of these)
    const int rc = append_memory(hb, n_frames, streams, gather_q16, carry_q16, keep, ball_max_age);
    yh_scene_batch_memory* m = hb->memory;
    if (rc) {
        // a call that fails after its checks leaves no frame and empties the memories of the streams it named
        h->ran = false; hb->n = 0;
        if (m) {
            m->frame = 0; m->replayable = false;
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
    if (!h->ran || !scene_batch_memory_is_last(hb) || !hb->memory->replayable || hb->memory->stagings != hb->stagings)
        return h->fail(YH_ESTATE, "the last frames did not come from yh_scene_batch_append_memory (or a memory was reset or a slot staged since)");
    SCHK(h, hipSetDevice(h->dev));
    struct Events { hipEvent_t a = nullptr, b = nullptr; ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev;
    SCHK(h, hipEventCreate(&ev.a)); SCHK(h, hipEventCreate(&ev.b));
    SCHK(h, hipEventRecord(ev.a, h->stream));
    // the last append's own slots, motions and streams (its device tables), from the state it started from - the other buffers of
    // every stream it named - into the state it left: the same bits again, so nothing is committed
    yh_scene_batch_memory* m = hb->memory;
    for (int r = 0; r < reps; ++r) {
        const int rc = run_memory(hb);
        if (rc) {
            h->ran = false; hb->n = 0; m->frame = 0; m->replayable = false;
            for (BankStream& k : m->bank) k.stale = true;
            return rc;
        }
    }
    SCHK(h, hipEventRecord(ev.b, h->stream));
    SCHK(h, hipEventSynchronize(ev.b));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ev.a, ev.b);
    *ms_per_batch = ms / reps;
    return YH_OK;
}

}  // extern "C"
