// scene_solve.hip — the field solver behind every planner (scene_path.hip: one field per frame, n targets; scene_tour.hip: K fields,
// one target each; scene_turn.hip and scene_turn_tour.hip with their own round kernel): the edge terms, the rounds of tile relaxation
// to the fixed point of DESIGN.md §11 "Path planner", and what the kinds' time and read entry points and their frame-major states
// have in common. Its state hangs off the scene handle (yh_scene::solve, scene_path_dev.h): one set of buffers for all kinds and
// both connectivities, the edge terms those of the handle's max_frames frames.
//   path_weights   one lane per pixel, the frame from blockIdx.z: conn0 / conn1 / map -> one float4 per pixel (right length, right
//                  height step, down length, down height step; <8>: a second one for down-right and down-left): the solver reads
//                  16 B per pixel instead of 32 B of connections + the map, length and step stay apart for the two roundings.
//   field_round    (the plain tour's; the plans' round kernels are their units') x rounds, grid (tiles x, tiles y, F = n Kmax): relax_tile
//                  (scene_path_dev.h) on field z with field z's flags and the edge terms of frame z / Kmax: a flagged
//                  tile relaxes in LDS to its local fixed point for the halo it loaded, and cells that changed go back with atomicMin
//                  on the u32 view (non-negative f32 order as their bits). Only a tile whose halo may have changed runs: a tile that
//                  lowered a cell of its border flags that neighbour for the NEXT round (two flag arrays, by round parity) and
//                  counts it once; the counters sum over the fields. No workgroup ever waits for another one: a round is a launch,
//                  the host enqueues SP_BATCH of them and reads the batch's counters back once (rounds past convergence, and the
//                  tiles of a converged field, find no flag and exit at once). F fields take the rounds of the slowest, not their sum.
// Round 0's flags come from the host (round0_flags): a seed's drop from +inf to 0 is a lowered cell like any other, and a neighbour
// whose border sees nothing but seeds (a wall of targets along a tile border) would otherwise never be flagged.
#include <hip/hip_runtime.h>

#include <string>

#include "scene.h"
#include "scene_path_dev.h"
#include "yh_internal.h"

using namespace yh;

namespace {

template <int CONN>
__global__ __launch_bounds__(256) void path_weights(const PathParams p) { weights_body<CONN>(frame_of(p, blockIdx.z, 0)); }

// field z = blockIdx.z of F = n kmax: field z % kmax of frame z / kmax, with that frame's edge terms and its own cost field and flags
template <int CONN>
__global__ __launch_bounds__(SP_NT) void field_round(const PathParams p, int kmax, int F, int parity, uint32_t* cnt_next) {
    const int z = blockIdx.z;
    relax_tile<CONN>(frame_of(p, z / kmax, 0), p.cost + (size_t)z * p.W * p.H, p.flags + (size_t)(parity * F + z) * p.ntiles, p.flags + (size_t)((parity ^ 1) * F + z) * p.ntiles, cnt_next);
}

int last_ok(yh_scene* h, const char* kind, const char* again, const SolveLast* q) {
    if (!q || !q->planned) return h->fail(YH_ESTATE, std::string("no ") + kind + " has been made");
    if (q->frame != h->frames) return h->fail(YH_ESTATE, std::string("a newer frame has been appended since the ") + kind + ": " + again);
    return YH_OK;
}

}  // namespace

namespace yh {

int solve_begin(yh_scene* h, int conn, int F, int n, PathParams& p) {
    if (!h->solve) h->solve = new yh_scene_solve();
    yh_scene_solve* s = h->solve;
    const size_t npx = (size_t)h->W * h->H, frames = (size_t)h->max_frames;
    s->tx = (h->W + SP_TW - 1) / SP_TW; s->ty = (h->H + SP_TH - 1) / SP_TH;
    if (!s->edge) SCHK(h, hipMalloc((void**)&s->edge, frames * npx * 16));
    if (conn == 8 && !s->edge2) SCHK(h, hipMalloc((void**)&s->edge2, frames * npx * 16));
    if (!s->cnt) SCHK(h, hipMalloc((void**)&s->cnt, (kSolveCnt + frames * kSolveTail) * 4));
    if (!s->host) SCHK(h, hipHostMalloc((void**)&s->host, (kSolveCnt + frames * kSolveTail) * 4, hipHostMallocDefault));
    if (F > s->cap_f) {
        if (s->flags) { SCHK(h, hipStreamSynchronize(h->stream)); SCHK(h, hipFree(s->flags)); s->flags = nullptr; s->cap_f = 0; }
        SCHK(h, hipMalloc((void**)&s->flags, (size_t)2 * F * s->tx * s->ty * 4));
        s->cap_f = F;
    }
    p.W = h->W; p.H = h->H; p.tx = s->tx; p.ntiles = s->tx * s->ty;
    p.map = h->map; p.conn0 = h->conn0; p.conn1 = h->conn1; p.edge = s->edge; p.edge2 = conn == 8 ? s->edge2 : nullptr; p.flags = s->flags;
    p.cost = nullptr; p.next = nullptr;
    hipLaunchKernelGGL(conn == 8 ? path_weights<8> : path_weights<4>, dim3((unsigned)((npx + 255) / 256), 1, (unsigned)n), dim3(256), 0, h->stream, p);
    return YH_OK;
}

SolveRound solve_field_round(yh_scene* h, const PathParams& p, int conn, int kmax, int F) {
    return SolveRound{ [=](const dim3& tiles, int parity, uint32_t* cnt_next) {
        hipLaunchKernelGGL(conn == 8 ? field_round<8> : field_round<4>, tiles, dim3(SP_NT), 0, h->stream, p, kmax, F, parity, cnt_next);
    }, 1 };
}

int plan_inputs_reserve(yh_scene* h, PlanInputs& in, size_t words) {
    if (words <= in.cap) return YH_OK;
    if (in.cap) SCHK(h, hipStreamSynchronize(h->stream));
    plan_inputs_free(in);
    SCHK(h, hipHostMalloc((void**)&in.host, words * 4, hipHostMallocDefault));
    SCHK(h, hipMalloc((void**)&in.dev, words * 4));
    in.cap = words;
    return YH_OK;
}

void plan_inputs_free(PlanInputs& in) {
    if (in.host) (void)hipHostFree(in.host);
    if (in.dev) (void)hipFree(in.dev);
    in = PlanInputs();
}

size_t plan_inputs_seeds(PlanFrames& q) {
    for (size_t k = 0; k < q.last_seeds.size(); ++k) { q.in.host[2 * k] = q.last_seeds[k]; q.in.host[2 * k + 1] = q.last_field[k]; }
    return 2 * q.last_seeds.size();
}

int solve_frame(yh_scene* h, const PlanFrames* q, int frame, size_t route_stride, const char* what, SolveLast& one) {
    one = q ? q->last : SolveLast();
    if (!one.planned || one.frame != h->frames) return YH_OK;   // (solve_read says which)
    if (q->status[frame] != YH_OK) return h->fail(YH_ESTATE, "frame " + std::to_string(frame) + " had no ball inside it: it has no " + what);
    one.path_len = q->path_len[frame]; one.nodes = q->nodes + frame * route_stride; one.dirs = q->dirs + frame * route_stride;
    return YH_OK;
}

int solve_rounds(yh_scene* h, const PathParams& p, int conn, int F, const std::vector<int32_t>& seeds, const char* who, int tail_words,
                 const std::function<void(uint32_t*)>& after, const SolveRound* own, const std::vector<int32_t>* field_of) {
    yh_scene_solve* s = h->solve;
    // round 0's work list: parity 0 of [2][F][ntiles]; parity 1 goes up in the same copy, all zero
    const size_t per = seeds.size() / F, nflags = (size_t)F * p.ntiles;
    if (field_of ? F < 1 || field_of->size() != seeds.size() : F < 1 || per < 1 || per * F != seeds.size()) return h->fail(YH_EINVAL, std::string(who) + " solver: the seeds are not equally many per field");
    s->flags0.assign(2 * nflags, 0u);
    long long active = 0;
    for (size_t k = 0; k < seeds.size(); ++k) {
        uint32_t* f0 = s->flags0.data() + (field_of ? (size_t)(*field_of)[k] : k / per) * p.ntiles;
        round0_flags(seeds[k] % h->W, seeds[k] / h->W, conn, [&](int bx, int by) {
            if (bx < 0 || bx >= s->tx || by < 0 || by >= s->ty) return;
            uint32_t& f = f0[(size_t)by * s->tx + bx];
            if (!f) { f = 1u; ++active; }
        });
    }
    SCHK(h, hipMemcpyAsync(s->flags, s->flags0.data(), 2 * nflags * 4, hipMemcpyHostToDevice, h->stream));
    s->rounds = 0; s->tile_runs = 0;
    const SolveRound round_kernel = own ? *own : solve_field_round(h, p, conn, F, F);   // (no kernel given: F fields of one frame)
    const long long cap = (long long)h->W * h->H * round_kernel.states;   // costs only decrease over a finite set: this never fires
    const dim3 tiles((unsigned)s->tx, (unsigned)s->ty, (unsigned)F);
    long long round = 0;
    while (active) {
        if (round >= cap) return h->fail(YH_EHIP, std::string(who) + " solver: round cap " + (round_kernel.states > 1 ? std::to_string(round_kernel.states) + "*" : "") + "W*H reached without convergence (fields not those of a SANE frame?)");
        SCHK(h, hipMemsetAsync(s->cnt, 0, kSolveCnt * 4, h->stream));
        for (int j = 0; j < SP_BATCH; ++j, ++round)
            round_kernel.launch(tiles, (int)(round & 1), s->cnt + j + 1);
        if (after) after(s->cnt + kSolveCnt);
        SCHK(h, hipGetLastError());
        SCHK(h, hipMemcpyAsync(s->host, s->cnt, (size_t)(kSolveCnt + tail_words) * 4, hipMemcpyDeviceToHost, h->stream));
        SCHK(h, hipStreamSynchronize(h->stream));
        s->host[0] = (uint32_t)active;   // tiles (of all fields) that ran in round j of the batch: host[j]
        for (int j = 0; j < SP_BATCH; ++j) if (s->host[j]) { ++s->rounds; s->tile_runs += s->host[j]; }
        active = s->host[SP_BATCH];
    }
    return YH_OK;
}

int solve_time(yh_scene* h, const char* kind, const char* again, const SolveLast* q, int reps, const std::function<int()>& run, float* ms, int32_t* rounds, int32_t* tile_runs) {
    int rc = last_ok(h, kind, again, q);
    if (rc) return rc;
    SCHK(h, hipSetDevice(h->dev));
    struct Events { hipEvent_t a = nullptr, b = nullptr; ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev;   // (on every return)
    SCHK(h, hipEventCreate(&ev.a)); SCHK(h, hipEventCreate(&ev.b));
    SCHK(h, hipEventRecord(ev.a, h->stream));
    for (int r = 0; r < reps; ++r) if ((rc = run())) return rc;
    SCHK(h, hipEventRecord(ev.b, h->stream));
    SCHK(h, hipEventSynchronize(ev.b));
    float total = 0;
    (void)hipEventElapsedTime(&total, ev.a, ev.b);
    *ms = total / reps;   // (the host's waits for the batches' counters, and what else run() does on the host, are inside)
    if (rounds) *rounds = (int32_t)h->solve->rounds;
    if (tile_runs) *tile_runs = (int32_t)h->solve->tile_runs;
    return YH_OK;
}

int solve_read(yh_scene* h, const char* kind, const char* again, const SolveLast* q, std::initializer_list<SolveCopy> fields, int32_t* path_xy, float* directions,
               int32_t path_capacity, int32_t* path_len, bool per_node) {
    const int rc = last_ok(h, kind, again, q);
    if (rc) return rc;
    if (path_len) *path_len = q->path_len;
    if ((path_xy || directions || per_node) && path_capacity < q->path_len)
        return h->fail(YH_EOVERFLOW, "path_capacity " + std::to_string(path_capacity) + " < the route's " + std::to_string(q->path_len) + " nodes");
    SCHK(h, hipSetDevice(h->dev));
    for (const SolveCopy& c : fields) if (c.dst) SCHK(h, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, h->stream));
    if (path_xy) SCHK(h, hipMemcpyAsync(path_xy, q->nodes, (size_t)q->path_len * sizeof(int2), hipMemcpyDeviceToHost, h->stream));
    if (directions && q->path_len > 1) SCHK(h, hipMemcpyAsync(directions, q->dirs, (size_t)(q->path_len - 1) * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    return YH_OK;
}

void scene_solve_free(yh_scene* h) {
    yh_scene_solve* s = h->solve;
    if (!s) return;
    void* bufs[] = { s->edge, s->edge2, s->flags, s->cnt };
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (s->host) (void)hipHostFree(s->host);
    delete s;
    h->solve = nullptr;
}

}  // namespace yh
