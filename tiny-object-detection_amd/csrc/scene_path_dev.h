// scene_path_dev.h — what scene_path.hip (one multi-source field per frame, yh_scene_plan and yh_scene_batch_plan) and scene_tour.hip
// (K single-target fields, yh_scene_plan_tour) share: the field solver of scene_solve.hip, declared here, what the frame-major planner
// states have in common, and the planner's device code - the tile relaxation, the successor rule and the windowed chase. scene_turn.hip
// and scene_turn_tour.hip (the turn-aware plan and tour) run their own round kernel through the same host loop (SolveRound) and take
// their edge terms through around<8>. What they compute and why it is unique is said at the head of scene_path.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <initializer_list>
#include <vector>

#ifndef SP_TW
#define SP_TW 32   // tile width and height (even). Measured alternatives: DESIGN.md §11
#endif
#ifndef SP_TH
#define SP_TH 32
#endif
#ifndef SP_INNER
#define SP_INNER 4   // sweeps between two workgroup votes
#endif
#ifndef SP_BATCH
#define SP_BATCH 16   // rounds enqueued per host read of the counters
#endif
#define SP_NT ((SP_TW / 2) * (SP_TH / 2))
#define SP_P (SP_TW + 2)
#define SP_WS 32   // the chase's window
#define SP_INF __uint_as_float(0x7f800000u)

static_assert(SP_TW % 2 == 0 && SP_TH % 2 == 0 && SP_NT % 64 == 0 && SP_NT <= 1024, "tile: whole waves of 2 x 2 blocks");

struct yh_scene;
// ---- host side (this struct and the solve_* declarations below). The solver's state (yh_scene::solve, scene_solve.hip): allocated at
// the first plan or tour of a handle, shared by both kinds and both connectivities - every run recomputes the edge terms.
struct yh_scene_solve {
    float4* edge = nullptr;      // [max_frames][H][W]: right length, right |dh|, down length, down |dh| (length -1 off the frame)
    float4* edge2 = nullptr;     // [max_frames][H][W]: down-right length, |dh|, down-left length, |dh|; allocated at the first 8-connected run
    uint32_t* flags = nullptr;   // [2][F][ntiles], by round parity; sized for cap_f fields, grows only
    uint32_t* cnt = nullptr;     // [kSolveCnt] counters, then kSolveTail words per frame of max_frames for the caller's after-batch kernel
    uint32_t* host = nullptr;    // pinned: the cnt block as read back
    std::vector<uint32_t> flags0;   // [2][F][ntiles]: round 0's tile flags, built on the host, and the zeroes of the other parity
    int cap_f = 0, tx = 0, ty = 0;
    long long rounds = 0, tile_runs = 0;   // of the last run
};

namespace yh {

struct PathParams {
    int W, H, tx, ntiles;
    const uint32_t* map;
    const float4 *conn0, *conn1;
    float4* edge;
    float4* edge2;   // 8-connected plans only (else nullptr)
    float* cost;
    int32_t* next;
    uint32_t* flags;
};

constexpr int kSolveCnt = SP_BATCH + 1, kSolveTail = 42;   // cnt[j + 1] = tiles flagged by round j of the batch; the tail: words per frame

// What a kind of run (plan, tour) remembers of its last one, as far as the shared time and read code needs it
struct SolveLast {
    bool planned = false;
    uint64_t frame = 0;
    int32_t start = 0, path_len = 0, conn = 4;
    int2* nodes = nullptr;    // the route
    float2* dirs = nullptr;
};
struct SolveCopy { void* dst; const void* src; size_t bytes; };   // a device array a read hands out (skipped if dst is null)
// A round kernel other than field_round (the turn planner's, scene_turn.hip): launch(tiles, parity, cnt_next) enqueues one round over
// the grid of tiles with the flags of that parity; states: the states per pixel, which scale the round cap
struct SolveRound { std::function<void(const dim3&, int, uint32_t*)> launch; int states; };

// The per-call inputs of a frame-major planner state - seeds [ns][2] (pixel, field), then starts [n], then headings [n] or the
// turn tour's points and legs - as one pinned block the host fills and its device copy: they go up in ONE copy, and the kernels
// take pointers into dev. Both grow only. reserve waits for the stream before it frees a block that is too small.
struct PlanInputs { int32_t *host = nullptr, *dev = nullptr; size_t cap = 0; };
int plan_inputs_reserve(yh_scene* h, PlanInputs& in, size_t words);
void plan_inputs_free(PlanInputs& in);
// What the four frame-major planner states (plan, tour, turn plan, turn tour) have in common: the routes, the inputs of the last call
// (the replay of *_time runs exactly these) and its per-frame results. A yh_scene holds one frame, a yh_scene_batch's core max_frames.
struct PlanFrames {
    int2* nodes = nullptr;         // [max][route_stride] the routes
    float2* dirs = nullptr;
    int32_t* walk_out = nullptr;   // per frame: length, status (the turn tour: 4 * YH_TOUR_MAX words)
    PlanInputs in;
    SolveLast last;                // planned, frame generation, connectivity
    int n = 0;                     // frames of the last call
    std::vector<int32_t> status, path_len, last_seeds, last_field;   // per frame; per seed: its pixel and its solver field
};
// in.host filled with the seed pairs of q; returns the words they take (the caller appends the rest and uploads)
size_t plan_inputs_seeds(PlanFrames& q);
// Frame `frame`'s part of q's last call, as the read code takes it: YH_ESTATE ("it has no <what>") if that frame had no ball
int solve_frame(yh_scene* h, const PlanFrames* q, int frame, size_t route_stride, const char* what, SolveLast& one);

// Allocates what F fields of connectivity conn need on a handle of h->max_frames frames, fills p (but cost and next: the caller's),
// enqueues path_weights over the first n frames (once for all fields of a frame)
int solve_begin(yh_scene* h, int conn, int F, int n, PathParams& p);
// Relaxes the F fields at p.cost, which the caller has filled (+inf, 0 at the seeds), to their fixed points. seeds: the pixels that
// start at 0, equally many per field, field by field. who: the kind of run ("path", "tour", "batch turn", ..), for the error text. after(tail), if given, enqueues
// the caller's kernel after each batch's rounds: what it writes to tail[0 .. tail_words) (at most max_frames * kSolveTail words) arrives
// in host[kSolveCnt ..] with the counters. own, if given, is the round kernel in place of field_round<conn> over F fields of one frame
// (round 0's flags still follow conn). field_of, if given, is the ragged form: seed k belongs to field (*field_of)[k], any number per field - a field without a seed flags nothing and its tiles exit at once.
int solve_rounds(yh_scene* h, const PathParams& p, int conn, int F, const std::vector<int32_t>& seeds, const char* who, int tail_words = 0,
                 const std::function<void(uint32_t*)>& after = nullptr, const SolveRound* own = nullptr, const std::vector<int32_t>* field_of = nullptr);
// The plain tour's round kernel (field_round<conn>, scene_solve.hip) over F = n kmax fields: field z relaxes with the edge terms of
// frame z / kmax
SolveRound solve_field_round(yh_scene* h, const PathParams& p, int conn, int kmax, int F);
// run() reps times between two events; a failing run's code is returned as it is. kind, again: for the error texts ("plan", "plan again")
int solve_time(yh_scene* h, const char* kind, const char* again, const SolveLast* q, int reps, const std::function<int()>& run, float* ms, int32_t* rounds, int32_t* tile_runs);
// The checks of the read entry points (a run of this frame exists, the capacity holds the route - also asked for if per_node, an array
// among `fields` that is as long as the route), then the copies
int solve_read(yh_scene* h, const char* kind, const char* again, const SolveLast* q, std::initializer_list<SolveCopy> fields, int32_t* path_xy, float* directions,
               int32_t path_capacity, int32_t* path_len, bool per_node = false);

// Round 0's tiles for a target at (x, y), through flag(tile x, tile y) (which ignores tiles outside the grid): its own tile, the tile
// across every tile border it lies on and, with diagonals, the tile diagonally across a tile corner it lies on.
template <class F>
inline void round0_flags(int x, int y, int conn, F&& flag) {
    const int bx = x / SP_TW, by = y / SP_TH;
    const int sx = x % SP_TW == 0 ? -1 : x % SP_TW == SP_TW - 1 ? 1 : 0, sy = y % SP_TH == 0 ? -1 : y % SP_TH == SP_TH - 1 ? 1 : 0;
    flag(bx, by);
    if (sx) flag(bx + sx, by);
    if (sy) flag(bx, by + sy);
    if (conn == 8 && sx && sy) flag(bx + sx, by + sy);
}

// Frame b of a frame-major batch (b = blockIdx.z; a yh_scene has the one frame 0): the scene's fields and the edge terms advance
// by W H, cost by cost_stride: W H for the plain plan, Kmax W H for the tour, 8 W H for the turn plan, Kmax 8 W H for the turn tour,
// 0 where there is no cost yet (path_weights) or the caller advances it by field (field_round). next is the plain plan's alone: its kernels advance it themselves (scene_path.hip).
__device__ __forceinline__ PathParams frame_of(const PathParams& p, int b, size_t cost_stride) {
    PathParams q = p;
    const size_t npx = (size_t)p.W * p.H;
    q.map += b * npx; q.conn0 += b * npx; q.conn1 += b * npx; q.edge += b * npx; q.cost += b * cost_stride;
    if (q.edge2) q.edge2 += b * npx;   // (8-connected runs only)
    return q;
}

// Before the body of a one-wave walk kernel (turn_walk, tt_walk): the code that follows starts on a 64-byte instruction cache line,
// whatever the kernel's entry sequence was. One wave steps through a route for tens of milliseconds in a maze, and how its loops lie
// in the instruction cache shows: with the same instructions, the longer entry of the frame-major kernels (the frame advance) made
// turn_walk 3.5 % and tt_walk 8 % slower than the parent commit's one-frame forms; started on a cache line they run as those did
// ("One driver per kind"; tt_arrive ran 5 % and the plain tour's tour_walk 6 % slower with it than without:
// they are left where they fall).
#define SP_BODY_ON_CACHE_LINE() asm volatile(".p2align 6")

__device__ __forceinline__ float cand(float dn, float len, float dh) { return __fadd_rn(__fadd_rn(dn, len), dh); }

// One workgroup of SP_NT lanes, tile (blockIdx.x, blockIdx.y) of the field `cost`: if `mine` flags the tile, relax it to its local
// fixed point for the halo it loads, write back what got smaller, flag in `theirs` the tiles across every border that moved and
// count each newly flagged one in *cnt_next. CONN = 4: the straight edges; CONN = 8: the diagonals too - a lane reads the twelve
// cells round its 2 x 2 block (the halo has the corners), sweeps six inner and twenty outer edges, all fifty-two edge terms in
// registers (a workgroup is one wave per SIMD: the register file is not what limits it), and a lowered CORNER cell flags the tile
// diagonally across as well: that tile reads the cell in its halo, and neither side tile has to lower anything because of it.
template <int CONN>
__device__ __forceinline__ void relax_tile(const PathParams& p, float* cost, uint32_t* mine, uint32_t* theirs, uint32_t* cnt_next) {
    __shared__ float dl[(SP_TH + 2) * SP_P];
    __shared__ uint32_t active, border;
    const int tid = threadIdx.x;
    const int tile = blockIdx.y * p.tx + blockIdx.x;
    if (tid == 0) { active = mine[tile]; border = 0u; }
    __syncthreads();
    if (!active) return;   // (workgroup-uniform)
    if (tid == 0) mine[tile] = 0u;   // this array is next read two rounds on; nobody sets it during this round
    const int x0 = blockIdx.x * SP_TW, y0 = blockIdx.y * SP_TH;
    for (int i = tid; i < (SP_TH + 2) * SP_P; i += SP_NT) {
        const int ly = i / SP_P, lx = i - ly * SP_P;
        const int gx = x0 + lx - 1, gy = y0 + ly - 1;
        dl[i] = gx >= 0 && gx < p.W && gy >= 0 && gy < p.H ? cost[(size_t)gy * p.W + gx] : SP_INF;
    }
    // this lane's 2 x 2 block: a b / c d. Edge terms: (length, |dh|); an edge with an end off the frame (by the frame's geometry,
    // whatever the fields say) has length +inf: such a candidate is never smaller, a cell off the frame (ragged tiles) keeps its
    // +inf and is never stored
    const int cx = 2 * (tid % (SP_TW / 2)), cy = 2 * (tid / (SP_TW / 2));
    const int gx = x0 + cx, gy = y0 + cy;
    const bool in_a = gx < p.W && gy < p.H, in_b = gx + 1 < p.W && gy < p.H, in_c = gx < p.W && gy + 1 < p.H, in_d = gx + 1 < p.W && gy + 1 < p.H;
    const bool has_l = gx > 0, has_r = gx + 2 < p.W, has_u = gy > 0, has_d = gy + 2 < p.H;
    const float4 none = make_float4(-1.0f, 0.0f, -1.0f, 0.0f);
    const size_t ga = (size_t)gy * p.W + gx;
    const float4 ea = in_a ? p.edge[ga] : none, eb = in_b ? p.edge[ga + 1] : none;
    const float4 ec = in_c ? p.edge[ga + p.W] : none, ed = in_d ? p.edge[ga + p.W + 1] : none;
    const float4 ela = has_l && in_a ? p.edge[ga - 1] : none, elc = has_l && in_c ? p.edge[ga + p.W - 1] : none;
    const float4 eua = has_u && in_a ? p.edge[ga - p.W] : none, eub = has_u && in_b ? p.edge[ga - p.W + 1] : none;
#define SP_LEN(ok, v) ((ok) && (v) >= 0.0f ? (v) : SP_INF)
    const float l_ab = SP_LEN(in_a && in_b, ea.x), h_ab = ea.y, l_cd = SP_LEN(in_c && in_d, ec.x), h_cd = ec.y;   // inside the block
    const float l_ac = SP_LEN(in_a && in_c, ea.z), h_ac = ea.w, l_bd = SP_LEN(in_b && in_d, eb.z), h_bd = eb.w;
    const float l_la = SP_LEN(has_l && in_a, ela.x), h_la = ela.y, l_lc = SP_LEN(has_l && in_c, elc.x), h_lc = elc.y;   // to the left of a, c
    const float l_rb = SP_LEN(has_r && in_b, eb.x), h_rb = eb.y, l_rd = SP_LEN(has_r && in_d, ed.x), h_rd = ed.y;       // to the right of b, d
    const float l_ua = SP_LEN(has_u && in_a, eua.z), h_ua = eua.w, l_ub = SP_LEN(has_u && in_b, eub.z), h_ub = eub.w;   // above a, b
    const float l_dc = SP_LEN(has_d && in_c, ec.z), h_dc = ec.w, l_dd = SP_LEN(has_d && in_d, ed.z), h_dd = ed.w;       // below c, d
    // the diagonals: (length, |dh|) of the pixel's down-right and down-left edge; an up-left / up-right edge is the upper pixel's
    float l_ad = 0, h_ad = 0, l_bc = 0, h_bc = 0;                                          // inside the block
    float l_ula = 0, h_ula = 0, l_ura = 0, h_ura = 0, l_dla = 0, h_dla = 0;                // a: up-left, up-right (above b), down-left (left of c)
    float l_ulb = 0, h_ulb = 0, l_urb = 0, h_urb = 0, l_drb = 0, h_drb = 0;                // b: up-left (above a), up-right, down-right (right of d)
    float l_ulc = 0, h_ulc = 0, l_dlc = 0, h_dlc = 0, l_drc = 0, h_drc = 0;                // c: up-left (left of a), down-left, down-right (below d)
    float l_urd = 0, h_urd = 0, l_dld = 0, h_dld = 0, l_drd = 0, h_drd = 0;                // d: up-right (right of b), down-left (below c), down-right
    if constexpr (CONN == 8) {
        const bool has_r1 = gx + 1 < p.W;   // (the column of b and d)
        const float4 fa = in_a ? p.edge2[ga] : none, fb = in_b ? p.edge2[ga + 1] : none;
        const float4 fc = in_c ? p.edge2[ga + p.W] : none, fd = in_d ? p.edge2[ga + p.W + 1] : none;
        const float4 fla = has_l && in_a ? p.edge2[ga - 1] : none, frb = has_r && in_b ? p.edge2[ga + 2] : none;
        const float4 ful = has_u && has_l && in_a ? p.edge2[ga - p.W - 1] : none, fua = has_u && in_a ? p.edge2[ga - p.W] : none;
        const float4 fub = has_u && in_b ? p.edge2[ga - p.W + 1] : none, fur = has_u && has_r && in_b ? p.edge2[ga - p.W + 2] : none;
        l_ad = SP_LEN(in_a && in_d, fa.x); h_ad = fa.y; l_bc = SP_LEN(in_b && in_c, fb.z); h_bc = fb.w;
        l_ula = SP_LEN(has_u && has_l && in_a, ful.x); h_ula = ful.y; l_ura = SP_LEN(has_u && in_a && has_r1, fub.z); h_ura = fub.w;
        l_dla = SP_LEN(has_l && in_c, fa.z); h_dla = fa.w;
        l_ulb = SP_LEN(has_u && in_b, fua.x); h_ulb = fua.y; l_urb = SP_LEN(has_u && has_r && in_b, fur.z); h_urb = fur.w;
        l_drb = SP_LEN(has_r && in_d, fb.x); h_drb = fb.y;
        l_ulc = SP_LEN(has_l && in_c, fla.x); h_ulc = fla.y; l_dlc = SP_LEN(has_l && has_d && in_c, fc.z); h_dlc = fc.w;
        l_drc = SP_LEN(has_d && in_d, fc.x); h_drc = fc.y;
        l_urd = SP_LEN(has_r && in_d, frb.z); h_urd = frb.w; l_dld = SP_LEN(has_d && in_d, fd.z); h_dld = fd.w;
        l_drd = SP_LEN(has_r && has_d && in_d, fd.x); h_drd = fd.y;
    }
#undef SP_LEN
    const int ia = (cy + 1) * SP_P + cx + 1, ib = ia + 1, ic = ia + SP_P, id = ic + 1;
    __syncthreads();
    // other lanes store between two of this lane's reads: relaxed workgroup-scope atomics, so that every read is a read (and stays a
    // ds_read: a volatile access would go through the flat path)
#define SP_LD(i) __hip_atomic_load(&dl[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define SP_ST(i, v) __hip_atomic_store(&dl[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
    float va = SP_LD(ia), vb = SP_LD(ib), vc = SP_LD(ic), vd = SP_LD(id);
    const float oa = va, ob = vb, oc = vc, od = vd;
    int any;
    do {
        int ch = 0;
#pragma unroll
        for (int k = 0; k < SP_INNER; ++k) {
            const float na_l = SP_LD(ia - 1), nc_l = SP_LD(ic - 1), nb_r = SP_LD(ib + 1), nd_r = SP_LD(id + 1);
            const float na_u = SP_LD(ia - SP_P), nb_u = SP_LD(ib - SP_P), nc_d = SP_LD(ic + SP_P), nd_d = SP_LD(id + SP_P);
            float a = fminf(va, fminf(cand(na_l, l_la, h_la), cand(na_u, l_ua, h_ua)));
            float b = fminf(vb, fminf(cand(nb_r, l_rb, h_rb), cand(nb_u, l_ub, h_ub)));
            float c = fminf(vc, fminf(cand(nc_l, l_lc, h_lc), cand(nc_d, l_dc, h_dc)));
            float d = fminf(vd, fminf(cand(nd_r, l_rd, h_rd), cand(nd_d, l_dd, h_dd)));
            if constexpr (CONN == 8) {
                const float n_ul = SP_LD(ia - SP_P - 1), n_ur = SP_LD(ib - SP_P + 1), n_dl = SP_LD(ic + SP_P - 1), n_dr = SP_LD(id + SP_P + 1);
                a = fminf(a, fminf(cand(n_ul, l_ula, h_ula), fminf(cand(nb_u, l_ura, h_ura), cand(nc_l, l_dla, h_dla))));
                b = fminf(b, fminf(cand(na_u, l_ulb, h_ulb), fminf(cand(n_ur, l_urb, h_urb), cand(nd_r, l_drb, h_drb))));
                c = fminf(c, fminf(cand(na_l, l_ulc, h_ulc), fminf(cand(n_dl, l_dlc, h_dlc), cand(nd_d, l_drc, h_drc))));
                d = fminf(d, fminf(cand(nb_r, l_urd, h_urd), fminf(cand(nc_d, l_dld, h_dld), cand(n_dr, l_drd, h_drd))));
                a = fminf(a, fminf(fminf(cand(b, l_ab, h_ab), cand(c, l_ac, h_ac)), cand(d, l_ad, h_ad)));   // forwards a, b, c, d
                b = fminf(b, fminf(fminf(cand(a, l_ab, h_ab), cand(d, l_bd, h_bd)), cand(c, l_bc, h_bc)));
                c = fminf(c, fminf(fminf(cand(a, l_ac, h_ac), cand(d, l_cd, h_cd)), cand(b, l_bc, h_bc)));
                d = fminf(d, fminf(fminf(cand(b, l_bd, h_bd), cand(c, l_cd, h_cd)), cand(a, l_ad, h_ad)));
                c = fminf(c, cand(d, l_cd, h_cd));                                                           // and back
                b = fminf(b, fminf(cand(d, l_bd, h_bd), cand(c, l_bc, h_bc)));
                a = fminf(a, fminf(fminf(cand(b, l_ab, h_ab), cand(c, l_ac, h_ac)), cand(d, l_ad, h_ad)));
            } else {
                a = fminf(a, fminf(cand(b, l_ab, h_ab), cand(c, l_ac, h_ac)));       // forwards a, b, c, d
                b = fminf(b, fminf(cand(a, l_ab, h_ab), cand(d, l_bd, h_bd)));
                c = fminf(c, fminf(cand(a, l_ac, h_ac), cand(d, l_cd, h_cd)));
                d = fminf(d, fminf(cand(b, l_bd, h_bd), cand(c, l_cd, h_cd)));
                c = fminf(c, cand(d, l_cd, h_cd));                                   // and back
                b = fminf(b, cand(d, l_bd, h_bd));
                a = fminf(a, fminf(cand(b, l_ab, h_ab), cand(c, l_ac, h_ac)));
            }
            if (a < va) { SP_ST(ia, a); va = a; ch = 1; }
            if (b < vb) { SP_ST(ib, b); vb = b; ch = 1; }
            if (c < vc) { SP_ST(ic, c); vc = c; ch = 1; }
            if (d < vd) { SP_ST(id, d); vd = d; ch = 1; }
        }
        any = __syncthreads_or(ch);
    } while (any);
#undef SP_LD
#undef SP_ST
    // back to the field, and which borders moved
    uint32_t* cu = reinterpret_cast<uint32_t*>(cost);
    const bool ca = va < oa, cb = vb < ob, cc = vc < oc, cd = vd < od;
    if (ca && in_a) atomicMin(cu + ga, __float_as_uint(va));
    if (cb && in_b) atomicMin(cu + ga + 1, __float_as_uint(vb));
    if (cc && in_c) atomicMin(cu + ga + p.W, __float_as_uint(vc));
    if (cd && in_d) atomicMin(cu + ga + p.W + 1, __float_as_uint(vd));
    uint32_t m = 0u;
    if (cx == 0 && (ca || cc)) m |= 1u;
    if (cx == SP_TW - 2 && (cb || cd)) m |= 2u;
    if (cy == 0 && (ca || cb)) m |= 4u;
    if (cy == SP_TH - 2 && (cc || cd)) m |= 8u;
    if constexpr (CONN == 8) {   // the four corner cells: bits 4 .. 7 = up-left, up-right, down-left, down-right
        if (cx == 0 && cy == 0 && ca) m |= 16u;
        if (cx == SP_TW - 2 && cy == 0 && cb) m |= 32u;
        if (cx == 0 && cy == SP_TH - 2 && cc) m |= 64u;
        if (cx == SP_TW - 2 && cy == SP_TH - 2 && cd) m |= 128u;
    }
    if (m) atomicOr(&border, m);
    __syncthreads();
    if (tid < CONN && ((border >> tid) & 1u)) {
        const int sx = tid == 0 ? -1 : tid == 1 ? 1 : tid < 4 ? 0 : (tid & 1) ? 1 : -1, sy = tid < 2 ? 0 : tid == 2 ? -1 : tid == 3 ? 1 : tid < 6 ? -1 : 1;
        const int bx = (int)blockIdx.x + sx, by = (int)blockIdx.y + sy;
        if (bx >= 0 && bx < p.tx && by >= 0 && by < (int)gridDim.y && atomicExch(theirs + by * p.tx + bx, 1u) == 0u) atomicAdd(cnt_next, 1u);
    }
}

// The edges of pixel i in the successor's order (left, right, up, down, up-left, up-right, down-left, down-right; the first CONN of
// them): the neighbour's linear index (-1 off the frame) and the edge's terms. Read once per pixel, whatever the number of fields.
template <int CONN>
struct Around { int at[CONN]; float len[CONN], dh[CONN]; };

template <int CONN>
__device__ __forceinline__ Around<CONN> around(const PathParams& p, int i) {
    const int x = i % p.W, y = i / p.W;
    const bool l = x > 0, r = x + 1 < p.W, u = y > 0, d = y + 1 < p.H;
    Around<CONN> e;
    auto put = [&](int k, bool ok, int at, float len, float dh) { e.at[k] = ok ? at : -1; e.len[k] = len; e.dh[k] = dh; };
    const float4 none = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 own = p.edge[i], le = l ? p.edge[i - 1] : none, up = u ? p.edge[i - p.W] : none;
    put(0, l, i - 1, le.x, le.y);
    put(1, r, i + 1, own.x, own.y);
    put(2, u, i - p.W, up.z, up.w);
    put(3, d, i + p.W, own.z, own.w);
    if constexpr (CONN == 8) {
        const float4 own2 = p.edge2[i], ul = u && l ? p.edge2[i - p.W - 1] : none, ur = u && r ? p.edge2[i - p.W + 1] : none;
        put(4, u && l, i - p.W - 1, ul.x, ul.y);
        put(5, u && r, i - p.W + 1, ur.z, ur.w);
        put(6, d && l, i + p.W - 1, own2.z, own2.w);
        put(7, d && r, i + p.W + 1, own2.x, own2.y);
    }
    return e;
}

// next[i] of the field `cost`: the first neighbour in that order whose candidate equals d[i] bitwise, -1 if none
template <int CONN>
__device__ __forceinline__ int successor(const Around<CONN>& e, const float* cost, int i) {
    const uint32_t dv = __float_as_uint(cost[i]);
    int nx = -1;
    // (in reverse, so that the first of the order wins)
#pragma unroll
    for (int k = CONN - 1; k >= 0; --k)
        if (e.at[k] >= 0 && __float_as_uint(cand(cost[e.at[k]], e.len[k], e.dh[k])) == dv) nx = e.at[k];
    return nx;
}

// next[] of pixel blockIdx.x * 256 + threadIdx.x (scene_path.hip: plan_next)
template <int CONN>
__device__ __forceinline__ void next_body(const PathParams& p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < p.W * p.H) p.next[i] = successor(around<CONN>(p, i), p.cost, i);
}

// rot_i at node a between the step z -> a and the step a -> b (each to one of the eight neighbours): with k the number of 45-degree
// steps between the two headings, float32((4 - k) * pi / 4): pi straight on, pi / 2 for a right angle (all a 4-connected route has),
// 0 for a reversal (at a tour's junction only). Five constants, no device acosf.
__device__ __forceinline__ float rotation(int2 z, int2 a, int2 b) {
    // heading (dx, dy) -> 0 .. 7 round the compass, 4 bits each at 4 * (3 * (dy + 1) + (dx + 1))
    const uint64_t compass = 0x5ull | 0x6ull << 4 | 0x7ull << 8 | 0x4ull << 12 | 0x0ull << 20 | 0x3ull << 24 | 0x2ull << 28 | 0x1ull << 32;
    const int in = (int)(compass >> (4 * (3 * (a.y - z.y + 1) + (a.x - z.x + 1)))) & 7, out = (int)(compass >> (4 * (3 * (b.y - a.y + 1) + (b.x - a.x + 1)))) & 7;
    const int t = (in - out) & 7, k = t > 4 ? 8 - t : t;
    constexpr double pi = 3.14159265358979323846;
    return k == 0 ? (float)pi : k == 1 ? (float)(3.0 * pi / 4.0) : k == 2 ? (float)(pi / 2.0) : k == 3 ? (float)(pi / 4.0) : 0.0f;
}

// One wave chases `next` from `start` through a SP_WS x SP_WS window of it held in LDS (reloaded when the route leaves it) and
// writes the nodes it visits, start and target included. Returns their number; lost = no -1 met within W * H nodes (costs
// strictly decrease along `next`, so this cannot happen on SANE fields; the bound is what keeps the loop finite on any input).
// The nodes are visible to the whole wave on return.
__device__ __forceinline__ int chase(const int32_t* next, int W, int H, int start, int2* nodes, bool& lost) {
    __shared__ int win[SP_WS * SP_WS];
    const int lane = threadIdx.x, npx = W * H;
    int cx = start % W, cy = start / W, n = 0;
    bool done = false;
    lost = false;
    while (!done && !lost) {   // (wave-uniform)
        const int wx0 = max(0, min(cx - SP_WS / 2, W - SP_WS)), wy0 = max(0, min(cy - SP_WS / 2, H - SP_WS));
        for (int i = lane; i < SP_WS * SP_WS; i += 64) {
            const int gx = wx0 + i % SP_WS, gy = wy0 + i / SP_WS;
            win[i] = gx < W && gy < H ? next[(size_t)gy * W + gx] : -1;
        }
        __syncthreads();
        while (true) {
            if (n >= npx) { lost = true; break; }
            if (lane == 0) nodes[n] = make_int2(cx, cy);
            ++n;
            const int nx = win[(cy - wy0) * SP_WS + (cx - wx0)];
            if (nx < 0) { done = true; break; }
            cx = nx % W; cy = nx / W;
            if (cx < wx0 || cx >= wx0 + SP_WS || cy < wy0 || cy >= wy0 + SP_WS) break;
        }
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    return n;
}

// The edge terms of pixel blockIdx.x * 256 + threadIdx.x (scene_solve.hip: path_weights)
template <int CONN>
__device__ __forceinline__ void weights_body(const PathParams& p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.W * p.H) return;
    const int x = i % p.W, y = i / p.W;
    const float h = (float)p.map[i];
    const float hr = x + 1 < p.W ? fabsf(__fsub_rn(h, (float)p.map[i + 1])) : 0.0f;
    const float hd = y + 1 < p.H ? fabsf(__fsub_rn(h, (float)p.map[i + p.W])) : 0.0f;
    const float4 c0 = p.conn0[i], c1 = p.conn1[i];
    p.edge[i] = make_float4(x + 1 < p.W ? c0.z : -1.0f, hr, y + 1 < p.H ? c1.x : -1.0f, hd);
    if constexpr (CONN == 8) {
        const bool dr = x + 1 < p.W && y + 1 < p.H, dl = x > 0 && y + 1 < p.H;
        const float hdr = dr ? fabsf(__fsub_rn(h, (float)p.map[i + p.W + 1])) : 0.0f;
        const float hdl = dl ? fabsf(__fsub_rn(h, (float)p.map[i + p.W - 1])) : 0.0f;
        p.edge2[i] = make_float4(dr ? c0.w : -1.0f, hdr, dl ? c1.y : -1.0f, hdl);
    }
}

// One wave (scene_path.hip: plan_walk): the route from `start` and its directions.
// out[0] = nodes on the route (start and target included), out[1] = 0, or 1 if the walk did not end within W * H nodes (costs
// strictly decrease along `next`, so this cannot happen on SANE fields; the bound is what keeps the loop finite on any input)
__device__ __forceinline__ void walk_body(const PathParams& p, int start, int2* nodes, float2* dirs, int32_t* out) {
    const int lane = threadIdx.x;
    bool lost;
    const int n = chase(p.next, p.W, p.H, start, nodes, lost);
    // directions[i] = (d[n_i] - d[n_i+1], rot_i): rot_0 = 0, else the angle at n_i between n_i-1 and n_i+1 - on a 4-grid without
    // backtracking pi when straight, pi / 2 for a turn; with diagonals 3 pi / 4 and pi / 4 too (constants, not a device acosf)
    for (int i = lane; i + 1 < n; i += 64) {
        const int2 a = nodes[i], b = nodes[i + 1];
        const float mag = __fsub_rn(p.cost[(size_t)a.y * p.W + a.x], p.cost[(size_t)b.y * p.W + b.x]);
        dirs[i] = make_float2(mag, i > 0 ? rotation(nodes[i - 1], a, b) : 0.0f);
    }
    if (lane == 0) { out[0] = n; out[1] = lost ? 1 : 0; }
}

}  // namespace yh
