// scene_pyramid_norm_dev.h — the scene memory's normalised pyramid registration (scene_pyramid_norm.hip; the definition is DESIGN.md
// section 11 "Scene memory: normalised pyramid registration"): the pyramid registration of scene_pyramid_dev.h with every level
// decided by the weighted Jaccard ratio S / U of scene_register_norm_dev.h instead of by S, so that the descent itself, and not only
// the last choice, holds on a dense map. The tables of a level are register_norm_scores_body, unchanged, on that level's maps.
// pyramid_norm_select_body: per hypothesis the best qualified shift of a level and the next level's bases; at level 0 the choice
// over all hypotheses into the SceneRegisterRecord and the SceneRegisterNormRecord the flat searches leave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scene_pyramid_dev.h"
#include "scene_register_norm_dev.h"

namespace yh {

// what the select kernel leaves beside the two records, for yh_scene_pyramid_norm_read: whether any entry of hypothesis h of level l
// qualified (C >= m_l and U > 0)
struct ScenePyramidNormExt {
    int qualified[SP_MAX_LEVELS + 1][SR_MAX_ROT];
};

// m_l: min_inside carried to level l, rounded up - a cell of level l covers up to 4^l pixels
__host__ __device__ inline long long pyramid_norm_min_inside(int min_inside, int level) { return ((long long)min_inside + (1ll << (2 * level)) - 1) >> (2 * level); }

// words of the level tables of levels above `level` (each: sum_n, then S, T and C, [hyp][2 rho + 1][2 rho + 1] each); with
// level = levels + 1, of all
inline size_t pyramid_norm_acc_offset(const ScenePyramidPlan& plan, int level) {
    size_t o = 0;
    for (int l = 0; l < level; ++l) o += 1 + 3 * register_norm_table_words(plan.hyp(l), plan.rho(l));
    return o;
}

// register_norm_scores_body (scene_register_norm_dev.h) for the rows of shifts vi0 <= vi < vi1 alone: a copy that differs in the
// range of its two loops over vi and of its last loop, and in who adds sum_n (the workgroup of the first rows: once per tile).
// The coarsest level has few tiles and (2R + 1)^2 shifts: its rows are spread over blockIdx.z. Every workgroup stages the whole
// window and zeroes the whole LDS tables, which is little at that level; S, T, C, the tile constants and tile_n are added once per
// shift, by the one workgroup that owns the shift's row.
__device__ __forceinline__ void pyramid_norm_scores_rows_body(const SceneRegisterParams& p, const SceneRegisterBases& bases, int vi0, int vi1) {
    __shared__ uint32_t win[SR_LDS_WORDS];
    __shared__ unsigned long long part_s[SR_MAX_NU * SR_MAX_NU], part_t[SR_MAX_NU * SR_MAX_NU], part_c[SR_MAX_NU * SR_MAX_NU];
    __shared__ unsigned long long tile_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_x = (p.W + SR_TW - 1) / SR_TW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * SR_TW, y0 = ty * SR_TH;
    const int k = blockIdx.y, R = bases.radius, nu = 2 * R + 1;
    const int x = x0 + lane;

    uint32_t n[SR_PX], vm[SR_PX];
    unsigned long long sum = 0;
#pragma unroll
    for (int r = 0; r < SR_PX; ++r) {
        const int y = y0 + wave + 4 * r;
        const bool valid = x < p.W && y < p.H;
        vm[r] = valid ? 0xFFFFFFFFu : 0u;
        n[r] = valid ? p.stamp[(size_t)y * p.W + x] : 0u;
        sum += n[r];
    }
#pragma unroll
    for (int bit = 32; bit >= 1; bit >>= 1) sum += __shfl_xor(sum, bit);
    if (k == 0 && vi0 == 0 && lane == 0 && sum) atomicAdd(p.acc, sum);   // sum_n, once per tile

    const int g0 = bases.g[k][0], g1 = bases.g[k][1], g2 = bases.g[k][2], g3 = bases.g[k][3], g4 = bases.g[k][4], g5 = bases.g[k][5];
    const int x1 = min(x0 + SR_TW, p.W) - 1, y1 = min(y0 + SR_TH, p.H) - 1;
    const long long ax = affine_q16(g0, g1, g2, x0, y0), bx = affine_q16(g0, g1, g2, x1, y0), cx = affine_q16(g0, g1, g2, x0, y1), dx = affine_q16(g0, g1, g2, x1, y1);
    const long long ay = affine_q16(g3, g4, g5, x0, y0), by = affine_q16(g3, g4, g5, x1, y0), cy = affine_q16(g3, g4, g5, x0, y1), dy = affine_q16(g3, g4, g5, x1, y1);
    const long long wx0 = min(min(ax, bx), min(cx, dx)) - R, wx1 = max(max(ax, bx), max(cx, dx)) + R;
    const long long wy0 = min(min(ay, by), min(cy, dy)) - R, wy1 = max(max(ay, by), max(cy, dy)) + R;
    const long long ww = wx1 - wx0 + 1, wh = wy1 - wy0 + 1;
    const bool in_lds = ww <= SR_LDS_WORDS && wh <= SR_LDS_WORDS && (ww | 1) * wh <= SR_LDS_WORDS;
    const int pitch = in_lds ? (int)(ww | 1) : 0;
    const bool all_inside = wx0 >= 0 && wx1 < p.W && wy0 >= 0 && wy1 < p.H;
    const bool full = x0 + SR_TW <= p.W && y0 + SR_TH <= p.H;

    for (int i = tid; i < nu * nu; i += 256) { part_s[i] = 0ull; part_t[i] = 0ull; part_c[i] = 0ull; }
    if (tid == 0) tile_n = 0ull;
    int off[SR_PX];
#pragma unroll
    for (int r = 0; r < SR_PX; ++r) {
        const int y = y0 + wave + 4 * r;
        const long long sx = affine_q16(g0, g1, g2, x, y), sy = affine_q16(g3, g4, g5, x, y);
        off[r] = (in_lds && vm[r]) ? (int)(sy - R - wy0) * pitch + (int)(sx - R - wx0) : 0;
    }
    if (in_lds) {
        const int cells = pitch * (int)wh;
        for (int i = tid; i < cells; i += 256) {
            const int cy_ = i / pitch, cx_ = i - cy_ * pitch;
            const long long mx = wx0 + cx_, my = wy0 + cy_;
            win[i] = (mx >= 0 && mx < p.W && my >= 0 && my < p.H) ? p.mem[(size_t)my * p.W + (size_t)mx] : 0u;
        }
    }
    __syncthreads();
    if (lane == 0 && sum) atomicAdd(&tile_n, sum);

    for (int vi = vi0; vi < vi1; ++vi) {
        unsigned long long s[SR_MAX_NU], t[SR_MAX_NU];
#pragma unroll
        for (int ui = 0; ui < SR_MAX_NU; ++ui) { s[ui] = 0ull; t[ui] = 0ull; }
        if (in_lds) {
            if (full) register_norm_row<false, true>(win, off, n, vm, vi * pitch, nu, s);
            else register_norm_row<true, true>(win, off, n, vm, vi * pitch, nu, s);
            register_norm_row_out(s, lane, nu, part_s + vi * nu);
            if (full) register_norm_row<false, false>(win, off, n, vm, vi * pitch, nu, t);
            else register_norm_row<true, false>(win, off, n, vm, vi * pitch, nu, t);
            register_norm_row_out(t, lane, nu, part_t + vi * nu);
        } else {
#pragma unroll
            for (int which = 0; which < 2; ++which) {
                unsigned long long (&a)[SR_MAX_NU] = which ? t : s;
#pragma unroll
                for (int r = 0; r < SR_PX; ++r) {
                    const int y = y0 + wave + 4 * r;
                    const long long sx = affine_q16(g0, g1, g2, x, y), my = affine_q16(g3, g4, g5, x, y) + (vi - R);
                    const bool row_in = vm[r] != 0u && my >= 0 && my < p.H;
#pragma unroll
                    for (int ui = 0; ui < SR_MAX_NU; ++ui) {
                        if (ui < nu) {
                            const long long mx = sx + (ui - R);
                            uint32_t q = 0u;
                            if (row_in && mx >= 0 && mx < p.W) q = p.mem[(size_t)my * p.W + (size_t)mx];
                            a[ui] += which ? q : min(n[r], q);
                        }
                    }
                }
                register_norm_row_out(a, lane, nu, (which ? part_t : part_s) + vi * nu);
            }
        }
    }

    if (!all_inside) {
        uint32_t cols[SR_PX];
        int vlo[SR_PX], vhi[SR_PX];
#pragma unroll
        for (int r = 0; r < SR_PX; ++r) {
            const int y = y0 + wave + 4 * r;
            const long long sx = affine_q16(g0, g1, g2, x, y), sy = affine_q16(g3, g4, g5, x, y);
            const long long ulo = max(0ll, R - sx), uhi = min((long long)nu - 1, (long long)p.W - 1 + R - sx);
            const long long lo = max(0ll, R - sy), hi = min((long long)nu - 1, (long long)p.H - 1 + R - sy);
            cols[r] = (vm[r] != 0u && ulo <= uhi) ? ((2u << (int)uhi) - (1u << (int)ulo)) : 0u;
            vlo[r] = lo <= hi ? (int)lo : 1; vhi[r] = lo <= hi ? (int)hi : 0;
        }
        for (int vi = vi0; vi < vi1; ++vi) {
            unsigned long long a[SR_MAX_NU];
#pragma unroll
            for (int ui = 0; ui < SR_MAX_NU; ++ui) a[ui] = 0ull;
#pragma unroll
            for (int r = 0; r < SR_PX; ++r) {
                const uint32_t m = (vi >= vlo[r] && vi <= vhi[r]) ? cols[r] : 0u;
#pragma unroll
                for (int ui = 0; ui < SR_MAX_NU; ++ui) {
                    if (ui < nu) {
                        const uint32_t keep = 0u - ((m >> ui) & 1u);
                        a[ui] += ((unsigned long long)(keep & (1u << (SRN_COUNT_SHIFT - 32))) << 32) | (keep & n[r]);
                    }
                }
            }
            register_norm_row_out_packed(a, lane, nu, part_t + vi * nu, part_c + vi * nu);
        }
    }
    __syncthreads();
    const size_t words = register_norm_table_words(bases.n_rot, R);
    unsigned long long* tab_s = p.acc + 1 + (size_t)k * nu * nu;
    const unsigned long long add_n = all_inside ? tile_n : 0ull, add_c = all_inside ? (unsigned long long)((x1 - x0 + 1) * (y1 - y0 + 1)) : 0ull;
    for (int i = vi0 * nu + tid; i < vi1 * nu; i += 256) {   // (the rows of this workgroup alone: the tile constants once per shift)
        const unsigned long long s = part_s[i], t = part_t[i] + add_n, c = part_c[i] + add_c;
        if (s) atomicAdd(tab_s + i, s);
        if (t) atomicAdd(tab_s + words + i, t);
        if (c) atomicAdd(tab_s + 2 * words + i, c);
    }
}

// whether qualified entry (s, u, tie) beats qualified entry (bs, bu, btie): the larger s / u - s bu against bs u as exact 128-bit
// products, as register_norm_better forms them -, then the smaller pyramid_tie key
__device__ __forceinline__ bool pyramid_norm_better(unsigned long long s, unsigned long long u, unsigned long long tie, unsigned long long bs, unsigned long long bu,
                                                    unsigned long long btie) {
    const unsigned long long ah = __umul64hi(s, bu), al = s * bu, bh = __umul64hi(bs, u), bl = bs * u;
    if (ah != bh) return ah > bh;
    if (al != bl) return al > bl;
    return tie < btie;
}

// One workgroup of 256 lanes, pyramid_select_body's shape. level > 0: hypothesis blockIdx.x of that level - its best qualified total
// shift (none qualified: its own centre), and twice it as the centre of the level below, into the table. level == 0: the choice over
// every qualified entry of every hypothesis (none: (0, 0, 0) of base 0), into rec and nrec. An entry that is not qualified never
// enters the reduction: the key ~0 marks a lane, and a slot, that holds none.
__device__ __forceinline__ void pyramid_norm_select_body(const unsigned long long* acc, ScenePyramidTable* t, int level, int min_inside, SceneRegisterRecord* rec,
                                                         SceneRegisterNormRecord* nrec, ScenePyramidNormExt* ext) {
    __shared__ unsigned long long bs[256], bu[256], bt[256];
    __shared__ int bi[256];
    __shared__ int any[SR_MAX_ROT];
    const SceneRegisterBases& bases = t->lv[level];
    const int tid = threadIdx.x, R = bases.radius, nu = 2 * R + 1, nn = nu * nu, total = bases.n_rot * nn;
    const int h0 = level ? (int)blockIdx.x : 0, h1 = level ? h0 + 1 : bases.n_rot;
    const int home = level ? -1 : bases.n_rot - 1;   // the home hypothesis counts as base 0
    const unsigned long long *tab_s = acc + 1, *tab_t = tab_s + total, *tab_c = tab_t + total;
    const unsigned long long need = (unsigned long long)pyramid_norm_min_inside(min_inside, level);
    if (tid < SR_MAX_ROT) any[tid] = 0;
    __syncthreads();
    unsigned long long s = 0ull, u = 0ull, tie = ~0ull;
    int best = 0;
    for (int i = h0 * nn + tid; i < h1 * nn; i += 256) {
        const int h = i / nn, r = i - h * nn, j = r / nu, v = t->centre[level][h][1] + j - R, uu = t->centre[level][h][0] + (r - j * nu) - R;
        const unsigned long long si = tab_s[i], ui = tab_t[i] - si;
        if (tab_c[i] < need || ui == 0ull) continue;
        any[h] = 1;   // (every writer writes the same value)
        const unsigned long long ti = pyramid_tie(h == home ? 0 : (level ? 0 : h), uu, v);
        if (tie == ~0ull || pyramid_norm_better(si, ui, ti, s, u, tie)) { s = si; u = ui; tie = ti; best = i; }
    }
    bs[tid] = s; bu[tid] = u; bt[tid] = tie; bi[tid] = best;
    __syncthreads();
    for (int step = 128; step >= 1; step >>= 1) {
        if (tid < step && bt[tid + step] != ~0ull &&
            (bt[tid] == ~0ull || pyramid_norm_better(bs[tid + step], bu[tid + step], bt[tid + step], bs[tid], bu[tid], bt[tid]))) {
            bs[tid] = bs[tid + step]; bu[tid] = bu[tid + step]; bt[tid] = bt[tid + step]; bi[tid] = bi[tid + step];
        }
        __syncthreads();
    }
    if (tid >= h0 && tid < h1) ext->qualified[level][tid] = any[tid];
    if (tid != 0) return;
    const unsigned long long key = bt[0];
    const int qualified = key != ~0ull;
    int u_ = (int)(key & 255) - 128, v_ = (int)((key >> 8) & 255) - 128, k = (int)((key >> 16) & 15);
    if (level) {   // (the host has checked that the shifted offsets of every level fit int32)
        if (!qualified) { u_ = t->centre[level][h0][0]; v_ = t->centre[level][h0][1]; }
        const int below = level - 1;
        t->centre[below][h0][0] = 2 * u_; t->centre[below][h0][1] = 2 * v_;
        t->lv[below].g[h0][2] = (int)((long long)t->home[below][h0][0] + 2ll * u_ * 65536);
        t->lv[below].g[h0][5] = (int)((long long)t->home[below][h0][1] + 2ll * v_ * 65536);
        return;
    }
    const int prior = home * nn + R * nu + R;   // (0, 0, 0): the home hypothesis' centre
    if (!qualified) { u_ = 0; v_ = 0; k = 0; }
    const int at = qualified ? bi[0] : prior;
    rec->chosen[0] = k; rec->chosen[1] = u_; rec->chosen[2] = v_; rec->pad = 0;
    rec->score[0] = tab_s[at]; rec->score[1] = tab_s[prior]; rec->score[2] = acc[0];
    nrec->chosen[0] = tab_s[at]; nrec->chosen[1] = tab_t[at]; nrec->chosen[2] = tab_c[at];
    nrec->prior[0] = tab_s[prior]; nrec->prior[1] = tab_t[prior]; nrec->prior[2] = tab_c[prior];
    nrec->qualified = qualified; nrec->pad = 0;
    // gather and carry of the choice: as pyramid_select_body builds them
    const int* g = bases.g[k];
    const int* c = bases.c[k];
    for (int j = 0; j < 6; ++j) { rec->g[j] = g[j]; rec->c[j] = c[j]; }
    rec->g[2] = (int)((long long)t->home[0][k][0] + (long long)u_ * 65536);
    rec->g[5] = (int)((long long)t->home[0][k][1] + (long long)v_ * 65536);
    rec->c[2] = (int)((long long)c[2] - ((long long)c[0] * u_ + (long long)c[1] * v_));
    rec->c[5] = (int)((long long)c[5] - ((long long)c[3] * u_ + (long long)c[4] * v_));
}

struct ScenePyramidNormBufs {
    unsigned long long* acc = nullptr;    // the level tables, level 0 first, contiguous: three times the plain pyramid's
    ScenePyramidNormExt* ext = nullptr;
};

}  // namespace yh

struct yh_scene;
namespace yh {
// scene_pyramid_norm.hip, on the handle's stream (its device current). The plan, the table and the pooled levels are the plain
// pyramid's (scene_pyramid_plan_make, ScenePyramidBufs: its acc is not used). search: the table uploaded (unless replayed), the
// levels of both maps, the level tables cleared, tables and select per level, the choice into rec and nrec, the flags into nb.ext.
size_t scene_pyramid_norm_acc_bytes();
int scene_pyramid_norm_reserve(yh_scene* h, ScenePyramidNormBufs& nb);
void scene_pyramid_norm_release(ScenePyramidNormBufs& nb);
int scene_pyramid_norm_search(yh_scene* h, const uint32_t* stamp, const uint32_t* mem, const ScenePyramidPlan& plan, int min_inside, const ScenePyramidBufs& b,
                              const ScenePyramidNormBufs& nb, SceneRegisterRecord* rec, SceneRegisterNormRecord* nrec, bool upload);
}
