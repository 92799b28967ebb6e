// scene_pyramid_dev.h — the scene memory's pyramid registration (scene_pyramid.hip; the definition is DESIGN.md section 11 "Scene
// memory: pyramid registration"): the registration of scene_register_dev.h run coarse to fine over max-pooled levels of N and M.
// pyramid_body: levels 1 .. L of one map, every level formed in the wave that loaded its pixels and written once.
// pyramid_select_body: per hypothesis the best shift of a level and the next level's bases; at level 0 the choice over all of them
// into the SceneRegisterRecord the plain search leaves. The scores of a level are register_scores_body, unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "scene_register_dev.h"

namespace yh {

#define SP_MAX_LEVELS 3
#define SP_MAX_ROT (SR_MAX_ROT - 1)   // one slot of a level's bases is the home hypothesis'

// Geometry of one workgroup (256 lanes, 4 waves): a tile of 64 x 16 pixels, a wave 32 x 8 of them, a lane one 2 x 2 quad - lane
// bits 0 .. 3 the quad's column, bits 4 .. 5 its row - so a wave's loads of a pixel row are 128 consecutive bytes and the wave holds
// whole cells of every level up to 3 (8 x 8 pixels): the further levels are cross-lane maxima, no LDS and no second read.
#define SP_TW 64
#define SP_TH 16

struct ScenePyramidParams {
    const uint32_t* src[2];             // level 0 of N and of M, [H][W]
    uint32_t* dst[2][SP_MAX_LEVELS];    // their levels 1 .. L
    int W, H, levels;
};

// The device table of one search. The host uploads it whole; pyramid_select then writes only lv[l].g[k][2], lv[l].g[k][5] and
// centre[l][k] of the levels below L, from `home`, so that the same launches on the same table give the same table again.
struct ScenePyramidTable {
    SceneRegisterBases lv[SP_MAX_LEVELS + 1];     // level l as scored: n_rot = its hypotheses, radius = its radius, g = the level gather with the centre added; lv[0].c = the carries
    int home[SP_MAX_LEVELS + 1][SR_MAX_ROT][2];   // c_l, f_l of the level gather around centre (0, 0)
    int centre[SP_MAX_LEVELS + 1][SR_MAX_ROT][2]; // the centre each hypothesis of the level is scored around
};

__host__ __device__ inline int pyramid_dim(int n, int level) { return (n + (1 << level) - 1) >> level; }

__device__ __forceinline__ uint32_t pyramid_quad(const uint32_t* __restrict__ src, int W, int H, int x, int y) {
    uint32_t v = 0u;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (y + j >= H) continue;
        const uint32_t* row = src + (size_t)(y + j) * W + x;
        if (x + 1 < W) {   // (a row of odd width starts at an odd word: 4-byte aligned, one 8-byte load all the same)
            uint32_t two[2];
            memcpy(two, row, 8);
            v = max(v, max(two[0], two[1]));
        } else if (x < W) {
            v = max(v, row[0]);
        }
    }
    return v;
}

__device__ __forceinline__ void pyramid_body(const ScenePyramidParams& p) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int which = blockIdx.y;
    const int tiles_x = (p.W + SP_TW - 1) / SP_TW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int qx = lane & 15, qy = lane >> 4;
    const int x = tx * SP_TW + (wave & 1) * 32 + 2 * qx, y = ty * SP_TH + (wave >> 1) * 8 + 2 * qy;
    const bool in = x < p.W && y < p.H;   // (x and y are even: the cell (x >> l, y >> l) exists at level l exactly if the pixel does)
    // u32 maxima: a zero for what lies outside changes nothing
    uint32_t v = pyramid_quad(which ? p.src[1] : p.src[0], p.W, p.H, x, y);
    uint32_t* d1 = which ? p.dst[1][0] : p.dst[0][0];
    if (in) d1[(size_t)(y >> 1) * pyramid_dim(p.W, 1) + (x >> 1)] = v;
    if (p.levels < 2) return;   // (uniform)
    v = max(v, (uint32_t)__shfl_xor((int)v, 1));
    v = max(v, (uint32_t)__shfl_xor((int)v, 16));
    uint32_t* d2 = which ? p.dst[1][1] : p.dst[0][1];
    if (in && !(qx & 1) && !(qy & 1)) d2[(size_t)(y >> 2) * pyramid_dim(p.W, 2) + (x >> 2)] = v;
    if (p.levels < 3) return;
    v = max(v, (uint32_t)__shfl_xor((int)v, 2));
    v = max(v, (uint32_t)__shfl_xor((int)v, 32));
    uint32_t* d3 = which ? p.dst[1][2] : p.dst[0][2];
    if (in && !(qx & 3) && !(qy & 3)) d3[(size_t)(y >> 3) * pyramid_dim(p.W, 3) + (x >> 3)] = v;
}

// the order among equal scores as one number, the smaller the better: u^2 + v^2 of the total shift (< 2^15: |u|, |v| <= 120), then
// k, then v, then u
__device__ __forceinline__ unsigned long long pyramid_tie(int k, int u, int v) {
    return ((unsigned long long)(u * u + v * v) << 20) | ((unsigned long long)k << 16) | ((unsigned long long)(v + 128) << 8) | (unsigned long long)(u + 128);
}

// One workgroup of 256 lanes. level > 0: hypothesis blockIdx.x of that level - its best total shift, and twice it as the centre of
// the level below, into the table. level == 0: the choice over every entry of every hypothesis, into rec.
__device__ __forceinline__ void pyramid_select_body(const unsigned long long* acc, ScenePyramidTable* t, int level, SceneRegisterRecord* rec) {
    __shared__ unsigned long long bs[256], bt[256];
    const SceneRegisterBases& bases = t->lv[level];
    const int tid = threadIdx.x, R = bases.radius, nu = 2 * R + 1, nn = nu * nu;
    const int h0 = level ? (int)blockIdx.x : 0, h1 = level ? h0 + 1 : bases.n_rot;
    const int home = level ? -1 : bases.n_rot - 1;   // the home hypothesis counts as base 0
    const unsigned long long* scores = acc + 1;
    unsigned long long s = 0ull, tie = ~0ull;   // (loses to every real candidate, or ties with score 0 and loses on the order)
    for (int i = h0 * nn + tid; i < h1 * nn; i += 256) {
        const int h = i / nn, r = i - h * nn, j = r / nu, v = t->centre[level][h][1] + j - R, u = t->centre[level][h][0] + (r - j * nu) - R;
        const unsigned long long si = scores[i], ti = pyramid_tie(h == home ? 0 : (level ? 0 : h), u, v);
        if (si > s || (si == s && ti < tie)) { s = si; tie = ti; }
    }
    bs[tid] = s; bt[tid] = tie;
    __syncthreads();
    for (int step = 128; step >= 1; step >>= 1) {
        if (tid < step && (bs[tid + step] > bs[tid] || (bs[tid + step] == bs[tid] && bt[tid + step] < bt[tid]))) { bs[tid] = bs[tid + step]; bt[tid] = bt[tid + step]; }
        __syncthreads();
    }
    if (tid != 0) return;
    const unsigned long long best = bt[0];
    const int u = (int)(best & 255) - 128, v = (int)((best >> 8) & 255) - 128, k = (int)((best >> 16) & 15);
    if (level) {   // (the host has checked that the shifted offsets of every level fit int32)
        const int below = level - 1;
        t->centre[below][h0][0] = 2 * u; t->centre[below][h0][1] = 2 * v;
        t->lv[below].g[h0][2] = (int)((long long)t->home[below][h0][0] + 2ll * u * 65536);
        t->lv[below].g[h0][5] = (int)((long long)t->home[below][h0][1] + 2ll * v * 65536);
        return;
    }
    rec->chosen[0] = k; rec->chosen[1] = u; rec->chosen[2] = v; rec->pad = 0;
    rec->score[0] = bs[0]; rec->score[1] = scores[home * nn + R * nu + R]; rec->score[2] = acc[0];
    const int* g = bases.g[k];
    const int* c = bases.c[k];
    for (int j = 0; j < 6; ++j) { rec->g[j] = g[j]; rec->c[j] = c[j]; }
    rec->g[2] = (int)((long long)t->home[0][k][0] + (long long)u * 65536);
    rec->g[5] = (int)((long long)t->home[0][k][1] + (long long)v * 65536);
    rec->c[2] = (int)((long long)c[2] - ((long long)c[0] * u + (long long)c[1] * v));
    rec->c[5] = (int)((long long)c[5] - ((long long)c[3] * u + (long long)c[4] * v));
}

// what one pyramid search runs on, on the host: the table as uploaded, and where each level's maps and score table lie
struct ScenePyramidPlan {
    int n_rot = 0, levels = 0, radius = 0, refine = 0;
    ScenePyramidTable table = {};
    int hyp(int level) const { return level ? n_rot : n_rot + 1; }
    int rho(int level) const { return level == levels ? radius : refine; }
    // words of the score tables of levels above `level` (each: sum_n, then [hyp][2 rho + 1][2 rho + 1]); with level = levels + 1, of all
    size_t acc_offset(int level) const {
        size_t o = 0;
        for (int l = 0; l < level; ++l) o += 1 + (size_t)hyp(l) * (2 * rho(l) + 1) * (2 * rho(l) + 1);
        return o;
    }
};

struct ScenePyramidBufs {
    uint32_t* maps = nullptr;            // levels 1 .. 3 of N, then of M (scene_pyramid_map_words each)
    unsigned long long* acc = nullptr;   // the level tables, level 0 first, contiguous
    ScenePyramidTable* table = nullptr;
};

}  // namespace yh

struct yh_scene;
namespace yh {
// scene_pyramid.hip, on the handle's stream (its device current). plan_make: the parameter ranges and the int32 conditions of the
// definition (YH_EINVAL and why; touches nothing), then the table. search: the table uploaded (unless replayed), the levels of both
// maps, the level tables cleared, scores and select per level, the choice into rec.
size_t scene_pyramid_map_words(int W, int H);   // levels 1 .. SP_MAX_LEVELS of one map
size_t scene_pyramid_map_offset(int W, int H, int level);   // where level `level` >= 1 starts in them
size_t scene_pyramid_acc_bytes();
int scene_pyramid_plan_make(yh_scene* h, int32_t n_rot, const int32_t* gather_q16, const int32_t* carry_q16, int32_t levels, int32_t radius, int32_t refine, ScenePyramidPlan& plan);
int scene_pyramid_reserve(yh_scene* h, ScenePyramidBufs& b);
void scene_pyramid_release(ScenePyramidBufs& b);
int scene_pyramid_search(yh_scene* h, const uint32_t* stamp, const uint32_t* mem, const ScenePyramidPlan& plan, const ScenePyramidBufs& b, SceneRegisterRecord* rec, bool upload);
void scene_pyramid_levels(yh_scene* h, const uint32_t* stamp, const uint32_t* mem, int levels, const ScenePyramidBufs& b, ScenePyramidParams& pp);
}
