// scene_register_dev.h — the scene memory's registration (scene_register.hip; the definition is DESIGN.md section 11 "Scene memory:
// registration"): the frame's stamps N scored against the memory M over a grid of candidate motions, the best one chosen on the
// device, and the record the fuse and the ball carry then read their motion from.
// register_scores_body: S(k, u, v) = sum over pixels of min(N[y][x], M[sy + v][sx + u]) for every shift of one base motion, one tile.
// register_select_body: the argmax under the tie rule, and the chosen candidate's twelve coefficients.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scene_memory_dev.h"

namespace yh {

#define SR_MAX_ROT 16
#define SR_MAX_R 8
#define SR_MAX_NU (2 * SR_MAX_R + 1)   // 17 shifts a side

// the base motions, by value in the kernel arguments (784 bytes): host arrays are free when the call returns
struct SceneRegisterBases {
    int n_rot, radius;
    int g[SR_MAX_ROT][6];   // gather_q16 of base k
    int c[SR_MAX_ROT][6];   // carry_q16 of base k
};

// what the select kernel leaves for scene_fuse_dev, scene_balls_memory_dev and yh_scene_motion_read
struct SceneRegisterRecord {
    int chosen[3];                 // k, u, v
    int pad;
    unsigned long long score[3];   // S chosen, S(0, 0, 0), sum_n
    int g[6], c[6];                // the chosen candidate's gather and carry
};

struct SceneRegisterParams {
    const uint32_t* stamp;      // N [H][W]
    const uint32_t* mem;        // M [H][W]
    unsigned long long* acc;    // [0] = sum_n, then scores [n_rot][2R+1][2R+1] (v, then u): cleared before the launch
    int W, H;
};

// Geometry of one workgroup (256 lanes, 4 waves): a tile of 64 x 16 pixels of N; wave w owns rows w, w + 4, w + 8, w + 12, a lane
// one column, so a lane holds four N values and four base sources in registers and a wave's reads of a window row are 64
// consecutive words. 300 tiles at 640 x 480.
#define SR_TW 64
#define SR_TH 16
#define SR_PX (SR_TH / 4)
// The window of M a tile can read, staged in LDS when pitch x rows fits this many words (16 KiB; with the 2.3 KiB of partial sums
// LDS would allow eight workgroups a CU, the 119 registers allow four; 32 KiB measured 22 % slower at n_rot 9, R 8).
// A rigid motion of up to 0.25 rad fits at R = 8 ((64 + 4 + 1 + 16 | 1) x (16 + 16 + 1 + 16) = 85 x 49), and so does a quarter
// turn (33 x 80); a magnification by 2 does not.
#define SR_LDS_WORDS 4096

// sum over the wave of v[0 .. 16], each a 64-bit lane-private partial. v[0 .. 15] go through a transposing butterfly: at lane bit
// 32, 16, 8, 4 a lane keeps one half of its values and sends the other to its partner, so 8 + 4 + 2 + 1 exchanges leave ONE sum per
// lane - u = (lane >> 2) & 15 - and two plain steps over bits 2 and 1 finish it: 17 exchanges where sixteen butterflies take 96.
// v[16] takes a plain butterfly. Returns the sum of value u_of_lane in `mine` and that of v[16] in `last` (every lane).
__device__ __forceinline__ void register_wave_sums(unsigned long long (&v)[SR_MAX_NU], int lane, unsigned long long& mine, unsigned long long& last) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int half = 8 >> s, bit = 32 >> s;
        const bool up = (lane & bit) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            const unsigned long long lo = v[i], hi = v[i + half];   // (both read first: a select of two array cells would pin the array in memory)
            v[i] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, bit);
        }
    }
    unsigned long long a = v[0], b = v[SR_MAX_NU - 1];
    a += __shfl_xor(a, 2);
    a += __shfl_xor(a, 1);
#pragma unroll
    for (int bit = 32; bit >= 1; bit >>= 1) b += __shfl_xor(b, bit);
    mine = a; last = b;
}

__device__ __forceinline__ void register_scores_body(const SceneRegisterParams& p, const SceneRegisterBases& bases) {
    __shared__ uint32_t win[SR_LDS_WORDS];
    __shared__ unsigned long long part[SR_MAX_NU * SR_MAX_NU];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_x = (p.W + SR_TW - 1) / SR_TW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * SR_TW, y0 = ty * SR_TH;
    const int k = blockIdx.y, R = bases.radius, nu = 2 * R + 1;
    const int x = x0 + lane;

    uint32_t n[SR_PX];
    uint32_t any = 0u;
#pragma unroll
    for (int r = 0; r < SR_PX; ++r) {
        const int y = y0 + wave + 4 * r;
        n[r] = (x < p.W && y < p.H) ? p.stamp[(size_t)y * p.W + x] : 0u;
        any |= n[r];
    }
    // nothing stamped in this tile: every min is 0 (uniform over the workgroup: the barrier's own reduction of the waves' ballots)
    if (!__syncthreads_or(any != 0u)) return;

    unsigned long long sum = 0;
#pragma unroll
    for (int r = 0; r < SR_PX; ++r) sum += n[r];
    if (k == 0) {   // sum_n, once per tile
#pragma unroll
        for (int bit = 32; bit >= 1; bit >>= 1) sum += __shfl_xor(sum, bit);
        if (lane == 0 && sum) atomicAdd(p.acc, sum);
    }

    const int g0 = bases.g[k][0], g1 = bases.g[k][1], g2 = bases.g[k][2], g3 = bases.g[k][3], g4 = bases.g[k][4], g5 = bases.g[k][5];
    // the tile's sources lie in the box its four corners span (affine, and floor is monotone)
    const int x1 = min(x0 + SR_TW, p.W) - 1, y1 = min(y0 + SR_TH, p.H) - 1;
    const long long ax = affine_q16(g0, g1, g2, x0, y0), bx = affine_q16(g0, g1, g2, x1, y0), cx = affine_q16(g0, g1, g2, x0, y1), dx = affine_q16(g0, g1, g2, x1, y1);
    const long long ay = affine_q16(g3, g4, g5, x0, y0), by = affine_q16(g3, g4, g5, x1, y0), cy = affine_q16(g3, g4, g5, x0, y1), dy = affine_q16(g3, g4, g5, x1, y1);
    const long long wx0 = min(min(ax, bx), min(cx, dx)) - R, wx1 = max(max(ax, bx), max(cx, dx)) + R;
    const long long wy0 = min(min(ay, by), min(cy, dy)) - R, wy1 = max(max(ay, by), max(cy, dy)) + R;
    // (each extent first, so that the product stays small; the pitch is odd: a quarter turn reads a window COLUMN per wave, and the
    // banks of ds_read_b32 are word address mod 32)
    const long long ww = wx1 - wx0 + 1, wh = wy1 - wy0 + 1;
    const bool in_lds = ww <= SR_LDS_WORDS && wh <= SR_LDS_WORDS && (ww | 1) * wh <= SR_LDS_WORDS;
    const int pitch = in_lds ? (int)(ww | 1) : 0;

    for (int i = tid; i < nu * nu; i += 256) part[i] = 0ull;
    long long sx[SR_PX], sy[SR_PX];   // the fallback's sources
    int off[SR_PX];                   // the staged path's: window cell of the source shifted by (-R, -R)
#pragma unroll
    for (int r = 0; r < SR_PX; ++r) {
        const int y = y0 + wave + 4 * r;
        sx[r] = affine_q16(g0, g1, g2, x, y); sy[r] = affine_q16(g3, g4, g5, x, y);
        // (a lane off the frame has N = 0 and reads cell 0: its source need not lie in the window)
        off[r] = (in_lds && x < p.W && y < p.H) ? (int)(sy[r] - R - wy0) * pitch + (int)(sx[r] - R - wx0) : 0;
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

    for (int vi = 0; vi < nu; ++vi) {
        unsigned long long acc[SR_MAX_NU];
#pragma unroll
        for (int ui = 0; ui < SR_MAX_NU; ++ui) acc[ui] = 0ull;
        if (in_lds) {
#pragma unroll
            for (int r = 0; r < SR_PX; ++r) {
                const uint32_t* row = win + off[r] + vi * pitch;
#pragma unroll
                for (int ui = 0; ui < SR_MAX_NU; ++ui)
                    if (ui < nu) acc[ui] += min(n[r], row[ui]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < SR_PX; ++r) {
                const long long my = sy[r] + (vi - R);
                const bool row_in = my >= 0 && my < p.H;
#pragma unroll
                for (int ui = 0; ui < SR_MAX_NU; ++ui) {
                    if (ui < nu) {
                        const long long mx = sx[r] + (ui - R);
                        uint32_t q = 0u;
                        if (n[r] != 0u && row_in && mx >= 0 && mx < p.W) q = p.mem[(size_t)my * p.W + (size_t)mx];
                        acc[ui] += min(n[r], q);
                    }
                }
            }
        }
        unsigned long long mine, last;
        register_wave_sums(acc, lane, mine, last);
        const int u = (lane >> 2) & 15;
        if ((lane & 3) == 0 && u < nu && mine) atomicAdd(&part[vi * nu + u], mine);
        if (lane == 0 && nu == SR_MAX_NU && last) atomicAdd(&part[vi * nu + SR_MAX_NU - 1], last);
    }
    __syncthreads();
    // one 64-bit add per tile and shift: integer sums, so the order the tiles arrive in changes nothing
    unsigned long long* scores = p.acc + 1 + (size_t)k * nu * nu;
    for (int i = tid; i < nu * nu; i += 256) {
        const unsigned long long s = part[i];
        if (s) atomicAdd(scores + i, s);
    }
}

// whether candidate (s, d2, i) beats (bs, bd, bi): the larger S, then the smaller u^2 + v^2, then the smaller index - which, the
// table being [k][v][u], is the smaller k, then v, then u
__device__ __forceinline__ bool register_better(unsigned long long s, int d2, int i, unsigned long long bs, int bd, int bi) {
    if (s != bs) return s > bs;
    if (d2 != bd) return d2 < bd;
    return i < bi;
}

// one workgroup of 256 lanes
__device__ __forceinline__ void register_select_body(const unsigned long long* acc, const SceneRegisterBases& bases, SceneRegisterRecord* rec) {
    __shared__ unsigned long long bs[256];
    __shared__ int bd[256], bi[256];
    const int tid = threadIdx.x, R = bases.radius, nu = 2 * R + 1, nn = nu * nu, total = bases.n_rot * nn;
    const unsigned long long* scores = acc + 1;
    unsigned long long s = 0ull;
    int d2 = 0x7fffffff, best = 0x7fffffff;   // (loses to every real candidate; total >= 1, so lane 0 always holds one)
    for (int i = tid; i < total; i += 256) {
        const int r = i % nn, v = r / nu - R, u = r % nu - R;
        const unsigned long long si = scores[i];
        if (best == 0x7fffffff || register_better(si, u * u + v * v, i, s, d2, best)) { s = si; d2 = u * u + v * v; best = i; }
    }
    bs[tid] = s; bd[tid] = d2; bi[tid] = best;
    __syncthreads();
    for (int step = 128; step >= 1; step >>= 1) {
        if (tid < step && bi[tid + step] != 0x7fffffff &&
            (bi[tid] == 0x7fffffff || register_better(bs[tid + step], bd[tid + step], bi[tid + step], bs[tid], bd[tid], bi[tid]))) {
            bs[tid] = bs[tid + step]; bd[tid] = bd[tid + step]; bi[tid] = bi[tid + step];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const int i = bi[0], k = i / nn, r = i % nn, v = r / nu - R, u = r % nu - R;
    rec->chosen[0] = k; rec->chosen[1] = u; rec->chosen[2] = v; rec->pad = 0;
    rec->score[0] = bs[0]; rec->score[1] = scores[R * nu + R]; rec->score[2] = acc[0];
    // gather: the base's source pixel plus (u, v); carry: its inverse shifted the same way (the host has checked that all four fit)
    const int* g = bases.g[k];
    const int* c = bases.c[k];
    for (int j = 0; j < 6; ++j) { rec->g[j] = g[j]; rec->c[j] = c[j]; }
    rec->g[2] = (int)((long long)g[2] + (long long)u * 65536);
    rec->g[5] = (int)((long long)g[5] + (long long)v * 65536);
    rec->c[2] = (int)((long long)c[2] - ((long long)c[0] * u + (long long)c[1] * v));
    rec->c[5] = (int)((long long)c[5] - ((long long)c[3] * u + (long long)c[4] * v));
}

}  // namespace yh

struct yh_scene;
namespace yh {
// scene_register.hip, on the handle's stream (its device current). bases_check: the int32 conditions of the definition on n_rot
// gathers and, if given, carries (YH_EINVAL and why; touches nothing). search: acc cleared, the scores, the choice into rec.
// fuse: scene_balls_memory and scene_fuse with their motions read from rec.
size_t scene_register_acc_bytes();
int scene_register_bases_check(yh_scene* h, int32_t n_rot, const int32_t* gather_q16, const int32_t* carry_q16, int32_t radius);
int scene_register_search(yh_scene* h, const uint32_t* stamp, const uint32_t* mem, const SceneRegisterBases& bases, unsigned long long* acc, SceneRegisterRecord* rec);
int scene_register_fuse(yh_scene* h, const SceneFuseParams& f, const SceneBallsMemParams& b, const SceneRegisterRecord* rec);
}
