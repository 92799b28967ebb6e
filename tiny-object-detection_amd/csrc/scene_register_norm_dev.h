// scene_register_norm_dev.h — the scene memory's normalised registration (scene_register_norm.hip; the definition is DESIGN.md
// section 11 "Scene memory: normalised registration"): the plain search's candidates, ranked by the weighted Jaccard ratio S / U over
// the pixels both maps cover instead of by S alone, so that a dense map's large true shift does not lose to "no motion".
// register_norm_scores_body: for every shift of one base motion, one tile: S = sum over inside pixels of min(N, Q), T = sum over
//                            inside pixels of N + Q, C = the number of inside pixels (inside: the shifted source lies in the frame).
// register_norm_select_body: the argmax of S / (T - S) over the candidates with C >= min_inside and T - S > 0, by exact 128-bit
//                            cross products, under the plain search's tie rule; the plain search's record, and an extension record.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scene_register_dev.h"

namespace yh {

// what the select kernel leaves beside the SceneRegisterRecord, for yh_scene_motion_norm_read
struct SceneRegisterNormRecord {
    unsigned long long chosen[3];   // S, T, C of the choice
    unsigned long long prior[3];    // S, T, C of (0, 0, 0)
    int qualified, pad;             // 0: no candidate qualified, the choice is the prior
};

// the accumulator (SceneRegisterParams::acc): [0] = sum_n, then the S, T and C tables, each [n_rot][2R+1][2R+1] (v, then u)
__host__ __device__ __forceinline__ size_t register_norm_table_words(int n_rot, int radius) { return (size_t)n_rot * (2 * radius + 1) * (2 * radius + 1); }

// one row of shifts (vi) of a lane's four pixels against the staged window: a += min(N, Q) (MIN) or a += Q. The window holds zeros
// outside the frame, so those Q add nothing. MASKED: the tile hangs over the frame's right or bottom edge - a lane off the frame reads
// cell 0 of the window, a real value, and vm (all ones or zero) takes it out.
template <bool MASKED, bool MIN>
__device__ __forceinline__ void register_norm_row(const uint32_t* win, const int (&off)[SR_PX], const uint32_t (&n)[SR_PX], const uint32_t (&vm)[SR_PX], int at, int nu,
                                                  unsigned long long (&a)[SR_MAX_NU]) {
#pragma unroll
    for (int r = 0; r < SR_PX; ++r) {
        const uint32_t* row = win + off[r] + at;
#pragma unroll
        for (int ui = 0; ui < SR_MAX_NU; ++ui) {
            if (ui < nu) {
                const uint32_t q = MASKED ? (row[ui] & vm[r]) : row[ui];
                a[ui] += MIN ? min(n[r], q) : q;
            }
        }
    }
}

// the wave's sums of one row of shifts into an LDS table (register_wave_sums leaves value u = (lane >> 2) & 15 in lanes u * 4, and
// value 16 everywhere)
__device__ __forceinline__ void register_norm_row_out(unsigned long long (&v)[SR_MAX_NU], int lane, int nu, unsigned long long* part_row) {
    unsigned long long mine, last;
    register_wave_sums(v, lane, mine, last);
    const int u = (lane >> 2) & 15;
    if ((lane & 3) == 0 && u < nu && mine) atomicAdd(&part_row[u], mine);
    if (lane == 0 && nu == SR_MAX_NU && last) atomicAdd(&part_row[SR_MAX_NU - 1], last);
}

// the second pass's sums, two in one 64-bit value: the masked N of a lane's four pixels below bit 44 (a wave's sum is under 2^40),
// their count from bit 44 up (a wave's is at most 256)
#define SRN_COUNT_SHIFT 44
__device__ __forceinline__ void register_norm_row_out_packed(unsigned long long (&v)[SR_MAX_NU], int lane, int nu, unsigned long long* part_n_row, unsigned long long* part_c_row) {
    unsigned long long mine, last;
    register_wave_sums(v, lane, mine, last);
    const unsigned long long low = (1ull << SRN_COUNT_SHIFT) - 1;
    const int u = (lane >> 2) & 15;
    if ((lane & 3) == 0 && u < nu && mine) {
        if (mine & low) atomicAdd(&part_n_row[u], mine & low);
        atomicAdd(&part_c_row[u], mine >> SRN_COUNT_SHIFT);   // (a masked N may be 0, a count under a non-zero sum is not)
    }
    if (lane == 0 && nu == SR_MAX_NU && last) {
        if (last & low) atomicAdd(&part_n_row[SR_MAX_NU - 1], last & low);
        atomicAdd(&part_c_row[SR_MAX_NU - 1], last >> SRN_COUNT_SHIFT);
    }
}

// Geometry, window, fallback, lane-private sums and wave sums are register_scores_body's (scene_register_dev.h). What differs:
//   two sums per shift in the main pass, S and then the sum of Q, 64-bit each, one after the other over the same window row: 17
//   accumulators a lane at a time, as in the plain kernel (both at once cost the fourth workgroup a CU and measured the same);
//   no early exit on an empty tile of N: its Q and its pixels count;
//   the inside predicate. A tile whose dilated window lies wholly in the frame (workgroup-uniform) has every pixel inside under
//   every shift: C and sum of N are the tile's constants, added once per shift at the end. Any other tile runs a second pass
//   over the shifts with no memory reads at all: per pixel the range of u and of v whose source is in the frame, per shift the
//   masked N and the count - packed into one 64-bit sum -, in the registers the first pass has freed.
__device__ __forceinline__ void register_norm_scores_body(const SceneRegisterParams& p, const SceneRegisterBases& bases) {
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
    if (k == 0 && lane == 0 && sum) atomicAdd(p.acc, sum);   // sum_n, once per tile

    const int g0 = bases.g[k][0], g1 = bases.g[k][1], g2 = bases.g[k][2], g3 = bases.g[k][3], g4 = bases.g[k][4], g5 = bases.g[k][5];
    // the tile's sources lie in the box its four corners span (affine, and floor is monotone)
    const int x1 = min(x0 + SR_TW, p.W) - 1, y1 = min(y0 + SR_TH, p.H) - 1;
    const long long ax = affine_q16(g0, g1, g2, x0, y0), bx = affine_q16(g0, g1, g2, x1, y0), cx = affine_q16(g0, g1, g2, x0, y1), dx = affine_q16(g0, g1, g2, x1, y1);
    const long long ay = affine_q16(g3, g4, g5, x0, y0), by = affine_q16(g3, g4, g5, x1, y0), cy = affine_q16(g3, g4, g5, x0, y1), dy = affine_q16(g3, g4, g5, x1, y1);
    const long long wx0 = min(min(ax, bx), min(cx, dx)) - R, wx1 = max(max(ax, bx), max(cx, dx)) + R;
    const long long wy0 = min(min(ay, by), min(cy, dy)) - R, wy1 = max(max(ay, by), max(cy, dy)) + R;
    const long long ww = wx1 - wx0 + 1, wh = wy1 - wy0 + 1;
    const bool in_lds = ww <= SR_LDS_WORDS && wh <= SR_LDS_WORDS && (ww | 1) * wh <= SR_LDS_WORDS;
    const int pitch = in_lds ? (int)(ww | 1) : 0;
    // every source of every shift in the frame: C and the sum of N do not depend on the shift
    const bool all_inside = wx0 >= 0 && wx1 < p.W && wy0 >= 0 && wy1 < p.H;
    const bool full = x0 + SR_TW <= p.W && y0 + SR_TH <= p.H;

    for (int i = tid; i < nu * nu; i += 256) { part_s[i] = 0ull; part_t[i] = 0ull; part_c[i] = 0ull; }
    if (tid == 0) tile_n = 0ull;
    // (the sources are worked out again where the fallback and the second pass need them: eight 64-bit values held across the
    // main pass would cost the fourth workgroup a CU)
    int off[SR_PX];                   // the staged path's: window cell of the source shifted by (-R, -R)
#pragma unroll
    for (int r = 0; r < SR_PX; ++r) {
        const int y = y0 + wave + 4 * r;
        const long long sx = affine_q16(g0, g1, g2, x, y), sy = affine_q16(g3, g4, g5, x, y);
        // (a lane off the frame reads cell 0 and masks what it reads: its source need not lie in the window)
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

    for (int vi = 0; vi < nu; ++vi) {
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
            for (int which = 0; which < 2; ++which) {   // S, then the sum of Q: the second reading comes from the cache
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
        // the shifts whose source lies in the frame, per pixel: ui in [ulo, uhi], vi in [vlo, vhi] (empty: lo > hi), the columns as a
        // mask of 17 bits
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
        for (int vi = 0; vi < nu; ++vi) {
            unsigned long long a[SR_MAX_NU];   // (N and the count in one: register_norm_row_out_packed)
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
    // one 64-bit add per tile, shift and table: integer sums, so the order the tiles arrive in changes nothing
    const size_t words = register_norm_table_words(bases.n_rot, R);
    unsigned long long* tab_s = p.acc + 1 + (size_t)k * nu * nu;
    const unsigned long long add_n = all_inside ? tile_n : 0ull, add_c = all_inside ? (unsigned long long)((x1 - x0 + 1) * (y1 - y0 + 1)) : 0ull;
    for (int i = tid; i < nu * nu; i += 256) {
        const unsigned long long s = part_s[i], t = part_t[i] + add_n, c = part_c[i] + add_c;
        if (s) atomicAdd(tab_s + i, s);
        if (t) atomicAdd(tab_s + words + i, t);
        if (c) atomicAdd(tab_s + 2 * words + i, c);
    }
}

// whether candidate (s, u, d2, i) beats (bs, bu, bd, bi), both qualified (u, bu > 0): the larger s / u - s bu against bs u as exact
// 128-bit products -, then the smaller u^2 + v^2, then the smaller index (the table being [k][v][u]: the smaller k, then v, then u)
__device__ __forceinline__ bool register_norm_better(unsigned long long s, unsigned long long u, int d2, int i, unsigned long long bs, unsigned long long bu, int bd, int bi) {
    const unsigned long long ah = __umul64hi(s, bu), al = s * bu, bh = __umul64hi(bs, u), bl = bs * u;
    if (ah != bh) return ah > bh;
    if (al != bl) return al > bl;
    if (d2 != bd) return d2 < bd;
    return i < bi;
}

// one workgroup of 256 lanes
__device__ __forceinline__ void register_norm_select_body(const unsigned long long* acc, const SceneRegisterBases& bases, int min_inside, SceneRegisterRecord* rec,
                                                          SceneRegisterNormRecord* ext) {
    __shared__ unsigned long long bs[256], bu[256];
    __shared__ int bd[256], bi[256];
    const int tid = threadIdx.x, R = bases.radius, nu = 2 * R + 1, nn = nu * nu, total = bases.n_rot * nn;
    const unsigned long long *tab_s = acc + 1, *tab_t = tab_s + total, *tab_c = tab_t + total;
    unsigned long long s = 0ull, u = 0ull;
    int d2 = 0x7fffffff, best = 0x7fffffff;   // (no qualified candidate seen)
    for (int i = tid; i < total; i += 256) {
        const int r = i % nn, dv = r / nu - R, du = r % nu - R;
        const unsigned long long si = tab_s[i], ui = tab_t[i] - si;
        if (tab_c[i] < (unsigned long long)min_inside || ui == 0ull) continue;
        if (best == 0x7fffffff || register_norm_better(si, ui, du * du + dv * dv, i, s, u, d2, best)) { s = si; u = ui; d2 = du * du + dv * dv; best = i; }
    }
    bs[tid] = s; bu[tid] = u; bd[tid] = d2; bi[tid] = best;
    __syncthreads();
    for (int step = 128; step >= 1; step >>= 1) {
        if (tid < step && bi[tid + step] != 0x7fffffff &&
            (bi[tid] == 0x7fffffff || register_norm_better(bs[tid + step], bu[tid + step], bd[tid + step], bi[tid + step], bs[tid], bu[tid], bd[tid], bi[tid]))) {
            bs[tid] = bs[tid + step]; bu[tid] = bu[tid + step]; bd[tid] = bd[tid + step]; bi[tid] = bi[tid + step];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const int qualified = bi[0] != 0x7fffffff;
    const int prior = R * nu + R;
    const int i = qualified ? bi[0] : prior, k = i / nn, r = i % nn, v = r / nu - R, du = r % nu - R;
    rec->chosen[0] = k; rec->chosen[1] = du; rec->chosen[2] = v; rec->pad = 0;
    rec->score[0] = tab_s[i]; rec->score[1] = tab_s[prior]; rec->score[2] = acc[0];
    ext->chosen[0] = tab_s[i]; ext->chosen[1] = tab_t[i]; ext->chosen[2] = tab_c[i];
    ext->prior[0] = tab_s[prior]; ext->prior[1] = tab_t[prior]; ext->prior[2] = tab_c[prior];
    ext->qualified = qualified; ext->pad = 0;
    // gather and carry of the choice: as register_select_body builds them
    const int* g = bases.g[k];
    const int* c = bases.c[k];
    for (int j = 0; j < 6; ++j) { rec->g[j] = g[j]; rec->c[j] = c[j]; }
    rec->g[2] = (int)((long long)g[2] + (long long)du * 65536);
    rec->g[5] = (int)((long long)g[5] + (long long)v * 65536);
    rec->c[2] = (int)((long long)c[2] - ((long long)c[0] * du + (long long)c[1] * v));
    rec->c[5] = (int)((long long)c[5] - ((long long)c[3] * du + (long long)c[4] * v));
}

}  // namespace yh

struct yh_scene;
namespace yh {
// scene_register_norm.hip, on the handle's stream (its device current). acc_bytes: the accumulator of the largest search (it holds
// the plain search's too). search: acc cleared, the three tables, the choice into rec and ext.
size_t scene_register_norm_acc_bytes();
int scene_register_norm_search(yh_scene* h, const uint32_t* stamp, const uint32_t* mem, const SceneRegisterBases& bases, int min_inside, unsigned long long* acc,
                               SceneRegisterRecord* rec, SceneRegisterNormRecord* ext);
}
