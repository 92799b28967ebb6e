// scene_dev.h — the scene back-end's device code, shared by scene.hip (one frame per launch, yh_scene) and scene_batch.hip (N frames per
// launch, yh_scene_batch: the frame is blockIdx.z, the kernel advances its own copy of the parameter block and runs the same body).
// What is computed and why is said at the head of scene.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace yh {

#define SC_MAX_DEPTH 4000.0f
#define SC_TAN_HALF_YFOV 0.55430907f
#define SC_TAN_HALF_XFOV 0.9489646f
#define SC_BOT_AVOID 100.0f
#define SC_BOT_NORM 20
#define SC_TERRAIN_NORM 10
#define SC_BUMP_ERR 0.1f

struct SceneParams {
    const uint16_t* depth;        // [H][W]
    const uint8_t* cls_id;        // [H][W][2] (class, id), or nullptr when `frame` is given
    const uint32_t* frame;        // [H][W] packed pixels as classify leaves them
    int frame_mode;               // with `frame`: 0 = low 16 bits as src/scene.rs:93 reads them, 1 = class bits 31-24, id bits 23-16
    int W, H, mode;
    int band_h;                   // map rows per workgroup of scene_cloud_strips (<= SC_BH; chosen so that the grid is one round of the chip)
    uint32_t* map;                // [H][W]
    float4 *world, *conn0, *conn1;
    long long* ball_acc;          // [3][100]: sum x, sum y, count
    float4* balls;                // [100]
    // the bump profiles, tabulated once per handle: a tap's height depends only on (val, dx, dy), and val is the pixel's
    // ROW for terrain (pt_cloud.comp:116) or the constant 100 for robots (:122)
    const uint32_t* terrain_tab;  // [H][ly 20][lx 20]
    const uint32_t* robot_tab;    // [ly 40][lx 40]
};

// pt_cloud.comp main (:84-123) and its bump() (:44-76), privatised. Geometry of one workgroup (512 lanes, 8 waves):
//   strip   pixel columns [c0, c0 + 16): a pixel (x, y) stamps around (nx, ny) = (x, H - dic(depth)), i.e. map columns
//           x - L .. x + L - 1 with L <= 20: the strip's taps land in map columns [c0 - 20, c0 + 36) - the LDS image's 56 columns;
//   band    map rows [r0, r0 + band_h): every workgroup of a strip walks ALL of the strip's pixels (16 x H: cheap) and stamps the taps
//           of each bump that fall into its own band; band_h = 64 (320 workgroups at 640 x 480; a grid of ONE round - 80-row bands - measured slower);
//           the image is 21 KB.
// A wave takes four pixel rows at a time: its 64 lanes compute the 4 x 16 pixels (the shader's arithmetic, one IEEE
// operation per operator), then the wave stamps the bump pixels one at a time (ballot + readlane: wave-uniform target),
// lane t owning taps t, t + 64, ... of the bump. The tap HEIGHTS sit in registers: a terrain tap depends on the pixel's row only
// (pt_cloud.comp:116), so the row's 400-entry table is loaded once per row (7 coalesced loads, only if some pixel of the row hits
// the band) and serves its 16 pixels; the robot table (1 600 entries, a constant) is loaded once per workgroup (25 registers). The
// stamping loop therefore has no memory read: per tap a range test and one ds_max_u32 (row pitch 84 words). A tap of height 0
// changes nothing and is not issued. (First version of this kernel, a wave per pixel with the table read from global memory inside
// the tap loop: 0.56-0.65 ms per frame against 2.0-2.3 for the global-atomic form; it waited for one L2 round trip per 64 taps.)
// Ball pixels add their position to 64-bit sums in LDS (band 0 only: once per pixel), flushed once per workgroup.
#define SC_CW 16
#define SC_BH 96   // most map rows a workgroup's LDS image holds; the launch picks band_h <= SC_BH (yh_scene_create)
#define SC_HALO 20
#define SC_LDW 84   // 56 columns used; 84 = 64 + 20: a wave's 3.2 consecutive tap rows of a terrain bump fall on 64 different banks
#define SC_TT (4 * SC_TERRAIN_NORM * SC_TERRAIN_NORM)   // 400 taps
#define SC_RT (4 * SC_BOT_NORM * SC_BOT_NORM)           // 1600 taps
#define SC_TK ((SC_TT + 63) / 64)                       // 7 taps per lane
#define SC_RK (SC_RT / 64)                              // 25 taps per lane
__device__ __forceinline__ void cloud_strips_body(const SceneParams& p) {
    __shared__ uint32_t img[SC_BH * SC_LDW];
    __shared__ unsigned long long ball[300];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * SC_CW, r0 = blockIdx.y * p.band_h;
    const bool do_balls = blockIdx.y == 0;
    const int ncell = p.band_h * SC_LDW;
    for (int i = tid; i < ncell; i += 512) img[i] = 0u;
    if (do_balls) for (int i = tid; i < 300; i += 512) ball[i] = 0ull;
    uint32_t rt[SC_RK];   // the robot bump, this lane's taps
#pragma unroll
    for (int k = 0; k < SC_RK; ++k) rt[k] = p.robot_tab[lane + 64 * k];
    __syncthreads();
    const int cw = min(SC_CW, p.W - c0);
    const int band_lo = max(r0, 1), band_hi = min(r0 + p.band_h, p.H - 1);   // rows y with 0 < y < H - 1 inside the band
    const int ibase = -r0 * SC_LDW - (c0 - SC_HALO);                       // img[ibase + y * SC_LDW + x] = the cell of map (x, y)
    // FOUR pixel rows per wave and iteration (lane = 16 (row in the group) + column): the depth / class loads of 64 pixels are one
    // latency, not four, and the four rows' terrain tables are requested together before the first stamp (the first version of this loop
    // took one row at a time: 60 exposed round trips per wave on a grid of ~1.25 workgroups per CU)
    const int lr = lane >> 4, lc = lane & 15;
    for (int y4 = 4 * wave; y4 < p.H; y4 += 32) {
        const int y = y4 + lr;
        int nx = 0, ny = 0, L = 0;
        if (lc < cw && y < p.H) {
            const int x = c0 + lc;
            const size_t i = (size_t)y * p.W + x;
            const float ty = __fdiv_rn(__fmul_rn(__fmul_rn(SC_TAN_HALF_YFOV, (float)y), 2.0f), (float)p.H);
            const float tx = __fdiv_rn(__fmul_rn(__fmul_rn(SC_TAN_HALF_XFOV, (float)x), 2.0f), (float)p.W);
            const float cy = __fdiv_rn(1.0f, __builtin_sqrtf(__fadd_rn(1.0f, __fmul_rn(ty, ty))));
            const float cx = __fdiv_rn(1.0f, __builtin_sqrtf(__fadd_rn(1.0f, __fmul_rn(tx, tx))));
            const float d = __fmul_rn(__fmul_rn((float)p.depth[i], cy), cx);
            const int dic = (int)__fdiv_rn(__fmul_rn((float)p.H, d), SC_MAX_DEPTH);
            int cls, id;
            if (p.cls_id) { cls = p.cls_id[2 * i]; id = p.cls_id[2 * i + 1]; }
            else {
                const uint32_t px = p.frame[i];
                if (p.frame_mode == 0) { cls = (int)(px & 0xFFu); id = (int)((px >> 8) & 0xFFu); }   // `as u16` then R8G8 (scene.rs:93, :198)
                else { cls = (int)(px >> 24); id = (int)((px >> 16) & 0xFFu); }
            }
            int action = cls;
            if (action > 1) action = action - 1;
            nx = x; ny = p.H - dic;
            if (action == 0) L = SC_TERRAIN_NORM;
            else if (action == 2) {
                if (do_balls && id < 100) {
                    __hip_atomic_fetch_add(&ball[id], (unsigned long long)(long long)nx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(&ball[100 + id], (unsigned long long)(long long)ny, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(&ball[200 + id], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            } else L = SC_BOT_NORM;
        }
        const bool hit = L > 0 && max(ny - L, band_lo) < min(ny + L, band_hi);   // this lane's bump meets the band
        const unsigned long long hit_t = __ballot(hit && L == SC_TERRAIN_NORM);
        unsigned long long todo_r = __ballot(hit && L == SC_BOT_NORM);
        if (hit_t) {
            uint32_t tt[4][SC_TK];   // the terrain bumps of the four rows, this lane's taps (a row without a hit is not fetched)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if ((hit_t >> (16 * r)) & 0xFFFFull) {
                    const uint32_t* trow = p.terrain_tab + (size_t)(y4 + r) * SC_TT;
#pragma unroll
                    for (int k = 0; k < SC_TK; ++k) tt[r][k] = lane + 64 * k < SC_TT ? trow[lane + 64 * k] : 0u;
                } else {
#pragma unroll
                    for (int k = 0; k < SC_TK; ++k) tt[r][k] = 0u;
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                unsigned long long todo_t = hit_t & (0xFFFFull << (16 * r));
                while (todo_t) {
                    const int j = __ffsll((long long)todo_t) - 1;
                    todo_t &= todo_t - 1;
                    const int x0 = __builtin_amdgcn_readlane(nx, j) - SC_TERRAIN_NORM, y0 = __builtin_amdgcn_readlane(ny, j) - SC_TERRAIN_NORM;
#pragma unroll
                    for (int k = 0; k < SC_TK; ++k) {
                        const int t = lane + 64 * k, ly = t / (2 * SC_TERRAIN_NORM), lx = t - ly * (2 * SC_TERRAIN_NORM);
                        const int yy = y0 + ly, xx = x0 + lx;
                        if (tt[r][k] && yy >= band_lo && yy < band_hi && xx > 0 && xx < p.W - 1)
                            __hip_atomic_fetch_max(&img[ibase + yy * SC_LDW + xx], tt[r][k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
        }
        while (todo_r) {
            const int j = __ffsll((long long)todo_r) - 1;
            todo_r &= todo_r - 1;
            const int x0 = __builtin_amdgcn_readlane(nx, j) - SC_BOT_NORM, y0 = __builtin_amdgcn_readlane(ny, j) - SC_BOT_NORM;
#pragma unroll
            for (int k = 0; k < SC_RK; ++k) {
                const int t = lane + 64 * k, ly = t / (2 * SC_BOT_NORM), lx = t - ly * (2 * SC_BOT_NORM);
                const int yy = y0 + ly, xx = x0 + lx;
                if (rt[k] && yy >= band_lo && yy < band_hi && xx > 0 && xx < p.W - 1)
                    __hip_atomic_fetch_max(&img[ibase + yy * SC_LDW + xx], rt[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < ncell; i += 512) {
        const uint32_t v = img[i];
        if (v) {
            const int row = i / SC_LDW, col = i - row * SC_LDW;
            atomicMax(p.map + (size_t)(r0 + row) * p.W + (c0 - SC_HALO + col), v);
        }
    }
    if (do_balls)
        for (int i = tid; i < 300; i += 512)
            if (ball[i]) atomicAdd((unsigned long long*)p.ball_acc + i, ball[i]);
}

__device__ __forceinline__ void balls_body(const SceneParams& p) {
    const int k = threadIdx.x;
    if (k >= 100) return;
    const long long sx = p.ball_acc[k], sy = p.ball_acc[100 + k], n = p.ball_acc[200 + k];
    p.balls[k] = make_float4(n ? (float)((double)sx / (double)n) : 0.0f, n ? (float)((double)sy / (double)n) : 0.0f, (float)n, 0.0f);
}

// pt_cloud_weights.comp stage 1 (:57-87)
__device__ __forceinline__ void world_body(const SceneParams& p) {
    const int x = blockIdx.x * 8 + threadIdx.x, y = blockIdx.y * 8 + threadIdx.y;
    if (x >= p.W || y >= p.H) return;
    const size_t i = (size_t)y * p.W + x;
    p.world[i] = make_float4((float)x, (float)p.map[i], (float)y, 0.0f);
}

// stage 2 (:91-111): r (x, y+1), g (x-1, y+1), b (x-1, y), a (x-1, y-1)
__device__ __forceinline__ void conn1_body(const SceneParams& p) {
    const int x = blockIdx.x * 8 + threadIdx.x, y = blockIdx.y * 8 + threadIdx.y;
    if (x >= p.W || y >= p.H) return;
    const size_t i = (size_t)y * p.W + x;
    const float4 me = p.world[i];
    const int ox[4] = { 0, -1, -1, -1 }, oy[4] = { 1, 1, 0, -1 };
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qx = x + ox[k], qy = y + oy[k];
        v[k] = -1.0f;
        if (qx >= 0 && qx < p.W && qy >= 0 && qy < p.H) {
            // STRICT: pack(x, y) = float((x << 16) & y) is 0 for every pixel (pt_cloud_weights.comp:32), so unpack()
            // returns world(0, 0) whoever the neighbour is; SANE: the neighbour's own position
            const float4 o = p.world[p.mode == 0 ? 0 : (size_t)qy * p.W + qx];
            const float dx = __fsub_rn(me.x, o.x), dy = __fsub_rn(me.y, o.y), dz = __fsub_rn(me.z, o.z);
            v[k] = __builtin_sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
        }
    }
    p.conn1[i] = make_float4(v[0], v[1], v[2], v[3]);
}

// stage 3 (:115-123): r (x, y-1), g (x+1, y-1), b (x+1, y), a (x+1, y+1)
__device__ __forceinline__ void conn0_body(const SceneParams& p) {
    const int x = blockIdx.x * 8 + threadIdx.x, y = blockIdx.y * 8 + threadIdx.y;
    if (x >= p.W || y >= p.H) return;
    const size_t i = (size_t)y * p.W + x;
    const int ox[4] = { 0, 1, 1, 1 }, oy[4] = { -1, -1, 0, 1 };
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qx = x + ox[k], qy = y + oy[k];
        v[k] = -1.0f;
        if (qx >= 0 && qx < p.W && qy >= 0 && qy < p.H) {
            const float4 o = p.conn1[(size_t)qy * p.W + qx];
            v[k] = k == 0 ? o.x : (k == 1 ? o.y : (k == 2 ? o.z : o.w));
        }
    }
    p.conn0[i] = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace yh
