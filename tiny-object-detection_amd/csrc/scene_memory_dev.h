// scene_memory_dev.h — the scene memory's device code (scene_memory.hip; the definition is DESIGN.md section 11 "Scene memory").
// fuse_body: the previous map moved by the robot's motion, faded, merged with the frame's stamps, and the connection fields of
// the result, in ONE pass over the frame. balls_memory_body: the ball table carried the other way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace yh {

struct SceneFuseParams {
    const uint32_t* stamp;      // N [H][W]: the frame's own bumps (scene_cloud_strips)
    const uint32_t* mem_prev;   // M [H][W]: the memory as the previous memory append left it
    uint32_t* mem_next;         // F, the new memory: never one of the two above (neighbouring workgroups still read those); null: not kept
    uint32_t* map;              // F again: the handle's map
    float4 *world, *conn0, *conn1;
    int W, H;
    int g[6];                   // gather_q16: current-map pixel -> previous-map pixel
    int keep;                   // 0 .. 256
};

struct SceneBallsMemParams {
    const long long* ball_acc;  // [3][100]: the frame's sums (the count says whether an id was seen)
    float4* balls;              // [100]: the frame's own rows (scene_balls), rewritten for ids that are only remembered
    const int4* tab_prev;       // B [100] = (x, y, count, age)
    int4* tab_next;
    int W, H;
    int c[6];                   // carry_q16: previous-map pixel -> current-map pixel
    int max_age;                // 0 .. 255
};

// The batch's device tables (scene_batch_memory.hip): what one grid z of a fuse round, one frame of a stream's ball chain and one
// chain run on. A frame's arrays are the by-value parameter block's advanced by `frame` frames.
struct SceneFuseSlot {
    const uint32_t* mem_prev;   // the stream's bank map (its first frame in the call) or the predecessor's map slot
    uint32_t* mem_next;         // the bank's other map for the stream's last frame in the call, else null
    int frame;
    int g[6];
    int pad;
};
struct SceneBallsStep { int frame; int c[6]; int pad; };
struct SceneBallsChain {
    const int4* tab_prev;       // the stream's bank table
    int4* tab_next;             // the bank's other table: the chain's last table again
    int first, count;           // its steps, in batch order
};

// floor((a x + b y + c + 2^15) / 2^16) in 64 bits: |a x| < 2^31 * 2^20 for every x either body passes, so nothing overflows
__device__ __forceinline__ long long affine_q16(int a, int b, int c, int x, int y) {
    return ((long long)a * x + (long long)b * y + (long long)c + 32768LL) >> 16;
}

// Geometry of one workgroup (256 lanes, 4 waves): a tile of 64 x 8 pixels; wave w owns rows w and w + 4, a lane one column, so
// that a wave's float4 stores of world, conn0 and conn1 are 64 consecutive 16-byte slots (1 KiB per instruction). F of the tile
// and a one-pixel halo sits in LDS: 10 rows x 66 cells, 660 gathers for 512 pixels (a 64 x 4 tile would make 396 for 256).
// The row pitch needs no padding: every LDS access of a wave is 64 consecutive words (b32: conflict-free at any pitch).
#define SF_TW 64
#define SF_TH 8
#define SF_LW (SF_TW + 2)
#define SF_LH (SF_TH + 2)

// one edge length as conn1_body computes it for pixel `me` towards neighbour `o` (SANE): single IEEE operations
__device__ __forceinline__ float fuse_len(float mx, float my, float mz, float ox, float oy, float oz) {
    const float dx = __fsub_rn(mx, ox), dy = __fsub_rn(my, oy), dz = __fsub_rn(mz, oz);
    return __builtin_sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
}

__device__ __forceinline__ void fuse_body(const SceneFuseParams& p) {
    __shared__ uint32_t F[SF_LH * SF_LW];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SF_TW, y0 = blockIdx.y * SF_TH;
    for (int i = tid; i < SF_LH * SF_LW; i += 256) {
        const int cy = i / SF_LW, cx = i - cy * SF_LW;
        const int gx = x0 - 1 + cx, gy = y0 - 1 + cy;
        uint32_t f = 0u;   // (a cell outside the frame is never read as a height: its edges are -1)
        if (gx >= 0 && gx < p.W && gy >= 0 && gy < p.H) {
            f = p.stamp[(size_t)gy * p.W + gx];
            // the source pixel, checked on the 64-bit values before anything is narrowed or used as an address
            const long long sx = affine_q16(p.g[0], p.g[1], p.g[2], gx, gy), sy = affine_q16(p.g[3], p.g[4], p.g[5], gx, gy);
            if (sx >= 0 && sx < p.W && sy >= 0 && sy < p.H) {
                const uint32_t prev = p.mem_prev[(size_t)sy * p.W + (size_t)sx];
                f = max(f, (uint32_t)(((unsigned long long)prev * (unsigned long long)p.keep) >> 8));
            }
        }
        F[i] = f;
    }
    __syncthreads();
    const int lx = tid & 63, x = x0 + lx;
    if (x >= p.W) return;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int ly = (tid >> 6) + 4 * r, y = y0 + ly;
        if (y >= p.H) continue;
        const uint32_t* c = F + (ly + 1) * SF_LW + (lx + 1);   // this pixel's cell
        const uint32_t fm = c[0];
        const float X = (float)x, Y = (float)y, Hm = (float)fm;
        // conn1 (pt_cloud_weights.comp:91-111): this pixel towards (x, y+1), (x-1, y+1), (x-1, y), (x-1, y-1)
        // conn0 (:115-123): the entries the neighbours (x, y-1), (x+1, y-1), (x+1, y), (x+1, y+1) hold for the same edges, i.e. the
        // lengths computed FROM the neighbour towards this pixel (the same bits: only the signs of the differences change)
        const int ox[4] = { 0, -1, -1, -1 }, oy[4] = { 1, 1, 0, -1 };
        float v1[4], v0[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int qx = x + ox[k], qy = y + oy[k];
            v1[k] = -1.0f;
            if (qx >= 0 && qx < p.W && qy >= 0 && qy < p.H)
                v1[k] = fuse_len(X, Hm, Y, (float)qx, (float)c[oy[k] * SF_LW + ox[k]], (float)qy);
            const int nx = x - ox[k], ny = y - oy[k];
            v0[k] = -1.0f;
            if (nx >= 0 && nx < p.W && ny >= 0 && ny < p.H)
                v0[k] = fuse_len((float)nx, (float)c[-oy[k] * SF_LW - ox[k]], (float)ny, X, Hm, Y);
        }
        const size_t i = (size_t)y * p.W + x;
        p.map[i] = fm;
        if (p.mem_next) p.mem_next[i] = fm;   // (uniform: a frame of a batch that is not its stream's last keeps F in its map slot only)
        p.world[i] = make_float4(X, Hm, Y, 0.0f);
        p.conn0[i] = make_float4(v0[0], v0[1], v0[2], v0[3]);
        p.conn1[i] = make_float4(v1[0], v1[1], v1[2], v1[3]);
    }
}

// step 4 of the definition: one lane per ball id
__device__ __forceinline__ void balls_memory_body(const SceneBallsMemParams& p) {
    const int k = threadIdx.x;
    if (k >= 100) return;
    const long long n = p.ball_acc[200 + k];
    int4 b = make_int4(0, 0, 0, 0);
    if (n > 0) {   // seen: the frame's own row stays
        const float4 row = p.balls[k];
        b = make_int4((int)row.x, (int)row.y, (int)n, 0);
    } else {
        const int4 old = p.tab_prev[k];
        float4 row = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (old.z > 0 && old.w + 1 <= p.max_age) {
            const long long cx = affine_q16(p.c[0], p.c[1], p.c[2], old.x, old.y), cy = affine_q16(p.c[3], p.c[4], p.c[5], old.x, old.y);
            const long long lim = 1LL << 20;
            if (cx > -lim && cx < lim && cy > -lim && cy < lim) {
                b = make_int4((int)cx, (int)cy, old.z, old.w + 1);
                if (cx >= 0 && cx < p.W && cy >= 0 && cy < p.H) row = make_float4((float)(int)cx, (float)(int)cy, (float)old.z, (float)old.w);
            }
        }
        p.balls[k] = row;
    }
    p.tab_next[k] = b;
}

}  // namespace yh
