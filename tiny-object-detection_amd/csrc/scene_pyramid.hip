// scene_pyramid.hip — the scene memory's pyramid registration (DESIGN.md section 11 "Scene memory: pyramid registration"): the
// registration of scene_register.hip searched coarse to fine. N and M are max-pooled into levels 1 .. L; every base is scored at
// level L over (2R + 1)^2 shifts, then followed down, (2r + 1)^2 shifts around twice the shift chosen one level up, to level 0, where
// one more hypothesis - base 0 around no shift at all - joins and the choice is made over all of them. The reach is T_0 pixels,
// T_L = R, T_l = 2 T_(l+1) + r, at a cost that barely grows with it. The launches, on the handle's stream, between scene_stamp and
// the fuse:
//   (upload)            the table of level bases, one copy (not when a call is replayed)
//   scene_pyramid       grid (tiles of 64 x 16, 2 maps): levels 1 .. L of N and of M, each formed in registers, written once
//   (clear)             the score tables of every level, one memset
//   per level L .. 0:
//     pyramid_scores    grid (tiles of the level, its hypotheses): register_scores_body, the bases read in place from the table
//     pyramid_select    level > 0: a workgroup per hypothesis - its best shift, the bases of the level below into the table;
//                       level 0: one workgroup - the choice into the SceneRegisterRecord the plain search leaves
//   scene_balls_memory_dev, scene_fuse_dev   (scene_register.hip, unchanged)
// 2 L + 6 launches after the stamps' four. yh_scene_append_memory_pyramid itself lives with the memory's state
// (scene_memory.hip); yh_scene_op_pyramid, everything above but the last line on two given maps, is here.
#include <hip/hip_runtime.h>

#include <string>

#include "scene.h"
#include "scene_pyramid_dev.h"
#include "yh_internal.h"

using namespace yh;

namespace {

__global__ __launch_bounds__(256) void scene_pyramid(const ScenePyramidParams p) { pyramid_body(p); }
// (the address of the bases is uniform over the workgroup: the body's reads of the coefficients are scalar loads)
__global__ __launch_bounds__(256) void pyramid_scores(const SceneRegisterParams p, const SceneRegisterBases* __restrict__ bases) { register_scores_body(p, *bases); }
__global__ __launch_bounds__(256) void pyramid_select(const unsigned long long* acc, ScenePyramidTable* t, const int level, SceneRegisterRecord* rec) {
    pyramid_select_body(acc, t, level, rec);
}

long long abs64(long long v) { return v < 0 ? -v : v; }
long long floor_div(long long a, long long b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }

}  // namespace

namespace yh {

size_t scene_pyramid_map_offset(int W, int H, int level) {
    size_t o = 0;
    for (int l = 1; l < level; ++l) o += (size_t)pyramid_dim(W, l) * pyramid_dim(H, l);
    return o;
}
size_t scene_pyramid_map_words(int W, int H) { return scene_pyramid_map_offset(W, H, SP_MAX_LEVELS + 1); }
size_t scene_pyramid_acc_bytes() { return (SP_MAX_LEVELS + 1) * scene_register_acc_bytes(); }

int scene_pyramid_plan_make(yh_scene* h, int32_t n_rot, const int32_t* g, const int32_t* c, int32_t levels, int32_t radius, int32_t refine, ScenePyramidPlan& plan) {
    if (n_rot < 1 || n_rot > SP_MAX_ROT) return h->fail(YH_EINVAL, "n_rot outside 1 .. 15");
    if (levels < 1 || levels > SP_MAX_LEVELS) return h->fail(YH_EINVAL, "levels outside 1 .. 3");
    if (radius < 0 || radius > SR_MAX_R) return h->fail(YH_EINVAL, "radius outside 0 .. 8");
    if (refine < 0 || refine > SR_MAX_R) return h->fail(YH_EINVAL, "refine outside 0 .. 8");
    long long T[SP_MAX_LEVELS + 1];
    T[levels] = radius;
    for (int l = levels - 1; l >= 0; --l) T[l] = 2 * T[l + 1] + refine;
    const long long top = 2147483647LL;
    plan = ScenePyramidPlan();
    plan.n_rot = n_rot; plan.levels = levels; plan.radius = radius; plan.refine = refine;
    ScenePyramidTable& t = plan.table;
    for (int l = 0; l <= levels; ++l) {
        t.lv[l].n_rot = plan.hyp(l); t.lv[l].radius = plan.rho(l);
        const long long s = (1ll << l) - 1, den = 2ll << l;
        for (int k = 0; k < n_rot; ++k) {
            const int32_t* gk = g + 6 * k;
            // the base carried to the centres of the level's cells
            const long long cl = floor_div(((long long)gk[0] + gk[1] - 65536) * s + 2ll * gk[2], den);
            const long long fl = floor_div(((long long)gk[3] + gk[4] - 65536) * s + 2ll * gk[5], den);
            if (abs64(cl) + T[l] * 65536 > top || abs64(fl) + T[l] * 65536 > top)
                return h->fail(YH_EINVAL, "base " + std::to_string(k) + ": a shifted gather offset leaves int32 at level " + std::to_string(l));
            int* q = t.lv[l].g[k];
            q[0] = gk[0]; q[1] = gk[1]; q[2] = (int)cl; q[3] = gk[3]; q[4] = gk[4]; q[5] = (int)fl;
            t.home[l][k][0] = (int)cl; t.home[l][k][1] = (int)fl;
        }
    }
    for (int k = 0; k < n_rot && c; ++k) {
        const int32_t* ck = c + 6 * k;
        if (abs64(ck[2]) + T[0] * (abs64(ck[0]) + abs64(ck[1])) > top || abs64(ck[5]) + T[0] * (abs64(ck[3]) + abs64(ck[4])) > top)
            return h->fail(YH_EINVAL, "base " + std::to_string(k) + ": a shifted carry offset leaves int32");
        for (int i = 0; i < 6; ++i) t.lv[0].c[k][i] = ck[i];
    }
    // the home hypothesis: base 0 around no shift, scored at level 0 only
    for (int i = 0; i < 6; ++i) { t.lv[0].g[n_rot][i] = t.lv[0].g[0][i]; t.lv[0].c[n_rot][i] = t.lv[0].c[0][i]; }
    t.home[0][n_rot][0] = t.home[0][0][0]; t.home[0][n_rot][1] = t.home[0][0][1];
    return YH_OK;
}

int scene_pyramid_reserve(yh_scene* h, ScenePyramidBufs& b) {
    if (!b.maps) SCHK(h, hipMalloc((void**)&b.maps, 2 * scene_pyramid_map_words(h->W, h->H) * 4));
    if (!b.acc) SCHK(h, hipMalloc((void**)&b.acc, scene_pyramid_acc_bytes()));
    if (!b.table) SCHK(h, hipMalloc((void**)&b.table, sizeof(ScenePyramidTable)));
    return YH_OK;
}

void scene_pyramid_release(ScenePyramidBufs& b) {
    for (void* p : { (void*)b.maps, (void*)b.acc, (void*)b.table }) if (p) hipFree(p);
    b = ScenePyramidBufs();
}

int scene_pyramid_search(yh_scene* h, const uint32_t* stamp, const uint32_t* mem, const ScenePyramidPlan& plan, const ScenePyramidBufs& b, SceneRegisterRecord* rec, bool upload) {
    const int W = h->W, H = h->H, L = plan.levels;
    if (upload) SCHK(h, hipMemcpyAsync(b.table, &plan.table, sizeof(ScenePyramidTable), hipMemcpyHostToDevice, h->stream));
    const size_t words = scene_pyramid_map_words(W, H);
    ScenePyramidParams pp = {};
    pp.src[0] = stamp; pp.src[1] = mem; pp.W = W; pp.H = H; pp.levels = L;
    for (int l = 1; l <= L; ++l) {
        pp.dst[0][l - 1] = b.maps + scene_pyramid_map_offset(W, H, l);
        pp.dst[1][l - 1] = b.maps + words + scene_pyramid_map_offset(W, H, l);
    }
    const unsigned tiles0 = (unsigned)(((W + SP_TW - 1) / SP_TW) * ((H + SP_TH - 1) / SP_TH));   // <= 128 * 512
    hipLaunchKernelGGL(scene_pyramid, dim3(tiles0, 2), dim3(256), 0, h->stream, pp);
    SCHK(h, hipMemsetAsync(b.acc, 0, plan.acc_offset(L + 1) * sizeof(unsigned long long), h->stream));
    for (int l = L; l >= 0; --l) {
        SceneRegisterParams p;
        p.stamp = l ? pp.dst[0][l - 1] : stamp; p.mem = l ? pp.dst[1][l - 1] : mem;
        p.acc = b.acc + plan.acc_offset(l); p.W = pyramid_dim(W, l); p.H = pyramid_dim(H, l);
        const unsigned tiles = (unsigned)(((p.W + SR_TW - 1) / SR_TW) * ((p.H + SR_TH - 1) / SR_TH));
        hipLaunchKernelGGL(pyramid_scores, dim3(tiles, (unsigned)plan.hyp(l)), dim3(256), 0, h->stream, p, (const SceneRegisterBases*)&b.table->lv[l]);
        hipLaunchKernelGGL(pyramid_select, dim3(l ? (unsigned)plan.n_rot : 1u), dim3(256), 0, h->stream, (const unsigned long long*)p.acc, b.table, l, rec);
    }
    SCHK(h, hipGetLastError());
    return YH_OK;
}

// the scene_pyramid launch alone, for a search that scores the levels with kernels of its own (scene_pyramid_norm.hip): where the
// levels lie comes back in pp
void scene_pyramid_levels(yh_scene* h, const uint32_t* stamp, const uint32_t* mem, int levels, const ScenePyramidBufs& b, ScenePyramidParams& pp) {
    const int W = h->W, H = h->H;
    const size_t words = scene_pyramid_map_words(W, H);
    pp = ScenePyramidParams();
    pp.src[0] = stamp; pp.src[1] = mem; pp.W = W; pp.H = H; pp.levels = levels;
    for (int l = 1; l <= levels; ++l) {
        pp.dst[0][l - 1] = b.maps + scene_pyramid_map_offset(W, H, l);
        pp.dst[1][l - 1] = b.maps + words + scene_pyramid_map_offset(W, H, l);
    }
    const unsigned tiles0 = (unsigned)(((W + SP_TW - 1) / SP_TW) * ((H + SP_TH - 1) / SP_TH));   // <= 128 * 512
    hipLaunchKernelGGL(scene_pyramid, dim3(tiles0, 2), dim3(256), 0, h->stream, pp);
}

}  // namespace yh

extern "C" {

int yh_scene_op_pyramid(yh_scene* h, const uint32_t* n_host, const uint32_t* m_host, int32_t n_rot, const int32_t* gather_q16, int32_t levels, int32_t radius,
                        int32_t refine, int32_t* chosen, uint64_t* score, uint32_t* pyr_n, uint32_t* pyr_m, int32_t* centres, uint64_t* scores) {
    if (!h || !n_host || !m_host || !gather_q16) return YH_EINVAL;
    ScenePyramidPlan plan;
    int rc = scene_pyramid_plan_make(h, n_rot, gather_q16, nullptr, levels, radius, refine, plan);
    if (rc) return rc;
    SCHK(h, hipSetDevice(h->dev));
    // maps, levels, tables and record of its own: nothing of the handle's frame or memory is read or written
    const size_t npx = (size_t)h->W * h->H, lw = scene_pyramid_map_offset(h->W, h->H, levels + 1);
    uint32_t* maps = nullptr;
    SceneRegisterRecord* rec = nullptr;
    ScenePyramidBufs b;
    SceneRegisterRecord out = {};
    ScenePyramidTable table = {};
    hipError_t e = hipMalloc((void**)&maps, 2 * npx * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&rec, sizeof(SceneRegisterRecord));
    if (e == hipSuccess && (rc = scene_pyramid_reserve(h, b))) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMemcpyAsync(maps, n_host, npx * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(maps + npx, m_host, npx * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) rc = scene_pyramid_search(h, maps, maps + npx, plan, b, rec, true);
    if (e == hipSuccess && rc == YH_OK) {
        e = hipMemcpyAsync(&out, rec, sizeof(out), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && pyr_n) e = hipMemcpyAsync(pyr_n, b.maps, lw * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && pyr_m) e = hipMemcpyAsync(pyr_m, b.maps + scene_pyramid_map_words(h->W, h->H), lw * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && centres) e = hipMemcpyAsync(&table, b.table, sizeof(table), hipMemcpyDeviceToHost, h->stream);
        for (int l = 0; l <= levels && scores && e == hipSuccess; ++l)   // (level 0 first, each without its sum_n)
            e = hipMemcpyAsync(scores + plan.acc_offset(l) - l, b.acc + plan.acc_offset(l) + 1, (plan.acc_offset(l + 1) - plan.acc_offset(l) - 1) * 8, hipMemcpyDeviceToHost, h->stream);
    }
    const hipError_t es = hipStreamSynchronize(h->stream);   // (also before the buffers go, whatever failed)
    if (e == hipSuccess) e = es;
    for (void* p : { (void*)maps, (void*)rec }) if (p) hipFree(p);
    scene_pyramid_release(b);
    if (rc) return rc;
    if (e != hipSuccess) return h->fail(YH_EHIP, std::string("yh_scene_op_pyramid: ") + hipGetErrorString(e));
    for (int i = 0; i < 3; ++i) { if (chosen) chosen[i] = out.chosen[i]; if (score) score[i] = out.score[i]; }
    if (centres)
        for (int l = 0; l <= levels; ++l)
            for (int k = 0; k < plan.hyp(l); ++k, centres += 2) { centres[0] = table.centre[l][k][0]; centres[1] = table.centre[l][k][1]; }
    return YH_OK;
}

}  // extern "C"
