// scene_pyramid_norm.hip — the scene memory's normalised pyramid registration (DESIGN.md section 11 "Scene memory: normalised
// pyramid registration"): the pyramid registration (scene_pyramid.hip) with every level, and the choice, decided by S / U, U = T - S,
// among the entries that keep at least m_l cells inside (scene_register_norm.hip's score). Levels, level bases, hypotheses, reach and
// int32 conditions are the plain pyramid's: its plan, its table and its pooled levels are used as they are. The launches, on the
// handle's stream, between scene_stamp and the fuse:
//   (upload)              the table of level bases, one copy (not when a call is replayed)
//   scene_pyramid         scene_pyramid.hip's, unchanged: levels 1 .. L of N and of M
//   (clear)               the level tables of every level, one memset
//   per level L .. 0:
//     pyramid_norm_scores grid (tiles of the level, its hypotheses): register_norm_scores_body, the bases read in place from the table;
//                         at level L pyramid_norm_scores_rows, grid (tiles, hypotheses, 2 R + 1): a row of shifts a workgroup
//     pyramid_norm_select level > 0: a workgroup per hypothesis - its best qualified shift, the bases of the level below into the table;
//                         level 0: one workgroup - the choice into the two records the flat normalised search leaves
//   scene_balls_memory_dev, scene_fuse_dev   (scene_register.hip, unchanged)
// 2 L + 6 launches after the stamps' four, as the plain pyramid. yh_scene_append_memory_pyramid_norm itself lives with the memory's
// state (scene_memory.hip); yh_scene_op_pyramid_norm, everything above but the last line on two given maps, is here.
#include <hip/hip_runtime.h>

#include <string>

#include "scene.h"
#include "scene_pyramid_norm_dev.h"
#include "yh_internal.h"

using namespace yh;

namespace {

// (the address of the bases is uniform over the workgroup: the body's reads of the coefficients are scalar loads)
__global__ __launch_bounds__(256, 4) void pyramid_norm_scores(const SceneRegisterParams p, const SceneRegisterBases* __restrict__ bases) {
    register_norm_scores_body(p, *bases);
}
// the coarsest level: row blockIdx.z of the shifts alone
__global__ __launch_bounds__(256, 4) void pyramid_norm_scores_rows(const SceneRegisterParams p, const SceneRegisterBases* __restrict__ bases) {
    pyramid_norm_scores_rows_body(p, *bases, (int)blockIdx.z, (int)blockIdx.z + 1);
}
__global__ __launch_bounds__(256) void pyramid_norm_select(const unsigned long long* acc, ScenePyramidTable* t, const int level, const int min_inside, SceneRegisterRecord* rec,
                                                           SceneRegisterNormRecord* nrec, ScenePyramidNormExt* ext) {
    pyramid_norm_select_body(acc, t, level, min_inside, rec, nrec, ext);
}

}  // namespace

namespace yh {

size_t scene_pyramid_norm_acc_bytes() { return (SP_MAX_LEVELS + 1) * scene_register_norm_acc_bytes(); }

int scene_pyramid_norm_reserve(yh_scene* h, ScenePyramidNormBufs& nb) {
    if (!nb.acc) SCHK(h, hipMalloc((void**)&nb.acc, scene_pyramid_norm_acc_bytes()));
    if (!nb.ext) SCHK(h, hipMalloc((void**)&nb.ext, sizeof(ScenePyramidNormExt)));
    return YH_OK;
}

void scene_pyramid_norm_release(ScenePyramidNormBufs& nb) {
    for (void* p : { (void*)nb.acc, (void*)nb.ext }) if (p) hipFree(p);
    nb = ScenePyramidNormBufs();
}

int scene_pyramid_norm_search(yh_scene* h, const uint32_t* stamp, const uint32_t* mem, const ScenePyramidPlan& plan, int min_inside, const ScenePyramidBufs& b,
                              const ScenePyramidNormBufs& nb, SceneRegisterRecord* rec, SceneRegisterNormRecord* nrec, bool upload) {
    const int W = h->W, H = h->H, L = plan.levels;
    if (upload) SCHK(h, hipMemcpyAsync(b.table, &plan.table, sizeof(ScenePyramidTable), hipMemcpyHostToDevice, h->stream));
    ScenePyramidParams pp;
    scene_pyramid_levels(h, stamp, mem, L, b, pp);
    SCHK(h, hipMemsetAsync(nb.acc, 0, pyramid_norm_acc_offset(plan, L + 1) * sizeof(unsigned long long), h->stream));
    for (int l = L; l >= 0; --l) {
        SceneRegisterParams p;
        p.stamp = l ? pp.dst[0][l - 1] : stamp; p.mem = l ? pp.dst[1][l - 1] : mem;
        p.acc = nb.acc + pyramid_norm_acc_offset(plan, l); p.W = pyramid_dim(W, l); p.H = pyramid_dim(H, l);
        const unsigned tiles = (unsigned)(((p.W + SR_TW - 1) / SR_TW) * ((p.H + SR_TH - 1) / SR_TH));
        // (the coarsest level has the fewest tiles and the most shifts: a workgroup per row of them)
        if (l == L) hipLaunchKernelGGL(pyramid_norm_scores_rows, dim3(tiles, (unsigned)plan.hyp(l), (unsigned)(2 * plan.rho(l) + 1)), dim3(256), 0, h->stream, p, (const SceneRegisterBases*)&b.table->lv[l]);
        else hipLaunchKernelGGL(pyramid_norm_scores, dim3(tiles, (unsigned)plan.hyp(l)), dim3(256), 0, h->stream, p, (const SceneRegisterBases*)&b.table->lv[l]);
        hipLaunchKernelGGL(pyramid_norm_select, dim3(l ? (unsigned)plan.n_rot : 1u), dim3(256), 0, h->stream, (const unsigned long long*)p.acc, b.table, l, min_inside, rec, nrec,
                           nb.ext);
    }
    SCHK(h, hipGetLastError());
    return YH_OK;
}

}  // namespace yh

extern "C" {

int yh_scene_op_pyramid_norm(yh_scene* h, const uint32_t* n_host, const uint32_t* m_host, int32_t n_rot, const int32_t* gather_q16, int32_t levels, int32_t radius,
                             int32_t refine, int32_t* chosen, uint64_t* score, uint32_t* pyr_n, uint32_t* pyr_m, int32_t* centres, uint64_t* scores, int32_t min_inside,
                             uint64_t* totals, uint64_t* inside, int32_t* qualified, uint64_t* chosen_stc) {
    if (!h || !n_host || !m_host || !gather_q16) return YH_EINVAL;
    ScenePyramidPlan plan;
    int rc = scene_pyramid_plan_make(h, n_rot, gather_q16, nullptr, levels, radius, refine, plan);
    if (rc) return rc;
    const size_t npx = (size_t)h->W * h->H;
    if (min_inside < 1 || (size_t)min_inside > npx) return h->fail(YH_EINVAL, "min_inside outside 1 .. width x height");
    SCHK(h, hipSetDevice(h->dev));
    // maps, levels, tables and records of its own: nothing of the handle's frame or memory is read or written
    const size_t lw = scene_pyramid_map_offset(h->W, h->H, levels + 1);
    uint32_t* maps = nullptr;
    SceneRegisterRecord* rec = nullptr;
    SceneRegisterNormRecord* nrec = nullptr;
    ScenePyramidBufs b;
    ScenePyramidNormBufs nb;
    SceneRegisterRecord out = {};
    SceneRegisterNormRecord out_n = {};
    ScenePyramidTable table = {};
    ScenePyramidNormExt ext = {};
    hipError_t e = hipMalloc((void**)&maps, 2 * npx * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&rec, sizeof(SceneRegisterRecord));
    if (e == hipSuccess) e = hipMalloc((void**)&nrec, sizeof(SceneRegisterNormRecord));
    if (e == hipSuccess && ((rc = scene_pyramid_reserve(h, b)) || (rc = scene_pyramid_norm_reserve(h, nb)))) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMemcpyAsync(maps, n_host, npx * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(maps + npx, m_host, npx * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) rc = scene_pyramid_norm_search(h, maps, maps + npx, plan, min_inside, b, nb, rec, nrec, true);
    if (e == hipSuccess && rc == YH_OK) {
        e = hipMemcpyAsync(&out, rec, sizeof(out), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&out_n, nrec, sizeof(out_n), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&ext, nb.ext, sizeof(ext), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && pyr_n) e = hipMemcpyAsync(pyr_n, b.maps, lw * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && pyr_m) e = hipMemcpyAsync(pyr_m, b.maps + scene_pyramid_map_words(h->W, h->H), lw * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && centres) e = hipMemcpyAsync(&table, b.table, sizeof(table), hipMemcpyDeviceToHost, h->stream);
        uint64_t* const tabs[3] = { scores, totals, inside };
        for (int l = 0; l <= levels; ++l) {   // (level 0 first, each table without the level's sum_n)
            const size_t words = register_norm_table_words(plan.hyp(l), plan.rho(l));
            for (int t = 0; t < 3; ++t)
                if (e == hipSuccess && tabs[t])
                    e = hipMemcpyAsync(tabs[t] + plan.acc_offset(l) - l, nb.acc + pyramid_norm_acc_offset(plan, l) + 1 + t * words, words * 8, hipMemcpyDeviceToHost, h->stream);
        }
    }
    const hipError_t es = hipStreamSynchronize(h->stream);   // (also before the buffers go, whatever failed)
    if (e == hipSuccess) e = es;
    for (void* p : { (void*)maps, (void*)rec, (void*)nrec }) if (p) hipFree(p);
    scene_pyramid_release(b);
    scene_pyramid_norm_release(nb);
    if (rc) return rc;
    if (e != hipSuccess) return h->fail(YH_EHIP, std::string("yh_scene_op_pyramid_norm: ") + hipGetErrorString(e));
    for (int i = 0; i < 3; ++i) { if (chosen) chosen[i] = out.chosen[i]; if (score) score[i] = out.score[i]; if (chosen_stc) chosen_stc[i] = out_n.chosen[i]; }
    for (int l = 0; l <= levels; ++l)
        for (int k = 0; k < plan.hyp(l); ++k) {
            if (centres) { centres[0] = table.centre[l][k][0]; centres[1] = table.centre[l][k][1]; centres += 2; }
            if (qualified) *qualified++ = ext.qualified[l][k];
        }
    if (qualified) *qualified = out_n.qualified;   // (after the flags of every level: whether the choice itself qualified)
    return YH_OK;
}

}  // extern "C"
