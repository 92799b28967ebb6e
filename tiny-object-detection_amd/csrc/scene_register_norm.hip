// scene_register_norm.hip — the scene memory's normalised registration (DESIGN.md section 11 "Scene memory: normalised
// registration"): the plain search (scene_register.hip) with the candidates ranked by S / U, U = T - S, over the pixels both maps
// cover, among the candidates that keep at least min_inside pixels inside. The launches between scene_stamp and the fuse:
//   (clear)                        sum_n and the S, T and C tables, one memset
//   scene_register_norm_scores     grid (tiles of 64 x 16, n_rot): S, T and C of every shift of one base, one tile
//   scene_register_norm_select     one workgroup: argmax of the ratio under the tie rule, the record and its extension
//   scene_balls_memory_dev, scene_fuse_dev   scene_register.hip's, unchanged: they read the record
// yh_scene_append_memory_search_norm itself lives with the memory's state (scene_memory.hip); yh_scene_op_register_norm, the two
// kernels alone on two given maps, is here.
#include <hip/hip_runtime.h>

#include <string>

#include "scene.h"
#include "scene_register_norm_dev.h"
#include "yh_internal.h"

using namespace yh;

namespace {

__global__ __launch_bounds__(256, 4) void scene_register_norm_scores(const SceneRegisterParams p, const SceneRegisterBases bases) { register_norm_scores_body(p, bases); }
__global__ __launch_bounds__(256) void scene_register_norm_select(const unsigned long long* acc, const SceneRegisterBases bases, int min_inside, SceneRegisterRecord* rec,
                                                                  SceneRegisterNormRecord* ext) {
    register_norm_select_body(acc, bases, min_inside, rec, ext);
}

}  // namespace

namespace yh {

size_t scene_register_norm_acc_bytes() { return (1 + 3 * register_norm_table_words(SR_MAX_ROT, SR_MAX_R)) * sizeof(unsigned long long); }

int scene_register_norm_search(yh_scene* h, const uint32_t* stamp, const uint32_t* mem, const SceneRegisterBases& bases, int min_inside, unsigned long long* acc,
                               SceneRegisterRecord* rec, SceneRegisterNormRecord* ext) {
    SCHK(h, hipMemsetAsync(acc, 0, (1 + 3 * register_norm_table_words(bases.n_rot, bases.radius)) * sizeof(unsigned long long), h->stream));
    SceneRegisterParams p;
    p.stamp = stamp; p.mem = mem; p.acc = acc; p.W = h->W; p.H = h->H;
    const unsigned tiles = (unsigned)(((h->W + SR_TW - 1) / SR_TW) * ((h->H + SR_TH - 1) / SR_TH));   // <= 128 * 512
    hipLaunchKernelGGL(scene_register_norm_scores, dim3(tiles, (unsigned)bases.n_rot), dim3(256), 0, h->stream, p, bases);
    hipLaunchKernelGGL(scene_register_norm_select, dim3(1), dim3(256), 0, h->stream, (const unsigned long long*)acc, bases, min_inside, rec, ext);
    SCHK(h, hipGetLastError());
    return YH_OK;
}

}  // namespace yh

extern "C" {

int yh_scene_op_register_norm(yh_scene* h, const uint32_t* n_host, const uint32_t* m_host, int32_t n_rot, const int32_t* gather_q16, int32_t radius, int32_t min_inside,
                              uint64_t* scores, uint64_t* totals, uint64_t* inside, int32_t* chosen, int32_t* qualified, uint64_t* sum_n) {
    if (!h || !n_host || !m_host || !gather_q16) return YH_EINVAL;
    int rc = scene_register_bases_check(h, n_rot, gather_q16, nullptr, radius);
    if (rc) return rc;
    const size_t npx = (size_t)h->W * h->H;
    if (min_inside < 1 || (size_t)min_inside > npx) return h->fail(YH_EINVAL, "min_inside outside 1 .. width x height");
    SCHK(h, hipSetDevice(h->dev));
    SceneRegisterBases bases = {};
    bases.n_rot = n_rot; bases.radius = radius;
    for (int k = 0; k < n_rot; ++k)
        for (int i = 0; i < 6; ++i) bases.g[k][i] = gather_q16[6 * k + i];
    // maps, tables and records of its own: nothing of the handle's frame or memory is read or written
    const size_t nsc = register_norm_table_words(n_rot, radius);
    uint32_t* maps = nullptr;
    unsigned long long* acc = nullptr;
    SceneRegisterRecord* rec = nullptr;
    SceneRegisterNormRecord* ext = nullptr;
    SceneRegisterRecord out = {};
    SceneRegisterNormRecord out_ext = {};
    hipError_t e = hipMalloc((void**)&maps, 2 * npx * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&acc, scene_register_norm_acc_bytes());
    if (e == hipSuccess) e = hipMalloc((void**)&rec, sizeof(SceneRegisterRecord));
    if (e == hipSuccess) e = hipMalloc((void**)&ext, sizeof(SceneRegisterNormRecord));
    if (e == hipSuccess) e = hipMemcpyAsync(maps, n_host, npx * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(maps + npx, m_host, npx * 4, hipMemcpyHostToDevice, h->stream);
    rc = YH_OK;
    if (e == hipSuccess) rc = scene_register_norm_search(h, maps, maps + npx, bases, min_inside, acc, rec, ext);
    if (e == hipSuccess && rc == YH_OK) {
        e = hipMemcpyAsync(&out, rec, sizeof(out), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&out_ext, ext, sizeof(out_ext), hipMemcpyDeviceToHost, h->stream);
        uint64_t* const tabs[3] = { scores, totals, inside };
        for (int t = 0; t < 3; ++t)
            if (e == hipSuccess && tabs[t]) e = hipMemcpyAsync(tabs[t], acc + 1 + t * nsc, nsc * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream);
    }
    const hipError_t es = hipStreamSynchronize(h->stream);   // (also before the buffers go, whatever failed)
    if (e == hipSuccess) e = es;
    for (void* b : { (void*)maps, (void*)acc, (void*)rec, (void*)ext }) if (b) hipFree(b);
    if (rc) return rc;
    if (e != hipSuccess) return h->fail(YH_EHIP, std::string("yh_scene_op_register_norm: ") + hipGetErrorString(e));
    if (chosen) for (int i = 0; i < 3; ++i) chosen[i] = out.chosen[i];
    if (qualified) *qualified = out_ext.qualified;
    if (sum_n) *sum_n = out.score[2];
    return YH_OK;
}

}  // extern "C"
