// scene_register.hip — the scene memory's registration (DESIGN.md section 11 "Scene memory: registration"): where the robot's motion
// is not known, or only roughly, the frame's stamps N are scored against the memory M over n_rot base motions x (2R + 1)^2 whole-
// pixel shifts, the best candidate is chosen on the device, and the fuse and the ball carry read their motion from the record it
// leaves - no host wait in between. The launches, on the handle's stream, between scene_stamp and the fuse:
//   (clear)                   sum_n and the score table, one memset
//   scene_register_scores     grid (tiles of 64 x 16, n_rot): the tile's window of M in LDS, every shift read from there
//   scene_register_select     one workgroup: argmax under the tie rule, the chosen twelve coefficients
//   scene_balls_memory_dev, scene_fuse_dev   balls_memory_body / fuse_body of scene_memory_dev.h with c / g taken from the record
// yh_scene_append_memory_search itself lives with the memory's state (scene_memory.hip); yh_scene_op_register, the first two
// kernels alone on two given maps, is here.
#include <hip/hip_runtime.h>

#include <string>

#include "scene.h"
#include "scene_register_dev.h"
#include "yh_internal.h"

using namespace yh;

namespace {

__global__ __launch_bounds__(256) void scene_register_scores(const SceneRegisterParams p, const SceneRegisterBases bases) { register_scores_body(p, bases); }
__global__ __launch_bounds__(256) void scene_register_select(const unsigned long long* acc, const SceneRegisterBases bases, SceneRegisterRecord* rec) {
    register_select_body(acc, bases, rec);
}
// the existing bodies, unchanged, on the by-value block with the motion overwritten from the device record
__global__ __launch_bounds__(256) void scene_fuse_dev(SceneFuseParams p, const SceneRegisterRecord* rec) {
#pragma unroll
    for (int i = 0; i < 6; ++i) p.g[i] = rec->g[i];
    fuse_body(p);
}
__global__ __launch_bounds__(128) void scene_balls_memory_dev(SceneBallsMemParams p, const SceneRegisterRecord* rec) {
#pragma unroll
    for (int i = 0; i < 6; ++i) p.c[i] = rec->c[i];
    balls_memory_body(p);
}

long long abs64(long long v) { return v < 0 ? -v : v; }

}  // namespace

namespace yh {

size_t scene_register_acc_bytes() { return (1 + (size_t)SR_MAX_ROT * SR_MAX_NU * SR_MAX_NU) * sizeof(unsigned long long); }

int scene_register_bases_check(yh_scene* h, int32_t n_rot, const int32_t* g, const int32_t* c, int32_t radius) {
    if (n_rot < 1 || n_rot > SR_MAX_ROT) return h->fail(YH_EINVAL, "n_rot outside 1 .. 16");
    if (radius < 0 || radius > SR_MAX_R) return h->fail(YH_EINVAL, "radius outside 0 .. 8");
    const long long R = radius, top = 2147483647LL;
    for (int k = 0; k < n_rot; ++k) {
        const int32_t* gk = g + 6 * k;
        if (abs64(gk[2]) + R * 65536 > top || abs64(gk[5]) + R * 65536 > top)
            return h->fail(YH_EINVAL, "base " + std::to_string(k) + ": a shifted gather offset leaves int32");
        if (!c) continue;
        const int32_t* ck = c + 6 * k;
        if (abs64(ck[2]) + R * (abs64(ck[0]) + abs64(ck[1])) > top || abs64(ck[5]) + R * (abs64(ck[3]) + abs64(ck[4])) > top)
            return h->fail(YH_EINVAL, "base " + std::to_string(k) + ": a shifted carry offset leaves int32");
    }
    return YH_OK;
}

int scene_register_search(yh_scene* h, const uint32_t* stamp, const uint32_t* mem, const SceneRegisterBases& bases, unsigned long long* acc, SceneRegisterRecord* rec) {
    const int nu = 2 * bases.radius + 1;
    SCHK(h, hipMemsetAsync(acc, 0, (1 + (size_t)bases.n_rot * nu * nu) * sizeof(unsigned long long), h->stream));
    SceneRegisterParams p;
    p.stamp = stamp; p.mem = mem; p.acc = acc; p.W = h->W; p.H = h->H;
    const unsigned tiles = (unsigned)(((h->W + SR_TW - 1) / SR_TW) * ((h->H + SR_TH - 1) / SR_TH));   // <= 128 * 512
    hipLaunchKernelGGL(scene_register_scores, dim3(tiles, (unsigned)bases.n_rot), dim3(256), 0, h->stream, p, bases);
    hipLaunchKernelGGL(scene_register_select, dim3(1), dim3(256), 0, h->stream, (const unsigned long long*)acc, bases, rec);
    SCHK(h, hipGetLastError());
    return YH_OK;
}

int scene_register_fuse(yh_scene* h, const SceneFuseParams& f, const SceneBallsMemParams& b, const SceneRegisterRecord* rec) {
    hipLaunchKernelGGL(scene_balls_memory_dev, dim3(1), dim3(128), 0, h->stream, b, rec);
    hipLaunchKernelGGL(scene_fuse_dev, dim3((unsigned)((h->W + SF_TW - 1) / SF_TW), (unsigned)((h->H + SF_TH - 1) / SF_TH)), dim3(256), 0, h->stream, f, rec);
    SCHK(h, hipGetLastError());
    return YH_OK;
}

}  // namespace yh

extern "C" {

int yh_scene_op_register(yh_scene* h, const uint32_t* n_host, const uint32_t* m_host, int32_t n_rot, const int32_t* gather_q16, int32_t radius,
                         uint64_t* scores, int32_t* chosen, uint64_t* sum_n) {
    if (!h || !n_host || !m_host || !gather_q16) return YH_EINVAL;
    int rc = scene_register_bases_check(h, n_rot, gather_q16, nullptr, radius);
    if (rc) return rc;
    SCHK(h, hipSetDevice(h->dev));
    SceneRegisterBases bases = {};
    bases.n_rot = n_rot; bases.radius = radius;
    for (int k = 0; k < n_rot; ++k)
        for (int i = 0; i < 6; ++i) bases.g[k][i] = gather_q16[6 * k + i];
    // maps, table and record of its own: nothing of the handle's frame or memory is read or written
    const size_t npx = (size_t)h->W * h->H, nsc = (size_t)n_rot * (2 * radius + 1) * (2 * radius + 1);
    uint32_t* maps = nullptr;
    unsigned long long* acc = nullptr;
    SceneRegisterRecord* rec = nullptr;
    SceneRegisterRecord out = {};
    hipError_t e = hipMalloc((void**)&maps, 2 * npx * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&acc, scene_register_acc_bytes());
    if (e == hipSuccess) e = hipMalloc((void**)&rec, sizeof(SceneRegisterRecord));
    if (e == hipSuccess) e = hipMemcpyAsync(maps, n_host, npx * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(maps + npx, m_host, npx * 4, hipMemcpyHostToDevice, h->stream);
    rc = YH_OK;
    if (e == hipSuccess) rc = scene_register_search(h, maps, maps + npx, bases, acc, rec);
    if (e == hipSuccess && rc == YH_OK) {
        e = hipMemcpyAsync(&out, rec, sizeof(out), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && scores) e = hipMemcpyAsync(scores, acc + 1, nsc * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream);
    }
    const hipError_t es = hipStreamSynchronize(h->stream);   // (also before the buffers go, whatever failed)
    if (e == hipSuccess) e = es;
    for (void* b : { (void*)maps, (void*)acc, (void*)rec }) if (b) hipFree(b);
    if (rc) return rc;
    if (e != hipSuccess) return h->fail(YH_EHIP, std::string("yh_scene_op_register: ") + hipGetErrorString(e));
    if (chosen) for (int i = 0; i < 3; ++i) chosen[i] = out.chosen[i];
    if (sum_n) *sum_n = out.score[2];
    return YH_OK;
}

}  // extern "C"
