// scene.hip — the reference's scene back-end on the GPU: height map with sigmoid "bumps" and
// ball centroids (/root/reference/shaders/pt_cloud.comp), world positions and 8-neighbour edge lengths
// (/root/reference/shaders/pt_cloud_weights.comp), driven as /root/reference/src/scene.rs:147-331 (append_scene)
// drives its two Vulkan dispatches of [80,60,1] x 8x8 over a 640x480 frame (scene.rs:245,:256).
//
// What is computed is the deterministic reading frozen in DESIGN.md §Scene and restated in oracle/orc_scene.c (the
// shaders as written race - store_ball, barrier() used as a grid barrier - and call pow() where GLSL leaves it
// undefined): every stage completes over the whole frame before the next starts (one launch per stage); texel (x, y)
// is read for pixel (x, y); squares are products; a bump whose sigmoid base is not positive adds nothing; ball
// centroids are exact integer means. Integer outputs and every float are bit-identical to the oracle: one IEEE
// operation per operator (-ffp-contract=off; sqrtf and / are correctly rounded in HIP by default, unlike __fsqrt_rn,
// which maps to the native approximate instruction).
// Atomic-bound byte work. The height map is a max over ~150 M bump taps per 640 x 480 frame; the shader (and rounds 2-4 here)
// gives every pixel a lane that walks its 400 / 1 600 taps through imageAtomicMax in global memory (2.0-2.3 ms per frame). Round 5
// (scene_cloud_strips): the map is PRIVATISED in LDS - a workgroup owns a strip of 16 pixel columns x a band of 64 map rows, stamps
// every tap that lands there with ds_max_u32 (a wave per pixel, a lane per tap: uniform tap counts, coalesced table reads,
// consecutive lanes on consecutive LDS words) and merges its image into the global map with one atomicMax per touched cell. A max
// is order-free, so the result is the shader's imageAtomicMax result bit for bit. The other stages keep one lane per pixel in
// 8x8 workgroups, the dispatch the reference uses (scene.rs:245,:256).
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>

#include "scene.h"
#include "scene_dev.h"
#include "yh_internal.h"

using namespace yh;

namespace {

// height of one bump tap (pt_cloud.comp:55-73): val / (1 + C_1^(C_2 prox - 1)), truncated; 0 where the shader's pow() is undefined
__device__ __forceinline__ uint32_t bump_tap(float val, int L, int lx, int ly) {
    const float C1 = __fsub_rn(__fdiv_rn(val, SC_BUMP_ERR), 1.0f), C2 = __fdiv_rn(2.0f, (float)L);
    if (!(C1 > 0.0f)) return 0u;
    const float logC1 = spec_logf(C1);   // pow(C_1, e) = exp(e * log(C_1))
    const int dx = L - lx, dy = L - ly;  // pos - loc with loc = pos - L + (lx, ly)
    const float prox = __builtin_sqrtf((float)(dx * dx + dy * dy));
    const float e = __fsub_rn(__fmul_rn(C2, prox), 1.0f);
    const float y_add = __fdiv_rn(val, __fadd_rn(1.0f, spec_expf(__fmul_rn(e, logC1))));
    return y_add >= 1.0f ? (uint32_t)y_add : 0u;
}

// one lane per table entry: terrain [H][ly][lx] with val = row, robot [ly][lx] with val = 100 (lx fastest: consecutive lanes of
// scene_cloud_strips take consecutive lx = consecutive map columns)
__global__ __launch_bounds__(256) void scene_tables(uint32_t* terrain, uint32_t* robot, int H) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int nt = H * 4 * SC_TERRAIN_NORM * SC_TERRAIN_NORM, nr = 4 * SC_BOT_NORM * SC_BOT_NORM;
    if (t < nt) {
        const int y = t / (4 * SC_TERRAIN_NORM * SC_TERRAIN_NORM), r = t % (4 * SC_TERRAIN_NORM * SC_TERRAIN_NORM);
        terrain[t] = bump_tap((float)y, SC_TERRAIN_NORM, r % (2 * SC_TERRAIN_NORM), r / (2 * SC_TERRAIN_NORM));
    } else if (t - nt < nr) {
        const int r = t - nt;
        robot[r] = bump_tap(SC_BOT_AVOID, SC_BOT_NORM, r % (2 * SC_BOT_NORM), r / (2 * SC_BOT_NORM));
    }
}

__global__ __launch_bounds__(512) void scene_cloud_strips(const SceneParams p) { cloud_strips_body(p); }
__global__ void scene_balls(const SceneParams p) { balls_body(p); }
__global__ __launch_bounds__(64) void scene_world(const SceneParams p) { world_body(p); }
__global__ __launch_bounds__(64) void scene_conn1(const SceneParams p) { conn1_body(p); }
__global__ __launch_bounds__(64) void scene_conn0(const SceneParams p) { conn0_body(p); }

thread_local std::string g_scene_create_error;

}  // namespace

namespace {
int run_scene(yh_scene* h, const uint16_t* depth_dev, const uint8_t* cls_dev, const uint32_t* frame_dev, int frame_mode, int mode) {
    SceneParams p;
    p.depth = depth_dev; p.cls_id = cls_dev; p.frame = frame_dev; p.frame_mode = frame_mode;
    p.W = h->W; p.H = h->H; p.mode = mode; p.band_h = h->band_h;
    p.terrain_tab = h->terrain_tab; p.robot_tab = h->robot_tab;
    p.map = h->map; p.world = h->world; p.conn0 = h->conn0; p.conn1 = h->conn1; p.ball_acc = h->ball_acc; p.balls = h->balls;
    const int rc = scene_stamp(h, p);
    if (rc) return rc;
    const dim3 grid((unsigned)((h->W + 7) / 8), (unsigned)((h->H + 7) / 8)), block(8, 8);   // [80,60,1] x 8x8 at 640x480 (scene.rs:245,:256)
    hipLaunchKernelGGL(scene_world, grid, block, 0, h->stream, p);
    hipLaunchKernelGGL(scene_conn1, grid, block, 0, h->stream, p);
    hipLaunchKernelGGL(scene_conn0, grid, block, 0, h->stream, p);
    SCHK(h, hipGetLastError());
    h->ran = true;
    h->last_cls = cls_dev; h->last_frame = frame_dev; h->last_frame_mode = frame_mode; h->last_mode = mode;
    h->diag_ok = true; h->diag_why.clear();   // (a frame's own diagonals: both ends hold the same length, sqrt((1 + dy^2) + 1))
    return YH_OK;
}

}  // namespace

namespace yh {
int scene_stamp(yh_scene* h, const SceneParams& p) {
    SCHK(h, hipMemsetAsync(p.map, 0, (size_t)p.W * p.H * 4, h->stream));
    SCHK(h, hipMemsetAsync(p.ball_acc, 0, 300 * sizeof(long long), h->stream));
    hipLaunchKernelGGL(scene_cloud_strips, dim3((unsigned)((p.W + SC_CW - 1) / SC_CW), (unsigned)((p.H + p.band_h - 1) / p.band_h)), dim3(512), 0, h->stream, p);
    hipLaunchKernelGGL(scene_balls, dim3(1), dim3(128), 0, h->stream, p);
    return YH_OK;
}

// copy_from_slice semantics for host inputs (as yh_set_input_u8): the caller's buffers are free again when the call
// returns. The runtime has staged a copy from PAGEABLE memory by then; from pinned / registered memory the DMA is still
// reading, so wait for the copies (not for the kernels behind them: the event sits between the two).
int host_sources_done(yh_scene* h, const void* a, const void* b) {
    bool pinned = false;
    for (const void* p : { a, b }) {
        if (!p) continue;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost) pinned = true;
        else (void)hipGetLastError();   // (an unregistered pointer is reported as an error: not one)
    }
    if (!pinned) return YH_OK;
    SCHK(h, hipEventRecord(h->copied, h->stream));
    SCHK(h, hipEventSynchronize(h->copied));
    return YH_OK;
}

// The bump tables of a handle of height h->H (terrain [H][20][20], robot [40][40]), allocated and enqueued on its stream
hipError_t scene_tables_build(yh_scene* h) {
    const size_t nt = (size_t)h->H * 4 * SC_TERRAIN_NORM * SC_TERRAIN_NORM, nr = 4 * SC_BOT_NORM * SC_BOT_NORM;
    hipError_t e = hipMalloc((void**)&h->terrain_tab, nt * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->robot_tab, nr * 4);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(scene_tables, dim3((unsigned)((nt + nr + 255) / 256)), dim3(256), 0, h->stream, h->terrain_tab, h->robot_tab, h->H);
    return hipGetLastError();
}
}  // namespace yh

extern "C" {

const char* yh_scene_last_error(const yh_scene* h) { return h ? h->err.c_str() : g_scene_create_error.c_str(); }

int yh_scene_create(int32_t device, int32_t width, int32_t height, yh_scene** out) {
    if (!out) { g_scene_create_error = "null argument"; return YH_EINVAL; }
    *out = nullptr;
    if (width < 3 || height < 3 || width > 8192 || height > 8192) { g_scene_create_error = "frame size out of range"; return YH_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { g_scene_create_error = "no such HIP device (no CPU fallback)"; return YH_EHIP; }
    yh_scene* h = new yh_scene();
    h->dev = device; h->W = width; h->H = height;
    h->band_h = 64;   // map rows per workgroup of the stamping kernel. Measured at 640 x 480 (ms per frame, terrain only / robots + balls): 32 rows
                      // 0.238 / 0.270, 64 rows 0.229 / 0.262, 80 rows (one round of the chip: 240 workgroups) 0.250 / 0.304
    const size_t npx = (size_t)width * height;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->copied, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void**)&h->depth, npx * 2);
    if (e == hipSuccess) e = hipMalloc((void**)&h->cls_id, npx * 2);
    if (e == hipSuccess) e = hipMalloc((void**)&h->frame, npx * 4);
    // (input images start defined: nothing the handle can be asked to run ever reads uninitialised device memory)
    if (e == hipSuccess) e = hipMemsetAsync(h->depth, 0, npx * 2, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->cls_id, 0, npx * 2, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->frame, 0, npx * 4, h->stream);
    if (e == hipSuccess) e = hipMalloc((void**)&h->map, npx * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->world, npx * 16);
    if (e == hipSuccess) e = hipMalloc((void**)&h->conn0, npx * 16);
    if (e == hipSuccess) e = hipMalloc((void**)&h->conn1, npx * 16);
    if (e == hipSuccess) e = hipMalloc((void**)&h->balls, 100 * 16);
    if (e == hipSuccess) e = hipMalloc((void**)&h->ball_acc, 300 * sizeof(long long));
    if (e == hipSuccess) e = scene_tables_build(h);
    if (e != hipSuccess) { g_scene_create_error = std::string("scene setup: ") + hipGetErrorString(e); yh_scene_destroy(h); return YH_EHIP; }
    *out = h;
    return YH_OK;
}

void yh_scene_destroy(yh_scene* h) {
    if (!h) return;
    hipSetDevice(h->dev);
    if (h->stream) hipStreamSynchronize(h->stream);
    scene_path_free(h);
    scene_tour_free(h);
    scene_turn_free(h);
    scene_turn_tour_free(h);
    scene_solve_free(h);
    scene_memory_free(h);
    void* bufs[] = { h->depth, h->cls_id, h->frame, h->map, h->world, h->conn0, h->conn1, h->balls, h->ball_acc, h->terrain_tab, h->robot_tab };
    for (void* b : bufs) if (b) hipFree(b);
    if (h->copied) hipEventDestroy(h->copied);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

int yh_scene_append(yh_scene* h, const uint16_t* depth_host, const uint8_t* class_id_host, int32_t mode) {
    if (!h || !depth_host || !class_id_host) return YH_EINVAL;
    if (mode != YH_COMPAT_STRICT && mode != YH_COMPAT_SANE) return h->fail(YH_EINVAL, "bad compat mode");
    SCHK(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)h->W * h->H;
    SCHK(h, hipMemcpyAsync(h->depth, depth_host, npx * 2, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipMemcpyAsync(h->cls_id, class_id_host, npx * 2, hipMemcpyHostToDevice, h->stream));
    const int rc = host_sources_done(h, depth_host, class_id_host);
    if (rc) return rc;
    ++h->frames;
    return run_scene(h, h->depth, h->cls_id, nullptr, 0, mode);
}

int yh_scene_append_classified(yh_scene* h, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device, int32_t mode) {
    if (!h || !depth_host || !frame) return YH_EINVAL;
    if (mode != YH_COMPAT_STRICT && mode != YH_COMPAT_SANE) return h->fail(YH_EINVAL, "bad compat mode");
    SCHK(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)h->W * h->H;
    SCHK(h, hipMemcpyAsync(h->depth, depth_host, npx * 2, hipMemcpyHostToDevice, h->stream));
    const uint32_t* fdev = frame;
    if (!frame_on_device) { SCHK(h, hipMemcpyAsync(h->frame, frame, npx * 4, hipMemcpyHostToDevice, h->stream)); fdev = h->frame; }
    const int rc = host_sources_done(h, depth_host, frame_on_device ? nullptr : frame);
    if (rc) return rc;
    ++h->frames;
    return run_scene(h, h->depth, nullptr, fdev, mode == YH_COMPAT_STRICT ? 0 : 1, mode);
}

int yh_scene_read(yh_scene* h, uint32_t* map, float* world, float* conn0, float* conn1, float* balls) {
    if (!h) return YH_EINVAL;
    if (!h->ran) return h->fail(YH_ESTATE, "no frame has been appended");
    SCHK(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)h->W * h->H;
    if (map) SCHK(h, hipMemcpyAsync(map, h->map, npx * 4, hipMemcpyDeviceToHost, h->stream));
    if (world) SCHK(h, hipMemcpyAsync(world, h->world, npx * 16, hipMemcpyDeviceToHost, h->stream));
    if (conn0) SCHK(h, hipMemcpyAsync(conn0, h->conn0, npx * 16, hipMemcpyDeviceToHost, h->stream));
    if (conn1) SCHK(h, hipMemcpyAsync(conn1, h->conn1, npx * 16, hipMemcpyDeviceToHost, h->stream));
    if (balls) SCHK(h, hipMemcpyAsync(balls, h->balls, 100 * 16, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    return YH_OK;
}

int yh_scene_time(yh_scene* h, int32_t reps, float* ms_per_frame) {
    if (!h || reps < 1 || !ms_per_frame) return YH_EINVAL;
    if (!h->ran) return h->fail(YH_ESTATE, "no frame has been appended");
    if (scene_memory_is_pyramid_norm(h)) return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory_pyramid_norm: yh_scene_memory_pyramid_norm_time replays it");
    if (scene_memory_is_norm(h)) return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory_search_norm: yh_scene_memory_search_norm_time replays it");
    if (scene_memory_is_search(h))
        return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory_search: yh_scene_memory_search_time replays it");
    if (scene_memory_is_pyramid(h))
        return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory_pyramid: yh_scene_memory_pyramid_time replays it");
    if (scene_memory_is_last(h))
        return h->fail(YH_ESTATE, "the last frame came from yh_scene_append_memory: yh_scene_memory_time replays it");
    SCHK(h, hipSetDevice(h->dev));
    hipEvent_t a, b;
    SCHK(h, hipEventCreate(&a)); SCHK(h, hipEventCreate(&b));
    SCHK(h, hipEventRecord(a, h->stream));
    // the last append's own inputs and mode (a frame appended through yh_scene_append_classified is replayed from the
    // frame it was given - a device frame must still be valid -, not from the class image buffer it never wrote)
    const uint8_t* cls = h->last_cls; const uint32_t* fr = h->last_frame; const int fm = h->last_frame_mode, md = h->last_mode;
    for (int r = 0; r < reps; ++r) { const int rc = run_scene(h, h->depth, cls, fr, fm, md); if (rc) { hipEventDestroy(a); hipEventDestroy(b); return rc; } }
    SCHK(h, hipEventRecord(b, h->stream));
    SCHK(h, hipEventSynchronize(b));
    float ms = 0;
    hipEventElapsedTime(&ms, a, b);
    hipEventDestroy(a); hipEventDestroy(b);
    *ms_per_frame = ms / reps;
    return YH_OK;
}

}  // extern "C"
