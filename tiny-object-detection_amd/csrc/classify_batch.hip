// classify_batch.hip - yh_classify_batch_u32: Yolact::classify (src/yolact.rs:192-234) on n camera frames as ONE step of 2n tiles
// (DESIGN.md section 11 "Classify batch"). Frame-major front and back end around the engine's step:
//   resize_tables        once per geometry (W, H, S): every sample window of the four Triangle passes (vertical H -> S, horizontal
//                        W -> 2S, and back: vertical S -> H, horizontal 2S -> W) with its weights, computed with refpath.hip's own
//                        helpers (refpath_dev.h) - the quotients tri_w / sum are the single-frame kernels' bits by construction
//   classify_pre_batch   packed frames -> RGB8 tiles 2b, 2b + 1 in the engine's input buffer: unpack, vertical pass into LDS (f32,
//                        only the source columns the block's horizontal windows cover), horizontal pass from LDS, clamp, round,
//                        tile split on the store. A geometry whose block window does not fit the LDS budget (strong horizontal
//                        minification) takes the fallback form: the same arithmetic looping over global memory.
//   classify_post_batch  codes [2n][grid^2] -> packed frames: the frame's 2 grid^2 codes in LDS, per output pixel the vertical sums
//                        of the source columns of its horizontal window (shared inside an 8-column run, where they are equal),
//                        then the horizontal sum, clamp, round, repack. Neither the x8 upsampled image nor an f32 intermediate
//                        exists.
// Every output value is the sequence of __fmul_rn / __fadd_rn the two-pass kernels of refpath.hip perform, in their order: taps left
// to right from 0.0f, vertical first into f32, then horizontal; no FMA, no reassociation. cells_f32 and cells_postprocess are the
// single call's kernels at 2n tiles. The batch's buffers are its own.
// The three kernels, their tables and the pre kernel's plan are reached through classify_geo.h's geometry record and functions, which
// take a stream: the TFLite executor's batch (tflite_exec.hip, yh_tfl_classify_batch_u32) issues the same launches around its invoke.
#include "engine.h"
#include "refpath_dev.h"

using namespace yh;

namespace {

constexpr int kPreBX = 32, kPreBY = 8;          // output pixels of a classify_pre_batch block (256 lanes, one each)
constexpr int kPreLdsCols = 256;                // LDS budget of its vertical pass: 3 x kPreBY x 256 f32 = 24 KB
constexpr int kPostBX = 64, kPostTY = 4, kPostBY = 32;   // classify_post_batch: 64 x 4 lanes walk 64 x 32 output pixels

struct ResizeTabs { ResizeTab t[4]; };

// One lane per output index of each table.
__global__ __launch_bounds__(256) void resize_tables(ResizeTabs tabs) {
    int o = blockIdx.x * 256 + threadIdx.x;
    ResizeTab t = tabs.t[0];
    bool found = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (found) continue;
        if (o < tabs.t[k].out_size) { t = tabs.t[k]; found = true; }
        else o -= tabs.t[k].out_size;
    }
    if (!found) return;
    const SampleWin s = sample_window(o, t.in_size, t.out_size);
    t.win[o] = make_int2(s.left, s.n);
    float* w = t.w + (size_t)o * t.pitch;
    for (int i = 0; i < s.n && i < t.pitch; ++i) w[i] = __fdiv_rn(tri_w(s.left + i, s.inputc, s.sratio), s.sum);
}

__device__ __forceinline__ void unpack3(uint32_t px, float& c0, float& c1, float& c2) {
    c0 = (float)(px >> 24); c1 = (float)((px >> 16) & 0xFFu); c2 = (float)((px >> 8) & 0xFFu);
}

// grid (ceil(2S / 32), ceil(S / 8), n). frames [n][H][W] packed, tiles [2n][S][S][3]; tv: H -> S, th: W -> 2S.
// LDS form: vs [3][kPreBY][cols] f32 holds the vertical pass of source columns c0 .. c0 + ncols - 1 for the block's rows, where
// [c0, c0 + ncols) is the union of the block's horizontal windows (lefts and rights are monotone in the output column).
template <bool LDS>
__global__ __launch_bounds__(256) void classify_pre_batch(const uint32_t* __restrict__ frames, int W, int H, int S, ResizeTab tv,
                                                          ResizeTab th, int cols, uint8_t* __restrict__ tiles) {
    extern __shared__ float vs[];
    const int tid = threadIdx.x, tx = tid & (kPreBX - 1), ty = tid / kPreBX;
    const int ox0 = blockIdx.x * kPreBX, oy0 = blockIdx.y * kPreBY, ox = ox0 + tx, oy = oy0 + ty;
    const size_t b = blockIdx.z;
    const uint32_t* src = frames + b * W * H;
    const bool live = ox < 2 * S && oy < S;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    if (LDS) {
        const int oxl = min(ox0 + kPreBX, 2 * S) - 1, rows = min(kPreBY, S - oy0);
        const int c0 = th.win[ox0].x;
        const int2 wl = th.win[oxl];
        const int ncols = min(wl.x + wl.y - c0, cols);
        for (int idx = tid; idx < rows * ncols; idx += 256) {
            const int r = idx / ncols, c = idx - r * ncols;
            const int2 wv = tv.win[oy0 + r];
            const float* wp = tv.w + (size_t)(oy0 + r) * tv.pitch;
            const uint32_t* q = src + (size_t)wv.x * W + c0 + c;
            float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
            for (int i = 0; i < wv.y; ++i) {
                const float w = wp[i];
                float c0f, c1f, c2f;
                unpack3(q[(size_t)i * W], c0f, c1f, c2f);
                v0 = __fadd_rn(v0, __fmul_rn(c0f, w));
                v1 = __fadd_rn(v1, __fmul_rn(c1f, w));
                v2 = __fadd_rn(v2, __fmul_rn(c2f, w));
            }
            vs[(0 * kPreBY + r) * cols + c] = v0;
            vs[(1 * kPreBY + r) * cols + c] = v1;
            vs[(2 * kPreBY + r) * cols + c] = v2;
        }
        __syncthreads();
        if (!live) return;
        const int2 wh = th.win[ox];
        const float* wp = th.w + (size_t)ox * th.pitch;
        const int k0 = wh.x - c0;
        const int nt = min(wh.y, cols - k0);   // (= wh.y: the window lies inside the block's columns)
        for (int i = 0; i < nt; ++i) {
            const float w = wp[i];
            a0 = __fadd_rn(a0, __fmul_rn(vs[(0 * kPreBY + ty) * cols + k0 + i], w));
            a1 = __fadd_rn(a1, __fmul_rn(vs[(1 * kPreBY + ty) * cols + k0 + i], w));
            a2 = __fadd_rn(a2, __fmul_rn(vs[(2 * kPreBY + ty) * cols + k0 + i], w));
        }
    } else {
        if (!live) return;
        const int2 wh = th.win[ox], wv = tv.win[oy];
        const float* whp = th.w + (size_t)ox * th.pitch;
        const float* wvp = tv.w + (size_t)oy * tv.pitch;
        for (int i = 0; i < wh.y; ++i) {
            const uint32_t* q = src + (size_t)wv.x * W + wh.x + i;
            float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
            for (int j = 0; j < wv.y; ++j) {
                const float w = wvp[j];
                float c0f, c1f, c2f;
                unpack3(q[(size_t)j * W], c0f, c1f, c2f);
                v0 = __fadd_rn(v0, __fmul_rn(c0f, w));
                v1 = __fadd_rn(v1, __fmul_rn(c1f, w));
                v2 = __fadd_rn(v2, __fmul_rn(c2f, w));
            }
            const float w = whp[i];
            a0 = __fadd_rn(a0, __fmul_rn(v0, w));
            a1 = __fadd_rn(a1, __fmul_rn(v1, w));
            a2 = __fadd_rn(a2, __fmul_rn(v2, w));
        }
    }
    // yolact.rs:213-214: output column ox belongs to tile ox / S (a block may straddle the two tiles)
    const int tile = ox >= S ? 1 : 0, txs = ox - tile * S;
    uint8_t* d = tiles + (((2 * b + tile) * S + oy) * S + txs) * 3;
    d[0] = (uint8_t)to_u8(a0); d[1] = (uint8_t)to_u8(a1); d[2] = (uint8_t)to_u8(a2);
}

// grid (ceil(W / 64), ceil(H / 32), n). codes [2n][grid^2] (tile-major, as cells_postprocess writes them), out [n][H][W];
// tv: S -> H, th: 2S -> W. cs [grid][2 grid]: the frame's codes stitched t1 | t2 (yolact.rs:219-220); pixel (x, y) of the x8
// upsampled stitched image is cs[y >> 3][x >> 3] because S is a multiple of 8.
__global__ __launch_bounds__(256) void classify_post_batch(const uint32_t* __restrict__ codes, int grid, int W, int H, ResizeTab tv,
                                                           ResizeTab th, uint32_t* __restrict__ out) {
    extern __shared__ uint32_t cs[];
    const int tid = threadIdx.x, nc = grid * grid, g2 = 2 * grid;
    const size_t b = blockIdx.z;
    const uint32_t* cb = codes + b * 2 * nc;
    for (int c = tid; c < 2 * nc; c += 256) {
        const int tile = c >= nc ? 1 : 0, r = c - tile * nc, y = r / grid, x = r - y * grid;
        cs[y * g2 + tile * grid + x] = cb[c];
    }
    __syncthreads();
    const int ox = blockIdx.x * kPostBX + (tid & (kPostBX - 1));
    if (ox >= W) return;
    const int2 wh = th.win[ox];
    const float* whp = th.w + (size_t)ox * th.pitch;
    uint32_t* ob = out + b * W * H;
    for (int k = 0; k < kPostBY / kPostTY; ++k) {
        const int oy = blockIdx.y * kPostBY + k * kPostTY + tid / kPostBX;
        if (oy >= H) break;
        const int2 wv = tv.win[oy];
        const float* wvp = tv.w + (size_t)oy * tv.pitch;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
        int pcx = -1;
        for (int i = 0; i < wh.y; ++i) {
            const int cx = (wh.x + i) >> 3;
            if (cx != pcx) {   // the vertical sum of a source column depends on the column through its cell alone
                v0 = v1 = v2 = 0.0f;
                for (int j = 0; j < wv.y; ++j) {
                    const float w = wvp[j];
                    float c0f, c1f, c2f;
                    unpack3(cs[((wv.x + j) >> 3) * g2 + cx], c0f, c1f, c2f);
                    v0 = __fadd_rn(v0, __fmul_rn(c0f, w));
                    v1 = __fadd_rn(v1, __fmul_rn(c1f, w));
                    v2 = __fadd_rn(v2, __fmul_rn(c2f, w));
                }
                pcx = cx;
            }
            const float w = whp[i];
            a0 = __fadd_rn(a0, __fmul_rn(v0, w));
            a1 = __fadd_rn(a1, __fmul_rn(v1, w));
            a2 = __fadd_rn(a2, __fmul_rn(v2, w));
        }
        ob[(size_t)oy * W + ox] = (to_u8(a0) << 24) | (to_u8(a1) << 16) | (to_u8(a2) << 8);   // yolact.rs:230-233
    }
}

// The row pitch of a table: no window has more taps. A window is [floor(c - s), ceil(c + s)) clamped to the source, s = max(1, ratio).
int tab_pitch(int in_size, int out_size) {
    const double r = (double)in_size / (double)out_size;
    const int bound = (int)(2.0 * (r < 1.0 ? 1.0 : r)) + 4;
    return bound < in_size ? bound : in_size;
}

}  // namespace

namespace yh {

hipError_t classify_geo_ensure(ClassifyGeo* g, int w, int hh, int S, hipStream_t s) {
    if (g->tab && g->w == w && g->h == hh && g->S == S) return hipSuccess;
    const int in[4] = { hh, w, S, 2 * S }, out[4] = { S, 2 * S, hh, w };
    size_t n_out = 0, n_w = 0;
    for (int k = 0; k < 4; ++k) { n_out += (size_t)out[k]; n_w += (size_t)out[k] * tab_pitch(in[k], out[k]); }
    g->w = g->h = g->S = 0;
    const size_t bytes = n_out * sizeof(int2) + n_w * sizeof(float);
    if (bytes > g->tab_cap) {   // (grows only; the old one is freed)
        if (g->tab) hipFree(g->tab);
        g->tab = nullptr; g->tab_cap = 0;
        if (hipMalloc(&g->tab, bytes) != hipSuccess) { (void)hipGetLastError(); return hipErrorOutOfMemory; }
        g->tab_cap = bytes;
    }
    ResizeTabs tabs;
    int2* win = (int2*)g->tab;
    float* wts = (float*)(win + n_out);
    for (int k = 0; k < 4; ++k) {
        tabs.t[k] = ResizeTab{ win, wts, tab_pitch(in[k], out[k]), in[k], out[k] };
        win += out[k];
        wts += (size_t)out[k] * tabs.t[k].pitch;
        g->tabs[k] = tabs.t[k];
    }
    hipLaunchKernelGGL(resize_tables, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, tabs);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // plan: the source columns a block of kPreBX output columns can cover, from the ratio; past the LDS budget: the fallback form
    const double r = (double)w / (double)(2 * S);
    int cols = (int)((kPreBX - 1) * r + 2.0 * (r < 1.0 ? 1.0 : r)) + 5;
    if (cols > w) cols = w;
    g->pre_cols = cols <= kPreLdsCols ? cols : 0;
    g->w = w; g->h = hh; g->S = S;
    return hipSuccess;
}

hipError_t classify_geo_pre(const ClassifyGeo& g, const uint32_t* frames_dev, int n, uint8_t* tiles, hipStream_t s) {
    const int S = g.S, cols = g.pre_cols;
    const dim3 grid((unsigned)((2 * S + kPreBX - 1) / kPreBX), (unsigned)((S + kPreBY - 1) / kPreBY), (unsigned)n);
    if (cols > 0)
        hipLaunchKernelGGL((classify_pre_batch<true>), grid, dim3(256), (size_t)3 * kPreBY * cols * sizeof(float), s, frames_dev, g.w, g.h,
                           S, g.tabs[0], g.tabs[1], cols, tiles);
    else
        hipLaunchKernelGGL((classify_pre_batch<false>), grid, dim3(256), 0, s, frames_dev, g.w, g.h, S, g.tabs[0], g.tabs[1], 0, tiles);
    return hipGetLastError();
}

hipError_t classify_geo_post(const ClassifyGeo& g, const uint32_t* codes, int n, uint32_t* out, hipStream_t s) {
    const int grid = g.S / 8;
    const dim3 gr((unsigned)((g.w + kPostBX - 1) / kPostBX), (unsigned)((g.h + kPostBY - 1) / kPostBY), (unsigned)n);
    hipLaunchKernelGGL(classify_post_batch, gr, dim3(256), (size_t)2 * grid * grid * sizeof(uint32_t), s, codes, grid, g.w, g.h, g.tabs[2],
                       g.tabs[3], out);
    return hipGetLastError();
}

void classify_geo_free(ClassifyGeo* g) {
    if (g->tab) hipFree(g->tab);
    *g = ClassifyGeo();
}

}  // namespace yh

namespace {

// The tables of geometry (w, hh, S) exist on the device (enqueued on the stream if they had to be built).
int ensure_tables(yh_engine* h, int w, int hh) {
    const hipError_t e = classify_geo_ensure(&h->clsb_geo, w, hh, h->S, h->stream);
    if (e == hipErrorOutOfMemory) return h->fail(YH_ENOMEM, "hipMalloc classify batch tables");
    if (e != hipSuccess) return h->fail(YH_EHIP, std::string("classify batch tables: ") + hipGetErrorString(e));
    return YH_OK;
}

int enqueue_pre(yh_engine* h, const uint32_t* frames_dev, int n, uint8_t* tiles) {
    HIPCHK(h, classify_geo_pre(h->clsb_geo, frames_dev, n, tiles, h->stream));
    return YH_OK;
}

// clsb_cells [2n] -> codes -> clsb_frames [n], the read of the 2n flags (and of the frames) and the one wait. STRICT holds the
// frames back until the flags are known: out_host stays untouched when a frame diverges.
int post_stage(yh_engine* h, int n, int w, int hh, int mode, uint32_t* out_host, int32_t* diverged_host) {
    const int grid = h->S / 8;
    const size_t npx = (size_t)w * hh;
    hipError_t e = launch_cells_postprocess(h->clsb_cells, 2 * n, grid, h->C, mode, h->clsb_codes, h->clsb_div, h->stream);
    if (e != hipSuccess) return h->fail(YH_EHIP, std::string("classify batch post: ") + hipGetErrorString(e));
    HIPCHK(h, classify_geo_post(h->clsb_geo, h->clsb_codes, n, h->clsb_frames, h->stream));
    std::vector<int> div((size_t)2 * n);
    HIPCHK(h, hipMemcpyAsync(div.data(), h->clsb_div, div.size() * 4, hipMemcpyDeviceToHost, h->stream));
    const bool early = out_host && mode == YH_COMPAT_SANE;   // (SANE never diverges)
    if (early) HIPCHK(h, hipMemcpyAsync(out_host, h->clsb_frames, (size_t)n * npx * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    bool any = false;
    for (int b = 0; b < n; ++b) {
        const int d = (div[2 * b] || div[2 * b + 1]) ? 1 : 0;
        if (diverged_host) diverged_host[b] = d;
        any = any || d;
    }
    if (any) return h->fail(YH_EDIVERGE, "reference flood fill (yolact.rs:57-78) does not terminate on a frame of this batch");
    if (out_host && !early) HIPCHK(h, hipMemcpy(out_host, h->clsb_frames, (size_t)n * npx * 4, hipMemcpyDeviceToHost));
    h->clsb_n = n;
    return YH_OK;
}

// What every entry here checks before it touches anything; nullptr: fine.
const char* batch_check(const yh_engine* h, int n, int w, int hh) {
    if (n < 1) return "classify batch: n_frames must be at least 1";
    if (w < 1 || hh < 1) return "classify batch: bad frame size";
    if (h->S % 8 != 0 || h->S / 8 > 64) return "classify batch needs input_size % 8 == 0 (<= 512)";
    if (n > h->cfg.max_batch / 2) return "classify batch: 2 n_frames tiles exceed max_batch";
    return nullptr;
}

int grow_batch(yh_engine* h, int n, int w, int hh) {
    const int grid = h->S / 8;
    const size_t nt = (size_t)2 * n;
    int rc;
    if ((rc = instance_grow(h, (void**)&h->clsb_frames, &h->clsb_frames_cap, (size_t)n * w * hh * 4))) return rc;
    if ((rc = instance_grow(h, (void**)&h->clsb_cells, &h->clsb_cells_cap, nt * grid * grid * h->C * 4))) return rc;
    if ((rc = instance_grow(h, (void**)&h->clsb_codes, &h->clsb_codes_cap, nt * grid * grid * 4))) return rc;
    if ((rc = instance_grow(h, (void**)&h->clsb_div, &h->clsb_div_cap, nt * 4))) return rc;
    return ensure_tables(h, w, hh);
}

}  // namespace

namespace yh {

void classify_batch_free(yh_engine* h) {
    void* bufs[] = { h->clsb_frames, h->clsb_cells, h->clsb_codes, h->clsb_div };
    for (void* b : bufs) if (b) hipFree(b);
    classify_geo_free(&h->clsb_geo);
}

}  // namespace yh

extern "C" {

int yh_classify_batch_u32(yh_engine* h, const uint32_t* frames, int32_t frames_on_device, int32_t n, int32_t w, int32_t hh, int32_t mode,
                          uint32_t* out_host, int32_t* diverged_host) {
    if (!h || !frames) return YH_EINVAL;
    if (!h->weights_loaded) return h->fail(YH_ESTATE, "weights not loaded");
    if (const char* why = batch_check(h, n, w, hh)) return h->fail(YH_EINVAL, why);
    if (mode != YH_COMPAT_STRICT && mode != YH_COMPAT_SANE) return h->fail(YH_EINVAL, "bad compat mode");
    HIPCHK(h, hipSetDevice(h->dev));
    TraceRange tr("yh_classify_batch_u32");
    const int grid = h->S / 8;
    const size_t npx = (size_t)w * hh;
    h->clsb_n = -1;   // (until this batch is complete there is none: the buffers below may move)
    int rc = grow_batch(h, n, w, hh);
    if (rc) return rc;
    // yolact.rs:195-214 per frame: unpack, resize_exact(2S, S), crop two tiles -> tiles 2b, 2b + 1 of the engine's input
    if ((rc = wait_input(h))) return rc;
    const uint32_t* src = frames;
    if (!frames_on_device) {
        HIPCHK(h, hipMemcpyAsync(h->clsb_frames, frames, (size_t)n * npx * 4, hipMemcpyHostToDevice, h->stream));
        src = h->clsb_frames;
    }
    if ((rc = enqueue_pre(h, src, n, h->in_u8()))) return rc;
    // yolact.rs:216-217 + :163: the 2n tiles as one batch
    h->cur_n = 2 * n;
    if ((rc = run(h, 0))) return rc;
    // yolact.rs:169-189 (results[4] as f32), :90-131, :219-233
    const hipError_t e = launch_cells_f32(h->heads.d, 2 * n, h->cells, grid * grid, h->ldh, h->C, h->clsb_cells, h->stream);
    if (e != hipSuccess) return h->fail(YH_EHIP, std::string("classify batch cells: ") + hipGetErrorString(e));
    return post_stage(h, n, w, hh, mode, out_host, diverged_host);
}

const uint32_t* yh_classify_batch_device_frames(const yh_engine* h) { return h && h->clsb_n >= 1 ? h->clsb_frames : nullptr; }

int yh_op_classify_pre_batch(yh_engine* h, const uint32_t* frames_host, int32_t n, int32_t w, int32_t hh, uint8_t* tiles_host,
                             int32_t* form) {
    if (!h || !frames_host || !tiles_host) return YH_EINVAL;
    if (const char* why = batch_check(h, n, w, hh)) return h->fail(YH_EINVAL, why);
    HIPCHK(h, hipSetDevice(h->dev));
    h->clsb_n = -1;   // (the frames of an earlier batch are overwritten by the upload)
    int rc = grow_batch(h, n, w, hh);
    if (rc) return rc;
    const size_t nb = (size_t)2 * n * h->S * h->S * 3;
    uint8_t* tiles = nullptr;
    if (hipMalloc((void**)&tiles, nb) != hipSuccess) return h->fail(YH_ENOMEM, "hipMalloc tiles");
    hipError_t e = hipMemcpyAsync(h->clsb_frames, frames_host, (size_t)n * w * hh * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        rc = enqueue_pre(h, h->clsb_frames, n, tiles);
        if (rc == YH_OK) e = hipMemcpyAsync(tiles_host, tiles, nb, hipMemcpyDeviceToHost, h->stream);
    }
    const hipError_t es = hipStreamSynchronize(h->stream);
    hipFree(tiles);
    if (rc) return rc;
    if (e != hipSuccess || es != hipSuccess)
        return h->fail(YH_EHIP, std::string("classify pre batch: ") + hipGetErrorString(e != hipSuccess ? e : es));
    if (form) *form = h->clsb_geo.pre_cols > 0 ? 0 : 1;
    return YH_OK;
}

int yh_op_classify_post_batch(yh_engine* h, const float* cells_host, int32_t n, int32_t w, int32_t hh, int32_t mode,
                              uint32_t* frames_host, int32_t* diverged_host) {
    if (!h || !cells_host) return YH_EINVAL;
    if (const char* why = batch_check(h, n, w, hh)) return h->fail(YH_EINVAL, why);
    if (mode != YH_COMPAT_STRICT && mode != YH_COMPAT_SANE) return h->fail(YH_EINVAL, "bad compat mode");
    HIPCHK(h, hipSetDevice(h->dev));
    h->clsb_n = -1;
    int rc = grow_batch(h, n, w, hh);
    if (rc) return rc;
    const int grid = h->S / 8;
    HIPCHK(h, hipMemcpyAsync(h->clsb_cells, cells_host, (size_t)2 * n * grid * grid * h->C * 4, hipMemcpyHostToDevice, h->stream));
    return post_stage(h, n, w, hh, mode, frames_host, diverged_host);
}

}  // extern "C"
