// tflite_kernels.hip — the device code of the TFLite executor (tflite_exec.hip holds the plan and the C ABI): uint8 per-tensor
// quantised kernels whose arithmetic restates TensorFlow Lite's published uint8 reference kernels (gemmlowp fixed-point
// requantisation), their int8 / per-channel forms (DESIGN.md section 11 "TFLite int8"), and one launcher per kernel family
// (tflite_exec.h).
//
// Most are HBM/latency-bound byte kernels on small tensors (a 224x224 MobileNetV2 is ~0.3 GMAC): one lane per output element, output
// channel fastest (coalesced NHWC stores, broadcast input reads), int32 accumulation; the convolutions with Ci % 4 == 0 also have
// dot-product and int8 MFMA forms.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "tflite_exec.h"

using namespace yh;

namespace {
__device__ __forceinline__ int q_srdhm(int a, int b) {
    if (a == INT_MIN && b == INT_MIN) return INT_MAX;
    const long long ab = (long long)a * (long long)b;
    const long long nudge = ab >= 0 ? (1ll << 30) : (1ll - (1ll << 30));
    return (int)((ab + nudge) / (1ll << 31));
}
__device__ __forceinline__ int q_rdbpot(int x, int e) {
    if (e == 0) return x;
    const int mask = (1 << e) - 1, rem = x & mask, thr = (mask >> 1) + (x < 0 ? 1 : 0);
    return (x >> e) + (rem > thr ? 1 : 0);
}
__device__ __forceinline__ int q_mbqm(int x, int m, int shift) {
    const int left = shift > 0 ? shift : 0, right = shift > 0 ? 0 : -shift;
    return q_rdbpot(q_srdhm(x * (1 << left), m), right);
}
__device__ __forceinline__ int q_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// A quantised byte as the integer it stands for: S = the tensor is int8.
template <bool S> __device__ __forceinline__ int ldq(const uint8_t* p) { return S ? (int)(int8_t)*p : (int)*p; }
template <bool S> __device__ __forceinline__ int byteq(unsigned word, int e) { const unsigned b = (word >> (8 * e)) & 255u; return S ? (int)(int8_t)b : (int)b; }

// OS: the folded ADD's other operand is int8 (the producer's own signedness: fuse_plan folds no ADD of another type)
template <bool OS = false>
__device__ __forceinline__ int apply_post(const PostOps& po, int q, long long img, long long elem) {
    // (compile-time step indices: a run-time index into the kernel-argument block makes the compiler copy the whole block to
    // scratch - 344 bytes of private memory per lane in every convolution kernel, +45 % per invoke when first measured)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (i >= po.n) break;
        const PostStep& t = po.st[i];
        if (t.kind == 1) q = q_clamp(q_mbqm(q - t.zi, t.m, t.s) + t.zo, t.lo, t.hi);
        else if (t.kind == 2) q = t.lut[q];
        else if (t.kind == 4) q = (int)(int8_t)t.lut[q];   // (an int8 table: its entry is the byte of a signed value)
        else {
            const int o = ldq<OS>(po.other + img * po.other_s + elem);
            const int a = po.q_is_a ? q : o, b = po.q_is_a ? o : q;
            const int v1 = q_mbqm((a - po.za) * (1 << 20), po.m1, po.s1), v2 = q_mbqm((b - po.zb) * (1 << 20), po.m2, po.s2);
            q = q_clamp(q_mbqm(v1 + v2, po.mo, po.so) + po.azo, po.alo, po.ahi);
        }
    }
    return q;
}

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v4i_u __attribute__((ext_vector_type(4), aligned(4)));   // (a 16-byte load from a dword-aligned address)

// A convolution's accumulator (bias added) to its output value: one multiplier for the tensor (uint8), or channel oc's (int8, SGN)
template <bool SGN, class P>
__device__ __forceinline__ int conv_requant(const P& p, int acc, int oc) {
    return q_clamp(q_mbqm(acc, SGN ? p.mtab[oc] : p.mult, SGN ? p.stab[oc] : p.shift) + p.zo, p.lo, p.hi);
}

// Every kernel below that reads quantised bytes is a body with the signedness as a template parameter and two entry points: the
// uint8 one under its old name, compiled to what it was, and the int8 one (.._s8: int8 activations, symmetric int8 weights, one
// multiplier per output channel). (The px8 kernel takes the flag as a fourth parameter of the kernel template instead: as a body
// behind two entry points its uint8 instance compiled to other register counts.)
template <bool SGN>
__device__ __forceinline__ void conv_scalar_body(const ConvQ& p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.Ho * p.Wo * p.Co) return;
    const uint8_t* const px = p.x + blockIdx.y * p.xs;
    uint8_t* const py = p.y + blockIdx.y * p.ys;
    const int oc = t % p.Co, r0 = t / p.Co, ox = r0 % p.Wo, oy = r0 / p.Wo;
    int acc = 0;
    for (int r = 0; r < p.kh; ++r) {
        const int iy = oy * p.sh - p.ph + r * p.dh;
        if ((unsigned)iy >= (unsigned)p.H) continue;
        for (int s = 0; s < p.kw; ++s) {
            const int ix = ox * p.sw - p.pw + s * p.dw;
            if ((unsigned)ix >= (unsigned)p.W) continue;
            const uint8_t* xp = px + ((size_t)iy * p.W + ix) * p.Ci;
            const uint8_t* wp = p.w + (((size_t)oc * p.kh + r) * p.kw + s) * p.Ci;
            for (int c = 0; c < p.Ci; ++c) acc += (ldq<SGN>(xp + c) - p.zx) * (ldq<SGN>(wp + c) - p.zw);
        }
    }
    acc += p.bias ? p.bias[oc] : 0;
    py[t] = (uint8_t)apply_post<SGN>(p.po, conv_requant<SGN>(p, acc, oc), blockIdx.y, t);
}
__global__ __launch_bounds__(256) void tfl_conv_u8(const ConvQ p) { conv_scalar_body<false>(p); }
__global__ __launch_bounds__(256) void tfl_conv_s8(const ConvQ p) { conv_scalar_body<true>(p); }

// The same for layers the dot-product and MFMA kernels cannot take (Ci % 4 != 0: the model's first convolution, 3 channels) when
// yh_tuning.tfl_dot >= 1: one lane = one pixel x 8 output channels instead of one output element. The workgroup (256 pixels x 8
// channels) first puts its 8 x K weights, zero point already subtracted, into LDS as [k][8] ints: a lane then loads each input byte
// once for eight MACs and reads its weights with two broadcast ds_read_b128 (the element-per-lane kernel loads an input byte and a
// weight byte per MAC: 19.2 us for the 224 x 224 x 3 -> 112 x 112 x 32 layer of two images; this form: see DESIGN.md section 8).
template <int KH, int KW, int CI, bool SGN>   // (0, 0, 0: run-time extent; 3, 3, 3: the RGB stem; SGN: the int8 form)
__global__ __launch_bounds__(256) void tfl_conv_u8_px8(const ConvQ p) {
    __shared__ __attribute__((aligned(16))) int wl[kPx8MaxK * 8];
    const int K = p.kh * p.kw * p.Ci, oc0 = blockIdx.y * 8;
    for (int i = threadIdx.x; i < K * 8; i += 256) {
        const int k = i >> 3, j = i & 7, oc = oc0 + j < p.Co ? oc0 + j : p.Co - 1;   // (the clamped duplicates are not stored)
        wl[i] = ldq<SGN>(p.w + (size_t)oc * K + k) - p.zw;
    }
    __syncthreads();
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= p.Ho * p.Wo) return;
    const uint8_t* const px = p.x + blockIdx.z * p.xs;
    uint8_t* const py = p.y + blockIdx.z * p.ys;
    const int ox = pix % p.Wo, oy = pix / p.Wo;
    int acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if constexpr (KH > 0) {   // extent known at compile time: every input byte of the lane is asked for before the first MAC
        int xv[KH * KW * CI];
#pragma unroll
        for (int r = 0; r < KH; ++r)
#pragma unroll
            for (int s = 0; s < KW; ++s) {
                const int iy = oy * p.sh - p.ph + r * p.dh, ix = ox * p.sw - p.pw + s * p.dw;
                const bool in = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                const uint8_t* xp = px + ((size_t)(in ? iy : 0) * p.W + (in ? ix : 0)) * CI;
#pragma unroll
                for (int c = 0; c < CI; ++c) { const int v = ldq<SGN>(xp + c); xv[(r * KW + s) * CI + c] = in ? v - p.zx : 0; }
            }
#pragma unroll
        for (int k = 0; k < KH * KW * CI; ++k) {
            const v4i w0 = *(const v4i*)(wl + k * 8), w1 = *(const v4i*)(wl + k * 8 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { acc[j] += xv[k] * w0[j]; acc[4 + j] += xv[k] * w1[j]; }
        }
    } else {
        for (int r = 0; r < p.kh; ++r) {
            const int iy = oy * p.sh - p.ph + r * p.dh;
            if ((unsigned)iy >= (unsigned)p.H) continue;
            for (int s = 0; s < p.kw; ++s) {
                const int ix = ox * p.sw - p.pw + s * p.dw;
                if ((unsigned)ix >= (unsigned)p.W) continue;
                const uint8_t* xp = px + ((size_t)iy * p.W + ix) * p.Ci;
                const int* wk = wl + (r * p.kw + s) * p.Ci * 8;
                for (int c = 0; c < p.Ci; ++c) {
                    const int xv = ldq<SGN>(xp + c) - p.zx;
                    const v4i w0 = *(const v4i*)(wk + c * 8), w1 = *(const v4i*)(wk + c * 8 + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { acc[j] += xv * w0[j]; acc[4 + j] += xv * w1[j]; }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int oc = oc0 + j;
        if (oc < p.Co) {
            const int a = acc[j] + (p.bias ? p.bias[oc] : 0);
            py[(size_t)pix * p.Co + oc] = (uint8_t)apply_post<SGN>(p.po, conv_requant<SGN>(p, a, oc), blockIdx.z, (long long)pix * p.Co + oc);
        }
    }
}

// Same arithmetic, four MACs per instruction: for Ci % 4 == 0 the sum over the valid taps of
// (x - zx)(w - zw) is  sum(x w) - zw sum(x) - zx sum(w) + n zx zw  with the first two as
// v_dot4_u32_u8 over raw bytes and sum(w) per (channel, tap) tabulated at load time — all exact in
// int32 (|sum(x w)| <= 65025 * 9 * 1024 < 2^31 is checked when the plan is built). One lane = one
// pixel x 8 output channels; the channel block is the grid's y index, so weight words are
// wave-uniform and arrive through the scalar cache.
// A workgroup = 64 pixels x 8 channels; with KS == 4 its four waves each take a quarter of the input
// channels (the model's layers are small: 28 x 28 pixels x 128 channels is 13 x 16 workgroups, and
// the serial chain per lane is what takes the time) and wave 0 adds the partial sums from LDS.
template <int KS>
__global__ __launch_bounds__(64 * KS) void tfl_conv_u8_dot(const ConvQ p) {
    __shared__ unsigned part[KS > 1 ? (KS - 1) * 9 * 64 : 1];
    const uint8_t* const px = p.x + blockIdx.z * p.xs;
    uint8_t* const py = p.y + blockIdx.z * p.ys;
    const int lane = threadIdx.x & 63, ks = threadIdx.x >> 6;
    const int pix = blockIdx.x * 64 + lane, oc0 = blockIdx.y * 8;
    const bool live = pix < p.Ho * p.Wo;
    const int ox = live ? pix % p.Wo : 0, oy = live ? pix / p.Wo : 0, ci4 = p.Ci >> 2, ntaps = p.kh * p.kw;
    const int c_lo = ks * (ci4 / KS), c_hi = c_lo + ci4 / KS;
    const unsigned* w32 = (const unsigned*)p.w;
    unsigned acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, sx = 0;
    int ws[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, nv = 0;
    for (int r = 0; r < p.kh; ++r) {
        const int iy = oy * p.sh - p.ph + r * p.dh;
        for (int s = 0; s < p.kw; ++s) {
            const int ix = ox * p.sw - p.pw + s * p.dw, tap = r * p.kw + s;
            if (!live || (unsigned)iy >= (unsigned)p.H || (unsigned)ix >= (unsigned)p.W) continue;
            const unsigned* xp = (const unsigned*)(px + ((size_t)iy * p.W + ix) * p.Ci);
            for (int c = c_lo; c < c_hi; ++c) {
                const unsigned xv = xp[c];
                sx = __builtin_amdgcn_udot4(xv, 0x01010101u, sx, false);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int oc = oc0 + j < p.Co ? oc0 + j : p.Co - 1;   // wave-uniform; the clamped duplicates are not stored
                    acc[j] = __builtin_amdgcn_udot4(xv, w32[((size_t)oc * ntaps + tap) * ci4 + c], acc[j], false);
                }
            }
            if (ks == 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) ws[j] += p.wsum[(oc0 + j < p.Co ? oc0 + j : p.Co - 1) * ntaps + tap];
                ++nv;
            }
        }
    }
    if (KS > 1) {
        if (ks > 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) part[((ks - 1) * 9 + j) * 64 + lane] = acc[j];
            part[((ks - 1) * 9 + 8) * 64 + lane] = sx;
        }
        __syncthreads();
        if (ks > 0) return;
#pragma unroll
        for (int k = 0; k < KS - 1; ++k) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += part[(k * 9 + j) * 64 + lane];
            sx += part[(k * 9 + 8) * 64 + lane];
        }
    }
    if (!live) return;
    const int base = nv * p.Ci * p.zx * p.zw - p.zw * (int)sx;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int oc = oc0 + j;
        if (oc < p.Co) {
            const int a = (int)acc[j] + base - p.zx * ws[j] + (p.bias ? p.bias[oc] : 0);
            py[(size_t)pix * p.Co + oc] = (uint8_t)apply_post(p.po, q_clamp(q_mbqm(a, p.mult, p.shift) + p.zo, p.lo, p.hi), blockIdx.z, (long long)pix * p.Co + oc);
        }
    }
}

// ---- CONV_2D on the int8 matrix pipes: Ci % 64 == 0 (the FPN / protonet / head 3x3 convolutions of the
// model family - 85 % of its MACs - and the wide 1x1 convolutions). uint8 operands become int8 by flipping the top bit
// (x' = x - 128, w' = w - 128), v_mfma_i32_16x16x64_i8 accumulates sum(x' w') exactly in int32, and
//   sum (x - zx)(w - zw) = sum x'w' + (128 - zw) sum x' + (128 - zx) sum w' + K (128 - zx)(128 - zw)
// restores TFLite's value bit for bit: sum w' per channel is tabulated at load time, sum x' per output pixel is a v_dot4 beside
// the MFMAs, and a padded tap is fed the input's zero point (x - zx = 0: TFLite skips it). Implicit GEMM: a workgroup owns
// 64 channels x 64 output pixels (images of the batch plan are folded into the pixel index), four waves of 32 x 32, one tap's
// 64 channels per k-step, register-staged double buffer (tiles are 4 KB: the layers are small and latency-bound).
// Epilogue of the int8 MFMA convolutions: lane = pixel (wm, j, l15), channels (wc, i, 4 lg + e) [C/D layout of the 16 x 16 MFMA:
// column = lane & 15, rows 4 (lane >> 4) + e]; sx[j] = sum of the raw input bytes over the whole K of pixel (wm, j, l15).
//
// int8 tensors (SGN; DESIGN.md section 11 "TFLite int8") are the native form of the same kernels: with symmetric weights (zw = 0)
//   sum (x - zx) w = sum x w - zx sum w,
// the bytes go to the MFMA as loaded - no sum of x, no top-bit flip - the second term is in cterm[oc] with the bias (equal modulo
// 2^32, which is all the int32 accumulator keeps), a padded tap is fed the byte of zx, and the epilogue takes channel oc's
// multiplier and shift from tables padded like cterm.
template <int TI, int TJ, bool SGN>   // MFMA tiles per wave along the channels / the pixels
__device__ __forceinline__ void conv_i8_epilogue(const ConvI8& p, const v4i (&acc)[TI][TJ], const unsigned (&sx)[TJ], int m0, int ch0, int wc, int wm, int l15, int lg, int HoWo) {
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
        const int mo = m0 + wm * 16 * TJ + j * 16 + l15;
        if (mo >= p.M) continue;
        const int im = mo / HoWo, px = mo - im * HoWo;
        uint8_t* yrow = p.y + (long long)im * p.ys + (size_t)px * p.Co;
        const int xterm = SGN ? 0 : (128 - p.zw) * ((int)sx[j] - 128 * p.K);
#pragma unroll
        for (int i = 0; i < TI; ++i) {
            const int ch = ch0 + wc * 16 * TI + i * 16 + 4 * lg;
            if (ch >= p.Co) continue;
            unsigned packed = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int a = acc[i][j][e] + xterm + p.cterm[ch + e];   // (cterm is padded to CoPad)
                const unsigned q = (unsigned)apply_post<SGN>(p.po, conv_requant<SGN>(p, a, ch + e), im, (long long)px * p.Co + (ch + e < p.Co ? ch + e : 0));
                packed |= (q & 255u) << (8 * e);   // (a folded chain may end in int8 behind a uint8 producer too: the value's low byte)
            }
            if ((p.Co & 3) == 0 && (((size_t)yrow) & 3) == 0) *(unsigned*)(yrow + ch) = packed;   // (a CONCATENATION part may start at any byte)
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (ch + e < p.Co) yrow[ch + e] = (uint8_t)(packed >> (8 * e));
            }
        }
    }
}


template <bool SGN>
__device__ __forceinline__ void conv_i8_mfma_body(const ConvI8& p, char (&lds)[2][8192]) {   // lds: [stage][A 64 rows x 64 B | B 64 rows x 64 B]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    const int m0 = blockIdx.x * 64, ch0 = blockIdx.y * 64;
    // loader role: 16-byte chunk `lchunk` of row `lrow` of both tiles
    const int lrow = tid >> 2, lchunk = tid & 3;
    const int HoWo = p.Ho * p.Wo;
    const int m = m0 + lrow;
    const bool mlive = m < p.M;
    const int img = mlive ? m / HoWo : 0, rem = mlive ? m - img * HoWo : 0, oy = rem / p.Wo, ox = rem - oy * p.Wo;
    const uint8_t* ximg = p.x + (long long)img * p.xs;
    const uint8_t* wrow = p.wq + (size_t)(ch0 + lrow) * p.K + lchunk * 16;
    const unsigned zx4 = (unsigned)(SGN ? p.zx & 255 : p.zx) * 0x01010101u;
    const int lds_w = lrow * 64 + ((lchunk ^ ((lrow >> 2) & 3)) << 4);
    const int cchunks = p.Ci >> 6, nsteps = p.kh * p.kw * cchunks;
    // Register ring: the tiles of the next THREE k-steps are in flight while one is computed. The layers are small (50-200
    // workgroups of 2-18 k-steps) and every step used to wait one L2 round trip for the single tile it had prefetched: the kernel
    // was bound by steps x latency (12 us per launch, 46 launches = 0.67 of a 0.97 ms invoke). The ring is rotated by register
    // moves (a move waits for the load that fills its source, so four slots give three steps of distance).
    struct Tile { uint4 a, b; };
    // position of the NEXT tile to fetch along K, advanced incrementally (k order: tap outer, 64-channel chunk inner): the step
    // index is wave-uniform, and two integer divisions per k-step were a third of a step's instructions on a wave that has its
    // SIMD to itself (one workgroup of four waves per CU: nothing else hides them)
    int f_r = 0, f_s = 0, f_cc = 0, f_step = 0;
    const int iy0 = oy * p.sh - p.ph, ix0 = ox * p.sw - p.pw;
    const uint8_t* const xlane = ximg + lchunk * 16;
    auto fetch = [&]() {
        Tile t;
        t.a = *(const uint4*)(wrow + (size_t)f_step * 64);       // K index = tap * Ci + cc * 64 = step * 64
        const int iy = iy0 + f_r * p.dh, ix = ix0 + f_s * p.dw;
        const bool in = mlive && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        // padded tap (and rows past M): x = zx contributes (x - zx) = 0. (The address is clamped into the image, the value selected.)
        const uint4 v = *(const uint4*)(xlane + (unsigned)(((in ? iy : 0) * p.W + (in ? ix : 0)) * p.Ci + f_cc * 64));
        t.b = in ? v : make_uint4(zx4, zx4, zx4, zx4);
        if (f_step + 1 < nsteps) {                                // (past the end: the last tile again, never used)
            ++f_step;
            if (++f_cc == cchunks) { f_cc = 0; if (++f_s == p.kw) { f_s = 0; ++f_r; } }
        }
        return t;
    };
    auto stash = [&](int st, const Tile& t) {
        *(uint4*)(lds[st] + lds_w) = t.a;
        *(uint4*)(lds[st] + 4096 + lds_w) = t.b;
    };
    const int wc = wave >> 1, wm = wave & 1;
    v4i acc[2][2];
    unsigned sx[2] = { 0u, 0u };
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = v4i{ 0, 0, 0, 0 };
    Tile t0 = fetch(), t1 = fetch(), t2 = fetch(), t3 = fetch();
    stash(0, t0);
    __syncthreads();
    for (int step = 0; step < nsteps; ++step) {
        const int st = step & 1;
        // t1, t2, t3 = tiles step + 1 .. step + 3 (in flight); the slot of the tile now in LDS takes tile step + 4
        t0 = fetch();
        v4i fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = wc * 32 + i * 16 + l15;
            fa[i] = *(const v4i*)(lds[st] + row * 64 + ((lg ^ ((row >> 2) & 3)) << 4));
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = wm * 32 + j * 16 + l15;
            const v4i raw = *(const v4i*)(lds[st] + 4096 + row * 64 + ((lg ^ ((row >> 2) & 3)) << 4));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (SGN) fb[j][e] = raw[e];
                else {
                    sx[j] = __builtin_amdgcn_udot4((unsigned)raw[e], 0x01010101u, sx[j], false);
                    fb[j][e] = raw[e] ^ (int)0x80808080u;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
        stash(st ^ 1, t1);                                     // (the other stage was last read one step ago, behind a barrier; after the last step: unused)
        __syncthreads();
        t1 = t2; t2 = t3; t3 = t0;
    }
    // sum x over the whole K of this lane's pixel: the four lane groups hold the four 16-byte quarters of every k-step
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        sx[j] += __shfl_xor(sx[j], 16);
        sx[j] += __shfl_xor(sx[j], 32);
    }
    conv_i8_epilogue<2, 2, SGN>(p, acc, sx, m0, ch0, wc, wm, l15, lg, HoWo);
}
__global__ __launch_bounds__(256) void tfl_conv_i8_mfma(const ConvI8 p) {
    __shared__ __attribute__((aligned(16))) char lds[2][8192];
    conv_i8_mfma_body<false>(p, lds);
}
__global__ __launch_bounds__(256) void tfl_conv_s8_mfma(const ConvI8 p) {
    __shared__ __attribute__((aligned(16))) char lds[2][8192];
    conv_i8_mfma_body<true>(p, lds);
}

// ---- The same convolution with NO LDS and no barrier (yh_tuning.tfl_dot = 3, the default, for the launches conv_i8_direct_pays()
// names): one wave = ONE 16 x 16 MFMA tile, and every operand register is one 16-byte global load - lane (l15, lg) of
// v_mfma_i32_16x16x64_i8 holds bytes 16 lg .. 16 lg + 15 of row l15's 64-deep K chunk, which is contiguous both in the weight panel
// [Co][K] and in an NHWC pixel's channels. What a launch of the LDS tiles costs (tools/study/tfl_layer_table.py: the per-launch
// timeline of the 136-op model) is not its MFMAs: it is the serial k-loop (0.36 us per step: stash / barrier / fragment reads on
// waves that have their SIMD to themselves) and the epilogue - 16 outputs per lane, each a fixed-point requantisation and, where an
// ADD or a LUT is folded in, that arithmetic too (a projection convolution with the residual ADD folded in: 15.6 us against 8.5
// without) - on 2 to 50 workgroups of a 256-CU chip. Here a lane finishes 4 outputs, a 7-workgroup layer becomes 100 waves, a k-step
// is 2 loads, 4 v_dot4, 4 v_xor and 1 MFMA, and D steps of loads are in flight (a ring of registers indexed at compile time). The
// re-reads of the operands (each weight row by every pixel tile, each pixel by every channel tile) are L2 hits. K chunks past Ci
// (Ci % 4 == 0, not % 64: 16, 24, 32, 96, 144 channels) are fed zeros on both sides, which add nothing to sum x'w' nor to sum x.
// D = the depth of the register ring = the k-steps of one loop iteration. The loop body has NO branch: with a wave-uniform
// `if (step < nsteps)` around each step hipcc's wait insertion gave up counting and put s_waitcnt vmcnt(0..3) in front of every step
// - eight steps of loads "in flight" that were waited for one by one. So the k-steps are rounded up to a multiple of D (the launch
// picks the D that pads least), and the steps past the end load the last step again and are fed zeros.
// ONCE: the launch has exactly D k-steps - every load of the wave is asked for before its first MFMA and nothing is fetched again
// (the 3x3 x 128-channel head convolutions, 18 steps: 9.5 -> 7 us against two drained iterations of a ring of 9).
// KK (ONCE only): the kernel extent, 1 x 1 or 3 x 3 - the tap and the channel chunk of step d are then compile-time constants and
// the position bookkeeping below disappears from the prologue (0: run-time extent, looped form).
template <int D, bool ONCE, int KK, bool SGN>
__device__ __forceinline__ void conv_i8_direct_tile(const ConvI8& p, int tile_m, int tile_c) {
    static_assert(KK == 0 || (ONCE && D % (KK * KK) == 0), "compile-time extents: the launch's k-steps are exactly D");
    const int lane = threadIdx.x, l15 = lane & 15, lg = lane >> 4;
    const int m0 = tile_m * 16, ch0 = tile_c * 16;
    const int HoWo = p.Ho * p.Wo;
    const int m = m0 + l15;
    const bool live = m < p.M;
    const int img = live ? m / HoWo : 0, rem = live ? m - img * HoWo : 0, oy = rem / p.Wo, ox = rem - oy * p.Wo;
    const uint8_t* const xb = p.x + (long long)img * p.xs;
    const int iy0 = oy * p.sh - p.ph, ix0 = ox * p.sw - p.pw;
    const uint8_t* const wa = p.wq + (size_t)(ch0 + l15) * p.K;   // (rows up to CoPad exist)
    const int cchunks = (p.Ci + 63) >> 6, nsteps = p.kh * p.kw * cchunks;
    const int zx4 = (int)((unsigned)(SGN ? p.zx & 255 : p.zx) * 0x01010101u);
    struct Tile { v4i a, b; };
    int f_r = 0, f_s = 0, f_cc = 0, f_tap = 0, f_n = 0;   // the next k-step to fetch: tap (f_r, f_s) = f_tap, 64-channel chunk f_cc
    auto fetch_at = [&](int r, int s_, int tap, int cc, bool more) {
        Tile t;
        // (per lane group: the last chunk of a Ci that is not a multiple of 64 holds nd < 4 dwords of this lane's 16 bytes - the rest
        // belongs to the next tap / pixel and is fed zeros; Ci % 4 == 0, so the loads are dword-aligned, not 16-byte aligned)
        const int left = p.Ci - (cc * 64 + lg * 16), nd = !more ? 0 : (left >= 16 ? 4 : (left > 0 ? left >> 2 : 0));
        const int coff = left > 0 ? cc * 64 + lg * 16 : 0;   // (a lane group past Ci reads its row's first bytes: nothing is read more than 12 bytes past a row)
        const v4i va = *(const v4i_u*)(wa + tap * p.Ci + coff);
        const int iy = iy0 + r * p.dh, ix = ix0 + s_ * p.dw;
        const bool in = live && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        // padded tap (and rows past M): x = zx contributes (x - zx) = 0. (The address is clamped into the image, the value selected.)
        const v4i vb = *(const v4i_u*)(xb + (unsigned)(((in ? iy : 0) * p.W + (in ? ix : 0)) * p.Ci + coff));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            t.a[e] = e < nd ? va[e] : 0;
            t.b[e] = e < nd ? (in ? vb[e] : zx4) : 0;
        }
        return t;
    };
    auto fetch = [&](int d) {
        if constexpr (KK > 0) {
            constexpr int CC = D / (KK * KK);
            const int tap = d / CC;
            return fetch_at(tap / KK, tap % KK, tap, d % CC, true);
        } else {
            // (wave-uniform position; past the end it stays on the last step and the tile is zeros)
            const Tile t = fetch_at(f_r, f_s, f_tap, f_cc, f_n < nsteps);
            // advance (selects, no branch); the last step is never left
            const int adv = f_n + 1 < nsteps;
            f_n += f_n < nsteps;
            const int ncc = f_cc + 1, wrap_c = ncc == cchunks;
            const int ns = f_s + 1, wrap_s = wrap_c && ns == p.kw;
            f_cc = adv ? (wrap_c ? 0 : ncc) : f_cc;
            f_tap = adv ? f_tap + wrap_c : f_tap;
            f_s = adv ? (wrap_c ? (wrap_s ? 0 : ns) : f_s) : f_s;
            f_r = adv ? f_r + wrap_s : f_r;
            return t;
        }
    };
    v4i acc[1][1] = { { v4i{ 0, 0, 0, 0 } } };
    unsigned sx[1] = { 0u };
    Tile ring[D];
#pragma unroll
    for (int d = 0; d < D; ++d) ring[d] = fetch(d);
    for (int step = 0; step < (ONCE ? 1 : nsteps); step += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const Tile t = ring[d];
            if (!ONCE) ring[d] = fetch(d);   // (k-step step + d + D: asked for before this step's MFMA is issued)
            v4i fb = t.b;   // (int8: the operand as loaded - the k-step is 2 loads and 1 MFMA)
            if constexpr (!SGN) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    sx[0] = __builtin_amdgcn_udot4((unsigned)t.b[e], 0x01010101u, sx[0], false);
                    fb[e] = t.b[e] ^ (int)0x80808080u;
                }
            }
            acc[0][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(t.a, fb, acc[0][0], 0, 0, 0);
        }
    }
    if constexpr (!SGN) {
        sx[0] += __shfl_xor(sx[0], 16);
        sx[0] += __shfl_xor(sx[0], 32);
    }
    conv_i8_epilogue<1, 1, SGN>(p, acc, sx, m0, ch0, 0, 0, l15, lg, HoWo);
}
template <int D, bool ONCE, int KK>
__global__ __launch_bounds__(64) void tfl_conv_i8_direct(const ConvI8 p) {
    conv_i8_direct_tile<D, ONCE, KK, false>(p, blockIdx.x, blockIdx.y);
}
template <int D, bool ONCE, int KK>
__global__ __launch_bounds__(64) void tfl_conv_s8_direct(const ConvI8 p) {
    conv_i8_direct_tile<D, ONCE, KK, true>(p, blockIdx.x, blockIdx.y);
}
// Several INDEPENDENT convolutions of one kernel form as ONE launch (yh_tuning.tfl_group; group_plan): the prediction head's
// tower convolutions of the five pyramid levels, then its fifteen output convolutions, the FPN's output convolutions. The
// problems' parameter blocks sit in device memory; a workgroup finds its problem in the tile prefix table (at most kMaxGroup
// entries, wave-uniform) and runs the same tile code on it.
template <int D, bool ONCE, int KK, bool SGN>
__device__ __forceinline__ void conv_i8_direct_group_body(const ConvI8* __restrict__ probs, const int* __restrict__ tile_start, int nprob) {
    const int bid = blockIdx.x;
    int pi = 0;
    for (int i = 1; i < nprob; ++i) pi = bid >= tile_start[i] ? i : pi;
    const ConvI8 p = probs[pi];
    const int t = bid - tile_start[pi], mtiles = (p.M + 15) >> 4;
    conv_i8_direct_tile<D, ONCE, KK, SGN>(p, t % mtiles, t / mtiles);
}
template <int D, bool ONCE, int KK>
__global__ __launch_bounds__(64) void tfl_conv_i8_direct_group(const ConvI8* __restrict__ probs, const int* __restrict__ tile_start, int nprob) {
    conv_i8_direct_group_body<D, ONCE, KK, false>(probs, tile_start, nprob);
}
template <int D, bool ONCE, int KK>
__global__ __launch_bounds__(64) void tfl_conv_s8_direct_group(const ConvI8* __restrict__ probs, const int* __restrict__ tile_start, int nprob) {
    conv_i8_direct_group_body<D, ONCE, KK, true>(probs, tile_start, nprob);
}
// The forms the register-fed kernel is built in, one row each: taking the two kernels' addresses instantiates them, and nothing else
// names a (D, ONCE, KK). conv_i8_direct_form (below) finds a convolution's row; a group's members share one. The rows' order - and
// group before single within a row - is the kernels' order in the code object, which can move a step by a few tenths of a percent
// (DESIGN.md section 4).
struct DirectForm {
    int D; bool once; int KK;
    void (*group)(const ConvI8*, const int*, int);
    void (*single)(const ConvI8);
    void (*group_s8)(const ConvI8*, const int*, int);   // the row's second instantiation: int8 activations (not a row of its own)
    void (*single_s8)(const ConvI8);
};
template <int D, bool ONCE, int KK>
constexpr DirectForm direct_form() {
    return { D, ONCE, KK, tfl_conv_i8_direct_group<D, ONCE, KK>, tfl_conv_i8_direct<D, ONCE, KK>, tfl_conv_s8_direct_group<D, ONCE, KK>, tfl_conv_s8_direct<D, ONCE, KK> };
}
constexpr DirectForm kDirectForms[] = {
    // the whole K in one pass, 3 x 3: 64 and 128 input channels
    direct_form<9, true, 3>(), direct_form<18, true, 3>(),
    // ... 1 x 1: up to 384 input channels, 512, 576, 768, 960, 1152
    direct_form<1, true, 1>(), direct_form<2, true, 1>(), direct_form<3, true, 1>(), direct_form<4, true, 1>(), direct_form<5, true, 1>(), direct_form<6, true, 1>(),
    direct_form<8, true, 1>(), direct_form<9, true, 1>(), direct_form<12, true, 1>(), direct_form<15, true, 1>(), direct_form<18, true, 1>(),
    // looped, run-time extent: every other step count or extent
    direct_form<4, false, 0>(), direct_form<5, false, 0>(), direct_form<6, false, 0>(), direct_form<8, false, 0>(), direct_form<9, false, 0>(),
};
constexpr int kDirectFormCount = (int)(sizeof kDirectForms / sizeof kDirectForms[0]);

// (Round 4 also built the same convolution with its K split over the four waves of the workgroup - every wave the whole 64 x 64
// tile for a quarter of the k-steps, partial tiles added through LDS atomics: bit-identical, and SLOWER everywhere (18 k-steps: 13 ->
// 16-20 us, 4 k-steps: 5.3 -> 9.5 us). A launch costs 6.4 us + 0.36 us per k-step whatever its pixel count (tools/study/
// tfl_conv_steps.py), and that per-step cost is the wave's own instruction issue - 88 instructions - not a latency the split
// could overlap: four times the work per wave and step took four times as long. Removed.)

template <bool SGN>
__device__ __forceinline__ void dwconv_body(const ConvQ& p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.Ho * p.Wo * p.Co) return;
    const uint8_t* const px = p.x + blockIdx.y * p.xs;
    uint8_t* const py = p.y + blockIdx.y * p.ys;
    const int oc = t % p.Co, r0 = t / p.Co, ox = r0 % p.Wo, oy = r0 / p.Wo, ic = oc / p.dm;
    int acc = 0;
    for (int r = 0; r < p.kh; ++r) {
        const int iy = oy * p.sh - p.ph + r * p.dh;
        if ((unsigned)iy >= (unsigned)p.H) continue;
        for (int s = 0; s < p.kw; ++s) {
            const int ix = ox * p.sw - p.pw + s * p.dw;
            if ((unsigned)ix >= (unsigned)p.W) continue;
            acc += (ldq<SGN>(px + ((size_t)iy * p.W + ix) * p.Ci + ic) - p.zx) * (ldq<SGN>(p.w + ((size_t)r * p.kw + s) * p.Co + oc) - p.zw);
        }
    }
    acc += p.bias ? p.bias[oc] : 0;
    py[t] = (uint8_t)apply_post<SGN>(p.po, conv_requant<SGN>(p, acc, oc), blockIdx.y, t);
}
__global__ __launch_bounds__(256) void tfl_dwconv_u8(const ConvQ p) { dwconv_body<false>(p); }
__global__ __launch_bounds__(256) void tfl_dwconv_s8(const ConvQ p) { dwconv_body<true>(p); }

// Depth multiplier 1, channels a multiple of 4, dword-aligned tensors, kernel extent known at compile time (3 x 3: every depthwise
// layer of the model family): one lane = one pixel x FOUR channels - a tap is one dword of input and one dword of weights for four
// MACs - and the loop over the taps has no branch: all KH x KW input dwords are asked for at once (a tap outside the image loads
// from a clamped address and is given the zero point, (x - zx) = 0), so a lane waits one memory latency instead of one per tap. The
// element-per-lane kernel above takes 5.2 us (small layers) to 10.7 us (112 x 112 x 32 x 2 images) per launch.
template <int KH, int KW, bool SGN>
__device__ __forceinline__ void dwconv_c4_body(const ConvQ& p) {
    const int c4n = p.Co >> 2;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.Ho * p.Wo * c4n) return;
    const uint8_t* const px = p.x + blockIdx.y * p.xs + 4 * (t % c4n);
    uint8_t* const py = p.y + blockIdx.y * p.ys;
    const int cg = t % c4n, r0 = t / c4n, ox = r0 % p.Wo, oy = r0 / p.Wo;
    const unsigned zx4 = (unsigned)(SGN ? p.zx & 255 : p.zx) * 0x01010101u;
    unsigned xv[KH * KW], wv[KH * KW];
#pragma unroll
    for (int r = 0; r < KH; ++r)
#pragma unroll
        for (int s = 0; s < KW; ++s) {
            const int iy = oy * p.sh - p.ph + r * p.dh, ix = ox * p.sw - p.pw + s * p.dw;
            const bool in = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
            const unsigned v = *(const unsigned*)(px + ((size_t)(in ? iy : 0) * p.W + (in ? ix : 0)) * p.Ci);
            xv[r * KW + s] = in ? v : zx4;
            wv[r * KW + s] = *(const unsigned*)(p.w + (size_t)(r * KW + s) * p.Co + 4 * cg);
        }
    int acc[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int k = 0; k < KH * KW; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += (byteq<SGN>(xv[k], e) - p.zx) * (byteq<SGN>(wv[k], e) - p.zw);
    const long long e0 = (long long)r0 * p.Co + 4 * cg;
    unsigned packed = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int a = acc[e] + (p.bias ? p.bias[4 * cg + e] : 0);
        const unsigned q = (unsigned)apply_post<SGN>(p.po, conv_requant<SGN>(p, a, 4 * cg + e), blockIdx.y, e0 + e);
        packed |= (q & 255u) << (8 * e);
    }
    if ((((size_t)py) & 3) == 0) *(unsigned*)(py + e0) = packed;   // (a CONCATENATION part may start at any byte)
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e) py[e0 + e] = (uint8_t)(packed >> (8 * e));
    }
}
template <int KH, int KW>
__global__ __launch_bounds__(256) void tfl_dwconv_u8_c4(const ConvQ p) { dwconv_c4_body<KH, KW, false>(p); }
template <int KH, int KW>
__global__ __launch_bounds__(256) void tfl_dwconv_s8_c4(const ConvQ p) { dwconv_c4_body<KH, KW, true>(p); }

// RESHAPE: a plain device copy as a kernel (a memcpy NODE in the captured plan crashed rocprofv3's
// kernel tracing on graph replay; kernels are also what the profiler can attribute)
__global__ __launch_bounds__(256) void tfl_copy_bytes(const uint8_t* __restrict__ x, uint8_t* __restrict__ y, long long n) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n16 = n >> 4;
    if (t < n16) ((uint4*)y)[t] = ((const uint4*)x)[t];
    if (t < (n & 15)) y[(n16 << 4) + t] = x[(n16 << 4) + t];
}

template <bool SGN>
__device__ __forceinline__ void add_body(const AddQ& p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.n) return;
    const int v1 = q_mbqm((ldq<SGN>(p.a + t) - p.za) * (1 << 20), p.m1, p.s1);
    const int v2 = q_mbqm((ldq<SGN>(p.b + t) - p.zb) * (1 << 20), p.m2, p.s2);
    p.y[t] = (uint8_t)q_clamp(q_mbqm(v1 + v2, p.mo, p.so) + p.zo, p.lo, p.hi);
}
__global__ __launch_bounds__(256) void tfl_add_u8(const AddQ p) { add_body<false>(p); }
__global__ __launch_bounds__(256) void tfl_add_s8(const AddQ p) { add_body<true>(p); }

// requantise (QUANTIZE u8->u8, RELU/RELU6) : clamp(mbqm(q - zi) + zo, lo, hi)
__global__ __launch_bounds__(256) void tfl_requant_u8(const uint8_t* x, uint8_t* y, long long n, int zi, int zo, int m, int s, int lo, int hi) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n) y[t] = (uint8_t)q_clamp(q_mbqm((int)x[t] - zi, m, s) + zo, lo, hi);
}
// ... of an int8 input (QUANTIZE i8->i8 and i8->u8, RELU / RELU6 on int8; u8->i8 is the kernel above: the output's type is its range)
__global__ __launch_bounds__(256) void tfl_requant_s8(const uint8_t* x, uint8_t* y, long long n, int zi, int zo, int m, int s, int lo, int hi) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n) y[t] = (uint8_t)q_clamp(q_mbqm(ldq<true>(x + t) - zi, m, s) + zo, lo, hi);
}
template <bool SGN>
__device__ __forceinline__ void quantize_f32_body(const float* x, uint8_t* y, long long n, float scale, int zo) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const float v = __fdiv_rn(x[t], scale);
    const float r = v >= 0.0f ? floorf(__fadd_rn(v, 0.5f)) : ceilf(__fsub_rn(v, 0.5f));
    y[t] = (uint8_t)q_clamp((int)r + zo, SGN ? -128 : 0, SGN ? 127 : 255);
}
__global__ __launch_bounds__(256) void tfl_quantize_f32(const float* x, uint8_t* y, long long n, float scale, int zo) { quantize_f32_body<false>(x, y, n, scale, zo); }
__global__ __launch_bounds__(256) void tfl_quantize_f32_s8(const float* x, uint8_t* y, long long n, float scale, int zo) { quantize_f32_body<true>(x, y, n, scale, zo); }
__global__ __launch_bounds__(256) void tfl_dequantize_u8(const uint8_t* x, float* y, long long n, float scale, int z) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n) y[t] = __fmul_rn(scale, (float)((int)x[t] - z));   // yolact.rs:177
}
__global__ __launch_bounds__(256) void tfl_dequantize_s8(const uint8_t* x, float* y, long long n, float scale, int z) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n) y[t] = __fmul_rn(scale, (float)(ldq<true>(x + t) - z));
}
__global__ __launch_bounds__(256) void tfl_lut_u8(const uint8_t* x, uint8_t* y, long long n, const uint8_t* lut) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n) y[t] = lut[x[t]];
}
__global__ __launch_bounds__(256) void tfl_pad_u8(const PadQ p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n = (long long)p.od[0] * p.od[1] * p.od[2] * p.od[3];
    if (t >= n) return;
    int c[4];
    long long r = t;
    for (int d = 3; d >= 0; --d) { c[d] = (int)(r % p.od[d]) - p.before[d]; r /= p.od[d]; }
    bool in = true;
    for (int d = 0; d < 4; ++d) in = in && (unsigned)c[d] < (unsigned)p.id[d];
    p.y[t] = in ? p.x[(((long long)c[0] * p.id[1] + c[1]) * p.id[2] + c[2]) * p.id[3] + c[3]] : (uint8_t)p.fill;
}
__global__ __launch_bounds__(256) void tfl_resize_bilinear_u8(const ResizeQ p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.Ho * p.Wo * p.C) return;
    const uint8_t* const px = p.x + (size_t)blockIdx.y * p.H * p.W * p.C;   // (batch plan: image-major)
    uint8_t* const py = p.y + blockIdx.y * p.ys;
    const int c = t % p.C, r0 = t / p.C, ox = r0 % p.Wo, oy = r0 / p.Wo;
    const float iy = p.half_pixel ? __fsub_rn(__fmul_rn(__fadd_rn((float)oy, 0.5f), p.hs), 0.5f) : __fmul_rn((float)oy, p.hs);
    const float ix = p.half_pixel ? __fsub_rn(__fmul_rn(__fadd_rn((float)ox, 0.5f), p.ws), 0.5f) : __fmul_rn((float)ox, p.ws);
    int y0 = (int)floorf(iy), y1 = (int)ceilf(iy), x0 = (int)floorf(ix), x1 = (int)ceilf(ix);
    y0 = y0 < 0 ? 0 : y0; x0 = x0 < 0 ? 0 : x0;
    y1 = y1 > p.H - 1 ? p.H - 1 : y1; x1 = x1 > p.W - 1 ? p.W - 1 : x1;
    const float fy = __fsub_rn(iy, (float)y0), fx = __fsub_rn(ix, (float)x0);
    const float gy = __fsub_rn(1.0f, fy), gx = __fsub_rn(1.0f, fx);
    auto at = [&](int yy, int xx) { return (float)px[((size_t)yy * p.W + xx) * p.C + c]; };
    float v = __fmul_rn(__fmul_rn(at(y0, x0), gy), gx);
    v = __fadd_rn(v, __fmul_rn(__fmul_rn(at(y1, x0), fy), gx));
    v = __fadd_rn(v, __fmul_rn(__fmul_rn(at(y0, x1), gy), fx));
    v = __fadd_rn(v, __fmul_rn(__fmul_rn(at(y1, x1), fy), fx));
    const float r = floorf(__fadd_rn(v, 0.5f));
    py[t] = (uint8_t)apply_post(p.po, r < 0.0f ? 0 : (r > 255.0f ? 255 : (int)r), blockIdx.y, t);
}
// RESIZE_BILINEAR of int8: not the float interpolation above but TFLite's integer kernel - positions and weights in 10-bit fixed
// point (hs10 / ws10: the plan's steps), the four products summed in 64 bits and rounded half away from zero at bit 20; `/` here
// truncates toward zero as the definition's does. Input and output share scale and zero point.
__global__ __launch_bounds__(256) void tfl_resize_bilinear_s8(const ResizeQ p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.Ho * p.Wo * p.C) return;
    const uint8_t* const px = p.x + (size_t)blockIdx.y * p.H * p.W * p.C;
    uint8_t* const py = p.y + blockIdx.y * p.ys;
    const int c = t % p.C, r0 = t / p.C, ox = r0 % p.Wo, oy = r0 / p.Wo;
    const int iy = p.half_pixel ? oy * p.hs10 + p.hs10 / 2 - (1 << 9) : oy * p.hs10;
    const int ix = p.half_pixel ? ox * p.ws10 + p.ws10 / 2 - (1 << 9) : ox * p.ws10;
    int y0 = iy / (1 << 10), y1 = (iy + (1 << 10) - 1) / (1 << 10), x0 = ix / (1 << 10), x1 = (ix + (1 << 10) - 1) / (1 << 10);
    // (the definition bounds y0 below and y1 above only; a step rounded up can carry y0 past the last row when Ho is in the thousands
    // and H is not - bounded here, and in the tests' reference, so that nothing is read outside the image)
    y0 = y0 < 0 ? 0 : (y0 > p.H - 1 ? p.H - 1 : y0); x0 = x0 < 0 ? 0 : (x0 > p.W - 1 ? p.W - 1 : x0);
    y1 = y1 > p.H - 1 ? p.H - 1 : y1; x1 = x1 > p.W - 1 ? p.W - 1 : x1;
    const long long fy = iy - (1 << 10) * y0, fx = ix - (1 << 10) * x0, gy = (1 << 10) - fy, gx = (1 << 10) - fx;
    auto at = [&](int yy, int xx) { return (long long)ldq<true>(px + ((size_t)yy * p.W + xx) * p.C + c); };
    const long long v = at(y0, x0) * gy * gx + at(y1, x0) * fy * gx + at(y0, x1) * gy * fx + at(y1, x1) * fy * fx;
    const int q = (int)(int8_t)((v + (v > 0 ? (1ll << 19) : -(1ll << 19))) / (1ll << 20));
    py[t] = (uint8_t)apply_post<true>(p.po, q, blockIdx.y, t);
}
__global__ __launch_bounds__(256) void tfl_concat_part(const CatQ p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.outer * p.inner * p.esz) return;
    const long long e = t / p.esz;
    const int b = (int)(t - e * p.esz);
    const long long o = e / p.inner;
    const int i = (int)(e - o * p.inner);
    const long long dst = ((o * p.row) + p.off + i) * p.esz + b;
    if (p.rescale) {
        const float v = __fadd_rn(__fmul_rn((float)p.x[t], p.sc), p.bias);
        const float r = v >= 0.0f ? floorf(__fadd_rn(v, 0.5f)) : ceilf(__fsub_rn(v, 0.5f));
        p.y[dst] = (uint8_t)q_clamp((int)r + p.zo, 0, 255);
    } else p.y[dst] = p.x[t];
}

inline unsigned nblk(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

namespace yh {

ConvU8Kernel conv_u8_kernel(const ConvQ& p, bool dot) {
    if (p.wsum) return p.Ci % 16 == 0 ? CONV_U8_DOT4 : CONV_U8_DOT1;
    return dot && p.kh * p.kw * p.Ci <= kPx8MaxK ? CONV_U8_PX8 : CONV_U8_SCALAR;
}
void launch_conv_u8(const ConvQ& p, bool dot, unsigned nb, hipStream_t s) {
    const ConvU8Kernel k = conv_u8_kernel(p, dot);
    if (k == CONV_U8_DOT4 || k == CONV_U8_DOT1) {
        const dim3 grid((unsigned)(((long long)p.Ho * p.Wo + 63) / 64), (unsigned)((p.Co + 7) / 8), nb);
        if (k == CONV_U8_DOT4) hipLaunchKernelGGL(tfl_conv_u8_dot<4>, grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL(tfl_conv_u8_dot<1>, grid, dim3(64), 0, s, p);
    }
    else if (k == CONV_U8_PX8) {
        const dim3 grid((unsigned)(((long long)p.Ho * p.Wo + 255) / 256), (unsigned)((p.Co + 7) / 8), nb);
        if (p.sgn) hipLaunchKernelGGL((tfl_conv_u8_px8<0, 0, 0, true>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((tfl_conv_u8_px8<0, 0, 0, false>), grid, dim3(256), 0, s, p);   // (the <3, 3, 3> form - all 27 input bytes asked for up front - measured 13.0 us against 10.6)
    }
    else hipLaunchKernelGGL(p.sgn ? tfl_conv_s8 : tfl_conv_u8, dim3(nblk((long long)p.Ho * p.Wo * p.Co), nb), dim3(256), 0, s, p);
}
bool dwconv_u8_takes_c4(const ConvQ& p, bool dot) {
    return dot && p.dm == 1 && p.kh == 3 && p.kw == 3 && p.Co % 4 == 0 && (((size_t)p.x | (size_t)p.w) & 3) == 0;
}
void launch_dwconv_u8(const ConvQ& p, bool dot, unsigned nb, hipStream_t s) {
    if (dwconv_u8_takes_c4(p, dot))
        hipLaunchKernelGGL((p.sgn ? tfl_dwconv_s8_c4<3, 3> : tfl_dwconv_u8_c4<3, 3>), dim3(nblk((long long)p.Ho * p.Wo * (p.Co >> 2)), nb), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(p.sgn ? tfl_dwconv_s8 : tfl_dwconv_u8, dim3(nblk((long long)p.Ho * p.Wo * p.Co), nb), dim3(256), 0, s, p);
}
void launch_conv_i8_mfma(const ConvI8& q, hipStream_t s) { hipLaunchKernelGGL(q.sgn ? tfl_conv_s8_mfma : tfl_conv_i8_mfma, dim3((unsigned)((q.M + 63) / 64), (unsigned)((q.Co + 63) / 64)), dim3(256), 0, s, q); }

// The row of a convolution of n = taps x 64-channel chunks k-steps: the one-pass row of exactly n steps and this extent; else a
// looped row - where one-pass rows of n steps exist for other extents only, the deepest ring that n fills, otherwise the ring that
// pads n least (the steps are rounded up to a multiple of D), the deepest among equals; a ring deeper than n is never taken unless
// all are.
int conv_i8_direct_form(int kh, int kw, int Ci) {
    const int n = kh * kw * ((Ci + 63) / 64);
    const int kk = kh == 1 && kw == 1 ? 1 : (kh == 3 && kw == 3 ? 3 : 0);
    bool exact = false;
    int shallowest = -1, deepest = -1, least = -1, pad = 1 << 30;   // looped rows: of all / of those with D <= n / the least padding's
    for (int i = 0; i < kDirectFormCount; ++i) {
        const DirectForm& f = kDirectForms[i];
        if (f.once) {
            if (f.D == n && f.KK == kk) return i;
            exact = exact || f.D == n;
            continue;
        }
        if (shallowest < 0 || f.D < kDirectForms[shallowest].D) shallowest = i;
        if (f.D > n) continue;
        if (deepest < 0 || f.D > kDirectForms[deepest].D) deepest = i;
        const int q = (n + f.D - 1) / f.D * f.D - n;
        if (q < pad || (q == pad && f.D > kDirectForms[least].D)) { pad = q; least = i; }
    }
    const int fits = exact ? deepest : least;
    return fits >= 0 ? fits : shallowest;
}
int conv_i8_direct_form_count() { return kDirectFormCount; }
void conv_i8_direct_form_row(int i, int* D, int* once, int* KK) { *D = kDirectForms[i].D; *once = kDirectForms[i].once ? 1 : 0; *KK = kDirectForms[i].KK; }
// Which int8 MFMA launches take the register-fed kernel: every one whose input channels the LDS tiles cannot take (Ci % 64 != 0), and
// the small ones - up to 2048 waves (8 per CU), or up to 8 k-steps. A large layer with a long K (the protonet's 3x3 x 128 channels
// at 56 x 56 x 2 images: 3136 waves of 18 steps) re-reads its operands once per 16 x 16 tile and measured 26.0 us against 14.2 on
// the 64 x 64 LDS tiles.
bool conv_i8_direct_pays(const ConvI8& q) {
    if (q.Ci % 64 != 0) return true;
    const long long waves = (long long)((q.M + 15) / 16) * ((q.Co + 15) / 16);
    return waves <= 2048 || q.kh * q.kw * (q.Ci / 64) <= 8;
}
void launch_conv_i8_direct(int form, const ConvI8& q, hipStream_t s) {
    hipLaunchKernelGGL(q.sgn ? kDirectForms[form].single_s8 : kDirectForms[form].single, dim3((unsigned)((q.M + 15) / 16), (unsigned)((q.Co + 15) / 16)), dim3(64), 0, s, q);
}
void launch_conv_i8_direct_group(int form, bool sgn, const ConvI8* probs, const int* tile_start, int nprob, int tiles, hipStream_t s) {
    hipLaunchKernelGGL(sgn ? kDirectForms[form].group_s8 : kDirectForms[form].group, dim3((unsigned)tiles), dim3(64), 0, s, probs, tile_start, nprob);
}

void launch_add_u8(const AddQ& p, unsigned nb, hipStream_t s) { AddQ q = p; q.n *= nb; hipLaunchKernelGGL(q.sgn ? tfl_add_s8 : tfl_add_u8, dim3(nblk(q.n)), dim3(256), 0, s, q); }
void launch_requant_u8(const uint8_t* x, uint8_t* y, long long n, int zi, int zo, int m, int sh, int lo, int hi, hipStream_t s, bool sgn) {
    hipLaunchKernelGGL(sgn ? tfl_requant_s8 : tfl_requant_u8, dim3(nblk(n)), dim3(256), 0, s, x, y, n, zi, zo, m, sh, lo, hi);
}
void launch_quantize_f32(const float* x, uint8_t* y, long long n, float scale, int zo, hipStream_t s, bool sgn) { hipLaunchKernelGGL(sgn ? tfl_quantize_f32_s8 : tfl_quantize_f32, dim3(nblk(n)), dim3(256), 0, s, x, y, n, scale, zo); }
void launch_dequantize_u8(const uint8_t* x, float* y, long long n, float scale, int z, hipStream_t s, bool sgn) { hipLaunchKernelGGL(sgn ? tfl_dequantize_s8 : tfl_dequantize_u8, dim3(nblk(n)), dim3(256), 0, s, x, y, n, scale, z); }
void launch_lut_u8(const uint8_t* x, uint8_t* y, long long n, const uint8_t* lut, hipStream_t s) { hipLaunchKernelGGL(tfl_lut_u8, dim3(nblk(n)), dim3(256), 0, s, x, y, n, lut); }
void launch_pad_u8(const PadQ& p, unsigned nb, hipStream_t s) {
    PadQ q = p;
    q.id[0] *= (int)nb; q.od[0] *= (int)nb;
    hipLaunchKernelGGL(tfl_pad_u8, dim3(nblk((long long)q.od[0] * q.od[1] * q.od[2] * q.od[3])), dim3(256), 0, s, q);
}
void launch_resize_bilinear_u8(const ResizeQ& p, unsigned nb, hipStream_t s) { hipLaunchKernelGGL(p.sgn ? tfl_resize_bilinear_s8 : tfl_resize_bilinear_u8, dim3(nblk((long long)p.Ho * p.Wo * p.C), nb), dim3(256), 0, s, p); }
void launch_concat_part(const CatQ& p, unsigned nb, hipStream_t s) { CatQ c = p; c.outer *= nb; hipLaunchKernelGGL(tfl_concat_part, dim3(nblk(c.outer * c.inner * c.esz)), dim3(256), 0, s, c); }
void launch_copy_bytes(const uint8_t* x, uint8_t* y, long long n, hipStream_t s) { hipLaunchKernelGGL(tfl_copy_bytes, dim3(nblk((n >> 4) + 16)), dim3(256), 0, s, x, y, n); }

}  // namespace yh
