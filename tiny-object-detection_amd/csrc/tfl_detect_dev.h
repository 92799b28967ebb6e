// tfl_detect_dev.h — device helpers of tfl_detect.hip, the only unit that includes this file. box_iou and radix_select_kth restate
// detect.hip's (same operations, same order): detect.hip itself is left byte for byte as it is, so nothing is
// shared with it through a template or a header it would have to include.
#pragma once
#include "tfl_detect.h"
#include "yh_internal.h"

namespace yh {

// rule 1: the value of a quantised element (raw: the byte, zero- or sign-extended)
__device__ __forceinline__ float td_deq(const TflHead& t, int raw) { return __fmul_rn((float)(raw - t.zp), t.scale); }
__device__ __forceinline__ int td_raw(int kind, unsigned byte) { return kind == TQ_I8 ? (int)(int8_t)byte : (int)byte; }

__device__ __forceinline__ float td_box_iou(const float4 a, const float4 b) {
    float iw = __fsub_rn(fminf(a.z, b.z), fmaxf(a.x, b.x));
    float ih = __fsub_rn(fminf(a.w, b.w), fmaxf(a.y, b.y));
    iw = iw < 0.0f ? 0.0f : iw;
    ih = ih < 0.0f ? 0.0f : ih;
    const float inter = __fmul_rn(iw, ih);
    const float aa = __fmul_rn(__fsub_rn(a.z, a.x), __fsub_rn(a.w, a.y));
    const float ab = __fmul_rn(__fsub_rn(b.z, b.x), __fsub_rn(b.w, b.y));
    const float uni = __fsub_rn(__fadd_rn(aa, ab), inter);
    return uni > 0.0f ? __fdiv_rn(inter, uni) : 0.0f;
}

// Exact k-th largest of n UNIQUE 64-bit keys by MSB-first radix select: 8 passes of a 256-bin LDS histogram over the keys that
// still match the prefix; the bin holding the k-th key is found by one wave. Every thread of the workgroup must call it.
template <int NT, class KeyFn>
__device__ unsigned long long td_radix_select_kth(KeyFn key_of, int n, int k, int* hist, int* sh) {
    const int tid = threadIdx.x;
    unsigned long long prefix = 0, mask = 0;
    int kk = k;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += NT) hist[i] = 0;
        __syncthreads();
        int run_bin = -1, run_cnt = 0;   // (run-length aggregation per lane: the high bytes of score keys take two or three values)
        for (int i = tid; i < n; i += NT) {
            const unsigned long long key = key_of(i);
            if ((key & mask) == prefix) {
                const int bin = (int)((key >> shift) & 255ull);
                if (bin == run_bin) ++run_cnt;
                else { if (run_cnt) atomicAdd(&hist[run_bin], run_cnt); run_bin = bin; run_cnt = 1; }
            }
        }
        if (run_cnt) atomicAdd(&hist[run_bin], run_cnt);
        __syncthreads();
        if (tid < 64) {
            const int h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
            const int mine = h0 + h1 + h2 + h3;
            int incl = mine;  // inclusive suffix sum over lanes >= tid
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_down(incl, d);
                incl += (tid + d < 64) ? o : 0;
            }
            const int above = incl - mine;
            if (above < kk && kk <= incl) {  // exactly one lane
                int c = above, bsel;
                if (c + h3 >= kk) bsel = 3;
                else { c += h3; if (c + h2 >= kk) bsel = 2; else { c += h2; if (c + h1 >= kk) bsel = 1; else { c += h1; bsel = 0; } } }
                sh[0] = 4 * tid + bsel;
                sh[1] = kk - c;
            }
        }
        __syncthreads();
        prefix |= (unsigned long long)(unsigned)sh[0] << shift;
        mask |= 0xFFull << shift;
        kk = sh[1];
        __syncthreads();
    }
    return prefix;
}

}  // namespace yh
