// refpath_dev.h - the Triangle resampler's arithmetic (image 0.24.1's separable f32 algorithm, one explicit round-to-nearest op
// per operator, bit-identical to oracle/orc_ref.c), shared by refpath.hip (one frame: resize_v / resize_h) and classify_batch.hip
// (n frames: resize_tables computes every window once with these, the batch kernels read the tables). There is one definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace yh {

struct SampleWin { int left, n; float inputc, sratio, sum; };

__device__ __forceinline__ float tri_w(int i, float inputc, float sratio) {
    const float x = __fdiv_rn(__fsub_rn((float)i, inputc), sratio);
    const float a = fabsf(x);
    return a < 1.0f ? __fsub_rn(1.0f, a) : 0.0f;
}

__device__ __forceinline__ SampleWin sample_window(int out_i, int in_size, int out_size) {
    SampleWin s;
    const float ratio = __fdiv_rn((float)in_size, (float)out_size);
    s.sratio = ratio < 1.0f ? 1.0f : ratio;
    const float support = __fmul_rn(1.0f, s.sratio);
    float inputc = __fmul_rn(__fadd_rn((float)out_i, 0.5f), ratio);
    long long left = (long long)floorf(__fsub_rn(inputc, support));
    left = left < 0 ? 0 : (left > in_size - 1 ? in_size - 1 : left);
    long long right = (long long)ceilf(__fadd_rn(inputc, support));
    right = right < left + 1 ? left + 1 : (right > in_size ? in_size : right);
    s.inputc = __fsub_rn(inputc, 0.5f);
    s.left = (int)left;
    s.n = (int)(right - left);
    float sum = 0.0f;
    for (int i = 0; i < s.n; ++i) sum = __fadd_rn(sum, tri_w(s.left + i, s.inputc, s.sratio));
    s.sum = sum;
    return s;
}

__device__ __forceinline__ uint32_t to_u8(float v) {
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    return (uint32_t)roundf(v);
}

}  // namespace yh
