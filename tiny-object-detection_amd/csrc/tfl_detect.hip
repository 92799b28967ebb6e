// tfl_detect.hip — the detection tail on a TFLite model's own output tensors (DESIGN.md section 11 "TFLite detections").
//
// detect.hip's four stages for heads that lie as a .tflite model leaves them: loc [n][P][4], conf [n][P][C], mask [n][P][32] and
// proto [n][hp][wp][32], each uint8, int8 or float32 with one scale and zero point, read where they lie and dequantised in the
// register (value = (float)(q - z) * scale, one f32 multiply). Scores, candidates, decode, NMS, ranking and crop windows are
// oracle/orc_detect.c on those values, operation for operation; priors are indexed by the prior (no three anchors per cell, no
// assumption about P). The mask bit of two quantised tensors is the sign of the exact integer sum
// S = sum_k (proto_q[k] - z_p)(mask_q[k] - z_m); with a float32 tensor among the two it is the oracle's fmaf chain.
//
//   K1q tfl_det_softmax_cand : 128 priors per workgroup, one lane per prior. Their conf rows are one contiguous run of bytes: it is
//                              fetched with coalesced dword loads from the dword below its first byte and re-pitched into LDS.
//   K2q tfl_det_class_nms    : detect.hip's K2; a selected prior's four loc values are one dword (quantised) or one float4.
//   K3q tfl_det_frame_top    : detect.hip's K3; writes a kept detection's coefficients as 32 bytes + their sum, or as 32 f32.
//   K4q tfl_det_masks_q      : v_dot4 on 8 + 8 dwords per (pixel, detection); tfl_det_masks_f: the fmaf chain.
#include "tfl_detect_dev.h"

namespace yh {

// K1q. LDS row pitch: PD dwords with PD odd (bytes: 4 PD >= C; f32: PD >= C). Lane l reads byte 4 PD l + c (or dword PD l + c):
// a ds_read_b32 is served in two groups of 32 lanes and the bank is (a / 4) mod 32 (MI355X_MICROARCH.md, LDS table), so the 32 lanes
// of a group sit on dwords PD l + const, an odd multiple apart: 32 different banks, no conflict. The table lists no ds_read_u8: the
// byte read is ASSUMED to bank by its dword as the dword read does (not measured).
#define TD_K1_PRIORS 128
template <int KIND>
__global__ __launch_bounds__(TD_K1_PRIORS) void tfl_det_softmax_cand(const TflDetectParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t zw[];   // [128][PD]
    constexpr int ESZ = KIND == TQ_F32 ? 4 : 1;
    const int C = p.C, tid = threadIdx.x, b = blockIdx.y;
    const int p0 = blockIdx.x * TD_K1_PRIORS;
    const int np = p.P - p0 < TD_K1_PRIORS ? p.P - p0 : TD_K1_PRIORS;
    const int PD = ((C * ESZ + 3) / 4) | 1;
    // the rows of priors p0 .. p0 + np - 1 of image b: nbytes bytes from address a0, which need not be dword aligned (C = 81)
    const unsigned long long a0 = (unsigned long long)p.conf.p + ((unsigned long long)b * (unsigned long long)p.conf.stride + (unsigned long long)p0 * C) * ESZ;
    const uint32_t* src = (const uint32_t*)(a0 & ~3ull);
    const int sh = (int)(a0 & 3ull), nbytes = np * C * ESZ, ndw = (sh + nbytes + 3) / 4;
    if (KIND == TQ_F32) {
        for (int i = tid; i < ndw; i += TD_K1_PRIORS) { const int r = i / C, c = i - r * C; zw[r * PD + c] = src[i]; }
    } else {
        uint8_t* zb = (uint8_t*)zw;
        for (int i = tid; i < ndw; i += TD_K1_PRIORS) {
            const uint32_t v = src[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * i + e - sh;
                if (j >= 0 && j < nbytes) { const int r = j / C, c = j - r * C; zb[r * PD * 4 + c] = (uint8_t)(v >> (8 * e)); }
            }
        }
    }
    __syncthreads();
    const bool valid = tid < np;
    const int pr = p0 + tid;
    auto z = [&](int c) -> float {   // dequantise on the read
        if (KIND == TQ_F32) return __uint_as_float(zw[tid * PD + c]);
        return td_deq(p.conf, td_raw(KIND, ((const uint8_t*)zw)[tid * PD * 4 + c]));
    };
    float m = 0.0f, s = 1.0f;
    if (valid) {
        m = z(0);
        for (int c = 1; c < C; ++c) { const float v = z(c); m = v > m ? v : m; }
        s = 0.0f;
        for (int c = 0; c < C; ++c) s = __fadd_rn(s, spec_expf(__fsub_rn(z(c), m)));
    }
    // wave-aggregated append: one atomic per (wave, class) that has any candidate. The exponential is formed again (the same
    // operation on the same operands: the same bits) - a byte row has no room to park it.
    const int lane = tid & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int c = 1; c < C; ++c) {
        const float pc = valid ? __fdiv_rn(spec_expf(__fsub_rn(z(c), m)), s) : 0.0f;
        const bool hit = pc > p.conf_thresh;
        const unsigned long long mask = __ballot(hit);
        if (mask == 0ull) continue;  // wave-uniform
        const int list = b * (C - 1) + (c - 1);
        int base = 0;
        if (lane == __ffsll((long long)mask) - 1) base = atomicAdd(&p.cls_count[list], __popcll(mask));
        base = __shfl(base, __ffsll((long long)mask) - 1);
        // (a list holds at most P entries - every prior once; a stale count of an abandoned call must not carry the store past the list)
        const int slot = base + __popcll(mask & lt);
        if (hit && slot < p.P) p.cand[(long long)list * p.P + slot] = make_uint2(__float_as_uint(pc), (unsigned)pr);
    }
}

#define TD_K2_STAGE 4096

// K2q: one workgroup per (image, class). detect.hip's det_class_nms with the loc values of a selected prior read from loc[n][P][4].
__global__ __launch_bounds__(256) void tfl_det_class_nms(const TflDetectParams p) {
    __shared__ unsigned long long stage[TD_K2_STAGE];   // candidate keys (when they fit)
    __shared__ unsigned long long sel[kTdTopkMax];      // the K selected keys, then sorted
    __shared__ unsigned long long sorted[kTdTopkMax];
    __shared__ float4 sel_box[kTdTopkMax];
    __shared__ int supp[kTdTopkMax];
    __shared__ int hist[256];
    __shared__ int sh[4];
    __shared__ int sh_nc;
    const int list = blockIdx.x;  // b*(C-1) + c
    const int b = list / (p.C - 1);
    const int tid = threadIdx.x;
    // this workgroup is the one consumer of its list's counter: it takes the count and leaves zero for the next call
    if (tid == 0) { sh_nc = p.cls_count[list]; p.cls_count[list] = 0; }
    __syncthreads();
    const int nc = sh_nc < p.P ? sh_nc : p.P;
    const uint2* cand = p.cand + (long long)list * p.P;
    const int K = nc < p.top_k ? nc : p.top_k;
    const long long so = (long long)list * p.top_k;
    if (nc == 0) {  // uniform
        for (int j = tid; j < p.top_k; j += 256) p.surv_score[so + j] = -1.0f;
        return;
    }
    // key = score bits (positive float: monotone) : ~prior  -> larger key = better, keys unique
    const bool staged = nc <= TD_K2_STAGE;
    if (staged) {
        for (int i = tid; i < nc; i += 256) { const uint2 c = cand[i]; stage[i] = ((unsigned long long)c.x << 32) | (unsigned long long)(0xFFFFFFFFu - c.y); }
    }
    if (tid == 0) sh[2] = 0;
    __syncthreads();
    auto key_of = [&](int i) -> unsigned long long {
        if (staged) return stage[i];
        const uint2 c = cand[i];
        return ((unsigned long long)c.x << 32) | (unsigned long long)(0xFFFFFFFFu - c.y);
    };
    unsigned long long T = 0;
    if (nc > p.top_k) T = td_radix_select_kth<256>(key_of, nc, K, hist, sh);
    for (int i = tid; i < nc; i += 256) {
        const unsigned long long key = key_of(i);
        if (key >= T) sel[atomicAdd(&sh[2], 1)] = key;  // exactly K keys pass
    }
    __syncthreads();
    if (tid < K) {  // order the K selected keys by counting
        const unsigned long long me = sel[tid];
        int rank = 0;
        for (int j = 0; j < K; ++j) rank += sel[j] > me ? 1 : 0;
        sorted[rank] = me;
    }
    __syncthreads();
    if (tid < K) {
        const int pr = (int)(0xFFFFFFFFu - (unsigned)(sorted[tid] & 0xFFFFFFFFull));
        const long long le = (long long)b * p.loc.stride + (long long)pr * 4;   // element index of the prior's four values
        float l0, l1, l2, l3;
        if (p.loc.kind == TQ_F32) {
            const float4 v = *(const float4*)((const float*)p.loc.p + le);
            l0 = v.x; l1 = v.y; l2 = v.z; l3 = v.w;
        } else {
            const uint32_t v = *(const uint32_t*)((const uint8_t*)p.loc.p + le);
            l0 = td_deq(p.loc, td_raw(p.loc.kind, v & 255u));
            l1 = td_deq(p.loc, td_raw(p.loc.kind, (v >> 8) & 255u));
            l2 = td_deq(p.loc, td_raw(p.loc.kind, (v >> 16) & 255u));
            l3 = td_deq(p.loc, td_raw(p.loc.kind, v >> 24));
        }
        const float4 q = *(const float4*)(p.priors + (long long)pr * 4);
        const float cx = __fadd_rn(q.x, __fmul_rn(__fmul_rn(l0, 0.1f), q.z));
        const float cy = __fadd_rn(q.y, __fmul_rn(__fmul_rn(l1, 0.1f), q.w));
        const float w = __fmul_rn(q.z, spec_expf(__fmul_rn(l2, 0.2f)));
        const float h = __fmul_rn(q.w, spec_expf(__fmul_rn(l3, 0.2f)));
        float4 bx;
        bx.x = __fsub_rn(cx, __fmul_rn(w, 0.5f));
        bx.y = __fsub_rn(cy, __fmul_rn(h, 0.5f));
        bx.z = __fadd_rn(w, bx.x);
        bx.w = __fadd_rn(h, bx.y);
        sel_box[tid] = bx;
    }
    __syncthreads();
    // Fast-NMS: box j survives iff no better-ranked box i < j overlaps it by more than the threshold; the K (K - 1) / 2 pairs are
    // dealt evenly over the workgroup (rows j and K - j folded into one row of K)
    for (int j = tid; j < kTdTopkMax; j += 256) supp[j] = 0;
    __syncthreads();
    {
        const int half_rows = (K - 1) / 2, folded = half_rows * K;
        for (int t = tid; t < folded; t += 256) {
            const int r = t / K, c = t - r * K, j0 = r + 1;
            const int j = c < j0 ? j0 : K - j0, i = c < j0 ? c : c - j0;
            if (td_box_iou(sel_box[i], sel_box[j]) > p.nms_thresh) supp[j] = 1;
        }
        if ((K & 1) == 0 && K >= 2) {   // the unpaired middle row
            const int j = K / 2;
            for (int i = tid; i < j; i += 256)
                if (td_box_iou(sel_box[i], sel_box[j]) > p.nms_thresh) supp[j] = 1;
        }
    }
    __syncthreads();
    for (int j = tid; j < p.top_k; j += 256) {
        float out = -1.0f;
        if (j < K && supp[j] == 0) {
            out = __uint_as_float((unsigned)(sorted[j] >> 32));
            p.surv_prior[so + j] = (int)(0xFFFFFFFFu - (unsigned)(sorted[j] & 0xFFFFFFFFull));
            *(float4*)(p.surv_box + (so + j) * 4) = sel_box[j];
        }
        p.surv_score[so + j] = out;
    }
}

// K3q: one workgroup per image: survivors -> exact top max_dets in (score desc, slot asc) order, their crop windows and coefficients.
__global__ __launch_bounds__(1024) void tfl_det_frame_top(const TflDetectParams p) {
    __shared__ unsigned long long keys[kTdSlotsMax];
    __shared__ unsigned long long sel[kTdDetsMax];
    __shared__ int hist[256];
    __shared__ int sh[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int NS = (p.C - 1) * p.top_k;
    if (tid == 0) { sh[2] = 0; sh[3] = 0; }
    __syncthreads();
    const float* ss = p.surv_score + (long long)b * NS;
    for (int i = tid; i < NS; i += 1024) {
        const float s = ss[i];
        if (s >= 0.0f) keys[atomicAdd(&sh[2], 1)] = ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
    }
    __syncthreads();
    const int nv = sh[2];
    const int K = nv < p.max_dets ? nv : p.max_dets;
    if (tid == 0) p.det_count[b] = K;
    if (nv == 0) return;
    unsigned long long T = 0;
    if (nv > p.max_dets) T = td_radix_select_kth<1024>([&](int i) { return keys[i]; }, nv, K, hist, sh);
    for (int i = tid; i < nv; i += 1024)
        if (keys[i] >= T) sel[atomicAdd(&sh[3], 1)] = keys[i];
    __syncthreads();
    if (tid < K) {
        const unsigned long long me = sel[tid];
        int rank = 0;
        for (int j = 0; j < K; ++j) rank += sel[j] > me ? 1 : 0;
        const int ie = (int)(0xFFFFFFFFu - (unsigned)(me & 0xFFFFFFFFull));
        const long long slot = (long long)b * NS + ie;
        yh_detection d;
        d.class_id = ie / p.top_k;
        d.prior = p.surv_prior[slot];
        d.score = __uint_as_float((unsigned)(me >> 32));
        const float4 bx = *(const float4*)(p.surv_box + slot * 4);
        d.box[0] = bx.x; d.box[1] = bx.y; d.box[2] = bx.z; d.box[3] = bx.w;
        const long long di = (long long)b * p.max_dets + rank;
        p.dets[di] = d;
        const float fw = (float)p.wp, fh = (float)p.hp;
        const float x1 = __fmul_rn(bx.x, fw), x2 = __fmul_rn(bx.z, fw);
        const float y1 = __fmul_rn(bx.y, fh), y2 = __fmul_rn(bx.w, fh);
        float xa = __fsub_rn(fminf(x1, x2), 1.0f), xb = __fadd_rn(fmaxf(x1, x2), 1.0f);
        float ya = __fsub_rn(fminf(y1, y2), 1.0f), yb = __fadd_rn(fmaxf(y1, y2), 1.0f);
        xa = xa < 0.0f ? 0.0f : xa;
        ya = ya < 0.0f ? 0.0f : ya;
        xb = xb > fw ? fw : xb;
        yb = yb > fh ? fh : yb;
        *(float4*)(p.det_crop + di * 4) = make_float4(xa, xb, ya, yb);
        // the detection's 32 coefficients, dense, for the mask kernel
        const long long me0 = (long long)b * p.mask.stride + (long long)d.prior * 32;   // element index
        if (p.int_mask) {
            // rule 3: the raw bytes, in the uint8 domain (an int8 byte q becomes q + 128 by flipping its top bit), and their sum
            const uint32_t* src = (const uint32_t*)((const uint8_t*)p.mask.p + me0);
            const uint32_t flip = p.mask.kind == TQ_I8 ? 0x80808080u : 0u;
            uint32_t* co = (uint32_t*)p.det_coef + di * 8;
            uint32_t v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = src[q] ^ flip;
            unsigned cs = 0u;
#pragma unroll
            for (int q = 0; q < 8; ++q) { co[q] = v[q]; cs = __builtin_amdgcn_udot4(v[q], 0x01010101u, cs, false); }
            p.det_csum[di] = (int)cs;
        } else {
            float* co = (float*)p.det_coef + di * 32;
            if (p.mask.kind == TQ_F32) {
                const float* src = (const float*)p.mask.p + me0;
                for (int k = 0; k < 32; ++k) co[k] = src[k];
            } else {
                const uint32_t* src = (const uint32_t*)((const uint8_t*)p.mask.p + me0);
                for (int q = 0; q < 8; ++q) {
                    const uint32_t v = src[q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) co[q * 4 + e] = td_deq(p.mask, td_raw(p.mask.kind, (v >> (8 * e)) & 255u));
                }
            }
        }
    }
}

// What K4q's two forms share: which detections can touch this workgroup's 256 pixels (rows y_lo .. y_hi of the prototype map), and
// the store. A lane decides one pixel of one detection; the wave's 64 decisions are one ballot, and lane (j, q) = (lane >> 4,
// lane & 15) writes pixels 4 q .. 4 q + 3 of detection d + j as ONE dword - when hp * wp is a multiple of 4, so that a dword is
// wholly inside one mask and aligned. A TFLite model's prototype map is arbitrary: any other hp * wp takes the byte path, a
// byte per lane and detection.
struct TdMaskBlock {
    float4* crop; unsigned* rel;
    int b, tid, nd, npx, px, lane, d0, d1;
    bool live; float fx, fy;
};
__device__ __forceinline__ void td_mask_block(const TflDetectParams& p, TdMaskBlock& k) {
    k.b = blockIdx.y; k.tid = threadIdx.x;
    k.nd = p.det_count[k.b];
    if (k.tid < kTdDetsMax / 32) k.rel[k.tid] = 0u;
    __syncthreads();
    k.npx = p.hp * p.wp;
    const int p_lo = blockIdx.x * 256, p_hi = min(p_lo + 255, k.npx - 1);
    const float y_lo = (float)(p_lo / p.wp), y_hi = (float)(p_hi / p.wp);
    for (int d = k.tid; d < k.nd; d += 256) {
        const float4 c = *(const float4*)(p.det_crop + ((long long)k.b * p.max_dets + d) * 4);
        k.crop[d] = c;
        if (y_hi >= c.z && y_lo < c.w) atomicOr(&k.rel[d >> 5], 1u << (d & 31));   // some row y in [y_lo, y_hi] has c.z <= y < c.w
    }
    __syncthreads();
    k.px = blockIdx.x * 256 + k.tid;
    k.live = k.px < k.npx;
    const int y = k.px / p.wp, x = k.px - y * p.wp;
    k.fx = (float)x; k.fy = (float)y;
    k.lane = k.tid & 63;
    // small batches: the detections are dealt over gridDim.z groups (whole groups of four detections: a group is one store)
    const int per = ((p.max_dets + (int)gridDim.z - 1) / (int)gridDim.z + 3) & ~3;
    k.d0 = (int)blockIdx.z * per;
    k.d1 = k.d0 + per < k.nd ? k.d0 + per : k.nd;
}
__device__ __forceinline__ void td_mask_store(const TflDetectParams& p, const TdMaskBlock& k, int d, const unsigned long long m[4]) {
    uint8_t* mo = p.masks + (long long)k.b * p.max_dets * k.npx;
    if ((k.npx & 3) == 0) {   // (uniform)
        const int lj = k.lane >> 4, lq = k.lane & 15;
        const int at = k.px - k.lane + 4 * lq;
        const unsigned long long mine = lj == 0 ? m[0] : (lj == 1 ? m[1] : (lj == 2 ? m[2] : m[3]));
        const unsigned nib = (unsigned)(mine >> (4 * lq)) & 15u;
        if (at < k.npx && d + lj < k.d1) *(unsigned*)(mo + (long long)(d + lj) * k.npx + at) = (nib * 0x00204081u) & 0x01010101u;
    } else if (k.live) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (d + j < k.d1) mo[(long long)(d + j) * k.npx + k.px] = (uint8_t)((m[j] >> k.lane) & 1ull);
    }
}

// K4q, both tensors quantised (rule 3). A pixel's 32 prototype bytes are 8 dwords in registers, a detection's 32 coefficient bytes
// 8 dwords in LDS (uniform per wave: broadcast reads); both are in the uint8 domain (p' = p ^ 0x80 for int8, z' = z + 128), so
//   S = sum p' c' - z'_m sum p' - z'_p sum c' + 32 z'_p z'_m      (sum p' once per pixel, sum c' once per detection: K3q)
// with 8 v_dot4_u32_u8 per (pixel, detection); every term is below 2^22, the sum exact in 32 bits.
__global__ __launch_bounds__(256) void tfl_det_masks_q(const TflDetectParams p) {
    __shared__ uint32_t coef[kTdDetsMax * 8];
    __shared__ int csum[kTdDetsMax];
    __shared__ float4 crop[kTdDetsMax];
    __shared__ unsigned rel[kTdDetsMax / 32];
    TdMaskBlock k; k.crop = crop; k.rel = rel;
    td_mask_block(p, k);   // (its barriers order the loads below too)
    for (int i = k.tid; i < k.nd * 8; i += 256) coef[i] = ((const uint32_t*)p.det_coef)[(long long)k.b * p.max_dets * 8 + i];   // (written by K3q)
    for (int i = k.tid; i < k.nd; i += 256) csum[i] = p.det_csum[(long long)k.b * p.max_dets + i];
    __syncthreads();
    const uint4* pp = (const uint4*)((const uint8_t*)p.proto.p + (long long)k.b * p.proto.stride + (long long)(k.live ? k.px : 0) * 32);
    const uint4 pa = pp[0], pb = pp[1];
    const uint32_t flip = p.proto.kind == TQ_I8 ? 0x80808080u : 0u;
    const uint32_t pv[8] = { pa.x ^ flip, pa.y ^ flip, pa.z ^ flip, pa.w ^ flip, pb.x ^ flip, pb.y ^ flip, pb.z ^ flip, pb.w ^ flip };
    unsigned sp = 0u;
#pragma unroll
    for (int q = 0; q < 8; ++q) sp = __builtin_amdgcn_udot4(pv[q], 0x01010101u, sp, false);
    const int zp = p.proto.zp + (p.proto.kind == TQ_I8 ? 128 : 0), zm = p.mask.zp + (p.mask.kind == TQ_I8 ? 128 : 0);
    const int px_term = 32 * zp * zm - zm * (int)sp;
    for (int d = k.d0; d < k.d1; d += 4) {
        unsigned long long m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m[j] = 0ull;
            if (d + j < k.d1 && ((rel[(d + j) >> 5] >> ((d + j) & 31)) & 1u)) {   // (wave-uniform)
                const float4 c = crop[d + j];
                const bool inside = k.live && k.fx >= c.x && k.fx < c.y && k.fy >= c.z && k.fy < c.w;
                int S = 0;
                if (__ballot(inside) != 0ull) {   // wave-uniform: no lane of these 64 pixels lies in the crop window -> all zeros
                    const uint32_t* co = coef + (d + j) * 8;
                    unsigned dot = 0u;
#pragma unroll
                    for (int q = 0; q < 8; ++q) dot = __builtin_amdgcn_udot4(pv[q], co[q], dot, false);
                    S = (int)dot - zp * csum[d + j] + px_term;
                }
                m[j] = __ballot(inside && S > 0);
            }
        }
        td_mask_store(p, k, d, m);
    }
}

// K4q with a float32 tensor among mask and proto (rule 4): det_masks' arithmetic - acc = fmaf(proto[k], coef[k], acc), k = 0 .. 31,
// then > 0 - on the values of rule 1; the prototypes are dequantised as they are loaded, the coefficients by K3q.
__global__ __launch_bounds__(256) void tfl_det_masks_f(const TflDetectParams p) {
    __shared__ float coef[kTdDetsMax * 32];
    __shared__ float4 crop[kTdDetsMax];
    __shared__ unsigned rel[kTdDetsMax / 32];
    TdMaskBlock k; k.crop = crop; k.rel = rel;
    td_mask_block(p, k);
    for (int i = k.tid; i < k.nd * 32; i += 256) coef[i] = ((const float*)p.det_coef)[(long long)k.b * p.max_dets * 32 + i];   // (written by K3q)
    __syncthreads();
    float pv[32];
    const long long pe = (long long)k.b * p.proto.stride + (long long)(k.live ? k.px : 0) * 32;   // element index
    if (p.proto.kind == TQ_F32) {
        const float4* pp = (const float4*)((const float*)p.proto.p + pe);
#pragma unroll
        for (int q = 0; q < 8; ++q) { const float4 v = pp[q]; pv[4 * q] = v.x; pv[4 * q + 1] = v.y; pv[4 * q + 2] = v.z; pv[4 * q + 3] = v.w; }
    } else {
        const uint4* pp = (const uint4*)((const uint8_t*)p.proto.p + pe);
        const uint4 pa = pp[0], pb = pp[1];
        const uint32_t w[8] = { pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w };
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) pv[4 * q + e] = td_deq(p.proto, td_raw(p.proto.kind, (w[q] >> (8 * e)) & 255u));
    }
    for (int d = k.d0; d < k.d1; d += 4) {
        unsigned long long m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m[j] = 0ull;
            if (d + j < k.d1 && ((rel[(d + j) >> 5] >> ((d + j) & 31)) & 1u)) {   // (wave-uniform)
                const float4 c = crop[d + j];
                const bool inside = k.live && k.fx >= c.x && k.fx < c.y && k.fy >= c.z && k.fy < c.w;
                float acc = 0.0f;
                if (__ballot(inside) != 0ull) {
                    const float* co = coef + (d + j) * 32;
#pragma unroll
                    for (int kk = 0; kk < 32; ++kk) acc = __fmaf_rn(pv[kk], co[kk], acc);
                }
                m[j] = __ballot(inside && acc > 0.0f);
            }
        }
        td_mask_store(p, k, d, m);
    }
}

int tfl_detect_launch_count() { return 4; }

const char* tfl_detect_stage_name(int stage) {
    static const char* n[4] = { "tfl_det_softmax_cand", "tfl_det_class_nms", "tfl_det_frame_top", "tfl_det_masks" };
    return stage >= 0 && stage < 4 ? n[stage] : "?";
}

hipError_t launch_tfl_detect_stage(const TflDetectParams& p, int stage, hipStream_t s) {
    switch (stage) {
        case 0: {   // (the candidate counters are zero on entry: K2q re-zeroes what it consumes)
            const dim3 grid((unsigned)((p.P + TD_K1_PRIORS - 1) / TD_K1_PRIORS), (unsigned)p.n);
            const int esz = p.conf.kind == TQ_F32 ? 4 : 1;
            const size_t lds = (size_t)TD_K1_PRIORS * (size_t)(((p.C * esz + 3) / 4) | 1) * 4;   // <= 128 x 81 dwords = 41 KB
            if (p.conf.kind == TQ_F32) hipLaunchKernelGGL(tfl_det_softmax_cand<TQ_F32>, grid, dim3(TD_K1_PRIORS), lds, s, p);
            else if (p.conf.kind == TQ_I8) hipLaunchKernelGGL(tfl_det_softmax_cand<TQ_I8>, grid, dim3(TD_K1_PRIORS), lds, s, p);
            else hipLaunchKernelGGL(tfl_det_softmax_cand<TQ_U8>, grid, dim3(TD_K1_PRIORS), lds, s, p);
            break;
        }
        case 1: hipLaunchKernelGGL(tfl_det_class_nms, dim3((unsigned)(p.n * (p.C - 1))), dim3(256), 0, s, p); break;
        case 2: hipLaunchKernelGGL(tfl_det_frame_top, dim3((unsigned)p.n), dim3(1024), 0, s, p); break;
        case 3: {
            const dim3 grid((unsigned)((p.hp * p.wp + 255) / 256), (unsigned)p.n, p.n <= 2 ? 8u : (p.n <= 8 ? 2u : 1u));
            if (p.int_mask) hipLaunchKernelGGL(tfl_det_masks_q, grid, dim3(256), 0, s, p);
            else hipLaunchKernelGGL(tfl_det_masks_f, grid, dim3(256), 0, s, p);
            break;
        }
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_tfl_detect(const TflDetectParams& p, hipStream_t s) {
    for (int st = 0; st < 4; ++st) {
        hipError_t e = launch_tfl_detect_stage(p, st, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace yh
