// tflite_exec.hip — executes a parsed TFLite model (uint8 per-tensor quantised MobileNetV2-style
// graphs: the reference's FRC_model.tflite family, data/README.md:5-16 - and what today's converter writes of it: int8
// tensors, per-channel weight scales, uint8 at the edges; DESIGN.md section 11 "TFLite int8") on the GPU.
//
// SURVEY.md §8f-1. Replaces, for a user who holds the reference's model file, the whole of
// interpreter.invoke() (src/yolact.rs:163) plus the surrounding classify
// (:192-234). The arithmetic restates TensorFlow Lite's published uint8 reference kernels
// (gemmlowp fixed-point requantisation); the runtime itself is the un-vendored tflite 0.9.0 crate
// (Cargo.lock:1106-1108), so parity with it is UNPINNED; tests check this executor bit for bit
// against oracle/tfl_oracle.py on synthetic models.
//
// This unit is the host side: the plan (one Prepared per operator: prepare), its fusion (fuse_plan) and grouping (group_plan)
// passes, the launches of one invoke (enqueue_plan), their capture (run_plan) and the yh_tfl_* C ABI - among it the classify batch
// (yh_tfl_classify_batch_u32: n frames as one invoke of 2n images on a handle made by yh_tfl_create_batch). The kernels, their
// parameter structs and launchers are tflite_kernels.hip / tflite_exec.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <limits.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "classify_geo.h"
#include "instance_host.h"
#include "tfl_detect.h"
#include "tfl_instance.h"
#include "tflite_exec.h"
#include "tflite_model.h"
#include "yh_internal.h"

using namespace yh;

namespace {
// ---- host-side quantisation helpers (tflite::QuantizeMultiplier etc.)
void quantize_multiplier(double m, int* mult, int* shift) {
    if (m == 0.0) { *mult = 0; *shift = 0; return; }
    int e;
    const double q = frexp(m, &e);
    long long qf = (long long)floor(q * (double)(1ll << 31) + 0.5);
    if (qf == (1ll << 31)) { qf /= 2; ++e; }
    if (e < -31) { e = 0; qf = 0; }
    *mult = (int)qf; *shift = e;
}
// (sgn: the output is int8 - the type range is [-128, 127] instead of [0, 255])
void act_range(int act, float scale, int zp, int* lo, int* hi, bool sgn = false) {
    auto q = [&](float v) { const float d = v / scale; return zp + (int)(d >= 0 ? floorf(d + 0.5f) : ceilf(d - 0.5f)); };
    const int tlo = sgn ? -128 : 0, thi = sgn ? 127 : 255;
    *lo = tlo; *hi = thi;
    if (act == 1) { *lo = q(0.0f) > tlo ? q(0.0f) : tlo; }
    else if (act == 3) { *lo = q(0.0f) > tlo ? q(0.0f) : tlo; *hi = q(6.0f) < thi ? q(6.0f) : thi; }
    else if (act == 2) { *lo = q(-1.0f) > tlo ? q(-1.0f) : tlo; *hi = q(1.0f) < thi ? q(1.0f) : thi; }
}
void same_pad(int in, int k, int stride, int dil, int* out, int* before) {
    *out = (in + stride - 1) / stride;
    const int eff = (k - 1) * dil + 1, total = (*out - 1) * stride + eff - in;
    *before = total > 0 ? total / 2 : 0;
}

enum PKind { P_CONV, P_DW, P_ADD, P_REQUANT, P_QUANT_F32, P_DEQUANT, P_LUT, P_PAD, P_RESIZE, P_CONCAT, P_COPY, P_CONV_I8 };
struct Prepared {
    PKind kind;
    int oi = -1;         // operator index in the model
    bool dead = false;   // folded into another launch (fuse_plan)
    int group = -1;           // >= 0: this convolution is launched as part of h->groups[group] (group_plan), by the group's first member
    ConvQ conv;               // every convolution's one record: the passes patch this, the int8 kernels' argument is built from it (conv_i8_args)
    const uint8_t* wq = nullptr; const int* cterm = nullptr;   // P_CONV_I8: the int8 weight panel and the per-channel constant term (ConvI8)
    int form = -1;            // P_CONV_I8, tfl_dot >= 3: the register-fed kernel's form (conv_i8_direct_form; the convolutions of a group share it)
    AddQ add; PadQ pad; ResizeQ rs;
    std::vector<CatQ> cat;
    const void* src = nullptr; void* dst = nullptr; long long n = 0;
    int zi = 0, zo = 0, m = 0, s = 0, lo = 0, hi = 255; float scale = 1.0f;
    bool sgn_in = false, sgn_out = false;   // element-wise entries: the input / the output is int8 (a QUANTIZE may change type)
    const uint8_t* lut = nullptr;
};

}  // namespace

struct yh_tfl {
    int dev = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::vector<uint8_t> file;
    TflModel m;
    std::vector<void*> tens;
    std::vector<char> alias;    // tens[i] shares another tensor's buffer (RESHAPE): not freed twice
    std::vector<char> per_image;   // constant i is read as an operator's DATA operand (ADD, CONCATENATION, RESHAPE ...): stored once per image
    std::vector<void*> extra;   // LUTs etc.
    std::vector<Prepared> plan;
    int max_images = 2;                          // images per invoke the buffers are sized for: 2 (the two tiles of yolact.rs:216-217) or yh_tfl_create_batch's
    int nb = 1;                                  // images of the next invoke (yh_tfl_set_batch)
    bool batch_ok = true;                        // no operator of the model touches the image axis
    std::vector<hipGraphExec_t> gexecs;          // [max_images]: the plan per batch size, captured at its first invoke and replayed (tensor addresses never change)
    // yh_tuning.tfl_group (round 4): independent register-fed convolutions of one kernel form and one depth of the plan's DAG as ONE
    // launch (group_plan); `order` is the plan in execution order (by depth; the identity when nothing is grouped)
    // (the tables of image count nb at [nb - 1]: 1 and 2 built at create, every other at the first invoke of that nb - group_tables)
    struct ConvGroup { std::vector<int> members; std::vector<const ConvI8*> probs; std::vector<const int*> tile_start; std::vector<int> tiles; };
    int use_group = 1;
    std::vector<ConvGroup> groups;
    std::vector<int> order;
    int use_fuse = 1;                 // yh_tuning.tfl_fuse: element-wise operators / PAD / CONCATENATION parts folded into their producers (fuse_plan)
    std::vector<char> gone;           // tensor i is never written by the fused plan (yh_tfl_tensor_read says so)
    int use_dot = 3, use_graph = 0;   // yh_tuning.tfl_dot (0 scalar kernel, 1 v_dot4 kernel, 2 + int8 MFMA kernel on LDS tiles where Ci % 64 == 0, 3 + its register-fed form - one wave per 16 x 16 tile - where Ci % 4 == 0: default) / tfl_graph
    hipStream_t side = nullptr;       // tfl_graph: carries the second branch of the captured graph
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    void* side_word = nullptr;
    // classify scratch
    uint32_t *frame_dev = nullptr, *codes_dev = nullptr, *stitch_dev = nullptr;
    uint8_t* tiles_dev = nullptr;
    float *rs_tmp = nullptr, *cells_dev = nullptr;
    int* diverged_dev = nullptr;
    size_t frame_cap = 0, rs_cap = 0;
    // classify batch (yh_tfl_classify_batch_u32): its own buffers, allocated at the first call, grow only
    uint32_t* clsb_frames = nullptr;  // [n][height][width]: the frames as uploaded, then as classified
    float* clsb_cells = nullptr;      // [2n][cells][C] output 4 of the invoke as f32
    uint32_t* clsb_codes = nullptr;   // [2n][cells]
    int* clsb_div = nullptr;          // [2n] divergence flags
    size_t clsb_frames_cap = 0, clsb_cells_cap = 0, clsb_codes_cap = 0, clsb_div_cap = 0;
    yh::ClassifyGeo clsb_geo;         // the resize tables of the last geometry and the pre kernel's plan (classify_geo.h)
    int clsb_n = -1;                  // frames of the last batch; -1: no batch
    // detection tail on the model's own outputs (yh_tfl_detect_setup; DESIGN.md section 11 "TFLite detections"): the setup's
    // parameters and workspaces, the test entry's own (yh_tfl_op_detect), and whose results are current
    struct DetSet { bool ready = false; yh::TflDetectParams p{}; int max_images = 0; std::vector<void*> bufs; std::vector<int> sig; };
    DetSet det, opdet;
    const DetSet* det_last = nullptr; // what yh_tfl_read_detections shows; nullptr: nothing current (no tail yet, or a newer input / invoke)
    int det_last_n = 0;               // its images
    int last_nb = 0;                  // images of the last invoke; 0: none yet
    // instance frames painted from the setup's detections (tfl_instance.hip; DESIGN.md section 11 "TFLite instance frames"): one
    // batch, filled by yh_tfl_instance_batch, yh_tfl_instance_frames or yh_tfl_op_instance_frames, whichever ran last
    yh::TflInstance inst;
    int fail(int code, const std::string& msg) { err = msg; return code; }
};

namespace {
thread_local std::string g_tfl_create_error;

#define TCHK(h, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return (h)->fail(YH_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

// Host data to a new device allocation that the handle owns (freed with h->extra).
template <class T>
int upload(yh_tfl* h, const T* src, size_t count, const char* what, const T** out) {
    void* d = nullptr;
    if (hipMalloc(&d, count * sizeof(T)) != hipSuccess) return h->fail(YH_ENOMEM, std::string("hipMalloc ") + what);
    h->extra.push_back(d);
    if (hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return h->fail(YH_EHIP, std::string(what) + " upload");
    *out = (const T*)d;
    return YH_OK;
}
// The bytes of a tensor's device allocation: a constant's own, an activation's for max_images images (image-major: room for the
// batch plan), and 16 more (the kernels' dword and 16-byte loads may reach past the last element). A constant that an operator reads
// where an activation could stand (an ADD operand, a CONCATENATION part, a RESHAPE's input ...) is stored like one, a copy per image:
// the kernels index every data operand image-major, and the second image of a batch plan must meet the same constant, not the bytes behind it.
size_t tensor_alloc_bytes(const yh_tfl* h, size_t i) {
    const TflTensor& t = h->m.tensors[i];
    return t.count() * t.elem() * (t.data && !h->per_image[i] ? 1 : (size_t)h->max_images) + 16;
}

// One operator on its way into the plan: its tensors and their device buffers by tensor index, its YH_EINVAL, and one function per
// operator family that fills the plan entry or returns the error.
struct OpPrep {
    yh_tfl* h; const TflOp& op; size_t oi;
    const TflTensor& T(int i) const { return h->m.tensors[i]; }
    bool u8(int i) const { return T(i).type == TFL_U8 && T(i).quant; }
    bool i8(int i) const { return T(i).type == TFL_I8 && T(i).quant; }
    bool q8(int i) const { return u8(i) || i8(i); }
    bool same8(int a, int b) const { return q8(a) && T(a).type == T(b).type && T(b).quant; }   // both uint8 or both int8
    void* dev(int i) const { return h->tens[i]; }
    int bad(const std::string& what) const { return h->fail(YH_EINVAL, what + " (operator " + std::to_string(oi) + ")"); }
    // CONV_2D / DEPTHWISE_CONV_2D: the record, and what the kernel form that tfl_dot selects needs beside it in device memory
    int conv(Prepared& pr) const {
        if (!(op.in.size() >= 2 && op.out.size() == 1)) return bad("conv: bad arity");
        const TflTensor &x = T(op.in[0]), &w = T(op.in[1]), &y = T(op.out[0]);
        const bool dw = op.code == TFL_DEPTHWISE_CONV_2D;
        const int bi = op.in.size() > 2 ? op.in[2] : -1;
        if (u8(op.in[0]) && w.per_channel()) return bad("conv: uint8 activations with per-channel weight scales are not supported");
        if (i8(op.in[0]) && u8(op.in[1])) return bad("conv: int8 activations with uint8 weights are not supported");
        const bool sgn = i8(op.in[0]);   // int8 activations, symmetric int8 weights (the reader has checked their zero points), int8 output
        if (!(((u8(op.in[0]) && u8(op.in[1]) && u8(op.out[0])) || (sgn && i8(op.in[1]) && i8(op.out[0]))) && x.shape.size() == 4 && w.shape.size() == 4 &&
              y.shape.size() == 4 && x.shape[0] == 1 && (bi < 0 || (T(bi).type == TFL_I32 && T(bi).data)) && w.data))
            return bad("conv: only uint8 per-tensor, or int8 with int8 per-tensor / per-channel weights, quantised NHWC batch-1 convolutions with constant weights are supported");
        ConvQ& c = pr.conv;
        c.H = x.shape[1]; c.W = x.shape[2]; c.Ci = x.shape[3];
        c.kh = w.shape[1]; c.kw = w.shape[2];
        c.Co = dw ? w.shape[3] : w.shape[0];
        c.dm = dw ? op.depth_mult : 1;
        c.sh = op.stride_h; c.sw = op.stride_w; c.dh = op.dil_h; c.dw = op.dil_w;
        if (op.padding == 0) { same_pad(c.H, c.kh, c.sh, c.dh, &c.Ho, &c.ph); same_pad(c.W, c.kw, c.sw, c.dw, &c.Wo, &c.pw); }
        else { c.Ho = (c.H - ((c.kh - 1) * c.dh + 1) + c.sh) / c.sh; c.Wo = (c.W - ((c.kw - 1) * c.dw + 1) + c.sw) / c.sw; c.ph = c.pw = 0; }
        if (!(y.shape[1] == c.Ho && y.shape[2] == c.Wo && y.shape[3] == c.Co && (dw ? (w.shape[0] == 1 && c.Co == c.Ci * c.dm) : w.shape[3] == c.Ci) &&
              (bi < 0 || (int)T(bi).count() == c.Co)))
            return bad("conv: tensor shapes are inconsistent");
        c.x = (const uint8_t*)dev(op.in[0]); c.w = (const uint8_t*)dev(op.in[1]);
        c.bias = bi >= 0 ? (const int*)dev(bi) : nullptr; c.y = (uint8_t*)dev(op.out[0]);
        c.zx = x.zp; c.zw = w.zp; c.zo = y.zp;
        c.xs = (long long)c.H * c.W * c.Ci; c.ys = (long long)c.Ho * c.Wo * c.Co;
        quantize_multiplier((double)x.scale * (double)w.scale / (double)y.scale, &c.mult, &c.shift);
        act_range(op.act, y.scale, y.zp, &c.lo, &c.hi, sgn);
        pr.kind = dw ? P_DW : P_CONV;
        const int CoPad = (c.Co + 63) / 64 * 64;
        if (sgn) {   // one multiplier per output channel (a single weight scale: all equal), padded like the MFMA kernels' cterm
            std::vector<int> mt(CoPad, 0), st(CoPad, 0);
            for (int oc = 0; oc < c.Co; ++oc)
                quantize_multiplier((double)x.scale * (double)(w.per_channel() ? w.scales[oc] : w.scale) / (double)y.scale, &mt[oc], &st[oc]);
            if (int rc = upload(h, mt.data(), mt.size(), "multiplier table", &c.mtab)) return rc;
            if (int rc = upload(h, st.data(), st.size(), "shift table", &c.stab)) return rc;
            c.sgn = 1;
        }
        if (!dw && h->use_dot >= 2 && c.Ci % (h->use_dot >= 3 ? 4 : 64) == 0 && (((size_t)c.x) & 3) == 0 && (long long)c.kh * c.kw * c.Ci < 131072) {
            // int8 MFMA form: the weight panel as int8 (w ^ 0x80) padded to 64-channel tiles, and per channel
            //   cterm = (128 - zx) sum(w - 128) + K (128 - zx)(128 - zw) + bias   (all exact in int32: |.| < 2^31 for K < 2^17)
            // int8 (sgn), the native form: the weight bytes as they are and cterm = bias - zx sum(w), computed in 64 bits and kept modulo
            //   2^32 - which is all the kernel's int32 accumulator keeps of sum(x w) too, so the sum of the two is TFLite's value
            //   whenever TFLite's own accumulator does not overflow
            const int K = c.kh * c.kw * c.Ci;
            std::vector<uint8_t> wq((size_t)CoPad * K + 16, sgn ? 0x00 : 0x80);   // padding rows: w' = 0 (+ 16 bytes: the register-fed kernel's last load of a row may reach past it)
            std::vector<int> ct(CoPad, 0);
            const int* bias_h = bi >= 0 ? (const int*)T(bi).data : nullptr;
            for (int oc = 0; oc < c.Co; ++oc) {
                long long sw = 0;
                if (sgn) {
                    for (int k = 0; k < K; ++k) { const uint8_t b = w.data[(size_t)oc * K + k]; wq[(size_t)oc * K + k] = b; sw += (int)(int8_t)b; }
                    ct[oc] = (int)(uint32_t)(uint64_t)((long long)(bias_h ? bias_h[oc] : 0) - (long long)c.zx * sw);
                    continue;
                }
                for (int k = 0; k < K; ++k) { const uint8_t b = w.data[(size_t)oc * K + k]; wq[(size_t)oc * K + k] = (uint8_t)(b ^ 0x80); sw += (int)b - 128; }
                ct[oc] = (int)((128 - c.zx) * sw + (long long)K * (128 - c.zx) * (128 - c.zw) + (bias_h ? bias_h[oc] : 0));
            }
            if (int rc = upload(h, wq.data(), wq.size(), "int8 panel", &pr.wq)) return rc;
            if (int rc = upload(h, ct.data(), ct.size(), "int8 panel", &pr.cterm)) return rc;
            pr.kind = P_CONV_I8;
            if (h->use_dot >= 3 && (pr.form = conv_i8_direct_form(c.kh, c.kw, c.Ci)) < 0) return bad("conv: the register-fed kernel has no form for this extent and depth");
            return YH_OK;
        }
        if (!dw && !sgn && h->use_dot && c.Ci % 4 == 0 && (long long)c.kh * c.kw * c.Ci * 65025ll < (1ll << 31)) {
            // per (channel, tap) sums of the raw weight bytes for the dot-product kernel
            const int ntaps = c.kh * c.kw;
            std::vector<int> ws((size_t)c.Co * ntaps, 0);
            for (int oc = 0; oc < c.Co; ++oc)
                for (int tp = 0; tp < ntaps; ++tp) {
                    int sum = 0;
                    const uint8_t* wp = w.data + ((size_t)oc * ntaps + tp) * c.Ci;
                    for (int ch = 0; ch < c.Ci; ++ch) sum += wp[ch];
                    ws[(size_t)oc * ntaps + tp] = sum;
                }
            return upload(h, ws.data(), ws.size(), "weight sums", &c.wsum);
        }
        return YH_OK;
    }
    int add(Prepared& pr) const {
        if (!(op.in.size() == 2 && same8(op.in[0], op.in[1]) && same8(op.in[0], op.out[0]) && T(op.in[0]).count() == T(op.out[0]).count() &&
              T(op.in[1]).count() == T(op.out[0]).count()))
            return bad("add: only same-shape tensors of one type, uint8 or int8, are supported");
        const TflTensor &a = T(op.in[0]), &b = T(op.in[1]), &y = T(op.out[0]);
        AddQ& q = pr.add; pr.kind = P_ADD;
        q.a = (const uint8_t*)dev(op.in[0]); q.b = (const uint8_t*)dev(op.in[1]); q.y = (uint8_t*)dev(op.out[0]);
        q.n = (long long)y.count(); q.za = a.zp; q.zb = b.zp; q.zo = y.zp;
        const double twice = 2.0 * (a.scale > b.scale ? (double)a.scale : (double)b.scale);
        quantize_multiplier((double)a.scale / twice, &q.m1, &q.s1);
        quantize_multiplier((double)b.scale / twice, &q.m2, &q.s2);
        quantize_multiplier(twice / ((double)(1 << 20) * (double)y.scale), &q.mo, &q.so);
        q.sgn = i8(op.out[0]) ? 1 : 0;
        act_range(op.act, y.scale, y.zp, &q.lo, &q.hi, q.sgn != 0);
        return YH_OK;
    }
    // RELU / RELU6 / QUANTIZE: a requantisation of uint8 or int8 (QUANTIZE: to either type), or QUANTIZE of float32
    int requant(Prepared& pr) const {
        if (!(op.in.size() == 1 && op.out.size() == 1 && q8(op.out[0]) && T(op.in[0]).count() == T(op.out[0]).count())) return bad("quantize/relu: bad tensors");
        const TflTensor &x = T(op.in[0]), &y = T(op.out[0]);
        pr.src = dev(op.in[0]); pr.dst = dev(op.out[0]); pr.n = (long long)y.count();
        pr.sgn_in = i8(op.in[0]); pr.sgn_out = i8(op.out[0]);
        if (x.type == TFL_F32 && op.code == TFL_QUANTIZE) { pr.kind = P_QUANT_F32; pr.scale = y.scale; pr.zo = y.zp; return YH_OK; }
        if (!q8(op.in[0])) return bad("quantize/relu: input must be float32 or quantised uint8 / int8");
        if (op.code != TFL_QUANTIZE && pr.sgn_in != pr.sgn_out) return bad("relu: input and output must be of one type");
        pr.kind = P_REQUANT; pr.zi = x.zp; pr.zo = y.zp;
        quantize_multiplier((double)x.scale / (double)y.scale, &pr.m, &pr.s);
        act_range(op.code == TFL_RELU ? 1 : (op.code == TFL_RELU6 ? 3 : 0), y.scale, y.zp, &pr.lo, &pr.hi, pr.sgn_out);
        return YH_OK;
    }
    int dequant(Prepared& pr) const {
        if (!(op.in.size() == 1 && q8(op.in[0]) && T(op.out[0]).type == TFL_F32 && T(op.in[0]).count() == T(op.out[0]).count())) return bad("dequantize: bad tensors");
        pr.kind = P_DEQUANT; pr.src = dev(op.in[0]); pr.dst = dev(op.out[0]); pr.n = (long long)T(op.out[0]).count();
        pr.scale = T(op.in[0]).scale; pr.zi = T(op.in[0]).zp; pr.sgn_in = i8(op.in[0]);
        return YH_OK;
    }
    int tanh_table(Prepared& pr) const {
        if (!(op.in.size() == 1 && same8(op.in[0], op.out[0]) && T(op.in[0]).count() == T(op.out[0]).count())) return bad("tanh: only uint8 -> uint8 and int8 -> int8 are supported");
        const TflTensor &x = T(op.in[0]), &y = T(op.out[0]);
        const bool sgn = i8(op.in[0]);
        // uint8: entry q of 256. int8: one entry per value q in [-128, 127], stored at index q AND at its raw byte's index q + 256 -
        // 384 entries from index -128, `lut` pointing at index 0: the kernel's byte and a folded chain's true integer find the same one
        uint8_t lut[384];
        const float inv = 1.0f / y.scale;
        const int first = sgn ? -128 : 0, tlo = sgn ? -128 : 0, thi = sgn ? 127 : 255;
        for (int i = first; i < 256; ++i) {   // PopulateLookupTable
            const int q = sgn && i > 127 ? i - 256 : i;
            const float xv = x.scale * (float)(q - x.zp);
            const float yv = (float)tanh((double)xv);
            const float r = yv * inv;
            const int rr = (int)(r >= 0 ? floorf(r + 0.5f) : ceilf(r - 0.5f)) + y.zp;
            lut[i - first] = (uint8_t)(rr < tlo ? tlo : (rr > thi ? thi : rr));
        }
        pr.kind = P_LUT; pr.src = dev(op.in[0]); pr.dst = dev(op.out[0]); pr.n = (long long)y.count();
        pr.sgn_in = pr.sgn_out = sgn;
        if (int rc = upload(h, lut, (size_t)(256 - first), "tanh table", &pr.lut)) return rc;
        pr.lut -= first;
        return YH_OK;
    }
    int pad(Prepared& pr) const {
        if (!(op.in.size() == 2 && same8(op.in[0], op.out[0]) && T(op.in[1]).type == TFL_I32 && T(op.in[1]).data &&
              T(op.in[0]).shape.size() == 4 && T(op.in[1]).count() == 8))
            return bad("pad: need a uint8 or int8 4-D input, an output of its type and constant [4,2] paddings");
        const TflTensor &x = T(op.in[0]), &y = T(op.out[0]);
        const int* pp = (const int*)T(op.in[1]).data;
        PadQ& q = pr.pad; pr.kind = P_PAD;
        for (int d = 0; d < 4; ++d) {
            q.id[d] = x.shape[d]; q.before[d] = pp[2 * d]; q.od[d] = x.shape[d] + pp[2 * d] + pp[2 * d + 1];
            if (!(pp[2 * d] >= 0 && pp[2 * d + 1] >= 0 && y.shape[d] == q.od[d])) return bad("pad: output shape mismatch");
        }
        if (q.id[0] != 1 || q.od[0] != 1) h->batch_ok = false;
        q.x = (const uint8_t*)dev(op.in[0]); q.y = (uint8_t*)dev(op.out[0]); q.fill = y.zp;
        return YH_OK;
    }
    int resize(Prepared& pr) const {
        if (!(op.in.size() == 2 && same8(op.in[0], op.out[0]) && T(op.in[1]).type == TFL_I32 && T(op.in[1]).data && T(op.in[1]).count() == 2 &&
              T(op.in[0]).shape.size() == 4 && T(op.in[0]).shape[0] == 1))
            return bad("resize_bilinear: need uint8 or int8 NHWC batch 1, an output of its type and a constant size");
        const TflTensor &x = T(op.in[0]), &y = T(op.out[0]);
        const int* sz = (const int*)T(op.in[1]).data;
        ResizeQ& q = pr.rs; pr.kind = P_RESIZE;
        q.H = x.shape[1]; q.W = x.shape[2]; q.C = x.shape[3]; q.Ho = sz[0]; q.Wo = sz[1]; q.half_pixel = op.half_pixel ? 1 : 0;
        if (!(y.shape[1] == q.Ho && y.shape[2] == q.Wo && y.shape[3] == q.C)) return bad("resize_bilinear: output shape mismatch");
        q.hs = (op.align_corners && q.Ho > 1) ? (float)(q.H - 1) / (float)(q.Ho - 1) : (float)q.H / (float)q.Ho;
        q.ws = (op.align_corners && q.Wo > 1) ? (float)(q.W - 1) / (float)(q.Wo - 1) : (float)q.W / (float)q.Wo;
        q.x = (const uint8_t*)dev(op.in[0]); q.y = (uint8_t*)dev(op.out[0]); q.ys = (long long)q.Ho * q.Wo * q.C;
        if (i8(op.in[0])) {   // TFLite's integer kernel: the steps in 10-bit fixed point (the positions stay inside 32 bits: sizes <= 2^16)
            if (x.scale != y.scale || x.zp != y.zp) return bad("resize_bilinear: an int8 input and its output must share scale and zero point");
            if (q.H > 65536 || q.W > 65536 || q.Ho > 65536 || q.Wo > 65536 || q.Ho < 1 || q.Wo < 1) return bad("resize_bilinear: int8 sizes must be 1 .. 65536");
            auto step10 = [&](int in, int out) {
                return op.align_corners && out > 1 ? (int)(((1ll << 10) * (in - 1) + (out - 1) / 2) / (out - 1)) : (int)(((1ll << 10) * in + out / 2) / out);
            };
            q.sgn = 1; q.hs10 = step10(q.H, q.Ho); q.ws10 = step10(q.W, q.Wo);
        }
        return YH_OK;
    }
    int concat(Prepared& pr) const {
        const TflTensor& y = T(op.out[0]);
        const int nd = (int)y.shape.size();
        const int axis = op.axis < 0 ? op.axis + nd : op.axis;
        if (!(axis >= 0 && axis < nd && !op.in.empty())) return bad("concatenation: bad axis");
        if (axis == 0) h->batch_ok = false;   // (joins along the image axis: this model runs one image per invoke only)
        long long outer = 1; int inner_o = 1;
        for (int d = 0; d < axis; ++d) outer *= y.shape[d];
        for (int d = axis; d < nd; ++d) inner_o *= y.shape[d];
        int off = 0;
        for (int ii : op.in) {
            const TflTensor& x = T(ii);
            if (!(x.type == y.type && (int)x.shape.size() == nd)) return bad("concatenation: type/rank mismatch");
            int inner = 1;
            for (int d = axis; d < nd; ++d) inner *= x.shape[d];
            CatQ c;
            c.x = (const uint8_t*)dev(ii); c.y = (uint8_t*)dev(op.out[0]); c.outer = outer; c.inner = inner; c.row = inner_o; c.off = off;
            c.esz = x.type == TFL_U8 || x.type == TFL_I8 ? 1 : 4; c.rescale = 0; c.sc = 1.0f; c.bias = 0.0f; c.zo = y.zp;
            if (x.type == TFL_I8 && (x.zp != y.zp || x.scale != y.scale))   // (TFLite rescales only uint8)
                return bad("concatenation: every int8 input must have the output's scale and zero point");
            if (x.type == TFL_U8 && y.quant && (x.zp != y.zp || x.scale != y.scale)) {  // ConcatenationWithScaling
                const float inv = 1.0f / y.scale;
                c.rescale = 1; c.sc = x.scale * inv; c.bias = (float)(-x.zp) * c.sc;
            }
            pr.cat.push_back(c);
            off += inner;
        }
        pr.kind = P_CONCAT;
        return off == inner_o ? YH_OK : bad("concatenation: output shape mismatch");
    }
    // RESHAPE moves no bytes: every tensor is written once by its producer, so the output can share the input's buffer (ops are in
    // topological order: its consumers are prepared later and pick the shared pointer up) and the plan gets no entry (*shares). Only
    // a reshape of a constant keeps its own copy.
    int reshape(Prepared& pr, bool* shares) const {
        if (!(!op.in.empty() && T(op.in[0]).count() * T(op.in[0]).elem() == T(op.out[0]).count() * T(op.out[0]).elem())) return bad("reshape: size mismatch");
        *shares = !T(op.in[0]).data && !T(op.out[0]).data;
        if (!*shares) { pr.kind = P_COPY; pr.src = dev(op.in[0]); pr.dst = dev(op.out[0]); pr.n = (long long)(T(op.out[0]).count() * T(op.out[0]).elem()); return YH_OK; }
        hipFree(h->tens[op.out[0]]);
        h->tens[op.out[0]] = h->tens[op.in[0]];
        h->alias[op.out[0]] = 1;
        return YH_OK;
    }
};

// The tensors' device buffers, then one plan entry per operator.
int prepare(yh_tfl* h) {
    TflModel& m = h->m;
    h->tens.assign(m.tensors.size(), nullptr);
    h->alias.assign(m.tensors.size(), 0);
    h->per_image.assign(m.tensors.size(), 0);
    for (const TflOp& op : m.ops) {   // the data operands: every input of ADD and CONCATENATION, the first of every other operator
        const size_t nd = op.code == TFL_ADD || op.code == TFL_CONCATENATION ? op.in.size() : (op.in.empty() ? 0 : 1);
        for (size_t k = 0; k < nd; ++k)
            if (op.in[k] >= 0 && op.in[k] < (int)m.tensors.size() && m.tensors[op.in[k]].data) h->per_image[op.in[k]] = 1;
    }
    for (size_t i = 0; i < m.tensors.size(); ++i) {
        const TflTensor& t = m.tensors[i];
        const size_t bytes = t.count() * t.elem();
        if (bytes == 0) continue;
        const size_t alloc = tensor_alloc_bytes(h, i);
        TCHK(h, hipMalloc(&h->tens[i], alloc));
        if (t.data) {
            for (int k = 0; k < (h->per_image[i] ? h->max_images : 1); ++k)
                TCHK(h, hipMemcpy((char*)h->tens[i] + (size_t)k * bytes, t.data, bytes, hipMemcpyHostToDevice));
        }
        else TCHK(h, hipMemset(h->tens[i], 0, alloc));
    }
    for (size_t oi = 0; oi < m.ops.size(); ++oi) {
        const OpPrep o{ h, m.ops[oi], oi };
        Prepared pr = Prepared();   // (value-initialised: the kernel parameter blocks start zeroed - no folded operators)
        pr.oi = (int)oi;
        bool shares = false;   // (a RESHAPE that shares its input's buffer: no plan entry)
        int rc;
        switch (o.op.code) {
            case TFL_CONV_2D: case TFL_DEPTHWISE_CONV_2D: rc = o.conv(pr); break;
            case TFL_ADD: rc = o.add(pr); break;
            case TFL_RELU: case TFL_RELU6: case TFL_QUANTIZE: rc = o.requant(pr); break;
            case TFL_DEQUANTIZE: rc = o.dequant(pr); break;
            case TFL_TANH: rc = o.tanh_table(pr); break;
            case TFL_PAD: rc = o.pad(pr); break;
            case TFL_RESIZE_BILINEAR: rc = o.resize(pr); break;
            case TFL_CONCATENATION: rc = o.concat(pr); break;
            case TFL_RESHAPE: rc = o.reshape(pr, &shares); break;
            default:
                rc = o.bad(o.op.code == TFL_CUSTOM ? "custom operator '" + o.op.custom + "' (an EdgeTPU-compiled model? load the non-compiled FRC_model.tflite instead)"
                                                   : "unsupported builtin operator code " + std::to_string(o.op.code));
        }
        if (rc) return rc;
        if (!shares) h->plan.push_back(pr);
    }
    return YH_OK;
}

// Plan-time operator fusion (yh_tuning.tfl_fuse, default on). The reference runs 138 of its 141 operators as
// ONE compiled unit on the EdgeTPU (data/README.md:34-39); one launch per operator made ~70 small kernels at their ~5 us floor
// 0.35 ms of a 0.9 ms invoke. Folded here, all bit-exact by construction (PostOps above):
//   * QUANTIZE / RELU / RELU6 (uint8 -> uint8), TANH and ADD into the epilogue of the convolution, depthwise convolution or
//     RESIZE_BILINEAR that produces their operand last - when that tensor has no other reader and is not a graph output;
//   * a CONCATENATION part whose quantisation equals the output's and which is one contiguous block per image: its producer
//     writes straight into the concatenated tensor;
//   * PAD (height / width only) in front of convolutions: the convolution reads the unpadded tensor with the padding as its own.
// RESHAPE already shares its input's buffer. Tensors that are no longer written are listed in h->gone.
void fuse_plan(yh_tfl* h) {
    const TflModel& m = h->m;
    const int nt = (int)m.tensors.size(), nops = (int)m.ops.size();
    std::vector<int> root(nt), plan_of(nops, -1), out_refs(nt, 0), prod(nt, -1);
    for (int i = 0; i < nt; ++i) root[i] = i;
    for (const TflOp& op : m.ops)   // (topological order: the input's root is final when its reshape is met)
        if (op.code == TFL_RESHAPE && !op.in.empty() && h->tens[op.out[0]] == h->tens[op.in[0]]) root[op.out[0]] = root[op.in[0]];
    for (size_t pi = 0; pi < h->plan.size(); ++pi) plan_of[h->plan[pi].oi] = (int)pi;
    std::vector<std::vector<int>> cons(nt);
    for (int oi = 0; oi < nops; ++oi) {
        if (plan_of[oi] < 0) continue;   // (buffer-sharing RESHAPE: transparent)
        for (int t : m.ops[oi].in) if (t >= 0 && !m.tensors[t].data) cons[root[t]].push_back(oi);
        for (int t : m.ops[oi].out) prod[root[t]] = plan_of[oi];
    }
    for (int t : m.outputs) ++out_refs[root[t]];
    auto mark_gone = [&](int r) { for (int t = 0; t < nt; ++t) if (root[t] == r) h->gone[t] = 1; };
    auto is_conv = [](PKind k) { return k == P_CONV || k == P_CONV_I8 || k == P_DW; };
    // ---- PAD into the convolutions that read it
    for (Prepared& pd : h->plan) {
        if (pd.kind != P_PAD) continue;
        const PadQ& q = pd.pad;
        const int r = root[m.ops[pd.oi].out[0]];
        if (q.before[0] || q.before[3] || q.od[0] != q.id[0] || q.od[3] != q.id[3] || out_refs[r]) continue;
        bool all = !cons[r].empty();
        for (int c : cons[r]) all = all && is_conv(h->plan[plan_of[c]].kind) && root[m.ops[c].in[0]] == r;
        if (!all) continue;
        for (int c : cons[r]) {
            ConvQ& k = h->plan[plan_of[c]].conv;
            k.x = q.x; k.H = q.id[1]; k.W = q.id[2]; k.ph += q.before[1]; k.pw += q.before[2]; k.xs = (long long)k.H * k.W * k.Ci;
        }
        pd.dead = true;
        mark_gone(r);
    }
    // ---- element-wise consumers, ADD and contiguous CONCATENATION parts into their producers
    for (size_t pi = 0; pi < h->plan.size(); ++pi) {
        Prepared& p = h->plan[pi];
        if (p.dead || !(is_conv(p.kind) || p.kind == P_RESIZE)) continue;
        PostOps po;
        memset(&po, 0, sizeof po);
        int cur = root[m.ops[p.oi].out[0]];
        uint8_t* y = nullptr;
        long long ys = 0;
        bool has_add = false;
        const int prod_sgn = p.kind == P_RESIZE ? p.rs.sgn : p.conv.sgn;   // the producer kernel's signedness: how it reads an ADD's other operand
        while (!out_refs[cur] && cons[cur].size() == 1) {
            const int c = cons[cur][0], cp = plan_of[c];
            if (cp <= (int)pi) break;
            Prepared& q = h->plan[cp];
            if (q.dead) break;
            if ((q.kind == P_REQUANT || q.kind == P_LUT) && po.n < 3) {
                PostStep& t = po.st[po.n++];
                t.kind = q.kind == P_REQUANT ? 1 : (q.sgn_out ? 4 : 2);
                t.zi = q.zi; t.zo = q.zo; t.m = q.m; t.s = q.s; t.lo = q.lo; t.hi = q.hi; t.lut = q.lut;
            } else if (q.kind == P_ADD && !has_add && po.n < 3 && q.add.sgn == prod_sgn) {
                const int a = root[m.ops[c].in[0]], b = root[m.ops[c].in[1]], other = a == cur ? b : a;
                // the other operand must be complete when this producer runs: written by an earlier launch (or the graph input / a constant)
                if (a == b || (prod[other] >= (int)pi) || h->gone[other]) break;
                po.st[po.n++].kind = 3;
                has_add = true;
                po.q_is_a = a == cur;
                po.other = po.q_is_a ? q.add.b : q.add.a;
                po.other_s = q.add.n;   // (uint8: elements = bytes per image)
                po.za = q.add.za; po.zb = q.add.zb; po.m1 = q.add.m1; po.s1 = q.add.s1; po.m2 = q.add.m2; po.s2 = q.add.s2;
                po.mo = q.add.mo; po.so = q.add.so; po.azo = q.add.zo; po.alo = q.add.lo; po.ahi = q.add.hi;
            } else if (q.kind == P_CONCAT) {
                size_t k = 0;
                for (; k < q.cat.size(); ++k) if (q.cat[k].x == (const uint8_t*)h->tens[cur]) break;
                if (k == q.cat.size()) break;
                const CatQ part = q.cat[k];
                if (part.rescale || part.esz != 1 || part.outer != 1) break;
                y = part.y + part.off; ys = part.row;
                q.cat.erase(q.cat.begin() + (long)k);
                if (q.cat.empty()) q.dead = true;
                mark_gone(cur);
                cur = -1;
                break;
            } else break;
            q.dead = true;
            mark_gone(cur);
            cur = root[m.ops[c].out[0]];
        }
        if (cur >= 0 && cur != root[m.ops[p.oi].out[0]]) { y = (uint8_t*)h->tens[cur]; h->gone[cur] = 0; for (int t = 0; t < nt; ++t) if (root[t] == cur) h->gone[t] = 0; }
        if (p.kind == P_RESIZE) { p.rs.po = po; if (y) { p.rs.y = y; if (ys) p.rs.ys = ys; } }
        else { p.conv.po = po; if (y) { p.conv.y = y; if (ys) p.conv.ys = ys; } }
    }
}

// What a plan entry reads and writes (device pointers into the tensors' allocations).
struct EntryIo { std::vector<const void*> rd, wr; };
static void entry_io(const Prepared& p, EntryIo& io) {
    switch (p.kind) {
        case P_CONV: case P_DW: case P_CONV_I8: io.rd = { p.conv.x }; io.wr = { p.conv.y }; if (p.conv.po.other) io.rd.push_back(p.conv.po.other); break;
        case P_ADD: io.rd = { p.add.a, p.add.b }; io.wr = { p.add.y }; break;
        case P_PAD: io.rd = { p.pad.x }; io.wr = { p.pad.y }; break;
        case P_RESIZE: io.rd = { p.rs.x }; io.wr = { p.rs.y }; if (p.rs.po.other) io.rd.push_back(p.rs.po.other); break;
        case P_CONCAT: for (const CatQ& c : p.cat) { io.rd.push_back(c.x); io.wr.push_back(c.y); } break;
        default: io.rd = { p.src }; io.wr = { p.dst }; break;
    }
}

// The int8 MFMA kernels' argument of a P_CONV_I8 entry for `nb` images: the record's fields, the int8 panel, K and M.
static ConvI8 conv_i8_args(const Prepared& p, int nb) {
    const ConvQ& c = p.conv;
    ConvI8 q = {};
    q.x = c.x; q.wq = p.wq; q.cterm = p.cterm; q.y = c.y;
    q.H = c.H; q.W = c.W; q.Ci = c.Ci; q.Ho = c.Ho; q.Wo = c.Wo; q.Co = c.Co; q.kh = c.kh; q.kw = c.kw; q.sh = c.sh; q.sw = c.sw;
    q.ph = c.ph; q.pw = c.pw; q.dh = c.dh; q.dw = c.dw; q.zx = c.zx; q.zw = c.zw; q.zo = c.zo; q.mult = c.mult; q.shift = c.shift;
    q.lo = c.lo; q.hi = c.hi; q.K = c.kh * c.kw * c.Ci; q.M = c.Ho * c.Wo * nb; q.xs = c.xs; q.ys = c.ys; q.po = c.po;
    q.mtab = c.mtab; q.stab = c.stab; q.sgn = c.sgn;
    return q;
}

// yh_tuning.tfl_group: the plan is a DAG, and on this part a dependent launch costs 4.4 us however little it does - so independent
// convolutions that run the same register-fed kernel are launched TOGETHER. Every live entry gets its depth (longest chain of
// producers in front of it: an entry depends on the earlier writers of what it reads and, conservatively, on the earlier readers and
// writers of what it writes); the plan runs in depth order, which is a topological order; within a depth, the register-fed
// convolutions of one kernel form (same extent and k-steps) become one launch of tfl_conv_i8_direct_group with their parameter blocks in
// device memory. The 136-op model: the five levels' tower convolutions, their fifteen output convolutions and the FPN's three output
// convolutions are three launches instead of twenty-three. Same kernels on the same operands: same bytes.
// ---- the depth of every plan entry (dead ones: 0)
std::vector<int> plan_depths(const yh_tfl* h) {
    struct Range { const char* lo; const char* hi; };
    std::vector<Range> al;
    for (size_t i = 0; i < h->tens.size(); ++i)
        if (h->tens[i] && !h->alias[i]) al.push_back(Range{ (const char*)h->tens[i], (const char*)h->tens[i] + tensor_alloc_bytes(h, i) });
    auto alloc_of = [&](const void* q) -> int {
        for (size_t i = 0; i < al.size(); ++i) if ((const char*)q >= al[i].lo && (const char*)q < al[i].hi) return (int)i;
        return -1;
    };
    const int np = (int)h->plan.size();
    std::vector<std::vector<int>> writers(al.size()), readers(al.size());
    std::vector<EntryIo> io((size_t)np);
    std::vector<int> depth((size_t)np, 0);
    for (int i = 0; i < np; ++i) {
        if (h->plan[i].dead) continue;
        entry_io(h->plan[i], io[i]);
        int dmax = 0;
        for (const void* q : io[i].rd) { const int a = alloc_of(q); if (a >= 0) for (int w : writers[a]) dmax = std::max(dmax, depth[w] + 1); }
        for (const void* q : io[i].wr) {
            const int a = alloc_of(q);
            if (a < 0) continue;
            for (int r : readers[a]) if (r != i) dmax = std::max(dmax, depth[r] + 1);
            // (writers of other PARTS of one allocation - CONCATENATION parts written in place - are independent of each other; a writer of the
            // same bytes is not)
            for (int w : writers[a])
                for (const void* q2 : io[w].wr) if (q2 == q) dmax = std::max(dmax, depth[w] + 1);
        }
        depth[i] = dmax;
        for (const void* q : io[i].rd) { const int a = alloc_of(q); if (a >= 0) readers[a].push_back(i); }
        for (const void* q : io[i].wr) { const int a = alloc_of(q); if (a >= 0) writers[a].push_back(i); }
    }
    return depth;
}
// ---- a group's parameter blocks and tile prefix table for `nb` images, in device memory the handle owns (uploaded with blocking
// copies: never inside a capture window, never behind a launch of the invoke that needs them - run_plan calls group_tables first)
int group_tables_of(yh_tfl* h, yh_tfl::ConvGroup& g, int nb) {
    if (g.probs[nb - 1]) return YH_OK;
    std::vector<ConvI8> probs;
    std::vector<int> start(1, 0);
    long long total = 0;
    for (int mi : g.members) {
        probs.push_back(conv_i8_args(h->plan[mi], nb));
        total += (long long)((probs.back().M + 15) / 16) * ((probs.back().Co + 15) / 16);
        if (total > INT_MAX) return h->fail(YH_EINVAL, "a convolution group's tiles at this image count exceed a 32-bit grid");
        start.push_back((int)total);
    }
    if (int rc = upload(h, probs.data(), probs.size(), "conv group", &g.probs[nb - 1])) return rc;
    if (int rc = upload(h, start.data(), start.size(), "conv group", &g.tile_start[nb - 1])) return rc;
    g.tiles[nb - 1] = start.back();
    return YH_OK;
}
int group_tables(yh_tfl* h, int nb) {
    for (yh_tfl::ConvGroup& g : h->groups) if (int rc = group_tables_of(h, g, nb)) return rc;
    return YH_OK;
}
// ---- the entries of one depth (in execution order): those that run the register-fed kernel, bucketed by its form, as groups of 2 to kMaxGroup.
// Membership is decided at two images whatever max_images is: the groups of a handle are the same at every image count.
int group_one_depth(yh_tfl* h, const int* first, const int* last) {
    std::map<int, std::vector<int>> byform;   // (key: the form, then the signedness - a uint8 and an int8 convolution never share a group)
    for (const int* k = first; k != last; ++k) {
        const Prepared& p = h->plan[*k];
        if (p.kind == P_CONV_I8 && h->use_dot >= 3 && conv_i8_direct_pays(conv_i8_args(p, 2))) byform[2 * p.form + p.conv.sgn].push_back(*k);
    }
    for (auto& kv : byform) {
        std::vector<int>& v = kv.second;
        for (size_t c0 = 0; c0 + 1 < v.size(); c0 += kMaxGroup) {
            const size_t c1 = std::min(v.size(), c0 + (size_t)kMaxGroup);
            if (c1 - c0 < 2) break;
            yh_tfl::ConvGroup g;
            g.members.assign(v.begin() + c0, v.begin() + c1);
            g.probs.assign((size_t)h->max_images, nullptr); g.tile_start.assign((size_t)h->max_images, nullptr); g.tiles.assign((size_t)h->max_images, 0);
            for (int nb = 1; nb <= std::min(2, h->max_images); ++nb)
                if (int rc = group_tables_of(h, g, nb)) return rc;
            for (int mi : g.members) h->plan[mi].group = (int)h->groups.size();
            h->groups.push_back(g);
        }
    }
    return YH_OK;
}
int group_plan(yh_tfl* h) {
    const std::vector<int> depth = plan_depths(h);
    h->order.clear();
    for (int i = 0; i < (int)h->plan.size(); ++i) if (!h->plan[i].dead) h->order.push_back(i);
    std::stable_sort(h->order.begin(), h->order.end(), [&](int a, int b) { return depth[a] < depth[b]; });
    for (size_t a = 0; a < h->order.size();) {   // consecutive runs of one depth in `order`
        size_t b = a;
        while (b < h->order.size() && depth[h->order[b]] == depth[h->order[a]]) ++b;
        if (int rc = group_one_depth(h, h->order.data() + a, h->order.data() + b)) return rc;
        a = b;
    }
    return YH_OK;
}

// Whether a P_CONV_I8 entry runs the register-fed kernel (its own launch or its group's) for `nb` images, else the LDS tiles.
bool conv_i8_runs_direct(const yh_tfl* h, const Prepared& p, int nb) {
    return p.group >= 0 || (h->use_dot >= 3 && conv_i8_direct_pays(conv_i8_args(p, nb)));
}
// Whether a plan entry issues a launch of its own: it is not folded into another (fuse_plan), and a group is launched by its first member.
bool launches(const yh_tfl* h, size_t pi) { const Prepared& p = h->plan[pi]; return !p.dead && (p.group < 0 || h->groups[p.group].members[0] == (int)pi); }

int enqueue_plan(yh_tfl* h) {
    const hipStream_t s = h->stream;
    const unsigned nb = (unsigned)h->nb;   // images of this invoke: activations are image-major, so element-wise ops just see nb x the elements
    TraceRange tr_all("yh_tfl:plan(enqueue)");
    for (size_t oi = 0; oi < h->order.size(); ++oi) {
        const size_t pi = (size_t)h->order[oi];   // (execution order: by depth of the plan's DAG where convolutions are grouped, else the file's)
        if (!launches(h, pi)) continue;
        const Prepared& p = h->plan[pi];
        static const char* kind_name[] = { "CONV_2D", "DEPTHWISE_CONV_2D", "ADD", "RELU/QUANTIZE", "QUANTIZE(f32)", "DEQUANTIZE", "TANH", "PAD", "RESIZE_BILINEAR", "CONCATENATION", "RESHAPE(copy)", "CONV_2D(int8 MFMA)" };
        TraceRange tr(kind_name[p.kind]);   // (roctx: one range per operator, named by its TFLite op; a no-op unless a tracer is attached)
        switch (p.kind) {
            case P_CONV: launch_conv_u8(p.conv, h->use_dot != 0, nb, s); break;
            case P_CONV_I8: {
                const yh_tfl::ConvGroup* g = p.group >= 0 ? &h->groups[p.group] : nullptr;
                const ConvI8 q = conv_i8_args(p, (int)nb);
                if (g) launch_conv_i8_direct_group(p.form, p.conv.sgn != 0, g->probs[nb - 1], g->tile_start[nb - 1], (int)g->members.size(), g->tiles[nb - 1], s);
                else if (conv_i8_runs_direct(h, p, (int)nb)) launch_conv_i8_direct(p.form, q, s);
                else launch_conv_i8_mfma(q, s);
                break;
            }
            case P_DW: launch_dwconv_u8(p.conv, h->use_dot != 0, nb, s); break;
            case P_ADD: launch_add_u8(p.add, nb, s); break;
            case P_REQUANT: launch_requant_u8((const uint8_t*)p.src, (uint8_t*)p.dst, p.n * nb, p.zi, p.zo, p.m, p.s, p.lo, p.hi, s, p.sgn_in); break;
            case P_QUANT_F32: launch_quantize_f32((const float*)p.src, (uint8_t*)p.dst, p.n * nb, p.scale, p.zo, s, p.sgn_out); break;
            case P_DEQUANT: launch_dequantize_u8((const uint8_t*)p.src, (float*)p.dst, p.n * nb, p.scale, p.zi, s, p.sgn_in); break;
            case P_LUT: launch_lut_u8((const uint8_t*)p.src, (uint8_t*)p.dst, p.n * nb, p.lut, s); break;
            case P_PAD: launch_pad_u8(p.pad, nb, s); break;
            case P_RESIZE: launch_resize_bilinear_u8(p.rs, nb, s); break;
            case P_CONCAT: for (const CatQ& c : p.cat) launch_concat_part(c, nb, s); break;
            case P_COPY: launch_copy_bytes((const uint8_t*)p.src, (uint8_t*)p.dst, p.n * nb, s); break;
        }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return h->fail(YH_EHIP, std::string("tflite plan launch: ") + hipGetErrorString(e));
    return YH_OK;
}
// yh_tuning.tfl_graph: 0 eager launches (default), 1 the plan as one captured hipGraph (with a 4-byte memset captured on
// a side stream beside it, so that the graph has two branches). Per invoke on the 136-op model (set_input + invoke + read
// output 4, median of 300): eager 1.104 ms, two-branch graph 1.222 ms, single-branch graph 1.096 ms - the step is bound by
// kernel time, not by launches, and the one graph form that is not slower is the one that cannot ship:
// round 1 shipped eager launches because `rocprofv3 --kernel-trace` crashed inside hipGraphLaunch on the graph. The cause
// (round 2, profiles/r02_graph_replay_under_rocprofv3.md with the logs) is not the plan: the HIP runtime replays a
// SINGLE-BRANCH graph from AQL packets it pre-built at instantiation, and rocprofv3's queue interception faults on that
// path - the YOLACT engine's own step crashes the same way when captured without a second branch, every forked capture is
// fine, and so is the single-branch form with DEBUG_CLR_GRAPH_PACKET_CAPTURE=0. The same replay path later produced a GPU
// memory access fault WITHOUT the profiler (engine.hip, enqueue_all), so this library never builds a single-branch graph.
int run_plan(yh_tfl* h) {
    if (int rc = group_tables(h, h->nb)) return rc;   // (an image count's first invoke: before the capture and before any launch)
    h->det_last = nullptr;   // (detections of an earlier invoke are no longer the handle's state)
    if (!h->use_graph) { const int rc = enqueue_plan(h); if (!rc) h->last_nb = h->nb; return rc; }
    hipGraphExec_t& gexec = h->gexecs[h->nb - 1];
    if (!gexec) {
        hipGraph_t g = nullptr;
        TCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed));
        // Inside the capture window nothing returns early: a failure is collected, the side stream is joined and the capture
        // is ENDED in every case (a stream left capturing would fail every later call on the handle).
        hipError_t ce = hipSuccess;
        const char* where = "";
        auto step = [&](hipError_t e, const char* what) { if (ce == hipSuccess && e != hipSuccess) { ce = e; where = what; } };
        // a second branch: the runtime then replays the graph node by node (see above)
        step(hipEventRecord(h->ev_fork, h->stream), "fork record");
        step(hipStreamWaitEvent(h->side, h->ev_fork, 0), "fork wait");
        step(launch_side_touch((unsigned*)h->side_word, h->side), "side branch");   // (a kernel node: no memset node in any capture)
        step(hipEventRecord(h->ev_join, h->side), "join record");
        const int rc = ce == hipSuccess ? enqueue_plan(h) : YH_OK;
        step(hipStreamWaitEvent(h->stream, h->ev_join, 0), "join wait");   // (also after a failed enqueue: an unjoined fork invalidates the capture)
        const hipError_t e = hipStreamEndCapture(h->stream, &g);
        if (rc || ce != hipSuccess || e != hipSuccess || !g) {
            if (g) hipGraphDestroy(g);
            (void)hipGetLastError();
            if (rc) return rc;   // (enqueue_plan has set the message)
            return h->fail(YH_EHIP, ce != hipSuccess ? std::string("tflite plan capture (") + where + "): " + hipGetErrorString(ce)
                                                     : std::string("tflite plan capture: ") + hipGetErrorString(e));
        }
        const hipError_t ei = hipGraphInstantiate(&gexec, g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        if (ei != hipSuccess) { gexec = nullptr; return h->fail(YH_EHIP, std::string("tflite plan instantiate: ") + hipGetErrorString(ei)); }
    }
    TCHK(h, hipGraphLaunch(gexec, h->stream));
    h->last_nb = h->nb;
    return YH_OK;
}

void fill_info(const TflTensor& t, yh_tensor_info* info) {
    info->name = t.name.c_str();
    info->kind = t.type == TFL_U8 ? YH_KIND_U8 : (t.type == TFL_F32 ? YH_KIND_F32 : t.type);
    info->ndims = (int)(t.shape.size() < 4 ? t.shape.size() : 4);
    for (int d = 0; d < 4; ++d) info->dims[d] = d < (int)t.shape.size() ? t.shape[d] : 1;
    info->scale = t.scale; info->zero_point = t.zp;
}

// yolact.rs:169-182: `n` elements of output 4 -> f32 (results[4]) at dst
int output4_to_f32(yh_tfl* h, size_t n, float* dst) {
    const TflTensor& o4 = h->m.tensors[h->m.outputs[4]];
    if (o4.type == TFL_U8) launch_dequantize_u8((const uint8_t*)h->tens[h->m.outputs[4]], dst, (long long)n, o4.scale, o4.zp, h->stream);
    else TCHK(h, hipMemcpyAsync(dst, h->tens[h->m.outputs[4]], n * 4, hipMemcpyDeviceToDevice, h->stream));
    return YH_OK;
}

// What classify asks of the model (the single call and the batch): its tile size S and the logits per cell C; nullptr: fine.
const char* classify_model_check(const yh_tfl* h, int* S_out, int* C_out) {
    const TflTensor& in = h->m.tensors[h->m.inputs[0]];
    if (in.type != TFL_U8 || in.shape.size() != 4 || in.shape[0] != 1 || in.shape[1] != in.shape[2] || in.shape[3] != 3 || in.shape[1] % 8 != 0 || in.shape[1] / 8 > 64)
        return "classify needs a [1,S,S,3] uint8 input with S % 8 == 0";
    if (h->m.outputs.size() < 5) return "classify reads output index 4 (yolact.rs:91): the model has fewer outputs";
    const TflTensor& o4 = h->m.tensors[h->m.outputs[4]];
    const int S = in.shape[1], grid = S / 8;
    const size_t cells = (size_t)grid * grid;
    if (o4.type == TFL_I8)
        return "output 4 is int8: classify reads it as uint8 or float32 only (yolact.rs:171-186) - end the model with a QUANTIZE to uint8 or a DEQUANTIZE";
    if (o4.count() % cells != 0 || o4.count() / cells < 4 || (o4.type != TFL_U8 && o4.type != TFL_F32))
        return "output 4 must hold (S/8)^2 cells of >= 4 uint8 or float32 logits";
    *S_out = S; *C_out = (int)(o4.count() / cells);
    return nullptr;
}

// A device buffer of the classify batch that only grows (the old one is freed).
int batch_grow(yh_tfl* h, void** p, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return YH_OK;
    if (*p) hipFree(*p);
    *p = nullptr; *cap = 0;
    if (hipMalloc(p, bytes) != hipSuccess) return h->fail(YH_ENOMEM, "hipMalloc classify batch");
    *cap = bytes;
    return YH_OK;
}

// ---- detection tail on the model's own outputs (DESIGN.md section 11 "TFLite detections") ----
void det_release(yh_tfl::DetSet& d) {
    for (void* q : d.bufs) hipFree(q);
    d = yh_tfl::DetSet();
}
// What the tail's kernels hold (the engine's limits: detect.hip); nullptr: fine. Nothing is touched.
const char* det_limits_check(int P, int C, int hp, int wp, int top_k, int max_dets, float conf_thresh, float nms_thresh) {
    if (P < 1) return "detect: the number of priors must be at least 1";
    if (C < 2 || C > kTdClassesMax) return "detect: conf must hold 2 .. 81 classes per prior (background first)";
    if (hp < 1 || hp > 4096 || wp < 1 || wp > 4096) return "detect: proto must be 1 .. 4096 pixels high and wide";
    if (top_k < 1 || top_k > kTdTopkMax) return "detect: top_k must be 1 .. 256 (YH_TOPK_MAX)";
    if (max_dets < 1 || max_dets > kTdDetsMax) return "detect: max_dets must be 1 .. 128 (YH_DETS_MAX)";
    if ((C - 1) * top_k > kTdSlotsMax) return "detect: (classes - 1) x top_k must not exceed 16384";
    if (!(conf_thresh >= 0.0f) || !(nms_thresh >= 0.0f)) return "detect: conf_thresh and nms_thresh must be non-negative numbers";
    return nullptr;
}
const char* det_quant_check(int kind, float scale, int zp, const char* name, std::string* why) {
    if (kind == TQ_F32) return nullptr;
    if (!(scale > 0.0f) || !std::isfinite(scale)) { *why = std::string("detect: the scale of ") + name + " must be finite and positive"; return why->c_str(); }
    if (kind == TQ_U8 ? (zp < 0 || zp > 255) : (zp < -128 || zp > 127)) { *why = std::string("detect: the zero point of ") + name + " lies outside its type's range"; return why->c_str(); }
    return nullptr;
}
// The workspaces for n images of d.p's geometry (P, C, hp, wp, top_k, max_dets set by the caller) and the priors; every buffer is
// recorded in d.bufs as it is made, so a failure half way is undone by det_release.
int det_alloc(yh_tfl* h, yh_tfl::DetSet& d, int n, const float* priors_host) {
    TflDetectParams& q = d.p;
    const size_t N = (size_t)n, Cf = (size_t)q.C - 1, px = (size_t)q.hp * q.wp;
    void* a;
#define TD_AL(field, type, count) do { a = nullptr; if (hipMalloc(&a, sizeof(type) * (size_t)(count)) != hipSuccess) { (void)hipGetLastError(); return h->fail(YH_ENOMEM, "hipMalloc detect workspaces (see yh_tfl_detect_config.max_images)"); } d.bufs.push_back(a); q.field = (type*)a; } while (0)
    TD_AL(cls_count, int, N * Cf);
    TD_AL(cand, uint2, N * Cf * q.P);
    TD_AL(surv_score, float, N * Cf * q.top_k);
    TD_AL(surv_prior, int, N * Cf * q.top_k);
    TD_AL(surv_box, float, N * Cf * q.top_k * 4);
    TD_AL(det_count, int, N);
    TD_AL(dets, yh_detection, N * q.max_dets);
    TD_AL(det_crop, float, N * q.max_dets * 4);
    TD_AL(det_csum, int, N * q.max_dets);
    TD_AL(masks, uint8_t, N * q.max_dets * px + 16);
    a = nullptr;
    if (hipMalloc(&a, sizeof(float) * N * q.max_dets * 32) != hipSuccess) { (void)hipGetLastError(); return h->fail(YH_ENOMEM, "hipMalloc detect workspaces"); }
    d.bufs.push_back(a); q.det_coef = a;
    float* pr = nullptr;
    if (hipMalloc((void**)&pr, sizeof(float) * (size_t)q.P * 4) != hipSuccess) { (void)hipGetLastError(); return h->fail(YH_ENOMEM, "hipMalloc detect priors"); }
    d.bufs.push_back(pr); q.priors = pr;
#undef TD_AL
    // the candidate counters start at zero and their one consumer (K2q) leaves them at zero; the detection counts start at zero too
    if (hipMemcpy(pr, priors_host, sizeof(float) * (size_t)q.P * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(q.cls_count, 0, sizeof(int) * N * Cf) != hipSuccess || hipMemset(q.det_count, 0, sizeof(int) * N) != hipSuccess)
        return h->fail(YH_EHIP, "detect workspace initialisation failed");
    d.max_images = n;
    d.ready = true;
    return YH_OK;
}
// The tail's four launches on the setup's tensors for the n images of the last invoke, eagerly on the handle's stream.
int det_run(yh_tfl* h, int n) {
    h->det.p.n = n;
    TraceRange tr("yh_tfl:detect");
    const hipError_t e = launch_tfl_detect(h->det.p, h->stream);
    if (e != hipSuccess) return h->fail(YH_EHIP, std::string("tflite detect: ") + hipGetErrorString(e));
    h->det_last = &h->det;
    h->det_last_n = n;
    return YH_OK;
}

}  // namespace

extern "C" {

int yh_tfl_validate(const void* model_bytes, size_t nbytes, int32_t* n_tensors, int32_t* n_ops, char* err, size_t err_cap) {
    if (!model_bytes) return YH_EINVAL;
    TflModel m;
    const bool ok = m.parse((const uint8_t*)model_bytes, nbytes);
    if (n_tensors) *n_tensors = (int32_t)m.tensors.size();
    if (n_ops) *n_ops = (int32_t)m.ops.size();
    if (err && err_cap) { strncpy(err, m.error.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    return ok ? YH_OK : YH_EWEIGHTS;
}

const char* yh_tfl_last_error(const yh_tfl* h) { return h ? h->err.c_str() : g_tfl_create_error.c_str(); }

int yh_tfl_create(const void* model_bytes, size_t nbytes, int32_t device, yh_tfl** out) {
    return yh_tfl_create_tuned(model_bytes, nbytes, device, nullptr, out);
}

int yh_tfl_create_tuned(const void* model_bytes, size_t nbytes, int32_t device, const yh_tuning* tune, yh_tfl** out) {
    return yh_tfl_create_batch_tuned(model_bytes, nbytes, device, 2, tune, out);
}

int yh_tfl_create_batch(const void* model_bytes, size_t nbytes, int32_t device, int32_t max_images, yh_tfl** out) {
    return yh_tfl_create_batch_tuned(model_bytes, nbytes, device, max_images, nullptr, out);
}

int yh_tfl_create_batch_tuned(const void* model_bytes, size_t nbytes, int32_t device, int32_t max_images, const yh_tuning* tune, yh_tfl** out) {
    if (!model_bytes || !out) { g_tfl_create_error = "null argument"; return YH_EINVAL; }
    *out = nullptr;
    if (max_images < 1 || max_images > YH_TFL_MAX_IMAGES) { g_tfl_create_error = "max_images must be 1 .. " + std::to_string(YH_TFL_MAX_IMAGES); return YH_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { g_tfl_create_error = "no such HIP device (no CPU fallback)"; return YH_EHIP; }
    yh_tfl* h = new yh_tfl();
    h->dev = device;
    h->max_images = max_images;
    h->gexecs.assign((size_t)max_images, nullptr);
    if (tune && tune->tfl_dot >= 0) h->use_dot = tune->tfl_dot;
    if (tune && tune->tfl_graph >= 0) h->use_graph = tune->tfl_graph;
    if (tune && tune->tfl_fuse >= 0) h->use_fuse = tune->tfl_fuse;
    if (tune && tune->tfl_group >= 0) h->use_group = tune->tfl_group;
    h->file.assign((const uint8_t*)model_bytes, (const uint8_t*)model_bytes + nbytes);
    auto bail = [&](int rc) { g_tfl_create_error = h->err; yh_tfl_destroy(h); return rc; };
    if (!h->m.parse(h->file.data(), h->file.size())) { h->err = "tflite parse: " + h->m.error; return bail(YH_EWEIGHTS); }
    if (h->m.inputs.size() != 1) { h->err = "expected exactly one graph input"; return bail(YH_EINVAL); }
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess || hipMalloc(&h->side_word, 16) != hipSuccess) { h->err = "device setup failed"; return bail(YH_EHIP); }
    int rc = prepare(h);
    if (rc) return bail(rc);
    // the int8 MFMA kernels fold the images into a 32-bit pixel index (ConvI8::M = Ho Wo nb, rounded up to a tile by the grid)
    for (const Prepared& p : h->plan)
        if (p.kind == P_CONV_I8 && (long long)p.conv.Ho * p.conv.Wo * max_images > INT_MAX - 64) {
            h->err = "a convolution's output pixels times max_images exceed a 32-bit index (operator " + std::to_string(p.oi) + ")";
            return bail(YH_EINVAL);
        }
    h->gone.assign(h->m.tensors.size(), 0);
    if (h->use_fuse) fuse_plan(h);
    for (int i = 0; i < (int)h->plan.size(); ++i) h->order.push_back(i);
    if (h->use_group && (rc = group_plan(h))) return bail(rc);
    *out = h;
    return YH_OK;
}

// Launches per invoke of the plan, and how many of them are CONV_2D / of those on the int8 matrix pipes.
int yh_tfl_plan_info(const yh_tfl* h, int32_t* launches_out, int32_t* conv_launches, int32_t* conv_mfma_launches) {
    if (!h) return YH_EINVAL;
    int n = 0, nc = 0, nm = 0;
    for (size_t i = 0; i < h->plan.size(); ++i) {
        const Prepared& p = h->plan[i];
        if (p.dead) continue;
        if (launches(h, i)) n += p.kind == P_CONCAT ? (int)p.cat.size() : 1;   // (a convolution launched with its group counts as a convolution, not as a launch)
        if (p.kind == P_CONV || p.kind == P_CONV_I8) ++nc;
        if (p.kind == P_CONV_I8) ++nm;
    }
    if (launches_out) *launches_out = n;
    if (conv_launches) *conv_launches = nc;
    if (conv_mfma_launches) *conv_mfma_launches = nm;
    return YH_OK;
}

// The rows of the register-fed kernel's table of forms (no device is touched).
int yh_tfl_direct_forms(int32_t* rows, int32_t cap) {
    const int n = conv_i8_direct_form_count();
    for (int i = 0; rows && i < n && i < cap; ++i) {
        int D, once, KK;
        conv_i8_direct_form_row(i, &D, &once, &KK);
        rows[3 * i] = D; rows[3 * i + 1] = once; rows[3 * i + 2] = KK;
    }
    return n;
}
// What operator `op` of the model runs on in the handle's plan, for the image count of the next invoke: the answers of the very
// functions the launches ask (conv_u8_kernel, dwconv_u8_takes_c4, conv_i8_runs_direct, launches).
int yh_tfl_op_info(const yh_tfl* h, int32_t op, int32_t* family, int32_t* form_row, int32_t* grouped, int32_t* folded) {
    if (!h || op < 0 || op >= (int)h->m.ops.size()) return YH_EINVAL;
    int fam = YH_TFL_FAM_NONE, row = -1, grp = 0, fold = 1;   // (a RESHAPE that shares its input's buffer has no plan entry)
    for (const Prepared& p : h->plan) {
        if (p.oi != op) continue;
        fold = p.dead ? 1 : 0;
        switch (p.kind) {
            case P_CONV: {
                static const int fams[] = { YH_TFL_FAM_CONV_SCALAR, YH_TFL_FAM_CONV_PX8, YH_TFL_FAM_CONV_DOT1, YH_TFL_FAM_CONV_DOT4 };
                fam = fams[conv_u8_kernel(p.conv, h->use_dot != 0)];
                break;
            }
            case P_CONV_I8:
                if (conv_i8_runs_direct(h, p, h->nb)) { fam = YH_TFL_FAM_CONV_I8_DIRECT; row = p.form; grp = p.group >= 0 ? 1 : 0; }
                else fam = YH_TFL_FAM_CONV_I8_LDS;
                break;
            case P_DW: fam = dwconv_u8_takes_c4(p.conv, h->use_dot != 0) ? YH_TFL_FAM_DW_C4 : YH_TFL_FAM_DW_SCALAR; break;
            case P_ADD: fam = YH_TFL_FAM_ADD; break;
            case P_REQUANT: fam = YH_TFL_FAM_REQUANT; break;
            case P_QUANT_F32: fam = YH_TFL_FAM_QUANTIZE_F32; break;
            case P_DEQUANT: fam = YH_TFL_FAM_DEQUANTIZE; break;
            case P_LUT: fam = YH_TFL_FAM_LUT; break;
            case P_PAD: fam = YH_TFL_FAM_PAD; break;
            case P_RESIZE: fam = YH_TFL_FAM_RESIZE; break;
            case P_CONCAT: fam = YH_TFL_FAM_CONCAT; break;
            case P_COPY: fam = YH_TFL_FAM_COPY; break;
        }
        break;
    }
    if (family) *family = fam;
    if (form_row) *form_row = row;
    if (grouped) *grouped = grp;
    if (folded) *folded = fold;
    return YH_OK;
}

// Operator `op`'s output type and whether its launch takes its multipliers from per-channel tables (the int8 convolutions do).
int yh_tfl_op_quant(const yh_tfl* h, int32_t op, int32_t* signed_act, int32_t* per_channel) {
    if (!h || op < 0 || op >= (int)h->m.ops.size() || h->m.ops[op].out.empty()) return YH_EINVAL;
    const TflTensor& y = h->m.tensors[h->m.ops[op].out[0]];
    // (an int8 convolution always reads its multipliers from tables; what is reported is whether they differ: the weights' scale vector)
    const TflOp& o = h->m.ops[op];
    const int pc = (o.code == TFL_CONV_2D || o.code == TFL_DEPTHWISE_CONV_2D) && y.type == TFL_I8 && h->m.tensors[o.in[1]].per_channel() ? 1 : 0;
    if (signed_act) *signed_act = y.type == TFL_U8 ? 0 : (y.type == TFL_I8 ? 1 : -1);
    if (per_channel) *per_channel = pc;
    return YH_OK;
}

void yh_tfl_destroy(yh_tfl* h) {
    if (!h) return;
    hipSetDevice(h->dev);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (hipGraphExec_t ge : h->gexecs) if (ge) hipGraphExecDestroy(ge);
    if (h->side) { hipStreamSynchronize(h->side); hipStreamDestroy(h->side); }
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    if (h->side_word) hipFree(h->side_word);
    for (size_t i = 0; i < h->tens.size(); ++i) if (h->tens[i] && !(i < h->alias.size() && h->alias[i])) hipFree(h->tens[i]);
    for (void* p : h->extra) hipFree(p);
    void* scratch[] = { h->frame_dev, h->codes_dev, h->stitch_dev, h->tiles_dev, h->rs_tmp, h->cells_dev, h->diverged_dev,
                        h->clsb_frames, h->clsb_cells, h->clsb_codes, h->clsb_div };
    for (void* p : scratch) if (p) hipFree(p);
    classify_geo_free(&h->clsb_geo);
    for (void* p : h->det.bufs) hipFree(p);
    for (void* p : h->opdet.bufs) hipFree(p);
    tfl_instance_free(h->inst);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

int yh_tfl_input_info(const yh_tfl* h, yh_tensor_info* info) {
    if (!h || !info) return YH_EINVAL;
    fill_info(h->m.tensors[h->m.inputs[0]], info);
    return YH_OK;
}
int yh_tfl_output_count(const yh_tfl* h) { return h ? (int)h->m.outputs.size() : YH_EINVAL; }
int yh_tfl_output_info(const yh_tfl* h, int32_t i, yh_tensor_info* info) {
    if (!h || !info || i < 0 || i >= (int)h->m.outputs.size()) return YH_EINVAL;
    fill_info(h->m.tensors[h->m.outputs[i]], info);
    return YH_OK;
}
int yh_tfl_tensor_count(const yh_tfl* h) { return h ? (int)h->m.tensors.size() : YH_EINVAL; }

int yh_tfl_set_batch(yh_tfl* h, int32_t n_images) {
    if (!h) return YH_EINVAL;
    if (n_images < 1 || n_images > h->max_images)
        return h->fail(YH_EINVAL, h->max_images == 2 ? std::string("1 or 2 images per invoke") : "1 .. " + std::to_string(h->max_images) + " images per invoke (yh_tfl_create_batch's max_images)");
    if (n_images > 1 && !h->batch_ok) return h->fail(YH_EINVAL, "an operator of this model works along the image axis: one image per invoke only");
    h->nb = n_images;
    return YH_OK;
}

int yh_tfl_set_input(yh_tfl* h, const void* data, size_t nbytes) {
    if (!h || !data) return YH_EINVAL;
    const TflTensor& t = h->m.tensors[h->m.inputs[0]];
    if (nbytes != t.count() * t.elem() * (size_t)h->nb) return h->fail(YH_EINVAL, "input size mismatch");   // the reference only warns (yolact.rs:151-158)
    h->det_last = nullptr;
    TCHK(h, hipSetDevice(h->dev));
    TCHK(h, hipMemcpyAsync(h->tens[h->m.inputs[0]], data, nbytes, hipMemcpyHostToDevice, h->stream));
    // copy_from_slice semantics (yolact.rs:161-162): the caller's buffer is free again on return. From pageable memory the
    // runtime has staged the bytes by now; from pinned / registered memory the DMA is still reading: wait for it.
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, data) == hipSuccess && at.type == hipMemoryTypeHost) TCHK(h, hipStreamSynchronize(h->stream));
    else (void)hipGetLastError();
    return YH_OK;
}
int yh_tfl_invoke(yh_tfl* h) {
    if (!h) return YH_EINVAL;
    TCHK(h, hipSetDevice(h->dev));
    TraceRange tr("yh_tfl_invoke");
    return run_plan(h);
}
int yh_tfl_tensor_read(yh_tfl* h, int32_t tensor, void* dst, size_t nbytes) {
    if (!h || !dst || tensor < 0 || tensor >= (int)h->m.tensors.size()) return YH_EINVAL;
    const TflTensor& t = h->m.tensors[tensor];
    if (tensor < (int)h->gone.size() && h->gone[tensor])
        return h->fail(YH_ESTATE, "tensor '" + t.name + "' is folded into its producer's launch and never written (yh_tuning.tfl_fuse = 0 materialises every tensor)");
    if (nbytes != t.count() * t.elem() * (size_t)(t.data ? 1 : h->nb)) return h->fail(YH_EINVAL, "tensor size mismatch (activations hold yh_tfl_set_batch images)");
    TCHK(h, hipSetDevice(h->dev));
    TCHK(h, hipMemcpyAsync(dst, h->tens[tensor], nbytes, hipMemcpyDeviceToHost, h->stream));
    TCHK(h, hipStreamSynchronize(h->stream));
    return YH_OK;
}
int yh_tfl_output_read(yh_tfl* h, int32_t i, void* dst, size_t nbytes) {
    if (!h || i < 0 || i >= (int)h->m.outputs.size()) return YH_EINVAL;
    return yh_tfl_tensor_read(h, h->m.outputs[i], dst, nbytes);
}

int yh_tfl_classify_frame_u32(yh_tfl* h, uint32_t* frame, int32_t w, int32_t hh, int32_t mode) {
    if (!h || !frame || w < 1 || hh < 1) return YH_EINVAL;
    if (mode != YH_COMPAT_STRICT && mode != YH_COMPAT_SANE) return h->fail(YH_EINVAL, "bad compat mode");
    int S = 0, C = 0;
    if (const char* why = classify_model_check(h, &S, &C)) return h->fail(YH_EINVAL, why);
    const int grid = S / 8;
    const size_t cells = (size_t)grid * grid;
    TCHK(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)w * hh;
    auto grow = [&](void** p, size_t* cap, size_t bytes) { if (bytes <= *cap) return true; if (*p) hipFree(*p); *p = nullptr; *cap = 0; if (hipMalloc(p, bytes) != hipSuccess) return false; *cap = bytes; return true; };
    const size_t tmp_need = (size_t)12 * ((size_t)w * S > (size_t)2 * S * hh ? (size_t)w * S : (size_t)2 * S * hh);
    if (!grow((void**)&h->frame_dev, &h->frame_cap, npx * 4) || !grow((void**)&h->rs_tmp, &h->rs_cap, tmp_need)) return h->fail(YH_ENOMEM, "hipMalloc scratch");
    if (!h->tiles_dev) {
        if (hipMalloc((void**)&h->tiles_dev, (size_t)2 * S * S * 3) != hipSuccess || hipMalloc((void**)&h->cells_dev, 2 * cells * C * 4) != hipSuccess ||
            hipMalloc((void**)&h->codes_dev, 2 * cells * 4) != hipSuccess || hipMalloc((void**)&h->stitch_dev, (size_t)2 * S * S * 4) != hipSuccess ||
            hipMalloc((void**)&h->diverged_dev, 8) != hipSuccess) return h->fail(YH_ENOMEM, "hipMalloc scratch");
    }
    hipStream_t s = h->stream;
    TraceRange tr("yh_tfl_classify_frame_u32");
    // yolact.rs:195-214
    TCHK(h, hipMemcpyAsync(h->frame_dev, frame, npx * 4, hipMemcpyHostToDevice, s));
    hipError_t e = launch_resize_v_u32(h->frame_dev, w, hh, h->rs_tmp, S, s);
    const int nb_saved = h->nb;
    if (h->batch_ok && h->max_images >= 2) {   // (a handle made for one image per invoke - yh_tfl_create_batch(.., 1, ..) - takes the per-tile loop below)
        // yolact.rs:216-217: the two tiles are independent - they run as ONE invoke of the batch plan (the horizontal resize
        // writes them, image-major, straight into the input tensor): half the launches per frame, twice the work per launch
        if (e == hipSuccess) e = launch_resize_h(h->rs_tmp, w, S, h->tens[h->m.inputs[0]], 2 * S, 1, s);
        if (e != hipSuccess) return h->fail(YH_EHIP, "classify pre failed");
        h->nb = 2;
        const int rc = run_plan(h);
        h->nb = nb_saved;
        if (rc) return rc;
        if (int rc2 = output4_to_f32(h, 2 * cells * C, h->cells_dev)) return rc2;   // both tiles
    } else {
        if (e == hipSuccess) e = launch_resize_h(h->rs_tmp, w, S, h->tiles_dev, 2 * S, 1, s);
        if (e != hipSuccess) return h->fail(YH_EHIP, "classify pre failed");
        h->nb = 1;
        for (int t = 0; t < 2; ++t) {   // one invoke per tile (an operator of this model works along the image axis, or the handle holds one image)
            TCHK(h, hipMemcpyAsync(h->tens[h->m.inputs[0]], h->tiles_dev + (size_t)t * S * S * 3, (size_t)S * S * 3, hipMemcpyDeviceToDevice, s));
            int rc = run_plan(h);
            if (!rc) rc = output4_to_f32(h, cells * C, h->cells_dev + (size_t)t * cells * C);
            if (rc) { h->nb = nb_saved; return rc; }
        }
        h->nb = nb_saved;
    }
    e = launch_cells_postprocess(h->cells_dev, 2, grid, C, mode, h->codes_dev, h->diverged_dev, s);   // yolact.rs:90-131
    if (e == hipSuccess) e = launch_upsample_codes(h->codes_dev, 2, grid, h->stitch_dev, 1, s);        // :127-128, :219-220
    if (e == hipSuccess) e = launch_resize_v_u32(h->stitch_dev, 2 * S, S, h->rs_tmp, hh, s);            // :222-231
    if (e == hipSuccess) e = launch_resize_h(h->rs_tmp, 2 * S, hh, h->frame_dev, w, 2, s);
    if (e != hipSuccess) return h->fail(YH_EHIP, "classify post failed");
    int div[2] = { 0, 0 };
    TCHK(h, hipMemcpyAsync(div, h->diverged_dev, 8, hipMemcpyDeviceToHost, s));
    TCHK(h, hipStreamSynchronize(s));
    if (div[0] || div[1]) return h->fail(YH_EDIVERGE, "reference flood fill (yolact.rs:57-78) does not terminate on this frame");
    TCHK(h, hipMemcpy(frame, h->frame_dev, npx * 4, hipMemcpyDeviceToHost));
    return YH_OK;
}

// Yolact::classify on n frames as ONE invoke of 2n images (DESIGN.md section 11 "TFLite classify batch"): the engine's batch
// (classify_batch.hip) with this executor in the middle - the same pre / post kernels through classify_geo.h, the same host logic.
int yh_tfl_classify_batch_u32(yh_tfl* h, const uint32_t* frames, int32_t frames_on_device, int32_t n, int32_t w, int32_t hh, int32_t mode,
                              uint32_t* out_host, int32_t* diverged_host) {
    if (!h || !frames) return YH_EINVAL;
    if (n < 1) return h->fail(YH_EINVAL, "classify batch: n_frames must be at least 1");
    if (w < 1 || hh < 1) return h->fail(YH_EINVAL, "classify batch: bad frame size");
    if (mode != YH_COMPAT_STRICT && mode != YH_COMPAT_SANE) return h->fail(YH_EINVAL, "bad compat mode");
    int S = 0, C = 0;
    if (const char* why = classify_model_check(h, &S, &C)) return h->fail(YH_EINVAL, why);
    if (!h->batch_ok)
        return h->fail(YH_EINVAL, "an operator of this model works along the image axis (one image per invoke): classify its frames one by one with yh_tfl_classify_frame_u32");
    if (n > h->max_images / 2) return h->fail(YH_EINVAL, "classify batch: 2 n_frames images exceed the handle's max_images (yh_tfl_create_batch)");
    TCHK(h, hipSetDevice(h->dev));
    TraceRange tr("yh_tfl_classify_batch_u32");
    const int grid = S / 8;
    const size_t cells = (size_t)grid * grid, npx = (size_t)w * hh, nt = (size_t)2 * n;
    const hipStream_t s = h->stream;
    h->clsb_n = -1;   // (until this batch is complete there is none: the buffers below may move)
    int rc;
    if ((rc = batch_grow(h, (void**)&h->clsb_frames, &h->clsb_frames_cap, (size_t)n * npx * 4))) return rc;
    if ((rc = batch_grow(h, (void**)&h->clsb_cells, &h->clsb_cells_cap, nt * cells * C * 4))) return rc;
    if ((rc = batch_grow(h, (void**)&h->clsb_codes, &h->clsb_codes_cap, nt * cells * 4))) return rc;
    if ((rc = batch_grow(h, (void**)&h->clsb_div, &h->clsb_div_cap, nt * 4))) return rc;
    hipError_t e = classify_geo_ensure(&h->clsb_geo, w, hh, S, s);
    if (e == hipErrorOutOfMemory) return h->fail(YH_ENOMEM, "hipMalloc classify batch tables");
    if (e != hipSuccess) return h->fail(YH_EHIP, std::string("classify batch tables: ") + hipGetErrorString(e));
    // yolact.rs:195-214 per frame: unpack, resize_exact(2S, S), crop two tiles -> images 2b, 2b + 1 of the model's input tensor
    const uint32_t* src = frames;
    if (!frames_on_device) {
        TCHK(h, hipMemcpyAsync(h->clsb_frames, frames, (size_t)n * npx * 4, hipMemcpyHostToDevice, s));
        src = h->clsb_frames;
    }
    TCHK(h, classify_geo_pre(h->clsb_geo, src, n, (uint8_t*)h->tens[h->m.inputs[0]], s));
    // yolact.rs:216-217 + :163: the 2n tiles as one invoke (the caller's yh_tfl_set_batch value survives)
    const int nb_saved = h->nb;
    h->nb = 2 * n;
    rc = run_plan(h);
    h->nb = nb_saved;
    if (rc) return rc;
    // yolact.rs:169-189 (results[4] as f32), :90-131, :219-233
    if ((rc = output4_to_f32(h, nt * cells * C, h->clsb_cells))) return rc;
    e = launch_cells_postprocess(h->clsb_cells, 2 * n, grid, C, mode, h->clsb_codes, h->clsb_div, s);
    if (e != hipSuccess) return h->fail(YH_EHIP, std::string("classify batch post: ") + hipGetErrorString(e));
    TCHK(h, classify_geo_post(h->clsb_geo, h->clsb_codes, n, h->clsb_frames, s));
    // the read of the 2n flags (and of the frames) and the one wait. STRICT holds the frames back until the flags are known:
    // out_host stays untouched when a frame diverges.
    std::vector<int> div(nt);
    TCHK(h, hipMemcpyAsync(div.data(), h->clsb_div, nt * 4, hipMemcpyDeviceToHost, s));
    const bool early = out_host && mode == YH_COMPAT_SANE;   // (SANE never diverges)
    if (early) TCHK(h, hipMemcpyAsync(out_host, h->clsb_frames, (size_t)n * npx * 4, hipMemcpyDeviceToHost, s));
    TCHK(h, hipStreamSynchronize(s));
    bool any = false;
    for (int b = 0; b < n; ++b) {
        const int d = (div[2 * b] || div[2 * b + 1]) ? 1 : 0;
        if (diverged_host) diverged_host[b] = d;
        any = any || d;
    }
    if (any) return h->fail(YH_EDIVERGE, "reference flood fill (yolact.rs:57-78) does not terminate on a frame of this batch");
    if (out_host && !early) TCHK(h, hipMemcpy(out_host, h->clsb_frames, (size_t)n * npx * 4, hipMemcpyDeviceToHost));
    h->clsb_n = n;
    return YH_OK;
}

const uint32_t* yh_tfl_classify_batch_device_frames(const yh_tfl* h) { return h && h->clsb_n >= 1 ? h->clsb_frames : nullptr; }

void yh_tfl_default_detect_config(yh_tfl_detect_config* cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    for (int i = 0; i < 4; ++i) cfg->outputs[i] = i;
    cfg->top_k = 200; cfg->max_dets = 100;
    cfg->conf_thresh = 0.05f; cfg->nms_thresh = 0.5f;
}

int yh_tfl_detect_setup(yh_tfl* h, const yh_tfl_detect_config* cfg, const float* priors_host, int32_t n_priors) {
    if (!h || !cfg || !priors_host) return YH_EINVAL;
    // every rule first: a refused setup has touched nothing, and an earlier setup stays
    static const char* role[4] = { "loc", "conf", "mask", "proto" };
    const TflTensor* t[4];
    for (int i = 0; i < 4; ++i) {
        if (cfg->outputs[i] < 0 || cfg->outputs[i] >= (int)h->m.outputs.size())
            return h->fail(YH_EINVAL, std::string("detect setup: outputs[") + role[i] + "] is not an index into the model's outputs");
        t[i] = &h->m.tensors[h->m.outputs[cfg->outputs[i]]];
        if (t[i]->type != TFL_U8 && t[i]->type != TFL_I8 && t[i]->type != TFL_F32)
            return h->fail(YH_EINVAL, std::string("detect setup: ") + role[i] + " ('" + t[i]->name + "') must be uint8, int8 or float32");
        // (a constant is stored once, not per image - tensor_alloc_bytes - and the tail strides over images; a graph output is never
        // folded away by fuse_plan, which counts it as a reader, so there is no "never written" case to refuse)
        if (t[i]->data)
            return h->fail(YH_EINVAL, std::string("detect setup: ") + role[i] + " ('" + t[i]->name + "') is a constant of the model, not a tensor an invoke writes");
        if (t[i]->type != TFL_F32 && (t[i]->per_channel() || t[i]->zps.size() > 1))
            return h->fail(YH_EINVAL, std::string("detect setup: ") + role[i] + " ('" + t[i]->name + "') is quantised per channel: a head tensor needs one scale and zero point");
    }
    for (int i = 0; i < 4; ++i) if (cfg->reserved[i] != 0) return h->fail(YH_EINVAL, "detect setup: reserved fields must be zero");
    const std::vector<int>&ls = t[0]->shape, &cs = t[1]->shape, &ms = t[2]->shape, &ps = t[3]->shape;
    if (ls.size() != 3 || ls[0] != 1 || ls[2] != 4) return h->fail(YH_EINVAL, "detect setup: loc must be [1,P,4]");
    if (cs.size() != 3 || cs[0] != 1 || cs[2] < 2) return h->fail(YH_EINVAL, "detect setup: conf must be [1,P,C] with C >= 2");
    if (ms.size() != 3 || ms[0] != 1 || ms[2] != 32) return h->fail(YH_EINVAL, "detect setup: mask must be [1,P,32] (a model with another number of prototypes, or transposed heads, is not supported)");
    if (ps.size() != 4 || ps[0] != 1 || ps[3] != 32) return h->fail(YH_EINVAL, "detect setup: proto must be [1,hp,wp,32] (a model with another number of prototypes, or transposed heads, is not supported)");
    if (ls[1] != cs[1] || ls[1] != ms[1]) return h->fail(YH_EINVAL, "detect setup: loc, conf and mask disagree on the number of priors P");
    if (ls[1] != n_priors) return h->fail(YH_EINVAL, "detect setup: n_priors is " + std::to_string(n_priors) + ", the model's heads hold P = " + std::to_string(ls[1]));
    if (const char* why = det_limits_check(ls[1], cs[2], ps[1], ps[2], cfg->top_k, cfg->max_dets, cfg->conf_thresh, cfg->nms_thresh)) return h->fail(YH_EINVAL, why);
    TflHead hd[4];
    for (int i = 0; i < 4; ++i) {
        hd[i].p = h->tens[h->m.outputs[cfg->outputs[i]]];
        hd[i].kind = t[i]->type == TFL_U8 ? TQ_U8 : (t[i]->type == TFL_I8 ? TQ_I8 : TQ_F32);
        hd[i].scale = t[i]->type == TFL_F32 ? 1.0f : t[i]->scale;
        hd[i].zp = t[i]->type == TFL_F32 ? 0 : t[i]->zp;
        hd[i].stride = (long long)t[i]->count();
        std::string why;
        if (det_quant_check(hd[i].kind, hd[i].scale, hd[i].zp, role[i], &why)) return h->fail(YH_EINVAL, why);
    }
    if (cfg->max_images < 0 || cfg->max_images > h->max_images) return h->fail(YH_EINVAL, "detect setup: max_images must be 0 (the handle's) .. the handle's max_images");
    const int mi = cfg->max_images ? cfg->max_images : h->max_images;
    if (mi > 1 && !h->batch_ok) return h->fail(YH_EINVAL, "detect setup: an operator of this model works along the image axis (one image per invoke): set max_images = 1");
    TCHK(h, hipSetDevice(h->dev));
    yh_tfl::DetSet nd;
    nd.p.loc = hd[0]; nd.p.conf = hd[1]; nd.p.mask = hd[2]; nd.p.proto = hd[3];
    nd.p.P = ls[1]; nd.p.C = cs[2]; nd.p.hp = ps[1]; nd.p.wp = ps[2];
    nd.p.top_k = cfg->top_k; nd.p.max_dets = cfg->max_dets;
    nd.p.conf_thresh = cfg->conf_thresh; nd.p.nms_thresh = cfg->nms_thresh;
    nd.p.int_mask = hd[2].kind != TQ_F32 && hd[3].kind != TQ_F32 ? 1 : 0;
    if (int rc = det_alloc(h, nd, mi, priors_host)) { det_release(nd); return rc; }
    // a second setup replaces the first (whose launches, if any are in flight, finish first)
    if (hipStreamSynchronize(h->stream) != hipSuccess) { det_release(nd); return h->fail(YH_EHIP, "detect setup: hipStreamSynchronize failed"); }
    if (h->det_last == &h->det) h->det_last = nullptr;
    det_release(h->det);
    h->det = nd;
    return YH_OK;
}

int yh_tfl_evaluate(yh_tfl* h) {
    if (!h) return YH_EINVAL;
    if (!h->det.ready) return h->fail(YH_ESTATE, "yh_tfl_evaluate before yh_tfl_detect_setup");
    if (h->nb > h->det.max_images) return h->fail(YH_EINVAL, "the batch exceeds the detect setup's max_images");
    TCHK(h, hipSetDevice(h->dev));
    TraceRange tr("yh_tfl_evaluate");
    if (int rc = run_plan(h)) return rc;
    return det_run(h, h->last_nb);
}

int yh_tfl_detect(yh_tfl* h) {
    if (!h) return YH_EINVAL;
    if (!h->det.ready) return h->fail(YH_ESTATE, "yh_tfl_detect before yh_tfl_detect_setup");
    if (h->last_nb < 1) return h->fail(YH_ESTATE, "yh_tfl_detect before any invoke");
    if (h->last_nb > h->det.max_images) return h->fail(YH_EINVAL, "the last invoke's batch exceeds the detect setup's max_images");
    TCHK(h, hipSetDevice(h->dev));
    return det_run(h, h->last_nb);
}

int yh_tfl_read_detections(yh_tfl* h, int32_t image, int32_t* count, yh_detection* dets, int32_t cap, uint8_t* masks, size_t masks_cap) {
    if (!h || !count) return YH_EINVAL;
    if (!h->det_last) return h->fail(YH_ESTATE, "no detections: yh_tfl_evaluate / yh_tfl_detect has not run since the last yh_tfl_set_input or invoke");
    if (image < 0 || image >= h->det_last_n) return h->fail(YH_EINVAL, "image out of range");
    const TflDetectParams& q = h->det_last->p;
    TCHK(h, hipSetDevice(h->dev));
    TraceRange tr("yh_tfl_read_detections");
    TCHK(h, hipStreamSynchronize(h->stream));
    int nd = 0;
    TCHK(h, hipMemcpy(&nd, q.det_count + image, 4, hipMemcpyDeviceToHost));
    *count = nd;
    if (dets) {
        if (cap < nd) return h->fail(YH_EINVAL, "dets capacity too small");
        TCHK(h, hipMemcpy(dets, q.dets + (size_t)image * q.max_dets, sizeof(yh_detection) * (size_t)nd, hipMemcpyDeviceToHost));
    }
    if (masks) {
        const size_t px = (size_t)q.hp * q.wp;
        if (masks_cap < px * nd) return h->fail(YH_EINVAL, "masks capacity too small");
        TCHK(h, hipMemcpy(masks, q.masks + (size_t)image * q.max_dets * px, px * nd, hipMemcpyDeviceToHost));
    }
    return YH_OK;
}

int yh_tfl_proto_dims(const yh_tfl* h, int32_t dims[2]) {
    if (!h || !dims || !h->det.ready) return YH_EINVAL;
    dims[0] = h->det.p.hp; dims[1] = h->det.p.wp;
    return YH_OK;
}
const yh_detection* yh_tfl_detections_device(const yh_tfl* h) { return h && h->det.ready ? h->det.p.dets : nullptr; }
const int32_t* yh_tfl_detection_counts_device(const yh_tfl* h) { return h && h->det.ready ? h->det.p.det_count : nullptr; }
const uint8_t* yh_tfl_masks_device(const yh_tfl* h) { return h && h->det.ready ? h->det.p.masks : nullptr; }

// The setup's tail on the outputs of the last invoke, `reps` times, each of its launches between two events: ms per launch (mean).
int yh_tfl_detect_stage_times(yh_tfl* h, int32_t reps, float* ms_out) {
    if (!h || !ms_out || reps < 1) return YH_EINVAL;
    if (!h->det.ready) return h->fail(YH_ESTATE, "yh_tfl_detect_stage_times before yh_tfl_detect_setup");
    if (h->last_nb < 1) return h->fail(YH_ESTATE, "yh_tfl_detect_stage_times before any invoke");
    if (h->last_nb > h->det.max_images) return h->fail(YH_EINVAL, "the last invoke's batch exceeds the detect setup's max_images");
    TCHK(h, hipSetDevice(h->dev));
    const int ns = tfl_detect_launch_count();
    std::vector<hipEvent_t> ev((size_t)ns + 1, nullptr);
    for (hipEvent_t& e : ev) if (hipEventCreate(&e) != hipSuccess) { for (hipEvent_t& f : ev) if (f) hipEventDestroy(f); return h->fail(YH_EHIP, "hipEventCreate"); }
    std::vector<double> sum((size_t)ns, 0.0);
    h->det.p.n = h->last_nb;
    hipError_t e = hipSuccess;
    for (int r = 0; r < reps && e == hipSuccess; ++r) {
        e = hipEventRecord(ev[0], h->stream);
        for (int st = 0; st < ns && e == hipSuccess; ++st) {
            e = launch_tfl_detect_stage(h->det.p, st, h->stream);
            if (e == hipSuccess) e = hipEventRecord(ev[(size_t)st + 1], h->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        for (int st = 0; st < ns && e == hipSuccess; ++st) { float ms = 0.0f; e = hipEventElapsedTime(&ms, ev[(size_t)st], ev[(size_t)st + 1]); sum[(size_t)st] += ms; }
    }
    for (hipEvent_t& f : ev) hipEventDestroy(f);
    if (e != hipSuccess) return h->fail(YH_EHIP, std::string("detect stage times: ") + hipGetErrorString(e));
    for (int st = 0; st < ns; ++st) ms_out[st] = (float)(sum[(size_t)st] / reps);
    h->det_last = &h->det;
    h->det_last_n = h->last_nb;
    return YH_OK;
}

// The tail on caller-provided bytes, no model involved (include/yolact_hip_debug.h): buffers and workspaces of its own, kept from one
// call to the next of the same geometry, kinds and limits (as they were left), made anew by any other call.
int yh_tfl_op_detect(yh_tfl* h, int32_t n, int32_t P, int32_t C, int32_t hp, int32_t wp,
                     const void* loc, int32_t loc_kind, float loc_scale, int32_t loc_zp,
                     const void* conf, int32_t conf_kind, float conf_scale, int32_t conf_zp,
                     const void* mask, int32_t mask_kind, float mask_scale, int32_t mask_zp,
                     const void* proto, int32_t proto_kind, float proto_scale, int32_t proto_zp,
                     const float* priors, int32_t top_k, int32_t max_dets, float conf_thresh, float nms_thresh) {
    if (!h || !loc || !conf || !mask || !proto || !priors) return YH_EINVAL;
    if (n < 1 || n > YH_TFL_MAX_IMAGES) return h->fail(YH_EINVAL, "detect op: n must be 1 .. YH_TFL_MAX_IMAGES");
    if (const char* why = det_limits_check(P, C, hp, wp, top_k, max_dets, conf_thresh, nms_thresh)) return h->fail(YH_EINVAL, why);
    static const char* role[4] = { "loc", "conf", "mask", "proto" };
    const void* src[4] = { loc, conf, mask, proto };
    const int kinds[4] = { loc_kind, conf_kind, mask_kind, proto_kind };
    const float scales[4] = { loc_scale, conf_scale, mask_scale, proto_scale };
    const int zps[4] = { loc_zp, conf_zp, mask_zp, proto_zp };
    const long long per[4] = { (long long)P * 4, (long long)P * C, (long long)P * 32, (long long)hp * wp * 32 };
    TflHead hd[4];
    for (int i = 0; i < 4; ++i) {
        if (kinds[i] != YH_KIND_U8 && kinds[i] != YH_KIND_I8 && kinds[i] != YH_KIND_F32) return h->fail(YH_EINVAL, std::string("detect op: ") + role[i] + " must be YH_KIND_U8, YH_KIND_I8 or YH_KIND_F32");
        hd[i].kind = kinds[i] == YH_KIND_U8 ? TQ_U8 : (kinds[i] == YH_KIND_I8 ? TQ_I8 : TQ_F32);
        hd[i].scale = hd[i].kind == TQ_F32 ? 1.0f : scales[i];
        hd[i].zp = hd[i].kind == TQ_F32 ? 0 : zps[i];
        hd[i].stride = per[i];
        std::string why;
        if (det_quant_check(hd[i].kind, hd[i].scale, hd[i].zp, role[i], &why)) return h->fail(YH_EINVAL, why);
    }
    TCHK(h, hipSetDevice(h->dev));
    TCHK(h, hipStreamSynchronize(h->stream));
    if (h->det_last == &h->opdet) h->det_last = nullptr;
    yh_tfl::DetSet& d = h->opdet;
    // A call of the geometry, kinds and limits of the one before runs on that call's buffers and workspaces AS THEY WERE LEFT
    // (counters, survivor slots, masks): what a handle's second evaluate meets. Any other call makes them anew.
    const std::vector<int> sig = { n, P, C, hp, wp, top_k, max_dets, hd[0].kind, hd[1].kind, hd[2].kind, hd[3].kind };
    const bool reuse = d.ready && d.sig == sig;
    if (!reuse) det_release(d);
    for (int i = 0; i < 4; ++i) {   // (16 bytes behind each tensor, as the executor's own allocations have: K1q's last dword may reach past the last byte)
        const size_t bytes = (size_t)per[i] * (size_t)n * (hd[i].kind == TQ_F32 ? 4 : 1);
        void* a = reuse ? d.bufs[i] : nullptr;
        if (!reuse) {
            if (hipMalloc(&a, bytes + 16) != hipSuccess) { (void)hipGetLastError(); det_release(d); return h->fail(YH_ENOMEM, "hipMalloc detect op tensors"); }
            d.bufs.push_back(a);
        }
        if (hipMemcpy(a, src[i], bytes, hipMemcpyHostToDevice) != hipSuccess) { det_release(d); return h->fail(YH_EHIP, "detect op upload failed"); }
        hd[i].p = a;
    }
    d.p.loc = hd[0]; d.p.conf = hd[1]; d.p.mask = hd[2]; d.p.proto = hd[3];
    d.p.P = P; d.p.C = C; d.p.hp = hp; d.p.wp = wp; d.p.top_k = top_k; d.p.max_dets = max_dets;
    d.p.conf_thresh = conf_thresh; d.p.nms_thresh = nms_thresh;
    d.p.int_mask = hd[2].kind != TQ_F32 && hd[3].kind != TQ_F32 ? 1 : 0;
    if (reuse) { if (hipMemcpy((void*)d.p.priors, priors, sizeof(float) * (size_t)P * 4, hipMemcpyHostToDevice) != hipSuccess) { det_release(d); return h->fail(YH_EHIP, "detect op upload failed"); } }
    else if (int rc = det_alloc(h, d, n, priors)) { det_release(d); return rc; }
    d.sig = sig;
    d.p.n = n;
    const hipError_t e = launch_tfl_detect(d.p, h->stream);
    if (e != hipSuccess) return h->fail(YH_EHIP, std::string("tflite detect op: ") + hipGetErrorString(e));
    TCHK(h, hipStreamSynchronize(h->stream));
    h->det_last = &d;
    h->det_last_n = n;
    return YH_OK;
}

// ---- instance frames from the setup's detections (tfl_instance.hip; DESIGN.md section 11 "TFLite instance frames") ----
// Both calls: every check, then the one run on the setup's buffers where the tail left them. per_frame: `first` and `n` count
// camera frames of two images each.
static int tfl_instance_call(yh_tfl* h, bool per_frame, int32_t first, int32_t n, int32_t width, int32_t height, const uint8_t* class_map,
                             float min_score, uint32_t* out_host) {
    if (!h) return YH_EINVAL;
    const char* what = per_frame ? "instance frames" : "instance batch";
    if (!h->det.ready) return h->fail(YH_ESTATE, std::string(what) + " before yh_tfl_detect_setup");
    if (h->det_last != &h->det)
        return h->fail(YH_ESTATE, std::string(what) + ": no detections: yh_tfl_evaluate / yh_tfl_detect has not run since the last yh_tfl_set_input or invoke");
    if (n < 1) return h->fail(YH_EINVAL, std::string(what) + (per_frame ? ": n_frames must be at least 1" : ": n_images must be at least 1"));
    const int have = per_frame ? h->det_last_n / 2 : h->det_last_n;
    if (first < 0 || first >= have || n > have - first)
        return h->fail(YH_EINVAL, std::string(what) + (per_frame ? ": frames outside the last tail's images (frame b is images 2b and 2b + 1)"
                                                                 : ": images outside the last tail's"));
    const TflDetectParams& q = h->det.p;
    if (const char* why = instance_check(width, height, class_map, q.C - 1, min_score)) return h->fail(YH_EINVAL, why);
    TCHK(h, hipSetDevice(h->dev));
    TraceRange tr(per_frame ? "yh_tfl_instance_frames" : "yh_tfl_instance_batch");
    const size_t img = (size_t)first * (per_frame ? 2 : 1), px = (size_t)q.hp * q.wp;
    const TflInstSource src = { q.masks + img * q.max_dets * px, q.dets + img * q.max_dets, q.det_count + img, q.max_dets, q.hp, q.wp, q.C - 1 };
    return tfl_instance_run(h->inst, h->stream, &h->err, src, n, per_frame, width, height, class_map, min_score, out_host, false);
}

int yh_tfl_instance_batch(yh_tfl* h, int32_t first_image, int32_t n_images, int32_t width, int32_t height, const uint8_t* class_map,
                          float min_score, uint32_t* out_host) {
    return tfl_instance_call(h, false, first_image, n_images, width, height, class_map, min_score, out_host);
}

int yh_tfl_instance_frames(yh_tfl* h, int32_t first_frame, int32_t n_frames, int32_t width, int32_t height, const uint8_t* class_map,
                           float min_score, uint32_t* out_host) {
    return tfl_instance_call(h, true, first_frame, n_frames, width, height, class_map, min_score, out_host);
}

const uint32_t* yh_tfl_instance_device_frames(const yh_tfl* h) { return h ? tfl_instance_frames(h->inst) : nullptr; }

int yh_tfl_instance_row_width(const yh_tfl* h) { return h ? h->inst.row_width : YH_EINVAL; }

int yh_tfl_instance_read(yh_tfl* h, int32_t index, int32_t* n_instances, int32_t* table, int32_t capacity) {
    if (!h || !n_instances) return YH_EINVAL;
    if (h->inst.n < 1) return h->fail(YH_ESTATE, "instance table: no instance batch yet");
    if (index < 0 || index >= h->inst.n) return h->fail(YH_EINVAL, "instance table: index outside the last batch");
    const std::vector<int32_t>& t = h->inst.tables[(size_t)index];
    *n_instances = (int32_t)(t.size() / (size_t)h->inst.row_width);
    if (!table) return YH_OK;
    if (capacity < *n_instances) return h->fail(YH_EOVERFLOW, "instance table: capacity too small");
    memcpy(table, t.data(), t.size() * sizeof(int32_t));
    return YH_OK;
}

// The per-frame kernels on caller-provided detections, no model and no setup (include/yolact_hip_debug.h): the handle gives the
// device, the stream and the error text. The mask slots past an image's count are uploaded as 0xFF - a kernel that read them would
// paint them - and the frames are painted between two guard bands of 0xFF that are read back and checked (tfl_instance_run).
int yh_tfl_op_instance_frames(yh_tfl* h, const uint8_t* masks, const int32_t* class_ids, const float* scores, const int32_t* counts,
                              int32_t n_frames, int32_t n_dets, int32_t hp, int32_t wp, int32_t width, int32_t height,
                              const uint8_t* class_map, float min_score, uint32_t* out_host) {
    if (!h || !counts || (n_dets > 0 && (!masks || !class_ids || !scores))) return YH_EINVAL;
    if (n_frames < 1 || n_frames > 64) return h->fail(YH_EINVAL, "instance frames op: n_frames outside 1 .. 64");
    if (n_dets < 0 || n_dets > kTdDetsMax) return h->fail(YH_EINVAL, "instance frames op: n_dets outside 0 .. 128");
    if (hp < 1 || hp > 4096 || wp < 1 || wp > 4096) return h->fail(YH_EINVAL, "instance frames op: hp and wp must be in 1 .. 4096");
    const int images = 2 * n_frames;
    for (int b = 0; b < images; ++b) {
        if (counts[b] < 0 || counts[b] > n_dets) return h->fail(YH_EINVAL, "instance frames op: a count outside 0 .. n_dets");
        for (int d = 0; d < counts[b]; ++d) {
            const size_t i = (size_t)b * n_dets + d;
            if (class_ids[i] < 0 || class_ids[i] >= kTflOpClasses) return h->fail(YH_EINVAL, "instance frames op: class id outside 0 .. 79");
            if (d > 0 && !(scores[i] <= scores[i - 1]))
                return h->fail(YH_EINVAL, "instance frames op: an image's scores are not non-increasing (the order the tail returns)");
        }
    }
    if (const char* why = instance_check(width, height, class_map, kTflOpClasses, min_score)) return h->fail(YH_EINVAL, why);
    TCHK(h, hipSetDevice(h->dev));
    const size_t px = (size_t)hp * wp, slots = (size_t)images * n_dets;
    std::vector<yh_detection> dets(slots + 1);
    memset(dets.data(), 0, dets.size() * sizeof(yh_detection));
    std::vector<uint8_t> ms(slots * px + 16, 0xFF);
    for (int b = 0; b < images; ++b) {
        const size_t o = (size_t)b * n_dets;
        if (counts[b] > 0) memcpy(&ms[o * px], &masks[o * px], (size_t)counts[b] * px);
        for (int d = 0; d < counts[b]; ++d) { dets[o + d].class_id = class_ids[o + d]; dets[o + d].score = scores[o + d]; }
    }
    TflInstance& st = h->inst;
    TCHK(h, hipStreamSynchronize(h->stream));   // (the buffers below may move: nothing of an earlier call is in flight)
    st.n = -1;
    if (!instance_grow_bytes(&st.op_masks, &st.op_masks_cap, ms.size()) ||
        !instance_grow_bytes(&st.op_dets, &st.op_dets_cap, dets.size() * sizeof(yh_detection)) ||
        !instance_grow_bytes(&st.op_counts, &st.op_counts_cap, (size_t)images * sizeof(int)))
        return h->fail(YH_ENOMEM, "hipMalloc instance frames op");
    TCHK(h, hipMemcpy(st.op_masks, ms.data(), ms.size(), hipMemcpyHostToDevice));
    TCHK(h, hipMemcpy(st.op_dets, dets.data(), dets.size() * sizeof(yh_detection), hipMemcpyHostToDevice));
    TCHK(h, hipMemcpy(st.op_counts, counts, (size_t)images * sizeof(int), hipMemcpyHostToDevice));
    const TflInstSource src = { (const uint8_t*)st.op_masks, (const yh_detection*)st.op_dets, (const int*)st.op_counts, n_dets, hp, wp, kTflOpClasses };
    return tfl_instance_run(st, h->stream, &h->err, src, n_frames, true, width, height, class_map, min_score, out_host, true);
}

}  // extern "C"
