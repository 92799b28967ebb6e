// fp8.hip - fp8 precision (DESIGN.md section "Precision"): which ops run E4M3, the per-channel activation scales, the weight
// requantisation they imply, the calibration, and the yh_fp8_* entry points.
#include <math.h>
#include <string.h>

#include "engine.h"

using namespace yh;

namespace yh {

// fp8 precision: which convolutions read E4M3 operands, and what each producer therefore writes.
// Rule: 3x3 convolutions with >= 256 input channels (a multiple of 128: one 128-byte LDS row is
// one K step of the block-scaled MFMA) and a multiple of 256 output channels (the fp8 kernel's tile). Everything else
// stays f16. A tensor read only by fp8 convolutions is stored only as E4M3; one with both kinds of reader (the FPN
// laterals: pred conv and bilinear upsample) is written in both forms by its producer's epilogue.
void plan_fp8(yh_engine* h) {
    struct Range { int sid; long long off, len; };
    auto range = [&](const Buf& b) { return Range{ b.sid, (long long)(b.d - h->act[b.sid].base), (long long)b.h * b.w * b.c }; };
    auto overlap = [](const Range& a, const Range& b) { return a.sid == b.sid && a.off < b.off + b.len && b.off < a.off + a.len; };
    for (size_t i = 0; i < h->ops.size(); ++i) {
        Op& o = h->ops[i];
        if (o.kind != OP_CONV) continue;
        Panel& pn = h->panels[o.panel];
        const ConvDesc& d0 = h->convs[pn.src[0]];
        // (yh_config.fp8_f16_layers: groups kept in f16 - bit 0 head trunk, 1 protonet, 2 FPN pred / down, 3 backbone)
        const int keep = h->cfg.fp8_f16_layers;
        const bool is_head = o.name.compare(0, 6, "head_t") == 0, is_proto = o.name.compare(0, 5, "proto") == 0, is_bb = o.name[0] == 'l';
        const bool is_fpn = o.name[0] == 'p' && !is_proto;
        if (((keep & 1) && is_head) || ((keep & 2) && is_proto) || ((keep & 4) && is_fpn) || ((keep & 8) && is_bb)) continue;
        if (pn.k == 3 && d0.cin % 128 == 0 && d0.cin >= 256 && pn.cout % 256 == 0 && pn.coutPad % 256 == 0 && o.in.q) {
            o.fp8 = true; pn.fp8 = true; pn.in_sid = o.in.sid;
            h->fp8_ops.push_back((int)i);
        }
    }
    for (size_t i = 0; i < h->ops.size(); ++i) {
        Op& o = h->ops[i];
        if (o.kind == OP_PRE) continue;
        const Range w = range(o.out);
        bool need_q = false, need_f16 = h->cfg.debug_tensors != 0;
        for (size_t j = i + 1; j < h->ops.size(); ++j) {
            const Op& c = h->ops[j];
            if (c.kind == OP_PRE) continue;
            if (overlap(w, range(c.in))) { if (c.fp8) need_q = true; else need_f16 = true; }
            if (c.has_res && c.kind == OP_CONV && overlap(w, range(c.res))) need_f16 = true;
            if (c.dual && overlap(w, range(c.in2))) need_f16 = true;
        }
        if (overlap(w, range(h->heads)) || overlap(w, range(h->proto))) need_f16 = true;   // engine outputs, read by the tail
        if (!need_q && !need_f16) need_f16 = true;
        o.write_q = need_q; o.write_f16 = need_f16;
    }
    // accounting (profile / roofline): E4M3 operands are one byte
    for (Op& o : h->ops) {
        if (o.kind != OP_CONV && o.kind != OP_BILINEAR) continue;
        const double out_b = (o.write_f16 ? 2.0 : 0.0) + (o.write_q ? 1.0 : 0.0);
        if (o.kind == OP_BILINEAR) { o.bytes_per_img = 2.0 * o.in.c * (double)o.in.h * o.in.w + out_b * o.in.c * (double)o.out.h * o.out.w; continue; }
        const Panel& pn = h->panels[o.panel];
        const ConvDesc& d0 = h->convs[pn.src[0]];
        if (o.dual) continue;   // (f16 on both sides: the figures set at construction stand)
        const double K = (double)pn.k * pn.k * d0.cin, in_elems = o.nlev ? (double)h->cells * d0.cin : (double)o.in.h * o.in.w * d0.cin;
        o.bytes_per_img = (o.fp8 ? 1.0 : 2.0) * in_elems + (double)o.P * o.Q * pn.cout * (out_b + (o.has_res ? 2.0 : 0.0));
        o.bytes_fixed = (o.fp8 ? 1.0 : 2.0) * pn.cout * K;
        if (o.fp8) o.label = std::string(conv_tile_symbol(TILE_256x256_FP8)) + ":" + o.name;
    }
    for (const auto& kv : h->named) {
        const Range r = range(kv.second);
        for (const Op& o : h->ops)
            if (o.kind != OP_PRE && overlap(r, range(o.out)) && !o.write_f16) h->q_only.insert(kv.first);
    }
}

// Does the plan write the E4M3 form of every element of tensor `b` (a named tensor or a slice of one)? True when at least one op
// writes into its range and every op that does has write_q (yh_debug_read_tensor_e4m3: codes nobody wrote are not a result).
bool fp8_writes_codes(const yh_engine* h, const Buf& b) {
    if (!b.q || b.sid < 0) return false;
    const long long off = b.d - h->act[b.sid].base, len = (long long)b.h * b.w * b.c;
    int writers = 0;
    for (const Op& o : h->ops) {
        if (o.kind == OP_PRE || o.out.sid != b.sid) continue;
        const long long ooff = o.out.d - h->act[b.sid].base, olen = (long long)o.out.h * o.out.w * o.out.c;
        if (!(off < ooff + olen && ooff < off + len)) continue;
        if (!o.write_q) return false;
        ++writers;
    }
    return writers > 0;
}

// fp8 precision: the E4M3 layers whose input tensor has no scale yet (comma-separated; empty = every tensor is set)
std::string fp8_missing(const yh_engine* h) {
    std::string out;
    for (int oi : h->fp8_ops)
        if (!h->act[h->ops[oi].in.sid].scale_set) out += (out.empty() ? "" : ", ") + h->ops[oi].name;
    return out;
}

}  // namespace yh

namespace {

// One activation scale per channel of allocation `sid` (host copy, device tables of the scale and of its reciprocal).
int set_sid_scales(yh_engine* h, int sid, const std::vector<float>& v) {
    if ((int)v.size() != h->act[sid].c || !h->act[sid].inv_dev) return h->fail(YH_EINVAL, "fp8: channel scale count does not match the tensor");
    std::vector<float> inv(v.size());
    float mx = 0.0f;
    for (size_t c = 0; c < v.size(); ++c) {
        if (!(v[c] > 0.0f) || !(v[c] < 3.0e38f)) return h->fail(YH_EINVAL, "activation scale must be a positive finite number");
        inv[c] = 1.0f / v[c];
        mx = v[c] > mx ? v[c] : mx;
    }
    HIPCHK(h, hipMemcpy(h->act[sid].inv_dev, inv.data(), inv.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->act[sid].sc_dev, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    h->act[sid].ch = v;
    h->act[sid].scale = mx;      // (what yh_fp8_layer_info reports: the largest channel scale)
    h->act[sid].scale_set = true;
    return YH_OK;
}

}  // namespace

namespace yh {

// The E4M3 weights of the fp8 convolutions that read allocation `sid` (-1: all of them): the input tensor's channel scales s[c]
// are folded into the K axis, then one scale per output channel - t = w * s[c], s_w = max_k |t| / 448 (1 for an all-zero row),
// codes = e4m3(t * (1 / s_w)) by the device's own conversion - and the epilogue's multiplier is s_w alone
// (y = fma(acc, s_w[ch], bias)). The same operations in the same order as oracle/orc_net.c's fp8 forward mode.
int refresh_fp8_scales(yh_engine* h, int sid) {
    if (!h->weights_loaded) return YH_OK;
    for (Panel& p : h->panels) {
        if (!p.fp8 || (sid >= 0 && p.in_sid != sid) || h->act[p.in_sid].ch.empty()) continue;
        if (p.coutPad > 1024 || h->act[p.in_sid].c != p.cin_store) return h->fail(YH_EINVAL, "fp8: weight panel geometry");
        const float* col = h->act[p.in_sid].sc_dev;
        if (launch_rowmax_scaled_f16(p.w, p.coutPad, p.Kpad, p.cin_store, col, h->rowmax_dev, h->stream) != hipSuccess) return h->fail(YH_EHIP, "weight row maxima launch failed");
        std::vector<unsigned> bits(p.coutPad);
        HIPCHK(h, hipMemcpyAsync(bits.data(), h->rowmax_dev, bits.size() * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        p.sw.assign(p.coutPad, 1.0f);
        std::vector<float> inv(p.coutPad, 1.0f);
        for (int r = 0; r < p.coutPad; ++r) {
            float a; memcpy(&a, &bits[r], 4);
            p.sw[r] = a > 0.0f ? a / 448.0f : 1.0f;
            inv[r] = 1.0f / p.sw[r];
        }
        HIPCHK(h, hipMemcpy(p.scale, inv.data(), inv.size() * 4, hipMemcpyHostToDevice));   // (borrowed as the 1 / s_w table for this one launch)
        if (launch_quantize_rows_e4m3(p.w, p.w8, p.coutPad, p.Kpad, p.cin_store, col, p.scale, h->stream) != hipSuccess) return h->fail(YH_EHIP, "weight quantisation launch failed");
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(p.scale, p.sw.data(), p.sw.size() * 4, hipMemcpyHostToDevice));
    }
    return YH_OK;
}

}  // namespace yh

extern "C" {

// ---- fp8 precision (configs[4]) ----------------------------------------------------------------------------
int yh_fp8_layer_count(const yh_engine* h) { return h ? (int)h->fp8_ops.size() : YH_EINVAL; }

int yh_fp8_layer_info(const yh_engine* h, int32_t i, const char** conv_name, float* act_scale) {
    if (!h || i < 0 || i >= (int)h->fp8_ops.size()) return YH_EINVAL;
    const Op& o = h->ops[h->fp8_ops[i]];
    if (conv_name) *conv_name = o.name.c_str();
    if (act_scale) *act_scale = h->act[o.in.sid].scale;
    return YH_OK;
}

static int fp8_set_scales_impl(yh_engine* h, int32_t i, const std::vector<float>& v) {
    HIPCHK(h, hipSetDevice(h->dev));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    drop_graphs(h);   // the scales are baked into the captured launches
    const int sid = h->ops[h->fp8_ops[i]].in.sid;
    const int rc = set_sid_scales(h, sid, v);
    if (rc) return rc;
    // the handle counts as calibrated once EVERY E4M3 input tensor has its scales (they belong to the tensor: layers that read
    // one allocation - P3..P7 of the pyramid: p6, p7, head_t, proto0 - share them, include/yolact_hip.h)
    h->fp8_ready = fp8_missing(h).empty(); h->fp8_active = h->fp8_ready;
    return refresh_fp8_scales(h, sid);
}

int yh_fp8_set_layer_scale(yh_engine* h, int32_t i, float act_scale) {
    if (!h || i < 0 || i >= (int)h->fp8_ops.size()) return YH_EINVAL;
    if (!(act_scale > 0.0f) || !(act_scale < 3.0e38f)) return h->fail(YH_EINVAL, "activation scale must be a positive finite number");
    return fp8_set_scales_impl(h, i, std::vector<float>((size_t)h->act[h->ops[h->fp8_ops[i]].in.sid].c, act_scale));
}

int yh_fp8_layer_channels(const yh_engine* h, int32_t i) {
    if (!h || i < 0 || i >= (int)h->fp8_ops.size()) return YH_EINVAL;
    return h->act[h->ops[h->fp8_ops[i]].in.sid].c;
}

int yh_fp8_layer_channel_scales(const yh_engine* h, int32_t i, float* scales, int32_t n) {
    if (!h || !scales || i < 0 || i >= (int)h->fp8_ops.size()) return YH_EINVAL;
    const int sid = h->ops[h->fp8_ops[i]].in.sid;
    if (n != h->act[sid].c) return YH_EINVAL;
    for (int c = 0; c < n; ++c) scales[c] = h->act[sid].ch.empty() ? 1.0f : h->act[sid].ch[c];
    return YH_OK;
}

int yh_fp8_set_layer_channel_scales(yh_engine* h, int32_t i, const float* scales, int32_t n) {
    if (!h || !scales || i < 0 || i >= (int)h->fp8_ops.size()) return YH_EINVAL;
    if (n != h->act[h->ops[h->fp8_ops[i]].in.sid].c) return h->fail(YH_EINVAL, "fp8: channel scale count does not match the layer's input tensor");
    return fp8_set_scales_impl(h, i, std::vector<float>(scales, scales + n));
}

// Test hook: E4M3 layer i's weight codes as the kernel reads them, [cout][k * k * cin], and the per-output-channel scales of its
// epilogue, both read back from the device.
int yh_debug_fp8_weights(yh_engine* h, int32_t i, uint8_t* codes, float* s_w, int32_t dims[2]) {
    if (!h || !dims || i < 0 || i >= (int)h->fp8_ops.size()) return YH_EINVAL;
    const Op& o = h->ops[h->fp8_ops[i]];
    const Panel& p = h->panels[o.panel];
    if (!h->weights_loaded) return h->fail(YH_ESTATE, "fp8 weights of " + o.name + ": no weights are loaded");
    if (!h->act[p.in_sid].scale_set || h->act[p.in_sid].ch.empty()) return h->fail(YH_ESTATE, "fp8 weights of " + o.name + ": its input tensor has no scales yet");
    const int K = p.k * p.k * p.cin_store;
    dims[0] = p.cout; dims[1] = K;
    HIPCHK(h, hipSetDevice(h->dev));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (codes) HIPCHK(h, hipMemcpy2D(codes, (size_t)K, p.w8, (size_t)p.Kpad, (size_t)K, (size_t)p.cout, hipMemcpyDeviceToHost));
    if (s_w) HIPCHK(h, hipMemcpy(s_w, p.scale, (size_t)p.cout * 4, hipMemcpyDeviceToHost));
    return YH_OK;
}

int yh_fp8_calibrate(yh_engine* h) {
    if (!h) return YH_EINVAL;
    if (h->cfg.precision != YH_PRECISION_FP8) return h->fail(YH_ESTATE, "the handle was not created with YH_PRECISION_FP8");
    if (!h->weights_loaded) return h->fail(YH_ESTATE, "weights not loaded");
    if (h->cur_n < 1) return h->fail(YH_ESTATE, "no input set: calibration runs on the frames last set");
    HIPCHK(h, hipSetDevice(h->dev));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    drop_graphs(h);
    // 1. the f16 forward of these frames (every tensor in f16, bit for bit what a YH_PRECISION_F16 handle with the same tuning and
    // debug_tensors computes: tests/test_gpu_fp8_exact.py); a NaN or an Inf in a tensor an E4M3 layer reads refuses the call; 2. one scale per
    // CHANNEL of every tensor that an fp8 convolution reads: max(2 max |x[.., c]|, max |x| / 16) / 448 (448: E4M3's largest finite
    // value; the factor and the floor: headroom for frames the calibration has not seen, below; yh_config.fp8_per_tensor = 1:
    // the tensor's maximum in every channel, no headroom - round 3's scheme). On any failure the handle keeps the scales
    // (and the form of the forward) it had.
    std::set<int> sids;
    for (int oi : h->fp8_ops) sids.insert(h->ops[oi].in.sid);
    constexpr int MT = yh_engine::kMaxFp8Tensors, MC = yh_engine::kMaxFp8Channels;
    if ((int)sids.size() > MT) return h->fail(YH_EINVAL, "too many fp8 input tensors");
    for (int sid : sids) if (h->act[sid].c > MC) return h->fail(YH_EINVAL, "fp8 input tensor with more than 512 channels");
    std::vector<unsigned> bits((size_t)MT * MC);
    h->fp8_active = false;
    h->dets_valid = false;
    const int rc = [&]() -> int {
        int r = wait_input(h);
        if (r) return r;
        r = enqueue_all(h, h->cur_n, 0);
        if (r) return r;
        HIPCHK(h, hipMemsetAsync(h->absmax_dev, 0, bits.size() * 4, h->stream));
        int k = 0;
        for (int sid : sids)
            if (launch_absmax_channels_f16(h->act[sid].base, (long long)h->cur_n * h->act[sid].img / h->act[sid].c, h->act[sid].c, h->absmax_dev + (size_t)(k++) * MC, h->stream) != hipSuccess)
                return h->fail(YH_EHIP, "absmax launch failed");
        HIPCHK(h, hipMemcpyAsync(bits.data(), h->absmax_dev, bits.size() * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        k = 0;
        for (int sid : sids) {   // (absmax_channels_f16 takes the maxima on bit patterns: Inf and every NaN lie above all finite values and win)
            for (int c = 0; c < h->act[sid].c; ++c) {
                float a; memcpy(&a, &bits[(size_t)k * MC + c], 4);
                if (!(a < 3.0e38f)) {
                    std::string who;
                    for (int oi : h->fp8_ops) if (h->ops[oi].in.sid == sid) who += (who.empty() ? "" : ", ") + h->ops[oi].name;
                    return h->fail(YH_ESTATE, "fp8 calibration: the f16 forward of these frames overflowed (Inf / NaN) in the input tensor of " + who + "; no scale was changed");
                }
            }
            ++k;
        }
        return YH_OK;
    }();
    if (rc) { h->fp8_active = h->fp8_ready; return rc; }
    int k = 0;
    for (int sid : sids) {
        const int C = h->act[sid].c;
        std::vector<float> v((size_t)C);
        float amax = 0.0f;
        for (int c = 0; c < C; ++c) { float a; memcpy(&a, &bits[(size_t)k * MC + c], 4); v[c] = a; amax = a > amax ? a : amax; }
        // Per channel (round 5): twice the channel's own maximum, and never less than a sixteenth of the tensor's. The maxima
        // are those of the CALIBRATION frames; a channel that is quiet there and active later saturated at 448 s[c] - calibrated on the
        // reference's test image and evaluated on a noise frame the scheme matched 21 of the f16 oracle's 31 detections where one scale
        // per tensor matched 25 (tests/test_gpu_fp8_sweep.py, held-out test). Headroom is free in a floating-point code: E4M3 keeps its
        // 3-bit mantissa over 2^15 of range, the values after a ReLU span a few octaves, so a scale 2 ... 16 x larger loses no bit.
        for (int c = 0; c < C; ++c) {
            const float a = h->cfg.fp8_per_tensor ? amax : fmaxf(2.0f * v[c], amax * (1.0f / 16.0f));
            v[c] = a > 0.0f ? a / 448.0f : 1.0f;
        }
        const int r2 = set_sid_scales(h, sid, v);
        if (r2) return r2;
        ++k;
    }
    h->fp8_ready = true; h->fp8_active = true;
    return refresh_fp8_scales(h);
}

}  // extern "C"
