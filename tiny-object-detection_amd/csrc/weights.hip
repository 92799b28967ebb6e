// weights.hip - everything that knows the YHW1 weight blob (DESIGN.md section "Weight blob"): the canonical conv table and its
// offsets, the blob check, the synthetic generator, the repack into the launched panels, yh_load_weights_*.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "engine.h"

using namespace yh;

namespace {

uint64_t splitmix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
float unit_rand(uint64_t seed, uint64_t conv, uint64_t stream, uint64_t e) {
    const uint64_t u = splitmix(splitmix(seed + conv * 1000003ull + stream) + e);
    return ((float)(uint32_t)(u >> 40) - 8388608.0f) * (1.0f / 8388608.0f);
}
uint16_t f32_to_f16_bits(float f) {  // round to nearest even, IEEE binary16
    const _Float16 h = (_Float16)f;
    uint16_t b;
    memcpy(&b, &h, 2);
    return b;
}

}  // namespace

namespace yh {

// Canonical conv table (DESIGN.md §Weight blob) — order defines the blob layout.
void build_conv_table(yh_engine* h) {
    auto add = [&](int co, int ci, int k, float g, int conf) {
        ConvDesc d; d.cout = co; d.cin = ci; d.k = k; d.gain = g; d.is_conf = conf; d.blob_w_off = d.blob_b_off = 0;
        h->convs.push_back(d);
    };
    add(64, 3, 7, 1.0f, 0);
    int inc = 64;
    for (int L = 0; L < 4; ++L) {
        const int planes = 64 << L;
        // a block's last conv: gain 0.3 in stages of up to six blocks; ResNet-101's 23-block stage scales it by sqrt(6 / blocks) so
        // that the residual stream grows over the stage as it does in ResNet-50 (the same two f32 operations as the oracle)
        const int nb_stage = blocks_of(h->cfg.backbone, L);
        const float g3 = nb_stage > 6 ? 0.3f * sqrtf(6.0f / (float)nb_stage) : 0.3f;
        for (int b = 0; b < blocks_of(h->cfg.backbone, L); ++b) {
            add(planes, inc, 1, 1.0f, 0);
            add(planes, planes, 3, 1.0f, 0);
            add(planes * 4, planes, 1, g3, 0);
            if (b == 0) add(planes * 4, inc, 1, 1.0f, 0);
            inc = planes * 4;
        }
    }
    add(256, 2048, 1, 0.2f, 0); add(256, 1024, 1, 0.2f, 0); add(256, 512, 1, 0.2f, 0);
    for (int i = 0; i < 3; ++i) add(256, 256, 3, 0.7f, 0);
    for (int i = 0; i < 2; ++i) add(256, 256, 3, 1.0f, 0);
    for (int i = 0; i < 4; ++i) add(256, 256, 3, 1.0f, 0);
    add(32, 256, 1, 1.0f, 0);
    add(256, 256, 3, 1.0f, 0);
    add(12, 256, 3, 2.0f, 0);
    add(3 * h->C, 256, 3, 0.7f, 1);
    add(96, 256, 3, 0.5f, 2);
    size_t off = 16;
    for (auto& d : h->convs) {
        off += 16;
        d.blob_w_off = off;
        off += pad16((size_t)d.cout * d.k * d.k * d.cin * 2);
        d.blob_b_off = off;
        off += pad16((size_t)d.cout * 4);
    }
    h->blob_bytes = off;
}

int alloc_panels(yh_engine* h) {
    for (Panel& p : h->panels) {
        void* q;
        int rc;
        if ((rc = dev_alloc(h, &q, (size_t)p.coutPad * p.Kpad * 2))) return rc;
        p.w = (half_t*)q;
        if ((rc = dev_alloc(h, &q, (size_t)p.coutPad * 4))) return rc;
        p.bias = (float*)q;
        if (p.fp8) {
            if ((rc = dev_alloc(h, &q, (size_t)p.coutPad * p.Kpad))) return rc;
            p.w8 = (uint8_t*)q;
            if ((rc = dev_alloc(h, &q, (size_t)p.coutPad * 4))) return rc;
            p.scale = (float*)q;
        }
        if (p.tile == TILE_64x256_SMALLC) {
            const int nt = p.Kpad / 8, cpr = (p.k + 1) / 2;  // chunks per kernel row
            std::vector<int2> t(nt);
            for (int i = 0; i < nt; ++i) t[i] = i < p.k * cpr ? make_int2(i / cpr, 2 * (i % cpr)) : make_int2(1 << 20, 0);
            if ((rc = dev_alloc(h, &q, sizeof(int2) * nt))) return rc;
            p.rs_table = (int2*)q;
            HIPCHK(h, hipMemcpy(q, t.data(), sizeof(int2) * nt, hipMemcpyHostToDevice));
        }
    }
    return YH_OK;
}

int check_blob(yh_engine* h, const uint8_t* b, size_t nbytes) {
    if (nbytes != h->blob_bytes) return h->fail(YH_EWEIGHTS, "weight blob size mismatch");
    if (memcmp(b, "YHW1", 4) != 0) return h->fail(YH_EWEIGHTS, "weight blob magic mismatch");
    uint32_t hdr[3];
    memcpy(hdr, b + 4, 12);
    if (hdr[0] != h->convs.size() || (int)hdr[1] != h->cfg.backbone || (int)hdr[2] != h->C)
        return h->fail(YH_EWEIGHTS, "weight blob header does not match the architecture");
    for (const ConvDesc& d : h->convs) {
        uint32_t rec[4];
        memcpy(rec, b + d.blob_w_off - 16, 16);
        if ((int)rec[0] != d.cout || (int)rec[1] != d.cin || (int)rec[2] != d.k || (int)rec[3] != d.k)
            return h->fail(YH_EWEIGHTS, "weight blob layer record mismatch");
    }
    return YH_OK;
}

int upload_panels(yh_engine* h, const uint8_t* blob) {
    HIPCHK(h, hipSetDevice(h->dev));
    for (Panel& p : h->panels) {
        std::vector<uint16_t> w((size_t)p.coutPad * p.Kpad, 0);
        std::vector<float> bias(p.coutPad, 0.0f);
        int row0 = 0;
        for (int s : p.src) {
            const ConvDesc& d = h->convs[s];
            const uint16_t* src = (const uint16_t*)(blob + d.blob_w_off);
            const size_t K = (size_t)d.k * d.k * d.cin;
            for (int o = 0; o < d.cout; ++o) {
                uint16_t* dst = w.data() + (size_t)(row0 + o) * p.Kpad;
                if (p.cin_store == d.cin) memcpy(dst, src + (size_t)o * K, K * 2);
                else {  // stem: chunk (r, j) holds pixels s = 2j, 2j+1 with 4 channels each; s = k and c = 3 are zero
                    const int cpr = (d.k + 1) / 2;
                    for (int r = 0; r < d.k; ++r)
                        for (int sx = 0; sx < d.k; ++sx)
                            for (int c = 0; c < d.cin; ++c)
                                dst[(size_t)(r * cpr + sx / 2) * 8 + (sx & 1) * 4 + c] = src[(size_t)o * K + ((size_t)r * d.k + sx) * d.cin + c];
                }
            }
            memcpy(bias.data() + row0, blob + d.blob_b_off, (size_t)d.cout * 4);
            row0 += d.cout;
        }
        if (p.kcat >= 0) {   // two-source form: the second conv's rows continue along K, its bias adds (one f32 addition)
            const ConvDesc& d = h->convs[p.kcat];
            const size_t K1 = (size_t)p.Kpad - d.cin;
            const uint16_t* src = (const uint16_t*)(blob + d.blob_w_off);
            const float* b2 = (const float*)(blob + d.blob_b_off);
            for (int o = 0; o < d.cout; ++o) {
                memcpy(w.data() + (size_t)o * p.Kpad + K1, src + (size_t)o * d.cin, (size_t)d.cin * 2);
                float bb; memcpy(&bb, b2 + o, 4);
                bias[o] = bias[o] + bb;
            }
        }
        HIPCHK(h, hipMemcpy(p.w, w.data(), w.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(p.bias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
        // (fp8 panels: the E4M3 codes depend on the input tensor's channel scales - refresh_fp8_scales makes them once those are known)
    }
    if (h->weights_loaded && h->cfg.precision == YH_PRECISION_FP8) {
        // a RE-load: the activation scales were calibrated for the old weights - they have to be set again (a first load
        // keeps scales that were stored with the model and set beforehand)
        for (ActAlloc& a : h->act) { a.scale_set = false; a.ch.clear(); }
        h->fp8_ready = false; h->fp8_active = false;
        drop_graphs(h);
    }
    h->weights_loaded = true;
    if (h->cfg.precision == YH_PRECISION_FP8) {
        // a handle whose plan has NO E4M3 layer (yh_config.fp8_f16_layers = 15) has no scale to wait for: it is ready as soon as its
        // weights are (nothing else would ever set fp8_ready: yh_fp8_set_layer_scale has no layer to be called with)
        if (h->fp8_ops.empty()) { h->fp8_ready = true; h->fp8_active = true; }
        const int rc = refresh_fp8_scales(h);   // (the panels whose input tensor already has its scales)
        if (rc) return rc;
    }
    return YH_OK;
}

// The handle's copy of the canonical blob in device memory (the send / receive buffer of the weight broadcast): allocated on first use.
int ensure_blob(yh_engine* h) {
    if (h->blob_dev) return YH_OK;
    void* q = nullptr;
    const int rc = dev_alloc(h, &q, h->blob_bytes);
    if (rc) return rc;
    h->blob_dev = (uint8_t*)q;
    return YH_OK;
}
static int keep_blob(yh_engine* h, const void* src, hipMemcpyKind kind) {
    const int rc = ensure_blob(h);
    if (rc) return rc;
    if (src != h->blob_dev) HIPCHK(h, hipMemcpy(h->blob_dev, src, h->blob_bytes, kind));
    return YH_OK;
}

}  // namespace yh

extern "C" {

size_t yh_weights_nbytes(const yh_engine* h) { return h ? h->blob_bytes : 0; }
const void* yh_weights_device_ptr(const yh_engine* h) { return h && h->weights_loaded ? h->blob_dev : nullptr; }

int yh_weights_generate(const yh_engine* hc, uint64_t seed, void* blob_host, size_t nbytes) {
    yh_engine* h = const_cast<yh_engine*>(hc);
    if (!h || !blob_host) return YH_EINVAL;
    if (nbytes != h->blob_bytes) return h->fail(YH_EINVAL, "blob size mismatch");
    uint8_t* b = (uint8_t*)blob_host;
    memset(b, 0, nbytes);
    memcpy(b, "YHW1", 4);
    const uint32_t hdr[3] = { (uint32_t)h->convs.size(), (uint32_t)h->cfg.backbone, (uint32_t)h->C };
    memcpy(b + 4, hdr, 12);
    for (size_t i = 0; i < h->convs.size(); ++i) {
        const ConvDesc& d = h->convs[i];
        const uint32_t rec[4] = { (uint32_t)d.cout, (uint32_t)d.cin, (uint32_t)d.k, (uint32_t)d.k };
        memcpy(b + d.blob_w_off - 16, rec, 16);
        const size_t ne = (size_t)d.cout * d.k * d.k * d.cin;
        const float fan_in = (float)(d.k * d.k * d.cin);
        const float a = d.gain * sqrtf(6.0f / fan_in);
        uint16_t* w = (uint16_t*)(b + d.blob_w_off);
        for (size_t e = 0; e < ne; ++e) w[e] = f32_to_f16_bits(unit_rand(seed, i, 0, e) * a);
        float* bias = (float*)(b + d.blob_b_off);
        for (int e = 0; e < d.cout; ++e) {
            float v = unit_rand(seed, i, 1, (uint64_t)e) * 0.1f;
            if (d.is_conf == 1 && (e % h->C) == 0) v = v + 10.0f;   // background logit: detections stay sparse
            if (d.is_conf == 2) v = v + 0.1f;                         // mask head: logits not centred on their threshold
            bias[e] = v;
        }
    }
    return YH_OK;
}

int yh_load_weights_host(yh_engine* h, const void* blob_host, size_t nbytes) {
    if (!h || !blob_host) return YH_EINVAL;
    int rc = check_blob(h, (const uint8_t*)blob_host, nbytes);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->dev));
    if ((rc = keep_blob(h, blob_host, hipMemcpyHostToDevice))) return rc;
    return upload_panels(h, (const uint8_t*)blob_host);
}

int yh_load_weights_device(yh_engine* h, const void* blob_dev, size_t nbytes) {
    if (!h || !blob_dev) return YH_EINVAL;
    if (nbytes != h->blob_bytes) return h->fail(YH_EWEIGHTS, "weight blob size mismatch");
    HIPCHK(h, hipSetDevice(h->dev));
    std::vector<uint8_t> host(nbytes);
    HIPCHK(h, hipMemcpy(host.data(), blob_dev, nbytes, hipMemcpyDeviceToHost));
    int rc = check_blob(h, host.data(), nbytes);
    if (rc) return rc;
    if ((rc = keep_blob(h, blob_dev, hipMemcpyDeviceToDevice))) return rc;
    return upload_panels(h, host.data());
}

}  // extern "C"
