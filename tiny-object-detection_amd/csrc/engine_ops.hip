// engine_ops.hip - the single-op entry points (yh_op_*): one kernel on caller-supplied tensors. Only tests call them.
#include <stdio.h>
#include <string.h>

#include "engine.h"

using namespace yh;

namespace {

// The NaN an element outside an uploaded input reads as: 0x7E00 per f16, 0x7FC00000 per f32, 0x7F per E4M3 code or raw byte.
enum NanBand { NAN_F16, NAN_F32, NAN_BYTE };

// The device buffers of one single-op call, allocated and uploaded in the order the call asks for them, freed when the call returns.
// Every one is guarded (Bounds):
//   an input  (upload, upload_padded)  kBand bytes of NaN | the data (| zeros up to `cap`) | kBand bytes of NaN - a plain load
//             outside the data poisons a stored value, and the value comparison every test makes fails;
//   an output (alloc_out, check_out)   kBand bytes | the payload | kGuardRows rows (no row stride: kBand bytes), all 0xFF before the
//             launch - the NaN pattern an unwritten element shows - and both guards read back behind it: a changed byte is
//             YH_EOVERFLOW (overflow_text);
//   the split-K workspace (paint_ws, check_ws)  the bytes behind the last slice's slab.
// kGuardRows is the largest row count of a tile in kConvTiles: a tile-granular overrun falls inside the back guard.
// The first HIP error is kept and every step after it is skipped.
struct OpStaging {
    static constexpr size_t kBand = 4096, kGuardRows = 256;
    struct Out { const char* name; uint8_t* base; size_t bytes, row_bytes, back; };   // base: the allocation's; payload at base + kBand
    struct Hit { const char* name = nullptr; bool front = false; size_t off = 0, row_bytes = 0; unsigned value = 0; };
    hipError_t e = hipSuccess;
    std::vector<void*> bufs;
    std::vector<Out> outs;
    Hit hit;                      // the first changed guard byte check_out met (name == nullptr: none)
    float* ws = nullptr;          // painted part of the split-K workspace: [ws_from, ws_to) bytes
    size_t ws_from = 0, ws_to = 0;
    bool ws_hit = false;
    OpStaging() = default;
    OpStaging(const OpStaging&) = delete;
    ~OpStaging() { for (void* d : bufs) hipFree(d); }
    bool ok() const { return e == hipSuccess; }
    // (unguarded: the instance ops' buffers, which belong to a later pull request's bounds work)
    template <class T> T* alloc(size_t bytes, int fill = -1) {
        void* d = nullptr;
        if (ok() && (e = hipMalloc(&d, bytes)) == hipSuccess) bufs.push_back(d);
        if (ok() && fill >= 0) e = hipMemset(d, fill, bytes);
        // (a device memset may return before it ran, and the handle's streams do not wait for the null stream: a launch right
        // behind it could have its stores painted over)
        if (ok() && fill >= 0) e = hipStreamSynchronize(nullptr);
        return ok() ? (T*)d : nullptr;
    }
    void put(const void* d, const void* src, size_t bytes) { if (ok()) e = hipMemcpy((void*)d, src, bytes, hipMemcpyHostToDevice); }
    template <class T> T* upload_raw(const void* src, size_t bytes) { T* d = alloc<T>(bytes); put(d, src, bytes); return d; }
    // an input between its NaN bands; cap > bytes: zeros from the data's end up to cap (upload_padded)
    template <class T> T* upload(const void* src, size_t bytes, NanBand nan, size_t cap = 0) {
        if (cap < bytes) cap = bytes;
        std::vector<uint8_t> img(kBand + cap + kBand, 0);
        for (uint8_t* band : { img.data(), img.data() + kBand + cap })
            for (size_t i = 0; i < kBand; ++i)
                band[i] = nan == NAN_BYTE ? 0x7F : nan == NAN_F16 ? ((i & 1) ? 0x7E : 0x00) : ((i & 3) == 3 ? 0x7F : (i & 3) == 2 ? 0xC0 : 0x00);
        memcpy(img.data() + kBand, src, bytes);
        uint8_t* d = alloc<uint8_t>(img.size());
        put(d, img.data(), img.size());
        return ok() ? (T*)(d + kBand) : nullptr;
    }
    // a conv input with its zero pixel behind the data: `cap` bytes, the data first, zeros behind; *zero_off = where the zeros start
    template <class T> T* upload_padded(const void* src, size_t bytes, size_t cap, unsigned* zero_off, NanBand nan = NAN_F16) {
        *zero_off = (unsigned)pad16(bytes);
        return upload<T>(src, bytes, nan, cap);
    }
    template <class T> T* alloc_out(const char* name, size_t bytes, size_t row_bytes) {
        const size_t back = row_bytes ? kGuardRows * row_bytes : kBand;
        uint8_t* d = alloc<uint8_t>(kBand + bytes + back, 0xFF);
        if (!d) return nullptr;
        outs.push_back(Out{ name, d, bytes, row_bytes, back });
        return (T*)(d + kBand);
    }
    void sync(hipStream_t s) { if (ok()) e = hipStreamSynchronize(s); }
    void get(void* dst, const void* d, size_t bytes) { if (ok()) e = hipMemcpy(dst, d, bytes, hipMemcpyDeviceToHost); }
    // reads an output of alloc_out back - guards and payload in one copy: the payload to dst (nullptr: not wanted), the first
    // changed guard byte, front guard first, to `hit`
    void check_out(const void* payload, void* dst) {
        const Out* o = nullptr;
        for (const Out& c : outs) if (c.base + kBand == (const uint8_t*)payload) o = &c;
        if (!ok() || !o) return;
        std::vector<uint8_t> all(kBand + o->bytes + o->back);
        get(all.data(), o->base, all.size());
        if (!ok()) return;
        if (dst) memcpy(dst, all.data() + kBand, o->bytes);
        for (size_t i = 0; i < all.size() && !hit.name; i = i + 1 == kBand ? kBand + o->bytes : i + 1)
            if (all[i] != 0xFF) hit = Hit{ o->name, i < kBand, i < kBand ? i : i - kBand - o->bytes, o->row_bytes, all[i] };
    }
    void paint_ws(float* w, size_t from, size_t to) {
        if (!ok() || from >= to) return;
        ws = w; ws_from = from; ws_to = to;
        e = hipMemset((char*)w + from, 0xFF, to - from);
        if (ok()) e = hipStreamSynchronize(nullptr);
    }
    void check_ws() {
        if (!ok() || !ws) return;
        std::vector<uint8_t> v(ws_to - ws_from);
        get(v.data(), (const char*)ws + ws_from, v.size());
        for (size_t i = 0; ok() && i < v.size() && !ws_hit; ++i) ws_hit = v[i] != 0xFF;
    }
    bool overflowed() const { return hit.name || ws_hit; }
    // who = the op's prefix and, where the entry knows it, the kernel's symbol: "bneck op: bneck_chain_f16<..>"
    std::string overflow_text(std::string who) const {
        while (!who.empty() && who.back() == ' ') who.pop_back();   // (no symbol: "bilinear op: stored ..")
        if (!hit.name) return who + " stored split-K partials past slice k_slices - 1";
        const std::string n = hit.name;
        char at[160];
        if (hit.front)
            snprintf(at, sizeof at, ": %s front guard, byte %zu (%zu in front of the payload) is 0x%02X", hit.name, hit.off, kBand - hit.off, hit.value);
        else if (hit.row_bytes)
            snprintf(at, sizeof at, ": %s back guard, byte %zu (row M + %zu) is 0x%02X", hit.name, hit.off, hit.off / hit.row_bytes, hit.value);
        else
            snprintf(at, sizeof at, ": %s back guard, byte %zu is 0x%02X", hit.name, hit.off, hit.value);
        return who + (hit.front ? " stored in front of " + n : hit.row_bytes ? " stored " + n + " rows past M" : " stored past the end of " + n) + at;
    }
    int status(yh_engine* h, const char* what) const { return ok() ? YH_OK : h->fail(YH_EHIP, std::string(what) + hipGetErrorString(e)); }
    // ... and YH_EOVERFLOW when a guard changed
    int status(yh_engine* h, const char* what, const std::string& symbol) const {
        if (!ok()) return status(h, what);
        return overflowed() ? h->fail(YH_EOVERFLOW, overflow_text(what + symbol)) : YH_OK;
    }
};

// rows of c values, zero-padded to rows of ld (input channels to the stored count, output channels to cout8) - and back
template <class T> std::vector<T> pad_rows(const T* src, size_t rows, size_t c, size_t ld) {
    std::vector<T> v(rows * ld, T(0));
    for (size_t m = 0; m < rows; ++m) memcpy(&v[m * ld], &src[m * c], c * sizeof(T));
    return v;
}
void unpad_rows(uint16_t* dst, const std::vector<uint16_t>& src, size_t rows, size_t c, size_t ld) {
    for (size_t m = 0; m < rows; ++m) memcpy(&dst[m * c], &src[m * ld], c * 2);
}

// test hook (tune.op_kslices): a forced split-K of a single-op launch (the engine decides it in fill_conv_params)
// Where it takes effect, up to kGuardRows rows of the workspace behind the last slice's slab are painted 0xFF (OpStaging::check_ws).
void force_split_k(yh_engine* h, OpStaging& st, ConvParams& p, size_t M, int coutPad) {
    const int ksl = h->tune.op_kslices;
    if (ksl < 2 || ksl > p.ksteps || (size_t)ksl * M * coutPad * 4 > yh_engine::kSplitKBytes) return;
    p.ksteps_per_slice = (p.ksteps + ksl - 1) / ksl;
    p.k_slices = (p.ksteps + p.ksteps_per_slice - 1) / p.ksteps_per_slice;
    p.partial_ld = coutPad;
    p.partial = h->splitk_ws;
    const size_t used = (size_t)p.k_slices * M * coutPad * 4, end = used + OpStaging::kGuardRows * (size_t)coutPad * 4, cap = yh_engine::kSplitKBytes;
    st.paint_ws(h->splitk_ws, used, end < cap ? end : cap);
}

// launch_conv_planned for a single-op call: counts and names the launches on the handle; false = no launch of the plan was made,
// because launch_conv has no kernel for one of them (the caller answers YH_EINVAL)
bool launch_op_conv(yh_engine* h, OpStaging& st, const ConvParams& p, ConvTile tile, int coutPad) {
    st.e = launch_conv_planned(h->tune, p, tile, coutPad, h->stream, &h->last_conv_launches, &h->last_conv_forms);
    if (st.e != hipErrorInvalidValue) return true;
    st.e = hipSuccess;
    return false;
}

}  // namespace

extern "C" {

// ---- single-op entry points (tests) ------------------------------------------------------------
// Each one reads: validate, stage (host-side repacking, then the device buffers), fill the kernel's parameters, launch, read back.
static int op_conv2d_impl(yh_engine* h, const uint16_t* x, int32_t n, int32_t hh, int32_t ww, int32_t cin, const uint16_t* w,
                          const float* bias, int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                          const uint16_t* residual, int32_t act, uint16_t* y, const int32_t* level_sizes, int32_t nlev) {
    if (!h || !x || !w || !bias || !y) return YH_EINVAL;
    if (kh != kw || kh < 1 || stride < 1 || n < 1 || (cin != 3 && cin % 64 != 0) || (act < 0 || act > 2))
        return h->fail(YH_EINVAL, "conv op: need square kernel and cin == 3 or cin % 64 == 0");
    HIPCHK(h, hipSetDevice(h->dev));
    const int cs = cin == 3 ? 8 : cin, k = kh;
    // multi-level form: x is [n][cells][cin], cells = the levels' squares laid end to end (hh = cells, ww = 1)
    const int P = nlev > 0 ? hh : out_dim(hh, k, stride, pad), Q = nlev > 0 ? 1 : out_dim(ww, k, stride, pad);
    if (P < 1 || Q < 1) return h->fail(YH_EINVAL, "conv op: empty output");
    ConvTile tile = cin == 3 ? TILE_64x256_SMALLC : (cout <= 32 ? TILE_32x256 : (cout <= 64 ? TILE_64x256 : TILE_128x128));
    const int Kpad = cin == 3 ? round_up(k * k, 8) * 8 : k * k * cin;
    if (tile == TILE_128x128 && Kpad >= 512) tile = (cout % 256 == 0) ? TILE_256x256_M16 : TILE_128x256;
    if (tile == TILE_128x256 && stride == 1) tile = TILE_128x256_M16;
    if (h->tune.op_tile >= 0 && cin != 3) tile = (ConvTile)h->tune.op_tile;   // test hook: force a tile variant
    if (conv_tile_ch(tile) == 0) return h->fail(YH_EINVAL, "conv op: tune.op_tile is not a tile id");
    const int coutPad = round_up(cout, conv_tile_ch(tile)), cout8 = round_up(cout, 8);
    const size_t M = (size_t)n * P * Q;
    // host-side staging: pad input channels, repack weights, pad output rows to cout8
    // (test hook, tune.op_xgap: every image is followed by `gap` elements of NaN (0x7E00), so the image stride is not the dense
    // H * W * C and a gap element that contributed to any sum, even times a zero weight, would show in the output)
    const int gap = h->tune.op_xgap;
    if (gap % 8 != 0) return h->fail(YH_EINVAL, "conv op: tune.op_xgap must be a multiple of 8");
    const size_t img = (size_t)hh * ww * cs;
    std::vector<uint16_t> xs = pad_rows(x, (size_t)n * hh * ww, cin, cs);
    if (gap > 0) {
        std::vector<uint16_t> g((img + gap) * n, 0x7E00);
        for (int b = 0; b < n; ++b) memcpy(&g[b * (img + gap)], &xs[b * img], img * 2);
        xs.swap(g);
    }
    std::vector<uint16_t> wp((size_t)coutPad * Kpad, 0), rs, ys(M * cout8);
    for (int o = 0; o < cout; ++o)
        for (int t = 0; t < k * k; ++t) memcpy(&wp[(size_t)o * Kpad + (size_t)t * cs], &w[((size_t)o * k * k + t) * cin], (size_t)cin * 2);
    // (+ 32: the 96-channel tile's epilogue has 16 lanes of 8 channels per row - 12 in use - and every lane reads its bias, so the
    // last channel tile reads up to channel coutPad + 31; the engine's bias arrays are padded to 384 behind that tile's base of 256)
    const std::vector<float> bp = pad_rows(bias, 1, cout, coutPad + 32);
    if (residual) rs = pad_rows(residual, M, cout, cout8);
    std::vector<int2> tab;
    if (cin == 3) { tab.resize(Kpad / 8); for (int i = 0; i < Kpad / 8; ++i) tab[i] = i < k * k ? make_int2(i / k, i % k) : make_int2(1 << 20, 0); }
    OpStaging st;
    unsigned zo = 0;
    const half_t* dx = st.upload_padded<half_t>(xs.data(), xs.size() * 2, xs.size() * 2 + 64, &zo);
    const half_t* dw = st.upload<half_t>(wp.data(), wp.size() * 2, NAN_F16);
    const float* db = st.upload<float>(bp.data(), bp.size() * 4, NAN_F32);
    half_t* dy = st.alloc_out<half_t>("y", ys.size() * 2, (size_t)cout8 * 2);
    const half_t* dr = residual ? st.upload<half_t>(rs.data(), rs.size() * 2, NAN_F16) : nullptr;
    const int2* dt = cin == 3 ? st.upload<int2>(tab.data(), tab.size() * sizeof(int2), NAN_BYTE) : nullptr;
    if (st.ok()) {
        ConvParams p;
        memset(&p, 0, sizeof p);
        p.x = dx; p.w = dw; p.bias = db; p.res = dr; p.y = dy; p.rs_table = dt;
        p.x_img_stride = (long long)(img + gap); p.y_img_stride = (long long)P * Q * cout8; p.res_img_stride = p.y_img_stride;
        p.x_zero_off = zo; p.x_bytes = zo + 16u;
        p.w_bytes = (unsigned)(wp.size() * 2);
        p.N = n; p.H = hh; p.W = ww; p.C = cs; p.P = P; p.Q = Q; p.R = k; p.S = k; p.stride = stride; p.pad = pad;
        p.M = (int)M; p.cout8 = cout8; p.ldw = Kpad; p.ksteps = Kpad / 64; p.ldy = cout8; p.ldres = cout8; p.y_dense = 1;
        p.act = act == 1 ? 1 : 0; p.tanh_from = act == 2 ? h->tune.op_tanh_from : INT_MAX; p.n_ch_tiles = coutPad / conv_tile_ch(tile);
        if (nlev > 0) {
            p.nlev = nlev;
            for (int l = 0, s = 0; l < nlev; ++l) { p.lev_start[l] = s; p.lev_h[l] = p.lev_w[l] = level_sizes[l]; s += level_sizes[l] * level_sizes[l]; }
        }
        force_split_k(h, st, p, M, coutPad);
        if (!launch_op_conv(h, st, p, tile, coutPad)) return h->fail(YH_EINVAL, "conv op: no conv kernel for these parameters on this tile (tune.op_tile, tune.op_kslices)");
    }
    st.sync(h->stream);
    st.check_out(dy, ys.data());
    st.check_ws();
    if (const int rc = st.status(h, "conv op: ", conv_tile_symbol(tile))) return rc;
    unpad_rows(y, ys, M, cout, cout8);
    return YH_OK;
}

int yh_op_conv2d_f16(yh_engine* h, const uint16_t* x, int32_t n, int32_t hh, int32_t ww, int32_t cin, const uint16_t* w,
                     const float* bias, int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad,
                     const uint16_t* residual, int32_t act, uint16_t* y) {
    return op_conv2d_impl(h, x, n, hh, ww, cin, w, bias, cout, kh, kw, stride, pad, residual, act, y, nullptr, 0);
}

int yh_op_conv2d_dual_f16(yh_engine* h, const uint16_t* x1, int32_t n, int32_t ho, int32_t wo, int32_t c1,
                          const uint16_t* x2, int32_t h2, int32_t w2, int32_t c2, int32_t stride2,
                          const uint16_t* w, const float* bias, int32_t cout, int32_t act, uint16_t* y) {
    if (!h || !x1 || !x2 || !w || !bias || !y) return YH_EINVAL;
    if (n < 1 || ho < 1 || wo < 1 || c1 < 64 || c1 % 64 != 0 || c2 < 64 || c2 % 64 != 0 || stride2 < 1 || cout < 1 || cout % 8 != 0 || act < 0 || act > 1 ||
        (ho - 1) * stride2 >= h2 || (wo - 1) * stride2 >= w2)
        return h->fail(YH_EINVAL, "dual conv op: need c1, c2 % 64 == 0, cout % 8 == 0 and x2 covering the strided output grid");
    HIPCHK(h, hipSetDevice(h->dev));
    ConvTile tile = TILE_128x128;
    if (h->tune.op_tile >= 0) tile = (ConvTile)h->tune.op_tile;
    if (!conv_tile_has(tile, FORM_DUAL)) return h->fail(YH_EINVAL, "dual conv op: tune.op_tile is not a tile of the two-source form");
    const int K = c1 + c2, coutPad = round_up(cout, conv_tile_ch(tile));
    const size_t M = (size_t)n * ho * wo, n1 = M * c1, n2 = (size_t)n * h2 * w2 * c2;
    const std::vector<uint16_t> wp = pad_rows(w, 1, (size_t)cout * K, (size_t)coutPad * K);
    const std::vector<float> bp = pad_rows(bias, 1, cout, coutPad);
    OpStaging st;
    unsigned z1 = 0, z2 = 0;
    const half_t* d1 = st.upload_padded<half_t>(x1, n1 * 2, n1 * 2 + 64, &z1);
    const half_t* d2 = st.upload_padded<half_t>(x2, n2 * 2, n2 * 2 + 64, &z2);
    const half_t* dw = st.upload<half_t>(wp.data(), wp.size() * 2, NAN_F16);
    const float* db = st.upload<float>(bp.data(), bp.size() * 4, NAN_F32);
    half_t* dy = st.alloc_out<half_t>("y", M * cout * 2, (size_t)cout * 2);
    if (st.ok()) {
        ConvParams p;
        memset(&p, 0, sizeof p);
        p.x = d1; p.w = dw; p.bias = db; p.y = dy;
        p.x_img_stride = (long long)ho * wo * c1; p.y_img_stride = (long long)ho * wo * cout;
        p.x_zero_off = z1; p.x_bytes = z1 + 16u;
        p.x2 = d2; p.x2_img_stride = (long long)h2 * w2 * c2;
        p.x2_zero_off = z2; p.x2_bytes = z2 + 16u;
        p.W2 = w2; p.C2 = c2; p.stride2 = stride2; p.k1steps = c1 / 64;
        p.w_bytes = (unsigned)(wp.size() * 2);
        p.N = n; p.H = ho; p.W = wo; p.C = c1; p.P = ho; p.Q = wo; p.R = 1; p.S = 1; p.stride = 1; p.pad = 0;
        p.M = (int)M; p.cout8 = cout; p.ldw = K; p.ksteps = K / 64; p.ldy = cout; p.y_dense = 1;
        p.act = act; p.tanh_from = INT_MAX; p.n_ch_tiles = coutPad / conv_tile_ch(tile); p.k_slices = 1;
        if (conv_tile_has(tile, FORM_DUAL_SPLITK)) force_split_k(h, st, p, M, coutPad);
        if (!launch_op_conv(h, st, p, tile, coutPad)) return h->fail(YH_EINVAL, "dual conv op: no conv kernel for these parameters on this tile");
    }
    st.sync(h->stream);
    st.check_out(dy, y);
    st.check_ws();
    return st.status(h, "dual conv op: ", conv_tile_symbol(tile));
}

// One launch of bneck.hip (a row of kBneckChains, or bneck_xn_f16 for 256 planes) on caller tensors. The host arrays are already
// the kernels' panels: w2 [planes][(r, s, c)], w3 [4 planes][planes (+ 64)], w1n [planes][4 planes].
int yh_op_bneck_f16(yh_engine* h, int32_t planes, int32_t tile_m, const uint16_t* a, int32_t n, int32_t hh, int32_t ww,
                    const uint16_t* w2, const float* bias2, int32_t stride, const uint16_t* w3, const float* bias3,
                    const uint16_t* res, const uint16_t* x2, int32_t h2, int32_t w2w, int32_t stride2,
                    const uint16_t* w1n, const float* bias1n, uint16_t* y, uint16_t* a_next, uint8_t* a_next8,
                    const float* inv_scale) {
    if (!h || !a || !w3 || !bias3 || !y) return YH_EINVAL;
    if (planes != 64 && planes != 128 && planes != 256) return h->fail(YH_EINVAL, "bneck op: planes must be 64, 128 or 256");
    if (n < 1 || hh < 1 || ww < 1) return h->fail(YH_EINVAL, "bneck op: empty input");
    const bool xn = planes == 256, dual = x2 != nullptr, next = w1n != nullptr;
    const int gap = h->tune.op_xgap;
    if (gap < 0 || gap % 8 != 0) return h->fail(YH_EINVAL, "bneck op: tune.op_xgap must be a multiple of 8");
    if (next && !bias1n) return h->fail(YH_EINVAL, "bneck op: w1n without bias1n");
    int P = hh, Q = ww;
    if (xn) {
        if (tile_m != 64) return h->fail(YH_EINVAL, "bneck op: bneck_xn_f16 runs on 64-pixel tiles");
        if (dual || !res || !next) return h->fail(YH_EINVAL, "bneck op: bneck_xn_f16 needs res and w1n, and has no two-source form");
        if (!a_next && !a_next8) return h->fail(YH_EINVAL, "bneck op: bneck_xn_f16 needs a_next or a_next8");
        if (a_next8 && !inv_scale) return h->fail(YH_EINVAL, "bneck op: a_next8 without inv_scale");
        if (gap) return h->fail(YH_EINVAL, "bneck op: bneck_xn_f16 reads dense rows, tune.op_xgap must be 0");
    } else {
        if (!w2 || !bias2 || (stride != 1 && stride != 2)) return h->fail(YH_EINVAL, "bneck op: a chain needs w2, bias2 and stride 1 or 2");
        if (a_next8) return h->fail(YH_EINVAL, "bneck op: only bneck_xn_f16 writes E4M3 codes");
        if (dual && res) return h->fail(YH_EINVAL, "bneck op: the two-source form has no identity shortcut (x2 and res given)");
        if (dual && !next) return h->fail(YH_EINVAL, "bneck op: the two-source form needs w1n");
        if (!dual && !res) return h->fail(YH_EINVAL, "bneck op: need res or x2");
        if (next != (a_next != nullptr)) return h->fail(YH_EINVAL, "bneck op: a_next goes with w1n");
        if (!strcmp(bneck_symbol(planes, tile_m, next, dual), "?")) return h->fail(YH_EINVAL, "bneck op: no bneck_chain_f16 for this planes, tile_m, w1n, x2");
        P = out_dim(hh, 3, stride, 1); Q = out_dim(ww, 3, stride, 1);
        if (dual && (stride2 < 1 || h2 < 1 || w2w < 1 || (long long)(P - 1) * stride2 >= h2 || (long long)(Q - 1) * stride2 >= w2w))
            return h->fail(YH_EINVAL, "bneck op: x2 must cover the strided output grid");
    }
    HIPCHK(h, hipSetDevice(h->dev));
    const int C4 = 4 * planes, C2 = dual ? 64 : 0;
    const size_t M = (size_t)n * P * Q, img = (size_t)hh * ww * planes, n2 = dual ? (size_t)n * h2 * w2w * 64 : 0;
    std::vector<uint16_t> as((img + gap) * n, 0x7E00);   // (test hook, tune.op_xgap: NaN behind every image)
    for (int b = 0; b < n; ++b) memcpy(&as[b * (img + gap)], &a[b * img], img * 2);
    const size_t ny = M * C4, nan_ = M * planes;
    OpStaging st;
    BneckParams p;
    memset(&p, 0, sizeof p);
    unsigned z2 = 0;
    p.a = st.upload_padded<half_t>(as.data(), as.size() * 2, as.size() * 2 + 64, &p.a_zero_off);
    p.a_bytes = p.a_zero_off + 16u; p.a_img_stride = (long long)(img + gap);
    p.N = n; p.H = hh; p.W = ww; p.P = P; p.Q = Q; p.stride = xn ? 1 : stride; p.M = (int)M; p.no_b = xn ? 1 : 0;
    if (!xn) {
        p.w2_bytes = (unsigned)((size_t)planes * 9 * planes * 2);
        p.w2 = st.upload<half_t>(w2, p.w2_bytes, NAN_F16); p.bias2 = st.upload<float>(bias2, (size_t)planes * 4, NAN_F32);
    }
    p.w3_bytes = (unsigned)((size_t)C4 * (planes + C2) * 2);
    p.w3 = st.upload<half_t>(w3, p.w3_bytes, NAN_F16); p.bias3 = st.upload<float>(bias3, (size_t)C4 * 4, NAN_F32);
    if (res) { p.res_bytes = (unsigned)(ny * 2); p.res = st.upload<half_t>(res, ny * 2, NAN_F16); }
    if (dual) {
        p.x2 = st.upload_padded<half_t>(x2, n2 * 2, n2 * 2 + 64, &z2);
        p.x2_bytes = z2 + 16u; p.x2_img_stride = (long long)h2 * w2w * 64; p.W2 = w2w; p.C2 = 64; p.stride2 = stride2;
    }
    if (next) {
        p.w1n_bytes = (unsigned)((size_t)planes * C4 * 2);
        p.w1n = st.upload<half_t>(w1n, p.w1n_bytes, NAN_F16); p.bias1n = st.upload<float>(bias1n, (size_t)planes * 4, NAN_F32);
    }
    p.y = st.alloc_out<half_t>("y", ny * 2, (size_t)C4 * 2);
    if (a_next) p.a_next = st.alloc_out<half_t>("a_next", nan_ * 2, (size_t)planes * 2);
    if (a_next8) { p.a_next8 = st.alloc_out<uint8_t>("a_next8", nan_, (size_t)planes); p.a_next8_inv = st.upload<float>(inv_scale, (size_t)planes * 4, NAN_F32); }
    if (st.ok()) {
        if (bneck_set_geometry(p) != hipSuccess) return h->fail(YH_EINVAL, "bneck op: row geometry out of range");
        st.e = launch_bneck(p, planes, tile_m, h->stream);
        if (st.e == hipErrorInvalidValue) return h->fail(YH_EINVAL, "bneck op: launch_bneck has no kernel for these parameters");   // (nothing was launched)
    }
    st.sync(h->stream);
    st.check_out(p.y, y);
    if (a_next) st.check_out(p.a_next, a_next);
    if (a_next8) st.check_out(p.a_next8, a_next8);
    return st.status(h, "bneck op: ", bneck_symbol(planes, tile_m, next, dual));
}

int yh_op_conv2d_levels_f16(yh_engine* h, const uint16_t* x, int32_t n, const int32_t* level_sizes, int32_t nlev, int32_t cin,
                            const uint16_t* w, const float* bias, int32_t cout, int32_t k, int32_t act, uint16_t* y) {
    if (!level_sizes || nlev < 1 || nlev > 5 || cin % 64 != 0 || (k != 1 && k != 3)) return YH_EINVAL;
    int cells = 0;
    for (int l = 0; l < nlev; ++l) { if (level_sizes[l] < 1) return YH_EINVAL; cells += level_sizes[l] * level_sizes[l]; }
    return op_conv2d_impl(h, x, n, cells, 1, cin, w, bias, cout, k, k, 1, k / 2, nullptr, act, y, level_sizes, nlev);
}

int yh_op_bilinear_f16(yh_engine* h, const uint16_t* x, int32_t n, int32_t hh, int32_t ww, int32_t c, int32_t ho, int32_t wo, uint16_t* y) {
    if (!h || !x || !y || c % 8 != 0 || n < 1) return YH_EINVAL;
    HIPCHK(h, hipSetDevice(h->dev));
    const size_t ni = (size_t)n * hh * ww * c, no = (size_t)n * ho * wo * c;
    OpStaging st;
    const half_t* dx = st.upload<half_t>(x, ni * 2, NAN_F16);
    half_t* dy = st.alloc_out<half_t>("y", no * 2, (size_t)c * 2);
    if (st.ok()) st.e = launch_bilinear(dx, dy, n, hh, ww, c, ho, wo, (long long)hh * ww * c, (long long)ho * wo * c, h->stream);
    st.sync(h->stream);
    st.check_out(dy, y);
    return st.status(h, "bilinear op: ", "");
}

int yh_op_maxpool3x3s2_f16(yh_engine* h, const uint16_t* x, int32_t n, int32_t hh, int32_t ww, int32_t c, uint16_t* y) {
    if (!h || !x || !y || c % 8 != 0 || n < 1) return YH_EINVAL;
    HIPCHK(h, hipSetDevice(h->dev));
    const int ho = out_dim(hh, 3, 2, 1), wo = out_dim(ww, 3, 2, 1);
    const size_t ni = (size_t)n * hh * ww * c, no = (size_t)n * ho * wo * c;
    OpStaging st;
    const half_t* dx = st.upload<half_t>(x, ni * 2, NAN_F16);
    half_t* dy = st.alloc_out<half_t>("y", no * 2, (size_t)c * 2);
    if (st.ok()) st.e = launch_maxpool3x3s2(dx, dy, n, hh, ww, c, ho, wo, h->stream);
    st.sync(h->stream);
    st.check_out(dy, y);
    return st.status(h, "maxpool op: ", "maxpool3x3s2_f16");
}

static int op_stem_pool_impl(yh_engine* h, const uint16_t* x, const uint8_t* rgb, int32_t n, int32_t S, const uint16_t* w, const float* bias,
                             uint16_t* stem_out, uint16_t* pool_out) {
    if (!h || (!x && !rgb) || !w || !bias || !pool_out || n < 1 || S < 8 || (S & 1)) return YH_EINVAL;
    HIPCHK(h, hipSetDevice(h->dev));
    const int Hp = S + 8, SO = out_dim(S, 7, 2, 3), PO = out_dim(SO, 3, 2, 1);
    // host-side staging, as the engine does it: zero-bordered 4-channel image, stem panel [64][256]
    std::vector<uint16_t> xs((size_t)n * Hp * Hp * 4, 0), wp((size_t)64 * 256, 0);
    if (x)
    for (int b = 0; b < n; ++b)
        for (int yy = 0; yy < S; ++yy)
            for (int xx = 0; xx < S; ++xx)
                memcpy(&xs[(((size_t)b * Hp + yy + 3) * Hp + xx + 3) * 4], &x[(((size_t)b * S + yy) * S + xx) * 3], 6);
    for (int o = 0; o < 64; ++o)
        for (int r = 0; r < 7; ++r)
            for (int sx = 0; sx < 7; ++sx)
                for (int c = 0; c < 3; ++c) wp[(size_t)o * 256 + r * 32 + sx * 4 + c] = w[(((size_t)o * 7 + r) * 7 + sx) * 3 + c];
    const size_t ns = (size_t)n * SO * SO * 64, np = (size_t)n * PO * PO * 64;
    OpStaging st;
    const half_t* dx = st.upload<half_t>(xs.data(), xs.size() * 2, NAN_F16);
    const uint8_t* drgb = rgb ? st.upload<uint8_t>(rgb, (size_t)n * S * S * 3, NAN_BYTE) : nullptr;
    const half_t* dw = st.upload<half_t>(wp.data(), wp.size() * 2, NAN_F16);
    const float* db = st.upload<float>(bias, 64 * 4, NAN_F32);
    // (the stem output is staged, and its guards checked, when the launch is told not to write it too)
    half_t* ds = st.alloc_out<half_t>("stem", ns * 2, 64 * 2);
    half_t* dp = st.alloc_out<half_t>("pool", np * 2, 64 * 2);
    if (st.ok()) {
        StemPoolParams sp;
        sp.x = dx; sp.w = dw; sp.bias = db; sp.pool = dp;
        sp.rgb = drgb; sp.S = S;
        sp.stem = stem_out ? ds : nullptr;
        sp.n = n; sp.Hp = Hp; sp.Wp = Hp; sp.SO = SO; sp.PO = PO; sp.tiles_y = (PO + 7) / 8; sp.tiles_x = (PO + 7) / 8;
        sp.x_img_stride = (long long)Hp * Hp * 4; sp.pool_img_stride = (long long)PO * PO * 64; sp.stem_img_stride = (long long)SO * SO * 64;
        st.e = launch_stem_pool(sp, h->stream);
    }
    st.sync(h->stream);
    st.check_out(ds, stem_out);
    st.check_out(dp, pool_out);
    return st.status(h, "stem+pool op: ", "stem_pool_f16");
}

int yh_op_stem_pool_f16(yh_engine* h, const uint16_t* x, int32_t n, int32_t S, const uint16_t* w, const float* bias,
                        uint16_t* stem_out, uint16_t* pool_out) {
    return op_stem_pool_impl(h, x, nullptr, n, S, w, bias, stem_out, pool_out);
}
int yh_op_stem_pool_rgb8(yh_engine* h, const uint8_t* rgb, int32_t n, int32_t S, const uint16_t* w, const float* bias,
                         uint16_t* stem_out, uint16_t* pool_out) {
    return op_stem_pool_impl(h, nullptr, rgb, n, S, w, bias, stem_out, pool_out);
}

// Experimental: the fp8 form of the convolution (the 256x256 tile unless tune.op_tile names another fp8 tile). x: E4M3
// codes [n][hh][ww][cin], w: E4M3 codes [cout][k][k][cin], out = act(acc * scale[ch] + bias[ch] (+ residual)) as f16.
// nlev > 0: the multi-level form, x [n][cells][cin] (hh = cells, ww = 1) as in op_conv2d_impl.
static int op_conv2d_fp8_impl(yh_engine* h, const uint8_t* x, int32_t n, int32_t hh, int32_t ww, int32_t cin, const uint8_t* w,
                              const float* scale, const float* bias, int32_t cout, int32_t k, int32_t stride, int32_t pad,
                              const uint16_t* residual, int32_t act, uint16_t* y, int32_t reps, float* ms_per_launch,
                              const int32_t* level_sizes, int32_t nlev) {
    if (!h || !x || !w || !scale || !bias || !y || n < 1 || k < 1 || stride < 1 || cout < 1 || cin < 128 || cin % 128 != 0 || (act < 0 || act > 1))
        return h ? h->fail(YH_EINVAL, "fp8 conv op: need cin % 128 == 0") : YH_EINVAL;
    const ConvTile tile = h->tune.op_tile >= 0 ? (ConvTile)h->tune.op_tile : TILE_256x256_FP8;
    if (!conv_tile_fp8(tile) || !conv_tile_has(tile, nlev > 0 ? FORM_ML : FORM_PLAIN))
        return h->fail(YH_EINVAL, "fp8 conv op: tune.op_tile is not an fp8 tile of this form");
    HIPCHK(h, hipSetDevice(h->dev));
    const int P = nlev > 0 ? hh : out_dim(hh, k, stride, pad), Q = nlev > 0 ? 1 : out_dim(ww, k, stride, pad);
    if (P < 1 || Q < 1) return h->fail(YH_EINVAL, "fp8 conv op: empty output");
    const int tch = conv_tile_ch(tile), Kpad = k * k * cin, coutPad = round_up(cout, tch), cout8 = round_up(cout, 8);
    const size_t M = (size_t)n * P * Q, xbytes = (size_t)n * hh * ww * cin;
    const std::vector<uint8_t> wp = pad_rows(w, 1, (size_t)cout * Kpad, (size_t)coutPad * Kpad);   // [cout][k][k][cin] is already the panel's K order
    const std::vector<float> bp = pad_rows(bias, 1, cout, coutPad), sp = pad_rows(scale, 1, cout, coutPad);
    std::vector<uint16_t> rs, ys(M * cout8);
    if (residual) rs = pad_rows(residual, M, cout, cout8);
    OpStaging st;
    unsigned zo = 0;
    const half_t* dx = st.upload_padded<half_t>(x, xbytes, pad16(xbytes) + 64, &zo, NAN_BYTE);
    const half_t* dw = st.upload<half_t>(wp.data(), wp.size(), NAN_BYTE);
    const float* db = st.upload<float>(bp.data(), bp.size() * 4, NAN_F32);
    const float* dsc = st.upload<float>(sp.data(), sp.size() * 4, NAN_F32);
    half_t* dy = st.alloc_out<half_t>("y", ys.size() * 2, (size_t)cout8 * 2);
    const half_t* dr = residual ? st.upload<half_t>(rs.data(), rs.size() * 2, NAN_F16) : nullptr;
    if (st.ok()) {
        ConvParams p;
        memset(&p, 0, sizeof p);
        p.x = dx; p.w = dw; p.bias = db; p.scale = dsc; p.res = dr; p.y = dy;
        // the loader's units are 2 bytes: two fp8 values
        p.x_img_stride = (long long)hh * ww * (cin / 2); p.y_img_stride = (long long)P * Q * cout8; p.res_img_stride = p.y_img_stride;
        p.x_zero_off = zo; p.x_bytes = zo + 16u; p.w_bytes = (unsigned)wp.size();
        p.N = n; p.H = hh; p.W = ww; p.C = cin / 2; p.P = P; p.Q = Q; p.R = k; p.S = k; p.stride = stride; p.pad = pad;
        p.M = (int)M; p.cout8 = cout8; p.ldw = Kpad / 2; p.ksteps = Kpad / 128; p.ldy = cout8; p.ldres = cout8; p.y_dense = 1;
        p.act = act; p.tanh_from = INT_MAX; p.n_ch_tiles = coutPad / tch; p.k_slices = 1;
        if (nlev > 0) {
            p.nlev = nlev;
            for (int l = 0, s = 0; l < nlev; ++l) { p.lev_start[l] = s; p.lev_h[l] = p.lev_w[l] = level_sizes[l]; s += level_sizes[l] * level_sizes[l]; }
        }
        if (conv_set_geometry(p, tile) != hipSuccess || !conv_launchable(p, tile)) return h->fail(YH_EINVAL, "fp8 conv op: no conv kernel for these parameters on this tile");
        int form = -1;
        st.e = launch_conv(p, tile, h->stream, &form);
        if (st.ok()) { h->last_conv_launches = 1; h->last_conv_forms.assign({ (int)tile, form }); }
        st.sync(h->stream);
        if (st.ok() && reps > 0 && ms_per_launch) {          // timing: reps back-to-back launches between two events
            hipEventRecord(h->ev0, h->stream);
            for (int r = 0; r < reps && st.ok(); ++r) st.e = launch_conv(p, tile, h->stream);
            hipEventRecord(h->ev1, h->stream);
            if (st.ok()) st.e = hipEventSynchronize(h->ev1);
            float ms = 0; hipEventElapsedTime(&ms, h->ev0, h->ev1);
            *ms_per_launch = ms / reps;
        }
    }
    st.check_out(dy, ys.data());
    if (const int rc = st.status(h, "fp8 conv op: ", conv_tile_symbol(tile))) return rc;
    unpad_rows(y, ys, M, cout, cout8);
    return YH_OK;
}

int yh_op_conv2d_fp8(yh_engine* h, const uint8_t* x, int32_t n, int32_t hh, int32_t ww, int32_t cin, const uint8_t* w,
                     const float* scale, const float* bias, int32_t cout, int32_t k, int32_t stride, int32_t pad,
                     const uint16_t* residual, int32_t act, uint16_t* y, int32_t reps, float* ms_per_launch) {
    return op_conv2d_fp8_impl(h, x, n, hh, ww, cin, w, scale, bias, cout, k, stride, pad, residual, act, y, reps, ms_per_launch, nullptr, 0);
}

int yh_op_conv2d_levels_fp8(yh_engine* h, const uint8_t* x, int32_t n, const int32_t* level_sizes, int32_t nlev, int32_t cin,
                            const uint8_t* w, const float* scale, const float* bias, int32_t cout, int32_t k, int32_t act, uint16_t* y) {
    if (!level_sizes || nlev < 1 || nlev > 5 || (k != 1 && k != 3)) return YH_EINVAL;
    int cells = 0;
    for (int l = 0; l < nlev; ++l) { if (level_sizes[l] < 1) return YH_EINVAL; cells += level_sizes[l] * level_sizes[l]; }
    return op_conv2d_fp8_impl(h, x, n, cells, 1, cin, w, scale, bias, cout, k, 1, k / 2, nullptr, act, y, 0, nullptr, level_sizes, nlev);
}

// The FPN lateral as the engine launches it (fill_conv_params with Op::res_up): a 1x1 conv, the residual the lower level resized in
// the epilogue - or, under a forced split-K, in splitk_reduce_f16.
int yh_op_conv2d_resup_f16(yh_engine* h, const uint16_t* x, int32_t n, int32_t P, int32_t Q, int32_t cin, const uint16_t* w,
                           const float* bias, int32_t cout, const uint16_t* res_lo, int32_t rh, int32_t rw, int32_t act, uint16_t* y) {
    if (!h || !x || !w || !bias || !res_lo || !y) return YH_EINVAL;
    if (n < 1 || P < 1 || Q < 1 || rh < 1 || rw < 1 || cout < 1 || cin < 64 || cin % 64 != 0 || act < 0 || act > 1)
        return h->fail(YH_EINVAL, "resup conv op: need cin % 64 == 0, act 0 or 1 and non-empty tensors");
    const ConvTile tile = h->tune.op_tile >= 0 ? (ConvTile)h->tune.op_tile : TILE_128x128;
    if (!conv_tile_has(tile, FORM_RESUP)) return h->fail(YH_EINVAL, "resup conv op: tune.op_tile is not a tile of the upsampled-residual form");
    HIPCHK(h, hipSetDevice(h->dev));
    const int tch = conv_tile_ch(tile), coutPad = round_up(cout, tch), cout8 = round_up(cout, 8);
    const size_t M = (size_t)n * P * Q, Mr = (size_t)n * rh * rw, nx = M * cin;
    const std::vector<uint16_t> wp = pad_rows(w, 1, (size_t)cout * cin, (size_t)coutPad * cin);
    const std::vector<float> bp = pad_rows(bias, 1, cout, coutPad);
    const std::vector<uint16_t> rs = pad_rows(res_lo, Mr, cout, cout8);
    std::vector<uint16_t> ys(M * cout8);
    OpStaging st;
    unsigned zo = 0;
    const half_t* dx = st.upload_padded<half_t>(x, nx * 2, nx * 2 + 64, &zo);
    const half_t* dw = st.upload<half_t>(wp.data(), wp.size() * 2, NAN_F16);
    const float* db = st.upload<float>(bp.data(), bp.size() * 4, NAN_F32);
    const half_t* dr = st.upload<half_t>(rs.data(), rs.size() * 2, NAN_F16);
    half_t* dy = st.alloc_out<half_t>("y", ys.size() * 2, (size_t)cout8 * 2);
    if (st.ok()) {
        ConvParams p;
        memset(&p, 0, sizeof p);
        p.x = dx; p.w = dw; p.bias = db; p.res = dr; p.y = dy;
        p.res_up = 1; p.res_h = rh; p.res_w = rw;
        p.x_img_stride = (long long)P * Q * cin; p.y_img_stride = (long long)P * Q * cout8; p.res_img_stride = (long long)rh * rw * cout8;
        p.x_zero_off = zo; p.x_bytes = zo + 16u; p.w_bytes = (unsigned)(wp.size() * 2);
        p.N = n; p.H = P; p.W = Q; p.C = cin; p.P = P; p.Q = Q; p.R = 1; p.S = 1; p.stride = 1; p.pad = 0;
        p.M = (int)M; p.cout8 = cout8; p.ldw = cin; p.ksteps = cin / 64; p.ldy = cout8; p.ldres = cout8; p.y_dense = 1;
        p.act = act; p.tanh_from = INT_MAX; p.n_ch_tiles = coutPad / tch; p.k_slices = 1;
        if (conv_tile_has(tile, FORM_SPLITK)) force_split_k(h, st, p, M, coutPad);
        if (!launch_op_conv(h, st, p, tile, coutPad)) return h->fail(YH_EINVAL, "resup conv op: no conv kernel for these parameters on this tile");
    }
    st.sync(h->stream);
    st.check_out(dy, ys.data());
    st.check_ws();
    if (const int rc = st.status(h, "resup conv op: ", conv_tile_symbol(tile))) return rc;
    unpad_rows(y, ys, M, cout, cout8);
    return YH_OK;
}

// The protonet's last two layers as the engine launches them (fill_conv_params with Op::tail_op): the first conv's 256 channels stay in
// LDS, only y2 is written. fp8: x and w are E4M3 codes (scale given), the loader's units two codes.
static int op_conv2d_tail_impl(yh_engine* h, const void* x, int32_t n, int32_t hh, int32_t ww, int32_t cin, const void* w, const float* scale,
                               const float* bias, int32_t cout, int32_t k, int32_t act, const uint16_t* w2, const float* bias2, uint16_t* y2,
                               bool fp8) {
    const char* const what = fp8 ? "fp8 tail conv op: " : "tail conv op: ";
    if (!h || !x || !w || !bias || !w2 || !bias2 || !y2 || (fp8 && !scale)) return YH_EINVAL;
    const int cq = fp8 ? 128 : 64;   // channels per K step
    if (n < 1 || hh < 1 || ww < 1 || k < 1 || !(k & 1) || cin < cq || cin % cq != 0 || act < 0 || act > 1)
        return h->fail(YH_EINVAL, std::string(what) + "need an odd square kernel, act 0 or 1 and cin a multiple of a K step");
    if (cout != 256) return h->fail(YH_EINVAL, std::string(what) + "the fused 1x1 tail runs on a convolution to exactly 256 channels");
    const ConvTile tile = h->tune.op_tile >= 0 ? (ConvTile)h->tune.op_tile : (fp8 ? TILE_256x256_FP8 : TILE_256x256_M16);
    if (!conv_tile_has(tile, FORM_TAIL) || conv_tile_fp8(tile) != fp8) return h->fail(YH_EINVAL, std::string(what) + "tune.op_tile is not a tile of the fused-tail form");
    HIPCHK(h, hipSetDevice(h->dev));
    const int es = fp8 ? 1 : 2, Kpad = k * k * cin;           // bytes per operand element
    const size_t M = (size_t)n * hh * ww, xbytes = M * cin * es, wbytes = (size_t)256 * Kpad * es, ny = M * 32;
    const NanBand nan = fp8 ? NAN_BYTE : NAN_F16;
    OpStaging st;
    unsigned zo = 0;
    const half_t* dx = st.upload_padded<half_t>(x, xbytes, pad16(xbytes) + 64, &zo, nan);
    const half_t* dw = st.upload<half_t>(w, wbytes, nan);
    const float* db = st.upload<float>(bias, 256 * 4, NAN_F32);
    const float* dsc = fp8 ? st.upload<float>(scale, 256 * 4, NAN_F32) : nullptr;
    const half_t* dw2 = st.upload<half_t>(w2, (size_t)32 * 256 * 2, NAN_F16);
    const float* db2 = st.upload<float>(bias2, 32 * 4, NAN_F32);
    half_t* dy2 = st.alloc_out<half_t>("y2", ny * 2, 32 * 2);   // (the only output: y and y8 are nullptr in this launch)
    if (st.ok()) {
        ConvParams p;
        memset(&p, 0, sizeof p);
        const int C = fp8 ? cin / 2 : cin;   // (fp8: the loader's units are 2 bytes, two codes)
        p.x = dx; p.w = dw; p.bias = db; p.scale = dsc; p.w2 = dw2; p.bias2 = db2; p.y2 = dy2;
        p.x_img_stride = (long long)hh * ww * C; p.y_img_stride = (long long)hh * ww * 256;
        p.x_zero_off = zo; p.x_bytes = zo + 16u; p.w_bytes = (unsigned)wbytes;
        p.N = n; p.H = hh; p.W = ww; p.C = C; p.P = hh; p.Q = ww; p.R = k; p.S = k; p.stride = 1; p.pad = k / 2;
        p.M = (int)M; p.cout8 = 256; p.ldw = fp8 ? Kpad / 2 : Kpad; p.ksteps = Kpad / cq; p.ldy = 256; p.y_dense = 1;
        p.act = act; p.tanh_from = INT_MAX; p.n_ch_tiles = 1; p.k_slices = 1;
        if (!launch_op_conv(h, st, p, tile, 256)) return h->fail(YH_EINVAL, std::string(what) + "no conv kernel for these parameters on this tile");
    }
    st.sync(h->stream);
    st.check_out(dy2, y2);
    return st.status(h, what, std::string(conv_tile_symbol(tile)) + "[+1x1]");
}

int yh_op_conv2d_tail_f16(yh_engine* h, const uint16_t* x, int32_t n, int32_t hh, int32_t ww, int32_t cin, const uint16_t* w,
                          const float* bias, int32_t cout, int32_t k, int32_t act, const uint16_t* w2, const float* bias2, uint16_t* y2) {
    return op_conv2d_tail_impl(h, x, n, hh, ww, cin, w, nullptr, bias, cout, k, act, w2, bias2, y2, false);
}
int yh_op_conv2d_tail_fp8(yh_engine* h, const uint8_t* x, int32_t n, int32_t hh, int32_t ww, int32_t cin, const uint8_t* w,
                          const float* scale, const float* bias, int32_t cout, int32_t k, int32_t act, const uint16_t* w2,
                          const float* bias2, uint16_t* y2) {
    return op_conv2d_tail_impl(h, x, n, hh, ww, cin, w, scale, bias, cout, k, act, w2, bias2, y2, true);
}

int yh_op_quantize_e4m3(yh_engine* h, const uint16_t* x, size_t n, float inv_scale, uint8_t* y) {
    if (!h || !x || !y || n < 1) return YH_EINVAL;
    HIPCHK(h, hipSetDevice(h->dev));
    OpStaging st;
    const half_t* dx = st.upload<half_t>(x, n * 2, NAN_F16);
    uint8_t* dy = st.alloc_out<uint8_t>("y", n, 0);
    if (st.ok()) st.e = launch_quantize_e4m3(dx, dy, (long long)n, inv_scale, h->stream);
    st.sync(h->stream);
    st.check_out(dy, y);
    return st.status(h, "quantize op: ", "quantize_e4m3");
}

int yh_op_absmax_channels_f16(yh_engine* h, const uint16_t* x, int64_t rows, int32_t C, uint32_t* out_bits) {
    if (!h || !x || !out_bits || rows < 1 || C < 1) return YH_EINVAL;
    HIPCHK(h, hipSetDevice(h->dev));
    OpStaging st;
    const half_t* dx = st.upload<half_t>(x, (size_t)rows * C * 2, NAN_F16);
    unsigned* dm = st.alloc_out<unsigned>("out_bits", (size_t)C * 4, 0);
    if (st.ok()) st.e = hipMemsetAsync(dm, 0, (size_t)C * 4, h->stream);   // (on the kernel's stream, as the calibration does: its atomicMax starts from these zeros)
    if (st.ok()) {
        st.e = launch_absmax_channels_f16(dx, (long long)rows, C, dm, h->stream);
        if (st.e == hipErrorInvalidValue) return h->fail(YH_EINVAL, "absmax op: C must be a multiple of 8 with 256 % (C / 8) == 0");   // (nothing was launched)
    }
    st.sync(h->stream);
    st.check_out(dm, out_bits);
    return st.status(h, "absmax op: ", "absmax_channels_f16");
}

// The check of the checker (no kernel): a guarded output of 3 rows x 64 f16 through alloc_out, one guard byte changed by a copy at
// `where` - 0 none, 1 the front guard's last byte, 2 the first byte behind the payload, 3 the back guard's last byte, 4 the front
// guard's first byte - and check_out on it. Every byte written lies inside the call's own allocation.
int yh_debug_guard_selfcheck(yh_engine* h, int32_t where) {
    if (!h) return YH_EINVAL;
    if (where < 0 || where > 4) return h->fail(YH_EINVAL, "guard selfcheck: where must be 0 .. 4");
    HIPCHK(h, hipSetDevice(h->dev));
    constexpr size_t row_bytes = 64 * 2, bytes = 3 * row_bytes, B = OpStaging::kBand;
    OpStaging st;
    const uint16_t* d = st.alloc_out<uint16_t>("y", bytes, row_bytes);
    if (st.ok() && where > 0) {
        const OpStaging::Out& o = st.outs.back();
        const size_t at[5] = { 0, B - 1, B + bytes, B + bytes + o.back - 1, 0 };
        const uint8_t changed = 0x00;
        st.put(o.base + at[where], &changed, 1);
    }
    st.check_out(d, nullptr);
    return st.status(h, "guard selfcheck: ", "");
}

int yh_op_detect(yh_engine* h, const uint16_t* loc, const uint16_t* conf, const uint16_t* mask, const uint16_t* proto, int32_t n) {
    if (!h || !loc || !conf || !mask || !proto) return YH_EINVAL;
    if (n < 1 || n > h->cfg.max_batch) return h->fail(YH_EINVAL, "n out of range");
    HIPCHK(h, hipSetDevice(h->dev));
    // interleave into the fused head rows [n][cells][ldh]
    const int C = h->C, ldh = h->ldh;
    std::vector<uint16_t> rows((size_t)n * h->cells * ldh, 0);
    for (size_t r = 0; r < (size_t)n * h->cells; ++r) {
        uint16_t* d = &rows[r * ldh];
        memcpy(d, &loc[r * 12], 24);
        memcpy(d + 12, &conf[r * 3 * C], (size_t)3 * C * 2);
        memcpy(d + 12 + 3 * C, &mask[r * 96], 192);
    }
    HIPCHK(h, hipMemcpy(h->heads.d, rows.data(), rows.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->proto.d, proto, (size_t)n * h->hp * h->wp * 32 * 2, hipMemcpyHostToDevice));
    h->cur_n = n;
    h->det.n = n;
    h->dets_valid = false;   // (a tail on caller-provided heads is not a yh_evaluate)
    hipError_t e = launch_detect(h->det, h->stream);
    if (e != hipSuccess) return h->fail(YH_EHIP, std::string("detect: ") + hipGetErrorString(e));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return YH_OK;
}

// The instance frame's kernels (instance.hip) on caller-provided masks of any hp x wp: what yh_instance_frame runs on the tail's
// (trk: what yh_instance_track runs, instance_track.hip's kernels between them).
static int op_instance_impl(yh_engine* h, const uint8_t* masks, const int32_t* class_ids, const float* scores, int32_t n, int32_t hp,
                            int32_t wp, int32_t width, int32_t height, const uint8_t* class_map, float min_score, uint32_t* out_host,
                            int32_t* table, int32_t table_capacity, int32_t* n_instances, const InstTrack* trk) {
    if (!h || !out_host || !n_instances || (n > 0 && (!masks || !class_ids || !scores))) return YH_EINVAL;
    if (n < 0 || n > h->cfg.max_dets) return h->fail(YH_EINVAL, "instance frame op: n outside 0 .. max_dets");
    if (hp < 1 || hp > 4096 || wp < 1 || wp > 4096) return h->fail(YH_EINVAL, "instance frame op: hp and wp must be in 1 .. 4096");
    for (int d = 0; d < n; ++d)
        if (class_ids[d] < 0 || class_ids[d] >= h->C - 1) return h->fail(YH_EINVAL, "instance frame op: class id out of range");
    if (const char* why = instance_check(width, height, class_map, h->C - 1, min_score)) return h->fail(YH_EINVAL, why);
    if (trk)
        if (const char* why = track_check(trk->iou_permille, trk->max_age)) return h->fail(YH_EINVAL, why);
    HIPCHK(h, hipSetDevice(h->dev));
    const size_t px = (size_t)hp * wp;
    std::vector<yh_detection> dets((size_t)(n > 0 ? n : 1));
    memset(dets.data(), 0, dets.size() * sizeof(yh_detection));
    for (int d = 0; d < n; ++d) { dets[d].class_id = class_ids[d]; dets[d].score = scores[d]; }
    OpStaging st;
    // (0xFF behind the n masks in use: the slots past the count are stale in the engine too, and must not be read)
    uint8_t* dm = st.alloc<uint8_t>((size_t)h->cfg.max_dets * px, 0xFF);
    if (n > 0) st.put(dm, masks, (size_t)n * px);
    const yh_detection* dd = st.upload_raw<yh_detection>(dets.data(), dets.size() * sizeof(yh_detection));
    const int* dc = st.upload_raw<int>(&n, sizeof(int));
    if (const int rc = st.status(h, "instance frame op: ")) {
        if (trk) track_drop(h);
        return rc;
    }
    if (const int rc = instance_run(h, dm, dd, dc, h->cfg.max_dets, hp, wp, width, height, class_map, min_score, out_host, trk)) return rc;
    return yh_instance_read(h, n_instances, table, table_capacity);
}

int yh_op_instance_frame(yh_engine* h, const uint8_t* masks, const int32_t* class_ids, const float* scores, int32_t n, int32_t hp, int32_t wp,
                         int32_t width, int32_t height, const uint8_t* class_map, float min_score, uint32_t* out_host, int32_t* table,
                         int32_t table_capacity, int32_t* n_instances) {
    return op_instance_impl(h, masks, class_ids, scores, n, hp, wp, width, height, class_map, min_score, out_host, table, table_capacity,
                            n_instances, nullptr);
}

int yh_op_instance_track(yh_engine* h, const uint8_t* masks, const int32_t* class_ids, const float* scores, int32_t n, int32_t hp, int32_t wp,
                         int32_t width, int32_t height, const uint8_t* class_map, float min_score, int32_t iou_permille, int32_t max_age,
                         uint32_t* out_host, int32_t* table, int32_t table_capacity, int32_t* n_instances) {
    const InstTrack trk = { iou_permille, max_age };
    return op_instance_impl(h, masks, class_ids, scores, n, hp, wp, width, height, class_map, min_score, out_host, table, table_capacity,
                            n_instances, &trk);
}

// The instance batch's kernels (instance_batch.hip) on caller-provided detections of n_frames frames, n_dets slots each: what
// yh_instance_batch runs on the tail's. The slots past a frame's count are uploaded as 0xFF: a kernel that read them would paint them.
// (trk: what yh_instance_track_batch runs, instance_track_batch.hip's rounds between the two launches, on the handle's bank.)
static int op_instance_batch_impl(yh_engine* h, const uint8_t* masks, const int32_t* class_ids, const float* scores, const int32_t* counts,
                                  int32_t n_frames, int32_t n_dets, int32_t hp, int32_t wp, int32_t width, int32_t height,
                                  const uint8_t* class_map, float min_score, uint32_t* out_host, const InstTrackBatch* trk) {
    if (!h || !counts || (n_dets > 0 && (!masks || !class_ids || !scores))) return YH_EINVAL;
    if (n_frames < 1 || n_frames > 64) return h->fail(YH_EINVAL, "instance batch op: n_frames outside 1 .. 64");
    if (n_dets < 0 || n_dets > h->cfg.max_dets) return h->fail(YH_EINVAL, "instance batch op: n_dets outside 0 .. max_dets");
    if (hp < 1 || hp > 4096 || wp < 1 || wp > 4096) return h->fail(YH_EINVAL, "instance batch op: hp and wp must be in 1 .. 4096");
    for (int b = 0; b < n_frames; ++b) {
        if (counts[b] < 0 || counts[b] > n_dets) return h->fail(YH_EINVAL, "instance batch op: a count outside 0 .. n_dets");
        for (int d = 0; d < counts[b]; ++d)
            if (class_ids[(size_t)b * n_dets + d] < 0 || class_ids[(size_t)b * n_dets + d] >= h->C - 1)
                return h->fail(YH_EINVAL, "instance batch op: class id out of range");
    }
    if (const char* why = instance_check(width, height, class_map, h->C - 1, min_score)) return h->fail(YH_EINVAL, why);
    if (trk) {
        if (const char* why = track_check(trk->p.iou_permille, trk->p.max_age)) return h->fail(YH_EINVAL, why);
        const std::string why = track_batch_check(n_frames, trk->streams);
        if (!why.empty()) return h->fail(YH_EINVAL, why);
    }
    HIPCHK(h, hipSetDevice(h->dev));
    const size_t px = (size_t)hp * wp, slots = (size_t)n_frames * n_dets;
    std::vector<yh_detection> dets(slots + 1);
    memset(dets.data(), 0, dets.size() * sizeof(yh_detection));
    std::vector<uint8_t> ms(slots * px + 1, 0xFF);
    for (int b = 0; b < n_frames; ++b) {
        const size_t o = (size_t)b * n_dets;
        if (counts[b] > 0) memcpy(&ms[o * px], &masks[o * px], (size_t)counts[b] * px);
        for (int d = 0; d < counts[b]; ++d) { dets[o + d].class_id = class_ids[o + d]; dets[o + d].score = scores[o + d]; }
    }
    OpStaging st;
    const uint8_t* dm = st.upload_raw<uint8_t>(ms.data(), ms.size());
    const yh_detection* dd = st.upload_raw<yh_detection>(dets.data(), dets.size() * sizeof(yh_detection));
    const int* dc = st.upload_raw<int>(counts, (size_t)n_frames * sizeof(int));
    if (const int rc = st.status(h, "instance batch op: ")) {
        if (trk) track_batch_drop(h, n_frames, *trk);
        return rc;
    }
    return instance_batch_run(h, dm, dd, dc, n_dets, n_frames, hp, wp, width, height, class_map, min_score, out_host, trk);
}

int yh_op_instance_batch(yh_engine* h, const uint8_t* masks, const int32_t* class_ids, const float* scores, const int32_t* counts,
                         int32_t n_frames, int32_t n_dets, int32_t hp, int32_t wp, int32_t width, int32_t height, const uint8_t* class_map,
                         float min_score, uint32_t* out_host) {
    return op_instance_batch_impl(h, masks, class_ids, scores, counts, n_frames, n_dets, hp, wp, width, height, class_map, min_score,
                                  out_host, nullptr);
}

int yh_op_instance_track_batch(yh_engine* h, const uint8_t* masks, const int32_t* class_ids, const float* scores, const int32_t* counts,
                               int32_t n_frames, int32_t n_dets, int32_t hp, int32_t wp, int32_t width, int32_t height,
                               const uint8_t* class_map, float min_score, int32_t iou_permille, int32_t max_age, const int32_t* streams,
                               uint32_t* out_host) {
    const InstTrackBatch trk = { { iou_permille, max_age }, streams };
    return op_instance_batch_impl(h, masks, class_ids, scores, counts, n_frames, n_dets, hp, wp, width, height, class_map, min_score,
                                  out_host, &trk);
}

}  // extern "C"
