// engine_probe.hip - what looks INTO a handle: tensor readers, allocation map, graph-node dump, per-launch profiler, step timers,
// CU mask, phase runs (yh_debug_*, yh_profile_*, yh_time_steps: include/yolact_hip_debug.h).
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "engine.h"

using namespace yh;

extern "C" {

int yh_debug_set_cu_mask(yh_engine* h, const uint32_t* mask, int32_t n_words) {
    if (!h || !mask || n_words < 1 || n_words > 16) return YH_EINVAL;
    HIPCHK(h, hipSetDevice(h->dev));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->side));
    drop_graphs(h);   // captured for the old streams
    hipStream_t ns = nullptr, nd = nullptr;
    HIPCHK(h, hipExtStreamCreateWithCUMask(&ns, (uint32_t)n_words, mask));
    const hipError_t e2 = hipExtStreamCreateWithCUMask(&nd, (uint32_t)n_words, mask);
    if (e2 != hipSuccess) { hipStreamDestroy(ns); return h->fail(YH_EHIP, std::string("hipExtStreamCreateWithCUMask: ") + hipGetErrorString(e2)); }   // (the handle keeps its streams)
    hipStreamDestroy(h->stream); hipStreamDestroy(h->side);
    h->stream = ns; h->side = nd;
    return YH_OK;
}

int yh_debug_run_phase(yh_engine* h, int32_t phase, int32_t reps, float* ms_total) {
    if (!h || reps < 1 || (phase != 0 && phase != 1)) return YH_EINVAL;
    if (!h->weights_loaded || h->cur_n < 1) return h->fail(YH_ESTATE, "weights and an input first");
    h->dets_valid = false;
    HIPCHK(h, hipSetDevice(h->dev));
    int rc = wait_input(h);
    if (rc) return rc;
    size_t p3 = h->ops.size();
    for (size_t i = 0; i < h->ops.size(); ++i) if (h->ops[i].name == "p3") { p3 = i; break; }
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    for (int r = 0; r < reps; ++r)
        for (size_t i = 0; i < h->ops.size(); ++i) {
            const bool second = i >= p3 || h->ops[i].side;   // p3, the FPN's P4..P7 convolutions, the head, the protonet
            if (second != (phase == 1)) continue;
            if ((rc = launch_op(h, h->ops[i], h->cur_n, false))) return rc;
        }
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev1));
    float ms = 0.0f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    if (ms_total) *ms_total = ms;
    return YH_OK;
}

int yh_debug_setup_audit(int64_t out[4]) {
    if (!out) return YH_EINVAL;
    yh::SetupAudit& a = yh::setup_audit();
    out[0] = a.setups.load(); out[1] = a.worker_jobs.load(); out[2] = a.overlaps.load(); out[3] = (int64_t)a.setup_active.load() + a.worker_active.load();
    return YH_OK;
}

int yh_debug_last_conv_launches(const yh_engine* h) { return h ? h->last_conv_launches : 0; }
int yh_debug_last_conv_forms(const yh_engine* h, int32_t* pairs, int32_t cap) {
    if (!h) return 0;
    const int n = (int)(h->last_conv_forms.size() / 2);
    for (int i = 0; pairs && i < n && i < cap; ++i) { pairs[2 * i] = h->last_conv_forms[2 * i]; pairs[2 * i + 1] = h->last_conv_forms[2 * i + 1]; }
    return n;
}

// Is `name` the output of a conv whose 1x1 tail ran in its epilogue at the current batch size (the tensor was not written)?
static bool absorbed_output(yh_engine* h, const char* name) {
    if (h->cur_n < 1) return false;
    for (const Op& o : h->ops) {
        if (o.kind == OP_CONV && o.tail_op >= 0 && o.name == name) return conv_absorbed(h, h->ops[o.tail_op], h->cur_n);
        if (o.kind == OP_CONV && o.chain_c >= 0 && o.name == name) return chain_active(h, o, h->cur_n);   // b stays in LDS
    }
    return false;
}

// One body for both readers. one: the single frame `frame` (dims[0] = 1); otherwise every frame of the last step.
static int read_tensor(yh_engine* h, const char* name, bool one, int32_t frame, float* dst, size_t nfloats, int32_t dims[4]) {
    if (!h || !name || !dims) return YH_EINVAL;
    if ((h->fused_away.count(name) && !h->cfg.debug_tensors) || absorbed_output(h, name))
        return h->fail(YH_ESTATE, std::string("the ") + name + " tensor is fused away; create the engine with debug_tensors = 1 to materialise it");
    auto it = h->named.find(name);
    if (it == h->named.end()) return h->fail(YH_EINVAL, std::string("unknown tensor ") + name);
    if (h->cur_n < 1) return h->fail(YH_ESTATE, "no inference has run");
    if (one && (frame < 0 || frame >= h->cur_n)) return h->fail(YH_EINVAL, "frame out of range");
    const Buf& b = it->second;
    const int first = one ? frame : 0, n = one ? 1 : h->cur_n;
    const size_t per = (size_t)b.h * b.w * b.c;
    dims[0] = n; dims[1] = b.h; dims[2] = b.w; dims[3] = b.c;
    if (!dst) return YH_OK;
    if (nfloats < per * n) return h->fail(YH_EINVAL, "destination too small");
    HIPCHK(h, hipSetDevice(h->dev));
    int rc = ensure_out_f32(h, per * n);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        hipError_t e;
        if (h->fp8_active && h->q_only.count(name))   // fp8 precision: this tensor exists only as E4M3 codes
            e = launch_dequant_e4m3_f32(b.q + (long long)(first + i) * b.img_stride, h->out_f32 + (size_t)i * per, (long long)per, h->act[b.sid].sc_dev, b.c, h->stream);
        else e = launch_f16_to_f32(b.d + (long long)(first + i) * b.img_stride, h->out_f32 + (size_t)i * per, (long long)per, h->stream);
        if (e != hipSuccess) return h->fail(YH_EHIP, "debug read convert");
    }
    HIPCHK(h, hipMemcpyAsync(dst, h->out_f32, per * n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return YH_OK;
}

int yh_debug_read_tensor(yh_engine* h, const char* name, float* dst, size_t nfloats, int32_t dims[4]) {
    return read_tensor(h, name, false, 0, dst, nfloats, dims);
}
int yh_debug_read_tensor_frame(yh_engine* h, const char* name, int32_t frame, float* dst, size_t nfloats, int32_t dims[4]) {
    return read_tensor(h, name, true, frame, dst, nfloats, dims);
}

// The raw codes of the named tensor's E4M3 twin (one frame), as the last step wrote them: no decoding in between.
int yh_debug_read_tensor_e4m3(yh_engine* h, const char* name, int32_t frame, uint8_t* dst, size_t n, int32_t dims[4]) {
    if (!h || !name || !dims) return YH_EINVAL;
    auto it = h->named.find(name);
    if (it == h->named.end()) return h->fail(YH_EINVAL, std::string("unknown tensor ") + name);
    if (h->cfg.precision != YH_PRECISION_FP8 || !h->fp8_active) return h->fail(YH_ESTATE, std::string("no E4M3 form of ") + name + ": the handle does not run its fp8 forward (precision, scales)");
    if (h->cur_n < 1) return h->fail(YH_ESTATE, "no inference has run");
    if (frame < 0 || frame >= h->cur_n) return h->fail(YH_EINVAL, "frame out of range");
    const Buf& b = it->second;
    if (absorbed_output(h, name) || !fp8_writes_codes(h, b)) return h->fail(YH_ESTATE, std::string("the plan writes no E4M3 form of ") + name);
    const size_t per = (size_t)b.h * b.w * b.c;
    dims[0] = 1; dims[1] = b.h; dims[2] = b.w; dims[3] = b.c;
    if (!dst) return YH_OK;
    if (n < per) return h->fail(YH_EINVAL, "destination too small");
    HIPCHK(h, hipSetDevice(h->dev));
    HIPCHK(h, hipMemcpyAsync(dst, b.q + (long long)frame * b.img_stride, per, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return YH_OK;
}

// ---- audit hooks (profiles/r03_fault_audit.md): where every buffer of a handle lives, and what a captured step consists of ----
// One line per allocation: kind, name (layer tensors by their DESIGN.md names), [base, end), size and the offsets of base and
// end inside their 2 MiB page - the three GPU memory-access faults of round 2 all hit an address 8 KiB below a 2 MiB boundary.
int yh_debug_alloc_map(yh_engine* h, char* out, size_t cap) {
    if (!h || !out || cap < 2) return YH_EINVAL;
    std::string t;
    char ln[320];
    auto line = [&](const char* kind, const std::string& name, const void* base, size_t bytes) {
        const unsigned long long b = (unsigned long long)(uintptr_t)base, e = b + bytes;
        snprintf(ln, sizeof ln, "%-7s %-14s base 0x%012llx end 0x%012llx bytes %12zu  base%%2MiB 0x%06llx  end%%2MiB 0x%06llx\n", kind, name.c_str(), b, e, bytes,
                 b & 0x1FFFFFull, e & 0x1FFFFFull);
        t += ln;
    };
    std::map<const void*, std::string> names;
    for (const auto& kv : h->named) if (!names.count(kv.second.d)) names[kv.second.d] = kv.first;
    for (const auto& kv : h->named) if (kv.second.q && !names.count(kv.second.q)) names[kv.second.q] = kv.first + ".e4m3";
    names[h->in_buf[0]] = "in_u8[0]"; names[h->in_buf[1]] = "in_u8[1]"; names[h->splitk_ws] = "splitk_ws"; names[h->splitk_ws_side] = "splitk_ws_side";
    names[h->blob_dev] = "weight_blob"; names[h->side_word] = "side_word"; names[h->priors_dev] = "priors";
    names[h->det.cls_count] = "det.cls_count"; names[h->det.cand] = "det.cand"; names[h->det.surv_score] = "det.surv_score"; names[h->det.surv_prior] = "det.surv_prior";
    names[h->det.surv_box] = "det.surv_box"; names[h->det.det_count] = "det.det_count"; names[h->det.dets] = "det.dets"; names[h->det.det_crop] = "det.det_crop"; names[h->det.masks] = "det.masks";
    for (size_t i = 0; i < h->panels.size(); ++i) {
        const Panel& p = h->panels[i];
        const std::string nm = "panel" + std::to_string(i);
        names[p.w] = nm + ".w"; names[p.bias] = nm + ".bias";
        if (p.w8) names[p.w8] = nm + ".w8";
        if (p.scale) names[p.scale] = nm + ".scale";
        if (p.rs_table) names[p.rs_table] = nm + ".rs";
    }
    for (size_t i = 0; i < h->allocs.size(); ++i) {
        auto it = names.find(h->allocs[i].p);
        line("device", it != names.end() ? it->second : "alloc" + std::to_string(i), h->allocs[i].p, h->allocs[i].bytes);
    }
    if (h->out_f32) line("device", "out_f32", h->out_f32, h->out_f32_cap * 4);
    if (h->frame_dev) line("device", "frame_dev", h->frame_dev, h->frame_cap);
    if (h->rs_tmp) line("device", "rs_tmp", h->rs_tmp, h->rs_tmp_cap);
    for (int k = 0; k < 2; ++k) if (h->stage[k]) line("pinned", "stage" + std::to_string(k), h->stage[k], yh_engine::kStageBytes);
    snprintf(out, cap, "%s", t.c_str());
    return (int)t.size() < (int)cap ? YH_OK : YH_EOVERFLOW;
}

// The step for the current batch size, captured (not instantiated) under the handle's current tuning: one line per graph
// node - kernel symbol, grid, block, and for the single-struct kernels of this library the pointers and sizes in the launch
// argument - plus node / edge / root counts. Two captures (with and without the forks) can then be diffed as text.
int yh_debug_graph_nodes(yh_engine* h, int32_t with_tail, char* out, size_t cap) {
    if (!h || !out || cap < 2) return YH_EINVAL;
    if (!h->weights_loaded || h->cur_n < 1) return h->fail(YH_ESTATE, "weights and input must be set");
    HIPCHK(h, hipSetDevice(h->dev));
    int rc = wait_input(h);
    if (rc) return rc;
    hipGraph_t g = nullptr;
    HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed));
    h->capturing = true;
    rc = enqueue_all(h, h->cur_n, with_tail);
    h->capturing = false;
    const hipError_t ce = hipStreamEndCapture(h->stream, &g);
    if (rc) { if (g) hipGraphDestroy(g); return rc; }
    if (ce != hipSuccess || !g) return h->fail(YH_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
    size_t nn = 0, ne = 0, nr = 0;
    hipGraphGetNodes(g, nullptr, &nn);
    hipGraphGetEdges(g, nullptr, nullptr, &ne);
    hipGraphGetRootNodes(g, nullptr, &nr);
    std::vector<hipGraphNode_t> nodes(nn);
    if (nn) hipGraphGetNodes(g, nodes.data(), &nn);
    std::string t;
    char ln[640];
    snprintf(ln, sizeof ln, "# nodes %zu edges %zu roots %zu (batch %d, with_tail %d)\n", nn, ne, nr, h->cur_n, with_tail);
    t += ln;
    std::vector<std::string> lines;
    for (hipGraphNode_t nd : nodes) {
        hipGraphNodeType ty;
        if (hipGraphNodeGetType(nd, &ty) != hipSuccess) continue;
        if (ty == hipGraphNodeTypeKernel) {
            hipKernelNodeParams kp;
            memset(&kp, 0, sizeof kp);
            if (hipGraphKernelNodeGetParams(nd, &kp) != hipSuccess) { lines.push_back("kernel ?"); continue; }
            const char* nm = hipKernelNameRefByPtr(kp.func, h->stream);
            std::string name = nm ? nm : "?";
            std::string args;
            if (kp.kernelParams && kp.kernelParams[0]) {
                if (name.find("conv_igemm_f16") != std::string::npos || name.find("splitk_reduce_f16") != std::string::npos) {
                    const ConvParams* q = (const ConvParams*)kp.kernelParams[0];
                    snprintf(ln, sizeof ln, " x %p w %p bias %p res %p y %p y8 %p x2 %p w2 %p y2 %p scale %p partial %s M %d C %d ksteps %d k_slices %d m_tile0 %d ch_tile0 %d n_ch_tiles %d x_bytes %u w_bytes %u",
                             (const void*)q->x, (const void*)q->w, (const void*)q->bias, (const void*)q->res, (void*)q->y, (void*)q->y8, (const void*)q->x2, (const void*)q->w2, (void*)q->y2,
                             (const void*)q->scale, !q->partial ? "-" : (q->partial == h->splitk_ws ? "ws_main" : (q->partial == h->splitk_ws_side ? "ws_side" : "?")), q->M, q->C, q->ksteps, q->k_slices,
                             q->m_tile0, q->ch_tile0, q->n_ch_tiles, q->x_bytes, q->w_bytes);
                    args = ln;
                } else if (name.find("det_") != std::string::npos) {
                    const DetectParams* q = (const DetectParams*)kp.kernelParams[0];
                    snprintf(ln, sizeof ln, " heads %p proto %p cand %p dets %p masks %p n %d", (const void*)q->heads, (const void*)q->proto, (void*)q->cand, (void*)q->dets, (void*)q->masks, q->n);
                    args = ln;
                } else if (name.find("stem_pool_f16") != std::string::npos) {
                    const StemPoolParams* q = (const StemPoolParams*)kp.kernelParams[0];
                    snprintf(ln, sizeof ln, " x %p rgb %s w %p pool %p n %d", (const void*)q->x, q->rgb == h->in_buf[0] ? "in_u8[0]" : (q->rgb == h->in_buf[1] ? "in_u8[1]" : (q->rgb ? "?" : "-")), (const void*)q->w, (void*)q->pool, q->n);
                    args = ln;
                }
            }
            snprintf(ln, sizeof ln, "kernel grid %u,%u,%u block %u shmem %u %s", kp.gridDim.x, kp.gridDim.y, kp.gridDim.z, kp.blockDim.x, kp.sharedMemBytes, name.c_str());
            lines.push_back(std::string(ln) + args);
        } else if (ty == hipGraphNodeTypeMemset) {
            hipMemsetParams mp;
            memset(&mp, 0, sizeof mp);
            hipGraphMemsetNodeGetParams(nd, &mp);
            snprintf(ln, sizeof ln, "memset dst %s width %zu height %zu elem %u value %u", mp.dst == (void*)h->side_word ? "side_word" : (mp.dst == (void*)h->det.cls_count ? "det.cls_count" : "?"),
                     mp.width, mp.height, mp.elementSize, mp.value);
            lines.push_back(ln);
        } else {
            snprintf(ln, sizeof ln, "node type %d", (int)ty);
            lines.push_back(ln);
        }
    }
    hipGraphDestroy(g);
    std::sort(lines.begin(), lines.end());   // (node order of a multi-branch graph is not a property of the step)
    for (const std::string& l : lines) t += l + "\n";
    snprintf(out, cap, "%s", t.c_str());
    return t.size() < cap ? YH_OK : YH_EOVERFLOW;
}

// ---- measurement hooks -------------------------------------------------------------------------
// One profile entry per KERNEL launch (so that the averages agree with rocprofv3's per-kernel stats):
// a conv op planned as two launches (wave-quantisation tail, channel split, split-K + reduce) gives
// two entries, its algorithmic FLOPs and bytes shared out by the rows / channels each launch covers.
// The entries follow plan_op: a SKIP op has none (it is accounted with the launch that computes it), a CONV op one per
// plan_conv launch, every other op one (launched through launch_op).
struct ProfEntry { int op; int stage; OpLaunch::Form form; int tile_m; KLaunch k; };

static int build_profile_entries(yh_engine* h, int n, int with_tail, std::vector<ProfEntry>* out) {
    out->clear();
    for (int i = 0; i < (int)h->ops.size(); ++i) {
        OpLaunch pl;
        const int rc = plan_op(h, h->ops[i], n, &pl);
        if (rc) return rc;
        KLaunch k[3] = {};
        const int nk = pl.form == OpLaunch::CONV ? plan_conv(h->tune, pl.p, pl.tile, h->panels[h->ops[i].panel].coutPad, k)
                                                  : (pl.form == OpLaunch::SKIP ? 0 : 1);
        for (int j = 0; j < nk; ++j) out->push_back(ProfEntry{ i, -1, pl.form, pl.tile_m, k[j] });
    }
    if (with_tail)
        for (int st = 0; st < detect_launch_count(); ++st) out->push_back(ProfEntry{ -1, st, OpLaunch::OTHER, 0, KLaunch{} });
    return YH_OK;
}

int yh_profile_launch_count(const yh_engine* h, int32_t with_tail) {
    if (!h) return YH_EINVAL;
    std::vector<ProfEntry> ent;
    yh_engine* hm = const_cast<yh_engine*>(h);
    if (build_profile_entries(hm, h->cur_n >= 1 ? h->cur_n : h->cfg.max_batch, with_tail, &ent)) return YH_EINVAL;
    return (int)ent.size();
}

int yh_profile_run(yh_engine* h, int32_t with_tail, int32_t reps, float* ms, double* flops, double* bytes, const char** names) {
    if (!h || !ms || reps < 1) return YH_EINVAL;
    if (!h->weights_loaded || h->cur_n < 1) return h->fail(YH_ESTATE, "weights and input must be set");
    h->dets_valid = false;
    HIPCHK(h, hipSetDevice(h->dev));
    const int n = h->cur_n;
    std::vector<ProfEntry> ent;
    int rc = wait_input(h);
    if (rc) return rc;
    rc = build_profile_entries(h, n, with_tail, &ent);
    if (rc) return rc;
    const int nl = (int)ent.size();
    std::vector<hipEvent_t> ev((size_t)nl * 2);
    for (auto& e : ev) HIPCHK(h, hipEventCreate(&e));
    std::vector<double> acc(nl, 0.0);
    h->det.n = n;
    for (int r = 0; r < reps && rc == YH_OK; ++r) {
        for (int i = 0; i < nl && rc == YH_OK; ++i) {
            const ProfEntry& pe = ent[i];
            hipEventRecord(ev[2 * i], h->stream);
            if (pe.form == OpLaunch::CONV) { if (launch_k(pe.k, h->stream) != hipSuccess) rc = h->fail(YH_EHIP, "conv launch failed in profile run"); }
            else if (pe.op >= 0) rc = launch_op(h, h->ops[pe.op], n);
            else if (launch_detect_stage(h->det, pe.stage, h->stream) != hipSuccess) rc = h->fail(YH_EHIP, "detect stage launch failed");
            hipEventRecord(ev[2 * i + 1], h->stream);
        }
        if (rc) break;
        if (hipStreamSynchronize(h->stream) != hipSuccess) { rc = h->fail(YH_EHIP, "sync failed in profile run"); break; }
        for (int i = 0; i < nl; ++i) { float t = 0; hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]); acc[i] += t; }
    }
    for (auto& e : ev) hipEventDestroy(e);
    if (rc) {   // a pass that stopped between the tail's K1 and K2 leaves candidate counts behind: clear them as run()'s error path does
        hipStreamSynchronize(h->stream); hipStreamSynchronize(h->side);
        hipMemset(h->det.cls_count, 0, sizeof(int) * (size_t)h->cfg.max_batch * (h->C - 1));
        return rc;
    }
    h->prof_labels.assign(nl, std::string());
    for (int i = 0; i < nl; ++i) {
        const ProfEntry& pe = ent[i];
        ms[i] = (float)(acc[i] / reps);
        double fl = 0.0, by = 0.0;
        if (pe.op >= 0) {
            const Op& o = h->ops[pe.op];
            const double frac = pe.form == OpLaunch::CONV ? pe.k.frac : 1.0;
            fl = o.flops_per_img * n * frac;
            by = (o.bytes_per_img * n + o.bytes_fixed) * frac;
            if (pe.form == OpLaunch::CONV && pe.k.reduce) {
                h->prof_labels[i] = "splitk_reduce_f16:" + o.name;
                by = (double)pe.k.p.M * pe.k.p.partial_ld * 4.0 * pe.k.p.k_slices + (double)pe.k.p.M * pe.k.p.cout8 * 2.0;
            } else if (pe.form == OpLaunch::CONV) {
                h->prof_labels[i] = conv_label(pe.k.p, pe.k.tile) + ":" + o.name + pe.k.what;
                if (pe.k.p.w2) {   // fused 1x1 tail: both convolutions' FLOPs; this conv's input and the tail's output
                    const Op& t = h->ops[o.tail_op];
                    h->prof_labels[i] += "+" + t.name;
                    fl += t.flops_per_img * n;
                    by += t.bytes_fixed + 2.0 * n * ((double)t.P * t.Q * h->panels[t.panel].cout - (double)o.P * o.Q * h->panels[o.panel].cout * (h->fp8_active && !o.write_f16 ? 0.0 : 1.0));
                }
            } else if (pe.form == OpLaunch::XN) {
                // expand conv + next reduce conv: both convolutions' FLOPs; HBM bytes = b + residual in, y + a' out, the weights
                const Op& oa = h->ops[o.xn_a];
                const double px = (double)n * o.P * o.Q;
                h->prof_labels[i] = std::string(bneck_symbol(256, pe.tile_m, true, false)) + ":" + o.name + "+" + oa.name;
                fl += oa.flops_per_img * n;
                by = 2.0 * px * (256.0 + 1024.0 + 1024.0) + px * 256.0 * ((oa.write_f16 || !h->fp8_active ? 2.0 : 0.0) + (h->fp8_active && oa.write_q ? 1.0 : 0.0)) + o.bytes_fixed + oa.bytes_fixed;
            } else if (pe.form == OpLaunch::CHAIN) {
                // a bottleneck chain: the FLOPs of its two or three convolutions; HBM bytes = a + residual in, y (+ a') out, the weights
                const Op& oc = h->ops[o.chain_c];
                const int planes = h->panels[o.panel].cout;
                const double px = (double)n * o.P * o.Q;
                h->prof_labels[i] = std::string(bneck_symbol(planes, pe.tile_m, o.chain_a >= 0, oc.dual)) + ":" + o.name + "+" + oc.name;
                fl += oc.flops_per_img * n;
                by = 2.0 * ((double)n * o.in.h * o.in.w * planes + px * 4.0 * planes * (oc.dual ? 1.0 : 2.0) + (oc.dual ? px * oc.in2.c : 0.0)) + o.bytes_fixed + oc.bytes_fixed;
                if (o.chain_a >= 0) {
                    const Op& oa = h->ops[o.chain_a];
                    h->prof_labels[i] += "+" + oa.name;
                    fl += oa.flops_per_img * n;
                    by += 2.0 * px * planes + oa.bytes_fixed;
                }
            } else h->prof_labels[i] = o.label;
        } else h->prof_labels[i] = detect_stage_name(pe.stage);
        if (flops) flops[i] = fl;
        if (bytes) bytes[i] = by;
        if (names) names[i] = h->prof_labels[i].c_str();
    }
    return YH_OK;
}

// ---- activation guards (Bounds): a step of n < max_batch frames must leave images n .. max_batch - 1 of every
// activation allocation, and the 256 zero bytes behind each, as they were. Memsets and copies only: nothing is launched.
static size_t next_changed(const uint8_t* b, size_t i, size_t end, uint8_t want) {   // the first index in [i, end) whose byte is not `want`, or end
    const uint64_t pat = want ? ~0ull : 0ull;
    for (uint64_t w; i + 8 <= end; i += 8) { memcpy(&w, b + i, 8); if (w != pat) break; }
    while (i < end && b[i] == want) ++i;
    return i;
}

static int act_guard_args(yh_engine* h, int32_t first_image) {
    if (!h->weights_loaded) return h->fail(YH_ESTATE, "activation guards: load the weights first");
    if (first_image < 1 || first_image >= h->cfg.max_batch) return h->fail(YH_EINVAL, "activation guards: first_image outside 1 .. max_batch - 1");
    HIPCHK(h, hipSetDevice(h->dev));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->side));
    return YH_OK;
}

int yh_debug_act_paint(yh_engine* h, int32_t first_image) {
    if (!h) return YH_EINVAL;
    if (const int rc = act_guard_args(h, first_image)) return rc;
    for (const ActAlloc& a : h->act) {
        const size_t from = (size_t)first_image * a.img * 2;
        HIPCHK(h, hipMemsetAsync((char*)a.base + from, 0xFF, a.bytes - from, h->stream));
        if (a.q) HIPCHK(h, hipMemsetAsync(a.q + from / 2, 0xFF, (a.bytes - from) / 2, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return YH_OK;
}

int yh_debug_act_check(yh_engine* h, int32_t first_image, char* out, size_t cap) {
    if (!h) return YH_EINVAL;
    if (out && cap) out[0] = 0;
    if (const int rc = act_guard_args(h, first_image)) return rc;
    std::vector<uint8_t> host;
    std::string text;
    int hits = 0;
    // one region of one allocation: [from, data) must be 0xFF, [data, data + 256) zero; es = bytes per element
    auto scan = [&](const std::string& name, const uint8_t* dev, size_t from, size_t data, const ActAlloc& a, size_t es) -> hipError_t {
        host.resize(data + 256 - from);
        const hipError_t e = hipMemcpy(host.data(), dev + from, host.size(), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        const size_t img = (size_t)a.img * es, row = (size_t)a.c * es;
        for (int trailer = 0; trailer < 2; ++trailer) {
            const size_t end = trailer ? host.size() : data - from;
            const uint8_t want = trailer ? 0x00 : 0xFF;
            for (size_t i = next_changed(host.data(), trailer ? data - from : 0, end, want); i < end && hits < 9; i = next_changed(host.data(), i + 1, end, want)) {
                const size_t off = from + i;
                char ln[256];
                if (!trailer)
                    snprintf(ln, sizeof ln, "%s: image %zu row %zu byte %zu is 0x%02X, painted 0xFF\n", name.c_str(), off / img, (off % img) / row, off % img, host[i]);
                else
                    snprintf(ln, sizeof ln, "%s: trailer byte %zu behind image %d is 0x%02X, not 0\n", name.c_str(), off - data, h->cfg.max_batch - 1, host[i]);
                text += ln;
                ++hits;
            }
        }
        return hipSuccess;
    };
    for (const ActAlloc& a : h->act) {
        if (hits >= 9) break;
        HIPCHK(h, scan(a.name, (const uint8_t*)a.base, (size_t)first_image * a.img * 2, a.bytes, a, 2));
        if (a.q && hits < 9) HIPCHK(h, scan(a.name + ".e4m3", a.q, (size_t)first_image * a.img, a.bytes / 2, a, 1));
    }
    if (!hits) return YH_OK;
    if (out && cap) snprintf(out, cap, "%s", text.c_str());
    return h->fail(YH_EOVERFLOW, "activation guards: a step stored outside its " + std::to_string(first_image) + " image(s): " + text.substr(0, text.find('\n')));
}

int yh_time_steps(yh_engine* h, int32_t with_tail, int32_t steps, float* ms_total) {
    if (!h || !ms_total || steps < 1) return YH_EINVAL;
    HIPCHK(h, hipSetDevice(h->dev));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    for (int i = 0; i < steps; ++i) { int rc = run(h, with_tail); if (rc) return rc; }
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev1));
    HIPCHK(h, hipEventElapsedTime(ms_total, h->ev0, h->ev1));
    return YH_OK;
}

}  // extern "C"
