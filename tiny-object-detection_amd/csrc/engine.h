// engine.h - the engine's data model and the functions that cross its translation units (internal, beside yh_internal.h).
// Units: engine.hip (network, planner, step, C ABI), weights.hip (YHW1 blob), fp8.hip, rccl.hip, engine_probe.hip
// (yh_debug_* / yh_profile_*), engine_ops.hip (yh_op_*), instance.hip, instance_batch.hip, instance_track.hip and
// instance_track_batch.hip (yh_instance_*), classify_batch.hip (yh_classify_batch_*). DESIGN.md section 4 says what each may see.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>

#include <map>
#include <set>
#include <string>
#include <vector>

#include "classify_geo.h"
#include "instance_host.h"
#include "yh_internal.h"

// (hidden: nothing declared here is exported from the shared library)
namespace yh __attribute__((visibility("hidden"))) {

struct ConvDesc {          // one canonical conv of the blob
    int cout, cin, k;
    float gain;
    int is_conf;   // 0 plain, 1 conf head (background bias), 2 mask head (bias)
    size_t blob_w_off, blob_b_off;  // byte offsets in the canonical blob
};

struct Panel {             // device-side repacked weights of one launched conv
    half_t* w = nullptr;   // [coutPad][Kpad]
    float* bias = nullptr; // [coutPad]
    int2* rs_table = nullptr;
    int cout = 0, coutPad = 0, Kpad = 0, cin_store = 0, k = 0;
    ConvTile tile = TILE_128x128;
    std::vector<int> src;  // canonical conv indices concatenated along cout
    int kcat = -1;         // >= 0: this canonical conv's weights are appended ALONG K (two-source 1x1 form, ConvParams::x2); biases add
    // fp8 precision: the same weights as E4M3 codes, one scale per output channel
    bool fp8 = false;
    uint8_t* w8 = nullptr;     // [coutPad][Kpad] E4M3
    float* scale = nullptr;    // [coutPad]: s_x (input tensor) * s_w[ch], refreshed by the calibration
    std::vector<float> sw;     // [coutPad] weight scales (host)
    int in_sid = -1;           // scale id of the input tensor these weights are applied to
};

struct Buf {               // dense NHWC f16 tensor [max_batch][h][w][c] or a slice of one
    half_t* d = nullptr;
    int h = 0, w = 0, c = 0;       // c = row stride in elements
    long long img_stride = 0;      // elements per image
    half_t* zero = nullptr;        // 16-byte zero block at the end of the owning allocation
    // fp8 precision: the same tensor as E4M3 codes (same element offsets, one byte each), the allocation's scale id
    uint8_t* q = nullptr;
    uint8_t* qzero = nullptr;
    int sid = -1;
};

struct DevAlloc { void* p; size_t bytes; };   // one hipMalloc of a handle

// One tracker of the handle's bank (instance_track.hip): stream 0 is yh_instance_track's, the others are reached through
// yh_instance_track_batch only. Device buffers are allocated at the stream's first use and freed by yh_destroy.
struct TrkStream {
    uint4* img = nullptr;           // T [hp * wp]: bit s = slot s's last seen mask is on there
    int32_t* state = nullptr;       // slots [128][4] = (class or 0, id, age, area), rank of slot, slot of rank, keep [4]
    size_t img_cap = 0;
    int hp = 0, wp = 0;             // the prototype size T was built at
    bool live = false;              // false: the next tracked call starts from an empty tracker
    std::vector<int32_t> table;     // [rows][6] = (slot, class, id, age, area, rank or -1) after the stream's last tracked frame
    int rows = -1;                  // -1: no tracked call on this stream yet
};
constexpr int kTrkStreams = 64;     // YH_TRACK_STREAMS_MAX

// One activation allocation (new_buf), indexed by Buf::sid: where it lies and, in fp8 handles, its scales.
// Round 4: one activation scale per CHANNEL of every allocation an fp8 convolution reads (a per-tensor scale is the same value in
// every channel). The channel scale is folded into the consumer's weights along K before their per-output-channel quantisation
// (refresh_fp8_scales) and the producer's epilogue multiplies by the reciprocal table instead of a scalar: no extra pass.
struct ActAlloc {
    std::string name;              // new_buf's name (the layer's): what yh_debug_act_check reports
    half_t* base = nullptr;        // first element
    size_t bytes = 0;              // max_batch images; 256 bytes of zeros (the zero pixel first) follow them
    uint8_t* q = nullptr;          // fp8 handles: the E4M3 twin, bytes / 2 and its own 256 zeros
    long long img = 0;             // elements per image
    int c = 0;                     // channels (= row stride in elements)
    float scale = 1.0f;            // the largest channel scale (what yh_fp8_layer_info reports)
    bool scale_set = false;        // the scale was set by a calibration or by yh_fp8_set_layer_scale since the weights were loaded
    std::vector<float> ch;         // [c] channel scales; empty: not set
    float *inv_dev = nullptr, *sc_dev = nullptr;   // device tables of 1 / scale and scale ([c]; fp8 handles only)
};

enum OpKind { OP_PRE, OP_CONV, OP_POOL, OP_BILINEAR, OP_STEMPOOL };

struct Op {
    OpKind kind;
    std::string name;      // layer name (matches the oracle's intermediate names)
    std::string label;     // "kernel_symbol:layer"
    Buf in, out, res;
    bool has_res = false;
    bool res_up = false;   // the residual is the bilinear resize of the lower-resolution tensor `res` (ConvParams::res_up)
    int tail_op = -1;      // index of the 1x1 conv that may run in this conv's epilogue (ConvParams::w2) when the launch plan allows
    // bottleneck chain (bneck.hip; tune.chain): on an identity block's 3x3 conv - the block's last 1x1 conv and (if any) the next
    // block's first 1x1 conv that run inside its launch; on those two - the 3x3 conv that absorbs them
    int chain_c = -1, chain_a = -1, in_chain = -1;
    // ... the no-3x3 form (256 planes, layer 3): on the block's last 1x1 conv - the next block's first 1x1 conv that runs inside its
    // launch; on that one - the conv that absorbs it
    int xn_a = -1, in_xn = -1;
    int fused_into = -1;   // ... and on that 1x1 conv: the index of the conv that may absorb it
    bool side = false;     // may run on the second stream: nothing on the main stream reads its output before the step's join
    bool dual = false;     // two-source 1x1 form: K continues over `in2` read at `stride2` (ConvParams::x2)
    Buf in2;
    int stride2 = 1;
    int panel = -1;
    int stride = 1, pad = 0, act = 0, tanh_from = INT_MAX;
    int P = 0, Q = 0;      // output spatial
    int nlev = 0, lev_start[5] = {0, 0, 0, 0, 0}, lev_h[5] = {0, 0, 0, 0, 0}, lev_w[5] = {0, 0, 0, 0, 0};   // multi-level input (ConvParams)
    double flops_per_img = 0, bytes_per_img = 0, bytes_fixed = 0;
    // fp8 precision: this conv reads E4M3 operands; what its output is written as (decided by who reads it)
    bool fp8 = false, write_q = false, write_f16 = true;
};

// The handle's tuning with every default resolved (include/yolact_hip_debug.h: yh_tuning; -1 = default there).
struct Tune {
    int plan_cus, chsplit, upfuse, ablate, op_tile, op_kslices, tailfork, dsfuse, headfork_maxb, protofuse, chain, op_xgap, op_tanh_from;
};

// A convolution is planned as one to two kernel launches; `frac` is the share of the op's
// algorithmic work a launch does (profile attribution), `what` a label suffix.
struct KLaunch { bool reduce; ConvParams p; ConvTile tile; double frac; const char* what; };

// What op `o` becomes at batch n. Decided here only: launch_op issues the plan, the profiler lists and labels the same plan.
struct OpLaunch {
    enum Form { SKIP, XN, CHAIN, CONV, OTHER } form;   // SKIP: computed inside another op's launch; OTHER: not a convolution
    int planes, tile_m;                                // XN, CHAIN: launch_bneck's arguments besides bp
    BneckParams bp;
    ConvParams p;                                      // CONV: plan_conv's arguments besides the panel's coutPad
    ConvTile tile;
};

}  // namespace yh

struct yh_engine {
    yh_config cfg;
    yh::Tune tune;
    int dev = 0, device_cus = 256;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;   // the detection tail's K1-K3 run here underneath the protonet
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_forks[4] = { nullptr, nullptr, nullptr, nullptr };   // one per fork point of a step (enqueue_all)
    std::string err;

    int S = 0, C = 0, ldh = 0;
    int lvl[5] = { 0, 0, 0, 0, 0 }, lvl_off[5] = { 0, 0, 0, 0, 0 };
    int cells = 0, P = 0, hp = 0, wp = 0;
    double flops_per_frame = 0;

    std::vector<yh::ConvDesc> convs;
    size_t blob_bytes = 0;
    std::vector<yh::Panel> panels;
    std::vector<yh::Op> ops;
    std::vector<yh::DevAlloc> allocs;   // everything dev_alloc handed out (freed by yh_destroy; listed by yh_debug_alloc_map)
    std::map<std::string, yh::Buf> named;
    std::set<std::string> fused_away;   // named tensors that production runs never write (debug_tensors = 1 materialises them)
    // fp8 precision (yh_config.precision): per-allocation activation scales, filled by yh_fp8_calibrate
    std::vector<yh::ActAlloc> act;      // by Buf::sid
    std::vector<int> fp8_ops;           // indices of the ops that read E4M3 operands
    std::set<std::string> q_only;       // named tensors that exist only as E4M3 while fp8 is active
    bool fp8_active = false;            // the op list currently runs its fp8 form (false during calibration and in f16 engines)
    bool fp8_ready = false;             // every E4M3 layer's input tensor has its scales (no E4M3 layer in the plan: once the weights are loaded)
    unsigned* absmax_dev = nullptr;     // calibration scratch: kMaxFp8Tensors x kMaxFp8Channels channel maxima (as bit patterns)
    static constexpr int kMaxFp8Tensors = 64, kMaxFp8Channels = 512;
    unsigned* rowmax_dev = nullptr;           // [1024]: row maxima of a weight panel with the channel scales folded in

    // Two input buffers and a copy stream: yh_set_input_* fills the buffer the running step does NOT read, so frame k+1's
    // host -> device copy runs underneath step k (the limiter of the sharded path is host-side H2D). A step is
    // captured once per buffer (the stem kernel's source pointer is a launch argument).
    uint8_t* in_buf[2] = { nullptr, nullptr };
    int in_cur = 0;                 // the buffer the next step reads
    bool in_pending = false;        // a copy into in_buf[in_cur] has been issued that no step has waited for yet
    hipStream_t copy = nullptr;
    hipEvent_t in_ready[2] = { nullptr, nullptr }, in_free[2] = { nullptr, nullptr };
    bool in_free_rec[2] = { false, false };
    uint8_t* in_u8() const { return in_buf[in_cur]; }
    int in_hp = 0;
    yh::Buf in_f16, pyr, pyr_t, heads, proto;
    float* priors_dev = nullptr;
    std::vector<float> priors_host;

    // tail workspaces / outputs
    yh::DetectParams det{};
    // compat-path scratch
    uint32_t* frame_dev = nullptr;
    float* rs_tmp = nullptr;
    float* cells_dev = nullptr;
    uint32_t* codes_dev = nullptr;
    uint32_t* stitch_dev = nullptr;
    int* diverged_dev = nullptr;
    size_t frame_cap = 0, rs_tmp_cap = 0;
    // instance frame (instance.hip): allocated at the first yh_instance_frame, grow only
    bool dets_valid = false;        // the handle's last step was a yh_evaluate: det holds that batch's detections
    uint4* inst_bits = nullptr;     // [hp * wp] 128-bit sets at prototype resolution
    uint32_t* inst_frame = nullptr; // [height][width] class << 24 | id << 16
    uint32_t* inst_meta = nullptr;  // [2][128]: packed value per rank (0: not eligible), pixels won per rank
    uint8_t* inst_cmap = nullptr;   // [C - 1] the call's class map
    size_t inst_bits_cap = 0, inst_frame_cap = 0;
    std::vector<uint8_t> inst_cmap_host;
    uint32_t inst_meta_host[256] = {};   // where inst_meta is read back to (a member: the copy is asynchronous)
    std::vector<int32_t> inst_table;   // [inst_rows][4] = (rank, class, id, pixels) of the last instance frame
    int inst_rows = -1;             // -1: no instance frame yet
    // instance batch (instance_batch.hip): its own buffers, allocated at the first yh_instance_batch, grow only
    uint4* instb_bits = nullptr;      // [n][hp * wp]
    uint32_t* instb_frames = nullptr; // [n][height][width]
    uint32_t* instb_meta = nullptr;   // [n][2][128]
    uint8_t* instb_cmap = nullptr;    // [C - 1]
    size_t instb_bits_cap = 0, instb_frames_cap = 0, instb_meta_cap = 0, instb_cmap_cap = 0;
    std::vector<uint8_t> instb_cmap_host;
    std::vector<uint32_t> instb_meta_host;          // [n][2][128] as read back
    std::vector<std::vector<int32_t>> instb_tables; // per frame of the last batch: [rows][4]
    int instb_n = -1;                 // frames of the last batch; -1: no batch
    // classify batch (classify_batch.hip): its own buffers, allocated at the first yh_classify_batch_u32, grow only
    uint32_t* clsb_frames = nullptr;  // [n][height][width]: the frames as uploaded, then as classified
    float* clsb_cells = nullptr;      // [2n][cells][C] output 4 of the step
    uint32_t* clsb_codes = nullptr;   // [2n][cells]
    int* clsb_div = nullptr;          // [2n] divergence flags
    size_t clsb_frames_cap = 0, clsb_cells_cap = 0, clsb_codes_cap = 0, clsb_div_cap = 0;
    yh::ClassifyGeo clsb_geo;         // the four resize tables of the last geometry (W, H, S) and the pre kernel's plan (classify_geo.h)
    int clsb_n = -1;                  // frames of the last batch; -1: no batch
    // instance tracks (instance_track.hip): the bank of trackers, stream 0 the one yh_instance_track advances
    yh::TrkStream trk[yh::kTrkStreams];
    uint32_t* trk_ov = nullptr;     // I [128][128] then A [128]: zeroed on the stream by every tracked call
    int32_t trk_host[640] = {};     // where the slots and their ranks are read back to (a member: the copy is asynchronous)
    // instance track batch (instance_track_batch.hip): a tracked batch is an instance batch (instb_*) plus these, grow only
    uint32_t* trkb_ov = nullptr;    // [n][128 * 128 + 128]: I and A of every frame, zeroed on the stream by every tracked batch
    int32_t* trkb_snap = nullptr;   // [n][640]: the slots and their ranks of the frame's stream right after that frame
    void* trkb_desc = nullptr;      // the call's (round, entry) descriptors
    size_t trkb_ov_cap = 0, trkb_snap_cap = 0, trkb_desc_cap = 0;
    std::vector<uint8_t> trkb_desc_host;             // (members: the copies are asynchronous)
    std::vector<int32_t> trkb_snap_host;
    std::vector<std::vector<int32_t>> trkb_tables;  // per frame of the last tracked batch: [rows][6]
    int trkb_n = -1;                // frames of the last batch if it was a tracked one; -1: it was not (or there is none)
    // output staging
    float* out_f32 = nullptr;
    size_t out_f32_cap = 0;
    float* splitk_ws = nullptr;
    static const size_t kSplitKBytes = (size_t)48 << 20;

    bool weights_loaded = false, capturing = false;
    bool worker_mode = false;   // the handle is a group member being driven from its worker thread: no capture, no allocation there
    unsigned* side_word = nullptr;   // target of the captured side-branch memset (enqueue_all)
    uint8_t* blob_dev = nullptr;   // the canonical blob as loaded (send / receive buffer of the RCCL weight broadcast)
    int cur_n = 0;
    static constexpr size_t kStageBytes = 4u << 20;   // pinned staging for small host inputs
    uint8_t* stage[2] = { nullptr, nullptr };
    hipEvent_t stage_ev[2] = { nullptr, nullptr };
    int stage_idx = 0;
    int last_conv_launches = 0;   // yh_debug_last_conv_launches
    std::vector<int> last_conv_forms;   // yh_debug_last_conv_forms: (tile, form) of every kernel the last single-op conv call launched
    bool stem_fused = false;
    int tail_fork_op = 0;   // ops[tail_fork_op..] (the protonet) do not feed the tail's K1-K3
    int head_fork_op = 0;   // ops[head_fork_op .. tail_fork_op) are the shared prediction head; the protonet does not read them
    float* splitk_ws_side = nullptr;   // split-K workspace of convolutions launched on the side stream
    std::map<int, hipGraphExec_t> graphs;  // key = n*2 + with_tail
    std::vector<std::string> prof_labels;  // storage behind the names yh_profile_run returns

    int fail(int code, const std::string& m) { err = m; return code; }
};

#define HIPCHK(h, call)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return (h)->fail(YH_EHIP, std::string(#call) + ": " + hipGetErrorString(e_));      \
    } while (0)

namespace yh __attribute__((visibility("hidden"))) {

// engine.hip
std::string& create_error();   // what yh_last_error(NULL) returns: set by yh_create and by the entry points that take no handle
size_t pad16(size_t v);
int round_up(int v, int m);
int out_dim(int h, int k, int s, int p);
int blocks_of(int backbone, int layer);
int dev_alloc(yh_engine* h, void** p, size_t bytes);
int ensure_out_f32(yh_engine* h, size_t nfloats);
void drop_graphs(yh_engine* h);   // captured steps bake in tuning, scales, streams: whoever changes one of those drops them
int plan_conv(const Tune& tu, const ConvParams& p, ConvTile tile, int coutPad, KLaunch out[3]);
hipError_t launch_k(const KLaunch& k, hipStream_t stream);
// n_launches (the single-op entry points): the plan's launch count and, in forms, the (tile, form) pair of every kernel launched - the
// split-K reduce as (-1, YH_FORM_REDUCE); hipErrorInvalidValue BEFORE the first launch, both left as they were, when launch_conv
// would refuse one of the plan's launches.
hipError_t launch_conv_planned(const Tune& tu, const ConvParams& p, ConvTile tile, int coutPad, hipStream_t stream, int* n_launches = nullptr,
                               std::vector<int>* forms = nullptr);
bool conv_absorbed(yh_engine* h, const Op& o, int n);
bool chain_active(const yh_engine* h, const Op& ob, int n);
int plan_op(yh_engine* h, const Op& o, int n, OpLaunch* out);
int launch_op(yh_engine* h, const Op& o, int n, bool side = false);
int enqueue_all(yh_engine* h, int n, int with_tail);
int wait_input(yh_engine* h);
int run(yh_engine* h, int with_tail);
// weights.hip
void build_conv_table(yh_engine* h);
int alloc_panels(yh_engine* h);
int check_blob(yh_engine* h, const uint8_t* b, size_t nbytes);
int upload_panels(yh_engine* h, const uint8_t* blob);
int ensure_blob(yh_engine* h);
// instance.hip (instance_check, instance_class_map, instance_table and instance_grow_bytes need no handle: instance_host.h)
struct InstTrack { int iou_permille, max_age; };   // a tracked call's parameters (instance_run: nullptr = yh_instance_frame's ids)
int instance_run(yh_engine* h, const uint8_t* masks, const yh_detection* dets, const int* count, int max_n, int hp, int wp,
                 int width, int height, const uint8_t* class_map, float min_score, uint32_t* out_host, const InstTrack* trk = nullptr);
void instance_free(yh_engine* h);
int instance_grow(yh_engine* h, void** p, size_t* cap, size_t bytes);   // instance_grow_bytes, a failure as the handle's YH_ENOMEM
// instance_batch.hip: n frames in one pair of launches; frame b reads masks + b max_n px, dets + b max_n, count + b
struct InstTrackBatch { InstTrack p; const int32_t* streams; };   // a tracked batch: streams [n] or nullptr (all 0); checked by the caller
int instance_batch_run(yh_engine* h, const uint8_t* masks, const yh_detection* dets, const int* count, int max_n, int n, int hp, int wp,
                       int width, int height, const uint8_t* class_map, float min_score, uint32_t* out_host,
                       const InstTrackBatch* trk = nullptr);
void instance_batch_free(yh_engine* h);
// instance_track.hip: the stages instance_run puts between inst_pack and inst_paint, behind the read-back and behind the wait
const char* track_check(int iou_permille, int max_age);   // nullptr: fine
int track_prepare(yh_engine* h, int stream, int hp, int wp);   // the stream's T and state exist; not live or another size: emptied on the stream
int track_enqueue(yh_engine* h, int hp, int wp, const InstTrack& trk);
int track_readback(yh_engine* h);
void track_finish(yh_engine* h);
void track_rows(const int32_t* st, std::vector<int32_t>& table);   // the slots and their ranks as read back -> rows (slot, class, id, age, area, rank)
void track_drop(yh_engine* h, int stream = 0);   // an empty tracker (a tracked call that failed, yh_instance_track_reset)
void track_free(yh_engine* h);
// instance_track_batch.hip: the stages instance_batch_run puts between inst_batch_pack and inst_batch_paint, behind the read-back
// and behind the wait, for n frames each on its stream's tracker
std::string track_batch_check(int n, const int32_t* streams);   // empty: fine
int track_batch_enqueue(yh_engine* h, int n, int hp, int wp, const InstTrackBatch& trk);
int track_batch_readback(yh_engine* h, int n);
void track_batch_finish(yh_engine* h, int n, const InstTrackBatch& trk);
void track_batch_drop(yh_engine* h, int n, const InstTrackBatch& trk);   // empties every tracker the call named
void track_batch_free(yh_engine* h);
// classify_batch.hip
void classify_batch_free(yh_engine* h);
// fp8.hip
void plan_fp8(yh_engine* h);
std::string fp8_missing(const yh_engine* h);
bool fp8_writes_codes(const yh_engine* h, const Buf& b);
int refresh_fp8_scales(yh_engine* h, int sid = -1);

}  // namespace yh
