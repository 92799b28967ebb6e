/*
 * yolact_hip.h — C ABI of the MI355X-native YOLACT inference library (libyolact_hip.so).
 *
 * This is the drop-in boundary for the reference's L2 layer: it stands in for the
 * TFLite interpreter + EdgeTPU delegate that /root/reference/src/yolact.rs drives.  Each entry
 * point names the reference call (file:line, relative to the reference checkout) it replaces.
 * Plain C types only; no exceptions cross the boundary; no global state; every handle owns a
 * private HIP stream and binds its device on every entry, so calls may arrive from different OS
 * threads over time (tokio worker migration, src/main.rs:63-75) but never concurrently per handle.
 *
 * Status convention: every function returning int returns YH_OK (0) on success and a negative
 * YH_E* code otherwise; yh_last_error(h) then holds a human-readable message.  The reference
 * `.expect()`s every failure (src/yolact.rs:20,25,27,29,35,163); the host shim decides to panic.
 */
#ifndef YOLACT_HIP_H
#define YOLACT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YH_ABI_VERSION 4

enum {
    YH_OK = 0,
    YH_EINVAL = -1,     /* bad argument */
    YH_EHIP = -2,       /* HIP runtime error */
    YH_ENOMEM = -3,
    YH_EWEIGHTS = -4,   /* weight blob does not match the architecture */
    YH_ESTATE = -5,     /* call out of order (e.g. invoke before weights) */
    YH_EDIVERGE = -6,   /* strict compat: the reference's flood fill would not terminate here
                           (src/yolact.rs:57-78) */
    YH_EOVERFLOW = -7   /* a bounded device list overflowed (never silently truncated) */
};

/* Backbone depth of the YOLACT architecture. */
enum { YH_BACKBONE_R50 = 50, YH_BACKBONE_R101 = 101 };

/* Output tensor element kinds; mirrors tflite::context::ElementKind as used at src/yolact.rs:171-186. */
enum { YH_KIND_F32 = 1, YH_KIND_U8 = 3, YH_KIND_I8 = 9, YH_KIND_F16 = 10 };   /* (I8: an int8 tensor of a TFLite model; its bytes are read as they are) */

/* Reference-compat behaviour of yh_classify_frame_u32. */
enum {
    YH_COMPAT_STRICT = 0, /* bit-for-bit what src/yolact.rs computes, quirks A8'/A9 included; returns
                             YH_EDIVERGE where the reference would loop forever */
    YH_COMPAT_SANE = 1    /* 4-connected component ids, `|` packing: what the author meant */
};

typedef struct yh_engine yh_engine; /* opaque; replaces struct Yolact<'a> (src/yolact.rs:13-15) */

/* Arithmetic of the K-heavy convolutions. F16: f16 operands everywhere (configs[1]-[3]).
 * FP8: 3x3 convolutions with >= 256 input channels read OCP E4M3 activations (written by the producing layer's
 * epilogue, one calibrated scale per tensor) and E4M3 weights (one scale per output channel) on the block-scaled
 * fp8 MFMA; everything else stays f16 (configs[4]; the reference's own model is quantised end to end,
 * data/README.md:5-10, data/FRC_model_edgetpu.log:7-19). */
enum { YH_PRECISION_F16 = 0, YH_PRECISION_FP8 = 1 };


/* Measurement / test knobs of one handle: 32 ints, every one -1 = the library's default (yh_default_config sets them so). A host leaves
 * them alone; what they are is written down in include/yolact_hip_debug.h, which names the fields of this very struct (same layout) and
 * declares the measurement, study and test entry points - nothing the reference's caller needs ("a lab notebook is not an
 * ABI"). There are no process-global switches: the library reads no environment variable. */
#ifndef YH_TUNING_DEFINED
#define YH_TUNING_DEFINED
typedef struct yh_tuning { int32_t knob[32]; } yh_tuning;
#endif

typedef struct yh_config {
    int32_t abi_version;   /* must be YH_ABI_VERSION */
    int32_t device;        /* HIP device ordinal */
    int32_t backbone;      /* YH_BACKBONE_R50 | YH_BACKBONE_R101 */
    int32_t input_size;    /* square input: 550 (YOLACT-550), 700, 224 (reference tile, yolact.rs:143-144) ... */
    int32_t max_batch;     /* frames per invoke the arena is sized for (1..256) */
    int32_t num_classes;   /* incl. background; 81 (src/yolact.rs:108: chunks(81)) */
    int32_t top_k;         /* per-class candidates kept before Fast-NMS (200) */
    int32_t max_dets;      /* detections kept per frame (100) */
    float conf_thresh;     /* 0.05 */
    float nms_thresh;      /* 0.5 */
    int32_t use_graph;     /* 1: capture the forward in a hipGraph after the first invoke */
    int32_t debug_tensors; /* 1: also materialise tensors that production runs fuse away (the pre-pool
                            * "stem" tensor, the bilinear upsamples) for yh_debug_read_tensor; 0 (default): do not */
    int32_t precision;     /* YH_PRECISION_F16 (default) | YH_PRECISION_FP8 */
    int32_t fp8_f16_layers;/* YH_PRECISION_FP8 only: groups of the K-heavy 3x3 layers that stay f16 (a hybrid: accuracy for speed, DESIGN.md
                            * §10 table): bit 0 the shared head trunk, bit 1 the protonet (proto0..3), bit 2 the FPN's pred / down convs
                            * (p3..p7), bit 3 the backbone (layers 3-4). 0 (default): all 36 of YOLACT-700 R101 run fp8 */
    int32_t fp8_per_tensor;/* YH_PRECISION_FP8 only: 0 (default) yh_fp8_calibrate sets one activation scale per INPUT CHANNEL of every E4M3
                            * tensor (folded into the consuming conv's weights along K, applied by the producer's epilogue as a vector:
                            * no extra pass); 1: one scale per tensor (round 3's scheme) */
    int32_t reserved[4];   /* zero */
    yh_tuning tune;        /* yh_default_config sets every field to -1 */
} yh_config;

/* Mirrors tflite TensorInfo {name, element_kind, dims, params{scale, zero_point}} as read at
 * src/yolact.rs:150 and :170-175. dims are NHWC-ordered, dims[0] = current batch. */
typedef struct yh_tensor_info {
    const char* name;
    int32_t kind;      /* YH_KIND_* */
    int32_t ndims;
    int32_t dims[4];
    float scale;       /* 1.0 for float tensors */
    int32_t zero_point;/* 0 for float tensors */
} yh_tensor_info;

/* One detection of the fused path (absent in the reference, src/yolact.rs:3-5). */
typedef struct yh_detection {
    int32_t class_id;   /* 0..num_classes-2 (foreground index; background removed) */
    int32_t prior;      /* prior index the detection came from */
    float score;
    float box[4];       /* x1,y1,x2,y2 relative to the frame, unclamped */
} yh_detection;

/* ---- life cycle --------------------------------------------------------------------------- */

/* edgetpu::version() (src/scene.rs:62). Static string. */
const char* yh_version(void);

/* Fills *cfg with the YOLACT-550 R50 defaults (every tuning field -1). */
void yh_default_config(yh_config* cfg);

/* FlatBufferModel::build_from_file + InterpreterBuilder::new/build + EdgeTpuContext::open_device +
 * set_num_threads + allocate_tensors (src/yolact.rs:18-35): builds the layer table for cfg,
 * allocates the whole activation arena and a private stream on cfg->device. No weights yet. */
int yh_create(const yh_config* cfg, yh_engine** out);
void yh_destroy(yh_engine* h);
const char* yh_last_error(const yh_engine* h); /* h may be NULL: last create error of this thread */

/* ---- weights ------------------------------------------------------------------------------ */

/* Size in bytes of the canonical weight blob (DESIGN.md §Weight blob) for this architecture. */
size_t yh_weights_nbytes(const yh_engine* h);
/* The canonical blob as loaded, in device memory on the handle's device (NULL before a load): what
 * yh_load_weights_device of another handle on the same device, or the RCCL broadcast below, reads. */
const void* yh_weights_device_ptr(const yh_engine* h);
/* Writes the seeded synthetic blob (He-scaled uniform, BN folded to bias) into host memory. The
 * reference's model file is absent (.MISSING_LARGE_BLOBS:1-2); this is its stand-in. */
int yh_weights_generate(const yh_engine* h, uint64_t seed, void* blob_host, size_t nbytes);
/* Loads a canonical blob from host memory: validates the per-layer header, repacks to the kernels'
 * padded KRSC panels on device. Replaces build_from_file("data/FRC_model_edgetpu.tflite"), yolact.rs:18-20. */
int yh_load_weights_host(yh_engine* h, const void* blob_host, size_t nbytes);
/* Same, blob already in device memory on this handle's device (e.g. the receive buffer of an RCCL
 * broadcast from rank 0 over xGMI: SURVEY.md §8e). */
int yh_load_weights_device(yh_engine* h, const void* blob_dev, size_t nbytes);

/* ---- fp8 precision (yh_config.precision = YH_PRECISION_FP8; BASELINE.json configs[4]) -------------------------
 * The K-heavy 3x3 convolutions read OCP E4M3 operands on the block-scaled fp8 MFMA. Activations: one scale per INPUT
 * CHANNEL of every tensor such a convolution reads (round 4; yh_config.fp8_per_tensor = 1: one per tensor), which must be
 * set before the first invoke - by calibration on representative frames, or layer by layer from stored values. The channel
 * scale s[c] is folded into the consumer's weights along K (t = w * s[c]) before their quantisation with one scale per
 * output channel (s_w = max |t| / 448), so the weights' E4M3 codes are (re)made whenever a tensor's scales are set; the
 * producer's epilogue multiplies by 1 / s[c] - a vector instead of a scalar, no extra pass. */
/* Runs the f16 forward of the frames last set and sets the scales of every fp8 input tensor to
 * max(2 max|x[.., c]|, max|x| / 16) / 448 - twice the channel's own maximum on the calibration frames and never less than a sixteenth of
 * the tensor's: headroom for frames the calibration has not seen (free in a floating-point code; round 5). YH_ESTATE
 * (and no scale changed) if that forward overflowed: a non-finite maximum would make every code of the tensor 0. */
int yh_fp8_calibrate(yh_engine* h);
/* The convolutions that read E4M3 operands, in execution order: layer name (DESIGN.md layer names: "l3b0_b", "p5",
 * "proto0", "head_t" ...) and the LARGEST channel scale of its input tensor (yh_fp8_layer_channel_scales gives them all). */
int yh_fp8_layer_count(const yh_engine* h);
int yh_fp8_layer_info(const yh_engine* h, int32_t i, const char** conv_name, float* act_scale);
/* Channels of layer i's input tensor / its channel scales (n must equal the channel count; 1.0 where none is set yet). */
int yh_fp8_layer_channels(const yh_engine* h, int32_t i);
int yh_fp8_layer_channel_scales(const yh_engine* h, int32_t i, float* scales, int32_t n);
/* Scales belong to TENSORS (allocations), not to layers: layers that read one allocation share theirs - P3..P7 live in one
 * pyramid buffer, so setting the scales of "p6" also sets them for "p7", "head_t" and "proto0" (yh_fp8_layer_info shows it).
 * Positive finite values are required. yh_invoke / yh_evaluate return YH_ESTATE, naming the layers, until EVERY E4M3
 * input tensor has its scales (by calibration or by these calls). Loading weights AGAIN on a handle discards the scales (they
 * were calibrated for the old weights); scales set before the first load are kept. yh_fp8_set_layer_scale sets the same
 * value in every channel (a per-tensor scale). */
int yh_fp8_set_layer_scale(yh_engine* h, int32_t i, float act_scale);
int yh_fp8_set_layer_channel_scales(yh_engine* h, int32_t i, const float* scales, int32_t n);

/* ---- multi-GPU: the path's one collective (north_star: "weights replicated once via RCCL
 * broadcast over xGMI, no per-step collectives"). The reference's caller is a Rust process (src/main.rs:63-75,
 * src/scene.rs:63), not torch, so the broadcast is reachable through this ABI; librccl.so is opened on first use.
 * Frames then shard over the handles with no further communication. ------------------------------------------- */
#define YH_RCCL_ID_BYTES 128
/* One process, one handle per GPU (a host thread + stream per device): copies the weights
 * loaded on handles[root] to every other handle (ncclCommInitAll + grouped ncclBroadcast of the canonical blob,
 * then the usual validation and repack on each device). */
int yh_group_broadcast_weights(yh_engine** handles, int32_t n, int32_t root);
/* One process per GPU: rank `root` has its weights loaded; every rank calls this with the same id (from
 * yh_rccl_unique_id on one rank, handed to the others by the host's own means: ncclCommInitRank + ncclBroadcast). */
int yh_rccl_unique_id(void* id_out /* YH_RCCL_ID_BYTES */);
int yh_rank_broadcast_weights(yh_engine* h, const void* id, int32_t rank, int32_t nranks, int32_t root);

/* ---- frame sharding over the GPUs of one node: one process, one engine handle per device,
 * one host worker thread + stream per handle, contiguous frame blocks, no per-step collective. The reference's caller is
 * ONE process that owns the frame loop (src/main.rs:63-75, src/scene.rs:77-92); this is what it calls with N frames to get
 * N results over 8 devices. Two members may name the same device (they then share it: the form a one-GPU box can run). */
typedef struct yh_group yh_group;
/* cfg: the per-member configuration (cfg->device is ignored; cfg->max_batch = frames per member per step). */
int yh_group_create(const yh_config* cfg, const int32_t* devices, int32_t n, yh_group** out);
void yh_group_destroy(yh_group* g);
const char* yh_group_last_error(const yh_group* g);   /* g may be NULL: last create error of this thread */
int yh_group_size(const yh_group* g);
/* Member i's own handle (weights on member 0, per-handle tuning, yh_debug_*, ...); owned by the group. */
yh_engine* yh_group_member(yh_group* g, int32_t i);
/* Loads the canonical blob on member 0 and replicates it: ONE RCCL broadcast over the distinct devices
 * (yh_group_broadcast_weights), device-to-device copies for members that share a device with an earlier member, the host as
 * the fallback when librccl cannot be used. yh_group_weights_replication says which of these ran. */
int yh_group_load_weights_host(yh_group* g, const void* blob_host, size_t nbytes);
/* The replication alone (member 0 already holds its weights, e.g. from yh_weights_generate + yh_load_weights_host). */
int yh_group_replicate_weights(yh_group* g);
const char* yh_group_weights_replication(const yh_group* g);
/* fp8 precision: member 0 calibrates on the frames last set on it, every member runs with member 0's scales. */
int yh_group_fp8_calibrate(yh_group* g);
/* n_frames u8 RGB frames [n][S][S][3] in host memory, 1 <= n_frames <= members * max_batch: member i takes a contiguous block
 * (the first n_frames % members members one frame more), copies it in underneath its previous step and enqueues
 * yh_evaluate (with_tail = 1) or yh_invoke (0). Returns when every member has enqueued its step: the frames are free again,
 * the GPUs run on; consecutive calls pipeline. */
int yh_group_evaluate(yh_group* g, const uint8_t* frames_host, int32_t n_frames, int32_t with_tail);
/* The same with frames resident on each member's own device: frames_dev[i] holds counts[i] frames (0: the member sits out). */
int yh_group_evaluate_device(yh_group* g, const uint8_t* const* frames_dev, const int32_t* counts, int32_t with_tail);
/* Captures, on the CALLING thread and one member after the other, the step every member would run for a call with n_frames frames
 * (both input buffers of each member's block size): what the first yh_group_evaluate* of that size would otherwise do before it starts
 * its workers. A host calls it for the frame counts it will use at start-up, so that no capture falls into its frame loop (the
 * reference allocates everything in Yolact::init, src/yolact.rs:28-35). Needs the weights (fp8 precision: and the scales). The group's
 * worker threads never capture and never allocate: DESIGN.md section 7. */
int yh_group_prepare(yh_group* g, int32_t n_frames, int32_t with_tail);
int yh_group_sync(yh_group* g);
/* Results by GLOBAL frame index of the last yh_group_evaluate* (waits for that member's step): as yh_read_detections. */
int yh_group_read_detections(yh_group* g, int32_t frame, int32_t* count, yh_detection* dets, int32_t dets_capacity, uint8_t* masks, size_t masks_capacity);
/* Which member holds global frame `frame` of the last evaluate, and at which index of its batch. */
int yh_group_frame_owner(const yh_group* g, int32_t frame, int32_t* member, int32_t* local);

/* ---- interpreter-shaped surface (lets classify_tile, src/yolact.rs:133-190, port unchanged) -- */

/* interpreter.inputs()[0] + tensor_info(..).dims (src/yolact.rs:149-150): {max_batch,S,S,3}. */
int yh_input_dims(const yh_engine* h, int32_t dims[4]);
/* tensor_data_mut(in).copy_from_slice (src/yolact.rs:161-162): copies n frames of u8 RGB NHWC
 * from host memory into the engine-owned input buffer. The caller's buffer is free again on return, whether it is
 * pageable or pinned (the copy itself is asynchronous on the handle's stream). */
int yh_set_input_u8(yh_engine* h, const uint8_t* rgb_host, int32_t n_frames);
/* Same with frames already resident in device memory (bench path: inputs in HBM). */
int yh_set_input_u8_device(yh_engine* h, const uint8_t* rgb_dev, int32_t n_frames);
/* interpreter.invoke() (src/yolact.rs:163): the network forward for the frames last set.
 * Asynchronous on the handle's stream; yh_sync or any output read waits for it. */
int yh_invoke(yh_engine* h);
/* allocate_tensors() at its proper time (src/yolact.rs:35): captures the step for n_frames frames (with_tail: yh_evaluate's, else
 * yh_invoke's) for both input buffers NOW, on the calling thread, instead of at the first yh_invoke / yh_evaluate of that batch size.
 * A no-op for use_graph = 0. A host that drives several handles from several threads calls this for each handle, serially, before
 * those threads start (a capture is once-only work deep in the HIP runtime; the library never does it on a group's worker thread). */
int yh_prepare(yh_engine* h, int32_t n_frames, int32_t with_tail);
int yh_sync(yh_engine* h);
/* interpreter.outputs().len() / tensor_info(output) (src/yolact.rs:166,170). Output order:
 *   0 loc    [n,P,4]  f16   box regressions
 *   1 conf   [n,P,C]  f16   class logits (pre-softmax)
 *   2 mask   [n,P,32] f16   tanh mask coefficients
 *   3 proto  [n,Hp,Wp,32] f16 prototypes (ReLU)
 *   4 cells  [n,H3,W3,C] f32 class logits of anchor 0 on the stride-8 level: for a 224 input this
 *            is the 28*28*81 tensor the reference reads as results[4] (src/yolact.rs:91,108). */
int yh_output_count(const yh_engine* h);
int yh_output_info(const yh_engine* h, int32_t index, yh_tensor_info* info);
/* tensor_data::<u8|f32>(output) (src/yolact.rs:173,180): copies output `index` to host memory
 * converted to f32 (the reference dequantises to Vec<f32> at :176-181). nfloats = capacity. */
int yh_output_read_f32(yh_engine* h, int32_t index, float* dst_host, size_t nfloats);
/* Device pointer of the engine-owned output buffer; valid until the next yh_invoke. */
const void* yh_output_device_ptr(const yh_engine* h, int32_t index);

/* ---- fused detection path (north_star "Yolact::evaluate") ---------------- */

/* Forward + softmax/threshold + per-class top-k + box decode + Fast-NMS + top max_dets +
 * mask assembly (mask-coeff x prototypes, logit>0 == sigmoid>0.5, box crop) for the frames last
 * set. Asynchronous; results are read with yh_read_detections. */
int yh_evaluate(yh_engine* h);
/* Copies results of the last yh_evaluate for frame `frame`: counts[0] = number of detections d,
 * dets[0..d), and (if masks != NULL) d binary masks of Hp*Wp bytes each (0/1). */
int yh_read_detections(yh_engine* h, int32_t frame, int32_t* count, yh_detection* dets,
                       int32_t dets_capacity, uint8_t* masks, size_t masks_capacity);
int yh_proto_dims(const yh_engine* h, int32_t dims[2]); /* {Hp, Wp} */
int yh_num_priors(const yh_engine* h);
/* Copies the P x 4 prior table (cx,cy,w,h) to host memory. */
int yh_read_priors(const yh_engine* h, float* dst_host, size_t nfloats);

/* ---- instance frame: the detections of the last yh_evaluate painted for the scene (DESIGN.md section 11 "Instance frame") -----
 * What the reference's stop-gap stands in for (src/yolact.rs:1-5 "shoddy replacements", :108 "TODO differentiate between
 * instances", :126 "TODO use confidence to shape mask"; pt_cloud.comp:119): frame `frame` of the last batch, its detections in the
 * rank order yh_read_detections returns, rasterised on the device into a width x height frame of class << 24 | id << 16 (low 16 bits
 * zero) - the layout yh_scene_append_classified(.., frame_on_device = 1, YH_COMPAT_SANE) reads.
 *   class_map  u8 [num_classes - 1], every value 0 .. 3: foreground class -> the scene's class (0 terrain, 1 red robot, 2 blue robot,
 *              3 ball); NULL: the reference's model, 0 -> 1, 1 -> 2, 2 -> 3, everything else 0 (yolact.rs:99-101, :113-115).
 *   eligible   class_map[class_id] != 0 and score >= min_score; any other detection paints nothing and occludes nothing.
 *   id         the number of eligible detections of the same output class with smaller rank (ball 0 is the most confident ball);
 *              an occluded detection keeps its id.
 *   mask       the binary mask (Hp x Wp) resized bilinearly with half-pixel centres and thresholded at > 0.5, in exact integers:
 *              nx = max((2x+1) Wp - W, 0), u0 = nx div 2W, fx = nx mod 2W, u1 = min(u0 + 1, Wp - 1), the same along y; S = (2W-fx)
 *              (2H-fy) M[v0][u0] + fx (2H-fy) M[v0][u1] + (2W-fx) fy M[v1][u0] + fx fy M[v1][u1]; on iff S > 2 W H (a tie is off).
 *   pixel      the value of the eligible detection of smallest rank whose resized mask is on there, or 0.
 * Synchronous, as yh_classify_frame_u32 is: on return the device frame and the instance table are complete (a scene handle on
 * another stream may read the frame), and out_host, if not NULL, holds the width * height pixels. YH_ESTATE: the handle's last step
 * was not a yh_evaluate (nothing run, yh_invoke only, or new input set since); YH_EINVAL: frame outside the last batch, a size outside
 * 1 .. 4096, a class_map value above 3, a NaN min_score. A refused call has touched nothing: an earlier instance frame stays
 * readable. The buffers are allocated at the first call, only grow, and are freed by yh_destroy. */
int yh_instance_frame(yh_engine* h, int32_t frame, int32_t width, int32_t height, const uint8_t* class_map, float min_score,
                      uint32_t* out_host /* or NULL */);
/* Device copy of the last instance frame (NULL before one); valid until the next yh_instance_frame on the handle. */
const uint32_t* yh_instance_device_frame(const yh_engine* h);
/* The instance table of the last instance frame: i32 [m][4] = (detection rank, output class, id, pixels won), one row per eligible
 * detection in rank order, rows with 0 pixels included. *n_instances = m; table may be NULL (the count alone). YH_EOVERFLOW (the
 * count set, nothing copied) if capacity < m rows; YH_ESTATE before an instance frame. */
int yh_instance_read(yh_engine* h, int32_t* n_instances, int32_t* table, int32_t capacity);

/* ---- instance tracks: ids that persist from frame to frame (DESIGN.md section 11 "Instance tracks") ---------------------------
 * yh_instance_frame's id is the detection's place among its class in THIS frame's score order, so two balls swap ids whenever their
 * scores cross. yh_instance_track is the same call with the ids taken from the handle's tracker instead: 128 slots, each with a
 * class, an id, an age (tracked calls since it was last matched) and its last seen mask at prototype resolution. Per call, on the
 * device: the overlap I of every live slot's mask with every eligible detection's, the candidate pairs of equal class with I > 0
 * and 1000 I >= iou_permille (area_slot + area_det - I), matched greedily by largest I / U (ties: smaller age, rank, slot); an
 * unmatched slot ages and dies when age > max_age; an unmatched detection takes the smallest free slot (the oldest lost slots make
 * room if need be) and the smallest id no live slot of its class holds, so a ball that returns within max_age calls gets its id
 * back and a newcomer never takes it. The frame and the instance table are yh_instance_frame's with the track id in the id's
 * place; on an empty tracker they are exactly yh_instance_frame's.
 * States and errors are yh_instance_frame's, plus YH_EINVAL for iou_permille outside 1 .. 1000 or max_age outside 0 .. 255. A
 * refused call has touched nothing (tracker, frame, tables); a call that fails later leaves an empty tracker and no frame. On
 * return yh_instance_device_frame and yh_instance_read show this frame. yh_instance_frame neither reads nor changes the tracker.
 * The tracker is created at the first tracked call and freed by yh_destroy. */
int yh_instance_track(yh_engine* h, int32_t frame, int32_t width, int32_t height, const uint8_t* class_map, float min_score,
                      int32_t iou_permille, int32_t max_age, uint32_t* out_host /* or NULL */);
/* The tracker after the last tracked call: i32 [m][6] = (slot, output class, id, age, area at prototype resolution, detection rank
 * in that call or -1), one row per live slot in slot order. Conventions of yh_instance_read: table may be NULL, YH_EOVERFLOW (the
 * count set, nothing copied) if capacity < m rows; YH_ESTATE before any tracked call. */
int yh_instance_tracks_read(yh_engine* h, int32_t* n_tracks, int32_t* table, int32_t capacity);
/* Empties the tracker (the next tracked call sees no slot; a track table already readable becomes empty). Valid at any time, also
 * before the first tracked call; the instance frame is not touched. */
int yh_instance_track_reset(yh_engine* h);

/* ---- instance batch: the instance frames of n frames of a step in one pair of launches (DESIGN.md section 11 "Instance batch") --
 * Frames first_frame .. first_frame + n_frames - 1 of the last yh_evaluate painted at once: frame b of the batch has exactly the
 * packed frame and the instance table yh_instance_frame(h, first_frame + b, width, height, class_map, min_score, ..) gives - the
 * same device code runs per frame. One upload of the class map, one read-back, one wait, whatever n_frames is. out_host, if not
 * NULL, receives the n_frames * width * height pixels, frame after frame.
 * States and errors are yh_instance_frame's, plus YH_EINVAL for n_frames < 1 or first_frame + n_frames beyond the last step's
 * batch. Synchronous. Everything is checked before anything is touched: a refused call leaves the earlier batch's frames, tables
 * and pointer as they were; a call that fails later leaves no batch. The batch has buffers of its own (allocated at the first
 * call, grow only, freed by yh_destroy): it does not disturb yh_instance_device_frame, yh_instance_read or the tracker, and
 * yh_instance_frame / yh_instance_track do not disturb the batch. The batch with ids that persist is yh_instance_track_batch
 * below; a plain batch after a tracked one replaces its frames and leaves every tracker alone. */
int yh_instance_batch(yh_engine* h, int32_t first_frame, int32_t n_frames, int32_t width, int32_t height, const uint8_t* class_map,
                      float min_score, uint32_t* out_host /* [n][H][W] or NULL */);
/* Device copy of the last batch's frames [n][H][W] (NULL before a batch); valid until the next yh_instance_batch on the handle.
 * It is what yh_scene_batch_stage_frames(.., frames_on_device = 1) takes. */
const uint32_t* yh_instance_batch_device_frames(const yh_engine* h);
/* The instance table of frame `frame` (0 .. n - 1) of the last batch, with yh_instance_read's conventions: table may be NULL,
 * YH_EOVERFLOW (the count set, nothing copied) if capacity < m rows, YH_ESTATE before a batch; YH_EINVAL for a frame outside it. */
int yh_instance_batch_read(yh_engine* h, int32_t frame, int32_t* n_instances, int32_t* table, int32_t capacity);

/* ---- instance track batch: a step's frames tracked per camera stream, one wait (DESIGN.md section 11 "Instance track batch") ---
 * The handle holds a bank of YH_TRACK_STREAMS_MAX trackers; stream 0 is the one yh_instance_track, yh_instance_tracks_read and
 * yh_instance_track_reset use. yh_instance_track_batch on frames first_frame .. first_frame + n_frames - 1 is exactly this: for
 * b = 0 .. n_frames - 1 in order, a yh_instance_track call on frame first_frame + b against the tracker of streams[b]. Frame b's
 * packed frame and instance table are that call's, its track table is that tracker's right after that call, and every tracker ends
 * in the state those calls leave; trackers of different streams never see each other. Single and batched calls on stream 0
 * continue each other in both directions. Frames of different streams share launches, frames of one stream are a chain on the
 * device: there is one wait, whatever n_frames is.
 * A tracked batch is an instance batch: its frames and instance tables replace the last batch's (yh_instance_batch_device_frames,
 * yh_instance_batch_read, with the track id in the id's place); yh_instance_device_frame and yh_instance_read are not touched.
 * States and errors are yh_instance_batch's, plus yh_instance_track's for iou_permille and max_age, plus YH_EINVAL for a stream
 * outside 0 .. YH_TRACK_STREAMS_MAX - 1 (the message names the frame). Everything is checked before anything is touched: a
 * refused call leaves the previous batch (frames, tables, pointer, track tables) and every tracker as they were; a call that
 * fails later leaves no batch and empties every tracker it named. A stream's tracker is created at its first use and freed by
 * yh_destroy. */
#define YH_TRACK_STREAMS_MAX 64
int yh_instance_track_batch(yh_engine* h, int32_t first_frame, int32_t n_frames, int32_t width, int32_t height,
                            const uint8_t* class_map, float min_score, int32_t iou_permille, int32_t max_age,
                            const int32_t* streams /* [n_frames], each 0 .. YH_TRACK_STREAMS_MAX - 1, or NULL: all 0 */,
                            uint32_t* out_host /* [n][H][W] or NULL */);
/* The tracker of frame `frame`'s stream right after that frame of the last tracked batch: i32 [m][6], yh_instance_tracks_read's
 * layout and conventions. YH_ESTATE if the handle's last instance batch was not a tracked one (a plain yh_instance_batch since
 * replaces the frames); YH_EINVAL for a frame outside the batch. */
int yh_instance_track_batch_read(yh_engine* h, int32_t frame, int32_t* n_tracks, int32_t* table, int32_t capacity);
/* Empties one stream's tracker, as yh_instance_track_reset does stream 0's; stream -1: all of them. Valid at any time. */
int yh_instance_track_reset_stream(yh_engine* h, int32_t stream);

/* ---- reference-compat path: Yolact::classify (src/yolact.rs:39-41, :192-234) --------------- */

/* In-place classify of one packed camera frame: `frame` holds width*height u32 pixels packed
 * r<<24|g<<16|b<<8 (src/scene.rs:86). Runs, all on device: unpack (yolact.rs:195-201), Triangle
 * resize to (2S x S) (yolact.rs:208), two S x S tiles as one batch of 2 (yolact.rs:213-217),
 * forward, output-4 gated argmax (yolact.rs:108-118), ids (yolact.rs:52-88), pack + x8 nearest
 * upsample (yolact.rs:127-128), stitch (yolact.rs:219-220), Triangle resize back (yolact.rs:231)
 * and repack (yolact.rs:233). Requires input_size*2 x input_size tiles, input_size % 8 == 0
 * (224 for the reference) and max_batch >= 2. Synchronous (the reference's classify is). */
int yh_classify_frame_u32(yh_engine* h, uint32_t* frame_host, int32_t width, int32_t height,
                          int32_t compat_mode);
/* ---- classify batch: n camera frames through one network step (DESIGN.md section 11 "Classify batch") ----------------------------
 * Yolact::classify on n frames at once. frames: [n][H][W] packed u32 (r<<24|g<<16|b<<8), on the host or
 * (frames_on_device = 1) on the device. The 2n tiles run as ONE step of the engine (needs 2n <= max_batch).
 * out_host: [n][H][W] or NULL; it may be the host `frames` itself (in place, as the reference's classify).
 * diverged_host: [n] ints or NULL.
 * What "equal" means: the engine's launch plan depends on the batch size (tile choice, split-K), so output 4 of tile t in a step
 * of 2n tiles is not promised to be the bits of the same tile in a step of 2. Everything around the network is exact: tiles 2b and
 * 2b + 1 of the step are the reference's pre half of frame b (unpack, Triangle resize to 2S x S, crop), frame b of the result is
 * the reference's post half (argmax, ids, pack, x8 upsample, stitch, Triangle resize back, repack) of the engine's own output 4
 * for those two tiles, and with n = 1 the whole call equals yh_classify_frame_u32 bit for bit.
 * Synchronous. One host-to-device copy when the frames are on the host, one read-back and one wait per call, whatever n (in
 * YH_COMPAT_STRICT with out_host the frames are read back behind the divergence flags, a second wait). Everything is checked
 * before anything is touched: YH_EINVAL for n_frames < 1, 2 n_frames > max_batch, a bad mode or size, or input_size not a multiple
 * of 8 (<= 512); YH_ESTATE without weights; a refused call leaves the previous batch and its pointer as they were, a call that
 * fails later leaves no batch. The batch has buffers of its own (allocated at the first call, grow only, freed by yh_destroy): it
 * does not disturb yh_classify_device_frame, and yh_classify_frame_u32 does not disturb the batch.
 * In YH_COMPAT_STRICT a frame whose flood fill would not terminate makes the call return YH_EDIVERGE: out_host is untouched,
 * diverged_host[b] is 1 for exactly the frames that diverged, and no batch is left (the pointer is NULL). On success
 * diverged_host is all zero. */
int yh_classify_batch_u32(yh_engine* h, const uint32_t* frames, int32_t frames_on_device, int32_t n_frames,
                          int32_t width, int32_t height, int32_t compat_mode,
                          uint32_t* out_host, int32_t* diverged_host);
/* Device copy of the last batch's classified frames [n][H][W]; NULL before a batch or after a failed one; valid until the next
 * yh_classify_batch_u32 on the handle. It is what yh_scene_batch_stage_frames(.., frames_on_device = 1) takes. */
const uint32_t* yh_classify_batch_device_frames(const yh_engine* h);
/* The post-network half only, on caller-provided output-4 logits (n_tiles x cells x C f32, host):
 * exactly `postprocess` (src/yolact.rs:90-131) per tile. out: n_tiles x (S*S) u32. Lets the
 * reference's integer logic be checked bit-for-bit without a network in the loop. */
int yh_postprocess_cells(yh_engine* h, const float* cells_host, int32_t n_tiles, uint32_t* out_host,
                         int32_t compat_mode);
/* Device Triangle resize of an RGB8 image, the `image` crate call at src/yolact.rs:208,:231. */
int yh_resize_triangle_rgb8(yh_engine* h, const uint8_t* src_host, int32_t sw, int32_t sh,
                            uint8_t* dst_host, int32_t dw, int32_t dh);

/* ---- TFLite model path: run the reference's own model family ---------------- */
/* A user who holds data/FRC_model.tflite (uint8 per-tensor quantised MobileNetV2-FPN YOLACT,
 * data/README.md:5-16; absent from the checkout) runs it here instead of tflite+EdgeTPU - and so does
 * one who converts such a model today: int8 tensors, int8 weights with zero point 0 and one scale per
 * tensor or per output channel, uint8 or float32 at the graph's edges behind QUANTIZE / DEQUANTIZE
 * (DESIGN.md section 11 "TFLite int8"; classify still asks for a uint8 input and a uint8 or float32
 * output 4, as yolact.rs:171-186 does). Supported
 * builtin ops: the histogram of data/FRC_model_edgetpu.log:7-19 (CONV_2D, DEPTHWISE_CONV_2D, ADD,
 * PAD, RESIZE_BILINEAR, TANH, RELU, CONCATENATION, RESHAPE, QUANTIZE) plus RELU6 and DEQUANTIZE.
 * The EdgeTPU-compiled file is one custom op and is rejected with a message naming it. */
typedef struct yh_tfl yh_tfl;
/* Parses only (no GPU needed): YH_OK or YH_EWEIGHTS with a message; never reads out of bounds. */
int yh_tfl_validate(const void* model_bytes, size_t nbytes, int32_t* n_tensors, int32_t* n_ops, char* err, size_t err_cap);
/* FlatBufferModel::build_from_file + InterpreterBuilder + allocate_tensors (src/yolact.rs:18-35). */
int yh_tfl_create(const void* model_bytes, size_t nbytes, int32_t device, yh_tfl** out);
/* The same with room for up to max_images images per invoke, 1 .. YH_TFL_MAX_IMAGES (yh_tfl_create: 2, the two tiles of a frame).
 * Every activation, every constant an operator reads as a data operand and the graph input are stored max_images times
 * (image-major); a classify batch of n frames needs max_images >= 2n, and 512 is the 256 frames of a yh_scene_batch. YH_EINVAL,
 * before the device is touched, for any other max_images. Why 512 holds: every launch of the executor's kernels was checked at that
 * image count. Element-wise kernels, PAD, CONCATENATION and RESHAPE index with 64 bits; the per-image kernels take the image
 * as a grid dimension (<= 65535) and index one image with the 32 bits they use at one image; the only 32-bit expression the image
 * count enters is the int8 MFMA convolutions' pixel index (M = Ho x Wo x images, rounded up to a tile by the grid), and the tile
 * prefix sums of a convolution group built on it. A model where Ho x Wo x max_images of a convolution passes 2^31 - 65 is refused
 * at create (YH_EINVAL), a group whose tiles pass 2^31 - 1 at the first invoke of that image count: no model is capped below 512
 * by its size alone (a 224 x 224 MobileNetV2's largest convolution: 112 x 112 x 512 = 6.4 M pixels). */
#define YH_TFL_MAX_IMAGES 512
int yh_tfl_create_batch(const void* model_bytes, size_t nbytes, int32_t device, int32_t max_images, yh_tfl** out);
void yh_tfl_destroy(yh_tfl* h);
const char* yh_tfl_last_error(const yh_tfl* h);
int yh_tfl_input_info(const yh_tfl* h, yh_tensor_info* info);                 /* inputs()[0], :149-150 */
int yh_tfl_output_count(const yh_tfl* h);                                      /* outputs(), :166 */
int yh_tfl_output_info(const yh_tfl* h, int32_t i, yh_tensor_info* info);      /* tensor_info(output), :170-175 */
/* Images per invoke: 1 (default) .. the handle's max_images (2 unless it came from yh_tfl_create_batch) - the model is batch 1 (yolact.rs:149-150), its two tiles per frame are independent
 * (:216-217) and run as one pass of a batch plan (activations image-major; yh_tfl_classify_frame_u32 does this itself).
 * yh_tfl_set_input then takes n images, yh_tfl_output_read / yh_tfl_tensor_read return n. YH_EINVAL for a model with an
 * operator along the image axis. */
int yh_tfl_set_batch(yh_tfl* h, int32_t n_images);
int yh_tfl_set_input(yh_tfl* h, const void* data, size_t nbytes);              /* tensor_data_mut copy, :161-162 */
int yh_tfl_invoke(yh_tfl* h);                                                  /* interpreter.invoke(), :163 */
int yh_tfl_output_read(yh_tfl* h, int32_t i, void* dst, size_t nbytes);        /* tensor_data::<u8|f32>, :173,:180 */
/* Yolact::classify (src/yolact.rs:192-234) with this model in the middle: two S x S tiles, one
 * invoke each, output 4 dequantised (:177) and post-processed (:90-131), all on device. (The two tiles
 * share one invoke of two images where the handle has room for two and no operator works along the
 * image axis; a handle made with max_images = 1 runs them one after the other: the same bytes.) */
int yh_tfl_classify_frame_u32(yh_tfl* h, uint32_t* frame_host, int32_t width, int32_t height, int32_t compat_mode);
/* ---- TFLite classify batch: n camera frames through one invoke of 2n images (DESIGN.md section 11 "TFLite classify batch") -----
 * yh_classify_batch_u32 for a yh_tfl handle. frames: [n][H][W] packed u32 (r<<24|g<<16|b<<8), on the host or
 * (frames_on_device = 1) on the device. The 2n tiles are written straight into the model's input tensor as images 2b, 2b + 1 and
 * run as ONE invoke (needs 2n <= max_images: yh_tfl_create_batch). out_host: [n][H][W] or NULL; it may be the host `frames`
 * itself (in place, as the reference's classify). diverged_host: [n] ints or NULL.
 * What "equal" means: MORE than for the engine. Every kernel form of the executor is integer-exact, so an image's bytes do not
 * depend on how many images share its invoke: frame b of the result is yh_tfl_classify_frame_u32 on frame b alone, bit for bit,
 * for every n - and with it the reference's pre half, TFLite's uint8 arithmetic on each tile, and the reference's post half.
 * Synchronous. One host-to-device copy when the frames are on the host, one read-back and one wait per call, whatever n (in
 * YH_COMPAT_STRICT with out_host the frames are read back behind the divergence flags, a second wait). Everything is checked
 * before anything is touched: YH_EINVAL for n_frames < 1, 2 n_frames > max_images, a bad mode or size, a model
 * yh_tfl_classify_frame_u32 refuses (input not [1,S,S,3] uint8 with S % 8 == 0, S <= 512; fewer than five outputs; output 4 not
 * (S/8)^2 cells of >= 4 logits), or a model with an operator along the image axis (one image per invoke: classify its frames one
 * by one with yh_tfl_classify_frame_u32); a refused call leaves the previous batch and its pointer as they were, a call that
 * fails later leaves no batch. The batch has buffers of its own (allocated at the first call, grow only, freed by yh_tfl_destroy):
 * yh_tfl_classify_frame_u32 does not disturb the batch's frames and the batch does not disturb the single call; both run the
 * handle's one plan, so the model's tensors hold whichever ran last. The yh_tfl_set_batch value of the caller survives the call.
 * In YH_COMPAT_STRICT a frame whose flood fill would not terminate makes the call return YH_EDIVERGE: out_host is untouched,
 * diverged_host[b] is 1 for exactly the frames that diverged, and no batch is left (the pointer is NULL). On success
 * diverged_host is all zero. */
int yh_tfl_classify_batch_u32(yh_tfl* h, const uint32_t* frames, int32_t frames_on_device, int32_t n_frames,
                              int32_t width, int32_t height, int32_t compat_mode,
                              uint32_t* out_host, int32_t* diverged_host);
/* Device copy of the last batch's classified frames [n][H][W]; NULL before a batch or after a failed one; valid until the next
 * yh_tfl_classify_batch_u32 on the handle. It is what yh_scene_batch_stage_frames(.., frames_on_device = 1) takes. */
const uint32_t* yh_tfl_classify_batch_device_frames(const yh_tfl* h);

/* ---- TFLite detections: the detection tail on the model's own output tensors (DESIGN.md section 11 "TFLite detections") -----
 * The reference stops at an argmax over output 4 (src/yolact.rs:3-5, :93-95, :108). The model's other four outputs - loc [1,P,4],
 * conf [1,P,C], mask [1,P,32], proto [1,hp,wp,32] - are what a YOLACT detection tail reads: softmax and threshold, per-class
 * top-k, SSD decode, Fast-NMS, top max_dets, mask assembly. yh_tfl_detect_setup binds that tail to four outputs of the handle's
 * model; it then runs on the device on the tensors as they lie - uint8, int8 or float32, no host copy, no f16 copy - for every
 * image of the last invoke. What is computed: a quantised element's value is (float)(q - zero_point) * scale (one f32 multiply);
 * scores, candidates, boxes, NMS, ranking and crop windows are the engine's tail (yh_evaluate) on those values, operation for
 * operation, with priors indexed by the prior; the mask bit of a pixel inside a detection's crop window is the sign of the exact
 * integer sum over k of (proto_q[k] - z_proto)(mask_q[k] - z_mask) when mask and proto are both quantised, and the engine's
 * fmaf chain on the values above when either is float32.
 * A .tflite file holds no priors: the host passes them, [P][4] cx, cy, w, h (yolact_amd.tfl_priors builds YOLACT's).
 * yh_tfl_detect_setup checks everything before it allocates, and yh_tfl_last_error names the rule: each of the four tensors is a
 * graph output of kind YH_KIND_U8 / _I8 / _F32 with one scale and zero point (a per-channel head is refused), shaped as above with
 * one P that equals n_priors and C in 2 .. 81 (a model whose heads are transposed or that has another number of prototypes than
 * 32 is refused); a quantised tensor's scale is finite and positive and its zero point inside its type's range; top_k, max_dets
 * and (C - 1) * top_k within the engine's limits (256, 128, 16384); max_images in 0 .. the handle's, and 1 for a model with an
 * operator along the image axis. A refused setup returns YH_EINVAL and leaves the handle - an earlier setup included - as it was.
 * A second setup replaces the first.
 * MEMORY: the workspaces are allocated by the setup, never by a later call, for max_images images. The candidate lists alone take
 *     max_images * (C - 1) * P * 8 bytes
 * (every (class, prior) pair may pass the threshold) - 128 MB at 64 images of an 81-class model with 3 117 priors (MobileNetV2-FPN at
 * 224 x 224), 1.02 GB at 512 - and the masks max_images * max_dets * hp * wp bytes; the rest is small beside them
 * ((C - 1) * top_k * 24 + max_dets * 176 bytes per image). Hence max_images: a handle made for 512 images (classify batches)
 * that detects on 8 at a time pays for 8.
 * yh_tfl_evaluate: yh_tfl_invoke and the tail on every image of that invoke; asynchronous, the tail's four launches follow the
 * invoke on the handle's stream (eager launches, outside the invoke's captured graph). yh_tfl_detect: the tail alone on the
 * outputs of the last invoke, whoever made it (yh_tfl_invoke, yh_tfl_classify_frame_u32, yh_tfl_classify_batch_u32: its 2n tiles).
 * States: yh_tfl_evaluate / yh_tfl_detect before a setup, yh_tfl_detect before any invoke, and yh_tfl_read_detections when no tail
 * has run since the last yh_tfl_set_input or invoke return YH_ESTATE; a batch larger than the setup's max_images YH_EINVAL. A
 * refused call has touched nothing. */
typedef struct yh_tfl_detect_config {
    int32_t outputs[4];   /* indices into the model's outputs: loc, conf, mask, proto; yh_tfl_default_detect_config sets 0,1,2,3 */
    int32_t top_k, max_dets;          /* 200, 100; limits as the engine's tail (256, 128) */
    float conf_thresh, nms_thresh;    /* 0.05, 0.5 */
    int32_t max_images;               /* images the workspaces are sized for; 0: the handle's max_images */
    int32_t reserved[4];              /* zero */
} yh_tfl_detect_config;
void yh_tfl_default_detect_config(yh_tfl_detect_config* cfg);
int yh_tfl_detect_setup(yh_tfl* h, const yh_tfl_detect_config* cfg, const float* priors_host /* [P][4] cx,cy,w,h */, int32_t n_priors);
int yh_tfl_evaluate(yh_tfl* h);
int yh_tfl_detect(yh_tfl* h);
/* As yh_read_detections, for image `image` of the last yh_tfl_evaluate / yh_tfl_detect: the one wait. */
int yh_tfl_read_detections(yh_tfl* h, int32_t image, int32_t* count, yh_detection* dets, int32_t dets_capacity,
                           uint8_t* masks, size_t masks_capacity);
int yh_tfl_proto_dims(const yh_tfl* h, int32_t dims[2]);   /* {hp, wp} of the setup; YH_EINVAL before one */
/* The setup's result buffers on the device (NULL before a setup; valid until the next setup or yh_tfl_destroy; written by the
 * tail's launches on the handle's stream): what yh_tfl_instance_batch / yh_tfl_instance_frames read. */
const yh_detection* yh_tfl_detections_device(const yh_tfl* h);   /* [max_images][max_dets] */
const int32_t*      yh_tfl_detection_counts_device(const yh_tfl* h);
const uint8_t*      yh_tfl_masks_device(const yh_tfl* h);        /* [max_images][max_dets][hp*wp] */

/* ---- TFLite instance frames: the setup's detections painted for the scene (DESIGN.md section 11 "TFLite instance frames") ------
 * What yh_instance_batch is to yh_evaluate: the detections of the last yh_tfl_evaluate / yh_tfl_detect, read on the device where the
 * tail left them, rasterised into packed class << 24 | id << 16 frames of width x height that yh_scene_batch_stage_frames takes.
 * yh_tfl_instance_batch paints images first_image .. first_image + n_images - 1, each exactly as yh_instance_batch paints a frame
 * (eligibility class_map[class_id] != 0 and score >= min_score; id = the eligible detections of the same output class with smaller
 * rank; the exact-integer bilinear mask resize, on iff S > 2 W H; the smallest rank wins a pixel); its table rows are int32 [4] =
 * (rank, output class, id, pixels won).
 * yh_tfl_instance_frames paints camera frames: after yh_tfl_classify_batch_u32 the tail's images are the two S x S tiles of each
 * frame, and frame b is painted from images 2 (first_frame + b) (tile 0, the left half) and 2 (first_frame + b) + 1 (tile 1).
 * The eligible detections of both tiles are ordered by score descending (float32), ties to tile 0 before tile 1 and then to the
 * smaller rank - the stable merge of the two lists - which gives the frame rank q < 2 max_dets; the id counts the eligible
 * detections of the same output class with smaller q, across the tiles; a detection of tile t has the stitched hp x 2wp mask that
 * is its own on columns t wp .. (t + 1) wp - 1 and 0 elsewhere, resized by the same rule with input width 2wp; the smallest q wins
 * a pixel. Its table rows are int32 [5] = (tile, rank within the tile, output class, id, pixels won) in frame order. An object
 * across the seam is two instances, one per tile; a seam pixel whose horizontal weight is exactly one half (a whole column at odd
 * width) belongs to neither tile and stays 0.
 * class_map: uint8 [C - 1] of the setup's C with values 0 .. 3, NULL: foreground 0, 1, 2 -> 1, 2, 3. out_host: [n][height][width]
 * or NULL. Both calls are synchronous (one class-map upload, one read-back, one wait, whatever n): on return another stream may
 * read the frames. Both fill the handle's ONE batch - the later call replaces the earlier - with buffers of its own (allocated at
 * the first call, grow only, freed by yh_tfl_destroy; the sets take images x hp x wp x 16 bytes); neither touches the detections,
 * the classify batch's frames, the model's tensors or the invoke's captured graph.
 * Checked before anything is touched: YH_ESTATE before a setup, or when no tail has run since the last yh_tfl_set_input or invoke
 * (what yh_tfl_read_detections refuses); YH_EINVAL for n < 1, images or frames outside the last tail's (per frame:
 * 2 (first_frame + n_frames) <= its images), a size outside 1 .. 4096, a class_map value above 3, a NaN min_score. A refused call
 * leaves the previous batch, its pointer and its tables as they were; a call that fails later leaves no batch. */
int yh_tfl_instance_batch(yh_tfl* h, int32_t first_image, int32_t n_images, int32_t width, int32_t height,
                          const uint8_t* class_map, float min_score, uint32_t* out_host /* [n][H][W] or NULL */);
int yh_tfl_instance_frames(yh_tfl* h, int32_t first_frame, int32_t n_frames, int32_t width, int32_t height,
                           const uint8_t* class_map, float min_score, uint32_t* out_host /* [n][H][W] or NULL */);
/* Device copy of the last batch's frames [n][H][W]; NULL before a batch or after a failed one; valid until the next instance call on
 * the handle. It is what yh_scene_batch_stage_frames(.., frames_on_device = 1) takes. */
const uint32_t* yh_tfl_instance_device_frames(const yh_tfl* h);
/* The table of image / frame `index` of the last batch, with the conventions of yh_instance_batch_read (capacity in rows; table
 * NULL: the row count only; YH_EOVERFLOW if it does not fit); a row has yh_tfl_instance_row_width ints: 4 after
 * yh_tfl_instance_batch, 5 after yh_tfl_instance_frames. */
int yh_tfl_instance_read(yh_tfl* h, int32_t index, int32_t* n_instances, int32_t* table, int32_t capacity);
int yh_tfl_instance_row_width(const yh_tfl* h);

/* ---- scene back-end: append_scene's two compute dispatches (src/scene.rs:147-331) --------------
 * shaders/pt_cloud.comp (depth + class image -> bird's-eye height map with sigmoid bumps, ball centroids) and
 * shaders/pt_cloud_weights.comp (world positions, 8-neighbour edge lengths) as HIP kernels, one lane per pixel in
 * 8x8 workgroups ([80,60,1] at 640x480: scene.rs:245,:256). The shaders as written race and use undefined GLSL;
 * what is computed is the deterministic reading of DESIGN.md §Scene (stage-by-stage completion, exact ball means).
 * compat_mode: YH_COMPAT_STRICT keeps pack()'s `&` (pt_cloud_weights.comp:32: every neighbour position decodes to
 * world(0,0)); YH_COMPAT_SANE measures the distance to the actual neighbour. */
typedef struct yh_scene yh_scene;
int yh_scene_create(int32_t device, int32_t width, int32_t height, yh_scene** out);   /* scene.rs:150-155: the storage images */
void yh_scene_destroy(yh_scene* h);
const char* yh_scene_last_error(const yh_scene* h);
/* One frame: depth u16 [h][w] (the R16_UINT texture, scene.rs:197) and the class image [h][w][2] = (class, id) (the
 * R8G8_UINT texture, scene.rs:198), both in host memory; the buffers are free again on return (pageable or pinned).
 * The computation is asynchronous on the handle's stream. */
int yh_scene_append(yh_scene* h, const uint16_t* depth_host, const uint8_t* class_id_host, int32_t compat_mode);
/* The class image taken straight from a classified frame as yh_classify_frame_u32 leaves it (packed u32 [h][w];
 * frame_on_device = 1: a device pointer, e.g. yh_classify_device_frame - no host round trip of the class image).
 * STRICT reads it as the reference does - the low 16 bits (src/scene.rs:93), class = bits 7-0, id = bits 15-8, which
 * classify leaves zero - SANE reads class = bits 31-24, id = bits 23-16. */
int yh_scene_append_classified(yh_scene* h, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device, int32_t compat_mode);
/* scene.rs:284-330: height map u32 [h][w], world / connections0 / connections1 f32 [h][w][4], balls f32 [100][4]
 * = (mean x, mean y, pixel count, 0). Any pointer may be NULL. Waits for the frame. */
int yh_scene_read(yh_scene* h, uint32_t* map, float* world, float* conn0, float* conn1, float* balls);
/* modify_path (src/path.rs:25-120) on the fields of the last appended frame, which stay on the device: the multi-source cost
 * field from the targets over the 4-connected pixel grid - an edge costs the scene's connection length plus the height step
 * (path.rs:59) -, every pixel's successor, and the route from the start pixel to a target. The reference's function cannot run
 * (it indexes 224 x 224 arrays by x + y * 480); what is computed is the definition of DESIGN.md section 11 "Path planner".
 * targets_xy: n_targets pixels (x, y), or NULL: the first n_targets balls that have pixels, in id order, at their truncated
 * means (balls[..3], path.rs:37-38; scene.rs:321), those outside the frame dropped. (start_x, start_y): the robot's pixel
 * (START_NODE, path.rs:93: (400, 479) at 640 x 480). Synchronous: returns when the route is known. The planner's buffers are
 * allocated at the first plan on a handle. YH_ESTATE: no frame yet, the last frame was appended in YH_COMPAT_STRICT (its
 * connections are all distances to world(0,0): no planner is defined on them), or targets_xy is NULL and no ball is usable;
 * YH_EINVAL: n_targets < 1, a target or the start outside the frame, or (W + H) * (2 * max(H, 101) + 1) >= 2^24. A call refused
 * with YH_EINVAL or YH_ESTATE has touched nothing: an earlier plan of the same frame stays readable. A call that fails later
 * (YH_EHIP) leaves no plan. */
int yh_scene_plan(yh_scene* h, const int32_t* targets_xy /* [n][2] or NULL: the frame's balls */, int32_t n_targets,
                  int32_t start_x, int32_t start_y);
/* yh_scene_plan on the 4- or the 8-connected pixel grid (DESIGN.md section 11 "Diagonals"); yh_scene_plan is this function
 * with connectivity 4. With 8 the four diagonal lengths of the connections join the graph (up-left conn1[..][3], up-right
 * conn0[..][1], down-left conn1[..][1], down-right conn0[..][3]; the same cost equation, the minimum over up to eight
 * neighbours), the successor is the first neighbour in the order (left, right, up, down, up-left, up-right, down-left,
 * down-right) that achieves the cost, and a rotation is float32((4 - k) * pi / 4) for k in 0 .. 4 steps of 45 degrees between
 * the heading into a node and the heading out of it: pi, 3 pi / 4, pi / 2, pi / 4, 0. The plan remembers its connectivity
 * (yh_scene_plan_time replays it). Errors as yh_scene_plan, and YH_EINVAL for a connectivity other than 4 or 8; YH_ESTATE for 8
 * on fields uploaded through yh_scene_set_fields whose diagonal lengths are not all finite, >= 1 and equal at both ends
 * (frames appended in YH_COMPAT_SANE always are). A refused call has touched nothing. */
int yh_scene_plan_conn(yh_scene* h, const int32_t* targets_xy /* [n][2] or NULL: the frame's balls */, int32_t n_targets,
                       int32_t start_x, int32_t start_y, int32_t connectivity /* 4 or 8 */);
/* The last plan (path.rs:93-119: the walk from START_NODE, Path.directions): cost f32 [h][w], next i32 [h][w] (linear index
 * y * w + x of the successor, -1 at targets), path_xy i32 [cap][2] (the route's pixels, start and target included),
 * directions f32 [cap][2] = (magnitude, rotation) per step of the route (*path_len - 1 pairs, what Path::serialize sends,
 * path.rs:17-21); any pointer may be NULL. *path_len = nodes on the route. YH_EOVERFLOW (and *path_len set, nothing copied)
 * if path_capacity < *path_len while path_xy or directions is asked for; YH_ESTATE before a plan, or when a frame was
 * appended since the plan. */
int yh_scene_plan_read(yh_scene* h, float* cost, int32_t* next, int32_t* path_xy, float* directions,
                       int32_t path_capacity, int32_t* path_len);
/* The tour: which target first, then which, and the whole route (DESIGN.md section 11 "Tour"; path.rs:38 "Dijkstra's algorithm
 * with 3 targets", :35,:66 ball[node]). K <= YH_TOUR_MAX distinct targets, chosen as yh_scene_plan chooses them (explicit pixels,
 * or NULL: the first n_targets balls; of those a ball outside the frame, or on an earlier ball's pixel, is dropped). Per target
 * t_b the single-target cost field d_b and successor field next_b of yh_scene_plan (K fields solved in the same launches), the
 * label of the nearest target per pixel, the leg matrix, the visiting order of least total cost (all K! orders, on the host from
 * the leg matrix, f32 sums left to right, ties to the lexicographically smallest) and the legs' walks joined into one route.
 * Synchronous. The tour's buffers are allocated at the first tour on a handle, sized by the K in use (they only grow), and are
 * not the single plan's: yh_scene_plan and yh_scene_plan_tour do not disturb each other's results. Errors as yh_scene_plan, and
 * YH_EINVAL for n_targets > YH_TOUR_MAX and for two equal explicit targets. A call refused with YH_EINVAL or YH_ESTATE has
 * touched nothing: an earlier tour of the same frame stays readable. A call that fails later (YH_EHIP) leaves no tour. */
#define YH_TOUR_MAX 6
int yh_scene_plan_tour(yh_scene* h, const int32_t* targets_xy /* [n][2] or NULL: the frame's balls */, int32_t n_targets,
                       int32_t start_x, int32_t start_y);
/* yh_scene_plan_tour with every field, successor and rotation taken on the 4- or the 8-connected grid, as yh_scene_plan_conn
 * defines them; labels, leg matrix, order and joining are unchanged. yh_scene_plan_tour is this function with connectivity 4.
 * The tour remembers its connectivity (yh_scene_tour_time replays it). Errors as yh_scene_plan_tour and yh_scene_plan_conn. */
int yh_scene_plan_tour_conn(yh_scene* h, const int32_t* targets_xy /* [n][2] or NULL: the frame's balls */, int32_t n_targets,
                            int32_t start_x, int32_t start_y, int32_t connectivity /* 4 or 8 */);
/* The last tour; any pointer may be NULL. With K = *n_targets (<= YH_TOUR_MAX; size the small arrays for YH_TOUR_MAX):
 *   targets_xy i32 [K][2]   the targets in use, t_0 .. t_{K-1}
 *   order      i32 [K]      the visiting order o: indices into targets_xy
 *   legs       f32 [K+1][K] legs[0][b] = d_b[start], legs[1 + a][b] = d_b[t_a]: the cost to travel FROM t_a TO t_b (diagonal 0)
 *   total      f32          the order's total, fl(..fl(legs[0][o_0] + legs[1 + o_0][o_1]) + ..)
 *   cost       f32 [K][h][w], next i32 [K][h][w]   field b has the single target t_b (next_b is -1 at t_b only)
 *   label      u8  [h][w]   the smallest b with d_b[v] == min over b of d_b[v]
 *   path_xy    i32 [cap][2] the joined route: start .. t_{o_0} .. t_{o_1} .., a junction node once; a leg whose start is its own
 *                           target adds no node. *path_len = its nodes
 *   directions f32 [cap][2] (magnitude, rotation) per step, *path_len - 1 pairs: the magnitude of a step inside leg j is the
 *                           difference of d_{o_j}; rotation 0 at step 0 and where the route reverses (at a junction only),
 *                           float32(pi) when straight, float32(pi / 2) for a turn (8-connected: also 3 pi / 4 and pi / 4)
 *   leg_ends   i32 [K]      index in path_xy of the node where leg j ends (t_{o_j})
 * YH_EOVERFLOW (and *path_len set, nothing copied) if path_capacity < *path_len while path_xy or directions is asked for;
 * YH_ESTATE before a tour, or when a frame was appended since the tour. */
int yh_scene_tour_read(yh_scene* h, int32_t* n_targets, int32_t* targets_xy, int32_t* order, float* legs, float* total,
                       float* cost, int32_t* next, uint8_t* label, int32_t* path_xy, float* directions, int32_t* leg_ends,
                       int32_t path_capacity, int32_t* path_len);
/* The turn-aware plan (DESIGN.md section 11 "Turns"): yh_scene_plan_conn(.., 8)'s graph over states (pixel, heading) with a price
 * for turning in place, so that the route handed to a drive base does not zig-zag between near-equal headings. Heading h in 0 .. 7
 * is the compass index 0 right (1, 0), 1 down-right, 2 down, 3 down-left, 4 left, 5 up-left, 6 up (0, -1), 7 up-right; h + 1 is
 * clockwise on the image (y down), indices wrap. State (v, h) may drive to (v + s_h, h) for the 8-connected plan's edge term of
 * that direction, fl(fl(d[h][v + s_h] + length) + height step), or turn to (v, h - 1) or (v, h + 1) for fl(d + turn_price).
 * d f32 [8][h][w] is 0 at every target in every layer (arrive facing any way) and the minimum candidate elsewhere; act u8
 * [8][h][w] is 255 at targets, else the first of (drive = 0, turn to h - 1 = 1, turn to h + 1 = 2) whose candidate equals d
 * bitwise. The route follows act from (start, start_heading): turns in place add no node. Targets, start and every other rule as
 * yh_scene_plan_conn with connectivity 8. Synchronous. Errors as yh_scene_plan_conn(.., 8), and YH_EINVAL for a heading outside
 * 0 .. 7, for a turn price that is NaN, infinite or outside [1, 1024], and where (W + H) * (2 * max(H, 101) + 1) + 8 * 1024 >=
 * 2^24. A call refused with YH_EINVAL or YH_ESTATE has touched nothing: an earlier turn plan of the same frame stays readable. A
 * call that fails later (YH_EHIP) leaves no turn plan. The turn plan's buffers (cost 32, action 8, route and turns 20 bytes per
 * pixel) are its own, allocated at the first call on a handle: a plan, a tour and a turn plan do not disturb each other's results. */
int yh_scene_plan_turn(yh_scene* h, const int32_t* targets_xy /* [n][2] or NULL: the frame's balls */, int32_t n_targets,
                       int32_t start_x, int32_t start_y, int32_t start_heading /* 0 .. 7 */, float turn_price /* per 45 degrees */);
/* The last turn plan; any pointer may be NULL. cost f32 [8][h][w], act u8 [8][h][w], path_xy i32 [cap][2] (the pixels visited,
 * start and target included), and per drive step i of the route (*path_len - 1 of them): turns i32 [cap], the signed number of
 * 45-degree steps made at node i before driving (+ towards h + 1; a reversal is -4, never more than 4 either way), and directions
 * f32 [cap][2] = (the drive edge alone, d[h_i][n_i] - d[h_i][n_i+1] with h_i the heading driven; float32((4 - |turns[i]|) * pi /
 * 4), at step 0 too: the start has a heading). YH_EOVERFLOW (and *path_len set, nothing copied) if path_capacity < *path_len
 * while path_xy, directions or turns is asked for; YH_ESTATE before a turn plan, or when a frame was appended since. */
int yh_scene_turn_read(yh_scene* h, float* cost, uint8_t* act, int32_t* path_xy, float* directions, int32_t* turns,
                       int32_t path_capacity, int32_t* path_len);
/* The turn-aware tour (DESIGN.md section 11 "Turn tour"): yh_scene_plan_tour's question - which target first, then which, and the
 * whole route - answered on yh_scene_plan_turn's graph, so that the route can be followed by a drive base. Everything not said here
 * is yh_scene_plan_turn's (states, headings, edge terms, turn_price, the size guard, the action rule, turns and directions) and
 * yh_scene_plan_tour's (K <= YH_TOUR_MAX distinct targets and how they are chosen, all K! orders on the host, the joining). Per
 * target t_b the turn plan's cost field d_b f32 [8][h][w] and action field act_b u8 [8][h][w] with the single target t_b (0 and 255
 * at t_b in all eight layers; K fields solved in the same launches, the edge terms computed once), the label of the nearest target
 * per state, and the leg table with rows r = 0 .. 8 K: row 0 is the state (start, start_heading), row 1 + 8 a + g the state (t_a,
 * g); legs[r][b] = d_b at row r's state, arrive[r][b] = the heading with which the walk along act_b from that state reaches t_b
 * (the row's own heading where its pixel is t_b). An order's total starts from row 0: tot = fl(tot + legs[row][o_j]), then the row
 * becomes that of (t_{o_j}, arrive[row][o_j]) - each leg is the turn plan's route from the state in which the leg before ended,
 * the arrival heading taken as it comes (what chaining yh_scene_plan_turn gives), not optimised over. The order of least total,
 * compared in f32, ties to the lexicographically smallest; its legs' walks joined. Synchronous. Errors as yh_scene_plan_turn and
 * yh_scene_plan_tour together. A call refused with YH_EINVAL or YH_ESTATE has touched nothing: an earlier turn tour of the same
 * frame stays readable. A call that fails later (YH_EHIP, a walk that meets no target included) leaves no turn tour. The buffers
 * (per target 32 bytes of cost, 8 of actions and 40 of route per pixel) are the turn tour's own, allocated at the first call on a
 * handle and sized by the K in use (they only grow): a plan, a tour, a turn plan and a turn tour do not disturb each other's results. */
int yh_scene_plan_turn_tour(yh_scene* h, const int32_t* targets_xy /* [n][2] or NULL: the frame's balls */, int32_t n_targets,
                            int32_t start_x, int32_t start_y, int32_t start_heading /* 0 .. 7 */, float turn_price /* per 45 degrees */);
/* The last turn tour; any pointer may be NULL. With K = *n_targets (<= YH_TOUR_MAX; size the small arrays for YH_TOUR_MAX):
 *   targets_xy   i32 [K][2]      the targets in use, t_0 .. t_{K-1}
 *   order        i32 [K]         the visiting order o: indices into targets_xy
 *   legs         f32 [1+8K][K]   arrive u8 [1+8K][K]: the leg table described above
 *   total        f32             the order's total
 *   leg_headings i32 [K]         the heading with which leg j arrives at t_{o_j} - the heading leg j + 1 starts with
 *   cost         f32 [K][8][h][w], act u8 [K][8][h][w]   field b has the single target t_b
 *   label        u8  [8][h][w]   the smallest b with d_b[g][v] == min over b of d_b[g][v]
 *   path_xy      i32 [cap][2]    the joined route: start .. t_{o_0} .. t_{o_1} .., a junction node once; a leg that starts on its own
 *                                target adds no node and passes its heading on. A pixel may recur across legs: *path_len <= K w h
 *   turns        i32 [cap]       per drive step i (*path_len - 1 of them) the signed 45-degree steps made at node i before driving; at
 *                                a junction counted from the heading the leg before arrived with, in the next leg's action field
 *   directions   f32 [cap][2]    (d_{o_j}[h_i][n_i] - d_{o_j}[h_i][n_i+1], float32((4 - |turns[i]|) * pi / 4)), j the leg of step i
 *   leg_ends     i32 [K]         index in path_xy of the node where leg j ends (t_{o_j})
 * YH_EOVERFLOW (and *path_len set, nothing copied) if path_capacity < *path_len while path_xy, directions or turns is asked for;
 * YH_ESTATE before a turn tour, or when a frame was appended since. */
int yh_scene_turn_tour_read(yh_scene* h, int32_t* n_targets, int32_t* targets_xy, int32_t* order, float* legs, uint8_t* arrive,
                            float* total, int32_t* leg_headings, float* cost, uint8_t* act, uint8_t* label, int32_t* path_xy,
                            float* directions, int32_t* turns, int32_t* leg_ends, int32_t path_capacity, int32_t* path_len);
/* ---- scene memory (DESIGN.md section 11 "Scene memory"): map and balls carried across frames by the robot's motion -----------
 * A yh_scene holds a memory: M, u32 [h][w], and a ball table B[100] of (x, y, count, age) i32, count = 0 meaning empty. It is empty
 * after create and after yh_scene_memory_reset; yh_scene_append, yh_scene_append_classified, yh_scene_set_fields and the planners
 * leave it untouched. yh_scene_append_memory is yh_scene_append_classified(.., YH_COMPAT_SANE) - the same inputs, the same stamps N
 * and frame balls - followed by, all in integers (64-bit intermediates), bit-exact:
 *   carry   for every map pixel (x, y), with gather_q16 = (a, b, c, d, e, f): sx = floor((a x + b y + c + 2^15) / 2^16),
 *           sy = floor((d x + e y + f + 2^15) / 2^16); P = M[sy][sx] inside the frame, else 0; P' = (P * keep) >> 8
 *           (keep 0 .. 256: 256 never fades, 0 keeps nothing);
 *   fuse    F = max(N, P') is the handle's map and the new M; world, connections0 and connections1 are those of a SANE frame
 *           whose height map is F, bit for bit;
 *   balls   carry_q16 (the same formula; it maps a PREVIOUS-map pixel to a current-map pixel, the other direction from
 *           gather_q16). An id the frame sees: B[k] = ((int)mean x, (int)mean y, count, 0), balls[k] the frame's own row. An id it
 *           does not see, with B[k].count > 0 and B[k].age + 1 <= ball_max_age (0 .. 255): (x', y') = carry(B[k].x, B[k].y); the
 *           entry is cleared if |x'| or |y'| >= 2^20, otherwise B[k] = (x', y', count, age + 1) and balls[k] = (x', y', count, age)
 *           as floats - age as it was before this frame - if (x', y') lies inside the frame, zeros if not: a remembered ball
 *           behind the robot stays in B and comes back when the robot turns, and meanwhile takes none of the n_targets of a plan
 *           on the frame's balls. Every other entry is cleared, its balls[k] zeros.
 * Ball ids carry meaning from frame to frame only when they are TRACK ids (yh_instance_track's frames); the ids of
 * yh_instance_frame are per-frame detection indices, and a memory of those joins unrelated balls.
 * Any six int32 values are a valid motion (affine, not only rigid); where it comes from is the caller's business (odometry; without it,
 * yh_scene_append_memory_search below finds it).
 * It counts as a new frame (earlier plans become unreadable) in YH_COMPAT_SANE, and every planner runs on it as on any other.
 * With an empty memory, or keep = 0 and ball_max_age = 0, every output equals yh_scene_append_classified(.., YH_COMPAT_SANE)'s.
 * Asynchronous on the handle's stream; host buffers (depth, a host frame, the two motions) are free again on return.
 * YH_EINVAL with nothing touched, the memory included, for a null pointer, keep outside 0 .. 256 or ball_max_age outside 0 .. 255;
 * a call that fails later (YH_EHIP) leaves no frame and an empty memory. The memory's buffers (three maps) are allocated at the
 * first memory append. */
int yh_scene_append_memory(yh_scene* h, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device,
                           const int32_t* gather_q16 /* [6] */, const int32_t* carry_q16 /* [6] */, int32_t keep, int32_t ball_max_age);
/* The memory as the last memory append left it: map_mem u32 [h][w], balls_mem i32 [100][4] = (x, y, count, age). Either pointer may
 * be NULL. Waits. Zeros before any memory append and after a reset. */
int yh_scene_memory_read(yh_scene* h, uint32_t* map_mem, int32_t* balls_mem /* [100][4] */);
/* Empties the memory (asynchronous on the handle's stream). The last frame's fields and plans stay as they are. */
int yh_scene_memory_reset(yh_scene* h);
/* ---- scene memory: registration (DESIGN.md section 11 "Scene memory: registration"): the motion found on the device -----------
 * yh_scene_append_memory with the motion searched for instead of given: the frame's stamps N are scored against the memory M over
 * candidate motions around a prior, the best is chosen on the device, and the append runs with it - no host wait in between.
 *   candidates  n_rot (1 .. 16) base motions, gather_q16 [n_rot][6] and carry_q16 [n_rot][6], row 0 the prior (the others typically
 *               the prior turned by a few steps either way about the robot's pixel), times the shifts -radius <= u, v <= radius
 *               (radius 0 .. 8). Candidate (k, u, v)'s gather is base k with c += u 65536, f += v 65536 - its source pixel is base
 *               k's plus (u, v) exactly -, its carry base k's (A, B, Cc, D, E, Ff) with Cc -= A u + B v, Ff -= D u + E v.
 *   score       S(k, u, v) = sum over frame pixels (x, y) of min(N[y][x], Q), Q = M[sy + v][sx + u] inside the frame, else 0,
 *               (sx, sy) the source pixel of (x, y) under base k's gather (the carry formula of yh_scene_append_memory); M unfaded.
 *               Exact in 64 bits. sum_n = sum of N bounds every S.
 *   choice      the largest S; ties go to the smaller u^2 + v^2, then the smaller k, then the smaller v, then the smaller u: an
 *               empty memory, an empty frame or a featureless map choose the prior, (0, 0, 0).
 * Then yh_scene_append_memory's steps run with the chosen candidate's twelve integers: every output and the memory equal what that
 * call gives when handed them (yh_scene_motion_read returns them), and the call counts as a memory append in every respect. With
 * n_rot = 1 and radius = 0 it IS yh_scene_append_memory with row 0. Integer only, bit-exact. Asynchronous on the handle's stream;
 * host buffers are free again on return.
 * YH_EINVAL with nothing touched, the memory included, for a null pointer, n_rot or radius out of range, keep or ball_max_age out
 * of yh_scene_append_memory's ranges, or - checked in 64 bits, so that every candidate's coefficients are int32 - unless for every
 * k: |c| + radius 65536 <= INT32_MAX and |f| + radius 65536 <= INT32_MAX on the gather, |Cc| + radius (|A| + |B|) <= INT32_MAX and
 * |Ff| + radius (|D| + |E|) <= INT32_MAX on the carry. A call that fails later (YH_EHIP) leaves no frame and an empty memory. */
int yh_scene_append_memory_search(yh_scene* h, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device, int32_t n_rot,
                                  const int32_t* gather_q16 /* [n_rot][6] */, const int32_t* carry_q16 /* [n_rot][6] */, int32_t radius,
                                  int32_t keep, int32_t ball_max_age);
/* What the last yh_scene_append_memory_search chose: its gather and carry, chosen = (k, u, v), score = (S chosen, S of the prior
 * (0, 0, 0), sum_n), and the whole table scores u64 [n_rot][2 radius + 1][2 radius + 1], indexed [k][v + radius][u + radius]. Any
 * pointer may be NULL. Waits. YH_ESTATE unless the handle's last memory append was a search (a yh_scene_append_memory or a
 * yh_scene_memory_reset since ends that; plain appends and plans do not). */
int yh_scene_motion_read(yh_scene* h, int32_t* gather_q16 /* [6] */, int32_t* carry_q16 /* [6] */, int32_t* chosen /* [3] = k, u, v */,
                         uint64_t* score /* [3] = S chosen, S prior, sum_n */, uint64_t* scores /* [n_rot][2R+1][2R+1] or NULL */);
/* Scene memory: pyramid registration (DESIGN.md section 11 "Scene memory: pyramid registration"): the search made coarse to fine.
 * yh_scene_append_memory_search with a reach of tens of pixels at about the cost of a small search. N and M (unfaded) are pooled into
 * levels 1 .. levels (1 .. 3): level l + 1 is ceil(W_l / 2) x ceil(H_l / 2), a cell the MAX of the up to four cells under it.
 *   level bases  base k's gather (a, b, c, d, e, f) at level l keeps a, b, d, e and has c_l = floor(((a + b - 65536)(2^l - 1) + 2 c)
 *                / 2^(l+1)), f_l likewise from d, e, f (64 bits): the base carried to the centres of the level's cells. Scores at a
 *                level are S of yh_scene_append_memory_search on that level's maps and sizes.
 *   descent      every base (n_rot 1 .. 15) on its own: at the top level the (2 radius + 1)^2 shifts around (0, 0), radius 0 .. 8; at
 *                each level below the (2 refine + 1)^2 shifts, refine 0 .. 8, around TWICE the total shift chosen one level up. Best
 *                of a level: the larger S, then the smaller U^2 + V^2 of the total shift, then the smaller V, then the smaller U.
 *                At level 0 hypothesis n_rot joins: base 0 around (0, 0) - "the prior was right".
 *   choice       over every level-0 entry of all n_rot + 1 hypotheses (hypothesis n_rot counts as k = 0), (u, v) the total shift:
 *                the largest S, then the smaller u^2 + v^2, then the smaller k, then the smaller v, then the smaller u. The chosen
 *                S is S(k, u, v) of the plain search exactly; it is never below the plain search's best for base 0 at radius
 *                refine; an empty memory or an empty frame chooses (0, 0, 0).
 *   reach        T_levels = radius, T_l = 2 T_(l+1) + refine: 71 pixels at levels 3, radius 8, refine 1.
 * The chosen candidate's twelve integers are yh_scene_append_memory_search's for (k, u, v), and everything after the choice is that
 * call's. S is not normalised: on a map dense everywhere a large true shift can lose to "no motion" (DESIGN.md); the home
 * hypothesis makes the outcome there the plain search's. Integer only, bit-exact, no host wait; host buffers are free on return.
 * YH_EINVAL with nothing touched, the memory included, for a null pointer, a parameter out of range, or - in 64 bits - unless for
 * every base and level |c_l| + T_l 65536 <= INT32_MAX and |f_l| + T_l 65536 <= INT32_MAX, and the two carry conditions of
 * yh_scene_append_memory_search hold with T_0 in place of radius. */
int yh_scene_append_memory_pyramid(yh_scene* h, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device, int32_t n_rot,
                                   const int32_t* gather_q16 /* [n_rot][6] */, const int32_t* carry_q16 /* [n_rot][6] */, int32_t levels,
                                   int32_t radius, int32_t refine, int32_t keep, int32_t ball_max_age);
/* One level (0 .. levels) of the last yh_scene_append_memory_pyramid: the centre each hypothesis was scored around, its score
 * table indexed [hyp][V - centre_y + p][U - centre_x + p] with p = radius at the top level and refine below, hyp = n_rot or, at
 * level 0, n_rot + 1, and the sum of the level's N. Any pointer may be NULL. Waits. YH_ESTATE unless the handle's last memory
 * append was a pyramid append; YH_EINVAL for a level outside 0 .. levels. After a pyramid append yh_scene_motion_read returns the
 * gather, carry, chosen and score (S chosen, S(0, 0, 0), sum_n) with scores NULL, and YH_EINVAL naming this call if scores is given. */
int yh_scene_pyramid_read(yh_scene* h, int32_t level, int32_t* centres /* [hyp][2] */, uint64_t* scores /* [hyp][2p+1][2p+1] */, uint64_t* sum_n);
/* Scene memory: normalised registration (DESIGN.md section 11 "Scene memory: normalised registration"): yh_scene_append_memory_search
 * with the choice made by a normalised score, for maps that are dense - a height map stamped at every pixel the camera sees -, where
 * the plain S favours whichever candidate keeps the most pixels inside the frame. Candidates, int32 conditions and refusals are the
 * plain search's. For candidate (k, u, v), over the frame pixels whose source (sx + u, sy + v) lies in the frame ("inside"; the test
 * is made on the 64-bit values), Q = M at that source:
 *   S = sum of min(N, Q) - the plain S exactly -, T = sum of N + Q, C = the number of inside pixels; U = T - S = sum of max(N, Q).
 *   qualified   C >= min_inside (1 .. width x height) and U > 0. The score S / U is 1 wherever the maps agree on their overlap,
 *               however small that is: min_inside is what keeps a sliver of overlap from winning.
 *   choice      among the qualified candidates the largest S / U, compared as exact 128-bit cross products (no division, no float);
 *               ties go to the smaller u^2 + v^2, then the smaller k, then the smaller v, then the smaller u. None qualified (an empty
 *               frame on an empty memory, or every candidate short of min_inside): the prior (0, 0, 0).
 * Everything after the choice is yh_scene_append_memory_search's; with n_rot = 1 and radius = 0 it IS yh_scene_append_memory with
 * row 0. Integer only, bit-exact, no host wait. Afterwards yh_scene_motion_read works as after a plain search (score = S chosen,
 * S(0, 0, 0), sum_n; scores = the S table). YH_EINVAL with nothing touched as there, and for min_inside out of range. */
int yh_scene_append_memory_search_norm(yh_scene* h, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device, int32_t n_rot,
                                       const int32_t* gather_q16 /* [n_rot][6] */, const int32_t* carry_q16 /* [n_rot][6] */, int32_t radius,
                                       int32_t min_inside, int32_t keep, int32_t ball_max_age);
/* What the last yh_scene_append_memory_search_norm saw beside yh_scene_motion_read's: the tables totals (T) and inside (C), u64
 * [n_rot][2 radius + 1][2 radius + 1] laid out as scores there, (S, T, C) of the choice and of (0, 0, 0), and qualified: 0 if no
 * candidate qualified. Any pointer may be NULL. Waits. YH_ESTATE unless the handle's last memory append was a normalised search. */
int yh_scene_motion_norm_read(yh_scene* h, uint64_t* totals /* [n_rot][2R+1][2R+1] or NULL */, uint64_t* inside /* likewise */,
                              uint64_t* chosen_stc /* [3] = S, T, C */, uint64_t* prior_stc /* [3] */, int32_t* qualified);
/* Scene memory: normalised pyramid registration (DESIGN.md section 11 "Scene memory: normalised pyramid registration"):
 * yh_scene_append_memory_pyramid with every level, and the choice, decided by the normalised score of
 * yh_scene_append_memory_search_norm - the reach of the one on the dense maps of the other. Pooled levels, level bases, hypotheses,
 * the home hypothesis, reach, the chosen candidate's twelve integers and the int32 conditions are yh_scene_append_memory_pyramid's.
 *   tables      at level l, S, T and C of yh_scene_append_memory_search_norm on that level's maps, gathers and radius; "inside" is
 *               taken against the level's W_l x H_l.
 *   qualified   at level l: C >= m_l = (min_inside + 4^l - 1) >> 2 l, and U = T - S > 0. min_inside is 1 .. width x height.
 *   descent     per hypothesis, among its qualified entries the largest S / U as exact 128-bit cross products; ties: the smaller
 *               U^2 + V^2 of the total shift, then the smaller V, then the smaller U. None qualified: the hypothesis keeps its
 *               centre (relative shift 0).
 *   choice      over the qualified level-0 entries of all n_rot + 1 hypotheses (hypothesis n_rot counts as k = 0) the largest S / U;
 *               ties: the smaller u^2 + v^2, then k, then v, then u. None qualified: (0, 0, 0) of base 0.
 * The chosen (S, T, C) are the flat normalised search's for that gather; if the prior (0, 0, 0) qualifies the chosen ratio is never
 * below its ratio; an empty memory or an empty frame chooses (0, 0, 0); with n_rot = 1, radius = refine = 0 it IS
 * yh_scene_append_memory with row 0. Integer only, bit-exact, no host wait; host buffers are free on return. Afterwards
 * yh_scene_motion_read and yh_scene_pyramid_read (centres, the S tables, sum_n) work as after yh_scene_append_memory_pyramid, and
 * yh_scene_motion_norm_read returns chosen_stc, prior_stc - (S, T, C) of (0, 0, 0) at the home hypothesis - and qualified with
 * totals and inside NULL (YH_EINVAL naming yh_scene_pyramid_norm_read if either is given). YH_EINVAL with nothing touched as
 * yh_scene_append_memory_pyramid, and for min_inside out of range. */
int yh_scene_append_memory_pyramid_norm(yh_scene* h, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device, int32_t n_rot,
                                        const int32_t* gather_q16 /* [n_rot][6] */, const int32_t* carry_q16 /* [n_rot][6] */, int32_t levels,
                                        int32_t radius, int32_t refine, int32_t min_inside, int32_t keep, int32_t ball_max_age);
/* One level (0 .. levels) of the last yh_scene_append_memory_pyramid_norm: centres, scores (S) and sum_n as yh_scene_pyramid_read
 * returns them, totals (T) and inside (C) laid out as scores, the level's threshold m_l, and per hypothesis whether any of its
 * entries qualified. Any pointer may be NULL. Waits. YH_ESTATE unless the handle's last memory append was a normalised pyramid
 * append; YH_EINVAL for a level outside 0 .. levels. */
int yh_scene_pyramid_norm_read(yh_scene* h, int32_t level, int32_t* centres /* [hyp][2] */, uint64_t* scores /* [hyp][2p+1][2p+1] */,
                               uint64_t* totals /* likewise */, uint64_t* inside /* likewise */, uint64_t* sum_n, int32_t* level_min_inside,
                               int32_t* qualified /* [hyp] */);
/* ---- scene batch (DESIGN.md section 11 "Scene batch"): append and plan N frames in one set of launches -------------
 * Frame b of a batch has EXACTLY the results a yh_scene handle of the same size gives when it is fed that frame alone with the same
 * mode, targets, start and connectivity - bit for bit, every output: the kernels run the single handle's device code with the frame
 * taken from the grid, and the planner's field is unique, so frames that share the solver's rounds cannot change each other.
 * Sizes as yh_scene_create; max_frames 1 .. 256. create allocates the staged inputs and the scene fields of max_frames frames (58
 * bytes per pixel and frame) and builds the bump tables once; the planner's buffers (40, with connectivity 8 56 bytes per pixel and
 * frame) are allocated at the first plan. */
typedef struct yh_scene_batch yh_scene_batch;
int yh_scene_batch_create(int32_t device, int32_t width, int32_t height, int32_t max_frames, yh_scene_batch** out);
void yh_scene_batch_destroy(yh_scene_batch* h);
const char* yh_scene_batch_last_error(const yh_scene_batch* h);
/* Copies one frame into slot `slot` of the handle's own input buffers: depth u16 [h][w] from the host, and the packed u32 frame
 * [h][w] from the host or (frame_on_device = 1) from a device pointer, as yh_scene_append_classified takes it (a (class, id) image
 * packed as class << 24 | id << 16 | id << 8 | class reads the same in both modes). On return the caller's buffers, host or device,
 * are free again: a device source - which must be complete when the call is made, as yh_instance_device_frame and
 * yh_classify_device_frame are - is copied on the handle's stream and waited for, so each can be staged before the next
 * yh_instance_frame / yh_classify_frame_u32 overwrites it. A slot stays staged until it is staged again. YH_EINVAL for a slot
 * outside 0 .. max_frames - 1. */
int yh_scene_batch_stage(yh_scene_batch* h, int32_t slot, const uint16_t* depth_host, const uint32_t* frame, int32_t frame_on_device);
/* yh_scene_batch_stage for slots first_slot .. first_slot + n_frames - 1 at once: depth u16 [n][h][w] from the host and the packed
 * frames u32 [n][h][w] from the host or (frames_on_device = 1) from a device pointer such as yh_instance_batch_device_frames, yh_classify_batch_device_frames or yh_tfl_instance_device_frames. The slot
 * buffers are contiguous, so this is one depth copy and one frame copy on the handle's stream, then the waits yh_scene_batch_stage
 * makes: on return the caller's buffers are free again. The slots are marked staged only on success. YH_EINVAL for n_frames < 1 or a
 * range outside 0 .. max_frames - 1. */
int yh_scene_batch_stage_frames(yh_scene_batch* h, int32_t first_slot, int32_t n_frames, const uint16_t* depth_host /* [n][H][W] */,
                                const uint32_t* frames /* [n][H][W] */, int32_t frames_on_device);
/* Runs frames 0 .. n_frames - 1 as staged, asynchronously on the handle's stream; STRICT and SANE read the frame exactly as
 * yh_scene_append_classified does. YH_EINVAL for n_frames outside 1 .. max_frames or a bad mode, YH_ESTATE (naming the slot) if one
 * of those slots has never been staged. Each append is a new frame generation: an earlier plan becomes unreadable. */
int yh_scene_batch_append(yh_scene_batch* h, int32_t n_frames, int32_t compat_mode);
/* One frame of the last append, laid out as yh_scene_read; any pointer may be NULL. Waits for the frame. YH_ESTATE before an
 * append, YH_EINVAL for frame >= the last n_frames. */
int yh_scene_batch_read(yh_scene_batch* h, int32_t frame, uint32_t* map, float* world, float* conn0, float* conn1, float* balls);
/* yh_scene_plan_conn for every frame of the last append in the same launches: the batch takes the solver rounds of its slowest
 * frame, not their sum. targets_xy: n_targets pixels per frame (all inside the frame, else YH_EINVAL; duplicates allowed), or NULL:
 * each frame's own first n_targets balls by yh_scene_plan's rule (one read-back of the n ball tables; frames may end up with
 * different numbers of targets). starts_xy: every frame's start. status, if not NULL, receives per frame YH_OK, or YH_ESTATE for a
 * frame with no usable ball: that frame gets no plan, the others are planned, and the call returns YH_OK - unless NO frame has a
 * target: then YH_ESTATE. Every other check is yh_scene_plan_conn's (YH_ESTATE after a STRICT append, the size guard, a start
 * outside the frame, a connectivity other than 4 or 8) and YH_EINVAL for starts_xy NULL; they are made for all frames before
 * anything is touched, so a refused call leaves an earlier plan of the same append readable. A call that fails later (YH_EHIP)
 * leaves no plan. Synchronous. */
int yh_scene_batch_plan(yh_scene_batch* h, const int32_t* targets_xy /* [n][n_targets][2] or NULL: each frame's balls */, int32_t n_targets,
                        const int32_t* starts_xy /* [n][2] */, int32_t connectivity /* 4 or 8 */, int32_t* status /* [n] or NULL */);
/* One frame of the last plan, as yh_scene_plan_read (YH_EOVERFLOW with *path_len set included). YH_ESTATE for a frame whose status
 * was YH_ESTATE, before a plan, and after a newer append; YH_EINVAL for a frame outside the last append. */
int yh_scene_batch_plan_read(yh_scene_batch* h, int32_t frame, float* cost, int32_t* next, int32_t* path_xy, float* directions,
                             int32_t path_capacity, int32_t* path_len);
/* yh_scene_plan_tour_conn for every frame of the last append in shared solver rounds (DESIGN.md section 11 "Scene batch: tours"):
 * frame b has exactly the results of yh_scene_plan_tour_conn on a yh_scene of the same size fed that frame alone with the same
 * targets, start and connectivity - every output of yh_scene_tour_read, bit for bit. n_targets (<= YH_TOUR_MAX) is one number per
 * call; frame b uses K_b <= n_targets of them: with targets_xy NULL its first n_targets balls that have pixels, a ball outside the
 * frame or on an earlier ball's pixel dropped; explicit targets must all lie inside the frame and be distinct. targets_xy, starts_xy
 * and status as yh_scene_batch_plan: a frame with no usable ball gets no tour and status[b] = YH_ESTATE, the others are planned and
 * the call returns YH_OK - unless NO frame has a target: then YH_ESTATE. The checks are yh_scene_batch_plan's and the tour's, made
 * for all frames before anything is touched: YH_EINVAL for n_targets < 1 or > YH_TOUR_MAX, starts_xy NULL, a target or start outside
 * the frame, two equal explicit targets in one frame (the text names the frame), a connectivity other than 4 or 8 and the planner's
 * size guard; YH_ESTATE before an append, after a STRICT append, and with connectivity 8 for a frame whose uploaded diagonals allow
 * 4-connected plans only. A refused call leaves an earlier batched tour of the same append readable; a call that fails later
 * (YH_EHIP, a lost walk included: the text names the frame and the leg) leaves none.
 * The tour's buffers are its own, allocated at the first call for max_frames frames x the largest n_targets used so far; they only
 * grow (growing drops the last batched tour). They take 32 bytes per pixel, frame and target (cost 4, next 4, the legs' walks 8,
 * the joined route 16) plus 1 per pixel and frame for the label: 640 x 480 with max_frames = 64 and n_targets = 6 is 3.8 GB - size
 * max_frames and n_targets accordingly. The batch's plan, tour, turn plan and turn tour do not disturb each other's results. Beyond
 * the solver's batches of rounds, one wait per call, whatever n. Synchronous. */
int yh_scene_batch_plan_tour(yh_scene_batch* h, const int32_t* targets_xy /* [n][n_targets][2] or NULL */, int32_t n_targets,
                             const int32_t* starts_xy /* [n][2] */, int32_t connectivity /* 4 or 8 */, int32_t* status /* [n] or NULL */);
/* One frame of the last batched tour, as yh_scene_tour_read (YH_EOVERFLOW with *path_len set and nothing copied included).
 * YH_ESTATE for a frame whose status was YH_ESTATE, before a batched tour, and after a newer append; YH_EINVAL for a frame outside
 * the last append. */
int yh_scene_batch_tour_read(yh_scene_batch* h, int32_t frame, int32_t* n_targets, int32_t* targets_xy, int32_t* order, float* legs,
                             float* total, float* cost, int32_t* next, uint8_t* label, int32_t* path_xy, float* directions,
                             int32_t* leg_ends, int32_t path_capacity, int32_t* path_len);
/* yh_scene_plan_turn for every frame of the last append in shared solver rounds (DESIGN.md section 11 "Scene batch: turns"): frame b
 * has exactly the results of yh_scene_plan_turn on a yh_scene fed that frame alone with the same targets, start, start heading and
 * turn price - cost, act, route, turns and directions, bit for bit. targets_xy, n_targets, starts_xy and status as
 * yh_scene_batch_plan; start_headings: every frame's start heading, 0 .. 7; turn_price: one price per call (a property of the drive
 * base, not of the frame). The checks are yh_scene_plan_turn's, made for all frames before anything is touched: YH_EINVAL for
 * starts_xy or start_headings NULL, a heading outside 0 .. 7 (the text names the frame), a turn price that is NaN, infinite or
 * outside [1, 1024], a target or start outside the frame, n_targets < 1 and the turn planner's size guard; YH_ESTATE before an
 * append, after a STRICT append, for a frame whose uploaded diagonals allow 4-connected plans only, and when no frame has a target.
 * A refused call leaves an earlier turn plan of the same append readable; a call that fails later (YH_EHIP) leaves none. The turn
 * plan's buffers (60 bytes per pixel and frame, for max_frames frames) are its own, allocated at the first call: the batch's plan
 * and its turn plan do not disturb each other's results. Synchronous. */
int yh_scene_batch_plan_turn(yh_scene_batch* h, const int32_t* targets_xy /* [n][n_targets][2] or NULL */, int32_t n_targets,
                             const int32_t* starts_xy /* [n][2] */, const int32_t* start_headings /* [n], 0 .. 7 */,
                             float turn_price, int32_t* status /* [n] or NULL */);
/* One frame of the last batched turn plan, as yh_scene_turn_read (YH_EOVERFLOW with *path_len set included). YH_ESTATE for a frame
 * whose status was YH_ESTATE, before a turn plan, and after a newer append; YH_EINVAL for a frame outside the last append. */
int yh_scene_batch_turn_read(yh_scene_batch* h, int32_t frame, float* cost, uint8_t* act, int32_t* path_xy, float* directions,
                             int32_t* turns, int32_t path_capacity, int32_t* path_len);
/* yh_scene_plan_turn_tour for every frame of the last append in shared solver rounds (DESIGN.md section 11 "Scene batch: turn
 * tours"): frame b has exactly the results of yh_scene_plan_turn_tour on a yh_scene fed that frame alone with the same targets, start,
 * start heading and turn price - every output of yh_scene_turn_tour_read, bit for bit. n_targets (<= YH_TOUR_MAX) is one number per
 * call; frame b uses K_b <= n_targets of them: with targets_xy NULL its first n_targets balls that have pixels, a ball on an earlier
 * ball's pixel dropped; a frame with no usable ball gets no tour and status[b] = YH_ESTATE, the others are planned. starts_xy,
 * start_headings, turn_price and status as yh_scene_batch_plan_turn. The checks are yh_scene_batch_plan_turn's and the tour's, made
 * for all frames before anything is touched: YH_EINVAL also for n_targets > YH_TOUR_MAX and for two equal explicit targets in one
 * frame (the text names the frame). A refused call leaves an earlier batched turn tour of the same append readable; a call that
 * fails later (YH_EHIP: a lost chase or walk, the text names the frame and the entry or leg) leaves none.
 * The turn tour's buffers are its own, allocated at the first call for max_frames frames x the largest n_targets used so far; they
 * only grow (growing drops the last batched turn tour). They take 80 bytes per pixel, frame and target (cost 32, act 8, the legs'
 * walks 20, the joined route 20) plus 8 per pixel and frame for the label: 640 x 480 with max_frames = 64 and n_targets = 6 is
 * 9.6 GB - size max_frames and n_targets accordingly. The batch's plan, tour, turn plan and turn tour do not disturb each other's
 * results. Two waits per call, whatever n. Synchronous. */
int yh_scene_batch_plan_turn_tour(yh_scene_batch* h, const int32_t* targets_xy /* [n][n_targets][2] or NULL */, int32_t n_targets,
                                  const int32_t* starts_xy /* [n][2] */, const int32_t* start_headings /* [n], 0 .. 7 */,
                                  float turn_price, int32_t* status /* [n] or NULL */);
/* One frame of the last batched turn tour, as yh_scene_turn_tour_read (YH_EOVERFLOW with *path_len set and nothing copied included).
 * YH_ESTATE for a frame whose status was YH_ESTATE, before a batched turn tour, and after a newer append; YH_EINVAL for a frame
 * outside the last append. */
int yh_scene_batch_turn_tour_read(yh_scene_batch* h, int32_t frame, int32_t* n_targets, int32_t* targets_xy, int32_t* order, float* legs,
                                  uint8_t* arrive, float* total, int32_t* leg_headings, float* cost, uint8_t* act, uint8_t* label,
                                  int32_t* path_xy, float* directions, int32_t* turns, int32_t* leg_ends, int32_t path_capacity,
                                  int32_t* path_len);
/* ---- scene batch: memory (DESIGN.md section 11 "Scene batch: memory"): a memory per camera stream, carried in the batch ----------
 * A yh_scene_batch holds a bank of YH_SCENE_STREAMS_MAX memories, each what a yh_scene holds ("scene memory" above: a map M u32
 * [h][w] and a ball table B[100] of (x, y, count, age)), each empty after create and after a reset. yh_scene_batch_append_memory on
 * slots 0 .. n_frames - 1 as staged is EXACTLY this: for b = 0 .. n_frames - 1 in order, a yh_scene_append_memory call on a yh_scene
 * of the same size that holds the memory of streams[b], fed slot b's depth and packed frame, gather_q16[b], carry_q16[b], keep and
 * ball_max_age. Frame b's map, world, connections0, connections1 and balls are that call's (yh_scene_batch_read), every stream named
 * in the call ends in the state those calls leave, a stream not named is untouched, and batched calls on a stream continue each other
 * from call to call. keep and ball_max_age are one value per call (properties of the robot, as turn_price is). The step itself is
 * the one defined in the "scene memory" section; nothing about it is redefined here. Ball ids carry meaning across frames only as
 * TRACK ids: the batched producer is yh_instance_track_batch, whose streams are these streams.
 * Frames of different streams share launches; frames of one stream form a chain on the device: with R the most frames one stream has
 * in the call, R + 5 launches, whatever n. It counts as a YH_COMPAT_SANE append of n_frames frames (earlier plans become unreadable,
 * all four batched planners run on the fused frames; with targets_xy NULL a remembered ball inside the frame is a target by the
 * usual rule, one outside the frame is not). yh_scene_batch_append and yh_scene_batch_set_fields leave the bank alone.
 * Checks, for every frame before anything is touched: YH_EINVAL for a null handle or null motion arrays, n_frames outside
 * 1 .. max_frames, keep outside 0 .. 256, ball_max_age outside 0 .. 255, a stream outside the bank (the text names the frame);
 * YH_ESTATE, naming the slot, for a slot that was never staged. A refused call leaves frames, plans and every memory as they were; a
 * call that fails later (YH_EHIP) leaves no frame and empties the memories of the streams it named. Asynchronous on the handle's
 * stream; the caller's arrays are free again on return. The stamps' own array (4 bytes per pixel and frame) is allocated at the first
 * memory append, a stream's two maps and two tables (8 bytes per pixel and stream: 157 MB for 64 streams at 640 x 480) at its first use. */
#define YH_SCENE_STREAMS_MAX 64
int yh_scene_batch_append_memory(yh_scene_batch* h, int32_t n_frames,
                                 const int32_t* streams /* [n], each 0 .. YH_SCENE_STREAMS_MAX - 1, or NULL: all 0 */,
                                 const int32_t* gather_q16 /* [n][6] */, const int32_t* carry_q16 /* [n][6] */,
                                 int32_t keep, int32_t ball_max_age);
/* The memory of one stream as the last call that named it left it, laid out as yh_scene_memory_read; either pointer may be NULL.
 * Waits. Zeros for a stream never used or reset. YH_EINVAL for a stream outside the bank. */
int yh_scene_batch_memory_read(yh_scene_batch* h, int32_t stream, uint32_t* map_mem, int32_t* balls_mem /* [100][4] */);
/* The ball table of frame `frame`'s stream right after that frame of the last memory append. YH_ESTATE unless the current frames came
 * from yh_scene_batch_append_memory, YH_EINVAL for a frame outside it. Waits. */
int yh_scene_batch_memory_frame_balls(yh_scene_batch* h, int32_t frame, int32_t* balls_mem /* [100][4] */);
/* Empties the memory of one stream, or of all (stream = -1); asynchronous on the handle's stream. The current frames and plans stay
 * as they are. YH_EINVAL for a stream outside the bank. */
int yh_scene_batch_memory_reset(yh_scene_batch* h, int32_t stream /* -1: all */);
/* ---- scene batch: registration (DESIGN.md section 11 "Scene batch: registration"): each stream's motion found on the device -----
 * yh_scene_batch_append_memory with every frame's motion searched for instead of given. On slots 0 .. n_frames - 1 as staged it is
 * EXACTLY this: for b = 0 .. n_frames - 1 in order, a yh_scene_append_memory_search call on a yh_scene of the same size that holds
 * the memory of streams[b], fed slot b's depth and packed frame, the n_rot bases of row b (gather_q16[b], carry_q16[b]), radius, keep
 * and ball_max_age. Frame b's five outputs, its ball table (yh_scene_batch_memory_frame_balls), every named stream's final memory,
 * and frame b's chosen (k, u, v), twelve coefficients, three scores and whole score table (yh_scene_batch_motion_read) are that
 * call's, bit for bit. So frame r of a stream is scored against the memory frame r - 1 of that stream has just fused, on the device:
 * with R the most frames one stream has in the call, 3 R + 6 launches, whatever n, and no host wait. n_rot, radius, keep and
 * ball_max_age are one value per call. Candidates, score, tie rule and int32 conditions are those of the "scene memory:
 * registration" section; nothing is redefined here. With n_rot = 1 and radius = 0 it IS yh_scene_batch_append_memory with the same
 * motions. It counts as a memory append of n_frames frames in every respect (earlier plans become unreadable, all four batched
 * planners run on the fused frames, yh_scene_batch_memory_read, _memory_frame_balls and _memory_reset work as after it).
 * Checks, for every frame before anything is touched: every check of yh_scene_batch_append_memory; YH_EINVAL for n_rot outside
 * 1 .. 16 or radius outside 0 .. 8, and unless the four int32 conditions hold for every frame and base (the text names both). A
 * refused call leaves frames, plans, memories and the last readable motions as they were; a call that fails later behaves as
 * yh_scene_batch_append_memory does. Asynchronous on the handle's stream; the caller's arrays are free again on return. The score
 * tables and records (max_frames x (37000 + 88) bytes: 9.5 MB for 256 frames) are allocated at the first batched search. */
int yh_scene_batch_append_memory_search(yh_scene_batch* h, int32_t n_frames, const int32_t* streams /* [n] or NULL */,
                                        int32_t n_rot, const int32_t* gather_q16 /* [n][n_rot][6] */,
                                        const int32_t* carry_q16 /* [n][n_rot][6] */, int32_t radius,
                                        int32_t keep, int32_t ball_max_age);
/* What the last yh_scene_batch_append_memory_search chose for frame `frame`, laid out as yh_scene_motion_read; any pointer may be
 * NULL. Waits. YH_ESTATE unless the current frames came from a batched search append, YH_EINVAL for a frame outside it. */
int yh_scene_batch_motion_read(yh_scene_batch* h, int32_t frame, int32_t* gather_q16, int32_t* carry_q16,
                               int32_t* chosen, uint64_t* score, uint64_t* scores);
/* ---- scene batch: pyramid registration (DESIGN.md section 11 "Scene batch: pyramid registration"): the search coarse to fine ------
 * yh_scene_batch_append_memory_search with every frame's motion searched for coarse to fine over a map pyramid. On slots
 * 0 .. n_frames - 1 as staged it is EXACTLY this: for b = 0 .. n_frames - 1 in order, a yh_scene_append_memory_pyramid call on a
 * yh_scene of the same size that holds the memory of streams[b], fed slot b's depth and packed frame, the n_rot bases of row b, levels,
 * radius, refine, keep and ball_max_age. Frame b's five outputs, its ball table, every named stream's final memory, frame b's chosen
 * (k, u, v), twelve coefficients and three scores (yh_scene_batch_motion_read) and every level's centres and score tables
 * (yh_scene_batch_pyramid_read) are that call's, bit for bit. Frame r of a stream is registered against the memory frame r - 1 of
 * that stream has just fused - both maps are pooled round by round on the device: with R the most frames one stream has in the call,
 * R (2 levels + 4) + 5 launches, whatever n, and no host wait. n_rot (1 .. 15), levels (1 .. 3), radius and refine (0 .. 8), keep and
 * ball_max_age are one value per call. Levels, level bases, descent, choice, reach and int32 conditions are those of the "scene
 * memory: pyramid registration" section; nothing is redefined here. It counts as a memory append of n_frames frames in every respect,
 * as yh_scene_batch_append_memory_search does.
 * Checks, for every frame before anything is touched: every check of yh_scene_batch_append_memory; YH_EINVAL for a parameter outside
 * its range, and unless the int32 conditions of yh_scene_append_memory_pyramid hold for every frame, base and level (the text names
 * the frame, the base and, where a coarse level alone refuses, the level). A refused call leaves frames, plans, memories, the last
 * readable motions and level tables as they were; a call that fails later behaves as yh_scene_batch_append_memory does. Asynchronous
 * on the handle's stream; the caller's arrays are free again on return. The pooled levels (2 x 4 bytes x the 21 / 64 of a frame's
 * pixels that levels 1 .. 3 have: 0.8 MB per frame at 640 x 480), the level tables (148 KB per frame), tables of level bases and
 * records of max_frames frames are allocated at the first batched pyramid append. */
int yh_scene_batch_append_memory_pyramid(yh_scene_batch* h, int32_t n_frames, const int32_t* streams /* [n] or NULL */,
                                         int32_t n_rot, const int32_t* gather_q16 /* [n][n_rot][6] */,
                                         const int32_t* carry_q16 /* [n][n_rot][6] */, int32_t levels, int32_t radius,
                                         int32_t refine, int32_t keep, int32_t ball_max_age);
/* One level (0 .. levels) of what the last yh_scene_batch_append_memory_pyramid did for frame `frame`, laid out as
 * yh_scene_pyramid_read; any pointer may be NULL. Waits. YH_ESTATE unless the last memory append of the batch was a pyramid append
 * whose frames are the current ones (a memory reset since ends that too); YH_EINVAL for a frame outside it or a level outside
 * 0 .. levels. After a pyramid append yh_scene_batch_motion_read returns the gather, carry, chosen and score with scores NULL, and
 * YH_EINVAL naming this call if scores is given. */
int yh_scene_batch_pyramid_read(yh_scene_batch* h, int32_t frame, int32_t level, int32_t* centres /* [hyp][2] */,
                                uint64_t* scores /* [hyp][2p+1][2p+1] */, uint64_t* sum_n);
/* ---- batched normalised registration (DESIGN.md section 11 "Scene batch: normalised registration") --------------------------------
 * yh_scene_batch_append_memory_search with the candidates ranked by the normalised score of the "scene memory: normalised
 * registration" section, as a dense height map needs. On slots 0 .. n_frames - 1 as staged it is EXACTLY this: for
 * b = 0 .. n_frames - 1 in order, a yh_scene_append_memory_search_norm call on a yh_scene of the same size that holds the memory of
 * streams[b], fed slot b's depth and packed frame, the n_rot bases of row b, radius, min_inside, keep and ball_max_age. Frame b's five
 * outputs, its ball table, every named stream's final memory, frame b's chosen (k, u, v), twelve coefficients, three scores and S
 * table (yh_scene_batch_motion_read) and its T and C tables, (S, T, C) of the choice and of the prior and `qualified`
 * (yh_scene_batch_motion_norm_read) are that call's, bit for bit. Frame r of a stream is scored against the memory frame r - 1 of
 * that stream has just fused, on the device: with R the most frames one stream has in the call, 3 R + 6 launches, as the plain batched
 * search, and no host wait. n_rot, radius, min_inside (1 .. width x height), keep and ball_max_age are one value per call. Score,
 * qualification, choice, tie rule and int32 conditions are the single handle's; nothing is redefined here. With n_rot = 1 and
 * radius = 0 it IS yh_scene_batch_append_memory with the same motions. It counts as a memory append of n_frames frames in every
 * respect, as yh_scene_batch_append_memory_search does.
 * Checks, for every frame before anything is touched: every check of yh_scene_batch_append_memory_search, with its texts; YH_EINVAL
 * for min_inside out of range. A refused call leaves frames, plans, memories and the last readable motions and tables as they were;
 * a call that fails later behaves as yh_scene_batch_append_memory does. Asynchronous on the handle's stream; the caller's arrays are
 * free again on return. The tables (three times the plain search's: 110 984 bytes per frame), records (88 bytes) and extensions
 * (56 bytes) of max_frames frames are allocated at the first batched normalised search: 28.4 MB for 256 frames. */
int yh_scene_batch_append_memory_search_norm(yh_scene_batch* h, int32_t n_frames, const int32_t* streams /* [n] or NULL */,
                                             int32_t n_rot, const int32_t* gather_q16 /* [n][n_rot][6] */,
                                             const int32_t* carry_q16 /* [n][n_rot][6] */, int32_t radius, int32_t min_inside,
                                             int32_t keep, int32_t ball_max_age);
/* What yh_scene_batch_motion_read leaves out after the last yh_scene_batch_append_memory_search_norm, for frame `frame`, laid out
 * as yh_scene_motion_norm_read; any pointer may be NULL. Waits. YH_ESTATE unless the current frames came from a batched normalised
 * append, YH_EINVAL for a frame outside it. After yh_scene_batch_append_memory_pyramid_norm it returns chosen_stc, prior_stc and
 * qualified with totals and inside NULL, and YH_EINVAL naming yh_scene_batch_pyramid_norm_read if either is given. */
int yh_scene_batch_motion_norm_read(yh_scene_batch* h, int32_t frame, uint64_t* totals, uint64_t* inside,
                                    uint64_t* chosen_stc /* [3] */, uint64_t* prior_stc /* [3] */, int32_t* qualified);
/* ---- batched normalised pyramid registration (DESIGN.md section 11 "Scene batch: normalised pyramid registration") ---------------
 * yh_scene_batch_append_memory_pyramid with every level, and the choice, decided by the normalised score. On slots
 * 0 .. n_frames - 1 as staged it is EXACTLY this: for b = 0 .. n_frames - 1 in order, a yh_scene_append_memory_pyramid_norm call on
 * a yh_scene of the same size that holds the memory of streams[b], fed slot b's depth and packed frame, the n_rot bases of row b,
 * levels, radius, refine, min_inside, keep and ball_max_age. Frame b's five outputs, its ball table, every named stream's final
 * memory, its chosen (k, u, v), twelve coefficients and three scores (yh_scene_batch_motion_read with scores NULL), (S, T, C) of
 * the choice and of the prior and `qualified` (yh_scene_batch_motion_norm_read) and every level's centres, S, T and C tables, sum_n,
 * threshold m_l and per-hypothesis flags (yh_scene_batch_pyramid_norm_read; centres, S and sum_n through yh_scene_batch_pyramid_read
 * too) are that call's, bit for bit. With R the most frames one stream has in the call, R (2 levels + 4) + 5 launches, as the plain
 * batched pyramid, and no host wait. Levels, descent, thresholds, choice, reach and int32 conditions are those of the "scene
 * memory: normalised pyramid registration" section; nothing is redefined here. With n_rot = 1 and radius = refine = 0 it IS
 * yh_scene_batch_append_memory with the same motions.
 * Checks, for every frame before anything is touched: every check of yh_scene_batch_append_memory_pyramid, with its texts;
 * YH_EINVAL for min_inside out of range. A refused call leaves frames, plans, memories, the last readable motions and level tables
 * as they were; a call that fails later behaves as yh_scene_batch_append_memory does. Asynchronous on the handle's stream. The
 * level tables (three times the plain pyramid's: 443 936 bytes per frame), the flags (256 bytes per frame), the pooled levels,
 * tables of level bases, records and extensions of max_frames frames are allocated at the first batched normalised pyramid append:
 * 113.6 MB of level tables for 256 frames, beside the plain batched pyramid's 0.8 MB of pooled levels per frame at 640 x 480. */
int yh_scene_batch_append_memory_pyramid_norm(yh_scene_batch* h, int32_t n_frames, const int32_t* streams /* [n] or NULL */,
                                              int32_t n_rot, const int32_t* gather_q16 /* [n][n_rot][6] */,
                                              const int32_t* carry_q16 /* [n][n_rot][6] */, int32_t levels, int32_t radius,
                                              int32_t refine, int32_t min_inside, int32_t keep, int32_t ball_max_age);
/* One level (0 .. levels) of what the last yh_scene_batch_append_memory_pyramid_norm did for frame `frame`, laid out as
 * yh_scene_pyramid_norm_read; any pointer may be NULL. Waits. YH_ESTATE unless the last memory append of the batch was a normalised
 * pyramid append whose frames are the current ones (a memory reset since ends that too); YH_EINVAL for a frame outside it or a level
 * outside 0 .. levels. */
int yh_scene_batch_pyramid_norm_read(yh_scene_batch* h, int32_t frame, int32_t level, int32_t* centres /* [hyp][2] */,
                                     uint64_t* scores, uint64_t* totals, uint64_t* inside /* [hyp][2p+1][2p+1] each */,
                                     uint64_t* sum_n, int32_t* level_min_inside, int32_t* qualified /* [hyp] */);
/* Device copy of the frame the last yh_classify_frame_u32 produced (valid until the next classify on this handle). */
const uint32_t* yh_classify_device_frame(const yh_engine* h);

#ifdef __cplusplus
}
#endif
#endif /* YOLACT_HIP_H */
