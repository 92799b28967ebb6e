/*
 * yolact_hip_debug.h - measurement, study and test surface of libyolact_hip.so: the named fields of yh_tuning, yh_set_tuning /
 * yh_get_tuning, the profiling hooks bench.py uses, the single-op entry points the parity tests call, the yh_debug_* hooks.
 * NOT part of the drop-in boundary (include/yolact_hip.h): a host that replaces src/yolact.rs needs none of it, and the C++ host
 * mirror (tiny-object-detection_amd/host/) compiles against yolact_hip.h alone. Include THIS header instead of yolact_hip.h to get
 * both; the struct it defines has the layout of the public header's opaque `yh_tuning { int32_t knob[32]; }`.
 */
#ifndef YOLACT_HIP_DEBUG_H
#define YOLACT_HIP_DEBUG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YH_TUNING_DEFINED
/* Measurement and test knobs of ONE handle. Every field: -1 = the library's default.
 * None of them changes results beyond the stated f16 tolerance (most are bit-equivalent); they exist so that tests
 * can reach every plan with small tensors and check one form against another. A field no test sets does not exist
 * (tests/test_abi.py guards it): the launch planner's own thresholds are constants beside it (csrc/engine.hip).
 * There are no process-global switches: the library reads no environment variable. */
typedef struct yh_tuning {
    int32_t plan_cus;        /* CU count the launch plans assume (default: the device's multiProcessorCount) */
    int32_t chsplit;         /* 256 + 128 channel split of the 384-channel head (1) */
    int32_t upfuse;          /* FPN top-down upsamples evaluated in the lateral conv's epilogue instead of a kernel and a
                              * tensor of their own (1); creation time only */
    int32_t ablate;          /* timing only (results are garbage): bit 0 / bit 1 drop the activation / weight stream (zero-record
                              * descriptors: the loads issue, nothing moves), bit 2 issues no loader instruction at all */
    int32_t op_tile;         /* single-op entry points: force this ConvTile id (-1: the engine's choice) */
    int32_t op_kslices;      /* single-op entry points: force a split-K with this many slices */
    int32_t tfl_dot;         /* TFLite path (yh_tfl handles only), CONV_2D: 0 one lane per output element, 1 the v_dot4 kernel (Ci % 4 == 0),
                              * 2 also the int8 MFMA kernel on 64 x 64 LDS tiles where Ci % 64 == 0, 3 (default) the int8 MFMA kernel fed from
                              * registers - one wave per 16 x 16 tile of v_mfma_i32_16x16x64_i8, no LDS, a ring of 1-18 k-steps of loads in
                              * flight - where Ci % 4 == 0 (large long-K layers keep the LDS tiles); all four give the same bytes */
    int32_t tfl_graph;       /* TFLite path: 0 eager launches (default, and the faster form: 0.33 vs 0.37 ms per invoke of the 136-op
                              * model), 1 hipGraph replay of the plan (captured with a second, one-node branch: DESIGN.md §8) */
    int32_t tailfork;        /* the detection tail's K1-K3 on a second stream underneath the protonet (1); 0 keeps them on
                              * the main stream */
    int32_t dsfuse;          /* a stage's projection shortcut evaluated inside the block's last 1x1 conv (two-source K, 1);
                              * creation time only */
    int32_t headfork_maxb;   /* batches up to this size run the prediction head (and the tail's K1-K3) on the second stream
                              * beside the protonet (default: every batch size); 0: never (the tail's K1-K3 alone fork) */
    int32_t protofuse;       /* the 1x1 conv that makes the 32 prototypes evaluated in the epilogue of the 3x3 conv in front of it
                              * wherever that one runs as single 256 x 256-tile launches (1); creation time only */
    int32_t chain;           /* identity bottleneck blocks of layers 1-2 as ONE launch each: 3x3 conv + 1x1 expand conv with the residual
                              * add + the next block's 1x1 reduce conv (csrc/bneck.hip; bit-identical to the separate launches). Bit 0
                              * on; bit 4 also fuse launches that only fill 64-pixel tiles (small batches: 3 % faster at batch 1-8).
                              * Default 17 (bits 0 and 4). Test switches: bit 1 layer 3's expand + next-reduce launch (bneck_xn_f16)
                              * wherever it is eligible instead of only inside its window (64-pixel tiles filling more than half a round
                              * of workgroups and at most one), bit 5 layer 1 only, bit 6 without the fused form of layer 1's FIRST block
                              * (projection shortcut), bit 7 without layer 3's launch. Bits 2-3 (round 3's persistent grid and phase
                              * stagger) are retired and ignored */
    int32_t tfl_fuse;        /* TFLite path: 1 (default) element-wise operators (QUANTIZE / RELU / RELU6 / TANH / ADD), PAD and contiguous
                              * CONCATENATION parts folded into the launch of the convolution / resize that produces their operand -
                              * same bytes, fewer launches; 0: one launch per operator, every tensor materialised (the checker) */
    int32_t tfl_group;       /* TFLite path: 1 (default) independent register-fed convolutions of one kernel form at one depth of the plan's
                              * graph as ONE launch (the prediction head's convolutions over the pyramid levels: 23 launches become 3), the
                              * plan in depth order; 0: one launch per convolution in file order. Same bytes */
    int32_t op_xgap;         /* single-op conv entry points: the staged input keeps this many extra f16 elements (a multiple of 8,
                              * filled with NaN, 0x7E00) behind every image, so x_img_stride is not the dense H * W * C (0: dense) */
    int32_t op_tanh_from;    /* single-op conv entry points with act = 2: tanh on the channels from this one on (0: all of them) */
    int32_t reserved[15];    /* ignored by the library (the slots of retired fields: DESIGN.md §9) */
} yh_tuning;

#ifdef __cplusplus
}
#endif

typedef char yh_tuning_has_the_public_headers_size[sizeof(yh_tuning) == 32 * sizeof(int32_t) ? 1 : -1];

#include "yolact_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Replaces the run-time tuning fields of a live handle (captured graphs are dropped and re-captured on the next
 * call); YH_ESTATE if a creation-time field (upfuse, dsfuse, protofuse) differs from the handle's. */
int yh_set_tuning(yh_engine* h, const yh_tuning* tune);
/* The handle's tuning with every default resolved (plan_cus = the CU count the plans really use, ...). The tfl_* fields belong to
 * yh_tfl handles (yh_tfl_create_tuned) and stay -1: an engine handle does not carry them. */
int yh_get_tuning(const yh_engine* h, yh_tuning* out);

/* ---- measurement hooks (bench.py; not part of the reference surface) ------------------------ */

/* Number of kernel launches in one forward(+tail if with_tail) for the current batch. */
int yh_profile_launch_count(const yh_engine* h, int32_t with_tail);
/* Runs `reps` forwards with a hipEvent pair around every launch on the handle's own stream and
 * writes, per launch: mean milliseconds, algorithmic FLOPs and algorithmic bytes, and a static
 * name ("kernel_symbol:layer"). Arrays must hold yh_profile_launch_count entries. */
int yh_profile_run(yh_engine* h, int32_t with_tail, int32_t reps, float* ms, double* flops,
                   double* bytes, const char** names);
/* Times `steps` back-to-back yh_evaluate (or yh_invoke if !with_tail) calls with one hipEvent
 * pair on the handle's stream; returns total milliseconds in *ms_total. */
int yh_time_steps(yh_engine* h, int32_t with_tail, int32_t steps, float* ms_total);
/* Algorithmic conv FLOPs of one frame for this architecture (2 x MAC, convs only). */
double yh_flops_per_frame(const yh_engine* h);

/* Same with the TFLite fields of a tuning struct (tfl_dot, tfl_graph, tfl_fuse, tfl_group; tune may be NULL). */
int yh_tfl_create_tuned(const void* model_bytes, size_t nbytes, int32_t device, const yh_tuning* tune, yh_tfl** out);
/* yh_tfl_create_batch with the same fields. */
int yh_tfl_create_batch_tuned(const void* model_bytes, size_t nbytes, int32_t device, int32_t max_images, const yh_tuning* tune, yh_tfl** out);

/* Kernel launches per invoke of the prepared plan; how many are CONV_2D and how many of those run on the int8 matrix pipes. */
int yh_tfl_plan_info(const yh_tfl* h, int32_t* launches, int32_t* conv_launches, int32_t* conv_mfma_launches);

/* Test hooks: which kernel every operator of a plan runs on (tests/test_gpu_tflite_forms.py asserts it case by case).
 * yh_tfl_direct_forms: the rows of the register-fed int8 convolution's table of forms - returns their number and writes (D, once, KK)
 * of the first `cap` rows to rows[3 * i ..] (rows may be NULL). No handle, no device: a CPU test calls it.
 * yh_tfl_op_info: operator `op` of the model (file order) in the handle's plan, for the image count of the next invoke: its kernel
 * family (below; the answer of the same functions the launches ask), the row of the table of forms it runs (-1: not register-fed),
 * whether it is launched as a member of a group, and whether it is folded into another launch (then it has no launch of its own;
 * a RESHAPE that shares its input's buffer reports YH_TFL_FAM_NONE, folded). Any of the four pointers may be NULL.
 * yh_tfl_op_quant: the type of the operator's output - 0 uint8, 1 int8, -1 any other - and whether it is an int8 convolution whose
 * weights carry one scale per output channel (its launch reads a multiplier table either way; with a single scale the entries are
 * equal and 0 is reported). Both pointers may be NULL. */
enum {
    YH_TFL_FAM_NONE = -1,
    YH_TFL_FAM_CONV_SCALAR = 0, YH_TFL_FAM_CONV_PX8 = 1, YH_TFL_FAM_CONV_DOT1 = 2, YH_TFL_FAM_CONV_DOT4 = 3,
    YH_TFL_FAM_CONV_I8_LDS = 4, YH_TFL_FAM_CONV_I8_DIRECT = 5, YH_TFL_FAM_DW_SCALAR = 6, YH_TFL_FAM_DW_C4 = 7,
    YH_TFL_FAM_ADD = 8, YH_TFL_FAM_REQUANT = 9, YH_TFL_FAM_QUANTIZE_F32 = 10, YH_TFL_FAM_DEQUANTIZE = 11, YH_TFL_FAM_LUT = 12,
    YH_TFL_FAM_PAD = 13, YH_TFL_FAM_RESIZE = 14, YH_TFL_FAM_CONCAT = 15, YH_TFL_FAM_COPY = 16
};
int yh_tfl_direct_forms(int32_t* rows, int32_t cap);
int yh_tfl_op_info(const yh_tfl* h, int32_t op, int32_t* family, int32_t* form_row, int32_t* grouped, int32_t* folded);
int yh_tfl_op_quant(const yh_tfl* h, int32_t op, int32_t* signed_act, int32_t* per_channel);

int yh_tfl_tensor_count(const yh_tfl* h);

int yh_tfl_tensor_read(yh_tfl* h, int32_t tensor, void* dst, size_t nbytes);   /* test hook: any tensor by index */

/* Measurement hook: mean device milliseconds per frame over `reps` re-runs of the last appended frame, with the inputs and
 * the compat mode of that append (a device frame given to yh_scene_append_classified must still be valid). The re-runs
 * overwrite the outputs with the same values. */
int yh_scene_time(yh_scene* h, int32_t reps, float* ms_per_frame);
/* The same for a frame that came from yh_scene_append_memory (yh_scene_time refuses such a frame with YH_ESTATE and names this
 * hook): its launches - stamps, ball memory, fuse - replayed with its inputs and motions on the memory as it was BEFORE that
 * append, so the re-runs rewrite the outputs and the memory with the same values and commit nothing. YH_ESTATE unless the
 * handle's last frame is a memory append (a plain append, yh_scene_set_fields or yh_scene_memory_reset since ends that). */
int yh_scene_memory_time(yh_scene* h, int32_t reps, float* ms_per_frame);
/* The same for a frame that came from yh_scene_append_memory_search (yh_scene_time and yh_scene_memory_time refuse such a frame
 * with YH_ESTATE and name this hook): the whole append - stamps, registration, ball memory, fuse - replayed from the state it
 * started from, ms_per_frame; then its registration launches alone (the clear, the scores, the choice), ms_search. Both rewrite
 * the same values and commit nothing. YH_ESTATE unless the handle's last frame is a search append. */
int yh_scene_memory_search_time(yh_scene* h, int32_t reps, float* ms_per_frame, float* ms_search);
/* Test hook: the registration kernels alone on two caller-given maps u32 [h][w] - n_host as the frame's stamps N, m_host as the
 * memory M - with n_rot gathers [n_rot][6] and the radius as yh_scene_append_memory_search takes them (the same YH_EINVAL checks on
 * the gathers; there are no carries). scores u64 [n_rot][2 radius + 1][2 radius + 1] as yh_scene_motion_read lays them out, chosen
 * [3] = k, u, v, sum_n: each may be NULL. Waits. Reads and writes nothing of the handle's frame, memory or plans: it reaches values
 * (up to 2^32 - 1) and shapes no depth frame produces. */
int yh_scene_op_register(yh_scene* h, const uint32_t* n_host, const uint32_t* m_host, int32_t n_rot, const int32_t* gather_q16 /* [n_rot][6] */,
                         int32_t radius, uint64_t* scores, int32_t* chosen /* [3] */, uint64_t* sum_n);
/* The same for a frame that came from yh_scene_append_memory_pyramid (yh_scene_time, yh_scene_memory_time and
 * yh_scene_memory_search_time refuse such a frame with YH_ESTATE and name this hook): the whole append replayed from the state it
 * started from, ms_per_frame; then its registration launches alone (the levels, the clear, scores and select per level),
 * ms_search. Both rewrite the same values and commit nothing. YH_ESTATE unless the handle's last frame is a pyramid append. */
int yh_scene_memory_pyramid_time(yh_scene* h, int32_t reps, float* ms_per_frame, float* ms_search);
/* The same for a frame that came from yh_scene_append_memory_search_norm (yh_scene_time, yh_scene_memory_time,
 * yh_scene_memory_search_time and yh_scene_memory_pyramid_time refuse such a frame with YH_ESTATE and name this hook): the whole
 * append replayed from the state it started from, ms_per_frame; then its registration launches alone (the clear, the three tables,
 * the choice), ms_search. Both rewrite the same values and commit nothing. YH_ESTATE unless the last frame is a normalised search. */
int yh_scene_memory_search_norm_time(yh_scene* h, int32_t reps, float* ms_per_frame, float* ms_search);
/* Test hook: the normalised registration's two kernels alone on two caller-given maps u32 [h][w], as yh_scene_op_register runs the
 * plain ones, with min_inside as yh_scene_append_memory_search_norm takes it (the same YH_EINVAL checks). scores (S), totals (T) and
 * inside (C), each u64 [n_rot][2 radius + 1][2 radius + 1]; chosen [3] = k, u, v; qualified; sum_n: each may be NULL. Waits. Reads
 * and writes nothing of the handle's frame, memory or plans. */
int yh_scene_op_register_norm(yh_scene* h, const uint32_t* n_host, const uint32_t* m_host, int32_t n_rot, const int32_t* gather_q16 /* [n_rot][6] */,
                              int32_t radius, int32_t min_inside, uint64_t* scores, uint64_t* totals, uint64_t* inside, int32_t* chosen /* [3] */,
                              int32_t* qualified, uint64_t* sum_n);
/* Test hook: the pyramid registration alone - the levels, every level's scores, the descent and the choice - on two caller-given
 * maps u32 [h][w], with buffers of its own; n_rot gathers, levels, radius and refine as yh_scene_append_memory_pyramid takes them
 * (the same YH_EINVAL checks; there are no carries). chosen [3] = k, u, v; score [3] = S chosen, S(0, 0, 0), sum_n; pyr_n and
 * pyr_m the pooled levels 1 .. levels of each map, concatenated; centres and scores what yh_scene_pyramid_read returns, levels
 * 0 .. levels concatenated. Each may be NULL. Waits. Reads and writes nothing of the handle's frame, memory or plans. */
int yh_scene_op_pyramid(yh_scene* h, const uint32_t* n_host, const uint32_t* m_host, int32_t n_rot, const int32_t* gather_q16 /* [n_rot][6] */,
                        int32_t levels, int32_t radius, int32_t refine, int32_t* chosen /* [3] */, uint64_t* score /* [3] */, uint32_t* pyr_n,
                        uint32_t* pyr_m, int32_t* centres, uint64_t* scores);
/* The same for a frame that came from yh_scene_append_memory_pyramid_norm (yh_scene_time, yh_scene_memory_time,
 * yh_scene_memory_search_time, yh_scene_memory_pyramid_time and yh_scene_memory_search_norm_time refuse such a frame with YH_ESTATE
 * and name this hook): the whole append replayed from the state it started from, ms_per_frame; then its registration launches alone
 * (the levels, the clear, tables and select per level), ms_search. Both rewrite the same values and commit nothing. YH_ESTATE
 * unless the handle's last frame is a normalised pyramid append. */
int yh_scene_memory_pyramid_norm_time(yh_scene* h, int32_t reps, float* ms_per_frame, float* ms_search);
/* Test hook: the normalised pyramid registration alone on two caller-given maps, as yh_scene_op_pyramid runs the plain one, with
 * min_inside as yh_scene_append_memory_pyramid_norm takes it (the same YH_EINVAL checks). The arguments up to scores are
 * yh_scene_op_pyramid's (scores: the S tables); totals (T) and inside (C) are laid out as scores; qualified holds one flag per
 * hypothesis, levels 0 .. levels concatenated as centres are - whether any of its entries qualified - and after them one more:
 * whether the choice qualified; chosen_stc [3] = S, T, C of the choice. Each may be NULL. Waits. Buffers of its own: reads and writes
 * nothing of the handle's frame, memory or plans. */
int yh_scene_op_pyramid_norm(yh_scene* h, const uint32_t* n_host, const uint32_t* m_host, int32_t n_rot, const int32_t* gather_q16 /* [n_rot][6] */,
                             int32_t levels, int32_t radius, int32_t refine, int32_t* chosen /* [3] */, uint64_t* score /* [3] */, uint32_t* pyr_n,
                             uint32_t* pyr_m, int32_t* centres, uint64_t* scores, int32_t min_inside, uint64_t* totals, uint64_t* inside,
                             int32_t* qualified, uint64_t* chosen_stc /* [3] */);
/* Test hook: uploads host fields (height map u32 [h][w], connections0 / connections1 f32 [h][w][4], laid out as yh_scene_read
 * returns them) as if a YH_COMPAT_SANE frame had produced them, so that yh_scene_plan runs on constructed mazes. The planner reads
 * conn0[..][2] (right) and conn1[..][0] (down) and takes left / up from the neighbour, as SANE's symmetry allows: YH_EINVAL (nothing
 * uploaded) unless every in-frame right / down length is finite, >= 1 and equal to the neighbour's left / up entry. The diagonal entries
 * (conn0[..][1], [3], conn1[..][1], [3]) are no reason to refuse: whether every in-frame one is finite, >= 1 and equal to the
 * other end's entry is recorded, and an 8-connected plan or tour on fields that fail it returns YH_ESTATE. world and balls are zeroed; it counts as a new frame. A yh_scene_time after it replays the handle's own input buffers and
 * overwrites the fields. */
int yh_scene_set_fields(yh_scene* h, const uint32_t* map, const float* conn0, const float* conn1);
/* Measurement hook: replays the last yh_scene_plan `reps` times: mean milliseconds per plan between two events on the handle's
 * stream (the host's reads of the solver's counters fall inside, as they do for a caller), the solver's rounds (launches in
 * which some tile ran) and tile executions of one plan. The replay has the plan's connectivity. */
int yh_scene_plan_time(yh_scene* h, int32_t reps, float* ms_per_plan, int32_t* rounds, int32_t* tile_runs);
/* The same for the last yh_scene_plan_tour (the host's choice of the order and the walks fall inside too): rounds = launches in
 * which some tile of some field ran, tile_runs summed over the fields. */
int yh_scene_tour_time(yh_scene* h, int32_t reps, float* ms_per_tour, int32_t* rounds, int32_t* tile_runs);
/* The same for the last yh_scene_plan_turn, replayed with its start heading and turn price: rounds and tile runs of the
 * eight-layer field (a tile run relaxes the tile in all eight layers). */
int yh_scene_turn_time(yh_scene* h, int32_t reps, float* ms_per_plan, int32_t* rounds, int32_t* tile_runs);
/* The same for the last yh_scene_plan_turn_tour, replayed with its start heading and turn price (the read of the leg table, the
 * host's choice of the order and the walks fall inside): rounds = launches in which some tile of some field ran, tile_runs summed
 * over the fields (a tile run relaxes the tile in all eight layers of one field). */
int yh_scene_turn_tour_time(yh_scene* h, int32_t reps, float* ms_per_tour, int32_t* rounds, int32_t* tile_runs);
/* Measurement hook: mean device milliseconds per BATCH over `reps` re-runs of the last yh_scene_batch_append (its n_frames and
 * mode) from the staged slots as they are now. It counts as an append: an earlier plan becomes unreadable. */
int yh_scene_batch_time(yh_scene_batch* h, int32_t reps, float* ms_per_batch);
/* The same for frames that came from yh_scene_batch_append_memory (yh_scene_batch_time refuses such frames with YH_ESTATE and names
 * this function): the append's own slots, motions and streams, replayed from the state every stream it named was in before it - the
 * bank keeps two maps and two tables per stream - into the state it left, so every field and every memory is rewritten with the same
 * bits and nothing is committed. YH_ESTATE unless the current frames are a memory append's (a plain append, yh_scene_batch_set_fields,
 * yh_scene_batch_memory_reset or a staged slot since ends that). */
int yh_scene_batch_memory_time(yh_scene_batch* h, int32_t reps, float* ms_per_batch);
/* The same for frames that came from yh_scene_batch_append_memory_search (yh_scene_batch_time and yh_scene_batch_memory_time refuse
 * such frames with YH_ESTATE and name this function): the whole append - stamps, the rounds' registration and fuse, the ball
 * chains - replayed from the state it started from, ms_per_batch; then its registration launches alone (the clear, every round's
 * scores and choice; the frames' map slots still hold each predecessor's fused map), ms_search. Both rewrite the same bits and commit
 * nothing. Refused as yh_scene_batch_memory_time refuses. */
int yh_scene_batch_memory_search_time(yh_scene_batch* h, int32_t reps, float* ms_per_batch, float* ms_search);
/* The same for frames that came from yh_scene_batch_append_memory_pyramid (yh_scene_batch_time, yh_scene_batch_memory_time and
 * yh_scene_batch_memory_search_time refuse such frames with YH_ESTATE and name this function): the whole append replayed from the
 * state it started from and the tables of level bases as they stand on the device, ms_per_batch; then its registration launches
 * alone (the clear, every round's levels, scores and choices), ms_search. Both rewrite the same bits and commit nothing. Refused as
 * yh_scene_batch_memory_search_time refuses. */
int yh_scene_batch_memory_pyramid_time(yh_scene_batch* h, int32_t reps, float* ms_per_batch, float* ms_search);
/* The same for frames that came from yh_scene_batch_append_memory_search_norm (the four hooks above refuse such frames with
 * YH_ESTATE and name this function): the whole append replayed from the state it started from, ms_per_batch; then its registration
 * launches alone (the clear, every round's three tables and choice), ms_search. Both rewrite the same bits and commit nothing.
 * YH_ESTATE in every other state: frames of any other append, a memory reset or a slot staged since. */
int yh_scene_batch_memory_search_norm_time(yh_scene_batch* h, int32_t reps, float* ms_per_batch, float* ms_search);
/* The same for frames that came from yh_scene_batch_append_memory_pyramid_norm (the four hooks above refuse such frames with
 * YH_ESTATE and name this function): the whole append replayed from the state it started from and the tables of level bases as they
 * stand on the device, ms_per_batch; then its registration launches alone (the clear, every round's levels, tables and choices),
 * ms_search. Refused as yh_scene_batch_memory_search_norm_time refuses. */
int yh_scene_batch_memory_pyramid_norm_time(yh_scene_batch* h, int32_t reps, float* ms_per_batch, float* ms_search);
/* yh_scene_plan_time for the last yh_scene_batch_plan: milliseconds per batch; rounds = launches in which some tile of some frame
 * ran (those of the slowest frame), tile_runs summed over the frames. */
int yh_scene_batch_plan_time(yh_scene_batch* h, int32_t reps, float* ms_per_batch, int32_t* rounds, int32_t* tile_runs);
/* The same for the last yh_scene_batch_plan_turn, replayed with its start headings and turn price: rounds and tile runs of the
 * frames' eight-layer fields. */
int yh_scene_batch_turn_time(yh_scene_batch* h, int32_t reps, float* ms_per_batch, int32_t* rounds, int32_t* tile_runs);
/* The same for the last yh_scene_batch_plan_turn_tour, replayed with its targets, start states and turn price (the read of the leg
 * tables, the host's choice of every frame's order and the walks fall inside): rounds = launches in which some tile of some field
 * of some frame ran, tile_runs summed over all fields. */
int yh_scene_batch_turn_tour_time(yh_scene_batch* h, int32_t reps, float* ms_per_batch, int32_t* rounds, int32_t* tile_runs);
/* The same for the last yh_scene_batch_plan_tour, replayed with its targets, starts and connectivity (the host's choice of every
 * frame's order and the walks fall inside): rounds = launches in which some tile of some field of some frame ran, tile_runs summed
 * over all fields. */
int yh_scene_batch_tour_time(yh_scene_batch* h, int32_t reps, float* ms_per_batch, int32_t* rounds, int32_t* tile_runs);
/* yh_scene_set_fields for one frame of a batch, with the same checks, so that constructed mazes can sit beside easy frames. The first
 * use after create or an append starts a new batch whose n is the highest frame set + 1 (a plan refuses, YH_ESTATE, while a frame
 * below n has been given no fields). It counts as a YH_COMPAT_SANE append (a new frame generation). */
int yh_scene_batch_set_fields(yh_scene_batch* h, int32_t frame, const uint32_t* map, const float* conn0, const float* conn1);

/* Test hook: copies the named intermediate tensor of the last forward (layer names of DESIGN.md:
 * "stem", "pool", "c2".."c5", "lat3".."lat5", "p3".."p7", "proto0".."proto3", "proto_up", "head_t0"..) to
 * host memory as f32 NHWC; dims receives {n,h,w,c}. Returns YH_EINVAL for unknown names. "stem" is
 * fused into the pool kernel and only materialised by engines created with debug_tensors = 1 (YH_ESTATE otherwise). */
int yh_debug_read_tensor(yh_engine* h, const char* name, float* dst_host, size_t nfloats, int32_t dims[4]);
/* Same for ONE frame of the batch (dims receives {1,h,w,c}): a batch-64 tensor is gigabytes as f32. */
int yh_debug_read_tensor_frame(yh_engine* h, const char* name, int32_t frame, float* dst_host, size_t nfloats, int32_t dims[4]);
/* Test hook, fp8 precision: the raw OCP E4M3 codes of the named tensor's E4M3 twin for ONE frame, as the last step wrote them (NHWC, one
 * byte per element, no decoding); dims receives {1,h,w,c}; dst may be NULL to ask for the dims. The value of a code is
 * table[code] * s[channel] with the channel scales of the tensor's allocation (yh_fp8_layer_channel_scales of a layer that reads it).
 * Pyramid level slices ("p3".."p7") work as in yh_debug_read_tensor. YH_ESTATE (with a reason in yh_last_error) when the handle does
 * not run its fp8 forward (f16 precision, scales not set) or the plan does not write that form of this tensor. */
int yh_debug_read_tensor_e4m3(yh_engine* h, const char* name, int32_t frame, uint8_t* dst, size_t n, int32_t dims[4]);
/* Test hook, fp8 precision: E4M3 layer layer_index's (yh_fp8_layer_info) weight codes as its kernel reads them, codes[cout][k*k*cin]
 * (K index = tap * cin + c), and the per-output-channel scales s_w[cout] of its epilogue; dims receives {cout, k*k*cin}; codes / s_w
 * may be NULL. YH_ESTATE while no weights are loaded or the layer's input tensor has no scales. */
int yh_debug_fp8_weights(yh_engine* h, int32_t layer_index, uint8_t* codes, float* s_w, int32_t dims[2]);
/* Test hook: number of conv kernel launches the last yh_op_conv2d_f16 on this handle was planned as
 * (1 = single launch, 2 = two-phase or channel-split plan; the split-K reduce is not counted). */
int yh_debug_last_conv_launches(const yh_engine* h);
/* The forms conv_igemm_f16 is instantiated in (ConvForm, csrc/yh_internal.h): plain, the streaming tile's 3x3 form, split-K (the slice
 * kernel; splitk_reduce_f16 finishes it), multi-level, multi-level split-K, two-source, two-source split-K, upsampled residual, fused
 * 1x1 tail, dense 1x1. YH_FORM_REDUCE is no form of the table: it stands for splitk_reduce_f16 in yh_debug_last_conv_forms. */
enum { YH_FORM_PLAIN = 0, YH_FORM_K3, YH_FORM_SPLITK, YH_FORM_ML, YH_FORM_ML_SPLITK, YH_FORM_DUAL, YH_FORM_DUAL_SPLITK, YH_FORM_RESUP,
       YH_FORM_TAIL, YH_FORM_LIN, YH_CONV_FORMS, YH_FORM_REDUCE = YH_CONV_FORMS };
/* The table of conv kernel instances (kConvTiles, csrc/conv_igemm.hip) as it was compiled: returns the number of tiles and writes, for
 * the first `cap` of them, rows[5 i ..] = { tile id, channels per tile, rows per tile, 1 if the tile reads E4M3 operands, form mask
 * (bit f: the tile is instantiated in form f) }. Takes no handle and touches no device: tests/test_conv_form_cases.py holds the
 * table against the tests' cases (a (tile, form) without a case does not ship). rows may be NULL. */
int yh_conv_forms(int32_t* rows, int32_t cap);
/* Test hook: the kernels the last single-op conv call on this handle launched, in order: pairs[2 i] = tile id, pairs[2 i + 1] = form
 * (the value the launch was made with, not a re-derivation); a split-K call lists its reduce kernel as (-1, YH_FORM_REDUCE).
 * Returns their number and writes the first `cap` pairs. A refused call (YH_EINVAL) leaves the list as it was. */
int yh_debug_last_conv_forms(const yh_engine* h, int32_t* pairs, int32_t cap);

/* Audit hooks (profiles/r03_fault_audit.md). Text into out[cap] (YH_EOVERFLOW if truncated): every buffer of the handle
 * with [base, end) and where those sit inside their 2 MiB page; the nodes of the step for the current batch size as the
 * handle's tuning captures it (kernel symbol, grid, block, the pointers of its launch argument), sorted. */
int yh_debug_alloc_map(yh_engine* h, char* out, size_t cap);
/* Process-wide counters of the setup discipline: out[0] once-only setup sections entered (graph captures), out[1]
 * jobs run by group worker threads, out[2] times one of the former overlapped one of the latter anywhere in the process (must stay 0),
 * out[3] sections / jobs in flight right now. */
int yh_debug_setup_audit(int64_t out[4]);
/* Study hook (tools/study/cu_mask_scaling.py, profiles/r05_overlap.txt): re-creates the handle's two compute streams with
 * hipExtStreamCreateWithCUMask - bit i of mask[] enables CU i (the driver deals the bits over the XCDs round-robin) - and drops the
 * captured steps. How every kernel of a step scales with the CUs it is given is what decides whether two engines on disjoint CU
 * sets can overlap the step's memory-bound and matrix-bound phases. */
int yh_debug_set_cu_mask(yh_engine* h, const uint32_t* mask, int32_t n_words);
/* ... and one PHASE of the forward for the frames last set, `reps` times back to back, eagerly on the handle's stream (timing only: the
 * second phase reads whatever the first last left): phase 0 = backbone + FPN laterals (the memory-bound half of a batch-64 step),
 * phase 1 = the FPN's 3x3 convolutions, the protonet and the prediction head (the matrix-bound half). *ms_total: device time. */
int yh_debug_run_phase(yh_engine* h, int32_t phase, int32_t reps, float* ms_total);
/* Test hook, process-wide: allow = 1 lets yh_group_broadcast_weights / yh_group_replicate_weights treat handles that share a device as
 * separate RCCL ranks. Real RCCL refuses two ranks on one GPU, so this is only meaningful under the stand-in librccl of
 * tests/rccl_standin/ (which is how a one-GPU box executes the n > 1 collective code). Returns the previous setting. */
int yh_debug_rccl_shared_device(int32_t allow);
/* Test hook, process-wide, before the first RCCL call of the process (YH_ESTATE afterwards): open THIS file instead of searching for
 * librccl.so.1. A process that has torch loaded already holds torch's bundled librccl under that soname, so the loader's search path
 * cannot reach the stand-in there (bench.py --rccl-library); processes without torch find it through LD_LIBRARY_PATH, hook unused. */
int yh_debug_rccl_library(const char* path);
int yh_debug_graph_nodes(yh_engine* h, int32_t with_tail, char* out, size_t cap);
/* Bounds hooks ("Bounds"); none of the three launches a kernel.
 * yh_debug_guard_selfcheck: the check of the single-op entry points' output guards on itself. It stages an output of 3 rows x 64 f16
 * as those entry points do - 4096 bytes in front of the payload, 256 rows behind it, all 0xFF - changes ONE guard byte with a copy
 * (where: 0 none, 1 the last byte of the front guard, 2 the first byte behind the payload, 3 the last byte of the back guard, 4 the
 * first byte of the front guard) and runs the same check: YH_OK for 0, YH_EOVERFLOW for 1 .. 4 with a message that names the
 * output, the side and the byte. YH_EINVAL for any other `where`.
 * yh_debug_act_paint: fills images first_image .. max_batch - 1 of every activation allocation of the handle (and of its E4M3 twin
 * in fp8 handles) with 0xFF - NaN in both formats; the 256 zero bytes behind each allocation, zero pixel first, are not touched.
 * yh_debug_act_check: the painted images must still be 0xFF in every byte and those 256 bytes zero: YH_EOVERFLOW otherwise, the first
 * changed byte (allocation, image, row, byte) in yh_last_error and, one per line, up to nine of them in out[cap] (out may be NULL).
 * Both: YH_EINVAL for first_image outside 1 .. max_batch - 1, YH_ESTATE before the weights are loaded; both wait for the handle's
 * streams first. A step of n <= first_image frames between the two must leave everything painted as it was. */
int yh_debug_guard_selfcheck(yh_engine* h, int32_t where);
int yh_debug_act_paint(yh_engine* h, int32_t first_image);
int yh_debug_act_check(yh_engine* h, int32_t first_image, char* out, size_t cap);

/* ---- single-op entry points (parity tests call kernels through the C ABI) ------------------- */

/* One NHWC f16 convolution on the MFMA implicit-GEMM kernel with fused bias (+residual) (+act).
 * All pointers are host memory; the call stages, runs and copies back (test-only convenience).
 * x: [n,h,w,cin] f16 bits; w: [cout,kh,kw,cin] f16 bits; bias: [cout] f32; residual (nullable):
 * [n,ho,wo,cout] f16 bits; y: [n,ho,wo,cout] f16 bits. act: 0 none, 1 relu, 2 tanh. */
int yh_op_conv2d_f16(yh_engine* h, const uint16_t* x, int32_t n, int32_t hh, int32_t ww, int32_t cin,
                     const uint16_t* w, const float* bias, int32_t cout, int32_t kh, int32_t kw,
                     int32_t stride, int32_t pad, const uint16_t* residual, int32_t act,
                     uint16_t* y);
/* The two-source 1x1 convolution (a bottleneck block's last conv and its projection shortcut as one accumulation):
 * y[n][ho][wo][cout] = act(bias + sum_c w[o][c] x1[n][p][q][c] + sum_c w[o][c1 + c] x2[n][p*stride2][q*stride2][c]),
 * x1: [n][ho][wo][c1], x2: [n][h2][w2][c2], w: [cout][c1 + c2] f16 bits; c1, c2 % 64 == 0, cout % 8 == 0; act 0 / 1 (relu).
 * tune.op_tile selects the tile (those of the two-source form only), tune.op_kslices a split-K. */
int yh_op_conv2d_dual_f16(yh_engine* h, const uint16_t* x1, int32_t n, int32_t ho, int32_t wo, int32_t c1,
                          const uint16_t* x2, int32_t h2, int32_t w2, int32_t c2, int32_t stride2,
                          const uint16_t* w, const float* bias, int32_t cout, int32_t act, uint16_t* y);
/* One bottleneck launch of csrc/bneck.hip on caller tensors (dense host arrays, f16 as bits), the only way to run a row of
 * kBneckChains or bneck_xn_f16 without a network around it:
 *   b  = relu(conv3x3(a; stride, pad 1) + bias2)            a [n][hh][ww][planes], w2 [planes][3][3][planes], stride 1 or 2
 *   y  = relu(w3 [b ; x2] + bias3 (+ res))                   w3 [4 planes][planes (+ 64)], y [M][4 planes], M = n P Q
 *   a' = relu(w1n y + bias1n)                                w1n [planes][4 planes], a_next [M][planes]
 * planes 64 / 128 with tile_m, w1n != NULL (the next block's reduce conv) and x2 != NULL (the stage's first block) select the row
 * of kBneckChains; either res [M][4 planes] (identity shortcut) or x2 [n][h2][w2][64] read at stride2 (pixel (p, q) <- (p stride2,
 * q stride2)) together with w1n. a_next is written iff w1n is given. planes 256, tile_m 64: bneck_xn_f16 - a IS b, [n][hh][ww][256]
 * (w2, bias2, stride unused), res and w1n required, and a' goes to a_next and / or, as E4M3 codes of a' * inv_scale[channel],
 * to a_next8 [M][256] (at least one of the two). YH_EINVAL with a message, and no launch, for a combination launch_bneck has no
 * kernel for. tune.op_xgap: every image of a is followed by that many elements of NaN (chains only: bneck_xn_f16 reads dense
 * rows and refuses a gap). Like every single-op convolution, resize, pool, quantise and absmax entry point here, it stages each
 * output between guards of 0xFF - 4096 bytes in front, 256 rows behind row M - 1 - and each input between 4096-byte bands of NaN:
 * YH_EOVERFLOW with a message (output, side, byte, row) if the launch changed a guard byte. */
int yh_op_bneck_f16(yh_engine* h, int32_t planes, int32_t tile_m, const uint16_t* a, int32_t n, int32_t hh, int32_t ww,
                    const uint16_t* w2, const float* bias2, int32_t stride, const uint16_t* w3, const float* bias3,
                    const uint16_t* res, const uint16_t* x2, int32_t h2, int32_t w2w, int32_t stride2,
                    const uint16_t* w1n, const float* bias1n, uint16_t* y, uint16_t* a_next, uint8_t* a_next8,
                    const float* inv_scale);
/* Bilinear resize (align_corners = false) of an NHWC f16 tensor, optional accumulate into dst. */
int yh_op_bilinear_f16(yh_engine* h, const uint16_t* x, int32_t n, int32_t hh, int32_t ww, int32_t c,
                       int32_t ho, int32_t wo, uint16_t* y);
/* 3x3 stride-2 pad-1 max pool of an NHWC f16 tensor. */
int yh_op_maxpool3x3s2_f16(yh_engine* h, const uint16_t* x, int32_t n, int32_t hh, int32_t ww,
                           int32_t c, uint16_t* y);
/* The shared prediction head's form of the convolution: x[n][cells][cin] holds nlev square pyramid
 * levels (edge lengths level_sizes[]) end to end per image; a k x k stride-1 'same' conv runs over all
 * of them in one launch, every tap staying inside its row's own level. y[n][cells][cout]. */
int yh_op_conv2d_levels_f16(yh_engine* h, const uint16_t* x, int32_t n, const int32_t* level_sizes, int32_t nlev, int32_t cin,
                            const uint16_t* w, const float* bias, int32_t cout, int32_t k, int32_t act, uint16_t* y);
/* The fused stem (conv 7x7 stride 2 pad 3, 3 -> 64, bias, ReLU; then max pool 3x3 stride 2 pad 1) on
 * x[n][S][S][3] f16 bits with w[64][7][7][3]; S even. Writes pool_out[n][PO][PO][64] and, if not NULL,
 * stem_out[n][SO][SO][64] (the pre-pool tensor, a test hook). */
int yh_op_stem_pool_f16(yh_engine* h, const uint16_t* x, int32_t n, int32_t S, const uint16_t* w, const float* bias,
                        uint16_t* stem_out, uint16_t* pool_out);
/* The same from raw frames rgb[n][S][S][3] uint8: the kernel's loader also does the preprocessing
 * ((v - mean) / std per channel, rounded to f16), as in production runs. */
int yh_op_stem_pool_rgb8(yh_engine* h, const uint8_t* rgb, int32_t n, int32_t S, const uint16_t* w, const float* bias,
                         uint16_t* stem_out, uint16_t* pool_out);
/* The quantiser of the fp8 forward (the producers' epilogues apply the same conversion): y[i] = OCP FP8 E4M3 code of
 * x[i] * inv_scale (x: f16 bits), round to nearest even, saturating at +-448, NaN -> 0x7F | sign. */
int yh_op_quantize_e4m3(yh_engine* h, const uint16_t* x, size_t n, float inv_scale, uint8_t* y);
/* The calibration's kernel (yh_fp8_calibrate) on caller data: out_bits[c] = the bit pattern of max over rows of |x[r][c]| as f32, x:
 * [rows][C] f16 bits in host memory. A NaN in a channel wins (a NaN pattern comes back), Inf lies above every finite value.
 * YH_EINVAL for a C the kernel's launcher rejects (C % 8 != 0 or 256 % (C / 8) != 0). */
int yh_op_absmax_channels_f16(yh_engine* h, const uint16_t* x, int64_t rows, int32_t C, uint32_t* out_bits);
/* One fp8 convolution on the 256 x 256 tile the YH_PRECISION_FP8 forward uses: x[n][hh][ww][cin] and w[cout][k][k][cin]
 * are E4M3 codes (cin % 128 == 0), f32 accumulation on the block-scaled MFMA with unit block scales,
 * y = act(acc * scale[ch] + bias[ch] + residual) rounded to f16. If reps > 0, *ms_per_launch receives the mean
 * kernel time of `reps` further launches. */
int yh_op_conv2d_fp8(yh_engine* h, const uint8_t* x, int32_t n, int32_t hh, int32_t ww, int32_t cin, const uint8_t* w,
                     const float* scale, const float* bias, int32_t cout, int32_t k, int32_t stride, int32_t pad,
                     const uint16_t* residual, int32_t act, uint16_t* y, int32_t reps, float* ms_per_launch);
/* tune.op_tile may name another fp8 tile (TILE_128x128_FP8 = 23, TILE_64x64_FP8 = 24; the weight panel is then padded to that tile's
 * channels); YH_EINVAL, and no launch, for a tile that is not an fp8 tile of the plain form.
 * The multi-level form of the fp8 convolution (yh_op_conv2d_levels_f16's layout, E4M3 codes as in yh_op_conv2d_fp8; k 1 or 3, stride 1,
 * 'same' padding) on the fp8 tiles that have it: tune.op_tile 20 (default) or 23. */
int yh_op_conv2d_levels_fp8(yh_engine* h, const uint8_t* x, int32_t n, const int32_t* level_sizes, int32_t nlev, int32_t cin,
                            const uint8_t* w, const float* scale, const float* bias, int32_t cout, int32_t k, int32_t act, uint16_t* y);
/* The FPN lateral: a 1x1 convolution whose residual is the lower pyramid level resized in the epilogue (ConvParams::res_up),
 *   y[n][P][Q][cout] = f16(act((acc + bias) + f16(bilinear(res_lo -> P x Q)))),   x [n][P][Q][cin], w [cout][cin], res_lo [n][rh][rw][cout]
 * (cin % 64 == 0; act 0 / 1). tune.op_tile selects the tile (default TILE_128x128); tune.op_kslices forces a split-K on the tiles that
 * have that form (the residual is then resized by splitk_reduce_f16). YH_EINVAL, and no launch, for a tile without the form. */
int yh_op_conv2d_resup_f16(yh_engine* h, const uint16_t* x, int32_t n, int32_t P, int32_t Q, int32_t cin, const uint16_t* w,
                           const float* bias, int32_t cout, const uint16_t* res_lo, int32_t rh, int32_t rw, int32_t act, uint16_t* y);
/* A k x k stride-1 'same' convolution to exactly 256 channels with the 1x1 convolution to 32 channels run on its LDS image in the
 * epilogue (ConvParams::w2: the protonet's last two layers as one launch):
 *   t = f16(act(conv(x, w) + bias)),  y2[M][32] = f16(relu(w2 t + bias2)),   w [256][k][k][cin], w2 [32][256], M = n hh ww
 * (cin % 64 == 0, act 0 / 1; t is never stored). tune.op_tile: a tile with the form (default TILE_256x256_M16). y2 is staged between
 * guards of 0xFF as every output here: YH_EOVERFLOW if the launch changed one of their bytes. YH_EINVAL, and no launch, for cout != 256
 * or a tile without the form. */
int yh_op_conv2d_tail_f16(yh_engine* h, const uint16_t* x, int32_t n, int32_t hh, int32_t ww, int32_t cin, const uint16_t* w,
                          const float* bias, int32_t cout, int32_t k, int32_t act, const uint16_t* w2, const float* bias2, uint16_t* y2);
/* ... with E4M3 operands for the first convolution (x, w: codes, cin % 128 == 0; t = f16(act(acc * scale[ch] + bias[ch]))), on
 * TILE_256x256_FP8. */
int yh_op_conv2d_tail_fp8(yh_engine* h, const uint8_t* x, int32_t n, int32_t hh, int32_t ww, int32_t cin, const uint8_t* w,
                          const float* scale, const float* bias, int32_t cout, int32_t k, int32_t act, const uint16_t* w2,
                          const float* bias2, uint16_t* y2);
/* Detection tail alone on caller-provided head outputs (host f16 bits, layouts as outputs 0..3)
 * for n frames; results are then read with yh_read_detections. Lets the tail be checked
 * bit-for-bit against the oracle on identical inputs. */
int yh_op_detect(yh_engine* h, const uint16_t* loc, const uint16_t* conf, const uint16_t* mask,
                 const uint16_t* proto, int32_t n);

/* The instance frame (yh_instance_frame) on caller-provided detections: n <= max_dets binary masks u8 [n][hp][wp] (hp, wp in
 * 1 .. 4096), class ids i32 [n] (0 .. num_classes - 2) and scores f32 [n] in rank order, all in host memory; the same kernels run,
 * so the definition can be checked at tiny shapes without a network. out_host: width * height pixels; table / table_capacity /
 * n_instances as yh_instance_read (which, like yh_instance_device_frame, then shows this frame). */
int yh_op_instance_frame(yh_engine* h, const uint8_t* masks, const int32_t* class_ids, const float* scores, int32_t n, int32_t hp, int32_t wp,
                         int32_t width, int32_t height, const uint8_t* class_map, float min_score, uint32_t* out_host, int32_t* table,
                         int32_t table_capacity, int32_t* n_instances);
/* A tracked call (yh_instance_track) on caller-provided detections: yh_op_instance_frame's arguments plus iou_permille and max_age;
 * the same kernels run, on the handle's tracker, so successive calls form a sequence that can be checked at tiny shapes without a
 * network (a call at another hp x wp starts from an empty tracker). The track table is then read with yh_instance_tracks_read. */
int yh_op_instance_track(yh_engine* h, const uint8_t* masks, const int32_t* class_ids, const float* scores, int32_t n, int32_t hp, int32_t wp,
                         int32_t width, int32_t height, const uint8_t* class_map, float min_score, int32_t iou_permille, int32_t max_age,
                         uint32_t* out_host, int32_t* table, int32_t table_capacity, int32_t* n_instances);

/* yh_op_instance_frame for n_frames frames of caller-provided detections at once (yh_instance_batch's kernels): masks u8
 * [n_frames][n_dets][hp][wp], class ids i32 and scores f32 [n_frames][n_dets] in rank order per frame, counts i32 [n_frames], each in
 * 0 .. n_dets, with n_dets <= max_dets and n_frames in 1 .. 64. The mask slots past a frame's count are overwritten with 0xFF in the
 * upload, so a kernel that read them would paint them. out_host: n_frames * width * height pixels, or NULL; the tables are read with
 * yh_instance_batch_read (yh_instance_batch_device_frames then shows this batch). */
int yh_op_instance_batch(yh_engine* h, const uint8_t* masks, const int32_t* class_ids, const float* scores, const int32_t* counts,
                         int32_t n_frames, int32_t n_dets, int32_t hp, int32_t wp, int32_t width, int32_t height, const uint8_t* class_map,
                         float min_score, uint32_t* out_host);
/* A tracked batch (yh_instance_track_batch) on caller-provided detections: yh_op_instance_batch's arguments and limits plus
 * iou_permille, max_age and streams i32 [n_frames] (or NULL: all 0); the same kernels run, against the handle's bank of trackers, so
 * successive calls - and yh_op_instance_track calls on stream 0 between them - form the sequences. A stream whose tracker was
 * built at another hp x wp starts empty. The track tables are read with yh_instance_track_batch_read. */
int yh_op_instance_track_batch(yh_engine* h, const uint8_t* masks, const int32_t* class_ids, const float* scores, const int32_t* counts,
                               int32_t n_frames, int32_t n_dets, int32_t hp, int32_t wp, int32_t width, int32_t height,
                               const uint8_t* class_map, float min_score, int32_t iou_permille, int32_t max_age, const int32_t* streams,
                               uint32_t* out_host);

/* The classify batch's two kernels without the network (yh_classify_batch_u32, csrc/classify_batch.hip), for edge shapes; both need
 * 2n <= max_batch and neither needs weights. The pre half: n packed frames u32 [n][hgt][w] from the host -> the RGB8 tiles
 * [2n][S][S][3] the step would read (tiles 2b, 2b + 1 of frame b). *form (if not NULL) receives the form the kernel took at this
 * geometry: 0 the vertical pass in LDS, 1 the fallback that loops over global memory. The frames of an earlier batch are overwritten:
 * yh_classify_batch_device_frames is NULL afterwards. */
int yh_op_classify_pre_batch(yh_engine* h, const uint32_t* frames_host, int32_t n, int32_t w, int32_t hgt,
                             uint8_t* tiles_host /* [2n][S][S][3] */, int32_t* form /* 0 LDS, 1 fallback */);
/* The post half on caller-provided output-4 logits f32 [2n][cells][C]: cells_postprocess and classify_post_batch, with the batch
 * call's results and errors (YH_EDIVERGE, frames_host untouched, diverged_host [n]); frames_host and diverged_host may be NULL.
 * On success yh_classify_batch_device_frames shows this batch. */
int yh_op_classify_post_batch(yh_engine* h, const float* cells_host /* [2n][cells][C] */, int32_t n, int32_t w, int32_t hgt,
                              int32_t compat_mode, uint32_t* frames_host /* [n][hgt][w] */, int32_t* diverged_host);

/* Measurement: the handle's detection tail (yh_tfl_detect_setup) on the outputs of the last invoke, `reps` times, each of its four
 * launches (softmax and candidates, per-class NMS, top max_dets, masks) between two events on the handle's stream: ms_out[4], the
 * mean ms per launch. Synchronous; the states of yh_tfl_detect. */
int yh_tfl_detect_stage_times(yh_tfl* h, int32_t reps, float* ms_out);
/* The TFLite detection tail (yh_tfl_detect_setup's kernels) on caller-provided bytes, no model involved: what yh_op_detect is to
 * the engine. n images; loc [n][P][4], conf [n][P][C], mask [n][P][32], proto [n][hp][wp][32] in host memory, each with its kind
 * (YH_KIND_U8, YH_KIND_I8 or YH_KIND_F32), scale and zero point (ignored for float32); priors [P][4]. The handle gives the device,
 * the stream and the error text only; its model and its detect setup are not touched. Checks as yh_tfl_detect_setup's (YH_EINVAL).
 * Synchronous; the results are read with yh_tfl_read_detections. */
int yh_tfl_op_detect(yh_tfl* h, int32_t n, int32_t P, int32_t C, int32_t hp, int32_t wp,
                     const void* loc, int32_t loc_kind, float loc_scale, int32_t loc_zp,
                     const void* conf, int32_t conf_kind, float conf_scale, int32_t conf_zp,
                     const void* mask, int32_t mask_kind, float mask_scale, int32_t mask_zp,
                     const void* proto, int32_t proto_kind, float proto_scale, int32_t proto_zp,
                     const float* priors, int32_t top_k, int32_t max_dets, float conf_thresh, float nms_thresh);
/* yh_tfl_instance_frames' kernels on caller-provided detections, no model and no setup: what yh_op_instance_batch is to the engine.
 * n_frames (1 .. 64) camera frames of two images each, image 2b the left tile of frame b: masks uint8 [2n][n_dets][hp][wp],
 * class_ids and scores [2n][n_dets] in rank order per image, counts [2n], n_dets 0 .. 128. There is no setup to give C: a class id
 * lies in 0 .. 79 and class_map, if not NULL, has 80 entries. The mask slots past an image's count are uploaded as 0xFF (a kernel
 * that read them would paint them). YH_EINVAL as yh_tfl_instance_frames, and when the scores within an image's count are not
 * non-increasing (the order the tail returns and the kernels may rely on). The frames are painted between two guard bands of 4096
 * bytes of 0xFF, which are read back: YH_EOVERFLOW, naming the band and the byte, if one changed. The handle gives the device, the
 * stream and the error text only; on success the batch is the handle's (yh_tfl_instance_read, yh_tfl_instance_device_frames). */
int yh_tfl_op_instance_frames(yh_tfl* h, const uint8_t* masks, const int32_t* class_ids, const float* scores, const int32_t* counts,
                              int32_t n_frames, int32_t n_dets, int32_t hp, int32_t wp, int32_t width, int32_t height,
                              const uint8_t* class_map, float min_score, uint32_t* out_host /* [n][H][W] or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* YOLACT_HIP_DEBUG_H */
