// yolact.cpp — see yolact.hpp. Thin, allocation-free per call; all arithmetic is in libyolact_hip.so.
#include "yolact.hpp"

#include <fstream>
#include <iterator>
#include <stdexcept>
#include <utility>

namespace tod {

namespace {
[[noreturn]] void expect_failed(const char* what, const char* detail) {   // Rust: .expect("what")
    throw std::runtime_error(std::string(what) + ": " + (detail ? detail : ""));
}
}  // namespace

std::string Yolact::version() { return yh_version(); }

Yolact Yolact::init(const InitOptions& opt) {
    Yolact y;
    y.opt_ = opt;
    if (!opt.model_path.empty()) {
        std::ifstream f(opt.model_path, std::ios::binary);
        if (!f) expect_failed("failed to load model", opt.model_path.c_str());            // yolact.rs:20
        std::vector<char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (yh_tfl_create(bytes.data(), bytes.size(), opt.device, &y.tfl_) != YH_OK)
            expect_failed("must build interpreter", yh_tfl_last_error(nullptr));           // yolact.rs:29
        return y;
    }
    yh_config cfg;
    yh_default_config(&cfg);
    cfg.device = opt.device;
    cfg.input_size = opt.input_size;
    cfg.max_batch = 2;                         // the two tiles of yolact.rs:216-217 run as one batch
    if (yh_create(&cfg, &y.engine_) != YH_OK) expect_failed("must create interpreter builder", yh_last_error(nullptr));   // :25
    const std::size_t n = yh_weights_nbytes(y.engine_);
    std::vector<unsigned char> blob(n);
    if (yh_weights_generate(y.engine_, opt.seed, blob.data(), n) != YH_OK || yh_load_weights_host(y.engine_, blob.data(), n) != YH_OK)
        expect_failed("failed to allocate tensors.", yh_last_error(y.engine_));            // yolact.rs:35
    return y;
}

Yolact::Yolact(Yolact&& o) noexcept : engine_(o.engine_), tfl_(o.tfl_), opt_(std::move(o.opt_)) { o.engine_ = nullptr; o.tfl_ = nullptr; }

Yolact::~Yolact() {
    if (engine_) yh_destroy(engine_);
    if (tfl_) yh_tfl_destroy(tfl_);
}

void Yolact::classify(std::uint32_t* frame_buffer, std::size_t len) {
    if (len != static_cast<std::size_t>(opt_.frame_width) * opt_.frame_height)
        expect_failed("frame buffer", "length does not match width * height");            // ImageBuffer::from_vec(..).unwrap(), :207
    const int rc = engine_ ? yh_classify_frame_u32(engine_, frame_buffer, opt_.frame_width, opt_.frame_height, opt_.compat_mode)
                           : yh_tfl_classify_frame_u32(tfl_, frame_buffer, opt_.frame_width, opt_.frame_height, opt_.compat_mode);
    if (rc != YH_OK) expect_failed("invoke failed", engine_ ? yh_last_error(engine_) : yh_tfl_last_error(tfl_));   // :163
}

std::vector<std::vector<float>> Yolact::classify_tile_outputs(const std::uint8_t* rgb_tile) {
    if (!engine_) expect_failed("classify_tile", "interpreter-shaped calls are exposed for the YOLACT engine");
    std::int32_t dims[4];
    yh_input_dims(engine_, dims);                                                          // :149-150
    if (yh_set_input_u8(engine_, rgb_tile, 1) != YH_OK) expect_failed("must data", yh_last_error(engine_));   // :161-162
    if (yh_invoke(engine_) != YH_OK) expect_failed("invoke failed", yh_last_error(engine_));                    // :163
    std::vector<std::vector<float>> results;
    for (int i = 0; i < yh_output_count(engine_); ++i) {                                   // :166-188
        yh_tensor_info info;
        if (yh_output_info(engine_, i, &info) != YH_OK) expect_failed("must data", yh_last_error(engine_));
        std::size_t n = 1;
        for (int d = 0; d < info.ndims; ++d) n *= static_cast<std::size_t>(info.dims[d]);
        std::vector<float> out(n);
        if (yh_output_read_f32(engine_, i, out.data(), n) != YH_OK) expect_failed("must data", yh_last_error(engine_));
        results.push_back(std::move(out));
    }
    return results;
}

void Yolact::evaluate(const std::uint8_t* rgb_frames, int n) {
    if (!engine_) expect_failed("evaluate", "the detection tail belongs to the YOLACT engine");
    if (yh_set_input_u8(engine_, rgb_frames, n) != YH_OK) expect_failed("must data", yh_last_error(engine_));   // :161-162
    if (yh_evaluate(engine_) != YH_OK) expect_failed("invoke failed", yh_last_error(engine_));                  // :163
}

void Yolact::tfl_detect_setup(const float* priors, int n_priors, const yh_tfl_detect_config* cfg) {
    if (!tfl_) expect_failed("tfl_detect_setup", "this handle runs the YOLACT engine: its tail is evaluate()");
    yh_tfl_detect_config c;
    yh_tfl_default_detect_config(&c);
    if (yh_tfl_detect_setup(tfl_, cfg ? cfg : &c, priors, n_priors) != YH_OK) expect_failed("detect setup failed", yh_tfl_last_error(tfl_));
}

void Yolact::tfl_evaluate(const std::uint8_t* images, std::size_t nbytes, int n) {
    if (!tfl_) expect_failed("tfl_evaluate", "this handle runs the YOLACT engine: its tail is evaluate()");
    if (yh_tfl_set_batch(tfl_, n) != YH_OK || yh_tfl_set_input(tfl_, images, nbytes) != YH_OK) expect_failed("must data", yh_tfl_last_error(tfl_));   // :161-162
    if (yh_tfl_evaluate(tfl_) != YH_OK) expect_failed("invoke failed", yh_tfl_last_error(tfl_));                                                        // :163
}

std::vector<yh_detection> Yolact::tfl_detections(int image, std::vector<std::uint8_t>* masks_out) {
    if (!tfl_) expect_failed("tfl_detections", "this handle runs the YOLACT engine");
    std::int32_t n = 0, dims[2] = { 0, 0 };
    if (yh_tfl_read_detections(tfl_, image, &n, nullptr, 0, nullptr, 0) != YH_OK || yh_tfl_proto_dims(tfl_, dims) != YH_OK)
        expect_failed("must data", yh_tfl_last_error(tfl_));
    std::vector<yh_detection> dets(static_cast<std::size_t>(n));
    if (masks_out) masks_out->assign(static_cast<std::size_t>(n) * dims[0] * dims[1], 0);
    if (yh_tfl_read_detections(tfl_, image, &n, dets.data(), n, masks_out ? masks_out->data() : nullptr, masks_out ? masks_out->size() : 0) != YH_OK)
        expect_failed("must data", yh_tfl_last_error(tfl_));
    return dets;
}

std::vector<std::int32_t> Yolact::instance_frame(int frame, int width, int height, const std::uint8_t* class_map, float min_score,
                                                 std::uint32_t* frame_out) {
    if (!engine_) expect_failed("instance_frame", "the detection tail belongs to the YOLACT engine");
    if (yh_instance_frame(engine_, frame, width, height, class_map, min_score, frame_out) != YH_OK)
        expect_failed("instance frame failed", yh_last_error(engine_));
    std::int32_t m = 0;
    if (yh_instance_read(engine_, &m, nullptr, 0) != YH_OK) expect_failed("must data", yh_last_error(engine_));
    std::vector<std::int32_t> table(static_cast<std::size_t>(m) * 4);
    if (yh_instance_read(engine_, &m, table.data(), m) != YH_OK) expect_failed("must data", yh_last_error(engine_));
    return table;
}

const std::uint32_t* Yolact::instance_device_frame() const { return engine_ ? yh_instance_device_frame(engine_) : nullptr; }

std::vector<std::vector<std::int32_t>> Yolact::instance_batch(int first, int n, int width, int height, const std::uint8_t* class_map,
                                                              float min_score, std::uint32_t* frames_out) {
    if (!engine_) expect_failed("instance_batch", "the detection tail belongs to the YOLACT engine");
    if (yh_instance_batch(engine_, first, n, width, height, class_map, min_score, frames_out) != YH_OK)
        expect_failed("instance batch failed", yh_last_error(engine_));
    std::vector<std::vector<std::int32_t>> tables(static_cast<std::size_t>(n));
    for (int b = 0; b < n; ++b) {
        std::int32_t m = 0;
        if (yh_instance_batch_read(engine_, b, &m, nullptr, 0) != YH_OK) expect_failed("must data", yh_last_error(engine_));
        tables[b].resize(static_cast<std::size_t>(m) * 4);
        if (yh_instance_batch_read(engine_, b, &m, tables[b].data(), m) != YH_OK) expect_failed("must data", yh_last_error(engine_));
    }
    return tables;
}

const std::uint32_t* Yolact::instance_batch_device_frames() const { return engine_ ? yh_instance_batch_device_frames(engine_) : nullptr; }

std::vector<std::int32_t> Yolact::instance_track(int frame, int width, int height, const std::uint8_t* class_map, float min_score,
                                                 int iou_permille, int max_age, std::uint32_t* frame_out) {
    if (!engine_) expect_failed("instance_track", "the detection tail belongs to the YOLACT engine");
    if (yh_instance_track(engine_, frame, width, height, class_map, min_score, iou_permille, max_age, frame_out) != YH_OK)
        expect_failed("instance track failed", yh_last_error(engine_));
    std::int32_t m = 0;
    if (yh_instance_read(engine_, &m, nullptr, 0) != YH_OK) expect_failed("must data", yh_last_error(engine_));
    std::vector<std::int32_t> table(static_cast<std::size_t>(m) * 4);
    if (yh_instance_read(engine_, &m, table.data(), m) != YH_OK) expect_failed("must data", yh_last_error(engine_));
    return table;
}

std::vector<std::int32_t> Yolact::tracks() {
    if (!engine_) expect_failed("tracks", "the detection tail belongs to the YOLACT engine");
    std::int32_t m = 0;
    if (yh_instance_tracks_read(engine_, &m, nullptr, 0) != YH_OK) expect_failed("must data", yh_last_error(engine_));
    std::vector<std::int32_t> table(static_cast<std::size_t>(m) * 6);
    if (yh_instance_tracks_read(engine_, &m, table.data(), m) != YH_OK) expect_failed("must data", yh_last_error(engine_));
    return table;
}

void Yolact::track_reset(int stream) {
    if (!engine_) expect_failed("track_reset", "the detection tail belongs to the YOLACT engine");
    if (yh_instance_track_reset_stream(engine_, stream) != YH_OK) expect_failed("track reset failed", yh_last_error(engine_));
}

std::vector<std::vector<std::int32_t>> Yolact::instance_track_batch(int first, int n, int width, int height, const std::uint8_t* class_map,
                                                                    float min_score, int iou_permille, int max_age,
                                                                    const std::int32_t* streams, std::uint32_t* frames_out) {
    if (!engine_) expect_failed("instance_track_batch", "the detection tail belongs to the YOLACT engine");
    if (yh_instance_track_batch(engine_, first, n, width, height, class_map, min_score, iou_permille, max_age, streams, frames_out) != YH_OK)
        expect_failed("instance track batch failed", yh_last_error(engine_));
    std::vector<std::vector<std::int32_t>> tables(static_cast<std::size_t>(n));
    for (int b = 0; b < n; ++b) {
        std::int32_t m = 0;
        if (yh_instance_batch_read(engine_, b, &m, nullptr, 0) != YH_OK) expect_failed("must data", yh_last_error(engine_));
        tables[b].resize(static_cast<std::size_t>(m) * 4);
        if (yh_instance_batch_read(engine_, b, &m, tables[b].data(), m) != YH_OK) expect_failed("must data", yh_last_error(engine_));
    }
    return tables;
}

std::vector<std::int32_t> Yolact::tracks_of(int b) {
    if (!engine_) expect_failed("tracks_of", "the detection tail belongs to the YOLACT engine");
    std::int32_t m = 0;
    if (yh_instance_track_batch_read(engine_, b, &m, nullptr, 0) != YH_OK) expect_failed("must data", yh_last_error(engine_));
    std::vector<std::int32_t> table(static_cast<std::size_t>(m) * 6);
    if (yh_instance_track_batch_read(engine_, b, &m, table.data(), m) != YH_OK) expect_failed("must data", yh_last_error(engine_));
    return table;
}

// ---- YolactGroup ---------------------------------------------------------------------------------------------------
YolactGroup YolactGroup::init(const GroupOptions& opt) {
    YolactGroup y;
    y.opt_ = opt;
    yh_config cfg;
    yh_default_config(&cfg);
    cfg.input_size = opt.input_size;
    cfg.backbone = opt.backbone;
    cfg.max_batch = opt.frames_per_member;
    cfg.precision = opt.precision;
    y.max_dets_ = cfg.max_dets;
    std::vector<std::int32_t> devs(opt.devices.begin(), opt.devices.end());
    if (yh_group_create(&cfg, devs.data(), static_cast<std::int32_t>(devs.size()), &y.g_) != YH_OK)
        expect_failed("must create interpreter builder", yh_group_last_error(nullptr));                     // yolact.rs:25, once per device
    yh_engine* m0 = yh_group_member(y.g_, 0);
    const std::size_t n = yh_weights_nbytes(m0);
    std::vector<unsigned char> blob(n);
    if (yh_weights_generate(m0, opt.seed, blob.data(), n) != YH_OK) expect_failed("failed to load model", yh_last_error(m0));   // :20
    if (yh_group_load_weights_host(y.g_, blob.data(), n) != YH_OK) expect_failed("failed to allocate tensors.", yh_group_last_error(y.g_));   // :35
    std::int32_t pd[2] = {0, 0};
    yh_proto_dims(m0, pd);
    y.hp_ = pd[0]; y.wp_ = pd[1];
    // allocate_tensors() (yolact.rs:35) for the full-capacity call: every member's step is captured now, on this thread, one member
    // after the other - no capture is left for the frame loop (fp8 precision: after the calibration instead, see prepare())
    if (opt.precision == YH_PRECISION_F16) y.prepare(y.capacity());
    return y;
}

void YolactGroup::prepare(int n_frames) {
    if (yh_group_prepare(g_, n_frames, 1) != YH_OK) expect_failed("failed to allocate tensors.", yh_group_last_error(g_));   // yolact.rs:35
}

YolactGroup::YolactGroup(YolactGroup&& o) noexcept : g_(o.g_), opt_(std::move(o.opt_)), hp_(o.hp_), wp_(o.wp_), max_dets_(o.max_dets_) { o.g_ = nullptr; }
YolactGroup::~YolactGroup() { if (g_) yh_group_destroy(g_); }
int YolactGroup::members() const { return yh_group_size(g_); }
std::string YolactGroup::weights_replication() const { return yh_group_weights_replication(g_); }

void YolactGroup::evaluate(const std::uint8_t* frames, int n) {
    if (yh_group_evaluate(g_, frames, n, 1) != YH_OK) expect_failed("invoke failed", yh_group_last_error(g_));   // yolact.rs:163
}

FrameDetections YolactGroup::detections(int frame, bool want_masks) {
    FrameDetections out;
    out.dets.resize(static_cast<std::size_t>(max_dets_));
    if (want_masks) out.masks.resize(static_cast<std::size_t>(max_dets_) * hp_ * wp_);
    std::int32_t nd = 0;
    if (yh_group_read_detections(g_, frame, &nd, out.dets.data(), max_dets_, want_masks ? out.masks.data() : nullptr, out.masks.size()) != YH_OK)
        expect_failed("must data", yh_group_last_error(g_));                                                 // yolact.rs:173,:180
    out.dets.resize(static_cast<std::size_t>(nd));
    if (want_masks) out.masks.resize(static_cast<std::size_t>(nd) * hp_ * wp_);
    return out;
}

void YolactGroup::sync() {
    if (yh_group_sync(g_) != YH_OK) expect_failed("invoke failed", yh_group_last_error(g_));
}

}  // namespace tod
