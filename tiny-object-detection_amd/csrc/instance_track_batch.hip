// instance_track_batch.hip - yh_instance_track_batch: n frames of the last yh_evaluate tracked, each against the tracker of its camera
// stream, with one wait (DESIGN.md section 11 "Instance track batch"). The definition is the single call's (instance_track.hip, steps
// 1 - 8): the batch is exactly n yh_instance_track calls in batch order, frame b on the tracker of streams[b]. Frames of different
// streams are independent and share a launch; frames of one stream are a chain on the device, in the order of the handle's stream.
// The schedule is rounds: frame b's round is the number of earlier frames of the batch on its stream, R = the largest round + 1.
//   inst_track_sweep  round r = 0 .. R, grid z = the streams with a frame in round r or r - 1: per prototype pixel it applies the
//                     update of the stream's frame of round r - 1 (T' = (T & keep) | permute(C_prev), inst_retrack's body), stores T'
//                     and accumulates I = T'^T C_cur and A of the stream's frame of round r (inst_overlap's body) in the same pass;
//   inst_track_match  round r < R, grid z = the frames of round r: inst_match's body on the frame's matrix, its values and its
//                     stream's state, then a copy of the slots and their ranks into the frame's snapshot for the read-back.
// Both take stream and frames from a descriptor table the host uploads once per call; the bodies are instance_track_dev.h's, there
// is no second definition of anything. Around them instance_batch.hip's inst_batch_pack and inst_batch_paint run as they are: a
// tracked batch is an instance batch whose ids come from the trackers.
#include <string.h>

#include "engine.h"
#include "instance_dev.h"
#include "instance_track_dev.h"

using namespace yh;

namespace {

// One stream in one round: its track image and state, its frame of this round and of the round before (-1: none; never both).
struct TrkDesc { uint4* img; int32_t* st; int32_t cur, prev; };
constexpr int kDescMax = 2 * kTrkStreams;   // a frame is `cur` in its round and `prev` in the next: at most two entries per frame

// grid (min(ceil(px / 256), kTrkOvGridMax), 1, entries of the round), a lane = a prototype pixel per round of its loop.
// bits [n][px], ov [n][kTrkOvInts]. Whether an entry has a frame on either side is uniform in the workgroup.
__global__ void __launch_bounds__(kTrkOvLanes) inst_track_sweep(const TrkDesc* __restrict__ desc, const uint4* __restrict__ bits, int px,
                                                                uint32_t* __restrict__ ov) {
    __shared__ int s_map[kTrkRanks];
    __shared__ uint32_t s_keep[4];
    const TrkDesc d = desc[blockIdx.z];
    const int t = threadIdx.x;
    const bool has_prev = d.prev >= 0, has_cur = d.cur >= 0;
    const uint4* cprev = bits + (size_t)(has_prev ? d.prev : 0) * px;
    const uint4* ccur = bits + (size_t)(has_cur ? d.cur : 0) * px;
    if (has_prev) inst_retrack_maps(d.st, s_map, s_keep);
    uint32_t acc[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) acc[j] = 0;
    uint32_t area = 0;
    const int groups = (px + kTrkOvLanes - 1) / kTrkOvLanes;
    for (int g = blockIdx.x; g < groups; g += gridDim.x) {
        const int q = g * kTrkOvLanes + t;
        uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
        if (q < px) {
            a = d.img[q];
            if (has_prev) {
                a = inst_retrack_pixel(a, cprev[q], s_map, s_keep);
                d.img[q] = a;
            }
            if (has_cur) b = ccur[q];
        }
        if (has_cur) inst_overlap_group(a, b, acc, area);
    }
    if (has_cur) inst_overlap_merge(acc, area, ov + (size_t)d.cur * kTrkOvInts);
}

// grid (1, 1, frames of the round): the entries with a frame come first in a round's descriptors. meta [n][2][128], snap [n][kTrkStRead].
__global__ void __launch_bounds__(kTrkMatchLanes) inst_track_match(const TrkDesc* __restrict__ desc, const uint32_t* __restrict__ ov,
                                                                   uint32_t* __restrict__ meta, int32_t* __restrict__ snap,
                                                                   int iou_permille, int max_age) {
    const TrkDesc d = desc[blockIdx.z];
    const size_t cur = (size_t)d.cur;
    inst_match_body(ov + cur * kTrkOvInts, meta + cur * 2 * kInstRanks, d.st, iou_permille, max_age);
    const int t = threadIdx.x;
    if (t < kTrkRanks) {                                                        // (what this lane stored itself)
        int32_t* o = snap + cur * kTrkStRead;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[kTrkStSlots + 4 * t + k] = d.st[kTrkStSlots + 4 * t + k];
        o[kTrkStRankOf + t] = d.st[kTrkStRankOf + t];
    }
}

int stream_of(const InstTrackBatch& trk, int b) { return trk.streams ? trk.streams[b] : 0; }

}  // namespace

namespace yh {

std::string track_batch_check(int n, const int32_t* streams) {
    if (n > kTrkStreams) return "instance track batch: n_frames must be at most 64";
    if (streams)
        for (int b = 0; b < n; ++b)
            if (streams[b] < 0 || streams[b] >= kTrkStreams)
                return "instance track batch: the stream of frame " + std::to_string(b) + " is outside 0 .. 63";
    return std::string();
}

int track_batch_enqueue(yh_engine* h, int n, int hp, int wp, const InstTrackBatch& trk) {
    const int px = hp * wp;
    int rc;
    // the schedule: the frames of every stream in batch order; R rounds
    std::vector<int> frames_of[kTrkStreams];
    std::vector<int> named;                                                     // the streams in the order of their first frame
    int R = 0;
    for (int b = 0; b < n; ++b) {
        std::vector<int>& f = frames_of[stream_of(trk, b)];
        if (f.empty()) named.push_back(stream_of(trk, b));
        f.push_back(b);
        R = (int)f.size() > R ? (int)f.size() : R;
    }
    if ((rc = instance_grow(h, (void**)&h->trkb_ov, &h->trkb_ov_cap, (size_t)n * kTrkOvInts * 4))) return rc;
    if ((rc = instance_grow(h, (void**)&h->trkb_snap, &h->trkb_snap_cap, (size_t)n * kTrkStRead * 4))) return rc;
    if ((rc = instance_grow(h, &h->trkb_desc, &h->trkb_desc_cap, kDescMax * sizeof(TrkDesc)))) return rc;
    for (int s : named)
        if ((rc = track_prepare(h, s, hp, wp))) return rc;
    h->trkb_desc_host.resize(kDescMax * sizeof(TrkDesc));
    TrkDesc* desc = (TrkDesc*)h->trkb_desc_host.data();
    int off[kTrkStreams + 2], ncur[kTrkStreams + 1], total = 0;
    for (int r = 0; r <= R; ++r) {
        off[r] = total;
        for (int pass = 0; pass < 2; ++pass)                                    // the entries with a frame in this round first
            for (int s : named) {
                const std::vector<int>& f = frames_of[s];
                const int cur = r < (int)f.size() ? f[r] : -1, prev = r >= 1 && r - 1 < (int)f.size() ? f[r - 1] : -1;
                if ((pass == 0) != (cur >= 0) || (cur < 0 && prev < 0)) continue;
                desc[total++] = TrkDesc{ h->trk[s].img, h->trk[s].state, cur, prev };
            }
        ncur[r] = 0;
        for (int k = off[r]; k < total; ++k) ncur[r] += desc[k].cur >= 0 ? 1 : 0;
    }
    off[R + 1] = total;
    HIPCHK(h, hipMemcpyAsync(h->trkb_desc, desc, (size_t)total * sizeof(TrkDesc), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->trkb_ov, 0, (size_t)n * kTrkOvInts * 4, h->stream));
    const int groups = (px + kTrkOvLanes - 1) / kTrkOvLanes;
    const unsigned gx = (unsigned)(groups < kTrkOvGridMax ? groups : kTrkOvGridMax);
    const TrkDesc* dd = (const TrkDesc*)h->trkb_desc;
    for (int r = 0; r <= R; ++r) {
        hipLaunchKernelGGL(inst_track_sweep, dim3(gx, 1, (unsigned)(off[r + 1] - off[r])), dim3(kTrkOvLanes), 0, h->stream, dd + off[r],
                           (const uint4*)h->instb_bits, px, h->trkb_ov);
        if (r < R)
            hipLaunchKernelGGL(inst_track_match, dim3(1, 1, (unsigned)ncur[r]), dim3(kTrkMatchLanes), 0, h->stream, dd + off[r],
                               (const uint32_t*)h->trkb_ov, h->instb_meta, h->trkb_snap, trk.p.iou_permille, trk.p.max_age);
    }
    HIPCHK(h, hipGetLastError());
    for (int s : named) h->trk[s].live = true;
    return YH_OK;
}

int track_batch_readback(yh_engine* h, int n) {
    h->trkb_snap_host.resize((size_t)n * kTrkStRead);
    HIPCHK(h, hipMemcpyAsync(h->trkb_snap_host.data(), h->trkb_snap, (size_t)n * kTrkStRead * 4, hipMemcpyDeviceToHost, h->stream));
    return YH_OK;
}

void track_batch_finish(yh_engine* h, int n, const InstTrackBatch& trk) {
    h->trkb_tables.resize((size_t)n);
    for (int b = 0; b < n; ++b) {                                               // (in batch order: a stream keeps its last frame's table)
        track_rows(h->trkb_snap_host.data() + (size_t)b * kTrkStRead, h->trkb_tables[b]);
        TrkStream& s = h->trk[stream_of(trk, b)];
        s.table = h->trkb_tables[b];
        s.rows = (int)(s.table.size() / 6);
    }
    h->trkb_n = n;
}

void track_batch_drop(yh_engine* h, int n, const InstTrackBatch& trk) {
    for (int b = 0; b < n; ++b) track_drop(h, stream_of(trk, b));
}

void track_batch_free(yh_engine* h) {
    void* bufs[] = { h->trkb_ov, h->trkb_snap, h->trkb_desc };
    for (void* b : bufs) if (b) hipFree(b);
}

}  // namespace yh

extern "C" {

int yh_instance_track_batch(yh_engine* h, int32_t first_frame, int32_t n_frames, int32_t width, int32_t height, const uint8_t* class_map,
                            float min_score, int32_t iou_permille, int32_t max_age, const int32_t* streams, uint32_t* out_host) {
    if (!h) return YH_EINVAL;
    if (!h->dets_valid) return h->fail(YH_ESTATE, "instance track batch: the handle's last step was not a yh_evaluate");
    if (n_frames < 1) return h->fail(YH_EINVAL, "instance track batch: n_frames must be at least 1");
    if (first_frame < 0 || first_frame >= h->cur_n || n_frames > h->cur_n - first_frame)
        return h->fail(YH_EINVAL, "instance track batch: frames outside the last step's batch");
    if (const char* why = instance_check(width, height, class_map, h->C - 1, min_score)) return h->fail(YH_EINVAL, why);
    if (const char* why = track_check(iou_permille, max_age)) return h->fail(YH_EINVAL, why);
    const std::string why = track_batch_check(n_frames, streams);
    if (!why.empty()) return h->fail(YH_EINVAL, why);
    HIPCHK(h, hipSetDevice(h->dev));
    TraceRange tr("yh_instance_track_batch");
    const size_t px = (size_t)h->hp * h->wp, md = (size_t)h->cfg.max_dets;
    const InstTrackBatch trk = { { iou_permille, max_age }, streams };
    return instance_batch_run(h, h->det.masks + (size_t)first_frame * md * px, h->det.dets + (size_t)first_frame * md,
                              h->det.det_count + first_frame, (int)md, n_frames, h->hp, h->wp, width, height, class_map, min_score,
                              out_host, &trk);
}

int yh_instance_track_batch_read(yh_engine* h, int32_t frame, int32_t* n_tracks, int32_t* table, int32_t capacity) {
    if (!h || !n_tracks) return YH_EINVAL;
    if (h->trkb_n < 1 || h->instb_n < 1) return h->fail(YH_ESTATE, "track batch table: the last instance batch was not a tracked one");
    if (frame < 0 || frame >= h->trkb_n) return h->fail(YH_EINVAL, "track batch table: frame outside the last batch");
    const std::vector<int32_t>& t = h->trkb_tables[(size_t)frame];
    *n_tracks = (int32_t)(t.size() / 6);
    if (!table) return YH_OK;
    if (capacity < *n_tracks) return h->fail(YH_EOVERFLOW, "track batch table: capacity too small");
    memcpy(table, t.data(), t.size() * sizeof(int32_t));
    return YH_OK;
}

}  // extern "C"
