// instance_track.hip - instance tracks (DESIGN.md section 11 "Instance tracks"): the eligible detections of a frame associated with
// the tracker's live slots by mask overlap at prototype resolution, so that the instance frame carries ids that persist. A tracked
// call is inst_pack (instance.hip, as it is), the three kernels below, then inst_paint (as it is), all on the handle's stream:
//   inst_overlap  I[s][c] = |T_s AND C_c| and A_c = |C_c| from the two 128-bit set images: a wave transposes 64 pixels' sets into 64-bit
//                 pixel masks per slot and per rank with ballots, the workgroup sums popcounts in registers, one atomicAdd per entry;
//   inst_match    one workgroup: candidates, the greedy match (as rounds of mutually best pairs), ageing, room, births; it overwrites
//                 meta[rank] with the tracked class << 24 | id << 16 and writes the rank -> slot map and the slot table;
//   inst_retrack  per prototype pixel T' = (T & keep) | permute(C).
// All arithmetic is integer: tests/track_ref.py restates it and every result is compared with array_equal. The handle holds a bank
// of trackers (TrkStream, engine.h); the calls here advance stream 0, instance_track_batch.hip advances any of them.
#include <string.h>

#include "engine.h"
#include "instance_track_dev.h"

using namespace yh;

namespace {

constexpr int kRanks = kTrkRanks, kOvLanes = kTrkOvLanes, kOvGridMax = kTrkOvGridMax, kMatchLanes = kTrkMatchLanes,
              kRetrackLanes = kTrkRetrackLanes;
constexpr int kStSlots = kTrkStSlots, kStRankOf = kTrkStRankOf, kStInts = kTrkStInts, kStRead = kTrkStRead, kOvInts = kTrkOvInts;

// The bodies of the three kernels are instance_track_dev.h's (instance_track_batch.hip runs the same ones per stream and frame).
// grid min(ceil(px / 256), kOvGridMax), a lane = a prototype pixel per round
__global__ void __launch_bounds__(kOvLanes) inst_overlap(const uint4* __restrict__ trk, const uint4* __restrict__ bits, int px,
                                                         uint32_t* __restrict__ ov) {
    inst_overlap_body(trk, bits, px, ov);
}

// One workgroup.
__global__ void __launch_bounds__(kMatchLanes) inst_match(const uint32_t* __restrict__ ov, uint32_t* __restrict__ meta,
                                                          int32_t* __restrict__ st, int iou_permille, int max_age) {
    inst_match_body(ov, meta, st, iou_permille, max_age);
}

// grid ceil(px / 256), a lane per prototype pixel
__global__ void __launch_bounds__(kRetrackLanes) inst_retrack(uint4* __restrict__ trk, const uint4* __restrict__ bits, int px,
                                                              const int32_t* __restrict__ st) {
    inst_retrack_body(trk, bits, px, st);
}

void drop(yh_engine* h, int stream) {
    TrkStream& s = h->trk[stream];
    s.live = false;
    if (s.rows >= 0) { s.rows = 0; s.table.clear(); }
}

}  // namespace

namespace yh {

const char* track_check(int iou_permille, int max_age) {
    if (iou_permille < 1 || iou_permille > 1000) return "instance track: iou_permille must be in 1 .. 1000";
    if (max_age < 0 || max_age > 255) return "instance track: max_age must be in 0 .. 255";
    return nullptr;
}

// A stream's buffers are its own, so the first use of one stream moves nothing of another that is live.
int track_prepare(yh_engine* h, int stream, int hp, int wp) {
    TrkStream& s = h->trk[stream];
    const size_t px = (size_t)hp * wp;
    if (!s.state && hipMalloc((void**)&s.state, kStInts * 4) != hipSuccess) return h->fail(YH_ENOMEM, "hipMalloc instance tracks");
    if (!s.live || s.hp != hp || s.wp != wp) {                                 // an empty tracker at this prototype size
        drop(h, stream);
        if (px * 16 > s.img_cap) {
            if (s.img) hipFree(s.img);
            s.img = nullptr; s.img_cap = 0;
            if (hipMalloc((void**)&s.img, px * 16) != hipSuccess) return h->fail(YH_ENOMEM, "hipMalloc instance tracks");
            s.img_cap = px * 16;
        }
        HIPCHK(h, hipMemsetAsync(s.img, 0, px * 16, h->stream));
        HIPCHK(h, hipMemsetAsync(s.state, 0, kStInts * 4, h->stream));
        s.hp = hp; s.wp = wp;
    }
    return YH_OK;
}

int track_enqueue(yh_engine* h, int hp, int wp, const InstTrack& trk) {
    const int px = hp * wp;
    static_assert(sizeof h->trk_host == kStRead * 4, "trk_host holds the slots and their ranks");
    if (!h->trk_ov && hipMalloc((void**)&h->trk_ov, kOvInts * 4) != hipSuccess) return h->fail(YH_ENOMEM, "hipMalloc instance tracks");
    if (const int rc = track_prepare(h, 0, hp, wp)) return rc;
    TrkStream& s = h->trk[0];
    HIPCHK(h, hipMemsetAsync(h->trk_ov, 0, kOvInts * 4, h->stream));
    const int groups = (px + kOvLanes - 1) / kOvLanes;
    hipLaunchKernelGGL(inst_overlap, dim3((unsigned)(groups < kOvGridMax ? groups : kOvGridMax)), dim3(kOvLanes), 0, h->stream,
                       (const uint4*)s.img, (const uint4*)h->inst_bits, px, h->trk_ov);
    hipLaunchKernelGGL(inst_match, dim3(1), dim3(kMatchLanes), 0, h->stream, (const uint32_t*)h->trk_ov, h->inst_meta, s.state,
                       trk.iou_permille, trk.max_age);
    hipLaunchKernelGGL(inst_retrack, dim3((unsigned)((px + kRetrackLanes - 1) / kRetrackLanes)), dim3(kRetrackLanes), 0, h->stream,
                       s.img, (const uint4*)h->inst_bits, px, (const int32_t*)s.state);
    HIPCHK(h, hipGetLastError());
    s.live = true;
    return YH_OK;
}

int track_readback(yh_engine* h) {
    HIPCHK(h, hipMemcpyAsync(h->trk_host, h->trk[0].state, sizeof h->trk_host, hipMemcpyDeviceToHost, h->stream));
    return YH_OK;
}

void track_rows(const int32_t* st, std::vector<int32_t>& table) {
    table.clear();
    for (int s = 0; s < kRanks; ++s)
        if (st[kStSlots + 4 * s] != 0) {
            const int32_t row[6] = { s, st[4 * s], st[4 * s + 1], st[4 * s + 2], st[4 * s + 3], st[kStRankOf + s] };
            table.insert(table.end(), row, row + 6);
        }
}

void track_finish(yh_engine* h) {
    track_rows(h->trk_host, h->trk[0].table);
    h->trk[0].rows = (int)(h->trk[0].table.size() / 6);
}

void track_drop(yh_engine* h, int stream) { drop(h, stream); }

void track_free(yh_engine* h) {
    for (TrkStream& s : h->trk) {
        if (s.img) hipFree(s.img);
        if (s.state) hipFree(s.state);
    }
    if (h->trk_ov) hipFree(h->trk_ov);
    track_batch_free(h);
}

}  // namespace yh

extern "C" {

int yh_instance_track(yh_engine* h, int32_t frame, int32_t width, int32_t height, const uint8_t* class_map, float min_score,
                      int32_t iou_permille, int32_t max_age, uint32_t* out_host) {
    if (!h) return YH_EINVAL;
    if (!h->dets_valid) return h->fail(YH_ESTATE, "instance track: the handle's last step was not a yh_evaluate");
    if (frame < 0 || frame >= h->cur_n) return h->fail(YH_EINVAL, "instance track: frame out of range");
    if (const char* why = instance_check(width, height, class_map, h->C - 1, min_score)) return h->fail(YH_EINVAL, why);
    if (const char* why = track_check(iou_permille, max_age)) return h->fail(YH_EINVAL, why);
    HIPCHK(h, hipSetDevice(h->dev));
    TraceRange tr("yh_instance_track");
    const size_t px = (size_t)h->hp * h->wp, md = (size_t)h->cfg.max_dets;
    const InstTrack trk = { iou_permille, max_age };
    return instance_run(h, h->det.masks + (size_t)frame * md * px, h->det.dets + (size_t)frame * md, h->det.det_count + frame, (int)md,
                        h->hp, h->wp, width, height, class_map, min_score, out_host, &trk);
}

int yh_instance_tracks_read(yh_engine* h, int32_t* n_tracks, int32_t* table, int32_t capacity) {
    if (!h || !n_tracks) return YH_EINVAL;
    const TrkStream& s = h->trk[0];
    if (s.rows < 0) return h->fail(YH_ESTATE, "track table: no tracked call yet");
    *n_tracks = s.rows;
    if (!table) return YH_OK;
    if (capacity < s.rows) return h->fail(YH_EOVERFLOW, "track table: capacity too small");
    memcpy(table, s.table.data(), s.table.size() * sizeof(int32_t));
    return YH_OK;
}

int yh_instance_track_reset(yh_engine* h) {
    if (!h) return YH_EINVAL;
    drop(h, 0);
    return YH_OK;
}

int yh_instance_track_reset_stream(yh_engine* h, int32_t stream) {
    if (!h) return YH_EINVAL;
    if (stream < -1 || stream >= kTrkStreams) return h->fail(YH_EINVAL, "instance track reset: stream must be -1 (all) or in 0 .. 63");
    for (int s = 0; s < kTrkStreams; ++s)
        if (stream < 0 || stream == s) drop(h, s);
    return YH_OK;
}

}  // extern "C"
