// rccl.hip - the weight broadcast: the library's one collective, bound to librccl by name at first use.
#include <dlfcn.h>
#include <string.h>

#include "engine.h"

using namespace yh;

namespace yh {
static std::atomic<int> g_rccl_shared_device{0};
bool rccl_shared_device_allowed() { return g_rccl_shared_device.load() != 0; }
}  // namespace yh

extern "C" {

// ---- multi-GPU: the path's ONE collective, behind the C ABI --------------------------------------------
// SURVEY.md §8e / north_star: frames shard over the GPUs of a node with no per-step collective; the weights are
// replicated once by an RCCL broadcast over xGMI. The reference's caller is a Rust process (src/main.rs:63-75),
// not torch, so the broadcast lives here. librccl.so (573 MB) is opened on first use only; the symbols are
// declared locally (rccl.h: ncclUniqueId = 128 opaque bytes, ncclUint8 = 1, ncclSuccess = 0).
namespace {
struct RcclId { char internal[YH_RCCL_ID_BYTES]; };
typedef void* rccl_comm;
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(RcclId*) = nullptr;
    int (*CommInitRank)(rccl_comm*, int, RcclId, int) = nullptr;
    int (*CommInitAll)(rccl_comm*, int, const int*) = nullptr;
    int (*CommDestroy)(rccl_comm) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, rccl_comm, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string err;
};
void rccl_open(Rccl& r);
std::atomic<int> g_rccl_opened{0};
std::string& rccl_path_override() { static std::string s; return s; }   // yh_debug_rccl_library (tests: the stand-in of tests/rccl_standin/, by path)
Rccl* rccl() {   // opened once per process (thread-safe: C++11 static initialisation); a failed open is remembered with its reason
    static Rccl r = [] { Rccl x; g_rccl_opened.store(1); rccl_open(x); return x; }();
    return &r;
}
void rccl_open(Rccl& r) {
    if (!rccl_path_override().empty()) r.lib = dlopen(rccl_path_override().c_str(), RTLD_NOW | RTLD_LOCAL);
    else
        for (const char* name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" }) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (r.lib) break;
        }
    if (!r.lib) { const char* why = dlerror(); r.err = std::string("dlopen librccl.so: ") + (why ? why : "not found"); return; }
    auto sym = [&](const char* n) { void* p = dlsym(r.lib, n); if (!p && r.err.empty()) r.err = std::string("librccl.so lacks ") + n; return p; };
    r.GetUniqueId = (int (*)(RcclId*))sym("ncclGetUniqueId");
    r.CommInitRank = (int (*)(rccl_comm*, int, RcclId, int))sym("ncclCommInitRank");
    r.CommInitAll = (int (*)(rccl_comm*, int, const int*))sym("ncclCommInitAll");
    r.CommDestroy = (int (*)(rccl_comm))sym("ncclCommDestroy");
    r.Broadcast = (int (*)(const void*, void*, size_t, int, int, rccl_comm, hipStream_t))sym("ncclBroadcast");
    r.GroupStart = (int (*)())sym("ncclGroupStart");
    r.GroupEnd = (int (*)())sym("ncclGroupEnd");
    r.GetErrorString = (const char* (*)(int))sym("ncclGetErrorString");
}
extern "C++" std::string rccl_msg(Rccl* r, const char* what, int rc) { return std::string(what) + ": " + (r->GetErrorString ? r->GetErrorString(rc) : "error"); }
// after the receive: validate and repack exactly as yh_load_weights_device does
int adopt_received_blob(yh_engine* h) {
    std::vector<uint8_t> host(h->blob_bytes);
    HIPCHK(h, hipMemcpy(host.data(), h->blob_dev, h->blob_bytes, hipMemcpyDeviceToHost));
    const int rc = check_blob(h, host.data(), h->blob_bytes);
    if (rc) return rc;
    return upload_panels(h, host.data());
}
}  // namespace

int yh_rccl_unique_id(void* id_out) {
    if (!id_out) return YH_EINVAL;
    Rccl* r = rccl();
    if (!r->err.empty()) { create_error() = r->err; return YH_EHIP; }
    RcclId id;
    const int rc = r->GetUniqueId(&id);
    if (rc) { create_error() = rccl_msg(r, "ncclGetUniqueId", rc); return YH_EHIP; }
    memcpy(id_out, &id, sizeof id);
    return YH_OK;
}

int yh_rank_broadcast_weights(yh_engine* h, const void* id_bytes, int32_t rank, int32_t nranks, int32_t root) {
    if (!h || !id_bytes) return YH_EINVAL;
    if (nranks < 1 || rank < 0 || rank >= nranks || root < 0 || root >= nranks) return h->fail(YH_EINVAL, "rank / nranks / root out of range");
    if (rank == root && !h->weights_loaded) return h->fail(YH_ESTATE, "the root rank must have its weights loaded before the broadcast");
    Rccl* r = rccl();
    if (!r->err.empty()) return h->fail(YH_EHIP, r->err);
    HIPCHK(h, hipSetDevice(h->dev));
    // non-root: the receive buffer. (Round 5, the first execution with two ranks - behind the stand-in librccl of tests/rccl_standin/ -
    // found this line as keep_blob(h, h->blob_dev, ...): the argument was read, still null, before the allocation inside, and every
    // rank that had never held weights failed with "hipMemcpy: invalid argument" - the path could not have worked on an 8-GPU node.)
    int rc = rank == root ? YH_OK : ensure_blob(h);
    if (rc) return rc;
    RcclId id;
    memcpy(&id, id_bytes, sizeof id);
    rccl_comm comm = nullptr;
    int e = r->CommInitRank(&comm, nranks, id, rank);
    if (e) return h->fail(YH_EHIP, rccl_msg(r, "ncclCommInitRank", e));
    e = r->Broadcast(h->blob_dev, h->blob_dev, h->blob_bytes, /*ncclUint8*/ 1, root, comm, h->stream);
    const hipError_t se = hipStreamSynchronize(h->stream);
    r->CommDestroy(comm);
    if (e) return h->fail(YH_EHIP, rccl_msg(r, "ncclBroadcast", e));
    if (se != hipSuccess) return h->fail(YH_EHIP, std::string("weight broadcast: ") + hipGetErrorString(se));
    return rank == root ? YH_OK : adopt_received_blob(h);
}

int yh_group_broadcast_weights(yh_engine** hs, int32_t n, int32_t root) {
    if (!hs || n < 1 || root < 0 || root >= n) return YH_EINVAL;
    for (int i = 0; i < n; ++i) if (!hs[i]) return YH_EINVAL;
    yh_engine* h0 = hs[root];
    if (!h0->weights_loaded) return h0->fail(YH_ESTATE, "the root handle must have its weights loaded before the broadcast");
    for (int i = 0; i < n; ++i) {
        if (hs[i]->blob_bytes != h0->blob_bytes) return h0->fail(YH_EINVAL, "handles of one group must share the architecture");
        for (int j = 0; j < i; ++j) if (hs[j]->dev == hs[i]->dev && !yh::rccl_shared_device_allowed()) return h0->fail(YH_EINVAL, "one handle per device: RCCL refuses two ranks on one GPU");
    }
    if (n == 1) return YH_OK;
    Rccl* r = rccl();
    if (!r->err.empty()) return h0->fail(YH_EHIP, r->err);
    std::vector<int> devs(n);
    for (int i = 0; i < n; ++i) {
        devs[i] = hs[i]->dev;
        if (i != root) {
            if (hipSetDevice(hs[i]->dev) != hipSuccess) return h0->fail(YH_EHIP, "hipSetDevice failed for handle " + std::to_string(i));
            const int rc = ensure_blob(hs[i]);
            if (rc) return h0->fail(rc, "handle " + std::to_string(i) + ": " + hs[i]->err);   // (the caller reads the ROOT handle's error)
        }
    }
    std::vector<rccl_comm> comms(n, nullptr);
    int e = r->CommInitAll(comms.data(), n, devs.data());
    if (e) return h0->fail(YH_EHIP, rccl_msg(r, "ncclCommInitAll", e));
    e = r->GroupStart();   // one thread drives every device: the n broadcasts must be one group
    for (int i = 0; i < n && !e; ++i) e = r->Broadcast(hs[i]->blob_dev, hs[i]->blob_dev, h0->blob_bytes, 1, root, comms[i], hs[i]->stream);
    const int ge = r->GroupEnd();
    if (!e) e = ge;
    hipError_t se = hipSuccess;
    for (int i = 0; i < n; ++i) { hipSetDevice(hs[i]->dev); const hipError_t s1 = hipStreamSynchronize(hs[i]->stream); if (se == hipSuccess) se = s1; }
    for (rccl_comm c : comms) if (c) r->CommDestroy(c);
    if (e) return h0->fail(YH_EHIP, rccl_msg(r, "ncclBroadcast (group)", e));
    if (se != hipSuccess) return h0->fail(YH_EHIP, std::string("weight broadcast: ") + hipGetErrorString(se));
    for (int i = 0; i < n; ++i)
        if (i != root) {
            if (hipSetDevice(hs[i]->dev) != hipSuccess) return h0->fail(YH_EHIP, "hipSetDevice failed for handle " + std::to_string(i));
            const int rc = adopt_received_blob(hs[i]);
            if (rc) return h0->fail(rc, "handle " + std::to_string(i) + ": " + hs[i]->err);
        }
    return YH_OK;
}

int yh_debug_rccl_library(const char* path) {
    if (!path || !*path) return YH_EINVAL;
    if (g_rccl_opened.load()) { create_error() = "librccl has already been opened in this process"; return YH_ESTATE; }
    rccl_path_override() = path;
    return YH_OK;
}

int yh_debug_rccl_shared_device(int32_t allow) { return yh::g_rccl_shared_device.exchange(allow ? 1 : 0); }

}  // extern "C"
