// group.hip — several GPUs behind ONE call ("ta_ctx_create(device_ids[], n_dev, &ctx)
// ... multi-GPU fan-out and the RCCL reduce happen inside the call"; 8(e): atoms are the sharded
// axis, one reduce of the (n_frames,) lag sums, by-particle blocks copied into column ranges of one
// host array).  One host thread, one frame loop: member i owns a ta_ctx on device_ids[i], stages
// and correlates atoms [A i / n, A (i + 1) / n) and the members' lag sums are added once:
//   n_dev = 1                      no reduce (and librccl is never loaded);
//   n_dev > 1, distinct devices    ncclReduce(sum, float64, n_frames) in one RCCL group call, the
//                                  communicators from ncclCommInitAll (one process, n devices);
//                                  librccl.so is dlopen'ed on first use;
//   otherwise (two members on one GPU -- what a one-GPU box can test -- or RCCL failing)
//                                  the members' vectors are copied to member 0's device
//                                  (hipMemcpyPeerAsync) and added there in member order.
// "reduce_mode" (ta_group_set_option; $TA_AMD_GROUP_REDUCE = auto | peer | rccl) overrides the choice:
// 1 = peer copies whatever the devices, 2 = RCCL or an error ("force_rccl" 1 is the same), which also
// runs the collective for ONE member: the only form of this branch a one-GPU box can execute.
// Replaces, for several GPUs at once, the same reference code as the single-context calls:
// velocityautocorr.py:142-153,178-238, viscosity.py:111-142,167-233 (the atom mean at
// velocityautocorr.py:214,237 / viscosity.py:233 is the reduce + one division).
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>  // types and prototypes only: librccl.so is dlopen'ed (struct Rccl)
#else  // a ROCm install without the RCCL development headers: the few declarations this file needs, as RCCL 2.x publishes them
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
typedef enum { ncclFloat64 = 8 } ncclDataType_t;
ncclResult_t ncclCommInitAll(ncclComm_t* comm, int ndev, const int* devlist);
ncclResult_t ncclCommDestroy(ncclComm_t comm);
ncclResult_t ncclCommAbort(ncclComm_t comm);
ncclResult_t ncclCommCount(const ncclComm_t comm, int* count);
ncclResult_t ncclReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op, int root,
                        ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclGroupStart(void);
ncclResult_t ncclGroupEnd(void);
const char* ncclGetErrorString(ncclResult_t result);
}
#endif

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ta_hip.h"
#include "ta_internal.hpp"
#include "unwrap_box.hpp"

using namespace ta;

namespace {

thread_local std::string g_group_tls_error;

// The RCCL entry points of the reduce, resolved from librccl.so when first needed (the library does
// not link librccl: a one-GPU user never loads it).  <rccl/rccl.h> is included for its TYPES only: every
// pointer below is declared as decltype(&ncclX), so a call through it is compiled against the
// header's own prototype, and the static_asserts pin the prototypes this file was written against
// (a header that reorders or retypes an argument fails the build instead of corrupting a call).
struct Rccl {
    void* handle = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;  // (optional: a library without it destroys the communicator instead)
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclReduce) Reduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool load(std::string* why) {
        if (handle) return true;
        const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names)
            if ((handle = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
        if (!handle) {
            const char* e = dlerror();
            *why = std::string("librccl.so not loadable: ") + (e ? e : "?");
            return false;
        }
        auto sym = [&](const char* n) { return dlsym(handle, n); };
        CommInitAll = (decltype(CommInitAll))sym("ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
        CommAbort = (decltype(CommAbort))sym("ncclCommAbort");
        CommCount = (decltype(CommCount))sym("ncclCommCount");
        Reduce = (decltype(Reduce))sym("ncclReduce");
        GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
        GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
        if (!CommInitAll || !CommDestroy || !Reduce || !GroupStart || !GroupEnd) {
            *why = "librccl.so lacks an entry point of the reduce";
            dlclose(handle);
            handle = nullptr;
            return false;
        }
        return true;
    }
    std::string what(ncclResult_t rc) const { return GetErrorString ? GetErrorString(rc) : "failed"; }
};
Rccl g_rccl;
static_assert(std::is_same_v<decltype(&ncclCommInitAll), ncclResult_t (*)(ncclComm_t*, int, const int*)>);
static_assert(std::is_same_v<decltype(&ncclCommDestroy), ncclResult_t (*)(ncclComm_t)>);
static_assert(std::is_same_v<decltype(&ncclCommCount), ncclResult_t (*)(const ncclComm_t, int*)>);
static_assert(std::is_same_v<decltype(&ncclReduce), ncclResult_t (*)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t,
                                                                     int, ncclComm_t, hipStream_t)>);
static_assert(std::is_same_v<decltype(&ncclGroupStart), ncclResult_t (*)()>);
static_assert(std::is_same_v<decltype(&ncclGroupEnd), ncclResult_t (*)()>);
static_assert(std::is_same_v<decltype(&ncclGetErrorString), const char* (*)(ncclResult_t)>);
static_assert(ncclFloat64 == 8 && ncclSum == 0 && ncclSuccess == 0);

// how the members' lag sums are added: "reduce_mode" option, $TA_AMD_GROUP_REDUCE = auto | peer | rccl
enum { RED_AUTO = 0, RED_PEER = 1, RED_RCCL = 2 };

}  // namespace

struct ta_group {
    std::vector<int> devices;
    std::vector<ta_ctx*> ctx;
    std::vector<int64_t> lo, hi;  // atom range of member i (after ta_group_stage_alloc)
    int64_t T = 0, A = 0;
    int D = 0, n_slabs = 0;
    bool distinct = true;          // all members on different devices
    std::vector<ncclComm_t> comms;  // RCCL communicators (distinct devices), created on first reduce
    bool rccl_tried = false;
    int reduce_mode = RED_AUTO;     // "reduce_mode" option / $TA_AMD_GROUP_REDUCE
    int rccl_ranks = 0;             // ncclCommCount of the communicator the last RCCL reduce ran on
    std::string reduce_kind = "none";
    std::string reduce_note;        // why RED_AUTO fell back to peer copies (empty: it did not)
    std::string err;
    // on the reducing member's device: [n + 1][T] rows for the copy-and-add reduce; events to order the devices
    double* d_rows = nullptr;
    size_t rows_bytes = 0;
    int rows_device = -1;
    std::vector<hipEvent_t> ev;
};

namespace {

int gfail(ta_group* g, int code, const std::string& msg) noexcept {
    try {
        if (g) g->err = msg;
        g_group_tls_error = msg;
    } catch (...) {
    }
    return code;
}
#define TAG_TRY(g, expr)                                                                             \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return gfail(g, e_ == hipErrorOutOfMemory ? TA_E_NOMEM : TA_E_HIP,                       \
                         std::string(#expr) + ": " + hipGetErrorString(e_));                         \
    } while (0)
// a member's failure, with its message
int mfail(ta_group* g, int i, int rc) {
    return gfail(g, rc, "device member " + std::to_string(i) + ": " + ta_last_error(g->ctx[i]));
}

void shard(int64_t A, int i, int n, int64_t* lo, int64_t* hi) {  // as transport_analysis_amd/dist.py:atom_shard
    *lo = A * i / n;
    *hi = A * (i + 1) / n;
}

// The (n_frames,) sums of the members `who` (d_tot[j] on member who[j]'s device, ready on that member's
// stream) -> their sum on member who[0]'s device, in d_tot[0], ready on that member's stream.
// RED_AUTO: RCCL when every member holds atoms on a device of its own (n > 1), peer copies when that
// fails (reduce_note says why) or does not apply; RED_PEER: peer copies; RED_RCCL: RCCL or an error --
// also for ONE member (ncclCommInitAll(1) + ncclReduce onto itself: what a one-GPU box can execute of
// this branch, tests/test_gpu_dist.py::test_group_forced_rccl_one_member).
int reduce_members(ta_group* g, const std::vector<int>& who, std::vector<double*>& d_tot) {
    const int n = (int)g->ctx.size(), m = (int)who.size();
    const int64_t T = g->T;
    const int mode = g->reduce_mode;
    if (m <= 1 && mode != RED_RCCL) {
        g->reduce_kind = "none";
        return TA_OK;
    }
    const bool rccl_applies = m == n && g->distinct;
    if (mode == RED_RCCL && !rccl_applies)
        return gfail(g, TA_E_UNSUPPORTED, "reduce_mode rccl: every member needs atoms and a device of its own");
    if (mode != RED_PEER && rccl_applies && !g->rccl_tried) {
        g->rccl_tried = true;
        std::string why;
        if (g_rccl.load(&why)) {
            g->comms.assign(n, nullptr);
            const ncclResult_t rc = g_rccl.CommInitAll(g->comms.data(), n, g->devices.data());
            if (rc != ncclSuccess) {
                g->comms.clear();
                why = "ncclCommInitAll: " + g_rccl.what(rc);
            }
        }
        g->reduce_note = why;
    }
    if (mode != RED_PEER && rccl_applies && !g->comms.empty()) {
        // ONE collective: every member's vector is added into member 0's (in place on the root).  Nothing
        // returns between ncclGroupStart and ncclGroupEnd: an open group on this thread would swallow
        // every later RCCL call made from it (the caller's torch.distributed ones included).
        ncclResult_t rc = g_rccl.GroupStart();
        hipError_t he = hipSuccess;
        int launched = 0;  // calls RCCL accepted inside the group
        if (rc == ncclSuccess) {
            for (int i = 0; i < n && rc == ncclSuccess && he == hipSuccess; ++i) {
                he = hipSetDevice(g->devices[i]);
                if (he == hipSuccess) {
                    rc = g_rccl.Reduce(d_tot[i], d_tot[i], (size_t)T, ncclFloat64, ncclSum, 0, g->comms[i],
                                       ctx_stream(g->ctx[i]));
                    if (rc == ncclSuccess) ++launched;
                }
            }
            const ncclResult_t rc2 = g_rccl.GroupEnd();
            if (rc == ncclSuccess) rc = rc2;
        }
        if (rc == ncclSuccess && he == hipSuccess) {
            int cnt = 0;
            if (g_rccl.CommCount && g_rccl.CommCount(g->comms[0], &cnt) == ncclSuccess) g->rccl_ranks = cnt;
            g->reduce_kind = "rccl";
            return TA_OK;
        }
        const std::string why = he != hipSuccess ? std::string("hipSetDevice: ") + hipGetErrorString(he)
                                                 : "ncclReduce: " + g_rccl.what(rc);
        if (mode == RED_RCCL) return gfail(g, TA_E_HIP, why);
        // RED_AUTO.  Falling back to peer copies is only safe when NOTHING of the collective was enqueued: the reduce is
        // in place on the root's vector, and ncclGroupEnd launches whatever calls were accepted before the failing one.
        // That is the case when ncclGroupStart itself failed, or the very first member's hipSetDevice / ncclReduce did
        // (`launched` counts the calls RCCL accepted).  Otherwise the members' sums may be half-reduced and their streams
        // may wait on ranks that never arrive: the communicators are aborted and the call fails.
        if (launched > 0) {
            for (ncclComm_t c : g->comms)
                if (c) (void)(g_rccl.CommAbort ? g_rccl.CommAbort(c) : g_rccl.CommDestroy(c));
            g->comms.clear();
            g->reduce_note = why;
            return gfail(g, TA_E_HIP, "RCCL reduce failed after " + std::to_string(launched) + " of " + std::to_string(n) +
                                          " ranks had joined (" + why + "): the lag sums are not trustworthy; re-run with reduce_mode 1 (peer copies)");
        }
        for (ncclComm_t c : g->comms)
            if (c) (void)g_rccl.CommDestroy(c);
        g->comms.clear();
        g->reduce_note = why;
    } else if (mode == RED_RCCL) {
        return gfail(g, TA_E_HIP, "reduce_mode rccl: " + (g->reduce_note.empty() ? std::string("no communicator") : g->reduce_note));
    }
    if (m <= 1) {
        g->reduce_kind = "none";
        return TA_OK;
    }
    // copy-and-add on the first member's device, in member order (bitwise reproducible)
    const int root = who[0];
    TAG_TRY(g, hipSetDevice(g->devices[root]));
    const size_t need = sizeof(double) * (size_t)T * (n + 1);
    if (g->rows_bytes < need || g->rows_device != g->devices[root]) {
        if (g->d_rows) {
            (void)hipSetDevice(g->rows_device);
            (void)hipFree(g->d_rows);
            (void)hipSetDevice(g->devices[root]);
        }
        g->d_rows = nullptr, g->rows_bytes = 0;
        TAG_TRY(g, hipMalloc((void**)&g->d_rows, need));
        g->rows_bytes = need, g->rows_device = g->devices[root];
    }
    if (g->ev.empty()) {
        g->ev.assign(n, nullptr);
        for (int i = 0; i < n; ++i) {
            TAG_TRY(g, hipSetDevice(g->devices[i]));
            TAG_TRY(g, hipEventCreateWithFlags(&g->ev[i], hipEventDisableTiming));
        }
    }
    hipStream_t s0 = ctx_stream(g->ctx[root]);
    for (int j = 1; j < m; ++j) {  // member who[j]'s sum is ready on its own stream: the root's stream waits for it
        TAG_TRY(g, hipSetDevice(g->devices[who[j]]));
        TAG_TRY(g, hipEventRecord(g->ev[who[j]], ctx_stream(g->ctx[who[j]])));
    }
    TAG_TRY(g, hipSetDevice(g->devices[root]));
    for (int j = 0; j < m; ++j) {
        if (j) TAG_TRY(g, hipStreamWaitEvent(s0, g->ev[who[j]], 0));
        TAG_TRY(g, hipMemcpyPeerAsync(g->d_rows + (size_t)j * T, g->devices[root], d_tot[j], g->devices[who[j]],
                                      sizeof(double) * T, s0));
    }
    TAG_TRY(g, launch_sum_partials(g->d_rows, m, T, g->d_rows + (size_t)n * T, s0));
    d_tot[0] = g->d_rows + (size_t)n * T;
    g->reduce_kind = "peer-copy";
    return TA_OK;
}

// ---- the members of a call ---------------------------------------------------------------------------------------------
// fn(i) for every member that holds atoms (all of them unless there are more devices than atoms), in member order.  A
// member's failure ends the walk and becomes the group's, with the member's message (mfail).  who (or NULL) collects the
// members fn was called for, the failing one included: its launch may have queued work already.
template <class Fn>
int for_members(ta_group* g, std::vector<int>* who, Fn&& fn) {
    for (int i = 0; i < (int)g->ctx.size(); ++i) {
        if (g->hi[i] == g->lo[i]) continue;
        if (who) who->push_back(i);
        if (const int rc = fn(i)) return mfail(g, i, rc);
    }
    return TA_OK;
}

// everything queued so far on the members `who` has finished (their kernels and their copies into the caller's host
// arrays): every member is waited for, whatever an earlier one reports; the first failure is the one returned
int wait_members(ta_group* g, const std::vector<int>& who) {
    int rc = TA_OK;
    for (int i : who) {
        const int r = host_wait(g->ctx[i]);
        if (r && !rc) rc = mfail(g, i, r);
    }
    return rc;
}
// ... before an error is returned, so that the caller may free those arrays: the error stays the one being returned
int drained(ta_group* g, const std::vector<int>& who, int rc) {
    for (int i : who) (void)host_wait(g->ctx[i]);
    return rc;
}

// The sum over members of what each leaves on its device.  launch(i, &d) queues member i's share and returns its device
// result, laid out by the call's `out` (ta_internal.hpp); of that result every part -- part j is segment j of the layout,
// float64 or int64; h NULL, or left out at the end: skipped -- is copied into a host vector of the member's own.  A copy's
// HIP error is the group's own failure ("<what> copy: ..."); any failure drains the members first.  Then every member is
// waited for, each part's h zeroed and the members' values added in member order, int64 parts as int64 (who: the members
// called).
struct MemberPart {
    enum Kind { F64, I64 };
    void* h;
    Kind kind = F64;
};
union MemberWord {  // (the copies fill it bytewise)
    double f;
    int64_t i;
};
template <class Launch>
int sum_members(ta_group* g, std::vector<int>& who, const char* what, const OutLayout& out, std::initializer_list<MemberPart> parts,
                Launch&& launch) {
    std::vector<std::vector<MemberWord>> got(g->ctx.size());
    // fn(part, j) for every part asked for, j its segment
    auto each = [&](auto&& fn) {
        int j = 0;
        for (const MemberPart& p : parts) {
            if (p.h) fn(p, j);
            ++j;
        }
    };
    size_t total = 0;
    each([&](const MemberPart&, int j) { total += out.len(j); });
    hipError_t he = hipSuccess;
    int rc = for_members(g, &who, [&](int i) {
        double* d = nullptr;
        if (const int r = launch(i, &d)) return r;
        got[i].resize(total);  // (once: copies into it are in flight from here on)
        MemberWord* dst = got[i].data();
        each([&](const MemberPart&, int j) {
            if (he != hipSuccess) return;
            he = hipMemcpyAsync(dst, out.at(d, j), sizeof(double) * out.len(j), hipMemcpyDeviceToHost, ctx_stream(g->ctx[i]));
            dst += out.len(j);
        });
        return he == hipSuccess ? TA_OK : TA_E_HIP;
    });
    if (he != hipSuccess) rc = gfail(g, TA_E_HIP, std::string(what) + " copy: " + hipGetErrorString(he));
    if (rc) return drained(g, who, rc);
    if ((rc = wait_members(g, who))) return rc;
    each([&](const MemberPart& p, int j) { memset(p.h, 0, sizeof(double) * out.len(j)); });  // (+0.0 and 0)
    for (int i : who) {
        const MemberWord* src = got[i].data();
        each([&](const MemberPart& p, int j) {
            const size_t n = out.len(j);
            if (p.kind == MemberPart::I64)
                for (size_t k = 0; k < n; ++k) ((int64_t*)p.h)[k] += src[k].i;
            else
                for (size_t k = 0; k < n; ++k) ((double*)p.h)[k] += src[k].f;
            src += n;
        });
    }
    return TA_OK;
}

// The shape of the host-facing group entries: the reporter drains every member, then fails -- an exception after the
// members' launches lets their queued work finish first (the caller may free its arrays as soon as the call returns)
template <class Body>
int group_call(ta_group* g, Body&& body) {
    return ta::guard(
        [&](int code, const std::string& msg) {
            if (g)
                for (ta_ctx* c : g->ctx)
                    if (c) (void)host_wait(c);
            return gfail(g, code, msg);
        },
        body);
}

int check_group(ta_group* g) { return g ? TA_OK : gfail(nullptr, TA_E_INVALID, "null group"); }
int check_staged(ta_group* g) { return g->T ? TA_OK : gfail(g, TA_E_STATE, "slabs have not been staged"); }
int check_fft(ta_group* g, int fft) { return fft == 0 || fft == 1 ? TA_OK : gfail(g, TA_E_INVALID, "fft must be 0 or 1"); }
#define TAG_CHECK(expr)                                                                              \
    do {                                                                                             \
        if (int rc_ = (expr)) return rc_;                                                            \
    } while (0)

int group_compute(ta_group* g, int which, const double* h_masses, double scale, double* h_ts, double* h_bp) {
    return group_call(g, [&]() -> int {
    TAG_CHECK(check_group(g));
    if (!h_ts) return gfail(g, TA_E_INVALID, "h_timeseries is NULL");
    TAG_CHECK(check_staged(g));
    if (which == W_HELFAND && !h_masses) return gfail(g, TA_E_INVALID, "h_masses is NULL");
    std::vector<double*> d_tot;
    std::vector<int> who;
    int rc = for_members(g, &who, [&](int i) {
        double* d = nullptr;
        const int r = host_launch(g->ctx[i], which, h_masses ? h_masses + g->lo[i] : nullptr, scale,
                                  h_bp ? h_bp + g->lo[i] : nullptr, g->A, &d);
        if (!r) d_tot.push_back(d);
        return r;
    });
    if (rc || (rc = reduce_members(g, who, d_tot))) return drained(g, who, rc);  // (copies into h_bp are in flight)
    const int root = who[0];
    hipError_t he = hipSetDevice(g->devices[root]);
    if (he == hipSuccess)
        he = hipMemcpyAsync(h_ts, d_tot[0], sizeof(double) * g->T, hipMemcpyDeviceToHost, ctx_stream(g->ctx[root]));
    if (he != hipSuccess) return drained(g, who, gfail(g, TA_E_HIP, std::string("timeseries copy: ") + hipGetErrorString(he)));
    TAG_CHECK(wait_members(g, who));
    const double n_at = (double)g->A;  // mean over ALL atoms (velocityautocorr.py:214,237; viscosity.py:233)
    for (int64_t k = 0; k < g->T; ++k) h_ts[k] /= n_at;
    return TA_OK;
    });
}

// ta_group_stage_alloc (host: pinned host slabs, their pointers into h_slabs[member * n_slabs + slab]) and
// ta_group_stage_alloc_device
int group_stage_alloc(ta_group* g, int64_t n_frames, int64_t n_atoms, int dim, int dtype, int n_slabs, bool host, void** h_slabs) {
    TAG_CHECK(check_group(g));
    if (host && !h_slabs) return gfail(g, TA_E_INVALID, "h_slabs is NULL");
    if (n_frames < 1 || n_atoms < 1 || dim < 1 || dim > 3 || n_slabs < 1 || n_slabs > 4)
        return gfail(g, TA_E_INVALID, "need n_frames >= 1, n_atoms >= 1, 1 <= dim <= 3, 1 <= n_slabs <= 4");
    const int n = (int)g->ctx.size();
    g->T = 0;
    for (int i = 0; i < n; ++i) {
        shard(n_atoms, i, n, &g->lo[i], &g->hi[i]);
        for (int s = 0; host && s < n_slabs; ++s) h_slabs[i * n_slabs + s] = nullptr;
        if (g->hi[i] == g->lo[i]) {  // more devices than atoms
            ta_stage_free(g->ctx[i]);
            continue;
        }
        const int rc = host ? ta_stage_alloc(g->ctx[i], n_frames, g->hi[i] - g->lo[i], dim, dtype, n_slabs, h_slabs + (size_t)i * n_slabs)
                            : ta_stage_alloc_device(g->ctx[i], n_frames, g->hi[i] - g->lo[i], dim, n_slabs);
        if (rc) return mfail(g, i, rc);
    }
    g->T = n_frames, g->A = n_atoms, g->D = dim, g->n_slabs = n_slabs;
    return TA_OK;
}

}  // namespace

extern "C" {

int ta_group_create(const int* device_ids, int n_dev, ta_group** out) {
    return ta::guarded(gfail, nullptr, [&]() -> int {
    if (!out) return gfail(nullptr, TA_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!device_ids || n_dev < 1 || n_dev > 64) return gfail(nullptr, TA_E_INVALID, "need 1..64 device ids");
    for (int i = 0; i < n_dev; ++i)
        if (device_ids[i] < 0) return gfail(nullptr, TA_E_UNSUPPORTED, "device groups are made of GPU contexts (TA_DEVICE_CPU is a context of its own)");
    ta_group* g = new (std::nothrow) ta_group();
    if (!g) return gfail(nullptr, TA_E_NOMEM, "out of host memory");
    for (int i = 0; i < n_dev; ++i) {
        ta_ctx* c = nullptr;
        const int rc = ta_ctx_create(device_ids[i], &c);
        if (rc) {
            const std::string msg = std::string("device ") + std::to_string(device_ids[i]) + ": " + ta_last_error(nullptr);
            ta_group_destroy(g);
            return gfail(nullptr, rc, msg);
        }
        g->devices.push_back(device_ids[i]);
        g->ctx.push_back(c);
        for (int j = 0; j < i; ++j)
            if (device_ids[j] == device_ids[i]) g->distinct = false;
    }
    g->lo.assign(n_dev, 0);
    g->hi.assign(n_dev, 0);
    if (const char* e = getenv("TA_AMD_GROUP_REDUCE")) {
        if (!strcmp(e, "peer")) g->reduce_mode = RED_PEER;
        else if (!strcmp(e, "rccl")) g->reduce_mode = RED_RCCL;
        else if (strcmp(e, "auto") && *e) {
            ta_group_destroy(g);
            return gfail(nullptr, TA_E_INVALID, "TA_AMD_GROUP_REDUCE must be auto, peer or rccl");
        }
    }
    // peer access for the copy-and-add reduce (harmless when RCCL does the reduce; errors ignored:
    // hipMemcpyPeerAsync works without it, through the host)
    for (int i = 1; i < n_dev; ++i)
        if (device_ids[i] != device_ids[0]) {
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, device_ids[0], device_ids[i]) == hipSuccess && can) {
                (void)hipSetDevice(device_ids[0]);
                (void)hipDeviceEnablePeerAccess(device_ids[i], 0);
                (void)hipGetLastError();
            }
        }
    *out = g;
    return TA_OK;
    });
}

int ta_group_destroy(ta_group* g) {
    return ta::guarded(gfail, g, [&]() -> int {
    if (!g) return TA_OK;
    for (size_t i = 0; i < g->comms.size(); ++i)
        if (g->comms[i] && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(g->comms[i]);
    for (size_t i = 0; i < g->ev.size(); ++i)
        if (g->ev[i]) {
            (void)hipSetDevice(g->devices[i]);
            (void)hipEventDestroy(g->ev[i]);
        }
    if (g->d_rows) {
        (void)hipSetDevice(g->rows_device);
        (void)hipFree(g->d_rows);
    }
    for (ta_ctx* c : g->ctx) ta_ctx_destroy(c);
    delete g;
    return TA_OK;
    });
}

const char* ta_group_last_error(const ta_group* g) { return g ? g->err.c_str() : g_group_tls_error.c_str(); }

int ta_group_size(const ta_group* g) { return g ? (int)g->ctx.size() : 0; }

int ta_group_member(ta_group* g, int i, ta_ctx** ctx, int* device) {
    return ta::guarded(gfail, g, [&]() -> int {
    if (!g || i < 0 || i >= (int)g->ctx.size()) return gfail(g, TA_E_INVALID, "no such member");
    if (ctx) *ctx = g->ctx[i];
    if (device) *device = g->devices[i];
    return TA_OK;
    });
}

int ta_group_shard(const ta_group* g, int64_t n_atoms, int i, int64_t* atom_lo, int64_t* atom_hi) {
    return ta::guarded(gfail, const_cast<ta_group*>(g), [&]() -> int {
    if (!g || i < 0 || i >= (int)g->ctx.size() || n_atoms < 0 || !atom_lo || !atom_hi)
        return gfail(const_cast<ta_group*>(g), TA_E_INVALID, "bad argument");
    shard(n_atoms, i, (int)g->ctx.size(), atom_lo, atom_hi);
    return TA_OK;
    });
}

const char* ta_group_reduce_kind(const ta_group* g) { return g ? g->reduce_kind.c_str() : ""; }

const char* ta_group_reduce_note(const ta_group* g) { return g ? g->reduce_note.c_str() : ""; }

int ta_group_rccl_ranks(const ta_group* g) { return g ? g->rccl_ranks : 0; }

int ta_group_set_option(ta_group* g, const char* key, int64_t value) {
    return ta::guarded(gfail, g, [&]() -> int {
    if (!g || !key) return gfail(g, TA_E_INVALID, "null argument");
    // the group's own options; every other key goes to the members' contexts
    const bool force = !strcmp(key, "force_rccl");
    if (force || !strcmp(key, "reduce_mode")) {
        const int mode = force ? (value ? RED_RCCL : RED_AUTO) : (int)value;
        if (mode < RED_AUTO || mode > RED_RCCL) return gfail(g, TA_E_INVALID, "reduce_mode: 0 auto, 1 peer copies, 2 RCCL");
        g->reduce_mode = mode;
        return TA_OK;
    }
    for (size_t i = 0; i < g->ctx.size(); ++i) {  // (every member, with or without atoms)
        const int rc = ta_set_option(g->ctx[i], key, value);
        if (rc) return mfail(g, (int)i, rc);
    }
    return TA_OK;
    });
}

int ta_group_stage_alloc(ta_group* g, int64_t n_frames, int64_t n_atoms, int dim, int dtype, int n_slabs,
                         void** h_slabs) {
    return ta::guarded(gfail, g, [&]() -> int {
    return group_stage_alloc(g, n_frames, n_atoms, dim, dtype, n_slabs, true, h_slabs);
    });
}

int ta_group_stage_alloc_device(ta_group* g, int64_t n_frames, int64_t n_atoms, int dim, int n_slabs) {
    return ta::guarded(gfail, g, [&]() -> int {
    return group_stage_alloc(g, n_frames, n_atoms, dim, TA_F64, n_slabs, false, nullptr);
    });
}

int ta_group_stage_synth(ta_group* g, int slab, uint64_t seed, int64_t col_offset, int64_t n_cols_total) {
    return ta::guarded(gfail, g, [&]() -> int {
    TAG_CHECK(check_group(g));
    TAG_CHECK(check_staged(g));
    return for_members(g, nullptr, [&](int i) {  // member i: its own columns of the ONE synthetic tensor
        return ta_stage_synth(g->ctx[i], slab, seed, col_offset + g->lo[i] * g->D, n_cols_total, (void*)ctx_stream(g->ctx[i]));
    });
    });
}

int ta_group_stage_commit(ta_group* g, int64_t frame_lo, int64_t frame_hi) {
    return ta::guarded(gfail, g, [&]() -> int {
    TAG_CHECK(check_group(g));
    if (g->T == 0) return gfail(g, TA_E_STATE, "ta_group_stage_alloc has not been called");
    // queued on each device's own streams: the devices overlap
    return for_members(g, nullptr, [&](int i) { return ta_stage_commit(g->ctx[i], frame_lo, frame_hi); });
    });
}

int ta_group_stage_free(ta_group* g) {
    return ta::guarded(gfail, g, [&]() -> int {
    TAG_CHECK(check_group(g));
    for (ta_ctx* c : g->ctx) ta_stage_free(c);
    g->T = g->A = 0;
    return TA_OK;
    });
}

int ta_group_vacf_fft(ta_group* g, double* h_ts, double* h_bp) { return group_compute(g, W_FFT, nullptr, 1.0, h_ts, h_bp); }
int ta_group_vacf_direct(ta_group* g, double* h_ts, double* h_bp) { return group_compute(g, W_DIRECT, nullptr, 1.0, h_ts, h_bp); }
int ta_group_helfand_msd(ta_group* g, const double* h_masses, double scale, double* h_ts, double* h_bp) {
    return group_compute(g, W_HELFAND, h_masses, scale, h_ts, h_bp);
}
int ta_group_msd(ta_group* g, int fft, double* h_ts, double* h_bp) {
    TAG_CHECK(check_fft(g, fft));
    return group_compute(g, fft ? W_MSD_FFT : W_MSD_DIRECT, nullptr, 1.0, h_ts, h_bp);
}

// Conductivity: every member's moment (and self lag sum) of its atoms, added on the host in member order, then ONE
// collective MSD of the summed moment on the first member that holds atoms (the MSD of a sum is not a sum of MSDs)
int ta_group_conductivity(ta_group* g, int fft, const double* h_charges, double* h_moment, double* h_collective,
                          double* h_self_lagsum) {
    return group_call(g, [&]() -> int {
    TAG_CHECK(check_group(g));
    TAG_CHECK(check_fft(g, fft));
    if (!h_charges || !h_moment || !h_collective) return gfail(g, TA_E_INVALID, "charges, moment or collective is NULL");
    TAG_CHECK(check_staged(g));
    std::vector<int> who;
    TAG_CHECK(sum_members(g, who, "moment", cond_out(g->T, g->D), {{h_moment}, {nullptr}, {h_self_lagsum}}, [&](int i, double** d) {
        return cond_launch(g->ctx[i], fft, h_charges + g->lo[i], false, h_self_lagsum != nullptr, d);
    }));
    if (const int rc = cond_collective_host(g->ctx[who[0]], fft, h_moment, g->T, g->D, h_collective)) return mfail(g, who[0], rc);
    return TA_OK;
    });
}

// Onsager moments / Green-Kubo currents: every member's species sums of its atoms (its slice of the labels and weights, the
// call's n_species), added on the host in member order, then ONE cross term of the summed moments / currents on the first
// member that holds atoms -- the rule of ta_group_conductivity
static int group_collective(ta_group* g, int kind, const char* noun, int fft, int n_species, const int32_t* h_species,
                            const double* h_weights, double* h_sums, double* h_cross) {
    return group_call(g, [&]() -> int {
    TAG_CHECK(check_group(g));
    TAG_CHECK(check_fft(g, fft));
    TAG_CHECK(check_species_count(gfail, g, n_species));
    if (!h_species || !h_sums) return gfail(g, TA_E_INVALID, std::string("species labels or ") + noun + " are NULL");
    TAG_CHECK(check_staged(g));
    TAG_CHECK(check_labels(gfail, g, h_species, g->A, n_species));
    std::vector<int> who;
    TAG_CHECK(sum_members(g, who, noun, coll_out(n_species, g->T, g->D), {{h_sums}}, [&](int i, double** d) {
        return coll_launch(g->ctx[i], kind, fft, n_species, h_species + g->lo[i], h_weights ? h_weights + g->lo[i] : nullptr, false, d);
    }));
    if (h_cross)
        if (const int rc = coll_cross_host(g->ctx[who[0]], kind, fft, h_sums, n_species, g->T, g->D, h_cross)) return mfail(g, who[0], rc);
    return TA_OK;
    });
}
int ta_group_onsager(ta_group* g, int fft, int n_species, const int32_t* h_species, const double* h_weights,
                     double* h_moments, double* h_cross) {
    return group_collective(g, COLL_MOMENTS, "moments", fft, n_species, h_species, h_weights, h_moments, h_cross);
}
int ta_group_current(ta_group* g, int fft, int n_species, const int32_t* h_species, const double* h_weights,
                     double* h_currents, double* h_cross) {
    return group_collective(g, COLL_CURRENTS, "currents", fft, n_species, h_species, h_weights, h_currents, h_cross);
}

// Species self terms: every member's (n_species, n_frames) lag sums and counts of its atoms (its slice of the labels and
// weights), added on the host in member order (lag sums are linear in atoms: nothing follows the sum)
int ta_group_species_self(ta_group* g, int quantity, int fft, int n_species, const int32_t* h_species, const double* h_weights,
                          double* h_self, int64_t* h_counts) {
    return group_call(g, [&]() -> int {
    TAG_CHECK(check_group(g));
    if (quantity != TA_SELF_MSD && quantity != TA_SELF_VACF)
        return gfail(g, TA_E_INVALID, "quantity must be TA_SELF_MSD (0) or TA_SELF_VACF (1)");
    TAG_CHECK(check_fft(g, fft));
    TAG_CHECK(check_species_count(gfail, g, n_species));
    if (!h_species || !h_self) return gfail(g, TA_E_INVALID, "species labels or self output are NULL");
    TAG_CHECK(check_staged(g));
    TAG_CHECK(check_labels(gfail, g, h_species, g->A, n_species));
    std::vector<std::vector<int64_t>> cnt(g->ctx.size());
    std::vector<int> who;
    TAG_CHECK(sum_members(g, who, "self terms", self_out(n_species, g->T), {{h_self}}, [&](int i, double** d) {
        cnt[i].assign(n_species, 0);
        return self_launch(g->ctx[i], quantity, fft, n_species, h_species + g->lo[i], h_weights ? h_weights + g->lo[i] : nullptr,
                           cnt[i].data(), d);
    }));
    if (h_counts) {
        std::fill(h_counts, h_counts + n_species, (int64_t)0);
        for (int i : who)
            for (int s = 0; s < n_species; ++s) h_counts[s] += cnt[i][s];
    }
    return TA_OK;
    });
}

// Intermediate scattering: every member's self parts and densities of its atoms for the same wavevectors, added on the
// host in member order, then ONE collective part of the summed density on the first member that holds atoms -- the rule of
// ta_group_conductivity (a density the caller does not ask for is summed into a vector of the call's own)
int ta_group_scatter(ta_group* g, int fft, int n_k, const double* h_kvecs, double* h_self, double* h_density, double* h_coll) {
    return group_call(g, [&]() -> int {
    TAG_CHECK(check_group(g));
    TAG_CHECK(check_kvecs(gfail, g, fft, n_k, h_kvecs, g->T ? g->D : 0, h_self || h_density || h_coll));
    TAG_CHECK(check_staged(g));
    const OutLayout out = scatter_out(n_k, g->T);
    std::vector<double> own;
    if (h_coll && !h_density) own.resize(out.len(1));
    double* dens = h_density ? h_density : h_coll ? own.data() : nullptr;
    std::vector<int> who;
    TAG_CHECK(sum_members(g, who, "scattering sums", out, {{h_self}, {dens}}, [&](int i, double** d) {
        return scatter_launch(g->ctx[i], fft, n_k, h_kvecs, h_self != nullptr, dens != nullptr, false, d);
    }));
    if (h_coll)
        if (const int rc = scatter_collective_host(g->ctx[who[0]], fft, dens, n_k, g->T, h_coll)) return mfail(g, who[0], rc);
    return TA_OK;
    });
}

// Current correlation functions: every member's current of its atoms (its slice of the weights) for the same wavevectors,
// added on the host in member order, then ONE pair of correlations of the summed current on the first member that holds
// atoms -- the rule of ta_group_conductivity (a current the caller does not ask for is summed into a vector of the call's own)
int ta_group_kcurrent(ta_group* g, int fft, int n_k, const double* h_kvecs, const double* h_weights, double* h_current,
                      double* h_long, double* h_trans) {
    return group_call(g, [&]() -> int {
    TAG_CHECK(check_group(g));
    TAG_CHECK(check_kcurrent(gfail, g, fft, n_k, h_kvecs, g->T ? g->D : 0, h_current || h_long || h_trans));
    TAG_CHECK(check_staged(g));
    const OutLayout out = kcurrent_out(n_k, g->T, g->D);
    std::vector<double> own;
    if (!h_current) own.resize(out.len(0));
    double* cur = h_current ? h_current : own.data();
    std::vector<int> who;
    TAG_CHECK(sum_members(g, who, "currents", out, {{cur}}, [&](int i, double** d) {
        return kcurrent_launch(g->ctx[i], fft, n_k, h_kvecs, h_weights ? h_weights + g->lo[i] : nullptr, false, d);
    }));
    if (h_long || h_trans)
        if (const int rc = kcurrent_correlate_host(g->ctx[who[0]], fft, cur, n_k, h_kvecs, g->T, g->D, h_long, h_trans))
            return mfail(g, who[0], rc);
    return TA_OK;
    });
}

// Partial scattering functions: every member's species-resolved density of its atoms (its slice of the labels and weights, the
// call's n_species) for the same wavevectors, added on the host in member order, then ONE cross term of the summed density on
// the first member that holds atoms -- the rule of ta_group_conductivity
int ta_group_partial_density(ta_group* g, int fft, int n_k, const double* h_kvecs, int n_species, const int32_t* h_species,
                             const double* h_weights, double* h_density, double* h_cross) {
    return group_call(g, [&]() -> int {
    TAG_CHECK(check_group(g));
    TAG_CHECK(check_partial(gfail, g, fft, n_k, h_kvecs, g->T ? g->D : 0, n_species, h_species, h_density));
    TAG_CHECK(check_staged(g));
    TAG_CHECK(check_labels(gfail, g, h_species, g->A, n_species));
    std::vector<int> who;
    TAG_CHECK(sum_members(g, who, "partial densities", partial_out(n_k, n_species, g->T), {{h_density}}, [&](int i, double** d) {
        return partial_launch(g->ctx[i], fft, n_k, h_kvecs, n_species, h_species + g->lo[i],
                              h_weights ? h_weights + g->lo[i] : nullptr, false, d);
    }));
    if (h_cross)
        if (const int rc = partial_cross_host(g->ctx[who[0]], fft, h_density, n_k, n_species, g->T, h_cross)) return mfail(g, who[0], rc);
    return TA_OK;
    });
}

// Self van Hove function: every member's counts and moments of its atoms for the same lags and bins, the counts added as
// int64 and the moments in member order (both add up over atoms: nothing follows the sums)
int ta_group_vanhove(ta_group* g, int n_lags, const int64_t* h_lags, int n_bins, double dr, int64_t* h_counts, double* h_moments) {
    return group_call(g, [&]() -> int {
    TAG_CHECK(check_group(g));
    TAG_CHECK(check_vanhove(gfail, g, n_lags, h_lags, n_bins, dr, g->T, h_counts || h_moments));
    TAG_CHECK(check_staged(g));
    std::vector<int> who;
    TAG_CHECK(sum_members(g, who, "van Hove sums", vanhove_out(n_lags, n_bins), {{h_counts, MemberPart::I64}, {h_moments}}, [&](int i, double** d) {
        return vanhove_launch(g->ctx[i], n_lags, h_lags, n_bins, dr, h_counts != nullptr, h_moments != nullptr, d);
    }));
    return TA_OK;
    });
}

// Self-overlap per origin: every member's Q of its atoms for the same lags and cutoffs, added as int64 (Q adds up over
// atoms; a variance over origins is the caller's, after this sum)
int ta_group_overlap(ta_group* g, int n_lags, const int64_t* h_lags, int n_cutoffs, const double* h_cutoffs, int64_t* h_q) {
    return group_call(g, [&]() -> int {
    TAG_CHECK(check_group(g));
    TAG_CHECK(check_overlap(gfail, g, n_lags, h_lags, n_cutoffs, h_cutoffs, g->T, h_q != nullptr));
    TAG_CHECK(check_staged(g));
    std::vector<int> who;
    TAG_CHECK(sum_members(g, who, "overlap counts", overlap_out(n_cutoffs, n_lags, g->T), {{h_q, MemberPart::I64}}, [&](int i, double** d) {
        return overlap_launch(g->ctx[i], n_lags, h_lags, n_cutoffs, h_cutoffs, d);
    }));
    return TA_OK;
    });
}

// Overlap field's density per origin: every member's W of its atoms for the same wavevectors, lags and cutoffs, added on the
// host in member order as float64 (W adds up over atoms; |W|^2 and a variance over origins are the caller's, after this sum)
int ta_group_overlap_density(ta_group* g, int n_k, const double* h_kvecs, int n_lags, const int64_t* h_lags, int n_cutoffs,
                             const double* h_cutoffs, double* h_w) {
    return group_call(g, [&]() -> int {
    TAG_CHECK(check_group(g));
    TAG_CHECK(check_overlap_density(gfail, g, n_k, h_kvecs, g->T ? g->D : 0, n_lags, h_lags, n_cutoffs, h_cutoffs, g->T, h_w != nullptr));
    TAG_CHECK(check_staged(g));
    std::vector<int> who;
    TAG_CHECK(sum_members(g, who, "overlap densities", overlap_density_out(n_k, n_cutoffs, n_lags, g->T), {{h_w}}, [&](int i, double** d) {
        return overlap_density_launch(g->ctx[i], n_k, h_kvecs, n_lags, h_lags, n_cutoffs, h_cutoffs, d);
    }));
    return TA_OK;
    });
}

// Unwrap: every member's block of slab `slab` with the same box table, queued on all devices, then waited for
int ta_group_unwrap(ta_group* g, int slab, const double* h_dimensions, const int* axes) {
    return group_call(g, [&]() -> int {
    TAG_CHECK(check_group(g));
    if (!h_dimensions || !axes) return gfail(g, TA_E_INVALID, "dimensions or axes are NULL");
    TAG_CHECK(check_staged(g));
    if (slab < 0 || slab >= g->n_slabs) return gfail(g, TA_E_INVALID, "no such slab");
    BoxTable box;
    const std::string why = box_table(h_dimensions, g->T, g->D, axes, 256, &box);
    if (!why.empty()) return gfail(g, TA_E_INVALID, "unwrap: " + why);
    std::vector<int> who;
    if (const int rc = for_members(g, &who, [&](int i) { return unwrap_launch(g->ctx[i], slab, box, axes); }))
        return drained(g, who, rc);
    return wait_members(g, who);
    });
}

}  // extern "C"
