// api.hip — C-ABI entry points of libta_hip.so (declared in include/ta_hip.h).
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ta_hip.h"
#include "bond_math.hpp"
#include "cpu_backend.hpp"
#include "direct_kernels.hpp"
#include "kcurrent_math.hpp"
#include "chain_math.hpp"
#include "orient_math.hpp"
#include "pair_math.hpp"
#include "phase_math.hpp"
#include "shell_msd_math.hpp"
#include "ta_internal.hpp"
#include "unwrap_box.hpp"
#include "vanhove_distinct_math.hpp"
#include "vanhove_math.hpp"

using namespace ta;

namespace {

thread_local std::string g_tls_error;

// A device workspace of a context.  Each one is a member of ta_ctx declared once, with whether ta_trim releases it; the
// constructor enters it in the context's list, which is what ta_trim and ta_ctx_destroy walk.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    const bool trimmed;
    DevBuf(std::vector<DevBuf*>& list, bool trimmed_by_ta_trim) : trimmed(trimmed_by_ta_trim) { list.push_back(this); }
    DevBuf(const DevBuf&) = delete;
    void release() {
        if (p) hipFree(p);
        p = nullptr, bytes = 0;
    }
};
constexpr bool kTrimmed = true, kKept = false;

// A table a call forms on the host and queues for upload before it is opened: the device copy (a kept workspace like any
// other), the host storage the asynchronous copy reads, and the event that says the last upload has left it.  begin():
// the device buffer ensured, that upload waited for, *h = `bytes` of host storage (8-byte aligned) to fill; send(): the
// copy and the event queued on `st`.  Members of ta_ctx, entered in its list (ta_ctx_destroy walks it for the events).
struct HostTable {
    DevBuf dev;
    std::vector<double> host;
    size_t n_bytes = 0;
    hipEvent_t ev = nullptr;
    HostTable(std::vector<DevBuf*>& workspaces, std::vector<HostTable*>& tables) : dev(workspaces, kKept) { tables.push_back(this); }
    int begin(ta_ctx* ctx, size_t bytes, void** h);
    int send(ta_ctx* ctx, hipStream_t st);
};

// ta_stage_commit hands its frame range to a worker thread that makes the HIP calls (copies in pieces, the transposition
// launches): the caller's frame loop never waits on the runtime — which it did, for as long as another thread's
// hipHostMalloc of the by-particle result held the runtime's lock (0.17 s of a 0.6 s loop at 10000 x 50000 x 3).
// The rules:
//   - the worker is the only thread that touches the slabs and the context's streams while a job is queued or running;
//     every other entry that touches them calls flush() first (order_after_staging does);
//   - push() never fails and never waits; a job's error is kept (the first one only) and returned ONCE, by the next
//     flush(), with the prefix "queued ta_stage_commit: ";
//   - the thread starts with the first push() and ends in stop(), which drains the queue first; an empty job
//     (frame_lo == frame_hi) copies nothing and only page-locks ahead (ta_stage_alloc queues one).
class CommitQueue {
public:
    explicit CommitQueue(ta_ctx* owner) : ctx_(owner) {}
    void push(int64_t frame_lo, int64_t frame_hi);
    int flush();  // every queued job has made its HIP calls (their work is queued on the context's streams)
    void stop();

private:
    void run();
    ta_ctx* ctx_;
    std::thread thread_;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<std::pair<int64_t, int64_t>> jobs_;
    bool stop_ = false, busy_ = false;
    int rc_ = TA_OK;
    std::string err_;
};

}  // namespace

// Every option of ta_set_option: X(key, default, hook) declares the field ctx->opt_<key> and its row of the table
// ta_set_option looks the key up in.  A hook (NULL: a plain store) runs before the store and may reject the value.
#define TA_OPTIONS(X)                                                                                                      \
    X(fft_nwg, 0, nullptr)         /* workgroups of the FFT kernels (0: by the device) */                                  \
    X(direct_nwg, 0, nullptr)      /* workgroups of k_direct (0: by the device) */                                         \
    X(direct_f32, 0, nullptr)      /* the float32 option of the O(T^2) correlators */                                      \
    X(direct_groups, 0, nullptr)   /* cap on k_direct's column groups per workgroup */                                     \
    X(direct_chunk, 0, nullptr)    /* k_direct's lags per chunk: 8 or 10 (0: by n_frames) */                               \
    X(direct_mfma, 1, opt_check_direct_mfma) /* which kernel evaluates a direct request: see direct_form */                \
    X(helfand_fft, 0, nullptr)     /* Helfand as S1 - 2 S2 where an FFT plan exists */                                     \
    X(bp_block, 0, nullptr)        /* atoms per block of a host-facing by-particle call (0: 16384) */                      \
    X(bp_spec_atoms, 0, nullptr)   /* atoms per block of spectra in the two-kernel by-particle path (0: 2.5 GiB's worth) */ \
    X(bp_prefetch, 2, nullptr)     /* k_winverse's prefetch depth */                                                       \
    /* "short_max": trajectories of up to this many frames (<= 64) take the register-resident kernels of short_kernels.hpp \
       wherever float64 slabs are asked for a by-particle array or an O(T^2) form (0: never); "short_lags_max": the FFT    \
       path's lag sums alone as well, up to this many frames (per 12 GB: 2.1 against 3.9 ms at 32 frames, 3.8 against 4.6  \
       at 48, 4.1 against 3.8 at 64: profiles/r06_short.txt) */                                                           \
    X(short_max, 64, nullptr)                                                                                              \
    X(short_lags_max, 48, nullptr)                                                                                         \
    X(mid_max, 512, nullptr)       /* k_mid (mid_kernels.hpp) under "direct_mfma" 1: see direct_form */                    \
    X(mid_all, 0, nullptr)                                                                                                 \
    X(mid_ncl, 0, nullptr)                                                                                                 \
    X(direct_subwave, 1, nullptr)  /* k_direct's column groups may be 16 or 32 lanes (under ~640 frames) */                \
    X(stage_device_f32, 0, nullptr) /* device slabs hold float32 when nothing wider is coming in */                        \
    X(timeline, 0, nullptr)        /* record the kernel timeline of every compute call (ta_kernel_timeline) */             \
    X(scatter_chunk, 0, opt_check_scatter_chunk) /* wavevectors per pass of ta_scatter* (0: as many as fit kScatterBudget) */ \
    X(kcurrent_chunk, 0, opt_check_kcurrent_chunk) /* wavevectors per launch of k_kcurrent (0: the tile's own count) */     \
    X(partial_chunk, 0, opt_check_partial_chunk) /* wavevectors per launch of k_species_density (0: the tile's own count) */ \
    X(partial_cross_chunk, 0, opt_check_partial_cross_chunk) /* wavevectors per batch of partial_cross (0: as many as fit kPartialCrossBudget) */ \
    X(chain_modes_chunk, 0, opt_check_chain_modes_chunk) /* functionals per batch of ta_chain_modes* (0: as many as fit kChainBudget) */ \
    X(vanhove_chunk, 0, opt_check_vanhove_chunk) /* lags per pass of ta_vanhove* (0: as many as fit a workgroup's LDS) */ \
    X(overlap_chunk, 0, opt_check_overlap_chunk) /* lags per launch of ta_overlap* (0: as many as the kernel's tile holds) */ \
    X(overlap_density_chunk, 0, opt_check_overlap_density_chunk) /* lags per launch of ta_overlap_density* (0: as many as the kernel's tile holds) */ \
    X(vanhove_distinct_chunk, 0, opt_check_vanhove_distinct_chunk) /* lags per pass of ta_vanhove_distinct* (0: as many as fit kVhdBudget) */ \
    X(pair_chunk, 0, opt_check_pair_chunk) /* candidate pairs per block of ta_pair_lifetime* (0: as many as fit kPairBudget) */ \
    X(pair_find_chunk, 0, opt_check_pair_find_chunk) /* searched frames per pass of ta_pair_find (0: as many as fit kVhdBudget) */ \
    X(shell_chunk, 0, opt_check_shell_chunk) /* 64-frame words per pass of ta_shell_residence* (0: as many as fit kVhdBudget) */ \
    X(shell_msd_chunk, 0, opt_check_shell_msd_chunk) /* origin frames per staged chunk of k_shell_msd (0: 512) */ \
    X(async_commit, 1, opt_flush_commits) /* ta_stage_commit goes through the commit queue; flushed before it changes */   \
    X(lock_ahead, 1, nullptr)      /* the commit worker page-locks the chunks behind the one it committed */               \
    X(cpu_threads, 0, opt_set_cpu_threads) /* CPU backend: OpenMP team size (0: the runtime's default) */                  \
    X(fail_alloc_after, 0, nullptr) /* test hooks of ensure(): the n-th call from now throws std::bad_alloc ... */         \
    X(fail_throw_after, 0, nullptr) /* ... or std::runtime_error */

struct ta_ctx {
    // a CPU context (ta_ctx_create(TA_DEVICE_CPU, ...): the opt-in backend of cpu_backend.cpp) owns host slabs only;
    // no HIP call is ever made on its behalf and every device-facing entry point rejects it (TA_NO_CPU).  Its entry
    // points branch to the cpu_* functions below (the seam) and nowhere else.
    bool is_cpu = false;
    int cpu_threads = 1;  // OpenMP team size of the CPU backend
    int device = 0;
    int n_cu = 256;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // device->host copies of by-particle blocks (host_launch)
    std::string err;
    std::map<int, cd*> wf_tables;  // wfft.hip twiddle tables, keyed by 64 * R0 + R
    // ---- device workspaces: this is the one list of them (kTrimmed: ta_trim releases it, kKept: it does not)
    std::vector<DevBuf*> workspaces;
    std::vector<HostTable*> tables;  // the host tables among them
    DevBuf partial{workspaces, kTrimmed}, spec{workspaces, kTrimmed}, ts_partial{workspaces, kTrimmed};
    DevBuf out_lagsum{workspaces, kKept}, out_bp{workspaces, kTrimmed}, masses{workspaces, kKept};
    DevBuf stage_buf{workspaces, kTrimmed}, helf_p{workspaces, kTrimmed}, helf_small{workspaces, kTrimmed};
    DevBuf pm_in[2] = {{workspaces, kTrimmed}, {workspaces, kTrimmed}};  // pair-major copies of frame-major *_dev inputs
    DevBuf bp_scratch{workspaces, kTrimmed};    // atom-major by-particle results before the transposition
    DevBuf bp_spec{workspaces, kTrimmed};       // per-atom power spectra of one block of atoms (two-kernel by-particle path)
    DevBuf unit_counter{workspaces, kKept};     // k_band_bp_vacf's work counter
    // conductivity (cond_pm): the moment's partial sums, the weighted slab of the self term (the input's size), the
    // charges and outputs of host-facing calls, the pair-major copy of the (n_frames, dim) moment
    DevBuf cond_part{workspaces, kTrimmed}, cond_w{workspaces, kTrimmed}, cond_q{workspaces, kKept};
    DevBuf cond_out{workspaces, kKept}, cond_mpm{workspaces, kTrimmed};
    // Onsager moments and Green-Kubo currents (coll_pm, coll_cross; ons_*: the first of the two to use them): the species
    // sums' partial sums, the labels and weights and the outputs of host-facing calls, the pair-major slab of the S^2
    // pseudo-particles, their by-particle lag sums (+ lag sums and the non-zero flags)
    DevBuf ons_part{workspaces, kTrimmed}, ons_lab{workspaces, kKept}, ons_w{workspaces, kKept};
    DevBuf ons_out{workspaces, kKept}, ons_pm{workspaces, kTrimmed}, ons_bp{workspaces, kTrimmed};
    DevBuf unwrap_box{workspaces, kTrimmed};    // ta_unwrap: the box table (unwrap_box.hpp) of the last call
    // species self terms (species_self_pm): the weighted slab with each species' atoms contiguous (the input's element
    // count x 8 bytes + at most one column per species), the atoms in sorted order (int32) and the output of host-facing calls
    DevBuf self_w{workspaces, kTrimmed}, self_out{workspaces, kKept};
    HostTable self_order{workspaces, tables};
    // intermediate scattering (scatter_pm): the phase slab Z of one chunk of wavevectors (trimmed), the zero labels of the
    // density sum, the wavevectors in turns, the pair-major copy of the densities with their by-particle lag sums (and the
    // density itself when the caller does not ask for it), the outputs of host-facing calls
    DevBuf scatter_z{workspaces, kTrimmed}, scatter_lab{workspaces, kKept};
    DevBuf scatter_work{workspaces, kTrimmed}, scatter_out{workspaces, kKept};
    HostTable scatter_q{workspaces, tables};
    // orientational correlation functions (orient_pm): the block Z of the orientation columns (3 n_vectors pitch 16 bytes,
    // shared by the two ranks; trimmed), the pair-major copy of the total (and the total itself when the caller does not
    // ask for it), the table (box rows, weights, index rows, zero labels), the outputs of host-facing calls
    DevBuf orient_z{workspaces, kTrimmed}, orient_work{workspaces, kTrimmed}, orient_out{workspaces, kKept};
    HostTable orient_tab{workspaces, tables};
    // chain normal modes (chain_pm): the blocks of one batch of functionals (3 n_chains pitch 8 bytes each; trimmed), the
    // table (box rows, coefficients, members), the output of host-facing calls
    DevBuf chain_z{workspaces, kTrimmed}, chain_out{workspaces, kKept};
    HostTable chain_tab{workspaces, tables};
    // current correlation functions (kcurrent_pm): the partial sums of one chunk of wavevectors (trimmed; its size does not
    // depend on their number), the pair-major slab of the pseudo-atoms jL, jT with their by-particle lag sums (and the current
    // itself when the caller does not ask for it), the wavevectors in turns with the unit vectors (and a host call's weights)
    // behind them, the outputs of host-facing calls
    DevBuf kcur_part{workspaces, kTrimmed}, kcur_work{workspaces, kTrimmed}, kcur_out{workspaces, kKept};
    HostTable kcur_tab{workspaces, tables};
    // partial scattering functions (partial_pm): the partial sums of one chunk of wavevectors (trimmed; its size does not
    // depend on their number or on the species), the wavevectors in turns (and a host call's weights behind them), a host
    // call's labels and outputs; the cross term's pseudo-particles and lag sums use the Onsager workspaces
    DevBuf psd_part{workspaces, kTrimmed}, psd_lab{workspaces, kKept}, psd_out{workspaces, kKept};
    HostTable psd_tab{workspaces, tables};
    // self van Hove function (vanhove_pm): the lags (int64) with the squared edges behind them, the uint64 histogram and
    // the workgroups' moment partials (the scratch: trimmed), the outputs of host-facing calls
    HostTable vh_tab{workspaces, tables};
    DevBuf vh_hist{workspaces, kTrimmed}, vh_part{workspaces, kTrimmed}, vh_out{workspaces, kKept};
    // self-overlap per origin (overlap_pm): the lags (int64) with the squared cutoffs behind them; Q goes straight into the
    // caller's array, so the only buffer is the output of host-facing calls (up to 1 GiB: trimmed)
    HostTable ov_tab{workspaces, tables};
    DevBuf ov_out{workspaces, kTrimmed};
    // overlap field's density per origin (overlap_density_pm): the lags (int64) with the squared cutoffs and the wavevectors
    // in turns behind them, the partial sums of one launch (trimmed; its size does not depend on the call's lists), the
    // output of host-facing calls (up to 1 GiB: trimmed)
    HostTable od_tab{workspaces, tables};
    DevBuf od_part{workspaces, kTrimmed}, od_out{workspaces, kTrimmed};
    // distinct van Hove function (vhd_pm): the table (lags, squared edges, box entries, padded index lists), the gathered
    // frame-major scratch GA | GB and the uint64 histogram (trimmed), the output of host-facing calls
    HostTable vhd_tab{workspaces, tables};
    DevBuf vhd_scr{workspaces, kTrimmed}, vhd_hist{workspaces, kTrimmed}, vhd_out{workspaces, kKept};
    // pair lifetimes (pair_find_pm, pair_life_pm): the search's table (a zero lag, box entries, padded index lists), its
    // bitmap with the block counts and offsets behind it (the gathered scratch is vhd_scr), the found list (n_pairs, 2)
    // int32 with its length and the staged atom count it was found for (pair_n < 0: none); the lifetime call's table (box
    // entries, pairs, zero labels), the indicator block Z of one block of pairs, the blocks' rows of lag sums and bonded
    // counts with the uint64 run histogram behind them, the outputs of host-facing calls.  A CPU context keeps its found
    // list in pair_host.
    HostTable pair_ftab{workspaces, tables}, pair_tab{workspaces, tables};
    DevBuf pair_bits{workspaces, kTrimmed}, pair_list{workspaces, kTrimmed}, pair_z{workspaces, kTrimmed};
    DevBuf pair_rows{workspaces, kTrimmed}, pair_out{workspaces, kKept};
    int64_t pair_n = -1, pair_A = 0;
    // shell residence times (shell_pm): the table (a zero lag, box entries, padded index lists, zero labels); the scratch is
    // vhd_scr, the level block and everything behind it the pair lifetimes' (pair_z, pair_rows, pair_out)
    HostTable shell_tab{workspaces, tables};
    // ta_shell_msd*: the packed words of g of one block of observed items, and k_shell_msd's partial rows
    DevBuf shell_words{workspaces, kTrimmed}, shell_part{workspaces, kTrimmed};
    std::vector<int32_t> pair_host;
    // ta_compound: the plan (offsets, members, member weights, their sums per compound) and the (n_frames, dim) weighted
    // mean F of the barycentric term; the per-atom frame weights and F's partial sums use the Onsager workspaces
    DevBuf comp_plan{workspaces, kTrimmed}, comp_f{workspaces, kTrimmed};
    // staging: two landing buffers, so that a piece crosses PCIe while the one before it is transposed
    DevBuf bounce{workspaces, kTrimmed}, bounce2{workspaces, kTrimmed};
    DevBuf clock_stamps{workspaces, kTrimmed};  // ta_clock_probe: the stamps of its last launch
    // ---- staging: pinned host slabs keep the reference's (n_frames, n_atoms, dim) layout, the device slabs are
    // pair-major (layout.hip) with st_pitch rows per column pair.  This is the one record of the staged shape, for GPU
    // and CPU contexts alike (a CPU context has host slabs only).
    int64_t st_T = 0, st_A = 0, st_pitch = 0;
    int st_D = 0, st_dtype = TA_F64, st_nslabs = 0;
    bool st_dev_f32 = false;  // device slabs hold float32 elements ("stage_device_f32")
    bool st_compound = false;  // slab 0 is ta_compound's: nothing can be staged into it (until the next ta_stage_alloc*)
    std::vector<void*> h_slabs;
    std::vector<HostBlock> h_blocks;  // the mapping behind h_slabs[i] (base == NULL: a hipHostMalloc block, the fallback)
    std::vector<double*> d_slabs;
    hipStream_t relayout_stream = nullptr;  // the transpositions of ta_stage_commit
    hipEvent_t ev_piece[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
    CommitQueue commits{this};
    // ---- timing: a ring of event quadruples, one per compute call (start, main kernel start, main kernel end, end), so
    // a caller can time K calls back to back and read all K durations afterwards (ta_timing_history) instead of
    // synchronising inside its loop
    static constexpr int kRing = 64;
    hipEvent_t ring[kRing][4] = {};
    hipEvent_t* ev = ring[0];
    hipEvent_t ev_stage = nullptr;  // orders a caller's stream behind the staging stream
    long n_calls = 0;  // compute calls completed (their events recorded)
    bool timing_valid = false;
    // kernel timeline of the last compute call ("timeline" option): an event before every launch, a last one at the
    // end; segment i = [mark i, mark i + 1) belongs to name i
    struct Mark {
        const char* name;
        hipEvent_t ev;
    };
    std::vector<Mark> marks;
    std::vector<hipEvent_t> mark_pool;
    size_t marks_used = 0;
    // ---- options
#define X(key, dflt, hook) int64_t opt_##key = dflt;
    TA_OPTIONS(X)
#undef X
};

namespace {

// (the commit worker thread reports errors too: the context's message is written and read under a lock)
std::mutex g_err_m;
int fail(ta_ctx* ctx, int code, const std::string& msg) noexcept {
    try {  // (a failing copy of the message must not turn an error return into an exception)
        if (ctx) {
            std::lock_guard<std::mutex> lk(g_err_m);
            ctx->err = msg;
        }
        g_tls_error = msg;
    } catch (...) {
    }
    return code;
}

#define TA_CHECK(expr)                                                                                                    \
    do {                                                                                                                  \
        if (int rc_ = (expr)) return rc_;                                                                                 \
    } while (0)

#define TA_HIP_TRY(ctx, expr)                                                                  \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return fail(ctx, (_e == hipErrorOutOfMemory) ? TA_E_NOMEM : TA_E_HIP,              \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                    \
    } while (0)

// ---- the argument and state checks of the entry points, each message written once -------------------------------------
int need_ctx(ta_ctx* ctx) { return ctx ? TA_OK : fail(nullptr, TA_E_INVALID, "null context"); }
int no_cpu(ta_ctx* ctx) {
    if (ctx && ctx->is_cpu)
        return fail(ctx, TA_E_UNSUPPORTED, "not available on the CPU backend (device pointers, streams and kernel timings belong to GPU contexts)");
    return TA_OK;
}
#define TA_NO_CPU(ctx) TA_CHECK(no_cpu(ctx))
int check_staged(ta_ctx* ctx, int n_slabs = 1) {
    return ctx->st_nslabs >= n_slabs ? TA_OK : fail(ctx, TA_E_STATE, "slabs have not been staged");
}
// the kernels index a slab's columns in 32 bits: "<prefix>n_atoms * <what> must be below 2^31" (D: what `what` names)
int check_cols(ta_ctx* ctx, const std::string& prefix, int64_t A, int D, const char* what = "dim") {
    return A * D < (int64_t)1 << 31 ? TA_OK : fail(ctx, TA_E_INVALID, prefix + "n_atoms * " + what + " must be below 2^31");
}
int check_slab(ta_ctx* ctx, int slab) {
    return slab >= 0 && slab < ctx->st_nslabs ? TA_OK : fail(ctx, TA_E_INVALID, "no such slab");
}
int check_not_compound(ta_ctx* ctx) {
    return !ctx->st_compound ? TA_OK
                             : fail(ctx, TA_E_STATE, "the staged slab holds ta_compound's compounds: ta_stage_alloc comes before frames can be staged again");
}
int check_frames(ta_ctx* ctx, int64_t frame_lo, int64_t frame_hi) {
    if (frame_lo < 0 || frame_hi > ctx->st_T || frame_lo > frame_hi) return fail(ctx, TA_E_INVALID, "frame range out of bounds");
    return TA_OK;
}
int check_ld_row(ta_ctx* ctx, int64_t ld_row, int64_t n_cols) {
    return ld_row >= n_cols ? TA_OK : fail(ctx, TA_E_INVALID, "ld_row smaller than n_atoms*dim");
}
int check_fft(ta_ctx* ctx, int fft) { return fft == 0 || fft == 1 ? TA_OK : fail(ctx, TA_E_INVALID, "fft must be 0 or 1"); }
int check_dtype(ta_ctx* ctx, int dtype) {
    return dtype == TA_F32 || dtype == TA_F64 ? TA_OK : fail(ctx, TA_E_INVALID, "bad dtype");
}
// the shape of host sums handed to a correlator (dim NULL: sums without that axis)
int check_sums_shape(ta_ctx* ctx, int64_t n_frames, const int* dim = nullptr) {
    if (n_frames < 1 || n_frames > (int64_t)1 << 30 || (dim && (*dim < 1 || *dim > 3)))
        return fail(ctx, TA_E_INVALID, std::string("need 1 <= n_frames <= 2^30") + (dim ? ", 1 <= dim <= 3" : ""));
    return TA_OK;
}
int check_shape(ta_ctx* ctx, int64_t T, int64_t A, int D, int64_t ld_row) {
    TA_CHECK(need_ctx(ctx));
    if (T < 1 || A < 1 || D < 1 || D > 3)
        return fail(ctx, TA_E_INVALID, "need n_frames >= 1, n_atoms >= 1, 1 <= dim <= 3");
    TA_CHECK(check_ld_row(ctx, ld_row, A * D));
    if (T > (int64_t)1 << 30) return fail(ctx, TA_E_INVALID, "n_frames too large");
    return TA_OK;
}

int ensure(ta_ctx* ctx, DevBuf& b, size_t bytes) {
    // test hooks ("fail_alloc_after" / "fail_throw_after" n): the n-th call from now throws what a failing host allocation /
    // any other library exception would, so that the tests can see the C boundary turn it into a status
    if (ctx->opt_fail_alloc_after > 0 && --ctx->opt_fail_alloc_after == 0) throw std::bad_alloc();
    if (ctx->opt_fail_throw_after > 0 && --ctx->opt_fail_throw_after == 0) throw std::runtime_error("fail_throw_after");
    if (b.bytes >= bytes && b.p) return TA_OK;
    b.release();
    if (bytes == 0) bytes = 16;
    TA_HIP_TRY(ctx, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return TA_OK;
}

// A host-facing call's output buffer `b`, sized by the call's layout (before the call is opened) ...
template <class E>  // (double, or int64_t where the call's only segment holds counts)
int out_buffer(ta_ctx* ctx, DevBuf& b, const OutLayout& o, E** out) {
    static_assert(sizeof(E) == 8);
    TA_CHECK(ensure(ctx, b, sizeof(E) * o.total()));
    *out = (E*)b.p;
    return TA_OK;
}
// ... and the call's tail: the segments at d_out copied into the caller's arrays `h`, in segment order (NULL, or left out at
// the end: not asked for), then everything the call queued waited for
int out_finish(ta_ctx* ctx, const OutLayout& o, const double* d_out, std::initializer_list<void*> h) {
    HostCopy c[OutLayout::kMax] = {};
    int i = 0;
    for (void* p : h) c[i] = {(double*)p, d_out + o.off[i], o.len(i)}, ++i;
    return host_finish(ctx, {c[0], c[1], c[2], c[3]});
}

// host sums queued for upload into segment i of a call's layout (the correlators of host sums)
int upload_segment(ta_ctx* ctx, const OutLayout& o, double* out, int i, const double* h, hipStream_t st) {
    TA_HIP_TRY(ctx, hipMemcpyAsync(o.at(out, i), h, sizeof(double) * o.len(i), hipMemcpyHostToDevice, st));
    return TA_OK;
}

int HostTable::begin(ta_ctx* ctx, size_t bytes, void** h) {
    TA_CHECK(ensure(ctx, dev, bytes));
    if (!ev) TA_HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    else TA_HIP_TRY(ctx, hipEventSynchronize(ev));  // the last call's upload has left `host`
    host.resize((bytes + 7) / 8);
    n_bytes = bytes;
    *h = host.data();
    return TA_OK;
}
int HostTable::send(ta_ctx* ctx, hipStream_t st) {
    TA_HIP_TRY(ctx, hipMemcpyAsync(dev.p, host.data(), n_bytes, hipMemcpyHostToDevice, st));
    TA_HIP_TRY(ctx, hipEventRecord(ev, st));
    return TA_OK;
}

// timeline mark: the work queued on `st` from here to the next mark is `name`'s
void tl_mark(ta_ctx* ctx, const char* name, hipStream_t st) {
    if (!ctx->opt_timeline) return;
    if (ctx->marks_used == ctx->mark_pool.size()) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return;
        ctx->mark_pool.push_back(e);
    }
    hipEvent_t e = ctx->mark_pool[ctx->marks_used++];
    if (hipEventRecord(e, st) == hipSuccess) ctx->marks.push_back({name, e});
}
void tl_reset(ta_ctx* ctx) {
    ctx->marks.clear();
    ctx->marks_used = 0;
}

inline int64_t pm_pitch(int64_t n_frames) { return (n_frames + 7) / 8 * 8; }
inline size_t pm_bytes(int64_t n_frames, int64_t n_cols, bool f32 = false) {
    return (size_t)((n_cols + 1) / 2) * (size_t)pm_pitch(n_frames) * (f32 ? 8 : 16);
}

int get_wf_table(ta_ctx* ctx, int R0, int R, cd** out) {
    const int key = 64 * R0 + R;
    auto it = ctx->wf_tables.find(key);
    if (it != ctx->wf_tables.end()) {
        *out = it->second;
        return TA_OK;
    }
    std::vector<cd> a(wfft_table_elems(R0, R));
    wfft_fill_table(R0, R, a.data());
    cd* d = nullptr;
    TA_HIP_TRY(ctx, hipMalloc((void**)&d, sizeof(cd) * a.size()));
    hipError_t e = hipMemcpy(d, a.data(), sizeof(cd) * a.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(d);
        return fail(ctx, TA_E_HIP, std::string("twiddle table upload: ") + hipGetErrorString(e));
    }
    ctx->wf_tables[key] = d;
    *out = d;
    return TA_OK;
}

// ---- the brackets every timed call is made of -----------------------------------------------------------------------
// A compute call owns one event quadruple of the ring: call_begin records ev[0] and empties the timeline, call_end records
// ev[3] and counts the call (on success only: a call that failed leaves timing_valid false).  The *_dev entries open the
// bracket before their relayout, everyone else right before compute_pm / cond_pm, which close it.
int call_begin(ta_ctx* ctx, hipStream_t st) {
    ctx->timing_valid = false;
    ctx->ev = ctx->ring[ctx->n_calls % ta_ctx::kRing];
    TA_HIP_TRY(ctx, hipEventRecord(ctx->ev[0], st));
    tl_reset(ctx);
    return TA_OK;
}
int call_end(ta_ctx* ctx, hipStream_t st) {
    tl_mark(ctx, "end", st);
    TA_HIP_TRY(ctx, hipEventRecord(ctx->ev[3], st));
    ctx->timing_valid = true;
    ++ctx->n_calls;
    return TA_OK;
}

// one launch under its timeline name ...
#define TA_LAUNCH(ctx, name, st, launch)                                                                                  \
    do {                                                                                                                  \
        tl_mark(ctx, name, st);                                                                                           \
        TA_HIP_TRY(ctx, launch);                                                                                          \
    } while (0)
// ... and the call's main kernel: ev[1] / ev[2] around it are what ta_last_timing reports as the main kernel's time
#define TA_LAUNCH_MAIN(ctx, name, st, launch)                                                                             \
    do {                                                                                                                  \
        tl_mark(ctx, name, st);                                                                                           \
        TA_HIP_TRY(ctx, hipEventRecord(ctx->ev[1], st));                                                                  \
        TA_HIP_TRY(ctx, launch);                                                                                          \
        TA_HIP_TRY(ctx, hipEventRecord(ctx->ev[2], st));                                                                  \
    } while (0)

// The by-particle tail of every form whose kernel leaves atom-major lags in bp_scratch (pitch pm_pitch(T)): the
// transposition into the caller's (n_frames, ld_bp) array, which also adds up its 64 atoms per lag into a row of ts_partial
// (both ensured by the caller), then the sum of those tile rows.  halves: the kernel's units add undivided halves of a
// lag, the transposition divides once (k_band_bp_vacf).
int bp_tail(ta_ctx* ctx, int64_t T, int64_t A, double* d_lagsum, double* d_bp, int64_t ld_bp, hipStream_t st,
            bool halves = false) {
    const int64_t Tp = pm_pitch(T), n_tiles = (A + 63) / 64;
    TA_LAUNCH(ctx, "k_bp_transpose", st,
              launch_bp_transpose((const double*)ctx->bp_scratch.p, Tp, A, T, d_bp, ld_bp, (double*)ctx->ts_partial.p, st,
                                  halves));
    TA_LAUNCH(ctx, "k_sum_partials", st, launch_sum_partials((const double*)ctx->ts_partial.p, (int)n_tiles, T, d_lagsum, st));
    return TA_OK;
}

// ---- the O(T^2) forms --------------------------------------------------------------------------------------------------
// Which kernel evaluates a direct request.  "direct_mfma": 1 = by trajectory length (the default), 3 = the matrix cores
// always, 0 = the vector kernel always (the parity tests' second opinion); 0 / 3 leave k_short and k_mid aside too.
// (The column-packed forms of rounds 4-5 -- "direct_mfma" 2, inline-assembly LDS-DMA -- live under tools/band/ since round 6.)
enum Form { F_SHORT, F_MID, F_BAND_VACF64, F_BAND_HELF64, F_BAND_HELF32, F_VECTOR };

// the float32 option: products and block sums in float32 (float64 accumulation); the Einstein MSD stays float64
bool direct_f32(const ta_ctx* ctx, int mode) { return ctx->opt_direct_f32 != 0 && mode != MODE_MSD; }

// Short trajectories (short_kernels.hpp): a lane per column, every lag in its registers; the by-particle array is written in
// place, the lag sums leave as one row per wave
bool short_applies(const ta_ctx* ctx, int64_t T) { return T <= ctx->opt_short_max && T <= short_max_frames(); }

// src_f32: the slabs hold float32 elements; it only comes with the float32 option (compute_pm)
Form direct_form(const ta_ctx* ctx, int mode, int64_t T, bool src_f32 = false) {
    const int mf = (int)ctx->opt_direct_mfma;
    const bool f32 = direct_f32(ctx, mode), f64 = !f32 && !src_f32;
    if (f64 && mf == 1 && short_applies(ctx, T)) return F_SHORT;
    // k_mid where it wins (profiles/r06_direct_mid_sweep.txt): the windowed VACF from 97 to 512 frames (9.4 against 16.5 ms per
    // 12 GB at 128 frames with the by-particle array, 21.9 against 25.8 at 512), Helfand from 97 to 128 (18 against 23);
    // "mid_max" 0: never; "mid_all" 1: wherever the kernel can run (65 ... 512 frames, both quantities: the parity tests).
    // The Einstein MSD (no product stage) from 65 to 512 frames: 14 - 38 ms against the vector kernel's 21 - 44 per 12 GB
    // with the by-particle array, within 8 % where it loses (160 frames; tools/sweep_msd.py)
    if (f64 && mf == 1 && T > 64 && T <= ctx->opt_mid_max && T <= mid_max_frames() &&
        (ctx->opt_mid_all || mode == MODE_MSD || (T >= 97 && (mode == MODE_VACF || T <= 128))))
        return F_MID;
    // The O(T^2) correlators run on the matrix cores wherever that wins: FP64 (bandbp_kernels.hpp) and, for the float32
    // option's Helfand forms, FP32 (band32tp_kernels.hpp: P rounded once to float32 like the float32 vector kernel's staged
    // values, float32 products, float64 accumulation) -- the k-slots of the MFMA filled from the time axis.  These kernels
    // pay a ring fill and an epilogue per particle (block) and lag group; the vector kernel, whose column groups are 8 - 32
    // lanes under ~640 frames, wins the windowed VACF up to 512 frames, Helfand float64 up to 351, float32 up to 447
    // (profiles/r06_direct_mid_sweep.txt, 12 GB of input at every length).
    auto time_packed = [&](int64_t from_frames) { return mf == 3 || (mf == 1 && T >= from_frames); };
    if (T >= ((int64_t)1 << 24)) return F_VECTOR;
    if (f32 && mode == MODE_HELFAND && time_packed(448)) return F_BAND_HELF32;
    if (f64 && mode == MODE_VACF && time_packed(513)) return F_BAND_VACF64;
    if (f64 && mode == MODE_HELFAND && time_packed(352)) return F_BAND_HELF64;
    return F_VECTOR;
}

int short_impl(ta_ctx* ctx, int mode, const double* d_vel, const double* d_pos, const double* d_masses, int64_t T, int64_t A,
               int D, int64_t pitch, double scale, double* d_lagsum, double* d_bp, int64_t ld_bp, hipStream_t st) {
    const int nwg = short_grid(ctx->n_cu, mode, (int)T, A, D, d_bp != nullptr);
    const int rows = nwg * short_waves();
    int rc = ensure(ctx, ctx->ts_partial, sizeof(double) * (size_t)rows * T);
    if (rc) return rc;
    TA_LAUNCH_MAIN(ctx, "k_short", st,
                   launch_short(mode, nwg, d_vel, d_pos, d_masses, pitch, (int)T, A, D, mode == MODE_HELFAND ? scale / (double)D : 1.0,
                                d_bp, ld_bp, (double*)ctx->ts_partial.p, st));
    TA_LAUNCH(ctx, "k_sum_partials", st, launch_sum_partials((const double*)ctx->ts_partial.p, rows, T, d_lagsum, st));
    return TA_OK;
}

// 65 ... 512 frames (mid_kernels.hpp): a lane per (column, pair of 16-lag blocks), sliding window in registers
int mid_impl(ta_ctx* ctx, int mode, const double* d_vel, const double* d_pos, const double* d_masses, int64_t T, int64_t A, int D,
             int64_t pitch, double scale, double* d_lagsum, double* d_bp, int64_t ld_bp, hipStream_t st) {
    const int nwg = mid_grid(ctx->n_cu, mode, (int)T, A, D, (int)ctx->opt_mid_ncl);
    int rc = ensure(ctx, ctx->ts_partial, sizeof(double) * (size_t)nwg * T);
    if (rc) return rc;
    TA_LAUNCH_MAIN(ctx, "k_mid", st,
                   launch_mid(mode, nwg, d_vel, d_pos, d_masses, pitch, (int)T, A, D, mode == MODE_HELFAND ? scale / (double)D : 1.0,
                              d_bp, ld_bp, (double*)ctx->ts_partial.p, (int)ctx->opt_mid_ncl, st));
    TA_LAUNCH(ctx, "k_sum_partials", st, launch_sum_partials((const double*)ctx->ts_partial.p, nwg, T, d_lagsum, st));
    return TA_OK;
}

// The matrix-core forms, each with and without the by-particle array.  With it the kernel leaves atom-major lags and
// bp_tail follows; without, the kernel of the by-particle form runs with the particles of a unit summed in its
// accumulators (work handed out by a counter: windowed VACF 51.4 ms at 5000 x 50000 x 3, Helfand 463 ms per configs[4]
// share) and writes the lag sums itself.  The Helfand forms read the product slab P = (m v) x, made first (T*A*D*8 bytes
// more, 4 in float32).
struct BandForm {
    Form form;
    int slab_elem;    // bytes per element of the product slab helf_p (0: the kernel reads the velocities)
    bool q_partials;  // k_helfand_product also writes its row partials, into helf_small
    bool halves;      // bp_tail's flag
};
constexpr BandForm kBandForms[] = {{F_BAND_VACF64, 0, false, true},
                                   {F_BAND_HELF64, 8, true, false},
                                   {F_BAND_HELF32, 4, false, false}};

// Queues form f.  *queued false: a buffer could not be had (not an error of the call: the vector kernel needs none of
// them, and the caller goes on to it).
int band_impl(ta_ctx* ctx, const BandForm& f, const void* d_vel, const void* d_pos, bool src_f32, const double* d_masses, int64_t T,
              int64_t A, int D, int64_t pitch, double scale, double* d_lagsum, double* d_bp, int64_t ld_bp, hipStream_t st,
              bool* queued) {
    const int64_t n_cols = A * D, Tp = pm_pitch(T), n_tiles = (A + 63) / 64;
    const int n_parts = (int)std::min<int64_t>(1024, (n_cols + 1) / 2);
    const size_t scratch = d_bp ? (size_t)A * Tp : band_bp_helf_partial_doubles(ctx->n_cu, (int)T, A);
    *queued = (!f.slab_elem || ensure(ctx, ctx->helf_p, pm_bytes(T, n_cols, f.slab_elem == 4)) == TA_OK) &&
              (!f.q_partials || ensure(ctx, ctx->helf_small, sizeof(double) * (size_t)n_parts * T) == TA_OK) &&
              ensure(ctx, ctx->bp_scratch, sizeof(double) * scratch) == TA_OK &&
              (!d_bp || ensure(ctx, ctx->ts_partial, sizeof(double) * (size_t)n_tiles * T) == TA_OK) &&
              ensure(ctx, ctx->unit_counter, 64) == TA_OK;
    if (!*queued) {
        (void)hipGetLastError();
        return TA_OK;
    }
    double* part = (double*)ctx->bp_scratch.p;
    unsigned long long* counter = (unsigned long long*)ctx->unit_counter.p;
    const double factor = scale / (double)D;
    if (f.form == F_BAND_VACF64) {
        const double* v = (const double*)d_vel;
        if (d_bp)
            TA_LAUNCH_MAIN(ctx, "k_band_bp_vacf", st,
                           launch_band_bp_vacf(ctx->n_cu, v, pitch, (int)T, A, D, part, Tp, counter, st));
        else
            TA_LAUNCH_MAIN(ctx, "k_band_bp_vacf", st,
                           launch_band_bp_vacf_lags(ctx->n_cu, v, pitch, (int)T, A, D, part, counter, d_lagsum, st));
    } else if (f.form == F_BAND_HELF64) {
        const double* P = (const double*)ctx->helf_p.p;
        TA_LAUNCH(ctx, "k_helfand_product", st,
                  launch_helfand_product((const double*)d_vel, (const double*)d_pos, d_masses, pitch, T, n_cols, D,
                                         (double*)ctx->helf_p.p, (double*)ctx->helf_small.p, n_parts, st));
        if (d_bp)
            TA_LAUNCH_MAIN(ctx, "k_band_bp_helf", st,
                           launch_band_bp_helf(ctx->n_cu, P, pitch, (int)T, A, D, factor, part, Tp, counter, st));
        else
            TA_LAUNCH_MAIN(ctx, "k_band_bp_helf", st,
                           launch_band_bp_helf_lags(ctx->n_cu, P, pitch, (int)T, A, D, factor, part, counter, d_lagsum, st));
    } else {
        const float* P = (const float*)ctx->helf_p.p;
        TA_LAUNCH(ctx, "k_helfand_product32", st,
                  launch_helfand_product32(d_vel, d_pos, src_f32, d_masses, pitch, T, n_cols, D, (float*)ctx->helf_p.p, st));
        if (d_bp)
            TA_LAUNCH_MAIN(ctx, "k_band32_tp", st,
                           launch_band32_tp_bp(ctx->n_cu, P, pitch, (int)T, A, D, factor, part, Tp, counter, st));
        else
            TA_LAUNCH_MAIN(ctx, "k_band32_tp", st,
                           launch_band32_tp_lags(ctx->n_cu, P, pitch, (int)T, A, D, factor, part, counter, d_lagsum, st));
    }
    return d_bp ? bp_tail(ctx, T, A, d_lagsum, d_bp, ld_bp, st, f.halves) : TA_OK;
}

// Shape of the vector kernel's launch.  A thread owns one chunk pair (2L lags); a column group = W waves;
// a workgroup = G groups working on G atoms at once, so that ONE workgroup fills a CU's
// 16 wave slots (G*W <= 16) and its waves are dealt evenly to the 4 SIMDs.  The column
// must be resident next to the compute units: in LDS when it fits (float64: <= 16376
// frames, float32: <= 27296), otherwise in an L2-resident per-group staging buffer
// (slower, any length).  L (8 or 10 lags per chunk) is the one that wastes fewer lanes
// and SIMD slots for this n_frames.
// Trajectories under ~1000 frames have fewer chunk pairs than a wave has lanes: a column group is then 16 or 32 LANES
// ("direct_subwave" 1, the default), several groups per wave, up to 64 atoms per workgroup.
struct Shape {
    int L, GT, G;  // lags per chunk, threads per column group, groups per workgroup
    size_t col;    // bytes of a resident column
    bool gs;       // columns in the global staging buffer
    double eff;    // < 0: no chunk size is to be had ("direct_chunk")
};
Shape direct_shape(const ta_ctx* ctx, int64_t T, int64_t A, bool f32) {
    const size_t lds_cap = 160 * 1024;
    Shape best{0, 0, 0, 0, false, -1.0};
    for (int L : {8, 10}) {
        if (ctx->opt_direct_chunk > 0 && L != ctx->opt_direct_chunk) continue;
        if (!direct_chunk_supported(L)) continue;
        Shape c;
        c.L = L;
        c.col = direct_lds_bytes((int)T, f32, L);
        c.gs = c.col > lds_cap;
        const int npairs = ((int)((T + L - 1) / L) + 1) / 2;
        c.GT = 64 * std::min(16, (npairs + 63) / 64);  // threads per column group
        if (ctx->opt_direct_subwave && npairs <= 32) c.GT = npairs <= 8 ? 8 : npairs <= 16 ? 16 : 32;
        c.G = 1024 / c.GT;
        if (!c.gs) c.G = (int)std::min<size_t>(c.G, lds_cap / c.col);
        if (ctx->opt_direct_groups > 0) c.G = (int)std::min<int64_t>(c.G, ctx->opt_direct_groups);
        c.G = (int)std::max<int64_t>(1, std::min<int64_t>(c.G, A));
        if (c.GT < 64) c.G = std::max(64 / c.GT, c.G / (64 / c.GT) * (64 / c.GT));  // whole waves
        const int rounds = (npairs + c.GT - 1) / c.GT;
        const int waves = (c.G * c.GT + 63) / 64;
        c.eff = (double)npairs / ((double)rounds * c.GT) *       // active lanes
                (double)waves / (4.0 * ((waves + 3) / 4)) *      // SIMD balance
                (1.0 - 0.6 / L);                                 // per-tile overhead
        if (c.GT < 64)  // sub-wave groups: the lanes in use decide; at equal use 8 lags per chunk are 5 - 15 % ahead
            c.eff = 2.0 + (double)npairs / ((double)rounds * c.GT) * (L == 8 ? 1.0 : 0.93);
        if (c.eff > best.eff) best = c;
    }
    return best;
}

// One O(T^2) evaluation by the form direct_form names (the thresholds and where they were measured: there).  A matrix-core
// form that cannot have its buffers gives way to the vector kernel.
int direct_impl(ta_ctx* ctx, int mode, const void* d_vel, const void* d_pos,
                const double* d_masses, int64_t T, int64_t A, int D, int64_t pitch, double scale,
                double* d_lagsum, double* d_bp, int64_t ld_bp, hipStream_t st, bool src_f32 = false) {
    const Form form = direct_form(ctx, mode, T, src_f32);
    if (form == F_SHORT)
        return short_impl(ctx, mode, (const double*)d_vel, (const double*)d_pos, d_masses, T, A, D, pitch, scale, d_lagsum, d_bp,
                          ld_bp, st);
    if (form == F_MID)
        return mid_impl(ctx, mode, (const double*)d_vel, (const double*)d_pos, d_masses, T, A, D, pitch, scale, d_lagsum, d_bp, ld_bp,
                        st);
    int rc;
    for (const BandForm& f : kBandForms) {
        if (f.form != form) continue;
        bool queued = false;
        rc = band_impl(ctx, f, d_vel, d_pos, src_f32, d_masses, T, A, D, pitch, scale, d_lagsum, d_bp, ld_bp, st, &queued);
        if (rc || queued) return rc;
    }
    const bool f32 = direct_f32(ctx, mode);
    const Shape sh = direct_shape(ctx, T, A, f32);
    if (sh.eff < 0) return fail(ctx, TA_E_INVALID, "direct_chunk option: unsupported chunk size");
    const int nt = sh.G * sh.GT;
    const size_t lds = sh.gs ? 0 : sh.col * (size_t)sh.G;
    const int per_cu = direct_max_wg_per_cu(mode, f32, sh.L, nt, lds, sh.gs);
    int64_t nwg = ctx->opt_direct_nwg > 0 ? ctx->opt_direct_nwg : (int64_t)ctx->n_cu * per_cu;
    nwg = std::max<int64_t>(1, std::min<int64_t>(nwg, (A + sh.G - 1) / sh.G));
    const size_t rows = (size_t)nwg * sh.G;
    if ((rc = ensure(ctx, ctx->ts_partial, sizeof(double) * rows * T))) return rc;
    void* stage_buf = nullptr;
    if (sh.gs) {
        if ((rc = ensure(ctx, ctx->stage_buf, sh.col * rows))) return rc;
        stage_buf = ctx->stage_buf.p;
    }
    // by-particle values leave the kernel atom-major (contiguous stores) and are transposed
    // into the caller's (n_frames, ld_bp) array afterwards
    double* bp_am = nullptr;
    const int64_t Tp = pm_pitch(T);
    if (d_bp) {
        if ((rc = ensure(ctx, ctx->bp_scratch, sizeof(double) * (size_t)A * Tp))) return rc;
        bp_am = (double*)ctx->bp_scratch.p;
    }
    TA_LAUNCH(ctx, "memset", st, hipMemsetAsync(ctx->ts_partial.p, 0, sizeof(double) * rows * T, st));
    TA_LAUNCH_MAIN(ctx, "k_direct", st,
                   launch_direct(mode, f32, src_f32, sh.L, d_vel, d_pos, d_masses, pitch, (int)T, A, D, scale, bp_am, Tp,
                                 (double*)ctx->ts_partial.p, (int)nwg, nt, lds, stage_buf, sh.GT, st));
    TA_LAUNCH(ctx, "k_sum_partials", st, launch_sum_partials((const double*)ctx->ts_partial.p, (int)rows, T, d_lagsum, st));
    if (d_bp) TA_LAUNCH(ctx, "k_bp_transpose", st, launch_bp_transpose(bp_am, Tp, A, T, d_bp, ld_bp, nullptr, st));
    return TA_OK;
}


// ---- compute on pair-major slabs (every entry point ends up here) --------------------------
// FFT VACF (wfft.hpp): n_frames <= 512 the wave-independent 512-point kernels; up to 10240 frames
// one on-chip transform per pass (R = 1), up to 163840 frames an outer radix R <= 16 in front of
// it; beyond that the direct correlator (same quantity: velocityautocorr.py:217-238 == :208-215
// mathematically).  Lag sums: forward kernel -> partial spectra per tuple of workgroups -> their
// sum -> ONE inverse transform.  By-particle array: per block of atoms, forward kernel -> the
// atoms' power spectra in scratch -> inverse kernel -> atom-major lags; then bp_tail.
// pm_f32: the slab holds float32 elements (fft_reads_f32 says for which lengths the kernels take it)
bool fft_reads_f32(int64_t T) {
    int R0 = 0, R = 1;
    return wfft_choose((long)T, &R0, &R) && R == 1 && R0 > 1;
}

int fft_impl(ta_ctx* ctx, const double* pm, int64_t pitch, int64_t T, int64_t A, int D,
             double* d_lagsum, double* d_bp, int64_t ld_bp, hipStream_t st, bool pm_f32 = false) {
    int rc;
    const int64_t n_cols = A * D, n_pairs = (n_cols + 1) / 2;
    int R0 = 0, R = 1;
    if (!wfft_choose((long)T, &R0, &R))
        return direct_impl(ctx, MODE_VACF, pm, nullptr, nullptr, T, A, D, pitch, 1.0, d_lagsum, d_bp, ld_bp, st);
    if (!pm_f32 && short_applies(ctx, T) && (d_bp || T <= ctx->opt_short_lags_max))
        return short_impl(ctx, MODE_VACF, pm, nullptr, nullptr, T, A, D, pitch, 1.0, d_lagsum, d_bp, ld_bp, st);
    cd* tw = nullptr;
    if ((rc = get_wf_table(ctx, R0, R, &tw))) return rc;
    const int64_t Tp = pm_pitch(T), n_tiles = (A + 63) / 64;
    const int64_t L = 2L * R * R0 * 512;  // doubles per spectrum
    const int64_t cap = ctx->opt_fft_nwg > 0 ? ctx->opt_fft_nwg : (int64_t)ctx->n_cu * wfft_max_wg_per_cu(R0);
    // forward grid: whole tuples of 2R workgroups on each of the 8 XCDs, no more tuples than groups of units
    auto forward_grid = [&](int64_t n_groups) {
        const int64_t gran = 16 * R;
        return std::max<int64_t>(gran, std::min<int64_t>(cap, 2 * R * n_groups) / gran * gran);
    };
    if (d_bp) {
        if ((rc = ensure(ctx, ctx->bp_scratch, sizeof(double) * (size_t)A * Tp))) return rc;
        if ((rc = ensure(ctx, ctx->ts_partial, sizeof(double) * (size_t)n_tiles * T))) return rc;
    }
    if (R0 == 1) {
        if (!d_bp) {
            const int64_t nwg = std::max<int64_t>(1, std::min(cap, (n_pairs + 3) / 4));  // a wave per pair
            const int n_parts = (int)(4 * nwg);
            if ((rc = ensure(ctx, ctx->partial, sizeof(double) * (size_t)n_parts * L))) return rc;
            if ((rc = ensure(ctx, ctx->spec, sizeof(double) * (size_t)L))) return rc;
            TA_LAUNCH_MAIN(ctx, "k_w1_accum", st,
                           launch_w1_accum((int)nwg, st, pm, pitch, (int)T, n_pairs, tw, (double*)ctx->partial.p));
            TA_LAUNCH(ctx, "k_wf_sum+k_wf_fold+k_wf_lags", st,
                      launch_wfft_finish(R0, (const double*)ctx->partial.p, n_parts, tw, (int)T, (double*)ctx->spec.p, d_lagsum, st));
            return TA_OK;
        }
        const int64_t nwg = std::max<int64_t>(1, std::min(cap, (A + 3) / 4));  // a wave per atom
        TA_LAUNCH_MAIN(ctx, "k_w1_bp", st,
                       launch_w1_bp((int)nwg, st, pm, pitch, (int)T, A, D, tw, (double*)ctx->bp_scratch.p, Tp));
    } else if (!d_bp) {
        const int64_t nwg = forward_grid(n_pairs), n_tuples = nwg / (2 * R);
        if ((rc = ensure(ctx, ctx->partial, sizeof(double) * (size_t)n_tuples * L))) return rc;
        if ((rc = ensure(ctx, ctx->spec, sizeof(double) * (size_t)L))) return rc;
        TA_LAUNCH_MAIN(ctx, "k_wsplit_accum", st,
                       launch_wfft_forward(R0, R, false, pm_f32, (int)nwg, st, pm, pitch, (int)T, n_pairs, D, tw,
                                           (double*)ctx->partial.p));
        // the summed spectrum -> lag sums: ONE inverse transform per launch
        TA_LAUNCH(ctx, "k_sum_partials", st,
                  launch_sum_partials((const double*)ctx->partial.p, (int)n_tuples, L, (double*)ctx->spec.p, st));
        TA_LAUNCH(ctx, "k_winverse", st,
                  launch_wfft_inverse(R0, R, 1, st, (const double*)ctx->spec.p, (int)T, 1, tw, d_lagsum, 0, 0));
        return TA_OK;
    } else {
        // blocks of atoms sized by the spectrum scratch (2.5 GiB unless the bp_spec_atoms option
        // says otherwise); a block starts on an even atom, so on a column-pair boundary
        const size_t spec_bytes = sizeof(double) * (size_t)L;
        int64_t CA = ctx->opt_bp_spec_atoms > 0 ? ctx->opt_bp_spec_atoms : (int64_t)(((size_t)5 << 29) / spec_bytes);
        CA = std::min<int64_t>(A, std::max<int64_t>(2, (CA + 1) / 2 * 2));
        {  // equal blocks instead of full ones and a remainder
            const int64_t n_blocks = (A + CA - 1) / CA;
            CA = std::min<int64_t>(CA, ((A + n_blocks - 1) / n_blocks + 1) / 2 * 2);
        }
        if ((rc = ensure(ctx, ctx->bp_spec, spec_bytes * (size_t)CA))) return rc;
        // (the main-kernel interval spans every block's pair of launches)
        TA_HIP_TRY(ctx, hipEventRecord(ctx->ev[1], st));
        for (int64_t a0 = 0; a0 < A; a0 += CA) {
            const int64_t ca = std::min(CA, A - a0);
            const int64_t groups = D & 1 ? (ca + 1) / 2 : ca;  // a tuple of workgroups per group of atoms
            // (a block starts on a column-pair boundary; pairs of a float32 slab are 8-byte rows)
            const double* pm_blk = pm_f32 ? (const double*)((const float*)pm + (a0 * D / 2) * pitch * 2)
                                          : pm + (a0 * D / 2) * pitch * 2;
            TA_LAUNCH(ctx, "k_wsplit_accum", st,
                      launch_wfft_forward(R0, R, true, pm_f32, (int)forward_grid(groups), st, pm_blk, pitch, (int)T, ca, D, tw,
                                          (double*)ctx->bp_spec.p));
            TA_LAUNCH(ctx, "k_winverse", st,
                      launch_wfft_inverse(R0, R, (int)std::min<int64_t>(cap, ca), st, (const double*)ctx->bp_spec.p, (int)T, ca, tw,
                                          (double*)ctx->bp_scratch.p + a0 * Tp, Tp, (int)ctx->opt_bp_prefetch));
        }
        TA_HIP_TRY(ctx, hipEventRecord(ctx->ev[2], st));
    }
    return bp_tail(ctx, T, A, d_lagsum, d_bp, ld_bp, st);
}

// Mean squared differences of a prepared slab as S1 - 2 S2 (helfand_fft.hip), wherever wfft_choose has a plan: the
// prepare kernel writes P and its squares' sums (lag sums: row partials Qpart, summed into Q; by particle: Ca per atom),
// fft_impl gives S2 as the autocorrelation of P, the combine kernels put factor * (S1 - 2 S2) together.
bool s1_2s2_applies(int64_t T) {
    int r0 = 0, ro = 0;
    return T >= 2 && wfft_choose((long)T, &r0, &ro);
}
enum Prepare { PREP_HELFAND /* P = (m v) x */, PREP_MSD /* P = x - x[t=0] (msd.hip) */ };

// pm: the velocities (PREP_MSD: the positions, and nothing else)
int s1_2s2_impl(ta_ctx* ctx, Prepare prep, const double* pm, const double* pm_pos, const double* d_masses, int64_t pitch, int64_t T,
                int64_t A, int D, double factor, double* d_lagsum, double* d_bp, int64_t ld_bp, hipStream_t st) {
    int rc;
    const int64_t n_cols = A * D, n_pairs = (n_cols + 1) / 2;
    const char* name = prep == PREP_HELFAND ? "k_helfand_product" : "k_msd_prepare";
    if ((rc = ensure(ctx, ctx->helf_p, pm_bytes(T, n_cols)))) return rc;
    double* P = (double*)ctx->helf_p.p;
    if (!d_bp) {
        const int n_parts = (int)std::min<int64_t>(1024, n_pairs);
        if ((rc = ensure(ctx, ctx->helf_small, sizeof(double) * ((size_t)n_parts * T + 3 * (size_t)T + 1)))) return rc;
        double* Qpart = (double*)ctx->helf_small.p;
        double* Q = Qpart + (size_t)n_parts * T;
        double* S2 = Q + T;
        double* C = S2 + T;
        TA_LAUNCH(ctx, name, st,
                  prep == PREP_HELFAND ? launch_helfand_product(pm, pm_pos, d_masses, pitch, T, n_cols, D, P, Qpart, n_parts, st)
                                       : launch_msd_prepare(pm, pitch, T, n_cols, P, Qpart, n_parts, st));
        TA_LAUNCH(ctx, "k_sum_partials", st, launch_sum_partials(Qpart, n_parts, T, Q, st));
        if ((rc = fft_impl(ctx, P, pitch, T, A, D, S2, nullptr, 0, st))) return rc;
        TA_LAUNCH(ctx, "k_helfand_combine", st, launch_helfand_combine(Q, S2, C, (int)T, factor, d_lagsum, st));
        return TA_OK;
    }
    if ((rc = ensure(ctx, ctx->helf_small, sizeof(double) * ((size_t)T + 1) * A))) return rc;
    double* Ca = (double*)ctx->helf_small.p;
    if (n_cols & 1)  // the unpaired last column's partner is never written by the prepare kernel
        TA_HIP_TRY(ctx, hipMemsetAsync(P + (size_t)(n_pairs - 1) * pitch * 2, 0, (size_t)pitch * 16, st));
    TA_LAUNCH(ctx, name, st,
              prep == PREP_HELFAND ? launch_helfand_product_bp(pm, pm_pos, d_masses, pitch, T, A, D, P, Ca, st)
                                   : launch_msd_prepare_bp(pm, pitch, T, A, D, P, Ca, st));
    if ((rc = fft_impl(ctx, P, pitch, T, A, D, d_lagsum, d_bp, ld_bp, st))) return rc;
    TA_LAUNCH(ctx, "k_helfand_combine", st, launch_helfand_combine_bp(Ca, A, (int)T, factor, d_bp, ld_bp, st));
    TA_LAUNCH(ctx, "k_row_sums", st, launch_row_sums(d_bp, T, A, ld_bp, d_lagsum, st));
    return TA_OK;
}

// Helfand mean squared differences (viscosity.py:201-233); the "helfand_fft" option evaluates
// them as S1 - 2 S2 where an FFT path exists for the request.
int helfand_impl(ta_ctx* ctx, const double* pm_vel, const double* pm_pos, const double* d_masses,
                 int64_t pitch, int64_t T, int64_t A, int D, double scale, double* d_lagsum,
                 double* d_bp, int64_t ld_bp, hipStream_t st) {
    if (ctx->opt_helfand_fft && s1_2s2_applies(T))
        return s1_2s2_impl(ctx, PREP_HELFAND, pm_vel, pm_pos, d_masses, pitch, T, A, D, scale / (double)D, d_lagsum, d_bp,
                           ld_bp, st);
    return direct_impl(ctx, MODE_HELFAND, pm_vel, pm_pos, d_masses, T, A, D, pitch, scale, d_lagsum, d_bp,
                       ld_bp, st);
}

// Einstein MSD (MDAnalysis.analysis.msd.EinsteinMSD) on the position slab alone.  fft: up to short_max frames k_short
// (exact, and faster there, as for the VACF); beyond, S1 - 2 S2 on P = x - x[t=0] (the combine kernels with factor 1)
// wherever wfft_choose has a plan.  !fft, and fft beyond the largest plan: the direct forms under
// direct_form's thresholds (k_short up to 64 frames, k_mid 65 ... 512: re-measured for MSD, k_direct beyond).
int msd_impl(ta_ctx* ctx, bool fft, const double* pm_pos, int64_t pitch, int64_t T, int64_t A, int D, double* d_lagsum,
             double* d_bp, int64_t ld_bp, hipStream_t st) {
    if (fft && direct_form(ctx, MODE_MSD, T) != F_SHORT && s1_2s2_applies(T))
        return s1_2s2_impl(ctx, PREP_MSD, pm_pos, nullptr, nullptr, pitch, T, A, D, 1.0, d_lagsum, d_bp, ld_bp, st);
    return direct_impl(ctx, MODE_MSD, pm_pos, nullptr, nullptr, T, A, D, pitch, 1.0, d_lagsum, d_bp, ld_bp, st);
}

// float32 device slab -> *pm: its float64 copy (same layout) in the context's scratch slab k
int widen_input(ta_ctx* ctx, int k, int64_t pitch, int64_t n_cols, hipStream_t st, const void** pm) {
    const size_t n_el = (size_t)((n_cols + 1) / 2) * (size_t)pitch * 2;
    int rc = ensure(ctx, ctx->pm_in[k], n_el * sizeof(double));
    if (rc) return rc;
    TA_LAUNCH(ctx, "k_widen_f32", st, launch_widen_f32((const float*)*pm, (double*)ctx->pm_in[k].p, (long)n_el, st));
    *pm = ctx->pm_in[k].p;
    return TA_OK;
}

// one compute call on pair-major slabs; the caller has opened the call's bracket (call_begin), it is closed here
int compute_pm(ta_ctx* ctx, int which, const void* pm_vel_any, const void* pm_pos_any, const double* d_masses,
               int64_t pitch, int64_t T, int64_t A, int D, double scale, double* d_lagsum, double* d_bp,
               int64_t ld_bp, hipStream_t st, bool pm_f32 = false) {
    int rc;
    // float32 device slabs are read as they are by the float32 direct correlators; every other
    // evaluation works on a float64 copy (same layout) in the context's scratch slabs
    const bool direct_on_f32 = pm_f32 && ctx->opt_direct_f32 &&
                               (which == W_DIRECT || (which == W_HELFAND && !(ctx->opt_helfand_fft && T >= 2)));
    // ... and by the FFT kernels of the plans without an outer radix (513 ... 10240 frames)
    const bool fft_on_f32 = pm_f32 && which == W_FFT && fft_reads_f32(T);
    if (pm_f32 && !direct_on_f32 && !fft_on_f32) {
        if ((rc = widen_input(ctx, 0, pitch, A * D, st, &pm_vel_any))) return rc;
        if (pm_pos_any && (rc = widen_input(ctx, 1, pitch, A * D, st, &pm_pos_any))) return rc;
    }
    const double* pm_vel = (const double*)pm_vel_any;
    const double* pm_pos = (const double*)pm_pos_any;
    // paths without a dominant kernel of their own re-record ev[1]/ev[2] inside
    TA_HIP_TRY(ctx, hipEventRecord(ctx->ev[1], st));
    TA_HIP_TRY(ctx, hipEventRecord(ctx->ev[2], st));
    if (which == W_FFT) rc = fft_impl(ctx, pm_vel, pitch, T, A, D, d_lagsum, d_bp, ld_bp, st, fft_on_f32);
    else if (which == W_DIRECT)
        rc = direct_impl(ctx, MODE_VACF, pm_vel_any, nullptr, nullptr, T, A, D, pitch, 1.0, d_lagsum, d_bp, ld_bp, st,
                         direct_on_f32);
    else if (is_msd(which))
        rc = msd_impl(ctx, which == W_MSD_FFT, pm_vel, pitch, T, A, D, d_lagsum, d_bp, ld_bp, st);
    else if (direct_on_f32)
        rc = direct_impl(ctx, MODE_HELFAND, pm_vel_any, pm_pos_any, d_masses, T, A, D, pitch, scale, d_lagsum, d_bp,
                         ld_bp, st, true);
    else rc = helfand_impl(ctx, pm_vel, pm_pos, d_masses, pitch, T, A, D, scale, d_lagsum, d_bp, ld_bp, st);
    return rc ? rc : call_end(ctx, st);
}

// frame-major device input of a *_dev entry point -> the context's pair-major scratch slab
int relayout_input(ta_ctx* ctx, int k, const double* d_src, int64_t T, int64_t n_cols, int64_t ld_row,
                   hipStream_t st, const double** out) {
    int rc = ensure(ctx, ctx->pm_in[k], pm_bytes(T, n_cols));
    if (rc) return rc;
    TA_LAUNCH(ctx, "k_relayout", st, launch_relayout(d_src, false, ld_row, n_cols, T, ctx->pm_in[k].p, false, pm_pitch(T), 0, st));
    *out = (const double*)ctx->pm_in[k].p;
    return TA_OK;
}

int dev_entry(ta_ctx* ctx, int which, const double* d_vel, const double* d_pos, const double* d_masses,
              int64_t T, int64_t A, int D, int64_t ld_row, double scale, double* d_lagsum, double* d_bp,
              int64_t ld_bp, void* stream) {
    TA_NO_CPU(ctx);
    int rc = check_shape(ctx, T, A, D, ld_row);
    if (rc) return rc;
    if (!d_vel || !d_lagsum || (which == W_HELFAND && (!d_pos || !d_masses)))
        return fail(ctx, TA_E_INVALID, "null device pointer");
    if (d_bp && ld_bp < A) return fail(ctx, TA_E_INVALID, "ld_bp smaller than n_atoms");
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;  // NULL = the legacy default stream, as for any HIP call
    if ((rc = call_begin(ctx, st))) return rc;
    const double *pv = nullptr, *px = nullptr;
    if ((rc = relayout_input(ctx, 0, d_vel, T, A * D, ld_row, st, &pv))) return rc;
    if (which == W_HELFAND && (rc = relayout_input(ctx, 1, d_pos, T, A * D, ld_row, st, &px))) return rc;
    return compute_pm(ctx, which, pv, px, d_masses, pm_pitch(T), T, A, D, scale, d_lagsum, d_bp, ld_bp, st);
}

// frames committed by ta_stage_commit travel on the context's own stream: a caller's stream that
// is about to touch the slabs waits for them (a no-op when nothing is pending)
int order_after_staging(ta_ctx* ctx, hipStream_t st) {
    if (int rc = ctx->commits.flush()) return rc;  // queued commits have made their calls on ctx->stream
    if (st == ctx->stream) return TA_OK;
    TA_HIP_TRY(ctx, hipEventRecord(ctx->ev_stage, ctx->stream));
    TA_HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_stage, 0));
    return TA_OK;
}

int staged_entry(ta_ctx* ctx, int which, const double* d_masses, double scale, double* d_lagsum,
                 double* d_bp, int64_t ld_bp, void* stream) {
    TA_CHECK(need_ctx(ctx));
    TA_NO_CPU(ctx);
    const int need = slabs_needed(which);
    TA_CHECK(check_staged(ctx, need));
    if (!d_lagsum || (which == W_HELFAND && !d_masses)) return fail(ctx, TA_E_INVALID, "null device pointer");
    if (d_bp && ld_bp < ctx->st_A) return fail(ctx, TA_E_INVALID, "ld_bp smaller than n_atoms");
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = order_after_staging(ctx, (hipStream_t)stream);
    if (rc || (rc = call_begin(ctx, (hipStream_t)stream))) return rc;
    return compute_pm(ctx, which, ctx->d_slabs[0], need == 2 ? ctx->d_slabs[1] : nullptr, d_masses,
                      ctx->st_pitch, ctx->st_T, ctx->st_A, ctx->st_D, scale, d_lagsum, d_bp, ld_bp,
                      (hipStream_t)stream, ctx->st_dev_f32);
}

// ---- the slab bracket of the collective quantities (conductivity, moments, currents, species self terms) ------------
// Where a call's pair-major slab is, and the stream the call runs on
struct Slab {
    const void* pm;
    bool f32;
    int64_t pitch, T, A;
    int D;
    hipStream_t st;
    const void* pm1 = nullptr;  // staged slab 1 where there is one (the positions behind slab 0's velocities)
};
// the frame-major device input of a *_dev entry
struct DevSrc {
    const double* d;
    int64_t T, A;
    int D;
    int64_t ld_row;
};
constexpr auto no_args = []() -> int { return TA_OK; };
constexpr auto no_pre = [](const Slab&) -> int { return TA_OK; };

// One call on slab 0: of `dev` (a *_dev entry: check_shape, the call opened, then its relayout into the scratch slab) or,
// dev NULL, the staged one (check_staged; the caller's stream ordered behind the queued commits, then the call opened).
// args(): the entry's own argument checks, at their place among the shared ones; pre(slab): what the call queues or
// allocates BEFORE it is opened (uploads, self_plan; slab.pm of a *_dev entry is not set yet); body(slab) closes the call.
template <class Args, class Pre, class Body>
int slab_entry(ta_ctx* ctx, const DevSrc* dev, void* stream, Args&& args, Pre&& pre, Body&& body) {
    if (dev) {
        TA_NO_CPU(ctx);
        TA_CHECK(check_shape(ctx, dev->T, dev->A, dev->D, dev->ld_row));
        TA_CHECK(args());
        if (!dev->d) return fail(ctx, TA_E_INVALID, "null device pointer");
    } else {
        TA_CHECK(need_ctx(ctx));
        TA_NO_CPU(ctx);
        TA_CHECK(args());
        TA_CHECK(check_staged(ctx));
    }
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;  // NULL = the legacy default stream, as for any HIP call
    Slab s = dev ? Slab{nullptr, false, pm_pitch(dev->T), dev->T, dev->A, dev->D, st}
                 : Slab{ctx->d_slabs[0], ctx->st_dev_f32, ctx->st_pitch, ctx->st_T, ctx->st_A, ctx->st_D, st};
    if (!dev && ctx->st_nslabs > 1) s.pm1 = ctx->d_slabs[1];
    TA_CHECK(pre(s));
    if (!dev) TA_CHECK(order_after_staging(ctx, st));
    TA_CHECK(call_begin(ctx, st));
    if (dev) {
        const double* px = nullptr;
        TA_CHECK(relayout_input(ctx, 0, dev->d, s.T, s.A * s.D, dev->ld_row, st, &px));
        s.pm = px;
    }
    return body(s);
}

// ---- Einstein-Helfand conductivity (conductivity.hip) ---------------------------------------------------------------
// Phi(k) of the (n_frames, dim) frame-major moment at d_moment: its pair-major copy is a one-atom slab, and its MSD lag
// sum (msd_impl, the EinsteinMSD dispatch) is Phi.
int cond_collective(ta_ctx* ctx, bool fft, const double* d_moment, int64_t T, int D, double* d_coll, hipStream_t st) {
    int rc = ensure(ctx, ctx->cond_mpm, pm_bytes(T, D));
    if (rc) return rc;
    TA_LAUNCH(ctx, "k_relayout", st, launch_relayout(d_moment, false, D, D, T, ctx->cond_mpm.p, false, pm_pitch(T), 0, st));
    return msd_impl(ctx, fft, (const double*)ctx->cond_mpm.p, pm_pitch(T), T, 1, D, d_coll, nullptr, 0, st);
}

// One conductivity call on a pair-major position slab (the caller has opened the call's bracket, it is closed here): the
// moment pass (and with d_self the weighted slab W = q (x - x[0])), the fixed-order sum of its partials into d_moment,
// then the self term = the MSD lag sum of W (sum_n q_n^2 MSD_n: the MSD is invariant under the shift and |d(q x)|^2 = q^2 |dx|^2) and the
// collective Phi of the moment, each by msd_impl.  d_coll / d_self NULL: skipped.  ev[1] / ev[2] bracket the moment
// pass, unless an FFT evaluation after it records its own forward kernel there.
int cond_pm(ta_ctx* ctx, bool fft, const Slab& s, const double* d_q, double* d_moment, double* d_coll, double* d_self) {
    int rc;
    const int64_t pitch = s.pitch, T = s.T, A = s.A, n_cols = s.A * s.D;
    const int D = s.D;
    hipStream_t st = s.st;
    const void* pm_any = s.pm;
    // float32 device slabs: a float64 copy first, as for every other evaluation but the float32 kernels
    if (s.f32 && (rc = widen_input(ctx, 0, pitch, n_cols, st, &pm_any))) return rc;
    const double* pm = (const double*)pm_any;
    const int n_parts = cond_moment_parts(ctx->n_cu, (long)T, (long)n_cols);
    if ((rc = ensure(ctx, ctx->cond_part, sizeof(double) * (size_t)n_parts * T * D))) return rc;
    double* W = nullptr;
    if (d_self) {
        if ((rc = ensure(ctx, ctx->cond_w, pm_bytes(T, n_cols)))) return rc;
        W = (double*)ctx->cond_w.p;
    }
    TA_LAUNCH_MAIN(ctx, "k_cond_moment", st,
                   launch_cond_moment(pm, (long)pitch, (long)T, (long)n_cols, D, d_q, (double*)ctx->cond_part.p, n_parts, W, st));
    TA_LAUNCH(ctx, "k_sum_partials", st,
              launch_sum_partials((const double*)ctx->cond_part.p, n_parts, (long)(T * D), d_moment, st));
    if (d_self && (rc = msd_impl(ctx, fft, W, pitch, T, A, D, d_self, nullptr, 0, st))) return rc;
    if (d_coll && (rc = cond_collective(ctx, fft, d_moment, T, D, d_coll, st))) return rc;
    return call_end(ctx, st);
}

int cond_args(ta_ctx* ctx, int fft, const void* charges, const void* moment) {
    TA_CHECK(check_fft(ctx, fft));
    if (!charges) return fail(ctx, TA_E_INVALID, "charges are NULL");
    if (!moment) return fail(ctx, TA_E_INVALID, "moment output is NULL");
    return TA_OK;
}

// ---- species-collective quantities: Onsager moments, Green-Kubo currents (species_sum.hip) ---------------------------
// Per-species sums over atoms Q_s[t, d] in ONE pass over the slab, and their cross-correlation C[k, i, j] by polarisation.
// The two quantities run the same host code; Collective holds everything that differs between them.

// the VACF's dispatch with msd_impl's signature (the by-particle autocorrelations of the currents, the VACF self terms)
int acf_impl(ta_ctx* ctx, bool fft, const double* pm, int64_t pitch, int64_t T, int64_t A, int D, double* d_lagsum, double* d_bp,
             int64_t ld_bp, hipStream_t st) {
    if (fft) return fft_impl(ctx, pm, pitch, T, A, D, d_lagsum, d_bp, ld_bp, st);
    return direct_impl(ctx, MODE_VACF, pm, nullptr, nullptr, T, A, D, pitch, 1.0, d_lagsum, d_bp, ld_bp, st);
}

struct Collective {
    const char* noun;       // of the sums, in messages
    const char* pass_name;  // the pass that forms every species' sum (k_species_sum): the call's main kernel
    // the pass subtracts frame 0.  The shifted pass reads float64 only, so this also says that a float32 slab gets a
    // float64 copy first (as cond_pm does); without it the pass reads the slab as it is
    bool shift;
    // the (T, S^2) by-particle lag sums of the pseudo-particles under the polarisation step
    int (*corr)(ta_ctx*, bool fft, const double* pm, int64_t pitch, int64_t T, int64_t A, int D, double* d_lagsum, double* d_bp,
                int64_t ld_bp, hipStream_t st);
    const char* finish_name;  // of k_cross_finish
    bool lag0;  // C[0] is kept (<Q_i . Q_j>), or exactly 0 (a mean squared difference: one frame needs no kernel at all)
    // the CPU backend's whole call and its cross term
    int (*cpu)(const ta::cpu::State&, bool fft, int S, const int32_t* species, const double* w, double* sums, double* cross);
    int (*cpu_cross)(int threads, bool fft, const double* sums, int S, int64_t T, int D, double* cross);
};
// indexed by ta::CollKind.  Moments: Q = w (x - x[0]), C_ij = 1/4 (MSD(M_i + M_j) - MSD(M_i - M_j)) by the EinsteinMSD
// dispatch.  Currents: Q = w v of a slab of either element type, C_ij = 1/4 (ACF(J_i + J_j) - ACF(J_i - J_j)) by the VACF's.
constexpr Collective kCollective[2] = {
    {"moments", "k_species_moment", true, msd_impl, "k_onsager_finish", false, ta::cpu::onsager, ta::cpu::onsager_cross},
    {"currents", "k_species_current", false, acf_impl, "k_current_finish", true, ta::cpu::current, ta::cpu::current_cross},
};

// C[k, i, j] of the (S, T, D) sums at d_sums into d_cross (T, S, S), by polarisation in ONE q.corr call: the S^2
// pseudo-particles Q_i, Q_i + Q_j, Q_i - Q_j as a pair-major slab (k_onsager_combos, in the Onsager workspaces), their
// (T, S^2) by-particle lag sums with the call's fft, then the finish.
int coll_cross(ta_ctx* ctx, const Collective& q, bool fft, const double* d_sums, int S, int64_t T, int D, double* d_cross,
               hipStream_t st) {
    const int64_t P = (int64_t)S * S, pitch = pm_pitch(T);
    if (!q.lag0 && T < 2) {  // lag 0 alone: exactly 0
        TA_HIP_TRY(ctx, hipMemsetAsync(d_cross, 0, sizeof(double) * (size_t)(T * P), st));
        return TA_OK;
    }
    TA_CHECK(ensure(ctx, ctx->ons_pm, pm_bytes(T, P * D)));
    TA_CHECK(ensure(ctx, ctx->ons_bp, sizeof(double) * (size_t)(T * P + T) + sizeof(int) * TA_ONSAGER_MAX_SPECIES));
    double* bp = (double*)ctx->ons_bp.p;
    double* lagsum = bp + T * P;
    int* nz = (int*)(lagsum + T);
    TA_HIP_TRY(ctx, hipMemsetAsync(nz, 0, sizeof(int) * TA_ONSAGER_MAX_SPECIES, st));
    TA_LAUNCH(ctx, "k_onsager_combos", st, launch_onsager_combos(d_sums, S, (long)T, D, (long)pitch, (double*)ctx->ons_pm.p, nz, st));
    TA_CHECK(q.corr(ctx, fft, (const double*)ctx->ons_pm.p, pitch, T, P, D, lagsum, bp, P, st));
    TA_LAUNCH(ctx, q.finish_name, st, launch_cross_finish(bp, S, (long)T, nz, q.lag0, d_cross, st));
    return TA_OK;
}

// One call on a pair-major slab (the caller has opened the call's bracket, it is closed here): the one pass that forms
// every species' sum, the fixed-order sum of its partials into d_sums (S, T, D), and with d_cross their cross term.
// ev[1] / ev[2] bracket the pass, unless an FFT evaluation after it records its own forward kernel there.
int coll_pm(ta_ctx* ctx, const Collective& q, bool fft, const Slab& s, int S, const int32_t* d_species, const double* d_w,
            double* d_sums, double* d_cross) {
    const int64_t T = s.T, n_cols = s.A * s.D;
    TA_CHECK(check_cols(ctx, std::string("Onsager ") + q.noun + ": ", s.A, s.D));
    const void* pm = s.pm;
    const bool widen = s.f32 && q.shift;
    if (widen) TA_CHECK(widen_input(ctx, 0, s.pitch, n_cols, s.st, &pm));
    const int n_parts = species_sum_parts(ctx->n_cu, S, (long)T, (long)n_cols);
    const size_t n_out = (size_t)S * T * s.D;
    TA_CHECK(ensure(ctx, ctx->ons_part, sizeof(double) * (size_t)n_parts * n_out));
    TA_LAUNCH_MAIN(ctx, q.pass_name, s.st,
                   launch_species_sum(pm, s.f32 && !widen, q.shift, (long)s.pitch, (long)T, (long)n_cols, s.D, S, d_species, d_w,
                                      (double*)ctx->ons_part.p, n_parts, s.st));
    TA_LAUNCH(ctx, "k_sum_partials", s.st, launch_sum_partials((const double*)ctx->ons_part.p, n_parts, (long)n_out, d_sums, s.st));
    if (d_cross) TA_CHECK(coll_cross(ctx, q, fft, d_sums, S, T, s.D, d_cross, s.st));
    return call_end(ctx, s.st);
}

// The weighted total of a pair-major block of n atoms with D columns each, sum_n w_n x[t, n, :] -> d_total (T, D): ONE
// species-sum pass without shift (one species: the n zero labels d_lab; d_w NULL: weights 1) and the fixed-order sum of
// its partials.  n_parts = species_sum_parts(n_cu, 1, T, n D), and ons_part holds n_parts T D doubles: the caller's ensure,
// which comes before its launches.
int weighted_total(ta_ctx* ctx, const void* pm, bool f32, int64_t pitch, int64_t T, int64_t n, int D, const int* d_lab,
                   const double* d_w, int n_parts, double* d_total, hipStream_t st) {
    TA_LAUNCH(ctx, "k_species_current", st,
              launch_species_sum(pm, f32, false, (long)pitch, (long)T, (long)(n * D), D, 1, d_lab, d_w, (double*)ctx->ons_part.p,
                                 n_parts, st));
    TA_LAUNCH(ctx, "k_sum_partials", st, launch_sum_partials((const double*)ctx->ons_part.p, n_parts, (long)(T * D), d_total, st));
    return TA_OK;
}

int coll_args(ta_ctx* ctx, const Collective& q, int fft, int S, const void* species, const void* sums) {
    TA_CHECK(check_fft(ctx, fft));
    TA_CHECK(check_species_count(fail, ctx, S));
    if (!species) return fail(ctx, TA_E_INVALID, "species labels are NULL");
    if (!sums) return fail(ctx, TA_E_INVALID, std::string(q.noun) + " output is NULL");
    return TA_OK;
}

// ---- species-resolved self terms (species_self.hip) ------------------------------------------------------------------
int self_args(ta_ctx* ctx, int quantity, int fft, int S, const void* species, const void* out) {
    if (quantity != TA_SELF_MSD && quantity != TA_SELF_VACF)
        return fail(ctx, TA_E_INVALID, "quantity must be TA_SELF_MSD (0) or TA_SELF_VACF (1)");
    TA_CHECK(check_fft(ctx, fft));
    TA_CHECK(check_species_count(fail, ctx, S));
    if (!species) return fail(ctx, TA_E_INVALID, "species labels are NULL");
    if (!out) return fail(ctx, TA_E_INVALID, "self output is NULL");
    return TA_OK;
}

// The host half of one call: the labels checked, the blocks laid out, the sorted order (one int32 per atom) queued for
// upload on `st`.  Nothing on the device has been written when this fails.
int self_plan(ta_ctx* ctx, int S, const int32_t* h_species, int64_t A, int D, hipStream_t st, SortPlan* plan) {
    TA_CHECK(check_cols(ctx, "species self terms: ", A, D));
    TA_CHECK(check_labels(fail, ctx, h_species, A, S));
    void* order = nullptr;
    TA_CHECK(ctx->self_order.begin(ctx, sizeof(int32_t) * (size_t)A, &order));
    species_sort_plan(h_species, A, D, S, plan, (int32_t*)order);
    return ctx->self_order.send(ctx, st);
}

// One self-term call on a pair-major slab of either element type, read as it is (the caller has opened the call's
// bracket, it is closed here): the sort pass writes W = w (x - shift x[0]) with each species' atoms contiguous, then
// every species with atoms gets ONE lag-sum evaluation on its block -- a pair-major slab of its own with N_s atoms -- by
// the dispatch ta_msd_staged / ta_vacf_fft_staged / ta_vacf_direct_staged use, into d_self + s T.  A species without
// atoms: exact zeros, no call.  ev[1] / ev[2] bracket the pass, unless an evaluation after it records its own kernel.
int species_self_pm(ta_ctx* ctx, int quantity, bool fft, const Slab& slab, const SortPlan& plan, const double* d_w,
                    double* d_self) {
    const int64_t pitch = slab.pitch, T = slab.T;
    const int D = slab.D;
    hipStream_t st = slab.st;
    TA_CHECK(ensure(ctx, ctx->self_w, (size_t)plan.n_pairs * (size_t)pitch * 16));
    double* W = (double*)ctx->self_w.p;
    TA_LAUNCH_MAIN(ctx, "k_species_sort", st,
                   launch_species_sort(ctx->n_cu, slab.pm, slab.f32, (long)pitch, (long)T, (long)(slab.A * D), D, plan,
                                       (const int*)ctx->self_order.dev.p, d_w, quantity == TA_SELF_MSD, W, st));
    for (int s = 0; s < plan.n_species; ++s) {
        double* out = d_self + (size_t)s * T;
        const int64_t n = plan.count[s];
        if (n == 0) {
            TA_HIP_TRY(ctx, hipMemsetAsync(out, 0, sizeof(double) * (size_t)T, st));
            continue;
        }
        const double* blk = W + (size_t)plan.pair0[s] * (size_t)pitch * 2;
        TA_CHECK((quantity == TA_SELF_MSD ? msd_impl : acf_impl)(ctx, fft, blk, pitch, T, n, D, out, nullptr, 0, st));
    }
    return call_end(ctx, st);
}

// ---- intermediate scattering functions (scatter.hip) -----------------------------------------------------------------
// The scratch budget of the phase slab: a chunk holds as many wavevectors as fit (at least one).  A choice, not a
// measurement: two wavevectors of the headline shape (10000 x 100000: 16 GB each) next to its 24 GB slab and the FFT
// workspaces on a 288 GB device.
constexpr size_t kScatterBudget = (size_t)32 << 30;

int scatter_args(ta_ctx* ctx, int fft, int n_k, const double* h_kvecs, int D, const void* o_self, const void* o_density,
                 const void* o_coll) {
    return check_kvecs(fail, ctx, fft, n_k, h_kvecs, D, o_self || o_density || o_coll);
}

// bytes of scatter_work for K wavevectors of T frames: the pair-major densities, their (T, K) by-particle lag sums and the
// lag sum, then (own_density) the densities themselves
size_t scatter_work_bytes(int64_t T, int K, bool own_density) {
    return pm_bytes(T, 2 * (int64_t)K) + sizeof(double) * ((size_t)T * K + (size_t)T + (own_density ? (size_t)K * T * 2 : 0));
}
double* scatter_own_density(ta_ctx* ctx, int64_t T, int K) {
    return (double*)((char*)ctx->scatter_work.p + pm_bytes(T, 2 * (int64_t)K)) + (size_t)T * K + (size_t)T;
}

// The host half of one call, before it is opened: the wavevectors in turns (q = k / 2 pi) queued for upload on `st`, the
// buffers that do not depend on the chunking.  Nothing on the device has been written when this fails.
int scatter_plan(ta_ctx* ctx, int K, const double* h_kvecs, int64_t A, int D, hipStream_t st) {
    TA_CHECK(check_cols(ctx, "scatter: ", A, std::max(D, 2), "max(dim, 2)"));
    void* q = nullptr;
    TA_CHECK(ctx->scatter_q.begin(ctx, sizeof(double) * (size_t)K * D, &q));
    TA_CHECK(ensure(ctx, ctx->scatter_lab, sizeof(int32_t) * (size_t)A));
    for (size_t i = 0; i < (size_t)K * D; ++i) ((double*)q)[i] = phase_turns(h_kvecs[i]);
    return ctx->scatter_q.send(ctx, st);
}

// coll (K, T) of the densities (K, T, 2) at d_density: their pair-major copy is a slab of K "atoms" with D = 2
// (k_relayout, one wavevector at a time: a density is a frame-major (T, 2) array), ONE by-particle autocorrelation of it
// by the VACF's dispatch, then the (T, K) -> (K, T) transposition.  scatter_work is ensured by the caller.
int scatter_collective(ta_ctx* ctx, bool fft, const double* d_density, int K, int64_t T, double* d_coll, hipStream_t st) {
    const int64_t pitch = pm_pitch(T);
    double* pm = (double*)ctx->scatter_work.p;
    double* bp = (double*)((char*)pm + pm_bytes(T, 2 * (int64_t)K));
    double* lagsum = bp + (size_t)T * K;
    if (pitch > T)  // rows T ... pitch - 1 as zeros, like every block of Z: the workspace is reused
        TA_HIP_TRY(ctx, hipMemsetAsync(pm, 0, pm_bytes(T, 2 * (int64_t)K), st));
    for (int j = 0; j < K; ++j)
        TA_LAUNCH(ctx, "k_relayout", st,
                  launch_relayout(d_density + (size_t)j * T * 2, false, 2, 2, (long)T, pm + (size_t)j * pitch * 2, false, (long)pitch, 0, st));
    TA_CHECK(acf_impl(ctx, fft, pm, pitch, T, K, 2, lagsum, bp, K, st));
    TA_LAUNCH(ctx, "k_scatter_transpose", st, launch_scatter_transpose(bp, (long)T, K, d_coll, st));
    return TA_OK;
}

// One scattering call on a pair-major position slab of either element type, read as it is (the caller has opened the
// call's bracket, it is closed here; scatter_plan has queued the wavevectors).  Per chunk of Kc wavevectors: the phase
// pass writes Z; then per wavevector its block of A pairs -- a pair-major slab of A atoms with D = 2 of its own -- gets
// ONE VACF lag-sum evaluation (d_self + j T) and ONE species-sum pass without shift, one species, no weights, with the
// fixed-order sum of its partials (the density, (T, 2) at j).  After the last chunk the collective part of the K densities.
// Nothing depends on Kc but which launches share a pass: the same bits for every chunk size.  ev[1] / ev[2] bracket the
// (last) pass, unless an evaluation after it records its own kernel.
int scatter_pm(ta_ctx* ctx, bool fft, const Slab& slab, int K, double* d_self, double* d_density, double* d_coll) {
    const int64_t pitch = slab.pitch, T = slab.T, A = slab.A;
    const int D = slab.D;
    hipStream_t st = slab.st;
    const size_t per = (size_t)A * (size_t)pitch * 16;  // Z of one wavevector
    const int64_t Kc = ctx->opt_scatter_chunk > 0 ? std::min<int64_t>(ctx->opt_scatter_chunk, K)
                                                   : std::max<int64_t>(1, std::min<int64_t>(K, (int64_t)(kScatterBudget / per)));
    TA_CHECK(ensure(ctx, ctx->scatter_z, (size_t)Kc * per));
    double* Z = (double*)ctx->scatter_z.p;
    const bool sums = d_density || d_coll;
    if (d_coll) TA_CHECK(ensure(ctx, ctx->scatter_work, scatter_work_bytes(T, K, !d_density)));
    double* rho = d_density ? d_density : d_coll ? scatter_own_density(ctx, T, K) : nullptr;
    const int n_parts = species_sum_parts(ctx->n_cu, 1, (long)T, (long)(2 * A));
    if (sums) {
        TA_CHECK(ensure(ctx, ctx->ons_part, sizeof(double) * (size_t)n_parts * T * 2));
        TA_HIP_TRY(ctx, hipMemsetAsync(ctx->scatter_lab.p, 0, sizeof(int32_t) * (size_t)A, st));
    }
    const double* d_q = (const double*)ctx->scatter_q.dev.p;
    for (int64_t j0 = 0; j0 < K; j0 += Kc) {
        const int kc = (int)std::min<int64_t>(Kc, K - j0);
        TA_LAUNCH_MAIN(ctx, "k_phase", st,
                       launch_phase(ctx->n_cu, slab.pm, slab.f32, (long)pitch, (long)T, (long)A, D, d_q + j0 * D, kc, Z, st));
        for (int jl = 0; jl < kc; ++jl) {
            const double* blk = Z + (size_t)jl * A * pitch * 2;
            const int64_t j = j0 + jl;
            if (d_self) TA_CHECK(acf_impl(ctx, fft, blk, pitch, T, A, 2, d_self + (size_t)j * T, nullptr, 0, st));
            if (!sums) continue;
            TA_CHECK(weighted_total(ctx, blk, false, pitch, T, A, 2, (const int*)ctx->scatter_lab.p, nullptr, n_parts,
                                    rho + (size_t)j * T * 2, st));
        }
    }
    if (d_coll) TA_CHECK(scatter_collective(ctx, fft, rho, K, T, d_coll, st));
    return call_end(ctx, st);
}

// ---- orientational correlation functions (orient.hip) ---------------------------------------------------------------
// The caller's arguments of ta_orient*, as they came (outputs: which of c1, c2, total, coll are asked for)
struct OrientArgs {
    int fft, mode;
    int64_t N;
    const int32_t* h_index;
    const double *h_dims, *h_w;
    bool c1, c2, total, coll;
};

// Every check of ta_orient* (both kinds of context), all of them before anything is written; T, A, D: the shape of slab 0
// (D 0: nothing staged).  With h_dims the box table (unwrap_box.hpp; per-frame rows padded to the pitch) is left in *box.
int orient_check(ta_ctx* ctx, const OrientArgs& a, int64_t T, int64_t A, int D, BoxTable* box) {
    const std::string p = "orient: ";
    if (a.mode < ORIENT_BOND || a.mode > ORIENT_NORMAL)
        return fail(ctx, TA_E_INVALID, p + "mode must be TA_ORIENT_BOND (0), TA_ORIENT_BISECTOR (1) or TA_ORIENT_NORMAL (2)");
    TA_CHECK(check_fft(ctx, a.fft));
    if (!(a.c1 || a.c2 || a.total || a.coll)) return fail(ctx, TA_E_INVALID, p + "the c1, c2, total and collective outputs are all NULL");
    if (D == 0) return fail(ctx, TA_E_INVALID, p + "no position slab is staged");
    if (D != 3) return fail(ctx, TA_E_INVALID, p + "the position slab must hold three columns per atom (dim = " + std::to_string(D) + ")");
    if (a.N < 1) return fail(ctx, TA_E_INVALID, p + "n_vectors must be >= 1");
    if (!a.h_index) return fail(ctx, TA_E_INVALID, p + "the index table is NULL");
    if (A * 3 >= (int64_t)1 << 31 || a.N * 6 >= (int64_t)1 << 31)
        return fail(ctx, TA_E_INVALID, p + "n_atoms * 3 and n_vectors * 6 must be below 2^31");
    const int K = orient_row_len(a.mode);
    for (int64_t n = 0; n < a.N; ++n) {
        const int32_t* r = a.h_index + n * K;
        for (int j = 0; j < K; ++j)
            if (r[j] < 0 || r[j] >= A)
                return fail(ctx, TA_E_INVALID, p + "index " + std::to_string(r[j]) + " of vector " + std::to_string(n) +
                                                   " is outside 0 ... n_atoms - 1");
        if (r[0] == r[1] || (K == 3 && (r[0] == r[2] || r[1] == r[2])))
            return fail(ctx, TA_E_INVALID, p + "vector " + std::to_string(n) + " names an atom twice");
    }
    for (int64_t n = 0; a.h_w && n < a.N; ++n)
        if (!(a.h_w[n] - a.h_w[n] == 0.0)) return fail(ctx, TA_E_INVALID, p + "weight " + std::to_string(n) + " is not finite");
    if (a.h_dims) {
        const int axes[3] = {0, 1, 2};
        const std::string why = box_table(a.h_dims, T, 3, axes, 8, box);
        if (!why.empty()) return fail(ctx, TA_E_INVALID, p + why);
    }
    return TA_OK;
}

// The nine rows of orient_math.hpp's box (H's six entries, M's diagonal) of unwrap_box.hpp's table, tpitch doubles each
void orient_box_rows(const BoxTable& box, double* out) {
    static const int rows[kOrientBoxRows] = {0, 1, 2, 3, 4, 5, 6 + diag_row(0), 6 + diag_row(1), 6 + diag_row(2)};
    for (int r = 0; r < kOrientBoxRows; ++r)
        memcpy(out + (size_t)r * box.tpitch, box.tab.data() + (size_t)rows[r] * box.tpitch, sizeof(double) * (size_t)box.tpitch);
}

// The table of a call on the device: box rows | weights | index rows (int32) | N zero labels (int32: the one species of the sum)
struct OrientTab {
    const double *box, *w;
    long tpitch;
    const int *index, *lab;
};
struct OrientPlan {
    int mode = 0;
    int64_t N = 0, tpitch = 0;  // tpitch 0: no box
    bool weights = false;
    size_t n_box() const { return (size_t)kOrientBoxRows * (size_t)tpitch; }
    size_t n_index() const { return ((size_t)N * orient_row_len(mode) + 1) / 2; }  // in doubles
};
// The host half of one call, before it is opened: the table queued for upload on `st`.  Nothing on the device has been
// written when this fails.
int orient_plan(ta_ctx* ctx, const OrientArgs& a, const BoxTable& box, hipStream_t st, OrientPlan* p) {
    p->mode = a.mode, p->N = a.N, p->tpitch = a.h_dims ? box.tpitch : 0, p->weights = a.h_w != nullptr;
    const size_t n = p->n_box() + (p->weights ? (size_t)a.N : 0) + p->n_index() + ((size_t)a.N + 1) / 2;
    double* h = nullptr;
    TA_CHECK(ctx->orient_tab.begin(ctx, sizeof(double) * n, (void**)&h));
    memset(h, 0, sizeof(double) * n);
    if (a.h_dims) orient_box_rows(box, h);
    h += p->n_box();
    if (a.h_w) memcpy(h, a.h_w, sizeof(double) * (size_t)a.N), h += a.N;
    memcpy(h, a.h_index, sizeof(int32_t) * (size_t)a.N * orient_row_len(a.mode));
    return ctx->orient_tab.send(ctx, st);
}
OrientTab orient_tab(ta_ctx* ctx, const OrientPlan& p) {
    const double* d = (const double*)ctx->orient_tab.dev.p;
    const double* w = d + p.n_box();
    const double* idx = w + (p.weights ? (size_t)p.N : 0);
    return {p.tpitch ? d : nullptr, p.weights ? w : nullptr, (long)p.tpitch, (const int*)idx, (const int*)(idx + p.n_index())};
}

// One orientation call on a pair-major position slab of either element type, read as it is (the caller has opened the
// call's bracket, it is closed here; orient_plan has queued the table).  Rank 1, when c1, total or coll is asked for: the
// pass writes the block of N atoms u into Z, ONE VACF lag-sum evaluation of it is c1, ONE species-sum pass (one species,
// the weights) with the fixed-order sum of its partials the total (T, 3).  Rank 2, when c2 is asked for: the pass writes
// the 2 N pseudo-atoms of Q into the SAME scratch, ONE evaluation is c2.  coll: the pair-major copy of the total as one
// atom with D = 3, ONE evaluation.  The call does not chunk (a lag sum split over vectors would change its bits): Z is
// 3 N pitch 16 bytes or TA_E_NOMEM.  ev[1] / ev[2] bracket the (last) pass, unless an evaluation after it records its own.
int orient_pm(ta_ctx* ctx, bool fft, const Slab& slab, const OrientPlan& p, double* d_c1, double* d_c2, double* d_total,
              double* d_coll) {
    const int64_t pitch = slab.pitch, T = slab.T, N = p.N;
    hipStream_t st = slab.st;
    TA_CHECK(ensure(ctx, ctx->orient_z, (size_t)3 * (size_t)N * (size_t)pitch * 16));
    double* Z = (double*)ctx->orient_z.p;
    const OrientTab tab = orient_tab(ctx, p);
    double* tot = d_total;
    if (d_coll) {
        TA_CHECK(ensure(ctx, ctx->orient_work, pm_bytes(T, 3) + (d_total ? 0 : sizeof(double) * (size_t)T * 3)));
        if (!tot) tot = (double*)((char*)ctx->orient_work.p + pm_bytes(T, 3));
    }
    const int n_parts = species_sum_parts(ctx->n_cu, 1, (long)T, (long)(3 * N));
    if (tot) TA_CHECK(ensure(ctx, ctx->ons_part, sizeof(double) * (size_t)n_parts * T * 3));
    auto pass = [&](int rank) -> int {
        TA_LAUNCH_MAIN(ctx, "k_orient", st,
                       launch_orient(ctx->n_cu, slab.pm, slab.f32, (long)pitch, (long)T, (long)slab.A, slab.D, p.mode, rank, (long)N,
                                     tab.index, tab.box, tab.tpitch, Z, st));
        return TA_OK;
    };
    if (d_c1 || tot) {
        TA_CHECK(pass(1));
        if (d_c1) TA_CHECK(acf_impl(ctx, fft, Z, pitch, T, N, 3, d_c1, nullptr, 0, st));
        if (tot) TA_CHECK(weighted_total(ctx, Z, false, pitch, T, N, 3, tab.lab, tab.w, n_parts, tot, st));
    }
    if (d_c2) {
        TA_CHECK(pass(2));
        TA_CHECK(acf_impl(ctx, fft, Z, pitch, T, 2 * N, 3, d_c2, nullptr, 0, st));
    }
    if (d_coll) {  // (the phantom column and the rows T ... pitch - 1 as zeros: the workspace is reused)
        TA_HIP_TRY(ctx, hipMemsetAsync(ctx->orient_work.p, 0, pm_bytes(T, 3), st));
        TA_LAUNCH(ctx, "k_relayout", st, launch_relayout(tot, false, 3, 3, (long)T, ctx->orient_work.p, false, (long)pitch, 0, st));
        TA_CHECK(acf_impl(ctx, fft, (const double*)ctx->orient_work.p, pitch, T, 1, 3, d_coll, nullptr, 0, st));
    }
    return call_end(ctx, st);
}

// ta_orient_dev / ta_orient_staged (dev NULL) and the device half of ta_orient (out != NULL: the context's own output
// buffer, laid out by orient_out, takes the place of the d_* pointers, which then only say what is asked for)
int orient_entry(ta_ctx* ctx, const DevSrc* dev, int fft, int mode, int64_t N, const int32_t* h_index, const double* h_dims,
                 const double* h_w, double* d_c1, double* d_c2, double* d_total, double* d_coll, void* stream, double** out) {
    const OrientArgs a{fft, mode, N, h_index, h_dims, h_w, d_c1 != nullptr, d_c2 != nullptr, d_total != nullptr, d_coll != nullptr};
    BoxTable box;
    OrientPlan plan;
    return slab_entry(
        ctx, dev, stream,
        [&] {
            return dev ? orient_check(ctx, a, dev->T, dev->A, dev->D, &box)
                       : orient_check(ctx, a, ctx->st_T, ctx->st_A, ctx->st_nslabs ? ctx->st_D : 0, &box);
        },
        [&](const Slab& s) -> int {
            TA_CHECK(orient_plan(ctx, a, box, s.st, &plan));
            if (out) TA_CHECK(out_buffer(ctx, ctx->orient_out, orient_out(s.T), out));
            return TA_OK;
        },
        [&](const Slab& s) {
            if (!out) return orient_pm(ctx, fft != 0, s, plan, d_c1, d_c2, d_total, d_coll);
            const OutLayout o = orient_out(s.T);
            return orient_pm(ctx, fft != 0, s, plan, o.at(*out, 0, a.c1), o.at(*out, 1, a.c2), o.at(*out, 2, a.total), o.at(*out, 3, a.coll));
        });
}

// ---- chain normal modes (chain_modes.hip) ---------------------------------------------------------------------------
// The budget of the blocks of one batch of functionals (3 n_chains pitch 8 bytes each): a choice, not a measurement.  It
// bounds memory and nothing else: a functional's lag sum does not depend on its neighbours in the batch.
constexpr size_t kChainBudget = (size_t)2 << 30;

// The caller's arguments of ta_chain_modes*, as they came
struct ChainArgs {
    int fft;
    int64_t C, N;  // chains, beads per chain
    const int32_t* h_members;
    int Q;
    const double *h_coeff, *h_dims;
    const void* out;
};

// Every check of ta_chain_modes* (both kinds of context), all of them before anything is written.  With h_dims the box table
// (unwrap_box.hpp; per-frame rows padded to the pitch) is left in *box.
int chain_check(ta_ctx* ctx, const ChainArgs& a, BoxTable* box) {
    const std::string p = "chain_modes: ";
    TA_CHECK(check_fft(ctx, a.fft));
    if (a.C < 1) return fail(ctx, TA_E_INVALID, p + "n_chains must be >= 1");
    if (a.N < 2) return fail(ctx, TA_E_INVALID, p + "chain_len must be >= 2");
    if (a.Q < 1) return fail(ctx, TA_E_INVALID, p + "n_modes must be >= 1");
    if (!a.h_members) return fail(ctx, TA_E_INVALID, p + "the member table is NULL");
    if (!a.h_coeff) return fail(ctx, TA_E_INVALID, p + "the coefficient matrix is NULL");
    if (!a.out) return fail(ctx, TA_E_INVALID, p + "the acf output is NULL");
    TA_CHECK(check_staged(ctx));
    const int64_t T = ctx->st_T, A = ctx->st_A;
    if (ctx->st_D != 3)
        return fail(ctx, TA_E_INVALID, p + "the position slab must hold three columns per atom (dim = " + std::to_string(ctx->st_D) + ")");
    if (A * 3 >= (int64_t)1 << 31 || a.N >= (int64_t)1 << 31 || a.C >= (int64_t)1 << 31 || (int64_t)a.Q * a.C * 3 >= (int64_t)1 << 31)
        return fail(ctx, TA_E_INVALID, p + "n_atoms * 3 and n_modes * n_chains * 3 must be below 2^31");
    std::vector<int32_t> row((size_t)a.N);
    for (int64_t c = 0; c < a.C; ++c) {
        const int32_t* r = a.h_members + c * a.N;
        for (int64_t n = 0; n < a.N; ++n)
            if (r[n] < 0 || r[n] >= A)
                return fail(ctx, TA_E_INVALID, p + "member " + std::to_string(r[n]) + " of chain " + std::to_string(c) +
                                                   " is outside 0 ... n_atoms - 1");
        row.assign(r, r + a.N);
        std::sort(row.begin(), row.end());
        if (std::adjacent_find(row.begin(), row.end()) != row.end())
            return fail(ctx, TA_E_INVALID, p + "chain " + std::to_string(c) + " names an atom twice");
    }
    for (int64_t i = 0; i < (int64_t)a.Q * a.N; ++i)
        if (!(a.h_coeff[i] - a.h_coeff[i] == 0.0))
            return fail(ctx, TA_E_INVALID, p + "coefficient " + std::to_string(i % a.N) + " of mode " + std::to_string(i / a.N) + " is not finite");
    if (a.h_dims) {
        const int axes[3] = {0, 1, 2};
        const std::string why = box_table(a.h_dims, T, 3, axes, 8, box);
        if (!why.empty()) return fail(ctx, TA_E_INVALID, p + why);
    }
    return TA_OK;
}

// The host half of one call, before it is opened: the table -- box rows (orient_box_rows) | coefficients (Q, N) | members
// (C, N) int32 -- queued for upload on `st`.  Nothing on the device has been written when this fails.
struct ChainPlan {
    int64_t C = 0, N = 0, tpitch = 0;  // tpitch 0: no box
    int Q = 0;
    size_t n_box() const { return (size_t)kOrientBoxRows * (size_t)tpitch; }
};
int chain_plan(ta_ctx* ctx, const ChainArgs& a, const BoxTable& box, hipStream_t st, ChainPlan* p) {
    p->C = a.C, p->N = a.N, p->Q = a.Q, p->tpitch = a.h_dims ? box.tpitch : 0;
    const size_t n_coeff = (size_t)a.Q * (size_t)a.N, n_member = (size_t)a.C * (size_t)a.N;
    const size_t n = p->n_box() + n_coeff + (n_member + 1) / 2;
    double* h = nullptr;
    TA_CHECK(ctx->chain_tab.begin(ctx, sizeof(double) * n, (void**)&h));
    memset(h, 0, sizeof(double) * n);
    if (a.h_dims) orient_box_rows(box, h);
    h += p->n_box();
    memcpy(h, a.h_coeff, sizeof(double) * n_coeff);
    memcpy(h + n_coeff, a.h_members, sizeof(int32_t) * n_member);
    return ctx->chain_tab.send(ctx, st);
}

// One call on the pair-major position slab of either element type, read as it is (the caller has opened the call's bracket,
// it is closed here; chain_plan has queued the table).  Per batch of B functionals -- as many as keep their blocks under
// kChainBudget, at least one; "chain_modes_chunk" n: min(n, that count) -- ceil(B / tile modes) passes, each a read of the
// slab, write the batch's blocks, then ONE VACF lag-sum evaluation per functional on its block is its row of d_acf (Q, T).
// A functional's block and evaluation do not depend on the batch or the launch it was in: the same bits for every chunk.
// ev[1] / ev[2] bracket the (last) pass, unless an evaluation after it records its own.
int chain_pm(ta_ctx* ctx, bool fft, const Slab& slab, const ChainPlan& p, double* d_acf) {
    const int64_t pitch = slab.pitch, T = slab.T;
    hipStream_t st = slab.st;
    int MC = 1, F = 2;
    chain_modes_tile(&MC, &F);
    const size_t block = (size_t)((3 * p.C + 1) / 2) * (size_t)pitch * 2;  // doubles per functional
    const int fit = (int)std::max<size_t>(1, std::min<size_t>((size_t)p.Q, kChainBudget / (block * sizeof(double))));
    const int B = ctx->opt_chain_modes_chunk > 0 ? (int)std::min<int64_t>(ctx->opt_chain_modes_chunk, fit) : fit;
    TA_CHECK(ensure(ctx, ctx->chain_z, block * sizeof(double) * (size_t)B));
    double* Z = (double*)ctx->chain_z.p;
    const double* tab = (const double*)ctx->chain_tab.dev.p;
    const double* box = p.tpitch ? tab : nullptr;
    const double* coeff = tab + p.n_box();
    const int* member = (const int*)(coeff + (size_t)p.Q * (size_t)p.N);
    for (int q0 = 0; q0 < p.Q; q0 += B) {
        const int nb = std::min(B, p.Q - q0);
        for (int l0 = 0; l0 < nb; l0 += MC)
            TA_LAUNCH_MAIN(ctx, "k_chain_modes", st,
                           launch_chain_modes(ctx->n_cu, slab.pm, slab.f32, (long)pitch, (long)T, (long)slab.A, slab.D, (long)p.C, (int)p.N,
                                              member, coeff + (size_t)(q0 + l0) * (size_t)p.N, std::min(MC, nb - l0), box, (long)p.tpitch,
                                              Z + (size_t)l0 * block, st));
        for (int b = 0; b < nb; ++b)
            TA_CHECK(acf_impl(ctx, fft, Z + (size_t)b * block, pitch, T, p.C, 3, d_acf + (size_t)(q0 + b) * (size_t)T, nullptr, 0, st));
    }
    return call_end(ctx, st);
}

// ta_chain_modes_staged and the device half of ta_chain_modes (out != NULL: the context's own output buffer takes d_acf's place)
int chain_entry(ta_ctx* ctx, const ChainArgs& a, double* d_acf, void* stream, double** out) {
    BoxTable box;
    ChainPlan plan;
    return slab_entry(
        ctx, nullptr, stream, [&] { return chain_check(ctx, a, &box); },
        [&](const Slab& s) -> int {
            TA_CHECK(chain_plan(ctx, a, box, s.st, &plan));
            if (out) TA_CHECK(out_buffer(ctx, ctx->chain_out, chain_modes_out(a.Q, s.T), out));
            return TA_OK;
        },
        [&](const Slab& s) { return chain_pm(ctx, a.fft != 0, s, plan, out ? *out : d_acf); });
}

// ---- current correlation functions (kcurrent.hip) -------------------------------------------------------------------
// The budget of k_kcurrent's partial-sum buffer: G KC pitch D 16 bytes bound its atom groups G.  A choice, not a
// measurement: the headline shape (10000 x 100000 x 3) asks for ~100 groups = 0.2 GB next to its 48 GB of slabs; the cap
// bites only for trajectories of a million frames, where one group per frame block still has every atom to itself.
constexpr size_t kKcurBudget = (size_t)1 << 30;

// the family's argument checks (GPU and CPU contexts, one set of messages): both slabs staged and their columns ...
int kcurrent_slabs(ta_ctx* ctx) {
    TA_CHECK(check_staged(ctx, 2));
    return check_cols(ctx, "kcurrent: ", ctx->st_A, ctx->st_D);
}
// ... behind the wavevectors and outputs
int kcurrent_args(ta_ctx* ctx, int fft, int n_k, const double* h_kvecs, const void* o_current, const void* o_long,
                  const void* o_trans) {
    TA_CHECK(check_kcurrent(fail, ctx, fft, n_k, h_kvecs, ctx->st_nslabs ? ctx->st_D : 0, o_current || o_long || o_trans));
    return kcurrent_slabs(ctx);
}

// bytes of kcur_work for K wavevectors of T frames: the pair-major pseudo-atoms, their (T, K S) by-particle lag sums and the
// lag sum, then (own_current) the current itself
size_t kcurrent_work_bytes(int64_t T, int K, int D, bool own_current) {
    const size_t P = (size_t)K * kcur_series(D);
    return pm_bytes(T, 2 * (int64_t)P) + sizeof(double) * ((size_t)T * P + (size_t)T + (own_current ? (size_t)K * T * D * 2 : 0));
}

// The host half of one call, before it is opened: ONE table -- the wavevectors in turns (q = k / 2 pi), the unit vectors
// behind them, then a host-facing call's weights (n_w of them) -- queued for upload on `st`.  Nothing on the device has
// been written when this fails.
int kcurrent_plan(ta_ctx* ctx, int K, const double* h_kvecs, int D, const double* h_w, int64_t n_w, hipStream_t st) {
    const size_t n = (size_t)K * D;
    void* h = nullptr;
    TA_CHECK(ctx->kcur_tab.begin(ctx, sizeof(double) * (2 * n + (h_w ? (size_t)n_w : 0)), &h));
    double* q = (double*)h;
    for (size_t i = 0; i < n; ++i) q[i] = phase_turns(h_kvecs[i]);
    for (int j = 0; j < K; ++j) kcur_khat(D, h_kvecs + (size_t)j * D, q + n + (size_t)j * D);
    if (h_w) memcpy(q + 2 * n, h_w, sizeof(double) * (size_t)n_w);
    return ctx->kcur_tab.send(ctx, st);
}

// long (K, T) and trans (K, T) of the current (K, T, D, 2) at d_current (either output may be NULL): the projections jL, jT_d
// as a pair-major slab of K S pseudo-atoms with D = 2 (S = 1 + D; D = 1: 1), ONE by-particle autocorrelation of it by the
// VACF's dispatch, then the pass that transposes, adds the D transverse series and divides by D - 1.  kcur_work is ensured by
// the caller, the unit vectors are in kcur_tab (kcurrent_plan).
int kcurrent_correlation(ta_ctx* ctx, bool fft, const double* d_current, int K, int64_t T, int D, double* d_long, double* d_trans,
                         hipStream_t st) {
    const int64_t pitch = pm_pitch(T), P = (int64_t)K * kcur_series(D);
    double* pm = (double*)ctx->kcur_work.p;
    double* bp = (double*)((char*)pm + pm_bytes(T, 2 * P));
    double* lagsum = bp + (size_t)T * P;
    const double* khat = (const double*)ctx->kcur_tab.dev.p + (size_t)K * D;
    TA_LAUNCH(ctx, "k_kcurrent_project", st, launch_kcurrent_project(d_current, khat, K, (long)T, D, (long)pitch, pm, st));
    TA_CHECK(acf_impl(ctx, fft, pm, pitch, T, P, 2, lagsum, bp, P, st));
    TA_LAUNCH(ctx, "k_kcurrent_finish", st, launch_kcurrent_finish(bp, K, (long)T, D, d_long, d_trans, st));
    return TA_OK;
}

// One call on the two pair-major slabs of either element type (slab 0 = velocities, slab 1 = positions), read as they are
// (the caller has opened the call's bracket, it is closed here; kcurrent_plan has queued the table).  Per chunk of at most
// KC wavevectors (the kernel's tile; "kcurrent_chunk" n: min(n, KC)) ONE fused pass and the fixed-order sum of its partials
// into the current; after the last chunk the correlations.  The atom groups depend on the slab and the device only: the
// same bits for every chunk size.  ev[1] / ev[2] bracket the (last) pass, unless an evaluation after it records its own.
int kcurrent_pm(ta_ctx* ctx, bool fft, const Slab& s, int K, const double* d_w, double* d_current, double* d_long, double* d_trans) {
    const int64_t pitch = s.pitch, T = s.T, A = s.A;
    const int D = s.D;
    hipStream_t st = s.st;
    int KC = 1, f64 = 1, f32 = 2;
    kcurrent_tile(&KC, &f64, &f32);
    const int Kc = ctx->opt_kcurrent_chunk > 0 ? (int)std::min<int64_t>(ctx->opt_kcurrent_chunk, KC) : KC;
    const bool corr = d_long || d_trans;
    const int G = kcurrent_parts(ctx->n_cu, s.f32, (long)pitch, (long)A, D, kKcurBudget);
    TA_CHECK(ensure(ctx, ctx->kcur_part, (size_t)G * KC * (size_t)T * D * 16));
    if (corr) TA_CHECK(ensure(ctx, ctx->kcur_work, kcurrent_work_bytes(T, K, D, !d_current)));
    double* part = (double*)ctx->kcur_part.p;
    double* cur = d_current ? d_current
                            : (double*)((char*)ctx->kcur_work.p + kcurrent_work_bytes(T, K, D, false));  // (then corr: kcurrent_args)
    const double* d_q = (const double*)ctx->kcur_tab.dev.p;
    const size_t per = (size_t)T * D * 2;  // doubles of one wavevector's current
    for (int j0 = 0; j0 < K; j0 += Kc) {
        const int kc = std::min(Kc, K - j0);
        TA_LAUNCH_MAIN(ctx, "k_kcurrent", st,
                       launch_kcurrent(s.pm, s.pm1, s.f32, (long)pitch, (long)T, (long)A, D, d_q + (size_t)j0 * D, kc, d_w, part, G, st));
        TA_LAUNCH(ctx, "k_sum_partials", st, launch_sum_partials(part, G, (long)(kc * per), cur + j0 * per, st));
    }
    if (corr) TA_CHECK(kcurrent_correlation(ctx, fft, cur, K, T, D, d_long, d_trans, st));
    return call_end(ctx, st);
}

// ---- partial scattering functions (species_density.hip) --------------------------------------------------------------
// The budget of k_species_density's partial-sum buffer, G (ST KC <= 16) pitch 16 bytes, as kKcurBudget; and of the cross
// term's workspaces (the pseudo-particles and their by-particle lag sums of one chunk of wavevectors): choices, not
// measurements.  At 10000 frames and 8 species a wavevector's share of the latter is 15 MB: the cap bites above ~70.
constexpr size_t kPartialBudget = (size_t)1 << 30;
constexpr size_t kPartialCrossBudget = (size_t)1 << 30;

// the family's argument checks (GPU and CPU contexts, one set of messages), in the order of ta_scatter and ta_onsager; D:
// the components per wavevector (0: not known, nothing staged -- reported after these)
int partial_args(ta_ctx* ctx, int fft, int n_k, const double* h_kvecs, int D, int S, const void* species, const void* o_density) {
    return check_partial(fail, ctx, fft, n_k, h_kvecs, D, S, species, o_density);
}
// ... and, behind them, the staged slab and its columns
int partial_slab(ta_ctx* ctx) {
    TA_CHECK(check_staged(ctx));
    return check_cols(ctx, "partial density: ", ctx->st_A, ctx->st_D);
}

// The host half of one call, before it is opened: ONE table -- the wavevectors in turns (q = k / 2 pi), then a host-facing
// call's weights (n_w of them) -- queued for upload on `st`.  Nothing on the device has been written when this fails.
int partial_plan(ta_ctx* ctx, int K, const double* h_kvecs, int D, const double* h_w, int64_t n_w, hipStream_t st) {
    const size_t n = (size_t)K * D;
    void* h = nullptr;
    TA_CHECK(ctx->psd_tab.begin(ctx, sizeof(double) * (n + (h_w ? (size_t)n_w : 0)), &h));
    double* q = (double*)h;
    for (size_t i = 0; i < n; ++i) q[i] = phase_turns(h_kvecs[i]);
    if (h_w) memcpy(q + n, h_w, sizeof(double) * (size_t)n_w);
    return ctx->psd_tab.send(ctx, st);
}

// cross (K, T, S, S) of the densities (K, S, T, 2) at d_density: a complex density is a species sum with dim 2, so wavevector
// j's block is the (S, T, 2) sums coll_cross takes, and its S^2 pseudo-particles rho_a, rho_a + rho_b, rho_a - rho_b are S^2
// whole pairs.  Per chunk of Kx wavevectors -- as many as keep the Onsager workspaces under kPartialCrossBudget, which bounds
// memory and nothing else: a particle's autocorrelation does not depend on its neighbours; "partial_cross_chunk" n: min(n,
// that count) -- k_onsager_combos per wavevector, ONE by-particle evaluation of the chunk's Kx S^2 particles by the VACF's
// dispatch, and the finish.
int partial_cross(ta_ctx* ctx, bool fft, const double* d_density, int K, int S, int64_t T, double* d_cross, hipStream_t st) {
    const int64_t P1 = (int64_t)S * S, pitch = pm_pitch(T);
    const size_t per_k = pm_bytes(T, 2 * P1) + sizeof(double) * (size_t)(T * P1);
    const int Kfit = (int)std::max<size_t>(1, std::min<size_t>((size_t)K, kPartialCrossBudget / per_k));
    const int Kx = ctx->opt_partial_cross_chunk > 0 ? (int)std::min<int64_t>(ctx->opt_partial_cross_chunk, Kfit) : Kfit;
    TA_CHECK(ensure(ctx, ctx->ons_pm, pm_bytes(T, 2 * P1 * Kx)));
    TA_CHECK(ensure(ctx, ctx->ons_bp, sizeof(double) * (size_t)(T * P1 * Kx + T) + sizeof(int) * TA_ONSAGER_MAX_SPECIES * (size_t)Kx));
    double* pm = (double*)ctx->ons_pm.p;
    double* bp = (double*)ctx->ons_bp.p;
    double* lagsum = bp + T * P1 * Kx;
    int* nz = (int*)(lagsum + T);
    for (int j0 = 0; j0 < K; j0 += Kx) {
        const int kx = std::min(Kx, K - j0);
        TA_HIP_TRY(ctx, hipMemsetAsync(nz, 0, sizeof(int) * TA_ONSAGER_MAX_SPECIES * (size_t)kx, st));
        for (int b = 0; b < kx; ++b)
            TA_LAUNCH(ctx, "k_onsager_combos", st,
                      launch_onsager_combos(d_density + (size_t)(j0 + b) * S * T * 2, S, (long)T, 2, (long)pitch,
                                            pm + (size_t)b * P1 * pitch * 2, nz + b * TA_ONSAGER_MAX_SPECIES, st));
        TA_CHECK(acf_impl(ctx, fft, pm, pitch, T, P1 * kx, 2, lagsum, bp, P1 * kx, st));
        TA_LAUNCH(ctx, "k_partial_finish", st, launch_partial_finish(bp, kx, S, (long)T, nz, d_cross + (size_t)j0 * T * P1, st));
    }
    return TA_OK;
}

// One call on the pair-major position slab of either element type, read as it is (the caller has opened the call's bracket,
// it is closed here; partial_plan has queued the table).  Per chunk of at most KC wavevectors (the tile of the call's species
// count; "partial_chunk" n: min(n, KC)) ONE pass and the fixed-order sum of its partials into the density (K, S, T, 2); after
// the last chunk the cross term.  The atom groups depend on the slab and the device only: the same bits for every chunk
// size.  ev[1] / ev[2] bracket the (last) pass, unless an evaluation after it records its own.
int partial_pm(ta_ctx* ctx, bool fft, const Slab& s, int K, int S, const int32_t* d_species, const double* d_w, double* d_density,
               double* d_cross) {
    const int64_t pitch = s.pitch, T = s.T, A = s.A;
    hipStream_t st = s.st;
    int ST = 1, KC = 1, f64 = 1, f32 = 2;
    species_density_tile(S, &ST, &KC, &f64, &f32);
    const int Kc = ctx->opt_partial_chunk > 0 ? (int)std::min<int64_t>(ctx->opt_partial_chunk, KC) : KC;
    const int G = species_density_parts(ctx->n_cu, s.f32, (long)pitch, (long)A, kPartialBudget);
    TA_CHECK(ensure(ctx, ctx->psd_part, (size_t)G * KC * S * (size_t)T * 16));
    double* part = (double*)ctx->psd_part.p;
    const double* d_q = (const double*)ctx->psd_tab.dev.p;
    const size_t per = (size_t)S * T * 2;  // doubles of one wavevector's density
    for (int j0 = 0; j0 < K; j0 += Kc) {
        const int kc = std::min(Kc, K - j0);
        TA_LAUNCH_MAIN(ctx, "k_species_density", st,
                       launch_species_density(s.pm, s.f32, (long)pitch, (long)T, (long)A, s.D, d_q + (size_t)j0 * s.D, kc, S, d_species,
                                              d_w, part, G, st));
        TA_LAUNCH(ctx, "k_sum_partials", st, launch_sum_partials(part, G, (long)(kc * per), d_density + j0 * per, st));
    }
    if (d_cross) TA_CHECK(partial_cross(ctx, fft, d_density, K, S, T, d_cross, st));
    return call_end(ctx, st);
}

// ---- self van Hove function (vanhove.hip) and self-overlap (overlap.hip): what their host halves share --------------
// The host half of one call, before it is opened: the lags, then the n_tail doubles that fill(tail) forms once, here, queued
// for upload on `st` as one table.  Nothing on the device has been written when this fails.
template <class Fill>
int lag_table_plan(ta_ctx* ctx, HostTable& tab, const char* prefix, int L, const int64_t* h_lags, size_t n_tail, Fill&& fill,
                   int64_t A, int D, hipStream_t st) {
    TA_CHECK(check_cols(ctx, prefix, A, D));
    void* h = nullptr;
    TA_CHECK(tab.begin(ctx, sizeof(double) * ((size_t)L + n_tail), &h));
    static_assert(sizeof(int64_t) == sizeof(double), "the lags travel in the table's first n_lags slots");
    memcpy(h, h_lags, sizeof(int64_t) * (size_t)L);
    fill((double*)h + L);
    return tab.send(ctx, st);
}
// the lags of one launch: the family's chunk option (0: all L), at most L and what the kernel fits
int lag_chunk(int64_t opt, int L, int fit) { return (int)std::min<int64_t>({opt > 0 ? opt : (int64_t)L, (int64_t)L, (int64_t)fit}); }

// ---- self van Hove function (vanhove.hip) ---------------------------------------------------------------------------
// the table's tail: the squared edges e[0 ... B]
int vanhove_plan(ta_ctx* ctx, int L, const int64_t* h_lags, int B, double dr, int64_t A, int D, hipStream_t st) {
    return lag_table_plan(ctx, ctx->vh_tab, "vanhove: ", L, h_lags, (size_t)B + 1, [&](double* e) { vh_edges(B, dr, e); }, A, D, st);
}

// One van Hove call on a pair-major position slab of either element type, read as it is (the caller has opened the call's
// bracket, it is closed here; vanhove_plan has queued the table).  The uint64 histogram is zeroed, then one k_vanhove
// launch per chunk of Lc lags adds its bins and writes its columns of the workgroups' moment partials; after the last chunk
// the partials are added in a fixed order (k_sum_partials) and the histogram is copied out.  Nothing depends on Lc but which lags share a
// launch: the same bits for every chunk size.  ev[1] / ev[2] bracket the (last) pass.
int vanhove_pm(ta_ctx* ctx, const Slab& slab, int L, int B, double dr, int64_t* d_counts, double* d_moments) {
    hipStream_t st = slab.st;
    const int Lc = lag_chunk(ctx->opt_vanhove_chunk, L, vanhove_max_chunk(B));
    const int n_parts = vanhove_parts(ctx->n_cu, (long)slab.pitch, (long)slab.A);
    const size_t hist_bytes = sizeof(int64_t) * (size_t)L * (size_t)(B + 1);
    TA_CHECK(ensure(ctx, ctx->vh_hist, hist_bytes));
    TA_CHECK(ensure(ctx, ctx->vh_part, sizeof(double) * (size_t)n_parts * 2 * (size_t)L));
    const int64_t* d_lags = (const int64_t*)ctx->vh_tab.dev.p;
    const double* d_e = (const double*)ctx->vh_tab.dev.p + L;
    TA_HIP_TRY(ctx, hipMemsetAsync(ctx->vh_hist.p, 0, hist_bytes, st));
    for (int l0 = 0; l0 < L; l0 += Lc)
        TA_LAUNCH_MAIN(ctx, "k_vanhove", st,
                       launch_vanhove(ctx->n_cu, slab.pm, slab.f32, (long)slab.pitch, (long)slab.T, (long)slab.A, slab.D, d_lags, l0,
                                      std::min(Lc, L - l0), L, d_e, B, vh_inv_dr(dr), (unsigned long long*)ctx->vh_hist.p,
                                      (double*)ctx->vh_part.p, st));
    if (d_moments)
        TA_LAUNCH(ctx, "k_sum_partials", st, launch_sum_partials((const double*)ctx->vh_part.p, n_parts, 2L * L, d_moments, st));
    if (d_counts) TA_HIP_TRY(ctx, hipMemcpyAsync(d_counts, ctx->vh_hist.p, hist_bytes, hipMemcpyDeviceToDevice, st));
    return call_end(ctx, st);
}

// ---- self-overlap per origin (overlap.hip) --------------------------------------------------------------------------
// the table's tail: the squared cutoffs a2[c] = fl(a_c a_c)
int overlap_plan(ta_ctx* ctx, int L, const int64_t* h_lags, int C, const double* h_cutoffs, int64_t A, int D, hipStream_t st) {
    return lag_table_plan(ctx, ctx->ov_tab, "overlap: ", L, h_lags, (size_t)C, [&](double* a2) { vh_cutoffs2(C, h_cutoffs, a2); }, A, D, st);
}

// One overlap call on a pair-major position slab of either element type, read as it is (the caller has opened the call's
// bracket, it is closed here; overlap_plan has queued the table).  d_q (C, L, T) is zeroed, then one k_overlap launch per
// chunk of Lc lags adds its counts: Lc C <= the kernel's slots.  Nothing depends on Lc but which lags share a launch: the
// same bits for every chunk size.  ev[1] / ev[2] bracket the (last) launch.
int overlap_pm(ta_ctx* ctx, const Slab& slab, int L, int C, int64_t* d_q) {
    hipStream_t st = slab.st;
    const int Lc = lag_chunk(ctx->opt_overlap_chunk, L, std::max(1, overlap_slots() / C));
    const int64_t* d_lags = (const int64_t*)ctx->ov_tab.dev.p;
    const double* d_a2 = (const double*)ctx->ov_tab.dev.p + L;
    TA_HIP_TRY(ctx, hipMemsetAsync(d_q, 0, sizeof(int64_t) * (size_t)C * (size_t)L * (size_t)slab.T, st));
    for (int l0 = 0; l0 < L; l0 += Lc)
        TA_LAUNCH_MAIN(ctx, "k_overlap", st,
                       launch_overlap(ctx->n_cu, slab.pm, slab.f32, (long)slab.pitch, (long)slab.T, (long)slab.A, slab.D, d_lags, l0,
                                      std::min(Lc, L - l0), L, d_a2, C, (unsigned long long*)d_q, st));
    return call_end(ctx, st);
}

// ---- overlap field's density per origin (overlap_density.hip) ----------------------------------------------------------
constexpr size_t kOdBudget = (size_t)1 << 30;  // k_overlap_density's partial-sum buffer, as kPartialBudget (a choice)

// the table's tail: the squared cutoffs a2[c] = fl(a_c a_c), then the wavevectors in turns (q = k / 2 pi)
int overlap_density_plan(ta_ctx* ctx, int K, const double* h_kvecs, int L, const int64_t* h_lags, int C, const double* h_cutoffs,
                         int64_t A, int D, hipStream_t st) {
    return lag_table_plan(
        ctx, ctx->od_tab, "overlap_density: ", L, h_lags, (size_t)C + (size_t)K * D,
        [&](double* tail) {
            vh_cutoffs2(C, h_cutoffs, tail);
            for (size_t i = 0; i < (size_t)K * D; ++i) tail[C + i] = phase_turns(h_kvecs[i]);
        },
        A, D, st);
}

// One call on a pair-major position slab of either element type, read as it is (the caller has opened the call's bracket, it
// is closed here; overlap_density_plan has queued the table).  Per chunk of at most KC wavevectors and Lc lags (Lc C <= the
// tile's slots; "overlap_density_chunk" n: min(n, L, that count)) ONE k_overlap_density launch and the fixed-order sum of
// its partials into its corner of d_w (K, C, L, T, 2): every element is written, those at t0 >= T - tau as the +0.0 nothing
// was added to.  The atom groups depend on the slab and the device only: the same bits for every chunk size.  ev[1] / ev[2]
// bracket the (last) launch.
int overlap_density_pm(ta_ctx* ctx, const Slab& s, int K, int L, int C, double* d_w) {
    hipStream_t st = s.st;
    int SL = 1, KC = 1, F = 2;
    overlap_density_tile(&SL, &KC, &F);
    const int Lc = lag_chunk(ctx->opt_overlap_density_chunk, L, std::max(1, SL / C));
    const int G = overlap_density_parts(ctx->n_cu, (long)s.pitch, (long)s.A, kOdBudget);
    TA_CHECK(ensure(ctx, ctx->od_part, (size_t)G * SL * KC * (size_t)s.T * 16));
    double* part = (double*)ctx->od_part.p;
    const int64_t* d_lags = (const int64_t*)ctx->od_tab.dev.p;
    const double* d_a2 = (const double*)ctx->od_tab.dev.p + L;
    const double* d_q = d_a2 + C;
    for (int j0 = 0; j0 < K; j0 += KC) {
        const int kc = std::min(KC, K - j0);
        for (int l0 = 0; l0 < L; l0 += Lc) {
            const int lc = std::min(Lc, L - l0);
            TA_LAUNCH_MAIN(ctx, "k_overlap_density", st,
                           launch_overlap_density(s.pm, s.f32, (long)s.pitch, (long)s.T, (long)s.A, s.D, d_lags, l0, lc, L, d_a2, C,
                                                  d_q + (size_t)j0 * s.D, kc, part, G, st));
            TA_LAUNCH(ctx, "k_overlap_density_sum", st,
                      launch_overlap_density_sum(part, G, (long)s.T, lc, C, L, kc,
                                                 d_w + (((size_t)j0 * C) * L + l0) * (size_t)s.T * 2, st));
        }
    }
    return call_end(ctx, st);
}

// ---- distinct van Hove function (vanhove_distinct.hip) --------------------------------------------------------------
constexpr size_t kVhdBudget = (size_t)4 << 30;  // the gathered scratch of one pass (a choice, not a measurement)

// The caller's arguments of ta_vanhove_distinct*, as they came
struct VhdArgs {
    int L, B;
    double dr;
    int64_t stride, n_a, n_b;
    const int64_t *h_lags, *h_idx_a, *h_idx_b;
    const double* h_dims;
    const int* axes;
};

// What ta_vanhove_distinct* can check without the staged shape: the van Hove checks of ta_internal.hpp with the family's
// own between them.  T: the frames the lags are checked against (0: nothing staged -- the caller reports that next)
int vhd_args(ta_ctx* ctx, const VhdArgs& a, int64_t T, const void* out) {
    TA_CHECK(check_vanhove_grid(fail, ctx, "vanhove_distinct: ", a.L, a.h_lags, a.B, a.dr));
    if (a.stride < 1) return fail(ctx, TA_E_INVALID, "vanhove_distinct: origin_stride must be >= 1");
    if (!out) return fail(ctx, TA_E_INVALID, "vanhove_distinct: the counts output is NULL");
    if (a.h_idx_a && a.n_a < 1) return fail(ctx, TA_E_INVALID, "vanhove_distinct: n_a must be >= 1");
    if (a.h_idx_b && a.n_b < 1) return fail(ctx, TA_E_INVALID, "vanhove_distinct: n_b must be >= 1");
    if (a.h_dims && !a.axes) return fail(ctx, TA_E_INVALID, "vanhove_distinct: dimensions without axes");
    return check_vanhove_lags(fail, ctx, "vanhove_distinct: ", a.L, a.h_lags, T);
}

// ---- what the pair family's calls share on the host (both kinds of context): the box, the item lists, the table's tail ----
// The box of a call: per box H[3], M[3] of the staged columns (one box, or one per frame).  n_box 0: no box.
struct PairBox {
    bool per_frame = false;
    int64_t n_box = 0;
    std::vector<double> hm;
    const double* data() const { return hm.empty() ? nullptr : hm.data(); }
};
// Only the analysed axes' lengths count: the others are set to 1 before the table is made, so a zero length there (a slab
// geometry) is no error and a length that changes there makes no per-frame box.  who: "<call>: "
int image_box(ta_ctx* ctx, const std::string& who, const double* h_dims, const int* axes, int64_t T, int D, PairBox* b) {
    for (int d = 0; d < D; ++d)
        if (axes[d] < 0 || axes[d] > 2) return fail(ctx, TA_E_INVALID, who + "axes: every entry must be 0, 1 or 2");
    std::vector<double> dims(h_dims, h_dims + 6 * (size_t)T);
    for (int k = 0; k < 3; ++k)
        if (std::find(axes, axes + D, k) == axes + D)
            for (int64_t t = 0; t < T; ++t) dims[6 * (size_t)t + k] = 1.0;
    BoxTable box;
    const std::string why = box_table(dims.data(), T, D, axes, 1, &box);
    if (!why.empty()) return fail(ctx, TA_E_INVALID, who + why);
    if (box.triclinic)
        return fail(ctx, TA_E_INVALID, who + "a non-orthogonal box is not supported (the one-step image is not the minimum image there)");
    b->per_frame = box.per_frame;
    b->n_box = box.per_frame ? T : 1;
    b->hm.assign((size_t)b->n_box * 6, 1.0);
    for (int64_t t = 0; t < b->n_box; ++t)
        for (int d = 0; d < D; ++d) {
            b->hm[(size_t)t * 6 + d] = box.tab[(size_t)diag_row(axes[d]) * box.tpitch + t];
            b->hm[(size_t)t * 6 + 3 + d] = box.tab[(size_t)(6 + diag_row(axes[d])) * box.tpitch + t];
        }
    return TA_OK;
}
// `value` (reported as `name`) against half the box on the boxes of the frames 0, stride, 2 stride, ...
int half_box(ta_ctx* ctx, const std::string& who, const char* name, double value, const PairBox& b, int D, int64_t stride) {
    for (int64_t t = 0; t < b.n_box; t += stride)
        for (int d = 0; d < D; ++d)
            if (const double h = b.hm[(size_t)t * 6 + d]; !(value <= 0.5 * h))
                return fail(ctx, TA_E_INVALID, who + name + " = " + std::to_string(value) + " exceeds half the box length " + std::to_string(h) +
                                                   " of frame " + std::to_string(t));
    return TA_OK;
}

// The two index lists padded to the pair kernels' tiles (-1: padding); no b list: b = a.  who: "<call>"
struct ItemLists {
    int64_t n_a = 0, n_b = 0, pitch_a = 0, pitch_b = 0;
    std::vector<int32_t> ida, idb;
};
static int vhd_index_list(ta_ctx* ctx, const std::string& who, const char* name, int64_t n, const int64_t* idx, int64_t A, int64_t tile,
                          std::vector<int32_t>* out, int64_t* pitch) {
    for (int64_t i = 0; idx && i < n; ++i) {
        if (idx[i] < 0 || idx[i] >= A)
            return fail(ctx, TA_E_INVALID, who + ": index list " + name + ": entry " + std::to_string(idx[i]) +
                                               " is outside 0 ... n_atoms - 1");
        if (i && idx[i] <= idx[i - 1])
            return fail(ctx, TA_E_INVALID, who + ": index list " + name + " must be strictly increasing");
    }
    *pitch = (n + tile - 1) / tile * tile;
    out->assign((size_t)*pitch, -1);
    for (int64_t i = 0; i < n; ++i) (*out)[(size_t)i] = (int32_t)(idx ? idx[i] : i);
    return TA_OK;
}
int item_lists(ta_ctx* ctx, const std::string& who, int64_t n_a, const int64_t* h_idx_a, int64_t n_b, const int64_t* h_idx_b, int64_t A,
               ItemLists* p) {
    p->n_a = h_idx_a ? n_a : A;
    TA_CHECK(vhd_index_list(ctx, who, "a", p->n_a, h_idx_a, A, VHD_TILE_A, &p->ida, &p->pitch_a));
    if (!h_idx_b) h_idx_b = h_idx_a, n_b = p->n_a;  // b = a
    p->n_b = n_b;
    TA_CHECK(vhd_index_list(ctx, who, "b", p->n_b, h_idx_b, A, VHD_TILE_B, &p->idb, &p->pitch_b));
    // (a launch's grid is a-tiles x b-tiles in x: 256 threads each, below 2^32 threads)
    if ((p->pitch_a / VHD_TILE_A) * (p->pitch_b / VHD_TILE_B) >= VHD_MAX_TILES)
        return fail(ctx, TA_E_INVALID, who + ": ceil(n_a / " + std::to_string(VHD_TILE_A) + ") * ceil(n_b / " + std::to_string(VHD_TILE_B) +
                                           ") must be below 2^24 (about 2 million items on both sides)");
    return TA_OK;
}

// The tail hm | ida | idb of a call's table behind the caller's own head: its doubles (both pitches are even), the packer
// and the device pointers
struct PairTail {
    const double* hm;
    const int *ida, *idb;
};
size_t pair_tail_size(const PairBox& box, const ItemLists& l) { return box.hm.size() + (size_t)(l.pitch_a + l.pitch_b) / 2; }
void pair_tail_pack(double* q, const PairBox& box, const ItemLists& l) {
    static_assert(sizeof(int64_t) == sizeof(double) && 2 * sizeof(int32_t) == sizeof(double), "the table's slots");
    if (!box.hm.empty()) memcpy(q, box.hm.data(), sizeof(double) * box.hm.size());
    q += box.hm.size();
    memcpy(q, l.ida.data(), sizeof(int32_t) * l.ida.size());
    memcpy(q + l.pitch_a / 2, l.idb.data(), sizeof(int32_t) * l.idb.size());
}
PairTail pair_tail(const double* q, const PairBox& box, const ItemLists& l) {
    const int* ids = (const int*)(q + box.hm.size());
    return {box.hm.empty() ? nullptr : q, ids, ids + l.pitch_a};
}

// The host side of one van Hove call: the lists, the box, the origins of lag 0
struct VhdPlan : ItemLists {
    int L = 0, B = 0, D = 0;
    int64_t T = 0, stride = 1, n_orig = 0;
    PairBox box;
};

// Everything that needs the staged shape (T, A, D), checked before anything is written
int vhd_plan(ta_ctx* ctx, const VhdArgs& args, int64_t T, int64_t A, int D, VhdPlan* p) {
    auto [L, B, dr, stride, n_a, n_b, h_lags, h_idx_a, h_idx_b, h_dims, axes] = args;
    TA_CHECK(check_cols(ctx, "vanhove_distinct: ", A, D));
    p->L = L, p->B = B, p->D = D, p->T = T, p->stride = stride;
    TA_CHECK(item_lists(ctx, "vanhove_distinct", n_a, h_idx_a, n_b, h_idx_b, A, p));
    p->n_orig = vhd_origins(T, 0, stride);
    if (!h_dims) return TA_OK;
    TA_CHECK(image_box(ctx, "vanhove_distinct: ", h_dims, axes, T, D, &p->box));
    if (p->box.per_frame && h_lags[L - 1] > 0)
        return fail(ctx, TA_E_INVALID, "vanhove_distinct: per-frame boxes are accepted only when every lag is 0");
    return half_box(ctx, "vanhove_distinct: ", "n_bins * dr", (double)B * dr, p->box, D, stride);  // (origin frames only)
}

// The table of a call queued for upload on `st`, before the call is opened: lags (int64) | e[0 ... B] | hm | ida | idb
int vhd_upload(ta_ctx* ctx, const VhdPlan& p, const int64_t* h_lags, double dr, hipStream_t st) {
    double* h = nullptr;
    TA_CHECK(ctx->vhd_tab.begin(ctx, sizeof(double) * ((size_t)p.L + (size_t)p.B + 1 + pair_tail_size(p.box, p)), (void**)&h));
    memcpy(h, h_lags, sizeof(int64_t) * (size_t)p.L);
    vh_edges(p.B, dr, h + p.L);
    pair_tail_pack(h + p.L + p.B + 1, p.box, p);
    return ctx->vhd_tab.send(ctx, st);
}

// One call on a pair-major position slab of either element type (the caller has opened the call's bracket, it is closed
// here; vhd_upload has queued the table).  The uint64 histogram is zeroed; then per chunk of Lc lags one k_vhd_gather
// launch (GA with the first chunk) and one k_vhd_pairs launch per 65535 origins.  Nothing depends on Lc but which lags
// share a launch, and every add is an integer add: the same bits for every chunk size.  ev[1] / ev[2] bracket the LAST
// k_vhd_pairs launch only (as vanhove_pm's): with several chunks or more than 65535 origins ta_last_timing's main-kernel
// time is that launch's; the kernel timeline has them all.
int vhd_pm(ta_ctx* ctx, const Slab& slab, const VhdPlan& p, double dr, int64_t* d_counts) {
    hipStream_t st = slab.st;
    const int L = p.L, B = p.B, D = p.D;
    const double per_a = 8.0 * (double)p.n_orig * D * (double)p.pitch_a, per_lag = 8.0 * (double)p.n_orig * D * (double)p.pitch_b;
    if (per_a + per_lag > 4e18) return fail(ctx, TA_E_INVALID, "vanhove_distinct: the gathered scratch of one lag does not fit");
    const size_t bytes_a = (size_t)p.n_orig * D * (size_t)p.pitch_a * 8, bytes_lag = (size_t)p.n_orig * D * (size_t)p.pitch_b * 8;
    const int64_t fit = kVhdBudget > bytes_a + bytes_lag ? (int64_t)((kVhdBudget - bytes_a) / bytes_lag) : 1;
    const int Lc = (int)std::min<int64_t>(L, ctx->opt_vanhove_distinct_chunk > 0 ? ctx->opt_vanhove_distinct_chunk : fit);
    const size_t hist_bytes = sizeof(int64_t) * (size_t)L * (size_t)(B + 1);
    TA_CHECK(ensure(ctx, ctx->vhd_scr, bytes_a + (size_t)Lc * bytes_lag));
    TA_CHECK(ensure(ctx, ctx->vhd_hist, hist_bytes));
    const int64_t* lags = (const int64_t*)ctx->vhd_tab.dev.p;
    const double* e = (const double*)(lags + L);
    const PairTail tab = pair_tail(e + B + 1, p.box, p);
    double* ga = (double*)ctx->vhd_scr.p;
    double* gb = ga + bytes_a / 8;
    TA_HIP_TRY(ctx, hipMemsetAsync(ctx->vhd_hist.p, 0, hist_bytes, st));
    for (int l0 = 0; l0 < L; l0 += Lc) {
        const int lc = std::min(Lc, L - l0);
        TA_LAUNCH(ctx, "k_vhd_gather", st,
                  launch_vhd_gather(slab.pm, slab.f32, (long)slab.pitch, (long)slab.T, (long)slab.A, D, (long)p.stride, (long)p.n_orig,
                                    lags + l0, lc, l0 == 0, tab.ida, tab.idb, (long)p.pitch_a, (long)p.pitch_b, ga, gb, st));
        for (int64_t o0 = 0; o0 < p.n_orig; o0 += 65535)
            TA_LAUNCH_MAIN(ctx, "k_vhd_pairs", st,
                           launch_vhd_pairs(ga, gb, tab.ida, tab.idb, (long)p.pitch_a, (long)p.pitch_b, (long)p.n_a, (long)p.n_b, D,
                                            (long)slab.T, (long)p.stride, (long)p.n_orig, (long)o0,
                                            (int)std::min<int64_t>(65535, p.n_orig - o0), lags + l0, lc, tab.hm, p.box.per_frame, e, B,
                                            vh_inv_dr(dr), (unsigned long long*)ctx->vhd_hist.p + (size_t)l0 * (size_t)(B + 1), st));
    }
    TA_HIP_TRY(ctx, hipMemcpyAsync(d_counts, ctx->vhd_hist.p, hist_bytes, hipMemcpyDeviceToDevice, st));
    return call_end(ctx, st);
}

// What ta_vanhove_distinct_staged and ta_vanhove_distinct share once the plan is made: the table queued, the call opened,
// vhd_pm.  d_counts NULL = the context's own output buffer; *d_out (d_out NULL: not asked) tells where the counts are
int vhd_launch(ta_ctx* ctx, const VhdPlan& plan, const int64_t* h_lags, double dr, int64_t* d_counts, void* stream, int64_t** d_out) {
    return slab_entry(
        ctx, nullptr, stream, no_args,
        [&](const Slab& s) -> int {
            TA_CHECK(vhd_upload(ctx, plan, h_lags, dr, s.st));
            if (!d_counts) TA_CHECK(out_buffer(ctx, ctx->vhd_out, vhd_out(plan.L, plan.B), &d_counts));
            if (d_out) *d_out = d_counts;
            return TA_OK;
        },
        [&](const Slab& s) { return vhd_pm(ctx, s, plan, dr, d_counts); });
}

// ---- pair lifetimes: candidate search, indicator series, run lengths (pair_lifetime.hip) ----------------------------
constexpr size_t kPairBudget = (size_t)32 << 30;  // the indicator block of one block of pairs (a choice, as kScatterBudget)

// what both pair calls check of r_cut and the box arguments before the staged shape is needed
int pair_cut_args(ta_ctx* ctx, const std::string& who, double r_cut, const double* h_dims, const int* axes) {
    if (!(r_cut > 0.0) || !(r_cut - r_cut == 0.0)) return fail(ctx, TA_E_INVALID, who + "r_cut must be finite and greater than 0");
    if (h_dims && !axes) return fail(ctx, TA_E_INVALID, who + "dimensions without axes");
    return TA_OK;
}

// two lists must be the same list twice or disjoint ones (both increase strictly: one merge walk); *same: b is a
int lists_same_or_disjoint(ta_ctx* ctx, const std::string& who, const ItemLists& l, bool two_lists, bool* same) {
    *same = !two_lists;
    if (*same) return TA_OK;
    *same = l.n_a == l.n_b && std::equal(l.ida.begin(), l.ida.begin() + l.n_a, l.idb.begin());
    for (int64_t i = 0, j = 0; !*same && i < l.n_a && j < l.n_b;) {
        if (l.ida[i] == l.idb[j])
            return fail(ctx, TA_E_INVALID, who + "the index lists overlap (item " + std::to_string(l.ida[i]) +
                                               " is in both) but differ: they must be one list or disjoint");
        l.ida[i] < l.idb[j] ? ++i : ++j;
    }
    return TA_OK;
}

// The host side of one search (both kinds of context)
struct PairFindPlan : ItemLists {
    int D = 0;
    int64_t T = 0, A = 0, stride = 1, n_srch = 0;
    bool same = false;
    double rc2 = 0.0;
    PairBox box;
};
int pair_find_plan(ta_ctx* ctx, int64_t n_a, const int64_t* h_idx_a, int64_t n_b, const int64_t* h_idx_b, const double* h_dims,
                   const int* axes, double r_cut, int64_t stride, const void* out, PairFindPlan* p) {
    const std::string who = "pair_find: ";
    if (!out) return fail(ctx, TA_E_INVALID, who + "the n_pairs output is NULL");
    if (stride < 1) return fail(ctx, TA_E_INVALID, who + "search_stride must be >= 1");
    if (h_idx_a && n_a < 1) return fail(ctx, TA_E_INVALID, who + "n_a must be >= 1");
    if (h_idx_b && n_b < 1) return fail(ctx, TA_E_INVALID, who + "n_b must be >= 1");
    TA_CHECK(pair_cut_args(ctx, who, r_cut, h_dims, axes));
    TA_CHECK(check_staged(ctx));
    const int64_t T = ctx->st_T, A = ctx->st_A;
    const int D = ctx->st_D;
    TA_CHECK(check_cols(ctx, who, A, D));
    p->D = D, p->T = T, p->A = A, p->stride = stride, p->rc2 = r_cut * r_cut;
    TA_CHECK(item_lists(ctx, "pair_find", n_a, h_idx_a, n_b, h_idx_b, A, p));
    TA_CHECK(lists_same_or_disjoint(ctx, who, *p, h_idx_b != nullptr, &p->same));
    if (p->pitch_a * p->pitch_b > (int64_t)1 << 35)
        return fail(ctx, TA_E_INVALID, who + "the pair bitmap of " + std::to_string(p->pitch_a) + " x " + std::to_string(p->pitch_b) +
                                           " padded items exceeds 2^35 bits (4 GiB)");
    p->n_srch = vhd_origins(T, 0, stride);
    if (!h_dims) return TA_OK;
    TA_CHECK(image_box(ctx, who, h_dims, axes, T, D, &p->box));
    return half_box(ctx, who, "r_cut", r_cut, p->box, D, 1);
}

// One search on the staged position slab of either element type (the caller has opened the call's bracket, it is closed
// here; the table zero lag | hm | ida | idb has been queued).  The bitmap is zeroed; per chunk of searched frames one
// k_vhd_gather launch at lag 0 and one k_pair_find launch; k_pair_count, the block counts copied to the host (the call's
// only synchronisation) and scanned there, k_pair_list.  Nothing depends on the chunk: OR is idempotent.
int pair_find_pm(ta_ctx* ctx, const Slab& slab, const PairFindPlan& p) {
    hipStream_t st = slab.st;
    const int D = p.D;
    const int64_t* lag0 = (const int64_t*)ctx->pair_ftab.dev.p;
    const auto [hm, ida, idb] = pair_tail((const double*)(lag0 + 1), p.box, p);
    const size_t per = sizeof(double) * (size_t)D * (size_t)(p.pitch_a + p.pitch_b);
    const int64_t fit = std::max<int64_t>(1, (int64_t)(kVhdBudget / per));
    const int64_t oc = std::min<int64_t>({p.n_srch, 65535, ctx->opt_pair_find_chunk > 0 ? ctx->opt_pair_find_chunk : fit});
    const long n_words = (long)(p.pitch_a * p.pitch_b / 64), n_blk = pair_list_blocks(n_words);
    const size_t bits_bytes = sizeof(uint64_t) * (size_t)n_words, cnt_bytes = (sizeof(unsigned) * (size_t)n_blk + 7) / 8 * 8;
    TA_CHECK(ensure(ctx, ctx->vhd_scr, (size_t)oc * per));
    TA_CHECK(ensure(ctx, ctx->pair_bits, bits_bytes + cnt_bytes + sizeof(long long) * (size_t)n_blk));
    unsigned long long* bitmap = (unsigned long long*)ctx->pair_bits.p;
    unsigned* counts = (unsigned*)((char*)ctx->pair_bits.p + bits_bytes);
    long long* offs = (long long*)((char*)counts + cnt_bytes);
    double* ga = (double*)ctx->vhd_scr.p;
    ctx->pair_n = -1;
    TA_HIP_TRY(ctx, hipMemsetAsync(bitmap, 0, bits_bytes, st));
    for (int64_t o0 = 0; o0 < p.n_srch; o0 += oc) {
        const int64_t n_o = std::min(oc, p.n_srch - o0);
        double* gb = ga + (size_t)n_o * D * (size_t)p.pitch_a;
        TA_LAUNCH(ctx, "k_vhd_gather", st,
                  launch_vhd_gather(slab.pm, slab.f32, (long)slab.pitch, (long)slab.T, (long)slab.A, D, (long)p.stride, (long)n_o, lag0, 1,
                                    true, ida, idb, (long)p.pitch_a, (long)p.pitch_b, ga, gb, st, (long)o0));
        TA_LAUNCH_MAIN(ctx, "k_pair_find", st,
                       launch_pair_find(ga, gb, ida, idb, (long)p.pitch_a, (long)p.pitch_b, (long)p.n_a, (long)p.n_b, D, (long)slab.T,
                                        (long)p.stride, (long)o0, (int)n_o, hm, p.box.per_frame, p.rc2, p.same, bitmap, st));
    }
    TA_LAUNCH(ctx, "k_pair_count", st, launch_pair_count(bitmap, n_words, counts, st));
    std::vector<unsigned> h_counts((size_t)n_blk);
    std::vector<long long> h_offs((size_t)n_blk);
    TA_HIP_TRY(ctx, hipMemcpyAsync(h_counts.data(), counts, sizeof(unsigned) * (size_t)n_blk, hipMemcpyDeviceToHost, st));
    TA_HIP_TRY(ctx, hipStreamSynchronize(st));
    long long total = 0;
    for (long b = 0; b < n_blk; ++b) h_offs[(size_t)b] = total, total += h_counts[(size_t)b];
    if (total >= (long long)1 << 30)
        return fail(ctx, TA_E_INVALID, "pair_find: " + std::to_string(total) + " pairs found: the list holds fewer than 2^30");
    TA_CHECK(ensure(ctx, ctx->pair_list, sizeof(int32_t) * 2 * (size_t)total));
    if (total) {
        TA_HIP_TRY(ctx, hipMemcpyAsync(offs, h_offs.data(), sizeof(long long) * (size_t)n_blk, hipMemcpyHostToDevice, st));
        TA_LAUNCH(ctx, "k_pair_list", st, launch_pair_list(bitmap, n_words, (long)(p.pitch_b / 64), offs, ida, idb, (int*)ctx->pair_list.p, st));
        TA_HIP_TRY(ctx, hipStreamSynchronize(st));  // (h_offs leaves with this scope)
    }
    ctx->pair_n = total, ctx->pair_A = p.A;
    return call_end(ctx, st);
}

int pair_find_launch(ta_ctx* ctx, const PairFindPlan& p) {
    return slab_entry(
        ctx, nullptr, ctx->stream, no_args,
        [&](const Slab& s) -> int {
            double* h = nullptr;
            TA_CHECK(ctx->pair_ftab.begin(ctx, sizeof(double) * (1 + pair_tail_size(p.box, p)), (void**)&h));
            memset(h, 0, sizeof(double));  // the zero lag (int64)
            pair_tail_pack(h + 1, p.box, p);
            return ctx->pair_ftab.send(ctx, s.st);
        },
        [&](const Slab& s) { return pair_find_pm(ctx, s, p); });
}

// The outputs of a lifetime or shell call as the caller gave them, on the device (the staged entries) or on the host: lags is
// ci of the three-output calls and sums of the gated ones (ta_shell_msd*, ta_shell_orient*), which alone have count.  NULL:
// not asked for.
struct LifePtrs {
    double* lags;
    int64_t* count;
    int64_t* runs;
    double* nb;
    bool any() const { return lags || count || runs || nb; }
};
// Where a host-facing call's results lie in ctx->pair_out, in LifePtrs' order: ci (T) | no count | runs (T + 1) | nb (T) of
// the three-output calls (n_sums 0), sums ((L + 1) n_sums) | count (L + 1) | runs | nb of the gated ones.
OutLayout life_out(int64_t T, int64_t L = 0, int n_sums = 0) {
    return {n_sums ? out_n(L + 1, n_sums) : out_n(T), n_sums ? out_n(L + 1) : 0, out_n(T + 1), out_n(T)};
}
// the device outputs of those asked for in `want`, in the buffer at `base`
LifePtrs life_at(const OutLayout& o, double* base, const LifePtrs& want) {
    return {o.at(base, 0, want.lags), (int64_t*)o.at(base, 1, want.count), (int64_t*)o.at(base, 2, want.runs), o.at(base, 3, want.nb)};
}
// the tail of a host-facing call: the results at d_out copied into those of `h` asked for
int life_finish(ta_ctx* ctx, const OutLayout& o, const LifePtrs& h, const double* d_out) {
    return out_finish(ctx, o, d_out, {h.lags, h.count, h.runs, h.nb});
}

// What ta_bond_lifetime* add to a lifetime call: items per row, the break criterion, the gap tolerance
struct BondArgs {
    int n_at;
    double r_break, cos_cut, cos_break;
    int gap;
};
// The host side of one lifetime call (both kinds of context).  h_pairs NULL: the context's found list.  A pair call is a
// bond call of 2 items per row whose break criterion is its form criterion, without gap tolerance: bond == false, and
// the pair kernels run as ever.
struct PairLifePlan {
    int64_t P = 0;
    const int32_t* h_pairs = nullptr;
    double rc2 = 0.0;
    PairBox box;
    bool bond = false;
    int n_at = 2, gap = 0;
    ta::BondCuts cuts{};
    // the level block needs k_pair_filter: a gap to close, or a break criterion apart from the form criterion
    bool filter() const { return gap > 0 || cuts.rb2 != cuts.rc2 || (n_at == 3 && cuts.cb2 != cuts.c2); }
    OutLayout out;
};
int bond_rows(ta_ctx* ctx, const std::string& who, int64_t n_bonds, int n_at, const int32_t* h_atoms, int64_t A) {
    if (n_bonds < 1 || n_bonds >= (int64_t)1 << 30) return fail(ctx, TA_E_INVALID, who + "n_bonds must be 1 ... 2^30 - 1");
    if (!h_atoms) return fail(ctx, TA_E_INVALID, who + "the atoms list is NULL");
    for (int64_t n = 0; n < n_bonds; ++n) {
        const int32_t* r = h_atoms + (size_t)n_at * (size_t)n;
        for (int i = 0; i < n_at; ++i) {
            if (r[i] < 0 || r[i] >= A)
                return fail(ctx, TA_E_INVALID, who + "bond " + std::to_string(n) + " names item " + std::to_string(r[i]) +
                                                   " outside 0 ... n_atoms - 1");
            for (int j = 0; j < i; ++j)
                if (r[j] == r[i]) return fail(ctx, TA_E_INVALID, who + "bond " + std::to_string(n) + " names item " + std::to_string(r[i]) + " twice");
        }
    }
    return TA_OK;
}
int pair_life_plan(ta_ctx* ctx, int fft, int64_t n_pairs, const int32_t* h_pairs, const double* h_dims, const int* axes, double r_cut,
                   bool any_out, PairLifePlan* p, const BondArgs* bond = nullptr) {
    const std::string who = bond ? "bond_lifetime: " : "pair_lifetime: ";
    TA_CHECK(check_fft(ctx, fft));
    if (!any_out) return fail(ctx, TA_E_INVALID, who + "the ci, runs and nb outputs are all NULL");
    if (bond && bond->n_at != 2 && bond->n_at != 3) return fail(ctx, TA_E_INVALID, who + "n_at must be 2 (pairs) or 3 (donor, hydrogen, acceptor)");
    TA_CHECK(pair_cut_args(ctx, who, r_cut, h_dims, axes));
    p->rc2 = r_cut * r_cut, p->h_pairs = h_pairs;
    p->cuts = ta::BondCuts{p->rc2, p->rc2, 0.0, 0.0};
    if (bond) {
        p->bond = true, p->n_at = bond->n_at, p->gap = bond->gap;
        if (!(bond->r_break - bond->r_break == 0.0) || bond->r_break < r_cut)
            return fail(ctx, TA_E_INVALID, who + "r_break must be finite and at least r_cut");
        p->cuts.rb2 = bond->r_break * bond->r_break;
        if (bond->n_at == 3) {  // (pairs have no angle: their cosines are not looked at)
            for (const double c : {bond->cos_cut, bond->cos_break})
                if (!(c >= -1.0 && c <= 0.0)) return fail(ctx, TA_E_INVALID, who + "cos_cut and cos_break must lie in [-1, 0] (angles of 90 ... 180 degrees)");
            if (bond->cos_break < bond->cos_cut)
                return fail(ctx, TA_E_INVALID, who + "cos_break must be at least cos_cut (the break angle at most the form angle)");
            p->cuts.c2 = bond->cos_cut * bond->cos_cut, p->cuts.cb2 = bond->cos_break * bond->cos_break;
        }
        if (bond->gap < 0 || bond->gap > 63)
            return fail(ctx, TA_E_INVALID, who + "gap must be 0 ... 63 (absences are closed inside a window of three 64-frame words)");
    }
    TA_CHECK(check_staged(ctx));
    const int64_t T = ctx->st_T, A = ctx->st_A;
    TA_CHECK(check_cols(ctx, who, A, ctx->st_D));
    if (bond) {
        TA_CHECK(bond_rows(ctx, who, n_pairs, bond->n_at, h_pairs, A));
        p->P = n_pairs;
    } else if (h_pairs) {
        if (n_pairs < 1 || n_pairs >= (int64_t)1 << 30) return fail(ctx, TA_E_INVALID, who + "n_pairs must be 1 ... 2^30 - 1");
        for (int64_t n = 0; n < n_pairs; ++n) {
            const int32_t a = h_pairs[2 * n], b = h_pairs[2 * n + 1];
            if (a < 0 || a >= A || b < 0 || b >= A)
                return fail(ctx, TA_E_INVALID, who + "pair " + std::to_string(n) + " (" + std::to_string(a) + ", " + std::to_string(b) +
                                                   ") is outside 0 ... n_atoms - 1");
            if (a == b) return fail(ctx, TA_E_INVALID, who + "pair " + std::to_string(n) + " names item " + std::to_string(a) + " twice");
        }
        p->P = n_pairs;
    } else {
        const bool have = ctx->pair_n >= 0 && ctx->pair_A == A && (ctx->is_cpu || ctx->pair_list.p);
        if (!have)
            return fail(ctx, TA_E_STATE, who + "no pair list has been found for the staged slab (ta_pair_find comes first; ta_trim "
                                               "releases it)");
        if (ctx->pair_n == 0) return fail(ctx, TA_E_STATE, who + "the found pair list is empty");
        p->P = ctx->pair_n;
    }
    p->out = life_out(T);
    if (!h_dims) return TA_OK;
    TA_CHECK(image_box(ctx, who, h_dims, axes, T, ctx->st_D, &p->box));
    return half_box(ctx, who, bond ? "r_break" : "r_cut", bond ? bond->r_break : r_cut, p->box, ctx->st_D, 1);
}

// the candidate pairs per block: "pair_chunk", or as many as kPairBudget holds of the indicator block
int64_t pair_block(const ta_ctx* ctx, int64_t P, int64_t pitch) {
    const int64_t fit = std::max<int64_t>(2, 2 * (int64_t)(kPairBudget / ((size_t)pitch * 16)));
    return std::min<int64_t>(P, ctx->opt_pair_chunk > 0 ? ctx->opt_pair_chunk : fit);
}
// The table of a lifetime call, hm | pairs (the int32 rows of an explicit list) | Pc zero labels: the pairs per block, where
// the parts begin and the whole, in doubles
struct PairTab {
    int64_t Pc;
    size_t pairs, lab, n;
};
PairTab pair_tab_layout(const ta_ctx* ctx, const PairLifePlan& p, int64_t pitch) {
    const int64_t Pc = pair_block(ctx, p.P, pitch);
    const size_t pairs = p.box.hm.size(), lab = pairs + (p.h_pairs ? ((size_t)p.n_at * (size_t)p.P + 1) / 2 : 0);
    return {Pc, pairs, lab, lab + ((size_t)Pc + 1) / 2};
}

// One lifetime call on the staged position slab of either element type, read as it is (the caller has opened the call's
// bracket, it is closed here; the table hm | pairs | zero labels has been queued).  Per block of pairs: k_pair_series
// writes the indicator block Z (P_b pseudo-atoms of dim 1), k_pair_runs adds its runs to the histogram, ONE VACF lag-sum
// evaluation of Z is the block's row of ci / (T - tau), ONE species-sum pass with unit weights its row of nb.  The rows are
// added in block order by k_pair_reduce, which also takes the 1 / (T - tau) out again: with fft = 0 every product is exact,
// a row's value times (T - tau) is within (partial sums + 2) 2^-53 of the integer it stands for (at most P_b T <= 2^32 with
// the automatic block), and rint gives that integer: the same bits for every block size.  ev[1] / ev[2] bracket the
// (last) k_pair_series launch, unless a lag-sum evaluation after it records its own main kernel.  A bond call (p.bond) has
// k_bond_series in k_pair_series' place, rows of p.n_at items, and k_pair_filter behind it where p.filter() says so.
// What follows a block's level or indicator block Z, for pair_life_pm and shell_pm alike: the workspaces of a call of P
// series in blocks of Pc (begin), the block's passes over Z (block: the filter where asked for, the runs, the lag sums, the
// bonded counts; lab: Pc zero labels on the device), the rows added in block order into the outputs and the call closed (end).
struct LifeSums {
    bool fft = false;
    int64_t T = 0, pitch = 0, Pc = 0, n_blocks = 0;
    int parts_full = 0, parts_last = 0;
    double *Z = nullptr, *ci_rows = nullptr, *nb_rows = nullptr, *d_ci = nullptr, *d_nb = nullptr;
    unsigned long long* runs = nullptr;
    int64_t* d_runs = nullptr;
    hipStream_t st = nullptr;
};
int life_sums_begin(ta_ctx* ctx, bool fft, const Slab& slab, int64_t P, int64_t Pc, double* d_ci, int64_t* d_runs, double* d_nb, LifeSums* s) {
    const int64_t T = slab.T, n_blocks = (P + Pc - 1) / Pc;
    *s = LifeSums{fft, T, slab.pitch, Pc, n_blocks};
    s->d_ci = d_ci, s->d_runs = d_runs, s->d_nb = d_nb, s->st = slab.st;
    TA_CHECK(ensure(ctx, ctx->pair_z, (size_t)((Pc + 1) / 2) * (size_t)slab.pitch * 16));
    const size_t n_rows = (size_t)n_blocks * (size_t)T;
    TA_CHECK(ensure(ctx, ctx->pair_rows, sizeof(double) * (2 * n_rows + (size_t)T + 1)));
    s->ci_rows = (double*)ctx->pair_rows.p;
    s->nb_rows = s->ci_rows + n_rows;
    s->runs = (unsigned long long*)(s->nb_rows + n_rows);
    const int64_t P_last = P - (n_blocks - 1) * Pc;
    s->parts_full = species_sum_parts(ctx->n_cu, 1, (long)T, (long)Pc), s->parts_last = species_sum_parts(ctx->n_cu, 1, (long)T, (long)P_last);
    if (d_nb) TA_CHECK(ensure(ctx, ctx->ons_part, sizeof(double) * (size_t)std::max(s->parts_full, s->parts_last) * (size_t)T));
    s->Z = (double*)ctx->pair_z.p;
    if (d_runs) TA_HIP_TRY(ctx, hipMemsetAsync(s->runs, 0, sizeof(uint64_t) * ((size_t)T + 1), s->st));
    return TA_OK;
}
int life_sums_block(ta_ctx* ctx, const LifeSums& s, int64_t b, int64_t pb, bool filter, int gap, const int* lab) {
    hipStream_t st = s.st;
    const int64_t T = s.T, pitch = s.pitch;
    double* Z = s.Z;
    if (filter) TA_LAUNCH(ctx, "k_pair_filter", st, launch_pair_filter(ctx->n_cu, Z, (long)pitch, (long)T, (long)pb, gap, st));
    if (s.d_runs) TA_LAUNCH(ctx, "k_pair_runs", st, launch_pair_runs(ctx->n_cu, Z, (long)pitch, (long)T, (long)pb, s.runs, st));
    if (s.d_ci) TA_CHECK(acf_impl(ctx, s.fft, Z, pitch, T, pb, 1, s.ci_rows + (size_t)b * T, nullptr, 0, st));
    if (s.d_nb)
        TA_CHECK(weighted_total(ctx, Z, false, pitch, T, pb, 1, lab, nullptr, pb == s.Pc ? s.parts_full : s.parts_last,
                                s.nb_rows + (size_t)b * T, st));
    return TA_OK;
}
int life_sums_end(ta_ctx* ctx, const LifeSums& s) {
    hipStream_t st = s.st;
    const int64_t T = s.T;
    if (s.d_ci)
        TA_LAUNCH(ctx, "k_pair_reduce", st,
                  launch_pair_reduce(s.ci_rows, (int)s.n_blocks, (long)T, (long)T, s.fft ? PAIR_LAGS : PAIR_LAGS_INT, s.d_ci, st));
    if (s.d_nb) TA_LAUNCH(ctx, "k_pair_reduce", st, launch_pair_reduce(s.nb_rows, (int)s.n_blocks, (long)T, (long)T, PAIR_SUM, s.d_nb, st));
    if (s.d_runs) TA_HIP_TRY(ctx, hipMemcpyAsync(s.d_runs, s.runs, sizeof(int64_t) * ((size_t)T + 1), hipMemcpyDeviceToDevice, st));
    return call_end(ctx, st);
}

int pair_life_pm(ta_ctx* ctx, bool fft, const Slab& slab, const PairLifePlan& p, const LifePtrs& d) {
    hipStream_t st = slab.st;
    const int64_t T = slab.T, pitch = slab.pitch, P = p.P;
    const PairTab t = pair_tab_layout(ctx, p, pitch);
    const int64_t Pc = t.Pc;
    const double* tab = (const double*)ctx->pair_tab.dev.p;
    const double* hm = p.box.n_box ? tab : nullptr;
    const int* pairs = p.h_pairs ? (const int*)(tab + t.pairs) : (const int*)ctx->pair_list.p;
    const int* lab = (const int*)(tab + t.lab);
    LifeSums s;
    TA_CHECK(life_sums_begin(ctx, fft, slab, P, Pc, d.lags, d.runs, d.nb, &s));
    for (int64_t b = 0; b < s.n_blocks; ++b) {
        const int64_t p0 = b * Pc, pb = std::min(Pc, P - p0);
        if (p.bond)
            TA_LAUNCH_MAIN(ctx, "k_bond_series", st,
                           launch_bond_series(ctx->n_cu, slab.pm, slab.f32, (long)pitch, (long)T, (long)slab.A, slab.D, (long)pb, p.n_at,
                                              pairs + p.n_at * p0, hm, p.box.per_frame, p.cuts, p.filter() ? 2.0 : 1.0, s.Z, st));
        else
            TA_LAUNCH_MAIN(ctx, "k_pair_series", st,
                           launch_pair_series(ctx->n_cu, slab.pm, slab.f32, (long)pitch, (long)T, (long)slab.A, slab.D, (long)pb, pairs + 2 * p0,
                                              hm, p.box.per_frame, p.rc2, s.Z, st));
        TA_CHECK(life_sums_block(ctx, s, b, pb, p.filter(), p.gap, lab));
    }
    return life_sums_end(ctx, s);
}

// ta_pair_lifetime_staged and the device half of ta_pair_lifetime (out != NULL: the context's own output buffer, laid out by
// p.out, takes the place of the pointers of d, which then only say what is asked for)
int pair_life_launch(ta_ctx* ctx, int fft, const PairLifePlan& p, const LifePtrs& d, void* stream, double** out) {
    return slab_entry(
        ctx, nullptr, stream, no_args,
        [&](const Slab& s) -> int {
            const PairTab t = pair_tab_layout(ctx, p, s.pitch);
            double* h = nullptr;
            TA_CHECK(ctx->pair_tab.begin(ctx, sizeof(double) * t.n, (void**)&h));
            memset(h, 0, sizeof(double) * t.n);
            if (!p.box.hm.empty()) memcpy(h, p.box.hm.data(), sizeof(double) * p.box.hm.size());
            if (p.h_pairs) memcpy(h + t.pairs, p.h_pairs, sizeof(int32_t) * (size_t)p.n_at * (size_t)p.P);
            if (out) TA_CHECK(out_buffer(ctx, ctx->pair_out, p.out, out));
            return ctx->pair_tab.send(ctx, s.st);
        },
        [&](const Slab& s) { return pair_life_pm(ctx, fft != 0, s, p, out ? life_at(p.out, *out, d) : d); });
}

// ---- shell residence times: the level of an observed item against a group of reference items (shell.hip) ------------
// The three kinds of call: the residence sums alone (ta_shell_residence*), or in ci's place the gated sums over the lags
// 0 ... max_lag of squared displacements (ta_shell_msd*) or of the unit vectors' products (ta_shell_orient*)
enum ShellKind { SHELL_RESIDENCE, SHELL_MSD, SHELL_ORIENT };
// The caller's arguments, as they came; behind gap those of the gated kinds, and behind max_lag those of ta_shell_orient* alone
struct ShellArgs {
    int64_t n_a, n_b;
    const int64_t *h_idx_a, *h_idx_b;
    const double* h_dims;
    const int* axes;
    double r_cut, r_break;
    int gap;
    int condition = 0;
    int64_t max_lag = 0;
    int mode = 0, anchor = 0;
    const int32_t* h_index = nullptr;
};
// The host side of one call (both kinds of context): a = the reference items, b = the observed ones, one series per b-item.
// The b list carries one more tile of padding than item_lists gives it: a block of observed items is read from its first
// item on, a whole number of tiles long.  n_sums: the gated sums per lag (0: SHELL_RESIDENCE, D: SHELL_MSD, 2:
// SHELL_ORIENT); row_len: the atoms per index row of h_index, one row per observed item (0 but for SHELL_ORIENT).
struct ShellPlan : ItemLists {
    ShellKind kind = SHELL_RESIDENCE;
    int D = 0, gap = 0;
    int64_t T = 0, A = 0;
    ta::BondCuts cuts{};
    PairBox box;
    int condition = 0, n_sums = 0, mode = 0, row_len = 0;
    int64_t L = 0;
    const int32_t* h_index = nullptr;
    OutLayout out;
    bool filter() const { return gap > 0 || cuts.rb2 != cuts.rc2; }
    // what the CPU backend's three calls share
    ta::cpu::ShellItems cpu() const { return {n_a, ida.data(), n_b, idb.data(), box.data(), box.per_frame, &cuts, gap}; }
};
// The argument checks of a call of `kind`, in the order the entries have always made them: what the gated kinds check before
// anything else (the mode, the anchor column and the index table; the condition), what every kind checks, and what the gated
// kinds check against the staged shape (max_lag against the frames and the cap; three staged columns and the box on x, y, z,
// ta_orient's checks of the index rows, and every row's anchor against the observed items)
int shell_plan(ta_ctx* ctx, ShellKind kind, int fft, const ShellArgs& a, bool any_out, ShellPlan* p) {
    const char* name = kind == SHELL_RESIDENCE ? "shell_residence" : kind == SHELL_MSD ? "shell_msd" : "shell_orient";
    const std::string who = std::string(name) + ": ";
    p->kind = kind;
    if (kind == SHELL_ORIENT) {
        if (a.mode < ORIENT_BOND || a.mode > ORIENT_NORMAL)
            return fail(ctx, TA_E_INVALID, who + "mode must be TA_ORIENT_BOND (0), TA_ORIENT_BISECTOR (1) or TA_ORIENT_NORMAL (2)");
        p->mode = a.mode, p->row_len = orient_row_len(a.mode), p->h_index = a.h_index;
        if (a.anchor < 0 || a.anchor >= p->row_len)
            return fail(ctx, TA_E_INVALID, who + "anchor must be a column of the index rows, 0 ... " + std::to_string(p->row_len - 1));
        if (!a.h_index) return fail(ctx, TA_E_INVALID, who + "the index table is NULL");
    }
    if (kind != SHELL_RESIDENCE && a.condition != ta::SHELL_CONTINUOUS && a.condition != ta::SHELL_ENDPOINTS)
        return fail(ctx, TA_E_INVALID, who + "condition must be 0 (continuous) or 1 (endpoints)");

    TA_CHECK(check_fft(ctx, fft));
    if (!any_out)
        return fail(ctx, TA_E_INVALID, who + "the " + (kind == SHELL_RESIDENCE ? "ci, runs and nb" : "sums, count, runs and nb") + " outputs are all NULL");
    if (a.h_idx_a && a.n_a < 1) return fail(ctx, TA_E_INVALID, who + "n_a must be >= 1");
    if (a.h_idx_b && a.n_b < 1) return fail(ctx, TA_E_INVALID, who + "n_b must be >= 1");
    TA_CHECK(pair_cut_args(ctx, who, a.r_cut, a.h_dims, a.axes));
    if (!(a.r_break - a.r_break == 0.0) || a.r_break < a.r_cut) return fail(ctx, TA_E_INVALID, who + "r_break must be finite and at least r_cut");
    if (a.gap < 0 || a.gap > 63)
        return fail(ctx, TA_E_INVALID, who + "gap must be 0 ... 63 (absences are closed inside a window of three 64-frame words)");
    TA_CHECK(check_staged(ctx));
    const int64_t T = ctx->st_T, A = ctx->st_A;
    const int D = ctx->st_D;
    TA_CHECK(check_cols(ctx, who, A, D));
    p->D = D, p->T = T, p->A = A, p->gap = a.gap;
    p->cuts = ta::BondCuts{a.r_cut * a.r_cut, a.r_break * a.r_break, 0.0, 0.0};
    TA_CHECK(item_lists(ctx, name, a.n_a, a.h_idx_a, a.n_b, a.h_idx_b, A, p));
    bool same = false;
    TA_CHECK(lists_same_or_disjoint(ctx, who, *p, a.h_idx_b != nullptr, &same));
    if (p->n_b >= (int64_t)1 << 30) return fail(ctx, TA_E_INVALID, who + "n_b must be below 2^30");
    p->pitch_b += VHD_TILE_B;
    p->idb.resize((size_t)p->pitch_b, -1);
    if (a.h_dims) {
        TA_CHECK(image_box(ctx, who, a.h_dims, a.axes, T, D, &p->box));
        TA_CHECK(half_box(ctx, who, "r_break", a.r_break, p->box, D, 1));
    }

    if (kind != SHELL_RESIDENCE) {
        if (a.max_lag < 0 || a.max_lag > T - 1)
            return fail(ctx, TA_E_INVALID, who + "max_lag must be 0 ... n_frames - 1 = " + std::to_string(T - 1));
        if (a.max_lag > ta::kShellMsdMaxLag)
            return fail(ctx, TA_E_INVALID, who + "max_lag must be at most " + std::to_string(ta::kShellMsdMaxLag) + " (eight passes of 256 lags)");
        p->condition = a.condition, p->L = a.max_lag, p->n_sums = kind == SHELL_ORIENT ? 2 : D;
    }
    p->out = life_out(T, p->L, p->n_sums);
    if (kind != SHELL_ORIENT) return TA_OK;
    if (D != 3) return fail(ctx, TA_E_INVALID, who + "the position slab must hold three columns per atom (dim = " + std::to_string(D) + ")");
    if (a.h_dims && !(a.axes[0] == 0 && a.axes[1] == 1 && a.axes[2] == 2))
        return fail(ctx, TA_E_INVALID, who + "the box needs the three columns x, y, z (axes {0, 1, 2})");
    if (A * 3 >= (int64_t)1 << 31 || p->n_b * 6 >= (int64_t)1 << 31)
        return fail(ctx, TA_E_INVALID, who + "n_atoms * 3 and n_vectors * 6 must be below 2^31");
    const int K = p->row_len;
    for (int64_t n = 0; n < p->n_b; ++n) {
        const int32_t* r = a.h_index + n * K;
        for (int j = 0; j < K; ++j)
            if (r[j] < 0 || r[j] >= A)
                return fail(ctx, TA_E_INVALID, who + "index " + std::to_string(r[j]) + " of vector " + std::to_string(n) +
                                                   " is outside 0 ... n_atoms - 1");
        if (r[0] == r[1] || (K == 3 && (r[0] == r[2] || r[1] == r[2])))
            return fail(ctx, TA_E_INVALID, who + "vector " + std::to_string(n) + " names an atom twice");
        if (r[a.anchor] != p->idb[(size_t)n])
            return fail(ctx, TA_E_INVALID, who + "the anchor of vector " + std::to_string(n) + " (atom " + std::to_string(r[a.anchor]) +
                                               ") is not observed item " + std::to_string(n) + " (atom " + std::to_string(p->idb[(size_t)n]) + ")");
    }
    return TA_OK;
}

// the observed items per block: pair_block's count of series; a block behind the first starts at an even item
int64_t shell_block(const ta_ctx* ctx, int64_t n_b, int64_t pitch) {
    const int64_t Qc = pair_block(ctx, n_b, pitch);
    return Qc < n_b ? std::max<int64_t>(2, Qc & ~(int64_t)1) : Qc;
}
// The table of a call, zero lag | hm | ida | idb (pair_tail_*) | Qc zero labels | index rows (n_b rows of row_len int32): the
// observed items per block, where the parts begin and the whole, in doubles
struct ShellTab {
    int64_t Qc;
    size_t tail, lab, rows, n;
};
ShellTab shell_tab_layout(const ta_ctx* ctx, const ShellPlan& p, int64_t pitch) {
    const int64_t Qc = shell_block(ctx, p.n_b, pitch);
    const size_t tail = 1, lab = tail + pair_tail_size(p.box, p), rows = lab + ((size_t)Qc + 1) / 2;
    return {Qc, tail, lab, rows, rows + ((size_t)p.n_b * (size_t)p.row_len + 1) / 2};
}

// One call on the staged position slab of either element type (the caller has opened the call's bracket, it is closed here;
// the table has been queued).  Per block of observed items: per chunk of whole 64-frame words one k_vhd_gather launch at
// lag 0, stride 1 (the reference items and the block's observed items, read in the slab's own element type) and one
// k_shell_series launch, which writes the chunk's rows of the level block Z; then life_sums_block, pair_life_pm's passes.
// Neither chunking changes a bit: every row of Z has one writer whatever the chunk, and the blocks' rows are added as
// pair_life_pm's.  ev[1] / ev[2] bracket the (last) k_shell_series launch, unless a lag-sum evaluation after it records its
// own main kernel.
// A gated call (p.n_sums; no ci) with sums or count asked for: behind a block's filter k_shell_bits packs its series,
// k_shell_msd (shell_msd.hip) adds up the gated squared displacements of the block's items over the lags 0 ... L and
// k_shell_fold adds the workgroups' partial rows in row order onto sums and count: the blocks in block order.
// SHELL_ORIENT: k_shell_orient (shell_orient.hip) stands in k_shell_msd's place, the walk over the unit vectors of the block's
// index rows (one per observed item, its anchor) with the distance pass's boxes for the image step; two sums per lag.
// ids: the block's observed items; rows, hm (SHELL_ORIENT): the block's index rows and the boxes on the device
int shell_gated_block(ta_ctx* ctx, const ShellPlan& p, const Slab& slab, const LifeSums& s, int64_t b, int64_t nb, const int* ids,
                      const int* rows, const double* hm, const LifePtrs& d) {
    hipStream_t st = slab.st;
    const int G = ta::shell_msd_groups(ctx->n_cu, (long)nb, (long)p.L), chunk = ta::shell_msd_chunk((long)ctx->opt_shell_msd_chunk);
    unsigned long long* words = (unsigned long long*)ctx->shell_words.p;
    TA_LAUNCH(ctx, "k_shell_bits", st, ta::launch_shell_bits(ctx->n_cu, s.Z, (long)s.pitch, (long)s.T, (long)nb, words, st));
    if (p.kind == SHELL_ORIENT)
        TA_LAUNCH(ctx, "k_shell_orient", st,
                  ta::launch_shell_orient(slab.pm, slab.f32, (long)slab.pitch, (long)slab.T, (long)slab.A, slab.D, p.mode, rows, (long)nb, hm,
                                          p.box.per_frame, words, p.condition, (long)p.L, chunk, G, ctx->shell_part.p, st));
    else
        TA_LAUNCH(ctx, "k_shell_msd", st,
                  ta::launch_shell_msd(slab.pm, slab.f32, (long)slab.pitch, (long)slab.T, (long)slab.A, slab.D, ids, (long)nb, words,
                                       p.condition, (long)p.L, chunk, G, ctx->shell_part.p, st));
    TA_LAUNCH(ctx, "k_shell_fold", st,
              ta::launch_shell_fold(ctx->shell_part.p, G, (long)p.L, p.n_sums, b == 0, d.lags, (long long*)d.count, st));
    return TA_OK;
}
int shell_pm(ta_ctx* ctx, bool fft, const Slab& slab, const ShellPlan& p, const LifePtrs& d) {
    hipStream_t st = slab.st;
    const int D = p.D;
    const ShellTab t = shell_tab_layout(ctx, p, slab.pitch);
    const int64_t T = slab.T, pitch = slab.pitch, N = p.n_b, Qc = t.Qc;
    const double* tab = (const double*)ctx->shell_tab.dev.p;
    const int64_t* lag0 = (const int64_t*)tab;
    const auto [hm, ida, idb] = pair_tail(tab + t.tail, p.box, p);
    const int *lab = (const int*)(tab + t.lab), *rows = (const int*)(tab + t.rows);
    const int64_t pitch_q = (Qc + VHD_TILE_B - 1) / VHD_TILE_B * VHD_TILE_B, words = (T + 63) / 64;
    const size_t per = sizeof(double) * (size_t)D * (size_t)(p.pitch_a + pitch_q);  // a gathered frame
    const int64_t fit = std::max<int64_t>(1, (int64_t)(kVhdBudget / (64 * per)));
    const int64_t wc = std::min<int64_t>({words, 65535, ctx->opt_shell_chunk > 0 ? ctx->opt_shell_chunk : fit});
    TA_CHECK(ensure(ctx, ctx->vhd_scr, (size_t)std::min(T, 64 * wc) * per));
    double* ga = (double*)ctx->vhd_scr.p;
    const bool gated = p.n_sums && (d.lags || d.count);
    if (gated) {
        TA_CHECK(ensure(ctx, ctx->shell_words, sizeof(uint64_t) * (size_t)Qc * (size_t)words));
        TA_CHECK(ensure(ctx, ctx->shell_part,
                        ta::shell_msd_part_bytes(ta::shell_msd_groups(ctx->n_cu, (long)Qc, (long)p.L), (long)p.L, p.n_sums)));
    }
    LifeSums s;
    TA_CHECK(life_sums_begin(ctx, fft, slab, N, Qc, p.n_sums ? nullptr : d.lags, d.runs, d.nb, &s));
    for (int64_t b = 0; b < s.n_blocks; ++b) {
        const int64_t q0 = b * Qc, nb = std::min(Qc, N - q0), pitch_b = (nb + VHD_TILE_B - 1) / VHD_TILE_B * VHD_TILE_B;
        for (int64_t w0 = 0; w0 < words; w0 += wc) {
            const int64_t f_base = 64 * w0, n_f = std::min(T, 64 * (w0 + wc)) - f_base;
            double* gb = ga + (size_t)n_f * D * (size_t)p.pitch_a;
            TA_LAUNCH(ctx, "k_vhd_gather", st,
                      launch_vhd_gather(slab.pm, slab.f32, (long)pitch, (long)T, (long)slab.A, D, 1, (long)n_f, lag0, 1, true, ida, idb + q0,
                                        (long)p.pitch_a, (long)pitch_b, ga, gb, st, (long)f_base));
            TA_LAUNCH_MAIN(ctx, "k_shell_series", st,
                           launch_shell_series(ga, gb, ida, idb + q0, (long)p.pitch_a, (long)pitch_b, (long)p.n_a, (long)nb, D, (long)T,
                                               (long)pitch, (long)f_base, (long)n_f, hm, p.box.per_frame, p.cuts.rc2, p.cuts.rb2,
                                               p.filter() ? 2.0 : 1.0, s.Z, st));
        }
        TA_CHECK(life_sums_block(ctx, s, b, nb, p.filter(), p.gap, lab));
        if (gated) TA_CHECK(shell_gated_block(ctx, p, slab, s, b, nb, idb + q0, rows + p.row_len * q0, hm, d));
    }
    return life_sums_end(ctx, s);
}

// The staged entries and the device half of the host-facing ones (out as pair_life_launch's)
int shell_launch(ta_ctx* ctx, int fft, const ShellPlan& p, const LifePtrs& d, void* stream, double** out) {
    return slab_entry(
        ctx, nullptr, stream, no_args,
        [&](const Slab& s) -> int {
            const ShellTab t = shell_tab_layout(ctx, p, s.pitch);
            double* h = nullptr;
            TA_CHECK(ctx->shell_tab.begin(ctx, sizeof(double) * t.n, (void**)&h));
            memset(h, 0, sizeof(double) * t.n);  // (the zero lag in front, the zero labels)
            pair_tail_pack(h + t.tail, p.box, p);
            std::copy_n(p.h_index, (size_t)p.n_b * (size_t)p.row_len, (int32_t*)(h + t.rows));
            if (out) TA_CHECK(out_buffer(ctx, ctx->pair_out, p.out, out));
            return ctx->shell_tab.send(ctx, s.st);
        },
        [&](const Slab& s) { return shell_pm(ctx, fft != 0, s, p, out ? life_at(p.out, *out, d) : d); });
}

// ---- the staged shape, and the CPU backend's side of the entry points ----------------------------------------------
// This is the seam: a CPU context's staging and host-facing calls end up in the cpu_* functions below, reached by one
// early branch of their entry point (after the checks both kinds of context share); nothing below makes a HIP call.
void set_staged(ta_ctx* ctx, int64_t T, int64_t A, int D, int dtype, int n_slabs, bool dev_f32) {
    ctx->st_T = T, ctx->st_A = A, ctx->st_D = D, ctx->st_dtype = dtype, ctx->st_nslabs = n_slabs;
    ctx->st_dev_f32 = dev_f32;
    ctx->st_pitch = pm_pitch(T);
    ctx->pair_n = -1;  // (a found pair list belongs to the staging it was found in)
}

// what cpu_backend.cpp works on: the staged shape and the host slabs, read where they are
ta::cpu::State cpu_state(const ta_ctx* ctx) {
    ta::cpu::State s;
    s.T = ctx->st_T, s.A = ctx->st_A, s.D = ctx->st_D, s.dtype = ctx->st_dtype, s.threads = ctx->cpu_threads;
    s.slabs = ctx->h_slabs;
    return s;
}

// host slabs in the reference's (n_frames, n_atoms, dim) layout, zero-filled mappings like the GPU contexts' (never
// page-locked)
int cpu_stage_alloc(ta_ctx* ctx, int64_t n_frames, int64_t n_atoms, int dim, int dtype, int n_slabs, void** h_slabs) {
    if (!h_slabs) return fail(ctx, TA_E_UNSUPPORTED, "the CPU backend has no device slabs");
    ta_stage_free(ctx);
    const size_t bytes = (size_t)n_frames * n_atoms * dim * (dtype == TA_F32 ? 4 : 8);
    for (int i = 0; i < n_slabs; ++i) {
        HostBlock blk;
        if (host_block_map(bytes, &blk) != 0) {
            ta_stage_free(ctx);
            return fail(ctx, TA_E_NOMEM, "staging allocation failed: no host memory for the slab");
        }
        ctx->h_slabs.push_back(blk.base);
        ctx->h_blocks.push_back(blk);
        h_slabs[i] = blk.base;
    }
    set_staged(ctx, n_frames, n_atoms, dim, dtype, n_slabs, false);
    return TA_OK;
}

// the tail of every CPU branch: the backend's return code (0, or TA_E_NOMEM) as the entry's
int cpu_rc(ta_ctx* ctx, int rc) { return rc ? fail(ctx, rc, "CPU backend: out of host memory") : TA_OK; }

int cpu_shell(ta_ctx* ctx, bool fft, const ShellPlan& p, const LifePtrs& h) {
    const ta::cpu::State s = cpu_state(ctx);
    return cpu_rc(ctx, p.kind == SHELL_RESIDENCE ? ta::cpu::shell_residence(s, fft, p.cpu(), h.lags, h.runs, h.nb)
                       : p.kind == SHELL_MSD     ? ta::cpu::shell_msd(s, p.condition, p.L, p.cpu(), h.lags, h.count, h.runs, h.nb)
                                                 : ta::cpu::shell_orient(s, p.condition, p.L, p.mode, p.h_index, p.cpu(), h.lags, h.count, h.runs, h.nb));
}

// the mean over atoms of a lag-indexed sum (velocityautocorr.py:214,237; viscosity.py:233)
void atom_mean(const ta_ctx* ctx, double* h_ts) {
    const double n_at = (double)ctx->st_A;
    for (int64_t k = 0; k < ctx->st_T; ++k) h_ts[k] /= n_at;
}

int cpu_compute(ta_ctx* ctx, int which, const double* h_masses, double scale, double* h_ts, double* h_bp) {
    TA_CHECK(check_staged(ctx, slabs_needed(which)));
    if (which == W_HELFAND && !h_masses) return fail(ctx, TA_E_INVALID, "h_masses is NULL");
    const ta::cpu::State s = cpu_state(ctx);
    const int rc = which == W_FFT      ? ta::cpu::vacf_fft(s, h_ts, h_bp)
                   : which == W_DIRECT ? ta::cpu::vacf_direct(s, h_ts, h_bp)
                   : is_msd(which)     ? ta::cpu::msd(s, which == W_MSD_FFT, h_ts, h_bp)
                                       : ta::cpu::helfand(s, h_masses, scale, h_ts, h_bp);
    TA_CHECK(cpu_rc(ctx, rc));
    atom_mean(ctx, h_ts);
    return TA_OK;
}

int cpu_conductivity(ta_ctx* ctx, bool fft, const double* h_charges, double* h_moment, double* h_collective,
                     double* h_self_lagsum) {
    return cpu_rc(ctx, ta::cpu::conductivity(cpu_state(ctx), fft, h_charges, h_moment, h_collective, h_self_lagsum));
}

// ---- options: the table behind ta_set_option ------------------------------------------------------------------------
int opt_check_direct_mfma(ta_ctx* ctx, int64_t value) {
    if (value != 0 && value != 1 && value != 3)
        return fail(ctx, TA_E_INVALID, "direct_mfma: 0 vector kernels, 1 by trajectory length (default), 3 matrix cores always "
                                       "(2, the column-packed forms, left the library in round 6: tools/band/)");
    return TA_OK;
}
int opt_set_cpu_threads(ta_ctx* ctx, int64_t value) {
    if (value < 0 || value > 4096) return fail(ctx, TA_E_INVALID, "cpu_threads: 0 (default) .. 4096");
    ctx->cpu_threads = value > 0 ? (int)value : ta::cpu::hardware_threads();
    return TA_OK;
}
int opt_flush_commits(ta_ctx* ctx, int64_t) { return ctx->commits.flush(); }
int opt_check_kcurrent_chunk(ta_ctx* ctx, int64_t value) {
    return value >= 0 ? TA_OK : fail(ctx, TA_E_INVALID, "kcurrent_chunk: 0 (the tile's count) or the wavevectors per launch");
}
int opt_check_partial_chunk(ta_ctx* ctx, int64_t value) {
    return value >= 0 ? TA_OK : fail(ctx, TA_E_INVALID, "partial_chunk: 0 (the tile's count) or the wavevectors per launch");
}
int opt_check_partial_cross_chunk(ta_ctx* ctx, int64_t value) {
    return value >= 0 ? TA_OK : fail(ctx, TA_E_INVALID, "partial_cross_chunk: 0 (automatic) or the wavevectors per batch");
}
int opt_check_chain_modes_chunk(ta_ctx* ctx, int64_t value) {
    return value >= 0 ? TA_OK : fail(ctx, TA_E_INVALID, "chain_modes_chunk: 0 (automatic) or the modes per batch");
}
int opt_check_scatter_chunk(ta_ctx* ctx, int64_t value) {
    return value >= 0 ? TA_OK : fail(ctx, TA_E_INVALID, "scatter_chunk: 0 (automatic) or the wavevectors per pass");
}
int opt_check_vanhove_distinct_chunk(ta_ctx* ctx, int64_t value) {
    return value >= 0 ? TA_OK : fail(ctx, TA_E_INVALID, "vanhove_distinct_chunk: 0 (automatic) or the lags per pass");
}
int opt_check_pair_chunk(ta_ctx* ctx, int64_t value) {
    return value >= 0 ? TA_OK : fail(ctx, TA_E_INVALID, "pair_chunk: 0 (automatic) or the candidate pairs per block");
}
int opt_check_pair_find_chunk(ta_ctx* ctx, int64_t value) {
    return value >= 0 ? TA_OK : fail(ctx, TA_E_INVALID, "pair_find_chunk: 0 (automatic) or the searched frames per pass");
}
int opt_check_shell_chunk(ta_ctx* ctx, int64_t value) {
    return value >= 0 ? TA_OK : fail(ctx, TA_E_INVALID, "shell_chunk: 0 (automatic) or the 64-frame words per pass");
}
int opt_check_shell_msd_chunk(ta_ctx* ctx, int64_t value) {
    return value >= 0 ? TA_OK : fail(ctx, TA_E_INVALID, "shell_msd_chunk: 0 (automatic) or the origin frames per staged chunk");
}
int opt_check_overlap_chunk(ta_ctx* ctx, int64_t value) {
    return value >= 0 ? TA_OK : fail(ctx, TA_E_INVALID, "overlap_chunk: 0 (automatic) or the lags per launch");
}
int opt_check_overlap_density_chunk(ta_ctx* ctx, int64_t value) {
    return value >= 0 ? TA_OK : fail(ctx, TA_E_INVALID, "overlap_density_chunk: 0 (automatic) or the lags per launch");
}
int opt_check_vanhove_chunk(ta_ctx* ctx, int64_t value) {
    return value >= 0 ? TA_OK : fail(ctx, TA_E_INVALID, "vanhove_chunk: 0 (automatic) or the lags per pass");
}

struct Option {
    const char* key;
    int64_t ta_ctx::*field;
    int (*hook)(ta_ctx*, int64_t);
};
#define X(key, dflt, hook) {#key, &ta_ctx::opt_##key, hook},
const Option kOptions[] = {TA_OPTIONS(X)};
#undef X

}  // namespace

extern "C" {

int ta_abi_version(void) { return 6; }

int ta_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* ta_last_error(const ta_ctx* ctx) {
    if (!ctx) return g_tls_error.c_str();
    // a copy made under the lock, owned by the calling thread until its next call
    thread_local std::string copy;
    try {
        std::lock_guard<std::mutex> lk(g_err_m);
        copy = ctx->err;
    } catch (...) {
        return "out of memory while reading the error message";
    }
    return copy.c_str();
}

int ta_ctx_create(int device, ta_ctx** out) {
    return ta::guarded(fail, nullptr, [&]() -> int {
    if (!out) return fail(nullptr, TA_E_INVALID, "out is NULL");
    *out = nullptr;
    if (device == TA_DEVICE_CPU) {  // the opt-in CPU backend: no HIP call at all
        if (!ta::cpu::supported()) return fail(nullptr, TA_E_UNSUPPORTED, "the CPU backend is built for hosts with AVX2 and FMA");
        ta_ctx* c = new (std::nothrow) ta_ctx();
        if (!c) return fail(nullptr, TA_E_NOMEM, "out of host memory");
        c->is_cpu = true;
        c->device = TA_DEVICE_CPU;
        c->n_cu = 0;
        c->cpu_threads = ta::cpu::hardware_threads();
        *out = c;
        return TA_OK;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n < 1)
        return fail(nullptr, TA_E_HIP,
                    "no usable HIP device (this library has no CPU fallback): " +
                        std::string(e != hipSuccess ? hipGetErrorString(e) : "device count 0"));
    if (device < 0 || device >= n) return fail(nullptr, TA_E_INVALID, "device index out of range (TA_DEVICE_CPU = -1 asks for the CPU backend)");
    ta_ctx* ctx = new (std::nothrow) ta_ctx();
    if (!ctx) return fail(nullptr, TA_E_NOMEM, "out of host memory");
    ctx->device = device;
    hipDeviceProp_t prop;
    e = hipSetDevice(device);
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    for (auto& q : ctx->ring)
        for (auto& ev : q)
            if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_stage, hipEventDisableTiming);
    if (e != hipSuccess) {
        const std::string msg = std::string("context setup: ") + hipGetErrorString(e);
        ta_ctx_destroy(ctx);  // frees whatever was created
        return fail(nullptr, TA_E_HIP, msg);
    }
    ctx->n_cu = prop.multiProcessorCount;
    *out = ctx;
    return TA_OK;
    });
}

int ta_stage_free(ta_ctx* ctx) {
    return ta::guarded(fail, ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    if (!ctx->is_cpu) {  // nothing queued may still read or write the slabs
        (void)ctx->commits.flush();  // (an error of a commit into slabs that are going away is dropped with them)
        hipSetDevice(ctx->device);
        if (ctx->stream) hipStreamSynchronize(ctx->stream);
        if (ctx->relayout_stream) hipStreamSynchronize(ctx->relayout_stream);
    }
    for (size_t i = 0; i < ctx->h_slabs.size(); ++i) {
        if (ctx->h_blocks[i].base) host_block_unmap(ctx->h_blocks[i]);
        else if (ctx->h_slabs[i]) hipHostFree(ctx->h_slabs[i]);  // (GPU contexts only: the allocator's fallback block)
    }
    for (double* d : ctx->d_slabs)
        if (d) hipFree(d);
    ctx->h_blocks.clear();
    ctx->h_slabs.clear();
    ctx->d_slabs.clear();
    ctx->st_nslabs = 0;
    ctx->st_T = ctx->st_A = ctx->st_pitch = 0;
    ctx->st_compound = false;
    return TA_OK;
    });
}

int ta_ctx_destroy(ta_ctx* ctx) {
    return ta::guarded(fail, ctx, [&]() -> int {
    if (!ctx) return TA_OK;
    if (ctx->is_cpu) {
        ta_stage_free(ctx);
        delete ctx;
        return TA_OK;
    }
    (void)ctx->commits.flush();
    ctx->commits.stop();
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    ta_stage_free(ctx);
    for (auto& kv : ctx->wf_tables) hipFree(kv.second);
    for (DevBuf* b : ctx->workspaces) b->release();
    for (auto& q : ctx->ring)
        for (auto& ev : q)
            if (ev) hipEventDestroy(ev);
    if (ctx->ev_stage) hipEventDestroy(ctx->ev_stage);
    for (HostTable* t : ctx->tables)
        if (t->ev) {
            hipEventSynchronize(t->ev);  // (the upload may be on a caller's stream)
            hipEventDestroy(t->ev);
        }
    for (hipEvent_t e : ctx->mark_pool) hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) {
        if (ctx->ev_piece[i]) hipEventDestroy(ctx->ev_piece[i]);
        if (ctx->ev_done[i]) hipEventDestroy(ctx->ev_done[i]);
    }
    if (ctx->relayout_stream) hipStreamDestroy(ctx->relayout_stream);
    if (ctx->copy_stream) hipStreamDestroy(ctx->copy_stream);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
    return TA_OK;
    });
}

int ta_trim(ta_ctx* ctx) {
    return ta::guarded(fail, ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    if (ctx->is_cpu) return TA_OK;  // (no workspaces outlive a call)
    TA_CHECK(ctx->commits.flush());
    hipSetDevice(ctx->device);
    hipDeviceSynchronize();
    for (DevBuf* b : ctx->workspaces)
        if (b->trimmed) b->release();
    return TA_OK;
    });
}

int ta_set_option(ta_ctx* ctx, const char* key, int64_t value) {
    return ta::guarded(fail, ctx, [&]() -> int {
    if (!ctx || !key) return fail(ctx, TA_E_INVALID, "null argument");
    for (const Option& o : kOptions) {
        if (strcmp(key, o.key)) continue;
        if (o.hook) TA_CHECK(o.hook(ctx, value));
        ctx->*o.field = value;
        return TA_OK;
    }
    return fail(ctx, TA_E_INVALID, std::string("unknown option ") + key);
    });
}

int ta_fft_plan_info(int64_t n_frames, int64_t* m_out, int* n_threads, int* n_stages) {
    return ta::guarded(fail, nullptr, [&]() -> int {
    int R0 = 0, R = 1;
    if (!wfft_choose((long)n_frames, &R0, &R))
        return fail(nullptr, TA_E_UNSUPPORTED, "n_frames exceeds the largest FFT plan");
    // [outer radix R while the rows are read,] first-stage radix R0 (none up to 512 frames), then
    // one wave per 512-point sub-series (8 x 8 x 8)
    if (m_out) *m_out = (int64_t)R * R0 * 512;
    if (n_threads) *n_threads = wfft_threads(R0);
    if (n_stages) *n_stages = (R0 == 1 ? 3 : 4) + (R > 1 ? 1 : 0);
    return TA_OK;
    });
}

/* --------------------------------------------- pinned host memory for results */
}  // extern "C"

namespace {
// result arrays handed out by ta_host_alloc*: mapping -> page-locked in one piece (a 2-D device->host copy spans all of
// it); ta_host_free finds them here by address
std::mutex g_host_m;
std::map<void*, size_t> g_host_blocks;  // base -> mapped length
}  // namespace

extern "C" {

int ta_host_alloc_on(int device, int64_t n_bytes, void** h_out) {
    return ta::guarded(fail, nullptr, [&]() -> int {
    if (!h_out || n_bytes < 0) return fail(nullptr, TA_E_INVALID, "bad argument");
    *h_out = nullptr;
    // the allocating thread may be a fresh helper thread whose current device is 0: bind it to the
    // analysis' own GPU first, so that no context is created on a device the rank does not use
    if (device >= 0) {
        const hipError_t es = hipSetDevice(device);
        if (es != hipSuccess)
            return fail(nullptr, TA_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(es));
    }
    // an anonymous mapping page-locked by ONE hipHostRegister (portable: usable by every device's copy engines; the
    // result outlives the context): 4 GiB in ~0.2 s where hipHostMalloc takes 0.5-0.9 s with the runtime's lock held
    const size_t len = ((size_t)std::max<int64_t>(n_bytes, 16) + ((size_t)2 << 20) - 1) / ((size_t)2 << 20) * ((size_t)2 << 20);
    void* m = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m != MAP_FAILED) {
        (void)madvise(m, len, MADV_HUGEPAGE);
        if (hipHostRegister(m, len, hipHostRegisterPortable) == hipSuccess) {
            std::lock_guard<std::mutex> lk(g_host_m);
            g_host_blocks[m] = len;
            *h_out = m;
            return TA_OK;
        }
        (void)hipGetLastError();
        munmap(m, len);
    }
    void* h = nullptr;
    const hipError_t e = hipHostMalloc(&h, (size_t)std::max<int64_t>(n_bytes, 16), hipHostMallocPortable);
    if (e != hipSuccess)
        return fail(nullptr, TA_E_NOMEM, std::string("pinned host allocation failed: ") + hipGetErrorString(e));
    *h_out = h;
    return TA_OK;
    });
}

int ta_host_alloc(int64_t n_bytes, void** h_out) { return ta_host_alloc_on(-1, n_bytes, h_out); }

int ta_host_free(void* h) {
    return ta::guarded(fail, nullptr, [&]() -> int {
    if (!h) return TA_OK;
    size_t len = 0;
    {
        std::lock_guard<std::mutex> lk(g_host_m);
        auto it = g_host_blocks.find(h);
        if (it != g_host_blocks.end()) len = it->second, g_host_blocks.erase(it);
    }
    if (len) {
        const hipError_t e = hipHostUnregister(h);
        munmap(h, len);
        return e == hipSuccess ? TA_OK : fail(nullptr, TA_E_HIP, std::string("hipHostUnregister: ") + hipGetErrorString(e));
    }
    const hipError_t e = hipHostFree(h);
    return e == hipSuccess ? TA_OK : fail(nullptr, TA_E_HIP, std::string("hipHostFree: ") + hipGetErrorString(e));
    });
}

/* ------------------------------------------------------------------ staging */
static int stage_alloc_common(ta_ctx* ctx, int64_t n_frames, int64_t n_atoms, int dim, int dtype,
                              int n_slabs, void** h_slabs) {
    TA_CHECK(check_shape(ctx, n_frames, n_atoms, dim, n_atoms * dim));
    if (n_slabs < 1 || n_slabs > 4) return fail(ctx, TA_E_INVALID, "bad slab count");
    TA_CHECK(check_dtype(ctx, dtype));
    if (ctx->is_cpu) return cpu_stage_alloc(ctx, n_frames, n_atoms, dim, dtype, n_slabs, h_slabs);
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ta_stage_free(ctx);
    const size_t n = (size_t)n_frames * n_atoms * dim;
    const size_t esz = dtype == TA_F32 ? 4 : 8;
    // device slabs hold float32 when the option asks for it and nothing wider is coming in
    const bool dev_f32 = ctx->opt_stage_device_f32 && (dtype == TA_F32 || !h_slabs);
    const size_t dbytes = pm_bytes(n_frames, n_atoms * dim, dev_f32);
    for (int i = 0; i < n_slabs; ++i) {
        void* h = nullptr;
        double* d = nullptr;
        hipError_t e = hipSuccess;
        HostBlock blk;
        if (h_slabs) {
            // zero-filled like the reference's np.zeros (velocityautocorr.py:150); page-locked as it is committed
            if (host_block_map(n * esz, &blk) == 0) h = blk.base;
            else {  // no mapping to be had: the runtime's allocator
                e = hipHostMalloc(&h, n * esz, hipHostMallocDefault);
                if (e == hipSuccess) host_zero(h, n * esz);
            }
        }
        if (e == hipSuccess) e = hipMalloc((void**)&d, dbytes);
        if (e != hipSuccess) {
            if (blk.base) host_block_unmap(blk);
            else if (h) hipHostFree(h);
            ta_stage_free(ctx);
            return fail(ctx, TA_E_NOMEM, std::string("staging allocation failed: ") + hipGetErrorString(e));
        }
        ctx->h_slabs.push_back(h);
        ctx->h_blocks.push_back(blk);
        ctx->d_slabs.push_back(d);
        // frames never committed read as zeros, like the reference's np.zeros slab
        TA_HIP_TRY(ctx, hipMemsetAsync(d, 0, dbytes, ctx->stream));
        if (h_slabs) h_slabs[i] = h;
    }
    set_staged(ctx, n_frames, n_atoms, dim, dtype, n_slabs, dev_f32);
    // the zero fill ran on the context's stream; later fills may come on any stream
    TA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // the worker starts page-locking the slabs' first chunks while the caller sets up its frame loop (an empty job)
    if (h_slabs && ctx->opt_async_commit && ctx->opt_lock_ahead) ctx->commits.push(0, 0);
    return TA_OK;
}

int ta_stage_alloc(ta_ctx* ctx, int64_t n_frames, int64_t n_atoms, int dim, int dtype, int n_slabs,
                   void** h_slabs) {
    return ta::guarded(fail, ctx, [&]() -> int {
    if (!h_slabs) return fail(ctx, TA_E_INVALID, "h_slabs is NULL");
    return stage_alloc_common(ctx, n_frames, n_atoms, dim, dtype, n_slabs, h_slabs);
    });
}

int ta_stage_alloc_device(ta_ctx* ctx, int64_t n_frames, int64_t n_atoms, int dim, int n_slabs) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return stage_alloc_common(ctx, n_frames, n_atoms, dim, TA_F64, n_slabs, nullptr);
    });
}

}  // extern "C"

// Frames [frame_lo, frame_hi) of every host slab -> the device slabs.  The range is not empty and has been checked by
// ta_stage_commit, the only way here (directly, or through the commit queue).
static int stage_commit_now(ta_ctx* ctx, int64_t frame_lo, int64_t frame_hi) {
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t row = (size_t)ctx->st_A * ctx->st_D;
    const size_t esz = ctx->st_dtype == TA_F32 ? 4 : 8;
    // frames cross PCIe in their native width into one of two landing buffers (<= 64 MiB each) and
    // are transposed into the pair-major slab on the device (float32 widened on the way), on a
    // second stream: piece i + 1 crosses PCIe while piece i is transposed
    const int64_t per = std::max<int64_t>(1, (int64_t)(((size_t)64 << 20) / (row * esz)));
    const int64_t chunk = std::min<int64_t>(per, frame_hi - frame_lo);
    TA_CHECK(ensure(ctx, ctx->bounce, (size_t)chunk * row * esz));
    TA_CHECK(ensure(ctx, ctx->bounce2, (size_t)chunk * row * esz));
    if (!ctx->relayout_stream) {
        TA_HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->relayout_stream, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            TA_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_piece[i], hipEventDisableTiming));
            TA_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_done[i], hipEventDisableTiming));
        }
    }
    void* land[2] = {ctx->bounce.p, ctx->bounce2.p};
    bool used[2] = {false, false};
    // the slabs may still be read by work queued earlier on the context's stream
    TA_HIP_TRY(ctx, hipEventRecord(ctx->ev_stage, ctx->stream));
    TA_HIP_TRY(ctx, hipStreamWaitEvent(ctx->relayout_stream, ctx->ev_stage, 0));
    int piece = 0;
    for (int i = 0; i < ctx->st_nslabs; ++i) {
        for (int64_t f = frame_lo; f < frame_hi; f += chunk, ++piece) {
            const int b = piece & 1;
            const int64_t m = std::min(chunk, frame_hi - f);
            const char* src = (const char*)ctx->h_slabs[i] + (size_t)f * row * esz;
            if (used[b]) TA_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_done[b], 0));  // buffer free again
            HostBlock& blk = ctx->h_blocks[i];
            if (blk.base) {
                // page-lock the chunks these frames live in (first commit of each: 64 MiB at 23 GB/s), then copy in
                // segments that stay inside one chunk
                const size_t s0 = (size_t)f * row * esz, s1 = s0 + (size_t)m * row * esz;
                TA_HIP_TRY(ctx, host_block_lock(blk, s0, s1));
                for (size_t p = s0; p < s1;) {
                    const size_t e = std::min(s1, (p / HostBlock::kChunk + 1) * HostBlock::kChunk);
                    TA_HIP_TRY(ctx, hipMemcpyAsync((char*)land[b] + (p - s0), blk.base + p, e - p, hipMemcpyHostToDevice, ctx->stream));
                    p = e;
                }
            } else
                TA_HIP_TRY(ctx, hipMemcpyAsync(land[b], src, (size_t)m * row * esz, hipMemcpyHostToDevice, ctx->stream));
            TA_HIP_TRY(ctx, hipEventRecord(ctx->ev_piece[b], ctx->stream));
            TA_HIP_TRY(ctx, hipStreamWaitEvent(ctx->relayout_stream, ctx->ev_piece[b], 0));
            TA_HIP_TRY(ctx, launch_relayout(land[b], ctx->st_dtype == TA_F32, (long)row, (long)row, m,
                                            ctx->d_slabs[i], ctx->st_dev_f32, ctx->st_pitch, f, ctx->relayout_stream));
            TA_HIP_TRY(ctx, hipEventRecord(ctx->ev_done[b], ctx->relayout_stream));
            used[b] = true;
        }
    }
    // whatever follows on the context's stream sees the transposed frames
    for (int b = 0; b < 2; ++b)
        if (used[b]) TA_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_done[b], 0));
    return TA_OK;
}

// Page-locking ahead of the frame loop (round 6): behind a commit the worker registers the next chunks of every slab --
// pages no frame has touched yet, which the registration faults in -- so that the filling threads find their pages present
// and the commits that follow find their chunks registered (before: every chunk was registered by the commit that first
// needed it, with the loop's threads page-faulting on it meanwhile: frame fills 0.12 s -> 0.42 s at 10000 x 50000 x 3).
static void stage_lock_ahead(ta_ctx* ctx, int64_t frame_from) {
    constexpr size_t kAhead = 3;
    const size_t row = (size_t)ctx->st_A * ctx->st_D, esz = ctx->st_dtype == TA_F32 ? 4 : 8;
    const size_t s0 = (size_t)frame_from * row * esz;
    for (size_t i = 0; i < ctx->h_blocks.size(); ++i) {
        HostBlock& blk = ctx->h_blocks[i];
        if (blk.base && s0 < blk.bytes) (void)host_block_lock(blk, s0, std::min(blk.bytes, s0 + kAhead * HostBlock::kChunk));
    }
}

// ---- the commit queue (rules: on the class) ------------------------------------------------------------------------
void CommitQueue::push(int64_t frame_lo, int64_t frame_hi) {
    if (!thread_.joinable()) thread_ = std::thread([this] { run(); });
    {
        std::lock_guard<std::mutex> lk(m_);
        jobs_.emplace_back(frame_lo, frame_hi);
    }
    cv_.notify_all();
}

void CommitQueue::run() {
    (void)hipSetDevice(ctx_->device);
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
        cv_.wait(lk, [&] { return stop_ || !jobs_.empty(); });
        if (jobs_.empty()) return;  // stop requested and nothing left
        const auto job = jobs_.front();
        jobs_.pop_front();
        busy_ = true;
        lk.unlock();
        // (an exception on this thread would end the process: it becomes the queued commit's error)
        const int rc = ta::guarded(fail, ctx_, [&]() -> int {
            TA_CHECK(job.second > job.first ? stage_commit_now(ctx_, job.first, job.second) : TA_OK);
            if (ctx_->opt_lock_ahead) stage_lock_ahead(ctx_, job.second);
            return TA_OK;
        });
        lk.lock();
        if (rc && rc_ == TA_OK) {  // the first failure is the one reported
            std::lock_guard<std::mutex> el(g_err_m);
            rc_ = rc, err_ = ctx_->err;
        }
        busy_ = false;
        cv_.notify_all();
    }
}

int CommitQueue::flush() {
    if (!thread_.joinable()) return TA_OK;
    std::unique_lock<std::mutex> lk(m_);
    cv_.wait(lk, [&] { return jobs_.empty() && !busy_; });
    const int rc = rc_;
    if (!rc) return TA_OK;
    const std::string msg = err_;
    rc_ = TA_OK;
    lk.unlock();
    return fail(ctx_, rc, "queued ta_stage_commit: " + msg);
}

void CommitQueue::stop() {
    if (!thread_.joinable()) return;
    {
        std::lock_guard<std::mutex> lk(m_);
        stop_ = true;
    }
    cv_.notify_all();
    thread_.join();
    stop_ = false;
}

extern "C" {

int ta_stage_commit(ta_ctx* ctx, int64_t frame_lo, int64_t frame_hi) {
    return ta::guarded(fail, ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    if (ctx->st_nslabs == 0) return fail(ctx, TA_E_STATE, "ta_stage_alloc has not been called");
    TA_CHECK(check_not_compound(ctx));
    TA_CHECK(check_frames(ctx, frame_lo, frame_hi));
    if (!ctx->h_slabs[0]) return fail(ctx, TA_E_STATE, "device-only slabs: use ta_stage_commit_dev");
    if (frame_hi == frame_lo) return TA_OK;
    if (ctx->is_cpu) return TA_OK;  // the CPU backend reads the host slab in place
    if (ctx->opt_async_commit) {
        ctx->commits.push(frame_lo, frame_hi);
        return TA_OK;
    }
    TA_CHECK(ctx->commits.flush());
    return stage_commit_now(ctx, frame_lo, frame_hi);
    });
}

int ta_stage_commit_dev(ta_ctx* ctx, int slab, const void* d_src, int dtype, int64_t ld_row,
                        int64_t frame_lo, int64_t frame_hi, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    if (!ctx || !d_src) return fail(ctx, TA_E_INVALID, "null argument");
    TA_NO_CPU(ctx);
    TA_CHECK(check_slab(ctx, slab));
    TA_CHECK(check_not_compound(ctx));
    TA_CHECK(check_dtype(ctx, dtype));
    TA_CHECK(check_frames(ctx, frame_lo, frame_hi));
    TA_CHECK(check_ld_row(ctx, ld_row, ctx->st_A * ctx->st_D));
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    TA_CHECK(order_after_staging(ctx, (hipStream_t)stream));
    TA_HIP_TRY(ctx, launch_relayout(d_src, dtype == TA_F32, ld_row, ctx->st_A * ctx->st_D, frame_hi - frame_lo,
                                    ctx->d_slabs[slab], ctx->st_dev_f32, ctx->st_pitch, frame_lo,
                                    (hipStream_t)stream));
    return TA_OK;
    });
}

int ta_stage_synth(ta_ctx* ctx, int slab, uint64_t seed, int64_t col_offset, int64_t n_cols_total,
                   void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(check_slab(ctx, slab));
    if (col_offset < 0 || col_offset + ctx->st_A * ctx->st_D > n_cols_total)
        return fail(ctx, TA_E_INVALID, "column block outside the synthetic tensor");
    if (ctx->is_cpu) {  // the same generator into the host slab
        ta::cpu::synth(cpu_state(ctx), slab, seed, col_offset, n_cols_total);
        return TA_OK;
    }
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    TA_CHECK(order_after_staging(ctx, (hipStream_t)stream));
    TA_HIP_TRY(ctx, launch_synth(ctx->d_slabs[slab], ctx->st_dev_f32, ctx->st_pitch, ctx->st_A * ctx->st_D, ctx->st_T, seed,
                                 col_offset, n_cols_total, (hipStream_t)stream));
    return TA_OK;
    });
}

int ta_stage_read_dev(ta_ctx* ctx, int slab, double* d_dst, int64_t ld_row, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    if (!ctx || !d_dst) return fail(ctx, TA_E_INVALID, "null argument");
    TA_NO_CPU(ctx);
    TA_CHECK(check_slab(ctx, slab));
    TA_CHECK(check_ld_row(ctx, ld_row, ctx->st_A * ctx->st_D));
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    TA_CHECK(order_after_staging(ctx, (hipStream_t)stream));
    TA_HIP_TRY(ctx, launch_unlayout(ctx->d_slabs[slab], ctx->st_dev_f32, ctx->st_pitch, ctx->st_A * ctx->st_D, ctx->st_T, d_dst,
                                    ld_row, (hipStream_t)stream));
    return TA_OK;
    });
}

int ta_stage_device(ta_ctx* ctx, int slab, double** d_slab, int64_t* pitch_rows, int64_t* n_pairs) {
    return ta::guarded(fail, ctx, [&]() -> int {
    if (!ctx || !d_slab) return fail(ctx, TA_E_INVALID, "null argument");
    TA_NO_CPU(ctx);
    TA_CHECK(check_slab(ctx, slab));
    *d_slab = ctx->d_slabs[slab];
    if (pitch_rows) *pitch_rows = ctx->st_pitch;
    if (n_pairs) *n_pairs = (ctx->st_A * ctx->st_D + 1) / 2;
    return TA_OK;
    });
}

/* --------------------------------------------------------- device compute */
int ta_vacf_fft_dev(ta_ctx* ctx, const double* d_vel, int64_t T, int64_t A, int D, int64_t ld_row,
                    double* d_lagsum, double* d_bp, int64_t ld_bp, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return dev_entry(ctx, W_FFT, d_vel, nullptr, nullptr, T, A, D, ld_row, 1.0, d_lagsum, d_bp, ld_bp, stream);
    });
}

int ta_vacf_direct_dev(ta_ctx* ctx, const double* d_vel, int64_t T, int64_t A, int D, int64_t ld_row,
                       double* d_lagsum, double* d_bp, int64_t ld_bp, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return dev_entry(ctx, W_DIRECT, d_vel, nullptr, nullptr, T, A, D, ld_row, 1.0, d_lagsum, d_bp, ld_bp, stream);
    });
}

int ta_helfand_msd_dev(ta_ctx* ctx, const double* d_vel, const double* d_pos, const double* d_masses,
                       int64_t T, int64_t A, int D, int64_t ld_row, double scale, double* d_lagsum,
                       double* d_bp, int64_t ld_bp, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return dev_entry(ctx, W_HELFAND, d_vel, d_pos, d_masses, T, A, D, ld_row, scale, d_lagsum, d_bp, ld_bp, stream);
    });
}

int ta_vacf_fft_staged(ta_ctx* ctx, double* d_lagsum, double* d_bp, int64_t ld_bp, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return staged_entry(ctx, W_FFT, nullptr, 1.0, d_lagsum, d_bp, ld_bp, stream);
    });
}

int ta_vacf_direct_staged(ta_ctx* ctx, double* d_lagsum, double* d_bp, int64_t ld_bp, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return staged_entry(ctx, W_DIRECT, nullptr, 1.0, d_lagsum, d_bp, ld_bp, stream);
    });
}

int ta_helfand_msd_staged(ta_ctx* ctx, const double* d_masses, double scale, double* d_lagsum,
                          double* d_bp, int64_t ld_bp, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return staged_entry(ctx, W_HELFAND, d_masses, scale, d_lagsum, d_bp, ld_bp, stream);
    });
}

// Einstein MSD: slab 0 / d_pos holds the positions (the vel argument of the shared paths)
static int msd_which(int fft) { return fft ? W_MSD_FFT : W_MSD_DIRECT; }

int ta_msd_dev(ta_ctx* ctx, const double* d_pos, int64_t T, int64_t A, int D, int64_t ld_row, int fft, double* d_lagsum,
               double* d_bp, int64_t ld_bp, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    TA_CHECK(check_fft(ctx, fft));
    return dev_entry(ctx, msd_which(fft), d_pos, nullptr, nullptr, T, A, D, ld_row, 1.0, d_lagsum, d_bp, ld_bp, stream);
    });
}

int ta_msd_staged(ta_ctx* ctx, int fft, double* d_lagsum, double* d_bp, int64_t ld_bp, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    TA_CHECK(check_fft(ctx, fft));
    return staged_entry(ctx, msd_which(fft), nullptr, 1.0, d_lagsum, d_bp, ld_bp, stream);
    });
}

// The *_dev / *_staged pairs of the collective quantities: one body each on slab_entry; dev NULL = the staged slab.
// Einstein-Helfand conductivity: slab 0 / d_pos holds the positions
static int cond_entry(ta_ctx* ctx, const DevSrc* dev, int fft, const double* d_charges, double* d_moment, double* d_collective,
                      double* d_self_lagsum, void* stream) {
    return slab_entry(ctx, dev, stream, [&] { return cond_args(ctx, fft, d_charges, d_moment); }, no_pre, [&](const Slab& s) {
        return cond_pm(ctx, fft != 0, s, d_charges, d_moment, d_collective, d_self_lagsum);
    });
}
int ta_conductivity_dev(ta_ctx* ctx, const double* d_pos, int64_t T, int64_t A, int D, int64_t ld_row, int fft,
                        const double* d_charges, double* d_moment, double* d_collective, double* d_self_lagsum,
                        void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    const DevSrc src{d_pos, T, A, D, ld_row};
    return cond_entry(ctx, &src, fft, d_charges, d_moment, d_collective, d_self_lagsum, stream);
    });
}
int ta_conductivity_staged(ta_ctx* ctx, int fft, const double* d_charges, double* d_moment, double* d_collective,
                           double* d_self_lagsum, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return cond_entry(ctx, nullptr, fft, d_charges, d_moment, d_collective, d_self_lagsum, stream);
    });
}

// Onsager moments (slab 0 / d_pos holds the positions) and Green-Kubo currents (the velocities; the staged slab is read
// in its own element type, never widened); device labels are not checked (the pass skips an atom whose label is out of range)
static int coll_entry(ta_ctx* ctx, const Collective& q, const DevSrc* dev, int fft, int n_species, const int32_t* d_species,
                      const double* d_weights, double* d_sums, double* d_cross, void* stream) {
    return slab_entry(ctx, dev, stream, [&] { return coll_args(ctx, q, fft, n_species, d_species, d_sums); }, no_pre,
                      [&](const Slab& s) { return coll_pm(ctx, q, fft != 0, s, n_species, d_species, d_weights, d_sums, d_cross); });
}
int ta_onsager_dev(ta_ctx* ctx, const double* d_pos, int64_t T, int64_t A, int D, int64_t ld_row, int fft, int n_species,
                   const int32_t* d_species, const double* d_weights, double* d_moments, double* d_cross, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    const DevSrc src{d_pos, T, A, D, ld_row};
    return coll_entry(ctx, kCollective[COLL_MOMENTS], &src, fft, n_species, d_species, d_weights, d_moments, d_cross, stream);
    });
}
int ta_onsager_staged(ta_ctx* ctx, int fft, int n_species, const int32_t* d_species, const double* d_weights,
                      double* d_moments, double* d_cross, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return coll_entry(ctx, kCollective[COLL_MOMENTS], nullptr, fft, n_species, d_species, d_weights, d_moments, d_cross, stream);
    });
}
int ta_current_dev(ta_ctx* ctx, const double* d_vel, int64_t T, int64_t A, int D, int64_t ld_row, int fft, int n_species,
                   const int32_t* d_species, const double* d_weights, double* d_currents, double* d_cross, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    const DevSrc src{d_vel, T, A, D, ld_row};
    return coll_entry(ctx, kCollective[COLL_CURRENTS], &src, fft, n_species, d_species, d_weights, d_currents, d_cross, stream);
    });
}
int ta_current_staged(ta_ctx* ctx, int fft, int n_species, const int32_t* d_species, const double* d_weights,
                      double* d_currents, double* d_cross, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return coll_entry(ctx, kCollective[COLL_CURRENTS], nullptr, fft, n_species, d_species, d_weights, d_currents, d_cross, stream);
    });
}

// Species self terms: slab 0 / d_x holds the positions (TA_SELF_MSD) or the velocities (TA_SELF_VACF); the staged slab
// is read in its own element type (never widened); the labels are HOST arrays: the block sizes decide the launches, and
// self_plan runs before the call is opened
static int self_entry(ta_ctx* ctx, const DevSrc* dev, int quantity, int fft, int n_species, const int32_t* h_species,
                      const double* d_weights, double* d_self, void* stream) {
    SortPlan plan;
    return slab_entry(
        ctx, dev, stream, [&] { return self_args(ctx, quantity, fft, n_species, h_species, d_self); },
        [&](const Slab& s) { return self_plan(ctx, n_species, h_species, s.A, s.D, s.st, &plan); },
        [&](const Slab& s) { return species_self_pm(ctx, quantity, fft != 0, s, plan, d_weights, d_self); });
}
int ta_species_self_dev(ta_ctx* ctx, const double* d_x, int64_t T, int64_t A, int D, int64_t ld_row, int quantity, int fft,
                        int n_species, const int32_t* h_species, const double* d_weights, double* d_self, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    const DevSrc src{d_x, T, A, D, ld_row};
    return self_entry(ctx, &src, quantity, fft, n_species, h_species, d_weights, d_self, stream);
    });
}
int ta_species_self_staged(ta_ctx* ctx, int quantity, int fft, int n_species, const int32_t* h_species, const double* d_weights,
                           double* d_self, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return self_entry(ctx, nullptr, quantity, fft, n_species, h_species, d_weights, d_self, stream);
    });
}

// Intermediate scattering: slab 0 / d_pos holds the positions; the staged slab is read in its own element type (never
// widened); the wavevectors are a HOST array: they size the launches, and scatter_plan runs before the call is opened
static int scatter_entry(ta_ctx* ctx, const DevSrc* dev, int fft, int n_k, const double* h_kvecs, double* d_self,
                         double* d_density, double* d_coll, void* stream) {
    return slab_entry(
        ctx, dev, stream,
        [&] { return scatter_args(ctx, fft, n_k, h_kvecs, dev ? dev->D : ctx->st_nslabs ? ctx->st_D : 0, d_self, d_density, d_coll); },
        [&](const Slab& s) { return scatter_plan(ctx, n_k, h_kvecs, s.A, s.D, s.st); },
        [&](const Slab& s) { return scatter_pm(ctx, fft != 0, s, n_k, d_self, d_density, d_coll); });
}
int ta_scatter_dev(ta_ctx* ctx, const double* d_pos, int64_t T, int64_t A, int D, int64_t ld_row, int fft, int n_k,
                   const double* h_kvecs, double* d_self, double* d_density, double* d_coll, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    const DevSrc src{d_pos, T, A, D, ld_row};
    return scatter_entry(ctx, &src, fft, n_k, h_kvecs, d_self, d_density, d_coll, stream);
    });
}
int ta_scatter_staged(ta_ctx* ctx, int fft, int n_k, const double* h_kvecs, double* d_self, double* d_density, double* d_coll,
                      void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return scatter_entry(ctx, nullptr, fft, n_k, h_kvecs, d_self, d_density, d_coll, stream);
    });
}

// Orientational correlation functions: slab 0 / d_pos holds the positions (three columns per atom); the staged slab is read
// in its own element type (never widened); the index rows, the boxes and the weights are HOST arrays, checked and queued
// for upload before the call is opened
int ta_orient_dev(ta_ctx* ctx, const double* d_pos, int64_t T, int64_t A, int D, int64_t ld_row, int fft, int mode, int64_t n_vectors,
                  const int32_t* h_index, const double* h_dimensions, const double* h_weights, double* d_c1, double* d_c2,
                  double* d_total, double* d_coll, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    const DevSrc src{d_pos, T, A, D, ld_row};
    return orient_entry(ctx, &src, fft, mode, n_vectors, h_index, h_dimensions, h_weights, d_c1, d_c2, d_total, d_coll, stream, nullptr);
    });
}
int ta_orient_staged(ta_ctx* ctx, int fft, int mode, int64_t n_vectors, const int32_t* h_index, const double* h_dimensions,
                     const double* h_weights, double* d_c1, double* d_c2, double* d_total, double* d_coll, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return orient_entry(ctx, nullptr, fft, mode, n_vectors, h_index, h_dimensions, h_weights, d_c1, d_c2, d_total, d_coll, stream, nullptr);
    });
}

// Current correlation functions: slab 0 holds the velocities, slab 1 the positions, both read in the element type they have
// (never widened); the wavevectors are a HOST array, the weights a device one (or NULL); there is no frame-major entry
int ta_kcurrent_staged(ta_ctx* ctx, int fft, int n_k, const double* h_kvecs, const double* d_weights, double* d_current,
                       double* d_long, double* d_trans, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return slab_entry(
        ctx, nullptr, stream, [&] { return kcurrent_args(ctx, fft, n_k, h_kvecs, d_current, d_long, d_trans); },
        [&](const Slab& s) { return kcurrent_plan(ctx, n_k, h_kvecs, s.D, nullptr, 0, s.st); },
        [&](const Slab& s) { return kcurrent_pm(ctx, fft != 0, s, n_k, d_weights, d_current, d_long, d_trans); });
    });
}

// Partial scattering functions: slab 0 holds the positions, read in the element type it has (never widened); the wavevectors
// are a HOST array, the labels and weights device ones (weights or NULL); there is no frame-major entry
int ta_partial_density_staged(ta_ctx* ctx, int fft, int n_k, const double* h_kvecs, int n_species, const int32_t* d_species,
                              const double* d_weights, double* d_density, double* d_cross, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return slab_entry(
        ctx, nullptr, stream,
        [&]() -> int {
            TA_CHECK(partial_args(ctx, fft, n_k, h_kvecs, ctx->st_nslabs ? ctx->st_D : 0, n_species, d_species, d_density));
            return partial_slab(ctx);
        },
        [&](const Slab& s) { return partial_plan(ctx, n_k, h_kvecs, s.D, nullptr, 0, s.st); },
        [&](const Slab& s) { return partial_pm(ctx, fft != 0, s, n_k, n_species, d_species, d_weights, d_density, d_cross); });
    });
}

// Self van Hove function: slab 0 / d_pos holds the positions; the staged slab is read in its own element type (never
// widened); the lags are a HOST array: they size the launches, and vanhove_plan runs before the call is opened
static int vanhove_entry(ta_ctx* ctx, const DevSrc* dev, int n_lags, const int64_t* h_lags, int n_bins, double dr,
                         int64_t* d_counts, double* d_moments, void* stream) {
    return slab_entry(
        ctx, dev, stream,
        [&] { return check_vanhove(fail, ctx, n_lags, h_lags, n_bins, dr, dev ? dev->T : ctx->st_nslabs ? ctx->st_T : 0, d_counts || d_moments); },
        [&](const Slab& s) { return vanhove_plan(ctx, n_lags, h_lags, n_bins, dr, s.A, s.D, s.st); },
        [&](const Slab& s) { return vanhove_pm(ctx, s, n_lags, n_bins, dr, d_counts, d_moments); });
}
int ta_vanhove_dev(ta_ctx* ctx, const double* d_pos, int64_t T, int64_t A, int D, int64_t ld_row, int n_lags, const int64_t* h_lags,
                   int n_bins, double dr, int64_t* d_counts, double* d_moments, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    const DevSrc src{d_pos, T, A, D, ld_row};
    return vanhove_entry(ctx, &src, n_lags, h_lags, n_bins, dr, d_counts, d_moments, stream);
    });
}
int ta_vanhove_staged(ta_ctx* ctx, int n_lags, const int64_t* h_lags, int n_bins, double dr, int64_t* d_counts, double* d_moments,
                      void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return vanhove_entry(ctx, nullptr, n_lags, h_lags, n_bins, dr, d_counts, d_moments, stream);
    });
}

// Self-overlap per origin: slab 0 / d_pos holds the positions; the staged slab is read in its own element type (never
// widened); the lags and cutoffs are HOST arrays: they size the launches, and overlap_plan runs before the call is opened
static int overlap_entry(ta_ctx* ctx, const DevSrc* dev, int n_lags, const int64_t* h_lags, int n_cutoffs, const double* h_cutoffs,
                         int64_t* d_q, void* stream) {
    return slab_entry(
        ctx, dev, stream,
        [&] { return check_overlap(fail, ctx, n_lags, h_lags, n_cutoffs, h_cutoffs, dev ? dev->T : ctx->st_nslabs ? ctx->st_T : 0, d_q != nullptr); },
        [&](const Slab& s) { return overlap_plan(ctx, n_lags, h_lags, n_cutoffs, h_cutoffs, s.A, s.D, s.st); },
        [&](const Slab& s) { return overlap_pm(ctx, s, n_lags, n_cutoffs, d_q); });
}
int ta_overlap_dev(ta_ctx* ctx, const double* d_pos, int64_t T, int64_t A, int D, int64_t ld_row, int n_lags, const int64_t* h_lags,
                   int n_cutoffs, const double* h_cutoffs, int64_t* d_q, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    const DevSrc src{d_pos, T, A, D, ld_row};
    return overlap_entry(ctx, &src, n_lags, h_lags, n_cutoffs, h_cutoffs, d_q, stream);
    });
}
int ta_overlap_staged(ta_ctx* ctx, int n_lags, const int64_t* h_lags, int n_cutoffs, const double* h_cutoffs, int64_t* d_q,
                      void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return overlap_entry(ctx, nullptr, n_lags, h_lags, n_cutoffs, h_cutoffs, d_q, stream);
    });
}

// Overlap field's density per origin: the staged slab 0 holds the positions, read in its own element type (never widened);
// the wavevectors, lags and cutoffs are HOST arrays: they size the launches, and overlap_density_plan runs before the call
// is opened; there is no frame-major entry
int ta_overlap_density_staged(ta_ctx* ctx, int n_k, const double* h_kvecs, int n_lags, const int64_t* h_lags, int n_cutoffs,
                              const double* h_cutoffs, double* d_w, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    return slab_entry(
        ctx, nullptr, stream,
        [&] {
            return check_overlap_density(fail, ctx, n_k, h_kvecs, ctx->st_nslabs ? ctx->st_D : 0, n_lags, h_lags, n_cutoffs, h_cutoffs,
                                         ctx->st_nslabs ? ctx->st_T : 0, d_w != nullptr);
        },
        [&](const Slab& s) { return overlap_density_plan(ctx, n_k, h_kvecs, n_lags, h_lags, n_cutoffs, h_cutoffs, s.A, s.D, s.st); },
        [&](const Slab& s) { return overlap_density_pm(ctx, s, n_k, n_lags, n_cutoffs, d_w); });
    });
}

// Distinct van Hove function on the staged slab 0, read in its own element type; every list is a HOST array
int ta_vanhove_distinct_staged(ta_ctx* ctx, int n_lags, const int64_t* h_lags, int64_t origin_stride, int64_t n_a,
                               const int64_t* h_idx_a, int64_t n_b, const int64_t* h_idx_b, const double* h_dimensions, const int* axes,
                               int n_bins, double dr, int64_t* d_counts, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    const VhdArgs a{n_lags, n_bins, dr, origin_stride, n_a, n_b, h_lags, h_idx_a, h_idx_b, h_dimensions, axes};
    VhdPlan plan;
    TA_CHECK(need_ctx(ctx));
    TA_NO_CPU(ctx);
    TA_CHECK(vhd_args(ctx, a, ctx->st_nslabs ? ctx->st_T : 0, d_counts));
    TA_CHECK(check_staged(ctx));
    TA_CHECK(vhd_plan(ctx, a, ctx->st_T, ctx->st_A, ctx->st_D, &plan));
    return vhd_launch(ctx, plan, h_lags, dr, d_counts, stream, nullptr);
    });
}

// Pair lifetimes on the staged slab 0, read in its own element type; the pair list and the box are HOST arrays.  Bond
// lifetimes (bond != NULL) take the same path with k_bond_series (and k_pair_filter where needed)
static int life_staged(ta_ctx* ctx, int fft, int64_t n_rows, const int32_t* h_rows, const double* h_dimensions, const int* axes, double r_cut,
                       const BondArgs* bond, const LifePtrs& d, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    PairLifePlan plan;
    TA_CHECK(need_ctx(ctx));
    TA_NO_CPU(ctx);
    TA_CHECK(pair_life_plan(ctx, fft, n_rows, h_rows, h_dimensions, axes, r_cut, d.any(), &plan, bond));
    return pair_life_launch(ctx, fft, plan, d, stream, nullptr);
    });
}
int ta_pair_lifetime_staged(ta_ctx* ctx, int fft, int64_t n_pairs, const int32_t* h_pairs, const double* h_dimensions, const int* axes,
                            double r_cut, double* d_ci, int64_t* d_runs, double* d_nb, void* stream) {
    return life_staged(ctx, fft, n_pairs, h_pairs, h_dimensions, axes, r_cut, nullptr, {d_ci, nullptr, d_runs, d_nb}, stream);
}
int ta_bond_lifetime_staged(ta_ctx* ctx, int fft, int64_t n_bonds, int n_at, const int32_t* h_atoms, const double* h_dimensions,
                            const int* axes, double r_cut, double r_break, double cos_cut, double cos_break, int gap, double* d_ci,
                            int64_t* d_runs, double* d_nb, void* stream) {
    const BondArgs bond{n_at, r_break, cos_cut, cos_break, gap};
    return life_staged(ctx, fft, n_bonds, h_atoms, h_dimensions, axes, r_cut, &bond, {d_ci, nullptr, d_runs, d_nb}, stream);
}

// The shell calls on the staged slab 0, read in its own element type; the index lists, the box and (ta_shell_orient_staged)
// the index rows are HOST arrays, the outputs on the device
static int shell_staged(ta_ctx* ctx, ShellKind kind, int fft, const ShellArgs& a, const LifePtrs& d, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    ShellPlan plan;
    TA_CHECK(need_ctx(ctx));
    TA_NO_CPU(ctx);
    TA_CHECK(shell_plan(ctx, kind, fft, a, d.any(), &plan));
    return shell_launch(ctx, fft, plan, d, stream, nullptr);
    });
}
int ta_shell_residence_staged(ta_ctx* ctx, int fft, int64_t n_a, const int64_t* h_idx_a, int64_t n_b, const int64_t* h_idx_b,
                              const double* h_dimensions, const int* axes, double r_cut, double r_break, int gap, double* d_ci,
                              int64_t* d_runs, double* d_nb, void* stream) {
    return shell_staged(ctx, SHELL_RESIDENCE, fft, {n_a, n_b, h_idx_a, h_idx_b, h_dimensions, axes, r_cut, r_break, gap},
                        {d_ci, nullptr, d_runs, d_nb}, stream);
}
int ta_shell_msd_staged(ta_ctx* ctx, int condition, int64_t max_lag, int64_t n_a, const int64_t* h_idx_a, int64_t n_b,
                        const int64_t* h_idx_b, const double* h_dimensions, const int* axes, double r_cut, double r_break, int gap,
                        double* d_sums, int64_t* d_count, int64_t* d_runs, double* d_nb, void* stream) {
    return shell_staged(ctx, SHELL_MSD, 0, {n_a, n_b, h_idx_a, h_idx_b, h_dimensions, axes, r_cut, r_break, gap, condition, max_lag},
                        {d_sums, d_count, d_runs, d_nb}, stream);
}
int ta_chain_modes_staged(ta_ctx* ctx, int fft, int64_t n_chains, int64_t chain_len, const int32_t* h_members, int n_modes,
                           const double* h_coeff, const double* h_dimensions, double* d_acf, void* stream) {
    return ta::guarded(fail, ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    return chain_entry(ctx, ChainArgs{fft, n_chains, chain_len, h_members, n_modes, h_coeff, h_dimensions, d_acf}, d_acf, stream, nullptr);
    });
}

int ta_shell_orient_staged(ta_ctx* ctx, int condition, int64_t max_lag, int mode, int anchor, const int32_t* h_index, int64_t n_a,
                           const int64_t* h_idx_a, int64_t n_b, const int64_t* h_idx_b, const double* h_dimensions, const int* axes,
                           double r_cut, double r_break, int gap, double* d_sums, int64_t* d_count, int64_t* d_runs, double* d_nb,
                           void* stream) {
    return shell_staged(ctx, SHELL_ORIENT, 0,
                        {n_a, n_b, h_idx_a, h_idx_b, h_dimensions, axes, r_cut, r_break, gap, condition, max_lag, mode, anchor, h_index},
                        {d_sums, d_count, d_runs, d_nb}, stream);
}

int ta_last_timing(ta_ctx* ctx, float* total_ms, float* main_kernel_ms) {
    return ta::guarded(fail, ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    TA_NO_CPU(ctx);
    if (!ctx->timing_valid) return fail(ctx, TA_E_STATE, "no completed compute call to time");
    TA_HIP_TRY(ctx, hipEventSynchronize(ctx->ev[3]));
    float t = 0.f, m = 0.f;
    TA_HIP_TRY(ctx, hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[3]));
    TA_HIP_TRY(ctx, hipEventElapsedTime(&m, ctx->ev[1], ctx->ev[2]));
    if (total_ms) *total_ms = t;
    if (main_kernel_ms) *main_kernel_ms = m;
    return TA_OK;
    });
}

int ta_timing_history(ta_ctx* ctx, int max_n, float* total_ms, float* main_kernel_ms, int* n_out) {
    return ta::guarded(fail, ctx, [&]() -> int {
    if (!ctx || !n_out) return fail(ctx, TA_E_INVALID, "null argument");
    TA_NO_CPU(ctx);
    const long have = std::min<long>(ctx->n_calls, ta_ctx::kRing);
    const int n = (int)std::min<long>(have, std::max(0, max_n));
    for (int i = 0; i < n; ++i) {  // chronological: oldest of the last n first
        hipEvent_t* q = ctx->ring[(ctx->n_calls - n + i) % ta_ctx::kRing];
        TA_HIP_TRY(ctx, hipEventSynchronize(q[3]));
        float t = 0.f, m = 0.f;
        TA_HIP_TRY(ctx, hipEventElapsedTime(&t, q[0], q[3]));
        TA_HIP_TRY(ctx, hipEventElapsedTime(&m, q[1], q[2]));
        if (total_ms) total_ms[i] = t;
        if (main_kernel_ms) main_kernel_ms[i] = m;
    }
    *n_out = n;
    return TA_OK;
    });
}

int ta_clock_probe(ta_ctx* ctx, int n_launches, double* mhz, double* cycles_per_unit_pass, double* ms_per_launch) {
    return ta::guarded(fail, ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    TA_NO_CPU(ctx);
    TA_CHECK(check_staged(ctx));
    if (n_launches < 1) return fail(ctx, TA_E_INVALID, "need at least one launch");
    if (ctx->st_dev_f32) return fail(ctx, TA_E_UNSUPPORTED, "clock probe: float64 device slabs only");
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t T = ctx->st_T, n_pairs = (ctx->st_A * ctx->st_D + 1) / 2;
    int R0 = 0, R = 1;
    if (!wfft_choose((long)T, &R0, &R) || R != 1 || !(R0 == 8 || R0 == 10 || R0 == 12 || R0 == 16 || R0 == 20))
        return fail(ctx, TA_E_UNSUPPORTED, "clock probe: plans R0 = 8, 10, 12, 16, 20 without an outer radix only");
    cd* tw = nullptr;
    TA_CHECK(get_wf_table(ctx, R0, R, &tw));
    const int64_t cap = ctx->opt_fft_nwg > 0 ? ctx->opt_fft_nwg : (int64_t)ctx->n_cu * wfft_max_wg_per_cu(R0);
    const int64_t nwg = std::max<int64_t>(16, std::min<int64_t>(cap, 2 * n_pairs) / 16 * 16), n_tuples = nwg / 2;
    const int64_t L = 2L * R0 * 512;
    TA_CHECK(ensure(ctx, ctx->partial, sizeof(double) * (size_t)n_tuples * L));
    TA_CHECK(ensure(ctx, ctx->clock_stamps, sizeof(unsigned long long) * 16 * (size_t)nwg));
    unsigned long long* stamps = (unsigned long long*)ctx->clock_stamps.p;
    TA_CHECK(order_after_staging(ctx, ctx->stream));
    hipEvent_t e0 = nullptr, e1 = nullptr;  // its own events: the probe is not a compute call and leaves the timing ring alone
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, ctx->stream);
    for (int i = 0; i < n_launches && e == hipSuccess; ++i)
        e = launch_wfft_forward_stamp(R0, (int)nwg, ctx->stream, ctx->d_slabs[0], ctx->st_pitch, (int)T, n_pairs, tw,
                                      (double*)ctx->partial.p, stamps);
    if (e == hipSuccess) e = hipEventRecord(e1, ctx->stream);
    std::vector<unsigned long long> h(16 * (size_t)nwg);
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), stamps, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return fail(ctx, TA_E_HIP, std::string("clock probe: ") + hipGetErrorString(e));
    // the last launch's stamps, wave 0 of every workgroup: [0] S1, [1] S2 cycles, [2] the kernel's span
    // in shader cycles, [3] in 100 MHz ticks
    double cyc = 0.0, span = 0.0, ticks = 0.0;
    for (int64_t w = 0; w < nwg; ++w) {
        cyc += (double)h[16 * w + 0] + (double)h[16 * w + 1];
        span += (double)h[16 * w + 2];
        ticks += (double)h[16 * w + 3];
    }
    const double unit_passes = 2.0 * (double)n_pairs;  // every pair in both passes, over all workgroups
    if (mhz) *mhz = ticks > 0 ? span / ticks * 100.0 : 0.0;
    if (cycles_per_unit_pass) *cycles_per_unit_pass = cyc / unit_passes;
    if (ms_per_launch) *ms_per_launch = ms / n_launches;
    return TA_OK;
    });
}

int ta_kernel_timeline(ta_ctx* ctx, int max_n, const char** names, float* ms, int* n_out) {
    return ta::guarded(fail, ctx, [&]() -> int {
    if (!ctx || !n_out) return fail(ctx, TA_E_INVALID, "null argument");
    TA_NO_CPU(ctx);
    *n_out = 0;
    if (ctx->marks.size() < 2) return TA_OK;  // option off, or no call yet
    TA_HIP_TRY(ctx, hipEventSynchronize(ctx->marks.back().ev));
    std::vector<std::pair<const char*, float>> agg;  // by name, in order of first appearance
    for (size_t i = 0; i + 1 < ctx->marks.size(); ++i) {
        float d = 0.f;
        TA_HIP_TRY(ctx, hipEventElapsedTime(&d, ctx->marks[i].ev, ctx->marks[i + 1].ev));
        size_t j = 0;
        while (j < agg.size() && strcmp(agg[j].first, ctx->marks[i].name)) ++j;
        if (j == agg.size()) agg.push_back({ctx->marks[i].name, 0.f});
        agg[j].second += d;
    }
    const int n = (int)std::min<size_t>(agg.size(), (size_t)std::max(0, max_n));
    for (int i = 0; i < n; ++i) {
        if (names) names[i] = agg[i].first;
        if (ms) ms[i] = agg[i].second;
    }
    *n_out = n;
    return TA_OK;
    });
}

int ta_kernel_launches(ta_ctx* ctx, const char* name, int* n_out) {
    return ta::guarded(fail, ctx, [&]() -> int {
    if (!ctx || !name || !n_out) return fail(ctx, TA_E_INVALID, "null argument");
    TA_NO_CPU(ctx);
    int n = 0;
    for (size_t i = 0; i + 1 < ctx->marks.size(); ++i) n += !strcmp(ctx->marks[i].name, name);
    *n_out = n;
    return TA_OK;
    });
}

/* ------------------------------------------------- host-facing (blocking) */
}  // extern "C"

namespace ta {
// One context's share of a host-facing call, queued but not waited for: compute on the staged
// slabs, by-particle blocks copied into the caller's host array (row stride ld_host elements: the
// caller's array may be wider than this context's block of atoms -- the column range of one GPU
// in a multi-device group), and the lag-indexed SUM over this context's atoms left on the device
// in *d_total ((n_frames,) float64, valid once host_wait has returned or for work queued behind it
// on ctx->stream).  h_masses: this context's atoms.
int host_launch(ta_ctx* ctx, int which, const double* h_masses, double scale, double* h_bp, int64_t ld_host,
                double** d_total) {
    TA_CHECK(need_ctx(ctx));
    TA_NO_CPU(ctx);
    const int need = slabs_needed(which);
    TA_CHECK(check_staged(ctx, need));
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t T = ctx->st_T, A = ctx->st_A;
    if (h_bp && ld_host < A) return fail(ctx, TA_E_INVALID, "host row stride smaller than n_atoms");
    // With a by-particle array the device->host copy (8 GB at 10000 x 100000) is several times
    // the compute: atoms go in blocks, the copy of block c (a strided 2-D copy into the caller's
    // (n_frames, ld_host) array, on a second stream) runs under the compute of block c + 1.
    const int64_t CH = ctx->opt_bp_block > 0 ? (ctx->opt_bp_block + 63) / 64 * 64 : 16384;
    const bool blocked = h_bp && A >= 2 * CH;
    const int64_t n_blocks = blocked ? (A + CH - 1) / CH : 1;
    // rows [0, n_blocks): per-block lag sums; row n_blocks: their sum (one block: row 0 is the sum)
    TA_CHECK(ensure(ctx, ctx->out_lagsum, sizeof(double) * T * (n_blocks + 1)));
    double* d_ls = (double*)ctx->out_lagsum.p;
    double* d_bp = nullptr;
    if (h_bp) {
        TA_CHECK(ensure(ctx, ctx->out_bp, sizeof(double) * (size_t)T * A));
        d_bp = (double*)ctx->out_bp.p;
    }
    const double* d_m = nullptr;
    if (which == W_HELFAND) {
        if (!h_masses) return fail(ctx, TA_E_INVALID, "h_masses is NULL");
        TA_CHECK(ensure(ctx, ctx->masses, sizeof(double) * A));
        TA_HIP_TRY(ctx, hipMemcpyAsync(ctx->masses.p, h_masses, sizeof(double) * A, hipMemcpyHostToDevice,
                                       ctx->stream));
        d_m = (const double*)ctx->masses.p;
    }
    if (!blocked) {
        TA_CHECK(staged_entry(ctx, which, d_m, scale, d_ls, d_bp, A, (void*)ctx->stream));
        if (h_bp)
            TA_HIP_TRY(ctx, hipMemcpy2DAsync(h_bp, sizeof(double) * ld_host, d_bp, sizeof(double) * A,
                                             sizeof(double) * A, T, hipMemcpyDeviceToHost, ctx->stream));
        *d_total = d_ls;
        return TA_OK;
    }
    if (!ctx->copy_stream) TA_HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    // the blocks go to compute_pm directly (staged_entry is not on this path): join the commit worker here, or the
    // first block is queued ahead of frames whose copies the worker has not issued yet
    TA_CHECK(order_after_staging(ctx, ctx->stream));
    const int D = ctx->st_D;
    for (int64_t b = 0; b < n_blocks; ++b) {
        const int64_t lo = b * CH, hi = std::min(A, lo + CH);
        const int64_t pair_lo = lo * D / 2;  // lo is a multiple of 64: a pair boundary
        const size_t off = (size_t)pair_lo * ctx->st_pitch * (ctx->st_dev_f32 ? 8 : 16);  // bytes
        const void* v = (const char*)ctx->d_slabs[0] + off;
        const void* x = need == 2 ? (const char*)ctx->d_slabs[1] + off : nullptr;
        TA_CHECK(call_begin(ctx, ctx->stream));
        TA_CHECK(compute_pm(ctx, which, v, x, d_m ? d_m + lo : nullptr, ctx->st_pitch, T, hi - lo, D, scale,
                            d_ls + b * T, d_bp + lo, A, ctx->stream, ctx->st_dev_f32));
        TA_HIP_TRY(ctx, hipEventRecord(ctx->ev_stage, ctx->stream));
        TA_HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_stage, 0));
        TA_HIP_TRY(ctx, hipMemcpy2DAsync(h_bp + lo, sizeof(double) * ld_host, d_bp + lo, sizeof(double) * A,
                                         sizeof(double) * (hi - lo), T, hipMemcpyDeviceToHost,
                                         ctx->copy_stream));
    }
    // the blocks' lag sums, added on the device in a fixed order
    TA_HIP_TRY(ctx, launch_sum_partials(d_ls, (int)n_blocks, T, d_ls + n_blocks * T, ctx->stream));
    *d_total = d_ls + n_blocks * T;
    return TA_OK;
}

// Conductivity share of a host-facing call, queued on ctx->stream and not waited for: charges (this context's atoms)
// uploaded, the moment (and with self the self lag sum, with coll Phi) left on the device in *d_out, laid out by cond_out
int cond_launch(ta_ctx* ctx, int fft, const double* h_q, bool coll, bool self, double** d_out) {
    return slab_entry(
        ctx, nullptr, ctx->stream, no_args,
        [&](const Slab& s) -> int {
            TA_CHECK(ensure(ctx, ctx->cond_q, sizeof(double) * s.A));
            TA_CHECK(out_buffer(ctx, ctx->cond_out, cond_out(s.T, s.D), d_out));
            TA_HIP_TRY(ctx, hipMemcpyAsync(ctx->cond_q.p, h_q, sizeof(double) * s.A, hipMemcpyHostToDevice, ctx->stream));
            return TA_OK;
        },
        [&](const Slab& s) {
            const OutLayout o = cond_out(s.T, s.D);
            return cond_pm(ctx, fft != 0, s, (const double*)ctx->cond_q.p, o.at(*d_out, 0), o.at(*d_out, 1, coll), o.at(*d_out, 2, self));
        });
}

// Phi of a host (T, D) moment on this context's device, blocking (the group's collective after its members' sums)
int cond_collective_host(ta_ctx* ctx, int fft, const double* h_moment, int64_t T, int D, double* h_coll) {
    const OutLayout o = cond_out(T, D);
    double* out = nullptr;
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    TA_CHECK(out_buffer(ctx, ctx->cond_out, o, &out));
    TA_CHECK(upload_segment(ctx, o, out, 0, h_moment, ctx->stream));
    TA_CHECK(cond_collective(ctx, fft != 0, o.at(out, 0), T, D, o.at(out, 1), ctx->stream));
    return out_finish(ctx, o, out, {nullptr, h_coll});
}

// Moments' / currents' share of a host-facing call, queued on ctx->stream and not waited for: the labels and weights (this
// context's atoms, labels already checked) uploaded, the sums and with cross the cross term left on the device in *d_out,
// laid out by coll_out (the Onsager buffers serve both quantities: one call at a time uses them).
int coll_launch(ta_ctx* ctx, int kind, int fft, int S, const int32_t* h_species, const double* h_w, bool cross, double** d_out) {
    return slab_entry(
        ctx, nullptr, ctx->stream, no_args,
        [&](const Slab& s) -> int {
            TA_CHECK(ensure(ctx, ctx->ons_lab, sizeof(int32_t) * s.A));
            if (h_w) TA_CHECK(ensure(ctx, ctx->ons_w, sizeof(double) * s.A));
            TA_CHECK(out_buffer(ctx, ctx->ons_out, coll_out(S, s.T, s.D), d_out));
            TA_HIP_TRY(ctx, hipMemcpyAsync(ctx->ons_lab.p, h_species, sizeof(int32_t) * s.A, hipMemcpyHostToDevice, ctx->stream));
            if (h_w) TA_HIP_TRY(ctx, hipMemcpyAsync(ctx->ons_w.p, h_w, sizeof(double) * s.A, hipMemcpyHostToDevice, ctx->stream));
            return TA_OK;
        },
        [&](const Slab& s) {
            const OutLayout o = coll_out(S, s.T, s.D);
            return coll_pm(ctx, kCollective[kind], fft != 0, s, S, (const int32_t*)ctx->ons_lab.p,
                           h_w ? (const double*)ctx->ons_w.p : nullptr, o.at(*d_out, 0), o.at(*d_out, 1, cross));
        });
}

// A correlation of host sums on this context's device, blocking, as a compute call of its own (the *_cross and
// *_collective entries; a group's ONE evaluation after its members' sums).  Needs no staged slab.  upload(st): the
// workspaces ensured, the sums queued for upload into their segment of the call's layout; body(st): the correlation,
// inside the call's bracket (no dominant kernel of its own, unless the correlator records one).  The caller's out_finish
// copies the correlation's segments to the host.
template <class Upload, class Body>
int host_sums_call(ta_ctx* ctx, Upload&& upload, Body&& body) {
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    TA_CHECK(ctx->commits.flush());
    hipStream_t st = ctx->stream;
    TA_CHECK(upload(st));
    TA_CHECK(call_begin(ctx, st));
    TA_HIP_TRY(ctx, hipEventRecord(ctx->ev[1], st));
    TA_HIP_TRY(ctx, hipEventRecord(ctx->ev[2], st));
    TA_CHECK(body(st));
    return call_end(ctx, st);
}
// The cross term of host sums (ta_onsager_cross, ta_current_cross)
int coll_cross_host(ta_ctx* ctx, int kind, int fft, const double* h_sums, int S, int64_t T, int D, double* h_cross) {
    const OutLayout o = coll_out(S, T, D);
    double* out = nullptr;
    TA_CHECK(host_sums_call(
        ctx,
        [&](hipStream_t st) -> int {
            TA_CHECK(out_buffer(ctx, ctx->ons_out, o, &out));
            return upload_segment(ctx, o, out, 0, h_sums, st);
        },
        [&](hipStream_t st) { return coll_cross(ctx, kCollective[kind], fft != 0, o.at(out, 0), S, T, D, o.at(out, 1), st); }));
    return out_finish(ctx, o, out, {nullptr, h_cross});
}

// Self-term share of a host-facing call, queued on ctx->stream and not waited for: the labels (this context's atoms)
// checked and sorted, the weights uploaded (the Onsager weight buffer: one call at a time uses it), the lag sums left on
// the device in *d_out (self_out); h_counts (S) or NULL: this context's atoms per species.
int self_launch(ta_ctx* ctx, int quantity, int fft, int S, const int32_t* h_species, const double* h_w, int64_t* h_counts,
                double** d_out) {
    SortPlan plan;
    TA_CHECK(slab_entry(
        ctx, nullptr, ctx->stream, no_args,
        [&](const Slab& s) -> int {
            TA_CHECK(self_plan(ctx, S, h_species, s.A, s.D, ctx->stream, &plan));
            if (h_w) TA_CHECK(ensure(ctx, ctx->ons_w, sizeof(double) * s.A));
            TA_CHECK(out_buffer(ctx, ctx->self_out, self_out(S, s.T), d_out));
            if (h_w) TA_HIP_TRY(ctx, hipMemcpyAsync(ctx->ons_w.p, h_w, sizeof(double) * s.A, hipMemcpyHostToDevice, ctx->stream));
            return TA_OK;
        },
        [&](const Slab& s) { return species_self_pm(ctx, quantity, fft != 0, s, plan, h_w ? (const double*)ctx->ons_w.p : nullptr, *d_out); }));
    if (h_counts)
        for (int s = 0; s < S; ++s) h_counts[s] = plan.count[s];
    return TA_OK;
}

// Scattering share of a host-facing call, queued on ctx->stream and not waited for: the wavevectors (checked by the
// caller) uploaded, the outputs asked for left on the device in *d_out, laid out by scatter_out
int scatter_launch(ta_ctx* ctx, int fft, int K, const double* h_kvecs, bool self, bool density, bool coll, double** d_out) {
    return slab_entry(
        ctx, nullptr, ctx->stream, no_args,
        [&](const Slab& s) -> int {
            TA_CHECK(scatter_plan(ctx, K, h_kvecs, s.A, s.D, ctx->stream));
            return out_buffer(ctx, ctx->scatter_out, scatter_out(K, s.T), d_out);
        },
        [&](const Slab& s) {
            const OutLayout o = scatter_out(K, s.T);
            return scatter_pm(ctx, fft != 0, s, K, o.at(*d_out, 0, self), o.at(*d_out, 1, density), o.at(*d_out, 2, coll));
        });
}

// Van Hove share of a host-facing call, queued on ctx->stream and not waited for: the lags and bins (checked by the caller)
// uploaded, the outputs asked for left on the device in *d_out, laid out by vanhove_out
int vanhove_launch(ta_ctx* ctx, int L, const int64_t* h_lags, int B, double dr, bool counts, bool moments, double** d_out) {
    const OutLayout o = vanhove_out(L, B);
    return slab_entry(
        ctx, nullptr, ctx->stream, no_args,
        [&](const Slab& s) -> int {
            TA_CHECK(vanhove_plan(ctx, L, h_lags, B, dr, s.A, s.D, ctx->stream));
            return out_buffer(ctx, ctx->vh_out, o, d_out);
        },
        [&](const Slab& s) { return vanhove_pm(ctx, s, L, B, dr, (int64_t*)o.at(*d_out, 0, counts), o.at(*d_out, 1, moments)); });
}

// Overlap share of a host-facing call, queued on ctx->stream and not waited for: the lags and cutoffs (checked by the caller)
// uploaded, Q left on the device in *d_out (overlap_out)
int overlap_launch(ta_ctx* ctx, int L, const int64_t* h_lags, int C, const double* h_cutoffs, double** d_out) {
    return slab_entry(
        ctx, nullptr, ctx->stream, no_args,
        [&](const Slab& s) -> int {
            TA_CHECK(overlap_plan(ctx, L, h_lags, C, h_cutoffs, s.A, s.D, ctx->stream));
            return out_buffer(ctx, ctx->ov_out, overlap_out(C, L, s.T), d_out);
        },
        [&](const Slab& s) { return overlap_pm(ctx, s, L, C, (int64_t*)*d_out); });
}

// Overlap-density share of a host-facing call, queued on ctx->stream and not waited for: the wavevectors, lags and cutoffs
// (checked by the caller) uploaded, W left on the device in *d_out (overlap_density_out)
int overlap_density_launch(ta_ctx* ctx, int K, const double* h_kvecs, int L, const int64_t* h_lags, int C, const double* h_cutoffs,
                           double** d_out) {
    return slab_entry(
        ctx, nullptr, ctx->stream, no_args,
        [&](const Slab& s) -> int {
            TA_CHECK(overlap_density_plan(ctx, K, h_kvecs, L, h_lags, C, h_cutoffs, s.A, s.D, ctx->stream));
            return out_buffer(ctx, ctx->od_out, overlap_density_out(K, C, L, s.T), d_out);
        },
        [&](const Slab& s) { return overlap_density_pm(ctx, s, K, L, C, *d_out); });
}

// The collective part (K, T) of a host (K, T, 2) density (ta_scatter_collective)
int scatter_collective_host(ta_ctx* ctx, int fft, const double* h_density, int K, int64_t T, double* h_coll) {
    const OutLayout o = scatter_out(K, T);
    double* out = nullptr;
    TA_CHECK(host_sums_call(
        ctx,
        [&](hipStream_t st) -> int {
            TA_CHECK(out_buffer(ctx, ctx->scatter_out, o, &out));
            TA_CHECK(ensure(ctx, ctx->scatter_work, scatter_work_bytes(T, K, false)));
            return upload_segment(ctx, o, out, 1, h_density, st);
        },
        [&](hipStream_t st) { return scatter_collective(ctx, fft != 0, o.at(out, 1), K, T, o.at(out, 2), st); }));
    return out_finish(ctx, o, out, {nullptr, nullptr, h_coll});
}

// Current-correlation share of a host-facing call, queued on ctx->stream and not waited for: the table (wavevectors, checked
// by the caller, and this context's atoms' weights) uploaded, the current and (correlate) long and trans left on the device in
// *d_out, laid out by kcurrent_out
int kcurrent_launch(ta_ctx* ctx, int fft, int K, const double* h_kvecs, const double* h_w, bool correlate, double** d_out) {
    return slab_entry(
        ctx, nullptr, ctx->stream, [&] { return kcurrent_slabs(ctx); },
        [&](const Slab& s) -> int {
            TA_CHECK(kcurrent_plan(ctx, K, h_kvecs, s.D, h_w, s.A, ctx->stream));
            return out_buffer(ctx, ctx->kcur_out, kcurrent_out(K, s.T, s.D), d_out);
        },
        [&](const Slab& s) {
            const OutLayout o = kcurrent_out(K, s.T, s.D);
            const double* d_w = h_w ? (const double*)ctx->kcur_tab.dev.p + 2 * (size_t)K * s.D : nullptr;
            return kcurrent_pm(ctx, fft != 0, s, K, d_w, o.at(*d_out, 0), o.at(*d_out, 1, correlate), o.at(*d_out, 2, correlate));
        });
}

// long and trans of a host current (ta_kcurrent_correlate)
int kcurrent_correlate_host(ta_ctx* ctx, int fft, const double* h_current, int K, const double* h_kvecs, int64_t T, int D,
                            double* h_long, double* h_trans) {
    const OutLayout o = kcurrent_out(K, T, D);
    double* out = nullptr;
    TA_CHECK(host_sums_call(
        ctx,
        [&](hipStream_t st) -> int {
            TA_CHECK(out_buffer(ctx, ctx->kcur_out, o, &out));
            TA_CHECK(ensure(ctx, ctx->kcur_work, kcurrent_work_bytes(T, K, D, false)));
            TA_CHECK(kcurrent_plan(ctx, K, h_kvecs, D, nullptr, 0, st));
            return upload_segment(ctx, o, out, 0, h_current, st);
        },
        [&](hipStream_t st) { return kcurrent_correlation(ctx, fft != 0, o.at(out, 0), K, T, D, o.at(out, 1), o.at(out, 2), st); }));
    return out_finish(ctx, o, out, {nullptr, h_long, h_trans});
}

// Partial-density share of a host-facing call, queued on ctx->stream and not waited for: the table (wavevectors, checked by
// the caller, and this context's atoms' weights) and the labels (checked by the caller) uploaded, the density and (cross) the
// cross term left on the device in *d_out, laid out by partial_out
int partial_launch(ta_ctx* ctx, int fft, int K, const double* h_kvecs, int S, const int32_t* h_species, const double* h_w,
                   bool cross, double** d_out) {
    return slab_entry(
        ctx, nullptr, ctx->stream, [&] { return partial_slab(ctx); },
        [&](const Slab& s) -> int {
            TA_CHECK(partial_plan(ctx, K, h_kvecs, s.D, h_w, s.A, ctx->stream));
            TA_CHECK(ensure(ctx, ctx->psd_lab, sizeof(int32_t) * (size_t)s.A));
            TA_CHECK(out_buffer(ctx, ctx->psd_out, partial_out(K, S, s.T), d_out));
            TA_HIP_TRY(ctx, hipMemcpyAsync(ctx->psd_lab.p, h_species, sizeof(int32_t) * s.A, hipMemcpyHostToDevice, ctx->stream));
            return TA_OK;
        },
        [&](const Slab& s) {
            const OutLayout o = partial_out(K, S, s.T);
            const double* d_w = h_w ? (const double*)ctx->psd_tab.dev.p + (size_t)K * s.D : nullptr;
            return partial_pm(ctx, fft != 0, s, K, S, (const int32_t*)ctx->psd_lab.p, d_w, o.at(*d_out, 0), o.at(*d_out, 1, cross));
        });
}

// The cross term of a host density (ta_partial_cross)
int partial_cross_host(ta_ctx* ctx, int fft, const double* h_density, int K, int S, int64_t T, double* h_cross) {
    const OutLayout o = partial_out(K, S, T);
    double* out = nullptr;
    TA_CHECK(host_sums_call(
        ctx,
        [&](hipStream_t st) -> int {
            TA_CHECK(out_buffer(ctx, ctx->psd_out, o, &out));
            return upload_segment(ctx, o, out, 0, h_density, st);
        },
        [&](hipStream_t st) { return partial_cross(ctx, fft != 0, o.at(out, 0), K, S, T, o.at(out, 1), st); }));
    return out_finish(ctx, o, out, {nullptr, h_cross});
}

// One context's unwrap of staged slab `slab` (ta_unwrap, ta_group_unwrap), queued on ctx->stream behind the queued commits
// and bracketed by the timing events: the box table's copy (box.tab must stay valid until host_wait), then the kernel
int unwrap_launch(ta_ctx* ctx, int slab, const BoxTable& box, const int* axes) {
    TA_CHECK(check_slab(ctx, slab));
    if (ctx->st_dev_f32) return fail(ctx, TA_E_UNSUPPORTED, "unwrap: float64 device slabs only (stage_device_f32 is on)");
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    TA_CHECK(order_after_staging(ctx, ctx->stream));
    const size_t bytes = box.tab.size() * sizeof(double);
    TA_CHECK(ensure(ctx, ctx->unwrap_box, bytes));
    hipStream_t st = ctx->stream;
    TA_CHECK(call_begin(ctx, st));
    TA_LAUNCH(ctx, "box_copy", st, hipMemcpyAsync(ctx->unwrap_box.p, box.tab.data(), bytes, hipMemcpyHostToDevice, st));
    TA_LAUNCH_MAIN(ctx, box.triclinic ? "k_unwrap_tric" : "k_unwrap_ortho", st,
                   launch_unwrap(ctx->d_slabs[slab], (long)ctx->st_pitch, (long)ctx->st_T, (long)ctx->st_A, ctx->st_D, axes,
                                 box.triclinic, box.per_frame, (const double*)ctx->unwrap_box.p, (long)box.tpitch, st));
    return call_end(ctx, st);
}
int host_wait(ta_ctx* ctx) {
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    TA_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->copy_stream) TA_HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
    return TA_OK;
}
// the tail of a host-facing call: the small results (n doubles each; a NULL destination is skipped) copied back on the
// context's stream, then everything the call queued waited for
int host_finish(ta_ctx* ctx, std::initializer_list<HostCopy> copies) {
    for (const HostCopy& c : copies)
        if (c.h) TA_HIP_TRY(ctx, hipMemcpyAsync(c.h, c.d, sizeof(double) * c.n, hipMemcpyDeviceToHost, ctx->stream));
    return host_wait(ctx);
}
hipStream_t ctx_stream(ta_ctx* ctx) { return ctx->stream; }
int ctx_device(const ta_ctx* ctx) { return ctx->device; }
int64_t ctx_staged_frames(const ta_ctx* ctx) { return ctx->st_nslabs ? ctx->st_T : 0; }
int ctx_fail(ta_ctx* ctx, int code, const std::string& msg) { return fail(ctx, code, msg); }
int ctx_host_slab(ta_ctx* ctx, int slab, void** h, int64_t* T, int64_t* A, int* D, int* dtype) {
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(check_slab(ctx, slab));
    TA_CHECK(check_not_compound(ctx));
    if (!ctx->h_slabs[slab]) return fail(ctx, TA_E_STATE, "device-only slabs have no host side to fill");
    *h = ctx->h_slabs[slab], *T = ctx->st_T, *A = ctx->st_A, *D = ctx->st_D, *dtype = ctx->st_dtype;
    return TA_OK;
}
}  // namespace ta

// The shape of every host-facing (blocking) entry: the body runs under a reporter that waits before it reports -- an
// exception after the launch lets the queued kernels and the copies into the caller's arrays finish before the error
// returns, so the caller may free its arrays at once -- and ends in host_finish.
template <class Body>
static int host_call(ta_ctx* ctx, Body&& body) {
    return ta::guard(
        [&](int code, const std::string& msg) {
            if (ctx && !ctx->is_cpu) (void)host_wait(ctx);
            return fail(ctx, code, msg);
        },
        body);
}

extern "C" {

static int host_compute(ta_ctx* ctx, int which, const double* h_masses, double scale,
                        double* h_ts, double* h_bp) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    if (!h_ts) return fail(ctx, TA_E_INVALID, "h_timeseries is NULL");
    if (ctx->is_cpu) return cpu_compute(ctx, which, h_masses, scale, h_ts, h_bp);
    double* d_total = nullptr;
    TA_CHECK(host_launch(ctx, which, h_masses, scale, h_bp, ctx->st_A, &d_total));
    TA_CHECK(host_finish(ctx, {{h_ts, d_total, (size_t)ctx->st_T}}));
    atom_mean(ctx, h_ts);
    return TA_OK;
    });
}

int ta_vacf_fft(ta_ctx* ctx, double* h_ts, double* h_bp) { return host_compute(ctx, W_FFT, nullptr, 1.0, h_ts, h_bp); }
int ta_vacf_direct(ta_ctx* ctx, double* h_ts, double* h_bp) { return host_compute(ctx, W_DIRECT, nullptr, 1.0, h_ts, h_bp); }
int ta_helfand_msd(ta_ctx* ctx, const double* h_masses, double scale, double* h_ts, double* h_bp) {
    return host_compute(ctx, W_HELFAND, h_masses, scale, h_ts, h_bp);
}
int ta_msd(ta_ctx* ctx, int fft, double* h_ts, double* h_bp) {
    TA_CHECK(check_fft(ctx, fft));
    return host_compute(ctx, msd_which(fft), nullptr, 1.0, h_ts, h_bp);
}

int ta_conductivity(ta_ctx* ctx, int fft, const double* h_charges, double* h_moment, double* h_collective,
                    double* h_self_lagsum) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(cond_args(ctx, fft, h_charges, h_moment));
    TA_CHECK(check_staged(ctx));
    if (ctx->is_cpu) return cpu_conductivity(ctx, fft != 0, h_charges, h_moment, h_collective, h_self_lagsum);
    double* d_out = nullptr;
    TA_CHECK(ta::cond_launch(ctx, fft, h_charges, h_collective != nullptr, h_self_lagsum != nullptr, &d_out));
    return out_finish(ctx, cond_out(ctx->st_T, ctx->st_D), d_out, {h_moment, h_collective, h_self_lagsum});
    });
}

// ta_onsager / ta_current, and ta_onsager_cross / ta_current_cross: one body each
static int coll_host(ta_ctx* ctx, int kind, int fft, int n_species, const int32_t* h_species, const double* h_weights,
                     double* h_sums, double* h_cross) {
    return host_call(ctx, [&]() -> int {
    const Collective& q = kCollective[kind];
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(coll_args(ctx, q, fft, n_species, h_species, h_sums));
    TA_CHECK(check_staged(ctx));
    TA_CHECK(check_labels(fail, ctx, h_species, ctx->st_A, n_species));
    if (ctx->is_cpu) return cpu_rc(ctx, q.cpu(cpu_state(ctx), fft != 0, n_species, h_species, h_weights, h_sums, h_cross));
    double* d_out = nullptr;
    TA_CHECK(ta::coll_launch(ctx, kind, fft, n_species, h_species, h_weights, h_cross != nullptr, &d_out));
    return out_finish(ctx, coll_out(n_species, ctx->st_T, ctx->st_D), d_out, {h_sums, h_cross});
    });
}
static int coll_cross_call(ta_ctx* ctx, int kind, int fft, const double* h_sums, int n_species, int64_t n_frames, int dim,
                           double* h_cross) {
    return host_call(ctx, [&]() -> int {
    const Collective& q = kCollective[kind];
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(check_fft(ctx, fft));
    TA_CHECK(check_species_count(fail, ctx, n_species));
    if (!h_sums || !h_cross) return fail(ctx, TA_E_INVALID, std::string(q.noun) + " or cross output is NULL");
    TA_CHECK(check_sums_shape(ctx, n_frames, &dim));
    if (ctx->is_cpu) return cpu_rc(ctx, q.cpu_cross(ctx->cpu_threads, fft != 0, h_sums, n_species, n_frames, dim, h_cross));
    return ta::coll_cross_host(ctx, kind, fft, h_sums, n_species, n_frames, dim, h_cross);
    });
}
int ta_onsager(ta_ctx* ctx, int fft, int n_species, const int32_t* h_species, const double* h_weights, double* h_moments,
               double* h_cross) {
    return coll_host(ctx, COLL_MOMENTS, fft, n_species, h_species, h_weights, h_moments, h_cross);
}
int ta_onsager_cross(ta_ctx* ctx, int fft, const double* h_moments, int n_species, int64_t n_frames, int dim, double* h_cross) {
    return coll_cross_call(ctx, COLL_MOMENTS, fft, h_moments, n_species, n_frames, dim, h_cross);
}
int ta_current(ta_ctx* ctx, int fft, int n_species, const int32_t* h_species, const double* h_weights, double* h_currents,
               double* h_cross) {
    return coll_host(ctx, COLL_CURRENTS, fft, n_species, h_species, h_weights, h_currents, h_cross);
}
int ta_current_cross(ta_ctx* ctx, int fft, const double* h_currents, int n_species, int64_t n_frames, int dim, double* h_cross) {
    return coll_cross_call(ctx, COLL_CURRENTS, fft, h_currents, n_species, n_frames, dim, h_cross);
}

int ta_species_self(ta_ctx* ctx, int quantity, int fft, int n_species, const int32_t* h_species, const double* h_weights,
                    double* h_self, int64_t* h_counts) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(self_args(ctx, quantity, fft, n_species, h_species, h_self));
    TA_CHECK(check_staged(ctx));
    if (ctx->is_cpu) {
        TA_CHECK(check_labels(fail, ctx, h_species, ctx->st_A, n_species));
        return cpu_rc(ctx, ta::cpu::species_self(cpu_state(ctx), quantity == TA_SELF_MSD, fft != 0, n_species, h_species, h_weights,
                                                 h_self, h_counts));
    }
    double* d_out = nullptr;
    TA_CHECK(ta::self_launch(ctx, quantity, fft, n_species, h_species, h_weights, h_counts, &d_out));
    return out_finish(ctx, self_out(n_species, ctx->st_T), d_out, {h_self});
    });
}

int ta_scatter(ta_ctx* ctx, int fft, int n_k, const double* h_kvecs, double* h_self, double* h_density, double* h_coll) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(scatter_args(ctx, fft, n_k, h_kvecs, ctx->st_nslabs ? ctx->st_D : 0, h_self, h_density, h_coll));
    TA_CHECK(check_staged(ctx));
    if (ctx->is_cpu) return cpu_rc(ctx, ta::cpu::scatter(cpu_state(ctx), fft != 0, n_k, h_kvecs, h_self, h_density, h_coll));
    double* d_out = nullptr;
    TA_CHECK(ta::scatter_launch(ctx, fft, n_k, h_kvecs, h_self != nullptr, h_density != nullptr, h_coll != nullptr, &d_out));
    return out_finish(ctx, scatter_out(n_k, ctx->st_T), d_out, {h_self, h_density, h_coll});
    });
}

int ta_orient(ta_ctx* ctx, int fft, int mode, int64_t n_vectors, const int32_t* h_index, const double* h_dimensions,
              const double* h_weights, double* h_c1, double* h_c2, double* h_total, double* h_coll) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    if (ctx->is_cpu) {
        const OrientArgs a{fft, mode, n_vectors, h_index, h_dimensions, h_weights, h_c1 != nullptr, h_c2 != nullptr, h_total != nullptr,
                           h_coll != nullptr};
        BoxTable box;
        TA_CHECK(orient_check(ctx, a, ctx->st_T, ctx->st_A, ctx->st_nslabs ? ctx->st_D : 0, &box));
        std::vector<double> rows;
        if (h_dimensions) {
            rows.resize((size_t)kOrientBoxRows * (size_t)box.tpitch);
            orient_box_rows(box, rows.data());
        }
        return cpu_rc(ctx, ta::cpu::orient(cpu_state(ctx), fft != 0, mode, n_vectors, h_index, h_dimensions ? rows.data() : nullptr,
                                           box.tpitch, h_weights, h_c1, h_c2, h_total, h_coll));
    }
    double* d_out = nullptr;
    TA_CHECK(orient_entry(ctx, nullptr, fft, mode, n_vectors, h_index, h_dimensions, h_weights, h_c1, h_c2, h_total, h_coll, ctx->stream,
                          &d_out));
    return out_finish(ctx, orient_out(ctx->st_T), d_out, {h_c1, h_c2, h_total, h_coll});
    });
}

int ta_chain_modes(ta_ctx* ctx, int fft, int64_t n_chains, int64_t chain_len, const int32_t* h_members, int n_modes,
                   const double* h_coeff, const double* h_dimensions, double* h_acf) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    const ChainArgs a{fft, n_chains, chain_len, h_members, n_modes, h_coeff, h_dimensions, h_acf};
    if (ctx->is_cpu) {
        BoxTable box;
        TA_CHECK(chain_check(ctx, a, &box));
        std::vector<double> rows;
        if (h_dimensions) {
            rows.resize((size_t)kOrientBoxRows * (size_t)box.tpitch);
            orient_box_rows(box, rows.data());
        }
        return cpu_rc(ctx, ta::cpu::chain_modes(cpu_state(ctx), fft != 0, n_chains, chain_len, h_members, n_modes, h_coeff,
                                                h_dimensions ? rows.data() : nullptr, box.tpitch, h_acf));
    }
    double* d_out = nullptr;
    TA_CHECK(chain_entry(ctx, a, nullptr, ctx->stream, &d_out));
    return out_finish(ctx, chain_modes_out(n_modes, ctx->st_T), d_out, {h_acf});
    });
}

int ta_chain_modes_tile(int* modes, int* frames) {
    int a = 0, b = 0;
    ta::chain_modes_tile(&a, &b);
    if (modes) *modes = a;
    if (frames) *frames = b;
    return TA_OK;
}

int ta_scatter_collective(ta_ctx* ctx, int fft, const double* h_density, int n_k, int64_t n_frames, double* h_coll) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(check_fft(ctx, fft));
    if (!h_density || !h_coll) return fail(ctx, TA_E_INVALID, "density or collective output is NULL");
    TA_CHECK(check_n_k(fail, ctx, n_k));
    TA_CHECK(check_sums_shape(ctx, n_frames));
    if (ctx->is_cpu) return cpu_rc(ctx, ta::cpu::scatter_collective(ctx->cpu_threads, fft != 0, h_density, n_k, n_frames, h_coll));
    return ta::scatter_collective_host(ctx, fft, h_density, n_k, n_frames, h_coll);
    });
}

int ta_kcurrent(ta_ctx* ctx, int fft, int n_k, const double* h_kvecs, const double* h_weights, double* h_current, double* h_long,
                double* h_trans) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(kcurrent_args(ctx, fft, n_k, h_kvecs, h_current, h_long, h_trans));
    if (ctx->is_cpu)
        return cpu_rc(ctx, ta::cpu::kcurrent(cpu_state(ctx), fft != 0, n_k, h_kvecs, h_weights, h_current, h_long, h_trans));
    double* d_out = nullptr;
    TA_CHECK(ta::kcurrent_launch(ctx, fft, n_k, h_kvecs, h_weights, h_long || h_trans, &d_out));
    return out_finish(ctx, kcurrent_out(n_k, ctx->st_T, ctx->st_D), d_out, {h_current, h_long, h_trans});
    });
}

int ta_kcurrent_correlate(ta_ctx* ctx, int fft, const double* h_current, int n_k, const double* h_kvecs, int64_t n_frames, int dim,
                          double* h_long, double* h_trans) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(check_sums_shape(ctx, n_frames, &dim));
    if (!h_current) return fail(ctx, TA_E_INVALID, "current is NULL");
    TA_CHECK(check_kcurrent(fail, ctx, fft, n_k, h_kvecs, dim, h_long || h_trans));
    if (ctx->is_cpu)
        return cpu_rc(ctx, ta::cpu::kcurrent_correlate(ctx->cpu_threads, fft != 0, h_current, n_k, h_kvecs, n_frames, dim, h_long, h_trans));
    return ta::kcurrent_correlate_host(ctx, fft, h_current, n_k, h_kvecs, n_frames, dim, h_long, h_trans);
    });
}

int ta_kcurrent_tile(int* kc, int* frames_f64, int* frames_f32) {
    int a = 0, b = 0, c = 0;
    ta::kcurrent_tile(&a, &b, &c);
    if (kc) *kc = a;
    if (frames_f64) *frames_f64 = b;
    if (frames_f32) *frames_f32 = c;
    return TA_OK;
}

int ta_partial_density(ta_ctx* ctx, int fft, int n_k, const double* h_kvecs, int n_species, const int32_t* h_species,
                       const double* h_weights, double* h_density, double* h_cross) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(partial_args(ctx, fft, n_k, h_kvecs, ctx->st_nslabs ? ctx->st_D : 0, n_species, h_species, h_density));
    TA_CHECK(partial_slab(ctx));
    TA_CHECK(check_labels(fail, ctx, h_species, ctx->st_A, n_species));
    if (ctx->is_cpu)
        return cpu_rc(ctx, ta::cpu::partial_density(cpu_state(ctx), fft != 0, n_k, h_kvecs, n_species, h_species, h_weights, h_density,
                                                    h_cross));
    double* d_out = nullptr;
    TA_CHECK(ta::partial_launch(ctx, fft, n_k, h_kvecs, n_species, h_species, h_weights, h_cross != nullptr, &d_out));
    return out_finish(ctx, partial_out(n_k, n_species, ctx->st_T), d_out, {h_density, h_cross});
    });
}

int ta_partial_cross(ta_ctx* ctx, int fft, const double* h_density, int n_k, int n_species, int64_t n_frames, double* h_cross) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(check_fft(ctx, fft));
    TA_CHECK(check_species_count(fail, ctx, n_species));
    if (!h_density || !h_cross) return fail(ctx, TA_E_INVALID, "partial density or cross output is NULL");
    TA_CHECK(check_n_k(fail, ctx, n_k));
    TA_CHECK(check_sums_shape(ctx, n_frames));
    if (ctx->is_cpu)
        return cpu_rc(ctx, ta::cpu::partial_cross(ctx->cpu_threads, fft != 0, h_density, n_k, n_species, n_frames, h_cross));
    return ta::partial_cross_host(ctx, fft, h_density, n_k, n_species, n_frames, h_cross);
    });
}

int ta_partial_density_tile(int n_species, int* st, int* kc, int* frames_f64, int* frames_f32) {
    int a = 0, b = 0, c = 0, d = 0;
    if (!ta::species_density_tile(n_species, &a, &b, &c, &d))
        return fail(nullptr, TA_E_INVALID, "n_species must be 1 ... " + std::to_string(TA_ONSAGER_MAX_SPECIES));
    if (st) *st = a;
    if (kc) *kc = b;
    if (frames_f64) *frames_f64 = c;
    if (frames_f32) *frames_f32 = d;
    return TA_OK;
}

int ta_vanhove(ta_ctx* ctx, int n_lags, const int64_t* h_lags, int n_bins, double dr, int64_t* h_counts, double* h_moments) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(check_vanhove(fail, ctx, n_lags, h_lags, n_bins, dr, ctx->st_nslabs ? ctx->st_T : 0, h_counts || h_moments));
    TA_CHECK(check_staged(ctx));
    if (ctx->is_cpu) {
        TA_CHECK(check_cols(ctx, "vanhove: ", ctx->st_A, ctx->st_D));
        return cpu_rc(ctx, ta::cpu::vanhove(cpu_state(ctx), n_lags, h_lags, n_bins, dr, h_counts, h_moments));
    }
    double* d_out = nullptr;
    TA_CHECK(ta::vanhove_launch(ctx, n_lags, h_lags, n_bins, dr, h_counts != nullptr, h_moments != nullptr, &d_out));
    return out_finish(ctx, vanhove_out(n_lags, n_bins), d_out, {h_counts, h_moments});
    });
}

int ta_overlap(ta_ctx* ctx, int n_lags, const int64_t* h_lags, int n_cutoffs, const double* h_cutoffs, int64_t* h_q) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(check_overlap(fail, ctx, n_lags, h_lags, n_cutoffs, h_cutoffs, ctx->st_nslabs ? ctx->st_T : 0, h_q != nullptr));
    TA_CHECK(check_staged(ctx));
    if (ctx->is_cpu) {
        TA_CHECK(check_cols(ctx, "overlap: ", ctx->st_A, ctx->st_D));
        return cpu_rc(ctx, ta::cpu::overlap(cpu_state(ctx), n_lags, h_lags, n_cutoffs, h_cutoffs, h_q));
    }
    double* d_out = nullptr;
    TA_CHECK(ta::overlap_launch(ctx, n_lags, h_lags, n_cutoffs, h_cutoffs, &d_out));
    return out_finish(ctx, overlap_out(n_cutoffs, n_lags, ctx->st_T), d_out, {h_q});
    });
}

int ta_overlap_tile(int* slots) {
    if (slots) *slots = ta::overlap_slots();
    return TA_OK;
}

int ta_overlap_density(ta_ctx* ctx, int n_k, const double* h_kvecs, int n_lags, const int64_t* h_lags, int n_cutoffs,
                       const double* h_cutoffs, double* h_w) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(check_overlap_density(fail, ctx, n_k, h_kvecs, ctx->st_nslabs ? ctx->st_D : 0, n_lags, h_lags, n_cutoffs, h_cutoffs,
                                   ctx->st_nslabs ? ctx->st_T : 0, h_w != nullptr));
    TA_CHECK(check_staged(ctx));
    if (ctx->is_cpu) {
        TA_CHECK(check_cols(ctx, "overlap_density: ", ctx->st_A, ctx->st_D));
        return cpu_rc(ctx, ta::cpu::overlap_density(cpu_state(ctx), n_k, h_kvecs, n_lags, h_lags, n_cutoffs, h_cutoffs, h_w));
    }
    double* d_out = nullptr;
    TA_CHECK(ta::overlap_density_launch(ctx, n_k, h_kvecs, n_lags, h_lags, n_cutoffs, h_cutoffs, &d_out));
    return out_finish(ctx, overlap_density_out(n_k, n_cutoffs, n_lags, ctx->st_T), d_out, {h_w});
    });
}

int ta_overlap_density_tile(int* slots, int* kc, int* frames) {
    int a = 0, b = 0, c = 0;
    ta::overlap_density_tile(&a, &b, &c);
    if (slots) *slots = a;
    if (kc) *kc = b;
    if (frames) *frames = c;
    return TA_OK;
}

int ta_vanhove_distinct(ta_ctx* ctx, int n_lags, const int64_t* h_lags, int64_t origin_stride, int64_t n_a, const int64_t* h_idx_a,
                        int64_t n_b, const int64_t* h_idx_b, const double* h_dimensions, const int* axes, int n_bins, double dr,
                        int64_t* h_counts) {
    return host_call(ctx, [&]() -> int {
    const VhdArgs a{n_lags, n_bins, dr, origin_stride, n_a, n_b, h_lags, h_idx_a, h_idx_b, h_dimensions, axes};
    VhdPlan p;
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(vhd_args(ctx, a, ctx->st_nslabs ? ctx->st_T : 0, h_counts));
    TA_CHECK(check_staged(ctx));
    TA_CHECK(vhd_plan(ctx, a, ctx->st_T, ctx->st_A, ctx->st_D, &p));
    if (ctx->is_cpu)
        return cpu_rc(ctx, ta::cpu::vanhove_distinct(cpu_state(ctx), n_lags, h_lags, origin_stride, p.n_a, p.ida.data(), p.n_b, p.idb.data(),
                                                     p.box.data(), p.box.per_frame, n_bins, dr, h_counts));
    int64_t* d_out = nullptr;
    TA_CHECK(vhd_launch(ctx, p, h_lags, dr, nullptr, ctx->stream, &d_out));
    return out_finish(ctx, vhd_out(n_lags, n_bins), (const double*)d_out, {h_counts});
    });
}

int ta_pair_find(ta_ctx* ctx, int64_t n_a, const int64_t* h_idx_a, int64_t n_b, const int64_t* h_idx_b, const double* h_dimensions,
                 const int* axes, double r_cut, int64_t search_stride, int64_t* n_pairs) {
    return host_call(ctx, [&]() -> int {
    PairFindPlan p;
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(pair_find_plan(ctx, n_a, h_idx_a, n_b, h_idx_b, h_dimensions, axes, r_cut, search_stride, n_pairs, &p));
    if (ctx->is_cpu) {
        ctx->pair_n = -1;
        TA_CHECK(cpu_rc(ctx, ta::cpu::pair_find(cpu_state(ctx), p.n_a, p.ida.data(), p.n_b, p.idb.data(), p.same, search_stride,
                                                p.box.data(), p.box.per_frame, p.rc2, &ctx->pair_host)));
        ctx->pair_n = (int64_t)(ctx->pair_host.size() / 2), ctx->pair_A = p.A;
    } else {
        TA_CHECK(pair_find_launch(ctx, p));
    }
    *n_pairs = ctx->pair_n;
    return TA_OK;
    });
}

int ta_pair_find_read(ta_ctx* ctx, int64_t capacity, int32_t* h_pairs) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    if (ctx->pair_n < 0 || (!ctx->is_cpu && !ctx->pair_list.p))
        return fail(ctx, TA_E_STATE, "pair_find_read: no pair list has been found (ta_pair_find comes first; ta_trim and a new staging release it)");
    if (capacity < ctx->pair_n)
        return fail(ctx, TA_E_INVALID, "pair_find_read: capacity " + std::to_string(capacity) + " is smaller than the " +
                                           std::to_string(ctx->pair_n) + " pairs found");
    if (ctx->pair_n == 0) return fail(ctx, TA_E_STATE, "pair_find_read: the found pair list is empty");
    if (!h_pairs) return fail(ctx, TA_E_INVALID, "pair_find_read: the pairs output is NULL");
    const size_t bytes = sizeof(int32_t) * 2 * (size_t)ctx->pair_n;
    if (ctx->is_cpu) {
        memcpy(h_pairs, ctx->pair_host.data(), bytes);
        return TA_OK;
    }
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    TA_HIP_TRY(ctx, hipMemcpyAsync(h_pairs, ctx->pair_list.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return host_wait(ctx);
    });
}

// ta_pair_lifetime and (bond != NULL) ta_bond_lifetime: the plan, the CPU backend or the device half, the outputs copied back
static int life_host(ta_ctx* ctx, int fft, int64_t n_rows, const int32_t* h_rows, const double* h_dimensions, const int* axes, double r_cut,
                     const BondArgs* bond, const LifePtrs& h) {
    return host_call(ctx, [&]() -> int {
    PairLifePlan p;
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(pair_life_plan(ctx, fft, n_rows, h_rows, h_dimensions, axes, r_cut, h.any(), &p, bond));
    if (ctx->is_cpu && bond)
        return cpu_rc(ctx, ta::cpu::bond_lifetime(cpu_state(ctx), fft != 0, p.P, p.n_at, h_rows, p.box.data(), p.box.per_frame, p.cuts, p.gap,
                                                  h.lags, h.runs, h.nb));
    if (ctx->is_cpu)
        return cpu_rc(ctx, ta::cpu::pair_lifetime(cpu_state(ctx), fft != 0, p.P, h_rows ? h_rows : ctx->pair_host.data(), p.box.data(),
                                                  p.box.per_frame, p.rc2, h.lags, h.runs, h.nb));
    double* d_out = nullptr;
    TA_CHECK(pair_life_launch(ctx, fft, p, h, ctx->stream, &d_out));
    return life_finish(ctx, p.out, h, d_out);
    });
}
int ta_pair_lifetime(ta_ctx* ctx, int fft, int64_t n_pairs, const int32_t* h_pairs, const double* h_dimensions, const int* axes,
                     double r_cut, double* h_ci, int64_t* h_runs, double* h_nb) {
    return life_host(ctx, fft, n_pairs, h_pairs, h_dimensions, axes, r_cut, nullptr, {h_ci, nullptr, h_runs, h_nb});
}
int ta_bond_lifetime(ta_ctx* ctx, int fft, int64_t n_bonds, int n_at, const int32_t* h_atoms, const double* h_dimensions, const int* axes,
                     double r_cut, double r_break, double cos_cut, double cos_break, int gap, double* h_ci, int64_t* h_runs, double* h_nb) {
    const BondArgs bond{n_at, r_break, cos_cut, cos_break, gap};
    return life_host(ctx, fft, n_bonds, h_atoms, h_dimensions, axes, r_cut, &bond, {h_ci, nullptr, h_runs, h_nb});
}

// ta_shell_residence, ta_shell_msd and ta_shell_orient: the plan, the CPU backend or the device half, the outputs copied back
static int shell_host(ta_ctx* ctx, ShellKind kind, int fft, const ShellArgs& a, const LifePtrs& h) {
    return host_call(ctx, [&]() -> int {
    ShellPlan p;
    TA_CHECK(need_ctx(ctx));
    TA_CHECK(shell_plan(ctx, kind, fft, a, h.any(), &p));
    if (ctx->is_cpu) return cpu_shell(ctx, fft != 0, p, h);
    double* d_out = nullptr;
    TA_CHECK(shell_launch(ctx, fft, p, h, ctx->stream, &d_out));
    return life_finish(ctx, p.out, h, d_out);
    });
}
int ta_shell_residence(ta_ctx* ctx, int fft, int64_t n_a, const int64_t* h_idx_a, int64_t n_b, const int64_t* h_idx_b,
                       const double* h_dimensions, const int* axes, double r_cut, double r_break, int gap, double* h_ci, int64_t* h_runs,
                       double* h_nb) {
    return shell_host(ctx, SHELL_RESIDENCE, fft, {n_a, n_b, h_idx_a, h_idx_b, h_dimensions, axes, r_cut, r_break, gap},
                      {h_ci, nullptr, h_runs, h_nb});
}
int ta_shell_msd(ta_ctx* ctx, int condition, int64_t max_lag, int64_t n_a, const int64_t* h_idx_a, int64_t n_b, const int64_t* h_idx_b,
                 const double* h_dimensions, const int* axes, double r_cut, double r_break, int gap, double* h_sums, int64_t* h_count,
                 int64_t* h_runs, double* h_nb) {
    return shell_host(ctx, SHELL_MSD, 0, {n_a, n_b, h_idx_a, h_idx_b, h_dimensions, axes, r_cut, r_break, gap, condition, max_lag},
                      {h_sums, h_count, h_runs, h_nb});
}
int ta_shell_orient(ta_ctx* ctx, int condition, int64_t max_lag, int mode, int anchor, const int32_t* h_index, int64_t n_a,
                    const int64_t* h_idx_a, int64_t n_b, const int64_t* h_idx_b, const double* h_dimensions, const int* axes, double r_cut,
                    double r_break, int gap, double* h_sums, int64_t* h_count, int64_t* h_runs, double* h_nb) {
    return shell_host(ctx, SHELL_ORIENT, 0,
                      {n_a, n_b, h_idx_a, h_idx_b, h_dimensions, axes, r_cut, r_break, gap, condition, max_lag, mode, anchor, h_index},
                      {h_sums, h_count, h_runs, h_nb});
}

// The host slabs of a context go away (ta_compound: they hold atoms, the staged slab no longer does)
static void release_host_slabs(ta_ctx* ctx) {
    for (size_t i = 0; i < ctx->h_slabs.size(); ++i) {
        if (ctx->h_blocks[i].base) host_block_unmap(ctx->h_blocks[i]);
        else if (ctx->h_slabs[i]) hipHostFree(ctx->h_slabs[i]);
        ctx->h_blocks[i] = HostBlock{};
        ctx->h_slabs[i] = nullptr;
    }
}

int ta_compound(ta_ctx* ctx, int64_t n_compounds, const int64_t* h_offsets, const int32_t* h_members, const double* h_weights,
                const double* h_frame_weights, void** h_out) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    if (h_out) *h_out = nullptr;
    if (!h_offsets || !h_members) return fail(ctx, TA_E_INVALID, "compound: offsets or members are NULL");
    if (n_compounds < 1) return fail(ctx, TA_E_INVALID, "compound: need n_compounds >= 1");
    TA_CHECK(check_staged(ctx));
    if (ctx->st_nslabs != 1) return fail(ctx, TA_E_UNSUPPORTED, "compound: one staged slab only (this context holds " + std::to_string(ctx->st_nslabs) + ")");
    const int64_t T = ctx->st_T, A = ctx->st_A, C = n_compounds;
    const int D = ctx->st_D;
    TA_CHECK(check_cols(ctx, "compound: ", A, D));
    if (C * D >= (int64_t)1 << 31) return fail(ctx, TA_E_INVALID, "compound: n_compounds * dim must be below 2^31");
    if (h_offsets[0] != 0) return fail(ctx, TA_E_INVALID, "compound: offsets must start at 0");
    for (int64_t c = 0; c < C; ++c)
        if (h_offsets[c + 1] <= h_offsets[c] || h_offsets[c + 1] >= (int64_t)1 << 31)
            return fail(ctx, TA_E_INVALID, "compound: offsets must be strictly increasing (no empty compound) and end below 2^31 (compound " + std::to_string(c) + ")");
    const int64_t M = h_offsets[C];
    for (int64_t i = 0; i < M; ++i)
        if (h_members[i] < 0 || h_members[i] >= A)
            return fail(ctx, TA_E_INVALID, "compound: member " + std::to_string(h_members[i]) + " (entry " + std::to_string(i) + ") is outside 0 ... n_atoms - 1");
    const size_t out_elems = (size_t)T * (size_t)C * (size_t)D;
    if (ctx->is_cpu) {
        HostBlock blk;
        if (host_block_map(out_elems * sizeof(double), &blk) != 0) return fail(ctx, TA_E_NOMEM, "compound: no host memory for the new slab");
        if (int rc = ta::cpu::compound(cpu_state(ctx), C, h_offsets, h_members, h_weights, h_frame_weights, (double*)blk.base)) {
            host_block_unmap(blk);
            return cpu_rc(ctx, rc);
        }
        release_host_slabs(ctx);
        ctx->h_slabs[0] = blk.base, ctx->h_blocks[0] = blk;
        set_staged(ctx, T, C, D, TA_F64, 1, false);
        ctx->st_compound = true;
        if (h_out) *h_out = blk.base;
        return TA_OK;
    }
    TA_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the plan as the kernel reads it: int32 offsets and members, float64 member weights and their sums in member order
    const size_t n_off = (size_t)C + 1, n_int = (n_off + (size_t)M + 1) / 2 * 2;
    const size_t n_dbl = (h_weights ? (size_t)M : 0) + (size_t)C;
    std::vector<double> plan(n_int / 2 + n_dbl);
    int32_t* p_off = reinterpret_cast<int32_t*>(plan.data());
    int32_t* p_mem = p_off + n_off;
    double* p_w = plan.data() + n_int / 2;
    double* p_g = p_w + (h_weights ? (size_t)M : 0);
    for (size_t c = 0; c < n_off; ++c) p_off[c] = (int32_t)h_offsets[c];
    std::copy(h_members, h_members + M, p_mem);
    if (h_weights) std::copy(h_weights, h_weights + M, p_w);
    for (int64_t c = 0; c < C; ++c) {
        double g = 0.0;
        for (int64_t i = h_offsets[c]; i < h_offsets[c + 1]; ++i) g += h_weights ? h_weights[i] : 1.0;
        p_g[c] = g;
    }
    hipStream_t st = ctx->stream;
    const int64_t pitch = ctx->st_pitch, n_cols = A * D;
    double* d_new = nullptr;
    TA_HIP_TRY(ctx, hipMalloc((void**)&d_new, pm_bytes(T, C * D)));
    struct DevFree {
        void operator()(void* p) const { hipFree(p); }
    };
    std::unique_ptr<void, DevFree> fresh(d_new);  // (an exception below: host_call waits, then this frees)
    // everything queued from here on is waited for before the plan's host copy, or on failure the new slab, goes away
    const int rc = [&]() -> int {
        TA_CHECK(ensure(ctx, ctx->comp_plan, sizeof(double) * plan.size()));
        TA_CHECK(order_after_staging(ctx, st));
        TA_HIP_TRY(ctx, hipMemcpyAsync(ctx->comp_plan.p, plan.data(), sizeof(double) * plan.size(), hipMemcpyHostToDevice, st));
        const int* d_off = (const int*)ctx->comp_plan.p;
        const double* d_w = (const double*)ctx->comp_plan.p + n_int / 2;
        const double* d_F = nullptr;
        if (h_frame_weights) {  // F = the one-species "current" of the slab with w = u: the slab read as it is
            const int n_parts = species_sum_parts(ctx->n_cu, 1, (long)T, (long)n_cols);
            TA_CHECK(ensure(ctx, ctx->ons_part, sizeof(double) * (size_t)n_parts * T * D));
            TA_CHECK(ensure(ctx, ctx->ons_lab, sizeof(int32_t) * (size_t)A));
            TA_CHECK(ensure(ctx, ctx->ons_w, sizeof(double) * (size_t)A));
            TA_CHECK(ensure(ctx, ctx->comp_f, sizeof(double) * (size_t)T * D));
            TA_HIP_TRY(ctx, hipMemsetAsync(ctx->ons_lab.p, 0, sizeof(int32_t) * (size_t)A, st));
            TA_HIP_TRY(ctx, hipMemcpyAsync(ctx->ons_w.p, h_frame_weights, sizeof(double) * (size_t)A, hipMemcpyHostToDevice, st));
            d_F = (const double*)ctx->comp_f.p;
        }
        TA_CHECK(call_begin(ctx, st));
        if (d_F)
            TA_CHECK(weighted_total(ctx, ctx->d_slabs[0], ctx->st_dev_f32, pitch, T, A, D, (const int*)ctx->ons_lab.p,
                                    (const double*)ctx->ons_w.p, species_sum_parts(ctx->n_cu, 1, (long)T, (long)n_cols),
                                    (double*)ctx->comp_f.p, st));
        TA_LAUNCH_MAIN(ctx, "k_compound", st,
                       launch_compound(ctx->n_cu, ctx->d_slabs[0], ctx->st_dev_f32, (long)pitch, (long)T, (long)n_cols, D, (long)C,
                                       d_off, d_off + n_off, h_weights ? d_w : nullptr, d_w + (h_weights ? (size_t)M : 0), d_F,
                                       d_new, st));
        return call_end(ctx, st);
    }();
    const int rc_wait = host_wait(ctx);
    if (rc || rc_wait) return rc ? rc : rc_wait;
    // the call has completed: the old device slab and the host slabs (they hold atoms) go
    hipFree(ctx->d_slabs[0]);
    ctx->d_slabs[0] = (double*)fresh.release();
    release_host_slabs(ctx);
    set_staged(ctx, T, C, D, ctx->st_dtype, 1, false);
    ctx->st_compound = true;
    return TA_OK;
    });
}

int ta_unwrap(ta_ctx* ctx, int slab, const double* h_dimensions, const int* axes) {
    return host_call(ctx, [&]() -> int {
    TA_CHECK(need_ctx(ctx));
    if (!h_dimensions || !axes) return fail(ctx, TA_E_INVALID, "dimensions or axes are NULL");
    TA_CHECK(check_staged(ctx));
    TA_CHECK(check_slab(ctx, slab));
    BoxTable box;
    const std::string why = box_table(h_dimensions, ctx->st_T, ctx->st_D, axes, 256, &box);
    if (!why.empty()) return fail(ctx, TA_E_INVALID, "unwrap: " + why);
    if (ctx->is_cpu) {
        ta::cpu::unwrap(cpu_state(ctx), slab, box, axes);
        return TA_OK;
    }
    TA_CHECK(unwrap_launch(ctx, slab, box, axes));
    return host_wait(ctx);
    });
}

}  // extern "C"
