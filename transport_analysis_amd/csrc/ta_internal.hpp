// ta_internal.hpp — shared between the translation units of libta_hip.so
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <exception>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "../../include/ta_hip.h"
#include "fft_engine.hpp"
#include "kcurrent_math.hpp"

struct ta_ctx;

namespace ta {

struct BoxTable;  // unwrap_box.hpp

// No exception leaves an extern "C" function (every call returns an int status).  Every entry point's
// body runs inside guard(report, body): std::bad_alloc becomes TA_E_NOMEM, anything else TA_E_HIP, the message goes
// through `report(code, text)` -- the file's fail / gfail, which records it for ta_last_error and returns the code
// (and must not throw itself: they swallow a failing string copy).
template <class Report, class Body>
int guard(Report&& report, Body&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        try {
            return report(TA_E_NOMEM, "out of host memory (std::bad_alloc inside the library)");
        } catch (...) {
            return TA_E_NOMEM;
        }
    } catch (const std::exception& e) {
        try {
            return report(TA_E_HIP, std::string("internal error: ") + e.what());
        } catch (...) {
            return TA_E_HIP;
        }
    } catch (...) {
        try {
            return report(TA_E_HIP, "internal error: unknown exception");
        } catch (...) {
            return TA_E_HIP;
        }
    }
}

// ... with the reporter nearly every entry point uses: the file's `fail(owner, code, text)` on the call's context / group
// (NULL where there is none).  An entry point whose reporter does more (waits for queued work first) spells it out with guard.
template <class Fail, class Owner, class Body>
int guarded(Fail fail, Owner owner, Body&& body) noexcept {
    return guard([&](int code, const std::string& text) { return fail(owner, code, text); }, body);
}

// Which quantity a compute request asks for (api.hip's dispatch, and group.hip's requests to its members)
enum Which { W_FFT = 0, W_DIRECT = 1, W_HELFAND = 2 /* needs two slabs: velocities, positions */, W_MSD_FFT = 3, W_MSD_DIRECT = 4 };
inline bool is_msd(int which) { return which == W_MSD_FFT || which == W_MSD_DIRECT; }
inline int slabs_needed(int which) { return which == W_HELFAND ? 2 : 1; }

// api.hip, for group.hip (several contexts driven by one host thread): one context's share of a host-facing call queued
// on its streams, the sum over its atoms left on the device; host_wait blocks until that work and its copies are done,
// host_finish queues the copies of small results (n doubles each; a NULL destination is skipped) first
int host_launch(ta_ctx* ctx, int which, const double* h_masses, double scale, double* h_bp, int64_t ld_host,
                double** d_total);
int host_wait(ta_ctx* ctx);
struct HostCopy {
    double* h;
    const double* d;
    size_t n;
};
int host_finish(ta_ctx* ctx, std::initializer_list<HostCopy> copies);

// Where a host-facing call's results lie in the context's output buffer for that call, in 8-byte elements (int64 counts
// travel as doubles): segment i is [off[i], off[i + 1]), off[n] the buffer's size.  One function per call below lays its
// segments out, and every consumer asks it: the launch half for the buffer's size and the device outputs (at), the blocking
// entry for the copies back (api.hip's out_finish), the correlators of host sums for their slices, the group for the parts
// it sums over its members (group.hip's sum_members).  The comment on each function is the one record of that call's order.
struct OutLayout {
    static constexpr int kMax = 4;
    int n = 0;
    size_t off[kMax + 1] = {};
    OutLayout() = default;
    OutLayout(std::initializer_list<size_t> len) {
        for (size_t l : len) off[n + 1] = off[n] + l, ++n;
    }
    size_t total() const { return off[n]; }
    size_t len(int i) const { return off[i + 1] - off[i]; }
    // segment i of the buffer at `base`, or NULL where it is not wanted
    double* at(double* base, int i, bool want = true) const { return want ? base + off[i] : nullptr; }
};
inline size_t out_n(int64_t a, int64_t b = 1, int64_t c = 1, int64_t d = 1, int64_t e = 1) {
    return (size_t)a * (size_t)b * (size_t)c * (size_t)d * (size_t)e;
}
// ta_conductivity: moment (T, D) | Phi (T) | self lag sum (T)
inline OutLayout cond_out(int64_t T, int D) { return {out_n(T, D), out_n(T), out_n(T)}; }
// ta_onsager / ta_current: sums (S, T, D) | cross term (T, S, S)
inline OutLayout coll_out(int S, int64_t T, int D) { return {out_n(S, T, D), out_n(T, S, S)}; }
// ta_species_self: self lag sums (S, T)
inline OutLayout self_out(int S, int64_t T) { return {out_n(S, T)}; }
// ta_scatter: self (K, T) | density (K, T, 2) | coll (K, T)
inline OutLayout scatter_out(int K, int64_t T) { return {out_n(K, T), out_n(K, T, 2), out_n(K, T)}; }
// ta_orient: c1 (T) | c2 (T) | total (T, 3) | coll (T)
inline OutLayout orient_out(int64_t T) { return {out_n(T), out_n(T), out_n(T, 3), out_n(T)}; }
// ta_chain_modes: acf (Q, T)
inline OutLayout chain_modes_out(int Q, int64_t T) { return {out_n(Q, T)}; }
// ta_kcurrent: current (K, T, D, 2) | long (K, T) | trans (K, T)
inline OutLayout kcurrent_out(int K, int64_t T, int D) { return {out_n(K, T, D, 2), out_n(K, T), out_n(K, T)}; }
// ta_partial_density: density (K, S, T, 2) | cross term (K, T, S, S)
inline OutLayout partial_out(int K, int S, int64_t T) { return {out_n(K, S, T, 2), out_n(K, T, S, S)}; }
// ta_vanhove: counts (L, B + 1) int64 | moments (L, 2)
inline OutLayout vanhove_out(int L, int B) { return {out_n(L, B + 1), out_n(L, 2)}; }
// ta_overlap: Q (C, L, T) int64
inline OutLayout overlap_out(int C, int L, int64_t T) { return {out_n(C, L, T)}; }
// ta_overlap_density: W (K, C, L, T, 2)
inline OutLayout overlap_density_out(int K, int C, int L, int64_t T) { return {out_n(K, C, L, T, 2)}; }
// ta_vanhove_distinct: counts (L, B + 1) int64
inline OutLayout vhd_out(int L, int B) { return {out_n(L, B + 1)}; }

// api.hip, for group.hip: one context's conductivity share (ta_conductivity on its staged slab 0 with its atoms' charges
// h_q), queued: *d_out = cond_out's segments (Phi with coll, the self lag sum with self), valid after host_wait; and Phi
// of a host (n_frames, dim) moment on the context's device, blocking
int cond_launch(ta_ctx* ctx, int fft, const double* h_q, bool coll, bool self, double** d_out);
int cond_collective_host(ta_ctx* ctx, int fft, const double* h_moment, int64_t T, int D, double* h_coll);
// api.hip, for group.hip: the two species-collective quantities, Onsager moments (ta_onsager*) and Green-Kubo currents
// (ta_current*), share one host path (api.hip's Collective table, indexed by `kind`).  One context's share (its staged
// slab 0 with its atoms' labels h_species and weights h_w or NULL, n_species the call's), queued: *d_out = coll_out's
// segments (the cross term with cross), valid after host_wait; and the cross term of host sums on the context's device,
// blocking
enum CollKind { COLL_MOMENTS = 0, COLL_CURRENTS = 1 };
int coll_launch(ta_ctx* ctx, int kind, int fft, int S, const int32_t* h_species, const double* h_w, bool cross, double** d_out);
int coll_cross_host(ta_ctx* ctx, int kind, int fft, const double* h_sums, int S, int64_t T, int D, double* h_cross);
// the species-count and host-label checks of a context (fail, ctx) or a group (gfail, g): the same messages for both; the
// atom index is relative to h_species
template <class Fail, class Owner>
static int check_species_count(Fail fail, Owner* owner, int S) {
    if (S < 1 || S > TA_ONSAGER_MAX_SPECIES)
        return fail(owner, TA_E_INVALID, "n_species must be 1 ... " + std::to_string(TA_ONSAGER_MAX_SPECIES));
    return TA_OK;
}
template <class Fail, class Owner>
static int check_labels(Fail fail, Owner* owner, const int32_t* h_species, int64_t n, int S) {
    for (int64_t a = 0; a < n; ++a)
        if (h_species[a] < 0 || h_species[a] >= S)
            return fail(owner, TA_E_INVALID, "species label " + std::to_string(h_species[a]) + " of atom " + std::to_string(a) +
                                                 " is outside 0 ... n_species - 1");
    return TA_OK;
}
// api.hip, for group.hip: one context's ta_species_self share (its staged slab 0 with its atoms' labels and weights, the
// call's n_species; labels checked here), queued: *d_out = self_out's segment, valid after host_wait; h_counts (n_species)
// or NULL: its atoms per species
int self_launch(ta_ctx* ctx, int quantity, int fft, int S, const int32_t* h_species, const double* h_w, int64_t* h_counts,
                double** d_out);
// "[<prefix>]n_k must be 1 ... TA_SCATTER_MAX_K", for every call that takes wavevectors
template <class Fail, class Owner>
static int check_n_k(Fail fail, Owner* owner, int n_k, const std::string& p = "") {
    if (n_k < 1 || n_k > TA_SCATTER_MAX_K) return fail(owner, TA_E_INVALID, p + "n_k must be 1 ... " + std::to_string(TA_SCATTER_MAX_K));
    return TA_OK;
}
// the wavevector checks of ta_scatter* on a context (fail, ctx) or a group (gfail, g): the same messages for both.  D: the
// components per wavevector (0: not known, nothing staged -- the caller reports that next)
template <class Fail, class Owner>
static int check_kvecs(Fail fail, Owner* owner, int fft, int n_k, const double* h_kvecs, int D, bool any_output) {
    if (fft != 0 && fft != 1) return fail(owner, TA_E_INVALID, "fft must be 0 or 1");
    if (!any_output) return fail(owner, TA_E_INVALID, "scatter: the self, density and collective outputs are all NULL");
    if (!h_kvecs) return fail(owner, TA_E_INVALID, "wavevectors are NULL");
    if (const int rc = check_n_k(fail, owner, n_k)) return rc;
    for (int64_t i = 0; i < (int64_t)n_k * D; ++i)
        if (!(h_kvecs[i] - h_kvecs[i] == 0.0))
            return fail(owner, TA_E_INVALID, "wavevector " + std::to_string(i / D) + " has a non-finite component");
    return TA_OK;
}
// api.hip, for group.hip: one context's ta_scatter share (its staged slab 0, the call's wavevectors, checked by the caller),
// queued: *d_out = scatter_out's segments -- the ones asked for are valid after host_wait; and the collective part of a
// host density on the context's device, blocking
int scatter_launch(ta_ctx* ctx, int fft, int n_k, const double* h_kvecs, bool self, bool density, bool coll, double** d_out);
int scatter_collective_host(ta_ctx* ctx, int fft, const double* h_density, int n_k, int64_t T, double* h_coll);
// the argument checks of ta_kcurrent* on a context (fail, ctx) or a group (gfail, g): the same messages for both.  D: the
// components per wavevector (0: not known, nothing staged -- the caller reports that next)
template <class Fail, class Owner>
static int check_kcurrent(Fail fail, Owner* owner, int fft, int n_k, const double* h_kvecs, int D, bool any_output) {
    if (fft != 0 && fft != 1) return fail(owner, TA_E_INVALID, "fft must be 0 or 1");
    if (!any_output) return fail(owner, TA_E_INVALID, "kcurrent: the current, longitudinal and transverse outputs are all NULL");
    if (!h_kvecs) return fail(owner, TA_E_INVALID, "wavevectors are NULL");
    if (const int rc = check_n_k(fail, owner, n_k)) return rc;
    for (int j = 0; j < n_k && D > 0; ++j) {
        for (int d = 0; d < D; ++d) {
            const double c = h_kvecs[(int64_t)j * D + d];
            if (!(c - c == 0.0)) return fail(owner, TA_E_INVALID, "wavevector " + std::to_string(j) + " has a non-finite component");
        }
        const double n2 = kcur_norm2(D, h_kvecs + (int64_t)j * D);  // (the unit vector divides by its root)
        if (!(n2 > 0.0) || !(n2 - n2 == 0.0))
            return fail(owner, TA_E_INVALID, "wavevector " + std::to_string(j) + " is zero, or too small or too large to normalise "
                                             "(|k|^2 under- or overflows): use ta_current for k = 0");
    }
    return TA_OK;
}
// api.hip, for group.hip: one context's ta_kcurrent share (its staged slabs 0 and 1, the call's wavevectors, checked by the
// caller, its atoms' weights h_w or NULL), queued: *d_out = kcurrent_out's segments (long and trans with correlate), valid
// after host_wait; and the two correlations of a host current on the context's device, blocking
int kcurrent_launch(ta_ctx* ctx, int fft, int n_k, const double* h_kvecs, const double* h_w, bool correlate, double** d_out);
int kcurrent_correlate_host(ta_ctx* ctx, int fft, const double* h_current, int n_k, const double* h_kvecs, int64_t T, int D,
                            double* h_long, double* h_trans);
// the argument checks of ta_partial_density* on a context (fail, ctx) or a group (gfail, g): the same messages for both, in
// the order of ta_scatter and ta_onsager.  D: the components per wavevector (0: not known, nothing staged -- the caller
// reports that next)
template <class Fail, class Owner>
static int check_partial(Fail fail, Owner* owner, int fft, int n_k, const double* h_kvecs, int D, int S, const void* species,
                         const void* o_density) {
    if (fft != 0 && fft != 1) return fail(owner, TA_E_INVALID, "fft must be 0 or 1");
    if (const int rc = check_species_count(fail, owner, S)) return rc;
    if (!h_kvecs) return fail(owner, TA_E_INVALID, "wavevectors are NULL");
    if (const int rc = check_n_k(fail, owner, n_k)) return rc;
    for (int64_t i = 0; i < (int64_t)n_k * D; ++i)
        if (!(h_kvecs[i] - h_kvecs[i] == 0.0))
            return fail(owner, TA_E_INVALID, "wavevector " + std::to_string(i / D) + " has a non-finite component");
    if (!species) return fail(owner, TA_E_INVALID, "species labels are NULL");
    if (!o_density) return fail(owner, TA_E_INVALID, "partial density output is NULL");
    return TA_OK;
}
// api.hip, for group.hip: one context's ta_partial_density share (its staged slab 0, the call's wavevectors, checked by the
// caller, its atoms' labels h_species (checked by the caller) and weights h_w or NULL), queued: *d_out = partial_out's
// segments (the cross term with cross), valid after host_wait; and the cross term of a host density on the context's
// device, blocking
int partial_launch(ta_ctx* ctx, int fft, int n_k, const double* h_kvecs, int S, const int32_t* h_species, const double* h_w,
                   bool cross, double** d_out);
int partial_cross_host(ta_ctx* ctx, int fft, const double* h_density, int n_k, int S, int64_t T, double* h_cross);
// the argument checks the van Hove families share, on a context (fail, ctx) or a group (gfail, g), under the family's
// message prefix `p`: the lags' array, the counts and the bin width ...
template <class Fail, class Owner>
static int check_vanhove_grid(Fail fail, Owner* owner, const std::string& p, int n_lags, const int64_t* h_lags, int n_bins, double dr) {
    if (!h_lags) return fail(owner, TA_E_INVALID, p + "lags are NULL");
    if (n_lags < 1 || n_lags > TA_VANHOVE_MAX_LAGS)
        return fail(owner, TA_E_INVALID, p + "n_lags must be 1 ... " + std::to_string(TA_VANHOVE_MAX_LAGS));
    if (n_bins < 1 || n_bins > TA_VANHOVE_MAX_BINS)
        return fail(owner, TA_E_INVALID, p + "n_bins must be 1 ... " + std::to_string(TA_VANHOVE_MAX_BINS));
    if (!(dr - dr == 0.0) || !(dr > 0.0)) return fail(owner, TA_E_INVALID, p + "dr must be finite and > 0");
    return TA_OK;
}
// ... and, after the family's own checks, the lags against T frames (0: not known, nothing staged -- the caller reports
// that next)
template <class Fail, class Owner>
static int check_vanhove_lags(Fail fail, Owner* owner, const std::string& p, int n_lags, const int64_t* h_lags, int64_t T) {
    for (int l = 0; l < n_lags; ++l) {
        if (h_lags[l] < 0 || (T > 0 && h_lags[l] >= T))
            return fail(owner, TA_E_INVALID, p + "lag " + std::to_string(h_lags[l]) + " is outside 0 ... n_frames - 1");
        if (l && h_lags[l] <= h_lags[l - 1]) return fail(owner, TA_E_INVALID, p + "the lags must be strictly increasing");
    }
    return TA_OK;
}
// the argument checks of ta_vanhove* (context or group: the same messages for both)
template <class Fail, class Owner>
static int check_vanhove(Fail fail, Owner* owner, int n_lags, const int64_t* h_lags, int n_bins, double dr, int64_t T,
                         bool any_output) {
    if (const int rc = check_vanhove_grid(fail, owner, "vanhove: ", n_lags, h_lags, n_bins, dr)) return rc;
    if (!any_output) return fail(owner, TA_E_INVALID, "vanhove: the counts and moments outputs are both NULL");
    return check_vanhove_lags(fail, owner, "vanhove: ", n_lags, h_lags, T);
}
// api.hip, for group.hip: one context's ta_vanhove share (its staged slab 0, the call's lags and bins, checked by the
// caller), queued: *d_out = vanhove_out's segments -- the ones asked for are valid after host_wait
int vanhove_launch(ta_ctx* ctx, int n_lags, const int64_t* h_lags, int n_bins, double dr, bool counts, bool moments, double** d_out);
// the argument checks of ta_overlap* (context or group: the same messages for both), all of them before anything is written.
// T: the frames (0: not known, nothing staged -- the caller reports that next).  check_overlap_lists: the lags, the cutoffs and
// the output under the family's message prefix `p`, shared with ta_overlap_density*
template <class Fail, class Owner>
static int check_overlap_lists(Fail fail, Owner* owner, const std::string& p, int n_lags, const int64_t* h_lags, int n_cutoffs,
                               const double* h_cutoffs, int64_t T, bool any_output) {
    if (!h_lags) return fail(owner, TA_E_INVALID, p + "lags are NULL");
    if (n_lags < 1 || n_lags > TA_VANHOVE_MAX_LAGS)
        return fail(owner, TA_E_INVALID, p + "n_lags must be 1 ... " + std::to_string(TA_VANHOVE_MAX_LAGS));
    if (!h_cutoffs) return fail(owner, TA_E_INVALID, p + "cutoffs are NULL");
    if (n_cutoffs < 1 || n_cutoffs > TA_OVERLAP_MAX_CUTOFFS)
        return fail(owner, TA_E_INVALID, p + "n_cutoffs must be 1 ... " + std::to_string(TA_OVERLAP_MAX_CUTOFFS));
    for (int c = 0; c < n_cutoffs; ++c) {
        const double a = h_cutoffs[c];
        if (!(a - a == 0.0) || !(a > 0.0)) return fail(owner, TA_E_INVALID, p + "cutoff " + std::to_string(c) + " must be finite and > 0");
        if (c && !(a > h_cutoffs[c - 1])) return fail(owner, TA_E_INVALID, p + "the cutoffs must be strictly increasing");
    }
    if (!any_output) return fail(owner, TA_E_INVALID, p + "the output is NULL");
    return check_vanhove_lags(fail, owner, p, n_lags, h_lags, T);
}
template <class Fail, class Owner>
static int check_overlap(Fail fail, Owner* owner, int n_lags, const int64_t* h_lags, int n_cutoffs, const double* h_cutoffs,
                         int64_t T, bool any_output) {
    const std::string p = "overlap: ";
    if (const int rc = check_overlap_lists(fail, owner, p, n_lags, h_lags, n_cutoffs, h_cutoffs, T, any_output)) return rc;
    if ((int64_t)n_cutoffs * n_lags * T > (int64_t)1 << 27)
        return fail(owner, TA_E_INVALID, p + "n_cutoffs * n_lags * n_frames = " + std::to_string((int64_t)n_cutoffs * n_lags * T) +
                                             " exceeds 2^27 (1 GiB of output): fewer lags or cutoffs per call");
    return TA_OK;
}
// the argument checks of ta_overlap_density* (context or group: the same messages for both), all of them before anything is
// allocated or written: the wavevectors as ta_partial_density's, then ta_overlap's lists under this family's prefix, the
// output and its size.  T, D: the frames and the components per wavevector (0: not known, nothing staged -- the caller
// reports that next)
template <class Fail, class Owner>
static int check_overlap_density(Fail fail, Owner* owner, int n_k, const double* h_kvecs, int D, int n_lags, const int64_t* h_lags,
                                 int n_cutoffs, const double* h_cutoffs, int64_t T, bool any_output) {
    const std::string p = "overlap_density: ";
    if (!h_kvecs) return fail(owner, TA_E_INVALID, p + "wavevectors are NULL");
    if (const int rc = check_n_k(fail, owner, n_k, p)) return rc;
    for (int64_t i = 0; i < (int64_t)n_k * D; ++i)
        if (!(h_kvecs[i] - h_kvecs[i] == 0.0))
            return fail(owner, TA_E_INVALID, p + "wavevector " + std::to_string(i / D) + " has a non-finite component");
    if (const int rc = check_overlap_lists(fail, owner, p, n_lags, h_lags, n_cutoffs, h_cutoffs, T, any_output)) return rc;
    const int64_t n_out = (int64_t)n_k * n_cutoffs * n_lags * T;  // (<= 2^12 2^2 2^10 T)
    if (n_out > (int64_t)1 << 26)
        return fail(owner, TA_E_INVALID, p + "n_k * n_cutoffs * n_lags * n_frames = " + std::to_string(n_out) +
                                             " exceeds 2^26 (1 GiB of output): fewer wavevectors, lags or cutoffs per call");
    return TA_OK;
}
// api.hip, for group.hip: one context's ta_overlap_density share (its staged slab 0, the call's wavevectors, lags and
// cutoffs, checked by the caller), queued: *d_out = overlap_density_out's segment, valid after host_wait
int overlap_density_launch(ta_ctx* ctx, int n_k, const double* h_kvecs, int n_lags, const int64_t* h_lags, int n_cutoffs,
                           const double* h_cutoffs, double** d_out);
// api.hip, for group.hip: one context's ta_overlap share (its staged slab 0, the call's lags and cutoffs, checked by the
// caller), queued: *d_out = overlap_out's segment, valid after host_wait
int overlap_launch(ta_ctx* ctx, int n_lags, const int64_t* h_lags, int n_cutoffs, const double* h_cutoffs, double** d_out);
// api.hip, for group.hip: one context's ta_unwrap queued on its stream (box.tab must stay valid until host_wait)
int unwrap_launch(ta_ctx* ctx, int slab, const BoxTable& box, const int* axes);
hipStream_t ctx_stream(ta_ctx* ctx);
int ctx_device(const ta_ctx* ctx);
int64_t ctx_staged_frames(const ta_ctx* ctx);
int ctx_fail(ta_ctx* ctx, int code, const std::string& msg);  // records the message, returns code
void host_zero(void* p, size_t bytes);  // stage_host.hip: memset 0 on several threads, streaming stores
// stage_host.hip: an anonymous, zero-filled, huge-page backed mapping that is page-locked (hipHostRegister) chunk by
// chunk on demand; copies out of it must not span two chunks
struct HostBlock {
    static constexpr size_t kChunk = (size_t)64 << 20;
    char* base = nullptr;
    size_t bytes = 0;               // mapped length: a multiple of kChunk
    std::vector<unsigned char> locked;  // per chunk
};
int host_block_map(size_t bytes, HostBlock* b);                    // 0, or -1 when the mapping fails
hipError_t host_block_lock(HostBlock& b, size_t b0, size_t b1);    // page-lock the chunks covering [b0, b1)
void host_block_unmap(HostBlock& b);

// direct.hip
// vel / pos: pair-major slabs (layout.hip) of `pitch` rows per pair, float64 or (src_f32, with the
// float32 arithmetic path only) float32 elements
hipError_t launch_direct(int mode, bool f32, bool src_f32, int L, const void* vel, const void* pos,
                         const double* masses, long pitch, int T, long n_atoms, int D,
                         double scale, double* by_particle, long ld_bp, double* ts_partial, int nwg,
                         int nt, size_t lds_bytes, void* stage_buf, int gnt, hipStream_t st);
bool direct_chunk_supported(int L);       // lags per chunk compiled in (8, 10)
size_t direct_lds_bytes(int T, bool f32, int L);
int direct_max_wg_per_cu(int mode, bool f32, int L, int nt, size_t lds_bytes, bool global_stage);

// band32tp.hip: the float32 product slab of the Einstein-Helfand float32 option: P32 = float32((m v) x) in a pair-major float32
// slab (vel / pos: pair-major float64 slabs, or float32 ones with src_f32)
hipError_t launch_helfand_product32(const void* vel, const void* pos, bool src_f32, const double* masses, long pitch, long T,
                                    long n_cols, int D, float* P32, hipStream_t st);

// short.hip: trajectories of up to short_max_frames() frames, a lane per column (short_kernels.hpp); bp (n_frames, ld_bp) or
// NULL; partial [nwg * short_waves()][T] lag sums per wave (normalised); factor 1 (VACF) or scale / D (Helfand)
int short_max_frames();
int short_waves();
int short_grid(int n_cu, int mode, int T, long n_atoms, int D, bool by_particle);
hipError_t launch_short(int mode, int nwg, const double* vel, const double* pos, const double* masses, long pitch, int T,
                        long n_atoms, int D, double factor, double* bp, long ld_bp, double* partial, hipStream_t st);

// mid.hip: 65 ... mid_max_frames() frames, a lane per (column, pair of 16-lag blocks) walking a sliding window (mid_kernels.hpp);
// bp (n_frames, ld_bp) or NULL; partial [nwg][T]; factor 1 (VACF) or scale / D (Helfand)
struct MidShape {
    int ncl_log2, nc, ts, threads;
    size_t lds;
};
int mid_max_frames();
MidShape mid_shape(int T, int D, int ncl_log2 = 0);  // ncl_log2 3..6: lanes per pair of blocks forced (0: by n_frames)
int mid_grid(int n_cu, int mode, int T, long n_atoms, int D, int ncl_log2);
hipError_t launch_mid(int mode, int nwg, const double* vel, const double* pos, const double* masses, long pitch, int T,
                      long n_atoms, int D, double factor, double* bp, long ld_bp, double* partial, int ncl_log2, hipStream_t st);

hipError_t launch_row_sums(const double* bp, long n_rows, long n_cols, long ld, double* out,
                           hipStream_t st);
// bandbp.hip: the windowed VACF with its by-particle array on the FP64 matrix cores (atom-major scratch, zeroed inside)
hipError_t launch_band_bp_vacf(int n_cu, const double* pm, long pitch, int T, long n_atoms, int D, double* bp_am, long ld_am,
                               unsigned long long* next_unit, hipStream_t st);
hipError_t launch_band_bp_vacf_lags(int n_cu, const double* pm, long pitch, int T, long n_atoms, int D, double* partial,
                                    unsigned long long* next_unit, double* lagsum, hipStream_t st);
hipError_t launch_band_bp_helf(int n_cu, const double* P, long pitch, int T, long n_atoms, int D, double factor, double* bp_am,
                               long ld_am, unsigned long long* next_unit, hipStream_t st);
int band_bp_helf_block(int n_cu, int T, long n_atoms);
size_t band_bp_helf_partial_doubles(int n_cu, int T, long n_atoms);
// band32tp.hip: the float32 option's Helfand forms, k-slots from the time axis
hipError_t launch_band32_tp_bp(int n_cu, const float* P32, long pitch, int T, long n_atoms, int D, double factor, double* bp_am, long ld_am,
                               unsigned long long* next_unit, hipStream_t st);
hipError_t launch_band32_tp_lags(int n_cu, const float* P32, long pitch, int T, long n_atoms, int D, double factor, double* partial,
                                 unsigned long long* next_unit, double* lagsum, hipStream_t st);
hipError_t launch_band_bp_helf_lags(int n_cu, const double* P, long pitch, int T, long n_atoms, int D, double factor, double* partial,
                                    unsigned long long* next_unit, double* lagsum, hipStream_t st);
hipError_t launch_sum_partials(const double* partial, int n_parts, long n, double* out,
                               hipStream_t st);
// helfand_fft.hip: optional FFT evaluation of the Helfand lag sums
// pair-major slabs in, product slab P out in the same layout; Qpart [n_parts][T] written in full
hipError_t launch_helfand_product(const double* vel, const double* pos, const double* masses,
                                  long pitch, long T, long n_cols, int D, double* P, double* Qpart,
                                  int n_parts, hipStream_t st);
hipError_t launch_helfand_combine(const double* Q, const double* s2n, double* C, int T, double factor,
                                  double* out, hipStream_t st);
hipError_t launch_helfand_product_bp(const double* vel, const double* pos, const double* masses,
                                     long pitch, long T, long n_atoms, int D, double* P, double* Ca,
                                     hipStream_t st);  // Ca: (T+1, n_atoms)
hipError_t launch_helfand_combine_bp(double* Ca, long n_atoms, int T, double factor, double* bp,
                                     long ld_bp, hipStream_t st);

// msd.hip: the FFT form of the Einstein MSD.  P = x - x[t=0] per column into a pair-major slab (the unpaired last column's
// partner written as 0); Qpart [n_parts][T] written in full (lag sums) or Ca rows 1..T of (T+1, n_atoms) (by particle); the
// helfand_combine kernels above finish with factor 1
hipError_t launch_msd_prepare(const double* pos, long pitch, long T, long n_cols, double* P, double* Qpart, int n_parts,
                              hipStream_t st);
hipError_t launch_msd_prepare_bp(const double* pos, long pitch, long T, long n_atoms, int D, double* P, double* Ca,
                                 hipStream_t st);

// conductivity.hip: the charge-weighted moment M[t, d] = sum_n q_n (x[t, n, d] - x[0, n, d]) of a float64 pair-major
// slab as n_parts partial sums partial [n_parts][T][D] (written in full; k_sum_partials adds them in order), and with
// W != NULL the weighted shifted slab W = q (x - x[0]) in the same layout (rows < T; an unpaired column's partner 0)
int cond_moment_parts(int n_cu, long T, long n_cols);
hipError_t launch_cond_moment(const double* pos, long pitch, long T, long n_cols, int D, const double* q, double* partial,
                              int n_parts, double* W, hipStream_t st);

// species_sum.hip: the species sums Q[s, t, d] = sum_{n: species[n] = s} w_n (x[t, n, d] - shift x[0, n, d]) of a pair-major
// slab of float64 or (f32, without shift only) float32 elements in one pass over it as it is, as n_parts partial sums
// partial [n_parts][S][T][D] (written in full; n_parts from species_sum_parts; k_sum_partials adds them in order);
// species: (n_atoms,) int32 device labels, one outside [0, S) is skipped; w: (n_atoms,) weights or NULL (all 1).
// combos: the pair-major slab (pitch rows per pair) of the S^2 pseudo-particles Q_i, Q_i + Q_j, Q_i - Q_j of the sums
// Q (S, T, D), and nz[s] != 0 where Q_s has a non-zero element (nz zeroed by the caller); finish: C (T, S, S) from their
// (T, S^2) by-particle lag sums, lag 0 kept (lag0) or exactly 0
int species_sum_parts(int n_cu, int S, long T, long n_cols);
hipError_t launch_species_sum(const void* pm, bool f32, bool shift, long pitch, long T, long n_cols, int D, int S,
                              const int* species, const double* w, double* partial, int n_parts, hipStream_t st);
hipError_t launch_onsager_combos(const double* M, int S, long T, int D, long pitch, double* pm, int* nz, hipStream_t st);
hipError_t launch_cross_finish(const double* bp, int S, long T, const int* nz, bool lag0, double* C, hipStream_t st);

// species_self.hip: the weighted slab W = w (x - shift x[0]) of a pair-major slab of float64 or (f32) float32 elements with
// each species' atoms contiguous, as a float64 pair-major slab of plan.n_pairs pairs: species s's block starts at pair
// plan.pair0[s] and is a slab of count[s] atoms of its own (a phantom last column and the rows T ... pitch - 1 written as
// zeros).  species_sort_plan: the blocks and order (n_atoms,) = the atoms species by species, input order kept, from
// host labels in [0, S) (checked by the caller); order goes to the device, one int32 per atom.
struct SortPlan {
    int n_species, n_units;  // units: two consecutive atoms of one species in sorted order
    long n_pairs;
    int count[TA_ONSAGER_MAX_SPECIES], pos0[TA_ONSAGER_MAX_SPECIES], unit0[TA_ONSAGER_MAX_SPECIES];
    long pair0[TA_ONSAGER_MAX_SPECIES];
};
void species_sort_plan(const int32_t* h_species, int64_t n_atoms, int D, int S, SortPlan* plan, int32_t* order);
hipError_t launch_species_sort(int n_cu, const void* x, bool f32, long pitch, long T, long n_cols, int D, const SortPlan& plan,
                               const int* order, const double* w, bool shift, double* W, hipStream_t st);

// compound.hip: the float64 pair-major slab of n_compounds compounds of a pair-major slab of float64 or (f32) float32 elements,
// read as it is: out[t, D c + d] = sum_{i in [off[c], off[c + 1])} w_i x[t, D member[i] + d] - g[c] F[t, d], in member order.
// off (n_compounds + 1), member, w (or NULL: all 1; one per member entry), g (n_compounds) and F ((T, D), or NULL: no such
// term) are device arrays; out has (n_compounds D + 1) / 2 pairs of `pitch` rows, every one of them written.
hipError_t launch_compound(int n_cu, const void* x, bool f32, long pitch, long T, long n_cols, int D, long n_compounds,
                           const int* off, const int* member, const double* w, const double* g, const double* F, double* out,
                           hipStream_t st);

// scatter.hip: the phase slab Z of Kc wavevectors q (Kc, D) (device array, turns per length unit) of a pair-major slab of
// float64 or (f32) float32 elements, read as it is: pair jl n_atoms + n of Z = rows (cos, sin)(2 pi q_jl . x[t, n]), `pitch`
// rows per pair, rows T ... pitch - 1 zeros; and the (T, K) -> (K, T) transposition of the collective part
hipError_t launch_phase(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, const double* q, int Kc,
                        double* Z, hipStream_t st);
hipError_t launch_scatter_transpose(const double* bp, long T, long K, double* out, hipStream_t st);

// orient.hip: one float64 pair-major block of the orientation columns of n_vectors vectors (orient_math.hpp: mode, the index
// rows of orient_row_len(mode) atoms, device int32) of a pair-major slab of float64 or (f32) float32 elements with D = 3, read
// as it is: rank 1 = n_vectors atoms of dim 3 holding u, rank 2 = 2 n_vectors pseudo-atoms of dim 3 holding Q's six columns;
// `pitch` rows per pair, rows T ... pitch - 1 zeros; Z has 3 n_vectors pairs.  box: NULL (no image step) or the device table
// of kOrientBoxRows rows of tpitch doubles (tpitch 1: one constant box; else one box per frame, tpitch >= T)
hipError_t launch_orient(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, int mode, int rank,
                         long n_vectors, const int* index, const double* box, long tpitch, double* Z, hipStream_t st);

// chain_modes.hip: the blocks of n_q <= tile modes linear functionals (coeff (n_q, chain_len), device float64) of n_chains
// chains (member (n_chains, chain_len), device int32: atoms of the slab in backbone order) of a pair-major slab of float64 or
// (f32) float32 elements with D = 3, read as it is (chain_math.hpp: the chain made whole bead by bead).  Z: n_q float64
// pair-major blocks behind each other, each n_chains pseudo-atoms of dim 3 = ceil(3 n_chains / 2) pairs of `pitch` rows, rows
// T ... pitch - 1 and the phantom column zeros.  box: as launch_orient's.  chain_modes_tile: the modes per launch and the
// frames per thread of the one tile (a workgroup covers 256 frames of them).
hipError_t launch_chain_modes(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, long n_chains, int chain_len,
                              const int* member, const double* coeff, int n_q, const double* box, long tpitch, double* Z,
                              hipStream_t st);
void chain_modes_tile(int* modes, int* frames);

// kcurrent.hip: the k-space current of kc <= KC wavevectors q (kc, D) (device array, turns per length unit) from the pair-major
// slabs v (velocities) and x (positions) of float64 or (f32) float32 elements, both read as they are, in one pass: partial
// [n_parts][kc][T][D] (re, im) sums over the atoms g, g + n_parts, ... of w_n v (cos, sin)(2 pi q . x) (written in full;
// n_parts from kcurrent_parts, which depends on the slab and the device only; k_sum_partials adds them in order); w:
// (n_atoms,) device weights or NULL (all 1).  kcurrent_tile: KC and the frames per thread on a float64 / float32 slab.
// project: the pair-major slab (pitch rows per pair, dim 2) of the K kcur_series(D) pseudo-atoms jL, jT_d of a current
// (K, T, D, 2) with the unit vectors khat (K, D); finish: lon (K, T), trans (K, T) (either may be NULL) from their
// (T, K kcur_series(D)) by-particle autocorrelations (kcurrent_math.hpp)
void kcurrent_tile(int* kc, int* frames_f64, int* frames_f32);
int kcurrent_parts(int n_cu, bool f32, long pitch, long n_atoms, int D, size_t budget);
hipError_t launch_kcurrent(const void* v, const void* x, bool f32, long pitch, long T, long n_atoms, int D, const double* q,
                           int kc, const double* w, double* partial, int n_parts, hipStream_t st);
hipError_t launch_kcurrent_project(const double* current, const double* khat, int K, long T, int D, long pitch, double* pm,
                                   hipStream_t st);
hipError_t launch_kcurrent_finish(const double* bp, int K, long T, int D, double* lon, double* trans, hipStream_t st);

// species_density.hip: the species-resolved density of kc <= KC wavevectors q (kc, D) (device array, turns per length unit) and
// S species from the pair-major position slab x of float64 or (f32) float32 elements, read as it is, in one pass: partial
// [n_parts][kc][S][T] (re, im) sums over the atoms g, g + n_parts, ... of w_n (cos, sin)(2 pi q . x), each into the row of
// its label (written in full; n_parts from species_density_parts, which depends on the slab and the device only;
// k_sum_partials adds them in order); species: (n_atoms,) int32 device labels, one outside [0, S) is skipped; w: (n_atoms,)
// device weights or NULL (all 1).  species_density_tile: the species slots ST and the wavevectors per launch KC of the tile
// that serves n_species, and the frames per thread on a float64 / float32 slab (false: n_species outside 1 ... 8).
// finish: C (B, T, S, S) of a batch of B wavevectors from the (T, B S^2) by-particle autocorrelations of their pseudo-particles
// (launch_onsager_combos per wavevector, dim 2) and the flags nz (B, TA_ONSAGER_MAX_SPECIES); lag 0 is kept
bool species_density_tile(int n_species, int* st, int* kc, int* frames_f64, int* frames_f32);
int species_density_parts(int n_cu, bool f32, long pitch, long n_atoms, size_t budget);
hipError_t launch_species_density(const void* x, bool f32, long pitch, long T, long n_atoms, int D, const double* q, int kc, int S,
                                  const int* species, const double* w, double* partial, int n_parts, hipStream_t st);
hipError_t launch_partial_finish(const double* bp, int B, int S, long T, const int* nz, double* C, hipStream_t st);

// vanhove.hip: the self van Hove histogram of a pair-major slab of float64 or (f32) float32 elements, read as it is, for the
// lags [l0, l0 + Lc) of L (device array `lags`): counts (L, B + 1) uint64 (zeroed by the caller before the first chunk)
// gets the chunk's bins added, partial [vanhove_parts][L][2] the chunk's (sum r2, sum r2 r2) per workgroup (k_sum_partials
// adds them in order once every chunk has run).  e: the B + 1 squared edges (device), inv_dr: the float32 bin guess's
// factor (vanhove_math.hpp).  vanhove_max_chunk: the lags per launch that fit a workgroup's LDS (at least 1).
int vanhove_max_chunk(int B);
int vanhove_parts(int n_cu, long pitch, long n_atoms);
hipError_t launch_vanhove(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, const int64_t* lags, int l0,
                          int Lc, int L, const double* e, int B, float inv_dr, unsigned long long* counts, double* partial,
                          hipStream_t st);

// overlap.hip: the self-overlap per origin of a pair-major slab of float64 or (f32) float32 elements, read as it is, for the
// lags [l0, l0 + Lc) of L (device array `lags`) and C cutoffs with squared values a2 (device): q (C, L, T) uint64 (zeroed by
// the caller before the first launch) gets the launch's counts added.  Lc C <= overlap_slots(), the kernel's tile.
int overlap_slots();
hipError_t launch_overlap(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, const int64_t* lags, int l0,
                          int Lc, int L, const double* a2, int C, unsigned long long* q, hipStream_t st);

// overlap_density.hip: the overlap field's density per origin of a pair-major slab of float64 or (f32) float32 elements, read
// as it is, for the lags [l0, l0 + Lc) of L (device array `lags`), C cutoffs with squared values a2 (device) and kc <= KC
// wavevectors q (kc, D) (device, turns per length unit): partial [n_parts][kc][Lc C][T] (re, im) sums over the atoms g, g +
// n_parts, ... (written in full; n_parts from overlap_density_parts, which depends on the slab and the device only).
// sum: w[jl, c, l, t] (the launch's corner of W (K, C, L, T, 2)) = the parts added in k_sum_partials' order.
// overlap_density_tile: the (lag, cutoff) slots SL, the wavevectors KC and the frames per thread of the one tile.
void overlap_density_tile(int* slots, int* kc, int* frames);
int overlap_density_parts(int n_cu, long pitch, long n_atoms, size_t budget);
hipError_t launch_overlap_density(const void* x, bool f32, long pitch, long T, long n_atoms, int D, const int64_t* lags, int l0,
                                  int Lc, int L, const double* a2, int C, const double* q, int kc, double* partial, int n_parts,
                                  hipStream_t st);
hipError_t launch_overlap_density_sum(const double* partial, int n_parts, long T, int Lc, int C, int L, int kc, double* w,
                                      hipStream_t st);

// vanhove_distinct.hip: the distinct van Hove histogram in two passes.  The item pitches of the scratch and of the padded
// index lists (ids; -1: padding) are multiples of the pair kernel's tiles.  n_orig = ceil(T / stride): the origins of lag 0,
// which size the scratch of every lag.
//   launch_vhd_gather: the frame-major float64 scratch of a chunk of Lc lags (device array `lags`: the chunk's) from a
//   pair-major slab of float64 or (f32) float32 elements, read as it is: ga [n_orig][D][pitch_a] (with_a: written by this
//   launch), gb [Lc][n_orig][D][pitch_b]; rows at or past T are neither read nor written.  o_base: origin 0 of the scratch
//   is origin o_base of the slab (the pair search gathers its frames in chunks; 0: the whole set of origins).
//   launch_vhd_pairs: origins [o0, o0 + n_o) (n_o <= 65535) of the chunk's lags: counts (Lc, B + 1) uint64 (zeroed by the
//   caller before the first launch) gets the bins added.  hm: NULL (no box) or per box H[3], M[3] of the staged columns
//   (one box, or one per frame: box_per_frame); e: the B + 1 squared edges (device), inv_dr: vanhove_math.hpp's factor.
constexpr int VHD_TILE_A = 256, VHD_TILE_B = 1024;
constexpr long VHD_MAX_TILES = 1L << 24;  // a-tiles x b-tiles of one launch: x 256 threads stays below 2^32
hipError_t launch_vhd_gather(const void* x, bool f32, long pitch, long T, long n_atoms, int D, long stride, long n_orig,
                             const int64_t* lags, int Lc, bool with_a, const int* ida, const int* idb, long pitch_a, long pitch_b,
                             double* ga, double* gb, hipStream_t st, long o_base = 0);
hipError_t launch_vhd_pairs(const double* ga, const double* gb, const int* ida, const int* idb, long pitch_a, long pitch_b, long n_a,
                            long n_b, int D, long T, long stride, long n_orig, long o0, int n_o, const int64_t* lags, int Lc,
                            const double* hm, bool box_per_frame, const double* e, int B, float inv_dr, unsigned long long* counts,
                            hipStream_t st);

// pair_lifetime.hip: the pair population correlation functions (pair_math.hpp).
//   launch_pair_find: the searched frames [o_base, o_base + n_o) stride (n_o <= 65535) of the scratch ga [n_o][D][pitch_a],
//   gb [n_o][D][pitch_b] that launch_vhd_gather wrote at lag 0 with the same o_base: bit (p, q) of bitmap [pitch_a][pitch_b /
//   64] (zeroed by the caller before the first chunk) is set where items a_p != b_q are closer than sqrt(rc2) (same: b is a,
//   only q > p).  hm as launch_vhd_pairs'.
//   launch_pair_count / launch_pair_list: counts[block] = the set bits of the block's words (pair_list_blocks(n_words)
//   blocks); with offs[block] their exclusive scan, pairs (n, 2) int32 = the item ids of the set bits in (a, b) order.
//   launch_pair_series: the float64 indicator block Z (ceil(n_pairs / 2) destination pairs of `pitch` rows: n_pairs
//   pseudo-atoms of dim 1, 1.0 / 0.0, rows T ... pitch - 1 and an odd n_pairs' phantom column zeros) of the atom pairs
//   `pairs` (n_pairs, 2) (device int32) of a pair-major slab of float64 or (f32) float32 elements, read as it is.
//   launch_pair_runs: runs[l] += the maximal runs of l consecutive bonded frames of such a block (T + 1 entries, uint64).
//   launch_pair_reduce: out[i] = sum over n_rows rows of n values in row order: as they are (PAIR_SUM), times T - i
//   (PAIR_LAGS: the lag sums carry 1 / (T - i)), or that rounded to the integer it stands for (PAIR_LAGS_INT).
//   launch_bond_series: launch_pair_series for the bonds `atoms` (n_bonds, n_at) of n_at = 2 or 3 items with the cutoffs k
//   (bond_math.hpp): Z gets the level 0.0 / 1.0 / `two` per frame, two = 2.0 where launch_pair_filter follows, else 1.0.
//   launch_pair_filter: such a level block becomes the 0/1 block of the hysteresis-resolved series with absences of up to
//   gap (0 ... 63) frames closed, in place.
enum { PAIR_SUM = 0, PAIR_LAGS = 1, PAIR_LAGS_INT = 2 };
struct BondCuts;
long pair_list_blocks(long n_words);
hipError_t launch_bond_series(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, long n_bonds, int n_at,
                              const int* atoms, const double* hm, bool box_per_frame, const BondCuts& k, double two, double* Z,
                              hipStream_t st);
hipError_t launch_pair_filter(int n_cu, double* Z, long pitch, long T, long n_pairs, int gap, hipStream_t st);
hipError_t launch_pair_find(const double* ga, const double* gb, const int* ida, const int* idb, long pitch_a, long pitch_b, long n_a,
                            long n_b, int D, long T, long stride, long o_base, int n_o, const double* hm, bool box_per_frame,
                            double rc2, bool same, unsigned long long* bitmap, hipStream_t st);
hipError_t launch_pair_count(const unsigned long long* bitmap, long n_words, unsigned* counts, hipStream_t st);
hipError_t launch_pair_list(const unsigned long long* bitmap, long n_words, long words_b, const long long* offs, const int* ida,
                            const int* idb, int* pairs, hipStream_t st);
hipError_t launch_pair_series(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, long n_pairs,
                              const int* pairs, const double* hm, bool box_per_frame, double rc2, double* Z, hipStream_t st);
hipError_t launch_pair_runs(int n_cu, const double* Z, long pitch, long T, long n_pairs, unsigned long long* runs, hipStream_t st);
hipError_t launch_pair_reduce(const double* rows, int n_rows, long n, long T, int mode, double* out, hipStream_t st);

// shell.hip: the level block of the shell residence times.  The frames [f_base, f_base + n_f) of the slab (f_base a multiple of
// 64, at most 65535 64-frame words) are the scratch ga [n_f][D][pitch_a], gb [n_f][D][pitch_b] that launch_vhd_gather wrote at
// lag 0, stride 1, o_base = f_base; pitch_b = ceil(n_b / VHD_TILE_B) VHD_TILE_B.  Rows f_base ... of Z (ceil(n_b / 2) destination
// pairs of `pitch` rows, one pseudo-atom of dim 1 per b-item) get the level 0.0 / 1.0 / `two` of b-item q against ALL a-items
// (bond_math.hpp, shell_level; an a-item with q's id does not count), the launch that holds frame T - 1 also the zeros of the
// rows T ... pitch - 1 and of an odd n_b's phantom column.  hm as launch_vhd_pairs'; two as launch_bond_series'.
hipError_t launch_shell_series(const double* ga, const double* gb, const int* ida, const int* idb, long pitch_a, long pitch_b, long n_a,
                               long n_b, int D, long T, long pitch, long f_base, long n_f, const double* hm, bool box_per_frame,
                               double rc2, double rb2, double two, double* Z, hipStream_t st);

// shell_msd.hip: the shell-resolved MSD of one block of observed items behind k_pair_filter (shell_msd_math.hpp: the conditions,
// the cap kShellMsdMaxLag).  launch_shell_bits: the block Z (ceil(n_items / 2) destination pairs of `pitch` rows, 0/1) -> words,
// n_items rows of ceil(T / 64) packed words.  launch_shell_msd: the items ids[0 ... n_items) (atoms of the slab x, read through
// PmAtom in its own element type and left as it is) over the lags 0 ... max_lag < T under `condition`, origins in chunks of
// `chunk` frames (shell_msd_chunk of the option: a multiple of 64, 64 ... 1024), G workgroups per pass of 256 lags
// (shell_msd_groups of the device, the FULL block's count or fewer); part: shell_msd_part_bytes of the largest G.
// launch_shell_fold: part's G rows added in row order into (first) or onto sums (max_lag + 1, D) and count (max_lag + 1),
// either may be NULL.
int shell_msd_chunk(long option);
int shell_msd_groups(int n_cu, long n_items, long max_lag);
size_t shell_msd_part_bytes(int G, long max_lag, int D);
hipError_t launch_shell_bits(int n_cu, const double* Z, long pitch, long T, long n_items, unsigned long long* words, hipStream_t st);
hipError_t launch_shell_msd(const void* x, bool f32, long pitch, long T, long n_atoms, int D, const int* ids, long n_items,
                            const unsigned long long* words, int condition, long max_lag, int chunk, int G, void* part,
                            hipStream_t st);
hipError_t launch_shell_fold(const void* part, int G, long max_lag, int D, bool first, double* sums, long long* count, hipStream_t st);

// shell_orient.hip: the shell-resolved reorientation of one block of observed items, between launch_shell_bits and
// launch_shell_fold (D = 2) and with launch_shell_msd's words, lags, chunk, G and part (two sums per lag).  index: the block's
// n_items rows of orient_row_len(mode) atoms of the slab x (dim 3), one per observed item (the vector's anchor), device int32;
// hm: NULL or the distance pass's boxes (H[3], M[3] per box; per_frame: one per frame), the image step's orthorhombic box
hipError_t launch_shell_orient(const void* x, bool f32, long pitch, long T, long n_atoms, int D, int mode, const int* index, long n_items,
                               const double* hm, bool per_frame, const unsigned long long* words, int condition, long max_lag, int chunk,
                               int G, void* part, hipStream_t st);

// unwrap.hip: NoJump unwrapping of a float64 pair-major slab in place (rows < T; an unpaired column's partner untouched),
// box table of unwrap_box.hpp on the device (tpitch rows per entry; a constant box: element 0)
hipError_t launch_unwrap(double* slab, long pitch, long T, long n_atoms, int D, const int* axes, bool triclinic,
                         bool per_frame, const double* d_tab, long tpitch, hipStream_t st);

hipError_t launch_widen_f32(const float* in, double* out, long n, hipStream_t st);

// layout.hip: frame-major (n_frames, ld_row) float32/float64 rows -> pair-major slab rows
// (dst_f32 / pm_f32: the slab holds float32 elements)
hipError_t launch_relayout(const void* src, bool src_f32, long ld_row, long n_cols, long t_count,
                           void* dst, bool dst_f32, long pitch, long t_dst0, hipStream_t st);
hipError_t launch_unlayout(const void* pm, bool pm_f32, long pitch, long n_cols, long t_count, double* dst,
                           long ld_row, hipStream_t st);
// atom-major by-particle scratch -> (n_frames, ld_bp); partial: [ceil(n_atoms/64)][T] or NULL; split_div: the lags
// 256 g + 241 ... 256 g + 255 hold undivided sums (k_band_bp_vacf), divided by T - lag on the way
hipError_t launch_bp_transpose(const double* src, long src_ld, long n_atoms, long T, double* bp, long ld_bp,
                               double* partial, hipStream_t st, bool split_div = false);
hipError_t launch_synth(void* pm, bool pm_f32, long pitch, long n_cols, long T, unsigned long long seed,
                        long col_offset, long n_cols_total, hipStream_t st);

// wfft.hip: FFT evaluation on pair-major slabs, padded length L = 2 R R0 512 (wfft.hpp)
bool wfft_choose(long n_frames, int* R0, int* R);  // smallest R R0 512 >= n_frames
size_t wfft_table_elems(int R0, int R);
void wfft_fill_table(int R0, int R, cd* table);
int wfft_max_wg_per_cu(int R0);
int wfft_threads(int R0);
// forward kernel (R0 > 1), nwg a multiple of 16 R: lag-sum mode n_units column pairs ->
// accg [nwg / 2R][L] partial spectra; by-particle mode n_units atoms -> accg [n_units][L]
// src_f32: pm points at a float32 slab (8-byte rows); R = 1 only
hipError_t launch_wfft_forward(int R0, int R, bool by_particle, bool src_f32, int nwg, hipStream_t st, const double* pm,
                               long pitch, int T, long n_units, int D, const cd* tw, double* accg);
// the lag-sum forward kernel built with in-kernel clock stamps (plans R0 = 8, 10, 12, 16, 20 without an
// outer radix): stamps[16 * workgroup + ...], see wfft.hpp (ta_clock_probe)
hipError_t launch_wfft_forward_stamp(int R0, int nwg, hipStream_t st, const double* pm, long pitch, int T,
                                     long n_units, const cd* tw, double* accg, unsigned long long* stamps);
// inverse kernel (R0 > 1): lag values of n_items spectra, out[item * ld + lag]
hipError_t launch_wfft_inverse(int R0, int R, int nwg, hipStream_t st, const double* spec, int T, long n_items,
                               const cd* tw, double* out, long ld, int prefetch);
// n_frames <= 512 (R0 = 1): lag-sum kernel (accg [4 nwg][1024], natural bin order) with its
// finish (sum, cosine sums), and the fused by-particle kernel (atom-major out[atom * ld + lag])
hipError_t launch_w1_accum(int nwg, hipStream_t st, const double* pm, long pitch, int T, long n_pairs,
                           const cd* tw, double* accg);
hipError_t launch_w1_bp(int nwg, hipStream_t st, const double* pm, long pitch, int T, long n_atoms, int D,
                        const cd* tw, double* out, long ld);
hipError_t launch_wfft_finish(int R0, const double* partial, int n_parts, const cd* tw, int T,
                              double* spec /* [2M] */, double* lagsum, hipStream_t st);

}  // namespace ta
