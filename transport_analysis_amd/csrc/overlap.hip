// overlap.hip — the self-overlap per time origin, the sum behind the four-point susceptibility chi_4: for L lags tau_l and C
// cutoffs a_c the number of atoms that have moved less than a_c between an origin frame t0 and t0 + tau_l
//
//   Q[c, l, t0] = #{n: r2 < a2[c]},  r2 = |x[t0 + tau_l, n] - x[t0, n]|^2,  t0 < T - tau_l  (0 from there on)     uint64 (C, L, T)
//
// with r2 of vanhove_math.hpp and a2 = fl(a a) (vh_cutoffs2; the CPU backend follows both: equal counts for any input).
// The slab is read as it is, a float32 one as float32, with k_vanhove's work split and reads (vanhove.hip).  What differs is
// the reduction: k_vanhove adds every origin into one histogram per lag, here the origins stay apart, so a thread keeps a
// uint32 counter per (slot, origin frame of its own) in registers across its whole atom loop -- a slot being one (lag, cutoff)
// of the launch -- and adds the non-zero ones to Q once, at the end.  No LDS, no atomics inside the loop.
//
// Determinism.  Integers only: the 64-bit adds into Q give the same bits in any order, and for any number of lags per launch.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pm_read.hpp"
#include "ta_internal.hpp"
#include "vanhove_math.hpp"

namespace ta {
namespace {

// (lag, cutoff) slots of one launch: kOvSlots kPmFrames counters per thread.  8: 32 counters; the six instantiations take
// 96 ... 128 VGPRs without scratch, four or five waves per SIMD (the resource-usage report: DESIGN 4.18's table)
constexpr int kOvSlots = 8;
static_assert(kOvSlots >= TA_OVERLAP_MAX_CUTOFFS, "one lag's cutoffs share a launch");

// Workgroup (bx, g) as k_vanhove's: origin frames [1024 bx, 1024 bx + 1024), atoms g, g + G, ... (G = gridDim.y); the atom's
// columns at the thread's kPmFrames origin frames stay in registers across the launch's lags, and the lagged rows are read
// as k_vanhove reads them, by pm_lagged (pm_read.hpp; a pair with t + tau >= T reads row 0 and counts nothing).
// Slot s = l C + c of the launch's lags l < Lc and the cutoffs c < C (Lc C <= kOvSlots).  Every index of cnt and thr is a
// constant after unrolling: the lag loop is not unrolled, and which slots a lag owns is a UNIFORM test per slot.
// lags: the launch's (lags + l0); q: Q + l0 T, its cutoffs q_ld = L T apart.
template <class E, int D>
__global__ void __launch_bounds__(kPmThreads)
    k_overlap(const E* __restrict__ x, long pitch, long T, int n_atoms, const long* __restrict__ lags, int Lc,
              const double* __restrict__ a2, int C, unsigned long long* __restrict__ q, long q_ld) {
    constexpr bool kF32 = std::is_same_v<E, float>;
    constexpr int F = kPmFrames, S = kOvSlots;
    const int n_slots = Lc * C;
    double thr[S];
    unsigned cnt[S][F];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        thr[s] = a2[s < n_slots ? s % C : 0];
#pragma unroll
        for (int f = 0; f < F; ++f) cnt[s][f] = 0;
    }
    const long tb = (long)blockIdx.x * (kPmThreads * F);
    for (int n = blockIdx.y; n < n_atoms; n += gridDim.y) {
        const PmAtom<E, D> a(x, pitch, (unsigned)n);  // (atom D < 2^31: launch_overlap)
        double col[F][3];
        pm_load(a, T, tb, col);
        for (int l = 0; l < Lc; ++l) {
            const long tau = lags[l];
            double r2[F];
            pm_lagged(a, T, tb, tau, [&](int f, bool live, const double(&x1)[3]) { r2[f] = ov_r2<D>(live, col[f], x1); });
            const int s0 = l * C;  // the lag's slots [s0, s0 + C): its cutoffs, smallest first
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (s >= s0 && s < s0 + C) {
#pragma unroll
                    for (int f = 0; f < F; ++f) cnt[s][f] += r2[f] < thr[s] ? 1u : 0u;
                }
            }
        }
    }
    // a counter is non-zero only where t0 + tau < T: nothing at or past Q[c, l, T - tau] is touched
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (s < n_slots) {
            const int l = s / C, c = s - l * C;
            unsigned long long* row = q + (size_t)c * (size_t)q_ld + (size_t)l * (size_t)T;
#pragma unroll
            for (int f = 0; f < F; ++f)
                if (cnt[s][f]) atomicAdd(&row[pm_frame<kF32>(tb, f)], (unsigned long long)cnt[s][f]);
        }
    }
}

}  // namespace

int overlap_slots() { return kOvSlots; }

hipError_t launch_overlap(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, const int64_t* lags, int l0,
                          int Lc, int L, const double* a2, int C, unsigned long long* q, hipStream_t st) {
    if (!pm_slab_ok(pitch, T, n_atoms, D) || C < 1 || C > TA_OVERLAP_MAX_CUTOFFS || Lc < 1 || Lc * C > kOvSlots || l0 < 0 ||
        l0 + Lc > L)
        return hipErrorInvalidValue;
    const dim3 grid = pm_unit_grid(n_cu, pitch, n_atoms);
    const long* lg = pm_lags(lags) + l0;
    unsigned long long* q0 = q + (size_t)l0 * (size_t)T;
    const long q_ld = (long)L * T;
    pm_dispatch(f32, D, [&](auto e, auto d) {
        using E = decltype(e);
        hipLaunchKernelGGL((k_overlap<E, d()>), grid, dim3(kPmThreads), 0, st, (const E*)x, pitch, T, (int)n_atoms, lg, Lc, a2, C, q0,
                           q_ld);
    });
    return hipGetLastError();
}

}  // namespace ta
