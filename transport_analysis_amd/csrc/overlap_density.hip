// overlap_density.hip — the overlap field's density per time origin, the sum behind the four-point structure factor S_4(k, t):
// for K wavevectors k_j, L lags tau_l and C cutoffs a_c
//
//   W[j, c, l, t0] = sum_{n: r2 < a2[c]} (cos, sin)(k_j . x[t0, n]),  r2 = |x[t0 + tau_l, n] - x[t0, n]|^2,  t0 < T - tau_l
//                    (+0.0, +0.0) from there on                                                       float64 (K, C, L, T, 2)
//
// with r2 and a2 exactly ta_overlap's (vanhove_math.hpp) and the phase exactly phase_math.hpp's, of the ORIGIN frame.  The
// slab is read as it is, a float32 one as float32, with k_overlap's work split and reads (overlap.hip).  The phase depends on
// the origin frame only: one sincospi per (atom, owned frame, wavevector of the launch) serves every (lag, cutoff) slot of
// the launch.  A thread keeps one complex sum per (slot, wavevector, owned frame) in registers across its whole atom loop and
// writes them once, as partial sums per group of atoms, which k_overlap_density_sum adds in a fixed order: no atomics.
//
// Determinism.  An entry's partial of atom group g is the sum over the atoms g, g + G, ... in that order, whatever lags and
// wavevectors share its launch, and G depends on the slab and the device only: the same bits for every chunk and run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "phase_math.hpp"
#include "pm_read.hpp"
#include "ta_internal.hpp"
#include "vanhove_math.hpp"

namespace ta {
namespace {

// The tile: SL (lag, cutoff) slots x KC wavevectors x F frames per thread, one complex sum each, in registers: 16 complex
// sums, 64 VGPRs of accumulators.  DESIGN.md section 4.26 has the resource-usage table behind 4 x 2 (against 8 x 1).
constexpr int kOdSlots = 4, kOdKc = 2, kOdFrames = 2;
static_assert(kOdSlots * kOdKc * kOdFrames <= 16, "16 complex sums per thread");
static_assert(kOdSlots >= TA_OVERLAP_MAX_CUTOFFS, "one lag's cutoffs share a launch");
static_assert(kOdFrames % 2 == 0, "a float32 load is two frames");

// Workgroup (bx, g): origin frames [256 F bx, 256 F (bx + 1)), atoms g, g + G, ... (G = gridDim.y).  Per atom the origin
// columns are read once (pm_load) and the phase of each of the launch's wavevectors is formed once per owned frame, before
// the lag loop; per lag the lagged rows come by pm_lagged (pm_read.hpp; a pair with t + tau >= T reads row 0, its r2 is NaN
// and it adds nothing).  Slot s = l C + c of the launch's lags l < Lc and the cutoffs c < C (Lc C <= SL).  Every index of
// are, aim, cs and thr is a constant after unrolling: the lag loop is not unrolled, and which slots a lag owns is a UNIFORM
// test per slot.  The update is a select, acc = inside ? acc + c : acc: an atom outside adds nothing, not even 0 NaN.
// A slot jl >= kc computes on wavevector 0 and stores nothing; a slot s >= Lc C stores nothing.
// lags: the launch's (lags + l0); q: the launch's (q + j0 D); partial[g][jl][s][t] = (re, im), jl < kc, s < Lc C, t < T.
template <class E, int D>
__global__ void __launch_bounds__(kPmThreads)
    k_overlap_density(const E* __restrict__ x, long pitch, long T, int n_atoms, const long* __restrict__ lags, int Lc,
                      const double* __restrict__ a2, int C, const double* __restrict__ q, int kc, double* __restrict__ partial) {
    constexpr bool kF32 = std::is_same_v<E, float>;
    constexpr int F = kOdFrames, SL = kOdSlots, KC = kOdKc;
    const int n_slots = Lc * C;
    double thr[SL], qk[KC][3];
    double are[SL][KC][F], aim[SL][KC][F];
#pragma unroll
    for (int s = 0; s < SL; ++s) {
        thr[s] = a2[s < n_slots ? s % C : 0];
#pragma unroll
        for (int jl = 0; jl < KC; ++jl)
#pragma unroll
            for (int f = 0; f < F; ++f) are[s][jl][f] = 0.0, aim[s][jl][f] = 0.0;
    }
#pragma unroll
    for (int jl = 0; jl < KC; ++jl) {
        const int j = jl < kc ? jl : 0;
        qk[jl][0] = q[j * D], qk[jl][1] = D > 1 ? q[j * D + 1] : 0.0, qk[jl][2] = D > 2 ? q[j * D + 2] : 0.0;
    }
    const long tb = (long)blockIdx.x * (kPmThreads * F);
    for (int n = blockIdx.y; n < n_atoms; n += gridDim.y) {
        const PmAtom<E, D> a(x, pitch, (unsigned)n);  // (atom D < 2^31: launch_overlap_density)
        double col[F][3];
        pm_load(a, T, tb, col);
        double2 cs[KC][F];
#pragma unroll
        for (int jl = 0; jl < KC; ++jl)
#pragma unroll
            for (int f = 0; f < F; ++f) cs[jl][f] = phase_cs<D>(qk[jl][0], qk[jl][1], qk[jl][2], col[f]);
#pragma unroll 1
        for (int l = 0; l < Lc; ++l) {
            const long tau = lags[l];
            double r2[F];
            pm_lagged<F>(a, T, tb, tau, [&](int f, bool live, const double(&x1)[3]) { r2[f] = ov_r2<D>(live, col[f], x1); });
            const int s0 = l * C;  // the lag's slots [s0, s0 + C): its cutoffs, smallest first
#pragma unroll
            for (int s = 0; s < SL; ++s) {
                if (s >= s0 && s < s0 + C) {
#pragma unroll
                    for (int f = 0; f < F; ++f) {
                        const bool inside = r2[f] < thr[s];
#pragma unroll
                        for (int jl = 0; jl < KC; ++jl) {
                            are[s][jl][f] = inside ? are[s][jl][f] + cs[jl][f].x : are[s][jl][f];
                            aim[s][jl][f] = inside ? aim[s][jl][f] + cs[jl][f].y : aim[s][jl][f];
                        }
                    }
                }
            }
        }
    }
    double2* out = reinterpret_cast<double2*>(partial) + (long)blockIdx.y * kc * n_slots * T;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const long t = pm_frame<kF32>(tb, f);
        if (t >= T) continue;
#pragma unroll
        for (int jl = 0; jl < KC; ++jl) {
            if (jl >= kc) continue;
#pragma unroll
            for (int s = 0; s < SL; ++s)
                if (s < n_slots) out[((long)jl * n_slots + s) * T + t] = double2{are[s][jl][f], aim[s][jl][f]};
        }
    }
}

// W[jl, c, l, t] = sum_g partial[g][jl][l C + c][t] in k_sum_partials' order (direct.hip), whose row map (one contiguous
// output) does not fit W's (cutoff, lag) order.  Workgroup (bx, row = jl n_slots + s) takes 16 adjacent doubles of the row's
// 2 T; thread (g, e) adds the parts g, g + 16, ... in two interleaved chains, then the 16 group sums are added in a fixed
// tree: the result does not depend on the launch.  w: W + ((j0 C) L + l0) T 2; its wavevectors C L T 2 doubles apart.
__global__ void __launch_bounds__(256)
    k_overlap_density_sum(const double* __restrict__ partial, int n_parts, long T, int n_slots, int C, long L, long rows,
                          double* __restrict__ w) {
    __shared__ double red[16][17];
    const int tid = threadIdx.x, g = tid >> 4, e = tid & 15;
    const long n = 2 * T, i = (long)blockIdx.x * 16 + e;
    const int row = blockIdx.y, jl = row / n_slots, s = row - jl * n_slots, l = s / C, c = s - l * C;
    const double* src = partial + (long)row * n;
    const long part_ld = rows * n;
    double s0 = 0.0, s1 = 0.0;
    if (i < n) {
        int p = g;
        for (; p + 16 < n_parts; p += 32) {
            s0 += src[(long)p * part_ld + i];
            s1 += src[(long)(p + 16) * part_ld + i];
        }
        if (p < n_parts) s0 += src[(long)p * part_ld + i];
    }
    red[g][e] = s0 + s1;
    __syncthreads();
    for (int h = 8; h > 0; h >>= 1) {
        if (g < h) red[g][e] += red[g + h][e];
        __syncthreads();
    }
    if (g == 0 && i < n) w[(((long)jl * C + c) * L + l) * n + i] = red[0][e];
}

long od_blocks(long pitch) {
    const long fpb = (long)kPmThreads * kOdFrames;
    return (pitch + fpb - 1) / fpb;
}

}  // namespace

void overlap_density_tile(int* slots, int* kc, int* frames) { *slots = kOdSlots, *kc = kOdKc, *frames = kOdFrames; }

int overlap_density_parts(int n_cu, long pitch, long n_atoms, size_t budget) {
    // as species_density_parts: about eight workgroups per CU over the frame blocks, at most one group per atom, and no more
    // than the partial buffer's budget holds: G (SL KC) pitch 16 bytes.  Nothing here depends on the chunk.
    const long n_tb = od_blocks(pitch);
    const long want = (8L * n_cu + n_tb - 1) / n_tb;
    const long fit = (long)(budget / ((size_t)(kOdSlots * kOdKc) * (size_t)pitch * 16));
    return (int)std::max(1L, std::min({want, n_atoms, fit, 65535L}));
}

hipError_t launch_overlap_density(const void* x, bool f32, long pitch, long T, long n_atoms, int D, const int64_t* lags, int l0,
                                  int Lc, int L, const double* a2, int C, const double* q, int kc, double* partial, int n_parts,
                                  hipStream_t st) {
    if (!pm_slab_ok(pitch, T, n_atoms, D) || C < 1 || C > TA_OVERLAP_MAX_CUTOFFS || Lc < 1 || Lc * C > kOdSlots || l0 < 0 ||
        l0 + Lc > L || kc < 1 || kc > kOdKc || n_parts < 1 || n_parts > 65535)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)od_blocks(pitch), (unsigned)n_parts);
    const long* lg = pm_lags(lags) + l0;
    pm_dispatch(f32, D, [&](auto e, auto d) {
        using E = decltype(e);
        hipLaunchKernelGGL((k_overlap_density<E, d()>), grid, dim3(kPmThreads), 0, st, (const E*)x, pitch, T, (int)n_atoms, lg, Lc, a2,
                           C, q, kc, partial);
    });
    return hipGetLastError();
}

hipError_t launch_overlap_density_sum(const double* partial, int n_parts, long T, int Lc, int C, int L, int kc, double* w,
                                      hipStream_t st) {
    const int n_slots = Lc * C, rows = kc * n_slots;
    if (n_parts < 1 || T < 1 || n_slots < 1 || n_slots > kOdSlots || kc < 1 || kc > kOdKc) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_overlap_density_sum, dim3((unsigned)((2 * T + 15) / 16), (unsigned)rows), dim3(256), 0, st, partial, n_parts,
                       T, n_slots, C, (long)L, (long)rows, w);
    return hipGetLastError();
}

}  // namespace ta
