// compound.hip — a staged slab of atoms reduced to a slab of compounds (molecules, ions): weighted centres, optionally in the
// frame of a weighted mean over all atoms (the barycentric frame).
//
//   out[t, D c + d] = sum_{i in [off[c], off[c + 1])} w_i x[t, D member[i] + d]  -  g_c F[t, d],      g_c = sum_i w_i
//
// The sum of a compound runs in member order in float64: the first product as it is, every further term one fma; with F the
// result is fma(-g_c, F, sum).  No atomics, every destination element has one writer: the same bits from run to run, and a
// one-member compound of weight 1 without F is its atom's column bit for bit.  Every row < pitch of every destination pair
// is written (rows >= T and the phantom column of an odd n_compounds * D as zeros): the destination is a fresh allocation.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pm_read.hpp"
#include "ta_internal.hpp"

namespace ta {
namespace {

// A work unit (pm_read.hpp) is two consecutive compounds (2 u, 2 u + 1); the last unit of an odd compound count holds one.
// Every member atom is read as the whole source pairs that cover its D columns.  Workgroup (bx, g): frames [1024 bx,
// 1024 bx + 1024) of the pitch, units g, g + G, ... (G = gridDim.y).  A unit's member range, its members and their weights
// depend on blockIdx and loop counters only: plain indexed reads, scalar registers, read-only.  The member loop is
// unrolled by two: both members' loads (up to 16 of 16 bytes per thread) are in flight before the first is used; the
// terms are still added in member order.
template <class E, int D>
__global__ void __launch_bounds__(kPmThreads)
    k_compound(const E* __restrict__ x, long pitch, long T, int n_compounds, const int* __restrict__ off,
               const int* __restrict__ member, const double* __restrict__ w, const double* __restrict__ g,
               const double* __restrict__ F, double* __restrict__ out) {
    constexpr bool kF32 = std::is_same_v<E, float>;
    constexpr int NF = kPmFrames;
    const long tb = (long)blockIdx.x * (kPmThreads * NF);
    // (atom D < 2^31: launch_compound)
    auto load = [&](int m, double (&col)[NF][3]) { pm_load(PmAtom<E, D>(x, pitch, (unsigned)member[m]), T, tb, col); };
    const int n_units = (n_compounds + 1) / 2;
    for (int unit = blockIdx.y; unit < n_units; unit += gridDim.y) {
        const bool two = 2 * unit + 1 < n_compounds;
        double val[NF][2 * D];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            if (a == 1 && !two) {
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int j = 0; j < D; ++j) val[f][D + j] = 0.0;
                continue;
            }
            const int cmp = 2 * unit + a;
            const int lo = off[cmp], hi = off[cmp + 1];  // (hi > lo: no empty compound)
            double acc[NF][3], ca[NF][3], cb[NF][3];
            {
                const double w0 = w ? w[lo] : 1.0;
                load(lo, ca);
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int j = 0; j < D; ++j) acc[f][j] = w0 * ca[f][j];
            }
            int m = lo + 1;
            for (; m + 1 < hi; m += 2) {
                const double wa = w ? w[m] : 1.0, wb = w ? w[m + 1] : 1.0;
                load(m, ca);
                load(m + 1, cb);
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int j = 0; j < D; ++j) acc[f][j] = fma(wb, cb[f][j], fma(wa, ca[f][j], acc[f][j]));
            }
            if (m < hi) {
                const double wa = w ? w[m] : 1.0;
                load(m, ca);
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int j = 0; j < D; ++j) acc[f][j] = fma(wa, ca[f][j], acc[f][j]);
            }
            if (F) {  // the barycentric term: F[t] once per frame
                const double gc = -g[cmp];
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    const long t = pm_frame<kF32>(tb, f), i = t < T ? t : 0;
#pragma unroll
                    for (int j = 0; j < D; ++j) acc[f][j] = fma(gc, F[i * D + j], acc[f][j]);
                }
            }
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int j = 0; j < D; ++j) val[f][a * D + j] = acc[f][j];
        }
        const int n_out = two ? D : (D + 1) / 2;
        double2* dst = reinterpret_cast<double2*>(out) + (long)D * unit * pitch;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const long t = pm_frame<kF32>(tb, f);
            if (t >= pitch) continue;
            pm_store_row<D>(dst, pitch, t, t < T, n_out, val[f]);
        }
    }
}

}  // namespace

hipError_t launch_compound(int n_cu, const void* x, bool f32, long pitch, long T, long n_cols, int D, long n_compounds,
                           const int* off, const int* member, const double* w, const double* g, const double* F, double* out,
                           hipStream_t st) {
    if (D < 1 || D > 3 || n_cols < 1 || n_cols >= (1L << 31) || (pitch & 7) || T < 1 || T > pitch || n_compounds < 1 ||
        n_compounds * D >= (1L << 31) || (F && !g))
        return hipErrorInvalidValue;
    const dim3 grid = pm_unit_grid(n_cu, pitch, (n_compounds + 1) / 2);
    pm_dispatch(f32, D, [&](auto e, auto d) {
        using E = decltype(e);
        hipLaunchKernelGGL((k_compound<E, d()>), grid, dim3(kPmThreads), 0, st, (const E*)x, pitch, T, (int)n_compounds, off, member,
                           w, g, F, out);
    });
    return hipGetLastError();
}

}  // namespace ta
