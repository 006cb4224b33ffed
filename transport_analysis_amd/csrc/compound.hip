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

#include <algorithm>
#include <type_traits>

#include "ta_internal.hpp"

namespace ta {
namespace {

constexpr int kCmpThreads = 256, kCmpFrames = 4;  // k_species_sort's geometry: a workgroup covers 1024 consecutive frames

// k_species_sort's selects (species_self.hip: sort_pick): column c + j of an atom (odd = c & 1) is element j + odd of the
// source pairs (ax, ay), (bx, by) that cover it; selects on loaded VALUES with constant destinations, nothing in scratch
template <int D, class V>
__device__ __forceinline__ void cmp_pick(V ax, V ay, V bx, V by, bool odd, double (&out)[3]) {
    if constexpr (D == 2) {
        out[0] = (double)ax, out[1] = (double)ay;
    } else {
        out[0] = (double)(odd ? ay : ax);
        if constexpr (D == 3) out[1] = (double)(odd ? bx : ay), out[2] = (double)(odd ? by : bx);
    }
}

// The D columns of one atom in the thread's four frames: the whole source pairs that cover them (one for D = 1, 2, two for
// D = 3), 16-byte loads along time.
//   float64 slab: a load = row t of a pair; the thread's frames are tb + tid + 256 i, i < 4
//   float32 slab: a load = rows 2 q, 2 q + 1 of a pair (8-byte rows), widened in registers; q = tb / 2 + tid + 256 i, i < 2
// A load that would start at or past row T reads row 0 instead (its result is never stored).
template <class E, int D>
__device__ __forceinline__ void cmp_load(const E* __restrict__ x, long pitch, long T, long tb, unsigned atom,
                                         double (&col)[kCmpFrames][3]) {
    constexpr bool kF32 = std::is_same_v<E, float>;
    constexpr int NP = D == 3 ? 2 : 1;
    const unsigned c = atom * (unsigned)D;  // (n_atoms dim < 2^31: launch_compound)
    const bool odd = c & 1;
    if constexpr (!kF32) {
        const double2* src = reinterpret_cast<const double2*>(x) + (long)(c >> 1) * pitch;
#pragma unroll
        for (int f = 0; f < kCmpFrames; ++f) {
            const long t = tb + threadIdx.x + kCmpThreads * f, i = t < T ? t : 0;
            const double2 qa = src[i], qb = NP == 2 ? src[pitch + i] : qa;
            cmp_pick<D>(qa.x, qa.y, qb.x, qb.y, odd, col[f]);
        }
    } else {
        const long hp = pitch / 2;
        const float4* src = reinterpret_cast<const float4*>(x) + (long)(c >> 1) * hp;
#pragma unroll
        for (int f = 0; f < kCmpFrames; f += 2) {
            const long t = 2 * (tb / 2 + threadIdx.x + kCmpThreads * (f / 2)), i = t < T ? t / 2 : 0;
            const float4 qa = src[i], qb = NP == 2 ? src[hp + i] : qa;
            cmp_pick<D>(qa.x, qa.y, qb.x, qb.y, odd, col[f]);
            cmp_pick<D>(qa.z, qa.w, qb.z, qb.w, odd, col[f + 1]);
        }
    }
}

// A work unit is two consecutive compounds (2 u, 2 u + 1): 2 D columns = D WHOLE destination pairs, so every store is a full
// 16-byte row and a wave's stores of one pair are contiguous along time.  The last unit of an odd compound count holds one
// compound: ceil(D / 2) pairs, the phantom column (odd D) written as 0.  Workgroup (bx, g): frames [1024 bx, 1024 bx + 1024)
// of the pitch, units g, g + G, ... (G = gridDim.y).  A unit's member range, its members and their weights depend on
// blockIdx and loop counters only: plain indexed reads, scalar registers, read-only.  The member loop is unrolled by two:
// both members' loads (up to 16 of 16 bytes per thread) are in flight before the first is used; the terms are still added
// in member order.
template <class E, int D>
__global__ void __launch_bounds__(kCmpThreads)
    k_compound(const E* __restrict__ x, long pitch, long T, int n_compounds, const int* __restrict__ off,
               const int* __restrict__ member, const double* __restrict__ w, const double* __restrict__ g,
               const double* __restrict__ F, double* __restrict__ out) {
    constexpr bool kF32 = std::is_same_v<E, float>;
    constexpr int NF = kCmpFrames;
    const long tb = (long)blockIdx.x * (kCmpThreads * NF);
    auto frame = [&](int f) -> long {
        if constexpr (kF32) return 2 * (tb / 2 + threadIdx.x + kCmpThreads * (f / 2)) + f % 2;
        else return tb + threadIdx.x + kCmpThreads * f;
    };
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
                cmp_load<E, D>(x, pitch, T, tb, (unsigned)member[lo], ca);
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int j = 0; j < D; ++j) acc[f][j] = w0 * ca[f][j];
            }
            int m = lo + 1;
            for (; m + 1 < hi; m += 2) {
                const double wa = w ? w[m] : 1.0, wb = w ? w[m + 1] : 1.0;
                cmp_load<E, D>(x, pitch, T, tb, (unsigned)member[m], ca);
                cmp_load<E, D>(x, pitch, T, tb, (unsigned)member[m + 1], cb);
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int j = 0; j < D; ++j) acc[f][j] = fma(wb, cb[f][j], fma(wa, ca[f][j], acc[f][j]));
            }
            if (m < hi) {
                const double wa = w ? w[m] : 1.0;
                cmp_load<E, D>(x, pitch, T, tb, (unsigned)member[m], ca);
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int j = 0; j < D; ++j) acc[f][j] = fma(wa, ca[f][j], acc[f][j]);
            }
            if (F) {  // the barycentric term: F[t] once per frame
                const double gc = -g[cmp];
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    const long t = frame(f), i = t < T ? t : 0;
#pragma unroll
                    for (int j = 0; j < D; ++j) acc[f][j] = fma(gc, F[i * D + j], acc[f][j]);
                }
            }
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int j = 0; j < D; ++j) val[f][a * D + j] = acc[f][j];
        }
        const int n_out = two ? D : (D + 1) / 2;  // whole pairs of this unit
        double2* dst = reinterpret_cast<double2*>(out) + (long)D * unit * pitch;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const long t = frame(f);
            if (t >= pitch) continue;
            const bool live = t < T;
#pragma unroll
            for (int j = 0; j < D; ++j)
                if (j < n_out) dst[j * pitch + t] = live ? double2{val[f][2 * j], val[f][2 * j + 1]} : double2{0.0, 0.0};
        }
    }
}

template <class E, int D>
void cmp_launch(dim3 grid, hipStream_t st, const void* x, long pitch, long T, int C, const int* off, const int* member,
                const double* w, const double* g, const double* F, double* out) {
    hipLaunchKernelGGL((k_compound<E, D>), grid, dim3(kCmpThreads), 0, st, (const E*)x, pitch, T, C, off, member, w, g, F, out);
}
template <class E>
void cmp_launch_dim(int D, dim3 grid, hipStream_t st, const void* x, long pitch, long T, int C, const int* off,
                    const int* member, const double* w, const double* g, const double* F, double* out) {
    if (D == 1) cmp_launch<E, 1>(grid, st, x, pitch, T, C, off, member, w, g, F, out);
    else if (D == 2) cmp_launch<E, 2>(grid, st, x, pitch, T, C, off, member, w, g, F, out);
    else cmp_launch<E, 3>(grid, st, x, pitch, T, C, off, member, w, g, F, out);
}

}  // namespace

hipError_t launch_compound(int n_cu, const void* x, bool f32, long pitch, long T, long n_cols, int D, long n_compounds,
                           const int* off, const int* member, const double* w, const double* g, const double* F, double* out,
                           hipStream_t st) {
    if (D < 1 || D > 3 || n_cols < 1 || n_cols >= (1L << 31) || (pitch & 7) || T < 1 || T > pitch || n_compounds < 1 ||
        n_compounds * D >= (1L << 31) || (F && !g))
        return hipErrorInvalidValue;
    // about sixteen workgroups per CU over the frame blocks, at most one group per unit
    const long n_tb = (pitch + kCmpThreads * kCmpFrames - 1) / (kCmpThreads * kCmpFrames);
    const long n_units = (n_compounds + 1) / 2;
    const long want = (16L * n_cu + n_tb - 1) / n_tb;
    const dim3 grid((unsigned)n_tb, (unsigned)std::max(1L, std::min({want, n_units, 65535L})));
    if (f32) cmp_launch_dim<float>(D, grid, st, x, pitch, T, (int)n_compounds, off, member, w, g, F, out);
    else cmp_launch_dim<double>(D, grid, st, x, pitch, T, (int)n_compounds, off, member, w, g, F, out);
    return hipGetLastError();
}

}  // namespace ta
