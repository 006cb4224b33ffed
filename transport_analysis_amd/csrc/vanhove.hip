// vanhove.hip — the self part of the van Hove function: for L lags tau_l the histogram of the squared displacements
// |x[t + tau, n] - x[t, n]|^2 over all pairs (t, n) with t + tau < T, against squared bin edges, and their first two moments
//
//   counts[l, b]  = #{(t, n): e[b] <= r2 < e[b + 1]}  (b = B: r2 >= e[B], the overflow bin)      uint64 (L, B + 1)
//   moments[l, :] = (sum r2, sum r2 r2)                                                          float64 (L, 2)
//
// with the arithmetic of vanhove_math.hpp (the CPU backend follows it: equal counts for any input).  The slab is read as it
// is, a float32 one as float32.  A histogram is no correlation: there is no FFT form and nothing else in the library
// computes it; k_vanhove is one pass over the slab per chunk of Lc lags.
//
// Determinism.  The counts are integers: LDS and global integer adds give the same bits in any order.  The moments use
// no floating-point atomics: a thread adds its frames in order, a wave reduces by a fixed butterfly, each wave adds into
// its own LDS slot in atom-loop order, the workgroup adds its waves' slots in wave order into ONE partial per (workgroup,
// lag), and k_sum_partials adds the partials in its fixed order.  None of this depends on Lc: the same bits for every chunk size.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pm_read.hpp"
#include "ta_internal.hpp"
#include "vanhove_math.hpp"

namespace ta {
namespace {

constexpr int kVhWaves = kPmThreads / 64;
// A workgroup adds at most kPmThreads kPmFrames = 1024 to a bin per (atom, lag): its uint32 bins are flushed into the
// uint64 histogram at the latest every 2^21 atoms of its loop (2^31 per bin)
constexpr int kVhFlushAtoms = 1 << 21;
constexpr size_t kVhLdsBudget = 64 << 10;  // a choice (two workgroups on a CU's 160 KB), not a measurement

// LDS of a workgroup: e[B + 1] doubles, the waves' moment slots [wave][Lc][2] doubles, the histogram [Lc][B + 1] uint32
constexpr size_t vh_lds_bytes(int B, int Lc) {
    return sizeof(double) * (size_t)(B + 1) + (size_t)Lc * (sizeof(double) * 2 * kVhWaves + sizeof(unsigned) * (size_t)(B + 1));
}

// LDS bins (uint32) of the chunk's lags into the uint64 histogram, and cleared (callers: between two barriers)
__device__ __forceinline__ void vh_flush(unsigned* hist, int n, unsigned long long* __restrict__ counts) {
    for (int i = threadIdx.x; i < n; i += kPmThreads) {
        const unsigned v = hist[i];
        if (v) {
            atomicAdd(&counts[i], (unsigned long long)v);
            hist[i] = 0;
        }
    }
}

// A work unit (pm_read.hpp) is one atom.  Workgroup (bx, g): origin frames [1024 bx, 1024 bx + 1024), atoms g, g + G, ...
// (G = gridDim.y).  The atom's columns at the thread's kPmFrames origin frames stay in registers across the chunk's lags;
// per lag the row t + tau of the same pairs is read by pm_lagged (pm_read.hpp): a pair with t + tau >= T reads row 0 and
// contributes nothing.
// lags, counts, partial: the chunk's (lags + l0, counts + l0 (B + 1), partial + 2 l0; a workgroup's partials are 2 L apart).
template <class E, int D>
__global__ void __launch_bounds__(kPmThreads)
    k_vanhove(const E* __restrict__ x, long pitch, long T, int n_atoms, const long* __restrict__ lags, int Lc,
              const double* __restrict__ e_g, int B, float inv_dr, unsigned long long* __restrict__ counts,
              double* __restrict__ partial, int L, int flush_atoms) {
    constexpr int F = kPmFrames;
    extern __shared__ __attribute__((aligned(16))) unsigned char vh_lds[];
    const int nb = B + 1;
    double* e = reinterpret_cast<double*>(vh_lds);
    double* mom = e + nb;
    unsigned* hist = reinterpret_cast<unsigned*>(mom + 2 * kVhWaves * Lc);
    for (int i = threadIdx.x; i < nb; i += kPmThreads) e[i] = e_g[i];
    for (int i = threadIdx.x; i < 2 * kVhWaves * Lc; i += kPmThreads) mom[i] = 0.0;
    for (int i = threadIdx.x; i < Lc * nb; i += kPmThreads) hist[i] = 0;
    __syncthreads();

    const long tb = (long)blockIdx.x * (kPmThreads * F);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int since = 0;
    for (int n = blockIdx.y; n < n_atoms; n += gridDim.y) {
        const PmAtom<E, D> a(x, pitch, (unsigned)n);  // (atom D < 2^31: launch_vanhove)
        double col[F][3];
        pm_load(a, T, tb, col);
        for (int l = 0; l < Lc; ++l) {
            const long tau = lags[l];
            unsigned* h = hist + l * nb;
            double s2 = 0.0, s4 = 0.0;
            pm_lagged(a, T, tb, tau, [&](int f, bool live, const double(&x1)[3]) {
                const double r2 = vh_r2<D>(col[f], x1);
                if (live) {
                    s2 += r2;
                    s4 = fma(r2, r2, s4);
                    atomicAdd(&h[vh_bin(r2, e, B, inv_dr)], 1u);
                }
            });
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {  // the same pattern whatever the values: every lane ends with the wave's sum
                s2 += __shfl_xor(s2, m);
                s4 += __shfl_xor(s4, m);
            }
            if (lane == 0) {
                double* slot = mom + 2 * (wave * Lc + l);
                slot[0] += s2;
                slot[1] += s4;
            }
        }
        if (++since == flush_atoms) {
            __syncthreads();
            vh_flush(hist, Lc * nb, counts);
            __syncthreads();
            since = 0;
        }
    }
    __syncthreads();
    vh_flush(hist, Lc * nb, counts);
    double* out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(2 * L);
    for (int i = threadIdx.x; i < 2 * Lc; i += kPmThreads) {
        double s = mom[i];
#pragma unroll
        for (int w = 1; w < kVhWaves; ++w) s += mom[2 * w * Lc + i];
        out[i] = s;
    }
}

}  // namespace

int vanhove_max_chunk(int B) {
    return (int)std::max<size_t>(1, (kVhLdsBudget - sizeof(double) * (size_t)(B + 1)) /
                                        (sizeof(double) * 2 * kVhWaves + sizeof(unsigned) * (size_t)(B + 1)));
}

int vanhove_parts(int n_cu, long pitch, long n_atoms) {
    const dim3 grid = pm_unit_grid(n_cu, pitch, n_atoms);
    return (int)(grid.x * grid.y);
}

hipError_t launch_vanhove(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, const int64_t* lags, int l0,
                          int Lc, int L, const double* e, int B, float inv_dr, unsigned long long* counts, double* partial,
                          hipStream_t st) {
    if (!pm_slab_ok(pitch, T, n_atoms, D) || B < 1 || Lc < 1 || l0 < 0 || l0 + Lc > L || Lc > vanhove_max_chunk(B))
        return hipErrorInvalidValue;
    const dim3 grid = pm_unit_grid(n_cu, pitch, n_atoms);
    const size_t lds = vh_lds_bytes(B, Lc);
    const long* lg = pm_lags(lags) + l0;
    unsigned long long* cnt = counts + (size_t)l0 * (size_t)(B + 1);
    double* part = partial + 2 * (size_t)l0;
    return pm_dispatch(f32, D, [&](auto el, auto d) {
        using E = decltype(el);
        const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_vanhove<E, d()>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess) return err;
        hipLaunchKernelGGL((k_vanhove<E, d()>), grid, dim3(kPmThreads), lds, st, (const E*)x, pitch, T, (int)n_atoms, lg, Lc, e, B,
                           inv_dr, cnt, part, L, kVhFlushAtoms);
        return hipGetLastError();
    });
}

}  // namespace ta
