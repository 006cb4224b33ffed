// scatter.hip — the phase slab of the intermediate scattering functions F_s(k, t) and F(k, t).
//
//   Z[t, 2 (jl A + n) + {0, 1}] = (cos, sin)(k_jl . x[t, n, :])
//
// for the Kc wavevectors of one chunk: per wavevector a block of A pairs, one pair per atom -- exp(i k.x_n(t)) as a 16-byte
// row.  Every block is a pair-major slab of A "atoms" with D = 2 of its own (it starts on a pair boundary, there is no
// phantom column): the self part is its VACF lag sum, the density its sum over atoms (k_species_sum without the shift),
// both by the evaluations of api.hip unchanged.  Rows T ... pitch - 1 of every pair are written as zeros (the scratch is
// reused between calls), rows >= pitch are not written.  No atomics, every destination element has one writer: the same
// bits from run to run, and the same bits for every chunk size.
//
// The phase arithmetic (the CPU backend follows it): the host passes q = k / (2 pi), turns per length unit, as float64;
//   u = fma(q[2], x[2], fma(q[1], x[1], q[0] x[0]))   (as many terms as D),   r = u - rint(u)   (|r| <= 1/2, exact),
//   (cos, sin)(2 pi r) by sincospi(2 r).
// The reduced argument keeps sincospi on its fast path: no large-argument reduction, no table in private memory.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pm_read.hpp"
#include "ta_internal.hpp"

namespace ta {
namespace {

// A work unit (pm_read.hpp) is one atom, read as the whole source pairs that cover its D columns (a float32 slab as
// float32, widened in registers); the half that belongs to a neighbouring atom is that atom's unit's own load (cache).
// Workgroup (bx, g): frames [1024 bx, 1024 bx + 1024) of the pitch, atoms g, g + G, ... (G = gridDim.y).  The atom's
// columns stay in registers across the chunk's wavevectors; q[jl D + d] has a uniform address: scalar loads, scalar
// registers.  Each store is a full 16-byte row, contiguous along time across a wave; the float32 reader's two rows
// (2 m, 2 m + 1) go out side by side.
template <class E, int D>
__global__ void __launch_bounds__(kPmThreads)
    k_phase(const E* __restrict__ x, long pitch, long T, int n_atoms, const double* __restrict__ q, int Kc,
            double* __restrict__ Z) {
    constexpr bool kF32 = std::is_same_v<E, float>;
    constexpr int F = kPmFrames;
    const long tb = (long)blockIdx.x * (kPmThreads * F);
    for (int n = blockIdx.y; n < n_atoms; n += gridDim.y) {
        double col[F][3];
        pm_load(PmAtom<E, D>(x, pitch, (unsigned)n), T, tb, col);  // (atom D < 2^31: launch_phase)
        for (int jl = 0; jl < Kc; ++jl) {
            const double q0 = q[jl * D], q1 = D > 1 ? q[jl * D + 1] : 0.0, q2 = D > 2 ? q[jl * D + 2] : 0.0;
            double2* dst = reinterpret_cast<double2*>(Z) + ((long)jl * n_atoms + n) * pitch;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const long t = pm_frame<kF32>(tb, f);
                if (t >= pitch) continue;
                double u = q0 * col[f][0];
                if constexpr (D > 1) u = fma(q1, col[f][1], u);
                if constexpr (D > 2) u = fma(q2, col[f][2], u);
                const double r = u - rint(u);
                double s, c;
                sincospi(2.0 * r, &s, &c);
                dst[t] = t < T ? double2{c, s} : double2{0.0, 0.0};
            }
        }
    }
}

// (T, K) by-particle lag sums of the K densities -> (K, T)
__global__ void k_scatter_transpose(const double* __restrict__ bp, long T, long K, double* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * K) return;
    const long j = i / T, t = i - j * T;
    out[i] = bp[t * K + j];
}

template <class E, int D>
void phase_launch(dim3 grid, hipStream_t st, const void* x, long pitch, long T, int A, const double* q, int Kc, double* Z) {
    hipLaunchKernelGGL((k_phase<E, D>), grid, dim3(kPmThreads), 0, st, (const E*)x, pitch, T, A, q, Kc, Z);
}
template <class E>
void phase_launch_dim(int D, dim3 grid, hipStream_t st, const void* x, long pitch, long T, int A, const double* q, int Kc,
                      double* Z) {
    if (D == 1) phase_launch<E, 1>(grid, st, x, pitch, T, A, q, Kc, Z);
    else if (D == 2) phase_launch<E, 2>(grid, st, x, pitch, T, A, q, Kc, Z);
    else phase_launch<E, 3>(grid, st, x, pitch, T, A, q, Kc, Z);
}

}  // namespace

hipError_t launch_phase(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, const double* q, int Kc,
                        double* Z, hipStream_t st) {
    if (D < 1 || D > 3 || n_atoms < 1 || n_atoms * D >= (1L << 31) || (pitch & 7) || T < 1 || T > pitch || Kc < 1)
        return hipErrorInvalidValue;
    const dim3 grid = pm_unit_grid(n_cu, pitch, n_atoms);
    if (f32) phase_launch_dim<float>(D, grid, st, x, pitch, T, (int)n_atoms, q, Kc, Z);
    else phase_launch_dim<double>(D, grid, st, x, pitch, T, (int)n_atoms, q, Kc, Z);
    return hipGetLastError();
}

hipError_t launch_scatter_transpose(const double* bp, long T, long K, double* out, hipStream_t st) {
    const long n = T * K;
    hipLaunchKernelGGL(k_scatter_transpose, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bp, T, K, out);
    return hipGetLastError();
}

}  // namespace ta
