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
// The phase arithmetic is phase_math.hpp's (q = k / (2 pi) from the host).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "phase_math.hpp"
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
                const double2 cs = phase_cs<D>(q0, q1, q2, col[f]);
                dst[t] = t < T ? cs : double2{0.0, 0.0};
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

}  // namespace

hipError_t launch_phase(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, const double* q, int Kc,
                        double* Z, hipStream_t st) {
    if (!pm_slab_ok(pitch, T, n_atoms, D) || Kc < 1) return hipErrorInvalidValue;
    const dim3 grid = pm_unit_grid(n_cu, pitch, n_atoms);
    pm_dispatch(f32, D, [&](auto e, auto d) {
        using E = decltype(e);
        hipLaunchKernelGGL((k_phase<E, d()>), grid, dim3(kPmThreads), 0, st, (const E*)x, pitch, T, (int)n_atoms, q, Kc, Z);
    });
    return hipGetLastError();
}

hipError_t launch_scatter_transpose(const double* bp, long T, long K, double* out, hipStream_t st) {
    const long n = T * K;
    hipLaunchKernelGGL(k_scatter_transpose, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bp, T, K, out);
    return hipGetLastError();
}

}  // namespace ta
