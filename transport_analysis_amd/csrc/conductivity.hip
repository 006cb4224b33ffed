// conductivity.hip — the charge-weighted moment of a staged position slab (Einstein-Helfand ionic conductivity).
//
//   M[t, d] = sum_n q_n (x[t, n, d] - x[0, n, d])          (translational dipole displacement, (n_frames, dim))
//
// The collective MSD of M and the Nernst-Einstein self term are evaluated afterwards by the Einstein MSD paths
// (api.hip: cond_pm); this file only makes the one pass over the slab.  The first-frame shift matters: unwrapped
// coordinates sit far from the origin, and sum q x of a near-neutral system would cancel large terms against each
// other.  Reads go as in k_msd_prepare (whole column pairs along time, 16-byte rows); the moment leaves as partial
// sums per group of pairs, added afterwards in a fixed order by k_sum_partials: no atomics, so the moment is the same
// bits from run to run.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ta_internal.hpp"

namespace ta {
namespace {

constexpr int kCondThreads = 256, kCondRows = 4;  // a workgroup covers 1024 consecutive frames

// Workgroup (bx, g): frames [1024 bx, 1024 bx + 1024), column pairs g, g + G, g + 2 G, ... (G = gridDim.y).  A thread
// owns four frames (t = t0 + threadIdx.x + 256 i) and keeps their D sums in registers across the pairs, so a pair's
// two columns are added to dims (2 p) % D and (2 p + 1) % D by selects rather than a runtime register index; the
// unpaired last column's partner counts as charge 0.  partial[g][t][d] is written in full for t < T.  With W, the
// weighted shifted slab W[t, c] = q (x[t, c] - x[0, c]) is written in the same layout (the partner of an unpaired
// column as 0): the self term's input, so the position slab is read once.
__global__ void __launch_bounds__(kCondThreads)
    k_cond_moment(const double* __restrict__ pos, long pitch, long T, long n_cols, int D,
                  const double* __restrict__ q, double* __restrict__ partial, double* __restrict__ W) {
    const long n_pairs = (n_cols + 1) / 2;
    const long g = blockIdx.y, G = gridDim.y;
    const long t0 = (long)blockIdx.x * (kCondThreads * kCondRows) + threadIdx.x;
    double acc[kCondRows][3] = {};
    for (long pair = g; pair < n_pairs; pair += G) {
        const long c0 = 2 * pair, c1 = c0 + 1;
        const bool two = c1 < n_cols;
        const double q0 = q[c0 / D], q1 = two ? q[c1 / D] : 0.0;
        const int d0 = (int)(c0 % D), d1 = (int)(c1 % D);
        const double2* x = reinterpret_cast<const double2*>(pos) + pair * pitch;
        const double2 x0 = x[0];  // (one address for the whole workgroup)
        double2 r[kCondRows];
#pragma unroll
        for (int i = 0; i < kCondRows; ++i) {
            const long t = t0 + kCondThreads * i;
            r[i] = t < T ? x[t] : x0;
        }
#pragma unroll
        for (int i = 0; i < kCondRows; ++i) {
            const double a = q0 * (r[i].x - x0.x), b = q1 * (r[i].y - x0.y);
#pragma unroll
            for (int d = 0; d < 3; ++d) acc[i][d] += (d == d0 ? a : 0.0) + (d == d1 ? b : 0.0);
            const long t = t0 + kCondThreads * i;
            if (W && t < T) reinterpret_cast<double2*>(W)[pair * pitch + t] = double2{a, b};
        }
    }
    double* out = partial + g * T * D;
#pragma unroll
    for (int i = 0; i < kCondRows; ++i) {
        const long t = t0 + kCondThreads * i;
        if (t < T)
            for (int d = 0; d < D; ++d) out[t * D + d] = acc[i][d];
    }
}

}  // namespace

int cond_moment_parts(int n_cu, long T, long n_cols) {
    // about eight workgroups per CU over the frame blocks, at most one group per pair and 1024 groups
    const long n_tb = (T + kCondThreads * kCondRows - 1) / (kCondThreads * kCondRows);
    const long n_pairs = (n_cols + 1) / 2;
    const long want = (8L * n_cu + n_tb - 1) / n_tb;
    return (int)std::max(1L, std::min({want, n_pairs, 1024L}));
}

hipError_t launch_cond_moment(const double* pos, long pitch, long T, long n_cols, int D, const double* q, double* partial,
                              int n_parts, double* W, hipStream_t st) {
    if (D < 1 || D > 3 || n_parts < 1 || n_parts > 65535) return hipErrorInvalidValue;
    const long n_tb = (T + kCondThreads * kCondRows - 1) / (kCondThreads * kCondRows);
    hipLaunchKernelGGL(k_cond_moment, dim3((unsigned)n_tb, (unsigned)n_parts), dim3(kCondThreads), 0, st, pos, pitch, T,
                       n_cols, D, q, partial, W);
    return hipGetLastError();
}

}  // namespace ta
