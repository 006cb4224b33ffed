// msd.hip — the FFT form of the Einstein mean squared displacement (MDAnalysis.analysis.msd.EinsteinMSD, fft=True).
//
// With P[t] = x[t] - x[0] per column (MSD is invariant under the shift; unwrapped positions sit far from the origin, and
// the expansion below would otherwise cancel |x|^2 against |x|^2: SURVEY.md 7.3-5),
//   sum_{i<T-k} (P[i] - P[i+k])^2 = S1(k) - 2 S2(k),
//   S2(k) = sum_i P[i] P[i+k]                       -> the FFT VACF lag sums of the P slab (fft_impl)
//   S1(k) = sum_{i<T-k} P[i]^2 + sum_{i>=k} P[i]^2  -> prefix sums of Q[t] = sum_cols P[t]^2
// the identity of helfand_fft.hip, whose combine kernels finish the job with factor 1 (no mass, no division by D).
// One pass here reads the position slab and writes P into the context's scratch slab together with the norms:
// Qpart rows (lag sums) or the per-particle Ca array (by-particle form).
// Accuracy: each term is ~2 sum P^2 / (T-k) and their difference is formed in float64, so the absolute error is
// ~1e-16 of the largest squared displacement in the window; lags whose MSD is far below that (short lags of a long,
// drifting trajectory) lose relative accuracy by that ratio.
#include <hip/hip_runtime.h>

#include "ta_internal.hpp"

namespace ta {
namespace {

// Pair-major slabs in and out (layout.hip).  A workgroup walks whole column pairs along time (coalesced 16-byte rows):
// P[t, pair] = x[t] - x[0] for both columns (the unpaired last column's partner is written as 0), and the pair's
// P.x^2 + P.y^2, summed over the workgroup's pairs, go to its own row of Qpart ([gridDim.x][T], every element written).
__global__ void __launch_bounds__(256)
    k_msd_prepare(const double* __restrict__ pos, long pitch, long T, long n_cols, double* __restrict__ P,
                  double* __restrict__ Qpart) {
    const long n_pairs = (n_cols + 1) / 2;
    double* q = Qpart + (long)blockIdx.x * T;
    // time in pieces of 1024 rows, the workgroup's pairs inside: a thread's four contributions to Q stay in registers
    // across the pairs and are stored once per piece (as k_helfand_product)
    for (long t0 = 0; t0 < T; t0 += 1024) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (long pair = blockIdx.x; pair < n_pairs; pair += gridDim.x) {
            const bool two = 2 * pair + 1 < n_cols;
            const double2* x = reinterpret_cast<const double2*>(pos) + pair * pitch;
            double2* p = reinterpret_cast<double2*>(P) + pair * pitch;
            const double2 x0 = x[0];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long t = t0 + threadIdx.x + 256 * i;
                if (t < T) {
                    const double2 xx = x[t];
                    double2 r;
                    r.x = xx.x - x0.x;
                    r.y = two ? xx.y - x0.y : 0.0;
                    p[t] = r;
                    acc[i] += r.x * r.x + r.y * r.y;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long t = t0 + threadIdx.x + 256 * i;
            if (t < T) q[t] = acc[i];
        }
    }
}

// By-particle variant: P slab and Ca[t + 1, n] = sum_d P[t, n, d]^2 (rows 1..T of the (T+1, n_atoms) prefix array that
// k_helfand_combine_bp scans).  A workgroup takes a tile of 64 atoms x 64 frames.  Reads and P writes go with lanes
// along TIME (a wave covers 64 consecutive rows of one column: 1 KiB of its pair, whose other half the same workgroup
// touches for the neighbouring column), and a thread owns the cells (atom, t) of q for its lane and every fourth atom,
// so the sum over d needs no synchronisation and keeps the order d = 0, 1, 2; the tile's norms then leave with lanes
// along ATOMS: 512-byte rows of Ca.  (Lanes along atoms on the reads -- k_helfand_product_bp's form -- put a whole
// column pair between neighbouring lanes: 85 ms instead of ~10 for 24 GB.)
__global__ void __launch_bounds__(256)
    k_msd_prepare_bp(const double* __restrict__ pos, long pitch, long T, long n_atoms, int D, double* __restrict__ P,
                     double* __restrict__ Ca) {
    __shared__ double q[64][65];
    const long a0 = (long)blockIdx.x * 64, t0 = (long)blockIdx.y * 64;
    const int na = (int)min(64L, n_atoms - a0);
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long t = t0 + lane;
    for (int a = g; a < 64; a += 4) q[a][lane] = 0.0;
    for (int d = 0; d < D; ++d) {
        for (int a = g; a < na; a += 4) {
            const long c = (a0 + a) * D + d;
            const long base = (c >> 1) * pitch * 2 + (c & 1);
            const double x0 = pos[base];  // (one address for the whole wave)
            if (t < T) {
                const double val = pos[base + 2 * t] - x0;
                P[base + 2 * t] = val;
                q[a][lane] += val * val;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int a = i & 63, tt = i >> 6;
        if (a < na && t0 + tt < T) Ca[(t0 + tt + 1) * n_atoms + a0 + a] = q[a][tt];
    }
}

}  // namespace

hipError_t launch_msd_prepare(const double* pos, long pitch, long T, long n_cols, double* P, double* Qpart, int n_parts,
                              hipStream_t st) {
    hipLaunchKernelGGL(k_msd_prepare, dim3((unsigned)n_parts), dim3(256), 0, st, pos, pitch, T, n_cols, P, Qpart);
    return hipGetLastError();
}

hipError_t launch_msd_prepare_bp(const double* pos, long pitch, long T, long n_atoms, int D, double* P, double* Ca,
                                 hipStream_t st) {
    if (D < 1 || D > 3) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_msd_prepare_bp, dim3((unsigned)((n_atoms + 63) / 64), (unsigned)((T + 63) / 64)), dim3(256), 0, st,
                       pos, pitch, T, n_atoms, D, P, Ca);
    return hipGetLastError();
}

}  // namespace ta
