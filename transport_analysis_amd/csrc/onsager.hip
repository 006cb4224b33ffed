// onsager.hip — species-resolved moments of a staged position slab and the small kernels around their cross MSD
// (Onsager transport coefficients, OnsagerHelfand).
//
//   M[s, t, d] = sum_{n: species[n] = s} w_n (x[t, n, d] - x[0, n, d])          ((n_species, n_frames, dim))
//
// k_species_moment is k_cond_moment (conductivity.hip) with the sum split by a per-atom label: the slab is read ONCE, in
// 16-byte rows along time, whatever the number of species; the first-frame shift comes before the weight; the moments
// leave as partial sums per group of column pairs, added afterwards in a fixed order by k_sum_partials (no atomics: the
// same bits from run to run).  The cross MSD C[k, i, j] of the moments is evaluated by the Einstein MSD paths on S^2
// pseudo-particles (api.hip: ons_cross); k_onsager_combos and k_onsager_finish are its two ends.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "species_acc.hpp"
#include "ta_internal.hpp"

namespace ta {
namespace {

// Workgroup (bx, g): frames [256 ROWS bx, 256 ROWS (bx + 1)), column pairs g, g + G, g + 2 G, ... (G = gridDim.y), U of
// them per trip so that every thread has ROWS U 16-byte rows in flight.  A thread owns ROWS frames (t = t0 + 256 i) and
// keeps their SMAX x 3 sums in registers across the pairs.  Everything that picks an accumulator -- the species of the
// pair's two columns (two atoms for a straddling pair, possibly of different species) and their dims -- depends on
// blockIdx and the loop counter only: it is read through readfirstlane, so OnsAcc's index is a scalar.
// A label outside [0, S) is skipped (the host-facing calls reject it before it gets here); the unpaired last column's
// partner is skipped too.  partial[g][s][t][d] is written in full for s < S, t < T: a species without atoms gives zeros.
template <int SMAX, int ROWS, int U>
__global__ void __launch_bounds__(kOnsThreads)
    k_species_moment(const double* __restrict__ pos, long pitch, long T, long n_cols, int D, int S,
                     const int* __restrict__ species, const double* __restrict__ w, double* __restrict__ partial) {
    const long n_pairs = (n_cols + 1) / 2;
    const long g = blockIdx.y, G = gridDim.y;
    const long t0 = (long)blockIdx.x * (kOnsThreads * ROWS) + threadIdx.x;
    OnsAcc<SMAX> acc[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) acc[i].clear();
    for (long pair = g; pair < n_pairs; pair += G * U) {
        double rx[U][ROWS], ry[U][ROWS];  // x[t] - x[0] of the trip's pairs: all loads are issued before any is used
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // (a pair index past the end reads the trip's first pair again and adds nothing below)
            const long p = pair + (long)u * G < n_pairs ? pair + (long)u * G : pair;
            const double2* x = reinterpret_cast<const double2*>(pos) + p * pitch;
            const double2 x0 = x[0];  // (one address for the whole workgroup)
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                const long t = t0 + kOnsThreads * i;
                const double2 xt = x[t < T ? t : 0];  // (a frame past the end: x[0], a zero displacement)
                rx[u][i] = xt.x - x0.x, ry[u][i] = xt.y - x0.y;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long p = pair + (long)u * G;
            const long c0 = 2 * p, c1 = c0 + 1;
            int s0 = -1, s1 = -1, d0 = 0, d1 = 0;
            double w0 = 0.0, w1 = 0.0;
            if (c0 < n_cols) {
                const unsigned a0 = ons_atom((unsigned)c0, D);  // (n_cols < 2^31: launch_species_moment)
                s0 = species[a0];
                d0 = (int)((unsigned)c0 - a0 * (unsigned)D);
                w0 = w ? w[a0] : 1.0;
            }
            if (c1 < n_cols) {
                const unsigned a1 = ons_atom((unsigned)c1, D);
                s1 = species[a1];
                d1 = (int)((unsigned)c1 - a1 * (unsigned)D);
                w1 = w ? w[a1] : 1.0;
            }
            const int k0 = (unsigned)s0 < (unsigned)S ? __builtin_amdgcn_readfirstlane(s0) : -1;
            const int k1 = (unsigned)s1 < (unsigned)S ? __builtin_amdgcn_readfirstlane(s1) : -1;
            d0 = __builtin_amdgcn_readfirstlane(d0), d1 = __builtin_amdgcn_readfirstlane(d1);
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                acc[i].add(k0, d0, w0 * rx[u][i]);
                acc[i].add(k1, d1, w1 * ry[u][i]);
            }
        }
    }
    double* out = partial + g * (long)S * T * D;
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        const long t = t0 + kOnsThreads * i;
        if (t < T) {
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (s < S) {  // (constant indices)
                    double* o = out + ((long)s * T + t) * D;
                    o[0] = acc[i].get(3 * s);
                    if (D > 1) o[1] = acc[i].get(3 * s + 1);
                    if (D > 2) o[2] = acc[i].get(3 * s + 2);
                }
        }
    }
}

// The species classes (species_acc.hpp: kOnsClasses) use 90 - 96 VGPRs, 64 of them accumulators: five waves per SIMD; no
// scratch, no spills.

// Pair-major slab of the S^2 pseudo-particles whose MSDs give C by polarisation: particle i S + j is M_i (i == j),
// M_i + M_j (i < j), M_i - M_j (i > j).  One thread per (row, column pair); rows T ... pitch - 1 and the partner of an
// unpaired last column are written as 0.  nz[s] is raised when M_s has a non-zero element (cleared by the caller).
// Nothing here knows what M is: current.hip's cross-correlation passes the species currents.
__global__ void k_onsager_combos(const double* __restrict__ M, int S, long T, int D, long pitch, double* __restrict__ pm,
                                 int* __restrict__ nz) {
    const long n_cols = (long)S * S * D, n_pairs = (n_cols + 1) / 2;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long pair = blockIdx.y;
    if (t >= pitch || pair >= n_pairs) return;
    double v[2] = {0.0, 0.0};
    if (t < T) {
        for (int h = 0; h < 2; ++h) {
            const long c = 2 * pair + h;
            if (c >= n_cols) break;
            const int p = (int)(c / D), d = (int)(c % D), i = p / S, j = p % S;
            const double mi = M[((long)i * T + t) * D + d], mj = M[((long)j * T + t) * D + d];
            v[h] = i == j ? mi : i < j ? mi + mj : mi - mj;
            if (i == j && mi != 0.0) atomicOr(&nz[i], 1);
        }
    }
    reinterpret_cast<double2*>(pm)[pair * pitch + t] = double2{v[0], v[1]};
}

// C[k, i, j] = 1/4 (MSD(M_i + M_j) - MSD(M_i - M_j))[k] from the (T, S^2) by-particle array of the pseudo-particles; the
// diagonal is the MSD of M_i itself; both triangles get the same bits; lag 0, and every pair with an all-zero moment, is
// exactly 0.
__global__ void k_onsager_finish(const double* __restrict__ bp, int S, long T, const int* __restrict__ nz,
                                 double* __restrict__ C) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * S * S) return;
    const long k = idx / (S * S);
    const int i = (int)(idx % (S * S)) / S, j = (int)(idx % (S * S)) % S;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    double c = 0.0;
    if (k > 0 && nz[i] && nz[j]) {
        const double* row = bp + k * (long)S * S;
        c = i == j ? row[i * S + i] : 0.25 * (row[lo * S + hi] - row[hi * S + lo]);
    }
    C[idx] = c;
}

template <int SMAX, int ROWS, int U>
void ons_launch_one(dim3 grid, hipStream_t st, const double* pos, long pitch, long T, long n_cols, int D, int S,
                    const int* species, const double* w, double* partial) {
    hipLaunchKernelGGL((k_species_moment<SMAX, ROWS, U>), grid, dim3(kOnsThreads), 0, st, pos, pitch, T, n_cols, D, S, species,
                       w, partial);
}

}  // namespace

int species_moment_parts(int n_cu, int S, long T, long n_cols) {
    // as cond_moment_parts: about eight workgroups per CU over the frame blocks, at most one group per pair and 1024 groups
    const long fpb = (long)kOnsThreads * ons_class(S).rows;
    const long n_tb = (T + fpb - 1) / fpb;
    const long n_pairs = (n_cols + 1) / 2;
    const long want = (8L * n_cu + n_tb - 1) / n_tb;
    return (int)std::max(1L, std::min({want, n_pairs, 1024L}));
}

hipError_t launch_species_moment(const double* pos, long pitch, long T, long n_cols, int D, int S, const int* species,
                                 const double* w, double* partial, int n_parts, hipStream_t st) {
    if (D < 1 || D > 3 || S < 1 || S > TA_ONSAGER_MAX_SPECIES || n_parts < 1 || n_parts > 65535 ||
        n_cols < 1 || n_cols >= (1L << 31))
        return hipErrorInvalidValue;
    const OnsClass& k = ons_class(S);
    const long fpb = (long)kOnsThreads * k.rows;
    const dim3 grid((unsigned)((T + fpb - 1) / fpb), (unsigned)n_parts);
    if (k.smax == 2) ons_launch_one<2, 4, 1>(grid, st, pos, pitch, T, n_cols, D, S, species, w, partial);
    else if (k.smax == 4) ons_launch_one<4, 2, 2>(grid, st, pos, pitch, T, n_cols, D, S, species, w, partial);
    else ons_launch_one<8, 1, 4>(grid, st, pos, pitch, T, n_cols, D, S, species, w, partial);
    return hipGetLastError();
}

hipError_t launch_onsager_combos(const double* M, int S, long T, int D, long pitch, double* pm, int* nz, hipStream_t st) {
    const long n_pairs = ((long)S * S * D + 1) / 2;
    hipLaunchKernelGGL(k_onsager_combos, dim3((unsigned)((pitch + 255) / 256), (unsigned)n_pairs), dim3(256), 0, st, M, S, T, D,
                       pitch, pm, nz);
    return hipGetLastError();
}

hipError_t launch_onsager_finish(const double* bp, int S, long T, const int* nz, double* C, hipStream_t st) {
    const long n = T * S * S;
    hipLaunchKernelGGL(k_onsager_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bp, S, T, nz, C);
    return hipGetLastError();
}

}  // namespace ta
