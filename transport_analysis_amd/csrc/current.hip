// current.hip — species currents of a staged velocity slab and the finish of their cross-correlation (Green-Kubo
// conductivity and Onsager transport coefficients, OnsagerGreenKubo / ConductivityGreenKubo).
//
//   J[s, t, d] = sum_{n: species[n] = s} w_n v[t, n, d]                          ((n_species, n_frames, dim))
//
// k_species_current is k_species_moment (onsager.hip) without the first-frame shift and on the slab's own element type:
// the slab is read ONCE, in 16-byte loads along time, whatever the number of species; a float64 slab gives one frame of
// a column pair per load, a float32 slab (8-byte rows) two consecutive frames, widened in registers and summed in
// float64.  The currents leave as partial sums per group of column pairs, added afterwards in a fixed order by
// k_sum_partials (no atomics: the same bits from run to run).  Their cross-correlation C[k, i, j] is evaluated by the VACF
// paths on S^2 pseudo-particles (api.hip: cur_cross); k_onsager_combos (onsager.hip) and k_current_finish are its two ends.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "species_acc.hpp"
#include "ta_internal.hpp"

namespace ta {
namespace {

// the other lane of a lane pair (2 m, 2 m + 1): a DPP move, quad_perm [1, 0, 3, 2]; every lane of the wave takes part
__device__ __forceinline__ float cur_swap(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, true));
}

// Workgroup (bx, g): frames [256 ROWS bx, 256 ROWS (bx + 1)), column pairs g, g + G, g + 2 G, ... (G = gridDim.y), U of
// them per trip, ROWS U 16-byte loads per thread in flight (float32, ROWS = 1: U of them, see below).  A thread owns
// ROWS frames and keeps their SMAX x 3 sums in registers across the pairs; accumulator i belongs to frame
//   float64            : t0 + 256 i, t0 = 256 ROWS bx + tid           (a load = row t of the pair: x[t], y[t])
//   float32, ROWS >= 2 : 2 (q0 + 256 (i / 2)) + i % 2, q0 = 128 ROWS bx + tid
//                        (a load = rows 2 q, 2 q + 1 of the pair; the workgroup's loads of a pair are 4 KiB in a row)
//   float32, ROWS == 1 : 256 bx + tid.  Two frames per thread would double the accumulators (128 VGPRs for the 8-species
//                        class), so the lanes work in pairs instead: lanes 2 m and 2 m + 1 both address rows 2 q, 2 q + 1
//                        (q = 128 bx + m), the even lane of pair A = pair + u G, the odd lane of pair B = pair + (u + 1) G,
//                        and they swap halves: the even lane ends up with row 2 q of A and B, the odd lane with row
//                        2 q + 1 of both.  The workgroup's loads of one pair are 2 KiB in a row; U is even.
// Rows >= T are never stored; a load that would start at or past row T reads row 0 instead, and with an odd T the last
// load's second row is row T < pitch (pitch is a multiple of 8): nothing is read outside the pair's pitch rows.
// Everything that picks an accumulator -- the species of the pair's two columns (two atoms for a straddling pair,
// possibly of different species) and their dims -- depends on blockIdx and the loop counter only: it is read through
// readfirstlane, so OnsAcc's index is a scalar.  A label outside [0, S) is skipped (the host-facing calls reject it
// before it gets here); the unpaired last column's partner is skipped too.  partial[g][s][t][d] is written in full for
// s < S, t < T: a species without atoms gives zeros.  There is no term that depends on frame 0.
template <class E, int SMAX, int ROWS, int U>
__global__ void __launch_bounds__(kOnsThreads)
    k_species_current(const E* __restrict__ vel, long pitch, long T, long n_cols, int D, int S,
                      const int* __restrict__ species, const double* __restrict__ w, double* __restrict__ partial) {
    constexpr bool kF32 = std::is_same_v<E, float>;
    static_assert(!kF32 || ROWS % 2 == 0 || (ROWS == 1 && U % 2 == 0), "float32: whole loads per thread or lane pairs");
    const long n_pairs = (n_cols + 1) / 2;
    const long g = blockIdx.y, G = gridDim.y;
    const long tb = (long)blockIdx.x * (kOnsThreads * ROWS);
    auto frame = [&](int i) -> long {
        if constexpr (kF32 && ROWS >= 2) return tb + 2 * ((long)threadIdx.x + kOnsThreads * (i / 2)) + i % 2;
        else return tb + threadIdx.x + kOnsThreads * i;
    };
    OnsAcc<SMAX> acc[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) acc[i].clear();
    for (long pair = g; pair < n_pairs; pair += G * U) {
        double rx[U][ROWS], ry[U][ROWS];  // the trip's velocities: all loads are issued before any is used
        // (a pair index past the end reads the trip's first pair again and adds nothing below)
        auto pair_of = [&](int u) { return pair + (long)u * G < n_pairs ? pair + (long)u * G : pair; };
        if constexpr (!kF32) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double2* x = reinterpret_cast<const double2*>(vel) + pair_of(u) * pitch;
#pragma unroll
                for (int i = 0; i < ROWS; ++i) {
                    const long t = frame(i);
                    const double2 xt = x[t < T ? t : 0];
                    rx[u][i] = xt.x, ry[u][i] = xt.y;
                }
            }
        } else if constexpr (ROWS >= 2) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float4* x = reinterpret_cast<const float4*>(vel) + pair_of(u) * (pitch / 2);
#pragma unroll
                for (int i = 0; i < ROWS; i += 2) {
                    const long t = frame(i);  // even
                    const float4 xt = x[t < T ? t / 2 : 0];
                    rx[u][i] = (double)xt.x, ry[u][i] = (double)xt.y;
                    rx[u][i + 1] = (double)xt.z, ry[u][i + 1] = (double)xt.w;
                }
            }
        } else {
            const bool odd = threadIdx.x & 1;
            const long t = frame(0) - odd;  // the lane pair's even frame
#pragma unroll
            for (int u = 0; u < U; u += 2) {
                const float4* x = reinterpret_cast<const float4*>(vel) + pair_of(odd ? u + 1 : u) * (pitch / 2);
                const float4 xt = x[t < T ? t / 2 : 0];
                const float ox = cur_swap(odd ? xt.x : xt.z), oy = cur_swap(odd ? xt.y : xt.w);
                rx[u][0] = (double)(odd ? ox : xt.x), ry[u][0] = (double)(odd ? oy : xt.y);
                rx[u + 1][0] = (double)(odd ? xt.z : ox), ry[u + 1][0] = (double)(odd ? xt.w : oy);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long p = pair + (long)u * G;
            const long c0 = 2 * p, c1 = c0 + 1;
            int s0 = -1, s1 = -1, d0 = 0, d1 = 0;
            double w0 = 0.0, w1 = 0.0;
            if (c0 < n_cols) {
                const unsigned a0 = ons_atom((unsigned)c0, D);  // (n_cols < 2^31: launch_species_current)
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
        const long t = frame(i);
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

// C[k, i, j] = 1/4 (ACF(J_i + J_j) - ACF(J_i - J_j))[k] from the (T, S^2) by-particle array of the pseudo-particles; the
// diagonal is the ACF of J_i itself; both triangles get the same bits; every pair with an all-zero current is exactly 0.
// Lag 0 is kept: C[0, i, j] = <J_i . J_j>.
__global__ void k_current_finish(const double* __restrict__ bp, int S, long T, const int* __restrict__ nz,
                                 double* __restrict__ C) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * S * S) return;
    const long k = idx / (S * S);
    const int i = (int)(idx % (S * S)) / S, j = (int)(idx % (S * S)) % S;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    double c = 0.0;
    if (nz[i] && nz[j]) {
        const double* row = bp + k * (long)S * S;
        c = i == j ? row[i * S + i] : 0.25 * (row[lo * S + hi] - row[hi * S + lo]);
    }
    C[idx] = c;
}

template <class E, int SMAX, int ROWS, int U>
void cur_launch_one(dim3 grid, hipStream_t st, const void* vel, long pitch, long T, long n_cols, int D, int S,
                    const int* species, const double* w, double* partial) {
    hipLaunchKernelGGL((k_species_current<E, SMAX, ROWS, U>), grid, dim3(kOnsThreads), 0, st, (const E*)vel, pitch, T, n_cols, D,
                       S, species, w, partial);
}
template <class E>
void cur_launch(int smax, dim3 grid, hipStream_t st, const void* vel, long pitch, long T, long n_cols, int D, int S,
                const int* species, const double* w, double* partial) {
    if (smax == 2) cur_launch_one<E, 2, 4, 1>(grid, st, vel, pitch, T, n_cols, D, S, species, w, partial);
    else if (smax == 4) cur_launch_one<E, 4, 2, 2>(grid, st, vel, pitch, T, n_cols, D, S, species, w, partial);
    else cur_launch_one<E, 8, 1, 4>(grid, st, vel, pitch, T, n_cols, D, S, species, w, partial);
}

}  // namespace

// (the groups of pairs are species_moment_parts': the same frame blocks per class for both element types)
hipError_t launch_species_current(const void* vel, bool f32, long pitch, long T, long n_cols, int D, int S, const int* species,
                                  const double* w, double* partial, int n_parts, hipStream_t st) {
    if (D < 1 || D > 3 || S < 1 || S > TA_ONSAGER_MAX_SPECIES || n_parts < 1 || n_parts > 65535 ||
        n_cols < 1 || n_cols >= (1L << 31) || (pitch & 1))
        return hipErrorInvalidValue;
    const OnsClass& k = ons_class(S);
    const long fpb = (long)kOnsThreads * k.rows;
    const dim3 grid((unsigned)((T + fpb - 1) / fpb), (unsigned)n_parts);
    if (f32) cur_launch<float>(k.smax, grid, st, vel, pitch, T, n_cols, D, S, species, w, partial);
    else cur_launch<double>(k.smax, grid, st, vel, pitch, T, n_cols, D, S, species, w, partial);
    return hipGetLastError();
}

hipError_t launch_current_finish(const double* bp, int S, long T, const int* nz, double* C, hipStream_t st) {
    const long n = T * S * S;
    hipLaunchKernelGGL(k_current_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bp, S, T, nz, C);
    return hipGetLastError();
}

}  // namespace ta
