// species_sum.hip — per-species sums over atoms of a staged slab, and the two ends of their cross-correlation.
//
//   M[s, t, d] = sum_{n: species[n] = s} w_n (x[t, n, d] - x[0, n, d])      moments of positions (OnsagerHelfand)
//   J[s, t, d] = sum_{n: species[n] = s} w_n v[t, n, d]                      currents of velocities (OnsagerGreenKubo,
//                                                                            ConductivityGreenKubo)
//
// Both are k_species_sum, with and without the first-frame shift (in the kernel timeline: k_species_moment,
// k_species_current).  It is k_cond_moment (conductivity.hip) with the sum split by a per-atom label: the slab is read
// ONCE, in 16-byte loads along time, whatever the number of species; the shift comes before the weight; a float32 slab
// is widened in registers and summed in float64.  The sums leave as partial sums per group of column pairs, added
// afterwards in a fixed order by k_sum_partials (no atomics: the same bits from run to run).  Their cross term C[k, i, j]
// is evaluated by the Einstein MSD or the VACF paths on S^2 pseudo-particles (api.hip: coll_cross); k_onsager_combos and
// k_cross_finish are its two ends.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "pm_read.hpp"
#include "ta_internal.hpp"

namespace ta {
namespace {

// The accumulators of one frame: 3 SMAX sums, reached by a workgroup-uniform index 3 s + d.  They are register VECTORS
// (at most 16 float64 = 32 VGPRs, the widest register tuple), not an array: a uniform runtime index into a vector is a
// register-indexed move (s_set_gpr_idx / v_movrel), whereas a runtime-indexed array goes to scratch, and a uniform switch
// over named registers came back from the compiler as a runtime index again, or with every accumulator copied at every
// join of its branches (164 VGPRs, ~1000 moves per trip).  SMAX = 8 needs two vectors (species 0-3, 4-7): both are updated,
// the one that does not hold the species at its unused last slot, so there is no branch at all.
template <int N>
using OnsVec = double __attribute__((ext_vector_type(N)));
template <int SMAX>
struct OnsAcc {
    static constexpr int N = SMAX == 2 ? 8 : 16, H = SMAX == 8 ? 2 : 1, kPad = N - 1;  // 6 of 8, 12 of 16, 2 x 12 of 16 used
    OnsVec<N> v[H];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int h = 0; h < H; ++h) v[h] = OnsVec<N>(0.0);
    }
    // s in [0, SMAX) or -1 (adds into the unused slot), d in [0, 3)
    __device__ __forceinline__ void add(int s, int d, double x) {
        if constexpr (H == 1) {
            const int k = s >= 0 ? s * 3 + d : kPad;
            v[0][k] += x;
        } else {
            const int k0 = s >= 0 && s < 4 ? s * 3 + d : kPad, k1 = s >= 4 ? (s - 4) * 3 + d : kPad;
            v[0][k0] += x;
            v[1][k1] += x;
        }
    }
    __device__ __forceinline__ double get(int K) const {  // K = 3 s + d, a constant once the caller's loop is unrolled
        return v[K / 12 < H ? K / 12 : 0][K % 12];
    }
};

// column -> atom for dim 1, 2, 3 by constant divisors (a 64-bit division by a runtime dim costs ~150 scalar instructions)
__device__ __forceinline__ unsigned ons_atom(unsigned c, int D) { return D == 3 ? c / 3u : D == 2 ? c >> 1 : c; }

// The species classes: rows per thread x pairs per trip is 4 everywhere (64 bytes in flight per thread, as
// k_cond_moment), and every class holds 32 float64 accumulator slots per thread (4 x 8, 2 x 16, 1 x 2 x 16)
struct OnsClass {
    int smax, rows, pairs;
};
constexpr OnsClass kOnsClasses[] = {{2, 4, 1}, {4, 2, 2}, {8, 1, 4}};
inline const OnsClass& ons_class(int S) { return kOnsClasses[S <= 2 ? 0 : S <= 4 ? 1 : 2]; }

// the other lane of a lane pair (2 m, 2 m + 1): a DPP move, quad_perm [1, 0, 3, 2]; every lane of the wave takes part
__device__ __forceinline__ float lane_swap(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, true));
}

// Workgroup (bx, g): frames [256 ROWS bx, 256 ROWS (bx + 1)), column pairs g, g + G, g + 2 G, ... (G = gridDim.y), U of
// them per trip, ROWS U 16-byte loads per thread in flight (float32, ROWS = 1: U of them, see below).  A thread owns
// ROWS frames and keeps their SMAX x 3 sums in registers across the pairs; accumulator i belongs to frame pm_frame(i)
// (pm_read.hpp), except
//   float32, ROWS == 1 : 256 bx + tid.  Two frames per thread would double the accumulators (128 VGPRs for the 8-species
//                        class), so the lanes work in pairs instead: lanes 2 m and 2 m + 1 both address rows 2 q, 2 q + 1
//                        (q = 128 bx + m), the even lane of pair A = pair + u G, the odd lane of pair B = pair + (u + 1) G,
//                        and they swap halves: the even lane ends up with row 2 q of A and B, the odd lane with row
//                        2 q + 1 of both.  The workgroup's loads of one pair are 2 KiB in a row; U is even.
// Rows >= T are never stored (pm_read.hpp's rules for the loads).  SHIFT subtracts the pair's row 0 (one address for the
// whole workgroup) before the weight; it is a template parameter so that the kernels without it carry nothing of it, and
// it exists for float64 only.
// Everything that picks an accumulator -- the species of the pair's two columns (two atoms for a straddling pair,
// possibly of different species) and their dims -- depends on blockIdx and the loop counter only: it is read through
// readfirstlane, so OnsAcc's index is a scalar.  A label outside [0, S) is skipped (the host-facing calls reject it
// before it gets here); the unpaired last column's partner is skipped too.  partial[g][s][t][d] is written in full for
// s < S, t < T: a species without atoms gives zeros.
template <class E, bool SHIFT, int SMAX, int ROWS, int U>
__global__ void __launch_bounds__(kPmThreads)
    k_species_sum(const E* __restrict__ slab, long pitch, long T, long n_cols, int D, int S, const int* __restrict__ species,
                  const double* __restrict__ w, double* __restrict__ partial) {
    constexpr bool kF32 = std::is_same_v<E, float>;
    static_assert(!(kF32 && SHIFT), "the shifted pass reads float64 slabs only");
    static_assert(!kF32 || ROWS % 2 == 0 || (ROWS == 1 && U % 2 == 0), "float32: whole loads per thread or lane pairs");
    const long n_pairs = (n_cols + 1) / 2;
    const long g = blockIdx.y, G = gridDim.y;
    const long tb = (long)blockIdx.x * (kPmThreads * ROWS);
    auto frame = [&](int i) { return pm_frame<kF32 && ROWS >= 2>(tb, i); };
    OnsAcc<SMAX> acc[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) acc[i].clear();
    for (long pair = g; pair < n_pairs; pair += G * U) {
        double rx[U][ROWS], ry[U][ROWS];  // the trip's terms before the weight: all loads are issued before any is used
        // (a pair index past the end reads the trip's first pair again and adds nothing below)
        auto pair_of = [&](int u) { return pair + (long)u * G < n_pairs ? pair + (long)u * G : pair; };
        if constexpr (!kF32) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double2* x = reinterpret_cast<const double2*>(slab) + pair_of(u) * pitch;
                double2 x0{0.0, 0.0};
                if constexpr (SHIFT) x0 = x[0];
#pragma unroll
                for (int i = 0; i < ROWS; ++i) {
                    const long t = frame(i);
                    const double2 xt = x[t < T ? t : 0];  // (a frame past the end of a shifted pass: a zero displacement)
                    rx[u][i] = SHIFT ? xt.x - x0.x : xt.x, ry[u][i] = SHIFT ? xt.y - x0.y : xt.y;
                }
            }
        } else if constexpr (ROWS >= 2) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float4* x = reinterpret_cast<const float4*>(slab) + pair_of(u) * (pitch / 2);
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
                const float4* x = reinterpret_cast<const float4*>(slab) + pair_of(odd ? u + 1 : u) * (pitch / 2);
                const float4 xt = x[t < T ? t / 2 : 0];
                const float ox = lane_swap(odd ? xt.x : xt.z), oy = lane_swap(odd ? xt.y : xt.w);
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
                const unsigned a0 = ons_atom((unsigned)c0, D);  // (n_cols < 2^31: launch_species_sum)
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

// Pair-major slab of the S^2 pseudo-particles whose lag sums give C by polarisation: particle i S + j is Q_i (i == j),
// Q_i + Q_j (i < j), Q_i - Q_j (i > j).  One thread per (row, column pair); rows T ... pitch - 1 and the partner of an
// unpaired last column are written as 0.  nz[s] is raised when Q_s has a non-zero element (cleared by the caller).
// Nothing here knows what Q is: the moments or the currents.
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

// C[k, i, j] = 1/4 (R(Q_i + Q_j) - R(Q_i - Q_j))[k] from the (T, S^2) by-particle array R (MSD or ACF) of the
// pseudo-particles; the diagonal is R(Q_i) itself; both triangles get the same bits; every pair with an all-zero sum is
// exactly 0.  lag0: C[0, i, j] = <Q_i . Q_j> is kept (currents), or exactly 0 (moments: a mean squared difference).
__global__ void k_cross_finish(const double* __restrict__ bp, int S, long T, const int* __restrict__ nz, int lag0,
                               double* __restrict__ C) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * S * S) return;
    const long k = idx / (S * S);
    const int i = (int)(idx % (S * S)) / S, j = (int)(idx % (S * S)) % S;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    double c = 0.0;
    if ((lag0 || k > 0) && nz[i] && nz[j]) {
        const double* row = bp + k * (long)S * S;
        c = i == j ? row[i * S + i] : 0.25 * (row[lo * S + hi] - row[hi * S + lo]);
    }
    C[idx] = c;
}

template <class E, bool SHIFT, class... Args>
void sum_launch(int smax, dim3 grid, hipStream_t st, const void* slab, Args... args) {
    if (smax == 2) hipLaunchKernelGGL((k_species_sum<E, SHIFT, 2, 4, 1>), grid, dim3(kPmThreads), 0, st, (const E*)slab, args...);
    else if (smax == 4) hipLaunchKernelGGL((k_species_sum<E, SHIFT, 4, 2, 2>), grid, dim3(kPmThreads), 0, st, (const E*)slab, args...);
    else hipLaunchKernelGGL((k_species_sum<E, SHIFT, 8, 1, 4>), grid, dim3(kPmThreads), 0, st, (const E*)slab, args...);
}

}  // namespace

int species_sum_parts(int n_cu, int S, long T, long n_cols) {
    // as cond_moment_parts: about eight workgroups per CU over the frame blocks, at most one group per pair and 1024 groups
    const long fpb = (long)kPmThreads * ons_class(S).rows;
    const long n_tb = (T + fpb - 1) / fpb;
    const long n_pairs = (n_cols + 1) / 2;
    const long want = (8L * n_cu + n_tb - 1) / n_tb;
    return (int)std::max(1L, std::min({want, n_pairs, 1024L}));
}

hipError_t launch_species_sum(const void* pm, bool f32, bool shift, long pitch, long T, long n_cols, int D, int S,
                              const int* species, const double* w, double* partial, int n_parts, hipStream_t st) {
    if (D < 1 || D > 3 || S < 1 || S > TA_ONSAGER_MAX_SPECIES || n_parts < 1 || n_parts > 65535 ||
        n_cols < 1 || n_cols >= (1L << 31) || (pitch & 1) || (f32 && shift))
        return hipErrorInvalidValue;
    const OnsClass& k = ons_class(S);
    const long fpb = (long)kPmThreads * k.rows;
    const dim3 grid((unsigned)((T + fpb - 1) / fpb), (unsigned)n_parts);
    if (shift) sum_launch<double, true>(k.smax, grid, st, pm, pitch, T, n_cols, D, S, species, w, partial);
    else if (f32) sum_launch<float, false>(k.smax, grid, st, pm, pitch, T, n_cols, D, S, species, w, partial);
    else sum_launch<double, false>(k.smax, grid, st, pm, pitch, T, n_cols, D, S, species, w, partial);
    return hipGetLastError();
}

hipError_t launch_onsager_combos(const double* M, int S, long T, int D, long pitch, double* pm, int* nz, hipStream_t st) {
    const long n_pairs = ((long)S * S * D + 1) / 2;
    hipLaunchKernelGGL(k_onsager_combos, dim3((unsigned)((pitch + 255) / 256), (unsigned)n_pairs), dim3(256), 0, st, M, S, T, D,
                       pitch, pm, nz);
    return hipGetLastError();
}

hipError_t launch_cross_finish(const double* bp, int S, long T, const int* nz, bool lag0, double* C, hipStream_t st) {
    const long n = T * S * S;
    hipLaunchKernelGGL(k_cross_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bp, S, T, nz, (int)lag0, C);
    return hipGetLastError();
}

}  // namespace ta
