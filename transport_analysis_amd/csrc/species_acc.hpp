// species_acc.hpp — the per-frame species accumulators and the column -> atom mapping shared by k_species_moment
// (onsager.hip) and k_species_current (current.hip)
#pragma once
#include <hip/hip_runtime.h>

namespace ta {

constexpr int kOnsThreads = 256;

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

// The species classes of the two templates: rows per thread x pairs per trip is 4 everywhere (64 bytes in flight per
// thread, as k_cond_moment), and every class holds 32 float64 accumulator slots per thread (4 x 8, 2 x 16, 1 x 2 x 16)
struct OnsClass {
    int smax, rows, pairs;
};
constexpr OnsClass kOnsClasses[] = {{2, 4, 1}, {4, 2, 2}, {8, 1, 4}};
inline const OnsClass& ons_class(int S) { return kOnsClasses[S <= 2 ? 0 : S <= 4 ? 1 : 2]; }

}  // namespace ta
