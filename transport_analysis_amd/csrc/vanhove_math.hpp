// vanhove_math.hpp — the arithmetic of the self van Hove histogram that k_vanhove (vanhove.hip) and the CPU backend
// (cpu_backend.cpp) share, so that their counts are equal for any input (include/ta_hip.h, ta_vanhove):
//   d_j = x[t + tau, n, j] - x[t, n, j] in float64;   r2 = d_0 d_0, then fma(d_1, d_1, r2), then fma(d_2, d_2, r2);
//   e[b] = fl(fl(b dr) fl(b dr)), b = 0 ... B;   bin = the last b with e[b] <= r2, B (the overflow bin) when r2 >= e[B].
// Every product and sum below is either alone in its statement or an explicit fma: nothing is left for the compiler to
// contract, whatever -ffp-contract says.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define TA_VH_HD __host__ __device__ __forceinline__
#else
#define TA_VH_HD inline
#endif

namespace ta {

// the squared edges (B + 1 of them), formed once per call on the host
inline void vh_edges(int B, double dr, double* e) {
    for (int b = 0; b <= B; ++b) {
        const double r = (double)b * dr;
        e[b] = r * r;
    }
}
// the squared cutoffs of ta_overlap (C of them), formed once per call on the host: a2[c] = fl(a_c a_c)
inline void vh_cutoffs2(int C, const double* a, double* a2) {
    for (int c = 0; c < C; ++c) a2[c] = a[c] * a[c];
}
// the float32 factor of the bin guess
inline float vh_inv_dr(double dr) { return (float)(1.0 / dr); }

template <int D>
TA_VH_HD double vh_r2(const double (&a)[3], const double (&b)[3]) {
    const double d0 = b[0] - a[0];
    double r2 = d0 * d0;
    if constexpr (D > 1) {
        const double d1 = b[1] - a[1];
        r2 = fma(d1, d1, r2);
    }
    if constexpr (D > 2) {
        const double d2 = b[2] - a[2];
        r2 = fma(d2, d2, r2);
    }
    return r2;
}

// r2 of one pair as k_overlap (overlap.hip) and k_overlap_density (overlap_density.hip) take it: NaN (which no cutoff counts)
// for a pair whose lagged frame is at or past T
template <int D>
TA_VH_HD double ov_r2(bool live, const double (&x0)[3], const double (&x1)[3]) {
    const double r2 = vh_r2<D>(x0, x1);
    return live ? r2 : __builtin_nan("");
}

// A float32 guess (r2 >= 0, so it is >= 0; capped at B, which a NaN becomes too), stepped down and up against the table:
// the result is the bin of the definition whatever the guess was.  A NaN r2 compares false both ways from B: the overflow bin.
TA_VH_HD int vh_bin(double r2, const double* e, int B, float inv_dr) {
    int g = (int)fminf(sqrtf((float)r2) * inv_dr, (float)B);
    while (g > 0 && r2 < e[g]) --g;
    while (g < B && r2 >= e[g + 1]) ++g;
    return g;
}

}  // namespace ta
