// vanhove_distinct_math.hpp — the arithmetic of the distinct van Hove histogram that k_vhd_pairs (vanhove_distinct.hip) and
// the CPU backend (cpu_backend.cpp) share, on top of vanhove_math.hpp's r2 order, squared-edge table and bin
// (include/ta_hip.h, ta_vanhove_distinct):
//   d_j = x[t + tau, b_q, j] - x[t, a_p, j] in float64;
//   periodic axis: sc = d_j M_j;  k = rint(sc);  d_j = fma(-k, H_j, d_j)      (H_j the box length, M_j = 1 / H_j: the diagonal
//                                                                               entries of unwrap_box.hpp's table)
//   r2 = d_0 d_0, then fma(d_1, d_1, r2), then fma(d_2, d_2, r2);   bin = vh_bin(r2, ...)
// Every product below is either alone in its statement or an explicit fma: nothing is left for the compiler to contract,
// whatever -ffp-contract says, so both backends get the same bits and their counts are equal for any input.
#pragma once
#include "vanhove_math.hpp"

namespace ta {

// the one-step image of a difference along a periodic axis (the minimum image while |d| stays below 1.5 H)
TA_VH_HD double vhd_image(double d, double H, double M) {
    const double sc = d * M;
    const double k = rint(sc);
    return fma(-k, H, d);
}

// a: the a-item at the origin frame, b: the b-item at the lagged frame; H, M: the box of the origin frame per column
template <int D, bool PERIODIC>
TA_VH_HD double vhd_r2(const double (&a)[3], const double (&b)[3], const double (&H)[3], const double (&M)[3]) {
    double d0 = b[0] - a[0];
    if constexpr (PERIODIC) d0 = vhd_image(d0, H[0], M[0]);
    double r2 = d0 * d0;
    if constexpr (D > 1) {
        double d1 = b[1] - a[1];
        if constexpr (PERIODIC) d1 = vhd_image(d1, H[1], M[1]);
        r2 = fma(d1, d1, r2);
    }
    if constexpr (D > 2) {
        double d2 = b[2] - a[2];
        if constexpr (PERIODIC) d2 = vhd_image(d2, H[2], M[2]);
        r2 = fma(d2, d2, r2);
    }
    return r2;
}

// the origins of a lag: t = stride o with t + tau < T
inline long long vhd_origins(long long T, long long tau, long long stride) { return (T - tau + stride - 1) / stride; }

}  // namespace ta
