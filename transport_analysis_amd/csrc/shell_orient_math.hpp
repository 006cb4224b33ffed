// shell_orient_math.hpp — the arithmetic of the shell-resolved reorientation that k_shell_orient (shell_orient.hip) and the CPU
// backend (cpu_backend.cpp) share (include/ta_hip.h, ta_shell_orient).  u_n(t) is orient_math.hpp's unit vector (orient_diff,
// orient_combine, orient_unit; the box of the distance pass as its orthorhombic OrientBox), the gates are shell_msd_math.hpp's.
// A term (origin t, lag k) is
//   c = u(t) . u(t + k) = fma(a_2, b_2, fma(a_1, b_1, fl(a_0 b_0))),   s1 += c,   s2 = fma(c, c, s2).
// The product stands alone in its statement and the rest are explicit fmas: nothing is left for the compiler to contract.
#pragma once
#include <cmath>

#include "orient_math.hpp"
#include "shell_msd_math.hpp"

namespace ta {

// the box H[3], M[3] of the distance pass (pair family: the staged columns x, y, z) as the image step's box
TA_OR_HD OrientBox shell_orient_box(const double* hm) { return OrientBox{hm[0], 0.0, hm[1], 0.0, 0.0, hm[2], hm[3], hm[4], hm[5]}; }

// u of one vector in one frame from its atoms' positions (c unused for a bond)
template <int MODE, bool PERIODIC>
TA_OR_HD void shell_orient_unit(const double (&a)[3], const double (&b)[3], const double (&c)[3], const OrientBox& bx, double (&u)[3]) {
    double db[3], dc[3] = {0.0, 0.0, 0.0}, v[3];
    orient_diff<PERIODIC>(a, b, bx, db);
    if constexpr (MODE != ORIENT_BOND) orient_diff<PERIODIC>(a, c, bx, dc);
    orient_combine<MODE>(db, dc, v);
    orient_unit(v, u);
}

TA_OR_HD double shell_orient_dot(double a0, double a1, double a2, double b0, double b1, double b2) {
    const double p = a0 * b0;
    return fma(a2, b2, fma(a1, b1, p));
}
// one gated term: s1 += c, s2 += c c
TA_OR_HD void shell_orient_add(double& s1, double& s2, double c) {
    s1 += c;
    s2 = fma(c, c, s2);
}

}  // namespace ta
