// chain_math.hpp — the arithmetic of the chain pass that k_chain_modes (chain_modes.hip) and the CPU backend (cpu_backend.cpp)
// share (include/ta_hip.h, ta_chain_modes).  A chain is an ordered list of N >= 2 beads; per frame, in bead order:
//   s_1 = 0;   d = orient_diff(x[m_{n-1}], x[m_n])   (orient_math.hpp: the float64 difference, with a box one sequential
//              image step per axis, z, then y, then x, of the frame's own box);   s_j = s_j + d_j        (a plain add)
//   per functional q, from acc = 0:   acc_j = fma(coeff[q][n - 1], s_j, acc_j)        n = 2 ... N
// s is the chain made whole relative to its first bead (the MINIMUM image while every bond is shorter than half the smallest
// box width, orient_diff's condition), acc the linear functional Y_q = sum_n coeff[q][n - 1] s_n of the whole chain.  The
// coefficient of the first bead never enters (s_1 = 0): a functional whose coefficients sum to zero, such as a Rouse mode,
// is the same functional of the absolute positions.
// Every product below is an explicit fma: nothing is left for the compiler to contract, whatever -ffp-contract says, so both
// backends run the same operation sequence.  OrientBox and orient_diff are orient_math.hpp's own.
#pragma once
#include "orient_math.hpp"

namespace ta {

// s += img(cur - prev): the next bead's position relative to the first
template <bool PERIODIC>
TA_OR_HD void chain_step(const double (&prev)[3], const double (&cur)[3], const OrientBox& bx, double (&s)[3]) {
    double d[3];
    orient_diff<PERIODIC>(prev, cur, bx, d);
    s[0] = s[0] + d[0];
    s[1] = s[1] + d[1];
    s[2] = s[2] + d[2];
}

// acc += coeff s: one bead's term of one functional
TA_OR_HD void chain_term(double coeff, const double (&s)[3], double (&acc)[3]) {
    acc[0] = fma(coeff, s[0], acc[0]);
    acc[1] = fma(coeff, s[1], acc[1]);
    acc[2] = fma(coeff, s[2], acc[2]);
}

}  // namespace ta
