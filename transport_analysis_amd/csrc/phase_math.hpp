// phase_math.hpp — the phase exp(i k . x) as k_phase (scatter.hip) and k_kcurrent (kcurrent.hip) form it, bit for bit the same
// in both, and the host half that scatter_plan and kcurrent_plan (api.hip) apply to the wavevectors:
//   the host passes q = k / (2 pi), turns per length unit, as float64;
//   u = fma(q[2], x[2], fma(q[1], x[1], q[0] x[0]))   (as many terms as D),   r = u - rint(u)   (|r| <= 1/2, exact),
//   (cos, sin)(2 pi r) by sincospi(2 r).
// The reduced argument keeps sincospi on its fast path: no large-argument reduction, no table in private memory.  (The CPU
// backend follows this arithmetic with an expression of its own.)
#pragma once
#include <hip/hip_runtime.h>

namespace ta {

// k -> q, one component
inline double phase_turns(double k) { return k / 6.283185307179586476925; }

// (cos, sin)(k . x) of one position (q1, q2: unused beyond D)
template <int D>
__device__ __forceinline__ double2 phase_cs(double q0, double q1, double q2, const double (&x)[3]) {
    double u = q0 * x[0];
    if constexpr (D > 1) u = fma(q1, x[1], u);
    if constexpr (D > 2) u = fma(q2, x[2], u);
    const double r = u - rint(u);
    double s, c;
    sincospi(2.0 * r, &s, &c);
    return double2{c, s};
}

}  // namespace ta
