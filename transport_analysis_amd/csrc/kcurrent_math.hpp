// kcurrent_math.hpp — the arithmetic behind the current correlation functions that the kernels of kcurrent.hip and the CPU
// backend (cpu_backend.cpp) share (include/ta_hip.h, ta_kcurrent):
//   k^ = k / |k|,  |k|^2 = k_0 k_0, then fma(k_1, k_1, .), then fma(k_2, k_2, .);
//   jL = sum_d k^[d] current[d]  (a product, then one fma per further term; real and imaginary parts apart);
//   jT[d] = current[d] - k^[d] jL = fma(-k^[d], jL, current[d]);
//   trans = (bp[jT_0] + bp[jT_1] + ...) / (D - 1), in this order.
// Every product and sum below is either alone in its statement or an explicit fma: nothing is left for the compiler to
// contract, whatever -ffp-contract says.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define TA_KC_HD __host__ __device__ __forceinline__
#else
#define TA_KC_HD inline
#endif

namespace ta {

// pseudo-atoms per wavevector of the projected slab: jL, then (D > 1) the D components of jT
TA_KC_HD int kcur_series(int D) { return D > 1 ? 1 + D : 1; }

// |k|^2 of D components (0 for the zero vector: the entries refuse it)
inline double kcur_norm2(int D, const double* k) {
    double s = k[0] * k[0];
    for (int d = 1; d < D; ++d) s = std::fma(k[d], k[d], s);
    return s;
}
// the unit vector (formed once per call on the host)
inline void kcur_khat(int D, const double* k, double* kh) {
    const double n = std::sqrt(kcur_norm2(D, k));
    for (int d = 0; d < D; ++d) kh[d] = k[d] / n;
}

// cur: D (re, im) pairs of one (wavevector, frame) -> out: kcur_series(D) (re, im) pairs
TA_KC_HD void kcur_project(int D, const double* kh, const double* cur, double* out) {
    double lr = kh[0] * cur[0];
    double li = kh[0] * cur[1];
    for (int d = 1; d < D; ++d) {
        lr = fma(kh[d], cur[2 * d], lr);
        li = fma(kh[d], cur[2 * d + 1], li);
    }
    out[0] = lr, out[1] = li;
    if (D > 1)
        for (int d = 0; d < D; ++d) {
            out[2 + 2 * d] = fma(-kh[d], lr, cur[2 * d]);
            out[3 + 2 * d] = fma(-kh[d], li, cur[2 * d + 1]);
        }
}

// row: the kcur_series(D) autocorrelations of one (lag, wavevector) -> the longitudinal and the transverse value
TA_KC_HD void kcur_finish(int D, const double* row, double* lon, double* trans) {
    *lon = row[0];
    double t = 0.0;
    if (D > 1) {
        t = row[1];
        for (int d = 1; d < D; ++d) t = t + row[1 + d];
        t = t / (double)(D - 1);
    }
    *trans = t;
}

}  // namespace ta
