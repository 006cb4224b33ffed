// orient_math.hpp — the arithmetic of the orientation pass that k_orient (orient.hip) and the CPU backend (cpu_backend.cpp)
// share (include/ta_hip.h, ta_orient):
//   d(a -> b)_j = x[t, b, j] - x[t, a, j] in float64 (a float32 slab: widened first, then subtracted);
//   with a box, one sequential image step per axis, z, then y, then x, against the rows of H (lower-triangular, the box
//   vectors) and the diagonal of M = H^-1 of unwrap_box.hpp's table:
//       k = rint(d_2 M22);  d_2 = fma(-k, H22, d_2);  d_1 = fma(-k, H21, d_1);  d_0 = fma(-k, H20, d_0)
//       k = rint(d_1 M11);  d_1 = fma(-k, H11, d_1);  d_0 = fma(-k, H10, d_0)
//       k = rint(d_0 M00);  d_0 = fma(-k, H00, d_0)
//   An orthorhombic box is the same code with zero off-diagonals: fma(-k, 0, d) = d exactly, so one path serves both box
//   shapes bit for bit.  This is the MINIMUM image only while the vector is shorter than half the smallest box width (the
//   distance between opposite faces): a bond, a molecule's arm.  It is not a general triclinic minimum image.
//   v: bond d(a -> b); bisector d(a -> b) + d(a -> c); normal d(a -> b) x d(a -> c)  (p = b_j c_k, then fma(b_k', c_j', -p));
//   n2 = fma(v_2, v_2, fma(v_1, v_1, v_0 v_0));  u = v / sqrt(n2);  u = 0 where n2 == 0 (or not finite: never a NaN);
//   Q = u (x) u - 1/3: the six columns (Qxx, Qyy, Qzz, sqrt2 Qxy, sqrt2 Qxz, sqrt2 Qyz) = (fma(u_j, u_j, -fl(1/3)), ...,
//   fl(sqrt 2) fl(u_j u_k), ...), whose dot product is Q : Q' = (u . u')^2 - 1/3 = 2/3 P2(u . u'); zeros where u = 0.
// Every product below is either alone in its statement or an explicit fma: nothing is left for the compiler to contract,
// whatever -ffp-contract says, so both backends run the same operation sequence.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define TA_OR_HD __host__ __device__ __forceinline__
#else
#define TA_OR_HD inline
#endif

namespace ta {

enum OrientMode { ORIENT_BOND = 0, ORIENT_BISECTOR = 1, ORIENT_NORMAL = 2 };
inline int orient_row_len(int mode) { return mode == ORIENT_BOND ? 2 : 3; }  // atoms per index row

// The nine box entries of one frame, in the row order of the device table (orient_box_rows: rows of tpitch doubles)
constexpr int kOrientBoxRows = 9;  // H00 H10 H11 H20 H21 H22 M00 M11 M22
struct OrientBox {
    double h00, h10, h11, h20, h21, h22, m00, m11, m22;
};

// d = b - a, reduced by the sequential image step when PERIODIC
template <bool PERIODIC>
TA_OR_HD void orient_diff(const double (&a)[3], const double (&b)[3], const OrientBox& bx, double (&d)[3]) {
    d[0] = b[0] - a[0], d[1] = b[1] - a[1], d[2] = b[2] - a[2];
    if constexpr (PERIODIC) {
        const double s2 = d[2] * bx.m22;
        const double k2 = rint(s2);
        d[2] = fma(-k2, bx.h22, d[2]);
        d[1] = fma(-k2, bx.h21, d[1]);
        d[0] = fma(-k2, bx.h20, d[0]);
        const double s1 = d[1] * bx.m11;
        const double k1 = rint(s1);
        d[1] = fma(-k1, bx.h11, d[1]);
        d[0] = fma(-k1, bx.h10, d[0]);
        const double s0 = d[0] * bx.m00;
        const double k0 = rint(s0);
        d[0] = fma(-k0, bx.h00, d[0]);
    }
}

// v of the two differences b = d(a -> b), c = d(a -> c) (bond: c unused)
template <int MODE>
TA_OR_HD void orient_combine(const double (&b)[3], const double (&c)[3], double (&v)[3]) {
    if constexpr (MODE == ORIENT_BOND) {
        v[0] = b[0], v[1] = b[1], v[2] = b[2];
    } else if constexpr (MODE == ORIENT_BISECTOR) {
        v[0] = b[0] + c[0], v[1] = b[1] + c[1], v[2] = b[2] + c[2];
    } else {
        const double p0 = b[2] * c[1];
        const double p1 = b[0] * c[2];
        const double p2 = b[1] * c[0];
        v[0] = fma(b[1], c[2], -p0);
        v[1] = fma(b[2], c[0], -p1);
        v[2] = fma(b[0], c[1], -p2);
    }
}

// u = v / |v|, zeros for a vector without a direction
TA_OR_HD void orient_unit(const double (&v)[3], double (&u)[3]) {
    const double s = v[0] * v[0];
    const double n2 = fma(v[2], v[2], fma(v[1], v[1], s));
    const bool ok = n2 > 0.0 && n2 - n2 == 0.0;
    const double r = sqrt(ok ? n2 : 1.0);
    u[0] = ok ? v[0] / r : 0.0;
    u[1] = ok ? v[1] / r : 0.0;
    u[2] = ok ? v[2] / r : 0.0;
}

// the six rank-2 columns of u
TA_OR_HD void orient_q(const double (&u)[3], double (&q)[6]) {
    const double third = 1.0 / 3.0, root2 = 1.4142135623730951;
    const double s = u[0] * u[0];
    const bool ok = fma(u[2], u[2], fma(u[1], u[1], s)) > 0.0;
    const double pxy = u[0] * u[1];
    const double pxz = u[0] * u[2];
    const double pyz = u[1] * u[2];
    const double sxy = root2 * pxy;
    const double sxz = root2 * pxz;
    const double syz = root2 * pyz;
    q[0] = ok ? fma(u[0], u[0], -third) : 0.0;
    q[1] = ok ? fma(u[1], u[1], -third) : 0.0;
    q[2] = ok ? fma(u[2], u[2], -third) : 0.0;
    q[3] = sxy, q[4] = sxz, q[5] = syz;
}

}  // namespace ta
