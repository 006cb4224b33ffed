// bond_math.hpp — the arithmetic of the bond lifetimes (include/ta_hip.h, ta_bond_lifetime) that the kernels of
// bond_lifetime.hip and the CPU backend (cpu_backend.cpp) share, on top of pair_math.hpp's distance.  A bond is a row of
// NAT staged items: a pair (p, q) or a triplet (d, h, a) = donor, hydrogen, acceptor.  In frame t, with the box of frame t,
//   r2  = vhd_r2 between the FIRST and the LAST item of the row, exactly as pair_bonded forms it;
//   u_j = image(x_d,j - x_h,j),  v_j = image(x_a,j - x_h,j)                   (triplets; vhd_image per periodic axis)
//   dot = u_0 v_0, then fma(u_1, v_1, dot), then fma(u_2, v_2, dot);  uu and vv the same way
//   ang_ok(c2) = dot <= 0 && dot dot >= (c2 uu) vv,   c2 = fl(cos_cut cos_cut) formed once on the host:
//                the angle at the hydrogen is at least acos(cos_cut) for cos_cut in [-1, 0], without a root or an acos.
//                INCLUSIVE (a triplet exactly on the angle is bonded); the distance test stays STRICT, as pair_bonded's.
//   form = r2 < rc2 && ang_ok(c2),  brk = r2 < rb2 && ang_ok(cb2)  (rb2 >= rc2, cb2 <= c2: form implies brk)
//   s    = brk ? (form ? 2 : 1) : 0                                          the LEVEL of the bond in the frame
// Every product is alone in its statement or an explicit fma: nothing is left for the compiler to contract, so both
// backends get the same bits and their outputs are equal for any input.
//
// The filters work on the series packed 64 frames to a word (bit i of word j = frame 64 j + i), S the frames of level 2 and
// W those of level >= 1 (S is a subset of W):
//   hysteresis  h(t) = S(t) || (W(t) && h(t - 1)), h(-1) = 0: bond_hyst_word fills the S bits (and the carry h(64 j - 1)
//               into bit 0) upward through the runs of W bits in six shift / and / or steps; a word of 64 W bits passes
//               the carry through.  The next carry is bit 63 of the result.
//   closing     g(t) = h(t) || (t1 < t < t2 with h(t1) = h(t2) = 1 and t2 - t1 - 1 <= gap): with gap <= 63 both t1 and
//               t2 are at most 63 frames from t, so the words before, at and behind t's decide (bond_close_bit): this
//               three-word window is why gap stops at 63.  Absences at either end of the series have no t1 or no t2 and
//               are never filled (the words outside the series are zeros).
#pragma once
#include "pair_math.hpp"

namespace ta {

// the three dot products of a triplet's arms u = image(d - h), v = image(a - h)
template <int D, bool PERIODIC>
TA_VH_HD void bond_dots(const double (&d)[3], const double (&h)[3], const double (&a)[3], const double (&H)[3], const double (&M)[3],
                        double& dot, double& uu, double& vv) {
    double u0 = d[0] - h[0], v0 = a[0] - h[0];
    if constexpr (PERIODIC) u0 = vhd_image(u0, H[0], M[0]), v0 = vhd_image(v0, H[0], M[0]);
    dot = u0 * v0;
    uu = u0 * u0;
    vv = v0 * v0;
    if constexpr (D > 1) {
        double u1 = d[1] - h[1], v1 = a[1] - h[1];
        if constexpr (PERIODIC) u1 = vhd_image(u1, H[1], M[1]), v1 = vhd_image(v1, H[1], M[1]);
        dot = fma(u1, v1, dot), uu = fma(u1, u1, uu), vv = fma(v1, v1, vv);
    }
    if constexpr (D > 2) {
        double u2 = d[2] - h[2], v2 = a[2] - h[2];
        if constexpr (PERIODIC) u2 = vhd_image(u2, H[2], M[2]), v2 = vhd_image(v2, H[2], M[2]);
        dot = fma(u2, v2, dot), uu = fma(u2, u2, uu), vv = fma(v2, v2, vv);
    }
}

TA_VH_HD bool bond_ang_ok(double dot, double uu, double vv, double c2) {
    const double dd = dot * dot;
    const double cu = c2 * uu;
    const double rhs = cu * vv;
    return dot <= 0.0 && dd >= rhs;
}

// the squared cutoffs of a call: rc2 <= rb2 the distances, c2 >= cb2 the cosines (ignored by pairs)
struct BondCuts {
    double rc2, rb2, c2, cb2;
};

// the level s of one bond in one frame; x[0 ... NAT - 1] its items in row order
template <int D, bool PERIODIC, int NAT>
TA_VH_HD int bond_level(const double (&x)[NAT][3], const double (&H)[3], const double (&M)[3], const BondCuts& k) {
    const double r2 = vhd_r2<D, PERIODIC>(x[0], x[NAT - 1], H, M);
    bool form = r2 < k.rc2, brk = r2 < k.rb2;
    if constexpr (NAT == 3) {
        double dot, uu, vv;
        bond_dots<D, PERIODIC>(x[0], x[1], x[2], H, M, dot, uu, vv);
        form = form && bond_ang_ok(dot, uu, vv, k.c2);
        brk = brk && bond_ang_ok(dot, uu, vv, k.cb2);
    }
    return brk ? (form ? 2 : 1) : 0;
}

// the level of an observed item in a frame against a GROUP of reference items (ta_shell_residence): form = some reference
// item other than itself is closer than sqrt(rc2), brk = some is closer than sqrt(rb2) (rb2 >= rc2: form implies brk)
TA_VH_HD int shell_level(bool form, bool brk) { return brk ? (form ? 2 : 1) : 0; }

// one word of h from its S and W bits and the carry h(frame before the word): a fixed six steps, whatever the data
TA_VH_HD unsigned long long bond_hyst_word(unsigned long long S, unsigned long long W, bool carry) {
    unsigned long long g = S | (carry ? W & 1ull : 0ull), p = W;
    g |= p & (g << 1), p &= p << 1;
    g |= p & (g << 2), p &= p << 2;
    g |= p & (g << 4), p &= p << 4;
    g |= p & (g << 8), p &= p << 8;
    g |= p & (g << 16), p &= p << 16;
    g |= p & (g << 32);
    return g;
}

// is the clear bit i of the h word `cur` inside an absence of at most `gap` frames (0 ... 63) between two set bits?
// prev, next: the h words before and behind (zeros outside the series)
TA_VH_HD bool bond_close_bit(unsigned long long prev, unsigned long long cur, unsigned long long next, int i, int gap) {
    // below: the 64 frames under the bit, the nearest in bit 63; above: the 64 frames over it, the nearest in bit 0
    const unsigned long long below = i ? (cur << (64 - i)) | (prev >> i) : prev;
    const unsigned long long above = i < 63 ? (cur >> (i + 1)) | (next << (63 - i)) : next;
    if (!below || !above) return false;
    // t - t1 = clz(below) + 1, t2 - t = ctz(above) + 1: the absence has t2 - t1 - 1 = clz + ctz + 1 frames
    return pair_clz64(below) + __builtin_ctzll(above) + 1 <= gap;
}

}  // namespace ta
