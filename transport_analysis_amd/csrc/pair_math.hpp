// pair_math.hpp — the arithmetic of the pair lifetime correlations that the kernels of pair_lifetime.hip and the CPU backend
// (cpu_backend.cpp) share (include/ta_hip.h, ta_pair_find / ta_pair_lifetime).  The bond indicator of items p and q in
// frame t is
//   h = vhd_r2<D, PERIODIC>(x_p(t), x_q(t), H(t), M(t)) < rc2,      rc2 = fl(r_cut r_cut), formed once on the host,
// with vanhove_distinct_math.hpp's difference, one-step image and r2 order: both backends get the same bits, so their found
// lists, run-length histograms and (fft = 0) lag sums are equal for any input.  Both items are taken at the SAME frame: the
// box of frame t reduces frame t, whatever the other frames' boxes are.
//
// The runs of a 0/1 series packed 64 frames to a word (bit i of word j = frame 64 j + i) are walked word by word with one
// carry, the length of the run still open at the end of the word before: pair_runs_word gives, for a set bit i whose
// successor inside the word is clear (a run's end; bit 63 never is one here, its run goes on into the carry), the run's
// length.  The kernel asks it per lane, the CPU backend per end bit; pair_runs_carry is the carry behind the word.
#pragma once
#include <cstdint>

#include "vanhove_distinct_math.hpp"

namespace ta {

template <int D, bool PERIODIC>
TA_VH_HD bool pair_bonded(const double (&a)[3], const double (&b)[3], const double (&H)[3], const double (&M)[3], double rc2) {
    return vhd_r2<D, PERIODIC>(a, b, H, M) < rc2;
}

TA_VH_HD int pair_clz64(unsigned long long v) { return __builtin_clzll(v); }  // (v != 0)

// bit i < 63 of m is set and bit i + 1 is clear: the length of the run that ends at i (carry: frames of it before this word)
TA_VH_HD long long pair_runs_word(unsigned long long m, int i, long long carry) {
    const unsigned long long below = ~m & ((1ull << i) - 1ull);  // the clear bits under i
    if (!below) return carry + i + 1;                             // the run started before this word (or at its bit 0)
    return i - (63 - pair_clz64(below));                          // ... or behind the highest clear bit under i
}
// the length of the run open at the end of word m (0: bit 63 is clear)
TA_VH_HD long long pair_runs_carry(unsigned long long m, long long carry) {
    if (!(m >> 63)) return 0;
    if (!~m) return carry + 64;
    return pair_clz64(~m);  // the ones above the highest clear bit
}

}  // namespace ta
