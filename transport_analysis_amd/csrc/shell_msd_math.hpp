// shell_msd_math.hpp — the arithmetic of the shell-resolved MSD that the kernels of shell_msd.hip and the CPU backend
// (cpu_backend.cpp) share (include/ta_hip.h, ta_shell_msd).  g is ta_shell_residence's 0/1 series of one observed item,
// packed 64 frames to a word (bit i of word j = frame 64 j + i, frames at or past T clear).  A term (origin s, lag k, axis j)
//   w (x_j(s + k) - x_j(s))^2,   the difference in float64 after widening the slab's elements, no image,
// is added by fma(d, d, acc) in both backends, and its gate w is
//   "continuous": k < left(s), left(s) = the frames from s on to the first frame outside (0: s is outside),
//   "endpoints":  bit s + k of g, given that bit s is set.
// left comes from a walk over the words from the last one down with one carry, the position of the first clear bit behind the
// word (shell_left, shell_left_carry); the end-point bits of 64 consecutive origins at one lag are one 64-bit window of two
// neighbouring words (shell_window), whose AND with the origins' word counts that lag's terms by a popcount.
#pragma once
#include <cmath>
#include <cstdint>

#include "vanhove_distinct_math.hpp"

namespace ta {

enum { SHELL_CONTINUOUS = 0, SHELL_ENDPOINTS = 1 };
constexpr int64_t kShellMsdMaxLag = 2047;  // the cap on max_lag: eight passes of 256 lags

// one gated term of one axis
TA_VH_HD double shell_msd_add(double acc, double x_origin, double x_lagged) {
    const double d = x_lagged - x_origin;
    return fma(d, d, acc);
}

// bits [sh, sh + 64) of the 128-bit number hi : lo (sh = 0 ... 63)
TA_VH_HD unsigned long long shell_window(unsigned long long lo, unsigned long long hi, int sh) {
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

// frame `base + i` of word m (i = 0 ... 63): the frames from it on to the first clear bit; behind: the position of the first
// clear bit behind the word (shell_left_carry of the words behind it)
TA_VH_HD long long shell_left(unsigned long long m, int i, long long base, long long behind) {
    const unsigned long long z = ~m >> i;
    return z ? (long long)__builtin_ctzll(z) : behind - (base + i);
}
// ... and that position as the word in front sees it
TA_VH_HD long long shell_left_carry(unsigned long long m, long long base, long long behind) {
    return ~m ? base + (long long)__builtin_ctzll(~m) : behind;
}

}  // namespace ta
