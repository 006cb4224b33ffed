// shell_gate.hpp — the gated lag walk that the kernels behind ta_shell_residence's 0/1 series g share: k_shell_msd
// (shell_msd.hip) and k_shell_orient (shell_orient.hip) are its two instantiations.  shell_msd_math.hpp has the gates.
//
// Grid (G, passes).  Workgroup (x, y) owns the 256 lags [256 y, 256 y + 256), one per thread, and the items x, x + G, ... of
// the block, one at a time, in chunks of C origin frames (C a multiple of 64).  Per (item, chunk): the words of the chunk and of
// the lagged frames behind it go to LDS; a chunk without a frame inside is left at once (a workgroup-uniform branch: with sparse
// residence most of the work); the Source's NV values of the frames INSIDE among [c0 + 256 y, c0 + 256 y + C + 256) are kept
// in LDS as Source::Kept (a frame outside is never the lagged frame of a term under either gate, so it is not loaded); "continuous": wave 0 walks the words from the last down and leaves left(s), the frames from s on to the first
// frame outside.  Then per 64-frame word of origins (skipped where zero): lane i of every wave loads origin 64 j + i's values
// with the same Source, and per SET bit i of the word (a scalar loop, its trip count the same for every lane) the origin comes
// out of lane i by v_readlane, the lagged frame out of LDS (consecutive lanes, consecutive addresses), widened, and the Term
// runs under the gate: "continuous" lag < left(s), with origins whose run ends below the pass's first lag skipped for the
// whole workgroup; "endpoints" bit i of the thread's window of g at its lag, whose popcount against the origins' word is that
// lag's count.  A thread's NS sums and its count stay in registers over all items of the workgroup and are stored once: the
// partial rows [G][256 passes].
//
//   Source   NV, Kept, load(t, double (&v)[NV]): the values of frame t < T of one item, made per item by `make(q)`
//   Term     NS, add(double (&acc)[NS], bool gate, origin, lagged): one term, added where `gate`; origin(d), lagged(d) give
//            value d < NV of the origin (the readlane) and of the lagged frame (the LDS read), each asked for once
// No atomics, no ballots inside divergent branches; every loop's trip count depends on the shapes or on workgroup-uniform
// words of g alone.
#pragma once
#include <hip/hip_runtime.h>

#include "pm_read.hpp"
#include "shell_msd_math.hpp"

namespace ta {

constexpr int kSmLags = kPmThreads;  // lags per pass: one per thread

__device__ __forceinline__ unsigned long long sm_uniform(unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
// lane i's value (i wave-uniform), widened
__device__ __forceinline__ double sm_from_lane(double v, int i) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), i), __builtin_amdgcn_readlane(__double2loint(v), i));
}
__device__ __forceinline__ double sm_from_lane(float v, int i) {
    return (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
}

// Dynamic LDS of a walk: (C + 256 y_max + 256) / 64 words | C ints | NV (C + 256) Kept
inline size_t shell_gate_lds_bytes(int C, int n_pass, int NV, size_t kept_bytes) {
    return 8 * (size_t)((C + (n_pass - 1) * kSmLags) / 64 + 4) + 4 * (size_t)C + (size_t)NV * (C + kSmLags) * kept_bytes;
}

// words: k_shell_bits' rows of the block's n_items items (nw words each); C: origins per chunk; part_s [G][256 passes][NS],
// part_n [G][256 passes]
template <int COND, class Term, class Make>
__device__ __forceinline__ void shell_gate_walk(long T, long n_items, const unsigned long long* __restrict__ words, long nw, int C,
                                                double* __restrict__ part_s, unsigned long long* __restrict__ part_n, Make&& make) {
    using Source = decltype(make(0L));
    using Kept = typename Source::Kept;
    constexpr int NV = Source::NV, NS = Term::NS;
    extern __shared__ unsigned long long sm_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const long k0 = (long)blockIdx.y * kSmLags, lag = k0 + tid;
    const int n_ww = (int)((C + k0) / 64) + 4, n_ow = C / 64, n_x = C + kSmLags;
    unsigned long long* wd = sm_lds;                                                      // n_ww words from frame c0 on
    int* left = reinterpret_cast<int*>(sm_lds + ((C + (long)(gridDim.y - 1) * kSmLags) / 64 + 4));  // C
    Kept* xs = reinterpret_cast<Kept*>(left + C);                                         // [NV][n_x] from frame c0 + k0 on
    double acc[NS] = {};
    unsigned long long cnt = 0;
    for (long q = blockIdx.x; q < n_items; q += gridDim.x) {
        const unsigned long long* wq = words + q * nw;
        const Source src = make(q);
        for (long c0 = 0; c0 + k0 < T; c0 += C) {
            __syncthreads();  // (the chunk before has been read)
            if (tid < n_ww) wd[tid] = c0 / 64 + tid < nw ? wq[c0 / 64 + tid] : 0ull;
            __syncthreads();
            unsigned long long any = 0;
            for (int j = 0; j < n_ow; ++j) any |= wd[j];
            if (!sm_uniform(any)) continue;  // (the same words for every thread)
            for (int i = tid; i < n_x; i += kPmThreads) {
                const long t = c0 + k0 + i;
                // (under either gate the lagged frame of a term is itself inside: a frame outside is never read as one)
                if (!((wd[(k0 + i) >> 6] >> ((k0 + i) & 63)) & 1ull)) continue;
                double v[NV];
                src.load(t < T ? t : 0, v);
#pragma unroll
                for (int d = 0; d < NV; ++d) xs[d * n_x + i] = (Kept)v[d];
            }
            if (COND == SHELL_CONTINUOUS && tid < 64) {
                long long behind = c0 + 64L * n_ww;  // (frames behind the words: no lag of this pass reaches them)
                for (int w = n_ww - 1; w >= 0; --w) {
                    const unsigned long long m = wd[w];
                    if (w < n_ow) left[64 * w + lane] = (int)shell_left(m, lane, c0 + 64L * w, behind);
                    behind = shell_left_carry(m, c0 + 64L * w, behind);
                }
            }
            __syncthreads();
            for (int j = 0; j < n_ow; ++j) {
                const unsigned long long m = sm_uniform(wd[j]);
                if (!m) continue;
                const long s = c0 + 64L * j + lane;
                double o[NV] = {};
                if ((m >> lane) & 1ull) src.load(s < T ? s : 0, o);  // (only the origins inside are taken out of their lanes)
                Kept xo[NV];
#pragma unroll
                for (int d = 0; d < NV; ++d) xo[d] = (Kept)o[d];
                unsigned long long gates = 0;
                if (COND == SHELL_ENDPOINTS) {
                    const long rel = 64L * j + lag;
                    gates = m & shell_window(wd[rel >> 6], wd[(rel >> 6) + 1], (int)(rel & 63));
                    cnt += __popcll(gates);
                }
                for (unsigned long long mm = m; mm; mm &= mm - 1) {
                    const int i = __builtin_ctzll(mm);
                    bool gate;
                    if (COND == SHELL_CONTINUOUS) {
                        const int lf = __builtin_amdgcn_readfirstlane(left[64 * j + i]);
                        if (lf <= k0) continue;  // (the run ends below this pass's lags)
                        gate = lag < lf;
                        cnt += gate;
                    } else {
                        gate = (gates >> i) & 1ull;
                    }
                    Term::add(acc, gate, [&](int d) { return sm_from_lane(xo[d], i); },
                              [&](int d) { return (double)xs[d * n_x + 64 * j + i + tid]; });
                }
            }
        }
    }
    const size_t row = (size_t)blockIdx.x * ((size_t)gridDim.y * kSmLags) + (size_t)lag;
#pragma unroll
    for (int d = 0; d < NS; ++d) part_s[row * NS + d] = acc[d];
    part_n[row] = cnt;
}

}  // namespace ta
