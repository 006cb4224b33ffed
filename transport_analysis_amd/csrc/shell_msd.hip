// shell_msd.hip — the kernels of the shell-resolved MSD (include/ta_hip.h, ta_shell_msd): the squared displacements of the
// observed items over the lags 0 ... L, every term gated by bits of ta_shell_residence's 0/1 series g (the block Z behind
// k_pair_filter).  shell_msd_math.hpp has the arithmetic, which the CPU backend follows.
//
//   k_shell_bits                a wave per destination pair of Z at a time, as k_pair_runs: lane l reads frame 64 j + l, the
//                               ballots are the two items' 64-frame words of g, stored packed (ceil(T / 64) words per item):
//                               Z is read ONCE, everything behind works on 1 / 64 of its bytes.
//   k_shell_msd<E, D, COND>     grid (G, passes).  Workgroup (x, y) owns the 256 lags [256 y, 256 y + 256), one per thread, and
//                               the items x, x + G, ... of the block, one at a time, in chunks of C origin frames (C a
//                               multiple of 64).  Per (item, chunk): the words of the chunk and of the lagged frames behind it
//                               go to LDS; a chunk without a frame inside is left at once (a workgroup-uniform branch: with
//                               sparse residence most of the work); the item's D columns of the frames [c0 + 256 y,
//                               c0 + 256 y + C + 256) are read through PmAtom in the slab's own element type and kept in LDS
//                               in that type; "continuous": wave 0 walks the words from the last down and leaves left(s), the
//                               frames from s on to the first frame outside.  Then per 64-frame word of origins (skipped
//                               where zero): lane i of every wave reads origin 64 j + i's columns from the slab, and per SET
//                               bit i of the word (a scalar loop, its trip count the same for every lane) the origin comes
//                               out of lane i by v_readlane, the lagged frame out of LDS (consecutive lanes, consecutive
//                               addresses), widened, and fma(d, d, acc) runs under the gate: "continuous" lag < left(s), with
//                               origins whose run ends below the pass's first lag skipped for the whole workgroup;
//                               "endpoints" bit i of the thread's window of g at its lag, whose popcount against the
//                               origins' word is that lag's count.  A thread's D sums and its count stay in registers over
//                               all items of the workgroup and are stored once: the partial rows [G][256 passes].
//   k_shell_fold                the G partial rows added in row order (the counts as integers), into the outputs (the first
//                               block of observed items) or onto them (the blocks behind it: block order).
// No atomics, no float adds whose order depends on timing: repeat runs give the same bits.  Every loop's trip count depends on
// the shapes or on workgroup-uniform words of g alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "pm_read.hpp"
#include "shell_msd_math.hpp"

namespace ta {
namespace {

constexpr int kSmLags = kPmThreads;  // lags per pass: one per thread

// Z: the 0/1 block (n_units destination pairs of `pitch` rows).  words: n_items rows of nw = ceil(T / 64) words.
__global__ void __launch_bounds__(kPmThreads)
    k_shell_bits(const double* __restrict__ Z, long pitch, long T, long n_items, long nw, unsigned long long* __restrict__ words) {
    const int lane = threadIdx.x & 63;
    const long n_waves = (long)gridDim.x * (kPmThreads / 64), n_units = (n_items + 1) / 2;
    for (long g = (long)blockIdx.x * (kPmThreads / 64) + (threadIdx.x >> 6); g < n_units; g += n_waves) {  // (a whole wave)
        const double2* z = reinterpret_cast<const double2*>(Z) + g * pitch;
        for (long j = 0; j < nw; ++j) {
            const long t = j * 64 + lane;
            double2 v = {0.0, 0.0};
            if (t < T) v = z[t];
            const unsigned long long m0 = __ballot(v.x != 0.0), m1 = __ballot(v.y != 0.0);
            if (lane == 0) {
                words[2 * g * nw + j] = m0;
                if (2 * g + 1 < n_items) words[(2 * g + 1) * nw + j] = m1;
            }
        }
    }
}

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

// x: the staged slab; ids: the block's observed items (atoms of the slab); words: k_shell_bits' rows; C: origins per chunk;
// part_s [G][256 passes][D], part_n [G][256 passes].  Dynamic LDS: (C + 256 y_max + 256) / 64 words | C ints | D (C + 256) E.
template <class E, int D, int COND>
__global__ void __launch_bounds__(kPmThreads)
    k_shell_msd(const E* __restrict__ x, long pitch, long T, const int* __restrict__ ids, long n_items,
                const unsigned long long* __restrict__ words, long nw, int C, double* __restrict__ part_s,
                unsigned long long* __restrict__ part_n) {
    extern __shared__ unsigned long long sm_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const long k0 = (long)blockIdx.y * kSmLags, lag = k0 + tid;
    const int n_ww = (int)((C + k0) / 64) + 4, n_ow = C / 64, n_x = C + kSmLags;
    unsigned long long* wd = sm_lds;                                                      // n_ww words from frame c0 on
    int* left = reinterpret_cast<int*>(sm_lds + ((C + (long)(gridDim.y - 1) * kSmLags) / 64 + 4));  // C
    E* xs = reinterpret_cast<E*>(left + C);                                               // [D][n_x] from frame c0 + k0 on
    double acc[D] = {};
    unsigned long long cnt = 0;
    for (long q = blockIdx.x; q < n_items; q += gridDim.x) {
        const unsigned long long* wq = words + q * nw;
        const PmAtom<E, D> atom(x, pitch, (unsigned)ids[q]);
        for (long c0 = 0; c0 + k0 < T; c0 += C) {
            __syncthreads();  // (the chunk before has been read)
            if (tid < n_ww) wd[tid] = c0 / 64 + tid < nw ? wq[c0 / 64 + tid] : 0ull;
            __syncthreads();
            unsigned long long any = 0;
            for (int j = 0; j < n_ow; ++j) any |= wd[j];
            if (!sm_uniform(any)) continue;  // (the same words for every thread)
            for (int i = tid; i < n_x; i += kPmThreads) {
                const long t = c0 + k0 + i;
                double v[3];
                atom.row(t < T ? t : 0, v);
#pragma unroll
                for (int d = 0; d < D; ++d) xs[d * n_x + i] = (E)v[d];
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
                double o[3];
                atom.row(s < T ? s : 0, o);
                E xo[D];
#pragma unroll
                for (int d = 0; d < D; ++d) xo[d] = (E)o[d];
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
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        const double a = sm_from_lane(xo[d], i), b = (double)xs[d * n_x + 64 * j + i + tid];
                        if (gate) acc[d] = shell_msd_add(acc[d], a, b);
                    }
                }
            }
        }
    }
    const size_t row = (size_t)blockIdx.x * ((size_t)gridDim.y * kSmLags) + (size_t)lag;
#pragma unroll
    for (int d = 0; d < D; ++d) part_s[row * D + d] = acc[d];
    part_n[row] = cnt;
}

// sums (L + 1, D), count (L + 1): the G partial rows (Lp lags each) added in row order; first: stored, otherwise added on
__global__ void __launch_bounds__(kPmThreads)
    k_shell_fold(const double* __restrict__ part_s, const unsigned long long* __restrict__ part_n, int G, long Lp, long n_lags, int D,
                 int first, double* __restrict__ sums, long long* __restrict__ count) {
    const long i = (long)blockIdx.x * kPmThreads + threadIdx.x;
    if (sums && i < n_lags * D) {
        double acc = 0.0;
        for (int g = 0; g < G; ++g) acc += part_s[(size_t)g * Lp * D + i];
        sums[i] = first ? acc : sums[i] + acc;
    }
    if (count && i < n_lags) {
        unsigned long long acc = 0;
        for (int g = 0; g < G; ++g) acc += part_n[(size_t)g * Lp + i];
        count[i] = (first ? 0 : count[i]) + (long long)acc;
    }
}

size_t sm_lds_bytes(int C, int n_pass, int D, bool f32) {
    return 8 * (size_t)((C + (n_pass - 1) * kSmLags) / 64 + 4) + 4 * (size_t)C + (size_t)D * (C + kSmLags) * (f32 ? 4 : 8);
}

}  // namespace

int shell_msd_chunk(long option) {
    if (option <= 0) return 512;
    return (int)std::min<long>(1024, (option + 63) / 64 * 64);
}

int shell_msd_groups(int n_cu, long n_items, long max_lag) {
    const long n_pass = max_lag / kSmLags + 1;
    return (int)std::max<long>(1, std::min<long>(n_items, (8L * std::max(n_cu, 1) + n_pass - 1) / n_pass));
}

size_t shell_msd_part_bytes(int G, long max_lag, int D) { return sizeof(double) * (size_t)G * (size_t)((max_lag / kSmLags + 1) * kSmLags) * (D + 1); }

hipError_t launch_shell_bits(int n_cu, const double* Z, long pitch, long T, long n_items, unsigned long long* words, hipStream_t st) {
    const long n_units = (n_items + 1) / 2;
    if (n_items < 1 || T < 1 || T > pitch || !Z || !words) return hipErrorInvalidValue;
    const long n_wg = std::min<long>(8L * std::max(n_cu, 1), (n_units + kPmThreads / 64 - 1) / (kPmThreads / 64));
    hipLaunchKernelGGL(k_shell_bits, dim3((unsigned)n_wg), dim3(kPmThreads), 0, st, Z, pitch, T, n_items, (T + 63) / 64, words);
    return hipGetLastError();
}

hipError_t launch_shell_msd(const void* x, bool f32, long pitch, long T, long n_atoms, int D, const int* ids, long n_items,
                            const unsigned long long* words, int condition, long max_lag, int chunk, int G, void* part,
                            hipStream_t st) {
    const long n_pass = max_lag / kSmLags + 1;
    if (!pm_slab_ok(pitch, T, n_atoms, D) || n_items < 1 || n_items >= (1L << 30) || max_lag < 0 || max_lag > kShellMsdMaxLag || max_lag >= T ||
        chunk < 64 || chunk > 1024 || chunk % 64 || G < 1 || G > n_items || (condition != SHELL_CONTINUOUS && condition != SHELL_ENDPOINTS) ||
        !x || !ids || !words || !part)
        return hipErrorInvalidValue;
    const size_t lds = sm_lds_bytes(chunk, (int)n_pass, D, f32);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    double* part_s = (double*)part;
    unsigned long long* part_n = (unsigned long long*)(part_s + (size_t)G * (size_t)(n_pass * kSmLags) * D);
    pm_dispatch(f32, D, [&](auto e, auto d) {
        pm_switch<SHELL_CONTINUOUS, SHELL_ENDPOINTS>(condition, [&](auto c) {
            using E = decltype(e);
            hipLaunchKernelGGL((k_shell_msd<E, d(), c()>), dim3((unsigned)G, (unsigned)n_pass), dim3(kPmThreads), lds, st, (const E*)x, pitch, T,
                               ids, n_items, words, (T + 63) / 64, chunk, part_s, part_n);
        });
    });
    return hipGetLastError();
}

hipError_t launch_shell_fold(const void* part, int G, long max_lag, int D, bool first, double* sums, long long* count, hipStream_t st) {
    const long n_lags = max_lag + 1, Lp = (max_lag / kSmLags + 1) * kSmLags;
    if (G < 1 || max_lag < 0 || D < 1 || D > 3 || !part || (!sums && !count)) return hipErrorInvalidValue;
    const double* part_s = (const double*)part;
    hipLaunchKernelGGL(k_shell_fold, dim3((unsigned)((n_lags * D + kPmThreads - 1) / kPmThreads)), dim3(kPmThreads), 0, st, part_s,
                       (const unsigned long long*)(part_s + (size_t)G * (size_t)Lp * D), G, Lp, n_lags, D, first ? 1 : 0, sums, count);
    return hipGetLastError();
}

}  // namespace ta
