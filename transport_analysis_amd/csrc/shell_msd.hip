// shell_msd.hip — the kernels of the shell-resolved MSD (include/ta_hip.h, ta_shell_msd): the squared displacements of the
// observed items over the lags 0 ... L, every term gated by bits of ta_shell_residence's 0/1 series g (the block Z behind
// k_pair_filter).  shell_msd_math.hpp has the arithmetic, which the CPU backend follows.
//
//   k_shell_bits                a wave per destination pair of Z at a time, as k_pair_runs: lane l reads frame 64 j + l, the
//                               ballots are the two items' 64-frame words of g, stored packed (ceil(T / 64) words per item):
//                               Z is read ONCE, everything behind works on 1 / 64 of its bytes.
//   k_shell_msd<E, D, COND>     shell_gate_walk (shell_gate.hpp: the chunks, the words in LDS, the two gates, the partial rows)
//                               with the item's D columns as its Source, read through PmAtom in the slab's own element type
//                               and kept in LDS in that type, and fma(d, d, acc) per axis as its Term.  k_shell_orient
//                               (shell_orient.hip) is the walk's other instantiation.
//   k_shell_fold                the G partial rows added in row order (the counts as integers), into the outputs (the first
//                               block of observed items) or onto them (the blocks behind it: block order).
// No atomics, no float adds whose order depends on timing: repeat runs give the same bits.  Every loop's trip count depends on
// the shapes or on workgroup-uniform words of g alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "pm_read.hpp"
#include "shell_gate.hpp"
#include "shell_msd_math.hpp"

namespace ta {
namespace {

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

// The walk's Source of the MSD: the item's D columns, read through PmAtom::row and kept in the slab's own element type
template <class E, int D>
struct ShellMsdSource {
    static constexpr int NV = D;
    using Kept = E;
    PmAtom<E, D> atom;
    __device__ __forceinline__ void load(long t, double (&v)[D]) const {
        double r[3];
        atom.row(t, r);
#pragma unroll
        for (int d = 0; d < D; ++d) v[d] = r[d];
    }
};
// ... and its Term: shell_msd_add per axis
template <int D>
struct ShellMsdTerm {
    static constexpr int NS = D;
    template <class A, class B>
    static __device__ __forceinline__ void add(double (&acc)[D], bool gate, A&& origin, B&& lagged) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double a = origin(d), b = lagged(d);
            if (gate) acc[d] = shell_msd_add(acc[d], a, b);
        }
    }
};

// x: the staged slab; ids: the block's observed items (atoms of the slab); the rest as shell_gate_walk's (shell_gate.hpp)
template <class E, int D, int COND>
__global__ void __launch_bounds__(kPmThreads)
    k_shell_msd(const E* __restrict__ x, long pitch, long T, const int* __restrict__ ids, long n_items,
                const unsigned long long* __restrict__ words, long nw, int C, double* __restrict__ part_s,
                unsigned long long* __restrict__ part_n) {
    shell_gate_walk<COND, ShellMsdTerm<D>>(T, n_items, words, nw, C, part_s, part_n, [&](long q) {
        return ShellMsdSource<E, D>{PmAtom<E, D>(x, pitch, (unsigned)ids[q])};
    });
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
    const size_t lds = shell_gate_lds_bytes(chunk, (int)n_pass, D, f32 ? 4 : 8);
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
