// pair_lifetime.hip — the kernels of the pair population correlation functions (ion pairs, solvation contacts, hydrogen
// bonds): which pairs of items are ever bonded, their 0/1 indicator series as a pair-major block, and the histogram of the
// lengths of their runs of bonded frames.  pair_math.hpp has the arithmetic, which the CPU backend follows.
//
//   k_pair_find<D, PERIODIC>    the candidate search: k_vhd_pairs' walk (pair_tile_walk of pair_tile.hpp: a workgroup per (256
//                               a-items, 1024 b-items, searched frame), a lane owning 4 b-items in registers, the a-item read
//                               by scalar loads) over the frame-major scratch that k_vhd_gather writes at lag 0, with another
//                               visitor.  No histogram: a wave's 64 lanes hold 64 consecutive b-items, so its ballot of "bonded
//                               and a different item" IS the 64-bit word of the bitmap [pitch_a][pitch_b / 64]; one lane ORs it
//                               in, and only when it is non-zero.  OR is idempotent: the same bitmap from run to run and for
//                               every chunk.
//   k_pair_count, k_pair_list   the bitmap -> the list of (item a, item b) as int32, sorted by (a, b): popcounts per block
//                               of 1024 words, an exclusive scan of the block counts on the host, then every block expands
//                               its bits behind its offset (a wave scan and the waves' totals order the threads).
//   k_pair_series<E, D, BOX>    k_orient's shape in bond mode: workgroup (bx, g) covers frames [1024 bx, 1024 bx + 1024) of
//                               the pitch and the units g, g + G, ...; a unit is two candidate pairs = one whole destination
//                               pair of columns of a float64 block of P pseudo-atoms with D = 1, values 1.0 / 0.0, rows
//                               T ... pitch - 1 and the phantom column of an odd P zeros.  The atoms are read through PmAtom
//                               in the slab's own element type.  Every element has one writer.  All of that is series_body,
//                               which k_bond_series shares; the kernel's own part is its row, pair_indicator (one compare).
//   k_pair_runs                 a wave per destination pair at a time (two series): lane l reads frame 64 j + l, the ballot
//                               is the 64-frame word, a lane at a run's end finds the run's start with bit operations on the
//                               word and the carry of the run open since the words before.  Runs of up to kRunsSmall frames are
//                               counted in a register per lane and added once per wave (which walks several pairs); longer
//                               ones take one 64-bit integer atomic each.  Integer adds only: the same bits in any order.
//   k_pair_reduce               the blocks' rows added in block order (the lag sums rescaled to integers on the way).
// and of the bond lifetimes (bond_math.hpp: pairs or donor-hydrogen-acceptor triplets, a form and a break criterion):
//   k_bond_series<E, D, BOX, NAT>  series_body with bond_levels as its row: NAT atoms per row, the frame's LEVEL 0 / 1 / 2 as
//                               its value.  (Pair calls do not go through it with NAT = 2: the pair row keeps its one compare.)
//   k_pair_filter               the level block -> the 0/1 block in place, on k_pair_runs' walk: hysteresis (a fill of the
//                               level-2 bits through the runs of level >= 1, one carry bit across words) and the closing of
//                               absences of up to 63 frames (a window of three resolved words).  No atomics, no LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "bond_math.hpp"
#include "pair_tile.hpp"

namespace ta {
namespace {

// grid (a-tiles x b-tiles, the chunk's searched frames).  ga [n_o][D][pitch_a], gb [n_o][D][pitch_b]: the chunk's gathered
// frames; frame y of the chunk is frame (o_base + y) stride of the slab (its box with box_per_frame).  hm as k_vhd_pairs'.
// same: b is a, only q > p is kept (the lists increase strictly: idq > id).  bitmap: pitch_a rows of pitch_b / 64 words.
template <int D, bool PERIODIC>
__global__ void __launch_bounds__(kPmThreads)
    k_pair_find(const double* __restrict__ ga, const double* __restrict__ gb, const int* __restrict__ ida,
                const int* __restrict__ idb, long pitch_a, long pitch_b, int n_a, int n_tb, long stride, long o_base,
                const double* __restrict__ hm, int box_per_frame, double rc2, int same, unsigned long long* __restrict__ bitmap) {
    const long o = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const long words_b = pitch_b / 64;
    const long w0 = ((long)(blockIdx.x % n_tb) * VHD_TILE_B + (threadIdx.x - lane)) / 64;  // the wave's word of r = 0
    const PairTile tile = pair_tile_of(blockIdx.x, n_a, n_tb);
    pair_tile_walk<D, PERIODIC>(ga + (size_t)o * D * (size_t)pitch_a, gb + (size_t)o * D * (size_t)pitch_b, ida, idb, pitch_a, pitch_b, tile.p0,
                                tile.p1, tile.tile_b, hm + (box_per_frame ? (o_base + o) * stride * 6 : 0),
                                [&](int p, int r, int id, int idq, double r2) {  // ballot, one lane ORs a non-zero word
                                    const unsigned long long word = __ballot(r2 < rc2 && idq >= 0 && (same ? idq > id : idq != id));
                                    if (lane == 0 && word) atomicOr(&bitmap[(size_t)p * words_b + w0 + r * (kPmThreads / 64)], word);
                                });
}

constexpr int kPlWords = 4;                          // words per thread of the two list kernels
constexpr int kPlBlock = kPmThreads * kPlWords;      // words per workgroup

__device__ __forceinline__ unsigned pl_count(const unsigned long long* __restrict__ bitmap, long n_words, long w0) {
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < kPlWords; ++j)
        if (w0 + j < n_words) c += __popcll(bitmap[w0 + j]);
    return c;
}

__global__ void __launch_bounds__(kPmThreads)
    k_pair_count(const unsigned long long* __restrict__ bitmap, long n_words, unsigned* __restrict__ counts) {
    __shared__ unsigned wave_sum[kPmThreads / 64];
    unsigned c = pl_count(bitmap, n_words, ((long)blockIdx.x * kPmThreads + threadIdx.x) * kPlWords);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

// offs[block]: the pairs in front of the block's words.  Thread i takes words 4 i ... 4 i + 3 of the block, so the order of
// the threads is the order of the words, which is (a, b) order; pairs (n_pairs, 2) int32 gets the staged item ids
__global__ void __launch_bounds__(kPmThreads)
    k_pair_list(const unsigned long long* __restrict__ bitmap, long n_words, long words_b, const long long* __restrict__ offs,
                const int* __restrict__ ida, const int* __restrict__ idb, int* __restrict__ pairs) {
    __shared__ unsigned wave_sum[kPmThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long w0 = ((long)blockIdx.x * kPmThreads + threadIdx.x) * kPlWords;
    const unsigned c = pl_count(bitmap, n_words, w0);
    unsigned inc = c;  // the inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned v = __shfl_up(inc, d);
        if (lane >= d) inc += v;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    unsigned base = 0;
    for (int k = 0; k < wave; ++k) base += wave_sum[k];
    long long k = offs[blockIdx.x] + base + inc - c;
    for (int j = 0; j < kPlWords; ++j) {
        if (w0 + j >= n_words) break;
        unsigned long long m = bitmap[w0 + j];
        const long p = (w0 + j) / words_b, q0 = (w0 + j) % words_b * 64;
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            pairs[2 * k] = ida[p], pairs[2 * k + 1] = idb[q0 + b];
            ++k;
        }
    }
}

enum { BOX_NONE = 0, BOX_CONST = 1, BOX_FRAME = 2 };

// the boxes of the thread's frames: H[3] then M[3] of the staged columns per box (BOX_CONST: one, in slot 0; BOX_FRAME: one per
// frame, loaded ONCE per thread before the loop over units)
template <bool F32, int D, int BOX>
__device__ __forceinline__ void pair_boxes(const double* __restrict__ hm, long T, long tb, double (&H)[kPmFrames][3],
                                           double (&M)[kPmFrames][3]) {
    constexpr int F = kPmFrames;
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
        for (int d = 0; d < 3; ++d) H[f][d] = 1.0, M[f][d] = 1.0;
    if constexpr (BOX == BOX_CONST) {
#pragma unroll
        for (int d = 0; d < D; ++d) H[0][d] = hm[d], M[0][d] = hm[3 + d];
    }
    if constexpr (BOX == BOX_FRAME) {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const long t = pm_frame<F32>(tb, f);
            const double* box = hm + (t < T ? t : 0) * 6;  // (a frame >= T stores zeros: any box will do)
#pragma unroll
            for (int d = 0; d < D; ++d) H[f][d] = box[d], M[f][d] = box[3 + d];
        }
    }
}

// the indicator of pair `row` (its atoms at a workgroup-uniform address: scalar loads) in the thread's frames
template <class E, int D, int BOX>
__device__ __forceinline__ void pair_indicator(const E* __restrict__ x, long pitch, long T, long tb, const int* __restrict__ row,
                                               const double (&H)[kPmFrames][3], const double (&M)[kPmFrames][3], double rc2,
                                               double (&h)[kPmFrames]) {
    constexpr int F = kPmFrames;
    double a[F][3] = {}, b[F][3] = {};
    pm_load(PmAtom<E, D>(x, pitch, (unsigned)row[0]), T, tb, a);  // (atom D < 2^31: launch_pair_series)
    pm_load(PmAtom<E, D>(x, pitch, (unsigned)row[1]), T, tb, b);
#pragma unroll
    for (int f = 0; f < F; ++f) {
        constexpr bool kPeriodic = BOX != BOX_NONE;
        const int fb = BOX == BOX_FRAME ? f : 0;
        h[f] = pair_bonded<D, kPeriodic>(a[f], b[f], H[fb], M[fb], rc2) ? 1.0 : 0.0;
    }
}

// The body of both series kernels.  grid pm_unit_grid(units = ceil(P / 2)).  rows (P, NAT) int32 atoms of the slab; hm: per box
// H[3] then M[3] of the staged columns (BOX_CONST: one; BOX_FRAME: one per frame, loaded ONCE per thread before the loop over
// units).  Z: ceil(P / 2) destination pairs of `pitch` rows.  row(atoms, tb, H, M, v): the values of one row in the thread's
// frames; the second row's atoms are loaded after the first row's values are formed (three float64 atoms of D = 3 are 72
// registers).
template <class E, int D, int BOX, class Row>
__device__ __forceinline__ void series_body(long pitch, long T, int P, const int* __restrict__ rows, int NAT, const double* __restrict__ hm,
                                            double* __restrict__ Z, Row&& row) {
    constexpr bool kF32 = std::is_same_v<E, float>;
    constexpr int F = kPmFrames;
    const long tb = (long)blockIdx.x * (kPmThreads * F);
    double H[F][3], M[F][3];
    pair_boxes<kF32, D, BOX>(hm, T, tb, H, M);
    double2* Zp = reinterpret_cast<double2*>(Z);
    const int n_units = (P + 1) / 2;
    for (int g = blockIdx.y; g < n_units; g += gridDim.y) {
        double v0[F], v1[F] = {};
        row(rows + 2L * NAT * g, tb, H, M, v0);
        if (2 * g + 1 < P) row(rows + 2L * NAT * g + NAT, tb, H, M, v1);  // (workgroup-uniform)
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const long t = pm_frame<kF32>(tb, f);
            if (t >= pitch) continue;
            const double v[2] = {v0[f], v1[f]};
            pm_store_row<1>(Zp + (long)g * pitch, pitch, t, t < T, 1, v);
        }
    }
}

// series_body with pair_indicator as its row: the 0/1 indicator of the pairs (P, 2), one compare per frame
template <class E, int D, int BOX>
__global__ void __launch_bounds__(kPmThreads)
    k_pair_series(const E* __restrict__ x, long pitch, long T, int P, const int* __restrict__ pairs, const double* __restrict__ hm,
                  double rc2, double* __restrict__ Z) {
    series_body<E, D, BOX>(pitch, T, P, pairs, 2, hm, Z, [&](const int* row, long tb, const auto& H, const auto& M, double (&h)[kPmFrames]) {
        pair_indicator<E, D, BOX>(x, pitch, T, tb, row, H, M, rc2, h);
    });
}

// the level of bond `row` (NAT atoms at a workgroup-uniform address) in the thread's frames: 0.0, 1.0, or `two` for level 2
template <class E, int D, int BOX, int NAT>
__device__ __forceinline__ void bond_levels(const E* __restrict__ x, long pitch, long T, long tb, const int* __restrict__ row,
                                            const double (&H)[kPmFrames][3], const double (&M)[kPmFrames][3], const BondCuts& k,
                                            double two, double (&s)[kPmFrames]) {
    constexpr int F = kPmFrames;
    double at[NAT][F][3] = {};
#pragma unroll
    for (int i = 0; i < NAT; ++i) pm_load(PmAtom<E, D>(x, pitch, (unsigned)row[i]), T, tb, at[i]);  // (atom D < 2^31: the launcher)
#pragma unroll
    for (int f = 0; f < F; ++f) {
        constexpr bool kPeriodic = BOX != BOX_NONE;
        const int fb = BOX == BOX_FRAME ? f : 0;
        double xs[NAT][3];
#pragma unroll
        for (int i = 0; i < NAT; ++i)
#pragma unroll
            for (int d = 0; d < 3; ++d) xs[i][d] = at[i][f][d];
        const int level = bond_level<D, kPeriodic, NAT>(xs, H[fb], M[fb], k);
        s[f] = level == 2 ? two : level == 1 ? 1.0 : 0.0;
    }
}

// series_body with bond_levels as its row, for bonds of NAT items and two levels (bond_math.hpp): atoms (P, NAT) int32; Z gets
// the LEVEL 0.0 / 1.0 / two per frame, two = 2.0 in front of k_pair_filter and 1.0 where no filter follows (the break criterion
// is then the form criterion, level 1 does not occur and the level-2 frames are the series).
template <class E, int D, int BOX, int NAT>
__global__ void __launch_bounds__(kPmThreads)
    k_bond_series(const E* __restrict__ x, long pitch, long T, int P, const int* __restrict__ atoms, const double* __restrict__ hm,
                  BondCuts k, double two, double* __restrict__ Z) {
    series_body<E, D, BOX>(pitch, T, P, atoms, NAT, hm, Z, [&](const int* row, long tb, const auto& H, const auto& M, double (&s)[kPmFrames]) {
        bond_levels<E, D, BOX, NAT>(x, pitch, T, tb, row, H, M, k, two, s);
    });
}

// one series' filter state: the hysteresis carry and the h words before and at the word that is closed next
struct FilterState {
    bool carry = false;
    unsigned long long prev = 0, cur = 0;
};
// the word behind `cur` has been resolved to `next`: lane's frame of `cur` after closing, the window moved on
__device__ __forceinline__ bool filter_step(FilterState& f, unsigned long long next, int lane, int gap) {
    const bool on = ((f.cur >> lane) & 1ull) || (gap && bond_close_bit(f.prev, f.cur, next, lane, gap));
    f.prev = f.cur, f.cur = next;
    return on;
}

// Z: the LEVEL block k_bond_series wrote with two = 2.0 (n_units destination pairs of `pitch` rows) becomes the 0/1 block of
// g(t) in place: hysteresis, then closing of absences of up to `gap` frames.  A wave per destination pair at a time, as
// k_pair_runs: lane l reads frame 64 j + l, the ballots of v == 2 and v >= 1 are the words S and W, bond_hyst_word resolves
// word j with the wave-uniform carry, and word j - 1 is closed against words j - 2 and j and written back, one frame per
// lane.  Every trip count depends on T alone.  Rows >= T and the phantom column stay as they are: zeros.
__global__ void __launch_bounds__(kPmThreads)
    k_pair_filter(double* __restrict__ Z, long pitch, long T, long n_units, int gap) {
    const int lane = threadIdx.x & 63;
    const long n_waves = (long)gridDim.x * (kPmThreads / 64), n_words = (T + 63) / 64;
    for (long g = (long)blockIdx.x * (kPmThreads / 64) + (threadIdx.x >> 6); g < n_units; g += n_waves) {  // (a whole wave)
        double2* z = reinterpret_cast<double2*>(Z) + g * pitch;
        FilterState f0, f1;
        for (long j = 0; j <= n_words; ++j) {  // (trip n_words: word n_words is the zeros behind the series)
            const long t = j * 64 + lane;
            double2 v = {0.0, 0.0};
            if (t < T) v = z[t];
            const unsigned long long h0 = bond_hyst_word(__ballot(v.x == 2.0), __ballot(v.x >= 1.0), f0.carry);
            const unsigned long long h1 = bond_hyst_word(__ballot(v.y == 2.0), __ballot(v.y >= 1.0), f1.carry);
            f0.carry = h0 >> 63, f1.carry = h1 >> 63;
            const bool on0 = filter_step(f0, h0, lane, gap), on1 = filter_step(f1, h1, lane, gap);
            if (j > 0 && t - 64 < T) z[t - 64] = double2{on0 ? 1.0 : 0.0, on1 ? 1.0 : 0.0};
        }
    }
}

constexpr int kRunsSmall = 8;  // run lengths counted in registers (lane k - 1 counts length k)

// a run of the wave-uniform length len: lane len - 1's register, or one atomic for a long one
__device__ __forceinline__ void runs_count(long long len, int lane, unsigned& small, unsigned long long* __restrict__ runs) {
    if (len <= kRunsSmall) small += lane == len - 1;
    else if (lane == 0) atomicAdd(&runs[len], 1ull);
}

// one 64-frame word m of one series: its run ends counted, the carry moved on
__device__ __forceinline__ void runs_word(unsigned long long m, int lane, long long& carry, unsigned& small,
                                          unsigned long long* __restrict__ runs) {
    if (carry && !(m & 1ull)) runs_count(carry, lane, small, runs);  // the run that ended with the word before
    const bool end = lane < 63 && ((m >> lane) & 1ull) && !((m >> (lane + 1)) & 1ull);
    const long long len = end ? pair_runs_word(m, lane, carry) : 0;
#pragma unroll
    for (int k = 1; k <= kRunsSmall; ++k) {
        const unsigned long long b = __ballot(end && len == k);
        if (lane == k - 1) small += __popcll(b);
    }
    if (end && len > kRunsSmall) atomicAdd(&runs[len], 1ull);
    carry = pair_runs_carry(m, carry);
}

// Z: the indicator block (n_units destination pairs of `pitch` rows, rows >= T zeros, an odd P's phantom column zeros: it
// has no runs).  runs[l], l = 1 ... T (T + 1 entries) gets the counts added.  A wave takes the destination pairs w, w + W, ...
// (W the waves of the grid) and keeps its short-run counters across them: kRunsSmall atomics per wave, not per pair.
__global__ void __launch_bounds__(kPmThreads)
    k_pair_runs(const double* __restrict__ Z, long pitch, long T, long n_units, unsigned long long* __restrict__ runs) {
    const int lane = threadIdx.x & 63;
    const long n_waves = (long)gridDim.x * (kPmThreads / 64);
    unsigned small = 0;
    for (long g = (long)blockIdx.x * (kPmThreads / 64) + (threadIdx.x >> 6); g < n_units; g += n_waves) {  // (a whole wave)
        const double2* z = reinterpret_cast<const double2*>(Z) + g * pitch;
        long long carry0 = 0, carry1 = 0;
        for (long j = 0; j * 64 < T; ++j) {
            const long t = j * 64 + lane;
            double2 v = {0.0, 0.0};
            if (t < T) v = z[t];
            const unsigned long long m0 = __ballot(v.x != 0.0), m1 = __ballot(v.y != 0.0);
            runs_word(m0, lane, carry0, small, runs);
            runs_word(m1, lane, carry1, small, runs);
        }
        // the run open at frame T - 1 ends there (T a multiple of 64: otherwise it ended inside the last word)
        if (carry0) runs_count(carry0, lane, small, runs);
        if (carry1) runs_count(carry1, lane, small, runs);
    }
    if (lane < kRunsSmall && small) atomicAdd(&runs[lane + 1], (unsigned long long)small);
}

// out[i] = sum_r f(rows[r][i]) in row order, i < n.  PAIR_SUM: f = identity; PAIR_LAGS: f(v) = v (T - i), the library's lag
// sums carry 1 / (T - i); PAIR_LAGS_INT: rint of that (a sum of products of 0/1 values is an integer)
__global__ void __launch_bounds__(kPmThreads)
    k_pair_reduce(const double* __restrict__ rows, int n_rows, long n, long T, int mode, double* __restrict__ out) {
    const long i = (long)blockIdx.x * kPmThreads + threadIdx.x;
    if (i >= n) return;
    const double scale = mode == PAIR_SUM ? 1.0 : (double)(T - i);
    double acc = 0.0;
    for (int r = 0; r < n_rows; ++r) {
        const double v = rows[(size_t)r * n + i] * scale;
        acc += mode == PAIR_LAGS_INT ? rint(v) : v;
    }
    out[i] = acc;
}

}  // namespace

hipError_t launch_pair_find(const double* ga, const double* gb, const int* ida, const int* idb, long pitch_a, long pitch_b, long n_a,
                            long n_b, int D, long T, long stride, long o_base, int n_o, const double* hm, bool box_per_frame,
                            double rc2, bool same, unsigned long long* bitmap, hipStream_t st) {
    const long n_ta = (n_a + VHD_TILE_A - 1) / VHD_TILE_A, n_tb = (n_b + VHD_TILE_B - 1) / VHD_TILE_B;
    if (!pair_tile_ok(pitch_a, pitch_b, n_a, n_b, D, T, stride, n_o) || o_base < 0 || (o_base + n_o - 1) * stride >= T || !(rc2 > 0.0) || !bitmap)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(n_ta * n_tb), (unsigned)n_o);
    auto launch = [&](auto periodic) {
        pm_switch<1, 3>(D, [&](auto d) {
            hipLaunchKernelGGL((k_pair_find<decltype(d)::value, decltype(periodic)::value>), grid, dim3(kPmThreads), 0, st, ga, gb, ida, idb,
                               pitch_a, pitch_b, (int)n_a, (int)n_tb, stride, o_base, hm, hm && box_per_frame ? 1 : 0, rc2, same ? 1 : 0,
                               bitmap);
        });
    };
    if (hm) launch(std::true_type{});
    else launch(std::false_type{});
    return hipGetLastError();
}

long pair_list_blocks(long n_words) { return (n_words + kPlBlock - 1) / kPlBlock; }

hipError_t launch_pair_count(const unsigned long long* bitmap, long n_words, unsigned* counts, hipStream_t st) {
    if (n_words < 1 || pair_list_blocks(n_words) >= (1L << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pair_count, dim3((unsigned)pair_list_blocks(n_words)), dim3(kPmThreads), 0, st, bitmap, n_words, counts);
    return hipGetLastError();
}

hipError_t launch_pair_list(const unsigned long long* bitmap, long n_words, long words_b, const long long* offs, const int* ida,
                            const int* idb, int* pairs, hipStream_t st) {
    if (n_words < 1 || words_b < 1 || n_words % words_b || pair_list_blocks(n_words) >= (1L << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pair_list, dim3((unsigned)pair_list_blocks(n_words)), dim3(kPmThreads), 0, st, bitmap, n_words, words_b, offs,
                       ida, idb, pairs);
    return hipGetLastError();
}

// what both series launchers check and switch on: launch(grid, E(), D, BOX) is the one launch line (ok: the caller's own checks)
template <class Launch>
static hipError_t launch_series(int n_cu, bool f32, long pitch, long T, long n_atoms, int D, long n_rows, const int* rows, const double* hm,
                                bool box_per_frame, const double* Z, bool ok, Launch&& launch) {
    if (!pm_slab_ok(pitch, T, n_atoms, D) || n_rows < 1 || n_rows >= (1L << 30) || !rows || !ok || !Z) return hipErrorInvalidValue;
    const dim3 grid = pm_unit_grid(n_cu, pitch, (n_rows + 1) / 2);
    const int box = !hm ? BOX_NONE : box_per_frame ? BOX_FRAME : BOX_CONST;
    pm_dispatch(f32, D, [&](auto e, auto d) { pm_switch<BOX_NONE, BOX_FRAME>(box, [&](auto b) { launch(grid, e, d, b); }); });
    return hipGetLastError();
}

hipError_t launch_pair_series(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, long n_pairs,
                              const int* pairs, const double* hm, bool box_per_frame, double rc2, double* Z, hipStream_t st) {
    return launch_series(n_cu, f32, pitch, T, n_atoms, D, n_pairs, pairs, hm, box_per_frame, Z, rc2 > 0.0, [&](dim3 grid, auto e, auto d, auto b) {
        using E = decltype(e);
        hipLaunchKernelGGL((k_pair_series<E, d(), b()>), grid, dim3(kPmThreads), 0, st, (const E*)x, pitch, T, (int)n_pairs, pairs, hm, rc2, Z);
    });
}

hipError_t launch_bond_series(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, long n_bonds, int n_at,
                              const int* atoms, const double* hm, bool box_per_frame, const BondCuts& k, double two, double* Z,
                              hipStream_t st) {
    const bool ok = (n_at == 2 || n_at == 3) && k.rc2 > 0.0 && k.rb2 >= k.rc2 && k.cb2 <= k.c2 && (two == 1.0 || two == 2.0);
    return launch_series(n_cu, f32, pitch, T, n_atoms, D, n_bonds, atoms, hm, box_per_frame, Z, ok, [&](dim3 grid, auto e, auto d, auto b) {
        pm_switch<2, 3>(n_at, [&](auto nat) {
            using E = decltype(e);
            hipLaunchKernelGGL((k_bond_series<E, d(), b(), nat()>), grid, dim3(kPmThreads), 0, st, (const E*)x, pitch, T, (int)n_bonds, atoms,
                               hm, k, two, Z);
        });
    });
}

// the grid of the two kernels that walk a block a wave per destination pair: eight workgroups per CU, at most one wave per pair
static long pair_walk_grid(int n_cu, long n_units) {
    return std::min<long>(8L * std::max(n_cu, 1), (n_units + kPmThreads / 64 - 1) / (kPmThreads / 64));
}

hipError_t launch_pair_filter(int n_cu, double* Z, long pitch, long T, long n_pairs, int gap, hipStream_t st) {
    const long n_units = (n_pairs + 1) / 2;
    if (n_pairs < 1 || T < 1 || T > pitch || gap < 0 || gap > 63 || !Z) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pair_filter, dim3((unsigned)pair_walk_grid(n_cu, n_units)), dim3(kPmThreads), 0, st, Z, pitch, T, n_units, gap);
    return hipGetLastError();
}

hipError_t launch_pair_runs(int n_cu, const double* Z, long pitch, long T, long n_pairs, unsigned long long* runs, hipStream_t st) {
    // eight workgroups per CU (22 VGPRs: eight waves per SIMD), at most one wave per destination pair
    const long n_units = (n_pairs + 1) / 2, n_wg = pair_walk_grid(n_cu, n_units);
    if (n_pairs < 1 || T < 1 || T > pitch || !Z || !runs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pair_runs, dim3((unsigned)n_wg), dim3(kPmThreads), 0, st, Z, pitch, T, n_units, runs);
    return hipGetLastError();
}

hipError_t launch_pair_reduce(const double* rows, int n_rows, long n, long T, int mode, double* out, hipStream_t st) {
    if (n_rows < 1 || n < 1 || (mode != PAIR_SUM && n > T) || mode < PAIR_SUM || mode > PAIR_LAGS_INT) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pair_reduce, dim3((unsigned)((n + kPmThreads - 1) / kPmThreads)), dim3(kPmThreads), 0, st, rows, n_rows, n, T,
                       mode, out);
    return hipGetLastError();
}

}  // namespace ta
