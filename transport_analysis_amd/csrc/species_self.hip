// species_self.hip — the weighted slab of a staged slab with each species' atoms contiguous (the per-species SELF terms of
// the Onsager analyses: sum_{n in s} w_n^2 MSD_n, sum_{n in s} w_n^2 VACF_n).
//
//   W[t, D r(n) + d + base(s_n)] = w_n (x[t, D n + d] - shift x[0, D n + d])
//
// s_n the label of atom n, r(n) its stable rank among its species' atoms, base(s) the first column of species s's block.
// Every block starts on a column-pair boundary, so it is a pair-major slab of its own with N_s atoms: the lag-sum
// evaluations of api.hip run on it unchanged, once per species (lag sums are linear in atoms).  A block with an odd
// N_s D ends in a phantom column of zeros, and rows T ... pitch - 1 of every pair are written as zeros: the scratch is
// reused between calls.  No atomics, every destination element has one writer: the same bits from run to run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "ta_internal.hpp"

namespace ta {
namespace {

constexpr int kSortThreads = 256, kSortFrames = 4;  // a workgroup covers 1024 consecutive frames, a thread four of them

// Column c + j of an atom (c its first column, odd = c & 1) is element j + odd of the source pairs (ax, ay), (bx, by) that
// cover it; the selects work on loaded VALUES with constant destinations (a select between two array elements comes back
// from the compiler as a runtime index, and the array then lives in scratch or LDS)
template <int D, class V>
__device__ __forceinline__ void sort_pick(V ax, V ay, V bx, V by, bool odd, double (&out)[3]) {
    if constexpr (D == 2) {
        out[0] = (double)ax, out[1] = (double)ay;  // (an atom's first column is even)
    } else {
        out[0] = (double)(odd ? ay : ax);
        if constexpr (D == 3) out[1] = (double)(odd ? bx : ay), out[2] = (double)(odd ? by : bx);
    }
}

// A work unit is two consecutive atoms (2 u, 2 u + 1) of one species in sorted order: 2 D columns = D WHOLE destination
// pairs, so every store is a full 16-byte row and a wave's stores of one pair are contiguous along time.  The last
// unit of a species with an odd count holds one atom: ceil(D / 2) pairs, the phantom column (odd D) written as 0 --
// nothing of the next species' block is touched.  Each source atom is read as the whole source pairs that cover its D
// columns (one pair for D = 1, 2, two for D = 3), 16-byte loads along time; the half that belongs to a neighbouring
// atom is that atom's unit's own load a moment earlier or later (cache).
//   float64 slab: a load = row t of a pair; the thread's frames are tb + tid + 256 i, i < 4
//   float32 slab: a load = rows 2 q, 2 q + 1 of a pair (8-byte rows), widened in registers; q = tb / 2 + tid + 256 i, i < 2
// Workgroup (bx, g): frames [1024 bx, 1024 bx + 1024) of the pitch (every row < pitch is written, those >= T as zeros; a
// load that would start at or past row T reads row 0 instead), units g, g + G, ... (G = gridDim.y).  Which unit, its
// species, atoms, weights and column parity depend on blockIdx and the loop counter only: scalar registers.
template <class E, int D>
__global__ void __launch_bounds__(kSortThreads)
    k_species_sort(const E* __restrict__ x, long pitch, long T, SortPlan plan, const int* __restrict__ order,
                   const double* __restrict__ w, int shift, double* __restrict__ W) {
    constexpr bool kF32 = std::is_same_v<E, float>;
    constexpr int NP = D == 3 ? 2 : 1;  // source pairs per atom
    constexpr int F = kSortFrames;
    const long tb = (long)blockIdx.x * (kSortThreads * F);
    auto frame = [&](int f) -> long {
        if constexpr (kF32) return 2 * (tb / 2 + threadIdx.x + kSortThreads * (f / 2)) + f % 2;
        else return tb + threadIdx.x + kSortThreads * f;
    };
    for (int unit = blockIdx.y; unit < plan.n_units; unit += gridDim.y) {
        // the unit's species: the last one whose first unit is not past it (constant indices: the plan stays in SGPRs)
        int u0 = 0, pos0 = 0, cnt = plan.count[0];
        long dp0 = 0;
#pragma unroll
        for (int s = 1; s < TA_ONSAGER_MAX_SPECIES; ++s)
            if (s < plan.n_species && unit >= plan.unit0[s])
                u0 = plan.unit0[s], pos0 = plan.pos0[s], cnt = plan.count[s], dp0 = plan.pair0[s];
        const int r0 = 2 * (unit - u0);
        const bool two = r0 + 1 < cnt;
        const unsigned atom[2] = {(unsigned)order[pos0 + r0], (unsigned)order[pos0 + r0 + (two ? 1 : 0)]};
        const double wt[2] = {w ? w[atom[0]] : 1.0, w ? w[atom[1]] : 1.0};
        double val[F][2 * D];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const unsigned c = atom[a] * (unsigned)D;  // (n_atoms dim < 2^31: launch_species_sort)
            const bool odd = c & 1;
            // the D columns of the atom in every frame of the thread, and in the first frame
            double col[F][3], col0[3];
            if constexpr (!kF32) {
                const double2* src = reinterpret_cast<const double2*>(x) + (long)(c >> 1) * pitch;
                const double2 a0 = src[0], b0 = NP == 2 ? src[pitch] : a0;  // (one address for the whole workgroup)
                sort_pick<D>(a0.x, a0.y, b0.x, b0.y, odd, col0);
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    const long t = frame(f), i = t < T ? t : 0;
                    const double2 qa = src[i], qb = NP == 2 ? src[pitch + i] : qa;
                    sort_pick<D>(qa.x, qa.y, qb.x, qb.y, odd, col[f]);
                }
            } else {
                const long hp = pitch / 2;
                const float4* src = reinterpret_cast<const float4*>(x) + (long)(c >> 1) * hp;
                const float4 a0 = src[0], b0 = NP == 2 ? src[hp] : a0;
                sort_pick<D>(a0.x, a0.y, b0.x, b0.y, odd, col0);
#pragma unroll
                for (int f = 0; f < F; f += 2) {
                    const long t = frame(f), i = t < T ? t / 2 : 0;  // t is even
                    const float4 qa = src[i], qb = NP == 2 ? src[hp + i] : qa;
                    sort_pick<D>(qa.x, qa.y, qb.x, qb.y, odd, col[f]);
                    sort_pick<D>(qa.z, qa.w, qb.z, qb.w, odd, col[f + 1]);
                }
            }
            // the shift comes before the weight (k_cond_moment's W)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const double first = shift ? col0[j] : 0.0;
#pragma unroll
                for (int f = 0; f < F; ++f) val[f][a * D + j] = a == 0 || two ? wt[a] * (col[f][j] - first) : 0.0;
            }
        }
        const int n_out = two ? D : (D + 1) / 2;  // whole pairs of this unit inside its species' block
        double2* dst = reinterpret_cast<double2*>(W) + (dp0 + (long)D * (unit - u0)) * pitch;
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const long t = frame(f);
            if (t >= pitch) continue;
            const bool live = t < T;
#pragma unroll
            for (int j = 0; j < D; ++j)
                if (j < n_out) dst[j * pitch + t] = live ? double2{val[f][2 * j], val[f][2 * j + 1]} : double2{0.0, 0.0};
        }
    }
}

template <class E, int D>
void sort_launch(dim3 grid, hipStream_t st, const void* x, long pitch, long T, const SortPlan& plan, const int* order,
                 const double* w, int shift, double* W) {
    hipLaunchKernelGGL((k_species_sort<E, D>), grid, dim3(kSortThreads), 0, st, (const E*)x, pitch, T, plan, order, w, shift, W);
}
template <class E>
void sort_launch_dim(int D, dim3 grid, hipStream_t st, const void* x, long pitch, long T, const SortPlan& plan, const int* order,
                     const double* w, int shift, double* W) {
    if (D == 1) sort_launch<E, 1>(grid, st, x, pitch, T, plan, order, w, shift, W);
    else if (D == 2) sort_launch<E, 2>(grid, st, x, pitch, T, plan, order, w, shift, W);
    else sort_launch<E, 3>(grid, st, x, pitch, T, plan, order, w, shift, W);
}

}  // namespace

// The blocks and the sorted order of host labels in [0, S) (checked by the caller): order[pos0[s] + r] = the atom of rank
// r in species s (input order kept), count[s] atoms in units unit0[s] ... of two, first destination pair pair0[s].
void species_sort_plan(const int32_t* h_species, int64_t n_atoms, int D, int S, SortPlan* plan, int32_t* order) {
    *plan = SortPlan{};
    plan->n_species = S;
    for (int64_t a = 0; a < n_atoms; ++a) ++plan->count[h_species[a]];
    int pos = 0, unit = 0;
    long pair = 0;
    for (int s = 0; s < S; ++s) {
        plan->pos0[s] = pos, plan->unit0[s] = unit, plan->pair0[s] = pair;
        pos += plan->count[s];
        unit += (plan->count[s] + 1) / 2;
        pair += ((long)plan->count[s] * D + 1) / 2;
    }
    plan->n_units = unit, plan->n_pairs = pair;
    int next[TA_ONSAGER_MAX_SPECIES];
    for (int s = 0; s < S; ++s) next[s] = plan->pos0[s];
    for (int64_t a = 0; a < n_atoms; ++a) order[next[h_species[a]]++] = (int32_t)a;
}

hipError_t launch_species_sort(int n_cu, const void* x, bool f32, long pitch, long T, long n_cols, int D, const SortPlan& plan,
                               const int* order, const double* w, bool shift, double* W, hipStream_t st) {
    if (D < 1 || D > 3 || n_cols < 1 || n_cols >= (1L << 31) || (pitch & 7) || T < 1 || T > pitch || plan.n_units < 1)
        return hipErrorInvalidValue;
    // about sixteen workgroups per CU over the frame blocks, at most one group per unit
    const long n_tb = (pitch + kSortThreads * kSortFrames - 1) / (kSortThreads * kSortFrames);
    const long want = (16L * n_cu + n_tb - 1) / n_tb;
    const dim3 grid((unsigned)n_tb, (unsigned)std::max(1L, std::min({want, (long)plan.n_units, 65535L})));
    if (f32) sort_launch_dim<float>(D, grid, st, x, pitch, T, plan, order, w, shift, W);
    else sort_launch_dim<double>(D, grid, st, x, pitch, T, plan, order, w, shift, W);
    return hipGetLastError();
}

}  // namespace ta
