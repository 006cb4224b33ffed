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

#include <type_traits>

#include "pm_read.hpp"
#include "ta_internal.hpp"

namespace ta {
namespace {

// A work unit (pm_read.hpp) is two consecutive atoms (2 u, 2 u + 1) of one species in sorted order; the last unit of a
// species with an odd count holds one atom, and nothing of the next species' block is touched.  Each source atom is read
// as the whole source pairs that cover its D columns; the half that belongs to a neighbouring atom is that atom's unit's
// own load a moment earlier or later (cache).  Workgroup (bx, g): frames [1024 bx, 1024 bx + 1024) of the pitch, units g,
// g + G, ... (G = gridDim.y).  Which unit, its species, atoms, weights and column parity depend on blockIdx and the loop
// counter only: scalar registers.
template <class E, int D>
__global__ void __launch_bounds__(kPmThreads)
    k_species_sort(const E* __restrict__ x, long pitch, long T, SortPlan plan, const int* __restrict__ order,
                   const double* __restrict__ w, int shift, double* __restrict__ W) {
    constexpr int F = kPmFrames;
    const long tb = (long)blockIdx.x * (kPmThreads * F);
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
            const PmAtom<E, D> src(x, pitch, atom[a]);
            double col[F][3], col0[3];
            pm_load0(src, col0);
            pm_load(src, T, tb, col);
            // the shift comes before the weight (k_cond_moment's W)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const double first = shift ? col0[j] : 0.0;
#pragma unroll
                for (int f = 0; f < F; ++f) val[f][a * D + j] = a == 0 || two ? wt[a] * (col[f][j] - first) : 0.0;
            }
        }
        double2* dst = reinterpret_cast<double2*>(W) + (dp0 + (long)D * (unit - u0)) * pitch;
        const int n_out = two ? D : (D + 1) / 2;
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const long t = pm_frame<std::is_same_v<E, float>>(tb, f);
            if (t >= pitch) continue;
            pm_store_row<D>(dst, pitch, t, t < T, n_out, val[f]);
        }
    }
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
    const dim3 grid = pm_unit_grid(n_cu, pitch, plan.n_units);
    pm_dispatch(f32, D, [&](auto e, auto d) {
        using E = decltype(e);
        hipLaunchKernelGGL((k_species_sort<E, d()>), grid, dim3(kPmThreads), 0, st, (const E*)x, pitch, T, plan, order, w, (int)shift, W);
    });
    return hipGetLastError();
}

}  // namespace ta
