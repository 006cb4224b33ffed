// orient.hip — the orientation columns of the rotational correlation functions C_1(t), C_2(t) and of the dipole sum.
//
// A vector n is a row of the index table into the staged atoms: (a, b) for a bond, (a, b, c) for a bisector or a normal
// (orient_math.hpp has the arithmetic, which the CPU backend follows).  One launch writes one float64 pair-major block in
// the conventions of pm_store_row (pm_read.hpp):
//   rank 1: N "atoms" with D = 3 holding u_n(t): columns 3 n + {0, 1, 2}.  A work unit is two vectors = three whole pairs;
//           the last unit of an odd N holds one vector and writes its phantom column as 0 (two pairs).
//   rank 2: 2 N pseudo-atoms with D = 3: for vector n (Qxx, Qyy, Qzz) and (sqrt2 Qxy, sqrt2 Qxz, sqrt2 Qyz), columns
//           6 n + {0 ... 5}.  A work unit is one vector = three whole pairs.
// The VACF lag sum of the rank-1 block is sum_n <u . u'> = sum_n P1, that of the rank-2 block sum_n <Q : Q'> = 2/3 sum_n P2;
// the rank-1 block's weighted sum over its atoms (k_species_sum) is the total dipole.  Rows T ... pitch - 1 of every pair
// are written as zeros (the scratch is reused between the ranks and between calls), rows >= pitch are not written.  No
// atomics, every destination element has one writer: the same bits from run to run.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "orient_math.hpp"
#include "pm_read.hpp"
#include "ta_internal.hpp"

namespace ta {
namespace {

enum { BOX_NONE = 0, BOX_CONST = 1, BOX_FRAME = 2 };

__device__ __forceinline__ OrientBox orient_box_at(const double* __restrict__ box, long tpitch, long t) {
    return OrientBox{box[t],
                     box[tpitch + t],
                     box[2 * tpitch + t],
                     box[3 * tpitch + t],
                     box[4 * tpitch + t],
                     box[5 * tpitch + t],
                     box[6 * tpitch + t],
                     box[7 * tpitch + t],
                     box[8 * tpitch + t]};
}

// u of vector `row` (its atoms at a workgroup-uniform address: scalar loads) in the thread's frames.  The atoms are read as
// the whole source pairs that cover their three columns, in the slab's element type (a float32 slab as float32, widened
// in registers); one atom's columns are dead before the next one's are loaded.
template <class E, int MODE, int BOX>
__device__ __forceinline__ void orient_vector(const E* __restrict__ x, long pitch, long T, long tb, const int* __restrict__ row,
                                              const OrientBox (&bx)[kPmFrames], double (&u)[kPmFrames][3]) {
    constexpr int F = kPmFrames;
    double a[F][3], p[F][3], db[F][3];
    pm_load(PmAtom<E, 3>(x, pitch, (unsigned)row[0]), T, tb, a);  // (atom 3 < 2^31: launch_orient)
    pm_load(PmAtom<E, 3>(x, pitch, (unsigned)row[1]), T, tb, p);
#pragma unroll
    for (int f = 0; f < F; ++f) orient_diff<BOX != BOX_NONE>(a[f], p[f], bx[BOX == BOX_FRAME ? f : 0], db[f]);
    if constexpr (MODE != ORIENT_BOND) pm_load(PmAtom<E, 3>(x, pitch, (unsigned)row[2]), T, tb, p);
#pragma unroll
    for (int f = 0; f < F; ++f) {
        double dc[3] = {0.0, 0.0, 0.0}, v[3];
        if constexpr (MODE != ORIENT_BOND) orient_diff<BOX != BOX_NONE>(a[f], p[f], bx[BOX == BOX_FRAME ? f : 0], dc);
        orient_combine<MODE>(db[f], dc, v);
        orient_unit(v, u[f]);
    }
}

// Workgroup (bx, g): frames [1024 bx, 1024 bx + 1024) of the pitch, units g, g + G, ... (G = gridDim.y), as k_phase.  The
// box entries a thread's frames need do not depend on the unit: a constant box is nine scalar values, a per-frame box is
// loaded ONCE before the loop over units into registers (9 per frame; DESIGN has the compiled figures behind that choice).
// Each store is a full 16-byte row, contiguous along time across a wave.
template <class E, int MODE, int RANK, int BOX>
__global__ void __launch_bounds__(kPmThreads)
    k_orient(const E* __restrict__ x, long pitch, long T, int N, const int* __restrict__ index, const double* __restrict__ box,
             long tpitch, double* __restrict__ Z) {
    constexpr bool kF32 = std::is_same_v<E, float>;
    constexpr int F = kPmFrames, K = MODE == ORIENT_BOND ? 2 : 3;
    const long tb = (long)blockIdx.x * (kPmThreads * F);
    OrientBox bx[F] = {};
    if constexpr (BOX == BOX_CONST) bx[0] = orient_box_at(box, 1, 0);
    if constexpr (BOX == BOX_FRAME) {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const long t = pm_frame<kF32>(tb, f);
            bx[f] = orient_box_at(box, tpitch, t < T ? t : 0);  // (a frame >= T stores zeros: any box will do)
        }
    }
    double2* Zp = reinterpret_cast<double2*>(Z);
    const int n_units = RANK == 1 ? (N + 1) / 2 : N;
    for (int g = blockIdx.y; g < n_units; g += gridDim.y) {
        double2* dst = Zp + 3L * g * pitch;
        if constexpr (RANK == 1) {
            const bool two = 2 * g + 1 < N;  // (workgroup-uniform)
            double u0[F][3], u1[F][3] = {};
            orient_vector<E, MODE, BOX>(x, pitch, T, tb, index + (long)(2 * g) * K, bx, u0);
            if (two) orient_vector<E, MODE, BOX>(x, pitch, T, tb, index + (long)(2 * g + 1) * K, bx, u1);
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const long t = pm_frame<kF32>(tb, f);
                if (t >= pitch) continue;
                const double v[6] = {u0[f][0], u0[f][1], u0[f][2], u1[f][0], u1[f][1], u1[f][2]};
                pm_store_row<3>(dst, pitch, t, t < T, two ? 3 : 2, v);
            }
        } else {
            double u[F][3];
            orient_vector<E, MODE, BOX>(x, pitch, T, tb, index + (long)g * K, bx, u);
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const long t = pm_frame<kF32>(tb, f);
                if (t >= pitch) continue;
                double v[6];
                orient_q(u[f], v);
                pm_store_row<3>(dst, pitch, t, t < T, 3, v);
            }
        }
    }
}

}  // namespace

hipError_t launch_orient(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, int mode, int rank,
                         long n_vectors, const int* index, const double* box, long tpitch, double* Z, hipStream_t st) {
    if (D != 3 || !pm_slab_ok(pitch, T, n_atoms, D) || n_vectors < 1 || 2 * n_vectors * 3 >= (1L << 31) || mode < ORIENT_BOND ||
        mode > ORIENT_NORMAL || (rank != 1 && rank != 2) || !index || (box && tpitch != 1 && tpitch < T))
        return hipErrorInvalidValue;
    const dim3 grid = pm_unit_grid(n_cu, pitch, rank == 1 ? (n_vectors + 1) / 2 : n_vectors);
    // <MODE, RANK, BOX> as one variant number for the switch
    static_assert(ORIENT_BOND == 0 && ORIENT_NORMAL == 2 && BOX_NONE == 0 && BOX_FRAME == 2, "the variant's digits");
    const int variant = (mode * 2 + (rank - 1)) * 3 + (!box ? BOX_NONE : tpitch == 1 ? BOX_CONST : BOX_FRAME);
    pm_element(f32, [&](auto e) {
        pm_switch<0, 17>(variant, [&](auto v) {
            using E = decltype(e);
            constexpr int c = decltype(v)::value;
            hipLaunchKernelGGL((k_orient<E, c / 6, c / 3 % 2 + 1, c % 3>), grid, dim3(kPmThreads), 0, st, (const E*)x, pitch, T,
                               (int)n_vectors, index, box, tpitch, Z);
        });
    });
    return hipGetLastError();
}

}  // namespace ta
