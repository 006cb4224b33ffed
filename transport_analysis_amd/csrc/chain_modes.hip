// chain_modes.hip — linear functionals of whole chains (Rouse normal modes, the end-to-end vector) of a staged position slab.
//
// A chain c is row c of the member table, N >= 2 atoms of the slab in backbone order.  Per frame the pass walks the beads
// once, makes the chain whole on the way and keeps up to MC functionals in registers (chain_math.hpp has the arithmetic,
// which the CPU backend follows):
//   s_1 = 0,  s_n = s_{n-1} + img(x[m_n] - x[m_{n-1}]),     Y_q(c, t) = sum_{n = 2 ... N} coeff[q][n - 1] s_n
// One launch writes the blocks of its n_q <= MC functionals, mode-major: block q is a float64 pair-major block in the
// conventions of pm_store_row (pm_read.hpp) of n_chains pseudo-atoms with D = 3 holding Y_q: columns 3 c + {0, 1, 2}.  A work
// unit is two consecutive chains = three whole pairs; the last unit of an odd n_chains holds one chain and writes its
// phantom column as 0 (two pairs).  Rows T ... pitch - 1 of every pair are written as zeros (the block is reused between
// batches and calls), rows >= pitch are not written.  No atomics, no LDS, every destination element has one writer: the same
// bits from run to run, and a functional's block does not depend on which launch or batch formed it.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "chain_math.hpp"
#include "pm_read.hpp"
#include "ta_internal.hpp"

// The shipped tile: MC functionals x F frames per thread, chosen by measurement among (2, 4), (4, 4), (4, 2) and (8, 2): a
// launch costs one streaming read of the slab for every one of them while a per-frame box does not push the kernel to one
// wave per SIMD (both F = 4 tiles: 1.4 - 1.6x there), so the widest tile that stays at two waves wins -- half the launches
// of (4, 2) at 16 modes for 1.08x (float64 slab) / 1.29x (float32) its launch (DESIGN 4.27 and docs/HISTORY.md have the
// figures).  -DTA_CHAIN_MC / -DTA_CHAIN_F build another one.
#ifndef TA_CHAIN_MC
#define TA_CHAIN_MC 8
#endif
#ifndef TA_CHAIN_F
#define TA_CHAIN_F 2
#endif

namespace ta {
namespace {

constexpr int kChainModes = TA_CHAIN_MC, kChainFrames = TA_CHAIN_F;
static_assert(kChainFrames % 2 == 0, "a float32 load is two frames");

enum { BOX_NONE = 0, BOX_CONST = 1, BOX_FRAME = 2 };

__device__ __forceinline__ OrientBox chain_box_at(const double* __restrict__ box, long tpitch, long t) {
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

// Workgroup (bx, g): frames [256 F bx, 256 F (bx + 1)) of the pitch, units g, g + G, ... (G = gridDim.y), as k_compound.  A
// chain's members and the coefficients depend on blockIdx and loop counters only: plain indexed reads, scalar registers,
// read-only.  The box entries a thread's frames need do not depend on the unit: a constant box is nine scalar values, a
// per-frame box is loaded once before the loop over units (k_orient's choice).  The bead loop is unrolled by two: both
// beads' loads are in flight before the first is used; the terms still enter s and acc in bead order.
// Live across the bead loop: MC F 3 accumulators, s, the previous bead and the two beads in flight (4 F 3).  The first
// chain's (x, y) is a whole destination row and is stored as soon as the chain is done; only its z waits for the second
// chain's x: the store buffer is MC F doubles.
template <class E, int BOX, int MC, int F>
__global__ void __launch_bounds__(kPmThreads)
    k_chain_modes(const E* __restrict__ x, long pitch, long T, int n_chains, int N, const int* __restrict__ member,
                  const double* __restrict__ coeff, int n_q, const double* __restrict__ box, long tpitch,
                  double* __restrict__ Z, long block_pairs) {
    constexpr bool kF32 = std::is_same_v<E, float>;
    constexpr bool kPeriodic = BOX != BOX_NONE;
    const long tb = (long)blockIdx.x * (kPmThreads * F);
    OrientBox bx[F] = {};
    if constexpr (BOX == BOX_CONST) bx[0] = chain_box_at(box, 1, 0);
    if constexpr (BOX == BOX_FRAME) {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const long t = pm_frame<kF32>(tb, f);
            bx[f] = chain_box_at(box, tpitch, t < T ? t : 0);  // (a frame >= T stores zeros: any box will do)
        }
    }
    double2* Zp = reinterpret_cast<double2*>(Z);
    const int n_units = (n_chains + 1) / 2;
    for (int unit = blockIdx.y; unit < n_units; unit += gridDim.y) {
        const bool two = 2 * unit + 1 < n_chains;  // (workgroup-uniform)
        double2* dst = Zp + 3L * unit * pitch;
        double zbuf[MC][F];  // the first chain's z
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            if (a == 1 && !two) continue;
            const int* row = member + (long)(2 * unit + a) * N;
            double acc[MC][F][3] = {}, s[F][3] = {}, prev[F][3], ca[F][3], cb[F][3];
            // (atom 3 < 2^31: launch_chain_modes)
            auto load = [&](int n, double (&col)[F][3]) { pm_load<E, 3, F>(PmAtom<E, 3>(x, pitch, (unsigned)row[n]), T, tb, col); };
            auto bead = [&](int n, const double (&from)[F][3], const double (&to)[F][3]) {
#pragma unroll
                for (int f = 0; f < F; ++f) chain_step<kPeriodic>(from[f], to[f], bx[BOX == BOX_FRAME ? f : 0], s[f]);
#pragma unroll
                for (int q = 0; q < MC; ++q) {
                    if (q >= n_q) continue;  // (workgroup-uniform)
                    const double cq = coeff[(long)q * N + n];
#pragma unroll
                    for (int f = 0; f < F; ++f) chain_term(cq, s[f], acc[q][f]);
                }
            };
            load(0, prev);
            int n = 1;
            for (; n + 1 < N; n += 2) {
                load(n, ca);
                load(n + 1, cb);
                bead(n, prev, ca);
                bead(n + 1, ca, cb);
#pragma unroll
                for (int f = 0; f < F; ++f) prev[f][0] = cb[f][0], prev[f][1] = cb[f][1], prev[f][2] = cb[f][2];
            }
            if (n < N) {
                load(n, ca);
                bead(n, prev, ca);
            }
#pragma unroll
            for (int q = 0; q < MC; ++q) {
                if (q >= n_q) continue;
                double2* d = dst + q * block_pairs * pitch;
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    const long t = pm_frame<kF32>(tb, f);
                    if (t >= pitch) continue;
                    const bool live = t < T;
                    const double2 zero{0.0, 0.0};
                    if (a == 0) {
                        d[t] = live ? double2{acc[q][f][0], acc[q][f][1]} : zero;
                        if (two) zbuf[q][f] = acc[q][f][2];
                        else d[pitch + t] = live ? double2{acc[q][f][2], 0.0} : zero;  // (the phantom column)
                    } else {
                        d[pitch + t] = live ? double2{zbuf[q][f], acc[q][f][0]} : zero;
                        d[2 * pitch + t] = live ? double2{acc[q][f][1], acc[q][f][2]} : zero;
                    }
                }
            }
        }
    }
}

// pm_unit_grid for a workgroup of 256 F frames
template <int F>
dim3 chain_grid(int n_cu, long pitch, long n_units) {
    if constexpr (F == kPmFrames) return pm_unit_grid(n_cu, pitch, n_units);
    const long n_tb = (pitch + kPmThreads * F - 1) / (kPmThreads * F);
    const long want = (16L * n_cu + n_tb - 1) / n_tb;
    return dim3((unsigned)n_tb, (unsigned)std::max(1L, std::min({want, n_units, 65535L})));
}

}  // namespace

void chain_modes_tile(int* modes, int* frames) { *modes = kChainModes, *frames = kChainFrames; }

hipError_t launch_chain_modes(int n_cu, const void* x, bool f32, long pitch, long T, long n_atoms, int D, long n_chains, int chain_len,
                              const int* member, const double* coeff, int n_q, const double* box, long tpitch, double* Z,
                              hipStream_t st) {
    if (D != 3 || !pm_slab_ok(pitch, T, n_atoms, D) || n_chains < 1 || chain_len < 2 || n_q < 1 || n_q > kChainModes ||
        (long)n_q * n_chains * 3 >= (1L << 31) || !member || !coeff || !Z || (box && tpitch != 1 && tpitch < T))
        return hipErrorInvalidValue;
    const dim3 grid = chain_grid<kChainFrames>(n_cu, pitch, (n_chains + 1) / 2);
    const long block_pairs = (3 * n_chains + 1) / 2;
    const int variant = !box ? BOX_NONE : tpitch == 1 ? BOX_CONST : BOX_FRAME;
    pm_element(f32, [&](auto e) {
        pm_switch<BOX_NONE, BOX_FRAME>(variant, [&](auto v) {
            using E = decltype(e);
            hipLaunchKernelGGL((k_chain_modes<E, decltype(v)::value, kChainModes, kChainFrames>), grid, dim3(kPmThreads), 0, st,
                               (const E*)x, pitch, T, (int)n_chains, chain_len, member, coeff, n_q, box, tpitch, Z, block_pairs);
        });
    });
    return hipGetLastError();
}

}  // namespace ta
