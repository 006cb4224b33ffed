// pair_tile.hpp — the tile walk that k_vhd_pairs (vanhove_distinct.hip), k_pair_find (pair_lifetime.hip) and k_shell_series
// (shell.hip) share, over the frame-major float64 scratch of k_vhd_gather.  A workgroup of the first two takes (VHD_TILE_A
// a-items, VHD_TILE_B b-items) of one frame pair; k_shell_series' takes all a-items against one b-tile, frame after frame.
// A lane keeps kPairR b-items (kPairR (2 D + 1) VGPRs for D = 3: 28 of them; the bound is registers: twice as many would cost
// occupancy without saving anything, the a-item's scalar loads are already shared by 4 pairs per lane), so the b-tile is
// 256 kPairR = 1024 items; the a-tile is 256 items, bounded by nothing but the wish for enough workgroups per frame at a few
// thousand items.  A workgroup visits at most 2^18 pairs: a uint32 count of them stays below 2^31 by construction.
#pragma once
#include "pm_read.hpp"
#include "ta_internal.hpp"
#include "vanhove_distinct_math.hpp"

namespace ta {

constexpr int kPairR = VHD_TILE_B / kPmThreads;  // b-items per lane
static_assert(kPmThreads * kPairR == VHD_TILE_B && kPairR == 4, "a lane's b-items are r kPmThreads + threadIdx.x: a wave's 64 lanes hold 64 consecutive ones");
static_assert((long)VHD_TILE_A * VHD_TILE_B < (1L << 31), "a workgroup's pair count must stay below 2^31");

// what both launchers check of the lists, the tiles and the frames of one launch (n_o: the grid's y)
inline bool pair_tile_ok(long pitch_a, long pitch_b, long n_a, long n_b, int D, long T, long stride, int n_o) {
    const long n_ta = (n_a + VHD_TILE_A - 1) / VHD_TILE_A, n_tb = (n_b + VHD_TILE_B - 1) / VHD_TILE_B;
    return D >= 1 && D <= 3 && n_a >= 1 && n_b >= 1 && n_a <= pitch_a && n_b <= pitch_b && pitch_a % VHD_TILE_A == 0 &&
           pitch_b % VHD_TILE_B == 0 && n_ta * n_tb < VHD_MAX_TILES && T >= 1 && stride >= 1 && n_o >= 1 && n_o <= 65535;
}

// tile x = tile_a n_tb + tile_b of a grid of a-tiles x b-tiles (k_vhd_pairs, k_pair_find): its a-items [p0, p1) and its b-tile
struct PairTile {
    int p0, p1, tile_b;
};
__device__ __forceinline__ PairTile pair_tile_of(unsigned x, int n_a, int n_tb) {
    const int p0 = (int)(x / n_tb) * VHD_TILE_A;
    return {p0, min(p0 + VHD_TILE_A, n_a), (int)(x % n_tb)};
}

// The walk of the a-items [p0, p1) against b-tile tile_b, all three workgroup-uniform (a tile of pair_tile_of, or every a-item
// against one b-tile: k_shell_series).  gao [D][pitch_a], gbo [D][pitch_b]: the two frames' gathered items; ida,
// idb: the padded lists (-1: padding); box: H[3] then M[3] of the a-frame (PERIODIC).  The lane's b-items q = tile_b VHD_TILE_B
// + r kPmThreads + threadIdx.x, r < kPairR, sit in registers; the a-items p come by scalar loads (the loop is uniform: visit
// may hold a ballot).  visit(p, r, id_a, id_b, r2) for every (p, r): r2 = vhd_r2<D, PERIODIC>; id_b < 0 is padding, which the
// visitor tests with its own id rule (handed over as a flag formed here, the hoisted flag took VCC for the whole loop and
// every compare of k_vhd_pairs' bin search went to a scalar pair: docs/HISTORY.md).
template <int D, bool PERIODIC, class Visit>
__device__ __forceinline__ void pair_tile_walk(const double* __restrict__ gao, const double* __restrict__ gbo, const int* __restrict__ ida,
                                               const int* __restrict__ idb, long pitch_a, long pitch_b, int p0, int p1, int tile_b,
                                               const double* __restrict__ box, Visit&& visit) {
    double H[3] = {1.0, 1.0, 1.0}, M[3] = {1.0, 1.0, 1.0};
    if constexpr (PERIODIC) {
#pragma unroll
        for (int d = 0; d < D; ++d) H[d] = box[d], M[d] = box[3 + d];
    }
    double xb[kPairR][3];
    int idq[kPairR];
#pragma unroll
    for (int r = 0; r < kPairR; ++r) {
        const long q = (long)tile_b * VHD_TILE_B + r * kPmThreads + threadIdx.x;  // (< pitch_b: a multiple of the tile)
        idq[r] = idb[q];
#pragma unroll
        for (int d = 0; d < 3; ++d) xb[r][d] = d < D ? gbo[(size_t)d * pitch_b + q] : 0.0;
    }
    for (int p = p0; p < p1; ++p) {  // (uniform: the a-item comes by scalar loads)
        double xa[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int d = 0; d < D; ++d) xa[d] = gao[(size_t)d * pitch_a + p];
        const int id = ida[p];
#pragma unroll
        for (int r = 0; r < kPairR; ++r) visit(p, r, id, idq[r], vhd_r2<D, PERIODIC>(xa, xb[r], H, M));
    }
}

}  // namespace ta
