// shell.hip — the kernel of the shell residence times (include/ta_hip.h, ta_shell_residence): the level of every OBSERVED item
// against a whole group of reference items,
//   form_q(t) = some reference item p != q with r2(p, q, t) < rc2,   brk_q(t) = the same with rb2 >= rc2,
//   level = shell_level(form, brk) of bond_math.hpp,
// written as the pair-major float64 block Z that k_pair_filter, k_pair_runs and the lag sums of pair_lifetime.hip read: one
// pseudo-atom of dim 1 per observed item.  r2 is vhd_r2 with d = x_q - x_p, the compares are strict, rc2 and rb2 come from
// the host: a group of ONE reference item gives k_bond_series' block of the rows (p, q), bit for bit.
//
//   k_shell_series<D, PERIODIC>  grid (b-tiles, 64-frame words of the chunk).  A workgroup owns VHD_TILE_B observed items (a lane
//                                kPairR of them, in registers) and the frames [64 w, 64 w + 64) of the frame-major scratch
//                                that k_vhd_gather wrote at lag 0, stride 1.  Per frame it walks ALL reference items with
//                                pair_tile_walk (scalar loads, a uniform loop) and ORs the two flags per owned item.  A
//                                wave's lanes hold 64 consecutive items, so its ballots of the flags after frame f ARE the
//                                64-item words of that frame; lane f keeps them (2 kPairR words per lane).  After the last
//                                frame lane f holds every item's bits at frame 64 w + f: the transposition from item-major
//                                ballots to time-major rows took no LDS and no shuffle.  Per pair of items (2 i, 2 i + 1) the
//                                lane stores ONE 16-byte row of Z; the wave's 64 rows are 1024 contiguous bytes.  Every row
//                                below the pitch of every destination pair has one writer: rows T ... pitch - 1 (never
//                                walked) and padding items (an odd count's phantom column) are zeros.  No atomics, no LDS,
//                                every trip count depends on the shapes alone, the ballots sit outside every divergent branch.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "bond_math.hpp"
#include "pair_tile.hpp"

namespace ta {
namespace {

// ga [n_f][D][pitch_a], gb [n_f][D][pitch_b]: the chunk's gathered frames, frame y of the chunk is frame f_base + y of the
// slab (f_base a multiple of 64; its box with box_per_frame).  ida, idb: the padded lists of the scratch (-1: padding).
// Z: n_units destination pairs of `pitch` rows: unit u holds the items 2 u, 2 u + 1 of idb.
template <int D, bool PERIODIC>
__global__ void __launch_bounds__(kPmThreads)
    k_shell_series(const double* __restrict__ ga, const double* __restrict__ gb, const int* __restrict__ ida,
                   const int* __restrict__ idb, long pitch_a, long pitch_b, int n_a, long n_f, long f_base,
                   const double* __restrict__ hm, int box_per_frame, double rc2, double rb2, double two, long pitch, long n_units,
                   double* __restrict__ Z) {
    const int lane = threadIdx.x & 63;
    const long f0 = (long)blockIdx.y * 64;  // the word's first frame in the chunk
    bool real[kPairR];
#pragma unroll
    for (int r = 0; r < kPairR; ++r) real[r] = idb[(long)blockIdx.x * VHD_TILE_B + r * kPmThreads + threadIdx.x] >= 0;
    unsigned long long F[kPairR] = {}, B[kPairR] = {};  // lane f: the items' form / break bits of frame f0 + f
    const int nf = (int)min(64L, n_f - f0);             // (the last word of the series may be partial)
    for (int f = 0; f < nf; ++f) {
        const long o = f0 + f;
        bool in_form[kPairR] = {}, in_brk[kPairR] = {};
        pair_tile_walk<D, PERIODIC>(ga + (size_t)o * D * (size_t)pitch_a, gb + (size_t)o * D * (size_t)pitch_b, ida, idb, pitch_a, pitch_b, 0,
                                    n_a, (int)blockIdx.x, hm + (box_per_frame ? (f_base + o) * 6 : 0),
                                    [&](int, int r, int id, int idq, double r2) {
                                        const bool other = id != idq;
                                        in_form[r] |= r2 < rc2 && other;
                                        in_brk[r] |= r2 < rb2 && other;
                                    });
#pragma unroll
        for (int r = 0; r < kPairR; ++r) {
            const unsigned long long wf = __ballot(in_form[r] && real[r]), wb = __ballot(in_brk[r] && real[r]);
            if (lane == f) F[r] = wf, B[r] = wb;
        }
    }
    const long t = f_base + f0 + lane;
    if (t >= pitch) return;
    double2* Zp = reinterpret_cast<double2*>(Z);
#pragma unroll
    for (int r = 0; r < kPairR; ++r) {
        const long u0 = ((long)blockIdx.x * VHD_TILE_B + r * kPmThreads + (threadIdx.x - lane)) / 2;  // the wave's first unit of r
        const int n_u = (int)max(0L, min(32L, n_units - u0));                                           // (wave-uniform)
        for (int i = 0; i < n_u; ++i) {
            const int l0 = shell_level((F[r] >> (2 * i)) & 1ull, (B[r] >> (2 * i)) & 1ull);
            const int l1 = shell_level((F[r] >> (2 * i + 1)) & 1ull, (B[r] >> (2 * i + 1)) & 1ull);
            Zp[(size_t)(u0 + i) * (size_t)pitch + t] = double2{l0 == 2 ? two : l0 == 1 ? 1.0 : 0.0, l1 == 2 ? two : l1 == 1 ? 1.0 : 0.0};
        }
    }
}

}  // namespace

hipError_t launch_shell_series(const double* ga, const double* gb, const int* ida, const int* idb, long pitch_a, long pitch_b, long n_a,
                               long n_b, int D, long T, long pitch, long f_base, long n_f, const double* hm, bool box_per_frame,
                               double rc2, double rb2, double two, double* Z, hipStream_t st) {
    const long n_tb = (n_b + VHD_TILE_B - 1) / VHD_TILE_B, n_words = (n_f + 63) / 64;
    if (D < 1 || D > 3 || n_a < 1 || n_b < 1 || n_a > pitch_a || n_a >= (1L << 31) || pitch_a % VHD_TILE_A || pitch_b != n_tb * VHD_TILE_B ||
        n_tb >= (1L << 31) || T < 1 || T > pitch || f_base < 0 || f_base % 64 || n_f < 1 || f_base + n_f > T || n_words > 65535 || !(rc2 > 0.0) ||
        !(rb2 >= rc2) || (two != 1.0 && two != 2.0) || !ga || !gb || !ida || !idb || !Z)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)n_tb, (unsigned)n_words);
    auto launch = [&](auto periodic) {
        pm_switch<1, 3>(D, [&](auto d) {
            hipLaunchKernelGGL((k_shell_series<decltype(d)::value, decltype(periodic)::value>), grid, dim3(kPmThreads), 0, st, ga, gb, ida, idb,
                               pitch_a, pitch_b, (int)n_a, n_f, f_base, hm, hm && box_per_frame ? 1 : 0, rc2, rb2, two, pitch, (n_b + 1) / 2, Z);
        });
    };
    if (hm) launch(std::true_type{});
    else launch(std::false_type{});
    return hipGetLastError();
}

}  // namespace ta
