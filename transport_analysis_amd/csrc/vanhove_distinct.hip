// vanhove_distinct.hip — the distinct part of the van Hove function: for L lags tau_l the histogram of the distances between
// item a_p at an origin frame t and item b_q at frame t + tau, a_p != b_q, under the one-step minimum image of an
// orthorhombic box, against squared bin edges
//
//   counts[l, b] = #{(o, p, q): t = stride o, t + tau_l < T, a_p != b_q, e[b] <= r2 < e[b + 1]}   (b = B: r2 >= e[B])   uint64 (L, B + 1)
//
// with the arithmetic of vanhove_distinct_math.hpp (the CPU backend follows it: equal counts for any input).  The cost is
// O(Na Nb) per origin and lag, and the pair-major slab is contiguous along TIME: a lane per frame would put a wave's 64
// lanes on one LDS bin (a pair's distance hardly moves between neighbouring frames).  So there are two passes:
//
//   k_vhd_gather<E, D>   O(N) per chunk of lags: reads the slab through PmAtom in its own element type (a float32 slab as
//                        float32, one 8-byte row per load: nothing at or past row T is read) and writes frame-major
//                        float64 scratch with the ITEM index contiguous, GA[o][d][p] = x[stride o, a_p, d] and
//                        GB[l][o][d][q] = x[stride o + tau_l, b_q, d], the item pitch padded to the pair kernel's tiles
//                        (padding written as zeros; its ids are -1).  The element type, the index lists, the stride and
//                        the lag's parity are settled here.
//   k_vhd_pairs<D, PERIODIC>   the hot pass: a workgroup takes one (lag, origin, tile of a, tile of b) and walks it with
//                        pair_tile_walk (pair_tile.hpp, shared with k_pair_find of pair_lifetime.hip: the tiles, the lane's
//                        b-items in registers, the a-items by scalar loads, the id rule's operands and r2).  The kernel
//                        itself is the LDS setup, the visitor "r2 < e[B]: vh_bin and one LDS integer add; otherwise a register
//                        counter", and the flush: the non-zero bins and the waves' overflow sums go into the uint64
//                        histogram by integer atomics.
//
// Only integer adds: the same bits in any order, from run to run and for every chunk size.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "pair_tile.hpp"

namespace ta {
namespace {

// grid (item blocks of the pitch, origins (looped), slots): slot z < with_a is GA, the others the chunk's lags.  ids: the
// padded index list of the slot's side (-1: padding, written as zeros).  A lagged row t + tau >= T is neither read nor
// written: k_vhd_pairs never starts a workgroup for it.  o_base: the scratch's origin 0 is origin o_base of the slab (0 for
// the van Hove passes; the pair search of pair_lifetime.hip gathers its searched frames in chunks).
template <class E, int D>
__global__ void __launch_bounds__(kPmThreads)
    k_vhd_gather(const E* __restrict__ x, long pitch, long T, long stride, long n_orig, const long* __restrict__ lags, int with_a,
                 const int* __restrict__ ida, const int* __restrict__ idb, long pitch_a, long pitch_b, double* __restrict__ ga,
                 double* __restrict__ gb, long o_base) {
    const int z = blockIdx.z;
    const bool side_a = z < with_a;
    const long ip = side_a ? pitch_a : pitch_b;
    const long p = (long)blockIdx.x * kPmThreads + threadIdx.x;
    if (p >= ip) return;
    const int id = side_a ? ida[p] : idb[p];
    const long tau = side_a ? 0 : lags[z - with_a];
    double* out = side_a ? ga : gb + (size_t)(z - with_a) * (size_t)n_orig * D * (size_t)pitch_b;
    for (long o = blockIdx.y; o < n_orig; o += gridDim.y) {
        const long t = (o_base + o) * stride + tau;
        if (t >= T) break;
        double v[3] = {0.0, 0.0, 0.0};
        if (id >= 0) {
            PmAtom<E, D>(x, pitch, (unsigned)id).row(t, v);  // (atom D < 2^31: launch_vhd_gather; row t alone: t + 1 may be row T)
        }
#pragma unroll
        for (int d = 0; d < D; ++d) out[((size_t)o * D + d) * (size_t)ip + p] = v[d];
    }
}

// grid (a-tiles x b-tiles, origins o0 + y, the chunk's lags).  lags, counts: the chunk's.  hm: per box (one, or one per
// frame: box_per_frame) H[3] then M[3] of the staged columns.  LDS: e[B + 1] doubles, then the uint32 histogram [B + 1].
template <int D, bool PERIODIC>
__global__ void __launch_bounds__(kPmThreads)
    k_vhd_pairs(const double* __restrict__ ga, const double* __restrict__ gb, const int* __restrict__ ida,
                const int* __restrict__ idb, long pitch_a, long pitch_b, int n_a, int n_tb, long T, long stride, long n_orig,
                long o0, const long* __restrict__ lags, const double* __restrict__ hm, int box_per_frame,
                const double* __restrict__ e_g, int B, float inv_dr, unsigned long long* __restrict__ counts) {
    const long o = o0 + blockIdx.y;
    const long t = o * stride;
    if (o >= n_orig || t + lags[blockIdx.z] >= T) return;  // (the whole workgroup: before any barrier)
    extern __shared__ __attribute__((aligned(16))) unsigned char vhd_lds[];
    const int nb = B + 1;
    double* e = reinterpret_cast<double*>(vhd_lds);
    unsigned* hist = reinterpret_cast<unsigned*>(e + nb);
    for (int i = threadIdx.x; i < nb; i += kPmThreads) e[i] = e_g[i], hist[i] = 0;
    __syncthreads();

    const double e_top = e_g[B];
    unsigned over = 0;
    const PairTile tile = pair_tile_of(blockIdx.x, n_a, n_tb);
    pair_tile_walk<D, PERIODIC>(ga + (size_t)o * D * (size_t)pitch_a, gb + ((size_t)blockIdx.z * (size_t)n_orig + (size_t)o) * D * (size_t)pitch_b,
                                ida, idb, pitch_a, pitch_b, tile.p0, tile.p1, tile.tile_b, hm + (box_per_frame ? t * 6 : 0),
                                [&](int, int, int id, int idq, double r2) {  // bin or overflow
                                    if (idq >= 0 && idq != id) {
                                        if (r2 < e_top) atomicAdd(&hist[vh_bin(r2, e, B, inv_dr)], 1u);
                                        else ++over;
                                    }
                                });
    __syncthreads();
    unsigned long long* row = counts + (size_t)blockIdx.z * nb;
    for (int i = threadIdx.x; i < B; i += kPmThreads) {
        const unsigned v = hist[i];
        if (v) atomicAdd(&row[i], (unsigned long long)v);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) over += __shfl_xor(over, m);  // (a wave's sum: at most 2^18)
    if ((threadIdx.x & 63) == 0 && over) atomicAdd(&row[B], (unsigned long long)over);
}

}  // namespace

hipError_t launch_vhd_gather(const void* x, bool f32, long pitch, long T, long n_atoms, int D, long stride, long n_orig,
                             const int64_t* lags, int Lc, bool with_a, const int* ida, const int* idb, long pitch_a, long pitch_b,
                             double* ga, double* gb, hipStream_t st, long o_base) {
    if (!pm_slab_ok(pitch, T, n_atoms, D) || stride < 1 || n_orig < 1 || o_base < 0 || (o_base + n_orig - 1) * stride >= T || Lc < 1 ||
        Lc > TA_VANHOVE_MAX_LAGS || pitch_a < 1 || pitch_b < 1 || pitch_a % VHD_TILE_A || pitch_b % VHD_TILE_B)
        return hipErrorInvalidValue;
    const long ip = std::max(pitch_a, pitch_b);
    const dim3 grid((unsigned)((ip + kPmThreads - 1) / kPmThreads), (unsigned)std::min(n_orig, 65535L), (unsigned)(Lc + (with_a ? 1 : 0)));
    pm_dispatch(f32, D, [&](auto e, auto d) {
        using E = decltype(e);
        hipLaunchKernelGGL((k_vhd_gather<E, d()>), grid, dim3(kPmThreads), 0, st, (const E*)x, pitch, T, stride, n_orig, pm_lags(lags),
                           with_a ? 1 : 0, ida, idb, pitch_a, pitch_b, ga, gb, o_base);
    });
    return hipGetLastError();
}

hipError_t launch_vhd_pairs(const double* ga, const double* gb, const int* ida, const int* idb, long pitch_a, long pitch_b, long n_a,
                            long n_b, int D, long T, long stride, long n_orig, long o0, int n_o, const int64_t* lags, int Lc,
                            const double* hm, bool box_per_frame, const double* e, int B, float inv_dr, unsigned long long* counts,
                            hipStream_t st) {
    const long n_ta = (n_a + VHD_TILE_A - 1) / VHD_TILE_A, n_tb = (n_b + VHD_TILE_B - 1) / VHD_TILE_B;
    if (!pair_tile_ok(pitch_a, pitch_b, n_a, n_b, D, T, stride, n_o) || n_orig < 1 || (n_orig - 1) * stride >= T || o0 < 0 ||
        o0 + n_o > n_orig || Lc < 1 || Lc > TA_VANHOVE_MAX_LAGS || B < 1 || B > TA_VANHOVE_MAX_BINS)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(n_ta * n_tb), (unsigned)n_o, (unsigned)Lc);
    const size_t lds = (sizeof(double) + sizeof(unsigned)) * (size_t)(B + 1);
    auto launch = [&](auto periodic) {  // (without a box box_per_frame is 0)
        return pm_switch<1, 3>(D, [&](auto d) {
            auto* kernel = k_vhd_pairs<decltype(d)::value, decltype(periodic)::value>;
            const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (err != hipSuccess) return err;
            hipLaunchKernelGGL(kernel, grid, dim3(kPmThreads), lds, st, ga, gb, ida, idb, pitch_a, pitch_b, (int)n_a, (int)n_tb, T, stride,
                               n_orig, o0, pm_lags(lags), hm, hm && box_per_frame ? 1 : 0, e, B, inv_dr, counts);
            return hipGetLastError();
        });
    };
    return hm ? launch(std::true_type{}) : launch(std::false_type{});
}

}  // namespace ta
