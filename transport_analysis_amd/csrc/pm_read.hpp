// pm_read.hpp — reading a pair-major slab in its own element type, and writing whole pairs of a float64 one.  Who shares what:
//   pm_frame                      every kernel that walks frames: k_species_sum (species_sum.hip) and all of the following
//   PmAtom, pm_load               k_species_sort (species_self.hip), k_compound (compound.hip), k_phase (scatter.hip), k_kcurrent
//                                 (kcurrent.hip, PmAtom::load), k_orient (orient.hip), k_vanhove (vanhove.hip), k_overlap (overlap.hip)
//   pm_lagged                     k_vanhove, k_overlap, k_overlap_density (overlap_density.hip): row t + tau of the same atom
//   PmAtom::row                   pm_lagged's odd float32 lag and float64 rows, k_vhd_gather (vanhove_distinct.hip)
//   pm_store_row                  k_species_sort, k_compound, k_orient
//   pm_unit_grid                  the launchers of the kernels that walk units
//   pm_slab_ok, pm_lags,          the launchers: the shared precondition, the lags as the kernels read them, and the runtime
//   pm_switch, pm_element,        (element type, dim) as template arguments of the one launch line
//   pm_dispatch
//
// A pair is `pitch` rows of two columns along time (pitch a multiple of 8, T <= pitch frames are live).  Every load is 16
// bytes: row t of a float64 pair, rows 2 q, 2 q + 1 of a float32 one (8-byte rows), widened in registers.  The rules:
//   * a load that would start at or past row T reads row 0 instead (its value is never stored, or adds a zero);
//   * with an odd T the last float32 load's second row is row T < pitch: nothing is read outside the pair's pitch rows;
//   * selects work on loaded VALUES with constant destinations (a select between two elements of a local array comes back
//     from the compiler as a runtime index, and the array then lives in scratch or LDS).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace ta {

constexpr int kPmThreads = 256;  // threads per workgroup of every kernel here
constexpr int kPmFrames = 4;     // frames per thread of the kernels that walk units: a workgroup covers 1024 consecutive frames

// The frame of slot i of a thread whose workgroup starts at frame tb (a multiple of 2 kPmThreads) and gives each thread F
// slots (kPmFrames, or the species sum's ROWS).  float64: tb + tid + 256 i, one load per slot.  float32: 2 (tb / 2 + tid + 256 (i / 2)) + i % 2, one load per two
// slots (F even), the workgroup's loads of a pair 4 KiB in a row.
template <bool F32>
__device__ __forceinline__ long pm_frame(long tb, int i) {
    if constexpr (F32) return tb + 2 * ((long)threadIdx.x + kPmThreads * (i / 2)) + i % 2;
    else return tb + threadIdx.x + kPmThreads * i;
}

// Column c + j of an atom (c its first column, odd = c & 1) is element j + odd of the source pairs (ax, ay), (bx, by) that
// cover its D columns: one pair for D = 1, 2 (b unused), two for D = 3
template <int D, class V>
__device__ __forceinline__ void pm_pick(V ax, V ay, V bx, V by, bool odd, double (&out)[3]) {
    if constexpr (D == 2) {
        out[0] = (double)ax, out[1] = (double)ay;  // (an atom's first column is even)
    } else {
        out[0] = (double)(odd ? ay : ax);
        if constexpr (D == 3) out[1] = (double)(odd ? bx : ay), out[2] = (double)(odd ? by : bx);
    }
}

// The one or two source pairs that cover an atom's D columns (atom D < 2^31: the launchers)
template <class E, int D>
struct PmAtom {
    static constexpr bool kF32 = std::is_same_v<E, float>;
    using Row = std::conditional_t<kF32, float4, double2>;  // what one 16-byte load gives
    const Row* src;  // the first pair
    long next;       // loads from it to the second (D = 3)
    bool odd;
    __device__ __forceinline__ PmAtom(const E* __restrict__ x, long pitch, unsigned atom)
        : next(kF32 ? pitch / 2 : pitch), odd((atom * (unsigned)D) & 1) {
        src = reinterpret_cast<const Row*>(x) + (long)((atom * (unsigned)D) >> 1) * next;
    }
    // load i of both pairs, picked into one frame's columns (float64) or two consecutive frames' (float32)
    __device__ __forceinline__ void load(long i, double (&lo)[3], double (&hi)[3]) const {
        const Row qa = src[i], qb = D == 3 ? src[next + i] : qa;
        pm_pick<D>(qa.x, qa.y, qb.x, qb.y, odd, lo);
        if constexpr (kF32) pm_pick<D>(qa.z, qa.w, qb.z, qb.w, odd, hi);
    }
    // row r (one frame) alone, in the slab's own type: float64 is load()'s 16 bytes, float32 one 8-byte load per source pair,
    // for the readers that must not take row r + 1 along (pm_lagged at an odd lag, k_vhd_gather)
    __device__ __forceinline__ void row(long r, double (&out)[3]) const {
        if constexpr (kF32) {
            const float2* p = reinterpret_cast<const float2*>(src);
            const float2 qa = p[r], qb = D == 3 ? p[2 * next + r] : qa;
            pm_pick<D>(qa.x, qa.y, qb.x, qb.y, odd, out);
        } else {
            double unused[3];
            load(r, out, unused);
        }
    }
};

// The D columns of one atom in the thread's F frames (kPmFrames, or the 2 of k_overlap_density: a workgroup then starts at
// a multiple of 256 F) ...
template <class E, int D, int F = kPmFrames>
__device__ __forceinline__ void pm_load(const PmAtom<E, D>& a, long T, long tb, double (&col)[F][3]) {
    constexpr bool kF32 = PmAtom<E, D>::kF32;
    static_assert(F % 2 == 0, "a float32 load is two frames");
#pragma unroll
    for (int f = 0; f < F; f += kF32 ? 2 : 1) {
        const long t = pm_frame<kF32>(tb, f);  // (float32: even)
        a.load(t < T ? (kF32 ? t / 2 : t) : 0, col[f], col[kF32 ? f + 1 : f]);
    }
}
// ... and in frame 0 (one address for the whole workgroup)
template <class E, int D>
__device__ __forceinline__ void pm_load0(const PmAtom<E, D>& a, double (&col0)[3]) {
    double unused[3];
    a.load(0, col0, unused);
}

// Row t + tau of the same atom for the thread's F (default kPmFrames) origin frames t = pm_frame(tb, f): fn(f, live, row) per frame, in
// frame order.  A float64 row is one 16-byte load at any t; two float32 rows share a 16-byte load when tau is even (origin
// frames 2 m, 2 m + 1 -> rows 2 m + tau, 2 m + tau + 1), an odd tau takes 8-byte loads.  A row at or past T reads row 0 and is
// not live: nothing is read at or past row T, but the second half of a float32 load at row T - 1 of an odd T, which lies
// inside the pitch.
template <int F = kPmFrames, class E, int D, class Fn>
__device__ __forceinline__ void pm_lagged(const PmAtom<E, D>& a, long T, long tb, long tau, Fn&& fn) {
    constexpr bool kF32 = PmAtom<E, D>::kF32;
    static_assert(F % 2 == 0, "a float32 load is two frames");
    if (kF32 && (tau & 1) == 0) {
#pragma unroll
        for (int f = 0; f < F; f += 2) {
            const long t2 = pm_frame<kF32>(tb, f) + tau;  // (even)
            double lo[3], hi[3];
            a.load(t2 < T ? t2 / 2 : 0, lo, hi);
            fn(f, t2 < T, lo);
            fn(f + 1, t2 + 1 < T, hi);
        }
    } else {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const long t2 = pm_frame<kF32>(tb, f) + tau;
            double lo[3];
            a.row(t2 < T ? t2 : 0, lo);
            fn(f, t2 < T, lo);
        }
    }
}

// A work unit is two consecutive items (atoms, compounds) of D columns: 2 D columns = D WHOLE destination pairs from
// dst on, so every store is a full 16-byte row and a wave's stores of one pair are contiguous along time.  A unit that
// holds one item (its v[D ...] are zeros) is n_out = ceil(D / 2) pairs, the phantom column of an odd D written as 0:
// nothing behind it is touched.  This is row t < pitch of a unit: the callers write every row of their frames, those
// >= T (live == false) as zeros.  (The loop over a thread's frames stays in the kernels: k_species_sort is at the
// SGPR limit with its plan, and with that loop in here two of its six instantiations came out one VGPR larger.)
template <int D>
__device__ __forceinline__ void pm_store_row(double2* dst, long pitch, long t, bool live, int n_out, const double (&v)[2 * D]) {
#pragma unroll
    for (int j = 0; j < D; ++j)
        if (j < n_out) dst[j * pitch + t] = live ? double2{v[2 * j], v[2 * j + 1]} : double2{0.0, 0.0};
}

// The grid of a kernel that walks units: (frame blocks of the pitch) x (groups of units), about sixteen workgroups per CU,
// at most one group per unit
inline dim3 pm_unit_grid(int n_cu, long pitch, long n_units) {
    const long n_tb = (pitch + kPmThreads * kPmFrames - 1) / (kPmThreads * kPmFrames);
    const long want = (16L * n_cu + n_tb - 1) / n_tb;
    return dim3((unsigned)n_tb, (unsigned)std::max(1L, std::min({want, n_units, 65535L})));
}


// ---- the host side of the launchers --------------------------------------------------------------------------------------
// What every launcher of a kernel that reads a staged slab through PmAtom asks of it
inline bool pm_slab_ok(long pitch, long T, long n_atoms, int D) {
    return D >= 1 && D <= 3 && n_atoms >= 1 && n_atoms * D < (1L << 31) && !(pitch & 7) && T >= 1 && T <= pitch;
}

// the lags of a host-facing call (int64) as the kernels read them
inline const long* pm_lags(const int64_t* lags) {
    static_assert(sizeof(long) == sizeof(int64_t), "lags are read as long");
    return reinterpret_cast<const long*>(lags);
}

// fn(std::integral_constant<int, v>) for a runtime v in [Lo, Hi] (checked by the caller: anything else takes Hi)
template <int Lo, int Hi, class Fn>
auto pm_switch(int v, Fn&& fn) {
    if constexpr (Lo == Hi) return fn(std::integral_constant<int, Lo>{});
    else return v == Lo ? fn(std::integral_constant<int, Lo>{}) : pm_switch<Lo + 1, Hi>(v, fn);
}
// fn(E()) for a slab's runtime element type, float32 or float64 ...
template <class Fn>
auto pm_element(bool f32, Fn&& fn) {
    return f32 ? fn(float()) : fn(double());
}
// ... and fn(E(), std::integral_constant<int, D>) with its dim 1 ... 3 as well: the kernel's <E, D> in the one launch line of a
// generic lambda
template <class Fn>
auto pm_dispatch(bool f32, int D, Fn&& fn) {
    return pm_element(f32, [&](auto e) { return pm_switch<1, 3>(D, [&](auto d) { return fn(e, d); }); });
}

}  // namespace ta
