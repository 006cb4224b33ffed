// shell_orient.hip — the kernel of the shell-resolved reorientation (include/ta_hip.h, ta_shell_orient): C_1 and C_2 sums of
// molecule-fixed unit vectors over the lags 0 ... L, every term gated by bits of ta_shell_residence's 0/1 series g of the
// vector's anchor atom.  shell_orient_math.hpp has the arithmetic, which the CPU backend follows.
//
//   k_shell_orient<E, MODE, BOX, COND>   shell_gate_walk (shell_gate.hpp: the chunks, the words in LDS, the two gates, the
//                               partial rows), the second instantiation next to k_shell_msd.  Its Source forms u where the MSD
//                               reads a row: the vector's 2 or 3 atoms of frame t (the index row at a workgroup-uniform
//                               address) through PmAtom<E, 3>::row, a float32 slab as float32, widened in registers; the image
//                               step with frame t's box of the distance pass (a constant box: scalar values; per-frame boxes:
//                               read by the lane for its frame); orient_combine, orient_unit.  u is kept in LDS as float64,
//                               3 (C + 256) doubles.  No block of u is ever written: a chunk without a frame inside costs its
//                               words alone.  The Term is c = u . u', s1 += c, s2 = fma(c, c, s2).
// k_shell_bits in front and k_shell_fold (D = 2) behind are shell_msd.hip's.  No atomics: repeat runs give the same bits.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pm_read.hpp"
#include "shell_gate.hpp"
#include "shell_orient_math.hpp"

namespace ta {
namespace {

enum { BOX_NONE = 0, BOX_CONST = 1, BOX_FRAME = 2 };

template <class E, int MODE, int BOX>
struct ShellOrientSource {
    static constexpr int NV = 3;
    using Kept = double;
    PmAtom<E, 3> a, b, c;  // (a bond: c is b, not read)
    const double* hm;      // H[3], M[3] per box
    __device__ __forceinline__ void load(long t, double (&u)[3]) const {
        double pa[3], pb[3], pc[3] = {0.0, 0.0, 0.0};
        a.row(t, pa);
        b.row(t, pb);
        if constexpr (MODE != ORIENT_BOND) c.row(t, pc);
        OrientBox bx{};
        if constexpr (BOX != BOX_NONE) bx = shell_orient_box(hm + (BOX == BOX_FRAME ? 6 * t : 0));
        shell_orient_unit<MODE, BOX != BOX_NONE>(pa, pb, pc, bx, u);
    }
};

struct ShellOrientTerm {
    static constexpr int NS = 2;
    template <class A, class B>
    static __device__ __forceinline__ void add(double (&acc)[2], bool gate, A&& origin, B&& lagged) {
        const double c = shell_orient_dot(origin(0), origin(1), origin(2), lagged(0), lagged(1), lagged(2));
        if (gate) shell_orient_add(acc[0], acc[1], c);
    }
};

// x: the staged slab (D = 3); index: the block's rows of K = 2 | 3 atoms, one per observed item; hm: the boxes; the rest as
// shell_gate_walk's
template <class E, int MODE, int BOX, int COND>
__global__ void __launch_bounds__(kPmThreads)
    k_shell_orient(const E* __restrict__ x, long pitch, long T, const int* __restrict__ index, long n_items,
                   const unsigned long long* __restrict__ words, long nw, int C, const double* __restrict__ hm,
                   double* __restrict__ part_s, unsigned long long* __restrict__ part_n) {
    constexpr int K = MODE == ORIENT_BOND ? 2 : 3;
    shell_gate_walk<COND, ShellOrientTerm>(T, n_items, words, nw, C, part_s, part_n, [&](long q) {
        const int* r = index + q * K;
        return ShellOrientSource<E, MODE, BOX>{PmAtom<E, 3>(x, pitch, (unsigned)r[0]), PmAtom<E, 3>(x, pitch, (unsigned)r[1]),
                                               PmAtom<E, 3>(x, pitch, (unsigned)r[K - 1]), hm};
    });
}

}  // namespace

hipError_t launch_shell_orient(const void* x, bool f32, long pitch, long T, long n_atoms, int D, int mode, const int* index, long n_items,
                               const double* hm, bool per_frame, const unsigned long long* words, int condition, long max_lag, int chunk,
                               int G, void* part, hipStream_t st) {
    const long n_pass = max_lag / kSmLags + 1;
    if (D != 3 || !pm_slab_ok(pitch, T, n_atoms, D) || n_items < 1 || n_items >= (1L << 30) || max_lag < 0 || max_lag > kShellMsdMaxLag ||
        max_lag >= T || chunk < 64 || chunk > 1024 || chunk % 64 || G < 1 || G > n_items ||
        (condition != SHELL_CONTINUOUS && condition != SHELL_ENDPOINTS) || mode < ORIENT_BOND || mode > ORIENT_NORMAL || !x || !index || !words ||
        !part)
        return hipErrorInvalidValue;
    const size_t lds = shell_gate_lds_bytes(chunk, (int)n_pass, 3, sizeof(double));
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    double* part_s = (double*)part;
    unsigned long long* part_n = (unsigned long long*)(part_s + (size_t)G * (size_t)(n_pass * kSmLags) * 2);
    // <MODE, BOX, COND> as one variant number for the switch
    static_assert(ORIENT_BOND == 0 && ORIENT_NORMAL == 2 && BOX_NONE == 0 && BOX_FRAME == 2 && SHELL_CONTINUOUS == 0 && SHELL_ENDPOINTS == 1,
                  "the variant's digits");
    const int variant = (mode * 3 + (!hm ? BOX_NONE : per_frame ? BOX_FRAME : BOX_CONST)) * 2 + condition;
    pm_element(f32, [&](auto e) {
        pm_switch<0, 17>(variant, [&](auto v) {
            using E = decltype(e);
            constexpr int c = decltype(v)::value;
            hipLaunchKernelGGL((k_shell_orient<E, c / 6, c / 2 % 3, c % 2>), dim3((unsigned)G, (unsigned)n_pass), dim3(kPmThreads), lds, st,
                               (const E*)x, pitch, T, index, n_items, words, (T + 63) / 64, chunk, hm, part_s, part_n);
        });
    });
    return hipGetLastError();
}

}  // namespace ta
