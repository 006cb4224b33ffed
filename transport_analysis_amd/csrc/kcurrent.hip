// kcurrent.hip — the k-space current of the longitudinal and transverse current correlation functions C_L(k, t), C_T(k, t).
//
//   current[j, t, d] = ( sum_n w_n v[t, n, d] cos phi_j[t, n],  sum_n w_n v[t, n, d] sin phi_j[t, n] ),   phi_j = k_j . x
//
// in ONE pass over both staged slabs (slab 0 = velocities, slab 1 = positions) per chunk of wavevectors: k_kcurrent reduces
// over atoms in registers and writes partial sums per group of atoms, which k_sum_partials adds in a fixed order (no
// atomics: the same bits from run to run).  Nothing of the size of a slab is written.  The phase is phase_math.hpp's, the
// one k_phase (scatter.hip) forms; every accumulator is then updated by one fma of (w_n v) with the cosine and one with the
// sine.  k_kcurrent_project and k_kcurrent_finish are the two ends of the correlation
// (kcurrent_math.hpp; api.hip: kcurrent_correlation).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "kcurrent_math.hpp"
#include "phase_math.hpp"
#include "pm_read.hpp"
#include "ta_internal.hpp"

namespace ta {
namespace {

// The tile: KC wavevectors x F frames per thread, D complex sums each, in registers.  ONE tile is shipped; the macros let
// tools/bench_kcurrent.py build the other candidates (DESIGN.md section 4.17 records the comparison).  A float32 load
// delivers two frames, so a float32 slab is read with an even F.
#ifndef TA_KCURRENT_KC
#define TA_KCURRENT_KC 4
#endif
#ifndef TA_KCURRENT_F
#define TA_KCURRENT_F 2
#endif
constexpr int kKC = TA_KCURRENT_KC, kF = TA_KCURRENT_F;
static_assert(kKC >= 1 && kKC <= 8 && (kF == 1 || kF == 2), "candidate tiles: KC in 1 ... 8, F in {1, 2}");
template <class E>
constexpr int kFramesOf = std::is_same_v<E, float> ? 2 : kF;

// Workgroup (bx, g): frames [256 F bx, 256 F (bx + 1)), atoms g, g + G, ... (G = gridDim.y).  A thread owns F frames
// (pm_frame) and keeps, for the chunk's kc <= KC wavevectors, their D complex sums in registers across the atoms.  Each atom
// is read ONCE from both slabs, as the whole source pairs that cover its D columns, in the slab's element type (a float32
// row pair in one 16-byte load, widened in registers); a load that would start at or past row T reads row 0 and its sums
// are never stored (pm_read.hpp).  q[j D + d] and w[n] have workgroup-uniform addresses: plain loads.  A slot jl >= kc does
// its arithmetic on wavevector 0 and stores nothing.  partial[g][jl][t][d] = (re, im), 16-byte rows, jl < kc, t < T.
template <class E, int D, int KC>
__global__ void __launch_bounds__(kPmThreads)
    k_kcurrent(const E* __restrict__ v, const E* __restrict__ x, long pitch, long T, int n_atoms, const double* __restrict__ q,
               int kc, const double* __restrict__ w, double* __restrict__ partial) {
    constexpr bool kF32 = std::is_same_v<E, float>;
    constexpr int F = kFramesOf<E>;
    constexpr int L = kF32 ? F / 2 : F;  // 16-byte loads per thread, slab and atom
    const long tb = (long)blockIdx.x * (kPmThreads * F);
    double are[KC][F][D], aim[KC][F][D];
#pragma unroll
    for (int jl = 0; jl < KC; ++jl)
#pragma unroll
        for (int f = 0; f < F; ++f)
#pragma unroll
            for (int d = 0; d < D; ++d) are[jl][f][d] = 0.0, aim[jl][f][d] = 0.0;
    for (int n = blockIdx.y; n < n_atoms; n += gridDim.y) {
        double vel[F][3], pos[F][3];
        const PmAtom<E, D> av(v, pitch, (unsigned)n), ax(x, pitch, (unsigned)n);  // (atom D < 2^31: launch_kcurrent)
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const int f = kF32 ? 2 * l : l;
            const long t = pm_frame<kF32>(tb, f);  // (float32: even)
            const long i = t < T ? (kF32 ? t / 2 : t) : 0;
            av.load(i, vel[f], vel[kF32 ? f + 1 : f]);
            ax.load(i, pos[f], pos[kF32 ? f + 1 : f]);
        }
        const double wn = w ? w[n] : 1.0;
#pragma unroll
        for (int f = 0; f < F; ++f)
#pragma unroll
            for (int d = 0; d < D; ++d) vel[f][d] = wn * vel[f][d];
#pragma unroll
        for (int jl = 0; jl < KC; ++jl) {
            const int j = jl < kc ? jl : 0;
            const double q0 = q[j * D], q1 = D > 1 ? q[j * D + 1] : 0.0, q2 = D > 2 ? q[j * D + 2] : 0.0;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const double2 cs = phase_cs<D>(q0, q1, q2, pos[f]);
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    are[jl][f][d] = fma(vel[f][d], cs.x, are[jl][f][d]);
                    aim[jl][f][d] = fma(vel[f][d], cs.y, aim[jl][f][d]);
                }
            }
        }
    }
    double2* out = reinterpret_cast<double2*>(partial) + (long)blockIdx.y * kc * T * D;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const long t = pm_frame<kF32>(tb, f);
        if (t >= T) continue;
#pragma unroll
        for (int jl = 0; jl < KC; ++jl) {
            if (jl >= kc) continue;
#pragma unroll
            for (int d = 0; d < D; ++d) out[((long)jl * T + t) * D + d] = double2{are[jl][f][d], aim[jl][f][d]};
        }
    }
}

// One thread per (row t < pitch, wavevector j): the kcur_series(D) pseudo-atoms of wavevector j -- jL, then the D components
// of jT (D > 1) -- as pairs j S + c of a pair-major slab of K S "atoms" with dim 2 (S = kcur_series(D)); rows T ... pitch - 1
// are zeros (the workspace is reused).  current (K, T, D, 2), khat (K, D).
__global__ void k_kcurrent_project(const double* __restrict__ current, const double* __restrict__ khat, int K, long T, int D,
                                   long pitch, double* __restrict__ pm) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (t >= pitch || j >= K) return;
    const int S = kcur_series(D);
    double out[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (t < T) {
        double cur[6], kh[3];
        for (int d = 0; d < D; ++d) {
            kh[d] = khat[(long)j * D + d];
            cur[2 * d] = current[(((long)j * T + t) * D + d) * 2];
            cur[2 * d + 1] = current[(((long)j * T + t) * D + d) * 2 + 1];
        }
        kcur_project(D, kh, cur, out);
    }
    double2* dst = reinterpret_cast<double2*>(pm) + (long)j * S * pitch + t;
    for (int c = 0; c < S; ++c) dst[c * pitch] = double2{out[2 * c], out[2 * c + 1]};
}

// (T, K S) by-particle autocorrelations of the pseudo-atoms -> lon (K, T), trans (K, T) (either may be NULL); D = 1: trans
// is written as zeros
__global__ void k_kcurrent_finish(const double* __restrict__ bp, int K, long T, int D, double* __restrict__ lon,
                                  double* __restrict__ trans) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * K) return;
    const long j = i / T, t = i - j * T;
    const int S = kcur_series(D);
    double row[4], l, tr;
    for (int c = 0; c < S; ++c) row[c] = bp[t * ((long)K * S) + j * S + c];
    kcur_finish(D, row, &l, &tr);
    if (lon) lon[i] = l;
    if (trans) trans[i] = tr;
}

long kcurrent_blocks(bool f32, long pitch) {
    const long fpb = (long)kPmThreads * (f32 ? kFramesOf<float> : kFramesOf<double>);
    return (pitch + fpb - 1) / fpb;
}

}  // namespace

void kcurrent_tile(int* kc, int* frames_f64, int* frames_f32) {
    *kc = kKC, *frames_f64 = kFramesOf<double>, *frames_f32 = kFramesOf<float>;
}

int kcurrent_parts(int n_cu, bool f32, long pitch, long n_atoms, int D, size_t budget) {
    // about eight workgroups per CU over the frame blocks (three waves per SIMD are resident: two to three rounds), at most
    // one group per atom, and no more than the partial buffer's budget holds: G KC pitch D 16 bytes
    const long n_tb = kcurrent_blocks(f32, pitch);
    const long want = (8L * n_cu + n_tb - 1) / n_tb;
    const long fit = (long)(budget / ((size_t)kKC * (size_t)pitch * (size_t)D * 16));
    return (int)std::max(1L, std::min({want, n_atoms, fit, 65535L}));
}

hipError_t launch_kcurrent(const void* v, const void* x, bool f32, long pitch, long T, long n_atoms, int D, const double* q,
                           int kc, const double* w, double* partial, int n_parts, hipStream_t st) {
    if (!pm_slab_ok(pitch, T, n_atoms, D) || kc < 1 || kc > kKC || n_parts < 1 || n_parts > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)kcurrent_blocks(f32, pitch), (unsigned)n_parts);
    pm_dispatch(f32, D, [&](auto e, auto d) {
        using E = decltype(e);
        hipLaunchKernelGGL((k_kcurrent<E, d(), kKC>), grid, dim3(kPmThreads), 0, st, (const E*)v, (const E*)x, pitch, T, (int)n_atoms,
                           q, kc, w, partial);
    });
    return hipGetLastError();
}

hipError_t launch_kcurrent_project(const double* current, const double* khat, int K, long T, int D, long pitch, double* pm,
                                   hipStream_t st) {
    hipLaunchKernelGGL(k_kcurrent_project, dim3((unsigned)((pitch + 255) / 256), (unsigned)K), dim3(256), 0, st, current, khat, K,
                       T, D, pitch, pm);
    return hipGetLastError();
}

hipError_t launch_kcurrent_finish(const double* bp, int K, long T, int D, double* lon, double* trans, hipStream_t st) {
    const long n = T * K;
    hipLaunchKernelGGL(k_kcurrent_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bp, K, T, D, lon, trans);
    return hipGetLastError();
}

}  // namespace ta
