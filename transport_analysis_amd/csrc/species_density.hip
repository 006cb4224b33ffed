// species_density.hip — the species-resolved density of the partial intermediate scattering functions F_ab(k, t), S_ab(k).
//
//   rho[j, a, t] = sum_{n: species[n] = a} w_n (cos, sin)(k_j . x[t, n, :])
//
// in ONE pass over the staged position slab (slab 0) per chunk of wavevectors: k_species_density is k_kcurrent (kcurrent.hip)
// without the velocity slab and with the sum split by a per-atom label.  It reduces over atoms in registers and writes
// partial sums per group of atoms, which k_sum_partials adds in a fixed order (no atomics: the same bits from run to run).
// Nothing of the size of a slab is written.  The phase is phase_math.hpp's, the one k_phase (scatter.hip) and k_kcurrent
// form; the accumulator of the atom's species is then updated by one fma of w_n with the cosine and one with the sine.
// k_partial_finish is the far end of the cross term (api.hip: partial_cross): k_cross_finish (species_sum.hip) over a batch
// of wavevectors whose pseudo-particles share ONE by-particle evaluation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "phase_math.hpp"
#include "pm_read.hpp"
#include "ta_internal.hpp"

namespace ta {
namespace {

// The tile: ST species slots x KC wavevectors x F frames per thread, one complex sum each, in registers.  ONE tile is
// shipped per ST in {1, 2, 4, 8} (the smallest that holds the call's species); DESIGN.md section 4.22 records why these.
// A float32 load delivers two frames, so a float32 slab is read with an even F.
struct SdTile {
    int st, kc;
};
constexpr SdTile kSdTiles[] = {{1, 8}, {2, 8}, {4, 4}, {8, 2}};
constexpr int kSdF64 = 1, kSdF32 = 2;
constexpr int kSdSlots = 16;  // ST KC at most: it sizes the partial buffer's rows whatever the tile
template <class E>
constexpr int kSdFramesOf = std::is_same_v<E, float> ? kSdF32 : kSdF64;
static_assert(kSdF32 % 2 == 0, "a float32 load is two frames");

constexpr int sd_slots(int S) { return S <= 1 ? 1 : S <= 2 ? 2 : S <= 4 ? 4 : 8; }
constexpr int sd_kc(int st) { return st == 1 ? kSdTiles[0].kc : st == 2 ? kSdTiles[1].kc : st == 4 ? kSdTiles[2].kc : kSdTiles[3].kc; }
static_assert(sd_kc(1) <= kSdSlots && 2 * sd_kc(2) <= kSdSlots && 4 * sd_kc(4) <= kSdSlots && 8 * sd_kc(8) <= kSdSlots, "ST KC <= 16");

// Workgroup (bx, g): frames [256 F bx, 256 F (bx + 1)), atoms g, g + G, ... (G = gridDim.y).  A thread owns F frames
// (pm_frame) and keeps, for the chunk's kc <= KC wavevectors and the ST species slots, one complex sum each in registers
// across the atoms.  Each atom is read ONCE, as the whole source pairs that cover its D columns, in the slab's element type
// (a float32 row pair in one 16-byte load, widened in registers); a load that would start at or past row T reads row 0 and
// its sums are never stored (pm_read.hpp).  q[j D + d], species[n] and w[n] have workgroup-uniform addresses: plain loads,
// and the accumulator is picked by a uniform branch over the unrolled slots -- never by a runtime index into the register
// arrays.  A label outside [0, ST) selects nothing (the host-facing calls reject labels outside [0, S) before they get
// here).  A slot jl >= kc does its arithmetic on wavevector 0 and stores nothing; a species slot a >= S stores nothing.
// partial[g][jl][a][t] = (re, im), 16-byte rows, jl < kc, a < S, t < T.
template <class E, int D, int ST, int KC>
__global__ void __launch_bounds__(kPmThreads)
    k_species_density(const E* __restrict__ x, long pitch, long T, int n_atoms, const double* __restrict__ q, int kc, int S,
                      const int* __restrict__ species, const double* __restrict__ w, double* __restrict__ partial) {
    constexpr bool kF32 = std::is_same_v<E, float>;
    constexpr int F = kSdFramesOf<E>;
    constexpr int L = kF32 ? F / 2 : F;  // 16-byte loads per thread and atom
    const long tb = (long)blockIdx.x * (kPmThreads * F);
    double are[ST][KC][F], aim[ST][KC][F];
#pragma unroll
    for (int a = 0; a < ST; ++a)
#pragma unroll
        for (int jl = 0; jl < KC; ++jl)
#pragma unroll
            for (int f = 0; f < F; ++f) are[a][jl][f] = 0.0, aim[a][jl][f] = 0.0;
    for (int n = blockIdx.y; n < n_atoms; n += gridDim.y) {
        double pos[F][3];
        const PmAtom<E, D> ax(x, pitch, (unsigned)n);  // (atom D < 2^31: launch_species_density)
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const int f = kF32 ? 2 * l : l;
            const long t = pm_frame<kF32>(tb, f);  // (float32: even)
            const long i = t < T ? (kF32 ? t / 2 : t) : 0;
            ax.load(i, pos[f], pos[kF32 ? f + 1 : f]);
        }
        const int lab = __builtin_amdgcn_readfirstlane(species[n]);
        const double wn = w ? w[n] : 1.0;
#pragma unroll
        for (int jl = 0; jl < KC; ++jl) {
            const int j = jl < kc ? jl : 0;
            const double q0 = q[j * D], q1 = D > 1 ? q[j * D + 1] : 0.0, q2 = D > 2 ? q[j * D + 2] : 0.0;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const double2 cs = phase_cs<D>(q0, q1, q2, pos[f]);
#pragma unroll
                for (int a = 0; a < ST; ++a)
                    if (lab == a) {
                        are[a][jl][f] = fma(wn, cs.x, are[a][jl][f]);
                        aim[a][jl][f] = fma(wn, cs.y, aim[a][jl][f]);
                    }
            }
        }
    }
    double2* out = reinterpret_cast<double2*>(partial) + (long)blockIdx.y * kc * S * T;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const long t = pm_frame<kF32>(tb, f);
        if (t >= T) continue;
#pragma unroll
        for (int jl = 0; jl < KC; ++jl) {
            if (jl >= kc) continue;
#pragma unroll
            for (int a = 0; a < ST; ++a)
                if (a < S) out[((long)jl * S + a) * T + t] = double2{are[a][jl][f], aim[a][jl][f]};
        }
    }
}

// k_cross_finish (species_sum.hip) over a batch of B wavevectors: bp (T, B S^2) holds the by-particle autocorrelations of the
// batch's pseudo-particles (wavevector b's at columns b S^2 ...), nz (B, TA_ONSAGER_MAX_SPECIES) their non-zero flags.
// C (B, T, S, S): the diagonal is R(rho_a) itself, off it 1/4 (R(rho_a + rho_b) - R(rho_a - rho_b)) with the same bits in
// both triangles; every pair with an all-zero density is exactly 0; lag 0 is kept.
__global__ void k_partial_finish(const double* __restrict__ bp, int B, int S, long T, const int* __restrict__ nz,
                                 double* __restrict__ C) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (idx >= T * S * S || b >= B) return;
    const long k = idx / (S * S);
    const int i = (int)(idx % (S * S)) / S, j = (int)(idx % (S * S)) % S;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const int* z = nz + (long)b * TA_ONSAGER_MAX_SPECIES;
    double c = 0.0;
    if (z[i] && z[j]) {
        const double* row = bp + (k * B + b) * (long)S * S;
        c = i == j ? row[i * S + i] : 0.25 * (row[lo * S + hi] - row[hi * S + lo]);
    }
    C[(long)b * T * S * S + idx] = c;
}

long sd_blocks(bool f32, long pitch) {
    const long fpb = (long)kPmThreads * (f32 ? kSdF32 : kSdF64);
    return (pitch + fpb - 1) / fpb;
}

}  // namespace

bool species_density_tile(int n_species, int* st, int* kc, int* frames_f64, int* frames_f32) {
    if (n_species < 1 || n_species > TA_ONSAGER_MAX_SPECIES) return false;
    *st = sd_slots(n_species), *kc = sd_kc(*st), *frames_f64 = kSdF64, *frames_f32 = kSdF32;
    return true;
}

int species_density_parts(int n_cu, bool f32, long pitch, long n_atoms, size_t budget) {
    // as kcurrent_parts: about eight workgroups per CU over the frame blocks, at most one group per atom, and no more than
    // the partial buffer's budget holds: G (ST KC <= 16) pitch 16 bytes.  Nothing here depends on the species or the chunk.
    const long n_tb = sd_blocks(f32, pitch);
    const long want = (8L * n_cu + n_tb - 1) / n_tb;
    const long fit = (long)(budget / ((size_t)kSdSlots * (size_t)pitch * 16));
    return (int)std::max(1L, std::min({want, n_atoms, fit, 65535L}));
}

hipError_t launch_species_density(const void* x, bool f32, long pitch, long T, long n_atoms, int D, const double* q, int kc, int S,
                                  const int* species, const double* w, double* partial, int n_parts, hipStream_t st) {
    int ST = 0, KC = 0, f64 = 0, f32f = 0;
    if (!species_density_tile(S, &ST, &KC, &f64, &f32f) || !pm_slab_ok(pitch, T, n_atoms, D) || kc < 1 || kc > KC || n_parts < 1 ||
        n_parts > 65535 || !species)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)sd_blocks(f32, pitch), (unsigned)n_parts);
    pm_dispatch(f32, D, [&](auto e, auto d) {
        using E = decltype(e);
        auto go = [&](auto slots) {
            constexpr int kSt = decltype(slots)::value;
            hipLaunchKernelGGL((k_species_density<E, d(), kSt, sd_kc(kSt)>), grid, dim3(kPmThreads), 0, st, (const E*)x, pitch, T,
                               (int)n_atoms, q, kc, S, species, w, partial);
        };
        if (ST == 1) go(std::integral_constant<int, 1>{});
        else if (ST == 2) go(std::integral_constant<int, 2>{});
        else if (ST == 4) go(std::integral_constant<int, 4>{});
        else go(std::integral_constant<int, 8>{});
    });
    return hipGetLastError();
}

hipError_t launch_partial_finish(const double* bp, int B, int S, long T, const int* nz, double* C, hipStream_t st) {
    const long n = T * S * S;
    hipLaunchKernelGGL(k_partial_finish, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, st, bp, B, S, T, nz, C);
    return hipGetLastError();
}

}  // namespace ta
