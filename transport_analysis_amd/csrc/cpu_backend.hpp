// cpu_backend.hpp — the opt-in CPU backend (cpu_backend.cpp) as api.hip sees it
#pragma once
#include <cstdint>
#include <vector>

namespace ta {
struct BoxTable;  // unwrap_box.hpp
struct BondCuts;  // bond_math.hpp
namespace cpu {

struct State {
    int64_t T = 0, A = 0;
    int D = 0, dtype = 0, threads = 1;
    std::vector<void*> slabs;  // (n_frames, n_atoms, dim) host slabs, float32 or float64 elements (owned by the context)
};

bool supported();        // the build targets AVX2 + FMA
int hardware_threads();  // OpenMP's default team size
// slab `slab` = columns [col_offset, col_offset + n_atoms dim) of the synthetic tensor of ta_stage_synth
void synth(const State& s, int slab, unsigned long long seed, int64_t col_offset, int64_t n_cols_total);
// timeseries: (n_frames,) SUMS over atoms; by_particle: (n_frames, n_atoms) or NULL.  Return TA_OK / TA_E_NOMEM.
int vacf_fft(const State& s, double* timeseries, double* by_particle);
int vacf_direct(const State& s, double* timeseries, double* by_particle);
int helfand(const State& s, const double* masses, double scale, double* timeseries, double* by_particle);
// Einstein MSD of slab 0 (the positions): fft = true by transforms of x - x[0] (S1 - 2 S2), false difference first
int msd(const State& s, bool fft, double* timeseries, double* by_particle);
// Einstein-Helfand conductivity of slab 0: moment (n_frames, dim) = sum_n q_n (x - x[0]); collective (or NULL) = the MSD lag
// sum of the moment; self_lagsum (or NULL) = sum_n q_n^2 MSD_n, both by msd() with the same fft
int conductivity(const State& s, bool fft, const double* charges, double* moment, double* collective, double* self_lagsum);
// Onsager: moments (n_species, n_frames, dim) = sum_{n: species[n] = s} w_n (x - x[0]) of slab 0 (w NULL: all 1; labels
// checked by the caller) and, with cross != NULL, onsager_cross of them
int onsager(const State& s, bool fft, int n_species, const int32_t* species, const double* w, double* moments, double* cross);
// cross (n_frames, S, S): C[k, i, j] = 1/4 (MSD(M_i + M_j) - MSD(M_i - M_j))[k] by ONE msd() call on the S^2 pseudo-particles
// M_i, M_i + M_j, M_i - M_j; lag 0 and every pair with an all-zero moment exactly 0
int onsager_cross(int threads, bool fft, const double* moments, int n_species, int64_t n_frames, int dim, double* cross);
// Green-Kubo: currents (n_species, n_frames, dim) = sum_{n: species[n] = s} w_n v of slab 0 (the velocities; nothing
// subtracted) and, with cross != NULL, current_cross of them
int current(const State& s, bool fft, int n_species, const int32_t* species, const double* w, double* currents, double* cross);
// cross (n_frames, S, S): C[k, i, j] = 1/4 (ACF(J_i + J_j) - ACF(J_i - J_j))[k] by ONE vacf call on the S^2 pseudo-particles;
// lag 0 is kept; every pair with an all-zero current exactly 0
int current_cross(int threads, bool fft, const double* currents, int n_species, int64_t n_frames, int dim, double* cross);
// species self terms: self (n_species, n_frames) = sum_{n: species[n] = s} w_n^2 f_n, f_n the by-particle MSD (msd_quantity) or
// VACF of slab 0: each species' atoms gathered in input order as w (x - x[0]) or w v into a float64 slab of their own, then
// msd() / vacf_fft() / vacf_direct() on it; counts (n_species) or NULL; a species without atoms: zeros
int species_self(const State& s, bool msd_quantity, bool fft, int n_species, const int32_t* species, const double* w,
                 double* self, int64_t* counts);
// ta_scatter: the intermediate scattering functions of slab 0 (the positions) for K wavevectors kvecs (K, dim) in rad per length
// unit, with scatter.hip's phase arithmetic (q = k / (2 pi); u = q . x by a product, then fma; r = u - rint(u); (cos, sin)(2 pi r)):
// per wavevector a float64 (n_frames, n_atoms, 2) slab, self (K, n_frames) = its vacf_fft / vacf_direct lag sums, density
// (K, n_frames, 2) = its plain sum in atom order, coll (K, n_frames) = scatter_collective of the density; each may be NULL
int scatter(const State& s, bool fft, int K, const double* kvecs, double* self, double* density, double* coll);
// coll (K, n_frames): the autocorrelations of the K densities (K, n_frames, 2), ONE by-particle vacf call on them as K atoms of dim 2
int scatter_collective(int threads, bool fft, const double* density, int K, int64_t n_frames, double* coll);
// ta_orient: the orientation columns of N vectors (index rows of 2 or 3 atoms of slab 0 by `mode`, dim 3) with orient_math.hpp's
// arithmetic, as orient.hip: OpenMP over frames, the frame-major (n_frames, N, 3) array of u and the (n_frames, 2 N, 3) array of
// Q's columns; c1, c2 (n_frames) = their vacf_fft / vacf_direct lag sums, total (n_frames, 3) = sum_n w_n u_n in vector order (w
// NULL: all 1), coll (n_frames) = the same evaluation of the total as one atom; each may be NULL.  box: NULL or the nine rows
// (H00 H10 H11 H20 H21 H22 M00 M11 M22) of tpitch doubles (tpitch 1: one constant box); arguments checked by the caller
int orient(const State& s, bool fft, int mode, int64_t N, const int32_t* index, const double* box, int64_t tpitch, const double* w,
           double* c1, double* c2, double* total, double* coll);
// ta_chain_modes: Q linear functionals (coeff (Q, N)) of C chains (members (C, N) atoms of slab 0, dim 3, in backbone order) with
// chain_math.hpp's sequence, as chain_modes.hip: OpenMP over chains, one frame-major (n_frames, C, 3) array per functional;
// acf (Q, n_frames) = their vacf_fft / vacf_direct lag sums, one evaluation per functional.  box, tpitch: as orient's
int chain_modes(const State& s, bool fft, int64_t C, int64_t N, const int32_t* members, int Q, const double* coeff, const double* box,
                int64_t tpitch, double* acf);
// ta_kcurrent: the k-space current of slab 0 (the velocities) and slab 1 (the positions) for K wavevectors kvecs (K, dim), with
// kcurrent.hip's arithmetic (the phase as scatter(); w_n v by a product, then one fma with the cosine and one with the sine):
// current (K, n_frames, dim, 2) = the plain sum in atom order (w NULL: all 1), lon / trans (K, n_frames) = kcurrent_correlate
// of it; each output may be NULL; arguments checked by the caller
int kcurrent(const State& s, bool fft, int K, const double* kvecs, const double* w, double* current, double* lon, double* trans);
// ta_partial_density: the species-resolved density of slab 0 (the positions) for K wavevectors, with species_density.hip's
// arithmetic (the phase as scatter(); one fma of w_n with the cosine and one with the sine): density (K, n_species, n_frames, 2)
// = the plain sum in atom order per species (labels in [0, n_species), checked by the caller; w NULL: all 1), cross (K,
// n_frames, S, S) = partial_cross of it (or NULL)
int partial_density(const State& s, bool fft, int K, const double* kvecs, int n_species, const int32_t* species, const double* w,
                    double* density, double* cross);
// cross (K, n_frames, S, S) of a density (K, S, n_frames, 2): current_cross on dim 2 per wavevector
int partial_cross(int threads, bool fft, const double* density, int K, int n_species, int64_t n_frames, double* cross);
// lon, trans (K, n_frames) of a current (K, n_frames, dim, 2): kcurrent_math.hpp's projections jL, jT_d as K (1 + dim) atoms
// of dim 2 (dim = 1: K), ONE by-particle vacf call on them, the transverse series added and divided by dim - 1 (dim = 1: zeros)
int kcurrent_correlate(int threads, bool fft, const double* current, int K, const double* kvecs, int64_t n_frames, int dim,
                       double* lon, double* trans);
// ta_vanhove: the self van Hove histogram of slab 0 (the positions) for L strictly increasing lags, B bins of width dr, with
// vanhove_math.hpp's arithmetic (r2 by a product, then fma; the squared-edge table; the bin of the definition), as
// vanhove.hip: counts (L, B + 1) int64 (OpenMP over atoms, a histogram per thread, added at the end), moments (L, 2) = (sum r2,
// sum r2 r2) per atom, then in atom order; either may be NULL; arguments checked by the caller
int vanhove(const State& s, int L, const int64_t* lags, int B, double dr, int64_t* counts, double* moments);
// ta_overlap: the self-overlap per origin of slab 0 for L lags and C cutoffs, with vanhove_math.hpp's r2 and a2 = fl(a a), as
// overlap.hip: q (C, L, T) int64, zeros at t0 >= T - lag.  OpenMP over the (lag, origin) pairs, each counted over all atoms by
// one thread: no per-thread copies of q, and nothing depends on the number of threads.
int overlap(const State& s, int L, const int64_t* lags, int C, const double* cutoffs, int64_t* q);
// ta_overlap_density: the overlap field's density per origin of slab 0 for K wavevectors, L lags and C cutoffs, with the r2 and
// a2 of ta_overlap and overlap_density.hip's phase expression of the origin frame: w (K, C, L, T, 2), +0.0 at t0 >= T - lag.
// OpenMP over the (lag, origin) pairs, each a plain sum in atom order: nothing depends on the number of threads.
int overlap_density(const State& s, int K, const double* kvecs, int L, const int64_t* lags, int C, const double* cutoffs, double* w);
// ta_vanhove_distinct: the distinct van Hove histogram of slab 0 with vanhove_distinct_math.hpp's arithmetic, as
// vanhove_distinct.hip: counts (L, B + 1) int64 over the ordered pairs (ida[p], idb[q]), ida[p] != idb[q], of the origins
// t = stride o and the lags with t + lag < n_frames (OpenMP over (origin, a-tile), a histogram per thread, added at the end).
// hm: NULL (no box) or H[3], M[3] of the staged columns per box (one, or per_frame: one per frame); arguments checked by
// the caller
int vanhove_distinct(const State& s, int L, const int64_t* lags, int64_t stride, int64_t n_a, const int32_t* ida, int64_t n_b,
                     const int32_t* idb, const double* hm, bool per_frame, int B, double dr, int64_t* counts);
// ta_pair_find: the pairs (ida[p], idb[q]) of different items of slab 0 that are closer than sqrt(rc2) in at least one of the
// frames t = stride o, with pair_math.hpp's arithmetic, as pair_lifetime.hip: *pairs = the list (n, 2) sorted by (a, b); same:
// b is a, only q > p is listed.  OpenMP over the a-items, each of which owns its row of the bitmap.  hm as vanhove_distinct's.
int pair_find(const State& s, int64_t n_a, const int32_t* ida, int64_t n_b, const int32_t* idb, bool same, int64_t stride,
              const double* hm, bool per_frame, double rc2, std::vector<int32_t>* pairs);
// ta_pair_lifetime: of the P atom pairs `pairs` (P, 2) of slab 0 with the indicator h of pair_math.hpp: ci (T) = sum over pairs and
// t < T - tau of h(t) h(t + tau) (fft false: popcounts of the packed series, exact integers; fft true: the FFT lag sums of the
// indicator array, times T - tau), runs (T + 1) = the histogram of the lengths of the maximal runs of bonded frames, nb (T) =
// the bonded pairs per frame; each may be NULL.  OpenMP over pairs, integer sums per thread, added at the end: nothing
// depends on the number of threads.
int pair_lifetime(const State& s, bool fft, int64_t P, const int32_t* pairs, const double* hm, bool per_frame, double rc2, double* ci,
                  int64_t* runs, double* nb);
// ta_bond_lifetime: the same three sums of the series g of the P bonds `atoms` (P, n_at), n_at = 2 or 3, with bond_math.hpp's
// level, hysteresis and closing of absences of up to `gap` frames on the packed words, as k_bond_series and k_pair_filter
int bond_lifetime(const State& s, bool fft, int64_t P, int n_at, const int32_t* atoms, const double* hm, bool per_frame,
                  const BondCuts& cuts, int gap, double* ci, int64_t* runs, double* nb);
// What the three shell calls share: the reference items ida and the observed items idb, hm and per_frame as
// vanhove_distinct's, the squared form and break radii (cuts->rc2, cuts->rb2) and the tolerated absence in frames
struct ShellItems {
    int64_t n_a;
    const int32_t* ida;
    int64_t n_b;
    const int32_t* idb;
    const double* hm;
    bool per_frame;
    const BondCuts* cuts;
    int gap;
};
// ta_shell_residence: the same three sums of the n_b series of the observed items idb against ALL reference items ida (one
// with the observed item's own id does not count): bond_math.hpp's shell_level of "some reference item closer than
// sqrt(rc2)" / "... sqrt(rb2)", then bond_lifetime's filters, as k_shell_series and k_pair_filter.  OpenMP over observed items.
int shell_residence(const State& s, bool fft, const ShellItems& c, double* ci, int64_t* runs, double* nb);
// ta_shell_msd: shell_residence's series g, its runs and nb, and sums (max_lag + 1, D), count (max_lag + 1): the squared
// displacements of the observed items over the lags 0 ... max_lag, gated by g under `condition` (shell_msd_math.hpp, as
// k_shell_msd: the same term and gates); any output may be NULL.  OpenMP over observed items.
int shell_msd(const State& s, int condition, int64_t max_lag, const ShellItems& c, double* sums, int64_t* count, int64_t* runs, double* nb);
// ta_shell_orient: shell_msd's gated sums with shell_orient_math.hpp's term in place of the squared displacement: sums
// (max_lag + 1, 2) = (sum c, sum c c), c = u(t) . u(t + k), u the unit vector of index row n (orient_row_len(mode) atoms of slab 0,
// dim 3; orient_math.hpp's sequence with hm as the image step's box), gated by the series of observed item n, the row's anchor
int shell_orient(const State& s, int condition, int64_t max_lag, int mode, const int32_t* index, const ShellItems& c, double* sums,
                 int64_t* count, int64_t* runs, double* nb);
// ta_compound: out (n_frames, n_compounds, dim) float64 = sum_{i in [offsets[c], offsets[c + 1])} w_i x[t, members[i], d] -
// g_c F[t, d] of slab 0 (g_c = sum_i w_i, F = sum_a u_a x[t, a, d]; frame_weights NULL: no such term; weights NULL: all 1),
// the sum in member order (the first product, then fma), parallel over compounds; arguments checked by the caller
int compound(const State& s, int64_t n_compounds, const int64_t* offsets, const int32_t* members, const double* weights,
             const double* frame_weights, double* out);
// ta_unwrap on host slab `slab` in place (box, axes checked by the caller)
void unwrap(const State& s, int slab, const BoxTable& box, const int* axes);

}  // namespace cpu
}  // namespace ta
