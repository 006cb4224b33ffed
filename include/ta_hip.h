/* ta_hip.h — C-ABI of the MI355X time-correlation library (libta_hip.so).
 *
 * This is the drop-in boundary for transport-analysis's time-correlation hot
 * path.  The reference has no native seam of its own (it is pure Python); the
 * entry points below are what a ctypes binding inside the reference's
 * `_prepare` / `_single_frame` / `_conclude` hooks calls, and each one cites
 * the reference code it replaces (paths relative to
 * /root/reference/transport_analysis).  See INTEGRATION.md for the binding.
 *
 * Conventions
 *   - every call returns int: 0 = TA_OK, negative = error (TA_E_*);
 *     ta_last_error() returns a human-readable message for the last failure
 *     on that context (or on the calling thread when ctx is NULL).
 *   - no C++ exception crosses this boundary: every entry point's body runs inside a catch-all
 *     (ta::guard, csrc/ta_internal.hpp); std::bad_alloc comes back as TA_E_NOMEM, any other
 *     exception as TA_E_HIP, both with a message; work already queued on behalf of the call is
 *     drained first, so the caller may free its arrays.  (Test hooks of ta_set_option:
 *     "fail_alloc_after" / "fail_throw_after" n make the n-th call of the library's allocation
 *     helper throw, tests/test_gpu_parity.py::test_exception_inside_the_library_becomes_a_status.)
 *   - HOST slabs (and the frame-major d_* inputs of the *_dev calls) are the reference's
 *     layout: (n_frames, n_atoms, dim) row-major (velocityautocorr.py:150-152,
 *     viscosity.py:128-134).  The library's own DEVICE slabs are "pair-major": the staging
 *     calls transpose frames as they are committed, so that a column pair (columns 2p, 2p+1
 *     of the n_atoms*dim columns) is one contiguous array of 16-byte rows (x[t], y[t]):
 *         element (t, c) -> slab[((c / 2) * pitch + t) * 2 + (c & 1)],  pitch = n_frames
 *     rounded up to 8; an odd last column is paired with zeros.  Every kernel reads that
 *     layout (coalesced along time); frame-major *_dev inputs are transposed into a scratch
 *     slab first (one more pass over the data and a second copy of it).
 *   - outputs are caller-owned.  "lagsum" outputs are lag-indexed SUMS over the
 *     atoms handled by this call, already divided by the frame-pair count
 *     (n_frames - lag): lagsum[k] = sum_n by_particle[k, n].  The caller divides
 *     by the total atom count after the (optional) cross-GPU reduce; this is the
 *     only cross-atom operation of the path (velocityautocorr.py:214,237,
 *     viscosity.py:233).
 *   - by_particle outputs are (n_frames, ld_bp) row-major float64 with
 *     ld_bp >= n_atoms (results.vacf_by_particle / results.visc_by_particle,
 *     velocityautocorr.py:145-147, viscosity.py:117-119); pass NULL to skip.
 *   - pointers named d_* are DEVICE pointers valid on the context's GPU;
 *     pointers named h_* are host pointers.
 *   - `stream` is a hipStream_t (void*); NULL = the legacy default (null) stream, exactly
 *     as for a HIP runtime call, so work queued by the caller on its default stream
 *     (PyTorch's default stream is the null stream) is ordered with the library's.
 *     The *_dev entry points are asynchronous on that stream; host-facing entry points
 *     run on a private non-blocking stream of the context and block until results are
 *     in the host buffers.
 *   - one context per analysis object; calls on one context are not re-entrant.
 *   - there is NO CPU fallback: without a usable GPU ta_ctx_create fails.
 */
#ifndef TA_HIP_H
#define TA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TA_OK 0
#define TA_E_INVALID -1   /* bad argument (shape, NULL, unsupported dim) */
#define TA_E_NOMEM -2     /* host or device allocation failed */
#define TA_E_HIP -3       /* a HIP runtime call or kernel launch failed */
#define TA_E_STATE -4     /* call order violated (e.g. compute before staging) */
#define TA_E_UNSUPPORTED -5

#define TA_F32 0
#define TA_F64 1

/* ta_ctx_create(TA_DEVICE_CPU, ...): the OPT-IN CPU backend behind the same symbols (csrc/cpu_backend.cpp, C++/OpenMP,
 * SURVEY.md section 8(b)): host slabs only, ta_stage_alloc / ta_stage_frame / ta_stage_commit (a no-op) / ta_vacf_fft /
 * ta_vacf_direct / ta_helfand_msd / ta_msd / ta_conductivity / ta_onsager / ta_onsager_cross / ta_current / ta_current_cross / ta_species_self / ta_orient / ta_chain_modes / ta_pair_find / ta_pair_find_read / ta_pair_lifetime / ta_bond_lifetime / ta_shell_residence / ta_shell_msd / ta_shell_orient / ta_unwrap / ta_compound / ta_stage_synth (into the host slab) / ta_set_option ("cpu_threads") / ta_stage_free /
 * ta_trim work as documented below and
 * compute on the host cores; every device-facing call (ta_stage_alloc_device, *_dev, *_staged, ta_stage_commit_dev,
 * timings, ta_group_*) returns TA_E_UNSUPPORTED.  It is never chosen on the caller's behalf: every other
 * device index is a GPU and fails without one.                                                              */
#define TA_DEVICE_CPU (-1)

typedef struct ta_ctx ta_ctx;

/* ---- context ---------------------------------------------------------- */
int ta_ctx_create(int device, ta_ctx **out);
int ta_ctx_destroy(ta_ctx *ctx);
/* the returned string is a per-thread copy: valid until the calling thread's next ta_last_error() */
const char *ta_last_error(const ta_ctx *ctx);
/* number of visible HIP devices (0 when none / runtime unusable) */
int ta_device_count(void);
/* library ABI version, bumped on any signature change */
int ta_abi_version(void);

/* ---- staging: replaces the per-frame slab fills ------------------------
 * VelocityAutocorr._prepare/_single_frame (velocityautocorr.py:142-153,178-194)
 * ViscosityHelfand._prepare/_single_frame (viscosity.py:111-142,167-199)
 *
 * ta_stage_alloc allocates n_slabs pinned host slabs of (n_frames, n_atoms,
 * dim) elements of `dtype` (TA_F32 is lossless for MDAnalysis data, which is
 * float32 at the source, and halves the PCIe bytes) plus float64 pair-major
 * device slabs; h_slabs[i] receives the host pointers, which the Python side
 * wraps as NumPy arrays and fills frame by frame.  ta_stage_commit moves
 * frames [frame_lo, frame_hi) of every slab host->device asynchronously in
 * their native width (<= 64 MiB pieces) and transposes them into the device
 * slabs there (the transposition of one piece runs while the next one crosses
 * PCIe).  The rows of a committed range must not be written again before the next compute / ta_stage_* call
 * on the context has returned (the copies are asynchronous, and by default queued to a worker thread:
 * option "async_commit").  Frames never committed read as zeros (np.zeros in the reference).
 * ta_stage_alloc_device: device slabs only, for data that is already on the
 * GPU; fill them with ta_stage_commit_dev (frame-major float32/float64 rows
 * [frame_lo, frame_hi) at d_src, row stride ld_row elements; asynchronous on
 * `stream`) or ta_stage_synth.  ta_stage_read_dev writes a frame-major
 * float64 copy of a slab (diagnostics / tests).  ta_stage_device returns the
 * pair-major device slab i, its pitch (rows per pair) and its pair count
 * (valid until the next ta_stage_alloc* / ta_stage_free / ta_ctx_destroy).
 * The pinned host views die with ta_stage_free / the next ta_stage_alloc.   */
int ta_stage_alloc(ta_ctx *ctx, int64_t n_frames, int64_t n_atoms, int dim, int dtype,
                   int n_slabs, void **h_slabs);
int ta_stage_alloc_device(ta_ctx *ctx, int64_t n_frames, int64_t n_atoms, int dim, int n_slabs);
int ta_stage_commit(ta_ctx *ctx, int64_t frame_lo, int64_t frame_hi);
/* The per-frame fill itself, natively: replaces
 *     self._velocities[i] = self.atomgroup.velocities[:, self._dim]        (velocityautocorr.py:192-194,
 *     viscosity.py:189-199; `atomgroup.velocities` is a gather ts.velocities[atomgroup.ix] into a temporary)
 * by ONE pass from the Timestep's own array into row `frame` of pinned slab `slab`:
 *     slab[frame, a, k] = (slab dtype) h_src[row(a) * ld_row + col0 + k * col_step],   a < n_atoms, k < n_col,
 *     row(a) = h_index ? h_index[a] : atom_lo + a
 * h_src: the frame's (n_atoms_universe, ld_row) float32 / float64 (src_dtype) rows, ld_row = 3 for an MDAnalysis
 * Timestep; n_col and n_atoms must equal the slab's dim and atom count.  The copy runs on a few host threads
 * ($TA_AMD_STAGE_THREADS, default 4 including the caller; ta_stage_threads() says how many); a ctypes caller's
 * GIL is released meanwhile.  ta_group_stage_frame: the same into every member's slab, member i taking atoms
 * [lo_i, hi_i) of the n_atoms (h_index + lo_i, or atom_lo + lo_i).  Callers keep the reference's guards
 * (ts.has_velocities etc.) in front of it; a source that is not a dense float array is staged through the
 * NumPy view of ta_stage_alloc instead.                                                        */
int ta_stage_frame(ta_ctx *ctx, int slab, int64_t frame, const void *h_src, int src_dtype, int64_t ld_row,
                   int col0, int col_step, int n_col, int64_t atom_lo, const int64_t *h_index, int64_t n_atoms);
int ta_stage_threads(void);
int ta_stage_commit_dev(ta_ctx *ctx, int slab, const void *d_src, int dtype, int64_t ld_row,
                        int64_t frame_lo, int64_t frame_hi, void *stream);
int ta_stage_read_dev(ta_ctx *ctx, int slab, double *d_dst, int64_t ld_row, void *stream);
int ta_stage_device(ta_ctx *ctx, int slab, double **d_slab, int64_t *pitch_rows, int64_t *n_pairs);
int ta_stage_free(ta_ctx *ctx);
/* Benchmark input (a stateless counter-based generator, so that the CPU baseline
 * and every GPU shard materialise the same tensor without shipping it): element (t, c) of the
 * slab = synth(seed, t * n_cols_total + col_offset + c), where synth(seed, i) is the sum of the
 * eight 16-bit fields of splitmix64(seed + 2 i) and splitmix64(seed + 2 i + 1), minus 262140,
 * times 1/sqrt(8 (65536^2 - 1) / 12): zero mean, unit variance, bit-identical in NumPy
 * (oracle/synth.py).  Asynchronous on `stream`.                                            */
int ta_stage_synth(ta_ctx *ctx, int slab, uint64_t seed, int64_t col_offset, int64_t n_cols_total,
                   void *stream);
/* Release the context's cached workspaces.  They are sized by the largest call so far and kept
 * until this call or ta_ctx_destroy: partial spectra (<= 42 MB), with a by-particle array the
 * atom-major scratch (n_atoms * n_frames * 8 bytes) and the power spectra of one block of atoms
 * (2.5 GiB unless "bp_spec_atoms" says otherwise), the pair-major copies of frame-major *_dev
 * inputs (the input's size, twice for Helfand), the 64 MiB landing buffer of ta_stage_commit,
 * the product slab of the "helfand_fft" option and of the Einstein MSD's FFT form (the input's size),
 * and for ta_conductivity* the moment's partial sums (<= 1024 * n_frames * dim * 8 bytes) and, with
 * the self term, the weighted slab (the input's size), and for ta_onsager* the species moments' partial sums
 * (<= 1024 * n_species * n_frames * dim * 8 bytes), the pair-major slab of the n_species^2 pseudo-particles and their
 * by-particle MSDs (n_species^2 * n_frames * (dim + 1) * 8 bytes); ta_current* use the same workspaces for the currents;
 * for ta_species_self* the weighted slab with each species' atoms contiguous (the input's element count * 8 bytes, plus at
 * most one column per species) beside what the lag-sum evaluation of one species needs; for ta_compound its plan (12 bytes per
 * member entry, 12 per compound) and, with frame weights, the (n_frames, dim) weighted mean and its partial sums (the
 * ta_onsager workspace); for ta_orient* the block of the orientation columns (3 * n_vectors * pitch * 16 bytes, shared by
 * the two ranks), the pair-major copy of the total (and the (n_frames, 3) total itself when it is not asked for) and the
 * sum's partial sums (the ta_onsager workspace); for ta_chain_modes* the blocks of one batch of modes (3 * n_chains * pitch * 8
 * bytes per mode);
 * the labels, weights and outputs of host-facing calls are kept.                                                                                                            */
int ta_trim(ta_ctx *ctx);

/* ---- pinned host memory for result arrays ---------------------------------
 * results.vacf_by_particle / results.visc_by_particle (velocityautocorr.py:145-147,
 * viscosity.py:117-119) are (n_frames, n_atoms) float64: 8 GB at 10000 x 100000.  Into a pageable
 * array the device->host copy of a host-facing call runs at ~16 GB/s the first time (the runtime
 * pins the pages on first use), into pinned memory at the link's rate.  ta_host_alloc returns
 * page-locked host memory that does NOT belong to a context (the result outlives the analysis
 * object); the Python side wraps it as the NumPy array it hands out and frees it with
 * ta_host_free when the last view dies.                                                   */
int ta_host_alloc(int64_t n_bytes, void **h_out);
/* the same with the calling thread bound to `device` first (hipSetDevice): a helper thread that
 * page-locks the array while frames are staged would otherwise create a HIP context on GPU 0 from
 * every rank.  device < 0: the calling thread's current device, as ta_host_alloc.            */
int ta_host_alloc_on(int device, int64_t n_bytes, void **h_out);
int ta_host_free(void *h);

/* ---- compute on staged slabs (host-facing, blocking) -------------------
 * ta_vacf_fft     : VelocityAutocorr._conclude_fft    (velocityautocorr.py:208-215,
 *                   incl. tidynamics.acf at :211-213)
 * ta_vacf_direct  : VelocityAutocorr._conclude_simple (velocityautocorr.py:217-238)
 * ta_helfand_msd  : ViscosityHelfand._conclude        (viscosity.py:201-233);
 *                   slab 0 = velocities, slab 1 = positions; `scale` is
 *                   1 / (2 * kB * mean(volumes) * temp_avg) (viscosity.py:229-231)
 * h_timeseries: (n_frames,) = mean over atoms; h_by_particle: (n_frames, n_atoms)
 * or NULL.  ta_vacf_fft beyond 163840 frames (the largest FFT plan) is evaluated by the
 * direct correlator (same quantity: the reference asserts their equality).      */
int ta_vacf_fft(ta_ctx *ctx, double *h_timeseries, double *h_by_particle);
int ta_vacf_direct(ta_ctx *ctx, double *h_timeseries, double *h_by_particle);
int ta_helfand_msd(ta_ctx *ctx, const double *h_masses, double scale, double *h_timeseries,
                   double *h_by_particle);
/* ta_msd          : MDAnalysis.analysis.msd.EinsteinMSD (_conclude_fft / _conclude_simple) on slab 0 = the
 *                   positions of the msd_type's columns: by_particle[k, n] = mean over t < n_frames - k of
 *                   sum_d (x[t+k,n,d] - x[t,n,d])^2, row 0 exactly 0; no masses, no division by dim.  fft = 1: up to 64
 *                   frames the exact register-resident kernel, beyond that S1 - 2 S2 on x - x[t=0] (n_frames <=
 *                   163840, else the direct form); fft = 0: the direct squared-difference forms.  fft other than 0 / 1:
 *                   TA_E_INVALID.  CPU backend: fft = 1 by zero-padded transforms of x - x[t=0], fft = 0 directly.
 *                   Float32 device slabs ("stage_device_f32") are widened to float64 first; "direct_f32" is ignored. */
int ta_msd(ta_ctx *ctx, int fft, double *h_timeseries, double *h_by_particle);
/* ta_conductivity : Einstein-Helfand ionic conductivity (no reference: a new analysis, ConductivityHelfand) on slab 0 = the
 *                   positions of the dim_type's columns and h_charges = the n_atoms charges q_n:
 *                     h_moment[t * dim + d] = M[t, d] = sum_n q_n (x[t,n,d] - x[0,n,d])          ((n_frames, dim), required)
 *                     h_collective[k] = Phi(k) = 1 / (n_frames - k) sum_{i < n_frames - k} sum_d (M[i+k,d] - M[i,d])^2
 *                     h_self_lagsum[k] = sum_n q_n^2 MSD_n(k), MSD_n as in ta_msd (the Nernst-Einstein self term)
 *                   h_collective / h_self_lagsum NULL: skipped (without the self term no weighted slab is written).  One
 *                   pass over the slab forms M as fixed-order partial sums (no atomics: the same bits from run to run)
 *                   and, for the self term, the weighted slab q (x - x[0]) in the context's scratch (one slab of
 *                   n_frames * n_atoms * dim * 8 bytes, kept as ta_trim says); Phi and the self term are the lag sums of
 *                   ta_msd with the same fft (0 / 1, else TA_E_INVALID) on a one-atom copy of M and on the weighted slab
 *                   (the FFT form adds ta_msd's own product slab).  NULL h_charges / h_moment: TA_E_INVALID; nothing
 *                   staged: TA_E_STATE.  CPU backend: the same in C++/OpenMP.  Timings: the moment pass is the main
 *                   kernel unless an FFT evaluation follows it (ta_kernel_timeline names it k_cond_moment).          */
int ta_conductivity(ta_ctx *ctx, int fft, const double *h_charges, double *h_moment, double *h_collective,
                    double *h_self_lagsum);
/* ta_onsager      : species-resolved Onsager transport coefficients (no reference: a new analysis, OnsagerHelfand) on slab 0 =
 *                   the positions of the dim_type's columns, h_species = one int32 label in 0 ... n_species - 1 per atom, in
 *                   any order (interleaved topologies), h_weights = one weight per atom (NULL: all 1),
 *                   1 <= n_species <= TA_ONSAGER_MAX_SPECIES:
 *                     h_moments[(s * n_frames + t) * dim + d] = M_s[t, d] = sum_{n: species[n] = s} w_n (x[t,n,d] - x[0,n,d])
 *                                                                                  ((n_species, n_frames, dim), required)
 *                     h_cross[(k * S + i) * S + j] = C[k, i, j] = 1 / (n_frames - k) sum_{t < n_frames - k} sum_d
 *                                  (M_i[t+k,d] - M_i[t,d]) (M_j[t+k,d] - M_j[t,d])          ((n_frames, S, S), or NULL: skipped)
 *                   ONE pass over the slab forms every species' moment (k_species_moment: the pass of ta_conductivity with
 *                   the sum split by label; fixed-order partial sums, no atomics, the same bits from run to run; the shift
 *                   by the first frame comes before the weight; a species without atoms has an exactly zero moment).  C is
 *                   evaluated by polarisation, C_ij = 1/4 [MSD(M_i + M_j) - MSD(M_i - M_j)], C_ii = MSD(M_i), in one
 *                   by-particle evaluation of ta_msd's dispatch with the same fft (0 / 1) on n_species^2 pseudo-particles:
 *                   C is symmetric bit for bit, C[0] is exactly 0, and the row and column of a species whose moment is
 *                   identically zero are exactly 0.  ACCURACY: the error of C_ij is that of the two MSDs it is the
 *                   difference of, i.e. relative to max_k max(C_ii, C_jj) (1e-10 of it at worst, FFT form), NOT to |C_ij|:
 *                   two nearly uncorrelated species have a C_ij far below that scale.
 *                   NULL h_species / h_moments, fft other than 0 / 1, n_species out of range, a label outside
 *                   0 ... n_species - 1 (checked on the host before anything is uploaded): TA_E_INVALID; nothing staged:
 *                   TA_E_STATE.  CPU backend: the same in C++/OpenMP.  Timings: the pass is the main kernel unless an FFT
 *                   evaluation follows it (ta_kernel_timeline names it k_species_moment; k_species_current of
 *                   ta_current is the same kernel without the shift, on the slab's own element type).
 * ta_onsager_cross: C (n_frames, S, S) of caller-provided moments (S, n_frames, dim) alone, e.g. the sum of several shards'
 *                   moments (moments add up over shards, C does not).  Needs no staged slab and leaves one untouched.   */
#define TA_ONSAGER_MAX_SPECIES 8
int ta_onsager(ta_ctx *ctx, int fft, int n_species, const int32_t *h_species, const double *h_weights, double *h_moments,
               double *h_cross);
int ta_onsager_cross(ta_ctx *ctx, int fft, const double *h_moments, int n_species, int64_t n_frames, int dim,
                     double *h_cross);

/* ta_current      : the Green-Kubo twin of ta_onsager (OnsagerGreenKubo, ConductivityGreenKubo) on slab 0 = the VELOCITIES of the
 *                   dim_type's columns; h_species, h_weights, n_species as for ta_onsager:
 *                     h_currents[(s * n_frames + t) * dim + d] = J_s[t, d] = sum_{n: species[n] = s} w_n v[t,n,d]
 *                                                                                  ((n_species, n_frames, dim), required)
 *                     h_cross[(k * S + i) * S + j] = C[k, i, j] = 1/2 * 1 / (n_frames - k) sum_{t < n_frames - k} sum_d
 *                                  (J_i[t,d] J_j[t+k,d] + J_j[t,d] J_i[t+k,d])              ((n_frames, S, S), or NULL: skipped)
 *                   Nothing is subtracted from the velocities and no term depends on frame 0; lag 0 is kept
 *                   (C[0, i, j] = <J_i . J_j>).  The slab is read ONCE for all species, in the element type it has: a
 *                   float32 device slab ("stage_device_f32") is read as float32 and summed in float64, never widened
 *                   first.  The currents' partial sums per group of column pairs are added in a fixed order (no
 *                   atomics: the same bits from run to run); a species without atoms gives exact zeros in J and in its
 *                   row and column of C.  C is evaluated by polarisation, 1/4 (ACF(J_i + J_j) - ACF(J_i - J_j)), in ONE
 *                   autocorrelation call on the n_species^2 pseudo-particles J_i, J_i + J_j, J_i - J_j (the evaluations of
 *                   ta_vacf_fft with fft = 1, of ta_vacf_direct with fft = 0): symmetric bit for bit, its error relative
 *                   to max(C_ii(0), C_jj(0)).  Errors as ta_onsager (the currents output takes the moments' place in
 *                   the messages); n_atoms * dim must be below 2^31.  CPU backend: the same in C++/OpenMP.  Timings: the
 *                   pass is the main kernel unless an FFT evaluation follows it (ta_kernel_timeline names it
 *                   k_species_current).
 * ta_current_cross: C (n_frames, S, S) of caller-provided currents (S, n_frames, dim) alone, e.g. the sum of several shards'
 *                   currents (currents add up over shards, C does not).  Needs no staged slab and leaves one untouched.   */
int ta_current(ta_ctx *ctx, int fft, int n_species, const int32_t *h_species, const double *h_weights, double *h_currents,
               double *h_cross);
int ta_current_cross(ta_ctx *ctx, int fft, const double *h_currents, int n_species, int64_t n_frames, int dim,
                     double *h_cross);

/* ta_species_self : the per-species SELF terms of the Onsager analyses (OnsagerHelfand / OnsagerGreenKubo with self_terms=True)
 *                   on slab 0, labels, weights and n_species as for ta_onsager:
 *                     h_self[s * n_frames + k] = sum_{n: species[n] = s} w_n^2 f_n(k)          ((n_species, n_frames), required)
 *                   quantity TA_SELF_MSD: slab 0 = the positions, f_n = ta_msd's by-particle series (row 0 exactly 0);
 *                   quantity TA_SELF_VACF: slab 0 = the velocities, f_n = the VACF's by-particle series (lag 0 kept).
 *                   h_counts (n_species) or NULL: the atoms per species.  No division by counts anywhere.  ONE pass over the
 *                   slab, in the element type it has (a float32 device slab is read as float32 and widened in registers),
 *                   writes the float64 slab W = w (x - x[0]) (MSD: the shift comes before the weight, as ta_conductivity's
 *                   self term) or w v (VACF) with each species' atoms contiguous and in input order, every species' block
 *                   starting on a column pair (k_species_sort: no atomics, one writer per element); then every species
 *                   with atoms gets one lag-sum evaluation on its block, the one ta_msd / ta_vacf_fft (fft = 1) /
 *                   ta_vacf_direct (fft = 0) would run on a slab of that species' weighted atoms alone -- the same bits.
 *                   A species without atoms: exact zeros.  With one species and weights = charges, TA_SELF_MSD is
 *                   ta_conductivity's h_self_lagsum bit for bit.  NULL h_species / h_self, quantity or fft other than
 *                   0 / 1, n_species out of range, a label outside 0 ... n_species - 1 (checked on the host before
 *                   anything is written): TA_E_INVALID; nothing staged: TA_E_STATE; n_atoms * dim must be below 2^31.  CPU
 *                   backend: each species gathered and weighted on the host, then its MSD / VACF routines.  Timings: the
 *                   pass is the main kernel unless an evaluation after it records its own (ta_kernel_timeline names it
 *                   k_species_sort).                                                                                   */
#define TA_SELF_MSD 0
#define TA_SELF_VACF 1
int ta_species_self(ta_ctx *ctx, int quantity, int fft, int n_species, const int32_t *h_species, const double *h_weights,
                    double *h_self, int64_t *h_counts);

/* ta_scatter : the intermediate scattering functions of the positions in slab 0 (IntermediateScattering) for n_k
 *              wavevectors h_kvecs (n_k, dim), rad per length unit, one component per staged column.  With the phase
 *              phi_j[t, n] = sum_d k_j[d] x[t, n, d]:
 *                h_self[j * n_frames + tau]   = 1/(T - tau) sum_{t < T - tau} sum_n cos(phi_j[t + tau, n] - phi_j[t, n])
 *                h_density[(j * n_frames + t) * 2 + {0, 1}] = sum_n {cos, sin} phi_j[t, n]
 *                h_coll[j * n_frames + tau]   = 1/(T - tau) sum_{t < T - tau} (rc[t] rc[t + tau] + rs[t] rs[t + tau]),
 *              rc, rs the two density components of wavevector j.  Lag 0 is kept (self: ~ n_atoms); NOTHING is divided
 *              by an atom count.  Each output may be NULL (not computed), not all three.  self and density add up over
 *              atoms -- shards, group members, ranks; coll does not: it is formed once from the summed density
 *              (ta_scatter_collective; needs no staged slab and touches none), as ta_current_cross from summed currents.
 *              The pass k_phase reads the slab ONCE per chunk of Kc wavevectors, in the element type it has (a float32
 *              device slab is read as float32 and widened in registers), and writes the float64 scratch slab Z: for
 *              wavevector jl of the chunk and atom n, pair jl n_atoms + n holds the rows (cos phi, sin phi) along time, in
 *              the input's pitch; rows n_frames ... pitch - 1 are zeros.  Every block of n_atoms pairs is a pair-major
 *              slab of n_atoms "atoms" with dim 2: self is ONE lag-sum evaluation of ta_vacf_fft (fft = 1) /
 *              ta_vacf_direct (fft = 0) per wavevector on its block, the density the fixed-order sum over its atoms (no
 *              atomics: the same bits from run to run), coll one by-particle autocorrelation of the n_k densities.
 *              Chunking: Kc = n_k when n_k n_atoms pitch 16 bytes fit 32 GiB, else the largest count that does (at least
 *              1); option "scatter_chunk" n >= 1 forces Kc = min(n, n_k).  The results do not depend on Kc bit for bit.
 *              ta_trim releases Z.
 *              Phases: the host passes q = k / (2 pi) (turns); u = sum_d q[d] x[d] in float64 (a product, then fma),
 *              r = u - rint(u), (cos, sin)(2 pi r).  With U = max |k . x| / (2 pi) over the call every phase carries at most
 *              2 pi (dim + 1) 2^-53 U rad of rounding plus the math functions' few ulp: each density component is within
 *              n_atoms (2 pi (dim + 2) 2^-53 U + 8 2^-53) of the exact sum; the correlations are the library's usual
 *              1e-10 of the series' scale for U up to ~1e3.  A wavevector commensurate with a constant box gives phases that
 *              are invariant under periodic wrapping: wrapped positions need no ta_unwrap.
 *              All outputs NULL, NULL h_kvecs, a non-finite component, fft other than 0 / 1, n_k outside
 *              1 ... TA_SCATTER_MAX_K (checked before anything is written): TA_E_INVALID; nothing staged: TA_E_STATE;
 *              n_atoms * max(dim, 2) must be below 2^31.  CPU backend: the same phase arithmetic, per wavevector a host
 *              slab (n_frames, n_atoms, 2) and its VACF routines, the density a plain sum in atom order.  Timings: the
 *              pass is the main kernel unless an evaluation after it records its own (ta_kernel_timeline names it
 *              k_phase).                                                                                              */
#define TA_SCATTER_MAX_K 4096
int ta_scatter(ta_ctx *ctx, int fft, int n_k, const double *h_kvecs, double *h_self, double *h_density, double *h_coll);
int ta_scatter_collective(ta_ctx *ctx, int fft, const double *h_density, int n_k, int64_t n_frames, double *h_coll);

/* ta_kcurrent : the longitudinal and transverse current correlation functions (CurrentCorrelation) of n_k wavevectors
 *              h_kvecs (n_k, dim), rad per length unit, one component per staged column.  Slab 0 holds the velocities v,
 *              slab 1 the positions x (ta_helfand_msd's convention); h_weights: one weight per atom (mass, charge), or
 *              NULL (all 1).  With T frames, D staged columns:
 *                phi_j[t, n]        = sum_d k_j[d] x[t, n, d]
 *                current[j, t, d]   = ( sum_n w_n v[t, n, d] cos phi_j[t, n],  sum_n w_n v[t, n, d] sin phi_j[t, n] )   (n_k, T, D, 2)
 *                k^_j = k_j / |k_j|;  jL[j, t] = sum_d k^_j[d] current[j, t, d]  (complex);
 *                jT[j, t, d] = current[j, t, d] - k^_j[d] jL[j, t]
 *                long[j, tau]  = 1/(T - tau) sum_{t < T - tau} Re( conj(jL[j, t]) jL[j, t + tau] )                        (n_k, T)
 *                trans[j, tau] = 1/(D - 1) 1/(T - tau) sum_{t < T - tau} sum_d Re( conj(jT[j, t, d]) jT[j, t + tau, d] )  (n_k, T)
 *              (D = 1: trans is zeros).  NOTHING is divided by an atom count.  Each output may be NULL (not computed), not
 *              all three.  current adds up over atoms -- shards, group members, ranks; long and trans do not: they are
 *              formed once from the summed current (ta_kcurrent_correlate; needs no staged slab and touches none).
 *              The pass k_kcurrent reads each atom ONCE per launch from both slabs, in the element type they have (a
 *              float32 row pair in one 16-byte load, widened in registers), keeps the D complex sums of KC wavevectors
 *              and F frames per thread in registers over the atoms of its group and writes one partial sum per group;
 *              k_sum_partials adds the groups in a fixed order (no atomics: the same bits from run to run).  The groups
 *              depend on the slab and the device only.  Chunking: one launch per KC wavevectors (ta_kcurrent_tile);
 *              option "kcurrent_chunk" n >= 1 forces min(n, KC).  The results do not depend on it bit for bit.  The partial
 *              buffer (groups x KC x T x D x 16 bytes, at most 1 GiB) does not depend on n_k; ta_trim releases it.
 *              Phases as ta_scatter's: q = k / (2 pi), u = sum_d q[d] x[d] (a product, then fma), r = u - rint(u),
 *              (cos, sin)(2 pi r); w_n v is one product, each sum one fma with the cosine and one with the sine.  With
 *              U = max |k . x| / (2 pi) and S_d = max_t sum_n |w_n v[t, n, d]| each component of current is within
 *              S_d (2 pi (D + 2) 2^-53 U + (10 + n_atoms) 2^-53) of the exact sum.  The correlations: the projections
 *              jL, jT_d (kcurrent_math.hpp) are K (1 + D) pseudo-atoms (D = 1: K) with dim 2 in ONE by-particle evaluation
 *              of ta_vacf_fft (fft = 1) / ta_vacf_direct (fft = 0), to the library's usual 1e-10 of the trace's scale.
 *              All outputs NULL, NULL h_kvecs, a non-finite component, a wavevector with |k| = 0 ("use ta_current for
 *              k = 0"; also one whose |k|^2 under- or overflows float64, which cannot be normalised), fft other than 0 / 1, n_k outside 1 ... TA_SCATTER_MAX_K (checked before anything is written):
 *              TA_E_INVALID; fewer than two staged slabs: TA_E_STATE; n_atoms * dim must be below 2^31.  CPU backend: the
 *              same phase arithmetic, a plain sum in atom order, the same projections, its VACF routines.  Timings: the
 *              main kernel of ta_last_timing / ta_timing_history is the LAST launch of k_kcurrent alone -- with n_k > KC
 *              one chunk's launch, not the whole pass -- unless an evaluation after it records its own; the time of all
 *              launches is in ta_kernel_timeline, which names the kernels k_kcurrent, k_sum_partials,
 *              k_kcurrent_project, k_kcurrent_finish.
 * ta_kcurrent_tile : KC, and the frames per thread F on a float64 / a float32 slab, of the one tile the library ships
 *              (a workgroup of k_kcurrent covers 256 F frames); each pointer may be NULL.                             */
int ta_kcurrent(ta_ctx *ctx, int fft, int n_k, const double *h_kvecs, const double *h_weights, double *h_current,
                double *h_long, double *h_trans);
int ta_kcurrent_correlate(ta_ctx *ctx, int fft, const double *h_current, int n_k, const double *h_kvecs, int64_t n_frames,
                          int dim, double *h_long, double *h_trans);
int ta_kcurrent_tile(int *kc, int *frames_f64, int *frames_f32);

/* ta_partial_density : the species-resolved density behind the partial intermediate scattering functions F_ab(k, t) and the
 *              partial structure factors S_ab(k) (PartialScattering), for n_k wavevectors h_kvecs (n_k, dim), rad per length
 *              unit, one component per staged column, of the positions in slab 0.  h_species: one label in
 *              0 ... n_species - 1 per atom, in any order (S = n_species <= TA_ONSAGER_MAX_SPECIES); h_weights: one weight
 *              per atom (scattering length, charge), or NULL (all 1).  With T frames:
 *                phi_j[t, n]      = sum_d k_j[d] x[t, n, d]
 *                rho[j, a, t]     = sum_{n: species[n] = a} w_n ( cos phi_j[t, n], sin phi_j[t, n] )               (n_k, S, T, 2)
 *                cross[j, tau, a, b] = 1/2 1/(T - tau) sum_{t < T - tau} Re( conj(rho[j, a, t]) rho[j, b, t + tau]
 *                                                                        + conj(rho[j, b, t]) rho[j, a, t + tau] )  (n_k, T, S, S)
 *              Lag 0 is kept; NOTHING is divided by an atom count.  h_cross may be NULL (not computed).  The density adds up
 *              over atoms -- shards, group members, ranks; the cross term does not: it is formed once from the summed
 *              density (ta_partial_cross; needs no staged slab and touches none).  Summed over a and b with unit weights
 *              the cross term is h_coll of ta_scatter.
 *              The pass k_species_density is k_kcurrent without the velocity slab and with the sum split by the label: it
 *              reads each atom ONCE per launch, in the element type the slab has (a float32 row pair in one 16-byte load,
 *              widened in registers), keeps ST x KC complex sums for each of its F frames per thread in registers over
 *              the atoms of its group (ST: the smallest of 1, 2, 4, 8 that holds S; the label picks the accumulator by a
 *              workgroup-uniform branch) and writes one partial sum per group; k_sum_partials adds the groups in a fixed
 *              order (no atomics: the same bits from run to run).  The groups depend on the slab and the device only.
 *              Chunking: one launch per KC wavevectors (ta_partial_density_tile); option "partial_chunk" n >= 1 forces
 *              min(n, KC).  The results do not depend on it bit for bit.  The partial buffer (groups x KC x S x T x 16
 *              bytes, at most 1 GiB) does not depend on n_k; ta_trim releases it.
 *              Phases as ta_scatter's: q = k / (2 pi), u = sum_d q[d] x[d] (a product, then fma), r = u - rint(u),
 *              (cos, sin)(2 pi r); each sum is one fma of w_n with the cosine and one with the sine.  With
 *              U = max |k . x| / (2 pi), n_a the atoms of species a and W_a = sum_{n in a} |w_n| each component of rho[., a, .]
 *              is within W_a (2 pi (dim + 2) 2^-53 U + (10 + n_a) 2^-53) of the exact sum.  The cross term: a complex
 *              density is a species sum with dim 2 (Re(conj(p) r) is the dot product), so it is ta_current_cross's
 *              polarisation on the S^2 pseudo-particles rho_a, rho_a + rho_b, rho_a - rho_b of every wavevector, ONE
 *              by-particle evaluation of ta_vacf_fft (fft = 1) / ta_vacf_direct (fft = 0) for all wavevectors of a chunk
 *              (as many as keep its workspace under 1 GiB); symmetric in (a, b) bit for bit; a species without atoms (or
 *              with an all-zero density) gives exact zeros in its density and in its row and column.  Accuracy: the
 *              library's usual 1e-10 of max(cross[j, 0, a, a], cross[j, 0, b, b]), NOT of |cross[j, tau, a, b]| -- an off-diagonal
 *              element is a difference of two autocorrelations of that size (ta_onsager gives the same warning).
 *              Checked before anything is written, TA_E_INVALID: fft other than 0 / 1, n_species outside
 *              1 ... TA_ONSAGER_MAX_SPECIES, NULL h_kvecs, n_k outside 1 ... TA_SCATTER_MAX_K, a non-finite component,
 *              NULL h_species or h_density, a label outside 0 ... S - 1, n_atoms * dim not below 2^31; nothing staged:
 *              TA_E_STATE.  CPU backend: the same phase arithmetic, a plain sum in atom order per species, ta_current_cross's
 *              routine on dim 2 per wavevector.  Timings: the main kernel of ta_last_timing / ta_timing_history is the LAST
 *              launch of k_species_density alone -- with n_k > KC one chunk's launch, not the whole pass -- unless an
 *              evaluation after it records its own; the time of all launches is in ta_kernel_timeline, which names the
 *              kernels k_species_density, k_sum_partials, k_onsager_combos, the lag kernels, k_partial_finish.
 * ta_partial_cross : the cross term (n_k, n_frames, S, S) of a host density (n_k, S, n_frames, 2), e.g. the sum of several
 *              shards' densities; TA_E_INVALID for fft other than 0 / 1, n_species or n_k out of range, a NULL array,
 *              n_frames outside 1 ... 2^30.
 * ta_partial_density_tile : for n_species (1 ... TA_ONSAGER_MAX_SPECIES, else TA_E_INVALID) the species slots ST and the
 *              wavevectors per launch KC of the tile that serves it, and the frames per thread F on a float64 / a float32
 *              slab (a workgroup of k_species_density covers 256 F frames); each pointer may be NULL.                  */
int ta_partial_density(ta_ctx *ctx, int fft, int n_k, const double *h_kvecs, int n_species, const int32_t *h_species,
                       const double *h_weights, double *h_density, double *h_cross);
int ta_partial_cross(ta_ctx *ctx, int fft, const double *h_density, int n_k, int n_species, int64_t n_frames,
                     double *h_cross);
int ta_partial_density_tile(int n_species, int *st, int *kc, int *frames_f64, int *frames_f32);

/* ta_vanhove : the self part of the van Hove function of the positions in slab 0 (VanHoveSelf): for n_lags frame lags
 *              h_lags (strictly increasing, 0 <= lag < n_frames) the histogram of the displacements after a lag in n_bins
 *              bins of width dr (r_max = n_bins dr) and their second and fourth moments.  With T frames, D staged columns:
 *                d_j   = x[t + tau, n, j] - x[t, n, j]                 float64 (a float32 slab: widened first, then subtracted)
 *                r2    = d_0 d_0, then fma(d_1, d_1, r2), then fma(d_2, d_2, r2)           (as many terms as D, in this order)
 *                e[b]  = fl(fl(b dr) fl(b dr)), b = 0 ... n_bins      float64, formed once on the host
 *                bin   = the b with e[b] <= r2 < e[b + 1];  r2 >= e[n_bins]: bin n_bins, the overflow bin
 *                h_counts[l * (n_bins + 1) + b] = #{(t, n): t < T - tau_l, bin = b}                         int64
 *                h_moments[l * 2 + {0, 1}]      = (sum r2, sum r2 r2) over the same pairs; r2 r2 added by fma(r2, r2, s4)
 *              NOTHING is divided by an atom count or by T - tau.  The bin is defined on r2 against SQUARED edges, not on
 *              sqrt(r2): the histogram is an exact integer quantity whenever r2 is exact, and because the CPU backend
 *              follows the same operation order for r2, its counts equal the GPU's for any input.  Either output may be
 *              NULL (not returned), not both; asking for one gives the same bits as asking for both.  counts and moments
 *              add up over atoms -- shards, group members, ranks.
 *              The pass k_vanhove reads the slab in the element type it has (a float32 device slab is read as float32 and
 *              widened in registers), once per chunk of Lc lags: a workgroup keeps its origin frames in registers,
 *              counts in a uint32 histogram in LDS (flushed into the uint64 one by integer atomic adds before it can
 *              overflow) and adds the moments without floating-point atomics: a fixed reduction within a wave, a slot per
 *              wave, one partial per (workgroup, lag), the partials added in a fixed order.  The same bits from run to
 *              run.  Chunking: Lc = the largest count for which 8 (n_bins + 1) + Lc (64 + 4 (n_bins + 1)) bytes of LDS stay
 *              within 64 KiB (at least 1), at most n_lags; option "vanhove_chunk" n >= 1 forces min(n, n_lags, that
 *              count).  The results do not depend on Lc bit for bit.  ta_trim releases the scratch histogram and partials.
 *              NULL h_lags, n_lags outside 1 ... TA_VANHOVE_MAX_LAGS, a lag < 0 or >= n_frames, lags not strictly
 *              increasing, n_bins outside 1 ... TA_VANHOVE_MAX_BINS, dr not finite or <= 0, both outputs NULL (all checked
 *              before anything is written): TA_E_INVALID; nothing staged: TA_E_STATE; n_atoms * dim must be below 2^31.
 *              CPU backend: the same r2 arithmetic and table, OpenMP over atoms with int64 histograms per thread added at
 *              the end, the moments per atom and then in atom order.  Timings: k_vanhove is the main kernel.              */
#define TA_VANHOVE_MAX_LAGS 1024
#define TA_VANHOVE_MAX_BINS 4096
int ta_vanhove(ta_ctx *ctx, int n_lags, const int64_t *h_lags, int n_bins, double dr, int64_t *h_counts, double *h_moments);

/* ta_overlap : the self-overlap of the positions in slab 0 per time origin (DynamicSusceptibility): the sum whose variance
 *              over origins is the four-point susceptibility chi_4.  With T frames, N atoms, D staged columns, n_lags lags
 *              under ta_vanhove's rules (strictly increasing, 0 <= tau < T, at most TA_VANHOVE_MAX_LAGS) and n_cutoffs
 *              cutoffs a_c (finite, > 0, strictly increasing, 1 <= n_cutoffs <= TA_OVERLAP_MAX_CUTOFFS):
 *                r2      = ta_vanhove's, of x[t0] and x[t0 + tau]: the same order, the same fma's; a float32 slab widened first
 *                a2[c]   = fl(a_c a_c)                                             float64, formed once on the host
 *                h_q[(c * n_lags + l) * T + t0] = #{n: r2 < a2[c]}  for t0 < T - tau_l,  0 for t0 >= T - tau_l       int64
 *              The comparison is strict, as the upper side of ta_vanhove's bins: with a_c = b dr the sum over t0 of
 *              Q[c, l, :] equals the sum of ta_vanhove's counts[l, b'] over b' < b, exactly.  A NaN r2 is not counted.
 *              NOTHING is divided; Q adds up over atoms -- shards, group members, ranks -- and a variance over origins is to
 *              be taken AFTER that sum (Q^2 does not add up), which is why the counts leave this interface per origin.
 *              A call with n_cutoffs * n_lags * T > 2^27 is refused: the output would pass 1 GiB.  That limit is a choice.
 *              The pass k_overlap reads the slab in the element type it has, with k_vanhove's reads, once per launch of Lc
 *              lags: a thread keeps a uint32 counter per (lag, cutoff, origin frame of its own) in registers across its
 *              atoms and adds the non-zero ones to the zeroed Q by 64-bit integer atomic adds at the end -- integers, so the
 *              same bits in any order, from run to run and for every Lc.  Lc = floor(S / n_cutoffs) with S the slots of
 *              the kernel's tile (ta_overlap_tile), at most n_lags; option "overlap_chunk" n >= 1 forces min(n, n_lags,
 *              that count).  ta_trim releases the output buffer of the host-facing calls.
 *              NULL h_lags, n_lags outside 1 ... TA_VANHOVE_MAX_LAGS, NULL h_cutoffs, n_cutoffs outside 1 ...
 *              TA_OVERLAP_MAX_CUTOFFS, a cutoff not finite or <= 0, cutoffs not strictly increasing, a NULL output, a lag
 *              < 0 or >= n_frames, lags not strictly increasing, the 2^27 bound (all checked before anything is written):
 *              TA_E_INVALID; nothing staged: TA_E_STATE; n_atoms * dim must be below 2^31.
 *              CPU backend: the same r2 and a2; OpenMP over the (lag, origin) pairs, each of which one thread counts over
 *              all atoms: the bits do not depend on the number of threads.  Timings: k_overlap is the main kernel.        */
#define TA_OVERLAP_MAX_CUTOFFS 4
int ta_overlap(ta_ctx *ctx, int n_lags, const int64_t *h_lags, int n_cutoffs, const double *h_cutoffs, int64_t *h_q);
/* the (lag, cutoff) slots S of one k_overlap launch, a compile-time tile of the library */
int ta_overlap_tile(int *slots);

/* ta_overlap_density : the density of the overlap field of the positions in slab 0 per time origin (FourPointStructureFactor):
 *              the sum whose variance over origins is the four-point structure factor S_4(k, t).  With T frames, N atoms, D
 *              staged columns, n_k wavevectors h_kvecs (n_k, D) in rad per length unit (1 <= n_k <= TA_SCATTER_MAX_K; k = 0
 *              is allowed), n_lags lags under ta_vanhove's rules and n_cutoffs cutoffs under ta_overlap's:
 *                r2, a2[c]  = exactly ta_overlap's (strict <; a float32 slab widened first; a NaN r2 counts nothing)
 *                (cos, sin) = exactly ta_partial_density's phase of x[t0], the ORIGIN frame: q = k / 2 pi on the host, u by
 *                             product-then-fma, r = u - rint(u), sincospi(2 r)
 *                h_w[(((j * n_cutoffs + c) * n_lags + l) * T + t0) * 2 + (0, 1)] = sum_{n: r2 < a2[c]} (cos, sin)
 *                             for t0 < T - tau_l,  (+0.0, +0.0) for t0 >= T - tau_l          float64, every element written
 *              NOTHING is divided and there are no weights.  The update is a select (an atom outside adds nothing, no 0 NaN
 *              arises).  With k = 0 the real part equals ta_overlap's Q exactly and the imaginary part is 0.  W adds up over
 *              atoms -- shards, group members, ranks --, |W|^2 does not: a variance over origins is to be taken AFTER that sum.
 *              A call with n_k * n_cutoffs * n_lags * T > 2^26 is refused: the output would pass 1 GiB.  That limit is a choice.
 *              The pass k_overlap_density reads the slab in the element type it has, with k_overlap's reads, once per launch
 *              of KC wavevectors and Lc lags: the phase depends on the origin frame only, so one sincospi per (atom, origin
 *              frame, wavevector) serves every (lag, cutoff) slot of the launch.  A thread keeps one complex sum per (slot,
 *              wavevector, origin frame of its own) in registers across its atoms; the sums leave as partials per group of
 *              atoms, added in a fixed order by k_overlap_density_sum: no atomics, and the groups depend on the slab and
 *              the device only, so the bits are the same from run to run and for every chunk.  Lc = floor(SL / n_cutoffs)
 *              with SL, KC of the kernel's tile (ta_overlap_density_tile), at most n_lags; option "overlap_density_chunk"
 *              n >= 1 forces min(n, n_lags, that count).  ta_trim releases the partials and the host-facing calls' output.
 *              NULL h_kvecs, n_k outside 1 ... TA_SCATTER_MAX_K, a non-finite component, then ta_overlap's checks of the
 *              lags and cutoffs, a NULL output, the 2^26 bound (all checked before anything is allocated or written, under
 *              the prefix "overlap_density: "): TA_E_INVALID; nothing staged: TA_E_STATE; n_atoms * dim must be below 2^31.
 *              CPU backend: the same r2, a2 and phase expression; OpenMP over the (lag, origin) pairs, each a plain sum in
 *              atom order: the bits do not depend on the number of threads.  Timings: k_overlap_density is the main kernel. */
int ta_overlap_density(ta_ctx *ctx, int n_k, const double *h_kvecs, int n_lags, const int64_t *h_lags, int n_cutoffs,
                       const double *h_cutoffs, double *h_w);
/* the (lag, cutoff) slots SL and the wavevectors KC of one k_overlap_density launch and the origin frames per thread (a
 * workgroup covers 256 frames of them), a compile-time tile of the library */
int ta_overlap_density_tile(int *slots, int *kc, int *frames);

/* ta_vanhove_distinct : the distinct part of the van Hove function of the positions in slab 0 (VanHoveDistinct): the
 *              histogram of the distances between item a_p at an origin frame and item b_q a lag later, over ORDERED pairs
 *              of different items.  With T frames, D staged columns:
 *                a[0 ... Na), b[0 ... Nb): index lists into the staged items, each strictly increasing and in range (HOST
 *                         arrays).  h_idx_a NULL: all items (n_a is ignored); h_idx_b NULL: b = a (n_b is ignored).
 *                lags   : ta_vanhove's rules (strictly increasing, 0 <= tau < T, at most TA_VANHOVE_MAX_LAGS)
 *                origins: t = origin_stride o, o = 0, 1, ...; lag l uses those with t + tau_l < T:
 *                         n_orig[l] = ceil((T - tau_l) / origin_stride)
 *                d_j    = x[t + tau, b_q, j] - x[t, a_p, j]          float64 (a float32 slab: widened first, then subtracted)
 *                         periodic axis:  sc = d_j M_j;  k = rint(sc);  d_j = fma(-k, H_j, d_j)
 *                         (H_j, M_j: the diagonal entries of the box table of ta_unwrap for that column's axis: the box
 *                         length and its reciprocal; the box of the ORIGIN frame)
 *                r2     = d_0 d_0, then fma(d_1, d_1, r2), then fma(d_2, d_2, r2)                     (ta_vanhove's order)
 *                bin    = ta_vanhove's, against its squared edges e[b] = fl(fl(b dr) fl(b dr)); r2 >= e[n_bins]: bin n_bins
 *                h_counts[l * (n_bins + 1) + bin] += 1 for every ordered pair (p, q) with a_p != b_q and every origin of lag l
 *              int64.  Exact for every call:  sum_bin h_counts[l, :] = n_orig[l] (Na Nb - |a n b|).  NOTHING is divided by a
 *              pair count, a volume or a shell measure (VanHoveDistinct does that); g(r) is the lag-0 row, normalised.
 *              Box: h_dimensions (n_frames, 6) and axes (dim entries) as for ta_unwrap; h_dimensions NULL: no periodicity
 *              (axes is ignored).  A non-orthogonal box in any frame: TA_E_INVALID (the one-step image is not the minimum
 *              image there).  Per-frame boxes are accepted only when every lag is 0 (the image uses the origin frame's box);
 *              with a lag > 0 the box must be constant.  fl(n_bins dr) must be <= half of every analysed box length in every
 *              origin frame.  For an orthorhombic box the one-step image is the minimum image whichever periodic images
 *              the positions are (an unwrapped trajectory included): nothing needs unwrapping or wrapping first.
 *              Two passes.  k_vhd_gather (O(N) per chunk of lags) reads the slab in the element type it has -- a float32
 *              device slab as float32, never a row at or past T -- and writes frame-major float64 scratch with the item
 *              index contiguous; k_vhd_pairs (the hot pass, O(Na Nb) per origin and lag) takes one (lag, origin, 256 a-items,
 *              1024 b-items) per workgroup, a lane owning 4 b-items in registers, counts into a uint32 LDS histogram (the
 *              overflow bin in a register) and adds the non-zero bins to the uint64 histogram by integer atomics.  Only
 *              integer adds: the same bits from run to run.  Lags go in chunks whose scratch fits 4 GiB (at least 1 lag);
 *              option "vanhove_distinct_chunk" n >= 1 forces min(n, n_lags).  The results do not depend on the chunk bit
 *              for bit.  ta_trim releases the scratch and the histogram.
 *              The CPU backend follows the same arithmetic (vanhove_distinct_math.hpp): its counts EQUAL the GPU's for any
 *              input, and do not depend on the number of threads.
 *              NULL h_lags, n_lags / n_bins / dr outside ta_vanhove's limits, a bad lag, origin_stride < 1, NULL h_counts,
 *              a list entry out of range or not increasing, n_a or n_b < 1 with a list, h_dimensions without axes, a box
 *              this call cannot use (all checked before anything is written): TA_E_INVALID; nothing staged: TA_E_STATE;
 *              n_atoms * dim must be below 2^31, and ceil(Na / 256) ceil(Nb / 1024) below 2^24 (about 2 million items on
 *              both sides; TA_E_INVALID, on both backends).  Of the box only the analysed axes' lengths are looked at: a
 *              zero or changing length on another axis is neither an error nor a per-frame box.  There is no ta_group_*
 *              form: pair sums would cross the members' atom shards.  Timings: k_vhd_pairs is the main kernel;
 *              ta_last_timing's main-kernel time is that of its LAST launch (one launch per chunk of lags and per 65535
 *              origins), ta_kernel_timeline lists every launch.                                                         */
int ta_vanhove_distinct(ta_ctx *ctx, int n_lags, const int64_t *h_lags, int64_t origin_stride, int64_t n_a,
                        const int64_t *h_idx_a, int64_t n_b, const int64_t *h_idx_b, const double *h_dimensions,
                        const int *axes, int n_bins, double dr, int64_t *h_counts);

/* ta_pair_find, ta_pair_find_read, ta_pair_lifetime : how long a pair of items stays together (PairLifetime): Rapaport's
 *              and Luzar-Chandler's pair population correlation functions of the positions in slab 0.  With T frames, D
 *              staged columns and the bond indicator of items p, q in frame t
 *                d_j    = x[t, q, j] - x[t, p, j]                      float64 (a float32 slab: widened first, then subtracted)
 *                         periodic axis:  sc = d_j M_j;  k = rint(sc);  d_j = fma(-k, H_j, d_j)        (ta_vanhove_distinct's
 *                         one-step image, H_j, M_j of frame t: both items are taken at the SAME frame)
 *                r2     = d_0 d_0, then fma(d_1, d_1, r2), then fma(d_2, d_2, r2)
 *                h_pq(t) = r2 < rc2,   rc2 = fl(r_cut r_cut) formed once in float64 on the host        (csrc/pair_math.hpp)
 *              the three calls give
 *                ta_pair_find     : the candidate pairs: every (a_p, b_q), a_p != b_q, with h = 1 in at least one SEARCHED
 *                         frame t = search_stride o, o = 0, 1, ... .  a, b: index lists as for ta_vanhove_distinct (strictly
 *                         increasing, in range, HOST arrays; h_idx_a NULL: all items; h_idx_b NULL: b = a).  With b = a (NULL,
 *                         or the same list twice) the pairs are unordered and only a_p < b_q is listed.  Two different lists
 *                         must be DISJOINT.  The list is kept in a workspace of the context, sorted by (a, b), as int32 staged
 *                         item ids; *n_pairs gets its length.  ta_trim, and a new staging, release it.
 *                ta_pair_find_read : copies the list into h_pairs (capacity, 2) int32, capacity >= the found count; with
 *                         nothing found (no search, or a search that found no pair) there is nothing to read: TA_E_STATE.
 *                ta_pair_lifetime : of the n_pairs pairs h_pairs (n_pairs, 2) int32 (HOST; two distinct in-range items per row;
 *                         rows named twice are counted twice: the caller's business), or with h_pairs NULL of the context's
 *                         found list (n_pairs is ignored).  An explicit list need not come from the search: donor-acceptor
 *                         lists of hydrogen bonds, 1-4 pairs.
 *                           h_ci[tau] = sum_pairs sum_{t < T - tau} h(t) h(t + tau)                     (T)      float64
 *                           h_runs[l] = the number of maximal runs of exactly l consecutive bonded frames,
 *                                       l = 1 ... T, h_runs[0] = 0; the run open at frame T - 1 ends there   (T + 1)  int64
 *                           h_nb[t]   = sum_pairs h(t)                                                  (T)      float64
 *                         NOTHING is divided: ci is NOT divided by T - tau (the other lag sums of this header are).  Each
 *                         output may be NULL (not computed), not all three.  With every frame an origin, the continuous
 *                         function's sum over origins is sum_l max(0, l - tau) h_runs[l], and sum_l l h_runs[l] = sum_t h_nb[t].
 *              Exactness.  h_runs and h_nb are integers for any input.  h_ci with fft = 0 is a sum of products of 0 / 1
 *              values: every path of ta_vacf_direct gives the partial sums exactly and divides them by T - tau; the call
 *              multiplies each block's row by T - tau again and rounds to the nearest integer, which is the exact sum while
 *              (the kernel's partial sums + 2) P_b T stays below 2^52 (the automatic block keeps P_b T at or below 2^32, which
 *              leaves room for 2^20 partial sums; the kernels use fewer than 2^18): exact integers, the same for every block
 *              size.  With fft = 1 the lag sums come from ta_vacf_fft's transforms, within the library's usual
 *              1e-10 of h_ci[0], and are not rounded.
 *              Box: h_dimensions (n_frames, 6) and axes (dim entries) as for ta_unwrap; NULL: no periodicity (axes is
 *              ignored).  Per-frame orthorhombic boxes are always accepted (frame t's box reduces frame t).  A
 *              non-orthogonal box in any frame: TA_E_INVALID.  r_cut must be finite, > 0 and, with a box, at most half of
 *              every analysed box length in every frame.  Of the box only the analysed axes' lengths are looked at.
 *              Passes.  ta_pair_find: k_vhd_gather at lag 0 writes the searched frames as frame-major float64 scratch (the
 *              slab read in the element type it has), k_pair_find takes one (256 a-items, 1024 b-items, searched frame) per
 *              workgroup on k_vhd_pairs' tile walk (one walk for both kernels, each with its own visitor); a wave's
 *              ballot of "bonded and a different item" over its 64 consecutive
 *              b-items is a word of the device bitmap [pitch_a][pitch_b / 64] and is ORed in by one lane when non-zero.
 *              The searched frames go in chunks whose scratch fits 4 GiB (option "pair_find_chunk" n >= 1 forces
 *              min(n, frames)); OR is idempotent: the same list for every chunk, from run to run.  k_pair_count takes
 *              popcounts per block of words, the block counts are scanned on the host (one small copy, the call's only
 *              synchronisation), k_pair_list expands the bits in (a, b) order.  ta_pair_lifetime: per block of pairs
 *              k_pair_series writes the indicator as a float64 pair-major block of P_b pseudo-atoms of dim 1 (1.0 / 0.0, rows
 *              n_frames ... pitch - 1 and an odd count's phantom column zeros; the slab read as it is, a float32 slab never
 *              widened first), k_pair_runs adds the block's run lengths by 64-bit integer atomics (runs of up to 8 frames
 *              are counted in registers first), ONE lag-sum evaluation of the block is its part of ci, ONE species-sum pass
 *              with unit weights its part of nb; the parts are added in block order.  Blocks hold as many pairs as fit
 *              32 GiB of indicator block (option "pair_chunk" n >= 1 forces min(n, n_pairs)).  Only integer atomics: the
 *              same bits from run to run.  ta_trim releases the scratch, the bitmap, the found list and the block.  The
 *              staged slab is not changed.
 *              The CPU backend follows the same arithmetic: its found lists and runs EQUAL the GPU's for any input, and so
 *              do ci and nb with fft = 0; nothing depends on the number of threads.
 *              Errors, all checked before anything is written.  TA_E_INVALID: NULL n_pairs, search_stride < 1, n_a or n_b < 1
 *              with a list, a list entry out of range or not increasing, two lists that overlap but differ, r_cut not finite
 *              or <= 0 or above half a box length, h_dimensions without axes, a box this call cannot use, fft other than
 *              0 / 1, all three outputs NULL, n_pairs < 1 or >= 2^30 with a list, a row out of range or naming an item twice,
 *              a capacity below the found count; ceil(Na / 256) ceil(Nb / 1024) at or above 2^24, a bitmap of more than 2^35
 *              bits (4 GiB: the padded item counts' product), n_atoms * dim at or above 2^31.  TA_E_STATE: nothing staged;
 *              ta_pair_find_read, or ta_pair_lifetime with h_pairs NULL, without a found list (never searched, trimmed,
 *              restaged) or with an EMPTY one.  There is no ta_group_* form: pairs cross the
 *              members' atom shards.  Timings: k_pair_find is the main kernel of ta_pair_find (its LAST launch, one per
 *              chunk of frames); k_pair_series (its last launch, one per block) is the main kernel of ta_pair_lifetime
 *              unless a lag-sum evaluation after it records its own; ta_kernel_timeline lists every launch.          */
int ta_pair_find(ta_ctx *ctx, int64_t n_a, const int64_t *h_idx_a, int64_t n_b, const int64_t *h_idx_b,
                 const double *h_dimensions, const int *axes, double r_cut, int64_t search_stride, int64_t *n_pairs);
int ta_pair_find_read(ta_ctx *ctx, int64_t capacity, int32_t *h_pairs);
int ta_pair_lifetime(ta_ctx *ctx, int fft, int64_t n_pairs, const int32_t *h_pairs /* (n_pairs, 2); NULL: the found list */,
                     const double *h_dimensions, const int *axes, double r_cut, double *h_ci /* (T) */,
                     int64_t *h_runs /* (T + 1), [0] = 0 */, double *h_nb /* (T) */);

/* ta_bond_lifetime : ta_pair_lifetime's three sums for bonds with an angle criterion, separate form and break criteria
 *              (hysteresis) and a tolerated absence (HydrogenBondLifetime, PairLifetime(r_break=, intermittency=)).  A bond
 *              is row n of h_atoms (n_bonds, n_at) int32 (HOST; distinct in-range items of slab 0): n_at = 2 a pair (p, q),
 *              n_at = 3 a triplet (d, h, a) = donor, hydrogen, acceptor.  In frame t, with the box of frame t
 *                r2   = ta_pair_lifetime's r2 between the FIRST and the LAST item of the row, in its order
 *                u_j  = image(x[t, d, j] - x[t, h, j]),  v_j = image(x[t, a, j] - x[t, h, j])        (triplets; the one-step image)
 *                dot  = u_0 v_0, then fma(u_1, v_1, dot), then fma(u_2, v_2, dot);  uu = u.u and vv = v.v the same way
 *                ang_ok(c2) = dot <= 0 && dot dot >= (c2 uu) vv      every product alone in its statement; c2 = fl(cos_cut cos_cut)
 *                             and cb2 = fl(cos_break cos_break) formed once on the host: the angle D-H-A is at least
 *                             acos(cos_cut), for cos_cut in [-1, 0] (90 ... 180 degrees), without a square root or an acos
 *                form = r2 < rc2 && ang_ok(c2),   brk = r2 < rb2 && ang_ok(cb2),   rc2 = fl(r_cut r_cut), rb2 = fl(r_break r_break)
 *                s(t) = brk ? (form ? 2 : 1) : 0                                                        the level
 *                h(t) = [s(t) = 2] || ([s(t) >= 1] && h(t - 1)),  h(-1) = 0                             hysteresis
 *                g(t) = h(t) || (t1 < t < t2 exist with h(t1) = h(t2) = 1 and t2 - t1 - 1 <= gap)        gap tolerance
 *              and h_ci, h_runs, h_nb are ta_pair_lifetime's outputs of the 0/1 series g; its exactness statements carry
 *              over.  Choices: the angle test is INCLUSIVE (a triplet exactly on the angle is bonded), the distance test
 *              STRICT as ta_pair_lifetime's.  With n_at = 2 there is no angle: cos_cut and cos_break are IGNORED (not even
 *              checked).  r_break >= r_cut and cos_break >= cos_cut: form implies brk; with both equal h = form.  A bond
 *              forms at level 2 and lasts while the level stays >= 1 (the stable-states picture).  An absence of at most
 *              gap frames BETWEEN two bonded frames is filled and counts as bonded in every output (MDAnalysis'
 *              intermittency, the tolerated absence t* of residence times); absences at the start and the end of the
 *              series are never filled.  gap is 0 ... 63: the series are filtered as 64-frame words, and an absence of up to
 *              63 frames is decided by a window of three words (the one before, the frame's own, the one behind).
 *              Passes: ta_pair_lifetime's, on its blocks ("pair_chunk"), with k_bond_series in k_pair_series' place (one
 *              kernel body under both, a row function each: the pair row keeps its single compare): it
 *              writes the level 0.0 / 1.0 / 2.0, and k_pair_filter turns the block into g in place (a wave per destination
 *              pair; the ballots of v == 2 and v >= 1 are the words; hysteresis is a fill of six shift / and / or steps with
 *              one carry bit across words; no atomics, no loop whose trip count depends on the data).  With gap = 0 and the
 *              break criterion equal to the form criterion there is nothing to filter: k_pair_filter is not launched and
 *              k_bond_series writes 1.0 for level 2; with n_at = 2 the outputs then have ta_pair_lifetime's bits.  The CPU
 *              backend follows the same arithmetic on the same packed words: its outputs (ci with fft = 0) EQUAL the GPU's.
 *              Errors, all checked before anything is written.  TA_E_INVALID: fft other than 0 / 1; all three outputs NULL;
 *              n_at other than 2 or 3; r_cut not finite or <= 0; r_break not finite or below r_cut; a cosine outside
 *              [-1, 0] or not finite; cos_break < cos_cut; gap outside 0 ... 63; n_bonds < 1 or >= 2^30, h_atoms NULL; a row
 *              naming an item out of range or twice; h_dimensions without axes, a non-orthogonal box, r_break above half an
 *              analysed box length in any frame; n_atoms * dim at or above 2^31.  TA_E_STATE: nothing staged.  There is no
 *              found-list form and no ta_group_* form.  k_bond_series (its last launch) is the main kernel.            */
int ta_bond_lifetime(ta_ctx *ctx, int fft, int64_t n_bonds, int n_at, const int32_t *h_atoms /* (n_bonds, n_at) */,
                     const double *h_dimensions, const int *axes, double r_cut, double r_break, double cos_cut,
                     double cos_break, int gap, double *h_ci /* (T) */, int64_t *h_runs /* (T + 1) */, double *h_nb /* (T) */);

/* ta_shell_residence : residence times in the shell of a GROUP (ShellResidence): ta_pair_lifetime's three sums of one series
 *              per OBSERVED item q of h_idx_b, whose indicator is the OR over all REFERENCE items p of h_idx_a (the residence
 *              function of Impey, Madden and McDonald).  In frame t, with the box of frame t and ta_pair_lifetime's r2 of
 *              d = x_q - x_p,
 *                form = [some p in a with id(p) != id(q) has r2 < rc2],   brk = [some such p has r2 < rb2],
 *                s(t) = brk ? (form ? 2 : 1) : 0,    rc2 = fl(r_cut r_cut), rb2 = fl(r_break r_break), both tests STRICT,
 *              then ta_bond_lifetime's hysteresis h and gap tolerance g, and h_ci, h_runs, h_nb are ta_pair_lifetime's
 *              outputs of the n_b series g: ci[tau] = sum_q sum_t g(t) g(t + tau) (undivided), runs[l] the maximal runs of
 *              l frames inside, nb[t] the observed items inside; the exactness statements carry over.  An item that passes
 *              from the shell of one reference item into that of another without a frame outside is ONE residence: no
 *              combination of pair-resolved calls gives that.  With ONE reference item the outputs have the bits of
 *              ta_bond_lifetime on the rows (a_0, q).
 *              Index lists as ta_pair_find's: HOST, strictly increasing, in range; h_idx_a NULL: all items; h_idx_b NULL:
 *              b = a; two lists are the same list or disjoint.  The same list means "in the shell of ANOTHER member".
 *              Box, r_cut, r_break, gap as ta_bond_lifetime's (r_break against half of every frame's analysed box lengths).
 *              Passes.  Per block of observed items and chunk of whole 64-frame words: k_vhd_gather at lag 0 writes the
 *              chunk's frames as frame-major float64 scratch (the slab read in the element type it has, never widened
 *              first); k_shell_series gives a workgroup 1024 observed items (4 per lane, in registers) and ONE 64-frame
 *              word, walks ALL reference items per frame on k_pair_find's tile walk and ORs the two flags; a wave's ballots
 *              after frame f are the 64-item words of that frame and lane f keeps them, so after the last frame lane f holds
 *              every item's bits at frame 64 w + f and stores one 16-byte row per pair of items: the block Z of
 *              ta_bond_lifetime (level 0.0 / 1.0 / 2.0, or 1.0 for level 2 where nothing is filtered), every row with one
 *              writer, without atomics, LDS or shuffles.  Then ta_bond_lifetime's passes, unchanged: k_pair_filter where
 *              needed, k_pair_runs, one lag-sum evaluation and one unit-weight species sum per block.  Blocks hold as many
 *              observed items as "pair_chunk" allows series (a block behind the first starts at an even item: a forced odd
 *              n counts as n - 1, at least 2); the frames go in chunks of words whose scratch fits 4 GiB, at most 65535
 *              (option "shell_chunk" n >= 1 forces min(n, words)).  Neither chunking changes a bit of the outputs.  The CPU
 *              backend follows the same arithmetic on packed words: its outputs (ci with fft = 0) EQUAL the GPU's.
 *              Errors, all checked before anything is written.  TA_E_INVALID: fft other than 0 / 1; all three outputs NULL;
 *              n_a or n_b < 1 with a list, a list entry out of range or not increasing, two lists that overlap but differ;
 *              n_b at or above 2^30; r_cut not finite or <= 0; r_break not finite or below r_cut; gap outside 0 ... 63;
 *              h_dimensions without axes, a non-orthogonal box, r_break above half an analysed box length in any frame;
 *              ceil(Na / 256) ceil(Nb / 1024) at or above 2^24; n_atoms * dim at or above 2^31.  TA_E_STATE: nothing staged.
 *              There is no ta_group_* form.  k_shell_series (its last launch) is the main kernel unless a lag-sum
 *              evaluation after it records its own.                                                                      */
int ta_shell_residence(ta_ctx *ctx, int fft, int64_t n_a, const int64_t *h_idx_a /* reference items; NULL: all */,
                       int64_t n_b, const int64_t *h_idx_b /* observed items; NULL: b = a */, const double *h_dimensions,
                       const int *axes, double r_cut, double r_break, int gap, double *h_ci /* (T) */,
                       int64_t *h_runs /* (T + 1) */, double *h_nb /* (T) */);

/* ta_shell_msd : the mean squared displacement of the observed items WHILE they are in the shell of the group (ShellMSD; the
 *              shell-resolved diffusion of Liu, Harder and Berne, MDAnalysis' waterdynamics zone MSD).  With g_q(t) the 0/1
 *              series of ta_shell_residence (same arguments, same bits), for the lags tau = 0 ... max_lag and axes j < dim
 *                w_q(t, tau) = prod_{s = t ... t + tau} g_q(s)         condition TA_SHELL_CONTINUOUS (0)
 *                w_q(t, tau) = g_q(t) g_q(t + tau)                     condition TA_SHELL_ENDPOINTS  (1)
 *                h_sums[tau][j] = sum_q sum_{t < T - tau} w_q(t, tau) (x_qj(t + tau) - x_qj(t))^2      float64 (max_lag + 1, dim)
 *                h_count[tau]   = sum_q sum_{t < T - tau} w_q(t, tau)                                  exact int64 (max_lag + 1)
 *              h_runs, h_nb: ta_shell_residence's.  The difference is formed in float64 after widening a float32 slab's
 *              elements in registers; NO image is applied to it: the positions must be unwrapped (ta_unwrap subtracts whole
 *              boxes of the frame itself, so the distance pass, which keeps its rint image, gives the same g on the unwrapped
 *              slab for orthorhombic boxes).  Every term is fma(d, d, acc).  count[tau] under "continuous" equals
 *              sum_{l > tau} runs[l] (l - tau), under "endpoints" ta_shell_residence's ci[tau] with fft = 0.
 *              Passes.  ta_shell_residence's, per block of observed items, up to k_pair_filter, k_pair_runs and the nb sum;
 *              then k_shell_bits packs the block's series by ballots (Z is read once more, everything behind reads 1 / 64 of
 *              it); k_shell_msd gives a workgroup the 256 lags of one pass, one per thread, and the items x, x + G, ... of
 *              the block: per chunk of origin frames ("shell_msd_chunk") the item's columns of the lagged frames go from the
 *              slab, in its own element type and through the same reader as every pair-major kernel, to LDS; a chunk without
 *              a frame inside is left after its words have been read; per origin inside (a scalar loop over the set bits of
 *              a workgroup-uniform word) the origin comes from a lane by v_readlane, the lagged frame from LDS, and the gate
 *              is one compare against the frames left in the run ("continuous"; origins whose run ends below the pass's
 *              lags are skipped by the whole workgroup) or one bit of the thread's window of g ("endpoints", whose popcount
 *              is the count).  Sums and counts stay in registers over all items of a workgroup; k_shell_fold adds the
 *              workgroups' rows in row order, the blocks in block order.  No atomics, no float add whose order depends on
 *              timing: repeat runs give the same bits.  The staged slab is only read.  The CPU backend follows the same
 *              arithmetic (shell_msd_math.hpp): on inputs whose sums are exact in float64 the outputs are EQUAL, otherwise
 *              within the library's 1e-10 scale-relative bound (the order of the adds differs).
 *              Errors, all checked before anything is written.  ta_shell_residence's (without fft), and TA_E_INVALID:
 *              condition other than 0 / 1; all four outputs NULL; max_lag < 0, above n_frames - 1 or above the cap 2047
 *              (eight passes of 256 lags; the message names it).  There is no ta_group_* form.                          */
#define TA_SHELL_CONTINUOUS 0
#define TA_SHELL_ENDPOINTS 1
int ta_shell_msd(ta_ctx *ctx, int condition, int64_t max_lag, int64_t n_a, const int64_t *h_idx_a /* reference; NULL: all */,
                 int64_t n_b, const int64_t *h_idx_b /* observed; NULL: b = a */, const double *h_dimensions, const int *axes,
                 double r_cut, double r_break, int gap, double *h_sums /* (max_lag + 1, dim) */,
                 int64_t *h_count /* (max_lag + 1) */, int64_t *h_runs /* (T + 1) */, double *h_nb /* (T) */);

/* ta_shell_orient : the reorientation of molecule-fixed unit vectors WHILE their molecule is in the shell of the group
 *              (ShellOrientation; MDAnalysis' waterdynamics WaterOrientationalRelaxation).  A vector n is row n of h_index, an
 *              int32 array (n_b, 2) for TA_ORIENT_BOND, (n_b, 3) for TA_ORIENT_BISECTOR / TA_ORIENT_NORMAL, atoms of slab 0 as
 *              ta_orient's; u_n(t) is formed by ta_orient's operation sequence (csrc/orient_math.hpp: orient_diff,
 *              orient_combine, orient_unit), a degenerate vector giving u = 0, never a NaN.  Column `anchor` of the row
 *              (0 <= anchor < row length) is the vector's ANCHOR atom: the anchors are the observed items of the shell,
 *              h_idx_b[n] must equal h_index[n][anchor]; with h_idx_b NULL the anchors must be the reference list itself ("in
 *              the shell of another member": water around water).  The anchors are therefore pairwise distinct and strictly
 *              increasing, as ta_shell_residence demands of its lists.  Two vectors on one anchor (OH1 and OH2 of a water)
 *              are two calls: their sums and counts add.  With g_n(t) ta_shell_residence's series of the anchor (same
 *              arguments, same bits: r_cut, r_break, gap, h_dimensions) and w_n(t, tau) ta_shell_msd's gate under
 *              `condition`, for the lags tau = 0 ... max_lag, with c = u_n(t) . u_n(t + tau),
 *                h_sums[tau][0] = sum_n sum_{t < T - tau} w_n(t, tau) c         float64 (max_lag + 1, 2)
 *                h_sums[tau][1] = sum_n sum_{t < T - tau} w_n(t, tau) c c
 *                h_count[tau]   = sum_n sum_{t < T - tau} w_n(t, tau)           exact int64 (max_lag + 1)
 *              h_runs, h_nb: ta_shell_residence's.  Arithmetic (csrc/shell_orient_math.hpp, shared with the CPU backend):
 *              c = fma(a_2, b_2, fma(a_1, b_1, fl(a_0 b_0))); per term s1 += c and s2 = fma(c, c, s2).  NOTHING is divided:
 *              ShellOrientation forms C_1 = S1 / N and C_2 = (3 S2 / N - 1) / 2.  A degenerate vector adds zeros to the sums
 *              and IS counted in N, because the gate is the shell alone; S1[0] is the number of non-degenerate terms at lag
 *              0, which shows it.
 *              The box.  h_dimensions serves both the distance pass (its rint image, orthorhombic boxes only) and the vectors'
 *              image step (ta_orient's, with the same H and M; only the orthorhombic entries can be non-zero here); NULL:
 *              neither.  It requires axes = {0, 1, 2}; three staged columns are required in any case.
 *              Passes.  ta_shell_msd's with ONE kernel exchanged: k_shell_orient stands in k_shell_msd's place and is the
 *              second instantiation of the same gated walk (csrc/shell_gate.hpp).  It forms u where the MSD reads a row:
 *              the vector's atoms of a frame through the same slab reader (a float32 slab as float32, widened in registers),
 *              the image step with that frame's box, u kept in LDS as float64, for the frames INSIDE only (under either
 *              gate a term's lagged frame is itself inside; ta_shell_msd's kernel now skips the others too, without a
 *              changed bit).  No block of u is written (ta_orient's route
 *              would need 3 n_b pitch 16 bytes); a chunk of origins without a frame inside costs its words alone.
 *              k_shell_fold adds the partial rows with two sums per lag.  Options "pair_chunk" and "shell_msd_chunk" as for
 *              ta_shell_msd; a block's index rows are the rows of its observed items.  No atomics: repeat runs give the
 *              same bits.  The CPU backend follows the same arithmetic: on inputs whose sums are exact the outputs are
 *              EQUAL, otherwise within the library's 1e-10 scale-relative bound.
 *              Errors, all checked before anything is written.  ta_shell_msd's (the cap 2047 on max_lag included), and
 *              TA_E_INVALID: a mode other than the three; anchor outside 0 ... row length - 1; NULL h_index; dim != 3; a box
 *              with axes other than {0, 1, 2}; n_atoms * 3 or n_b * 6 at or above 2^31; an index out of range; an atom twice
 *              in a row; a row whose anchor is not the observed item of the same number.  There is no ta_group_* form.
 *              ta_kernel_timeline names the kernel k_shell_orient.                                                      */
int ta_shell_orient(ta_ctx *ctx, int condition, int64_t max_lag, int mode, int anchor, const int32_t *h_index /* (n_b, 2 | 3) */,
                    int64_t n_a, const int64_t *h_idx_a /* reference; NULL: all */, int64_t n_b,
                    const int64_t *h_idx_b /* the anchors; NULL: b = a */, const double *h_dimensions, const int *axes, double r_cut,
                    double r_break, int gap, double *h_sums /* (max_lag + 1, 2) */, int64_t *h_count /* (max_lag + 1) */,
                    int64_t *h_runs /* (T + 1) */, double *h_nb /* (T) */);

/* ta_orient  : the rotational correlation functions of molecule-fixed unit vectors of the positions in slab 0
 *              (OrientationalCorrelation), three staged columns per atom.  A vector n is row n of h_index, atoms of slab 0,
 *              pairwise distinct and in [0, n_atoms):
 *                TA_ORIENT_BOND     (a, b)    : v = d(a -> b)
 *                TA_ORIENT_BISECTOR (a, b, c) : v = d(a -> b) + d(a -> c)              (a water's dipole direction, a = O)
 *                TA_ORIENT_NORMAL   (a, b, c) : v = d(a -> b) x d(a -> c)
 *              h_index is (n_vectors, 2) for a bond, else (n_vectors, 3), int32, row-major.  With u_n(t) = v / |v|:
 *                h_c1[tau]          = 1/(T - tau) sum_{t < T - tau} sum_n u_n(t) . u_n(t + tau)
 *                h_c2[tau]          = 1/(T - tau) sum_{t < T - tau} sum_n Q_n(t) : Q_n(t + tau),   Q = u (x) u - 1/3
 *                                   = 1/(T - tau) sum sum ((u . u')^2 - 1/3) = 2/3 sum sum P2(u . u')
 *                h_total[t * 3 + d] = M(t)_d = sum_n w_n u_n(t)_d             (h_weights: n_vectors values, NULL: all 1)
 *                h_coll[tau]        = 1/(T - tau) sum_{t < T - tau} M(t) . M(t + tau)
 *              Lag 0 is kept (c1: the number of non-degenerate vectors, c2: 2/3 of it).  NOTHING is divided by n_vectors or
 *              multiplied by 3/2 (OrientationalCorrelation does that).  The weights enter total and coll only.  Each output
 *              may be NULL (not computed), not all four.  c1, c2 and total add up over disjoint vector lists; coll does
 *              not: it is the autocorrelation of the summed total.
 *              Arithmetic (csrc/orient_math.hpp; the CPU backend runs the same sequence).  d(a -> b)_j = x[t, b, j] -
 *              x[t, a, j] in float64 (a float32 slab: widened first).  h_dimensions (n_frames, 6) as for ta_unwrap, or NULL
 *              (nothing is reduced): with H(t) the box vectors as rows (lower-triangular) and M = H^-1 of ta_unwrap's
 *              table, the difference is reduced by ONE sequential image step per axis, z, then y, then x:
 *                k = rint(d_2 M22);  d_2 = fma(-k, H22, d_2);  d_1 = fma(-k, H21, d_1);  d_0 = fma(-k, H20, d_0)
 *                k = rint(d_1 M11);  d_1 = fma(-k, H11, d_1);  d_0 = fma(-k, H10, d_0)
 *                k = rint(d_0 M00);  d_0 = fma(-k, H00, d_0)
 *              An orthorhombic box is the same code with zero off-diagonals (fma(-k, 0, d) = d exactly): an orthorhombic
 *              box given with angles that make it a triclinic table of the same H gives the same bits.  This is the
 *              MINIMUM image while the true vector is shorter than half the smallest box width (the distance between
 *              opposite faces) -- a bond, a molecule's arm -- whichever periodic images the atoms are; it is not a general
 *              triclinic minimum image.  The box of frame t reduces frame t: per-frame boxes (NPT) are followed.
 *              normal: v_0 = fma(b_1, c_2, -fl(b_2 c_1)) and cyclic.  n2 = fma(v_2, v_2, fma(v_1, v_1, fl(v_0 v_0))),
 *              u = v / sqrt(n2), u = 0 where n2 == 0 (or is not finite): a degenerate vector contributes zeros to every
 *              output, never a NaN.  Q's six columns: fma(u_j, u_j, -fl(1/3)) and fl(sqrt 2) fl(u_j u_k), zeros where u = 0.
 *              Error bounds per component of u, with e = 2^-53, from that operation sequence.  A difference is one
 *              rounding, e |d|.  Each of the (up to three) image steps a component goes through is one fma, i.e. one
 *              rounding of an intermediate no larger than the raw difference: with a box at most 3 e R |v| more, R = the
 *              largest raw |x_b - x_a| component over the smallest |v| of the call (R = 0 without a box; for wrapped
 *              molecules R is about the box length over the bond length).  Combining: nothing (bond), one rounding
 *              (bisector), two (normal: the product and the fma), relative to max(|d_ab|, |d_ac|)^2 there, so a nearly
 *              degenerate vector loses in proportion to max(|d_ab|, |d_ac|) / |v| (bisector) or |d_ab| |d_ac| / |v|
 *              (normal); for vectors that are not (that ratio <= 2) v is within 4 e |v| per component.  n2: three
 *              roundings of positive terms, sqrt and the division one each.  Together every component of u is within
 *              B_u e of the exact unit vector's, B_u = 12 + 3 R.  total: component d of M(t) is within
 *              (B_u + 1 + n_vectors) e sum_n |w_n| of the exact sum -- B_u e |w_n| per term from u, one rounding of the
 *              product w_n u_n, and at most n_vectors - 1 roundings of partial sums, each bounded by sum |w| (the pass
 *              adds its partials in a fixed order; the bound holds for any order), as the density's bound of ta_scatter
 *              grows with n_atoms.  c1, c2, coll: the library's usual 1e-10 of the series' maximum.
 *              The pass k_orient reads the slab in the element type it has (a float32 device slab as float32, widened in
 *              registers; never widened first), once per rank asked for, and writes a float64 pair-major block: rank 1
 *              (c1, total or coll asked for) n_vectors "atoms" of dim 3 holding u, rank 2 (c2) 2 n_vectors pseudo-atoms of
 *              dim 3 holding Q's columns, rows n_frames ... pitch - 1 zeros.  c1 and c2 are ONE lag-sum evaluation of
 *              ta_vacf_fft (fft = 1) / ta_vacf_direct (fft = 0) each on their block, total the fixed-order weighted sum
 *              over the rank-1 block's atoms (no atomics: the same bits from run to run), coll one evaluation of the total
 *              as one atom of dim 3.  The block is 3 n_vectors pitch 16 bytes, shared by the two ranks; the call does not
 *              chunk (a lag sum split over vectors would change its bits): TA_E_NOMEM when it does not fit.  ta_trim
 *              releases it.  The staged slab is not changed.
 *              A mode other than the three, fft other than 0 / 1, all outputs NULL, nothing staged or dim != 3,
 *              n_vectors < 1, NULL h_index, n_atoms * 3 or n_vectors * 6 at or above 2^31, an index out of range, an atom
 *              twice in a row, a non-finite weight, a box ta_unwrap's table rejects (all checked before anything is
 *              written): TA_E_INVALID.  CPU backend: the same arithmetic, OpenMP over frames, frame-major u and Q arrays
 *              and its VACF routines, total in vector order.  There is no ta_group_* form: a vector's atoms would have to
 *              share a shard.  Timings: the pass is the main kernel unless an evaluation after it records its own
 *              (ta_kernel_timeline names it k_orient, once per rank).                                                   */
#define TA_ORIENT_BOND 0
#define TA_ORIENT_BISECTOR 1
#define TA_ORIENT_NORMAL 2
int ta_orient(ta_ctx *ctx, int fft, int mode, int64_t n_vectors, const int32_t *h_index, const double *h_dimensions,
              const double *h_weights, double *h_c1, double *h_c2, double *h_total, double *h_coll);

/* ta_chain_modes : autocorrelations of linear functionals of whole chains of the positions in slab 0 (RouseModes: the Rouse
 *              normal modes X_p, the end-to-end vector), three staged columns per atom.  Chain c is row c of h_members
 *              (n_chains, chain_len) int32, row-major: chain_len = N >= 2 atoms (beads) of slab 0 in backbone order, pairwise
 *              distinct within the row and in [0, n_atoms); chains may share atoms.  h_coeff (n_modes, N) float64, row-major,
 *              is all the call knows about the functionals.  Per frame t:
 *                s_1 = 0,   s_n = s_{n-1} + img(x[t, m_n] - x[t, m_{n-1}])            n = 2 ... N
 *                Y_q(c, t) = sum_{n = 2 ... N} h_coeff[q * N + n - 1] * s_n           q = 0 ... n_modes - 1
 *                h_acf[q * T + tau] = 1/(T - tau) sum_{t < T - tau} sum_c Y_q(c, t) . Y_q(c, t + tau)
 *              s is the chain made whole relative to its first bead; h_coeff[q * N + 0] is read and checked but multiplies
 *              s_1 = 0.  A row of coefficients that sums to zero is therefore the same functional of the absolute positions,
 *              without any unwrapping: cos(p pi (n - 1/2) / N) / N is the Rouse mode X_p = 1/N sum_n r_n cos(p pi (n - 1/2) / N),
 *              p = 1 ... N - 1, and the unit row e_N the end-to-end vector r_N - r_1.  Lag 0 is kept.  NOTHING is divided by
 *              n_chains (RouseModes does that).  h_acf adds up over disjoint chain lists.
 *              Arithmetic (csrc/chain_math.hpp; the CPU backend runs the same sequence).  img is ta_orient's difference
 *              (csrc/orient_math.hpp, orient_diff): x[m_n] - x[m_{n-1}] in float64 (a float32 slab: widened first), and with
 *              h_dimensions (n_frames, 6) as for ta_unwrap (NULL: nothing is reduced) ONE sequential image step per axis, z,
 *              then y, then x, with the box of frame t, bit for bit the step documented under ta_orient: an orthorhombic box
 *              given as a triclinic table of the same H gives the same bits, per-frame boxes (NPT) are followed, and it is
 *              the MINIMUM image while every bond is shorter than half the smallest box width, whichever periodic images
 *              the beads are.  Then s_j = s_j + d_j, a plain add, and per mode acc_j = fma(coeff, s_j, acc_j) from acc = 0,
 *              in bead order.
 *              Error bound per component of Y_q, with e = 2^-53, from that sequence.  A bond d: one rounding of the raw
 *              difference and, with a box, one rounding per image step it goes through, each of an intermediate no larger
 *              than the raw difference: within (1 + 3 R) e b, b the longest bond and R = the largest raw |x_b - x_a|
 *              component over b (0 without a box; about the box length over the bond length for wrapped chains).  s_n: n - 1
 *              bonds and n - 2 roundings of partial sums no larger than the chain's extent S = max_n |s_n| <= (N - 1) b, so
 *              within ((1 + 3 R) b + S) (N - 1) e.  Y_q: N - 1 fmas, each one rounding of a partial sum bounded by
 *              A_q S, A_q = sum_n |coeff[q][n]|: every component of Y_q is within (N - 1) e (2 S + (1 + 3 R) b) A_q of the
 *              exact functional of the staged values -- a few thousand e times the chain's extent for chains of a hundred
 *              beads, far inside the lag sums' bar.  acf: the library's usual 1e-10 of the series' maximum.
 *              The pass k_chain_modes reads the slab in the element type it has (a float32 device slab as float32, widened
 *              in registers; never widened first) and walks every chain once for up to M modes, M of ta_chain_modes_tile:
 *              a call takes ceil(B / M) passes per batch of B modes, each a read of the slab.  A pass writes one float64
 *              pair-major block per mode, n_chains pseudo-atoms of dim 3 holding Y_q, rows n_frames ... pitch - 1 zeros
 *              (no atomics, one writer per element: the same bits from run to run); each row of h_acf is ONE lag-sum
 *              evaluation of ta_vacf_fft (fft = 1) / ta_vacf_direct (fft = 0) on its block.  A batch is as many modes as
 *              keep the blocks (3 n_chains pitch 8 bytes each) under 2 GiB, at least one (TA_E_NOMEM when that does not
 *              fit); option "chain_modes_chunk".  A mode's result does not depend on the batch or the pass it was in, bit
 *              for bit.  ta_trim releases the blocks.  The staged slab is not changed.
 *              fft other than 0 / 1, n_chains < 1, chain_len < 2, n_modes < 1, a NULL h_members, h_coeff or output, dim != 3,
 *              n_atoms * 3 or n_modes * n_chains * 3 at or above 2^31, a member out of range, an atom twice in a chain, a
 *              non-finite coefficient, a box ta_unwrap's table rejects (all checked before anything is written):
 *              TA_E_INVALID; nothing staged: TA_E_STATE.  CPU backend: the same arithmetic, OpenMP over chains, one
 *              frame-major array per mode and its VACF routines.  There is no *_dev entry and no ta_group_* form: a chain's
 *              atoms would have to share a shard.  Cross-correlations between modes and per-chain results are not formed.
 *              Timings: the (last) pass is the main kernel unless an evaluation after it records its own
 *              (ta_kernel_timeline names it k_chain_modes, once per pass).
 * ta_chain_modes_tile: *modes = M, the modes one pass of k_chain_modes serves, *frames = the frames per thread (a workgroup
 *              covers 256 of them); either may be NULL.                                                                  */
int ta_chain_modes(ta_ctx *ctx, int fft, int64_t n_chains, int64_t chain_len, const int32_t *h_members, int n_modes,
                   const double *h_coeff, const double *h_dimensions, double *h_acf);
int ta_chain_modes_tile(int *modes, int *frames);

/* ---- periodic unwrapping of a staged position slab ---------------------------------------------------------------
 * ta_unwrap: undo periodic wrapping of staging slab `slab` in place (MDAnalysis' NoJump), over the staged frames
 * in order.  h_dimensions: (n_frames, 6) float64 rows [a, b, c, alpha, beta, gamma] (A, degrees; ts.dimensions).
 * axes: `dim` entries, the box axis (0 = x, 1 = y, 2 = z) of each staged column d of an atom.
 * Non-orthogonal frames need axes == {0, 1, 2}; lengths <= 0 / non-finite, NULL pointers, bad axes -> TA_E_INVALID;
 * no slab -> TA_E_STATE.
 *   H(t) = the box vectors of frame t as rows (MDAnalysis' triclinic_vectors, float64), f(t) = x(t) H(t)^-1,
 *   n(0) = 0, n(t) = n(t-1) + rint(f(t) - f(t-1)) (an integer 3-vector per atom, round-half-even),
 *   x_u(t) = x(t) - n(t) H(t)
 * Frame 0 keeps its bits; a particle that moves more than half a box between two staged frames cannot be unwrapped (not
 * detected).  A box that changes from frame to frame (NPT) is followed, as by NoJump.  Works on slabs filled by
 * ta_stage_commit, ta_stage_commit_dev or ta_stage_synth: one in-place pass over the float64 device slab (unwrap.hip:
 * k_unwrap_ortho when every frame is orthogonal, else k_unwrap_tric), after the queued commits, blocking; recorded as a
 * compute call (ta_timing_history; the kernel is the main kernel, ta_kernel_timeline: box_copy, k_unwrap_*).  Float32
 * device slabs ("stage_device_f32"): TA_E_UNSUPPORTED.  CPU backend: the same arithmetic on the host slab, written back in
 * its element type (a TA_F32 slab holds the unwrapped positions rounded to float32, as NoJump's own output).
 * ta_group_unwrap (below, with the device groups): every member's block, with the same boxes.                       */
int ta_unwrap(ta_ctx *ctx, int slab, const double *h_dimensions, const int *axes);

/* ---- molecules instead of atoms: a staging transformation, like ta_unwrap -----------------------------------------
 * ta_compound: replace staged slab 0, (n_frames, n_atoms, dim), by a float64 slab of (n_frames, n_compounds, dim):
 *     out[t, c, d] = sum_{i in [h_offsets[c], h_offsets[c+1])} w_i x[t, h_members[i], d]  -  g_c F[t, d]
 *     g_c = sum_i w_i,      F[t, d] = sum_{a < n_atoms} u_a x[t, a, d]
 * w = h_weights, one per MEMBER ENTRY (NULL: all 1; weights that add up to 1 per compound give its weighted centre, masses /
 * the molecule's mass its centre of mass); u = h_frame_weights, one per atom (NULL: no F term at all; masses / the total mass
 * put the compounds into the barycentric frame of the system).  h_offsets: n_compounds + 1 entries, starting at 0, strictly
 * increasing (no empty compound), the last one = the number of member entries, below 2^31.  Members lie in 0 ... n_atoms - 1,
 * in any order, interleaved across compounds or not; an atom no compound names is dropped.
 *   Afterwards the context's staged shape is that of the new slab (same pitch, float64 elements whatever the old slab
 * held); the old device slab is freed once the call has completed and the pinned host slabs are released as by
 * ta_stage_free.  ta_stage_frame and ta_stage_commit* return TA_E_STATE until the next ta_stage_alloc*;
 * ta_stage_device, ta_stage_read_dev, ta_unwrap and every compute entry point see the new slab (ta_msd divides by
 * n_compounds).  Works on slabs filled by ta_stage_commit, ta_stage_commit_dev or ta_stage_synth.
 *   A compound's sum runs in member order in float64 (the first product as it is, every further term one fma; with F the
 * result is fma(-g_c, F, sum)); no atomics, one writer per element: the same bits from run to run.  Without frame weights a
 * one-member compound of weight 1 is its atom's column bit for bit.  The rows n_frames ... pitch - 1 of every pair and the
 * phantom column of an odd n_compounds * dim are written as zeros.  ONE pass over the slab in the element type it has
 * (k_compound, compound.hip: a float32 slab is read as float32 and widened in registers); F is formed first by
 * k_species_current with one species and its fixed-order partial sums.
 *   NULL h_offsets / h_members, bad offsets, a member out of range, n_compounds < 1 (checked on the host before anything is
 * written): TA_E_INVALID; nothing staged: TA_E_STATE; more than one staged slab: TA_E_UNSUPPORTED; n_atoms * dim and
 * n_compounds * dim must be below 2^31.  Blocking; recorded as a compute call (k_compound is the main kernel; the timeline
 * shows k_species_current first when F is asked for).  h_out (may be NULL): on a GPU context *h_out = NULL; on the CPU
 * backend *h_out = the new host slab, (n_frames, n_compounds, dim) float64 row-major, valid until the next ta_stage_alloc /
 * ta_stage_free (the same arithmetic and member order, parallel over compounds).                                        */
int ta_compound(ta_ctx *ctx, int64_t n_compounds, const int64_t *h_offsets, const int32_t *h_members,
                const double *h_weights, const double *h_frame_weights, void **h_out);

/* ---- compute on caller-provided device memory (asynchronous) -----------
 * Same arithmetic as above on a device-resident FRAME-MAJOR shard: d_vel / d_pos are
 * (n_frames, n_atoms, dim) float64 with row stride ld_row elements between
 * frames (ld_row >= n_atoms*dim; == for a dense slab, larger when the shard is a
 * column block of a wider slab).  The shard is first transposed into a pair-major
 * scratch slab owned by the context (see Conventions; ta_stage_alloc_device +
 * ta_stage_commit_dev + ta_*_staged avoid the copy).  d_lagsum: (n_frames,) SUM over
 * this shard's atoms.  d_by_particle: (n_frames, ld_bp) or NULL.                   */
int ta_vacf_fft_dev(ta_ctx *ctx, const double *d_vel, int64_t n_frames, int64_t n_atoms,
                    int dim, int64_t ld_row, double *d_lagsum, double *d_by_particle,
                    int64_t ld_bp, void *stream);
int ta_vacf_direct_dev(ta_ctx *ctx, const double *d_vel, int64_t n_frames, int64_t n_atoms,
                       int dim, int64_t ld_row, double *d_lagsum, double *d_by_particle,
                       int64_t ld_bp, void *stream);
int ta_helfand_msd_dev(ta_ctx *ctx, const double *d_vel, const double *d_pos,
                       const double *d_masses, int64_t n_frames, int64_t n_atoms, int dim,
                       int64_t ld_row, double scale, double *d_lagsum,
                       double *d_by_particle, int64_t ld_bp, void *stream);
int ta_msd_dev(ta_ctx *ctx, const double *d_pos, int64_t n_frames, int64_t n_atoms, int dim, int64_t ld_row,
               int fft, double *d_lagsum, double *d_by_particle, int64_t ld_bp, void *stream);
/* d_charges: (n_atoms,) device array; d_moment (n_frames, dim) required, d_collective / d_self_lagsum (n_frames,) or NULL.
 * A shard's moment and self lag sum add up over shards; Phi does not (reduce the moments, then ta_msd_dev with
 * n_atoms = 1, ld_row = dim on the sum).                                                                            */
int ta_conductivity_dev(ta_ctx *ctx, const double *d_pos, int64_t n_frames, int64_t n_atoms, int dim, int64_t ld_row,
                        int fft, const double *d_charges, double *d_moment, double *d_collective,
                        double *d_self_lagsum, void *stream);
/* d_species: (n_atoms,) int32 device labels, NOT checked: an atom whose label is outside 0 ... n_species - 1 is left out of
 * every moment.  d_weights: (n_atoms,) or NULL (all 1); d_moments (n_species, n_frames, dim) required; d_cross
 * (n_frames, n_species, n_species) or NULL.  Shards' moments add up; C does not (reduce the moments, then ta_onsager_cross). */
int ta_onsager_dev(ta_ctx *ctx, const double *d_pos, int64_t n_frames, int64_t n_atoms, int dim, int64_t ld_row, int fft,
                   int n_species, const int32_t *d_species, const double *d_weights, double *d_moments, double *d_cross,
                   void *stream);
/* d_vel: frame-major float64 velocities; d_species, d_weights as for ta_onsager_dev; d_currents (n_species, n_frames, dim)
 * required; d_cross (n_frames, n_species, n_species) or NULL.  Shards' currents add up; C does not. */
int ta_current_dev(ta_ctx *ctx, const double *d_vel, int64_t n_frames, int64_t n_atoms, int dim, int64_t ld_row, int fft,
                   int n_species, const int32_t *d_species, const double *d_weights, double *d_currents, double *d_cross,
                   void *stream);

/* d_x: frame-major float64 positions (TA_SELF_MSD) or velocities (TA_SELF_VACF); h_species: HOST labels (the block sizes
 * decide the launches; checked before anything is written); d_weights: (n_atoms,) device array or NULL (all 1); d_self
 * (n_species, n_frames).  Shards' self terms add up. */
int ta_species_self_dev(ta_ctx *ctx, const double *d_x, int64_t n_frames, int64_t n_atoms, int dim, int64_t ld_row,
                        int quantity, int fft, int n_species, const int32_t *h_species, const double *d_weights,
                        double *d_self, void *stream);

/* d_pos: frame-major float64 positions; h_kvecs: HOST wavevectors (n_k, dim) (they size the launches; checked before
 * anything is written); d_self (n_k, n_frames), d_density (n_k, n_frames, 2), d_coll (n_k, n_frames): device arrays, each
 * may be NULL, not all three.  Shards' self parts and densities add up. */
int ta_scatter_dev(ta_ctx *ctx, const double *d_pos, int64_t n_frames, int64_t n_atoms, int dim, int64_t ld_row, int fft,
                   int n_k, const double *h_kvecs, double *d_self, double *d_density, double *d_coll, void *stream);

/* d_pos: frame-major float64 positions, dim must be 3; h_index, h_dimensions, h_weights: HOST arrays, as for ta_orient (they
 * size the launches; checked before anything is written); d_c1 (n_frames), d_c2 (n_frames), d_total (n_frames, 3), d_coll
 * (n_frames): device arrays, each may be NULL, not all four.  c1, c2 and total of disjoint vector lists add up. */
int ta_orient_dev(ta_ctx *ctx, const double *d_pos, int64_t n_frames, int64_t n_atoms, int dim, int64_t ld_row, int fft,
                  int mode, int64_t n_vectors, const int32_t *h_index, const double *h_dimensions, const double *h_weights,
                  double *d_c1, double *d_c2, double *d_total, double *d_coll, void *stream);

/* d_pos: frame-major float64 positions; h_lags: HOST lags (they size the launches; checked before anything is written);
 * d_counts (n_lags, n_bins + 1) int64, d_moments (n_lags, 2) float64: device arrays, either may be NULL, not both.
 * Shards' counts and moments add up. */
int ta_vanhove_dev(ta_ctx *ctx, const double *d_pos, int64_t n_frames, int64_t n_atoms, int dim, int64_t ld_row, int n_lags,
                   const int64_t *h_lags, int n_bins, double dr, int64_t *d_counts, double *d_moments, void *stream);

/* d_pos: frame-major float64 positions; h_lags, h_cutoffs: HOST arrays, as for ta_overlap (they size the launches; checked
 * before anything is written); d_q (n_cutoffs, n_lags, n_frames) int64: a device array, every element of it written (zeros
 * at t0 >= n_frames - lag).  Shards' Q add up. */
int ta_overlap_dev(ta_ctx *ctx, const double *d_pos, int64_t n_frames, int64_t n_atoms, int dim, int64_t ld_row, int n_lags,
                   const int64_t *h_lags, int n_cutoffs, const double *h_cutoffs, int64_t *d_q, void *stream);

/* ---- compute on the staged (pair-major) slabs, device outputs, asynchronous on `stream` ----
 * Same arithmetic and outputs as the *_dev calls, on the slabs of ta_stage_alloc*: no
 * transposition, no second copy.  d_masses: (n_atoms,) float64 device array.              */
int ta_vacf_fft_staged(ta_ctx *ctx, double *d_lagsum, double *d_by_particle, int64_t ld_bp,
                       void *stream);
int ta_vacf_direct_staged(ta_ctx *ctx, double *d_lagsum, double *d_by_particle, int64_t ld_bp,
                          void *stream);
int ta_helfand_msd_staged(ta_ctx *ctx, const double *d_masses, double scale, double *d_lagsum,
                          double *d_by_particle, int64_t ld_bp, void *stream);
int ta_msd_staged(ta_ctx *ctx, int fft, double *d_lagsum, double *d_by_particle, int64_t ld_bp, void *stream);
int ta_conductivity_staged(ta_ctx *ctx, int fft, const double *d_charges, double *d_moment, double *d_collective,
                           double *d_self_lagsum, void *stream);
int ta_onsager_staged(ta_ctx *ctx, int fft, int n_species, const int32_t *d_species, const double *d_weights,
                      double *d_moments, double *d_cross, void *stream);
/* slab 0 holds the velocities, float64 or ("stage_device_f32") float32 elements: read as they are */
int ta_current_staged(ta_ctx *ctx, int fft, int n_species, const int32_t *d_species, const double *d_weights,
                      double *d_currents, double *d_cross, void *stream);

/* h_species: HOST labels, as for ta_species_self_dev; slab 0 is read in the element type it has */
int ta_species_self_staged(ta_ctx *ctx, int quantity, int fft, int n_species, const int32_t *h_species,
                           const double *d_weights, double *d_self, void *stream);

/* h_kvecs: HOST wavevectors, as for ta_scatter_dev; slab 0 (the positions) is read in the element type it has */
int ta_scatter_staged(ta_ctx *ctx, int fft, int n_k, const double *h_kvecs, double *d_self, double *d_density,
                      double *d_coll, void *stream);

/* h_index, h_dimensions, h_weights: HOST arrays, as for ta_orient_dev; slab 0 (the positions) is read in the element type it has */
int ta_orient_staged(ta_ctx *ctx, int fft, int mode, int64_t n_vectors, const int32_t *h_index, const double *h_dimensions,
                     const double *h_weights, double *d_c1, double *d_c2, double *d_total, double *d_coll, void *stream);

/* h_members, h_coeff, h_dimensions: HOST arrays, as for ta_chain_modes (checked before anything is written); d_acf (n_modes,
 * n_frames) on the device; asynchronous on `stream`, as ta_orient_staged; slab 0 (the positions) is read in the element type
 * it has */
int ta_chain_modes_staged(ta_ctx *ctx, int fft, int64_t n_chains, int64_t chain_len, const int32_t *h_members, int n_modes,
                          const double *h_coeff, const double *h_dimensions, double *d_acf, void *stream);

/* h_kvecs: HOST wavevectors, d_weights: device weights (n_atoms) or NULL, as ta_conductivity_staged's charges; slab 0 (the
 * velocities) and slab 1 (the positions) are read in the element type they have; each output may be NULL, not all three */
int ta_kcurrent_staged(ta_ctx *ctx, int fft, int n_k, const double *h_kvecs, const double *d_weights, double *d_current,
                       double *d_long, double *d_trans, void *stream);

/* h_kvecs: HOST wavevectors; d_species (n_atoms) int32 device labels (one outside 0 ... n_species - 1 is skipped: only a host
 * array can be checked), d_weights: device weights (n_atoms) or NULL; d_density (n_k, S, n_frames, 2), d_cross (n_k, n_frames,
 * S, S) or NULL: device outputs; slab 0 (the positions) is read in the element type it has */
int ta_partial_density_staged(ta_ctx *ctx, int fft, int n_k, const double *h_kvecs, int n_species, const int32_t *d_species,
                              const double *d_weights, double *d_density, double *d_cross, void *stream);

/* h_lags: HOST lags, as for ta_vanhove_dev; slab 0 (the positions) is read in the element type it has */
int ta_vanhove_staged(ta_ctx *ctx, int n_lags, const int64_t *h_lags, int n_bins, double dr, int64_t *d_counts,
                      double *d_moments, void *stream);

/* h_lags, h_cutoffs: HOST arrays, as for ta_overlap_dev; slab 0 (the positions) is read in the element type it has */
int ta_overlap_staged(ta_ctx *ctx, int n_lags, const int64_t *h_lags, int n_cutoffs, const double *h_cutoffs, int64_t *d_q,
                      void *stream);

/* h_kvecs, h_lags, h_cutoffs: HOST arrays, as for ta_overlap_density (they size the launches; checked before anything is
 * written); d_w (n_k, n_cutoffs, n_lags, n_frames, 2) float64 on the device; slab 0 (the positions) is read in the element
 * type it has.  Asynchronous on `stream`; there is no frame-major (_dev) entry */
int ta_overlap_density_staged(ta_ctx *ctx, int n_k, const double *h_kvecs, int n_lags, const int64_t *h_lags, int n_cutoffs,
                              const double *h_cutoffs, double *d_w, void *stream);

/* every list and the box: HOST arrays, as for ta_vanhove_distinct (they size the launches; checked before anything is
 * written); d_counts (n_lags, n_bins + 1) int64: a device array; slab 0 is read in the element type it has */
int ta_vanhove_distinct_staged(ta_ctx *ctx, int n_lags, const int64_t *h_lags, int64_t origin_stride, int64_t n_a,
                               const int64_t *h_idx_a, int64_t n_b, const int64_t *h_idx_b, const double *h_dimensions,
                               const int *axes, int n_bins, double dr, int64_t *d_counts, void *stream);
/* the pair list (or NULL: the context's found list) and the box: HOST arrays, as for ta_pair_lifetime (checked before anything
 * is written); slab 0 is read in the element type it has; d_ci (T), d_runs (T + 1) int64, d_nb (T) on the device, each may be
 * NULL, not all three */
int ta_pair_lifetime_staged(ta_ctx *ctx, int fft, int64_t n_pairs, const int32_t *h_pairs, const double *h_dimensions,
                            const int *axes, double r_cut, double *d_ci, int64_t *d_runs, double *d_nb, void *stream);
/* the bond list and the box: HOST arrays, as for ta_bond_lifetime (checked before anything is written); the outputs on the
 * device, as ta_pair_lifetime_staged's */
int ta_bond_lifetime_staged(ta_ctx *ctx, int fft, int64_t n_bonds, int n_at, const int32_t *h_atoms, const double *h_dimensions,
                            const int *axes, double r_cut, double r_break, double cos_cut, double cos_break, int gap,
                            double *d_ci, int64_t *d_runs, double *d_nb, void *stream);
/* the index lists and the box: HOST arrays, as for ta_shell_residence (checked before anything is written); the outputs on
 * the device, as ta_pair_lifetime_staged's */
int ta_shell_residence_staged(ta_ctx *ctx, int fft, int64_t n_a, const int64_t *h_idx_a, int64_t n_b, const int64_t *h_idx_b,
                              const double *h_dimensions, const int *axes, double r_cut, double r_break, int gap, double *d_ci,
                              int64_t *d_runs, double *d_nb, void *stream);
/* the index lists and the box: HOST arrays, as for ta_shell_msd (checked before anything is written); the outputs on the
 * device: d_sums (max_lag + 1, dim) float64, d_count (max_lag + 1) int64, d_runs (T + 1) int64, d_nb (T) float64 */
int ta_shell_msd_staged(ta_ctx *ctx, int condition, int64_t max_lag, int64_t n_a, const int64_t *h_idx_a, int64_t n_b,
                        const int64_t *h_idx_b, const double *h_dimensions, const int *axes, double r_cut, double r_break, int gap,
                        double *d_sums, int64_t *d_count, int64_t *d_runs, double *d_nb, void *stream);

/* the index rows, the index lists and the box: HOST arrays, as for ta_shell_orient (checked before anything is written); the
 * outputs on the device: d_sums (max_lag + 1, 2) float64, d_count (max_lag + 1) int64, d_runs (T + 1) int64, d_nb (T) float64 */
int ta_shell_orient_staged(ta_ctx *ctx, int condition, int64_t max_lag, int mode, int anchor, const int32_t *h_index, int64_t n_a,
                           const int64_t *h_idx_a, int64_t n_b, const int64_t *h_idx_b, const double *h_dimensions, const int *axes,
                           double r_cut, double r_break, int gap, double *d_sums, int64_t *d_count, int64_t *d_runs, double *d_nb,
                           void *stream);

/* ---- several GPUs behind one call (one process, one frame loop) ---------------------------
 * the multi-GPU fan-out and the reduce happen INSIDE the call.  A group owns
 * one context per entry of device_ids; member i stages and correlates the contiguous atom range
 * [n_atoms i / n_dev, n_atoms (i + 1) / n_dev) (ta_group_shard; the same split as one process per
 * GPU under torch.distributed), so the host fills n_dev pinned slabs per frame -- each GPU's column
 * block of the reference's slab (velocityautocorr.py:150-152,192-194; viscosity.py:128-134,189-199)
 * -- in ONE pass over the trajectory.  A compute call queues every member's kernels on its own
 * device, adds the members' (n_frames,) lag sums ONCE and divides by the total atom count
 * (velocityautocorr.py:214,237; viscosity.py:233); by-particle blocks are copied device->host
 * straight into the column range [lo_i, hi_i) of the caller's ONE (n_frames, n_atoms) array.
 * The reduce: n_dev = 1 none (librccl is not loaded); n_dev > 1 on distinct devices ncclReduce in
 * one RCCL group call (librccl.so dlopen'ed on first use; communicators from ncclCommInitAll);
 * members that share a device, or RCCL failing: peer copies to the first member + a sum in
 * member order.  ta_group_reduce_kind names what the last call used: "none" | "rccl" | "peer-copy";
 * ta_group_reduce_note says why an automatic choice fell back from RCCL to peer copies ("" when it
 * did not), ta_group_rccl_ranks how many ranks the communicator of the last RCCL reduce had
 * (ncclCommCount).  ta_group_set_option keys of the group itself (every other key goes to the
 * members' contexts, as ta_set_option):
 *   "reduce_mode" 0|1|2 : 0 automatic (above; also $TA_AMD_GROUP_REDUCE=auto), 1 peer copies whatever
 *                      the devices (=peer), 2 RCCL or an error (=rccl) -- with ONE member this runs
 *                      ncclCommInitAll(1) + ncclReduce onto itself, the form of the RCCL branch a
 *                      one-GPU box can execute;  "force_rccl" 1 = "reduce_mode" 2.
 * h_slabs of ta_group_stage_alloc: n_dev * n_slabs pointers, member i's slab s at [i * n_slabs + s]
 * (NULL for a member without atoms: more devices than atoms), each (n_frames, hi_i - lo_i, dim).
 * h_masses of ta_group_helfand_msd: all n_atoms.  ta_group_msd: ta_msd on every member's slab 0.  Options go to every member.                */
typedef struct ta_group ta_group;
int ta_group_create(const int *device_ids, int n_dev, ta_group **out);
int ta_group_destroy(ta_group *g);
const char *ta_group_last_error(const ta_group *g);
int ta_group_size(const ta_group *g);
int ta_group_member(ta_group *g, int i, ta_ctx **ctx, int *device);
int ta_group_shard(const ta_group *g, int64_t n_atoms, int i, int64_t *atom_lo, int64_t *atom_hi);
const char *ta_group_reduce_kind(const ta_group *g);
const char *ta_group_reduce_note(const ta_group *g);
int ta_group_rccl_ranks(const ta_group *g);
int ta_group_set_option(ta_group *g, const char *key, int64_t value);
int ta_group_stage_alloc(ta_group *g, int64_t n_frames, int64_t n_atoms, int dim, int dtype,
                         int n_slabs, void **h_slabs);
int ta_group_stage_commit(ta_group *g, int64_t frame_lo, int64_t frame_hi);
int ta_group_stage_frame(ta_group *g, int slab, int64_t frame, const void *h_src, int src_dtype, int64_t ld_row,
                         int col0, int col_step, int n_col, int64_t atom_lo, const int64_t *h_index, int64_t n_atoms);
/* device slabs only + the benchmark generator on every member's columns of the one synthetic
 * tensor (member i: col_offset + lo_i * dim), as ta_stage_alloc_device / ta_stage_synth          */
int ta_group_stage_alloc_device(ta_group *g, int64_t n_frames, int64_t n_atoms, int dim, int n_slabs);
int ta_group_stage_synth(ta_group *g, int slab, uint64_t seed, int64_t col_offset, int64_t n_cols_total);
int ta_group_stage_free(ta_group *g);
int ta_group_vacf_fft(ta_group *g, double *h_timeseries, double *h_by_particle);
int ta_group_vacf_direct(ta_group *g, double *h_timeseries, double *h_by_particle);
int ta_group_helfand_msd(ta_group *g, const double *h_masses, double scale, double *h_timeseries,
                         double *h_by_particle);
int ta_group_msd(ta_group *g, int fft, double *h_timeseries, double *h_by_particle);
/* ta_group_conductivity: ta_conductivity on every member (h_charges: all n_atoms); the members' moments and self lag sums
 * are SUMMED on the host in member order, then ONE collective MSD of the summed moment runs on the first member that holds
 * atoms.  h_collective is required here.                                                                             */
int ta_group_conductivity(ta_group *g, int fft, const double *h_charges, double *h_moment, double *h_collective,
                          double *h_self_lagsum);
/* ta_group_onsager: ta_onsager on every member with its slice of h_species / h_weights (all n_atoms; labels checked first)
 * and the call's n_species; the members' moments are SUMMED on the host in member order, then ONE cross evaluation of the
 * summed moments runs on the first member that holds atoms.  h_cross NULL: the moments alone.                          */
int ta_group_onsager(ta_group *g, int fft, int n_species, const int32_t *h_species, const double *h_weights,
                     double *h_moments, double *h_cross);
/* ta_group_current: ta_current on every member in the same way: the members' currents are SUMMED on the host in member
 * order, then ONE cross evaluation of the summed currents runs on the first member that holds atoms.                   */
int ta_group_current(ta_group *g, int fft, int n_species, const int32_t *h_species, const double *h_weights,
                     double *h_currents, double *h_cross);
/* ta_group_species_self: ta_species_self on every member with its slice of h_species / h_weights (all n_atoms; labels checked
 * first); the members' (n_species, n_frames) arrays and counts are SUMMED on the host in member order.               */
int ta_group_species_self(ta_group *g, int quantity, int fft, int n_species, const int32_t *h_species,
                          const double *h_weights, double *h_self, int64_t *h_counts);
/* ta_group_scatter: ta_scatter on every member with the same wavevectors (checked first): the members' self parts and
 * densities are SUMMED on the host in member order, then ONE collective part of the summed density runs on the first
 * member that holds atoms.                                                                                          */
int ta_group_scatter(ta_group *g, int fft, int n_k, const double *h_kvecs, double *h_self, double *h_density,
                     double *h_coll);
/* ta_group_kcurrent: ta_kcurrent on every member with the same wavevectors (checked first) and its slice of h_weights (all
 * n_atoms, or NULL): the members' currents are SUMMED on the host in member order, then ONE pair of correlations of the
 * summed current runs on the first member that holds atoms.                                                          */
int ta_group_kcurrent(ta_group *g, int fft, int n_k, const double *h_kvecs, const double *h_weights, double *h_current,
                      double *h_long, double *h_trans);
/* ta_group_partial_density: ta_partial_density on every member with the same wavevectors (checked first) and its slice of
 * h_species and h_weights (all n_atoms; weights or NULL): the members' densities are SUMMED on the host in member order,
 * then ONE cross term of the summed density runs on the first member that holds atoms.                               */
int ta_group_partial_density(ta_group *g, int fft, int n_k, const double *h_kvecs, int n_species, const int32_t *h_species,
                             const double *h_weights, double *h_density, double *h_cross);
/* ta_group_vanhove: ta_vanhove on every member with the same lags and bins (checked first): the members' counts are SUMMED
 * on the host as int64, their moments in member order.                                                               */
int ta_group_vanhove(ta_group *g, int n_lags, const int64_t *h_lags, int n_bins, double dr, int64_t *h_counts,
                     double *h_moments);
/* ta_group_overlap: ta_overlap on every member with the same lags and cutoffs (checked first): the members' Q are SUMMED on
 * the host as int64 -- the per-origin counts add up over atoms, their squares do not.                                */
int ta_group_overlap(ta_group *g, int n_lags, const int64_t *h_lags, int n_cutoffs, const double *h_cutoffs, int64_t *h_q);
/* ta_group_overlap_density: ta_overlap_density on every member with the same wavevectors, lags and cutoffs (checked first):
 * the members' W are SUMMED on the host in member order as float64 -- the per-origin sums add up over atoms, |W|^2 does not. */
int ta_group_overlap_density(ta_group *g, int n_k, const double *h_kvecs, int n_lags, const int64_t *h_lags, int n_cutoffs,
                             const double *h_cutoffs, double *h_w);
/* ta_group_unwrap: ta_unwrap on every member's block of slab `slab` (declared with ta_unwrap above) */
int ta_group_unwrap(ta_group *g, int slab, const double *h_dimensions, const int *axes); /* every member's block */

/* ---- instrumentation ----------------------------------------------------
 * Device time of the last *_dev / host-facing compute call on this context,
 * measured with hipEvents recorded on the stream the kernels were launched on.
 * total_ms covers the whole launch sequence; main_kernel_ms only the dominant
 * kernel (FFT accumulate pass / direct correlator).  Blocks until the events
 * have completed.                                                            */
int ta_last_timing(ta_ctx *ctx, float *total_ms, float *main_kernel_ms);
/* the same for the last min(max_n, 64, calls so far) compute calls on this context, oldest
 * first (a caller times K calls back to back and reads the K durations afterwards);
 * *n_out = number of entries written.  Blocks until those calls have completed.      */
int ta_timing_history(ta_ctx *ctx, int max_n, float *total_ms, float *main_kernel_ms, int *n_out);
/* With the "timeline" option on, every compute call records an event before each of its kernel
 * launches.  ta_kernel_timeline returns, for the last compute call, the device time per kernel
 * NAME in order of first appearance (a kernel launched once per block of atoms is summed):
 * names[i] (static strings owned by the library), ms[i], *n_out entries (<= max_n).  The sum is
 * the call's total_ms.  Blocks until the call has completed.                              */
int ta_kernel_timeline(ta_ctx *ctx, int max_n, const char **names, float *ms, int *n_out);
/* the number of launches recorded under `name` in the last compute call's timeline (0: none, or the option is off) */
int ta_kernel_launches(ta_ctx *ctx, const char *name, int *n_out);
/* The clock the headline kernel actually runs at (MI355X lowers it under load; board power and
 * the driver's sclk are not the test).  Launches a DIAGNOSTIC build of the lag-sum forward kernel
 * (in-kernel s_memtime / s_memrealtime stamps; the product kernels execute no stamp) n_launches
 * times back to back on the staged float64 slab -- ask for >= 2 s worth -- and reports, from the
 * last launch: *mhz = delta s_memtime / delta s_memrealtime x 100 MHz (mean over workgroups),
 * *cycles_per_unit_pass = shader cycles one workgroup spends per column pair and pass, and
 * *ms_per_launch (events around all launches; the stamped build is a few per cent slower than the
 * product kernel).  Plans R0 = 8, 10, 12, 16, 20 without an outer radix (n_frames in (3584, 4096],
 * (4608, 5120], (5120, 6144], (7168, 8192], (9216, 10240]); otherwise TA_E_UNSUPPORTED.        */
int ta_clock_probe(ta_ctx *ctx, int n_launches, double *mhz, double *cycles_per_unit_pass,
                   double *ms_per_launch);
/* FFT length bookkeeping for a given n_frames: *m_out = padded half-length M
 * (the transform computes a 2M-point correlation, 2M >= 2*n_frames-1): M = R * R0 * 512 with
 * R0 in {1,...,10,12,14,16,18,20} and the outer radix R = 1 up to 10240 frames (one on-chip
 * transform per pass), R in {2,3,4,5,8,16} with R0 in {12,14,16,18,20} up to 163840 frames (n_stages
 * counts the outer step).
 * Beyond that ta_vacf_fft* compute the same quantity with the direct correlator and this
 * call returns TA_E_UNSUPPORTED.                                              */
int ta_fft_plan_info(int64_t n_frames, int64_t *m_out, int *n_threads, int *n_stages);
/* options (key, value):
 *   "direct_f32" 0|1 : direct correlators (ta_vacf_direct*, ta_helfand_msd*) round the staged values (Helfand:
 *                      P = (m v) x, formed in float64) ONCE to float32, form products / squared differences
 *                      in float32 and accumulate in float64 (BASELINE configs[4]'s float32 path; within 2e-6
 *                      of the series' scale).  Helfand runs on the FP32 matrix cores (band32tp_kernels.hpp:
 *                      v_mfma_f32_16x16x4_f32 on a float32 product slab, T*A*D*4 bytes more), with or without
 *                      the by-particle array, any dim: 2.2x the float32 vector kernel; the windowed VACF stays on
 *                      the vector kernel.  Default 0 = float64.
 *   "direct_mfma" 1|0|3: ta_vacf_direct* and ta_helfand_msd* on the matrix cores (float64: FP64,
 *                      v_mfma_f64_16x16x4_f64; under "direct_f32": FP32 for Helfand) -- bandbp_kernels.hpp,
 *                      band32tp_kernels.hpp: the instruction's k-slots are filled from the time axis, a particle's
 *                      columns live in a per-wave LDS ring; with or without the by-particle arrays; Helfand from
 *                      products of rows centred on a nearby frame (every lag and particle within 1e-9 of the
 *                      difference-first vector kernel, pure trend included; needs T*A*D*8 (float32: *4) bytes for
 *                      the product slab, else the vector kernel runs).
 *                      1 (default) = by n_frames (these kernels fill a ring and run an epilogue per particle and lag
 *                      group; the vector kernel packs 2 - 8 particles into a wave under ~640 frames): windowed VACF from
 *                      513 frames, Helfand float64 from 352, its float32 option from 448 (below: the vector kernel; up
 *                      to 64 frames see "short_max").  0 = the vector kernels everywhere; 3 = matrix cores always.
 *                      (2, the column-packed forms of rounds 4-5 with their inline-assembly LDS-DMA, is rejected
 *                      since round 6: those kernels are tools/band/, built on demand as a second opinion.)
 *   "short_max" n    : trajectories of up to n frames (default and maximum 64; 0 = never) take the register-resident
 *                      kernels of short_kernels.hpp wherever float64 arithmetic on float64 slabs is asked for a
 *                      by-particle array (all three quantities) or an O(T^2) form ("direct_mfma" 1 only: 0 and 3 force
 *                      their forms): a lane per column, every lag in its registers, the by-particle array written in
 *                      place.  "short_lags_max" n (default 48): the lag sums of ta_vacf_fft* alone as well, up to n frames.
 *   "helfand_fft" 0|1: ta_helfand_msd* evaluate the mean squared differences in O(T log T)
 *                      (n_frames <= 163840, else as default): sum (P[i]-P[i+k])^2 = S1(k) - 2 S2(k), S2 by the FFT
 *                      lag sums of the product slab P = (m v) x, S1 by prefix sums.  An
 *                      extension (the reference has only the O(T^2) loop,
 *                      viscosity.py:201-233, which stays the default): ~1e-15 of the series'
 *                      scale, but the relative error of lags whose mean squared difference
 *                      is far below P^2 grows by that ratio.  Needs T*A*D*8 bytes more.
 *   "bp_block" n     : host-facing calls with a by-particle array process atoms in blocks of n
 *                      (rounded up to 64; default 16384) so that a block's device->host copy
 *                      runs under the next block's compute;
 *   "fft_nwg", "direct_nwg" : persistent workgroup counts (0 = automatic);
 *   "direct_chunk" 0|8|10, "direct_groups" n : force the direct correlators' lags per chunk /
 *                      cap the atoms a workgroup works on at once (0 = automatic);
 *   "mid_max" n      : trajectories of 97 ... n frames (default and maximum 512; 0 = never) take k_mid (mid_kernels.hpp: a
 *                      lane per column and pair of 16-lag blocks, a sliding window in registers) for the windowed VACF, and
 *                      for the Einstein-Helfand sums up to 128 frames (the Einstein MSD: 65 ... 512 frames), under "direct_mfma" 1 and float64 arithmetic;
 *                      "mid_all" 1: wherever the kernel can run (65 ... 512 frames, both quantities); "mid_ncl" 3..6:
 *                      log2 of the lanes per pair of lag blocks, i.e. the columns per tile (tools/mid_shapes.py; 0: by length);
 *   "direct_subwave" 1|0 : the vector kernel's column groups may be 8, 16 or 32 lanes where a column has that few
 *                      pairs of lag chunks (under ~640 frames): several particles per wave, 3x at 65 ... 256 frames
 *                      (0: a whole wave per column, as before round 6);
 *   "stage_device_f32" 0|1 : device slabs allocated AFTERWARDS hold float32 elements when the host
 *                      slabs are TA_F32 (or there are none: ta_stage_alloc_device): half the
 *                      device footprint (BASELINE configs[4]: 12 GB instead of 24 GB per GPU).
 *                      The float32 direct correlators ("direct_f32" 1) read them as they are, and
 *                      so do the FFT kernels for 513 ... 10240 frames (8-byte rows widened exactly
 *                      in the first stage: 3-14 % faster than from float64 slabs, float64
 *                      arithmetic, results equal to float64 slabs of the same values to rounding);
 *                      every other evaluation first widens them into float64 scratch slabs.  ta_stage_device
 *                      then returns a pointer to float rows (8 bytes per pair row).
 *   "bp_spec_atoms" n : FFT path with a by-particle array: atoms per block of power spectra
 *                      (scratch = n * 16 * M bytes; 0 = as many as fit 2.5 GiB);
 *   "bp_prefetch" 0..3 : sub-series of the next atom's spectrum the inverse kernel requests
 *                      ahead (default 2);
 *   "timeline" 0|1   : record an event before every kernel launch of a compute call
 *                      (ta_kernel_timeline);
 *   "scatter_chunk" n : wavevectors per pass of ta_scatter* (0, the default: as many as fit 32 GiB of scratch; n >= 1:
 *                      min(n, n_k)); the results do not depend on it;
 *   "kcurrent_chunk" n : wavevectors per launch of ta_kcurrent*'s pass (0, the default: KC, the tile's count; n >= 1:
 *                      min(n, KC)); the results do not depend on it;
 *   "partial_chunk" n : wavevectors per launch of ta_partial_density*'s pass (0, the default: KC, the count of the tile
 *                      that serves the call's species; n >= 1: min(n, KC)); the results do not depend on it;
 *   "partial_cross_chunk" n : wavevectors per batch of the cross term of ta_partial_density* and ta_partial_cross (0, the
 *                      default: as many as keep the batch's workspaces under 1 GiB, at least 1; n >= 1: min(n, that count)).
 *                      A batch is ONE by-particle evaluation of its n S^2 pseudo-particles.  With fft = 0, and with an even
 *                      S^2, the results do not depend on it; with fft = 1 and an odd S^2 other pseudo-particles share a
 *                      transform in another batching and the results agree within the FFT path's bound;
 *   "chain_modes_chunk" n : modes per batch of ta_chain_modes* (0, the default: as many as keep the batch's blocks under
 *                      2 GiB, at least 1; n >= 1: min(n, that count)); the results do not depend on it bit for bit;
 *   "vanhove_chunk" n : lags per pass of ta_vanhove* (0, the default: as many as fit 64 KiB of LDS; n >= 1: min(n, n_lags,
 *                      that count)); the results do not depend on it;
 *   "overlap_chunk" n : lags per launch of ta_overlap* (0, the default: floor(S / n_cutoffs), S of ta_overlap_tile; n >= 1:
 *                      min(n, n_lags, that count)); the results do not depend on it;
 *   "overlap_density_chunk" n : lags per launch of ta_overlap_density* (0, the default: floor(SL / n_cutoffs), SL of
 *                      ta_overlap_density_tile; n >= 1: min(n, n_lags, that count)); the results do not depend on it bit for bit;
 *   "vanhove_distinct_chunk" n : lags per pass of ta_vanhove_distinct* (0, the default: as many as fit 4 GiB of gathered
 *                      scratch, at least 1; n >= 1: min(n, n_lags)); the results do not depend on it;
 *   "pair_chunk" n : candidate pairs per block of ta_pair_lifetime* (0, the default: as many as fit 32 GiB of indicator
 *                      block, at least 2; n >= 1: min(n, n_pairs)); the results do not depend on it (ci with fft = 0 bit for
 *                      bit; with fft = 1 within the FFT path's bound); ta_shell_residence* takes it as observed items per block;
 *   "pair_find_chunk" n : searched frames per pass of ta_pair_find (0, the default: as many as fit 4 GiB of gathered scratch,
 *                      at least 1, at most 65535; n >= 1: min(n, frames)); the found list does not depend on it;
 *   "shell_chunk" n : 64-frame words per pass of ta_shell_residence* (0, the default: as many as fit 4 GiB of gathered
 *                      scratch, at least 1, at most 65535; n >= 1: min(n, words)); the results do not depend on it;
 *   "shell_msd_chunk" n : origin frames per staged chunk of k_shell_msd (0, the default: 512; n >= 1: n rounded up to a
 *                      multiple of 64, at most 1024); counts do not depend on it, sums by the order of a thread's adds only
 *                      (the origins stay in frame order: the same bits);
 *   "async_commit" 1|0 : ta_stage_commit hands its frame range to a worker thread of the context, which
 *                      makes the HIP calls (the caller's frame loop never waits on the runtime, e.g. while
 *                      another thread page-locks a result array); every call that touches the slabs joins
 *                      the queue first and returns a queued commit's error.  0: the calls are made by
 *                      ta_stage_commit itself.   Unknown keys return TA_E_INVALID.          */
int ta_set_option(ta_ctx *ctx, const char *key, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* TA_HIP_H */
