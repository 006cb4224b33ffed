"""The species-resolved family per lag, per species and per pair against exact sums and extended-precision references:
the Onsager moments and their cross term C[k, i, j] (ta_onsager), the Green-Kubo currents and theirs (ta_current) and the
per-species self terms (ta_species_self).  The shape tests hold these to 1e-10 ... 1e-12 of an array's LARGEST element;
the users read the slope of C_ij(k) and self_s(k) at early lags, where a diffusive C_ii is 1 / T of its maximum, and a
small species next to a large one is held to even less.  Here every element has a bound of its own, as in
test_exact_parity.py (whose frame counts, shifts and helpers are used):

(a) Integer inputs (oracle.exact.int_walk at 2^30, int_velocities, nonzero integer weights), where every sum the kernels
    form is exact -- a CONDITION, asserted by oracle.exact.budget on w (y - y[0]) over A D T terms and on the moments /
    currents and the pseudo-particle series Q_i +- Q_j over D T terms (test_budget_holds_for_every_case, no GPU needed):
      * moments and currents bit-equal to the integer sums, an empty species exact zeros;
      * C_ii(k) within 2 ulps of the correctly rounded R(Q_i)(k) / (T - k) (k_cross_finish copies the by-particle element
        of pseudo-particle i S + i through); moments: lag 0 exactly 0;
      * C_ij(k), i != j: with R+- = R(Q_i +- Q_j)(k) / (T - k) exact rationals,
            |C_ij(k) - 1/4 (R+ - R-)| <= u (|R+| + |R-|) + u |C_ij(k)|.
        Derivation from k_cross_finish as written, c = 0.25 * (row[lo S + hi] - row[hi S + lo]): each by-particle element
        is within 2 ulps <= 4 u |R| of its rational, so the difference of the two carries 4 u (|R+| + |R-|) and one
        rounding of the subtraction, u |r+ - r-| = 4 u |C_ij| to first order; the factor 1/4 is exact.  k_onsager_combos
        forms Q_i +- Q_j without rounding (integers under the budget).  For the moments R+ + R- = 2 (C_ii + C_jj): a few u
        of max(C_ii(k), C_jj(k)) AT THAT LAG.  Both triangles bit-equal; row and column of an empty species exactly 0.
        The reference is the exact rational (int64 numerators, long double quotient), never an output of the library;
      * self terms: |self_s(k) - sum_{n in s} w_n^2 f_n(k)| <= (N_s + 2) u sum_{n in s} |w_n^2 f_n(k)|, f_n the exact
        per-atom MSD / VACF quotient (test_exact_parity.check_lag_sums as a sum); the MSD's lag 0 exactly 0; counts equal.
    Labels "alt" (n % S: with D = 3 every straddling column pair holds two species) and "rand" (random order, unequal
    sizes, species 1 exactly ONE atom -- a one-atom unit and a phantom column in its sorted block -- and, from three
    species on, the last label carried by nobody).  Every path forced as test_exact_parity.PATHS does and its kernel
    asserted from the timeline; float32 device slabs for the currents and the velocity self terms.  Frame counts
    SHORT_T + MID_T + LONG_T (the workgroup tiles 256 / 512 / 1024 of the three k_species_sum classes among them), every
    S = 1 ... 8, each class at its own tile edge (species_counts), D and A cycling with T; LOOPING: shapes whose workgroups
    loop, so that one partial sum mixes pairs of several species and k_species_sort's groups walk several units.
(b) The same with the weights of species s multiplied by 2^SHIFTS[s % 4]: each species' own sums stay exact, so the
    moments / currents (bit-equal), C_ii (2 ulps) and the self terms (the bound of (a)) hold to their own bounds while
    the neighbouring species are 2^24 ... 2^72 larger -- any leak between accumulator slots, pair halves, sorted blocks
    or shared transforms shows.  C_ij between species of different shift mixes scales inside Q_i +- Q_j by construction
    and is not exact: it is checked in (a) and (c) only (here: symmetric bit for bit, zero for an empty species).
(c) Float inputs, fft=True, against the long double references (difference first) at the lags of orc.lag_sample, per
    element within oracle.exact.fft_bound (C = 16, L the plan length, E the energy of the pseudo-particle columns that
    share a transform: fft_energy_bp over the S^2 pseudo-particles in slab order); off-diagonals 1/4 (B+ + B-) + u |C_ij|;
    self terms the sum of their atoms' bounds plus (N_s + 2) u |ref_s(k)| (<= (N_s + 2) u sum_n |ref_n(k)|: the smaller
    of the two, next to an FFT term a hundred times larger).  The cross term is referred to the moments / currents the
    call returned (the bound of the correlation stage alone, as test_conductivity_fft_error_model).  The worst ratio per
    analysis and plan is recorded (record_property "fft_ratio").

test_cpu_backend_*: the assertions of (a) and (b) minus the kernel names on _lib.Context("cpu"), which implements the
same entries independently: on a host without a GPU this is the check that references, budgets and bounds are
satisfiable at all, and it covers the CPU twin itself."""
import functools

import numpy as np
import pytest

import current_ref
import onsager_ref
from oracle import exact as ex
from oracle import numpy_oracle as orc
from species_self_ref import SELF_MSD, SELF_VACF, self_at_lags
from test_exact_parity import ALL_T, LONG_T, MID_T, MSD_OFFSET, SHIFTS, SHORT_T, fft_plan_length, needs_longdouble, ratios, shape
from transport_analysis_amd import _lib

gpu = pytest.mark.gpu
U = ex.U
LD = np.longdouble

# the workgroup tile of each k_species_sum class (256 threads x 4 / 2 / 1 rows): both species counts of the class there
EDGE_S = {1023: (1, 2), 1024: (1, 2), 1025: (1, 2), 511: (3, 4), 512: (3, 4), 513: (3, 4), 255: (5, 8), 256: (5, 8), 257: (5, 8)}


def species_counts(T):
    """The species counts run at T frames: both of a class at its tile edge, else 1 ... 8 cycling along ALL_T."""
    return EDGE_S.get(T, (1 + ALL_T.index(T) % 8,))


def grid_shape(T, S):
    """(A, D): D = 1, 2, 3 cycling with T as test_exact_parity.shape does, A = S + 4 + T % 4 (odd and even counts)."""
    return S + 4 + T % 4, shape(T)[1]


def make_labels(kind, A, S, seed):
    """"alt": n % S.  "rand": a random order with unequal sizes; species 1 is ONE atom (S >= 2), label S - 1 is carried by
    nobody (S >= 3), every other species has at least one atom and species 0 about two thirds of the rest."""
    if kind == "alt":
        return (np.arange(A) % S).astype(np.int32)
    rng = np.random.default_rng(seed)
    rest = [0] + list(range(2, S - 1))
    lab = ([1] if S >= 2 else []) + rest
    extra = A - len(lab)
    assert extra >= 2, (A, S)
    p = np.array([2.0 * len(rest)] + [1.0] * (len(rest) - 1))
    lab = np.array(lab + list(rng.choice(rest, size=extra, p=p / p.sum())), dtype=np.int32)
    return rng.permutation(lab).astype(np.int32)


# ------------------------------------------------------------------------------------------- (a), (b): integer inputs
@functools.lru_cache(maxsize=None)
def int_slab(kind, T, A, D):
    """("pos": walks at 2^30 with a drift; "vel" / "vel32": velocities up to 1000 / 12 (float32 device slabs), nonzero
    integer weights up to 3), read-only."""
    seed = 13 * T + 7 * A + D
    if kind == "pos":
        y = ex.int_walk(T, A, D, 5, seed, drift=1, offset=MSD_OFFSET)
    else:
        y = ex.int_velocities(T, A, D, 12 if kind == "vel32" else 1000, seed)
    q = ex.int_charges(A, 3, seed + 1)
    y.setflags(write=False)
    q.setflags(write=False)
    return y, q


@functools.lru_cache(maxsize=None)
def int_case(kind, T, A, D, S, labels):
    """(y, q, lab, Q (S, T, D) int64, P (T, S^2, D) int64) with the budget asserted for every series that enters a sum."""
    y, q = int_slab(kind, T, A, D)
    lab = make_labels(labels, A, S, seed=T + A + S)
    shift = kind == "pos"
    Q = ex.species_moment_exact(y, q, lab, S, shift=shift)
    P = ex.pseudo_particles(Q)
    ex.budget(q[None, :, None] * (y - y[0] if shift else y), A * D * T)
    ex.budget(Q, D * T)
    ex.budget(P, D * T)
    if kind == "vel32":  # a float32 slab holds the values themselves; every sum after it is float64
        assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
    return y, q, lab, Q, P


@functools.lru_cache(maxsize=None)
def cross_numerators(kind, T, A, D, S, labels):
    """(T, S^2) exact numerators of the pseudo-particles' lag sums."""
    Q = int_case(kind, T, A, D, S, labels)[3]
    return ex.pseudo_num(Q, acf=kind != "pos")


@functools.lru_cache(maxsize=None)
def atom_numerators(kind, T, A, D):
    """(T, A) exact numerators of w_n^2 f_n(k): the per-atom MSD or VACF numerators times the squared integer weight."""
    y, q = int_slab(kind, T, A, D)
    qi = np.rint(q).astype(np.int64)
    return (ex.msd_num(y) if kind == "pos" else ex.vacf_num(y)) * (qi * qi)[None, :]


def species_shifts(S, hetero):
    return np.array([SHIFTS[s % 4] if hetero else 0 for s in range(S)])


def check_sums(got, Q, sh, what):
    want = Q.astype(np.float64) * np.ldexp(1.0, sh)[:, None, None]
    assert got.shape == want.shape, (what, got.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "species, frame, dim", bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def check_cross(C, R, Q, sh, acf, plain, what):
    """C (T, S, S) against the exact numerators R (T, S^2) of the unscaled inputs; `plain`: the off-diagonals too."""
    T, S = C.shape[0], C.shape[1]
    den = ex.lag_den(T)
    assert np.array_equal(C, C.transpose(0, 2, 1)), (what, "both triangles must be bit-equal")
    if not acf:
        assert not C[0].any(), (what, "the moments' lag 0 must be exactly 0")
    for i in range(S):
        if not Q[i].any():  # an empty species (or an all-zero sum): its row and column exactly 0
            assert not C[:, i, :].any() and not C[:, :, i].any(), (what, "species", i, "has an all-zero sum")
        want = ex.divide(R[:, i * S + i], den) * np.ldexp(1.0, 2 * sh[i])
        u = ex.ulps(C[:, i, i], want)
        k = int(np.argmax(u))
        assert u.max() <= 2, (what, "C_ii: species", i, "lag", k, u[k], C[k, i, i], want[k])
    if not plain:
        return
    for i in range(S):
        for j in range(i + 1, S):
            rp, rm = R[:, i * S + j], R[:, j * S + i]
            ref = (rp - rm).astype(LD) / (4 * den).astype(LD)
            bound = U * (np.abs(rp) + np.abs(rm)).astype(np.float64) / den + U * np.abs(C[:, i, j])
            err = np.abs(C[:, i, j].astype(LD) - ref).astype(np.float64)
            k = int(np.argmax(err - bound))
            assert np.all(err <= bound), (what, "C_ij: pair", (i, j), "lag", k, err[k], bound[k])


def check_self(got, counts, num, lab, sh, msd, what):
    """(S, T) self terms against the (T, A) exact numerators of the unscaled inputs."""
    T, S = num.shape[0], got.shape[0]
    den = ex.lag_den(T)
    assert np.array_equal(counts, np.bincount(lab, minlength=S)), (what, counts)
    for s in range(S):
        sel = np.flatnonzero(lab == s)
        if not sel.size:
            assert not got[s].any(), (what, "species", s, "has no atoms: exact zeros")
            continue
        scale = np.ldexp(1.0, 2 * int(sh[s]))
        want_n = ex.divide(num[:, sel], den[:, None])
        ref = num[:, sel].sum(axis=1).astype(LD) / den.astype(LD) * LD(scale)
        bound = (sel.size + 2) * U * np.abs(want_n).sum(axis=1) * scale
        err = np.abs(got[s].astype(LD) - ref).astype(np.float64)
        k = int(np.argmax(err - bound))
        assert np.all(err <= bound), (what, "self: species", s, "lag", k, err[k], bound[k])
        if msd:
            assert got[s, 0] == 0.0, (what, "the MSD's lag 0 must be exactly 0")


def context(slab, options, device=0):
    """test_exact_parity.context for one slab, on a GPU or on the CPU backend (which takes no kernel options)."""
    T, A, D = slab.shape
    c = _lib.Context(device)
    if not c.is_cpu:
        for key, val in options.items():
            c.set_option(key, val)
    dtype = np.float32 if options.get("stage_device_f32") else np.float64
    (view,) = c.stage_alloc(T, A, D, dtype=dtype)
    view[:] = slab
    c.stage_commit(0, T)
    if not c.is_cpu:
        c.set_option("timeline", 1)
    return c


def timeline(c):
    return [n for n, _ in c.kernel_timeline(64)]


def default_vacf_kernel(T):
    """the windowed VACF's default dispatch on a float64 slab (api.hip: direct_form)"""
    return "k_short" if T <= 64 else "k_direct" if T < 97 else "k_mid" if T <= 512 else "k_band_bp_vacf"


def slab_kind(analysis, options):
    if analysis in ("onsager", "self_msd"):
        return "pos"
    return "vel32" if options.get("stage_device_f32") else "vel"


def units_loop(c, lab, S):
    """k_species_sort's units (two atoms of one species) against its groups (pm_read.hpp: pm_unit_grid)"""
    import torch

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    pitch = c.stage_device(0)[1]
    n_tb = -(-pitch // 1024)
    units = int(((np.bincount(lab, minlength=S) + 1) // 2).sum())
    return units > max(1, min(-(-16 * n_cu // n_tb), units, 65535))


def exact_case(analysis, fft, options, kernel, T, A, D, species, label_kinds=("alt", "rand"), device=0, sort_loops=False):
    """One path at one shape on ONE context: every species count, both label kinds, plain and with the species 2^s apart
    (labels and weights are arguments of the calls).  kernel: a name, or a function of T; None: no timeline (CPU)."""
    kind = slab_kind(analysis, options)
    y, q = int_slab(kind, T, A, D)
    c = context(y, options, device)
    try:
        for S in species:
            for labels in label_kinds:
                _, _, lab, Q, _ = int_case(kind, T, A, D, S, labels)
                for hetero in (False, True):
                    sh = species_shifts(S, hetero)
                    w = q * np.ldexp(1.0, sh)[lab]
                    what = (analysis, fft, kernel if isinstance(kernel, (str, type(None))) else kernel(T), T, A, D, S, labels,
                            "hetero" if hetero else "plain", options)
                    if analysis in ("onsager", "current"):
                        acf = analysis == "current"
                        sums, C = (c.current if acf else c.onsager)(fft, lab, n_species=S, weights=w)
                        names = None if c.is_cpu else timeline(c)
                        check_sums(sums, Q, sh, what)
                        check_cross(C, cross_numerators(kind, T, A, D, S, labels), Q, sh, acf, not hetero, what)
                        want = {"k_species_current" if acf else "k_species_moment", "k_sum_partials"}
                        if acf or T >= 2:  # (one frame of moments: lag 0 alone, nothing to correlate)
                            want |= {"k_onsager_combos", "k_current_finish" if acf else "k_onsager_finish", what[2]}
                    else:
                        msd = analysis == "self_msd"
                        got, counts = c.species_self(SELF_MSD if msd else SELF_VACF, fft, lab, n_species=S, weights=w)
                        names = None if c.is_cpu else timeline(c)
                        check_self(got, counts, atom_numerators(kind, T, A, D), lab, sh, msd, what)
                        want = {"k_species_sort", what[2]}
                        if sort_loops:
                            assert units_loop(c, lab, S), (what, "k_species_sort's groups must walk several units")
                    if names is not None:
                        assert want <= set(names), (what, names)
                        # a float32 slab is read as it is by the current pass and by the sort pass
                        assert "k_widen_f32" not in names, (what, names)
    finally:
        c.close()


# (id, analysis, fft, options, frame counts, kernel)
PATHS = [
    ("onsager-k_short", "onsager", 0, {}, SHORT_T, "k_short"),
    ("onsager-fft-k_short", "onsager", 1, {}, SHORT_T, "k_short"),
    ("onsager-k_mid", "onsager", 0, {}, MID_T, "k_mid"),
    ("onsager-k_direct", "onsager", 0, {"direct_mfma": 0}, ALL_T, "k_direct"),
    ("onsager-k_direct-default", "onsager", 0, {}, LONG_T, "k_direct"),
    ("current-k_short", "current", 0, {}, SHORT_T, "k_short"),
    ("current-fft-k_short", "current", 1, {}, SHORT_T, "k_short"),
    ("current-k_mid", "current", 0, {"mid_all": 1}, MID_T, "k_mid"),
    ("current-k_direct", "current", 0, {"direct_mfma": 0}, ALL_T, "k_direct"),
    ("current-k_band_bp_vacf", "current", 0, {"direct_mfma": 3}, ALL_T, "k_band_bp_vacf"),
    ("current-k_band_bp_vacf-default", "current", 0, {}, LONG_T, "k_band_bp_vacf"),
    ("self_msd-k_short", "self_msd", 0, {}, SHORT_T, "k_short"),
    ("self_msd-fft-k_short", "self_msd", 1, {}, SHORT_T, "k_short"),
    ("self_msd-k_mid", "self_msd", 0, {}, MID_T, "k_mid"),
    ("self_msd-k_direct", "self_msd", 0, {"direct_mfma": 0}, ALL_T, "k_direct"),
    ("self_msd-k_direct-default", "self_msd", 0, {}, LONG_T, "k_direct"),
    ("self_vacf-k_short", "self_vacf", 0, {}, SHORT_T, "k_short"),
    ("self_vacf-k_mid", "self_vacf", 0, {"mid_all": 1}, MID_T, "k_mid"),
    ("self_vacf-k_direct", "self_vacf", 0, {"direct_mfma": 0}, ALL_T, "k_direct"),
    ("self_vacf-k_band_bp_vacf", "self_vacf", 0, {"direct_mfma": 3}, ALL_T, "k_band_bp_vacf"),
    ("self_vacf-k_band_bp_vacf-default", "self_vacf", 0, {}, LONG_T, "k_band_bp_vacf"),
    # float32 device slabs: k_species_current and k_species_sort read them as they are; what follows is float64, by the
    # default dispatch (test_species_self_shapes.lag_kernels; k_short, k_direct, k_mid, k_band_bp_vacf along ALL_T)
    ("f32slab-current", "current", 0, {"stage_device_f32": 1}, ALL_T, default_vacf_kernel),
    ("f32slab-self_vacf", "self_vacf", 0, {"stage_device_f32": 1}, ALL_T, default_vacf_kernel),
]

# shapes whose workgroups loop: (id, T, A, D, S, labels, k_species_sort's groups walk several units)
LOOPING = [
    ("odd_cols_d3_s2", 1100, 1501, 3, 2, "alt", False),
    ("straddle_d3_s3", 513, 700, 3, 3, "alt", False),
    ("odd_blocks_d1_s5", 257, 2101, 1, 5, "alt", False),
    ("d2_s7", 300, 1100, 2, 7, "rand", False),
    ("sort_units_loop_s8", 48, 20011, 3, 8, "rand", True),
]
# (analysis, options, kernel at a frame count)
LOOP_RUNS = [
    ("onsager", {}, lambda T: "k_short" if T <= 64 else "k_mid" if T <= 512 else "k_direct"),
    ("current", {}, default_vacf_kernel),
    ("self_msd", {}, lambda T: "k_short" if T <= 64 else "k_mid" if T <= 512 else "k_direct"),
    ("self_vacf", {}, default_vacf_kernel),
    ("self_vacf", {"stage_device_f32": 1}, default_vacf_kernel),
]


def test_every_species_count_and_tile_edge_is_reached():
    """S = 1 ... 8 all occur, S = 6 and 7 on the short, the mid and (7: the looping case) the long side, and each
    k_species_sum class -- <2, 4, 1>, <4, 2, 2>, <8, 1, 4>: 1024, 512, 256 frames per workgroup -- meets its tile edge
    with both of its species counts."""
    seen = {S for T in ALL_T for S in species_counts(T)} | {c[4] for c in LOOPING}
    assert seen == set(range(1, 9))
    assert {6, 7} <= {S for T in SHORT_T for S in species_counts(T)}
    assert {6, 7} <= {S for T in MID_T for S in species_counts(T)}
    assert 6 in {S for T in LONG_T for S in species_counts(T)} and 7 in {c[4] for c in LOOPING}
    for edge, pair in ((1024, (1, 2)), (512, (3, 4)), (256, (5, 8))):
        for T in (edge - 1, edge, edge + 1):
            assert T in ALL_T and species_counts(T) == pair
    for T in ALL_T:
        for S in species_counts(T):
            lab = make_labels("rand", grid_shape(T, S)[0], S, seed=T)
            counts = np.bincount(lab, minlength=S)
            assert counts.sum() == grid_shape(T, S)[0] and (S < 2 or counts[1] == 1) and (S < 3 or counts[S - 1] == 0)
            assert all(counts[s] >= 1 for s in range(S) if not (S >= 3 and s == S - 1))


def test_budget_holds_for_every_case():
    """Exactness is a condition: oracle.exact.budget on w (y - y[0]) over A D T terms and on the moments / currents and
    the pseudo-particle series over D T terms, for every case of (a) and (b) (int_case asserts it)."""
    for kind in ("pos", "vel", "vel32"):
        for T in ALL_T:
            for S in species_counts(T):
                for labels in ("alt", "rand"):
                    int_case(kind, T, *grid_shape(T, S), S, labels)
        for _, T, A, D, S, labels, _ in LOOPING:
            int_case(kind, T, A, D, S, labels)


@gpu
@pytest.mark.parametrize("analysis,fft,options,frames,kernel", [pytest.param(*p[1:], id=p[0]) for p in PATHS])
def test_species_paths_exact_on_integers(analysis, fft, options, frames, kernel):
    for T in frames:
        for S in species_counts(T):  # (A depends on S: one context per species count)
            exact_case(analysis, fft, options, kernel, T, *grid_shape(T, S), (S,))


@gpu
@pytest.mark.parametrize("analysis,options,kernel", [pytest.param(*r, id=f"{r[0]}{'-f32slab' if r[1] else ''}") for r in LOOP_RUNS])
@pytest.mark.parametrize("T,A,D,S,labels,sort_loops", [pytest.param(*c[1:], id=c[0]) for c in LOOPING])
def test_species_paths_exact_where_workgroups_loop(T, A, D, S, labels, sort_loops, analysis, options, kernel):
    """Each k_species_sum group takes several pairs (of several species: one partial sum mixes them), k_species_sort's
    groups walk several units in the last case, with neighbouring species 2^12 ... 2^36 apart in scale."""
    n_pairs = (A * D + 1) // 2
    assert n_pairs > 1024, "more pairs than k_species_sum has groups at most (species_sum_parts)"
    exact_case(analysis, 0, options, kernel, T, A, D, (S,), label_kinds=(labels,),
               sort_loops=sort_loops and analysis.startswith("self"))


@pytest.mark.parametrize("analysis", ["onsager", "current", "self_msd", "self_vacf"])
def test_cpu_backend_exact_on_integers(analysis):
    """(a) and (b) on the CPU backend, fft=False (its direct forms; its FFT is no exact path), at every frame count."""
    for T in ALL_T:
        for S in species_counts(T):
            exact_case(analysis, 0, {}, None, T, *grid_shape(T, S), (S,), device="cpu")


@pytest.mark.parametrize("analysis", ["onsager", "current", "self_msd", "self_vacf"])
def test_cpu_backend_exact_at_a_looping_shape(analysis):
    _, T, A, D, S, labels, _ = LOOPING[3]
    exact_case(analysis, 0, {}, None, T, A, D, (S,), label_kinds=(labels,), device="cpu")


# ------------------------------------------------------------------------------------------------ (c): float inputs
FFT_T = [65, 513, 1100, 2049, 10300]
FFT_S = [2, 3, 8]
FFT_A = 200


@functools.lru_cache(maxsize=4)
def float_case(kind, T, S):
    """(y, lab, w): onsager_ref.species_walk moved to +1e4 with a shared drift, or current_ref.species_velocities."""
    if kind == "pos":
        y, lab, w = onsager_ref.species_walk(T, FFT_A + T % 3, S, seed=T + S, D=3, drift=3.0)
        y = y + 9000.0
    else:
        y, lab, w = current_ref.species_velocities(T, FFT_A + T % 3, S, seed=T + S, D=3)
    for a in (y, lab, w):
        a.setflags(write=False)
    return y, lab, w


def record_ratio(record_property, analysis, T, S, **r):
    r = {k: float(v) for k, v in r.items()}
    print(f"    fft_ratio {analysis} T={T} S={S} {_lib.fft_plan_info(T)}: {r}")
    record_property("fft_ratio", {"analysis": analysis, "S": S, "plan": str(_lib.fft_plan_info(T)), **r})


@gpu
@needs_longdouble
@pytest.mark.parametrize("S", FFT_S)
@pytest.mark.parametrize("T", FFT_T)
@pytest.mark.parametrize("analysis", ["onsager", "current"])
def test_cross_fft_error_model(analysis, T, S, record_property):
    """C[k, i, j] with fft=True per lag and pair, against the long double cross term of the sums the call returned: the
    diagonal within fft_bound of pseudo-particle i S + i, E over the pseudo-particles 2 m, 2 m + 1 that share a
    transform in slab order; the off-diagonals within 1/4 (B+ + B-) + u |C_ij|."""
    acf = analysis == "current"
    y, lab, w = float_case("vel" if acf else "pos", T, S)
    c = context(y, {})
    try:
        sums, C = (c.current if acf else c.onsager)(1, lab, n_species=S, weights=w)
        names = timeline(c)
    finally:
        c.close()
    assert {"k_onsager_combos", "k_winverse" if T > 512 else "k_w1_bp"} <= set(names), names
    assert ("k_msd_prepare" in names) == (not acf), names
    lags = orc.lag_sample(T)
    ref = (current_ref if acf else onsager_ref).cross_at_lags(sums, lags)
    # the pseudo-particles as k_onsager_combos forms them: one IEEE addition each
    P = np.empty((T, S * S, 3))
    for i in range(S):
        for j in range(S):
            P[:, i * S + j] = sums[i] if i == j else sums[i] + sums[j] if i < j else sums[i] - sums[j]
    E = ex.fft_energy_bp(ex.column_energy(P).sum(axis=1))
    S1 = None if acf else ex.s1_float(P).sum(axis=2)
    B = ex.fft_bound(T, fft_plan_length(T), E, S1)[lags]  # (lags, S^2)
    assert np.array_equal(C, C.transpose(0, 2, 1))
    r_diag = r_off = 0.0
    for i in range(S):
        r_diag = max(r_diag, ratios(C[lags, i, i], ref[:, i, i], B[:, i * S + i]).max())
        for j in range(i + 1, S):
            b = 0.25 * (B[:, i * S + j] + B[:, j * S + i]) + U * np.abs(C[lags, i, j])
            r_off = max(r_off, ratios(C[lags, i, j], ref[:, i, j], b).max())
    record_ratio(record_property, analysis, T, S, diag=r_diag, off=r_off)
    assert r_diag <= 1.0 and r_off <= 1.0, (r_diag, r_off)


@gpu
@needs_longdouble
@pytest.mark.parametrize("S", FFT_S)
@pytest.mark.parametrize("T", FFT_T)
@pytest.mark.parametrize("quantity", [pytest.param(SELF_MSD, id="msd"), pytest.param(SELF_VACF, id="vacf")])
def test_self_fft_error_model(quantity, T, S, record_property):
    """self_s(k) with fft=True per lag and species, against species_self_ref.self_at_lags: within the sum of its atoms'
    fft_bound (linear in E and S1: the bound of the summed energies; a lag sum's columns share no transform with another
    species' block) plus (N_s + 2) u |ref_s(k)|."""
    msd = quantity == SELF_MSD
    y, lab, w = float_case("pos" if msd else "vel", T, S)
    c = context(y, {})
    try:
        got, counts = c.species_self(quantity, 1, lab, n_species=S, weights=w)
        names = timeline(c)
    finally:
        c.close()
    assert {"k_species_sort", "k_w1_accum" if T <= 512 else "k_wsplit_accum"} <= set(names), names
    assert ("k_msd_prepare" in names) == msd, names
    assert np.array_equal(counts, np.bincount(lab, minlength=S))
    lags = orc.lag_sample(T)
    ref = self_at_lags(y, lab, w, S, quantity, lags)
    a = w[None, :, None] * (y - y[0] if msd else y)
    e = ex.column_energy(a).sum(axis=1)  # (A,)
    S1 = ex.s1_float(a).sum(axis=2) if msd else None  # (T, A)
    L = fft_plan_length(T)
    worst = 0.0
    for s in range(S):
        sel = np.flatnonzero(lab == s)
        b = ex.fft_bound(T, L, e[sel].sum(), S1[:, sel].sum(axis=1) if msd else None)[lags]
        b = b + (sel.size + 2) * U * np.abs(ref[s])
        worst = max(worst, ratios(got[s][lags], ref[s], b).max())
        if msd:
            assert got[s, 0] == 0.0
    record_ratio(record_property, "self_msd" if msd else "self_vacf", T, S, self=worst)
    assert worst <= 1.0, worst
