"""ta_partial_density and ta_partial_cross (PartialScattering's density and cross term) at EVERY lag, every wavevector and
every pair of species against exact sums (oracle/exact.py: partial_exact), as test_exact_kspace holds ta_scatter and
test_exact_species the Onsager cross term; their helpers are used, not copied.

partial_ref.assert_cross compares a dozen lags at 1e-10 of max(cross_aa(0), cross_bb(0)): an off-diagonal element at a long
lag of a large wavevector, orders of magnitude below that, a neighbouring wavevector's leak into a small one and the batches
of partial_cross are not held by it at all.  Here every element has a bar of its own.

The slab of the cross term (api.hip, partial_cross).  A batch of Kx wavevectors -- all K of a call unless the option
"partial_cross_chunk" n sets min(n, K) -- is ONE by-particle evaluation of Kx S^2 pseudo-particles of two columns:
wavevector b's at slab positions b S^2 + i S + j, holding rho_i (i == j), rho_i + rho_j (i < j), rho_i - rho_j (i > j)
(k_onsager_combos).  On the FFT forms pseudo-particles 2 m and 2 m + 1 OF THE SLAB share a transform (oracle.exact.
fft_energy_bp): with odd S^2 the last of wavevector b and the first of b + 1, and which ones meet depends on the batch.
batch_energy models exactly that: fft_energy_bp over each batch's energies in slab order.  The CPU backend evaluates each
wavevector by itself (cpu_backend.cpp, partial_cross: one current_cross per wavevector): batches of one.

(a) Exact inputs: integer walks, wavevectors k = 2 pi q with q in multiples of 1/4 (test_exact_kspace.SCATTER_Q, q = 0 among
    them), integer weights or none, labels "alt" and "rand" of test_exact_species.make_labels (a one-atom species, from
    three species on a label nobody carries).  Every phase factor is one of 1, i, -1, -i, so densities and lag-sum
    numerators are integers.  The exactness is a CONDITION, asserted without a GPU (test_budget_holds_for_every_case):
    oracle.exact.budget on the weighted terms of a density sum over A terms, and on the pseudo-particle series over 2 T
    terms (two columns, T frames).  The float32 slab holds positions alone and every sum behind it is float64
    (species_density.hip: "double are[ST][KC][F], aim[ST][KC][F]"), so the float32 path sums nothing in float32: its
    condition is that the positions survive the round trip through float32, asserted next to the budgets.
      * density: bit-equal to the integers -- k_species_density adds w_n cs by "fma(wn, cs.x, are[a][jl][f])" with cs one of
        0, +-1 (phase_math.hpp at quarter turns, as test_phase_exact_at_quarter_turns holds k_phase), every partial sum an
        integer below 2^53, and k_sum_partials adds integers.  An empty species: exact zeros.  Both slab types and
        "partial_chunk" 1, 2, 0 the same bits.
      * cross[j, k, a, a] on the direct by-particle forms: within 2 ulps of the correctly rounded num / (T - k), exactly 0
        where the numerator is 0 (k_partial_finish copies "row[i * S + i]" through; the by-particle bar of
        test_exact_kspace.check_by_particle).  On the FFT forms: oracle.exact.fft_bound(T, L, E), E = batch_energy.
      * cross[j, k, a, b], a != b, against 1/4 (R+ - R-) with R+- = num[a S + b], num[b S + a] over T - k, exact rationals in
        long double.  k_partial_finish is k_cross_finish: "0.25 * (row[lo * S + hi] - row[hi * S + lo])"; each row element
        within 2 ulps <= 4 u |R| of its rational, one rounding of the subtraction u |r+ - r-| = 4 u |C_ab|, the factor 1/4
        exact (test_exact_species' docstring): u (|R+| + |R-|) + u |C_ab|.  FFT forms: 1/4 (B+ + B-) + u |C_ab| with B+-
        the FFT bounds of the two pseudo-particles.  k_onsager_combos forms rho_a +- rho_b without rounding (integers).
      * both triangles bit-equal; row and column of a species whose density is all zero exactly 0.
      * the kernels from the timeline: k_species_density, k_onsager_combos, k_partial_finish, the by-particle kernel of
        test_exact_kspace.by_particle_kernel; no k_widen_f32.
      * "partial_cross_chunk" 1, 2 (a last batch of ONE wavevector), 3 and 0 at K = 5: k_partial_finish launched ceil(K / n)
        times, every run within the bars of ITS batches, and the same bits wherever the batches cannot change what a
        pseudo-particle shares a transform with: on the direct forms (a particle's lag sums do not depend on its
        neighbours); on the multi-pass FFT forms beyond 512 frames (a pseudo-particle has two columns, an even number, so
        its transforms are its own: oracle.exact.fft_energy_bp's docstring; the bound still takes the pair's energy, which
        is no smaller); and on the one-pass form k_w1_bp whenever n S^2 is even (every batch starts at an even slab
        position, so the pairs 2 m, 2 m + 1 are those of the unbatched slab).  With n S^2 odd k_w1_bp inverts P_a + i P_b
        with another b in another batching and rounds a's result differently: there the bars hold in every batching and
        the bits need not agree (on the MI355X they do not: T = 65, S = 7, n = 1 and 3).
(b) The same with the weights of species s multiplied by 2^SHIFTS[s % 4]: each species' own sums stay exact, density stays
    bit-equal and the diagonals keep their own bars next to neighbours 2^24 ... 2^72 larger (on an FFT form: the bar of the
    transform the diagonal's pseudo-particle shares).  Off-diagonals between species of different shift mix scales inside
    rho_a +- rho_b: symmetric bit for bit and zero for an empty species, no more (test_exact_species (b)); between species of
    the SAME shift (a and a + 4) they scale exactly and are held as in (a).
(c) Leaks between wavevectors: ta_partial_cross on random integer densities (K, S, T, 2) in [-40, 40], wavevector j scaled
    by 2^SHIFTS[j % 4].  Every element of wavevector j, off-diagonals included, scales exactly by 2^(2 s_j): all bars of
    (a) per wavevector, on the GPU and on the CPU backend; on the GPU at odd S^2 once more with "partial_cross_chunk" 2.
(d) Float inputs (partial_ref.case), GPU and CPU backend, every lag, against the long-double defining sum of the RETURNED
    density per pseudo-particle p (p formed exactly): with u = 2^-53,
      * direct: (2 (T - k) + 6) u sum_t |p_t| |p_t+k| / (T - k), the by-particle bound of test_exact_kspace for a pseudo-atom
        of two columns;
      * FFT: fft_bound with batch_energy;
      * off the diagonal the library holds fl(rho_a +- rho_b), one rounding per component, |delta| <= u |p|: the lag sum
        moves by sum_t (|delta_t| |p_t+k| + |p_t| |delta_t+k|) <= 2 u sum_t |p_t| |p_t+k| / (T - k), added to that
        pseudo-particle's bound; then 1/4 (B+ + B-) + u |C_ab| as in (a).
    The CPU backend runs (a) and (b) at these bounds (its phase, cos / sin of fl(2 pi) r, is 1e-16 off at quarter turns):
    density within partial_ref.density_bar of the integers, the cross term against the density it returned.

The worst error / bound per family and form is recorded (record_property "partial_ratio") and printed."""
import functools

import numpy as np
import pytest

import partial_ref
from oracle import exact as ex
from test_exact_kspace import (BACKENDS, SCATTER_Q, SHIFTS, SLABS, assert_ratio, by_particle_kernel, check_by_particle, cross_abs,
                               fft_length, gpu, is_fft_form, ld_acf, needs_longdouble, ratios, staged, timeline)
from test_exact_species import make_labels, species_shifts
from transport_analysis_amd import _lib

LD = np.longdouble
U = ex.U

# (T, S, K, D): every frame count at which the by-particle dispatch changes form, S = 1 ... 8 cycling (each meets a direct
# form with fft = 0 and, beyond 64 frames, an FFT form with fft = 1), D = 1, 2, 3 cycling, K in 1, 3, 5; A = S + 4 + T % 4
FRAMES = [1, 2, 3, 48, 49, 64, 65, 96, 97, 256, 257, 512, 513, 1025, 2049]
K_CYCLE = [1, 3, 5, 1, 3, 5, 5, 1, 3, 5, 3, 1, 5, 3, 1]
CASES = [(T, 1 + i % 8, K_CYCLE[i], 1 + i % 3, 1 + i % 8 + 4 + T % 4) for i, T in enumerate(FRAMES)]
OUTER = (10300, 2, 1, 3, 3)  # the outer radix; three atoms: labels "alt" alone
VARIANTS = [("alt", False), ("alt", True), ("rand", False), ("rand", True)]  # (labels, weighted)


def variants(case):
    return VARIANTS[:2] if case == OUTER else VARIANTS


def test_every_form_meets_an_odd_slab():
    """S = 1 ... 8 all occur beyond 64 frames (an FFT form) and at every length (a direct form); K = 5 -- the batches of
    "partial_cross_chunk" -- on k_short, on a one-pass FFT form and on a multi-pass one; odd S^2 with K >= 2 on the FFT forms
    up to 256 frames and beyond 512."""
    assert {S for T, S, *_ in CASES if T > 64} == set(range(1, 9))
    assert {K for _, _, K, _, _ in CASES} == {1, 3, 5} and {D for *_, D, _ in CASES} == {1, 2, 3}
    assert any(64 < T <= 256 and S % 2 and K >= 2 for T, S, K, _, _ in CASES)
    assert any(T > 512 and S % 2 and K >= 2 for T, S, K, _, _ in CASES)
    assert {T for T, _, K, _, _ in CASES if K == 5} >= {3, 64, 65, 256, 513}


@pytest.mark.parametrize("device", BACKENDS)
def test_partial_cross_chunk_refuses_a_negative_count(device):
    c = _lib.Context(device)
    try:
        for n in (0, 1, 7):
            c.set_option("partial_cross_chunk", n)
        with pytest.raises(_lib.TAError, match="partial_cross_chunk"):
            c.set_option("partial_cross_chunk", -1)
    finally:
        c.close()


def note(record_property, family, form, ratio):
    """record and print the error / bound of one (family, form)"""
    record_property("partial_ratio", {"family": family, "form": form, "ratio": float(ratio)})
    print(f"partial_ratio {family} {form} {ratio:.4f}")


# ------------------------------------------------------------------------------------------------------- the slab's model
def batches(K, n):
    """[(first wavevector, count)] of partial_cross with n wavevectors per batch"""
    return [(j0, min(n, K - j0)) for j0 in range(0, K, n)]


def pseudo(rho_j, dtype=np.float64):
    """(T, S^2, 2): one wavevector's pseudo-particles of a (S, T, 2) density in slab order, one addition each in `dtype`"""
    r = np.asarray(rho_j, dtype=dtype)
    S, T, _ = r.shape
    P = np.empty((T, S * S, 2), dtype=dtype)
    for i in range(S):
        for j in range(S):
            P[:, i * S + j] = r[i] if i == j else r[i] + r[j] if i < j else r[i] - r[j]
    return P


def batch_energy(rho, n):
    """(K, S^2): E of every pseudo-particle of a (K, S, T, 2) density evaluated n wavevectors per batch -- the energy of
    the pair 2 m, 2 m + 1 of ITS batch's slab (module docstring)"""
    K, S = rho.shape[:2]
    e = np.stack([(pseudo(rho[j]) ** 2).sum(axis=(0, 2)) for j in range(K)])  # (K, S^2)
    out = np.empty_like(e)
    for j0, kx in batches(K, n):
        out[j0:j0 + kx] = ex.fft_energy_bp(e[j0:j0 + kx].ravel()).reshape(kx, S * S)
    return out


def batch_of(device, K, chunk=0):
    """the wavevectors per batch on `device`: all K on the GPU (the budget rule is far away at these shapes) or min(chunk,
    K); one on the CPU backend"""
    return 1 if device == "cpu" else min(chunk, K) if chunk else K


def assert_zero_species(cross_j, rho_j, what):
    for a in range(rho_j.shape[0]):
        if not np.any(rho_j[a]):
            assert not cross_j[:, a, :].any() and not cross_j[:, :, a].any(), (what, "species", a, "has an all-zero density")


# ----------------------------------------------------------------------------------------------- bars on exact inputs
def check_exact_cross(cross, rho, num, sh, fft_form, L, batch, what):
    """cross (K, T, S, S) of the integer density rho (K, S, T, 2) whose species a of wavevector j is scaled by 2^sh[j, a],
    against the exact numerators num (K, T, S^2) of the UNSCALED density (module docstring (a); off-diagonals where both
    species carry the same shift).  -> {"diag": worst error / bar, "off": ...}"""
    K, T, S, _ = cross.shape
    den = ex.lag_den(T)
    denf = den.astype(LD)
    assert np.array_equal(cross, cross.transpose(0, 1, 3, 2)), (what, "both triangles must be bit-equal")
    scaled = rho.astype(np.float64) * np.ldexp(1.0, sh)[:, :, None, None]
    B = ex.fft_bound(T, L, batch_energy(scaled, batch)) if fft_form else None  # (T, K, S^2)
    worst = {"diag": 0.0, "off": 0.0}
    for j in range(K):
        C = cross[j]
        assert_zero_species(C, rho[j], (what, j))
        sc2 = np.ldexp(1.0, 2 * sh[j])
        d = np.arange(S) * S + np.arange(S)
        got = C[:, np.arange(S), np.arange(S)]
        if fft_form:
            want = num[j][:, d].astype(LD) * sc2[None, :] / denf[:, None]
            r = assert_ratio(ratios(got, want, B[:, j][:, d]), (what, "diag", j))
        else:
            r = check_by_particle(got / sc2[None, :], num[j][:, d], (what, "diag", j))
        worst["diag"] = max(worst["diag"], r)
        for a in range(S):
            for b in range(a + 1, S):
                if sh[j, a] != sh[j, b]:
                    continue
                rp, rm = num[j][:, a * S + b], num[j][:, b * S + a]
                ref = (rp - rm).astype(LD) * sc2[a] / (4 * denf)
                if fft_form:
                    bound = 0.25 * (B[:, j, a * S + b] + B[:, j, b * S + a]) + U * np.abs(C[:, a, b])
                else:
                    bound = U * (np.abs(rp) + np.abs(rm)).astype(np.float64) * sc2[a] / den + U * np.abs(C[:, a, b])
                worst["off"] = max(worst["off"], assert_ratio(ratios(C[:, a, b], ref, bound), (what, "off", j, a, b)))
    return worst


# ------------------------------------------------------------------------------------------------ bars on float inputs
def check_float_cross(cross, rho, fft_form, L, batch, what):
    """cross (K, T, S, S) against the long-double defining sum of the RETURNED density rho (K, S, T, 2), per pseudo-particle
    (module docstring (d)).  -> {"diag": ..., "off": ...}"""
    K, T, S, _ = cross.shape
    den = ex.lag_den(T).astype(np.float64)[:, None]
    assert np.array_equal(cross, cross.transpose(0, 1, 3, 2)), (what, "both triangles must be bit-equal")
    E = ex.fft_bound(T, L, batch_energy(rho, batch)) if fft_form else None  # (T, K, S^2)
    offd = np.array([i != j for i in range(S) for j in range(S)])
    worst = {"diag": 0.0, "off": 0.0}
    for j in range(K):
        C = cross[j]
        assert_zero_species(C, rho[j], (what, j))
        P = pseudo(rho[j], LD)
        R = ld_acf(P) / den.astype(LD)  # (T, S^2)
        a_abs = np.abs(P).astype(np.float64)
        absum = cross_abs(a_abs, a_abs) / 2 / den  # sum_t |p_t| |p_t+k| / (T - k), both columns
        B = E[:, j] if fft_form else (2 * den + 6) * U * absum
        B = B + np.where(offd[None, :], 2 * U * absum, 0.0)
        d = np.arange(S) * S + np.arange(S)
        r = assert_ratio(ratios(C[:, np.arange(S), np.arange(S)], R[:, d], B[:, d]), (what, "diag", j))
        worst["diag"] = max(worst["diag"], r)
        for a in range(S):
            for b in range(a + 1, S):
                ref = (R[:, a * S + b] - R[:, b * S + a]) / 4
                bound = 0.25 * (B[:, a * S + b] + B[:, b * S + a]) + U * np.abs(C[:, a, b])
                worst["off"] = max(worst["off"], assert_ratio(ratios(C[:, a, b], ref, bound), (what, "off", j, a, b)))
    return worst


def note_both(record_property, family, form, worst):
    note(record_property, family + " diag", form, worst["diag"])
    note(record_property, family + " off", form, worst["off"])


# ======================================================================================================== (a), (b): cases
@functools.lru_cache(maxsize=None)
def exact_case(T, S, K, D, A, labels, weighted):
    """(x, k, w or None, lab, density (K, S, T, 2) int64, numerators (K, T, S^2) int64), the budgets asserted; computed once,
    not to be modified"""
    seed = 13 * T + A + D
    x = ex.int_walk(T, A, D, 1, seed)
    q = np.array(SCATTER_Q[D][:K])
    w = ex.int_charges(A, 3, seed + 1) if weighted else None
    lab = make_labels(labels, A, S, seed=T + A + S)
    rho, num = ex.partial_exact(x, w, lab, S, q)
    ex.budget(np.ones(A) if w is None else w, A)  # the terms w_n (0, +-1) of a density sum
    ex.budget(rho, 2 * T)
    ex.budget(np.stack([pseudo(rho[j], np.int64) for j in range(K)]), 2 * T)
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)  # what the float32 slab holds
    out = (x, ex.quarter_wavevectors(q), w, lab, rho, num)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def shifted(case, hetero):
    """(weights or None, shifts (K, S)) of a case with the species 2^SHIFTS[s % 4] apart, or as they are"""
    x, k, w, lab, rho, _ = case
    S = rho.shape[1]
    sh = species_shifts(S, hetero)
    ww = (np.ones(x.shape[1]) if w is None else w) * np.ldexp(1.0, sh)[lab] if hetero else w
    return ww, np.broadcast_to(sh, (len(k), S))


def case_id(c):
    return "T{}-S{}-K{}-D{}-A{}".format(*c)


def test_budget_holds_for_every_case():
    """Exactness is a condition (module docstring (a)): exact_case and cross_talk_case assert oracle.exact.budget on every
    series that enters a sum, and that the positions are float32 values."""
    for c in CASES + [OUTER]:
        for labels, weighted in variants(c):
            exact_case(*c, labels, weighted)
    for T, S, K in XT_CASES:
        cross_talk_case(T, S, K)


def run_exact_gpu(case_key, labels, weighted, hetero, record_property):
    T, S, K, D, A = case_key
    case = exact_case(*case_key, labels, weighted)
    x, k, _, lab, rho, num = case
    w, sh = shifted(case, hetero)
    want_rho = rho.astype(np.float64) * np.ldexp(1.0, sh)[:, :, None, None]
    L = fft_length(T, 0)
    KC = _lib.partial_density_tile(S)["KC"]
    family = "species apart" if hetero else "exact"
    first = {}
    for dtype in SLABS:
        c = staged(0, [x], dtype)
        try:
            runs = []
            for chunk in (1, 2, 0) if K > 1 else (0,):
                c.set_option("partial_chunk", chunk)
                runs.append(c.partial_density(0, k, lab, S, w, cross=False)[0])
                assert c.kernel_launches("k_species_density") == -(-K // min(chunk or KC, KC)), chunk
            assert all(np.array_equal(runs[0], r) for r in runs[1:]), "partial_chunk changes the density"
            bad = np.argwhere(runs[0] != want_rho)
            assert bad.size == 0, (dtype.__name__, "density: wavevector, species, frame, part", bad[:5].tolist())
            for fft in (0, 1):
                what = f"T={T} S={S} K={K} {labels} fft={fft} {dtype.__name__}"
                fft_form = is_fft_form(0, T, fft, True)
                form = "fft" if fft_form else by_particle_kernel(T, fft)
                got = {}
                for n in (1, 2, 3, 0) if K == 5 else (0,):
                    c.set_option("partial_cross_chunk", n)
                    dens, got[n] = c.partial_density(fft, k, lab, S, w)
                    assert c.kernel_launches("k_partial_finish") == (-(-K // n) if n else 1), n
                    assert np.array_equal(dens, want_rho), (what, "density next to the cross term")
                    note_both(record_property, family, form,
                              check_exact_cross(got[n], rho, num, sh, fft_form, L, batch_of(0, K, n), (what, "chunk", n)))
                names = timeline(c)
                want = {"k_species_density", "k_onsager_combos", "k_partial_finish", by_particle_kernel(T, fft)}
                assert want <= set(names) and "k_widen_f32" not in names, (what, names)
                same = {n: np.array_equal(got[0], g) for n, g in got.items()}
                print(f"partial_bits {what} S^2={S * S} batches equal: {same}")
                for n, equal in same.items():  # (module docstring: where the batches cannot change a transform's pair)
                    if not fft_form or by_particle_kernel(T, fft) != "k_w1_bp" or (n * S * S) % 2 == 0:
                        assert equal, (what, "partial_cross_chunk changes the bits", n, same)
                if fft in first:
                    assert np.array_equal(first[fft], got[0]), (what, "slab types differ")
                first.setdefault(fft, got[0])
        finally:
            c.close()


def run_exact_cpu(case_key, labels, weighted, hetero, record_property):
    """(a) / (b) on the CPU backend at the bounds of (d)"""
    T, S, K, D, A = case_key
    case = exact_case(*case_key, labels, weighted)
    x, k, _, lab, rho, _ = case
    w, sh = shifted(case, hetero)
    want_rho = rho.astype(LD) * np.ldexp(1.0, sh).astype(LD)[:, :, None, None]
    bar = partial_ref.density_bar(x, w, lab, S, k)
    L = fft_length(T, "cpu")
    c = staged("cpu", [x])
    try:
        c.set_option("partial_cross_chunk", 2)  # accepted and ignored, as "partial_chunk" is
        for fft in (0, 1):
            what = f"cpu T={T} S={S} K={K} {labels} fft={fft}"
            dens, cross = c.partial_density(fft, k, lab, S, w)
            err = np.max(np.abs(dens.astype(LD) - want_rho), axis=(0, 2, 3)).astype(np.float64)
            assert np.all(err <= bar), (what, "density", err, bar)
            for a in range(S):
                if not np.any(lab == a):
                    assert not dens[:, a].any(), (what, "an empty species' density is not exactly zero", a)
            fft_form = is_fft_form("cpu", T, fft, True)
            note_both(record_property, "cpu " + ("species apart" if hetero else "quarter"), "fft" if fft_form else "direct",
                      check_float_cross(cross, dens, fft_form, L, 1, what))
    finally:
        c.close()


@gpu
@needs_longdouble
@pytest.mark.parametrize("labels,weighted", [pytest.param(*v, id=f"{v[0]}-{'w' if v[1] else 'now'}") for v in VARIANTS])
@pytest.mark.parametrize("case", [pytest.param(c, id=case_id(c)) for c in CASES])
def test_partial_exact(case, labels, weighted, record_property):
    """(a): density bit-equal to the Gaussian integers, every cross[j, k, a, b] at its own bar, both slab types, fft 0 and 1,
    "partial_chunk" and (K = 5) "partial_cross_chunk" the same result"""
    run_exact_gpu(case, labels, weighted, False, record_property)


@gpu
@needs_longdouble
@pytest.mark.parametrize("labels,weighted", [pytest.param(*v, id=f"{v[0]}-{'w' if v[1] else 'now'}") for v in VARIANTS])
@pytest.mark.parametrize("case", [pytest.param(c, id=case_id(c)) for c in CASES])
def test_partial_exact_species_apart(case, labels, weighted, record_property):
    """(b): the weights of species s times 2^SHIFTS[s % 4]"""
    run_exact_gpu(case, labels, weighted, True, record_property)


@gpu
@needs_longdouble
@pytest.mark.parametrize("hetero", [False, True], ids=["plain", "apart"])
@pytest.mark.parametrize("weighted", [False, True], ids=["now", "w"])
def test_partial_exact_outer_radix(weighted, hetero, record_property):
    """(a) and (b) at 10300 frames, three atoms, two species, one wavevector: the outer radix of the FFT forms"""
    run_exact_gpu(OUTER, "alt", weighted, hetero, record_property)


@needs_longdouble
@pytest.mark.parametrize("hetero", [False, True], ids=["plain", "apart"])
@pytest.mark.parametrize("case", [pytest.param(c, id=case_id(c)) for c in CASES[::2] if c[0] <= 513])
def test_partial_quarter_turns_on_the_cpu_backend(case, hetero, record_property):
    """(a) and (b) on the CPU backend: on a host without a GPU the check that references, budgets and bounds are
    satisfiable (up to 513 frames: the long-double reference of all lags is quadratic in the frames)"""
    for labels, weighted in (("alt", False), ("rand", True)):
        run_exact_cpu(case, labels, weighted, hetero, record_property)


# ================================================================================ (c) no cross-talk between wavevectors
XT_CASES = [(T, S, K) for T in (49, 200, 513) for S in (1, 2, 3, 5, 8) for K in (2, 5)]


@functools.lru_cache(maxsize=None)
def cross_talk_case(T, S, K):
    """(density (K, S, T, 2) of integers in [-40, 40], numerators (K, T, S^2)); S >= 3: the last species all zero in
    wavevector 1"""
    rng = np.random.default_rng(31 * T + 7 * S + K)
    rho = rng.integers(-40, 41, size=(K, S, T, 2))
    if S >= 3:
        rho[1, S - 1] = 0
    P = np.stack([pseudo(rho[j], np.int64) for j in range(K)])
    ex.budget(P, 2 * T)
    num = np.stack([ex.pair_acf_num(P[j]) for j in range(K)])
    rho.setflags(write=False)
    num.setflags(write=False)
    return rho, num


@needs_longdouble
@pytest.mark.parametrize("device", BACKENDS)
@pytest.mark.parametrize("T,S,K", [pytest.param(*c, id="T{}-S{}-K{}".format(*c)) for c in XT_CASES])
def test_partial_cross_no_cross_talk(T, S, K, device, record_property):
    """(c): ta_partial_cross with wavevector j scaled by 2^SHIFTS[j % 4]: every element of every wavevector at the bars of
    (a) next to neighbours 2^24 ... 2^72 larger; on the GPU with odd S^2 also two wavevectors per batch, where other
    pseudo-particles share a transform"""
    rho, num = cross_talk_case(T, S, K)
    sh = np.broadcast_to(np.array([SHIFTS[j % 4] for j in range(K)])[:, None], (K, S))
    scaled = rho.astype(np.float64) * np.ldexp(1.0, sh)[:, :, None, None]
    L = fft_length(T, device)
    c = _lib.Context(device)
    try:
        if device != "cpu":
            c.set_option("timeline", 1)
        for chunk in (0, 2) if device != "cpu" and S % 2 else (0,):
            c.set_option("partial_cross_chunk", chunk)
            for fft in (0, 1):
                cross = c.partial_cross(scaled, fft)
                if device != "cpu":
                    assert c.kernel_launches("k_partial_finish") == (-(-K // chunk) if chunk else 1), chunk
                fft_form = is_fft_form(device, T, fft, True)
                what = f"{device} T={T} S={S} K={K} fft={fft} chunk={chunk}"
                note_both(record_property, f"{device} cross-talk", "fft" if fft_form else "direct",
                          check_exact_cross(cross, rho, num, sh, fft_form, L, batch_of(device, K, chunk), what))
    finally:
        c.close()


# ====================================================================================================== (d) float inputs
FLOAT_CASES = [(T, 12 + T % 5, 1 + i % 3, 3, S) for i, T in enumerate((65, 300, 1100)) for S in (2, 3)]  # (T, A, D, K, S)


@needs_longdouble
@pytest.mark.parametrize("device", BACKENDS)
@pytest.mark.parametrize("T,A,D,K,S", [pytest.param(*c, id="T{}-A{}-D{}-K{}-S{}".format(*c)) for c in FLOAT_CASES])
def test_partial_float_every_lag(T, A, D, K, S, device, record_property):
    """(d): partial_ref's walks, dyadic weights and interleaved labels; every lag of every pair of every wavevector against
    the long-double defining sum of the returned density; the density within partial_ref's bar"""
    ref = partial_ref.case(T, A, D, K, S)
    x, w, lab, k = ref[:4]
    L = fft_length(T, device)
    c = staged(device, [x])
    try:
        for fft in (0, 1):
            dens, cross = c.partial_density(fft, k, lab, S, w)
            partial_ref.assert_density(dens, ref, f"{device} fft={fft}")
            fft_form = is_fft_form(device, T, fft, True)
            note_both(record_property, f"{device} float", "fft" if fft_form else "direct",
                      check_float_cross(cross, dens, fft_form, L, batch_of(device, K), f"{device} T={T} S={S} fft={fft}"))
    finally:
        c.close()
