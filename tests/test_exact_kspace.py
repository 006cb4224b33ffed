"""ta_scatter, ta_kcurrent and ta_orient (and the correlate entries behind them) at EVERY lag and every wavevector against
exact sums (oracle/exact.py), as test_exact_parity / test_exact_species / test_fft_plans hold the correlators they sit on.

scatter_ref.assert_scatter, kcurrent_ref.assert_correlations and orient_ref.assert_orient compare a dozen lags with one
scale per call at 1e-10 of the largest element (for the self part: lag 0, n_atoms); the long lags of a large wavevector,
five orders of magnitude below that, are not checked by them at all.  Here every lag of every wavevector has a bar of its
own.

Exact inputs (tests 1 - 5).  Integer positions and wavevectors k = 2 pi q with q in multiples of 1/4
(exact.quarter_wavevectors asserts on the host that k / 2 pi gives q back): every phase factor is one of 1, i, -1, -i, so
densities, currents and lag-sum numerators are integers (exact.scatter_exact, current_exact); molecules whose orientation
vector is exactly +-e_x, +-e_y, +-e_z (exact.axis_molecules, orient_exact).  Every case runs on a float64 and a float32
device slab holding the same integers: the two must agree bit for bit.

The bars on exact inputs, and where they are wider than "2 ulps of the correctly rounded quotient":

  * by-particle values (coll, long, trans: ONE by-particle evaluation of the VACF dispatch) with fft = 0, and with fft = 1
    up to 64 frames (k_short): 2 ulps, as test_exact_parity.check_bp holds the VACF's by-particle elements.
  * lag sums (self, c1, c2, orient's coll: ONE lag-sum evaluation) on the matrix-core form (from 513 frames,
    k_band_bp_vacf): 2 ulps, and exactly 0 where the numerator is 0 -- k_bandbp_gather adds the integer partials of all
    particle blocks and divides ONCE (bandbp_kernels.hpp, "lagsum[k] = ... factor * (t / (double)(T - k))").
  * lag sums on the other direct forms: (A + 2) u sum_n |num_n| / (T - k) with num_n the exact numerator of atom n, the
    bar test_exact_parity.check_lag_sums derives for the VACF.  These forms do NOT scale an exact total once: k_direct
    divides per atom and adds the quotients (direct_kernels.hpp, "double val = ... / (double)(T - k)" followed by
    "ts_out[k] += val"), k_short scales each wave's partial by the rounded reciprocal rn[k] = fl(1 / (T - k)) before
    k_sum_partials adds the waves (short_kernels.hpp, "prow[k] = s * rn[k]"), k_mid each workgroup's
    (mid_kernels.hpp, "prow[tid] = ... tot0 * rn[tid]"), the CPU backend divides per atom (cpu_backend.cpp, direct_t:
    "acc /= (double)(T - k)").  A partial is two roundings at most, 2 u |partial|; adding P <= A of them costs
    (P - 1) u sum |partial|; sum |partial| <= sum_n |num_n| / (T - k).  Where the atoms' numerators cancel (the self part
    of a large wavevector at a long lag) that is more than 2 ulps of the small total, and nothing less holds for these
    forms; where they do not cancel (q = 0: every numerator is T - k) it is (A + 2) / 2 ulps.  The bar is zero, so the
    value exactly 0, where every atom's numerator is 0.
  * FFT forms: exact.fft_bound as test_fft_plans applies it to the VACF (C = 16, L = 2 M of the plan): lag sums with
    E the energy of all columns (|z| = 1: exactly n_atoms n_frames for the self part), by-particle values with
    exact.fft_energy_bp (pseudo-atoms 2 m and 2 m + 1 share a transform).
  * trans = (bp[jT_0] + bp[jT_1] + ...) / (D - 1) (kcur_finish): every quotient has its 2 ulps, each addition one rounding
    of the partial sum, D - 1 is 1 or 2 (an exact division; one more ulp is allowed as for a general divisor).
  * c2: Q's diagonal holds fl(1 - fl(1/3)) and -fl(1/3) (orient_q: fma(u_j, u_j, -third)), relative errors of at most
    1.5 u and u, so a product of two entries is off by at most 3 u of itself; the 3 (T - k) N non-zero products of a lag
    are summed in some order over 2 N pseudo-atoms: (3 + 3 (T - k) N + 2 N + 6) u sum |terms| / (T - k), with
    sum |terms| = 2/3 n_same + 5/9 n_diff exactly (same axis: 4/9 + 1/9 + 1/9; different axes: 2/9 + 2/9 + 1/9).

Float inputs, GPU and CPU backend.  The walks of scatter_ref, kcurrent_ref and orient_ref, all lags, np.longdouble
references.  The CPU backend forms the phase by an expression of its own (cos and sin of fl(2 pi) r, 1e-16 off at quarter
turns), so it runs the exact inputs above at THESE bounds (test_*_on_the_cpu_backend), not bit for bit; its direct sums of
integers are exact, and it runs the cross-talk test as the GPU does.  With u = 2^-53 and eps = (2 pi (D + 2) U + 8) u
the phase bound of ta_hip.h:

  * self: A (2 eps + (4 (T - k) + A + 6) u) -- each cos(phi' - phi) carries both phases' errors, the direct form of a
    slab with two columns per atom the rest; with fft = 1 (beyond 48 frames) 2 A eps + fft_bound(E = A T).
  * density, current, total: the bars ta_hip.h states (scatter_ref.density_bar, kcurrent_ref.current_bar,
    orient_ref.total_bar).  coll (both families), long and trans are compared with the long-double correlation of the
    series the call RETURNED, so no input term enters them; the by-particle direct bound of test_exact_parity (c) is
    (2 (T - k) + 6) u sum_t |a a'| / (T - k) for a pseudo-atom of two columns, orient's coll one atom of three in a lag
    sum: (3 (T - k) + 7) u sum |a a'| / (T - k).
  * long and trans: kcur_project forms k^ in float64 (|k|^2: D roundings, sqrt, division: under 4 u per component), jL in D
    roundings and every jT_d in one more: a projected value is within (D + 10) u n(t) of the exact projection of the
    returned current, n(t) = sum_d |current_d(t)| of its part.  That enters a lag as sum_t (delta_t |a_t+k| +
    delta_t+k |a_t|) / (T - k); behind it the by-particle bound above on each of the 1 + D pseudo-atoms, and for trans the
    D roundings of kcur_finish's sum.
  * c1, c2: every component of u within B_u u of the exact unit vector (ta_hip.h: B_u = 12 + 3 R, R = 0 without a box);
    Q's entries then within (2 B_u + 4) u (a square or a product of two components, the fl(1/3) or fl(sqrt 2), one
    rounding each); the input term as above, then the lag sum of N atoms of three columns (c2: 2 N pseudo-atoms) in any
    order: (3 N (T - k) + N + 6) u sum |terms| / (T - k) (c2: 6 N (T - k) + 2 N + 6).

The worst error / bound per family and form is recorded (record_property "kspace_ratio") and printed."""
import functools
import math

import numpy as np
import pytest

import kcurrent_ref
import orient_ref
import scatter_ref
from oracle import exact as ex
from transport_analysis_amd import _lib

gpu = pytest.mark.gpu
needs_longdouble = pytest.mark.skipif(not ex.longdouble_ok(), reason="np.longdouble has no 64-bit significand here")
LD = np.longdouble
U = ex.U
SLABS = (np.float64, np.float32)
BACKENDS = [pytest.param("cpu", id="cpu"), pytest.param(0, id="gpu", marks=gpu)]


# --------------------------------------------------------------------------------------------------------- plumbing
def staged(device, slabs, dtype=np.float64):
    """a context on `device` (0, or "cpu") with `slabs` staged in `dtype` and kept in that element type; the timeline on"""
    T, A, D = slabs[0].shape
    c = _lib.Context(device)
    if device != "cpu":
        c.set_option("stage_device_f32", int(dtype == np.float32))
    views = c.stage_alloc(T, A, D, n_slabs=len(slabs), dtype=dtype)
    for view, s in zip(views, slabs):
        view[:] = s
    c.stage_commit(0, T)
    if device != "cpu":
        c.set_option("timeline", 1)
    return c


def timeline(c):
    return [n for n, _ in c.kernel_timeline(64)]


def lag_sum_kernel(T, fft):
    """the kernel that ONE lag-sum evaluation of the VACF dispatch launches on a float64 slab (api.hip: fft_impl,
    direct_form with the default options)"""
    if T <= 48 or (not fft and T <= 64):
        return "k_short"
    if fft:
        return "k_w1_accum" if T <= 512 else "k_wsplit_accum"
    return "k_direct" if T <= 96 else "k_mid" if T <= 512 else "k_band_bp_vacf"


def by_particle_kernel(T, fft):
    """the kernel of ONE by-particle evaluation"""
    if T <= 64:
        return "k_short"
    if fft:
        return "k_w1_bp" if T <= 512 else "k_wsplit_accum"
    return "k_direct" if T <= 96 else "k_mid" if T <= 512 else "k_band_bp_vacf"


def is_fft_form(device, T, fft, by_particle):
    """fft = 1 runs an FFT: on the GPU beyond 64 frames by particle and beyond 48 for lag sums (k_short below: fft_impl);
    on the CPU backend at every length"""
    return bool(fft) and (device == "cpu" or T > (64 if by_particle else 48))


def fft_length(T, device):
    """L of the FFT bound: 2 M of the plan; the CPU backend pads to a power of two of at least 2 T"""
    L = 2 * _lib.fft_plan_info(T)["M"]
    return L if device != "cpu" else max(L, 1 << int(math.ceil(math.log2(max(2 * T, 2)))))


def note(record_property, family, form, ratio):
    """record and print the error / bound of one (family, form)"""
    record_property("kspace_ratio", {"family": family, "form": form, "ratio": float(ratio)})
    print(f"kspace_ratio {family} {form} {ratio:.4f}")


def ratios(got, want, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (np.abs(np.asarray(got, dtype=LD) - want) / bound).astype(np.float64)
    r[(np.asarray(bound) == 0) & (np.asarray(got, dtype=LD) == want)] = 0.0
    return np.nan_to_num(r, nan=np.inf)


def assert_ratio(r, what):
    worst = np.unravel_index(int(np.argmax(r)), r.shape) if r.size else ()
    assert r.size == 0 or r.max() <= 1.0, (what, "worst at", tuple(int(i) for i in worst), float(r.max()))
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------- the bars on exact inputs
def check_lag_sum(got, num_by_atom, kernel, what):
    """One lag-sum evaluation on exact inputs: got (T,), num_by_atom (T, A) the atoms' exact numerators.  -> the worst
    error / bar (module docstring: 2 ulps behind one division of the exact total, else (A + 2) u sum_n |num_n| / (T - k))"""
    T, A = num_by_atom.shape
    den = ex.lag_den(T)
    tot = num_by_atom.sum(axis=1)
    if kernel == "k_band_bp_vacf":
        u = ex.ulps(got, ex.divide(tot, den))
        assert u.max() <= 2, (what, kernel, "lag", int(np.argmax(u)), float(u.max()))
        return float(u.max()) / 2
    bound = (A + 2) * U * np.abs(num_by_atom).sum(axis=1).astype(LD) / den
    u = ex.ulps(got, ex.divide(tot, den))
    print(f"kspace_ulps {kernel} A={A} {float(np.max(u[np.isfinite(u)], initial=0.0)):.1f} nonzero_at_zero={int(np.isinf(u).sum())}")
    return assert_ratio(ratios(got, tot.astype(LD) / den, bound), (what, kernel))


def check_by_particle(got, num, what, max_ulps=2):
    """by-particle values (T, P) on exact inputs within max_ulps of the correctly rounded quotient, 0 exactly where the
    numerator is 0"""
    T = num.shape[0]
    u = ex.ulps(got, ex.divide(num, ex.lag_den(T)[:, None]))
    worst = np.unravel_index(int(np.argmax(u)), u.shape)
    assert u.max() <= max_ulps, (what, "lag, pseudo-atom", tuple(int(i) for i in worst), float(u.max()))
    return float(u.max()) / max_ulps


def check_fft_lag_sum(got, num_total, E, L, what):
    T = num_total.shape[0]
    return assert_ratio(ratios(got, num_total.astype(LD) / ex.lag_den(T), ex.fft_bound(T, L, E)), what)


def check_fft_by_particle(got, num, energy, L, what):
    """got, num (T, P); energy (P,) of the pseudo-atoms: 2 m and 2 m + 1 share a transform"""
    T = num.shape[0]
    return assert_ratio(ratios(got, num.astype(LD) / ex.lag_den(T)[:, None], ex.fft_bound(T, L, ex.fft_energy_bp(energy))), what)


# ================================================================================== 1. k_phase is exact at quarter turns
PHASE_Q = {
    1: [[0.25], [0.5], [0.75], [-0.25], [1.25], [2.5], [4.0], [-3.5], [0.0]],
    2: [[0.25, 0.0], [0.0, -0.75], [0.25, 0.5], [-0.75, 1.25], [0.5, 0.5], [2.5, -0.25], [0.0, 0.0]],
    3: [[0.0, 0.0, 0.25], [0.25, 0.5, -0.25], [-0.75, 1.25, 0.5], [0.5, 0.5, 0.5], [2.5, -0.5, 0.25], [-3.0, 0.25, 4.0],
        [0.0, 0.0, 0.0]],
}


def phase_positions(D, T=96):
    """one atom on integers of both signs: component 0 runs through -48 ... 47, the others through short cycles"""
    t = np.arange(T)
    cols = [t - T // 2, (3 * t) % 7 - 3, (5 * t) % 11 - 5]
    return np.stack(cols[:D], axis=1).astype(np.float64).reshape(T, 1, D)


@gpu
@pytest.mark.parametrize("dtype", SLABS, ids=["slab64", "slab32"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_phase_exact_at_quarter_turns(D, dtype):
    """One atom, so the density IS (cos, sin) of k_phase: bit-equal to 1, 0, -1 at every frame, for reduced arguments
    r = 0, +1/4, -1/4, +1/2 and -1/2 (sincospi at multiples of 1/2; a -0.0 equals 0.0)."""
    x = phase_positions(D)
    q = np.array(PHASE_Q[D])
    k = ex.quarter_wavevectors(q)
    u = np.einsum("kd,tnd->ktn", q, x)
    r = u - np.rint(u)
    assert set(np.unique(r).tolist()) == {-0.5, -0.25, 0.0, 0.25, 0.5}  # every residue, both signs
    assert set(np.unique(ex.quarter_phases(x, q)).tolist()) == {0, 1, 2, 3}
    c, s = ex.quarter_cs(x, q)
    c_ctx = staged(0, [x], dtype)
    try:
        _, rho, _ = c_ctx.scatter(0, k, self_part=False, collective=False)
        assert "k_phase" in timeline(c_ctx), timeline(c_ctx)
    finally:
        c_ctx.close()
    want = np.stack([c[:, :, 0], s[:, :, 0]], axis=2).astype(np.float64)
    bad = np.argwhere(rho != want)
    assert np.array_equal(rho, want), ("(wavevector, frame, part)", bad[:5].tolist(), rho[tuple(bad[0])] if len(bad) else None)


# ============================================================================================================ 2. scattering
SCATTER_T = [1, 2, 3, 47, 48, 49, 63, 64, 65, 96, 97, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049]
A_CYCLE = [1, 2, 7, 16, 33, 40, 21, 32]
SCATTER_Q = {  # an axis-aligned wavevector first, then a mixed one, then q = 0
    1: [[0.25], [0.5], [0.0], [-0.75], [2.5]],
    2: [[0.0, 0.25], [0.25, 0.5], [0.0, 0.0], [-0.75, 1.25], [2.5, -0.5]],
    3: [[0.0, 0.25, 0.0], [0.25, 0.5, -0.25], [0.0, 0.0, 0.0], [-0.75, 1.25, 0.5], [2.5, -0.5, 0.25]],
}


def scatter_shape(i):
    """(A, D, K): D = 1, 2, 3 and K = 1, 3, 5 in all nine combinations, odd and even atom counts from 1 to 40"""
    return A_CYCLE[i % len(A_CYCLE)], 1 + i % 3, (1, 3, 5)[(i // 3) % 3]


SCATTER_CASES = [(T,) + scatter_shape(i) for i, T in enumerate(SCATTER_T)] + [(10300, 3, 3, 1)]
assert {(D, K) for _, _, D, K in SCATTER_CASES} >= {(D, K) for D in (1, 2, 3) for K in (1, 3, 5)}


@functools.lru_cache(maxsize=None)
def scatter_case(T, A, D, K):
    """(x, q, k, density, self numerators by atom, coll numerators): walks with steps of -1, 0, 1 per component, so that
    consecutive phases are correlated; computed once, not to be modified"""
    x = ex.int_walk(T, A, D, 1, seed=13 * T + A + D)
    q = np.array(SCATTER_Q[D][:K])
    out = (x, q, ex.quarter_wavevectors(q)) + ex.scatter_exact(x, q)
    for a in out:
        a.setflags(write=False)
    return out


def check_scatter_exact(got, case, fft, L, what, record_property):
    x, q, k, rho, self_num, coll_num = case
    T, A, _ = x.shape
    fs, dens, coll = got
    assert np.array_equal(dens, rho.astype(np.float64)), (what, "density")
    kernel = lag_sum_kernel(T, fft)
    for j in range(len(q)):
        if fft and T > 48:
            r = check_fft_lag_sum(fs[j], self_num[j].sum(axis=1), float(A * T), L, (what, "self", j))
            note(record_property, "scatter self", "fft", r)
        else:
            r = check_lag_sum(fs[j], self_num[j], kernel, (what, "self", j))
            note(record_property, "scatter self", kernel, r)
    if fft and T > 64:
        e = (rho.astype(np.float64) ** 2).sum(axis=(1, 2))
        note(record_property, "scatter coll", "fft", check_fft_by_particle(coll.T, coll_num.T, e, L, (what, "coll")))
    else:
        note(record_property, "scatter coll", by_particle_kernel(T, fft), check_by_particle(coll.T, coll_num.T, (what, "coll")))


@gpu
@pytest.mark.parametrize("T,A,D,K", [pytest.param(*c, id="T{}-A{}-D{}-K{}".format(*c)) for c in SCATTER_CASES])
def test_scatter_exact(T, A, D, K, record_property):
    """density bit-equal to the Gaussian-integer sums; self and coll at all T lags for every wavevector (module docstring);
    "scatter_chunk" 1, 2 and automatic the same bits; the float32 slab the same bits as the float64 one; the lag kernels
    named from the timeline.  10300 x 3 x 1: the outer radix and eleven frame blocks."""
    case = scatter_case(T, A, D, K)
    x, k = case[0], case[2]
    L = fft_length(T, 0)
    first = {}
    for dtype in SLABS:
        c = staged(0, [x], dtype)
        try:
            for fft in (0, 1):
                runs = []
                for chunk in (1, 2, 0) if K > 1 else (0,):
                    c.set_option("scatter_chunk", chunk)
                    runs.append(c.scatter(fft, k))
                    assert c.kernel_launches("k_phase") == (-(-K // chunk) if chunk else 1), chunk
                for r in runs[1:]:
                    assert all(np.array_equal(a, b) for a, b in zip(runs[0], r)), ("chunks differ", fft)
                c.scatter(fft, k, density=False, collective=False)
                names = timeline(c)
                assert "k_phase" in names and lag_sum_kernel(T, fft) in names and "k_widen_f32" not in names, (fft, names)
                c.scatter(fft, k, self_part=False)
                names = timeline(c)
                assert by_particle_kernel(T, fft) in names and "k_scatter_transpose" in names, (fft, names)
                check_scatter_exact(runs[-1], case, fft, L, f"T={T} fft={fft} {dtype.__name__}", record_property)
                if fft in first:
                    assert all(np.array_equal(a, b) for a, b in zip(first[fft], runs[-1])), ("slab types differ", fft)
                first.setdefault(fft, runs[-1])
        finally:
            c.close()


# ============================================================================================================== 3. currents
KCUR_T = [1, 3, 48, 65, 97, 257, 511, 512, 513, 1025]
KCUR_Q = {  # the axis-aligned ones (one non-zero component) and the mixed ones alternate; none is zero
    1: [[0.25], [-0.5], [0.75], [-0.75], [1.25], [2.5], [0.5], [-1.25], [1.0]],
    2: [[0.25, 0.0], [0.25, 0.5], [0.0, -0.5], [-0.75, 1.25], [2.5, 0.0], [0.5, 0.5], [0.0, -1.25], [1.0, -0.25], [-0.75, 0.0]],
    3: [[0.25, 0.0, 0.0], [0.25, 0.5, -0.25], [0.0, -0.5, 0.0], [-0.75, 1.25, 0.5], [0.0, 0.0, 0.75], [0.5, 0.5, 0.0],
        [2.5, 0.0, 0.0], [1.0, -0.25, 2.0], [0.0, 0.0, -1.25]],
}


def kcur_shape(i):
    """(A, D, K, weighted): K = 1, 4, 5, 9 on both sides of the kernel's tile of wavevectors"""
    return A_CYCLE[(i + 2) % len(A_CYCLE)], 1 + i % 3, (1, 4, 5, 9, 9, 5, 4, 1, 5, 9)[i % 10], i % 2 == 0


KCUR_CASES = [(T,) + kcur_shape(i) for i, T in enumerate(KCUR_T)]
assert {K for *_, K, _ in KCUR_CASES} == {1, 4, 5, 9} and {D for _, _, D, _, _ in KCUR_CASES} == {1, 2, 3}


@functools.lru_cache(maxsize=None)
def kcur_case(T, A, D, K, weighted):
    """(x, v, w or None, q, k, current (K, T, D, 2) int64)"""
    seed = 17 * T + A + D
    x = ex.int_walk(T, A, D, 1, seed=seed)
    v = ex.int_velocities(T, A, D, 20, seed + 1)
    w = ex.int_charges(A, 3, seed + 2) if weighted else None
    q = np.array(KCUR_Q[D][:K])
    cur = ex.current_exact(x, v, w, q)
    ex.budget(cur, 2 * D * T)
    for a in (x, v, q, cur):
        a.setflags(write=False)
    return x, v, w, q, ex.quarter_wavevectors(q), cur


def one_axis(qj):
    """the index of the one non-zero component of an axis-aligned q, else None"""
    nz = np.flatnonzero(qj)
    return int(nz[0]) if len(nz) == 1 else None


def cross_abs(a, b):
    """(T, P): sum_t sum_c (a[t] b[t + k] + b[t] a[t + k]) of non-negative (T, P, C) arrays (float64: a bound's term)"""
    T = a.shape[0]
    out = np.zeros((T,) + a.shape[1:2])
    for k in range(T):
        out[k] = (a[:T - k] * b[k:] + b[:T - k] * a[k:]).sum(axis=(0, 2))
    return out


def ld_acf(a):
    """(T, P) long-double sum_t sum_c a[t] a[t + k] of a (T, P, C) series"""
    a = np.asarray(a, dtype=LD)
    T = a.shape[0]
    out = np.zeros((T,) + a.shape[1:2], dtype=LD)
    for k in range(T):
        out[k] = (a[:T - k] * a[k:]).sum(axis=(0, 2))
    return out


def projected_bounds(cur_j, kj, fft_form, L, T):
    """One wavevector's current (T, D, 2) -> (long reference (T,), trans reference (T,), long bound, trans bound), all lags,
    long double: the projection in long double, the (D + 10) u n(t) of kcur_project, then the by-particle bound of the
    form on each pseudo-atom and kcur_finish's sum (module docstring)."""
    D = cur_j.shape[1]
    den = ex.lag_den(T).astype(LD)
    jl, jt = kcurrent_ref.project(np.asarray(cur_j, dtype=LD)[None], np.asarray(kj)[None])
    series = np.concatenate([jl[0][:, None, :], jt[0]], axis=1) if D > 1 else jl[0][:, None, :]  # (T, S, 2)
    ref = ld_acf(series)  # (T, S)
    a_abs = np.abs(series).astype(np.float64)
    delta = np.broadcast_to(((D + 10) * U * np.abs(np.asarray(cur_j, dtype=np.float64)).sum(axis=1))[:, None, :], a_abs.shape)
    inp = cross_abs(a_abs, delta)
    absum = cross_abs(a_abs, a_abs) / 2
    if fft_form:
        # (a pseudo-atom may share a transform with a neighbour: the whole wavevector's energy covers its own, the caller
        # adds the neighbouring wavevectors')
        form = (ex.fft_bound(T, L, float((a_abs ** 2).sum())) * den)[:, None]
    else:
        form = (2 * den[:, None] + 6) * U * absum
    b = (inp + form) / den[:, None]
    lon_ref, lon_b = ref[:, 0] / den, b[:, 0]
    if D == 1:
        return lon_ref, np.zeros(T, dtype=LD), lon_b, np.zeros(T)
    tr_abs = (absum[:, 1:].sum(axis=1) / den).astype(np.float64)
    tr_b = (b[:, 1:].sum(axis=1) + (D + 1) * U * tr_abs) / (D - 1)
    return lon_ref, ref[:, 1:].sum(axis=1) / den / (D - 1), lon_b, tr_b


def check_kcur_exact(got, case, fft, L, what, record_property):
    x, v, w, q, k, cur = case
    T, _, D = x.shape
    g_cur, lon, tr = got
    assert np.array_equal(g_cur, cur.astype(np.float64)), (what, "current")
    den = ex.lag_den(T)
    exact_form = not (fft and T > 64)
    kernel = by_particle_kernel(T, fft)
    for j in range(len(q)):
        axis = one_axis(q[j])
        if D == 1:
            assert not np.any(tr[j]), (what, "D = 1: trans is zeros")
        if axis is not None and exact_form:
            num_l, num_t = ex.axis_current_num(cur[j], axis)
            note(record_property, "kcurrent long", kernel, check_by_particle(lon[j][:, None], num_l[:, None], (what, "long", j)))
            if D > 1:
                parts = ex.divide(num_t, den[:, None])
                bound = (2 * np.spacing(np.abs(parts)).sum(axis=1) + 2 * np.spacing(np.abs(parts.sum(axis=1)))) / (D - 1)
                want = num_t.sum(axis=1).astype(LD) / den / (D - 1)
                note(record_property, "kcurrent trans", kernel, assert_ratio(ratios(tr[j], want, bound), (what, "trans", j)))
            continue
        # a mixed wavevector, or an FFT form: the long-double projection of the exact current.  With fft the neighbours'
        # energy: pseudo-atoms j S - 1 and (j + 1) S may share a transform with this wavevector's first and last
        lon_ref, tr_ref, lon_b, tr_b = projected_bounds(cur[j], k[j], not exact_form, L, T)
        if not exact_form:
            near = sum(float((cur[i].astype(np.float64) ** 2).sum()) for i in (j - 1, j + 1) if 0 <= i < len(q))
            extra = ex.fft_bound(T, L, near)
            lon_b, tr_b = lon_b + extra, tr_b + (extra * D / (D - 1) if D > 1 else 0.0)
        form = "fft" if not exact_form else kernel + " mixed"
        note(record_property, "kcurrent long", form, assert_ratio(ratios(lon[j], lon_ref, lon_b), (what, "long", j)))
        if D > 1:
            note(record_property, "kcurrent trans", form, assert_ratio(ratios(tr[j], tr_ref, tr_b), (what, "trans", j)))


@gpu
@needs_longdouble
@pytest.mark.parametrize("T,A,D,K,weighted",
                         [pytest.param(*c, id="T{}-A{}-D{}-K{}-{}".format(*c[:4], "w" if c[4] else "now")) for c in KCUR_CASES])
def test_kcurrent_exact(T, A, D, K, weighted, record_property):
    """current bit-equal to the integer sums (every fma exact); long and trans at all lags: integer numerators for the
    axis-aligned wavevectors, the long-double projection of the exact current for the mixed ones; "kcurrent_chunk" 1 and
    automatic the same bits; both slab types the same bits; D = 1: trans all zeros."""
    case = kcur_case(T, A, D, K, weighted)
    x, v, w, _, k, _ = case
    L = fft_length(T, 0)
    KC = _lib.kcurrent_tile()["KC"]
    first = {}
    for dtype in SLABS:
        c = staged(0, [v, x], dtype)
        try:
            for fft in (0, 1):
                runs = []
                for chunk in (1, 0):
                    c.set_option("kcurrent_chunk", chunk)
                    runs.append(c.kcurrent(fft, k, w))
                    names = timeline(c)
                    assert c.kernel_launches("k_kcurrent") == -(-K // (chunk or KC)), (chunk, names)
                    assert {"k_kcurrent_project", "k_kcurrent_finish", by_particle_kernel(T, fft)} <= set(names), (fft, names)
                assert all(np.array_equal(a, b) for a, b in zip(*runs)), ("chunks differ", fft)
                check_kcur_exact(runs[-1], case, fft, L, f"T={T} fft={fft} {dtype.__name__}", record_property)
                if fft in first:
                    assert all(np.array_equal(a, b) for a, b in zip(first[fft], runs[-1])), ("slab types differ", fft)
                first.setdefault(fft, runs[-1])
        finally:
            c.close()


# ==================================================================== 4. no cross-talk between wavevectors (correlate entries)
XT_CASES = [(63, 4, 1), (65, 5, 2), (511, 9, 3), (513, 4, 3), (1023, 5, 2), (1025, 9, 1)]  # (T, K, D of the current)
SHIFTS = (0, -12, -24, -36)


def shifts(K):
    return np.array([SHIFTS[j % 4] for j in range(K)])


def xt_axis(j, D):
    return j % D


@functools.lru_cache(maxsize=None)
def xt_case(T, K, D):
    """integer densities (K, T, 2) and currents (K, T, D, 2) with their exact numerators, wavevector j along axis j mod D"""
    rng = np.random.default_rng(29 * T + K)
    rho = rng.integers(-40, 41, size=(K, T, 2)).astype(np.float64)
    cur = rng.integers(-40, 41, size=(K, T, D, 2)).astype(np.float64)
    q = np.zeros((K, D))
    for j in range(K):
        q[j, xt_axis(j, D)] = (0.25, -0.5, 0.75, 1.25)[j % 4]
    coll_num = ex.pair_acf_num(rho.transpose(1, 0, 2))  # (T, K)
    nums = [ex.axis_current_num(cur[j], xt_axis(j, D)) for j in range(K)]
    return rho, cur, ex.quarter_wavevectors(q), coll_num, nums


def check_xt(device, T, K, D, rho, cur, k, record_property, what):
    """ta_scatter_collective and ta_kcurrent_correlate on series scaled by 2^s_j: every wavevector at the bars of its own
    values (fft = 0: few ulps; fft = 1: the FFT bound with the energy of its own transform)"""
    _, _, _, coll_num, nums = xt_case(T, K, D)
    s = shifts(K)
    den = ex.lag_den(T)
    L = fft_length(T, device)
    scale2 = np.ldexp(1.0, 2 * s)
    c = _lib.Context(device)
    try:
        for fft in (0, 1):
            exact_form = not is_fft_form(device, T, fft, True)
            coll = c.scatter_collective(rho, fft)
            lon, tr = c.kcurrent_correlate(cur, k, fft)
            want = coll_num.astype(LD) * scale2[None, :]
            if exact_form:
                u = ex.ulps(coll.T, ex.divide(coll_num, den[:, None]) * scale2[None, :])
                assert u.max() <= 2, (what, fft, "coll: lag, wavevector", np.unravel_index(int(np.argmax(u)), u.shape), float(u.max()))
                note(record_property, "cross-talk coll", "direct", float(u.max()) / 2)
            else:
                e = (rho ** 2).sum(axis=(1, 2))
                b = ex.fft_bound(T, L, ex.fft_energy_bp(e))
                note(record_property, "cross-talk coll", "fft", assert_ratio(ratios(coll.T, want / den[:, None], b), (what, "coll")))
            # the pseudo-atoms of the current: (jL, jT_0 ... jT_D-1) per wavevector (D = 1: jL alone)
            S = 1 + D if D > 1 else 1
            e_ps = np.zeros(K * S)
            for j in range(K):
                ax = xt_axis(j, D)
                e_d = (cur[j] ** 2).sum(axis=(0, 2))  # (D,)
                e_ps[j * S] = e_d[ax]
                if D > 1:
                    e_ps[j * S + 1:(j + 1) * S] = np.where(np.arange(D) == ax, 0.0, e_d)
            b_ps = ex.fft_bound(T, L, ex.fft_energy_bp(e_ps))  # (T, K S)
            for j in range(K):
                num_l, num_t = nums[j]
                sc = scale2[j]
                if D == 1:
                    assert not np.any(tr[j])
                if exact_form:
                    u = ex.ulps(lon[j], ex.divide(num_l, den) * sc)
                    assert u.max() <= 2, (what, fft, "long", j, int(np.argmax(u)), float(u.max()))
                    if D > 1:
                        parts = ex.divide(num_t, den[:, None]) * sc
                        bound = (2 * np.spacing(np.abs(parts)).sum(axis=1) + 2 * np.spacing(np.abs(parts.sum(axis=1)))) / (D - 1)
                        wt = num_t.sum(axis=1).astype(LD) * sc / den / (D - 1)
                        note(record_property, "cross-talk trans", "direct", assert_ratio(ratios(tr[j], wt, bound), (what, "trans", j)))
                else:
                    wl = num_l.astype(LD) * sc / den
                    note(record_property, "cross-talk long", "fft", assert_ratio(ratios(lon[j], wl, b_ps[:, j * S]), (what, "long", j)))
                    if D > 1:
                        wt = num_t.sum(axis=1).astype(LD) * sc / den / (D - 1)
                        bt = (b_ps[:, j * S + 1:(j + 1) * S].sum(axis=1) + (D + 1) * U * np.abs(num_t).sum(axis=1) * sc / den) / (D - 1)
                        note(record_property, "cross-talk trans", "fft", assert_ratio(ratios(tr[j], wt, bt), (what, "trans", j)))
    finally:
        c.close()


@needs_longdouble
@pytest.mark.parametrize("device", BACKENDS)
@pytest.mark.parametrize("T,K,D", [pytest.param(*c, id="T{}-K{}-D{}".format(*c)) for c in XT_CASES])
def test_correlate_entries_no_cross_talk(T, K, D, device, record_property):
    """Wavevector j's series scaled by 2^s_j, s_j = 0, -12, -24, -36 cycling (the device of test_exact_parity (b)): every
    sum stays exact, so coll, long and trans of each wavevector keep their own few-ulp bar next to neighbours 2^24 ... 2^72
    larger; with fft = 1 the FFT bound with the energy of the transform a pseudo-atom shares."""
    rho, cur, k, _, _ = xt_case(T, K, D)
    f = np.ldexp(1.0, shifts(K))
    check_xt(device, T, K, D, rho * f[:, None, None], cur * f[:, None, None, None], k, record_property, f"T={T} K={K} D={D}")


# ============================================================================================================ 5. orientation
ORIENT_CASES = [  # (T, n_vectors, mode, box: None / "const" / "frames", weighted)
    (1, 1, "bond", None, False), (2, 2, "normal", "const", True), (49, 7, "bisector", "frames", True),
    (64, 33, "bond", "const", True), (65, 2, "bisector", None, False), (97, 33, "normal", "frames", True),
    (257, 7, "bond", "frames", False), (513, 33, "bisector", "const", True), (600, 7, "normal", None, True),
    (1025, 1, "normal", "const", True), (1025, 2, "bond", None, True),
]
assert {c[1] for c in ORIENT_CASES} == {1, 2, 7, 33}
assert {(c[2], c[3]) for c in ORIENT_CASES} >= {(m, b) for m in orient_ref.MODES for b in ("const", "frames")}


@functools.lru_cache(maxsize=None)
def orient_case(T, N, mode, box, weighted):
    """(x, index, dimensions or None, weights or None, exact.orient_exact(...), u (T, N, 3) int64)"""
    seed = 31 * T + N
    lengths = None if box is None else np.full(T, 16) if box == "const" else np.where(np.arange(T) % 3 == 0, 32, 16)
    x, idx, u = ex.axis_molecules(T, N, mode, seed, box=lengths)
    dims = None if box is None else np.column_stack([lengths, lengths, lengths, np.full((T, 3), 90.0)]).astype(np.float64)
    w = ex.int_charges(N, 3, seed + 1) if weighted else None
    if N >= 7:
        assert (np.abs(u).sum(axis=2) == 0).any()  # some degenerate vectors
    if box is not None:  # the wrapping has cut some molecules: the image step has work to do
        raw = x[:, idx[:, 1]] - x[:, idx[:, 0]]
        assert T < 49 or (np.abs(raw) > 8).any()
    return x, idx, dims, w, ex.orient_exact(u, w), u


def check_orient_exact(got, case, fft, L, what, record_property):
    (c1_num, n_same, n_diff, total, coll_num) = case[4]
    T, N = c1_num.shape
    c1, c2, tot, coll = got
    den = ex.lag_den(T)
    kernel = lag_sum_kernel(T, fft)
    assert np.array_equal(tot, total.astype(np.float64)), (what, "total")
    e_total = float((total.astype(np.float64) ** 2).sum())
    if fft and T > 48:
        # (lag 0 of c1: the frames with a direction, the energy of u)
        note(record_property, "orient c1", "fft", check_fft_lag_sum(c1, c1_num.sum(axis=1), float(c1_num[0].sum()), L, (what, "c1")))
        note(record_property, "orient coll", "fft", check_fft_lag_sum(coll, coll_num, e_total, L, (what, "coll")))
    else:
        note(record_property, "orient c1", kernel, check_lag_sum(c1, c1_num, kernel, (what, "c1")))
        note(record_property, "orient coll", kernel, check_lag_sum(coll, coll_num[:, None], kernel, (what, "coll")))
    # c2 = (2/3 n_same - 1/3 n_diff) / (T - k): the exact rational in long double (2 n_same - n_diff is an integer)
    want = (2 * n_same - n_diff).astype(LD) / 3 / den
    terms = (6 * n_same + 5 * n_diff).astype(LD) / 9  # sum |terms| of the lag
    if fft and T > 48:
        # the energy of Q: 4/9 + 1/9 + 1/9 = 2/3 per frame with a direction; the fl(1/3) as for the direct form
        b = ex.fft_bound(T, L, 2.0 / 3.0 * float(c1_num[0].sum())) + 3 * U * terms / den
        note(record_property, "orient c2", "fft", assert_ratio(ratios(c2, want, b), (what, "c2")))
    else:
        b = (3 + 3 * den * N + 2 * N + 6) * U * terms / den
        note(record_property, "orient c2", kernel, assert_ratio(ratios(c2, want, b), (what, "c2")))


@gpu
@needs_longdouble
@pytest.mark.parametrize("T,N,mode,box,weighted",
                         [pytest.param(*c, id="T{}-N{}-{}-{}".format(c[0], c[1], c[2], c[3] or "nobox")) for c in ORIENT_CASES])
def test_orient_exact(T, N, mode, box, weighted, record_property):
    """Unit vectors exactly along the axes (bond, normal and bisector constructions; no box, a constant power-of-two box
    with the atoms wrapped, per-frame boxes of 16 and 32; a few degenerate vectors): total bit-equal to the integer sums,
    c1, c2 and coll at all lags (module docstring), both slab types the same bits."""
    case = orient_case(T, N, mode, box, weighted)
    x, idx, dims, w = case[:4]
    L = fft_length(T, 0)
    first = {}
    for dtype in SLABS:
        c = staged(0, [x], dtype)
        try:
            for fft in (0, 1):
                got = c.orient(fft, idx, mode, dimensions=dims, weights=w)
                names = timeline(c)
                assert "k_orient" in names and lag_sum_kernel(T, fft) in names and "k_widen_f32" not in names, (fft, names)
                check_orient_exact(got, case, fft, L, f"T={T} fft={fft} {dtype.__name__}", record_property)
                if fft in first:
                    assert all(np.array_equal(a, b) for a, b in zip(first[fft], got)), ("slab types differ", fft)
                first.setdefault(fft, got)
        finally:
            c.close()


# ================================================================== 6. float inputs: every lag, every wavevector, both backends
FLOAT_SCATTER = [(70, 33, 3, 3), (300, 21, 2, 2), (600, 9, 1, 2), (1100, 33, 3, 3)]  # (T, A, D, K)
FLOAT_KCUR = [(70, 33, 3, 4), (300, 21, 2, 5), (1100, 9, 1, 2), (1100, 16, 3, 3)]
FLOAT_ORIENT = [(70, 33, "bond"), (300, 7, "normal"), (1100, 12, "bisector")]  # (T, n_vectors, mode)


def pseudo_bound(series, fft, L, T, device):
    """(T, P): the by-particle bound of a returned (T, P, C) series at every lag -- direct: (C (T - k) + 6) u sum |a a'| /
    (T - k); FFT: fft_bound with the energy of the pseudo-atoms 2 m and 2 m + 1 together"""
    a = np.abs(np.asarray(series, dtype=np.float64))
    den = ex.lag_den(T).astype(np.float64)[:, None]
    if is_fft_form(device, T, fft, True):
        return ex.fft_bound(T, L, ex.fft_energy_bp((a ** 2).sum(axis=(0, 2))))
    return (a.shape[2] * den + 6) * U * (cross_abs(a, a) / 2) / den


def run_scatter_float(device, x, k, fs_ref, rho_ref, tag, record_property):
    """ta_scatter on `device` with fft 0 and 1 against a long-double self part (K, T) and density: the density within its
    bar, self within A (2 eps + (4 (T - k) + A + 6) u) (an FFT: 2 A eps + fft_bound), coll against the long-double
    autocorrelation of the returned density"""
    T, A, D = x.shape
    L = fft_length(T, device)
    den = ex.lag_den(T).astype(np.float64)
    eps = (2 * np.pi * (D + 2) * scatter_ref.unit_scale(x, k) + 8) * U
    c = staged(device, [x])
    try:
        for fft in (0, 1):
            fs, rho, coll = c.scatter(fft, k)
            assert np.max(np.abs(rho.astype(LD) - rho_ref)) <= scatter_ref.density_bar(x, k), (fft, "density")
            form = "fft" if is_fft_form(device, T, fft, False) else "direct"
            b = 2 * A * eps + ex.fft_bound(T, L, float(A * T)) if form == "fft" else A * (2 * eps + (4 * den + A + 6) * U)
            note(record_property, f"{device} {tag} self", form, assert_ratio(ratios(fs, fs_ref, b[None, :]), (fft, "self")))
            series = rho.transpose(1, 0, 2)  # (T, K, 2)
            want = ld_acf(series) / den.astype(LD)[:, None]
            form = "fft" if is_fft_form(device, T, fft, True) else "direct"
            r = ratios(coll.T, want, pseudo_bound(series, fft, L, T, device))
            note(record_property, f"{device} {tag} coll", form, assert_ratio(r, (fft, "coll")))
    finally:
        c.close()


def run_kcurrent_float(device, x, v, w, k, cur_ref, tag, record_property):
    """ta_kcurrent on `device` with fft 0 and 1: the current within the bar of ta_hip.h of cur_ref (long double or exact
    integers), long and trans against the long-double projection and autocorrelation of the RETURNED current"""
    T, _, D = x.shape
    K = len(k)
    L = fft_length(T, device)
    bar = kcurrent_ref.current_bar(x, v, w, k)
    c = staged(device, [v, x])
    try:
        for fft in (0, 1):
            cur, lon, tr = c.kcurrent(fft, k, w)
            kcurrent_ref.assert_current(cur, (None,) * 5 + (cur_ref, bar), what=f"fft={fft}")
            form = "fft" if is_fft_form(device, T, fft, True) else "direct"
            for j in range(K):
                lon_ref, tr_ref, lon_b, tr_b = projected_bounds(cur[j], k[j], form == "fft", L, T)
                if form == "fft":  # the neighbours that may share a transform with this wavevector's first and last pseudo-atom
                    extra = ex.fft_bound(T, L, sum(float((cur[i] ** 2).sum()) for i in (j - 1, j + 1) if 0 <= i < K))
                    lon_b, tr_b = lon_b + extra, tr_b + (extra * D / (D - 1) if D > 1 else 0.0)
                note(record_property, f"{device} {tag} long", form, assert_ratio(ratios(lon[j], lon_ref, lon_b), (fft, "long", j)))
                if D > 1:
                    note(record_property, f"{device} {tag} trans", form, assert_ratio(ratios(tr[j], tr_ref, tr_b), (fft, "trans", j)))
                else:
                    assert not np.any(tr[j])
    finally:
        c.close()


def rank2(u):
    """Q's six columns (T, N, 6) of long-double unit vectors, zeros where u = 0"""
    u = np.asarray(u, dtype=LD)
    live = ((u * u).sum(axis=2) > 0)[..., None]
    root2 = np.sqrt(LD(2))
    Q = np.stack([u[..., 0] ** 2 - LD(1) / 3, u[..., 1] ** 2 - LD(1) / 3, u[..., 2] ** 2 - LD(1) / 3,
                  root2 * u[..., 0] * u[..., 1], root2 * u[..., 0] * u[..., 2], root2 * u[..., 1] * u[..., 2]], axis=2)
    return np.where(live, Q, LD(0))


def lag_sum_float(series, delta, n_atoms, fft_form, L, T):
    """(reference (T,), bound (T,)) of ONE lag-sum evaluation of a (T, P, C) long-double series whose elements the library
    holds within `delta`: the input term sum (delta |a'| + delta |a|), then every product of the lag in one sum in any
    order, (P C (T - k) + n_atoms + 6) u sum |a a'| -- or fft_bound with the energy of all columns -- over T - k"""
    den = ex.lag_den(T).astype(LD)
    a = np.abs(series).astype(np.float64)
    ref = ld_acf(series).sum(axis=1) / den
    inp = cross_abs(a, np.full_like(a, delta)).sum(axis=1)
    absum = (cross_abs(a, a) / 2).sum(axis=1)
    if fft_form:
        return ref, inp / den + ex.fft_bound(T, L, float((a ** 2).sum()))
    return ref, (inp + (a.shape[1] * a.shape[2] * den + n_atoms + 6) * U * absum) / den


def run_orient_float(device, x, idx, mode, dims, w, u, ratio, tag, record_property):
    """ta_orient on `device` with fft 0 and 1 against long-double unit vectors u (T, N, 3): c1 and c2 within the bound that
    follows from B_u = 12 + 3 `ratio` and the lag sum in any order, the total within its bar, coll against the long-double
    autocorrelation of the returned total"""
    T, N = u.shape[:2]
    L = fft_length(T, device)
    B_u = 12.0 + 3.0 * ratio
    Q = rank2(u)
    total_ref = (np.asarray(u, dtype=LD) * (np.ones(N, dtype=LD) if w is None else np.asarray(w, dtype=LD))[None, :, None]).sum(axis=1)
    c = staged(device, [x])
    try:
        for fft in (0, 1):
            c1, c2, tot, coll = c.orient(fft, idx, mode, dimensions=dims, weights=w)
            assert np.max(np.abs(tot.astype(LD) - total_ref)) <= orient_ref.total_bar(N, w, ratio), (fft, "total")
            form = "fft" if is_fft_form(device, T, fft, False) else "direct"
            ref1, b1 = lag_sum_float(np.asarray(u, dtype=LD), B_u * U, N, form == "fft", L, T)
            note(record_property, f"{device} {tag} c1", form, assert_ratio(ratios(c1, ref1, b1), (fft, "c1")))
            ref2, b2 = lag_sum_float(Q, (2 * B_u + 4) * U, 2 * N, form == "fft", L, T)
            note(record_property, f"{device} {tag} c2", form, assert_ratio(ratios(c2, ref2, b2), (fft, "c2")))
            refc, bc = lag_sum_float(np.asarray(tot, dtype=LD)[:, None, :], 0.0, 1, form == "fft", L, T)
            note(record_property, f"{device} {tag} orient coll", form, assert_ratio(ratios(coll, refc, bc), (fft, "coll")))
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def scatter_float_case(T, A, D, K):
    """(x, k, long-double self at all lags (K, T), long-double density)"""
    x, k = scatter_ref.walk(T, A, D, 1), scatter_ref.wavevectors(K, D, 1)
    fs, rho, _ = scatter_ref.reference(x, k, np.arange(T))
    return x, k, fs, rho


@needs_longdouble
@pytest.mark.parametrize("device", BACKENDS)
@pytest.mark.parametrize("T,A,D,K", [pytest.param(*c, id="T{}-A{}-D{}-K{}".format(*c)) for c in FLOAT_SCATTER])
def test_scatter_float_every_lag(T, A, D, K, device, record_property):
    """scatter_ref's walks and wavevectors, every lag of every wavevector (run_scatter_float; module docstring)"""
    run_scatter_float(device, *scatter_float_case(T, A, D, K), "float", record_property)


@needs_longdouble
@pytest.mark.parametrize("device", BACKENDS)
@pytest.mark.parametrize("T,A,D,K", [pytest.param(*c, id="T{}-A{}-D{}-K{}".format(*c)) for c in FLOAT_KCUR])
def test_kcurrent_float_every_lag(T, A, D, K, device, record_property):
    """kcurrent_ref's walks, velocities and dyadic weights, every lag of every wavevector (run_kcurrent_float)"""
    x, v, w, k, _, cur_ref, _ = kcurrent_ref.case(T, A, D, K)
    run_kcurrent_float(device, x, v, w, k, cur_ref, "float", record_property)


@needs_longdouble
@pytest.mark.parametrize("device", BACKENDS)
@pytest.mark.parametrize("T,N,mode", [pytest.param(*c, id="T{}-N{}-{}".format(*c)) for c in FLOAT_ORIENT])
def test_orient_float_every_lag(T, N, mode, device, record_property):
    """orient_ref's tumbling molecules without a box (B_u = 12), every lag (run_orient_float)"""
    x, idx, w, _ = orient_ref.case(T, N, mode, weighted=True)
    run_orient_float(device, x, idx, mode, None, w, orient_ref.unit_vectors(x, idx, mode), 0.0, "float", record_property)


# ------------------------------------------------- the exact inputs of 2, 3 and 5 on the CPU backend, at the float bounds
# The CPU backend forms the phase as cos / sin(2 pi r) with a rounded 2 pi: it is not exact at quarter turns (1e-16 off),
# so the integer references are held to the bounds above, not to bit equality.
@needs_longdouble
@pytest.mark.parametrize("T,A,D,K", [pytest.param(*c, id="T{}-A{}-D{}-K{}".format(*c)) for c in SCATTER_CASES[::2]])
def test_scatter_quarter_turns_on_the_cpu_backend(T, A, D, K, record_property):
    x, q, k, rho, self_num, _ = scatter_case(T, A, D, K)
    fs_ref = self_num.sum(axis=2).astype(LD) / ex.lag_den(T)[None, :]
    run_scatter_float("cpu", x, k, fs_ref, rho.astype(LD), "quarter", record_property)


@needs_longdouble
@pytest.mark.parametrize("T,A,D,K,weighted",
                         [pytest.param(*c, id="T{}-A{}-D{}-K{}-{}".format(*c[:4], "w" if c[4] else "now")) for c in KCUR_CASES[::2]])
def test_kcurrent_quarter_turns_on_the_cpu_backend(T, A, D, K, weighted, record_property):
    x, v, w, q, k, cur = kcur_case(T, A, D, K, weighted)
    run_kcurrent_float("cpu", x, v, w, k, cur.astype(LD), "quarter", record_property)


@needs_longdouble
@pytest.mark.parametrize("T,N,mode,box,weighted",
                         [pytest.param(*c, id="T{}-N{}-{}-{}".format(c[0], c[1], c[2], c[3] or "nobox")) for c in ORIENT_CASES[1::2]])
def test_orient_axes_on_the_cpu_backend(T, N, mode, box, weighted, record_property):
    """(the backend shares orient_math.hpp with the kernel, so these are exact there too; held to the float bounds with R
    of ta_hip.h from the wrapped differences: the largest raw component over the smallest |v| = 1)"""
    x, idx, dims, w, _, u = orient_case(T, N, mode, box, weighted)
    raw = max(float(np.abs(x[:, idx[:, j]] - x[:, idx[:, 0]]).max()) for j in range(1, idx.shape[1]))
    run_orient_float("cpu", x, idx, mode, dims, w, u, raw if dims is not None else 0.0, "axes", record_property)
