"""OnsagerGreenKubo, ConductivityGreenKubo and the ta_current* entry points: the closed form of two ballistic species,
parity with a long-double restatement on every dispatch path, the identities with VelocityAutocorr and between the two
classes, invariance under permutation and relabelling, exactness on a grid, errors, the raw C-ABI, several devices and
torch.distributed.  Every class-level test runs on the library's CPU backend and, marked gpu, on the HIP path."""
import ctypes
import os

import numpy as np
import pytest

from conftest import scale_rel_err
from current_ref import assert_cross, assert_currents, cross_ref, currents_ref, pair_scale, species_velocities, velocity_case
from transport_analysis_amd import ConductivityGreenKubo, OnsagerGreenKubo, VelocityAutocorr, _lib
from transport_analysis_amd._base import NoDataError, UpdatingAtomGroup
from transport_analysis_amd._mini_mda import ArrayUniverse

DIMS = [("xyz", [0, 1, 2]), ("xy", [0, 1]), ("xz", [0, 2]), ("yz", [1, 2]), ("x", [0]), ("y", [1]), ("z", [2])]
BOX = [40.0, 50.0, 60.0, 90, 90, 90]
VOL = 40.0 * 50.0 * 60.0
K_B, E = 1.380649e-23, 1.602176634e-19
TA_E_INVALID, TA_E_STATE, TA_E_UNSUPPORTED = -1, -4, -5
MAX_SPECIES = 8


@pytest.fixture(params=["cpu", pytest.param("hip", marks=pytest.mark.gpu)])
def backend(request, monkeypatch):
    if request.param == "cpu":
        monkeypatch.setenv("TA_AMD_DEVICE", "cpu")  # the library's opt-in CPU backend behind the same C symbols
    else:
        monkeypatch.delenv("TA_AMD_DEVICE", raising=False)
        assert _lib.device_count() >= 1
    return request.param


def float64_universe(v, charges=None, dt=1.0, box=BOX):
    """Timesteps that hand out float64 velocities (the closed forms are not exact in float32)."""
    u = ArrayUniverse(velocities=v, charges=charges, dimensions=box, dt=dt)
    u.trajectory._vel = np.ascontiguousarray(v, dtype=np.float64)
    return u


def context(backend):
    return _lib.Context("cpu" if backend == "cpu" else 0)


def staged(backend, v, dtype=np.float64):
    c = context(backend)
    (view,) = c.stage_alloc(*v.shape, dtype=dtype)
    view[:] = v
    c.stage_commit(0, v.shape[0])
    return c


# ------------------------------------------------------------------------------ 1. closed form
@pytest.fixture(scope="module")
def two_species():
    """N+ atoms at +v and N- at -v along every axis, interleaved: J+- = +-N+- v at every frame, C++ = D (N+ v)^2,
    C+- = -D N+ N- v^2 at every lag, lag 0 included."""
    T, n_plus, n_minus, v, dt = 400, 3, 2, 0.5, 2.0
    lab = np.array([0, 1, 0, 1, 0])
    vel = np.empty((T, 5, 3))
    for n, s in enumerate(lab):
        vel[:, n, :] = v if s == 0 else -v
    return float64_universe(vel, dt=dt), lab, n_plus, n_minus, v, dt


@pytest.mark.parametrize("fft", [True, False])
@pytest.mark.parametrize("dim_type,cols", DIMS)
def test_closed_form_two_species(backend, two_species, dim_type, cols, fft):
    u, lab, n_p, n_m, v, dt = two_species
    D = len(cols)
    T_avg = 350.0
    factor = 1e22 / (D * K_B * VOL * T_avg)

    def check(o, step):
        n = o.n_frames
        want_j = np.stack([np.full((n, D), n_p * v), np.full((n, D), -n_m * v)])
        assert o.results.currents.shape == (2, n, D)
        assert scale_rel_err(o.results.currents, want_j) <= 1e-12
        c = o.results.timeseries
        assert c.shape == (n, 2, 2)
        scale = D * (max(n_p, n_m) * v) ** 2
        want = np.array([[D * (n_p * v) ** 2, -D * n_p * n_m * v * v], [-D * n_p * n_m * v * v, D * (n_m * v) ** 2]])
        assert np.max(np.abs(c - want[None])) <= 1e-10 * scale  # every lag, lag 0 included
        assert np.array_equal(c[:, 0, 1], c[:, 1, 0])
        np.testing.assert_allclose(o.lag_times(), np.arange(n) * step * dt)
        # a constant integrand: the lags 0 ... k span k dt, and both rules are exact
        for k in (1, 10, n - 1):
            got = o.onsager_gk(stop=k + 1)
            assert got.shape == (2, 2)
            assert np.max(np.abs(got - want * k * step * dt * factor)) <= 1e-10 * scale * k * step * dt * factor
        for k in (2, 10):  # (an even number of intervals)
            assert np.max(np.abs(o.onsager_gk_odd(stop=k + 1) - want * k * step * dt * factor)) <= 1e-10 * scale * k * step * dt * factor
        # start / stop / step of the window: lags 4, 7, ..., 31 span 27 lag spacings
        assert np.max(np.abs(o.onsager_gk(4, 32, 3) - want * 27 * step * dt * factor)) <= 1e-10 * scale * 27 * step * dt * factor
        ri = o.running_integral()
        assert ri.shape == (n, 2, 2) and not ri[0].any()
        assert np.max(np.abs(ri[-1] - o.onsager_gk())) <= 1e-12 * np.abs(ri[-1]).max()

    kw = dict(temp_avg=T_avg, dim_type=dim_type, fft=fft, stage_dtype=np.float64)
    check(OnsagerGreenKubo(u.atoms, lab, **kw).run(), 1)
    o = OnsagerGreenKubo(u.atoms, lab, **kw).run(start=10, stop=390, step=4)
    assert o.n_frames == 95
    check(o, 4)
    assert list(o.results.species) == [0, 1]


# ----------------------------------------------------------------------- 2. random velocities
CASES = [(1, 5, 2), (2, 5, 2), (64, 40, 2), (65, 9, 3), (300, 501, 3), (513, 40, 4), (1100, 1501, 4), (2049, 1100, 8)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T,A,S", CASES)
def test_random_velocity_parity(backend, T, A, S, dtype):
    f32 = dtype == np.float32
    v, lab, w, want_j, scale, want_c = velocity_case(T, A, S, f32=f32)
    sizes = np.bincount(lab, minlength=S)
    assert sizes.min() >= 1 and (A < 10 or sizes[0] > 0.5 * A)  # unequal species, nobody missing
    u = ArrayUniverse(velocities=v, dimensions=BOX) if f32 else float64_universe(v)
    for fft in (True, False):
        o = OnsagerGreenKubo(u.atoms, lab, fft=fft, weights=w, stage_dtype=dtype).run()
        assert_currents(o.results.currents, want_j, scale)
        assert_cross(o.results.timeseries, want_c)


# ----------------------------------------------------------------------------------- 3. identities
@pytest.mark.parametrize("fft", [True, False])
def test_identities(backend, fft):
    T, A, S = 300, 41, 3
    v, lab, w = species_velocities(T, A, S, seed=5)
    u = ArrayUniverse(velocities=v, charges=w, dimensions=BOX)
    # one atom, unit weight, one species: its velocity autocorrelation
    atom = u.atoms[7:8]
    o1 = OnsagerGreenKubo(atom, ["a"], fft=fft).run()
    va = VelocityAutocorr(atom, fft=fft).run()
    assert scale_rel_err(o1.results.timeseries[:, 0, 0], va.results.timeseries) <= 1e-10
    assert list(o1.results.species) == ["a"]
    # sum_ij C_ij is the correlation of the summed current: each C_ij is within 1e-10 of its pair scale, the one-species
    # C within 1e-10 of its own C(0), so the two agree within the sum of those bounds
    o = OnsagerGreenKubo(u.atoms, lab, fft=fft, weights=w).run()
    one = OnsagerGreenKubo(u.atoms, np.zeros(A, dtype=int), fft=fft, weights=w).run()
    c, c1 = o.results.timeseries, one.results.timeseries
    bound = 1e-10 * (float(pair_scale(c).sum()) + float(c1[0, 0, 0]))
    assert np.max(np.abs(c.sum(axis=(1, 2)) - c1[:, 0, 0])) <= bound
    assert scale_rel_err(o.results.currents.sum(axis=0), one.results.currents[0]) <= 1e-12
    # ConductivityGreenKubo is that one-species run, bit for bit
    cond = ConductivityGreenKubo(u.atoms, fft=fft).run()  # atomgroup.charges
    assert cond.results.current.shape == (T, 3) and cond.results.timeseries.shape == (T,)
    assert np.array_equal(cond.results.current, one.results.currents[0])
    assert np.array_equal(cond.results.timeseries, c1[:, 0, 0])
    cond2 = ConductivityGreenKubo(u.atoms, charges=w, fft=fft).run()
    assert np.array_equal(cond2.results.timeseries, cond.results.timeseries)
    assert cond.conductivity_gk(0, 100) == E ** 2 * one.onsager_gk(0, 100)[0, 0]
    assert cond.conductivity_gk_odd(0, 101) == E ** 2 * one.onsager_gk_odd(0, 101)[0, 0]


@pytest.mark.parametrize("fft", [True, False])
def test_conductivity_and_transference(backend, fft):
    """Unit weights and one charge number per species against ConductivityGreenKubo with charges z[species]."""
    T, A, S = 300, 41, 3
    v, lab, _ = species_velocities(T, A, S, seed=6)
    z = np.array([1.0, -1.0, 2.0])
    u = ArrayUniverse(velocities=v, charges=z[lab], dimensions=BOX)
    o = OnsagerGreenKubo(u.atoms, lab, fft=fft, temp_avg=320.0).run()
    cond = ConductivityGreenKubo(u.atoms, fft=fft, temp_avg=320.0).run()
    c = o.results.timeseries
    factor = 1e22 / (3 * K_B * VOL * 320.0)

    def bound(window, rule_weight=1.0):
        """sigma is linear in C: the 1e-10 bounds of sum_ij z_i z_j C_ij and of the one-species C, carried through the
        rule's weights (trapezoid: they add up to the window's span; Simpson: at most 4/3 of a trapezoid weight)"""
        t = o.lag_times()[slice(window[0], window[1] or T, window[2])]
        per_lag = float((np.abs(np.outer(z, z)) * pair_scale(c)).sum()) + float(cond.results.timeseries[0])
        return 1e-10 * E ** 2 * factor * float(t[-1] - t[0]) * per_lag * rule_weight

    for window in ((0, 0, 1), (0, 120, 1), (5, 200, 3)):
        assert abs(o.conductivity(z, *window) - cond.conductivity_gk(*window)) <= bound(window)
        tn = o.transference_numbers(z, *window)
        assert tn.shape == (S,) and abs(tn.sum() - 1.0) <= 1e-12
    assert abs(o.conductivity(z, 0, 101, odd=True) - cond.conductivity_gk_odd(0, 101)) <= bound((0, 101, 1), 4.0 / 3.0)
    L = o.onsager_gk()
    assert L.shape == (S, S) and np.array_equal(L, L.T)
    with pytest.raises(ValueError, match="charges for 3 species"):
        o.conductivity(z[:2])
    with pytest.raises(RuntimeError, match="must be run"):
        OnsagerGreenKubo(u.atoms, lab).onsager_gk()


def test_units(backend, two_species):
    u, lab, n_p, n_m, v, dt = two_species
    T_avg, k = 350.0, 100
    o = OnsagerGreenKubo(u.atoms, lab, temp_avg=T_avg, dim_type="xy", stage_dtype=np.float64).run()
    L = o.onsager_gk(stop=k + 1)
    for (i, j), amp in (((0, 0), n_p * n_p), ((1, 1), n_m * n_m), ((0, 1), -n_p * n_m)):
        integral = 2 * amp * v * v * k * dt  # A^2 / ps: D = 2
        want = (integral * 1e-20 / 1e-12) / (2 * VOL * 1e-30 * K_B * T_avg)  # 1 / (J m s)
        assert abs(L[i, j] - want) <= 1e-9 * abs(want)
    z = np.array([1.0, -1.0])
    sigma = o.conductivity(z, stop=k + 1)
    assert abs(sigma - E ** 2 * (z[:, None] * z[None, :] * L).sum()) <= 1e-12 * sigma


# ------------------------------------------------------------------------------------ 4. invariance
@pytest.mark.parametrize("fft", [True, False])
def test_permutation_and_relabelling(backend, fft):
    T, A, S = 200, 37, 4
    v, lab, w = species_velocities(T, A, S, seed=9)
    base = OnsagerGreenKubo(float64_universe(v).atoms, lab, fft=fft, weights=w, stage_dtype=np.float64).run()
    scale = currents_ref(v, lab, w, S)[1].max(axis=1)
    cs = pair_scale(base.results.timeseries)
    rng = np.random.default_rng(1)
    perm = rng.permutation(A)
    p = OnsagerGreenKubo(float64_universe(v[:, perm]).atoms, lab[perm], fft=fft, weights=w[perm], stage_dtype=np.float64).run()
    assert (np.abs(p.results.currents - base.results.currents).max(axis=(1, 2)) <= 1e-12 * scale).all()
    assert (np.abs(p.results.timeseries - base.results.timeseries).max(axis=0) <= 1e-10 * cs).all()
    # new names whose sort order permutes the species: index i of the new result is species order[i] of the old
    names = np.array(["d", "b", "a", "c"])
    order = np.argsort(names)
    r = OnsagerGreenKubo(float64_universe(v).atoms, names[lab], fft=fft, weights=w, stage_dtype=np.float64).run()
    assert list(r.results.species) == ["a", "b", "c", "d"]
    assert (np.abs(r.results.currents - base.results.currents[order]).max(axis=(1, 2)) <= 1e-12 * scale[order]).all()
    want_c = base.results.timeseries[:, order][:, :, order]
    assert (np.abs(r.results.timeseries - want_c).max(axis=0) <= 1e-10 * cs[order][:, order]).all()


@pytest.mark.parametrize("fft", [True, False])
def test_empty_species_is_exactly_zero(backend, fft):
    """Labels 0 and 2 with n_species = 4 through the binding: species 1 and 3 have no atoms."""
    T, A = 150, 23
    v, lab, w = species_velocities(T, A, 2, seed=3)
    lab = (2 * lab).astype(np.int32)
    c = staged(backend, v)
    try:
        j, cr = c.current(fft, lab, n_species=4, weights=w)
    finally:
        c.close()
    want_j, scale = currents_ref(v, lab, w, 4)
    assert_currents(j, want_j, scale)
    assert_cross(cr, cross_ref(want_j))
    for s in (1, 3):
        assert not j[s].any() and not cr[:, s, :].any() and not cr[:, :, s].any()
    assert cr[:, 0, 2].any() and cr[0, 0, 0] > 0


# ------------------------------------------------------------------------------------- 5. exactness
def grid_velocities(T, A, S, seed):
    """Velocities on a 1/64 grid (exact in float32 too) and integer weights: every partial sum is exact in float64."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-4000, 4001, size=(T, A, 3))
    lab = rng.permutation(np.where(rng.random(A) < 0.7, 0, rng.integers(1, S, size=A))).astype(np.int32)
    w = rng.integers(-2, 4, size=A).astype(np.float64)
    return k, k / 64.0, lab, w


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_currents_and_bit_identical_repeats(backend, dtype):
    T, A, S = 1101, 1501, 3
    k, v, lab, w = grid_velocities(T, A, S, seed=11)
    want = np.stack([(k[:, lab == s, :] * w[lab == s].astype(np.int64)[None, :, None]).sum(axis=1) for s in range(S)]) / 64.0
    c = context(backend)
    if backend == "hip" and dtype == np.float32:
        c.set_option("stage_device_f32", 1)
    (view,) = c.stage_alloc(T, A, 3, dtype=dtype)
    view[:] = v
    c.stage_commit(0, T)
    try:
        for fft in (True, False):
            j1, c1 = c.current(fft, lab, weights=w)
            j2, c2 = c.current(fft, lab, weights=w)
            assert np.array_equal(j1, want), "exact partial sums: the currents do not depend on the summation order"
            assert np.array_equal(j1, j2) and np.array_equal(c1, c2)
            assert_cross(c1, cross_ref(want))
    finally:
        c.close()


# ------------------------------------------------------------------------------------ 6. errors
def test_api_errors(backend):
    v = species_velocities(10, 3, 2, seed=1)[0]
    u = ArrayUniverse(velocities=v, dimensions=BOX)
    lab = [0, 1, 0]
    with pytest.raises(NoDataError, match="velocities and box volume"):  # positions only
        OnsagerGreenKubo(ArrayUniverse(positions=v, dimensions=BOX).atoms, lab).run()
    with pytest.raises(NoDataError, match="velocities and box volume"):
        ConductivityGreenKubo(ArrayUniverse(positions=v, charges=[1, -1, 1], dimensions=BOX).atoms).run()
    with pytest.raises(NoDataError):  # zero volume
        OnsagerGreenKubo(ArrayUniverse(velocities=v).atoms, lab).run()
    with pytest.raises(ValueError, match="species: 2 labels for 3 atoms"):
        OnsagerGreenKubo(u.atoms, [0, 1])
    with pytest.raises(ValueError, match="weights: 2 values for 3 atoms"):
        OnsagerGreenKubo(u.atoms, lab, weights=[1.0, 2.0])
    with pytest.raises(ValueError, match="weights: 2 values for 3 atoms"):
        ConductivityGreenKubo(u.atoms, charges=[1.0, 2.0])
    big = ArrayUniverse(velocities=species_velocities(4, 9, 2, seed=1)[0], dimensions=BOX)
    with pytest.raises(ValueError, match="9 distinct labels, at most 8"):
        OnsagerGreenKubo(big.atoms, np.arange(9))
    assert OnsagerGreenKubo(big.atoms, np.arange(9) % 8).run().results.timeseries.shape == (4, 8, 8)
    for cls, args in ((OnsagerGreenKubo, (lab,)), (ConductivityGreenKubo, ([1.0, -1.0, 1.0],))):
        with pytest.raises(TypeError, match="UpdatingAtomGroup"):
            cls(UpdatingAtomGroup(), *args)
        with pytest.raises(TypeError, match="by_particle"):
            cls(u.atoms, *args, by_particle=True)
        with pytest.raises(TypeError, match="unwrap is not accepted"):
            cls(u.atoms, *args, unwrap=True)
        with pytest.raises(ValueError, match="invalid dim_type: foo specified"):
            cls(u.atoms, *args, dim_type="foo")
        with pytest.raises(ValueError, match="exclusive"):
            cls(u.atoms, *args, devices=[0], distributed=True)
    assert OnsagerGreenKubo(u.atoms, lab, by_particle=False).run().results.timeseries.shape == (10, 2, 2)
    # species by the name of a per-atom attribute of the group
    u.atoms.types = np.array(["Li", "TFSI", "Li"])
    o = OnsagerGreenKubo(u.atoms, "types").run()
    assert list(o.results.species) == ["Li", "TFSI"] and list(o.species_index) == [0, 1, 0]


def test_float32_staging_stays_float32_on_the_device(monkeypatch):
    """_set_options keeps a float32 staging slab float32 on the device at every n_frames (and a float64 one float64)."""
    seen = []

    class Probe:
        def set_option(self, key, value):
            seen.append((key, value))

    o = OnsagerGreenKubo(ArrayUniverse(velocities=np.zeros((4, 2, 3)), dimensions=BOX).atoms, [0, 1])
    o._ctx = Probe()
    for n_frames in (4, 600, 20000):
        o.n_frames = n_frames
        o._set_options(np.dtype(np.float32))
        o._set_options(np.dtype(np.float64))
    assert seen == [("stage_device_f32", 1), ("stage_device_f32", 0)] * 3


def test_no_run_hooks_of_mdanalysis():
    """MDAnalysis >= 2.8's run() calls these private hooks; a class (or its StagedAnalysis base) defining one breaks it."""
    from transport_analysis_amd import _base

    hooks = {"_compute", "_configure_backend", "_setup_computation_groups", "_get_aggregator", "_define_run_frames",
             "_prepare_sliced_trajectory"}
    for cls in (OnsagerGreenKubo, ConductivityGreenKubo):
        mro = cls.__mro__
        own = [k for c in mro[:mro.index(_base.AnalysisBase)] for k in vars(c)]
        assert not set(own) & hooks


def last_error(c):
    return _lib.lib().ta_last_error(c._h).decode()


def test_cabi_argument_checks(backend):
    """ta_current / ta_current_cross: every TA_E_INVALID and TA_E_STATE case with its message; the cross-correlation of
    hand-made currents with no slab staged; on the CPU backend the device entry points are unsupported."""
    L = _lib.lib()
    P = _lib._ptr
    c = context(backend)
    T, A, D, S = 8, 5, 2, 3
    v = species_velocities(T, A, S, seed=2, D=D)[0]
    lab = np.array([0, 2, 1, 0, 2], dtype=np.int32)
    w = np.array([1.0, 2.0, 0.5, 1.0, 2.0])
    cur, cr = np.zeros((S, T, D)), np.zeros((T, S, S))
    # the cross-correlation of given currents needs no staged slab
    hand = np.random.default_rng(4).standard_normal((S, 70, D))
    for fft in (0, 1):
        assert_cross(c.current_cross(hand, fft), cross_ref(hand))
    assert_cross(c.current_cross(hand[:, :1], 1), cross_ref(hand[:, :1]))  # one frame: lag 0 alone, <J_i . J_j>
    with pytest.raises(ValueError, match="expected \\(n_species, n_frames, dim\\)"):
        c.current_cross(hand[0], 1)
    assert L.ta_current(c._h, 1, S, P(lab), P(w), P(cur), P(cr)) == TA_E_STATE
    assert "not been staged" in last_error(c)
    (view,) = c.stage_alloc(T, A, D)
    view[:] = v
    c.stage_commit(0, T)
    assert L.ta_current(c._h, 2, S, P(lab), P(w), P(cur), P(cr)) == TA_E_INVALID
    assert "fft must be 0 or 1" in last_error(c)
    for bad in (0, -1, MAX_SPECIES + 1):
        assert L.ta_current(c._h, 1, bad, P(lab), P(w), P(cur), P(cr)) == TA_E_INVALID
        assert "n_species must be 1 ... 8" in last_error(c)
    assert L.ta_current(c._h, 1, S, None, P(w), P(cur), P(cr)) == TA_E_INVALID
    assert "species labels are NULL" in last_error(c)
    assert L.ta_current(c._h, 1, S, P(lab), P(w), None, P(cr)) == TA_E_INVALID
    assert "currents output is NULL" in last_error(c)
    assert L.ta_current(None, 1, S, P(lab), P(w), P(cur), P(cr)) == TA_E_INVALID
    for bad in (3, -1):  # a label outside 0 ... n_species - 1, checked on the host
        lab_bad = lab.copy()
        lab_bad[3] = bad
        assert L.ta_current(c._h, 1, S, P(lab_bad), P(w), P(cur), P(cr)) == TA_E_INVALID
        assert f"species label {bad} of atom 3 is outside 0 ... n_species - 1" in last_error(c)
    assert L.ta_current_cross(c._h, 2, P(cur), S, T, D, P(cr)) == TA_E_INVALID
    assert "fft must be 0 or 1" in last_error(c)
    assert L.ta_current_cross(c._h, 1, P(cur), 9, T, D, P(cr)) == TA_E_INVALID
    assert "n_species must be 1 ... 8" in last_error(c)
    assert L.ta_current_cross(c._h, 1, None, S, T, D, P(cr)) == TA_E_INVALID
    assert "currents or cross output is NULL" in last_error(c)
    assert L.ta_current_cross(c._h, 1, P(cur), S, T, D, None) == TA_E_INVALID
    assert "currents or cross output is NULL" in last_error(c)
    assert L.ta_current_cross(c._h, 1, P(cur), S, 0, D, P(cr)) == TA_E_INVALID
    assert "need 1 <= n_frames <= 2^30, 1 <= dim <= 3" in last_error(c)
    assert L.ta_current_cross(c._h, 1, P(cur), S, T, 4, P(cr)) == TA_E_INVALID
    assert "need 1 <= n_frames <= 2^30, 1 <= dim <= 3" in last_error(c)
    assert L.ta_current_cross(None, 1, P(cur), S, T, D, P(cr)) == TA_E_INVALID
    assert L.ta_group_current(None, 1, S, P(lab), P(w), P(cur), P(cr)) == TA_E_INVALID
    want_j, scale = currents_ref(v, lab, w, S)
    for fft in (0, 1):
        assert L.ta_current(c._h, fft, S, P(lab), P(w), P(cur), P(cr)) == 0
        assert_currents(cur, want_j, scale)
        assert_cross(cr, cross_ref(want_j))
    assert L.ta_current(c._h, 1, S, P(lab), None, P(cur), None) == 0  # unit weights, the currents alone
    assert_currents(cur, *currents_ref(v, lab, None, S))
    assert_cross(c.current_cross(cur, 1), cross_ref(cur))  # ... and the staged slab is still there
    assert L.ta_current(c._h, 1, S, P(lab), P(w), P(cur), P(cr)) == 0
    with pytest.raises(ValueError, match="species: 2 labels for 5 atoms"):
        c.current(True, lab[:2])
    with pytest.raises(ValueError, match="weights"):
        c.current(True, lab, weights=w[:2])
    if backend == "cpu":
        p = ctypes.c_void_p(16)
        assert L.ta_current_staged(c._h, 1, S, p, p, p, None, None) == TA_E_UNSUPPORTED
        assert L.ta_current_dev(c._h, p, T, A, D, A * D, 1, S, p, p, p, None, None) == TA_E_UNSUPPORTED
        assert "CPU backend" in last_error(c)
    c.close()


@pytest.mark.gpu
def test_current_dev_and_staged_argument_checks():
    import torch

    T, A, D, S = 40, 7, 3, 2
    v, lab, w = species_velocities(T, A, S, seed=8)
    dev = torch.device("cuda", 0)
    d_v, d_lab, d_w = torch.from_numpy(v.reshape(T, A * D)).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(w).to(dev)
    cur = torch.zeros((S, T, D), dtype=torch.float64, device=dev)
    L = _lib.lib()
    c = _lib.Context(0)
    V = ctypes.c_void_p
    p, pl, pw, pc = V(d_v.data_ptr()), V(d_lab.data_ptr()), V(d_w.data_ptr()), V(cur.data_ptr())
    assert L.ta_current_staged(c._h, 1, S, pl, pw, pc, None, None) == TA_E_STATE  # nothing staged
    assert "not been staged" in last_error(c)
    assert L.ta_current_dev(c._h, p, T, A, 4, A * D, 1, S, pl, pw, pc, None, None) == TA_E_INVALID  # dim
    assert L.ta_current_dev(c._h, p, T, A, D, A * D - 1, 1, S, pl, pw, pc, None, None) == TA_E_INVALID  # ld_row
    assert L.ta_current_dev(c._h, p, 0, A, D, A * D, 1, S, pl, pw, pc, None, None) == TA_E_INVALID  # n_frames
    assert L.ta_current_dev(c._h, None, T, A, D, A * D, 1, S, pl, pw, pc, None, None) == TA_E_INVALID
    assert "null device pointer" in last_error(c)
    assert L.ta_current_dev(c._h, p, T, A, D, A * D, 1, S, None, pw, pc, None, None) == TA_E_INVALID  # labels
    assert "species labels are NULL" in last_error(c)
    assert L.ta_current_dev(c._h, p, T, A, D, A * D, 1, S, pl, pw, None, None, None) == TA_E_INVALID  # currents
    assert "currents output is NULL" in last_error(c)
    assert L.ta_current_dev(c._h, p, T, A, D, A * D, 2, S, pl, pw, pc, None, None) == TA_E_INVALID  # fft
    assert L.ta_current_dev(c._h, p, T, A, D, A * D, 1, 9, pl, pw, pc, None, None) == TA_E_INVALID  # n_species
    c.current_dev(d_v.data_ptr(), T, A, D, A * D, True, S, d_lab.data_ptr(), cur.data_ptr(), d_w.data_ptr())
    torch.cuda.synchronize()
    assert_currents(cur.cpu().numpy(), *currents_ref(v, lab, w, S))
    # device labels are not checked: an atom with a label out of range is left out of every current
    lab_bad = lab.copy()
    lab_bad[2], lab_bad[5] = 7, -3
    c.current_dev(d_v.data_ptr(), T, A, D, A * D, True, S, torch.from_numpy(lab_bad).to(dev).data_ptr(), cur.data_ptr(),
                  d_w.data_ptr())
    torch.cuda.synchronize()
    keep = np.ones(A, dtype=bool)
    keep[[2, 5]] = False
    assert_currents(cur.cpu().numpy(), *currents_ref(v[:, keep], lab[keep], w[keep], S))
    c.close()


# -------------------------------------------------------------- 7. several devices, distributed
@pytest.mark.gpu
@pytest.mark.parametrize("fft", [True, False])
def test_devices_two_members_one_gpu(fft):
    v, lab, w = species_velocities(400, 11, 3, seed=8)
    u = ArrayUniverse(velocities=v, dimensions=BOX)
    kw = dict(fft=fft, weights=w)
    one = OnsagerGreenKubo(u.atoms, lab, **kw).run()
    two = OnsagerGreenKubo(u.atoms, lab, devices=[0, 0], **kw).run()
    assert two.results.device_ranges == [(0, 5), (5, 11)]
    scale = currents_ref(v.astype(np.float32).astype(np.float64), lab, w, 3)[1].max(axis=1)
    assert (np.abs(two.results.currents - one.results.currents).max(axis=(1, 2)) <= 1e-12 * scale).all()
    assert (np.abs(two.results.timeseries - one.results.timeseries).max(axis=0) <= 1e-10 * pair_scale(one.results.timeseries)).all()
    np.testing.assert_allclose(two.onsager_gk(0, 200), one.onsager_gk(0, 200), rtol=1e-9, atol=1e-9 * np.abs(one.onsager_gk(0, 200)).max())


@pytest.mark.gpu
@pytest.mark.parametrize("fft", [True, False], ids=["fft", "direct"])
def test_group_current_odd_member_slabs(fft):
    """ta_group_current on devices=[0, 0] at 1502 atoms x 3: each member holds 751 atoms, 2253 columns, so both slabs end
    on an unpaired column and the second member starts mid-way (atom 751) through the labels and weights."""
    T, A, S = 1100, 1502, 3
    v, lab, w = species_velocities(T, A, S, seed=5)
    want_j, scale = currents_ref(v, lab, w, S)
    c = staged("hip", v)
    try:
        one = c.current(fft, lab, weights=w)
    finally:
        c.close()
    g = _lib.Group([0, 0])
    try:
        (views,) = g.stage_alloc(T, A, 3)
        assert g.shards == [(0, 751), (751, 1502)]
        for (lo, hi), view in zip(g.shards, views):
            view[:] = v[:, lo:hi]
        g.stage_commit(0, T)
        j, cr = g.current(fft, lab, weights=w)
        bad = lab.copy()
        bad[1000] = 3
        assert _lib.lib().ta_group_current(g._h, int(fft), S, _lib._ptr(bad), None, _lib._ptr(j), None) == TA_E_INVALID
        assert "species label 3 of atom 1000" in _lib.lib().ta_group_last_error(g._h).decode()
        assert _lib.lib().ta_group_current(g._h, int(fft), S, _lib._ptr(lab), None, None, None) == TA_E_INVALID
        assert "species labels or currents are NULL" in _lib.lib().ta_group_last_error(g._h).decode()
    finally:
        g.close()
    assert_currents(j, want_j, scale)
    assert (np.abs(j - one[0]).max(axis=2) <= 1e-12 * scale).all()
    assert_cross(cr, cross_ref(want_j))
    assert (np.abs(cr - one[1]).max(axis=0) <= 1e-10 * pair_scale(one[1])).all()


def _current_worker(rank, world, port, T, A, out_dir):
    import sys

    import torch.distributed as dist

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from current_ref import species_velocities
    from transport_analysis_amd import OnsagerGreenKubo
    from transport_analysis_amd._mini_mda import ArrayUniverse

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    v, lab, w = species_velocities(T, A, 2, seed=12)
    u = ArrayUniverse(velocities=v, dimensions=BOX)
    out = {}
    for fft in (True, False):
        o = OnsagerGreenKubo(u.atoms, lab, fft=fft, weights=w, distributed=True, device="cpu").run()
        out[f"j_{int(fft)}"] = o.results.currents
        out[f"c_{int(fft)}"] = o.results.timeseries
        out[f"l_{int(fft)}"] = o.onsager_gk(0, 60)
        out["range"] = np.array(o.results.particle_range)
    np.savez(os.path.join(out_dir, f"cur_{rank}.npz"), **out)
    dist.destroy_process_group()


@pytest.mark.parametrize("A", [7, 1])
def test_distributed_gloo_world2_cpu_backend(tmp_path, A):
    """A = 7, xyz: rank 0 holds atoms 0-2 = 9 columns, so the column pair (8, 9) of the whole slab is cut between the
    ranks; A = 1: one rank holds no atom and contributes zeros."""
    import torch.multiprocessing as mp

    T, world = 90, 2
    port = 39600 + (os.getpid() % 2000) + A
    mp.spawn(_current_worker, args=(world, port, T, A, str(tmp_path)), nprocs=world, join=True)
    v, lab, w = species_velocities(T, A, 2, seed=12)
    u = ArrayUniverse(velocities=v, dimensions=BOX)
    for fft in (True, False):
        serial = OnsagerGreenKubo(u.atoms, lab, fft=fft, weights=w, device="cpu").run()
        scale = currents_ref(v.astype(np.float32).astype(np.float64), lab, w, serial.n_species)[1].max(axis=1)
        for r in range(world):
            z = np.load(tmp_path / f"cur_{r}.npz")
            assert tuple(z["range"]) == ((A * r) // world, (A * (r + 1)) // world)
            assert (np.abs(z[f"j_{int(fft)}"] - serial.results.currents).max(axis=(1, 2)) <= 1e-12 * scale).all()
            assert (np.abs(z[f"c_{int(fft)}"] - serial.results.timeseries).max(axis=0)
                    <= 1e-10 * pair_scale(serial.results.timeseries)).all()
            want = serial.onsager_gk(0, 60)
            np.testing.assert_allclose(z[f"l_{int(fft)}"], want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
