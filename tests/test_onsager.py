"""OnsagerHelfand and the ta_onsager* entry points: the closed form of two ballistic species, parity with a long-double
restatement on every dispatch path, the identities with ConductivityHelfand and EinsteinMSD, invariance under permutation
and relabelling, exactness on a grid, unwrapping, errors, the raw C-ABI, several devices and torch.distributed.  Every
class-level test runs on the library's CPU backend and, marked gpu, on the HIP path."""
import ctypes
import os

import numpy as np
import pytest

from conftest import scale_rel_err
from onsager_ref import assert_cross, assert_moments, cross_ref, moments_ref, pair_scale, species_walk, walk_case
from transport_analysis_amd import ConductivityHelfand, EinsteinMSD, OnsagerHelfand, _lib
from transport_analysis_amd._base import NoDataError, UpdatingAtomGroup
from transport_analysis_amd._mini_mda import ArrayUniverse

DIMS = [("xyz", [0, 1, 2]), ("xy", [0, 1]), ("xz", [0, 2]), ("yz", [1, 2]), ("x", [0]), ("y", [1]), ("z", [2])]
BOX = [40.0, 50.0, 60.0, 90, 90, 90]
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


def float64_universe(x, charges=None, dt=1.0, box=BOX):
    """Timesteps that hand out float64 positions (the closed forms are not exact in float32)."""
    u = ArrayUniverse(positions=x, charges=charges, dimensions=box, dt=dt)
    u.trajectory._pos = np.ascontiguousarray(x, dtype=np.float64)
    return u


def context(backend):
    return _lib.Context("cpu" if backend == "cpu" else 0)


def staged(backend, x, dtype=np.float64):
    c = context(backend)
    (view,) = c.stage_alloc(*x.shape, dtype=dtype)
    view[:] = x
    c.stage_commit(0, x.shape[0])
    return c


# ------------------------------------------------------------------------------ 1. closed form
@pytest.fixture(scope="module")
def two_species():
    """N+ atoms at +v and N- at -v along every axis, interleaved: M+- = +-N+- v t, C++ = D (N+ v k dt)^2,
    C+- = -D N+ N- (v k dt)^2."""
    T, n_plus, n_minus, v, dt = 400, 3, 2, 0.5, 2.0
    t = np.arange(T) * dt
    lab = np.array([0, 1, 0, 1, 0])
    x = np.empty((T, 5, 3))
    for n, s in enumerate(lab):
        x[:, n, :] = 100.0 * (n + 1) + (v if s == 0 else -v) * t[:, None]
    return float64_universe(x, dt=dt), lab, n_plus, n_minus, v, dt


@pytest.mark.parametrize("fft", [True, False])
@pytest.mark.parametrize("dim_type,cols", DIMS)
def test_closed_form_two_species(backend, two_species, dim_type, cols, fft):
    u, lab, n_p, n_m, v, dt = two_species
    D = len(cols)

    def check(o, step):
        k = np.arange(o.n_frames) * step * dt
        want_m = np.stack([np.repeat((n_p * v * k)[:, None], D, axis=1), np.repeat((-n_m * v * k)[:, None], D, axis=1)])
        assert o.results.moments.shape == (2, o.n_frames, D)
        assert scale_rel_err(o.results.moments, want_m) <= 1e-12
        c = o.results.timeseries
        assert c.shape == (o.n_frames, 2, 2) and not c[0].any()
        assert scale_rel_err(c[:, 0, 0], D * (n_p * v * k) ** 2) <= 1e-10
        assert scale_rel_err(c[:, 1, 1], D * (n_m * v * k) ** 2) <= 1e-10
        scale = D * (max(n_p, n_m) * v * k[-1]) ** 2
        assert np.max(np.abs(c[:, 0, 1] + D * n_p * n_m * (v * k) ** 2)) <= 1e-10 * scale
        assert np.array_equal(c[:, 0, 1], c[:, 1, 0])
        np.testing.assert_allclose(o.lag_times(), k)

    check(OnsagerHelfand(u.atoms, lab, dim_type=dim_type, fft=fft, stage_dtype=np.float64).run(), 1)
    o = OnsagerHelfand(u.atoms, lab, dim_type=dim_type, fft=fft, stage_dtype=np.float64).run(start=10, stop=390, step=4)
    assert o.n_frames == 95
    check(o, 4)
    assert list(o.results.species) == [0, 1]


# ----------------------------------------------------------------------- 2. random-walk parity
WALKS = [(2, 5, 2), (64, 40, 2), (65, 9, 3), (300, 501, 3), (513, 40, 4), (1100, 1501, 4), (2049, 1100, 8)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T,A,S", WALKS)
def test_random_walk_parity(backend, T, A, S, dtype):
    f32 = dtype == np.float32
    x, lab, w, want_m, scale, want_c = walk_case(T, A, S, f32=f32)
    sizes = np.bincount(lab, minlength=S)
    assert sizes.min() >= 1 and (A < 10 or sizes[0] > 0.5 * A)  # unequal species, nobody missing
    u = ArrayUniverse(positions=x, dimensions=BOX) if f32 else float64_universe(x)
    for fft in (True, False):
        o = OnsagerHelfand(u.atoms, lab, fft=fft, weights=w, stage_dtype=dtype).run()
        assert_moments(o.results.moments, want_m, scale)
        assert_cross(o.results.timeseries, want_c)


# ----------------------------------------------------------------------------------- 3. identities
@pytest.mark.parametrize("fft", [True, False])
def test_identities_with_conductivity_and_msd(backend, fft):
    T, A, S = 300, 41, 3
    x, lab, _ = species_walk(T, A, S, seed=5)
    z = np.array([1.0, -1.0, 2.0])
    q = z[lab]
    win = (10, 200)
    u = ArrayUniverse(positions=x, charges=q, dimensions=BOX)
    cond = ConductivityHelfand(u.atoms, fft=fft, linear_fit_window=win).run()
    # one species, weights = the charges: the conductivity's own moment and Phi
    one = OnsagerHelfand(u.atoms, np.zeros(A, dtype=int), fft=fft, weights=q).run()
    assert scale_rel_err(one.results.moments[0], cond.results.moment) <= 1e-12
    assert scale_rel_err(one.results.timeseries[:, 0, 0], cond.results.timeseries) <= 1e-10
    # species-constant charges: sum_ij z_i z_j C_ij = Phi, sigma and the transference numbers
    o = OnsagerHelfand(u.atoms, lab, fft=fft, linear_fit_window=win).run()
    c = o.results.timeseries
    phi = np.einsum("i,j,kij->k", z, z, c)
    bound = 1e-10 * float((np.abs(np.outer(z, z)) * pair_scale(c)).sum())
    assert np.max(np.abs(phi - cond.results.timeseries)) <= bound
    assert o.results.onsager.shape == (S, S) and np.array_equal(o.results.onsager, o.results.onsager.T)
    assert abs(o.conductivity(z) - cond.results.conductivity) <= 1e-9 * abs(cond.results.conductivity)
    tn = o.transference_numbers(z)
    assert tn.shape == (S,) and abs(tn.sum() - 1.0) <= 1e-12
    with pytest.raises(ValueError, match="linear_fit_window"):
        OnsagerHelfand(u.atoms, lab, fft=fft).run().conductivity(z)
    with pytest.raises(ValueError, match="charges for 3 species"):
        o.conductivity(z[:2])
    # one species of one atom: its Einstein MSD
    atom = u.atoms[7:8]
    o1 = OnsagerHelfand(atom, ["a"], fft=fft).run()
    m1 = EinsteinMSD(atom, fft=fft).run()
    assert scale_rel_err(o1.results.timeseries[:, 0, 0], m1.results.timeseries) <= 1e-12
    assert list(o1.results.species) == ["a"]


def test_units(backend, two_species):
    u, lab, n_p, n_m, v, dt = two_species
    lo, hi, T_avg = 20, 300, 350.0
    o = OnsagerHelfand(u.atoms, lab, temp_avg=T_avg, dim_type="xy", linear_fit_window=(lo, hi), stage_dtype=np.float64).run()
    t = np.arange(400) * dt
    vol, k_b, e = 40.0 * 50.0 * 60.0, 1.380649e-23, 1.602176634e-19
    for (i, j), amp in (((0, 0), n_p * n_p), ((1, 1), n_m * n_m), ((0, 1), -n_p * n_m)):
        slope = np.polyfit(t[lo:hi], 2 * amp * (v * t[lo:hi]) ** 2, 1)[0]  # A^2 / ps
        want = (slope * 1e-20 / 1e-12) / (2 * 2 * vol * 1e-30 * k_b * T_avg)  # 1 / (J m s)
        assert abs(o.results.onsager[i, j] - want) <= 1e-9 * abs(want)
    z = np.array([1.0, -1.0])
    assert abs(o.conductivity(z) - e ** 2 * (z[:, None] * z[None, :] * o.results.onsager).sum()) <= 1e-12 * o.conductivity(z)
    assert "onsager" not in OnsagerHelfand(u.atoms, lab).run().results


# ------------------------------------------------------------------------------------ 4. invariance
@pytest.mark.parametrize("fft", [True, False])
def test_permutation_and_relabelling(backend, fft):
    T, A, S = 200, 37, 4
    x, lab, w = species_walk(T, A, S, seed=9)
    base = OnsagerHelfand(float64_universe(x).atoms, lab, fft=fft, weights=w, stage_dtype=np.float64).run()
    scale = moments_ref(x, lab, w, S)[1]
    cs = pair_scale(base.results.timeseries)
    rng = np.random.default_rng(1)
    perm = rng.permutation(A)
    p = OnsagerHelfand(float64_universe(x[:, perm]).atoms, lab[perm], fft=fft, weights=w[perm], stage_dtype=np.float64).run()
    assert (np.abs(p.results.moments - base.results.moments).max(axis=(1, 2)) <= 1e-12 * scale).all()
    assert (np.abs(p.results.timeseries - base.results.timeseries).max(axis=0) <= 1e-10 * cs).all()
    # new names whose sort order permutes the species: index i of the new result is species order[i] of the old
    names = np.array(["d", "b", "a", "c"])
    order = np.argsort(names)
    r = OnsagerHelfand(float64_universe(x).atoms, names[lab], fft=fft, weights=w, stage_dtype=np.float64).run()
    assert list(r.results.species) == ["a", "b", "c", "d"]
    assert (np.abs(r.results.moments - base.results.moments[order]).max(axis=(1, 2)) <= 1e-12 * scale[order]).all()
    want_c = base.results.timeseries[:, order][:, :, order]
    assert (np.abs(r.results.timeseries - want_c).max(axis=0) <= 1e-10 * cs[order][:, order]).all()


@pytest.mark.parametrize("fft", [True, False])
def test_empty_species_is_exactly_zero(backend, fft):
    """Labels 0 and 2 with n_species = 4 through the binding: species 1 and 3 have no atoms."""
    T, A = 150, 23
    x, lab, w = species_walk(T, A, 2, seed=3)
    lab = (2 * lab).astype(np.int32)
    c = staged(backend, x)
    try:
        m, cr = c.onsager(fft, lab, n_species=4, weights=w)
    finally:
        c.close()
    want_m, scale = moments_ref(x, lab, w, 4)
    assert_moments(m, want_m, scale)
    assert_cross(cr, cross_ref(want_m))
    for s in (1, 3):
        assert not m[s].any() and not cr[:, s, :].any() and not cr[:, :, s].any()
    assert cr[:, 0, 2].any()


# ------------------------------------------------------------------------------------- 5. exactness
def grid_walk(T, A, S, seed):
    """Positions on a 1/64 grid (exact in float32 too) and integer weights: every partial sum is exact in float64."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 64 * 64, size=(1, A, 3)) + np.cumsum(rng.integers(-40, 41, size=(T, A, 3)), axis=0)
    lab = rng.permutation(np.where(rng.random(A) < 0.7, 0, rng.integers(1, S, size=A))).astype(np.int32)
    w = rng.integers(1, 4, size=A).astype(np.float64)
    return k, k / 64.0, lab, w


def test_exact_moments_and_bit_identical_repeats(backend):
    T, A, S = 1100, 1501, 3
    k, x, lab, w = grid_walk(T, A, S, seed=11)
    dk = k - k[0]
    want = np.stack([(dk[:, lab == s, :] * w[lab == s].astype(np.int64)[None, :, None]).sum(axis=1) for s in range(S)]) / 64.0
    c = staged(backend, x)
    try:
        for fft in (True, False):
            m1, c1 = c.onsager(fft, lab, weights=w)
            m2, c2 = c.onsager(fft, lab, weights=w)
            assert np.array_equal(m1, want), "exact partial sums: the moments do not depend on the summation order"
            assert np.array_equal(m1, m2) and np.array_equal(c1, c2)
            assert_cross(c1, cross_ref(want))
    finally:
        c.close()


# ---------------------------------------------------------------------------------------- 6. unwrap
@pytest.mark.parametrize("fft", [True, False])
def test_wrapped_equals_unwrapped(backend, fft):
    rng = np.random.default_rng(17)
    T, A = 300, 9
    L = np.array([16.0, 32.0, 8.0])
    k0 = rng.integers(0, 64 * 8, size=(1, A, 3))
    steps = rng.choice([-1, 1], size=(1, A, 3)) * 48 + rng.integers(-40, 41, size=(T - 1, A, 3))
    u = np.concatenate([k0, k0 + np.cumsum(steps, axis=0)]) / 64.0 * (L / 8.0)
    x = u - np.floor(u / L) * L
    box = [*L, 90.0, 90.0, 90.0]
    lab = np.arange(A) % 3
    for dim_type in ("xyz", "xz", "y"):
        kw = dict(fft=fft, dim_type=dim_type, linear_fit_window=(10, 200))
        want = OnsagerHelfand(ArrayUniverse(positions=u, dimensions=box).atoms, lab, **kw).run()
        got = OnsagerHelfand(ArrayUniverse(positions=x, dimensions=box).atoms, lab, unwrap=True, **kw).run()
        assert np.array_equal(got.results.moments, want.results.moments)  # grid positions, integer image shifts
        assert (np.abs(got.results.timeseries - want.results.timeseries).max(axis=0)
                <= 1e-10 * pair_scale(want.results.timeseries)).all()
        np.testing.assert_allclose(got.results.onsager, want.results.onsager, rtol=1e-9, atol=1e-9 * np.abs(want.results.onsager).max())
        raw = OnsagerHelfand(ArrayUniverse(positions=x, dimensions=box).atoms, lab, **kw).run()
        assert scale_rel_err(raw.results.moments, want.results.moments) > 0.5


# ------------------------------------------------------------------------------------ 7. errors
def test_api_errors(backend):
    x = species_walk(10, 3, 2, seed=1)[0]
    u = ArrayUniverse(positions=x, dimensions=BOX)
    lab = [0, 1, 0]
    with pytest.raises(NoDataError, match="positions and box volume"):  # no positions
        no_pos = ArrayUniverse(velocities=x, dimensions=BOX)
        no_pos.trajectory._pos = None
        OnsagerHelfand(no_pos.atoms, lab).run()
    with pytest.raises(NoDataError):  # zero volume
        OnsagerHelfand(ArrayUniverse(positions=x).atoms, lab).run()
    with pytest.raises(ValueError, match="species: 2 labels for 3 atoms"):
        OnsagerHelfand(u.atoms, [0, 1])
    with pytest.raises(ValueError, match="weights: 2 values for 3 atoms"):
        OnsagerHelfand(u.atoms, lab, weights=[1.0, 2.0])
    big = ArrayUniverse(positions=species_walk(4, 9, 2, seed=1)[0], dimensions=BOX)
    with pytest.raises(ValueError, match="9 distinct labels, at most 8"):
        OnsagerHelfand(big.atoms, np.arange(9))
    assert OnsagerHelfand(big.atoms, np.arange(9) % 8).run().results.timeseries.shape == (4, 8, 8)
    with pytest.raises(TypeError, match="UpdatingAtomGroup"):
        OnsagerHelfand(UpdatingAtomGroup(), lab)
    with pytest.raises(ValueError, match="invalid dim_type: foo specified"):
        OnsagerHelfand(u.atoms, lab, dim_type="foo")
    with pytest.raises(TypeError, match="by_particle"):
        OnsagerHelfand(u.atoms, lab, by_particle=True)
    assert OnsagerHelfand(u.atoms, lab, by_particle=False).run().results.timeseries.shape == (10, 2, 2)
    with pytest.raises(ValueError, match="exclusive"):
        OnsagerHelfand(u.atoms, lab, devices=[0], distributed=True)
    # species by the name of a per-atom attribute of the group
    u.atoms.types = np.array(["Li", "TFSI", "Li"])
    o = OnsagerHelfand(u.atoms, "types").run()
    assert list(o.results.species) == ["Li", "TFSI"] and list(o.species_index) == [0, 1, 0]


def test_no_run_hooks_of_mdanalysis():
    """MDAnalysis >= 2.8's run() calls these private hooks; a class (or its StagedAnalysis base) defining one breaks it."""
    from transport_analysis_amd import _base

    hooks = {"_compute", "_configure_backend", "_setup_computation_groups", "_get_aggregator", "_define_run_frames",
             "_prepare_sliced_trajectory"}
    mro = OnsagerHelfand.__mro__
    own = [k for c in mro[:mro.index(_base.AnalysisBase)] for k in vars(c)]
    assert not set(own) & hooks


def last_error(c):
    return _lib.lib().ta_last_error(c._h).decode()


def test_cabi_argument_checks(backend):
    """ta_onsager / ta_onsager_cross: every TA_E_INVALID and TA_E_STATE case with its message; the cross MSD of hand-made
    moments with no slab staged; on the CPU backend the device entry points are unsupported."""
    L = _lib.lib()
    P = _lib._ptr
    c = context(backend)
    T, A, D, S = 8, 5, 2, 3
    x = species_walk(T, A, S, seed=2, D=D)[0]
    lab = np.array([0, 2, 1, 0, 2], dtype=np.int32)
    w = np.array([1.0, 2.0, 0.5, 1.0, 2.0])
    mom, cr = np.zeros((S, T, D)), np.zeros((T, S, S))
    # the cross MSD of given moments needs no staged slab
    hand = np.cumsum(np.random.default_rng(4).standard_normal((S, 70, D)), axis=1)
    for fft in (0, 1):
        assert_cross(c.onsager_cross(hand, fft), cross_ref(hand))
    assert not c.onsager_cross(hand[:, :1], 1).any()  # one frame: lag 0 alone
    assert L.ta_onsager(c._h, 1, S, P(lab), P(w), P(mom), P(cr)) == TA_E_STATE
    assert "not been staged" in last_error(c)
    (view,) = c.stage_alloc(T, A, D)
    view[:] = x
    c.stage_commit(0, T)
    assert L.ta_onsager(c._h, 2, S, P(lab), P(w), P(mom), P(cr)) == TA_E_INVALID
    assert "fft must be 0 or 1" in last_error(c)
    for bad in (0, -1, MAX_SPECIES + 1):
        assert L.ta_onsager(c._h, 1, bad, P(lab), P(w), P(mom), P(cr)) == TA_E_INVALID
        assert "n_species must be 1 ... 8" in last_error(c)
    assert L.ta_onsager(c._h, 1, S, None, P(w), P(mom), P(cr)) == TA_E_INVALID
    assert "species labels are NULL" in last_error(c)
    assert L.ta_onsager(c._h, 1, S, P(lab), P(w), None, P(cr)) == TA_E_INVALID
    assert "moments output is NULL" in last_error(c)
    assert L.ta_onsager(None, 1, S, P(lab), P(w), P(mom), P(cr)) == TA_E_INVALID
    for bad in (3, -1):  # a label outside 0 ... n_species - 1, checked on the host
        lab_bad = lab.copy()
        lab_bad[3] = bad
        assert L.ta_onsager(c._h, 1, S, P(lab_bad), P(w), P(mom), P(cr)) == TA_E_INVALID
        assert f"species label {bad} of atom 3" in last_error(c)
    assert L.ta_onsager_cross(c._h, 2, P(mom), S, T, D, P(cr)) == TA_E_INVALID
    assert L.ta_onsager_cross(c._h, 1, P(mom), 9, T, D, P(cr)) == TA_E_INVALID
    assert L.ta_onsager_cross(c._h, 1, None, S, T, D, P(cr)) == TA_E_INVALID
    assert L.ta_onsager_cross(c._h, 1, P(mom), S, T, D, None) == TA_E_INVALID
    assert L.ta_onsager_cross(c._h, 1, P(mom), S, 0, D, P(cr)) == TA_E_INVALID
    assert L.ta_onsager_cross(c._h, 1, P(mom), S, T, 4, P(cr)) == TA_E_INVALID
    assert L.ta_onsager_cross(None, 1, P(mom), S, T, D, P(cr)) == TA_E_INVALID
    assert L.ta_group_onsager(None, 1, S, P(lab), P(w), P(mom), P(cr)) == TA_E_INVALID
    want_m, scale = moments_ref(x, lab, w, S)
    for fft in (0, 1):
        assert L.ta_onsager(c._h, fft, S, P(lab), P(w), P(mom), P(cr)) == 0
        assert_moments(mom, want_m, scale)
        assert_cross(cr, cross_ref(want_m))
    assert L.ta_onsager(c._h, 1, S, P(lab), None, P(mom), None) == 0  # unit weights, the moments alone
    assert_moments(mom, *moments_ref(x, lab, None, S))
    assert_cross(c.onsager_cross(mom, 1), cross_ref(mom))  # ... and the staged slab is still there
    assert L.ta_onsager(c._h, 1, S, P(lab), P(w), P(mom), P(cr)) == 0
    with pytest.raises(ValueError, match="species: 2 labels for 5 atoms"):
        c.onsager(True, lab[:2])
    with pytest.raises(ValueError, match="weights"):
        c.onsager(True, lab, weights=w[:2])
    if backend == "cpu":
        v = ctypes.c_void_p(16)
        assert L.ta_onsager_staged(c._h, 1, S, v, v, v, None, None) == TA_E_UNSUPPORTED
        assert L.ta_onsager_dev(c._h, v, T, A, D, A * D, 1, S, v, v, v, None, None) == TA_E_UNSUPPORTED
        assert "CPU backend" in last_error(c)
    c.close()


@pytest.mark.gpu
def test_onsager_dev_and_staged_argument_checks():
    import torch

    T, A, D, S = 40, 7, 3, 2
    x, lab, w = species_walk(T, A, S, seed=8)
    dev = torch.device("cuda", 0)
    d_x, d_lab, d_w = torch.from_numpy(x.reshape(T, A * D)).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(w).to(dev)
    mom = torch.zeros((S, T, D), dtype=torch.float64, device=dev)
    L = _lib.lib()
    c = _lib.Context(0)
    V = ctypes.c_void_p
    p, pl, pw, pm = V(d_x.data_ptr()), V(d_lab.data_ptr()), V(d_w.data_ptr()), V(mom.data_ptr())
    assert L.ta_onsager_staged(c._h, 1, S, pl, pw, pm, None, None) == TA_E_STATE  # nothing staged
    assert L.ta_onsager_dev(c._h, p, T, A, 4, A * D, 1, S, pl, pw, pm, None, None) == TA_E_INVALID  # dim
    assert L.ta_onsager_dev(c._h, p, T, A, D, A * D - 1, 1, S, pl, pw, pm, None, None) == TA_E_INVALID  # ld_row
    assert L.ta_onsager_dev(c._h, p, 0, A, D, A * D, 1, S, pl, pw, pm, None, None) == TA_E_INVALID  # n_frames
    assert L.ta_onsager_dev(c._h, None, T, A, D, A * D, 1, S, pl, pw, pm, None, None) == TA_E_INVALID
    assert L.ta_onsager_dev(c._h, p, T, A, D, A * D, 1, S, None, pw, pm, None, None) == TA_E_INVALID  # labels
    assert L.ta_onsager_dev(c._h, p, T, A, D, A * D, 1, S, pl, pw, None, None, None) == TA_E_INVALID  # moments
    assert L.ta_onsager_dev(c._h, p, T, A, D, A * D, 2, S, pl, pw, pm, None, None) == TA_E_INVALID  # fft
    assert L.ta_onsager_dev(c._h, p, T, A, D, A * D, 1, 9, pl, pw, pm, None, None) == TA_E_INVALID  # n_species
    c.onsager_dev(d_x.data_ptr(), T, A, D, A * D, True, S, d_lab.data_ptr(), mom.data_ptr(), d_w.data_ptr())
    torch.cuda.synchronize()
    assert_moments(mom.cpu().numpy(), *moments_ref(x, lab, w, S))
    # device labels are not checked: an atom with a label out of range is left out of every moment
    lab_bad = lab.copy()
    lab_bad[2], lab_bad[5] = 7, -3
    c.onsager_dev(d_x.data_ptr(), T, A, D, A * D, True, S, torch.from_numpy(lab_bad).to(dev).data_ptr(), mom.data_ptr(),
                  d_w.data_ptr())
    torch.cuda.synchronize()
    keep = np.ones(A, dtype=bool)
    keep[[2, 5]] = False
    assert_moments(mom.cpu().numpy(), *moments_ref(x[:, keep], lab[keep], w[keep], S))
    c.close()


# -------------------------------------------------------------- 8. several devices, distributed
@pytest.mark.gpu
@pytest.mark.parametrize("fft", [True, False])
def test_devices_two_members_one_gpu(fft):
    x, lab, w = species_walk(400, 11, 3, seed=8)
    u = ArrayUniverse(positions=x, dimensions=BOX)
    kw = dict(fft=fft, weights=w, linear_fit_window=(10, 200))
    one = OnsagerHelfand(u.atoms, lab, **kw).run()
    two = OnsagerHelfand(u.atoms, lab, devices=[0, 0], **kw).run()
    assert two.results.device_ranges == [(0, 5), (5, 11)]
    scale = moments_ref(x, lab, w, 3)[1]
    assert (np.abs(two.results.moments - one.results.moments).max(axis=(1, 2)) <= 1e-12 * scale).all()
    assert (np.abs(two.results.timeseries - one.results.timeseries).max(axis=0) <= 1e-10 * pair_scale(one.results.timeseries)).all()
    np.testing.assert_allclose(two.results.onsager, one.results.onsager, rtol=1e-9, atol=1e-9 * np.abs(one.results.onsager).max())


@pytest.mark.gpu
@pytest.mark.parametrize("fft", [True, False], ids=["fft", "direct"])
def test_group_onsager_odd_member_slabs(fft):
    """ta_group_onsager on devices=[0, 0] at 1502 atoms x 3: each member holds 751 atoms, 2253 columns, so both slabs end
    on an unpaired column and the second member starts mid-way (atom 751) through the labels and weights."""
    T, A, S = 1100, 1502, 3
    x, lab, w = species_walk(T, A, S, seed=5)
    want_m, scale = moments_ref(x, lab, w, S)
    c = staged("hip", x)
    try:
        one = c.onsager(fft, lab, weights=w)
    finally:
        c.close()
    g = _lib.Group([0, 0])
    try:
        (views,) = g.stage_alloc(T, A, 3)
        assert g.shards == [(0, 751), (751, 1502)]
        for (lo, hi), v in zip(g.shards, views):
            v[:] = x[:, lo:hi]
        g.stage_commit(0, T)
        m, cr = g.onsager(fft, lab, weights=w)
        bad = lab.copy()
        bad[1000] = 3
        assert _lib.lib().ta_group_onsager(g._h, int(fft), S, _lib._ptr(bad), None, _lib._ptr(m), None) == TA_E_INVALID
    finally:
        g.close()
    assert_moments(m, want_m, scale)
    assert (np.abs(m - one[0]).max(axis=(1, 2)) <= 1e-12 * scale).all()
    assert_cross(cr, cross_ref(want_m))
    assert (np.abs(cr - one[1]).max(axis=0) <= 1e-10 * pair_scale(one[1])).all()


def _onsager_worker(rank, world, port, T, A, out_dir):
    import sys

    import torch.distributed as dist

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from onsager_ref import species_walk
    from transport_analysis_amd import OnsagerHelfand
    from transport_analysis_amd._mini_mda import ArrayUniverse

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    x, lab, w = species_walk(T, A, 2, seed=12)
    u = ArrayUniverse(positions=x, dimensions=BOX)
    out = {}
    for fft in (True, False):
        o = OnsagerHelfand(u.atoms, lab, fft=fft, weights=w, linear_fit_window=(5, 60), distributed=True, device="cpu").run()
        out[f"m_{int(fft)}"] = o.results.moments
        out[f"c_{int(fft)}"] = o.results.timeseries
        out[f"l_{int(fft)}"] = o.results.onsager
        out["range"] = np.array(o.results.particle_range)
    np.savez(os.path.join(out_dir, f"ons_{rank}.npz"), **out)
    dist.destroy_process_group()


@pytest.mark.parametrize("A", [7, 1])
def test_distributed_gloo_world2_cpu_backend(tmp_path, A):
    """A = 7, xyz: rank 0 holds atoms 0-2 = 9 columns, so the column pair (8, 9) of the whole slab is cut between the
    ranks; A = 1: one rank holds no atom and contributes zeros."""
    import torch.multiprocessing as mp

    T, world = 90, 2
    port = 37600 + (os.getpid() % 2000) + A
    mp.spawn(_onsager_worker, args=(world, port, T, A, str(tmp_path)), nprocs=world, join=True)
    x, lab, w = species_walk(T, A, 2, seed=12)
    u = ArrayUniverse(positions=x, dimensions=BOX)
    for fft in (True, False):
        serial = OnsagerHelfand(u.atoms, lab, fft=fft, weights=w, linear_fit_window=(5, 60), device="cpu").run()
        scale = moments_ref(x.astype(np.float32).astype(np.float64), lab, w, serial.n_species)[1]
        for r in range(world):
            z = np.load(tmp_path / f"ons_{r}.npz")
            assert tuple(z["range"]) == ((A * r) // world, (A * (r + 1)) // world)
            assert (np.abs(z[f"m_{int(fft)}"] - serial.results.moments).max(axis=(1, 2)) <= 1e-12 * scale).all()
            assert (np.abs(z[f"c_{int(fft)}"] - serial.results.timeseries).max(axis=0)
                    <= 1e-10 * pair_scale(serial.results.timeseries)).all()
            np.testing.assert_allclose(z[f"l_{int(fft)}"], serial.results.onsager, rtol=1e-9,
                                       atol=1e-9 * np.abs(serial.results.onsager).max())
