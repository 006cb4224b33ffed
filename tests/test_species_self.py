"""self_terms=True of OnsagerHelfand / OnsagerGreenKubo / ConductivityGreenKubo and the ta_species_self* entry points: parity
with the reference of species_self_ref at random shapes from one frame up, the closed form of ballistic species, what
self_terms=False leaves alone, the distinct part of one-atom species, the identities with ConductivityHelfand,
VelocityAutocorr and EinsteinMSD, every C-ABI error with its message, several devices and torch.distributed.  Every
class-level test runs on the library's CPU backend and, marked gpu, on the HIP path."""
import ctypes
import os

import numpy as np
import pytest

from conftest import scale_rel_err
from species_self_ref import SELF_MSD, SELF_VACF, assert_self, self_at_lags
from current_ref import species_velocities
from onsager_ref import species_walk
from transport_analysis_amd import (ConductivityGreenKubo, ConductivityHelfand, EinsteinMSD, OnsagerGreenKubo, OnsagerHelfand,
                                    VelocityAutocorr, _lib)
from transport_analysis_amd._mini_mda import ArrayUniverse

DIMS = [("xyz", [0, 1, 2]), ("xy", [0, 1]), ("xz", [0, 2]), ("yz", [1, 2]), ("x", [0]), ("y", [1]), ("z", [2])]
BOX = [40.0, 50.0, 60.0, 90, 90, 90]
TA_E_INVALID, TA_E_STATE, TA_E_UNSUPPORTED = -1, -4, -5
SELF_KEYS = ("timeseries_self", "species_counts", "species_weight2", "onsager_self", "onsager_distinct")


@pytest.fixture(params=["cpu", pytest.param("hip", marks=pytest.mark.gpu)])
def backend(request, monkeypatch):
    if request.param == "cpu":
        monkeypatch.setenv("TA_AMD_DEVICE", "cpu")  # the library's opt-in CPU backend behind the same C symbols
    else:
        monkeypatch.delenv("TA_AMD_DEVICE", raising=False)
        assert _lib.device_count() >= 1
    return request.param


def universe(positions=None, velocities=None, dt=1.0, f64=True, **kw):
    """Timesteps that hand out float64 arrays with f64 (the closed forms are not exact in float32)"""
    u = ArrayUniverse(positions=positions, velocities=velocities, dimensions=BOX, dt=dt, **kw)
    if f64 and positions is not None:
        u.trajectory._pos = np.ascontiguousarray(positions, dtype=np.float64)
    if f64 and velocities is not None:
        u.trajectory._vel = np.ascontiguousarray(velocities, dtype=np.float64)
    return u


def context(backend):
    return _lib.Context("cpu" if backend == "cpu" else 0)


# --------------------------------------------------------------------------- 1. parity at random shapes
def random_shapes():
    """(T, A, S) from one frame up: fixed corners and draws of a seeded generator"""
    rng = np.random.default_rng(20261017)
    shapes = [(1, 5, 2), (2, 9, 3), (64, 40, 2), (65, 9, 3), (513, 40, 4)]
    shapes += [(int(rng.integers(3, 700)), int(rng.integers(1, 300)), int(rng.integers(1, 9))) for _ in range(4)]
    return shapes


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["stage32", "stage64"])
@pytest.mark.parametrize("T,A,S", random_shapes())
def test_random_parity_both_routes(backend, T, A, S, dtype):
    f32 = dtype == np.float32
    lags = np.arange(T)
    x, lab, w = species_walk(T, A, S, seed=T + A + S)
    v = species_velocities(T, A, S, seed=T + A + S)[0]
    if f32:
        x, v = x.astype(np.float32).astype(np.float64), v.astype(np.float32).astype(np.float64)
    S_run = int(np.unique(lab).size)  # the classes index the labels that occur
    idx = np.unique(lab, return_inverse=True)[1]
    want_x, want_v = self_at_lags(x, idx, w, S_run, SELF_MSD, lags), self_at_lags(v, idx, w, S_run, SELF_VACF, lags)
    u = universe(x, v, f64=not f32)
    for fft in (True, False):
        o = OnsagerHelfand(u.atoms, lab, fft=fft, weights=w, stage_dtype=dtype, self_terms=True).run()
        assert o.results.timeseries_self.shape == (T, S_run) and not o.results.timeseries_self[0].any()
        assert_self(o.results.timeseries_self.T, want_x, lags, what=f"helfand fft={fft}")
        g = OnsagerGreenKubo(u.atoms, lab, fft=fft, weights=w, stage_dtype=dtype, self_terms=True).run()
        assert g.results.timeseries_self.shape == (T, S_run)
        assert_self(g.results.timeseries_self.T, want_v, lags, what=f"green-kubo fft={fft}")
        for r in (o.results, g.results):
            assert np.array_equal(r.species_counts, np.bincount(idx, minlength=S_run))
            np.testing.assert_allclose(r.species_weight2, np.bincount(idx, weights=w ** 2, minlength=S_run), rtol=1e-14)


@pytest.mark.parametrize("dim_type,cols", DIMS)
def test_dim_types_and_frame_windows(backend, dim_type, cols):
    T, A, S = 200, 23, 3
    x, lab, w = species_walk(T, A, S, seed=31)
    v = species_velocities(T, A, S, seed=31)[0]
    u = universe(x, v)
    sl = slice(10, 190, 4)
    lags = np.arange(45)
    o = OnsagerHelfand(u.atoms, lab, dim_type=dim_type, weights=w, stage_dtype=np.float64, self_terms=True).run(start=10, stop=190, step=4)
    g = OnsagerGreenKubo(u.atoms, lab, dim_type=dim_type, weights=w, stage_dtype=np.float64, self_terms=True).run(start=10, stop=190, step=4)
    assert o.n_frames == g.n_frames == 45
    assert_self(o.results.timeseries_self.T, self_at_lags(x[sl][:, :, cols], lab, w, S, SELF_MSD, lags), lags, what=dim_type)
    assert_self(g.results.timeseries_self.T, self_at_lags(v[sl][:, :, cols], lab, w, S, SELF_VACF, lags), lags, what=dim_type)


# -------------------------------------------------------------------------------- 2. closed form
@pytest.mark.parametrize("fft", [True, False])
def test_closed_form_ballistic_species(backend, fft):
    """Species s moves at speed u_s along every axis: MSD_n = D (u_s k dt)^2 and the VACF is D u_s^2 at every lag."""
    T, dt, D = 300, 2.0, 3
    lab = np.array([0, 1, 2, 1, 0, 1, 0])
    speed = np.array([0.5, -0.25, 1.5])
    w = np.array([1.0, 2.0, 0.5, 1.0, 2.0, 0.5, 1.0])
    t = np.arange(T) * dt
    vel = np.broadcast_to(speed[lab][None, :, None], (T, lab.size, D)).copy()
    pos = 100.0 * (np.arange(lab.size) + 1)[None, :, None] + vel * t[:, None, None]
    u = universe(pos, vel, dt=dt)
    w2 = np.bincount(lab, weights=w ** 2)
    o = OnsagerHelfand(u.atoms, lab, fft=fft, weights=w, stage_dtype=np.float64, self_terms=True, linear_fit_window=(20, 250)).run()
    g = OnsagerGreenKubo(u.atoms, lab, fft=fft, weights=w, stage_dtype=np.float64, self_terms=True).run()
    for s in range(3):
        assert scale_rel_err(o.results.timeseries_self[:, s], w2[s] * D * (speed[s] * t) ** 2) <= 1e-10
        assert scale_rel_err(g.results.timeseries_self[:, s], np.full(T, w2[s] * D * speed[s] ** 2)) <= 1e-10
    # the integral of a constant: D_s = u_s^2 (t_stop - t_start), the rule does not matter
    np.testing.assert_allclose(g.self_diffusivities(0, 101, 1), speed ** 2 * 100 * dt, rtol=1e-9)
    np.testing.assert_allclose(g.self_diffusivities(0, 101, 1, odd=True), speed ** 2 * 100 * dt, rtol=1e-9)
    np.testing.assert_allclose(g.onsager_self_gk_odd(0, 101, 1), g.onsager_self_gk(0, 101, 1), rtol=1e-9)
    # the slope of a parabola over the window, as polyfit sees it
    want = np.array([np.polyfit(t[20:250], (speed[s] * t[20:250]) ** 2, 1)[0] / 2 for s in range(3)])
    np.testing.assert_allclose(o.self_diffusivities(), want, rtol=1e-9)


# ------------------------------------------------------------------- 3. self_terms=False changes nothing
def test_self_terms_false_leaves_results_and_timeline(backend):
    T, A, S = 120, 17, 3
    x, lab, w = species_walk(T, A, S, seed=3)
    v = species_velocities(T, A, S, seed=3)[0]
    u = universe(x, v)
    for cls, keys in ((OnsagerHelfand, {"species", "moments", "timeseries"}), (OnsagerGreenKubo, {"species", "currents", "timeseries"})):
        kw = dict(linear_fit_window=(5, 60)) if cls is OnsagerHelfand else {}
        plain = cls(u.atoms, lab, weights=w, **kw).run()
        also = cls(u.atoms, lab, weights=w, self_terms=True, **kw).run()
        extra = set(SELF_KEYS) & set(plain.results)
        assert not extra, extra
        assert keys <= set(plain.results)
        for k in set(plain.results) - {"species"}:
            if isinstance(plain.results[k], np.ndarray):
                assert np.array_equal(plain.results[k], also.results[k]), k  # the self pass does not disturb the rest
        for method in ("self_diffusivities", "conductivity_nernst_einstein", "ionicity"):
            with pytest.raises(ValueError, match="pass self_terms=True"):
                getattr(plain, method)(*(() if method == "self_diffusivities" else (np.ones(S),)))
    with pytest.raises(ValueError, match="pass self_terms=True"):
        OnsagerGreenKubo(u.atoms, lab).run().onsager_self_gk()
    with pytest.raises(ValueError, match="pass self_terms=True"):
        OnsagerGreenKubo(u.atoms, lab).run().onsager_self_gk_odd()
    with pytest.raises(ValueError, match="linear_fit_window"):
        OnsagerHelfand(u.atoms, lab, self_terms=True).run().self_diffusivities()
    if backend == "hip":  # no extra kernel: the timeline of the plain calls holds no sort pass
        c = _lib.Context(0)
        c.set_option("timeline", 1)
        (view,) = c.stage_alloc(T, A, 3)
        view[:] = x
        c.stage_commit(0, T)
        c.onsager(True, lab, weights=w)
        assert "k_species_sort" not in [n for n, _ in c.kernel_timeline(64)]
        c.current(True, lab, weights=w)
        assert "k_species_sort" not in [n for n, _ in c.kernel_timeline(64)]
        c.species_self(SELF_MSD, 1, lab, weights=w)
        assert "k_species_sort" in [n for n, _ in c.kernel_timeline(64)]
        c.close()


# -------------------------------------------------------------------------------- 4. identities
@pytest.mark.parametrize("fft", [True, False])
def test_one_atom_per_species_has_no_distinct_part(backend, fft):
    T, A = 300, 5
    x, _, w = species_walk(T, A, A, seed=13)
    o = OnsagerHelfand(universe(x).atoms, np.arange(A), fft=fft, weights=w, stage_dtype=np.float64, self_terms=True,
                       linear_fit_window=(10, 200)).run()
    c = o.results.timeseries
    for s in range(A):  # C_ss is the weighted MSD of the species' one atom
        assert scale_rel_err(o.results.timeseries_self[:, s], c[:, s, s]) <= 1e-10
    assert np.abs(np.diag(o.results.onsager_distinct)).max() <= 1e-9 * np.abs(np.diag(o.results.onsager)).max()
    off = ~np.eye(A, dtype=bool)
    assert np.array_equal(o.results.onsager_distinct[off], o.results.onsager[off])


@pytest.mark.parametrize("fft", [True, False])
def test_nernst_einstein_and_diffusivities_helfand(backend, fft):
    T, A, S = 300, 41, 3
    x, lab, _ = species_walk(T, A, S, seed=5)
    z = np.array([1.0, -1.0, 2.0])
    win = (10, 200)
    u = ArrayUniverse(positions=x, charges=z[lab], dimensions=BOX)
    cond = ConductivityHelfand(u.atoms, fft=fft, linear_fit_window=win, nernst_einstein=True).run()
    o = OnsagerHelfand(u.atoms, lab, fft=fft, linear_fit_window=win, self_terms=True).run()
    ne = o.conductivity_nernst_einstein(z)
    assert abs(ne - cond.results.conductivity_self) <= 1e-9 * abs(cond.results.conductivity_self)
    assert abs(o.ionicity(z) - cond.results.conductivity / cond.results.conductivity_self) <= 1e-8 * abs(o.ionicity(z))
    assert o.results.onsager_self.shape == (S,)
    np.testing.assert_allclose(o.results.onsager_distinct, o.results.onsager - np.diag(o.results.onsager_self), rtol=0, atol=0)
    with pytest.raises(ValueError, match="charges for 3 species"):
        o.conductivity_nernst_einstein(z[:2])
    # per species: EinsteinMSD on its atoms (a mean over them) has the same slope / (2 D)
    d = o.self_diffusivities()
    for s in range(S):
        sel = np.flatnonzero(lab == s)
        m = EinsteinMSD(ArrayUniverse(positions=x[:, sel], dimensions=BOX), fft=fft).run()
        t = np.arange(T, dtype=np.float64)
        want = np.polyfit(t[win[0]:win[1]], m.results.timeseries[win[0]:win[1]], 1)[0] / (2 * 3)
        assert abs(d[s] - want) <= 1e-9 * abs(want)


@pytest.mark.parametrize("fft", [True, False])
def test_self_gk_one_species_is_velocity_autocorr(backend, fft):
    from scipy import integrate

    T, A = 300, 29
    v = species_velocities(T, A, 1, seed=7)[0]
    u = ArrayUniverse(velocities=v, charges=np.ones(A), dimensions=BOX)
    va = VelocityAutocorr(u.atoms, fft=fft, by_particle=False).run()
    g = OnsagerGreenKubo(u.atoms, np.zeros(A, dtype=int), fft=fft, self_terms=True).run()
    lag_sum = va.results.timeseries * A  # the class divides by the atoms
    assert scale_rel_err(g.results.timeseries_self[:, 0], lag_sum) <= 1e-10
    t = g.lag_times()
    for window in ((0, 0, 1), (5, 200, 3)):
        sl = slice(window[0], window[1] or T, window[2])
        factor = g._factor()
        want = integrate.trapezoid(lag_sum[sl], t[sl]) * factor
        assert abs(g.onsager_self_gk(*window)[0] - want) <= 1e-9 * abs(want)
        want = integrate.simpson(y=lag_sum[sl], x=t[sl]) * factor
        assert abs(g.onsager_self_gk_odd(*window)[0] - want) <= 1e-9 * abs(want)
        assert abs(g.self_diffusivities(*window)[0] - va.self_diffusivity_gk(*window)) <= 1e-9 * abs(va.self_diffusivity_gk(*window))
    # ConductivityGreenKubo passes the keyword on: sum_n q_n^2 VACF_n, here with unit charges
    cg = ConductivityGreenKubo(u.atoms, fft=fft, self_terms=True).run()
    assert cg.results.timeseries_self.shape == (T, 1)
    assert np.array_equal(cg.results.timeseries_self, g.results.timeseries_self)
    e2 = 1.602176634e-19 ** 2
    assert abs(cg.conductivity_nernst_einstein([1.0]) - e2 * g.onsager_self_gk()[0]) <= 1e-12 * abs(e2 * g.onsager_self_gk()[0])
    assert abs(cg.ionicity([1.0]) - cg.conductivity_gk() / cg.conductivity_nernst_einstein([1.0])) <= 1e-12
    assert "timeseries_self" not in ConductivityGreenKubo(u.atoms, fft=fft).run().results


# ------------------------------------------------------------------------------------ 5. C-ABI
def last_error(c):
    return _lib.lib().ta_last_error(c._h).decode()


def test_cabi_argument_checks(backend):
    """ta_species_self: every TA_E_INVALID and TA_E_STATE case with its message; counts; NULL weights and counts; on the CPU
    backend the device entry points are unsupported."""
    L = _lib.lib()
    P = _lib._ptr
    c = context(backend)
    T, A, D, S = 8, 5, 2, 3
    x = species_walk(T, A, S, seed=2, D=D)[0]
    lab = np.array([0, 2, 1, 0, 2], dtype=np.int32)
    w = np.array([1.0, 2.0, 0.5, 1.0, 2.0])
    out, cnt = np.zeros((S, T)), np.zeros(S, dtype=np.int64)
    assert L.ta_species_self(c._h, 0, 1, S, P(lab), P(w), P(out), P(cnt)) == TA_E_STATE
    assert "not been staged" in last_error(c)
    (view,) = c.stage_alloc(T, A, D)
    view[:] = x
    c.stage_commit(0, T)
    for bad in (2, -1):
        assert L.ta_species_self(c._h, bad, 1, S, P(lab), P(w), P(out), P(cnt)) == TA_E_INVALID
        assert "quantity must be TA_SELF_MSD (0) or TA_SELF_VACF (1)" in last_error(c)
    assert L.ta_species_self(c._h, 0, 2, S, P(lab), P(w), P(out), P(cnt)) == TA_E_INVALID
    assert "fft must be 0 or 1" in last_error(c)
    for bad in (0, -1, 9):
        assert L.ta_species_self(c._h, 0, 1, bad, P(lab), P(w), P(out), P(cnt)) == TA_E_INVALID
        assert "n_species must be 1 ... 8" in last_error(c)
    assert L.ta_species_self(c._h, 0, 1, S, None, P(w), P(out), P(cnt)) == TA_E_INVALID
    assert "species labels are NULL" in last_error(c)
    assert L.ta_species_self(c._h, 0, 1, S, P(lab), P(w), None, P(cnt)) == TA_E_INVALID
    assert "self output is NULL" in last_error(c)
    assert L.ta_species_self(None, 0, 1, S, P(lab), P(w), P(out), P(cnt)) == TA_E_INVALID
    assert L.ta_group_species_self(None, 0, 1, S, P(lab), P(w), P(out), P(cnt)) == TA_E_INVALID
    out[:] = 7.0
    for bad in (3, -1):  # a label outside 0 ... n_species - 1: checked on the host before anything is written
        lab_bad = lab.copy()
        lab_bad[3] = bad
        assert L.ta_species_self(c._h, 0, 1, S, P(lab_bad), P(w), P(out), P(cnt)) == TA_E_INVALID
        assert f"species label {bad} of atom 3" in last_error(c)
        assert (out == 7.0).all()
    lags = np.arange(T)
    for quantity in (SELF_MSD, SELF_VACF):
        for fft in (0, 1):
            assert L.ta_species_self(c._h, quantity, fft, S, P(lab), P(w), P(out), P(cnt)) == 0
            assert_self(out, self_at_lags(x, lab, w, S, quantity, lags), lags)
            assert list(cnt) == [2, 1, 2]
    assert L.ta_species_self(c._h, 0, 1, S, P(lab), None, P(out), None) == 0  # unit weights, no counts
    assert_self(out, self_at_lags(x, lab, None, S, SELF_MSD, lags), lags)
    with pytest.raises(ValueError, match="species: 2 labels for 5 atoms"):
        c.species_self(0, True, lab[:2])
    with pytest.raises(ValueError, match="weights"):
        c.species_self(0, True, lab, weights=w[:2])
    if backend == "cpu":
        v = ctypes.c_void_p(16)
        assert L.ta_species_self_staged(c._h, 0, 1, S, P(lab), v, v, None) == TA_E_UNSUPPORTED
        assert "CPU backend" in last_error(c)
        assert L.ta_species_self_dev(c._h, v, T, A, D, A * D, 0, 1, S, P(lab), v, v, None) == TA_E_UNSUPPORTED
    c.close()


@pytest.mark.gpu
def test_species_self_dev_and_staged_argument_checks():
    import torch

    T, A, D, S = 40, 7, 3, 2
    x, lab, w = species_walk(T, A, S, seed=8)
    dev = torch.device("cuda", 0)
    d_x, d_w = torch.from_numpy(x.reshape(T, A * D)).to(dev), torch.from_numpy(w).to(dev)
    out = torch.full((S, T), 7.0, dtype=torch.float64, device=dev)
    L = _lib.lib()
    c = _lib.Context(0)
    V = ctypes.c_void_p
    p, pl, pw, po = V(d_x.data_ptr()), _lib._ptr(lab), V(d_w.data_ptr()), V(out.data_ptr())
    assert L.ta_species_self_staged(c._h, 0, 1, S, pl, pw, po, None) == TA_E_STATE  # nothing staged
    assert "not been staged" in last_error(c)
    assert L.ta_species_self_dev(c._h, p, T, A, 4, A * D, 0, 1, S, pl, pw, po, None) == TA_E_INVALID  # dim
    assert L.ta_species_self_dev(c._h, p, T, A, D, A * D - 1, 0, 1, S, pl, pw, po, None) == TA_E_INVALID  # ld_row
    assert L.ta_species_self_dev(c._h, p, 0, A, D, A * D, 0, 1, S, pl, pw, po, None) == TA_E_INVALID  # n_frames
    assert L.ta_species_self_dev(c._h, None, T, A, D, A * D, 0, 1, S, pl, pw, po, None) == TA_E_INVALID
    assert L.ta_species_self_dev(c._h, p, T, A, D, A * D, 0, 1, S, None, pw, po, None) == TA_E_INVALID  # labels
    assert L.ta_species_self_dev(c._h, p, T, A, D, A * D, 0, 1, S, pl, pw, None, None) == TA_E_INVALID  # output
    assert L.ta_species_self_dev(c._h, p, T, A, D, A * D, 2, 1, S, pl, pw, po, None) == TA_E_INVALID  # quantity
    assert L.ta_species_self_dev(c._h, p, T, A, D, A * D, 0, 2, S, pl, pw, po, None) == TA_E_INVALID  # fft
    assert L.ta_species_self_dev(c._h, p, T, A, D, A * D, 0, 1, 9, pl, pw, po, None) == TA_E_INVALID  # n_species
    bad = lab.copy()
    bad[4] = S
    assert L.ta_species_self_dev(c._h, p, T, A, D, A * D, 0, 1, S, _lib._ptr(bad), pw, po, None) == TA_E_INVALID
    assert f"species label {S} of atom 4" in last_error(c)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all(), "a rejected call writes nothing"
    lags = np.arange(T)
    c.species_self_dev(d_x.data_ptr(), T, A, D, A * D, SELF_MSD, 1, S, lab, out.data_ptr(), d_w.data_ptr())
    torch.cuda.synchronize()
    assert_self(out.cpu().numpy(), self_at_lags(x, lab, w, S, SELF_MSD, lags), lags)
    c.species_self_dev(d_x.data_ptr(), T, A, D, A * D, SELF_VACF, 0, S, lab, out.data_ptr())  # unit weights
    torch.cuda.synchronize()
    assert_self(out.cpu().numpy(), self_at_lags(x, lab, None, S, SELF_VACF, lags), lags)
    c.close()


# -------------------------------------------------------------- 6. several devices, distributed
@pytest.mark.gpu
@pytest.mark.parametrize("fft", [True, False])
def test_devices_two_members_one_gpu(fft):
    T, A, S = 400, 11, 3
    x, lab, w = species_walk(T, A, S, seed=8)
    v = species_velocities(T, A, S, seed=8)[0]
    u = ArrayUniverse(positions=x, velocities=v, dimensions=BOX)
    for cls, kw in ((OnsagerHelfand, dict(linear_fit_window=(10, 200))), (OnsagerGreenKubo, {})):
        one = cls(u.atoms, lab, fft=fft, weights=w, self_terms=True, **kw).run()
        two = cls(u.atoms, lab, fft=fft, weights=w, self_terms=True, devices=[0, 0], **kw).run()
        assert two.results.device_ranges == [(0, 5), (5, 11)]
        for s in range(S):
            assert scale_rel_err(two.results.timeseries_self[:, s], one.results.timeseries_self[:, s]) <= 1e-10
        assert np.array_equal(two.results.species_counts, one.results.species_counts)


def _self_worker(rank, world, port, T, A, out_dir):
    import sys

    import torch.distributed as dist

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from current_ref import species_velocities
    from onsager_ref import species_walk
    from transport_analysis_amd import OnsagerGreenKubo, OnsagerHelfand
    from transport_analysis_amd._mini_mda import ArrayUniverse

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    x, lab, w = species_walk(T, A, 2, seed=12)
    v = species_velocities(T, A, 2, seed=12)[0]
    u = ArrayUniverse(positions=x, velocities=v, dimensions=BOX)
    out = {}
    for fft in (True, False):
        o = OnsagerHelfand(u.atoms, lab, fft=fft, weights=w, linear_fit_window=(5, 60), distributed=True, device="cpu",
                           self_terms=True).run()
        g = OnsagerGreenKubo(u.atoms, lab, fft=fft, weights=w, distributed=True, device="cpu", self_terms=True).run()
        out[f"h_{int(fft)}"] = o.results.timeseries_self
        out[f"l_{int(fft)}"] = o.results.onsager_self
        out[f"g_{int(fft)}"] = g.results.timeseries_self
        out["counts"] = o.results.species_counts
        out["c"] = o.results.timeseries
    np.savez(os.path.join(out_dir, f"self_{rank}.npz"), **out)
    dist.destroy_process_group()


@pytest.mark.parametrize("A", [7, 1])
def test_distributed_gloo_world2_cpu_backend(tmp_path, A):
    """A = 7: the ranks hold 3 and 4 atoms of both species; A = 1: one rank holds no atom and contributes zeros."""
    import torch.multiprocessing as mp

    T, world = 90, 2
    port = 39600 + (os.getpid() % 2000) + A
    mp.spawn(_self_worker, args=(world, port, T, A, str(tmp_path)), nprocs=world, join=True)
    x, lab, w = species_walk(T, A, 2, seed=12)
    v = species_velocities(T, A, 2, seed=12)[0]
    u = ArrayUniverse(positions=x, velocities=v, dimensions=BOX)
    for fft in (True, False):
        o = OnsagerHelfand(u.atoms, lab, fft=fft, weights=w, linear_fit_window=(5, 60), device="cpu", self_terms=True).run()
        g = OnsagerGreenKubo(u.atoms, lab, fft=fft, weights=w, device="cpu", self_terms=True).run()
        for r in range(world):
            z = np.load(tmp_path / f"self_{r}.npz")
            assert np.array_equal(z["counts"], o.results.species_counts)
            for s in range(o.n_species):
                assert scale_rel_err(z[f"h_{int(fft)}"][:, s], o.results.timeseries_self[:, s]) <= 1e-10
                assert scale_rel_err(z[f"g_{int(fft)}"][:, s], g.results.timeseries_self[:, s]) <= 1e-10
            np.testing.assert_allclose(z[f"l_{int(fft)}"], o.results.onsager_self, rtol=1e-9,
                                       atol=1e-9 * np.abs(o.results.onsager_self).max())
