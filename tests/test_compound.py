"""ta_compound, compound_plan and the compound / compound_weights / reference_frame keywords on the CPU backend (no GPU
needed): the C-ABI against compound_ref's long-double reference within its derived bar, the error returns one per cause,
and the classes against the same classes run on the centres of mass formed in NumPy."""
import ctypes
import functools

import numpy as np
import pytest

from compound_ref import assert_compound, compound_case, compound_ref
from conftest import scale_rel_err
from transport_analysis_amd import (ConductivityGreenKubo, ConductivityHelfand, EinsteinMSD, OnsagerGreenKubo, OnsagerHelfand,
                                    VelocityAutocorr, ViscosityHelfand, _lib)
from transport_analysis_amd._mini_mda import ArrayUniverse
from transport_analysis_amd.compound import compound_plan

INVALID, STATE, UNSUPPORTED = -1, -4, -5
BOX = [4096.0, 4096.0, 4096.0, 90.0, 90.0, 90.0]


def cpu_context(y, dtype=np.float64, n_slabs=1):
    c = _lib.Context("cpu")
    views = c.stage_alloc(y.shape[0], y.shape[1], y.shape[2], n_slabs=n_slabs, dtype=dtype)
    for v in views:
        v[:] = y
    c.stage_commit(0, y.shape[0])
    return c


def raw_compound(c, n, off, mem, w=None, u=None, out=True):
    """ta_compound itself, no checks of the binding in front of it: (status, h_out)"""
    ptr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t).ctypes.data_as(ctypes.c_void_p)
    keep = [ptr(off, np.int64), ptr(mem, np.int32), ptr(w, np.float64), ptr(u, np.float64)]
    h = ctypes.c_void_p()
    rc = _lib.lib().ta_compound(c._h, int(n), *keep, ctypes.byref(h) if out else None)
    return rc, h.value


# (T, A, D, plan, odd compound count): the GPU suite's shapes at a size the host does in a second or two
CPU_CASES = [(1, 200, 3, "mixed", False), (2, 200, 3, "inter", True), (3, 201, 2, "mixed", True), (65, 200, 1, "inter", True),
             (130, 203, 3, "mixed", True), (130, 200, 2, "inter", False), (64, 201, 1, "mixed", False)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["slab64", "slab32"])
@pytest.mark.parametrize("T,A,D,kind,odd", CPU_CASES)
def test_cabi_cpu_against_reference(T, A, D, kind, odd, dtype):
    x, off, mem, w, u, plain, framed = compound_case(T, A, D, kind, odd)
    C = off.size - 1
    for frame, (want, bar) in ((None, plain), (u, framed)):
        c = cpu_context(x, dtype)
        try:
            got = c.compound(off, mem, w, frame)
            assert got.shape == (T, C, D) and got.dtype == np.float64 and c.shape == (T, C, D)
            assert_compound(got, want, bar, f"cpu T={T} A={A} D={D} {kind} frame={'yes' if frame is not None else 'no'}")
            # every compute entry point sees the new slab: ta_msd divides by n_compounds
            ts, bp = c.msd(False, by_particle=True)
            assert bp.shape == (T, C)
            if T > 1:
                assert scale_rel_err(ts, bp.mean(axis=1)) <= 1e-12
        finally:
            c.close()


def test_cabi_cpu_identity_and_unit_weights():
    """every atom its own compound, weights NULL, no frame: the slab bit for bit; power-of-two weights: NumPy's products"""
    x = compound_case(130, 203, 3, "mixed", True)[0]
    A = x.shape[1]
    c = cpu_context(x)
    try:
        assert np.array_equal(c.compound(np.arange(A + 1), np.arange(A)), x)
    finally:
        c.close()
    w = 2.0 ** np.random.default_rng(3).integers(-3, 4, size=A) * np.where(np.arange(A) % 3 == 0, -1.0, 1.0)
    perm = np.random.default_rng(4).permutation(A)
    c = cpu_context(x, np.float32)
    try:
        assert np.array_equal(c.compound(np.arange(A + 1), perm, w), x[:, perm] * w[None, :, None])
    finally:
        c.close()


def test_cabi_errors_one_per_cause():
    x = np.arange(5 * 6 * 3, dtype=np.float64).reshape(5, 6, 3)
    off, mem = np.array([0, 2, 6]), np.arange(6)
    c = _lib.Context("cpu")
    try:
        assert raw_compound(c, 2, off, mem)[0] == STATE  # nothing staged
    finally:
        c.close()
    causes = {
        "null offsets": (2, None, mem),
        "null members": (2, off, None),
        "no compounds": (0, np.array([0]), mem),
        "offsets do not start at 0": (2, np.array([1, 2, 6]), mem),
        "an empty compound": (2, np.array([0, 0, 6]), mem),
        "offsets decrease": (2, np.array([0, 4, 3]), mem),
        "member too large": (2, off, np.array([0, 1, 2, 3, 4, 6])),
        "member negative": (2, off, np.array([0, 1, -1, 3, 4, 5])),
    }
    c = cpu_context(x)
    try:
        for what, (n, o, m) in causes.items():
            assert raw_compound(c, n, o, m)[0] == INVALID, what
            assert c.shape == (5, 6, 3)
            assert _lib.lib().ta_last_error(c._h), what
        # nothing was written by the failed calls: the slab still holds the atoms, and frames can still be staged
        c.stage_commit(0, 5)
        rc, h = raw_compound(c, 2, off, mem, out=False)  # h_out itself may be NULL
        assert rc == 0
        # ... and no longer after it, until the next ta_stage_alloc
        with pytest.raises(_lib.TAError) as e:
            c.stage_commit(0, 5)
        assert e.value.code == STATE
        src = np.zeros((6, 3), dtype=np.float32)
        with pytest.raises(_lib.TAError) as e:
            c.stage_frame(0, 0, _lib.frame_source(src), [0, 1, 2], _lib.atom_rows(np.arange(2)))
        assert e.value.code == STATE
        (view,) = c.stage_alloc(5, 6, 3)
        view[:] = x
        c.stage_commit(0, 5)
        assert np.array_equal(c.compound(off, mem)[:, 0], x[:, 0] + x[:, 1])
    finally:
        c.close()
    c = cpu_context(x, n_slabs=2)  # ViscosityHelfand's pair of slabs
    try:
        assert raw_compound(c, 2, off, mem)[0] == UNSUPPORTED
    finally:
        c.close()


def test_compound_plan():
    labels = np.array([7, 3, 7, 5, 3, 7, 5])
    w = np.array([1.0, 2.0, 3.0, 4.0, 6.0, 4.0, 4.0])
    ids, off, mem, wn = compound_plan(labels, w)
    assert np.array_equal(ids, [3, 5, 7])  # np.unique order
    assert np.array_equal(off, [0, 2, 4, 7])
    assert np.array_equal(mem, [1, 4, 3, 6, 0, 2, 5])  # stable input order within a compound
    assert np.array_equal(wn, [0.25, 0.75, 0.5, 0.5, 0.125, 0.375, 0.5])
    assert np.allclose(np.add.reduceat(wn, off[:-1]), 1.0, rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="weights sum to"):
        compound_plan(labels, np.array([1.0, 2.0, 3.0, 4.0, -2.0, 4.0, 4.0]))  # compound 3: 2 - 2
    with pytest.raises(ValueError):
        compound_plan(labels, w[:-1])


# ---- the classes ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def molecules(T=120, n_mol=20, seed=11):
    """Walks on a 1/64 grid in molecules of three atoms with masses (1, 1, 2) times a power of two: positions, drift and
    the centres of mass are all exact in float32 (what the stand-in trajectory holds), and NumPy's float64 centres of
    mass are exact whatever the order.  -> (x (T, A, 3), labels, masses, com (T, n_mol, 3))"""
    rng = np.random.default_rng(seed)
    A = 3 * n_mol
    x = (np.cumsum(rng.integers(-32, 33, size=(T, A, 3)), axis=0) + rng.integers(0, 4096, size=(1, A, 3)) + 4096) / 64.0
    labels = np.repeat(np.arange(n_mol), 3)[rng.permutation(A)]  # interleaved topology
    m = np.empty(A)
    for c in range(n_mol):
        m[labels == c] = np.array([1.0, 1.0, 2.0]) * 2.0 ** (c % 3)
    wn = m / np.bincount(labels, weights=m)[labels]
    com = np.stack([(x[:, labels == c] * wn[labels == c][None, :, None]).sum(axis=1) for c in range(n_mol)], axis=1)
    assert np.array_equal(com.astype(np.float32), com)
    for a in (x, labels, m, com):
        a.setflags(write=False)
    return x, labels, m, com


@pytest.mark.parametrize("fft", [True, False])
def test_einstein_msd_of_molecules(fft):
    x, labels, m, com = molecules()
    got = EinsteinMSD(ArrayUniverse(positions=x, masses=m), compound=labels, device="cpu", fft=fft).run()
    want = EinsteinMSD(ArrayUniverse(positions=com), device="cpu", fft=fft, stage_dtype=np.float64).run()
    assert got.n_particles == com.shape[1] and np.array_equal(got.results.compound_ids, np.arange(com.shape[1]))
    assert got.results.msds_by_particle.shape == want.results.msds_by_particle.shape
    assert scale_rel_err(got.results.timeseries, want.results.timeseries) <= 1e-10
    assert scale_rel_err(got.results.msds_by_particle, want.results.msds_by_particle) <= 1e-10
    # the atoms' own MSD is something else
    atoms = EinsteinMSD(ArrayUniverse(positions=x, masses=m), device="cpu", fft=fft).run()
    assert scale_rel_err(atoms.results.timeseries, want.results.timeseries) > 0.1
    # equal weights: the geometric centre
    geo = np.stack([x[:, labels == c].sum(axis=1) for c in range(com.shape[1])], axis=1) / 3.0
    got = EinsteinMSD(ArrayUniverse(positions=x, masses=m), compound=labels, compound_weights="geometry", device="cpu", fft=fft).run()
    assert got.n_particles == com.shape[1]
    ref = np.zeros(x.shape[0])
    for k in range(1, x.shape[0]):
        ref[k] = ((geo[k:] - geo[:-k]) ** 2).sum(axis=2).mean()
    assert scale_rel_err(got.results.timeseries, ref) <= 1e-10


@pytest.mark.parametrize("fft", [True, False])
@pytest.mark.parametrize("cls,key", [(OnsagerHelfand, "positions"), (OnsagerGreenKubo, "velocities")])
def test_onsager_of_molecules(cls, key, fft):
    x, labels, m, com = molecules()
    if key == "velocities":  # the same exact numbers, read as velocities (differences stay on the grid)
        x, com = x - x[:1], com - com[:1]
    n_mol = com.shape[1]
    species = np.array(["anion", "cation", "solvent"])[np.arange(n_mol) % 3]
    z = np.array([-1.0, 1.0, 0.5])[np.arange(n_mol) % 3]
    got = cls(ArrayUniverse(**{key: x}, masses=m, dimensions=BOX).atoms, species[labels], compound=labels, weights=z,
              self_terms=True, fft=fft, device="cpu").run()
    want = cls(ArrayUniverse(**{key: com}, dimensions=BOX).atoms, species, weights=z, self_terms=True, fft=fft, device="cpu",
               stage_dtype=np.float64).run()
    assert np.array_equal(got.results.species, want.results.species)
    assert np.array_equal(got.results.species_counts, want.results.species_counts)
    assert got.results.species_counts.sum() == n_mol
    assert scale_rel_err(got.results.timeseries, want.results.timeseries) <= 1e-10
    assert scale_rel_err(got.results.timeseries_self, want.results.timeseries_self) <= 1e-10
    # species given per compound is the same thing
    again = cls(ArrayUniverse(**{key: x}, masses=m, dimensions=BOX).atoms, species, compound=labels, weights=z, self_terms=True,
                fft=fft, device="cpu").run()
    assert np.array_equal(again.results.timeseries, got.results.timeseries)


def test_species_must_be_uniform_within_a_compound():
    x, labels, m, com = molecules()
    species = (np.arange(com.shape[1]) % 2)[labels]
    species[5] += 1
    for cls, key in ((OnsagerHelfand, "positions"), (OnsagerGreenKubo, "velocities")):
        with pytest.raises(ValueError, match="same for all atoms of a compound"):
            cls(ArrayUniverse(**{key: x}, masses=m, dimensions=BOX).atoms, species, compound=labels, device="cpu")
        with pytest.raises(ValueError, match="weights"):  # one value per compound
            cls(ArrayUniverse(**{key: x}, masses=m, dimensions=BOX).atoms, labels % 2, compound=labels, weights=np.ones(x.shape[1]),
                device="cpu")


def test_conductivity_green_kubo_of_molecules():
    """the one-species subclass: per-atom charges (the default) add up within every compound"""
    x, labels, m, com = molecules()
    v, vcom = x - x[:1], com - com[:1]
    q = np.array([-0.5, 0.25, 1.0])[np.arange(x.shape[1]) % 3]
    qmol = np.bincount(labels, weights=q)
    got = ConductivityGreenKubo(ArrayUniverse(velocities=v, masses=m, charges=q, dimensions=BOX).atoms, compound=labels,
                                self_terms=True, device="cpu").run()
    want = ConductivityGreenKubo(ArrayUniverse(velocities=vcom, charges=qmol, dimensions=BOX).atoms, self_terms=True, device="cpu",
                                 stage_dtype=np.float64).run()
    assert np.array_equal(got.charges, qmol)
    assert scale_rel_err(got.results.timeseries, want.results.timeseries) <= 1e-10
    assert scale_rel_err(got.results.timeseries_self, want.results.timeseries_self) <= 1e-10
    assert scale_rel_err(got.results.current, want.results.current) <= 1e-10


@pytest.mark.parametrize("fft", [True, False])
def test_barycentric_frame_removes_a_common_drift(fft):
    x, labels, m, com = molecules()
    T, A, _ = x.shape
    drift = np.cumsum(np.random.default_rng(5).integers(-128, 129, size=(T, 1, 3)), axis=0) / 64.0
    moved = x + drift
    assert np.array_equal(moved.astype(np.float32), moved)  # still exact in the trajectory
    walk_rms = float(np.sqrt(((com[-1] - com[0]) ** 2).sum(axis=1).mean()))
    assert np.abs(drift[-1]).max() > 0 and np.sqrt((drift ** 2).sum(axis=2).max()) > 2 * walk_rms

    def run(pos, **kw):
        return EinsteinMSD(ArrayUniverse(positions=pos, masses=m), compound=labels, device="cpu", fft=fft, **kw).run().results

    lab_frame, lab_moved = run(x), run(moved)
    assert scale_rel_err(lab_moved.timeseries, lab_frame.timeseries) > 0.5  # the drift is in the laboratory-frame MSD
    still, drifting = run(x, reference_frame="barycentric"), run(moved, reference_frame="barycentric")
    scale = float(np.abs(still.timeseries).max())
    # the setup keeps rounding out of the way: the derived per-element bar of ta_compound on the drifted input, propagated
    # into an MSD as 2 sqrt(MSD) delta, is below a tenth of the 1e-10 bar
    ids, off, mem, wn = compound_plan(labels, m)
    delta = float(compound_ref(moved, off, mem, wn, m / m.sum())[1].max())
    print(f"    barycentric: delta {delta:.3e}, 2 sqrt(scale) delta / scale = {2 * np.sqrt(scale) * delta / scale:.3e}")
    assert 2 * np.sqrt(scale) * delta <= 0.1 * 1e-10 * scale
    err = scale_rel_err(drifting.timeseries, still.timeseries)
    print(f"    barycentric: drifted against undrifted {err:.3e}")
    assert err <= 1e-10
    assert scale_rel_err(drifting.msds_by_particle, still.msds_by_particle) <= 1e-10
    # compound=None: every atom its own compound, in the barycentric frame
    a = EinsteinMSD(ArrayUniverse(positions=x, masses=m), reference_frame="barycentric", device="cpu", fft=fft).run()
    b = EinsteinMSD(ArrayUniverse(positions=moved, masses=m), reference_frame="barycentric", device="cpu", fft=fft).run()
    assert a.n_particles == A and scale_rel_err(b.results.timeseries, a.results.timeseries) <= 1e-10


def test_keywords_need_one_device():
    x, labels, m, _ = molecules()
    u = ArrayUniverse(positions=x, velocities=x, masses=m, dimensions=BOX)
    for kw in ({"compound": labels}, {"reference_frame": "barycentric"}, {"compound_weights": "geometry"}):
        for place in ({"devices": [0, 0]}, {"distributed": True}):
            with pytest.raises(ValueError, match="share a shard"):
                EinsteinMSD(u, **kw, **place)
            with pytest.raises(ValueError, match="share a shard"):
                OnsagerHelfand(u.atoms, labels % 2, **kw, **place)
            with pytest.raises(ValueError, match="share a shard"):
                OnsagerGreenKubo(u.atoms, labels % 2, **kw, **place)
    with pytest.raises(ValueError, match="resindices"):
        EinsteinMSD(u, compound="residues", device="cpu")  # the stand-in has no residues
    with pytest.raises(ValueError, match="compound"):
        EinsteinMSD(u, compound="chains", device="cpu")
    with pytest.raises(ValueError, match="reference_frame"):
        EinsteinMSD(u, reference_frame="lab", device="cpu")


def outcome(make):
    try:
        make()
    except Exception as e:  # noqa: BLE001 - the type is what is compared
        return type(e)
    return None


@pytest.mark.parametrize("kw", ["compound", "compound_weights", "reference_frame"])
def test_classes_without_the_keywords_treat_them_as_unknown(kw, monkeypatch):
    """VelocityAutocorr, ViscosityHelfand and ConductivityHelfand do not take them: the keyword reaches AnalysisBase
    untouched, like any unknown keyword (its TypeError under MDAnalysis), while the accepting classes consume it"""
    from transport_analysis_amd import _base

    seen = []
    base_init = _base.AnalysisBase.__init__

    def recording_init(self, *args, **kwargs):
        seen.append(dict(kwargs))
        return base_init(self, *args, **kwargs)

    monkeypatch.setattr(_base.AnalysisBase, "__init__", recording_init)
    x, labels, m, _ = molecules()
    u = ArrayUniverse(positions=x, velocities=x, masses=m, charges=np.ones(x.shape[1]), dimensions=BOX)
    value = {"compound": labels, "compound_weights": "geometry", "reference_frame": "barycentric"}[kw]
    for cls in (VelocityAutocorr, ViscosityHelfand, ConductivityHelfand):
        del seen[:]
        got = outcome(lambda: cls(u.atoms, device="cpu", **{kw: value}))
        assert len(seen) == 1 and seen[0].get(kw) is value, (cls.__name__, seen)  # not consumed on the way
        assert got == outcome(lambda: cls(u.atoms, device="cpu", no_such_keyword=value)), cls.__name__
        assert seen[1].get("no_such_keyword") is value
        if _base.HAVE_MDANALYSIS:
            assert got is TypeError
        assert not cls._accepts_compound
    makers = [lambda **k: EinsteinMSD(u, device="cpu", **k), lambda **k: OnsagerHelfand(u.atoms, labels % 2, device="cpu", **k),
              lambda **k: OnsagerGreenKubo(u.atoms, labels % 2, device="cpu", **k),
              lambda **k: ConductivityGreenKubo(u.atoms, device="cpu", **k)]
    for make in makers:
        del seen[:]
        obj = make(**{kw: value})
        assert type(obj)._accepts_compound and len(seen) == 1 and kw not in seen[0], (type(obj).__name__, seen)


def test_default_compound_weights_ask_for_nothing():
    """compound_weights="mass" is the default: spelled out, it does not trip the one-device rule by itself"""
    x, labels, m, _ = molecules()
    u = ArrayUniverse(positions=x, velocities=x, masses=m, charges=np.ones(x.shape[1]), dimensions=BOX)
    EinsteinMSD(u, compound_weights="mass", distributed=True)
    OnsagerGreenKubo(u.atoms, labels % 2, compound_weights="mass", distributed=True)
    for place in ({"devices": [0, 0]}, {"distributed": True}):
        for kw in ({"compound": labels}, {"reference_frame": "barycentric"}, {"compound": labels, "compound_weights": "mass"}):
            with pytest.raises(ValueError, match="share a shard"):
                ConductivityGreenKubo(u.atoms, **kw, **place)


def test_conductivity_green_kubo_barycentric():
    """the one-species subclass in the barycentric frame: a common drift velocity leaves the current correlation alone"""
    x, labels, m, _ = molecules()
    v = x - x[:1]
    drift = np.cumsum(np.random.default_rng(6).integers(-16, 17, size=(v.shape[0], 1, 3)), axis=0) / 64.0
    q = np.array([-0.5, 0.25, 1.0])[np.arange(v.shape[1]) % 3]

    def run(vel):
        return ConductivityGreenKubo(ArrayUniverse(velocities=vel, masses=m, charges=q, dimensions=BOX).atoms, compound=labels,
                                     reference_frame="barycentric", self_terms=True, device="cpu").run().results

    still, moved = run(v), run(v + drift)
    assert scale_rel_err(moved.timeseries, still.timeseries) <= 1e-10
    assert scale_rel_err(moved.timeseries_self, still.timeseries_self) <= 1e-10
    lab = ConductivityGreenKubo(ArrayUniverse(velocities=v + drift, masses=m, charges=q, dimensions=BOX).atoms, compound=labels,
                                device="cpu").run().results
    assert scale_rel_err(lab.timeseries, still.timeseries) > 1e-3  # the drift is in the laboratory-frame current


def test_one_atom_compounds_in_another_order():
    """As many compounds as atoms, labels unsorted: a value's size does not say whether it is per atom or per compound.
    The group's own charges and a named species attribute are per atom; anything else is refused, not guessed."""
    rng = np.random.default_rng(8)
    T, A = 40, 6
    v = np.cumsum(rng.integers(-8, 9, size=(T, A, 3)), axis=0) / 64.0
    labels = np.array([5, 3, 4, 0, 2, 1])  # compound order (np.unique) = atoms 3, 5, 4, 1, 2, 0
    q = np.array([1.0, -1.0, 0.5, -0.5, 2.0, -2.0])
    u = ArrayUniverse(velocities=v, charges=q, dimensions=BOX)
    got = ConductivityGreenKubo(u.atoms, compound=labels, device="cpu").run()
    assert np.array_equal(got.charges, q[np.argsort(labels)])  # every charge stays on its atom
    want = ConductivityGreenKubo(u.atoms, device="cpu").run()
    assert scale_rel_err(got.results.current, want.results.current) <= 1e-12
    with pytest.raises(ValueError, match="cannot be told apart"):
        ConductivityGreenKubo(u.atoms, charges=q, compound=labels, device="cpu")
    with pytest.raises(ValueError, match="cannot be told apart"):
        OnsagerGreenKubo(u.atoms, np.arange(A) % 2, compound=labels, device="cpu")
    # sorted labels: atoms and compounds coincide, nothing to tell apart
    same = ConductivityGreenKubo(u.atoms, charges=q, compound=np.arange(A), device="cpu").run()
    assert np.array_equal(same.charges, q) and np.array_equal(same.results.timeseries, want.results.timeseries)
    ok = OnsagerGreenKubo(u.atoms, np.arange(A) % 2, compound=np.arange(A), device="cpu").run()
    assert np.array_equal(ok.species_index, np.arange(A) % 2)
