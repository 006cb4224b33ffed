"""The partial scattering functions (ta_partial_density*, ta_partial_cross, PartialScattering) on the CPU backend
(Context("cpu"), device="cpu"): the long-double reference of partial_ref, closed forms, the argument checks and the class."""
import ctypes

import numpy as np
import pytest

import partial_ref as ref
import placement
from transport_analysis_amd import IntermediateScattering, PartialScattering, _lib
from transport_analysis_amd._mini_mda import ArrayUniverse

TWO_PI = 2.0 * np.pi
LD = ref.LD


def cpu_context(x, dtype=np.float64):
    T, A, D = x.shape
    c = _lib.Context("cpu")
    (pos,) = c.stage_alloc(T, A, D, dtype=dtype)
    pos[:] = x
    c.stage_commit(0, T)
    return c


def test_symbols():
    names = {"ta_partial_density", "ta_partial_density_staged", "ta_partial_cross", "ta_partial_density_tile",
             "ta_group_partial_density"}
    assert names <= set(_lib.EXPORTS)
    for S, st in ((1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (8, 8)):
        t = _lib.partial_density_tile(S)
        assert t["ST"] == st and t["KC"] >= 1 and t["ST"] * t["KC"] <= 16 and t["F64"] in (1, 2) and t["F32"] == 2
    for S in (0, 9):
        with pytest.raises(_lib.TAError, match="n_species must be 1 ... 8"):
            _lib.partial_density_tile(S)


@pytest.mark.parametrize("fft", [1, 0])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["stage64", "stage32"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_walks_against_reference(D, dtype, fft):
    """symmetry bit for bit and an empty species' exact zeros are part of assert_partial"""
    for T in (1, 2, 3, 65, 200):
        for A, S, empty in ((1, 2, 1), (2, 2, None), (33, 1, None), (33, 3, 1), (33, 8, None)):
            for weighted in (True, False):
                case = ref.case(T, A, D, 3, S, weighted=weighted, empty=empty)
                c = cpu_context(case[0], dtype)
                try:
                    rho, cr = c.partial_density(fft, case[3], case[2], S, case[1])
                    ref.assert_partial(rho, cr, case, what=f"T={T} A={A} S={S} w={weighted}")
                    only = c.partial_density(fft, case[3], case[2], S, case[1], cross=False)
                    assert only[1] is None and np.array_equal(only[0], rho)
                finally:
                    c.close()


def lattice(n, a):
    g = np.arange(n) * a
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def test_static_lattice_with_a_reciprocal_wavevector():
    """Static atoms on a simple-cubic lattice (4^3 sites, spacing 2) and k = 2 pi / 2 x^, a reciprocal vector: every phase
    is a multiple of 2 pi, so rho_a = (sum_{n in a} w_n, 0) within the bar and the cross term W_a W_b at every lag."""
    n, a, T = 4, 2.0, 40
    sites = lattice(n, a)
    N = n ** 3
    k = np.array([[TWO_PI / a, 0.0, 0.0]])
    x = np.broadcast_to(sites, (T, N, 3)).copy()
    lab = ref.labels(N, 3)
    w = ref.weights(N, 3)
    W = np.bincount(lab, weights=w, minlength=3)
    bar = ref.density_bar(x, w, lab, 3, k)
    c = cpu_context(x)
    try:
        for fft in (0, 1):
            rho, cr = c.partial_density(fft, k, lab, 3, w)
            assert np.all(np.max(np.abs(rho[0, :, :, 0] - W[:, None]), axis=1) <= bar)
            assert np.all(np.max(np.abs(rho[0, :, :, 1]), axis=1) <= bar)
            want = W[:, None] * W[None, :]
            scale = np.maximum.outer(W * W, W * W)
            err = np.max(np.abs(cr[0] - want[None]), axis=0)
            print(f"    lattice fft={fft}: {np.max(err / scale):.3e}")
            assert np.all(err <= 1e-10 * scale)
    finally:
        c.close()


def test_two_species_moving_ballistically_in_opposite_directions():
    """Species 0 moves with +v, species 1 with -v along x, all atoms of a species on a line commensurate with k (so their
    phases agree): rho_0 = N_0 e^{i k v t}, rho_1 = N_1 e^{-i k v t} up to a constant phase, hence cross_00 = N_0^2 cos(k v tau),
    cross_11 = N_1^2 cos(k v tau) and cross_01 = N_0 N_1 <cos(k v (2 t + tau) + phi)> over the origins -- compared with the
    defining sum of the exact densities in long double."""
    T, k0, v = 96, 1.25, 3.0 / 64
    N0, N1 = 5, 3
    lam = TWO_PI / k0
    t = np.arange(T)
    x = np.zeros((T, N0 + N1, 3))
    x[:, :N0, 0] = 1.0 + v * t[:, None]
    x[:, N0:, 0] = 2.5 - v * t[:, None]
    x[:, :, 1] = np.arange(N0 + N1) * 0.5  # (k has no y component)
    lab = np.array([0] * N0 + [1] * N1, dtype=np.int32)
    k = np.array([[k0, 0.0, 0.0]])
    ph0, ph1 = LD(k0) * (1.0 + LD(v) * t), LD(k0) * (2.5 - LD(v) * t)
    exact = np.zeros((1, 2, T, 2), dtype=LD)
    exact[0, 0, :, 0], exact[0, 0, :, 1] = N0 * np.cos(ph0), N0 * np.sin(ph0)
    exact[0, 1, :, 0], exact[0, 1, :, 1] = N1 * np.cos(ph1), N1 * np.sin(ph1)
    lags = np.arange(T)
    want = ref.cross_at(exact, lags)
    tau = LD(k0) * LD(v) * lags
    assert np.max(np.abs(want[0, :, 0, 0] - N0 * N0 * np.cos(tau))) < 1e-12 and lam > 0
    assert np.max(np.abs(want[0, :, 1, 1] - N1 * N1 * np.cos(tau))) < 1e-12
    bar = ref.density_bar(x, None, lab, 2, k)
    c = cpu_context(x)
    try:
        for fft in (0, 1):
            rho, cr = c.partial_density(fft, k, lab, 2)
            assert np.all(np.max(np.abs(rho.astype(LD) - exact), axis=(0, 2, 3)) <= bar)
            scale = float(max(N0, N1) ** 2)
            # the returned density differs from the exact one by at most `bar`: that moves a product by about 2 N bar
            err = float(np.max(np.abs(cr[0].astype(LD) - want[0])))
            print(f"    ballistic fft={fft}: {err / scale:.3e}")
            assert err <= 1e-10 * scale + 4 * max(N0, N1) * float(np.max(bar))
    finally:
        c.close()


def test_commensurate_wavevectors_need_no_unwrap():
    rng = np.random.default_rng(5)
    box = np.array([16.0, 12.0, 20.0])
    walk = (np.cumsum(rng.integers(-40, 41, size=(80, 9, 3)), axis=0) + 512) / 64.0
    wrapped = walk - np.floor(walk / box) * box
    m = np.array([[1, 0, 0], [0, 2, 1], [3, 1, 2]])
    k = TWO_PI * m / box
    lab = ref.labels(9, 2)
    bar = ref.density_bar(walk, None, lab, 2, k) + ref.density_bar(wrapped, None, lab, 2, k)
    a, b = cpu_context(walk), cpu_context(wrapped)
    try:
        ra, ca = a.partial_density(1, k, lab, 2)
        rb, cb = b.partial_density(1, k, lab, 2)
        assert np.all(np.max(np.abs(ra - rb), axis=(0, 2, 3)) <= bar)
        d0 = np.einsum("kaa->ka", ca[:, 0])
        assert np.all(np.max(np.abs(ca - cb), axis=1) <= 1e-10 * np.maximum(d0[:, :, None], d0[:, None, :]) + 1e-9)
    finally:
        a.close()
        b.close()


def test_chunks_bit_equal():
    case = ref.case(65, 33, 3, 5, 3)
    c = cpu_context(case[0])
    try:
        runs = []
        for chunk in (1, 2, 0):
            c.set_option("partial_chunk", chunk)
            runs.append(c.partial_density(1, case[3], case[2], 3, case[1]))
        for r in runs[1:]:
            assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1])
        with pytest.raises(_lib.TAError, match="partial_chunk"):
            c.set_option("partial_chunk", -1)
    finally:
        c.close()


def test_cross_of_a_given_density_and_two_shards():
    case = ref.case(65, 33, 3, 3, 3)
    x, w, lab, k = case[:4]
    c = cpu_context(x)
    other = _lib.Context("cpu")  # nothing staged: none is needed
    try:
        for fft in (0, 1):
            rho, cr = c.partial_density(fft, k, lab, 3, w)
            for ctx in (other, c):
                assert np.array_equal(ctx.partial_cross(rho, fft), cr)
        assert c.shape == (65, 33, 3)
        total = 0.0
        for lo, hi in ((0, 16), (16, 33)):
            s = cpu_context(x[:, lo:hi])
            try:
                total = total + s.partial_density(1, k, lab[lo:hi], 3, w[lo:hi], cross=False)[0]
            finally:
                s.close()
        ref.assert_partial(total, other.partial_cross(total, 1), case, what="two shards")
    finally:
        c.close()
        other.close()


def test_error_returns_leave_the_outputs_untouched():
    L = _lib.lib()
    case = ref.case(7, 13, 3, 3, 2)
    k = np.ascontiguousarray(case[3])
    lab = np.ascontiguousarray(case[2])
    c = cpu_context(case[0])
    empty = _lib.Context("cpu")
    rho, cr = np.full((3, 2, 7, 2), -7.0), np.full((3, 7, 2, 2), -7.0)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731

    def fails(ctx, code, match, fft=1, n_k=3, kv=k, S=2, labels=lab, out=rho):
        rc = L.ta_partial_density(ctx._h, fft, n_k, p(kv), S, p(labels), None, p(out), p(cr))
        assert rc == code, (rc, L.ta_last_error(ctx._h).decode())
        assert match in L.ta_last_error(ctx._h).decode(), L.ta_last_error(ctx._h).decode()
        assert np.all(rho == -7.0) and np.all(cr == -7.0)

    try:
        fails(c, -1, "fft must be 0 or 1", fft=2)
        fails(c, -1, "n_species must be 1 ... 8", S=0)
        fails(c, -1, "n_species must be 1 ... 8", S=9)
        fails(c, -1, "wavevectors are NULL", kv=None)
        fails(c, -1, "n_k must be 1 ... 4096", n_k=0)
        fails(c, -1, "n_k must be 1 ... 4096", n_k=4097)
        for value in (np.inf, np.nan):
            bad = k.copy()
            bad[2, 1] = value
            fails(c, -1, "wavevector 2 has a non-finite component", kv=bad)
        fails(c, -1, "species labels are NULL", labels=None)
        fails(c, -1, "partial density output is NULL", out=None)
        fails(empty, -4, "slabs have not been staged")
        for value, text in ((-1, "species label -1 of atom 4"), (2, "species label 2 of atom 4")):
            bad = lab.copy()
            bad[4] = value
            fails(c, -1, text + " is outside 0 ... n_species - 1", labels=bad)
        # ta_partial_cross
        good = np.zeros((3, 2, 7, 2))

        def cross_fails(code, match, fft=1, density=good, n_k=3, S=2, T=7, out=cr):
            rc = L.ta_partial_cross(c._h, fft, p(density), n_k, S, T, p(out))
            assert rc == code and match in L.ta_last_error(c._h).decode(), (rc, L.ta_last_error(c._h).decode())
            assert np.all(cr == -7.0)

        cross_fails(-1, "fft must be 0 or 1", fft=3)
        cross_fails(-1, "n_species must be 1 ... 8", S=9)
        cross_fails(-1, "partial density or cross output is NULL", density=None)
        cross_fails(-1, "partial density or cross output is NULL", out=None)
        cross_fails(-1, "n_k must be", n_k=0)
        cross_fails(-1, "1 <= n_frames", T=0)
        with pytest.raises(ValueError, match="expected \\(n_k, 3\\)"):
            c.partial_density(1, np.ones((2, 2)), lab, 2)
        with pytest.raises(ValueError, match="weights: 5 values for 13 atoms"):
            c.partial_density(1, k, lab, 2, np.ones(5))
        with pytest.raises(ValueError, match="expected \\(n_k, n_species, n_frames, 2\\)"):
            c.partial_cross(np.zeros((3, 7, 2)), 1)
    finally:
        c.close()
        empty.close()


# ---- the class ----------------------------------------------------------------------------------------------------------
def universe(T=50, A=12, box=None, seed=11):
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.normal(scale=0.2, size=(T, A, 3)), axis=0) + 20
    kw = {} if box is None else {"dimensions": box}
    return ArrayUniverse(positions=x, **kw), x


def class_partials_add_up_to_intermediate_scattering(**place):
    """the body of test_class_partials_add_up_to_intermediate_scattering under the placement keywords `place`
    (test_classes_gpu.py runs the class bodies on the GPU)"""
    T, A = 50, 12
    u, x = universe(T, A, box=[15, 15, 15, 90, 90, 90])
    lab = np.array(list("ABBCABBCABBA"))
    for fft in (True, False):
        r = PartialScattering(u.atoms, species=lab, q=[0.5, 0.9], dq=0.2, max_vectors=4, fft=fft, **place).run()
        s = IntermediateScattering(u.atoms, q=[0.5, 0.9], dq=0.2, max_vectors=4, fft=fft, **place).run().results
        res = r.results
        K = res.kvectors.shape[0]
        assert list(res.species) == ["A", "B", "C"] and list(res.species_counts) == [4, 6, 2]
        assert np.array_equal(res.kvectors, s.kvectors) and np.array_equal(res.shell, s.shell) and np.allclose(res.q_shell, s.q_shell)
        assert res.density.shape == (K, 3, T, 2) and res.f_partial_by_kvector.shape == (T, K, 3, 3)
        assert res.f_partial.shape == (T, 2, 3, 3) and res.s_partial.shape == (2, 3, 3)
        assert np.array_equal(res.s_partial, res.f_partial[0])
        assert np.array_equal(res.f_partial, res.f_partial.transpose(0, 1, 3, 2))
        for sh in (0, 1):
            assert np.allclose(res.f_partial[:, sh], res.f_partial_by_kvector[:, res.shell == sh].mean(axis=1), rtol=0, atol=1e-13)
        assert np.max(np.abs(res.f_partial.sum(axis=(2, 3)) - s.f)) <= 1e-10 * np.max(np.abs(s.f[0]))
        assert np.max(np.abs(res.f_partial_by_kvector.sum(axis=(2, 3)) - s.f_by_kvector)) <= 1e-10 * np.max(np.abs(s.f_by_kvector[0]))
        assert np.max(np.abs(r.total() - s.f)) <= 1e-10 * np.max(np.abs(s.f[0]))
        bt_error = "defined for two species"
        with pytest.raises(ValueError, match=bt_error):
            r.bhatia_thornton()


def test_class_partials_add_up_to_intermediate_scattering():
    class_partials_add_up_to_intermediate_scattering(device="cpu")


def class_one_species_is_intermediate_scattering(**place):
    T, A = 50, 12
    u, x = universe(T, A)
    k = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0]])
    x32 = x.astype(np.float32).astype(np.float64)
    r = PartialScattering(u.atoms, k, species=np.zeros(A, dtype=int), **place).run().results
    s = IntermediateScattering(u.atoms, k, **place).run().results
    bar = ref.density_bar(x32, None, np.zeros(A, dtype=np.int32), 1, k)[0]
    assert np.max(np.abs(r.density[:, 0] - s.density)) <= 2 * bar
    assert np.max(np.abs(r.f_partial[:, :, 0, 0] - s.f)) <= 1e-10 * np.max(np.abs(s.f[0]))
    assert np.array_equal(r.shell, np.arange(2))


def test_class_one_species_is_intermediate_scattering():
    class_one_species_is_intermediate_scattering(device="cpu")


def class_total_and_the_normalisations(**place):
    T, A = 50, 12
    u, x = universe(T, A)
    k = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.6, 0.8, 0.0]])
    lab = np.arange(A) % 2
    r = PartialScattering(u.atoms, k, species=lab, fft=False, **place).run()
    res = r.results
    b = np.array([0.5, -2.0])
    lags = ref.lag_sample(T)
    # |sum_a b_a rho_a|^2 correlated: the defining sum of the b-weighted density, in long double
    rho_b = np.einsum("a,kath->kth", b.astype(LD), res.density.astype(LD))[:, None]
    want = ref.cross_at(rho_b, lags)[:, :, 0, 0].T / A  # (lags, K)
    scale = float(np.max(np.abs(b)) ** 2 * np.max(np.einsum("tkaa->tka", res.f_partial_by_kvector)[0]))
    assert np.max(np.abs(r.total(b)[lags] - want)) <= 1e-10 * 4 * scale
    with pytest.raises(ValueError, match="b: 3 values for 2 species"):
        r.total([1.0, 2.0, 3.0])
    bt = r.bhatia_thornton()
    assert set(bt) == {"nn", "nc", "cc"} and np.allclose(bt["nn"], r.total(), rtol=0, atol=1e-13)
    f = res.f_partial
    assert np.allclose(bt["cc"], 0.25 * (f[..., 0, 0] + f[..., 1, 1] - 2 * f[..., 0, 1]), rtol=0, atol=1e-13)  # c_a = 1/2
    assert np.allclose(bt["nc"], 0.5 * (f[..., 0, 0] - f[..., 1, 1]), rtol=0, atol=1e-13)
    z = np.array([1.0, -1.0])
    zz = r.bhatia_thornton(z)["zz"]
    assert np.allclose(zz, 4.0 * bt["cc"], rtol=0, atol=1e-12)  # z = (+1, -1) at c = 1/2: the charge density is 2 N (c - <c>)
    with pytest.raises(ValueError, match="z: 1 values for 2 species"):
        r.bhatia_thornton([1.0])
    al = r.ashcroft_langreth()
    assert np.allclose(al, f * 2.0, rtol=0, atol=1e-13)  # N / sqrt(6 * 6)
    # a species label that no atom carries cannot arise from labels; an empty species comes from index order only: NaN rule
    r.results.species_counts = np.array([12, 0])
    assert np.all(np.isnan(r.ashcroft_langreth()[..., 1, 1]) | np.isinf(r.ashcroft_langreth()[..., 1, 1]))
    fresh = PartialScattering(u.atoms, k, species=lab, **place)
    for call in (fresh.total, fresh.ashcroft_langreth, fresh.bhatia_thornton):
        with pytest.raises(RuntimeError, match="must be run"):
            call()


def test_class_total_and_the_normalisations():
    class_total_and_the_normalisations(device="cpu")


def class_weights_and_attribute_names(**place):
    T, A = 40, 12
    rng = np.random.default_rng(3)
    x = np.cumsum(rng.normal(scale=0.2, size=(T, A, 3)), axis=0) + 20
    types = np.array(["Na", "Cl"] * 6)
    u = ArrayUniverse(positions=x)
    u.atoms.types = types  # species by the name of a per-atom attribute of the group
    k = np.array([[1.0, 0.0, 0.0]])
    w = ref.weights(A, 2)
    r = PartialScattering(u.atoms, k, species="types", weights=w, **place).run().results
    assert list(r.species) == ["Cl", "Na"]
    x32 = x.astype(np.float32).astype(np.float64)
    lab = np.where(types == "Cl", 0, 1).astype(np.int32)
    want = ref.density_of(x32, w, lab, 2, k)
    assert np.all(np.max(np.abs(r.density - want), axis=(0, 2, 3)) <= ref.density_bar(x32, w, lab, 2, k))


def test_class_weights_and_attribute_names():
    class_weights_and_attribute_names(device="cpu")


def test_class_refusals():
    u, _ = universe()
    k = np.eye(3)
    lab = np.arange(12) % 2
    with pytest.raises(TypeError, match="species"):
        PartialScattering(u.atoms, k)
    with pytest.raises(ValueError, match="exactly one of kvectors"):
        PartialScattering(u.atoms, species=lab)
    with pytest.raises(ValueError, match="dq"):
        PartialScattering(u.atoms, species=lab, q=1.0)
    with pytest.raises(TypeError, match="by_particle"):
        PartialScattering(u.atoms, k, species=lab, by_particle=True)
    with pytest.raises(ValueError, match="species: 3 labels for 12 atoms"):
        PartialScattering(u.atoms, k, species=[0, 1, 0])
    with pytest.raises(ValueError, match="9 distinct labels"):
        PartialScattering(u.atoms, k, species=np.arange(12) % 9)
    with pytest.raises(ValueError, match="weights: 3 values for 12 atoms"):
        PartialScattering(u.atoms, k, species=lab, weights=np.ones(3))
    with pytest.raises(ValueError, match="needs the periodic box"):
        PartialScattering(u.atoms, species=lab, q=1.0, dq=0.2, device="cpu").run()


def class_compound_with_per_compound_labels(**place):
    """molecules of three atoms: the partials of their centres of mass, one label per compound, against the class run on the
    centres themselves"""
    T, A = 30, 12
    rng = np.random.default_rng(7)
    x = (np.cumsum(rng.normal(scale=0.2, size=(T, A, 3)), axis=0) + 20).astype(np.float32).astype(np.float64)
    m = rng.uniform(1.0, 16.0, size=A)
    mol = np.arange(A) // 3
    k = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0]])
    lab = np.array([0, 1, 1, 0])
    r = PartialScattering(ArrayUniverse(positions=x, masses=m).atoms, k, species=lab, compound=mol, fft=False, **place).run().results
    wn = m / np.bincount(mol, weights=m)[mol]
    com = np.stack([(x[:, mol == c] * wn[mol == c][None, :, None]).sum(axis=1) for c in range(4)], axis=1)
    assert r.density.shape == (2, 2, T, 2) and list(r.species_counts) == [2, 2]
    want = ref.density_of(com, None, lab.astype(np.int32), 2, k)
    assert np.max(np.abs(r.density - want)) <= 1e-9  # (the centres themselves carry the rounding of their weighted means)
    d0 = ref.cross_at(r.density, [0])[:, 0] / 4.0  # N = 4 compounds
    assert np.max(np.abs(r.f_partial_by_kvector[0] - d0)) <= 1e-10 * np.max(np.abs(d0))


def test_class_compound_with_per_compound_labels():
    class_compound_with_per_compound_labels(device="cpu")


# ---- the class on several ranks: distributed=True -----------------------------------------------------------------------
PLACED_T = 65
INTEGER_KEYS = ()  # (nothing here is an integer)
placement.PORTS.setdefault(__name__, 52000)  # (this module's first port, beside the other classes': test_classes_gpu.py too)


def placed_case(A):
    return ref.case(PLACED_T, A, 3, 3, 3 if A > 1 else 1)


def placed_results(A, **place):
    """PartialScattering on partial_ref's case of A atoms -- interleaved labels and non-uniform weights, so a block that took
    the wrong slice of either shows -- with fft True and False under the placement keywords `place`: {name: array}"""
    from placement import record_ranges

    x, w, lab, k = placed_case(A)[:4]
    u = ArrayUniverse(positions=x)
    out = {}
    for fft in (1, 0):
        r = PartialScattering(u.atoms, k, species=lab, weights=w, fft=bool(fft), **place).run().results
        out[f"rho_{fft}"], out[f"f_{fft}"] = r.density, r.f_partial_by_kvector
        record_ranges(out, r)
    return out


def check_placed(out, A, what):
    """placed_results against the reference over ALL atoms (f_partial_by_kvector is cross / N, (T, K, S, S))"""
    case = placed_case(A)
    for fft in (1, 0):
        ref.assert_partial(out[f"rho_{fft}"], out[f"f_{fft}"].transpose(1, 0, 2, 3) * A, case, what=f"{what} fft={fft}")


@pytest.mark.parametrize("A", [33, 1])
def test_class_distributed_two_gloo_ranks_cpu_backend(tmp_path, A):
    """A = 33: the ranks hold 16 and 17 atoms, each with its own slice of the labels and weights; A = 1: rank 0 holds no atom
    and contributes zeros (_no_moments).  The densities are summed over the ranks BEFORE the cross term (ta_partial_cross)."""
    import sys

    placement.check_ranks(sys.modules[__name__], A, 2, "cpu", tmp_path, dict(device="cpu"))
