"""The intermediate scattering functions (ta_scatter*, IntermediateScattering) on the CPU backend (Context("cpu"),
device="cpu"): closed forms, the long-double reference of scatter_ref, the argument checks and the class."""
import ctypes

import numpy as np
import pytest

import scatter_ref as ref
from transport_analysis_amd import IntermediateScattering, _lib, kvectors_from_box
from transport_analysis_amd._mini_mda import ArrayUniverse
from transport_analysis_amd.scattering import triclinic_vectors

TWO_PI = 2.0 * np.pi


def cpu_context(x, dtype=np.float64):
    T, A, D = x.shape
    c = _lib.Context("cpu")
    (view,) = c.stage_alloc(T, A, D, dtype=dtype)
    view[:] = x
    c.stage_commit(0, T)
    return c


def test_ballistic_closed_form():
    """x = x0 + v t: self[j, tau] = sum_n cos(k_j . v_n tau), whatever the time origin"""
    rng = np.random.default_rng(3)
    T, A, D = 40, 11, 3
    x0, v = rng.uniform(0, 30, (A, D)), rng.normal(scale=0.2, size=(A, D))
    x = x0[None] + v[None] * np.arange(T)[:, None, None]
    k = rng.uniform(-3, 3, (4, D))
    want = np.cos(np.einsum("kd,nd->kn", k, v)[:, None, :] * np.arange(T)[None, :, None]).sum(axis=2)
    c = cpu_context(x)
    try:
        for fft in (0, 1):
            fs, _, _ = c.scatter(fft, k, density=False, collective=False)
            assert np.max(np.abs(fs - want)) <= 1e-10 * A, fft
    finally:
        c.close()


def test_static_lattice():
    """A static cubic lattice (spacing a, n^3 sites): at a reciprocal-lattice vector the density is (N, 0) and coll N^2 at
    every lag; at a commensurate vector of the box that is no lattice vector the density cancels"""
    n, a, T = 4, 2.5, 9
    g = np.arange(n) * a
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + 0.3
    N = n ** 3
    x = np.broadcast_to(sites, (T, N, 3)).copy()
    k = np.array([[TWO_PI / a, 0.0, 0.0], [TWO_PI / a, -2 * TWO_PI / a, TWO_PI / a], [TWO_PI / (n * a), 0.0, 0.0]])
    bar = ref.density_bar(x, k)
    c = cpu_context(x)
    try:
        for fft in (0, 1):
            fs, rho, coll = c.scatter(fft, k)
            phase0 = np.einsum("kd,d->k", k[:2], np.full(3, 0.3))  # the lattice's offset turns the density by k . 0.3
            want = N * np.stack([np.cos(phase0), np.sin(phase0)], axis=1)
            assert np.max(np.abs(rho[:2] - want[:, None, :])) <= bar
            assert np.max(np.abs(coll[:2] - N ** 2)) <= 1e-10 * N ** 2
            assert np.max(np.abs(rho[2])) <= bar and np.max(np.abs(coll[2])) <= 1e-10 * N ** 2
            assert np.max(np.abs(fs - N)) <= 1e-10 * N  # nothing moves
    finally:
        c.close()


@pytest.mark.parametrize("fft", [1, 0])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["stage64", "stage32"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_walks_against_reference(D, dtype, fft):
    for T in (1, 2, 3, 7, 65, 200):
        case = ref.case(T, 13, D, 3)
        c = cpu_context(case[0], dtype)
        try:
            fs, rho, coll = c.scatter(fft, case[1])
            ref.assert_scatter(fs, rho, coll, case, what=f"T={T}")
            only_self = c.scatter(fft, case[1], density=False, collective=False)
            assert only_self[1] is None and only_self[2] is None and np.array_equal(only_self[0], fs)
            only_coll = c.scatter(fft, case[1], self_part=False, density=False)
            assert np.array_equal(only_coll[2], coll)
        finally:
            c.close()


def test_collective_of_a_given_density():
    case = ref.case(65, 13, 3, 3)
    c = cpu_context(case[0])
    other = _lib.Context("cpu")  # nothing staged: none is needed
    try:
        for fft in (0, 1):
            _, rho, coll = c.scatter(fft, case[1])
            assert np.array_equal(other.scatter_collective(rho, fft), coll)
            assert np.array_equal(c.scatter_collective(rho, fft), coll)
        assert c.shape == (65, 13, 3)
    finally:
        c.close()
        other.close()


def test_two_shards_add_up():
    case = ref.case(65, 13, 3, 3)
    x, k = case[0], case[1]
    parts = []
    for lo, hi in ((0, 6), (6, 13)):
        c = cpu_context(x[:, lo:hi])
        try:
            parts.append(c.scatter(1, k, collective=False))
        finally:
            c.close()
    fs, rho = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    c = _lib.Context("cpu")
    try:
        ref.assert_scatter(fs, rho, c.scatter_collective(rho, 1), case, what="two shards")
    finally:
        c.close()


def wrapped_walk():
    """a walk on a 1/64 grid and its image in a constant orthorhombic box (both exact in float32)"""
    rng = np.random.default_rng(5)
    box = np.array([16.0, 12.0, 20.0])
    walk = (np.cumsum(rng.integers(-40, 41, size=(120, 9, 3)), axis=0) + 512) / 64.0
    return walk, walk - np.floor(walk / box) * box, box


def wrapped_positions_need_no_unwrap(**place):
    """the body of test_wrapped_positions_need_no_unwrap under the placement keywords `place` (test_classes_gpu.py runs it
    on the GPU)"""
    walk, wrapped, box = wrapped_walk()
    dims = [*box, 90, 90, 90]
    N = walk.shape[1]
    runs = [IntermediateScattering(ArrayUniverse(positions=p, dimensions=dims).atoms, q=[0.9, 1.6], dq=0.4, max_vectors=5,
                                   **place).run() for p in (walk, wrapped)]
    k = runs[0].results.kvectors
    assert np.array_equal(k, runs[1].results.kvectors) and k.shape[0] >= 6
    m = k * box / TWO_PI
    assert np.max(np.abs(m - np.rint(m))) < 1e-12  # commensurate with the box
    # fs is self / N: the bar is 1e-10 of its scale, 1
    assert np.max(np.abs(runs[0].results.fs_by_kvector - runs[1].results.fs_by_kvector)) <= 1e-10
    assert np.max(np.abs(runs[0].results.density - runs[1].results.density)) <= ref.density_bar(walk, k) + ref.density_bar(wrapped, k)
    # one incommensurate vector: the wrapped series is another function altogether
    bad = np.vstack([k[:2], [[1.0, 0.3, 0.2]]])
    a, b = (IntermediateScattering(ArrayUniverse(positions=p, dimensions=dims).atoms, bad, coherent=False, **place).run()
            for p in (walk, wrapped))
    diff = np.max(np.abs(a.results.fs_by_kvector - b.results.fs_by_kvector), axis=0)
    assert diff[0] <= 1e-10 and diff[1] <= 1e-10 and diff[2] > 1e-3, diff
    assert N == 9
    # ... and unwrap=True on the wrapped positions gives the walk's series for that vector too
    c = IntermediateScattering(ArrayUniverse(positions=wrapped, dimensions=dims).atoms, bad, coherent=False, unwrap=True, **place).run()
    assert np.max(np.abs(a.results.fs_by_kvector - c.results.fs_by_kvector)) <= 1e-10


def test_wrapped_positions_need_no_unwrap():
    wrapped_positions_need_no_unwrap(device="cpu")


def test_kvectors_from_box():
    box = [10.0, 12.0, 14.0, 90, 90, 90]
    k, shell = kvectors_from_box(box, [0.7, 1.3], 0.3, max_vectors=6)
    assert k.shape[1] == 3 and shell.tolist() == sorted(shell.tolist()) and set(shell) == {0, 1}
    assert np.bincount(shell).max() <= 6
    kn = np.linalg.norm(k, axis=1)
    assert np.all(np.abs(kn - np.array([0.7, 1.3])[shell]) <= 0.15 + 1e-12)  # shell membership
    m = np.rint(k * np.array(box[:3]) / TWO_PI)
    assert np.allclose(k, TWO_PI * m / np.array(box[:3]), rtol=0, atol=1e-13)
    keys = {tuple(r) for r in m.astype(int)}
    assert all(tuple(-np.array(r)) not in keys for r in keys)  # one of each +-k pair
    for s in (0, 1):  # sorted by (|m|^2, m lexicographic) within a shell
        ms = m[shell == s].astype(int)
        order = [((r * r).sum(), *r) for r in ms]
        assert order == sorted(order)
    again = kvectors_from_box(box, [0.7, 1.3], 0.3, max_vectors=6)
    assert np.array_equal(again[0], k) and np.array_equal(again[1], shell)  # deterministic
    # without the cap: every lattice vector of the shell, half of the +-k pairs
    full, _ = kvectors_from_box(box, 1.3, 0.3, max_vectors=10 ** 6)
    grid = np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    norms = np.linalg.norm(TWO_PI * grid / np.array(box[:3]), axis=1)
    assert 2 * full.shape[0] == np.count_nonzero(np.abs(norms - 1.3) <= 0.15)
    # planar: the components of dim_type only, m = 0 along the axis left out
    kxy, _ = kvectors_from_box(box, 1.0, 0.4, dim_type="xy")
    assert kxy.shape[1] == 2 and np.all(np.abs(np.linalg.norm(kxy, axis=1) - 1.0) <= 0.2 + 1e-12)
    # triclinic: exp(i k . (x + lattice vector)) = exp(i k . x) for every box vector
    tri = [10.0, 11.0, 12.0, 80.0, 95.0, 100.0]
    kt, st = kvectors_from_box(tri, [0.9], 0.3, max_vectors=8)
    H = triclinic_vectors(tri)
    turns = kt @ H.T / TWO_PI
    assert kt.shape == (8, 3) and np.max(np.abs(turns - np.rint(turns))) < 1e-12
    assert np.all(np.abs(np.linalg.norm(kt, axis=1) - 0.9) <= 0.15 + 1e-12)
    with pytest.raises(ValueError, match="dim_type='xyz'"):
        kvectors_from_box(tri, 0.9, 0.3, dim_type="xy")
    with pytest.raises(ValueError, match="no wavevector"):
        kvectors_from_box(box, 0.05, 0.01)  # below the smallest vector of the box: an empty shell


def test_argument_checks_with_messages():
    L = _lib.lib()
    x = ref.case(7, 13, 3, 3)[0]
    k = np.ascontiguousarray(ref.case(7, 13, 3, 3)[1])
    c = cpu_context(x)
    empty = _lib.Context("cpu")
    out = np.empty((3, 7))
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731

    def fails(code, match, call):
        rc = call()
        assert rc == code, rc
        assert match in L.ta_last_error(c._h).decode() or match in L.ta_last_error(empty._h).decode()

    try:
        with pytest.raises(_lib.TAError, match="outputs are all NULL") as e:
            c.scatter(1, k, self_part=False, density=False, collective=False)
        assert e.value.code == -1
        fails(-1, "wavevectors are NULL", lambda: L.ta_scatter(c._h, 1, 3, None, p(out), None, None))
        bad = k.copy()
        bad[1, 2] = np.inf
        with pytest.raises(_lib.TAError, match="wavevector 1 has a non-finite component"):
            c.scatter(1, bad)
        bad[1, 2] = np.nan
        with pytest.raises(_lib.TAError, match="non-finite"):
            c.scatter(0, bad)
        with pytest.raises(_lib.TAError, match="fft must be 0 or 1") as e:
            c.scatter(2, k)
        assert e.value.code == -1
        fails(-1, "n_k must be 1 ... 4096", lambda: L.ta_scatter(c._h, 1, 0, p(k), p(out), None, None))
        fails(-1, "n_k must be 1 ... 4096", lambda: L.ta_scatter(c._h, 1, 4097, p(k), p(out), None, None))
        with pytest.raises(_lib.TAError, match="slabs have not been staged") as e:
            empty.scatter(1, np.ones((1, 1)))
        assert e.value.code == -4
        rho = np.zeros((3, 7, 2))
        fails(-1, "density or collective output is NULL", lambda: L.ta_scatter_collective(c._h, 1, None, 3, 7, p(out)))
        fails(-1, "fft must be 0 or 1", lambda: L.ta_scatter_collective(c._h, 3, p(rho), 3, 7, p(out)))
        fails(-1, "n_k must be", lambda: L.ta_scatter_collective(c._h, 1, p(rho), 0, 7, p(out)))
        with pytest.raises(ValueError, match="expected \\(n_k, 3\\)"):
            c.scatter(1, np.ones((2, 2)))
        with pytest.raises(_lib.TAError, match="scatter_chunk"):
            c.set_option("scatter_chunk", -1)
        c.set_option("scatter_chunk", 2)
    finally:
        c.close()
        empty.close()


def class_refusals_and_results(**place):
    """the body of test_class_refusals_and_results under the placement keywords `place`"""
    rng = np.random.default_rng(11)
    T, A = 50, 12
    x = np.cumsum(rng.normal(scale=0.2, size=(T, A, 3)), axis=0) + 20
    u = ArrayUniverse(positions=x)  # no box: ts.volume == 0 is accepted with explicit kvectors
    k = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.6, 0.8, 0.0]])
    with pytest.raises(ValueError, match="exactly one of kvectors"):
        IntermediateScattering(u.atoms)
    with pytest.raises(ValueError, match="exactly one of kvectors"):
        IntermediateScattering(u.atoms, k, q=1.0, dq=0.1)
    with pytest.raises(ValueError, match="dq"):
        IntermediateScattering(u.atoms, q=1.0)
    with pytest.raises(TypeError, match="by_particle"):
        IntermediateScattering(u.atoms, k, by_particle=True)
    with pytest.raises(ValueError, match="expected \\(K, 2\\)"):
        IntermediateScattering(u.atoms, k, dim_type="xy")
    with pytest.raises(ValueError, match="needs the periodic box"):
        IntermediateScattering(u.atoms, q=1.0, dq=0.2, **place).run()
    r = IntermediateScattering(u.atoms, k, **place, fft=False).run()
    res = r.results
    x32 = x.astype(np.float32).astype(np.float64)
    lags = ref.lag_sample(T)
    fs, rho, _ = ref.reference(x32, k, lags)
    assert res.kvectors.shape == (3, 3) and res.shell.tolist() == [0, 1, 2] and np.allclose(res.q_shell, 1.0)
    assert res.fs_by_kvector.shape == (T, 3) and res.fs.shape == (T, 3) and res.f.shape == (T, 3)
    assert res.density.shape == (3, T, 2) and res.f_by_kvector.shape == (T, 3) and res.sk.shape == (3,)
    assert np.max(np.abs(res.fs_by_kvector[lags].T * A - fs)) <= 1e-10 * A
    assert np.max(np.abs(res.density - rho)) <= ref.density_bar(x32, k)
    assert np.array_equal(res.sk, res.f[0]) and np.array_equal(res.fs, res.fs_by_kvector)
    assert np.allclose(res.f_by_kvector[0], (res.density ** 2).sum(axis=2).mean(axis=1) / A, rtol=1e-12)
    assert np.array_equal(r.lag_times(), np.arange(T) * 1.0)
    inc = IntermediateScattering(u.atoms, k, **place, coherent=False).run()
    assert inc.results.density is None and inc.results.f is None
    assert np.max(np.abs(inc.results.fs - res.fs)) <= 1e-10
    # shells: the mean over a shell's vectors
    boxed = ArrayUniverse(positions=x, dimensions=[15, 15, 15, 90, 90, 90])
    sh = IntermediateScattering(boxed.atoms, q=[0.5, 0.9], dq=0.2, max_vectors=4, **place).run().results
    for s in (0, 1):
        assert np.allclose(sh.fs[:, s], sh.fs_by_kvector[:, sh.shell == s].mean(axis=1), rtol=0, atol=1e-15)
        assert np.isclose(sh.q_shell[s], np.linalg.norm(sh.kvectors[sh.shell == s], axis=1).mean())
    # molecules: N is the number of compounds
    mol = np.arange(A) // 3
    com = IntermediateScattering(u.atoms, k, **place, compound=mol, compound_weights="geometry", coherent=False).run()
    centres = x32.reshape(T, A // 3, 3, 3).mean(axis=2)
    want = ref.reference(centres, k, lags)[0]
    assert np.max(np.abs(com.results.fs_by_kvector[lags].T * (A // 3) - want)) <= 1e-10 * (A // 3)


def test_class_refusals_and_results():
    class_refusals_and_results(device="cpu")


def test_relaxation_times_of_an_exponential():
    u = ArrayUniverse(positions=np.zeros((30, 2, 3)))
    r = IntermediateScattering(u.atoms, np.eye(3), device="cpu", coherent=False)
    with pytest.raises(RuntimeError, match="must be run"):
        r.relaxation_times()
    r.run()
    t = r.lag_times()
    r.results.fs = np.stack([np.exp(-t / 4.0), np.exp(-t / 100.0), 2 * np.exp(-t / 0.5)], axis=1)
    tau = r.relaxation_times()
    # linear interpolation of an exponential between the two lags around the crossing
    i = 4  # exp(-4 / 4) = 1/e is reached exactly at lag 4
    assert abs(tau[0] - 4.0) < 1e-9 and np.isnan(tau[1]) and 0 < tau[2] < 1
    y0, y1 = np.exp(-3 / 4.0), np.exp(-4 / 4.0)
    half = r.relaxation_times(level=0.4)
    assert np.isclose(half[0], 3 + (0.4 - y0) / (y1 - y0)) and i == 4


# ---- the class on several devices and ranks: devices=[...], distributed=True ------------------------------------------------
PLACED_T = 65
INTEGER_KEYS = ()  # (nothing here is an integer)


def placed_results(A, **place):
    """IntermediateScattering on scatter_ref.case(65, A, 3, 3) with fft True and False under the placement keywords `place`:
    {name: array} (placement.py)"""
    from placement import record_ranges

    x, k = ref.case(PLACED_T, A, 3, 3)[:2]
    u = ArrayUniverse(positions=x)
    out = {}
    for fft in (1, 0):
        r = IntermediateScattering(u.atoms, k, fft=bool(fft), **place).run().results
        out[f"fs_{fft}"], out[f"rho_{fft}"], out[f"f_{fft}"] = r.fs_by_kvector, r.density, r.f_by_kvector
        record_ranges(out, r)
    return out


def check_placed(out, A, what):
    """placed_results against the reference over ALL atoms at test_walks_against_reference's bars (fs and f are self / N
    and coll / N)"""
    case = ref.case(PLACED_T, A, 3, 3)
    for fft in (1, 0):
        ref.assert_scatter(out[f"fs_{fft}"].T * A, out[f"rho_{fft}"], out[f"f_{fft}"].T * A, case, what=f"{what} fft={fft}")


def own_correlations_differ(A, blocks):
    """what a block-wise correlation would give: the sum of the blocks' own collective functions differs from the function
    of the summed density by far more than the bar of 1e-10 -- check_placed can tell the two orders apart"""
    x, k, lags, _, rho, _ = ref.case(PLACED_T, A, 3, 3)
    want = ref.coll_at(rho, lags)
    own = sum(ref.reference(x[:, lo:hi], k, lags)[2] for lo, hi in blocks)
    rel = float(np.max(np.abs(own - want)) / np.max(np.abs(want)))
    print(f"    the blocks' own F(k, t) summed: {rel:.3e} of the scale from the reference")
    assert rel > 1e-3


@pytest.mark.parametrize("A", [13, 1])
def test_class_distributed_two_gloo_ranks_cpu_backend(tmp_path, A):
    """A = 13: the ranks hold 6 and 7 atoms; A = 1: rank 0 holds no atom and contributes zeros (_no_moments).  The self
    parts and the densities are summed over the ranks BEFORE the collective correlation."""
    import sys

    import placement

    placement.check_ranks(sys.modules[__name__], A, 2, "cpu", tmp_path, dict(device="cpu"))
    if A > 1:
        own_correlations_differ(A, [(0, A // 2), (A // 2, A)])
