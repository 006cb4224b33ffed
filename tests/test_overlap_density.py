"""The overlap field's density per origin and S_4 (ta_overlap_density*, FourPointStructureFactor) on the CPU backend
(Context("cpu"), device="cpu"): the C-ABI and every error return, closed forms, the long-double reference of
overlap_density_ref (within its bar), shards, threads and the class.  (The one return that needs a slab of 2^31 columns,
n_atoms dim >= 2^31, is not reached here.)  The class tests' bodies take the placement keywords: test_classes_gpu.py calls
them with device=0, and placed_results / check_placed (placement.py) are the class on device groups and across ranks --
here two gloo ranks on the CPU backend, chosen by device="cpu" and by $TA_AMD_DEVICE=cpu."""
import ctypes
import functools
import sys

import numpy as np
import pytest

import overlap_density_ref as ref
import placement
import test_exact_overlap_density as exact_density
from oracle import exact
from test_vanhove import wrapped_walk
from transport_analysis_amd import DynamicSusceptibility, FourPointStructureFactor, _lib, log_lags
from transport_analysis_amd._base import UpdatingAtomGroup
from transport_analysis_amd._mini_mda import ArrayUniverse
from transport_analysis_amd.scattering import kvectors_from_box

LD = np.longdouble
TWO_PI = 6.283185307179586476925


def cpu_context(x, dtype=np.float64):
    T, A, D = x.shape
    c = _lib.Context("cpu")
    (view,) = c.stage_alloc(T, A, D, dtype=dtype)
    view[:] = x
    c.stage_commit(0, T)
    return c


def test_exports_and_tile():
    assert {"ta_overlap_density", "ta_overlap_density_staged", "ta_group_overlap_density", "ta_overlap_density_tile"} <= set(_lib.EXPORTS)
    assert "ta_overlap_density_dev" not in _lib.EXPORTS
    tile = _lib.overlap_density_tile()
    assert tile["SL"] >= 4  # one lag's cutoffs share a launch
    assert tile["SL"] * tile["KC"] * tile["F"] <= 16 and tile["F"] == 2
    assert _lib.lib().ta_abi_version() == 6
    assert FourPointStructureFactor.__name__ in __import__("transport_analysis_amd").__dict__


def test_static_lattice_with_a_reciprocal_wavevector():
    """atoms at rest on the integer lattice, k = 2 pi (1, 0, 2): every phase is a whole number of turns and every atom stays
    inside, so W = N exactly at all lags; S_4 = 0 and the uncentred one is N"""
    g = np.arange(3)
    x0 = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=3).reshape(1, 27, 3).astype(np.float64)
    x = np.broadcast_to(x0, (12, 27, 3)).copy()
    lags = ref.lag_sample(12)
    k = np.array([[1.0, 0.0, 2.0]]) * TWO_PI
    r = FourPointStructureFactor(ArrayUniverse(positions=x).atoms, k, lags, cutoff=(0.25, 1.0), device="cpu").run().results
    W = r.w_by_origin
    assert W.dtype == np.complex128 and W.shape == (1, 2, len(lags), 12)
    for i, tau in enumerate(lags):
        assert np.all(W[:, :, i, :12 - tau] == 27) and not W[:, :, i, 12 - tau:].any()
    ok = r.n_origins >= 2
    assert np.all(r.s4_by_kvector[:, :, ok] == 0.0) and np.all(np.isnan(r.s4_by_kvector[:, :, ~ok]))
    assert np.all(r.s4_uncentred_by_kvector == 27.0)


def test_static_and_ballistic_halves():
    """5 atoms at rest on integers and 4 that move 1/8 per frame along x from integers, k = 2 pi (2, 0, 0): a moving atom's
    phase at frame t is t quarter turns, and it is inside a = 0.5 while tau < 4 -- AT tau = 4 (r2 = 0.25 = a2 exactly) it is not
    counted -- and inside a = 0.7 while tau <= 5.  W[t0] = 5 + [inside] 4 i^t0, exactly"""
    T = 20
    x = np.zeros((T, 9, 3))
    x[:, :, 0] = np.arange(9)[None, :]
    x[:, :, 1] = 3.0 * np.arange(9)[None, :]
    x[:, 5:, 0] += np.arange(T)[:, None] / 8.0
    lags = np.array([0, 1, 3, 4, 5, 6, 10], dtype=np.int64)
    k = np.array([[2.0, 0.0, 0.0]]) * TWO_PI
    unit = np.array([1, 1j, -1, -1j])[np.arange(T) % 4]
    for dtype in (np.float64, np.float32):
        c = cpu_context(x, dtype)
        try:
            W = c.overlap_density(k, lags, (0.5, 0.7))
        finally:
            c.close()
        for i, tau in enumerate(lags):
            n = T - tau
            assert np.array_equal(W[0, 0, i, :n], 5 + 4 * unit[:n] * (tau < 4)), (tau, W[0, 0, i])
            assert np.array_equal(W[0, 1, i, :n], 5 + 4 * unit[:n] * (tau <= 5)), (tau, W[0, 1, i])
            assert not W[:, :, i, n:].any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["stage64", "stage32"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_walks_against_reference(D, dtype):
    for T in (1, 2, 3, 7, 65, 200):
        case = ref.case(T, 13, D)
        x, k, lags = case[:3]
        c = cpu_context(x, dtype)
        try:
            w = c.overlap_density(k, lags, ref.CUTOFFS)
            ref.assert_w(w, case, what=f"T={T} D={D}")
            q = c.overlap(lags, ref.CUTOFFS)
            assert np.array_equal(w[-1].real, q) and not w[-1].imag.any()  # the k = 0 row
            one = c.overlap_density(k[:2], lags, ref.CUTOFFS[2])  # a scalar cutoff: the axis stays
            assert one.shape == (2, 1, len(lags), T) and np.array_equal(one[:, 0], w[:2, 2])
        finally:
            c.close()


def test_reference_cases_are_what_they_are_chosen_for():
    for D in (1, 2, 3):
        x, k, lags, W, Q, bar = ref.case(200, 13, D)
        assert ref.non_trivial(W, Q, k, lags, 13) >= 8
        assert not np.any(k[-1]) and np.all(np.any(k[:-1], axis=1))
        assert np.array_equal(W[-1, ..., 0].astype(np.int64), Q) and not W[-1, ..., 1].any()
        assert 0 < float(bar.max()) < 1e-11  # (no entry is compared with a bar that would hide a wrong atom: terms are O(1))


def test_two_shards_add_up():
    case = ref.case(65, 13, 3)
    x, k, lags = case[:3]
    parts = []
    for lo, hi in ((0, 6), (6, 13)):
        c = cpu_context(x[:, lo:hi])
        try:
            parts.append(c.overlap_density(k, lags, ref.CUTOFFS))
        finally:
            c.close()
    ref.assert_w(parts[0] + parts[1], case, what="two shards", extra_bar=13 * ref.U_R)  # (one more rounding: the add)
    assert np.max(np.abs(parts[0] - (parts[0] + parts[1]))) > 0.5


def test_threads_do_not_change_the_bits():
    case = ref.case(65, 13, 3)
    x, k, lags = case[:3]
    runs = []
    for threads in (1, 4):
        c = cpu_context(x)
        try:
            c.set_option("cpu_threads", threads)
            runs.append(c.overlap_density(k, lags, ref.CUTOFFS))
        finally:
            c.close()
    assert np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64))
    ref.assert_w(runs[0], case, what="threads")


def test_more_wavevectors_than_one_block():
    """33 wavevectors (the CPU backend walks them in blocks of 16): each row equals the one-wavevector call bit for bit"""
    x, _, lags = ref.case(65, 13, 3)[:3]
    k = np.random.default_rng(3).uniform(-6, 6, size=(33, 3))
    c = cpu_context(x)
    try:
        w = c.overlap_density(k, lags, ref.CUTOFFS)
        for j in (0, 15, 16, 31, 32):
            assert np.array_equal(w[j].view(np.uint64), c.overlap_density(k[j:j + 1], lags, ref.CUTOFFS)[0].view(np.uint64)), j
    finally:
        c.close()


def test_argument_checks_with_messages():
    L = _lib.lib()
    x, kv, lags = ref.case(7, 13, 3)[:3]
    lags, kv = np.ascontiguousarray(lags), np.ascontiguousarray(kv[:2])
    cut = np.array([0.5, 0.7])
    c = cpu_context(x)
    empty = _lib.Context("cpu")
    w = np.full((2, 2, len(lags), 7, 2), -7.5)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731

    def fails(code, match, call):
        rc = call()
        assert rc == code, rc
        assert match in L.ta_last_error(c._h).decode() or match in L.ta_last_error(empty._h).decode(), L.ta_last_error(c._h)

    def call(h=None, n_k=2, k=kv, n_lags=len(lags), lg=lags, n_cut=2, cu=cut, out=w):
        return L.ta_overlap_density(h or c._h, n_k, None if k is None else p(k), n_lags, None if lg is None else p(lg), n_cut,
                                    None if cu is None else p(cu), None if out is None else p(out))

    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    try:
        # the order of the header: the wavevectors first, whatever else is wrong
        fails(-1, "overlap_density: wavevectors are NULL", lambda: call(k=None, lg=None, out=None))
        fails(-1, "overlap_density: n_k must be 1 ... 4096", lambda: call(n_k=0, lg=None))
        fails(-1, "overlap_density: n_k must be 1 ... 4096", lambda: call(n_k=4097, lg=None))
        for bad in (np.nan, np.inf, -np.inf):
            kb = kv.copy()
            kb[1, 2] = bad
            fails(-1, "overlap_density: wavevector 1 has a non-finite component", lambda: call(k=kb, lg=None))
        fails(-1, "overlap_density: lags are NULL", lambda: call(lg=None, cu=None))
        fails(-1, "overlap_density: n_lags must be 1 ... 1024", lambda: call(n_lags=0))
        fails(-1, "overlap_density: n_lags must be 1 ... 1024", lambda: call(n_lags=1025))
        fails(-1, "overlap_density: cutoffs are NULL", lambda: call(cu=None, out=None))
        fails(-1, "overlap_density: n_cutoffs must be 1 ... 4", lambda: call(n_cut=0))
        fails(-1, "overlap_density: n_cutoffs must be 1 ... 4", lambda: call(n_cut=5, cu=np.arange(1.0, 6.0)))
        for bad in (np.nan, np.inf, 0.0, -0.5):
            fails(-1, "overlap_density: cutoff 1 must be finite and > 0", lambda: call(cu=np.array([0.5, bad])))
        fails(-1, "overlap_density: the cutoffs must be strictly increasing", lambda: call(cu=np.array([0.5, 0.5])))
        fails(-1, "overlap_density: the cutoffs must be strictly increasing", lambda: call(cu=np.array([0.7, 0.5])))
        fails(-1, "overlap_density: the output is NULL", lambda: call(out=None))
        fails(-1, "overlap_density: lag -1 is outside", lambda: call(n_lags=2, lg=i64(-1, 2)))
        fails(-1, "overlap_density: lag 7 is outside", lambda: call(n_lags=2, lg=i64(1, 7)))
        fails(-1, "overlap_density: the lags must be strictly increasing", lambda: call(n_lags=3, lg=i64(1, 3, 3)))
        fails(-1, "overlap_density: the lags must be strictly increasing", lambda: call(n_lags=3, lg=i64(1, 3, 2)))
        # a rejected call writes nothing
        assert np.all(w == -7.5)
        fails(-4, "slabs have not been staged", lambda: call(h=empty._h))
        assert np.all(w == -7.5)
        assert call() == 0 and not np.any(w == -7.5)
        with pytest.raises(_lib.TAError, match="slabs have not been staged") as e:
            empty.overlap_density(kv, lags, cut)
        assert e.value.code == -4
        with pytest.raises(ValueError, match="kvectors: shape"):
            c.overlap_density(kv[:, :2], lags, cut)
        with pytest.raises(ValueError, match="expected \\(n_lags,\\)"):
            c.overlap_density(kv, np.ones((2, 2), dtype=np.int64), cut)
        with pytest.raises(ValueError, match="cutoffs: shape"):
            c.overlap_density(kv, lags, np.ones((2, 2)))
        with pytest.raises(_lib.TAError, match="overlap_density_chunk"):
            c.set_option("overlap_density_chunk", -1)
        c.set_option("overlap_density_chunk", 2)  # accepted and ignored on the CPU backend
        # k = 0 is a wavevector like any other
        assert not c.overlap_density(np.zeros((1, 3)), lags, cut).imag.any()
    finally:
        c.close()
        empty.close()


def test_output_bound():
    """n_k n_cutoffs n_lags n_frames > 2^26 is refused before anything is written; at the bound's own side the call runs"""
    L = _lib.lib()
    T = 2 ** 15 + 8
    c = cpu_context(np.zeros((T, 1, 1)))
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    try:
        lags = np.arange(256, dtype=np.int64)
        cut = np.array(ref.CUTOFFS)
        k = np.zeros((2, 1))
        w = np.full(8, -7.5)
        assert 2 * 4 * 256 * T > 2 ** 26 >= 2 * 4 * 256 * (T - 8)
        assert L.ta_overlap_density(c._h, 2, p(k), 256, p(lags), 4, p(cut), p(w)) == -1
        msg = L.ta_last_error(c._h).decode()
        assert "exceeds 2^26" in msg and str(2 * 4 * 256 * T) in msg, msg
        assert np.all(w == -7.5)
        got = c.overlap_density(k[:1], lags[:2], cut[:1])
        assert got.shape == (1, 1, 2, T) and np.all(got[0, 0, 0] == 1.0) and got[0, 0, 1, T - 1] == 0.0
    finally:
        c.close()


# ---- the class ---------------------------------------------------------------------------------------------------------
def s4_of(W, lags, n_particles):
    """((K, C, L) S_4, the uncentred one) of long-double parts W (K, C, L, T, 2): the two-pass formula over the valid origins"""
    K, C, L, T = W.shape[:4]
    s4, unc = np.full((K, C, L), np.nan, dtype=LD), np.zeros((K, C, L), dtype=LD)
    for i, tau in enumerate(int(t) for t in lags):
        v = W[:, :, i, :T - tau].astype(LD)
        unc[:, :, i] = (v * v).sum(axis=(2, 3)) / LD(T - tau) / LD(n_particles)
        if T - tau >= 2:
            dev = v - v.mean(axis=2, keepdims=True)
            s4[:, :, i] = (dev * dev).sum(axis=(2, 3)) / LD(T - tau) / LD(n_particles)
    return s4, unc


def rel_err(got, want):
    want = want.astype(np.float64)
    return float(np.max(np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)))


def class_against_reference(**place):
    for D, dim_type in ((3, "xyz"), (2, "xy"), (1, "x")):
        x3 = ref.scatter_ref.walk(200, 13, 3, 1)
        x = x3[:, :, :D]
        lags = ref.lag_sample(200)
        k = ref.wavevectors(5, D)
        W, Q = ref.reference(x, k, lags, ref.CUTOFFS)
        case = (x, k, lags, W, Q, ref.bar(x, k, Q))
        r = FourPointStructureFactor(ArrayUniverse(positions=x3).atoms, k, lags, cutoff=ref.CUTOFFS, dim_type=dim_type,
                                     **place).run().results
        ref.assert_w(r.w_by_origin, case, what=f"class {dim_type}")
        assert np.array_equal(r.lags, lags) and np.array_equal(r.times, lags * 1.0) and np.array_equal(r.cutoffs, ref.CUTOFFS)
        assert np.array_equal(r.n_origins, 200 - lags) and np.array_equal(r.kvectors, k) and np.array_equal(r.shell, np.arange(5))
        assert np.allclose(r.q_shell, np.linalg.norm(k, axis=1), rtol=1e-15)
        assert r.s4_by_kvector.shape == r.s4_uncentred_by_kvector.shape == r.s4.shape == (5, 4, len(lags))
        s4, unc = s4_of(W, lags, 13)
        ok = r.n_origins >= 2
        assert ok.sum() == len(lags) - 1 and np.all(np.isnan(r.s4_by_kvector[:, :, ~ok]))  # lag T - 1: one origin
        err_s, err_u = rel_err(r.s4_by_kvector[:, :, ok], s4[:, :, ok]), rel_err(r.s4_uncentred_by_kvector, unc)
        print(f"    {dim_type}: s4 {err_s:.2e}, uncentred {err_u:.2e} relative")
        assert err_s <= 1e-12 and err_u <= 1e-12
        assert float(s4[:-1][:, :, ok].max()) > 0.1
        # explicit kvectors: each its own shell
        assert np.array_equal(r.s4, r.s4_by_kvector, equal_nan=True) and np.array_equal(r.s4_uncentred, r.s4_uncentred_by_kvector)
        # k = 0: chi_4
        chi = DynamicSusceptibility(ArrayUniverse(positions=x3).atoms, lags, cutoff=ref.CUTOFFS, dim_type=dim_type, **place).run().results
        assert np.array_equal(r.w_by_origin[-1].real, chi.overlap_by_origin) and not r.w_by_origin[-1].imag.any()
        err_c = rel_err(r.s4_by_kvector[-1][:, ok], chi.chi4[:, ok])
        print(f"    {dim_type}: k = 0 against chi4 {err_c:.2e} relative")
        assert err_c <= 1e-12


def test_class_against_reference():
    class_against_reference(device="cpu")


def class_scalar_cutoff_and_default_lags(**place):
    case = ref.case(200, 13, 3)
    x, k = case[:2]
    r = FourPointStructureFactor(ArrayUniverse(positions=x).atoms, k, cutoff=1.5, **place).run().results
    lags = log_lags(200)
    assert np.array_equal(r.lags, lags)
    assert r.w_by_origin.shape == (5, 1, len(lags), 200) and r.s4.shape == (5, 1, len(lags))
    W, Q = ref.reference(x, k, lags, (1.5,))
    ref.assert_w(r.w_by_origin, (x, k, lags, W, Q, ref.bar(x, k, Q)), what="scalar cutoff")


def test_class_scalar_cutoff_and_default_lags():
    class_scalar_cutoff_and_default_lags(device="cpu")


def class_float32_staging_is_the_same(**place):
    case = ref.case(65, 13, 3)
    x, k, lags = case[:3]
    r = FourPointStructureFactor(ArrayUniverse(positions=x.astype(np.float32)).atoms, k, lags, cutoff=ref.CUTOFFS, **place).run().results
    ref.assert_w(r.w_by_origin, case, what="float32 staging")


def test_class_float32_staging_is_the_same():
    class_float32_staging_is_the_same(device="cpu")


def class_box_shells_and_unwrap(**place):
    """q= on the box of a wrapped walk: the shell's vectors are commensurate, so the PHASE does not care about wrapping, but the
    DISPLACEMENT does: unwrap=True on the wrapped walk gives the unwrapped walk's W, and leaving it out does not.  s4 is the
    mean of s4_by_kvector over a shell's vectors."""
    walk, wrapped, box = wrapped_walk()
    dims = [*box, 90, 90, 90]
    lags = ref.lag_sample(120)
    kw = dict(q=(0.55, 0.8), dq=0.3, cutoff=(0.5, 1.5, 4.0), **place)
    a = FourPointStructureFactor(ArrayUniverse(positions=walk, dimensions=dims).atoms, None, lags, **kw).run().results
    b = FourPointStructureFactor(ArrayUniverse(positions=wrapped, dimensions=dims).atoms, None, lags, unwrap=True, **kw).run().results
    w = FourPointStructureFactor(ArrayUniverse(positions=wrapped, dimensions=dims).atoms, None, lags, **kw).run().results
    assert np.array_equal(a.kvectors, b.kvectors) and a.kvectors.shape[0] > 2 and set(a.shell) == {0, 1}
    x, k = walk, a.kvectors
    W, Q = ref.reference(x, k, lags, (0.5, 1.5, 4.0))
    case = (x, k, lags, W, Q, ref.bar(x, k, Q))
    ref.assert_w(a.w_by_origin, case, what="box wavevectors")
    ref.assert_w(b.w_by_origin, case, what="unwrap")
    assert np.max(np.abs(w.w_by_origin - a.w_by_origin)) > 0.5  # (the wrapped series is another walk)
    for s in (0, 1):
        sel = a.shell == s
        assert np.allclose(a.s4[s], a.s4_by_kvector[sel].mean(axis=0), rtol=1e-14, equal_nan=True)
        assert np.allclose(a.s4_uncentred[s], a.s4_uncentred_by_kvector[sel].mean(axis=0), rtol=1e-14)
        assert np.isclose(a.q_shell[s], np.linalg.norm(k[sel], axis=1).mean(), rtol=1e-14)
        assert abs(a.q_shell[s] - kw["q"][s]) <= 0.15
    assert "unwrap=True" in FourPointStructureFactor.__doc__ and "DISPLACEMENT" in FourPointStructureFactor.__doc__


def test_class_box_shells_and_unwrap():
    class_box_shells_and_unwrap(device="cpu")


def compounds_with_dyadic_weights(**place):
    """16 atoms of equal mass in molecules of 4: the weights 1/4 and 1/16 are dyadic, so the centres (and the centres in the
    barycentric frame) stay on a grid and the indicator is exact; N is the number of compounds"""
    x, k, lags = ref.case(65, 16, 3)[:3]
    mol = np.arange(16) // 4
    u = ArrayUniverse(positions=x, masses=np.full(16, 2.0))
    centres = x.reshape(65, 4, 4, 3).mean(axis=2)
    kw = dict(cutoff=ref.CUTOFFS, **place)
    for frame, pos in ((None, centres), ("barycentric", centres - x.mean(axis=1)[:, None, :])):
        extra = {} if frame is None else {"reference_frame": frame}
        r = FourPointStructureFactor(u.atoms, k, lags, compound=mol, **extra, **kw).run().results
        W, Q = ref.reference(pos, k, lags, ref.CUTOFFS)
        ref.assert_w(r.w_by_origin, (pos, k, lags, W, Q, ref.bar(pos, k, Q)), what=f"compound {frame}")
        s4, _ = s4_of(W, lags, 4)
        ok = r.n_origins >= 2
        assert rel_err(r.s4_by_kvector[:, :, ok], s4[:, :, ok]) <= 1e-12  # N is 4


def test_compounds_with_dyadic_weights():
    compounds_with_dyadic_weights(device="cpu")


def test_class_refusals():
    x, k, lags = ref.case(7, 13, 3)[:3]
    u = ArrayUniverse(positions=x)
    with pytest.raises(TypeError, match="by_particle"):
        FourPointStructureFactor(u.atoms, k, lags, cutoff=1.0, by_particle=True)
    with pytest.raises(TypeError, match="UpdatingAtomGroup"):
        FourPointStructureFactor(UpdatingAtomGroup(), k, lags, cutoff=1.0)
    with pytest.raises(TypeError):
        FourPointStructureFactor(u.atoms, k, lags)  # cutoff is required
    with pytest.raises(ValueError, match="exactly one of kvectors"):
        FourPointStructureFactor(u.atoms, None, lags, cutoff=1.0)
    with pytest.raises(ValueError, match="exactly one of kvectors"):
        FourPointStructureFactor(u.atoms, k, lags, cutoff=1.0, q=1.0, dq=0.1)
    with pytest.raises(ValueError, match="needs the shell width dq"):
        FourPointStructureFactor(u.atoms, None, lags, cutoff=1.0, q=1.0)
    with pytest.raises(ValueError, match="kvectors: shape"):
        FourPointStructureFactor(u.atoms, k[:, :2], lags, cutoff=1.0)
    with pytest.raises(ValueError, match="kvectors must be finite"):
        FourPointStructureFactor(u.atoms, np.full_like(k, np.inf), lags, cutoff=1.0)
    for bad in ([], [1.5, 2.0], [2, 1], [1, 1], [-1, 2], [[1, 2]]):
        with pytest.raises(ValueError, match="lags"):
            FourPointStructureFactor(u.atoms, k, bad, cutoff=1.0)
    for bad in ([], [1, 2, 3, 4, 5], 0.0, -1.0, np.nan, np.inf, [2.0, 1.0], [1.0, 1.0], [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="cutoff"):
            FourPointStructureFactor(u.atoms, k, lags, cutoff=bad)
    with pytest.raises(ValueError, match="needs more than the 7 analysed frames"):
        FourPointStructureFactor(u.atoms, k, [1, 7], cutoff=1.0, device="cpu").run()
    with pytest.raises(ValueError, match="at least two analysed frames"):
        FourPointStructureFactor(ArrayUniverse(positions=x[:1]).atoms, k, cutoff=1.0, device="cpu").run()
    with pytest.raises(ValueError, match="needs the periodic box"):
        FourPointStructureFactor(u.atoms, k, lags, cutoff=1.0, unwrap=True, device="cpu").run()
    with pytest.raises(ValueError, match="needs the periodic box"):
        FourPointStructureFactor(u.atoms, None, lags, cutoff=1.0, q=1.0, dq=0.5, device="cpu").run()
    doc = FourPointStructureFactor.__doc__
    assert "ensemble-dependent" in doc and "origins are correlated" in doc
    assert not hasattr(FourPointStructureFactor, "fit") and "No fit" in doc


# ---- the class on several devices and ranks: devices=[...], distributed=True ------------------------------------------------
PLACED_T = 65
INTEGER_KEYS = ("exact_w", "exact_q", "box_shell")
placement.PORTS.setdefault(__name__, 54500)  # (this module's first port, beside the other classes': test_classes_gpu.py too)
EXACT_SEED = 11
BOX_KW = dict(q=(0.55, 0.8), dq=0.3, cutoff=(0.5, 1.5, 4.0))


@functools.lru_cache(maxsize=None)
def placed_case(A):
    """the grid walk of A atoms as overlap_density_ref.case would give it, without that function's 0 < Q_e < N (one atom
    cannot have it): (x, k, lags, W, Q, bar), computed once"""
    x = ref.scatter_ref.walk(PLACED_T, A, 3, 1)
    k, lags = ref.wavevectors(5, 3), ref.lag_sample(PLACED_T)
    assert not np.any(k[-1]) and np.all(np.any(k[:-1], axis=1))
    W, Q = ref.reference(x, k, lags, ref.CUTOFFS)
    return x, k, lags, W, Q, ref.bar(x, k, Q)


@functools.lru_cache(maxsize=None)
def exact_case(A):
    """(x, k, lags, W int64 (K, C, L, T, 2)): integer walks and quarter-turn phases, W a Gaussian integer in every entry"""
    x = exact.int_walk(PLACED_T, A, 3, 1, EXACT_SEED)
    lags = exact_density.LAGS[exact_density.LAGS < PLACED_T]
    W, _, _ = exact_density.exact_w(x, exact_density.QUARTER_Q, lags, exact_density.CUTOFFS)
    return x, exact.quarter_wavevectors(exact_density.QUARTER_Q), lags, W


@functools.lru_cache(maxsize=None)
def box_case():
    """test_vanhove.wrapped_walk()'s nine atoms: (walk, wrapped, dims, k, shell, lags, W, Q, bar) with the shells' vectors
    of the constant box and the reference on the UNWRAPPED walk"""
    walk, wrapped, box = wrapped_walk()
    dims = [*box, 90, 90, 90]
    k, shell = kvectors_from_box(dims, BOX_KW["q"], BOX_KW["dq"])
    m = k * box / TWO_PI  # commensurate: whole numbers of periods along every edge, in both shells
    assert np.allclose(m, np.rint(m), atol=1e-12) and set(shell) == {0, 1} and k.shape[0] > 2
    lags = ref.lag_sample(walk.shape[0])
    W, Q = ref.reference(walk, k, lags, BOX_KW["cutoff"])
    return walk, wrapped, dims, k, shell, lags, W, Q, ref.bar(walk, k, Q)


def placed_results(A, **place):
    """FourPointStructureFactor under the placement keywords `place`: {name: array} (placement.py) of three runs --
    (a) the grid walk of A atoms, (b) the exact integer case of A atoms, with DynamicSusceptibility's Q under the same
    placement, and for A > 1 (c) the nine wrapped atoms with the wavevectors of the box and unwrap=True, and the unwrapped
    ones in per-frame boxes of which only frame 0 is that box (the wavevectors are frame 0's on every rank and member)"""
    from placement import record_ranges

    out = {}
    x, k, lags = placed_case(A)[:3]
    r = FourPointStructureFactor(ArrayUniverse(positions=x).atoms, k, lags, cutoff=ref.CUTOFFS, **place).run().results
    record_ranges(out, r)
    out.update(w=ref.as_parts(r.w_by_origin), s4=r.s4_by_kvector, s4_uncentred=r.s4_uncentred_by_kvector, n_origins=r.n_origins)
    x, k, lags, _ = exact_case(A)
    u = ArrayUniverse(positions=x)
    got = ref.as_parts(FourPointStructureFactor(u.atoms, k, lags, cutoff=exact_density.CUTOFFS, **place).run().results.w_by_origin)
    assert np.array_equal(got, np.rint(got))  # whole numbers, whatever they are: nothing is lost in the int64
    out["exact_w"] = got.astype(np.int64)
    out["exact_q"] = DynamicSusceptibility(u.atoms, lags, cutoff=exact_density.CUTOFFS, **place).run().results.overlap_by_origin
    out["box_shell"] = np.zeros(0, dtype=np.int64)
    if A > 1:
        walk, wrapped, dims, _, _, lags = box_case()[:6]
        r = FourPointStructureFactor(ArrayUniverse(positions=wrapped, dimensions=dims).atoms, None, lags, unwrap=True, **BOX_KW,
                                     **place).run().results
        out.update(box_k=r.kvectors, box_shell=r.shell, box_w=ref.as_parts(r.w_by_origin))
        moving = np.tile(np.array(dims, dtype=np.float64), (len(walk), 1))
        moving[1:, :2] = moving[0, 1::-1]  # (the edges along x and y change places: other vectors, as many per shell)
        r =FourPointStructureFactor(ArrayUniverse(positions=walk, dimensions=moving).atoms, None, lags[:2], **BOX_KW,
                                     **place).run().results
        out.update(first_box_k=r.kvectors, first_box_shell=r.shell)
    return out


def check_placed(out, A, what):
    """placed_results against the references over ALL atoms.  (a) W within overlap_density_ref's bar and A u_r, the one
    re-association of the blocks' sums (test_overlap_density_shapes.py's allowance for a group); S_4 and the uncentred one
    within 1e-12 relative of s4_of(reference W) (test_class_against_reference's bar): the blocks' W are added before
    anything is squared; NaN exactly where a lag has fewer than two origins.  (b) W EQUAL to exact_w's integers, its k = 0
    row DynamicSusceptibility's Q.  (c) the wavevectors and shells those of frame 0's box, W of the wrapped atoms with
    unwrap=True within the bar of the reference on the unwrapped walk."""
    case = placed_case(A)
    lags, W = case[2], case[3]
    ref.assert_w(out["w"], case, what=what, extra_bar=A * ref.U_R)
    s4, unc = s4_of(W, lags, A)
    assert np.array_equal(out["n_origins"], PLACED_T - lags)
    ok = out["n_origins"] >= 2
    assert ok.sum() == len(lags) - 1  # lag T - 1: one origin
    err_s, err_u = rel_err(out["s4"][:, :, ok], s4[:, :, ok]), rel_err(out["s4_uncentred"], unc)
    print(f"    {what}: s4 {err_s:.2e}, uncentred {err_u:.2e} relative")
    assert err_s <= 1e-12 and err_u <= 1e-12
    assert np.array_equal(np.isnan(out["s4"]), np.broadcast_to(~ok, out["s4"].shape)) and not np.isnan(out["s4_uncentred"]).any()
    x, k, lags, W = exact_case(A)
    bad = int(np.count_nonzero(out["exact_w"] != W))
    print(f"    {what}: exact W, {bad} of {W.size} components differ (sum |W| {int(np.abs(W).sum())})")
    assert out["exact_w"].dtype == np.int64 and out["exact_w"].shape == W.shape and bad == 0
    K0 = exact_density.K0
    assert np.array_equal(out["exact_w"][K0, ..., 0], out["exact_q"]) and not out["exact_w"][K0, ..., 1].any()
    assert out["exact_q"].dtype == np.int64 and out["exact_q"][:, 0, :].min() == A  # lag 0: every atom overlaps itself
    if A > 1:
        walk, _, _, k, shell, lags, W, Q, b = box_case()
        for key in ("box_k", "first_box_k"):
            assert np.array_equal(out[key], k), key
        assert np.array_equal(out["box_shell"], shell) and np.array_equal(out["first_box_shell"], shell)
        ref.assert_w(out["box_w"], (walk, k, lags, W, Q, b), what=f"{what} box, unwrap", extra_bar=walk.shape[1] * ref.U_R)
    else:
        assert out["box_shell"].size == 0


@pytest.mark.parametrize("A", [13, 1])
def test_class_distributed_two_gloo_ranks_cpu_backend(tmp_path, A):
    """A = 13: the ranks hold 6 and 7 atoms (and 4 and 5 of the nine wrapped ones); A = 1: rank 0 holds no atom and contributes
    zeros (_no_moments).  W travels through the all-reduce as float64 (..., 2) and is squared only after it: the S_4 of the
    two blocks' own W would not add up to the reference's (k = 0, test_overlap_density_shapes.py's threshold)."""
    placement.check_ranks(sys.modules[__name__], A, 2, "cpu", tmp_path, dict(device="cpu"))
    if A > 1:
        x, k, lags, W = placed_case(A)[:4]
        ok = (PLACED_T - lags) >= 2
        s4, _ = s4_of(W, lags, A)
        halves = [s4_of(ref.reference(x[:, lo:hi], k, lags, ref.CUTOFFS)[0], lags, A)[0] for lo, hi in ((0, A // 2), (A // 2, A))]
        assert float(np.max(np.abs((halves[0] + halves[1])[-1][:, ok] - s4[-1][:, ok]))) > 1e-3  # (what summing variances would give)


def test_class_distributed_with_the_cpu_backend_from_the_environment(tmp_path):
    """the ranks set $TA_AMD_DEVICE=cpu and give no device=: dist.default_device() hands the CPU backend on as
    _lib.device_index does (it used to be int("cpu")).  The same checks as with device="cpu"."""
    placement.check_ranks(sys.modules[__name__], 13, 2, "cpu-env", tmp_path, dict(device="cpu"))


def test_default_device_and_a_cpu_backend_under_nccl(monkeypatch):
    from transport_analysis_amd import dist as tad

    monkeypatch.setenv("TA_AMD_DEVICE", "cpu")
    assert tad.default_device() == _lib.DEVICE_CPU == _lib.device_index(tad.default_device())
    monkeypatch.setattr(tad, "uses_device_reduce", lambda: True)
    with pytest.raises(ValueError, match="selects the CPU backend, but the process group's backend is nccl"):
        tad.default_device()
    with pytest.raises(ValueError, match="selects the CPU backend, but the process group's backend is nccl"):
        tad.check_backend(_lib.DEVICE_CPU, 'device="cpu"')
    monkeypatch.setenv("TA_AMD_DEVICE", "3")
    assert tad.default_device() == 3 == tad.check_backend(3, "device=3")
