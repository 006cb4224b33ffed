"""ta_chain_modes on the CPU backend and RouseModes (device="cpu"): chains built from prescribed modes against the closed
form (also wrapped into constant and per-frame triclinic boxes), Parseval's R_g^2, the symmetries, the bit-identities, the
argument checks and the class.  Runs without a GPU."""
import numpy as np
import pytest

import chain_ref as ref
from transport_analysis_amd import RouseModes, _lib
from transport_analysis_amd._mini_mda import ArrayUniverse

LD = np.longdouble
TRIC = np.array([12.0, 13.0, 14.0, 70.0, 80.0, 65.0])


def staged(x, dtype=np.float64):
    T, A, D = x.shape
    c = _lib.Context("cpu")
    (view,) = c.stage_alloc(T, A, D, dtype=dtype)
    view[:] = x
    c.stage_commit(0, T)
    return c


def chain_modes(x, members, coeff, fft=1, dims=None, dtype=np.float64, chunk=None):
    c = staged(np.asarray(x, dtype=np.float64), dtype)
    try:
        if chunk is not None:
            c.set_option("chain_modes_chunk", chunk)
        return c.chain_modes(fft, members, coeff, dimensions=dims)
    finally:
        c.close()


@pytest.fixture(scope="module")
def prescribed():
    """T = 200, 5 chains of N = 16 from all 15 modes: X_p(c, t) = a cos(w t + phi) e with its own a, w, phi, e per chain and
    mode, X_0 drifting.  -> (x (T, 80, 3) unwrapped, members, closed-form acf (15, T), r (T, 5, 16, 3))"""
    T, C, N = 200, 5, 16
    rng = np.random.default_rng(42)
    p = np.arange(1, N)
    a = rng.uniform(0.05, 0.25, size=(C, N - 1))
    w = rng.uniform(0.01, 0.3, size=(C, N - 1))
    phi = rng.uniform(0, 2 * np.pi, size=(C, N - 1))
    e = rng.normal(size=(C, N - 1, 3))
    e /= np.linalg.norm(e, axis=2, keepdims=True)
    t = np.arange(T)
    osc = a[None] * np.cos(w[None] * t[:, None, None] + phi[None])  # (T, C, P)
    X = osc[..., None] * e[None]  # (T, C, P, 3)
    X0 = rng.uniform(3, 9, size=(1, C, 3)) + np.cumsum(rng.normal(scale=0.05, size=(T, C, 3)), axis=0)
    basis = np.cos(p[:, None] * np.pi * (np.arange(1, N + 1)[None, :] - 0.5) / N)  # (P, N)
    r = X0[:, :, None, :] + 2.0 * np.einsum("tcpd,pn->tcnd", X, basis)
    want = np.zeros((N - 1, T))
    for k in range(T):
        want[:, k] = (osc[:T - k] * osc[k:]).sum(axis=(0, 1)) / (T - k)
    members = ref.member_table(C, N, "blocked")
    return ref.place(r, members), members, want, r


def per_frame_box(T):
    d = np.tile(TRIC, (T, 1))
    d[:, :3] *= (1.0 + 0.03 * np.sin(0.4 * np.arange(T)))[:, None]
    return d


def assert_rows(got, want, bar=1e-10, what=""):
    for q in range(want.shape[0]):
        scale = float(np.max(np.abs(want[q])))
        err = float(np.max(np.abs(got[q] - want[q]))) / scale
        print(f"    {what} row {q}: {err:.3e} of {scale:.3e}")
        assert err <= bar, (what, q, err)


@pytest.mark.parametrize("fft", [1, 0])
@pytest.mark.parametrize("box", ["none", "constant", "per-frame"])
def test_prescribed_modes_closed_form(prescribed, box, fft):
    x, members, want, _ = prescribed
    T, N = x.shape[0], members.shape[1]
    dims = None
    if box != "none":
        dims = np.tile(TRIC, (T, 1)) if box == "constant" else per_frame_box(T)
        H = ref.boxes(dims, T)
        widths = np.stack([1.0 / np.linalg.norm(np.linalg.inv(h), axis=0) for h in H])
        r = x[:, members.ravel()].reshape(T, members.shape[0], N, 3)
        longest = float(np.linalg.norm(r[:, :, 1:] - r[:, :, :-1], axis=3).max())
        print(f"    longest bond {longest:.3f}, smallest width {widths.min():.3f}")
        assert longest <= 0.3 * widths.min()  # the sequential step is the minimum image
        x = ref.wrap(x - 6.0, dims)  # (moved to the box's origin corner, so that its faces cut the chains)
        r = x[:, members.ravel()].reshape(T, members.shape[0], N, 3)
        cut = np.abs(r[:, :, 1:] - r[:, :, :-1]).max(axis=3) > 5.0
        assert cut.any() and not cut.all()  # some bonds are cut by a face in some frames
    got = chain_modes(x, members, ref.rouse_coeff(N, np.arange(1, N)), fft=fft, dims=dims)
    assert_rows(got, want, what=f"{box} fft={fft}")


def test_rg2_and_r2_by_parseval(prescribed):
    x, members, _, _ = prescribed
    x32 = x.astype(np.float32).astype(np.float64)  # what the in-memory universe hands out
    T, (C, N) = x.shape[0], members.shape
    r = x32[:, members.ravel()].reshape(T, C, N, 3).astype(LD)
    rg2 = float(((r - r.mean(axis=2, keepdims=True)) ** 2).sum(axis=3).mean())
    r2 = float(((r[:, :, -1] - r[:, :, 0]) ** 2).sum(axis=2).mean())
    res = RouseModes(ArrayUniverse(positions=x32).atoms, members, modes=N - 1, minimum_image=False, device="cpu").run().results
    print(f"    rg2 {res.rg2!r} against {rg2!r}; r2 {res.r2!r} against {r2!r}")
    assert abs(res.rg2 - rg2) <= 1e-10 * rg2
    assert abs(res.r2 - r2) <= 1e-10 * r2
    assert np.array_equal(res.amplitude, res.acf[:, 0]) and np.array_equal(res.modes, np.arange(1, N))
    assert res.end_to_end_acf.shape == (T,) and res.end_to_end_acf[0] == res.r2


@pytest.mark.parametrize("fft", [1, 0])
def test_two_beads_mode_is_an_eighth_of_end_to_end(fft):
    x, members, _, _ = ref.case(150, 4, 2)
    co = np.concatenate([ref.rouse_coeff(2, [1]), ref.end_to_end_row(2)])
    assert abs(co[0, 1] + np.sqrt(2) / 4) < 1e-16  # X_1 = -(sqrt 2 / 4)(r_2 - r_1)
    got = chain_modes(x, members, co, fft=fft)
    assert np.abs(got[0] - got[1] / 8).max() <= 1e-12 * np.abs(got[1] / 8).max()


def test_reversed_translated_drifting_chains_agree(prescribed):
    x, members, _, _ = prescribed
    N = members.shape[1]
    co = np.concatenate([ref.rouse_coeff(N, np.arange(1, N)), ref.end_to_end_row(N)])
    base = chain_modes(x, members, co)
    rev = chain_modes(x, members[:, ::-1].copy(), co)  # X_p -> (-1)^p X_p, R -> -R
    assert_rows(rev, base, what="reversed")
    rng = np.random.default_rng(3)
    moved = x + np.array([3.25, -1.5, 7.0]) + np.cumsum(rng.normal(scale=0.2, size=(x.shape[0], 1, 3)), axis=0)
    assert_rows(chain_modes(moved, members, co), base, what="translated and drifting")


def test_orthorhombic_box_in_a_triclinic_table_gives_the_same_bits():
    """One image path for both box shapes: the frames with the orthorhombic box give the same bits whether the table is
    orthorhombic and constant or per-frame with a triclinic frame in it.  The call returns lag sums only, so in the last frame --
    the triclinic one -- every chain's beads sit in one place: its functionals are exact zeros under any box, and the lag sums
    are those of the orthorhombic frames' blocks."""
    T, C, N = 40, 3, 6
    r = ref.chain_coordinates(T, C, N, seed=4).copy()
    r[-1] = r[-1, :, :1]
    members = ref.member_table(C, N, "permuted")
    ortho = np.tile(np.array(ref.ORTHO), (T, 1))
    x = ref.wrap(ref.place(r, members) + 24.0, ortho)
    co = ref.mixed_coeff(N, 3)
    mixed = ortho.copy()
    mixed[-1] = [30.0, 31.0, 32.0, 80.0, 85.0, 75.0]
    for fft in (1, 0):
        a = chain_modes(x, members, co, fft=fft, dims=ortho)
        b = chain_modes(x, members, co, fft=fft, dims=mixed)
        assert np.array_equal(a, b) and np.abs(a).max() > 0
    # and against the reference with the box, and the unwrapped chains without one
    ref.assert_chain(chain_modes(x, members, co, dims=ortho), ref.reference(x, members, co, ortho), what="ortho")
    ref.assert_chain(chain_modes(x, members, co, dims=ortho), ref.reference(ref.place(r, members), members, co), what="unwrapped")


def test_chunks_and_repeats_give_the_same_bits():
    x, members, co, want = ref.case(130, 5, 7, Q=5)
    for fft in (1, 0):
        runs = [chain_modes(x, members, co, fft=fft, chunk=n) for n in (1, 2, 3, 0, 0)]
        ref.assert_chain(runs[0], want, what=f"fft={fft}")
        assert all(np.array_equal(runs[0], r) for r in runs[1:])
    c = staged(x)
    try:
        with pytest.raises(_lib.TAError, match="chain_modes_chunk"):
            c.set_option("chain_modes_chunk", -1)
    finally:
        c.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T,C,N", [(1, 1, 2), (2, 2, 2), (3, 1, 3), (65, 3, 4), (200, 4, 17)])
def test_walks_against_reference(T, C, N, dtype):
    x, members, co, want = ref.case(T, C, N, Q=3, layout="permuted")
    for fft in (1, 0):
        ref.assert_chain(chain_modes(x, members, co, fft=fft, dtype=dtype), want, what=f"fft={fft}")
    dims = ref.box_frames(ref.TRIC, T, True)
    wrapped = ref.cut_wrapped(x, members, dims, need_cut=T * C * N > 100).astype(dtype).astype(np.float64)  # what the slab holds
    ref.assert_chain(chain_modes(wrapped, members, co, dims=dims, dtype=dtype), ref.reference(wrapped, members, co, dims), what="wrapped")


def test_refusals():
    x, members, co, _ = ref.case(20, 3, 4)
    c = staged(x)
    L = _lib.lib()
    T = 20
    acf = np.empty((co.shape[0], T))
    mem = np.ascontiguousarray(members, dtype=np.int32)
    co = np.ascontiguousarray(co)

    def call(ctx=c, fft=1, C=3, N=4, m=mem, Q=co.shape[0], k=co, dims=None, out=acf):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        rc = L.ta_chain_modes(ctx._h, fft, C, N, p(m), Q, p(k), p(dims), p(out))
        return rc, L.ta_last_error(ctx._h).decode()

    try:
        acf[:] = 7.5
        bad_member, twice, nan = mem.copy(), mem.copy(), co.copy()
        bad_member[1, 2] = x.shape[1]
        twice[2, 3] = twice[2, 0]
        nan[1, 2] = np.inf
        bad_box = np.tile(np.array(ref.TRIC), (T, 1))
        bad_box[5, 0] = -1.0
        for kw, text in ((dict(fft=2), "fft must be 0 or 1"), (dict(C=0), "n_chains must be >= 1"), (dict(N=1), "chain_len must be >= 2"),
                         (dict(Q=0), "n_modes must be >= 1"), (dict(m=None), "member table is NULL"), (dict(k=None), "coefficient matrix is NULL"),
                         (dict(out=None), "acf output is NULL"), (dict(m=bad_member), "member 12 of chain 1 is outside 0 ... n_atoms - 1"),
                         (dict(m=twice), "chain 2 names an atom twice"), (dict(k=nan), "coefficient 2 of mode 1 is not finite"),
                         (dict(dims=bad_box), "chain_modes: ")):
            rc, msg = call(**kw)
            assert rc == -1 and text in msg, (kw.keys(), rc, msg)
        assert np.all(acf == 7.5)  # nothing was written
        rc, msg = call(Q=2**29, C=3)  # n_modes * n_chains * 3 >= 2^31 (found before the coefficients are read)
        assert rc == -1 and "must be below 2^31" in msg, (rc, msg)
        rc, msg = call()
        assert rc == 0, msg
    finally:
        c.close()
    # dim != 3, and nothing staged
    c2 = staged(np.zeros((4, 6, 2)))
    empty = _lib.Context("cpu")
    try:
        rc, msg = call(ctx=c2)
        assert rc == -1 and "three columns per atom (dim = 2)" in msg, (rc, msg)
        rc, msg = call(ctx=empty)
        assert rc == -4 and "have not been staged" in msg, (rc, msg)
    finally:
        c2.close()
        empty.close()


def labelled(u, labels):
    ag = u.atoms
    ag.resindices = np.asarray(labels)
    return ag


def test_class_chains_and_compound_agree():
    T, C, N = 60, 4, 6
    r = ref.chain_coordinates(T, C, N, seed=8)
    members = ref.member_table(C, N, "interleaved")
    x = ref.place(r, members)
    dims = list(ref.TRIC)
    wrapped = ref.cut_wrapped(x, members, np.tile(np.array(dims), (T, 1)))
    u = ArrayUniverse(positions=wrapped, dimensions=dims)
    a = RouseModes(u.atoms, members, device="cpu").run().results
    labels = np.empty(C * N, dtype=np.int64)
    labels[members.ravel()] = np.repeat(np.arange(C), N)  # interleaved chains: the atoms of one label, in group order
    b = RouseModes(labelled(u, labels), compound="residues", device="cpu").run().results
    assert np.array_equal(a.modes, np.arange(1, N)) and a.rg2 is not None
    for key in ("acf", "amplitude", "normalized", "end_to_end_acf"):
        assert np.array_equal(getattr(a, key), getattr(b, key)), key
    assert a.r2 == b.r2 and a.rg2 == b.rg2
    # against the reference of the float32 values the universe hands out, per chain
    w32 = wrapped.astype(np.float32).astype(np.float64)
    co = np.concatenate([ref.rouse_coeff(N, np.arange(1, N)), ref.end_to_end_row(N)])
    lags, want = ref.reference(w32, members, co, np.tile(np.array(dims), (T, 1)))
    ref.assert_chain(np.concatenate([a.acf, a.end_to_end_acf[None]]) * C, (lags, want), what="class")
    # without the image step the wrapped chains are torn
    torn = RouseModes(u.atoms, members, minimum_image=False, device="cpu").run().results
    assert torn.r2 > 2 * a.r2
    # modes: a count, a list, the default; rg2 only for the full set; no end-to-end
    few = RouseModes(u.atoms, members, modes=[3, 1], end_to_end=False, device="cpu").run().results
    assert np.array_equal(few.modes, [3, 1]) and few.rg2 is None and few.end_to_end_acf is None and few.r2 is None
    assert np.array_equal(few.acf, a.acf[[2, 0]])
    assert np.array_equal(RouseModes(u.atoms, members, modes=2, device="cpu").run().results.acf, a.acf[:2])
    long = RouseModes(ArrayUniverse(positions=np.zeros((2, 12, 3))).atoms, np.arange(12)[None], minimum_image=False, device="cpu")
    assert np.array_equal(long.modes, np.arange(1, 9))  # None: 1 ... min(N - 1, 8)
    res = long.run().results  # all beads in one place: zero amplitudes, NaN rows, no warning
    assert not res.amplitude.any() and np.all(np.isnan(res.normalized)) and res.rg2 is None


def test_class_refusals():
    u = ArrayUniverse(positions=np.zeros((3, 10, 3)))
    chains = np.arange(10).reshape(2, 5)
    for kw in (dict(), dict(chains=chains, compound="residues")):
        with pytest.raises(ValueError, match="exactly one of"):
            RouseModes(u.atoms, **kw)
    with pytest.raises(ValueError, match="unequal lengths"):
        RouseModes(labelled(u, [0] * 4 + [1] * 6), compound="residues")
    with pytest.raises(ValueError, match="compound"):
        RouseModes(u.atoms, compound="chains")
    for bad in (0, 5, [1, 1], [0, 1], [5], [], [1.5], True):
        with pytest.raises(ValueError, match="modes"):
            RouseModes(u.atoms, chains, modes=bad)
    for bad in (np.arange(10), np.arange(10).reshape(10, 1), chains.astype(float), chains + 6, np.array([[0, 1, 1]])):
        with pytest.raises(ValueError, match="chains"):
            RouseModes(u.atoms, bad)
    with pytest.raises(ValueError, match="devices"):
        RouseModes(u.atoms, chains, devices=[0, 0])
    with pytest.raises(ValueError, match="distributed"):
        RouseModes(u.atoms, chains, distributed=True)
    with pytest.raises(TypeError, match="by_particle"):
        RouseModes(u.atoms, chains, by_particle=True)
    with pytest.raises(ValueError, match="minimum_image=True"):  # no box in the trajectory
        RouseModes(u.atoms, chains, device="cpu").run()
    with pytest.raises(RuntimeError, match="prior"):
        RouseModes(u.atoms, chains, device="cpu").relaxation_times()


def test_relaxation_times_of_an_exponential_construction():
    """mode p of every chain an AR(1) series with its own decay rate, long enough for the time average to find it"""
    T, C, N = 4000, 40, 4
    rng = np.random.default_rng(5)
    tau = np.array([30.0, 12.0, 5.0])
    X = np.zeros((T, C, N - 1, 3))
    phi = np.exp(-1.0 / tau)[None, :, None]
    X[0] = rng.normal(size=(C, N - 1, 3))
    for t in range(1, T):
        X[t] = phi * X[t - 1] + np.sqrt(1 - phi ** 2) * rng.normal(size=(C, N - 1, 3))
    basis = np.cos(np.arange(1, N)[:, None] * np.pi * (np.arange(1, N + 1)[None, :] - 0.5) / N)
    r = 5.0 + 2.0 * np.einsum("tcpd,pn->tcnd", 0.1 * X, basis)
    members = ref.member_table(C, N, "blocked")
    an = RouseModes(ArrayUniverse(positions=ref.place(r, members)).atoms, members, minimum_image=False, device="cpu").run()
    got, tau_ee = an.relaxation_times()
    print(f"    tau_p {got}, tau_ee {tau_ee}")
    assert np.all(np.abs(got - tau) <= 0.15 * tau)  # (the statistical scatter of 40 chains x 3 axes over 4000 frames)
    assert tau[1] < tau_ee < tau[0]  # odd modes only: dominated by p = 1, pulled down by p = 3
    assert np.all(an.relaxation_times(level=0.5)[0] < got)


def test_symbols_and_abi():
    assert {"ta_chain_modes", "ta_chain_modes_staged", "ta_chain_modes_tile"} <= set(_lib.EXPORTS)
    assert _lib.lib().ta_abi_version() == 6
    tile = _lib.chain_modes_tile()
    assert tile["modes"] >= 1 and tile["frames"] >= 2 and tile["frames"] % 2 == 0
