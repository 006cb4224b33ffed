"""Where a host-facing call's results lie in the context's output buffer (api.hip's *_out layouts): the segments of the
collective, k-space and van Hove family -- conductivity, Onsager moments / Green-Kubo currents, species self terms,
scattering, orientation, current correlations, partial scattering, the self and distinct van Hove functions, the overlap and
its density -- through every consumer of a layout.  GPU only.

  - the host-facing call against the matching *_staged call, which writes into caller-owned tensors and never sees an
    output buffer: bit for bit, for every non-empty subset of the optional outputs (those that make the library form a
    density or a current of its own included); an output not asked for comes back as None;
  - the five correlators of host sums against the cross / collective segment of the full call: bit for bit;
  - the ten group entries on Group([0]): equal as values to the single context's; on Group([0, 0]): int64 outputs exact,
    float64 outputs within the figure the call's own two-member test uses (named at each case).

One context on device 0 in float64; two slabs of 7 frames x 5 atoms x 3; 2 wavevectors, 2 species, 2 lags, 3 bins, 2
cutoffs: the segments of every call have unequal lengths where the call allows it (14 | 28 | 14, 21 | 7 | 7, 8 | 4), so a
slipped offset does not land on a segment boundary.  Every case is a handful of tiny launches."""
import itertools

import numpy as np
import pytest

import kcurrent_ref
import overlap_density_ref
import partial_ref
import scatter_ref
from conftest import scale_rel_err
from current_ref import currents_ref
from onsager_ref import moments_ref, pair_scale
from oracle import numpy_oracle as orc
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu

T, A, D = 7, 5, 3
K, S, L, B, C = 2, 2, 2, 3, 2
RNG = np.random.default_rng(7)
X = np.cumsum(RNG.normal(scale=0.4, size=(T, A, D)), axis=0) + RNG.uniform(0, 3, size=(1, A, D))  # slab 0
Y = np.cumsum(RNG.normal(scale=0.3, size=(T, A, D)), axis=0) + RNG.uniform(0, 3, size=(1, A, D))  # slab 1
CHARGES = np.array([1.0, -1.0, 2.0, -0.5, 1.5])
LABELS = np.array([0, 1, 1, 0, 1], dtype=np.int32)
WEIGHTS = np.array([0.5, 1.0, 2.0, -1.0, 0.25])
KVECS = np.array([[0.9, 0.0, 0.3], [0.0, 1.3, 0.4]])
LAGS = (1, 3)
DR = 0.5
CUTOFFS = (0.6, 1.2)
INDEX = np.array([[0, 1], [2, 3], [4, 0]])  # three bond vectors
VECTOR_WEIGHTS = np.array([1.0, 2.0, -0.5])
FFT = (1, 0)


def stage(handle):
    """slab 0 = X, slab 1 = Y on a context or, member by member, on a group"""
    slabs = handle.stage_alloc(T, A, D, n_slabs=2, dtype=np.float64)
    for views, data in zip(slabs, (X, Y)):
        if isinstance(handle, _lib.Group):
            for (lo, hi), view in zip(handle.shards, views):
                if view is not None:
                    view[:] = data[:, lo:hi]
        else:
            views[:] = data
    handle.stage_commit(0, T)
    return handle


@pytest.fixture(scope="module")
def ctx():
    c = stage(_lib.Context(0))
    yield c
    c.close()


_on_device = {}


def dev(a):
    """the device pointer of a copy of one of the module's arrays, kept for the module's life (a call reads it after this
    returns)"""
    import torch

    if id(a) not in _on_device:
        _on_device[id(a)] = torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")
    return _on_device[id(a)].data_ptr()


def staged(want, shapes, call):
    """call(pointers) with one sentinel-filled tensor per wanted output (0 for the others), then what it wrote (None for
    one not asked for)"""
    import torch

    outs = [torch.full(shape, -7, dtype=getattr(torch, dt), device="cuda:0") if w else None for w, (shape, dt) in zip(want, shapes)]
    call(*[o.data_ptr() if o is not None else 0 for o in outs])
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() if o is not None else None for o in outs)


def same_bits(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (i, "asked for" if w is not None else "not asked for")
        if w is not None:
            g = np.ascontiguousarray(g)
            assert g.dtype == w.dtype and g.size == w.size, (i, g.dtype, g.shape, w.shape)
            assert np.array_equal(g.reshape(-1).view(np.uint64), w.reshape(-1).view(np.uint64)), (i, g, w)


F, I = "float64", "int64"
# call -> (the outputs that may be left out, the shapes of all outputs, host(c, fft, want), staged(c, fft, want))
CALLS = {
    "conductivity": (
        (1, 2), [((T, D), F), ((T,), F), ((T,), F)],
        lambda c, fft, w: c.conductivity(fft, CHARGES, self_term=w[2], collective=w[1]),
        lambda c, fft, w, sh: staged(w, sh, lambda m, phi, s: c.conductivity_staged(fft, dev(CHARGES), m, phi, s))),
    "onsager": (
        (1,), [((S, T, D), F), ((T, S, S), F)],
        lambda c, fft, w: c.onsager(fft, LABELS, S, WEIGHTS, cross=w[1]),
        lambda c, fft, w, sh: staged(w, sh, lambda m, cr: c.onsager_staged(fft, S, dev(LABELS), m, dev(WEIGHTS), cr))),
    "current": (
        (1,), [((S, T, D), F), ((T, S, S), F)],
        lambda c, fft, w: c.current(fft, LABELS, S, WEIGHTS, cross=w[1]),
        lambda c, fft, w, sh: staged(w, sh, lambda m, cr: c.current_staged(fft, S, dev(LABELS), m, dev(WEIGHTS), cr))),
    "species_self": (
        (), [((S, T), F)],
        lambda c, fft, w: c.species_self(0, fft, LABELS, S, WEIGHTS)[:1],
        lambda c, fft, w, sh: staged(w, sh, lambda o: c.species_self_staged(0, fft, S, LABELS, o, dev(WEIGHTS)))),
    "scatter": (
        (0, 1, 2), [((K, T), F), ((K, T, 2), F), ((K, T), F)],
        lambda c, fft, w: c.scatter(fft, KVECS, self_part=w[0], density=w[1], collective=w[2]),
        lambda c, fft, w, sh: staged(w, sh, lambda s, rho, f: c.scatter_staged(fft, KVECS, s, rho, f))),
    "orient": (
        (0, 1, 2, 3), [((T,), F), ((T,), F), ((T, 3), F), ((T,), F)],
        lambda c, fft, w: c.orient(fft, INDEX, "bond", weights=VECTOR_WEIGHTS, c1=w[0], c2=w[1], total=w[2], collective=w[3]),
        lambda c, fft, w, sh: staged(w, sh, lambda a, b, tot, coll: c.orient_staged(fft, INDEX, "bond", weights=VECTOR_WEIGHTS, d_c1=a,
                                                                                    d_c2=b, d_total=tot, d_coll=coll))),
    "kcurrent": (
        (0, 1, 2), [((K, T, D, 2), F), ((K, T), F), ((K, T), F)],
        lambda c, fft, w: c.kcurrent(fft, KVECS, WEIGHTS, current=w[0], longitudinal=w[1], transverse=w[2]),
        lambda c, fft, w, sh: staged(w, sh, lambda cur, lon, tr: c.kcurrent_staged(fft, KVECS, cur, lon, tr, dev(WEIGHTS)))),
    "partial_density": (
        (1,), [((K, S, T, 2), F), ((K, T, S, S), F)],
        lambda c, fft, w: c.partial_density(fft, KVECS, LABELS, S, WEIGHTS, cross=w[1]),
        lambda c, fft, w, sh: staged(w, sh, lambda rho, cr: c.partial_density_staged(fft, KVECS, S, dev(LABELS), rho, cr,
                                                                                     dev(WEIGHTS)))),
    "vanhove": (
        (0, 1), [((L, B + 1), I), ((L, 2), F)],
        lambda c, fft, w: c.vanhove(LAGS, B, DR, counts=w[0], moments=w[1]),
        lambda c, fft, w, sh: staged(w, sh, lambda cnt, mom: c.vanhove_staged(LAGS, B, DR, cnt, mom))),
    "overlap": (
        (), [((C, L, T), I)],
        lambda c, fft, w: (c.overlap(LAGS, CUTOFFS),),
        lambda c, fft, w, sh: staged(w, sh, lambda q: c.overlap_staged(LAGS, CUTOFFS, q))),
    "overlap_density": (
        (), [((K, C, L, T, 2), F)],
        lambda c, fft, w: (np.ascontiguousarray(c.overlap_density(KVECS, LAGS, CUTOFFS)).view(np.float64),),
        lambda c, fft, w, sh: staged(w, sh, lambda o: c.overlap_density_staged(KVECS, LAGS, CUTOFFS, o))),
    "vanhove_distinct": (
        (), [((L, B + 1), I)],
        lambda c, fft, w: (c.vanhove_distinct(LAGS, B, DR),),
        lambda c, fft, w, sh: staged(w, sh, lambda cnt: c.vanhove_distinct_staged(LAGS, B, DR, cnt))),
}
WITHOUT_FFT = {"vanhove", "overlap", "overlap_density", "vanhove_distinct"}
# scattering, orientation, current correlations and the van Hove function need one output at least; the others always
# return their first
ALL_OPTIONAL = {"scatter", "orient", "kcurrent", "vanhove"}


def subsets(name):
    """every `want` tuple of the call: the outputs that cannot be left out, with each subset of the optional ones (a call all
    of whose outputs are optional: each non-empty subset)"""
    optional, shapes = CALLS[name][:2]
    for r in range(len(optional) + 1):
        for picked in itertools.combinations(optional, r):
            want = tuple(i in picked or i not in optional for i in range(len(shapes)))
            if any(want):
                yield want


CASES = [(name, want) for name in CALLS for want in subsets(name)]


@pytest.mark.parametrize("name,want", CASES, ids=[f"{n}-{''.join(str(int(w)) for w in want)}" for n, want in CASES])
def test_host_call_equals_staged_call(ctx, name, want):
    assert name not in ALL_OPTIONAL or any(want)
    _, shapes, host, on_device = CALLS[name]
    for fft in (FFT[:1] if name in WITHOUT_FFT else FFT):
        reference = on_device(ctx, fft, want, shapes)
        got = host(ctx, fft, want)
        same_bits(got, reference)
        same_bits(host(ctx, fft, want), reference)  # (the output buffer is reused: a second call says the same)


@pytest.mark.parametrize("fft", FFT)
def test_correlators_of_host_sums(ctx, fft):
    """onsager_cross, current_cross, scatter_collective, kcurrent_correlate, partial_cross of the sums a full call returned
    = that call's cross / collective segment, bit for bit"""
    moments, cross = ctx.onsager(fft, LABELS, S, WEIGHTS)
    same_bits((ctx.onsager_cross(moments, fft),), (cross,))
    currents, cross = ctx.current(fft, LABELS, S, WEIGHTS)
    same_bits((ctx.current_cross(currents, fft),), (cross,))
    _, rho, coll = ctx.scatter(fft, KVECS)
    same_bits((ctx.scatter_collective(rho, fft),), (coll,))
    cur, lon, tr = ctx.kcurrent(fft, KVECS, WEIGHTS)
    same_bits(ctx.kcurrent_correlate(cur, KVECS, fft), (lon, tr))
    rho, cross = ctx.partial_density(fft, KVECS, LABELS, S, WEIGHTS)
    same_bits((ctx.partial_cross(rho, fft),), (cross,))


# ---- the ten group entries: what each returns on a handle (a context or a group), and per output the largest difference a
# two-member group may show against the single context -- the figure of the call's own Group([0, 0]) test, named here
def rel(bound):
    """scale_rel_err <= bound (tests/conftest.py)"""
    return lambda got, one: scale_rel_err(got, one) <= bound


def within(bar):
    """|got - one| <= bar, elementwise (bar broadcasts)"""
    return lambda got, one: bool(np.all(np.abs(got - one) <= bar))


exact = np.array_equal


def cross_bound(got, one):
    """tests/test_onsager.py::test_group_onsager_odd_member_slabs, tests/test_greenkubo.py (the group case): 1e-10 of pair_scale"""
    return bool((np.abs(got - one).max(axis=0) <= 1e-10 * pair_scale(one)).all())


def kcurrent_corr_bound(got, one, lon, tr):
    """kcurrent_ref.assert_correlations: 1e-10 of max |long + (D - 1) trans|"""
    return bool(np.max(np.abs(got - one)) <= 1e-10 * np.max(np.abs(lon + (D - 1) * tr)))


def partial_cross_bound(got, one):
    """partial_ref.assert_cross: 1e-10 of max(cross_aa(0), cross_bb(0)) per (wavevector, a, b)"""
    diag0 = np.einsum("kaa->ka", one[:, 0])
    scale = np.maximum(diag0[:, :, None], diag0[:, None, :])
    return bool(np.all(np.abs(got - one).max(axis=1) <= 1e-10 * scale))


def vanhove_moments_bound(got, one):
    """vanhove_ref.assert_vanhove: 1e-10 relative, each entry by its own value"""
    return bool(np.all(np.abs(got - one) <= 1e-10 * np.where(one > 0, one, 1.0)))


def group_calls(fft):
    """name -> (call(handle) -> outputs, per output the check of a two-member group's value against the single context's)"""
    cond_scale = np.max(orc.cond_moment(X, CHARGES)[1])
    mom_scale = moments_ref(X, LABELS, WEIGHTS, S)[1]
    cur_scale = currents_ref(X, LABELS, WEIGHTS, S)[1]
    cur_bar = kcurrent_ref.current_bar(Y, X, WEIGHTS, KVECS)  # (slab 0 holds the velocities of this call, slab 1 the positions)
    rho_bar = partial_ref.density_bar(X, WEIGHTS, LABELS, S, KVECS)
    q = overlap_ref_q()
    w_bar = overlap_density_ref.bar(X, KVECS, q)[None, ..., None] + A * overlap_density_ref.U_R * (q[None, ..., None] > 0)
    return {
        # tests/test_msd_cond_shapes.py::test_group_conductivity_odd_member_slabs: the moment 1e-12 of the scale, Phi and
        # the self term 1e-10 scale-relative
        "conductivity": (lambda h: h.conductivity(fft, CHARGES, self_term=True), [within(1e-12 * cond_scale), rel(1e-10), rel(1e-10)]),
        # tests/test_onsager.py::test_group_onsager_odd_member_slabs and tests/test_greenkubo.py's twin: the sums 1e-12 of
        # their scale, the cross term 1e-10 of pair_scale
        "onsager": (lambda h: h.onsager(fft, LABELS, S, WEIGHTS), [within(1e-12 * mom_scale[:, None, None]), cross_bound]),
        "current": (lambda h: h.current(fft, LABELS, S, WEIGHTS), [within(1e-12 * cur_scale[:, :, None]), cross_bound]),
        # tests/test_species_self_shapes.py (the Group([0, 0]) case): 1e-10 scale-relative, the counts equal
        "species_self": (lambda h: h.species_self(0, fft, LABELS, S, WEIGHTS), [rel(1e-10), exact]),
        # tests/test_scattering_shapes.py (the Group([0, 0]) case), scatter_ref.assert_scatter: the density within
        # density_bar, self and coll 1e-10 of their largest value
        "scatter": (lambda h: h.scatter(fft, KVECS), [rel(1e-10), within(scatter_ref.density_bar(X, KVECS)), rel(1e-10)]),
        "scatter, own density": (lambda h: h.scatter(fft, KVECS, density=False)[::2], [rel(1e-10), rel(1e-10)]),
        # tests/test_current_correlation_shapes.py (the Group([0, 0]) case), kcurrent_ref.assert_kcurrent: the current within
        # current_bar per component, long and trans 1e-10 of max |long + (D - 1) trans|
        "kcurrent": (lambda h: h.kcurrent(fft, KVECS, WEIGHTS), [within(cur_bar[None, None, :, None]), kcurrent_corr_bound, kcurrent_corr_bound]),
        "kcurrent, own current": (lambda h: h.kcurrent(fft, KVECS, WEIGHTS, current=False)[1:], [kcurrent_corr_bound, kcurrent_corr_bound]),
        # tests/test_partial_scattering_shapes.py (the Group([0, 0]) case), partial_ref.assert_partial: the density within
        # density_bar per species, the cross term 1e-10 of max(cross_aa(0), cross_bb(0))
        "partial_density": (lambda h: h.partial_density(fft, KVECS, LABELS, S, WEIGHTS), [within(rho_bar[None, :, None, None]), partial_cross_bound]),
        # tests/test_vanhove_shapes.py (the Group([0, 0]) case), vanhove_ref.assert_vanhove: the counts equal, the moments
        # 1e-10 relative
        "vanhove": (lambda h: h.vanhove(LAGS, B, DR), [exact, vanhove_moments_bound]),
        # tests/test_overlap_shapes.py (the Group([0, 0]) case): equal
        "overlap": (lambda h: (h.overlap(LAGS, CUTOFFS),), [exact]),
        # tests/test_overlap_density_shapes.py (the Group([0, 0]) case), overlap_density_ref.assert_w with extra_bar = A u_r:
        # either component within bar(x, k, Q) + A u_r where Q > 0
        "overlap_density": (lambda h: (np.ascontiguousarray(h.overlap_density(KVECS, LAGS, CUTOFFS)).view(np.float64).reshape(K, C, L, T, 2),),
                            [within(w_bar)]),
    }


def overlap_ref_q():
    """Q (C, L, T) of slab 0, from the definition (ta_overlap): the atoms with |x(t0 + lag) - x(t0)| < a_c"""
    q = np.zeros((C, L, T), dtype=np.int64)
    for i, lag in enumerate(LAGS):
        r = np.linalg.norm(X[lag:] - X[:T - lag], axis=2)  # (T - lag, A)
        for c, a in enumerate(CUTOFFS):
            q[c, i, :T - lag] = (r < a).sum(axis=1)
    return q


def group_check(name, check, got, one, outs):
    if check is kcurrent_corr_bound:
        lon, tr = outs[-2:]
        return check(got, one, lon, tr)
    return check(got, one)


@pytest.mark.parametrize("devices", [[0], [0, 0]], ids=["one-member", "two-members"])
def test_group_entries(ctx, devices):
    g = stage(_lib.Group(devices))
    try:
        for fft in FFT:
            for name, (call, checks) in group_calls(fft).items():
                one, got = call(ctx), call(g)
                assert len(one) == len(got) == len(checks), name
                for i, (a, b, check) in enumerate(zip(got, one, checks)):
                    assert a.dtype == b.dtype and a.shape == b.shape, (name, i)
                    if len(devices) == 1 or a.dtype == np.int64:
                        assert np.array_equal(a, b), (name, i, fft, a, b)
                    else:
                        print(f"    {name}[{i}] fft={fft}: largest difference {float(np.max(np.abs(a - b))):.3e}")
                        assert group_check(name, check, a, b, one), (name, i, fft, float(np.max(np.abs(a - b))))
    finally:
        g.close()
