"""ta_overlap_density on inputs whose result is an exact Gaussian integer, on both backends (the GPU part marked gpu).

Inputs: oracle.exact.int_walk(T, A, D, 1, seed) -- integer positions, steps in {-1, 0, 1} per column --, the cutoffs (1.5, 2.0,
3.0, 4.5) and oracle.exact.quarter_wavevectors of the turns QUARTER_Q cut to D columns (k = 0 among them).  Every squared
displacement is an integer, so the indicator is exact and 2.0 and 3.0 sit ON attainable values (r2 = 4, 9: the strict side
decides those pairs); every phase is a whole number of quarter turns, so (cos, sin) is one of (1, 0), (0, 1), (-1, 0), (0, -1)
and W = sum_inside quarter_cs is a Gaussian integer that float64 sums reproduce in any order.  Asserted, every entry:

  * W is BIT-EQUAL to those integers on float64 and float32 stagings / slabs, zeros (+0.0) at t0 >= T - lag;
  * the k = 0 row equals ta_overlap's Q and has zero imaginary part;
  * a two-member group with an odd split gives the same bits (GPU);
  * every "overlap_density_chunk" gives the same bits (GPU).

The module asserts what the case is chosen for rather than assuming it (T = 100, A = 301, D = 3, seed 3: hundreds of pairs
exactly on the cutoffs 2.0 and 3.0 at lags 2 and 7, Q varying over the origins at every lag from 1 to 63, W varying over
the origins for all four non-zero wavevectors)."""
import functools

import numpy as np
import pytest

from oracle import exact
from transport_analysis_amd import _lib

CUTOFFS = (1.5, 2.0, 3.0, 4.5)
QUARTER_Q = np.array([[.25, 0, 0], [.5, .25, -.75], [0, 0, 0], [1.25, -.5, .25], [0, 0, .5]])
K0 = 2  # the k = 0 row
LAGS = np.array([0, 1, 2, 7, 31, 63, 64, 98, 99], dtype=np.int64)
# (T, A, D, seed)
MAIN = (100, 301, 3, 3)
CASES = [MAIN, (65, 40, 2, 4), (67, 33, 1, 5), (3, 2, 3, 6), (1, 1, 3, 7)]


def exact_w(x, q, lags, cutoffs):
    """(W (K, C, L, T, 2) int64, Q (C, L, T) int64, pairs exactly on a cutoff (C, L))"""
    T = x.shape[0]
    xi = x.astype(np.int64)
    c, s = exact.quarter_cs(x, q)  # (K, T, A)
    a2 = np.array([a * a for a in cutoffs])
    W = np.zeros((len(q), len(a2), len(lags), T, 2), dtype=np.int64)
    Q = np.zeros((len(a2), len(lags), T), dtype=np.int64)
    on = np.zeros((len(a2), len(lags)), dtype=np.int64)
    for i, tau in enumerate(int(t) for t in lags):
        d = xi[tau:] - xi[:T - tau]
        r2 = (d * d).sum(axis=2).astype(np.float64)
        for ci, e in enumerate(a2):
            inside = (r2 < e).astype(np.int64)
            Q[ci, i, :T - tau] = inside.sum(axis=1)
            on[ci, i] = int((r2 == e).sum())
            W[:, ci, i, :T - tau, 0] = np.einsum("ktn,tn->kt", c[:, :T - tau], inside)
            W[:, ci, i, :T - tau, 1] = np.einsum("ktn,tn->kt", s[:, :T - tau], inside)
    return W, Q, on


@functools.lru_cache(maxsize=None)
def case(T, A, D, seed):
    """(x, k, lags, W, Q): computed once and shared; not to be modified"""
    x = exact.int_walk(T, A, D, 1, seed)
    q = np.ascontiguousarray(QUARTER_Q[:, :D])
    k = exact.quarter_wavevectors(q)
    lags = LAGS[LAGS < T]
    W, Q, on = exact_w(x, q, lags, CUTOFFS)
    if (T, A, D, seed) == MAIN:
        for ci in (1, 2):  # cutoffs 2.0 and 3.0
            for li in (2, 3):  # lags 2 and 7
                assert on[ci, li] >= 100, ("too few pairs exactly on the cutoff", CUTOFFS[ci], int(lags[li]), int(on[ci, li]))
        _, Q63, _ = exact_w(x, q[:1], np.arange(1, 64), CUTOFFS)
        for l in range(63):
            v = Q63[:, l, :T - 1 - l]
            assert np.any(v.max(axis=1) > v.min(axis=1)), ("Q does not vary over the origins at lag", l + 1)
        for j in range(len(q)):
            if j != K0 and np.any(q[j]):
                v = W[j, :, 1, :T - 1]
                assert np.any(v.max(axis=1) > v.min(axis=1)), ("W does not vary over the origins for wavevector", j)
        assert sum(bool(np.any(r)) for r in q) == 4
    for a in (x, k, lags, W, Q):
        a.setflags(write=False)
    return x, k, lags, W, Q


def parts(w):
    return np.ascontiguousarray(w).view(np.float64).reshape(w.shape + (2,))


def assert_exact(w, W, lags, what):
    """complex128 (K, C, L, T) from a host-facing call, or float64 parts, against the integers: bit-equal, +0.0 past the
    last origin"""
    got = parts(w) if np.iscomplexobj(w) else np.asarray(w)
    assert got.dtype == np.float64 and got.shape == W.shape, (what, got.dtype, got.shape, W.shape)
    bad = int(np.count_nonzero(got != W))
    print(f"    {what}: {bad} of {W.size} components differ (sum |W| {int(np.abs(W).sum())})")
    assert bad == 0, (what, np.argwhere(got != W)[:5])
    T = W.shape[3]
    for i, tau in enumerate(int(t) for t in lags):
        tail = got[:, :, i, T - tau:]
        assert not tail.any() and not np.signbit(tail).any(), (what, "entries past the last origin of lag", tau)


def staged_cpu(x, dtype):
    c = _lib.Context("cpu")
    (view,) = c.stage_alloc(*x.shape, dtype=dtype)
    view[:] = x
    c.stage_commit(0, x.shape[0])
    return c


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["stage64", "stage32"])
@pytest.mark.parametrize("T,A,D,seed", [pytest.param(*c, id=f"T{c[0]}-A{c[1]}-D{c[2]}") for c in CASES])
def test_exact_on_the_cpu_backend(T, A, D, seed, dtype):
    x, k, lags, W, Q = case(T, A, D, seed)
    c = staged_cpu(x, dtype)
    try:
        w = c.overlap_density(k, lags, CUTOFFS)
        assert_exact(w, W, lags, f"cpu {dtype.__name__}")
        q = c.overlap(lags, CUTOFFS)
        assert np.array_equal(q, Q)
        assert np.array_equal(w[K0].real, q) and not w[K0].imag.any()
    finally:
        c.close()


def run_staged(c, k, lags, cutoffs):
    """ta_overlap_density_staged into a sentinel-filled device array -> float64 (K, C, L, T, 2)"""
    import torch

    out = torch.full((len(k), len(cutoffs), len(lags), c.shape[0], 2), -7.5, dtype=torch.float64, device="cuda:0")
    c.overlap_density_staged(k, lags, cutoffs, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["slab64", "slab32"])
@pytest.mark.parametrize("T,A,D,seed", [pytest.param(*c, id=f"T{c[0]}-A{c[1]}-D{c[2]}") for c in CASES])
def test_exact_on_the_gpu(T, A, D, seed, dtype):
    import torch

    from test_vanhove_shapes import stage, timeline

    x, k, lags, W, Q = case(T, A, D, seed)
    c = stage(_lib.Context(0), x, dtype)
    try:
        got = run_staged(c, k, lags, CUTOFFS)
        names = timeline(c)
        assert "k_overlap_density" in names and "k_widen_f32" not in names, names
        assert_exact(got, W, lags, f"gpu staged {dtype.__name__}")
        w = c.overlap_density(k, lags, CUTOFFS)
        assert np.array_equal(parts(w), got)  # the host-facing call
        q = torch.full(Q.shape, -7, dtype=torch.int64, device="cuda:0")
        c.overlap_staged(lags, CUTOFFS, q.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(got[K0, ..., 0], q.cpu().numpy()) and not got[K0, ..., 1].any()
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["slab64", "slab32"])
def test_every_chunk_gives_the_same_bits(dtype):
    from test_vanhove_shapes import stage

    x, k, lags, W, _ = case(*MAIN)
    c = stage(_lib.Context(0), x, dtype)
    try:
        for cuts in ((1, ), (0, 1, 3), (0, 1, 2, 3)):
            cutoffs = [CUTOFFS[i] for i in cuts]
            for chunk in (0, 1, 2, 3, 4, 64):
                c.set_option("overlap_density_chunk", chunk)
                assert_exact(run_staged(c, k, lags, cutoffs), W[:, list(cuts)], lags, f"C={len(cuts)} chunk={chunk}")
    finally:
        c.close()


@pytest.mark.gpu
def test_two_member_group_with_an_odd_split():
    x, k, lags, W, _ = case(*MAIN)
    T, A, D = x.shape
    g = _lib.Group([0, 0])
    try:
        (views,) = g.stage_alloc(T, A, D)
        assert any((hi - lo) % 2 for lo, hi in g.shards)
        for (lo, hi), view in zip(g.shards, views):
            view[:] = x[:, lo:hi]
        g.stage_commit(0, T)
        assert_exact(g.overlap_density(k, lags, CUTOFFS), W, lags, "group")
    finally:
        g.close()
