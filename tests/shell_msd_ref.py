"""Reference of the shell-resolved MSD sums, written from the definitions of include/ta_hip.h (ta_shell_msd) and independent of
the library, on top of shell_ref.  With g = shell_ref.filtered(shell_ref.levels(...), gap) (N_b, T) and the observed items'
positions in INTEGER grid units (int64 multiples of 2^-10), for tau = 0 ... L

    w_c[tau] = w_c[tau - 1][:, :-1] & g[:, tau:]       "continuous": inside in every frame from t to t + tau
    w_e[tau] = g[:, :T - tau] & g[:, tau:]             "endpoints"
    S[tau, j] = sum over (q, t) of w (x_j(t + tau) - x_j(t))^2,     N[tau] = sum over (q, t) of w

as exact integers.  Every S[tau, j] is asserted to stay below 2^53 grid units squared (and every squared difference with it):
the float64 sums of any order are then exact, and EVERY comparison is for equality, S included."""
import functools

import numpy as np

import shell_ref
from pair_ref import sums as pair_sums

GRID = shell_ref.GRID
CONDITIONS = ("continuous", "endpoints")


def gated_sums(x, b, g, L, condition):
    """(S (L + 1, D) float64 in position units squared, N (L + 1,) int64).  x (T, A, D) on the grid; b: the observed items
    (None: all); g (N_b, T) bool"""
    x = np.asarray(x, dtype=np.float64)
    T, A, D = x.shape
    b = np.arange(A) if b is None else np.asarray(b)
    g = np.asarray(g, dtype=bool)
    assert g.shape == (b.size, T) and 0 <= L <= T - 1 and condition in CONDITIONS
    xi = shell_ref.grid_units(x[:, b], "a position").transpose(1, 0, 2)  # (N_b, T, D)
    S = np.zeros((L + 1, D), dtype=np.int64)
    N = np.zeros(L + 1, dtype=np.int64)
    w = g.copy()
    for tau in range(L + 1):
        if tau:
            w = (w[:, :-1] & g[:, tau:]) if condition == "continuous" else (g[:, :T - tau] & g[:, tau:])
        d = xi[:, tau:] - xi[:, :T - tau]
        assert np.abs(d).max(initial=0) < 2 ** 26
        sq = (d * d) * w[:, :, None]
        S[tau] = sq.sum(axis=(0, 1))
        N[tau] = w.sum()
    assert S.max(initial=0) < 2 ** 53, "a sum would leave the exact range of float64"
    return S / float(GRID * GRID), N


def check_counts(g, L, N, condition):
    """N against pair_ref.sums of the same series: cc under "continuous", ci under "endpoints" """
    ci, runs, nb, cc = pair_sums(np.asarray(g, dtype=bool))
    assert np.array_equal(N, (cc if condition == "continuous" else ci)[:L + 1].astype(np.int64))
    return runs, nb


@functools.lru_cache(maxsize=None)
def case(T, Na, Nb, D, kind, boxed, gap, L, seed=1):
    """shell_ref.case with (g, {condition: (S, N)}, runs, nb) added: computed once and shared; not to be modified"""
    x, a, b, dims, axes, cuts, s, (ci, runs, nb, cc) = shell_ref.case(T, Na, Nb, D, kind, boxed, gap, seed)
    g = shell_ref.filtered(s, gap)
    want = {}
    for condition in CONDITIONS:
        S, N = gated_sums(x, b, g, L, condition)
        r, n = check_counts(g, L, N, condition)
        assert np.array_equal(r, runs) and np.array_equal(n, nb)
        S.setflags(write=False), N.setflags(write=False)
        want[condition] = (S, N)
    return x, a, b, dims, axes, cuts, g, want, runs, nb


def nojump(xw, box):
    """the NoJump recurrence ta_unwrap follows on an orthorhombic box (include/ta_hip.h): f(t) = x(t) / H(t), n(0) = 0,
    n(t) = n(t - 1) + rint(f(t) - f(t - 1)), x_u(t) = x(t) - n(t) H(t); xw (T, A, D) wrapped positions, box (T, D).  Exact
    for grid positions and power-of-two boxes.  (With a box that changes from frame to frame this is NOT the walk that was
    wrapped: its image count may change by more than one per frame; it is what the library's MSD is taken of.)"""
    xw = np.asarray(xw, dtype=np.float64)
    out = xw.copy()
    n = np.zeros(xw.shape[1:])
    for t in range(1, xw.shape[0]):
        n = n + np.rint(xw[t] / box[t][None, :] - xw[t - 1] / box[t - 1][None, :])
        out[t] = xw[t] - n * box[t][None, :]
    return out
