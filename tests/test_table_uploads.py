"""The host tables of ta_species_self_staged (the sorted order), ta_scatter_staged (the wavevectors), ta_vanhove_staged (lags
and edges), ta_vanhove_distinct_staged (lags, edges, index lists), ta_pair_lifetime_staged and ta_bond_lifetime_staged (box,
rows, labels) and the three ta_shell_*_staged calls (box, index lists, labels, index rows) travel to the device by an
asynchronous copy out of host storage the context keeps.  Staging call n + 1's table must not disturb the upload of call n:
two calls with DIFFERENT tables of the SAME byte size are queued on one stream into separate outputs with no synchronisation
between them, and each output must equal, bit for bit, that of the same call made alone and synchronised.  GPU only.

One context, 9 frames x 70 atoms x 3 in float64; every case is a handful of tiny launches."""
import numpy as np
import pytest

from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu

T, A, D = 9, 70, 3


@pytest.fixture(scope="module")
def ctx():
    rng = np.random.default_rng(31)
    x = np.cumsum(rng.normal(scale=0.4, size=(T, A, D)), axis=0) + rng.uniform(0, 6, size=(1, A, D))
    c = _lib.Context(0)
    (view,) = c.stage_alloc(T, A, D, dtype=np.float64)
    view[:] = x
    c.stage_commit(0, T)
    yield c
    c.close()


def _outputs(shapes):
    import torch

    return [torch.full(s, -7, dtype=dt, device="cuda:0") for s, dt in shapes]


def _bits(tensors):
    import torch

    torch.cuda.synchronize()
    return [t.cpu().numpy().view(np.uint64) for t in tensors]


# each of these queues one call with the given table into fresh output tensors and returns them, unsynchronised
def _species_self(c, labels):
    import torch

    (out,) = outs = _outputs([((3, T), torch.float64)])
    c.species_self_staged(0, 1, 3, labels, out.data_ptr())
    return outs


def _scatter(c, kvecs):
    import torch

    s, rho, f = outs = _outputs([((2, T), torch.float64), ((2, T, 2), torch.float64), ((2, T), torch.float64)])
    c.scatter_staged(1, kvecs, s.data_ptr(), rho.data_ptr(), f.data_ptr())
    return outs


def _vanhove(c, lags):
    import torch

    cnt, mom = outs = _outputs([((3, 9), torch.int64), ((3, 2), torch.float64)])
    c.vanhove_staged(lags, 8, 0.25, cnt.data_ptr(), mom.data_ptr())
    return outs


def _vanhove_distinct(c, idx_a):
    import torch

    (cnt,) = outs = _outputs([((2, 9), torch.int64)])
    c.vanhove_distinct_staged([0, 3], 8, 0.75, cnt.data_ptr(), idx_a=idx_a)
    return outs


# The pair and shell family: pair_tab (box | rows | zero labels) and shell_tab (zero lag | box | idx_a | idx_b | zero labels |
# index rows).  The shell tables carry a box and, for shell_orient, index rows: every segment of the layout is there.  The
# gated calls run to max_lag = T - 1.
BOX = np.tile([9.0, 9.0, 9.0, 90.0, 90.0, 90.0], (T, 1))
REFERENCE = np.arange(0, 20)
OBSERVED = np.arange(20, 50), np.arange(35, 65)  # two b lists of one length, both disjoint from the reference items
SHELL = dict(r_break=2.4, gap=1, idx_a=REFERENCE, dimensions=BOX)
LIFE = [((T,), "float64"), ((T + 1,), "int64"), ((T,), "float64")]


def _life_outputs(n_sums=0):
    """(ci, runs, nb), or with n_sums sums per lag (sums, count, runs, nb), and their device pointers"""
    import torch

    gated = [((T, n_sums), "float64"), ((T,), "int64")] if n_sums else LIFE[:1]
    outs = _outputs([(s, getattr(torch, dt)) for s, dt in gated + LIFE[1:]])
    return outs, [o.data_ptr() for o in outs]


def _pair_lifetime(c, pairs):
    outs, (ci, runs, nb) = _life_outputs()
    c.pair_lifetime_staged(0, 2.0, pairs, d_ci=ci, d_runs=runs, d_nb=nb)
    return outs


def _bond_lifetime(c, atoms):
    outs, (ci, runs, nb) = _life_outputs()
    c.bond_lifetime_staged(0, atoms, 3.0, r_break=3.6, cos_cut=0.0, gap=1, dimensions=BOX, d_ci=ci, d_runs=runs, d_nb=nb)
    return outs


def _shell_residence(c, idx_b):
    outs, (ci, runs, nb) = _life_outputs()
    c.shell_residence_staged(0, 1.8, idx_b=idx_b, d_ci=ci, d_runs=runs, d_nb=nb, **SHELL)
    return outs


def _shell_msd(c, idx_b):
    outs, (sums, count, runs, nb) = _life_outputs(D)
    c.shell_msd_staged("continuous", T - 1, 1.8, idx_b=idx_b, d_sums=sums, d_count=count, d_runs=runs, d_nb=nb, **SHELL)
    return outs


def _shell_orient(c, partner):
    # bond vectors anchor -> partner: the same anchors, the observed items, in both tables
    outs, (sums, count, runs, nb) = _life_outputs(2)
    c.shell_orient_staged("endpoints", T - 1, np.stack([OBSERVED[0], partner], axis=1), "bond", 1.8, idx_b=OBSERVED[0], d_sums=sums,
                          d_count=count, d_runs=runs, d_nb=nb, **SHELL)
    return outs


USERS = {
    "species_self_staged": (_species_self, (np.arange(A) % 3, np.arange(A) // 24)),
    "scatter_staged": (_scatter, (np.array([[0.9, 0.0, 0.0], [0.0, 1.3, 0.4]]), np.array([[0.0, 0.0, 1.1], [0.7, 0.7, 0.0]]))),
    "vanhove_staged": (_vanhove, ((0, 1, 4), (0, 2, 5))),
    "vanhove_distinct_staged": (_vanhove_distinct, (np.arange(0, 40), np.arange(25, 65))),
    "pair_lifetime_staged": (_pair_lifetime, tuple(np.stack([np.arange(30), np.arange(30) + k], axis=1) for k in (1, 35))),
    "bond_lifetime_staged": (_bond_lifetime, tuple(np.stack([np.arange(30), np.arange(30) + k, np.arange(30) + 2 * k], axis=1)
                                                   for k in (1, 20))),
    "shell_residence_staged": (_shell_residence, OBSERVED),
    "shell_msd_staged": (_shell_msd, OBSERVED),
    "shell_orient_staged": (_shell_orient, (OBSERVED[0] + 1, OBSERVED[0] + 20)),
}

_alone = {}


def alone(c, user, i):
    """the bits of `user`'s call with its table i made alone and synchronised: computed once, shared, left unchanged"""
    if (user, i) not in _alone:
        import torch

        torch.cuda.synchronize()
        call, tables = USERS[user]
        _alone[user, i] = _bits(call(c, tables[i]))
    return _alone[user, i]


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("user", list(USERS))
def test_two_tables_back_to_back(ctx, user):
    call, tables = USERS[user]
    want = [alone(ctx, user, 0), alone(ctx, user, 1)]
    assert not same(want[0], want[1]), "the two tables must give different outputs, or nothing is tested"
    first = call(ctx, tables[0])
    second = call(ctx, tables[1])  # queued while the first call's upload may still be in flight
    got = _bits(first), _bits(second)
    assert same(got[0], want[0]), f"{user}: the first call's output differs from the same call made alone"
    assert same(got[1], want[1]), f"{user}: the second call's output differs from the same call made alone"


def test_one_call_of_each_back_to_back(ctx):
    want = {user: alone(ctx, user, 0) for user in USERS}
    queued = {user: call(ctx, tables[0]) for user, (call, tables) in USERS.items()}
    for user, outs in queued.items():
        assert same(_bits(outs), want[user]), f"{user}: its output differs from the same call made alone"
