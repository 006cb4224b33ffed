"""Every compiled FFT plan (csrc/wfft.hpp, wfft_choose in csrc/wfft.hip) per lag and per particle.

The engine is a family of plans compiled per (R0, R), M = R R0 512: 15 on-chip plans (R = 1, R0 = 1 ... 10, 12, 14,
16, 18, 20) and 23 outer-radix plans (R = 2, 3, 4, 5, 8, 16 in front of R0 = 12 ... 20) that the cost rule
M (1 + 0.15 R) can return.  Each has its own Dft<R0> butterfly, row requests, LDS size, twiddle table, four forward
variants, two float32-slab variants and an inverse kernel; an error confined to one of them -- an output permutation
of a butterfly, a twiddle index, a row request past the end at one padding, an outer residue out of order -- shows
only where that plan runs.

(1) test_plans_table_is_complete (host): PLANS below is the whole table, first and last frame count of every plan;
    a new radix or another cost rule fails here until the sweep covers it.
(2) test_plan_sweep (gpu): every plan at its first frame count (the most padding, rows past the end) and at T = M
    (none), column shapes cycling through odd and even counts, particles scaled 2^0 ... 2^-36, by particle and lag
    sums: (a) np.longdouble sums on some 200 lags (sparse_lags), every lag and particle held to exact.fft_bound (the
    comparison of test_exact_parity.test_vacf_fft_error_model, FFT_C as it stands); (b) the NumPy oracle at ALL
    lags, scale-relative 1e-10 -- a bin error reaches every lag, an inverse-kernel output stored one place off only
    some.  test_plan_sweep_f32_slabs: the on-chip plans R0 >= 2 on float32 device slabs, which they read as they
    are, and one outer-radix plan, where k_widen_f32 must run.
(3) test_one_line_per_column (gpu): a constant plus one cosine per column whose line sits between two bins, the
    columns of a case covering every outer residue, the first / second / middle / last sub-series and the positions
    where a digit of the position carries.
(4) test_many_units_per_workgroup_outer_plan (gpu): 450 column pairs on plan (3, 14).
(5) test_msd_fft_plan_5_18, test_helfand_fft_plan_8_14 (gpu): the S1 - 2 S2 forms on outer plans they had not met,
    and the CPU backend inside the same bound at 40961 frames (host)."""
import functools

import numpy as np
import pytest

from conftest import scale_rel_err
from oracle import exact as ex
from oracle import numpy_oracle as orc
from test_exact_parity import context, float_walk, hetero, needs_longdouble, ratios, timeline
from transport_analysis_amd import _lib

TOL = 1e-10  # the project's parity bar (scale-relative)
T_MAX = 163840  # the largest plan; beyond, ta_vacf_fft runs the direct correlators

# (R, R0, M, first T, last T): M = R R0 512, last T = M.  On-chip plans, then the outer-radix plans wfft_choose returns.
PLANS = [
    (1, 1, 512, 1, 512),
    (1, 2, 1024, 513, 1024),
    (1, 3, 1536, 1025, 1536),
    (1, 4, 2048, 1537, 2048),
    (1, 5, 2560, 2049, 2560),
    (1, 6, 3072, 2561, 3072),
    (1, 7, 3584, 3073, 3584),
    (1, 8, 4096, 3585, 4096),
    (1, 9, 4608, 4097, 4608),
    (1, 10, 5120, 4609, 5120),
    (1, 12, 6144, 5121, 6144),
    (1, 14, 7168, 6145, 7168),
    (1, 16, 8192, 7169, 8192),
    (1, 18, 9216, 8193, 9216),
    (1, 20, 10240, 9217, 10240),
    (2, 12, 12288, 10241, 12288),
    (2, 14, 14336, 12289, 14336),
    (2, 16, 16384, 14337, 16384),
    (2, 18, 18432, 16385, 18432),
    (2, 20, 20480, 18433, 20480),
    (3, 14, 21504, 20481, 21504),
    (3, 16, 24576, 21505, 24576),
    (3, 18, 27648, 24577, 27648),
    (3, 20, 30720, 27649, 30720),
    (4, 16, 32768, 30721, 32768),
    (4, 18, 36864, 32769, 36864),
    (4, 20, 40960, 36865, 40960),
    (5, 18, 46080, 40961, 46080),
    (5, 20, 51200, 46081, 51200),
    (8, 14, 57344, 51201, 57344),
    (8, 16, 65536, 57345, 65536),
    (8, 18, 73728, 65537, 73728),
    (8, 20, 81920, 73729, 81920),
    (16, 12, 98304, 81921, 98304),
    (16, 14, 114688, 98305, 114688),
    (16, 16, 131072, 114689, 131072),
    (16, 18, 147456, 131073, 147456),
    (16, 20, 163840, 147457, 163840),
]
assert len(PLANS) == 15 + 23 and all(M == R * R0 * 512 == last for R, R0, M, _, last in PLANS)
assert len({M for _, _, M, _, _ in PLANS}) == len(PLANS)  # M names the plan
OUTER_RADICES = sorted({R for R, *_ in PLANS})
FIRST_RADICES = sorted({R0 for _, R0, *_ in PLANS})

# (A, D): 3, 4, 3, 6 columns -- a pair and an unpaired real column of one particle, two aligned pairs, three single
# columns in either half of a pair, two particles that share their middle pair
COLUMN_SHAPES = [(1, 3), (2, 2), (3, 1), (2, 3)]


def column_shape(i_plan, i_frames):
    return COLUMN_SHAPES[(i_plan + i_frames) % 4]


def sweep_cases():
    """(R, R0, M, T, A, D): every plan at its first and last frame count; R0 = 1 at 257 frames as well (the first
    count of its two-pass kernels: up to 256 frames pass A alone is pad enough)."""
    out = []
    for i, (R, R0, M, first, last) in enumerate(PLANS):
        for j, T in enumerate((first, last) + ((257,) if M == 512 else ())):
            out.append((R, R0, M, T) + column_shape(i, j))
    return out


SWEEP = sweep_cases()
# every outer radix and every first-stage radix with an odd column count (an unpaired last column, single-column units)
# and with an even one
for _odd in (0, 1):
    assert {c[0] for c in SWEEP if c[4] * c[5] % 2 == _odd} == set(OUTER_RADICES)
    assert {c[1] for c in SWEEP if c[4] * c[5] % 2 == _odd} == set(FIRST_RADICES)
assert all(T <= T_MAX for _, _, _, T, _, _ in SWEEP)

# float32 device slabs: the on-chip plans R0 >= 2 at their first frame count, and the outer plan (2, 14)
SWEEP_F32 = [(R, R0, M, first) + column_shape(i, 2) for i, (R, R0, M, first, _) in enumerate(PLANS) if R == 1 and R0 >= 2]
SWEEP_F32.append((2, 14, 14336, 12289, 2, 3))
assert len(SWEEP_F32) == 14 + 1

SPARSE_N = 65 + 64 + 65 + 9  # at most: lags 0 ... 64, the last 64, a stride of T // 64, three around 512, M / 2 and M
FEW_N = 17 + 16 + 31  # the many-column cases


def sparse_lags(T, M):
    """Lags 0 ... 64, the last 64, a stride of T // 64, and k - 1, k, k + 1 around 512, M / 2 and M below T."""
    lags = set(range(min(65, T))) | set(range(max(0, T - 64), T)) | set(range(0, T, max(1, T // 64)))
    for k in (512, M // 2, M):
        lags |= {n for n in (k - 1, k, k + 1) if 0 <= n < T}
    assert len(lags) <= SPARSE_N
    return np.array(sorted(lags))


def few_lags(T):
    """The first 17 lags, the last 16 and 31 at a stride of T / 32."""
    lags = set(range(min(17, T))) | set(range(max(0, T - 16), T)) | {i * T // 32 for i in range(1, 32)}
    assert len(lags) <= FEW_N
    return np.array(sorted(lags))


def plan_of(T):
    """The row of PLANS whose frame counts include T."""
    (row,) = [p for p in PLANS if p[3] <= T <= p[4]]
    return row


# ------------------------------------------------------------------------------------------------- (1) completeness
def test_plans_table_is_complete():
    """Both sides of every multiple of 512 up to the largest plan through ta_fft_plan_info: the M values seen are
    those of PLANS and no others, every frame count lies in the range of the row with its M, and the ranges tile
    1 ... 163840 (one frame has the plan R0 = 1; 163841 has none)."""
    assert _lib.fft_plan_info(1)["M"] == 512
    assert _lib.fft_plan_info(T_MAX + 1) is None
    rows = {M: (first, last) for _, _, M, first, last in PLANS}
    seen = set()
    for j in range(T_MAX // 512 + 1):
        for T in (512 * j, 512 * j + 1):
            info = _lib.fft_plan_info(T)
            if T > T_MAX:
                assert info is None, T
                continue
            seen.add(info["M"])
            if T >= 1:
                assert info["M"] in rows, (T, info)
                first, last = rows[info["M"]]
                assert first <= T <= last, (T, info, first, last)
    assert seen == set(rows), seen ^ set(rows)
    edge = 1
    for R, R0, M, first, last in PLANS:
        assert first == edge, (R, R0, first, edge)  # the ranges follow one another
        edge = last + 1
        for T in (first, last):
            info = _lib.fft_plan_info(T)
            assert info["M"] == M, (R, R0, T, info)
            assert info["n_stages"] == (3 if R0 == 1 else 4) + (R > 1), (R, R0, info)
    assert edge == T_MAX + 1


# ------------------------------------------------------------------------------------------------ the comparisons
def vacf_calls(v, options, widened=False):
    """vacf_fft by particle and lag sums alone on a fresh context: (ts of the by-particle call, bp, ts).  Neither
    call takes k_short; k_widen_f32 runs exactly where `widened`; the plan's own kernels are in the timeline."""
    T = v.shape[0]
    on_chip_512 = plan_of(T)[2] == 512
    c = context([v], options)
    try:
        ts, bp = c.vacf_fft(by_particle=True)
        names_bp = timeline(c)
        ts2, none = c.vacf_fft(by_particle=False)
        names_ts = timeline(c)
    finally:
        c.close()
    assert none is None
    for names, kernels in ((names_bp, ("k_w1_bp",) if on_chip_512 else ("k_wsplit_accum", "k_winverse")),
                           (names_ts, ("k_w1_accum",) if on_chip_512 else ("k_wsplit_accum", "k_winverse"))):
        assert "k_short" not in names, names
        assert ("k_widen_f32" in names) == widened, (widened, names)
        assert all(k in names for k in kernels), (kernels, names)
    return ts, bp, ts2


def check_vacf(v, M, got, lags, label, record_property):
    """(a) np.longdouble sums at `lags`: every by-particle element within fft_bound(T, 2 M, E of the particles that
    share its transforms), the lag sums of both calls within fft_bound(T, 2 M, sum E) / A.  (b) the NumPy oracle at
    every lag, scale-relative TOL."""
    ts, bp, ts2 = got
    T, A, D = v.shape
    assert bp.shape == (T, A) and ts.shape == ts2.shape == (T,)
    den = (T - lags).astype(np.longdouble)[:, None]
    ref = ex.ld_corr(v.reshape(T, A * D), lags).reshape(len(lags), A, D).sum(axis=2) / den
    e = ex.column_energy(v).sum(axis=1)
    r_bp = ratios(bp[lags], ref, ex.fft_bound(T, 2 * M, ex.fft_energy_bp(e))[lags])
    want_ts = ref.sum(axis=1) / A
    b_ts = ex.fft_bound(T, 2 * M, e.sum())[lags] / A
    r_ts1, r_ts2 = ratios(ts[lags], want_ts, b_ts), ratios(ts2[lags], want_ts, b_ts)
    r_ts = max(r_ts1.max(), r_ts2.max())
    want_bp, want_mean = orc.vacf_fft_batched(v, atom_block=64)
    rel = {"bp": scale_rel_err(bp, want_bp), "ts_bp": scale_rel_err(ts, want_mean), "ts": scale_rel_err(ts2, want_mean)}
    record_property("fft_ratio", {"plan": label, "shape": [T, A, D], "bp": float(r_bp.max()), "ts": float(r_ts),
                                  "rel": {k: float(x) for k, x in rel.items()}})
    print(f"fft_ratio {label} T={T} A={A} D={D} bp={r_bp.max():.4f} ts={r_ts:.4f} "
          f"rel_bp={rel['bp']:.2e} rel_ts={max(rel['ts_bp'], rel['ts']):.2e}")
    worst = np.unravel_index(int(np.argmax(r_bp)), r_bp.shape)
    assert r_bp.max() <= 1.0, (label, "by particle: lag", int(lags[worst[0]]), "particle", int(worst[1]), float(r_bp.max()))
    assert r_ts <= 1.0, (label, "lag sums: lag", int(lags[int(np.argmax(np.maximum(r_ts1, r_ts2)))]), float(r_ts))
    assert max(rel.values()) < TOL, (label, rel)


def plan_id(R, R0, T, A, D):
    return f"R{R}-R0_{R0}-T{T}-{A}x{D}"


# ------------------------------------------------------------------------------------------------- (2) the sweep
@needs_longdouble
@pytest.mark.gpu
@pytest.mark.parametrize("R,R0,M,T,A,D", [pytest.param(*c, id=plan_id(c[0], c[1], *c[3:])) for c in SWEEP])
def test_plan_sweep(R, R0, M, T, A, D, record_property):
    """Every plan at its first frame count, at T = M (R0 = 1: and at 257), float64 slabs; "short_max" 0 keeps k_short
    out of the short ones."""
    assert _lib.fft_plan_info(T)["M"] == M
    v = orc.synthetic_velocities(T, A, D, seed=4000 + T) * hetero(A)
    got = vacf_calls(v, {"short_max": 0})
    check_vacf(v, M, got, sparse_lags(T, M), f"R={R} R0={R0} f64", record_property)


@needs_longdouble
@pytest.mark.gpu
@pytest.mark.parametrize("R,R0,M,T,A,D", [pytest.param(*c, id=plan_id(c[0], c[1], *c[3:])) for c in SWEEP_F32])
def test_plan_sweep_f32_slabs(R, R0, M, T, A, D, record_property):
    """float32 device slabs ("stage_device_f32") of velocities rounded to float32: the on-chip plans R0 >= 2 read them
    as they are (k_wsplit_accum<..., SRC32>, no k_widen_f32); behind an outer radix they are widened first."""
    assert _lib.fft_plan_info(T)["M"] == M
    v = (orc.synthetic_velocities(T, A, D, seed=4000 + T) * hetero(A)).astype(np.float32).astype(np.float64)
    got = vacf_calls(v, {"short_max": 0, "stage_device_f32": 1}, widened=R > 1)
    check_vacf(v, M, got, sparse_lags(T, M), f"R={R} R0={R0} f32slab", record_property)


# ------------------------------------------------------------------------------------------ (3) one line per column
# positions s = a + 8 b + 64 cc where a digit carries, and a neighbour of each
CARRY_POSITIONS = [0, 1, 7, 6, 8, 9, 63, 62, 64, 65, 511, 510]
LINE_PLANS = [p for p in PLANS if p[0] > 1 or p[1] >= 2]


def line_targets(R, R0):
    """(rho, q, s) per column of a one-line case.  Bin k = 2 R (q + R0 s) + c of the L = 2 M point transform is position
    s < 512 of sub-series q < R0 in pass c < 2 R of the forward kernel (wfft.hpp: Z[2 R s' + c] = FFT_M(u_c)[s'], and
    bin s' = q + R0 s of a pass), c = 2 rho + p: rho < R the residue of the outer radix (u_c sums the R strided rows
    with W_R^{rho jo}), p the half-bin twist (R = 1: pass A / pass B).  Column j: rho = j mod R; q from 0, 1, R0 / 2,
    R0 - 1, advancing with j and once more every fourth column; s = CARRY_POSITIONS[5 j mod 12].  15 columns as
    (5, 3) -- an odd count, particles that share a column pair -- and 18 as (6, 3) behind R = 16."""
    qs = sorted({0, 1 % R0, R0 // 2, R0 - 1})
    n_cols = 18 if R > 12 else 15
    t = [(j % R, qs[(j + j // 4) % len(qs)], CARRY_POSITIONS[5 * j % 12]) for j in range(n_cols)]
    assert {rho for rho, _, _ in t} == set(range(R))
    assert {q for _, q, _ in t} == set(qs)
    assert {s for _, _, s in t} == set(CARRY_POSITIONS)
    return t


for _R, _R0, *_ in LINE_PLANS:
    line_targets(_R, _R0)


@needs_longdouble
@pytest.mark.gpu
@pytest.mark.parametrize("R,R0,M", [pytest.param(*p[:3], id=f"R{p[0]}-R0_{p[1]}") for p in LINE_PLANS])
def test_one_line_per_column(R, R0, M, record_property):
    """T = M frames, column j = 0.3 + 0.1 j + (1 + 0.25 j) cos(2 pi t / period_j + 0.7 j) with period_j = L / (k_j + 1/2),
    k_j = 2 R (q_j + R0 s_j) + 2 rho_j: its line falls between the passes 2 rho_j and 2 rho_j + 1 of position s_j of
    sub-series q_j (line_targets: every rho < R; q = 0, 1, R0 / 2, R0 - 1; s = 0, 7, 8, 63, 64, 511 and a neighbour of
    each).  The construction of test_mirror_twiddles_concentrated_spectrum on every plan with a first stage, by
    particle and lag sums, at FEW_N lags against np.longdouble sums and at all lags against the NumPy oracle."""
    T, L = M, 2 * M
    targets = line_targets(R, R0)
    D = 3
    A = len(targets) // D
    t = np.arange(T, dtype=np.float64)
    v = np.empty((T, A, D))
    for j, (rho, q, s) in enumerate(targets):
        k = 2 * R * (q + R0 * s) + 2 * rho
        assert 0 <= k < L - 1
        period = L / (k + 0.5)
        assert (512 / period) % 1 and (L / period) % 1  # divides neither
        v[:, j // D, j % D] = 0.3 + 0.1 * j + (1.0 + 0.25 * j) * np.cos(2 * np.pi * t / period + 0.7 * j)
    got = vacf_calls(v, {})
    check_vacf(v, M, got, few_lags(T), f"R={R} R0={R0} lines", record_property)


# ------------------------------------------------------------------------- (4) many units per workgroup, plan (3, 14)
@needs_longdouble
@pytest.mark.gpu
def test_many_units_per_workgroup_outer_plan(record_property):
    """20481 x 300 x 3: 450 column pairs on plan (3, 14), more than its workgroups, so every tuple of six carries its
    accumulators across several pairs; lag sums, all lags against the NumPy oracle and 16 lags against np.longdouble
    sums (the references of 900 columns are most of this test's time)."""
    T, A, D = 20481, 300, 3
    R, R0, M = plan_of(T)[:3]
    assert (R, R0) == (3, 14) and _lib.fft_plan_info(T)["M"] == M
    v = orc.synthetic_velocities(T, A, D, seed=4000 + T)
    c = context([v], {})
    try:
        ts, none = c.vacf_fft(by_particle=False)
        names = timeline(c)
    finally:
        c.close()
    assert none is None and "k_wsplit_accum" in names and "k_winverse" in names, names
    lags = np.array([0, 1, 63, 64, 65, 512, 513, T // 2 - 1, T // 2, T // 2 + 1, M // 2, T - 65, T - 64, T - 63, T - 2,
                     T - 1])
    assert len(lags) == 16
    want = ex.ld_corr(v.reshape(T, A * D), lags).sum(axis=1) / (T - lags).astype(np.longdouble) / A
    r = ratios(ts[lags], want, ex.fft_bound(T, 2 * M, ex.column_energy(v).sum())[lags] / A)
    _, want_all = orc.vacf_fft_batched(v, atom_block=32)
    rel = scale_rel_err(ts, want_all)
    record_property("fft_ratio", {"plan": f"R={R} R0={R0} many pairs", "ts": float(r.max()), "rel": rel})
    print(f"fft_ratio R={R} R0={R0} many-pairs T={T} A={A} D={D} ts={r.max():.4f} rel_ts={rel:.2e}")
    assert r.max() <= 1.0, ("lag", int(lags[int(np.argmax(r))]), float(r.max()))
    assert rel < TOL, rel


# ------------------------------------------------------------------------------------------- (5) the S1 - 2 S2 forms
MSD_T, MSD_A, MSD_D = 40961, 2, 3  # plan (5, 18)
HELF_T, HELF_A, HELF_D = 51201, 2, 2  # plan (8, 14)


@functools.lru_cache(maxsize=1)
def msd_case():
    """(x, lags, np.longdouble MSD by particle at lags, by-particle bound, lag-sum bound) of float_walk at MSD_T."""
    T, A, D = MSD_T, MSD_A, MSD_D
    M = plan_of(T)[2]
    x = float_walk(T, A, D, seed=T)
    a = x - x[0]
    lags = sparse_lags(T, M)
    den = (T - lags).astype(np.longdouble)
    ref = ex.ld_sqdiff(x.reshape(T, A * D), lags).reshape(len(lags), A, D).sum(axis=2) / den[:, None]
    e = ex.column_energy(a).sum(axis=1)
    S1 = ex.s1_float(a).sum(axis=2)
    b_bp = ex.fft_bound(T, 2 * M, ex.fft_energy_bp(e), S1)[lags]
    b_ts = ex.fft_bound(T, 2 * M, e.sum(), S1.sum(axis=1))[lags] / A
    return x, lags, ref, b_bp, b_ts


def s1_2s2_ratios(lags, ref, b_bp, b_ts, ts, bp, ts2):
    A = ref.shape[1]
    want_ts = ref.sum(axis=1) / A
    r_bp = ratios(bp[lags], ref, b_bp)
    return float(r_bp.max()), float(max(ratios(ts[lags], want_ts, b_ts).max(), ratios(ts2[lags], want_ts, b_ts).max()))


@needs_longdouble
def test_msd_fft_bound_on_the_host_at_40961():
    """The CPU backend's msd(True) on the input of test_msd_fft_plan_5_18 within the bound that test holds the GPU to
    (L = 2 M of plan (5, 18), below the backend's own 2^17): the bound is not too tight for an FFT at this length."""
    x, lags, ref, b_bp, b_ts = msd_case()
    c = _lib.Context("cpu")
    try:
        (slab,) = c.stage_alloc(*x.shape)
        slab[:] = x
        c.stage_commit(0, x.shape[0])
        ts, bp = c.msd(True, by_particle=True)
        ts2, _ = c.msd(True, by_particle=False)
    finally:
        c.close()
    r_bp, r_ts = s1_2s2_ratios(lags, ref, b_bp, b_ts, ts, bp, ts2)
    print(f"cpu backend msd fft T={MSD_T}: bp={r_bp:.4f} ts={r_ts:.4f}")
    assert r_bp <= 1.0 and r_ts <= 1.0, (r_bp, r_ts)


@needs_longdouble
@pytest.mark.gpu
def test_msd_fft_plan_5_18(record_property):
    """msd(True) (k_msd_prepare: P = x - x[0], S1 - 2 S2) at 40961 frames, plan (5, 18): walks at +1e4 with a drift,
    particles scaled 1 and 2^-12, by particle and lag sums within fft_bound(..., S1) at the lags of sparse_lags."""
    x, lags, ref, b_bp, b_ts = msd_case()
    assert plan_of(MSD_T)[:2] == (5, 18) and _lib.fft_plan_info(MSD_T)["M"] == 46080
    c = context([x], {})
    try:
        ts, bp = c.msd(True, by_particle=True)
        assert "k_msd_prepare" in timeline(c) and "k_wsplit_accum" in timeline(c), timeline(c)
        ts2, _ = c.msd(True, by_particle=False)
        assert "k_msd_prepare" in timeline(c) and "k_wsplit_accum" in timeline(c), timeline(c)
    finally:
        c.close()
    r_bp, r_ts = s1_2s2_ratios(lags, ref, b_bp, b_ts, ts, bp, ts2)
    record_property("fft_ratio", {"plan": "R=5 R0=18 msd", "bp": r_bp, "ts": r_ts})
    print(f"fft_ratio R=5 R0=18 msd T={MSD_T} A={MSD_A} D={MSD_D} bp={r_bp:.4f} ts={r_ts:.4f}")
    assert r_bp <= 1.0, ("by particle", r_bp)
    assert r_ts <= 1.0, ("lag sums", r_ts)


@needs_longdouble
@pytest.mark.gpu
def test_helfand_fft_plan_8_14(record_property):
    """The "helfand_fft" option (S1 - 2 S2 on P = (m v) x) at 51201 frames, plan (8, 14): the input of
    test_exact_parity.helfand_float (masses 1 ... 200, P carrying the particle's 2^s_n once) at the lags of
    sparse_lags."""
    T, A, D = HELF_T, HELF_A, HELF_D
    R, R0, M = plan_of(T)[:3]
    assert (R, R0) == (8, 14) and _lib.fft_plan_info(T)["M"] == M
    rng = np.random.default_rng(T + 17)
    v = rng.standard_normal((T, A, D)) * hetero(A)
    x = float_walk(T, A, D, seed=T + 1) / hetero(A)
    m = rng.uniform(1.0, 200.0, size=A)
    P = (m[None, :, None] * v) * x
    lags = sparse_lags(T, M)
    ref = ex.ld_sqdiff(P.reshape(T, A * D), lags).reshape(len(lags), A, D).sum(axis=2)
    ref = ref / (D * (T - lags)).astype(np.longdouble)[:, None]
    e = ex.column_energy(P).sum(axis=1)
    S1 = ex.s1_float(P).sum(axis=2)
    b_bp = ex.fft_bound(T, 2 * M, ex.fft_energy_bp(e), S1)[lags] / D
    b_ts = ex.fft_bound(T, 2 * M, e.sum(), S1.sum(axis=1))[lags] / (D * A)
    c = context([v, x], {"helfand_fft": 1})
    try:
        ts, bp = c.helfand_msd(m, 1.0, by_particle=True)
        assert "k_helfand_combine" in timeline(c) and "k_wsplit_accum" in timeline(c), timeline(c)
        ts2, _ = c.helfand_msd(m, 1.0, by_particle=False)
        assert "k_helfand_combine" in timeline(c) and "k_wsplit_accum" in timeline(c), timeline(c)
    finally:
        c.close()
    r_bp, r_ts = s1_2s2_ratios(lags, ref, b_bp, b_ts, ts, bp, ts2)
    record_property("fft_ratio", {"plan": "R=8 R0=14 helfand", "bp": r_bp, "ts": r_ts})
    print(f"fft_ratio R=8 R0=14 helfand T={T} A={A} D={D} bp={r_bp:.4f} ts={r_ts:.4f}")
    assert r_bp <= 1.0, ("by particle", r_bp)
    assert r_ts <= 1.0, ("lag sums", r_ts)
