"""EinsteinMSD and ConductivityHelfand on the GPU at shapes that reach every tile, stride and tail of their kernels.

The parity tests of test_msd.py and test_conductivity.py use a few dozen columns, so each workgroup of k_msd_prepare and
k_cond_moment sees one column pair, k_msd_prepare_bp one partial atom tile, and the MODE_MSD direct kernels one pass over
their atoms.  The cases here are sized so that:
  * k_msd_prepare (lag sums) and k_cond_moment run with more column pairs than workgroups (n_pairs > 1024, and the
    20000-frame case whose 20 frame blocks cut k_cond_moment's group count to ~8 n_cu / 20), with even and odd column
    counts and pairs that straddle two atoms at D = 1, 2, 3;
  * k_msd_prepare_bp runs many 64-atom tiles whose last atom tile and last time tile are partial;
  * k_short, k_mid and k_direct in MODE_MSD loop over several column groups per workgroup, and write the by-particle
    array through k_bp_transpose / k_row_sums into rows wider than n_atoms;
  * the FFT form runs a plan with an outer radix (10300 and 20000 frames).
Each case asserts from the kernel timeline that it ran the kernel it is there for, and compares with the float64
direct forms of oracle/numpy_oracle.py at the lags of lag_sample (every lag next to a 64- or 1024-frame boundary) or,
for Phi, at every lag.  test_reference_helpers_match_full_restatements pins those helpers without a GPU."""
import functools

import numpy as np
import pytest

from conftest import scale_rel_err
from oracle import numpy_oracle as orc
from test_conductivity import mixed_charges, moment_np, msd_lags, self_term_np
from test_msd import msd_direct
from transport_analysis_amd import ConductivityHelfand, EinsteinMSD, _lib
from transport_analysis_amd._mini_mda import ArrayUniverse

BOX = [40.0, 50.0, 60.0, 90, 90, 90]
LDS_PER_CU = 160 * 1024  # gfx950


# ------------------------------------------------------------------------------------------------ inputs, references
@functools.lru_cache(maxsize=None)
def walk(T, A, D, seed, drift=0.0):
    """Random walks 1000 away from the origin, like unwrapped positions; `drift` adds one walk shared by every atom,
    `drift` times the atoms' own step (a moving centre of mass: a neutral system's moment cancels it)."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.standard_normal((T, A, D)), axis=0) + 1000.0
    if drift:
        x += drift * np.cumsum(rng.standard_normal((T, 1, D)), axis=0)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def msd_ref(T, A, D, seed, drift=0.0, f32=False):
    """(lags, per-atom MSD at those lags) of walk(...), float32-rounded first with f32."""
    x = walk(T, A, D, seed, drift)
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    lags = orc.lag_sample(T)
    return lags, orc.msd_at_lags(x, lags)


def near_neutral_charges(A, seed):
    rng = np.random.default_rng(seed + 2)
    q = rng.uniform(-1.5, 1.5, size=A)
    q -= q.mean()
    q[0] += 1e-6  # not exactly neutral
    return q


def staged_context(x, dtype=np.float64):
    T, A, D = x.shape
    c = _lib.Context(0)
    (view,) = c.stage_alloc(T, A, D, dtype=dtype)
    view[:] = x
    c.stage_commit(0, T)
    c.set_option("timeline", 1)
    return c


def timeline(c):
    return [n for n, _ in c.kernel_timeline(64)]


def n_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


# -------------------------------------------------------------------------------------- the reference, without a GPU
@pytest.mark.parametrize("T,A,D", [(1, 3, 3), (2, 4, 2), (67, 5, 3), (130, 3, 1), (150, 4, 2)])
def test_reference_helpers_match_full_restatements(T, A, D):
    x = walk(T, A, D, seed=T + A)
    q = mixed_charges(A, seed=T)
    lags = np.arange(T)
    bp = orc.msd_at_lags(x, lags)
    assert bp.shape == (T, A)
    assert scale_rel_err(bp, msd_direct(x)) <= 1e-14
    assert scale_rel_err(bp.sum(axis=1), msd_direct(x).sum(axis=1)) <= 1e-14
    m, s = orc.cond_moment(x, q)
    assert np.max(np.abs(m - moment_np(x, q))) <= 1e-13 * max(np.max(s), 1e-300)
    assert np.all(s * (1 + 1e-12) >= np.abs(m))
    assert scale_rel_err(orc.moment_msd(m), msd_lags(m)) <= 1e-14
    assert scale_rel_err(orc.self_term_at_lags(x, q, lags), self_term_np(x, q)) <= 1e-14
    sub = orc.lag_sample(T)[::3]  # any subset of lags, in the order given
    assert scale_rel_err(orc.msd_at_lags(x, sub[::-1]), msd_direct(x)[sub[::-1]]) <= 1e-14


def test_lag_sample_covers_the_boundaries():
    for T in (1, 50, 64, 65, 300, 1100, 2048, 2049, 10300):
        lags = orc.lag_sample(T)
        assert np.all(np.diff(lags) > 0) and lags[0] == 0 and lags[-1] == T - 1
        have = set(lags.tolist())
        assert set(range(min(65, T))) <= have
        assert set(range(max(0, T - 64), T)) <= have
        for b in range(64, T, 64):  # every 64-frame boundary (so every 1024-frame one) from both sides
            assert {b - 1, b} <= have, (T, b)
    assert len(orc.lag_sample(10300)) < 600


# ----------------------------------------------------------------------------------------------------- EinsteinMSD
# (id, T, A, D, forms): forms = [(fft, kernel the call must run)].  Frame counts select the dispatch:
# k_short <= 64 for both forms; fft=False k_mid 65 ... 512, k_direct beyond; fft=True the FFT form (k_msd_prepare).
MSD_CASES = [
    # k_short with more 21-atom tiles than 4 waves x (1 or 2 workgroups per CU) x n_cu: every wave loops
    ("short_loop", 50, 48001, 3, [(True, "k_short"), (False, "k_short")]),
    # k_mid with 1000 groups of 15 columns over at most 3 workgroups per CU; FFT form: 7500 pairs, 79 atom tiles (the last
    # 8 atoms) x 5 time tiles (the last 44 frames)
    ("mid_loop", 300, 5000, 3, [(False, "k_mid"), (True, "k_msd_prepare")]),
    # n_pairs > 1024 at every D, odd and even column counts; atoms and frames not multiples of 64
    ("odd_cols_d3", 1100, 1501, 3, [(False, "k_direct"), (True, "k_msd_prepare")]),
    ("even_cols_d3", 1100, 1500, 3, [(False, "k_direct"), (True, "k_msd_prepare")]),
    ("d2", 1100, 1100, 2, [(False, "k_direct"), (True, "k_msd_prepare")]),
    ("odd_cols_d1", 300, 2101, 1, [(False, "k_mid"), (True, "k_msd_prepare")]),
    # an FFT plan with an outer radix (12288 = 2 x 12 x 512)
    ("outer_radix", 10300, 700, 3, [(True, "k_msd_prepare")]),
]
MSD_KERNELS = {"k_short", "k_mid", "k_direct", "k_msd_prepare"}


def _msd_case_params():
    for case_id, T, A, D, forms in MSD_CASES:
        for fft, kernel in forms:
            yield pytest.param(T, A, D, fft, kernel, id=f"{case_id}-T{T}-A{A}-D{D}-{'fft' if fft else 'direct'}-{kernel}")


@pytest.mark.gpu
@pytest.mark.parametrize("T,A,D,fft,kernel", list(_msd_case_params()))
def test_msd_shapes(T, A, D, fft, kernel):
    lags, want_bp = msd_ref(T, A, D, seed=T + A + D)
    want_ts = want_bp.mean(axis=1)  # the host call's timeseries: the mean over atoms (the device calls: the sum)
    if kernel == "k_short":
        # a wave's tile is 64 columns of whole atoms; 4 waves per workgroup and per_cu <= the kernel's waves per SIMD
        # (amdgpu_waves_per_eu: 1 with the by-particle array, 2 without)
        assert -(-A // ((63 if D == 3 else 64) // D)) > 4 * 2 * n_cu(), "the case no longer loops over tiles"
    if kernel == "k_mid" and A * D > 10000:
        # mid.hip mid_shape: 2^4 lanes per column group above 256 frames, (ncl ts + T) doubles of LDS per workgroup
        ncl = 16 if T > 256 else 32 if T > 128 else 64
        ts = (T + 15) // 16 * 16 + 18
        per_cu = LDS_PER_CU // (8 * (ncl * ts + T))
        assert -(-A * D // (ncl // D * D)) > per_cu * n_cu(), "the case no longer loops over tiles"
    if kernel == "k_msd_prepare":  # several pairs per workgroup or an outer radix; partial last 64 x 64 tiles
        assert (A * D + 1) // 2 > 1024 or _lib.fft_plan_info(T)["n_stages"] == 5
        assert A % 64 and T % 64
    c = staged_context(walk(T, A, D, seed=T + A + D))
    try:
        for by_particle in (False, True):
            ts, bp = c.msd(fft, by_particle=by_particle)
            names = timeline(c)
            assert kernel in names and not (MSD_KERNELS - {kernel}) & set(names), names
            assert ts[0] == 0.0
            assert scale_rel_err(ts[lags], want_ts) <= 1e-10, by_particle
            if by_particle:
                assert bp.shape == (T, A)
                assert scale_rel_err(bp[lags], want_bp) <= 1e-10
                assert np.all(bp[0] == 0.0)
    finally:
        c.close()


@pytest.mark.gpu
def test_msd_direct_workgroups_loop():
    """k_direct with the grid capped ("direct_nwg") below the atom groups: every workgroup takes several."""
    T, A, D = 1100, 1100, 2
    lags, want_bp = msd_ref(T, A, D, seed=T + A + D)
    c = staged_context(walk(T, A, D, seed=T + A + D))
    try:
        c.set_option("direct_nwg", 7)
        for by_particle in (False, True):
            ts, bp = c.msd(False, by_particle=by_particle)
            assert "k_direct" in timeline(c)
            assert scale_rel_err(ts[lags], want_bp.mean(axis=1)) <= 1e-10
            if by_particle:
                assert scale_rel_err(bp[lags], want_bp) <= 1e-10
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("device_f32", [0, 1], ids=["device_f64", "device_f32"])
def test_msd_float32_staged(device_f32):
    """Float32 staging: the reference is the float32-rounded positions in float64.  The device slab is float64, or with
    "stage_device_f32" float32, widened by k_widen_f32 before the MSD kernels."""
    T, A, D = 300, 2101, 1
    lags, want_bp = msd_ref(T, A, D, seed=T + A + D, f32=True)
    c = _lib.Context(0)
    try:
        c.set_option("stage_device_f32", device_f32)
        (view,) = c.stage_alloc(T, A, D, dtype=np.float32)
        view[:] = walk(T, A, D, seed=T + A + D)
        c.stage_commit(0, T)
        c.set_option("timeline", 1)
        for fft, kernel in ((True, "k_msd_prepare"), (False, "k_mid")):
            ts, bp = c.msd(fft, by_particle=True)
            names = timeline(c)
            assert kernel in names and ("k_widen_f32" in names) == bool(device_f32), names
            assert scale_rel_err(bp[lags], want_bp) <= 1e-10, fft
            assert scale_rel_err(ts[lags], want_bp.mean(axis=1)) <= 1e-10, fft
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fft,kernel", [(True, "k_msd_prepare"), (False, "k_direct")])
def test_msd_dev_wide_rows_many_atom_tiles(fft, kernel):
    """ta_msd_dev: a frame-major tensor with ld_row > A D and a by-particle array with ld_bp > A across 24 atom tiles of
    k_bp_transpose / k_helfand_combine_bp and k_row_sums; the padding columns stay untouched."""
    import torch

    T, A, D = 1100, 1501, 3
    ld_row, ld_bp = A * D + 5, A + 7
    lags, want_bp = msd_ref(T, A, D, seed=T + A + D)
    wide = np.full((T, ld_row), 7.5e3)
    wide[:, :A * D] = walk(T, A, D, seed=T + A + D).reshape(T, A * D)
    dev = torch.device("cuda", 0)
    d_x = torch.from_numpy(wide).to(dev)
    c = _lib.Context(0)
    try:
        c.set_option("timeline", 1)
        lag = torch.zeros(T, dtype=torch.float64, device=dev)
        bp = torch.full((T, ld_bp), -1.0, dtype=torch.float64, device=dev)
        c.msd_dev(d_x.data_ptr(), T, A, D, ld_row, fft, lag.data_ptr(), bp.data_ptr(), ld_bp)
        torch.cuda.synchronize()
        assert kernel in timeline(c)
        got = bp.cpu().numpy()
        assert np.all(got[:, A:] == -1.0)
        assert scale_rel_err(got[lags, :A], want_bp) <= 1e-10
        assert scale_rel_err(lag.cpu().numpy()[lags], want_bp.sum(axis=1)) <= 1e-10
        assert np.array_equal(d_x.cpu().numpy(), wide)  # the input is read only
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fft", [True, False])
def test_einstein_msd_class_large(fft):
    T, A, D = 1100, 1501, 3
    lags, want_bp = msd_ref(T, A, D, seed=T + A + D)
    u = ArrayUniverse(positions=walk(T, A, D, seed=T + A + D))
    u.trajectory._pos = np.ascontiguousarray(walk(T, A, D, seed=T + A + D))  # float64 Timesteps
    m = EinsteinMSD(u, msd_type="xyz", fft=fft, stage_dtype=np.float64).run()
    assert scale_rel_err(m.results.msds_by_particle[lags], want_bp) <= 1e-10
    assert scale_rel_err(m.results.timeseries[lags], want_bp.mean(axis=1)) <= 1e-10


# ---------------------------------------------------------------------------------------------- ConductivityHelfand
def cond_groups(T, n_pairs):
    """k_cond_moment's group count (conductivity.hip: cond_moment_parts)."""
    n_tb = (T + 1023) // 1024
    return max(1, min(-(-8 * n_cu() // n_tb), n_pairs, 1024))


# (id, T, A, D, charges, drift): T ends inside a 1024-frame block (1100, 2049, 20000) or on one (2048); every case has
# more column pairs than k_cond_moment groups, so a group sums pairs that land on different dims and atoms
COND_CASES = [
    ("odd_cols_d3", 1100, 1501, 3, "mixed", 0.0),
    ("near_neutral_d3", 1100, 1501, 3, "neutral", 30.0),
    ("d2", 2049, 1100, 2, "mixed", 0.0),
    ("odd_cols_d1", 2048, 2101, 1, "mixed", 0.0),
    # 20 frame blocks: ~8 n_cu / 20 groups over 317 pairs; an FFT plan with an outer radix
    ("long_outer_radix", 20000, 211, 3, "mixed", 0.0),
]


def charges(kind, A, seed):
    return mixed_charges(A, seed) if kind == "mixed" else near_neutral_charges(A, seed)


@functools.lru_cache(maxsize=None)
def cond_ref(T, A, D, kind, drift):
    seed = T + A + D
    x = walk(T, A, D, seed, drift)
    q = charges(kind, A, seed)
    m, s = orc.cond_moment(x, q)
    lags, bp = msd_ref(T, A, D, seed, drift)
    return q, m, s, orc.moment_msd(m), lags, bp @ (q * q)


@pytest.mark.gpu
@pytest.mark.parametrize("fft", [True, False], ids=["fft", "direct"])
@pytest.mark.parametrize("T,A,D,kind,drift", [pytest.param(*c[1:], id=f"{c[0]}-T{c[1]}-A{c[2]}-D{c[3]}") for c in COND_CASES])
def test_conductivity_shapes(T, A, D, kind, drift, fft):
    q, want_m, scale, want_phi, lags, want_self = cond_ref(T, A, D, kind, drift)
    n_pairs = (A * D + 1) // 2
    assert n_pairs > cond_groups(T, n_pairs), "each k_cond_moment group must take several pairs"
    if kind == "neutral":
        assert np.max(np.abs(want_m)) < 0.05 * np.max(scale)  # the moment cancels
    self_kernel = "k_short" if T <= 64 else "k_msd_prepare" if fft else "k_mid" if T <= 512 else "k_direct"
    c = staged_context(walk(T, A, D, T + A + D, drift))
    try:
        runs = []
        for _ in range(2):
            runs.append(c.conductivity(fft, q, self_term=True))
            names = timeline(c)
            assert "k_cond_moment" in names and self_kernel in names, names
        (m, phi, slf), (m2, phi2, slf2) = runs
        assert np.array_equal(m, m2) and np.array_equal(phi, phi2) and np.array_equal(slf, slf2)
        assert np.max(np.abs(m - want_m)) <= 1e-12 * np.max(scale)
        assert phi[0] == 0.0 and slf[0] == 0.0
        assert scale_rel_err(phi, want_phi) <= 1e-10
        assert scale_rel_err(slf[lags], want_self) <= 1e-10
        m3, phi3, none = c.conductivity(fft, q)  # without the weighted slab: the same moment
        assert none is None and np.array_equal(m3, m) and np.array_equal(phi3, phi)
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fft", [True, False], ids=["fft", "direct"])
def test_conductivity_class_large(fft):
    T, A, D = 1100, 1501, 3
    q, want_m, scale, want_phi, lags, want_self = cond_ref(T, A, D, "mixed", 0.0)
    x = walk(T, A, D, T + A + D)
    u = ArrayUniverse(positions=x, charges=q, dimensions=BOX)
    u.trajectory._pos = np.ascontiguousarray(x)  # float64 Timesteps
    cnd = ConductivityHelfand(u.atoms, fft=fft, nernst_einstein=True, stage_dtype=np.float64).run()
    assert np.max(np.abs(cnd.results.moment - want_m)) <= 1e-12 * np.max(scale)
    assert scale_rel_err(cnd.results.timeseries, want_phi) <= 1e-10
    assert scale_rel_err(cnd.results.timeseries_self[lags], want_self) <= 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("fft", [True, False], ids=["fft", "direct"])
def test_group_conductivity_odd_member_slabs(fft):
    """ta_group_conductivity on devices=[0, 0] at 1502 atoms x 3: each member holds 751 atoms, 2253 columns, so both
    slabs end on an unpaired column and the second member starts mid-way (atom 751) through the charges."""
    T, A, D = 1100, 1502, 3
    x = walk(T, A, D, seed=5)
    q = mixed_charges(A, seed=5)
    want_m, scale = orc.cond_moment(x, q)
    c = staged_context(x)
    try:
        one = c.conductivity(fft, q, self_term=True)
    finally:
        c.close()
    g = _lib.Group([0, 0])
    try:
        (views,) = g.stage_alloc(T, A, D)
        assert g.shards == [(0, 751), (751, 1502)]
        for (lo, hi), v in zip(g.shards, views):
            v[:] = x[:, lo:hi]
        g.stage_commit(0, T)
        m, phi, slf = g.conductivity(fft, q, self_term=True)
    finally:
        g.close()
    assert np.max(np.abs(m - one[0])) <= 1e-12 * np.max(scale)
    assert np.max(np.abs(m - want_m)) <= 1e-12 * np.max(scale)
    assert scale_rel_err(phi, one[1]) <= 1e-10
    assert scale_rel_err(slf, one[2]) <= 1e-10
