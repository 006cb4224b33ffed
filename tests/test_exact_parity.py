"""Every correlator per lag and per particle against exact and extended-precision references (oracle/exact.py).

The other parity tests compare an array with its reference at 1e-10 of the array's LARGEST element, so a short lag of a
long MSD or a light particle next to a heavy one is barely checked, and a kernel that lost three digits would pass.
Here every element is held to a bound of its own:

(a) Direct forms on integer-valued inputs, where every sum a kernel forms is exact (oracle.exact.budget): by-particle
    elements within 2 ulps of the correctly rounded quotient (VACF, MSD; Helfand 4: the 1 / D and the scale), lag 0
    exactly 0 for the squared differences, lag sums within (A + 2) u sum_n |bp_n| (/ A: the host calls return the mean
    over particles), the conductivity moment bit-equal to the integer moment.  Each path is forced by its option and
    its kernel asserted from the timeline; frame counts on both sides of 16, 64, 96 / 97, 128, 240 / 256, 272, 512,
    1024 and 2048, and 1 and 2; float32 device slabs ("stage_device_f32"); and shapes from test_msd_cond_shapes.py
    large enough that workgroups loop over atoms.
(b) The same inputs with particle n scaled by 2^s_n, s_n = 0, -12, -24, -36 cycling: each particle's sums stay exact,
    so each by-particle element keeps its own few-ulp bound while its neighbours are 2^24 ... 2^72 larger -- any
    cross-talk between particles, pair halves or shared transforms shows.  (The lag sums then mix scales in one
    accumulator and are not exact: they are checked in (a) and (c).)
(c) Float inputs against a np.longdouble reference, element by element at the lags of orc.lag_sample: the FFT forms
    within [C u log2(L) E + 4 u S1(k)] / (T - k) (oracle.exact.fft_bound, C = 16, L = 2 M of the plan, E the energy of
    every column that shares a transform with the element: oracle.exact.fft_energy_bp), the difference-first direct
    forms within (D (T - k) + 6) u |ref| by particle and (c D (T - k) + A + 6) u |ref| for lag sums (VACF: |ref| the
    windowed sum of |v_i v_{i+k}|), and the matrix-core Helfand forms (the square expanded on centred columns) within
    1e-10 per lag.  The worst ratio per FFT plan is recorded (record_property "fft_ratio").
(d) VelocityAutocorr, ViscosityHelfand, EinsteinMSD and ConductivityHelfand end to end on integer inputs exact in
    float32, through the default float32 staging: the bounds of (a), 6 ulps where a class applies a factor of its own.
(e) Unwrapping on orthorhombic power-of-two boxes (constant and changing per frame) with positions on a 1/64 grid:
    the unwrapped slab and the image counts bit-equal to the walk."""
import functools

import numpy as np
import pytest

from oracle import exact as ex
from oracle import numpy_oracle as orc
from test_unwrap import AXES, SHAPES as UNWRAP_SHAPES, unwrap_slab
from transport_analysis_amd import ConductivityHelfand, EinsteinMSD, VelocityAutocorr, ViscosityHelfand, _lib
from transport_analysis_amd._mini_mda import ArrayUniverse

pytestmark = pytest.mark.gpu
needs_longdouble = pytest.mark.skipif(not ex.longdouble_ok(), reason="np.longdouble has no 64-bit significand here")

U = ex.U
SHORT_T = [1, 2, 15, 16, 17, 63, 64]
MID_T = [65, 96, 97, 127, 128, 129, 240, 241, 255, 256, 257, 271, 272, 273, 511, 512]
LONG_T = [513, 1023, 1024, 1025, 2047, 2048, 2049]
ALL_T = SHORT_T + MID_T + LONG_T
SHIFTS = (0, -12, -24, -36)
MSD_OFFSET = 2.0 ** 30  # positions far from the origin: x^2 + w^2 - 2 x w is not exact there, (x - w)^2 is


def shape(T):
    """(A, D): D = 1, 2, 3 and odd / even particle counts, cycling with T."""
    return 5 + T % 4, 1 + T % 3


def shifts(A):
    return np.array([SHIFTS[n % 4] for n in range(A)])


def timeline(c):
    return [n for n, _ in c.kernel_timeline(64)]


def context(slabs, options):
    """A context with `options` set and `slabs` staged: float32 host and device slabs under "stage_device_f32"."""
    T, A, D = slabs[0].shape
    c = _lib.Context(0)
    for key, val in options.items():
        c.set_option(key, val)
    dtype = np.float32 if options.get("stage_device_f32") else np.float64
    views = c.stage_alloc(T, A, D, n_slabs=len(slabs), dtype=dtype)
    for view, s in zip(views, slabs):
        view[:] = s
    c.stage_commit(0, T)
    c.set_option("timeline", 1)
    return c


# ------------------------------------------------------------------------------------------- (a), (b): integer inputs
@functools.lru_cache(maxsize=None)
def int_inputs(qty, T, A, D):
    """(slabs, masses or None, exact by-particle numerators (T, A), the integer factor of the denominator)."""
    seed = 7 * T + 11 * A + D
    n_terms = A * D * T
    if qty in ("vacf", "vacf32"):
        v = ex.int_velocities(T, A, D, 12 if qty == "vacf32" else 1000, seed)
        ex.budget(v, n_terms, f32=qty == "vacf32")
        return (v,), None, ex.vacf_num(v), 1
    if qty in ("helf", "helf32"):
        f32 = qty == "helf32"
        v = ex.int_velocities(T, A, D, 3 if f32 else 30, seed)
        x = ex.int_velocities(T, A, D, 2, seed + 1) if f32 else ex.int_walk(T, A, D, 2, seed + 1, offset=-20)
        m = ex.int_masses(A, 1, 2 if f32 else 8, seed + 2)
        ex.budget(ex.helfand_product(v, x, m), n_terms, f32=f32)
        return (v, x), m, ex.helfand_num(v, x, m), D
    assert qty in ("msd", "msd32")
    x = ex.int_walk(T, A, D, 7, seed, drift=1, offset=MSD_OFFSET if qty == "msd" else 2.0 ** 20)
    ex.budget(x - x[0], n_terms)
    return (x,), None, ex.msd_num(x), 1


def call(qty, c, masses, by_particle):
    if qty.startswith("vacf_fft"):
        return c.vacf_fft(by_particle=by_particle)
    if qty.startswith("vacf"):
        return c.vacf_direct(by_particle=by_particle)
    if qty.startswith("helf"):
        return c.helfand_msd(masses, 1.0, by_particle=by_particle)
    return c.msd(qty == "msd_fft", by_particle=by_particle)


def check_bp(bp, want, max_ulps, zero_lag0, what):
    """Every element within max_ulps of the correctly rounded value."""
    u = ex.ulps(bp, want)
    worst = np.unravel_index(int(np.argmax(u)), u.shape)
    assert u.max() <= max_ulps, (what, "lag, particle", worst, u.max(), bp[worst], want[worst])
    if zero_lag0:
        assert np.all(bp[0] == 0.0), what


def check_lag_sums(ts, want_bp, A, zero_lag0, what):
    """|ts - mean_n bp_n| <= (A + 2) u sum_n |bp_n| / A at every lag: the rounding of the A per-particle values and of
    any order of their sum and mean, the particle sums themselves being exact."""
    want = want_bp.astype(np.longdouble).sum(axis=1) / A
    bound = (A + 2) * U * np.abs(want_bp).sum(axis=1) / A
    err = np.abs(ts.astype(np.longdouble) - want).astype(np.float64)
    k = int(np.argmax(err - bound))
    assert np.all(err <= bound), (what, "lag", k, err[k], bound[k])
    if zero_lag0:
        assert ts[0] == 0.0, what


# (id, quantity, options, frame counts, kernel)
PATHS = [
    ("vacf-k_short", "vacf", {}, SHORT_T, "k_short"),
    ("vacf-k_mid", "vacf", {"mid_all": 1}, MID_T, "k_mid"),
    ("vacf-k_direct", "vacf", {"direct_mfma": 0}, ALL_T, "k_direct"),
    ("vacf-k_direct-short_max0", "vacf", {"short_max": 0}, SHORT_T, "k_direct"),
    ("vacf-k_band_bp_vacf", "vacf", {"direct_mfma": 3}, ALL_T, "k_band_bp_vacf"),
    ("vacf-f32-k_direct", "vacf32", {"direct_f32": 1, "direct_mfma": 0}, ALL_T, "k_direct"),
    ("vacf_fft-k_short", "vacf_fft", {}, SHORT_T, "k_short"),
    ("helf-k_short", "helf", {}, SHORT_T, "k_short"),
    ("helf-k_mid", "helf", {"mid_all": 1}, MID_T, "k_mid"),
    ("helf-k_direct", "helf", {"direct_mfma": 0}, ALL_T, "k_direct"),
    ("helf-k_band_bp_helf", "helf", {"direct_mfma": 3}, ALL_T, "k_band_bp_helf"),
    ("helf-f32-k_direct", "helf32", {"direct_f32": 1, "direct_mfma": 0}, ALL_T, "k_direct"),
    ("helf-f32-k_band32_tp", "helf32", {"direct_f32": 1, "direct_mfma": 3}, ALL_T, "k_band32_tp"),
    ("msd-k_short", "msd", {}, SHORT_T, "k_short"),
    ("msd-k_mid", "msd", {}, MID_T, "k_mid"),
    ("msd-k_direct", "msd", {"direct_mfma": 0}, ALL_T, "k_direct"),
    ("msd_fft-k_short", "msd_fft", {}, SHORT_T, "k_short"),
    # float32 device slabs: read as they are by the float32 correlators (SrcT = float), widened by k_widen_f32 for the
    # float64 ones
    ("f32slab-vacf-k_direct-f32", "vacf32", {"direct_f32": 1, "direct_mfma": 0, "stage_device_f32": 1}, ALL_T, "k_direct"),
    ("f32slab-vacf-k_band_bp_vacf", "vacf", {"direct_mfma": 3, "stage_device_f32": 1}, ALL_T, "k_band_bp_vacf"),
    ("f32slab-vacf-k_short", "vacf", {"stage_device_f32": 1}, SHORT_T, "k_short"),
    ("f32slab-helf-k_direct-f32", "helf32", {"direct_f32": 1, "direct_mfma": 0, "stage_device_f32": 1}, ALL_T, "k_direct"),
    ("f32slab-helf-k_band32_tp", "helf32", {"direct_f32": 1, "direct_mfma": 3, "stage_device_f32": 1}, ALL_T, "k_band32_tp"),
    ("f32slab-helf-k_band_bp_helf", "helf", {"direct_mfma": 3, "stage_device_f32": 1}, ALL_T, "k_band_bp_helf"),
    ("f32slab-msd-k_mid", "msd32", {"stage_device_f32": 1}, MID_T, "k_mid"),
    ("f32slab-msd-k_direct", "msd32", {"direct_mfma": 0, "stage_device_f32": 1}, ALL_T, "k_direct"),
]

# shapes of test_msd_cond_shapes.py / test_gpu_parity.py whose workgroups loop over atoms: (id, quantity, options, T, A,
# D, kernel)
LOOPING = [
    ("short_loop-msd", "msd", {}, 50, 48001, 3, "k_short"),
    ("short_loop-vacf", "vacf", {}, 50, 48001, 3, "k_short"),
    ("mid_loop-msd", "msd", {}, 300, 5000, 3, "k_mid"),
    ("odd_cols_d3-msd", "msd", {}, 1100, 1501, 3, "k_direct"),
    ("odd_cols_d3-vacf-band", "vacf", {"direct_mfma": 3}, 1100, 1501, 3, "k_band_bp_vacf"),
    ("odd_cols_d1-helf-band", "helf", {"direct_mfma": 3}, 300, 2001, 1, "k_band_bp_helf"),
    ("direct_nwg7-msd", "msd", {"direct_nwg": 7}, 1100, 1100, 2, "k_direct"),
    ("direct_nwg7-vacf", "vacf", {"direct_mfma": 0, "direct_nwg": 7}, 1100, 1100, 2, "k_direct"),
]


def exact_case(qty, options, kernel, T, A, D):
    """One path at one shape, plain and with particle n scaled by 2^s_n: by-particle elements within 2 ulps (Helfand
    4), lag sums of the plain inputs within (A + 2) u sum |bp| / A, the kernel asserted from the timeline."""
    base = qty.replace("32", "").replace("_fft", "")  # vacf, helf, msd
    max_ulps = 4 if base == "helf" else 2
    diff = base != "vacf"
    f32slab = bool(options.get("stage_device_f32"))
    slabs, masses, num, den_d = int_inputs(qty.replace("_fft", ""), T, A, D)
    exact_bp = ex.divide(num, den_d * ex.lag_den(T)[:, None])
    for hetero in (False, True):
        s = shifts(A) if hetero else np.zeros(A, dtype=np.int64)
        scaled = [slabs[0] * np.ldexp(1.0, s)[None, :, None]] + list(slabs[1:])  # Helfand: P is linear in v
        want_bp = exact_bp * np.ldexp(1.0, 2 * s)[None, :]
        what = (qty, kernel, T, A, D, "hetero" if hetero else "plain", options)
        c = context(scaled, options)
        try:
            for by_particle in (True, False):
                ts, bp = call(qty, c, masses, by_particle)
                names = timeline(c)
                # (the FFT VACF's lag sums take k_short up to short_lags_max = 48 frames, an FFT plan beyond)
                lags_exact = not (qty == "vacf_fft" and not by_particle and T > 48)
                if lags_exact:
                    assert kernel in names, (what, by_particle, names)
                    widened = "k_widen_f32" in names
                    assert widened == (f32slab and not options.get("direct_f32")), (what, names)
                if by_particle:
                    check_bp(bp, want_bp, max_ulps, diff, what)
                if not hetero and lags_exact:
                    check_lag_sums(ts, want_bp, A, diff, what + (by_particle,))
        finally:
            c.close()


@pytest.mark.parametrize("qty,options,frames,kernel", [pytest.param(*p[1:], id=p[0]) for p in PATHS])
def test_direct_paths_exact_on_integers(qty, options, frames, kernel):
    for T in frames:
        A, D = shape(T)
        exact_case(qty, options, kernel, T, A, D)


@pytest.mark.parametrize("qty,options,T,A,D,kernel", [pytest.param(*p[1:], id=p[0]) for p in LOOPING])
def test_direct_paths_exact_where_workgroups_loop(qty, options, T, A, D, kernel):
    """Every workgroup takes several atom tiles / column groups (the grid capped by "direct_nwg" for k_direct), with
    neighbouring particles 2^12 ... 2^36 apart in scale."""
    exact_case(qty, options, kernel, T, A, D)


@functools.lru_cache(maxsize=None)
def cond_inputs(T, A, D):
    seed = 5 * T + A + D
    x = ex.int_walk(T, A, D, 5, seed, drift=1, offset=MSD_OFFSET)
    q = ex.int_charges(A, 3, seed + 1)
    M = ex.moment_exact(x, q)
    ex.budget(M, D * T)
    ex.budget(q[None, :, None] * (x - x[0]), A * D * T)
    return x, q, M


@pytest.mark.parametrize("fft", [False, True], ids=["direct", "fft_short"])
def test_conductivity_exact_on_integers(fft):
    """k_cond_moment bit-equal to the integer moment; Phi (the MSD of the moment) and the self term sum_n q_n^2
    MSD_n on their direct paths (fft=True up to 64 frames is k_short as well): Phi within 3 u |Phi| (one particle's
    lag sum), the self term within (A + 2) u of its exact value, lag 0 exactly 0."""
    for T in SHORT_T if fft else ALL_T:
        A, D = shape(T)
        x, q, M = cond_inputs(T, A, D)
        want_phi = ex.divide(ex.phi_num(M), ex.lag_den(T))
        want_self = ex.divide(ex.self_num(x, q), ex.lag_den(T))
        c = context([x], {})
        try:
            m, phi, slf = c.conductivity(fft, q, self_term=True)
            names = timeline(c)
        finally:
            c.close()
        what = (T, A, D, fft)
        assert "k_cond_moment" in names, (what, names)
        if T <= 64:
            assert "k_short" in names, (what, names)
        assert np.array_equal(m, M.astype(np.float64)), what
        assert phi[0] == 0.0 and slf[0] == 0.0, what
        err = np.abs(phi - want_phi)
        assert np.all(err <= 3 * U * want_phi), (what, int(np.argmax(err - 3 * U * want_phi)))
        err = np.abs(slf - want_self)
        assert np.all(err <= (A + 2) * U * want_self), (what, int(np.argmax(err - (A + 2) * U * want_self)))


def test_group_exact_per_quantity():
    """Group([0, 0]): two members on one device, the lag sums reduced inside the library and the by-particle blocks
    copied into one array -- every quantity on integer inputs at the bounds of (a)."""
    T, A, D = 300, 9, 3
    g = _lib.Group([0, 0])
    try:
        for qty in ("vacf", "helf", "msd"):
            slabs, masses, num, den_d = int_inputs(qty, T, A, D)
            views = g.stage_alloc(T, A, D, n_slabs=len(slabs))
            for member_views, s in zip(views, slabs):
                for (lo, hi), view in zip(g.shards, member_views):
                    view[:] = s[:, lo:hi]
            g.stage_commit(0, T)
            want_bp = ex.divide(num, den_d * ex.lag_den(T)[:, None])
            ts, bp = call(qty, g, masses, True)
            check_bp(bp, want_bp, 4 if qty == "helf" else 2, qty != "vacf", ("group", qty))
            check_lag_sums(ts, want_bp, A, qty != "vacf", ("group", qty))
        x, q, M = cond_inputs(T, A, D)
        (views,) = g.stage_alloc(T, A, D)
        for (lo, hi), view in zip(g.shards, views):
            view[:] = x[:, lo:hi]
        g.stage_commit(0, T)
        m, phi, slf = g.conductivity(False, q, self_term=True)
    finally:
        g.close()
    assert np.array_equal(m, M.astype(np.float64))
    want_phi = ex.divide(ex.phi_num(M), ex.lag_den(T))
    want_self = ex.divide(ex.self_num(x, q), ex.lag_den(T))
    assert np.all(np.abs(phi - want_phi) <= 3 * U * want_phi)
    assert np.all(np.abs(slf - want_self) <= (A + 2) * U * want_self)


# ------------------------------------------------------------------------------------------------ (c): float inputs
def hetero(A):
    return np.ldexp(1.0, shifts(A))[None, :, None]


@functools.lru_cache(maxsize=None)
def float_walk(T, A, D, seed):
    """Random walks with a drift, 1e4 away from the origin, particle n scaled by 2^s_n."""
    rng = np.random.default_rng(seed)
    x = 1e4 + np.cumsum(rng.standard_normal((T, A, D)), axis=0) + 0.3 * np.arange(T)[:, None, None]
    x = x * hetero(A)
    x.setflags(write=False)
    return x


def fft_plan_length(T):
    return 2 * _lib.fft_plan_info(T)["M"]


def ratios(got, ref, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (np.abs(got - ref) / bound).astype(np.float64)
    r[bound == 0] = 0.0
    return r


FFT_T = [30, 60, 100, 200, 256, 512, 513, 1000, 2049, 3500, 4600, 7000, 9100, 10000, 10240, 10300]


@functools.lru_cache(maxsize=None)
def vacf_fft_ref(T, A, D, f32=False):
    v = orc.synthetic_velocities(T, A, D, seed=4000 + T) * hetero(A)
    if f32:
        v = v.astype(np.float32).astype(np.float64)
    lags = orc.lag_sample(T)
    ref = ex.ld_corr(v.reshape(T, A * D), lags).reshape(len(lags), A, D).sum(axis=2)
    return v, lags, ref / (T - lags).astype(np.longdouble)[:, None]


@needs_longdouble
@pytest.mark.parametrize("T,f32slab", [(T, False) for T in FFT_T] + [(1000, True), (4600, True), (10240, True)])
def test_vacf_fft_error_model(T, f32slab, record_property):
    """FFT VACF over the plans of test_gpu_parity.SHAPES: the packed short plans (2 / 4 / 8 column pairs in one
    transform; "short_max" 0 keeps k_short out), one pass (256), the wave-local transform (512), first-stage radices
    7, 9, 14, 18, 20, the outer radix (10300); and float32 device slabs ("stage_device_f32"), which the plans without
    an outer radix read as they are (no k_widen_f32)."""
    A, D = shape(T)
    v, lags, ref = vacf_fft_ref(T, A, D, f32slab)
    L = fft_plan_length(T)
    e = ex.column_energy(v).sum(axis=1)
    c = context([v], {"short_max": 0, "stage_device_f32": int(f32slab)})
    try:
        ts, bp = c.vacf_fft(by_particle=True)
        assert "k_short" not in timeline(c) and "k_widen_f32" not in timeline(c), timeline(c)
        ts2, _ = c.vacf_fft(by_particle=False)
        assert "k_short" not in timeline(c) and "k_widen_f32" not in timeline(c), timeline(c)
    finally:
        c.close()
    r_bp = ratios(bp[lags], ref, ex.fft_bound(T, L, ex.fft_energy_bp(e))[lags])
    want_ts = ref.sum(axis=1) / A
    b_ts = ex.fft_bound(T, L, e.sum())[lags] / A
    r_ts = max(ratios(ts[lags], want_ts, b_ts).max(), ratios(ts2[lags], want_ts, b_ts).max())
    record_property("fft_ratio", {"plan": str(_lib.fft_plan_info(T)), "bp": float(r_bp.max()), "ts": float(r_ts)})
    worst = np.unravel_index(int(np.argmax(r_bp)), r_bp.shape)
    assert r_bp.max() <= 1.0, ("by particle: lag", lags[worst[0]], "particle", worst[1], r_bp.max())
    assert r_ts <= 1.0, ("lag sums", r_ts)


MSD_FFT_T = [65, 100, 300, 1100, 2049, 10300]


@needs_longdouble
@pytest.mark.parametrize("T,A,D", [(T,) + shape(T) for T in MSD_FFT_T] + [(1100, 1501, 3)])
def test_msd_fft_error_model(T, A, D, record_property):
    """MSD fft=True (k_msd_prepare: P = x - x[0], S1 - 2 S2) on walks at +1e4 with a drift, per particle and for the
    lag sums; 1100 x 1501 x 3 (odd_cols_d3 of test_msd_cond_shapes.py) has more column pairs than k_msd_prepare has
    workgroups and 24 atom tiles of the by-particle form."""
    x = float_walk(T, A, D, seed=T)
    a = x - x[0]
    lags = orc.lag_sample(T)
    den = (T - lags).astype(np.longdouble)
    ref = ex.ld_sqdiff(x.reshape(T, A * D), lags).reshape(len(lags), A, D).sum(axis=2) / den[:, None]
    L = fft_plan_length(T)
    e = ex.column_energy(a).sum(axis=1)
    S1 = ex.s1_float(a).sum(axis=2)
    c = context([x], {})
    try:
        ts, bp = c.msd(True, by_particle=True)
        assert "k_msd_prepare" in timeline(c)
        ts2, _ = c.msd(True, by_particle=False)
        assert "k_msd_prepare" in timeline(c)
    finally:
        c.close()
    r_bp = ratios(bp[lags], ref, ex.fft_bound(T, L, ex.fft_energy_bp(e), S1)[lags])
    want_ts = ref.sum(axis=1) / A
    b_ts = ex.fft_bound(T, L, e.sum(), S1.sum(axis=1))[lags] / A
    r_ts = max(ratios(ts[lags], want_ts, b_ts).max(), ratios(ts2[lags], want_ts, b_ts).max())
    record_property("fft_ratio", {"plan": str(_lib.fft_plan_info(T)), "bp": float(r_bp.max()), "ts": float(r_ts)})
    assert r_bp.max() <= 1.0, ("by particle", r_bp.max())
    assert r_ts <= 1.0, ("lag sums", r_ts)


@functools.lru_cache(maxsize=None)
def helfand_float(T, A, D):
    rng = np.random.default_rng(T + 17)
    v = rng.standard_normal((T, A, D)) * hetero(A)
    x = float_walk(T, A, D, seed=T + 1) / hetero(A)  # P = (m v) x carries the particle's 2^s_n once
    m = rng.uniform(1.0, 200.0, size=A)
    P = (m[None, :, None] * v) * x
    lags = orc.lag_sample(T)
    ref = ex.ld_sqdiff(P.reshape(T, A * D), lags).reshape(len(lags), A, D).sum(axis=2)
    return v, x, m, P, lags, ref / (D * (T - lags)).astype(np.longdouble)[:, None]


@needs_longdouble
@pytest.mark.parametrize("T", [100, 300, 1100, 2049])
def test_helfand_fft_option_error_model(T, record_property):
    """The "helfand_fft" option (S1 - 2 S2 on P = (m v) x, helfand_fft.hip) with masses 1 ... 200."""
    A, D = shape(T)
    v, x, m, P, lags, ref = helfand_float(T, A, D)
    L = fft_plan_length(T)
    e = ex.column_energy(P).sum(axis=1)
    S1 = ex.s1_float(P).sum(axis=2)
    c = context([v, x], {"helfand_fft": 1})
    try:
        ts, bp = c.helfand_msd(m, 1.0, by_particle=True)
        assert "k_helfand_combine" in timeline(c)
        ts2, _ = c.helfand_msd(m, 1.0, by_particle=False)
        assert "k_helfand_combine" in timeline(c)
    finally:
        c.close()
    r_bp = ratios(bp[lags], ref, ex.fft_bound(T, L, ex.fft_energy_bp(e), S1)[lags] / D)
    want_ts = ref.sum(axis=1) / A
    b_ts = ex.fft_bound(T, L, e.sum(), S1.sum(axis=1))[lags] / (D * A)
    r_ts = max(ratios(ts[lags], want_ts, b_ts).max(), ratios(ts2[lags], want_ts, b_ts).max())
    record_property("fft_ratio", {"plan": str(_lib.fft_plan_info(T)), "bp": float(r_bp.max()), "ts": float(r_ts)})
    assert r_bp.max() <= 1.0, ("by particle", r_bp.max())
    assert r_ts <= 1.0, ("lag sums", r_ts)


@needs_longdouble
@pytest.mark.parametrize("T", [100, 1100])
def test_conductivity_fft_error_model(T, record_property):
    """Phi with fft=True, against the moment the call returned (the bound of the MSD stage alone), and the self term
    (the MSD lag sums of W = q (x - x[0])), charges +-0.1 ... 2; the moment within A u sum_n |q_n (x - x0)|."""
    A, D = shape(T)
    x = float_walk(T, A, D, seed=T + 5) / hetero(A)
    rng = np.random.default_rng(T)
    q = rng.uniform(0.1, 2.0, size=A) * np.where(np.arange(A) % 2, -1.0, 1.0)
    lags = orc.lag_sample(T)
    den = (T - lags).astype(np.longdouble)
    L = fft_plan_length(T)
    c = context([x], {})
    try:
        m, phi, slf = c.conductivity(True, q, self_term=True)
        names = timeline(c)
    finally:
        c.close()
    assert "k_cond_moment" in names and "k_msd_prepare" in names, names
    want_m, scale = orc.cond_moment(x, q)
    assert np.all(np.abs(m - want_m) <= A * U * scale)
    ref_phi = ex.ld_sqdiff(m, lags).sum(axis=1) / den
    r_phi = ratios(phi[lags], ref_phi, ex.fft_bound(T, L, ex.column_energy(m).sum(), ex.s1_float(m).sum(axis=1))[lags])
    W = q[None, :, None] * (x - x[0])
    ref_self = ex.ld_sqdiff(W.reshape(T, A * D), lags).sum(axis=1) / den
    b_self = ex.fft_bound(T, L, ex.column_energy(W).sum(), ex.s1_float(W.reshape(T, A * D)).sum(axis=1))[lags]
    r_self = ratios(slf[lags], ref_self, b_self)
    record_property("fft_ratio", {"plan": str(_lib.fft_plan_info(T)), "phi": float(r_phi.max()),
                                  "self": float(r_self.max())})
    assert r_phi.max() <= 1.0 and r_self.max() <= 1.0, (r_phi.max(), r_self.max())


# (quantity, options, T, kernel, c): c = the most particles whose terms one accumulator takes before it is stored
# ("A": all of them).  k_direct adds an atom's D columns into one accumulator and stores a value per atom; k_mid and
# k_short (above 32 frames the lag-sum accumulators are reset per tile and per block of 32 lags) hold one column's
# terms: c = 1.  k_band_bp_vacf's lag-sum units sum band_bp_helf_block(n_cu, T, A) consecutive particles in the same
# accumulators -- every particle at these few: c = A.
DIFF_PATHS = [
    ("msd", {}, 50, "k_short", 1),
    ("msd", {}, 300, "k_mid", 1),
    ("msd", {}, 1100, "k_direct", 1),
    ("msd", {"direct_mfma": 0}, 200, "k_direct", 1),
    ("helf", {}, 50, "k_short", 1),
    ("helf", {"mid_all": 1}, 300, "k_mid", 1),
    ("helf", {"direct_mfma": 0}, 1100, "k_direct", 1),
    ("vacf", {}, 50, "k_short", 1),
    ("vacf", {"mid_all": 1}, 300, "k_mid", 1),
    ("vacf", {"direct_mfma": 0}, 1100, "k_direct", 1),
    ("vacf", {"direct_mfma": 3}, 1100, "k_band_bp_vacf", "A"),
]


@needs_longdouble
@pytest.mark.parametrize("qty,options,T,kernel,c_acc",
                         [pytest.param(*p, id=f"{p[0]}-{p[3]}-T{p[2]}") for p in DIFF_PATHS])
def test_direct_forms_error_model_on_floats(qty, options, T, kernel, c_acc):
    """Float inputs (walks at +1e4 with a drift, masses 1 ... 200, particles scaled by 2^s_n): every direct form within
    (D (T - k) + 6) u |ref| per particle and (c D (T - k) + A D + 6) u sum_n |ref_n| / A for the lag sums (c from
    DIFF_PATHS; A D: at most that many stored values are added afterwards) -- the rounding of every term that enters
    one accumulator, valid for any order.  A form that expanded the square, or lost the difference, exceeds it at the
    short lags by the ratio of |x|^2 to the squared displacement."""
    A, D = shape(T)
    c_acc = A if c_acc == "A" else c_acc
    lags = orc.lag_sample(T)
    den = (T - lags).astype(np.longdouble)[:, None]
    if qty == "msd":
        x = float_walk(T, A, D, seed=T + 9)
        slabs, masses = [x], None
        ref = ex.ld_sqdiff(x.reshape(T, A * D), lags).reshape(len(lags), A, D).sum(axis=2) / den
        scale = np.abs(ref)
    elif qty == "helf":
        v, x, masses, P, lags, ref = helfand_float(T, A, D)
        slabs = [v, x]
        scale = np.abs(ref)
    else:
        v = orc.synthetic_velocities(T, A, D, seed=T + 3) * hetero(A)
        slabs, masses = [v], None
        ref = ex.ld_corr(v.reshape(T, A * D), lags).reshape(len(lags), A, D).sum(axis=2) / den
        scale = ex.abs_corr(v.reshape(T, A * D), lags).reshape(len(lags), A, D).sum(axis=2) / den.astype(np.float64)
    kk = (T - lags)[:, None].astype(np.float64)
    b_bp = (D * kk + 6) * U * scale
    b_ts = (c_acc * D * kk[:, 0] + A * D + 6) * U * scale.sum(axis=1) / A
    c = context(slabs, options)
    try:
        for by_particle in (True, False):
            ts, bp = call(qty, c, masses, by_particle)
            assert kernel in timeline(c), (kernel, timeline(c))
            if by_particle:
                r = ratios(bp[lags], ref, b_bp)
                worst = np.unravel_index(int(np.argmax(r)), r.shape)
                assert r.max() <= 1.0, ("lag", lags[worst[0]], "particle", worst[1], r.max())
            r = ratios(ts[lags], ref.sum(axis=1) / A, b_ts)
            assert r.max() <= 1.0, ("lag sums", by_particle, "lag", lags[int(np.argmax(r))], r.max())
    finally:
        c.close()


@needs_longdouble
@pytest.mark.parametrize("T", [17, 300, 1100, 2049])
def test_helfand_matrix_cores_per_lag(T):
    """k_band_bp_helf expands the square on columns centred on a nearby frame: within 1e-10 of the np.longdouble
    reference at every lag and particle (not of the array's maximum), on the float data of (c) and on the pure cubic
    trend (v = t, x = t^2 / 2: P = m t^3 / 2 grows by nine orders of magnitude while the lag-1 differences stay
    small)."""
    A, D = shape(T)
    v, x, m, P, lags, ref = helfand_float(T, A, D)
    t = np.arange(T, dtype=np.float64)
    vt = np.repeat(t[:, None, None], 2, axis=1) * np.array([1.0, 0.5])[None, :, None]
    xt = np.repeat((t * t / 2)[:, None, None], 2, axis=1)
    mt = np.array([1.0, 2.0])
    Pt = (mt[None, :, None] * vt) * xt
    ref_t = ex.ld_sqdiff(Pt.reshape(T, 2), lags) / (T - lags).astype(np.longdouble)[:, None]
    for slabs, masses, want in (([v, x], m, ref), ([vt, xt], mt, ref_t)):
        n = slabs[0].shape[1]
        c = context(slabs, {"direct_mfma": 3})
        try:
            for by_particle in (True, False):
                ts, bp = c.helfand_msd(masses, 1.0, by_particle=by_particle)
                assert "k_band_bp_helf" in timeline(c)
                rel_ts = np.abs(ts[lags][1:] - want.sum(axis=1)[1:] / n) / (want.sum(axis=1)[1:] / n)
                assert rel_ts.max() <= 1e-10, ("lag sums", lags[1 + int(np.argmax(rel_ts))], float(rel_ts.max()))
                if by_particle:
                    rel = np.abs(bp[lags][1:] - want[1:]) / want[1:]
                    assert rel.max() <= 1e-10, ("by particle", float(rel.max()))
        finally:
            c.close()


# ------------------------------------------------------------------------------------------------ (d): the classes
@pytest.mark.parametrize("T", [50, 300, 600])
def test_classes_exact_on_integers_through_float32_staging(T):
    """VelocityAutocorr, ViscosityHelfand, EinsteinMSD and ConductivityHelfand (fft=False) on float32 arrays of
    integers, staged as float32 (the default for float32 trajectories): by-particle elements within 2 ulps (VACF,
    MSD) of the correctly rounded quotient, Helfand within 6 ulps of it times the class's factor 1 / (2 kB <V> T_avg),
    lag sums within (A + 2) u sum |bp| / A, the moment bit-equal, Phi and the self term as in
    test_conductivity_exact_on_integers.  50 / 300 / 600 frames take k_short, k_mid or the vector kernel, and the
    matrix-core kernels."""
    A, D, box = 7, 3, 16.0
    dims = [box, box, box, 90, 90, 90]
    (v,), _, vnum, _ = int_inputs("vacf", T, A, D)
    u = ArrayUniverse(positions=np.zeros(v.shape, np.float32), velocities=v.astype(np.float32), masses=np.ones(A),
                      dimensions=dims)
    r = VelocityAutocorr(u.atoms, fft=False).run().results
    want = ex.divide(vnum, ex.lag_den(T)[:, None])
    check_bp(r.vacf_by_particle, want, 2, False, ("VelocityAutocorr", T))
    check_lag_sums(r.timeseries, want, A, False, ("VelocityAutocorr", T))

    (hv, hx), m, hnum, _ = int_inputs("helf", T, A, D)
    u = ArrayUniverse(positions=hx.astype(np.float32), velocities=hv.astype(np.float32), masses=m, dimensions=dims)
    vh = ViscosityHelfand(u.atoms).run()
    scale = 1.0 / (2 * vh.boltzmann * box ** 3 * vh.temp_avg)
    want = ex.divide(hnum, D * ex.lag_den(T)[:, None]) * scale
    check_bp(vh.results.visc_by_particle, want, 6, True, ("ViscosityHelfand", T))
    check_lag_sums(vh.results.timeseries, want, A, True, ("ViscosityHelfand", T))

    (x,), _, mnum, _ = int_inputs("msd32", T, A, D)
    r = EinsteinMSD(ArrayUniverse(positions=x.astype(np.float32)), fft=False).run().results
    want = ex.divide(mnum, ex.lag_den(T)[:, None])
    check_bp(r.msds_by_particle, want, 2, True, ("EinsteinMSD", T))
    check_lag_sums(r.timeseries, want, A, True, ("EinsteinMSD", T))

    q = ex.int_charges(A, 3, seed=T)
    M = ex.moment_exact(x, q)
    r = ConductivityHelfand(ArrayUniverse(positions=x.astype(np.float32), charges=q, dimensions=dims).atoms, fft=False,
                            nernst_einstein=True).run().results
    assert np.array_equal(r.moment, M.astype(np.float64))
    want_phi = ex.divide(ex.phi_num(M), ex.lag_den(T))
    want_self = ex.divide(ex.self_num(x, q), ex.lag_den(T))
    assert r.timeseries[0] == 0.0 and r.timeseries_self[0] == 0.0
    assert np.all(np.abs(r.timeseries - want_phi) <= 3 * U * want_phi), ("Phi", T)
    assert np.all(np.abs(r.timeseries_self - want_self) <= (A + 2) * U * want_self), ("self term", T)


# --------------------------------------------------------------------------------------------- (e): unwrapping
ORTHO_SHAPES = [row for row in UNWRAP_SHAPES if row[3] in ("const", "npt")]


def grid_walk(T, A, kind, seed):
    """(unwrapped u, wrapped x, boxes, image counts n): fractional steps of drift (random sign per column) plus up to
    +-0.15 on a 1/1024 grid (every step below half a box), box lengths 16 / 32 / 64 -- 'npt': each axis doubling and
    halving every 37 frames -- so u = f L(t) and x = (f - floor f) L(t) lie on a 1/64 grid and are exact."""
    rng = np.random.default_rng(seed)
    f0 = rng.integers(0, 1024, size=(1, A, 3))
    steps = rng.choice([-123, 123], size=(1, A, 3)) + rng.integers(-153, 154, size=(max(T - 1, 0), A, 3))
    f = np.concatenate([f0, f0 + np.cumsum(steps, axis=0)]) / 1024.0
    base = np.array([16.0, 32.0, 64.0])
    t = np.arange(T)[:, None]
    L = base * (2.0 ** (((t // 37) + np.arange(3)) % 2) if kind == "npt" else np.ones((T, 1)))
    dims = np.concatenate([L, np.full((T, 3), 90.0)], axis=1)
    n = np.floor(f)
    return f * L[:, None, :], (f - n) * L[:, None, :], dims, n


@pytest.mark.parametrize("T,A,D,kind", ORTHO_SHAPES)
def test_unwrap_exact_on_a_grid(T, A, D, kind):
    """k_unwrap_ortho at the orthorhombic rows of test_unwrap.SHAPES: the unwrapped slab bit-equal to the walk and the
    image counts exact."""
    u, x, dims, n = grid_walk(T, A, kind, seed=T + A)
    ax = AXES[D]
    x, u, n = x[:, :, ax], u[:, :, ax], n[:, :, ax]
    got, names = unwrap_slab("hip", x, dims, ax, timeline=True)
    assert "k_unwrap_ortho" in names, names
    assert np.array_equal(got, u), np.max(np.abs(got - u))
    full = np.zeros((T, A, 3))
    full[:, :, ax] = x - got
    counts = np.rint(full / dims[:, None, :3])[:, :, ax]
    assert np.array_equal(counts, -n)
