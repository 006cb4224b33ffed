"""EinsteinMSD (MDAnalysis.analysis.msd.EinsteinMSD) and the ta_msd* entry points: closed forms, the reference's
Einstein-against-Green-Kubo check, random-walk parity with a NumPy restatement on every dispatch path, the raw C-ABI,
several devices and torch.distributed.  Every class-level test runs on the library's CPU backend and, marked gpu, on
the HIP path."""
import ctypes
import os

import numpy as np
import pytest
from scipy.stats import linregress

from conftest import scale_rel_err
from transport_analysis_amd import EinsteinMSD, VelocityAutocorr, _lib
from transport_analysis_amd._base import NoDataError
from transport_analysis_amd._mini_mda import ArrayUniverse

NSTEP = 5001
DIMS = [("xyz", [0, 1, 2]), ("xy", [0, 1]), ("xz", [0, 2]), ("yz", [1, 2]), ("x", [0]), ("y", [1]), ("z", [2])]
TA_E_INVALID, TA_E_STATE, TA_E_UNSUPPORTED = -1, -4, -5


@pytest.fixture(params=["cpu", pytest.param("hip", marks=pytest.mark.gpu)])
def backend(request, monkeypatch):
    if request.param == "cpu":
        monkeypatch.setenv("TA_AMD_DEVICE", "cpu")  # the library's opt-in CPU backend behind the same C symbols
    else:
        monkeypatch.delenv("TA_AMD_DEVICE", raising=False)
        assert _lib.device_count() >= 1
    return request.param


def msd_direct(x):
    """NumPy restatement of MDAnalysis' windowed form: (n_frames, n_atoms) by particle, row 0 zero."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    out = np.zeros((T, x.shape[1]))
    for k in range(1, T):
        d = x[k:] - x[:-k]
        out[k] = (d * d).sum(axis=2).mean(axis=0)
    return out


def float64_universe(x):
    """An in-memory universe whose Timesteps hand out float64 positions (an MDAnalysis MemoryReader can hold
    float64 too): the closed forms below are not exact in float32."""
    u = ArrayUniverse(positions=x)
    u.trajectory._pos = np.ascontiguousarray(x, dtype=np.float64)
    return u


def closed_form(frames, dim_fac):
    """MSD of x = t^2 / 2 on every axis sampled at `frames` (equally spaced, spacing s, first f0):
    x[j + k] - x[j] = s k (f0 + s j) + s^2 k^2 / 2, so MSD(k) = dim_fac mean_{j < n - k} (a + b j)^2 with
    a = s k f0 + s^2 k^2 / 2, b = s^2 k: sums of powers in closed form."""
    n = len(frames)
    f0 = float(frames[0])
    s = float(frames[1] - frames[0]) if n > 1 else 1.0
    out = np.zeros(n)
    for k in range(1, n):
        m = n - k
        a, b = s * k * f0 + s * s * k * k / 2.0, s * s * k
        s1, s2 = m * (m - 1) / 2.0, (m - 1) * m * (2 * m - 1) / 6.0
        out[k] = dim_fac * (a * a + 2 * a * b * s1 / m + b * b * s2 / m)
    return out


@pytest.fixture(scope="module")
def step_traj():
    t = np.arange(NSTEP, dtype=np.float64)
    x = np.repeat((t * t / 2)[:, None, None], 3, axis=2)
    return float64_universe(x)


# ------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("fft", [True, False])
@pytest.mark.parametrize("msd_type,cols", DIMS)
def test_closed_form_step_trajectory(backend, step_traj, msd_type, cols, fft):
    m = EinsteinMSD(step_traj, select="all", msd_type=msd_type, fft=fft, stage_dtype=np.float64).run()
    want = closed_form(np.arange(NSTEP), len(cols))
    assert m.results.timeseries[0] == 0.0
    assert scale_rel_err(m.results.timeseries, want) <= 1e-10
    assert scale_rel_err(m.results.msds_by_particle[:, 0], want) <= 1e-10
    assert m.results.msds_by_particle.shape == (NSTEP, 1)


@pytest.mark.parametrize("fft", [True, False])
@pytest.mark.parametrize("msd_type,cols", DIMS)
def test_closed_form_start_stop_step(backend, step_traj, msd_type, cols, fft):
    m = EinsteinMSD(step_traj, msd_type=msd_type, fft=fft, stage_dtype=np.float64).run(start=10, stop=1000, step=10)
    want = closed_form(np.arange(10, 1000, 10), len(cols))
    assert m.n_frames == 99
    assert scale_rel_err(m.results.timeseries, want) <= 1e-10


# ------------------------------------------------------------ Einstein against Green-Kubo
@pytest.mark.parametrize("msd_type,cols", DIMS)
def test_self_diffusivity_msd_all_dims(backend, msd_type, cols):
    """The reference's test_velocityautocorr.py::test_self_diffusivity_msd_all_dims: the Green-Kubo integral of
    the VACF of v = t against the Einstein slope of the MSD of x = t^2 / 2 over lags 3000 ... 5000."""
    t = np.arange(NSTEP, dtype=np.float64)
    v = np.repeat(t[:, None, None], 3, axis=2)
    x = np.repeat((t * t / 2)[:, None, None], 3, axis=2)
    u = ArrayUniverse(positions=x, velocities=v, masses=[16.0], dimensions=[2, 2, 2, 90, 90, 90])
    sd_actual = VelocityAutocorr(u.atoms, dim_type=msd_type, fft=True).run().self_diffusivity_gk()
    m = EinsteinMSD(u, select="all", msd_type=msd_type).run()
    lagtimes = np.arange(m.n_frames)
    fit = linregress(lagtimes[3000:5000], m.results.timeseries[3000:5000])
    sd_expected = fit.slope / (2 * len(cols))
    np.testing.assert_approx_equal(sd_actual, sd_expected, significant=2)


# -------------------------------------------------------- random walks, every dispatch path
# frame counts that land on every path: k_short (<= 64), the FFT form (65 ... 10240 one on-chip transform, 10300 an
# outer radix), and for fft=False k_mid (65 ... 512) and k_direct (513 and more)
WALK_FRAMES = [(2, 7), (17, 9), (64, 11), (65, 5), (100, 7), (128, 3), (300, 5), (513, 3), (1000, 3), (10300, 3)]


def random_walk(T, A, seed):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.standard_normal((T, A, 3)), axis=0) + 1000.0  # far from the origin, like unwrapped positions


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T,A", WALK_FRAMES)
def test_random_walk_parity(backend, T, A, dtype):
    x = random_walk(T, A, seed=T + A)
    if dtype == np.float32:
        u = ArrayUniverse(positions=x)  # float32 Timesteps, as MDAnalysis hands them out
        xs = x.astype(np.float32).astype(np.float64)
    else:
        u, xs = float64_universe(x), x
    kw = {"stage_dtype": dtype}
    for msd_type, cols in (("xyz", [0, 1, 2]), ("xz", [0, 2]), ("y", [1])):
        want_bp = msd_direct(xs[:, :, cols])
        want_ts = want_bp.mean(axis=1)
        for fft in (True, False):
            m = EinsteinMSD(u, msd_type=msd_type, fft=fft, **kw).run()
            assert m.results.msds_by_particle.shape == (T, A)
            assert scale_rel_err(m.results.msds_by_particle, want_bp) <= 1e-10, (msd_type, fft)
            assert scale_rel_err(m.results.timeseries, want_ts) <= 1e-10, (msd_type, fft)
            lags = EinsteinMSD(u, msd_type=msd_type, fft=fft, by_particle=False, **kw).run()
            assert lags.results.msds_by_particle is None
            assert scale_rel_err(lags.results.timeseries, want_ts) <= 1e-10, (msd_type, fft)


def test_selection_atomgroup_and_restaging(backend):
    x = random_walk(150, 9, seed=3)
    u = ArrayUniverse(positions=x)
    xs = x.astype(np.float32).astype(np.float64)
    m = EinsteinMSD(u, select="index 2:6", msd_type="XY", fft=True)
    assert (m.n_particles, m.msd_type, m.dim_fac, m.select, m.fft) == (5, "xy", 2, "index 2:6", True)
    assert m.results.timeseries is None and m.results.msds_by_particle is None  # before run, as MDAnalysis
    m.run()
    want = msd_direct(xs[:, 2:7, :2])
    assert scale_rel_err(m.results.msds_by_particle, want) <= 1e-10
    m.run(start=20, stop=140, step=3)  # a second run restages
    want = msd_direct(xs[20:140:3, 2:7, :2])
    assert m.results.msds_by_particle.shape == want.shape
    assert scale_rel_err(m.results.msds_by_particle, want) <= 1e-10
    ag = EinsteinMSD(u.atoms[1:4], fft=False).run(frames=[0, 5, 9, 30, 31, 100])  # an AtomGroup as `u`
    assert scale_rel_err(ag.results.msds_by_particle, msd_direct(xs[[0, 5, 9, 30, 31, 100], 1:4])) <= 1e-10


# -------------------------------------------------------------------------- API errors
def test_api_errors(backend):
    x = random_walk(10, 2, seed=1)
    with pytest.raises(ValueError, match="invalid msd_type: foo specified"):
        EinsteinMSD(ArrayUniverse(positions=x), msd_type="foo")
    with pytest.raises(ValueError, match="invalid msd_type"):
        EinsteinMSD(ArrayUniverse(positions=x), msd_type="yx")
    no_pos = ArrayUniverse(velocities=x)
    no_pos.trajectory._pos = None
    with pytest.raises(NoDataError):
        EinsteinMSD(no_pos).run()
    m = EinsteinMSD(ArrayUniverse(positions=x))
    assert m.results.timeseries is None
    with pytest.raises(AttributeError):
        m.results.no_such_result
    with pytest.raises(ValueError, match="exclusive"):
        EinsteinMSD(ArrayUniverse(positions=x), devices=[0], distributed=True)


def test_cpu_context_argument_checks():
    """ta_msd on the CPU backend: fft must be 0 or 1, slabs must be staged, device entry points are unsupported."""
    L = _lib.lib()
    c = _lib.Context("cpu")
    ts = np.zeros(8)
    assert L.ta_msd(c._h, 0, _lib._ptr(ts), None) == TA_E_STATE
    (view,) = c.stage_alloc(8, 3, 2)
    view[:] = random_walk(8, 3, seed=2)[:, :, :2]
    c.stage_commit(0, 8)
    assert L.ta_msd(c._h, 2, _lib._ptr(ts), None) == TA_E_INVALID
    assert L.ta_msd(c._h, -1, _lib._ptr(ts), None) == TA_E_INVALID
    assert L.ta_msd(c._h, 1, None, None) == TA_E_INVALID
    assert L.ta_msd(None, 1, _lib._ptr(ts), None) == TA_E_INVALID
    assert L.ta_msd_staged(c._h, 1, ctypes.c_void_p(16), None, 0, None) == TA_E_UNSUPPORTED
    assert L.ta_msd_dev(c._h, ctypes.c_void_p(16), 8, 3, 2, 6, 1, ctypes.c_void_p(16), None, 0, None) == TA_E_UNSUPPORTED
    assert L.ta_group_msd(None, 1, _lib._ptr(ts), None) == TA_E_INVALID
    ts, bp = c.msd(True, by_particle=True)
    assert scale_rel_err(bp, msd_direct(view)) <= 1e-12
    c.close()


# ------------------------------------------------------------------------- raw C-ABI (GPU)
@pytest.mark.gpu
def test_msd_dev_frame_major_wide_rows():
    """ta_msd_dev on a frame-major device tensor whose row pitch is wider than n_atoms * dim, by-particle output
    with ld_bp > n_atoms, both forms; then the argument checks."""
    import torch

    T, A, D, ld_row, ld_bp = 300, 13, 3, 13 * 3 + 7, 13 + 5
    x = random_walk(T, A, seed=4)
    wide = np.full((T, ld_row), 7.5e3)
    wide[:, :A * D] = x.reshape(T, A * D)
    want_bp = msd_direct(x)
    dev = torch.device("cuda", 0)
    d_x = torch.from_numpy(wide).to(dev)
    c = _lib.Context(0)
    for fft in (1, 0):
        lag = torch.zeros(T, dtype=torch.float64, device=dev)
        bp = torch.full((T, ld_bp), -1.0, dtype=torch.float64, device=dev)
        c.msd_dev(d_x.data_ptr(), T, A, D, ld_row, fft, lag.data_ptr(), bp.data_ptr(), ld_bp)
        torch.cuda.synchronize()
        got = bp.cpu().numpy()
        assert scale_rel_err(got[:, :A], want_bp) <= 1e-10
        assert np.all(got[:, A:] == -1.0)  # the padding columns are not written
        assert scale_rel_err(lag.cpu().numpy(), want_bp.sum(axis=1)) <= 1e-10
        lag2 = torch.zeros(T, dtype=torch.float64, device=dev)  # lag sums alone
        c.msd_dev(d_x.data_ptr(), T, A, D, ld_row, fft, lag2.data_ptr())
        torch.cuda.synchronize()
        assert scale_rel_err(lag2.cpu().numpy(), want_bp.sum(axis=1)) <= 1e-10
    L = _lib.lib()
    p, q = ctypes.c_void_p(d_x.data_ptr()), ctypes.c_void_p(lag.data_ptr())
    assert L.ta_msd_dev(c._h, p, T, A, 4, ld_row, 1, q, None, 0, None) == TA_E_INVALID  # dim
    assert L.ta_msd_dev(c._h, p, T, A, D, A * D - 1, 1, q, None, 0, None) == TA_E_INVALID  # ld_row
    assert L.ta_msd_dev(c._h, p, 0, A, D, ld_row, 1, q, None, 0, None) == TA_E_INVALID  # n_frames
    assert L.ta_msd_dev(c._h, None, T, A, D, ld_row, 1, q, None, 0, None) == TA_E_INVALID
    assert L.ta_msd_dev(c._h, p, T, A, D, ld_row, 1, None, None, 0, None) == TA_E_INVALID
    assert L.ta_msd_dev(c._h, p, T, A, D, ld_row, 1, q, ctypes.c_void_p(bp.data_ptr()), A - 1, None) == TA_E_INVALID
    assert L.ta_msd_dev(c._h, p, T, A, D, ld_row, 3, q, None, 0, None) == TA_E_INVALID  # fft
    c.close()


@pytest.mark.gpu
def test_msd_staged_caller_buffers_and_timeline():
    import torch

    T, A, D, ld_bp = 700, 9, 2, 9 + 4
    x = random_walk(T, A, seed=6)[:, :, :D]
    want_bp = msd_direct(x)
    dev = torch.device("cuda", 0)
    c = _lib.Context(0)
    assert _lib.lib().ta_msd_staged(c._h, 1, ctypes.c_void_p(16), None, 0, None) == TA_E_STATE  # nothing staged
    (view,) = c.stage_alloc(T, A, D, dtype=np.float32)
    view[:] = x
    c.stage_commit(0, T)
    want_bp = msd_direct(view.astype(np.float64))
    c.set_option("timeline", 1)
    for fft in (True, False):
        lag = torch.zeros(T, dtype=torch.float64, device=dev)
        bp = torch.full((T, ld_bp), -1.0, dtype=torch.float64, device=dev)
        c.msd_staged(fft, lag.data_ptr(), bp.data_ptr(), ld_bp)
        torch.cuda.synchronize()
        got = bp.cpu().numpy()
        assert scale_rel_err(got[:, :A], want_bp) <= 1e-10
        assert np.all(got[:, A:] == -1.0)
        assert scale_rel_err(lag.cpu().numpy(), want_bp.sum(axis=1)) <= 1e-10
        names = [n for n, _ in c.kernel_timeline()]
        assert ("k_msd_prepare" in names) == fft, names
        assert ("k_direct" in names) == (not fft), names
    hist = c.timing_history()
    assert len(hist) >= 2 and all(t > 0 for t, _ in hist[-2:])
    L = _lib.lib()
    q = ctypes.c_void_p(lag.data_ptr())
    assert L.ta_msd_staged(c._h, 2, q, None, 0, None) == TA_E_INVALID
    assert L.ta_msd_staged(c._h, 1, None, None, 0, None) == TA_E_INVALID
    assert L.ta_msd_staged(c._h, 1, q, ctypes.c_void_p(bp.data_ptr()), A - 1, None) == TA_E_INVALID
    c.close()


# ------------------------------------------------------------- several devices, distributed
@pytest.mark.gpu
@pytest.mark.parametrize("fft", [True, False])
def test_devices_two_members_one_gpu(fft):
    x = random_walk(400, 11, seed=8)
    u = ArrayUniverse(positions=x)
    one = EinsteinMSD(u, fft=fft).run()
    two = EinsteinMSD(u, fft=fft, devices=[0, 0]).run()
    assert two.results.device_ranges == [(0, 5), (5, 11)]
    assert scale_rel_err(two.results.timeseries, one.results.timeseries) <= 1e-13
    assert scale_rel_err(two.results.msds_by_particle, one.results.msds_by_particle) <= 1e-13
    lags = EinsteinMSD(u, fft=fft, devices=[0, 0], by_particle=False).run()
    assert scale_rel_err(lags.results.timeseries, one.results.timeseries) <= 1e-13


def _msd_worker(rank, world, port, T, A, out_dir):
    import sys

    import torch.distributed as dist

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from transport_analysis_amd import EinsteinMSD
    from transport_analysis_amd._mini_mda import ArrayUniverse

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    u = ArrayUniverse(positions=random_walk(T, A, seed=12))
    out = {}
    for fft in (True, False):
        m = EinsteinMSD(u, msd_type="xz", fft=fft, distributed=True, device="cpu").run()
        out[f"ts_{int(fft)}"] = m.results.timeseries
        out[f"bp_{int(fft)}"] = m.results.msds_by_particle
        out["range"] = np.array(m.results.particle_range)
    np.savez(os.path.join(out_dir, f"msd_{rank}.npz"), **out)
    dist.destroy_process_group()


@pytest.mark.parametrize("A", [7, 1])
def test_distributed_gloo_world2_cpu_backend(tmp_path, A):
    import torch.multiprocessing as mp

    T, world = 90, 2
    port = 33600 + (os.getpid() % 2000) + A
    mp.spawn(_msd_worker, args=(world, port, T, A, str(tmp_path)), nprocs=world, join=True)
    u = ArrayUniverse(positions=random_walk(T, A, seed=12))
    for fft in (True, False):
        serial = EinsteinMSD(u, msd_type="xz", fft=fft, device="cpu").run()
        for r in range(world):
            z = np.load(tmp_path / f"msd_{r}.npz", allow_pickle=True)
            lo, hi = z["range"]
            assert (lo, hi) == ((A * r) // world, (A * (r + 1)) // world)
            assert scale_rel_err(z[f"ts_{int(fft)}"], serial.results.timeseries) <= 1e-13
            if hi > lo:
                assert scale_rel_err(z[f"bp_{int(fft)}"], serial.results.msds_by_particle[:, lo:hi]) <= 1e-13
            else:
                assert z[f"bp_{int(fft)}"].shape == (T, 0)
