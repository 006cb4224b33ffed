"""Periodic unwrapping (ta_unwrap, Context.unwrap / Group.unwrap, EinsteinMSD / ConductivityHelfand(unwrap=True)).

Ground truth: an unwrapped random walk built in fractional coordinates (frame 0 inside the box, steps <= 0.3 of a box,
with a drift that carries image counts to +-50 and beyond across many 256-frame scan chunks), wrapped with
(f - floor f) H(t); the unwrapped slab must give the walk back and the image counts exactly.  NoJump parity against a
literal NumPy restatement of MDAnalysis' NoJump loop and its triclinic_vectors.  The classes on wrapped input with
unwrap=True against the same classes on the unwrapped input.  Shapes that reach every branch of k_unwrap_ortho and
k_unwrap_tric, properties (bit-identical repeats, idempotence, several devices, torch.distributed) and errors.  Every
case that takes a `backend` runs on the library's CPU backend and, marked gpu, on the HIP path."""
import ctypes
import os
import warnings

import numpy as np
import pytest

from conftest import scale_rel_err
from transport_analysis_amd import ConductivityHelfand, EinsteinMSD, _lib
from transport_analysis_amd._mini_mda import ArrayUniverse

TA_E_INVALID, TA_E_STATE, TA_E_UNSUPPORTED = -1, -4, -5
DIMS = [("xyz", [0, 1, 2]), ("xy", [0, 1]), ("xz", [0, 2]), ("yz", [1, 2]), ("x", [0]), ("y", [1]), ("z", [2])]


@pytest.fixture(params=["cpu", pytest.param("hip", marks=pytest.mark.gpu)])
def backend(request, monkeypatch):
    if request.param == "cpu":
        monkeypatch.setenv("TA_AMD_DEVICE", "cpu")  # the library's opt-in CPU backend behind the same C symbols
    else:
        monkeypatch.delenv("TA_AMD_DEVICE", raising=False)
        assert _lib.device_count() >= 1
    return request.param


# ------------------------------------------------------------------- NumPy restatement of MDAnalysis' NoJump
def triclinic_vectors(dimensions):
    """MDAnalysis.lib.mdamath.triclinic_vectors in float64: rows = box vectors; zeros for an invalid box."""
    dim = np.asarray(dimensions, dtype=np.float64)
    lx, ly, lz, alpha, beta, gamma = dim
    if not (np.all(dim > 0.0) and alpha < 180.0 and beta < 180.0 and gamma < 180.0):
        return np.zeros((3, 3))
    if alpha == beta == gamma == 90.0:
        return np.diag(dim[:3])
    box = np.zeros((3, 3))
    box[0, 0] = lx
    cos_alpha = 0.0 if alpha == 90.0 else np.cos(np.deg2rad(alpha))
    cos_beta = 0.0 if beta == 90.0 else np.cos(np.deg2rad(beta))
    if gamma == 90.0:
        cos_gamma, sin_gamma = 0.0, 1.0
    else:
        cos_gamma, sin_gamma = np.cos(np.deg2rad(gamma)), np.sin(np.deg2rad(gamma))
    box[1, 0] = ly * cos_gamma
    box[1, 1] = ly * sin_gamma
    box[2, 0] = lz * cos_beta
    box[2, 1] = lz * (cos_alpha - cos_beta * cos_gamma) / sin_gamma
    with np.errstate(invalid="ignore"):  # (NaN for angles that make no box: rejected below)
        box[2, 2] = np.sqrt(lz * lz - box[2, 0] ** 2 - box[2, 1] ** 2)
    return box if box[2, 2] > 0.0 else np.zeros((3, 3))


def nojump(x, dims):
    """MDAnalysis.transformations.nojump.NoJump._transform over the frames of x (T, A, 3), literally."""
    out = np.empty_like(x)
    prev = None
    for t in range(x.shape[0]):
        L = triclinic_vectors(dims[t])
        Linverse = np.linalg.inv(L)
        if prev is None:
            prev = x[t] @ Linverse
            out[t] = x[t]
            continue
        fcurrent = x[t] @ Linverse
        newpositions = fcurrent - np.round(fcurrent - prev)
        out[t] = newpositions @ L
        prev = newpositions
    return out


# -------------------------------------------------------------------------------------------------- inputs
def box_table(kind, T, seed=0, base=(20.0, 24.0, 28.0)):
    """(T, 6) boxes: 'const' orthorhombic, 'npt' orthorhombic +-3 % per frame, 'tric' constant triclinic,
    'tric_npt' triclinic with per-frame lengths and angles."""
    rng = np.random.default_rng(seed + 100)
    d = np.tile(np.array([*base, 90.0, 90.0, 90.0]), (T, 1))
    if kind in ("tric", "tric_npt"):
        d[:, 3:] = [70.0, 80.0, 65.0]
    if kind in ("npt", "tric_npt"):
        d[:, :3] *= 1.0 + 0.03 * np.sin(np.arange(T)[:, None] * 0.05 + rng.uniform(0, 6, 3))
    if kind == "tric_npt":
        d[:, 3:] += 2.0 * np.sin(np.arange(T)[:, None] * 0.03 + rng.uniform(0, 6, 3))
    return d


def fractional_walk(T, A, seed, drift=0.12):
    """Unwrapped fractional coordinates: frame 0 inside the box, then steps of drift (random sign per column) plus
    U(-0.15, 0.15): every step <= 0.27 of a box, image counts ~ drift * T."""
    rng = np.random.default_rng(seed)
    f0 = rng.uniform(0.0, 1.0, (1, A, 3))
    steps = rng.choice([-drift, drift], size=(1, A, 3)) + rng.uniform(-0.15, 0.15, (T - 1, A, 3))
    return np.concatenate([f0, f0 + np.cumsum(steps, axis=0)]) if T > 1 else f0


def wrapped_case(T, A, kind, seed):
    """(unwrapped u, wrapped x, boxes, image counts) in float64, (T, A, 3)."""
    dims = box_table(kind, T, seed)
    H = np.stack([triclinic_vectors(d) for d in dims])
    fu = fractional_walk(T, A, seed)
    u = np.einsum("tad,tde->tae", fu, H)
    x = np.einsum("tad,tde->tae", fu - np.floor(fu), H)
    return u, x, dims, np.floor(fu)


def open_ctx(backend):
    return _lib.Context("cpu" if backend == "cpu" else 0)


def read_slab(ctx, backend, slab, T, A, D, host):
    """The staged slab as (T, A, D) float64: the host slab on the CPU backend, a device read-back on the GPU."""
    if backend == "cpu":
        return np.array(host, dtype=np.float64)
    import torch

    out = torch.empty((T, A * D), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ctx.stage_read_dev(slab, out.data_ptr(), A * D, st)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(T, A, D)


def unwrap_slab(backend, x, dims, axes, timeline=False):
    """Stage x (T, A, D) float64, unwrap it, return (result, kernel names of the call or None)."""
    T, A, D = x.shape
    ctx = open_ctx(backend)
    if timeline and backend != "cpu":
        ctx.set_option("timeline", 1)
    (h,) = ctx.stage_alloc(T, A, D)
    h[...] = x
    ctx.stage_commit(0, T)
    ctx.unwrap(0, dims, axes)
    names = [n for n, _ in ctx.kernel_timeline()] if timeline and backend != "cpu" else None
    out = read_slab(ctx, backend, 0, T, A, D, h)
    ctx.close()
    return out, names


def image_counts(x, xu, dims):
    """n(t) of x_u = x - n H: rint((x - x_u) H^-1)"""
    Hinv = np.stack([np.linalg.inv(triclinic_vectors(d)) for d in dims])
    return np.rint(np.einsum("tad,tde->tae", x - xu, Hinv))


# -------------------------------------------------------------------------------------------- ground truth
@pytest.mark.parametrize("kind", ["const", "npt", "tric", "tric_npt"])
def test_ground_truth_random_walk(backend, kind):
    T, A = 520, 7
    u, x, dims, n = wrapped_case(T, A, kind, seed=3)
    assert np.abs(n).max() >= 50  # image counts reach +-50: many scan chunks carry a count
    got, _ = unwrap_slab(backend, x, dims, [0, 1, 2])
    L = dims[:, :3].max()
    assert np.max(np.abs(got - u)) <= 1e-12 * L
    assert np.array_equal(got[0], x[0])  # frame 0 keeps its bits
    assert np.array_equal(image_counts(x, got, dims), -n)  # x = x_u + n H with n = -floor(f_u)


def test_triclinic_vectors_known_boxes():
    """The restatement above (and through it the library's float64 box) on boxes with known vectors."""
    assert np.array_equal(triclinic_vectors([10, 20, 30, 90, 90, 90]), np.diag([10.0, 20.0, 30.0]))
    a = 12.0
    want = np.array([[a, 0, 0], [0, a, 0], [a / 2, a / 2, a / np.sqrt(2)]])
    assert np.allclose(triclinic_vectors([a, a, a, 60, 60, 90]), want, rtol=0, atol=1e-13)
    # a hexagonal cell: gamma = 120
    want = np.array([[a, 0, 0], [-a / 2, a * np.sqrt(3) / 2, 0], [0, 0, 7.0]])
    assert np.allclose(triclinic_vectors([a, a, 7.0, 90, 90, 120]), want, rtol=0, atol=1e-13)
    assert not triclinic_vectors([a, a, a, 10, 10, 150]).any()  # angles that make no box


@pytest.mark.parametrize("kind", ["const", "npt", "tric", "tric_npt"])
def test_nojump_parity(backend, kind):
    """Against NoJump itself on input that is not in the box at frame 0 and whose images jump by several boxes at
    once between frames (positions written with arbitrary image offsets)."""
    T, A = 300, 6
    u, x, dims, _ = wrapped_case(T, A, kind, seed=5)
    rng = np.random.default_rng(7)
    H = np.stack([triclinic_vectors(d) for d in dims])
    shift = rng.integers(-3, 4, size=(T, A, 3)).astype(np.float64)
    shift[0] = rng.integers(2, 5, size=(A, 3))  # frame 0 outside the box
    x = x + np.einsum("tad,tde->tae", shift, H)
    want = nojump(x, dims)
    got, _ = unwrap_slab(backend, x, dims, [0, 1, 2])
    assert np.max(np.abs(got - want)) <= 1e-12 * dims[:, :3].max()
    assert np.array_equal(got[0], x[0])
    # NoJump's unwrapped trajectory is the walk shifted by frame 0's image
    assert np.max(np.abs(got - (u + np.einsum("ad,tde->tae", shift[0], H)))) <= 1e-12 * dims[:, :3].max()


# --------------------------------------------------------------------------------------------------- classes
def grid_case(T, A, seed):
    """Positions exact in float32 (a 1/64 grid, power-of-two box lengths), so wrapped and unwrapped inputs stage the
    same values: (unwrapped, wrapped, dimensions)."""
    rng = np.random.default_rng(seed)
    L = np.array([16.0, 32.0, 8.0])
    k0 = rng.integers(0, 64 * 8, size=(1, A, 3))
    steps = rng.choice([-1, 1], size=(1, A, 3)) * 48 + rng.integers(-40, 41, size=(T - 1, A, 3))  # <= 88/512 of a box
    k = np.concatenate([k0, k0 + np.cumsum(steps, axis=0)])
    u = k / 64.0 * (L / 8.0)
    x = u - np.floor(u / L) * L
    return u, x, [*L, 90.0, 90.0, 90.0]


@pytest.mark.parametrize("fft", [True, False])
@pytest.mark.parametrize("stage_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("msd_type", [d for d, _ in DIMS])
def test_einstein_msd_wrapped_equals_unwrapped(backend, fft, stage_dtype, msd_type):
    u, x, box = grid_case(330, 9, seed=11)
    assert np.abs(np.floor(u / np.array(box[:3]))).max() >= 30
    kw = dict(msd_type=msd_type, fft=fft, stage_dtype=stage_dtype)
    want = EinsteinMSD(ArrayUniverse(positions=u, dimensions=box), **kw).run()
    got = EinsteinMSD(ArrayUniverse(positions=x, dimensions=box), unwrap=True, **kw).run()
    assert got.unwrap and not want.unwrap
    assert scale_rel_err(got.results.timeseries, want.results.timeseries) <= 1e-10
    assert scale_rel_err(got.results.msds_by_particle, want.results.msds_by_particle) <= 1e-10
    # the default is unchanged: the wrapped input gives the wrapped (wrong) MSD
    raw = EinsteinMSD(ArrayUniverse(positions=x, dimensions=box), **kw).run()
    assert scale_rel_err(raw.results.timeseries, want.results.timeseries) > 0.5


def float64_universe(x, dims, charges=None):
    """Timesteps that hand out float64 positions (triclinic boxes are not exact in float32)."""
    uni = ArrayUniverse(positions=x, dimensions=dims, charges=charges)
    uni.trajectory._pos = np.ascontiguousarray(x, dtype=np.float64)
    return uni


@pytest.mark.parametrize("kind", ["tric", "tric_npt", "npt"])
@pytest.mark.parametrize("fft", [True, False])
def test_einstein_msd_triclinic_and_npt(backend, kind, fft):
    u, x, dims, _ = wrapped_case(260, 5, kind, seed=13)
    want = EinsteinMSD(float64_universe(u, dims), fft=fft, stage_dtype=np.float64).run()
    got = EinsteinMSD(float64_universe(x, dims), fft=fft, stage_dtype=np.float64, unwrap=True).run()
    assert scale_rel_err(got.results.timeseries, want.results.timeseries) <= 1e-10
    assert scale_rel_err(got.results.msds_by_particle, want.results.msds_by_particle) <= 1e-10


@pytest.mark.parametrize("fft", [True, False])
@pytest.mark.parametrize("dim_type", ["xyz", "xz", "y"])
def test_conductivity_wrapped_equals_unwrapped(backend, fft, dim_type):
    u, x, box = grid_case(300, 8, seed=17)
    q = np.where(np.arange(8) % 2 == 0, 1.0, -0.75)
    kw = dict(fft=fft, dim_type=dim_type, nernst_einstein=True, linear_fit_window=(10, 200))
    want = ConductivityHelfand(ArrayUniverse(positions=u, dimensions=box, charges=q).atoms, **kw).run()
    got = ConductivityHelfand(ArrayUniverse(positions=x, dimensions=box, charges=q).atoms, unwrap=True, **kw).run()
    assert scale_rel_err(got.results.moment, want.results.moment) <= 1e-10
    assert scale_rel_err(got.results.timeseries, want.results.timeseries) <= 1e-10
    assert scale_rel_err(got.results.timeseries_self, want.results.timeseries_self) <= 1e-10
    assert abs(got.results.conductivity - want.results.conductivity) <= 1e-9 * abs(want.results.conductivity)
    assert abs(got.results.conductivity_self - want.results.conductivity_self) <= 1e-9 * abs(want.results.conductivity_self)
    raw = ConductivityHelfand(ArrayUniverse(positions=x, dimensions=box, charges=q).atoms, **kw).run()
    assert scale_rel_err(raw.results.moment, want.results.moment) > 0.5


def test_conductivity_triclinic_npt_volume(backend):
    u, x, dims, _ = wrapped_case(200, 6, "tric_npt", seed=19)
    q = np.array([1.0, -1.0, 0.5, -0.5, 2.0, -2.0])
    kw = dict(nernst_einstein=True, linear_fit_window=(5, 100), stage_dtype=np.float64)
    want = ConductivityHelfand(float64_universe(u, dims, q).atoms, **kw).run()
    got = ConductivityHelfand(float64_universe(x, dims, q).atoms, unwrap=True, **kw).run()
    assert scale_rel_err(got.results.moment, want.results.moment) <= 1e-10
    assert scale_rel_err(got.results.timeseries, want.results.timeseries) <= 1e-10
    vols = [np.linalg.det(triclinic_vectors(d)) for d in dims]
    assert abs(got._vol_avg - np.mean(vols)) <= 1e-12 * np.mean(vols)


def test_mini_mda_volume():
    """Per-frame boxes; triclinic volume; the orthorhombic product unchanged bit for bit."""
    d = [40.0, 50.0, 60.0, 90, 90, 90]
    ts = ArrayUniverse(positions=np.zeros((2, 1, 3)), dimensions=d).trajectory[1]
    assert ts.volume == float(d[0] * d[1] * d[2])
    dims = box_table("tric_npt", 4)
    traj = ArrayUniverse(positions=np.zeros((4, 1, 3)), dimensions=dims).trajectory
    for t in range(4):
        ts = traj[t]
        assert np.array_equal(ts.dimensions, dims[t])
        assert abs(ts.volume - np.linalg.det(triclinic_vectors(dims[t]))) <= 1e-12 * ts.volume


# ----------------------------------------------------------------------------------- shapes (every branch)
SHAPES = [  # T, A, D, kind
    (1, 3, 3, "const"), (2, 5, 3, "npt"), (63, 4, 1, "const"), (64, 3, 2, "npt"), (65, 7, 3, "const"),
    (255, 5, 2, "const"), (256, 3, 1, "npt"), (257, 7, 3, "npt"), (1023, 3, 3, "const"), (1024, 5, 1, "npt"),
    (1025, 2, 2, "const"), (20000, 3, 3, "npt"), (300, 2500, 3, "const"), (130, 1999, 1, "npt"),
    (1, 2, 3, "tric"), (2, 3, 3, "tric_npt"), (63, 4, 3, "tric"), (65, 5, 3, "tric_npt"), (255, 1, 3, "tric"),
    (257, 6, 3, "tric"), (1023, 3, 3, "tric_npt"), (1025, 4, 3, "tric"), (20000, 3, 3, "tric_npt"),
    (200, 1601, 3, "tric"), (150, 2000, 3, "tric_npt"),
]
AXES = {1: [1], 2: [0, 2], 3: [0, 1, 2]}


@pytest.mark.gpu
@pytest.mark.parametrize("T,A,D,kind", SHAPES)
def test_unwrap_shapes(T, A, D, kind):
    """Frames 1 ... 20000 (partial scan chunks, frames next to 64 / 256 / 1024), D = 1, 2, 3 with even and odd column
    counts and pairs that straddle atoms (and axes, for D = 2), odd atom counts for the triclinic kernel, more pairs
    than one workgroup covers; the kernel named in the timeline; rows n_frames ... pitch - 1 and the partner of an
    unpaired last column still zero in the raw device slab."""
    u, x, dims, n = wrapped_case(T, A, kind, seed=T + A)
    ax = AXES[D]
    x, u, n = x[:, :, ax], u[:, :, ax], n[:, :, ax]
    got, names = unwrap_slab("hip", x, dims, ax, timeline=True)
    assert ("k_unwrap_tric" if kind.startswith("tric") else "k_unwrap_ortho") in names
    L = dims[:, :3].max()
    # 1e-12 of the box up to +-50 images; beyond (20000 frames: ~2400) the positions' own rounding grows with |n|
    assert np.max(np.abs(got - u)) <= 1e-12 * L * max(1.0, np.abs(n).max() / 50)
    assert np.array_equal(got[0], x[0])

    # the raw slab: padding rows and the phantom column untouched
    ctx = _lib.Context(0)
    (h,) = ctx.stage_alloc(T, A, D)
    h[...] = x
    ctx.stage_commit(0, T)
    ctx.unwrap(0, dims, ax)
    ptr, pitch, n_pairs = ctx.stage_device(0)
    raw = np.empty(n_pairs * pitch * 2)
    L_ = _lib.lib()
    L_.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert L_.hipMemcpy(raw.ctypes.data, ptr, raw.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    raw = raw.reshape(n_pairs, pitch, 2)
    assert not raw[:, T:, :].any()
    if (A * D) % 2:
        assert not raw[-1, :, 1].any()
    cols = raw[:, :T, :].transpose(1, 0, 2).reshape(T, -1)[:, :A * D]
    assert np.array_equal(cols.reshape(T, A, D), got)
    ctx.close()


@pytest.mark.gpu
def test_unwrap_device_filled_slab():
    """A slab filled by ta_stage_commit_dev from frame-major device rows unwraps like a host-staged one."""
    import torch

    T, A = 700, 9
    u, x, dims, _ = wrapped_case(T, A, "npt", seed=23)
    ctx = _lib.Context(0)
    ctx.stage_alloc_device(T, A, 3)
    src = torch.from_numpy(x.reshape(T, A * 3).copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    ctx.stage_commit_dev(0, src.data_ptr(), A * 3, 0, T, stream=st)
    ctx.unwrap(0, dims, [0, 1, 2])
    got = read_slab(ctx, "hip", 0, T, A, 3, None)
    assert np.max(np.abs(got - u)) <= 1e-12 * dims[:, :3].max()


@pytest.mark.gpu
def test_unwrap_float32_device_slab_unsupported():
    ctx = _lib.Context(0)
    ctx.set_option("stage_device_f32", 1)
    ctx.stage_alloc(10, 2, 3, dtype=np.float32)
    ctx.stage_commit(0, 10)
    with pytest.raises(_lib.TAError) as e:
        ctx.unwrap(0, box_table("const", 10), [0, 1, 2])
    assert e.value.code == TA_E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("kind", ["npt", "tric_npt"])
def test_repeat_bit_identical_and_idempotent(backend, kind):
    T, A = 600, 11
    u, x, dims, _ = wrapped_case(T, A, kind, seed=29)
    a, _ = unwrap_slab(backend, x, dims, [0, 1, 2])
    b, _ = unwrap_slab(backend, x, dims, [0, 1, 2])
    assert np.array_equal(a, b)
    c, _ = unwrap_slab(backend, a, dims, [0, 1, 2])  # already unwrapped: unchanged
    assert np.array_equal(c, a)


@pytest.mark.gpu
@pytest.mark.parametrize("fft", [True, False])
def test_devices_two_members_one_gpu(fft):
    u, x, box = grid_case(200, 11, seed=31)
    one = EinsteinMSD(ArrayUniverse(positions=x, dimensions=box), fft=fft, unwrap=True).run()
    two = EinsteinMSD(ArrayUniverse(positions=x, dimensions=box), fft=fft, unwrap=True, devices=[0, 0]).run()
    assert two.results.device_ranges == [(0, 5), (5, 11)]
    assert scale_rel_err(two.results.timeseries, one.results.timeseries) <= 1e-13
    assert scale_rel_err(two.results.msds_by_particle, one.results.msds_by_particle) <= 1e-13
    q = np.linspace(-1, 1, 11) + 0.05
    kw = dict(fft=fft, nernst_einstein=True, unwrap=True)
    c1 = ConductivityHelfand(ArrayUniverse(positions=x, dimensions=box, charges=q).atoms, **kw).run()
    c2 = ConductivityHelfand(ArrayUniverse(positions=x, dimensions=box, charges=q).atoms, devices=[0, 0], **kw).run()
    assert scale_rel_err(c2.results.moment, c1.results.moment) <= 1e-13
    assert scale_rel_err(c2.results.timeseries, c1.results.timeseries) <= 1e-12


def _dist_worker(rank, world, port, out_dir):
    import sys

    import torch.distributed as dist

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_unwrap import grid_case
    from transport_analysis_amd import ConductivityHelfand, EinsteinMSD
    from transport_analysis_amd._mini_mda import ArrayUniverse

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    _, x, box = grid_case(120, 7, seed=37)
    q = np.linspace(-1, 1, 7) + 0.1
    m = EinsteinMSD(ArrayUniverse(positions=x, dimensions=box), unwrap=True, distributed=True, device="cpu").run()
    c = ConductivityHelfand(ArrayUniverse(positions=x, dimensions=box, charges=q).atoms, unwrap=True, distributed=True,
                            nernst_einstein=True, device="cpu").run()
    np.savez(os.path.join(out_dir, f"unwrap_{rank}.npz"), msd=m.results.timeseries, bp=m.results.msds_by_particle,
             rng=np.array(m.results.particle_range), moment=c.results.moment, phi=c.results.timeseries,
             self_=c.results.timeseries_self)
    dist.destroy_process_group()


def test_distributed_gloo_world2_cpu_backend(tmp_path):
    import torch.multiprocessing as mp

    world = 2
    port = 37600 + (os.getpid() % 2000)
    mp.spawn(_dist_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    _, x, box = grid_case(120, 7, seed=37)
    q = np.linspace(-1, 1, 7) + 0.1
    m = EinsteinMSD(ArrayUniverse(positions=x, dimensions=box), unwrap=True, device="cpu").run()
    c = ConductivityHelfand(ArrayUniverse(positions=x, dimensions=box, charges=q).atoms, unwrap=True,
                            nernst_einstein=True, device="cpu").run()
    for r in range(world):
        got = np.load(os.path.join(tmp_path, f"unwrap_{r}.npz"))
        lo, hi = got["rng"]
        assert scale_rel_err(got["msd"], m.results.timeseries) <= 1e-12
        assert scale_rel_err(got["bp"], m.results.msds_by_particle[:, lo:hi]) <= 1e-12
        assert scale_rel_err(got["moment"], c.results.moment) <= 1e-12
        assert scale_rel_err(got["phi"], c.results.timeseries) <= 1e-12
        assert scale_rel_err(got["self_"], c.results.timeseries_self) <= 1e-12


# ----------------------------------------------------------------------------------------------------- errors
def test_class_errors_and_warning(backend):
    u, x, box = grid_case(40, 3, seed=41)
    with pytest.raises(ValueError, match="periodic box"):
        EinsteinMSD(ArrayUniverse(positions=x), unwrap=True).run()
    bad = np.tile(np.array(box, dtype=np.float64), (40, 1))
    bad[17, 1] = 0.0
    with pytest.raises(ValueError, match="lengths > 0"):
        EinsteinMSD(ArrayUniverse(positions=x, dimensions=bad), unwrap=True).run()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match="lengths > 0"):
        ConductivityHelfand(ArrayUniverse(positions=x, dimensions=bad, charges=np.ones(3)).atoms, unwrap=True).run()
    tric = [16.0, 16.0, 16.0, 60.0, 60.0, 90.0]
    with pytest.raises(ValueError, match="non-orthogonal"):
        EinsteinMSD(ArrayUniverse(positions=x, dimensions=tric), msd_type="xy", unwrap=True).run()
    with pytest.raises(ValueError, match="non-orthogonal"):
        ConductivityHelfand(ArrayUniverse(positions=x, dimensions=tric, charges=np.ones(3)).atoms, dim_type="z",
                            unwrap=True).run()
    # not consecutive: a warning, then unwrapping over the analysed frames
    with pytest.warns(UserWarning, match="not consecutive"):
        got = EinsteinMSD(ArrayUniverse(positions=x, dimensions=box), unwrap=True).run(step=2)
    want = EinsteinMSD(ArrayUniverse(positions=u, dimensions=box)).run(step=2)
    assert scale_rel_err(got.results.timeseries, want.results.timeseries) <= 1e-10
    with pytest.warns(UserWarning, match="not consecutive"):
        EinsteinMSD(ArrayUniverse(positions=x, dimensions=box), unwrap=True).run(frames=[0, 1, 2, 5, 6])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        EinsteinMSD(ArrayUniverse(positions=x, dimensions=box), unwrap=True).run(start=3, stop=30)
        EinsteinMSD(ArrayUniverse(positions=x, dimensions=box)).run(step=2)  # no unwrapping, no warning


def test_abi_return_codes(backend):
    L = _lib.lib()
    ctx = open_ctx(backend)
    dims = np.tile(np.array([10.0, 10.0, 10.0, 90.0, 90.0, 90.0]), (6, 1))
    ax = np.array([0, 1, 2], dtype=np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    assert L.ta_unwrap(ctx._h, 0, p(dims), p(ax)) == TA_E_STATE  # nothing staged
    assert L.ta_unwrap(None, 0, p(dims), p(ax)) == TA_E_INVALID
    (h,) = ctx.stage_alloc(6, 2, 3)
    h[...] = 1.0
    ctx.stage_commit(0, 6)
    assert L.ta_unwrap(ctx._h, 0, None, p(ax)) == TA_E_INVALID
    assert L.ta_unwrap(ctx._h, 0, p(dims), None) == TA_E_INVALID
    assert L.ta_unwrap(ctx._h, 1, p(dims), p(ax)) == TA_E_INVALID  # no such slab
    assert L.ta_unwrap(ctx._h, 0, p(dims), p(np.array([0, 3, 2], dtype=np.int32))) == TA_E_INVALID
    for row, col, val in ((2, 0, 0.0), (4, 2, -1.0), (5, 1, np.inf), (3, 0, np.nan), (1, 3, 180.0)):
        d = dims.copy()
        d[row, col] = val
        assert L.ta_unwrap(ctx._h, 0, p(d), p(ax)) == TA_E_INVALID
        assert "frame" in L.ta_last_error(ctx._h).decode()
    tric = dims.copy()
    tric[3, 3:] = [60.0, 60.0, 90.0]
    assert L.ta_unwrap(ctx._h, 0, p(tric), p(np.array([0, 2, 1], dtype=np.int32))) == TA_E_INVALID
    assert L.ta_unwrap(ctx._h, 0, p(tric), p(ax)) == 0
    assert L.ta_unwrap(ctx._h, 0, p(dims), p(ax)) == 0
    ctx.stage_alloc(6, 3, 2)
    assert L.ta_unwrap(ctx._h, 0, p(tric), p(np.array([0, 1], dtype=np.int32))) == TA_E_INVALID  # triclinic needs dim 3
    assert L.ta_unwrap(ctx._h, 0, p(dims), p(np.array([2, 0], dtype=np.int32))) == 0
    with pytest.raises(ValueError, match="one box per staged frame"):
        ctx.unwrap(0, dims[:5], [0, 1])
    ctx.close()
    if backend == "cpu":
        g = ctypes.c_void_p()
        assert L.ta_group_create((ctypes.c_int * 1)(-1), 1, ctypes.byref(g)) == TA_E_UNSUPPORTED
    else:
        grp = _lib.Group([0, 0])
        assert L.ta_group_unwrap(grp._h, 0, p(dims), p(ax)) == TA_E_STATE
        grp.stage_alloc(6, 3, 3)
        assert L.ta_group_unwrap(grp._h, 0, None, p(ax)) == TA_E_INVALID
        assert L.ta_group_unwrap(grp._h, 2, p(dims), p(ax)) == TA_E_INVALID
        assert L.ta_group_unwrap(grp._h, 0, p(dims), p(ax)) == 0
        grp.close()
