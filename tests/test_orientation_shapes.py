"""k_orient and the evaluations behind it at shapes that reach every branch, through the C-ABI (ta_orient_staged, ta_orient_dev,
ta_orient), GPU only.  Every case runs with fft 1 and 0 on a float64 AND a float32 device slab holding the same values,
asserts k_orient in the kernel timeline with one launch per rank asked for, that no widening kernel ran, that repeat runs
agree bit for bit, that the staged slab's bits (padding included) are unchanged, and compares with orient_ref at lag_sample:
c1 and c2 within 1e-10 of their maxima, the total within the header's bound, coll within 1e-10 of its maximum against the
long-double autocorrelation of the returned total.

  * 1, 2, 3 frames with 1 and 2 vectors; an odd and an even vector count (the rank-1 phantom column, the one-item last unit);
    an odd frame count over two frame blocks (the float32 load whose second row is row T); more units than pm_unit_grid
    gives groups; eleven frame blocks with an outer-radix plan;
  * index rows with the first and the last atom of the slab, odd and even atoms in every position of a row (molecule m is
    atoms 3 m, 3 m + 1, 3 m + 2), atoms shared between vectors, a permuted list;
  * the three modes; no box, a constant and a per-frame box, orthorhombic and triclinic, on molecules the faces cut;
  * a smaller call straight after a larger one on one context without ta_trim; the frame-major entry with wide rows and the
    host-facing call against the staged one bit for bit; the CPU backend within the bars; each output alone."""
import ctypes

import numpy as np
import pytest

import orient_ref as ref
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu

LD = np.longdouble
SLABS = [pytest.param(np.float64, id="slab64"), pytest.param(np.float32, id="slab32")]


def stage(c, x, dtype):
    """x staged in `dtype` on context c (replacing what it held), kept in that element type on the device"""
    T, A, D = x.shape
    c.set_option("stage_device_f32", int(dtype == np.float32))
    (view,) = c.stage_alloc(T, A, D, dtype=dtype)
    view[:] = x
    c.stage_commit(0, T)
    c.set_option("timeline", 1)
    return c


def timeline(c):
    return [n for n, _ in c.kernel_timeline(64)]


def slab_bits(c, dtype):
    """the raw staged device slab, padding included, read after the calls on it have completed"""
    ptr, pitch, n_pairs = c.stage_device(0)
    raw = np.empty(n_pairs * pitch * 2, dtype=dtype)
    L = _lib.lib()
    L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert L.hipMemcpy(raw.ctypes.data, ptr, raw.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return raw.view(np.uint32 if dtype == np.float32 else np.uint64)


def staged_bits(c, x, dtype):
    """what the slab holds when nothing has touched it since staging: the pair-major layout of x in `dtype`, rows
    T ... pitch - 1 and the phantom column of an odd column count zero"""
    T, A, D = x.shape
    _, pitch, n_pairs = c.stage_device(0)
    want = np.zeros((n_pairs * 2, pitch), dtype=dtype)
    want[:A * D, :T] = x.reshape(T, A * D).T
    want = want.reshape(n_pairs, 2, pitch).transpose(0, 2, 1)
    return np.ascontiguousarray(want).ravel().view(np.uint32 if dtype == np.float32 else np.uint64)


ALL = (True, True, True, True)


def run_staged(c, fft, idx, mode, dims=None, w=None, ask=ALL, repeat=2):
    """ta_orient_staged into caller buffers, `repeat` times: the runs must agree bit for bit.  -> (c1, c2, total, coll), None
    for one not asked for"""
    import torch

    dev = torch.device("cuda", 0)
    T = c.shape[0]
    runs = []
    for _ in range(repeat):
        bufs = [torch.full(s, np.nan, dtype=torch.float64, device=dev) if a else None
                for s, a in zip(((T,), (T,), (T, 3), (T,)), ask)]
        c.orient_staged(fft, idx, mode, dims, w, *[b.data_ptr() if b is not None else 0 for b in bufs])
        torch.cuda.synchronize()
        runs.append([None if b is None else b.cpu().numpy() for b in bufs])
    for r in runs[1:]:
        assert all(a is None or np.array_equal(a, b) for a, b in zip(runs[0], r)), "repeat runs differ"
    return runs[0]


def check(c, dtype, x, idx, mode, want, dims=None, w=None, what=""):
    for fft in (1, 0):
        got = run_staged(c, fft, idx, mode, dims, w)
        names = timeline(c)
        assert c.kernel_launches("k_orient") == 2, names  # one launch per rank
        assert "k_widen_f32" not in names, names  # the slab is read in its own element type
        ref.assert_orient(got, want, what=f"{what} fft={fft}")
    assert np.array_equal(slab_bits(c, dtype), staged_bits(c, x, dtype)), "the staged slab's bits changed"
    return got


def units_loop_vectors():
    """more rank-1 units (two vectors each) than pm_unit_grid gives groups at one frame block: 16 groups per CU"""
    import torch

    return 2 * 16 * torch.cuda.get_device_properties(0).multi_processor_count + 907


# (id, T, N, molecules in the slab or None: one per vector); N None: units_loop_vectors()
SHAPE_CASES = [
    ("t1n1", 1, 1, None), ("t2n1", 2, 1, None), ("t3n1", 3, 1, None),
    ("t1n2", 1, 2, None), ("t2n2", 2, 2, None), ("t3n2", 3, 2, None),
    ("odd", 100, 1501, 1000), ("even", 100, 1500, 1000),
    ("two_frame_blocks", 1101, 300, None),
    ("units_loop", 48, None, None),
    ("outer_radix", 10300, 33, 20),
]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("T,N,n_mol", [pytest.param(*c[1:], id=f"{c[0]}-T{c[1]}-N{c[2]}") for c in SHAPE_CASES])
def test_orient_shapes(T, N, n_mol, mode, dtype):
    x, idx, w, want = ref.case(T, N or units_loop_vectors(), mode, weighted=True, n_mol=n_mol)
    A = x.shape[1]
    assert idx.min() == 0 and idx.max() == A - 1  # the first and the last atom of the slab
    if A >= 12:  # odd and even atoms in every position of a row
        assert all(len(set(idx[:, j] % 2)) == 2 for j in range(idx.shape[1]))
    c = stage(_lib.Context(0), x, dtype)
    try:
        got = check(c, dtype, x, idx, mode, want, w=w)
        host = c.orient(0, idx, mode, weights=w)  # the host-facing call
        assert all(np.array_equal(a, b) for a, b in zip(host, got))
    finally:
        c.close()


BOXES = [pytest.param(ref.ORTHO, False, id="ortho-constant"), pytest.param(ref.ORTHO, True, id="ortho-per-frame"),
         pytest.param(ref.TRIC, False, id="tric-constant"), pytest.param(ref.TRIC, True, id="tric-per-frame")]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("dims,moving", BOXES)
def test_orient_boxes(dims, moving, mode, dtype):
    """molecules the faces cut, 1101 frames (two frame blocks, odd) of 301 vectors: with the box the call matches the
    reference of the staged values with the same image step, and the unwrapped trajectory's functions; without it, it does not"""
    T, N = 1101, 301
    x, idx, _, free = ref.case(T, N, mode, seed=3)
    box = ref.box_frames(dims, T, moving)
    wrapped = ref.near_corner_wrapped(x, idx, box)
    wrapped = wrapped.astype(dtype).astype(np.float64)  # what the slab holds
    c = stage(_lib.Context(0), wrapped, dtype)
    try:
        got = check(c, dtype, wrapped, idx, mode, ref.reference(wrapped, idx, mode, box), dims=box)
        if dtype == np.float64 or (dims is ref.ORTHO and not moving):  # (float32 keeps the dyadic box's values exactly)
            lags, c1, c2 = free[:3]
            for g, w_, f in ((got[0], c1, 1.0), (got[1], c2, 1.5)):
                assert float(np.max(np.abs(f * g[lags].astype(LD) - w_))) <= 1e-10 * float(np.max(np.abs(w_)))
        bare = run_staged(c, 1, idx, mode, repeat=1)
        assert np.abs(bare[2] - got[2]).max() > 0.1
    finally:
        c.close()


def test_orient_stale_scratch():
    """A larger call (1101 frames, 300 vectors) then a smaller one (99 frames: rows 99 ... 103 of every pair, 151 vectors: a
    phantom column) on ONE context without ta_trim: the second call's block, its tail rows and the total's pair-major copy lie
    where the first left values."""
    c = _lib.Context(0)
    try:
        for T, N in ((1101, 300), (99, 151)):
            x, idx, w, want = ref.case(T, N, "bisector", weighted=True)
            stage(c, x, np.float64)
            check(c, np.float64, x, idx, "bisector", want, w=w, what=f"T={T}")
    finally:
        c.close()


def test_orient_dev_wide_rows():
    """ta_orient_dev on a frame-major tensor with ld_row > n_atoms dim equals the staged path bit for bit"""
    import torch

    T, N = 1101, 300
    x, idx, w, _ = ref.case(T, N, "normal", weighted=True)
    A = x.shape[1]
    box = ref.box_frames(ref.TRIC, T, True)
    ld_row = A * 3 + 7
    wide = np.full((T, ld_row), 7.5e3)
    wide[:, :A * 3] = x.reshape(T, A * 3)
    d_x = torch.from_numpy(wide).to("cuda:0")
    c = stage(_lib.Context(0), x, np.float64)
    try:
        for fft in (1, 0):
            want = run_staged(c, fft, idx, "normal", box, w)
            bufs = [torch.full(s, np.nan, dtype=torch.float64, device="cuda:0") for s in ((T,), (T,), (T, 3), (T,))]
            c.orient_dev(d_x.data_ptr(), T, A, 3, ld_row, fft, idx, "normal", box, w, *[b.data_ptr() for b in bufs])
            torch.cuda.synchronize()
            names = timeline(c)
            assert "k_relayout" in names and "k_orient" in names, names
            for a, b in zip(want, bufs):
                assert np.array_equal(a, b.cpu().numpy()), fft
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_orient_each_output_alone_and_cpu_backend(dtype):
    """every output alone has the bits it has with all four (and k_orient runs once per rank that output needs); the CPU
    backend's results agree within the bars"""
    T, N = 513, 77
    x, idx, w, want = ref.case(T, N, "bisector", weighted=True, n_mol=50)
    box = ref.box_frames(ref.ORTHO, T, True)
    c = stage(_lib.Context(0), x, dtype)
    cpu = _lib.Context("cpu")
    try:
        (view,) = cpu.stage_alloc(T, x.shape[1], 3, dtype=dtype)
        view[:] = x
        cpu.stage_commit(0, T)
        for fft in (1, 0):
            full = run_staged(c, fft, idx, "bisector", box, w)
            for i, launches in enumerate((1, 1, 1, 1)):
                ask = tuple(j == i for j in range(4))
                got = run_staged(c, fft, idx, "bisector", box, w, ask=ask, repeat=1)
                assert c.kernel_launches("k_orient") == launches
                assert np.array_equal(got[i], full[i]), (fft, i)
            host = cpu.orient(fft, idx, "bisector", dimensions=box, weights=w)
            for name, g, h in zip(("c1", "c2", "total", "coll"), full, host):
                scale = want[5] if name == "total" else float(np.max(np.abs(h)))
                err = float(np.max(np.abs(g - h))) / scale
                print(f"    GPU against CPU backend, fft={fft} {name}: {err:.3e} of {scale:.3e}")
                assert err <= 1e-10
    finally:
        c.close()
        cpu.close()


def test_orient_checks_before_anything_is_written():
    """a bad index row, found on the host: TA_E_INVALID, the device outputs untouched, no launch"""
    import torch

    x, idx, _, _ = ref.case(8, 4, "bond")
    c = stage(_lib.Context(0), x, np.float64)
    try:
        out = torch.full((8,), 7.5, dtype=torch.float64, device="cuda:0")
        bad = np.array(idx)
        bad[2, 1] = x.shape[1]
        with pytest.raises(_lib.TAError, match="is outside 0 ... n_atoms - 1") as e:
            c.orient_staged(1, bad, "bond", d_c1=out.data_ptr())
        assert e.value.code == -1
        torch.cuda.synchronize()
        assert bool((out == 7.5).all())
    finally:
        c.close()
