"""k_kcurrent and the correlations behind it at shapes that reach every branch, through the C-ABI (ta_kcurrent_staged,
ta_kcurrent, ta_group_kcurrent), GPU only.  Every shape runs with fft 1 and 0 on a float64 AND a float32 pair of device slabs
holding the same values, asserts k_kcurrent in the kernel timeline, that no widening kernel ran and that a lag kernel of the
family the VACF dispatch picks for (T, D = 2) did, that repeat runs agree bit for bit, that BOTH staged slabs' bits (padding
included) are unchanged, that the host and the staged entry agree bit for bit for both fft values (check()), and compares with kcurrent_ref: the current
within its derived bar, long and trans within 1e-10 of the trace against the long-double correlations of the returned current.

  * source pairs that straddle atoms (D = 3, odd A), D = 2, and D = 1, whose trans is all zeros;
  * 1, 2, 3 frames with 1 and 2 atoms; an odd frame count over two of the kernel's frame blocks (256 F frames each);
  * more atoms than the grid gives groups at one frame block; eleven frame blocks under an outer-radix plan;
  * the wavevector tail: K = 1, KC - 1, KC, KC + 1, 2 KC + 1 (KC from ta_kcurrent_tile);
  * five wavevectors with "kcurrent_chunk" 1, 2 and 0: the same bits, and the launches of k_kcurrent counted;
  * a small call after a large one, and a small one again, on one context without ta_trim;
  * weights NULL against all ones bit for bit; two group members on one GPU with an odd split; the CPU backend's current;
  * n_atoms dim >= 2^31 is refused before anything is allocated."""
import ctypes

import numpy as np
import pytest

import kcurrent_ref as ref
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu

SLABS = [pytest.param(np.float64, id="slab64"), pytest.param(np.float32, id="slab32")]


def stage(c, case, dtype):
    """the case's velocities (slab 0) and positions (slab 1) staged in `dtype` on context c (replacing what it held), kept in
    that element type on the device"""
    x, v = case[0], case[1]
    T, A, D = x.shape
    c.set_option("stage_device_f32", int(dtype == np.float32))
    vel, pos = c.stage_alloc(T, A, D, n_slabs=2, dtype=dtype)
    vel[:], pos[:] = v, x
    c.stage_commit(0, T)
    c.set_option("timeline", 1)
    return c


def timeline(c):
    return [n for n, _ in c.kernel_timeline(64)]


def run_staged(c, fft, k, w=None, repeat=2, corr=True):
    """ta_kcurrent_staged into caller buffers, `repeat` times: the runs must agree bit for bit.  -> (current, long, trans)"""
    import torch

    dev = torch.device("cuda", 0)
    T, D, K = c.shape[0], c.shape[2], k.shape[0]
    d_w = None if w is None else torch.from_numpy(np.array(w, dtype=np.float64)).to(dev)
    runs = []
    for _ in range(repeat):
        cur = torch.full((K, T, D, 2), np.nan, dtype=torch.float64, device=dev)
        lon = torch.full((K, T), np.nan, dtype=torch.float64, device=dev)
        tr = torch.full((K, T), np.nan, dtype=torch.float64, device=dev)
        c.kcurrent_staged(fft, k, cur.data_ptr(), lon.data_ptr() if corr else 0, tr.data_ptr() if corr else 0,
                          d_weights=0 if d_w is None else d_w.data_ptr())
        torch.cuda.synchronize()
        runs.append((cur.cpu().numpy(), lon.cpu().numpy() if corr else None, tr.cpu().numpy() if corr else None))
    for r in runs[1:]:
        assert all(a is None or np.array_equal(a, b) for a, b in zip(runs[0], r)), "repeat runs differ"
    return runs[0]


def slab_bits(c, slab, dtype):
    """a raw staged device slab, padding included, read after the calls on it have completed"""
    ptr, pitch, n_pairs = c.stage_device(slab)
    raw = np.empty(n_pairs * pitch * 2, dtype=dtype)
    L = _lib.lib()
    L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert L.hipMemcpy(raw.ctypes.data, ptr, raw.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return raw.view(np.uint32 if dtype == np.float32 else np.uint64)


def staged_bits(c, a, dtype):
    """what a slab holds when nothing has touched it since staging: the pair-major layout of `a` in `dtype`, rows
    T ... pitch - 1 and the phantom column of an odd column count zero"""
    T, A, D = a.shape
    _, pitch, n_pairs = c.stage_device(0)
    want = np.zeros((n_pairs * 2, pitch), dtype=dtype)
    want[:A * D, :T] = a.reshape(T, A * D).T
    want = want.reshape(n_pairs, 2, pitch).transpose(0, 2, 1)
    return np.ascontiguousarray(want).ravel().view(np.uint32 if dtype == np.float32 else np.uint64)


def lag_kernels(T, fft):
    """a kernel only the VACF lag-sum dispatch of this length launches on a float64 slab (api.hip: fft_impl, direct_impl with
    the default options) when the by-particle array is asked for, as the correlation of the pseudo-atoms does"""
    if T <= 64:
        return {"k_short"}
    if not fft:
        return {"k_mid"} if 97 <= T <= 512 else {"k_band_bp_vacf"} if T >= 513 else set()
    return {"k_w1_bp"} if T <= 512 else {"k_wsplit_accum", "k_winverse"}


def check(c, dtype, case, what="", launches=None):
    """What every case asserts, for fft 1 and 0: the kernels in the timeline (and, with `launches`, that many of k_kcurrent),
    repeat runs bit-equal, the reference's bars, the host entry bit-equal to the staged one; then both slabs' bits.
    -> {fft: (current, long, trans)}"""
    x, v, w, k = case[:4]
    out = {}
    for fft in (1, 0):
        cur, lon, tr = out[fft] = run_staged(c, fft, k, w)
        names = timeline(c)
        for name in ("k_kcurrent", "k_sum_partials", "k_kcurrent_project", "k_kcurrent_finish"):
            assert name in names, names
        assert "k_widen_f32" not in names, names  # both slabs are read in their own element type
        assert lag_kernels(x.shape[0], fft) <= set(names), (fft, names)
        if launches is not None:
            assert c.kernel_launches("k_kcurrent") == launches, (what, fft, c.kernel_launches("k_kcurrent"), launches)
        ref.assert_kcurrent(cur, lon, tr, case, what=f"{what} fft={fft}")
        host = c.kcurrent(fft, k, w)  # the host-facing call
        assert all(np.array_equal(a, b) for a, b in zip(host, (cur, lon, tr))), (what, fft, "host and staged entries differ")
    assert np.array_equal(slab_bits(c, 0, dtype), staged_bits(c, v, dtype)), "the velocity slab's bits changed"
    assert np.array_equal(slab_bits(c, 1, dtype), staged_bits(c, x, dtype)), "the position slab's bits changed"
    return out


def tile():
    return _lib.kcurrent_tile()


def frame_block(dtype):
    """frames per workgroup of k_kcurrent on a slab of `dtype`"""
    t = tile()
    return 256 * (t["F32"] if dtype == np.float32 else t["F64"])


def units_loop_atoms():
    """more atoms than kcurrent_parts gives groups at one frame block: eight groups per CU"""
    import torch

    return 8 * torch.cuda.get_device_properties(0).multi_processor_count + 905


# (id, T, A, D, K); T None: an odd count over two frame blocks; A None: units_loop_atoms()
SHAPE_CASES = [
    ("straddle", 100, 1501, 3, 3),
    ("d2", 65, 1100, 2, 2),
    ("d1", 513, 2101, 1, 5),
    ("t1a1", 1, 1, 3, 1), ("t2a1", 2, 1, 3, 1), ("t3a1", 3, 1, 3, 1),
    ("t1a2", 1, 2, 3, 1), ("t2a2", 2, 2, 3, 1), ("t3a2", 3, 2, 3, 1),
    ("two_frame_blocks", None, 300, 3, 2),
    ("units_loop", 48, None, 3, 2),
    ("outer_radix", 10300, 33, 3, 2),
]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T,A,D,K", [pytest.param(*c[1:], id=f"{c[0]}-T{c[1]}-A{c[2]}-D{c[3]}-K{c[4]}") for c in SHAPE_CASES])
def test_kcurrent_shapes(T, A, D, K, dtype):
    case = ref.case(T or frame_block(dtype) + 77, A or units_loop_atoms(), D, K)
    c = stage(_lib.Context(0), case, dtype)
    try:
        got = check(c, dtype, case)
        if D == 1:
            assert not np.any(got[1][2]) and not np.any(got[0][2])
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_kcurrent_wavevector_tail(dtype):
    """K around the tile's count: a runtime count handles the unused slots of the last launch"""
    KC = tile()["KC"]
    c = _lib.Context(0)
    try:
        staged = False
        for K in sorted({1, max(KC - 1, 1), KC, KC + 1, 2 * KC + 1}):
            case = ref.case(48, 700, 3, K)
            if not staged:  # (the slabs do not depend on K: the same seed)
                stage(c, case, dtype)
                staged = True
            check(c, dtype, case, what=f"K={K}", launches=-(-K // KC))
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_kcurrent_chunks_bit_equal(dtype):
    KC = tile()["KC"]
    case = ref.case(100, 301, 3, 5)
    c = stage(_lib.Context(0), case, dtype)
    try:
        runs = []
        for chunk, launches in ((1, 5), (2, -(-5 // min(2, KC))), (0, -(-5 // KC))):
            c.set_option("kcurrent_chunk", chunk)
            runs.append(check(c, dtype, case, what=f"chunk={chunk}", launches=launches))
        for r in runs[1:]:
            for fft in (1, 0):
                assert all(np.array_equal(a, b) for a, b in zip(runs[0][fft], r[fft])), fft
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_kcurrent_stale_scratch(dtype):
    """A larger call then a smaller one, and the smaller one again, on ONE context without ta_trim: the second and third
    calls' partial sums, pseudo-atoms (with their tail rows 99 ... 103) and lag sums lie where the first left values."""
    c = _lib.Context(0)
    try:
        for T, A, K in ((1101, 300, 5), (99, 150, 1), (99, 150, 1)):
            case = ref.case(T, A, 3, K)
            stage(c, case, dtype)
            check(c, dtype, case, what=f"T={T}")
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_kcurrent_no_weights_is_all_ones(dtype):
    case = ref.case(100, 301, 3, 2, weighted=False)
    c = stage(_lib.Context(0), case, dtype)
    try:
        got = check(c, dtype, case, what="no weights")
        for fft in (1, 0):
            ones = run_staged(c, fft, case[3], np.ones(301))
            assert all(np.array_equal(p, q) for p, q in zip(got[fft], ones)), fft
        only = run_staged(c, 1, case[3], None, corr=False)  # the current alone: no correlation kernels
        assert np.array_equal(only[0], got[1][0]) and "k_kcurrent_project" not in timeline(c)
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_group_kcurrent(dtype):
    """ta_group_kcurrent on devices [0, 0] (751 + 750 atoms: an odd split), the members' slabs in `dtype` on the device: the
    members' currents add up within the bar, long and trans are those of the summed current.  A group has no staged entry
    and no timeline of its own: the kernels are looked for in the members' timelines (the member that correlates holds the
    correlation's, the other one the pass's; a call for the current alone leaves the pass's in both), the slabs' bits in the
    members' slabs, and long / trans are compared bit for bit with ta_kcurrent_correlate of the returned current."""
    case = ref.case(100, 1501, 3, 3)
    x, v, w, k = case[:4]
    T, A, D = x.shape
    g = _lib.Group([0, 0])
    one = _lib.Context(0)
    try:
        g.set_option("stage_device_f32", int(dtype == np.float32))
        vels, poss = g.stage_alloc(T, A, D, n_slabs=2, dtype=dtype)
        assert any((hi - lo) % 2 for lo, hi in g.shards)
        for (lo, hi), vel, pos in zip(g.shards, vels, poss):
            vel[:], pos[:] = v[:, lo:hi], x[:, lo:hi]
        g.stage_commit(0, T)
        g.set_option("timeline", 1)
        members = [g.member_context(i) for i in range(2)]
        for m, (lo, hi) in zip(members, g.shards):
            m.shape = (T, hi - lo, D)
        for fft in (1, 0):
            cur, lon, tr = g.kcurrent(fft, k, w)
            first, second = timeline(members[0]), timeline(members[1])
            assert "k_kcurrent" in second and "k_sum_partials" in second, second
            assert {"k_kcurrent_project", "k_kcurrent_finish"} | lag_kernels(T, fft) <= set(first), (fft, first)
            assert "k_widen_f32" not in first + second
            again = g.kcurrent(fft, k, w)
            assert all(np.array_equal(a, b) for a, b in zip((cur, lon, tr), again)), "repeat runs differ"
            ref.assert_kcurrent(cur, lon, tr, case, what=f"group fft={fft}")
            lon1, tr1 = one.kcurrent_correlate(cur, k, fft)
            assert np.array_equal(lon, lon1) and np.array_equal(tr, tr1)
            _, lon2, tr2 = g.kcurrent(fft, k, w, current=False)  # the current summed inside the call
            assert np.array_equal(lon, lon2) and np.array_equal(tr, tr2)
            alone = g.kcurrent(fft, k, w, longitudinal=False, transverse=False)
            assert np.array_equal(alone[0], cur) and alone[1] is None and alone[2] is None
            for m in members:
                names = timeline(m)
                assert "k_kcurrent" in names and "k_widen_f32" not in names and "k_kcurrent_project" not in names, names
        for m, (lo, hi) in zip(members, g.shards):
            assert np.array_equal(slab_bits(m, 0, dtype), staged_bits(m, v[:, lo:hi], dtype)), "a velocity slab's bits changed"
            assert np.array_equal(slab_bits(m, 1, dtype), staged_bits(m, x[:, lo:hi], dtype)), "a position slab's bits changed"
    finally:
        one.close()
        g.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_kcurrent_against_cpu_backend(dtype):
    case = ref.case(100, 301, 3, 3)
    c = stage(_lib.Context(0), case, dtype)
    cpu = _lib.Context("cpu")
    try:
        vel, pos = cpu.stage_alloc(100, 301, 3, n_slabs=2, dtype=dtype)
        vel[:], pos[:] = case[1], case[0]
        cpu.stage_commit(0, 100)
        got = c.kcurrent(1, case[3], case[2])
        want = cpu.kcurrent(1, case[3], case[2])
        err = np.max(np.abs(got[0] - want[0]), axis=(0, 1, 3))
        print(f"    GPU - CPU current: {err} (bar {case[6]})")
        assert np.all(err <= case[6])
        ref.assert_correlations(want[0], want[1], want[2], case, what="cpu")
    finally:
        c.close()
        cpu.close()


def test_refuses_2_pow_31_columns():
    """n_atoms dim >= 2^31: TA_E_INVALID before anything is allocated or written.  The slabs are device-only, one frame of
    2^30 atoms x 2 float32 columns (never filled).  "fail_alloc_after" 1 makes the call's first workspace request fail with
    TA_E_NOMEM: the refusal comes first, so no workspace was asked for."""
    import torch

    c = _lib.Context(0)
    try:
        c.set_option("stage_device_f32", 1)
        c.stage_alloc_device(1, 2 ** 30, 2, n_slabs=2)
        cur = torch.full((1, 1, 2, 2), -7.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        c.set_option("fail_alloc_after", 1)
        with pytest.raises(_lib.TAError, match="n_atoms \\* dim must be below 2\\^31") as e:
            c.kcurrent_staged(1, np.array([[1.0, 0.5]]), cur.data_ptr())
        assert e.value.code == -1
        c.set_option("fail_alloc_after", 0)
        torch.cuda.synchronize()
        assert bool((cur == -7.0).all())
    finally:
        c.close()
