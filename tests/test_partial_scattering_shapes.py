"""k_species_density and the cross term behind it at shapes that reach every branch, through the C-ABI
(ta_partial_density_staged, ta_partial_density, ta_group_partial_density), GPU only.  Every shape runs with fft 1 and 0 on a
float64 AND a float32 device slab holding the same values, asserts k_species_density in the kernel timeline, that no widening
kernel ran and that a lag kernel of the family the VACF dispatch picks for (T, D = 2) did, that repeat runs agree bit for bit,
that the slab's bits (padding included) are unchanged, that the host and the staged entry agree bit for bit (check()), and
compares with partial_ref: the density of every species within its derived bar, the cross term within 1e-10 of
max(cross_aa(0), cross_bb(0)) against the long-double defining sum of the returned density, symmetric bit for bit.

  * source pairs that straddle atoms (D = 3, odd A) with three interleaved species, D = 2, and D = 1 with one species;
  * 1, 2, 3 frames with 1 and 2 atoms (one atom: one of the two species is empty); an odd frame count over two of the
    kernel's frame blocks (256 F frames each, F from ta_partial_density_tile) with four species;
  * more atoms than the grid gives groups at one frame block, with eight species; eleven frame blocks under an outer-radix plan;
  * the wavevector tail of every tile: K = 1, KC - 1, KC, KC + 1, 2 KC + 1 for ST = 1, 2, 4, 8 (KC from the tile entry);
  * the species tail: S = 1, 2, 3, 4, 5, 8 -- fewer species than slots, and a species without atoms in the middle of the range;
  * five wavevectors with "partial_chunk" 1, 2 and 0: the same bits, and the launches of k_species_density counted;
  * a small call after a large one, and a small one again, on one context without ta_trim;
  * weights NULL against all ones bit for bit; two group members on one GPU with an odd split; the CPU backend's density on
    non-grid walks; the sum over species against ta_scatter_staged's density;
  * n_atoms dim >= 2^31 is refused before anything is allocated; the class on cuda:0 and on a group of two members."""
import numpy as np
import pytest

import partial_ref as ref
from test_current_correlation_shapes import lag_kernels, slab_bits, staged_bits, timeline, units_loop_atoms
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu

SLABS = [pytest.param(np.float64, id="slab64"), pytest.param(np.float32, id="slab32")]


def stage(c, x, dtype):
    """positions x staged in `dtype` on context c (replacing what it held), kept in that element type on the device"""
    T, A, D = x.shape
    c.set_option("stage_device_f32", int(dtype == np.float32))
    (pos,) = c.stage_alloc(T, A, D, dtype=dtype)
    pos[:] = x
    c.stage_commit(0, T)
    c.set_option("timeline", 1)
    return c


def run_staged(c, fft, k, lab, S, w=None, repeat=2, cross=True):
    """ta_partial_density_staged into caller buffers, `repeat` times: the runs must agree bit for bit.  -> (density, cross)"""
    import torch

    dev = torch.device("cuda", 0)
    T, K = c.shape[0], k.shape[0]
    d_lab = torch.from_numpy(np.array(lab, dtype=np.int32)).to(dev)
    d_w = None if w is None else torch.from_numpy(np.array(w, dtype=np.float64)).to(dev)
    runs = []
    for _ in range(repeat):
        rho = torch.full((K, S, T, 2), np.nan, dtype=torch.float64, device=dev)
        cr = torch.full((K, T, S, S), np.nan, dtype=torch.float64, device=dev)
        c.partial_density_staged(fft, k, S, d_lab.data_ptr(), rho.data_ptr(), cr.data_ptr() if cross else 0,
                                 d_weights=0 if d_w is None else d_w.data_ptr())
        torch.cuda.synchronize()
        runs.append((rho.cpu().numpy(), cr.cpu().numpy() if cross else None))
    for r in runs[1:]:
        assert all(a is None or np.array_equal(a, b) for a, b in zip(runs[0], r)), "repeat runs differ"
    return runs[0]


def check(c, dtype, case, what="", launches=None):
    """What every case asserts, for fft 1 and 0: the kernels in the timeline (and, with `launches`, that many of
    k_species_density), repeat runs bit-equal, the reference's bars, the host entry bit-equal to the staged one; then the slab's
    bits.  -> {fft: (density, cross)}"""
    x, w, lab, k, S = case[0], case[1], case[2], case[3], case[7]
    out = {}
    for fft in (1, 0):
        rho, cr = out[fft] = run_staged(c, fft, k, lab, S, w)
        names = timeline(c)
        for name in ("k_species_density", "k_sum_partials", "k_onsager_combos", "k_partial_finish"):
            assert name in names, names
        assert "k_widen_f32" not in names, names  # the slab is read in its own element type
        assert lag_kernels(x.shape[0], fft) <= set(names), (fft, names)
        if launches is not None:
            got = c.kernel_launches("k_species_density")
            assert got == launches, (what, fft, got, launches)
        ref.assert_partial(rho, cr, case, what=f"{what} fft={fft}")
        host = c.partial_density(fft, k, lab, S, w)  # the host-facing call
        assert all(np.array_equal(a, b) for a, b in zip(host, (rho, cr))), (what, fft, "host and staged entries differ")
    assert np.array_equal(slab_bits(c, 0, dtype), staged_bits(c, x, dtype)), "the position slab's bits changed"
    return out


def tile(S):
    return _lib.partial_density_tile(S)


def frame_block(dtype, S):
    """frames per workgroup of k_species_density on a slab of `dtype`"""
    t = tile(S)
    return 256 * (t["F32"] if dtype == np.float32 else t["F64"])


# (id, T, A, D, K, S, empty); T None: an odd count over two frame blocks; A None: units_loop_atoms()
SHAPE_CASES = [
    ("straddle", 100, 1501, 3, 3, 3, None),
    ("d2", 65, 1100, 2, 2, 2, None),
    ("d1", 513, 2101, 1, 5, 1, None),
    ("t1a1", 1, 1, 3, 1, 2, 1), ("t2a1", 2, 1, 3, 1, 2, 1), ("t3a1", 3, 1, 3, 1, 2, 1),
    ("t1a2", 1, 2, 3, 1, 2, None), ("t2a2", 2, 2, 3, 1, 2, None), ("t3a2", 3, 2, 3, 1, 2, None),
    ("two_frame_blocks", None, 300, 3, 2, 4, None),
    ("units_loop", 48, None, 3, 2, 8, None),
    ("outer_radix", 10300, 33, 3, 2, 2, None),
]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T,A,D,K,S,empty",
                         [pytest.param(*c[1:], id=f"{c[0]}-T{c[1]}-A{c[2]}-D{c[3]}-K{c[4]}-S{c[5]}") for c in SHAPE_CASES])
def test_partial_shapes(T, A, D, K, S, empty, dtype):
    case = ref.case(T or frame_block(dtype, S) + 77, A or units_loop_atoms(), D, K, S, empty=empty)
    c = stage(_lib.Context(0), case[0], dtype)
    try:
        check(c, dtype, case)
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("S", [1, 2, 4, 8])
def test_partial_wavevector_tail(S, dtype):
    """K around the count of every tile (ST = S here): a runtime count handles the unused slots of the last launch"""
    t = tile(S)
    assert t["ST"] == S
    KC = t["KC"]
    c = _lib.Context(0)
    try:
        staged = False
        for K in sorted({1, max(KC - 1, 1), KC, KC + 1, 2 * KC + 1}):
            case = ref.case(48, 700, 3, K, S)
            if not staged:  # (the slab does not depend on K: the same seed)
                stage(c, case[0], dtype)
                staged = True
            check(c, dtype, case, what=f"S={S} K={K}", launches=-(-K // KC))
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("S,empty", [(1, None), (2, None), (3, 1), (4, None), (5, 2), (8, 3)])
def test_partial_species_tail(S, empty, dtype):
    """S < ST slots (3 of 4, 5 of 8), every slot used, and a species without atoms in the middle of the label range"""
    assert tile(S)["ST"] == (1 if S == 1 else 2 if S == 2 else 4 if S <= 4 else 8)
    case = ref.case(70, 403, 3, 2, S, empty=empty)
    c = stage(_lib.Context(0), case[0], dtype)
    try:
        got = check(c, dtype, case, what=f"S={S}")
        if empty is not None:
            for fft in (1, 0):
                assert not np.any(got[fft][0][:, empty]) and not np.any(got[fft][1][:, :, empty]) and not np.any(got[fft][1][..., empty])
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_partial_chunks_bit_equal(dtype):
    S = 3
    KC = tile(S)["KC"]
    case = ref.case(100, 301, 3, 5, S)
    c = stage(_lib.Context(0), case[0], dtype)
    try:
        runs = []
        for chunk, launches in ((1, 5), (2, -(-5 // min(2, KC))), (0, -(-5 // KC))):
            c.set_option("partial_chunk", chunk)
            runs.append(check(c, dtype, case, what=f"chunk={chunk}", launches=launches))
        for r in runs[1:]:
            for fft in (1, 0):
                assert all(np.array_equal(a, b) for a, b in zip(runs[0][fft], r[fft])), fft
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_partial_stale_scratch(dtype):
    """A larger call then a smaller one, and the smaller one again, on ONE context without ta_trim: the second and third
    calls' partial sums, pseudo-particles (with their tail rows 99 ... 103) and lag sums lie where the first left values."""
    c = _lib.Context(0)
    try:
        for T, A, K, S in ((1101, 300, 5, 4), (99, 150, 1, 2), (99, 150, 1, 2)):
            case = ref.case(T, A, 3, K, S)
            stage(c, case[0], dtype)
            check(c, dtype, case, what=f"T={T}")
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_partial_no_weights_is_all_ones(dtype):
    case = ref.case(100, 301, 3, 2, 3, weighted=False)
    c = stage(_lib.Context(0), case[0], dtype)
    try:
        got = check(c, dtype, case, what="no weights")
        for fft in (1, 0):
            ones = run_staged(c, fft, case[3], case[2], 3, np.ones(301))
            assert all(np.array_equal(p, q) for p, q in zip(got[fft], ones)), fft
        only = run_staged(c, 1, case[3], case[2], 3, None, cross=False)  # the density alone: no correlation kernels
        assert np.array_equal(only[0], got[1][0]) and "k_onsager_combos" not in timeline(c)
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_group_partial_density(dtype):
    """ta_group_partial_density on devices [0, 0] (751 + 750 atoms: an odd split), the members' slabs in `dtype` on the
    device: the members' densities add up within the bar, the cross term is that of the summed density, bit for bit
    ta_partial_cross of the returned density.  The kernels are looked for in the members' timelines, the slab's bits in the
    members' slabs."""
    case = ref.case(100, 1501, 3, 3, 3)
    x, w, lab, k = case[:4]
    T, A, D = x.shape
    g = _lib.Group([0, 0])
    one = _lib.Context(0)
    try:
        g.set_option("stage_device_f32", int(dtype == np.float32))
        (poss,) = g.stage_alloc(T, A, D, dtype=dtype)
        assert any((hi - lo) % 2 for lo, hi in g.shards)
        for (lo, hi), pos in zip(g.shards, poss):
            pos[:] = x[:, lo:hi]
        g.stage_commit(0, T)
        g.set_option("timeline", 1)
        members = [g.member_context(i) for i in range(2)]
        for fft in (1, 0):
            rho, cr = g.partial_density(fft, k, lab, 3, w)
            first, second = timeline(members[0]), timeline(members[1])
            assert "k_species_density" in second and "k_sum_partials" in second, second
            assert {"k_onsager_combos", "k_partial_finish"} | lag_kernels(T, fft) <= set(first), (fft, first)
            assert "k_widen_f32" not in first + second
            again = g.partial_density(fft, k, lab, 3, w)
            assert np.array_equal(rho, again[0]) and np.array_equal(cr, again[1]), "repeat runs differ"
            ref.assert_partial(rho, cr, case, what=f"group fft={fft}")
            assert np.array_equal(cr, one.partial_cross(rho, fft))
            alone = g.partial_density(fft, k, lab, 3, w, cross=False)
            assert np.array_equal(alone[0], rho) and alone[1] is None
        for m, (lo, hi) in zip(members, g.shards):
            m.shape = (T, hi - lo, D)
            assert np.array_equal(slab_bits(m, 0, dtype), staged_bits(m, x[:, lo:hi], dtype)), "a position slab's bits changed"
    finally:
        one.close()
        g.close()


def off_grid(case):
    """the case's walk moved off the 1/1024 grid (float32 values: both backends then stage the same numbers in either type)"""
    x = case[0] + np.random.default_rng(9).uniform(-0.01, 0.01, size=case[0].shape)
    return x.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("dtype", SLABS)
def test_partial_against_cpu_backend(dtype):
    """non-grid walks: the GPU's density against the CPU backend's within twice the bar (each is within one of the exact sum)"""
    case = ref.case(100, 301, 3, 3, 3)
    x = off_grid(case)
    w, lab, k = case[1], case[2], case[3]
    bar = 2 * ref.density_bar(x, w, lab, 3, k)
    c = stage(_lib.Context(0), x, dtype)
    cpu = _lib.Context("cpu")
    try:
        (pos,) = cpu.stage_alloc(100, 301, 3, dtype=dtype)
        pos[:] = x
        cpu.stage_commit(0, 100)
        got = c.partial_density(1, k, lab, 3, w)
        want = cpu.partial_density(1, k, lab, 3, w)
        err = np.max(np.abs(got[0] - want[0]), axis=(0, 2, 3))
        print(f"    GPU - CPU density: {err} (bar {bar})")
        assert np.all(err <= bar)
        ref.assert_cross(want[0], want[1], case, what="cpu")
        ref.assert_cross(got[0], got[1], case, what="gpu")
    finally:
        c.close()
        cpu.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_partial_sums_to_scatter_density(dtype):
    """unit weights: the sum over species against ta_scatter_staged's density on the same slab, within twice the bound of
    the whole group (the two orders of summation differ: not a bit comparison)"""
    import torch

    case = ref.case(100, 301, 3, 3, 3, weighted=False)
    x, lab, k = case[0], case[2], case[3]
    bar = 2 * ref.density_bar(x, None, np.zeros(301, dtype=np.int32), 1, k)[0]
    c = stage(_lib.Context(0), x, dtype)
    try:
        rho = run_staged(c, 1, k, lab, 3, None, repeat=1, cross=False)[0]
        d = torch.full((3, 100, 2), np.nan, dtype=torch.float64, device="cuda:0")
        c.scatter_staged(1, k, d_density=d.data_ptr())
        torch.cuda.synchronize()
        err = float(np.max(np.abs(rho.sum(axis=1) - d.cpu().numpy())))
        print(f"    sum over species - ta_scatter density: {err:.3e} (bar {bar:.3e})")
        assert err <= bar
    finally:
        c.close()


def test_refuses_2_pow_31_columns():
    """n_atoms dim >= 2^31: TA_E_INVALID before anything is allocated or written.  The slab is device-only, one frame of
    2^30 atoms x 2 float32 columns (never filled).  "fail_alloc_after" 1 makes the call's first workspace request fail with
    TA_E_NOMEM: the refusal comes first, so no workspace was asked for."""
    import torch

    c = _lib.Context(0)
    try:
        c.set_option("stage_device_f32", 1)
        c.stage_alloc_device(1, 2 ** 30, 2, n_slabs=1)
        rho = torch.full((1, 1, 1, 2), -7.0, dtype=torch.float64, device="cuda:0")
        lab = torch.zeros(4, dtype=torch.int32, device="cuda:0")  # (never read)
        torch.cuda.synchronize()
        c.set_option("fail_alloc_after", 1)
        with pytest.raises(_lib.TAError, match="n_atoms \\* dim must be below 2\\^31") as e:
            c.partial_density_staged(1, np.array([[1.0, 0.5]]), 1, lab.data_ptr(), rho.data_ptr())
        assert e.value.code == -1
        c.set_option("fail_alloc_after", 0)
        torch.cuda.synchronize()
        assert bool((rho == -7.0).all())
    finally:
        c.close()


@pytest.mark.parametrize("place", [pytest.param({}, id="one_device"), pytest.param({"devices": [0, 0]}, id="two_members")])
def test_class_on_the_gpu(place):
    """PartialScattering through the class on cuda:0 and on a group of two members (the densities added before the cross
    term): float32 staging stays float32 (the walk is exact in it), the results against the reference over all atoms"""
    from transport_analysis_amd import PartialScattering
    from transport_analysis_amd._mini_mda import ArrayUniverse

    case = ref.case(65, 33, 3, 3, 3)
    x, w, lab, k = case[:4]
    u = ArrayUniverse(positions=x)
    for fft in (True, False):
        r = PartialScattering(u.atoms, k, species=lab, weights=w, fft=fft, **place).run().results
        ref.assert_partial(r.density, r.f_partial_by_kvector.transpose(1, 0, 2, 3) * 33, case, what=f"class {place} fft={fft}")
        assert list(r.species_counts) == [11, 11, 11] and r.f_partial.shape == (65, 3, 3, 3)
