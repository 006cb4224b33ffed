"""k_bond_series and k_pair_filter at shapes that reach every branch, through the C-ABI (ta_bond_lifetime_staged,
ta_bond_lifetime), GPU only.  Every case runs on a float64 AND a float32 device slab holding the same values and asserts
k_bond_series in the kernel timeline, k_pair_filter there exactly when the call needs it, that neither k_pair_series nor a
widening kernel ran, the run lengths, bonded counts and (fft = 0) lag sums EQUAL to bond_ref's, repeat runs bit-equal, the
staged slab's bits (padding included) unchanged, and the host-facing entry bit-equal to the staged one.

  patterns  bond_ref.constructed_levels (absences of gap and gap + 1 frames inside a word and across the 63|64 and 1023|1024
            edges, a 63-frame absence from mid-word, leading and trailing absences, alternating, the hysteresis carry through
            three whole words, level 1 before the first 2, a 0 inside, level 1 only, 2 at frame 63 and 1 at 64, two hysteresis
            runs joined by the closing) at T = 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049, gap = 0, 1, 2, 63,
            P = 1, 2, 3, 15 and 129 bonds; "pair_chunk" 1, 2, automatic.
  walks     pairs and triplets, D = 1, 2, 3, no box, a constant box, per-frame boxes, an odd P; the boundary triplets and pairs.
  The filter is skipped (and the bits are ta_pair_lifetime's) where the break criterion is the form criterion and gap = 0; a
  small call straight after a large one without ta_trim; float64 positions off any grid with non-dyadic cutoffs: everything
  equal to the CPU backend's; n_atoms dim >= 2^31 is refused before anything is allocated."""
import functools

import numpy as np
import pytest

import bond_ref as ref
import pair_ref
from test_vanhove_distinct_shapes import SLABS, slab_bits, stage, staged_bits
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu

CUTS = dict(r_break=ref.R_BREAK, cos_cut=ref.COS_CUT, cos_break=ref.COS_BREAK)


def timeline(c):
    return [n for n, _ in c.kernel_timeline(4096)]


def run_bond(c, dtype, x, fft, bonds, r_cut, want, filtered, repeat=2, **kw):
    """ta_bond_lifetime_staged into a caller's buffers, `repeat` times, and ta_bond_lifetime: all bit-equal; against want =
    (ci, runs, nb, ...) of pair_ref.sums (None: not compared); filtered: whether the call needs k_pair_filter"""
    import torch

    T = x.shape[0]
    runs = []
    for _ in range(repeat):
        d_ci = torch.full((T,), -7.0, dtype=torch.float64, device="cuda:0")
        d_runs = torch.full((T + 1,), -7, dtype=torch.int64, device="cuda:0")
        d_nb = torch.full((T,), -7.0, dtype=torch.float64, device="cuda:0")
        c.bond_lifetime_staged(fft, bonds, r_cut, d_ci=d_ci.data_ptr(), d_runs=d_runs.data_ptr(), d_nb=d_nb.data_ptr(), **kw)
        torch.cuda.synchronize()
        runs.append((d_ci.cpu().numpy(), d_runs.cpu().numpy(), d_nb.cpu().numpy()))
        names = timeline(c)
        assert "k_bond_series" in names and "k_pair_runs" in names and "k_pair_reduce" in names, names
        assert ("k_pair_filter" in names) == filtered, (filtered, names)
        assert "k_pair_series" not in names and "k_widen_f32" not in names, names
    for r in runs[1:]:
        assert all(np.array_equal(p, q) for p, q in zip(runs[0], r)), "repeat runs differ"
    host = c.bond_lifetime(fft, bonds, r_cut, **kw)
    assert all(np.array_equal(p, q) for p, q in zip(runs[0], host)), "the host-facing entry differs from the staged one"
    ci, rl, nb = runs[0]
    if want is not None:
        assert np.array_equal(rl, want[1]), np.flatnonzero(rl != want[1])[:5]
        assert np.array_equal(nb, want[2]), np.flatnonzero(nb != want[2])[:5]
        if fft:
            err = float(np.max(np.abs(ci - want[0])))
            print(f"    fft: max |ci - exact| = {err:.3e}, bound {1e-10 * max(float(want[0][0]), 1.0):.3e}")
            assert err <= 1e-10 * max(float(want[0][0]), 1.0)
        else:
            assert np.array_equal(ci, want[0]), np.flatnonzero(ci != want[0])[:5]
    assert np.array_equal(slab_bits(c, dtype), staged_bits(c, x, dtype)), "the staged slab's bits changed"
    return runs[0]


# ---- constructed patterns -------------------------------------------------------------------------------------------------
TS = [1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049]
GAPS = [0, 1, 2, 63]


@functools.lru_cache(maxsize=None)
def pattern_sums(T, gap):
    """(levels (n, T), [pair_ref.sums of each filtered row alone]): the sums of a call add up over its bonds"""
    lv = ref.constructed_levels(T, gap)
    g = ref.filtered(lv, gap)
    return lv, [ref.sums(row[None, :]) for row in g]


def pattern_case(T, gap, which):
    lv, per_row = pattern_sums(T, gap)
    x, bonds = ref.pattern_positions(lv[which])
    return x, bonds, [sum(per_row[k][i] for k in which) for i in range(3)]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T", TS)
def test_constructed_patterns(T, dtype):
    c = _lib.Context(0)
    try:
        for gap in GAPS:
            n = pattern_sums(T, gap)[0].shape[0]
            for which in (np.arange(n), np.arange(1) + gap % n, np.arange(2) + 9, np.arange(3) + 12, np.arange(129) % n):
                x, bonds, want = pattern_case(T, gap, which % n)
                stage(c, x, dtype)
                first = which.size == n
                for fft in (0, 1) if first else (0,):
                    run_bond(c, dtype, x, fft, bonds, 0.5, want, True, repeat=2 if first else 1, r_break=0.75, gap=gap)
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_pair_chunks_bit_equal(dtype):
    T, P, gap = 1025, 129, 2
    which = np.arange(P) % pattern_sums(T, gap)[0].shape[0]
    x, bonds, want = pattern_case(T, gap, which)
    c = stage(_lib.Context(0), x, dtype)
    try:
        runs = []
        for chunk, launches in ((1, 129), (2, 65), (0, 1), (1000, 1)):
            c.set_option("pair_chunk", chunk)
            runs.append(run_bond(c, dtype, x, 0, bonds, 0.5, want, True, repeat=1, r_break=0.75, gap=gap))
            assert c.kernel_launches("k_bond_series") == launches == c.kernel_launches("k_pair_filter")
            assert c.kernel_launches("k_pair_runs") == launches
        for r in runs[1:]:
            assert all(np.array_equal(p, q) for p, q in zip(runs[0], r))
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_filter_runs_exactly_when_needed(dtype):
    """gap = 0 with the break criterion equal to the form criterion: no k_pair_filter launch, and with n_at = 2 the bits of
    ta_pair_lifetime; any one of gap, r_break and (triplets) cos_break apart from it: the launch"""
    x, a, b, dims, axes, pairs, sums = pair_ref.case(65, 40, 3, "explicit", True, 1)
    c = stage(_lib.Context(0), x, dtype)
    try:
        box = dict(dimensions=dims, axes=axes)
        for fft in (0, 1):
            got = run_bond(c, dtype, x, fft, pairs, pair_ref.R_CUT, sums, False, cos_cut=3.0, cos_break=np.nan, **box)
            want = c.pair_lifetime(fft, pair_ref.R_CUT, pairs, **box)
            assert all(np.array_equal(p, q) for p, q in zip(got, want)), "not the bits of ta_pair_lifetime"
        run_bond(c, dtype, x, 0, pairs, pair_ref.R_CUT, None, True, repeat=1, gap=1, **box)
        run_bond(c, dtype, x, 0, pairs, 0.75, None, True, repeat=1, r_break=1.0, **box)
        run_bond(c, dtype, x, 0, pairs, pair_ref.R_CUT, None, False, repeat=1, cos_cut=-0.5, cos_break=-0.25, **box)  # (pairs: ignored)
    finally:
        c.close()
    x, bonds, dims, axes, s, _ = ref.case(65, 24, 3, 3, True, 0)
    c = stage(_lib.Context(0), x, dtype)
    try:
        box = dict(dimensions=dims, axes=axes)
        form_only = pair_ref.sums(s == 2)
        run_bond(c, dtype, x, 0, bonds, ref.R_CUT, form_only, False, cos_cut=ref.COS_CUT, **box)
        run_bond(c, dtype, x, 0, bonds, ref.R_CUT, form_only, False, cos_cut=ref.COS_CUT, cos_break=ref.COS_CUT, r_break=ref.R_CUT, **box)
        run_bond(c, dtype, x, 0, bonds, ref.R_CUT, None, True, repeat=1, cos_cut=ref.COS_CUT, cos_break=ref.COS_BREAK, **box)
    finally:
        c.close()


# ---- walks, boxes, boundaries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("n_at", [2, 3])
def test_walks_and_boxes(n_at, D, dtype):
    """walks of 65 frames, 95 bonds (the phantom column), without a box, in the constant box and in per-frame boxes; D = 2 on
    the box axes {0, 2}, D = 1 on axis 1"""
    for boxed in (False, True, "frames"):
        x, bonds, dims, axes, s, want = ref.case(65, 24, D, n_at, boxed, 2, P=95)
        c = stage(_lib.Context(0), x, dtype)
        try:
            run_bond(c, dtype, x, 0, bonds, ref.R_CUT, want, True, gap=2, dimensions=dims, axes=axes, **CUTS)
            run_bond(c, dtype, x, 1, bonds, ref.R_CUT, want, True, repeat=1, gap=2, dimensions=dims, axes=axes, **CUTS)
        finally:
            c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_boundaries(dtype):
    """triplets exactly on cos_cut are bonded, pairs exactly on r_cut and r_break are not"""
    for (x, bonds), levels in ((ref.boundary_triplets(), [2, 0, 2, 1]), (ref.boundary_pairs(), [1, 0, 2])):
        c = stage(_lib.Context(0), x, dtype)
        try:
            for n, level in enumerate(levels):
                got = run_bond(c, dtype, x, 0, bonds[n:n + 1], ref.R_CUT, None, True, repeat=1, **CUTS)
                assert got[2][0] == (level == 2), (n, level)
                got = run_bond(c, dtype, x, 0, bonds[n:n + 1], ref.R_BREAK, None, False, repeat=1, cos_cut=ref.COS_BREAK)
                assert got[2][0] == (level >= 1), (n, level)
        finally:
            c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_stale_scratch(dtype):
    """a small call, a larger one, then the small one again on ONE context without ta_trim"""
    c = _lib.Context(0)
    try:
        for T, A in ((7, 12), (131, 30), (7, 12)):
            x, bonds, dims, axes, s, want = ref.case(T, A, 3, 3, True, 1)
            stage(c, x, dtype)
            run_bond(c, dtype, x, 0, bonds, ref.R_CUT, want, True, repeat=1, gap=1, dimensions=dims, axes=axes, **CUTS)
    finally:
        c.close()


def test_gpu_equals_cpu_backend():
    """float64 values off any grid in the non-dyadic box (3.3, 2.9, 4.1) with non-dyadic cutoffs and cosines: both backends
    follow bond_math.hpp, so runs, and ci and nb with fft = 0, are equal -- no tolerance, no excluded bonds"""
    rng = np.random.default_rng(17)
    T, A, D = 131, 300, 3
    x = np.cumsum(rng.normal(scale=0.1, size=(T, A, D)), axis=0) + rng.uniform(0, 50, size=(1, A, D))
    kw = dict(dimensions=pair_ref.dimensions((3.3, 2.9, 4.1), T), r_break=1.4, cos_cut=np.cos(np.deg2rad(150.0)),
              cos_break=np.cos(np.deg2rad(125.0)), gap=3)
    cpu = _lib.Context("cpu")
    c = stage(_lib.Context(0), x, np.float64)
    try:
        (view,) = cpu.stage_alloc(T, A, D, dtype=np.float64)
        view[:] = x
        cpu.stage_commit(0, T)
        for n_at in (2, 3):
            bonds = np.stack([rng.permutation(A)[:n_at] for _ in range(2001)]).astype(np.int32)
            w_ci, w_runs, w_nb = cpu.bond_lifetime(0, bonds, 1.1, **kw)
            assert w_nb.sum() > 1000
            ci, runs, nb = run_bond(c, np.float64, x, 0, bonds, 1.1, None, True, **kw)
            assert np.array_equal(runs, w_runs) and np.array_equal(ci, w_ci) and np.array_equal(nb, w_nb)
    finally:
        c.close()
        cpu.close()


def test_refuses_2_pow_31_columns():
    """n_atoms dim >= 2^31: TA_E_INVALID before anything is allocated or written (a device-only slab that is never filled;
    "fail_alloc_after" 1 would turn the call's first workspace request into TA_E_NOMEM: the refusal comes first)"""
    import torch

    c = _lib.Context(0)
    try:
        c.set_option("stage_device_f32", 1)
        c.stage_alloc_device(1, 2 ** 30, 2)
        out = torch.full((2,), -7, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        c.set_option("fail_alloc_after", 1)
        with pytest.raises(_lib.TAError, match="bond_lifetime: n_atoms \\* dim must be below 2\\^31") as e:
            c.bond_lifetime_staged(0, np.array([[0, 1, 2]]), 0.5, cos_cut=-0.5, d_runs=out.data_ptr())
        assert e.value.code == -1
        c.set_option("fail_alloc_after", 0)
        torch.cuda.synchronize()
        assert bool((out == -7).all())
    finally:
        c.close()
