"""k_species_sort and the per-species lag sums at shapes that reach every branch, through the C-ABI (ta_species_self_staged,
ta_species_self_dev, ta_group_species_self), GPU only.  Every shape runs with both quantities (the MSD of species_walk
positions, the VACF of species_velocities), both fft and on a float64 AND a float32 device slab holding the same values
(rounded to float32 first), asserts k_species_sort in the kernel timeline and that no widening kernel ran, that repeat
runs agree bit for bit, that the staged slab's padding is still zero, and compares every species with the reference of
species_self_ref at the lags of lag_sample: within 1e-10 of max_k |self_s(k)|.

  * column pairs that straddle two atoms OF DIFFERENT SPECIES (D = 3, labels alternating), blocks with an odd column count
    (a phantom column per block: D = 1 with five species has several), D = 2 and D = 1;
  * S = 1 (the sort is the identity layout) up to S = 8, equal and very unequal block sizes, a label no atom carries, a
    species of exactly one atom (a unit with one atom and nothing else);
  * 1, 2, 3, 48, 64, 65, 100, 513 frames: k_short, k_mid and the 512-point boundary of the lag-sum dispatch on sub-slabs;
    odd frame counts (the float32 load whose second row is row T); 20000 frames: 20 frame blocks, an outer-radix plan;
  * a scratch slab left over from a larger call (phantom columns and tail rows are written, not assumed);
  * bit-exact identities: each species against the lag sum of its own atoms staged alone, S = 1 against
    ta_conductivity_staged's self term, the frame-major entry against the staged one."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import scale_rel_err
from species_self_ref import SELF_MSD, SELF_VACF, assert_self, self_at_lags, self_case, self_inputs
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu

SLABS = [pytest.param(np.float64, id="slab64"), pytest.param(np.float32, id="slab32")]
QUANTITIES = [pytest.param(SELF_MSD, id="msd"), pytest.param(SELF_VACF, id="vacf")]


def stage(c, y, dtype):
    """y staged in `dtype` on context c (replacing what it held), kept in that element type on the device"""
    T, A, D = y.shape
    c.set_option("stage_device_f32", int(dtype == np.float32))
    (view,) = c.stage_alloc(T, A, D, dtype=dtype)
    view[:] = y
    c.stage_commit(0, T)
    c.set_option("timeline", 1)
    return c


def staged_context(y, dtype):
    return stage(_lib.Context(0), y, dtype)


def timeline(c):
    return [n for n, _ in c.kernel_timeline(64)]


def run_staged(c, quantity, fft, lab, w, S, repeat=2):
    """ta_species_self_staged into a caller buffer, twice: the runs must agree bit for bit.  -> (S, T)"""
    import torch

    dev = torch.device("cuda", 0)
    T = c.shape[0]
    d_w = torch.from_numpy(np.array(w, dtype=np.float64)).to(dev) if w is not None else None
    runs = []
    for _ in range(repeat):
        out = torch.full((S, T), np.nan, dtype=torch.float64, device=dev)
        c.species_self_staged(quantity, fft, S, lab, out.data_ptr(), d_w.data_ptr() if d_w is not None else 0)
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy())
    assert all(np.array_equal(runs[0], r) for r in runs[1:]), "repeat runs differ"
    return runs[0]


def slab_padding(c, dtype):
    """(rows T ... pitch - 1 of every pair, the phantom column's rows or None) of the raw staged device slab"""
    T, A, D = c.shape
    ptr, pitch, n_pairs = c.stage_device(0)
    raw = np.empty(n_pairs * pitch * 2, dtype=dtype)
    L = _lib.lib()
    L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert L.hipMemcpy(raw.ctypes.data, ptr, raw.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    raw = raw.reshape(n_pairs, pitch, 2)
    return raw[:, T:, :], (raw[-1, :, 1] if (A * D) % 2 else None)


def lag_kernels(quantity, T, fft):
    """a kernel only the lag-sum dispatch of this length launches on a float64 sub-slab (api.hip: msd_impl, fft_impl,
    direct_impl with the default options)"""
    if T <= 48 or (T <= 64 and (not fft or quantity == SELF_MSD)):
        return {"k_short"}
    if T <= 64:
        return {"k_w1_accum"}
    if not fft:
        if quantity == SELF_MSD:
            return {"k_mid"} if T <= 512 else {"k_direct"}
        return {"k_mid"} if 97 <= T <= 512 else set()  # (beyond: the matrix-core forms, named by the VACF tests)
    first = {"k_msd_prepare"} if quantity == SELF_MSD else set()
    return first | ({"k_w1_accum"} if T <= 512 else {"k_wsplit_accum", "k_winverse"})


def check(c, dtype, quantity, y, lab, w, S, lags, want, what):
    for fft in (1, 0):
        got = run_staged(c, quantity, fft, lab, w, S)
        names = timeline(c)
        assert "k_species_sort" in names, names
        assert "k_widen_f32" not in names, names  # the slab is read in its own element type
        assert lag_kernels(quantity, y.shape[0], fft) <= set(names), (fft, names)
        if quantity == SELF_MSD:
            assert not got[:, 0].any(), "the MSD's lag 0 must be exactly 0"
        assert_self(got, want, lags, what=f"{what} fft={fft}")
    tail, phantom = slab_padding(c, dtype)
    assert not tail.any(), "rows T ... pitch - 1 of the staged slab must still be zero"
    assert phantom is None or not phantom.any(), "the staged slab's phantom column must still be zero"
    return got


# (id, T, A, D, S, labels)
SHAPE_CASES = [
    ("straddle_odd_block_d3", 1100, 1501, 3, 2, "alt"),
    ("straddle_d3_s3", 1101, 1501, 3, 3, "alt"),
    ("d2", 2049, 1100, 2, 4, "alt"),
    ("odd_blocks_d1", 2048, 2101, 1, 5, "alt"),
    ("s1", 1100, 1501, 3, 1, "rand"),
    ("s8", 1101, 1501, 3, 8, "rand"),
    ("t1", 1, 700, 3, 3, "rand"),
    ("t2", 2, 700, 3, 3, "rand"),
    ("t3", 3, 700, 3, 3, "rand"),
    ("t48", 48, 700, 3, 3, "rand"),
    ("t64", 64, 700, 3, 3, "rand"),
    ("t65", 65, 700, 3, 3, "rand"),
    ("t100", 100, 700, 3, 3, "rand"),
    ("t513", 513, 700, 3, 3, "rand"),
    ("long_outer_radix", 20000, 211, 3, 2, "rand"),
]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("quantity", QUANTITIES)
@pytest.mark.parametrize("T,A,D,S,labels", [pytest.param(*c[1:], id=f"{c[0]}-T{c[1]}-A{c[2]}-D{c[3]}-S{c[4]}") for c in SHAPE_CASES])
def test_species_self_shapes(T, A, D, S, labels, quantity, dtype):
    y, lab, w, lags, want = self_case(T, A, D, S, labels, quantity)
    c = staged_context(y, dtype)
    try:
        got = check(c, dtype, quantity, y, lab, w, S, lags, want, "")
        host, counts = c.species_self(quantity, 0, lab, n_species=S, weights=w)  # the host-facing call
        assert np.array_equal(host, got) and np.array_equal(counts, np.bincount(lab, minlength=S))
    finally:
        c.close()


@functools.lru_cache(maxsize=2)
def gap_case(quantity, kind):
    """A = 701, D = 3, T = 300, S = 4: "empty": no atom carries label 2; "single": species 1 is exactly one atom"""
    T, A, D, S = 300, 701, 3, 4
    y, _, w = self_inputs(T, A, D, S, "rand", quantity)
    if kind == "empty":
        lab = np.array([0, 1, 3], dtype=np.int32)[np.arange(A) % 3]
    else:
        lab = np.array([0, 2, 3], dtype=np.int32)[np.arange(A) % 3]
        lab[350] = 1
    lags = np.arange(T)
    return y, lab, w, lags, self_at_lags(y, lab, w, S, quantity, lags)


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("quantity", QUANTITIES)
@pytest.mark.parametrize("kind", ["empty", "single"])
def test_species_self_empty_and_single(kind, quantity, dtype):
    y, lab, w, lags, want = gap_case(quantity, kind)
    counts = np.bincount(lab, minlength=4)
    assert counts[2] == 0 if kind == "empty" else counts[1] == 1
    c = staged_context(y, dtype)
    try:
        got = check(c, dtype, quantity, y, lab, w, 4, lags, want, kind)
        if kind == "empty":
            assert not got[2].any(), "a label no atom carries: exact zeros in its row"
    finally:
        c.close()


@pytest.mark.parametrize("quantity", QUANTITIES)
def test_species_self_stale_scratch(quantity):
    """A larger call (eight blocks, 1101 frames) then a smaller one (two blocks, 1100 frames: the same pitch) on ONE context
    without ta_trim: the second call's phantom column and its rows 1100 ... 1103 lie where the first left values."""
    first = self_case(1101, 1501, 3, 8, "rand", quantity)
    second = self_case(1100, 1501, 3, 2, "alt", quantity)
    c = _lib.Context(0)
    try:
        for (y, lab, w, lags, want), S in ((first, 8), (second, 2)):
            stage(c, y, np.float64)
            check(c, np.float64, quantity, y, lab, w, S, lags, want, f"S={S}")
    finally:
        c.close()


def lone_lag_sum(y, quantity, fft):
    """the lag sum ta_msd_staged / ta_vacf_fft_staged / ta_vacf_direct_staged give for y (T, N, D) staged alone"""
    import torch

    c = staged_context(y, np.float64)
    try:
        out = torch.full((y.shape[0],), np.nan, dtype=torch.float64, device="cuda:0")
        if quantity == SELF_MSD:
            c.msd_staged(fft, out.data_ptr())
        elif fft:
            c.vacf_fft_staged(out.data_ptr())
        else:
            c.vacf_direct_staged(out.data_ptr())
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        c.close()


@pytest.mark.parametrize("quantity", QUANTITIES)
@pytest.mark.parametrize("T,A,D,S", [(1101, 1501, 3, 3), (48, 700, 3, 3), (100, 700, 3, 3), (513, 700, 2, 3), (2048, 701, 1, 4)])
def test_species_self_permutation_bit_exact(T, A, D, S, quantity):
    """Each species' row equals, BIT FOR BIT, the lag sum of w (x - x[0]) / w v of that species' atoms alone and in order,
    formed in NumPy float64 and staged in a second context: the values, (T, N_s, D) and the dispatch are the same.  The
    weights are +-powers of two, so NumPy's products are the kernel's."""
    y, lab, w = self_inputs(T, A, D, S, "rand", quantity)
    c = staged_context(y, np.float64)
    try:
        for fft in (1, 0):
            got = run_staged(c, quantity, fft, lab, w, S, repeat=1)
            for s in range(S):
                sel = np.flatnonzero(lab == s)
                ys = (y[:, sel] - y[0, sel] if quantity == SELF_MSD else y[:, sel]) * w[sel][None, :, None]
                assert np.array_equal(got[s], lone_lag_sum(ys, quantity, fft)), (fft, s, sel.size)
    finally:
        c.close()


@pytest.mark.parametrize("T,A,D", [(1100, 1501, 3), (100, 701, 1)])
def test_species_self_is_conductivity_self_term(T, A, D):
    """S = 1 with weights = q: TA_SELF_MSD is ta_conductivity_staged's self lag sum bit for bit (the same W, the same call)"""
    import torch

    y, lab, _ = self_inputs(T, A, D, 1, "rand", SELF_MSD)
    q = np.where(np.arange(A) % 2 == 0, 1.0, -0.8)
    c = staged_context(y, np.float64)
    try:
        d_q = torch.from_numpy(q).to("cuda:0")
        for fft in (1, 0):
            got = run_staged(c, SELF_MSD, fft, lab, q, 1, repeat=1)
            m = torch.zeros((T, D), dtype=torch.float64, device="cuda:0")
            slf = torch.full((T,), np.nan, dtype=torch.float64, device="cuda:0")
            c.conductivity_staged(fft, d_q.data_ptr(), m.data_ptr(), 0, slf.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(got[0], slf.cpu().numpy()), fft
    finally:
        c.close()


@pytest.mark.parametrize("quantity", QUANTITIES)
def test_species_self_partition(quantity):
    """sum_s self[s] against the one-species result of the same atoms: within 1e-10 of its scale"""
    T, A, D, S = 1101, 1501, 3, 8
    y, lab, w = self_inputs(T, A, D, S, "rand", quantity)
    c = staged_context(y, np.float64)
    try:
        for fft in (1, 0):
            parts = run_staged(c, quantity, fft, lab, w, S, repeat=1)
            whole = run_staged(c, quantity, fft, np.zeros(A, dtype=np.int32), w, 1, repeat=1)
            err = scale_rel_err(parts.sum(axis=0), whole[0])
            print(f"    partition fft={fft}: {err:.3e}")
            assert err <= 1e-10
    finally:
        c.close()


@pytest.mark.parametrize("quantity", QUANTITIES)
def test_species_self_dev_wide_rows(quantity):
    """ta_species_self_dev on a frame-major tensor with ld_row > n_atoms dim equals the staged path bit for bit"""
    import torch

    T, A, D, S = 1101, 301, 3, 3
    ld_row = A * D + 7
    y, lab, w = self_inputs(T, A, D, S, "rand", quantity)
    wide = np.full((T, ld_row), 7.5e3)
    wide[:, :A * D] = y.reshape(T, A * D)
    d_y, d_w = torch.from_numpy(wide).to("cuda:0"), torch.from_numpy(np.array(w)).to("cuda:0")
    c = staged_context(y, np.float64)
    try:
        for fft in (1, 0):
            want = run_staged(c, quantity, fft, lab, w, S)
            out = torch.full((S, T), np.nan, dtype=torch.float64, device="cuda:0")
            c.species_self_dev(d_y.data_ptr(), T, A, D, ld_row, quantity, fft, S, lab, out.data_ptr(), d_w.data_ptr())
            torch.cuda.synchronize()
            names = timeline(c)
            assert "k_relayout" in names and "k_species_sort" in names, names
            assert np.array_equal(out.cpu().numpy(), want), fft
    finally:
        c.close()


@pytest.mark.parametrize("quantity", QUANTITIES)
def test_group_species_self(quantity):
    """ta_group_species_self on devices [0, 0] (751 + 751 atoms: odd member column counts) against one context: the
    members' rows and counts add up"""
    T, A, D, S = 700, 1502, 3, 3
    y, lab, w = self_inputs(T, A, D, S, "rand", quantity)
    c = staged_context(y, np.float64)
    g = _lib.Group([0, 0])
    try:
        (views,) = g.stage_alloc(T, A, D)
        for (lo, hi), view in zip(g.shards, views):
            assert ((hi - lo) * D) % 2 == 1
            view[:] = y[:, lo:hi]
        g.stage_commit(0, T)
        for fft in (1, 0):
            one, counts = c.species_self(quantity, fft, lab, n_species=S, weights=w)
            both, counts2 = g.species_self(quantity, fft, lab, n_species=S, weights=w)
            assert np.array_equal(counts, counts2) and np.array_equal(counts, np.bincount(lab, minlength=S))
            for s in range(S):
                assert scale_rel_err(both[s], one[s]) <= 1e-10, (fft, s)
    finally:
        g.close()
        c.close()
