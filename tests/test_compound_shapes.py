"""k_compound through the C-ABI (ta_compound) at the smallest shapes at which it can go wrong, GPU only.  Every case runs on
a float64 AND a float32 device slab holding the same values (rounded to float32 first), with and without frame weights,
and asserts k_compound in the kernel timeline and that no widening kernel ran, that a second run from a fresh staging
gives the same bits, that the new slab's tail rows and phantom column are zero, and compares every element with
compound_ref's long-double reference within its derived bar.

  * dim 1, 2, 3; an even and an odd compound count (a one-compound last unit); n_compounds * dim odd (a phantom column);
  * compounds of 1, 2, 3 and 15 atoms and one of 300 in one plan, members contiguous; members interleaved (atom n in compound
    n % C: with dim = 3 every straddling source pair holds two compounds); a few atoms that no compound names;
  * 1, 2, 3, 1023, 1024, 1025 and 2049 frames (the frame-block edge; odd counts on the float32 slab: the load whose second
    row is row T); around 1500 atoms; a context that held a larger slab before, without ta_trim;
  * bit-exact identities: the identity plan, power-of-two weights, the lag sums on the compound slab against the same values
    staged afresh; the CPU backend's slab within the bar;
  * ta_species_self and ta_onsager after ta_compound, and the accepting classes on device 0."""
import numpy as np
import pytest

from compound_ref import assert_compound, compound_case, compound_ref, positions
from conftest import scale_rel_err
from onsager_ref import assert_cross, assert_moments, cross_ref, moments_ref
from species_self_ref import SELF_MSD, SELF_VACF, assert_self, self_at_lags
from test_compound import BOX, molecules
from test_species_self_shapes import slab_padding, stage, staged_context, timeline
from transport_analysis_amd import ConductivityGreenKubo, EinsteinMSD, OnsagerGreenKubo, OnsagerHelfand, _lib
from transport_analysis_amd._mini_mda import ArrayUniverse
from transport_analysis_amd.compound import compound_plan

pytestmark = pytest.mark.gpu

SLABS = [pytest.param(np.float64, id="slab64"), pytest.param(np.float32, id="slab32")]


def read_slab(c):
    """ta_stage_read_dev of slab 0: (T, n, D) float64"""
    import torch

    T, A, D = c.shape
    out = torch.full((T, A * D), float("nan"), dtype=torch.float64, device="cuda:0")
    c.stage_read_dev(0, out.data_ptr(), A * D)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(T, A, D)


def compound_once(c, off, mem, w, frame):
    """ta_compound on a staged context with the checks every run gets: -> the new slab (T, C, D)"""
    T, _, D = c.shape
    assert c.compound(off, mem, w, frame) is None  # a GPU context has no host slab to hand out
    names = timeline(c)
    assert "k_compound" in names and "k_widen_f32" not in names, names
    if frame is None:
        assert "k_species_current" not in names, names
    else:
        assert names.index("k_species_current") < names.index("k_compound"), names
    assert c.shape == (T, off.size - 1, D)
    tail, phantom = slab_padding(c, np.float64)
    assert not tail.any(), "rows T ... pitch - 1 of the new slab must be zero"
    assert ((off.size - 1) * D) % 2 == (phantom is not None)
    assert phantom is None or not phantom.any(), "the new slab's phantom column must be zero"
    return read_slab(c)


def compound_twice(x, dtype, off, mem, w, frame):
    runs = []
    for _ in range(2):
        c = staged_context(x, dtype)
        try:
            runs.append(compound_once(c, off, mem, w, frame))
        finally:
            c.close()
    assert np.array_equal(runs[0], runs[1]), "a second run from a fresh staging differs"
    return runs[0]


# (id, T, A, D, plan, odd compound count)
SHAPE_CASES = [
    ("t1", 1, 1500, 3, "mixed", False),
    ("t2", 2, 1500, 3, "inter", True),          # 101 compounds x 3: a phantom column
    ("t3", 3, 1500, 2, "mixed", True),
    ("t1023", 1023, 1501, 3, "mixed", True),    # phantom column, one-compound last unit
    ("t1024", 1024, 1500, 3, "inter", False),
    ("t1025", 1025, 1500, 1, "mixed", True),    # dim 1, phantom column
    ("t2049", 2049, 1500, 3, "inter", True),    # three frame blocks
    ("d2", 1100, 1500, 2, "inter", False),
    ("d1_even", 1100, 1501, 1, "inter", False),
    ("d3_mixed_even", 1100, 1500, 3, "mixed", False),
]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T,A,D,kind,odd", [pytest.param(*c[1:], id=f"{c[0]}-T{c[1]}-A{c[2]}-D{c[3]}-{c[4]}") for c in SHAPE_CASES])
def test_compound_shapes(T, A, D, kind, odd, dtype):
    x, off, mem, w, u, plain, framed = compound_case(T, A, D, kind, odd)
    if kind == "mixed":
        sizes = set(np.diff(off).tolist())
        assert {1, 2, 3, 15, 300} <= sizes, sizes
    assert off[-1] < A  # some atoms belong to no compound
    for frame, (want, bar) in ((None, plain), (u, framed)):
        got = compound_twice(x, dtype, off, mem, w, frame)
        assert_compound(got, want, bar, f"T={T} A={A} D={D} {kind} {np.dtype(dtype).name} frame={'yes' if frame is not None else 'no'}")


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T,A,D", [(1025, 1501, 3), (1023, 1500, 2), (3, 1501, 1)])
def test_compound_bit_exact_identities(T, A, D, dtype):
    """(a) every atom its own compound, weight 1, no frame: ta_stage_read_dev of the input bit for bit; (b) one member per
    compound with +-power-of-two weights, in a permuted order: NumPy's products bit for bit"""
    x = positions(T, A, D, seed=T + A + D)
    c = staged_context(x, dtype)
    try:
        before = read_slab(c)
        assert np.array_equal(before, x)
        assert np.array_equal(compound_once(c, np.arange(A + 1), np.arange(A), None, None), before)
    finally:
        c.close()
    w = 2.0 ** np.random.default_rng(3).integers(-3, 4, size=A) * np.where(np.arange(A) % 3 == 0, -1.0, 1.0)
    perm = np.random.default_rng(4).permutation(A)
    c = staged_context(x, dtype)
    try:
        assert np.array_equal(compound_once(c, np.arange(A + 1), perm, w, None), x[:, perm] * w[None, :, None])
    finally:
        c.close()


@pytest.mark.parametrize("T,A,D,kind,odd", [(1100, 1500, 3, "mixed", False), (1023, 1501, 3, "mixed", True), (100, 1500, 2, "inter", False)])
def test_lag_sums_on_the_compound_slab_bit_exact(T, A, D, kind, odd):
    """(c) ta_msd_staged and ta_vacf_fft_staged on the compound slab equal, bit for bit, the same calls on a second context
    staged with that slab's values: the shape and the dispatch are the same"""
    import torch

    x, off, mem, w, u, _, _ = compound_case(T, A, D, kind, odd)

    def lag_sums(c):
        out = []
        for call in (lambda p: c.msd_staged(1, p), lambda p: c.msd_staged(0, p), lambda p: c.vacf_fft_staged(p)):
            d = torch.full((T,), float("nan"), dtype=torch.float64, device="cuda:0")
            call(d.data_ptr())
            torch.cuda.synchronize()
            out.append(d.cpu().numpy())
        return out

    c = staged_context(x, np.float32)
    try:
        slab = compound_once(c, off, mem, w, u)
        first = lag_sums(c)
    finally:
        c.close()
    c = staged_context(slab, np.float64)
    try:
        second = lag_sums(c)
    finally:
        c.close()
    for a, b in zip(first, second):
        assert np.isfinite(a).all() and np.array_equal(a, b)


@pytest.mark.parametrize("dtype", SLABS)
def test_gpu_slab_against_cpu_backend(dtype):
    """(d) the GPU slab against the CPU backend's h_out: within the derived bar"""
    x, off, mem, w, u, plain, framed = compound_case(1023, 1501, 3, "mixed", True)
    for frame, (_, bar) in ((None, plain), (u, framed)):
        cpu = _lib.Context("cpu")
        try:
            (view,) = cpu.stage_alloc(*x.shape, dtype=dtype)
            view[:] = x
            cpu.stage_commit(0, x.shape[0])
            host = np.array(cpu.compound(off, mem, w, frame))
        finally:
            cpu.close()
        c = staged_context(x, dtype)
        try:
            got = compound_once(c, off, mem, w, frame)
        finally:
            c.close()
        assert_compound(got, host, bar, f"gpu against cpu {np.dtype(dtype).name} frame={'yes' if frame is not None else 'no'}")


@pytest.mark.parametrize("dtype", SLABS)
def test_compound_after_a_larger_slab(dtype):
    """A larger slab (2049 frames, 101 compounds) then a smaller one (1023 frames) on ONE context without ta_trim"""
    big, small = compound_case(2049, 1500, 3, "inter", True), compound_case(1023, 1501, 3, "mixed", True)
    c = _lib.Context(0)
    try:
        for x, off, mem, w, u, _, (want, bar) in (big, small):
            stage(c, x, dtype)
            assert_compound(compound_once(c, off, mem, w, u), want, bar, f"T={x.shape[0]} on a reused context")
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_species_self_and_onsager_after_compound(dtype):
    """ta_species_self and ta_onsager on the compound slab against species_self_ref / onsager_ref on the reference centres"""
    T, A, D, S = 300, 1500, 3, 3
    x, off, mem, w, u, (com, _), _ = compound_case(T, A, D, "mixed", False)
    C = off.size - 1
    lab = (np.arange(C) % S).astype(np.int32)
    z = np.array([0.5, 1.0, 2.0])[np.arange(C) % 3][::-1].copy()
    lags = np.arange(T)
    c = staged_context(x, dtype)
    try:
        compound_once(c, off, mem, w, None)
        for fft in (1, 0):
            got, counts = c.species_self(SELF_MSD, fft, lab, n_species=S, weights=z)
            assert np.array_equal(counts, np.bincount(lab, minlength=S))
            assert_self(got, self_at_lags(com, lab, z, S, SELF_MSD, lags), lags, what=f"msd after compound fft={fft}")
            got, _ = c.species_self(SELF_VACF, fft, lab, n_species=S, weights=z)
            assert_self(got, self_at_lags(com, lab, z, S, SELF_VACF, lags), lags, what=f"vacf after compound fft={fft}")
            want_m, scale = moments_ref(com, lab, z, S)
            m, cr = c.onsager(fft, lab, n_species=S, weights=z)
            assert_moments(m, want_m, scale)
            assert_cross(cr, cross_ref(want_m))
    finally:
        c.close()


# ---- the classes on device 0, mirroring tests/test_compound.py ---------------------------------------------------------------
N_MOL, T_CLS = 66, 300  # about 300 frames x 200 atoms


@pytest.mark.parametrize("fft", [True, False])
def test_einstein_msd_of_molecules_gpu(fft):
    x, labels, m, com = molecules(T_CLS, N_MOL)
    got = EinsteinMSD(ArrayUniverse(positions=x, masses=m), compound=labels, device=0, fft=fft).run()
    want = EinsteinMSD(ArrayUniverse(positions=com), device=0, fft=fft, stage_dtype=np.float64).run()
    assert got.n_particles == N_MOL and got.results.msds_by_particle.shape == (T_CLS, N_MOL)
    assert scale_rel_err(got.results.timeseries, want.results.timeseries) <= 1e-10
    assert scale_rel_err(got.results.msds_by_particle, want.results.msds_by_particle) <= 1e-10
    drift = np.cumsum(np.random.default_rng(5).integers(-128, 129, size=(T_CLS, 1, 3)), axis=0) / 64.0
    still = EinsteinMSD(ArrayUniverse(positions=x, masses=m), compound=labels, reference_frame="barycentric", device=0, fft=fft).run()
    moved = EinsteinMSD(ArrayUniverse(positions=x + drift, masses=m), compound=labels, reference_frame="barycentric", device=0,
                        fft=fft).run()
    scale = float(np.abs(still.results.timeseries).max())
    delta = float(compound_ref(x + drift, *compound_plan(labels, m)[1:], m / m.sum())[1].max())
    assert 2 * np.sqrt(scale) * delta <= 0.1 * 1e-10 * scale
    assert scale_rel_err(moved.results.timeseries, still.results.timeseries) <= 1e-10


@pytest.mark.parametrize("fft", [True, False])
@pytest.mark.parametrize("cls,key", [(OnsagerHelfand, "positions"), (OnsagerGreenKubo, "velocities")])
def test_onsager_of_molecules_gpu(cls, key, fft):
    x, labels, m, com = molecules(T_CLS, N_MOL)
    if key == "velocities":
        x, com = x - x[:1], com - com[:1]
    species = np.array(["anion", "cation", "solvent"])[np.arange(N_MOL) % 3]
    z = np.array([-1.0, 1.0, 0.5])[np.arange(N_MOL) % 3]
    got = cls(ArrayUniverse(**{key: x}, masses=m, dimensions=BOX).atoms, species[labels], compound=labels, weights=z,
              self_terms=True, fft=fft, device=0).run()
    want = cls(ArrayUniverse(**{key: com}, dimensions=BOX).atoms, species, weights=z, self_terms=True, fft=fft, device=0,
               stage_dtype=np.float64).run()
    assert np.array_equal(got.results.species_counts, want.results.species_counts)
    assert scale_rel_err(got.results.timeseries, want.results.timeseries) <= 1e-10
    assert scale_rel_err(got.results.timeseries_self, want.results.timeseries_self) <= 1e-10


def test_conductivity_green_kubo_of_molecules_gpu():
    x, labels, m, com = molecules(T_CLS, N_MOL)
    v, vcom = x - x[:1], com - com[:1]
    q = np.array([-0.5, 0.25, 1.0])[np.arange(x.shape[1]) % 3]
    got = ConductivityGreenKubo(ArrayUniverse(velocities=v, masses=m, charges=q, dimensions=BOX).atoms, compound=labels,
                                self_terms=True, device=0).run()
    want = ConductivityGreenKubo(ArrayUniverse(velocities=vcom, charges=np.bincount(labels, weights=q), dimensions=BOX).atoms,
                                 self_terms=True, device=0, stage_dtype=np.float64).run()
    assert scale_rel_err(got.results.timeseries, want.results.timeseries) <= 1e-10
    assert scale_rel_err(got.results.timeseries_self, want.results.timeseries_self) <= 1e-10
