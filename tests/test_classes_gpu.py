"""The analysis classes on the HIP path, GPU only: IntermediateScattering, CurrentCorrelation, VanHoveSelf, VanHoveDistinct,
PairLifetime, HydrogenBondLifetime, OrientationalCorrelation, DynamicSusceptibility, PartialScattering and
FourPointStructureFactor (and, staged in pieces, ShellResidence, ShellMSD and ShellOrientation) through StagedAnalysis._prepare,
_single_frame and _conclude -- pinned slabs filled by ta_stage_frame, stage_commit in pieces, "stage_device_f32" as
_set_options asks for it, the unwrap and ta_compound before the call, the host-facing entry and _store.

  A  the cases of the classes' CPU tests on device=0, with float32 and float64 staging: the SAME bodies (the functions of
     test_scattering.py, test_current_correlation.py, ... that take the placement keywords), so the same references, bars and
     printed figures.  Every run of a class in this module is watched (the fixture `watched`): with float32 staging the
     device slabs hold the staged float32 values AS float32 and no widening kernel ran in the call.  One case per class is
     staged in pieces of 32, 32 and 1 frames: the same bits as in one commit.
  B  the six collective classes on devices=[0, 0] (and on three members of which the first is empty), under distributed=True with
     two gloo ranks on the one GPU and more ranks than atoms, and with one nccl (RCCL) rank: every result against the
     reference over ALL atoms at the single-device bar, the integers equal to the single-device run's."""
import ctypes

import numpy as np
import pytest

import placement
import test_bond_lifetime
import test_current_correlation
import test_orientation
import test_overlap
import test_overlap_density
import test_pair_lifetime
import test_partial_scattering as test_partial  # (test_partial_scattering is a test of this module)
import test_scattering
import test_shell_msd
import test_shell_orientation
import test_shell_residence
import test_vanhove
import test_vanhove_distinct
from transport_analysis_amd import _base, _lib

pytestmark = pytest.mark.gpu

STAGING = [pytest.param(np.float32, id="stage32"), pytest.param(np.float64, id="stage64")]
COLLECTIVE = [test_scattering, test_current_correlation, test_vanhove, test_overlap, test_partial, test_overlap_density]
MODULE_IDS = ["scattering", "current", "vanhove_self", "overlap", "partial_scattering", "four_point"]
ATOMS = {test_scattering: 13, test_current_correlation: 33, test_vanhove: 13, test_overlap: 13,
         test_partial: 33, test_overlap_density: 13}  # odd: the blocks differ


def device_slab_bits(c, slab, dtype):
    """the raw device slab, padding included, read as `dtype` elements (float32: at most the slab's own bytes, whatever
    it holds)"""
    ptr, pitch, n_pairs = c.stage_device(slab)
    raw = np.empty(n_pairs * pitch * 2, dtype=dtype)
    L = _lib.lib()
    L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert L.hipMemcpy(raw.ctypes.data, ptr, raw.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return raw.view(np.uint32)


def pair_major_bits(c, slab, x):
    """the pair-major float32 layout of the host slab x (T, A, D): rows T ... pitch - 1 and the phantom column zero"""
    T, A, D = x.shape
    _, pitch, n_pairs = c.stage_device(slab)
    want = np.zeros((n_pairs * 2, pitch), dtype=np.float32)
    want[:A * D, :T] = x.reshape(T, A * D).T
    return np.ascontiguousarray(want.reshape(n_pairs, 2, pitch).transpose(0, 2, 1)).ravel().view(np.uint32)


@pytest.fixture(autouse=True)
def watched(monkeypatch):
    """Every context a class opens records its kernel timeline, and after every run on float32 slabs that are read as they
    are (no unwrap, no ta_compound: both leave float64 slabs) the device slabs are compared with the pinned host slabs --
    float32 elements, the same bits -- and the call's timeline has no widening kernel.  Returns the class names checked."""
    seen = []
    open_context, conclude = _base.open_context, _base.StagedAnalysis._conclude

    def open_with_timeline(devices, device):
        c = open_context(devices, device)
        if device != _lib.DEVICE_CPU:
            c.set_option("timeline", 1)
        return c

    def conclude_and_check(self):
        conclude(self)
        if self._device == _lib.DEVICE_CPU or self._pick_stage_dtype() != np.float32 or self._unwrap or self._plan is not None:
            return
        if self._devices is not None:
            members = [i for i, (lo, hi) in enumerate(self._ctx.shards) if hi > lo]
            pairs = [(self._ctx.member_context(i), views) for i, (views, _, _) in zip(members, self._targets)]
        else:
            pairs = [(self._ctx, self._targets[0][0])] if self._n_local else []
        for c, views in pairs:
            names = [n for n, _ in c.kernel_timeline(256)]
            assert names and "k_widen_f32" not in names, names
            for k, view in enumerate(views):
                assert view.dtype == np.float32
                assert np.array_equal(device_slab_bits(c, k, np.float32), pair_major_bits(c, k, np.asarray(view))), \
                    f"{type(self).__name__}: device slab {k} does not hold the staged float32 values as float32"
            seen.append(type(self).__name__)

    monkeypatch.setattr(_base, "open_context", open_with_timeline)
    monkeypatch.setattr(_base.StagedAnalysis, "_conclude", conclude_and_check)
    return seen


def on_gpu(dtype):
    return dict(device=0, stage_dtype=dtype)


def saw(watched, name, dtype):
    """with float32 staging the class's runs were checked by `watched`; with float64 staging there is nothing to check"""
    assert (name in watched) == (dtype == np.float32), watched


# ---- A: the CPU class tests' bodies on device 0 ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", STAGING)
def test_intermediate_scattering(dtype, watched):
    """explicit kvectors and q= / dq= of the box, fft True and False, coherent True and False, compound=; the wrapped walk with
    and without unwrap=True"""
    test_scattering.class_refusals_and_results(**on_gpu(dtype))
    test_scattering.wrapped_positions_need_no_unwrap(**on_gpu(dtype))
    saw(watched, "IntermediateScattering", dtype)


@pytest.mark.parametrize("dtype", STAGING)
def test_current_correlation_class(dtype, watched):
    """weights "mass", "charge", None and an array, dim_type "xyz", "xy" and "z", fft True and False, the shells of the box,
    unwrap=True"""
    test_current_correlation.class_normalisation_and_weights(**on_gpu(dtype))
    test_current_correlation.class_shell_means_and_volume(**on_gpu(dtype))
    test_current_correlation.class_wrapped_positions_need_no_unwrap(**on_gpu(dtype))
    saw(watched, "CurrentCorrelation", dtype)


@pytest.mark.parametrize("dtype", STAGING)
def test_vanhove_self(dtype, watched):
    """explicit lags and lags=None, d = 1, 2, 3, unwrap=True, compound= with reference_frame="barycentric": the counts equal,
    msd, r4 and alpha2 at the CPU tests' bars"""
    test_vanhove.static_atoms(**on_gpu(dtype))
    test_vanhove.normalisation(**on_gpu(dtype))
    test_vanhove.default_lags_are_log_lags(**on_gpu(dtype))
    test_vanhove.unwrap_gives_the_unwrapped_walk(**on_gpu(dtype))
    test_vanhove.compounds_and_barycentric_frame(**on_gpu(dtype))
    saw(watched, "VanHoveSelf", dtype)


@pytest.mark.parametrize("dtype", STAGING)
def test_dynamic_susceptibility(dtype, watched):
    test_overlap.class_against_reference(**on_gpu(dtype))
    test_overlap.class_scalar_cutoff_and_default_lags(**on_gpu(dtype))
    test_overlap.class_float32_staging_is_the_same(**on_gpu(dtype))
    test_overlap.unwrap_gives_the_unwrapped_walk(**on_gpu(dtype))
    test_overlap.compounds_with_dyadic_weights(**on_gpu(dtype))
    saw(watched, "DynamicSusceptibility", dtype)


@pytest.mark.parametrize("dtype", STAGING)
def test_partial_scattering(dtype, watched):
    """the shells of the box against IntermediateScattering on the same placement, fft True and False; one species; total()
    and the normalisations; weights and labels by attribute name; compound= with one label per compound"""
    test_partial.class_partials_add_up_to_intermediate_scattering(**on_gpu(dtype))
    test_partial.class_one_species_is_intermediate_scattering(**on_gpu(dtype))
    test_partial.class_total_and_the_normalisations(**on_gpu(dtype))
    test_partial.class_weights_and_attribute_names(**on_gpu(dtype))
    test_partial.class_compound_with_per_compound_labels(**on_gpu(dtype))
    saw(watched, "PartialScattering", dtype)


@pytest.mark.parametrize("dtype", STAGING)
def test_four_point_structure_factor(dtype, watched):
    """explicit wavevectors in d = 1, 2, 3 with the k = 0 row against DynamicSusceptibility on the same placement, a scalar
    cutoff and lags=None, float32 positions, q= / dq= of the box at frame 0 with and without unwrap=True (ta_unwrap, then the
    kernel on float64 slabs), compound= with and without the barycentric frame (ta_compound, then the kernel on its slab)"""
    test_overlap_density.class_against_reference(**on_gpu(dtype))
    test_overlap_density.class_scalar_cutoff_and_default_lags(**on_gpu(dtype))
    test_overlap_density.class_float32_staging_is_the_same(**on_gpu(dtype))
    test_overlap_density.class_box_shells_and_unwrap(**on_gpu(dtype))
    test_overlap_density.compounds_with_dyadic_weights(**on_gpu(dtype))
    saw(watched, "FourPointStructureFactor", dtype)


_cpu_class = {}


@pytest.mark.parametrize("dtype", STAGING)
@pytest.mark.parametrize("kind,boxed,stride", test_vanhove_distinct.CLASS_CASES)
def test_vanhove_distinct_against_reference(kind, boxed, stride, dtype, watched):
    """the same group, two disjoint groups and overlapping ones; the constant box, per-frame boxes at lag 0 and
    periodic=False; origin strides 1 and 3: counts, overflow and n_origins equal to the reference's, and gd, g, rdf and
    coordination EQUAL to the device="cpu" class's (computed once per case)"""
    r = test_vanhove_distinct.class_on_case(kind, boxed, stride, **on_gpu(dtype))
    if (kind, boxed, stride) not in _cpu_class:
        _cpu_class[kind, boxed, stride] = test_vanhove_distinct.class_on_case(kind, boxed, stride, device="cpu")
    cpu = _cpu_class[kind, boxed, stride]
    for key in test_vanhove_distinct.DERIVED_KEYS:
        a, b = getattr(r, key), getattr(cpu, key)
        assert (a is None and b is None) or np.array_equal(a, b), key
    assert boxed or r.g is None
    saw(watched, "VanHoveDistinct", dtype)


@pytest.mark.parametrize("dtype", STAGING)
def test_vanhove_distinct_class_tests(dtype, watched):
    test_vanhove_distinct.class_normalisation(**on_gpu(dtype))
    test_vanhove_distinct.class_uniform_gas_has_g_of_one(**on_gpu(dtype))
    test_vanhove_distinct.class_same_group_twice_and_no_box(**on_gpu(dtype))
    saw(watched, "VanHoveDistinct", dtype)


@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("kind", ["same", "disjoint", "explicit"])
def test_pair_lifetime_against_reference(kind, D, watched):
    """the nine (kind, D) cases of test_class_against_reference, each without a box, in the constant box and in per-frame
    boxes, search strides 1 and 3: with fft=False everything equal, with fft=True that test's bar"""
    test_pair_lifetime.class_against_reference(kind, D, device=0)
    assert "PairLifetime" in watched


@pytest.mark.parametrize("kind,D", [("same", 3), ("disjoint", 1)])
def test_pair_lifetime_float64_staging(kind, D, watched):
    test_pair_lifetime.class_against_reference(kind, D, **on_gpu(np.float64))
    assert not watched


@pytest.mark.parametrize("dtype", STAGING)
def test_pair_lifetime_without_any_bond_and_with_filters(dtype, watched):
    test_pair_lifetime.class_without_any_bond_gives_nan_with_a_warning(**on_gpu(dtype))
    for kind in ("same", "explicit"):
        test_bond_lifetime.pair_lifetime_with_filters(kind, **on_gpu(dtype))
    saw(watched, "PairLifetime", dtype)


@pytest.mark.parametrize("dtype", STAGING)
def test_hydrogen_bond_lifetime_on_water(dtype, watched):
    test_bond_lifetime.hydrogen_bond_lifetime_on_water(**on_gpu(dtype))
    saw(watched, "HydrogenBondLifetime", dtype)


@pytest.mark.parametrize("dtype", STAGING)
def test_orientational_correlation(dtype, watched):
    """the modes bond, bisector and normal with and without weights, fft True and False; the class test's weighted bisectors
    of wrapped molecules"""
    for mode in test_orientation.ref.MODES:
        for weighted in (False, True):
            test_orientation.class_on_walks(mode, weighted, **on_gpu(dtype))
    test_orientation.class_results_and_normalisation(**on_gpu(dtype))
    saw(watched, "OrientationalCorrelation", dtype)


@pytest.mark.parametrize("dtype", STAGING)
@pytest.mark.parametrize("mode", test_orientation.ref.MODES)
@pytest.mark.parametrize("dims,moving", [(test_orientation.ORTHO, False), (test_orientation.ORTHO, True), (test_orientation.TRIC, False),
                                         (test_orientation.TRIC, True)],
                         ids=["ortho-constant", "ortho-per-frame", "tric-constant", "tric-per-frame"])
def test_orientational_correlation_minimum_image(dims, moving, mode, dtype, watched):
    test_orientation.class_on_wrapped_molecules(mode, dims, moving, **on_gpu(dtype))
    saw(watched, "OrientationalCorrelation", dtype)


# ---- staging in pieces --------------------------------------------------------------------------------------------------------
def piece_cases():
    """{class name: a function that builds the class on 65 frames on device 0}"""
    from transport_analysis_amd import (CurrentCorrelation, DynamicSusceptibility, FourPointStructureFactor, HydrogenBondLifetime,
                                        IntermediateScattering, OrientationalCorrelation, PartialScattering, ShellMSD,
                                        ShellOrientation, ShellResidence, VanHoveDistinct, VanHoveSelf)
    from transport_analysis_amd._mini_mda import ArrayUniverse

    def scattering():
        x, k = test_scattering.ref.case(65, 13, 3, 3)[:2]
        return IntermediateScattering(ArrayUniverse(positions=x).atoms, k, device=0)

    def current():
        x, v, w, k = test_current_correlation.ref.case(65, 33, 3, 3)[:4]
        return CurrentCorrelation(ArrayUniverse(positions=x, velocities=v).atoms, k, weights=w, device=0)

    def vanhove_self():
        x, lags, _ = test_vanhove.ref.case(65, 13, 3)
        return VanHoveSelf(ArrayUniverse(positions=x).atoms, lags, r_max=8.0, n_bins=64, device=0)

    def vanhove_distinct():
        x, lags, a, b, dims, axes, _ = test_vanhove_distinct.ref.case(65, 33, 3, 1, "overlap", True)
        u = ArrayUniverse(positions=x, dimensions=dims)
        return VanHoveDistinct(u.atoms[a], u.atoms[b], lags, r_max=1.0, n_bins=64, device=0)

    def pair_lifetime():
        from transport_analysis_amd import PairLifetime

        case = test_pair_lifetime.ref.case(65, 40, 3, "same", True, 2)
        return PairLifetime(test_pair_lifetime.universe(case).atoms, r_cut=test_pair_lifetime.ref.R_CUT, search_stride=2, fft=False,
                            device=0)

    def hydrogen_bonds():
        u, x, ox, hy, dh = test_bond_lifetime.water(n_frames=65)
        return HydrogenBondLifetime(u.atoms[ox], u.atoms[hy], u.atoms[ox], donor_hydrogen_pairs=dh, d_a_cutoff=3.2,
                                    d_h_a_angle_cutoff=150.0, d_a_break=3.6, angle_break=130.0, intermittency=1, fft=False, device=0)

    def orientation():
        x, idx, w, _ = test_orientation.ref.case(65, 9, "bisector", weighted=True, n_mol=6)
        return OrientationalCorrelation(ArrayUniverse(positions=x).atoms, idx, mode="bisector", weights=w, minimum_image=False, device=0)

    def susceptibility():
        x, lags, _, _, _ = test_overlap.ref.case(65, 13, 3)
        return DynamicSusceptibility(ArrayUniverse(positions=x).atoms, lags, cutoff=test_overlap.ref.CUTOFFS, device=0)

    def partial_scattering():
        x, w, lab, k = test_partial.ref.case(65, 33, 3, 3, 3)[:4]
        return PartialScattering(ArrayUniverse(positions=x).atoms, k, species=lab, weights=w, device=0)

    def four_point():
        x, k, lags = test_overlap_density.ref.case(65, 13, 3)[:3]
        return FourPointStructureFactor(ArrayUniverse(positions=x).atoms, k, lags, cutoff=test_overlap_density.ref.CUTOFFS, device=0)

    def shell_cuts(cuts, dims):
        return dict(r_cut=cuts["r_cut"], r_break=cuts["r_break"], intermittency=1, periodic=dims is not None, device=0)

    def shell_residence():
        x, a, b, dims, axes, cuts = test_shell_residence.ref.case(65, 6, 30, 3, "disjoint", True, 1)[:6]
        u = test_shell_residence.universe(x, dims, axes)
        return ShellResidence(u.atoms[a], u.atoms[b], fft=False, **shell_cuts(cuts, dims))

    def shell_msd():
        x, a, b, dims, axes, cuts = test_shell_msd.mref.case(65, 6, 30, 3, "disjoint", True, 1, 20)[:6]
        u = test_shell_residence.universe(x, dims, axes)
        return ShellMSD(u.atoms[a], u.atoms[b], max_lag=20, **shell_cuts(cuts, dims))

    def shell_orientation():
        _, reference, group, vectors, cuts = test_shell_orientation.class_case("bond", 0, True, n_frames=65)[:5]
        return ShellOrientation(reference, group, vectors, mode="bond", anchor=0, max_lag=30, **shell_cuts(cuts, True))

    return {f.__name__: f for f in (scattering, current, vanhove_self, vanhove_distinct, pair_lifetime, hydrogen_bonds, orientation,
                                    susceptibility, partial_scattering, four_point, shell_residence, shell_msd,
                                    shell_orientation)}


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(a).dtype.kind == "f")


@pytest.mark.parametrize("name", sorted(piece_cases()))
def test_staging_in_pieces_gives_the_same_bits(name, monkeypatch, watched):
    """65 frames committed as 32 + 32 + 1 ("_COMMIT_BYTES" set to 32 frames of the class's slabs; the last piece, a single
    frame, is _conclude's) against the one commit of the default: every result bit-equal"""
    build = piece_cases()[name]
    whole = build().run().results
    obj = build()
    n_atoms = obj._n_atoms if obj._plan is not None else obj.n_particles
    frame_bytes = len(obj._stage_arrays) * n_atoms * obj.dim_fac * obj._pick_stage_dtype().itemsize
    monkeypatch.setattr(_base, "_COMMIT_BYTES", 32 * frame_bytes)
    pieces = []
    commit = _lib.Context.stage_commit

    def logged_commit(self, lo, hi):
        pieces.append((lo, hi))
        return commit(self, lo, hi)

    monkeypatch.setattr(_lib.Context, "stage_commit", logged_commit)
    parts = obj.run().results
    assert pieces == [(0, 32), (32, 64), (64, 65)], pieces
    assert set(parts.keys()) == set(whole.keys())
    for key in whole.keys():
        assert same_bits(whole[key], parts[key]), key
    assert len(watched) == 2


# ---- B: several members, several ranks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod", COLLECTIVE, ids=MODULE_IDS)
def test_two_members_on_one_device(mod, watched):
    """devices=[0, 0] with an odd atom count: the members' sums are added BEFORE the correlation (or the variance)"""
    A = ATOMS[mod]
    single = mod.placed_results(A, device=0)
    out = mod.placed_results(A, devices=[0, 0])
    assert out["device_ranges"].tolist() == [[0, A // 2], [A // 2, A]] and "device_ranges" not in single
    mod.check_placed(out, A, "devices=[0, 0]")
    mod.check_placed(single, A, "device=0")
    for key in mod.INTEGER_KEYS:
        assert out[key].dtype == np.int64 and np.array_equal(out[key], single[key]), key
    if mod is test_scattering:
        test_scattering.own_correlations_differ(A, [(0, A // 2), (A // 2, A)])
    assert len(watched) >= 3  # (the single run and both members)


#: the fewest atoms a module's case can be built with (partial_ref's three species need three)
FEWEST_ATOMS = {test_partial: 3}


@pytest.mark.parametrize("mod", COLLECTIVE, ids=MODULE_IDS)
def test_three_members_two_atoms_one_member_empty(mod, watched):
    """A atoms on A + 1 members (two on devices=[0, 0, 0]; PartialScattering three on four): the FIRST member holds none, the
    others one atom each with its own slice of the per-atom weights and labels"""
    A = FEWEST_ATOMS.get(mod, 2)
    out = mod.placed_results(A, devices=[0] * (A + 1))
    assert out["device_ranges"].tolist() == [[0, 0]] + [[i, i + 1] for i in range(A)]
    mod.check_placed(out, A, f"devices={[0] * (A + 1)}")
    single = mod.placed_results(A, device=0)
    for key in mod.INTEGER_KEYS:
        assert out[key].dtype == np.int64 and np.array_equal(out[key], single[key]), key
    if mod is test_vanhove:
        assert out["device_ranges"].tolist() == [[0, 0], [0, 1], [1, 2]]
        assert np.array_equal(out["counts"], single["counts"])


@pytest.mark.parametrize("more_ranks_than_atoms", [False, True], ids=["odd", "one-atom"])
@pytest.mark.parametrize("mod", COLLECTIVE, ids=MODULE_IDS)
def test_two_gloo_ranks_on_one_gpu(mod, more_ranks_than_atoms, tmp_path):
    """distributed=True, each rank a fresh child on the one GPU ($TA_AMD_DEVICE=0): the blocks' sums go through
    dist.allreduce_sum (on the host under gloo) before _correlate / _store; with one atom rank 0 has none (_no_moments)"""
    A = 1 if more_ranks_than_atoms else ATOMS[mod]
    placement.check_ranks(mod, A, 2, "gloo", tmp_path, dict(device=0))


@pytest.mark.parametrize("mod", COLLECTIVE, ids=MODULE_IDS)
def test_one_nccl_rank(mod, tmp_path):
    """distributed=True under nccl (RCCL) at world size 1 with $TA_AMD_FORCE_COLLECTIVE=1: allreduce_sum's device branch"""
    placement.check_ranks(mod, ATOMS[mod], 1, "nccl", tmp_path, dict(device=0))
