"""Which kernels a request takes: the dispatch of api.hip as a table.

One parametrised test over rows of (entry, n_frames, output form, options) -> the exact list of kernel timeline names
("timeline" option, ta_kernel_timeline) of the call, on both sides of every threshold the dispatch tests: k_short up to 64
frames (FFT lag sums: up to "short_lags_max" 48), k_mid from 65 / 97 to 128 / 512, the matrix-core forms from 352 (Helfand
float64), 448 (Helfand float32) and 513 frames (windowed VACF), the 512-point FFT kernels up to 512 frames, the on-chip
transforms up to 10240, an outer radix up to 163840 and the direct form beyond.  Every row runs with 9 atoms (27 columns:
an unpaired last column) and with 70 (two 64-atom tiles).  The expected lists were written from the dispatch code and
checked on the device against the library as it was before the dispatch was rewritten; the values themselves are the
parity tests' business (test_gpu_parity.py, test_exact_parity.py).  The rows list the launches as they are queued;
ta_kernel_timeline reports a name once, at its first appearance, with its launches' times added up, so the assertion
compares against the row's names in that form."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEFAULTS = {"direct_mfma": 1, "direct_f32": 0, "helfand_fft": 0, "mid_all": 0, "mid_max": 512, "short_max": 64,
            "short_lags_max": 48, "stage_device_f32": 0}
SCALE = 0.37  # Helfand prefactor: any positive number

# ---- the pieces the lists are made of
TAIL = ["k_bp_transpose", "k_sum_partials"]  # atom-major by-particle scratch -> the caller's array, then the tile sums
SHORT = ["k_short", "k_sum_partials"]
MID = ["k_mid", "k_sum_partials"]
VEC = ["memset", "k_direct", "k_sum_partials"]
VEC_BP = VEC + ["k_bp_transpose"]
BAND_VACF = ["k_band_bp_vacf"]
BAND_HELF = ["k_helfand_product", "k_band_bp_helf"]
BAND32 = ["k_helfand_product32", "k_band32_tp"]
W1 = ["k_w1_accum", "k_wf_sum+k_wf_fold+k_wf_lags"]  # up to 512 frames, lag sums
W1_BP = ["k_w1_bp"] + TAIL
WF = ["k_wsplit_accum", "k_sum_partials", "k_winverse"]  # beyond 512 frames, lag sums
WF_BP = ["k_wsplit_accum", "k_winverse"] + TAIL  # (one block of atoms at these sizes)
WIDEN = ["k_widen_f32"]
RELAYOUT = ["k_relayout"]
MOMENT = ["k_cond_moment", "k_sum_partials"]
SPECIES = ["k_species_moment", "k_sum_partials"]


def s1_2s2(prepare, fft_names, by_particle):
    """S1 - 2 S2 around an FFT evaluation of the prepared slab (Helfand "helfand_fft" 1, Einstein MSD fft)."""
    if by_particle:
        return [prepare] + fft_names + ["k_helfand_combine", "k_row_sums"]
    return [prepare, "k_sum_partials"] + fft_names + ["k_helfand_combine"]


ROWS = []


def row(entry, T, form, expect, via="host", atoms=(9, 70), dtype=np.float64, **opts):
    """form: by-particle array or not; for the conductivity (self term, collective term); for Onsager ("S", n_species,
    cross term)."""
    for A in atoms:
        tag = "-".join([entry, via, f"T{T}", f"A{A}",
                        ("bp" if form else "lags") if not isinstance(form, tuple)
                        else "S%d_cross%d" % form[1:] if form[0] == "S" else "self%d_coll%d" % form] +
                       [f"{k}{v}" for k, v in sorted(opts.items())] + (["f32"] if dtype == np.float32 else []))
        ROWS.append(pytest.param(entry, via, T, A, form, dtype, opts, list(expect), id=tag))


# ---- windowed VACF
for bp in (False, True):
    tail = TAIL if bp else []
    row("vacf_direct", 64, bp, SHORT)
    row("vacf_direct", 65, bp, VEC_BP if bp else VEC)
    row("vacf_direct", 96, bp, VEC_BP if bp else VEC)
    row("vacf_direct", 97, bp, MID)
    row("vacf_direct", 512, bp, MID)
    row("vacf_direct", 513, bp, BAND_VACF + tail)
    row("vacf_direct", 700, bp, VEC_BP if bp else VEC, direct_mfma=0)
    row("vacf_direct", 700, bp, BAND_VACF + tail, direct_mfma=1)
    row("vacf_direct", 700, bp, BAND_VACF + tail, direct_mfma=3)
    row("vacf_direct", 64, bp, BAND_VACF + tail, direct_mfma=3)  # forced: no k_short either
    row("vacf_direct", 64, bp, VEC_BP if bp else VEC, direct_mfma=0)
    row("vacf_direct", 100, bp, MID, mid_all=1, direct_mfma=1)
    row("vacf_direct", 80, bp, MID, mid_all=1)
    row("vacf_direct", 100, bp, VEC_BP if bp else VEC, mid_all=1, direct_mfma=0)
    row("vacf_direct", 100, bp, VEC_BP if bp else VEC, mid_max=0)
    row("vacf_direct", 100, bp, MID, short_max=0)
    row("vacf_direct", 64, bp, VEC_BP if bp else VEC, short_max=0)

# ---- Helfand
for bp in (False, True):
    tail = TAIL if bp else []
    vec = VEC_BP if bp else VEC
    row("helfand", 64, bp, SHORT)
    row("helfand", 97, bp, MID)
    row("helfand", 128, bp, MID)
    row("helfand", 129, bp, vec)
    row("helfand", 351, bp, vec)
    row("helfand", 352, bp, BAND_HELF + tail)
    row("helfand", 64, bp, vec, direct_f32=1)  # the float32 option: neither k_short nor k_mid
    row("helfand", 447, bp, vec, direct_f32=1)
    row("helfand", 448, bp, BAND32 + tail, direct_f32=1)
    row("helfand", 700, bp, s1_2s2("k_helfand_product", WF_BP if bp else WF, bp), helfand_fft=1)
    row("helfand", 300, bp, s1_2s2("k_helfand_product", W1_BP if bp else W1, bp), helfand_fft=1)
    # float32 device slabs: widened (both slabs) unless the float32 correlators read them as they are
    row("helfand", 700, bp, WIDEN + WIDEN + BAND_HELF + tail, dtype=np.float32, stage_device_f32=1, direct_f32=0)
    row("helfand", 700, bp, BAND32 + tail, dtype=np.float32, stage_device_f32=1, direct_f32=1)

# ---- FFT VACF
row("vacf_fft", 48, False, SHORT)  # lag sums alone: "short_lags_max"
row("vacf_fft", 49, False, W1)
row("vacf_fft", 64, False, W1)
row("vacf_fft", 65, False, W1)
row("vacf_fft", 64, True, SHORT)
row("vacf_fft", 65, True, W1_BP)
for bp in (False, True):
    row("vacf_fft", 512, bp, W1_BP if bp else W1)
    row("vacf_fft", 513, bp, WF_BP if bp else WF)
    row("vacf_fft", 10240, bp, WF_BP if bp else WF)
    row("vacf_fft", 10241, bp, WF_BP if bp else WF)  # (an outer radix: the same kernels' names)
    row("vacf_fft", 163841, bp, BAND_VACF + (TAIL if bp else []), atoms=(4,))  # no plan: the direct form
    # float32 device slabs: read as they are by the plans without an outer radix from 513 frames
    row("vacf_fft", 700, bp, WF_BP if bp else WF, dtype=np.float32, stage_device_f32=1)
    row("vacf_fft", 300, bp, WIDEN + (W1_BP if bp else W1), dtype=np.float32, stage_device_f32=1)

# ---- Einstein MSD
for bp in (False, True):
    row("msd0", 64, bp, SHORT)
    row("msd0", 65, bp, MID)
    row("msd0", 160, bp, MID)
    row("msd0", 512, bp, MID)
    row("msd0", 513, bp, VEC_BP if bp else VEC)
    row("msd1", 64, bp, SHORT)
    row("msd1", 65, bp, s1_2s2("k_msd_prepare", W1_BP if bp else W1, bp))
    row("msd1", 160, bp, s1_2s2("k_msd_prepare", W1_BP if bp else W1, bp))
    row("msd1", 512, bp, s1_2s2("k_msd_prepare", W1_BP if bp else W1, bp))
    row("msd1", 513, bp, s1_2s2("k_msd_prepare", WF_BP if bp else WF, bp))
    # the forced forms leave the Einstein MSD's own k_short rule; fft_impl's holds (lag sums alone: up to 48 frames)
    row("msd1", 64, bp, s1_2s2("k_msd_prepare", SHORT if bp else W1, bp), direct_mfma=0)
    row("msd1", 48, bp, s1_2s2("k_msd_prepare", SHORT, bp), direct_mfma=0)
    row("msd1", 64, bp, s1_2s2("k_msd_prepare", W1_BP if bp else W1, bp), short_max=0)

# ---- conductivity: the moment, then the self term (an MSD lag sum) and the collective term (the moment's MSD)
for fft, T, msd in ((0, 64, SHORT), (0, 700, VEC), (1, 64, SHORT), (1, 700, s1_2s2("k_msd_prepare", WF, False))):
    row(f"cond{fft}", T, (1, 1), MOMENT + msd + RELAYOUT + msd)
    row(f"cond{fft}", T, (0, 1), MOMENT + RELAYOUT + msd)
    row(f"cond{fft}", T, (0, 0), MOMENT)

# ---- Onsager: every species' moment in one pass, then the cross MSD = the by-particle MSDs of the S^2 pseudo-particles
# M_i, M_i +- M_j between the combination kernel and the polarisation kernel (n_species 1, 3, 8: one per class of
# k_species_moment)
ONS_MSD = {(0, 64): SHORT, (0, 700): VEC_BP, (1, 64): SHORT, (1, 700): s1_2s2("k_msd_prepare", WF_BP, True)}
for via, pre in (("host", []), ("staged", []), ("dev", RELAYOUT)):
    for (fft, T), msd in ONS_MSD.items():
        for S in (1, 3, 8):
            row(f"ons{fft}", T, ("S", S, 1), pre + SPECIES + ["k_onsager_combos"] + msd + ["k_onsager_finish"], via=via)
            row(f"ons{fft}", T, ("S", S, 0), pre + SPECIES, via=via)

# ---- the staged entries and the *_dev entries (frame-major device input: relayout first)
for via, pre in (("staged", []), ("dev", RELAYOUT)):
    row("vacf_fft", 700, False, pre + WF, via=via)
    row("vacf_fft", 700, True, pre + WF_BP, via=via)
    row("vacf_direct", 100, True, pre + MID, via=via)
    row("vacf_direct", 513, False, pre + BAND_VACF, via=via)
    row("helfand", 400, False, pre + pre + BAND_HELF, via=via)
    row("helfand", 400, True, pre + pre + BAND_HELF + TAIL, via=via)
    row("msd0", 600, True, pre + VEC_BP, via=via)
    row("msd1", 160, True, pre + s1_2s2("k_msd_prepare", W1_BP, True), via=via)
    row("cond0", 64, (1, 1), pre + MOMENT + SHORT + RELAYOUT + SHORT, via=via)
    row("cond1", 700, (0, 1), pre + MOMENT + RELAYOUT + s1_2s2("k_msd_prepare", WF, False), via=via)


@pytest.fixture(scope="module")
def ctx():
    from transport_analysis_amd import _lib

    assert _lib.device_count() >= 1, "no GPU visible: the HIP path cannot run"
    c = _lib.Context(0)
    yield c
    c.close()


def inputs(entry, T, A, dtype):
    """(velocities or positions, positions, masses, charges) with a fixed seed per shape."""
    from oracle import numpy_oracle as orc

    v, x, m, _ = orc.synthetic_helfand(T, A, 3, seed=4100 + T + A)
    v, x = v.astype(dtype), x.astype(dtype)
    q = np.where(np.arange(A) % 2 == 0, 1.0, -0.8)
    first = v if entry in ("vacf_fft", "vacf_direct", "helfand") else x
    return first, x, m, q


def run_host(ctx, entry, form, first, x, m, q):
    if entry == "vacf_fft":
        return ctx.vacf_fft(by_particle=form)
    if entry == "vacf_direct":
        return ctx.vacf_direct(by_particle=form)
    if entry == "helfand":
        return ctx.helfand_msd(m, SCALE, by_particle=form)
    if entry in ("msd0", "msd1"):
        return ctx.msd(entry == "msd1", by_particle=form)
    if entry in ("ons0", "ons1"):
        return ctx.onsager(entry == "ons1", np.arange(len(q)) % form[1], form[1], weights=q, cross=bool(form[2]))
    return ctx.conductivity(entry == "cond1", q, self_term=bool(form[0]), collective=bool(form[1]))


def run_device(ctx, entry, via, form, first, x, m, q):
    """The staged / *_dev entry with device outputs; returns them as host arrays."""
    import torch

    T, A, D = first.shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    ptr = lambda t: t.data_ptr() if t is not None else 0
    d_first, d_x, d_m, d_q = dev(first), dev(x), dev(m), dev(q)
    where = (d_first.data_ptr(), T, A, D, A * D) if via == "dev" else ()
    if entry in ("ons0", "ons1"):
        S = form[1]
        d_lab = torch.from_numpy((np.arange(A) % S).astype(np.int32)).cuda()
        out = [zeros(S, T, D), zeros(T, S, S) if form[2] else None]
        fn = ctx.onsager_dev if via == "dev" else ctx.onsager_staged
        fn(*where, entry == "ons1", S, d_lab.data_ptr(), ptr(out[0]), d_q.data_ptr(), ptr(out[1]))
    elif entry in ("cond0", "cond1"):
        out = [zeros(T, D), zeros(T) if form[1] else None, zeros(T) if form[0] else None]
        fn = ctx.conductivity_dev if via == "dev" else ctx.conductivity_staged
        fn(*where, entry == "cond1", d_q.data_ptr(), ptr(out[0]), ptr(out[1]), ptr(out[2]))
    else:
        out = [zeros(T), zeros(T, A) if form else None]
        res = (ptr(out[0]), ptr(out[1]), A)
        if entry == "helfand" and via == "dev":
            ctx.helfand_msd_dev(d_first.data_ptr(), d_x.data_ptr(), d_m.data_ptr(), T, A, D, A * D, SCALE, *res)
        elif entry == "helfand":
            ctx.helfand_msd_staged(d_m.data_ptr(), SCALE, *res)
        elif entry in ("msd0", "msd1"):
            (ctx.msd_dev if via == "dev" else ctx.msd_staged)(*where, entry == "msd1", *res)
        else:
            getattr(ctx, f"{entry}_{via}")(*where, *res)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def run_row(ctx, entry, via, T, A, form, dtype, opts):
    """Stage the row's inputs, make its call under its options; (timeline names, the call's outputs)."""
    first, x, m, q = inputs(entry, T, A, dtype)
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.set_option("timeline", 1)
        if via != "dev":
            slabs = ctx.stage_alloc(T, A, 3, n_slabs=2 if entry == "helfand" else 1, dtype=dtype)
            slabs[0][...] = first
            if entry == "helfand":
                slabs[1][...] = x
            ctx.stage_commit(0, T)
        if via == "host":
            out = run_host(ctx, entry, form, first, x, m, q)
        else:
            out = run_device(ctx, entry, via, form, first, x, m, q)
        names = [n for n, _ in ctx.kernel_timeline()]
    finally:
        ctx.set_option("timeline", 0)
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)
    return names, out


@pytest.mark.parametrize("entry,via,T,A,form,dtype,opts,expect", ROWS)
def test_dispatch_table(ctx, entry, via, T, A, form, dtype, opts, expect):
    names, out = run_row(ctx, entry, via, T, A, form, dtype, opts)
    assert names == list(dict.fromkeys(expect))  # (a name once, in order of first appearance)
    assert all(np.isfinite(o).all() for o in out if o is not None)
