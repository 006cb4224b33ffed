"""k_chain_modes and the evaluations behind it at shapes that reach every branch, through the C-ABI (ta_chain_modes_staged,
ta_chain_modes), GPU only.  Every case runs with fft 1 and 0 on a float64 AND a float32 device slab holding the same values,
asserts k_chain_modes in the kernel timeline with exactly ceil(B / tile modes) launches per batch of B functionals, that no
widening kernel ran, that repeat runs agree bit for bit, that the staged slab's bits (padding included) are unchanged, and
compares with chain_ref at lag_sample: every functional's series within 1e-10 of its maximum.

  * 1, 2, 3 frames with 1 and 2 chains of two beads; chains of 2, 3, 4, 5 and 17 beads (the unrolled bead loop's empty body, its
    tail and no tail); an odd and an even chain count (the phantom column, the one-chain last unit); an odd frame count over
    two frame blocks (the float32 load whose second row is row T); eleven frame blocks with an outer-radix plan; more units
    than pm_unit_grid gives groups;
  * 1, M, M + 1 and 2 M + 1 functionals (M the tile's modes), some rows all zero (their series exactly 0), under
    "chain_modes_chunk" 1, 2 and 0: the same bits;
  * member tables with the first and the last atom of the slab, chains starting on odd and on even atoms, interleaved chains, a
    permuted chain list, an atom shared by two chains;
  * no box, a constant and a per-frame box, orthorhombic and triclinic, on chains the faces cut;
  * a smaller call straight after a larger one on one context without ta_trim; the host-facing call against the staged one
    bit for bit; the CPU backend and RouseModes(device=0) against device="cpu" within the bar."""
import numpy as np
import pytest

import chain_ref as ref
from test_orientation_shapes import slab_bits, stage, staged_bits
from transport_analysis_amd import RouseModes, _lib
from transport_analysis_amd._mini_mda import ArrayUniverse

pytestmark = pytest.mark.gpu

SLABS = [pytest.param(np.float64, id="slab64"), pytest.param(np.float32, id="slab32")]


def tile_modes():
    return _lib.chain_modes_tile()["modes"]


def launches(Q, chunk):
    """k_chain_modes launches of a call of Q functionals under "chain_modes_chunk" `chunk` (0: one batch -- the blocks of these
    shapes are far below the budget): ceil(B / tile modes) per batch of B"""
    M, B = tile_modes(), (Q if chunk == 0 else min(chunk, Q))
    return sum(-(-min(B, Q - q0) // M) for q0 in range(0, Q, B))


def run_staged(c, fft, members, coeff, dims=None, repeat=2):
    """ta_chain_modes_staged into a caller buffer, `repeat` times: the runs must agree bit for bit.  -> acf (Q, T)"""
    import torch

    T, Q = c.shape[0], coeff.shape[0]
    runs = []
    for _ in range(repeat):
        buf = torch.full((Q, T), np.nan, dtype=torch.float64, device="cuda:0")
        c.chain_modes_staged(fft, members, coeff, dims, buf.data_ptr())
        torch.cuda.synchronize()
        runs.append(buf.cpu().numpy())
    for r in runs[1:]:
        assert np.array_equal(runs[0], r), "repeat runs differ"
    return runs[0]


def check(c, dtype, x, members, coeff, want, dims=None, chunk=0, what=""):
    """-> {fft: acf}"""
    c.set_option("chain_modes_chunk", chunk)
    got = {}
    for fft in (1, 0):
        got[fft] = run_staged(c, fft, members, coeff, dims)
        assert c.kernel_launches("k_chain_modes") == launches(coeff.shape[0], chunk), (what, chunk)
        assert c.kernel_launches("k_widen_f32") == 0  # the slab is read in its own element type
        ref.assert_chain(got[fft], want, what=f"{what} fft={fft} chunk={chunk}")
    assert np.array_equal(slab_bits(c, dtype), staged_bits(c, x, dtype)), "the staged slab's bits changed"
    return got


def units_loop_chains():
    """more units (two chains each) than pm_unit_grid gives groups at one frame block: 16 groups per CU"""
    import torch

    return 2 * 16 * torch.cuda.get_device_properties(0).multi_processor_count + 907


# (id, T, chains or None: units_loop_chains(), beads)
SHAPE_CASES = [
    ("t1c1", 1, 1, 2), ("t2c1", 2, 1, 2), ("t3c1", 3, 1, 2), ("t1c2", 1, 2, 2), ("t2c2", 2, 2, 2), ("t3c2", 3, 2, 2),
    ("n3", 70, 5, 3), ("n4", 70, 5, 4), ("n5", 70, 5, 5), ("n17", 70, 5, 17),
    ("odd", 100, 1501, 4), ("even", 100, 1500, 4),
    ("two_frame_blocks", 1027, 3, 4),
    ("outer_radix", 10300, 3, 5),
    ("units_loop", 8, None, 2),
]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T,C,N", [pytest.param(*c[1:], id=f"{c[0]}-T{c[1]}-C{c[2]}-N{c[3]}") for c in SHAPE_CASES])
def test_chain_shapes(T, C, N, dtype):
    x, members, coeff, want = ref.case(T, C or units_loop_chains(), N, Q=2, layout="permuted")
    assert members.min() == 0 and members.max() == x.shape[1] - 1  # the first and the last atom of the slab
    c = stage(_lib.Context(0), x, dtype)
    try:
        got = check(c, dtype, x, members, coeff, want, what=f"T={T} N={N}")
        host = c.chain_modes(0, members, coeff)  # the host-facing call
        assert np.array_equal(host, got[0])
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("n_q", ["1", "M", "M+1", "2M+1"])
def test_chain_mode_counts_and_chunks(n_q, dtype):
    """some coefficient rows all zero; every chunk the same bits"""
    M = tile_modes()
    Q = {"1": 1, "M": M, "M+1": M + 1, "2M+1": 2 * M + 1}[n_q]
    zero = tuple(q for q in (1, M, 2 * M - 1) if q < Q)
    T, C, N = 300, 7, 6
    x, members, coeff, want = ref.case(T, C, N, Q=Q, layout="interleaved", zero_rows=zero)
    c = stage(_lib.Context(0), x, dtype)
    try:
        runs = [check(c, dtype, x, members, coeff, want, chunk=n, what=f"Q={Q}") for n in (1, 2, 0)]
        for r in runs[1:]:
            assert all(np.array_equal(runs[0][fft], r[fft]) for fft in (1, 0)), "chain_modes_chunk changes the bits"
        for q in zero:
            assert not runs[0][1][q].any() and not runs[0][0][q].any()
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("layout", ["blocked", "interleaved", "permuted", "shared"])
def test_chain_member_tables(layout, dtype):
    T, C, N = 90, 6, 5
    x, members, coeff, want = ref.case(T, C, N, Q=3, layout="blocked" if layout == "shared" else layout)
    if layout == "blocked":  # five beads: chains start on even and on odd atoms
        assert set(members[:, 0] % 2) == {0, 1}
    if layout == "interleaved":
        assert np.array_equal(members[2], 2 + C * np.arange(N))
    if layout == "shared":  # every atom of chain 0 once more, backwards, and one chain that crosses from chain 1 into chain 2
        members = np.concatenate([members, members[:1, ::-1], np.arange(N + 3, 2 * N + 3, dtype=np.int32)[None]])
        want = ref.reference(x, members, coeff)
    assert members.min() == 0 and members.max() == x.shape[1] - 1
    c = stage(_lib.Context(0), x, dtype)
    try:
        check(c, dtype, x, members, coeff, want, what=layout)
    finally:
        c.close()


BOXES = [pytest.param(None, False, id="no-box"),
         pytest.param(ref.ORTHO, False, id="ortho-constant"), pytest.param(ref.ORTHO, True, id="ortho-per-frame"),
         pytest.param(ref.TRIC, False, id="tric-constant"), pytest.param(ref.TRIC, True, id="tric-per-frame")]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("dims,moving", BOXES)
def test_chain_boxes(dims, moving, dtype):
    """chains the faces cut, 1027 frames (two frame blocks, odd) of 41 chains of 6 beads: with the box the call matches the
    reference of the staged values with the same image step, and the unwrapped trajectory's functions; without it, it does not"""
    T, C, N = 1027, 41, 6
    x, members, coeff, free = ref.case(T, C, N, Q=3, layout="permuted", seed=3)
    if dims is None:
        c = stage(_lib.Context(0), x, dtype)
        try:
            check(c, dtype, x, members, coeff, free, what="no box")
        finally:
            c.close()
        return
    box = ref.box_frames(dims, T, moving)
    wrapped = ref.cut_wrapped(x, members, box).astype(dtype).astype(np.float64)  # what the slab holds
    c = stage(_lib.Context(0), wrapped, dtype)
    try:
        got = check(c, dtype, wrapped, members, coeff, ref.reference(wrapped, members, coeff, box), dims=box)
        if dtype == np.float64 or (dims is ref.ORTHO and not moving):  # (float32 keeps the dyadic box's values exactly)
            ref.assert_chain(got[1], free, what="against the unwrapped chains")
        bare = run_staged(c, 1, members, coeff, repeat=1)
        assert np.abs(bare[:, 0] - got[1][:, 0]).max() > 0.1 * np.abs(got[1][:, 0]).max()
    finally:
        c.close()


def test_chain_stale_blocks():
    """A larger call (1027 frames, 40 chains, 5 functionals) then a smaller one (99 frames: rows 99 ... 103 of every pair, 7
    chains: a phantom column, 2 functionals) on ONE context without ta_trim: the second call's blocks and their tail rows lie
    where the first left values."""
    c = _lib.Context(0)
    try:
        for T, C, Q in ((1027, 40, 5), (99, 7, 2)):
            x, members, coeff, want = ref.case(T, C, 4, Q=Q)
            stage(c, x, np.float64)
            check(c, np.float64, x, members, coeff, want, what=f"T={T}")
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_chain_cpu_backend_and_class(dtype):
    """the CPU backend's results, and RouseModes on the GPU against device="cpu", agree within the bar"""
    T, C, N = 513, 9, 8
    x, members, coeff, _ = ref.case(T, C, N, Q=5, layout="interleaved")
    box = ref.box_frames(ref.ORTHO, T, True)
    wrapped = ref.cut_wrapped(x, members, box).astype(dtype).astype(np.float64)
    c = stage(_lib.Context(0), wrapped, dtype)
    cpu = _lib.Context("cpu")
    try:
        (view,) = cpu.stage_alloc(T, x.shape[1], 3, dtype=dtype)
        view[:] = wrapped
        cpu.stage_commit(0, T)
        for fft in (1, 0):
            g = run_staged(c, fft, members, coeff, box)
            h = cpu.chain_modes(fft, members, coeff, dimensions=box)
            for q in range(coeff.shape[0]):
                scale = float(np.max(np.abs(h[q])))
                err = float(np.max(np.abs(g[q] - h[q]))) / scale
                print(f"    GPU against CPU backend, fft={fft} functional {q}: {err:.3e} of {scale:.3e}")
                assert err <= 1e-10
    finally:
        c.close()
        cpu.close()
    u = ArrayUniverse(positions=wrapped, dimensions=box)
    a = RouseModes(u.atoms, members, stage_dtype=dtype, device=0).run().results
    b = RouseModes(u.atoms, members, stage_dtype=dtype, device="cpu").run().results
    assert a.rg2 is not None and abs(a.rg2 - b.rg2) <= 1e-10 * b.rg2 and abs(a.r2 - b.r2) <= 1e-10 * b.r2
    for key in ("acf", "end_to_end_acf"):
        ga, gb = np.atleast_2d(getattr(a, key)), np.atleast_2d(getattr(b, key))
        assert np.all(np.max(np.abs(ga - gb), axis=1) <= 1e-10 * np.max(np.abs(gb), axis=1)), key


def test_chain_checks_before_anything_is_written():
    """a bad member, found on the host: TA_E_INVALID, the device output untouched, no launch"""
    import torch

    x, members, coeff, _ = ref.case(8, 4, 3)
    c = stage(_lib.Context(0), x, np.float64)
    try:
        out = torch.full((coeff.shape[0], 8), 7.5, dtype=torch.float64, device="cuda:0")
        bad = np.array(members)
        bad[2, 1] = x.shape[1]
        with pytest.raises(_lib.TAError, match="is outside 0 ... n_atoms - 1") as e:
            c.chain_modes_staged(1, bad, coeff, d_acf=out.data_ptr())
        assert e.value.code == -1
        torch.cuda.synchronize()
        assert bool((out == 7.5).all())
    finally:
        c.close()
