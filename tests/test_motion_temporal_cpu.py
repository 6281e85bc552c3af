"""motion -b 1x1xD over a clip (temporal_rt.hip), the parts that need no device: the plan helper motion_temporal_plans, the f64 oracle's
own pieces (tests/motion_temporal_ref.py) against the oracle library, the kernel's phases (dspfun_amd/csrc/temporal_core.h) compiled with
g++ and run thread by thread against that oracle, what the emulation library still runs and what it answers -3, and the product library's
refusals ahead of any launch."""
import ctypes as C
import math

import numpy as np
import pytest

import motion_grid_ref as gr
import motion_ref as mr
import motion_temporal_ref as tr
import oracle_lib as ol
from dspfun_amd.engine import Plan, DspfftError, REDFT10, REDFT01, motion_temporal_plans
from temporal_shim import core, run_core, expected_tile  # noqa: F401  (core is a fixture)

FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned address for calls that are refused before anything reads it
IDS = [tr.pair_id(p) for p in tr.PAIRS]


# ---- (a) the plan helper ----
@pytest.mark.parametrize("D,S", tr.PAIRS, ids=IDS)
def test_motion_temporal_plans_crops_and_carries_motions_constants(D, S):
    from emul_lib import emul
    fwd, inv, info = motion_temporal_plans((3 * D + 1, tr.H, tr.W), D, S, lib=emul())
    assert info["in_shape"] == (3 * D, tr.H, tr.W) and info["out_shape"] == (3 * S, tr.H, tr.W) and info["nblocks"] == (3, tr.H, tr.W)
    assert info["active"] == (min(D, S), 1, 1)
    sf, nm = mr.consts((D, 1, 1), (S, 1, 1))
    assert info["scalefactor"] == sf == S / D and info["normalization"] == pytest.approx(nm, rel=1e-15) == pytest.approx(1 / math.sqrt(8 * S), rel=1e-15)
    assert info["out_mul"] == pytest.approx(sf * nm * nm, rel=1e-15)
    # a rank-1 strided pass each: one axis, a line per pixel and block (TINY up to 32 points, the column pass above)
    for pl, n in ((fwd, D), (inv, S)):
        lines = [l for l in pl.describe().splitlines() if l.startswith("axis")]
        assert len(lines) == 1 and lines[0].startswith("axis 0:") and f"N={n} " in lines[0], pl.describe()
        assert ("lines=900" in lines[0]) if n <= 32 else ("inner=300" in lines[0] and "COL" in lines[0]), lines[0]


def test_motion_temporal_plans_scales_are_motions():
    """the plans alone (the emulation library's own passes, no filter) give the oracle's coefficients and pixels: 2 sqrt 2 x 2 with 1 / sqrt 2
    at index 0 forward, 2 / (2 sqrt 2) with sqrt 2 at index 0 back, pinned against motion_ref.block_roundtrip on (D, 1, 1) blocks"""
    from emul_lib import emul
    D = 8
    ref = tr.case(D, D)
    fwd, inv, info = motion_temporal_plans(ref["vol"].shape, D, lib=emul())
    x = np.ascontiguousarray(ref["vol"][:3 * D], dtype=np.float32)
    c = x.copy()
    fwd.execute(c.ctypes.data)
    cols = np.ascontiguousarray(c.reshape(3, D, tr.P).transpose(0, 2, 1)).reshape(-1, D)
    assert np.abs(cols - ref["act"]).max() < 1e-2                         # coefficients of 8-bit samples reach 510 D
    inv.execute(c.ctypes.data)
    assert np.abs(c.astype(np.float64) * info["out_mul"] - ref["pel"]).max() < tr.TOL
    for col in (0, 7, 299, 300, 899):
        pix = np.ascontiguousarray(np.asarray(tr.columns(ref["vol"], D)[0][col]).reshape(D, 1, 1))
        o, coeffs, _ = mr.block_roundtrip(pix, (D, 1, 1), (D, 1, 1), (D, 1, 1))
        assert np.allclose(coeffs.ravel(), ref["act"][col], rtol=0, atol=1e-9)
        b, r = divmod(col, tr.P)
        assert np.array_equal(o.ravel(), ref["out8"].reshape(3, D, tr.P)[b, :, r])


def test_motion_temporal_plans_refuses_what_no_clip_is():
    from emul_lib import emul
    for shape, D, S in (((17, 5, 5), 8, 8),            # 25 samples per frame: no multiple of 4
                        ((7, 6, 50), 8, 8),            # no whole block
                        ((17, 6, 50), 1, 8)):          # a length of 1 is no transform
        with pytest.raises(ValueError):
            motion_temporal_plans(shape, D, S, lib=emul())


# ---- (b) the oracle's own pieces ----
@pytest.mark.parametrize("D,S", [(8, 16), (64, 32), (25, 25)], ids=["8-16", "64-32", "25-25"])
def test_oracle_chain_is_block_roundtrip_on_d11_blocks(D, S):
    """plain and quantised: every stage of motion_temporal_ref.oracle against motion_ref.block_roundtrip on (D, 1, 1) -> (D', 1, 1)"""
    for kind in ("plain", "quant"):
        ref = tr.case(D, S, kind)
        quant = ref["filter"]["quantizer"] / (8 * math.sqrt(S)) if kind == "quant" else 0.0      # motion.c:570 backwards
        cols, _ = tr.columns(ref["vol"], D)
        M = max(D, S)
        for col in (0, 1, 298, 299, 300, 601, 899):
            pix = np.zeros((M, 1, 1), dtype=np.uint8)
            pix[:D, 0, 0] = cols[col]
            o, coeffs, _ = mr.block_roundtrip(pix, (D, 1, 1), (S, 1, 1), (M, 1, 1), quant=quant)
            # (the quantiser here is the float the C ABI takes, block_roundtrip's a double: steps of q differ by 2^-24 of themselves)
            assert np.allclose(coeffs.ravel()[:min(D, S)], ref["act"][col], rtol=1e-6 if quant else 0, atol=1e-9)
            b, r = divmod(col, tr.P)
            assert np.array_equal(o.ravel()[:S], ref["out8"].reshape(3, S, tr.P)[b, :, r])


@pytest.mark.parametrize("kind", tr.KINDS[1:])
def test_filter_restatement_is_the_oracles_on_float32(kind):
    O = ol.lib()
    I3, I2 = C.c_int * 3, C.c_int * 2
    O.oracle_motion_filter_f32.restype = C.c_ulonglong
    O.oracle_motion_filter_f32.argtypes = [C.c_void_p] * 5 + [C.c_float] * 4 + [C.c_int, C.c_double, C.c_float]
    for D, S in ((25, 25), (24, 30), (64, 32)):
        f = tr.filter_dict(kind, D, S)
        ref = tr.case(D, S, kind)
        A = min(D, S)
        coeffs = tr.forward(ref["vol"], D, S)[0].astype(np.float32)
        got, coded = tr.filt(coeffs, f, np.float32)
        n = 0
        for col in range(0, len(coeffs), 37):
            line = coeffs[col].copy()
            n += O.oracle_motion_filter_f32(line.ctypes.data, I3(A, 1, 1), I2(1, 1), I3(*f["band_begin"]), I3(*f["band_end"]), f["damp"], f["boost"],
                                            f["threshold_lo"], f["threshold_hi"], f["preserve_dc"], f["grey_add"], f["quantizer"])
            assert np.array_equal(line, got[col]), (D, S, col)
        if kind == "quant":
            assert n == int(np.count_nonzero(got[::37])) > 0


# ---- (f) what the 8-bit rule leaves open ----
@pytest.mark.parametrize("D,S", tr.PAIRS, ids=IDS)
def test_few_oracle_pixels_lie_within_the_tolerance_of_a_half(D, S):
    for kind in tr.KINDS:
        ref = tr.case(D, S, kind)
        share = float(tr.near_half(ref["pel"]).mean())
        assert share <= 0.01, (kind, share)
        if ref["edge"] is not None:
            assert ref["edge"] > (gr.EDGE if kind == "quant" else tr.EDGE_REL)
        if kind == "quant":
            assert ref["coded"] > 0


# ---- (c) the header's phases on the CPU: a test-only shim that builds the arguments the engine derives (the planner's radix order, the
# column pass's tables) and walks every thread through every phase ----
# (the shim's source, its `core` fixture, run_core and expected_tile: tests/temporal_shim.py, shared with tests/test_lengths_cpu.py)


@pytest.mark.parametrize("D,S", tr.PAIRS, ids=IDS)
def test_phases_against_the_oracle(core, D, S):
    """index arithmetic, the short last tile, the held post items, zero padding and truncation; the tile starts as NaNs.  8-bit: the GPU
    test's rule.  Float: within TOL of the f64 pixels, with a band filter."""
    ref = tr.case(D, S)
    got, _, tile = run_core(core, ref, D, S)
    assert tile == expected_tile(D, S)
    tr.check_bytes(got, ref)
    for k in (16, 64):                  # other tile widths, the same bytes
        assert np.array_equal(run_core(core, ref, D, S, kforce=k)[0], got)
    band = tr.case(D, S, "band")
    f, _, _ = run_core(core, band, D, S, u8=False, flt=band["filter"])
    sf, nm = mr.consts((D, 1, 1), (S, 1, 1))
    err = float(np.abs(f.astype(np.float64) * sf * nm * nm - band["pel"]).max())
    assert err <= tr.TOL, err


@pytest.mark.parametrize("D,S", [(8, 8), (25, 25), (24, 30), (64, 32)], ids=["8-8", "25-25", "24-30", "64-32"])
def test_phases_with_each_filter(core, D, S):
    for kind in tr.KINDS[1:]:
        ref = tr.case(D, S, kind)
        got, coded, _ = run_core(core, ref, D, S, flt=ref["filter"])
        tr.check_bytes(got, ref)
        if kind == "quant":
            assert coded == ref["coded"] > 0


def test_phases_at_the_longest_length(core):
    """1024 frames in the narrowest tile, 512 threads: every held register in use"""
    D = 1024
    vol = ol.synth_u8(77, D * 8).reshape(D, 2, 4)
    out8, pel, _, _ = tr.oracle(vol, D, D)
    nd, sf_nm = 1, mr.consts((D, 1, 1), (D, 1, 1))
    out = np.zeros_like(vol)
    rc = core.run(None, np.ascontiguousarray(vol).ctypes.data, None, out.ctypes.data, nd, 8, D, D, 0, None, sf_nm[0] * sf_nm[1] ** 2, None)
    assert divmod(rc, 1000) == (16, 512)
    tr.check_bytes(out, dict(pel=pel, out8=out8))
    assert core.run(None, FAKE, None, FAKE, 1, 8, 1040, 1040, 0, None, 1.0, None) == -2      # beyond the budget


# ---- (d) the emulation library: what ran at the parent still runs, what the new kernel takes is answered -3 ----
def test_emulation_library_runs_the_parents_calls_and_refuses_the_new_ones():
    from emul_lib import emul
    L = emul()
    D, S = 8, 16
    ref = tr.case(D, D)
    fwd, inv, info = motion_temporal_plans(ref["vol"].shape, D, lib=L)
    x = np.ascontiguousarray(ref["vol"][:3 * D], dtype=np.float32)
    # no filter, equal extents, float: the plans' own passes, bit for bit what execute forward then inverse gives
    a, b = x.copy(), x.copy()
    fwd.roundtrip(inv, a.ctypes.data)
    fwd.execute(b.ctypes.data); inv.execute(b.ctypes.data)
    assert np.array_equal(a, b) and np.abs(a.astype(np.float64) * info["out_mul"] - ref["pel"]).max() < tr.TOL
    # ... and so does a pure quantiser, which needs no positions
    q = tr.case(D, D, "quant")
    a = np.ascontiguousarray(q["vol"][:3 * D], dtype=np.float32)
    coded = np.zeros(1, dtype=np.uint64)
    fwd.roundtrip(inv, a.ctypes.data, filter=q["filter"], d_coded=coded.ctypes.data)
    assert int(coded[0]) == q["coded"] and np.abs(a.astype(np.float64) * info["out_mul"] - q["pel"]).max() < tr.TOL
    # the 8-bit call, a filter that needs positions, the dithered call, a rescaled pair: -3, and nothing is written
    u8 = np.ascontiguousarray(ref["vol"])
    o8 = np.full(3 * S * tr.P, 9, dtype=np.uint8)
    work = np.full(3 * S * tr.P, 7.0, dtype=np.float32)
    rc = L.dspfft_execute_roundtrip_u8(fwd._h, inv._h, u8.ctypes.data, o8.ctypes.data, work.ctypes.data, info["out_mul"], None, None, None)
    assert rc == -3 and b"not built into this library" in L.dspfft_last_error()
    with pytest.raises(DspfftError, match="not built into this library"):
        fwd.roundtrip_u8_dither(inv, u8.ctypes.data, o8.ctypes.data, work.ctypes.data, info["scalefactor"], info["normalization"])
    a = x.copy()
    with pytest.raises(DspfftError, match="not built into this library"):
        fwd.roundtrip(inv, a.ctypes.data, filter=tr.filter_dict("band", D, D))
    assert np.array_equal(a, x)
    fwd2, inv2, info2 = motion_temporal_plans(ref["vol"].shape, D, S, lib=L)
    rc = L.dspfft_execute_roundtrip_u8(fwd2._h, inv2._h, u8.ctypes.data, o8.ctypes.data, None, info2["out_mul"], None, None, None)
    assert rc == -3 and b"not built into this library" in L.dspfft_last_error()
    of = np.full(3 * S * tr.P, 7.0, dtype=np.float32)
    with pytest.raises(DspfftError, match="not built into this library"):
        fwd2.roundtrip(inv2, x.ctypes.data, of.ctypes.data)
    assert np.all(o8 == 9) and np.all(work == 7.0) and np.all(of == 7.0)
    # a length beyond the narrowest tile is refused for its length, whichever library is asked
    fl, il, infol = motion_temporal_plans((1040, 2, 4), 1040, lib=L)
    rc = L.dspfft_execute_roundtrip_u8(fl._h, il._h, u8.ctypes.data, o8.ctypes.data, None, infol["out_mul"], None, None, None)
    assert rc == -2 and b"too long for the narrowest tile" in L.dspfft_last_error()


# ---- (e) the product library's refusals, all ahead of any launch ----
def test_refusals_of_the_product_library_come_before_any_launch():
    """plans of up to 32 points need no device tables, so the product library plans them here (the length beyond the narrowest tile, whose
    plan needs them: the emulation library above, and tests/test_motion_temporal_gpu.py)"""
    from dspfun_amd import _lib
    L = _lib.load()
    err = L.dspfft_last_error
    D, S = 8, 16
    shape = (3 * D + 1, tr.H, tr.W)
    fwd, inv, info = motion_temporal_plans(shape, D, lib=L)
    fwd2, inv2, info2 = motion_temporal_plans(shape, D, S, lib=L)
    call, call8 = L.dspfft_execute_roundtrip, L.dspfft_execute_roundtrip_u8
    band = Plan._filter_params(tr.filter_dict("band", D, D))
    # a coefficient limit below the block's length, in every entry that takes one
    cl = _lib.CoeffLimit()
    cl.keep, cl.outside_mul, cl.d_work, cl.work_bytes = 3, 1.0, None, 0
    assert L.dspfft_execute_roundtrip_topn(fwd._h, inv._h, FAKE, FAKE, C.byref(band), 3, None, 0, None, None) == -2 and b"coefficient limit" in err()
    assert L.dspfft_execute_roundtrip_u8_topn(fwd._h, inv._h, FAKE, FAKE, None, 1.0, None, 3, None, 0, None, None) == -2 and b"coefficient limit" in err()
    assert L.dspfft_execute_roundtrip_limit(fwd2._h, inv2._h, FAKE, FAKE, None, C.byref(cl), None, None) == -2 and b"coefficient limit" in err()
    assert L.dspfft_execute_roundtrip_u8_limit(fwd._h, inv._h, FAKE, FAKE, None, 1.0, None, C.byref(cl), None, None) == -2 and b"coefficient limit" in err()
    assert L.dspfft_execute_roundtrip_u8_dither_limit(fwd._h, inv._h, FAKE, FAKE, None, 1.0, 1.0, None, C.byref(cl), None, None) == -2 and b"coefficient limit" in err()
    # a prime factor above 13
    f17, i17, _ = motion_temporal_plans((17, tr.H, tr.W), 17, lib=L)
    assert call8(f17._h, i17._h, FAKE, FAKE, None, 1.0, None, None, None) == -2 and b"prime factor above 13" in err()
    f8, i29, _ = motion_temporal_plans((8, tr.H, tr.W), 8, 29, lib=L)
    assert call(f8._h, i29._h, FAKE, FAKE, None, None, None) == -2 and b"prime factor above 13" in err()
    # 6 samples per frame: the plans can be made, the fused kernel moves four samples at a time
    how = lambda n: [(3, n * 6, n * 6), (6, 1, 1)]
    f6 = Plan.guru([(D, 6, 6)], how(D), [REDFT10], lib=L)
    i6 = Plan.guru([(D, 6, 6)], how(D), [REDFT01], lib=L)
    assert call8(f6._h, i6._h, FAKE, FAKE, None, 1.0, None, None, None) == -2 and b"multiple of 4" in err()
    # float buffers off 16 bytes, 8-bit buffers off 4
    for a, b in ((4096 + 4, 4096), (4096, 4096 + 8)):
        assert call(fwd2._h, inv2._h, C.c_void_p(a), C.c_void_p(b), None, None, None) == -2 and b"aligned" in err()
        assert call(fwd._h, inv._h, C.c_void_p(a), C.c_void_p(b), C.byref(band), None, None) == -2 and b"aligned" in err()
    assert call8(fwd._h, inv._h, C.c_void_p(4096 + 2), FAKE, None, 1.0, None, None, None) == -2 and b"aligned" in err()
    assert call8(fwd._h, inv._h, FAKE, C.c_void_p(4096 + 1), None, 1.0, None, None, None) == -2 and b"aligned" in err()
    # (more than 2^31 - 1 workgroups cannot be asked for: a clip of that many tiles has more lines or tiles than a plan can be made for)
    # blocks that the two plans count differently are no temporal pair: the call goes where it went before
    _, inv4, _ = motion_temporal_plans((4 * S, tr.H, tr.W), S, lib=L)
    assert call8(fwd._h, inv4._h, FAKE, FAKE, FAKE, 1.0, None, None, None) < 0 and b"blocks along time" not in err()
