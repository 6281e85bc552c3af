"""motion -b with -s AND --coeff-limit on packed 8-bit pixels (block_rescale_packed_limit.hip, dspfft_execute_roundtrip_u8_packed_rescale_limit), the
parts that need no device: the wide tile's phases (dspfun_amd/csrc/block_rs_packed_wide_core.h) compiled with g++ and walked thread by thread
in the kernel's order, a serial selection stating topn_core.h's rule in place of its ballot rounds (tests/packed_rescale_wide.py), against the
f64 restatement of the reference on every component (tests/motion_grid_topn_ref.py: blocks on which the reference's ranking differs from
"scale everything, then rank"); the group rule's LDS budget; and the refusals of both new entries through the emulation library, which come
before the missing kernel is noticed, beside the unchanged refusals of the two old entries on a rescaled pair."""
import ctypes as C

import numpy as np
import pytest

import motion_grid_ref as gr
import motion_grid_topn_ref as tr
import packed_rescale_wide as pw
from dspfun_amd import _lib
from dspfun_amd.engine import Plan, DspfftError, motion_grid_plans

FAKE = C.c_void_p(4096)               # non-null, 16-byte aligned addresses for calls that are refused before anything reads them,
FAR = C.c_void_p(1 << 40)             # ... far enough apart that no clip planned here reaches from one to the other
NO_FIT = ((16, 16, 16), (8, 8, 8))    # the 16 x 16 x 16 embedding: four whole component tiles are 64 KB, no room for the tables


def plain_packed(comps):
    p = _lib.MotionPacked()
    p.components = comps
    return p


def coeff_limit(keep=16, outside_mul=1.0):
    c = _lib.CoeffLimit()
    c.keep = keep; c.outside_mul = outside_mul
    return c


@pytest.mark.parametrize("block,scaled", tr.PAIRS, ids=[tr.pair_id(p) for p in tr.PAIRS])
def test_phases_with_a_serial_selection_against_the_oracle_on_every_component(block, scaled):
    """rgb24, component c from seed 500 + 37 c on.  test_motion_grid_topn_gpu.py's bar: at most 1 LSB, fewer than 2 % of the bytes differing; the
    volumes' blocks tell the reference's rule from a selection over scaled values in every component (asserted).  Other groupings -- one
    pixel block, a short last group, an odd group -- give the same bytes."""
    clip, refs = pw.topn_clip(block, scaled)
    keep = refs[0]["keep"]
    for ref in refs:
        assert ref["gap"] > tr.GAP and ref["dc_kept"]
        assert ref["differs"] is (True if any(b > s for b, s in zip(block, scaled)) else None)
    G = pw.rule_G(block, scaled, 3, tr.NBLOCKS[2], True, False)
    assert 1 <= G <= tr.NBLOCKS[2]
    got, coded, _ = pw.run_wide(clip, block, scaled, G, keep=keep)
    assert coded == 0
    for c, ref in enumerate(refs):
        diff = np.abs(got[..., c].astype(int) - ref["out8"].astype(int))
        print(f"{tr.pair_id((block, scaled))} component {c}: seed {ref['seed']}, keep {keep}, gap {ref['gap']:.2e}, max {diff.max()} LSB, {(diff > 0).mean():.5f} of the bytes differ")
        assert diff.max() <= 1 and (diff > 0).mean() < 0.02, (c, diff.max(), (diff > 0).mean())
    for g in (1, 2, 3):
        if g != G and pw.fits(block, scaled, 3, g, True, False):
            assert np.array_equal(pw.run_wide(clip, block, scaled, g, keep=keep)[0], got), g
    assert np.array_equal(pw.run_wide(clip, block, scaled, min(5, pw.rule_G(block, scaled, 3, pw.NB, True, False)), keep=keep, block_major=True)[0], got)


def test_every_component_is_selected_and_filtered_with_its_own_values():
    """a band filter with preserve_dc = dc, a quantiser, a threshold and another damp / boost / grey_add per component, behind the selection:
    component c's bytes and count are those of a clip that holds component c three times with c's values at every byte position"""
    block, scaled = tr.PAIRS[0]
    clip, refs = pw.topn_clip(block, scaled)
    filt = pw.band_filter(block, scaled, 3, 1)
    per = []
    for c in range(3):
        q, lo, hi, damp, boost, grey, band = filt
        one = (q, lo, hi, [damp[c]] * 3, [boost[c]] * 3, [grey[c]] * 3, band)
        o, n, _ = pw.run_wide(np.repeat(clip[..., c:c + 1], 3, axis=-1), block, scaled, 4, keep=refs[0]["keep"], filt=one)
        assert np.array_equal(o[..., 0], o[..., 1]) and np.array_equal(o[..., 0], o[..., 2]) and n % 3 == 0
        per.append((o[..., 0], n // 3))
    got, coded, _ = pw.run_wide(clip, block, scaled, 4, keep=refs[0]["keep"], filt=filt)
    for c in range(3):
        assert np.array_equal(got[..., c], per[c][0]), c
    assert coded == sum(n for _, n in per) and len({n for _, n in per}) > 1 and min(n for _, n in per) > 0


def test_the_group_rule_fits_tile_tables_and_dither_rows_into_64_KB():
    refused = []
    for block, scaled in tr.PAIRS + [gr.PAIRS[2]]:
        for comps in (2, 3, 4):
            for limit, dither in ((True, False), (False, True), (True, True)):
                for nxb in (1, 7, 28, 240):
                    G = pw.rule_G(block, scaled, comps, nxb, limit, dither)
                    assert 0 <= G <= nxb
                    if not G:
                        refused.append((block, scaled, comps, limit))
    assert set(refused) == {(NO_FIT[0], NO_FIT[1], 4, True)}, refused


# ---- refusals, through the emulation library: each is -1 or -2 with its reason before the missing kernel (-3) is noticed, nothing is written ----
@pytest.fixture(scope="module")
def emu():
    from emul_lib import emul
    return emul()


def entries(L, info, cl=None):
    """the two entries as call(fwd, inv, a, b, pk) -> rc; the dithered one with cl (None: no limit)"""
    lim = coeff_limit(16, info["limit_outside_mul"])

    def limit(f, i, a=FAKE, b=FAR, pk=None, cl=lim):
        return L.dspfft_execute_roundtrip_u8_packed_rescale_limit(f._h if f else None, i._h if i else None, a, b, info["out_mul"], None,
                                                                  C.byref(pk) if pk is not None else None, C.byref(cl) if cl is not None else None, None, None)

    def dither(f, i, a=FAKE, b=FAR, pk=None, cl=cl, sf=info["scalefactor"], nm=info["normalization"]):
        return L.dspfft_execute_roundtrip_u8_packed_rescale_dither(f._h if f else None, i._h if i else None, a, b, sf, nm, None,
                                                                   C.byref(pk) if pk is not None else None, C.byref(cl) if cl is not None else None, None, None)
    return limit, dither


def test_refusals_of_both_entries_come_before_the_missing_kernel(emu):
    L = emu
    err = L.dspfft_last_error
    block, scaled = (8, 8, 8), (4, 4, 4)
    in_shape, out_shape = gr.shapes(block, scaled)
    fwd, inv, info = motion_grid_plans(in_shape, block, scaled, lib=L)
    p3, p4 = plain_packed(3), plain_packed(4)
    limit, dither = entries(L, info)
    names = {limit: b"over a rescaled grid of blocks with a coefficient limit", dither: b"dithered roundtrip on packed 8-bit pixels over a rescaled grid of blocks"}
    # keep == 0 and a NULL limit on _limit; keep == 0 on _dither (NULL is its call without a limit)
    assert limit(fwd, inv, pk=p3, cl=None) == -1 and b"null dspfft_coeff_limit" in err() and names[limit] in err()
    assert limit(fwd, inv, pk=p3, cl=coeff_limit(0)) == -1 and b"keep must be at least 1" in err()
    assert dither(fwd, inv, pk=p3, cl=coeff_limit(0)) == -1 and b"keep must be at least 1" in err()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert limit(fwd, inv, pk=p3, cl=coeff_limit(16, bad)) == -1 and b"outside_mul" in err()
        assert dither(fwd, inv, pk=p3, cl=coeff_limit(16, bad)) == -1 and b"outside_mul" in err()
    # bad scalefactor / normalization
    for s, n in ((0.0, 1.0), (-1.0, 1.0), (float("inf"), 1.0), (float("nan"), 1.0), (1.0, 0.0), (1.0, float("nan"))):
        assert dither(fwd, inv, pk=p3, sf=s, nm=n) == -1 and b"scalefactor and normalization must be finite and > 0" in err() and names[dither] in err()
    f64 = Plan.many_r2r([8, 8, 8], [5] * 3, howmany=4, idist=512, odist=512, lib=L, dtype="f64")
    fe, ie, _ = motion_grid_plans(in_shape, block, block, lib=L)
    f1 = Plan.many_r2r([8, 8, 8], [5] * 3, lib=L)
    i1 = Plan.many_r2r([4, 4, 4], [4] * 3, lib=L, first_axis_first=True)
    b16, s16 = NO_FIT
    f16, i16, info16 = motion_grid_plans(gr.shapes(b16, s16)[0], b16, s16, lib=L)
    in_bytes, out_bytes = int(np.prod(in_shape)) * 3, int(np.prod(out_shape)) * 3
    for call in (limit, dither):
        name = names[call]
        assert call(None, inv, pk=p3) == -1 and b"null plan or buffer" in err() and name in err()
        assert call(fwd, inv, a=None, pk=p3) == -1 and b"null plan or buffer" in err()
        assert call(fwd, inv, b=None, pk=p3) == -1 and b"null plan or buffer" in err()
        assert call(fwd, inv) == -1 and b"null dspfft_motion_packed" in err() and name in err()
        assert call(f64, inv, pk=p3) == -1 and b"f32 plans" in err() and name in err()
        for comps in (1, 5):
            assert call(fwd, inv, pk=plain_packed(comps)) == -2 and b"components must be 2, 3 or 4" in err() and name in err()
        assert call(fe, ie, pk=p3) == -2 and b"equal extents" in err() and name in err()
        assert call(f1, i1, pk=p3) == -2 and b"one block" in err() and b"not implemented" in err()
        for a, b in ((4096, 4096), (4096, 4096 + in_bytes - 4), (4096 + out_bytes - 4, 4096)):
            assert call(fwd, inv, a=C.c_void_p(a), b=C.c_void_p(b), pk=p3) == -2 and b"overlap" in err() and name in err()
        for a, b in ((4096 + 2, 1 << 40), (4096, (1 << 40) + 1)):
            assert call(fwd, inv, a=C.c_void_p(a), b=C.c_void_p(b), pk=p3) == -2 and b"4-byte aligned" in err()
    # rgba on the 16 x 16 x 16 embedding with a limit: the four whole component tiles are 64 KB
    lim16, dth16 = entries(L, info16, cl=coeff_limit(40, info16["limit_outside_mul"]))
    assert lim16(f16, i16, pk=p4) == -2 and b"64 KB of LDS" in err() and b"16x16x16" in err() and names[limit] in err()
    assert dth16(f16, i16, pk=p4) == -2 and b"64 KB of LDS" in err() and names[dither] in err()
    # ... three components fit, and a call that passes every check ends at the missing kernel
    assert lim16(f16, i16, pk=p3) == -3 and b"not built into this library" in err() and b"block_rescale_packed_limit.hip" in err()
    assert limit(fwd, inv, pk=p3) == -3 and b"block_rescale_packed_limit.hip" in err()
    assert dither(fwd, inv, pk=p3) == -3 and b"block_rescale_packed_dither.hip" in err()
    # keep >= the embedding's count is the plain call
    assert limit(fwd, inv, pk=p3, cl=coeff_limit(512)) == -3 and b"block_rescale_packed.hip" in err()


def test_refused_calls_write_nothing_and_the_python_layer_raises(emu):
    L = emu
    block, scaled = (8, 8, 8), (4, 4, 4)
    in_shape, out_shape = gr.shapes(block, scaled)
    fwd, inv, info = motion_grid_plans(in_shape, block, scaled, lib=L)
    u8 = np.full(int(np.prod(in_shape)) * 3, 7, dtype=np.uint8)
    o8 = np.full(int(np.prod(out_shape)) * 3, 9, dtype=np.uint8)
    p = plain_packed(3)
    with pytest.raises(DspfftError, match="not built into this library"):
        fwd.roundtrip_u8_packed_rescale(inv, u8.ctypes.data, o8.ctypes.data, info["out_mul"], p, coeff_limit=16, outside_mul=info["limit_outside_mul"])
    with pytest.raises(DspfftError, match="not built into this library"):
        fwd.roundtrip_u8_packed_rescale_dither(inv, u8.ctypes.data, o8.ctypes.data, info["scalefactor"], info["normalization"], p)
    with pytest.raises(DspfftError, match="not built into this library"):
        fwd.roundtrip_u8_packed_rescale_dither(inv, u8.ctypes.data, o8.ctypes.data, info["scalefactor"], info["normalization"], p, coeff_limit=16)
    with pytest.raises(DspfftError, match="components must be 2, 3 or 4"):
        fwd.roundtrip_u8_packed_rescale(inv, u8.ctypes.data, o8.ctypes.data, info["out_mul"], plain_packed(5), coeff_limit=16)
    with pytest.raises(DspfftError, match="overlap"):
        fwd.roundtrip_u8_packed_rescale_dither(inv, u8.ctypes.data, u8.ctypes.data, info["scalefactor"], info["normalization"], p)
    assert np.all(o8 == 9) and np.all(u8 == 7)


def test_the_old_entries_still_refuse_a_rescaled_pair_in_their_words(emu):
    L = emu
    block, scaled = (8, 8, 8), (4, 4, 4)
    fwd, inv, info = motion_grid_plans(gr.shapes(block, scaled)[0], block, scaled, lib=L)
    p3 = plain_packed(3)
    assert L.dspfft_execute_roundtrip_u8_packed(fwd._h, inv._h, FAKE, FAR, info["out_mul"], None, C.byref(p3), None, None, None) == -2
    assert b"(a rescaled block grid, motion -s) are not implemented on packed pixels" in L.dspfft_last_error()
    assert L.dspfft_execute_roundtrip_u8_packed_dither(fwd._h, inv._h, FAKE, FAR, info["scalefactor"], info["normalization"], None, C.byref(p3), None, None, None) == -2
    assert b"-d on a packed rescaled grid is not implemented" in L.dspfft_last_error()
