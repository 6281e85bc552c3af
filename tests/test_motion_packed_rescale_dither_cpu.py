"""motion -b with -s AND -d on packed 8-bit pixels (block_rescale_packed_dither.hip, dspfft_execute_roundtrip_u8_packed_rescale_dither), the parts
that need no device: the wide tile's phases (dspfun_amd/csrc/block_rs_packed_wide_core.h) compiled with g++ and walked thread by thread in the
kernel's order (tests/packed_rescale_wide.py).  The oracle is the reference's Floyd-Steinberg walk restated in numpy (tests/dither_ref.py)
applied to the phases' OWN floats -- what the inverse's x pass leaves in the tile, the planar dithered call's work buffer --, plane by plane
of every component: EQUAL bytes, with and without a coefficient limit; with a transfer characteristic at the output the oracle is the planar
store's walk (dither_core.h: dither_plane_serial) over the same floats.  The floats themselves are pinned to the undithered phases: rounding
them plainly gives the undithered call's bytes.  (The entries' refusals: test_motion_packed_rescale_limit_cpu.py.)"""
import ctypes as C

import numpy as np
import pytest

import dither_ref as dr
import motion_grid_ref as gr
import motion_grid_topn_ref as tr
import motion_ref as mr
import packed_rescale_wide as pw

# down, up, 2-D up and mixed (8x8x8 -> 4x16x8: the tile is wider than min(block, scaled) on no axis but taller)
PAIRS = [tr.PAIRS[0], tr.PAIRS[1], tr.PAIRS[5], gr.PAIRS[2]]
IDS = [gr.pair_id(p) for p in PAIRS]


def clip_of(block, comps):
    import oracle_lib as ol
    shape = gr.shapes(block, block, tr.NBLOCKS)[0]
    return ol.synth_u8(0xD17 + comps + 16 * block[0] + block[2], int(np.prod(shape)) * comps).reshape(shape + (comps,))


def dithered_blocks(floats, scaled, sf, nm, trc=0):
    """[D'][H'][W'][C] floats -> bytes: each component's volume cut into blocks of `scaled`, every z plane of every block dithered on its own"""
    out = np.empty(floats.shape, dtype=np.uint8)
    for c in range(floats.shape[-1]):
        blocks = gr.to_blocks(np.ascontiguousarray(floats[..., c]), scaled)        # [blocks][d][h][w]
        if trc:
            got = np.empty(blocks.shape, dtype=np.uint8)
            flat_in, flat_out = blocks.reshape(-1, scaled[1], scaled[2]), got.reshape(-1, scaled[1], scaled[2])
            for i in range(flat_in.shape[0]):
                plane, o = np.ascontiguousarray(flat_in[i]), np.empty(scaled[1:], dtype=np.uint8)
                pw.core().walk_serial_trc(o.ctypes.data, plane.ctypes.data, scaled[1], scaled[2], sf, nm, trc)
                flat_out[i] = o
        else:
            got = dr.dither_planes(blocks, sf, nm)
        out[..., c] = gr.from_blocks(got, scaled, tr.NBLOCKS)
    return out


@pytest.mark.parametrize("comps", [3, 4])
@pytest.mark.parametrize("block,scaled", PAIRS, ids=IDS)
def test_dithered_bytes_are_the_references_walk_over_the_phases_own_floats(block, scaled, comps):
    """no limit: the tile is SX columns wide.  The rule's group, one pixel block and a short last group; both layouts."""
    clip = clip_of(block, comps)
    sf, nm = mr.consts(block, scaled)
    filt = pw.band_filter(block, scaled, comps, 2)
    G = pw.rule_G(block, scaled, comps, tr.NBLOCKS[2], False, True)
    assert 1 <= G <= tr.NBLOCKS[2]
    got, coded, floats = pw.run_wide(clip, block, scaled, G, dither=True, filt=filt)
    assert not np.isnan(floats).any() and coded > 0
    want = dithered_blocks(floats, scaled, sf, nm)
    assert np.array_equal(got, want), int((got != want).sum())
    plain = np.clip(np.round(floats.astype(np.float64) * sf * nm * nm), 0, 255)
    assert (got != plain).any()          # the diffusion acts
    for g in (1, 2):
        o, n, f = pw.run_wide(clip, block, scaled, g, dither=True, filt=filt)
        assert np.array_equal(o, got) and n == coded and np.array_equal(f, floats), g
    o, n, f = pw.run_wide(clip, block, scaled, min(5, pw.rule_G(block, scaled, comps, pw.NB, False, True)), dither=True, filt=filt, block_major=True)
    assert np.array_equal(o, got) and n == coded and np.array_equal(f, floats)


@pytest.mark.parametrize("block,scaled", PAIRS, ids=IDS)
def test_the_floats_are_the_undithered_sequences(block, scaled):
    """what the inverse's x pass writes back to the tile rounds plainly to the bytes of the same sequence ending in the plain packed store,
    without and with a coefficient limit (the limit changes them)"""
    clip = clip_of(block, 3)
    sf, nm = mr.consts(block, scaled)
    seen = []
    for keep in (0, tr.KEEP.get((block, scaled), 16)):
        plain, _, _ = pw.run_wide(clip, block, scaled, 2, keep=keep)
        _, _, floats = pw.run_wide(clip, block, scaled, 2, keep=keep, dither=True)
        pel = floats.astype(np.float64) * sf * nm * nm
        off_tie = np.abs(pel - np.floor(pel) - 0.5) > 1e-3           # (the store's float product may part from the double one at a half)
        assert np.array_equal(np.clip(np.round(pel), 0, 255)[off_tie], plain[off_tie]) and off_tie.mean() > 0.99
        seen.append(floats)
    assert not np.array_equal(seen[0], seen[1])


@pytest.mark.parametrize("block,scaled", [PAIRS[0], PAIRS[1], PAIRS[2]], ids=IDS[:3])
def test_dithered_bytes_with_a_coefficient_limit(block, scaled):
    """with a limit the tile is MX columns wide and the planes are its first SX columns: the same oracle over the phases' own floats, on
    the clips whose blocks make the reference's ranking visible"""
    clip, refs = pw.topn_clip(block, scaled)
    sf, nm = mr.consts(block, scaled)
    G = pw.rule_G(block, scaled, 3, tr.NBLOCKS[2], True, True)
    got, _, floats = pw.run_wide(clip, block, scaled, G, keep=refs[0]["keep"], dither=True)
    assert not np.isnan(floats).any()
    want = dithered_blocks(floats, scaled, sf, nm)
    assert np.array_equal(got, want), int((got != want).sum())
    # the floats are the limit call's: within the oracle's bar of the f64 pixels
    for c, ref in enumerate(refs):
        err = np.abs(floats[..., c].astype(np.float64) * sf * nm * nm - ref["pel"]).max()
        assert err < 1e-2, (c, err)
    o, _, f = pw.run_wide(clip, block, scaled, 1, keep=refs[0]["keep"], dither=True)
    assert np.array_equal(o, got) and np.array_equal(f, floats)


@pytest.mark.parametrize("limit", [False, True], ids=["plain", "limit"])
@pytest.mark.parametrize("block,scaled", [PAIRS[0], PAIRS[2]], ids=[IDS[0], IDS[2]])
def test_a_transfer_characteristic_at_the_output(block, scaled, limit):
    """the byte is the encoded one, the error stays the reference's: the planar store's walk with the characteristic over the same floats"""
    clip = clip_of(block, 3)
    sf, nm = mr.consts(block, scaled)
    keep = tr.KEEP[(block, scaled)] if limit else 0
    got, _, floats = pw.run_wide(clip, block, scaled, 3, keep=keep, dither=True, trc=pw.SRGB)
    want = dithered_blocks(floats, scaled, sf, nm, trc=pw.SRGB)
    assert np.array_equal(got, want), int((got != want).sum())
    lin, _, lf = pw.run_wide(clip, block, scaled, 3, keep=keep, dither=True)
    assert np.array_equal(lf, floats) and not np.array_equal(lin, got)
