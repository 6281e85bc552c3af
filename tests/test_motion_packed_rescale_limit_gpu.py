"""motion -b with -s AND --coeff-limit on packed 8-bit pixels on the device (block_rescale_packed_limit.hip,
dspfft_execute_roundtrip_u8_packed_rescale_limit).  The kernel runs the planar limit kernel's phases over the component blocks of a wide tile and
topn_core.h's selection per component block, so the first oracle needs no tolerance: the bytes equal Plan.roundtrip_u8_limit on the same planar
grid pair on each de-interleaved component with that component's damp / boost / grey_add and info["limit_outside_mul"], and d_coeffs_coded is the
sum of the planar counts.  The second is the f64 restatement of the reference (tests/motion_grid_topn_ref.py) on the CPU test's seeds, at
test_motion_grid_topn_gpu.py's bar.  Clips are tr.NBLOCKS blocks; every packed output lies between two marker pages."""
import functools

import numpy as np
import pytest

import motion_grid_ref as gr
import motion_grid_topn_ref as tr
import oracle_lib as ol
import packed_rescale_wide as pw
from test_motion_packed_rescale_gpu import settings

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from dspfun_amd import _lib
    _lib.load()
    return torch


def grid_plans(block, scaled):
    from dspfun_amd.engine import motion_grid_plans
    return motion_grid_plans(gr.shapes(block, scaled, tr.NBLOCKS)[0], block, scaled)


@functools.lru_cache(maxsize=None)
def clip_of(block, comps):
    shape = gr.shapes(block, block, tr.NBLOCKS)[0]
    c = ol.synth_u8(0x11A + comps + 16 * block[0] + block[2], int(np.prod(shape)) * comps).reshape(shape + (comps,))
    c.setflags(write=False)
    return c


def run_packed(torch, fwd, inv, src, out_shape, info, packed, filt=None, keep=0):
    """src: the interleaved input clip; out_shape: the output clip's, components included.  Returns (bytes, coded)."""
    n = int(np.prod(out_shape))
    whole, out = pw.guarded(n)
    d_in = torch.from_numpy(np.array(src)).to("cuda:0").reshape(-1)
    coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    fwd.roundtrip_u8_packed_rescale(inv, d_in.data_ptr(), out.data_ptr(), info["out_mul"], packed, filter=filt, d_coded=coded.data_ptr(),
                                    stream=torch.cuda.current_stream().cuda_stream, coeff_limit=keep, outside_mul=info["limit_outside_mul"])
    torch.cuda.synchronize()
    assert pw.markers_intact(whole, n), "the call wrote outside the clip"
    return out.cpu().numpy().reshape(out_shape), int(coded.item())


def run_planes(torch, fwd, inv, src, out_shape, info, planes, keep):
    """Plan.roundtrip_u8_limit of the same pair on every de-interleaved component.  Returns (interleaved bytes, [coded per component])."""
    want = np.empty(out_shape, dtype=np.uint8)
    counts = []
    stream = torch.cuda.current_stream().cuda_stream
    for c, filt in enumerate(planes):
        d_in = torch.from_numpy(np.array(src[..., c])).to("cuda:0")
        d_out = torch.zeros(out_shape[:-1], dtype=torch.uint8, device="cuda:0")
        coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        fwd.roundtrip_u8_limit(inv, d_in.data_ptr(), d_out.data_ptr(), None, info["out_mul"], coeff_limit=keep, outside_mul=info["limit_outside_mul"], filter=filt,
                               d_coded=coded.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        want[..., c] = d_out.cpu().numpy()
        counts.append(int(coded.item()))
    return want, counts


def both(torch, block, scaled, comps, name, pdc=2, fmt=None, keep=None):
    fwd, inv, info = grid_plans(block, scaled)
    src = clip_of(block, comps)
    filt, packed, planes = settings(block, scaled, comps, info, name, fmt=fmt, pdc=pdc)
    out_shape = tuple(info["out_shape"]) + (comps,)
    keep = keep or tr.KEEP[(block, scaled)]
    got, coded = run_packed(torch, fwd, inv, src, out_shape, info, packed, filt, keep)
    want, counts = run_planes(torch, fwd, inv, src, out_shape, info, planes, keep)
    return got, coded, want, counts


# every pair at three components; down, 2-D up and the two-blocks-per-wave pair at four; the 16 x 16 x 16 embedding at two and three
CASES = [(p, 3) for p in tr.PAIRS] + [(tr.PAIRS[i], 4) for i in (0, 5, 6)] + [(tr.PAIRS[3], 2)]


@pytest.mark.parametrize("name", ["none", "quant", "dc", "grey"])
@pytest.mark.parametrize("pair,comps", CASES, ids=[tr.pair_id(p) + f"-c{c}" for p, c in CASES])
def test_packed_limit_call_equals_the_planar_limit_call_on_every_component(gpu, pair, comps, name):
    """no filter; --quant alone; a band with per-component damp and boost, --threshold and preserve_dc = dc / grey through motion_packed"""
    block, scaled = pair
    got, coded, want, counts = both(gpu, block, scaled, comps, "full" if name in ("dc", "grey") else name, pdc=1 if name == "dc" else 2)
    assert np.array_equal(got, want), int((got != want).sum())
    assert coded == sum(counts) and (name == "none") == (coded == 0), (coded, counts)
    if name in ("dc", "grey"):
        assert len(set(counts)) > 1          # the components were filtered differently


def test_the_limit_acts_and_a_limit_of_the_whole_embedding_is_the_plain_call(gpu):
    block, scaled = tr.PAIRS[0]
    fwd, inv, info = grid_plans(block, scaled)
    src = clip_of(block, 3)
    filt, packed, _ = settings(block, scaled, 3, info, "full")
    out_shape = tuple(info["out_shape"]) + (3,)
    plain, n0 = run_packed(gpu, fwd, inv, src, out_shape, info, packed, filt)
    for keep in (512, 513, 1 << 20):
        got, n = run_packed(gpu, fwd, inv, src, out_shape, info, packed, filt, keep=keep)
        assert np.array_equal(got, plain) and n == n0 > 0, keep
    lim, n = run_packed(gpu, fwd, inv, src, out_shape, info, packed, filt, keep=16)
    assert not np.array_equal(lim, plain) and 0 < n < n0


@pytest.mark.parametrize("forced", ["1", "3", "5"])
def test_a_lane_group_without_a_block(gpu, monkeypatch, forced):
    """1x4x8 -> 1x4x4: an embedding of 32 elements, two component blocks per wave.  At three components an odd group leaves an odd number
    of tile blocks (seven pixel blocks in threes: 9, 9 and 3; in fives: 15 and 6 ... ), so the last lane group of a wave has none"""
    block, scaled = tr.PAIRS[6]
    rule, coded, want, counts = both(gpu, block, scaled, 3, "full")
    assert np.array_equal(rule, want)
    monkeypatch.setenv("DSPFFT_PACKED_G", forced)
    got, coded2, _, _ = both(gpu, block, scaled, 3, "full")
    assert np.array_equal(got, rule) and coded2 == coded == sum(counts) > 0


@pytest.mark.parametrize("pair", [tr.PAIRS[0], tr.PAIRS[4]], ids=[tr.pair_id(tr.PAIRS[0]), tr.pair_id(tr.PAIRS[4])])
def test_a_short_last_group(gpu, monkeypatch, pair):
    """seven blocks along x in groups of 2, 2, 2, 1: the bytes of the rule's group"""
    block, scaled = pair
    rule, coded, want, _ = both(gpu, block, scaled, 3, "full")
    monkeypatch.setenv("DSPFFT_PACKED_G", "2")
    got, coded2, _, _ = both(gpu, block, scaled, 3, "full")
    assert np.array_equal(got, rule) and np.array_equal(rule, want) and coded2 == coded > 0


def test_bgr24_takes_the_components_values_to_bytes_2_1_0(gpu):
    block, scaled = tr.PAIRS[0]
    got, coded, want, counts = both(gpu, block, scaled, 3, "full", fmt="bgr24")
    assert np.array_equal(got, want) and coded == sum(counts) > 0
    rgb, _, _, _ = both(gpu, block, scaled, 3, "full", fmt="rgb24")
    assert not np.array_equal(rgb, got)


def test_block_major_stacks_give_the_volume_layouts_bytes(gpu):
    from dspfun_amd import Plan, REDFT10, REDFT01
    block, scaled = tr.PAIRS[0]
    vol, cv, _, _ = both(gpu, block, scaled, 3, "full")
    fv, iv, info = grid_plans(block, scaled)
    # the pair over block-major stacks, with the volume pair's scales
    import math
    r2 = math.sqrt(2.0)
    nb = pw.NB
    fwd = Plan.many_r2r(list(block), [REDFT10] * 3, howmany=nb, idist=int(np.prod(block)), odist=int(np.prod(block))).set_scale(2 * r2)
    inv = Plan.many_r2r(list(scaled), [REDFT01] * 3, howmany=nb, idist=int(np.prod(scaled)), odist=int(np.prod(scaled))).set_scale(1 / (2 * r2))
    for a in range(3):
        fwd.set_axis_scale0(a, 1.0, 1.0 / r2)
        inv.set_axis_scale0(a, r2, 1.0)
    filt, packed, _ = settings(block, scaled, 3, info, "full")
    got, coded = run_packed(gpu, fwd, inv, pw.to_stack(clip_of(block, 3), block), (nb,) + tuple(scaled) + (3,), info, packed, filt, keep=tr.KEEP[(block, scaled)])
    back = pw.from_stack(got, scaled)
    assert np.array_equal(back, vol), int((back != vol).sum())
    assert coded == cv > 0


ORACLE_PAIRS = [tr.PAIRS[0], tr.PAIRS[1], tr.PAIRS[4]]


@pytest.mark.parametrize("pair", ORACLE_PAIRS, ids=[tr.pair_id(p) for p in ORACLE_PAIRS])
def test_rgb24_against_the_f64_oracle(gpu, pair):
    """component c's plane is motion_grid_topn_ref's volume from seed 500 + 37 c on: at most 1 LSB, fewer than 2 % of the bytes differing, and
    the blocks tell the reference's ranking from "scale everything, then rank" in every component.  The header's phases meet the same bar on
    the same seeds on the CPU (test_motion_packed_rescale_limit_cpu.py)."""
    from dspfun_amd.engine import motion_packed
    block, scaled = pair
    src, refs = pw.topn_clip(block, scaled)
    for ref in refs:
        assert ref["gap"] > tr.GAP and ref["dc_kept"]
        assert ref["differs"] is (True if any(b > s for b, s in zip(block, scaled)) else None)
    fwd, inv, info = grid_plans(block, scaled)
    got, _ = run_packed(gpu, fwd, inv, src, tuple(info["out_shape"]) + (3,), info, motion_packed("rgb24"), keep=refs[0]["keep"])
    for c, ref in enumerate(refs):
        diff = np.abs(got[..., c].astype(int) - ref["out8"].astype(int))
        print(f"{tr.pair_id(pair)} component {c}: max {diff.max()} LSB, {(diff > 0).mean():.5f} of the bytes differ, seed {ref['seed']}")
        assert diff.max() <= 1 and (diff > 0).mean() < 0.02, (c, diff.max(), (diff > 0).mean())


def test_the_restored_dc_is_the_one_from_before_the_selection_for_the_component_that_asks(gpu):
    """preserve_dc = dc.  Component 1: every block is dark but for four bright pixels at its origin corner, so that more than `keep` low
    frequencies outrank the DC (the uniform range leaves the DC at the pixels' sum and low frequencies near 2 sqrt 2 of it; the pixels differ,
    so the ranks have no ties) and the selection drops it; boost = 2 over the whole active corner puts back the value from BEFORE the
    selection (motion.c:650, :734).  Restoring what the selection left -- zero -- would lower every byte of the block by its mean, most of an
    LSB: four bytes in ten would differ.  Components 0 and 2 keep their DC and are not boosted, so nothing is restored there.  The oracle is
    the f64 reference block by block; the planar limit call agrees byte for byte."""
    from dspfun_amd import _lib
    block, scaled = tr.PAIRS[0]
    keep = tr.KEEP[(block, scaled)]
    src3, refs = pw.topn_clip(block, scaled)
    stack = np.zeros((pw.NB,) + block, dtype=np.uint8)
    i = np.arange(pw.NB)
    stack[:, 0, 0, 0], stack[:, 0, 0, 1], stack[:, 0, 1, 0], stack[:, 1, 0, 0] = 200 + i * 2, 90 + (i * 7) % 23, 50 + (i * 5) % 17, 25 + (i * 3) % 11

    def boost(c, dc):
        c[:4, :4, :4] *= 2.0
        c[0, 0, 0] = dc
    res = [tr.oracle_block(b, block, scaled, keep, boost) for b in stack]
    assert all(r[3][0, 0, 0] == 0.0 for r in res) and all(r[2][0, 0, 0] > 0 for r in res)          # dropped by the selection; not zero before it
    assert min(tr.rule_check(r[2], block, scaled, keep)[0] for r in res) > tr.GAP
    want1 = gr.from_blocks(np.stack([np.clip(np.round(r[1]), 0, 255).astype(np.uint8) for r in res]), scaled, tr.NBLOCKS)
    src = np.array(src3)
    src[..., 1] = gr.from_blocks(stack, block, tr.NBLOCKS)
    fwd, inv, info = grid_plans(block, scaled)
    base = dict(active=info["active"], minbuf_hw=(8, 8), block_depth=8, band_begin=(0, 0, 0), band_end=info["active"], preserve_dc=1)
    p = _lib.MotionPacked()
    p.components = 3
    for k in range(3):
        p.damp[k], p.boost[k], p.grey_add[k] = 1.0, (2.0 if k == 1 else 1.0), 0.0
    out_shape = tuple(info["out_shape"]) + (3,)
    got, _ = run_packed(gpu, fwd, inv, src, out_shape, info, p, dict(base, damp=99.0, boost=99.0), keep=keep)
    diff = np.abs(got[..., 1].astype(int) - want1.astype(int))
    print(f"component 1: max {diff.max()} LSB, {(diff > 0).mean():.5f} of the bytes differ")
    assert diff.max() <= 1 and (diff > 0).mean() < 0.02, (diff.max(), (diff > 0).mean())
    for c in (0, 2):
        d = np.abs(got[..., c].astype(int) - refs[c]["out8"].astype(int))
        assert d.max() <= 1 and (d > 0).mean() < 0.02, (c, d.max(), (d > 0).mean())
    want, _ = run_planes(gpu, fwd, inv, src, out_shape, info, [dict(base, damp=1.0, boost=2.0 if k == 1 else 1.0) for k in range(3)], keep)
    assert np.array_equal(got, want)


def test_refusals_write_nothing(gpu):
    torch = gpu
    from dspfun_amd import DspfftError
    from dspfun_amd.engine import motion_grid_plans, motion_packed
    block, scaled = tr.PAIRS[0]
    fwd, inv, info = grid_plans(block, scaled)
    p3 = motion_packed("rgb24")
    src = torch.from_numpy(np.array(clip_of((16, 16, 16), 4))).to("cuda:0").reshape(-1)          # as large as any clip asked for below
    n = src.numel()
    whole, out = pw.guarded(n, fill=pw.MARK)

    def refused(f, i, reason, packed=p3, keep=16, d_out=None, nfo=info):
        with pytest.raises(DspfftError, match=reason):
            f.roundtrip_u8_packed_rescale(i, src.data_ptr(), d_out or out.data_ptr(), nfo["out_mul"], packed, stream=torch.cuda.current_stream().cuda_stream,
                                          coeff_limit=keep, outside_mul=nfo["limit_outside_mul"])
        torch.cuda.synchronize()
        assert bool((whole == pw.MARK).all())

    fe, ie, _ = motion_grid_plans(gr.shapes(block, block, tr.NBLOCKS)[0], block, block)
    refused(fe, ie, "equal extents")
    for comps in (1, 5):
        pc = motion_packed("rgb24")
        pc.components = comps
        refused(fwd, inv, f"with a coefficient limit: components must be 2, 3 or 4 bytes per pixel, got {comps}", packed=pc)
    f16, i16, info16 = grid_plans(*tr.PAIRS[3])
    refused(f16, i16, "with a coefficient limit.*64 KB of LDS", packed=motion_packed("rgba"), keep=40, nfo=info16)
    refused(fwd, inv, "overlap", d_out=src.data_ptr())
    with pytest.raises(DspfftError, match="outside_mul"):
        fwd.roundtrip_u8_packed_rescale(inv, src.data_ptr(), out.data_ptr(), info["out_mul"], p3, coeff_limit=16, outside_mul=0.0)
    torch.cuda.synchronize()
    assert bool((whole == pw.MARK).all())
