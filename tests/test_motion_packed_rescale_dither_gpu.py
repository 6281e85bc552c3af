"""motion -b with -s AND -d on packed 8-bit pixels on the device, with and without --coeff-limit (block_rescale_packed_dither.hip,
dspfft_execute_roundtrip_u8_packed_rescale_dither).  The kernel's inverse x pass leaves in its tile bit for bit what the planar dithered call
leaves in its work buffer, and one thread walks each plane with the planar store's arithmetic (dither_core.h), so the oracle needs no tolerance:
the bytes equal Plan.roundtrip_u8_dither (with coeff_limit: its limit twin) on the same planar grid pair on each de-interleaved component with
that component's damp / boost / grey_add, and d_coeffs_coded is the sum of the planar counts.  The walk itself is pinned to the reference's by
test_motion_dither_gpu.py and, for these phases, by test_motion_packed_rescale_dither_cpu.py.  Clips are tr.NBLOCKS blocks; every packed output
lies between two marker pages."""
import functools
import math

import numpy as np
import pytest

import motion_grid_ref as gr
import motion_grid_topn_ref as tr
import oracle_lib as ol
import packed_rescale_wide as pw
from test_motion_packed_rescale_gpu import settings

pytestmark = pytest.mark.gpu
# down, up, 2-D up, mixed (8x8x8 -> 4x16x8)
PAIRS = [tr.PAIRS[0], tr.PAIRS[1], tr.PAIRS[5], gr.PAIRS[2]]
KEEP = {PAIRS[0]: 16, PAIRS[1]: 12, PAIRS[2]: 12, PAIRS[3]: 24}
CASES = [(p, 3) for p in PAIRS] + [(PAIRS[0], 4)]
CASE_IDS = [gr.pair_id(p) + f"-c{c}" for p, c in CASES]
SRGB = "iec61966-2-1"


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
    c = ol.synth_u8(0xD1A + comps + 16 * block[0] + block[2], int(np.prod(shape)) * comps).reshape(shape + (comps,))
    c.setflags(write=False)
    return c


def run_packed(torch, fwd, inv, src, out_shape, info, packed, filt=None, keep=0):
    n = int(np.prod(out_shape))
    whole, out = pw.guarded(n)
    d_in = torch.from_numpy(np.array(src)).to("cuda:0").reshape(-1)
    coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    fwd.roundtrip_u8_packed_rescale_dither(inv, d_in.data_ptr(), out.data_ptr(), info["scalefactor"], info["normalization"], packed, filter=filt, coeff_limit=keep,
                                           outside_mul=info["limit_outside_mul"], d_coded=coded.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert pw.markers_intact(whole, n), "the call wrote outside the clip"
    return out.cpu().numpy().reshape(out_shape), int(coded.item())


def run_planes(torch, fwd, inv, src, out_shape, info, planes, keep=0):
    """Plan.roundtrip_u8_dither of the same pair on every de-interleaved component, through its float work buffer"""
    want = np.empty(out_shape, dtype=np.uint8)
    counts = []
    stream = torch.cuda.current_stream().cuda_stream
    for c, filt in enumerate(planes):
        d_in = torch.from_numpy(np.array(src[..., c])).to("cuda:0")
        d_out = torch.zeros(out_shape[:-1], dtype=torch.uint8, device="cuda:0")
        work = torch.zeros(out_shape[:-1], dtype=torch.float32, device="cuda:0")
        coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        fwd.roundtrip_u8_dither(inv, d_in.data_ptr(), d_out.data_ptr(), work.data_ptr(), info["scalefactor"], info["normalization"], filter=filt, d_coded=coded.data_ptr(),
                                stream=stream, coeff_limit=keep, outside_mul=info["limit_outside_mul"])
        torch.cuda.synchronize()
        want[..., c] = d_out.cpu().numpy()
        counts.append(int(coded.item()))
    return want, counts


def both(torch, block, scaled, comps, name, keep=0, trc=None, pdc=2):
    fwd, inv, info = grid_plans(block, scaled)
    for pl, t in zip((fwd, inv), trc or ()):
        pl.set_u8_trc(t)
    src = clip_of(block, comps)
    filt, packed, planes = settings(block, scaled, comps, info, name, pdc=pdc)
    out_shape = tuple(info["out_shape"]) + (comps,)
    got, coded = run_packed(torch, fwd, inv, src, out_shape, info, packed, filt, keep)
    want, counts = run_planes(torch, fwd, inv, src, out_shape, info, planes, keep)
    return got, coded, want, counts


@pytest.mark.parametrize("limit", [False, True], ids=["plain", "limit"])
@pytest.mark.parametrize("name", ["none", "dc", "grey"])
@pytest.mark.parametrize("pair,comps", CASES, ids=CASE_IDS)
def test_packed_dithered_call_equals_the_planar_dithered_call_on_every_component(gpu, pair, comps, name, limit):
    block, scaled = pair
    got, coded, want, counts = both(gpu, block, scaled, comps, "none" if name == "none" else "full", keep=KEEP[pair] if limit else 0, pdc=1 if name == "dc" else 2)
    assert np.array_equal(got, want), int((got != want).sum())
    assert coded == sum(counts) and (name == "none") == (coded == 0), (coded, counts)


def test_the_dither_acts_and_the_limit_acts(gpu):
    """against the undithered packed call, and with against without a limit; a limit of the whole embedding is the call without one"""
    block, scaled = PAIRS[0]
    fwd, inv, info = grid_plans(block, scaled)
    src = clip_of(block, 3)
    filt, packed, _ = settings(block, scaled, 3, info, "full")
    out_shape = tuple(info["out_shape"]) + (3,)
    d, _ = run_packed(gpu, fwd, inv, src, out_shape, info, packed, filt)
    dl, _ = run_packed(gpu, fwd, inv, src, out_shape, info, packed, filt, keep=16)
    whole, _ = run_packed(gpu, fwd, inv, src, out_shape, info, packed, filt, keep=512)
    n = int(np.prod(out_shape))
    guard, out = pw.guarded(n)
    d_in = gpu.from_numpy(np.array(src)).to("cuda:0")
    fwd.roundtrip_u8_packed_rescale(inv, d_in.data_ptr(), out.data_ptr(), info["out_mul"], packed, filter=filt, stream=gpu.cuda.current_stream().cuda_stream)
    gpu.cuda.synchronize()
    plain = out.cpu().numpy().reshape(out_shape)
    assert pw.markers_intact(guard, n)
    assert not np.array_equal(d, plain)
    assert not np.array_equal(dl, d) and np.array_equal(whole, d)


@pytest.mark.parametrize("limit", [False, True], ids=["plain", "limit"])
@pytest.mark.parametrize("pair", [PAIRS[0], PAIRS[2]], ids=[gr.pair_id(PAIRS[0]), gr.pair_id(PAIRS[2])])
def test_transfer_characteristic_on_both_ends_and_on_one(gpu, pair, limit):
    block, scaled = pair
    keep = KEEP[pair] if limit else 0
    got, coded, want, counts = both(gpu, block, scaled, 3, "full", keep=keep, trc=(SRGB, SRGB))
    assert np.array_equal(got, want), int((got != want).sum())
    assert coded == sum(counts) > 0
    got1, _, want1, _ = both(gpu, block, scaled, 3, "full", keep=keep, trc=(SRGB, 0))
    assert np.array_equal(got1, want1) and not np.array_equal(want1, want)
    got2, _, want2, _ = both(gpu, block, scaled, 3, "full", keep=keep, trc=(0, SRGB))
    assert np.array_equal(got2, want2) and not np.array_equal(want2, want) and not np.array_equal(want2, want1)


@pytest.mark.parametrize("limit", [False, True], ids=["plain", "limit"])
@pytest.mark.parametrize("pair", [PAIRS[0], PAIRS[1]], ids=[gr.pair_id(PAIRS[0]), gr.pair_id(PAIRS[1])])
def test_block_major_stacks_give_the_volume_layouts_bytes(gpu, pair, limit):
    from dspfun_amd import Plan, REDFT10, REDFT01
    block, scaled = pair
    keep = KEEP[pair] if limit else 0
    vol, cv, want, _ = both(gpu, block, scaled, 3, "full", keep=keep)
    assert np.array_equal(vol, want)
    _, _, info = grid_plans(block, scaled)
    r2 = math.sqrt(2.0)
    vf, vi = int(np.prod(block)), int(np.prod(scaled))
    fwd = Plan.many_r2r(list(block), [REDFT10] * 3, howmany=pw.NB, idist=vf, odist=vf).set_scale(2 * r2)
    inv = Plan.many_r2r(list(scaled), [REDFT01] * 3, howmany=pw.NB, idist=vi, odist=vi).set_scale(1 / (2 * r2))
    for a in range(3):
        fwd.set_axis_scale0(a, 1.0, 1.0 / r2)
        inv.set_axis_scale0(a, r2, 1.0)
    assert "block-major" in fwd.describe() and "block-major" in inv.describe()
    filt, packed, _ = settings(block, scaled, 3, info, "full")
    got, coded = run_packed(gpu, fwd, inv, pw.to_stack(clip_of(block, 3), block), (pw.NB,) + tuple(scaled) + (3,), info, packed, filt, keep=keep)
    back = pw.from_stack(got, scaled)
    assert np.array_equal(back, vol), int((back != vol).sum())
    assert coded == cv > 0


def test_a_short_last_group_and_one_pixel_block(gpu, monkeypatch):
    block, scaled = PAIRS[0]
    rule, coded, _, _ = both(gpu, block, scaled, 3, "full", keep=16)
    for forced in ("2", "1"):
        monkeypatch.setenv("DSPFFT_PACKED_G", forced)
        got, coded2, _, _ = both(gpu, block, scaled, 3, "full", keep=16)
        assert np.array_equal(got, rule) and coded2 == coded > 0, forced


def test_refusals_write_nothing(gpu):
    torch = gpu
    from dspfun_amd import DspfftError
    from dspfun_amd.engine import motion_grid_plans, motion_packed
    block, scaled = PAIRS[0]
    fwd, inv, info = grid_plans(block, scaled)
    p3 = motion_packed("rgb24")
    src = torch.from_numpy(np.array(clip_of((16, 16, 16), 4))).to("cuda:0").reshape(-1)          # as large as any clip asked for below
    whole, out = pw.guarded(src.numel(), fill=pw.MARK)
    name = "dithered roundtrip on packed 8-bit pixels over a rescaled grid of blocks"

    def refused(f, i, reason, packed=p3, keep=0, d_out=None, nfo=info, sf=None):
        with pytest.raises(DspfftError, match=reason):
            f.roundtrip_u8_packed_rescale_dither(i, src.data_ptr(), d_out or out.data_ptr(), nfo["scalefactor"] if sf is None else sf, nfo["normalization"], packed,
                                                 coeff_limit=keep, outside_mul=nfo["limit_outside_mul"], stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((whole == pw.MARK).all())

    fe, ie, _ = motion_grid_plans(gr.shapes(block, block, tr.NBLOCKS)[0], block, block)
    refused(fe, ie, name + ".*equal extents")
    for comps in (1, 5):
        pc = motion_packed("rgb24")
        pc.components = comps
        refused(fwd, inv, f"components must be 2, 3 or 4 bytes per pixel, got {comps}", packed=pc)
    f16, i16, info16 = grid_plans(*tr.PAIRS[3])
    refused(f16, i16, name + ".*64 KB of LDS", packed=motion_packed("rgba"), keep=40, nfo=info16)
    refused(fwd, inv, "overlap", d_out=src.data_ptr())
    refused(fwd, inv, "scalefactor and normalization must be finite and > 0", sf=0.0)
    refused(fwd, inv, "scalefactor and normalization must be finite and > 0", sf=float("nan"))
