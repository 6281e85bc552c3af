"""motion -d on packed 8-bit pixels on the device: dspfft_execute_roundtrip_u8_packed_dither (block_packed_dither.hip),
dspfft_motion_dither_u8_packed (motion_dither.hip with an element step) and dspfft_execute_roundtrip_u8_packed_frames_dither.  Byte equality
throughout, no tolerance:
  small blocks   the bytes equal Plan.roundtrip_u8_dither (and its coeff_limit form) of the SAME plan pair on each de-interleaved component
                 with that component's damp / boost / grey_add, the coded count the sum of the planar counts
  stand-alone    the bytes equal tests/dither_ref.py: dither_planes (pinned to the reference's compiled lines) per component
  full frames    the bytes equal dither_planes of the floats the call leaves in d_work, and those floats and the coded count are the
                 composition's: dspfft_u8_to_f32 -> execute(fwd) -> motion_filter_packed -> execute(inv)
Every output goes into a buffer with a marker page on each side."""
import math

import numpy as np
import pytest

import dither_ref as dr
import motion_packed_frames_ref as pf
import oracle_lib as ol
from test_motion_packed_gpu import check_frame, clip_of, framed, grid_plans, run_packed, settings
from test_motion_packed_frames_gpu import unfused

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
SRGB = "iec61966-2-1"


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from dspfun_amd import _lib
    _lib.load()
    return torch


# ---- small blocks ----
def run_packed_dither(torch, fwd, inv, src, info, packed, filt=None, keep=0, in_place=False):
    n = src.size
    buf, out = framed(torch, n)
    d_in = torch.from_numpy(np.ascontiguousarray(src)).to("cuda:0").reshape(-1)
    if in_place:
        out.copy_(d_in)
        d_in = out
    coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    fwd.roundtrip_u8_packed_dither(inv, d_in.data_ptr(), out.data_ptr(), info["scalefactor"], info["normalization"], packed, filter=filt, coeff_limit=keep,
                                   d_coded=coded.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check_frame(buf, n)
    return out.cpu().numpy().reshape(src.shape), int(coded.item())


def run_planes_dither(torch, fwd, inv, src, info, planes, keep=0):
    """the planar dithered call of the same plan pair on every de-interleaved component"""
    want = np.empty_like(src)
    counts = []
    stream = torch.cuda.current_stream().cuda_stream
    for c, filt in enumerate(planes):
        d_in = torch.from_numpy(np.ascontiguousarray(src[..., c])).to("cuda:0")
        d_out = torch.empty_like(d_in)
        work = torch.empty(d_in.numel(), dtype=torch.float32, device="cuda:0")
        coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        fwd.roundtrip_u8_dither(inv, d_in.data_ptr(), d_out.data_ptr(), work.data_ptr(), info["scalefactor"], info["normalization"], filter=filt,
                                d_coded=coded.data_ptr(), stream=stream, coeff_limit=keep)
        torch.cuda.synchronize()
        want[..., c] = d_out.cpu().numpy()
        counts.append(int(coded.item()))
    return want, counts


def coarse(filt, block):
    """the filter with motion's quantiser scale (motion.c:570: -q times 8 sqrt(block volume)): the helper's raw 12 or 20 leaves the floats of
    a large block so close to integers that the dither has nothing to diffuse"""
    return None if filt is None else dict(filt, quantizer=filt["quantizer"] * 8 * math.sqrt(float(block[0] * block[1] * block[2])))


BLOCKS = [(1, 4, 4), (1, 8, 8), (8, 8, 8), (1, 32, 32), (8, 16, 4)]
CASES = [(b, c) for b in BLOCKS for c in (2, 3, 4)] + [((16, 16, 16), 3)]


@pytest.mark.parametrize("block,comps", CASES, ids=["x".join(map(str, b)) + f"-c{c}" for b, c in CASES])
def test_dithered_packed_call_equals_the_planar_dithered_call_on_every_component(gpu, block, comps):
    """no filter, --quant alone, the per-component band-pass with preserve_dc; with and without --coeff-limit; out of place and in place"""
    fwd, inv, info = grid_plans(block)
    src = clip_of(block, comps)
    e = block[0] * block[1] * block[2]
    for name in ("none", "quant", "full"):
        filt, packed, planes = settings(block, comps, info, name)
        filt, planes = coarse(filt, block), [coarse(f, block) for f in planes]
        for keep in (0, max(2, e // 8)):
            want, counts = run_planes_dither(gpu, fwd, inv, src, info, planes, keep)
            for in_place in (False, True):
                got, coded = run_packed_dither(gpu, fwd, inv, src, info, packed, filt, keep, in_place)
                assert np.array_equal(got, want), (name, keep, in_place, int((got != want).sum()))
                assert coded == sum(counts) and (name == "none") == (coded == 0), (name, keep, coded, counts)
            if name != "none":          # not vacuous: the dither moved bytes of the undithered packed call
                plain, _ = run_packed(gpu, fwd, inv, src, info["out_mul"], packed, filt, keep=keep)
                assert (plain != want).any(), (name, keep)


def test_dithered_packed_call_with_a_transfer_characteristic_at_both_ends(gpu):
    block, comps = (8, 8, 8), 3
    fwd, inv, info = grid_plans(block)
    src = clip_of(block, comps)
    filt, packed, planes = settings(block, comps, info, "full")
    filt, planes = coarse(filt, block), [coarse(f, block) for f in planes]
    linear = run_packed_dither(gpu, fwd, inv, src, info, packed, filt)[0]
    fwd.set_u8_trc(SRGB)
    inv.set_u8_trc(SRGB)
    for keep in (0, 64):
        got, coded = run_packed_dither(gpu, fwd, inv, src, info, packed, filt, keep)
        want, counts = run_planes_dither(gpu, fwd, inv, src, info, planes, keep)
        assert np.array_equal(got, want), (keep, int((got != want).sum()))
        assert coded == sum(counts) > 0
    assert not np.array_equal(want, linear)
    # the store's end alone
    fwd.set_u8_trc(0)
    got, _ = run_packed_dither(gpu, fwd, inv, src, info, packed, filt)
    assert np.array_equal(got, run_planes_dither(gpu, fwd, inv, src, info, planes)[0])


# ---- the stand-alone kernel ----
def coeffs_of(seed, F, H, W, comps, sf, nm):
    """[F][H][W][C] floats built like dither_ref.case_inputs: pels in about [-20, 275] with a plateau of exact halves"""
    mul = F64(sf) * F64(nm) * F64(nm)
    u = ol.synth_f32(0xD17E1000 + seed, F * H * W * comps).reshape(F, H, W, comps).astype(F64)
    c = ((u * 295.0 - 20.0) / mul).astype(F32)
    ph, pw = max(1, H // 4), max(1, W // 3)
    k = (np.arange(ph * pw * comps).reshape(ph, pw, comps) % 200).astype(F64) + 20.5
    c[:, :ph, :pw, :] = (k / mul).astype(F32)
    return c


def run_stand_alone(torch, co, W, sf, nm, trc=0):
    """co: [F][H][P][C] floats, P >= W the row pitch in pixels.  Returns the [F][H][P][C] bytes (0xEE where nothing was written)."""
    from dspfun_amd.engine import motion_dither_u8_packed
    F, H, P, comps = co.shape
    n = co.size
    buf, out = framed(torch, n)
    out.fill_(0xEE)
    d_co = torch.from_numpy(co).to("cuda:0")
    motion_dither_u8_packed(out.data_ptr(), d_co.data_ptr(), (1, H, W), comps, row_pitch=P, nblocks=(F, 1, 1), block_step=(H * P, 0, 0), scalefactor=sf,
                            normalization=nm, stream=torch.cuda.current_stream().cuda_stream, trc=trc)
    torch.cuda.synchronize()
    check_frame(buf, n)
    assert np.array_equal(d_co.cpu().numpy().view(np.uint32), co.view(np.uint32))          # the coefficients are only read
    return out.cpu().numpy().reshape(co.shape)


SF_OF = lambda H, W: 1.0
NM_OF = lambda H, W: 1 / np.sqrt(float(H * W * 8))
# serial regime; wavefront regime with two and three bands and widths that are no multiple of the chunk; degenerate planes
ALONE = [(2, 9, 20, 3), (2, 70, 45, 3), (1, 130, 33, 4), (1, 1, 9, 2), (1, 9, 1, 2)]


@pytest.mark.parametrize("F,H,W,comps", ALONE, ids=lambda v: str(v))
def test_stand_alone_kernel_equals_the_reference_dither_on_every_component(gpu, F, H, W, comps):
    co = coeffs_of(H * W, F, H, W, comps, SF_OF(H, W), NM_OF(H, W))
    got = run_stand_alone(gpu, co, W, SF_OF(H, W), NM_OF(H, W))
    for c in range(comps):
        want = dr.dither_planes(np.ascontiguousarray(co[..., c]), SF_OF(H, W), NM_OF(H, W))
        assert np.array_equal(got[..., c], want), (c, int((got[..., c] != want).sum()))
    assert len(np.unique(got)) > (8 if H * W > 9 else 2)


@pytest.mark.parametrize("F,H,W,comps,P", [(2, 9, 20, 3, 23), (1, 70, 45, 2, 48)], ids=["serial", "wavefront"])
def test_stand_alone_kernel_with_a_row_pitch_above_the_width(gpu, F, H, W, comps, P):
    co = coeffs_of(7 + H, F, H, P, comps, SF_OF(H, W), NM_OF(H, W))
    got = run_stand_alone(gpu, co, W, SF_OF(H, W), NM_OF(H, W))
    assert (got[:, :, W:, :] == 0xEE).all()
    for c in range(comps):
        want = dr.dither_planes(np.ascontiguousarray(co[:, :, :W, c]), SF_OF(H, W), NM_OF(H, W))
        assert np.array_equal(got[:, :, :W, c], want), c


@pytest.mark.parametrize("F,H,W,comps", [(2, 9, 20, 3), (1, 70, 45, 4)], ids=["serial", "wavefront"])
def test_stand_alone_kernel_with_a_transfer_characteristic_equals_the_planar_kernel_on_every_plane(gpu, F, H, W, comps):
    from dspfun_amd.engine import motion_dither_u8
    torch = gpu
    co = coeffs_of(11 + H, F, H, W, comps, SF_OF(H, W), NM_OF(H, W))
    got = run_stand_alone(torch, co, W, SF_OF(H, W), NM_OF(H, W), trc=SRGB)
    assert not np.array_equal(got, run_stand_alone(torch, co, W, SF_OF(H, W), NM_OF(H, W)))
    for c in range(comps):
        plane = torch.from_numpy(np.ascontiguousarray(co[..., c])).to("cuda:0")
        o = torch.zeros(plane.shape, dtype=torch.uint8, device="cuda:0")
        motion_dither_u8(o.data_ptr(), plane.data_ptr(), (1, H, W), nblocks=(F, 1, 1), block_step=(H * W, 0, 0), scalefactor=SF_OF(H, W), normalization=NM_OF(H, W),
                         stream=torch.cuda.current_stream().cuda_stream, trc=SRGB)
        torch.cuda.synchronize()
        assert np.array_equal(got[..., c], o.cpu().numpy()), c


# ---- full frames ----
def composition_floats(torch, L, fwd, inv, src, packed, filt, trc_in=0):
    """dspfft_u8_to_f32 -> execute(fwd) -> motion_filter_packed -> execute(inv).  Returns (floats [F][h][w][C], coded)."""
    from dspfun_amd.engine import motion_filter_packed
    F, h, w, comps = src.shape
    n = src.size
    s = pf.stream_of(torch)
    d_in = torch.from_numpy(np.array(src)).to("cuda:0").reshape(-1)
    wk = torch.empty(n, dtype=torch.float32, device="cuda:0")
    coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    if trc_in:
        assert L.dspfft_u8_to_f32_trc(wk.data_ptr(), d_in.data_ptr(), n, trc_in, s) == 0
    else:
        assert L.dspfft_u8_to_f32(wk.data_ptr(), d_in.data_ptr(), n, s) == 0
    fwd.execute(wk.data_ptr(), stream=s)
    if filt is not None:
        motion_filter_packed(wk, h, w, comps, F, packed, dict(filt, active=(1, h, w), minbuf_hw=(h, w), block_depth=1), d_coded=coded.data_ptr(), stream=s)
    inv.execute(wk.data_ptr(), stream=s)
    torch.cuda.synchronize()
    return wk.cpu().numpy().reshape(src.shape), int(coded.item())


def run_frames_dither(torch, fwd, inv, src, info, packed, filt=None, in_place=False):
    """Returns (bytes, coded, the floats left in d_work)"""
    n = src.size
    buf, out = framed(torch, n)
    d_in = torch.from_numpy(np.array(src)).to("cuda:0").reshape(-1)
    if in_place:
        out.copy_(d_in)
        d_in = out
    wk = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda:0")
    coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    fwd.roundtrip_u8_packed_frames_dither(inv, d_in.data_ptr(), out.data_ptr(), wk.data_ptr(), info["scalefactor"], info["normalization"], packed, filter=filt,
                                          d_coded=coded.data_ptr(), stream=pf.stream_of(torch))
    torch.cuda.synchronize()
    check_frame(buf, n)
    return out.cpu().numpy().reshape(src.shape), int(coded.item()), wk.cpu().numpy().reshape(src.shape)


def dithered(floats, info):
    out = np.empty(floats.shape, dtype=np.uint8)
    for c in range(floats.shape[-1]):
        out[..., c] = dr.dither_planes(np.ascontiguousarray(floats[..., c]), info["scalefactor"], info["normalization"])
    return out


# the fused packed column roundtrip (256 rows), the generic passes, two components
FRAMES = [(2, 256, 256, 3), (2, 256, 80, 3), (3, 24, 40, 4), (2, 16, 12, 2)]


@pytest.mark.parametrize("F,h,w,comps", FRAMES, ids=lambda v: str(v))
def test_dithered_frames_call_equals_its_composition_and_the_reference_dither(gpu, F, h, w, comps):
    from dspfun_amd import _lib
    from dspfun_amd.engine import motion_packed_frame_plans
    L = _lib.load()
    fwd, inv, info = motion_packed_frame_plans(F, h, w, comps)
    src = pf.clip_of(F, h, w, comps)
    for name in ("none", "quant", "full-grey"):
        filt, packed, _ = pf.settings(h, w, comps, info, name)
        floats, wcoded = composition_floats(gpu, L, fwd, inv, src, packed, filt)
        assert (name == "none") == (wcoded == 0)
        want = dithered(floats, info)
        assert len(np.unique(want)) > 8
        if name != "none":          # not vacuous: the dither moved bytes of the undithered call
            assert (want != pf.run_call(gpu, fwd, inv, src, info, packed, filt)[0]).any(), name
        for fused in (True, False):
            for in_place in (False, True):
                if fused:
                    got, coded, left = run_frames_dither(gpu, fwd, inv, src, info, packed, filt, in_place)
                else:
                    with unfused():
                        got, coded, left = run_frames_dither(gpu, fwd, inv, src, info, packed, filt, in_place)
                assert np.array_equal(left.view(np.uint32), floats.view(np.uint32)), (name, fused, in_place)
                assert np.array_equal(got, want), (name, fused, in_place, int((got != want).sum()))
                assert coded == wcoded, (name, fused, in_place, coded, wcoded)


def test_dithered_frames_call_with_a_transfer_characteristic(gpu):
    """on `fwd` the flat sweep decodes, on `inv` the dither's trc variant encodes"""
    from dspfun_amd import _lib
    from dspfun_amd.engine import motion_packed_frame_plans, trc_id
    L = _lib.load()
    F, h, w, comps = 3, 24, 40, 4
    fwd, inv, info = motion_packed_frame_plans(F, h, w, comps)
    plain = motion_packed_frame_plans(F, h, w, comps)
    src = pf.clip_of(F, h, w, comps)
    fwd.set_u8_trc(SRGB)
    inv.set_u8_trc(SRGB)
    filt, packed, _ = pf.settings(h, w, comps, info, "full-grey")
    floats, wcoded = composition_floats(gpu, L, plain[0], plain[1], src, packed, filt, trc_in=trc_id(SRGB, L))
    got, coded, left = run_frames_dither(gpu, fwd, inv, src, info, packed, filt)
    assert np.array_equal(left.view(np.uint32), floats.view(np.uint32)) and coded == wcoded
    want = run_stand_alone(gpu, floats, w, info["scalefactor"], info["normalization"], trc=SRGB)
    assert np.array_equal(got, want) and not np.array_equal(got, dithered(floats, info))


def test_refusals_on_the_device_write_nothing(gpu):
    from dspfun_amd.engine import DspfftError, motion_packed, motion_packed_frame_plans
    torch = gpu
    # a width above the wavefront kernel's LDS rings: refused with that kernel's message before any pass runs
    F, h, w, comps = 1, 70, 9600, 2
    fwd, inv, info = motion_packed_frame_plans(F, h, w, comps)
    n = F * h * w * comps
    src = torch.full((n,), 77, dtype=torch.uint8, device="cuda:0")
    wk = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda:0")
    buf, out = framed(torch, n)
    with pytest.raises(DspfftError, match="plane too wide for the wavefront kernel's LDS rings"):
        fwd.roundtrip_u8_packed_frames_dither(inv, src.data_ptr(), out.data_ptr(), wk.data_ptr(), info["scalefactor"], info["normalization"], motion_packed("ya8"),
                                              stream=pf.stream_of(torch))
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all()) and bool(torch.isnan(wk).all())
    # a rescaled grid pair on the small-block entry
    from dspfun_amd.engine import motion_grid_plans
    fg, ig, ginfo = motion_grid_plans((16, 16, 88), (8, 8, 8), (4, 4, 4))
    with pytest.raises(DspfftError, match="-d on a packed rescaled grid is not implemented"):
        fg.roundtrip_u8_packed_dither(ig, src.data_ptr(), out.data_ptr(), ginfo["scalefactor"], ginfo["normalization"], motion_packed("rgb24"), stream=pf.stream_of(torch))
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
