"""motion -b 1x1xD (-s 1x1xD') on the device (temporal_rt.hip through dspfft_execute_roundtrip*): every block in time and every pixel
column of a 6 x 50 clip in ONE launch, against the f64 oracle column by column (tests/motion_temporal_ref.py), against the parent's
one-line device path, and against the compositions include/dspfft.h promises (the float call between the two conversions, a transfer
characteristic, the dithered call, in place).  P = 300: the last tile is short at every tile width."""
import math

import numpy as np
import pytest

import motion_ref as mr
import motion_temporal_ref as tr

pytestmark = pytest.mark.gpu
IDS = [tr.pair_id(p) for p in tr.PAIRS]
TRC = "iec61966-2-1"


def torch_or_fail():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return torch


def plans(vol, D, S, trc=None):
    from dspfun_amd.engine import motion_temporal_plans
    fwd, inv, info = motion_temporal_plans(vol.shape, D, S)
    if trc:
        fwd.set_u8_trc(trc); inv.set_u8_trc(trc)
    return fwd, inv, info


def run_u8(torch, D, S, vol, flt=None, trc=None, coded=False, dither=False, in_place=False, work=False):
    fwd, inv, info = plans(vol, D, S, trc)
    d_in = torch.from_numpy(np.array(vol)).to("cuda:0")
    d_out = d_in if in_place else torch.full(info["out_shape"], 9, dtype=torch.uint8, device="cuda:0")
    d_coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    d_work = torch.full(info["out_shape"], 7.0, dtype=torch.float32, device="cuda:0") if work else None
    wp = d_work.data_ptr() if work else None
    if dither:
        fwd.roundtrip_u8_dither(inv, d_in.data_ptr(), d_out.data_ptr(), wp, info["scalefactor"], info["normalization"], filter=flt,
                                d_coded=d_coded.data_ptr() if coded else 0)
    else:
        fwd.roundtrip_u8(inv, d_in.data_ptr(), d_out.data_ptr(), wp, info["out_mul"], filter=flt, d_coded=d_coded.data_ptr() if coded else 0)
    torch.cuda.synchronize()
    if work:
        assert bool((d_work == 7.0).all())                      # the call has no float intermediate
    out = d_out.cpu().numpy()[:info["out_shape"][0]]
    return (out, int(d_coded.item())) if coded else out


def run_f32(torch, D, S, vol, src, flt=None):
    """float in (a device tensor of the whole clip) -> the float output clip as a device tensor"""
    fwd, inv, info = plans(vol, D, S)
    d_out = torch.full(info["out_shape"], 7.0, dtype=torch.float32, device="cuda:0")
    fwd.roundtrip(inv, src.data_ptr(), d_out.data_ptr(), filter=flt)
    torch.cuda.synchronize()
    return d_out


@pytest.mark.parametrize("D,S", tr.PAIRS, ids=IDS)
def test_u8_against_the_oracle(D, S):
    """plain, a band with damp and boost, a threshold, preserve-dc = dc and grey, a quantiser: the bytes are the oracle's wherever its pixel
    is farther than the float tolerance from k + 1/2 and within 1 elsewhere; the coded count is the oracle's exactly"""
    torch = torch_or_fail()
    for kind in tr.KINDS:
        ref = tr.case(D, S, kind)
        got, coded = run_u8(torch, D, S, ref["vol"], flt=ref["filter"], coded=True, work=kind == "plain")
        diff = np.abs(got.astype(int) - ref["out8"].astype(int))
        print(f"{D}-{S} {kind}: {int((diff > 0).sum())} of {diff.size} bytes differ, max {diff.max()}; "
              f"{int(tr.near_half(ref['pel']).sum())} oracle pixels within {tr.TOL:.2e} of a half" + (f"; coded {coded} / {ref['coded']}" if kind == "quant" else ""))
        tr.check_bytes(got, ref)
        if kind == "quant":
            assert coded == ref["coded"] > 0


def one_line_path(torch, D, S, vol, flt):
    """the parent's own device path for one line: howmany = 1 rank-1 plans in one embedding of max(D, D') contiguous floats
    (one_block_plans of test_motion_block_rescale_gpu.py), over every pixel column of every block; returns the float output clip"""
    from dspfun_amd import Plan, REDFT10, REDFT01
    M, r2 = max(D, S), math.sqrt(2.0)
    fwd = Plan.many_r2r([D], [REDFT10], inembed=[M], onembed=[M]).set_scale(2 * r2 * 2).set_axis_scale0(0, 1.0, 1.0 / r2)
    inv = Plan.many_r2r([S], [REDFT01], inembed=[M], onembed=[M]).set_scale(2 / (2 * r2)).set_axis_scale0(0, r2, 1.0)
    cols, nd = tr.columns(np.asarray(vol), D)
    lines = np.zeros((len(cols), M), dtype=np.float32)
    lines[:, :D] = cols
    d = torch.from_numpy(lines).to("cuda:0")
    f = dict(flt, block_depth=M)
    for i in range(len(cols)):
        fwd.roundtrip(inv, d.data_ptr() + 4 * i * M, filter=f)
    torch.cuda.synchronize()
    out = d.cpu().numpy()[:, :S]
    return np.ascontiguousarray(out.reshape(nd, -1, S).transpose(0, 2, 1)).reshape((nd * S,) + vol.shape[1:])


@pytest.mark.parametrize("D,S", tr.RESCALED, ids=[tr.pair_id(p) for p in tr.RESCALED])
def test_f32_against_the_f64_pixels_and_the_one_line_path(D, S):
    """float in and out with a band filter: the largest error in pixels (value x out_mul against the oracle's f64 pixel) is at most twice
    that of the parent's one-line path over the same columns, measured here on the same device: only the summation order differs
    (test_motion_block_rescale_gpu.py's margin).  Measured on an MI355X (profiles/r14_motion_temporal.txt): see the numbers there."""
    torch = torch_or_fail()
    ref = tr.case(D, S, "band")
    sf, nm = mr.consts((D, 1, 1), (S, 1, 1))
    src = torch.from_numpy(np.asarray(ref["vol"], dtype=np.float32)).to("cuda:0")
    got = run_f32(torch, D, S, ref["vol"], src, flt=ref["filter"]).cpu().numpy().astype(np.float64) * sf * nm * nm
    one = one_line_path(torch, D, S, ref["vol"], ref["filter"]).astype(np.float64) * sf * nm * nm
    err, err_one = float(np.abs(got - ref["pel"]).max()), float(np.abs(one - ref["pel"]).max())
    print(f"{D}-{S} float, band filter: temporal kernel {err:.3e} pixels, one-line path {err_one:.3e} (bound {2 * err_one:.3e})")
    assert err_one < tr.TOL              # the bound's own reference is sound
    assert err <= 2 * err_one, (err, err_one)


@pytest.mark.parametrize("D,S", [(8, 8), (25, 25), (256, 256), (24, 30), (64, 32)], ids=["8-8", "25-25", "256-256", "24-30", "64-32"])
def test_exact_compositions(D, S):
    """all with a band filter, so that the float leg runs the new kernel; all byte for byte"""
    torch = torch_or_fail()
    from dspfun_amd.engine import u8_to_f32_trc, f32_to_u8_trc
    ref = tr.case(D, S, "band")
    flt, vol = ref["filter"], ref["vol"]
    sf, nm = mr.consts((D, 1, 1), (S, 1, 1))
    d_in = torch.from_numpy(np.array(vol)).to("cuda:0")
    got = run_u8(torch, D, S, vol, flt=flt)
    tr.check_bytes(got, ref)
    # the 8-bit call = dspfft_u8_to_f32 -> the float call -> dspfft_f32_to_u8(out_mul)
    mid = run_f32(torch, D, S, vol, u8_to_f32_trc(d_in, None), flt=flt)
    want = f32_to_u8_trc(mid, None, mul=sf * nm * nm)
    torch.cuda.synchronize()
    assert np.array_equal(got, want.cpu().numpy())
    # with a transfer characteristic on both plans = dspfft_u8_to_f32_trc -> the float call -> dspfft_f32_to_u8_trc
    got_trc = run_u8(torch, D, S, vol, flt=flt, trc=TRC)
    mid = run_f32(torch, D, S, vol, u8_to_f32_trc(d_in, TRC), flt=flt)
    want = f32_to_u8_trc(mid, TRC, mul=sf * nm * nm)
    torch.cuda.synchronize()
    assert np.array_equal(got_trc, want.cpu().numpy())
    assert (got_trc != got).mean() > 0.2                        # and it is not the plain call
    # the dithered call: a 1 x 1 block has nothing to diffuse into
    assert np.array_equal(run_u8(torch, D, S, vol, flt=flt, dither=True), got)
    assert np.array_equal(run_u8(torch, D, S, vol, flt=flt, dither=True, work=True), got)
    # in place, for equal extents: a tile reads all its frames before it writes any (the cropped frame stays)
    if D == S:
        inp = run_u8(torch, D, S, vol, flt=flt, in_place=True)
        assert np.array_equal(inp, got)


def test_unfiltered_equal_extent_float_call_is_the_plans_own_passes():
    """no filter, equal extents, float: nothing of this call changed -- bit for bit what Plan.execute forward then inverse gives -- and a
    pure quantiser, which needs no positions, stays with those passes too (its count is the oracle's)"""
    torch = torch_or_fail()
    for D in (8, 60):
        ref = tr.case(D, D)
        fwd, inv, info = plans(ref["vol"], D, D)
        x = torch.from_numpy(np.asarray(ref["vol"][:3 * D], dtype=np.float32)).to("cuda:0")
        a, b = x.clone(), x.clone()
        fwd.roundtrip(inv, a.data_ptr())
        fwd.execute(b.data_ptr()); inv.execute(b.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        assert float(np.abs(a.cpu().numpy().astype(np.float64) * info["out_mul"] - ref["pel"]).max()) < tr.TOL
        q = tr.case(D, D, "quant")
        c = torch.from_numpy(np.asarray(q["vol"][:3 * D], dtype=np.float32)).to("cuda:0")
        d_coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        fwd.roundtrip(inv, c.data_ptr(), filter=q["filter"], d_coded=d_coded.data_ptr())
        torch.cuda.synchronize()
        assert int(d_coded.item()) == q["coded"]


def test_refusals_that_need_device_plans():
    """a length beyond the narrowest tile, and one whose column pass would need Bluestein above 32 points"""
    torch_or_fail()
    from dspfun_amd.engine import DspfftError
    for D, what in ((1040, "too long for the narrowest tile"), (34, "prime factor above 13")):
        vol = np.zeros((D, 2, 4), dtype=np.uint8)
        fwd, inv, info = plans(vol, D, D)
        with pytest.raises(DspfftError, match=what):
            fwd.roundtrip_u8(inv, 4096, 4096, None, info["out_mul"])
