"""motion -b with -s over a block grid on the device (block_rescale.hip through dspfft_execute_roundtrip*): every block of a 2 x 2 x 9 grid
in ONE launch, against the f64 restatement of the reference block by block (tests/motion_grid_ref.py), against the block-major layout of
the same blocks, and against the compositions include/dspfft.h promises (transfer characteristic, dithered store)."""
import math

import numpy as np
import pytest

import motion_grid_ref as gr
import motion_ref as mr

pytestmark = pytest.mark.gpu
IDS = [gr.pair_id(p) for p in gr.PAIRS]

# Float in and out: the largest error, in pixels (output value x out_mul against the f64 oracle's pixel before rounding), of the ONE-BLOCK
# device path (howmany = 1 plans in one embedding, the engine's unfused passes) over the 36 blocks of each pair's volume, measured on an
# MI355X (profiles/r09_motion_block_rescale.txt); the grid kernel may show twice that: its arithmetic differs in summation order only.
ONE_BLOCK_ERR = {
    "8x8x8-4x4x4":      6.428e-05,   # bound 1.286e-04; the grid kernel showed 7.7e-05
    "4x4x4-8x8x8":      1.151e-04,   # bound 2.302e-04; the grid kernel showed 1.37e-04
    "8x8x8-4x16x8":     1.025e-04,   # bound 2.050e-04; the grid kernel showed 1.07e-04
    "16x4x8-8x8x16":    8.876e-05,   # bound 1.775e-04; the grid kernel showed 1.02e-04
    "4x16x16-16x16x4":  9.866e-05,   # bound 1.973e-04; the grid kernel showed 9.5e-05
    "1x8x8-1x16x16":    7.322e-05,   # bound 1.464e-04; the grid kernel showed 6.4e-05
    "1x32x8-1x16x32":   6.914e-05,   # bound 1.383e-04; the grid kernel showed 6.4e-05
}


def torch_or_fail():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return torch


def grid_plans(block, scaled, trc=None):
    from dspfun_amd.engine import motion_grid_plans
    fwd, inv, info = motion_grid_plans(gr.shapes(block, scaled)[0], block, scaled)
    if trc:
        fwd.set_u8_trc(trc); inv.set_u8_trc(trc)
    return fwd, inv, info


def motion_scales(fwd, inv, rank, two_d):
    r2 = math.sqrt(2.0)
    unit = r2 if two_d else 1.0          # the unit axis of the reference's 3-D plans (engine.motion_grid_plans)
    fwd.set_scale(2 * r2 * unit); inv.set_scale(unit / (2 * r2))
    for a in range(rank):
        fwd.set_axis_scale0(a, 1.0, 1.0 / r2); inv.set_axis_scale0(a, r2, 1.0)
    return fwd, inv


def stack_plans(block, scaled):
    """the same blocks as block-major stacks: howmany = nb, idist = odist = the block's own volume"""
    from dspfun_amd import Plan, REDFT10, REDFT01
    nb = int(np.prod(gr.NBLOCKS))
    nf, ni = [v for v in block if v > 1], [v for v in scaled if v > 1]
    vf, vi = int(np.prod(block)), int(np.prod(scaled))
    fwd = Plan.many_r2r(nf, [REDFT10] * len(nf), howmany=nb, idist=vf, odist=vf)
    inv = Plan.many_r2r(ni, [REDFT01] * len(ni), howmany=nb, idist=vi, odist=vi)
    return motion_scales(fwd, inv, len(nf), block[0] == 1)


def one_block_plans(block, scaled):
    """the one-block device path: both plans inside one embedding, howmany = 1 (tests/test_motion_rescale.py)"""
    from dspfun_amd import Plan, REDFT10, REDFT01
    two_d = block[0] == 1
    cut = 1 if two_d else 0
    minbuf = [max(b, s) for b, s in zip(block, scaled)][cut:]
    fwd = Plan.many_r2r(list(block[cut:]), [REDFT10] * len(minbuf), inembed=minbuf, onembed=minbuf)
    inv = Plan.many_r2r(list(scaled[cut:]), [REDFT01] * len(minbuf), inembed=minbuf, onembed=minbuf)
    return motion_scales(fwd, inv, len(minbuf), two_d)


def run_grid_u8(torch, block, scaled, vol, flt=None, trc=None, coded=False):
    fwd, inv, info = grid_plans(block, scaled, trc)
    d_in = torch.from_numpy(np.array(vol)).to("cuda:0")
    d_out = torch.zeros(info["out_shape"], dtype=torch.uint8, device="cuda:0")
    d_coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    if flt is not None:
        flt = dict(flt, active=info["active"])
    fwd.roundtrip_u8(inv, d_in.data_ptr(), d_out.data_ptr(), None, info["out_mul"], filter=flt, d_coded=d_coded.data_ptr() if coded else 0)
    torch.cuda.synchronize()
    return (d_out.cpu().numpy(), int(d_coded.item())) if coded else d_out.cpu().numpy()


def run_grid_f32(torch, block, scaled, src, flt=None):
    """float in (a numpy array or a device tensor of the input volume) -> the float output volume as a device tensor"""
    fwd, inv, info = grid_plans(block, scaled)
    d_in = src if torch.is_tensor(src) else torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32)).to("cuda:0")
    d_out = torch.full(info["out_shape"], 7.0, dtype=torch.float32, device="cuda:0")
    if flt is not None:
        flt = dict(flt, active=info["active"])
    fwd.roundtrip(inv, d_in.data_ptr(), d_out.data_ptr(), filter=flt)
    torch.cuda.synchronize()
    return d_out


def base_filter(block, scaled, **kw):
    minbuf = [max(b, s) for b, s in zip(block, scaled)]
    active = [min(b, s) for b, s in zip(block, scaled)]
    f = dict(active=active, minbuf_hw=minbuf[1:], block_depth=minbuf[0], band_begin=(0, 0, 0), band_end=active)
    f.update(kw)
    return f


def run_one_block_path(torch, block, scaled, vol, flt=None, u8=True):
    """every block of the volume through the one-block device path; returns the output volume (8-bit, or float values)"""
    fwd, inv = one_block_plans(block, scaled)
    minbuf = tuple(max(b, s) for b, s in zip(block, scaled))
    sf, nm = mr.consts(block, scaled)
    blocks = gr.to_blocks(vol, block)
    out = np.zeros((len(blocks),) + tuple(scaled), dtype=np.uint8 if u8 else np.float32)
    bd, bh, bw = block
    sd, sh, sw = scaled
    for b, blk in enumerate(blocks):
        emb = np.zeros(minbuf, dtype=np.uint8 if u8 else np.float32)
        emb[:bd, :bh, :bw] = blk
        d = torch.from_numpy(emb).to("cuda:0")
        if u8:
            d_o = torch.zeros_like(d)
            work = torch.zeros(minbuf, dtype=torch.float32, device="cuda:0")
            fwd.roundtrip_u8(inv, d.data_ptr(), d_o.data_ptr(), work.data_ptr(), sf * nm * nm, filter=flt)
        else:
            d_o = d
            fwd.roundtrip(inv, d.data_ptr(), filter=flt)
        out[b] = d_o.cpu().numpy()[:sd, :sh, :sw]
    return gr.from_blocks(out, scaled)


@pytest.mark.parametrize("block,scaled", gr.PAIRS, ids=IDS)
def test_u8_grid_against_the_oracle(block, scaled):
    """at most 1 LSB anywhere and fewer than 0.5 % of the bytes differ (test_motion_rescale.py's caps for this comparison)"""
    torch = torch_or_fail()
    ref = gr.case(block, scaled)
    got = run_grid_u8(torch, block, scaled, ref["vol"])
    diff = np.abs(got.astype(int) - ref["out8"].astype(int))
    print(f"{gr.pair_id((block, scaled))}: max {diff.max()} LSB, {(diff > 0).mean():.5f} of the bytes differ")
    assert diff.max() <= 1 and (diff > 0).mean() < 0.005, (diff.max(), (diff > 0).mean())


@pytest.mark.parametrize("block,scaled", gr.PAIRS, ids=IDS)
def test_u8_grid_with_a_quantiser(block, scaled):
    """share below 2 % (test_motion_rescale.py's cap); the volume's seed keeps every coefficient / quantizer of the f64 oracle more than
    1e-4 from a rounding boundary, so no quantum can flip: d_coeffs_coded is then the oracle's count of non-zero quanta exactly"""
    torch = torch_or_fail()
    quant = 0.4
    ref = gr.case(block, scaled, quant)
    assert ref["edge"] > gr.EDGE
    flt = base_filter(block, scaled, quantizer=gr.quantizer_of(quant, scaled))
    got, coded = run_grid_u8(torch, block, scaled, ref["vol"], flt=flt, coded=True)
    diff = np.abs(got.astype(int) - ref["out8"].astype(int))
    print(f"{gr.pair_id((block, scaled))}: max {diff.max()} LSB, {(diff > 0).mean():.5f} differ, coded {coded} (oracle {ref['nonzero']}), edge {ref['edge']:.2e}, seed {ref['seed']}")
    assert diff.max() <= 1 and (diff > 0).mean() < 0.02, (diff.max(), (diff > 0).mean())
    assert coded == ref["nonzero"] > 0


@pytest.mark.parametrize("block,scaled", gr.PAIRS, ids=IDS)
def test_f32_grid_against_the_oracles_pixels(block, scaled):
    """float in and out, in pixels against the f64 oracle's pixels before rounding: at most twice ONE_BLOCK_ERR, what the one-block device
    path shows on the same blocks (the table above; measured values and bounds are also in profiles/r09_motion_block_rescale.txt)"""
    torch = torch_or_fail()
    ref = gr.case(block, scaled)
    sf, nm = mr.consts(block, scaled)
    got = run_grid_f32(torch, block, scaled, ref["vol"]).cpu().numpy().astype(np.float64) * (sf * nm * nm)
    err = float(np.abs(got - ref["pel"]).max())
    bound = 2 * ONE_BLOCK_ERR[gr.pair_id((block, scaled))]
    print(f"{gr.pair_id((block, scaled))}: max error {err:.3e} pixels, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("block,scaled", gr.PAIRS, ids=IDS)
def test_block_major_stack_gives_the_volume_layouts_bytes(block, scaled):
    torch = torch_or_fail()
    ref = gr.case(block, scaled, 0.4)
    flt = base_filter(block, scaled, quantizer=gr.quantizer_of(0.4, scaled))
    vol, cv = run_grid_u8(torch, block, scaled, ref["vol"], flt=flt, coded=True)
    fwd, inv = stack_plans(block, scaled)
    assert "block-major" in fwd.describe() and "block-major" in inv.describe()
    sf, nm = mr.consts(block, scaled)
    d_in = torch.from_numpy(gr.to_blocks(ref["vol"], block)).to("cuda:0")
    d_out = torch.zeros((d_in.shape[0],) + tuple(scaled), dtype=torch.uint8, device="cuda:0")
    d_coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    fwd.roundtrip_u8(inv, d_in.data_ptr(), d_out.data_ptr(), 0, sf * nm * nm, filter=flt, d_coded=d_coded.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(gr.from_blocks(d_out.cpu().numpy(), scaled), vol) and int(d_coded.item()) == cv > 0


def test_band_pass_in_both_layouts_and_against_the_one_block_path():
    torch = torch_or_fail()
    block, scaled = gr.PAIRS[2]
    ref = gr.case(block, scaled)
    active = [min(b, s) for b, s in zip(block, scaled)]
    flt = base_filter(block, scaled, band_begin=(0, 1, 0), band_end=(active[0], active[1], active[2] - 1), damp=0.5, boost=1.25, preserve_dc=1,
                      threshold_lo=2.0, threshold_hi=1e9)
    vol = run_grid_u8(torch, block, scaled, ref["vol"], flt=flt)
    plain = run_grid_u8(torch, block, scaled, ref["vol"])
    assert (vol != plain).mean() > 0.2                        # the filter acts
    fwd, inv = stack_plans(block, scaled)
    sf, nm = mr.consts(block, scaled)
    d_in = torch.from_numpy(gr.to_blocks(ref["vol"], block)).to("cuda:0")
    d_out = torch.zeros((d_in.shape[0],) + tuple(scaled), dtype=torch.uint8, device="cuda:0")
    fwd.roundtrip_u8(inv, d_in.data_ptr(), d_out.data_ptr(), None, sf * nm * nm, filter=flt)
    torch.cuda.synchronize()
    assert np.array_equal(gr.from_blocks(d_out.cpu().numpy(), scaled), vol)
    one = run_one_block_path(torch, block, scaled, ref["vol"], flt=flt)
    assert np.abs(one.astype(int) - vol.astype(int)).max() <= 1


def test_transfer_characteristic_is_the_composition_of_the_three_calls():
    """dspfft.h: with a function set the result equals dspfft_u8_to_f32_trc -> float roundtrip -> dspfft_f32_to_u8_trc byte for byte"""
    torch = torch_or_fail()
    from dspfun_amd.engine import u8_to_f32_trc, f32_to_u8_trc
    trc = "iec61966-2-1"
    for block, scaled in (gr.PAIRS[0], gr.PAIRS[5]):
        ref = gr.case(block, scaled)
        got = run_grid_u8(torch, block, scaled, ref["vol"], trc=trc)
        sf, nm = mr.consts(block, scaled)
        lin = u8_to_f32_trc(torch.from_numpy(np.array(ref["vol"])).to("cuda:0"), trc)
        mid = run_grid_f32(torch, block, scaled, lin)
        want = f32_to_u8_trc(mid, trc, mul=sf * nm * nm)
        torch.cuda.synchronize()
        assert np.array_equal(got, want.cpu().numpy())
        assert (got != run_grid_u8(torch, block, scaled, ref["vol"])).mean() > 0.2        # and it is not the plain call


@pytest.mark.parametrize("trc", [None, "iec61966-2-1"])
def test_dithered_call_is_the_float_grid_roundtrip_and_the_dither_launch(trc):
    torch = torch_or_fail()
    from dspfun_amd.engine import motion_dither_u8, u8_to_f32_trc
    block, scaled = gr.PAIRS[0]
    ref = gr.case(block, scaled)
    fwd, inv, info = grid_plans(block, scaled, trc)
    Do, Ho, Wo = info["out_shape"]
    sd, sh, sw = scaled
    d_in = torch.from_numpy(np.array(ref["vol"])).to("cuda:0")
    d_out = torch.zeros(info["out_shape"], dtype=torch.uint8, device="cuda:0")
    d_work = torch.full(info["out_shape"], 7.0, dtype=torch.float32, device="cuda:0")
    fwd.roundtrip_u8_dither(inv, d_in.data_ptr(), d_out.data_ptr(), d_work.data_ptr(), info["scalefactor"], info["normalization"])
    torch.cuda.synchronize()
    src = u8_to_f32_trc(d_in, trc) if trc else d_in.to(torch.float32)
    mid = run_grid_f32(torch, block, scaled, src)
    want = torch.zeros_like(d_out)
    motion_dither_u8(want.data_ptr(), mid.data_ptr(), scaled, row_pitch=Wo, plane_pitch=Ho * Wo, nblocks=info["nblocks"],
                     block_step=(sd * Ho * Wo, sh * Wo, sw), scalefactor=info["scalefactor"], normalization=info["normalization"], trc=trc or 0)
    torch.cuda.synchronize()
    assert torch.equal(d_work, mid)                           # the work buffer holds the undithered floats
    assert torch.equal(d_out, want) and int((d_out != 0).sum()) > 0
    with pytest.raises(Exception, match="null plan or buffer"):
        fwd.roundtrip_u8_dither(inv, d_in.data_ptr(), d_out.data_ptr(), None, info["scalefactor"], info["normalization"])


def test_block_equal_scaled_through_motion_grid_plans_is_todays_call():
    torch = torch_or_fail()
    from dspfun_amd import Plan, REDFT10, REDFT01
    from dspfun_amd.engine import motion_grid_plans
    block = (8, 8, 8)
    (D, H, W), _ = gr.shapes(block, block)
    vol = gr.case(block, (4, 4, 4))["vol"]
    fwd, inv, info = motion_grid_plans((D, H, W), block, block)
    assert info["out_shape"] == (D, H, W) and "side by side" in fwd.describe()
    dims = [(8, H * W, H * W), (8, W, W), (8, 1, 1)]
    how = [(D // 8, 8 * H * W, 8 * H * W), (H // 8, 8 * W, 8 * W), (W // 8, 8, 8)]
    fh = Plan.guru(dims, how, [REDFT10] * 3)
    ih = Plan.guru(dims, how, [REDFT01] * 3)
    motion_scales(fh, ih, 3, False)
    flt = base_filter(block, block, quantizer=gr.quantizer_of(0.4, block))
    outs = []
    for f, i in ((fwd, inv), (fh, ih)):
        d_in = torch.from_numpy(np.array(vol)).to("cuda:0")
        d_out = torch.zeros_like(d_in)
        work = torch.zeros((D, H, W), dtype=torch.float32, device="cuda:0")
        f.roundtrip_u8(i, d_in.data_ptr(), d_out.data_ptr(), work.data_ptr(), info["out_mul"], filter=flt)
        torch.cuda.synchronize()
        outs.append(d_out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and outs[0].any()
    # identity without a filter: out_mul = 1 / (8 * 512), the roundtrip's own normalisation
    d_in = torch.from_numpy(np.array(vol)).to("cuda:0")
    d_out = torch.zeros_like(d_in)
    work = torch.zeros((D, H, W), dtype=torch.float32, device="cuda:0")
    fwd.roundtrip_u8(inv, d_in.data_ptr(), d_out.data_ptr(), work.data_ptr(), info["out_mul"])
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), vol)


def test_a_coefficient_limit_in_range_raises_and_nothing_is_written():
    torch = torch_or_fail()
    from dspfun_amd import DspfftError
    block, scaled = gr.PAIRS[0]
    ref = gr.case(block, scaled)
    fwd, inv, info = grid_plans(block, scaled)
    d_in = torch.from_numpy(np.array(ref["vol"])).to("cuda:0")
    d_out = torch.full(info["out_shape"], 9, dtype=torch.uint8, device="cuda:0")
    d_of = torch.full(info["out_shape"], 7.0, dtype=torch.float32, device="cuda:0")
    with pytest.raises(DspfftError, match="coefficient limit"):
        fwd.roundtrip_u8(inv, d_in.data_ptr(), d_out.data_ptr(), d_of.data_ptr(), info["out_mul"], coeff_limit=100)
    with pytest.raises(DspfftError, match="coefficient limit"):
        fwd.roundtrip(inv, d_in.to(torch.float32).data_ptr(), d_of.data_ptr(), coeff_limit=511)
    torch.cuda.synchronize()
    assert bool((d_out == 9).all()) and bool((d_of == 7.0).all())
    # at the embedding's count nothing is dropped: the plain call
    fwd.roundtrip_u8(inv, d_in.data_ptr(), d_out.data_ptr(), None, info["out_mul"], coeff_limit=512)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), run_grid_u8(torch, block, scaled, ref["vol"]))
