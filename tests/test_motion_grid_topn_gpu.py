"""motion --coeff-limit on a rescaled block grid on the device (block_rescale_topn.hip through dspfft_execute_roundtrip*_limit): every block
of a 2 x 2 x 7 grid in ONE launch, against the f64 restatement of the reference block by block (tests/motion_grid_topn_ref.py).  The
volumes' blocks hold strong coefficients outside min(block, scaled) that the reference ranks by their RAW value: a selection over scaled
values everywhere keeps another set (asserted on the CPU, per block), so the comparisons below see the rule."""
import numpy as np
import pytest

import motion_grid_topn_ref as tr
import motion_ref as mr

pytestmark = pytest.mark.gpu
IDS = [tr.pair_id(p) for p in tr.PAIRS]

# Float ends, in pixels against the f64 oracle's pixels before rounding: the bound test_motion_block_rescale_gpu.py holds the plain grid call
# to, twice its ONE_BLOCK_ERR, for the pairs that table lists.  The other pairs run the same float arithmetic -- at most six passes of
# tiny_dct over lines of at most 32 points on pixel values up to 255 -- and get 16 half-ulps of 255 in single precision, 16 x 255 x 2^-24 =
# 2.43e-04: the table's bounds are 8.5 ... 15.1 of these units (1.286e-04 ... 2.302e-04), the largest for the longest chains of passes.
HALF_ULP_255 = 255.0 * 2.0 ** -24


def float_bound(pair):
    from test_motion_block_rescale_gpu import ONE_BLOCK_ERR
    one = ONE_BLOCK_ERR.get(tr.pair_id(pair))
    return 2 * one if one is not None else 16 * HALF_ULP_255


def torch_or_fail():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return torch


def grid_plans(monkeypatch, block, scaled, trc=None):
    """the plan pair with the case's blocks per workgroup forced (read when the plans are made): two workgroups and more along x, the last short"""
    from dspfun_amd.engine import motion_grid_plans
    monkeypatch.setenv("DSPFFT_BLOCK_G", str(tr.FORCED_G[(block, scaled)]))
    in_shape = tuple(n * b for n, b in zip(tr.NBLOCKS, block))
    assert tr.NBLOCKS[2] % tr.FORCED_G[(block, scaled)] and in_shape[2] % 4 == 0
    fwd, inv, info = motion_grid_plans(in_shape, block, scaled)
    if trc:
        fwd.set_u8_trc(trc); inv.set_u8_trc(trc)
    return fwd, inv, info


def run_u8(torch, plans, vol, keep=0, flt=None):
    fwd, inv, info = plans
    d_in = torch.from_numpy(np.array(vol)).to("cuda:0")
    d_out = torch.zeros(info["out_shape"], dtype=torch.uint8, device="cuda:0")
    if keep:
        fwd.roundtrip_u8_limit(inv, d_in.data_ptr(), d_out.data_ptr(), None, info["out_mul"], coeff_limit=keep, outside_mul=info["limit_outside_mul"], filter=flt)
    else:
        fwd.roundtrip_u8(inv, d_in.data_ptr(), d_out.data_ptr(), None, info["out_mul"], filter=flt)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def run_f32(torch, plans, src, keep, flt=None):
    """float in (a numpy array or a device tensor of the input volume) -> the float output volume as a device tensor"""
    fwd, inv, info = plans
    d_in = src if torch.is_tensor(src) else torch.from_numpy(np.array(src, dtype=np.float32)).to("cuda:0")
    d_out = torch.full(info["out_shape"], 7.0, dtype=torch.float32, device="cuda:0")
    fwd.roundtrip_limit(inv, d_in.data_ptr(), d_out.data_ptr(), coeff_limit=keep, outside_mul=info["limit_outside_mul"], filter=flt)
    torch.cuda.synchronize()
    return d_out


def assert_rule_visible(ref, block, scaled):
    assert ref["gap"] > tr.GAP, ref["gap"]
    if any(b > s for b, s in zip(block, scaled)):
        assert ref["differs"] is True
    else:
        assert ref["differs"] is None


@pytest.mark.parametrize("block,scaled", tr.PAIRS, ids=IDS)
def test_u8_grid_with_a_limit_against_the_oracle(block, scaled, monkeypatch):
    """at most 1 LSB on under 2 % of the samples (test_topn_roundtrip_against_the_f64_reference's bar for this comparison)"""
    torch = torch_or_fail()
    ref = tr.case(block, scaled)
    assert_rule_visible(ref, block, scaled)
    assert ref["dc_kept"]
    plans = grid_plans(monkeypatch, block, scaled)
    got = run_u8(torch, plans, ref["vol"], ref["keep"])
    diff = np.abs(got.astype(int) - ref["out8"].astype(int))
    import motion_grid_ref as gr
    pdiff = np.abs(run_u8(torch, plans, ref["vol"]).astype(int) - gr.oracle(ref["vol"], block, scaled)[0].astype(int))
    print(f"{tr.pair_id((block, scaled))}: keep {ref['keep']}, gap {ref['gap']:.2e}, max {diff.max()} LSB, {(diff > 0).mean():.5f} of the bytes differ "
          f"(the plain grid call, no limit, against its own oracle on the same volume: {(pdiff > 0).mean():.5f})")
    assert diff.max() <= 1 and (diff > 0).mean() < 0.02, (diff.max(), (diff > 0).mean())


@pytest.mark.parametrize("block,scaled", tr.PAIRS, ids=IDS)
def test_f32_grid_with_a_limit_against_the_oracles_pixels(block, scaled, monkeypatch):
    torch = torch_or_fail()
    ref = tr.case(block, scaled, u8=False)
    assert_rule_visible(ref, block, scaled)
    sf, nm = mr.consts(block, scaled)
    got = run_f32(torch, grid_plans(monkeypatch, block, scaled), ref["vol"], ref["keep"]).cpu().numpy().astype(np.float64) * (sf * nm * nm)
    err = float(np.abs(got - ref["pel"]).max())
    bound = float_bound((block, scaled))
    print(f"{tr.pair_id((block, scaled))}: keep {ref['keep']}, max error {err:.3e} pixels, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("block,scaled", [tr.PAIRS[0], tr.PAIRS[4]], ids=[IDS[0], IDS[4]])
def test_the_restored_dc_is_the_one_from_before_the_selection(block, scaled, monkeypatch):
    """float ends, zero-mean blocks moved to a mean of 0.02, boost = 2 with preserve_dc = dc: the DC is not among the kept coefficients and
    still comes back at its value from BEFORE the selection (motion.c:650, :734).  Restoring what the selection left -- zero -- would miss
    by 0.02 of a pixel on every sample, a hundred times the bound."""
    torch = torch_or_fail()
    ref = tr.case(block, scaled, u8=False, mean=0.02, boost_dc=True)
    assert ref["gap"] > tr.GAP and not ref["dc_kept"] and np.all(np.abs(ref["dc_before"]) > 0)
    active = [min(b, s) for b, s in zip(block, scaled)]
    minbuf = [max(b, s) for b, s in zip(block, scaled)]
    flt = dict(active=active, minbuf_hw=minbuf[1:], block_depth=minbuf[0], band_begin=(0, 0, 0), band_end=active, boost=2.0, preserve_dc=1)
    sf, nm = mr.consts(block, scaled)
    got = run_f32(torch, grid_plans(monkeypatch, block, scaled), ref["vol"], ref["keep"], flt=flt).cpu().numpy().astype(np.float64) * (sf * nm * nm)
    err = float(np.abs(got - ref["pel"]).max())
    bound = float_bound((block, scaled))
    print(f"{tr.pair_id((block, scaled))}: max error {err:.3e} pixels, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("block,scaled", [tr.PAIRS[0], tr.PAIRS[5]], ids=[IDS[0], IDS[5]])
def test_keep_at_the_embeddings_count_is_the_plain_grid_call(block, scaled, monkeypatch):
    torch = torch_or_fail()
    ref = tr.case(block, scaled)
    plans = grid_plans(monkeypatch, block, scaled)
    E = int(np.prod([max(b, s) for b, s in zip(block, scaled)]))
    plain = run_u8(torch, plans, ref["vol"])
    assert np.array_equal(run_u8(torch, plans, ref["vol"], E), plain) and np.array_equal(run_u8(torch, plans, ref["vol"], E + 1), plain)
    assert not np.array_equal(run_u8(torch, plans, ref["vol"], E - 1), run_u8(torch, plans, ref["vol"], 1))       # (and below it the limit acts)
    x = np.array(ref["vol"], dtype=np.float32)
    fwd, inv, info = plans
    d_in = torch.from_numpy(x).to("cuda:0")
    d_plain = torch.zeros(info["out_shape"], dtype=torch.float32, device="cuda:0")
    fwd.roundtrip(inv, d_in.data_ptr(), d_plain.data_ptr())
    assert torch.equal(run_f32(torch, plans, d_in, E), d_plain)


@pytest.mark.parametrize("block,scaled", [tr.PAIRS[0], tr.PAIRS[5]], ids=[IDS[0], IDS[5]])
def test_transfer_characteristic_is_the_composition_of_the_three_calls(block, scaled, monkeypatch):
    """dspfft.h: with a function set on both plans the 8-bit result equals dspfft_u8_to_f32_trc -> the float-ends limit call ->
    dspfft_f32_to_u8_trc, byte for byte"""
    torch = torch_or_fail()
    from dspfun_amd.engine import u8_to_f32_trc, f32_to_u8_trc
    trc = "iec61966-2-1"
    ref = tr.case(block, scaled)
    keep = ref["keep"]
    got = run_u8(torch, grid_plans(monkeypatch, block, scaled, trc), ref["vol"], keep)
    sf, nm = mr.consts(block, scaled)
    plans = grid_plans(monkeypatch, block, scaled)
    lin = u8_to_f32_trc(torch.from_numpy(np.array(ref["vol"])).to("cuda:0"), trc)
    mid = run_f32(torch, plans, lin, keep)
    want = f32_to_u8_trc(mid, trc, mul=sf * nm * nm)
    torch.cuda.synchronize()
    assert np.array_equal(got, want.cpu().numpy())
    assert (got != run_u8(torch, plans, ref["vol"], keep)).any()               # and it is not the call without the function
