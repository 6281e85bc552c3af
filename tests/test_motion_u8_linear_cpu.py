"""motion --linear on 8-bit pixels, the parts that need no device: trc_u8_core.h's two tables and its byte function (built with g++ by
tests/trc_u8_ref.py) against the reference's own load and store lines (tests/golden/ref_motion_u8_linear.npz) and against the exact
evaluation, and dspfft_plan_set_u8_trc on the test-only emulation library, which has no HIP kernels."""
import numpy as np
import pytest

import oracle_lib as ol
import trc_ref as tr
import trc_u8_ref as tu8
from dspfun_amd.engine import Plan

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def fx():
    return np.load(tu8.FIXTURE)


@pytest.mark.parametrize("trc", tr.IDS)
def test_decode_lut_is_the_references_load_bit_for_bit(fx, trc):
    assert np.array_equal(tu8.decode_lut(trc).view(np.uint32), fx[f"lut_{trc}"].view(np.uint32))


@pytest.mark.parametrize("trc", tr.IDS)
def test_thresholds_are_the_least_doubles_that_reach_their_byte(trc):
    thr = tu8.thresholds(trc)
    assert thr[0] == -np.inf and thr.shape == (256,)
    k = np.arange(1, 256)
    t = thr[1:]
    assert np.all(np.isfinite(t)) and np.all(np.diff(t) >= 0)
    assert np.all(tu8.exact_bytes(trc, t) >= k)
    assert np.all(tu8.exact_bytes(trc, np.nextafter(t, -np.inf)) < k)


@pytest.mark.parametrize("trc", tu8.STORE_TRCS)
def test_bytes_are_the_references_store_on_the_fixture_inputs(fx, trc):
    sf, nm = tu8.store_scales()
    for co, want in ((fx[f"store_{trc}_in"], fx[f"store_{trc}_out"]), (tu8.random_coeffs(), fx[f"store_{trc}_rand_out"])):
        pel = tu8.store_pel(co, sf, nm)
        for mode in (0, 1, 2):
            assert np.array_equal(tu8.bytes_of(trc, pel, mode), want), mode
    assert np.unique(np.concatenate([fx[f"store_{trc}_out"], fx[f"store_{trc}_rand_out"]])).size == 256


@pytest.mark.parametrize("trc", tr.IDS)
def test_bytes_are_the_exact_evaluation_on_the_sweep(trc):
    x = tr.sweep().astype(F64)
    pel = np.where(np.isfinite(x), x * 96.0 - np.sign(x) * 64.0 + 0.0, x)        # [2^-12, 4) and its negative -> about -64..320 and -320..64
    pel = np.concatenate([pel, x])
    want = tu8.exact_bytes(trc, pel)
    nan = np.isnan(pel)
    assert nan.any() and np.all(tu8.bytes_of(trc, pel, 0)[nan] == 0)
    for mode in (0, 1, 2):
        got = tu8.bytes_of(trc, pel, mode)
        assert np.array_equal(got[~nan], want[~nan]), mode
    # the single-precision seed is worth having: within one step of the byte nearly everywhere
    ok = ~nan
    assert np.mean(np.abs(tu8.seeds_of(trc, pel)[ok].astype(int) - want[ok].astype(int)) <= 1) > 0.999


def _stack(L, n, nb):
    vol = int(np.prod(n))
    nrm = 1.0 / np.prod([2.0 * v for v in n])
    fwd = Plan.many_r2r(n, [5] * len(n), howmany=nb, idist=vol, odist=vol, lib=L)
    inv = Plan.many_r2r(n, [4] * len(n), howmany=nb, idist=vol, odist=vol, first_axis_first=True, lib=L).set_scale(nrm)
    return fwd, inv


def test_set_u8_trc_on_the_emulation_library_refuses_a_function_and_resets():
    from emul_lib import emul
    L = emul()
    n, nb = [8, 8, 8], 4
    fwd, inv = _stack(L, n, nb)
    u8 = ol.synth_u8(0x8B1, nb * 512)

    def run():
        o8 = np.zeros_like(u8); work = np.zeros(nb * 512, dtype=F32)
        fwd.roundtrip_u8(inv, u8.ctypes.data, o8.ctypes.data, work.ctypes.data, 1.0)
        return o8

    before = run()
    for p in (fwd, inv):
        assert L.dspfft_plan_set_u8_trc(p._h, 13) == -3 and b"HIP-only" in L.dspfft_last_error()
        assert L.dspfft_plan_set_u8_trc(p._h, 0) == 0
    assert L.dspfft_plan_set_u8_trc(None, 0) == -1
    assert L.dspfft_plan_set_u8_trc(fwd._h, 16) == -1 and L.dspfft_plan_set_u8_trc(fwd._h, 2) == -1
    after = run()
    assert before.any() and np.array_equal(before, after)
