"""GPU (-m gpu): motion --spectrogram / --ispectrogram as one fused call -- dspfft_execute_spectrogram_* and dspfft_execute_ispectrogram_*
on small-block plans (one kernel, block_spec.hip) and on every other plan (the plan's passes and motion_ops.hip's kernel over all blocks), and
dspfft_motion_spec_blocks_* / dspfft_motion_ispec_blocks_* alone -- against the float64 reference block by block (tests/motion_spec_ref.py).

Acceptance.  8-bit: no byte differs from the reference by more than 1, and the share that differs is capped per mode at 1.5 times the share
of the composition a caller could write before these calls existed, plus 4 bytes: dspfft_execute on the same kind of plan, dspfft_motion_filter
per block and dspfft_motion_store_u8 with the host-computed c (per block for abs; the other way round for the inverse direction:
dspfft_motion_load_u8, the filter, dspfft_execute, dspfft_f32_to_u8).  Float pixels: max error over max|ref| at most twice the
composition's.  motion_spec_ref.composition is that code; tools/bench_motion_spec.py --accuracy runs it over the cases of this file and prints the
shares, which are the constants COMPOSITION_* (profiles/r11_motion_spec.txt has the table and the commit)."""
import numpy as np
import pytest

import motion_grid_ref as gr
import motion_spec_ref as sr
from motion_spec_ref import dev, fused, composition, share_of, float_err, cases_of
from test_ref_motion import FIX, IO_GEOMS, ISPEC_MODES, SPEC_MODES, io_consts, check_load, check_store

pytestmark = pytest.mark.gpu

# share of bytes that differ from the reference (worst case over the cases of one mode) and max error / max|ref| of the float-pixel cases, of
# the COMPOSITION, per path and direction: tools/bench_motion_spec.py --accuracy on the kernels of commit 0b00809, the parent of the commit
# that added this file, which leaves them as they were (profiles/r11_motion_spec.txt)
COMPOSITION_SHARE = {
    ("blocks", "spec"): {"abs": 0.0, "shift": 5.425e-5, "flat": 2.40385e-3, "copy": 1.20192e-3},
    ("blocks", "ispec"): {"shift": 9.766e-5, "flat": 1.5319e-4, "copy": 1.5319e-4},
    ("passes", "spec"): {"abs": 2.6042e-4, "shift": 8.36e-6, "flat": 0.0, "copy": 0.0},
    ("passes", "ispec"): {"shift": 3.4722e-4, "flat": 2.6042e-4, "copy": 0.0},
}
COMPOSITION_FLOAT = {("blocks", "spec"): 1.281e-5, ("blocks", "ispec"): 3.311e-7, ("passes", "spec"): 1.270e-4, ("passes", "ispec"): 5.452e-7}
EXTRA_BYTES = 4

PASSES = sr.PASSES


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from dspfun_amd import _lib
    return torch, _lib.load()


def accept_bytes(got, ref, key, mode, what):
    sr.check_tie_share(ref, key[1] == "ispec")
    mx, n, size = share_of(got, ref["out8"], ref["tie"])
    cap = 1.5 * COMPOSITION_SHARE[key][mode] * size + EXTRA_BYTES
    print(f"{what}: max diff {mx}, {n} of {size} bytes differ ({n / size:.5%}), cap {cap:.1f} bytes")
    assert mx <= 1 and n <= cap, (what, mx, n, size, cap)


def accept_float(got, ref, key, what):
    err = float_err(got, ref["pel"], ref["tie"])
    print(f"{what}: max err / max|ref| {err:.3e}, cap {2 * COMPOSITION_FLOAT[key]:.3e}")
    assert err <= 2 * COMPOSITION_FLOAT[key], (what, err)


def report_coded(what, coded, ref, block):
    """the device's count (block_coded_add, motion_ops.hip's coded_add) equals the reference's to within the coefficients on a quantiser tie"""
    slack = sr.coded_slack(ref, block)
    print(f"{what}: coded {coded}, reference {ref['coded']}, difference {coded - ref['coded']}; on a quantiser tie: {slack} coefficients")
    assert coded > 0 and abs(coded - ref["coded"]) <= slack, (what, coded, ref["coded"], slack)


@pytest.mark.parametrize("shape", sr.SHAPES, ids=[sr.shape_id(s) for s in sr.SHAPES])
@pytest.mark.parametrize("inverse,mode", [(False, m) for m in sr.SPEC_MODES] + [(True, m) for m in sr.ISPEC_MODES], ids=lambda v: {False: "spec", True: "ispec"}.get(v, v))
def test_small_blocks_one_kernel(gpu, shape, inverse, mode):
    torch, L = gpu
    block, vol_shape = shape
    kind_of = sr.ol.REDFT01 if inverse else sr.ol.REDFT10
    plan = sr.volume_plan(block, vol_shape, kind_of)
    key = ("blocks", "ispec" if inverse else "spec")
    name = f"{key[1]} {mode} {sr.shape_id(shape)}"
    for kind, fl, ref, pix in cases_of(inverse, block, vol_shape, mode):
        got, coded = fused(torch, plan, inverse, pix, block, mode, ref["filt"])          # d_work = NULL
        if fl:
            accept_float(got, ref, key, f"{name} f32")
        else:
            accept_bytes(got, ref, key, mode, f"{name} filter={kind}")
        if kind in ("full", "q"):
            report_coded(f"{name} filter={kind}", coded, ref, block)
        else:
            assert coded == 0
        if sr.SHAPES.index(shape) in sr.BLOCK_MAJOR:
            nb = int(np.prod(sr.nblocks_of(block, vol_shape)))
            gotb, codedb = fused(torch, sr.stack_plan(block, nb, kind_of), inverse, gr.to_blocks(pix, block), block, mode, ref["filt"])
            assert np.array_equal(gr.from_blocks(gotb, block, sr.nblocks_of(block, vol_shape)), got) and codedb == coded
    if shape == sr.SHAPES[1]:
        kind, fl, ref, pix = next(cases_of(inverse, block, vol_shape, mode))
        same, _ = fused(torch, plan, inverse, pix, block, mode, in_place=True)
        assert np.array_equal(same, fused(torch, plan, inverse, pix, block, mode)[0])


@pytest.mark.parametrize("geom", PASSES, ids=["3x540x960", "3x24x40", "one-4x24x40"])
@pytest.mark.parametrize("inverse", [False, True], ids=["spec", "ispec"])
def test_every_other_plan_runs_its_passes_and_one_kernel_over_all_blocks(gpu, geom, inverse):
    torch, L = gpu
    block, nb = geom
    vol_shape = (nb * block[0], block[1], block[2])
    kind_of = sr.ol.REDFT01 if inverse else sr.ol.REDFT10
    plan = sr.stack_plan(block, nb, kind_of)
    text = plan.describe()
    assert "BLOCK" not in text and (("ROW*" in text and "COL*" in text) == (block[1:] == (540, 960)))
    key = ("passes", "ispec" if inverse else "spec")
    big = block[1] == 540
    for mode in (sr.ISPEC_MODES if inverse else sr.SPEC_MODES):
        name = f"{key[1]} {mode} {'x'.join(map(str, vol_shape))}"
        for kind, fl, ref, pix in cases_of(inverse, block, vol_shape, mode):
            if big and mode in ("flat", "copy") and kind:
                continue                 # (the large frames: every type, and every filter on abs and shift; flat and copy take the filters on the small ones)
            got, coded = fused(torch, plan, inverse, pix, block, mode, ref["filt"], with_work=True)
            if fl:
                accept_float(got, ref, key, f"{name} f32")
            else:
                accept_bytes(got, ref, key, mode, f"{name} filter={kind}")
            if kind in ("full", "q"):
                report_coded(f"{name} filter={kind}", coded, ref, block)


@pytest.mark.parametrize("g", range(len(IO_GEOMS)))
@pytest.mark.parametrize("px", ["u8", "f32"])
def test_blocks_kernels_alone_are_the_references_lines(gpu, g, px):
    """dspfft_motion_spec_blocks_* / _ispec_blocks_* with nblocks = 1 on the reference's own compiled lines (tests/golden/ref_motion.npz):
    check_store and check_load of tests/test_ref_motion.py unchanged.  abs: sp.c is the fixture's own c_abs, which the kernel does not read --
    it derives the same number from the fixture's element 0."""
    from dspfun_amd.engine import motion_spec_blocks, motion_ispec_blocks
    torch, L = gpu
    d, h, w, md, mh, mw = IO_GEOMS[g]
    sf, norm, cc, ic = io_consts(g)
    co = dev(torch, FIX[f"io{g}_coeffs"].copy())
    for name in SPEC_MODES:
        out = torch.zeros(md * mh * mw, dtype=torch.float32 if px == "f32" else torch.uint8, device="cuda:0")
        before = co.clone()
        motion_spec_blocks(out, co, (d, h, w), name, sf, norm, cc.get(name, 0.0), minbuf_hw=(mh, mw), pixels=px)
        torch.cuda.synchronize()
        check_store(out.cpu().numpy(), g, name, px)
        assert torch.equal(co, before)              # read only
    pix = dev(torch, FIX[f"io{g}_pix_{px}"].copy())
    for name in ISPEC_MODES:
        c = torch.zeros(md * mh * mw, dtype=torch.float32, device="cuda:0")
        motion_ispec_blocks(c, pix, (d, h, w), name, sf, norm, ic, minbuf_hw=(mh, mw), pixels=px)
        torch.cuda.synchronize()
        check_load(c.cpu().numpy(), g, name, px)


def test_a_plan_with_a_transfer_characteristic_is_refused_and_nothing_is_written(gpu):
    torch, L = gpu
    from dspfun_amd.engine import DspfftError
    block, vol_shape = sr.SHAPES[1]
    sf, nm, c = sr.constants(block)
    pix = dev(torch, sr.volume(block, vol_shape))
    for inverse in (False, True):
        plan = sr.volume_plan(block, vol_shape, sr.ol.REDFT01 if inverse else sr.ol.REDFT10).set_u8_trc("iec61966-2-1")
        out = torch.full_like(pix, 9)
        with pytest.raises(DspfftError, match="transfer characteristic"):
            (plan.ispectrogram if inverse else plan.spectrogram)(pix.data_ptr(), out.data_ptr(), "shift", sf, nm, c)
        torch.cuda.synchronize()
        assert bool((out == 9).all())


@pytest.mark.parametrize("mode", ["abs", "shift"])
def test_the_single_precision_encode_on_the_device_gives_the_double_kernels_bytes(gpu, mode):
    """dspfft_motion_spec_blocks_u8 (motion_spec_byte: single precision where it decides) against dspfft_motion_store_u8 (the double line
    alone) on 2^22 coefficients spaced evenly in log|pel| over [1e-6, 1e6], both signs, for three constants: equal bytes.  Under abs the
    blocks call takes its constant from element 0, which is set so that c comes out as asked."""
    from dspfun_amd.engine import motion_spec_blocks
    import ctypes as C
    torch, L = gpu
    sf, nm, _ = sr.constants((8, 8, 8))
    n = 1 << 21
    pel = np.exp(np.linspace(np.log(1e-6), np.log(1e6), n))
    for c in (8.0, 25.0, 60.0):
        v = np.concatenate([pel / (sf * nm), -pel / (sf * nm)]).astype(np.float32)
        cc = c
        if mode == "abs":
            v[0] = np.float32(np.expm1(255.0 / c) / (sf * nm))
            cc = 255.0 / np.log1p(abs(float(v[0]) * sf * nm))                # what both calls use
        co = dev(torch, v)
        fast, exact = (torch.zeros(v.size, dtype=torch.uint8, device="cuda:0") for _ in range(2))
        motion_spec_blocks(fast, co, (1, 1, v.size), mode, sf, nm, cc)
        assert L.dspfft_motion_store_u8(exact.data_ptr(), co.data_ptr(), (C.c_int * 3)(1, 1, v.size), (C.c_int * 2)(1, v.size), sr_mode(mode), sf, nm, cc, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(fast, exact), (mode, c, int((fast != exact).sum()))
        assert len(torch.unique(exact)) > 100


def sr_mode(mode):
    return {"abs": 1, "shift": 2}[mode]
