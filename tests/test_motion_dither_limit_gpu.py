"""motion --coeff-limit with -d on the device: dspfft_execute_roundtrip_u8_dither_limit must equal, byte for byte, the float-output limit
call into a work buffer followed by engine.motion_dither_u8 over that buffer -- on every kind of pair the dithered call takes: the fused
small-block kernel, the unfused passes with the stand-alone selection, and a rescaled block grid (block_rescale_topn.hip)."""
import math

import numpy as np
import pytest

import motion_grid_topn_ref as tr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
R2 = math.sqrt(2.0)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from dspfun_amd import _lib
    _lib.load()
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def motion_scales(fwd, inv, n):
    """motion's uniform range (motion.c:644-647, :748-751) as the plans' scales, and the transforms' 1 / prod(2 n) on the inverse: values are pixels"""
    fwd.set_scale(2 * R2)
    inv.set_scale(1.0 / (2 * R2) / float(np.prod([2.0 * v for v in n])))
    for a in range(len(n)):
        fwd.set_axis_scale0(a, 1.0, 1.0 / R2)
        inv.set_axis_scale0(a, R2, 1.0)
    return fwd, inv


def volume_plans(block, D, H, W):
    from dspfun_amd import Plan
    bd, bh, bw = block
    dims = [(bd, H * W, H * W), (bh, W, W), (bw, 1, 1)]
    how = [(D // bd, bd * H * W, bd * H * W), (H // bh, bh * W, bh * W), (W // bw, bw, bw)]
    fwd, inv = motion_scales(Plan.guru(dims, how, [5] * 3), Plan.guru(dims, how, [4] * 3), list(block))
    assert "side by side" in fwd.describe() and "BLOCK" in inv.describe()
    return fwd, inv


def dithered(gpu, fwd, inv, pix, out_shape, sf, nm, keep, outside_mul=1.0, flt=None):
    din = dev(gpu, pix)
    dout = gpu.full(out_shape, 7, dtype=gpu.uint8, device="cuda:0")
    work = gpu.full(out_shape, 7.0, dtype=gpu.float32, device="cuda:0")
    fwd.roundtrip_u8_dither(inv, din.data_ptr(), dout.data_ptr(), work.data_ptr(), sf, nm, filter=flt, coeff_limit=keep, outside_mul=outside_mul)
    gpu.cuda.synchronize()
    return dout, work


@pytest.mark.parametrize("trc,on_fwd", [(0, False), (13, False), (13, True)], ids=["plain", "trc-on-inv", "trc-on-both"])
def test_blocks_of_a_volume_through_the_fused_block_kernel(gpu, trc, on_fwd):
    """8 x 8 x 8 blocks of a 16 x 16 x 40 volume; trc: a transfer characteristic on the inverse plan, which the dithered store then encodes
    with, and (motion --linear sets both) on the forward plan too, whose 8-bit load then decodes"""
    from dspfun_amd import engine
    block, (D, H, W), keep = (8, 8, 8), (16, 16, 40), 24
    pix = ol.synth_u8(0xD17A, D * H * W).reshape(D, H, W)
    flt = dict(active=block, minbuf_hw=(8, 8), block_depth=8, band_begin=(0, 0, 0), band_end=block, quantizer=3.0)
    fwd, inv = volume_plans(block, D, H, W)
    f = engine.u8_to_f32_trc(dev(gpu, pix), trc) if on_fwd else dev(gpu, pix.astype(np.float32))
    mid = gpu.full(pix.shape, 7.0, dtype=gpu.float32, device="cuda:0")
    fwd.roundtrip_limit(inv, f.data_ptr(), mid.data_ptr(), coeff_limit=keep, filter=flt)
    plain = gpu.zeros_like(mid)
    fwd.roundtrip(inv, f.data_ptr(), plain.data_ptr(), filter=flt)
    want = gpu.zeros(pix.shape, dtype=gpu.uint8, device="cuda:0")
    engine.motion_dither_u8(want.data_ptr(), mid.data_ptr(), block, row_pitch=W, plane_pitch=H * W, nblocks=(D // 8, H // 8, W // 8),
                            block_step=(8 * H * W, 8 * W, 8), scalefactor=1.0, normalization=1.0, trc=trc)
    if trc:
        inv.set_u8_trc(trc)
    if on_fwd:
        fwd.set_u8_trc(trc)
    got, work = dithered(gpu, fwd, inv, pix, pix.shape, 1.0, 1.0, keep, flt=flt)
    assert gpu.equal(work, mid) and not gpu.equal(mid, plain)          # the work buffer holds the undithered floats, and the limit acted
    assert gpu.equal(got, want) and np.unique(got.cpu().numpy()).size > 20


def test_a_clip_of_per_frame_blocks_through_the_unfused_passes(gpu):
    """3 frames of 72 x 96 (6912 coefficients each, too long for LDS), keep = 300: forward passes, dspfft_motion_topn_blocks, inverse passes;
    the clip is not walked in slices when a limit is set"""
    from dspfun_amd import Plan, engine
    frames, h, w, keep = 3, 72, 96, 300
    pix = ol.synth_u8(0xD17B, frames * h * w).reshape(frames, h, w)
    fwd, inv = motion_scales(Plan.many_r2r([h, w], [5, 5], howmany=frames, idist=h * w, odist=h * w),
                             Plan.many_r2r([h, w], [4, 4], howmany=frames, idist=h * w, odist=h * w, first_axis_first=True), [h, w])
    mid = dev(gpu, pix.astype(np.float32))
    fwd.roundtrip_limit(inv, mid.data_ptr(), coeff_limit=keep)
    plain = dev(gpu, pix.astype(np.float32))
    fwd.roundtrip(inv, plain.data_ptr())
    want = gpu.zeros(pix.shape, dtype=gpu.uint8, device="cuda:0")
    engine.motion_dither_u8(want.data_ptr(), mid.data_ptr(), (1, h, w), nblocks=(frames, 1, 1), block_step=(h * w, 0, 0), scalefactor=1.0, normalization=1.0)
    got, work = dithered(gpu, fwd, inv, pix, pix.shape, 1.0, 1.0, keep)
    assert "in slices" not in fwd.describe()
    assert gpu.equal(work, mid) and not gpu.equal(mid, plain)
    assert gpu.equal(got, want) and np.unique(got.cpu().numpy()).size > 20
    # the _topn entries' work-buffer check, ahead of any launch
    import ctypes as C
    from dspfun_amd import _lib
    L = _lib.load()
    assert L.dspfft_roundtrip_topn_work_bytes(fwd._h, inv._h) > 0
    cl = _lib.CoeffLimit()
    cl.keep = keep; cl.outside_mul = 1.0
    dout = gpu.full(pix.shape, 7, dtype=gpu.uint8, device="cuda:0")
    rc = L.dspfft_execute_roundtrip_u8_dither_limit(fwd._h, inv._h, dev(gpu, pix).data_ptr(), dout.data_ptr(), work.data_ptr(), 1.0, 1.0, None, C.byref(cl), None, None)
    gpu.cuda.synchronize()
    assert rc == -1 and b"work buffer too small" in L.dspfft_last_error() and bool((dout == 7).all()) and gpu.equal(work, mid)


def test_a_rescaled_block_grid(gpu, monkeypatch):
    """(8, 8, 8) -> (4, 4, 4) over the 2 x 2 x 7 grid of tests/motion_grid_topn_ref.py: the new kernel stores floats into the work buffer"""
    from dspfun_amd.engine import motion_grid_plans, motion_dither_u8
    block, scaled = tr.PAIRS[0]
    ref = tr.case(block, scaled)
    keep = ref["keep"]
    monkeypatch.setenv("DSPFFT_BLOCK_G", str(ref["G"]))
    fwd, inv, info = motion_grid_plans(ref["vol"].shape, block, scaled)
    Do, Ho, Wo = info["out_shape"]
    sd, sh, sw = scaled
    f = dev(gpu, np.array(ref["vol"], dtype=np.float32))
    mid = gpu.full(info["out_shape"], 7.0, dtype=gpu.float32, device="cuda:0")
    fwd.roundtrip_limit(inv, f.data_ptr(), mid.data_ptr(), coeff_limit=keep, outside_mul=info["limit_outside_mul"])
    plain = gpu.zeros_like(mid)
    fwd.roundtrip(inv, f.data_ptr(), plain.data_ptr())
    want = gpu.zeros(info["out_shape"], dtype=gpu.uint8, device="cuda:0")
    motion_dither_u8(want.data_ptr(), mid.data_ptr(), scaled, row_pitch=Wo, plane_pitch=Ho * Wo, nblocks=info["nblocks"],
                     block_step=(sd * Ho * Wo, sh * Wo, sw), scalefactor=info["scalefactor"], normalization=info["normalization"])
    got, work = dithered(gpu, fwd, inv, np.array(ref["vol"]), info["out_shape"], info["scalefactor"], info["normalization"], keep, info["limit_outside_mul"])
    assert gpu.equal(work, mid) and not gpu.equal(mid, plain)
    assert gpu.equal(got, want) and int((got != 0).sum()) > 0
    # keep = 0 is the entry without a limit
    got0, work0 = dithered(gpu, fwd, inv, np.array(ref["vol"]), info["out_shape"], info["scalefactor"], info["normalization"], 0)
    assert gpu.equal(work0, plain)
