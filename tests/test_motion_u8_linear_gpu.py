"""GPU (-m gpu): motion --linear on 8-bit video.  The stand-alone kernels (load, store, dithered store, the flat pair) against the reference's own
lines (tests/golden/ref_motion_u8_linear.npz) and against trc_u8_core.h's exact evaluation on the host; every path of the 8-bit roundtrip
with dspfft_plan_set_u8_trc against the composition dspfft_u8_to_f32_trc -> float roundtrip -> dspfft_f32_to_u8_trc, byte for byte (the bar
tests/test_kernel_logic_cpu.py::test_roundtrip_u8_matches_float_path holds the plain path to); the reset; the refusals."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import trc_ref as tr
import trc_u8_ref as tu8

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F32, F64 = np.float32, np.float64
R2 = math.sqrt(2.0)
MUL = 0.9371          # (no simple fraction: see tests/test_motion_topn_gpu.py MUL8)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from dspfun_amd import _lib
    _lib.load()
    return torch


@pytest.fixture(scope="module")
def fx():
    return np.load(tu8.FIXTURE)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def block_index():
    (d, h, w), (md, mh, mw) = tr.MOTION_BLOCK, tr.MOTION_MINBUF
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    return ((z * mh + y) * mw + x).ravel()


# ---- the stand-alone kernels against the fixtures ----
@pytest.mark.parametrize("trc", tr.IDS)
def test_load_kernel_is_the_references_load_bit_for_bit(gpu, fx, trc):
    from dspfun_amd import engine
    idx, n = block_index(), int(np.prod(tr.MOTION_MINBUF))
    pix = np.full(n, 200, dtype=np.uint8)
    pix[idx] = np.arange(idx.size) % 256
    want = np.full(n, F32(-77.0))
    want[idx] = fx[f"lut_{trc}"][pix[idx]]
    d_pix, d_co = dev(gpu, pix), dev(gpu, np.full(n, F32(-77.0)))
    assert engine.motion_load_u8_linear(d_co, d_pix, tr.MOTION_BLOCK, tr.MOTION_MINBUF[1:], trc=trc) == 0
    gpu.cuda.synchronize()
    assert np.array_equal(d_co.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("trc", tu8.STORE_TRCS)
def test_store_kernel_is_the_references_store_byte_for_byte(gpu, fx, trc):
    from dspfun_amd import engine
    idx, n = block_index(), int(np.prod(tr.MOTION_MINBUF))
    sf, nm = tu8.store_scales()
    co = np.concatenate([fx[f"store_{trc}_in"], tu8.random_coeffs()])
    want = np.concatenate([fx[f"store_{trc}_out"], fx[f"store_{trc}_rand_out"]])
    nchunks = -(-co.size // idx.size)
    cbuf = np.zeros((nchunks, n), dtype=F32)
    used = np.zeros((nchunks, n), dtype=bool)
    for k in range(nchunks):
        part = co[k * idx.size:(k + 1) * idx.size]
        cbuf[k, idx[:part.size]] = part
        used[k, idx[:part.size]] = True
    d_co, d_pix = dev(gpu, cbuf), dev(gpu, np.full((nchunks, n), 99, dtype=np.uint8))
    for k in range(nchunks):
        assert engine.motion_store_u8_linear(d_pix[k], d_co[k], tr.MOTION_BLOCK, tr.MOTION_MINBUF[1:], sf, nm, trc=trc) == 0
    gpu.cuda.synchronize()
    got = d_pix.cpu().numpy()
    inside = np.zeros((nchunks, n), dtype=bool)
    inside[:, idx] = True
    assert np.all(got[~inside] == 99)
    assert np.array_equal(got[used], want)


@pytest.mark.parametrize("name", [c[0] for c in tu8.DITHER_CASES])
@pytest.mark.parametrize("trc", tu8.DITHER_TRCS)
def test_dither_kernel_is_the_references_dithered_store(gpu, fx, trc, name):
    from dspfun_amd import engine
    c, sf, nm = tu8.dither_inputs(trc, name)
    h, w = c.shape
    d_co, d_pix = dev(gpu, c), dev(gpu, np.zeros((h, w), dtype=np.uint8))
    engine.motion_dither_u8(d_pix.data_ptr(), d_co.data_ptr(), (1, h, w), scalefactor=sf, normalization=nm, trc=trc)
    gpu.cuda.synchronize()
    assert np.array_equal(d_pix.cpu().numpy(), fx[f"dither_{trc}_{name}"])
    assert np.array_equal(d_co.cpu().numpy().view(np.uint32), c.view(np.uint32))


# ---- the flat pair ----
@pytest.mark.parametrize("trc", tr.IDS)
def test_flat_decode_of_all_256_codes(gpu, fx, trc):
    from dspfun_amd import engine
    codes = np.tile(np.arange(256, dtype=np.uint8), 5)[:1237]           # a length that leaves a tail behind the four-sample groups
    out = engine.u8_to_f32_trc(dev(gpu, codes), trc)
    gpu.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), fx[f"lut_{trc}"][codes].view(np.uint32))


@pytest.mark.parametrize("trc", tu8.STORE_TRCS)
def test_flat_encode_on_the_boundary_inputs(gpu, fx, trc):
    """the fixture's coefficients with the reference's constants folded into one multiplier: pel = (double)c * mul is then another double than
    the reference's two-step product, so the bar is the exact evaluation of that pel on the host, which trc_u8_byte equals by construction"""
    from dspfun_amd import engine
    sf, nm = tu8.store_scales()
    mul = float(F64(sf) * F64(nm) * F64(nm))
    co = np.concatenate([fx[f"store_{trc}_in"], tu8.random_coeffs(), np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=F32)])
    out = engine.f32_to_u8_trc(dev(gpu, co), trc, mul)
    gpu.cuda.synchronize()
    pel = co.astype(F64) * mul
    want = tu8.exact_bytes(trc, pel)
    want[np.isnan(pel)] = 0
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert np.unique(got).size == 256


def test_flat_pair_at_every_alignment_and_short_lengths(gpu, fx):
    from dspfun_amd import engine
    trc = 13
    lut = fx[f"lut_{trc}"]
    codes = ol.synth_u8(0x8B2, 64)
    lin = ((ol.synth_f32(0x8B3, 64).astype(F64) * 300.0 - 20.0)).astype(F32)
    for off in range(4):
        for ln in range(1, 10):
            src8, dstf = dev(gpu, codes), dev(gpu, np.full(64, F32(-5.0)))
            engine.u8_to_f32_trc(src8[off:off + ln], trc, out=dstf[off:off + ln])
            srcf, dst8 = dev(gpu, lin), dev(gpu, np.full(64, 77, dtype=np.uint8))
            engine.f32_to_u8_trc(srcf[off:off + ln], trc, MUL, out=dst8[off:off + ln])
            gpu.cuda.synchronize()
            wantf = np.full(64, F32(-5.0)); wantf[off:off + ln] = lut[codes[off:off + ln]]
            want8 = np.full(64, 77, dtype=np.uint8); want8[off:off + ln] = tu8.exact_bytes(trc, lin[off:off + ln].astype(F64) * MUL)
            assert np.array_equal(dstf.cpu().numpy().view(np.uint32), wantf.view(np.uint32)), (off, ln)
            assert np.array_equal(dst8.cpu().numpy(), want8), (off, ln)


# ---- every path of the 8-bit roundtrip equals the composition ----
def motion_scales(fwd, inv, n):
    fwd.set_scale(2 * R2)
    inv.set_scale(1.0 / (2 * R2) / float(np.prod([2.0 * v for v in n])))
    for a in range(len(n)):
        fwd.set_axis_scale0(a, 1.0, 1.0 / R2)
        inv.set_axis_scale0(a, R2, 1.0)
    return fwd, inv


def composed(gpu, fwd, inv, pix, trc, flt, mul=MUL, zero_outside=None, **kw):
    """dspfft_u8_to_f32_trc -> float roundtrip (in place) -> dspfft_f32_to_u8_trc on plans that have NOT been given the function"""
    from dspfun_amd import engine
    f = engine.u8_to_f32_trc(dev(gpu, pix), trc)
    if zero_outside is not None:
        f = f * dev(gpu, zero_outside.astype(F32))
    fwd.roundtrip(inv, f.data_ptr(), filter=flt, **kw)
    out = engine.f32_to_u8_trc(f, trc, mul)
    gpu.cuda.synchronize()
    return out.cpu().numpy()


def fused(gpu, fwd, inv, pix, flt, mul=MUL, **kw):
    din = dev(gpu, pix); dout = gpu.zeros_like(din); work = gpu.full(pix.shape, 3.0, dtype=gpu.float32, device="cuda:0")
    fwd.roundtrip_u8(inv, din.data_ptr(), dout.data_ptr(), work.data_ptr(), mul, filter=flt, **kw)
    gpu.cuda.synchronize()
    return dout.cpu().numpy()


def frame_plans(frames, h, w):
    from dspfun_amd import Plan
    return motion_scales(Plan.many_r2r([h, w], [5, 5], howmany=frames, idist=h * w, odist=h * w),
                         Plan.many_r2r([h, w], [4, 4], howmany=frames, idist=h * w, odist=h * w, first_axis_first=True), [h, w])


def frame_filter(h, w):
    return dict(active=(1, h, w), minbuf_hw=(h, w), block_depth=1, band_begin=(0, 0, 0), band_end=(1, h, w), quantizer=20.0 * 8 * math.sqrt(w * h))


@pytest.mark.parametrize("trc", [13, 7])
def test_frames_through_the_row_ends_and_the_fused_column_roundtrip(gpu, trc):
    frames, h, w = 3, 540, 960
    pix = ol.synth_u8(0x8B10, frames * h * w).reshape(frames, h, w)
    fwd, inv = frame_plans(frames, h, w)
    d = fwd.describe().splitlines()
    assert "ROW*" in d[1] and "COL*" in d[2] and "ROW*" in inv.describe().splitlines()[2], (fwd.describe(), inv.describe())
    flt = frame_filter(h, w)
    want = composed(gpu, fwd, inv, pix, trc, flt)
    fwd.set_u8_trc(trc); inv.set_u8_trc(trc)
    assert tr.TABLE[trc][0] in fwd.describe()
    got = fused(gpu, fwd, inv, pix, flt)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.unique(got).size > 100
    # and the function matters: the plain call gives other bytes
    fwd.set_u8_trc(0); inv.set_u8_trc(0)
    assert (fused(gpu, fwd, inv, pix, flt) != got).mean() > 0.2


def test_one_3d_block_with_the_8_bit_ends(gpu):
    from dspfun_amd import Plan
    n = [4, 6, 960]
    fwd, inv = motion_scales(Plan.many_r2r(n, [5] * 3), Plan.many_r2r(n, [4] * 3, first_axis_first=True), n)
    assert "ROW*" in fwd.describe().splitlines()[1] and "ROW*" in inv.describe().splitlines()[-1], (fwd.describe(), inv.describe())
    pix = ol.synth_u8(0x8B11, int(np.prod(n))).reshape(n)
    flt = dict(active=tuple(n), minbuf_hw=(n[1], n[2]), block_depth=n[0], band_begin=(0, 0, 0), band_end=tuple(n), quantizer=6.0 * 8 * math.sqrt(np.prod(n)))
    want = composed(gpu, fwd, inv, pix, 13, flt)
    fwd.set_u8_trc(13); inv.set_u8_trc(13)
    assert np.array_equal(fused(gpu, fwd, inv, pix, flt), want)


def test_a_968_wide_clip_converts_by_sweeps(gpu):
    frames, h, w = 2, 24, 968
    fwd, inv = frame_plans(frames, h, w)
    assert "ROW*" not in fwd.describe(), fwd.describe()          # (no listed row kernel for 968 samples)
    pix = ol.synth_u8(0x8B12, frames * h * w).reshape(frames, h, w)
    flt = frame_filter(h, w)
    want = composed(gpu, fwd, inv, pix, 13, flt)
    fwd.set_u8_trc("iec61966-2-1"); inv.set_u8_trc("iec61966-2-1")
    assert np.array_equal(fused(gpu, fwd, inv, pix, flt), want)


def test_scaled_not_block(gpu):
    from dspfun_amd import Plan
    from test_motion_rescale import plans
    import motion_ref as mr
    block, scaled = (4, 12, 16), (4, 18, 24)
    minbuf = tuple(max(b, s) for b, s in zip(block, scaled))
    active = tuple(min(b, s) for b, s in zip(block, scaled))
    pix = ol.synth_u8(0x8B13, int(np.prod(minbuf))).reshape(minbuf)
    fwd, inv = plans(Plan, block, scaled, minbuf)
    sf, nm = mr.consts(block, scaled)
    mul = sf * nm * nm
    flt = dict(active=active, minbuf_hw=minbuf[1:], block_depth=minbuf[0], band_begin=(0, 0, 0), band_end=active, quantizer=0.4 * 8 * math.sqrt(float(np.prod(scaled))))
    inside = np.zeros(minbuf, dtype=bool)
    inside[:block[0], :block[1], :block[2]] = True
    want = composed(gpu, fwd, inv, pix, 13, flt, mul=mul, zero_outside=inside)
    fwd.set_u8_trc(13); inv.set_u8_trc(13)
    got = fused(gpu, fwd, inv, pix, flt, mul=mul)
    sd, sh, sw = scaled
    assert np.array_equal(got[:sd, :sh, :sw], want[:sd, :sh, :sw])
    assert not got[sd:].any() and not got[:, sh:].any() and not got[:, :, sw:].any()
    assert np.unique(got[:sd, :sh, :sw]).size > 50


def volume_plans(block, D, H, W):
    from dspfun_amd import Plan
    bd, bh, bw = block
    dims = [d for d in [(bd, H * W, H * W), (bh, W, W), (bw, 1, 1)] if d[0] > 1]
    how = [(D // bd, bd * H * W, bd * H * W), (H // bh, bh * W, bh * W), (W // bw, bw, bw)]
    n = [d[0] for d in dims]
    fwd, inv = motion_scales(Plan.guru(dims, how, [5] * len(n)), Plan.guru(dims, how, [4] * len(n)), n)
    assert "side by side" in fwd.describe() and "BLOCK" in inv.describe()
    return fwd, inv


def stack_plans(block, nb):
    from dspfun_amd import Plan
    n = [v for v in block if v > 1]
    vol = int(np.prod(block))
    fwd, inv = motion_scales(Plan.many_r2r(n, [5] * len(n), howmany=nb, idist=vol, odist=vol),
                             Plan.many_r2r(n, [4] * len(n), howmany=nb, idist=vol, odist=vol, first_axis_first=True), n)
    assert "block-major" in fwd.describe()
    return fwd, inv


@pytest.mark.parametrize("keep", [0, 5])
@pytest.mark.parametrize("layout,block", [("volume", (8, 8, 8)), ("volume", (1, 16, 16)), ("stack", (8, 8, 8))])
def test_fused_small_blocks(gpu, layout, block, keep):
    """the fused block kernel (keep = 5: its --coeff-limit twin) with the tables in LDS behind its tile.  16 x 32 x 64 samples: 16 blocks of
    8 x 8 x 8 (one partial group of a row of blocks) or 128 of 16 x 16 x 1"""
    D, H, W = 16, 32, 64
    bd, bh, bw = block
    pix = ol.synth_u8(0x8B14 + bd, D * H * W).reshape(D, H, W)
    flt = dict(active=block, minbuf_hw=(bh, bw), block_depth=bd, band_begin=(0, 0, 0), band_end=block, quantizer=3.0)
    if layout == "stack":
        nb = D * H * W // (bd * bh * bw)
        pix = pix.reshape(nb, bd * bh * bw)
        fwd, inv = stack_plans(block, nb)
    else:
        fwd, inv = volume_plans(block, D, H, W)
    kw = dict(coeff_limit=keep) if keep else {}
    want = composed(gpu, fwd, inv, pix, 13, flt, **kw)
    fwd.set_u8_trc(13); inv.set_u8_trc(13)
    got = fused(gpu, fwd, inv, pix, flt, **kw)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.unique(got).size > 50


def test_reset_gives_the_bytes_of_plans_that_were_never_told(gpu):
    frames, h, w = 2, 540, 960
    pix = ol.synth_u8(0x8B15, frames * h * w).reshape(frames, h, w)
    flt = frame_filter(h, w)
    never = fused(gpu, *frame_plans(frames, h, w), pix, flt)
    fwd, inv = frame_plans(frames, h, w)
    fwd.set_u8_trc(13); inv.set_u8_trc(13)
    told = fused(gpu, fwd, inv, pix, flt)
    fwd.set_u8_trc(0); inv.set_u8_trc(0)
    assert np.array_equal(fused(gpu, fwd, inv, pix, flt), never) and not np.array_equal(told, never)
    # blocks too
    block, (D, H, W) = (8, 8, 8), (16, 32, 64)
    vp = ol.synth_u8(0x8B16, D * H * W).reshape(D, H, W)
    bf = dict(active=block, minbuf_hw=(8, 8), block_depth=8, band_begin=(0, 0, 0), band_end=block, quantizer=3.0)
    never = fused(gpu, *volume_plans(block, D, H, W), vp, bf)
    fwd, inv = volume_plans(block, D, H, W)
    fwd.set_u8_trc(7); inv.set_u8_trc(7)
    told = fused(gpu, fwd, inv, vp, bf)
    fwd.set_u8_trc(None); inv.set_u8_trc("none")
    assert np.array_equal(fused(gpu, fwd, inv, vp, bf), never) and not np.array_equal(told, never)


def test_dithered_roundtrip_takes_the_function(gpu):
    """frames through the row load and the dither kernel: equal to decode sweep -> float roundtrip -> dspfft_motion_dither_u8_trc"""
    from dspfun_amd import engine
    frames, h, w = 2, 540, 960
    pix = ol.synth_u8(0x8B17, frames * h * w).reshape(frames, h, w)
    fwd, inv = frame_plans(frames, h, w)
    flt = frame_filter(h, w)
    sf, nm = 1.0, math.sqrt(MUL)
    f = engine.u8_to_f32_trc(dev(gpu, pix), 13)
    fwd.roundtrip(inv, f.data_ptr(), filter=flt)
    want = gpu.zeros(pix.shape, dtype=gpu.uint8, device="cuda:0")
    engine.motion_dither_u8(want.data_ptr(), f.data_ptr(), (1, h, w), nblocks=(frames, 1, 1), block_step=(h * w, 0, 0), scalefactor=sf, normalization=nm, trc=13)
    fwd.set_u8_trc(13); inv.set_u8_trc(13)
    din = dev(gpu, pix); dout = gpu.zeros_like(din); work = gpu.empty(pix.shape, dtype=gpu.float32, device="cuda:0")
    fwd.roundtrip_u8_dither(inv, din.data_ptr(), dout.data_ptr(), work.data_ptr(), sf, nm, filter=flt)
    gpu.cuda.synchronize()
    assert np.array_equal(dout.cpu().numpy(), want.cpu().numpy())


def test_dithered_block_roundtrip_takes_the_function(gpu):
    """8 x 8 x 8 blocks of a volume through the fused block kernel with the decode table and a float result, then the dither kernel: equal to
    decode sweep -> float roundtrip -> dspfft_motion_dither_u8_trc over the same blocks"""
    from dspfun_amd import engine
    block, (D, H, W) = (8, 8, 8), (16, 32, 64)
    pix = ol.synth_u8(0x8B19, D * H * W).reshape(D, H, W)
    flt = dict(active=block, minbuf_hw=(8, 8), block_depth=8, band_begin=(0, 0, 0), band_end=block, quantizer=3.0)
    fwd, inv = volume_plans(block, D, H, W)
    sf, nm = 1.0, math.sqrt(MUL)
    f = engine.u8_to_f32_trc(dev(gpu, pix), 13)
    fwd.roundtrip(inv, f.data_ptr(), filter=flt)
    want = gpu.zeros(pix.shape, dtype=gpu.uint8, device="cuda:0")
    engine.motion_dither_u8(want.data_ptr(), f.data_ptr(), block, row_pitch=W, plane_pitch=H * W, nblocks=(D // 8, H // 8, W // 8),
                            block_step=(8 * H * W, 8 * W, 8), scalefactor=sf, normalization=nm, trc=13)
    fwd.set_u8_trc(13); inv.set_u8_trc(13)
    din = dev(gpu, pix); dout = gpu.zeros_like(din); work = gpu.empty(pix.shape, dtype=gpu.float32, device="cuda:0")
    fwd.roundtrip_u8_dither(inv, din.data_ptr(), dout.data_ptr(), work.data_ptr(), sf, nm, filter=flt)
    gpu.cuda.synchronize()
    got = dout.cpu().numpy()
    assert np.array_equal(got, want.cpu().numpy()) and np.unique(got).size > 50


@pytest.mark.parametrize("keep", [0, 5])
def test_the_identity_function_gives_the_plain_kernels_bytes_and_counts(gpu, keep):
    """trc `linear` is the identity: its decode table is the byte itself and its thresholds are the half-integers, so the kernels with tables
    must give what the plain kernels give -- bytes and the count of coded coefficients.  The block kernels with tables are the plain
    kernels' sequence of phases (block_rt.h) with TRC = true."""
    block, (D, H, W) = (8, 8, 8), (16, 32, 64)
    pix = ol.synth_u8(0x8B1A, D * H * W).reshape(D, H, W)
    flt = dict(active=block, minbuf_hw=(8, 8), block_depth=8, band_begin=(0, 1, 0), band_end=(8, 8, 7), damp=0.5, boost=1.25, preserve_dc=1, quantizer=3.0)
    kw = dict(coeff_limit=keep) if keep else {}

    def run(fwd, inv, p, f):
        coded = gpu.zeros(1, dtype=gpu.int64, device="cuda:0")
        out = fused(gpu, fwd, inv, p, f, d_coded=coded.data_ptr(), **kw)
        return out, int(coded.item())

    plain = run(*volume_plans(block, D, H, W), pix, flt)
    fwd, inv = volume_plans(block, D, H, W)
    fwd.set_u8_trc("linear"); inv.set_u8_trc("linear")
    told = run(fwd, inv, pix, flt)
    assert np.array_equal(told[0], plain[0]) and told[1] == plain[1] > 0
    if not keep:
        frames, h, w = 2, 540, 960
        clip = ol.synth_u8(0x8B1B, frames * h * w).reshape(frames, h, w)
        ff = frame_filter(h, w)
        plain = run(*frame_plans(frames, h, w), clip, ff)
        fwd, inv = frame_plans(frames, h, w)
        fwd.set_u8_trc(8); inv.set_u8_trc(8)
        told = run(fwd, inv, clip, ff)
        assert np.array_equal(told[0], plain[0]) and told[1] == plain[1] > 0


# ---- a clip in slices: the switches are read once per process, so this is a child process (tests/test_rt_slices_gpu.py) ----
CHILD = r'''
import math, sys, zlib
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np, torch
import oracle_lib as ol
from dspfun_amd import Plan, engine
frames, h, w = 4, 1080, 1920
r2 = math.sqrt(2.0)
def plans():
    fwd = Plan.many_r2r([h, w], [5, 5], howmany=frames, idist=h * w, odist=h * w).set_scale(2.0)
    inv = Plan.many_r2r([h, w], [4, 4], howmany=frames, idist=h * w, odist=h * w, first_axis_first=True).set_scale(1.0 / 2.0 / (4.0 * h * w))
    for a in range(2):
        fwd.set_axis_scale0(a, 1.0, 1.0 / r2); inv.set_axis_scale0(a, r2, 1.0)
    return fwd, inv
src = torch.from_numpy(ol.synth_u8(0x8B18, frames * h * w).reshape(frames, h, w)).to("cuda:0")
flt = dict(active=(1, h, w), minbuf_hw=(h, w), block_depth=1, band_begin=(0, 0, 0), band_end=(1, h, w), quantizer=20.0 * 8 * math.sqrt(w * h))
def composed(trc):
    fwd, inv = plans()
    f = engine.u8_to_f32_trc(src, trc)
    fwd.roundtrip(inv, f.data_ptr(), filter=flt)
    return engine.f32_to_u8_trc(f, trc, %(mul)r)
fwd, inv = plans()
dst = torch.zeros_like(src); work = torch.empty(frames, h, w, device="cuda:0")
def run():
    fwd.roundtrip_u8(inv, src.data_ptr(), dst.data_ptr(), work.data_ptr(), %(mul)r, filter=flt, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dst.clone()
plain = run()
res = []
for trc in (13, 7, 0):
    fwd.set_u8_trc(trc); inv.set_u8_trc(trc)
    got = run()
    res.append(int(torch.equal(got, composed(trc) if trc else plain)))
    res.append(int(not torch.equal(got, plain)) if trc else 1)
d = fwd.describe()
print("RESULT", "sliced" if "roundtrip_u8 in slices of 2 frames" in d else "whole", *res)
'''


def test_a_clip_in_two_slices_and_a_function_set_between_runs():
    """1920 x 1080 x 4 in two slices of two frames: plain, then iec61966-2-1, then smpte240m, then reset, on the SAME plan pair -- the slice
    plans follow what their parents are told between runs; every run equals its composition"""
    e = dict(os.environ); e.update({"DSPFFT_RT_SLICE": "2", "DSPFFT_RT_STREAMS": "2"})
    r = subprocess.run([sys.executable, "-c", CHILD % dict(root=os.path.dirname(HERE), tests=HERE, mul=MUL)], env=e, capture_output=True, text=True, timeout=600)
    lines = [x for x in r.stdout.splitlines() if x.startswith("RESULT")]
    assert lines, r.stderr[-2000:]
    assert lines[0].split()[1:] == ["sliced"] + ["1"] * 6, lines[0]


# ---- refusals launch nothing ----
def test_refused_inputs_launch_nothing(gpu):
    from dspfun_amd import Plan, _lib, engine
    L = _lib.load()
    p64 = Plan.many_r2r([16, 16], [5, 5], dtype="f64")
    with pytest.raises(engine.DspfftError, match="f32 plans"):
        p64.set_u8_trc(13)
    p32 = Plan.many_r2r([16, 16], [5, 5])
    for bad in (16, 2):
        assert L.dspfft_plan_set_u8_trc(p32._h, bad) == -1 and b"not built" in L.dspfft_last_error()
    assert L.dspfft_plan_set_u8_trc(None, 13) == -1
    assert "transfer characteristic" not in p32.describe()
    n = 960
    f = dev(gpu, np.full(n, F32(-5.0))); b = dev(gpu, np.full(n, 77, dtype=np.uint8))
    ia = lambda v: (C.c_int * len(v))(*v)
    g = _lib.DitherGeom()
    g.n[:] = [1, 24, 40]; g.row_pitch = 40; g.plane_pitch = 960; g.nblocks[:] = [1, 1, 1]; g.block_step[:] = [0, 0, 0]
    st = C.c_void_p(gpu.cuda.current_stream().cuda_stream)
    fp, bp = C.c_void_p(f.data_ptr()), C.c_void_p(b.data_ptr())
    for bad in (16, 2, 0):
        assert L.dspfft_u8_to_f32_trc(fp, bp, n, bad, st) == -1
        assert L.dspfft_f32_to_u8_trc(bp, fp, 1.0, n, bad, st) == -1
        assert L.dspfft_motion_load_u8_linear(fp, bp, ia([1, 24, 40]), ia([24, 40]), bad, st) == -1
        assert L.dspfft_motion_store_u8_linear(bp, fp, ia([1, 24, 40]), ia([24, 40]), 1.0, 1.0, bad, st) == -1
        assert L.dspfft_motion_dither_u8_trc(bp, fp, C.byref(g), 1.0, 1.0, bad, st) == -1
    gpu.cuda.synchronize()
    assert bool((f == -5.0).all()) and bool((b == 77).all())
