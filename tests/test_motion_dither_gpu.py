"""GPU (-m gpu): motion's dithered 8-bit store (motion/motion.c:756-788 with -d) on the device.

* dspfft_motion_dither_u8 against tests/golden/ref_dither.npz: byte-identical to the reference's lines at COEFF=F / INTERMEDIATE=D, within the
  documented bar of its default long double build; the float input is left bit-identical; both wavefront schedules (a workgroup of waves per
  plane, one wave per plane: DSPFFT_DITHER_WAVES=1) agree.
* dspfft_execute_roundtrip_u8_dither end to end, every path of the undithered call: the float work buffer it leaves (the inverse transform's
  output) dithered by the test-side restatement (tests/dither_ref.py) is the output, byte for byte; sliced and unsliced clips agree; the
  count of coded coefficients is the undithered call's.
Every end-to-end setting runs in a child process (the library reads its switches once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def fixture_check(names=None):
    import torch
    import dither_ref as dr
    from dspfun_amd.engine import motion_dither_u8
    z = np.load(os.path.join(HERE, "golden", "ref_dither.npz"))
    stream = torch.cuda.current_stream().cuda_stream
    for i, (name, scaled, minbuf, nb, _) in enumerate(dr.CASES):
        if names and name not in names:
            continue
        c, sf, nm, scaled, minbuf, block = dr.case_inputs(i)
        md, mh, mw = minbuf
        dc = torch.from_numpy(np.ascontiguousarray(c)).cuda()
        before = dc.clone()
        pix = torch.zeros(c.shape, dtype=torch.uint8, device="cuda")
        motion_dither_u8(pix.data_ptr(), dc.data_ptr(), scaled, row_pitch=mw, plane_pitch=mh * mw, nblocks=(nb, 1, 1), block_step=(md * mh * mw, 0, 0),
                         scalefactor=sf, normalization=nm, stream=stream)
        torch.cuda.synchronize()
        d, h, w = scaled
        got = pix.cpu().numpy()[:, :d, :h, :w]
        fd, fl = z["out_fd_" + name], z["out_fl_" + name]
        assert np.array_equal(got, fd), (name, int((got != fd).sum()))
        assert np.abs(got.astype(int) - fl.astype(int)).max() <= 1, name
        assert torch.equal(dc.view(torch.int32), before.view(torch.int32)), name       # d_coeffs is read, never written
        outside = pix.cpu().numpy().copy()
        outside[:, :d, :h, :w] = 0
        assert not outside.any(), name                                                  # nothing written outside the scaled extent
    return True


def test_kernel_matches_reference_fixtures():
    assert fixture_check()


def test_geometry_refused():
    import torch
    from dspfun_amd.engine import motion_dither_u8, DspfftError
    buf = torch.zeros(64, device="cuda")
    pix = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(DspfftError, match="extents"):
        motion_dither_u8(pix.data_ptr(), buf.data_ptr(), (1, 0, 8))
    with pytest.raises(DspfftError, match="pitch"):
        motion_dither_u8(pix.data_ptr(), buf.data_ptr(), (1, 4, 8), row_pitch=4)
    with pytest.raises(DspfftError, match="null"):
        motion_dither_u8(0, buf.data_ptr(), (1, 4, 8))


CHILD = r'''
import math, sys, zlib
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
from dspfun_amd import Plan, REDFT10, REDFT01
mode = %(mode)r
if mode == "fixtures":
    import test_motion_dither_gpu as t
    t.fixture_check(); print("RESULT ok"); sys.exit(0)
import dither_ref as dr
dev = torch.device("cuda", 0)
r2 = math.sqrt(2.0)
st = torch.cuda.current_stream().cuda_stream
NM = 0.5                                # pel = value * sf * NM * NM: the inverse plans carry 1 / NM^2 so that pels are pixel-sized
flt = None
def planes_of(mode):
    global flt
    if mode in ("c5_3d", "chroma_3d"):
        d_, h, w = (256, 1080, 1920) if mode == "c5_3d" else (256, 540, 960)
        fwd = Plan.many_r2r([d_, h, w], [REDFT10] * 3).set_scale(2 * r2)
        inv = Plan.many_r2r([d_, h, w], [REDFT01] * 3, first_axis_first=True).set_scale(1.0 / (2 * r2) / (8.0 * d_ * h * w) / NM / NM)
        for a in range(3): fwd.set_axis_scale0(a, 1.0, 1.0 / r2); inv.set_axis_scale0(a, r2, 1.0)
        return fwd, inv, (d_, h, w), (d_, h, w), 1.0, [0, 1, 127, 255]
    if mode in ("frames16", "frames64"):
        nf, h, w = (16 if mode == "frames16" else 64), 1080, 1920
        fwd = Plan.many_r2r([h, w], [REDFT10] * 2, howmany=nf, idist=h * w, odist=h * w).set_scale(2.0)
        inv = Plan.many_r2r([h, w], [REDFT01] * 2, howmany=nf, idist=h * w, odist=h * w, first_axis_first=True).set_scale(1.0 / 2.0 / (4.0 * h * w) / NM / NM)
        for a in range(2): fwd.set_axis_scale0(a, 1.0, 1.0 / r2); inv.set_axis_scale0(a, r2, 1.0)
        flt = dict(active=(1, h, w), minbuf_hw=(h, w), block_depth=1, band_begin=(0, 0, 0), band_end=(1, h, w), quantizer=4.0 * 8 * math.sqrt(w * h))
        return fwd, inv, (nf, h, w), (nf, h, w), 1.0, [0, 1, nf // 2, nf - 1]
    if mode == "rescale":                # scaled != block: 360x640 blocks upscaled to 540x960 in one embedding (scalefactor 2.25)
        bh, bw, h, w = 360, 640, 540, 960
        fwd = Plan.many_r2r([bh, bw], [REDFT10] * 2, inembed=[h, w], onembed=[h, w]).set_scale(2.0)
        inv = Plan.many_r2r([h, w], [REDFT01] * 2, inembed=[h, w], onembed=[h, w], first_axis_first=True).set_scale(1.0 / 2.0 / (4.0 * bh * bw) / NM / NM / 2.25)
        for a in range(2): fwd.set_axis_scale0(a, 1.0, 1.0 / r2); inv.set_axis_scale0(a, r2, 1.0)
        return fwd, inv, (1, h, w), (1, h, w), 2.25, [0]
    if mode == "blocks":                 # 8x8x8 blocks as a block-major stack (the fused small-block kernel)
        nb = 256
        fwd = Plan.many_r2r([8, 8, 8], [REDFT10] * 3, howmany=nb, idist=512, odist=512).set_scale(2 * r2)
        inv = Plan.many_r2r([8, 8, 8], [REDFT01] * 3, howmany=nb, idist=512, odist=512, first_axis_first=True).set_scale(1.0 / (2 * r2) / (8.0 * 512) / NM / NM)
        for a in range(3): fwd.set_axis_scale0(a, 1.0, 1.0 / r2); inv.set_axis_scale0(a, r2, 1.0)
        return fwd, inv, (nb * 8, 8, 8), (nb * 8, 8, 8), 1.0, None
    if mode == "guru":                   # 8x8x8 blocks where they lie in a 16 x 64 x 64 volume
        D, H, W = 16, 64, 64
        dims = [(8, H * W, H * W), (8, W, W), (8, 1, 1)]
        hm = [(D // 8, 8 * H * W, 8 * H * W), (H // 8, 8 * W, 8 * W), (W // 8, 8, 8)]
        fwd = Plan.guru(dims, hm, [REDFT10] * 3).set_scale(2 * r2)
        inv = Plan.guru(dims, hm, [REDFT01] * 3).set_scale(1.0 / (2 * r2) / (8.0 * 512) / NM / NM)
        for a in range(3): fwd.set_axis_scale0(a, 1.0, 1.0 / r2); inv.set_axis_scale0(a, r2, 1.0)
        return fwd, inv, (D, H, W), (D, H, W), 1.0, "guru"
fwd, inv, shape, wshape, sf, check = planes_of(mode)
g = torch.Generator(device=dev); g.manual_seed(5)
src = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)
dst = torch.full(shape, 7, dtype=torch.uint8, device=dev)
work = torch.zeros(wshape, device=dev)
coded = torch.zeros(1, dtype=torch.int64, device=dev)
fwd.roundtrip_u8_dither(inv, src.data_ptr(), dst.data_ptr(), work.data_ptr(), sf, NM, filter=flt, d_coded=coded.data_ptr() if flt else 0, stream=st)
torch.cuda.synchronize()
out = dst.cpu().numpy(); wk = work.cpu().numpy()
bad = 0
if check == "guru":
    for bz in range(0, shape[0], 8):
        for by in range(0, shape[1], 8):
            for bx in range(0, shape[2], 8):
                ref = dr.dither_planes(wk[bz:bz + 8, by:by + 8, bx:bx + 8], sf, NM)
                bad += int((ref != out[bz:bz + 8, by:by + 8, bx:bx + 8]).sum())
elif check is None:
    bad = int((dr.dither_planes(wk, sf, NM) != out).sum())
else:
    for f in check:
        bad += int((dr.dither_plane(wk[f], sf, NM) != out[f]).sum())
extra = ""
if flt:
    c2 = torch.zeros(1, dtype=torch.int64, device=dev); d2 = torch.empty_like(dst)
    fwd.roundtrip_u8(inv, src.data_ptr(), d2.data_ptr(), work.data_ptr(), sf * NM * NM, filter=flt, d_coded=c2.data_ptr(), stream=st)
    torch.cuda.synchronize()
    extra = "coded %%d %%d" %% (int(coded.item()), int(c2.item()))
d = fwd.describe()
print("RESULT", bad, "%%08x" %% zlib.crc32(out.tobytes()), "sliced" if "roundtrip_u8 in slices of" in d else "whole", extra)
'''


def run(mode, env=None):
    e = dict(os.environ); e.update(env or {})
    r = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, tests=HERE, mode=mode)], env=e, capture_output=True, text=True, timeout=900)
    lines = [x for x in r.stdout.splitlines() if x.startswith("RESULT")]
    assert lines, (r.returncode, r.stderr[-3000:])
    return lines[0].split()[1:]


def test_one_wave_per_plane_schedule_matches_fixtures():
    assert run("fixtures", {"DSPFFT_DITHER_WAVES": "1"}) == ["ok"]


@pytest.mark.parametrize("mode", ["c5_3d", "chroma_3d", "frames16", "rescale", "blocks", "guru"])
def test_roundtrip_dither_end_to_end_exact(mode):
    got = run(mode, {"DSPFFT_RT_SLICE": "0"})
    assert got[0] == "0", got
    if mode == "frames16":
        assert got[3] == "coded" and got[4] == got[5] and int(got[4]) > 0, got      # the quantiser's count is the undithered call's


def test_sliced_clip_is_the_unsliced_clip():
    whole = run("frames64", {"DSPFFT_RT_SLICE": "0"})
    assert whole[0] == "0" and whole[2] == "whole", whole
    for env in ({}, {"DSPFFT_RT_SLICE": "7", "DSPFFT_RT_STREAMS": "1"}):
        got = run("frames64", env)
        assert got[2] == "sliced", (env, got)
        # (bytes by checksum: a sliced clip reuses its work areas, so d_work no longer holds every frame's floats)
        assert got[1] == whole[1] and got[3:] == whole[3:], (env, got, whole)


def test_dither_tracks_a_smooth_gradient_better():
    """sanity: on a slow ramp the undithered store is flat steps, the dithered one's 8x8 block means follow the float image"""
    import torch
    from dspfun_amd import _lib
    from dspfun_amd.engine import motion_dither_u8
    h, w = 256, 512
    ramp = (100.0 + np.linspace(0.0, 3.0, w, dtype=np.float64)[None, :] + np.linspace(0.0, 1.0, h)[:, None]).astype(np.float32)
    dc = torch.from_numpy(ramp).cuda()
    pd = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    pu = torch.zeros_like(pd)
    motion_dither_u8(pd.data_ptr(), dc.data_ptr(), (1, h, w), scalefactor=1.0, normalization=1.0)
    lib = _lib.load()
    assert lib.dspfft_f32_to_u8(pu.data_ptr(), dc.data_ptr(), 1.0, h * w, None) == 0
    torch.cuda.synchronize()
    means = lambda a: a.reshape(h // 8, 8, w // 8, 8).mean(axis=(1, 3))
    ref = means(ramp.astype(np.float64))
    ed = np.abs(means(pd.cpu().numpy().astype(np.float64)) - ref).mean()
    eu = np.abs(means(pu.cpu().numpy().astype(np.float64)) - ref).mean()
    assert ed < 0.5 * eu, (ed, eu)
