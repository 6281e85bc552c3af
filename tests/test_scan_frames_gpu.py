"""GPU (-m gpu): scan's output frames composed on the device (dspfft_scanframes_*, scan_frame.hip) against the restatement of scan.c's
frame loop over scan_frame_core.h (tests/scan_frames_ref.py) fed the device's own coefficients and per-frame images; against the fixture
of the reference's own lines (tests/golden/ref_scan_frames.npz) within scan's tolerances; the -i path's sum against the plain fused step;
host/scan_dev --video; a 7680x4320 frame with every option."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import scan_frames_ref as sfr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_scan_frames.npz")


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return torch


def _scan_frames(torch, o, w, h):
    from dspfun_amd import ScanFrames
    return ScanFrames(w, h, visualize=o["v"], spectrogram=o["s"], intermediates=o["i"], max_intermediates=o["M"], spec_gain=o["gain"],
                      spec_scale=o["scale"], spec_sign=o["sign"], parity_depth=o["P"])


def device_run(torch, case):
    """the case on the device: frames, per-frame images (fill first), coefficients, parity, final sum"""
    from dspfun_amd import Plan, REDFT10, REDFT01
    name, w, h, seed, method, step, _o, _n, invert, skip = case[:10]
    o = sfr.opts(case)
    n, npix = w * h * 3, w * h
    orig, _ = sfr.case_inputs(case)
    d_orig = torch.from_numpy(orig.ravel().copy()).cuda()
    d_co = d_orig.clone()
    Plan.image(h, w, 3, REDFT10).set_scale(1.0 / (4.0 * w * h)).execute(d_co.data_ptr())
    torch.cuda.synchronize()
    co = d_co.cpu().numpy().reshape(h, w, 3)
    order = sfr.orders(case, co)
    limit = len(order)
    offset, nframes = sfr.loop_params(case, limit)
    owner = np.full(npix, NONE, dtype=np.uint32)
    shared = False
    for i, cs in enumerate(order):
        for (y, x) in cs:
            shared |= owner[y * w + x] not in (NONE, i)
            owner[y * w + x] = i
    d_owner = torch.from_numpy(owner.view(np.int32)).cuda()
    inv = Plan.image(h, w, 3, REDFT01)
    sf = _scan_frames(torch, o, w, h)
    assert sf.frame_floats == 3 * w * (1 + o["v"]) * h * (1 + o["i"])
    frame = torch.empty(sf.frame_floats, dtype=torch.float32, device="cuda")
    frame.fill_(7.0)                                          # begin clears it
    d_sum = d_co[:3].repeat(npix).contiguous()
    image = torch.full((n,), -0.0, dtype=torch.float32, device="cuda")
    work = torch.empty(n, dtype=torch.float32, device="cuda")
    sf.begin(frame, d_co)
    images = []

    def lin_of(a, b):
        return torch.from_numpy(np.array([y * w + x for j in range(a, b) for (y, x) in order[j]] or [NONE], dtype=np.uint32).view(np.int32)).cuda()

    def mark(a, b, current):
        if shared:
            lin = lin_of(a, b)
            sf.mark_coords(frame, d_co, lin, current=current)
        else:
            sf.mark_range(frame, d_co, d_owner, a, b, current)

    def step_into_image(a, b):
        sel = np.full(npix, NONE, dtype=np.uint32)
        for j in range(a, b):
            for (y, x) in order[j]:
                sel[y * w + x] = 0
        sel[0] = NONE                                         # scan.c:406,445: DC cleared before every inverse
        ids = torch.from_numpy(sel.view(np.int32)).cuda()
        inv.execute_masked_accumulate(d_co.data_ptr(), work.data_ptr(), image.data_ptr(), ids.data_ptr(), 0, 3)

    if not skip and offset > 0:
        a, b = (limit - offset, limit) if invert else (0, offset)
        mark(a, b, False)
        step_into_image(a, b)
        images.append(image.cpu().numpy())
        d_sum += image
        image.fill_(-0.0)
    frames = []
    for k, i in enumerate(range(offset, offset + nframes)):
        lo = i * step
        hi = min(lo + step, limit)
        a, b = ((limit - hi, limit - lo) if invert else (lo, hi)) if lo < limit else (0, 0)
        mark(a, b, True)
        if b > a:
            step_into_image(a, b)
        images.append(image.cpu().numpy())
        sf.compose(frame, d_sum, image, d_co, d_orig if o["P"] else None, k)
        frames.append(frame.cpu().numpy().reshape(sfr.frame_shape(case)))
        assert torch.all(image.view(torch.int32) == np.int32(-2 ** 31)).item()        # compose refilled it with -0.0f
    par = sf.parity() if o["P"] else None
    return np.stack(frames), np.stack(images), co, orig, order, par, d_sum.cpu().numpy()


def _ulp_close(a, b, ulps):
    ai, bi = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ai - bi) <= ulps


@pytest.mark.parametrize("case", sfr.CASES, ids=[c[0] for c in sfr.CASES])
def test_device_frames_match_restatement(gpu, case):
    frames, images, co, orig, order, par, _ = device_run(gpu, case)
    want, want_par = sfr.run(case, co, orig, order, images=images)
    assert frames.shape == want.shape
    o = sfr.opts(case)
    w = case[1]
    if o["s"]:
        # spectrogram panels: device log1p against glibc's, within 1 float ulp; everything else bit for bit
        right = np.zeros(frames.shape, dtype=bool)
        right[..., w:] = True
        assert np.array_equal(frames[~right].view(np.int32), want[~right].view(np.int32)), case[0]
        assert _ulp_close(frames[right], want[right], 1).all(), case[0]
    else:
        assert np.array_equal(frames.view(np.int32), want.view(np.int32)), case[0]
    assert par == want_par, (case[0], par, want_par)


@pytest.mark.parametrize("case", sfr.CASES, ids=[c[0] for c in sfr.CASES])
def test_device_frames_near_reference_fixture(gpu, case):
    fx = np.load(FIXTURE)
    frames, images, co, orig, order, par, _ = device_run(gpu, case)
    ref = fx["frames_" + case[0]]
    assert frames.shape == ref.shape
    assert np.array_equal(np.isnan(frames), np.isnan(ref)), case[0]
    ok = ~np.isnan(ref)
    o = sfr.opts(case)
    w, h = case[1], case[2]
    # the f32 transform's differences from the stub inverse, amplified by -M's normalisation in the bottom-left panel
    err = np.abs(frames[ok].astype(np.float64) - ref[ok])
    assert err.max() <= (2e-3 if o["M"] else 2e-5), (case[0], err.max())
    # the mark masks (where a panel is lit) are the reference's exactly
    if o["v"]:
        assert np.array_equal(frames[..., :h, w:] != 0, ref[..., :h, w:] != 0), case[0]
    pfx = int(fx["parity_" + case[0]][0])
    if o["P"] == 8:
        assert par == (None if pfx < 0 else pfx), (case[0], par, pfx)


def test_intermediates_sum_equals_fused(gpu):
    """with -i the step adds into a -0.0f image and compose adds that to the sum: the same floats as the fused step into the sum"""
    torch = gpu
    from dspfun_amd import Plan, REDFT10, REDFT01, ScanFrames
    from dspfun_amd import _lib
    L = _lib.load()
    w, h, step = 96, 64, 97
    n, npix = w * h * 3, w * h
    x = ol.synth_f32(0x5F77, n)
    d_co = torch.from_numpy(x).cuda()
    Plan.image(h, w, 3, REDFT10).set_scale(1.0 / (4.0 * w * h)).execute(d_co.data_ptr())
    ids = torch.empty(npix, dtype=torch.int32, device="cuda")
    assert L.dspfft_scan_frame_ids(ids.data_ptr(), 2, w, h, step, None) == 0
    inv = Plan.image(h, w, 3, REDFT01)
    work = torch.empty(n, dtype=torch.float32, device="cuda")
    plain = d_co[:3].repeat(npix).contiguous()
    viai = plain.clone()
    image = torch.full((n,), -0.0, dtype=torch.float32, device="cuda")
    sf = ScanFrames(w, h, intermediates=True)
    frame = torch.empty(sf.frame_floats, dtype=torch.float32, device="cuda")
    sf.begin(frame, d_co)
    for f in range((npix + step - 1) // step):
        inv.execute_masked_accumulate(d_co.data_ptr(), work.data_ptr(), plain.data_ptr(), ids.data_ptr(), f, 3)
        inv.execute_masked_accumulate(d_co.data_ptr(), work.data_ptr(), image.data_ptr(), ids.data_ptr(), f, 3)
        sf.compose(frame, viai, image, d_co, None, f)
    torch.cuda.synchronize()
    assert torch.equal(plain.view(torch.int32), viai.view(torch.int32))


def _ppm(path, w, h, seed):
    px = ol.synth_u8(seed, w * h * 3)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(px.tobytes())
    return px.reshape(h, w, 3).astype(np.float32) / 255


def _run_scan_dev(args, tmp):
    exe = os.path.join(ROOT, "host", "scan_dev")
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, cwd=tmp)


def test_scan_dev_video(gpu, tmp_path):
    """--video: nframes raw gbrpf32le frames, equal to the Python path's; the final .pf unchanged by the option"""
    torch = gpu
    w, h, step = 24, 16, 40
    src = str(tmp_path / "in.ppm")
    _ppm(src, w, h, 0x5F88)
    vid = str(tmp_path / "v.raw")
    r0 = _run_scan_dev([src, str(tmp_path / "plain.pf"), str(step), "zigzag"], str(tmp_path))
    assert r0.returncode == 0, r0.stderr
    r1 = _run_scan_dev([src, str(tmp_path / "video.pf"), str(step), "zigzag", "-v", "-i", "-M", "-P", "--video", vid], str(tmp_path))
    assert r1.returncode == 0, r1.stderr
    assert "Reached parity" in r1.stderr or "Didn't reach parity" in r1.stderr
    with open(str(tmp_path / "plain.pf"), "rb") as a, open(str(tmp_path / "video.pf"), "rb") as b:
        assert a.read() == b.read()
    nframes = (w * h + step - 1) // step
    fw, fh = 2 * w, 2 * h
    assert os.path.getsize(vid) == nframes * 3 * fw * fh * 4
    got = np.fromfile(vid, dtype="<f4").reshape(nframes, 3, fh, fw)
    # the same run through the Python path
    case = ("video", w, h, 0x5F88, "zigzag", step, 0, 0, False, False, dict(v=1, i=1, M=1, P=8))
    from dspfun_amd import Plan, REDFT10, REDFT01
    L = __import__("dspfun_amd")._lib.load()
    pix = np.fromfile(src, dtype=np.uint8, offset=len(b"P6\n%d %d\n255\n" % (w, h))).astype(np.float32) / 255
    d_orig = torch.from_numpy(pix).cuda()
    d_co = d_orig.clone()
    Plan.image(h, w, 3, REDFT10).set_scale(1.0 / (4.0 * w * h)).execute(d_co.data_ptr())
    npix, n = w * h, w * h * 3
    owner = torch.empty(npix, dtype=torch.int32, device="cuda")
    assert L.dspfft_scan_owner_index(owner.data_ptr(), 2, w, h, None) == 0
    ids = torch.empty(npix, dtype=torch.int32, device="cuda")
    assert L.dspfft_scan_frame_ids(ids.data_ptr(), 2, w, h, step, None) == 0
    inv = Plan.image(h, w, 3, REDFT01)
    sf = _scan_frames(torch, sfr.opts(case), w, h)
    frame = torch.empty(sf.frame_floats, dtype=torch.float32, device="cuda")
    d_sum = d_co[:3].repeat(npix).contiguous()
    image = torch.full((n,), -0.0, dtype=torch.float32, device="cuda")
    work = torch.empty(n, dtype=torch.float32, device="cuda")
    sf.begin(frame, d_co)
    for f in range(nframes):
        sf.mark_range(frame, d_co, owner, f * step, min(f * step + step, npix), True)
        inv.execute_masked_accumulate(d_co.data_ptr(), work.data_ptr(), image.data_ptr(), ids.data_ptr(), f, 3)
        sf.compose(frame, d_sum, image, d_co, d_orig, f)
        assert np.array_equal(got[f].view(np.int32), frame.cpu().numpy().reshape(3, fh, fw).view(np.int32)), f
    par = sf.parity()
    want = "Reached parity with the original image at scan index %d" % par if par is not None else "Didn't reach parity"
    assert want in r1.stderr, r1.stderr


def test_8k_all_options_sampled_rows(gpu):
    """7680x4320 zigzag with -v -i -M -P over a few frames (a 1.6 GB frame: 64-bit offsets), checked on sampled rows"""
    torch = gpu
    from dspfun_amd import Plan, REDFT10, REDFT01, ScanFrames
    from dspfun_amd import _lib
    L = _lib.load()
    w, h, step = 7680, 4320, 2_000_000
    n, npix = w * h * 3, w * h
    x = torch.from_numpy(ol.synth_f32(0x5F8C, n)).cuda()
    d_co = x.clone()
    Plan.image(h, w, 3, REDFT10).set_scale(1.0 / (4.0 * w * h)).execute(d_co.data_ptr())
    owner = torch.empty(npix, dtype=torch.int32, device="cuda")
    assert L.dspfft_scan_owner_index(owner.data_ptr(), 2, w, h, None) == 0
    ids = torch.empty(npix, dtype=torch.int32, device="cuda")
    assert L.dspfft_scan_frame_ids(ids.data_ptr(), 2, w, h, step, None) == 0
    inv = Plan.image(h, w, 3, REDFT01)
    sf = ScanFrames(w, h, visualize=True, intermediates=True, max_intermediates=True, parity_depth=8)
    assert sf.frame_floats == 3 * 2 * w * 2 * h
    frame = torch.empty(sf.frame_floats, dtype=torch.float32, device="cuda")
    d_sum = d_co[:3].repeat(npix).contiguous()
    image = torch.full((n,), -0.0, dtype=torch.float32, device="cuda")
    work = torch.empty(n, dtype=torch.float32, device="cuda")
    sf.begin(frame, d_co)
    co = None
    own = owner.cpu().numpy().view(np.uint32).reshape(h, w)
    rows = [0, 1, 2159, 4318, 4319]
    for f in range(3):
        sf.mark_range(frame, d_co, owner, f * step, (f + 1) * step, True)
        inv.execute_masked_accumulate(d_co.data_ptr(), work.data_ptr(), image.data_ptr(), ids.data_ptr(), f, 3)
        img = image.view(h, w, 3).cpu().numpy()
        before = d_sum.view(h, w, 3).cpu().numpy()
        sf.compose(frame, d_sum, image, d_co, x, f)
        torch.cuda.synchronize()
        if co is None:
            co = d_co[:3].cpu().numpy()
        fr = frame.view(3, 2 * h, 2 * w)
        s = (before + img).astype(np.float32)
        mn = img.reshape(-1, 3).min(0) + co
        mx = img.reshape(-1, 3).max(0) + co
        for y in rows:
            planes = fr[:, [y, y + h], :].cpu().numpy()          # (3, 2, 2w)
            for z, p in ((0, 2), (1, 0), (2, 1)):
                assert np.array_equal(planes[p, 0, :w], s[y, :, z]), (f, y, z)
                inter = ((img[y, :, z] + co[z]) - mn[z]).astype(np.float32) / np.float32(mx[z] - mn[z])
                assert np.array_equal(planes[p, 1, :w], inter.astype(np.float32)), (f, y, z)
                lit = (own[y] >= f * step) & (own[y] < (f + 1) * step)
                assert np.array_equal(planes[p, 1, w:] != 0, lit), (f, y, z)
                seen = own[y] < (f + 1) * step
                assert np.array_equal(planes[p, 0, w:] != 0, seen), (f, y, z)
    assert sf.parity() is None
