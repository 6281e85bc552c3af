"""GPU (-m gpu): transfer characteristics on the device.  dspfft_trc_apply_f32 against the host's exact evaluation over the float sweep;
scan's frames, zoom's animation frames and motion's float load / store with a transfer characteristic against tests/golden/ref_trc.npz
(the reference's own loops with their hooks set, tests/golden/make_trc_fixtures.py); trc 0 against the same objects without the call;
host/scan_dev and host/zoom_dev --trc against the Python path."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import scan_frames_ref as sfr
import trc_ref as tr
import zoom_anim_ref as zr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
F32 = np.float32


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
    return np.load(tr.FIXTURE)


@pytest.fixture(scope="module")
def d_sweep(gpu):
    return gpu.from_numpy(tr.sweep().copy()).cuda()


# ---- dspfft_trc_apply_f32 ----
@pytest.mark.parametrize("inverse", (0, 1))
@pytest.mark.parametrize("trc", tr.IDS)
def test_apply_meets_the_bar_over_the_sweep(gpu, d_sweep, trc, inverse):
    """one launch over 6.35 M floats and the specials: within 1 float ulp of the host's (float)exact((double)x), bit-equal where that is
    +-0, NaN or +-inf; in place equals out of place"""
    from dspfun_amd import trc_apply
    out = trc_apply(d_sweep, trc, inverse=bool(inverse))
    inplace = d_sweep.clone()
    assert trc_apply(inplace, tr.TABLE[trc][0], inverse=bool(inverse), out=inplace) is inplace
    got = out.cpu().numpy()
    want = tr.want_f32(trc, inverse)
    bad = tr.bar_violations(got, want)
    off = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"trc {trc} inverse {inverse}: {off} of {got.size} differ from the host's rounding, {bad.size} miss the bar")
    assert bad.size == 0, (trc, inverse, tr.sweep()[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert gpu.equal(out.view(gpu.int32), inplace.view(gpu.int32))


@pytest.mark.parametrize("n", (1, 3, 4099))
def test_apply_unaligned_pointers_and_short_lengths(gpu, d_sweep, n):
    """source and destination one float past a 16-byte boundary (vector body with a scalar head), and at different offsets (all scalar);
    the floats around the destination stay as they were"""
    from dspfun_amd import trc_apply
    torch = gpu
    want = trc_apply(d_sweep[1000:1000 + n].clone(), 13).cpu().numpy()
    for so, do in ((5, 5), (5, 2), (4, 7)):
        s = torch.full((n + 16,), 7.0, dtype=torch.float32, device="cuda")
        s[so:so + n] = d_sweep[1000:1000 + n]
        dst = torch.full((n + 16,), -3.0, dtype=torch.float32, device="cuda")
        trc_apply(s[so:so + n], 13, out=dst[do:do + n])
        got = dst.cpu().numpy()
        assert got[do:do + n].tobytes() == want.tobytes(), (n, so, do)
        assert np.all(got[:do] == -3.0) and np.all(got[do + n:] == -3.0), (n, so, do)
    assert tr.bar_violations(want, tr.want_f32(13, 0)[1000:1000 + n]).size == 0


def test_apply_refuses_what_is_not_built(gpu):
    from dspfun_amd import _lib
    L = _lib.load()
    t = gpu.ones(8, dtype=gpu.float32, device="cuda")
    for trc in (0, 2, 9, 16, 18, 99):
        assert L.dspfft_trc_apply_f32(t.data_ptr(), t.data_ptr(), 8, trc, 0, None) == -1
    assert gpu.all(t == 1).item()


# ---- scan frames ----
def _ulp_close(a, b, ulps=1):
    return tr.ulps(a, b) <= ulps


def scan_run(torch, case, images, trc, call_set_trc=True):
    """the case's frame loop on the device, fed the recorded images of the stub inverse (the fill's first, unless the case skips it):
    frames, parity, final sum"""
    from dspfun_amd import ScanFrames
    name, w, h, seed, method, step, _o, _n, invert, skip = case[:10]
    o = sfr.opts(case)
    assert o["i"]                                           # every case here has the bottom panels: compose adds the image to the sum
    n, npix = w * h * 3, w * h
    orig, co = tr.scan_inputs(case)
    d_orig = torch.from_numpy(orig.ravel().copy()).cuda()
    d_co = torch.from_numpy(co.ravel().copy()).cuda()
    order = sfr.orders(case, co)
    limit = len(order)
    offset, nframes = sfr.loop_params(case, limit)
    owner = np.full(npix, NONE, dtype=np.uint32)
    for i, cs in enumerate(order):
        for (y, x) in cs:
            assert owner[y * w + x] in (NONE, i)
            owner[y * w + x] = i
    d_owner = torch.from_numpy(owner.view(np.int32)).cuda()
    kw = dict(visualize=o["v"], spectrogram=o["s"], intermediates=o["i"], max_intermediates=o["M"], spec_gain=o["gain"], spec_scale=o["scale"],
              spec_sign=o["sign"], parity_depth=o["P"])
    sf = ScanFrames(w, h, trc=trc, **kw) if call_set_trc else ScanFrames(w, h, **kw)
    if call_set_trc and not trc:
        sf.set_trc(0)
    frame = torch.full((sf.frame_floats,), 7.0, dtype=torch.float32, device="cuda")
    d_sum = d_co[:3].repeat(npix).contiguous()
    image = torch.full((n,), -0.0, dtype=torch.float32, device="cuda")
    sf.begin(frame, d_co)
    imgs = [torch.from_numpy(np.ascontiguousarray(im).ravel()).cuda() for im in images]
    k = 0
    if not skip:                                            # scan.c:389-417
        a, b = (limit - offset, limit) if invert else (0, offset)
        if offset > 0:
            sf.mark_range(frame, d_co, d_owner, a, b, False)
        d_sum += imgs[0]
        k = 1
    frames = []
    for f, i in enumerate(range(offset, offset + nframes)):
        lo = i * step
        hi = min(lo + step, limit)
        a, b = ((limit - hi, limit - lo) if invert else (lo, hi)) if lo < limit else (0, 0)
        sf.mark_range(frame, d_co, d_owner, a, b, True)
        image.copy_(imgs[k + f])
        sf.compose(frame, d_sum, image, d_co, d_orig if o["P"] else None, f)
        frames.append(frame.cpu().numpy().reshape(sfr.frame_shape(case)))
    par = sf.parity() if o["P"] else None
    return np.stack(frames), par, d_sum.cpu().numpy()


@pytest.mark.parametrize("trc", tr.SCAN_TRCS)
@pytest.mark.parametrize("name", tr.SCAN_CASES)
def test_scan_frames_match_the_reference_loop(gpu, fx, name, trc):
    case = tr.scan_case(name)
    o = sfr.opts(case)
    w, h = case[1], case[2]
    images = fx[f"scan_{name}_images"]
    ref, lin = fx[f"scan_{name}_{trc}_frames"], fx[f"scan_{name}_linear"]
    frames, par, dsum = scan_run(gpu, case, images, trc)
    frames0, par0, dsum0 = scan_run(gpu, case, images, 0)
    assert frames.shape == ref.shape
    # the right-hand panels are never encoded: the fixture's, and the same run's without a transfer characteristic, bit for bit
    if o["v"]:
        diff = int((frames[..., w:].view(np.int32) != ref[..., w:].view(np.int32)).sum())
        print(name, trc, "right-hand panel floats that differ from the fixture:", diff, "of", frames[..., w:].size)
        assert np.array_equal(frames[..., w:].view(np.int32), frames0[..., w:].view(np.int32))
        assert np.array_equal(ref[..., w:].view(np.int32), lin[..., w:].view(np.int32))
        assert diff == 0
    # the left-hand panels: the fixture's within 1 float ulp, its NaNs (-M of an all-zero image) where it has them
    left, rleft = frames[..., :w], ref[..., :w]
    nan = np.isnan(rleft)
    assert np.array_equal(np.isnan(left), nan)
    assert nan.any() == (name == "zero_M")
    worst = int(tr.ulps(left[~nan], rleft[~nan]).max())
    print(name, trc, "left-hand panels: largest distance from the fixture", worst, "ulp")
    assert worst <= 1
    # without a transfer characteristic the linear values are the fixture's own (the images are its stub inverse's)
    assert np.array_equal(frames0[..., :w][~nan].view(np.int32), lin[..., :w][~nan].view(np.int32))
    # the sum, -P and -M stay on linear values
    assert dsum.tobytes() == dsum0.tobytes() and par == par0
    pfx = int(fx[f"scan_{name}_parity"][0])
    assert par == (None if pfx < 0 else pfx)


def test_scan_frames_trc_zero_is_the_object_never_told(gpu, fx):
    for name in ("zigzag_P8_all", "iradial_vi_offset_invert"):
        case = tr.scan_case(name)
        a = scan_run(gpu, case, fx[f"scan_{name}_images"], 0, call_set_trc=True)
        b = scan_run(gpu, case, fx[f"scan_{name}_images"], 0, call_set_trc=False)
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2].tobytes() == b[2].tobytes()


# ---- zoom animation ----
def _animation(torch, geom, coeffs, trc):
    from dspfun_amd.zoom import Zoom
    z = Zoom(torch, torch.zeros((geom["h"], geom["w"], 3), dtype=torch.float32, device="cuda:0"))
    z.coeffs.copy_(torch.from_numpy(np.ascontiguousarray(coeffs, dtype=np.float32)))
    anim = z.animation(geom["vw"], geom["vh"], geom["type"], trc=trc)
    anim.refresh()
    return anim


@pytest.mark.parametrize("k", tr.ZOOM_CASES)
def test_zoom_frames_match_the_reference_loop(gpu, fx, k):
    geom, present, table, coeffs, _, kept = zr.cases()[k]
    ref, lin = fx[f"zoom_{k}_frames"], fx[f"zoom_{k}_linear"]
    assert list(fx[f"zoom_{k}_kept"]) == kept
    anim = _animation(gpu, geom, coeffs, "iec61966-2-1")
    args = (table, present, geom["vx"], geom["vy"], geom["xscale"], geom["yscale"])
    got = {d: f.cpu().numpy() for d, f in anim.frames(*args, showsamples=geom["show"], layout="gbr")}
    rgb = {d: f.cpu().numpy() for d, f in anim.frames(*args, showsamples=geom["show"], layout="rgb")}
    assert sorted(got) == kept
    from dspfun_amd import trc_apply
    one = F32(tr.exact(13, 0, np.array([1.0]))[0])
    dev = trc_apply(gpu.tensor([0.0, 1.0, 0.0], dtype=gpu.float32, device="cuda"), 13).cpu().numpy()      # the device's encode((0, 1, 0)): R, G, B
    assert dev[0] == 0 and dev[2] == 0 and tr.ulps(dev[1:2], np.array([one]))[0] <= 1
    painted = 0
    for j, d in enumerate(kept):
        # the linear bar of tests/test_zoom_anim_gpu.py, 1e-5 max|ref|, widened by the encode's largest slope
        err = np.abs(got[d] - ref[j]).max()
        print(k, d, "error", err, "of", 1e-5 * 12.92 * np.abs(ref[j]).max())
        assert err <= 1e-5 * 12.92 * np.abs(ref[j]).max(), (k, d)
        assert got[d].tobytes() == zr.to_gbr(rgb[d]).tobytes(), (k, d)
        # the marker went through the encode like any sample: encode((0, 1, 0)) at the fixture's positions (planes G, B, R)
        L = lin[j].reshape(3, -1)
        marked = (L[0] == 1) & (L[1] == 0) & (L[2] == 0)
        g = got[d].reshape(3, -1)
        green = (g[0] == dev[1]) & (g[1] == dev[2]) & (g[2] == dev[0])
        assert np.array_equal(green, marked), (k, d)
        r = ref[j].reshape(3, -1)
        assert np.all(r[0][marked] == one) and np.all(r[1][marked] == 0) and np.all(r[2][marked] == 0)
        painted += int(marked.sum())
    assert (painted > 0) == bool(geom["show"])


def test_zoom_trc_zero_is_the_object_never_told(gpu):
    geom, present, table, coeffs, _, kept = zr.cases()[11]
    args = (table, present, geom["vx"], geom["vy"], geom["xscale"], geom["yscale"])
    a, b = _animation(gpu, geom, coeffs, 0), _animation(gpu, geom, coeffs, "iec61966-2-1")
    b.set_trc(0)
    from dspfun_amd.zoom import Zoom
    z = Zoom(gpu, gpu.zeros((geom["h"], geom["w"], 3), dtype=gpu.float32, device="cuda:0"))
    z.coeffs.copy_(gpu.from_numpy(np.ascontiguousarray(coeffs, dtype=np.float32)))
    c = z.animation(geom["vw"], geom["vh"], geom["type"])
    c.refresh()
    for layout in ("gbr", "rgb"):
        fa, fb, fc = ([f.cpu().numpy().tobytes() for _, f in an.frames(*args, showsamples=geom["show"], layout=layout)] for an in (a, b, c))
        assert fa == fb == fc
    # and encoding the plain frame afterwards is what the object does in its last pass
    from dspfun_amd import trc_apply
    b.set_trc(13)
    for (_, plain), (_, enc) in zip(a.frames(*args, showsamples=geom["show"], layout="rgb"), b.frames(*args, showsamples=geom["show"], layout="rgb")):
        assert gpu.equal(trc_apply(plain, 13).view(gpu.int32), enc.view(gpu.int32))


# ---- motion --linear ----
@pytest.mark.parametrize("trc", tr.MOTION_TRCS)
def test_motion_linear_load_and_store(gpu, fx, trc):
    from dspfun_amd.engine import motion_load_f32_linear, motion_store_f32_linear
    torch = gpu
    (d, h, w), (md, mh, mw) = tr.MOTION_BLOCK, tr.MOTION_MINBUF
    pix, co = tr.motion_inputs()
    assert pix.min() < 0 and pix.max() > 1
    sf, nm = tr.motion_scales()
    block = np.zeros((md, mh, mw), dtype=bool)
    block[:d, :h, :w] = True
    block = block.ravel()
    d_pix, d_co = torch.from_numpy(pix).cuda(), torch.from_numpy(co).cuda()
    out = torch.full((pix.size,), -77.0, dtype=torch.float32, device="cuda")
    assert motion_load_f32_linear(out, d_pix, (d, h, w), (mh, mw), trc=trc) == 0
    got, want = out.cpu().numpy(), fx[f"motion_{trc}_load"]
    worst = int(tr.ulps(got[block], want[block]).max())
    print("motion load, trc", trc, "largest distance", worst, "ulp")
    assert worst <= 1 and np.all(got[~block] == -77.0)
    out.fill_(-77.0)
    assert motion_store_f32_linear(out, d_co, (d, h, w), (mh, mw), sf, nm, trc=tr.TABLE[trc][0]) == 0
    got, want = out.cpu().numpy(), fx[f"motion_{trc}_store"]
    assert co.min() < 0 and want[block].max() > 1             # (what leaves the encode below 0 depends on the function: 0, or the odd branch)
    worst = int(tr.ulps(got[block], want[block]).max())
    print("motion store, trc", trc, "largest distance", worst, "ulp")
    assert worst <= 1 and np.all(got[~block] == -77.0)
    copy = torch.full((pix.size,), -77.0, dtype=torch.float32, device="cuda")
    assert motion_store_f32_linear(copy, d_co, (d, h, w), (mh, mw), sf, nm, trc=trc, spec_mode="copy") == 0       # motion.c:765-769: copy stores alike
    assert torch.equal(copy.view(torch.int32), out.view(torch.int32))


def test_motion_linear_other_modes_write_nothing(gpu):
    from dspfun_amd.engine import motion_load_f32_linear, motion_store_f32_linear
    torch = gpu
    (d, h, w), (md, mh, mw) = tr.MOTION_BLOCK, tr.MOTION_MINBUF
    src = torch.full((md * mh * mw,), 0.5, dtype=torch.float32, device="cuda")
    out = torch.full((md * mh * mw,), -77.0, dtype=torch.float32, device="cuda")
    for mode in ("shift", "flat", "copy", 1):
        assert motion_load_f32_linear(out, src, (d, h, w), (mh, mw), trc=13, ispec_mode=mode) == -1
    for mode in ("abs", "shift", "flat", 2):
        assert motion_store_f32_linear(out, src, (d, h, w), (mh, mw), 1.0, 1.0, trc=13, spec_mode=mode) == -1
    assert motion_store_f32_linear(out, src, (d, h, w), (mh, mw), 1.0, 1.0, trc=0) == -1                          # no function given
    torch.cuda.synchronize()
    assert torch.all(out == -77.0).item()


# ---- the tools ----
def _pf(path, w, h, seed):
    x = ol.synth_f32(seed, w * h * 3)
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(x.tobytes())
    return x


def _read_pf(path, w, h):
    raw = open(path, "rb").read()
    head = b"PF\n%d %d\n-1.0\n" % (w, h)
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], dtype=np.float32)


def test_scan_dev_trc_video(gpu, tmp_path):
    """scan_dev --trc iec61966-2-1 --video on a 12 x 8 input: byte for byte the frames of the Python path with trc_apply(inverse) and trc="""
    torch = gpu
    from dspfun_amd import Plan, REDFT10, REDFT01, ScanFrames, trc_apply, _lib
    L = _lib.load()
    w, h, step = 12, 8, 10
    pix = _pf(str(tmp_path / "in.pf"), w, h, 0x7C11)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "scan_dev"])
    r = subprocess.run([os.path.join(ROOT, "host", "scan_dev"), "in.pf", "out.pf", str(step), "zigzag", "-v", "-i", "-M", "-P", "--trc", "iec61966-2-1",
                        "--video", "v.raw"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    npix, n = w * h, w * h * 3
    nframes = (npix + step - 1) // step
    fw, fh = 2 * w, 2 * h
    got = np.fromfile(str(tmp_path / "v.raw"), dtype="<f4").reshape(nframes, 3, fh, fw)
    d_orig = trc_apply(torch.from_numpy(pix.copy()).cuda(), "iec61966-2-1", inverse=True)
    d_co = d_orig.clone()
    Plan.image(h, w, 3, REDFT10).set_scale(1.0 / (4.0 * w * h)).execute(d_co.data_ptr())
    owner = torch.empty(npix, dtype=torch.int32, device="cuda")
    assert L.dspfft_scan_owner_index(owner.data_ptr(), 2, w, h, None) == 0
    ids = torch.empty(npix, dtype=torch.int32, device="cuda")
    assert L.dspfft_scan_frame_ids(ids.data_ptr(), 2, w, h, step, None) == 0
    inv = Plan.image(h, w, 3, REDFT01)
    sf = ScanFrames(w, h, visualize=True, intermediates=True, max_intermediates=True, parity_depth=32, trc="iec61966-2-1")
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
    assert want in r.stderr, r.stderr
    assert _read_pf(str(tmp_path / "out.pf"), w, h).tobytes() == trc_apply(d_sum, 13).cpu().numpy().tobytes()


def test_zoom_dev_trc_video(gpu, tmp_path):
    """zoom_dev --trc iec61966-2-1 --video on a 40 x 24 input: byte for byte ZoomAnimation's GBR frames over the decoded image"""
    torch = gpu
    from dspfun_amd import trc_apply
    from dspfun_amd.zoom import Zoom
    w, h, vw, vh = 40, 24, 72, 50
    x = _pf(str(tmp_path / "in.pf"), w, h, 0x7C12).reshape(h, w, 3)
    nan = float("nan")
    rows = [[1.5, 2.0, nan, 1.75, nan], [3.0, 1.0, nan, 2.5, nan], [4.0, 3.0, nan, 0.5, nan], [0.0, 0.0, nan, 2.0, nan]]
    with open(tmp_path / "p.txt", "w") as f:
        for r in rows:
            f.write(" ".join(repr(v) for v in r[:2]) + " - " + repr(r[3]) + " -\n")
    present = (1, 1, 0, 1, 0)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "zoom_dev"])
    r = subprocess.run([os.path.join(ROOT, "host", "zoom_dev"), "-s", "1.5x2", "-v", f"{vw}x{vh}", "-p", "0.5x0.25", "--basis", "centered",
                        "--showsamples=grid", "-n", str(len(rows)), "--params", "p.txt", "--trc", "iec61966-2-1", "--video", "v.raw", "in.pf", "out.pf"],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    z = Zoom(torch, trc_apply(torch.from_numpy(x.copy()).to("cuda:0"), "iec61966-2-1", inverse=True))
    anim = z.animation(vw, vh, 1, trc="iec61966-2-1")
    frames = [f.cpu().numpy() for _, f in anim.frames(np.array(rows), present, 0.5, 0.25, (1.5, 1.0), (2.0, 1.0), showsamples=2, layout="gbr")]
    assert len(frames) == len(rows)
    vid = np.fromfile(tmp_path / "v.raw", dtype=np.float32)
    assert vid.tobytes() == b"".join(f.tobytes() for f in frames)
    last = _read_pf(str(tmp_path / "out.pf"), vw, vh).reshape(vh, vw, 3)
    assert zr.to_gbr(last).tobytes() == frames[-1].tobytes()
    # without --video the output comes from the interleaved frame, encoded in place
    r = subprocess.run([os.path.join(ROOT, "host", "zoom_dev"), "-s", "1.5x2", "-v", f"{vw}x{vh}", "-p", "0.5x0.25", "--basis", "centered",
                        "--showsamples=grid", "--trc", "iec61966-2-1", "in.pf", "one.pf"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    one = anim.frame((1.5, 1.0), (2.0, 1.0), 0.5, 0.25, 2, "rgb").cpu().numpy()
    assert _read_pf(str(tmp_path / "one.pf"), vw, vh).tobytes() == one.tobytes()
