"""GPU (-m gpu): zoom's animation loop on the device (dspfft_zoomanim_*, Zoom.animation, zoom/zoom.c:320-410) against the reference's own
loop (tests/golden/ref_zoom_anim.npz: every basis, zoom-in through 1x, downscale, independent X / Y, pans, skipped frames, --showsamples
point and grid), the fixed-scale chirp-z object bit for bit, the f64 product at BASELINE config 3's size, and the memory it leaves."""
import ctypes as C

import numpy as np
import pytest

import zoom_anim_ref as zr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from dspfun_amd import _lib
    _lib.load()
    return torch


def animation(torch, geom, coeffs):
    """Zoom.animation over the fixture's coefficients (the forward transform of a placeholder image, then overwritten)"""
    from dspfun_amd.zoom import Zoom
    z = Zoom(torch, torch.zeros((geom["h"], geom["w"], 3), dtype=torch.float32, device="cuda:0"))
    z.coeffs.copy_(torch.from_numpy(np.ascontiguousarray(coeffs, dtype=np.float32)))
    return z, z.animation(geom["vw"], geom["vh"], geom["type"])


@pytest.mark.parametrize("k", range(len(zr.cases())))
def test_frames_match_the_reference(gpu, k):
    geom, present, table, coeffs, frames, kept = zr.cases()[k]
    _, anim = animation(gpu, geom, coeffs)
    anim.refresh()
    args = (table, present, geom["vx"], geom["vy"], geom["xscale"], geom["yscale"])
    got = {d: f.cpu().numpy() for d, f in anim.frames(*args, showsamples=geom["show"], layout="gbr")}
    rgb = {d: f.cpu().numpy() for d, f in anim.frames(*args, showsamples=geom["show"], layout="rgb")}
    assert sorted(got) == kept
    painted = 0
    for j, d in enumerate(kept):
        ref = frames[j]
        err = np.abs(got[d] - ref).max()
        assert err < 1e-5 * np.abs(ref).max(), (k, d, err / np.abs(ref).max())
        assert got[d].tobytes() == zr.to_gbr(rgb[d]).tobytes(), (k, d)          # the planar store is the interleaved frame permuted
        if geom["show"]:
            g = got[d].reshape(3, -1)
            green = (g[0] == 1) & (g[1] == 0) & (g[2] == 0)
            ref_green = (ref.reshape(3, -1)[0] == 1) & (ref.reshape(3, -1)[1] == 0) & (ref.reshape(3, -1)[2] == 0)
            assert np.array_equal(green, ref_green), (k, d)        # (none below 1x: zoom.c:378 needs both scales > 1)
            painted += int(green.sum())
    assert painted > 0 or not geom["show"]


def test_upscale_frames_equal_a_fresh_chirp_z_object(gpu):
    from test_zoom_czt_gpu import zoomczt
    n = 0
    for geom, present, table, coeffs, _, _ in zr.cases():
        if geom["show"]:
            continue
        _, anim = animation(gpu, geom, coeffs)
        from dspfun_amd.zoom import resolve_frames
        for d, xs, ys, vx, vy in resolve_frames(table, present, geom["vx"], geom["vy"], geom["xscale"], geom["yscale"]):
            if zr.ncomponents(geom["type"], *xs, geom["w"]) < geom["w"] or zr.ncomponents(geom["type"], *ys, geom["h"]) < geom["h"]:
                continue
            rc, want = zoomczt(gpu, coeffs, geom["type"], xs[0], xs[1], ys[0], ys[1], vx, vy, geom["vw"], geom["vh"])
            assert rc == 0
            got = anim.frame(xs, ys, vx, vy).cpu().numpy()
            assert got.tobytes() == want.tobytes(), (geom, d)
            n += 1
    assert n >= 20


def test_cztrows_execute_n_at_full_extent_is_execute(gpu):
    from dspfun_amd import _lib
    L = _lib.load()
    torch = gpu
    src = torch.randn((3 * 40, 700), dtype=torch.float32, device="cuda:0")
    outs = []
    for n in (False, True):
        dst = torch.zeros((3 * 40, 1900), dtype=torch.float32, device="cuda:0")
        p = C.c_void_p()
        assert L.dspfft_cztrows_create(C.byref(p), 700, 1900, 120, 3) == 0
        a = (src.data_ptr(), 2100, 700, 1, dst.data_ptr(), 5700, 1900, 1, 0.0031, 0.4, 0.25, None)
        rc = L.dspfft_cztrows_execute_n(p, 700, 120, *a) if n else L.dspfft_cztrows_execute(p, *a)
        torch.cuda.synchronize()
        L.dspfft_cztrows_destroy(p)
        assert rc == 0
        outs.append(dst.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()


def test_hundred_frames_allocate_nothing(gpu):
    torch = gpu
    from dspfun_amd.zoom import Zoom
    x = torch.rand((270, 480, 3), dtype=torch.float32, device="cuda:0")
    z = Zoom(torch, x)
    anim = z.animation(960, 540, 1)
    out = torch.empty((3, 540, 960), dtype=torch.float32, device="cuda:0")
    anim.frame((1.0, 1.0), (1.0, 1.0), 0.0, 0.0, 2, "gbr", out=out)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for i in range(100):
        s = 0.6 + 0.03 * i
        anim.frame((s, 1.0), (s * 1.01, 1.0), 0.37 * i, 0.21 * i, i % 3, "gbr", out=out)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("btype", [0, 1])
def test_config3_geometry_against_the_f64_product(gpu, btype):
    """1920x1080 -> 7680x4320 views at per-frame scales around 4, one object"""
    from test_zoom_c3_tolerance_gpu import reference_frame
    import oracle_lib as ol
    from dspfun_amd.zoom import Zoom
    torch = gpu
    x = ol.synth_f32(0xD5F2B01, 1080 * 1920 * 3).reshape(1080, 1920, 3)
    z = Zoom(torch, torch.from_numpy(x).to("cuda:0"))
    anim = z.animation(7680, 4320, btype)
    for s, vx, vy in ((3.9, 10.5, 20.25), (4.1, 0.0, 0.0)):
        got = anim.frame((s, 1.0), (s, 1.0), vx, vy)
        ref = reference_frame(torch, x, btype, s, vx, vy, 7680, 4320)
        rows = torch.arange(0, 4320, 37, device="cuda:0")
        err = float((got[rows].double() - ref[rows]).abs().max())
        assert err < 1e-5 * float(ref.abs().max()), (btype, s, err)
        del ref
        torch.cuda.empty_cache()


def test_zoom_dev_video_equals_the_python_frames(gpu, tmp_path):
    """host/zoom_dev --params ... --video: n_kept * vw * vh * 3 floats, byte for byte ZoomAnimation.frames' GBR frames; the .pf is the last
    frame interleaved"""
    import os
    import subprocess
    torch = gpu
    from dspfun_amd.zoom import Zoom
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w, h, vw, vh = 40, 24, 72, 50
    x = np.random.default_rng(11).random((h, w, 3), dtype=np.float32)
    with open(tmp_path / "in.pf", "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(x.tobytes())
    nan = float("nan")
    rows = [[1.5, 2.0, nan, 1.75, nan], [3.0, 1.0, nan, 2.5, nan], [nan, 0.5, nan, 3.25, nan], [2.0, 0.0, nan, float("inf"), nan],
            [4.0, 3.0, nan, 0.5, nan], [0.0, 0.0, nan, 2.0, nan]]
    with open(tmp_path / "p.txt", "w") as f:
        for r in rows:
            f.write(" ".join(repr(v) for v in r[:2]) + " - " + repr(r[3]) + " -\n")
    present = (1, 1, 0, 1, 0)
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "host"), "zoom_dev"])
    r = subprocess.run([os.path.join(root, "host", "zoom_dev"), "-s", "1.5x2", "-v", f"{vw}x{vh}", "-p", "0.5x0.25", "--basis", "centered",
                        "--showsamples=grid", "-n", str(len(rows)), "--params", "p.txt", "--video", "v.raw", "in.pf", "out.pf"],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert "Skipping non-finite expression result at frame 2" in r.stderr and "at frame 3" in r.stderr
    z = Zoom(torch, torch.from_numpy(x).to("cuda:0"))
    anim = z.animation(vw, vh, 1)
    frames = [(d, f.cpu().numpy()) for d, f in anim.frames(np.array(rows), present, 0.5, 0.25, (1.5, 1.0), (2.0, 1.0), showsamples=2, layout="gbr")]
    assert [d for d, _ in frames] == [0, 1, 4, 5]
    vid = np.fromfile(tmp_path / "v.raw", dtype=np.float32)
    assert vid.size == len(frames) * vw * vh * 3
    assert vid.tobytes() == b"".join(f.tobytes() for _, f in frames)
    raw = open(tmp_path / "out.pf", "rb").read()
    head = b"PF\n%d %d\n-1.0\n" % (vw, vh)
    assert raw.startswith(head)
    last = np.frombuffer(raw[len(head):], dtype=np.float32).reshape(vh, vw, 3)
    assert zr.to_gbr(last).tobytes() == frames[-1][1].tobytes()
    assert (frames[0][1][0] == 1).any()                # the grid is drawn (G plane)
