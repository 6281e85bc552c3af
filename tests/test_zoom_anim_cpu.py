"""CPU (-m "not gpu"): zoom's animation loop (dspfft_zoomanim_*, zoom/zoom.c:320-410) through the test-only emulation of the kernel phases:
sub-extent chirp-z rows (dspfft_cztrows_execute_n) against the float64 series with NaN past the active extent, the plain frame loop against
tests/golden/ref_zoom_anim.npz (the reference's own loop), the per-frame state resolution, the --showsamples rule of zoom_anim_core.h against
the reference's pixels, and dist.FrameShardedZoom in gloo worlds against one rank."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import zoom_anim_ref as zr
from emul_lib import emul
from test_cztrows_cpu import series, axis

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("pnc,nout,plines,group,nc,lines", [
    (300, 850, 12, 1, 300, 12),      # full extents
    (300, 850, 12, 1, 171, 12),
    (300, 850, 12, 1, 300, 5),
    (300, 850, 12, 3, 64, 6),        # channel groups, fewer of them
    (640, 1700, 9, 3, 1, 3),         # the constant term alone
])
def test_cztrows_sub_extent_reads_nothing_past_it(pnc, nout, plines, group, nc, lines):
    L = emul()
    rng = np.random.default_rng(pnc + nc + lines)
    src = np.full((plines, pnc), np.nan, dtype=np.float32)          # poison: everything outside the active extent
    src[:lines, :nc] = rng.standard_normal((lines, nc)).astype(np.float32)
    dst = np.full((plines, nout), np.float32(-77))
    omega, phi = axis(1, 2.83, 1.0, nc if nc > 1 else 2, 4.25)
    p = C.c_void_p()
    assert L.dspfft_cztrows_create(C.byref(p), pnc, nout, plines, group) == 0, L.dspfft_last_error()
    try:
        # lines (g, m) at g * group * pnc + m * pnc: a plain stack of lines whatever the group
        assert L.dspfft_cztrows_execute_n(p, nc, lines, src.ctypes.data, group * pnc, pnc, 1, dst.ctypes.data, group * nout, nout, 1,
                                          omega, phi, 0.5, None) == 0, L.dspfft_last_error()
        for bad in ((pnc + 1, lines), (nc, plines + group), (0, lines), (nc, 0)) + (((nc, lines - 1),) if group > 1 else ()):
            assert L.dspfft_cztrows_execute_n(p, *bad, src.ctypes.data, group * pnc, pnc, 1, dst.ctypes.data, group * nout, nout, 1,
                                              omega, phi, 0.5, None) == -1
    finally:
        L.dspfft_cztrows_destroy(p)
    want = series(src[:lines, :nc].astype(np.float64), nout, omega, phi, 0.5)
    assert np.all(np.isfinite(dst[:lines]))
    assert np.abs(dst[:lines] - want).max() < 2e-5 * max(1.0, np.abs(want).max())
    assert np.all(dst[lines:] == np.float32(-77))


def test_cztrows_execute_is_the_full_extent_call():
    L = emul()
    rng = np.random.default_rng(5)
    src = rng.standard_normal((6, 200)).astype(np.float32)
    outs = []
    for n in (False, True):
        dst = np.zeros((6, 500), dtype=np.float32)
        p = C.c_void_p()
        assert L.dspfft_cztrows_create(C.byref(p), 200, 500, 6, 3) == 0
        if n:
            rc = L.dspfft_cztrows_execute_n(p, 200, 6, src.ctypes.data, 600, 200, 1, dst.ctypes.data, 1500, 500, 1, 0.01, 0.02, 1.0, None)
        else:
            rc = L.dspfft_cztrows_execute(p, src.ctypes.data, 600, 200, 1, dst.ctypes.data, 1500, 500, 1, 0.01, 0.02, 1.0, None)
        L.dspfft_cztrows_destroy(p)
        assert rc == 0
        outs.append(dst)
    assert outs[0].tobytes() == outs[1].tobytes()


def emul_frames(geom, present, table, coeffs, layout=0, showsamples=0):
    """the resolved frames through the emulation's dspfft_zoomanim_*: {d: frame (vh, vw, 3)}, or the first nonzero return code"""
    from dspfun_amd.zoom import resolve_frames
    L = emul()
    z = C.c_void_p()
    rc = L.dspfft_zoomanim_create(C.byref(z), geom["w"], geom["h"], geom["type"], geom["vw"], geom["vh"])
    assert rc == 0, L.dspfft_zoomanim_last_error()
    out = {}
    try:
        c = np.array(coeffs, dtype=np.float32, order="C")            # a copy: it is poisoned below
        work = np.zeros(L.dspfft_zoomanim_work_floats(z), dtype=np.float32)
        assert L.dspfft_zoomanim_set_coeffs(z, c.ctypes.data, None) == 0
        c[:] = np.nan                      # the object holds its own transpose
        for d, xs, ys, vx, vy in resolve_frames(table, present, geom["vx"], geom["vy"], geom["xscale"], geom["yscale"]):
            f = np.full((geom["vh"], geom["vw"], 3), np.float32(-77))
            rc = L.dspfft_zoomanim_execute(z, xs[0], xs[1], ys[0], ys[1], vx, vy, showsamples, layout, f.ctypes.data, work.ctypes.data, None)
            if rc:
                return rc
            out[d] = f
    finally:
        L.dspfft_zoomanim_destroy(z)
    return out


@pytest.mark.parametrize("k", range(len(zr.cases())))
def test_plain_loop_matches_the_reference(k):
    geom, present, table, coeffs, frames, kept = zr.cases()[k]
    got = emul_frames(geom, present, table, coeffs)
    assert sorted(got) == kept
    for j, d in enumerate(kept):
        ref = frames[j]
        tol = 1e-5 * np.abs(ref).max()
        g = zr.to_gbr(got[d])
        if geom["show"]:              # the emulation has no overlay: compare off the reference's marked pixels
            keep = ~zr.core_mask(geom["show"], *_frame_state(geom, present, table, d), geom["vw"], geom["vh"]).reshape(geom["vh"], geom["vw"])
            assert np.abs(g - ref)[:, keep].max() < tol, (k, d)
        else:
            assert np.abs(g - ref).max() < tol, (k, d, np.abs(g - ref).max() / np.abs(ref).max())


def _frame_state(geom, present, table, d):
    from dspfun_amd.zoom import resolve_frames
    for dd, xs, ys, vx, vy in resolve_frames(table, present, geom["vx"], geom["vy"], geom["xscale"], geom["yscale"]):
        if dd == d:
            return xs, ys, vx, vy
    raise KeyError(d)


def test_overlay_and_planar_store_are_not_in_the_emulation():
    geom, present, table, coeffs, _, _ = zr.cases()[0]
    for layout, show in ((1, 0), (0, 1), (0, 2)):
        assert emul_frames(geom, present, table, coeffs, layout, show) == -3
    assert "not in this build" in emul().dspfft_zoomanim_last_error().decode()


def test_state_resolution_keeps_the_reference_frames():
    from dspfun_amd.zoom import resolve_frames
    for geom, present, table, _, _, kept in zr.cases():
        assert [f[0] for f in resolve_frames(table, present, geom["vx"], geom["vy"], geom["xscale"], geom["yscale"])] == kept


def test_state_resolution_order():
    """S sets both scales, X / Y override one axis, absent columns keep the state, a skipped frame's values persist"""
    from dspfun_amd.zoom import resolve_frames
    nan = float("nan")
    t = [[1.0, 2.0, 3.0, 4.0, nan], [nan, 5.0, nan, 6.0, nan], [7.0, 8.0, 2.0, 1.5, 2.5]]
    got = list(resolve_frames(t, (1, 1, 1, 1, 0), 0.0, 0.0, (5.0, 2.0), (7.0, 3.0)))
    assert got == [(0, (4.0, 1.0), (3.0, 1.0), 1.0, 2.0), (2, (1.5, 1.0), (2.0, 1.0), 7.0, 8.0)]
    assert list(resolve_frames([[nan] * 5] * 2, (0, 0, 0, 0, 0), 1.0, 2.0, (3.0, 2.0), (1.0, 1.0))) == [
        (0, (3.0, 2.0), (1.0, 1.0), 1.0, 2.0), (1, (3.0, 2.0), (1.0, 1.0), 1.0, 2.0)]


def test_overlay_rule_matches_the_reference_pixels():
    """zoom_anim_core.h's closed form == the loop as written == the pixels the reference painted (0, 1, 0)"""
    seen = 0
    for geom, present, table, _, frames, kept in zr.cases():
        if not geom["show"]:
            continue
        vw, vh = geom["vw"], geom["vh"]
        for j, d in enumerate(kept):
            xs, ys, vx, vy = _frame_state(geom, present, table, d)
            mask = zr.core_mask(geom["show"], xs, ys, vx, vy, vw, vh)
            loop = zr.overlay_loop(geom["show"], xs, ys, vx, vy, vw, vh)
            assert set(np.flatnonzero(mask)) == loop, (geom, d)
            g = frames[j].reshape(3, -1)
            green = (g[0] == 1) & (g[1] == 0) & (g[2] == 0)          # planes G, B, R
            assert np.array_equal(green, mask), (geom, d)
            seen += int(mask.sum())
    assert seen > 100


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("vw,vh,xs,ys,vx,vy", [
    (40, 24, (2.5, 1.0), (3.0, 1.0), 3.0, 5.0), (24, 40, (2.5, 1.0), (3.0, 1.0), 7.0, 1.0),      # vh > vw: writes past the frame dropped
    (33, 33, (7.0, 3.0), (1.01, 1.0), 0.0, 0.0), (50, 20, (4.75, 1.0), (1.9, 1.0), 123.5, 9.99), (20, 20, (0.9, 1.0), (3.0, 1.0), 0.0, 0.0),
    (64, 16, (1.5, 1.0), (1.5, 1.0), 2.0, 1.0),
])
def test_overlay_rule_matches_the_loop(mode, vw, vh, xs, ys, vx, vy):
    mask = zr.core_mask(mode, xs, ys, vx, vy, vw, vh)
    assert set(np.flatnonzero(mask)) == zr.overlay_loop(mode, xs, ys, vx, vy, vw, vh)


# ---- several ranks over gloo ----
def _anim_case():
    geom, present, table, coeffs, _, _ = zr.cases()[0]
    x = np.random.default_rng(3).standard_normal((geom["h"], geom["w"], 3)).astype(np.float32)
    return geom, present, table, x



def _sharded(lib):
    from dspfun_amd.dist import FrameShardedZoom
    geom, present, table, x = _anim_case()
    eng = FrameShardedZoom(torch.from_numpy(x.copy()), geom["vw"], geom["vh"], table, present, geom["type"], geom["vx"], geom["vy"],
                           geom["xscale"], geom["yscale"], lib=lib)
    return eng, {d: f.numpy().copy() for d, f in eng.frames()}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from emul_lib import emul as em
        eng, frames = _sharded(em())
        assert all(eng.owner(d) == rank for d in frames)
        q.put((rank, frames))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 4])
def test_gloo_worlds_match_one_rank(world):
    eng, single = _sharded(emul())
    assert sorted(single) == [f[0] for f in eng.frames_all] and len(single) == 7
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    seen = {}
    for r in range(world):
        assert got[r], (world, r)
        seen.update(got[r])
    assert sorted(seen) == sorted(single)
    for d, f in seen.items():
        assert f.tobytes() == single[d].tobytes(), (world, d)


def test_viewport_library_matches_the_reference():
    """host/libzoomargs.so's zoom_viewport (zoom.c:268-303: -r, -s, -v, -p, -%, -P, -c) equals the reference's lines compiled as they lie"""
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(HERE), "host"), "libzoomargs.so"])
    lib = C.CDLL(os.path.join(os.path.dirname(HERE), "host", "libzoomargs.so"))
    ld, sz, P = C.c_longdouble, C.c_size_t, C.POINTER
    lib.zoom_viewport.restype = None
    lib.zoom_viewport.argtypes = [sz, sz, ld, ld, P(ld), P(C.c_ulonglong), P(ld), P(C.c_ulonglong), P(sz), P(sz), P(ld), P(ld), C.c_int, C.c_int, C.c_int]
    vin, vout = zr.viewport()
    assert len(vin) == 720
    for row, want in zip(vin, vout):
        w, h, lw, lh, xn, xd, yn, yd, vw, vh, vx, vy, pct, inp, cen = row
        a = [ld(xn), C.c_ulonglong(int(xd)), ld(yn), C.c_ulonglong(int(yd)), sz(int(vw)), sz(int(vh)), ld(vx), ld(vy)]
        lib.zoom_viewport(int(w), int(h), lw, lh, *[C.byref(x) for x in a], int(pct), int(inp), int(cen))
        got = [float(x.value) for x in a]
        assert got == list(want), (row, got, list(want))


def test_non_positive_scales_clamp_as_the_reference():
    """zoom.c:37-41: a finite scale with len * scale < 1 (zero and negative included) becomes 1 / len -- the same frame as that scale"""
    geom, present, table, coeffs, _, _ = zr.cases()[0]
    w, h = geom["w"], geom["h"]
    rows = [[0.5, 0.25, s, float("nan"), float("nan")] for s in (0.0, -1.5, 1.0 / w)]
    got = emul_frames(geom, (1, 1, 1, 0, 0), np.array(rows), coeffs)
    assert sorted(got) == [0, 1, 2]
    assert got[0].tobytes() == got[1].tobytes()
    z = dict(geom, xscale=(1.0, float(w)), yscale=(1.0, float(h)))
    want = emul_frames(z, (1, 1, 0, 0, 0), np.array([[0.5, 0.25, 0, 0, 0]]), coeffs)[0]
    assert got[0].tobytes() == want.tobytes()
    assert np.all(np.isfinite(got[0]))


def _zoom_dev(args, tmp_path):
    import subprocess
    root = os.path.dirname(HERE)
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "host"), "zoom_dev"])
    return subprocess.run([os.path.join(root, "host", "zoom_dev")] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))


@pytest.mark.parametrize("opt,msg", [("-x", "--params"), ("-y", "--params"), ("-S", "--params"), ("-X", "--params"), ("-Y", "--params"),
                                     ("-g", "linear RGB")])
def test_zoom_dev_refuses_expressions_and_linear_rgb(tmp_path, opt, msg):
    r = _zoom_dev([opt] + (["t"] if opt != "-g" else []) + ["in.pf", "out.pf"], tmp_path)
    assert r.returncode == 2 and msg in r.stderr


@pytest.mark.parametrize("lines,msg", [
    (["1 2 - - -", "3 - - - -"], "mixes numbers and -"),
    (["1 2 - - -", "x 2 - - -"], "not a number"),
    (["1 2 - -"], "five columns"),
    (["1 2 - - - 7"], "more than five"),
    (["1 2 - - -"], "1 lines for 2 frames"),
])
def test_zoom_dev_params_file_rules(tmp_path, lines, msg):
    """--params is read before the device is touched: its column rules fail on a machine without one"""
    with open(tmp_path / "in.pf", "wb") as f:
        f.write(b"PF\n4 3\n-1.0\n" + np.zeros(36, dtype=np.float32).tobytes())
    (tmp_path / "p.txt").write_text("\n".join(lines) + "\n")
    r = _zoom_dev(["-n", "2", "--params", "p.txt", "in.pf", "out.pf"], tmp_path)
    assert r.returncode == 1 and msg in r.stderr, r.stderr
