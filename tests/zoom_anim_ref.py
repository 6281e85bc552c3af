"""TEST-ONLY: helpers for the zoom animation tests (dspfft_zoomanim_*, zoom/zoom.c:320-410): the fixture's cases, a restatement of
zoom.c:377-390's overlay loop in long double, and zoom_anim_core.h compiled with g++ for the closed form the device uses."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "ref_zoom_anim.npz")


def cases():
    """[(geom dict, present, table, coeffs (h, w, 3) f32, frames (k, 3, vh, vw) GBR f32, kept frame numbers)]"""
    f = np.load(FIXTURE)
    out = []
    for i in range(int(f["ncases"])):
        g = f[f"c{i}_geom"]
        geom = dict(w=int(g[0]), h=int(g[1]), type=int(g[2]), vw=int(g[3]), vh=int(g[4]), show=int(g[5]), vx=g[6], vy=g[7],
                    xscale=(g[8], g[9]), yscale=(g[10], g[11]))
        out.append((geom, tuple(int(p) for p in f[f"c{i}_present"]), f[f"c{i}_table"], f[f"c{i}_coeffs"], f[f"c{i}_frames"], list(f[f"c{i}_kept"])))
    return out


def viewport():
    f = np.load(FIXTURE)
    return f["viewport_in"], f["viewport_out"]


def overlay_loop(mode, xscale, yscale, vx, vy, vw, vh):
    """zoom.c:377-390 as written (long double scales, size_t loop variables truncated after each add): the set of linear indices
    y vh + x it writes, those >= vw vh dropped"""
    LD = np.longdouble
    xs, ys = LD(xscale[0]) / LD(xscale[1]), LD(yscale[0]) / LD(yscale[1])
    hits = set()
    if not mode or not (xs > 1 and ys > 1):
        return hits

    def start(s, v):
        return int(s - LD(int(v) % int(s)))

    def walk(p0, s, n):
        p = p0
        while p < n:
            yield p
            p = int(LD(p) + s)
    if mode == 1:
        for y in walk(start(ys, vy), ys, vh):
            for x in walk(start(xs, vx), xs, vw):
                hits.add(y * vh + x)
    else:
        for y in walk(start(ys, vy), ys, vh):
            for x in range(vw):
                hits.add(y * vh + x)
        for y in range(vh):
            for x in walk(start(xs, vx), xs, vw):
                hits.add(y * vh + x)
    return {h for h in hits if h < vw * vh}


_core = None


def core_lib():
    """zoom_anim_core.h's host scalars and per-pixel rule, built with g++ -ffp-contract=off"""
    global _core
    if _core is None:
        tmp = tempfile.mkdtemp(prefix="zoom_anim_core")
        src = os.path.join(tmp, "core.cpp")
        with open(src, "w") as f:
            f.write('#include "zoom_anim_core.h"\nusing namespace dspfft;\n'
                    'extern "C" void za_mask(int mode, double xn, double xd, double yn, double yd, double vx, double vy, int vw, int vh, unsigned char *m)\n'
                    '{ const ZaOverlay o = za_overlay(mode, xn, xd, yn, yd, vx, vy, vw, vh); for (long long i = 0; i < (long long)vw * vh; i++) m[i] = za_overlay_hit(o, i); }\n'
                    'extern "C" int za_nc(int type, double num, double den, int len, double off, double *w, double *p) { return za_axis(type, num, den, len, off, *w, *p); }\n')
        so = os.path.join(tmp, "core.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "dspfun_amd", "csrc"), src, "-o", so])
        lib = C.CDLL(so)
        lib.za_mask.argtypes = [C.c_int] + [C.c_double] * 6 + [C.c_int, C.c_int, C.c_void_p]
        lib.za_nc.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _core = lib
    return _core


def core_mask(mode, xscale, yscale, vx, vy, vw, vh):
    m = np.zeros(vw * vh, dtype=np.uint8)
    core_lib().za_mask(mode, xscale[0], xscale[1], yscale[0], yscale[1], vx, vy, vw, vh, m.ctypes.data)
    return m.astype(bool)


def ncomponents(typ, num, den, length):
    w, p = C.c_double(), C.c_double()
    return core_lib().za_nc(typ, num, den, length, 0.0, C.byref(w), C.byref(p))


def to_gbr(rgb):
    """(vh, vw, 3) -> (3, vh, vw) planes G, B, R"""
    return np.ascontiguousarray(np.transpose(rgb, (2, 0, 1))[[1, 2, 0]])
