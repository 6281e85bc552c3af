"""Regenerates tests/golden/ref_lib.npz from the reference's OWN include/speclib.c, scan/scan_precomputed.c and scan/scan_context.c,
compiled where they lie into oracle/_ref/libdspfun_ref.so by `make -C oracle` (COEFF_PRECISION=F / INTERMEDIATE_PRECISION=D).  Build
container only (needs the reference tree at generation time); the tests read the numbers alone.

  norm                          spec_normalization_pcfi(n), n = 0..7                      (speclib.c:79-85)
  c_cpu0, c_cpu1                the coefficient sets tests/test_ref_speclib.py encodes, one per range (f32, stored as inputs)
  cpu_<scale>_<sign>_<r>_scale  spec_scale_pcfi of each coefficient of c_cpu<r>, range r  (speclib.c:163-170)
  cpu_<scale>_<sign>_<r>_unscale  spec_unscale of the f32 rounding of that encoding      (speclib.c:172-178)
  scanfile_<method>_<w>x<h>_<fmt>_{intervals,yx}   scan_precomputed_unserialize of the `file` method's input that host/scan_orders.c
                                serialises for tests/test_scan_orders_cpu.py (coordinate / index plaintext)
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as ol  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(HERE))
SCAN_METHODS = ["horizontal", "vertical", "zigzag", "row", "column", "diagonal", "mirror", "box", "ibox", "radial", "iradial"]
SCAN_FILES = [("diagonal", 8, 8), ("box", 16, 9), ("ibox", 9, 16), ("mirror", 7, 5), ("zigzag", 6, 4), ("radial", 10, 6)]
SCALES = ["log", "linear"]
SIGNS = ["abs", "shift", "saturate"]


class Precomputed(C.Structure):          # scan/scan_precomputed.h:12-16
    _fields_ = [("limit", C.c_size_t), ("intervals", C.POINTER(C.c_size_t)), ("scans", C.POINTER(C.POINTER(C.c_size_t * 2)))]


class SpecParams(C.Structure):
    _fields_ = [("scaletype", C.c_int), ("signtype", C.c_int)]       # include/speclib.h:24-27


def coefficients(seed, h, w, d=3):
    """uniform-range DCT coefficients of a synthetic image (what spec.c:78 / scan.c:400 hand to the scaler): |c| <= 1, c[0,0] = mean"""
    x = ol.synth_f32(seed, h * w * d).reshape(h, w, d)
    f = np.ascontiguousarray(ol.dct2d_interleaved(x.astype(np.float64), ol.REDFT10))
    ol.lib().oracle_spec_normalise_f64(f.ctypes.data, w, h, d)
    return f.astype(np.float32)


def main():
    subprocess.check_call(["make", "-s", "-C", ol.ORACLE_DIR])
    r = ol.ref()
    if r is None:
        sys.exit("oracle/_ref/libdspfun_ref.so not built: the reference tree is needed to regenerate this fixture")
    r.spec_normalization_pcfi.restype = C.c_double
    r.spec_normalization_pcfi.argtypes = [C.c_size_t]
    r.spec_create_pcfi.restype = C.c_void_p
    r.spec_create_pcfi.argtypes = [C.POINTER(SpecParams), C.c_float, C.c_float]
    r.spec_scale_pcfi.restype = C.c_double
    r.spec_scale_pcfi.argtypes = [C.c_void_p, C.c_double]
    r.spec_unscale.restype = C.c_double
    r.spec_unscale.argtypes = [C.c_void_p, C.c_double]
    r.spec_destroy.argtypes = [C.c_void_p]
    r.spec_param_parse.restype = C.c_char_p
    r.spec_param_parse.argtypes = [C.POINTER(SpecParams), C.c_char_p, C.c_char_p]

    out = {"norm": np.array([r.spec_normalization_pcfi(n) for n in range(8)])}
    for rangetype in (0, 1):
        c = out[f"c_cpu{rangetype}"] = coefficients(11 + rangetype, 9, 16)
        h, w, _ = c.shape
        gain = np.float32(127.5 * np.sqrt(4.0 * w * h))
        mx = np.float32(1.0) if rangetype == 0 else np.float32(c[0, 0].max())
        for scale in SCALES:
            for sign in SIGNS:
                p = SpecParams(0, 0)
                assert r.spec_param_parse(C.byref(p), b"scale", scale.encode()) is None
                assert r.spec_param_parse(C.byref(p), b"sign", sign.encode()) is None
                sp = r.spec_create_pcfi(C.byref(p), mx, gain)
                assert sp
                enc = np.array([r.spec_scale_pcfi(sp, float(v)) for v in c.ravel()]).reshape(c.shape)
                dec = np.array([r.spec_unscale(sp, float(v)) for v in enc.astype(np.float32).ravel()]).reshape(c.shape)
                r.spec_destroy(sp)
                out[f"cpu_{scale}_{sign}_{rangetype}_scale"] = enc
                out[f"cpu_{scale}_{sign}_{rangetype}_unscale"] = dec
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "libscanorders.so"])
    so = C.CDLL(os.path.join(ROOT, "host", "libscanorders.so"))
    so.scan_order_serialize_coordinate.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_void_p]
    so.scan_order_serialize_index.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_void_p]
    r.scan_precomputed_unserialize.restype = C.POINTER(Precomputed)
    r.scan_precomputed_unserialize.argtypes = [C.c_void_p]
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    with tempfile.TemporaryDirectory() as tmp:
        for method, w, h in SCAN_FILES:
            for fmt in ("coordinate", "index"):
                if method == "box" and fmt == "index":
                    continue                         # the test skips it: box's shared pixels do not survive an index grid
                path = os.path.join(tmp, f"{method}_{fmt}.txt")
                f = libc.fopen(path.encode(), b"w")
                assert getattr(so, "scan_order_serialize_" + fmt)(SCAN_METHODS.index(method), w, h, f) == 0
                libc.fclose(f)
                f = libc.fopen(path.encode(), b"r")
                p = r.scan_precomputed_unserialize(f)
                libc.fclose(f)
                assert p
                iv = [p.contents.intervals[i] for i in range(p.contents.limit)]
                yx = [(p.contents.scans[i][j][0], p.contents.scans[i][j][1]) for i in range(len(iv)) for j in range(iv[i])]
                out[f"scanfile_{method}_{w}x{h}_{fmt}_intervals"] = np.array(iv, dtype=np.int64)
                out[f"scanfile_{method}_{w}x{h}_{fmt}_yx"] = np.array(yx, dtype=np.int64).reshape(-1, 2)
    path = os.path.join(HERE, "ref_lib.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
