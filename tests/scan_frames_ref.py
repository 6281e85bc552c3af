"""TEST-ONLY: scan's output frames (scan/scan.c:366-527) restated over dspfun_amd/csrc/scan_frame_core.h (tests/scan_frames_ref.cpp,
built here with g++ -ffp-contract=off), and the cases of tests/golden/ref_scan_frames.npz: geometry, options, and inputs regenerated from
recorded seeds.  Scan orders come from host/scan_orders.c (checked against the reference in tests/test_scan_orders_cpu.py); magnitude from
scan_device_checks.magnitude_reference (no qfactor: ties in order within one index do not change a frame)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import oracle_lib as ol
import scan_device_checks as sdc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32

# name, w, h, seed, method, step, offset, nframes, invert, skip, options
#   options: v s i M (flags), P (depth), gain (0: default), scale / sign (speclib names)
CASES = [
    ("zigzag_v", 12, 8, 0x5F01, "zigzag", 16, 0, 0, False, False, dict(v=1)),
    ("box_s", 16, 9, 0x5F02, "box", 2, 0, 0, False, False, dict(s=1)),
    ("ibox_s_log_shift_gain", 9, 16, 0x5F03, "ibox", 3, 0, 0, False, False, dict(s=1, scale="log", sign="shift", gain=1000.1)),
    ("column_s_linear_shift", 12, 8, 0x5F0D, "column", 3, 0, 0, False, False, dict(s=1, scale="linear", sign="shift")),
    ("radial_s_log_saturate_i", 12, 8, 0x5F04, "radial", 2, 0, 0, False, False, dict(s=1, scale="log", sign="saturate", i=1)),
    ("iradial_vi_offset_invert", 16, 9, 0x5F05, "iradial", 2, 3, 0, True, False, dict(v=1, i=1)),
    ("magnitude_vM_past_limit", 12, 8, 0x5F06, "magnitude", 8, 9, 0, False, False, dict(v=1, M=1)),
    ("file_shared_viP8_skip", 12, 8, 0x5F07, "file", 5, 2, 0, False, True, dict(v=1, i=1, P=8)),
    ("zigzag_s_abs_P32", 33, 20, 0x5F08, "zigzag", 110, 0, 0, False, False, dict(s=1, sign="abs", P=32)),
    ("zigzag_P8_all", 12, 8, 0x5F09, "zigzag", 4, 0, 0, False, False, dict(v=1, s=1, i=1, M=1, P=8)),
    ("row_s_linear_abs_invert", 16, 9, 0x5F0A, "row", 1, 0, 0, True, False, dict(s=1, scale="linear", sign="abs")),
    ("diagonal_vi_offset_invert_skip", 9, 16, 0x5F0B, "diagonal", 3, 2, 3, True, True, dict(v=1, i=1)),
    ("mirror_s_shift_i_offset", 16, 9, 0x5F0C, "mirror", 2, 3, 0, False, False, dict(s=1, sign="shift", i=1)),
]
SCALES = {"none": 0, "linear": 1, "log": 2}
SIGNS = {"none": 0, "abs": 1, "shift": 2, "saturate": 3}

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="scan_frames_ref_")
        so = os.path.join(d, "scan_frames_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "dspfun_amd", "csrc"),
                               "-I" + HERE, os.path.join(HERE, "scan_frames_ref.cpp"), "-o", so, "-lm"])
        _lib = C.CDLL(so)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        _lib.sfr_spec_values.argtypes = [u32, u32, vp, C.c_double, C.c_int, C.c_int, C.c_int, vp]
        _lib.sfr_spec_values.restype = None
        _lib.sfr_run.argtypes = [u32, u32, vp, vp, C.c_int, u64, vp, vp, u64, u64, u64] + [C.c_int] * 6 + [C.c_double, C.c_int, C.c_int, vp, vp, vp]
    return _lib


def case_inputs(case):
    """the original image (8-bit values / 255, HWC float32) and scan's normalised coefficients (REDFT10 / 4wh, float32)"""
    name, w, h, seed = case[:4]
    orig = (ol.synth_u8(seed, w * h * 3).astype(np.float64) / 255).astype(F32).reshape(h, w, 3)
    c = ol.dct2d_interleaved(orig.astype(np.float64), ol.REDFT10) / (4.0 * w * h)
    return orig, np.ascontiguousarray(c.astype(F32))


def file_order(w, h, seed):
    """a `file` order whose indices share pixels: a seeded permutation of the pixels in groups of 1..3, every third index repeating a
    pixel of the index before it"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(w * h)
    out, k = [], 0
    while k < len(perm):
        g = int(rng.integers(1, 4))
        idx = [int(p) for p in perm[k:k + g]]
        if len(out) % 3 == 2:
            idx.append(out[-1][0])
        out.append(idx)
        k += g
    return [[(p // w, p % w) for p in idx] for idx in out]


def orders(case, coeffs):
    """per scan index, the (y, x) pairs scan() yields"""
    name, w, h, seed, method = case[:5]
    if method == "magnitude":
        idx, limit = sdc.magnitude_reference(coeffs, w, h, 3, 0.0)
        out = [[] for _ in range(limit)]
        for p in range(w * h):
            out[idx[p]].append((p // w, p % w))
        return out
    if method == "file":
        return file_order(w, h, seed)
    so = sdc.host_lib()
    return sdc.host_orders(so, sdc.METHODS.index(method), w, h)


def loop_params(case, limit):
    """scan.c:346-348,385-386: (offset, nframes)"""
    step, offset, nframes = case[5], case[6], case[7]
    if not nframes or nframes > limit // step:
        nframes = (limit + step - 1) // step
    if offset >= limit:
        offset = limit - 1
    return offset, nframes


def opts(case):
    o = dict(v=0, s=0, i=0, M=0, P=0, gain=0.0, scale="none", sign="none")
    o.update(case[10])
    o["v"] = int(o["v"] or o["s"])
    o["i"] = int(o["i"] or o["M"])
    return o


def frame_shape(case):
    w, h = case[1], case[2]
    o = opts(case)
    return 3, h * (1 + o["i"]), w * (1 + o["v"])


def run(case, coeffs, original, order, images=None, gain=None):
    """the frames (nframes, 3, H', W') and the parity frame (None: not reached).  images: None (the stub inverse), or the fill's image
    (when the case fills) followed by every frame's"""
    name, w, h, seed, method, step, _o, _n, invert, skip = case[:10]
    o = opts(case)
    limit = len(order)
    offset, nframes = loop_params(case, limit)
    off = np.zeros(limit + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(c) for c in order])
    yx = np.array([p for c in order for p in c], dtype=np.uint32).reshape(-1, 2)
    if gain is None:
        gain = o["gain"] if o["gain"] else 127.5 * np.sqrt(float(w * h * 4))
    fs = frame_shape(case)
    frames = np.zeros((nframes,) + fs, dtype=F32)
    par = np.zeros(1, dtype=np.uint64)
    coeffs = np.ascontiguousarray(coeffs, dtype=F32)
    original = np.ascontiguousarray(original, dtype=F32)
    imgs = None if images is None else np.ascontiguousarray(images, dtype=F32)
    lib().sfr_run(w, h, coeffs.ctypes.data, original.ctypes.data, o["P"], limit, off.ctypes.data, yx.ctypes.data, step, offset, nframes,
                  int(invert), int(not skip and (imgs is None or offset > 0)), o["v"], o["s"], o["i"], o["M"], float(gain), SCALES[o["scale"]], SIGNS[o["sign"]],
                  None if imgs is None else imgs.ctypes.data, frames.ctypes.data, par.ctypes.data)
    return frames, (None if int(par[0]) == 2 ** 64 - 1 else int(par[0]))
