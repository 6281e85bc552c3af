"""Regenerates tests/golden/ref_motion_u8_linear.npz from the REFERENCE'S OWN 8-bit load, store and dithered store with linear = true.  Needs
the reference tree (DSPFUN_REFERENCE) and gcc; the tests only read the .npz.

Same method as make_trc_fixtures.py: make_ref_fixtures.build_motion_io and make_dither_fixtures.build are run as they are, and the
translation units they wrote are compiled once more with linear = true, float_pixels = false (an argument of the load / store stand-ins)
and input_trc / output_trc pointing at make_trc_fixtures.TRC_C:

  lut_<trc>             motion/motion.c:617-638 over the bytes 0..255, COEFF_PRECISION=F INTERMEDIATE_PRECISION=L, the ten built ids
  store_<trc>_in/_out   :755-776, F/L, ids 13, 1, 7, 5, 11, block trc_ref.MOTION_BLOCK in MOTION_MINBUF.  _in: coefficients whose linear pel
                        is, for every k = 0..254, the float nearest to the linear preimage of k + 0.5 moved by +-1, +-2 and +-3 float steps,
                        and that float itself where this script's double evaluation puts it 1e-9 or more from the half-integer (it is an
                        exact tie for some k in the linear toe of the curves)
  store_<trc>_rand_out  the bytes of tests/trc_u8_ref.random_coeffs(): 2000 seeded values whose pel spans -64..320
  dither_<trc>_<case>   :755-788, F/D (the bar dspfft_motion_dither_u8 meets), ids 13 and 7, planes 24 x 20 and 96 x 40

The store inputs also go through the F/D build: equal bytes on every kept input, and all 256 byte values must occur.  Only numbers go into
the .npz."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DSPFUN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import trc_ref as tr  # noqa: E402
import trc_u8_ref as tu8  # noqa: E402
import make_trc_fixtures as mtf  # noqa: E402
import make_dither_fixtures as mdf  # noqa: E402

F32, F64 = np.float32, np.float64
GCC = ["gcc", "-std=c11", "-D_GNU_SOURCE", "-DCOEFF_PRECISION=F", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-I" + os.path.join(REF, "include")]


def motion_libs(tmp):
    """make_trc_fixtures.motion_lib's translation unit (linear = true, the hooks set): its F/L build, and the same file built F/D"""
    fl = mtf.motion_lib(tmp)
    so = os.path.join(tmp, "motion_io_trc_fd.so")
    subprocess.check_call(GCC + ["-DINTERMEDIATE_PRECISION=D", os.path.join(tmp, "motion_io_trc.c"), "-o", so, "-lm"])
    fd = C.CDLL(so)
    vp = C.c_void_p
    fd.ref_motion_load.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp]
    fd.ref_motion_store.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_float, vp]
    return fl, fd


def dither_lib(tmp):
    mdf.build(tmp, "D")
    with open(os.path.join(tmp, "dither_D.c")) as f:
        tu = f.read()
    edits = [('#include "keyed_enum.h"\n', '#include "keyed_enum.h"\n' + mtf.TRC_C),
             ("bool float_pixels = false, linear = false, dithering = true;", "bool float_pixels = false, linear = true, dithering = true;"),
             ("intermediate (*output_trc)(intermediate) = NULL;", "double (*output_trc)(double) = trc_enc;")]
    for old, new in edits:
        assert tu.count(old) == 1, (old, tu.count(old))
        tu = tu.replace(old, new)
    src, so = os.path.join(tmp, "dither_D_trc.c"), os.path.join(tmp, "dither_D_trc.so")
    with open(src, "w") as f:
        f.write(tu)
    subprocess.check_call(GCC + ["-DINTERMEDIATE_PRECISION=D", src, "-o", so, "-lm"])
    lib = C.CDLL(so)
    lib.ref_dither_store.argtypes = [C.c_void_p] * 6
    return lib


def block_index():
    (d, h, w), (md, mh, mw) = tr.MOTION_BLOCK, tr.MOTION_MINBUF
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    return ((z * mh + y) * mw + x).ravel()


def geometry():
    (d, h, w), (md, mh, mw) = tr.MOTION_BLOCK, tr.MOTION_MINBUF
    return np.array([mw, mh, md], dtype=np.uint64), np.array([w, h, d], dtype=np.uint64), md * mh * mw


def load_lut(lib, trc):
    MB, A, n = geometry()
    idx = block_index()
    pix = np.zeros(n, dtype=np.uint8)
    pix[idx] = np.arange(idx.size) % 256
    out = np.full(n, F32(-77.0))
    cic = np.zeros(2, dtype=np.longdouble)
    lib.set_trc(trc)
    lib.ref_motion_load(out.ctypes.data, pix.ctypes.data, MB.ctypes.data, A.ctypes.data, A.ctypes.data, 0, 0, cic.ctypes.data)
    got = out[idx]
    lut = got[:256].copy()
    assert np.array_equal(got.view(np.uint32), lut[np.arange(idx.size) % 256].view(np.uint32))
    return lut


def store_bytes(lib, trc, co):
    """the reference's store over `co`, a block's worth at a time"""
    MB, A, n = geometry()
    idx = block_index()
    cic = np.zeros(2, dtype=np.longdouble)
    lib.set_trc(trc)
    out = np.empty(co.size, dtype=np.uint8)
    for i0 in range(0, co.size, idx.size):
        part = co[i0:i0 + idx.size]
        c = np.zeros(n, dtype=F32)
        c[idx[:part.size]] = part
        p = np.full(n, 99, dtype=np.uint8)
        lib.ref_motion_store(c.ctypes.data, p.ctypes.data, MB.ctypes.data, A.ctypes.data, A.ctypes.data, 0, 0, float(c[0]), cic.ctypes.data)
        out[i0:i0 + part.size] = p[idx[:part.size]]
    return out


def boundary_coeffs(trc):
    """coefficients around every rounding boundary of the store, and which of them are kept"""
    sf, nm = tu8.store_scales()
    mul = F64(sf) * F64(nm) * F64(nm)
    k = np.arange(255, dtype=F64) + 0.5
    target = tr.exact(trc, 1, k / 255) * 255                        # the linear pel whose encoding is k + 0.5
    c0 = (target / mul).astype(F32)
    cols = [c0]
    up, dn = c0, c0
    for _ in range(3):
        up, dn = np.nextafter(up, F32(np.inf)), np.nextafter(dn, F32(-np.inf))
        cols += [up, dn]
    co = np.stack(cols, axis=1)                                      # (255, 7): nearest, +1, -1, +2, -2, +3, -3
    enc = tr.exact(trc, 0, tu8.store_pel(co[:, 0], sf, nm) / 255) * 255
    keep = np.ones(co.shape, dtype=bool)
    keep[:, 0] = np.abs(enc - k) >= 1e-9
    return co[keep], int((~keep).sum())


def dither_run(lib, trc, name):
    c, sf, nm = tu8.dither_inputs(trc, name)
    h, w = c.shape
    lib.set_trc(trc)
    cb = np.ascontiguousarray(c).copy()
    ob = np.zeros(cb.shape, dtype=np.uint8)
    g = np.array([w, h, 1], dtype=np.uint64)
    sfnm = np.zeros(2, dtype=np.longdouble)
    lib.ref_dither_store(cb.ctypes.data, ob.ctypes.data, g.ctypes.data, g.ctypes.data, g.ctypes.data, sfnm.ctypes.data)
    assert float(sfnm[0]) == sf and abs(float(sfnm[1]) - nm) <= 1e-15 * nm, (sfnm, sf, nm)
    return ob


def main(path=os.path.join(HERE, "ref_motion_u8_linear.npz")):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fl, fd = motion_libs(tmp)
        for trc in tr.IDS:
            out[f"lut_{trc}"] = load_lut(fl, trc)
        rnd = tu8.random_coeffs()
        for trc in tu8.STORE_TRCS:
            co, dropped = boundary_coeffs(trc)
            b_l, b_d = store_bytes(fl, trc, co), store_bytes(fd, trc, co)
            r_l, r_d = store_bytes(fl, trc, rnd), store_bytes(fd, trc, rnd)
            assert np.array_equal(b_l, b_d) and np.array_equal(r_l, r_d), trc
            assert np.unique(np.concatenate([b_l, r_l])).size == 256, trc
            out[f"store_{trc}_in"], out[f"store_{trc}_out"], out[f"store_{trc}_rand_out"] = co, b_l, r_l
            print("store", trc, co.size, "boundary inputs,", dropped, "ties dropped")
        dl = dither_lib(tmp)
        for trc in tu8.DITHER_TRCS:
            for name, _hw in tu8.DITHER_CASES:
                out[f"dither_{trc}_{name}"] = dither_run(dl, trc, name)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
