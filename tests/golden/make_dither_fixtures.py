"""Regenerates tests/golden/ref_dither.npz from the REFERENCE'S OWN dithered 8-bit store.  Needs the reference tree (DSPFUN_REFERENCE) and
gcc; the GPU tests only read the .npz.

Same method as make_ref_fixtures.py: the text of these line ranges is read from the reference at generation time into a temporary translation
unit, around this script's own declarations of the variables they use (one component, i = 0), and compiled with plain gcc:

  motion/motion.c:18-35,58-60   the spectrogram / preserve-dc enums and struct coords
  motion/motion.c:559-573       scalefactor, normalization (and the other per-component constants)
  motion/motion.c:755-788       the output stage with dithering = true, spec = none, float_pixels = false, linear = false

compiled twice, -std=c11 -O2 -ffp-contract=off, no -march, no -ffast-math (make_ref_fixtures.py says why):
  COEFF_PRECISION=F INTERMEDIATE_PRECISION=D   -> out_fd_<case>: the bar the device kernel meets byte for byte
  COEFF_PRECISION=F INTERMEDIATE_PRECISION=L   -> out_fl_<case>: the tool's default build (motion/Makefile:1-2)

Inputs are not stored: tests/dither_ref.py regenerates them from recorded seeds (oracle_lib.synth_f32).  No reference text is written to the
repository; only the output bytes and the constants go into the fixture file."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DSPFUN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
import dither_ref as dr  # noqa: E402


def lines(path, a, b):
    with open(os.path.join(REF, path)) as f:
        src = f.read().split("\n")
    return "\n".join(src[a - 1:b]) + "\n"


def build(tmp, intermediate):
    tu = "#include <stdlib.h>\n#include <stdint.h>\n#include <stdbool.h>\n#include <string.h>\n#include <math.h>\n#include \"precision.h\"\n#include \"keyed_enum.h\"\n"
    tu += lines("motion/motion.c", 18, 35) + lines("motion/motion.c", 58, 60)
    tu += """
/* one block of {d,h,w} = minbuf_; the scaled extent is what is stored; sf_nm_out receives scalefactor[0], normalization[0] */
void ref_dither_store(float *coeffs_, unsigned char *pblock_, const uint64_t *minbuf_, const uint64_t *scaled_, const uint64_t *block_, long double *sf_nm_out)
{
	const int components = 1, i = 0;
	coords minbuf = {{minbuf_[0], minbuf_[1], minbuf_[2]}}, scaled = {{scaled_[0], scaled_[1], scaled_[2]}}, block = {{block_[0], block_[1], block_[2]}};
	intermediate threshold_min = 0, threshold_max = 0, quant = 0;
	enum spectype spec = spectype_none;
	enum ispectype ispec = ispectype_none;
	bool float_pixels = false, linear = false, dithering = true;
	intermediate (*output_trc)(intermediate) = NULL;
	coeff *coeffs = coeffs_;
	void *pblock = pblock_;
	coeff dc = 0;
"""
    tu += lines("motion/motion.c", 559, 573)
    tu += "\tif(!spec) {}\n" + lines("motion/motion.c", 755, 788)
    tu += "\tsf_nm_out[0] = scalefactor[0]; sf_nm_out[1] = normalization[0];\n"
    tu += "\t(void)components; (void)linear; (void)float_pixels; (void)output_trc; (void)quantizer; (void)threshold; (void)ispec; (void)c; (void)ic; (void)dc;\n}\n"
    src = os.path.join(tmp, f"dither_{intermediate}.c")
    so = os.path.join(tmp, f"dither_{intermediate}.so")
    with open(src, "w") as f:
        f.write(tu)
    subprocess.check_call(["gcc", "-std=c11", "-D_GNU_SOURCE", "-DCOEFF_PRECISION=F", f"-DINTERMEDIATE_PRECISION={intermediate}", "-O2", "-ffp-contract=off",
                           "-fPIC", "-shared", "-w", "-I" + os.path.join(REF, "include"), src, "-o", so, "-lm"])
    lib = C.CDLL(so)
    lib.ref_dither_store.argtypes = [C.c_void_p] * 6
    return lib


def run(lib, i):
    c, sf, nm, scaled, minbuf, block = dr.case_inputs(i)
    out = np.zeros(c.shape, dtype=np.uint8)
    u64 = lambda v: np.array([v[2], v[1], v[0]], dtype=np.uint64)      # coords are {w, h, d}
    sfnm = np.zeros(2, dtype=np.longdouble)
    for b in range(c.shape[0]):
        cb = np.ascontiguousarray(c[b]).copy()
        ob = np.zeros(cb.shape, dtype=np.uint8)
        mb, sc, bl = u64(minbuf), u64(scaled), u64(block)
        lib.ref_dither_store(cb.ctypes.data, ob.ctypes.data, mb.ctypes.data, sc.ctypes.data, bl.ctypes.data, sfnm.ctypes.data)
        out[b] = ob
    d, h, w = scaled
    assert float(sfnm[0]) == sf and abs(float(sfnm[1]) - nm) <= 1e-15 * nm, (sfnm, sf, nm)
    return out[:, :d, :h, :w]


def main(path=os.path.join(HERE, "ref_dither.npz")):
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        fd, fl = build(tmp, "D"), build(tmp, "L")
        for i, (name, *_rest) in enumerate(dr.CASES):
            arrays["out_fd_" + name] = run(fd, i)
            arrays["out_fl_" + name] = run(fl, i)
    np.savez_compressed(path, **arrays)
    print(path, sum(a.nbytes for a in arrays.values()), "bytes of outputs")


if __name__ == "__main__":
    main(*sys.argv[1:])
