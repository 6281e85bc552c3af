"""CPU: motion's dithered 8-bit store (motion/motion.c:756-788 with -d) against the reference's own lines (tests/golden/ref_dither.npz,
tests/golden/make_dither_fixtures.py), the shared per-pixel header dspfun_amd/csrc/dither_core.h compiled with g++, and the ABI of the two
new entry points (the dither kernel itself runs in tests/test_motion_dither_gpu.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dither_ref as dr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = np.load(os.path.join(HERE, "golden", "ref_dither.npz"))
NAMES = [c[0] for c in dr.CASES]


def planes(i):
    c, sf, nm, scaled, minbuf, block = dr.case_inputs(i)
    d, h, w = scaled
    return c[:, :d, :h, :w], sf, nm


@pytest.mark.parametrize("i", range(len(dr.CASES)), ids=NAMES)
def test_restatement_is_the_reference_fd_build(i):
    """the numpy restatement the GPU tests use at full size equals the reference's lines at COEFF=F / INTERMEDIATE=D, byte for byte"""
    c, sf, nm = planes(i)
    assert np.array_equal(dr.dither_planes(c, sf, nm), FIX["out_fd_" + NAMES[i]])


@pytest.mark.parametrize("i", range(len(dr.CASES)), ids=NAMES)
def test_long_double_build_bar(i):
    """the tool's default (INTERMEDIATE=L) against the F/D bytes: every pixel within +-1, the means of whole 8x8 blocks within 0.1 --
    the bar include/dspfft.h documents (error diffusion is chaotic: one last-bit difference moves the pattern downstream)"""
    fd, fl = FIX["out_fd_" + NAMES[i]].astype(np.float64), FIX["out_fl_" + NAMES[i]].astype(np.float64)
    assert np.abs(fd - fl).max() <= 1
    h, w = fd.shape[-2] // 8 * 8, fd.shape[-1] // 8 * 8
    if h and w:
        m = lambda a: a[..., :h, :w].reshape(*a.shape[:-2], h // 8, 8, w // 8, 8).mean(axis=(-3, -1))
        assert np.abs(m(fd) - m(fl)).max() <= 0.1


def test_fixtures_exercise_clamps_ties_and_differences():
    """the fixture inputs reach both clamps, and the two reference builds do differ somewhere (otherwise the bar above shows nothing)"""
    big = FIX["out_fd_960x540"]
    assert (big == 0).mean() > 0.01 and (big == 255).mean() > 0.01
    assert any((FIX["out_fd_" + n] != FIX["out_fl_" + n]).any() for n in NAMES)


CPP = r'''
#include <stdint.h>
#include <vector>
#include "dither_core.h"
extern "C" void run(uint8_t *serial, uint8_t *wave, const float *in, long long pitch, int h, int w, double sf, double nm)
{
	double tab[256];
	dspfft::dither_table(tab, sf, nm);
	std::vector<double> row(w), dp((size_t)h * w);
	dspfft::dither_plane_serial(serial, in, pitch, h, w, sf, nm, tab, row.data(), 1);
	dspfft::dither_plane_wavefront(wave, in, pitch, h, w, sf, nm, tab, dp.data());
}
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("dither_core")
    src, so = d / "core.cpp", d / "core.so"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "dspfun_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.run.argtypes = [C.c_void_p] * 3 + [C.c_longlong, C.c_int, C.c_int, C.c_double, C.c_double]
    return lib


@pytest.mark.parametrize("i", range(len(dr.CASES)), ids=NAMES)
def test_shared_header_serial_and_wavefront_orders(core, i):
    """dither_core.h's raster walk (the small-plane kernel's) and its anti-diagonal walk (the wavefront kernel's order) both give the F/D bytes"""
    c, sf, nm, scaled, minbuf, block = dr.case_inputs(i)
    d, h, w = scaled
    want = FIX["out_fd_" + NAMES[i]]
    for b in range(c.shape[0]):
        for z in range(d):
            plane = np.ascontiguousarray(c[b, z])
            s = np.zeros(plane.shape, dtype=np.uint8)
            v = np.zeros(plane.shape, dtype=np.uint8)
            core.run(s.ctypes.data, v.ctypes.data, plane.ctypes.data, plane.shape[1], h, w, sf, nm)
            assert np.array_equal(s[:h, :w], want[b, z]), (NAMES[i], b, z)
            assert np.array_equal(v[:h, :w], want[b, z]), (NAMES[i], b, z)


def declared():
    txt = open(os.path.join(ROOT, "include", "dspfft.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(dspfft_[a-z0-9_]+)\s*\(", txt))


def test_abi_declares_and_binds_the_dither_entry_points():
    from dspfun_amd import _lib
    for name in ("dspfft_motion_dither_u8", "dspfft_execute_roundtrip_u8_dither"):
        assert name in declared() and name in _lib.SYMBOLS, name
    assert [f for f, _ in _lib.DitherGeom._fields_] == ["n", "row_pitch", "plane_pitch", "nblocks", "block_step"]


def test_emulation_library_reports_the_missing_kernel():
    """the CPU emulation build of engine.cpp has no dither kernel: it still loads, and the dithered roundtrip fails with a message"""
    import emul_lib
    lib = emul_lib.emul()
    assert not hasattr(lib, "dspfft_motion_dither_u8")
    h = w = 16
    fwd, inv = C.c_void_p(), C.c_void_p()
    n = (C.c_int * 2)(h, w)
    assert lib.dspfft_plan_many_r2r(C.byref(fwd), 2, n, 1, None, 1, 0, None, 1, 0, (C.c_int * 2)(5, 5)) == 0
    assert lib.dspfft_plan_many_r2r_ordered(C.byref(inv), 2, n, 1, None, 1, 0, None, 1, 0, (C.c_int * 2)(4, 4), 1) == 0
    src = np.zeros(h * w, dtype=np.uint8)
    dst = np.zeros(h * w, dtype=np.uint8)
    work = np.zeros(h * w, dtype=np.float32)
    rc = lib.dspfft_execute_roundtrip_u8_dither(fwd, inv, src.ctypes.data, dst.ctypes.data, work.ctypes.data, 1.0, 0.5, None, None, None)
    assert rc < 0 and b"not in this build" in lib.dspfft_last_error()
    lib.dspfft_destroy_plan(fwd)
    lib.dspfft_destroy_plan(inv)
