"""CPU (-m "not gpu"): transfer characteristics (dspfun_amd/csrc/trc_core.h compiled with g++ -ffp-contract=off, tests/trc_ref.py): the
exact evaluation against an independent numpy statement of the table, bit for bit; inverse pairs; 8-bit code values; names and ids; the
production evaluation's host build against the 1-ulp bar; what the CPU emulation build answers; the tools' option parsing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import trc_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


def _bits(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


@pytest.mark.parametrize("inverse", (0, 1))
@pytest.mark.parametrize("trc", tr.IDS)
def test_exact_evaluation_is_the_table_bit_for_bit(trc, inverse):
    """over the float sweep (as doubles) and, in double, both neighbours of every threshold"""
    x = tr.sweep().astype(F64)
    th = np.array([t for i in tr.IDS for t in tr.thresholds(i)], dtype=F64)
    x = np.concatenate([x, th, np.nextafter(th, np.inf), np.nextafter(th, -np.inf)])
    got, want = tr.exact(trc, inverse, x), tr.np_eval(trc, inverse, x)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])
    assert nan.sum() == 1                                       # the one NaN of the sweep stays NaN


@pytest.mark.parametrize("trc", tr.IDS)
def test_edge_cases_follow_the_comparisons(trc):
    shape = tr.TABLE[trc][1]
    for inverse in (0, 1):
        y = tr.exact(trc, inverse, np.array([-0.0, 0.0, np.nan, np.inf, 1.0]))
        # -0.0 passes `0 > x` and comes out of the linear segment as -0.0; the pure gammas' pow makes it +0.0
        assert y[0] == 0 and np.signbit(y[0]) == (shape != "gamma"), (trc, inverse, y[0])
        assert y[1] == 0 and not np.signbit(y[1])
        assert np.isnan(y[2]) and y[3] == np.inf
        assert abs(y[4] - 1.0) < 1e-15
        neg = tr.exact(trc, inverse, np.array([-0.5, -np.inf]))
        if shape in ("toe", "gamma"):
            assert np.all(neg == 0) and not np.signbit(neg).any()
        elif shape == "sym":
            assert np.array_equal(neg, -tr.exact(trc, inverse, np.array([0.5, np.inf])))


@pytest.mark.parametrize("trc", tr.IDS)
def test_decode_of_encode_returns_the_argument(trc):
    """the sweep's values in (b, 4).  The thresholds and their neighbours are kept out: the piecewise functions are not continuous to this
    level where their pieces meet, and the neighbour of 0 is a subnormal whose logarithm (-103) multiplies the rounding of 1 / g."""
    x = tr.sweep().astype(F64)
    b = tr.TABLE[trc][3] or 0.0
    x = x[(x > b * 1.001) & (x >= 2.0 ** -12) & (x < 4)]
    assert x.size > 1_000_000
    back = tr.exact(trc, 1, tr.exact(trc, 0, x))
    err = np.abs(back - x) / x
    print(trc, "max relative error of decode(encode(x))", err.max())
    assert err.max() <= 1e-15


@pytest.mark.parametrize("trc", tr.IDS)
def test_8bit_code_values_survive_decode_and_encode(trc):
    v = np.arange(256, dtype=F64)
    assert np.array_equal(np.round(255 * tr.exact(trc, 0, tr.exact(trc, 1, v / 255))), v)


def test_names_and_ids():
    from emul_lib import emul
    L, R = emul(), tr.lib()
    for fn_from, fn_name in ((L.dspfft_trc_from_name, L.dspfft_trc_name), (R.trcr_from_name, R.trcr_name)):
        for trc in tr.IDS:
            name = tr.TABLE[trc][0]
            assert fn_from(name.encode()) == trc and fn_name(trc) == name.encode()
        for trc, name in tr.REFUSED.items():
            assert fn_name(trc) is None and fn_from(name.encode()) == -1, (trc, name)
        assert fn_from(b"") == -1 and fn_from(None) == -1 and fn_from(b"BT709") == -1 and fn_name(-1) is None and fn_name(20) is None


def test_python_names():
    from emul_lib import emul
    from dspfun_amd.engine import trc_id, DspfftError
    L = emul()
    assert trc_id("iec61966-2-1", L) == 13 and trc_id(13, L) == 13 and trc_id(0, L) == 0 and trc_id(None, L) == 0 and trc_id("bt2020-12", L) == 15
    for bad in ("smpte2084", "srgb", 16, 2, -1):
        with pytest.raises(DspfftError, match="unknown or not built"):
            trc_id(bad, L)


@pytest.mark.parametrize("inverse", (0, 1))
@pytest.mark.parametrize("trc", tr.IDS)
def test_production_evaluation_meets_the_bar_on_the_host(trc, inverse):
    """trc_eval_f32 is portable C++: its host build over the sweep, within 1 float ulp of (float)exact((double)x), bit-equal at 0, NaN, inf"""
    got = tr.eval_f32(trc, inverse, tr.sweep())
    bad = tr.bar_violations(got, tr.want_f32(trc, inverse))
    assert bad.size == 0, (trc, inverse, bad[:5], tr.sweep()[bad[:5]], got[bad[:5]], tr.want_f32(trc, inverse)[bad[:5]])


def test_lean_pow_against_libm_in_double():
    """the margin trc_core.h claims for trc_pow_lean (relative error below 2^-40), pinned directly: against libm's pow, itself within
    1 double ulp (2^-52), over the sweep's positive floats, every exponent of the table, and arguments the decodes form (not floats)"""
    x = tr.sweep().astype(F64)
    x = x[x > 0]
    x = x[np.isfinite(x)]
    x = np.concatenate([x, (x[::7] + 0.055) / 1.055, x[::11] * 1e-30, x[::13] * 1e30])
    worst = 0.0
    for e in sorted({g for t in tr.TABLE.values() for g in t[5:7] if g}):
        want, got = tr.libm_pow(x, e), tr.lean_pow(x, e)
        worst = max(worst, float((np.abs(got - want) / want).max()))
    print("trc_pow_lean: largest relative distance from libm's pow %.3g = 2^%.1f" % (worst, np.log2(worst)))
    assert worst < 2.0 ** -40
    sp = tr.lean_pow(np.array([0.0, -0.0, np.inf, np.nan, -1.0]), 0.45)
    assert sp[0] == 0 and sp[1] == 0 and not np.signbit(sp[:2]).any() and sp[2] == np.inf and np.isnan(sp[3]) and np.isnan(sp[4])


def test_production_evaluation_over_the_whole_float_range():
    """beyond the sweep: every 4099th bit pattern of every finite float, subnormals and the largest included (results that leave a
    float's range round to 0 or inf exactly where the exact evaluation's do)"""
    bits = np.arange(0, 0x7F800000, 4099, dtype=np.uint32)
    x = np.concatenate([bits.view(F32), -bits.view(F32), np.array([np.finfo(F32).max, np.finfo(F32).tiny, 1e-45], dtype=F32)])
    for trc in (13, 1, 5, 7, 11, 4):
        for inverse in (0, 1):
            with np.errstate(over="ignore"):
                want = tr.exact(trc, inverse, x.astype(F64)).astype(F32)
            bad = tr.bar_violations(tr.eval_f32(trc, inverse, x), want)
            assert bad.size == 0, (trc, inverse, x[bad[:5]])


def test_emulation_build_answers_set_trc_and_refuses_to_launch():
    from emul_lib import emul
    from dspfun_amd import _lib
    L = emul()
    buf = np.full(8, 0.5, dtype=F32)
    assert L.dspfft_trc_apply_f32(buf.ctypes.data, buf.ctypes.data, 8, 13, 0, None) == -3
    assert "not in this build" in L.dspfft_last_error().decode()
    assert np.all(buf == 0.5)
    assert L.dspfft_trc_apply_f32(buf.ctypes.data, buf.ctypes.data, 8, 16, 0, None) == -1        # smpte2084: not built, said before anything else
    assert "not built" in L.dspfft_last_error().decode()
    n, hw = (C.c_int * 3)(1, 2, 4), (C.c_int * 2)(2, 4)
    assert L.dspfft_motion_load_f32_linear(buf.ctypes.data, buf.ctypes.data, n, hw, 13, None) == -3
    assert "not in this build" in L.dspfft_last_error().decode()
    assert L.dspfft_motion_store_f32_linear(buf.ctypes.data, buf.ctypes.data, n, hw, 1.0, 1.0, 13, None) == -3
    assert L.dspfft_motion_store_f32_linear(buf.ctypes.data, buf.ctypes.data, n, hw, 1.0, 1.0, 0, None) == -1
    assert np.all(buf == 0.5)
    # scan frames: the handle takes a transfer characteristic; composing still needs the kernels
    sf = C.c_void_p()
    o = _lib.ScanFrameOpts(0, 0, 1, 0, 0.0, 0, 0, 0)
    assert L.dspfft_scanframes_create(C.byref(sf), 4, 2, C.byref(o)) == 0
    assert L.dspfft_scanframes_set_trc(sf, 13) == 0 and L.dspfft_scanframes_set_trc(sf, 0) == 0
    assert L.dspfft_scanframes_set_trc(sf, 16) == -1 and L.dspfft_scanframes_set_trc(None, 13) == -1
    L.dspfft_scanframes_destroy(sf)
    # zoom animation: trc 0 runs as before, a transfer characteristic needs the kernel
    z = C.c_void_p()
    assert L.dspfft_zoomanim_create(C.byref(z), 8, 6, 0, 12, 9) == 0
    co = np.ones(8 * 6 * 3, dtype=F32)
    work = np.zeros(L.dspfft_zoomanim_work_floats(z), dtype=F32)
    out = np.zeros(12 * 9 * 3, dtype=F32)
    assert L.dspfft_zoomanim_set_coeffs(z, co.ctypes.data, None) == 0
    assert L.dspfft_zoomanim_set_trc(z, 9) == -1 and L.dspfft_zoomanim_set_trc(z, 0) == 0
    assert L.dspfft_zoomanim_execute(z, 1.5, 1.0, 1.5, 1.0, 0.0, 0.0, 0, 0, out.ctypes.data, work.ctypes.data, None) == 0
    assert L.dspfft_zoomanim_set_trc(z, 13) == 0
    assert L.dspfft_zoomanim_execute(z, 1.5, 1.0, 1.5, 1.0, 0.0, 0.0, 0, 0, out.ctypes.data, work.ctypes.data, None) == -3
    assert "not in this build" in L.dspfft_zoomanim_last_error().decode()
    L.dspfft_zoomanim_destroy(z)


def _tool(name, args, tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), name])
    return subprocess.run([os.path.join(ROOT, "host", name)] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))


@pytest.mark.parametrize("tool", ("scan_dev", "zoom_dev"))
def test_tools_refuse_an_unknown_trc_before_the_device_is_touched(tool, tmp_path):
    """no input file exists and there is no device here: the option's own message comes first"""
    for name in ("nonsense", "smpte2084"):
        r = _tool(tool, ["--trc", name, "in.pf", "out.pf"], tmp_path)
        assert r.returncode == 2 and "--trc " + name in r.stderr and "unknown transfer characteristic" in r.stderr, r.stderr
    r = _tool(tool, ["in.pf"], tmp_path)
    assert r.returncode == 2 and "--trc NAME" in r.stderr                  # the help text names the option
    # a known name passes the option parser: the next complaint is about the input file
    r = _tool(tool, ["--trc", "iec61966-2-1", "in.pf", "out.pf"], tmp_path)
    assert r.returncode == 1 and "cannot read in.pf" in r.stderr, r.stderr


@pytest.mark.parametrize("tool,msg", (("scan_dev", "--linear is not supported"), ("zoom_dev", "-g (linear RGB) is not supported")))
def test_tools_still_refuse_g_and_point_at_trc(tool, msg, tmp_path):
    r = _tool(tool, ["-g", "in.pf", "out.pf"], tmp_path)
    assert r.returncode == 2 and msg in r.stderr and "--trc iec61966-2-1" in r.stderr, r.stderr
