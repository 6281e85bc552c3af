"""spec / ispec on 8-bit images as one fused call each way (dspfft_execute_spec_u8 / dspfft_execute_ispec_u8), the parts that need no device:
the new symbols, the emulation library's -3 (the kernels are HIP-only), every refusal ahead of any launch, the Python helpers, the two sweeps'
sample arithmetic (dspfun_amd/csrc/spec_image_core.h compiled with g++) against the oracle's spec.c / ispec.c restatements, and the 8-bit
ends of interleaved RGB lines (dct_spec.h RowU8Rgb: the emulation backend has no such entries, so the phases are compiled with g++ here and
walked thread by thread beside the plain float line's)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import spec_image_ref as sr
from dspfun_amd import _lib
from dspfun_amd.engine import Plan, DspfftError, REDFT01, REDFT10, spec_image_plans, spec_image_params

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "dspfun_amd", "csrc")
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned address for calls that are refused before anything reads it
NAMES = ("dspfft_execute_spec_u8", "dspfft_execute_ispec_u8")


def params(gain=1.0, rng=0, scale=1, sign=1):
    return _lib.SpecImageParams(gain, rng, scale, sign)


def test_the_new_symbols_exist_and_the_emulation_library_answers_minus_3_writing_nothing():
    from emul_lib import emul
    prod = C.CDLL(_lib.LIB_PATH)
    L = emul()
    for name in NAMES:
        assert hasattr(prod, name) and hasattr(L, name), name
        assert name in _lib.SYMBOLS
    h, w, c = 24, 40, 3
    n = h * w * c
    fwd, inv = spec_image_plans(h, w, c, lib=L)
    src = ol.synth_u8(7, n)
    for plan, inverse in ((fwd, False), (inv, True)):
        out, smap = np.full(n, 9, dtype=np.uint8), np.full(n, 5, dtype=np.uint8)
        work = np.full(n, 7.0, dtype=np.float32)
        dc = np.full(c, 3.0)
        p = params(100.0, 1, 0, 0)
        if inverse:
            rc = L.dspfft_execute_ispec_u8(plan._h, src.ctypes.data, smap.ctypes.data, out.ctypes.data, work.ctypes.data, (C.c_double * c)(*dc), 1, C.byref(p), None)
            with pytest.raises(DspfftError, match="not built into this library"):
                plan.ispec_u8(src.ctypes.data, out.ctypes.data, work.ctypes.data, p, dc=list(dc))
        else:
            rc = L.dspfft_execute_spec_u8(plan._h, src.ctypes.data, out.ctypes.data, smap.ctypes.data, work.ctypes.data, dc.ctypes.data, C.byref(p), None)
            with pytest.raises(DspfftError, match="not built into this library"):
                plan.spec_u8(src.ctypes.data, out.ctypes.data, work.ctypes.data, p)
        assert rc == -3
        assert np.all(out == 9) and np.all(smap == 5) and np.all(work == 7.0) and np.all(dc == 3.0)


@pytest.mark.parametrize("which", ["emulation", "product"])
def test_every_refusal_returns_minus_2_with_its_reason_before_any_launch(which):
    """the emulation library plans any size; the product library plans 16-point axes without a device (they need no device tables)"""
    if which == "emulation":
        from emul_lib import emul
        L, (h, w) = emul(), (24, 40)
    else:
        L, (h, w) = _lib.load(), (16, 16)
    err = L.dspfft_last_error
    S, I = L.dspfft_execute_spec_u8, L.dspfft_execute_ispec_u8
    fwd, inv = spec_image_plans(h, w, 3, lib=L)
    p = C.byref(params())
    dc3 = (C.c_double * 3)(0.5, 0.5, 0.5)
    spec = lambda plan, sp=p, smap=None, work=FAKE: S(plan._h, FAKE, FAKE, smap, work, None, sp, None)
    ispec = lambda plan, sp=p, smap=None, work=FAKE, dc=dc3, restore=0: I(plan._h, FAKE, smap, FAKE, work, dc, restore, sp, None)
    # an f64 plan
    f64 = Plan.image(h, w, 3, REDFT10, lib=L, dtype="f64")
    assert spec(f64) == -2 and b"f64" in err()
    assert ispec(Plan.image(h, w, 3, REDFT01, lib=L, dtype="f64")) == -2 and b"f64" in err()
    # rank
    r1 = Plan.many_r2r([w], [REDFT10], howmany=3, istride=3, idist=1, ostride=3, odist=1, lib=L)
    assert spec(r1) == -2 and b"rank 2" in err()
    r1i = Plan.many_r2r([w], [REDFT01], howmany=3, istride=3, idist=1, ostride=3, odist=1, lib=L, first_axis_first=True)
    assert ispec(r1i) == -2 and b"rank 2" in err()
    # kind
    assert spec(inv) == -2 and b"REDFT10" in err()
    assert ispec(fwd) == -2 and b"REDFT01" in err()
    # layout: planar channels, a padded pitch
    planar = Plan.many_r2r([h, w], [REDFT10] * 2, howmany=3, idist=h * w, odist=h * w, lib=L)
    assert spec(planar) == -2 and b"interleaved" in err()
    padded = Plan.many_r2r([h, w], [REDFT01] * 2, howmany=3, inembed=[h, w + 4], istride=3, idist=1, onembed=[h, w + 4], ostride=3, odist=1, lib=L, first_axis_first=True)
    assert ispec(padded) == -2 and b"dense" in err()
    # pass order
    fwd_cols_first = Plan.many_r2r([h, w], [REDFT10] * 2, howmany=3, istride=3, idist=1, ostride=3, odist=1, lib=L, first_axis_first=True)
    assert spec(fwd_cols_first) == -2 and b"pass order" in err()
    assert ispec(Plan.image(h, w, 3, REDFT01, lib=L)) == -2 and b"pass order" in err()
    # more channels than the decode handles
    f5, i5 = spec_image_plans(h, w, 5, lib=L)
    assert spec(f5) == -2 and b"5 channels" in err()
    assert ispec(i5, dc=(C.c_double * 5)(*[0.5] * 5)) == -2 and b"5 channels" in err()
    # a sign map with a sign type other than abs
    for sign in (1, 2, 3):
        sp = C.byref(params(sign=sign))
        assert spec(fwd, sp=sp, smap=FAKE) == -2 and b"sign map" in err()
        assert ispec(inv, sp=sp, smap=FAKE) == -2 and b"sign map" in err()
    # range dc / dcs, or restore_dc, without dc
    for rng in (1, 2):
        assert ispec(inv, sp=C.byref(params(rng=rng)), dc=None) == -2 and b"DC values" in err()
    assert ispec(inv, dc=None, restore=1) == -2 and b"DC values" in err()
    # no work buffer
    assert spec(fwd, work=None) == -2 and b"work buffer" in err()
    assert ispec(inv, work=None) == -2 and b"work buffer" in err()
    # (not refusals of the -2 kind, but also ahead of any launch: codes out of range, a null buffer)
    assert spec(fwd, sp=C.byref(params(rng=3))) == -1 and ispec(inv, sp=C.byref(params(sign=4))) == -1
    assert S(fwd._h, None, FAKE, None, FAKE, None, p, None) == -1
    with pytest.raises(DspfftError, match="f64"):
        f64.spec_u8(4096, 4096, 4096, params())


def test_spec_image_params_resolves_specs_presets_and_gains():
    h, w = 24, 40
    native = 127.5 * math.sqrt(w * h * 4)
    want = {"abs": (native, 1, 0, 0), "shift": (native, 0, 0, 1), "flat": (1.0, 0, 1, 1), "sign": (1.0, 0, 1, 2), "copy": (1.0, 0, 1, 3)}     # spec.h:71-76
    for name, (g, r, s, sg) in want.items():
        p = spec_image_params(h, w, name)
        assert (p.gain, p.rangetype, p.scaletype, p.signtype) == (g, r, s, sg), name
    p = spec_image_params(h, w, "abs", range="dcs", scale="linear", sign="retain", gain="reference")
    assert (p.gain, p.rangetype, p.scaletype, p.signtype) == (127.5 * 1024, 2, 1, 3)
    assert spec_image_params(h, w, "flat", gain=3.5).gain == 3.5 and spec_image_params(h, w, "copy", gain="native").gain == native
    assert spec_image_params(h, w).gain == sr.native_gain(h, w)


# ---- the sweeps' sample arithmetic on the CPU ----
POINTWISE = r'''
#include "spec_image_core.h"
using namespace dspfft;
extern "C" void enc(const float *f, uint64_t len, int d, double gain, int r, int s, int g, uint8_t *out, uint8_t *smap, double *dc)
{
	SpecImageEnc a; a.f = f; a.out = out; a.signmap = smap; a.dc = dc; a.len = len; a.d = d; a.gain = gain; a.rangetype = r; a.scaletype = s; a.signtype = g;
	float m[SPEC_IMAGE_MAX_CH];
	spec_image_divisors(m, f, d, gain, r, s);
	for (int z = 0; z < d; z++) dc[z] = (double)f[z];
	for (uint64_t i = 0; i < len; i++) spec_image_encode_at(a, m, i, (int)(i % d), out[i], smap[i]);
}
extern "C" void dec(const uint8_t *in, const uint8_t *map, uint64_t len, int d, double gain, int r, int s, int g, const double *dc, int restore, float *out)
{
	SpecImageDec a; a.in = in; a.signmap = map; a.f = out; a.len = len; a.d = d; a.gain = gain; a.scaletype = s; a.signtype = g; a.restore_dc = restore;
	for (int z = 0; z < SPEC_IMAGE_MAX_CH; z++) { a.mx[z] = 0; a.dc[z] = dc && z < d ? dc[z] : 0; }
	spec_image_decode_max(a.mx, a.dc, d, gain, r, s);
	for (uint64_t i = 0; i < len; i++) out[i] = spec_image_decode_at(a, i, (int)(i % d), in[i], map ? map[i] : 0);
}
'''


def build(tmp_path_factory, name, text):
    d = tmp_path_factory.mktemp(name)
    src, so = d / "core.cpp", d / "core.so"
    src.write_text(text)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", CSRC, str(src), "-o", str(so)])
    return C.CDLL(str(so))


@pytest.fixture(scope="module")
def pointwise(tmp_path_factory):
    lib = build(tmp_path_factory, "spec_image_core", POINTWISE)
    lib.enc.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dec.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.enc.restype = lib.dec.restype = None
    return lib


def oracle():
    O = ol.lib()
    O.oracle_spec_encode_f32.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int]
    O.oracle_ispec_decode_f32.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    return O


def lround_bytes(e):
    """clamp(lround(255 e)) on the FLOAT e the spectrogram holds, the product taken in double (as the 8-bit writer)"""
    p = e.astype(np.float64) * 255.0
    return np.clip(np.where(p >= 0, np.floor(p + 0.5), -np.floor(-p + 0.5)), 0, 255).astype(np.uint8)


def coefficients(c):
    """uniform-range coefficients of a 40 x 24 image (w x h) as the plan leaves them: float"""
    img = ol.synth_u8(0xC0EF + c, 24 * 40 * c).reshape(24, 40, c)
    return sr.coeffs64(img).astype(np.float32)


@pytest.mark.parametrize("c", [1, 3])
def test_encode_bytes_sign_map_and_dc_are_the_oracles(pointwise, c):
    O = oracle()
    f = coefficients(c)
    n = f.size
    gain = sr.native_gain(24, 40)
    for (rng, scale, sign) in sr.ALL_CODES:
        for g in (gain, 1.0):
            out, smap, dc = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(c)
            pointwise.enc(f.ctypes.data, n, c, g, rng, scale, sign, out.ctypes.data, smap.ctypes.data, dc.ctypes.data)
            e = f.copy()
            O.oracle_spec_encode_f32(e.ctypes.data, 24 * 40, c, g, rng, scale, sign)
            assert np.array_equal(out, lround_bytes(e.reshape(-1))), (rng, scale, sign, g)
            assert len(np.unique(out)) > (20 if scale == 0 and sign < 2 and g == gain else 1)
            # the `sign` preset's image (spec.h:75): the first pixel byte(f), everywhere else 255 * !signbit(f)  (ispec.c:92-95 reads it back)
            s = f.copy()
            O.oracle_spec_encode_f32(s.ctypes.data, 24 * 40, c, 1.0, 0, 1, 2)
            assert np.array_equal(smap, lround_bytes(s.reshape(-1)))
            flat = f.reshape(-1)
            assert np.array_equal(smap[c:], np.where(np.signbit(flat[c:]), 0, 255)) and np.array_equal(smap[:c], lround_bytes(flat[:c]))
            assert np.array_equal(dc, flat[:c].astype(np.float64))


@pytest.mark.parametrize("c", [1, 3])
def test_decode_floats_are_the_composition_of_the_oracle_functions(pointwise, c):
    O = oracle()
    n = 24 * 40 * c
    b = ol.synth_u8(0xDEC0 + c, n)
    smap = ol.synth_u8(0x51A9 + c, n)
    smap[3 * c] = 128                                                   # tmp[i] - 128 == 0: copysign(+0) keeps the magnitude positive
    dc = np.array([0.43, 0.51, 0.47][:c])
    gain = sr.native_gain(24, 40)
    for (rng, scale, sign) in sr.ALL_CODES:
        for restore in (0, 1):
            for use_map in ((False, True) if sign == 0 else (False,)):
                got = np.zeros(n, np.float32)
                pointwise.dec(b.ctypes.data, smap.ctypes.data if use_map else None, n, c, gain, rng, scale, sign, dc.ctypes.data, restore, got.ctypes.data)
                want = (b.astype(np.float64) / 255.0).astype(np.float32)
                if use_map:
                    want[c:] = np.copysign(want[c:], (smap[c:].astype(np.int32) - 128).astype(np.float32))           # ispec.c:94-95
                O.oracle_ispec_decode_f32(want.ctypes.data, 24 * 40, c, gain, rng, scale, sign, dc.ctypes.data, restore)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rng, scale, sign, restore, use_map)
                if use_map:
                    assert (got[c:] < 0).any() and (got[c:] > 0).any() and got[3 * c] >= 0


def test_the_float64_reference_leaves_few_saturate_samples_undecided():
    """the GPU test leaves out of its saturate comparisons the samples with |f_ref| <= 1e-5 max|f_ref|: at most 1 % on every input it uses"""
    for shape in sr.SHAPES:
        u = sr.saturate_undecided(sr.coeffs64(sr.image(shape)))
        print(f"{sr.shape_id(shape)}: {int(u.sum())} of {u.size} samples undecided ({u.mean():.4%})")
        assert u.mean() <= 0.01, shape


def test_the_float64_chain_inverts_itself():
    """spec_image_ref's decode64 undoes its encode64 (without the rounding to bytes): the reference the GPU tests compare with is one chain"""
    img = sr.image((24, 40, 3))
    f = sr.coeffs64(img)
    gain = sr.native_gain(24, 40)
    for (rng, scale, sign) in ((0, 0, 1), (2, 1, 3), (1, 0, 1)):
        e, _ = sr.encode64(f.copy(), gain, rng, scale, sign)
        dc = f.reshape(-1, 3)[0]
        p = ol.dct2d_interleaved(sr.decode64_values(e, None, gain, rng, scale, sign, dc, 0), ol.REDFT01, impl="port", threads=4)
        assert np.abs(p * 255.0 - img).max() < 1e-6


# ---- the 8-bit ends of interleaved RGB lines, phase by phase on the CPU ----
ROWS = r'''
#include <math.h>
#include <string.h>
#include <vector>
#include "dct_spec.h"
using namespace dspfft;
template <class S, int KIND>
static void walk(const PassArgs &a, const U8IO *io, int nlines)
{
	std::vector<unsigned char> lds(S::LDS + 32);
	cf *planes = (cf *)(((uintptr_t)lds.data() + 31) & ~(uintptr_t)31);
	for (int wg = 0; wg < nlines; wg++) {
		std::vector<typename S::template State<KIND>> st(S::T);
		long long bin, bout;
		row_base(a, wg, bin, bout);
		for (int tid = 0; tid < S::T; tid++) S::template prefetch<KIND>(a, bin, tid, st[tid], io);
		static_for<0, S::NPH>([&](auto ph) { for (int tid = 0; tid < S::T; tid++) S::template phase<KIND, ph>(a, planes, bout, tid, st[tid], io); });
	}
}
template <class S>
static int run(int kind, int u8, int nlines, const uint8_t *in8, const float *in, float *out, uint8_t *out8, double mul, float scale, float in0, float out0)
{
	const int N = S::N, L = N / 2;
	const long double pi = 3.14159265358979323846264338327950288L;
	std::vector<cf> T(N + 1), W(L);
	for (int j = 0; j <= N; j++) T[j] = cmk<float>((float)cosl(pi * j / (2.0L * N)), (float)-sinl(pi * j / (2.0L * N)));
	for (int t = 0; t < L; t++) W[t] = cmk<float>((float)cosl(2 * pi * t / L), (float)-sinl(2 * pi * t / L));
	PassArgs a;
	memset((void *)&a, 0, sizeof a);
	a.N = N; a.kind = kind; a.C = 3; a.LPW = 1; a.nlines = nlines; a.nb0 = nlines; a.nb1 = 1;
	a.sb0_in = a.sb0_out = 3LL * N;
	a.in = in; a.out = out; a.T = T.data(); a.W = W.data(); a.scale = scale; a.in_scale0 = in0; a.out_scale0 = out0;
	U8IO io; io.in = in8; io.out = out8; io.mul = mul;
	typedef RowU8Rgb<S> U;
	static_assert(sizeof(typename U::template State<KIND_REDFT01>) == sizeof(typename S::template State<KIND_REDFT01>), "the REDFT01 load is the plain line's");
	if (kind == KIND_REDFT10) { if (u8) walk<U, KIND_REDFT10>(a, &io, nlines); else walk<S, KIND_REDFT10>(a, nullptr, nlines); }
	else { if (u8) walk<U, KIND_REDFT01>(a, &io, nlines); else walk<S, KIND_REDFT01>(a, nullptr, nlines); }
	return 0;
}
extern "C" int rows(int N, int kind, int u8, int nlines, const uint8_t *in8, const float *in, float *out, uint8_t *out8, double mul, float scale, float in0, float out0)
{
	if (N == 256) return run<RowSpec<256, 3, 192, 8, 16>>(kind, u8, nlines, in8, in, out, out8, mul, scale, in0, out0);
	if (N == 512) return run<RowSpec<512, 3, 64, 16, 16>>(kind, u8, nlines, in8, in, out, out8, mul, scale, in0, out0);
	return -1;
}
'''


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    lib = build(tmp_path_factory, "row_u8_rgb", ROWS)
    lib.rows.argtypes = [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_double, C.c_float, C.c_float, C.c_float]
    return lib


def test_the_instantiated_lines_are_the_row_lists_entries():
    """the shim above names the radices and thread counts of spec_list.h's 256 x 3 and 512 x 3 entries"""
    text = open(os.path.join(CSRC, "spec_list.h")).read()
    assert "X(256, 3, 192, 8, 16)" in text and "X(512, 3, 64, 16, 16)" in text


@pytest.mark.parametrize("N", [256, 512])
def test_rgb_lines_read_bytes_as_the_float_line_reads_their_floats(rows, N):
    nlines = 3
    b = ol.synth_u8(0x8B17 + N, nlines * N * 3)
    f = b.astype(np.float32)
    scale, in0, out0 = 1.0 / (255.0 * 2 * N), 1.0, 1.0 / math.sqrt(2.0)
    want, got = np.zeros(b.size, np.float32), np.zeros(b.size, np.float32)
    assert rows.rows(N, 0, 0, nlines, None, f.ctypes.data, want.ctypes.data, None, 1.0, scale, in0, out0) == 0
    assert rows.rows(N, 0, 1, nlines, b.ctypes.data, None, got.ctypes.data, None, 1.0, scale, in0, out0) == 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and the line is the transform: DCT-II of every channel of every line, in double
    x = b.astype(np.float64).reshape(nlines, N, 3)
    k, n = np.arange(N)[:, None], np.arange(N)[None, :]
    ref = np.einsum("kn,lnc->lkc", 2 * np.cos(np.pi * k * (2 * n + 1) / (2 * N)), x) * scale
    ref[:, 0, :] *= out0
    assert np.abs(got.reshape(nlines, N, 3) - ref).max() <= 1e-5 * np.abs(ref).max()


@pytest.mark.parametrize("N", [256, 512])
def test_rgb_lines_write_the_bytes_of_the_quantised_float_line(rows, N):
    nlines = 3
    # coefficients whose REDFT01 line is a picture line: the DCT-II of bytes, with ispec's factors; mul = 255 on pixels 0..1
    x = ol.synth_u8(0x8B18 + N, nlines * N * 3).astype(np.float64).reshape(nlines, N, 3) / 255.0
    k, n = np.arange(N)[:, None], np.arange(N)[None, :]
    coef = np.einsum("kn,lnc->lkc", 2 * np.cos(np.pi * k * (2 * n + 1) / (2 * N)), x) / (2.0 * N)
    coef[:, 0, :] /= 2.0
    # push some pixels past both ends of the byte range and next to rounding boundaries
    coef[:, 0, :] *= np.array([0.9, 1.0, 1.3])[None, :]
    f = np.ascontiguousarray(coef, dtype=np.float32).reshape(-1)
    want, got = np.zeros(f.size, np.float32), np.full(f.size, 77, np.uint8)
    for (scale, in0) in ((1.0, 2.0), (0.5, math.sqrt(2.0))):
        assert rows.rows(N, 1, 0, nlines, None, f.ctypes.data, want.ctypes.data, None, 255.0, scale, in0, 1.0) == 0
        assert rows.rows(N, 1, 1, nlines, None, f.ctypes.data, None, got.ctypes.data, 255.0, scale, in0, 1.0) == 0
        p = want.astype(np.float64) * 255.0
        q = np.where(p > 255.0, 255, np.where(p < 0.0, 0, np.floor(np.abs(p) + 0.5))).astype(np.uint8)      # quantise_u8: dspfft_f32_to_u8's
        assert np.array_equal(got, q), int((got != q).sum())
        if scale == 1.0:
            assert np.abs(p.reshape(nlines, N, 3)[..., 1] - x[..., 1] * 255.0).max() < 1e-2      # (the line is the inverse transform)
            assert (q == 255).any() and (q == 0).any() and len(np.unique(q)) == 256
