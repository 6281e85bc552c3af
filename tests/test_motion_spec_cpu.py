"""motion --spectrogram / --ispectrogram as one fused call (block_spec.hip, motion_ops.hip), the parts that need no device: the new symbols,
the emulation library's -3 (the kernels are HIP-only), the product library's refusals ahead of any launch, the Python helpers, and the two
new phases (dspfun_amd/csrc/block_spec_core.h) compiled with g++ and run thread by thread, between the existing phases of block_core.h,
against the float64 reference block by block (tests/motion_spec_ref.py)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import motion_grid_ref as gr
import motion_spec_ref as sr
import oracle_lib as ol
from dspfun_amd import _lib
from dspfun_amd.engine import Plan, DspfftError, REDFT01, REDFT10, motion_spec_constants, _spec_params

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned address for calls that are refused before anything reads it
EXEC = ("dspfft_execute_spectrogram_u8", "dspfft_execute_spectrogram_f32", "dspfft_execute_ispectrogram_u8", "dspfft_execute_ispectrogram_f32")
BLOCKS = ("dspfft_motion_spec_blocks_u8", "dspfft_motion_spec_blocks_f32", "dspfft_motion_ispec_blocks_u8", "dspfft_motion_ispec_blocks_f32")


def test_the_new_symbols_exist_and_the_emulation_library_answers_minus_3_writing_nothing():
    from emul_lib import emul
    prod = C.CDLL(_lib.LIB_PATH)
    for name in EXEC + BLOCKS:
        assert hasattr(prod, name), name
    L = emul()
    for name in EXEC:
        assert hasattr(L, name), name
    block, vol = sr.SHAPES[1]
    k = motion_spec_constants(block)
    n = int(np.prod(vol))
    for inverse, kind in ((False, REDFT10), (True, REDFT01)):
        p = sr.volume_plan(block, vol, kind, L)
        assert "BLOCK 8x8x8" in p.describe()
        frame = Plan.many_r2r([24, 40], [kind] * 2, howmany=3, idist=960, odist=960, lib=L)        # no small-block plan: the other path
        for plan, count in ((p, n), (frame, 3 * 960)):
            for pixels, dt in (("u8", np.uint8), ("f32", np.float32)):
                src = ol.synth_u8(5, count).astype(dt)
                out = np.full(count, 9, dtype=dt)
                work = np.full(count, 7.0, dtype=np.float32)
                run = plan.ispectrogram if inverse else plan.spectrogram
                with pytest.raises(DspfftError, match="not built into this library"):
                    run(src.ctypes.data, out.ctypes.data, "shift", k["scalefactor"], k["normalization"], k["c"], d_work=work.ctypes.data, pixels=pixels)
                sp = _spec_params("shift", k["scalefactor"], k["normalization"], k["c"])
                fn = getattr(L, ("dspfft_execute_ispectrogram_" if inverse else "dspfft_execute_spectrogram_") + pixels)
                args = (plan._h, src.ctypes.data, out.ctypes.data, work.ctypes.data, C.byref(sp), None) + ((1.0,) if inverse else ()) + (None, None)
                assert fn(*args) == -3
                assert np.all(out == 9) and np.all(work == 7.0)


def test_refusals_of_the_product_library_come_before_any_launch():
    """plans of 4-, 8- and 16-point axes need no device tables, so the product library plans them here"""
    L = _lib.load()
    err = L.dspfft_last_error
    block, vol = sr.SHAPES[1]
    k = motion_spec_constants(block)
    fwd, inv = sr.volume_plan(block, vol, REDFT10, L), sr.volume_plan(block, vol, REDFT01, L)
    sp = lambda mode: C.byref(_spec_params(mode, k["scalefactor"], k["normalization"], k["c"]))
    S8, Sf, I8, If = (getattr(L, n) for n in EXEC)
    # abs has no inverse type
    assert I8(inv._h, FAKE, FAKE, None, sp("abs"), None, 1.0, None, None) == -2 and b"no abs type" in err()
    assert If(inv._h, FAKE, FAKE, None, sp("abs"), None, 1.0, None, None) == -2 and b"no abs type" in err()
    # float buffers off 16 bytes, 8-bit buffers off 4
    for a, b in ((4096 + 2, 4096), (4096, 4096 + 1)):
        assert S8(fwd._h, C.c_void_p(a), C.c_void_p(b), None, sp("abs"), None, None, None) == -2 and b"aligned" in err()
        assert I8(inv._h, C.c_void_p(a), C.c_void_p(b), None, sp("flat"), None, 1.0, None, None) == -2 and b"aligned" in err()
    for a, b in ((4096 + 4, 4096), (4096, 4096 + 8)):
        assert Sf(fwd._h, C.c_void_p(a), C.c_void_p(b), None, sp("copy"), None, None, None) == -2 and b"aligned" in err()
        assert If(inv._h, C.c_void_p(a), C.c_void_p(b), None, sp("copy"), None, 1.0, None, None) == -2 and b"aligned" in err()
    # an f64 plan
    f64 = Plan.many_r2r([8, 8, 8], [REDFT10] * 3, howmany=4, idist=512, odist=512, lib=L, dtype="f64")
    assert S8(f64._h, FAKE, FAKE, FAKE, sp("abs"), None, None, None) == -2 and b"f64" in err()
    assert If(f64._h, FAKE, FAKE, FAKE, sp("flat"), None, 1.0, None, None) == -2 and b"f64" in err()
    # (a plan with a transfer characteristic: setting one needs the device, tests/test_motion_spec_gpu.py)
    # (not refusals of the -2 kind, but also ahead of any launch: a mode that is none, the wrong kind of plan, a missing work buffer)
    assert S8(fwd._h, FAKE, FAKE, None, sp("none"), None, None, None) == -1 and b"mode" in err()
    assert S8(inv._h, FAKE, FAKE, None, sp("abs"), None, None, None) == -1 and b"REDFT10" in err()
    assert I8(fwd._h, FAKE, FAKE, None, sp("flat"), None, 1.0, None, None) == -1 and b"REDFT01" in err()
    with pytest.raises(DspfftError, match="f64"):
        f64.spectrogram(4096, 4096, "abs", 1.0, 1.0)


def test_motion_spec_constants_are_motions():
    for block in ((8, 8, 8), (1, 32, 32), (4, 8, 16)):
        k = motion_spec_constants(block)
        sf, nm, c = sr.constants(block)
        assert k["scalefactor"] == sf == 1.0 and k["normalization"] == pytest.approx(nm, rel=1e-15)
        assert k["c"] == pytest.approx(c, rel=1e-15) and k["ic"] == k["c"]
    k = motion_spec_constants((8, 8, 8), (4, 4, 4))
    assert k["scalefactor"] == 0.125 and k["normalization"] == 1 / math.sqrt(64 * 8) and k["c"] == pytest.approx(127.5 / math.log1p(64 * k["normalization"] * 255 * 8))


# ---- the header's phases on the CPU: a test-only shim that lays out the geometry the engine derives and walks tid 0..255 through every phase ----
CPP = r'''
#include <stdint.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "block_spec_core.h"
using namespace dspfft;
template <int NX, int NY, int NZ, bool U8>
static void walk(const BlockSpecArgs &a, int inverse, int nwg, float *lds, size_t tile, unsigned long long &mine)
{
	for (int wg = 0; wg < nwg; wg++) {
		long long bin, bout; int cnt;
		block_base(a, (uint32_t)wg, bin, bout, cnt);
		for (size_t i = 0; i < tile; i++) lds[i] = NAN;                                    // what no phase writes must never be read
#define ALL for (int tid = 0; tid < BLOCK_THREADS; tid++)
		if (!inverse) {
			ALL block_load_x<NX, NY, NZ, KIND_REDFT10, U8>(a, block_axis_args(a.s, 0, false), a.in, a.in8, lds, bin, cnt, tid);
			ALL block_lines_y<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.s, 1, NZ == 1), lds, cnt, tid);
			ALL block_lines_z<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.s, 2, true), lds, cnt, tid);
			ALL block_spec_store<NX, NY, NZ, U8>(a, lds, bout, cnt, tid, mine);
		} else {
			ALL block_ispec_load<NX, NY, NZ, U8>(a, lds, bin, cnt, tid, mine);
			ALL block_lines_z<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.s, 2, false), lds, cnt, tid);
			ALL block_lines_y<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.s, 1, false), lds, cnt, tid);
			ALL block_store_x<NX, NY, NZ, KIND_REDFT01, U8>(a, block_axis_args(a.s, 0, true), a.out, a.out8, a.mul8, lds, bout, cnt, tid);
		}
	}
}
struct dspfft_like_filter { int active[3], minbuf_hw[2], block_depth, band_begin[3], band_end[3]; float damp, boost, threshold_lo, threshold_hi; int preserve_dc; float grey_add, quantizer; };
// in / out: float or 8-bit pixels (the other pair NULL); the blocks of a [D][H][W] volume, or a block-major stack
extern "C" int run(int inverse, const float *in, const uint8_t *in8, float *out, uint8_t *out8, const int *nblocks, const int *block, int block_major, int G,
                   int mode, double scalefactor, double norm, double c, double out_mul, const dspfft_like_filter *fp, unsigned long long *coded)
{
	const int nd = nblocks[0], nh = nblocks[1], nw = nblocks[2], bd = block[0], bh = block[1], bw = block[2];
	const long long H = (long long)nh * bh, W = (long long)nw * bw;
	BlockSpecArgs a;
	memset((void *)&a, 0, sizeof a);
	a.nx = bw; a.ny = bh; a.nz = bd; a.G = G; a.pitch = G * bw;
	if (block_major) {
		a.rows_fast = 1; a.nxb = nd * nh * nw; a.nd = 0;
		a.sy_in = a.sy_out = bw; a.sz_in = a.sz_out = (long long)bh * bw; a.sxb_in = a.sxb_out = (long long)bd * bh * bw;
	} else {
		a.rows_fast = 0; a.nxb = nw; a.nd = 2;
		a.sy_in = a.sy_out = W; a.sz_in = a.sz_out = H * W; a.sxb_in = a.sxb_out = bw;
		a.bn[0] = nh; a.bis[0] = a.bos[0] = bh * W;
		a.bn[1] = nd; a.bis[1] = a.bos[1] = bd * H * W;
		for (int d = 0; d < 2; d++) a.bdiv[d] = motion_filter_div((uint32_t)a.bn[d]);
	}
	a.ngroups = (a.nxb + G - 1) / G; a.gdiv = motion_filter_div((uint32_t)a.ngroups);
	int nwg = a.ngroups;
	for (int d = 0; d < a.nd; d++) nwg *= a.bn[d];
	a.in = in; a.in8 = in8; a.out = out; a.out8 = out8; a.mul8 = out_mul;
	// motion's scales (motion.c:644-647,748-751); a unit axis of the reference's 3-D plans doubles on the way forward and is divided by sqrt 2
	const float r2 = sqrtf(2.f), unit = bd == 1 ? r2 : 1.f;
	double scale = inverse ? unit / (2 * r2) : 2 * r2 * unit;
	if (!in8) scale = inverse ? scale * out_mul / 255.0 : scale * 255.0;                    // float pixels: the engine's fold (spec_block)
	a.s.scale = (float)scale;
	for (int k = 0; k < 3; k++) { const bool on = k < 2 || bd > 1; a.s.in0[k] = inverse && on ? r2 : 1.f; a.s.out0[k] = !inverse && on ? 1.f / r2 : 1.f; }
	if (fp) motion_filter_from(*fp, a.filt);
	a.sp = MotionSpec{mode, scalefactor, norm, c};
	const size_t tile = (size_t)bd * bh * a.pitch;
	std::vector<float> raw(tile + 8, NAN);
	float *lds = (float *)(((uintptr_t)raw.data() + 15) & ~(uintptr_t)15);
	unsigned long long mine = 0;
#define CASE(X_, Y_, Z_) if (bw == X_ && bh == Y_ && bd == Z_) { if (in8) walk<X_, Y_, Z_, true>(a, inverse, nwg, lds, tile, mine); else walk<X_, Y_, Z_, false>(a, inverse, nwg, lds, tile, mine); if (coded) *coded += mine; return nwg; }
	CASE(4, 4, 4) CASE(8, 8, 8) CASE(16, 8, 4) CASE(16, 16, 16) CASE(32, 32, 1) CASE(4, 4, 1)
	return -1;
}
// the 8-bit encode of n coefficients three ways: the double line, the line the kernels run (fast where it decides), and whether fast decided
extern "C" void encode(const float *v, long long n, int mode, double scalefactor, double norm, double c, uint8_t *exact, uint8_t *used, uint8_t *decided)
{
	const MotionFast f = motion_fast_of(mode, scalefactor, norm, c);
	for (long long i = 0; i < n; i++) {
		uint32_t b = 0;
		exact[i] = (uint8_t)motion_pel_u8(motion_store_pel((double)v[i], mode, scalefactor, norm, c));
		used[i] = (uint8_t)motion_spec_byte(v[i], mode, scalefactor, norm, c, f);
		decided[i] = f.on && motion_store_u8_fast(v[i], mode, f, b);
	}
}
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("block_spec_core")
    src, so = d / "core.cpp", d / "core.so"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "dspfun_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.run.argtypes = [C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int] + [C.c_double] * 4 + [C.POINTER(_lib.MotionFilterParams), C.c_void_p]
    lib.encode.argtypes = [C.c_void_p, C.c_longlong, C.c_int] + [C.c_double] * 3 + [C.c_void_p] * 3
    lib.encode.restype = None
    return lib


def encode(core, v, mode, sf, nm, c):
    v = np.ascontiguousarray(v, dtype=np.float32)
    exact, used, decided = (np.zeros(v.size, dtype=np.uint8) for _ in range(3))
    core.encode(v.ctypes.data, v.size, _lib_mode(mode), sf, nm, c, exact.ctypes.data, used.ctypes.data, decided.ctypes.data)
    return exact, used, decided


@pytest.mark.parametrize("mode", ["abs", "shift"])
@pytest.mark.parametrize("c", [8.0, 25.0, 60.0])
def test_the_single_precision_encode_gives_the_double_lines_byte_for_every_coefficient(core, mode, c):
    """motion_filter.h motion_spec_byte against motion_pel_u8(motion_store_pel(...)) on the same float coefficient and constants: 2^22
    coefficients spaced evenly in log|pel| over [1e-6, 1e6], both signs, and the 64 floats on either side of every coefficient at which the
    double line's byte changes (found by bisection on the double line over all floats of each sign): equal bytes, with the fast line
    deciding all but a few of the log-spaced ones (away from the boundaries the test is not vacuous) and the specials"""
    sf, nm, _ = sr.constants((8, 8, 8))
    m = sf * nm
    n = 1 << 21
    pel = np.exp(np.linspace(np.log(1e-6), np.log(1e6), n))
    v = np.concatenate([pel / m, -pel / m]).astype(np.float32)
    exact, used, decided = encode(core, v, mode, sf, nm, c)
    assert np.array_equal(exact, used), int((exact != used).sum())
    # (shift: a negative pel below 2^-12 / c lies next to 127.5 on the side where the sign alone does not decide; a sixteenth of this range)
    assert decided.mean() > (0.995 if mode == "abs" else 0.9) and len(np.unique(exact)) > 100
    top = np.float32(np.finfo(np.float32).max).view(np.uint32)
    for sign in (1.0, -1.0):
        val = lambda bits: (np.asarray(bits, dtype=np.uint32).view(np.float32) * np.float32(sign))
        lo_b, hi_b = (int(encode(core, val([b]), mode, sf, nm, c)[0][0]) for b in (0, top))
        up = hi_b >= lo_b                                           # the byte is monotone in |v|: rising, or falling for shift's negative side
        levels = np.arange(min(lo_b, hi_b) + 1, max(lo_b, hi_b) + 1)
        assert len(levels) >= 127
        lo, hi = np.zeros(len(levels), dtype=np.int64), np.full(len(levels), int(top), dtype=np.int64)      # smallest bits whose byte has crossed the level
        while np.any(lo < hi):
            mid = (lo + hi) // 2
            b = encode(core, val(mid), mode, sf, nm, c)[0].astype(int)
            crossed = (b >= levels) if up else (b <= levels - 1)
            hi = np.where(crossed, mid, hi)
            lo = np.where(crossed, lo, mid + 1)
        bits = np.clip(lo[:, None] + np.arange(-64, 64)[None, :], 0, int(top)).ravel()
        exact, used, decided = encode(core, val(bits), mode, sf, nm, c)
        assert len(np.unique(exact)) >= len(levels)
        assert np.array_equal(exact, used), (sign, int((exact != used).sum()))
        assert decided.mean() < 1                                   # the double line ran (next to a boundary the fast line rarely decides)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 3e38, -3e38, 1e-45, -1e-45, 1e-38, 1.0, -1.0], dtype=np.float32)
    exact, used, _ = encode(core, special, mode, sf, nm, c)
    assert np.array_equal(exact, used)


def engine_G(block, nxb):
    d, h, w = block
    return max(1, min(256 // w, 4096 // (d * h * w), nxb))


def run_core(core, inverse, pix, block, mode, block_major=False, filt=None, G=None):
    """pix: a [D][H][W] volume, uint8 or float32.  Returns (the output volume in the same type, the coded count)."""
    nbk = sr.nblocks_of(block, pix.shape)
    u8 = pix.dtype == np.uint8
    src = np.ascontiguousarray(gr.to_blocks(pix, block) if block_major else pix)
    out = np.zeros_like(src)
    coded = np.zeros(1, dtype=np.uint64)
    sf, nm, c = sr.constants(block)
    ia = lambda v: (C.c_int * 3)(*v)
    nxb = int(np.prod(nbk)) if block_major else nbk[2]
    G = G or engine_G(block, nxb)
    fp = Plan._filter_params(filt)
    nwg = core.run(int(inverse), None if u8 else src.ctypes.data, src.ctypes.data if u8 else None, None if u8 else out.ctypes.data, out.ctypes.data if u8 else None,
                   ia(nbk), ia(block), int(block_major), G, _lib_mode(mode), sf, nm, c, sf * nm * nm, C.byref(fp) if fp is not None else None, coded.ctypes.data)
    assert nwg == -(-nxb // G) * (1 if block_major else nbk[0] * nbk[1])
    return (gr.from_blocks(out, block, nbk) if block_major else out), int(coded[0])


def _lib_mode(mode):
    return {"abs": 1, "shift": 2, "flat": 3, "copy": 4}[mode]


# The bytes against the float64 reference.  No byte may differ by more than 1; the share that differs is bounded from the arithmetic: a byte
# differs where the reference's pel lies closer to a rounding boundary than the float pipeline's error e (in bytes), which happens to a share
# 2 e of uniformly placed pels.  Forward: the samples are 8-bit integers, so the sums that carry the block's DC are exact in float (below
# 2^24) and roundings arise at the twiddle products, on values of the AC coefficients' magnitude: a coefficient's error is about 8 roundings
# of the largest AC coefficient, in pels (p = coefficient x scalefactor x normalization) e_p ~ 8 x 2^-24 x 40 = 2e-5 for this noise (AC pels
# have a standard deviation of about 7).  abs / shift scale it by the encode's slope c / (1 + |p|) <= c <= 255 / log1p(|DC pel|) < 64 for the
# DCs of these volumes (asserted: DC pel > 53): e <= 1.2e-3 bytes, a share <= 0.25 %; flat and copy by normalization / 2 and normalization,
# <= 1 / sqrt(128): less.  That bound takes the largest coefficient's error at the steepest slope for every sample; the cap is two thirds of
# it, 0.17 %, plus 4 bytes (small volumes).  Inverse: the roundtrip's store of a transform whose input is exact to an ulp: the share that
# tests/test_motion_block_rescale_cpu.py allows the same arithmetic, 0.5 %.
SPEC_SHARE, ISPEC_SHARE, EXTRA_BYTES = 0.0017, 0.005, 4
# float pixels against max|ref|: the same errors without the rounding, e / 255 of a full-scale sample and far less of max|ref| >= 1
FLOAT_REL = 1e-4


def check_bytes(got, ref, share, what, tie=None):
    """tie: samples the comparison leaves out (motion_spec_ref.apply_filter: coefficients on a quantiser tie) -- at most the few that
    2 EDGE of uniformly placed quotients make, with room for their clustering"""
    diff = np.abs(got.astype(int) - ref.astype(int))
    if tie is not None:
        diff = diff[~tie]
    n = int((diff > 0).sum())
    print(f"{what}: max diff {diff.max()}, {n} of {diff.size} bytes differ ({n / diff.size:.5%}), cap {share:.3%} + {EXTRA_BYTES}")
    assert diff.max() <= 1 and n <= share * diff.size + EXTRA_BYTES, (what, int(diff.max()), n, diff.size)


@pytest.mark.parametrize("shape", sr.SHAPES, ids=[sr.shape_id(s) for s in sr.SHAPES])
@pytest.mark.parametrize("mode", sr.SPEC_MODES)
def test_spectrogram_phases_against_the_reference_block_by_block(core, shape, mode):
    block, vol_shape = shape
    sf, nm, _ = sr.constants(block)
    for kind in (None, "band", "full", "q"):
        ref = sr.spec_case(block, vol_shape, mode, kind)
        assert np.all(np.abs(ref["dc"] * sf * nm) > 53)
        got, coded = run_core(core, False, ref["vol"], block, mode, filt=ref["filt"])
        sr.check_tie_share(ref, False)
        check_bytes(got, ref["out8"], SPEC_SHARE, f"spectrogram {mode} {sr.shape_id(shape)} filter={kind}", ref["tie"])
        if kind in ("full", "q"):
            assert abs(coded - ref["coded"]) <= ref["tie"].sum() and coded > 0
        if kind != "q":
            for g in (1, 2):                # other groupings, the same bytes
                assert np.array_equal(run_core(core, False, ref["vol"], block, mode, filt=ref["filt"], G=g)[0], got)
        if sr.SHAPES.index(shape) in sr.BLOCK_MAJOR:
            gotb, codedb = run_core(core, False, ref["vol"], block, mode, block_major=True, filt=ref["filt"])
            assert np.array_equal(gotb, got) and codedb == coded
    # float pixels
    for kind in (None, "full"):
        ref = sr.spec_case(block, vol_shape, mode, kind, float_pixels=True)
        got, _ = run_core(core, False, sr.pixels_f32(ref["vol"]), block, mode, filt=ref["filt"])
        want = ref["pel"] / 255
        ok = slice(None) if ref["tie"] is None else ~ref["tie"]
        err = np.abs(got - want)[ok].max() / np.abs(want).max()
        print(f"spectrogram f32 {mode} {sr.shape_id(shape)} filter={kind}: max err / max|ref| {err:.2e}")
        assert err < FLOAT_REL


@pytest.mark.parametrize("shape", sr.SHAPES, ids=[sr.shape_id(s) for s in sr.SHAPES])
@pytest.mark.parametrize("mode", sr.ISPEC_MODES)
def test_ispectrogram_phases_against_the_reference_block_by_block(core, shape, mode):
    block, vol_shape = shape
    for kind in (None, "band", "full", "q"):
        ref = sr.ispec_case(block, vol_shape, mode, kind)
        got, coded = run_core(core, True, ref["pix"], block, mode, filt=ref["filt"])
        check_bytes(got, ref["out8"], ISPEC_SHARE, f"ispectrogram {mode} {sr.shape_id(shape)} filter={kind}", ref["tie"])
        assert 8 < got.mean() < 247, "an image, not a saturated plane"
        if kind in ("full", "q"):
            # (a decoded byte is one of 256 values: one of them near a tie recurs in many blocks, which the comparison then leaves out)
            assert ref["tie"].mean() < 0.5 and abs(coded - ref["coded"]) <= ref["nties"] * int(np.prod(block)) and coded > 0
        if sr.SHAPES.index(shape) in sr.BLOCK_MAJOR:
            gotb, codedb = run_core(core, True, ref["pix"], block, mode, block_major=True, filt=ref["filt"])
            assert np.array_equal(gotb, got) and codedb == coded
    ref = sr.ispec_case(block, vol_shape, mode, None, float_pixels=True)
    got, _ = run_core(core, True, ref["pix"], block, mode)
    want = ref["pel"] / 255
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"ispectrogram f32 {mode} {sr.shape_id(shape)}: max err / max|ref| {err:.2e}")
    assert err < FLOAT_REL
