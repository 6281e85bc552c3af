"""motion --spectrogram / --ispectrogram on packed 8-bit pixels (dspfft_execute_spectrogram_u8_packed, dspfft_execute_ispectrogram_u8_packed),
the parts that need no device: the new encoded ends (dspfun_amd/csrc/block_spec_packed_core.h) compiled with g++ and walked thread by thread
over a NaN-filled tile, the refusal of the emulation library (the kernels are HIP-only), the refusals of the product library ahead of any
launch, and engine.motion_packed_frame_plans.  The oracle of the phases needs no tolerance: every component block runs the planar kernel's
phase (block_spec_core.h), so the packed bytes (tile contents) equal the planar phase run on each de-interleaved component with that
component's filter, and the coded count their sum."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from dspfun_amd import _lib
from dspfun_amd.engine import (Plan, DspfftError, REDFT01, REDFT10, motion_grid_plans, motion_packed, motion_packed_frame_plans,
                               motion_spec_constants)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned address for calls that are refused before anything reads it
MODES = {"abs": 1, "shift": 2, "flat": 3, "copy": 4}


def planar_G(block):
    """build_block's rule for the blocks per workgroup of a planar plan whose row holds more blocks than that"""
    bd, bh, bw = block
    return max(1, min(256 // bw, 4096 // (bd * bh * bw)))


def next_prime(n):
    p = n + 1
    while any(p % q == 0 for q in range(2, int(p ** 0.5) + 1)):
        p += 1
    return p


def plain_packed(comps):
    p = _lib.MotionPacked()
    p.components = comps
    return p


def spec_params(mode, k):
    return _lib.MotionSpecParams(MODES[mode], k["scalefactor"], k["normalization"], k["c"])


# ---- the header's phases on the CPU: a test-only shim that lays out the geometry the engine derives and walks tid 0..255 through the encoded
# end, once with the planar phase on one plane and once with the packed phase on the interleaved clip ----
CPP = r'''
#include <stdint.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "block_spec_packed_core.h"
using namespace dspfft;
// C bytes per pixel (1: a planar plane); volume layout [D][H][W][C]
static int geom(BlockGeom &a, const int *nblocks, const int *block, int G, int C)
{
	const int nd = nblocks[0], nh = nblocks[1], nw = nblocks[2], bd = block[0], bh = block[1], bw = block[2];
	const long long H = (long long)nh * bh, W = (long long)nw * bw;
	a.nx = bw; a.ny = bh; a.nz = bd; a.G = G; a.pitch = G * C * bw;
	a.rows_fast = 0; a.nxb = nw; a.nd = 2;
	a.sy_in = W * C; a.sz_in = H * W * C; a.sxb_in = (long long)bw * C;
	a.bn[0] = nh; a.bis[0] = bh * W * C; a.bn[1] = nd; a.bis[1] = bd * H * W * C;
	for (int d = 0; d < 2; d++) { a.bos[d] = a.bis[d]; a.bdiv[d] = motion_filter_div((uint32_t)a.bn[d]); }
	a.sy_out = a.sy_in; a.sz_out = a.sz_in; a.sxb_out = a.sxb_in;
	a.ngroups = (a.nxb + G - 1) / G; a.gdiv = motion_filter_div((uint32_t)a.ngroups);
	return a.ngroups * nh * nd;
}
// fl: {quantizer, thr_lo, thr_hi}; bp: band begin (d, h, w), band end (d, h, w), preserve_dc
static void filter(MotionFilter &f, const int *block, const float *fl, const int *bp, float damp, float boost, float grey_add)
{
	f.ad = block[0]; f.ah = block[1]; f.aw = block[2]; f.mh = f.mw = 1;
	f.b0d = bp[0]; f.b0h = bp[1]; f.b0w = bp[2]; f.b1d = bp[3]; f.b1h = bp[4]; f.b1w = bp[5]; f.preserve_dc = bp[6];
	f.quantizer = fl[0]; f.thr_lo = fl[1]; f.thr_hi = fl[2]; f.damp = damp; f.boost = boost; f.grey_add = grey_add; f.enabled = 1;
	motion_filter_set_divs(f, 1);
}
static float *nan_tile(std::vector<float> &raw, size_t n)          // what no phase writes must never be read
{
	raw.assign(n + 8, NAN);
	return (float *)(((uintptr_t)raw.data() + 15) & ~(uintptr_t)15);
}
#define EACH_TID for (int tid = 0; tid < BLOCK_THREADS; tid++)
// the coefficients of a workgroup's cnt pixel blocks out of `coef` (the clip's layout, C floats per pixel) into their places of the tile
// (component-major: tile block c * cnt + g), and nothing else
static void fill_tile(const BlockGeom &a, const float *coef, float *lds, long long base, int cnt, int C)
{
	for (int z = 0; z < a.nz; z++) for (int y = 0; y < a.ny; y++) for (int g = 0; g < cnt; g++) for (int c = 0; c < C; c++) for (int x = 0; x < a.nx; x++)
		lds[(z * a.ny + y) * a.pitch + (c * cnt + g) * a.nx + x] = coef[base + (long long)g * a.sxb_out + (long long)z * a.sz_out + (long long)y * a.sy_out + (long long)C * x + c];
}
// ... and the other way: the tile's filled part into `coef`'s layout; returns how many floats OUTSIDE that part are no longer NaN
static long long drain_tile(const BlockGeom &a, float *coef, const float *lds, size_t tile, long long base, int cnt, int C)
{
	std::vector<char> seen(tile, 0);
	for (int z = 0; z < a.nz; z++) for (int y = 0; y < a.ny; y++) for (int g = 0; g < cnt; g++) for (int c = 0; c < C; c++) for (int x = 0; x < a.nx; x++) {
		const size_t at = (size_t)(z * a.ny + y) * a.pitch + (c * cnt + g) * a.nx + x;
		seen[at] = 1;
		coef[base + (long long)g * a.sxb_in + (long long)z * a.sz_in + (long long)y * a.sy_in + (long long)C * x + c] = lds[at];
	}
	long long stray = 0;
	for (size_t i = 0; i < tile; i++) if (!seen[i] && !isnan(lds[i])) stray++;
	return stray;
}
#define SHAPES(X) X(4, 4, 1) X(8, 8, 8) X(32, 32, 1)

template <int NX, int NY, int NZ>
static long long seq_planar(const BlockSpecArgs &a, int inverse, int nwg, const float *coef_in, float *coef_out, unsigned long long &mine)
{
	std::vector<float> raw;
	long long stray = 0;
	const size_t tile = (size_t)NZ * NY * a.pitch;
	for (int wg = 0; wg < nwg; wg++) {
		long long bin, bout; int cnt;
		block_base(a, (uint32_t)wg, bin, bout, cnt);
		float *lds = nan_tile(raw, tile);
		if (inverse) {
			EACH_TID block_ispec_load<NX, NY, NZ, true>(a, lds, bin, cnt, tid, mine);
			stray += drain_tile(a, coef_out, lds, tile, bin, cnt, 1);
		} else {
			fill_tile(a, coef_in, lds, bout, cnt, 1);
			EACH_TID block_spec_store<NX, NY, NZ, true>(a, lds, bout, cnt, tid, mine);
		}
	}
	return stray;
}
template <int NX, int NY, int NZ, int C>
static long long seq_packed(const BlockSpecPackedArgs &a, int inverse, int nwg, const float *coef_in, float *coef_out, unsigned long long &mine)
{
	std::vector<float> raw;
	long long stray = 0;
	const size_t tile = (size_t)NZ * NY * a.pitch;
	for (int wg = 0; wg < nwg; wg++) {
		long long bin, bout; int cnt;
		block_base(a, (uint32_t)wg, bin, bout, cnt);
		float *lds = nan_tile(raw, tile);
		if (inverse) {
			EACH_TID packed_ispec_load<NX, NY, NZ, C>(a, lds, bin, cnt, tid, mine);
			stray += drain_tile(a, coef_out, lds, tile, bin, cnt, C);
		} else {
			fill_tile(a, coef_in, lds, bout, cnt, C);
			EACH_TID packed_spec_store<NX, NY, NZ, C>(a, lds, bout, cnt, tid, mine);
		}
	}
	return stray;
}

extern "C" int group_of(int nx, int ny, int nz, int comps, int nxb) { return packed_group_of(nx, ny, nz, comps, nxb); }

// spectrogram's store (inverse = 0): coef -> pix; ispectrogram's load (inverse = 1): pix -> coef.  sp: mode, scalefactor, normalization, c.
// One plane through the planar phase; fl NULL: no filter; fl[3..5]: damp, boost, grey_add.  Returns the stray floats of the tiles, or -1.
extern "C" long long run_planar(int inverse, uint8_t *pix, float *coef, const int *nblocks, const int *block, int G, const double *sp, const float *fl, const int *bp,
                                unsigned long long *coded)
{
	BlockSpecArgs a;
	memset((void *)&a, 0, sizeof a);
	const int nwg = geom(a, nblocks, block, G, 1);
	a.in8 = pix; a.out8 = pix; a.sp = MotionSpec{(int)sp[0], sp[1], sp[2], sp[3]};
	if (fl) filter(a.filt, block, fl, bp, fl[3], fl[4], fl[5]);
	unsigned long long mine = 0;
#define CASE(X_, Y_, Z_) if (a.nx == X_ && a.ny == Y_ && a.nz == Z_) { const long long s = seq_planar<X_, Y_, Z_>(a, inverse, nwg, coef, coef, mine); *coded += mine; return s; }
	SHAPES(CASE)
#undef CASE
	return -1;
}
// the interleaved clip through the packed phase; fl[3..6]: damp, fl[7..10]: boost, fl[11..14]: grey_add, by byte position
extern "C" long long run_packed(int inverse, uint8_t *pix, float *coef, const int *nblocks, const int *block, int comps, int G, const double *sp, const float *fl, const int *bp,
                                unsigned long long *coded)
{
	BlockSpecPackedArgs a;
	memset((void *)&a, 0, sizeof a);
	const int nwg = geom(a, nblocks, block, G, comps);
	a.in8 = pix; a.out8 = pix; a.comps = comps; a.sp = MotionSpec{(int)sp[0], sp[1], sp[2], sp[3]};
	if (fl) {
		filter(a.filt, block, fl, bp, NAN, NAN, NAN);          // (the three scalar fields are not read)
		for (int c = 0; c < 4; c++) { a.damp[c] = fl[3 + c]; a.boost[c] = fl[7 + c]; a.grey_add[c] = fl[11 + c]; }
	}
	unsigned long long mine = 0;
#define CASE(X_, Y_, Z_) if (a.nx == X_ && a.ny == Y_ && a.nz == Z_) { \
		long long s; \
		if (comps == 2) s = seq_packed<X_, Y_, Z_, 2>(a, inverse, nwg, coef, coef, mine); else if (comps == 3) s = seq_packed<X_, Y_, Z_, 3>(a, inverse, nwg, coef, coef, mine); \
		else s = seq_packed<X_, Y_, Z_, 4>(a, inverse, nwg, coef, coef, mine); \
		*coded += mine; return s; }
	SHAPES(CASE)
#undef CASE
	return -1;
}
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("block_spec_packed_core")
    src, so = d / "core.cpp", d / "core.so"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "dspfun_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.group_of.argtypes = [C.c_int] * 5
    lib.run_planar.restype = lib.run_packed.restype = C.c_longlong
    lib.run_planar.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4
    lib.run_packed.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 4
    return lib


GUARD = 64          # bytes / floats on either side of a buffer that a phase writes


def guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    raw = np.full(n + 2 * GUARD, fill, dtype=dtype)
    return raw, raw[GUARD:GUARD + n].reshape(shape)


def untouched(raw, fill):
    edge = np.concatenate([raw[:GUARD], raw[-GUARD:]])
    return bool(np.all(np.isnan(edge))) if isinstance(fill, float) and math.isnan(fill) else bool(np.all(edge == fill))


def run_both(core, block, comps, inverse, mode, filt):
    """the packed phase on an interleaved clip and the planar phase on each of its planes with that component's filter values.  filt: None or
    (quantizer, thr_lo, thr_hi, damp[comps], boost[comps], grey_add[comps], band + preserve_dc).  2 x 2 x P blocks, P the smallest prime
    above the packed group size and the planar G: the last group of a row is short in both."""
    bd, bh, bw = block
    nb = (2, 2, next_prime(max(planar_G(block), core.group_of(bw, bh, bd, comps, 1 << 20))))
    shape = (nb[0] * bd, nb[1] * bh, nb[2] * bw)
    n = int(np.prod(shape))
    ia = lambda v: (C.c_int * len(v))(*v)
    k = motion_spec_constants(block)
    sp = (C.c_double * 4)(MODES[mode], k["scalefactor"], k["normalization"], k["c"])
    Gp = core.group_of(bw, bh, bd, comps, nb[2])
    assert 1 <= Gp <= nb[2] and nb[2] % Gp, "the last group of a row must be short"
    Gl = min(planar_G(block), nb[2])
    fl = bp = None
    if filt:
        q, lo, hi, damp, boost, grey, band = filt
        pad = lambda v: list(v) + [0.0] * (4 - len(v))
        fl = (C.c_float * 15)(q, lo, hi, *pad(damp), *pad(boost), *pad(grey))
        bp = ia(band)
    flc = lambda c: (C.c_float * 6)(fl[0], fl[1], fl[2], fl[3 + c], fl[7 + c], fl[11 + c]) if filt else None
    coded, want_coded = np.zeros(1, dtype=np.uint64), []
    if not inverse:
        # coefficients as a forward transform leaves them: a large positive DC per component block, small signed values elsewhere, some zeros
        rng = np.random.default_rng(0x5EC0 + comps + 16 * bd + bw)
        amp = AMP / k["normalization"] ** 2          # (flat and copy store coefficient * normalization^2 / 2 and * normalization^2)
        coef = (rng.standard_normal(shape + (comps,)) * amp).astype(np.float32)
        coef[rng.random(coef.shape) < 0.1] = 0.0
        coef[::bd, ::bh, ::bw, :] = ((rng.random((nb[0], nb[1], nb[2], comps)) * 10 + 3) * amp).astype(np.float32)
        raw, out = guarded(shape + (comps,), np.uint8, 0xEE)
        assert core.run_packed(0, out.ctypes.data, coef.ctypes.data, ia(nb), ia(block), comps, Gp, sp, fl, bp, coded.ctypes.data) == 0
        assert untouched(raw, 0xEE)
        want = np.empty_like(out)
        for c in range(comps):
            plane = np.ascontiguousarray(coef[..., c])
            rawc, o = guarded(shape, np.uint8, 0xEE)
            cn = np.zeros(1, dtype=np.uint64)
            assert core.run_planar(0, o.ctypes.data, plane.ctypes.data, ia(nb), ia(block), Gl, sp, flc(c), bp, cn.ctypes.data) == 0
            want[..., c] = o
            want_coded.append(int(cn[0]))
        return out, want, int(coded[0]), want_coded
    pix = ol.synth_u8(0x15C0 + comps + 16 * bd + bw, n * comps).reshape(shape + (comps,))
    raw, out = guarded(shape + (comps,), np.float32, float("nan"))
    # (a stray write inside a tile -- outside the cnt * C * NX columns of its rows -- is counted by the shim; so is every NaN that stays)
    assert core.run_packed(1, pix.ctypes.data, out.ctypes.data, ia(nb), ia(block), comps, Gp, sp, fl, bp, coded.ctypes.data) == 0
    assert untouched(raw, float("nan")) and not np.isnan(out).any()
    want = np.empty_like(out)
    for c in range(comps):
        plane = np.ascontiguousarray(pix[..., c])
        o = np.full(shape, np.nan, dtype=np.float32)
        cn = np.zeros(1, dtype=np.uint64)
        assert core.run_planar(1, plane.ctypes.data, o.ctypes.data, ia(nb), ia(block), Gl, sp, flc(c), bp, cn.ctypes.data) == 0
        want[..., c] = o
        want_coded.append(int(cn[0]))
    return out, want, int(coded[0]), want_coded


AMP = 30.0          # the spread of the store test's coefficients as flat's pels


def full_filter(block, comps, pdc, inverse):
    """a quantiser and a threshold that zero a good share of the coefficients (the store's are AMP / normalization^2 wide, the load's are
    what the decodes make of bytes: flat's and copy's of the same order, shift's far smaller -- most of those go)"""
    bd, bh, bw = block
    amp = AMP / motion_spec_constants(block)["normalization"] ** 2
    damp, boost, grey = [0.25, 0.5, 0.0, 0.75][:comps], [2.0, 1.0, 0.5, 1.5][:comps], [30 * amp, -10 * amp, 0.0, 5 * amp][:comps]
    band = [1 if bd > 1 else 0, 0, 1, max(1, bd // 2), bh // 2 + 1, bw // 2 + 1, pdc]
    return (0.8 * amp, 0.1 * amp, 1e30, damp, boost, grey, band)


CASES = [((1, 4, 4), 2, 1), ((8, 8, 8), 3, 2), ((1, 32, 32), 4, 1)]
CASE_IDS = [f"{'x'.join(map(str, b))}-C{c}" for b, c, _ in CASES]


@pytest.mark.parametrize("mode", ["abs", "shift", "flat", "copy"])
@pytest.mark.parametrize("block,comps,pdc", CASES, ids=CASE_IDS)
def test_packed_spec_store_equals_block_spec_store_on_every_component(core, block, comps, pdc, mode):
    """the tile starts as NaNs and holds the workgroup's coefficients only: a read outside them reaches the bytes (abs: through c as well)"""
    for filt in (None, full_filter(block, comps, pdc, False)):
        out, want, coded, want_coded = run_both(core, block, comps, False, mode, filt)
        assert np.array_equal(out, want), (filt is not None, int((out != want).sum()))
        assert coded == sum(want_coded) and (coded > 0) == (filt is not None)
        if filt:
            assert len(set(want_coded)) == comps, want_coded          # every component's filter is another one
    assert len(np.unique(want)) > 8          # (the encodes spread these coefficients over the bytes; flat on a 4 x 4 block over few)


@pytest.mark.parametrize("mode", ["shift", "flat", "copy"])
@pytest.mark.parametrize("block,comps,pdc", CASES, ids=CASE_IDS)
def test_packed_ispec_load_equals_block_ispec_load_on_every_component(core, block, comps, pdc, mode):
    """the tile's contents, bit for bit; what lies outside the workgroup's columns stays NaN"""
    for filt in (None, full_filter(block, comps, pdc, True)):
        out, want, coded, want_coded = run_both(core, block, comps, True, mode, filt)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (filt is not None, int((out.view(np.uint32) != want.view(np.uint32)).sum()))
        assert coded == sum(want_coded) and (coded > 0) == (filt is not None)


# ---- the emulation library ----
def test_the_emulation_library_answers_minus_3_and_writes_nothing():
    from emul_lib import emul
    L = emul()
    block = (8, 8, 8)
    shape = (16, 16, 8 * next_prime(planar_G(block)))
    fwd, inv, info = motion_grid_plans(shape, block, block, lib=L)
    k = motion_spec_constants(block)
    sp = spec_params("shift", k)
    p = plain_packed(3)
    n = int(np.prod(shape)) * 3
    u8 = ol.synth_u8(5, n)
    for plan, call, tail in ((fwd, L.dspfft_execute_spectrogram_u8_packed, ()), (inv, L.dspfft_execute_ispectrogram_u8_packed, (info["out_mul"],))):
        o8 = np.full(n, 9, dtype=np.uint8)
        rc = call(plan._h, u8.ctypes.data, o8.ctypes.data, None, C.byref(sp), None, C.byref(p), *tail, None, None)
        assert rc == -3 and b"not built into this library" in L.dspfft_last_error()
        assert np.all(o8 == 9)
    with pytest.raises(DspfftError, match="not built into this library"):
        fwd.spectrogram_packed(u8.ctypes.data, u8.ctypes.data, "shift", k["scalefactor"], k["normalization"], p, c=k["c"])
    # full frames
    F, h, w = 2, 10, 12
    ff, fi, finfo = motion_packed_frame_plans(F, h, w, 3, lib=L)
    n = F * h * w * 3
    u8 = ol.synth_u8(6, n)
    wk = np.full(n, 7.0, dtype=np.float32)
    sp = _lib.MotionSpecParams(MODES["shift"], finfo["scalefactor"], finfo["normalization"], finfo["c"])
    for plan, call, tail in ((ff, L.dspfft_execute_spectrogram_u8_packed, ()), (fi, L.dspfft_execute_ispectrogram_u8_packed, (finfo["out_mul"],))):
        o8 = np.full(n, 9, dtype=np.uint8)
        rc = call(plan._h, u8.ctypes.data, o8.ctypes.data, wk.ctypes.data, C.byref(sp), None, C.byref(p), *tail, None, None)
        assert rc == -3 and b"not built into this library" in L.dspfft_last_error()
        assert np.all(o8 == 9) and np.all(wk == 7.0)


# ---- the product library: every refusal, its code and a reason that names the cause, ahead of any launch ----
def bad_filter(block):
    fp = _lib.MotionFilterParams()
    fp.active = (C.c_int * 3)(*block); fp.minbuf_hw = (C.c_int * 2)(block[1], block[2]); fp.block_depth = block[0]
    fp.band_end = (C.c_int * 3)(*block)
    fp.damp = fp.boost = 1.0
    fp.preserve_dc = 5
    return fp


def test_refusals_of_the_product_library_come_before_any_launch():
    L = _lib.load()
    err = L.dspfft_last_error
    block = (8, 8, 8)
    shape = (16, 16, 8 * next_prime(planar_G(block)))
    fwd, inv, info = motion_grid_plans(shape, block, block, lib=L)
    k = motion_spec_constants(block)
    ff, fi, finfo = motion_packed_frame_plans(2, 12, 20, 3, lib=L)
    p3, p4 = plain_packed(3), plain_packed(4)
    spec = lambda plan, a, b, wk, sp, fp, pk: L.dspfft_execute_spectrogram_u8_packed(plan, a, b, wk, sp, fp, pk, None, None)
    ispec = lambda plan, a, b, wk, sp, fp, pk: L.dspfft_execute_ispectrogram_u8_packed(plan, a, b, wk, sp, fp, pk, info["out_mul"], None, None)
    shift, ab = spec_params("shift", k), spec_params("abs", k)
    R = C.byref
    for call, small, frames, other in ((spec, fwd, ff, inv), (ispec, inv, fi, fwd)):
        # -1: a NULL plan, buffer, sp or packed
        assert call(None, FAKE, FAKE, None, R(shift), None, R(p3)) == -1 and b"null plan, buffer or parameters" in err()
        assert call(small._h, None, FAKE, None, R(shift), None, R(p3)) == -1 and b"null plan, buffer or parameters" in err()
        assert call(small._h, FAKE, None, None, R(shift), None, R(p3)) == -1 and b"null plan, buffer or parameters" in err()
        assert call(small._h, FAKE, FAKE, None, None, None, R(p3)) == -1 and b"null plan, buffer or parameters" in err()
        assert call(small._h, FAKE, FAKE, None, R(shift), None, None) == -1 and b"null dspfft_motion_packed" in err()
        # -1: a bad mode (none is the roundtrip's), bad filter parameters, the other side's transform kind, full frames without d_work
        for m in (0, 5, -1):
            bad = _lib.MotionSpecParams(m, 1.0, 1.0, 1.0)
            assert call(small._h, FAKE, FAKE, None, R(bad), None, R(p3)) == -1 and b"mode must be" in err()
        fp = bad_filter(block)
        assert call(small._h, FAKE, FAKE, None, R(shift), R(fp), R(p3)) == -1 and b"bad filter parameters" in err()
        assert call(other._h, FAKE, FAKE, None, R(shift), None, R(p3)) == -1 and b"the plan must be REDFT" in err()
        assert call(frames._h, FAKE, FAKE, None, R(shift), None, R(p3)) == -1 and b"float work buffer" in err()
        # -2: components outside 2..4
        for comps in (1, 5):
            pc = plain_packed(comps)
            assert call(small._h, FAKE, FAKE, None, R(shift), None, R(pc)) == -2 and b"components must be 2, 3 or 4" in err() and str(comps).encode() in err()
        # -2: an f64 plan
        f64 = Plan.many_r2r([8, 8, 8], [REDFT10 if call is spec else REDFT01] * 3, howmany=4, idist=512, odist=512, lib=L, dtype="f64")
        assert call(f64._h, FAKE, FAKE, None, R(shift), None, R(p3)) == -2 and b"f64 plans" in err()
        # (a plan with a transfer characteristic uploads its tables to a device: tests/test_motion_spec_packed_gpu.py)
        # -2, small blocks: buffers off by 2 bytes; 16 x 16 x 16 at four components: 64 KB of tiles, no room for the counter
        for a, b in ((4096 + 2, 4096), (4096, 4096 + 2)):
            assert call(small._h, C.c_void_p(a), C.c_void_p(b), None, R(shift), None, R(p3)) == -2 and b"4-byte aligned" in err()
        b16 = (16, 16, 16)
        pair16 = motion_grid_plans((32, 32, 16 * next_prime(planar_G(b16))), b16, b16, lib=L)
        assert call(pair16[0 if call is spec else 1]._h, FAKE, FAKE, None, R(shift), None, R(p4)) == -2 and b"64 KB of LDS" in err()
        # (more than 2^31 - 1 workgroups cannot be asked for: a plan over that many blocks has more lines than a plan can be made for)
        kind = REDFT10 if call is spec else REDFT01
        # -2, full frames: the unit-stride level counts 3, the call 4; a planar per-frame plan has none; a padded row pitch is not dense;
        # an out-of-place plan
        assert call(frames._h, FAKE, FAKE, FAKE, R(shift), None, R(p4)) == -2 and b"unit-stride batch level counts 3" in err()
        per_frame = Plan.many_r2r([12, 20], [kind] * 2, howmany=4, idist=240, odist=240, lib=L)
        assert call(per_frame._h, FAKE, FAKE, FAKE, R(shift), None, R(p3)) == -2 and b"unit-stride batch level counts 0" in err()
        padded = Plan.guru([(12, 66, 66), (20, 3, 3)], [(3, 1, 1), (2, 12 * 66, 12 * 66)], [kind] * 2, lib=L)
        assert call(padded._h, FAKE, FAKE, FAKE, R(shift), None, R(p3)) == -2 and b"dense in-place layout" in err()
        oop = Plan.guru([(12, 60, 60), (20, 3, 3)], [(3, 1, 1), (2, 720, 1440)], [kind] * 2, lib=L)
        assert call(oop._h, FAKE, FAKE, FAKE, R(shift), None, R(p3)) == -2 and b"dense in-place layout" in err()
        # -2: one 3-D block of interleaved pixels
        cube = Plan.guru([(6, 720, 720), (12, 60, 60), (20, 3, 3)], [(3, 1, 1)], [kind] * 3, lib=L)
        assert call(cube._h, FAKE, FAKE, FAKE, R(shift), None, R(p3)) == -2 and b"one 3-D block" in err()
    # -2: abs on the inverse side, small blocks and full frames
    assert ispec(inv._h, FAKE, FAKE, None, R(ab), None, R(p3)) == -2 and b"no abs type" in err()
    assert ispec(fi._h, FAKE, FAKE, FAKE, R(ab), None, R(p3)) == -2 and b"no abs type" in err()


# ---- engine.motion_packed_frame_plans ----
@pytest.mark.parametrize("frames,h,w,comps", [(3, 24, 40, 3), (1, 10, 18, 4), (2, 16, 256, 3)])
def test_motion_packed_frame_plans_layout_scales_and_info(frames, h, w, comps):
    """on the emulation library (the planner is the product's): the passes and scales from describe(), and the transform itself -- an
    impulse response against the reference's 2-D formulas with the unit z axis folded in"""
    from emul_lib import emul
    L = emul()
    fwd, inv, info = motion_packed_frame_plans(frames, h, w, comps, lib=L)
    k = motion_spec_constants((1, h, w))
    assert info == dict(scalefactor=1.0, normalization=k["normalization"], c=k["c"], ic=k["ic"], out_mul=k["normalization"] ** 2)
    assert info["normalization"] == 1.0 / math.sqrt(h * w * 8.0)
    assert fwd.num_passes == 2 and inv.num_passes == 2
    df, di = fwd.describe().splitlines(), inv.describe().splitlines()
    # fwd: the row pass (axis 1) begins it; inv: the row pass ends it
    assert [l for l in df if l.startswith("axis")][0].startswith("axis 1") and [l for l in di if l.startswith("axis")][-1].startswith("axis 1"), (df, di)
    # the layout and the scales: coefficients of a clip against the definition, and the inverse brings the clip back times 1 / out_mul
    n = frames * h * w * comps
    x = ol.synth_f32(0xF00 + w, n).reshape(frames, h, w, comps)
    buf = x.copy()
    fwd.execute(buf.ctypes.data)
    r2 = math.sqrt(2.0)

    def dct2(v, N, axis):
        i = np.arange(N)
        m = 2 * np.cos(np.pi * np.outer(i, 2 * i + 1) / (2 * N))
        m[0] /= r2
        return np.moveaxis(np.tensordot(m, np.moveaxis(v, axis, 0), axes=1), 0, axis)
    # motion.c:644-647: REDFT10 over (1, h, w) times 2 sqrt 2 with index 0 of every axis over sqrt 2; the unit axis doubles and divides by sqrt 2
    ref = dct2(dct2(x.astype(np.float64), h, 1), w, 2) * (2 * r2) * (2 / r2)
    assert np.abs(buf - ref).max() <= 2e-5 * np.abs(ref).max()
    inv.execute(buf.ctypes.data)
    assert np.abs(buf * info["out_mul"] - x).max() <= 1e-5


# ---- the float64 reference cases of tests/test_motion_spec_packed_gpu.py: what a comparison may leave out as ties stays within the cap ----
def test_the_reference_cases_of_the_gpu_test_stay_within_the_tie_share():
    import motion_spec_ref as sr
    import test_motion_spec_packed_gpu as tp
    for inverse, modes in ((False, tp.SPEC_MODES), (True, tp.ISPEC_MODES)):
        for mode in modes:
            for kind in (None, "band", "full", "q"):
                clip, refs = tp.ref_case(inverse, mode, kind)
                assert clip.shape == (tp.REF_FRAMES,) + tp.REF_BLOCK[1:] + (3,) and clip.dtype == np.uint8
                for ref in refs:
                    sr.check_tie_share(ref, inverse)
                    assert (kind in ("full", "q")) == (ref["coded"] > 0)
