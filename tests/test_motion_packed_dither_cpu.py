"""motion -d on packed 8-bit pixels (dspfft_execute_roundtrip_u8_packed_dither, _packed_frames_dither, dspfft_motion_dither_u8_packed), the parts
that need no device: the emulation library's -3, the product library's refusals ahead of any launch, and the new phases
(dspfun_amd/csrc/block_packed_core.h, dither_core.h) compiled with g++ and walked thread by thread over a NaN-filled tile.  No tolerance: the
packed bytes equal the planar phases on each de-interleaved component with the floats they store dithered plane by plane (dither_plane_serial)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from dspfun_amd import _lib
from dspfun_amd.engine import Plan, DspfftError, motion_grid_plans, motion_packed_frame_plans, motion_dither_u8_packed
from test_motion_packed_cpu import CPP as PACKED_CPP, FAKE, NBLOCKS_OF, plain_packed, volume_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRGB = 13          # AVCOL_TRC_IEC61966_2_1


def geom_of(n, nblocks=(1, 1, 1), block_step=(0, 0, 0), row_pitch=None):
    g = _lib.DitherGeom()
    g.n[:] = n
    g.row_pitch = n[2] if row_pitch is None else row_pitch
    g.plane_pitch = n[1] * g.row_pitch
    g.nblocks[:] = nblocks
    g.block_step[:] = block_step
    return g


# ---- the emulation library ----
def test_the_emulation_library_answers_minus_3_on_all_three_entries_and_writes_nothing():
    from emul_lib import emul
    L = emul()
    p = plain_packed(3)
    block = (8, 8, 8)
    shape = volume_of(block)
    fwd, inv, info = motion_grid_plans(shape, block, block, lib=L)
    n = int(np.prod(shape)) * 3
    u8 = ol.synth_u8(5, n)
    o8 = np.full(n, 9, dtype=np.uint8)
    rc = L.dspfft_execute_roundtrip_u8_packed_dither(fwd._h, inv._h, u8.ctypes.data, o8.ctypes.data, info["scalefactor"], info["normalization"], None, C.byref(p), None, None, None)
    assert rc == -3 and b"not built into this library" in L.dspfft_last_error() and b"dithered" in L.dspfft_last_error()
    with pytest.raises(DspfftError, match="not built into this library"):
        fwd.roundtrip_u8_packed_dither(inv, u8.ctypes.data, o8.ctypes.data, info["scalefactor"], info["normalization"], p)
    assert np.all(o8 == 9)
    # full frames
    F, h, w = 2, 16, 12
    ff, fi, finfo = motion_packed_frame_plans(F, h, w, 3, lib=L)
    m = F * h * w * 3
    work = np.full(m, 7.0, dtype=np.float32)
    o8 = np.full(m, 9, dtype=np.uint8)
    with pytest.raises(DspfftError, match="not built into this library"):
        ff.roundtrip_u8_packed_frames_dither(fi, u8.ctypes.data, o8.ctypes.data, work.ctypes.data, finfo["scalefactor"], finfo["normalization"], p)
    assert np.all(o8 == 9) and np.all(work == 7.0)
    # the stand-alone kernel
    g = geom_of((1, h, w), (F, 1, 1), (h * w, 0, 0))
    assert L.dspfft_motion_dither_u8_packed(o8.ctypes.data, work.ctypes.data, C.byref(g), 3, 1.0, 1.0, 0, None) == -3 and b"not built into this library" in L.dspfft_last_error()
    with pytest.raises(DspfftError, match="not built into this library"):
        motion_dither_u8_packed(o8.ctypes.data, work.ctypes.data, (1, h, w), 3, nblocks=(F, 1, 1), block_step=(h * w, 0, 0), lib=L)
    assert np.all(o8 == 9)


# ---- the product library: every refusal, its code and a reason that names the cause, ahead of any launch ----
def test_small_block_refusals_of_the_product_library_come_before_any_launch():
    L = _lib.load()
    err = L.dspfft_last_error
    call = L.dspfft_execute_roundtrip_u8_packed_dither
    block = (8, 8, 8)
    shape = volume_of(block)
    fwd, inv, info = motion_grid_plans(shape, block, block, lib=L)
    sf, nm = info["scalefactor"], info["normalization"]
    p3 = plain_packed(3)
    name = b"dithered roundtrip on packed 8-bit pixels"
    # the packed entry's own refusals, under this entry's name
    for comps in (1, 5):
        pc = plain_packed(comps)
        assert call(fwd._h, inv._h, FAKE, FAKE, sf, nm, None, C.byref(pc), None, None, None) == -2 and b"components must be 2, 3 or 4" in err() and name in err()
    f2 = Plan.many_r2r([12, 20], [5, 5], howmany=4, idist=240, odist=240, lib=L)
    i2 = Plan.many_r2r([12, 20], [4, 4], howmany=4, idist=240, odist=240, lib=L, first_axis_first=True)
    assert call(f2._h, i2._h, FAKE, FAKE, sf, nm, None, C.byref(p3), None, None, None) == -2 and b"fused block pass" in err() and name in err()
    for a, b in ((4096 + 2, 4096), (4096, 4096 + 2)):
        assert call(fwd._h, inv._h, C.c_void_p(a), C.c_void_p(b), sf, nm, None, C.byref(p3), None, None, None) == -2 and b"4-byte aligned" in err() and name in err()
    assert call(fwd._h, inv._h, FAKE, FAKE, sf, nm, None, None, None, None, None) == -1 and b"null dspfft_motion_packed" in err() and name in err()
    assert call(fwd._h, inv._h, None, FAKE, sf, nm, None, C.byref(p3), None, None, None) == -1 and b"null plan or buffer" in err()
    assert call(None, inv._h, FAKE, FAKE, sf, nm, None, C.byref(p3), None, None, None) == -1 and b"null plan or buffer" in err()
    f64 = Plan.many_r2r([8, 8, 8], [5] * 3, howmany=4, idist=512, odist=512, lib=L, dtype="f64")
    assert call(f64._h, inv._h, FAKE, FAKE, sf, nm, None, C.byref(p3), None, None, None) == -1 and b"f32 plans" in err()
    cl = _lib.CoeffLimit()
    cl.keep, cl.outside_mul = 0, 1.0
    assert call(fwd._h, inv._h, FAKE, FAKE, sf, nm, None, C.byref(p3), C.byref(cl), None, None) == -1 and b"keep must be at least 1" in err()
    # the two factors
    for s, n in ((0.0, nm), (-1.0, nm), (float("inf"), nm), (float("nan"), nm), (sf, 0.0), (sf, float("inf")), (sf, float("nan"))):
        assert call(fwd._h, inv._h, FAKE, FAKE, s, n, None, C.byref(p3), None, None, None) == -1 and b"scalefactor and normalization must be finite and > 0" in err()
    # a rescaled grid pair
    fg, ig, ginfo = motion_grid_plans(shape, block, (4, 4, 4), lib=L)
    assert call(fg._h, ig._h, FAKE, FAKE, ginfo["scalefactor"], ginfo["normalization"], None, C.byref(p3), None, None, None) == -2
    assert b"-d on a packed rescaled grid is not implemented" in err()
    # 16 x 16 x 16 at four components: 64 KB of tiles, no room for anything behind them
    b16 = (16, 16, 16)
    f16, i16, info16 = motion_grid_plans(volume_of(b16), b16, b16, lib=L)
    p4 = plain_packed(4)
    assert call(f16._h, i16._h, FAKE, FAKE, info16["scalefactor"], info16["normalization"], None, C.byref(p4), None, None, None) == -2 and b"64 KB of LDS" in err()


def test_frames_and_stand_alone_refusals_of_the_product_library_come_before_any_launch():
    L = _lib.load()
    err = L.dspfft_last_error
    call = L.dspfft_execute_roundtrip_u8_packed_frames_dither
    F, h, w = 2, 16, 12
    fwd, inv, info = motion_packed_frame_plans(F, h, w, 3, lib=L)
    sf, nm = info["scalefactor"], info["normalization"]
    p3 = plain_packed(3)
    name = b"dithered roundtrip on packed 8-bit pixels over full frames"
    assert call(fwd._h, inv._h, FAKE, FAKE, None, sf, nm, None, C.byref(p3), None, None) == -1 and b"null float work buffer" in err() and name in err()
    assert call(fwd._h, inv._h, FAKE, None, FAKE, sf, nm, None, C.byref(p3), None, None) == -1 and b"null plan or buffer" in err()
    assert call(fwd._h, inv._h, FAKE, FAKE, FAKE, sf, nm, None, None, None, None) == -1 and b"null dspfft_motion_packed" in err()
    for s, n in ((0.0, nm), (sf, -1.0), (float("nan"), nm), (sf, float("inf"))):
        assert call(fwd._h, inv._h, FAKE, FAKE, FAKE, s, n, None, C.byref(p3), None, None) == -1 and b"scalefactor and normalization must be finite and > 0" in err()
    p4 = plain_packed(4)
    assert call(fwd._h, inv._h, FAKE, FAKE, FAKE, sf, nm, None, C.byref(p4), None, None) == -2 and b"not the 4 components" in err() and name in err()
    bf, bi, binfo = motion_grid_plans(volume_of((8, 8, 8)), (8, 8, 8), (8, 8, 8), lib=L)
    assert call(bf._h, bi._h, FAKE, FAKE, FAKE, sf, nm, None, C.byref(p3), None, None) == -2 and b"dspfft_execute_roundtrip_u8_packed" in err()
    # (a width above the wavefront kernel's rings needs a plan whose tables live on the device: test_motion_packed_dither_gpu.py)
    # the stand-alone kernel
    dz = L.dspfft_motion_dither_u8_packed
    g = geom_of((1, h, w), (F, 1, 1), (h * w, 0, 0))
    for comps in (1, 5, 0, -3):
        assert dz(FAKE, FAKE, C.byref(g), comps, 1.0, 1.0, 0, None) == -1 and b"components must be 2, 3 or 4" in err()
    assert dz(None, FAKE, C.byref(g), 3, 1.0, 1.0, 0, None) == -1 and b"null pointer" in err()
    assert dz(FAKE, FAKE, None, 3, 1.0, 1.0, 0, None) == -1 and b"null pointer" in err()
    assert dz(FAKE, FAKE, C.byref(g), 3, 0.0, 1.0, 0, None) == -1 and b"finite and > 0" in err()
    assert dz(FAKE, FAKE, C.byref(g), 3, 1.0, 1.0, 99, None) == -1 and b"not built" in err()
    bad = geom_of((1, h, w), (F, 1, 1), (h * w, 0, 0), row_pitch=w - 1)
    assert dz(FAKE, FAKE, C.byref(bad), 3, 1.0, 1.0, 0, None) == -1 and b"row pitch below the row length" in err()
    wide = geom_of((1, 70, 9600))
    assert dz(FAKE, FAKE, C.byref(wide), 2, 1.0, 1.0, 0, None) == -1 and b"plane too wide" in err()


# ---- the phases on the CPU: test_motion_packed_cpu.py's shim (geometry, scales, filter, the planar and packed sequences) with the dithered ends ----
CPP = PACKED_CPP + r'''
#include "dither_core.h"
// the planar sequence ending in FLOATS (what the planar dithered call leaves in its work buffer) ...
template <int NX, int NY, int NZ>
static void seq_planar_f32(const BlockRtArgs &a, int nwg, unsigned long long &mine)
{
	std::vector<float> raw;
	for (int wg = 0; wg < nwg; wg++) {
		long long bin, bout; int cnt;
		block_base(a, (uint32_t)wg, bin, bout, cnt);
		float *lds = nan_tile(raw, (size_t)NZ * NY * a.pitch);
		EACH_TID block_load_x<NX, NY, NZ, KIND_REDFT10, true>(a, block_axis_args(a.f, 0, NY == 1 && NZ == 1), nullptr, a.in8, lds, bin, cnt, tid);
		if constexpr (NZ > 1) {
			if constexpr (NY > 1) EACH_TID block_lines_y<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.f, 1, false), lds, cnt, tid);
			EACH_TID block_lines_mid<NX, NY, NZ, true>(a, block_axis_args(a.f, 2, true), block_axis_args(a.i, 2, false), a.filt, lds, cnt, tid, mine);
			if constexpr (NY > 1) EACH_TID block_lines_y<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.i, 1, false), lds, cnt, tid);
		} else EACH_TID block_lines_mid<NX, NY, NZ, false>(a, block_axis_args(a.f, 1, true), block_axis_args(a.i, 1, false), a.filt, lds, cnt, tid, mine);
		EACH_TID block_store_x<NX, NY, NZ, KIND_REDFT01, false>(a, block_axis_args(a.i, 0, true), a.out, nullptr, 1.0, lds, bout, cnt, tid);
	}
}
// ... and the packed sequence ending in the three phases of -d; the dither's LDS (error table, error rows) starts as NaNs too
template <int NX, int NY, int NZ, int C>
static void seq_packed_dither(const BlockPackedDitherArgs &a, int nwg, const double *thr, const TrcParams &tp, unsigned long long &mine)
{
	std::vector<float> raw;
	std::vector<double> dl;
	for (int wg = 0; wg < nwg; wg++) {
		long long bin, bout; int cnt;
		block_base(a, (uint32_t)wg, bin, bout, cnt);
		float *lds = nan_tile(raw, (size_t)NZ * NY * a.pitch);
		dl.assign(256 + (size_t)a.slots * NX, NAN);
		dither_table(dl.data(), a.sf, a.norm);
		const int nb = cnt * C;
		EACH_TID packed_load_x<NX, NY, NZ, C>(a, block_axis_args(a.f, 0, NY == 1 && NZ == 1), a.in8, lds, bin, cnt, tid, nullptr);
		if constexpr (NZ > 1) {
			if constexpr (NY > 1) EACH_TID block_lines_y<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.f, 1, false), lds, nb, tid);
			EACH_TID packed_lines_mid<NX, NY, NZ, C, true>(a, block_axis_args(a.f, 2, true), block_axis_args(a.i, 2, false), lds, cnt, tid, mine);
			if constexpr (NY > 1) EACH_TID block_lines_y<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.i, 1, false), lds, nb, tid);
		} else EACH_TID packed_lines_mid<NX, NY, NZ, C, false>(a, block_axis_args(a.f, 1, true), block_axis_args(a.i, 1, false), lds, cnt, tid, mine);
		EACH_TID packed_inverse_x<NX, NY, NZ, C>(a, block_axis_args(a.i, 0, true), lds, cnt, tid);
		EACH_TID packed_dither_tile<NX, NY, NZ, C>(a, lds, cnt, tid, dl.data(), dl.data() + 256, thr, tp);
		EACH_TID packed_store_bytes<NX, NY, NZ, C>(a, a.out8, lds, bout, cnt, tid);
	}
}
// one plane: the planar phases into `work` (the plane's layout), then dither_plane_serial over every z plane of every block.  trc: 0, or the id
extern "C" int run_planar_dither(const uint8_t *in8, uint8_t *out8, float *work, const int *nblocks, const int *block, int G, const float *fl, const int *bp,
                                 double sf, double norm, int trc, unsigned long long *coded)
{
	BlockRtArgs a;
	memset((void *)&a, 0, sizeof a);
	const int nwg = geom(a, nblocks, block, 0, G, 1);
	scales(a, block[0]);
	a.in8 = in8; a.out = work;
	if (fl) filter(a.filt, block, fl, bp, fl[3], fl[4], fl[5]);
	unsigned long long mine = 0;
	bool ran = false;
#define CASE(X_, Y_, Z_) if (a.nx == X_ && a.ny == Y_ && a.nz == Z_) { seq_planar_f32<X_, Y_, Z_>(a, nwg, mine); ran = true; }
	SHAPES(CASE)
#undef CASE
	if (!ran) return -1;
	*coded += mine;
	double tab[256], thr[256];
	dither_table(tab, sf, norm);
	TrcParams tp = TrcParams();
	if (trc) { if (!trc_built(trc)) return -2; trc_u8_thresholds(thr, trc); tp = trc_params(trc); }
	const int bd = block[0], bh = block[1], bw = block[2];
	const long long H = (long long)nblocks[1] * bh, W = (long long)nblocks[2] * bw;
	std::vector<double> dprow(bw);
	for (int z = 0; z < nblocks[0] * bd; z++)
		for (int by = 0; by < nblocks[1]; by++)
			for (int bx = 0; bx < nblocks[2]; bx++) {
				const long long base = ((long long)z * H + (long long)by * bh) * W + (long long)bx * bw;
				dprow.assign(bw, NAN);
				if (trc) dither_plane_serial<true>(out8 + base, work + base, W, bh, bw, sf, norm, tab, dprow.data(), 1, thr, &tp);
				else dither_plane_serial(out8 + base, work + base, W, bh, bw, sf, norm, tab, dprow.data(), 1);
			}
	return nwg;
}
extern "C" int run_packed_dither(const uint8_t *in8, uint8_t *out8, const int *nblocks, const int *block, int comps, int G, const float *fl, const int *bp,
                                 double sf, double norm, int trc, unsigned long long *coded)
{
	BlockPackedDitherArgs a;
	memset((void *)&a, 0, sizeof a);
	const int nwg = geom(a, nblocks, block, 0, G, comps);
	scales(a, block[0]);
	a.in8 = in8; a.out8 = out8; a.mul8 = NAN; a.comps = comps; a.sf = sf; a.norm = norm; a.slots = packed_dither_slots(a.nz, comps, G);
	if (fl) {
		filter(a.filt, block, fl, bp, NAN, NAN, NAN);
		for (int c = 0; c < 4; c++) { a.damp[c] = fl[3 + c]; a.boost[c] = fl[7 + c]; a.grey_add[c] = fl[11 + c]; }
	}
	double thr[256];
	TrcParams tp = TrcParams();
	if (trc) { if (!trc_built(trc)) return -2; trc_u8_thresholds(thr, trc); tp = trc_params(trc); }
	unsigned long long mine = 0;
#define CASE(X_, Y_, Z_) if (a.nx == X_ && a.ny == Y_ && a.nz == Z_) { \
		if (comps == 2) seq_packed_dither<X_, Y_, Z_, 2>(a, nwg, trc ? thr : nullptr, tp, mine); else if (comps == 3) seq_packed_dither<X_, Y_, Z_, 3>(a, nwg, trc ? thr : nullptr, tp, mine); \
		else seq_packed_dither<X_, Y_, Z_, 4>(a, nwg, trc ? thr : nullptr, tp, mine); \
		*coded += mine; return nwg; }
	SHAPES(CASE)
#undef CASE
	return -1;
}
// a component's plane walked with the pixel step inside the interleaved buffers, and the de-interleaved plane walked with step 1
extern "C" void walk_step(uint8_t *out, const float *in, long long pitch, int step, int h, int w, double sf, double norm, int trc)
{
	double tab[256], thr[256];
	dither_table(tab, sf, norm);
	std::vector<double> dprow(w, NAN);
	if (trc) { trc_u8_thresholds(thr, trc); const TrcParams tp = trc_params(trc); dither_plane_step<true>(out, in, pitch, step, h, w, sf, norm, tab, dprow.data(), 1, thr, &tp); }
	else dither_plane_step(out, in, pitch, step, h, w, sf, norm, tab, dprow.data(), 1);
}
extern "C" void walk_serial(uint8_t *out, const float *in, long long pitch, int h, int w, double sf, double norm, int trc)
{
	double tab[256], thr[256];
	dither_table(tab, sf, norm);
	std::vector<double> dprow(w, NAN);
	if (trc) { trc_u8_thresholds(thr, trc); const TrcParams tp = trc_params(trc); dither_plane_serial<true>(out, in, pitch, h, w, sf, norm, tab, dprow.data(), 1, thr, &tp); }
	else dither_plane_serial(out, in, pitch, h, w, sf, norm, tab, dprow.data(), 1);
}
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("block_packed_dither_core")
    src, so = d / "core.cpp", d / "core.so"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "dspfun_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.group_of.argtypes = [C.c_int] * 5
    lib.run_planar_dither.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p]
    lib.run_packed_dither.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p]
    lib.walk_step.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
    lib.walk_step.restype = None
    lib.walk_serial.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
    lib.walk_serial.restype = None
    return lib


def run_both(core, block, comps, trc=0, G=None):
    """the packed dithered sequence on an interleaved clip (a quantiser and a band with per-component damp and boost, so that the floats lie
    between the bytes), and the planar sequence + dither_plane_serial on each of its planes with that component's values"""
    bd, bh, bw = block
    nb = NBLOCKS_OF(block)
    shape = (nb[0] * bd, nb[1] * bh, nb[2] * bw)
    clip = ol.synth_u8(0xD1 + comps + 16 * bd + bw, int(np.prod(shape)) * comps).reshape(shape + (comps,))
    ia = lambda v: (C.c_int * len(v))(*v)
    sf, norm = 1.0, 1.0 / np.sqrt(8.0 * bd * bh * bw)
    Gp = G or core.group_of(bw, bh, bd, comps, nb[2])
    assert 1 <= Gp <= nb[2]
    damp, boost, grey = [0.25, 0.5, 0.0, 0.75][:comps], [2.0, 1.0, 0.5, 1.5][:comps], [900.0, -300.0, 0.0, 150.0][:comps]
    band = ia([1 if bd > 1 else 0, 0, 1, max(1, bd // 2), bh // 2 + 1, bw // 2 + 1, 2])
    pad = lambda v: list(v) + [0.0] * (4 - len(v))
    fl = (C.c_float * 15)(24.0, 3.0, 1e9, *pad(damp), *pad(boost), *pad(grey))
    out = np.full(clip.shape, 0xEE, dtype=np.uint8)
    coded = np.zeros(1, dtype=np.uint64)
    nwg = core.run_packed_dither(clip.ctypes.data, out.ctypes.data, ia(nb), ia(block), comps, Gp, fl, band, sf, norm, trc, coded.ctypes.data)
    assert nwg == -(-nb[2] // Gp) * nb[0] * nb[1]
    want = np.empty_like(clip)
    want_coded = 0
    from test_motion_packed_cpu import planar_G
    for c in range(comps):
        plane = np.ascontiguousarray(clip[..., c])
        o = np.full(plane.shape, 0xEE, dtype=np.uint8)
        work = np.full(plane.shape, np.nan, dtype=np.float32)
        n = np.zeros(1, dtype=np.uint64)
        flc = (C.c_float * 6)(fl[0], fl[1], fl[2], fl[3 + c], fl[7 + c], fl[11 + c])
        assert core.run_planar_dither(plane.ctypes.data, o.ctypes.data, work.ctypes.data, ia(nb), ia(block), min(planar_G(block), nb[2]), flc, band, sf, norm, trc, n.ctypes.data) > 0
        assert np.isfinite(work).all()
        # (vacuity: the dithered bytes are not the plainly rounded ones)
        assert (o != np.clip(np.round(work.astype(np.float64) * sf * norm * norm), 0, 255)).any() or trc
        want[..., c] = o
        want_coded += int(n[0])
    return out, want, int(coded[0]), want_coded, Gp, nb[2]


BLOCKS = [(1, 4, 4), (8, 8, 8), (8, 16, 4)]


@pytest.mark.parametrize("comps", [2, 3, 4])
@pytest.mark.parametrize("block", BLOCKS, ids=["x".join(map(str, b)) for b in BLOCKS])
def test_dithered_packed_phases_equal_the_planar_phases_and_the_serial_dither_on_every_component(core, block, comps):
    out, want, coded, want_coded, Gp, nxb = run_both(core, block, comps)
    assert np.array_equal(out, want), int((out != want).sum())
    assert coded == want_coded > 0
    if Gp > 1:          # another grouping, the same bytes; one of the two has a short last group (the row holds a prime number of blocks)
        assert nxb % Gp or nxb % (Gp - 1)
        assert np.array_equal(run_both(core, block, comps, G=Gp - 1)[0], want)


@pytest.mark.parametrize("block,comps", [((8, 8, 8), 3), ((1, 4, 4), 4), ((8, 16, 4), 2)])
def test_dithered_packed_phases_with_a_transfer_characteristic_equal_the_trc_variant(core, block, comps):
    out, want, _, _, _, _ = run_both(core, block, comps, trc=SRGB)
    assert np.array_equal(out, want), int((out != want).sum())
    assert not np.array_equal(out, run_both(core, block, comps)[0])


@pytest.mark.parametrize("trc", [0, SRGB])
@pytest.mark.parametrize("h,w,comps,pad", [(9, 20, 3, 0), (5, 7, 4, 3), (1, 9, 2, 0), (9, 1, 2, 0)])
def test_the_pixel_step_walk_equals_the_step_1_walk_of_the_de_interleaved_plane(core, h, w, comps, pad, trc):
    rng = np.random.default_rng(h * 100 + w)
    pitch = w + pad
    co = (rng.random((h, pitch, comps)) * 295 - 20).astype(np.float32)
    co[h // 2, : w // 2] = np.round(co[h // 2, : w // 2]) + 0.5          # a plateau of exact halves
    out = np.full((h, pitch, comps), 0xEE, dtype=np.uint8)
    for c in range(comps):
        core.walk_step(out.ctypes.data + c, co.ctypes.data + 4 * c, pitch * comps, comps, h, w, 1.0, 1.0, trc)
    for c in range(comps):
        plane = np.ascontiguousarray(co[..., c])
        o = np.full((h, pitch), 0xEE, dtype=np.uint8)
        core.walk_serial(o.ctypes.data, plane.ctypes.data, pitch, h, w, 1.0, 1.0, trc)
        assert np.array_equal(out[..., c], o)
        assert np.all(out[:, w:, c] == 0xEE)
