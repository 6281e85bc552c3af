"""motion --coeff-limit on a rescaled block grid (block_rescale_topn.hip), the parts that need no device: the new phases of
dspfun_amd/csrc/block_rs_core.h compiled with g++ and run thread by thread, with a serial selection that states topn_core.h's rule in place
of its ballot rounds, against the f64 restatement of the reference block by block (tests/motion_grid_topn_ref.py: blocks on which the
reference's ranking differs from "scale everything, then rank"); and the refusals of the dspfft_execute_roundtrip*_limit entries, which come
before any launch, beside the unchanged refusal of the _topn entries on a grid pair."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_grid_ref as gr
import motion_grid_topn_ref as tr
import motion_ref as mr
from dspfun_amd.engine import Plan, motion_grid_plans

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned address for calls that are refused before anything reads it

# ---- the kernel's sequence of phases on the CPU: a test-only shim that lays out the geometry the engine derives (volume layout) and walks
# tid 0..255 through every phase; between the forward passes and the filter a serial selection per block ----
CPP = r'''
#include <stdint.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "block_rs_core.h"
#include "topn_core.h"
using namespace dspfft;
// topn_core.h's rule on block g of the tile: key = the bit pattern of |value|, the `keep` largest stay, ties to the smaller e = (z MY + y) MX + x
static void select_block(float *lds, const RsTile &t, int g, unsigned keep, bool restore)
{
	const int mx = t.tw, E = rs_topn_elems(t);
	auto at = [&](int e) -> float & { return lds[(e / mx) * t.pitch + g * t.tw + e % mx]; };
	const float dc = at(0);
	std::vector<int> order(E);
	std::vector<uint32_t> key(E);
	for (int e = 0; e < E; e++) { order[e] = e; const float v = at(e); uint32_t b; memcpy(&b, &v, 4); key[e] = b & 0x7fffffffu; }
	std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return key[p] > key[q]; });
	for (int r = (int)keep; r < E; r++) at(order[r]) = 0.f;
	if (restore) at(0) = dc;
}
// in / out: float or 8-bit (the other NULL); volume layout [D][H][W] -> [D'][H'][W']
extern "C" int run(const float *in, const uint8_t *in8, float *out, uint8_t *out8, const int *nblocks, const int *block, const int *scaled,
                   int G, unsigned keep, float boost, double mul8)
{
	const int nd = nblocks[0], nh = nblocks[1], nw = nblocks[2];
	const int bd = block[0], bh = block[1], bw = block[2], sd = scaled[0], sh = scaled[1], sw = scaled[2];
	const long long H = (long long)nh * bh, W = (long long)nw * bw, Ho = (long long)nh * sh, Wo = (long long)nw * sw;
	BlockRsTopnArgs a;
	memset((void *)&a, 0, sizeof a);
	a.nx = bw; a.ny = bh; a.nz = bd; a.ox = sw; a.oy = sh; a.oz = sd;
	a.tw = rs_max(bw, sw); a.G = G; a.pitch = G * a.tw;
	a.rows_fast = 0; a.nxb = nw; a.nd = 2;
	a.sy_in = W; a.sz_in = H * W; a.sxb_in = bw;
	a.sy_out = Wo; a.sz_out = Ho * Wo; a.sxb_out = sw;
	a.bn[0] = nh; a.bis[0] = bh * W; a.bos[0] = sh * Wo;
	a.bn[1] = nd; a.bis[1] = bd * H * W; a.bos[1] = sd * Ho * Wo;
	for (int d = 0; d < 2; d++) a.bdiv[d] = motion_filter_div((uint32_t)a.bn[d]);
	a.ngroups = (a.nxb + G - 1) / G; a.gdiv = motion_filter_div((uint32_t)a.ngroups);
	int nwg = a.ngroups;
	for (int d = 0; d < a.nd; d++) nwg *= a.bn[d];
	a.in = in; a.in8 = in8; a.out = out; a.out8 = out8; a.mul8 = mul8;
	// motion's scales as engine.motion_grid_plans sets them (motion.c:644-647,748-751; the unit axis of 2-D blocks folded in) ...
	const float r2 = sqrtf(2.f), unit = bd == 1 ? r2 : 1.f;
	a.f.scale = 2 * r2 * unit; a.i.scale = unit / (2 * r2);
	for (int k = 0; k < 3; k++) { const bool on = k < 2 || bd > 1; a.f.in0[k] = 1.f; a.f.out0[k] = on ? 1.f / r2 : 1.f; a.i.in0[k] = on ? r2 : 1.f; a.i.out0[k] = 1.f; }
	// ... and the keys' factors as engine.cpp's rt_run_grid derives them, with info["limit_outside_mul"]
	a.keep = keep;
	a.key_mul = (float)((bd == 1 ? 2.0 : 1.0) / (double)a.f.scale);
	for (int k = 0; k < 3; k++) a.key_mul0[k] = 1.f / a.f.out0[k];
	if (boost != 1.f) {
		MotionFilter &f = a.filt;
		f.ad = bd < sd ? bd : sd; f.ah = bh < sh ? bh : sh; f.aw = bw < sw ? bw : sw; f.mh = f.mw = 1;
		f.b1d = f.ad; f.b1h = f.ah; f.b1w = f.aw;
		f.damp = 1.f; f.boost = boost; f.preserve_dc = 1; f.enabled = 1;
		motion_filter_set_divs(f, 1);
	}
	const RsTile t = rs_tile_of(a), all = rs_tile_unpruned(t);
	const RsKeys keys = rs_keys_of(a);
	std::vector<float> raw(rs_tile_bytes(t) / sizeof(float) + 8, NAN);        // what no phase writes must never be read
	float *lds = (float *)(((uintptr_t)raw.data() + 15) & ~(uintptr_t)15);
	unsigned long long mine = 0;
	for (int wg = 0; wg < nwg; wg++) {
		long long bin, bout; int cnt;
		block_base(a, (uint32_t)wg, bin, bout, cnt);
		for (size_t i = 0; i < rs_tile_bytes(t) / sizeof(float); i++) lds[i] = NAN;
		for (int tid = 0; tid < BLOCK_THREADS; tid++) { rs_phase_load(all, lds, bin, cnt, tid, nullptr); rs_phase_zero_outside(t, lds, cnt, tid); }
		for (int tid = 0; tid < BLOCK_THREADS; tid++) rs_phase_fwd_y(all, lds, cnt, tid);
		for (int tid = 0; tid < BLOCK_THREADS; tid++) rs_phase_fwd_last_keys(t, keys, lds, cnt, tid);
		for (int g = 0; g < cnt; g++) {
			for (int e = 0; e < rs_topn_elems(t); e++) if (isnan(lds[(e / t.tw) * t.pitch + g * t.tw + e % t.tw])) return -1;   // the selection reads the whole embedding
			select_block(lds, t, g, keep, motion_filter_restores_dc(t.filt));
		}
		for (int tid = 0; tid < BLOCK_THREADS; tid++) rs_phase_filt_inv_last(t, lds, cnt, tid, mine);
		for (int tid = 0; tid < BLOCK_THREADS; tid++) rs_phase_inv_y(t, lds, cnt, tid);
		for (int tid = 0; tid < BLOCK_THREADS; tid++) rs_phase_store(t, lds, bout, cnt, tid, nullptr, 0);
	}
	return nwg;
}
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("block_rs_topn_core")
    src, so = d / "core.cpp", d / "core.so"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "dspfun_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.run.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_uint, C.c_float, C.c_double]
    return lib


def run_core(core, vol, block, scaled, G, keep, u8=True, boost=1.0):
    _, out_shape = gr.shapes(block, scaled, tr.NBLOCKS)
    ia = lambda v: (C.c_int * 3)(*v)
    src = np.ascontiguousarray(vol if u8 else vol.astype(np.float32))
    out = np.zeros(out_shape, dtype=np.uint8 if u8 else np.float32)
    sf, nm = mr.consts(block, scaled)
    nwg = core.run(None if u8 else src.ctypes.data, src.ctypes.data if u8 else None, None if u8 else out.ctypes.data, out.ctypes.data if u8 else None,
                   ia(tr.NBLOCKS), ia(block), ia(scaled), G, keep, boost, sf * nm * nm)
    assert nwg == -(-tr.NBLOCKS[2] // G) * tr.NBLOCKS[0] * tr.NBLOCKS[1], "a phase left part of an embedding unwritten" if nwg < 0 else nwg
    return out


CPU_PAIRS = [tr.PAIRS[0], tr.PAIRS[1], tr.PAIRS[2]]           # down, up, mixed


@pytest.mark.parametrize("block,scaled", CPU_PAIRS, ids=[tr.pair_id(p) for p in CPU_PAIRS])
def test_phases_with_a_serial_selection_against_the_oracle_block_by_block(core, block, scaled):
    """8-bit ends: at most 1 LSB on under 2 % of the samples, the bar of the same comparison for the block == scaled kernel
    (test_topn_roundtrip_against_the_f64_reference).  Float ends against the f64 pixels: 1e-3 of a pixel, test_motion_block_rescale_cpu.py's
    bar for the same float arithmetic.  The volumes' blocks tell the reference's rule from a selection over scaled values (asserted)."""
    ref = tr.case(block, scaled)
    assert ref["gap"] > tr.GAP and ref["differs"] in (True, None) and (ref["differs"] is None) == (block == (4, 4, 4)) and ref["dc_kept"]
    keep = ref["keep"]
    got = run_core(core, ref["vol"], block, scaled, ref["G"], keep)
    diff = np.abs(got.astype(int) - ref["out8"].astype(int))
    print(f"{tr.pair_id((block, scaled))}: keep {keep}, gap {ref['gap']:.2e}, max {diff.max()} LSB, {(diff > 0).mean():.5f} of the bytes differ")
    assert diff.max() <= 1 and (diff > 0).mean() < 0.02, (diff.max(), (diff > 0).mean())
    for g in (1, 2, 7):                 # other groupings, the same bytes
        assert np.array_equal(run_core(core, ref["vol"], block, scaled, g, keep), got)
    reff = tr.case(block, scaled, u8=False)
    assert reff["gap"] > tr.GAP
    sf, nm = mr.consts(block, scaled)
    f = run_core(core, reff["vol"], block, scaled, reff["G"], keep, u8=False)
    err = np.abs(f.astype(np.float64) * sf * nm * nm - reff["pel"]).max()
    print(f"float ends: max error {err:.3e} pixels")
    assert err < 1e-3


def test_the_restored_dc_is_the_one_from_before_the_selection(core):
    """zero-mean blocks moved to a mean of 0.02: the DC is far below the keep-th magnitude, the selection drops it, and boost = 2 with
    preserve_dc = dc puts back the value from BEFORE the selection (motion.c:650, :734).  Restoring what the selection left -- zero -- would
    miss by 0.02 of a pixel on every sample, twenty times the bar."""
    block, scaled = tr.PAIRS[0]
    ref = tr.case(block, scaled, u8=False, mean=0.02, boost_dc=True)
    assert ref["gap"] > tr.GAP and not ref["dc_kept"] and np.all(np.abs(ref["dc_before"]) > 0)
    sf, nm = mr.consts(block, scaled)
    f = run_core(core, ref["vol"], block, scaled, ref["G"], ref["keep"], u8=False, boost=2.0)
    err = np.abs(f.astype(np.float64) * sf * nm * nm - ref["pel"]).max()
    print(f"max error {err:.3e} pixels")
    assert err < 1e-3


def test_refusals_of_the_limit_entries_come_before_any_launch_and_the_topn_entries_still_refuse_a_grid():
    """through the product library with fake pointers: plans of 4-, 8- and 16-point axes need no device tables, so it plans them here"""
    from dspfun_amd import _lib
    L = _lib.load()
    err = L.dspfft_last_error
    block, scaled = (8, 8, 8), (4, 4, 4)
    in_shape, _ = gr.shapes(block, scaled)
    fwd, inv, info = motion_grid_plans(in_shape, block, scaled, lib=L)
    assert info["limit_outside_mul"] == 1.0 and motion_grid_plans((4, 32, 32), (1, 8, 8), (1, 4, 4), lib=L)[2]["limit_outside_mul"] == 2.0

    def cl(keep=16, outside_mul=1.0):
        c = _lib.CoeffLimit()
        c.keep = keep; c.outside_mul = outside_mul
        return C.byref(c)

    f32 = lambda c, a=FAKE, b=FAKE, f=fwd, i=inv: L.dspfft_execute_roundtrip_limit(f._h, i._h, a, b, None, c, None, None)
    u8 = lambda c, a=FAKE, b=FAKE, f=fwd, i=inv: L.dspfft_execute_roundtrip_u8_limit(f._h, i._h, a, b, None, 1.0, None, c, None, None)
    dth = lambda c, w=FAKE, f=fwd, i=inv: L.dspfft_execute_roundtrip_u8_dither_limit(f._h, i._h, FAKE, FAKE, w, 1.0, 1.0, None, c, None, None)
    for call in (f32, u8, dth):
        assert call(None) == -1 and b"null dspfft_coeff_limit" in err()
        assert call(cl(keep=0)) == -1 and b"keep must be at least 1" in err()
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert call(cl(outside_mul=bad)) == -1 and b"outside_mul" in err()
    # misaligned ends
    assert f32(cl(), a=C.c_void_p(4096 + 4)) == -2 and b"aligned" in err()
    assert f32(cl(), b=C.c_void_p(4096 + 8)) == -2 and b"aligned" in err()
    assert u8(cl(), a=C.c_void_p(4096 + 2)) == -2 and b"aligned" in err()
    assert u8(cl(), b=C.c_void_p(4096 + 1)) == -2 and b"aligned" in err()
    assert dth(cl(), w=None) == -1 and b"null plan or buffer" in err()
    # a pair that is almost a grid is refused as the plain call refuses it
    _, inv8, _ = motion_grid_plans((16, 16, 64), block, scaled, lib=L)
    assert f32(cl(), i=inv8) == -2 and b"different numbers of blocks" in err()
    # (the work-buffer check of the unfused passes needs plans with device tables: tests/test_motion_dither_limit_gpu.py)
    # and the entries without a dspfft_coeff_limit refuse a limit in range on a grid pair, as before
    assert L.dspfft_execute_roundtrip_topn(fwd._h, inv._h, FAKE, FAKE, None, 511, None, 0, None, None) == -2 and b"coefficient limit is not implemented" in err()
    assert L.dspfft_execute_roundtrip_u8_topn(fwd._h, inv._h, FAKE, FAKE, None, 1.0, None, 1, None, 0, None, None) == -2 and b"coefficient limit is not implemented" in err()


def test_the_emulation_library_has_the_entries_and_reports_the_missing_kernel():
    from emul_lib import emul
    from dspfun_amd import _lib
    L = emul()
    block, scaled = (8, 8, 8), (4, 4, 4)
    fwd, inv, info = motion_grid_plans(gr.shapes(block, scaled)[0], block, scaled, lib=L)
    c = _lib.CoeffLimit()
    c.keep = 16; c.outside_mul = info["limit_outside_mul"]
    assert L.dspfft_execute_roundtrip_limit(fwd._h, inv._h, FAKE, FAKE, None, C.byref(c), None, None) == -3 and b"not built into this library" in L.dspfft_last_error()
    # f64 plans (the product library plans them with device tables; the check is the same code)
    f64 = Plan.many_r2r([8, 8, 8], [5] * 3, howmany=4, idist=512, odist=512, lib=L, dtype="f64")
    assert L.dspfft_execute_roundtrip_limit(f64._h, f64._h, FAKE, FAKE, None, C.byref(c), None, None) == -1 and b"f32 plans" in L.dspfft_last_error()
    assert L.dspfft_execute_roundtrip_u8_limit(f64._h, f64._h, FAKE, FAKE, FAKE, 1.0, None, C.byref(c), None, None) == -1 and b"f32 plans" in L.dspfft_last_error()
    assert L.dspfft_execute_roundtrip_u8_dither_limit(f64._h, f64._h, FAKE, FAKE, FAKE, 1.0, 1.0, None, C.byref(c), None, None) == -1 and b"f32 plans" in L.dspfft_last_error()
