"""motion -b with -s over a block grid (block_rescale.hip), the parts that need no device: the refusals of the emulation library (the kernel
is HIP-only) and of the product library ahead of any launch, the plan helper motion_grid_plans, and the kernel's phases
(dspfun_amd/csrc/block_rs_core.h) compiled with g++ and run thread by thread against the f64 restatement of the reference, block by block."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_grid_ref as gr
import motion_ref as mr
import oracle_lib as ol
from dspfun_amd.engine import Plan, DspfftError, motion_grid_plans

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned address for calls that are refused before anything reads it


def test_a_grid_pair_is_refused_by_the_emulation_library_and_nothing_is_written():
    from emul_lib import emul
    L = emul()
    block, scaled = (8, 8, 8), (4, 4, 4)
    in_shape, out_shape = gr.shapes(block, scaled)
    fwd, inv, info = motion_grid_plans(in_shape, block, scaled, lib=L)
    assert "BLOCK 8x8x8" in fwd.describe() and "BLOCK 4x4x4" in inv.describe() and info["out_shape"] == out_shape
    u8 = ol.synth_u8(3, int(np.prod(in_shape)))
    o8 = np.full(int(np.prod(out_shape)), 9, dtype=np.uint8)
    work = np.full(int(np.prod(out_shape)), 7.0, dtype=np.float32)
    rc = L.dspfft_execute_roundtrip_u8(fwd._h, inv._h, u8.ctypes.data, o8.ctypes.data, work.ctypes.data, info["out_mul"], None, None, None)
    assert rc == -3 and b"not built into this library" in L.dspfft_last_error()
    with pytest.raises(DspfftError, match="not built into this library"):
        fwd.roundtrip_u8(inv, u8.ctypes.data, o8.ctypes.data, None, info["out_mul"])
    x = u8.astype(np.float32)
    of = np.full(int(np.prod(out_shape)), 7.0, dtype=np.float32)
    with pytest.raises(DspfftError, match="not built into this library"):
        fwd.roundtrip(inv, x.ctypes.data, of.ctypes.data)
    assert np.all(o8 == 9) and np.all(work == 7.0) and np.all(of == 7.0)


def test_refusals_of_the_product_library_come_before_any_launch():
    """plans of 4-, 8- and 16-point axes need no device tables, so the product library plans them here"""
    from dspfun_amd import _lib
    L = _lib.load()
    err = L.dspfft_last_error
    block, scaled = (8, 8, 8), (4, 4, 4)
    in_shape, _ = gr.shapes(block, scaled)
    fwd, inv, info = motion_grid_plans(in_shape, block, scaled, lib=L)
    call, call8 = L.dspfft_execute_roundtrip, L.dspfft_execute_roundtrip_u8
    # a coefficient limit in range; at the embedding's count (8 x 8 x 8) it would be the plain call
    assert L.dspfft_execute_roundtrip_topn(fwd._h, inv._h, FAKE, FAKE, None, 511, None, 0, None, None) == -2 and b"coefficient limit" in err()
    assert L.dspfft_execute_roundtrip_u8_topn(fwd._h, inv._h, FAKE, FAKE, None, 1.0, None, 1, None, 0, None, None) == -2 and b"coefficient limit" in err()
    # nine blocks along x against eight
    _, inv8, _ = motion_grid_plans((16, 16, 64), block, scaled, lib=L)
    assert call(fwd._h, inv8._h, FAKE, FAKE, None, None, None) == -2 and b"different numbers of blocks" in err()
    # 3-D blocks against 2-D blocks
    _, inv2, _ = motion_grid_plans(in_shape, (1, 8, 8), (1, 4, 4), lib=L)
    assert call(fwd._h, inv2._h, FAKE, FAKE, None, None, None) == -2 and b"different ranks" in err()
    assert call8(fwd._h, inv2._h, FAKE, FAKE, None, 1.0, None, None, None) == -2 and b"different ranks" in err()
    # an extent of 12
    Do, Ho, Wo = 2 * 12, 2 * 12, 9 * 12
    inv12 = Plan.guru([(12, Ho * Wo, Ho * Wo), (12, Wo, Wo), (12, 1, 1)], [(2, 12 * Ho * Wo, 12 * Ho * Wo), (2, 12 * Wo, 12 * Wo), (9, 12, 12)], [4] * 3, lib=L)
    assert call(fwd._h, inv12._h, FAKE, FAKE, None, None, None) == -2 and b"4, 8 or 16" in err()
    # float buffers off 16 bytes, 8-bit buffers off 4
    for a, b in ((4096 + 4, 4096), (4096, 4096 + 8)):
        assert call(fwd._h, inv._h, C.c_void_p(a), C.c_void_p(b), None, None, None) == -2 and b"aligned" in err()
    assert call8(fwd._h, inv._h, C.c_void_p(4096 + 2), FAKE, None, 1.0, None, None, None) == -2 and b"aligned" in err()
    assert call8(fwd._h, inv._h, FAKE, C.c_void_p(4096 + 1), None, 1.0, None, None, None) == -2 and b"aligned" in err()
    # the dithered call needs its work buffer
    assert L.dspfft_execute_roundtrip_u8_dither(fwd._h, inv._h, FAKE, FAKE, None, 1.0, 1.0, None, None, None) == -1 and b"null plan or buffer" in err()
    # and any other pair still needs the work buffer of the 8-bit call
    fb = Plan.many_r2r([8, 8, 8], [5] * 3, howmany=4, idist=512, odist=512, lib=L)
    ib = Plan.many_r2r([8, 8, 8], [4] * 3, howmany=4, idist=512, odist=512, lib=L, first_axis_first=True)
    assert call8(fb._h, ib._h, FAKE, FAKE, None, 1.0, None, None, None) == -1 and b"null plan or buffer" in err()


@pytest.mark.parametrize("shape,block,scaled", [((17, 21, 76), (8, 8, 8), (4, 16, 8)), ((5, 40, 100), (1, 32, 8), (1, 16, 32)), ((16, 16, 72), (8, 8, 8), (8, 8, 8))])
def test_motion_grid_plans_crops_and_carries_motions_constants(shape, block, scaled):
    from emul_lib import emul
    fwd, inv, info = motion_grid_plans(shape, block, scaled, lib=emul())
    nb = tuple(v // b for v, b in zip(shape, block))
    assert info["nblocks"] == nb
    assert info["in_shape"] == tuple(n * b for n, b in zip(nb, block)) and info["out_shape"] == tuple(n * s for n, s in zip(nb, scaled))
    assert info["active"] == tuple(min(b, s) for b, s in zip(block, scaled))
    sf, nm = mr.consts(block, scaled)
    assert info["scalefactor"] == sf and info["normalization"] == pytest.approx(nm, rel=1e-15) and info["out_mul"] == pytest.approx(sf * nm * nm, rel=1e-15)


def test_motion_grid_plans_refuses_what_no_grid_is():
    from emul_lib import emul
    for shape, block, scaled in (((16, 16, 70), (8, 8, 8), (4, 4, 4)),          # a row pitch that is no multiple of 4
                                 ((16, 16, 72), (1, 8, 8), (4, 4, 4)),          # 2-D blocks against 3-D blocks
                                 ((4, 16, 72), (8, 8, 8), (4, 4, 4))):          # no whole block
        with pytest.raises(ValueError):
            motion_grid_plans(shape, block, scaled, lib=emul())


# ---- the header's phases on the CPU: a test-only shim that lays out the geometry the engine derives and walks tid 0..255 through every phase ----
CPP = r'''
#include <stdint.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "block_rs_core.h"
using namespace dspfft;
// in / out: float or 8-bit (the other NULL); volume layout [D][H][W] -> [D'][H'][W'], or block-major stacks of nb blocks
extern "C" int run(const float *in, const uint8_t *in8, float *out, uint8_t *out8, const int *nblocks, const int *block, const int *scaled, int block_major,
                   int G, float quantizer, double mul8, unsigned long long *coded)
{
	const int nd = nblocks[0], nh = nblocks[1], nw = nblocks[2];
	const int bd = block[0], bh = block[1], bw = block[2], sd = scaled[0], sh = scaled[1], sw = scaled[2];
	const long long H = (long long)nh * bh, W = (long long)nw * bw, Ho = (long long)nh * sh, Wo = (long long)nw * sw;
	BlockRsArgs a;
	memset((void *)&a, 0, sizeof a);
	a.nx = bw; a.ny = bh; a.nz = bd; a.ox = sw; a.oy = sh; a.oz = sd;
	a.tw = rs_max(bw, sw); a.G = G; a.pitch = G * a.tw;
	if (block_major) {
		a.rows_fast = 1; a.nxb = nd * nh * nw; a.nd = 0;
		a.sy_in = bw; a.sz_in = (long long)bh * bw; a.sxb_in = (long long)bd * bh * bw;
		a.sy_out = sw; a.sz_out = (long long)sh * sw; a.sxb_out = (long long)sd * sh * sw;
	} else {
		a.rows_fast = 0; a.nxb = nw; a.nd = 2;
		a.sy_in = W; a.sz_in = H * W; a.sxb_in = bw;
		a.sy_out = Wo; a.sz_out = Ho * Wo; a.sxb_out = sw;
		a.bn[0] = nh; a.bis[0] = bh * W; a.bos[0] = sh * Wo;
		a.bn[1] = nd; a.bis[1] = bd * H * W; a.bos[1] = sd * Ho * Wo;
		for (int d = 0; d < 2; d++) a.bdiv[d] = motion_filter_div((uint32_t)a.bn[d]);
	}
	a.ngroups = (a.nxb + G - 1) / G; a.gdiv = motion_filter_div((uint32_t)a.ngroups);
	int nwg = a.ngroups;
	for (int d = 0; d < a.nd; d++) nwg *= a.bn[d];
	a.in = in; a.in8 = in8; a.out = out; a.out8 = out8; a.mul8 = mul8;
	// motion's scales (motion.c:644-647,748-751); a unit axis of the reference's 3-D plans doubles on the way forward and is divided by sqrt 2
	const float r2 = sqrtf(2.f), unit = bd == 1 ? r2 : 1.f;
	a.f.scale = 2 * r2 * unit; a.i.scale = unit / (2 * r2);
	for (int k = 0; k < 3; k++) { const bool on = k < 2 || bd > 1; a.f.in0[k] = 1.f; a.f.out0[k] = on ? 1.f / r2 : 1.f; a.i.in0[k] = on ? r2 : 1.f; a.i.out0[k] = 1.f; }
	if (quantizer > 0.f) {
		MotionFilter &f = a.filt;
		f.ad = bd < sd ? bd : sd; f.ah = bh < sh ? bh : sh; f.aw = bw < sw ? bw : sw; f.mh = f.mw = 1;
		f.b1d = f.ad; f.b1h = f.ah; f.b1w = f.aw;
		f.damp = f.boost = 1.f; f.quantizer = quantizer; f.enabled = 1;
		motion_filter_set_divs(f, 1);
	}
	const RsTile t = rs_tile_of(a);
	std::vector<float> raw(rs_tile_bytes(t) / sizeof(float) + 8, NAN);        // what no phase writes must never be read
	float *lds = (float *)(((uintptr_t)raw.data() + 15) & ~(uintptr_t)15);
	unsigned long long mine = 0;
	for (int wg = 0; wg < nwg; wg++) {
		long long bin, bout; int cnt;
		block_base(a, (uint32_t)wg, bin, bout, cnt);
		for (size_t i = 0; i < rs_tile_bytes(t) / sizeof(float); i++) lds[i] = NAN;
		for (int tid = 0; tid < BLOCK_THREADS; tid++) rs_phase_load(t, lds, bin, cnt, tid, nullptr);
		for (int tid = 0; tid < BLOCK_THREADS; tid++) rs_phase_fwd_y(t, lds, cnt, tid);
		for (int tid = 0; tid < BLOCK_THREADS; tid++) rs_phase_mid(t, lds, cnt, tid, mine);
		for (int tid = 0; tid < BLOCK_THREADS; tid++) rs_phase_inv_y(t, lds, cnt, tid);
		for (int tid = 0; tid < BLOCK_THREADS; tid++) rs_phase_store(t, lds, bout, cnt, tid, nullptr, 0);
	}
	if (coded) *coded += mine;
	return nwg;
}
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("block_rs_core")
    src, so = d / "core.cpp", d / "core.so"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "dspfun_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.run.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_float, C.c_double, C.c_void_p]
    return lib


def engine_G(block, scaled):
    m = [max(b, s) for b, s in zip(block, scaled)]
    return max(1, min(256 // m[2], 8192 // (m[0] * m[1] * m[2]), gr.NBLOCKS[2]))


def run_core(core, vol, block, scaled, block_major, G, u8=True, quant=0.0):
    _, out_shape = gr.shapes(block, scaled)
    ia = lambda v: (C.c_int * 3)(*v)
    src = gr.to_blocks(vol, block) if block_major else vol
    src = np.ascontiguousarray(src if u8 else src.astype(np.float32))
    nb = int(np.prod(gr.NBLOCKS))
    out = np.zeros((nb,) + tuple(scaled) if block_major else out_shape, dtype=np.uint8 if u8 else np.float32)
    coded = np.zeros(1, dtype=np.uint64)
    sf, nm = mr.consts(block, scaled)
    q = gr.quantizer_of(quant, scaled) if quant else 0.0
    nwg = core.run(None if u8 else src.ctypes.data, src.ctypes.data if u8 else None, None if u8 else out.ctypes.data, out.ctypes.data if u8 else None,
                   ia(gr.NBLOCKS), ia(block), ia(scaled), int(block_major), G, q, sf * nm * nm, coded.ctypes.data)
    groups = -(-(nb if block_major else gr.NBLOCKS[2]) // G)
    assert nwg == groups * (1 if block_major else gr.NBLOCKS[0] * gr.NBLOCKS[1])
    return (gr.from_blocks(out, scaled) if block_major else out), int(coded[0])


@pytest.mark.parametrize("block,scaled", gr.PAIRS, ids=[gr.pair_id(p) for p in gr.PAIRS])
def test_phases_against_the_oracle_block_by_block(core, block, scaled):
    """index arithmetic, pruning, the short last group and both layouts; the tile starts as NaNs, so a phase that read what no phase wrote
    would show.  8-bit: at most 1 LSB, fewer than 0.5 % of the bytes (test_motion_rescale.py's caps for this comparison).  Float against the
    f64 pixels: the phases are the float arithmetic of tiny_dct over at most six axes of at most 32 points, far inside 1e-3 of a pixel."""
    ref = gr.case(block, scaled)
    G = engine_G(block, scaled)
    got = {}
    for bm in (False, True):
        got[bm], _ = run_core(core, ref["vol"], block, scaled, bm, G)
        diff = np.abs(got[bm].astype(int) - ref["out8"].astype(int))
        assert diff.max() <= 1 and (diff > 0).mean() < 0.005, (bm, diff.max(), (diff > 0).mean())
    assert np.array_equal(got[False], got[True])
    for g in (1, 2):                    # other groupings, the same bytes
        assert np.array_equal(run_core(core, ref["vol"], block, scaled, False, g)[0], got[False])
    sf, nm = mr.consts(block, scaled)
    f, _ = run_core(core, ref["vol"], block, scaled, False, G, u8=False)
    assert np.abs(f.astype(np.float64) * sf * nm * nm - ref["pel"]).max() < 1e-3


@pytest.mark.parametrize("block,scaled", [gr.PAIRS[0], gr.PAIRS[3], gr.PAIRS[6]], ids=[gr.pair_id(gr.PAIRS[i]) for i in (0, 3, 6)])
def test_phases_with_a_quantiser_count_what_the_oracle_counts(core, block, scaled):
    ref = gr.case(block, scaled, 0.4)
    assert ref["edge"] > gr.EDGE
    got, coded = run_core(core, ref["vol"], block, scaled, False, engine_G(block, scaled), quant=0.4)
    diff = np.abs(got.astype(int) - ref["out8"].astype(int))
    assert diff.max() <= 1 and (diff > 0).mean() < 0.02, (diff.max(), (diff > 0).mean())
    assert coded == ref["nonzero"] > 0
    gotb, codedb = run_core(core, ref["vol"], block, scaled, True, engine_G(block, scaled), quant=0.4)
    assert np.array_equal(gotb, got) and codedb == coded
