"""motion -b with -s over a block grid on packed 8-bit pixels (block_rescale_packed.hip, dspfft_execute_roundtrip_u8_packed_rescale), the parts
that need no device: the refusal of the emulation library (the kernel is HIP-only), the refusals of the product library ahead of any launch,
engine.motion_packed's grey_add for a rescaled pair, the group rule, and the kernel's phases (dspfun_amd/csrc/block_rs_packed_core.h) compiled
with g++ and walked thread by thread over a NaN-filled tile.  Two oracles: the planar grid's phases (block_rs_core.h) on each de-interleaved
component with that component's values -- the bytes and the coded counts are EQUAL, no tolerance --, and the f64 restatement of the
reference (tests/motion_grid_ref.py) with test_motion_block_rescale_cpu.py's caps.
Two tests here are guards that pass without the feature, because they pin what already held and must go on holding: engine.motion_packed's
grey_add with scalefactor != 1 (it was right as it stood), and the small-block entry's refusal of a rescaled pair in its present words."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_grid_ref as gr
import motion_ref as mr
import oracle_lib as ol
from dspfun_amd import _lib
from dspfun_amd.engine import Plan, DspfftError, motion_grid_plans, motion_packed

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAKE = C.c_void_p(4096)               # non-null, 16-byte aligned addresses for calls that are refused before anything reads them,
FAR = C.c_void_p(1 << 40)             # ... far enough apart that no clip planned here reaches from one to the other
TABLES = 256 * 8 + 256 * 4 + 16       # TrcU8Tab and the counter behind a tile (rt_lds_group)
NO_FIT = ((16, 16, 16), (4, 4, 16))   # a pair whose tile is 16 x 16 x 16 floats per component: four of them leave no room for the tables


def plain_packed(comps):
    p = _lib.MotionPacked()
    p.components = comps
    return p


# ---- the emulation library ----
def test_the_emulation_library_answers_minus_3_and_writes_nothing():
    from emul_lib import emul
    L = emul()
    block, scaled = (8, 8, 8), (4, 4, 4)
    in_shape, out_shape = gr.shapes(block, scaled)
    fwd, inv, info = motion_grid_plans(in_shape, block, scaled, lib=L)
    u8 = ol.synth_u8(5, int(np.prod(in_shape)) * 3)
    o8 = np.full(int(np.prod(out_shape)) * 3, 9, dtype=np.uint8)
    p = plain_packed(3)
    rc = L.dspfft_execute_roundtrip_u8_packed_rescale(fwd._h, inv._h, u8.ctypes.data, o8.ctypes.data, info["out_mul"], None, C.byref(p), None, None)
    assert rc == -3 and b"not built into this library" in L.dspfft_last_error()
    with pytest.raises(DspfftError, match="not built into this library"):
        fwd.roundtrip_u8_packed_rescale(inv, u8.ctypes.data, o8.ctypes.data, info["out_mul"], p)
    assert np.all(o8 == 9)


# ---- the product library: every refusal, its code and a reason that names the cause, ahead of any launch ----
def test_refusals_of_the_product_library_come_before_any_launch():
    L = _lib.load()
    err = L.dspfft_last_error
    raw = L.dspfft_execute_roundtrip_u8_packed_rescale
    block, scaled = (8, 8, 8), (4, 4, 4)
    in_shape, _ = gr.shapes(block, scaled)
    fwd, inv, info = motion_grid_plans(in_shape, block, scaled, lib=L)
    mul = info["out_mul"]
    p3, p4 = plain_packed(3), plain_packed(4)
    R = C.byref

    def call(f, i, a=FAKE, b=FAR, fp=None, pk=p3):
        return raw(f._h if f else None, i._h if i else None, a, b, mul, fp, R(pk) if pk is not None else None, None, None)
    # -1: NULL plan, buffer, packed; an f64 plan; bad filter parameters
    assert call(None, inv) == -1 and b"null plan or buffer" in err()
    assert call(fwd, None) == -1 and b"null plan or buffer" in err()
    assert call(fwd, inv, a=None) == -1 and b"null plan or buffer" in err()
    assert call(fwd, inv, b=None) == -1 and b"null plan or buffer" in err()
    assert call(fwd, inv, pk=None) == -1 and b"null dspfft_motion_packed" in err()
    f64 = Plan.many_r2r([8, 8, 8], [5] * 3, howmany=4, idist=512, odist=512, lib=L, dtype="f64")
    assert call(f64, inv) == -1 and b"f32 plans" in err()
    bad = Plan._filter_params(dict(active=info["active"], minbuf_hw=(8, 8), block_depth=8, band_begin=(0, 0, 0), band_end=info["active"], preserve_dc=5))
    assert call(fwd, inv, fp=R(bad)) == -1 and b"bad filter parameters" in err()
    # -2: components 1 and 5
    for comps in (1, 5):
        assert call(fwd, inv, pk=plain_packed(comps)) == -2 and b"components must be 2, 3 or 4" in err() and str(comps).encode() in err()
    # equal extents: the small-block entry's pair
    fe, ie, _ = motion_grid_plans(in_shape, block, block, lib=L)
    assert call(fe, ie) == -2 and b"equal extents" in err() and b"dspfft_execute_roundtrip_u8_packed" in err()
    # a per-frame pair and one block
    f2 = Plan.many_r2r([12, 20], [5, 5], howmany=4, idist=240, odist=240, lib=L)
    i2 = Plan.many_r2r([6, 10], [4, 4], howmany=4, idist=60, odist=60, lib=L, first_axis_first=True)
    assert call(f2, i2) == -2 and b"dspfft_execute_roundtrip_u8_packed_frames" in err()
    f1 = Plan.many_r2r([8, 8, 8], [5] * 3, lib=L)
    i1 = Plan.many_r2r([4, 4, 4], [4] * 3, lib=L, first_axis_first=True)
    assert call(f1, i1) == -2 and b"one block" in err() and b"not implemented" in err()
    # what the planar grid refuses of a pair: block counts, ranks, an extent of 12, the forward plan in the inverse's place
    _, inv8, _ = motion_grid_plans((16, 16, 64), block, scaled, lib=L)
    assert call(fwd, inv8) == -2 and b"different numbers of blocks" in err()
    _, inv2d, _ = motion_grid_plans(in_shape, (1, 8, 8), (1, 4, 4), lib=L)
    assert call(fwd, inv2d) == -2 and b"different ranks" in err()
    Ho, Wo = 2 * 12, 9 * 12
    inv12 = Plan.guru([(12, Ho * Wo, Ho * Wo), (12, Wo, Wo), (12, 1, 1)], [(2, 12 * Ho * Wo, 12 * Ho * Wo), (2, 12 * Wo, 12 * Wo), (9, 12, 12)], [4] * 3, lib=L)
    assert call(fwd, inv12) == -2 and b"4, 8 or 16" in err()
    fwd4, _, _ = motion_grid_plans(gr.shapes(scaled, block)[0], scaled, block, lib=L)
    assert call(fwd, fwd4) == -2 and b"REDFT10 and the inverse REDFT01" in err()
    # buffers off 4 bytes
    for a, b in ((4096 + 2, 1 << 40), (4096, (1 << 40) + 1)):
        assert call(fwd, inv, a=C.c_void_p(a), b=C.c_void_p(b)) == -2 and b"4-byte aligned" in err()
    # the clips' byte ranges intersect: the same address, the output's first byte on the input's last dword, the input inside the output
    in_bytes, out_bytes = int(np.prod(in_shape)) * 3, int(np.prod(gr.shapes(block, scaled)[1])) * 3
    for a, b in ((4096, 4096), (4096, 4096 + in_bytes - 4), (4096 + out_bytes - 4, 4096)):
        assert call(fwd, inv, a=C.c_void_p(a), b=C.c_void_p(b)) == -2 and b"overlap" in err()
        assert str(in_bytes).encode() in err() and str(out_bytes).encode() in err()
    # a 16 x 16 x 16 embedding with 16 active columns at four components: 64 KB of tiles, no room for the tables
    b16, s16 = NO_FIT
    f16, i16, _ = motion_grid_plans(gr.shapes(b16, s16)[0], b16, s16, lib=L)
    assert call(f16, i16, pk=p4) == -2 and b"64 KB of LDS" in err() and b"16x16x16" in err()
    # (more than 2^31 - 1 workgroups: no plan reaches that guard -- the planner refuses a clip of that many blocks for its own passes, "too many
    # tiles for one launch", and its strides are 32 bits wide)
    with pytest.raises(DspfftError, match="too many tiles"):
        motion_grid_plans((8 * 32768, 8 * 32768, 64), block, scaled, lib=L)


def test_the_small_block_entry_still_refuses_a_rescaled_pair_in_its_words():
    L = _lib.load()
    block, scaled = (8, 8, 8), (4, 4, 4)
    fwd, inv, info = motion_grid_plans(gr.shapes(block, scaled)[0], block, scaled, lib=L)
    p3 = plain_packed(3)
    assert L.dspfft_execute_roundtrip_u8_packed(fwd._h, inv._h, FAKE, FAR, info["out_mul"], None, C.byref(p3), None, None, None) == -2
    assert b"(a rescaled block grid, motion -s) are not implemented on packed pixels" in L.dspfft_last_error()


# ---- engine.motion_packed with a rescaled pair's constants ----
@pytest.mark.parametrize("dcstop", [False, True])
@pytest.mark.parametrize("block,scaled", [gr.PAIRS[0], gr.PAIRS[1], gr.PAIRS[5]], ids=[gr.pair_id(gr.PAIRS[i]) for i in (0, 1, 5)])
def test_motion_packed_grey_add_is_the_references_line_for_a_rescaled_pair(block, scaled, dcstop):
    """motion.c:736 with scalefactor = scaled / block (:566) and the normalization of `scaled` (:567), per component at its byte"""
    sf, nm = mr.consts(block, scaled)
    assert sf == np.prod(scaled) / np.prod(block) != 1.0
    boost, damp = (2.0, 1.0, 0.5), (0.25, 0.5, 0.0)
    p = motion_packed("bgr24", boost=boost, damp=damp, dcstop=dcstop, normalization=nm, scalefactor=sf)
    for i, at in enumerate((2, 1, 0)):
        want = (1.0 - (damp[i] if dcstop else boost[i])) * 127.5 / (nm * nm * sf)
        assert p.grey_add[at] == np.float32(want)
    one = motion_packed("bgr24", boost=boost, damp=damp, dcstop=dcstop, normalization=nm, scalefactor=1.0)
    assert [one.grey_add[k] for k in range(3) if one.grey_add[k]] != [p.grey_add[k] for k in range(3) if p.grey_add[k]]


# ---- the header's phases on the CPU: a test-only shim that lays out the geometry the engine derives and walks tid 0..255 through every phase,
# once with the planar grid's phases on one plane and once with the packed phases on the interleaved clip ----
CPP = r'''
#include <stdint.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "block_rs_packed_core.h"
using namespace dspfft;
// C bytes per pixel (1: a planar plane); volume layout [D][H][W][C] -> [D'][H'][W'][C], or block-major stacks
static int geom(BlockRsArgs &a, const int *nblocks, const int *block, const int *scaled, int block_major, int G, int C)
{
	const int nd = nblocks[0], nh = nblocks[1], nw = nblocks[2];
	const int bd = block[0], bh = block[1], bw = block[2], sd = scaled[0], sh = scaled[1], sw = scaled[2];
	const long long H = (long long)nh * bh, W = (long long)nw * bw, Ho = (long long)nh * sh, Wo = (long long)nw * sw;
	a.nx = bw; a.ny = bh; a.nz = bd; a.ox = sw; a.oy = sh; a.oz = sd;
	a.tw = C == 1 ? rs_max(bw, sw) : rs_min(bw, sw); a.G = G; a.pitch = G * C * a.tw;          // (the planar grid's tile; the packed one)
	if (block_major) {
		a.rows_fast = 1; a.nxb = nd * nh * nw; a.nd = 0;
		a.sy_in = (long long)bw * C; a.sz_in = (long long)bh * bw * C; a.sxb_in = (long long)bd * bh * bw * C;
		a.sy_out = (long long)sw * C; a.sz_out = (long long)sh * sw * C; a.sxb_out = (long long)sd * sh * sw * C;
	} else {
		a.rows_fast = 0; a.nxb = nw; a.nd = 2;
		a.sy_in = W * C; a.sz_in = H * W * C; a.sxb_in = (long long)bw * C;
		a.sy_out = Wo * C; a.sz_out = Ho * Wo * C; a.sxb_out = (long long)sw * C;
		a.bn[0] = nh; a.bis[0] = bh * W * C; a.bos[0] = sh * Wo * C;
		a.bn[1] = nd; a.bis[1] = bd * H * W * C; a.bos[1] = sd * Ho * Wo * C;
		for (int d = 0; d < 2; d++) a.bdiv[d] = motion_filter_div((uint32_t)a.bn[d]);
	}
	a.ngroups = (a.nxb + G - 1) / G; a.gdiv = motion_filter_div((uint32_t)a.ngroups);
	int nwg = a.ngroups;
	for (int d = 0; d < a.nd; d++) nwg *= a.bn[d];
	// motion's scales (motion.c:644-647,748-751); a unit axis of the reference's 3-D plans doubles on the way forward and is divided by sqrt 2
	const float r2 = sqrtf(2.f), unit = bd == 1 ? r2 : 1.f;
	a.f.scale = 2 * r2 * unit; a.i.scale = unit / (2 * r2);
	for (int k = 0; k < 3; k++) { const bool on = k < 2 || bd > 1; a.f.in0[k] = 1.f; a.f.out0[k] = on ? 1.f / r2 : 1.f; a.i.in0[k] = on ? r2 : 1.f; a.i.out0[k] = 1.f; }
	return nwg;
}
// the filter over active = min(block, scaled); fl: {quantizer, thr_lo, thr_hi}; bp: band begin (d, h, w), band end (d, h, w), preserve_dc
static void filter(MotionFilter &f, const int *block, const int *scaled, const float *fl, const int *bp, float damp, float boost, float grey_add)
{
	f.ad = rs_min(block[0], scaled[0]); f.ah = rs_min(block[1], scaled[1]); f.aw = rs_min(block[2], scaled[2]); f.mh = f.mw = 1;
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

extern "C" int group_of(int mx, int my, int mz, int lines_in, int lines_out, int comps, int nxb) { return rs_packed_group_of(mx, my, mz, lines_in, lines_out, comps, nxb); }

// one plane through the planar grid's phases; fl NULL: no filter; fl[3..5]: damp, boost, grey_add
extern "C" int run_planar(const uint8_t *in8, uint8_t *out8, const int *nblocks, const int *block, const int *scaled, int block_major, int G, const float *fl,
                          const int *bp, double mul8, unsigned long long *coded)
{
	BlockRsArgs a;
	memset((void *)&a, 0, sizeof a);
	const int nwg = geom(a, nblocks, block, scaled, block_major, G, 1);
	a.in8 = in8; a.out8 = out8; a.mul8 = mul8;
	if (fl) filter(a.filt, block, scaled, fl, bp, fl[3], fl[4], fl[5]);
	const RsTile t = rs_tile_of(a);
	std::vector<float> raw;
	unsigned long long mine = 0;
	for (int wg = 0; wg < nwg; wg++) {
		long long bin, bout; int cnt;
		block_base(a, (uint32_t)wg, bin, bout, cnt);
		float *lds = nan_tile(raw, rs_tile_bytes(t) / sizeof(float));
		EACH_TID rs_phase_load(t, lds, bin, cnt, tid, nullptr);
		EACH_TID rs_phase_fwd_y(t, lds, cnt, tid);
		EACH_TID rs_phase_mid(t, lds, cnt, tid, mine);
		EACH_TID rs_phase_inv_y(t, lds, cnt, tid);
		EACH_TID rs_phase_store(t, lds, bout, cnt, tid, nullptr, 0);
	}
	*coded += mine;
	return nwg;
}
template <int C>
static void seq_packed(const BlockRsPackedArgs &a, int nwg, unsigned long long &mine)
{
	const RsTile t = rs_tile_of(a);
	std::vector<float> raw;
	for (int wg = 0; wg < nwg; wg++) {
		long long bin, bout; int cnt;
		block_base(a, (uint32_t)wg, bin, bout, cnt);
		float *lds = nan_tile(raw, rs_tile_bytes(t) / sizeof(float));
		const int nb = cnt * C;
		EACH_TID rs_packed_phase_load<C>(t, lds, bin, cnt, tid, nullptr);
		EACH_TID rs_phase_fwd_y(t, lds, nb, tid);
		EACH_TID rs_packed_phase_mid<C>(t, a, lds, cnt, tid, mine);
		EACH_TID rs_phase_inv_y(t, lds, nb, tid);
		EACH_TID rs_packed_phase_store<C>(t, lds, bout, cnt, tid, nullptr, TrcParams());
	}
}
// the interleaved clip through the packed phases; fl[3..6]: damp, fl[7..10]: boost, fl[11..14]: grey_add, by byte position
extern "C" int run_packed(const uint8_t *in8, uint8_t *out8, const int *nblocks, const int *block, const int *scaled, int comps, int block_major, int G,
                          const float *fl, const int *bp, double mul8, unsigned long long *coded)
{
	BlockRsPackedArgs a;
	memset((void *)&a, 0, sizeof a);
	const int nwg = geom(a, nblocks, block, scaled, block_major, G, comps);
	a.in8 = in8; a.out8 = out8; a.mul8 = mul8; a.comps = comps;
	if (fl) {
		filter(a.filt, block, scaled, fl, bp, NAN, NAN, NAN);          // (the three scalar fields are not read)
		for (int c = 0; c < 4; c++) { a.damp[c] = fl[3 + c]; a.boost[c] = fl[7 + c]; a.grey_add[c] = fl[11 + c]; }
	}
	unsigned long long mine = 0;
	if (comps == 2) seq_packed<2>(a, nwg, mine); else if (comps == 3) seq_packed<3>(a, nwg, mine); else if (comps == 4) seq_packed<4>(a, nwg, mine); else return -1;
	*coded += mine;
	return nwg;
}
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("block_rs_packed_core")
    src, so = d / "core.cpp", d / "core.so"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "dspfun_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.group_of.argtypes = [C.c_int] * 7
    lib.run_planar.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    lib.run_packed.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    return lib


SHAPES = [((8, 8, 8), (4, 4, 4)), ((4, 4, 4), (8, 8, 8)), ((16, 4, 8), (8, 8, 16)), ((1, 32, 8), (1, 16, 32))]
SHAPE_IDS = [gr.pair_id(p) for p in SHAPES]
NB = int(np.prod(gr.NBLOCKS))
ia = lambda v: (C.c_int * len(v))(*v)


def planar_G(block, scaled, nxb):
    """rt_grid's rule"""
    m = [max(b, s) for b, s in zip(block, scaled)]
    return max(1, min(256 // m[2], 8192 // (m[0] * m[1] * m[2]), nxb))


def tile_dims(block, scaled):
    """(x, y, z) of a component block's tile: the embedding's rows and planes, the active columns"""
    return min(block[2], scaled[2]), max(block[1], scaled[1]), max(block[0], scaled[0])


def rule_G(core, block, scaled, comps, nxb):
    return core.group_of(*tile_dims(block, scaled), block[0] * block[1], scaled[0] * scaled[1], comps, nxb)


def to_stack(v, ext):
    """[D][H][W][C] -> block-major [blocks][d][h][w][C]"""
    d, h, w = ext
    D, H, W, c = v.shape
    return np.ascontiguousarray(v.reshape(D // d, d, H // h, h, W // w, w, c).transpose(0, 2, 4, 1, 3, 5, 6)).reshape(-1, d, h, w, c)


def from_stack(s, ext):
    d, h, w = ext
    nd, nh, nw = gr.NBLOCKS
    c = s.shape[-1]
    return np.ascontiguousarray(s.reshape(nd, nh, nw, d, h, w, c).transpose(0, 3, 1, 4, 2, 5, 6)).reshape(nd * d, nh * h, nw * w, c)


def run_packed(core, clip, block, scaled, block_major, G, filt=None):
    """clip: [D][H][W][C].  Returns (the output clip [D'][H'][W'][C], coded)"""
    comps = clip.shape[-1]
    _, out_shape = gr.shapes(block, scaled)
    src = to_stack(clip, block) if block_major else np.ascontiguousarray(clip)
    out = np.full(((NB,) + tuple(scaled) if block_major else out_shape) + (comps,), 0xEE, dtype=np.uint8)
    sf, nm = mr.consts(block, scaled)
    fl = bp = None
    if filt:
        q, lo, hi, damp, boost, grey, band = filt
        pad = lambda v: list(v) + [0.0] * (4 - len(v))
        fl, bp = (C.c_float * 15)(q, lo, hi, *pad(damp), *pad(boost), *pad(grey)), ia(band)
    coded = np.zeros(1, dtype=np.uint64)
    nwg = core.run_packed(src.ctypes.data, out.ctypes.data, ia(gr.NBLOCKS), ia(block), ia(scaled), comps, int(block_major), G, fl, bp, sf * nm * nm, coded.ctypes.data)
    groups = -(-(NB if block_major else gr.NBLOCKS[2]) // G)
    assert nwg == groups * (1 if block_major else gr.NBLOCKS[0] * gr.NBLOCKS[1])
    return (from_stack(out, scaled) if block_major else out), int(coded[0])


def run_planes(core, clip, block, scaled, block_major, filt=None):
    """the planar grid's phases on every de-interleaved component.  Returns (the interleaved output clip, [coded per component])"""
    comps = clip.shape[-1]
    _, out_shape = gr.shapes(block, scaled)
    sf, nm = mr.consts(block, scaled)
    G = planar_G(block, scaled, NB if block_major else gr.NBLOCKS[2])
    want = np.empty(out_shape + (comps,), dtype=np.uint8)
    counts = []
    for c in range(comps):
        plane = np.ascontiguousarray(clip[..., c])
        src = gr.to_blocks(plane, block) if block_major else plane
        o = np.full((NB,) + tuple(scaled) if block_major else out_shape, 0xEE, dtype=np.uint8)
        flc = bp = None
        if filt:
            q, lo, hi, damp, boost, grey, band = filt
            flc, bp = (C.c_float * 6)(q, lo, hi, damp[c], boost[c], grey[c]), ia(band)
        n = np.zeros(1, dtype=np.uint64)
        assert core.run_planar(src.ctypes.data, o.ctypes.data, ia(gr.NBLOCKS), ia(block), ia(scaled), int(block_major), G, flc, bp, sf * nm * nm, n.ctypes.data) > 0
        want[..., c] = gr.from_blocks(o, scaled) if block_major else o
        counts.append(int(n[0]))
    return want, counts


def clip_of(block, comps):
    in_shape, _ = gr.shapes(block, block)
    return ol.synth_u8(0xB5C + comps + 16 * block[0] + block[2], int(np.prod(in_shape)) * comps).reshape(in_shape + (comps,))


def band_filter(block, scaled, comps, pdc):
    ad, ah, aw = (min(b, s) for b, s in zip(block, scaled))
    damp, boost, grey = [0.25, 0.5, 0.0, 0.75][:comps], [2.0, 1.0, 0.5, 1.5][:comps], [900.0, -300.0, 0.0, 150.0][:comps]
    band = [1 if ad > 1 else 0, 0, 1, max(1, ad // 2), ah // 2 + 1, aw // 2 + 1, pdc]
    return (24.0, 3.0, 1e9, damp, boost, grey, band)


@pytest.mark.parametrize("comps", [2, 3, 4])
@pytest.mark.parametrize("block,scaled", SHAPES, ids=SHAPE_IDS)
def test_packed_phases_equal_the_planar_grid_phases_on_every_component(core, block, scaled, comps):
    """load, the pruned middle phases and store over the component-major tile, in both layouts, with the rule's group and with a group that
    leaves a short last one (nine blocks along x in twos; 36 blocks of a stack in fives).  The tile starts as NaNs."""
    clip = clip_of(block, comps)
    want, _ = run_planes(core, clip, block, scaled, False)
    for bm, nxb, short in ((False, gr.NBLOCKS[2], 2), (True, NB, 5)):
        G = rule_G(core, block, scaled, comps, nxb)
        assert 1 <= G <= nxb
        for g in (G, short):
            got, coded = run_packed(core, clip, block, scaled, bm, g)
            assert np.array_equal(got, want), (bm, g, int((got != want).sum()))
            assert coded == 0
    assert np.array_equal(run_planes(core, clip, block, scaled, True)[0], want)


@pytest.mark.parametrize("block,scaled,comps,pdc", [(SHAPES[0][0], SHAPES[0][1], 3, 2), (SHAPES[1][0], SHAPES[1][1], 4, 1), (SHAPES[2][0], SHAPES[2][1], 2, 2),
                                                    (SHAPES[3][0], SHAPES[3][1], 3, 1)], ids=SHAPE_IDS)
def test_packed_phases_filter_every_component_with_its_own_values(core, block, scaled, comps, pdc):
    """a quantiser, a band inside min(block, scaled) with another damp and boost per component, a threshold and preserve_dc: the bytes are the
    planar ones of each component, the coded count is their sum, and every component contributes another count"""
    clip = clip_of(block, comps)
    filt = band_filter(block, scaled, comps, pdc)
    want, counts = run_planes(core, clip, block, scaled, False, filt)
    assert len(set(counts)) == comps and min(counts) > 0, counts
    assert not np.array_equal(want, run_planes(core, clip, block, scaled, False)[0])
    for bm, nxb, short in ((False, gr.NBLOCKS[2], 2), (True, NB, 5)):
        for g in (rule_G(core, block, scaled, comps, nxb), short):
            got, coded = run_packed(core, clip, block, scaled, bm, g, filt)
            assert np.array_equal(got, want), (bm, g, int((got != want).sum()))
            assert coded == sum(counts)


ORACLE_PAIRS = [gr.PAIRS[0], gr.PAIRS[1], gr.PAIRS[6]]


def oracle_clip(block, scaled, quant=0.0):
    """component c's plane is the grid oracle's seeded volume from seed 100 + 37 c on; returns (the interleaved clip, the per-component cases)"""
    refs = [gr.case(block, scaled, quant, seed0=100 + 37 * c) for c in range(3)]
    return np.ascontiguousarray(np.stack([r["vol"] for r in refs], axis=-1)), refs


@pytest.mark.parametrize("block,scaled", ORACLE_PAIRS, ids=[gr.pair_id(p) for p in ORACLE_PAIRS])
def test_packed_phases_against_the_f64_oracle(core, block, scaled):
    """test_motion_block_rescale_cpu.py's caps for this comparison: at most 1 LSB anywhere, fewer than 0.5 % of the bytes differing"""
    clip, refs = oracle_clip(block, scaled)
    got, _ = run_packed(core, clip, block, scaled, False, rule_G(core, block, scaled, 3, gr.NBLOCKS[2]))
    for c, ref in enumerate(refs):
        diff = np.abs(got[..., c].astype(int) - ref["out8"].astype(int))
        assert diff.max() <= 1 and (diff > 0).mean() < 0.005, (c, diff.max(), (diff > 0).mean())


@pytest.mark.parametrize("block,scaled", ORACLE_PAIRS, ids=[gr.pair_id(p) for p in ORACLE_PAIRS])
def test_packed_phases_with_a_quantiser_count_what_the_oracle_counts(core, block, scaled):
    """fewer than 2 % with quant = 0.4, and, the coefficients being off the rounding boundaries, the oracle's counts exactly"""
    quant = 0.4
    clip, refs = oracle_clip(block, scaled, quant)
    assert all(r["edge"] > gr.EDGE for r in refs)
    active = [min(b, s) for b, s in zip(block, scaled)]
    filt = (gr.quantizer_of(quant, scaled), 0.0, 0.0, [1.0] * 3, [1.0] * 3, [0.0] * 3, [0, 0, 0] + active + [0])
    got, coded = run_packed(core, clip, block, scaled, False, rule_G(core, block, scaled, 3, gr.NBLOCKS[2]), filt)
    for c, ref in enumerate(refs):
        diff = np.abs(got[..., c].astype(int) - ref["out8"].astype(int))
        assert diff.max() <= 1 and (diff > 0).mean() < 0.02, (c, diff.max(), (diff > 0).mean())
    assert coded == sum(r["nonzero"] for r in refs) > 0


# ---- the group rule ----
def test_the_group_rule_fits_the_tile_and_the_tables_into_64_KB(core):
    accepted, refused = 0, []
    for block, scaled in gr.PAIRS + SHAPES + [NO_FIT]:
        m = [max(b, s) for b, s in zip(block, scaled)]
        for comps in (2, 3, 4):
            block_bytes = int(np.prod(tile_dims(block, scaled))) * comps * 4
            for nxb in (1, 9, 36, 240):
                G = rule_G(core, block, scaled, comps, nxb)
                assert 1 <= G <= nxb, (block, scaled, comps, nxb, G)
                if block_bytes + TABLES <= 64 * 1024:          # the engine refuses the others (16 x 16 x 16 at four components)
                    assert G * block_bytes + TABLES <= 64 * 1024, (block, scaled, comps, nxb, G)
                    accepted += 1
                else:
                    refused.append((block, scaled, comps))
    assert accepted and refused == [(NO_FIT[0], NO_FIT[1], 4)] * 4
