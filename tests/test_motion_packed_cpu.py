"""motion on packed 8-bit pixels (block_packed.hip, dspfft_execute_roundtrip_u8_packed), the parts that need no device: the refusal of the
emulation library (the kernel is HIP-only), the refusals of the product library ahead of any launch, engine.motion_packed, and the kernel's new
ends and per-component filter (dspfun_amd/csrc/block_packed_core.h) compiled with g++ and walked thread by thread over a NaN-filled tile.
The oracle needs no tolerance: every component block runs the planar kernel's phases, so the packed bytes equal the planar phases run on each
de-interleaved component, and the coded count their sum."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from dspfun_amd import _lib
from dspfun_amd.engine import Plan, DspfftError, motion_grid_plans, motion_packed, PACKED_FORMATS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned address for calls that are refused before anything reads it


def planar_G(block):
    """build_block's rule for the blocks per workgroup of a planar plan whose row holds more blocks than that"""
    bd, bh, bw = block
    return max(1, min(256 // bw, 4096 // (bd * bh * bw)))


def next_prime(n):
    p = n + 1
    while any(p % q == 0 for q in range(2, int(p ** 0.5) + 1)):
        p += 1
    return p


def volume_of(block):
    """2 x 2 x P blocks, P the smallest prime above the planar G: whatever the packed call's G', its last group is short"""
    bd, bh, bw = block
    return (2 * bd, 2 * bh, next_prime(planar_G(block)) * bw)


def plain_packed(comps):
    p = _lib.MotionPacked()
    p.components = comps
    return p


# ---- the emulation library ----
def test_the_emulation_library_answers_minus_3_and_writes_nothing():
    from emul_lib import emul
    L = emul()
    block = (8, 8, 8)
    shape = volume_of(block)
    fwd, inv, info = motion_grid_plans(shape, block, block, lib=L)
    assert "BLOCK 8x8x8" in fwd.describe() and f"{planar_G(block)} blocks per workgroup" in fwd.describe()
    n = int(np.prod(shape)) * 3
    u8 = ol.synth_u8(5, n)
    o8 = np.full(n, 9, dtype=np.uint8)
    p = plain_packed(3)
    rc = L.dspfft_execute_roundtrip_u8_packed(fwd._h, inv._h, u8.ctypes.data, o8.ctypes.data, info["out_mul"], None, C.byref(p), None, None, None)
    assert rc == -3 and b"not built into this library" in L.dspfft_last_error()
    with pytest.raises(DspfftError, match="not built into this library"):
        fwd.roundtrip_u8_packed(inv, u8.ctypes.data, o8.ctypes.data, info["out_mul"], p)
    assert np.all(o8 == 9)


# ---- the product library: every refusal, its code and a reason that names the cause, ahead of any launch ----
def test_refusals_of_the_product_library_come_before_any_launch():
    L = _lib.load()
    err = L.dspfft_last_error
    call = L.dspfft_execute_roundtrip_u8_packed
    block = (8, 8, 8)
    shape = volume_of(block)
    fwd, inv, info = motion_grid_plans(shape, block, block, lib=L)
    mul = info["out_mul"]
    p3 = plain_packed(3)
    # components 1 and 5
    for comps in (1, 5):
        pc = plain_packed(comps)
        assert call(fwd._h, inv._h, FAKE, FAKE, mul, None, C.byref(pc), None, None, None) == -2 and b"components must be 2, 3 or 4" in err() and str(comps).encode() in err()
    # a pair of per-frame 2-D plans: no block pass
    f2 = Plan.many_r2r([12, 20], [5, 5], howmany=4, idist=240, odist=240, lib=L)
    i2 = Plan.many_r2r([12, 20], [4, 4], howmany=4, idist=240, odist=240, lib=L, first_axis_first=True)
    assert call(f2._h, i2._h, FAKE, FAKE, mul, None, C.byref(p3), None, None, None) == -2 and b"fused block pass" in err()
    # an 8x8x8 / 4x4x4 grid pair
    fg, ig, _ = motion_grid_plans(shape, block, (4, 4, 4), lib=L)
    assert call(fg._h, ig._h, FAKE, FAKE, mul, None, C.byref(p3), None, None, None) == -2 and b"rescaled block grid" in err()
    # 16 x 16 x 16 at four components: 64 KB of tiles, no room for the tables
    b16 = (16, 16, 16)
    f16, i16, info16 = motion_grid_plans(volume_of(b16), b16, b16, lib=L)
    p4 = plain_packed(4)
    assert call(f16._h, i16._h, FAKE, FAKE, info16["out_mul"], None, C.byref(p4), None, None, None) == -2 and b"64 KB of LDS" in err()
    # buffers off by 2 bytes
    for a, b in ((4096 + 2, 4096), (4096, 4096 + 2)):
        assert call(fwd._h, inv._h, C.c_void_p(a), C.c_void_p(b), mul, None, C.byref(p3), None, None, None) == -2 and b"4-byte aligned" in err()
    # NULL packed, NULL buffers, an f64 plan
    assert call(fwd._h, inv._h, FAKE, FAKE, mul, None, None, None, None, None) == -1 and b"null dspfft_motion_packed" in err()
    assert call(fwd._h, inv._h, None, FAKE, mul, None, C.byref(p3), None, None, None) == -1 and b"null plan or buffer" in err()
    assert call(None, inv._h, FAKE, FAKE, mul, None, C.byref(p3), None, None, None) == -1 and b"null plan or buffer" in err()
    f64 = Plan.many_r2r([8, 8, 8], [5] * 3, howmany=4, idist=512, odist=512, lib=L, dtype="f64")
    assert call(f64._h, inv._h, FAKE, FAKE, mul, None, C.byref(p3), None, None, None) == -1 and b"f32 plans" in err()
    # a coefficient limit with keep == 0
    cl = _lib.CoeffLimit()
    cl.keep, cl.outside_mul = 0, 1.0
    assert call(fwd._h, inv._h, FAKE, FAKE, mul, None, C.byref(p3), C.byref(cl), None, None) == -1 and b"keep must be at least 1" in err()


# ---- engine.motion_packed ----
def test_motion_packed_places_every_format_components_at_their_bytes():
    want = {"rgb24": (0, 1, 2), "bgr24": (2, 1, 0), "rgba": (0, 1, 2, 3), "bgra": (2, 1, 0, 3), "argb": (1, 2, 3, 0), "abgr": (3, 2, 1, 0), "ya8": (0, 1)}
    assert PACKED_FORMATS == want
    vals = (2.0, 3.0, 5.0, 7.0)          # R, G, B, A (Y, A)
    for fmt, pos in want.items():
        p = motion_packed(fmt, boost=vals[:len(pos)], damp=[v / 16 for v in vals[:len(pos)]])
        assert p.components == len(pos)
        for i, at in enumerate(pos):
            assert p.boost[at] == vals[i] and p.damp[at] == vals[i] / 16, (fmt, i, at)


def test_motion_packed_fills_up_boost_and_damp_as_the_reference_does():
    """motion.c:235-236: a missing entry repeats the one before it; none at all gives 1 for boost and 0 for damp"""
    one = motion_packed("rgba", boost=[3.0], damp=[0.25])
    assert list(one.boost) == [3.0] * 4 and list(one.damp) == [0.25] * 4
    two = motion_packed("argb", boost=[2.0, 0.5], damp=[0.5, 0.125])          # R, G given; B, A repeat G; bytes are A, R, G, B
    assert list(two.boost) == [0.5, 2.0, 0.5, 0.5] and list(two.damp) == [0.125, 0.5, 0.125, 0.125]
    none = motion_packed("rgb24")
    assert list(none.boost)[:3] == [1.0] * 3 and list(none.damp)[:3] == [0.0] * 3
    assert list(motion_packed("rgb24", boost=4.0).boost)[:3] == [4.0] * 3


@pytest.mark.parametrize("dcstop", [False, True])
def test_motion_packed_grey_add_is_the_references_line(dcstop):
    """motion.c:736, per component, at the component's byte"""
    boost, damp, nm, sf = (2.0, 1.0, 0.5), (0.25, 0.5, 0.0), 1.0 / np.sqrt(8.0 * 512), 1.0
    p = motion_packed("bgr24", boost=boost, damp=damp, dcstop=dcstop, normalization=nm, scalefactor=sf)
    for i, at in enumerate((2, 1, 0)):
        want = (1.0 - (damp[i] if dcstop else boost[i])) * 127.5 / (nm * nm * sf)
        assert p.grey_add[at] == np.float32(want)


@pytest.mark.parametrize("fmt", ["rgb0", "0rgb", "bgr0", "0bgr", "gray", "rgb48le", "rgbf32le", "yuv420p", "gbrp"])
def test_motion_packed_refuses_what_is_no_packed_8_bit_format(fmt):
    with pytest.raises(ValueError, match=fmt):
        motion_packed(fmt)


# ---- the header's phases on the CPU: a test-only shim that lays out the geometry the engine derives and walks tid 0..255 through every phase of
# block_rt.h's plain sequence, once with the planar ends on one plane and once with the packed ends on the interleaved clip ----
CPP = r'''
#include <stdint.h>
#include <math.h>
#include <string.h>
#include <vector>
#include "block_packed_core.h"
using namespace dspfft;
// C bytes per pixel (1: a planar plane); volume layout [D][H][W][C] or a block-major stack [blocks][bd][bh][bw][C]
static int geom(BlockGeom &a, const int *nblocks, const int *block, int block_major, int G, int C)
{
	const int nd = nblocks[0], nh = nblocks[1], nw = nblocks[2], bd = block[0], bh = block[1], bw = block[2];
	const long long H = (long long)nh * bh, W = (long long)nw * bw;
	a.nx = bw; a.ny = bh; a.nz = bd; a.G = G; a.pitch = G * C * bw;
	if (block_major) {
		a.rows_fast = 1; a.nxb = nd * nh * nw; a.nd = 0;
		a.sy_in = (long long)bw * C; a.sz_in = (long long)bh * bw * C; a.sxb_in = (long long)bd * bh * bw * C;
	} else {
		a.rows_fast = 0; a.nxb = nw; a.nd = 2;
		a.sy_in = W * C; a.sz_in = H * W * C; a.sxb_in = (long long)bw * C;
		a.bn[0] = nh; a.bis[0] = bh * W * C; a.bn[1] = nd; a.bis[1] = bd * H * W * C;
		for (int d = 0; d < 2; d++) { a.bos[d] = a.bis[d]; a.bdiv[d] = motion_filter_div((uint32_t)a.bn[d]); }
	}
	a.sy_out = a.sy_in; a.sz_out = a.sz_in; a.sxb_out = a.sxb_in;
	a.ngroups = (a.nxb + G - 1) / G; a.gdiv = motion_filter_div((uint32_t)a.ngroups);
	int nwg = a.ngroups;
	for (int d = 0; d < a.nd; d++) nwg *= a.bn[d];
	return nwg;
}
// motion's scales (motion.c:644-647,748-751); a unit axis of the reference's 3-D plans doubles on the way forward and is divided by sqrt 2
static void scales(BlockRtArgs &a, int bd)
{
	const float r2 = sqrtf(2.f), unit = bd == 1 ? r2 : 1.f;
	a.f.scale = 2 * r2 * unit; a.i.scale = unit / (2 * r2);
	for (int k = 0; k < 3; k++) { const bool on = k < 2 || bd > 1; a.f.in0[k] = 1.f; a.f.out0[k] = on ? 1.f / r2 : 1.f; a.i.in0[k] = on ? r2 : 1.f; a.i.out0[k] = 1.f; }
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

template <int NX, int NY, int NZ>
static void seq_planar(const BlockRtArgs &a, int nwg, unsigned long long &mine)
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
		EACH_TID block_store_x<NX, NY, NZ, KIND_REDFT01, true>(a, block_axis_args(a.i, 0, true), nullptr, a.out8, a.mul8, lds, bout, cnt, tid);
	}
}
template <int NX, int NY, int NZ, int C>
static void seq_packed(const BlockPackedArgs &a, int nwg, unsigned long long &mine)
{
	std::vector<float> raw;
	for (int wg = 0; wg < nwg; wg++) {
		long long bin, bout; int cnt;
		block_base(a, (uint32_t)wg, bin, bout, cnt);
		float *lds = nan_tile(raw, (size_t)NZ * NY * a.pitch);
		const int nb = cnt * C;
		EACH_TID packed_load_x<NX, NY, NZ, C>(a, block_axis_args(a.f, 0, NY == 1 && NZ == 1), a.in8, lds, bin, cnt, tid, nullptr);
		if constexpr (NZ > 1) {
			if constexpr (NY > 1) EACH_TID block_lines_y<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.f, 1, false), lds, nb, tid);
			EACH_TID packed_lines_mid<NX, NY, NZ, C, true>(a, block_axis_args(a.f, 2, true), block_axis_args(a.i, 2, false), lds, cnt, tid, mine);
			if constexpr (NY > 1) EACH_TID block_lines_y<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.i, 1, false), lds, nb, tid);
		} else EACH_TID packed_lines_mid<NX, NY, NZ, C, false>(a, block_axis_args(a.f, 1, true), block_axis_args(a.i, 1, false), lds, cnt, tid, mine);
		EACH_TID packed_store_x<NX, NY, NZ, C>(a, block_axis_args(a.i, 0, true), a.out8, a.mul8, lds, bout, cnt, tid, nullptr, TrcParams());
	}
}
#define SHAPES(X) X(4, 4, 1) X(8, 8, 8) X(32, 32, 1) X(4, 16, 8)

extern "C" int group_of(int nx, int ny, int nz, int comps, int nxb) { return packed_group_of(nx, ny, nz, comps, nxb); }

// one plane through the planar phases; fl NULL: no filter; fl[3..5]: damp, boost, grey_add
extern "C" int run_planar(const uint8_t *in8, uint8_t *out8, const int *nblocks, const int *block, int block_major, int G, const float *fl, const int *bp,
                          double mul8, unsigned long long *coded)
{
	BlockRtArgs a;
	memset((void *)&a, 0, sizeof a);
	const int nwg = geom(a, nblocks, block, block_major, G, 1);
	scales(a, block[0]);
	a.in8 = in8; a.out8 = out8; a.mul8 = mul8;
	if (fl) filter(a.filt, block, fl, bp, fl[3], fl[4], fl[5]);
	unsigned long long mine = 0;
#define CASE(X_, Y_, Z_) if (a.nx == X_ && a.ny == Y_ && a.nz == Z_) { seq_planar<X_, Y_, Z_>(a, nwg, mine); *coded += mine; return nwg; }
	SHAPES(CASE)
#undef CASE
	return -1;
}
// the interleaved clip through the packed phases; fl[3..6]: damp, fl[7..10]: boost, fl[11..14]: grey_add, by byte position
extern "C" int run_packed(const uint8_t *in8, uint8_t *out8, const int *nblocks, const int *block, int comps, int block_major, int G, const float *fl, const int *bp,
                          double mul8, unsigned long long *coded)
{
	BlockPackedArgs a;
	memset((void *)&a, 0, sizeof a);
	const int nwg = geom(a, nblocks, block, block_major, G, comps);
	scales(a, block[0]);
	a.in8 = in8; a.out8 = out8; a.mul8 = mul8; a.comps = comps;
	if (fl) {
		filter(a.filt, block, fl, bp, NAN, NAN, NAN);          // (the three scalar fields are not read)
		for (int c = 0; c < 4; c++) { a.damp[c] = fl[3 + c]; a.boost[c] = fl[7 + c]; a.grey_add[c] = fl[11 + c]; }
	}
	unsigned long long mine = 0;
#define CASE(X_, Y_, Z_) if (a.nx == X_ && a.ny == Y_ && a.nz == Z_) { \
		if (comps == 2) seq_packed<X_, Y_, Z_, 2>(a, nwg, mine); else if (comps == 3) seq_packed<X_, Y_, Z_, 3>(a, nwg, mine); else seq_packed<X_, Y_, Z_, 4>(a, nwg, mine); \
		*coded += mine; return nwg; }
	SHAPES(CASE)
#undef CASE
	return -1;
}
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("block_packed_core")
    src, so = d / "core.cpp", d / "core.so"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "dspfun_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.group_of.argtypes = [C.c_int] * 5
    lib.run_planar.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    lib.run_packed.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    return lib


NBLOCKS_OF = lambda block: (2, 2, next_prime(planar_G(block)))


def to_stack(v, block):
    """[D][H][W][...] -> [blocks][bd][bh][bw][...]"""
    bd, bh, bw = block
    D, H, W = v.shape[:3]
    rest = v.shape[3:]
    t = v.reshape((D // bd, bd, H // bh, bh, W // bw, bw) + rest)
    return np.ascontiguousarray(t.transpose((0, 2, 4, 1, 3, 5) + tuple(range(6, 6 + len(rest))))).reshape((-1, bd, bh, bw) + rest)


def run_both(core, block, comps, block_major, filt=None, G=None):
    """the packed phases on an interleaved clip, and the planar phases on each of its planes with that component's values; filt:
    (quantizer, thr_lo, thr_hi, damp[comps], boost[comps], grey_add[comps], band + preserve_dc)"""
    bd, bh, bw = block
    nb = NBLOCKS_OF(block)
    shape = (nb[0] * bd, nb[1] * bh, nb[2] * bw)
    clip = ol.synth_u8(0xC0 + comps + 16 * bd + bw, int(np.prod(shape)) * comps).reshape(shape + (comps,))
    src = to_stack(clip, block) if block_major else clip
    ia = lambda v: (C.c_int * len(v))(*v)
    mul8 = 1.0 / (8.0 * bd * bh * bw)
    nxb = int(np.prod(nb)) if block_major else nb[2]
    Gp = G or core.group_of(bw, bh, bd, comps, nxb)
    assert 1 <= Gp <= nxb and (G or Gp == 1 or Gp * comps * bd * bh * bw <= 8192)          # tiles of at most 32 KB, or one pixel block
    fl = bp = None
    if filt:
        q, lo, hi, damp, boost, grey, band = filt
        pad = lambda v: list(v) + [0.0] * (4 - len(v))
        fl = (C.c_float * 15)(q, lo, hi, *pad(damp), *pad(boost), *pad(grey))
        bp = ia(band)
    out = np.full(src.shape, 0xEE, dtype=np.uint8)
    coded = np.zeros(1, dtype=np.uint64)
    nwg = core.run_packed(src.ctypes.data, out.ctypes.data, ia(nb), ia(block), comps, int(block_major), Gp, fl, bp, mul8, coded.ctypes.data)
    assert nwg == -(-nxb // Gp) * (1 if block_major else nb[0] * nb[1])
    want = np.empty_like(src)
    want_coded = []
    Gl = min(planar_G(block), nxb)
    for c in range(comps):
        plane = np.ascontiguousarray(src[..., c])
        o = np.full(plane.shape, 0xEE, dtype=np.uint8)
        n = np.zeros(1, dtype=np.uint64)
        flc = (C.c_float * 6)(fl[0], fl[1], fl[2], fl[3 + c], fl[7 + c], fl[11 + c]) if filt else None
        assert core.run_planar(plane.ctypes.data, o.ctypes.data, ia(nb), ia(block), int(block_major), Gl, flc, bp, mul8, n.ctypes.data) > 0
        want[..., c] = o
        want_coded.append(int(n[0]))
    return out, want, int(coded[0]), want_coded, Gp, nxb


BLOCKS = [(1, 4, 4), (8, 8, 8), (1, 32, 32), (8, 16, 4)]


@pytest.mark.parametrize("comps", [2, 3, 4])
@pytest.mark.parametrize("block", BLOCKS, ids=["x".join(map(str, b)) for b in BLOCKS])
def test_packed_phases_equal_the_planar_phases_on_every_component(core, block, comps):
    """load, all middle phases and store; index arithmetic, the component-major tile, the short last group.  The tile starts as NaNs."""
    out, want, _, _, Gp, nxb = run_both(core, block, comps, False)
    assert np.array_equal(out, want), int((out != want).sum())
    if Gp > 1:          # another grouping, the same bytes; one of the two has a short last group (the row holds a prime number of blocks)
        assert nxb % Gp or nxb % (Gp - 1)
        assert np.array_equal(run_both(core, block, comps, False, G=Gp - 1)[0], want)


def test_packed_phases_on_a_block_major_stack(core):
    """44 blocks in one row of blocks: the rule's fours, and threes, whose last group is short"""
    for G in (None, 3):
        out, want, _, _, Gp, nxb = run_both(core, (8, 8, 8), 3, True, G=G)
        assert nxb == 44 and Gp == (G or 4)
        assert np.array_equal(out, want), int((out != want).sum())


@pytest.mark.parametrize("block,comps,pdc", [((8, 8, 8), 3, 2), ((1, 32, 32), 4, 1), ((8, 16, 4), 2, 2)])
def test_packed_phases_filter_every_component_with_its_own_values(core, block, comps, pdc):
    """a quantiser, a band with a different damp and boost per component, a threshold and preserve_dc: the bytes are the planar ones of
    each component, the coded count is their sum (and every component contributes another count)"""
    bd, bh, bw = block
    damp, boost, grey = [0.25, 0.5, 0.0, 0.75][:comps], [2.0, 1.0, 0.5, 1.5][:comps], [900.0, -300.0, 0.0, 150.0][:comps]
    band = [1 if bd > 1 else 0, 0, 1, max(1, bd // 2), bh // 2 + 1, bw // 2 + 1, pdc]
    filt = (24.0, 3.0, 1e9, damp, boost, grey, band)
    out, want, coded, want_coded, _, _ = run_both(core, block, comps, False, filt)
    assert np.array_equal(out, want), int((out != want).sum())
    assert coded == sum(want_coded) > 0 and len(set(want_coded)) == comps, (coded, want_coded)
    outb, wantb, codedb, _, _, _ = run_both(core, block, comps, True, filt)
    assert np.array_equal(outb, wantb) and codedb == coded
