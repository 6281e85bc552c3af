"""TEST INFRASTRUCTURE ONLY: what tests/test_motion_packed_rescale_limit_{cpu,gpu}.py and test_motion_packed_rescale_dither_{cpu,gpu}.py share --
the phases of dspfun_amd/csrc/block_rs_packed_wide_core.h compiled with g++ and walked thread by thread in the kernel's order (a serial
selection that states topn_core.h's rule stands in for the ballot rounds, as in test_motion_grid_topn_cpu.py, and the walk of one thread per plane
for the device's oy lanes per plane, which need a wave's shuffles: the GPU tests hold that schedule to the planar call's bytes), the rgb24 clips built from
tests/motion_grid_topn_ref.py's volumes, the filters, and the GPU tests' guarded output buffers."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import motion_grid_ref as gr
import motion_grid_topn_ref as tr
import motion_ref as mr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRGB = 13          # AVCOL_TRC_IEC61966_2_1
NB = int(np.prod(tr.NBLOCKS))
TABLES = 256 * 8 + 256 * 4 + 16       # TrcU8Tab and the counter behind a tile

CPP = r'''
#include <stdint.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "block_rs_packed_wide_core.h"
using namespace dspfft;
// C bytes per pixel; volume layout [D][H][W][C] -> [D'][H'][W'][C], or block-major stacks; tw: columns of a component block in the tile
static int geom(BlockRsArgs &a, const int *nblocks, const int *block, const int *scaled, int block_major, int G, int C, int tw)
{
	const int nd = nblocks[0], nh = nblocks[1], nw = nblocks[2];
	const int bd = block[0], bh = block[1], bw = block[2], sd = scaled[0], sh = scaled[1], sw = scaled[2];
	const long long H = (long long)nh * bh, W = (long long)nw * bw, Ho = (long long)nh * sh, Wo = (long long)nw * sw;
	a.nx = bw; a.ny = bh; a.nz = bd; a.ox = sw; a.oy = sh; a.oz = sd;
	a.tw = tw; a.G = G; a.pitch = G * C * a.tw;
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
static void filter(MotionFilter &f, const int *block, const int *scaled, const float *fl, const int *bp)
{
	f.ad = rs_min(block[0], scaled[0]); f.ah = rs_min(block[1], scaled[1]); f.aw = rs_min(block[2], scaled[2]); f.mh = f.mw = 1;
	f.b0d = bp[0]; f.b0h = bp[1]; f.b0w = bp[2]; f.b1d = bp[3]; f.b1h = bp[4]; f.b1w = bp[5]; f.preserve_dc = bp[6];
	f.quantizer = fl[0]; f.thr_lo = fl[1]; f.thr_hi = fl[2]; f.damp = f.boost = f.grey_add = NAN; f.enabled = 1;     // (the three scalar fields are not read)
	motion_filter_set_divs(f, 1);
}
static float *nan_tile(std::vector<float> &raw, size_t n)          // what no phase writes must never be read
{
	raw.assign(n + 8, NAN);
	return (float *)(((uintptr_t)raw.data() + 15) & ~(uintptr_t)15);
}
// topn_core.h's rule on tile block gb: key = the bit pattern of |value|, the `keep` largest stay, ties to the smaller e = (z MY + y) MX + x
static void select_block(float *lds, const RsTile &t, int gb, unsigned keep, bool restore)
{
	const int mx = t.tw, E = rs_topn_elems(t);
	auto at = [&](int e) -> float & { return lds[(e / mx) * t.pitch + gb * t.tw + e % mx]; };
	const float dc = at(0);
	std::vector<int> order(E);
	std::vector<uint32_t> key(E);
	for (int e = 0; e < E; e++) { order[e] = e; const float v = at(e); uint32_t b; memcpy(&b, &v, 4); key[e] = b & 0x7fffffffu; }
	std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return key[p] > key[q]; });
	for (int r = (int)keep; r < E; r++) at(order[r]) = 0.f;
	if (restore) at(0) = dc;
}
#define EACH_TID for (int tid = 0; tid < BLOCK_THREADS; tid++)

// the kernel's sequence (block_rescale_packed_wide_kernel); dump: NULL, or the floats the inverse's x pass leaves in the tile, in the output
// clip's layout.  -1: the selection would read an element of an embedding that no phase wrote
template <int C>
static int seq(const BlockRsPackedWideArgs &a, int nwg, const double *thr, const TrcParams &tp, float *dump, unsigned long long &mine)
{
	const RsTile t = rs_tile_of(a), all = rs_tile_unpruned(t);
	const RsKeys keys = rs_keys_of(a);
	const int my = rs_max(t.ny, t.oy);
	std::vector<float> raw;
	double tab[256];
	if (a.dither) dither_table(tab, a.sf, a.norm);
	std::vector<double> dprow((size_t)(a.dither ? a.slots * a.ox : 0), NAN);
	for (int wg = 0; wg < nwg; wg++) {
		long long bin, bout; int cnt;
		block_base(a, (uint32_t)wg, bin, bout, cnt);
		float *lds = nan_tile(raw, rs_tile_bytes(t) / sizeof(float));
		const int nb = cnt * C;
		if (a.keep) {
			EACH_TID { rs_packed_phase_load<C>(all, lds, bin, cnt, tid, nullptr); rs_phase_zero_outside(t, lds, nb, tid); }
			EACH_TID rs_phase_fwd_y(all, lds, nb, tid);
			EACH_TID rs_phase_fwd_last_keys(t, keys, lds, nb, tid);
			for (int gb = 0; gb < nb; gb++) {
				for (int e = 0; e < rs_topn_elems(t); e++) if (isnan(lds[(e / t.tw) * t.pitch + gb * t.tw + e % t.tw])) return -1;
				select_block(lds, t, gb, a.keep, motion_filter_restores_dc(packed_filter_of<C>(a, packed_comp_of<C>(gb, cnt), t.filt)));
			}
			EACH_TID rs_packed_phase_filt_inv_last<C>(t, a, lds, cnt, tid, mine);
		} else {
			EACH_TID rs_packed_phase_load<C>(t, lds, bin, cnt, tid, nullptr);
			EACH_TID rs_phase_fwd_y(t, lds, nb, tid);
			EACH_TID rs_packed_phase_mid<C>(t, a, lds, cnt, tid, mine);
		}
		EACH_TID rs_phase_inv_y(t, lds, nb, tid);
		if (a.dither) {
			EACH_TID rs_packed_phase_inverse_x<C>(t, lds, cnt, tid);
			if (dump)
				for (int g = 0; g < cnt; g++) for (int c = 0; c < C; c++) for (int z = 0; z < t.oz; z++) for (int y = 0; y < t.oy; y++) for (int x = 0; x < t.ox; x++)
					dump[bout + g * t.sxb_out + z * t.sz_out + y * t.sy_out + x * C + c] = lds[(z * my + y) * t.pitch + (c * cnt + g) * t.tw + x];
			EACH_TID rs_packed_phase_dither<C>(t, a.sf, a.norm, lds, cnt, tid, tab, dprow.data(), thr, tp);
			EACH_TID rs_packed_phase_store_bytes<C>(t, lds, bout, cnt, tid);
		} else if (a.keep) {          // with a limit the store runs in two phases
			EACH_TID rs_packed_phase_inverse_x<C>(t, lds, cnt, tid);
			EACH_TID rs_packed_phase_store_quant<C>(t, lds, bout, cnt, tid, nullptr, TrcParams());
		} else EACH_TID rs_packed_phase_store<C>(t, lds, bout, cnt, tid, nullptr, TrcParams());
	}
	return nwg;
}
// the interleaved clip through the wide tile's phases.  keep 0: no limit; dither: -d with sf, norm and (trc != 0) the output's transfer
// characteristic; fl NULL: no filter, else fl[3..6]: damp, fl[7..10]: boost, fl[11..14]: grey_add, by byte position
extern "C" int run_wide(const uint8_t *in8, uint8_t *out8, float *dump, const int *nblocks, const int *block, const int *scaled, int comps, int block_major, int G,
                        unsigned keep, double outside_mul, int dither, double sf, double norm, int trc, const float *fl, const int *bp, double mul8, unsigned long long *coded)
{
	BlockRsPackedWideArgs a;
	memset((void *)&a, 0, sizeof a);
	const int nwg = geom(a, nblocks, block, scaled, block_major, G, comps, rs_packed_wide_tw(block[2], scaled[2], keep != 0));
	a.in8 = in8; a.out8 = out8; a.mul8 = mul8; a.comps = comps;
	if (fl) {
		filter(a.filt, block, scaled, fl, bp);
		for (int c = 0; c < 4; c++) { a.damp[c] = fl[3 + c]; a.boost[c] = fl[7 + c]; a.grey_add[c] = fl[11 + c]; }
	}
	// the keys' factors as engine.cpp's rt_packed_grid derives them
	a.keep = keep; a.key_mul = (float)(outside_mul / (double)a.f.scale);
	for (int k = 0; k < 3; k++) a.key_mul0[k] = 1.f / a.f.out0[k];
	a.dither = dither; a.sf = sf; a.norm = norm; a.slots = packed_dither_slots(a.oz, comps, G);
	if (!rs_packed_wide_lds(a, nwg, rs_tile_bytes(rs_tile_of(a)))) return -2;       // what the launchers refuse
	double thr[256];
	TrcParams tp = TrcParams();
	if (trc) { if (!trc_built(trc)) return -3; trc_u8_thresholds(thr, trc); tp = trc_params(trc); }
	unsigned long long mine = 0;
	int rc = -4;
	if (comps == 2) rc = seq<2>(a, nwg, trc ? thr : nullptr, tp, dump, mine); else if (comps == 3) rc = seq<3>(a, nwg, trc ? thr : nullptr, tp, dump, mine);
	else if (comps == 4) rc = seq<4>(a, nwg, trc ? thr : nullptr, tp, dump, mine);
	*coded += mine;
	return rc;
}
// the planar dithered store's walk of one dense h x w plane with a transfer characteristic (dither_core.h)
extern "C" void walk_serial_trc(uint8_t *out, const float *in, int h, int w, double sf, double norm, int trc)
{
	double tab[256], thr[256];
	dither_table(tab, sf, norm);
	std::vector<double> dprow(w);
	trc_u8_thresholds(thr, trc);
	const TrcParams tp = trc_params(trc);
	dither_plane_serial<true>(out, in, w, h, w, sf, norm, tab, dprow.data(), 1, thr, &tp);
}
extern "C" int group_of(int mx, int my, int mz, int lines_in, int lines_out, int comps, int nxb) { return rs_packed_group_of(mx, my, mz, lines_in, lines_out, comps, nxb); }
extern "C" int wide_tw(int nx, int ox, int limit) { return rs_packed_wide_tw(nx, ox, limit != 0); }
extern "C" long long wide_dither_bytes(int ox, int oz, int comps, int G) { return (long long)rs_packed_wide_dither_bytes(ox, oz, comps, G, true, false); }          // (one lane per plane: the larger)
'''


@functools.lru_cache(maxsize=None)
def core():
    """the shim, compiled once per session into a directory of its own under the system's temporary directory"""
    import tempfile
    d = tempfile.mkdtemp(prefix="block_rs_packed_wide_core")
    src, so = os.path.join(d, "core.cpp"), os.path.join(d, "core.so")
    with open(src, "w") as f:
        f.write(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "dspfun_amd", "csrc"), src, "-o", so])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.run_wide.argtypes = [vp] * 6 + [C.c_int] * 3 + [C.c_uint, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, vp, vp, C.c_double, vp]
    lib.walk_serial_trc.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
    lib.group_of.argtypes = [C.c_int] * 7
    lib.wide_tw.argtypes = [C.c_int] * 3
    lib.wide_dither_bytes.argtypes = [C.c_int] * 4
    lib.wide_dither_bytes.restype = C.c_longlong
    return lib


ia = lambda v: (C.c_int * len(v))(*v)


def rule_G(block, scaled, comps, nxb, limit, dither):
    """engine.cpp's rt_packed_grid: rs_packed_group_of's rule on the wide tile, shrunk until everything fits 64 KB; 0: not even one pixel block does"""
    lib = core()
    tw = lib.wide_tw(block[2], scaled[2], int(limit))
    my, mz = max(block[1], scaled[1]), max(block[0], scaled[0])
    G = lib.group_of(tw, my, mz, block[0] * block[1], scaled[0] * scaled[1], comps, nxb)
    block_bytes = tw * my * mz * comps * 4
    total = lambda g: g * block_bytes + TABLES + (lib.wide_dither_bytes(scaled[2], scaled[0], comps, g) if dither else 0)
    while G > 0 and total(G) > 64 * 1024:
        G -= 1
    while dither and G > 1 and total(G) > 40 * 1024:          # -d: four workgroups to a CU's 160 KB
        G -= 1
    return G


def fits(block, scaled, comps, G, limit, dither):
    """whether a forced group of G pixel blocks stays within 64 KB (the engine shrinks one that does not)"""
    lib = core()
    block_bytes = lib.wide_tw(block[2], scaled[2], int(limit)) * max(block[1], scaled[1]) * max(block[0], scaled[0]) * comps * 4
    return G * block_bytes + TABLES + (lib.wide_dither_bytes(scaled[2], scaled[0], comps, G) if dither else 0) <= 64 * 1024


def to_stack(v, ext):
    """[D][H][W][C] -> block-major [blocks][d][h][w][C]"""
    d, h, w = ext
    D, H, W, c = v.shape
    return np.ascontiguousarray(v.reshape(D // d, d, H // h, h, W // w, w, c).transpose(0, 2, 4, 1, 3, 5, 6)).reshape(-1, d, h, w, c)


def from_stack(s, ext, nblocks=tr.NBLOCKS):
    d, h, w = ext
    nd, nh, nw = nblocks
    c = s.shape[-1]
    return np.ascontiguousarray(s.reshape(nd, nh, nw, d, h, w, c).transpose(0, 3, 1, 4, 2, 5, 6)).reshape(nd * d, nh * h, nw * w, c)


def run_wide(clip, block, scaled, G, keep=0, outside_mul=None, dither=False, trc=0, filt=None, block_major=False):
    """clip: [D][H][W][C] over tr.NBLOCKS blocks.  Returns (the output clip [D'][H'][W'][C], coded, with dither the floats that were dithered)"""
    comps = clip.shape[-1]
    _, out_shape = gr.shapes(block, scaled, tr.NBLOCKS)
    src = to_stack(clip, block) if block_major else np.ascontiguousarray(clip)
    shape = ((NB,) + tuple(scaled) if block_major else out_shape) + (comps,)
    out = np.full(shape, 0xEE, dtype=np.uint8)
    dump = np.full(shape, np.nan, dtype=np.float32) if dither else None
    sf, nm = mr.consts(block, scaled)
    fl = bp = None
    if filt:
        q, lo, hi, damp, boost, grey, band = filt
        pad = lambda v: list(v) + [0.0] * (4 - len(v))
        fl, bp = (C.c_float * 15)(q, lo, hi, *pad(damp), *pad(boost), *pad(grey)), ia(band)
    coded = np.zeros(1, dtype=np.uint64)
    if outside_mul is None:
        outside_mul = 2.0 if block[0] == 1 else 1.0           # motion_grid_plans' info["limit_outside_mul"]
    nwg = core().run_wide(src.ctypes.data, out.ctypes.data, dump.ctypes.data if dither else None, ia(tr.NBLOCKS), ia(block), ia(scaled), comps, int(block_major), G,
                          keep, outside_mul, int(dither), sf, nm, trc, fl, bp, sf * nm * nm, coded.ctypes.data)
    groups = -(-(NB if block_major else tr.NBLOCKS[2]) // G)
    assert nwg == groups * (1 if block_major else tr.NBLOCKS[0] * tr.NBLOCKS[1]), {-1: "a phase left part of an embedding unwritten", -2: "the launchers would refuse this"}.get(nwg, nwg)
    if block_major:
        out, dump = from_stack(out, scaled), (from_stack(dump, scaled) if dither else None)
    return out, int(coded[0]), dump


def topn_clip(block, scaled, comps=3):
    """component c's plane is motion_grid_topn_ref's seeded volume from seed 500 + 37 c on: (the interleaved clip, the per-component cases)"""
    refs = [tr.case(block, scaled, seed0=500 + 37 * c) for c in range(comps)]
    return np.ascontiguousarray(np.stack([r["vol"] for r in refs], axis=-1)), refs


def band_filter(block, scaled, comps, pdc):
    """test_motion_packed_rescale_cpu.py's: a quantiser, a band inside min(block, scaled) with another damp and boost per component, a threshold"""
    ad, ah, aw = (min(b, s) for b, s in zip(block, scaled))
    damp, boost, grey = [0.25, 0.5, 0.0, 0.75][:comps], [2.0, 1.0, 0.5, 1.5][:comps], [900.0, -300.0, 0.0, 150.0][:comps]
    band = [1 if ad > 1 else 0, 0, 1, max(1, ad // 2), ah // 2 + 1, aw // 2 + 1, pdc]
    return (24.0, 3.0, 1e9, damp, boost, grey, band)


# ---- the GPU tests: a device buffer with a marker page on each side of the output ----
PAGE, MARK = 4096, 0xA5


def guarded(nbytes, fill=0xEE):
    """(the whole uint8 device tensor, the view of nbytes bytes between the two marker pages)"""
    import torch
    whole = torch.full((nbytes + 2 * PAGE,), MARK, dtype=torch.uint8, device="cuda")
    view = whole[PAGE:PAGE + nbytes]
    view.fill_(fill)
    return whole, view


def markers_intact(whole, nbytes):
    w = whole.cpu().numpy()
    return bool(np.all(w[:PAGE] == MARK) and np.all(w[PAGE + nbytes:] == MARK))
