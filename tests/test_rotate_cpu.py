"""rotate (dspfun_amd/csrc/rotate.hip, rotate_core.h, dspfun_amd/rotate.py), the parts that need no device: the parse and the geometry
against the fixture compiled from the reference's own lines, the kernels' phases (rotate_core.h) compiled with g++ and walked workgroup by
workgroup and lane by lane, their 64-bit offsets, the product library's refusals ahead of any launch, and the host tool's build."""
import ctypes as C
import itertools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import rotate_ref as rr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
POISON = 0xA7


# ---- parse and geometry ----
def test_parse_is_the_references_on_all_162_spellings():
    from dspfun_amd import rotate
    fx = rr.fixture()
    assert len(fx["spellings"]) == 162
    for s, m, inv in zip(fx["spellings"], fx["map"], fx["invert"]):
        assert rotate.parse(str(s)) == (tuple(m), tuple(inv)), s
        assert rr.parse(str(s)) == (tuple(m), tuple(inv)), s
    # the 3-cycle quirk: the sign before y lands on input z
    assert rotate.parse("-yzx") == ((1, 2, 0), (1, 0, 0))


def test_parse_refuses_what_the_reference_refuses_and_non_permutations():
    from dspfun_amd import rotate
    fx = rr.fixture()
    assert {"xy", "xyw", "-", ""} <= set(str(s) for s in fx["rejected"])
    for s in [str(s) for s in fx["rejected"]] + ["xxy", "zzz", "x-xz"]:
        with pytest.raises(ValueError):
            rotate.parse(s)


def test_numpy_restatement_is_the_references_loop():
    fx = rr.fixture()
    for s, m, inv, out in zip(fx["spellings"], fx["map"], fx["invert"], fx["out"]):
        assert np.array_equal(rr.rotate(fx["vol"], tuple(m), tuple(inv)).ravel(), out), s


def test_geometry():
    from dspfun_amd import rotate
    w, h, f = 7, 3, 5
    want = {"xyz": (f, h, w), "xzy": (h, f, w), "yxz": (f, w, h), "yzx": (w, f, h), "zxy": (h, w, f), "zyx": (w, h, f)}
    for s, shape in want.items():
        g = rotate.geometry(s, (w, h, f))
        assert g == {"out_shape": shape, "rate": None}, s
    # rotate.c:124 by hand: zy-x at 25/1, -r same: len[map[2]] = len[0] = 7 frames out of 5 in the same time
    assert rotate.geometry("zy-x", (w, h, f), rate=Fraction(25, 1), same_duration=True)["rate"] == Fraction(7 * 25, 5 * 1)
    assert rotate.geometry("zy-x", (w, h, f), rate=Fraction(25, 1))["rate"] == Fraction(25, 1)
    assert rotate.geometry("xzy", (w, h, f), rate=Fraction(30000, 1001), same_duration=True)["rate"] == Fraction(3 * 30000, 5 * 1001)


# ---- rotate_core.h walked sequentially ----
CPP = r'''
#include <stdint.h>
#include <string.h>
#include <vector>
static const unsigned char *g_base; static unsigned char *g_cnt; static uint64_t g_len; static long long g_outside;
static void rot_note(const unsigned char *p, int n)
{
	for (int i = 0; i < n; i++) {
		const long long at = (p - g_base) + i;
		if (at < 0 || (uint64_t)at >= g_len) g_outside++;
		else if (g_cnt[at] < 255) g_cnt[at]++;
	}
}
#define ROT_NOTE_STORE(p, n) rot_note((const unsigned char *)(p), (n))
#include "rotate_core.h"
using namespace dspfft;

template <int E> static void rows(const RotArgs &a)
{
	for (uint64_t wg = 0; wg < a.nwg; wg++)
		for (int tid = 0; tid < ROT_THREADS; tid++) {
			if (a.flip[0]) rot_rows_thread<E, true>(a, wg, tid);
			else rot_rows_thread<1, false>(a, wg, tid);
		}
}
template <int E> static void tiles(const RotArgs &a, uint32_t poison)
{
	std::vector<uint32_t> lds(ROT_LDS_BYTES / 4);
	for (uint64_t wg = 0; wg < a.nwg; wg++) {
		for (auto &v : lds) v = poison;
		const RotTile t = rot_tile_of(a, wg);
		if (E == 1) {
			for (int tid = 0; tid < ROT_THREADS; tid++) rot_tile_load_b(a, t, lds.data(), tid);
			for (int tid = 0; tid < ROT_THREADS; tid++) rot_tile_store_b(a, t, lds.data(), tid);
		} else {
			for (int tid = 0; tid < ROT_THREADS; tid++) rot_tile_load_e<E>(a, t, lds.data(), tid);
			for (int tid = 0; tid < ROT_THREADS; tid++) rot_tile_store_e<E>(a, t, lds.data(), tid);
		}
	}
}
// the walk: every workgroup, every lane; cnt[i]: stores that hit output byte i; returns the stores outside the output (-1: no such case)
extern "C" long long walk(const unsigned char *in, unsigned char *out, unsigned char *cnt, const uint64_t *len, int E, const int *map, const int *invert, uint32_t poison)
{
	if (E < 1 || E > 4 || !rot_is_permutation(map)) return -1;
	RotArgs a;
	memset((void *)&a, 0, sizeof a);
	rot_setup(a, len, E, map, invert);
	a.in = in; a.out = out;
	g_base = out; g_cnt = cnt; g_len = len[0] * len[1] * len[2] * (uint64_t)E; g_outside = 0;
	if (map[0] == 0) { switch (E) { case 1: rows<1>(a); break; case 2: rows<2>(a); break; case 3: rows<3>(a); break; default: rows<4>(a); } }
	else { switch (E) { case 1: tiles<1>(a, poison); break; case 2: tiles<2>(a, poison); break; case 3: tiles<3>(a, poison); break; default: tiles<4>(a, poison); } }
	return g_outside;
}
// the input and output byte offsets the tile phases use for element (x, y, z); no memory is touched
extern "C" int offsets(const uint64_t *len, int E, const int *map, const int *invert, const uint64_t *xyz, uint64_t *in_off, uint64_t *out_off, uint64_t *nwg)
{
	if (map[0] == 0) return -1;
	RotArgs a;
	memset((void *)&a, 0, sizeof a);
	rot_setup(a, len, E, map, invert);
	*nwg = a.nwg;
	const uint64_t tx = xyz[0] / a.tile, ta = xyz[a.a] / a.tile, wg = (xyz[a.b] * a.nta + ta) * a.ntx + tx;
	const RotTile t = rot_tile_of(a, wg);
	const int xl = (int)(xyz[0] - t.x0), al = (int)(xyz[a.a] - t.a0);
	if (t.b != xyz[a.b] || xl < 0 || xl >= t.nx || al < 0 || al >= t.na) return -2;
	*in_off = rot_tile_in_row(a, t, al) + (uint64_t)xl * E;
	int pos = -1;
	for (int p = 0; p < t.na; p++) if (rot_tile_a_of(a, t, p) == al) pos = p;
	if (pos < 0) return -3;
	*out_off = rot_tile_out_row(a, t, xl) + (uint64_t)pos * E;
	return 0;
}
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("rotate_core")
    src, so = d / "core.cpp", d / "core.so"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-I", os.path.join(ROOT, "dspfun_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.walk.restype = C.c_longlong
    lib.walk.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.offsets.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


GUARD = 64


def walk(core, vol, m, inv, in_shift=0, out_shift=0):
    """vol[z][y][x][E] bytes -> the walked output, checked: every byte written exactly once, none outside, the guards untouched, no poison.
    in_shift / out_shift: the base addresses' offsets from a 64-byte boundary."""
    frames, h, w, E = vol.shape
    n = vol.size
    ibuf = np.zeros(n + 2 * GUARD + 64, dtype=np.uint8)
    obuf = np.full(n + 2 * GUARD + 64, 0x5A, dtype=np.uint8)
    i0 = (-ibuf.ctypes.data) % 64 + GUARD + in_shift
    o0 = (-obuf.ctypes.data) % 64 + GUARD + out_shift
    ibuf[i0:i0 + n] = vol.ravel()
    cnt = np.zeros(n, dtype=np.uint8)
    ln = np.array([w, h, frames], dtype=np.uint64)
    mm, ii = np.array(m, dtype=np.int32), np.array(inv, dtype=np.int32)
    outside = core.walk(ibuf.ctypes.data + i0, obuf.ctypes.data + o0, cnt.ctypes.data, ln.ctypes.data, E, mm.ctypes.data, ii.ctypes.data, POISON * 0x01010101)
    assert outside == 0, outside
    assert np.all(obuf[:o0] == 0x5A) and np.all(obuf[o0 + n:] == 0x5A)
    assert np.all(cnt == 1), (int(cnt.min()), int(cnt.max()))
    got = obuf[o0:o0 + n]
    assert not np.any(got == POISON)
    return got.reshape(frames if m[2] == 2 else (h if m[2] == 1 else w), h if m[1] == 1 else (frames if m[1] == 2 else w),
                       w if m[0] == 0 else (h if m[0] == 1 else frames), E)


def test_walk_gives_the_fixtures_bytes(core):
    fx = rr.fixture()
    vol = np.where(fx["vol"] == POISON, 1, fx["vol"]).astype(np.uint8)       # (the poison value is kept out of the input)
    for s, m, inv, out in zip(fx["spellings"], fx["map"], fx["invert"], fx["out"]):
        m, inv = tuple(int(v) for v in m), tuple(int(v) for v in inv)
        want = np.where(out == POISON, 1, out).astype(np.uint8)
        assert np.array_equal(walk(core, vol, m, inv).ravel(), want), s


@pytest.mark.parametrize("E", [1, 2, 3, 4])
def test_walk_against_numpy_on_volumes_around_the_tile(core, E):
    for vi, (w, h, f) in enumerate(rr.volumes(E)):
        vol = rr.pattern(1000 + 10 * E + vi, w * h * f * E, avoid=POISON).reshape(f, h, w, E)
        for spec in rr.maps48():
            m, inv = rr.parse(spec)
            assert np.array_equal(walk(core, vol, m, inv), rr.rotate(vol, m, inv)), (E, (w, h, f), spec)


@pytest.mark.parametrize("E", [1, 2, 3, 4])
def test_walk_from_and_to_bases_that_are_only_element_aligned(core, E):
    """every residue of the output base modulo 16 that the element allows, on a clip whose rows have heads, whole groups and tails"""
    w, h, f = (150, 5, 6) if E == 1 else (70, 5, 6)
    vol = rr.pattern(2000 + E, w * h * f * E, avoid=POISON).reshape(f, h, w, E)
    for k, spec in itertools.product(range(0, 16 // E + 1), ("-xzy", "x-yz", "zyx", "-z-y-x", "yzx", "-zx-y")):
        m, inv = rr.parse(spec)
        assert np.array_equal(walk(core, vol, m, inv, in_shift=E * ((3 * k + 1) % 16), out_shift=E * k), rr.rotate(vol, m, inv)), (E, spec, k)


# ---- 64-bit arithmetic ----
def test_offsets_beyond_32_bits_are_pythons_integers(core):
    w, h, f, E = 70000, 70000, 3, 4
    ln = np.array([w, h, f], dtype=np.uint64)
    for spec in ("zyx", "-y-z-x"):
        m, inv = rr.parse(spec)
        flip = [inv[m[a]] for a in range(3)]
        L = (w, h, f)
        for x, y, z in itertools.product((0, w - 1), (0, h - 1), (0, f - 1)):
            c = (x, y, z)
            o = [L[m[p]] - 1 - c[m[p]] if flip[m[p]] else c[m[p]] for p in range(3)]
            want_in = ((z * h + y) * w + x) * E
            want_out = ((o[2] * L[m[1]] + o[1]) * L[m[0]] + o[0]) * E
            i_off, o_off, nwg = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
            xyz = np.array(c, dtype=np.uint64)
            mm, ii = np.array(m, dtype=np.int32), np.array(inv, dtype=np.int32)
            assert core.offsets(ln.ctypes.data, E, mm.ctypes.data, ii.ctypes.data, xyz.ctypes.data, i_off.ctypes.data, o_off.ctypes.data, nwg.ctypes.data) == 0
            assert (int(i_off[0]), int(o_off[0])) == (want_in, want_out), (spec, c)
    assert want_in > 2 ** 35          # the far corner lies well past 32 bits


# ---- the product library's refusals, all ahead of any launch ----
def test_refusals_of_the_product_library_come_before_any_launch():
    from dspfun_amd import _lib
    L = _lib.load()
    err = L.dspfft_motion_last_error
    U3, I3 = C.c_uint64 * 3, C.c_int * 3
    A, B = C.c_void_p(1 << 20), C.c_void_p(1 << 50)          # fake, non-null, far apart: every call below is refused before anything reads them
    ident, none = I3(2, 1, 0), I3(0, 0, 0)

    def refused(what, out=B, inp=A, ln=(8, 8, 8), E=1, m=ident, inv=none):
        rc = L.dspfft_rotate(out, inp, U3(*ln), E, m, inv, None)
        assert rc != 0 and what in err().decode(), (what, rc, err())

    refused("zero extent", ln=(0, 8, 8))
    refused("zero extent", ln=(8, 0, 8))
    refused("zero extent", ln=(8, 8, 0))
    refused("element size", E=0)
    refused("element size", E=5)
    refused("no permutation", m=I3(0, 0, 1))
    refused("no permutation", m=I3(0, 1, 3))
    refused("null", out=None)
    refused("null", inp=None)
    refused("aligned", inp=C.c_void_p((1 << 20) + 2), E=4)
    refused("aligned", out=C.c_void_p((1 << 50) + 1), E=2)
    # overlap: the same buffer, and ranges that share their last / first element
    refused("overlap", out=A)
    refused("overlap", out=C.c_void_p((1 << 20) + 8 * 8 * 8 * 3 - 3), E=3)
    refused("overlap", out=C.c_void_p((1 << 20) - 8 * 8 * 8 * 3 + 3), E=3)
    # more workgroups than a grid holds: 2^32 rows of 4096 bytes; 2^16 x 2^16 tiles of one column each
    refused("launch grid", ln=(4096, 1 << 20, 1 << 12), m=I3(0, 2, 1))
    refused("launch grid", ln=(1, 1 << 22, 1 << 22), m=I3(2, 1, 0))
    refused("64 bits", ln=(1 << 30, 1 << 30, 1 << 30), E=4)


def test_rotate_dev_builds():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "rotate_dev"])
    assert os.access(os.path.join(ROOT, "host", "rotate_dev"), os.X_OK)
