"""motion's default block -b 0x0x1 on packed 8-bit pixels (dspfft_execute_roundtrip_u8_packed_frames, dspfft_motion_filter_packed), the parts
that need no device: the component-aware filter functions (dspfun_amd/csrc/motion_filter_packed.h) compiled with g++ and held, bit for bit,
against motion_filter_at on every de-interleaved component with that component's values; every refusal of the product library ahead of any
launch; the refusal of the emulation library (the kernels are HIP-only); and the float64 reference cases of the GPU test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_packed_frames_ref as pf
import motion_spec_ref as sr
from dspfun_amd import _lib
from dspfun_amd.engine import Plan, DspfftError, REDFT01, REDFT10, motion_grid_plans, motion_packed, motion_packed_frame_plans

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAKE = C.c_void_p(4096)          # a non-null, 16-byte aligned address for calls that are refused before anything reads it

CPP = r'''
#include <stdint.h>
#include <string.h>
#include "motion_filter_packed.h"
using namespace dspfft;
// fl: {quantizer, thr_lo, thr_hi}; bp: band begin (d, h, w), band end (d, h, w), preserve_dc
static void filter(MotionFilter &f, int h, int w, const float *fl, const int *bp, float damp, float boost, float grey_add)
{
	memset((void *)&f, 0, sizeof f);
	f.ad = 1; f.ah = h; f.aw = w; f.mh = h; f.mw = w;
	f.b0d = bp[0]; f.b0h = bp[1]; f.b0w = bp[2]; f.b1d = bp[3]; f.b1h = bp[4]; f.b1w = bp[5]; f.preserve_dc = bp[6];
	f.quantizer = fl[0]; f.thr_lo = fl[1]; f.thr_hi = fl[2]; f.damp = damp; f.boost = boost; f.grey_add = grey_add; f.enabled = 1;
	motion_filter_set_divs(f, 1);
}
// one component plane [F][h][w] through motion_filter_at, every frame a block; fl[3..5]: damp, boost, grey_add
extern "C" unsigned long long run_plane(float *c, int F, int h, int w, const float *fl, const int *bp)
{
	MotionFilter f;
	filter(f, h, w, fl, bp, fl[3], fl[4], fl[5]);
	unsigned long long coded = 0;
	for (int b = 0; b < F; b++) for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
		float &v = c[((size_t)b * h + y) * w + x];
		v = motion_filter_at(f, 0, y, x, v, coded);
	}
	return coded;
}
// the interleaved clip [F][h][w][C]; fl[3..6]: damp, fl[7..10]: boost, fl[11..14]: grey_add, by byte position.
// how 0: one element at a time (the kernel's scalar path); 1: groups of four by offset into the whole clip, the first group at `lead` -- they
// straddle pixels, rows and frames --, what is left over one element at a time; 2: groups of four inside rows (the kernel's float4 path; the
// row must be a multiple of 4).  quant_only: what the header derived (out).
extern "C" unsigned long long run_packed(float *c, int F, int h, int w, int C, const float *fl, const int *bp, int how, int lead, int *quant_only)
{
	MotionFilter f;
	filter(f, h, w, fl, bp, NAN, NAN, NAN);          // (the three scalar fields are not read)
	MotionFilterPacked p;
	memset((void *)&p, 0, sizeof p);
	motion_filter_packed_set(p, f, h, w, C, fl + 3, fl + 7, fl + 11);
	*quant_only = p.quant_only;
	const uint32_t row = (uint32_t)w * C, per = row * h, total = per * F;
	unsigned long long coded = 0;
	auto one = [&](uint32_t e) { const uint32_t el = e % per; c[e] = motion_filter_packed_elem(p, el / row, el % row, c[e], coded); };
	if (how == 0) { for (uint32_t e = 0; e < total; e++) one(e); return coded; }
	if (how == 2) {
		if (row % 4) return ~0ull;
		for (int b = 0; b < F; b++) for (uint32_t y = 0; y < (uint32_t)h; y++) for (uint32_t i = 0; i < row; i += 4) {
			float *at = c + (size_t)b * per + (size_t)y * row + i;
			float4 v; v.x = at[0]; v.y = at[1]; v.z = at[2]; v.w = at[3];
			v = motion_filter_packed4_at(p, y, i, v, coded);
			at[0] = v.x; at[1] = v.y; at[2] = v.z; at[3] = v.w;
		}
		return coded;
	}
	uint32_t e = 0;
	for (; e < (uint32_t)lead && e < total; e++) one(e);
	for (; e + 4 <= total; e += 4) {
		float4 v; v.x = c[e]; v.y = c[e + 1]; v.z = c[e + 2]; v.w = c[e + 3];
		v = motion_filter_packed4(p, e, v, coded);
		c[e] = v.x; c[e + 1] = v.y; c[e + 2] = v.z; c[e + 3] = v.w;
	}
	for (; e < total; e++) one(e);
	return coded;
}
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("motion_filter_packed")
    src, so = d / "core.cpp", d / "core.so"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "dspfun_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.run_plane.restype = lib.run_packed.restype = C.c_ulonglong
    lib.run_plane.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.run_packed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


def coefficients(F, h, w, comps):
    """as a forward transform leaves them: a large positive DC per component and frame, values of a few quantiser steps elsewhere, some zeros"""
    q = pf.quantizer_of(h, w)
    rng = np.random.default_rng(0xF17 + comps + 16 * h + w)
    c = (rng.standard_normal((F, h, w, comps)) * 2 * q).astype(np.float32)
    c[rng.random(c.shape) < 0.1] = 0.0
    c[:, 0, 0, :] = ((rng.random((F, comps)) * 10 + 30) * q).astype(np.float32)
    return c


@pytest.mark.parametrize("name", pf.FILTERS[1:])
@pytest.mark.parametrize("F,h,w,comps", pf.FILTER_SHAPES, ids=["x".join(map(str, s)) for s in pf.FILTER_SHAPES])
def test_the_packed_filter_equals_motion_filter_at_on_every_component(core, F, h, w, comps, name):
    """every form of the header -- one element, four by offset from leads 0 .. 3, four inside a row -- gives the bits and the count of
    motion_filter_at on the de-interleaved planes"""
    info = motion_packed_frame_plans(F, h, w, comps, lib=emul_lib())[2]
    filt, packed, planes = pf.settings(h, w, comps, info, name)
    pad = lambda v: list(v)[:4]
    fl = (C.c_float * 15)(filt["quantizer"], filt.get("threshold_lo", 0.0), filt.get("threshold_hi", 0.0), *pad(packed.damp), *pad(packed.boost), *pad(packed.grey_add))
    bp = (C.c_int * 7)(*filt["band_begin"], *filt["band_end"], filt.get("preserve_dc", 0))
    src = coefficients(F, h, w, comps)
    want, counts = np.empty_like(src), []
    for c, pl in enumerate(planes):
        plane = np.ascontiguousarray(src[..., c])
        flc = (C.c_float * 6)(fl[0], fl[1], fl[2], pl["damp"], pl["boost"], pl.get("grey_add", 0.0))
        counts.append(int(core.run_plane(plane.ctypes.data, F, h, w, flc, bp)))
        want[..., c] = plane
    assert sum(counts) > 0 and not np.array_equal(want, src)
    if name != "quant":
        assert len(set(counts)) == comps, counts          # every component's filter is another one
        # preserve_dc: dc puts the DC back, grey adds the component's grey_add to what damp left of it
        dc = src[:, 0, 0, :].astype(np.float64)
        q = filt["quantizer"]
        for at in range(comps):
            before = dc[:, at] if name == "full-dc" else np.float32(np.float32(dc[:, at] * np.float32(packed.damp[at])) + np.float32(packed.grey_add[at]))
            assert np.allclose(want[:, 0, 0, at], np.round(before / q) * q, rtol=1e-6, atol=0), (name, at)
    runs = [(0, 0), (1, 0), (1, 1), (1, 2), (1, 3)] + ([(2, 0)] if (w * comps) % 4 == 0 else [])
    for how, lead in runs:
        got = src.copy()
        qo = C.c_int(-1)
        coded = int(core.run_packed(got.ctypes.data, F, h, w, comps, fl, bp, how, lead, C.byref(qo)))
        assert qo.value == (1 if name == "quant" else 0)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (how, lead, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert coded == sum(counts), (how, lead, coded, counts)


def test_quant_only_holds_only_when_it_holds_for_every_component(core):
    """one component with a boost, or a smaller active block, and positions matter again"""
    F, h, w, comps = 2, 10, 18, 3
    q = pf.quantizer_of(h, w)
    bp = (C.c_int * 7)(0, 0, 0, 1, h, w, 0)
    src = coefficients(F, h, w, comps)
    for damp, boost, want in (([1, 1, 1], [1, 1, 1], 1), ([1, 1, 1], [1, 1, 2], 0), ([0.5, 1, 1], [1, 1, 1], 0), ([1, 1, 1], [1, 2, 1], 0)):
        # (a damp alone never acts while the band is the whole frame, but the planar rule -- motion_filter_set_divs -- asks for damp == 1)
        fl = (C.c_float * 15)(q, 0, 0, *damp, 1, *boost, 1, 0, 0, 0, 0)
        got, qo = src.copy(), C.c_int(-1)
        core.run_packed(got.ctypes.data, F, h, w, comps, fl, bp, 1, 0, C.byref(qo))
        assert qo.value == want, (damp, boost)
        for c in range(comps):
            plane = np.ascontiguousarray(src[..., c])
            core.run_plane(plane.ctypes.data, F, h, w, (C.c_float * 6)(q, 0, 0, damp[c], boost[c], 0), bp)
            assert np.array_equal(plane.view(np.uint32), got[..., c].view(np.uint32)), (damp, boost, c)


def emul_lib():
    from emul_lib import emul
    return emul()


# ---- the emulation library ----
def test_the_emulation_library_answers_minus_3_and_writes_nothing():
    L = emul_lib()
    F, h, w = 2, 10, 12
    fwd, inv, info = motion_packed_frame_plans(F, h, w, 3, lib=L)
    n = F * h * w * 3
    u8 = np.arange(n, dtype=np.uint8)
    wk = np.full(n, 7.0, dtype=np.float32)
    o8 = np.full(n, 9, dtype=np.uint8)
    p = motion_packed("rgb24")
    rc = L.dspfft_execute_roundtrip_u8_packed_frames(fwd._h, inv._h, u8.ctypes.data, o8.ctypes.data, wk.ctypes.data, info["out_mul"], None, C.byref(p), None, None)
    assert rc == -3 and b"not built into this library" in L.dspfft_last_error()
    assert np.all(o8 == 9) and np.all(wk == 7.0)
    with pytest.raises(DspfftError, match="not built into this library"):
        fwd.roundtrip_u8_packed_frames(inv, u8.ctypes.data, o8.ctypes.data, wk.ctypes.data, info["out_mul"], p)
    assert not hasattr(L, "dspfft_motion_filter_packed")


# ---- the product library: every refusal, its code and a reason that names the cause, ahead of any launch ----
def bad_filter(h, w):
    fp = _lib.MotionFilterParams()
    fp.active = (C.c_int * 3)(1, h, w); fp.minbuf_hw = (C.c_int * 2)(h, w); fp.block_depth = 1
    fp.band_end = (C.c_int * 3)(1, h, w)
    fp.damp = fp.boost = 1.0
    fp.preserve_dc = 5
    return fp


def test_refusals_of_the_product_library_come_before_any_launch():
    L = _lib.load()
    err = L.dspfft_last_error
    h, w = 12, 20
    fwd, inv, info = motion_packed_frame_plans(2, h, w, 3, lib=L)
    R = C.byref
    p3, p4 = motion_packed("rgb24"), motion_packed("rgba")
    call = lambda f, i, a, b, wk, fp, pk: L.dspfft_execute_roundtrip_u8_packed_frames(f, i, a, b, wk, info["out_mul"], fp, pk, None, None)
    # -1: a NULL plan, buffer, d_work or packed
    assert call(None, inv._h, FAKE, FAKE, FAKE, None, R(p3)) == -1 and b"null plan or buffer" in err()
    assert call(fwd._h, None, FAKE, FAKE, FAKE, None, R(p3)) == -1 and b"null plan or buffer" in err()
    assert call(fwd._h, inv._h, None, FAKE, FAKE, None, R(p3)) == -1 and b"null plan or buffer" in err()
    assert call(fwd._h, inv._h, FAKE, None, FAKE, None, R(p3)) == -1 and b"null plan or buffer" in err()
    assert call(fwd._h, inv._h, FAKE, FAKE, None, None, R(p3)) == -1 and b"work buffer" in err()
    assert call(fwd._h, inv._h, FAKE, FAKE, FAKE, None, None) == -1 and b"null dspfft_motion_packed" in err()
    # -1: an f64 plan on either side; bad filter parameters
    f64 = lambda kind: Plan.many_r2r([h, w], [kind] * 2, howmany=2, idist=h * w, odist=h * w, lib=L, dtype="f64")
    assert call(f64(REDFT10)._h, inv._h, FAKE, FAKE, FAKE, None, R(p3)) == -1 and b"f32 plans" in err()
    assert call(fwd._h, f64(REDFT01)._h, FAKE, FAKE, FAKE, None, R(p3)) == -1 and b"f32 plans" in err()
    fp = bad_filter(h, w)
    assert call(fwd._h, inv._h, FAKE, FAKE, FAKE, R(fp), R(p3)) == -1 and b"bad filter parameters" in err()
    # -2: components outside 2..4, or not the plans' unit-stride batch level
    for comps in (1, 5):
        pc = motion_packed("rgb24")
        pc.components = comps
        assert call(fwd._h, inv._h, FAKE, FAKE, FAKE, None, R(pc)) == -2 and b"components must be 2, 3 or 4" in err() and str(comps).encode() in err()
    assert call(fwd._h, inv._h, FAKE, FAKE, FAKE, None, R(p4)) == -2 and b"unit-stride batch level counts 3" in err()
    per_frame = lambda kind: Plan.many_r2r([h, w], [kind] * 2, howmany=4, idist=h * w, odist=h * w, lib=L, first_axis_first=kind == REDFT01)
    assert call(per_frame(REDFT10)._h, per_frame(REDFT01)._h, FAKE, FAKE, FAKE, None, R(p3)) == -2 and b"unit-stride batch level counts 0" in err()
    # -2: a small-block pair -- the message names its entry
    sf, si, _ = motion_grid_plans((16, 16, 88), (8, 8, 8), (8, 8, 8), lib=L)
    assert call(sf._h, si._h, FAKE, FAKE, FAKE, None, R(p3)) == -2 and b"small-block pair" in err() and b"dspfft_execute_roundtrip_u8_packed" in err()
    # ... and that entry goes on refusing per-frame pairs, in its present words (tests/test_roundtrip_refusals_cpu.py holds the whole text)
    assert L.dspfft_execute_roundtrip_u8_packed(fwd._h, inv._h, FAKE, FAKE, info["out_mul"], None, R(p3), None, None, None) == -2
    assert b"per-frame and single-block plans have no block pass" in err()
    # -2: rank 3 (one 3-D block)
    cube = lambda kind: Plan.guru([(6, 720, 720), (12, 60, 60), (20, 3, 3)], [(3, 1, 1)], [kind] * 3, lib=L, first_axis_first=kind == REDFT01)
    assert call(cube(REDFT10)._h, cube(REDFT01)._h, FAKE, FAKE, FAKE, None, R(p3)) == -2 and b"one 3-D block" in err()
    # -2: different forward and inverse extents (-s)
    other = motion_packed_frame_plans(2, h, w + 4, 3, lib=L)[1]
    assert call(fwd._h, other._h, FAKE, FAKE, FAKE, None, R(p3)) == -2 and b"different forward / inverse extents" in err()
    # -2: not the dense in-place layout: a padded row pitch, an out-of-place plan -- on either side
    pair = lambda kind, dims, how: Plan.guru(dims, how, [kind] * 2, lib=L, first_axis_first=kind == REDFT01)
    padded = lambda kind: pair(kind, [(h, 66, 66), (w, 3, 3)], [(3, 1, 1), (2, h * 66, h * 66)])
    oop = lambda kind: pair(kind, [(h, 60, 60), (w, 3, 3)], [(3, 1, 1), (2, 720, 1440)])
    for bad in (padded, oop):
        assert call(bad(REDFT10)._h, inv._h, FAKE, FAKE, FAKE, None, R(p3)) == -2 and b"dense in-place layout" in err()
        assert call(fwd._h, bad(REDFT01)._h, FAKE, FAKE, FAKE, None, R(p3)) == -2 and b"dense in-place layout" in err()
    # -2: frame counts that differ; REDFT01 in fwd or REDFT10 in inv; an inverse that runs its row pass first
    assert call(fwd._h, motion_packed_frame_plans(3, h, w, 3, lib=L)[1]._h, FAKE, FAKE, FAKE, None, R(p3)) == -2 and b"over the same frames" in err()
    dense = lambda kind, faf: Plan.guru([(h, w * 3, w * 3), (w, 3, 3)], [(3, 1, 1), (2, h * w * 3, h * w * 3)], [kind] * 2, lib=L, first_axis_first=faf)
    assert call(inv._h, inv._h, FAKE, FAKE, FAKE, None, R(p3)) == -2 and b"REDFT10 (forward) and REDFT01 (inverse)" in err()
    assert call(fwd._h, fwd._h, FAKE, FAKE, FAKE, None, R(p3)) == -2 and b"REDFT10 (forward) and REDFT01 (inverse)" in err()
    assert call(fwd._h, dense(REDFT01, False)._h, FAKE, FAKE, FAKE, None, R(p3)) == -2 and b"column pass first" in err()
    assert call(dense(REDFT10, True)._h, inv._h, FAKE, FAKE, FAKE, None, R(p3)) == -2 and b"column pass first" in err()
    # the Python method raises with the reason
    with pytest.raises(DspfftError, match="unit-stride batch level counts 3"):
        fwd.roundtrip_u8_packed_frames(inv, 4096, 4096, 4096, info["out_mul"], p4)


def test_a_frame_of_2_to_the_32_samples_is_refused():
    """65536 x 32768 pixels of two components: the stand-alone kernel's frame-local offsets are 32 bits wide.  On the emulation library,
    whose engine is the product's: the product library plans no transform of this size without a device for its tables, and this check
    comes ahead of the one for the missing kernels."""
    L = emul_lib()
    h, w = 65536, 32768
    dims, how = [(h, w * 2, w * 2), (w, 2, 2)], [(2, 1, 1)]
    fwd = Plan.guru(dims, how, [REDFT10] * 2, lib=L)
    inv = Plan.guru(dims, how, [REDFT01] * 2, lib=L, first_axis_first=True)
    p = motion_packed("ya8")
    rc = L.dspfft_execute_roundtrip_u8_packed_frames(fwd._h, inv._h, FAKE, FAKE, FAKE, 1.0, None, C.byref(p), None, None)
    assert rc == -2 and b"2^32 samples or more" in L.dspfft_last_error()


# ---- the float64 reference cases of tests/test_motion_packed_frames_gpu.py: the reference alone stays inside the tie cap ----
def test_the_reference_cases_of_the_gpu_test_stay_within_the_tie_share():
    seeds = pf.ref_seeds()
    assert len(seeds) == 3 and len(set(seeds)) == 3
    for kind in pf.REF_KINDS:
        clip, refs = pf.ref_case(kind)
        assert clip.shape == (pf.REF_FRAMES, pf.REF_H, pf.REF_W, 3) and clip.dtype == np.uint8
        for ref in refs:
            sr.check_tie_share(ref, True)
            assert (kind in ("full", "q")) == (ref["coded"] > 0)
            if ref["coeff_tie"] is not None:
                # the seeds keep every coefficient farther than EDGE from a rounding boundary; what the wider window of apply_filter
                # (EDGE + 1.2e-7 |t|) still catches is a handful at most
                assert int(ref["coeff_tie"].sum()) <= 2, int(ref["coeff_tie"].sum())
    # without a filter the reference returns the clip
    clip, refs = pf.ref_case(None)
    assert all(np.array_equal(r["out8"], clip[..., k]) for k, r in enumerate(refs))
