"""CPU: dspfft_execute_roundtrip_u8 over a clip in slices (engine.cpp roundtrip_sliced: slice plans on the narrow column tile, one reused work area
per stream, a remainder slice) gives the bytes and the count of coded coefficients of the whole clip in three launches -- motion's per-frame
blocks are independent (motion/motion.c:591,613-615).  The slice plans, made at the first such call, are planned as their parents were and follow
the scales their parents are given later.  Through the test-only emulation library; the switches are read once per process, so each setting runs
in a child."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

CHILD = r'''
import math, os, sys, zlib
import numpy as np
sys.path.insert(0, %(here)r); sys.path.insert(0, %(root)r)
import ctypes as C
from emul_lib import emul
from dspfun_amd import Plan, REDFT10, REDFT01
import oracle_lib as ol
L = emul()
frames, h, w = 5, 1080, 960
r2 = math.sqrt(2.0)
colk, rescale = %(colk)r, %(rescale)r
if colk:
    os.environ["DSPFFT_COL_K"] = colk                 # a planner switch while the two plans are made ...
fwd = Plan.many_r2r([h, w], [REDFT10] * 2, howmany=frames, idist=h * w, odist=h * w, lib=L).set_scale(2.0)
inv = Plan.many_r2r([h, w], [REDFT01] * 2, howmany=frames, idist=h * w, odist=h * w, first_axis_first=True, lib=L).set_scale(1.0 / 2.0 / (4.0 * h * w))
for a in range(2):
    fwd.set_axis_scale0(a, 1.0, 1.0 / r2); inv.set_axis_scale0(a, r2, 1.0)
if colk:
    del os.environ["DSPFFT_COL_K"]                    # ... and gone when the first roundtrip makes the slice plans
src = ol.synth_u8(0xD5F0005, frames * h * w)
dst = np.zeros_like(src)
work = np.zeros(frames * h * w, dtype=np.float32)
coded = np.zeros(1, dtype=np.uint64)
flt = dict(active=(1, h, w), minbuf_hw=(h, w), block_depth=1, band_begin=(0, 0, 0), band_end=(1, h, w), quantizer=20.0 * 8 * math.sqrt(w * h))
fwd.roundtrip_u8(inv, src.ctypes.data, dst.ctypes.data, work.ctypes.data, 1.0, filter=flt, d_coded=coded.ctypes.data)
print("RESULT", "%%08x" %% zlib.crc32(dst.tobytes()), int(coded[0]), int(np.abs(dst.astype(int) - src.astype(int)).max()), "sliced" if "roundtrip_u8 in slices of" in fwd.describe() and "K=8" in fwd.describe().split("roundtrip_u8 in slices of")[-1] else "whole", fwd.describe().split("roundtrip_u8 in slices of")[-1][:40].replace(" ", "_"))
for x in fwd.describe().splitlines():
    print("DESCRIBE", x)
if rescale:
    # other scales, so that the quantiser sees other magnitudes
    fwd.set_scale(3.0); inv.set_scale(1.0 / 3.0 / (4.0 * h * w))
    coded[0] = 0
    fwd.roundtrip_u8(inv, src.ctypes.data, dst.ctypes.data, work.ctypes.data, 1.0, filter=flt, d_coded=coded.ctypes.data)
    print("SECOND", "%%08x" %% zlib.crc32(dst.tobytes()), int(coded[0]))
'''


def run_child(env, colk=None, rescale=0):
    e = dict(os.environ); e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD % {"here": HERE, "root": os.path.dirname(HERE), "colk": colk, "rescale": rescale}], env=e, capture_output=True, text=True, timeout=900)
    assert [x for x in r.stdout.splitlines() if x.startswith("RESULT")], r.stderr[-2000:]
    return {tag: [x.split(None, 1)[1] for x in r.stdout.splitlines() if x.startswith(tag + " ")] for tag in ("RESULT", "DESCRIBE", "SECOND")}


def run(env):
    return run_child(env)["RESULT"][0].split()


def test_sliced_clip_is_the_whole_clip():
    whole = run({"DSPFFT_RT_SLICE": "0"})
    assert int(whole[2]) < 64 and int(whole[1]) > 0              # (a quantised roundtrip: close to the input, some coefficients coded)
    for env in ({"DSPFFT_RT_SLICE": "2", "DSPFFT_RT_STREAMS": "2"}, {"DSPFFT_RT_SLICE": "2", "DSPFFT_RT_STREAMS": "1"}, {"DSPFFT_RT_SLICE": "3", "DSPFFT_RT_STREAMS": "2"}):
        got = run(env)
        assert got[:3] == whole[:3], (env, got, whole)
        assert got[3] == "sliced" and whole[3] == "whole", (got, whole)
        assert got[4].startswith("_%s_frames_(last:_%d)_on_%s_stream" % (env["DSPFFT_RT_SLICE"], 5 % int(env["DSPFFT_RT_SLICE"]) or int(env["DSPFFT_RT_SLICE"]), env["DSPFFT_RT_STREAMS"])), got


def test_slice_plans_are_planned_as_their_parents_were():
    """DSPFFT_COL_K=4 is set while the two plans are made and unset before the first roundtrip: the slice plans take it from the parent's snapshot
    of the planner's switches, not from the environment of the call that makes them"""
    d = run_child({"DSPFFT_RT_SLICE": "2", "DSPFFT_RT_STREAMS": "2"}, colk="4")["DESCRIBE"]
    sliced = [x for x in d if "roundtrip_u8 in slices of" in x]
    col = [x for x in d if "COL*" in x and x not in sliced]
    assert len(sliced) == 1 and len(col) == 1, d
    assert col[0].endswith("(generic fallback: K=4)"), col
    assert sliced[0].endswith("(generic fallback: K=4)"), sliced


def test_slices_follow_scales_set_between_runs():
    """run, set other scales on both plans, run again: the second run in slices is the second run of the whole clip, and the quantiser, seeing other
    magnitudes, codes another number of coefficients than in the first"""
    whole = run_child({"DSPFFT_RT_SLICE": "0"}, rescale=1)
    got = run_child({"DSPFFT_RT_SLICE": "2", "DSPFFT_RT_STREAMS": "2"}, rescale=1)
    assert got["RESULT"][0].split()[3] == "sliced" and whole["RESULT"][0].split()[3] == "whole", (got, whole)
    assert got["RESULT"][0].split()[:3] == whole["RESULT"][0].split()[:3], (got, whole)
    assert got["SECOND"] == whole["SECOND"] and len(got["SECOND"]) == 1, (got, whole)
    assert int(got["SECOND"][0].split()[1]) != int(got["RESULT"][0].split()[1]), got
