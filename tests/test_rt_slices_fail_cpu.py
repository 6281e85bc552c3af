"""CPU: a launch that fails in the middle of a clip run in slices (engine.cpp roundtrip_sliced).  The slices alternate between the caller's stream and
one of the library's own; when a slice on the library's stream fails, the call still has to join that stream into the caller's before it returns,
or the library's stream may write the caller's buffers after the caller has synchronised its own stream and freed them.  The emulation library
(tests/emul/backend_emul.cpp) makes the k-th fused column roundtrip of the process return an error code -- an ordinary return value -- and keeps
a trace of event records, stream waits and those launches.
Three frames of 1080 x 960 in slices of one: 1080 is the column length with both a K = 16 and a K = 8 entry, which slicing needs, 960 the shortest
planar row with 8-bit kernels, and three slices are the fewest that put a failure (the second slice, on the library's stream) between a fork and
a join.  The switches are read once per process: each setting is a child."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

CHILD = r'''
import math, os, sys, zlib
import numpy as np
sys.path.insert(0, %(here)r); sys.path.insert(0, %(root)r)
import ctypes as C
from emul_lib import emul
from dspfun_amd import Plan, DspfftError, REDFT10, REDFT01
import oracle_lib as ol
L = emul()
L.dspfft_emul_trace.restype = C.c_size_t
L.dspfft_emul_trace.argtypes = [C.c_char_p, C.c_size_t]
frames, h, w = 3, 1080, 960
r2 = math.sqrt(2.0)
fwd = Plan.many_r2r([h, w], [REDFT10] * 2, howmany=frames, idist=h * w, odist=h * w, lib=L).set_scale(2.0)
inv = Plan.many_r2r([h, w], [REDFT01] * 2, howmany=frames, idist=h * w, odist=h * w, first_axis_first=True, lib=L).set_scale(1.0 / 2.0 / (4.0 * h * w))
for a in range(2):
    fwd.set_axis_scale0(a, 1.0, 1.0 / r2); inv.set_axis_scale0(a, r2, 1.0)
src = ol.synth_u8(0xD5F0005, frames * h * w)
dst = np.zeros_like(src)
work = np.zeros(frames * h * w, dtype=np.float32)
coded = np.zeros(1, dtype=np.uint64)
flt = dict(active=(1, h, w), minbuf_hw=(h, w), block_depth=1, band_begin=(0, 0, 0), band_end=(1, h, w), quantizer=20.0 * 8 * math.sqrt(w * h))
def clip():
    fwd.roundtrip_u8(inv, src.ctypes.data, dst.ctypes.data, work.ctypes.data, 1.0, filter=flt, d_coded=coded.ctypes.data)
if "DSPFFT_EMUL_FAIL_ROUNDTRIP" in os.environ:
    try:
        clip()
        print("ERROR none")
    except DspfftError as e:
        print("ERROR", e)
    buf = C.create_string_buffer(L.dspfft_emul_trace(None, 0) + 1)
    L.dspfft_emul_trace(buf, len(buf))
    for x in buf.value.decode().splitlines():
        print("TRACE", x)
    del os.environ["DSPFFT_EMUL_FAIL_ROUNDTRIP"]
    dst[:] = 0; coded[0] = 0
clip()
print("RESULT", "%%08x" %% zlib.crc32(dst.tobytes()), int(coded[0]), "sliced" if "roundtrip_u8 in slices of" in fwd.describe() else "whole")
'''


def run(env):
    e = dict(os.environ); e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD % {"here": HERE, "root": os.path.dirname(HERE)}], env=e, capture_output=True, text=True, timeout=900)
    assert [x for x in r.stdout.splitlines() if x.startswith("RESULT")], r.stderr[-2000:]
    return {tag: [x.split(None, 1)[1] for x in r.stdout.splitlines() if x.startswith(tag + " ")] for tag in ("ERROR", "TRACE", "RESULT")}


def test_a_failed_slice_on_the_side_stream_is_joined():
    whole = run({"DSPFFT_RT_SLICE": "0"})
    got = run({"DSPFFT_RT_SLICE": "1", "DSPFFT_RT_STREAMS": "2", "DSPFFT_EMUL_FAIL_ROUNDTRIP": "2"})
    assert len(got["ERROR"]) == 1 and "kernel launch failed (fused roundtrip)" in got["ERROR"][0], got["ERROR"]
    trace = got["TRACE"]
    launches = [i for i, x in enumerate(trace) if x.startswith("roundtrip ")]
    # the second launch, on the library's stream (the one stream this backend has created: 1), fails, and none follows it
    assert [trace[i] for i in launches] == ["roundtrip s0 ok", "roundtrip s1 fail"], trace
    after = trace[launches[-1] + 1:]
    records = [(i, re.fullmatch(r"record e(\d+) s1", x)) for i, x in enumerate(after)]
    records = [(i, m.group(1)) for i, m in records if m]
    assert records, trace                                        # an event recorded on the library's stream after the last launch ...
    assert any("wait s0 e%s" % ev in after[i + 1:] for i, ev in records), trace      # ... and the caller's stream made to wait for it
    # the same plans once more, the hook cleared: the clip in slices is the whole clip
    assert whole["RESULT"][0].split()[2] == "whole" and got["RESULT"][0].split()[2] == "sliced", (whole, got)
    assert got["RESULT"][0].split()[:2] == whole["RESULT"][0].split()[:2], (got, whole)
    assert int(whole["RESULT"][0].split()[1]) > 0
