"""Regenerates tests/golden/ref_rotate.npz from the REFERENCE'S OWN rotate (build container only: needs the reference tree and gcc).

  motion/rotate.c:74-89     the parse of the permutation argument: signs, letters, the usage() exits
  motion/rotate.c:159-164   the loop that writes every output pixel from the input buffer

The text of those line ranges is read from the reference at generation time into a temporary translation unit, around this script's own
declarations: usage() and ffapi_setpixel are macros, `buf` is the clip as rotate.c:139 declares it, and the closing brace of the frame loop
(whose body goes on with the container's frame write, :165-172) is supplied.  No reference text is written to the repository; only the
spellings, the parsed map / invert and the output bytes go into the fixture file.

For the 162 spellings (6 letter orders x {none, '-', '+'} per letter) of a 7 x 3 x 5 clip of 2-byte elements: spelling, map, invert, bytes;
and for strings the reference rejects, that it does.
"""
import ctypes as C
import itertools
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DSPFUN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
from oracle_lib import splitmix64_stream  # noqa: E402

W, H, FRAMES, COMPONENTS = 7, 3, 5, 2
REJECTED = ["xy", "xyw", "-", "", "x", "+-xyz", "XYZ"]


def lines(path, a, b):
    with open(os.path.join(REF, path)) as f:
        src = f.read().split("\n")
    return "\n".join(src[a - 1:b]) + "\n"


def spellings():
    out = []
    for order in itertools.permutations("xyz"):
        for signs in itertools.product(("", "-", "+"), repeat=3):
            out.append("".join(s + l for s, l in zip(signs, order)))
    return out


def build(tmp):
    tu = """#include <stdint.h>
#include <stdbool.h>
#include <string.h>
#include <setjmp.h>
static jmp_buf rejected;
#define usage() longjmp(rejected, 1)
#define ffapi_setpixel(out, oframe, x, y, pel) memcpy(dst + ((axis[map[2]] * len[map[1]] + (y)) * len[map[0]] + (x)) * components, (pel), components)
/* 0: parsed (and, with src, rotated); 1: the reference's usage() */
int ref_rotate(char *spec, const uint64_t *len_, int components, const unsigned char *src, unsigned char *dst, int *map_out, int *invert_out)
{
	char *args[1] = {spec};
	char **argv = args;
	uint64_t len[3] = {len_[0], len_[1], len_[2]};
	if (setjmp(rejected)) return 1;
"""
    tu += lines("motion/rotate.c", 74, 89)
    tu += """
	for (int i = 0; i < 3; i++) { map_out[i] = map[i]; invert_out[i] = invert[i]; }
	if (!src) return 0;
	const unsigned char (*buf)[components] = (const unsigned char (*)[components])src;
"""
    tu += lines("motion/rotate.c", 159, 164)
    tu += "\t}\n\treturn 0;\n}\n"
    src, so = os.path.join(tmp, "rotate_ref.c"), os.path.join(tmp, "rotate_ref.so")
    with open(src, "w") as f:
        f.write(tu)
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-fPIC", "-shared", "-w", src, "-o", so])
    lib = C.CDLL(so)
    lib.ref_rotate.argtypes = [C.c_char_p] + [C.c_void_p] + [C.c_int] + [C.c_void_p] * 4
    return lib


def main():
    assert os.path.isdir(REF), REF
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        ln = np.array([W, H, FRAMES], dtype=np.uint64)
        n = W * H * FRAMES * COMPONENTS
        vol = (splitmix64_stream(0xD5F3000, n) >> np.uint64(56)).astype(np.uint8)
        names, maps, inverts, outs = spellings(), [], [], []
        assert len(names) == len(set(names)) == 162
        for s in names:
            m, inv = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
            dst = np.full(n, 0xEE, dtype=np.uint8)
            arg = C.create_string_buffer(s.encode())
            assert lib.ref_rotate(arg, ln.ctypes.data, COMPONENTS, vol.ctypes.data, dst.ctypes.data, m.ctypes.data, inv.ctypes.data) == 0, s
            maps.append(m); inverts.append(inv); outs.append(dst)
        for s in REJECTED:
            m, inv = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
            arg = C.create_string_buffer(s.encode())
            assert lib.ref_rotate(arg, ln.ctypes.data, COMPONENTS, None, None, m.ctypes.data, inv.ctypes.data) == 1, s
    path = os.path.join(HERE, "ref_rotate.npz")
    np.savez_compressed(path, size=np.array([W, H, FRAMES, COMPONENTS]), vol=vol.reshape(FRAMES, H, W, COMPONENTS), spellings=np.array(names),
                        map=np.array(maps), invert=np.array(inverts), out=np.array(outs), rejected=np.array(REJECTED))
    print("wrote", path, os.path.getsize(path), len(names), "spellings")


if __name__ == "__main__":
    main()
