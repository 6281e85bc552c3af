"""rotate (motion/rotate.c:74-89, 159-164) restated in numpy, the cases the rotate tests share, and the fixture compiled from the
reference's own lines (tests/golden/ref_rotate.npz, written by tests/golden/make_rotate_fixtures.py)."""
import functools
import itertools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# (w, h, frames) around the tiles: 128 bytes at one-byte elements, 64 elements otherwise -- one over one, two and four tile widths of either
# (65 / 130 / 257 and 129 / 258 / 513 at one byte), single-element axes, and a clip smaller than any tile
VOLUMES = [(65, 33, 17), (130, 67, 5), (1, 64, 9), (64, 1, 9), (9, 64, 1), (257, 3, 66), (7, 5, 3)]
VOLUMES_E1 = [(129, 33, 17), (258, 67, 5), (1, 64, 9), (64, 1, 9), (9, 64, 1), (513, 3, 130), (7, 5, 3)]


def volumes(E):
    return VOLUMES_E1 if E == 1 else VOLUMES


def maps48():
    """the 48 (order, sign) spellings: 6 orders x a '-' or nothing before each letter"""
    return ["".join(s + l for s, l in zip(signs, order)) for order in itertools.permutations("xyz") for signs in itertools.product(("", "-"), repeat=3)]


def parse(spec):
    """rotate.c:74-89, for specs that hold three letters of xyz with optional signs"""
    m, inv, i = [], [0, 0, 0], 0
    for p in range(3):
        if spec[i] in "+-":
            inv[p] = int(spec[i] == "-")
            i += 1
        m.append("xyz".index(spec[i]))
        i += 1
    return tuple(m), tuple(inv)


def rotate(vol, m, inv):
    """vol[z][y][x][c]: flip numpy axis 2 - a for every input axis a with invert[map[a]], then output axis o runs over input axis map[o]"""
    v = vol
    for a in range(3):
        if inv[m[a]]:
            v = np.flip(v, axis=2 - a)
    return np.ascontiguousarray(v.transpose(2 - m[2], 2 - m[1], 2 - m[0], 3))


def inverse_spec(m, inv):
    """the spelling that undoes (map, invert): output axis p of the first call is input axis p of the second, which reads it backwards iff
    the first call flipped its input axis map[p]"""
    letters, signs = [None] * 3, [None] * 3
    for p in range(3):
        letters[m[p]] = "xyz"[p]          # the second call's output axis map[p] runs over its input axis p
    m2 = tuple("xyz".index(l) for l in letters)
    # the second call flips its input axis a iff invert2[m2[a]]; it must flip axis p iff the first flipped map[p], i.e. iff inv[m[m[p]]]
    inv2 = [0, 0, 0]
    for p in range(3):
        inv2[m2[p]] = inv[m[m[p]]]
    return "".join(("-" if inv2[p] else "") + letters[p] for p in range(3))


def pattern(seed, n, avoid=None):
    """n random bytes, none of them zero (nor `avoid`)"""
    rng = np.random.default_rng(seed)
    b = rng.integers(1, 256, size=n, dtype=np.uint16).astype(np.uint8)
    if avoid is not None:
        b[b == avoid] = 1
    return b


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(HERE, "golden", "ref_rotate.npz"))
    return {k: z[k] for k in z.files}
