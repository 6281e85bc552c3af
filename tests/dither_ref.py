"""TEST-ONLY: motion's dithered 8-bit store (motion/motion.c:756-788 with -d) restated in numpy, and the fixture cases of
tests/golden/ref_dither.npz (geometry, constants, inputs regenerated from recorded seeds).

The restatement walks a plane one anti-diagonal x + 2y at a time (every pixel on one is independent of the others) in float64 with the
reference's operation order: each `+=` into a float coefficient rounds to float32, numpy does not contract into FMAs.  It is byte-identical
to the reference's lines compiled with COEFF_PRECISION=F INTERMEDIATE_PRECISION=D (tests/test_motion_dither_cpu.py)."""
import numpy as np

from oracle_lib import synth_f32

F32, F64 = np.float32, np.float64


def motion_constants(scaled, block):
    """motion.c:562-563 for one component: scalefactor and normalization from the scaled and block extents (d, h, w)"""
    s = scaled[0] * scaled[1] * scaled[2]
    b = block[0] * block[1] * block[2]
    return s / float(b), 1 / np.sqrt(float(s * 8))


def _round_half_away(p):
    r = np.trunc(p)
    return r + np.where(np.abs(p - r) >= 0.5, np.sign(p), 0.0)


def dither_plane(c, scalefactor, norm):
    """one h x w float32 plane -> uint8 (what the reference writes; `c` is not modified)"""
    c = np.asarray(c, dtype=F32)
    h, w = c.shape
    sf, nm = F64(scalefactor), F64(norm)
    k = nm * nm * sf
    tab = np.arange(256, dtype=F64) / k
    dp = np.zeros((h, w), dtype=F64)
    out = np.zeros((h, w), dtype=np.uint8)
    for t in range(w + 2 * (h - 1)):
        y = np.arange(max(0, (t - w + 2) // 2), min(h - 1, t // 2) + 1)
        x = t - 2 * y
        ok = (x >= 0) & (x < w)
        y, x = y[ok], x[ok]
        if y.size == 0:
            continue
        v = c[y, x].copy()
        up = y > 0
        xm, xp = x > 0, x + 1 < w
        ya = np.maximum(y - 1, 0)
        m = up & xm
        v[m] = (v[m].astype(F64) + dp[ya[m], x[m] - 1] / 16).astype(F32)
        v[up] = (v[up].astype(F64) + dp[ya[up], x[up]] * 5 / 16).astype(F32)
        m = up & xp
        v[m] = (v[m].astype(F64) + dp[ya[m], x[m] + 1] * 3 / 16).astype(F32)
        v[xm] = (v[xm].astype(F64) + dp[y[xm], x[xm] - 1] * 7 / 16).astype(F32)
        pel = v.astype(F64) * sf * nm
        pel = pel * nm
        p = np.where(pel > 255, 255.0, np.where(pel < 0, 0.0, _round_half_away(pel))).astype(np.uint8)
        out[y, x] = p
        dp[y, x] = v.astype(F64) - tab[p]
    return out


def dither_planes(c, scalefactor, norm):
    """(..., h, w) -> uint8 of the same shape, plane by plane"""
    c = np.asarray(c, dtype=F32)
    flat = c.reshape(-1, c.shape[-2], c.shape[-1])
    return np.stack([dither_plane(p, scalefactor, norm) for p in flat]).reshape(c.shape)


# ---- fixture cases -------------------------------------------------------------------------------------------------------------------
# name, scaled (d, h, w), minbuf (d, h, w) of one block's buffer, blocks in the stack, scalefactor target (the block extents are chosen for it)
CASES = [
    ("1x1", (1, 1, 1), (1, 1, 1), 1, 1.0),
    ("1x9", (1, 1, 9), (1, 1, 9), 1, 1.0),
    ("9x1", (1, 9, 1), (1, 9, 1), 1, 1.0),
    ("2x2", (1, 2, 2), (1, 2, 2), 1, 1.0),
    ("3x5", (1, 3, 5), (1, 3, 5), 1, 0.5),
    ("17x33p40", (1, 17, 33), (1, 35, 40), 1, 1.0),
    ("64x48x3", (3, 48, 64), (3, 48, 64), 1, 2.25),
    ("127x65", (1, 65, 127), (1, 65, 127), 1, 0.5),
    ("blocks4x8x8x8", (8, 8, 8), (8, 8, 8), 4, 1.0),
    ("960x540", (1, 540, 960), (1, 540, 960), 1, 2.25),
]
SEED0 = 0xD17E0000


def block_for(scaled, sf):
    """block extents with scaled / block volume = sf (2.25: each of h and w scaled by 1.5; 0.5: w halved)"""
    d, h, w = scaled
    if sf == 1.0:
        return (d, h, w)
    if sf == 0.5:
        return (d, h, 2 * w)
    return (d, max(1, round(h / 1.5)), max(1, round(w / 1.5)))


def case_inputs(i):
    """(coeffs float32 (blocks, md, mh, mw), scalefactor, normalization, scaled, minbuf, block) of case i: synth_f32 mapped to pels in
    about [-20, 275] (both clamps), with a plateau of coefficients whose undiffused pel is an exact k + 0.5 where the constants allow it"""
    name, scaled, minbuf, nblocks, sft = CASES[i]
    block = block_for(scaled, sft)
    sf, nm = motion_constants(scaled, block)
    mul = F64(sf) * F64(nm) * F64(nm)
    n = nblocks * minbuf[0] * minbuf[1] * minbuf[2]
    u = synth_f32(SEED0 + i, n).reshape(nblocks, *minbuf).astype(F64)
    c = ((u * 295.0 - 20.0) / mul).astype(F32)
    d, h, w = scaled
    ph, pw = max(1, h // 4), max(1, w // 3)
    k = (np.arange(ph * pw).reshape(ph, pw) % 200).astype(F64) + 20.5
    c[:, :, :ph, :pw] = (k / mul).astype(F32)
    return c, sf, nm, scaled, minbuf, block
