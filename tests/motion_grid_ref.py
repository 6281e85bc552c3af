"""TEST INFRASTRUCTURE ONLY: motion --blocksize with --size over a whole grid of blocks (motion/motion.c:488-499,613-800), block by block
through the f64 restatement of one block (tests/motion_ref.py).  Shared by tests/test_motion_block_rescale_cpu.py and _gpu.py."""
import functools

import numpy as np

import motion_ref as mr
import oracle_lib as ol

# (block, scaled) as (d, h, w): down, up, mixed, per-axis permutations of 4 / 8 / 16, 2-D with 16 and 32
PAIRS = [((8, 8, 8), (4, 4, 4)),
         ((4, 4, 4), (8, 8, 8)),
         ((8, 8, 8), (4, 16, 8)),
         ((16, 4, 8), (8, 8, 16)),
         ((4, 16, 16), (16, 16, 4)),
         ((1, 8, 8), (1, 16, 16)),
         ((1, 32, 8), (1, 16, 32))]
NBLOCKS = (2, 2, 9)          # in z, y, x: nine blocks along x, so a workgroup's last group is short
EDGE = 1e-4                  # how close coefficient / quantizer may come to a rounding boundary (k + 1/2) in the quantiser tests


def pair_id(p):
    return "x".join(map(str, p[0])) + "-" + "x".join(map(str, p[1]))


def shapes(block, scaled, nblocks=NBLOCKS):
    return tuple(n * b for n, b in zip(nblocks, block)), tuple(n * s for n, s in zip(nblocks, scaled))


def to_blocks(vol, ext):
    """[D][H][W] -> block-major [nd * nh * nw][d][h][w]"""
    d, h, w = ext
    D, H, W = vol.shape
    return np.ascontiguousarray(vol.reshape(D // d, d, H // h, h, W // w, w).transpose(0, 2, 4, 1, 3, 5)).reshape(-1, d, h, w)


def from_blocks(stack, ext, nblocks=NBLOCKS):
    d, h, w = ext
    nd, nh, nw = nblocks
    return np.ascontiguousarray(stack.reshape(nd, nh, nw, d, h, w).transpose(0, 3, 1, 4, 2, 5)).reshape(nd * d, nh * h, nw * w)


def quantizer_of(quant, scaled):
    return quant * 8 * np.sqrt(float(np.prod(scaled)))           # motion.c:570


def oracle(vol_u8, block, scaled, quant=0.0):
    """the reference's result for every block of the grid.  Returns (8-bit output volume, its f64 pixels before clamp and rounding, the
    uniform-range coefficients of every block's active corner after the filters [nb][ad][ah][aw])"""
    minbuf = tuple(max(b, s) for b, s in zip(block, scaled))
    ad, ah, aw = (min(b, s) for b, s in zip(block, scaled))
    sd, sh, sw = scaled
    scalefactor, normalization = mr.consts(block, scaled)
    blocks = to_blocks(vol_u8, block)
    out8 = np.zeros((len(blocks),) + tuple(scaled), dtype=np.uint8)
    pel = np.zeros((len(blocks),) + tuple(scaled), dtype=np.float64)
    act = np.zeros((len(blocks), ad, ah, aw), dtype=np.float64)
    for b, blk in enumerate(blocks):
        pix = np.zeros(minbuf, dtype=np.uint8)
        pix[:block[0], :block[1], :block[2]] = blk
        o, coeffs, _ = mr.block_roundtrip(pix, block, scaled, minbuf, quant=quant)
        out8[b] = o[:sd, :sh, :sw]
        act[b] = coeffs[:ad, :ah, :aw]
        c = coeffs.copy()                                       # motion.c:748-753,759 once more, for the pixels before :776 rounds them
        ol.lib().oracle_motion_uniform_f64(c.ctypes.data, ad, ah, aw, minbuf[1], minbuf[2], -1)
        c = ol.r2r_many(c, list(scaled), [ol.REDFT01] * 3, inembed=list(minbuf), onembed=list(minbuf), impl="port").reshape(minbuf)
        pel[b] = c[:sd, :sh, :sw] * scalefactor * normalization * normalization
    nblocks = tuple(v // b for v, b in zip(vol_u8.shape, block))
    return from_blocks(out8, scaled, nblocks), from_blocks(pel, scaled, nblocks), act


@functools.lru_cache(maxsize=None)
def case(block, scaled, quant=0.0, seed0=100):
    """a seeded 8-bit volume of NBLOCKS blocks and its oracle result, computed once per session.  With a quantiser the seed is the first
    from seed0 on for which no coefficient of the unquantised oracle comes within EDGE of a rounding boundary of coefficient / quantizer;
    `edge` is the distance the chosen volume keeps (the tests assert it)."""
    in_shape, _ = shapes(block, scaled)
    n = int(np.prod(in_shape))
    for seed in range(seed0, seed0 + 200):
        vol = ol.synth_u8(seed, n).reshape(in_shape)
        edge, nonzero = None, None
        if quant:
            _, _, act0 = oracle(vol, block, scaled, 0.0)
            t = act0 / quantizer_of(quant, scaled)
            edge = float(np.abs(np.abs(t - np.floor(t)) - 0.5).min())
            if edge <= EDGE:
                continue
            nonzero = int(np.count_nonzero(np.round(t)))
        out8, pel, act = oracle(vol, block, scaled, quant)
        for a in (vol, out8, pel, act):
            a.setflags(write=False)
        return dict(vol=vol, out8=out8, pel=pel, act=act, edge=edge, nonzero=nonzero, seed=seed)
    raise AssertionError("no seed keeps the coefficients off the quantiser's rounding boundaries")
