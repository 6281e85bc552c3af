"""TEST INFRASTRUCTURE ONLY: motion --blocksize with --size AND --coeff-limit over a grid of blocks (motion/motion.c:613-800 with :652-668):
volumes whose blocks make the reference's ranking rule visible, and the f64 oracle's result for them, block by block through
tests/motion_ref.py block_roundtrip(topn=keep).  Shared by tests/test_motion_grid_topn_cpu.py, _gpu.py and test_motion_dither_limit_gpu.py.

The rule (include/dspfft.h, dspfft_coeff_limit): the reference multiplies only the A = min(block, scaled) corner by the uniform-range factors
and then ranks the whole M = max(block, scaled) embedding, so a coefficient inside N = block but outside A competes with its RAW value.  A
block with exactly `keep` strong coefficients cannot tell that from "scale everything, then rank"; these blocks can.  Per block, in
uniform-range ("scaled") units with a = 1:
  keep strong coefficients inside A                       magnitudes 1.00 ... 1.10, distinct
  WEAK weak ones inside A                                 0.45 ... 0.55: what any selection drops
  OUTSIDE ones inside N but outside A (where N > A)       scaled magnitude min(2, 0.85 rho) x (0.93 ... 1), rho = scaled / raw at that position
rho is 2 sqrt 2 over sqrt 2 per zero index -- for 2-D blocks the reference's unit z axis is one, always -- and at most one more zero index is
used, so rho is 2 sqrt 2 or 2 for 3-D blocks, 2 or sqrt 2 for 2-D blocks: the raw value the reference ranks is 0.66 ... 0.85, below every
strong one, and the scaled value 1.11 ... 2, above every strong one.  The reference keeps exactly the strong ones; a selection
over scaled values would keep the OUTSIDE ones instead.  With 8-bit pixels the DC (the block's mean, 128) is one of the `keep`."""
import functools
import math

import numpy as np

import motion_grid_ref as gr
import motion_ref as mr
import oracle_lib as ol

# (block, scaled) as (d, h, w) -> (keep, blocks per workgroup G forced through DSPFFT_BLOCK_G).  Seven blocks along x: two full workgroups
# and a ragged one at G = 3, one full and a ragged one at G = 5 (and with two blocks to a wave, 1x4x8, a lane group without a block).
PAIRS = [((8, 8, 8), (4, 4, 4)),           # downscale on every axis
         ((4, 4, 4), (8, 8, 8)),           # upscale on every axis
         ((8, 4, 16), (4, 8, 8)),          # mixed
         ((16, 16, 16), (8, 8, 8)),        # 64 keys per lane
         ((1, 32, 32), (1, 16, 16)),       # 2-D
         ((1, 8, 8), (1, 16, 16)),         # 2-D upscale
         ((1, 4, 8), (1, 4, 4))]           # an embedding of 32: two blocks per wave
KEEP = {PAIRS[0]: 16, PAIRS[1]: 12, PAIRS[2]: 16, PAIRS[3]: 40, PAIRS[4]: 24, PAIRS[5]: 12, PAIRS[6]: 6}
FORCED_G = {PAIRS[0]: 5, PAIRS[1]: 5, PAIRS[2]: 5, PAIRS[3]: 3, PAIRS[4]: 5, PAIRS[5]: 5, PAIRS[6]: 5}
NBLOCKS = (2, 2, 7)
OUTSIDE, WEAK = 8, 6
GAP = 1e-4                   # of the largest magnitude, between rank keep and rank keep + 1 (test_topn_roundtrip_against_the_f64_reference's bar)
PEAK = 100.0                 # pixel amplitude of a block's texture around its mean


def pair_id(p):
    return gr.pair_id(p)


def uniform_factors(block):
    """motion.c:644-647 for every position of a block: 2 sqrt 2, over sqrt 2 per zero index"""
    f = np.full(block, 2 * math.sqrt(2.0))
    for ax in range(3):
        idx = [slice(None)] * 3
        idx[ax] = 0
        f[tuple(idx)] /= math.sqrt(2.0)
    return f


def block_texture(rng, block, scaled, keep, with_dc):
    """one block's pixels minus their mean, from the sparse spectrum described above (amplitude PEAK)"""
    active = tuple(min(b, s) for b, s in zip(block, scaled))
    f = uniform_factors(block)
    inside = np.zeros(block, dtype=bool)
    inside[:active[0], :active[1], :active[2]] = True
    zeros = sum((np.indices(block)[ax] == 0).astype(int) for ax in range(3)) - (1 if block[0] == 1 else 0)     # zero indices among the real axes
    pos_in = [p for p in zip(*np.nonzero(inside)) if p != (0, 0, 0)]
    pos_out = [p for p in zip(*np.nonzero(~inside & (zeros <= 1)))]
    strong = keep - (1 if with_dc else 0)
    weak = min(WEAK, len(pos_in) - strong)
    nout = min(OUTSIDE, len(pos_out))
    assert strong >= 1 and weak >= 1 and len(pos_in) >= strong + weak
    pick = rng.permutation(len(pos_in))[:strong + weak]
    c = np.zeros(block)                                       # uniform-range units
    mags = 1.0 + 0.1 * rng.permutation(strong) / max(1, strong - 1) if strong > 1 else np.ones(1)
    for k, i in enumerate(pick):
        m = mags[k] if k < strong else 0.45 + 0.1 * rng.random()
        c[pos_in[i]] = m * rng.choice((-1.0, 1.0))
    for i in rng.permutation(len(pos_out))[:nout]:
        p = pos_out[i]
        rho = f[p]                                            # scaled over raw, the value the reference ranks there
        c[p] = min(2.0, 0.85 * rho) * (0.93 + 0.07 * rng.random()) * rng.choice((-1.0, 1.0))
    raw = c / f
    x = ol.r2r_many(raw, list(block), [ol.REDFT01] * 3, impl="port").reshape(block) / float(np.prod([2 * n for n in block]))
    return x * (PEAK / np.abs(x).max())


def oracle_block(pix, block, scaled, keep, between=None):
    """one block through the reference: (8-bit output [scaled], f64 pixels before rounding [scaled], coefficients before the selection
    [minbuf], after it [minbuf]).  between(after, dc): a filter on the selected coefficients, in place (dc: element 0 before the selection)"""
    minbuf = tuple(max(b, s) for b, s in zip(block, scaled))
    ad, ah, aw = (min(b, s) for b, s in zip(block, scaled))
    sd, sh, sw = scaled
    sf, nm = mr.consts(block, scaled)
    emb = np.zeros(minbuf, dtype=pix.dtype)
    emb[:block[0], :block[1], :block[2]] = pix
    _, before, _ = mr.block_roundtrip(emb, block, scaled, minbuf)
    o, after, _ = mr.block_roundtrip(emb, block, scaled, minbuf, topn=keep)
    c = after.copy()
    if between is not None:
        between(c, before[0, 0, 0])
    ol.lib().oracle_motion_uniform_f64(c.ctypes.data, ad, ah, aw, minbuf[1], minbuf[2], -1)
    c = ol.r2r_many(c, list(scaled), [ol.REDFT01] * 3, inembed=list(minbuf), onembed=list(minbuf), impl="port").reshape(minbuf)
    return o[:sd, :sh, :sw], c[:sd, :sh, :sw] * sf * nm * nm, before, after


def rule_check(before, block, scaled, keep):
    """(the oracle's gap between rank keep and rank keep + 1 over the largest magnitude, whether a selection over scaled values everywhere
    would keep another set than the reference's).  `before`: the embedding ahead of the selection, the A corner in uniform range."""
    bd, bh, bw = block
    ad, ah, aw = (min(b, s) for b, s in zip(block, scaled))
    mag = np.sort(np.abs(before).ravel())[::-1]
    gap = (mag[keep - 1] - mag[keep]) / mag[0]
    everything = before.copy()
    everything[:bd, :bh, :bw] *= uniform_factors(block)
    everything[:ad, :ah, :aw] = before[:ad, :ah, :aw]
    kept = lambda a: set(np.argsort(-np.abs(a).ravel(), kind="stable")[:keep].tolist())
    return float(gap), kept(before) != kept(everything)


@functools.lru_cache(maxsize=None)
def case(block, scaled, u8=True, mean=None, boost_dc=False, seed0=500):
    """a seeded volume of NBLOCKS such blocks and the oracle's result, computed once per session.  u8: 8-bit pixels around 128 (the DC is one
    of the kept), else float32 pixels around `mean` (default 128).  boost_dc: the oracle applies boost = 2 over A with preserve_dc = dc
    (motion.c:730-735).  The seed is the first from seed0 on whose every block keeps the oracle's rank gap above GAP; `gap` is the smallest
    gap of the chosen volume and `differs` whether, in every block with N > A, scale-everything would keep another set (the tests assert both)."""
    keep = KEEP[(block, scaled)]
    mean = 128.0 if mean is None else mean
    nb = int(np.prod(NBLOCKS))
    has_outside = any(b > s for b, s in zip(block, scaled))

    def boost(c, dc):
        ad, ah, aw = (min(b, s) for b, s in zip(block, scaled))
        c[:ad, :ah, :aw] *= 2.0
        c[0, 0, 0] = dc

    for seed in range(seed0, seed0 + 50):
        rng = np.random.default_rng(seed)
        stack = np.stack([block_texture(rng, block, scaled, keep, with_dc=abs(mean) > 1.0) + mean for _ in range(nb)])
        stack = np.clip(np.round(stack), 0, 255).astype(np.uint8) if u8 else stack.astype(np.float32)
        res = [oracle_block(b, block, scaled, keep, boost if boost_dc else None) for b in stack]
        checks = [rule_check(r[2], block, scaled, keep) for r in res]
        gap = min(g for g, _ in checks)
        if gap <= GAP:
            continue
        out8 = gr.from_blocks(np.stack([r[0] for r in res]), scaled, NBLOCKS)
        pel = gr.from_blocks(np.stack([r[1] for r in res]), scaled, NBLOCKS)
        vol = gr.from_blocks(stack, block, NBLOCKS)
        dc_kept = all(r[3][0, 0, 0] != 0.0 for r in res)
        dc_before = np.array([r[2][0, 0, 0] for r in res])
        for a in (vol, out8, pel):
            a.setflags(write=False)
        return dict(vol=vol, out8=out8, pel=pel, keep=keep, gap=gap, differs=all(d for _, d in checks) if has_outside else None,
                    dc_kept=dc_kept, dc_before=dc_before, seed=seed, G=FORCED_G[(block, scaled)])
    raise AssertionError("no seed keeps the oracle's rank gap")
