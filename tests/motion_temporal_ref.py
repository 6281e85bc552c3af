"""TEST INFRASTRUCTURE ONLY: motion --blocksize 1x1xD --size 1x1xD' over a [frames][H][W] plane (motion/motion.c:488-499,613-800 with
block = {D, 1, 1}, scaled = {D', 1, 1}), every pixel column of every block through the f64 oracle.  Shared by
tests/test_motion_temporal_cpu.py and _gpu.py.

The transforms are the oracle's (oracle/dct_oracle.c through oracle_lib.r2r_many, all columns in one call); the uniform range is
oracle_motion_uniform_f64's line for (z, 0, 0); the filter is a numpy restatement of motion.c:683-744 for z-only positions (`filt`), which
tests/test_motion_temporal_cpu.py pins to oracle_motion_filter_f32 on float32 inputs and, for the plain and quantised cases, the whole
chain to motion_ref.block_roundtrip on (D, 1, 1) blocks."""
import functools

import numpy as np

import motion_grid_ref as gr
import motion_ref as mr
import oracle_lib as ol

H, W = 6, 50                 # P = 300: the last tile is short at every tile width, five tiles at K = 64
P = H * W
NBLOCKS = 3                  # the clip has 3 D + 1 frames: three blocks in time, one frame cropped
EQUAL = [(8, 8), (25, 25), (60, 60), (256, 256)]
RESCALED = [(8, 16), (16, 8), (24, 30), (64, 32)]
PAIRS = EQUAL + RESCALED
KINDS = ["plain", "band", "thr", "dc", "grey", "quant"]
# The float tolerance, in pixels, between the float32 pipeline and the f64 oracle.  Every value of the chain is at most a few times 255 in
# the pixel's scale, and a float operation rounds by 2^-24 of its result.  A transform of N points is about log2 N + 3 roundings deep
# (stages, twiddles, the two-for-one split, the quarter-sample twiddle, the scales): 11 each way for the longest length here, 256, so about
# 25 roundings with the filter and the store's product.  Errors of independent roundings add as a random walk: 255 x 2^-24 x sqrt(25) =
# 7.6e-5 for a typical pixel.  The tests take the maximum over 10^5 to 10^6 pixels, some four to five standard deviations of a value that
# is itself a sum of D' terms; 2^-12 = 2.44e-4 of a pixel is 3.2 times that typical error and the bound the fused spectrogram stores
# already use for a single-precision pixel (motion_filter.h: B).  A pixel closer than that to k + 1/2 may round either way.
TOL = 2.0 ** -12
EDGE_REL = 1e-4              # how close |coefficient| may come to the threshold of the "thr" filter, relative to it


def pair_id(p):
    return f"{p[0]}-{p[1]}"


def filter_dict(kind, D, S):
    """the filter of one test case as dspfft_motion_filter_params' fields (float parameters rounded to float32, as the C ABI takes them),
    or None.  Bands are (z0, 0, 0) to (z1, 1, 1); threshold, grey and quantiser constants as motion.c:566-572,736 derives them from
    scaled = (D', 1, 1)."""
    if kind == "plain":
        return None
    A = min(D, S)
    f = dict(active=(A, 1, 1), minbuf_hw=(1, 1), block_depth=max(D, S), band_begin=(0, 0, 0), band_end=(A, 1, 1), damp=1.0, boost=1.0,
             threshold_lo=0.0, threshold_hi=0.0, preserve_dc=0, grey_add=0.0, quantizer=0.0)
    whd8 = 8.0 * S
    if kind == "band":
        f.update(band_begin=(1, 0, 0), band_end=(max(2, A // 2), 1, 1), damp=0.5, boost=1.5)
    elif kind == "band-pi":
        # the same band with factors that are no dyadic numbers: up to 5 frames a damp of 1 / 2 and a boost of 3 / 2 put a tenth to 40 %
        # of the pixels of integer samples exactly on k + 1/2 (D = 2: (a + b) / 4 +- 3 (a - b) / 4), where the 8-bit rule asks nothing
        f.update(band_begin=(1, 0, 0), band_end=(max(2, A // 2), 1, 1), damp=float(np.float32(1 / np.pi)), boost=float(np.float32(np.pi / 2)))
    elif kind == "thr":
        # A coefficient of 8-bit noise has a standard deviation of 592 sqrt D (74 sqrt(2 D) x 4 sqrt 2).  The threshold drops the smallest
        # 1.6 % of them; it sits where few coefficients are, so that a seed exists whose clip keeps all 900 min(D, D') of them EDGE_REL off it
        f.update(threshold_lo=float(np.float32(12.0 * np.sqrt(D))), threshold_hi=float(np.float32(1e9)))
    elif kind in ("dc", "grey"):
        # (a damp of 1 / 2 on the DC of 8 or 16 integers would put one pixel in 16 or 32 exactly on k + 1/2: no dyadic factor)
        damp = float(np.float32(1 / np.pi))
        f.update(band_begin=(1, 0, 0), band_end=(max(2, A // 2), 1, 1), damp=damp, preserve_dc=1 if kind == "dc" else 2)
        if kind == "grey":
            f.update(grey_add=float(np.float32((1 - damp) * 127.5 * whd8)))
    elif kind == "quant":
        # coefficient / quantizer has a standard deviation of 74 sqrt(D / D') / quant.  Up to 16 active rows the quantiser is fine (pi: a dyadic one
        # would tie with the DCs of integer samples, which are multiples of 4; every
        # coefficient is coded; 7200 or 14400 of them leave seeds that keep all of them EDGE off a rounding boundary).  Beyond, no clip of
        # noise could keep 20000 to 230000 fine-quantised coefficients off every boundary, so the quantiser is coarse: 0.15 standard
        # deviations a step, the DCs and about one coefficient in a thousand are coded and few come near +-1/2
        quant = np.pi if A <= 16 else 74.0 * np.sqrt(D / S) / 0.15
        f.update(quantizer=float(np.float32(gr.quantizer_of(quant, (S, 1, 1)))))
    else:
        raise ValueError(kind)
    return f


def filt(c, f, dtype=np.float64):
    """motion.c:683-744 at positions (z, 0, 0) on c[..., z] (z < active depth), every operation in `dtype`: float64 for the oracle, float32
    to compare with oracle_motion_filter_f32.  Returns (filtered, coded count)."""
    c = np.array(c, dtype=dtype)
    A = f["active"][0]
    z = np.arange(c.shape[-1])
    act = z < A
    b0, b1 = f["band_begin"], f["band_end"]
    inside = act & (z >= b0[0]) & (z < b1[0]) & (0 >= b0[1]) & (0 < b1[1]) & (0 >= b0[2]) & (0 < b1[2])
    damp, boost = dtype(f["damp"]), dtype(f["boost"])
    dc = c[..., 0].copy()
    if damp != 1:
        c[..., act & ~inside] *= damp                          # :683-714
    if boost != 1:
        c[..., inside] *= boost                                # :715-719
    lo, hi = dtype(f["threshold_lo"]), dtype(f["threshold_hi"])
    if hi > 0:                                                 # :721-728
        a = np.abs(c[..., :A])
        c[..., :A][(a < lo) | (a > hi)] = 0
    if f["preserve_dc"]:                                       # :730-738
        dcstop = any(b0)
        if dcstop or boost != 1 or hi > 0:
            if f["preserve_dc"] == 1:
                c[..., 0] = dc
            else:
                c[..., 0] += dtype(f["grey_add"])
    coded = 0
    q = dtype(f["quantizer"])
    if q > 0:                                                  # :740-744
        t = c[..., :A] / q
        r = np.where(t >= 0, np.floor(t + dtype(0.5)), -np.floor(-t + dtype(0.5)))    # round(): halves away from zero
        c[..., :A] = r * q
        coded = int(np.count_nonzero(c[..., :A]))
    return c, coded


def columns(vol, D):
    """[frames][H][W] -> [nd * P][D]: the 1-D blocks, leftover frames cropped"""
    nd = vol.shape[0] // D
    return np.ascontiguousarray(vol[:nd * D].reshape(nd, D, -1).transpose(0, 2, 1)).reshape(-1, D), nd


def forward(vol, D, S, impl="direct"):
    """uniform-range coefficients of the active corner, [nd * P][min(D, S)] float64 (motion.c:617-647).  impl: the oracle library's
    transform -- the direct O(N^2) sum, or "port" (pinned to it in tests/test_oracle.py) for the lengths the direct sum takes too long at"""
    cols, nd = columns(vol.astype(np.float64), D)
    n = len(cols)
    # REDFT10 over D; each of the two unit axes of the reference's 3-D plan doubles (REDFT10 of one sample)
    c = ol.r2r_many(cols, [D], [ol.REDFT10], howmany=n, idist=D, odist=D, impl=impl).reshape(n, D) * 4.0
    A = min(D, S)
    r2 = np.sqrt(2.0)
    s = np.full(A, 2 * r2 / (r2 * r2))                         # oracle_motion_uniform_f64 at (z, 0, 0)
    s[0] = 2 * r2 / (r2 * r2 * r2)
    return c[:, :A] * s, s, nd


def oracle(vol, D, S, f=None, impl="direct"):
    """the reference's result for every pixel column of every block.  Returns (8-bit output clip [nd * S][H][W], its f64 pixels before
    clamp and rounding, the active coefficients after the filter [nd * P][min(D, S)], the coded count)"""
    act, s, nd = forward(vol, D, S, impl)
    coded = 0
    if f is not None:
        act, coded = filt(act, f)
    n, A = act.shape
    c = np.zeros((n, S))                                       # :619 zero padding / truncation to `scaled`
    c[:, :A] = act / s                                         # :748-751
    c = ol.r2r_many(c, [S], [ol.REDFT01], howmany=n, idist=S, odist=S, impl=impl).reshape(n, S)      # :753 (REDFT01 of one sample: itself)
    scalefactor, normalization = mr.consts((D, 1, 1), (S, 1, 1))
    pel = c * scalefactor * normalization * normalization     # :759
    pel = np.ascontiguousarray(pel.reshape(nd, -1, S).transpose(0, 2, 1)).reshape((nd * S,) + vol.shape[1:])
    r = np.where(pel >= 0, np.floor(pel + 0.5), -np.floor(-pel + 0.5))                                    # :776
    return np.clip(r, 0, 255).astype(np.uint8), pel, act, coded


@functools.lru_cache(maxsize=None)
def case(D, S, kind="plain", seed0=300, hw=None, nblocks=None, impl="direct"):
    """a seeded 8-bit clip of 3 D + 1 frames of H x W pixels (hw, nblocks: of nblocks D + 1 frames of hw pixels) and its oracle result
    (impl: see forward), computed once per session.  With a quantiser the seed is
    the first from seed0 on for which no unquantised coefficient / quantizer comes within motion_grid_ref.EDGE of a rounding boundary;
    with a threshold, the first for which no |coefficient| comes within EDGE_REL of it relatively.  `edge` is the distance kept."""
    f = filter_dict(kind, D, S)
    shape = ((NBLOCKS if nblocks is None else nblocks) * D + 1,) + ((H, W) if hw is None else tuple(hw))
    for seed in range(seed0, seed0 + 400):
        vol = ol.synth_u8(seed, int(np.prod(shape))).reshape(shape)
        edge = None
        if kind == "quant":
            t = forward(vol, D, S, impl)[0] / f["quantizer"]
            edge = float(np.abs(np.abs(t - np.floor(t)) - 0.5).min())
            if edge <= gr.EDGE:
                continue
        elif kind == "thr":
            a = np.abs(forward(vol, D, S, impl)[0])
            edge = float(np.abs(a / f["threshold_lo"] - 1).min())
            if edge <= EDGE_REL:
                continue
        out8, pel, act, coded = oracle(vol, D, S, f, impl)
        for a in (vol, out8, pel, act):
            a.setflags(write=False)
        return dict(vol=vol, out8=out8, pel=pel, act=act, coded=coded, edge=edge, seed=seed, filter=f)
    raise AssertionError("no seed keeps the coefficients off the rounding boundaries")


def near_half(pel, tol=TOL):
    """pixels whose oracle value lies within tol of k + 1/2 (inside the range where rounding decides the byte)"""
    frac = pel - np.floor(pel)
    return (np.abs(frac - 0.5) <= tol) & (pel > -1) & (pel < 256)


def check_bytes(got, ref, tol=TOL):
    """the 8-bit rule of the issue: equal wherever the oracle's pixel is farther than `tol` from k + 1/2, within 1 elsewhere"""
    near = near_half(ref["pel"], tol)
    diff = np.abs(got.astype(int) - ref["out8"].astype(int))
    assert diff[~near].max() == 0, (int((diff[~near] > 0).sum()), int(diff.max()))
    assert diff.max() <= 1
    return float(near.mean())
