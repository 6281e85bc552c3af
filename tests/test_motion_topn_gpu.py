"""motion --coeff-limit per block on the device (motion/motion.c:652-668): the batched selection dspfft_motion_topn_blocks against a stable
argsort, the fused block kernel with its selection stage against the stages composed one by one, the unfused paths (block-major stacks
with DSPFFT_NO_BLOCK=1, a clip of per-frame blocks, one 3-D block, scaled != block) and the f64 restatement tests/motion_ref.py."""
import functools
import math

import numpy as np
import pytest

import motion_ref as mr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
R2 = math.sqrt(2.0)
# The 8-bit ends of the volume test store quantise(value * MUL8).  With integer samples, 4-point transforms and a multiplier of 1 the exact
# results of a block that keeps 2 of its 16 coefficients are multiples of 1/32: 5.8 % of the (1,4,4) case's samples lie ON a half-integer
# (counted on the CPU with the f64 port), where the last bit of either f32 evaluation order decides the byte.  A multiplier that is no
# such fraction leaves none there; the bar then measures the arithmetic and not a coin.
MUL8 = 0.9371
BLOCKS = [(1, 4, 4), (1, 8, 8), (8, 8, 8), (16, 16, 16), (1, 32, 32), (8, 16, 4)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from dspfun_amd import _lib
    _lib.load()
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def topn_rows(rows, keep):
    """the reference rule on every row of a 2-D array: the `keep` largest magnitudes stay, ties to the earliest (stable argsort)"""
    order = np.argsort(-np.abs(rows), axis=1, kind="stable")
    mask = np.zeros(rows.shape, dtype=bool)
    np.put_along_axis(mask, order[:, :keep], True, axis=1)
    return np.where(mask, rows, np.zeros_like(rows))


def motion_scales(fwd, inv, n):
    """motion's uniform range (motion.c:644-647, :748-751) as the plans' scales, and the transforms' 1 / prod(2 n) on the inverse"""
    fwd.set_scale(2 * R2)
    inv.set_scale(1.0 / (2 * R2) / float(np.prod([2.0 * v for v in n])))
    for a in range(len(n)):
        fwd.set_axis_scale0(a, 1.0, 1.0 / R2)
        inv.set_axis_scale0(a, R2, 1.0)
    return fwd, inv


def volume_plans(block, D, H, W):
    from dspfun_amd import Plan
    bd, bh, bw = block
    dims = [d for d in [(bd, H * W, H * W), (bh, W, W), (bw, 1, 1)] if d[0] > 1]
    how = [(D // bd, bd * H * W, bd * H * W), (H // bh, bh * W, bh * W), (W // bw, bw, bw)]
    n = [d[0] for d in dims]
    fwd, inv = motion_scales(Plan.guru(dims, how, [5] * len(n)), Plan.guru(dims, how, [4] * len(n)), n)
    assert "side by side" in fwd.describe() and "BLOCK" in inv.describe()
    return fwd, inv


def stack_plans(block, nb):
    from dspfun_amd import Plan
    n = [v for v in block if v > 1]
    vol = int(np.prod(block))
    return motion_scales(Plan.many_r2r(n, [5] * len(n), howmany=nb, idist=vol, odist=vol),
                         Plan.many_r2r(n, [4] * len(n), howmany=nb, idist=vol, odist=vol, first_axis_first=True), n)


def to_blocks(v, block):
    """[D][H][W] -> [blocks][E], a block's elements in its own z, y, x order"""
    bd, bh, bw = block
    D, H, W = v.shape
    return np.ascontiguousarray(v.reshape(D // bd, bd, H // bh, bh, W // bw, bw).transpose(0, 2, 4, 1, 3, 5)).reshape(-1, bd * bh * bw)


def from_blocks(b, block, shape):
    bd, bh, bw = block
    D, H, W = shape
    return np.ascontiguousarray(b.reshape(D // bd, H // bh, W // bw, bd, bh, bw).transpose(0, 3, 1, 4, 2, 5)).reshape(D, H, W)


def quantise_u8(v, mul=1.0):
    p = v.astype(np.float64) * mul
    return np.clip(np.where(p >= 0, np.floor(p + 0.5), -np.floor(-p + 0.5)), 0, 255).astype(np.uint8)


# ---- 1. the batched selection, exactly ----
NB, GAP = 7, 8


@functools.lru_cache(maxsize=None)
def select_case(count, keep):
    """7 runs of `count` floats, 8 sentinels after each: ties everywhere, a run of equal magnitudes across the threshold, one run all
    zeros, one with keep - 1 non-zeros"""
    c = (ol.synth_f32(99 + count, NB * count) - 0.5).astype(np.float32).reshape(NB, count)
    c[:, ::7] = np.round(c[:, ::7] * 16) / 16
    if 1 < keep < count:
        for b in range(NB):
            order = np.argsort(-np.abs(c[b]), kind="stable")
            run = order[max(0, keep - 3):min(count, keep + 4)]
            c[b, run] = np.abs(c[b, run[0]]) * np.where(run % 2, -1.0, 1.0).astype(np.float32)
    c[5] = 0.0
    nz = max(keep - 1, 0)
    c[6, np.argsort(ol.splitmix64_stream(7 + count, count), kind="stable")[nz:]] = 0.0
    assert np.count_nonzero(c[6]) <= nz
    buf = np.full((NB, count + GAP), 123.5, dtype=np.float32)
    buf[:, :count] = c
    want = buf.copy()
    want[:, :count] = topn_rows(c, keep) if keep else 0.0
    return buf, want


@pytest.mark.parametrize("keep_of", ["1", "count/3", "count-1", "count", "0"])
@pytest.mark.parametrize("count", [16, 64, 512, 1024, 4096, 200_000])
def test_topn_blocks_select_exactly(gpu, count, keep_of):
    """dspfft_motion_topn_blocks == a stable argsort per run: sub-wave, one-wave and multi-chunk runs in LDS (the fused kernel's code), the
    global path at 200 000; the sentinels between the runs survive.  The selection moves no arithmetic: array_equal."""
    from dspfun_amd import engine
    keep = {"1": 1, "count/3": count // 3, "count-1": count - 1, "count": count, "0": 0}[keep_of]
    buf, want = select_case(count, keep)
    d = dev(gpu, buf)
    engine.motion_topn_blocks(d.reshape(-1)[:NB * (count + GAP)], count, keep, stride=count + GAP)
    gpu.cuda.synchronize()
    got = d.cpu().numpy()
    assert np.array_equal(got[:, count:], want[:, count:]), "sentinels"
    assert np.array_equal(got, want), [int((got[b] != want[b]).sum()) for b in range(NB)]
    assert (np.count_nonzero(got[:, :count], axis=1) <= keep).all()


# ---- 2. the fused kernel on the blocks of a volume ----
def near_tie(coeff_blocks, keep):
    m = -np.sort(-np.abs(coeff_blocks.astype(np.float64)), axis=1)
    return (m[:, keep - 1] - m[:, keep]) <= 1e-5 * m[:, 0]


@functools.lru_cache(maxsize=None)
def volume_case(block, u8):
    bd, bh, bw = block
    D, H, W = 2 * bd, 3 * bh, 13 * bw
    n = D * H * W
    return ol.synth_u8(21 + bd + bh, n).reshape(D, H, W) if u8 else (ol.synth_f32(17 + bd + bw, n) - 0.5).astype(np.float32).reshape(D, H, W)


def composed_reference(gpu, fwd, inv, x, block, keep, between=None):
    """fwd.execute on the device, the selection (and `between`, a host filter) per block in numpy on those very coefficients, inv.execute"""
    d = dev(gpu, x.astype(np.float32))
    fwd.execute(d.data_ptr())
    gpu.cuda.synchronize()
    cb = to_blocks(d.cpu().numpy(), block)
    sel = topn_rows(cb, keep)
    if between is not None:
        sel = between(cb, sel)
    d = dev(gpu, from_blocks(sel, block, x.shape))
    inv.execute(d.data_ptr())
    gpu.cuda.synchronize()
    return d.cpu().numpy(), cb


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("block", BLOCKS)
def test_fused_block_topn_on_a_volume(gpu, block, u8):
    """block_roundtrip_topn_kernel (2 x 3 x 13 blocks: the last group of every row of blocks is partial, keep = E / 8) against forward,
    numpy selection, inverse.  Float ends within 1e-5 max|ref|, 8-bit ends +-1 on under 0.5 % of the samples.
    A block whose magnitudes at ranks keep and keep + 1 lie within 1e-5 of its largest may be left out.  This test is stricter than that
    allowance: it leaves out only such blocks that ALSO miss the bar, and at most 2 % of the blocks -- because on this white-noise input
    the criterion itself covers far more than 2 %: measured on the CPU with the f64 port (oracle_lib.r2r_many, same seeds) the blocks
    within 1e-5 max|c| at rank E / 8 are 0 / 0 / 0 / 3.8 / 0 / 1.3 % (float ends, in BLOCKS' order) and 0 / 0 / 1.3 / 66.7 / 12.8 / 7.7 %
    (8-bit ends, where max|c| is the DC, a hundred times the rest).  On the device the fused kernel computes its coefficients
    with the code fwd.execute runs, so no block has been seen to differ.  With a quantiser 0 < coded <= keep * blocks.
    The 8-bit ends store quantise(value * MUL8) and not value * 1: see MUL8 above (exact half-integers in the (1,4,4) case)."""
    bd, bh, bw = block
    E = bd * bh * bw
    keep = E // 8
    x = volume_case(block, u8)
    D, H, W = x.shape
    nb = (D // bd) * (H // bh) * (W // bw)
    fwd, inv = volume_plans(block, D, H, W)
    ref, cb = composed_reference(gpu, fwd, inv, x, block, keep)
    din = dev(gpu, x)
    if u8:
        dout = gpu.zeros_like(din); work = gpu.empty(D * H * W, dtype=gpu.float32, device="cuda:0")
        fwd.roundtrip_u8(inv, din.data_ptr(), dout.data_ptr(), work.data_ptr(), MUL8, coeff_limit=keep)
    else:
        dout = gpu.zeros_like(din)
        fwd.roundtrip(inv, din.data_ptr(), dout.data_ptr(), coeff_limit=keep)
    gpu.cuda.synchronize()
    got = dout.cpu().numpy()
    if u8:
        diff = np.abs(to_blocks(got, block).astype(np.int32) - to_blocks(quantise_u8(ref, MUL8), block).astype(np.int32))
        missed = diff.max(axis=1) > 1
    else:
        diff = np.abs(to_blocks(got, block).astype(np.float64) - to_blocks(ref, block))
        missed = diff.max(axis=1) > 1e-5 * np.abs(ref).max()
    tie = near_tie(cb, keep)
    print(f"block {block} u8={u8}: near ties {tie.mean():.4f}, blocks over the bar {missed.mean():.4f}, max diff {diff.max():.3g}, "
          f"bar {1 if u8 else 1e-5 * np.abs(ref).max():.3g}")
    assert not (missed & ~tie).any(), (int((missed & ~tie).sum()), float(diff.max()))
    assert missed.mean() <= 0.02
    if u8:
        assert (diff[~missed] > 0).mean() < 0.005
    # a quantiser: the selection bounds what can be coded
    flt = dict(active=block, minbuf_hw=(bh, bw), block_depth=bd, band_begin=(0, 0, 0), band_end=block, quantizer=1.0 if u8 else 1e-3)
    coded = gpu.zeros(1, dtype=gpu.int64, device="cuda:0")
    if u8:
        fwd.roundtrip_u8(inv, din.data_ptr(), dout.data_ptr(), work.data_ptr(), 1.0, filter=flt, d_coded=coded.data_ptr(), coeff_limit=keep)
    else:
        fwd.roundtrip(inv, din.data_ptr(), dout.data_ptr(), filter=flt, d_coded=coded.data_ptr(), coeff_limit=keep)
    gpu.cuda.synchronize()
    assert 0 < int(coded.item()) <= keep * nb, (int(coded.item()), keep * nb)


# ---- 3. volume layout = block-major, exactly; fused against unfused ----
@pytest.mark.parametrize("block", BLOCKS)
def test_fused_block_topn_volume_equals_block_major(gpu, block, monkeypatch):
    """the same blocks rearranged block-major give the same bytes and the same coded count; block-major fused against DSPFFT_NO_BLOCK=1
    (forward passes, dspfft_motion_topn_blocks, stand-alone filter, inverse passes): +-1 on under 1e-3 of the samples"""
    monkeypatch.delenv("DSPFFT_NO_BLOCK", raising=False)
    bd, bh, bw = block
    E = bd * bh * bw
    keep = E // 8
    x = volume_case(block, True)
    D, H, W = x.shape
    flt = dict(active=block, minbuf_hw=(bh, bw), block_depth=bd, band_begin=(0, 1, 0), band_end=(bd, bh, bw - 1), damp=0.5, boost=1.25, preserve_dc=1, quantizer=3.0)

    def run(fwd, inv, pix):
        din = dev(gpu, pix); dout = gpu.zeros_like(din); work = gpu.empty(pix.size, dtype=gpu.float32, device="cuda:0")
        coded = gpu.zeros(1, dtype=gpu.int64, device="cuda:0")
        fwd.roundtrip_u8(inv, din.data_ptr(), dout.data_ptr(), work.data_ptr(), 1.0, filter=flt, d_coded=coded.data_ptr(), coeff_limit=keep)
        gpu.cuda.synchronize()
        return dout.cpu().numpy(), int(coded.item())

    vol, vcoded = run(*volume_plans(block, D, H, W), x)
    bm = to_blocks(x, block)
    fb, ib = stack_plans(block, bm.shape[0])
    assert "block-major" in fb.describe()
    fused, fcoded = run(fb, ib, bm)
    assert np.array_equal(from_blocks(fused, block, x.shape), vol) and fcoded == vcoded and 0 < vcoded <= keep * bm.shape[0]
    monkeypatch.setenv("DSPFFT_NO_BLOCK", "1")
    fu, iu = stack_plans(block, bm.shape[0])
    assert "BLOCK" not in fu.describe()
    unfused, ucoded = run(fu, iu, bm)
    d = np.abs(fused.astype(np.int32) - unfused.astype(np.int32))
    print(f"block {block}: fused vs unfused max {d.max()}, share {(d > 0).mean():.2e}, coded {fcoded} / {ucoded}")
    assert d.max() <= 1 and (d > 0).mean() < 1e-3
    assert abs(fcoded - ucoded) <= max(4, ucoded // 10000)


# ---- 4. preserve_dc = dc restores the DC from before the selection ----
def test_fused_block_topn_restores_the_dc_from_before_the_selection(gpu):
    """(8,8,8) blocks with their means moved to 1e-3: the DC is far below the 8th magnitude and the selection drops it; boost = 2 with
    preserve_dc = dc puts back the value from BEFORE the selection (motion.c:650, :734).  A kernel that restored the value it finds after
    the selection -- zero -- would miss by 1e-3 on every sample, a hundred times the bar."""
    block = (8, 8, 8)
    D, H, W = 16, 24, 104
    x = volume_case(block, False)
    xb = to_blocks(x, block)
    x = from_blocks((xb - xb.mean(axis=1, keepdims=True, dtype=np.float64) + 1e-3).astype(np.float32), block, (D, H, W))
    fwd, inv = volume_plans(block, D, H, W)
    flt = dict(active=block, minbuf_hw=(8, 8), block_depth=8, band_begin=(0, 0, 0), band_end=block, boost=2.0, preserve_dc=1)

    def host_filter(cb, sel):
        out = (sel * np.float32(2.0)).astype(np.float32)
        out[:, 0] = cb[:, 0]
        return out

    ref, cb = composed_reference(gpu, fwd, inv, x, block, 8, between=host_filter)
    assert (np.abs(cb[:, 0]) < 0.1 * -np.sort(-np.abs(cb), axis=1)[:, 7]).all() and (np.abs(cb[:, 0]) > 0).all()
    din = dev(gpu, x); dout = gpu.zeros_like(din)
    fwd.roundtrip(inv, din.data_ptr(), dout.data_ptr(), filter=flt, coeff_limit=8)
    gpu.cuda.synchronize()
    err = np.abs(dout.cpu().numpy().astype(np.float64) - ref).max()
    print(f"dc rule: err {err:.3g}, bar {1e-5 * np.abs(ref).max():.3g}")
    assert err <= 1e-5 * np.abs(ref).max()


# ---- 5. against the f64 restatement of the reference ----
def sparse_block(seed, block, keep):
    """8-bit samples whose spectrum has the DC and keep - 1 strong coefficients above a floor of rounding noise: the reference's choice of
    `keep` coefficients then does not hang on the last bits of anybody's arithmetic"""
    n = int(np.prod(block))
    u = ol.splitmix64_stream(seed, 3 * n)
    pos = 1 + np.argsort(u[:n - 1], kind="stable")[:keep - 1]
    c = np.zeros(n)
    c[pos] = (0.4 + 0.6 * (u[n:2 * n][pos] >> np.uint64(11)) * 2.0 ** -53) * np.where(u[2 * n:][pos] & np.uint64(1), -1.0, 1.0)
    y = ol.r2r_many(c, list(block), [ol.REDFT01] * 3)
    y = (y - y.mean()) / y.std()
    return np.clip(np.round(127.5 + 40.0 * y), 0, 255).astype(np.uint8).reshape(block)


def oracle_gap(pix, block, scaled, minbuf, keep):
    """motion_ref.block_roundtrip's coefficients ahead of its selection: (magnitude at rank keep - at rank keep + 1) / the largest"""
    ad, ah, aw = (min(b, s) for b, s in zip(block, scaled))
    c = np.zeros(minbuf, dtype=np.float64)
    c[:block[0], :block[1], :block[2]] = pix[:block[0], :block[1], :block[2]]
    c = ol.r2r_many(c, list(block), [ol.REDFT10] * 3, inembed=list(minbuf), onembed=list(minbuf), impl="port").reshape(minbuf)
    ol.lib().oracle_motion_uniform_f64(c.ctypes.data, ad, ah, aw, minbuf[1], minbuf[2], 1)
    m = -np.sort(-np.abs(c.ravel()))
    return (m[keep - 1] - m[keep]) / m[0]


@pytest.mark.parametrize("block,scaled,keep,seed", [((4, 24, 40), (4, 36, 30), 500, 71)] + [((8, 8, 8), (8, 8, 8), 64, s) for s in (72, 73, 74, 75)])
def test_topn_roundtrip_against_the_f64_reference(gpu, block, scaled, keep, seed):
    """dspfft_execute_roundtrip_u8_topn on ONE block (scaled != block: the count is the whole embedding, 5760 floats, the radix-select path;
    8 x 8 x 8: 512 floats, the LDS path) against motion_ref.block_roundtrip(topn=keep): +-1 on under 2 % of the samples"""
    from dspfun_amd import Plan
    from test_motion_rescale import plans
    minbuf = tuple(max(b, s) for b, s in zip(block, scaled))
    pix = np.zeros(minbuf, dtype=np.uint8)
    pix[:block[0], :block[1], :block[2]] = sparse_block(seed, block, keep)
    gap = oracle_gap(pix, block, scaled, minbuf, keep)
    assert gap > 1e-4, gap
    fwd, inv = plans(Plan, block, scaled, minbuf)
    if block == scaled:         # (same extents: the roundtrip wants the inverse's first pass on the forward's last axis)
        inv = Plan.many_r2r(list(scaled), [4] * 3, inembed=list(minbuf), onembed=list(minbuf), first_axis_first=True).set_scale(1.0 / (2 * R2))
        for a in range(3):
            inv.set_axis_scale0(a, R2, 1.0)
    assert "BLOCK" not in fwd.describe()
    scalefactor, normalization = mr.consts(block, scaled)
    d_pix = dev(gpu, pix); d_out = gpu.zeros_like(d_pix)
    work = gpu.full(minbuf, 3.0, dtype=gpu.float32, device="cuda:0")
    fwd.roundtrip_u8(inv, d_pix.data_ptr(), d_out.data_ptr(), work.data_ptr(), scalefactor * normalization * normalization, coeff_limit=keep)
    gpu.cuda.synchronize()
    want, coeffs, _ = mr.block_roundtrip(pix, block, scaled, minbuf, topn=keep)
    assert np.count_nonzero(coeffs) == keep
    sd, sh, sw = scaled
    diff = np.abs(d_out.cpu().numpy()[:sd, :sh, :sw].astype(int) - want[:sd, :sh, :sw].astype(int))
    print(f"{block} -> {scaled}: rank gap {gap:.3g}, max diff {diff.max()}, share {(diff > 0).mean():.4f}")
    assert diff.max() <= 1 and (diff > 0).mean() < 0.02, (diff.max(), (diff > 0).mean())


# ---- a clip of per-frame blocks (motion's default -b 0x0x1): runs too long for LDS, several to a launch, with the DC rule ----
def clip_plans(h, w, frames):
    from dspfun_amd import Plan
    return motion_scales(Plan.many_r2r([h, w], [5, 5], howmany=frames, idist=h * w, odist=h * w),
                         Plan.many_r2r([h, w], [4, 4], howmany=frames, idist=h * w, odist=h * w, first_axis_first=True), [h, w])


def test_topn_roundtrip_on_a_clip_of_frames(gpu):
    """5 frames of 72 x 96 (6912 coefficients each), keep = 300, boost = 2 with preserve_dc = dc: forward passes, selection, filter, inverse
    passes -- the kernels fwd.execute and inv.execute run, so the composed reference sees the very same coefficients"""
    from dspfun_amd import _lib
    h, w, frames, keep = 72, 96, 5, 300
    x = (ol.synth_f32(31, frames * h * w) - 0.5).astype(np.float32).reshape(frames, h, w)
    fwd, inv = clip_plans(h, w, frames)
    L = _lib.load()
    assert L.dspfft_roundtrip_topn_work_bytes(fwd._h, inv._h) == L.dspfft_motion_topn_blocks_work_bytes(h * w, frames) > 0
    d = dev(gpu, x)
    fwd.execute(d.data_ptr())
    gpu.cuda.synchronize()
    c = d.cpu().numpy().reshape(frames, h * w)
    sel = (topn_rows(c, keep) * np.float32(2.0)).astype(np.float32)
    sel[:, 0] = c[:, 0]
    d = dev(gpu, sel.reshape(frames, h, w))
    inv.execute(d.data_ptr())
    gpu.cuda.synchronize()
    ref = d.cpu().numpy().astype(np.float64)
    flt = dict(active=(1, h, w), minbuf_hw=(h, w), block_depth=1, band_begin=(0, 0, 0), band_end=(1, h, w), boost=2.0, preserve_dc=1)
    din = dev(gpu, x); dout = gpu.zeros_like(din)
    fwd.roundtrip(inv, din.data_ptr(), dout.data_ptr(), filter=flt, coeff_limit=keep)
    gpu.cuda.synchronize()
    err = np.abs(dout.cpu().numpy() - ref).max()
    print(f"clip: err {err:.3g}, bar {1e-5 * np.abs(ref).max():.3g}")
    assert err <= 1e-5 * np.abs(ref).max()


# ---- 6. keep >= count and keep = 0 are the plain entry, byte for byte ----
def test_keep_zero_and_keep_at_the_count_are_the_plain_call(gpu):
    block = (8, 8, 8)
    x = volume_case(block, True)
    D, H, W = x.shape
    flt = dict(active=block, minbuf_hw=(8, 8), block_depth=8, band_begin=(0, 1, 0), band_end=(8, 8, 7), damp=0.5, boost=1.25, preserve_dc=1, quantizer=3.0)
    fwd, inv = volume_plans(block, D, H, W)
    outs = []
    for keep in (None, 0, 512, 513):
        din = dev(gpu, x); dout = gpu.zeros_like(din); work = gpu.empty(x.size, dtype=gpu.float32, device="cuda:0")
        coded = gpu.zeros(1, dtype=gpu.int64, device="cuda:0")
        fwd.roundtrip_u8(inv, din.data_ptr(), dout.data_ptr(), work.data_ptr(), 1.0, filter=flt, d_coded=coded.data_ptr(), **({} if keep is None else dict(coeff_limit=keep)))
        gpu.cuda.synchronize()
        outs.append((dout.cpu().numpy(), int(coded.item())))
    for o, c in outs[1:]:
        assert np.array_equal(o, outs[0][0]) and c == outs[0][1] > 0
    # a clip of frames, float ends, no filter: the fused column roundtrip's bytes
    h, w, frames = 72, 96, 3
    xf = (ol.synth_f32(33, frames * h * w) - 0.5).astype(np.float32).reshape(frames, h, w)
    fwd, inv = clip_plans(h, w, frames)
    outs = []
    for keep in (None, 0, h * w, h * w + 1):
        din = dev(gpu, xf); dout = gpu.zeros_like(din)
        fwd.roundtrip(inv, din.data_ptr(), dout.data_ptr(), **({} if keep is None else dict(coeff_limit=keep)))
        gpu.cuda.synchronize()
        outs.append(dout.cpu().numpy())
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    assert np.abs(outs[0] - xf).max() < 1e-5
