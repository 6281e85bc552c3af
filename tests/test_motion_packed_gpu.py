"""motion on packed 8-bit pixels on the device (block_packed.hip, dspfft_execute_roundtrip_u8_packed).  In the packed kernel every component
block runs the planar kernel's inlined phases, so the oracle needs no tolerance: the bytes equal the planar call (the same plan pair) on each
de-interleaved component with that component's damp / boost / grey_add, and d_coeffs_coded equals the sum of the planar counts.  The planar
call itself is pinned to the reference by the existing tests.  Every packed call writes into a buffer with a marker page on each side."""
import functools
import math

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu
BLOCKS = [(1, 4, 4), (1, 8, 8), (8, 8, 8), (16, 16, 16), (1, 32, 32), (8, 16, 4)]
FMT_OF = {2: "ya8", 3: "rgb24", 4: "rgba"}
PAGE, MARK = 4096, 0xA5
R2 = math.sqrt(2.0)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from dspfun_amd import _lib
    _lib.load()
    return torch


def planar_G(block):
    bd, bh, bw = block
    return max(1, min(256 // bw, 4096 // (bd * bh * bw)))


def next_prime(n):
    p = n + 1
    while any(p % q == 0 for q in range(2, int(p ** 0.5) + 1)):
        p += 1
    return p


def volume_of(block):
    """2 x 2 x P blocks, P the smallest prime above the planar G: the last group of a row of blocks is short"""
    bd, bh, bw = block
    return (2 * bd, 2 * bh, next_prime(planar_G(block)) * bw)


@functools.lru_cache(maxsize=None)
def clip_of(block, comps):
    shape = volume_of(block)
    return ol.synth_u8(0x9AC + comps + 16 * block[0] + block[2], int(np.prod(shape)) * comps).reshape(shape + (comps,))


def settings(block, comps, info, name, fmt=None, boost=None, damp=None, pdc=2):
    """(filter dict for the packed call, dspfft_motion_packed, per-byte planar filter dicts)"""
    from dspfun_amd.engine import motion_packed, PACKED_FORMATS
    fmt = fmt or FMT_OF[comps]
    bd, bh, bw = block
    base = dict(active=block, minbuf_hw=(bh, bw), block_depth=bd, band_begin=(0, 0, 0), band_end=block)
    if name == "none":
        return None, motion_packed(fmt), [None] * comps
    if name == "quant":
        f = dict(base, quantizer=20.0)
        # (-D's default of 0 never acts: the band is the whole block)
        return dict(f, damp=99.0, boost=99.0), motion_packed(fmt), [dict(f, damp=0.0, boost=1.0) for _ in range(comps)]
    boost = boost or [2.0, 1.0, 0.5, 1.5][:comps]
    damp = damp or [0.25, 0.5, 0.0, 0.75][:comps]
    f = dict(base, band_begin=(1 if bd > 1 else 0, 0, 1), band_end=(max(1, bd // 2), bh // 2 + 1, bw // 2 + 1), threshold_lo=2.0, threshold_hi=1e9,
             preserve_dc=pdc, quantizer=12.0)
    p = motion_packed(fmt, boost=boost, damp=damp, dcstop=True, normalization=info["normalization"], scalefactor=info["scalefactor"])
    planes = [dict(f, damp=p.damp[at], boost=p.boost[at], grey_add=p.grey_add[at]) for at in range(comps)]
    for i, at in enumerate(PACKED_FORMATS[fmt]):
        assert planes[at]["boost"] == np.float32(boost[i]) and planes[at]["damp"] == np.float32(damp[i])
    return dict(f, damp=99.0, boost=99.0, grey_add=99.0), p, planes


def framed(torch, n):
    """n output bytes with a marker page on each side"""
    buf = torch.full((n + 2 * PAGE,), MARK, dtype=torch.uint8, device="cuda:0")
    return buf, buf[PAGE:PAGE + n]


def check_frame(buf, n):
    b = buf.cpu().numpy()
    assert (b[:PAGE] == MARK).all() and (b[PAGE + n:] == MARK).all(), "the call wrote outside the clip"


def run_packed(torch, fwd, inv, src, mul, packed, filt=None, keep=0, in_place=False):
    """src: the interleaved clip (numpy, any shape ending in the components).  Returns (bytes, coded)."""
    n = src.size
    buf, out = framed(torch, n)
    d_in = torch.from_numpy(np.ascontiguousarray(src)).to("cuda:0").reshape(-1)
    if in_place:
        out.copy_(d_in)
        d_in = out
    coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    fwd.roundtrip_u8_packed(inv, d_in.data_ptr(), out.data_ptr(), mul, packed, filter=filt, coeff_limit=keep, d_coded=coded.data_ptr(),
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check_frame(buf, n)
    return out.cpu().numpy().reshape(src.shape), int(coded.item())


def run_planes(torch, fwd, inv, src, mul, planes, keep=0):
    """the planar call of the same plan pair on every de-interleaved component.  Returns (interleaved bytes, [coded per component])."""
    want = np.empty_like(src)
    counts = []
    stream = torch.cuda.current_stream().cuda_stream
    for c, filt in enumerate(planes):
        d_in = torch.from_numpy(np.ascontiguousarray(src[..., c])).to("cuda:0")
        d_out = torch.empty_like(d_in)
        work = torch.empty(d_in.numel(), dtype=torch.float32, device="cuda:0")
        coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        if keep:
            fwd.roundtrip_u8_limit(inv, d_in.data_ptr(), d_out.data_ptr(), work.data_ptr(), mul, coeff_limit=keep, filter=filt, d_coded=coded.data_ptr(), stream=stream)
        else:
            fwd.roundtrip_u8(inv, d_in.data_ptr(), d_out.data_ptr(), work.data_ptr(), mul, filter=filt, d_coded=coded.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        want[..., c] = d_out.cpu().numpy()
        counts.append(int(coded.item()))
    return want, counts


def grid_plans(block):
    from dspfun_amd.engine import motion_grid_plans
    fwd, inv, info = motion_grid_plans(volume_of(block), block, block)
    assert f"{planar_G(block)} blocks per workgroup" in fwd.describe() and "side by side" in fwd.describe()
    return fwd, inv, info


CASES = [(b, c) for b in BLOCKS for c in ((2, 3) if b == (16, 16, 16) else (3, 4))] + [((1, 8, 8), 2)]


@pytest.mark.parametrize("name", ["none", "quant", "dc", "grey"])
@pytest.mark.parametrize("block,comps", CASES, ids=["x".join(map(str, b)) + f"-c{c}" for b, c in CASES])
def test_packed_call_equals_the_planar_call_on_every_component(gpu, block, comps, name):
    """no filter; --quant alone; a band with per-component damp and boost, --threshold and preserve_dc = dc / grey through motion_packed"""
    fwd, inv, info = grid_plans(block)
    src = clip_of(block, comps)
    filt, packed, planes = settings(block, comps, info, "full" if name in ("dc", "grey") else name, pdc=1 if name == "dc" else 2)
    got, coded = run_packed(gpu, fwd, inv, src, info["out_mul"], packed, filt)
    want, counts = run_planes(gpu, fwd, inv, src, info["out_mul"], planes)
    assert np.array_equal(got, want), int((got != want).sum())
    assert coded == sum(counts) and (name == "none") == (coded == 0), (coded, counts)
    if name in ("dc", "grey"):
        assert len(set(counts)) > 1          # the components were filtered differently


@pytest.fixture(scope="module")
def rgb888(gpu):
    """(8, 8, 8) rgb24 with the full filter, preserve_dc = dc: the plans, the clip and the plain packed result"""
    block = (8, 8, 8)
    fwd, inv, info = grid_plans(block)
    src = clip_of(block, 3)
    filt, packed, planes = settings(block, 3, info, "full", pdc=1)
    plain = run_packed(gpu, fwd, inv, src, info["out_mul"], packed, filt)
    return dict(block=block, fwd=fwd, inv=inv, info=info, src=src, filt=filt, packed=packed, planes=planes, plain=plain)


def test_coeff_limit_selects_per_component_block(gpu, rgb888):
    r = rgb888
    got, coded = run_packed(gpu, r["fwd"], r["inv"], r["src"], r["info"]["out_mul"], r["packed"], r["filt"], keep=64)
    want, counts = run_planes(gpu, r["fwd"], r["inv"], r["src"], r["info"]["out_mul"], r["planes"], keep=64)
    assert np.array_equal(got, want), int((got != want).sum())
    assert coded == sum(counts) > 0
    assert not np.array_equal(got, r["plain"][0])          # the limit acted


def test_coeff_limit_at_the_blocks_count_is_the_plain_call(gpu, rgb888):
    r = rgb888
    got, coded = run_packed(gpu, r["fwd"], r["inv"], r["src"], r["info"]["out_mul"], r["packed"], r["filt"], keep=512)
    assert np.array_equal(got, r["plain"][0]) and coded == r["plain"][1]


def test_in_place(gpu, rgb888):
    r = rgb888
    got, coded = run_packed(gpu, r["fwd"], r["inv"], r["src"], r["info"]["out_mul"], r["packed"], r["filt"], in_place=True)
    assert np.array_equal(got, r["plain"][0]) and coded == r["plain"][1]


def test_transfer_characteristic_at_both_ends(gpu):
    block = (8, 8, 8)
    fwd, inv, info = grid_plans(block)
    fwd.set_u8_trc("iec61966-2-1")
    inv.set_u8_trc("iec61966-2-1")
    src = clip_of(block, 3)
    filt, packed, planes = settings(block, 3, info, "full")
    got, coded = run_packed(gpu, fwd, inv, src, info["out_mul"], packed, filt)
    want, counts = run_planes(gpu, fwd, inv, src, info["out_mul"], planes)
    assert np.array_equal(got, want), int((got != want).sum())
    assert coded == sum(counts) > 0
    # one end only: the other converts plainly
    inv.set_u8_trc(0)
    got, _ = run_packed(gpu, fwd, inv, src, info["out_mul"], packed, filt)
    want1, _ = run_planes(gpu, fwd, inv, src, info["out_mul"], planes)
    assert np.array_equal(got, want1) and not np.array_equal(want1, want)


def test_bgr24_takes_the_components_values_to_bytes_2_1_0(gpu):
    block = (8, 8, 8)
    fwd, inv, info = grid_plans(block)
    src = clip_of(block, 3)
    boost = [2.0, 1.0, 0.5]
    filt, packed, planes = settings(block, 3, info, "full", fmt="bgr24", boost=boost)
    assert [planes[at]["boost"] for at in (2, 1, 0)] == boost
    got, coded = run_packed(gpu, fwd, inv, src, info["out_mul"], packed, filt)
    want, counts = run_planes(gpu, fwd, inv, src, info["out_mul"], planes)
    assert np.array_equal(got, want) and coded == sum(counts) > 0
    _, _, rgb_planes = settings(block, 3, info, "full", fmt="rgb24", boost=boost)
    assert not np.array_equal(run_planes(gpu, fwd, inv, src, info["out_mul"], rgb_planes)[0], want)


def test_block_major_layout(gpu):
    """a stack of 44 blocks of [8][8][8][3] bytes: rows_fast's order of lines, four pixel blocks per workgroup"""
    from dspfun_amd import Plan
    block, nb = (8, 8, 8), 44
    fwd = Plan.many_r2r([8, 8, 8], [5] * 3, howmany=nb, idist=512, odist=512).set_scale(2 * R2)
    inv = Plan.many_r2r([8, 8, 8], [4] * 3, howmany=nb, idist=512, odist=512, first_axis_first=True).set_scale(1.0 / (2 * R2))
    for a in range(3):
        fwd.set_axis_scale0(a, 1.0, 1.0 / R2)
        inv.set_axis_scale0(a, R2, 1.0)
    assert "block-major" in fwd.describe()
    info = dict(normalization=1.0 / math.sqrt(8.0 * 512), scalefactor=1.0, out_mul=1.0 / (8.0 * 512))
    src = clip_of(block, 3).reshape(nb, 8, 8, 8, 3)
    filt, packed, planes = settings(block, 3, info, "full")
    got, coded = run_packed(gpu, fwd, inv, src, info["out_mul"], packed, filt)
    want, counts = run_planes(gpu, fwd, inv, src, info["out_mul"], planes)
    assert np.array_equal(got, want), int((got != want).sum())
    assert coded == sum(counts) > 0
