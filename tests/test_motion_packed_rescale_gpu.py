"""motion -b with -s over a block grid on packed 8-bit pixels on the device (block_rescale_packed.hip, dspfft_execute_roundtrip_u8_packed_rescale).
The packed kernel runs the planar grid kernel's inlined line functions per component, so the first oracle needs no tolerance: the bytes equal
the planar grid call (Plan.roundtrip_u8 on the same pair) on each de-interleaved component with that component's damp / boost / grey_add, and
d_coeffs_coded equals the sum of the planar counts.  The planar grid call itself is pinned to the f64 reference by
test_motion_block_rescale_gpu.py; the last test holds the packed call to that reference directly, with that file's caps.  Every packed call
writes into a buffer with a marker page on each side."""
import functools

import numpy as np
import pytest

import motion_grid_ref as gr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
IDS = [gr.pair_id(p) for p in gr.PAIRS]
FMT_OF = {2: "ya8", 3: "rgb24", 4: "rgba"}
PAGE, MARK = 4096, 0xA5


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from dspfun_amd import _lib
    _lib.load()
    return torch


def grid_plans(block, scaled):
    from dspfun_amd.engine import motion_grid_plans
    return motion_grid_plans(gr.shapes(block, scaled)[0], block, scaled)


@functools.lru_cache(maxsize=None)
def clip_of(block, comps):
    shape = gr.shapes(block, block)[0]
    c = ol.synth_u8(0x5CA + comps + 16 * block[0] + block[2], int(np.prod(shape)) * comps).reshape(shape + (comps,))
    c.setflags(write=False)
    return c


def settings(block, scaled, comps, info, name, fmt=None, boost=None, damp=None, pdc=2):
    """(filter dict for the packed call, dspfft_motion_packed, per-byte planar filter dicts); the filter is the planar grid's: active from
    info, minbuf_hw and block_depth of the embedding"""
    from dspfun_amd.engine import motion_packed, PACKED_FORMATS
    fmt = fmt or FMT_OF[comps]
    minbuf = [max(b, s) for b, s in zip(block, scaled)]
    ad, ah, aw = info["active"]
    base = dict(active=info["active"], minbuf_hw=minbuf[1:], block_depth=minbuf[0], band_begin=(0, 0, 0), band_end=info["active"])
    if name == "none":
        return None, motion_packed(fmt), [None] * comps
    if name == "quant":
        f = dict(base, quantizer=20.0)
        # (-D's default of 0 never acts: the band is the whole active corner)
        return dict(f, damp=99.0, boost=99.0), motion_packed(fmt), [dict(f, damp=0.0, boost=1.0) for _ in range(comps)]
    boost = boost or [2.0, 1.0, 0.5, 1.5][:comps]
    damp = damp or [0.25, 0.5, 0.0, 0.75][:comps]
    f = dict(base, band_begin=(1 if ad > 1 else 0, 0, 1), band_end=(max(1, ad // 2), ah // 2 + 1, aw // 2 + 1), threshold_lo=2.0, threshold_hi=1e9,
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


def run_packed(torch, fwd, inv, src, out_shape, mul, packed, filt=None):
    """src: the interleaved input clip (numpy, the last axis the components); out_shape: the output clip's, components included.
    Returns (bytes, coded)."""
    n = int(np.prod(out_shape))
    buf, out = framed(torch, n)
    d_in = torch.from_numpy(np.array(src)).to("cuda:0").reshape(-1)
    coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    fwd.roundtrip_u8_packed_rescale(inv, d_in.data_ptr(), out.data_ptr(), mul, packed, filter=filt, d_coded=coded.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check_frame(buf, n)
    return out.cpu().numpy().reshape(out_shape), int(coded.item())


def run_planes(torch, fwd, inv, src, out_shape, mul, planes):
    """the planar grid call of the same plan pair on every de-interleaved component.  Returns (interleaved bytes, [coded per component])."""
    want = np.empty(out_shape, dtype=np.uint8)
    counts = []
    stream = torch.cuda.current_stream().cuda_stream
    for c, filt in enumerate(planes):
        d_in = torch.from_numpy(np.array(src[..., c])).to("cuda:0")
        d_out = torch.zeros(out_shape[:-1], dtype=torch.uint8, device="cuda:0")
        coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        fwd.roundtrip_u8(inv, d_in.data_ptr(), d_out.data_ptr(), None, mul, filter=filt, d_coded=coded.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        want[..., c] = d_out.cpu().numpy()
        counts.append(int(coded.item()))
    return want, counts


def both(torch, block, scaled, comps, name, pdc=2, fmt=None, boost=None, trc=None, plans=None):
    """the packed call and the planar calls of one setting on the volume layout: (got, coded, want, counts)"""
    fwd, inv, info = plans or grid_plans(block, scaled)
    for pl, t in zip((fwd, inv), trc or ()):
        pl.set_u8_trc(t)
    src = clip_of(block, comps)
    filt, packed, planes = settings(block, scaled, comps, info, name, fmt=fmt, boost=boost, pdc=pdc)
    out_shape = tuple(info["out_shape"]) + (comps,)
    got, coded = run_packed(torch, fwd, inv, src, out_shape, info["out_mul"], packed, filt)
    want, counts = run_planes(torch, fwd, inv, src, out_shape, info["out_mul"], planes)
    return got, coded, want, counts


# ((4, 16, 16) -> (16, 16, 4), whose embedding is 16 x 16 x 16, at two and three components)
CASES = [(p, c) for p in gr.PAIRS for c in ((2, 3) if p == gr.PAIRS[4] else (3, 4))]


@pytest.mark.parametrize("name", ["none", "quant", "dc", "grey"])
@pytest.mark.parametrize("pair,comps", CASES, ids=[gr.pair_id(p) + f"-c{c}" for p, c in CASES])
def test_packed_grid_call_equals_the_planar_grid_call_on_every_component(gpu, pair, comps, name):
    """no filter; --quant alone; a band with per-component damp and boost, --threshold and preserve_dc = dc / grey through motion_packed"""
    block, scaled = pair
    got, coded, want, counts = both(gpu, block, scaled, comps, "full" if name in ("dc", "grey") else name, pdc=1 if name == "dc" else 2)
    assert np.array_equal(got, want), int((got != want).sum())
    assert coded == sum(counts) and (name == "none") == (coded == 0), (coded, counts)
    if name in ("dc", "grey"):
        assert len(set(counts)) > 1          # the components were filtered differently


def test_bgr24_takes_the_components_values_to_bytes_2_1_0(gpu):
    block, scaled = gr.PAIRS[0]
    boost = [2.0, 1.0, 0.5]
    fwd, inv, info = grid_plans(block, scaled)
    _, _, planes = settings(block, scaled, 3, info, "full", fmt="bgr24", boost=boost)
    assert [planes[at]["boost"] for at in (2, 1, 0)] == boost
    got, coded, want, counts = both(gpu, block, scaled, 3, "full", fmt="bgr24", boost=boost)
    assert np.array_equal(got, want) and coded == sum(counts) > 0
    rgb, _, _, _ = both(gpu, block, scaled, 3, "full", fmt="rgb24", boost=boost)
    assert not np.array_equal(rgb, got)


def to_stack(v, ext):
    """[D][H][W][C] -> block-major [blocks][d][h][w][C]"""
    d, h, w = ext
    D, H, W, c = v.shape
    return np.ascontiguousarray(v.reshape(D // d, d, H // h, h, W // w, w, c).transpose(0, 2, 4, 1, 3, 5, 6)).reshape(-1, d, h, w, c)


@pytest.mark.parametrize("pair", [gr.PAIRS[0], gr.PAIRS[5]], ids=[IDS[0], IDS[5]])
def test_block_major_stacks_give_the_volume_layouts_bytes(gpu, pair):
    from test_motion_block_rescale_gpu import stack_plans
    block, scaled = pair
    vol, cv, _, _ = both(gpu, block, scaled, 3, "full")
    _, _, info = grid_plans(block, scaled)
    fwd, inv = stack_plans(block, scaled)
    assert "block-major" in fwd.describe() and "block-major" in inv.describe()
    filt, packed, _ = settings(block, scaled, 3, info, "full")
    nb = int(np.prod(gr.NBLOCKS))
    got, coded = run_packed(gpu, fwd, inv, to_stack(clip_of(block, 3), block), (nb,) + tuple(scaled) + (3,), info["out_mul"], packed, filt)
    back = np.stack([gr.from_blocks(np.ascontiguousarray(got[..., c]), scaled) for c in range(3)], axis=-1)
    assert np.array_equal(back, vol), int((back != vol).sum())
    assert coded == cv > 0


def test_a_short_last_group(gpu, monkeypatch):
    """nine blocks along x in groups of 2, 2, 2, 2, 1: the same bytes as with the rule's group"""
    block, scaled = gr.PAIRS[0]
    plain, coded, _, _ = both(gpu, block, scaled, 3, "full")
    monkeypatch.setenv("DSPFFT_PACKED_G", "2")
    got, coded2, _, _ = both(gpu, block, scaled, 3, "full")
    assert np.array_equal(got, plain) and coded2 == coded > 0


@pytest.mark.parametrize("pair", [gr.PAIRS[0], gr.PAIRS[5]], ids=[IDS[0], IDS[5]])
def test_transfer_characteristic(gpu, pair):
    block, scaled = pair
    trc = "iec61966-2-1"
    got, coded, want, counts = both(gpu, block, scaled, 3, "full", trc=(trc, trc))
    assert np.array_equal(got, want), int((got != want).sum())
    assert coded == sum(counts) > 0
    # one end only: the other converts plainly
    got1, _, want1, _ = both(gpu, block, scaled, 3, "full", trc=(trc, 0))
    assert np.array_equal(got1, want1) and not np.array_equal(want1, want)
    got2, _, want2, _ = both(gpu, block, scaled, 3, "full", trc=(0, trc))
    assert np.array_equal(got2, want2) and not np.array_equal(want2, want) and not np.array_equal(want2, want1)


def test_refusals_write_nothing(gpu):
    torch = gpu
    from dspfun_amd import Plan, DspfftError
    from dspfun_amd.engine import motion_grid_plans, motion_packed
    block, scaled = gr.PAIRS[0]
    fwd, inv, info = grid_plans(block, scaled)
    p3 = motion_packed("rgb24")
    src = torch.from_numpy(np.array(clip_of((16, 16, 16), 4))).to("cuda:0").reshape(-1)          # as large as any clip asked for below
    buf, out = framed(torch, src.numel())

    def refused(f, i, reason, packed=p3, filt=None, d_out=None):
        with pytest.raises(DspfftError, match=reason):
            f.roundtrip_u8_packed_rescale(i, src.data_ptr(), d_out or out.data_ptr(), info["out_mul"], packed, filter=filt, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((buf == MARK).all())

    fe, ie, _ = motion_grid_plans(gr.shapes(block, block)[0], block, block)
    refused(fe, ie, "equal extents.*dspfft_execute_roundtrip_u8_packed")
    f2 = Plan.many_r2r([12, 20], [5, 5], howmany=4, idist=240, odist=240)
    i2 = Plan.many_r2r([6, 10], [4, 4], howmany=4, idist=60, odist=60, first_axis_first=True)
    refused(f2, i2, "dspfft_execute_roundtrip_u8_packed_frames")
    for comps in (1, 5):
        pc = motion_packed("rgb24")
        pc.components = comps
        refused(fwd, inv, f"components must be 2, 3 or 4 bytes per pixel, got {comps}", packed=pc)
    b16, s16 = (16, 16, 16), (4, 4, 16)          # a 16 x 16 x 16 embedding with 16 active columns: four component tiles are 64 KB
    f16, i16, _ = grid_plans(b16, s16)
    refused(f16, i16, "64 KB of LDS", packed=motion_packed("rgba"))
    refused(fwd, inv, "overlap", d_out=src.data_ptr())
    f64 = Plan.many_r2r([8, 8, 8], [5] * 3, howmany=4, idist=512, odist=512, dtype="f64")
    refused(f64, inv, "f32 plans")
    bad = dict(active=info["active"], minbuf_hw=(8, 8), block_depth=8, band_begin=(0, 0, 0), band_end=info["active"], preserve_dc=5)
    refused(fwd, inv, "bad filter parameters", filt=bad)


ORACLE_PAIRS = [gr.PAIRS[0], gr.PAIRS[1], gr.PAIRS[6]]


@pytest.mark.parametrize("quant", [0.0, 0.4], ids=["plain", "quant"])
@pytest.mark.parametrize("pair", ORACLE_PAIRS, ids=[gr.pair_id(p) for p in ORACLE_PAIRS])
def test_rgb24_against_the_f64_oracle(gpu, pair, quant):
    """component c's plane is the grid oracle's volume from seed 100 + 37 c on.  test_motion_block_rescale_gpu.py's caps: at most 1 LSB
    anywhere; fewer than 0.5 % of the bytes differ without a quantiser, fewer than 2 % with quant = 0.4, and then -- the seeds keep every
    coefficient / quantizer more than EDGE from a rounding boundary -- d_coeffs_coded is the oracle's count of non-zero quanta exactly.  The
    header's phases meet the same caps on the same seeds on the CPU (test_motion_packed_rescale_cpu.py)."""
    from dspfun_amd.engine import motion_packed
    block, scaled = pair
    refs = [gr.case(block, scaled, quant, seed0=100 + 37 * c) for c in range(3)]
    src = np.ascontiguousarray(np.stack([r["vol"] for r in refs], axis=-1))
    fwd, inv, info = grid_plans(block, scaled)
    filt = None
    if quant:
        assert all(r["edge"] > gr.EDGE for r in refs)
        minbuf = [max(b, s) for b, s in zip(block, scaled)]
        filt = dict(active=info["active"], minbuf_hw=minbuf[1:], block_depth=minbuf[0], band_begin=(0, 0, 0), band_end=info["active"],
                    quantizer=gr.quantizer_of(quant, scaled))
    got, coded = run_packed(gpu, fwd, inv, src, tuple(info["out_shape"]) + (3,), info["out_mul"], motion_packed("rgb24"), filt)
    for c, ref in enumerate(refs):
        diff = np.abs(got[..., c].astype(int) - ref["out8"].astype(int))
        print(f"{gr.pair_id(pair)} component {c}: max {diff.max()} LSB, {(diff > 0).mean():.5f} of the bytes differ, seed {ref['seed']}")
        assert diff.max() <= 1 and (diff > 0).mean() < (0.02 if quant else 0.005), (c, diff.max(), (diff > 0).mean())
    if quant:
        assert coded == sum(r["nonzero"] for r in refs) > 0
