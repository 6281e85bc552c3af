"""motion --spectrogram / --ispectrogram on packed 8-bit pixels on the device (dspfft_execute_spectrogram_u8_packed,
dspfft_execute_ispectrogram_u8_packed, dspfft_motion_spec_blocks_u8_packed, dspfft_motion_ispec_blocks_u8_packed).
  small blocks   one kernel (block_spec_packed.hip) whose component blocks run the planar kernel's inlined phases: the bytes equal
                 Plan.spectrogram / Plan.ispectrogram of the same plan on every de-interleaved component with that component's damp / boost /
                 grey_add, and d_coeffs_coded the sum of the planar counts.  No tolerance.
  full frames    the call equals, byte for byte, the composition dspfft_u8_to_f32 -> dspfft_execute -> the stand-alone packed kernel (and the
                 mirror); the stand-alone kernels equal the planar ones on the de-interleaved coefficient planes; and the call is held against
                 the float64 reference (tests/motion_spec_ref.py) per component by the rule of tests/test_motion_spec_gpu.py.
Every packed output goes into a buffer with a marker page on each side."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import oracle_lib as ol
import motion_spec_ref as sr

pytestmark = pytest.mark.gpu
FMT_OF = {2: "ya8", 3: "rgb24", 4: "rgba"}
PAGE, MARK = 4096, 0xA5
SPEC_MODES, ISPEC_MODES = ("abs", "shift", "flat", "copy"), ("shift", "flat", "copy")


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from dspfun_amd import _lib
    _lib.load()
    return torch


def packed_G(block, comps, nxb=1 << 20):
    """packed_group_of (block_packed_core.h) and rt_lds_group: the pixel blocks per workgroup of the packed kernels"""
    bd, bh, bw = block
    e, lines = bw * bh * bd * comps, bh * bd
    G = 6144 // e
    G = max(G, min(-(-128 // lines), 8192 // e))
    per = 256 // lines
    if per > 0 and G > per:
        G -= G % per
    G = max(1, min(G, nxb))
    while G and G * e * 4 + 3072 + 16 > 65536:          # (rt_lds_group: room for the tables of motion --linear, 3072 bytes, and the counter)
        G -= 1
    return G


def next_prime(n):
    p = n + 1
    while any(p % q == 0 for q in range(2, int(p ** 0.5) + 1)):
        p += 1
    return p


def volume_of(block, comps):
    """2 x 2 x P blocks, P the smallest prime above the packed group size: the last group of a row of blocks is short"""
    bd, bh, bw = block
    return (2 * bd, 2 * bh, next_prime(packed_G(block, comps)) * bw)


@functools.lru_cache(maxsize=None)
def clip_of(shape, comps, seed=0x5BAC):
    a = ol.synth_u8(seed + comps + 16 * shape[0] + shape[2], int(np.prod(shape)) * comps).reshape(tuple(shape) + (comps,))
    a.setflags(write=False)
    return a


def settings(block, comps, k, name, fmt=None, pdc=2):
    """(filter dict for the packed call, dspfft_motion_packed, per-byte planar filter dicts)"""
    from dspfun_amd.engine import motion_packed, PACKED_FORMATS
    fmt = fmt or FMT_OF[comps]
    bd, bh, bw = block
    base = dict(active=block, minbuf_hw=(bh, bw), block_depth=bd, band_begin=(0, 0, 0), band_end=block)
    if name == "none":
        return None, motion_packed(fmt), [None] * comps
    q = float(np.float32(sr.gr.quantizer_of(sr.QUANT, block)))
    if name == "quant":
        f = dict(base, quantizer=q)
        # (-D's default of 0 never acts: the band is the whole block)
        return dict(f, damp=99.0, boost=99.0), motion_packed(fmt), [dict(f, damp=0.0, boost=1.0) for _ in range(comps)]
    boost, damp = [2.0, 1.0, 0.5, 1.5][:comps], [0.25, 0.5, 0.0, 0.75][:comps]
    f = dict(base, band_begin=(1 if bd > 1 else 0, 0, 1), band_end=(max(1, bd // 2), bh // 2 + 1, bw // 2 + 1), threshold_lo=q / 8, threshold_hi=1e30,
             preserve_dc=pdc, quantizer=q)
    p = motion_packed(fmt, boost=boost, damp=damp, dcstop=True, normalization=k["normalization"], scalefactor=k["scalefactor"])
    planes = [dict(f, damp=p.damp[at], boost=p.boost[at], grey_add=p.grey_add[at]) for at in range(comps)]
    for i, at in enumerate(PACKED_FORMATS[fmt]):
        assert planes[at]["boost"] == np.float32(boost[i]) and planes[at]["damp"] == np.float32(damp[i])
    return dict(f, damp=99.0, boost=99.0, grey_add=99.0), p, planes


def framed(torch, n, offset=0):
    """n output bytes with a marker page on each side (offset: bytes off the page's alignment)"""
    buf = torch.full((n + 2 * PAGE + offset,), MARK, dtype=torch.uint8, device="cuda:0")
    return buf, buf[PAGE + offset:PAGE + offset + n]


def check_frame(buf, n, offset=0):
    b = buf.cpu().numpy()
    assert (b[:PAGE + offset] == MARK).all() and (b[PAGE + offset + n:] == MARK).all(), "the call wrote outside the clip"


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def run_packed(torch, plan, inverse, src, mode, k, packed, filt=None, work=False, in_place=False, offset=0):
    """one packed call on the interleaved clip src (numpy, any shape ending in the components).  Returns (bytes, coded)."""
    n = src.size
    buf, out = framed(torch, n, offset)
    if offset:          # (the input shares the output's misalignment)
        _, d_in = framed(torch, n, offset)
        d_in.copy_(torch.from_numpy(np.ascontiguousarray(src)).reshape(-1))
    else:
        d_in = torch.from_numpy(np.ascontiguousarray(src)).to("cuda:0").reshape(-1)
    if in_place:
        out.copy_(d_in)
        d_in = out
    wk = torch.empty(n, dtype=torch.float32, device="cuda:0") if work else None
    coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    run = plan.ispectrogram_packed if inverse else plan.spectrogram_packed
    run(d_in.data_ptr(), out.data_ptr(), mode, k["scalefactor"], k["normalization"], packed, c=k["c"], d_work=wk.data_ptr() if work else 0,
        filter=filt, d_coded=coded.data_ptr(), stream=stream_of(torch))
    torch.cuda.synchronize()
    check_frame(buf, n, offset)
    return out.cpu().numpy().reshape(src.shape), int(coded.item())


def run_planes(torch, plan, inverse, src, mode, k, planes, work=False):
    """the planar call of the same plan (or of `plan`, a planar twin) on every de-interleaved component.  Returns (interleaved bytes, [coded])."""
    want = np.empty_like(src)
    counts = []
    for c, filt in enumerate(planes):
        d_in = torch.from_numpy(np.ascontiguousarray(src[..., c])).to("cuda:0")
        d_out = torch.empty_like(d_in)
        wk = torch.empty(d_in.numel(), dtype=torch.float32, device="cuda:0") if work else None
        coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        run = plan.ispectrogram if inverse else plan.spectrogram
        run(d_in.data_ptr(), d_out.data_ptr(), mode, k["scalefactor"], k["normalization"], k["c"], d_work=wk.data_ptr() if work else 0, filter=filt,
            d_coded=coded.data_ptr(), stream=stream_of(torch))
        torch.cuda.synchronize()
        want[..., c] = d_out.cpu().numpy()
        counts.append(int(coded.item()))
    return want, counts


# ---- 1. small blocks: exact ----
BLOCKS = [(1, 4, 4), (1, 8, 8), (8, 8, 8), (4, 8, 16), (1, 32, 32)]
CASES = [(b, c) for b in BLOCKS for c in (2, 3, 4)] + [((16, 16, 16), 2), ((16, 16, 16), 3)]
VARIANTS = [("none", None, 2), ("quant", None, 2), ("full", None, 1), ("full", "permuted", 2)]


@pytest.mark.parametrize("block,comps", CASES, ids=["x".join(map(str, b)) + f"-c{c}" for b, c in CASES])
def test_small_blocks_equal_the_planar_calls_on_every_component(gpu, block, comps):
    """every spectrogram and ispectrogram mode; no filter, the quantiser alone, and a band off the origin with per-component damp / boost /
    grey_add, a threshold and preserve_dc = dc and grey, the latter with permuted byte positions (bgr24 / argb)"""
    from dspfun_amd.engine import motion_spec_constants
    shape = volume_of(block, comps)
    src = clip_of(shape, comps)
    k = motion_spec_constants(block)
    G = packed_G(block, comps)
    assert G == 1 or (shape[2] // block[2]) % G, "the last group of a row must be short"
    for inverse in (False, True):
        plan = sr.volume_plan(block, shape, sr.ol.REDFT01 if inverse else sr.ol.REDFT10)
        assert "BLOCK" in plan.describe() and "side by side" in plan.describe()
        for mode in (ISPEC_MODES if inverse else SPEC_MODES):
            # (the inverse reads a spectrogram of the clip in its own mode, so that its output is an image and not a saturated plane)
            pix = run_packed(gpu, sr.volume_plan(block, shape, sr.ol.REDFT10), False, src, mode, k, settings(block, comps, k, "none")[1])[0] if inverse else src
            for name, fmt, pdc in VARIANTS:
                fmt = {2: "ya8", 3: "bgr24", 4: "argb"}[comps] if fmt else None
                filt, packed, planes = settings(block, comps, k, name, fmt=fmt, pdc=pdc)
                got, coded = run_packed(gpu, plan, inverse, pix, mode, k, packed, filt)
                want, counts = run_planes(gpu, plan, inverse, pix, mode, k, planes)
                what = (inverse, mode, name, fmt)
                assert np.array_equal(got, want), (what, int((got != want).sum()))
                assert coded == sum(counts) and (name == "none") == (coded == 0), (what, coded, counts)
                if name == "full" and not inverse:
                    assert len(set(counts)) > 1, (what, counts)          # the components were filtered differently
            assert len(np.unique(got)) > 2, (inverse, mode)


def test_small_blocks_in_place_and_as_a_block_major_stack(gpu):
    from dspfun_amd.engine import motion_spec_constants
    block, comps, nb = (8, 8, 8), 3, 45
    k = motion_spec_constants(block)
    shape = volume_of(block, comps)
    src = clip_of(shape, comps)
    filt, packed, planes = settings(block, comps, k, "full", pdc=1)
    for inverse, mode in ((False, "abs"), (True, "shift")):
        kind = sr.ol.REDFT01 if inverse else sr.ol.REDFT10
        plan = sr.volume_plan(block, shape, kind)
        plain = run_packed(gpu, plan, inverse, src, mode, k, packed, filt)
        same = run_packed(gpu, plan, inverse, src, mode, k, packed, filt, in_place=True)
        assert np.array_equal(same[0], plain[0]) and same[1] == plain[1]
        # a stack of 45 blocks of [8][8][8][3] bytes: rows_fast's order of lines, and 45 is no multiple of the four blocks of a workgroup
        stack = sr.stack_plan(block, nb, kind)
        assert "block-major" in stack.describe() and nb % packed_G(block, comps, nb)
        blocks = clip_of((nb * 8, 8, 8), comps).reshape(nb, 8, 8, 8, comps)
        got, coded = run_packed(gpu, stack, inverse, blocks, mode, k, packed, filt)
        want, counts = run_planes(gpu, stack, inverse, blocks, mode, k, planes)
        assert np.array_equal(got, want), int((got != want).sum())
        assert coded == sum(counts) > 0


# ---- 2. full frames: exact against the composition ----
def frame_filters(h, w, comps, info, fmt=None):
    return settings((1, h, w), comps, info, "full", fmt=fmt, pdc=2)


def composition(torch, L, plan, inverse, src, mode, info, packed, filt, h, w):
    """dspfft_u8_to_f32 -> dspfft_execute -> dspfft_motion_spec_blocks_u8_packed, or dspfft_motion_ispec_blocks_u8_packed -> dspfft_execute ->
    dspfft_f32_to_u8.  Returns (bytes, coded, the coefficients the stand-alone kernel read or wrote)."""
    from dspfun_amd.engine import motion_spec_blocks_packed, motion_ispec_blocks_packed
    F, comps = src.shape[0], src.shape[-1]
    n = src.size
    s = stream_of(torch)
    d_in = torch.from_numpy(np.ascontiguousarray(src)).to("cuda:0").reshape(-1)
    wk = torch.empty(n, dtype=torch.float32, device="cuda:0")
    buf, out = framed(torch, n)
    coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    args = (h, w, comps, F, mode, info["scalefactor"], info["normalization"], packed)
    if not inverse:
        assert L.dspfft_u8_to_f32(wk.data_ptr(), d_in.data_ptr(), n, s) == 0
        plan.execute(wk.data_ptr(), stream=s)
        coeffs = wk.clone()
        motion_spec_blocks_packed(out, wk, *args, c=info["c"], filter=filt, d_coded=coded.data_ptr(), stream=s)
        torch.cuda.synchronize()
        assert torch.equal(wk, coeffs)          # read only
    else:
        motion_ispec_blocks_packed(wk, d_in, *args, c=info["ic"], filter=filt, d_coded=coded.data_ptr(), stream=s)
        coeffs = wk.clone()
        plan.execute(wk.data_ptr(), stream=s)
        assert L.dspfft_f32_to_u8(out.data_ptr(), wk.data_ptr(), info["out_mul"], n, s) == 0
    torch.cuda.synchronize()
    check_frame(buf, n)
    return out.cpu().numpy().reshape(src.shape), int(coded.item()), coeffs.cpu().numpy().reshape(src.shape)


def planar_blocks(torch, inverse, a, mode, info, planes, h, w):
    """motion_spec_blocks / motion_ispec_blocks on every de-interleaved plane of a ([F][h][w][C] coefficients, or pixels).  Returns (the
    interleaved result, [coded])"""
    from dspfun_amd.engine import motion_spec_blocks, motion_ispec_blocks
    F, comps = a.shape[0], a.shape[-1]
    out = np.empty(a.shape, dtype=np.float32 if inverse else np.uint8)
    counts = []
    for c, filt in enumerate(planes):
        src = torch.from_numpy(np.ascontiguousarray(a[..., c])).to("cuda:0")
        dst = torch.zeros(src.numel(), dtype=torch.float32 if inverse else torch.uint8, device="cuda:0")
        coded = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        run = motion_ispec_blocks if inverse else motion_spec_blocks
        run(dst, src, (1, h, w), mode, info["scalefactor"], info["normalization"], info["c"], nblocks=F, filter=filt, d_coded=coded.data_ptr(),
            stream=stream_of(torch))
        torch.cuda.synchronize()
        out[..., c] = dst.cpu().numpy().reshape(F, h, w)
        counts.append(int(coded.item()))
    return out, counts


#: widths with an interleaved 8-bit row end (spec_inst_row_u8c.hip): 256 is the smallest
FRAMES = [(3, 24, 40, 3, 0), (3, 24, 40, 4, 0), (2, 10, 18, 3, 0), (2, 16, 256, 3, 0), (2, 16, 256, 3, 1)]


@pytest.mark.parametrize("F,h,w,comps,offset", FRAMES, ids=[f"{f}x{h}x{w}x{c}" + ("-off1" if o else "") for f, h, w, c, o in FRAMES])
def test_full_frames_equal_their_composition(gpu, F, h, w, comps, offset):
    """every mode each way, the full filter and none: bytes and count of the call equal the composition's; the stand-alone packed kernels
    equal the planar ones on the de-interleaved planes.  10 x 18 x 3: rows of 54 bytes, the scalar path.  16 x 256 x 3: the first (last)
    pass is the interleaved 8-bit row kernel, unless the bytes start 1 off a multiple of 4 -- then dspfft_u8_to_f32 / _f32_to_u8 sweep."""
    from dspfun_amd import _lib
    from dspfun_amd.engine import motion_packed_frame_plans
    L = _lib.load()
    fwd, inv, info = motion_packed_frame_plans(F, h, w, comps)
    if w == 256:
        row = lambda plan: [l for l in plan.describe().splitlines() if l.startswith("axis 1")]
        assert all("ROW*" in l and "C=3" in l for l in row(fwd) + row(inv)) and row(fwd) and row(inv), (fwd.describe(), inv.describe())
    src = clip_of((F, h, w), comps)
    for inverse, plan in ((False, fwd), (True, inv)):
        for mode in (ISPEC_MODES if inverse else SPEC_MODES):
            pix = run_packed(gpu, fwd, False, src, mode, info, settings((1, h, w), comps, info, "none")[1], work=True)[0] if inverse else src
            for name in ("none", "full"):
                filt, packed, planes = settings((1, h, w), comps, info, name, fmt="bgr24" if comps == 3 and name == "full" else None)
                got, coded = run_packed(gpu, plan, inverse, pix, mode, info, packed, filt, work=True, offset=offset)
                want, wcoded, coeffs = composition(gpu, L, plan, inverse, pix, mode, info, packed, filt, h, w)
                what = (inverse, mode, name)
                assert np.array_equal(got, want), (what, int((got != want).sum()))
                assert coded == wcoded and (name == "none") == (coded == 0), (what, coded, wcoded)
                if offset:
                    continue
                # the stand-alone kernel against the planar one: spec reads `coeffs` and wrote `want`; ispec read `pix` and wrote `coeffs`
                alone, counts = planar_blocks(gpu, inverse, pix if inverse else coeffs, mode, info, planes, h, w)
                mine = coeffs if inverse else want
                assert np.array_equal(alone.view(np.uint32) if inverse else alone, mine.view(np.uint32) if inverse else mine), what
                assert sum(counts) == wcoded, (what, counts, wcoded)
            got_ip, coded_ip = run_packed(gpu, plan, inverse, pix, mode, info, packed, filt, work=True, in_place=True, offset=offset)
            assert np.array_equal(got_ip, got) and coded_ip == coded


# ---- 3. full frames against the reference's arithmetic ----
# Share of bytes that differ from the float64 reference for the PLANAR Plan.spectrogram / Plan.ispectrogram calls on the component planes of
# the clip below (worst filter case per mode): tools/bench_motion_spec_packed.py --accuracy on the kernels of commit 4eee687, the parent of the
# commit that added this file, which leaves the planar calls as they were (profiles/r18_motion_spec_packed.txt).
PLANAR_SHARE = {
    "spec": {"abs": 0.0, "shift": 0.0, "flat": 0.0, "copy": 0.0},
    "ispec": {"shift": 1.15741e-4, "flat": 1.15741e-4, "copy": 0.0},
}
EXTRA_BYTES = 4
REF_BLOCK, REF_FRAMES, REF_SEEDS = (1, 24, 40), 3, (300, 301, 302)


@functools.lru_cache(maxsize=None)
def ref_case(inverse, mode, kind):
    """per component: the float64 reference of a 3 x 24 x 40 plane (motion_spec_ref.spec_grid / ispec_grid, every frame a block); the inverse
    reads the reference's own spectrogram of the plane.  Returns (the interleaved rgb24 clip, [reference per component])."""
    shape = (REF_FRAMES,) + REF_BLOCK[1:]
    filt = sr.filter_kind(kind, REF_BLOCK)
    planes, refs = [], []
    for seed in REF_SEEDS:
        vol = sr.volume(REF_BLOCK, shape, seed)
        if inverse:
            pix = sr.spec_grid(vol, REF_BLOCK, mode)["out8"]
            r = sr.ispec_grid(pix, REF_BLOCK, mode, filt)
        else:
            pix, r = vol, sr.spec_grid(vol, REF_BLOCK, mode, filt)
        r["filt"] = filt
        planes.append(pix)
        refs.append(r)
    return np.ascontiguousarray(np.stack(planes, axis=-1)), refs


def packed_of(filt, comps=3):
    from dspfun_amd import _lib
    p = _lib.MotionPacked()
    p.components = comps
    for c in range(comps):
        p.damp[c], p.boost[c], p.grey_add[c] = (filt.get("damp", 1.0), filt.get("boost", 1.0), filt.get("grey_add", 0.0)) if filt else (1.0, 1.0, 0.0)
    return p


@pytest.mark.parametrize("inverse,mode", [(False, m) for m in SPEC_MODES] + [(True, m) for m in ISPEC_MODES], ids=lambda v: {False: "spec", True: "ispec"}.get(v, v))
def test_full_frames_against_the_float64_reference(gpu, inverse, mode):
    """no byte differs by more than 1; the share that differs is at most 1.5 times the planar calls' on the same planes, plus 4 bytes (the
    interleaved row and column kernels round in the last place differently from the planar ones, and a byte moves only where a value sits at
    a rounding boundary); the coded count is the reference's to within the coefficients on a quantiser tie"""
    from dspfun_amd.engine import motion_packed_frame_plans
    h, w = REF_BLOCK[1:]
    fwd, inv, info = motion_packed_frame_plans(REF_FRAMES, h, w, 3)
    sf, nm, c = sr.constants(REF_BLOCK)
    assert (sf, nm, c) == (info["scalefactor"], info["normalization"], info["c"])
    for kind in (None, "band", "full", "q"):
        clip, refs = ref_case(inverse, mode, kind)
        filt = refs[0]["filt"]
        got, coded = run_packed(gpu, inv if inverse else fwd, inverse, clip, mode, info, packed_of(filt), filt, work=True)
        diff = size = 0
        for k, ref in enumerate(refs):
            sr.check_tie_share(ref, inverse)
            mx, n, sz = sr.share_of(got[..., k], ref["out8"], ref["tie"])
            assert mx <= 1, (kind, k, mx)
            diff, size = diff + n, size + sz
        cap = 1.5 * PLANAR_SHARE["ispec" if inverse else "spec"][mode] * size + EXTRA_BYTES
        print(f"{'ispec' if inverse else 'spec'} {mode} filter={kind}: {diff} of {size} bytes differ ({diff / max(size, 1):.5%}), cap {cap:.1f} bytes")
        assert diff <= cap, (kind, diff, size, cap)
        if kind in ("full", "q"):
            want = sum(r["coded"] for r in refs)
            slack = sum(sr.coded_slack(r, REF_BLOCK) for r in refs)
            print(f"  coded {coded}, reference {want}, on a quantiser tie: {slack}")
            assert coded > 0 and abs(coded - want) <= slack, (kind, coded, want, slack)


# ---- 4. refusals on the device library: nothing is written between the marker pages ----
def test_refusals_write_nothing(gpu):
    from dspfun_amd.engine import DspfftError, Plan, motion_spec_constants, motion_packed_frame_plans, motion_packed
    torch = gpu
    block = (8, 8, 8)
    shape = volume_of(block, 3)
    k = motion_spec_constants(block)
    n4 = int(np.prod(shape)) * 4
    src = torch.full((n4 + 16,), 77, dtype=torch.uint8, device="cuda:0")
    wk = torch.zeros(n4, dtype=torch.float32, device="cuda:0")
    ff, fi, finfo = motion_packed_frame_plans(2, 12, 20, 3)
    b16 = (16, 16, 16)

    def refused(plan, inverse, mode, comps, match, kk=k, d_in=None, off=0, work=False):
        buf, out = framed(torch, n4, off)
        p = motion_packed(FMT_OF[comps]) if comps in FMT_OF else motion_packed("rgb24")
        p.components = comps
        run = plan.ispectrogram_packed if inverse else plan.spectrogram_packed
        with pytest.raises(DspfftError, match=match):
            run((d_in if d_in is not None else src).data_ptr(), out.data_ptr(), mode, kk["scalefactor"], kk["normalization"], p, c=kk["c"],
                d_work=wk.data_ptr() if work else 0, stream=stream_of(torch))
        torch.cuda.synchronize()
        assert bool((buf == MARK).all()), match
    for inverse in (False, True):
        kind = sr.ol.REDFT01 if inverse else sr.ol.REDFT10
        small = sr.volume_plan(block, shape, kind)
        frames = fi if inverse else ff
        for comps in (1, 5):
            refused(small, inverse, "shift", comps, "components must be 2, 3 or 4")
        refused(Plan.many_r2r([8, 8, 8], [kind] * 3, howmany=4, idist=512, odist=512, dtype="f64"), inverse, "shift", 3, "f64 plans")
        refused(sr.volume_plan(block, shape, kind).set_u8_trc("iec61966-2-1"), inverse, "shift", 3, "transfer characteristic")
        refused(small, inverse, "shift", 3, "4-byte aligned", off=2)
        refused(small, inverse, "shift", 3, "4-byte aligned", d_in=src[2:])
        refused(sr.volume_plan(b16, volume_of(b16, 3), kind), inverse, "shift", 4, "64 KB of LDS", kk=motion_spec_constants(b16))
        refused(frames, inverse, "shift", 4, "unit-stride batch level counts 3", kk=finfo, work=True)
        refused(Plan.guru([(12, 66, 66), (20, 3, 3)], [(3, 1, 1), (2, 12 * 66, 12 * 66)], [kind] * 2), inverse, "shift", 3, "dense in-place layout", kk=finfo, work=True)
        refused(Plan.guru([(6, 720, 720), (12, 60, 60), (20, 3, 3)], [(3, 1, 1)], [kind] * 3), inverse, "shift", 3, "one 3-D block", kk=finfo, work=True)
    refused(sr.volume_plan(block, shape, sr.ol.REDFT01), True, "abs", 3, "no abs type")
    refused(fi, True, "abs", 3, "no abs type", kk=finfo, work=True)
